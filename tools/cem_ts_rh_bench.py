"""ms per launch of the sampled rollout by row count (mbrl_rollout_cost_ts_rows: RESAMPLED at Q = 2, 3, 5 beside FIXED
P = 1, five rows) and per plan of mbrl_cem_plan_ts_rh -- cold at I = 5, keep = 0 beside mbrl_cem_plan_ts, warm at
I = 2, keep = 40 in FIXED P = 1 and RESAMPLED Q = 2 -- and of a B = 8 batch (N = 1024, H = 20) beside eight single
calls, on cheetah-shaped probabilistic members (s = 17, a = 6, E = 5, N = 4096, H = 30, 2 x 512 and 3 x 512). Every
variant of a shape interleaved in one run; events around `launches` back-to-back calls, `repeats` samples of each:
medians with quartiles (profiles/cem_ts_rh/README.md).

    python tools/cem_ts_rh_bench.py [--out file.json] [--repeats 9] [--launches 5]"""
import argparse
import ctypes
import functools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mujoco-mbrl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mbrl_amd import _lib, data, fused, models, planners  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--launches", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("cem_ts_rh_bench: no GPU (a time measured anywhere else says nothing)")
dev = torch.device("cuda:0")
lib = _lib.load()
P = _lib.ptr
stream = _lib.stream_handle(dev)
S, A, W, E, N, H = 17, 6, 512, 5, 4096, 30
LO, HI = -1.0, 1.0


def time_ms(go, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        go()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def interleaved(tag, runs, res, rows=None):
    for go in runs.values():
        for _ in range(2):
            go()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, go in runs.items():
            samples[k].append(time_ms(go, args.launches))
    for k, v in samples.items():
        q1, med, q3 = (float(x) for x in np.percentile(np.array(v), [25, 50, 75]))
        row = dict(median_ms=med, q1_ms=q1, q3_ms=q3)
        if rows and k in rows:
            row.update(rows=rows[k], ms_per_row=med / rows[k])
        res[f"{tag} {k}"] = row
        print(f"{tag} {k:28s}: median {med:.4f} ms  quartiles {q1:.4f} .. {q3:.4f}"
              + (f"  {row['ms_per_row']:.4f} ms/row" if "rows" in row else ""), flush=True)


def ts_rows(particles, mode):
    return fused.ts_rows(particles, 0, 99, 1.0, mode)


def rh_plan(prob, table, s0, n, h, k, iters, keep, rows, B=None, mu_rows=None, carry=None, want_carry=False):
    """A closure that enqueues one mbrl_cem_plan_ts_rh (B None) or batch call, and its output tensors."""
    rp = _lib.CemRhParams(_lib.CemParams(n, h, k, iters, 0.1, LO, HI, 0.0, 0.5, 0, 1234), keep, 0)
    nb = 1 if B is None else B
    need = lib.mbrl_cem_ts_rh_workspace_bytes(prob.refs[0], ctypes.byref(rp), ctypes.byref(rows), nb)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    lead = () if B is None else (B,)
    out = [torch.empty((*lead, h, x), device=dev) for x in (A, A, A, S)]
    cout = torch.empty((*lead, keep, h, A), device=dev) if want_carry else None
    head = [prob.refs[0], prob.refs[1], *table.refs, prob.refs[2], prob.refs[3], P(s0)]
    mid = [ctypes.byref(rp), ctypes.byref(rows), P(mu_rows), None, P(carry)]
    tail = [*[P(x) for x in out], P(cout), None, None, None, None, None, P(ws), ws.numel(), stream]

    def go(keepalive=(rp, rows, ws, out, cout, mu_rows, carry)):
        if B is None:
            rc = lib.mbrl_cem_plan_ts_rh(*head, *mid, *tail)
        else:
            rc = lib.mbrl_cem_plan_ts_rh_batch(*head, B, *mid, None, *tail)
        assert rc == 0, (rc, lib.mbrl_last_error())
    return go, out, cout


res = dict(shape=dict(s=S, a=A, W=W, E=E, N=N, H=H), launches_per_sample=args.launches, repeats=args.repeats)
for L in (2, 3):
    torch.manual_seed(L)
    ens = models.EnsembleModel([models.ProbabilisticModel(S, A, hidden_units=W, n_hidden=L, min_logvar=-6.0,
                                                          max_logvar=-1.0) for _ in range(E)]).to(dev)
    g = torch.Generator().manual_seed(7)
    stats = {"observations": {"mean": torch.rand(S, generator=g) - 0.5, "std": torch.rand(S, generator=g) * 1.5 + 0.5},
             "actions": {"mean": torch.rand(A, generator=g) - 0.5, "std": torch.rand(A, generator=g) * 1.5 + 0.5}}
    ds = data.TransitionsDataset.from_statistics(stats)
    goal = torch.randn(S, generator=g)
    model_fn = functools.partial(ens, **ds.normalizers())
    cost_fn = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(S), goal, 0.4), models.CoshLoss(0.25))
    _, _, prob = fused.describe_problem(model_fn, cost_fn, dev, 0)
    assert prob is not None
    table = fused.ts_members(ens, dev)
    s0 = torch.randn(S, generator=g).to(dev)
    actions = (torch.rand((H, N, A), generator=g) * 2 - 1).to(dev)

    # ---- launch time by row count
    runs, nrows = {}, {}
    for name, parts, mode, Q in (("FIXED P=1", 1, "fixed", E), ("RESAMPLED Q=2", 2, "resampled", 2),
                                 ("RESAMPLED Q=3", 3, "resampled", 3), ("RESAMPLED Q=5", 5, "resampled", 5)):
        costs = torch.empty((Q, N), device=dev)
        rows = ts_rows(parts, mode)

        def launch(costs=costs, rows=rows):
            rc = lib.mbrl_rollout_cost_ts_rows(table.models, E, ctypes.byref(table.bounds), prob.refs[2], prob.refs[3],
                                               P(s0), 0, P(actions), N, H, 0, ctypes.byref(rows), P(costs), None, None,
                                               stream)
            assert rc == 0, rc
        runs[name], nrows[name] = launch, Q
    interleaved(f"{L}x{W} launch", runs, res, nrows)
    base = res[f"{L}x{W} launch FIXED P=1"]["ms_per_row"]
    for Q in (2, 3, 5):
        r = res[f"{L}x{W} launch RESAMPLED Q={Q}"]
        r["per_row_ratio_to_fixed"] = r["ms_per_row"] / base

    # ---- plan time, cold and warm
    K, I = N // 10, 5
    cem = _lib.CemParams(N, H, K, I, 0.1, LO, HI, 0.0, 0.5, 0, 1234)
    tsp = fused.ts_params(1, 0, 99, 1.0)
    need = lib.mbrl_cem_ts_workspace_bytes(prob.refs[0], ctypes.byref(cem), ctypes.byref(tsp))
    ws_ts = torch.empty(need, dtype=torch.uint8, device=dev)
    out_ts = [torch.empty((H, x), device=dev) for x in (A, A, A, S)]

    def plan_ts():
        rc = lib.mbrl_cem_plan_ts(prob.refs[0], prob.refs[1], *table.refs, prob.refs[2], prob.refs[3], P(s0),
                                  ctypes.byref(cem), ctypes.byref(tsp), *[P(x) for x in out_ts], None, None, None,
                                  P(ws_ts), ws_ts.numel(), stream)
        assert rc == 0, rc
    plans = {"cem_plan_ts I=5 P=1": plan_ts}
    plans["ts_rh cold I=5 keep=0 FIXED P=1"], _, _ = rh_plan(prob, table, s0, N, H, K, I, 0, ts_rows(1, "fixed"))
    # a cold plan with kept rows gives the next control step's inputs: its actions and carry, shifted by one step
    for name, parts, mode in (("FIXED P=1", 1, "fixed"), ("RESAMPLED Q=2", 2, "resampled")):
        cold, out, cout = rh_plan(prob, table, s0, N, H, K, I, 40, ts_rows(parts, mode), want_carry=True)
        cold()
        torch.cuda.synchronize()
        mu_rows = torch.from_numpy(planners.mppi_warm_start_rows(out[2].cpu(), H, 1, LO, HI)).to(dev)
        carry = torch.from_numpy(planners.cem_shift_carry(cout.cpu(), 1, LO, HI)).to(dev)
        plans[f"ts_rh warm I=2 keep=40 {name}"], _, _ = rh_plan(prob, table, s0, N, H, K, 2, 40, ts_rows(parts, mode),
                                                                mu_rows=mu_rows, carry=carry)
    interleaved(f"{L}x{W} plan", plans, res)

    # ---- a batch of 8 beside 8 single calls
    B, Nb, Hb, Kb = 8, 1024, 20, 102
    s0s = torch.randn((B, S), generator=g).to(dev)
    batch, _, _ = rh_plan(prob, table, s0s, Nb, Hb, Kb, I, 40, ts_rows(1, "fixed"), B=B)
    singles = [rh_plan(prob, table, s0s[b].contiguous(), Nb, Hb, Kb, I, 40, ts_rows(1, "fixed"))[0] for b in range(B)]

    def eight():
        for go in singles:
            go()
    interleaved(f"{L}x{W} batch N={Nb} H={Hb} I={I}", {"B=8 one call": batch, "8 single calls": eight}, res)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
