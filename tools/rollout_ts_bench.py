"""ms per launch of the trajectory-sampling rollout (mbrl_rollout_cost_ts) and per plan of mbrl_cem_plan_ts at
I = 5 on cheetah-shaped probabilistic members (s = 17, a = 6, 2 x 512 and 3 x 512, N = 4096, H = 30, E = 5,
P = 1 and 4), beside -- in the same run, every variant of a shape interleaved -- the deterministic
mbrl_rollout_cost / mbrl_cem_plan on the mean ensemble (E rows) and a torch restatement of the same sampled
rollout on the GPU (batched matmuls over the Q rows, torch.randn for the noise). Events around `launches`
back-to-back calls, `repeats` samples of each: medians with quartiles, row-candidate-timesteps per second and
the fraction of the fp32 MFMA peak of the MLP's algorithmic FLOP (profiles/rollout_ts/README.md).

    python tools/rollout_ts_bench.py [--out file.json] [--repeats 9] [--launches 20]"""
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

from mbrl_amd import _lib, data, fused, models  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--candidates", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=30)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rollout_ts_bench: no GPU (a time measured anywhere else says nothing)")
dev = torch.device("cuda:0")
lib = _lib.load()
P = _lib.ptr
stream = _lib.stream_handle(dev)
S, A, W, E, N, H, I = 17, 6, 512, 5, args.candidates, args.horizon, 5
K = max(1, N // 10)


def time_ms(go, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        go()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def interleaved(tag, runs, counts, res):
    """runs: name -> callable; counts: name -> (rows, FLOP per call) for the rates."""
    for go in runs.values():
        for _ in range(3):
            go()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, go in runs.items():
            samples[k].append(time_ms(go, args.launches))
    for k, v in samples.items():
        q1, med, q3 = (float(x) for x in np.percentile(np.array(v), [25, 50, 75]))
        row = dict(median_ms=med, q1_ms=q1, q3_ms=q3)
        if k in counts:
            rows, flop = counts[k]
            row.update(rows=rows, row_candidate_steps_per_s=rows * N * H / (med * 1e-3),
                       us_per_row=1e3 * med / rows, mlp_tflops=flop / (med * 1e-3) / 1e12,
                       frac_of_fp32_mfma_peak=flop / (med * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS)
        res[f"{tag} {k}"] = row
        print(f"{tag} {k:22s}: median {med:.4f} ms  quartiles {q1:.4f} .. {q3:.4f}"
              + (f"  {row['row_candidate_steps_per_s']:.3e} row-cand-steps/s  {row['frac_of_fp32_mfma_peak']:.3f} of peak"
                 if k in counts else ""), flush=True)


def torch_rollout(ens, norm, cost, s0, actions, parts, scale):
    """The sampled rollout in torch on the GPU: the members' layers as batched matmuls over the Q rows."""
    Q = E * parts
    lins = [m.linears() for m in ens.members]
    ws = [torch.stack([l[i].weight for l in lins]).repeat_interleave(parts, 0).transpose(1, 2).contiguous()
          for i in range(len(lins[0]))]
    bs = [torch.stack([l[i].bias for l in lins]).repeat_interleave(parts, 0).unsqueeze(1) for i in range(len(lins[0]))]
    lo, hi = ens.members[0].min_logvar, ens.members[0].max_logvar
    om, os_, am, as_ = norm
    cw, goal, al_s, al_a = cost
    na = (actions - am) / as_

    @torch.no_grad()
    def go():
        st = s0.expand(Q, N, S)
        total = torch.zeros((Q, N), device=dev)
        for t in range(H):
            x = torch.cat([(st - om) / os_, na[t].expand(Q, N, A)], dim=2)
            for w, b in zip(ws[:-1], bs[:-1]):
                x = torch.relu(torch.baddbmm(b, x, w))
            out = torch.baddbmm(bs[-1], x, ws[-1])
            lv = models.bounded_logvar(out[..., S:], lo, hi)
            z = out[..., :S] + torch.exp(0.5 * lv) * scale * torch.randn((Q, N, S), device=dev)
            st = z * os_ + om
            d = (st - goal) * cw
            total += (torch.sqrt(d * d + al_s * al_s) - al_s).sum(-1) \
                + al_a * al_a * (torch.cosh(actions[t] / al_a) - 1).mean(-1)
        return total
    return go


res = dict(shape=dict(s=S, a=A, W=W, E=E, N=N, H=H, K=K, I=I), peak_tflops=PEAK_FP32_MFMA_TFLOPS,
           launches_per_sample=args.launches, repeats=args.repeats)
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
    flop_det = 2.0 * (W * (S + A) + (L - 1) * W * W + W * S) * N * H          # per row
    flop_ts = 2.0 * (W * (S + A) + (L - 1) * W * W + W * 2 * S) * N * H
    runs, counts = {}, {}
    det_costs = torch.empty((E, N), device=dev)

    def det():
        rc = lib.mbrl_rollout_cost(*prob.refs, P(s0), 0, P(actions), None, N, H, 0, P(det_costs), None, None, stream)
        assert rc == 0, rc
    runs["mean_rollout_cost"], counts["mean_rollout_cost"] = det, (E, E * flop_det)
    norm_t = [stats[k][f].to(dev) for k in ("observations", "actions") for f in ("mean", "std")]
    for parts in (1, 4):
        Q = E * parts
        costs = torch.empty((Q, N), device=dev)
        tsp = fused.ts_params(parts, 0, 99, 1.0)

        def ts(costs=costs, tsp=tsp):
            rc = lib.mbrl_rollout_cost_ts(table.models, E, ctypes.byref(table.bounds), prob.refs[2], prob.refs[3], P(s0), 0,
                                          P(actions), N, H, 0, ctypes.byref(tsp), P(costs), None, stream)
            assert rc == 0, rc
        runs[f"rollout_cost_ts P={parts}"], counts[f"rollout_cost_ts P={parts}"] = ts, (Q, Q * flop_ts)
        runs[f"torch_restatement P={parts}"] = torch_rollout(ens, norm_t, (torch.ones(S, device=dev), goal.to(dev), 0.4, 0.25),
                                                             s0, actions, parts, 1.0)
        counts[f"torch_restatement P={parts}"] = (Q, Q * flop_ts)
    interleaved(f"{L}x{W} launch", runs, counts, res)

    cem = _lib.CemParams(N, H, K, I, 0.1, -1.0, 1.0, 0.0, 0.5, 0, 1234)
    out = [torch.empty((H, x), device=dev) for x in (A, A, A, S)]
    plans = {}
    need = lib.mbrl_cem_workspace_bytes(prob.refs[0], ctypes.byref(cem))
    ws_det = torch.empty(need, dtype=torch.uint8, device=dev)

    def plan_det():
        rc = lib.mbrl_cem_plan(*prob.refs, P(s0), ctypes.byref(cem), *[P(x) for x in out], None, None, None, None,
                               P(ws_det), ws_det.numel(), stream)
        assert rc == 0, rc
    plans["cem_plan mean"] = plan_det
    for parts in (1, 4):
        tsp = fused.ts_params(parts, 0, 99, 1.0)
        need = lib.mbrl_cem_ts_workspace_bytes(prob.refs[0], ctypes.byref(cem), ctypes.byref(tsp))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def plan_ts(tsp=tsp, ws=ws):
            rc = lib.mbrl_cem_plan_ts(prob.refs[0], prob.refs[1], *table.refs, prob.refs[2], prob.refs[3], P(s0),
                                      ctypes.byref(cem), ctypes.byref(tsp), *[P(x) for x in out], None, None, None, P(ws),
                                      ws.numel(), stream)
            assert rc == 0, rc
        plans[f"cem_plan_ts P={parts}"] = plan_ts
    interleaved(f"{L}x{W} plan I={I}", plans, {}, res)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
