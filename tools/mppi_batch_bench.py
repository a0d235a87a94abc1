"""ms per batch of B plans of mbrl_mppi_plan_batch against B back-to-back mbrl_mppi_plan calls (the only way to
plan B MPPI problems before the batched entry existed; that entry is unchanged) and against
mbrl_cem_plan_batch (K = 102) at the same shape, for the update's cost per iteration. Cartpole service shape
(N = 1024, H = 20) at B = 8 and 16, I = 1, 2 and 5, classic MPPI and update_sigma; every problem mid-episode
(mean rows for all). Device time from one event pair per call; the variants of one (B, I, update_sigma) are
interleaved call by call, and the quartiles over the calls are reported (profiles/mppi_batch/README.md).

    python tools/mppi_batch_bench.py [--calls 300] [--out file.json]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mujoco-mbrl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mbrl_amd import _lib, fused, synthetic  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=300)
args = ap.parse_args()

N, H, K = 1024, 20, 102
pr = synthetic.make_problem(2, N=N, H=H)
_, _, prob = fused.describe_problem(pr["model"], pr["cost"], dev, 0)
a, s = prob.mdesc["a"], prob.mdesc["s"]
P = _lib.ptr
stream = _lib.stream_handle(dev)
BMAX = 16
gen = torch.Generator().manual_seed(0)
s0 = (pr["s0"].reshape(1, s) + 0.1 * torch.randn(BMAX, s, generator=gen)).to(dev).contiguous()
out = [torch.empty((BMAX, H, x), device=dev) for x in (a, a, a, s)]     # mu, sigma, actions, states
rows = torch.empty((BMAX, H, a), device=dev).uniform_(-0.5, 0.5)


def runner(kind, B, I, upd):
    if kind == "cem_batch":
        cem = _lib.CemParams(N, H, K, I, 0.1, -1.0, 1.0, 0.0, 0.5, 0, 1234)
        need = lib.mbrl_cem_plan_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(cem), B)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def go():
            rc = lib.mbrl_cem_plan_batch(*prob.refs, P(s0), B, ctypes.byref(cem), *[P(x) for x in out], P(ws),
                                         ws.numel(), stream)
            assert rc == 0, rc
        return go
    mp = _lib.MppiParams(N, H, I, upd, 1.0, 0.1, -1.0, 1.0, 0.0, 0.5, 1234)
    if kind == "mppi_batch":
        need = lib.mbrl_mppi_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(mp), B)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def go():
            rc = lib.mbrl_mppi_plan_batch(*prob.refs, P(s0), B, ctypes.byref(mp), P(rows), None, *[P(x) for x in out],
                                          None, None, None, None, P(ws), ws.numel(), stream)
            assert rc == 0, rc
        return go
    need = lib.mbrl_mppi_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(mp))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def go():   # B single plans, one after the other on the stream
        for b in range(B):
            rc = lib.mbrl_mppi_plan(*prob.refs, P(s0[b]), ctypes.byref(mp), P(rows[b]), *[P(x[b]) for x in out], None,
                                    None, None, None, None, P(ws), ws.numel(), stream)
            assert rc == 0, rc
    return go


def quartiles(v):
    q = np.percentile(np.array(v), [25, 50, 75])
    return dict(q1_ms=float(q[0]), median_ms=float(q[1]), q3_ms=float(q[2]), min_ms=float(min(v)), max_ms=float(max(v)))


res = dict(shape=dict(N=N, H=H, K_cem=K), calls=args.calls)
for B in (8, 16):
    for I in (1, 2, 5):
        for upd in (0, 1):
            runs = {"mppi_batch": runner("mppi_batch", B, I, upd), "mppi_singles": runner("singles", B, I, upd),
                    "cem_batch": runner("cem_batch", B, I, upd)}
            for go in runs.values():
                for _ in range(10):
                    go()
            torch.cuda.synchronize()
            pairs = {k: [] for k in runs}
            for _ in range(args.calls):               # interleaved: every variant in every round
                for k, go in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    go()
                    e1.record()
                    pairs[k].append((e0, e1))
            torch.cuda.synchronize()
            tag = f"B={B} I={I} update_sigma={upd}"
            stats = {k: quartiles([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in pairs.items()}
            for k, q in stats.items():
                res[f"{tag} {k}"] = q
                print(f"{tag} {k:12s}: median {q['median_ms']:.4f} ms  quartiles {q['q1_ms']:.4f}-{q['q3_ms']:.4f}  "
                      f"min {q['min_ms']:.4f}  max {q['max_ms']:.4f}", flush=True)
            ratio = stats["mppi_singles"]["median_ms"] / stats["mppi_batch"]["median_ms"]
            per_it = 1000.0 * (stats["mppi_batch"]["median_ms"] - stats["cem_batch"]["median_ms"]) / I
            res[f"{tag} singles_over_batch"] = float(ratio)
            res[f"{tag} mppi_minus_cem_us_per_iteration"] = float(per_it)
            print(f"{tag}: singles / batch {ratio:.2f}x; MPPI batch over CEM batch {per_it:+.1f} us per iteration",
                  flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
