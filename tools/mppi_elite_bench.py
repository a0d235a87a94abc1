"""What the elite-restricted MPPI plans cost over the classic ones: ms per plan of mbrl_mppi_plan_elite against
mbrl_mppi_plan (cheetah, N = 4096, H = 30, K = 409, I = 2 and 5) and ms per batch of mbrl_mppi_plan_elite_batch
against mbrl_mppi_plan_batch (cartpole service shape N = 1024, H = 20, K = 102, B = 8 and 16, I = 2), update_sigma
on, every problem mid-episode (mean rows). The classic entries are taken from --parent-lib when given (a library
built from the parent commit; the packed model and every struct are the same), else from this tree's library, where
they are unchanged. Device time from one event pair per call; the two variants of a shape are interleaved call by
call; the quartiles over the calls and the per-iteration difference of the medians are reported
(profiles/mppi_elite/README.md).

    python tools/mppi_elite_bench.py [--calls 300] [--parent-lib libmbrl_cem.so] [--out file.json]"""
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
ap.add_argument("--parent-lib", default=None)
args = ap.parse_args()

base = lib
if args.parent_lib:
    base = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in ("mbrl_mppi_workspace_bytes", "mbrl_mppi_plan", "mbrl_mppi_batch_workspace_bytes", "mbrl_mppi_plan_batch"):
        getattr(base, name).argtypes = getattr(lib, name).argtypes
        getattr(base, name).restype = getattr(lib, name).restype
P = _lib.ptr
stream = _lib.stream_handle(dev)
INF = float("inf")


def quartiles(v):
    q = np.percentile(np.array(v), [25, 50, 75])
    return dict(q1_ms=float(q[0]), median_ms=float(q[1]), q3_ms=float(q[2]), min_ms=float(min(v)), max_ms=float(max(v)))


def measure(runs, calls):
    for go in runs.values():
        for _ in range(10):
            go()
    torch.cuda.synchronize()
    pairs = {k: [] for k in runs}
    for _ in range(calls):               # interleaved: every variant in every round
        for k, go in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            go()
            e1.record()
            pairs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: quartiles([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in pairs.items()}


def problem(cid, N, H, B):
    pr = synthetic.make_problem(cid, N=N, H=H)
    _, _, prob = fused.describe_problem(pr["model"], pr["cost"], dev, 0)
    a, s = prob.mdesc["a"], prob.mdesc["s"]
    gen = torch.Generator().manual_seed(0)
    s0 = (pr["s0"].reshape(1, s) + 0.1 * torch.randn(B, s, generator=gen)).to(dev).contiguous()
    out = [torch.empty((B, H, x), device=dev) for x in (a, a, a, s)]     # mu, sigma, actions, states
    rows = torch.empty((B, H, a), device=dev).uniform_(-0.5, 0.5)
    return prob, s0, out, rows


def report(res, tag, stats, I):
    for k, q in stats.items():
        res[f"{tag} {k}"] = q
        print(f"{tag} {k:8s}: median {q['median_ms']:.4f} ms  quartiles {q['q1_ms']:.4f}-{q['q3_ms']:.4f}  "
              f"min {q['min_ms']:.4f}  max {q['max_ms']:.4f}", flush=True)
    per_it = 1000.0 * (stats["elite"]["median_ms"] - stats["classic"]["median_ms"]) / I
    res[f"{tag} elite_minus_classic_us_per_iteration"] = float(per_it)
    print(f"{tag}: elite over classic {per_it:+.1f} us per iteration", flush=True)


res = dict(calls=args.calls, parent_lib=bool(args.parent_lib))

# ---- the single plan: cheetah, N = 4096, H = 30, K = 409
N, H, K = 4096, 30, 409
prob, s0, out, rows = problem(3, N, H, 1)
for I in (2, 5):
    mp = _lib.MppiParams(N, H, I, 1, 1.0, 0.1, -1.0, 1.0, 0.0, 0.5, 1234)
    ep = _lib.MppiEliteParams(mp, K, 0, 0.0, INF)
    ws = torch.empty(max(base.mbrl_mppi_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(mp)),
                         lib.mbrl_mppi_elite_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(ep), 1)),
                     dtype=torch.uint8, device=dev)

    def classic(mp=mp, ws=ws):
        rc = base.mbrl_mppi_plan(*prob.refs, P(s0[0]), ctypes.byref(mp), P(rows[0]), *[P(x[0]) for x in out], None, None,
                                 None, None, None, P(ws), ws.numel(), stream)
        assert rc == 0, rc

    def elite(ep=ep, ws=ws):
        rc = lib.mbrl_mppi_plan_elite(*prob.refs, P(s0[0]), ctypes.byref(ep), P(rows[0]), None, *[P(x[0]) for x in out],
                                      None, None, None, None, None, None, P(ws), ws.numel(), stream)
        assert rc == 0, rc
    report(res, f"cheetah N={N} H={H} K={K} I={I}", measure(dict(classic=classic, elite=elite), args.calls), I)

# ---- the batch: cartpole service shape, N = 1024, H = 20, K = 102
N, H, K, I = 1024, 20, 102, 2
prob, s0, out, rows = problem(2, N, H, 16)
for B in (8, 16):
    mp = _lib.MppiParams(N, H, I, 1, 1.0, 0.1, -1.0, 1.0, 0.0, 0.5, 1234)
    ep = _lib.MppiEliteParams(mp, K, 0, 0.0, INF)
    ws = torch.empty(max(base.mbrl_mppi_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(mp), B),
                         lib.mbrl_mppi_elite_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(ep), B)),
                     dtype=torch.uint8, device=dev)

    def classic(mp=mp, ws=ws, B=B):
        rc = base.mbrl_mppi_plan_batch(*prob.refs, P(s0), B, ctypes.byref(mp), P(rows), None, *[P(x) for x in out], None,
                                       None, None, None, P(ws), ws.numel(), stream)
        assert rc == 0, rc

    def elite(ep=ep, ws=ws, B=B):
        rc = lib.mbrl_mppi_plan_elite_batch(*prob.refs, P(s0), B, ctypes.byref(ep), P(rows), None, None,
                                            *[P(x) for x in out], None, None, None, None, None, P(ws), ws.numel(), stream)
        assert rc == 0, rc
    report(res, f"cartpole N={N} H={H} K={K} I={I} B={B}", measure(dict(classic=classic, elite=elite), args.calls), I)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
