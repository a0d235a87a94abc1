"""ms/plan of mbrl_cem_plan_rh (keep = 0 and keep = 40) against mbrl_cem_plan on the cheetah headline
(N = 4096, H = 30, K = 409; I = 5 and I = 2), every variant interleaved in one run: 9 repeats of 100
back-to-back plans each, timed with events around the batch (profiles/cem_rh/README.md).

    python tools/cem_rh_bench.py [--baseline-lib path/to/another/libmbrl_cem.so] [--out file.json]

--baseline-lib: also time mbrl_cem_plan of another build of the library (e.g. the parent commit's)."""
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
ap.add_argument("--baseline-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
parent = None
if args.baseline_lib:
    parent = ctypes.CDLL(args.baseline_lib)
    for name in ("mbrl_cem_plan", "mbrl_cem_workspace_bytes"):
        getattr(parent, name).restype = getattr(lib, name).restype
        getattr(parent, name).argtypes = getattr(lib, name).argtypes

N, H, K = 4096, 30, 409
pr = synthetic.make_problem(3, N=N, H=H)
_, _, prob = fused.describe_problem(pr["model"], pr["cost"], dev, 0)
a, s = prob.mdesc["a"], prob.mdesc["s"]
s0 = pr["s0"].to(dev)
out = [torch.empty((H, x), device=dev) for x in (a, a, a, s)]
P = _lib.ptr
stream = _lib.stream_handle(dev)


def runner(kind, I, keep):
    cem = _lib.CemParams(N, H, K, I, 0.1, -1.0, 1.0, 0.0, 0.5, 0, 1234)
    if kind in ("plain", "parent"):
        L = parent if kind == "parent" else lib
        need = L.mbrl_cem_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(cem))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def go():
            rc = L.mbrl_cem_plan(*prob.refs, P(s0), ctypes.byref(cem), *[P(x) for x in out], None, None, None, None,
                                 P(ws), ws.numel(), stream)
            assert rc == 0, rc
        return go
    rp = _lib.CemRhParams(cem, keep, 0)
    need = lib.mbrl_cem_rh_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(rp))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    carry = torch.empty((max(keep, 1), H, a), device=dev)
    cret = torch.empty((max(keep, 1),), device=dev)

    def go():
        rc = lib.mbrl_cem_plan_rh(*prob.refs, P(s0), ctypes.byref(rp), None, None, None, *[P(x) for x in out],
                                  P(carry) if keep else None, P(cret) if keep else None, None, None, None, None, None,
                                  P(ws), ws.numel(), stream)
        assert rc == 0, rc
    return go


def time_ms(go, plans):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(plans):
        go()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / plans


res = {}
for I in (5, 2):
    runs = {"plain": runner("plain", I, 0), "rh_keep0": runner("rh", I, 0), "rh_keep40": runner("rh", I, 40)}
    if parent is not None:
        runs = dict(parent=runner("parent", I, 0), **runs)
    for go in runs.values():
        for _ in range(30):
            go()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for rep in range(9):                       # interleaved: every variant in every repeat
        for k, go in runs.items():
            samples[k].append(time_ms(go, 100))
    for k, v in samples.items():
        v = np.array(v)
        res[f"I={I} {k}"] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))
        print(f"I={I} {k:10s}: median {np.median(v):.4f} ms  min {v.min():.4f}  max {v.max():.4f}", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
