"""ms per plan of the coloured-noise plans (mbrl_cem_plan_rh_mixed, mbrl_cem_plan_rh_batch_mixed; a beta = 1
mix) against the white receding-horizon plans, every variant of one shape interleaved in one run: 7 repeats of
50 back-to-back plans each, timed with events around them (profiles/cem_noise/README.md).

  cheetah (N = 4096, H = 30, 3 x 512, K = 409), I = 2 and 5: white mbrl_cem_plan_rh with keep = 40 and keep = 0
      (the fused update), mixed with keep = 40 and keep = 0;
  the service shape (cartpole N = 1024, H = 20, K = 102, keep = 30), B = 8 and 16, I = 2 and 5: white
      mbrl_cem_plan_rh_batch against mixed.

    python tools/cem_noise_bench.py [--baseline-lib path/to/another/libmbrl_cem.so] [--out file.json]

--baseline-lib: run the white plans on another build of the library (the parent commit's); without it they
run on this tree's library."""
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
from mbrl_amd.planners import colored_noise_mix  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
ap = argparse.ArgumentParser()
ap.add_argument("--baseline-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--plans", type=int, default=50)
args = ap.parse_args()
white = lib
if args.baseline_lib:
    white = ctypes.CDLL(args.baseline_lib)
    for name in ("mbrl_cem_plan_rh", "mbrl_cem_rh_workspace_bytes", "mbrl_cem_plan_rh_batch",
                 "mbrl_cem_rh_batch_workspace_bytes"):
        getattr(white, name).restype = getattr(lib, name).restype
        getattr(white, name).argtypes = getattr(lib, name).argtypes
P = _lib.ptr
stream = _lib.stream_handle(dev)


def time_ms(go, plans):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(plans):
        go()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / plans


def interleaved(tag, runs, res):
    for go in runs.values():
        for _ in range(10):
            go()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for rep in range(args.repeats):            # interleaved: every variant in every repeat
        for k, go in runs.items():
            samples[k].append(time_ms(go, args.plans))
    for k, v in samples.items():
        v = np.array(v)
        res[f"{tag} {k}"] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))
        print(f"{tag} {k:18s}: median {np.median(v):.4f} ms  min {v.min():.4f}  max {v.max():.4f}", flush=True)
    return {k: float(np.median(v)) for k, v in samples.items()}


def single_runner(prob, N, H, K, I, keep, mix, rows, carry_in, s0, out, carry, cret):
    cem = _lib.CemParams(N, H, K, I, 0.1, -1.0, 1.0, 0.0, 0.5, 0, 1234)
    rp = _lib.CemRhParams(cem, keep, 0)
    ins = (P(rows), None, P(carry_in) if keep else None)
    tail = (*[P(x) for x in out], P(carry) if keep else None, P(cret) if keep else None, None, None, None, None, None)
    if mix is None:
        need = white.mbrl_cem_rh_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(rp))
        call, args_ = white.mbrl_cem_plan_rh, ins
    else:
        need = lib.mbrl_cem_rh_mixed_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(rp), 1)
        call, args_ = lib.mbrl_cem_plan_rh_mixed, ins + (P(mix),)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def go():
        rc = call(*prob.refs, P(s0), ctypes.byref(rp), *args_, *tail, P(ws), ws.numel(), stream)
        assert rc == 0, rc
    return go


def batch_runner(prob, B, N, H, K, I, keep, mix, rows, carry_in, s0, out, carry, cret):
    cem = _lib.CemParams(N, H, K, I, 0.1, -1.0, 1.0, 0.0, 0.5, 0, 1234)
    rp = _lib.CemRhParams(cem, keep, 0)
    ins = (P(rows), None, P(carry_in), None)
    tail = (*[P(x) for x in out], P(carry), P(cret), None, None, None, None)
    if mix is None:
        need = white.mbrl_cem_rh_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(rp), B)
        call, args_ = white.mbrl_cem_plan_rh_batch, ins
    else:
        need = lib.mbrl_cem_rh_mixed_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(rp), B)
        call, args_ = lib.mbrl_cem_plan_rh_batch_mixed, ins + (P(mix),)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def go():
        rc = call(*prob.refs, P(s0), B, ctypes.byref(rp), *args_, *tail, P(ws), ws.numel(), stream)
        assert rc == 0, rc
    return go


res = dict(white_plans_on="baseline-lib" if args.baseline_lib else "this tree", beta=1.0)

# ---- cheetah, single plans
N, H, K, KEEP = 4096, 30, 409, 40
pr = synthetic.make_problem(3, N=N, H=H)
_, _, prob = fused.describe_problem(pr["model"], pr["cost"], dev, 0)
a, s = prob.mdesc["a"], prob.mdesc["s"]
mix = torch.from_numpy(colored_noise_mix(H, 1.0)).to(dev)
s0 = pr["s0"].to(dev).contiguous()
out = [torch.empty((H, x), device=dev) for x in (a, a, a, s)]
carry, cret = torch.empty((KEEP, H, a), device=dev), torch.empty((KEEP,), device=dev)
rows = torch.empty((H, a), device=dev).uniform_(-0.5, 0.5)
carry_in = torch.empty((KEEP, H, a), device=dev).uniform_(-1.0, 1.0)
res["cheetah"] = dict(N=N, H=H, K=K, keep=KEEP)
for I in (2, 5):
    mk = lambda keep, m: single_runner(prob, N, H, K, I, keep, m, rows, carry_in, s0, out, carry, cret)  # noqa: E731
    med = interleaved(f"cheetah I={I}", {f"white_keep{KEEP}": mk(KEEP, None), f"mixed_keep{KEEP}": mk(KEEP, mix),
                                         "white_keep0_fused": mk(0, None), "mixed_keep0": mk(0, mix)}, res)
    over = 1000.0 * (med[f"mixed_keep{KEEP}"] - med[f"white_keep{KEEP}"]) / I
    over0 = 1000.0 * (med["mixed_keep0"] - med["white_keep0_fused"]) / I
    res[f"cheetah I={I} mixed_over_white_keep{KEEP}_us_per_iteration"] = over
    res[f"cheetah I={I} mixed_keep0_over_fused_us_per_iteration"] = over0
    print(f"cheetah I={I}: mixed {over:+.1f} us per iteration over white keep = {KEEP}; mixed keep = 0 {over0:+.1f} us "
          "per iteration over the fused white plan", flush=True)

# ---- the service shape, batched plans
N, H, K, KEEP = 1024, 20, 102, 30
pr = synthetic.make_problem(2, N=N, H=H)
_, _, prob = fused.describe_problem(pr["model"], pr["cost"], dev, 0)
a, s = prob.mdesc["a"], prob.mdesc["s"]
mix = torch.from_numpy(colored_noise_mix(H, 1.0)).to(dev)
BMAX = 16
gen = torch.Generator().manual_seed(0)
s0 = (pr["s0"].reshape(1, s) + 0.1 * torch.randn(BMAX, s, generator=gen)).to(dev).contiguous()
out = [torch.empty((BMAX, H, x), device=dev) for x in (a, a, a, s)]
carry, cret = torch.empty((BMAX, KEEP, H, a), device=dev), torch.empty((BMAX, KEEP), device=dev)
rows = torch.empty((BMAX, H, a), device=dev).uniform_(-0.5, 0.5)
carry_in = torch.empty((BMAX, KEEP, H, a), device=dev).uniform_(-1.0, 1.0)
res["service"] = dict(N=N, H=H, K=K, keep=KEEP)
for B in (8, 16):
    for I in (2, 5):
        mk = lambda m: batch_runner(prob, B, N, H, K, I, KEEP, m, rows, carry_in, s0, out, carry, cret)  # noqa: E731
        med = interleaved(f"service B={B} I={I}", {"white_batch": mk(None), "mixed_batch": mk(mix)}, res)
        over = 1000.0 * (med["mixed_batch"] - med["white_batch"]) / I
        res[f"service B={B} I={I} mixed_over_white_us_per_iteration"] = over
        print(f"service B={B} I={I}: mixed {over:+.1f} us per iteration over white", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
