"""MPPIPlanner against CEMPlanner on one tree and one machine, at the bench workload (cheetah, N = 4096,
H = 30, 3 x 512, I = 5), and the MPPI update alone at the humanoid shape (N = 32768, a = 21, H = 50).

Plans alternate CEM / MPPI so both see the same machine state. Two passes:
  spans  -- one event pair per plan around the C call that enqueues it: device ms per plan (median,
            quartiles), no event inside the plan;
  gaps   -- every iteration's rollout bracketed (rollout_events): the time from one rollout's end to
            the next one's start is the update launch between them (plus one event record, the same
            for both planners), and the bracketed time is the rollout itself.
The update alone is timed over back-to-back calls between two events (mean per call).
Usage: python tools/mppi_bench.py [--plans K] [--warmup W]; prints JSON lines."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mujoco-mbrl_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mbrl_amd import CEMPlanner, MPPIPlanner, fused, synthetic  # noqa: E402

I = 5


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()          # torch creates its events lazily: record once so the C ABI gets a live handle
    return e


def _q(x):
    x = np.asarray(x, np.float64)
    return dict(median=round(float(np.median(x)), 5), q1=round(float(np.percentile(x, 25)), 5),
                q3=round(float(np.percentile(x, 75)), 5), min=round(float(x.min()), 5), n=int(x.size))


def plans(args):
    prob = synthetic.make_problem(3)
    H, N = prob["cfg"]["H"], prob["cfg"]["N"]
    base = dict(num_candidates=N, num_iterations=I, seed=prob["rng_seed"], return_device=True)
    kinds = {
        "cem": (CEMPlanner, dict(base, num_elites=N // 10, alpha=0.1)),
        "mppi": (MPPIPlanner, dict(base, temperature=1.0, alpha=0.1, update_sigma=True)),
        "mppi_classic": (MPPIPlanner, dict(base, temperature=1.0)),
    }

    def run(kind, **extra):
        cls, kw = kinds[kind]
        return cls.plan_detailed(prob["s0"].cuda(), prob["model"], prob["cost"], prob["sample_action"], H, **kw, **extra)

    for kind in kinds:
        for _ in range(args.warmup):
            run(kind)
    torch.cuda.synchronize()
    spans = {k: [(_event(), _event()) for _ in range(args.plans)] for k in kinds}
    torch.cuda.synchronize()
    for i in range(args.plans):
        for kind in kinds:
            run(kind, plan_events=spans[kind][i])
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in spans.items()}
    for kind in kinds:
        print(json.dumps(dict(what="plan_ms", planner=kind, N=N, H=H, I=I, **_q(ms[kind]))), flush=True)
    for kind in ("mppi", "mppi_classic"):
        print(json.dumps(dict(what="plan_ratio_vs_cem", planner=kind,
                              ratio=round(float(np.median(ms[kind]) / np.median(ms["cem"])), 4))), flush=True)
    evs = {k: [[(_event(), _event()) for _ in range(I)] for _ in range(args.plans)] for k in kinds}
    torch.cuda.synchronize()
    for i in range(args.plans):
        for kind in kinds:
            run(kind, rollout_events=evs[kind][i])
    torch.cuda.synchronize()
    for kind in kinds:
        roll = [p[it][0].elapsed_time(p[it][1]) for p in evs[kind] for it in range(I)]
        gap = [p[it][1].elapsed_time(p[it + 1][0]) * 1e3 for p in evs[kind] for it in range(I - 1)]
        print(json.dumps(dict(what="rollout_ms", planner=kind, **_q(roll))), flush=True)
        print(json.dumps(dict(what="update_gap_us", planner=kind, **_q(gap))), flush=True)


def updates(args):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    for N, a, H, E, draw in [(4096, 6, 30, 1, True), (32768, 21, 50, 5, False)]:
        costs = torch.from_numpy(rng.uniform(130, 250, (E, N)).astype(np.float32)).to(dev)
        acts = torch.from_numpy(rng.uniform(-1, 1, (H, N, a)).astype(np.float32)).to(dev)
        mu, sg = torch.zeros((H, a), device=dev), torch.full((H, a), 0.5, device=dev)
        mu_o, sg_o = torch.empty_like(mu), torch.empty_like(sg)
        nxt = torch.empty((H, N, a), device=dev) if draw else None
        sp = fused.make_sampler(7, 1, mu, sg, -1.0, 1.0)
        calls = {f"mppi_update sigma={int(u)}": (lambda u=u: fused.mppi_update(costs, acts, sp, H, a, 10.0, 0.1, u, mu_o,
                                                                               sg_o, next_actions=nxt))
                 for u in (False, True)}
        if draw:
            calls["cem_update"] = lambda: fused.cem_update(costs[:1], N // 10, sp, H, a, 0.1, mu_o, sg_o, next_actions=nxt)
        for name, fn in calls.items():
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            reps, per = 5, 40
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / per)
            print(json.dumps(dict(what="update_us_per_call", call=name, N=N, a=a, H=H, E=E, draw=bool(draw),
                                  row_bytes=N * a * 4, **_q(us))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    print(json.dumps(dict(what="device", name=torch.cuda.get_device_name(0))), flush=True)
    plans(args)
    updates(args)


if __name__ == "__main__":
    main()
