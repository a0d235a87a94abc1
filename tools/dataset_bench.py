#!/usr/bin/env python
"""Times the data path of model fitting: add_rollouts and stacked() of DeviceTransitionsDataset against the
parent TransitionsDataset on the same rollouts, in one run on the GPU machine, and the two entries' device time
against the bytes they move.

    python tools/dataset_bench.py [--out profiles/dataset] [--reps 7] [--host-reps 3]

Shapes: s = o = 17, a = 6, float32 rollouts of 1000 steps; (rollouts, horizon) = (10, 1), (10, 5), (40, 1),
(100, 1). Every timing is a median of repeated calls with quartiles; a host clock around work that ends in a
device synchronise. The entries' own time is taken with device events around `--launches` back-to-back calls on
fixed inputs; the bytes are what the algorithm needs, computed from the shapes: mbrl_dataset_stack reads and
writes T * horizon * dim floats per field plus the window rows; mbrl_dataset_stats reads R * dim floats per field
twice plus the row lists twice. The copy rate to hold them against is the 6.29 TB/s a float4 copy reaches on the
MI355X. Needs a GPU: there is no CPU fallback for the device numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "mujoco-mbrl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_BYTES_PER_S = 6.29e12
SHAPES = ((10, 1), (10, 5), (40, 1), (100, 1))
S_DIM, A_DIM, STEPS = 17, 6, 1000


def make_rollouts(n, seed):
    from mbrl_amd.data import Rollout
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        st = torch.randn(STEPS, S_DIM, generator=g)
        ob = torch.randn(STEPS, S_DIM, generator=g)
        out.append(Rollout(states=list(st), observations=list(ob),
                           actions=list(torch.rand(STEPS - 1, A_DIM, generator=g) * 2 - 1),
                           rewards=list(torch.randn(STEPS - 1, generator=g))))
    return out


def quartiles(xs):
    q1, med, q3 = np.percentile(np.asarray(xs, np.float64), [25, 50, 75])
    return {"median_s": float(med), "q1_s": float(q1), "q3_s": float(q3), "n": len(xs)}


def timed(fn, reps, sync):
    out = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def device_time(fn, launches, reps):
    """Seconds per call from device events around `launches` back-to-back calls."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / launches)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dataset"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dataset_bench.py needs a GPU")
    from mbrl_amd import DeviceTransitionsDataset, device_data
    from mbrl_amd.data import TransitionsDataset
    dev = "cuda:0"
    results = []
    for n, horizon in SHAPES:
        rollouts = make_rollouts(n, seed=n + horizon)
        row = {"rollouts": n, "steps": STEPS, "horizon": horizon}
        # warm-up: code objects, allocator
        DeviceTransitionsDataset(rollouts, horizon=horizon, device=dev).stacked(dev)

        def fresh_device():
            return DeviceTransitionsDataset(rollouts, horizon=horizon, device=dev)
        row["device_add_rollouts"] = quartiles(timed(fresh_device, args.reps, True))
        ds = fresh_device()
        row["transitions"] = ds.num_transitions()

        def restack():
            ds._stacked = None
            ds.stacked(dev)
        row["device_stacked"] = quartiles(timed(restack, args.reps, True))
        row["host_add_rollouts"] = quartiles(timed(lambda: TransitionsDataset(rollouts, horizon=horizon),
                                                   args.host_reps, False))
        host = TransitionsDataset(rollouts, horizon=horizon)

        def host_restack():
            host._stacked = None
            host.stacked(dev)
        row["host_stacked"] = quartiles(timed(host_restack, args.host_reps, True))
        row["speedup_add_rollouts"] = row["host_add_rollouts"]["median_s"] / row["device_add_rollouts"]["median_s"]
        row["speedup_stacked"] = row["host_stacked"]["median_s"] / row["device_stacked"]["median_s"]

        # the entries alone, on fixed inputs
        lengths = np.asarray(ds._row_lens, np.int64) - 1
        win_row = torch.from_numpy(device_data.window_rows(lengths, horizon)[0]).to(dev)
        ins, outs = device_data.mode_fields("both")
        table = [(ds._store[f], ds._dev_stats[f][0], ds._dev_stats[f][1], sh) for f, sh in ins + outs]
        T = win_row.numel()
        stack_bytes = sum(2 * T * horizon * t[0].shape[1] * 4 for t in table) + 8 * T
        st = quartiles(device_time(lambda: device_data.dataset_stack(table, win_row, horizon), args.launches, args.reps))
        row["stack_kernel"] = dict(st, bytes=stack_bytes, bytes_per_s=stack_bytes / st["median_s"],
                                   share_of_copy_rate=stack_bytes / st["median_s"] / COPY_BYTES_PER_S)
        lists = device_data.stat_rows(lengths)
        rows = {f: torch.from_numpy(lists[f]).to(dev) for f in device_data.FIELDS}
        fields = [(ds._store[f], rows[f]) for f in device_data.FIELDS]
        stats_bytes = sum(2 * (r.numel() * s.shape[1] * 4 + r.numel() * 8) for s, r in fields)
        st = quartiles(device_time(lambda: device_data.dataset_stats(fields), args.launches, args.reps))
        row["stats_kernels"] = dict(st, launches=4, bytes=stats_bytes, bytes_per_s=stats_bytes / st["median_s"],
                                    share_of_copy_rate=stats_bytes / st["median_s"] / COPY_BYTES_PER_S)
        results.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "dataset_bench.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "copy_bytes_per_s": COPY_BYTES_PER_S,
                   "state_dim": S_DIM, "action_dim": A_DIM, "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
