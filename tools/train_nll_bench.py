"""Epoch time of EnsembleModel.train_members(loss="nll") on ProbabilisticModel members through
mbrl_train_epoch_nll against (a) the same loss through torch autograd (the member-by-member fallback) and
(b) mbrl_train_epoch_ensemble, the MSE epoch of the same build, on Model members of the same trunk on the same
dataset, on one GPU in one run.

The three paths are timed interleaved (a, b, new, a, b, new, ...), one whole epoch per sample between two
device synchronisations, after one untimed epoch each; medians and quartiles are reported. Shape: E = 5 members
of 2 x 512, s = 17, a = 6, batch 512, 10 240 rows, horizon 1. The NLL epoch's launches per batch are
n_hidden + 5 whatever E is (include/mbrl_cem.h): the run records the count the header states beside the times.

    python tools/train_nll_bench.py --out profiles/train_nll/epoch_ms.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mujoco-mbrl_amd"))


def dataset(s, a, horizon, rows, seed):
    from mbrl_amd import data
    rng = np.random.Generator(np.random.PCG64(seed))
    rolls, per = [], rows // 4 + horizon
    for _ in range(4):
        st = (0.3 * rng.standard_normal((per + 1, s))).astype(np.float32)
        rolls.append(data.Rollout(states=list(torch.from_numpy(st)), observations=list(torch.from_numpy(st)),
                                  actions=list(torch.from_numpy(rng.uniform(-1, 1, (per, a)).astype(np.float32))),
                                  rewards=list(torch.from_numpy(rng.standard_normal(per).astype(np.float32)))))
    ds = data.TransitionsDataset(rollouts=rolls, horizon=horizon)
    ds.set_data_mode("state_only")
    return ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rows", type=int, default=10240)
    ap.add_argument("--horizons", type=int, nargs="+", default=[1])
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mbrl_amd import models
    dev = torch.device("cuda", 0)
    s, a = 17, 6
    result = dict(gpu=torch.cuda.get_device_name(0), members=args.members, hidden=args.hidden, batch=args.batch,
                  state_dim=s, action_dim=a, samples=args.samples, horizons={})
    for H in args.horizons:
        ds = dataset(s, a, H, args.rows, seed=H)
        runs = {}
        for name in ("torch_nll", "native_mse", "native_nll"):
            torch.manual_seed(0)
            kind = models.Model if name == "native_mse" else models.ProbabilisticModel
            ens = models.EnsembleModel([kind(s, a, hidden_units=args.hidden) for _ in range(args.members)]).to(dev)
            opts = [torch.optim.Adam(m.parameters(), lr=1e-4) for m in ens.members]
            runs[name] = (ens, opts)

        def epoch(name, k):
            ens, opts = runs[name]
            models.NATIVE_TRAINING = name != "torch_nll"
            loss = "one_step" if name == "native_mse" else "nll"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ran = ens.train_members(ds, opts, batch_size=args.batch, num_epochs=1, seed=k, loss=loss)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            models.NATIVE_TRAINING = True
            assert ran == (0 if name == "torch_nll" else 1), (name, ran)
            return dt
        times = {name: [] for name in runs}
        for name in runs:
            epoch(name, 0)
        for k in range(args.samples):
            for name in runs:
                times[name].append(epoch(name, k + 1))
        row = dict(rows=ds.num_transitions(), launches_per_batch_by_contract=2 + 5)
        for name, t in times.items():
            q1, med, q3 = (float(x) for x in np.percentile(t, [25, 50, 75]))
            row[name] = dict(median_ms=med, q1_ms=q1, q3_ms=q3, samples_ms=[round(x, 3) for x in t])
        new, ref, one = row["native_nll"], row["torch_nll"], row["native_mse"]
        spread = (new["q3_ms"] - new["q1_ms"]) + (ref["q3_ms"] - ref["q1_ms"])
        row["speedup_over_torch"] = ref["median_ms"] / new["median_ms"]
        row["gain_ms"] = ref["median_ms"] - new["median_ms"]
        row["summed_quartile_spread_ms"] = spread
        row["beats_torch_beyond_spread"] = bool(row["gain_ms"] > spread)
        row["ratio_to_mse_epoch"] = new["median_ms"] / one["median_ms"]
        result["horizons"][str(H)] = row
        print(json.dumps({H: {k: v for k, v in row.items() if not isinstance(v, dict)}}), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
