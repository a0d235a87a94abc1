"""Epoch time of EnsembleModel.train_members(max_grad_norm=...) through the clipped epoch entries
(mbrl_train_epoch_open_loop_clipped, mbrl_train_epoch_ensemble_clipped) against
(a) the unclipped sibling entry of a library built from the parent commit's sources (--parent-lib),
(b) the unclipped sibling of this build, and
(c) the torch fallback with torch.nn.utils.clip_grad_norm_ (member by member through autograd),
on one GPU in one run.

The paths are timed interleaved, the order rotating from sample to sample, one whole epoch per sample between two
device synchronisations, after one untimed epoch each; medians and quartiles are reported, and the microseconds the two norm
launches add per batch over the unclipped sibling. Shape: E = 5 members of 2 x 512, s = 17, a = 6, batch 512,
10 240 rows; the open-loop loss at horizons 5 and 30 and the teacher-forced loss at horizon 1.

    make -C mujoco-mbrl_amd                       # in a checkout of the parent commit -> its libmbrl_cem.so
    python tools/grad_clip_bench.py --parent-lib <that libmbrl_cem.so> --out profiles/grad_clip/epoch_ms.json
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from train_open_loop_bench import dataset  # noqa: E402

LAUNCHES_ADDED = 2      # grad_sumsq_kernel and grad_norm_finish_kernel, ahead of the clipped Adam launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmbrl_cem.so built from the parent commit's sources")
    ap.add_argument("--members", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rows", type=int, default=10240)
    ap.add_argument("--horizons", type=int, nargs="+", default=[5, 30])
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mbrl_amd import _lib, models
    dev = torch.device("cuda", 0)
    s, a = 17, 6
    parent = _lib.load_other(args.parent_lib) if args.parent_lib else None
    names = ["torch_clipped", "native_unclipped", "native_clipped"] + (["parent_unclipped"] if parent else [])
    result = dict(gpu=torch.cuda.get_device_name(0), members=args.members, hidden=args.hidden, batch=args.batch,
                  state_dim=s, action_dim=a, samples=args.samples, max_norm=args.max_norm,
                  parent_lib=bool(parent), launches_added_per_batch=LAUNCHES_ADDED, cases={})
    for loss, H in [("open_loop", h) for h in args.horizons] + [("one_step", 1)]:
        ds = dataset(s, a, H, args.rows, seed=H)
        runs = {}
        for name in names:
            torch.manual_seed(0)
            ens = models.EnsembleModel([models.Model(s, a, hidden_units=args.hidden) for _ in range(args.members)]).to(dev)
            runs[name] = (ens, [torch.optim.Adam(m.parameters(), lr=1e-4) for m in ens.members])
        clipped_batches = []

        class Norms:                      # (only the untimed epoch takes a writer: it shows how many batches clip)
            def add_scalar(self, tag, value, it):
                if tag.startswith("grad_norm/"):
                    clipped_batches.append(float(value) > args.max_norm)

        def epoch(name, k, writer=None):
            ens, opts = runs[name]
            models.NATIVE_TRAINING = name != "torch_clipped"
            kw = {} if name.endswith("unclipped") else dict(max_grad_norm=args.max_norm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with models.native_library(parent if name == "parent_unclipped" else None):
                ran = ens.train_members(ds, opts, batch_size=args.batch, num_epochs=1, seed=k, loss=loss, writer=writer,
                                        **kw)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            models.NATIVE_TRAINING = True
            assert ran == (0 if name == "torch_clipped" else 1), (name, ran)
            return dt
        times = {name: [] for name in runs}
        for name in runs:
            epoch(name, 0, Norms() if name == "native_clipped" else None)
        order = list(runs)
        for k in range(args.samples):         # the order rotates: an epoch right after the torch fallback's runs slower
            for name in order[k % len(order):] + order[:k % len(order)]:
                times[name].append(epoch(name, k + 1))
        batches = -(-ds.num_transitions() // args.batch)
        row = dict(loss=loss, horizon=H, rows=ds.num_transitions(), batches=batches,
                   clipped_batches_first_epoch=int(sum(clipped_batches)), member_batches_first_epoch=len(clipped_batches))
        for name, t in times.items():
            q1, med, q3 = (float(x) for x in np.percentile(t, [25, 50, 75]))
            row[name] = dict(median_ms=med, q1_ms=q1, q3_ms=q3, samples_ms=[round(x, 3) for x in t])
        new, ref = row["native_clipped"], row["torch_clipped"]
        spread = (new["q3_ms"] - new["q1_ms"]) + (ref["q3_ms"] - ref["q1_ms"])
        row["speedup_over_torch"] = ref["median_ms"] / new["median_ms"]
        row["gain_ms"] = ref["median_ms"] - new["median_ms"]
        row["summed_quartile_spread_ms"] = spread
        row["beats_torch_beyond_spread"] = bool(row["gain_ms"] > spread)
        for base in ("native_unclipped", "parent_unclipped"):
            if base in row:
                row[f"added_us_per_batch_over_{base}"] = (new["median_ms"] - row[base]["median_ms"]) * 1e3 / batches
        result["cases"][f"{loss}_h{H}"] = row
        print(json.dumps({f"{loss}_h{H}": {k: v for k, v in row.items() if not isinstance(v, dict)}}), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
