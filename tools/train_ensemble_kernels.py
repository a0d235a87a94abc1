"""Per-launch device time of the ensemble training launches, from a rocprofv3 kernel trace: how one
launch's duration grows with E (one round of workgroups over the CUs per member, or several members a round).

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- \\
        python tools/train_ensemble_kernels.py run <E> [--lib libmbrl_cem_ens_xcd.so]
    python tools/train_ensemble_kernels.py summarise <dir> [<dir> ...] [--out file.json]

`run`: three train_members calls of 2 epochs (2 x 512 members, s = 17, a = 6, batch 512, 10240 transitions) --
one trace per E, each a run of its own. `summarise`: per trace, the median duration of every kernel whose name
holds train_gemm_ens_kernel or adam_step_kernel, keyed by its template arguments, over the full-size batches
(the last batch of an epoch here is full too), and their sum per batch (profiles/train_ensemble/README.md)."""
import csv
import glob
import json
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mujoco-mbrl_amd")]


def run(E, lib_path):
    import contextlib

    import numpy as np
    import torch

    from mbrl_amd import _lib, data, models
    S, A, W, BATCH, T = 17, 6, 512, 512, 10240
    rng = np.random.Generator(np.random.PCG64(0))
    st = rng.standard_normal((T + 2, S)).astype(np.float32)
    roll = data.Rollout(states=list(torch.from_numpy(st)), observations=list(torch.from_numpy(st)),
                        actions=list(torch.from_numpy(rng.uniform(-1, 1, (T + 1, A)).astype(np.float32))),
                        rewards=list(torch.from_numpy(rng.standard_normal(T + 1).astype(np.float32))))
    ds = data.TransitionsDataset(rollouts=[roll], horizon=1)
    ds.set_data_mode("state_only")
    torch.manual_seed(E)
    ens = models.EnsembleModel([models.Model(S, A, hidden_units=W) for _ in range(E)]).to("cuda:0")
    opts = [torch.optim.Adam(m.parameters(), lr=1e-4) for m in ens.members]
    ctx = models.native_library(_lib.load_other(lib_path)) if lib_path else contextlib.nullcontext()
    with ctx:
        for call in range(3):
            assert ens.train_members(ds, opts, batch_size=BATCH, num_epochs=2, seed=call) == 2
    torch.cuda.synchronize()
    print(f"E={E}: 3 train_members calls of 2 epochs done", flush=True)


def summarise(dirs, out):
    res = {}
    for d in dirs:
        trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
        by = {}
        for r in csv.DictReader(open(trace)):
            name = r["Kernel_Name"]
            if "train_gemm_ens_kernel" not in name and "adam_step_kernel" not in name:
                continue
            key = re.sub(r"^.*?(train_gemm_ens_kernel|adam_step_kernel)", r"\1", name).split("(")[0]
            dims = (int(r.get("Grid_Size_X", r.get("Grid_Size", 0))), int(r.get("Grid_Size_Y", 1) or 1))
            by.setdefault((key, dims), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        rows = {f"{k} grid={g}": dict(launches=len(v), median_us=statistics.median(v), min_us=min(v))
                for (k, g), v in sorted(by.items())}
        res[os.path.basename(os.path.normpath(d))] = rows
        print(d)
        for k, v in rows.items():
            print(f"  {v['median_us']:9.2f} us median  {v['min_us']:9.2f} min  x{v['launches']:5d}  {k}")
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None)
    else:
        args = sys.argv[2:]
        out = None
        if "--out" in args:
            out = args[args.index("--out") + 1]
            del args[args.index("--out"):args.index("--out") + 2]
        summarise(args, out)
