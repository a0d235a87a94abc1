"""What training an ensemble's members together costs against training them one after another: one
EnsembleModel.train_members call (mbrl_train_epoch_ensemble: the members on a grid axis of shared launches)
against E back-to-back train_model calls on the members (mbrl_train_epoch: the fused step, one model per
launch), cheetah-shaped 2 x 512 members (s = 17, a = 6), batch 512, E in {1, 2, 5, 8}. The back-to-back calls
run through --parent-lib when given (a library built from the parent commit; the structs are the same), else
through this tree's library, where that entry is unchanged. With --xcd-lib (`make ens-xcd`: the same launches
with the members XCD-major instead of member-major) a third variant, ensemble_xcd, runs train_members through
that build. All sides train on the same dataset for the same
number of epochs and batches; both stage their row orders the same way. Device time from one event pair per
call (the host's enqueue gaps inside a call are part of it, as a user sees them), the two variants interleaved
call by call, quartiles over the calls (profiles/train_ensemble/README.md).

    python tools/train_ensemble_bench.py [--calls 30] [--epochs 5] [--parent-lib libmbrl_cem.so]
                                         [--xcd-lib libmbrl_cem_ens_xcd.so] [--out file.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mujoco-mbrl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mbrl_amd import _lib, data, models  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--transitions", type=int, default=10240)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--xcd-lib", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
lib = _lib.load()
base = _lib.load_other(args.parent_lib) if args.parent_lib else lib
xcd = _lib.load_other(args.xcd_lib) if args.xcd_lib else None
S, A, W, BATCH = 17, 6, 512, 512


def dataset(T):
    rng = np.random.Generator(np.random.PCG64(0))
    st = rng.standard_normal((T + 2, S)).astype(np.float32)
    roll = data.Rollout(states=list(torch.from_numpy(st)), observations=list(torch.from_numpy(st)),
                        actions=list(torch.from_numpy(rng.uniform(-1, 1, (T + 1, A)).astype(np.float32))),
                        rewards=list(torch.from_numpy(rng.standard_normal(T + 1).astype(np.float32))))
    ds = data.TransitionsDataset(rollouts=[roll], horizon=1)
    ds.set_data_mode("state_only")
    return ds


def quartiles(v):
    q = np.percentile(np.array(v), [25, 50, 75])
    return dict(q1_ms=float(q[0]), median_ms=float(q[1]), q3_ms=float(q[2]), min_ms=float(min(v)), max_ms=float(max(v)))


def measure(runs, calls):
    for go in runs.values():
        for _ in range(3):
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
            torch.cuda.synchronize()     # a call starts on an idle GPU: no variant hides behind the other's tail
    return {k: quartiles([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in pairs.items()}


ds = dataset(args.transitions)
steps = args.epochs * ((ds.num_transitions() + BATCH - 1) // BATCH)
res = dict(calls=args.calls, epochs=args.epochs, transitions=ds.num_transitions(), batch=BATCH,
           adam_steps_per_member_per_call=steps, parent_lib=bool(args.parent_lib), xcd_lib=bool(args.xcd_lib))
print(f"2x{W} members, s={S} a={A}, batch {BATCH}, {ds.num_transitions()} transitions, {args.epochs} epochs "
      f"({steps} Adam steps per member per call); back-to-back through "
      f"{'the parent library' if args.parent_lib else 'this library'}", flush=True)
for E in (1, 2, 5, 8):
    torch.manual_seed(E)
    apart = [models.Model(S, A, hidden_units=W).to(dev) for _ in range(E)]
    opt_a = [torch.optim.Adam(m.parameters(), lr=1e-4) for m in apart]

    def back_to_back():
        with models.native_library(base):
            for m, o in zip(apart, opt_a):
                m.train_model(ds, o, batch_size=BATCH, num_epochs=args.epochs)

    def ensemble_through(library):
        ens = models.EnsembleModel([models.Model(S, A, hidden_units=W) for _ in range(E)]).to(dev)
        opts = [torch.optim.Adam(m.parameters(), lr=1e-4) for m in ens.members]
        calls = [0]

        def go():
            calls[0] += 1
            with models.native_library(library):
                ran = ens.train_members(ds, opts, batch_size=BATCH, num_epochs=args.epochs, seed=calls[0])
            assert ran == args.epochs, "train_members did not take the shared launches"
        return go
    runs = dict(back_to_back=back_to_back, ensemble=ensemble_through(lib))
    if xcd is not None:
        runs["ensemble_xcd"] = ensemble_through(xcd)
    stats = measure(runs, args.calls)
    for k, q in stats.items():
        q["us_per_step_per_member"] = 1000.0 * q["median_ms"] / (steps * E)
        res[f"E={E} {k}"] = q
        print(f"E={E} {k:12s}: median {q['median_ms']:.3f} ms  quartiles {q['q1_ms']:.3f}-{q['q3_ms']:.3f}  "
              f"min {q['min_ms']:.3f}  max {q['max_ms']:.3f}  ({q['us_per_step_per_member']:.1f} us per step and member)",
              flush=True)
    for k in runs:
        if k != "back_to_back":
            ratio = stats[k]["median_ms"] / stats["back_to_back"]["median_ms"]
            res[f"E={E} {k}_over_back_to_back"] = float(ratio)
            print(f"E={E}: {k} / back to back = {ratio:.3f}", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
