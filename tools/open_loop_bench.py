"""What the open-loop held-out metric costs: mbrl_eval_members_open_loop (one call: E x R chains of H fed-back
steps inside the workgroups) against the torch restatement of the same definition on the same GPU
(models._eval_members_open_loop_torch: E x H x (L + 1) matmul launches plus their glue, what a user had before
the entry), and EnsembleModel.fit_members per epoch with holdout_loss="open_loop" against "one_step" on the same
horizon-H holdout. Cheetah-shaped 2 x 512 members (s = 17, a = 6), E = 5, 2000 held-out rows, horizon 30; batch
512 on 10 240 one-step training rows. With --parent-lib (a build of the previous commit's sources) the one-step
entry and fit_members("one_step") are also timed through that library, interleaved with this one's, as the
regression check. All variants of a group are interleaved call by call in one process; device time from one
event pair per call (host gaps inside a call included, as a user sees them); every call starts on an idle GPU.

    python tools/open_loop_bench.py [--calls 100] [--fit-calls 30] [--epochs 5] [--parent-lib so] [--out file.json]"""
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
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--fit-calls", type=int, default=30)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--transitions", type=int, default=10240)
ap.add_argument("--holdout", type=int, default=2000)
ap.add_argument("--horizon", type=int, default=30)
ap.add_argument("--parent-lib", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "open_loop_bench.py measures on a GPU"
dev = torch.device("cuda:0")
S, A, W, BATCH, E = 17, 6, 512, 512, 5


def dataset(T, horizon, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    st = rng.standard_normal((T + horizon + 1, S)).astype(np.float32)
    roll = data.Rollout(states=list(torch.from_numpy(st)), observations=list(torch.from_numpy(st)),
                        actions=list(torch.from_numpy(rng.uniform(-1, 1, (T + horizon, A)).astype(np.float32))),
                        rewards=list(torch.from_numpy(rng.standard_normal(T + horizon).astype(np.float32))))
    ds = data.TransitionsDataset(rollouts=[roll], horizon=horizon)
    ds.set_data_mode("state_only")
    assert ds.num_transitions() == T
    return ds


def quartiles(v, per=1):
    q = np.percentile(np.array(v) / per, [25, 50, 75])
    return dict(q1_ms=float(q[0]), median_ms=float(q[1]), q3_ms=float(q[2]), min_ms=float(min(v) / per),
                max_ms=float(max(v) / per), calls=len(v))


def ensemble(seed):
    torch.manual_seed(seed)
    ens = models.EnsembleModel([models.Model(S, A, hidden_units=W) for _ in range(E)]).to(dev)
    return ens, [torch.optim.Adam(m.parameters(), lr=1e-4) for m in ens.members]


def interleaved(runs, calls, warmup=3):
    """{name: [ms per call]}: every variant in every round, the round's first variant rotating, each call
    between two events on an idle GPU."""
    for go in runs.values():
        for _ in range(warmup):
            go()
    torch.cuda.synchronize()
    pairs = {k: [] for k in runs}
    names = list(runs)
    for i in range(calls):
        for k in names[i % len(names):] + names[:i % len(names)]:     # (no variant always follows the same one)
            go = runs[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            go()
            e1.record()
            pairs[k].append((e0, e1))
            torch.cuda.synchronize()
    return {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in pairs.items()}


def report(title, times, per=1, unit="ms per call"):
    out = {}
    print(title, flush=True)
    for k, v in times.items():
        q = out[k] = quartiles(v, per)
        print(f"  {k:34s}: median {q['median_ms']:.3f} {unit}  quartiles {q['q1_ms']:.3f}-{q['q3_ms']:.3f}  "
              f"min {q['min_ms']:.3f}  max {q['max_ms']:.3f}  ({q['calls']} calls)", flush=True)
    return out


parent = _lib.load_other(args.parent_lib) if args.parent_lib else None
train, hold = dataset(args.transitions, 1, 0), dataset(args.holdout, args.horizon, 1)
R, H = hold.num_transitions(), hold.horizon
print(f"{E} members of 2x{W}, s={S} a={A}; holdout {R} rows at horizon {H}; {train.num_transitions()} training rows, "
      f"batch {BATCH}; {torch.cuda.get_device_name(0)}", flush=True)
res = dict(members=E, hidden=W, holdout_rows=R, horizon=H, transitions=train.num_transitions(), batch=BATCH,
           epochs_per_call=args.epochs, device=torch.cuda.get_device_name(0))

# ---- 1. the entry against the torch restatement (and the one-step entry, this library's and the parent's)
ens = ensemble(0)[0]
members = list(ens.members)
_, ins, outs = hold.stacked(dev)
rows = torch.arange(R, dtype=torch.int64, device=dev)
assert models._NativeEval.supported(members, hold, ins, outs)
native = models._NativeEval(members, ins, outs, H)
row_err = torch.empty((E, R, H), dtype=torch.float32, device=dev)
loss3 = torch.empty((E, 3), dtype=torch.float32, device=dev)


def torch_open_loop():
    err = models._eval_members_open_loop_torch(members, ins, outs, rows)[0]
    return (err.sum(1) / (R * S)).sum(1)


runs = dict(entry_open_loop=lambda: native.run_open_loop(rows, row_err, loss3), torch_open_loop=torch_open_loop,
            entry_one_step=lambda: native.run(rows, row_err, loss3))
if parent is not None:
    with models.native_library(parent):
        native_parent = models._NativeEval(members, ins, outs, H)
    runs["entry_one_step_parent_lib"] = lambda: native_parent.run(rows, row_err, loss3)
# the same definition: the two losses agree to rounding before anything is timed
native.run_open_loop(rows, row_err, loss3)
got, want = loss3[:, 0].clone(), torch_open_loop()
torch.cuda.synchronize()
rel = float(((got - want).abs() / want.abs()).max())
print(f"open-loop loss, entry against torch: max relative difference {rel:.2e}", flush=True)
assert rel < 1e-4, (got, want)
res["loss_max_rel_diff_entry_vs_torch"] = rel
res["evaluation"] = report("one evaluation of the holdout", interleaved(runs, args.calls))
ev = res["evaluation"]
spread = (ev["entry_open_loop"]["q3_ms"] - ev["entry_open_loop"]["q1_ms"]) + \
    (ev["torch_open_loop"]["q3_ms"] - ev["torch_open_loop"]["q1_ms"])
gain = ev["torch_open_loop"]["median_ms"] - ev["entry_open_loop"]["median_ms"]
res["torch_over_entry"] = ev["torch_open_loop"]["median_ms"] / ev["entry_open_loop"]["median_ms"]
res["faster_by_more_than_the_spread"] = bool(gain > spread)
print(f"torch / entry = {res['torch_over_entry']:.2f}; torch - entry = {gain:.3f} ms against a summed quartile spread of "
      f"{spread:.3f} ms: {'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}",
      flush=True)

# ---- 2. fit_members per epoch: open loop against one step (and one step through the parent's library)
seeds = [0]


def fit(side, holdout_loss, lib=None):
    def go():
        e, opts = side
        ctx = models.native_library(lib) if lib is not None else None
        if ctx is not None:
            ctx.__enter__()
        try:
            rep = e.fit_members(train, hold, opts, batch_size=BATCH, max_epochs=args.epochs, seed=seeds[0],
                                holdout_loss=holdout_loss)
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
        assert rep["native_epochs"] == args.epochs and rep["native_eval"], "fit_members left the native path"
    return go


def train_only(side):
    def go():
        e, opts = side
        assert e.train_members(train, opts, batch_size=BATCH, num_epochs=args.epochs, seed=seeds[0]) == args.epochs
    return go


runs = dict(fit_open_loop=fit(ensemble(1), "open_loop"), fit_one_step=fit(ensemble(2), "one_step"),
            train_members_only=train_only(ensemble(3)))
if parent is not None:
    runs["fit_one_step_parent_lib"] = fit(ensemble(4), "one_step", parent)
res["fit_members"] = report("fit_members, per epoch", interleaved(runs, args.fit_calls), per=args.epochs,
                            unit="ms per epoch")
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
