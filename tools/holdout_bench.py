"""What a held-out loss per epoch costs: EnsembleModel.fit_members (mbrl_eval_members and mbrl_keep_best
enqueued after every epoch of the shared training launches) against the route there was before it -- one
train_members call per epoch followed by DynamicsModel.evaluate_model on every member (per batch a torch
gather, the H = 1 rollout forward, a criterion and a .cpu()). Cheetah-shaped 2 x 512 members (s = 17, a = 6),
E = 5, batch 512, a 2000-row holdout. Two more variants show where fit_members' time goes: train_members alone
for the same epochs, and the two new entries alone, once per epoch. All variants are interleaved call by call
in one run; device time from one event pair per call (host gaps inside a call included, as a user sees them),
reported per epoch as quartiles over the calls (profiles/holdout/README.md).

    python tools/holdout_bench.py [--calls 30] [--epochs 5] [--out file.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mujoco-mbrl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mbrl_amd import data, models  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--transitions", type=int, default=10240)
ap.add_argument("--holdout", type=int, default=2000)
args = ap.parse_args()

dev = torch.device("cuda:0")
S, A, W, BATCH, E = 17, 6, 512, 512, 5


def dataset(T, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    st = rng.standard_normal((T + 2, S)).astype(np.float32)
    roll = data.Rollout(states=list(torch.from_numpy(st)), observations=list(torch.from_numpy(st)),
                        actions=list(torch.from_numpy(rng.uniform(-1, 1, (T + 1, A)).astype(np.float32))),
                        rewards=list(torch.from_numpy(rng.standard_normal(T + 1).astype(np.float32))))
    ds = data.TransitionsDataset(rollouts=[roll], horizon=1)
    ds.set_data_mode("state_only")
    return ds


def quartiles(v, epochs):
    q = np.percentile(np.array(v) / epochs, [25, 50, 75])
    return dict(q1_ms=float(q[0]), median_ms=float(q[1]), q3_ms=float(q[2]), min_ms=float(min(v) / epochs),
                max_ms=float(max(v) / epochs))


def ensemble(seed):
    torch.manual_seed(seed)
    ens = models.EnsembleModel([models.Model(S, A, hidden_units=W) for _ in range(E)]).to(dev)
    return ens, [torch.optim.Adam(m.parameters(), lr=1e-4) for m in ens.members]


train, hold = dataset(args.transitions, 0), dataset(args.holdout, 1)
calls = [0]


def fit_members():
    ens, opts = fit_side
    report = ens.fit_members(train, hold, opts, batch_size=BATCH, max_epochs=args.epochs, seed=calls[0])
    assert report["native_epochs"] == args.epochs and report["native_eval"], "fit_members left the native path"


def train_then_evaluate_model():
    ens, opts = old_side
    for k in range(args.epochs):
        assert ens.train_members(train, opts, batch_size=BATCH, num_epochs=1, seed=calls[0] + k) == 1
        for m in ens.members:
            m.evaluate_model(hold, BATCH)


def train_members_only():
    ens, opts = train_side
    assert ens.train_members(train, opts, batch_size=BATCH, num_epochs=args.epochs, seed=calls[0]) == args.epochs


def new_entries_only():
    for k in range(args.epochs):
        tracker.record(k)


fit_side, old_side, train_side, entry_side = (ensemble(i) for i in range(4))
tracker = models._Holdout(list(entry_side[0].members), hold, args.epochs)
assert tracker.native is not None
runs = dict(fit_members=fit_members, train_then_evaluate_model=train_then_evaluate_model,
            train_members_only=train_members_only, new_entries_only=new_entries_only)
for go in runs.values():
    for _ in range(3):
        go()
torch.cuda.synchronize()
pairs = {k: [] for k in runs}
for _ in range(args.calls):                  # interleaved: every variant in every round
    calls[0] += 1
    for k, go in runs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        pairs[k].append((e0, e1))
        torch.cuda.synchronize()             # a call starts on an idle GPU
steps = (train.num_transitions() + BATCH - 1) // BATCH
res = dict(calls=args.calls, epochs_per_call=args.epochs, transitions=train.num_transitions(),
           holdout=hold.num_transitions(), batch=BATCH, members=E, adam_steps_per_epoch=steps, unit="ms per epoch")
print(f"{E} members of 2x{W}, s={S} a={A}, batch {BATCH}, {train.num_transitions()} training rows ({steps} steps per "
      f"epoch), {hold.num_transitions()} held-out rows, {args.epochs} epochs per call, {args.calls} calls", flush=True)
for k, v in pairs.items():
    q = res[k] = quartiles([e0.elapsed_time(e1) for e0, e1 in v], args.epochs)
    print(f"{k:26s}: median {q['median_ms']:.3f} ms per epoch  quartiles {q['q1_ms']:.3f}-{q['q3_ms']:.3f}  "
          f"min {q['min_ms']:.3f}  max {q['max_ms']:.3f}", flush=True)
med = {k: res[k]["median_ms"] for k in runs}
res["fit_over_train_then_evaluate_model"] = med["fit_members"] / med["train_then_evaluate_model"]
res["fit_minus_train_minus_entries_ms"] = med["fit_members"] - med["train_members_only"] - med["new_entries_only"]
print(f"fit_members / (train_members + evaluate_model per member) = {res['fit_over_train_then_evaluate_model']:.3f}")
print(f"fit_members - train_members - the two entries = {res['fit_minus_train_minus_entries_ms']:+.3f} ms per epoch")
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
