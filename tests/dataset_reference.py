"""NumPy restatement of the device-resident transitions (include/mbrl_cem.h mbrl_dataset_stack,
mbrl_dataset_stats): the step-store layout, the window gather and the float64 summation
order, each with the single-mistake mutants the tests must tell from the real thing.
tests/test_dataset_host.py pins the restatement to TransitionsDataset on the CPU; tests/test_gpu_dataset.py
compares the kernels with it bit for bit."""
import numpy as np
import torch

from mbrl_amd.data import Rollout
from mbrl_amd.device_data import FIELDS, mode_fields, rollout_first_rows, stat_rows, window_rows

PAD = 1.0e6      # what the reference store holds where the layout has padding: a read of it shows


def make_rollouts(lengths, s=5, o=4, a=3, dtype=torch.float32, seed=0, offset=0.0):
    """Rollouts with K = lengths[i] transitions of seeded values (columns of different scale and mean)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for K in lengths:
        def field(n, d):
            x = torch.randn(n, d, generator=g, dtype=torch.float64) * torch.arange(1, d + 1) + offset
            return list(x.to(dtype))
        rewards = list((torch.randn(K, generator=g, dtype=torch.float64) * 3.0 - 1.0 + offset).to(dtype))
        out.append(Rollout(states=field(K + 1, s), observations=field(K + 1, o), actions=field(K, a), rewards=rewards))
    return out


def store_from_rollouts(rollouts, pad=PAD, dtype=np.float32):
    """field -> [S][dim]: K + 1 rows per rollout, row k = (s_k, o_k, a_k, r_k); the last row's action and the
    first row's reward are padding."""
    cols = {f: [] for f in FIELDS}
    for r in rollouts:
        n = len(r) + 1
        cols["states"].append(torch.stack(list(r.states)).reshape(n, -1).numpy().astype(dtype))
        cols["observations"].append(torch.stack(list(r.observations)).reshape(n, -1).numpy().astype(dtype))
        act = torch.stack(list(r.actions[:-1])).reshape(n - 1, -1).numpy().astype(dtype)
        cols["actions"].append(np.concatenate([act, np.full((1, act.shape[1]), pad, dtype)]))
        rew = torch.stack(list(r.rewards[1:])).reshape(n - 1, -1).numpy().astype(dtype)
        cols["rewards"].append(np.concatenate([np.full((1, 1), pad, dtype), rew]))
    return {f: np.concatenate(v) for f, v in cols.items()}


def stack_reference(src, mean, std, win_row, horizon, shift, ignore_shift=False):
    """dst[t][h][j] = (src[win_row[t] + h + shift][j] - mean[j]) / std[j] in fp32 (a copy without statistics)."""
    rows = np.asarray(win_row, np.int64)[:, None] + np.arange(horizon, dtype=np.int64)[None, :]
    x = src[rows + (0 if ignore_shift else shift)]
    if mean is None:
        return x.copy()
    with np.errstate(all="ignore"):
        return ((x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)).astype(np.float32)


def seam_crossing_window_rows(lengths, horizon):
    """Mutant: the windows of ONE long rollout of the same rows (starts that run over rollout seams)."""
    total = int((np.asarray(lengths, np.int64) + 1).sum())
    return np.arange(max(0, total - 1 - horizon), dtype=np.int64)


def stacked_reference(dataset, **mutant):
    """(ins, outs) of dataset.stacked() from the store layout: float32 rollouts, the dataset's statistics."""
    lengths = [len(r) for r in dataset.rollouts]
    store = store_from_rollouts(dataset.rollouts)
    if mutant.get("seam"):
        win_row = seam_crossing_window_rows(lengths, dataset.horizon)
    else:
        win_row = window_rows(lengths, dataset.horizon)[0]
    ins, outs = mode_fields(dataset._data_mode)

    def one(field, shift):
        st = dataset.statistics[field] if dataset._normalise else None
        mean = None if st is None else st["mean"].reshape(-1).numpy()
        std = None if st is None else st["std"].reshape(-1).numpy()
        return stack_reference(store[field], mean, std, win_row, dataset.horizon, shift,
                               ignore_shift=mutant.get("ignore_shift", False))
    return tuple(one(*f) for f in ins), tuple(one(*f) for f in outs)


def ordered_sum(x):
    """Column sums of float64 x [R][dim] in mbrl_dataset_stats' order: chunks of 1024 positions (absent ones +0.0),
    lane t of 256 forms ((x[4t] + x[4t+1]) + x[4t+2]) + x[4t+3], the pairwise tree d = 128 .. 1, then the chunk
    partials by mbrl_eval_members' rule (lane t of 1024 adds t, t + 1024, .. ascending, tree d = 512 .. 1)."""
    x = np.asarray(x, np.float64)
    R, dim = x.shape
    chunks = -(-R // 1024)
    padded = np.zeros((chunks * 1024, dim))
    padded[:R] = x
    v = padded.reshape(chunks, 256, 4, dim)
    lane = ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]) + v[:, :, 3]
    d = 128
    while d >= 1:
        lane = lane[:, :d] + lane[:, d:2 * d]
        d //= 2
    part = lane[:, 0]
    turns = -(-chunks // 1024)
    padded = np.zeros((turns * 1024, dim))
    padded[:chunks] = part
    acc = np.zeros((1024, dim))
    for k in range(turns):
        acc = acc + padded[k * 1024:(k + 1) * 1024]
    d = 512
    while d >= 1:
        acc = acc[:d] + acc[d:2 * d]
        d //= 2
    return acc[0]


def stats_reference(src, rows, biased=False, rounded_mean=False):
    """(mean, std, min, max) float32 [dim] over src[rows], as mbrl_dataset_stats defines them. Mutants: `biased`
    divides by R, `rounded_mean` takes the fp32 mean into the second pass."""
    x32 = np.asarray(src, np.float32)[np.asarray(rows, np.int64)]
    x = x32.astype(np.float64)
    R = len(x)
    with np.errstate(all="ignore"):
        mean64 = ordered_sum(x) / R
        centre = mean64.astype(np.float32).astype(np.float64) if rounded_mean else mean64
        dev = x - centre
        ss = ordered_sum(dev * dev)
        std = np.sqrt(ss / (R if biased else R - 1))
        return mean64.astype(np.float32), std.astype(np.float32), np.min(x32, axis=0), np.max(x32, axis=0)


def ulps32(got, want64):
    """|got - want| in units of the fp32 spacing at want (want in float64)."""
    want64 = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)


__all__ = ["make_rollouts", "store_from_rollouts", "stack_reference", "stacked_reference", "ordered_sum",
           "stats_reference", "ulps32", "seam_crossing_window_rows", "PAD", "rollout_first_rows", "stat_rows",
           "window_rows"]
