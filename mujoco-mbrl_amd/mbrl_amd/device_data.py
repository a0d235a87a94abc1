"""Device-resident transitions: TransitionsDataset with its steps in GPU memory.

`TransitionsDataset.stacked(device)` builds the training tensors with one `self[t]` per transition and
one torch.stack per step, and `add_rollouts` recomputes the statistics on the host; both are linear
in the dataset and paid again after every `add_rollouts` of an online loop. DeviceTransitionsDataset
keeps the parent's host rollout list and all of its bookkeeping (capacity eviction, `__len__`,
`num_transitions()`, `transition_index()`, `__getitem__`, data modes, `normalizers()`) and adds a
step store on the device (include/mbrl_cem.h, "device-resident transitions"):

  - one fp32 array [S][dim] per field (states, observations, actions, rewards); a rollout with K
    transitions holds K + 1 consecutive rows, row k = (s_k, o_k, a_k, r_k); the action of its last
    row and the reward of its first row are padding;
  - `add_rollouts` uploads the new rollouts' rows only (one host-to-device copy per field), drops
    evicted rows from the front, and recomputes `statistics` with mbrl_dataset_stats over row lists
    that reproduce the parent's exclusions;
  - `stacked(device)` issues one mbrl_dataset_stack launch for all fields of the data mode.

The row arithmetic is vectorised NumPy (`window_rows`, `stat_rows`: no Python loop over transitions or
steps; tests/test_dataset_host.py pins both to the parent). Storage is float32: for float64 rollouts
the statistics and the stacked tensors equal the parent's on rollouts cast to float32 first (the
parent normalises in float64 and rounds once at the end).
"""
import numpy as np
import torch

from . import _lib
from .data import TransitionsDataset, TransitionsDatasetDataMode

FIELDS = ("states", "observations", "actions", "rewards")


def rollout_first_rows(lengths):
    """The store row of each rollout's step 0: a rollout with K transitions occupies K + 1 rows."""
    rows = np.asarray(lengths, np.int64) + 1
    return np.cumsum(rows) - rows


def window_rows(lengths, horizon):
    """(win_row, roll_idx, start_idx), int64 [T] each: the store row of step 0 of every window, in
    `transition_index()`'s order -- rollout r has max(0, K_r - horizon) windows, starts ascending."""
    lengths = np.asarray(lengths, np.int64)
    count = np.maximum(lengths - int(horizon), 0)
    roll = np.repeat(np.arange(len(lengths), dtype=np.int64), count)
    start = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    return rollout_first_rows(lengths)[roll] + start, roll, start


def stat_rows(lengths):
    """The row lists of the statistics: every row for states and observations, all but each rollout's
    last row for actions, all but each rollout's first row for rewards (data.py _update_stats)."""
    lengths = np.asarray(lengths, np.int64)
    first = rollout_first_rows(lengths)
    rows = np.arange(int((lengths + 1).sum()), dtype=np.int64)
    return {"states": rows, "observations": rows, "actions": np.delete(rows, first + lengths),
            "rewards": np.delete(rows, first)}


def mode_fields(data_mode):
    """((field, shift), ..) of the inputs and of the outputs that `__getitem__` yields in `data_mode`."""
    mode = TransitionsDatasetDataMode(data_mode)
    if mode == TransitionsDatasetDataMode.state_only:
        return (("states", 0), ("actions", 0)), (("rewards", 1), ("states", 1))
    if mode == TransitionsDatasetDataMode.obs_only:
        return (("observations", 0), ("actions", 0)), (("rewards", 1), ("observations", 1))
    return ((("states", 0), ("observations", 0), ("actions", 0)),
            (("rewards", 1), ("states", 1), ("observations", 1)))


def _resolve(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def dataset_stack(fields, win_row, horizon):
    """mbrl_dataset_stack on the current stream: fields = [(src [S][dim], mean|None, std|None, shift)];
    returns the new [T][horizon][dim] tensors."""
    lib = _lib.load()
    T = win_row.numel()
    table = (_lib.StackField * len(fields))()
    outs = []
    for i, (src, mean, std, shift) in enumerate(fields):
        dst = torch.empty((T, horizon, src.shape[1]), dtype=torch.float32, device=src.device)
        table[i] = _lib.StackField(src.data_ptr(), None if mean is None else mean.data_ptr(),
                                   None if std is None else std.data_ptr(), dst.data_ptr(), src.shape[1], shift)
        outs.append(dst)
    _lib.check(lib.mbrl_dataset_stack(table, len(fields), _lib.ptr(win_row), T, horizon,
                                      _lib.stream_handle(win_row.device)), "mbrl_dataset_stack")
    return outs


def dataset_stats(fields):
    """mbrl_dataset_stats on the current stream: fields = [(src [S][dim], rows int64 [R])] (up to 4);
    returns one [4][dim] device tensor (mean, std, min, max) per field."""
    lib = _lib.load()
    table = (_lib.StatsField * len(fields))()
    outs = []
    for i, (src, rows) in enumerate(fields):
        out = torch.empty((4, src.shape[1]), dtype=torch.float32, device=src.device)
        table[i] = _lib.StatsField(src.data_ptr(), rows.data_ptr(), rows.numel(), out[0].data_ptr(),
                                   out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), src.shape[1], 0)
        outs.append(out)
    need = lib.mbrl_dataset_stats_workspace_bytes(table, len(fields))
    if need == 0:
        _lib.check(_lib.MBRL_EINVAL, "mbrl_dataset_stats_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=fields[0][0].device)
    _lib.check(lib.mbrl_dataset_stats(table, len(fields), _lib.ptr(ws), need,
                                      _lib.stream_handle(ws.device)), "mbrl_dataset_stats")
    return outs


class DeviceTransitionsDataset(TransitionsDataset):
    """TransitionsDataset whose steps live on `device` (flat observations only): the parent's
    constructor arguments, interface and bookkeeping; `statistics` and `stacked(device)` come from the
    HIP kernels. `stacked()` for another device falls back to the parent's host path."""

    def __init__(self, rollouts=None, transitions_capacity=int(1e6), horizon=1, normalise=True,
                 data_mode=TransitionsDatasetDataMode.both, device="cuda"):
        self._device = _resolve(device)
        self._store = None          # field -> [S][dim] fp32 on the device
        self._row_lens = []         # store rows per rollout, oldest first
        self._elem = None           # field -> (element shape, dtype) of the rollouts' values
        self._dev_stats = None      # field -> [4][dim] (mean, std, min, max) on the device
        self._pending = []
        super().__init__(rollouts, transitions_capacity, horizon, normalise, data_mode)

    device = property(lambda self: self._device)

    def add_rollouts(self, rollouts):
        if not all(r.flat_observations for r in rollouts):
            raise ValueError("DeviceTransitionsDataset needs flat (tensor) observations")
        self._pending = list(rollouts)
        try:
            super().add_rollouts(rollouts)      # the parent's bookkeeping; it ends in _update_stats()
        finally:
            self._pending = []

    def _upload(self, rollouts):
        """The new rollouts' rows, cast to float32: one host array and one copy per field."""
        lens = [len(r) + 1 for r in rollouts]
        first = np.cumsum(lens) - np.asarray(lens)
        r0 = rollouts[0]
        if self._elem is None:
            self._elem = {"states": (r0.states[0].shape, r0.states[0].dtype),
                          "observations": (r0.observations[0].shape, r0.observations[0].dtype),
                          "actions": (r0.actions[0].shape, r0.actions[0].dtype),
                          "rewards": (torch.as_tensor(r0.rewards[1]).shape, torch.as_tensor(r0.rewards[1]).dtype)}
        host = {f: torch.zeros((sum(lens), max(1, int(np.prod(self._elem[f][0])))), dtype=torch.float32)
                for f in FIELDS}
        for r, at in zip(rollouts, first.tolist()):
            n = len(r) + 1
            host["states"][at:at + n] = torch.stack(list(r.states)).reshape(n, -1)
            host["observations"][at:at + n] = torch.stack(list(r.observations)).reshape(n, -1)
            host["actions"][at:at + n - 1] = torch.stack(list(r.actions[:-1])).reshape(n - 1, -1)
            host["rewards"][at + 1:at + n] = torch.stack(list(r.rewards[1:])).reshape(n - 1, -1)
        new = {f: host[f].to(self._device) for f in FIELDS}
        self._store = new if self._store is None else {f: torch.cat((self._store[f], new[f])) for f in FIELDS}
        self._row_lens += lens

    def _update_stats(self):
        with torch.cuda.device(self._device):
            if self._pending:
                self._upload(self._pending)
            # what the parent evicted: whole rollouts from the front, then the head of the oldest one left
            gone = len(self._row_lens) - len(self._rollouts)
            drop = sum(self._row_lens[:gone])
            del self._row_lens[:gone]
            if self._row_lens:
                head = self._row_lens[0] - (len(self._rollouts[0]) + 1)
                drop += head
                self._row_lens[0] -= head
            if drop:
                self._store = {f: t[drop:] for f, t in self._store.items()}
            lists = stat_rows(np.asarray(self._row_lens, np.int64) - 1)
            order = ("states", "actions", "rewards")     # states and observations share one list
            dev = torch.from_numpy(np.concatenate([lists[f] for f in order])).to(self._device)
            ends = np.cumsum([len(lists[f]) for f in order])
            rows = {f: dev[e - len(lists[f]):e] for f, e in zip(order, ends.tolist())}
            rows["observations"] = rows["states"]
            outs = dataset_stats([(self._store[f], rows[f]) for f in FIELDS])
            self._dev_stats = dict(zip(FIELDS, outs))
            host = torch.cat(outs, dim=1).cpu()
        at = 0
        for f in FIELDS:
            shape, dtype = self._elem[f]
            dim = outs[FIELDS.index(f)].shape[1]
            self._stats[f] = {k: host[i, at:at + dim].reshape(shape).to(dtype)
                              for i, k in enumerate(("mean", "std", "min", "max"))}
            at += dim

    def stacked(self, device):
        """The parent's (index, inputs, outputs), from one mbrl_dataset_stack launch; the parent's host
        path for a device other than the dataset's."""
        key = str(device)
        if self._stacked is not None and self._stacked[0] == key:
            return self._stacked[1:]
        if _resolve(device) != self._device or self._store is None:
            return super().stacked(device)
        win_row, roll, start = window_rows(np.asarray(self._row_lens, np.int64) - 1, self.horizon)
        if len(win_row) == 0:
            return super().stacked(device)
        index = list(zip(roll.tolist(), start.tolist()))
        ins, outs = mode_fields(self._data_mode)
        with torch.cuda.device(self._device):
            table = []
            for f, shift in ins + outs:
                st = self._dev_stats[f] if self._normalise else None
                table.append((self._store[f], None if st is None else st[0], None if st is None else st[1], shift))
            res = dataset_stack(table, torch.from_numpy(win_row).to(self._device), self.horizon)
        ins, outs = tuple(res[:len(ins)]), tuple(res[len(ins):])
        self._stacked = (key, index, ins, outs)
        return index, ins, outs


__all__ = ["DeviceTransitionsDataset", "window_rows", "stat_rows", "rollout_first_rows", "mode_fields",
           "dataset_stack", "dataset_stats", "FIELDS"]
