"""Device-resident transitions, the host side (no GPU): the NumPy restatement of the step-store layout, the
window gather and the float64 summation order (tests/dataset_reference.py) is pinned to TransitionsDataset, and
every single-mistake mutant of it is told from the real thing. tests/test_gpu_dataset.py then holds the kernels
to the restatement bit for bit."""
import numpy as np
import pytest
import torch

import dataset_reference as ref
from mbrl_amd.data import TransitionsDataset
from mbrl_amd.device_data import stat_rows, window_rows

MODES = ("both", "state_only", "obs_only")


def lengths_for(horizon):
    """Unequal lengths; one rollout of exactly horizon + 1 steps; rollouts with no window (K = horizon, and
    K < horizon where that leaves a transition)."""
    out = [9, horizon + 1, horizon, 4 + horizon, 7]
    if horizon > 1:
        out.insert(2, horizon - 1)
    return out


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def parent_stacked(ds):
    _, ins, outs = ds.stacked("cpu")
    return tuple(t.numpy() for t in ins), tuple(t.numpy() for t in outs)


def all_same(got, want):
    return all(same_bytes(g, w) for part_g, part_w in zip(got, want) for g, w in zip(part_g, part_w))


@pytest.mark.parametrize("horizon", [1, 2, 5])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("normalise", [True, False])
def test_window_restatement_equals_the_parents_stacked(horizon, mode, normalise):
    ds = TransitionsDataset(ref.make_rollouts(lengths_for(horizon), seed=horizon), horizon=horizon,
                            normalise=normalise, data_mode=mode)
    want = parent_stacked(ds)
    got = ref.stacked_reference(ds)
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1])
    assert all_same(got, want)


@pytest.mark.parametrize("horizon", [1, 2])
def test_window_restatement_after_an_eviction_that_slices_the_oldest_rollout(horizon, capsys):
    rollouts = ref.make_rollouts([8, 6, 5], seed=3)
    ds = TransitionsDataset(rollouts[:2], transitions_capacity=14, horizon=horizon)
    ds.add_rollouts(rollouts[2:])
    assert len(ds.rollouts[0]) < 8 and ds.num_rollouts == 3      # the oldest one lost its head
    assert all_same(ref.stacked_reference(ds), parent_stacked(ds))


@pytest.mark.parametrize("horizon", [1, 2, 5])
def test_window_rows_address_transition_indexs_windows_in_its_order(horizon):
    lengths = lengths_for(horizon)
    ds = TransitionsDataset(ref.make_rollouts(lengths, seed=1), horizon=horizon)
    win_row, roll, start = window_rows(lengths, horizon)
    assert list(zip(roll.tolist(), start.tolist())) == ds.transition_index()
    assert len(win_row) == ds.num_transitions()
    first = ref.rollout_first_rows(lengths)
    assert np.array_equal(win_row, first[roll] + start)
    # every row a window reads lies inside its own rollout
    assert np.all(start + horizon <= np.asarray(lengths)[roll])


def test_row_lists_reproduce_the_parents_exclusions():
    lengths = [9, 1, 4, 7]
    rollouts = ref.make_rollouts(lengths, dtype=torch.float64, seed=5)
    ds = TransitionsDataset(rollouts)
    store = ref.store_from_rollouts(rollouts, dtype=np.float64)
    lists = stat_rows(lengths)
    assert len(lists["actions"]) == sum(lengths) == len(lists["rewards"])
    for f in ref.FIELDS:
        got = store[f][lists[f]].mean(axis=0)
        want = ds.statistics[f]["mean"].reshape(-1).numpy()
        assert np.allclose(got, want, rtol=1e-12, atol=0), f
        assert not np.any(store[f][lists[f]] == ref.PAD), f
    # mutant: the action list taken for the rewards reads a padding row and misses the parent's mean
    wrong = store["rewards"][lists["actions"]].mean(axis=0)
    assert not np.allclose(wrong, ds.statistics["rewards"]["mean"].reshape(-1).numpy(), rtol=1e-12, atol=0)
    # mutant: padding read as a value
    every = store["actions"].mean(axis=0)
    assert not np.allclose(every, ds.statistics["actions"]["mean"].reshape(-1).numpy(), rtol=1e-12, atol=0)


def torch_stats64(x32):
    x = torch.from_numpy(x32.astype(np.float64))
    return x.mean(dim=0).numpy(), x.std(dim=0).numpy(), x.min(dim=0).values.numpy(), x.max(dim=0).values.numpy()


@pytest.mark.parametrize("R", [2, 3, 1023, 1024, 1025, 4099, 1024 * 1024 + 1])
def test_summation_order_lies_within_one_ulp_of_float64(R):
    rng = np.random.default_rng(R)
    dim = 1 if R > 100000 else 6
    src = (rng.standard_normal((R + 5, dim)) * np.arange(1, dim + 1) + np.arange(dim)).astype(np.float32)
    src[:, -1] = 2.5 if dim > 1 else src[:, -1]                  # a constant column beside ordinary ones
    rows = rng.permutation(R + 5)[:R]
    if R > 3:
        rows[R // 2] = rows[0]                                    # a repeated row
    mean, std, lo, hi = ref.stats_reference(src, rows)
    m64, s64, lo64, hi64 = torch_stats64(src[rows])
    ordinary = slice(0, dim - 1) if dim > 1 else slice(0, 1)
    assert np.all(s64[ordinary] >= 1e-3 * np.abs(src[rows][:, ordinary]).max(axis=0))
    assert np.all(ref.ulps32(mean[ordinary], m64[ordinary]) <= 1.0)
    assert np.all(ref.ulps32(std[ordinary], s64[ordinary]) <= 1.0)
    assert np.array_equal(lo, lo64.astype(np.float32)) and np.array_equal(hi, hi64.astype(np.float32))
    if dim > 1:
        assert mean[-1] == np.float32(2.5) and std[-1] == 0.0 and lo[-1] == hi[-1] == np.float32(2.5)
    # mutant: the biased estimator misses the bar
    biased = ref.stats_reference(src, rows, biased=True)[1]
    if R <= 4099:
        assert np.any(ref.ulps32(biased[ordinary], s64[ordinary]) > 1.0)


def test_single_row_nan_and_inf_columns():
    src = np.array([[1.0, 2.0, 3.0], [4.0, np.nan, np.inf], [7.0, 8.0, 9.0]], np.float32)
    mean, std, lo, hi = ref.stats_reference(src, [0, 1, 2])
    assert mean[0] == 4.0 and std[0] == 3.0 and lo[0] == 1.0 and hi[0] == 7.0
    assert all(np.isnan(v[1]) for v in (mean, std, lo, hi))
    assert np.isposinf(mean[2]) and np.isnan(std[2]) and lo[2] == 3.0 and np.isposinf(hi[2])
    x = torch.from_numpy(src)
    assert np.array_equal(mean, x.mean(dim=0).numpy(), equal_nan=True)
    assert np.array_equal(std, x.std(dim=0).numpy(), equal_nan=True)
    assert np.array_equal(lo, x.min(dim=0).values.numpy(), equal_nan=True)
    assert np.array_equal(hi, x.max(dim=0).values.numpy(), equal_nan=True)
    one = ref.stats_reference(src, [2])
    assert np.array_equal(one[0], src[2]) and np.all(np.isnan(one[1]))      # R = 1: std = NaN, as torch.std


def test_mutant_rounded_mean_changes_the_bytes():
    """A mean rounded to fp32 before the second pass shows where the mean is large beside the spread."""
    rng = np.random.default_rng(7)
    src = (1000.0 + 0.01 * rng.standard_normal((4099, 8))).astype(np.float32)
    rows = np.arange(4099)
    good = ref.stats_reference(src, rows)[1]
    assert np.all(ref.ulps32(good, torch_stats64(src)[1]) <= 1.0)
    assert not same_bytes(good, ref.stats_reference(src, rows, rounded_mean=True)[1])


@pytest.mark.parametrize("mutant", ["ignore_shift", "seam"])
def test_mutant_windows_miss_the_byte_comparison(mutant):
    ds = TransitionsDataset(ref.make_rollouts([6, 5, 7], seed=2), horizon=2)
    want = parent_stacked(ds)
    assert all_same(ref.stacked_reference(ds), want)
    got = ref.stacked_reference(ds, **{mutant: True})
    assert not all(g.shape == w.shape and same_bytes(g, w) for g, w in zip(got[1], want[1]))


def test_device_dataset_rejects_dict_observations():
    from mbrl_amd import DeviceTransitionsDataset
    from mbrl_amd.data import Rollout
    roll = Rollout(states=[torch.zeros(2)] * 3, observations=[{"x": torch.zeros(2)}] * 3,
                   actions=[torch.zeros(1)] * 2, rewards=[torch.zeros(())] * 2)
    with pytest.raises(ValueError):
        DeviceTransitionsDataset([roll], device="cuda:0")
