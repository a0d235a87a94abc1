"""Device-resident transitions on the GPU: mbrl_dataset_stack and mbrl_dataset_stats against the NumPy
restatement (tests/dataset_reference.py, pinned to TransitionsDataset by tests/test_dataset_host.py) bit for bit,
their argument checks, and DeviceTransitionsDataset against a host TransitionsDataset on the same rollouts:
statistics, stacked tensors, training, planning and the fallback."""
import copy

import numpy as np
import pytest
import torch

import dataset_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (1, 3, 17, 67)


def _lib():
    from mbrl_amd import _lib
    return _lib


def _offset(array, k):
    """`array` on the device in a buffer that starts 4 * k bytes past an allocation's alignment."""
    flat = torch.empty(array.size + 4, dtype=torch.float32, device=DEV)
    view = flat[k:k + array.size].view(array.shape)
    view.copy_(torch.from_numpy(array))
    assert view.data_ptr() % 16 == (4 * k) % 16
    return view


def _stack_call(fields, win_row, T, horizon):
    L = _lib()
    table = (L.StackField * max(1, len(fields)))()
    for i, f in enumerate(fields):
        table[i] = L.StackField(*f)
    return L.load().mbrl_dataset_stack(table, len(fields), win_row, T, horizon, L.stream_handle(0))


def _same(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- mbrl_dataset_stack

@pytest.mark.parametrize("T", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("horizon", [1, 2, 5, 30])
def test_stack_is_bit_equal_to_the_restatement(T, horizon):
    """Every dim and both shifts at this (T, horizon), as launches of 8, 4 and 1 fields; sources, statistics and
    destinations at 4-byte offsets; with and without statistics; the destinations start as NaN."""
    rng = np.random.default_rng(1000 * T + horizon)
    S = T + horizon + 7
    win_row_h = rng.integers(0, S - horizon - 1, size=T).astype(np.int64)
    win_row_h[0] = S - horizon - 1                       # the last window the store can hold (shift 1: its last row)
    win_row = torch.from_numpy(win_row_h).to(DEV)
    cases = []                                           # (src host, mean, std, shift, offset k)
    for i, dim in enumerate(DIMS):
        src = (rng.standard_normal((S, dim)) * 3 + 1).astype(np.float32)
        mean = rng.standard_normal(dim).astype(np.float32)
        std = rng.uniform(0.5, 2.0, dim).astype(np.float32)
        for shift in (0, 1):
            cases.append((src, mean, std, shift, (i + 2 * shift + 1) % 4))
    launches = [cases, cases[1::2], cases[4:5], [(c[0], None, None, c[3], c[4]) for c in cases[:4]]]
    for group in launches:
        keep, table, dsts = [], [], []
        for src, mean, std, shift, k in group:
            d_src = _offset(src, k)
            d_mean = None if mean is None else _offset(mean, (k + 1) % 4)
            d_std = None if std is None else _offset(std, (k + 2) % 4)
            dst = _offset(np.full((T, horizon, src.shape[1]), np.nan, np.float32), (k + 3) % 4)
            keep += [d_src, d_mean, d_std]
            dsts.append(dst)
            table.append((d_src.data_ptr(), None if mean is None else d_mean.data_ptr(),
                          None if std is None else d_std.data_ptr(), dst.data_ptr(), src.shape[1], shift))
        rc = _stack_call(table, win_row.data_ptr(), T, horizon)
        assert rc == 0, _lib().load().mbrl_last_error()
        torch.cuda.synchronize()
        for (src, mean, std, shift, _), dst in zip(group, dsts):
            got = dst.cpu().numpy()
            assert not np.isnan(got).any()               # every element was written
            assert _same(got, ref.stack_reference(src, mean, std, win_row_h, horizon, shift)), (src.shape[1], shift)


def test_stack_argument_errors_leave_the_outputs_alone():
    L = _lib()
    T, H, dim = 10, 2, 3
    src = torch.randn(T + H + 1, dim, device=DEV)
    stat = torch.ones(dim, device=DEV)
    dst = torch.full((T, H, dim), float("nan"), device=DEV)
    win = torch.arange(T, dtype=torch.int64, device=DEV)
    ok = (src.data_ptr(), stat.data_ptr(), stat.data_ptr(), dst.data_ptr(), dim, 0)

    def f(**kw):
        d = dict(zip(("src", "mean", "std", "dst", "dim", "shift"), ok))
        d.update(kw)
        return tuple(d[k] for k in ("src", "mean", "std", "dst", "dim", "shift"))
    W = win.data_ptr()
    EINVAL, EUNSUP = L.MBRL_EINVAL, L.MBRL_EUNSUPPORTED
    cases = [
        ([f(src=None)], W, T, H, EINVAL), ([f(dst=None)], W, T, H, EINVAL), ([f(mean=None)], W, T, H, EINVAL),
        ([f(std=None)], W, T, H, EINVAL), ([f()], None, T, H, EINVAL), ([], W, T, H, EINVAL),
        ([f()] * 9, W, T, H, EINVAL), ([f()], W, 0, H, EINVAL), ([f()], W, T, 0, EINVAL),
        ([f(dim=0)], W, T, H, EINVAL), ([f(shift=2)], W, T, H, EINVAL), ([f(shift=-1)], W, T, H, EINVAL),
        ([f(), f(dim=-3)], W, T, H, EINVAL),
        ([f()], W, (1 << 31) // (H * dim) + 1, H, EUNSUP),          # T * horizon * dim >= 2^31, small buffers
        ([f()], W, 1 << 40, H, EUNSUP),
    ]
    for fields, w, t, h, want in cases:
        assert _stack_call(fields, w, t, h) == want, (fields, t, h)
        assert L.load().mbrl_last_error()
    L2 = L.load()
    assert L2.mbrl_dataset_stack(None, 1, W, T, H, L.stream_handle(0)) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()
    assert _stack_call([f()], W, T, H) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(dst).any()


# ---- mbrl_dataset_stats

def _stats_call(fields, fill=None, ws_bytes=None, ws_none=False):
    """fields: [(src device, rows device, dim)]; returns (rc, [out [4][dim] device])."""
    L = _lib()
    lib = L.load()
    table = (L.StatsField * max(1, len(fields)))()
    outs = []
    for i, (src, rows, dim) in enumerate(fields):
        out = torch.full((4, max(dim, 1)), 12345.0, device=DEV)
        table[i] = L.StatsField(None if src is None else src.data_ptr(), None if rows is None else rows.data_ptr(),
                                0 if rows is None else rows.numel(), out[0].data_ptr(), out[1].data_ptr(),
                                out[2].data_ptr(), out[3].data_ptr(), dim, 0)
        outs.append(out)
    need = lib.mbrl_dataset_stats_workspace_bytes(table, len(fields))
    ws = torch.zeros(max(need, 64) + 8, dtype=torch.uint8, device=DEV)
    if fill == "nan":
        ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    elif fill == "ff":
        ws.fill_(255)
    rc = lib.mbrl_dataset_stats(table, len(fields), None if ws_none else ws.data_ptr(),
                                need if ws_bytes is None else ws_bytes, L.stream_handle(0))
    torch.cuda.synchronize()
    return rc, outs, need


def _stats_case(R, dim, seed, special=False):
    rng = np.random.default_rng(seed)
    S = min(R, 5000) + 11
    src = (rng.standard_normal((S, dim)) * np.linspace(0.1, 30.0, dim) + np.linspace(-5.0, 5.0, dim)).astype(np.float32)
    if special:                                          # a NaN, an inf and a constant column beside ordinary ones
        src[:, 2] = np.float32(-7.25)
        src[S // 3, 5] = np.nan
        src[S // 2, 9] = np.inf
    rows = rng.integers(0, S, size=R).astype(np.int64)   # unsorted, repeated
    if special:
        rows[-1], rows[0] = S // 3, S // 2               # the NaN in the last chunk's tail, the inf in the first lane
    return src, rows


def _assert_stats(out, src, rows):
    got = out.cpu().numpy()
    want = ref.stats_reference(src, rows)
    for name, g, w in zip(("mean", "std", "min", "max"), got, want):
        assert np.array_equal(g, w, equal_nan=True), (name, np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])


@pytest.mark.parametrize("R", [1, 2, 3, 1023, 1024, 1025, 4099])
@pytest.mark.parametrize("dim", [1, 17, 1024])
def test_stats_are_bit_equal_to_the_restatement(R, dim):
    src, rows = _stats_case(R, dim, seed=R * 7 + dim, special=(dim == 17 and R >= 3))
    d_src, d_rows = _offset(src, 1 + dim % 3), torch.from_numpy(rows).to(DEV)
    for fill in ("nan", "ff"):
        rc, outs, _ = _stats_call([(d_src, d_rows, dim)], fill=fill)
        assert rc == 0, _lib().load().mbrl_last_error()
        _assert_stats(outs[0], src, rows)
    if dim == 17 and R >= 3:
        got = outs[0].cpu().numpy()
        assert np.isnan(got[:, 5]).all() and np.isposinf(got[0, 9]) and np.isnan(got[1, 9]) and np.isposinf(got[3, 9])
        assert got[0, 2] == np.float32(-7.25) and got[1, 2] == 0.0 and got[2, 2] == got[3, 2] == np.float32(-7.25)
    if R == 1:
        assert np.isnan(outs[0][1].cpu().numpy()).all()  # std of one row, as torch.std


def test_stats_the_1025th_partial():
    R = 1024 * 1024 + 1
    src, rows = _stats_case(R, 1, seed=4)
    rc, outs, _ = _stats_call([(torch.from_numpy(src).to(DEV), torch.from_numpy(rows).to(DEV), 1)], fill="ff")
    assert rc == 0
    _assert_stats(outs[0], src, rows)


def test_stats_fields_together_equal_each_alone():
    a_src, a_rows = _stats_case(1025, 17, seed=11, special=True)
    b_src, b_rows = _stats_case(300, 3, seed=12)
    A = (torch.from_numpy(a_src).to(DEV), torch.from_numpy(a_rows).to(DEV), 17)
    B = (_offset(b_src, 3), torch.from_numpy(b_rows).to(DEV), 3)
    rc, both, _ = _stats_call([A, B, A, B], fill="nan")
    assert rc == 0
    for one, got in ((A, both[0]), (B, both[1]), (A, both[2]), (B, both[3])):
        rc, alone, _ = _stats_call([one], fill="ff")
        assert rc == 0
        assert np.array_equal(got.cpu().numpy(), alone[0].cpu().numpy(), equal_nan=True)
    _assert_stats(both[0], a_src, a_rows)
    _assert_stats(both[1], b_src, b_rows)


def test_stats_argument_errors():
    L = _lib()
    src = torch.randn(20, 3, device=DEV)
    rows = torch.arange(10, dtype=torch.int64, device=DEV)
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    good = (src, rows, 3)
    for fields, kw, want in [
        ([(None, rows, 3)], {}, L.MBRL_EINVAL), ([(src, None, 3)], {}, L.MBRL_EINVAL),
        ([(src, empty, 3)], {}, L.MBRL_EINVAL), ([], {}, L.MBRL_EINVAL), ([good] * 5, {}, L.MBRL_EINVAL),
        ([good], {"ws_none": True}, L.MBRL_EINVAL),
        ([(src, rows, 0)], {}, L.MBRL_EUNSUPPORTED), ([(src, rows, 1025)], {}, L.MBRL_EUNSUPPORTED),
        ([good, (src, rows, -1)], {}, L.MBRL_EUNSUPPORTED),
    ]:
        rc, outs, _ = _stats_call(fields, **kw)
        assert rc == want, (fields, kw)
        assert all(bool((o == 12345.0).all()) for o in outs)
    rc, outs, need = _stats_call([good])
    assert rc == 0 and need > 0
    rc, outs, _ = _stats_call([good], ws_bytes=need - 1)
    assert rc == L.MBRL_EWORKSPACE and bool((outs[0] == 12345.0).all())
    lib = L.load()
    assert lib.mbrl_dataset_stats(None, 1, src.data_ptr(), 1 << 20, L.stream_handle(0)) == L.MBRL_EINVAL
    assert lib.mbrl_dataset_stats_workspace_bytes(None, 1) == 0


# ---- DeviceTransitionsDataset

S_DIM, A_DIM = 6, 2


def _pair(lengths, horizon=1, mode="both", normalise=True, capacity=int(1e6), seed=0):
    """A device dataset and a host TransitionsDataset on the same rollouts with the device dataset's statistics."""
    from mbrl_amd import DeviceTransitionsDataset
    from mbrl_amd.data import TransitionsDataset
    rollouts = ref.make_rollouts(lengths, s=S_DIM, o=S_DIM, a=A_DIM, seed=seed)
    dev = DeviceTransitionsDataset(rollouts, transitions_capacity=capacity, horizon=horizon, normalise=normalise,
                                   data_mode=mode, device=DEV)
    host = TransitionsDataset(rollouts, transitions_capacity=capacity, horizon=horizon, normalise=normalise,
                              data_mode=mode)
    return dev, _with_stats(host, dev)


def _with_stats(host, dev):
    host._stats = dict(dev.statistics)      # a copy: the host's own add_rollouts must not write into dev's
    host._stacked = None
    return host


def _assert_statistics_close(dev):
    """Within one fp32 ulp of the parent's statistics on float64 copies of the rollouts (the bar
    tests/test_dataset_host.py derives), on columns whose std is at least 1e-3 of their largest |x|."""
    from mbrl_amd.data import Rollout, TransitionsDataset
    wide = [Rollout(states=[x.double() for x in r.states], observations=[x.double() for x in r.observations],
                    actions=[x.double() for x in r.actions[:-1]], rewards=[x.double() for x in r.rewards[1:]])
            for r in dev.rollouts]
    want = TransitionsDataset(wide).statistics
    for f in ref.FIELDS:
        got = dev.statistics[f]
        assert set(got) == {"mean", "std", "min", "max"}
        for k in got:
            assert got[k].shape == want[f][k].shape and got[k].dtype == torch.float32 and not got[k].is_cuda
        big = np.maximum(np.abs(want[f]["min"].numpy()), np.abs(want[f]["max"].numpy()))
        assert np.all(want[f]["std"].numpy() >= 1e-3 * big)
        assert np.all(ref.ulps32(got["mean"].numpy(), want[f]["mean"].numpy()) <= 1.0), f
        assert np.all(ref.ulps32(got["std"].numpy(), want[f]["std"].numpy()) <= 1.0), f
        assert np.array_equal(got["min"].numpy(), want[f]["min"].numpy().astype(np.float32))
        assert np.array_equal(got["max"].numpy(), want[f]["max"].numpy().astype(np.float32))


def _assert_stacked_equal(dev, host):
    index, ins, outs = dev.stacked(DEV)
    h_index, h_ins, h_outs = host.stacked(DEV)
    assert index == h_index == dev.transition_index()
    assert len(ins) == len(h_ins) and len(outs) == len(h_outs)
    for got, want in zip(ins + outs, h_ins + h_outs):
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous()
        assert _same(got.cpu().numpy(), want.cpu().numpy())
    assert dev.stacked(DEV)[1][0] is ins[0]               # cached, as the parent's


def test_device_dataset_statistics_after_adds_and_an_eviction(capsys):
    from mbrl_amd import DeviceTransitionsDataset
    from mbrl_amd.data import TransitionsDataset
    rollouts = ref.make_rollouts([40, 25, 33, 30], s=S_DIM, o=S_DIM, a=A_DIM, seed=21)
    dev = DeviceTransitionsDataset(rollouts[:2], transitions_capacity=100, horizon=2, device=DEV)
    host = TransitionsDataset(rollouts[:2], transitions_capacity=100, horizon=2)
    _assert_statistics_close(dev)
    _assert_stacked_equal(dev, _with_stats(host, dev))
    dev.add_rollouts(rollouts[2:3])
    host.add_rollouts(rollouts[2:3])
    _assert_statistics_close(dev)
    _assert_stacked_equal(dev, _with_stats(host, dev))
    dev.add_rollouts(rollouts[3:])                        # over capacity: the oldest rollout loses its head
    host.add_rollouts(rollouts[3:])
    assert len(dev) == len(host) == 100 and len(dev.rollouts[0]) == len(host.rollouts[0]) < 40
    assert dev.num_transitions() == host.num_transitions()
    _assert_statistics_close(dev)
    _assert_stacked_equal(dev, _with_stats(host, dev))
    norm = dev.normalizers(reward=True)
    x = torch.randn(S_DIM)
    assert torch.equal(norm["normalize_state"](x), (x - dev.statistics["observations"]["mean"]) /
                       dev.statistics["observations"]["std"])


@pytest.mark.parametrize("mode", ["both", "state_only", "obs_only"])
@pytest.mark.parametrize("horizon,normalise", [(1, True), (5, True), (2, False)])
def test_device_dataset_stacked_is_bit_equal_to_the_parents(mode, horizon, normalise):
    dev, host = _pair([9, horizon + 1, horizon, 4 + horizon, 150], horizon=horizon, mode=mode, normalise=normalise,
                      seed=horizon)
    _assert_stacked_equal(dev, host)
    other = "state_only" if mode != "state_only" else "obs_only"
    dev.set_data_mode(other)
    host.set_data_mode(other)
    _assert_stacked_equal(dev, host)


def test_device_dataset_falls_back_for_another_device():
    dev, host = _pair([9, 4, 12], horizon=2)
    index, ins, outs = dev.stacked("cpu")
    h_index, h_ins, h_outs = host.stacked("cpu")
    assert index == h_index
    for got, want in zip(ins + outs, h_ins + h_outs):
        assert not got.is_cuda and torch.equal(got, want)


def _state_bytes(module, optimizers):
    """The parameters and every optimizer state entry (Adam: exp_avg, exp_avg_sq, step), as bytes."""
    out = [p.detach().cpu().numpy().tobytes() for p in module.parameters()]
    for opt in optimizers:
        for group in opt.param_groups:
            for p in group["params"]:
                st = opt.state.get(p, {})
                for k in sorted(st):
                    v = st[k]
                    out.append((k, v.detach().cpu().numpy().tobytes() if torch.is_tensor(v) else repr(v)))
    return out


@pytest.mark.parametrize("mode", ["state_only", "obs_only"])
def test_training_on_the_device_dataset_leaves_the_same_bytes(mode):
    from mbrl_amd import models
    dev, host = _pair([70, 55, 64], horizon=1, mode=mode, seed=31)
    got = {}
    for name, ds in (("device", dev), ("host", host)):
        torch.manual_seed(3)
        model = models.Model(S_DIM, A_DIM, hidden_units=64).to(DEV)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        np.random.seed(5)
        model.train_model(ds, opt, batch_size=32, num_epochs=2)
        torch.manual_seed(4)
        ens = models.EnsembleModel([models.Model(S_DIM, A_DIM, hidden_units=64) for _ in range(3)]).to(DEV)
        opts = [torch.optim.Adam(m.parameters(), lr=3e-3) for m in ens.members]
        ens.train_members(ds, opts, batch_size=32, num_epochs=2, seed=9)
        torch.cuda.synchronize()
        got[name] = _state_bytes(model, [opt]) + _state_bytes(ens, opts)
    assert len(got["device"]) == len(got["host"]) > 0
    assert got["device"] == got["host"]


def test_plan_after_training_on_the_device_dataset_uses_the_trained_weights():
    from mbrl_amd import CEMPlanner, env, models
    dev, _ = _pair([120, 100, 90], horizon=1, mode="state_only", seed=41)
    torch.manual_seed(1)
    ens = models.EnsembleModel([models.Model(S_DIM, A_DIM, hidden_units=48) for _ in range(2)]).to(DEV)
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(S_DIM), torch.zeros(S_DIM), 0.4),
                                  models.CoshLoss(0.25))
    sample = env.sample_action_fn(env.BoundedActionSpec(A_DIM, -1.0, 1.0))
    s0 = torch.linspace(-1, 1, S_DIM)

    def plan(module):
        res = CEMPlanner.plan_detailed(s0, module, cost, sample, 5, num_candidates=256, num_iterations=2, seed=3,
                                       device=DEV)
        return [res[k].detach().cpu().clone() for k in ("actions", "mu", "sigma")]
    before = plan(ens)
    ens.train_members(dev, [torch.optim.Adam(m.parameters(), lr=3e-3) for m in ens.members], batch_size=64,
                      num_epochs=3, seed=2)
    after = plan(ens)
    torch.manual_seed(7)
    fresh = models.EnsembleModel([models.Model(S_DIM, A_DIM, hidden_units=48) for _ in range(2)]).to(DEV)
    fresh.load_state_dict(copy.deepcopy(ens.state_dict()))
    want = plan(fresh)
    assert all(torch.equal(x, y) for x, y in zip(after, want))
    assert not all(torch.equal(x, y) for x, y in zip(after, before))
