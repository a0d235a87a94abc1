"""mbrl_train_grads_nll / mbrl_train_epoch_nll(_clipped) / mbrl_eval_members_nll and the ProbabilisticModel
interface on the GPU: gradients and row values against float64 (tests/train_nll_reference.py) at the project's
bar, and the byte-for-byte seams, independence, epoch, argument and Python contracts.

Bounds each comparison gave on an MI355X are written beside its test."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_nll_reference as ref
from test_gpu_train_ensemble import DEV, _Data, _dataset, _hp, _offset_like, _P, _scalars

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from mbrl_amd import _lib
    return _lib, _lib.load()


def _filled(n, fill):
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    if fill == "nan":
        ws[:n - n % 4].view(torch.float32).fill_(NAN)
    else:
        ws.fill_(0xFF if fill == "ff" else 0x5A)
    return ws


class _Member:
    """One probabilistic member's tensors: the trunk's Linears and the [2 s][W] head, gradients and Adam state."""

    def __init__(self, s, a, W, L, H, seed=0, values=None, offset=False):
        g = torch.Generator().manual_seed(seed)
        dims = [(W, s + a)] + [(W, W)] * (L - 1) + [(2 * s, W)]
        self.shape = (s, a, W, L, 0, H)
        if values is None:
            values = []
            for fo, fi in dims:
                bound = 1.0 / fi ** 0.5
                values.append(torch.rand((fo, fi), generator=g).mul(2 * bound).sub(bound).numpy())
                values.append(torch.rand((fo,), generator=g).mul(2 * bound).sub(bound).numpy())
        assert [tuple(v.shape) for v in values] == [x for fo, fi in dims for x in ((fo, fi), (fo,))]
        self.params = [torch.from_numpy(np.array(v, np.float32)).to(DEV) for v in values]
        self.grads = [torch.zeros_like(p) for p in self.params]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        if offset:                         # 4 bytes off 16: a trunk weight, the head's weight and bias, two gradients
            for i in (0, len(self.params) - 2, len(self.params) - 1):
                self.params[i] = _offset_like(self.params[i])
            for i in (1, len(self.params) - 2):
                self.grads[i] = _offset_like(self.grads[i])

    def clone(self):
        c = copy.copy(self)
        for k in ("params", "grads", "m", "v"):
            setattr(c, k, [_offset_like(t) if t.data_ptr() % 16 else t.clone() for t in getattr(self, k)])
        return c

    def fill(self, tm, s=None):
        tm.state_dim, tm.action_dim, tm.hidden, tm.n_hidden, tm.reward_head, tm.horizon = self.shape
        for i in range(len(self.params) // 2):
            tm.weight[i], tm.bias[i] = self.params[2 * i].data_ptr(), self.params[2 * i + 1].data_ptr()
            tm.weight_grad[i], tm.bias_grad[i] = self.grads[2 * i].data_ptr(), self.grads[2 * i + 1].data_ptr()

    def adam(self, table, at):
        for i, (p, g, m, v) in enumerate(zip(self.params, self.grads, self.m, self.v)):
            t = table[at + i]
            t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), \
                p.numel()


class _Bounds:
    def __init__(self, lo, hi):
        _l, _ = _lib()
        self.lo = torch.from_numpy(np.array(lo, np.float32)).to(DEV)
        self.hi = torch.from_numpy(np.array(hi, np.float32)).to(DEV)
        self.c = _l.NllBounds(self.lo.data_ptr(), self.hi.data_ptr())


def _tms(mems):
    _l, _ = _lib()
    t = (_l.TrainModel * len(mems))()
    for e, m in enumerate(mems):
        m.fill(t[e])
    return t


def run_grads(mems, data, didx, bounds, fill="5a", with_loss=True):
    """mbrl_train_grads_nll on device rows didx [E][batch] (gradient buffers pre-filled like the workspace):
    dict(loss [E][3], row_nll / row_err / row_lv [E][batch][H] from the workspace's head)."""
    _l, lib = _lib()
    E, batch = didx.shape
    H = mems[0].shape[5]
    tms = _tms(mems)
    for mem in mems:
        for g in mem.grads:
            g.fill_(NAN if fill == "nan" else -7.0 if fill == "ff" else 3.0)
    need = lib.mbrl_train_nll_workspace_bytes(tms, E, batch)
    assert need > 0
    ws = _filled(need, fill)
    loss = torch.full((E, 3), NAN, device=DEV)
    _l.check(lib.mbrl_train_grads_nll(tms, E, ctypes.byref(data.c), _P(didx), batch, ctypes.byref(bounds.c),
                                      _P(loss) if with_loss else None, _P(ws), ws.numel(), _l.stream_handle(DEV)),
             "mbrl_train_grads_nll")
    torch.cuda.synchronize()
    n = E * batch * H
    up = (n + 63) // 64 * 64
    f = ws[:12 * up].view(torch.float32)
    rows = [f[k * up:k * up + n].reshape(E, batch, H).clone() for k in range(3)]
    return dict(loss=loss, row_nll=rows[0], row_err=rows[1], row_lv=rows[2])


def run_eval(mems, data, rows, bounds, with_loss=True, fill=NAN):
    """mbrl_eval_members_nll on device rows [R]: the same dict, [E][R][H]."""
    _l, lib = _lib()
    E, R, H = len(mems), int(rows.numel()), mems[0].shape[5]
    out = torch.full((3, E, R, H), fill, device=DEV)
    loss = torch.full((E, 3), fill, device=DEV)
    _l.check(lib.mbrl_eval_members_nll(_tms(mems), E, ctypes.byref(data.c), _P(rows), R, ctypes.byref(bounds.c),
                                       _P(out[0]), _P(out[1]), _P(out[2]), _P(loss) if with_loss else None,
                                       _l.stream_handle(DEV)), "mbrl_eval_members_nll")
    torch.cuda.synchronize()
    return dict(loss=loss, row_nll=out[0], row_err=out[1], row_lv=out[2])


@functools.lru_cache(maxsize=None)
def device_data(name):
    c, p = ref.CASES[name], ref.problem(name)
    return _Data(c.s, c.a, c.H, p["T"], 0, arrays=p["data"])


@functools.lru_cache(maxsize=None)
def device_bounds(name):
    return _Bounds(*ref.problem(name)["bounds"])


def members(name, which=None):
    c, p = ref.CASES[name], ref.problem(name)
    return [_Member(c.s, c.a, c.W, c.L, c.H, values=p["members"][e], offset=c.offset and e == 1)
            for e in (range(c.E) if which is None else which)]


def rows_of(name, which=None):
    r = ref.problem(name)["rows"]
    return torch.from_numpy(np.ascontiguousarray(r if which is None else r[list(which)])).to(DEV)


@functools.lru_cache(maxsize=None)
def default_run(name):
    mems = members(name)
    return mems, run_grads(mems, device_data(name), rows_of(name), device_bounds(name))


def _same(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def _grads_equal(a, b):
    return all(_same(x, y) for x, y in zip(a.grads, b.grads))


def _runs_equal(a, b):
    return all(_same(a[k], b[k]) for k in ("loss", "row_nll", "row_err", "row_lv"))


@pytest.mark.parametrize("name", ref.NAMES)
def test_gradients_and_row_values_match_float64(name):
    """Every gradient and row array of every member within 8x the float32 CPU chain's own error, tensor-relative
    and per 32 x 32 tile.

    Measured on an MI355X, largest error / bar per case: b1 0.56, b15_s1 0.22, b16_s8 0.17, b17_s9 0.11,
    b33_s17 0.20, s33_l1 0.19, w1 0.10, w256 0.15, l8 0.41, w1024 0.17, repeats 0.18, offset 0.16. b1 is the case
    that needs the backward products' fp64 accumulation (csrc/train_nll.hip, nll_bptt_layer): hidden unit 32 of
    33 has a 32 x 32 tile of dW_0 and db_0 to itself, is active at one of the three positions, and its delta there
    is a sum of 33 products with 58x cancellation. An fp32 chain leaves 2.68e-06 and 2.71e-06 per tile there
    against bars of 2.60e-06 and 2.28e-06; the fp64 chain leaves 1.23e-06 and 1.27e-06."""
    mems, run = default_run(name)
    worst, missed = 0.0, []
    for e, mem in enumerate(mems):
        got = [g.cpu().numpy() for g in mem.grads] + [run[k][e].cpu().numpy() for k in ref.ROWS]
        for label, err, bar, own in zip(ref.tensor_names(name), ref.errors(name, got, e), ref.bars(name, e),
                                        ref.e32(name, e)):
            worst = max(worst, err[0] / bar[0], err[1] / bar[1])
            print(f"{name} member {e} {label}: err {err[0]:.3e} / {err[1]:.3e}  bar {bar[0]:.3e} / {bar[1]:.3e}  "
                  f"float32 CPU {own[0]:.3e} / {own[1]:.3e}")
            if not (err[0] <= bar[0] and err[1] <= bar[1]):
                missed.append((name, e, label, err, bar))
        want = ref.g64(name, e)["loss"]
        assert np.allclose(run["loss"][e].cpu().numpy(), want, rtol=1e-5, atol=1e-12), (name, e, run["loss"][e], want)
    print(f"{name}: largest error / bar = {worst:.3f}")
    assert not missed, missed


@pytest.mark.parametrize("name", ref.NAMES)
def test_gradient_entry_equals_the_evaluation_byte_for_byte(name):
    """loss_out and the three row arrays against mbrl_eval_members_nll, and row_err (and the MSE) against
    mbrl_eval_members on the same struct: a Model holding the trunk and the head's first s rows."""
    from test_gpu_holdout import run_eval as run_mse
    mems, run = default_run(name)
    rows = rows_of(name)
    for e, mem in enumerate(mems):
        want = run_eval([mem], device_data(name), rows[e].contiguous(), device_bounds(name))
        for k in ("loss", "row_nll", "row_err", "row_lv"):
            assert _same(run[k][e], want[k][0]), (name, e, k)
        mse = run_mse([mem], device_data(name), rows[e].contiguous())
        assert np.array_equal(mse["row_err"][0].view(np.int32), run["row_err"][e].cpu().numpy().view(np.int32))
        assert np.array_equal(mse["loss"][0, 1:2].view(np.int32), run["loss"][e, 1:2].cpu().numpy().view(np.int32))


@pytest.mark.parametrize("name", ["b33_s17", "offset"])
def test_a_member_alone_equals_the_member_among_the_others(name):
    mems, run = default_run(name)
    for e in (0, len(mems) - 1):
        alone = members(name, [e])
        one = run_grads(alone, device_data(name), rows_of(name, [e]), device_bounds(name))
        assert _grads_equal(alone[0], mems[e]), (name, e)
        assert all(_same(one[k][0], run[k][e]) for k in one)


@pytest.mark.parametrize("value", [NAN, float("inf")])
def test_a_non_finite_member_leaves_its_neighbours_alone(value):
    name = "b33_s17"
    mems, run = default_run(name)
    bad = members(name)
    bad[2].params[0][1, 2] = value
    out = run_grads(bad, device_data(name), rows_of(name), device_bounds(name))
    for e in (0, 1, 3, 4):
        assert _grads_equal(bad[e], mems[e]) and all(_same(out[k][e], run[k][e]) for k in out)
    assert not bool(torch.isfinite(out["loss"][2, 0]))


@pytest.mark.parametrize("name", ["b17_s9", "repeats", "w1024"])
def test_two_calls_agree_and_prior_bytes_never_matter(name):
    mems, run = default_run(name)
    for fill in ("nan", "ff"):
        again = members(name)
        out = run_grads(again, device_data(name), rows_of(name), device_bounds(name), fill=fill)
        assert _runs_equal(out, run), (name, fill)
        assert all(_grads_equal(x, y) for x, y in zip(again, mems)), (name, fill)
    no_loss = members(name)
    out = run_grads(no_loss, device_data(name), rows_of(name), device_bounds(name), with_loss=False)
    assert bool(torch.isnan(out["loss"]).all()) and all(_grads_equal(x, y) for x, y in zip(no_loss, mems))


# ---- epochs
def _table(mems):
    _l, _ = _lib()
    n = len(mems[0].params)
    table = (_l.AdamTensor * (len(mems) * n))()
    for e, m in enumerate(mems):
        m.adam(table, e * n)
    return table, n


def _epoch(mems, data, bounds, orders, batch, max_norm=None):
    """mbrl_train_epoch_nll(_clipped) over device orders [E][rows]: (losses [batches][E][3], norms or None)."""
    _l, lib = _lib()
    E, rows = orders.shape
    tms = _tms(mems)
    table, n = _table(mems)
    steps = -(-rows // batch)
    ss, bc = _scalars([0] * E, steps, n)
    hp = _hp()
    ws = _filled(lib.mbrl_train_nll_workspace_bytes(tms, E, min(batch, rows)), "nan")
    losses = torch.full((steps, E, 3), NAN, device=DEV)
    args = (tms, E, ctypes.byref(data.c), _P(orders), rows, batch, table, n, ctypes.byref(hp), ss, bc, _P(losses), _P(ws),
            ws.numel(), _l.stream_handle(DEV), ctypes.byref(bounds.c))
    norms = None
    if max_norm is None:
        _l.check(lib.mbrl_train_epoch_nll(*args), "mbrl_train_epoch_nll")
    else:
        cws = _filled(lib.mbrl_grad_clip_workspace_bytes(table, E, n), "ff")
        norms = torch.full((steps, E), NAN, device=DEV)
        clip = _l.GradClip(max_norm=max_norm, norms=norms.data_ptr(), workspace=cws.data_ptr(), ws_bytes=cws.numel())
        _l.check(lib.mbrl_train_epoch_nll_clipped(*args, ctypes.byref(clip)), "mbrl_train_epoch_nll_clipped")
    torch.cuda.synchronize()
    return losses, norms


def _stepwise(mems, data, bounds, orders, batch, max_norm=None):
    """The same epoch from its pieces: mbrl_train_grads_nll, then mbrl_adam_step -- or mbrl_grad_norm and
    mbrl_adam_step_clipped -- per batch."""
    _l, lib = _lib()
    E, rows = orders.shape
    table, n = _table(mems)
    steps = -(-rows // batch)
    ss, bc = _scalars([0] * E, steps, n)
    hp = _hp()
    st = _l.stream_handle(DEV)
    out, norms = [], []
    for b in range(steps):
        idx = orders[:, b * batch:(b + 1) * batch].contiguous()
        out.append(run_grads(mems, data, idx, bounds)["loss"])
        for i in range(E * n):
            table[i].step_size, table[i].bc2_sqrt = float(ss[b * E * n + i]), float(bc[b * E * n + i])
        if max_norm is None:
            _l.check(lib.mbrl_adam_step(table, E * n, ctypes.byref(hp), st), "mbrl_adam_step")
        else:
            cws = _filled(lib.mbrl_grad_clip_workspace_bytes(table, E, n), "5a")
            norm, coef = torch.full((E,), NAN, device=DEV), torch.full((E,), NAN, device=DEV)
            _l.check(lib.mbrl_grad_norm(table, E, n, max_norm, _P(norm), _P(coef), _P(cws), cws.numel(), st),
                     "mbrl_grad_norm")
            _l.check(lib.mbrl_adam_step_clipped(table, E, n, ctypes.byref(hp), _P(coef), st), "mbrl_adam_step_clipped")
            norms.append(norm)
        torch.cuda.synchronize()
    return torch.stack(out), torch.stack(norms) if norms else None


def _members_equal(xs, ys):
    return all(_same(p, q) for x, y in zip(xs, ys) for k in ("params", "m", "v", "grads")
               for p, q in zip(getattr(x, k), getattr(y, k)))


@pytest.mark.parametrize("s,a,W,L,H,E", [(9, 2, 33, 2, 3, 3), (17, 6, 64, 1, 1, 2)])
def test_epochs_equal_their_pieces(s, a, W, L, H, E):
    """The epoch entry against the gradient entry plus mbrl_adam_step per batch (three batches, the last of 13
    rows); the clipped epoch against its pieces at a norm that clips, and against the unclipped one at +inf."""
    T, batch = 45, 16
    data = _Data(s, a, H, T, seed=W)
    bounds = _Bounds(np.full(s, -5.0), np.full(s, 0.5))
    orders = torch.from_numpy(np.random.default_rng(W).integers(0, T, size=(E, T), dtype=np.int64)).to(DEV)
    start = [_Member(s, a, W, L, H, seed=10 * W + e) for e in range(E)]
    runs = [[m.clone() for m in start] for _ in range(5)]
    la, _ = _epoch(runs[0], data, bounds, orders, batch)
    lb, _ = _stepwise(runs[1], data, bounds, orders, batch)
    assert _same(la, lb) and _members_equal(runs[0], runs[1])
    assert not torch.equal(runs[0][0].params[0], start[0].params[0])
    lc, nc = _epoch(runs[2], data, bounds, orders, batch, max_norm=0.05)
    ld, nd = _stepwise(runs[3], data, bounds, orders, batch, max_norm=0.05)
    assert _same(lc, ld) and _same(nc, nd) and _members_equal(runs[2], runs[3])
    assert bool((nc > 0.05).any()) and not _members_equal(runs[2], runs[0])
    le, ne = _epoch(runs[4], data, bounds, orders, batch, max_norm=float("inf"))
    assert _same(le, la) and _members_equal(runs[4], runs[0]) and bool(torch.isfinite(ne).all())


# ---- argument checks
def test_argument_errors_come_before_any_launch():
    _l, lib = _lib()
    s, a, W, L, H, E, batch = 5, 2, 33, 2, 3, 2, 17
    data = _Data(s, a, H, 30, seed=1)
    bounds = _Bounds(np.full(s, -5.0), np.full(s, 0.5))
    mems = [_Member(s, a, W, L, H, seed=e) for e in range(E)]
    didx = torch.arange(E * batch, device=DEV).remainder(30).reshape(E, batch).contiguous()
    st = _l.stream_handle(DEV)
    tms = _tms(mems)
    need = lib.mbrl_train_nll_workspace_bytes(tms, E, batch)
    ws = _filled(need, "5a")
    loss = torch.full((E, 3), 5.0, device=DEV)
    for m in mems:
        for g in m.grads:
            g.fill_(9.0)
    half = _l.NllBounds(bounds.c.min_logvar, None)

    def call(t=tms, e=E, d=data.c, idx=didx, b=batch, w=ws, n=None, bd=bounds.c):
        return lib.mbrl_train_grads_nll(t, e, ctypes.byref(d) if d is not None else None,
                                        _P(idx) if idx is not None else None, b,
                                        ctypes.byref(bd) if bd is not None else None, _P(loss),
                                        _P(w) if w is not None else None, w.numel() if n is None else n, st)
    EINVAL, EUNSUP, EWS = _l.MBRL_EINVAL, _l.MBRL_EUNSUPPORTED, _l.MBRL_EWORKSPACE
    other = _tms([mems[0], _Member(s, a, W + 1, L, H, seed=5)])
    twice = _tms(mems)
    twice[1].bias_grad[0] = twice[0].bias_grad[0]
    nulled = _tms(mems)
    nulled[1].weight_grad[L] = None
    reward = _tms(mems)
    for t in reward:
        t.reward_head = 1
    nodata = _l.TrainData()
    nodata.states, nodata.actions, nodata.rewards = data.c.states, data.c.actions, data.c.rewards
    nodata.transitions = data.c.transitions           # (next_states stays NULL)
    wide = _tms(mems)
    for t in wide:
        t.state_dim = 633                             # 2 s = 1266: 32 rows of 1284 floats exceed the LDS
    deep = _tms(mems)
    for t in deep:
        t.n_hidden = 9
    many = _tms([_Member(s, a, W, L, H, seed=e) for e in range(9)])
    off = ws[4:]
    cases = [(call(t=other), EINVAL), (call(t=twice), EINVAL), (call(t=nulled), EINVAL), (call(t=None), EINVAL),
             (call(t=reward), EINVAL), (call(bd=None), EINVAL), (call(bd=half), EINVAL),
             (call(d=None), EINVAL), (call(d=nodata), EINVAL), (call(idx=None), EINVAL), (call(w=None, n=need), EINVAL),
             (call(w=off, n=need), EINVAL), (call(e=0), EINVAL), (call(b=0), EINVAL), (call(b=31), EINVAL),
             (call(t=many, e=9), EUNSUP), (call(t=wide), EUNSUP), (call(t=deep), EUNSUP), (call(n=need - 1), EWS)]
    torch.cuda.synchronize()
    for i, (rc, want) in enumerate(cases):
        assert rc == want, (i, rc, want)
    for bad in (other, reward, wide, deep):
        assert lib.mbrl_train_nll_workspace_bytes(bad, E, batch) == 0
    assert bool((loss == 5.0).all()) and bool((ws == 0x5A).all())
    assert all(bool((g == 9.0).all()) for m in mems for g in m.grads)
    # the epoch entries: the same codes
    table, n = _table(mems)
    ss, bc = _scalars([0] * E, 2, n)
    hp = _hp()
    cws = _filled(lib.mbrl_grad_clip_workspace_bytes(table, E, n), "5a")
    clip = _l.GradClip(max_norm=1.0, norms=None, workspace=cws.data_ptr(), ws_bytes=cws.numel())
    noclip = _l.GradClip(max_norm=-1.0, norms=None, workspace=cws.data_ptr(), ws_bytes=cws.numel())

    def epoch(t=tms, tab=table, nbytes=None, rows=batch, bd=bounds.c, cl=None):
        args = (t, E, ctypes.byref(data.c), _P(didx), rows, 16, tab, n, ctypes.byref(hp), ss, bc, None, _P(ws),
                ws.numel() if nbytes is None else nbytes, st, ctypes.byref(bd) if bd is not None else None)
        return lib.mbrl_train_epoch_nll(*args) if cl is None else lib.mbrl_train_epoch_nll_clipped(*args, ctypes.byref(cl))
    need16 = lib.mbrl_train_nll_workspace_bytes(tms, E, 16)
    for i, (rc, want) in enumerate([(epoch(t=other), EINVAL), (epoch(t=twice), EINVAL), (epoch(tab=None), EINVAL),
                                    (epoch(bd=None), EINVAL), (epoch(bd=half), EINVAL), (epoch(t=reward), EINVAL),
                                    (epoch(rows=0), EINVAL), (epoch(rows=31), EINVAL), (epoch(t=wide), EUNSUP),
                                    (epoch(nbytes=need16 - 1), EWS), (epoch(bd=None, cl=clip), EINVAL),
                                    (epoch(cl=noclip), EINVAL)]):
        assert rc == want, (i, rc, want)
    # the evaluation entry
    rows = didx[0].contiguous()
    out = torch.full((3, E, batch, H), 5.0, device=DEV)

    def ev(t=tms, bd=bounds.c, r=rows, R=batch, o0=out[0], o2=out[2]):
        return lib.mbrl_eval_members_nll(t, E, ctypes.byref(data.c), _P(r) if r is not None else None, R,
                                         ctypes.byref(bd) if bd is not None else None,
                                         _P(o0) if o0 is not None else None, _P(out[1]),
                                         _P(o2) if o2 is not None else None, _P(loss), st)
    for i, (rc, want) in enumerate([(ev(t=other), EINVAL), (ev(t=reward), EINVAL), (ev(bd=None), EINVAL),
                                    (ev(bd=half), EINVAL), (ev(r=None), EINVAL), (ev(R=0), EINVAL), (ev(o0=None), EINVAL),
                                    (ev(o2=None), EINVAL), (ev(t=wide), EUNSUP), (ev(t=deep), EUNSUP)]):
        assert rc == want, (i, rc, want)
    torch.cuda.synchronize()
    assert all(bool((g == 9.0).all()) for m in mems for g in m.grads) and bool((ws == 0x5A).all())
    assert all(bool((x == 0).all()) for m in mems for x in m.m + m.v)
    assert bool((out == 5.0).all()) and bool((loss == 5.0).all())


# ---- Python
def _sets():
    return _dataset(5, 2, 3, 96, seed=3), _dataset(5, 2, 3, 40, seed=4)


def _prob_ensemble(E, s, a, W, seed, n_hidden=2):
    from mbrl_amd import models
    torch.manual_seed(seed)
    return models.EnsembleModel([models.ProbabilisticModel(s, a, hidden_units=W, n_hidden=n_hidden, min_logvar=-6.0)
                                 for _ in range(E)]).to(DEV)


def _adam_for(ens, lr=1e-3):
    return [torch.optim.Adam(m.parameters(), lr=lr) for m in ens.members]


def _params(ens):
    return [p.detach().clone() for p in ens.parameters()]


class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, it):
        self.rows.append((tag, float(value), it))


@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
def test_train_members_nll_matches_its_fallback(monkeypatch, max_grad_norm):
    from mbrl_amd import models
    train, _ = _sets()
    a = _prob_ensemble(3, 5, 2, 32, seed=1)
    b = copy.deepcopy(a)
    wa, wb = _Writer(), _Writer()
    kw = dict(batch_size=32, num_epochs=3, seed=5, loss="nll", max_grad_norm=max_grad_norm)
    assert a.train_members(train, _adam_for(a), writer=wa, **kw) == 3
    monkeypatch.setattr(models, "NATIVE_TRAINING", False)
    assert b.train_members(train, _adam_for(b), writer=wb, **kw) == 0
    for p, q in zip(_params(a), _params(b)):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-4 * float(q.abs().max())), float((p - q).abs().max())
    ra, rb = (sorted(w.rows, key=lambda r: (r[0], r[2])) for w in (wa, wb))
    assert [(r[0], r[2]) for r in ra] == [(r[0], r[2]) for r in rb]
    assert len(ra) == 3 * 3 * 3 * (1 if max_grad_norm is None else 2)
    assert np.allclose([r[1] for r in ra], [r[1] for r in rb], rtol=1e-3, atol=1e-5)
    ea, eb = a.evaluate_members(train, nll=True), b.evaluate_members(train, nll=True)     # (b: the torch definitions)
    for k in ea:
        assert torch.allclose(ea[k], eb[k], rtol=2e-3, atol=1e-4), k
    assert not any(torch.equal(p, q) for p, q in zip(_params(a), _params(_prob_ensemble(3, 5, 2, 32, seed=1))))


def test_calls_without_the_argument_are_unchanged():
    """train_members / evaluate_members without the new arguments: the bytes of an explicit one-step call, on a
    Model ensemble (the native launches) and on a ProbabilisticModel one (its mean rows)."""
    from test_gpu_train_ensemble import _ensemble
    train, hold = _sets()
    for start in (_ensemble(2, 5, 2, 32, seed=2), _prob_ensemble(2, 5, 2, 32, seed=2)):
        runs = []
        for kw in ({}, {"loss": "one_step"}):
            e = copy.deepcopy(start)
            e.train_members(train, _adam_for(e), batch_size=32, num_epochs=2, seed=1, **kw)
            ev = e.evaluate_members(hold)
            assert set(ev) == {"loss", "per_step", "row_err"}
            runs.append(_params(e) + [ev[k] for k in sorted(ev)])
        assert all(torch.equal(x, y) for x, y in zip(*runs))
    # a probabilistic ensemble's default evaluation is the mean rows' held-out MSE
    ens = _prob_ensemble(2, 5, 2, 32, seed=3)
    plain, nll = ens.evaluate_members(hold), ens.evaluate_members(hold, nll=True)
    assert torch.equal(plain["row_err"], nll["row_err"]) and torch.equal(plain["loss"], nll["mse"])


def test_fit_members_nll_rows_are_evaluate_members_after_as_many_epochs():
    train, hold = _sets()
    start = _prob_ensemble(2, 5, 2, 32, seed=3)
    fit = copy.deepcopy(start)
    rep = fit.fit_members(train, hold, _adam_for(fit, 3e-3), batch_size=32, max_epochs=3, seed=2, train_loss="nll",
                          holdout_loss="nll", max_grad_norm=5.0)
    assert rep["native_epochs"] == 3 and rep["epochs_run"] == 3 and rep["native_eval"]
    after = []
    for k in range(3):
        run = copy.deepcopy(start)
        run.train_members(train, _adam_for(run, 3e-3), batch_size=32, num_epochs=k + 1, seed=2, loss="nll",
                          max_grad_norm=5.0)
        want = run.evaluate_members(hold, nll=True)["loss"].cpu()
        assert torch.equal(rep["val_loss"][k], want), (k, rep["val_loss"][k], want)
        after.append(run)
    # restore_best: each member holds the parameters of its best epoch
    for e, at in enumerate(rep["best_epoch"].tolist()):
        assert rep["val_loss"][at, e] == rep["val_loss"][:, e].min()
        for p, q in zip(fit.members[e].parameters(), after[at].members[e].parameters()):
            assert torch.equal(p, q)


def test_plans_on_probabilistic_members_are_the_plans_on_their_mean_rows():
    """A CEM plan and an MPPI plan on a ProbabilisticModel ensemble equal, byte for byte, the plans on Model
    copies of the trunk and the head's mean rows."""
    from mbrl_amd import CEMPlanner, MPPIPlanner, env, models
    s, a, W = 5, 2, 32
    ens = _prob_ensemble(2, s, a, W, seed=4)
    torch.manual_seed(0)
    plain = models.EnsembleModel([models.Model(s, a, hidden_units=W) for _ in range(2)]).to(DEV)
    with torch.no_grad():
        for m, p in zip(plain.members, ens.members):
            for dst, src in zip(m.linears(), p.mean_linears()):
                dst.weight.copy_(src.weight)
                dst.bias.copy_(src.bias)
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(s), torch.zeros(s), 0.4), models.CoshLoss(0.25))
    sample = env.sample_action_fn(env.BoundedActionSpec(a, -1.0, 1.0))
    s0 = torch.linspace(-1, 1, s)
    # the packer is handed the head's first s rows: both ensembles pack to the same fragment stream
    from mbrl_amd import fused
    de, dp = fused.describe_model(functools.partial(ens)), fused.describe_model(functools.partial(plain))
    assert (de["E"], de["s"], tuple(de["members"][0][-1].weight.shape)) == (2, s, (s, W))
    assert torch.equal(fused.packed_weights(de, DEV), fused.packed_weights(dp, DEV))
    for planner, keys in ((CEMPlanner, ("actions", "mu", "sigma")), (MPPIPlanner, ("actions",))):
        def plan(module):
            res = planner.plan_detailed(s0, module, cost, sample, 5, num_candidates=256, num_iterations=2, seed=3,
                                        device="cuda:0")
            return [res[k].detach().cpu().clone() for k in keys]
        got, want = plan(ens), plan(plain)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), planner.__name__
