"""Global-norm gradient clipping on the GPU (csrc/grad_clip.hip, include/mbrl_cem.h): mbrl_grad_norm against the NumPy
restatement of its order bit for bit (tests/grad_clip_reference.py), mbrl_adam_step_clipped against mbrl_adam_step on
pre-scaled gradients, the clipped epoch entries of both losses against their per-batch equivalents and their
unclipped siblings, the argument checks, and EnsembleModel.train_members / fit_members(max_grad_norm=...)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import grad_clip_reference as ref
from test_gpu_train_ensemble import DEV, _Data, _dataset, _ensemble, _hp, _Member, _offset_like, _P, _scalars

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F = np.float32


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


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- mbrl_grad_norm
def _device_grads(grads, offset=False):
    out = []
    for gs in grads:
        ts = [torch.from_numpy(np.ascontiguousarray(g)).to(DEV) for g in gs]
        out.append([_offset_like(t) if offset and t.numel() else t for t in ts])
    return out


def run_norm(grads, max_norm, offset=False, fill="5a", with_norm=True):
    """mbrl_grad_norm on [member][tensor] NumPy gradients: (norm [E] or None, coef [E]) as NumPy."""
    _l, lib = _lib()
    E, count = len(grads), max(len(gs) for gs in grads)      # (a member of fewer tensors: numel 0 in the rest)
    dev = _device_grads(grads, offset)
    table = (_l.AdamTensor * (E * count))()
    for e in range(E):
        for i, t in enumerate(dev[e]):
            table[e * count + i].grad = t.data_ptr() if t.numel() else None
            table[e * count + i].numel = t.numel()
    need = lib.mbrl_grad_clip_workspace_bytes(table, E, count)
    assert need > 0
    ws = _filled(need, fill)
    norm = torch.full((E,), -5.0, device=DEV)
    coef = torch.full((E,), -5.0, device=DEV)
    _l.check(lib.mbrl_grad_norm(table, E, count, max_norm, _P(norm) if with_norm else None, _P(coef), _P(ws),
                                ws.numel(), _l.stream_handle(DEV)), "mbrl_grad_norm")
    torch.cuda.synchronize()
    for gs, ds in zip(grads, dev):                       # the gradients are only read
        assert all(np.array_equal(g.view(np.int32), _bits(d)) for g, d in zip(gs, ds))
    return (norm.cpu().numpy() if with_norm else None), coef.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case_run(name):
    return run_norm(ref.gradients(name), ref.CASES[name]["max_norm"])


def _equal_or_both_nan(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    return np.array_equal(got.view(np.int32), want.view(np.int32)) or (np.isnan(got).all() and np.isnan(want).all())


@pytest.mark.parametrize("name", ref.NAMES)
def test_grad_norm_is_the_restatement_bit_for_bit(name):
    """numel in {0, 1, 3, 1023, 1024, 1025, 4099}, E in {1, 2, 3, 5, 8}, E * count = 64 and 80, P = 1024 and 1025,
    zero, tiny, NaN and inf members: norm_out and coef_out carry the restatement's bits."""
    norm, coef = case_run(name)
    for e, grads in enumerate(ref.gradients(name)):
        n = ref.norm(grads)
        c = ref.coef(n, ref.CASES[name]["max_norm"])
        assert _equal_or_both_nan(norm[e], n), (name, e, norm[e], n)
        assert _equal_or_both_nan(coef[e], c), (name, e, coef[e], c)


@pytest.mark.parametrize("name", ["seams", "e8_c10", "p1025"])
def test_pointer_alignment_and_prior_bytes_never_matter(name):
    """Gradients at 4-byte offsets (scalar loads) give the bytes of 16-byte-aligned ones (float4 loads); a workspace
    of NaNs or 0xFF bytes gives the bytes of any other; a NULL norm_out changes no coefficient."""
    norm, coef = case_run(name)
    for kw in (dict(offset=True), dict(fill="nan"), dict(fill="ff"), dict(with_norm=False)):
        n2, c2 = run_norm(ref.gradients(name), ref.CASES[name]["max_norm"], **kw)
        assert np.array_equal(coef.view(np.int32), c2.view(np.int32)), (name, kw)
        assert n2 is None or np.array_equal(norm.view(np.int32), n2.view(np.int32)), (name, kw)


@pytest.mark.parametrize("name", ["e5", "nan", "p1025", "e8_c8"])
def test_a_members_norm_depends_on_that_member_alone(name):
    """Not on E, on the member's position or on the other members (a NaN one included): alone, and in reverse."""
    norm, coef = case_run(name)
    grads, max_norm = ref.gradients(name), ref.CASES[name]["max_norm"]
    E = len(grads)
    nr, cr = run_norm(grads[::-1], max_norm)
    for e in range(E):
        assert _equal_or_both_nan(nr[E - 1 - e], norm[e]) and _equal_or_both_nan(cr[E - 1 - e], coef[e]), (name, e)
    for e in {0, E // 2, E - 1}:
        n1, c1 = run_norm([grads[e]], max_norm)
        assert _equal_or_both_nan(n1[0], norm[e]) and _equal_or_both_nan(c1[0], coef[e]), (name, e)


# ---- mbrl_adam_step_clipped
class _Group:
    """E members' Adam tensors of the given numels: parameters, gradients and non-trivial moments."""

    def __init__(self, numels, E, seed, grads=None):
        g = torch.Generator().manual_seed(seed)
        mk = lambda n, scale: (torch.randn(n, generator=g) * scale).to(DEV)
        self.E, self.count = E, len(numels)
        self.params = [[mk(n, 1.0) for n in numels] for _ in range(E)]
        self.grads = grads or [[mk(n, 0.1) for n in numels] for _ in range(E)]
        self.m = [[mk(n, 0.01) for n in numels] for _ in range(E)]
        self.v = [[mk(n, 0.01).square() for n in numels] for _ in range(E)]

    def clone(self, grads=None):
        c = copy.copy(self)
        for k in ("params", "m", "v"):
            setattr(c, k, [[t.clone() for t in ts] for ts in getattr(self, k)])
        c.grads = grads or [[t.clone() for t in ts] for ts in self.grads]
        return c

    def table(self, step=3):
        _l, _ = _lib()
        table = (_l.AdamTensor * (self.E * self.count))()
        ss, bc = _scalars([step + e for e in range(self.E)], 1, self.count)
        for e in range(self.E):
            for i in range(self.count):
                t = table[e * self.count + i]
                n = self.params[e][i].numel()
                t.param, t.grad, t.exp_avg, t.exp_avg_sq = [x[e][i].data_ptr() if n else None
                                                            for x in (self.params, self.grads, self.m, self.v)]
                t.numel = n
                t.step_size, t.bc2_sqrt = ss[e * self.count + i], bc[e * self.count + i]
        return table

    def state(self):
        return [t for k in ("params", "m", "v") for ts in getattr(self, k) for t in ts]


def _plain_step(group, wd):
    _l, lib = _lib()
    hp = _hp(wd)
    _l.check(lib.mbrl_adam_step(group.table(), group.E * group.count, ctypes.byref(hp), _l.stream_handle(DEV)),
             "mbrl_adam_step")
    torch.cuda.synchronize()


def _clipped_step(group, coef, wd):
    _l, lib = _lib()
    hp = _hp(wd)
    c = torch.tensor(coef, dtype=torch.float32, device=DEV)
    _l.check(lib.mbrl_adam_step_clipped(group.table(), group.E, group.count, ctypes.byref(hp), _P(c),
                                        _l.stream_handle(DEV)), "mbrl_adam_step_clipped")
    torch.cuda.synchronize()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("E,numels", [(2, [1, 3, 1023, 1024, 1025, 4099, 0]),
                                      (8, [33, 1, 1025, 0, 7, 1024, 3, 2049, 5, 1023])])
def test_adam_step_clipped_is_adam_step_on_prescaled_gradients(E, numels, wd):
    """Parameters, exp_avg and exp_avg_sq byte-equal to mbrl_adam_step on gradients multiplied by coef in fp32 on the
    host, with and without weight decay and across the 64-tensor split (8 x 10 tensors); coef = 1 is mbrl_adam_step
    itself; the gradient buffers keep the raw gradient."""
    start = _Group(numels, E, seed=E)
    coef = [F(0.37), F(1.0), F(1e-3), F(0.999999), F(0.5), F(1.0), F(0.25), F(0.8)][:E]
    raw = [[t.clone() for t in ts] for ts in start.grads]
    got = start.clone()
    _clipped_step(got, coef, wd)
    pre = [[torch.from_numpy(g.cpu().numpy() * c).to(DEV) for g in ts] for ts, c in zip(raw, coef)]
    want = start.clone(grads=pre)
    _plain_step(want, wd)
    for x, y in zip(got.state(), want.state()):
        assert _same(x, y)
    assert all(_same(x, y) for a, b in zip(got.grads, raw) for x, y in zip(a, b))
    assert not _same(got.params[0][2], start.params[0][2])
    ones, plain = start.clone(), start.clone()
    _clipped_step(ones, [F(1.0)] * E, wd)
    _plain_step(plain, wd)
    for x, y in zip(ones.state(), plain.state()):
        assert _same(x, y)


# ---- the epoch entries, both losses
ENTRIES = {
    "one_step": ("mbrl_train_epoch_ensemble", "mbrl_train_grads_ensemble", "mbrl_train_ensemble_workspace_bytes"),
    "open_loop": ("mbrl_train_epoch_open_loop", "mbrl_train_grads_open_loop", "mbrl_train_open_loop_workspace_bytes"),
}
#          s, a,  W, L, H, reward, E, batch      (45 rows: batches of 16, 16, 13 and of 17, 17, 11)
CONFIGS = [(5, 2, 33, 2, 3, 1, 3, 16), (17, 6, 64, 1, 1, 0, 2, 17), (4, 1, 33, 3, 3, 0, 2, 17)]
ROWS = 45


def _bind(mems):
    _l, _ = _lib()
    E, n = len(mems), len(mems[0].params)
    tms = (_l.TrainModel * E)()
    table = (_l.AdamTensor * (E * n))()
    for e, m in enumerate(mems):
        m.fill(tms[e])
        m.adam(table, e * n)
    return tms, table, n


def _clip_struct(table, E, n, max_norm, steps, fill="nan"):
    _l, lib = _lib()
    need = lib.mbrl_grad_clip_workspace_bytes(table, E, n)
    assert need > 0
    cws = _filled(need, fill)
    norms = torch.full((steps, E), -5.0, device=DEV)
    return _l.GradClip(max_norm=max_norm, norms=norms.data_ptr(), workspace=cws.data_ptr(), ws_bytes=need), norms, cws


def run_epoch(loss, mems, data, orders, batch, max_norm=None):
    """The epoch entry of `loss` (max_norm None: the unclipped sibling) over device orders [E][rows]:
    (losses [batches][E][3], norms [batches][E] or None)."""
    _l, lib = _lib()
    epoch, _, wsb = ENTRIES[loss]
    E, rows = orders.shape
    tms, table, n = _bind(mems)
    steps = -(-rows // batch)
    ss, bc = _scalars([0] * E, steps, n)
    hp = _hp()
    ws = _filled(getattr(lib, wsb)(tms, E, min(batch, rows)), "nan")
    losses = torch.full((steps, E, 3), NAN, device=DEV)
    args = (tms, E, ctypes.byref(data.c), _P(orders), rows, batch, table, n, ctypes.byref(hp), ss, bc, _P(losses),
            _P(ws), ws.numel(), _l.stream_handle(DEV))
    norms = None
    if max_norm is None:
        _l.check(getattr(lib, epoch)(*args), epoch)
    else:
        clip, norms, keep = _clip_struct(table, E, n, max_norm, steps)
        _l.check(getattr(lib, epoch + "_clipped")(*args, ctypes.byref(clip)), epoch + "_clipped")
    torch.cuda.synchronize()
    return losses, norms


def run_stepwise(loss, mems, data, orders, batch, max_norm):
    """The same epoch as the gradient entry, mbrl_grad_norm and mbrl_adam_step_clipped per batch."""
    _l, lib = _lib()
    _, grads_entry, wsb = ENTRIES[loss]
    E, rows = orders.shape
    tms, table, n = _bind(mems)
    steps = -(-rows // batch)
    ss, bc = _scalars([0] * E, steps, n)
    hp = _hp()
    st = _l.stream_handle(DEV)
    losses, norms = torch.full((steps, E, 3), NAN, device=DEV), torch.full((steps, E), NAN, device=DEV)
    coef = torch.full((E,), NAN, device=DEV)
    cws = _filled(lib.mbrl_grad_clip_workspace_bytes(table, E, n), "ff")
    for b in range(steps):
        idx = orders[:, b * batch:(b + 1) * batch].contiguous()
        ws = _filled(getattr(lib, wsb)(tms, E, idx.shape[1]), "5a")
        _l.check(getattr(lib, grads_entry)(tms, E, ctypes.byref(data.c), _P(idx), idx.shape[1], _P(losses[b]), _P(ws),
                                           ws.numel(), st), grads_entry)
        _l.check(lib.mbrl_grad_norm(table, E, n, max_norm, _P(norms[b]), _P(coef), _P(cws), cws.numel(), st),
                 "mbrl_grad_norm")
        for i in range(E * n):
            table[i].step_size, table[i].bc2_sqrt = float(ss[b * E * n + i]), float(bc[b * E * n + i])
        _l.check(lib.mbrl_adam_step_clipped(table, E, n, ctypes.byref(hp), _P(coef), st), "mbrl_adam_step_clipped")
        torch.cuda.synchronize()
    return losses, norms


def _members_equal(xs, ys, keys=("params", "m", "v", "grads")):
    return all(_same(p, q) for x, y in zip(xs, ys) for k in keys for p, q in zip(getattr(x, k), getattr(y, k)))


@functools.lru_cache(maxsize=None)
def _problem(loss, cfg):
    """The configuration's data, orders and start members, its unclipped and max_norm = +inf epochs, and a max_norm
    between the recorded norms (the midpoint of the two middle ones)."""
    s, a, W, L, H, reward, E, batch = cfg
    data = _Data(s, a, H, ROWS, seed=W + H)
    orders = torch.from_numpy(np.random.default_rng(W).integers(0, ROWS, size=(E, ROWS), dtype=np.int64)).to(DEV)
    start = [_Member(s, a, W, L, reward, H, seed=10 * W + e) for e in range(E)]
    plain, free = [m.clone() for m in start], [m.clone() for m in start]
    l_plain, _ = run_epoch(loss, plain, data, orders, batch)
    l_free, n_free = run_epoch(loss, free, data, orders, batch, INF)
    flat = np.sort(n_free.cpu().numpy().reshape(-1))
    mid = float((flat[flat.size // 2 - 1] + flat[flat.size // 2]) / 2)
    return dict(data=data, orders=orders, start=start, batch=batch, plain=(plain, l_plain), free=(free, l_free, n_free),
                max_norm=mid)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("loss", list(ENTRIES))
def test_infinite_max_norm_is_the_unclipped_sibling_and_fills_norms(loss, cfg):
    p = _problem(loss, cfg)
    (plain, l_plain), (free, l_free, n_free) = p["plain"], p["free"]
    assert _same(l_plain, l_free) and _members_equal(plain, free)
    assert bool(torch.isfinite(n_free).all()) and bool((n_free > 0).all())
    assert not _same(plain[0].params[0], p["start"][0].params[0])


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("loss", list(ENTRIES))
def test_clipped_epoch_equals_its_per_batch_sequence_and_clips_some_batches(loss, cfg):
    """Parameters, both moments, the last raw gradients, losses and norms byte-equal to the gradient entry,
    mbrl_grad_norm and mbrl_adam_step_clipped per batch; with max_norm between the recorded norms some batches clip
    and some do not, and a member's norms up to its first clipped batch are those of the max_norm = +inf run."""
    p = _problem(loss, cfg)
    m = p["max_norm"]
    a_run, b_run = [x.clone() for x in p["start"]], [x.clone() for x in p["start"]]
    la, na = run_epoch(loss, a_run, p["data"], p["orders"], p["batch"], m)
    lb, nb = run_stepwise(loss, b_run, p["data"], p["orders"], p["batch"], m)
    assert _same(la, lb) and _same(na, nb) and _members_equal(a_run, b_run)
    free, l_free, n_free = p["free"]
    got, was = na.cpu().numpy(), n_free.cpu().numpy()
    assert (got > m).any() and (got <= m).any()
    assert not _members_equal(a_run, free, keys=("params",))
    for e in range(got.shape[1]):
        clipped = np.nonzero(got[:, e] > m)[0]
        upto = got.shape[0] if clipped.size == 0 else clipped[0] + 1
        assert np.array_equal(got[:upto, e].view(np.int32), was[:upto, e].view(np.int32)), (e, got[:, e], was[:, e])
        if clipped.size == 0:
            assert _members_equal([a_run[e]], [free[e]])
    # the clipping is clip_grad_norm_'s: the first batch's norm against the restatement of the raw gradients it left
    # is covered per batch by the stepwise run; here the last batch's raw gradients give the last norms
    for e, mem in enumerate(a_run):
        want = ref.norm([g.cpu().numpy() for g in mem.grads])
        assert np.array_equal(F(want).view(np.int32), got[-1, e].view(np.int32))


@pytest.mark.parametrize("loss", list(ENTRIES))
def test_a_member_alone_equals_the_member_among_the_others(loss):
    p = _problem(loss, CONFIGS[0])
    m = p["max_norm"]
    ens = [x.clone() for x in p["start"]]
    le, ne = run_epoch(loss, ens, p["data"], p["orders"], p["batch"], m)
    for e in (0, len(ens) - 1):
        alone = [p["start"][e].clone()]
        l1, n1 = run_epoch(loss, alone, p["data"], p["orders"][e:e + 1].contiguous(), p["batch"], m)
        assert _members_equal(alone, [ens[e]]) and _same(l1[:, 0], le[:, e]) and _same(n1[:, 0], ne[:, e])


def test_a_nan_member_leaves_the_other_members_bytes_alone():
    loss = "open_loop"
    p = _problem(loss, CONFIGS[0])
    m = p["max_norm"]
    ens, bad = [x.clone() for x in p["start"]], [x.clone() for x in p["start"]]
    le, ne = run_epoch(loss, ens, p["data"], p["orders"], p["batch"], m)
    bad[1].params[0][1, 0] = NAN
    lb, nb = run_epoch(loss, bad, p["data"], p["orders"], p["batch"], m)
    for e in (0, 2):
        assert _members_equal([ens[e]], [bad[e]]) and _same(le[:, e], lb[:, e]) and _same(ne[:, e], nb[:, e])
    assert bool(torch.isnan(nb[:, 1]).all()) and bool(torch.isnan(bad[1].params[2]).all())


# ---- argument checks
def test_argument_errors_come_before_any_launch():
    _l, lib = _lib()
    EINVAL, EUNSUP, EWS = _l.MBRL_EINVAL, _l.MBRL_EUNSUPPORTED, _l.MBRL_EWORKSPACE
    s, a, W, L, H, reward, E, batch = 5, 2, 33, 2, 3, 1, 2, 16
    data = _Data(s, a, H, 30, seed=1)
    mems = [_Member(s, a, W, L, reward, H, seed=e) for e in range(9)]
    for mem in mems:
        for t in mem.grads + mem.m:
            t.fill_(3.0)
    before = [[t.clone() for t in mem.tensors()] for mem in mems]
    tms, table, n = _bind(mems[:E])
    big_tms, big_table, _ = _bind(mems)
    orders = torch.arange(E * 30, device=DEV).remainder(30).reshape(E, 30).contiguous()
    st = _l.stream_handle(DEV)
    ss, bc = _scalars([0] * 9, 2, n)
    hp = _hp()
    clip, norms, cws = _clip_struct(table, E, n, 1.0, 2, fill="5a")
    need = clip.ws_bytes

    def with_(**kw):
        c = _l.GradClip(max_norm=clip.max_norm, norms=clip.norms, workspace=clip.workspace, ws_bytes=clip.ws_bytes)
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)
    cases = []
    for loss, (epoch, _, wsb) in ENTRIES.items():
        ws = _filled(getattr(lib, wsb)(tms, E, batch), "5a")
        fn = getattr(lib, epoch + "_clipped")

        def call(c, t=tms, e=E, tab=table, o=orders, nbytes=None, ws=ws, fn=fn):
            return fn(t, e, ctypes.byref(data.c), _P(o) if o is not None else None, 30, batch, tab, n, ctypes.byref(hp),
                      ss, bc, None, _P(ws), ws.numel() if nbytes is None else nbytes, st, c)
        cases += [(call(None), EINVAL), (call(with_(max_norm=NAN)), EINVAL), (call(with_(max_norm=0.0)), EINVAL),
                  (call(with_(max_norm=-1.0)), EINVAL), (call(with_(workspace=None)), EINVAL),
                  (call(with_(ws_bytes=need - 1)), EWS), (call(with_(), o=None), EINVAL),
                  (call(with_(), nbytes=ws.numel() - 1), EWS), (call(with_(), t=big_tms, e=9, tab=big_table), EUNSUP)]
        torch.cuda.synchronize()
        assert bool((ws == 0x5A).all())
    coef = torch.full((9,), 7.0, device=DEV)

    def gnorm(tab=table, e=E, cnt=n, mx=1.0, c=coef, w=cws, nbytes=None):
        return lib.mbrl_grad_norm(tab, e, cnt, mx, _P(norms), _P(c) if c is not None else None,
                                  _P(w) if w is not None else None, need if nbytes is None else nbytes, st)
    negative, nograd = _bind(mems[:E])[1], _bind(mems[:E])[1]
    negative[1].numel = -1
    nograd[n + 1].grad = None
    cases += [(gnorm(mx=NAN), EINVAL), (gnorm(mx=0.0), EINVAL), (gnorm(c=None), EINVAL), (gnorm(w=None), EINVAL),
              (gnorm(e=0), EINVAL), (gnorm(cnt=0), EINVAL), (gnorm(tab=None), EINVAL), (gnorm(tab=negative), EINVAL),
              (gnorm(tab=nograd), EINVAL), (gnorm(tab=big_table, e=9), EUNSUP), (gnorm(nbytes=need - 1), EWS)]
    noparam = _bind(mems[:E])[1]
    noparam[2].param = None
    cases += [(lib.mbrl_adam_step_clipped(table, E, n, ctypes.byref(hp), None, st), EINVAL),
              (lib.mbrl_adam_step_clipped(table, E, n, None, _P(coef), st), EINVAL),
              (lib.mbrl_adam_step_clipped(noparam, E, n, ctypes.byref(hp), _P(coef), st), EINVAL),
              (lib.mbrl_adam_step_clipped(big_table, 9, n, ctypes.byref(hp), _P(coef), st), EUNSUP)]
    assert lib.mbrl_grad_clip_workspace_bytes(negative, E, n) == 0
    assert lib.mbrl_grad_clip_workspace_bytes(big_table, 9, n) == 0
    assert lib.mbrl_grad_clip_workspace_bytes(table, 0, n) == 0
    torch.cuda.synchronize()
    for i, (rc, want) in enumerate(cases):
        assert rc == want, (i, rc, want, lib.mbrl_last_error())
    assert bool((norms == -5.0).all()) and bool((coef == 7.0).all()) and bool((cws == 0x5A).all())
    for mem, snap in zip(mems, before):
        assert all(torch.equal(x, y) for x, y in zip(mem.tensors(), snap))


# ---- Python
class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, it):
        self.rows.append((tag, float(value), it))


def _sets():
    return _dataset(5, 2, 3, 96, seed=3), _dataset(5, 2, 3, 40, seed=4)


def _adam_for(ens):
    return [torch.optim.Adam(m.parameters(), lr=1e-3) for m in ens.members]


def _params(ens):
    return [p.detach().clone() for p in ens.parameters()]


def _middle_norm(start, train, loss, seed):
    """A max_grad_norm between the norms of one unclipped epoch from `start`: some batches clip, some do not."""
    w, probe = _Writer(), copy.deepcopy(start)
    assert probe.train_members(train, _adam_for(probe), batch_size=32, num_epochs=1, seed=seed, loss=loss, writer=w,
                               max_grad_norm=INF) == 1
    norms = sorted(r[1] for r in w.rows if r[0].startswith("grad_norm/"))
    assert len(norms) == 3 * len(start.members)
    return (norms[len(norms) // 2 - 1] + norms[len(norms) // 2]) / 2


def _first_batch_gradient(member, ds, rows, open_loop, dtype):
    """The member's gradient on its first batch by autograd in `dtype`, as NumPy float64 arrays."""
    m = copy.deepcopy(member).to(dtype)
    _, (states, actions), (_, next_states) = ds.stacked(DEV)
    idx = torch.from_numpy(rows).to(DEV)
    st, ac, ns = (x.index_select(0, idx).to(dtype) for x in (states, actions, next_states))
    x, loss = st[:, 0], 0
    for h in range(ds.horizon):
        x = m._forward(torch.cat([x if open_loop else st[:, h], ac[:, h]], dim=1))
        loss = loss + torch.nn.functional.mse_loss(x, ns[:, h])
    return [g.double().cpu().numpy() for g in torch.autograd.grad(loss, list(m.parameters()))]


@pytest.mark.parametrize("loss", ["one_step", "open_loop"])
def test_train_members_clipped_matches_its_torch_fallback(loss):
    """train_members(max_grad_norm=m) through the clipped entry against the fallback with clip_grad_norm_ (a member
    with `noise` set, here 0.0, sends every member there): parameters within the 1e-4 bar of train_members' fallback
    comparison. grad_norm tags: the first batch's -- both paths still hold the same parameters -- within the derived
    norm bar plus 8x the norm of the gradient's own fp32-to-float64 error (the factor the gradient tests allow the
    kernels over the fp32 chain's own error: a norm moves by at most the norm of the gradient's error); the later
    ones, whose parameters have drifted apart within the bar above, at the 1e-3 the loss tags are held to."""
    from mbrl_amd import models
    train, _ = _sets()
    a = _ensemble(3, 5, 2, 32, seed=1)
    b = copy.deepcopy(a)
    b.members[0].noise = 0.0
    start = copy.deepcopy(a)
    m = _middle_norm(a, train, loss, seed=5)
    wa, wb = _Writer(), _Writer()
    assert a.train_members(train, _adam_for(a), batch_size=32, num_epochs=3, seed=5, loss=loss, writer=wa,
                           max_grad_norm=m) == 3
    assert b.train_members(train, _adam_for(b), batch_size=32, num_epochs=3, seed=5, loss=loss, writer=wb,
                           max_grad_norm=m) == 0
    for p, q in zip(_params(a), _params(b)):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-4 * float(q.abs().max())), float((p - q).abs().max())
    ra, rb = (sorted(w.rows, key=lambda r: (r[0], r[2])) for w in (wa, wb))
    assert [(r[0], r[2]) for r in ra] == [(r[0], r[2]) for r in rb] and len(ra) == 2 * 3 * 3 * 3
    na, nb = ([r for r in rows if r[0].startswith("grad_norm/")] for rows in (ra, rb))
    assert [r[0] for r in na[::9]] == [f"grad_norm/member{e}/0" for e in range(3)]
    assert any(r[1] > m for r in na) and any(r[1] <= m for r in na)
    assert np.allclose([r[1] for r in na], [r[1] for r in nb], rtol=1e-3)
    assert np.allclose([r[1] for r in ra], [r[1] for r in rb], rtol=1e-3)
    n = train.num_transitions()
    for e, member in enumerate(start.members):
        rows = models.member_order(5, e, 0, n)[:32]
        g32 = _first_batch_gradient(member, train, rows, loss == "open_loop", torch.float32)
        g64 = _first_batch_gradient(member, train, rows, loss == "open_loop", torch.float64)
        own = float(np.sqrt(sum(np.sum((x - y) ** 2) for x, y in zip(g32, g64))))
        n64 = float(np.sqrt(sum(np.sum(y ** 2) for y in g64)))
        bar = ref.norm_bar([y.size for y in g64]) * n64 + 8 * own
        first_a, first_b = na[9 * e][1], nb[9 * e][1]
        print(f"{loss} member {e}: native {first_a:.9g}  fallback {first_b:.9g}  float64 {n64:.9g}  bar {bar:.3e}")
        assert abs(first_a - n64) <= bar and abs(first_b - n64) <= bar


def test_max_grad_norm_none_is_a_call_without_it_and_bad_values_raise():
    train, _ = _sets()
    start = _ensemble(2, 5, 2, 32, seed=2)
    runs = []
    for kw in ({}, {"max_grad_norm": None}, {"loss": "open_loop"}, {"loss": "open_loop", "max_grad_norm": None}):
        e = copy.deepcopy(start)
        opts = _adam_for(e)
        assert e.train_members(train, opts, batch_size=32, num_epochs=2, seed=1, **kw) == 2
        state = [t.clone() for o in opts for st in o.state.values() for t in (st["exp_avg"], st["exp_avg_sq"])]
        runs.append(_params(e) + state)
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))
    assert all(torch.equal(x, y) for x, y in zip(runs[2], runs[3]))
    before = _params(start)
    for bad in (0, -1.0, NAN, "1", True, [1.0]):
        with pytest.raises(ValueError):
            start.train_members(train, _adam_for(start), max_grad_norm=bad)
        with pytest.raises(ValueError):
            start.fit_members(train, train, _adam_for(start), max_grad_norm=bad)
    assert all(torch.equal(x, y) for x, y in zip(before, _params(start))) and start.train_iterations == 0


def test_fit_members_clipped_restores_each_member_to_its_best_epoch():
    train, hold = _sets()
    start = _ensemble(2, 5, 2, 32, seed=3)
    m = _middle_norm(start, train, "open_loop", seed=2)
    fit = copy.deepcopy(start)
    rep = fit.fit_members(train, hold, _adam_for(fit), batch_size=32, max_epochs=3, seed=2, train_loss="open_loop",
                          holdout_loss="open_loop", max_grad_norm=m)
    assert rep["native_epochs"] == 3 and rep["epochs_run"] == 3
    runs = []
    for k in range(3):
        run = copy.deepcopy(start)
        w = _Writer()
        run.train_members(train, _adam_for(run), batch_size=32, num_epochs=k + 1, seed=2, loss="open_loop",
                          max_grad_norm=m, writer=w)
        assert any(r[0].startswith("grad_norm/") and r[1] > m for r in w.rows)       # it did clip
        assert torch.equal(rep["val_loss"][k], run.evaluate_members(hold, open_loop=True)["loss"].cpu())
        runs.append(run)
    for e, at in enumerate(rep["best_epoch"].tolist()):
        assert at >= 0
        for p, q in zip(fit.members[e].parameters(), runs[at].members[e].parameters()):
            assert torch.equal(p, q), (e, at)


def test_plan_after_clipped_training_uses_the_new_weights():
    from mbrl_amd import CEMPlanner, env, models
    s, a, W = 5, 2, 32
    train, _ = _sets()
    ens = _ensemble(2, s, a, W, seed=4)
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(s), torch.zeros(s), 0.4), models.CoshLoss(0.25))
    sample = env.sample_action_fn(env.BoundedActionSpec(a, -1.0, 1.0))
    s0 = torch.linspace(-1, 1, s)

    def plan(module):
        res = CEMPlanner.plan_detailed(s0, module, cost, sample, 5, num_candidates=256, num_iterations=2, seed=3,
                                       device="cuda:0")
        return [res[k].detach().cpu().clone() for k in ("actions", "mu", "sigma")]
    before = plan(ens)
    ens.train_members(train, [torch.optim.Adam(m.parameters(), lr=3e-3) for m in ens.members], batch_size=32,
                      num_epochs=3, seed=2, loss="open_loop", max_grad_norm=0.5)
    after = plan(ens)
    fresh = _ensemble(2, s, a, W, seed=7)
    fresh.load_state_dict(copy.deepcopy(ens.state_dict()))
    want = plan(fresh)
    assert all(torch.equal(x, y) for x, y in zip(after, want))
    assert not all(torch.equal(x, y) for x, y in zip(after, before))
