"""Ensemble training on the GPU: mbrl_train_epoch_ensemble / mbrl_train_grads_ensemble (csrc/train_api.hip;
csrc/train.hip: the members on a grid axis of the multi-launch layout) against mbrl_train_epoch / mbrl_train_grads on each
member alone with its own row order. The contract is equality bit for bit -- parameters, Adam state, the
last gradients and every batch's losses -- so every comparison below is torch.equal on the raw tensors.
Then EnsembleModel.train_members (the Python entry) against its member-by-member fallback, and the
argument checks, which must return before any launch."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


class _Data:
    """Stacked transitions [T][H][.] as the C entries read them."""

    def __init__(self, s, a, H, T, seed, arrays=None):
        """arrays: the transitions themselves (states / actions / next_states [T][H][.], rewards [T][H] as
        NumPy) instead of the seeded draw. a = 0: the C struct's actions pointer is NULL."""
        from mbrl_amd import _lib
        g = torch.Generator().manual_seed(seed)
        if arrays is None:
            self.states = torch.randn((T, H, s), generator=g).to(DEV)
            self.actions = torch.rand((T, H, a), generator=g).mul(2).sub(1).to(DEV)
            self.next_states = torch.randn((T, H, s), generator=g).to(DEV)
            self.rewards = torch.randn((T, H), generator=g).to(DEV)
        else:
            self.states, self.actions, self.next_states, self.rewards = [
                torch.from_numpy(np.array(arrays[k], np.float32)).to(DEV)
                for k in ("states", "actions", "next_states", "rewards")]
            assert self.states.shape == (T, H, s) and self.actions.shape == (T, H, a)
            assert self.next_states.shape == (T, H, s) and self.rewards.shape == (T, H)
        self.T = T
        d = self.c = _lib.TrainData()
        d.states, d.actions, d.next_states, d.rewards = [x.data_ptr() for x in (self.states, self.actions,
                                                                                 self.next_states, self.rewards)]
        if a == 0:
            d.actions = None
        d.transitions = T


def _offset_like(t):
    """A copy of t as a view 4 bytes into a larger buffer: data_ptr() % 16 == 4."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


class _Member:
    """One member's tensors: every Linear's weight and bias, their gradients and Adam state."""

    def __init__(self, s, a, W, L, reward, H, seed, values=None, offset_params=(), offset_grads=()):
        """values: the parameters (NumPy, in params' order) instead of the seeded draw. offset_params /
        offset_grads: indices into params / grads of the tensors allocated as views 4 bytes into a larger
        buffer (_offset_like), so that their pointers are not 16-byte aligned."""
        g = torch.Generator().manual_seed(seed)
        dims = [(W, s + a)] + [(W, W)] * (L - 1) + [(s, W)] + ([(1, W)] if reward else [])
        self.shape = (s, a, W, L, int(reward), H)
        self.params = []
        for fo, fi in dims:
            bound = 1.0 / fi ** 0.5
            self.params.append(torch.rand((fo, fi), generator=g).mul(2 * bound).sub(bound).to(DEV))
            self.params.append(torch.rand((fo,), generator=g).mul(2 * bound).sub(bound).to(DEV))
        if values is not None:
            assert [tuple(v.shape) for v in values] == [tuple(p.shape) for p in self.params]
            self.params = [torch.from_numpy(np.array(v, np.float32)).to(DEV) for v in values]
        self.grads = [torch.zeros_like(p) for p in self.params]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        for i in offset_params:
            self.params[i] = _offset_like(self.params[i])
        for i in offset_grads:
            self.grads[i] = _offset_like(self.grads[i])

    def clone(self):
        c = copy.copy(self)
        for k in ("params", "grads", "m", "v"):
            setattr(c, k, [_offset_like(t) if t.data_ptr() % 16 else t.clone() for t in getattr(self, k)])
        return c

    def fill(self, tm):
        tm.state_dim, tm.action_dim, tm.hidden, tm.n_hidden, tm.reward_head, tm.horizon = self.shape
        for i in range(len(self.params) // 2):
            tm.weight[i], tm.bias[i] = self.params[2 * i].data_ptr(), self.params[2 * i + 1].data_ptr()
            tm.weight_grad[i], tm.bias_grad[i] = self.grads[2 * i].data_ptr(), self.grads[2 * i + 1].data_ptr()

    def adam(self, table, at):
        for i, (p, g, m, v) in enumerate(zip(self.params, self.grads, self.m, self.v)):
            t = table[at + i]
            t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), \
                p.numel()

    def tensors(self):
        return self.params + self.grads + self.m + self.v


def _scalars(first_steps, steps, n, lrs=None):
    """step_sizes / bc2_sqrt [steps][members * n] of `steps` Adam steps (adam.py): member j has done
    first_steps[j] steps before and steps at the rate lrs[j]; n tensors per member."""
    lrs = lrs or [LR] * len(first_steps)
    ss, bc = [], []
    for i in range(1, steps + 1):
        for first, lr in zip(first_steps, lrs):
            k = first + i
            ss += [(lr / (1 - B1 ** k)) * -1] * n
            bc += [(1 - B2 ** k) ** 0.5] * n
    return (ctypes.c_float * len(ss))(*ss), (ctypes.c_float * len(bc))(*bc)


def _hp(wd=0.0):
    from mbrl_amd import _lib
    return _lib.AdamHparams(1 - B1, B2, 1 - B2, EPS, wd)


def _orders(E, T, epochs, seed=0):
    """Bootstrap orders [epochs][E][T] (mbrl_amd.models.member_order): draws with replacement."""
    from mbrl_amd import models
    o = np.stack([np.stack([models.member_order(seed, e, k, T) for e in range(E)]) for k in range(epochs)])
    assert all(len(np.unique(o[k, e])) < T for k in range(epochs) for e in range(E))   # visible repeats
    return o


def _single_epochs(mem, data, orders, batch, wd=0.0, lr=LR, step0=0, make_ws=None, alloc=None):
    """mbrl_train_epoch on one member, one call per epoch; returns the losses [epochs][batches][3].
    make_ws(nbytes) -> the uint8 workspace (zeroed by its maker: the single-model contract) and
    alloc(*shape) -> an output tensor replace the private allocations (tests/workspace_cases.py)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    tm = _lib.TrainModel()
    mem.fill(tm)
    n = len(mem.params)
    table = (_lib.AdamTensor * n)()
    mem.adam(table, 0)
    need = lib.mbrl_train_workspace_bytes(ctypes.byref(tm), batch)
    ws = make_ws(need) if make_ws else torch.zeros(need, dtype=torch.uint8, device=DEV)
    rows = orders.shape[1]
    steps = (rows + batch - 1) // batch
    hp = _hp(wd)
    out = []
    for k in range(orders.shape[0]):
        order = torch.from_numpy(orders[k]).to(DEV)
        losses = alloc(steps, 3) if alloc else torch.zeros((steps, 3), device=DEV)
        ss, bc = _scalars([step0 + k * steps], steps, n, [lr])
        _lib.check(lib.mbrl_train_epoch(ctypes.byref(tm), ctypes.byref(data.c), _P(order), rows, batch, table, n,
                                        ctypes.byref(hp), ss, bc, _P(losses), _P(ws), ws.numel(),
                                        _lib.stream_handle(DEV)), "mbrl_train_epoch")
        torch.cuda.synchronize()
        out.append(losses)
    return torch.stack(out)


def _ensemble_epochs(mems, data, orders, batch, wd=0.0, lrs=None, step0s=None, make_ws=None, alloc=None):
    """mbrl_train_epoch_ensemble on the members, one call per epoch; losses [epochs][batches][E][3].
    orders: [epochs][E][rows]. make_ws / alloc: as _single_epochs' (this workspace needs no zeroing)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    E = len(mems)
    tms = (_lib.TrainModel * E)()
    n = len(mems[0].params)
    table = (_lib.AdamTensor * (E * n))()
    for e, mem in enumerate(mems):
        mem.fill(tms[e])
        mem.adam(table, e * n)
    need = lib.mbrl_train_ensemble_workspace_bytes(tms, E, batch)
    assert need > 0
    # the workspace needs no zeroing
    ws = make_ws(need) if make_ws else torch.empty(need, dtype=torch.uint8, device=DEV).fill_(0xA5)
    rows = orders.shape[2]
    steps = (rows + batch - 1) // batch
    hp = _hp(wd)
    out = []
    for k in range(orders.shape[0]):
        order = torch.from_numpy(np.ascontiguousarray(orders[k])).to(DEV)
        losses = alloc(steps, E, 3) if alloc else torch.zeros((steps, E, 3), device=DEV)
        ss, bc = _scalars([s0 + k * steps for s0 in (step0s or [0] * E)], steps, n, lrs)
        _lib.check(lib.mbrl_train_epoch_ensemble(tms, E, ctypes.byref(data.c), _P(order), rows, batch, table, n,
                                                 ctypes.byref(hp), ss, bc, _P(losses), _P(ws), ws.numel(),
                                                 _lib.stream_handle(DEV)), "mbrl_train_epoch_ensemble")
        torch.cuda.synchronize()
        out.append(losses)
    return torch.stack(out)


def _assert_member_equal(got, want, what):
    names = ["param", "grad", "exp_avg", "exp_avg_sq"]
    n = len(got.params)
    for i, (x, y) in enumerate(zip(got.tensors(), want.tensors())):
        assert torch.equal(x, y), (what, names[i // n], i % n, float((x - y).abs().max()))


SHAPES = [(3, 1, 16, 2), (5, 2, 50, 2), (4, 1, 64, 1), (4, 2, 32, 3)]
T, BATCH, EPOCHS = 70, 32, 2          # two full batches and a short one of 6, twice


@pytest.mark.parametrize("reward", [0, 1])
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("s,a,W,L", SHAPES)
@pytest.mark.parametrize("E", [1, 2, 5])
def test_epoch_ensemble_equals_each_member_alone(E, s, a, W, L, H, reward):
    """Every member of the shared launches ends where mbrl_train_epoch leaves that member trained alone
    on its own bootstrap order: parameters, exp_avg, exp_avg_sq, the last gradients and all per-batch
    losses byte-equal. E = 1 is the single call itself."""
    data = _Data(s, a, H, T, seed=s * 100 + W)
    orders = _orders(E, T, EPOCHS, seed=W)
    start = [_Member(s, a, W, L, reward, H, seed=10 * W + e) for e in range(E)]
    ens = [m.clone() for m in start]
    losses = _ensemble_epochs(ens, data, orders, BATCH)
    assert bool(torch.isfinite(losses).all())
    for e in range(E):
        alone = start[e].clone()
        want = _single_epochs(alone, data, orders[:, e], BATCH)
        _assert_member_equal(ens[e], alone, f"member {e}")
        assert torch.equal(losses[:, :, e], want), (e, losses[:, :, e], want)
        assert not torch.equal(alone.params[0], start[e].params[0])      # it did train


@pytest.mark.parametrize("T_,batch", [(T, BATCH), (230, 96)])
def test_single_model_layouts_agree_with_the_ensemble(T_, batch):
    """The single-model side in both of its layouts (MBRL_OPT_TRAIN_SPLIT = 0: the fused step where it
    applies -- two hidden layers and batch rows in (64, 128] at batch 96 -- and 1: the multi-launch
    layout) gives the bits the ensemble launches give, with weight decay on. Every member has its own
    learning rate and its own count of earlier steps, so each tensor's step_size and bc2_sqrt differ
    between the members: a mix-up of the [batches][E * count] scalars would show."""
    from mbrl_amd import _lib
    s, a, W, L, H, reward, E = 5, 2, 50, 2, 1, 0, 3
    lrs, step0s = [1e-3, 3e-3, 2e-4], [0, 7, 40]
    data = _Data(s, a, H, T_, seed=77)
    orders = _orders(E, T_, EPOCHS, seed=5)
    start = [_Member(s, a, W, L, reward, H, seed=40 + e) for e in range(E)]
    ens = [m.clone() for m in start]
    losses = _ensemble_epochs(ens, data, orders, batch, wd=1e-4, lrs=lrs, step0s=step0s)
    for split in (0, 1):
        with _lib.option("train_split", split):
            for e in range(E):
                alone = start[e].clone()
                want = _single_epochs(alone, data, orders[:, e], batch, wd=1e-4, lr=lrs[e], step0=step0s[e])
                _assert_member_equal(ens[e], alone, f"split {split} member {e}")
                assert torch.equal(losses[:, :, e], want), (split, e)


def _grads_ensemble(mems, data, didx, make_ws=None, alloc=None):
    """mbrl_train_grads_ensemble on device rows didx [E][batch]: the losses [E][3] (make_ws / alloc: as
    _single_epochs')."""
    from mbrl_amd import _lib
    lib = _lib.load()
    E, batch = didx.shape
    tms = (_lib.TrainModel * E)()
    for e, mem in enumerate(mems):
        mem.fill(tms[e])
    need = lib.mbrl_train_ensemble_workspace_bytes(tms, E, batch)
    ws = make_ws(need) if make_ws else torch.empty(need, dtype=torch.uint8, device=DEV).fill_(0x5A)
    loss = alloc(E, 3) if alloc else torch.zeros((E, 3), device=DEV)
    _lib.check(lib.mbrl_train_grads_ensemble(tms, E, ctypes.byref(data.c), _P(didx), batch, _P(loss), _P(ws), ws.numel(),
                                             _lib.stream_handle(DEV)), "mbrl_train_grads_ensemble")
    torch.cuda.synchronize()
    return loss


def _grads_single(mem, data, rows, make_ws=None, alloc=None):
    """mbrl_train_grads on one member and device rows [batch]: its loss [3]."""
    from mbrl_amd import _lib
    lib = _lib.load()
    batch = rows.numel()
    tm = _lib.TrainModel()
    mem.fill(tm)
    need = lib.mbrl_train_workspace_bytes(ctypes.byref(tm), batch)
    ws1 = make_ws(need) if make_ws else torch.zeros(need, dtype=torch.uint8, device=DEV)
    l1 = alloc(3) if alloc else torch.zeros(3, device=DEV)
    _lib.check(lib.mbrl_train_grads(ctypes.byref(tm), ctypes.byref(data.c), _P(rows), batch, _P(l1), _P(ws1),
                                    ws1.numel(), _lib.stream_handle(DEV)), "mbrl_train_grads")
    torch.cuda.synchronize()
    return l1


def _grads_calls(mems, data, idx):
    """mbrl_train_grads_ensemble on rows idx [E][batch]; then mbrl_train_grads per member on clones.
    Returns (ensemble losses [E][3], [(clone, its loss [3])])."""
    clones = [m.clone() for m in mems]
    didx = torch.from_numpy(np.ascontiguousarray(idx)).to(DEV)
    loss = _grads_ensemble(mems, data, didx)
    return loss, [(c, _grads_single(c, data, didx[e])) for e, c in enumerate(clones)]


@pytest.mark.parametrize("s,a,W,L,H,reward,batch", [(5, 2, 50, 2, 2, 1, 37), (4, 1, 64, 1, 1, 0, 32),
                                                   (6, 3, 96, 2, 1, 0, 100)])
def test_grads_ensemble_equals_train_grads(s, a, W, L, H, reward, batch):
    """One batch's gradients and losses per member, byte-equal to mbrl_train_grads on that member; member 1's
    rows are all the same index (a batch of one repeated transition)."""
    E = 3
    data = _Data(s, a, H, 120, seed=batch)
    rng = np.random.default_rng(batch)
    idx = rng.integers(0, 120, size=(E, batch), dtype=np.int64)
    idx[1, :] = 7
    mems = [_Member(s, a, W, L, reward, H, seed=3 * W + e) for e in range(E)]
    loss, singles = _grads_calls(mems, data, idx)
    for e, (c, l1) in enumerate(singles):
        _assert_member_equal(mems[e], c, f"member {e}")
        assert torch.equal(loss[e], l1), (e, loss[e], l1)
        assert float(mems[e].grads[0].abs().max()) > 0


def test_members_are_independent():
    """Changing member 1's order and initial weights changes no bit of member 0's results."""
    s, a, W, L, H, reward = 5, 2, 50, 2, 2, 1
    data = _Data(s, a, H, T, seed=1)
    orders = _orders(2, T, EPOCHS, seed=9)
    start = [_Member(s, a, W, L, reward, H, seed=e) for e in range(2)]
    a_run = [m.clone() for m in start]
    la = _ensemble_epochs(a_run, data, orders, BATCH)
    other = orders.copy()
    other[:, 1] = _orders(2, T, EPOCHS, seed=10)[:, 0]
    b_run = [start[0].clone(), _Member(s, a, W, L, reward, H, seed=99)]
    lb = _ensemble_epochs(b_run, data, other, BATCH)
    _assert_member_equal(a_run[0], b_run[0], "member 0")
    assert torch.equal(la[:, :, 0], lb[:, :, 0])
    assert not torch.equal(a_run[1].params[0], b_run[1].params[0])


def test_ensemble_gradients_match_float64_autograd():
    """Member gradients after one batch against float64 autograd of the same loss on the same rows (with
    the bootstrap's repeats), at the bar of tests/test_gpu_train_native.py: within 1e-4 relative plus 1e-4
    of the tensor's largest reference entry; losses within 1e-5 relative."""
    s, a, W, L, H, reward, E, batch = 5, 2, 50, 2, 2, 1, 2, 32
    data = _Data(s, a, H, T, seed=4)
    idx = _orders(E, T, 1, seed=3)[0][:, :batch]
    mems = [_Member(s, a, W, L, reward, H, seed=20 + e) for e in range(E)]
    loss, _ = _grads_calls(mems, data, idx)
    for e, mem in enumerate(mems):
        ps = [p.double().requires_grad_(True) for p in mem.params]
        rows = torch.from_numpy(idx[e]).to(DEV)
        total = 0.0
        for h in range(H):
            x = torch.cat([data.states[rows, h], data.actions[rows, h]], dim=1).double()
            for l in range(L):
                x = torch.relu(x @ ps[2 * l].T + ps[2 * l + 1])
            ys = x @ ps[2 * L].T + ps[2 * L + 1]
            yr = x @ ps[2 * L + 2].T + ps[2 * L + 3]
            total = total + torch.nn.functional.mse_loss(ys, data.next_states[rows, h].double()) + \
                torch.nn.functional.mse_loss(yr, data.rewards[rows, h].double().reshape(-1, 1))
        ref = torch.autograd.grad(total, ps)
        for i, (x, y) in enumerate(zip(mem.grads, ref)):
            y = y.float()
            scale = float(y.abs().max())
            assert torch.allclose(x, y, rtol=1e-4, atol=1e-4 * scale + 1e-12), (e, i, float((x - y).abs().max()), scale)
        total = float(total.detach())
        assert abs(float(loss[e, 0]) - total) <= 1e-5 * abs(total)


# ---- argument checks: each returns its code with a message before any launch (the parameters, the
# gradients and the Adam state are untouched)

def _call_epoch(tms, E, data, order, rows, batch, table, n, ws, ws_bytes=None, data_c=None):
    from mbrl_amd import _lib
    lib = _lib.load()
    steps = (rows + batch - 1) // batch
    ss, bc = _scalars([0] * max(E, 1), steps, n)
    hp = _hp()
    rc = lib.mbrl_train_epoch_ensemble(tms, E, ctypes.byref(data.c) if data_c is None else data_c,
                                       None if order is None else _P(order), rows, batch, table, n, ctypes.byref(hp),
                                       ss, bc, None, _P(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                       _lib.stream_handle(DEV))
    msg = lib.mbrl_last_error()
    return rc, (msg.decode() if msg else "")


def test_argument_checks_come_before_any_launch():
    from mbrl_amd import _lib
    lib = _lib.load()
    s, a, W, L, H, reward = 4, 2, 32, 2, 1, 0
    data = _Data(s, a, H, T, seed=2)
    EMAX = _lib.TRAIN_MAX_MEMBERS
    mems = [_Member(s, a, W, L, reward, H, seed=e) for e in range(EMAX + 1)]
    for m in mems:                       # a gradient and a state that a launch would overwrite
        for t in m.grads + m.m:
            t.fill_(3.0)
    before = [[t.clone() for t in m.tensors()] for m in mems]
    n = len(mems[0].params)

    def bind(members):
        tms = (_lib.TrainModel * len(members))()
        table = (_lib.AdamTensor * (len(members) * n))()
        for e, m in enumerate(members):
            m.fill(tms[e])
            m.adam(table, e * n)
        return tms, table
    tms, table = bind(mems[:2])
    order = torch.from_numpy(_orders(2, T, 1)[0]).to(DEV)
    ws = torch.empty(lib.mbrl_train_ensemble_workspace_bytes(tms, 2, BATCH), dtype=torch.uint8, device=DEV)
    assert lib.mbrl_train_ensemble_workspace_bytes(tms, 0, BATCH) == 0
    assert lib.mbrl_train_ensemble_workspace_bytes(tms, 2, 0) == 0
    cases = []
    cases.append(("E < 1", _lib.MBRL_EINVAL, _call_epoch(tms, 0, data, order, T, BATCH, table, n, ws)))
    big_tms, big_table = bind(mems)
    cases.append(("E above the bound", _lib.MBRL_EUNSUPPORTED,
                  _call_epoch(big_tms, EMAX + 1, data, order, T, BATCH, big_table, n, ws)))
    assert lib.mbrl_train_ensemble_workspace_bytes(big_tms, EMAX + 1, BATCH) == 0
    odd = _Member(s, a, W + 1, L, reward, H, seed=5)
    odd_tms, odd_table = bind([mems[0], odd])
    cases.append(("shapes differ", _lib.MBRL_EINVAL, _call_epoch(odd_tms, 2, data, order, T, BATCH, odd_table, n, ws)))
    assert lib.mbrl_train_ensemble_workspace_bytes(odd_tms, 2, BATCH) == 0
    cases.append(("NULL orders", _lib.MBRL_EINVAL, _call_epoch(tms, 2, data, None, T, BATCH, table, n, ws)))
    nodata = _lib.TrainData()
    nodata.transitions = T
    cases.append(("NULL states", _lib.MBRL_EINVAL,
                  _call_epoch(tms, 2, data, order, T, BATCH, table, n, ws, data_c=ctypes.byref(nodata))))
    null_tms, null_table = bind(mems[:2])
    null_tms[1].bias_grad[1] = None
    cases.append(("NULL gradient", _lib.MBRL_EINVAL, _call_epoch(null_tms, 2, data, order, T, BATCH, null_table, n, ws)))
    null_table[n + 1].exp_avg = None
    cases.append(("NULL Adam state", _lib.MBRL_EINVAL, _call_epoch(tms, 2, data, order, T, BATCH, null_table, n, ws)))
    for what in ("weight", "bias_grad"):
        dup_tms, dup_table = bind(mems[:2])
        getattr(dup_tms[1], what)[0] = getattr(dup_tms[0], what)[0]
        cases.append((f"shared {what}", _lib.MBRL_EINVAL,
                      _call_epoch(dup_tms, 2, data, order, T, BATCH, dup_table, n, ws)))
    cases.append(("small workspace", _lib.MBRL_EWORKSPACE,
                  _call_epoch(tms, 2, data, order, T, BATCH, table, n, ws, ws_bytes=ws.numel() - 1)))
    # the gradient entry shares the checks
    loss = torch.zeros((2, 3), device=DEV)
    dup_tms, _ = bind(mems[:2])
    dup_tms[1].weight_grad[2] = dup_tms[0].weight_grad[2]
    for what, want, args in [("grads: E above the bound", _lib.MBRL_EUNSUPPORTED, (big_tms, EMAX + 1, ws.numel())),
                             ("grads: shared gradient", _lib.MBRL_EINVAL, (dup_tms, 2, ws.numel())),
                             ("grads: small workspace", _lib.MBRL_EWORKSPACE, (tms, 2, 16))]:
        rc = lib.mbrl_train_grads_ensemble(args[0], args[1], ctypes.byref(data.c), _P(order), BATCH, _P(loss), _P(ws),
                                           args[2], _lib.stream_handle(DEV))
        msg = lib.mbrl_last_error()
        cases.append((what, want, (rc, msg.decode() if msg else "")))
    torch.cuda.synchronize()
    for what, want, (rc, msg) in cases:
        assert rc == want, (what, rc, msg)
        assert "ensemble" in msg or "train" in msg, (what, msg)
    for m, snap in zip(mems + [odd], before + [None]):
        if snap is not None:
            assert all(torch.equal(x, y) for x, y in zip(m.tensors(), snap))
    assert float(loss.abs().max()) == 0.0


# ---- Python: EnsembleModel.train_members

def _dataset(s, a, horizon, T_, seed):
    from mbrl_amd import data
    rng = np.random.Generator(np.random.PCG64(seed))
    rolls = []
    per = T_ // 3 + horizon
    for _ in range(3):
        st = rng.standard_normal((per + 1, s)).astype(np.float32)
        rolls.append(data.Rollout(states=list(torch.from_numpy(st)), observations=list(torch.from_numpy(st)),
                                  actions=list(torch.from_numpy(rng.uniform(-1, 1, (per, a)).astype(np.float32))),
                                  rewards=list(torch.from_numpy(rng.standard_normal(per).astype(np.float32)))))
    ds = data.TransitionsDataset(rollouts=rolls, horizon=horizon)
    ds.set_data_mode("state_only")
    return ds


def _ensemble(E, s, a, W, seed):
    from mbrl_amd import models
    torch.manual_seed(seed)
    return models.EnsembleModel([models.Model(s, a, hidden_units=W) for _ in range(E)]).to(DEV)


class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def test_train_members_matches_its_fallback_and_leaves_numpy_rng_alone(monkeypatch):
    """train_members through mbrl_train_epoch_ensemble against the member-by-member fallback (autograd) on
    the same seed, every member at its own learning rate: parameters within the 1e-4 the README states for
    train_model against the reference.
    The global NumPy RNG state is the same after the call; the writer gets one value per member and
    batch; the counters advance once."""
    from mbrl_amd import models
    ds = _dataset(6, 2, 2, 300, seed=3)
    calls = []
    real = models._NativeEnsemble.epoch
    monkeypatch.setattr(models._NativeEnsemble, "epoch", lambda self, *a: calls.append(1) or real(self, *a))
    out = {}
    for native in (True, False):
        ens = _ensemble(3, 6, 2, 48, seed=0)
        w = _Writer()
        monkeypatch.setattr(models, "NATIVE_TRAINING", native)
        np.random.seed(11)
        state = np.random.get_state()
        opts = [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(ens.members, (1e-3, 3e-3, 3e-4))]
        ran = ens.train_members(ds, opts, batch_size=64, num_epochs=4, seed=5, writer=w)
        assert ran == (4 if native else 0)
        torch.cuda.synchronize()
        after = np.random.get_state()
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        assert ens.train_iterations == 1 and all(m.train_iterations == 1 for m in ens.members)
        out[native] = ([p.detach().cpu() for p in ens.parameters()], w.rows)
    assert len(calls) == 4                                    # the native path ran, one call per epoch
    steps = 4 * ((ds.num_transitions() + 63) // 64)
    for native in (True, False):
        tags = sorted({r[0] for r in out[native][1]})
        assert tags == [f"loss/state/member{e}/0" for e in range(3)] and len(out[native][1]) == 3 * steps
    for x, y in zip(out[True][0], out[False][0]):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-5), float((x - y).abs().max())   # (tests/test_train.py's)
    members = [out[True][0][i * 6:(i + 1) * 6] for i in range(3)]
    assert not torch.equal(members[0][0], members[1][0])


def test_plan_after_train_members_sees_the_new_weights():
    """A CEM plan after train_members equals the plan of a freshly built EnsembleModel holding the trained
    weights (the fused planner's weight pack was refreshed), and differs from the plan before training."""
    from mbrl_amd import CEMPlanner, env, models
    s, a, W = 6, 2, 48
    ds = _dataset(s, a, 1, 300, seed=8)
    ens = _ensemble(2, s, a, W, seed=1)
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(s), torch.zeros(s), 0.4), models.CoshLoss(0.25))
    sample = env.sample_action_fn(env.BoundedActionSpec(a, -1.0, 1.0))
    s0 = torch.linspace(-1, 1, s)

    def plan(module):
        res = CEMPlanner.plan_detailed(s0, module, cost, sample, 5, num_candidates=256, num_iterations=2, seed=3,
                                       device="cuda:0")
        return [res[k].detach().cpu().clone() for k in ("actions", "mu", "sigma")]
    before = plan(ens)
    ens.train_members(ds, [torch.optim.Adam(m.parameters(), lr=3e-3) for m in ens.members], batch_size=64,
                      num_epochs=3, seed=2)
    after = plan(ens)
    fresh = _ensemble(2, s, a, W, seed=7)
    fresh.load_state_dict(copy.deepcopy(ens.state_dict()))
    want = plan(fresh)
    assert all(torch.equal(x, y) for x, y in zip(after, want))
    assert not all(torch.equal(x, y) for x, y in zip(after, before))
