"""mbrl_train_grads_open_loop / mbrl_train_epoch_open_loop and EnsembleModel.train_members(loss="open_loop") on
the GPU: gradients against float64 (tests/train_open_loop_reference.py) at the project's bar, losses against
mbrl_eval_members_open_loop byte for byte, and the byte-for-byte independence, epoch and argument contracts."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_open_loop_cases as tc
from test_gpu_train_ensemble import DEV, _Data, _dataset, _ensemble, _hp, _Member, _P, _scalars

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


def run_grads(mems, data, didx, fill="5a", with_loss=True, entry="mbrl_train_grads_open_loop", ws_name=None):
    """The gradient entry on device rows didx [E][batch] (gradient buffers pre-filled like the workspace): losses [E][3]."""
    _l, lib = _lib()
    E, batch = didx.shape
    tms = (_l.TrainModel * E)()
    for e, mem in enumerate(mems):
        mem.fill(tms[e])
        for g in mem.grads:
            g.fill_(NAN if fill == "nan" else -7.0 if fill == "ff" else 3.0)
    need = getattr(lib, ws_name or "mbrl_train_open_loop_workspace_bytes")(tms, E, batch)
    assert need > 0
    ws = _filled(need, fill)
    loss = torch.full((E, 3), NAN, device=DEV)
    _l.check(getattr(lib, entry)(tms, E, ctypes.byref(data.c), _P(didx), batch, _P(loss) if with_loss else None, _P(ws),
                                 ws.numel(), _l.stream_handle(DEV)), entry)
    torch.cuda.synchronize()
    return loss


@functools.lru_cache(maxsize=None)
def device_data(name):
    c, p = tc.CASES[name], tc.problem(name)
    return _Data(c.s, c.a, c.H, p["T"], 0, arrays=p["data"])


def members(name, which=None):
    c, p = tc.CASES[name], tc.problem(name)
    out = []
    for e in (range(c.E) if which is None else which):
        off = (0, 3) if (c.offset and e == 1) else ()
        out.append(_Member(c.s, c.a, c.W, c.L, c.reward, c.H, 0, values=p["members"][e], offset_params=off,
                           offset_grads=(1, 2) if off else ()))
    return out


def rows_of(name, which=None):
    r = tc.problem(name)["rows"]
    return torch.from_numpy(np.ascontiguousarray(r if which is None else r[list(which)])).to(DEV)


@functools.lru_cache(maxsize=None)
def default_run(name):
    mems = members(name)
    loss = run_grads(mems, device_data(name), rows_of(name))
    return mems, loss


def _grads_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a.grads, b.grads))


@pytest.mark.parametrize("name", tc.NAMES)
def test_gradients_match_float64(name):
    """Every weight and bias gradient of every member within 8x the float32 CPU chain's own error, tensor-relative
    and per 32 x 32 tile."""
    mems, loss = default_run(name)
    worst = 0.0
    for e, mem in enumerate(mems):
        got = [g.cpu().numpy() for g in mem.grads]
        for label, err, bar in zip(tc.tensor_names(name), tc.errors(name, got, e), tc.bars(name, e)):
            worst = max(worst, err[0] / bar[0], err[1] / bar[1])
            print(f"{name} member {e} {label}: err {err[0]:.3e} / {err[1]:.3e}  bar {bar[0]:.3e} / {bar[1]:.3e}")
            assert err[0] <= bar[0] and err[1] <= bar[1], (name, e, label, err, bar)
        want = tc.g64(name, e)["loss"]
        assert np.allclose(loss[e].cpu().numpy(), want, rtol=1e-5, atol=1e-12), (name, e, loss[e], want)
    print(f"{name}: largest error / bar = {worst:.3f}")


@pytest.mark.parametrize("name", tc.NAMES)
def test_loss_is_the_open_loop_evaluation_byte_for_byte(name):
    from test_gpu_open_loop import run_open
    mems, loss = default_run(name)
    rows = rows_of(name)
    for e, mem in enumerate(mems):
        want = run_open([mem], device_data(name), rows[e].contiguous(), with_pred=False)["loss"]
        assert np.array_equal(loss[e].cpu().numpy().view(np.int32), want[0].view(np.int32)), (name, e, loss[e], want)


def test_horizon_one_matches_the_one_step_ensemble_gradient():
    name = "h1_b17"
    mems, loss = default_run(name)
    ones = members(name)
    l1 = run_grads(ones, device_data(name), rows_of(name), entry="mbrl_train_grads_ensemble",
                   ws_name="mbrl_train_ensemble_workspace_bytes")
    for e, (a, b) in enumerate(zip(mems, ones)):
        got = [g.cpu().numpy() for g in b.grads]
        for err, bar in zip(tc.errors(name, got, e), tc.bars(name, e)):
            assert err[0] <= bar[0] and err[1] <= bar[1]
        for x, y in zip(a.grads, b.grads):
            scale = float(y.abs().max())
            assert float((x - y).abs().max()) <= 1e-5 * scale + 1e-12
    assert torch.allclose(loss, l1, rtol=1e-6)


@pytest.mark.parametrize("name", ["e5", "e8", "offset"])
def test_a_member_alone_equals_the_member_among_the_others(name):
    mems, loss = default_run(name)
    E = tc.CASES[name].E
    for e in {0, E - 1}:
        alone = members(name, [e])
        l1 = run_grads(alone, device_data(name), rows_of(name, [e]))
        assert _grads_equal(mems[e], alone[0]) and torch.equal(loss[e].view(torch.int32), l1[0].view(torch.int32))


@pytest.mark.parametrize("value", [NAN, float("inf")])
def test_a_non_finite_member_leaves_its_neighbours_alone(value):
    name = "e5"
    mems, loss = default_run(name)
    bad = members(name)
    bad[2].params[0][1, 0] = value
    lb = run_grads(bad, device_data(name), rows_of(name))
    for e in (0, 1, 3, 4):
        assert _grads_equal(mems[e], bad[e]) and torch.equal(loss[e].view(torch.int32), lb[e].view(torch.int32))
    assert not torch.isfinite(lb[2, 0]) and not all(bool(torch.isfinite(g).all()) for g in bad[2].grads)


@pytest.mark.parametrize("name", ["h7_b33", "s17_a0", "b257", "w520"])
def test_two_calls_agree_and_prior_bytes_never_matter(name):
    mems, loss = default_run(name)
    for fill in ("5a", "nan", "ff"):
        again = members(name)
        l2 = run_grads(again, device_data(name), rows_of(name), fill=fill)
        assert all(_grads_equal(a, b) for a, b in zip(mems, again)), (name, fill)
        assert torch.equal(loss.view(torch.int32), l2.view(torch.int32))
    quiet = members(name)
    run_grads(quiet, device_data(name), rows_of(name), with_loss=False)
    assert all(_grads_equal(a, b) for a, b in zip(mems, quiet))


@pytest.mark.parametrize("name", ["h3_b15", "h7_b33"])
def test_later_true_states_are_never_read(name):
    c, p = tc.CASES[name], tc.problem(name)
    mems, loss = default_run(name)
    arrays = {k: np.array(v) for k, v in p["data"].items()}
    arrays["states"][:, 1:] = NAN
    data = _Data(c.s, c.a, c.H, p["T"], 0, arrays=arrays)
    again = members(name)
    l2 = run_grads(again, data, rows_of(name))
    assert all(_grads_equal(a, b) for a, b in zip(mems, again)) and torch.equal(loss.view(torch.int32), l2.view(torch.int32))


# ---- the epoch entry
def _table(mems):
    _l, _ = _lib()
    n = len(mems[0].params)
    table = (_l.AdamTensor * (len(mems) * n))()
    for e, m in enumerate(mems):
        m.adam(table, e * n)
    return table, n


def _epoch(mems, data, orders, batch):
    """mbrl_train_epoch_open_loop over device orders [E][rows]: losses [batches][E][3]."""
    _l, lib = _lib()
    E, rows = orders.shape
    tms = (_l.TrainModel * E)()
    for e, m in enumerate(mems):
        m.fill(tms[e])
    table, n = _table(mems)
    steps = -(-rows // batch)
    ss, bc = _scalars([0] * E, steps, n)
    hp = _hp()
    need = lib.mbrl_train_open_loop_workspace_bytes(tms, E, min(batch, rows))
    ws = _filled(need, "nan")
    losses = torch.full((steps, E, 3), NAN, device=DEV)
    _l.check(lib.mbrl_train_epoch_open_loop(tms, E, ctypes.byref(data.c), _P(orders), rows, batch, table, n,
                                            ctypes.byref(hp), ss, bc, _P(losses), _P(ws), ws.numel(),
                                            _l.stream_handle(DEV)), "mbrl_train_epoch_open_loop")
    torch.cuda.synchronize()
    return losses


def _stepwise(mems, data, orders, batch):
    """The same epoch as mbrl_train_grads_open_loop + mbrl_adam_step per batch."""
    _l, lib = _lib()
    E, rows = orders.shape
    table, n = _table(mems)
    steps = -(-rows // batch)
    ss, bc = _scalars([0] * E, steps, n)
    hp = _hp()
    out = []
    for b in range(steps):
        idx = orders[:, b * batch:(b + 1) * batch].contiguous()
        keep = [[g.clone() for g in m.grads] for m in mems]
        loss = run_grads(mems, data, idx)
        del keep
        for i in range(E * n):
            table[i].step_size, table[i].bc2_sqrt = float(ss[b * E * n + i]), float(bc[b * E * n + i])
        _l.check(lib.mbrl_adam_step(table, E * n, ctypes.byref(hp), _l.stream_handle(DEV)), "mbrl_adam_step")
        torch.cuda.synchronize()
        out.append(loss)
    return torch.stack(out)


@pytest.mark.parametrize("s,a,W,L,H,reward,E", [(5, 2, 33, 2, 3, 1, 3), (17, 6, 64, 1, 2, 0, 2)])
def test_epoch_equals_its_step_by_step_equivalent(s, a, W, L, H, reward, E):
    T, batch = 45, 16                       # three batches, the last of 13 rows
    data = _Data(s, a, H, T, seed=W)
    orders = torch.from_numpy(np.random.default_rng(W).integers(0, T, size=(E, T), dtype=np.int64)).to(DEV)
    start = [_Member(s, a, W, L, reward, H, seed=10 * W + e) for e in range(E)]
    a_run, b_run = [m.clone() for m in start], [m.clone() for m in start]
    la = _epoch(a_run, data, orders, batch)
    lb = _stepwise(b_run, data, orders, batch)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    for x, y in zip(a_run, b_run):
        for k in ("params", "m", "v", "grads"):
            for p, q in zip(getattr(x, k), getattr(y, k)):
                assert torch.equal(p.view(torch.int32), q.view(torch.int32)), k
    assert not torch.equal(a_run[0].params[0], start[0].params[0])


# ---- argument checks
def test_argument_errors_come_before_any_launch():
    _l, lib = _lib()
    s, a, W, L, H, reward, E, batch = 5, 2, 33, 2, 3, 1, 2, 17
    data = _Data(s, a, H, 30, seed=1)
    mems = [_Member(s, a, W, L, reward, H, seed=e) for e in range(E)]
    didx = torch.arange(E * batch, device=DEV).remainder(30).reshape(E, batch).contiguous()
    st = _l.stream_handle(DEV)

    def tms_of(ms):
        t = (_l.TrainModel * len(ms))()
        for e, m in enumerate(ms):
            m.fill(t[e])
        return t
    tms = tms_of(mems)
    need = lib.mbrl_train_open_loop_workspace_bytes(tms, E, batch)
    ws = _filled(need, "5a")
    loss = torch.full((E, 3), 5.0, device=DEV)
    for m in mems:
        for g in m.grads:
            g.fill_(9.0)

    def call(t=tms, e=E, d=data.c, idx=didx, b=batch, w=ws, n=None):
        return lib.mbrl_train_grads_open_loop(t, e, ctypes.byref(d) if d is not None else None,
                                              _P(idx) if idx is not None else None, b, _P(loss),
                                              _P(w) if w is not None else None, w.numel() if n is None else n, st)
    EINVAL, EUNSUP, EWS = _l.MBRL_EINVAL, _l.MBRL_EUNSUPPORTED, _l.MBRL_EWORKSPACE
    other = tms_of([mems[0], _Member(s, a, W + 1, L, reward, H, seed=5)])
    twice = tms_of(mems)
    twice[1].bias_grad[0] = twice[0].bias_grad[0]
    nulled = tms_of(mems)
    nulled[1].weight_grad[1] = None
    nodata = _l.TrainData()
    nodata.states, nodata.actions, nodata.rewards = data.c.states, data.c.actions, data.c.rewards
    nodata.transitions = data.c.transitions           # (next_states stays NULL)
    big = tms_of(mems)
    for t in big:
        t.hidden, t.n_hidden = 1024, 8
    many = tms_of([_Member(s, a, W, L, reward, H, seed=e) for e in range(9)])
    cases = [(call(t=other), EINVAL), (call(t=twice), EINVAL), (call(t=nulled), EINVAL), (call(t=None), EINVAL),
             (call(d=None), EINVAL), (call(d=nodata), EINVAL), (call(idx=None), EINVAL), (call(w=None, n=need), EINVAL),
             (call(e=0), EINVAL), (call(b=0), EINVAL), (call(b=31), EINVAL), (call(t=many, e=9), EUNSUP),
             (call(t=big), EUNSUP), (call(n=need - 1), EWS)]
    torch.cuda.synchronize()
    for i, (rc, want) in enumerate(cases):
        assert rc == want, (i, rc, want)
    assert lib.mbrl_train_open_loop_workspace_bytes(other, E, batch) == 0
    assert lib.mbrl_train_open_loop_workspace_bytes(big, E, batch) == 0
    assert bool((loss == 5.0).all()) and bool((ws == 0x5A).all())
    assert all(bool((g == 9.0).all()) for m in mems for g in m.grads)
    # the epoch entry: the same codes
    table, n = _table(mems)
    ss, bc = _scalars([0] * E, 2, n)
    hp = _hp()
    orders = didx

    def epoch(t=tms, tab=table, w=ws, nbytes=None, rows=batch, hpp=hp):
        return lib.mbrl_train_epoch_open_loop(t, E, ctypes.byref(data.c), _P(orders), rows, 16, tab, n,
                                              ctypes.byref(hpp) if hpp is not None else None,
                                              ss, bc, None, _P(w), w.numel() if nbytes is None else nbytes, st)
    need16 = lib.mbrl_train_open_loop_workspace_bytes(tms, E, 16)
    for rc, want in [(epoch(t=other), EINVAL), (epoch(t=twice), EINVAL), (epoch(tab=None), EINVAL),
                     (epoch(hpp=None), EINVAL), (epoch(rows=0), EINVAL), (epoch(rows=31), EINVAL),
                     (epoch(t=big), EUNSUP), (epoch(nbytes=need16 - 1), EWS)]:
        assert rc == want, (rc, want)
    torch.cuda.synchronize()
    assert all(bool((g == 9.0).all()) for m in mems for g in m.grads) and bool((ws == 0x5A).all())
    assert all(bool((x == 0).all()) for m in mems for x in m.m + m.v)


# ---- Python
def _sets():
    return _dataset(5, 2, 3, 96, seed=3), _dataset(5, 2, 3, 40, seed=4)


def _adam_for(ens):
    return [torch.optim.Adam(m.parameters(), lr=1e-3) for m in ens.members]


def _params(ens):
    return [p.detach().clone() for p in ens.parameters()]


class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, it):
        self.rows.append((tag, float(value), it))


def test_train_members_open_loop_matches_its_fallback_and_leaves_numpy_rng_alone(monkeypatch):
    from mbrl_amd import models
    train, _ = _sets()
    a, b = _ensemble(3, 5, 2, 32, seed=1), None
    b = copy.deepcopy(a)
    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    wa, wb = _Writer(), _Writer()
    ran = a.train_members(train, _adam_for(a), batch_size=32, num_epochs=3, seed=5, loss="open_loop", writer=wa)
    assert ran == 3
    assert np.array_equal(np.random.get_state()[1], before)
    monkeypatch.setattr(models, "NATIVE_TRAINING", False)
    assert b.train_members(train, _adam_for(b), batch_size=32, num_epochs=3, seed=5, loss="open_loop", writer=wb) == 0
    for p, q in zip(_params(a), _params(b)):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-4 * float(q.abs().max())), float((p - q).abs().max())
    ra, rb = (sorted(w.rows, key=lambda r: (r[0], r[2])) for w in (wa, wb))       # (batch-major against member-major)
    assert [(r[0], r[2]) for r in ra] == [(r[0], r[2]) for r in rb] and len(ra) == 3 * 3 * 3
    assert np.allclose([r[1] for r in ra], [r[1] for r in rb], rtol=1e-3)
    with pytest.raises(ValueError):
        a.train_members(train, _adam_for(a), loss="two_step")
    with pytest.raises(ValueError):
        a.fit_members(train, train, _adam_for(a), train_loss="two_step")


def test_open_loop_training_differs_from_teacher_forcing_and_defaults_are_unchanged():
    train, _ = _sets()
    start = _ensemble(2, 5, 2, 32, seed=2)
    runs = []
    for kw in ({}, {}, {"loss": "one_step"}, {"loss": "open_loop"}):
        e = copy.deepcopy(start)
        opts = _adam_for(e)
        e.train_members(train, opts, batch_size=32, num_epochs=2, seed=1, **kw)
        state = [t.clone() for o in opts for st in o.state.values() for t in (st["exp_avg"], st["exp_avg_sq"])]
        runs.append(_params(e) + state)
    for x, y, z in zip(runs[0], runs[1], runs[2]):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert any(not torch.equal(x, y) for x, y in zip(runs[0], runs[3]))


def test_fit_members_open_loop_rows_are_evaluate_members_after_as_many_epochs():
    train, hold = _sets()
    start = _ensemble(2, 5, 2, 32, seed=3)
    fit = copy.deepcopy(start)
    rep = fit.fit_members(train, hold, _adam_for(fit), batch_size=32, max_epochs=3, seed=2, restore_best=False,
                          train_loss="open_loop", holdout_loss="open_loop")
    assert rep["native_epochs"] == 3 and rep["epochs_run"] == 3
    # train_members draws epoch k's rows from (seed, e, k): one call of 3 epochs, evaluated after each prefix
    for k in range(3):
        run = copy.deepcopy(start)
        run.train_members(train, _adam_for(run), batch_size=32, num_epochs=k + 1, seed=2, loss="open_loop")
        want = run.evaluate_members(hold, open_loop=True)["loss"].cpu()
        assert torch.equal(rep["val_loss"][k], want), (k, rep["val_loss"][k], want)


def test_plan_after_open_loop_training_uses_the_new_weights():
    """A CEM plan after train_members(loss="open_loop") equals the plan of a freshly built EnsembleModel holding
    the trained weights, and differs from the plan before training."""
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
                      num_epochs=3, seed=2, loss="open_loop")
    after = plan(ens)
    fresh = _ensemble(2, s, a, W, seed=7)
    fresh.load_state_dict(copy.deepcopy(ens.state_dict()))
    want = plan(fresh)
    assert all(torch.equal(x, y) for x, y in zip(after, want))
    assert not all(torch.equal(x, y) for x, y in zip(after, before))
