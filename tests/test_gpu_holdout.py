"""GPU: held-out evaluation and keep-best snapshots (csrc/eval.hip: mbrl_eval_members, mbrl_keep_best) and
EnsembleModel.evaluate_members / fit_members / elite on top of them.

Accuracy: over tests/holdout_cases.py, row_err, row_rew_err and loss_out against the float64 restatement of
tests/holdout_reference.py at the project's native-gradient bar -- the tensor-relative error
(train_grad_reference.err) within 8 x max(the float32 CPU chain's error on that tensor, the table's median of
it) -- and loss_out against mbrl_train_grads_ensemble's on the same rows at the same bar. Everything else is
equality byte for byte. On an MI355X the largest e(gpu) / bar over the table is 0.35 (s1_a0's total loss:
1.1e-7 against 3.1e-7); the row errors use at most 0.31 of theirs."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import holdout_cases as hc
import holdout_reference as href
import train_grad_reference as tref
from test_gpu_train_ensemble import DEV, _Data, _dataset, _ensemble, _grads_ensemble, _Member, _P

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _filled(shape, fill):
    """A float32 device tensor of NaNs (fill = "nan") or of 0xFF bytes."""
    t = torch.empty(shape, dtype=torch.float32, device=DEV)
    if fill == "nan":
        t.fill_(NAN)
    else:
        t.view(torch.uint8).fill_(0xFF)
    return t


def run_eval(mems, data, rows, with_loss=True, fill="nan"):
    """mbrl_eval_members on the members and device rows: dict(row_err [E][R][H], row_rew_err or None,
    loss [E][3] or None) as NumPy; the outputs hold `fill` before the call."""
    from mbrl_amd import _lib
    lib = _lib.load()
    E, R = len(mems), int(rows.numel())
    s, a, W, L, reward, H = mems[0].shape
    tms = (_lib.TrainModel * E)()
    for e, mem in enumerate(mems):
        mem.fill(tms[e])
    row_err = _filled((E, R, H), fill)
    rew = _filled((E, R, H), fill) if reward else None
    loss = _filled((E, 3), fill) if with_loss else None
    _lib.check(lib.mbrl_eval_members(tms, E, ctypes.byref(data.c), _P(rows), R, _P(row_err), None if rew is None else _P(rew),
                                     None if loss is None else _P(loss), _lib.stream_handle(DEV)), "mbrl_eval_members")
    torch.cuda.synchronize()
    return dict(row_err=row_err.cpu().numpy(), row_rew_err=None if rew is None else rew.cpu().numpy(),
                loss=None if loss is None else loss.cpu().numpy())


@functools.lru_cache(maxsize=None)
def device_data(name):
    c, p = hc.CASES[name], hc.problem(name)
    return _Data(c.s, c.a, c.H, p["T"], 0, arrays=p["data"])


def members(name, which=None):
    """The case's members (or those listed in `which`), each under the case's alignment policy."""
    c, p = hc.CASES[name], hc.problem(name)
    n = 2 * (c.L + 1 + c.reward)
    out = []
    for e in (range(c.E) if which is None else which):
        mem = _Member(c.s, c.a, c.W, c.L, c.reward, c.H, 0, values=p["params"][e],
                      offset_params=range(n) if e in c.offset else ())
        assert all((q.data_ptr() % 16 == 4) == (e in c.offset) for q in mem.params)
        out.append(mem)
    return out


def rows_of(name):
    return torch.from_numpy(np.array(hc.problem(name)["rows"])).to(DEV)


@functools.lru_cache(maxsize=None)
def default_run(name):
    return run_eval(members(name), device_data(name), rows_of(name))


def _same(x, y):
    return all((x[k] is None and y[k] is None) or x[k].tobytes() == y[k].tobytes() for k in x)


@pytest.mark.parametrize("name", hc.NAMES)
def test_eval_members_matches_float64(name):
    c = hc.CASES[name]
    got = default_run(name)
    failures = []
    for e in range(c.E):
        mine = {k: (None if v is None else v[e]) for k, v in got.items()}
        assert all(np.all(np.isfinite(v)) for v in mine.values() if v is not None), (name, e)
        err, own, bar = hc.errors(name, e, mine), hc.e32(name, e), hc.bars(name, e)
        for k in hc.KINDS:
            if k in err:
                print(f"RATIO {name} member {e} {k}: e(gpu) {err[k]:.3e}, e32 {own[k]:.3e}, bar {bar[k]:.3e}")
                if not err[k] <= bar[k]:
                    failures.append(f"member {e} {k}: e(gpu) = {err[k]:.3e} > bar = {bar[k]:.3e}")
        for label, x, x0, b in zip(("total", "state", "reward"), err["loss"], own["loss"], bar["loss"]):
            print(f"RATIO {name} member {e} loss_{label}: e(gpu) {x:.3e}, e32 {x0:.3e}, bar {b:.3e}")
            if not x <= b:
                failures.append(f"member {e} loss {label}: e(gpu) = {x:.3e} > bar = {b:.3e}")
    assert not failures, f"{name}: " + "; ".join(failures)


@pytest.mark.parametrize("name", hc.NAMES)
def test_loss_agrees_with_train_grads_ensemble(name):
    """loss_out against mbrl_train_grads_ensemble's loss of a batch made of the same rows: their distance,
    relative to the float64 loss, within the bar (an exactly zero reward loss on both sides)."""
    c = hc.CASES[name]
    rows = rows_of(name)
    train = _grads_ensemble(members(name), device_data(name), rows.repeat(c.E, 1).contiguous(),
                            alloc=lambda *sh: torch.full(sh, NAN, device=DEV)).cpu().numpy()
    got = default_run(name)["loss"]
    for e in range(c.E):
        l64, bar = hc.ref(name, e)["loss"], hc.bars(name, e)["loss"]
        for k in range(3):
            if l64[k] == 0:
                assert got[e, k] == 0 and train[e, k] == 0, (name, e, k)
            else:
                d = abs(float(got[e, k]) - float(train[e, k])) / abs(l64[k])
                print(f"RATIO {name} member {e} loss[{k}] eval vs train: {d:.3e}, bar {bar[k]:.3e}")
                assert d <= bar[k], (name, e, k, got[e], train[e])


E5 = "r257"          # five members, 257 repeated and unsorted rows


def test_a_member_alone_equals_the_member_among_five():
    full = default_run(E5)
    for e in range(hc.CASES[E5].E):
        one = run_eval(members(E5, [e]), device_data(E5), rows_of(E5))
        assert all(one[k] is None or one[k][0].tobytes() == full[k][e].tobytes() for k in one), e
    twice = run_eval(members(E5, [3, 3]), device_data(E5), rows_of(E5))       # a member listed twice
    assert all(twice[k] is None or twice[k][0].tobytes() == twice[k][1].tobytes() == full[k][3].tobytes() for k in twice)


@pytest.mark.parametrize("name", [E5, "s17_h3_e5", "offset_mid"])
def test_permuted_rows_give_permuted_outputs(name):
    full, rows = default_run(name), hc.problem(name)["rows"]
    perm = np.random.default_rng(3).permutation(len(rows))
    got = run_eval(members(name), device_data(name), torch.from_numpy(rows[perm]).to(DEV))
    for k in hc.KINDS:
        if full[k] is not None:
            assert got[k].tobytes() == np.ascontiguousarray(full[k][:, perm]).tobytes(), k


@pytest.mark.parametrize("name", [E5, "s17_h3_e5"])
def test_a_row_alone_equals_the_row_among_many(name):
    full, rows = default_run(name), hc.problem(name)["rows"]
    for r in (0, 15, 16, len(rows) - 1):
        one = run_eval(members(name), device_data(name), torch.from_numpy(rows[r:r + 1].copy()).to(DEV))
        for k in hc.KINDS:
            if full[k] is not None:
                assert one[k].tobytes() == np.ascontiguousarray(full[k][:, r:r + 1]).tobytes(), (k, r)
    rep = [np.flatnonzero(rows == v) for v in np.unique(rows)]
    rep = [ix for ix in rep if len(ix) > 1]
    assert rep, "the case has no repeated row"
    for ix in rep:
        for k in hc.KINDS:
            if full[k] is not None:
                assert all(full[k][:, i].tobytes() == full[k][:, ix[0]].tobytes() for i in ix), (k, ix)


@pytest.mark.parametrize("name", [E5, "h3_r17", "w1024_l2"])
def test_prior_output_bytes_never_matter_and_runs_repeat(name):
    base = default_run(name)
    assert _same(base, run_eval(members(name), device_data(name), rows_of(name), fill="ff"))
    assert _same(base, run_eval(members(name), device_data(name), rows_of(name), fill="nan"))
    no_loss = run_eval(members(name), device_data(name), rows_of(name), with_loss=False)
    assert all(no_loss[k] is None or no_loss[k].tobytes() == base[k].tobytes() for k in hc.KINDS)


def test_eval_members_refuses_before_any_launch():
    """Each refusal with real device buffers: the code, and no output byte written."""
    from mbrl_amd import _lib
    lib = _lib.load()
    mems, data, rows = members("e8"), device_data("e8"), rows_of("e8")
    E, R, H = 8, int(rows.numel()), 2
    out = [torch.full((E + 1, R, H), 7.0, device=DEV) for _ in range(2)] + [torch.full((E + 1, 3), 7.0, device=DEV)]
    tms = (_lib.TrainModel * (E + 1))()
    for e in range(E + 1):
        mems[e % E].fill(tms[e])

    def call(tms_=tms, E_=E, data_=data.c, rows_=_P(rows), R_=R, err=_P(out[0]), rew=_P(out[1])):
        return lib.mbrl_eval_members(tms_, E_, ctypes.byref(data_) if data_ is not None else None, rows_, R_, err, rew,
                                     _P(out[2]), _lib.stream_handle(DEV))
    odd = (_lib.TrainModel * 2)()
    mems[0].fill(odd[0])
    mems[1].fill(odd[1])
    odd[1].hidden += 1
    nullw = (_lib.TrainModel * 1)()
    mems[0].fill(nullw[0])
    nullw[0].bias[1] = None
    assert call(E_=E + 1) == _lib.MBRL_EUNSUPPORTED
    assert call(R_=(1 << 31) // (E * H)) == _lib.MBRL_EUNSUPPORTED
    for kw in (dict(tms_=None), dict(data_=None), dict(rows_=None), dict(err=None), dict(rew=None), dict(E_=0), dict(R_=0),
               dict(tms_=odd, E_=2), dict(tms_=nullw, E_=1)):
        assert call(**kw) == _lib.MBRL_EINVAL, kw
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out)
    assert call() == _lib.MBRL_OK
    torch.cuda.synchronize()


# ---- mbrl_keep_best

def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().tobytes()


def _keep_best(loss, stride, epoch, state, table, E, count):
    from mbrl_amd import _lib
    _lib.check(_lib.load().mbrl_keep_best(_P(loss), stride, E, epoch, _P(state[0]), _P(state[1]), _P(state[2]), table,
                                          count, _lib.stream_handle(DEV)), "mbrl_keep_best")
    torch.cuda.synchronize()


@pytest.mark.parametrize("count,sizes", [(2, (5, 1030)), (30, tuple(range(0, 30)))])
def test_keep_best_two_epochs(count, sizes):
    """E = 3, two epochs: (better, NaN, better) against +inf, then (equal, better, worse). Snapshots are the
    sources' bits (NaN payloads and -0.0 among them) of the epoch that was better, destinations of members
    that were not better keep their sentinel, bytes around every destination stay, and 3 x 30 tensors take
    two launches' worth of table. Odd tensors lie 4 bytes off 16-byte alignment."""
    from mbrl_amd import _lib
    E, SENT, GUARD = 3, -12345.0, 8
    g = torch.Generator().manual_seed(count)
    sizes = (sizes * count)[:count]

    def source(n, odd):
        buf = torch.randn(n + 8, generator=g).to(DEV)
        v = buf[1:1 + n] if odd else buf[4:4 + n]
        if n >= 3:
            v[0], v[2] = -0.0, NAN
            v.view(torch.int32)[1] = 0x7FC12345          # a NaN with a payload
        return v
    src = [[source(n, i % 2) for i, n in enumerate(sizes)] for _ in range(E)]
    dst_buf = [[torch.full((n + 2 * GUARD + 1,), SENT, device=DEV) for n in sizes] for _ in range(E)]
    dst = [[b[GUARD + (i % 2):GUARD + (i % 2) + n] for i, (b, n) in enumerate(zip(row, sizes))] for row in dst_buf]
    table = (_lib.CopyTensor * (E * count))()
    for e in range(E):
        for i in range(count):
            t = table[e * count + i]
            t.src, t.dst, t.numel = src[e][i].data_ptr(), dst[e][i].data_ptr(), sizes[i]
    state = [torch.full((E,), float("inf"), device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV),
             torch.zeros(E, dtype=torch.int32, device=DEV)]
    stride = 3
    loss0 = torch.tensor([[0.5, 9, 9], [NAN, 9, 9], [0.75, 9, 9]], device=DEV)
    _keep_best(loss0, stride, 0, state, table, E, count)
    assert state[0].tolist()[0] == 0.5 and state[0].tolist()[1] == float("inf") and state[0].tolist()[2] == 0.75
    assert state[1].tolist() == [0, -1, 0] and state[2].tolist() == [0, 1, 0]
    first = [[s.clone() for s in row] for row in src]
    for e in range(E):
        for i in range(count):
            if e == 1:
                assert bool((dst_buf[e][i] == SENT).all()), (e, i)
            else:
                assert _bits(dst[e][i]) == _bits(src[e][i]), (e, i)
    for row in src:                                     # the parameters move on
        for s in row:
            s.add_(1.0)
    loss1 = torch.tensor([[0.5, 0, 0], [0.25, 0, 0], [1.0, 0, 0]], device=DEV)
    _keep_best(loss1, stride, 1, state, table, E, count)
    assert state[0].tolist() == [0.5, 0.25, 0.75]
    assert state[1].tolist() == [0, 1, 0] and state[2].tolist() == [1, 0, 1]
    for e in range(E):
        for i, n in enumerate(sizes):
            want = src[e][i] if e == 1 else first[e][i]
            assert _bits(dst[e][i]) == _bits(want), (e, i)
            lo = GUARD + (i % 2)
            assert bool((dst_buf[e][i][:lo] == SENT).all()) and bool((dst_buf[e][i][lo + n:] == SENT).all()), (e, i)


def test_keep_best_refusals():
    from mbrl_amd import _lib
    lib = _lib.load()
    E = 2
    loss = torch.zeros(E, device=DEV)
    state = [torch.full((E,), 1.0, device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV),
             torch.zeros(E, dtype=torch.int32, device=DEV)]
    a, b = torch.ones(4, device=DEV), torch.full((4,), 7.0, device=DEV)
    table = (_lib.CopyTensor * E)()
    for t in table:
        t.src, t.dst, t.numel = a.data_ptr(), b.data_ptr(), 4
    bad = (_lib.CopyTensor * E)()
    bad[0].src, bad[0].dst, bad[0].numel = a.data_ptr(), None, 4

    def call(loss_=_P(loss), stride=1, E_=E, epoch=0, bl=_P(state[0]), be=_P(state[1]), st=_P(state[2]), tab=table, n=1):
        return lib.mbrl_keep_best(loss_, stride, E_, epoch, bl, be, st, tab, n, _lib.stream_handle(DEV))
    for kw in (dict(loss_=None), dict(bl=None), dict(be=None), dict(st=None), dict(E_=0), dict(stride=0), dict(epoch=-1),
               dict(n=-1), dict(tab=None), dict(tab=bad)):
        assert call(**kw) == _lib.MBRL_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((b == 7.0).all()) and state[1].tolist() == [-1, -1] and state[2].tolist() == [0, 0]


# ---- Python: evaluate_members, fit_members, elite

S, A, W, E, TRAIN, HOLD, EPOCHS, BATCH, LR = 5, 2, 64, 3, 300, 80, 6, 64, 2e-2


def _adam(ens):
    return [torch.optim.Adam(m.parameters(), lr=LR) for m in ens.members]


def _params(ens):
    return [p.detach().clone() for p in ens.parameters()]


def _adam_state(opts):
    return [v.clone() for o in opts for p in o.param_groups[0]["params"] for k, v in sorted(o.state[p].items())]


def _holdout(T_, seed):
    """A TransitionsDataset of exactly T_ one-step transitions in two rollouts."""
    from mbrl_amd import data
    rng = np.random.Generator(np.random.PCG64(seed))
    rolls = []
    for _ in range(2):
        st = rng.standard_normal((T_ // 2 + 2, S)).astype(np.float32)
        rolls.append(data.Rollout(states=list(torch.from_numpy(st)), observations=list(torch.from_numpy(st)),
                                  actions=list(torch.from_numpy(rng.uniform(-1, 1, (T_ // 2 + 1, A)).astype(np.float32))),
                                  rewards=list(torch.from_numpy(rng.standard_normal(T_ // 2 + 1).astype(np.float32)))))
    ds = data.TransitionsDataset(rollouts=rolls, horizon=1)
    ds.set_data_mode("state_only")
    assert ds.num_transitions() == T_
    return ds


@functools.lru_cache(maxsize=None)
def _sets():
    train = _dataset(S, A, 1, TRAIN, seed=21)
    assert train.num_transitions() == TRAIN
    return train, _holdout(HOLD, seed=22)


@functools.lru_cache(maxsize=None)
def _trained(epochs):
    """(parameters, Adam state, held-out losses [E]) after train_members of `epochs` epochs from seed 0."""
    train, hold = _sets()
    ens = _ensemble(E, S, A, W, seed=0)
    opts = _adam(ens)
    assert ens.train_members(train, opts, batch_size=BATCH, num_epochs=epochs, seed=4) == epochs
    return _params(ens), _adam_state(opts), ens.evaluate_members(hold)["loss"].clone()


@functools.lru_cache(maxsize=None)
def _fit(restore_best, patience=None, check_every=1):
    train, hold = _sets()
    ens = _ensemble(E, S, A, W, seed=0)
    opts = _adam(ens)
    report = ens.fit_members(train, hold, opts, batch_size=BATCH, max_epochs=EPOCHS, seed=4, restore_best=restore_best,
                             patience=patience, check_every=check_every)
    torch.cuda.synchronize()
    return ens, opts, report


def test_evaluate_members_is_the_native_call_and_matches_torch(monkeypatch):
    from mbrl_amd import models
    train, hold = _sets()
    ens = _ensemble(E, S, A, W, seed=0)
    rows = torch.tensor([5, 3, 3, 79, 0], device=DEV)
    calls = []
    real = models._NativeEval.run
    monkeypatch.setattr(models._NativeEval, "run", lambda self, *a: calls.append(1) or real(self, *a))
    got = ens.evaluate_members(hold, rows)
    assert calls == [1]
    assert got["row_err"].shape == (E, 5, 1) and got["per_step"].shape == (E, 1) and got["loss"].shape == (E,)
    assert all(v.is_cuda for v in got.values())
    assert torch.equal(got["row_err"][:, 1], got["row_err"][:, 2])
    monkeypatch.setattr(models, "NATIVE_TRAINING", False)
    want = ens.evaluate_members(hold, rows)
    assert calls == [1]                                                    # the torch restatement this time
    for k in got:
        assert torch.allclose(got[k], want[k], rtol=1e-4, atol=1e-6), k
    every = ens.evaluate_members(hold)
    assert every["row_err"].shape == (E, hold.num_transitions(), 1)


def test_fit_members_without_restore_is_train_members():
    ens, opts, report = _fit(False)
    params, state, _ = _trained(EPOCHS)
    assert report["epochs_run"] == EPOCHS and report["native_epochs"] == EPOCHS
    assert all(torch.equal(x, y) for x, y in zip(_params(ens), params))
    assert all(torch.equal(x, y) for x, y in zip(_adam_state(opts), state))
    assert ens.train_iterations == 1 and all(m.train_iterations == 1 for m in ens.members)


def test_fit_members_val_loss_and_restored_weights():
    """val_loss row k is evaluate_members after k + 1 epochs of train_members; the report is the NumPy rule on
    that table; member e's restored parameters are train_members' after best_epoch[e] + 1 epochs; the Adam
    state is the last epoch's."""
    ens, opts, report = _fit(True)
    val = torch.stack([_trained(k + 1)[2] for k in range(EPOCHS)]).cpu()
    assert torch.equal(report["val_loss"], val)
    want = href.rule(val.numpy())
    assert report["epochs_run"] == EPOCHS == want["epochs_run"]
    assert report["best_epoch"].tolist() == want["best_epoch"].tolist()
    assert report["best_loss"].numpy().tobytes() == want["best_loss"].tobytes()
    assert ens.holdout_report is report
    n = len(list(ens.members[0].parameters()))
    for e, m in enumerate(ens.members):
        at = _trained(int(report["best_epoch"][e]) + 1)[0][e * n:(e + 1) * n]
        assert all(torch.equal(p, q) for p, q in zip(m.parameters(), at)), e
    assert all(torch.equal(x, y) for x, y in zip(_adam_state(opts), _trained(EPOCHS)[1]))


@pytest.mark.parametrize("patience,check_every", [(1, 1), (1, 2), (2, 1)])
def test_fit_members_stops_where_the_rule_says(patience, check_every):
    full = _fit(True)[2]
    want = href.rule(full["val_loss"].numpy(), patience, check_every)
    ens, opts, report = _fit(True, patience, check_every)
    assert report["epochs_run"] == want["epochs_run"]
    assert torch.equal(report["val_loss"], full["val_loss"][:want["epochs_run"]])
    assert report["best_epoch"].tolist() == want["best_epoch"].tolist()
    assert report["best_loss"].numpy().tobytes() == want["best_loss"].tobytes()
    if (patience, check_every) == (1, 1):
        assert want["epochs_run"] < EPOCHS, "the case never stops early: it shows nothing"


def _plan(module):
    from mbrl_amd import CEMPlanner, env, models
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(S), torch.zeros(S), 0.4), models.CoshLoss(0.25))
    sample = env.sample_action_fn(env.BoundedActionSpec(A, -1.0, 1.0))
    res = CEMPlanner.plan_detailed(torch.linspace(-1, 1, S), module, cost, sample, 5, num_candidates=256,
                                   num_iterations=2, seed=3, device="cuda:0")
    return [res[k].detach().cpu().clone() for k in ("actions", "mu", "sigma")]


def test_plans_after_fit_members_and_on_the_elite():
    from mbrl_amd import models
    train, hold = _sets()
    ens = _ensemble(E, S, A, W, seed=0)
    before = _plan(ens)                                  # (the planner's weight pack is cached from here on)
    report = ens.fit_members(train, hold, _adam(ens), batch_size=BATCH, max_epochs=EPOCHS, seed=4)
    after = _plan(ens)
    fresh = _ensemble(E, S, A, W, seed=9)
    fresh.load_state_dict(copy.deepcopy(ens.state_dict()))
    assert all(torch.equal(x, y) for x, y in zip(after, _plan(fresh)))
    assert not all(torch.equal(x, y) for x, y in zip(after, before))
    elite = ens.elite(2)
    keep = sorted(np.argsort(report["best_loss"].numpy(), kind="stable")[:2].tolist())
    assert elite.elite_indices == keep and all(elite.members[i] is ens.members[j] for i, j in enumerate(keep))
    by_hand = models.EnsembleModel([copy.deepcopy(ens.members[j]) for j in keep]).to(DEV)
    assert all(torch.equal(x, y) for x, y in zip(_plan(elite), _plan(by_hand)))
    assert not all(torch.equal(x, y) for x, y in zip(_plan(elite), after))
