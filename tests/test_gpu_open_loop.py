"""GPU: open-loop evaluation of ensemble members (csrc/eval.hip: mbrl_eval_members_open_loop) and
EnsembleModel.evaluate_members(open_loop=True) / fit_members(holdout_loss="open_loop") on top of it.

Accuracy: over tests/open_loop_cases.py, row_err, row_rew_err, pred_out and loss_out against the float64
restatement of tests/open_loop_reference.py at the project's bar -- the tensor-relative error
(train_grad_reference.err) within 8 x max(the float32 CPU chain's error on that tensor, the table's median of
it). Everything else is equality byte for byte: against mbrl_eval_members at horizon 1 and step by step along
the chain, against shorter horizons, other E, R and row orders, poisoned outputs and NULL outputs."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import open_loop_cases as oc
from test_gpu_holdout import _filled, run_eval
from test_gpu_train_ensemble import DEV, _Data, _dataset, _ensemble, _Member, _P

pytestmark = pytest.mark.gpu
NAN = float("nan")
OUTS = ("row_err", "row_rew_err", "pred", "loss")


def run_open(mems, data, rows, with_loss=True, with_pred=True, fill="nan"):
    """mbrl_eval_members_open_loop on the members and device rows: dict(row_err [E][R][H], row_rew_err or None,
    pred [E][R][H][s] or None, loss [E][3] or None) as NumPy; the outputs hold `fill` before the call."""
    from mbrl_amd import _lib
    lib = _lib.load()
    E, R = len(mems), int(rows.numel())
    s, a, W, L, reward, H = mems[0].shape
    tms = (_lib.TrainModel * E)()
    for e, mem in enumerate(mems):
        mem.fill(tms[e])
    row_err = _filled((E, R, H), fill)
    rew = _filled((E, R, H), fill) if reward else None
    pred = _filled((E, R, H, s), fill) if with_pred else None
    loss = _filled((E, 3), fill) if with_loss else None
    opt = lambda t: None if t is None else _P(t)   # noqa: E731
    _lib.check(lib.mbrl_eval_members_open_loop(tms, E, ctypes.byref(data.c), _P(rows), R, _P(row_err), opt(rew), opt(pred),
                                               opt(loss), _lib.stream_handle(DEV)), "mbrl_eval_members_open_loop")
    torch.cuda.synchronize()
    return {k: None if t is None else t.cpu().numpy() for k, t in zip(OUTS, (row_err, rew, pred, loss))}


@functools.lru_cache(maxsize=None)
def device_data(name):
    c, p = oc.CASES[name], oc.problem(name)
    return _Data(c.s, c.a, c.H, p["T"], 0, arrays=p["data"])


def members(name, which=None, horizon=None):
    """The case's members (or those listed in `which`), each under the case's alignment policy."""
    c, p = oc.CASES[name], oc.problem(name)
    n = 2 * (c.L + 1 + c.reward)
    out = []
    for e in (range(c.E) if which is None else which):
        mem = _Member(c.s, c.a, c.W, c.L, c.reward, horizon or c.H, 0, values=p["params"][e],
                      offset_params=range(n) if e in c.offset else ())
        assert all((q.data_ptr() % 16 == 4) == (e in c.offset) for q in mem.params)
        out.append(mem)
    return out


def rows_of(name):
    return torch.from_numpy(np.array(oc.problem(name)["rows"])).to(DEV)


@functools.lru_cache(maxsize=None)
def default_run(name):
    return run_open(members(name), device_data(name), rows_of(name))


def _same(x, y, keys=OUTS):
    return all((x[k] is None and y[k] is None) or x[k].tobytes() == y[k].tobytes() for k in keys)


def _sliced(name, h0, h1, states=None):
    """The case's transitions restricted to the steps h0 .. h1 - 1 as contiguous device copies (states: the
    [T][h1 - h0][s] array to use instead of the dataset's)."""
    c, p = oc.CASES[name], oc.problem(name)
    arrays = {k: np.ascontiguousarray(v[:, h0:h1]) for k, v in p["data"].items()}
    if states is not None:
        arrays["states"] = states
    return _Data(c.s, c.a, h1 - h0, p["T"], 0, arrays=arrays)


@pytest.mark.parametrize("name", oc.NAMES)
def test_open_loop_matches_float64(name):
    c = oc.CASES[name]
    got = default_run(name)
    failures = []
    for e in range(c.E):
        mine = {k: (None if v is None else v[e]) for k, v in got.items()}
        assert all(np.all(np.isfinite(v)) for v in mine.values() if v is not None), (name, e)
        err, own, bar = oc.errors(name, e, mine), oc.e32(name, e), oc.bars(name, e)
        for k in oc.KINDS:
            if k in err:
                print(f"RATIO {name} member {e} {k}: e(gpu) {err[k]:.3e}, e32 {own[k]:.3e}, bar {bar[k]:.3e}")
                if not err[k] <= bar[k]:
                    failures.append(f"member {e} {k}: e(gpu) = {err[k]:.3e} > bar = {bar[k]:.3e}")
        for label, x, x0, b in zip(("total", "state", "reward"), err["loss"], own["loss"], bar["loss"]):
            print(f"RATIO {name} member {e} loss_{label}: e(gpu) {x:.3e}, e32 {x0:.3e}, bar {b:.3e}")
            if not x <= b:
                failures.append(f"member {e} loss {label}: e(gpu) = {x:.3e} > bar = {b:.3e}")
    assert not failures, f"{name}: " + "; ".join(failures)


@pytest.mark.parametrize("name", ["h1_r1", "h1_r33"])
def test_horizon_one_is_eval_members(name):
    want = run_eval(members(name), device_data(name), rows_of(name))
    assert _same(default_run(name), want, ("row_err", "row_rew_err", "loss"))


SEAM = ["h7_r17_s17_a0", "h3_r257_s5_a12", "h3_r16_s16_a1"]      # L = 2, 3 and 1; a = 0 with a reward head; E = 5


@pytest.mark.parametrize("name", SEAM)
def test_every_step_of_the_chain_is_eval_members_on_the_previous_prediction(name):
    """Step h of the horizon-H call against mbrl_eval_members on a horizon-1 dataset whose states are
    pred_out[:, :, h - 1] (row r of member e at dataset row r) and whose actions and targets are step h's."""
    c, p = oc.CASES[name], oc.problem(name)
    full, rows = default_run(name), p["rows"]
    seq = torch.arange(c.R, device=DEV)
    for h in range(c.H):
        for e in range(c.E):
            arrays = {k: np.ascontiguousarray(v[rows][:, h:h + 1]) for k, v in p["data"].items()}
            if h >= 1:
                arrays["states"] = np.ascontiguousarray(full["pred"][e][:, h - 1:h])
            step = run_eval(members(name, [e], horizon=1), _Data(c.s, c.a, 1, c.R, 0, arrays=arrays), seq, with_loss=False)
            assert step["row_err"][0, :, 0].tobytes() == np.ascontiguousarray(full["row_err"][e, :, h]).tobytes(), (h, e)
            if c.reward:
                assert step["row_rew_err"][0, :, 0].tobytes() == \
                    np.ascontiguousarray(full["row_rew_err"][e, :, h]).tobytes(), (h, e)


@pytest.mark.parametrize("name", ["h7_r17_s17_a0", "e5_h7"])
def test_the_first_steps_are_the_shorter_call(name):
    full = default_run(name)
    for h in (1, 2, 6):
        short = run_open(members(name, horizon=h), _sliced(name, 0, h), rows_of(name), with_loss=False)
        for k in ("row_err", "row_rew_err", "pred"):
            if full[k] is not None:
                assert short[k].tobytes() == np.ascontiguousarray(full[k][:, :, :h]).tobytes(), (k, h)


@pytest.mark.parametrize("name", ["a6_rew", "h30_w64", "s33_a0_w1"])
def test_later_true_states_are_never_read(name):
    c, p = oc.CASES[name], oc.problem(name)
    states = np.array(p["data"]["states"])
    states[:, 1:] = NAN
    got = run_open(members(name), _sliced(name, 0, c.H, states=states), rows_of(name))
    assert _same(got, default_run(name))


E5 = "h3_r257_s5_a12"          # five members, 257 repeated and unsorted rows, three steps


def test_a_member_alone_equals_the_member_among_five():
    full = default_run(E5)
    for e in range(oc.CASES[E5].E):
        one = run_open(members(E5, [e]), device_data(E5), rows_of(E5))
        assert all(one[k] is None or one[k][0].tobytes() == full[k][e].tobytes() for k in one), e
    twice = run_open(members(E5, [3, 3]), device_data(E5), rows_of(E5))
    assert all(twice[k] is None or twice[k][0].tobytes() == twice[k][1].tobytes() == full[k][3].tobytes() for k in twice)


@pytest.mark.parametrize("name", [E5, "e5_h7", "offset_mid"])
def test_permuted_rows_give_permuted_outputs(name):
    full, rows = default_run(name), oc.problem(name)["rows"]
    perm = np.random.default_rng(3).permutation(len(rows))
    got = run_open(members(name), device_data(name), torch.from_numpy(rows[perm]).to(DEV))
    for k in oc.KINDS:
        if full[k] is not None:
            assert got[k].tobytes() == np.ascontiguousarray(full[k][:, perm]).tobytes(), k


@pytest.mark.parametrize("name", [E5, "e5_h7"])
def test_a_row_alone_equals_the_row_among_many(name):
    full, rows = default_run(name), oc.problem(name)["rows"]
    for r in (0, 7, 8, 15, 16, len(rows) - 1):
        one = run_open(members(name), device_data(name), torch.from_numpy(rows[r:r + 1].copy()).to(DEV))
        for k in oc.KINDS:
            if full[k] is not None:
                assert one[k].tobytes() == np.ascontiguousarray(full[k][:, r:r + 1]).tobytes(), (k, r)
    rep = [np.flatnonzero(rows == v) for v in np.unique(rows)]
    rep = [ix for ix in rep if len(ix) > 1]
    assert rep, "the case has no repeated row"
    for ix in rep:
        for k in oc.KINDS:
            if full[k] is not None:
                assert all(full[k][:, i].tobytes() == full[k][:, ix[0]].tobytes() for i in ix), (k, ix)


@pytest.mark.parametrize("name", [E5, "h3_r16_s16_a1", "w1024_h2", "l8_w33"])
def test_prior_output_bytes_and_null_outputs_never_matter(name):
    base = default_run(name)
    assert _same(base, run_open(members(name), device_data(name), rows_of(name), fill="ff"))
    assert _same(base, run_open(members(name), device_data(name), rows_of(name), fill="nan"))
    for with_loss, with_pred in ((False, True), (True, False), (False, False)):
        got = run_open(members(name), device_data(name), rows_of(name), with_loss=with_loss, with_pred=with_pred)
        assert (got["loss"] is None) == (not with_loss) and (got["pred"] is None) == (not with_pred)
        assert all(got[k] is None or got[k].tobytes() == base[k].tobytes() for k in OUTS), (with_loss, with_pred)


@pytest.mark.parametrize("name,value", [("a6_rew", float("inf")), ("h7_r17_s17_a0", NAN), ("e5_h7", float("-inf"))])
def test_a_non_finite_row_stays_non_finite_and_leaves_its_neighbours_alone(name, value):
    """Dataset rows whose first state holds inf or NaN: their chains are non-finite at every step from the first,
    and every other row of their tiles keeps its bytes."""
    c, p = oc.CASES[name], oc.problem(name)
    rows = p["rows"]
    bad_rows = {int(rows[2]), int(rows[9]), int(rows[min(20, c.R - 1)])}   # (both halves of a tile, and the next tile)
    states = np.array(p["data"]["states"])
    for i in bad_rows:
        states[i, 0, c.s // 2] = value
    got = run_open(members(name), _sliced(name, 0, c.H, states=states), rows_of(name))
    base = default_run(name)
    bad = np.isin(rows, list(bad_rows))
    assert bad.sum() >= 3 and (~bad).sum() >= 8
    assert not np.isfinite(got["row_err"][:, bad]).any()
    assert not np.isfinite(got["pred"][:, bad]).all(axis=-1).any()
    for k in oc.KINDS:
        if base[k] is not None:
            assert np.ascontiguousarray(got[k][:, ~bad]).tobytes() == np.ascontiguousarray(base[k][:, ~bad]).tobytes(), k
    assert not np.isfinite(got["loss"][:, :2]).any()


def test_a_non_finite_reward_does_not_reach_the_next_state_without_actions():
    """a = 0 with a reward head: the reward head's output lies in the column right of the predicted state, which
    layer 0 of the next step reads as padding. A reward head whose bias is inf (and NaN) must change neither the
    predictions nor the state errors."""
    name = "h7_r17_s17_a0"
    base = default_run(name)
    for value in (float("inf"), NAN):
        mems = members(name)
        mems[0].params[-1].fill_(value)
        got = run_open(mems, device_data(name), rows_of(name))
        assert got["row_err"].tobytes() == base["row_err"].tobytes() and got["pred"].tobytes() == base["pred"].tobytes()
        assert not np.isfinite(got["row_rew_err"]).any()
        assert got["loss"][0, 1].tobytes() == base["loss"][0, 1].tobytes() and not np.isfinite(got["loss"][0, 0])


def test_open_loop_refuses_before_any_launch():
    """Each refusal with real device buffers: the code, and no output byte written."""
    from mbrl_amd import _lib
    lib = _lib.load()
    name = "e8"
    mems, data, rows = members(name), device_data(name), rows_of(name)
    c = oc.CASES[name]
    E, R, H = c.E, c.R, c.H
    out = [torch.full((E + 1, R, H), 7.0, device=DEV) for _ in range(2)] + \
        [torch.full((E + 1, R, H, c.s), 7.0, device=DEV), torch.full((E + 1, 3), 7.0, device=DEV)]
    tms = (_lib.TrainModel * (E + 1))()
    for e in range(E + 1):
        mems[e % E].fill(tms[e])

    def call(tms_=tms, E_=E, data_=data.c, rows_=_P(rows), R_=R, err=_P(out[0]), rew=_P(out[1])):
        return lib.mbrl_eval_members_open_loop(tms_, E_, ctypes.byref(data_) if data_ is not None else None, rows_, R_, err,
                                               rew, _P(out[2]), _P(out[3]), _lib.stream_handle(DEV))
    odd = (_lib.TrainModel * 2)()
    mems[0].fill(odd[0])
    mems[1].fill(odd[1])
    odd[1].horizon += 1
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
    assert all(bool((t[:E] != 7.0).any()) and bool((t[E:] == 7.0).all()) for t in out)


# ---- Python: evaluate_members(open_loop=True), fit_members(holdout_loss="open_loop"), elite

S, A, W, E, TRAIN, HOLD, HOLD_H, EPOCHS, BATCH, LR = 5, 2, 64, 3, 300, 80, 5, 5, 64, 2e-2


def _adam(ens):
    return [torch.optim.Adam(m.parameters(), lr=LR) for m in ens.members]


def _params(ens):
    return [p.detach().clone() for p in ens.parameters()]


@functools.lru_cache(maxsize=None)
def _sets():
    return _dataset(S, A, 1, TRAIN, seed=21), _dataset(S, A, HOLD_H, HOLD, seed=22)


@functools.lru_cache(maxsize=None)
def _trained(epochs):
    """(parameters, open-loop held-out losses [E]) after train_members of `epochs` epochs from seed 0."""
    train, hold = _sets()
    ens = _ensemble(E, S, A, W, seed=0)
    assert ens.train_members(train, _adam(ens), batch_size=BATCH, num_epochs=epochs, seed=4) == epochs
    return _params(ens), ens.evaluate_members(hold, open_loop=True)["loss"].clone()


def test_evaluate_members_open_loop_is_the_c_call(monkeypatch):
    from mbrl_amd import models
    _, hold = _sets()
    ens = _ensemble(E, S, A, W, seed=0)
    rows = torch.tensor([5, 3, 3, hold.num_transitions() - 1, 0], device=DEV)
    calls = []
    real = models._NativeEval.run_open_loop
    monkeypatch.setattr(models._NativeEval, "run_open_loop", lambda self, *a: calls.append(1) or real(self, *a))
    got = ens.evaluate_members(hold, rows, open_loop=True, predictions=True)
    assert calls == [1] and all(v.is_cuda for v in got.values())
    assert got["row_err"].shape == (E, 5, HOLD_H) and got["pred"].shape == (E, 5, HOLD_H, S) and got["loss"].shape == (E,)
    _, (st, ac), (rw, ns) = hold.stacked(DEV)
    arrays = dict(states=st.cpu().numpy(), actions=ac.cpu().numpy(), next_states=ns.cpu().numpy(),
                  rewards=rw.reshape(st.shape[0], HOLD_H).cpu().numpy())
    mems = [_Member(S, A, W, 2, 0, HOLD_H, 0, values=[t.detach().cpu().numpy() for lin in m.linears()
                                                     for t in (lin.weight, lin.bias)]) for m in ens.members]
    want = run_open(mems, _Data(S, A, HOLD_H, st.shape[0], 0, arrays=arrays), rows)
    assert got["row_err"].cpu().numpy().tobytes() == want["row_err"].tobytes()
    assert got["pred"].cpu().numpy().tobytes() == want["pred"].tobytes()
    assert got["loss"].cpu().numpy().tobytes() == np.ascontiguousarray(want["loss"][:, 0]).tobytes()
    assert "pred" not in ens.evaluate_members(hold, rows, open_loop=True) and calls == [1, 1]
    monkeypatch.setattr(models, "NATIVE_TRAINING", False)
    torch_path = ens.evaluate_members(hold, rows, open_loop=True, predictions=True)
    assert calls == [1, 1]                                                 # the torch restatement this time
    for k in got:
        assert torch.allclose(got[k], torch_path[k], rtol=1e-4, atol=1e-6), k


@functools.lru_cache(maxsize=None)
def _fit(restore_best, holdout_loss):
    train, hold = _sets()
    ens = _ensemble(E, S, A, W, seed=0)
    kw = {} if holdout_loss is None else dict(holdout_loss=holdout_loss)
    report = ens.fit_members(train, hold, _adam(ens), batch_size=BATCH, max_epochs=EPOCHS, seed=4,
                             restore_best=restore_best, **kw)
    torch.cuda.synchronize()
    return ens, report


def test_fit_members_open_loop_val_loss_and_restored_weights():
    import holdout_reference as href
    ens, report = _fit(True, "open_loop")
    assert report["holdout_loss"] == "open_loop" and report["native_eval"] and report["native_epochs"] == EPOCHS
    val = torch.stack([_trained(k + 1)[1] for k in range(EPOCHS)]).cpu()
    assert torch.equal(report["val_loss"], val)
    want = href.rule(val.numpy())
    assert report["best_epoch"].tolist() == want["best_epoch"].tolist()
    assert report["best_loss"].numpy().tobytes() == want["best_loss"].tobytes()
    n = len(list(ens.members[0].parameters()))
    for e, m in enumerate(ens.members):
        at = _trained(int(report["best_epoch"][e]) + 1)[0][e * n:(e + 1) * n]
        assert all(torch.equal(p, q) for p, q in zip(m.parameters(), at)), e


def test_fit_members_default_is_the_one_step_loss_as_before():
    """No holdout_loss and "one_step" give one result, whose val_loss rows are evaluate_members' default loss (the
    parent's fit_members, which tests/test_gpu_holdout.py holds to train_members epoch by epoch)."""
    train, hold = _sets()
    (ens0, rep0), (ens1, rep1) = _fit(True, None), _fit(True, "one_step")
    assert rep0["holdout_loss"] == rep1["holdout_loss"] == "one_step"
    for k in ("val_loss", "best_loss", "best_epoch"):
        assert torch.equal(rep0[k], rep1[k]), k
    assert all(torch.equal(x, y) for x, y in zip(_params(ens0), _params(ens1)))
    last = _ensemble(E, S, A, W, seed=0)
    last.train_members(train, _adam(last), batch_size=BATCH, num_epochs=EPOCHS, seed=4)
    assert torch.equal(rep0["val_loss"][-1], last.evaluate_members(hold)["loss"].cpu())
    assert not torch.equal(rep0["val_loss"], _fit(True, "open_loop")[1]["val_loss"])


def test_plans_on_the_open_loop_elite_use_the_selected_members():
    from mbrl_amd import CEMPlanner, env, models
    ens, report = _fit(True, "open_loop")

    def plan(module):
        cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(S), torch.zeros(S), 0.4), models.CoshLoss(0.25))
        sample = env.sample_action_fn(env.BoundedActionSpec(A, -1.0, 1.0))
        res = CEMPlanner.plan_detailed(torch.linspace(-1, 1, S), module, cost, sample, 5, num_candidates=256,
                                       num_iterations=2, seed=3, device="cuda:0")
        return [res[k].detach().cpu().clone() for k in ("actions", "mu", "sigma")]
    elite = ens.elite(2)
    keep = sorted(np.argsort(report["best_loss"].numpy(), kind="stable")[:2].tolist())
    assert elite.elite_indices == keep and all(elite.members[i] is ens.members[j] for i, j in enumerate(keep))
    by_hand = models.EnsembleModel([copy.deepcopy(ens.members[j]) for j in keep]).to(DEV)
    assert all(torch.equal(x, y) for x, y in zip(plan(elite), plan(by_hand)))
    assert not all(torch.equal(x, y) for x, y in zip(plan(elite), plan(ens)))
