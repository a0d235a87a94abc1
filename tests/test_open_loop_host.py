"""CPU: open-loop evaluation of ensemble members -- the restatement of tests/open_loop_reference.py against
tests/holdout_reference.py and the package's own modules, the case table's reach, its bars, the ReLU condition,
six single mistakes of the step seam against those bars, the refusals of mbrl_eval_members_open_loop (all
before any launch: no GPU needed), and EnsembleModel.evaluate_members / fit_members on the torch path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import holdout_reference as href
import open_loop_cases as oc
import open_loop_reference as oref
from conftest import REPO
from test_train_ensemble_host import A, S, W, _dataset, _members, _weights

BATCH, EPOCHS, LR = 32, 5, 2e-2


def _adam(m):
    return torch.optim.Adam(m.parameters(), lr=LR)


# ---- the restatement

@pytest.mark.parametrize("name", ["h1_r1", "h1_r33"])
def test_horizon_one_is_the_one_step_reference(name):
    c, p = oc.CASES[name], oc.problem(name)
    for e in range(c.E):
        for dtype in (torch.float64, torch.float32):
            mine = oc.ref(name, e, dtype)
            want = href.evaluate(p["params"][e], p["data"], p["rows"], oc.shape_of(name), dtype)
            for k in ("row_err", "row_rew_err", "loss"):
                assert (mine[k] is None and want[k] is None) or np.array_equal(mine[k], want[k]), (name, e, k)


@pytest.mark.parametrize("name", ["h7_r17_s17_a0", "a6_rew", "h3_r257_s5_a12", "l8_w33", "s33_a0_w1"])
def test_reference_equals_the_package_modules_in_float64(name):
    """open_loop_reference.evaluate against models.Model / ModelWithReward (their _forward, fed back by hand) in
    float64, and -- without a reward head -- EnsembleModel.evaluate_members(open_loop=True)'s torch path."""
    from mbrl_amd import models
    c, p = oc.CASES[name], oc.problem(name)
    D = {k: torch.from_numpy(np.array(v, np.float64)) for k, v in p["data"].items()}
    rows = torch.from_numpy(np.array(p["rows"]))
    mods = []
    for e in range(c.E):
        m = (models.ModelWithReward if c.reward else models.Model)(c.s, c.a, hidden_units=c.W, n_hidden=c.L).double()
        with torch.no_grad():
            for q, v in zip([t for lin in m.linears() for t in (lin.weight, lin.bias)], p["params"][e]):
                q.copy_(torch.from_numpy(np.array(v, np.float64)))
        mods.append(m)
        want = oc.ref(name, e)
        with torch.no_grad():
            x = D["states"][rows, 0]
            for h in range(c.H):
                out = m._forward(torch.cat([x, D["actions"][rows, h]], dim=1))
                x, rew = (out if c.reward else (out, None))
                assert np.allclose(x.numpy(), want["pred"][:, h], rtol=1e-12, atol=1e-14)
                err = ((x - D["next_states"][rows, h]) ** 2).sum(1).numpy()
                assert np.allclose(err, want["row_err"][:, h], rtol=1e-11, atol=0)
                if c.reward:
                    rerr = ((rew.reshape(-1) - D["rewards"][rows, h]) ** 2).numpy()
                    assert np.allclose(rerr, want["row_rew_err"][:, h], rtol=1e-10, atol=1e-24)
        state = sum(want["row_err"][:, h].sum() / (c.R * c.s) for h in range(c.H))
        rew = sum(want["row_rew_err"][:, h].sum() / c.R for h in range(c.H)) if c.reward else 0.0
        assert np.allclose(want["loss"], [state + rew, state, rew], rtol=1e-12, atol=0)
    if not c.reward:
        class Stacked:
            horizon = c.H

            def num_transitions(self):
                return p["T"]

            def stacked(self, dev):
                return None, (D["states"], D["actions"]), (D["rewards"], D["next_states"])
        got = models.EnsembleModel(mods).evaluate_members(Stacked(), np.array(p["rows"]), open_loop=True, predictions=True)
        assert got["pred"].shape == (c.E, c.R, c.H, c.s)
        for e in range(c.E):
            want = oc.ref(name, e)
            assert np.allclose(got["pred"][e].numpy(), want["pred"], rtol=1e-12, atol=1e-14)
            assert np.allclose(got["row_err"][e].numpy(), want["row_err"], rtol=1e-11, atol=0)
            assert np.allclose(float(got["loss"][e]), want["loss"][0], rtol=1e-11, atol=0)
            assert np.allclose(got["per_step"][e].numpy(), want["row_err"].sum(0) / (c.R * c.s), rtol=1e-11, atol=0)


def test_later_true_states_are_never_read():
    name = "a6_rew"
    p = oc.problem(name)
    data = dict(p["data"])
    data["states"] = data["states"].copy()
    data["states"][:, 1:] = np.nan
    got = oref.evaluate(p["params"][0], data, p["rows"], oc.shape_of(name), torch.float64)
    want = oc.ref(name, 0)
    assert all(np.array_equal(got[k], want[k]) for k in ("row_err", "row_rew_err", "pred", "loss"))


# ---- the table

def test_the_table_reaches_every_value():
    cs = list(oc.CASES.values())
    reached = dict(H={c.H for c in cs}, R={c.R for c in cs}, rows={c.rows for c in cs},
                   seam={(c.s, c.a) for c in cs if c.W >= 64 and c.H >= 2}, L={c.L for c in cs}, W={c.W for c in cs},
                   E={c.E for c in cs}, reward_at_a={(c.reward, c.a) for c in cs})
    for k, want in oc.REACH.items():
        assert want <= reached[k], (k, want - reached[k])
    assert all(c.W == 64 for c in cs if c.H == 30)                      # the long chain stays cheap
    assert all(c.H == 2 for c in cs if c.W == 1024)
    assert any(c.s == 33 and c.W == 1 and c.H >= 2 for c in cs)          # s > W
    assert any(c.s == 1 and c.H >= 2 for c in cs)
    # both parities of L (which buffer holds the outputs) feed a prediction back, with and without a reward head
    assert {(c.L % 2, c.reward) for c in cs if c.H >= 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for name, c in oc.CASES.items():
        rows = oc.problem(name)["rows"]
        if c.rows == "perm":
            assert len(np.unique(rows)) == c.R
        if c.rows == "repeat":
            assert len(np.unique(rows)) < c.R
        if c.rows != "seq" and c.R > 3:
            assert np.any(np.diff(rows) < 0), name                       # unsorted
    off = [c for c in cs if c.offset]
    assert {c.offset[0] == 0 for c in off} == {True, False} and all(len(c.offset) < c.E for c in off)
    assert all(c.W % 4 == 0 and c.H >= 2 for c in off)
    src = open(os.path.join(REPO, "mujoco-mbrl_amd", "csrc", "eval.hip")).read()
    assert int(re.search(r"constexpr int EVAL_TM = (\d+);", src).group(1)) == 16
    # the bars come from the float32 restatement alone, and are a few float32 ulps
    m = oc.medians()
    assert all(1e-8 < v < 1e-6 for v in m.values()), m


@pytest.mark.parametrize("name", oc.NAMES)
def test_float32_restatement_within_the_bars_and_no_relu_changes_side(name):
    c = oc.CASES[name]
    for e in range(c.E):
        own, bar = oc.e32(name, e), oc.bars(name, e)
        for k in oc.KINDS:
            if k in own:
                assert own[k] <= bar[k] and np.isfinite(bar[k]) and bar[k] < 1e-4, (name, e, k, own[k], bar[k])
        assert all(x <= b < 1e-4 for x, b in zip(own["loss"], bar["loss"])), (name, e)
        z64, z32 = oc.ref(name, e)["preacts"], oc.ref(name, e, torch.float32)["preacts"]
        assert z64.shape == (c.H, c.L, c.R, c.W)
        assert np.array_equal(z64 > 0, z32 > 0), (name, e, int(np.sum((z64 > 0) != (z32 > 0))))


@pytest.mark.parametrize("mutant", oref.MUTANTS)
def test_a_single_mistake_misses_the_bar_tenfold(mutant):
    """Each mistake in float64 against the float64 restatement: on every case it applies to, and every member,
    a tensor it touches is off by at least ten times its bar."""
    hit = 0
    for name, c in oc.CASES.items():
        if not oref.applies(mutant, oc.shape_of(name), c.R):
            continue
        hit += 1
        for e in range(c.E):
            err, bar = oc.errors(name, e, oc.ref(name, e, torch.float64, mutant)), oc.bars(name, e)
            worst = max(err[k] / bar[k] for k in ("row_err", "pred"))
            assert worst >= 10, (mutant, name, e, worst)
            if mutant != "prev_target":
                assert err["pred"] >= 10 * bar["pred"], (mutant, name, e)
            assert err["row_err"] >= 10 * bar["row_err"], (mutant, name, e)
    assert hit >= 5, (mutant, hit)


# ---- the C entry: signature and refusals (no launch, so no GPU)

def _shape(tm, s=17, a=6, W=512, L=2, reward=0, H=30, ptr=0x1000):
    tm.state_dim, tm.action_dim, tm.hidden, tm.n_hidden, tm.reward_head, tm.horizon = s, a, W, L, reward, H
    for i in range(L + 1 + reward):
        tm.weight[i], tm.bias[i] = ptr, ptr


def test_open_loop_signature_and_refusals():
    from mbrl_amd import _lib
    lib = _lib.load()
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert lib.mbrl_eval_members_open_loop.argtypes == [ctypes.POINTER(_lib.TrainModel), i32, ctypes.POINTER(_lib.TrainData),
                                                        P, i64, P, P, P, P, P]
    assert lib.mbrl_eval_members_open_loop.restype is i32
    hdr = open(os.path.join(REPO, "include", "mbrl_cem.h")).read()
    assert "#define MBRL_ABI_VERSION 13" in hdr and lib.mbrl_abi_version() == 13
    FAKE = P(0x1000)                     # never dereferenced: every call below returns before a launch
    MAX = _lib.TRAIN_MAX_MEMBERS

    def call(E=2, R=100, reward=0, rows=FAKE, err=FAKE, rew=None, pred=None, data="ok", members="ok", edit=None, **shape):
        tms = (_lib.TrainModel * (MAX + 1))()
        for tm in tms:
            _shape(tm, reward=reward, **shape)
        if edit:
            edit(tms)
        d = _lib.TrainData()
        d.states = d.actions = d.next_states = d.rewards = 0x1000
        d.transitions = 1000
        if callable(data):
            data(d)
        return lib.mbrl_eval_members_open_loop(tms if members == "ok" else None, E, ctypes.byref(d) if data is not None else None,
                                               rows, R, err, rew, pred, None, None)
    INV, UNS = _lib.MBRL_EINVAL, _lib.MBRL_EUNSUPPORTED
    assert call(members=None) == INV and call(data=None) == INV and call(rows=None) == INV and call(err=None) == INV
    assert b"eval_members_open_loop" in lib.mbrl_last_error()
    assert call(reward=1) == INV and call(reward=1, pred=FAKE) == INV    # row_rew_err missing
    assert call(rew=FAKE) == INV                                   # row_rew_err superfluous
    assert call(edit=lambda t: t[1].weight.__setitem__(2, None)) == INV
    assert call(edit=lambda t: t[0].bias.__setitem__(0, None)) == INV
    assert call(E=0) == INV and call(R=0) == INV and call(E=-1) == INV and call(H=0) == INV
    assert call(edit=lambda t: setattr(t[1], "hidden", 256)) == INV
    assert call(edit=lambda t: setattr(t[1], "horizon", 2)) == INV
    assert call(data=lambda d: setattr(d, "next_states", None)) == INV
    assert call(data=lambda d: setattr(d, "states", None)) == INV
    assert call(data=lambda d: setattr(d, "actions", None)) == INV
    assert call(E=MAX + 1) == UNS
    assert call(E=2, R=1 << 30, H=1) == UNS and call(E=1, R=1 << 31, H=1) == UNS and call(E=2, R=1 << 26, H=30) == UNS
    assert b"2^31" in lib.mbrl_last_error()
    assert call(W=1025) == UNS and call(L=9) == UNS and call(s=1000, a=25) == UNS and call(s=1025, a=0) == UNS
    assert b"envelope" in lib.mbrl_last_error()


# ---- Python on the torch path

def test_torch_fallback_equals_the_reference_and_defaults_are_unchanged():
    """evaluate_members(open_loop=True) on the CPU (float32 modules) against the float32 restatement: the same
    operations in the same order, so the same bits up to torch's choice of kernels -- held at 1e-6 of the largest
    value; the default call does not look at the new arguments."""
    from mbrl_amd import models
    hold = _dataset(horizon=3, seed=5)
    ens = models.EnsembleModel(_members(3))
    rows = np.array([5, 3, 3, 69, 0])
    got = ens.evaluate_members(hold, rows, open_loop=True, predictions=True)
    assert got["row_err"].shape == (3, 5, 3) and got["pred"].shape == (3, 5, 3, S) and got["loss"].shape == (3,)
    _, (st, ac), (rw, ns) = hold.stacked(torch.device("cpu"))
    data = dict(states=st.numpy(), actions=ac.numpy(), next_states=ns.numpy(), rewards=rw.reshape(st.shape[0], 3).numpy())
    for e, m in enumerate(ens.members):
        params = [t.detach().numpy() for lin in m.linears() for t in (lin.weight, lin.bias)]
        want = oref.evaluate(params, data, rows, (S, A, W, 2, 0, 3), torch.float32)
        for k in ("row_err", "pred"):
            assert np.allclose(got[k][e].numpy(), want[k], rtol=0, atol=1e-6 * np.abs(want[k]).max()), (e, k)
        assert np.allclose(float(got["loss"][e]), want["loss"][0], rtol=1e-5)
    assert torch.equal(got["row_err"][:, 1], got["row_err"][:, 2])
    # open loop and one step agree on step 0 and nowhere else
    one = ens.evaluate_members(hold, rows)
    assert set(one) == {"loss", "per_step", "row_err"}
    assert torch.equal(one["row_err"][:, :, 0], got["row_err"][:, :, 0])
    assert not torch.equal(one["row_err"][:, :, 1:], got["row_err"][:, :, 1:])
    same = ens.evaluate_members(hold, rows, open_loop=False, predictions=False)
    assert all(torch.equal(one[k], same[k]) for k in one)
    assert "pred" not in ens.evaluate_members(hold, rows, open_loop=True)


def test_value_errors_before_any_work():
    from mbrl_amd import models
    train, hold = _dataset(), _dataset(horizon=3, seed=5)
    ens = models.EnsembleModel(_members(2))
    before = [_weights(m) for m in ens.members]
    made = []

    def factory(m):
        made.append(m)
        return _adam(m)
    for bad in ("open-loop", "", "OPEN_LOOP", None, 1):
        with pytest.raises(ValueError, match="holdout_loss"):
            ens.fit_members(train, hold, factory, batch_size=BATCH, max_epochs=2, holdout_loss=bad)
    assert not made and ens.train_iterations == 0 and getattr(ens, "holdout_report", None) is None
    assert all(torch.equal(x, y) for b, m in zip(before, ens.members) for x, y in zip(b, _weights(m)))
    with pytest.raises(ValueError, match="open_loop"):
        ens.evaluate_members(hold, predictions=True)


def test_fit_members_open_loop_on_a_longer_holdout():
    """Training at horizon 1, holdout at horizon 3: val_loss row k is evaluate_members(open_loop=True) after k + 1
    epochs of train_members; restoring ends member e where train_members of best_epoch[e] + 1 epochs ends; the
    default is the one-step loss, as before."""
    from mbrl_amd import models
    train, hold = _dataset(), _dataset(horizon=3, seed=5)
    ens = models.EnsembleModel(_members(3))
    rep = ens.fit_members(train, hold, _adam, batch_size=BATCH, max_epochs=EPOCHS, seed=7, holdout_loss="open_loop")
    assert rep["holdout_loss"] == "open_loop" and rep["epochs_run"] == EPOCHS and rep["val_loss"].shape == (EPOCHS, 3)
    want = href.rule(rep["val_loss"].numpy())
    assert rep["best_epoch"].tolist() == want["best_epoch"].tolist()
    assert rep["best_loss"].numpy().tobytes() == want["best_loss"].tobytes()
    one_step_val = []
    for k in range(EPOCHS):
        other = models.EnsembleModel(_members(3))
        other.train_members(train, _adam, batch_size=BATCH, num_epochs=k + 1, seed=7)
        assert torch.equal(other.evaluate_members(hold, open_loop=True)["loss"], rep["val_loss"][k]), k
        one_step_val.append(other.evaluate_members(hold)["loss"])
        for e in range(3):
            if int(rep["best_epoch"][e]) == k:
                assert all(torch.equal(x, y) for x, y in zip(_weights(ens.members[e]), _weights(other.members[e]))), e
    assert ens.elite(2).elite_indices == sorted(np.argsort(rep["best_loss"].numpy(), kind="stable")[:2].tolist())
    default = models.EnsembleModel(_members(3)).fit_members(train, hold, _adam, batch_size=BATCH, max_epochs=EPOCHS, seed=7)
    assert default["holdout_loss"] == "one_step"
    assert torch.equal(default["val_loss"], torch.stack(one_step_val))
    assert not torch.equal(default["val_loss"], rep["val_loss"])
