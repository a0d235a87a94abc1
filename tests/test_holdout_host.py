"""CPU: held-out evaluation of ensemble members -- the float64 restatement against the package's own modules,
the case table's reach, the refusals of mbrl_eval_members / mbrl_keep_best (all before any launch: no GPU
needed), and EnsembleModel.evaluate_members / fit_members / elite on the torch path."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import holdout_cases as hc
import holdout_reference as href
from conftest import REPO
from test_train_ensemble_host import A, S, T, W, _dataset, _members, _weights

BATCH, EPOCHS, LR = 32, 6, 2e-2


def _adam(m):
    return torch.optim.Adam(m.parameters(), lr=LR)


# ---- the restatement

@pytest.mark.parametrize("name", ["h3_r17", "e8", "r65_a0", "w33_l8", "r33"])
def test_reference_equals_the_package_modules_in_float64(name):
    """holdout_reference.evaluate against models.Model / ModelWithReward (their _forward, no autograd) in
    float64 on the same rows, and -- without a reward head -- EnsembleModel.evaluate_members' torch path."""
    from mbrl_amd import models
    c, p = hc.CASES[name], hc.problem(name)
    D = {k: torch.from_numpy(np.array(v, np.float64)) for k, v in p["data"].items()}
    rows = torch.from_numpy(np.array(p["rows"]))
    mods = []
    for e in range(c.E):
        m = (models.ModelWithReward if c.reward else models.Model)(c.s, c.a, hidden_units=c.W, n_hidden=c.L).double()
        with torch.no_grad():
            for q, v in zip([t for lin in m.linears() for t in (lin.weight, lin.bias)], p["params"][e]):
                q.copy_(torch.from_numpy(np.array(v, np.float64)))
        mods.append(m)
        want = hc.ref(name, e)
        with torch.no_grad():
            for h in range(c.H):
                out = m._forward(torch.cat([D["states"][rows, h], D["actions"][rows, h]], dim=1))
                ns, rew = (out if c.reward else (out, None))
                err = ((ns - D["next_states"][rows, h]) ** 2).sum(1).numpy()
                assert np.allclose(err, want["row_err"][:, h], rtol=1e-12, atol=0)
                if c.reward:
                    rerr = ((rew.reshape(-1) - D["rewards"][rows, h]) ** 2).numpy()
                    assert np.allclose(rerr, want["row_rew_err"][:, h], rtol=1e-12, atol=0)
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
        got = models.EnsembleModel(mods).evaluate_members(Stacked(), np.array(p["rows"]))
        for e in range(c.E):
            want = hc.ref(name, e)
            assert np.allclose(got["row_err"][e].numpy(), want["row_err"], rtol=1e-12, atol=0)
            assert np.allclose(float(got["loss"][e]), want["loss"][0], rtol=1e-12, atol=0)
            assert np.allclose(got["per_step"][e].numpy(), want["row_err"].sum(0) / (c.R * c.s), rtol=1e-12, atol=0)


def test_rule_by_hand():
    nan = float("nan")
    val = np.array([[0.5, nan, 0.7], [0.5, 0.3, 0.9], [0.4, 0.3, 0.8], [0.6, nan, 0.95], [0.1, 0.1, 0.1]], np.float32)
    r = href.rule(val)
    assert r["best_epoch"].tolist() == [4, 4, 4] and r["epochs_run"] == 5
    r = href.rule(val[:4])
    assert r["best_epoch"].tolist() == [2, 1, 0] and r["stale"].tolist() == [1, 2, 3]
    assert r["best_loss"].tolist() == [np.float32(0.4), np.float32(0.3), np.float32(0.7)]
    assert href.rule(val, patience=1)["epochs_run"] == 4             # epoch 3: stale = (1, 2, 3)
    assert href.rule(val, patience=2)["epochs_run"] == 5
    assert href.rule(val, patience=1, check_every=3)["epochs_run"] == 5   # checked after epoch 2 only: stale 0 there
    assert href.rule(np.full((3, 2), nan), patience=1)["best_epoch"].tolist() == [-1, -1]
    assert href.rule(np.full((3, 2), nan), patience=2, check_every=1)["epochs_run"] == 2


def test_the_table_reaches_every_value():
    cs = list(hc.CASES.values())
    assert 30 <= len(cs) <= 40
    reached = dict(W={c.W for c in cs}, L={c.L for c in cs}, s={c.s for c in cs}, a={c.a for c in cs},
                   K0={c.s + c.a for c in cs}, H={c.H for c in cs}, reward={c.reward for c in cs}, E={c.E for c in cs},
                   R={c.R for c in cs}, rows={c.rows for c in cs})
    for k, want in hc.REACH.items():
        assert want <= reached[k], (k, want - reached[k])
    for name, c in hc.CASES.items():
        rows = hc.problem(name)["rows"]
        if c.rows == "perm":
            assert len(np.unique(rows)) == c.R
        if c.rows == "repeat":
            assert len(np.unique(rows)) < c.R
        if c.rows != "seq" and c.R > 3:
            assert np.any(np.diff(rows) < 0), name                       # unsorted
    # a member at offset parameters beside an aligned one, first, in the middle and last
    off = [c for c in cs if c.offset]
    assert {c.offset[0] == 0 for c in off} == {True, False} and all(len(c.offset) < c.E for c in off)
    assert all(c.W % 4 == 0 for c in off)                                # the pointer alone decides the load path
    # the kernel's one tile height (16 positions) has a case on each side at horizon 1, and inside a transition
    src = open(os.path.join(REPO, "mujoco-mbrl_amd", "csrc", "eval.hip")).read()
    assert int(re.search(r"constexpr int EVAL_TM = (\d+);", src).group(1)) == 16
    assert {15, 16, 17, 31, 32, 33} <= {c.R for c in cs if c.H == 1}
    assert any(c.H > 1 and (c.R * c.H) % 16 and c.R * c.H > 16 for c in cs)
    # the bars come from the float32 restatement alone, and are a few float32 ulps
    m = hc.medians()
    assert all(1e-8 < v < 5e-7 for v in m.values()), m


# ---- the C entries: symbols, struct layout, refusals (no launch, so no GPU)

def _shape(tm, s=17, a=6, W=512, L=2, reward=0, H=1, ptr=0x1000):
    tm.state_dim, tm.action_dim, tm.hidden, tm.n_hidden, tm.reward_head, tm.horizon = s, a, W, L, reward, H
    for i in range(L + 1 + reward):
        tm.weight[i], tm.bias[i] = ptr, ptr


def test_eval_members_signature_and_refusals():
    from mbrl_amd import _lib
    lib = _lib.load()
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert lib.mbrl_eval_members.argtypes == [ctypes.POINTER(_lib.TrainModel), i32, ctypes.POINTER(_lib.TrainData), P, i64,
                                              P, P, P, P]
    hdr = open(os.path.join(REPO, "include", "mbrl_cem.h")).read()
    assert "#define MBRL_ABI_VERSION 13" in hdr and lib.mbrl_abi_version() == 13
    FAKE = P(0x1000)                     # never dereferenced: every call below returns before a launch
    MAX = _lib.TRAIN_MAX_MEMBERS

    def call(E=2, R=100, reward=0, rows=FAKE, err=FAKE, rew=None, data="ok", members="ok", edit=None, **shape):
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
        return lib.mbrl_eval_members(tms if members == "ok" else None, E, ctypes.byref(d) if data is not None else None,
                                     rows, R, err, rew, None, None)
    INV, UNS = _lib.MBRL_EINVAL, _lib.MBRL_EUNSUPPORTED
    assert call(members=None) == INV and call(data=None) == INV and call(rows=None) == INV and call(err=None) == INV
    assert call(reward=1) == INV                                   # row_rew_err missing
    assert call(rew=FAKE) == INV                                   # row_rew_err superfluous
    assert call(edit=lambda t: t[1].weight.__setitem__(2, None)) == INV
    assert call(edit=lambda t: t[0].bias.__setitem__(0, None)) == INV
    assert call(E=0) == INV and call(R=0) == INV and call(E=-1) == INV
    assert call(edit=lambda t: setattr(t[1], "hidden", 256)) == INV
    assert call(edit=lambda t: setattr(t[1], "horizon", 2)) == INV
    assert call(data=lambda d: setattr(d, "next_states", None)) == INV
    assert call(data=lambda d: setattr(d, "actions", None)) == INV
    assert call(E=MAX + 1) == UNS
    assert call(E=2, R=1 << 30) == UNS and call(E=1, R=1 << 31) == UNS and call(E=2, R=1 << 29, H=2) == UNS
    assert b"2^31" in lib.mbrl_last_error()
    # beyond the envelope: MBRL_EUNSUPPORTED
    assert call(W=1025) == UNS and call(L=9) == UNS and call(s=1000, a=25) == UNS and call(s=1025, a=0) == UNS
    assert b"envelope" in lib.mbrl_last_error()


def test_keep_best_signature_layout_and_refusals():
    from mbrl_amd import _lib
    lib = _lib.load()
    P, i32 = ctypes.c_void_p, ctypes.c_int32
    assert lib.mbrl_keep_best.argtypes == [P, i32, i32, i32, P, P, P, ctypes.POINTER(_lib.CopyTensor), i32, P]
    assert ctypes.sizeof(_lib.CopyTensor) == 24
    assert [(_lib.CopyTensor.src.offset, _lib.CopyTensor.dst.offset, _lib.CopyTensor.numel.offset)] == [(0, 8, 16)]
    FAKE = P(0x1000)
    table = (_lib.CopyTensor * 4)()
    for t in table:
        t.src, t.dst, t.numel = 0x1000, 0x2000, 16

    def call(loss=FAKE, stride=3, E=2, epoch=0, best=FAKE, at=FAKE, stale=FAKE, tab=table, count=2):
        return lib.mbrl_keep_best(loss, stride, E, epoch, best, at, stale, tab, count, None)
    INV = _lib.MBRL_EINVAL
    assert call(loss=None) == INV and call(best=None) == INV and call(at=None) == INV and call(stale=None) == INV
    assert call(E=0) == INV and call(stride=0) == INV and call(epoch=-1) == INV and call(count=-1) == INV
    assert call(tab=None) == INV
    table[3].dst = None
    assert call() == INV
    table[3].dst, table[3].numel = 0x2000, -1
    assert call() == INV


# ---- Python on the torch path

def test_fit_members_cpu_follows_the_rule_on_its_own_val_loss():
    from mbrl_amd import models
    train, hold = _dataset(), _dataset(seed=5)
    full = models.EnsembleModel(_members(3)).fit_members(train, hold, _adam, batch_size=BATCH, max_epochs=EPOCHS, seed=7)
    assert full["native_epochs"] == 0 and full["epochs_run"] == EPOCHS and full["val_loss"].shape == (EPOCHS, 3)
    for patience, check_every in ((None, 1), (1, 1), (1, 2), (2, 1), (2, 3)):
        ens = models.EnsembleModel(_members(3))
        rep = ens.fit_members(train, hold, _adam, batch_size=BATCH, max_epochs=EPOCHS, seed=7, patience=patience,
                              check_every=check_every)
        want = href.rule(full["val_loss"].numpy(), patience, check_every)
        assert rep["epochs_run"] == want["epochs_run"], (patience, check_every)
        assert torch.equal(rep["val_loss"], full["val_loss"][:want["epochs_run"]])
        mine = href.rule(rep["val_loss"].numpy(), patience, check_every)
        assert rep["best_epoch"].tolist() == mine["best_epoch"].tolist() == want["best_epoch"].tolist()
        assert rep["best_loss"].numpy().tobytes() == mine["best_loss"].tobytes()
        assert ens.holdout_report is rep
        assert ens.train_iterations == 1 and [m.train_iterations for m in ens.members] == [1, 1, 1]
    assert href.rule(full["val_loss"].numpy(), 1, 1)["epochs_run"] < EPOCHS      # an early stop did fire


def test_restore_best_against_not_restoring_and_train_members():
    """restore_best=False ends where train_members ends; restore_best=True where train_members of
    best_epoch[e] + 1 epochs ends, member by member; val_loss row k is evaluate_members after k + 1 epochs."""
    from mbrl_amd import models
    train, hold = _dataset(), _dataset(seed=5)

    class Writer:
        rows = []

        def add_scalar(self, tag, value, step):
            self.rows.append((tag, float(torch.as_tensor(value).detach()), int(step)))
    runs = {}
    for restore in (False, True):
        ens = models.EnsembleModel(_members(3))
        rep = ens.fit_members(train, hold, _adam, batch_size=BATCH, max_epochs=EPOCHS, seed=7, restore_best=restore,
                              writer=Writer() if restore else None)
        runs[restore] = ([_weights(m) for m in ens.members], rep)
    assert torch.equal(runs[False][1]["val_loss"], runs[True][1]["val_loss"])
    rep = runs[True][1]
    after = {}
    for k in sorted(set(rep["best_epoch"].tolist()) | {EPOCHS - 1}):
        ens = models.EnsembleModel(_members(3))
        ens.train_members(train, _adam, batch_size=BATCH, num_epochs=k + 1, seed=7)
        after[k] = [_weights(m) for m in ens.members]
        assert torch.equal(ens.evaluate_members(hold)["loss"], rep["val_loss"][k])
    for e in range(3):
        assert all(torch.equal(x, y) for x, y in zip(runs[False][0][e], after[EPOCHS - 1][e]))
        assert all(torch.equal(x, y) for x, y in zip(runs[True][0][e], after[int(rep["best_epoch"][e])][e]))
    assert any(int(b) < EPOCHS - 1 for b in rep["best_epoch"])           # restoring changed something
    tags = {r[0] for r in Writer.rows}
    assert {f"loss/holdout/member{e}/0" for e in range(3)} <= tags
    hold_rows = [r for r in Writer.rows if r[0] == "loss/holdout/member1/0"]
    assert [r[2] for r in hold_rows] == list(range(1, EPOCHS + 1))
    assert np.array_equal(np.float32([r[1] for r in hold_rows]), rep["val_loss"][:, 1].numpy())


def test_elite_ordering_and_ties():
    from mbrl_amd import models
    ens = models.EnsembleModel(_members(5))
    with pytest.raises(ValueError):
        ens.elite(2)                                                   # no report yet
    report = dict(best_loss=torch.tensor([0.5, 0.2, 0.5, float("nan"), 0.2]))
    assert ens.elite(1, report).elite_indices == [1]                   # the tie goes to the lower index
    assert ens.elite(2, report).elite_indices == [1, 4]
    assert ens.elite(3, report).elite_indices == [0, 1, 4]
    assert ens.elite(4, report).elite_indices == [0, 1, 2, 4]          # the NaN last
    el = ens.elite(3, report)
    assert isinstance(el, models.EnsembleModel) and [m for m in el.members] == [ens.members[i] for i in (0, 1, 4)]
    assert all(a is b for a, b in zip(el.members[0].parameters(), ens.members[0].parameters()))   # shared
    for k in (0, 6):
        with pytest.raises(ValueError):
            ens.elite(k, report)
    ens.holdout_report = report
    assert ens.elite(2).elite_indices == [1, 4]
    x = torch.randn(7, S + A)
    assert torch.allclose(el._forward(x), torch.stack([ens.members[i]._forward(x) for i in (0, 1, 4)]).mean(0))
