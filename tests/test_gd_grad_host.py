"""CPU: the float64 reference of tests/test_gpu_gd_grad.py (gd_grad_reference) and its case table
(gd_grad_cases). The reference is the package's own classes' loss; its gradient is the finite-difference
slope of that loss; no ReLU of any case can change side between float32 and float64; and every case
tells every applicable single-factor mistake of a backward pass from a right one at the bar the GPU
test uses. These are conditions on the chosen seeds and shapes, asserted -- not measurements.

Which mutant is caught where (every case it applies to, by gd_grad_reference.applicable; asserted
below, with at least one case each):
  act_std dropped              every case with normalize_action whose loss depends on the states
  unnorm obs_std dropped       ... with unnormalize_state
  norm obs_std dropped         ... with normalize_state, H >= 2 or a reward head
  rew_std dropped              the reward-head cases with unnormalize_reward (all but rew:sn, rew:none)
  1/a dropped                  goal-state cases with the action cost and a >= 2
  one weight factor dropped    flags_*_weights_alphas
  relu mask of wrong layer     every L >= 2 case whose loss depends on the states
  relu mask >= 0               zero_unit_coop, zero_unit_single
  reward action share omitted  every reward-head case
  state gradient not carried   every H >= 2 case whose loss depends on the states"""
import numpy as np
import pytest

import gd_grad_cases as gc
import gd_grad_reference as ref


@pytest.mark.parametrize("name", gc.NAMES)
def test_reference_is_the_shipped_classes_loss_and_gradient(name):
    """Loss and gradient of the layer-by-layer restatement against Model / ModelWithReward.forward with
    the dataset's normalisers, SmoothAbsLoss, CoshLoss and the agents' closures, all float64: equal up
    to float64 rounding (the two sum in different orders)."""
    p = gc.problem(name)
    S0, A = gc.inputs(name)
    b = A.shape[0] - 1
    loss, g = ref.shipped_loss_and_grad(p, A[b], s0=S0[b])
    assert abs(ref.loss64(p, A[b], s0=S0[b]) - loss) <= 1e-12 * max(1.0, abs(loss))
    assert ref.err(gc.g64(name)[b], g) <= 1e-11


@pytest.mark.parametrize("name", ["single_w50_l2", "single_w16_l3", "coop_w256_l3", "coop_w64_l3",
                                  "flags_coop_weights_alphas", "flags_reward_rew_ur_sn", "zero_unit_coop"])
def test_gradient_is_the_finite_difference_slope_of_the_loss(name):
    p = gc.problem(name)
    S0, A = gc.inputs(name)
    g = gc.g64(name)[0]
    rng = np.random.default_rng(3)
    h = 1e-6
    for _ in range(6):
        t, j = int(rng.integers(A.shape[1])), int(rng.integers(A.shape[2]))
        if gc.CASES[name]["zero"] and j == 0:
            continue     # the zero unit's kink lies exactly at this coordinate's value
        d = np.zeros(A.shape[1:])
        d[t, j] = h
        up = ref.loss64(p, A[0].astype(np.float64) + d, s0=S0[0])      # perturbed in float64
        dn = ref.loss64(p, A[0].astype(np.float64) - d, s0=S0[0])
        fd = (up - dn) / (2 * h)
        assert abs(fd - g[t, j]) <= 1e-5 * np.max(np.abs(g)), (t, j, fd, g[t, j])


@pytest.mark.parametrize("name", gc.NAMES)
def test_no_relu_can_change_side_between_the_precisions(name):
    m, d = gc.margin(name)
    assert m >= gc.MARGIN_FACTOR * d, f"min |z| {m:.3e} < {gc.MARGIN_FACTOR:g} x float32 difference {d:.3e}"


@pytest.mark.parametrize("name", gc.NAMES)
def test_every_applicable_mutant_misses_the_bar_tenfold(name):
    bar = gc.bar(name)
    errs = gc.mutant_errors(name)
    assert errs, "no mutant applies"
    assert 0 < gc.e32(name) < 1e-4 and bar < 1e-3
    for label, e in errs.items():
        assert e >= gc.MUTANT_FACTOR * bar, f"{label}: e = {e:.3e} < 10 x bar = {10 * bar:.3e}"


def test_every_mutant_is_caught_by_some_case():
    caught = {label: [n for n in gc.NAMES if label in ref.applicable(gc.problem(n), gc.CASES[n]["H"])]
              for label in ref.MUTANTS}
    for label, names in caught.items():
        assert names, label
    assert caught["relu mask >= 0"] == ["zero_unit_coop", "zero_unit_single"]
    assert set(caught["one weight factor dropped"]) == {"flags_coop_weights_alphas", "flags_narrow_weights_alphas"}
    ur = {n for n in gc.NAMES if n.startswith("flags_reward_rew_ur")} | {"zero_unit_single"}
    assert ur <= set(caught["rew_std dropped"])


@pytest.mark.parametrize("name", ["coop_w64_l3", "flags_coop_weights_alphas", "zero_unit_single"])
def test_mutants_leave_the_forward_untouched(name):
    import torch
    p = gc.problem(name)
    S0, A = gc.inputs(name)
    base = ref._run(p, A[0], torch.float64, s0=S0[0])
    for label in ref.applicable(p, A.shape[1]):
        got = ref._run(p, A[0], torch.float64, mutant=label, s0=S0[0])
        for x, y in zip((base[0], base[2], base[3]), (got[0], got[2], got[3])):
            assert torch.equal(x, y), label
        assert not torch.equal(base[1], got[1]), label


def test_table_covers_what_the_issue_names():
    shape = lambda n: (gc.problem(n)["cfg"], gc.CASES[n])  # noqa: E731
    single = [n for n in gc.NAMES if not gc.coop_expected(n)]
    coop = [n for n in gc.NAMES if gc.coop_expected(n)]
    for n in gc.NAMES:      # the names say which kernel runs
        assert gc.coop_expected(n) == (not n.startswith(("single_", "flags_narrow", "zero_unit_single"))), n
    assert {(shape(n)[0]["W"], shape(n)[0]["L"]) for n in single} >= \
        {(W, L) for W in (16, 50, 100) for L in (1, 2, 3)} | {(300, 2), (512, 4)}
    assert {(shape(n)[0]["W"], shape(n)[0]["L"]) for n in coop} >= \
        {(W, L) for W in (64, 128, 256, 512) for L in (2, 3, 4)} - {(512, 4)}
    k0 = lambda names: {shape(n)[0]["s"] + shape(n)[0]["a"] for n in names}  # noqa: E731
    assert {6, 33} <= k0(single) and {2, 23, 32} <= k0(coop)
    assert any(shape(n)[0]["s"] == 1 for n in coop)
    assert {shape(n)[1]["H"] for n in single} >= {1, 2, 7, 16} and {shape(n)[1]["H"] for n in coop} >= {1, 5, 12}
    for names in (single, coop):
        assert {bool(shape(n)[0].get("reward")) for n in names} == {True, False}
    variants = {gc.CASES[n]["variant"] for n in gc.NAMES}
    import flag_cases as fc
    assert variants >= set(fc.GD_VARIANTS) | set(fc.REWARD) | {"norm_null", "no_state_cost", "no_action_cost"}
    assert [gc.CASES[n]["B"] for n in ("batch_b1", "batch_b3", "batch_b11")] == [1, 3, 11]
    assert all(gc.problem(n)["cfg"]["W"] == 512 and gc.coop_expected(n) for n in ("batch_b1", "batch_b3", "batch_b11"))
    for n in gc.HOP_CASES + gc.ABORT_CASES:
        assert gc.coop_expected(n), n
    S0, A = gc.inputs("batch_b11")
    assert len({x.tobytes() for x in S0}) == 11 and len({x.tobytes() for x in A}) == 11
