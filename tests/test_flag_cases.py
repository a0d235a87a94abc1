"""CPU check of the case table of tests/flag_cases.py, on the oracle alone: every (family, variant)
pair that tests/test_gpu_flags.py runs is one a wrong kernel could not pass, stays inside the split
kernels' operand range, and (whole plans) has no elite tie at the bar. These are conditions on the
chosen seeds and shapes, asserted -- not measurements. The gradient-descent families are held to the
outputs their GPU test compares (the optimised actions and states of the reference's host loop, plain
torch on the CPU); one flag is not visible there, see flag_cases.GD_BLIND."""
import numpy as np
import pytest

import flag_cases as fc

SENS_N = 64   # candidates the sensitivity mutants are rolled out on (a prefix of the family's own)


@pytest.mark.parametrize("family,variant", fc.pairs())
def test_pair_is_sensitive_and_in_range(family, variant):
    p = fc.problem(family, variant)
    A = fc.actions(p)
    worst, wmax = fc.magnitudes(p, A)
    assert worst < fc.RANGE_BAR, f"|state| or |layer input| reaches {worst}"
    assert wmax < fc.WEIGHT_BAR, f"|weight| reaches {wmax}"
    A = np.ascontiguousarray(A[:, :SENS_N])
    ret, states = fc.evaluate(p, A)
    assert np.all(np.isfinite(ret)) and np.all(np.isfinite(states))
    if variant == "no_cost":
        assert np.array_equal(ret, np.zeros_like(ret))       # exactly 0, not merely small
    if family in fc.GD_FAMILIES:
        return       # compared on the optimiser's outputs: test_gd_pair_is_sensitive_in_what_the_gpu_test_compares
    muts = fc.mutants(p)
    assert muts
    for label, q, moves_states in muts:
        r2, s2 = fc.evaluate(q, A)
        if family not in fc.STATES_ONLY:
            assert fc.rel_err(r2, ret) >= fc.MOVE_RETURNS, f"{label}: returns move by {fc.rel_err(r2, ret):.3e}"
        if moves_states:
            d = float(np.max(np.abs(s2[:, -1].astype(np.float64) - states[:, -1])))
            assert d >= fc.MOVE_STATES, f"{label}: final states move by {d:.3e}"


@pytest.mark.parametrize("family,variant", fc.pairs(*fc.GD_FAMILIES))
def test_gd_pair_is_sensitive_in_what_the_gpu_test_compares(family, variant):
    """test_gd_kernels compares the actions and states after GD_ITERS Adam steps with the reference's
    host loop. The same loop on each mutant's closures must leave those bars: the actions by
    MOVE_GD_ACTIONS, and (so) the comparison itself must fail. The one mutant that cannot be seen there,
    unnormalize_reward (flag_cases.GD_BLIND), is asserted to stay inside the bars, so that the gap is a
    recorded fact and not an assumption."""
    p = fc.problem(family, variant)
    A = fc.actions(p)
    st, ac = fc.gd_host_loop(p, A)
    assert np.all(np.isfinite(st)) and np.all(np.isfinite(ac))
    assert float(np.max(np.abs(ac - A[:, 0]))) >= 0.05      # the 8 steps of lr 0.01 really moved the actions
    muts = fc.mutants(p)
    assert [m for m in muts if m[0] not in fc.GD_BLIND]
    for label, q, _ in muts:
        st2, ac2 = fc.gd_host_loop(q, A)
        passes = np.allclose(ac2, ac, **fc.GD_ACTION_TOL) and np.allclose(st2, st, **fc.GD_STATE_TOL)
        d = float(np.max(np.abs(ac2 - ac)))
        if label in fc.GD_BLIND:
            assert passes, f"{label}: now visible (actions move by {d:.3e}); take it out of GD_BLIND"
        else:
            assert d >= fc.MOVE_GD_ACTIONS and not passes, f"{label}: actions move by {d:.3e}"


@pytest.mark.parametrize("variant", ["rew:ur+sn", "rew:ur"])
def test_the_gradient_case_does_show_unnormalize_reward(variant):
    """What the plan outputs above cannot show (GD_BLIND) the gradient comparison of
    tests/test_gpu_gd_grad.py can: the same family and variant as a gradient case (gd_grad_cases
    "flags_reward_*"), with rew_std left out of the backward pass, misses that test's bar tenfold."""
    import gd_grad_cases as gc
    name = "flags_reward_" + variant.replace(":", "_").replace("+", "_")
    cid, over, variants = fc.FAMILIES["gd_reward"]
    c = gc.CASES[name]
    assert (c["cid"], c["variant"]) == (cid, variant) and variant in variants
    assert c["over"] == {k: v for k, v in over.items() if k not in ("N", "H")} and c["H"] == over["H"]
    e = gc.mutant_errors(name)["rew_std dropped"]
    assert e >= gc.MUTANT_FACTOR * gc.bar(name), f"rew_std dropped: e = {e:.3e}, bar = {gc.bar(name):.3e}"


@pytest.mark.parametrize("family", fc.PLAN_FAMILIES)
def test_plan_has_no_elite_tie_at_the_bar(family):
    for variant in fc.FAMILIES[family][2]:
        _, gaps = fc.plan_gaps(fc.problem(family, variant))
        assert len(gaps) == fc.PLAN_ITERATIONS
        assert min(gaps) > fc.TIE_GAP, gaps


def test_table_covers_what_the_issue_names():
    assert len(fc.NORM_SUBSETS) == 8 and len({tuple(v.values()) for v in fc.NORM_SUBSETS.values()}) == 8
    for fam in ("traj_reg", "traj_coop", "traj_plain", "traj_fallback", "rollout_cid2"):
        assert set(fc.EIGHT) <= set(fc.FAMILIES[fam][2])
    for fam in ("rollout_ring_ereg", "rollout_ring_wide", "rollout_nonring", "rollout_r2", "rollout_tiles_cid2",
                "rollout_tiles_cid3", "rollout_pair", "rollout_split"):
        assert set(fc.FIVE) <= set(fc.FAMILIES[fam][2])
    # a cleared flag's statistics are NULL whenever no other flag needs them
    assert fc.null_stats(fc.problem("traj_coop", "norm:na")) == (True, False)
    assert fc.null_stats(fc.problem("traj_coop", "norm:us")) == (False, True)
    assert fc.null_stats(fc.problem("traj_coop", "norm_null")) == (True, True)
    w = fc.problem("rollout_cid2", "weights_alphas")["cost"]["weights"]
    assert np.sum(w == 0) == 1 and np.all((w == 0) | ((w >= 0.25) & (w < 3)))
