"""CPU: receding-horizon CEM (warm start and elite carry-over) on the host -- the NumPy restatement
(tests/cem_rh_reference.py) against the oracle's plain plan, its counter-space rule, the host helpers and
settings of CEMPlanner, the gap condition that lets the GPU test (tests/test_gpu_cem_rh.py) demand
identical index sets, and the feature's premise in a closed loop. No GPU."""
import numpy as np
import pytest
import torch

import cem_rh_reference as rh
from oracle import cem as ocem
from oracle.philox import cem_actions

F32 = np.float32


def test_restatement_without_inputs_is_the_oracles_plain_plan():
    N, H, I = 64, 4, 3
    p = ocem.synth_problem(2, N=N, H=H)
    ref = ocem.cem_plan(p, N=N, H=H, num_iterations=I)
    K = max(1, int(N * ocem.CEM_DEFAULTS["elite_frac"]))
    got = rh.plan(p, N, H, K, I)
    for it in range(I):
        for k in ("costs", "returns", "elites", "mu", "sigma"):
            assert np.asarray(got[k][it]).tobytes() == np.asarray(ref[k][it]).tobytes(), (it, k)
    assert got["final_actions"].tobytes() == ref["final_actions"].tobytes()
    assert got["final_states"].tobytes() == ref["final_states"].tobytes()


def test_kept_rows_take_slots_and_every_other_draw_keeps_its_counter():
    N, H, K, Kc = 64, 4, 6, 3
    p = ocem.synth_problem(2, N=N, H=H)
    got = rh.plan(p, N, H, K, 3, keep=Kc, final=False)
    # iteration 0 has no kept set without a carry: the plain draw from the initial distribution
    assert np.array_equal(got["actions"][0], cem_actions(got["mu0"], got["sigma0"], -1.0, 1.0, p["rng_seed"], 0,
                                                         np.arange(N)))
    for it in (1, 2):
        plain = cem_actions(got["mu"][it - 1], got["sigma"][it - 1], -1.0, 1.0, p["rng_seed"], it, np.arange(N))
        A = got["actions"][it]
        assert np.array_equal(A[:, Kc:], plain[:, Kc:]), it
        assert np.array_equal(A[:, :Kc].transpose(1, 0, 2), got["kept"][it]), it
        # the kept rows are the previous iteration's Kc best, in ascending candidate index
        best = got["best"][it - 1]
        assert np.array_equal(best, np.sort(np.argsort(got["returns"][it - 1], kind="stable")[:Kc]))
        assert np.array_equal(got["kept"][it], got["actions"][it - 1][:, best].transpose(1, 0, 2))
    assert np.array_equal(got["carry"], got["kept"][3])
    assert np.array_equal(got["carry_returns"], got["returns"][2][got["best"][2]])


def test_cem_shift_carry_shift_repeat_clip():
    from mbrl_amd import cem_shift_carry
    carry = np.array([[[0.1, -2.0], [0.2, 0.3], [0.4, 5.0]],
                      [[1.0, 1.0], [-0.5, 0.5], [-3.0, 0.0]]], F32)           # [Kc = 2, H = 3, a = 2]
    got = cem_shift_carry(torch.from_numpy(carry), 1)
    want = np.array([[[0.2, 0.3], [0.4, 1.0], [0.4, 1.0]],
                     [[-0.5, 0.5], [-1.0, 0.0], [-1.0, 0.0]]], F32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(cem_shift_carry(carry, 0), np.clip(carry, -1.0, 1.0))
    assert np.array_equal(cem_shift_carry(carry, 2, -0.5, 0.5)[0], np.array([[0.4, 0.5]] * 3, F32))
    assert cem_shift_carry(np.zeros((0, 3, 2), F32), 1).shape == (0, 3, 2)
    with pytest.raises(ValueError):
        cem_shift_carry(carry, 3)            # no step left
    with pytest.raises(ValueError):
        cem_shift_carry(carry[0], 1)         # not [Kc, H, a]


def _plan_settings(**kw):
    from mbrl_amd import CEMPlanner
    return CEMPlanner._settings_build(None, 5, dict(seed=1, **kw))


def _settings(**kw):
    """The receding-horizon settings of a plan with these kwargs (its K from the plan's own settings)."""
    from mbrl_amd.planners import _rh_settings
    return _rh_settings(kw, _plan_settings(**kw)["K"])


def test_keep_elites_resolves_counts_and_fractions():
    base = dict(num_candidates=200, num_elites=20)
    st = _settings(**base)
    assert (st["Kc"], st["warm_start"], st["shift"], st["warm_std"]) == (0, False, 1, None)
    assert _settings(keep_elites=7, **base)["Kc"] == 7
    assert _settings(keep_elites=20, **base)["Kc"] == 20
    assert _settings(keep_elites=0.3, **base)["Kc"] == 6
    assert _settings(keep_elites=0.26, **base)["Kc"] == 5        # rounded down
    assert _settings(keep_elites=0.01, **base)["Kc"] == 1        # at least one
    assert _settings(keep_elites=0.5, num_candidates=200)["Kc"] == 10   # of the default num_elites = N // 10
    assert _settings(keep_elites=3.0, **base)["Kc"] == 3
    for bad in (21, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            _settings(keep_elites=bad, **base)
    assert _settings(warm_start=True, shift=2, warm_std=0.25, **base)["warm_std"] == 0.25
    assert _settings(warm_std="keep", **base)["warm_std"] == "keep"
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _settings(warm_std=bad, **base)
    with pytest.raises(ValueError):
        _settings(shift=-1, **base)


def test_planner_has_no_warm_starts_attribute():
    """parallel.py keys on `warm_starts` to pass initial_trajectories to plan_batch; CEM's batch has none."""
    from mbrl_amd import CEMPlanner
    assert not hasattr(CEMPlanner, "warm_starts")


@pytest.mark.parametrize("kw", [dict(warm_start=True), dict(keep_elites=3), dict(keep_elites=0.5),
                                dict(warm_std=0.3), dict(carry=np.zeros((1, 5, 1), F32))])
def test_sharded_and_batched_plans_refuse_the_new_kwargs(kw):
    from mbrl_amd import CEMPlanner
    from mbrl_amd.planners import cem_plan_batch
    name = next(iter(kw))
    s0 = torch.zeros(5)
    with pytest.raises(NotImplementedError, match=name):
        CEMPlanner.plan(s0, None, None, None, 5, distributed=True, **kw)
    with pytest.raises(NotImplementedError, match=name):
        CEMPlanner.plan_batch(s0[None], None, None, None, 5, **kw)
    with pytest.raises(NotImplementedError, match=name):
        cem_plan_batch(s0[None], None, None, None, 5, **kw)


def test_receding_horizon_inputs_from_the_previous_plan():
    from mbrl_amd.planners import _rh_inputs, mppi_warm_start_rows

    def inputs(traj, **kw):
        return _rh_inputs(_plan_settings(**kw), traj, kw)
    acts = torch.tensor([[0.1], [0.2], [1.5], [0.4], [0.5]])
    traj = (None, acts)
    assert inputs(traj) is None                                 # nothing switched on: the plain path
    assert inputs(None, warm_start=True) is None                # an episode's first step
    assert inputs(traj, warm_start=False, warm_std=0.2) is None
    got = inputs(traj, warm_start=True)
    assert np.array_equal(got["mu_rows"], mppi_warm_start_rows(acts, 5, 1, -1.0, 1.0))
    assert got["sigma_rows"] is None and got["carry"] is None and got["Kc"] == 0
    got = inputs(traj, warm_start=True, warm_std=0.2, shift=2)
    assert np.array_equal(got["mu_rows"], mppi_warm_start_rows(acts, 5, 2, -1.0, 1.0))
    assert np.array_equal(got["sigma_rows"], np.full((5, 1), 0.2, F32))
    prev = np.array([[0.5], [0.4], [0.3], [0.2], [0.1]], F32)
    got = inputs(traj, warm_start=True, warm_std="keep", prev_sigma=prev)
    assert np.array_equal(got["sigma_rows"], np.array([[0.4], [0.3], [0.2], [0.1], [0.1]], F32))
    with pytest.raises(ValueError, match="prev_sigma"):
        inputs(traj, warm_start=True, warm_std="keep")
    for bad in (0.0, float("nan"), -0.1):                       # the C call's MBRL_EINVAL, made on the host
        prev[2, 0] = bad
        with pytest.raises(ValueError, match="finite and > 0"):
            inputs(traj, warm_start=True, warm_std="keep", prev_sigma=prev)
    kw = dict(num_candidates=100, keep_elites=2)
    got = inputs(None, carry=torch.zeros(2, 5, 1), **kw)
    assert got["carry"].shape == (2, 5, 1) and got["mu_rows"] is None and got["Kc"] == 2
    assert inputs(None, **kw) == dict(mu_rows=None, sigma_rows=None, carry=None, Kc=2)   # keeps rows: the rh path
    with pytest.raises(ValueError):
        inputs(None, carry=torch.zeros(3, 5, 1), **kw)
    with pytest.raises(ValueError, match="keep_elites == 0"):
        inputs(None, carry=torch.zeros(2, 5, 1))
    with pytest.raises(ValueError):
        inputs(None, num_candidates=100, keep_elites=11)        # more than num_elites = 10


@pytest.fixture(scope="module")
def case_plans():
    out = []
    for case in rh.CASES:
        p, kw = rh.make_case(case)
        out.append((case, rh.plan(p, case[3], rh.SMALL["H"], rh.SMALL["K"], rh.SMALL["I"], final=False, **kw)))
    return out


def test_gpu_fixture_cases_cover_the_shape_envelope():
    axes = list(zip(*[c[:6] for c in rh.CASES]))
    assert set(zip(axes[0], axes[1])) == {(64, 1), (256, 2)}
    assert set(axes[2]) == {1, 5, 8} and set(axes[3]) == {64, 100} and set(axes[4]) == {1, 2}
    assert set(axes[5]) == {0, 1, 3, 8}
    combos = {c[6] for c in rh.CASES}
    assert {(), ("mu",), ("sigma",), ("carry",), ("mu", "sigma", "carry")} <= combos


def test_gpu_fixture_cases_keep_their_selections_clear_of_ties(case_plans):
    """At every iteration of every fixture case the K-th and (K + 1)-th return, and the Kc-th and
    (Kc + 1)-th, differ by more than 1e-4 relative -- ten times the 1e-5 cost bar -- so costs within the bar
    give the same index sets and the GPU test may demand them identical."""
    for case, res in case_plans:
        g = rh.case_gaps(res, rh.SMALL["K"], case[5])
        print(f"{rh.case_id(case)}: smallest gap {g:.3g}")
        assert g > rh.GAP_MIN, (rh.case_id(case), g)
        for ret in res["returns"]:
            assert np.isfinite(ret).all()


def test_warm_start_with_carry_is_no_worse_than_cold_at_two_iterations():
    """The feature's premise on the restatement alone: a closed loop of 10 control steps with the synthetic
    cartpole model as its own environment, N = 256, H = 12, K = 25. Summed realised cost of cold I = 2,
    warm start with keep = 7 at I = 2, and cold I = 5 (recorded in DESIGN.md); asserted: warm <= cold I = 2
    over 3 seeds."""
    N, H, K, steps = 256, 12, 25, 10
    for seed in range(3):
        p = ocem.synth_problem(2, seed=9000 + seed, N=N, H=H)
        cold2 = rh.closed_loop(p, steps, N, H, K, 2, seed0=100 * seed)
        warm2 = rh.closed_loop(p, steps, N, H, K, 2, keep=7, warm=True, seed0=100 * seed)
        cold5 = rh.closed_loop(p, steps, N, H, K, 5, seed0=100 * seed)
        print(f"closed loop seed {seed}: cold I=2 {cold2:.4f}, warm keep=7 I=2 {warm2:.4f}, cold I=5 {cold5:.4f}")
        assert warm2 <= cold2, (seed, warm2, cold2)
