"""CPU: what the planners' host code decides before and after the C call -- the settings dicts of
CEMPlanner and MPPIPlanner (every key, compared with literal dicts), the float32 rounding of the
default init_std, the single seed draw from the global NumPy RNG, the argument errors and their
messages, the layout of the plan's output buffer (states, actions, mu, sigma at 0, H s, H (s + a),
H (s + 2 a)) and the plan tail that hands states and actions back in one host tensor."""
import numpy as np
import pytest
import torch

from mbrl_amd import env
from mbrl_amd.planners import CEMPlanner, MPPIPlanner

CEM_BASE = dict(N=1000, K=100, H=7, I=5, alpha=0.1, lo=-1.0, hi=1.0, init_std=0.5, seed=11, distributed=False,
                keep=False, record=False, events=None, plan_events=None, adim=6, precision=0)
MPPI_BASE = dict(N=1000, H=7, I=1, temperature=1.0, alpha=0.0, update_sigma=False, lo=-1.0, hi=1.0, init_std=0.5,
                 seed=11, shift=1, keep=False, record=False, events=None, plan_events=None, adim=6, precision=0)
HOOKS = [object()], [object(), object()]


@pytest.fixture(scope="module")
def sampler():
    """The synthetic problems' sampler: partial(_sample_action, action_spec=(6 dims, -1, 1))."""
    from mbrl_amd import synthetic
    return synthetic.make_problem(3, N=64, H=4)["sample_action"]


# (kwargs beside seed=11, the sampler: "synthetic", None or an action spec's (dim, lo, hi), what
# changes in the expected dict)
SHARED_CASES = {
    "defaults": ({}, "synthetic", {}),
    "action_bounds": (dict(action_bounds=(-2.0, 0.5)), "synthetic", dict(lo=-2.0, hi=0.5, init_std=0.625)),
    "init_std": (dict(init_std=0.2), "synthetic", dict(init_std=0.2)),
    "no_sampler": ({}, None, dict(adim=None)),
    "no_sampler_bounds": (dict(action_bounds=[0, 3]), None, dict(lo=0.0, hi=3.0, init_std=0.75, adim=None)),
    "spec_bounds": ({}, (2, -0.5, 0.25), dict(lo=-0.5, hi=0.25, init_std=0.1875, adim=2)),
    "spec_bounds_clipped": ({}, (3, -10.0, 10.0), dict(lo=-3.0, hi=3.0, init_std=1.5, adim=3)),
    "record": (dict(record=True), "synthetic", dict(record=True)),
    "return_device": (dict(return_device=1), "synthetic", dict(keep=True)),
    "hooks": (dict(rollout_events=HOOKS[0], plan_events=HOOKS[1]), "synthetic",
              dict(events=HOOKS[0], plan_events=HOOKS[1])),
    "alpha_iterations": (dict(alpha="0.25", num_iterations=3.0, num_candidates=50), "synthetic",
                         dict(alpha=0.25, I=3, N=50, K=5)),
    "f32": (dict(precision="f32"), "synthetic", dict(precision=0)),
    "f16x3": (dict(precision="f16x3"), "synthetic", dict(precision=1)),
    "f16x6": (dict(precision="F16X6"), "synthetic", dict(precision=2)),
}
CEM_CASES = {
    "num_elites_none_small": (dict(num_candidates=7, num_elites=None), "synthetic", dict(N=7, K=1)),
    "num_elites_none": (dict(num_candidates=64), "synthetic", dict(N=64, K=6)),
    "num_elites": (dict(num_candidates=64, num_elites=64), "synthetic", dict(N=64, K=64)),
    "distributed": (dict(distributed=True), "synthetic", dict(distributed=True)),
}
MPPI_CASES = {
    "mppi_own": (dict(temperature=0.5, update_sigma=1, shift=0, num_iterations=2), "synthetic",
                 dict(temperature=0.5, update_sigma=True, shift=0, I=2)),
}


def _sampler(which, synthetic_sampler):
    if which == "synthetic" or which is None:
        return synthetic_sampler if which else None
    return env.sample_action_fn(env.BoundedActionSpec(*which))


def _expected(base, changes):
    return {k: v for k, v in dict(base, **changes).items() if k in base}


@pytest.mark.parametrize("name", list(SHARED_CASES) + list(CEM_CASES))
def test_cem_settings_build_returns_exactly_this_dict(name, sampler):
    kw, which, changes = {**SHARED_CASES, **CEM_CASES}[name]
    got = CEMPlanner._settings_build(_sampler(which, sampler), 7, dict(kw, seed=11))
    assert got == _expected(CEM_BASE, changes)
    assert {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in _expected(CEM_BASE, changes).items()}


@pytest.mark.parametrize("name", list(SHARED_CASES) + list(MPPI_CASES))
def test_mppi_settings_build_returns_exactly_this_dict(name, sampler):
    kw, which, changes = {**SHARED_CASES, **MPPI_CASES}[name]
    got = MPPIPlanner._settings_build(_sampler(which, sampler), 7, dict(kw, seed=11))
    assert got == _expected(MPPI_BASE, changes)
    assert {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in _expected(MPPI_BASE, changes).items()}


@pytest.mark.parametrize("planner", [CEMPlanner, MPPIPlanner])
def test_default_init_std_is_a_float32_quotient(planner):
    """(hi - lo) / 4 is taken in float32: the double difference is rounded to float32, divided there,
    and the quotient widened again. (-0.3, 0.7) gives 0.25 either way; (-0.1, 0.2) gives
    0.07500000298023224 where double arithmetic would give 0.07500000000000001."""
    st = planner._settings_build(None, 3, dict(action_bounds=(-0.3, 0.7), seed=1))
    assert st["init_std"] == 0.25
    st = planner._settings_build(None, 3, dict(action_bounds=(-0.1, 0.2), seed=1))
    assert (0.2 - -0.1) / 4 == 0.07500000000000001
    assert st["init_std"] == float(np.float32(0.2 - -0.1) / np.float32(4.0)) == 0.07500000298023224
    assert (st["lo"], st["hi"]) == (-0.1, 0.2)      # the bounds themselves stay doubles


def _rng_state():
    s = np.random.get_state()
    return (s[0], s[1].tolist()) + tuple(s[2:])


@pytest.mark.parametrize("planner", [CEMPlanner, MPPIPlanner])
def test_seed_none_takes_one_draw_from_the_global_numpy_rng(planner, sampler):
    np.random.seed(123)
    want = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
    after = _rng_state()
    np.random.seed(123)
    st = planner._settings_build(sampler, 4, dict(num_candidates=64))
    assert st["seed"] == want and type(st["seed"]) is int and _rng_state() == after
    assert planner._settings_build(sampler, 4, dict(num_candidates=64, seed=None))["seed"] != want
    # a seed given: no draw
    np.random.seed(123)
    before = _rng_state()
    assert planner._settings_build(sampler, 4, dict(num_candidates=64, seed=0))["seed"] == 0
    assert planner._settings_build(None, 4, dict(seed=2 ** 63 + 5))["seed"] == 2 ** 63 + 5
    assert _rng_state() == before
    if planner is CEMPlanner:                        # the cached front of the same build
        assert CEMPlanner._settings(sampler, 4, dict(num_candidates=64, seed=9))["seed"] == 9
        assert _rng_state() == before
        assert CEMPlanner._settings(sampler, 4, dict(num_candidates=64))["seed"] == want
        assert _rng_state() == after


@pytest.mark.parametrize("K,N", [(0, 64), (65, 64), (-1, 8), (2, 1)])
def test_cem_num_elites_outside_1_to_n_raises(K, N):
    with pytest.raises(ValueError, match=rf"need 1 <= num_elites \({K}\) <= num_candidates \({N}\)"):
        CEMPlanner._settings_build(None, 4, dict(num_candidates=N, num_elites=K, seed=1))


def test_cem_num_elites_none_with_no_candidates_raises():
    with pytest.raises(ValueError, match=r"need 1 <= num_elites \(1\) <= num_candidates \(0\)"):
        CEMPlanner._settings_build(None, 4, dict(num_candidates=0, seed=1))


@pytest.mark.parametrize("t,shown", [(0, "0.0"), (-1.5, "-1.5"), (float("nan"), "nan"), (float("inf"), "inf")])
def test_mppi_temperature_must_be_finite_and_positive(t, shown):
    with pytest.raises(ValueError, match=f"temperature must be finite and > 0, got {shown}$"):
        MPPIPlanner._settings_build(None, 4, dict(temperature=t, seed=1))


@pytest.mark.parametrize("N,I", [(0, 1), (1, 0), (-3, 2)])
def test_mppi_needs_a_candidate_and_an_iteration(N, I):
    with pytest.raises(ValueError, match=rf"need num_candidates \({N}\) >= 1 and num_iterations \({I}\) >= 1"):
        MPPIPlanner._settings_build(None, 4, dict(num_candidates=N, num_iterations=I, seed=1))


def test_unknown_precision_raises():
    for planner in (CEMPlanner, MPPIPlanner):
        with pytest.raises(ValueError, match="precision must be one of .*got 'bf16'"):
            planner._settings_build(None, 4, dict(precision="bf16", seed=1))


def test_mppi_distributed_raises_before_anything_else(sampler):
    """NotImplementedError from the settings, which plan_detailed builds before it looks for a device
    (on a host without a GPU the device lookup would raise RuntimeError instead), and before the seed
    draw."""
    np.random.seed(5)
    before = _rng_state()
    with pytest.raises(NotImplementedError, match=r"distributed=True \(sharded MPPI\) is not implemented"):
        MPPIPlanner._settings_build(sampler, 4, dict(distributed=True))
    with pytest.raises(NotImplementedError, match=r"distributed=True \(sharded MPPI\) is not implemented"):
        MPPIPlanner.plan(torch.zeros(17), lambda s, a: s, lambda s, a: s[:, 0], sampler, 4, distributed=True)
    assert _rng_state() == before
    with pytest.raises(NotImplementedError, match="batched MPPI plans are not implemented"):
        MPPIPlanner.plan_batch(torch.zeros(2, 17), None, None, sampler, 4)


@pytest.mark.parametrize("H,s,a", [(1, 1, 1), (3, 5, 2), (4, 17, 6)])
def test_stage_out_cuts_the_output_buffer_at_the_documented_offsets(H, s, a):
    from mbrl_amd import planners
    assert planners._layout(H, s, a) == (H * s, H * (s + a), H * (s + 2 * a), H * (s + 3 * a))
    n = H * (s + 3 * a)
    arr = np.arange(n + s, dtype=np.float32)          # (a staging buffer keeps s0 behind the outputs)
    res = planners._stage_out(arr, H, s, a)
    assert res.pop("_host") is True and sorted(res) == ["actions", "mu", "sigma", "states"]
    want = dict(states=(0, s), actions=(H * s, a), mu=(H * (s + a), a), sigma=(H * (s + 2 * a), a))
    for k, (start, width) in want.items():
        assert res[k].dtype == torch.float32 and tuple(res[k].shape) == (H, width), k
        assert np.array_equal(res[k].numpy(), np.arange(start, start + H * width, dtype=np.float32).reshape(H, width)), k
    arr[:] = -1.0                                      # the results are copies, not views of the staging
    for k, (start, width) in want.items():
        assert float(res[k][0, 0]) == start and float(res[k][-1, -1]) == start + H * width - 1, k


@pytest.mark.parametrize("H,s,a", [(1, 1, 1), (3, 5, 2)])
def test_finish_hands_states_and_actions_back_as_views_of_one_host_tensor(H, s, a):
    from mbrl_amd import planners
    both = torch.arange(H * (s + a), dtype=torch.float32)
    mu = torch.zeros(H, a)
    res = dict(states=both[:H * s].view(H, s), actions=both[H * s:].view(H, a), mu=mu, _both=both)
    out = planners._finish(res, False)
    assert out is res and "_both" not in out and out["mu"] is mu
    assert tuple(out["states"].shape) == (H, s) and tuple(out["actions"].shape) == (H, a)
    assert torch.equal(out["states"].reshape(-1), both[:H * s]) and torch.equal(out["actions"].reshape(-1), both[H * s:])
    base = out["states"].untyped_storage().data_ptr()
    assert out["actions"].untyped_storage().data_ptr() == base          # one host tensor behind both
    assert out["actions"].data_ptr() - out["states"].data_ptr() == 4 * H * s
    # keep=True leaves the tensors as they are; without "_both" each goes to the host by itself
    res = dict(states=both[:H * s].view(H, s), actions=both[H * s:].view(H, a), _both=both)
    st, ac = res["states"], res["actions"]
    out = planners._finish(res, True)
    assert out["states"] is st and out["actions"] is ac and "_both" not in out
    out = planners._finish(dict(states=st, actions=ac), False)
    assert torch.equal(out["states"], st) and torch.equal(out["actions"], ac)
