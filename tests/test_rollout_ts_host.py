"""CPU: the trajectory-sampling rollout's restatement (tests/rollout_ts_reference.py) against the oracle it is
built from, the sensitivity of the GPU test's bar to every single mistake, and CEMPlanner's particle kwargs."""
import functools

import numpy as np
import pytest
import torch

import rollout_ts_reference as ref
from oracle import cem as ocem
from oracle import philox


def test_the_case_table_covers_every_dimension():
    cs = ref.CASES.values()
    assert {c.N for c in cs} >= set(ref.DIMENSIONS["N"]) and {c.H for c in cs} >= set(ref.DIMENSIONS["H"])
    assert {(c.s, c.a) for c in cs} >= set(ref.DIMENSIONS["sa"]) and {c.W for c in cs} >= set(ref.DIMENSIONS["W"])
    assert {c.L for c in cs} >= set(ref.DIMENSIONS["L"]) and {(c.E, c.P) for c in cs} >= set(ref.DIMENSIONS["EP"])
    assert {c.norm for c in cs} >= set(ref.DIMENSIONS["norm"]) and any(c.offset for c in cs)
    assert any(not c.state_cost for c in cs) and any(not c.action_cost for c in cs)
    # the raw log-variances lie below, between and above the bounds in every case
    for name in ref.NAMES:
        p, c = ref.problem(name), ref.CASES[name]
        lo, hi = p["bounds"]
        bias = p["members"][0][-1][1][c.s:]
        assert np.any(bias < lo - 1) and np.any(bias > hi + 1) and np.any((bias > lo + 0.5) & (bias < hi - 0.5)), name


@pytest.mark.parametrize("name", ref.NAMES)
def test_without_noise_it_is_the_oracles_rollout_on_the_mean_rows(name):
    p, c = ref.problem(name), ref.CASES[name]
    got = ref.restate(p, np.float32, noise_scale=0.0)
    mean_model = [[(w[:c.s], b[:c.s]) if i == len(layers) - 1 else (w, b) for i, (w, b) in enumerate(layers)]
                  for layers in p["members"]]
    costs, states = ocem.rollout(mean_model, p["norm"], p["cost"], p["s0"], p["actions"], store_states=True)
    for q in range(c.E * c.P):
        assert got["states"][q].tobytes() == states[q // c.P].tobytes(), q
        assert got["costs"][q].tobytes() == costs[q // c.P].tobytes(), q


def test_row_zero_iteration_zero_draws_the_proposals_normals():
    seed, H, N, s = 99, 3, 7, 9
    mine = ref.normals(seed, 0, 0, np.arange(N) + 2, H, s)
    theirs = philox.cem_normals(seed, 0, np.arange(N) + 2, H, s)     # counter (n, t, 0, d >> 2)
    assert mine.dtype == np.float32 and mine.tobytes() == theirs.tobytes()
    assert ref.normals(seed, 1, 0, np.arange(N), H, s).tobytes() != ref.normals(seed, 0, 0, np.arange(N), H, s).tobytes()
    assert ref.normals(seed, 0, 1, np.arange(N), H, s).tobytes() != ref.normals(seed, 0, 0, np.arange(N), H, s).tobytes()


@pytest.mark.parametrize("name", ref.NAMES)
def test_no_relu_changes_side_between_float32_and_float64(name):
    r64, r32 = ref.ref64(name), ref.ref32(name)
    assert r64["pre"].keys() == r32["pre"].keys() and r64["pre"]
    for k in r64["pre"]:
        assert np.array_equal(r64["pre"][k] > 0, r32["pre"][k] > 0), (name, k)


@functools.lru_cache(maxsize=None)
def _mutant_ratio(name, mutant):
    bar = ref.bars(name)
    e = ref.errors(name, ref.restate(ref.problem(name), np.float64, mutant=mutant))
    return max((e[k] / bar[k]) if bar[k] > 0 else (np.inf if e[k] > 0 else 0.0) for k in ref.KINDS)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_each_single_mistake_misses_the_bar_tenfold(mutant):
    hit = [n for n in ref.NAMES if mutant in ref.applicable(n)]
    assert len(hit) >= 2, mutant
    for name in hit:
        assert _mutant_ratio(name, mutant) >= ref.MUTANT_FACTOR, (name, mutant, _mutant_ratio(name, mutant))


def test_the_float32_chain_meets_its_own_bar():
    for name in ref.NAMES:
        e, bar = ref.e32(name), ref.bars(name)
        assert all(e[k] <= bar[k] for k in ref.KINDS), name


# ---- CEMPlanner's kwargs, without a GPU
def _plan(**kw):
    from mbrl_amd import planners
    return planners.CEMPlanner.plan_detailed(torch.zeros(3), None, None, None, 4, num_candidates=16, seed=1, **kw)


@pytest.mark.parametrize("kw", [dict(particles=-1), dict(particles=1.5), dict(particles=True),
                                dict(particles=2, particle_noise=-0.5), dict(particle_noise=float("nan")),
                                dict(particles=2, particle_seed=-3), dict(particles=0, particle_noise=float("inf"))])
def test_bad_particle_values_are_value_errors_before_any_work(kw):
    with pytest.raises(ValueError, match="particle"):
        _plan(device="cpu", **kw)


@pytest.mark.parametrize("kw, named", [
    (dict(distributed=True), "distributed"),
    (dict(warm_start=True), "warm_start"),
    (dict(keep_elites=2), "keep_elites"),
    (dict(warm_std=0.3), "warm_std"),
    (dict(carry=torch.zeros(1, 4, 2)), "carry"),
    (dict(noise_beta=1.0), "noise_beta"),
    (dict(noise_mix=np.eye(4, dtype=np.float32)), "noise_mix"),
    (dict(precision="f16x3"), "precision"),
    (dict(precision="f16x6"), "precision"),
    (dict(device="cpu"), "device"),
])
def test_particles_refuse_what_the_sampled_plan_has_no_form_for(kw, named):
    with pytest.raises(NotImplementedError, match=r"particles=2.*" + named):
        _plan(particles=2, **kw)


def test_plan_batch_refuses_particles():
    from mbrl_amd import planners
    for fn in (planners.CEMPlanner.plan_batch, planners.cem_plan_batch, planners.cem_plan_batch_rh):
        with pytest.raises(NotImplementedError, match="particles=3"):
            fn(torch.zeros(2, 3), None, None, None, 4, particles=3)
        with pytest.raises(ValueError, match="particles"):
            fn(torch.zeros(2, 3), None, None, None, 4, particles=-2)


def test_the_defaults_name_the_particle_kwargs_and_the_seed_is_derived():
    from mbrl_amd import planners
    d = planners.CEMPlanner.defaults
    assert (d["particles"], d["particle_noise"], d["particle_seed"]) == (0, 1.0, None)
    assert planners._ts_inputs(dict(particles=0, particle_noise=2.0)) is None
    assert planners._ts_inputs(dict(particles=4)) == dict(P=4, noise=1.0, seed=None)
    a, b = planners._ts_seed(7), planners._ts_seed(8)
    assert 0 <= a < 2 ** 64 and a != b and a != 7 and planners._ts_seed(7) == a
