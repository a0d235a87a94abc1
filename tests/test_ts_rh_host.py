"""CPU: the per-step member draw of the sampled rollout (tests/ts_rh_reference.py) -- its uniformity, its counter
space, the single mistakes the GPU test's checks must catch -- and what TrajectorySamplingCEMPlanner and CEMPlanner
refuse before anything needs a device."""
import numpy as np
import pytest
import torch

import rollout_ts_reference as ref
import ts_rh_reference as trh

SEED = ref.SEED64


@pytest.mark.parametrize("E", [2, 5, 8])
def test_the_member_draw_is_uniform(E):
    """Q = 256 rows x H = 20 steps x 20 iterations = 102400 draws: every member's count within five sigma of n / E."""
    e = np.concatenate([trh.members(SEED, it, 256, 20, E).reshape(-1) for it in range(20)])
    n = e.size
    assert n >= 10 ** 5 and e.min() >= 0 and e.max() < E
    sigma = np.sqrt(n * (1.0 / E) * (1.0 - 1.0 / E))
    counts = np.bincount(e, minlength=E)
    assert np.all(np.abs(counts - n / E) <= 5.0 * sigma), counts


def test_the_draw_is_the_top_bits_of_the_first_word():
    w = trh.member_words(SEED, 3, 7, 9)
    for E in (1, 2, 5, 8):
        want = np.array([[(int(x) * E) >> 32 for x in row] for row in w], np.int32)
        assert np.array_equal(trh.members(SEED, 3, 7, 9, E), want)
    assert np.all(trh.members(SEED, 3, 7, 9, 1) == 0)


@pytest.mark.parametrize("iteration", [0, 1, 255, (1 << 24) - 1])
def test_the_draws_counters_never_equal_a_noise_counter(iteration):
    """The noise's last word is (iteration << 8) | g with g < 158 (s <= 632); the draw's has g = 0xFF. The shift
    keeps the iteration out of the low byte, so no (iteration, g) pair of the noise gives the draw's word."""
    assert trh.MEMBER_GROUP >= trh.NOISE_GROUPS
    for s in (1, 17, 632):
        assert not trh.noise_counter_collides(iteration, 256, 9, s)
    draw = int(trh.member_counters(iteration, 1, 1)[0, 0, 3])
    noise = {(it << 8) | g for it in {0, 1, iteration, iteration ^ 0xFF, (iteration >> 8) & 0xFFFFFF} for g in range(158)}
    assert draw not in noise


def _applicable(mutant, c, Q, H):
    if c.E < 2:
        return False
    return dict(member_q_mod_E=True, draw_ignores_t=H > 1, draw_ignores_q=Q > 1,
                draw_ignores_iteration=c.iteration != 0)[mutant]


@pytest.mark.parametrize("mutant", trh.MEMBER_MUTANTS)
def test_each_single_mistake_is_caught(mutant):
    """On the bar table every mutant changes members_out wherever it applies, and -- where the wrong member sequence
    has noise of the states' size to act on -- misses the existing bar at least tenfold."""
    applied, worst = 0, 0.0
    for g in trh.BAR_GRID:
        p, Q = trh.grid_problem(*g), g[2]
        c, H = p["case"], p["actions"].shape[0]
        if not _applicable(mutant, c, Q, H):
            continue
        r64 = trh.grid_refs(*g)[0]
        bad = trh.restate(p, Q, np.float64, mutant=mutant)
        if np.array_equal(bad["members"], r64["members"]):
            continue                        # (a short sequence the mistake happens to reproduce)
        applied += 1
        bars = trh.grid_bars(*g)[0]
        miss = max(ref.err(bad[k], r64[k]) / bars[k] for k in ref.KINDS)
        print(f"MUTANT {mutant} {g}: misses the bar {miss:.1f}-fold")
        assert miss >= ref.MUTANT_FACTOR, (g, miss)
        worst = max(worst, miss)
    assert applied >= 3, applied


def test_the_draw_depends_on_q_t_iteration_and_both_key_words():
    base = trh.members(SEED, 3, 7, 9, 5)
    assert len({tuple(r) for r in base}) > 1 and len({tuple(c) for c in base.T}) > 1
    for other in (trh.members(SEED, 4, 7, 9, 5), trh.members(SEED & 0xFFFFFFFF, 3, 7, 9, 5),
                  trh.members(SEED + 1, 3, 7, 9, 5)):
        assert not np.array_equal(base, other)


# ---- the planners' host-side refusals
def _plan(planner, **kw):
    s0 = torch.zeros(5)
    return planner.plan_detailed(s0, None, None, None, 4, num_candidates=64, seed=1, **kw)


@pytest.mark.parametrize("kw, exc", [
    (dict(particle_mode="ts1"), ValueError), (dict(particle_mode=1), ValueError), (dict(particle_mode=None), ValueError),
    (dict(particles=0), ValueError), (dict(particles=-1), ValueError), (dict(particles=1.5), ValueError),
    (dict(particles=True), ValueError), (dict(particle_noise=-0.5), ValueError),
    (dict(particle_noise=float("nan")), ValueError), (dict(particle_seed=-3), ValueError),
    (dict(keep_elites=True), ValueError), (dict(keep_elites=1.5), ValueError), (dict(keep_elites=7), ValueError),
    (dict(warm_std=-1.0), ValueError), (dict(shift=-1), ValueError),
    (dict(keep_elites=0, carry=np.zeros((1, 4, 2), np.float32)), ValueError),
    (dict(keep_elites=2, carry=np.zeros((3, 4, 2), np.float32)), ValueError),
    (dict(distributed=True), NotImplementedError), (dict(noise_beta=1.0), NotImplementedError),
    (dict(noise_mix=np.eye(4, dtype=np.float32)), NotImplementedError), (dict(precision="f16x3"), NotImplementedError),
    (dict(device="cpu"), NotImplementedError),
], ids=lambda v: None if isinstance(v, type) else "-".join(f"{k}" for k in v))
def test_the_new_planners_kwarg_errors_need_no_gpu(kw, exc):
    from mbrl_amd import TrajectorySamplingCEMPlanner as TS
    with pytest.raises(exc):
        _plan(TS, **kw)
    if exc is NotImplementedError or "particle" in next(iter(kw)):
        with pytest.raises(exc):
            TS.plan_batch(torch.zeros(2, 5), None, None, None, 4, num_candidates=64, seed=1, **kw)


def test_the_new_planner_is_a_warm_starting_memo_planner_with_its_defaults():
    from mbrl_amd import ModelPlanner, TrajectorySamplingCEMPlanner as TS
    assert issubclass(TS, ModelPlanner) and TS.warm_starts is True and TS.plan_memo is True
    assert TS.ts_defaults == dict(particles=1, particle_mode="fixed", warm_start=True, keep_elites=0.3)
    with pytest.raises(TypeError, match="memos"):
        TS.plan_batch(torch.zeros(2, 5), None, None, None, 4, num_candidates=64, seed=1,
                      carry=np.zeros((1, 4, 2), np.float32))


@pytest.mark.parametrize("kw", [dict(warm_start=True), dict(keep_elites=2), dict(warm_std=0.2),
                                dict(keep_elites=1, carry=np.zeros((1, 4, 2), np.float32)), dict(distributed=True)],
                         ids=lambda kw: "-".join(kw))
def test_cem_planner_with_particles_still_refuses_the_receding_horizon_kwargs(kw):
    from mbrl_amd import CEMPlanner
    with pytest.raises(NotImplementedError):
        _plan(CEMPlanner, particles=2, **kw)


def test_the_batched_cem_entries_still_refuse_particles():
    from mbrl_amd import CEMPlanner, RecedingHorizonCEMPlanner, planners
    s0 = torch.zeros(2, 5)
    for call in (CEMPlanner.plan_batch, planners.cem_plan_batch, planners.cem_plan_batch_rh,
                 RecedingHorizonCEMPlanner.plan_batch):
        with pytest.raises(NotImplementedError, match="particles=2"):
            call(s0, None, None, None, 4, num_candidates=64, seed=1, particles=2)
