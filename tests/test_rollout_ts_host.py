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


def test_the_envelope_table_holds_every_row():
    """Every row of the envelope is in ENVELOPE (a dropped case fails its row), no case of it is in the first
    table, whose ten e32 values set the floor of every bar, and every case found its seed within the cap."""
    assert len(ref.NAMES) == 10 and not set(ref.ENVELOPE) & set(ref.CASES)
    for row, held in ref.ENVELOPE_ROWS.items():
        assert held(ref.ENVELOPE.values()), row
    for name in ref.ENV_NAMES:
        without = [c for n, c in ref.ENVELOPE.items() if n != name]
        assert not all(held(without) for held in ref.ENVELOPE_ROWS.values()), f"{name} belongs to no row"
        assert 1 <= ref.problem(name)["seed_tries"] <= ref.SEED_TRIES
    p = ref.problem("lv_pm1e4")
    r = ref.restate(p, np.float64)["states"]
    assert np.all(np.isfinite(r))
    lo, hi = ref.problem("lv_equal")["bounds"]
    assert lo.tobytes() == hi.tobytes()
    assert ref.problem("key_n_offset")["n_offset"] + 16 >= 1 << 31 and ref.problem("key_seed")["noise_seed"] >> 32


def test_the_first_tables_bars_are_the_recorded_ones():
    """The envelope moved no bar of the ten cases: profiles/rollout_ts/errors.json holds them from before it."""
    import json
    import pathlib
    rec = json.loads((pathlib.Path(__file__).resolve().parents[1] / "profiles/rollout_ts/errors.json").read_text())
    for name in ref.NAMES:
        for k in ref.KINDS:
            assert rec[name][k]["bar"] == ref.bars(name)[k] and rec[name][k]["e32"] == ref.e32(name)[k], (name, k)


@pytest.mark.parametrize("name", ref.ALL_NAMES)
def test_without_noise_it_is_the_oracles_rollout_on_the_mean_rows(name):
    p, c = ref.problem(name), ref.case(name)
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


@pytest.mark.parametrize("name", ref.ALL_NAMES)
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
    hit = [n for n in ref.ALL_NAMES if mutant in ref.applicable(n)]
    assert len(hit) >= 2, mutant
    for name in hit:
        assert _mutant_ratio(name, mutant) >= ref.MUTANT_FACTOR, (name, mutant, _mutant_ratio(name, mutant))


def test_the_float32_chain_meets_its_own_bar():
    for name in ref.ALL_NAMES:
        e, bar = ref.e32(name), ref.bars(name)
        assert all(e[k] <= bar[k] for k in ref.KINDS), name


# ---- the definition's noise is N(0, 1) and independent. Five-sigma bounds from the central limit theorem for n
# independent N(0, 1) draws: sd(mean) = 1 / sqrt(n), sd(var) = sqrt(2 / n), sd(fourth moment) = sqrt(96 / n),
# sd(correlation) = 1 / sqrt(n). The draws are deterministic, so nothing here can flake.
def _five_sigma(x):
    """x [streams][n], float64: the five statistics in units of their standard deviation, each at its worst."""
    n = x.shape[1]
    mean, var, m4 = x.mean(axis=1), x.var(axis=1), (x ** 4).mean(axis=1)
    corr = np.corrcoef(x)
    lag = np.array([np.corrcoef(r[:-1], r[1:])[0, 1] for r in x])
    return dict(mean=float(np.max(np.abs(mean)) * np.sqrt(n)), var=float(np.max(np.abs(var - 1)) / np.sqrt(2 / n)),
                fourth=float(np.max(np.abs(m4 - 3)) / np.sqrt(96 / n)),
                pairs=float(np.max(np.abs(corr - np.eye(len(x)))) * np.sqrt(n)),
                lag1=float(np.max(np.abs(lag)) * np.sqrt(n - 1)))


def _streams(x):
    """[q][t][n][j] -> one stream over n per (q, t, j)."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(x, np.float64), 2, -1)).reshape(-1, x.shape[2])


def test_the_definitions_normals_are_standard_and_independent():
    N, H, s = 4096, 2, 8
    eps = np.stack([ref.normals(ref.SEED64, 5, q, np.arange(N) + 3, H, s) for q in range(4)])
    x = _streams(eps)
    assert x.shape == (64, N)
    got = _five_sigma(x)
    print("FIVE SIGMA normals", got)
    assert all(v <= 5 for v in got.values()), got
    # the check bites: a stream that repeats across particles, steps or dimensions fails it, and so does a scale
    assert _five_sigma(np.concatenate([x[:63], x[:1]]))["pairs"] > 5 and _five_sigma(1.1 * x)["var"] > 5
    assert _five_sigma(np.repeat(x[:, ::2], 2, axis=1))["lag1"] > 5


def test_the_sampled_states_carry_that_noise_through_the_head():
    """Zero weights: m and the raw log-variance are the head's biases at every step, so (z - m) / (exp(lv / 2) *
    noise_scale) of the float64 restatement is the noise itself -- steps 3 to 6 of the header end to end."""
    p, c = ref.problem("moments"), ref.case("moments")
    assert (c.N, c.H, c.s, c.E * c.P, p["noise_seed"], p["iteration"], p["n_offset"]) == (4096, 2, 8, 4, ref.SEED64, 5, 3)
    bias = p["members"][0][-1][1].astype(np.float64)
    lv = ref.bounded_logvar(bias[c.s:], *(np.asarray(b, np.float64) for b in p["bounds"]))
    z = ref.ref64("moments")["states"]
    x = _streams((z - bias[:c.s]) / (np.exp(0.5 * lv) * np.float64(np.float32(c.noise))))
    got = _five_sigma(x)
    print("FIVE SIGMA states", got)
    assert all(v <= 5 for v in got.values()), got
    eps = np.stack([ref.normals(ref.SEED64, 5, q, np.arange(c.N) + 3, c.H, c.s) for q in range(4)])
    assert np.max(np.abs(x - _streams(eps))) < 1e-9


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
