"""CPU: coloured-noise proposals on the host -- the power-law mixing matrix (planners.colored_noise_mix), the
NumPy restatement (tests/cem_noise_reference.py) against the white restatement, the gap condition that lets
the GPU test (tests/test_gpu_cem_noise.py) demand identical index sets, the planners' kwargs and refusals, and
the statistics of the mixed normals. No GPU."""
import numpy as np
import pytest
import torch

import cem_noise_reference as nr
import cem_rh_reference as rh
from oracle.philox import cem_actions, cem_normals

F32 = np.float32


def _mix64(H, beta):
    from mbrl_amd.planners import _colored_noise_mix64
    return _colored_noise_mix64(H, beta)


@pytest.mark.parametrize("H", [2, 3, 20, 30, 50, 64])
def test_mix_rows_have_unit_norm_and_the_power_law_spectrum(H):
    from mbrl_amd.planners import colored_noise_mix
    for beta in (0.0, 0.5, 1.0, 2.0, 4.0):
        C = _mix64(H, beta)
        assert np.abs(np.sqrt((C * C).sum(1)) - 1.0).max() < 1e-12
        C32 = colored_noise_mix(H, beta)
        assert C32.dtype == np.float32 and C32.shape == (H, H) and np.array_equal(C32, C.astype(F32))
    # beta = 0: orthogonal
    C0 = colored_noise_mix(H, 0.0).astype(np.float64)
    assert np.abs(C0 @ C0.T - np.eye(H)).max() < 1e-6
    # the energy at frequency k, summed over the columns, is proportional to s_k^2, s_0 = s_1 (the sqrt(2) of
    # the DC and Nyquist columns gives each of them the energy of a cos / sin pair: 2 H^2 s_k^2 before scaling)
    for beta in (0.5, 1.0, 2.0):
        energy = (np.abs(np.fft.rfft(_mix64(H, beta), axis=0)) ** 2).sum(1)
        k = np.arange(1, H // 2 + 1)
        s2 = np.concatenate([[(1.0 / H) ** -beta], (k / H) ** -beta])
        ratio = energy / s2
        assert np.abs(ratio / ratio[0] - 1.0).max() < 1e-9, (H, beta)


def test_mix_edge_cases():
    from mbrl_amd.planners import colored_noise_mix
    assert np.array_equal(colored_noise_mix(1, 1.0), np.ones((1, 1), F32))
    assert np.array_equal(colored_noise_mix(1, 0.0), np.ones((1, 1), F32))
    for bad in (-0.1, 4.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            colored_noise_mix(10, bad)
    with pytest.raises(ValueError):
        colored_noise_mix(0, 1.0)


def test_identity_mix_is_the_white_restatement():
    """np.array_equal over cem_rh_reference's fixture cases (an identity mix adds signed zeros only)."""
    H, K, I = rh.SMALL["H"], rh.SMALL["K"], rh.SMALL["I"]
    for case in rh.CASES:
        p, kw = rh.make_case(case)
        white = rh.plan(p, case[3], H, K, I, final=False, **kw)
        ident = nr.plan(p, case[3], H, K, I, mix=np.eye(H, dtype=F32), final=False, **kw)
        for k in ("costs", "returns", "elites", "best", "actions", "mu", "sigma", "kept"):
            for it, (x, y) in enumerate(zip(white[k], ident[k])):
                assert np.array_equal(x, y, equal_nan=True), (rh.case_id(case), k, it)
        assert np.array_equal(white["carry"], ident["carry"])


def test_no_mix_calls_the_plain_path(monkeypatch):
    calls = []
    real = rh.plan
    monkeypatch.setattr(rh, "plan", lambda *a, **k: calls.append(1) or real(*a, **k))
    p, kw = rh.make_case(rh.CASES[4])
    got = nr.plan(p, 100, 3, 8, 2, mix=None, final=False, **kw)
    assert calls == [1] and np.array_equal(got["mu_out"], real(p, 100, 3, 8, 2, final=False, **kw)["mu_out"])
    mu, sg = np.zeros((3, 5), F32), np.full((3, 5), 0.5, F32)
    assert np.array_equal(nr.mixed_actions(mu, sg, -1, 1, 7, 1, np.arange(9)), cem_actions(mu, sg, -1, 1, 7, 1, np.arange(9)))
    assert np.array_equal(nr.mixed_normals(None, 7, 1, np.arange(9), 3, 5), cem_normals(7, 1, np.arange(9), 3, 5))


def test_batched_form_offsets_the_candidate_index():
    p, kw = rh.make_case(rh.CASES[0])
    mix = nr.beta_mix(3)
    A0 = nr.proposals(np.zeros((3, 1), F32), np.full((3, 1), 0.5, F32), -1, 1, 5, 0, 64, mix=mix, b=2)
    assert np.array_equal(A0, nr.mixed_actions(np.zeros((3, 1), F32), np.full((3, 1), 0.5, F32), -1, 1, 5, 0,
                                               128 + np.arange(64), mix))
    one = nr.plan(p, 64, 3, 8, 2, mix=mix, final=False)
    same = nr.plan(p, 64, 3, 8, 2, mix=mix, b=0, s0=p["s0"], final=False)
    assert np.array_equal(one["mu_out"], same["mu_out"])


def test_gpu_fixture_cases_cover_the_shape_envelope():
    axes = list(zip(*[c[:8] for c in nr.CASES]))
    assert set(zip(axes[0], axes[1])) == {(64, 1), (256, 2)}
    assert set(axes[2]) == {1, 5, 8} and set(axes[3]) == {64, 100} and set(axes[4]) == {1, 2}
    assert set(axes[5]) == {0, 1, 3, 8} and set(axes[7]) == {3, 12}
    combos = {c[6] for c in nr.CASES}
    assert {(), ("mu",), ("sigma",), ("carry",), ("mu", "sigma", "carry")} <= combos
    assert len(nr.BATCH_CASES) == 6 and {len(c[6]) for c in nr.BATCH_CASES} == {1, 2, 5}
    for c in nr.BATCH_CASES:
        assert all("c" not in x for x in c[6]) or c[5] > 0


def test_gpu_fixture_cases_keep_their_selections_clear_of_ties():
    """The stored seeds: at every iteration of every fixture case (and of every problem of every fixture batch)
    the K-th and Kc-th return gaps on the restatement exceed GAP_MIN = 1e-4, ten times the 1e-5 cost bar, so the
    GPU test may demand identical index sets."""
    for case in nr.CASES:
        res = nr.cached(nr.case_plan, case, final=True)
        g = rh.case_gaps(res, nr.SMALL["K"], case[5])
        print(f"{nr.case_id(case)}: smallest gap {g:.3g}")
        assert g >= nr.GAP_MIN, (nr.case_id(case), g)
        assert all(np.isfinite(r).all() for r in res["returns"])
    for case in nr.BATCH_CASES + [nr.WIDE_BATCH_CASE]:
        g = min(rh.case_gaps(res, nr.SMALL["K"], case[5]) for res in nr.cached(nr.batch_case_plans, case, final=True))
        print(f"{nr.batch_case_id(case)}: smallest gap {g:.3g}")
        assert g >= nr.GAP_MIN, (nr.batch_case_id(case), g)


def test_find_seed_reproduces_a_stored_seed():
    case = nr.CASES[0]
    assert nr.find_seed(case) == case[-1]


# ---- kwargs
def _st(H=5, **kw):
    from mbrl_amd import CEMPlanner
    return CEMPlanner._settings_build(None, H, dict(seed=1, **kw))


def test_noise_kwargs_route_to_the_receding_horizon_path():
    from mbrl_amd import CEMPlanner
    from mbrl_amd.planners import _noise_inputs, _rh_inputs, _rh_with_noise, colored_noise_mix
    assert CEMPlanner.defaults["noise_beta"] == 0.0 and CEMPlanner.defaults["noise_mix"] is None
    assert _noise_inputs({}, 5) is None and _noise_inputs(dict(noise_beta=0.0, noise_mix=None), 5) is None
    assert _rh_with_noise(None, None) is None                      # the defaults: the plain path
    key, m = _noise_inputs(dict(noise_beta=1.0), 5)
    assert np.array_equal(m, colored_noise_mix(5, 1.0)) and key == ("beta", 5, 1.0)
    assert _noise_inputs(dict(noise_beta=1.0), 5)[1] is m and not m.flags.writeable   # built once per (H, beta)
    routed = _rh_with_noise(None, (key, m))                        # no warm start, nothing kept: still the rh path
    assert routed["Kc"] == 0 and routed["mu_rows"] is None and routed["carry"] is None and routed["mix"][1] is m
    kw = dict(num_candidates=100, keep_elites=2)
    routed = _rh_with_noise(_rh_inputs(_st(**kw), None, kw), (key, m))
    assert routed["Kc"] == 2 and routed["mix"][0] == key
    explicit = np.eye(5, dtype=np.float64)[::-1]
    key2, m2 = _noise_inputs(dict(noise_mix=torch.from_numpy(explicit.copy())), 5)
    assert m2.dtype == np.float32 and m2.flags["C_CONTIGUOUS"] and np.array_equal(m2, explicit)
    assert key2 == ("mix", 5, m2.tobytes())
    # RecedingHorizonCEMPlanner does not turn the noise on
    from mbrl_amd import RecedingHorizonCEMPlanner
    assert "noise_beta" not in RecedingHorizonCEMPlanner.rh_defaults
    assert "noise_mix" not in RecedingHorizonCEMPlanner.rh_defaults


def test_noise_kwargs_are_checked_on_the_host():
    from mbrl_amd import CEMPlanner, cem_plan_batch_rh
    from mbrl_amd.planners import _noise_inputs
    with pytest.raises(ValueError, match="not both"):
        _noise_inputs(dict(noise_beta=1.0, noise_mix=np.eye(5)), 5)
    for bad in (-1.0, 4.5, float("nan")):
        with pytest.raises(ValueError, match="noise_beta"):
            _noise_inputs(dict(noise_beta=bad), 5)
    for bad in (np.eye(4), np.zeros((5, 4)), np.zeros(25)):
        with pytest.raises(ValueError, match="noise_mix must be"):
            _noise_inputs(dict(noise_mix=bad), 5)
    poisoned = np.eye(5, dtype=F32)
    poisoned[2, 3] = np.inf
    with pytest.raises(ValueError, match="finite"):
        _noise_inputs(dict(noise_mix=poisoned), 5)
    with pytest.raises(ValueError, match="horizon <= 64"):
        _noise_inputs(dict(noise_beta=1.0), 65)
    # ... and through the public entries, before anything touches a device
    s0 = torch.zeros(5)
    with pytest.raises(ValueError, match="finite"):
        CEMPlanner.plan(s0, None, None, None, 5, noise_mix=poisoned)
    with pytest.raises(ValueError, match="not both"):
        CEMPlanner.plan(s0, None, None, None, 5, noise_mix=np.eye(5), noise_beta=1.0)
    with pytest.raises(ValueError, match="noise_mix must be"):
        cem_plan_batch_rh(s0[None], None, None, None, 5, noise_mix=np.eye(4), seed=1)


@pytest.mark.parametrize("kw", [dict(noise_beta=1.0), dict(noise_mix=np.eye(5, dtype=F32))])
def test_plans_without_a_coloured_form_refuse_the_noise_kwargs(kw):
    from mbrl_amd import CEMPlanner, MPPIPlanner, RandomShootingPlanner
    from mbrl_amd.planners import cem_plan_batch
    name = next(iter(kw))
    s0 = torch.zeros(5)
    with pytest.raises(NotImplementedError, match=name):
        CEMPlanner.plan(s0, None, None, None, 5, distributed=True, **kw)
    with pytest.raises(NotImplementedError, match=name):
        CEMPlanner.plan_batch(s0[None], None, None, None, 5, **kw)
    with pytest.raises(NotImplementedError, match=name):
        cem_plan_batch(s0[None], None, None, None, 5, **kw)
    with pytest.raises(NotImplementedError, match=name):
        MPPIPlanner.plan(s0, None, None, None, 5, **kw)
    with pytest.raises(NotImplementedError, match=name):
        RandomShootingPlanner.plan(s0, None, None, None, 5, **kw)
    with pytest.raises(NotImplementedError, match=name):
        RandomShootingPlanner.plan_batch(s0[None], None, None, None, 5, **kw)


def test_mixed_normals_are_unit_variance_and_correlated_along_the_horizon():
    """4096 candidates, beta = 1, H = 30: the per-step sample variance within 0.1 of 1, and the lag-1
    autocorrelation at its expected value (C C^T)[t][t + 1] (rows of unit norm: a correlation), averaged over
    t, +- 0.05 -- which lies at least 0.2 above white's."""
    H, n = 30, 4096
    mix = nr.beta_mix(H, 1.0)
    e = nr.mixed_normals(mix, 123, 0, np.arange(n), H, 1)[:, :, 0].astype(np.float64)
    z = cem_normals(123, 0, np.arange(n), H, 1)[:, :, 0].astype(np.float64)
    var = e.var(axis=1)
    print(f"per-step variance in [{var.min():.3f}, {var.max():.3f}]")
    assert np.abs(var - 1.0).max() < 0.1
    C = mix.astype(np.float64)
    expected = float(np.mean(np.diag(C @ C.T, 1)))

    def lag1(x):
        x = x - x.mean(axis=1, keepdims=True)
        return float(np.mean((x[:-1] * x[1:]).mean(axis=1) / np.sqrt(x[:-1].var(axis=1) * x[1:].var(axis=1))))
    got, white = lag1(e), lag1(z)
    print(f"lag-1 autocorrelation: mixed {got:.3f} (expected {expected:.3f}), white {white:.3f}")
    assert abs(got - expected) < 0.05
    assert got > white + 0.2
