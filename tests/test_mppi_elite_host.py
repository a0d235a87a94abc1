"""CPU: MPPI over the K best on the host -- the five new C entries (names, the struct against a compiled C caller,
the sizing query, every argument check that fires before any launch), the planners' new kwargs, and the NumPy
restatement's own properties (tests/mppi_elite_reference.py), its plan fixtures' gap condition included. No GPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mppi_elite_reference as eref
import mppi_reference as mref
from conftest import REPO

HEADER = os.path.join(REPO, "include", "mbrl_cem.h")
F32 = np.float32
INF = float("inf")
NAN = float("nan")
NEW = ("mbrl_mppi_update_elite", "mbrl_mppi_update_elite_batch", "mbrl_mppi_elite_workspace_bytes",
       "mbrl_mppi_plan_elite", "mbrl_mppi_plan_elite_batch")


def _mppi(**kw):
    from mbrl_amd import _lib
    d = dict(N=256, H=4, iterations=2, update_sigma=1, temperature=1.0, alpha=0.0, lo=-1.0, hi=1.0, init_mu=0.0,
             init_sigma=0.5, seed=7)
    d.update(kw)
    return _lib.MppiParams(*[d[f] for f, _ in _lib.MppiParams._fields_])


def _params(K=25, sigma_min=0.0, sigma_max=INF, **kw):
    from mbrl_amd import _lib
    return _lib.MppiEliteParams(_mppi(**kw), K, 0, sigma_min, sigma_max)


def test_header_exported_list_and_library_agree_on_the_new_names():
    from mbrl_amd import _lib
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name) and name + "(" in text, name
        assert getattr(lib, name).argtypes is not None
    assert lib.mbrl_abi_version() == 13 and "#define MBRL_ABI_VERSION 13" in text      # additive within v13
    assert "MBRL_OPT_END = 23" in text                                                  # no new option id


def test_struct_layout_matches_a_compiled_c_caller():
    from mbrl_amd import _lib
    fields = ["mppi", "K", "sigma_min", "sigma_max"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("sizeof %zu\\n", sizeof(mbrl_mppi_elite_params));']
    lines += [f'printf("{f} %zu\\n", offsetof(mbrl_mppi_elite_params, {f}));' for f in fields]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        try:
            subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True, capture_output=True)
        except (FileNotFoundError, subprocess.CalledProcessError) as e:  # pragma: no cover
            pytest.skip(f"gcc unavailable: {e}")
        out = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True,
                                                           text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.MppiEliteParams) == int(out["sizeof"]) == ctypes.sizeof(_lib.MppiParams) + 16
    for f in fields:
        assert getattr(_lib.MppiEliteParams, f).offset == int(out[f]), f


BAD_PARAMS = [dict(N=0), dict(H=0), dict(iterations=0), dict(temperature=0.0), dict(temperature=NAN),
              dict(temperature=INF), dict(K=0), dict(K=-3), dict(K=257), dict(sigma_min=-0.1), dict(sigma_min=NAN),
              dict(sigma_max=NAN), dict(sigma_min=0.5, sigma_max=0.25), dict(sigma_min=INF, sigma_max=1.0)]


def test_sizing_query():
    from mbrl_amd import _lib
    lib = _lib.load()
    size = lib.mbrl_mppi_elite_workspace_bytes
    for sh in (_lib.MlpShape(17, 6, 512, 3, 1), _lib.MlpShape(5, 1, 256, 2, 5), _lib.MlpShape(24, 6, 512, 3, 1, 1)):
        for K in (1, 25, 256):
            good = _params(K=K)
            need = [size(ctypes.byref(sh), ctypes.byref(good), B) for B in (1, 2, 3, 8, 64)]
            assert all(x > 0 for x in need) and all(x <= y for x, y in zip(need, need[1:])) and need[-1] > need[0], need
            for B, x in zip((1, 2, 3, 8, 64), need):     # never below the plain query; room for a list and the keys
                plain = lib.mbrl_mppi_batch_workspace_bytes(ctypes.byref(sh), ctypes.byref(good.mppi), B)
                assert x >= plain + 8 * K + 4 * 256, (B, K)
            assert need[4] > 64 * (8 * K + 4 * 256)      # (B lists, B N keys)
            assert need[0] >= lib.mbrl_mppi_workspace_bytes(ctypes.byref(sh), ctypes.byref(good.mppi))
        good = _params()
        for B in (0, -1):
            assert size(ctypes.byref(sh), ctypes.byref(good), B) == 0
        for bad in BAD_PARAMS:
            assert size(ctypes.byref(sh), ctypes.byref(_params(**bad)), 2) == 0, bad
        assert size(ctypes.byref(sh), ctypes.byref(_params(K=256, sigma_min=0.0, sigma_max=INF)), 2) > 0   # the edges
        assert size(ctypes.byref(sh), ctypes.byref(_params(K=1, sigma_min=0.3, sigma_max=0.3)), 2) > 0
    sh = _lib.MlpShape(17, 6, 512, 3, 1)
    assert size(None, ctypes.byref(_params()), 2) == 0 and size(ctypes.byref(sh), None, 2) == 0
    assert size(ctypes.byref(_lib.MlpShape(0, 6, 512, 3, 1)), ctypes.byref(_params()), 2) == 0


def _dummy():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)   # non-NULL: the checks fire before anything is read or launched


def test_plan_argument_checks_return_the_stated_codes_without_a_device():
    from mbrl_amd import _lib
    lib = _lib.load()
    sh = _lib.MlpShape(17, 6, 512, 3, 1)
    p = _params()
    keep, ptr = _dummy()
    big = 1 << 40
    for B in (0, 3):     # 0: the single plan
        need = lib.mbrl_mppi_elite_workspace_bytes(ctypes.byref(sh), ctypes.byref(p), max(B, 1))

        def call(shape=ctypes.byref(sh), packed=ptr, s0=ptr, params=ctypes.byref(p), actions=ptr, states=ptr, ws=ptr,
                 nbytes=need, B=B):
            if B == 0:
                return lib.mbrl_mppi_plan_elite(shape, packed, None, None, s0, params, None, None, ptr, ptr, actions,
                                                states, None, None, None, None, None, None, ws, nbytes, None)
            return lib.mbrl_mppi_plan_elite_batch(shape, packed, None, None, s0, B, params, None, None, None, ptr, ptr,
                                                  actions, states, None, None, None, None, None, ws, nbytes, None)
        bad = (dict(packed=None), dict(s0=None), dict(params=None), dict(actions=None), dict(states=None), dict(ws=None))
        bad += tuple(dict(params=ctypes.byref(_params(**b))) for b in BAD_PARAMS)
        for kw in bad:
            assert call(**kw) == _lib.MBRL_EINVAL, (B, kw)
            assert lib.mbrl_last_error(), kw
        assert call(shape=ctypes.byref(_lib.MlpShape(0, 6, 512, 3, 1))) == _lib.MBRL_EUNSUPPORTED
        small = _lib.MBRL_EWORKSPACE if B else _lib.MBRL_EINVAL          # as the siblings
        assert call(nbytes=0) == small and b"workspace" in lib.mbrl_last_error()
        if B:
            assert call(nbytes=need - 1) == small
            assert call(B=-2) == _lib.MBRL_EINVAL
            assert call(B=65536, nbytes=big) == _lib.MBRL_EUNSUPPORTED and b"65535" in lib.mbrl_last_error()
        assert call(params=ctypes.byref(_params(N=32769)), nbytes=big) == _lib.MBRL_EUNSUPPORTED
        assert b"32768" in lib.mbrl_last_error()


def test_update_argument_checks_return_the_stated_codes_without_a_device():
    from mbrl_amd import _lib
    lib = _lib.load()
    keep, ptr = _dummy()
    keep2, ptr2 = _dummy()
    sp = _lib.Sampler(1, 0, 0, ptr, ptr, -1.0, 1.0)
    big = 1 << 40
    for B in (0, 2):     # 0: the single update
        def call(costs=ptr, E=1, N=8, K=3, actions=ptr, sampler=ctypes.byref(sp), H=2, a=3, lam=1.0, smin=0.0, smax=INF,
                 mu_out=ptr, sg_out=ptr, elites=ptr, nxt=None, off=0, cnt=0, ws=ptr, nbytes=big, B=B):
            if B == 0:
                return lib.mbrl_mppi_update_elite(costs, E, N, K, actions, sampler, H, a, lam, 0.0, 1, smin, smax, mu_out,
                                                  sg_out, elites, None, None, None, nxt, off, cnt, ws, nbytes, None)
            return lib.mbrl_mppi_update_elite_batch(costs, E, N, K, B, actions, sampler, H, a, lam, 0.0, 1, smin, smax,
                                                    mu_out, sg_out, elites, None, None, None, nxt, ws, nbytes, None)
        bad = [dict(costs=None), dict(actions=None), dict(sampler=None), dict(mu_out=None), dict(sg_out=None),
               dict(ws=None), dict(N=0), dict(E=0), dict(H=0), dict(a=0), dict(lam=0.0), dict(lam=-2.0), dict(lam=NAN),
               dict(lam=INF), dict(nxt=ptr), dict(K=0), dict(K=-1), dict(K=9), dict(smin=-1e-3), dict(smin=NAN),
               dict(smax=NAN), dict(smin=0.4, smax=0.3)]
        if B == 0:
            bad += [dict(nxt=ptr2, off=0, cnt=0), dict(nxt=ptr2, off=-1, cnt=4), dict(nxt=ptr2, off=5, cnt=4)]
        else:
            bad += [dict(B=-1)]
        for kw in bad:
            assert call(**kw) == _lib.MBRL_EINVAL, (B, kw)
            assert lib.mbrl_last_error(), kw
        nosp = _lib.Sampler(1, 0, 0, None, ptr, -1.0, 1.0)
        assert call(sampler=ctypes.byref(nosp)) == _lib.MBRL_EINVAL
        assert call(N=32769) == _lib.MBRL_EUNSUPPORTED and b"32768" in lib.mbrl_last_error()
        assert call(a=65) == _lib.MBRL_EUNSUPPORTED
        nb = max(B, 1)
        need = lib.mbrl_select_workspace_bytes(8 * nb)
        assert call(nbytes=need - 1) == _lib.MBRL_EWORKSPACE and b"workspace" in lib.mbrl_last_error()
        assert call(elites=None, nbytes=need) == _lib.MBRL_EWORKSPACE       # the list then lives behind the keys
        if B:
            assert call(B=65536) == _lib.MBRL_EUNSUPPORTED and b"65535" in lib.mbrl_last_error()
            assert call(B=65535, N=32768, K=5, nxt=ptr2) == _lib.MBRL_EUNSUPPORTED and b"B*N" in lib.mbrl_last_error()
    assert lib.mbrl_mppi_update_elite_batch(ptr, 1, 8, 3, 0, ptr, ctypes.byref(sp), 2, 3, 1.0, 0.0, 1, 0.0, INF, ptr, ptr,
                                            ptr, None, None, None, None, ptr, big, None) == _lib.MBRL_EINVAL


def test_kwargs_are_validated_on_the_host_before_looking_for_a_device():
    from mbrl_amd import MPPIPlanner, mppi_plan_batch
    from mbrl_amd.planners import BatchedMPPIPlanner
    assert MPPIPlanner.elite_defaults == dict(num_elites=None, min_std=0.0, max_std=None, warm_std=None)
    assert not set(MPPIPlanner.elite_defaults) & set(MPPIPlanner.defaults)
    s0 = torch.zeros(2, 5)
    prev = np.zeros((4, 2), F32)
    single = lambda **kw: MPPIPlanner.plan_detailed(s0[0], None, None, None, 4, kw.pop("init", None), **kw)  # noqa: E731
    batch = lambda **kw: mppi_plan_batch(s0, None, None, None, 4, kw.pop("inits", None), **kw)               # noqa: E731
    served = lambda **kw: BatchedMPPIPlanner.plan_batch(s0, None, None, None, 4, kw.pop("inits", None), **kw)  # noqa: E731
    for entry in (single, batch, served):
        for bad, match in ((dict(num_elites=0), "num_elites"), (dict(num_elites=1001), "num_elites"),
                           (dict(num_elites=17, num_candidates=16), "num_elites"), (dict(num_elites=2.5), "num_elites"),
                           (dict(num_elites=True), "num_elites"), (dict(min_std=-0.1), "min_std"),
                           (dict(min_std=NAN), "min_std"), (dict(min_std=INF), "min_std"),
                           (dict(max_std=NAN), "max_std"), (dict(min_std=0.5, max_std=0.4), "max_std"),
                           (dict(warm_std=0.0), "warm_std"), (dict(warm_std=NAN), "warm_std"),
                           (dict(warm_std=-1.0), "warm_std")):
            with pytest.raises(ValueError, match=match):
                entry(**bad)
        with pytest.raises(NotImplementedError, match="distributed"):
            entry(num_elites=10, distributed=True)
        with pytest.raises(NotImplementedError, match="noise_beta"):
            entry(num_elites=10, noise_beta=1.0)
    # warm_std="keep" needs the previous sigma, finite and > 0 and of the warm start's shape
    init = (None, prev)
    with pytest.raises(ValueError, match="prev_sigma"):
        single(init=init, num_elites=10, warm_std="keep")
    with pytest.raises(ValueError, match="finite and > 0"):
        single(init=init, num_elites=10, warm_std="keep", prev_sigma=np.zeros((4, 2), F32))
    with pytest.raises(ValueError, match="finite and > 0"):
        single(init=init, num_elites=10, warm_std="keep", prev_sigma=np.full((4, 2), NAN, F32))
    with pytest.raises(ValueError, match="rows"):
        single(init=init, num_elites=10, warm_std="keep", prev_sigma=np.ones((4, 3), F32))
    for entry in (batch, served):
        with pytest.raises(ValueError, match="prev_sigma"):
            entry(inits=[init, None], num_elites=10, warm_std="keep")
        with pytest.raises(ValueError, match="entries for 2"):
            entry(inits=[init, None], num_elites=10, warm_std="keep", prev_sigmas=[np.ones((4, 2), F32)])
        with pytest.raises(ValueError, match="finite and > 0"):
            entry(inits=[init, None], num_elites=10, warm_std="keep", prev_sigmas=[-np.ones((4, 2), F32), None])
        with pytest.raises(ValueError, match="prev_sigmas"):
            entry(inits=[init, None], num_elites=10, warm_std="keep", prev_sigma=np.ones((4, 2), F32))


def test_elite_settings_resolve_as_documented():
    from mbrl_amd import MPPIPlanner
    es = MPPIPlanner._elite_settings
    assert es({}, 100) is None and es(dict(num_elites=None, min_std=0.0, max_std=None), 100) is None
    assert es(dict(num_elites=7), 100) == dict(K=7, min_std=0.0, max_std=INF, warm_std=None)
    assert es(dict(min_std=0.1), 100) == dict(K=100, min_std=0.1, max_std=INF, warm_std=None)
    assert es(dict(max_std=2), 50)["K"] == 50 and es(dict(warm_std="keep"), 50)["warm_std"] == "keep"
    assert es(dict(num_elites=100, max_std=INF), 100)["K"] == 100


# ------------------------------------------------------------------------------------------------
# the restatement's own properties
# ------------------------------------------------------------------------------------------------
def _inputs(N, a=3, H=2, E=2, seed=0):
    rng = np.random.default_rng(seed)
    c = (100.0 + 3.0 * rng.standard_normal((E, N))).astype(F32)
    A = np.clip(rng.normal(0.1, 0.6, (H, N, a)), -1, 1).astype(F32)
    mu, sg = rng.uniform(-0.3, 0.3, (H, a)).astype(F32), rng.uniform(0.05, 0.6, (H, a)).astype(F32)
    return c, A, mu, sg


@pytest.mark.parametrize("N", [1, 31, 33, 100, 1025])
@pytest.mark.parametrize("upd", [False, True])
def test_all_candidates_elite_is_the_classic_restatement_bit_for_bit(N, upd):
    c, A, mu, sg = _inputs(N, seed=N)
    c[0, N // 2] = np.nan                       # one invalid candidate on either side
    got = eref.update_f32(c, A, mu, sg, 1.0, 0.1, upd, N)
    want = mref.update_f32(c, A, mu, sg, 1.0, 0.1, upd)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    u, v = eref.update(c, A, mu, sg, 1.0, 0.1, upd, N), mref.update(c, A, mu, sg, 1.0, 0.1, upd)
    assert np.array_equal(u["weights"], v["weights"]) and np.array_equal(u["mu"], v["mu"])
    assert np.array_equal(u["sigma"], v["sigma"])


@pytest.mark.parametrize("N", [1, 33, 1000])
def test_one_elite_without_smoothing_returns_the_best_row(N):
    c, A, mu, sg = _inputs(N, seed=7 * N)
    best = int(np.argmin(mref.returns_of(c)))
    m, s = eref.update_f32(c, A, mu, sg, 0.7, 0.0, False, 1)
    assert np.array_equal(m, A[:, best]) and s.tobytes() == sg.tobytes()
    u = eref.update(c, A, mu, sg, 0.7, 0.0, True, 1)
    assert np.array_equal(u["elites"], [best]) and u["eta"] == 1.0 and np.count_nonzero(u["weights"]) == 1
    assert np.array_equal(u["mu"], A[:, best].astype(np.float64)) and not u["var"].any()


def test_ties_invalid_rows_and_the_clamp():
    c, A, mu, sg = _inputs(40, E=1)
    c[0, [5, 9, 30]] = c[0].min() - 1.0              # a three-way tie for the best: K = 2 takes the lower indices
    u = eref.update(c, A, mu, sg, 1.0, 0.0, True, 2)
    assert np.array_equal(u["elites"], [5, 9]) and u["weights"][30] == 0 and u["weights"][5] == u["weights"][9] == 1
    c[0, :] = np.nan
    c[0, [3, 4]] = [2.0, 1.0]                        # fewer than K finite returns: the NaN rows stay invalid
    u = eref.update(c, A, mu, sg, 1.0, 0.0, True, 5)
    assert len(u["elites"]) == 5 and np.count_nonzero(u["weights"]) == 2 and u["beta"] == 1.0
    c[0, 7] = -np.inf                                # -inf sorts first and is invalid: K = 1 leaves nothing valid
    u = eref.update(c, A, mu, sg, 1.0, 0.0, True, 1)
    assert u["unchanged"] and np.array_equal(u["elites"], [7]) and np.isnan(u["beta"])
    c, A, mu, sg = _inputs(64)
    free = eref.update_f32(c, A, mu, sg, 1.0, 0.1, True, 8)[1]
    lo, hi = float(np.median(free)), float(np.max(free))
    for smin, smax in ((lo, INF), (0.0, lo), (lo, lo), (0.0, hi), (hi, INF)):
        m, s = eref.update_f32(c, A, mu, sg, 1.0, 0.1, True, 8, smin, smax)
        assert s.tobytes() == np.clip(free, F32(smin), F32(smax)).tobytes()
    assert eref.update_f32(c, A, mu, sg, 1.0, 0.1, False, 8, 10.0, 20.0)[1].tobytes() == sg.tobytes()  # classic: unclamped


@pytest.mark.parametrize("case", eref.PLAN_CASES, ids=lambda c: "cfg%d-N%d-K%d" % (c[0], c[1], c[4]))
def test_plan_fixtures_keep_the_elite_boundary_clear(case):
    """A condition on the fixture, not a measurement: at every iteration of the reference plan the K-th and the
    (K+1)-th return are at least GAP_MIN apart (relative), so a device plan whose returns agree to 1e-5 selects
    the same set. The seeds were picked on the CPU (find_seed)."""
    ref = eref.case_plan(case)
    assert len(ref["gaps"]) == case[3] and min(ref["gaps"]) >= eref.GAP_MIN, ref["gaps"]
    assert all(len(e) == case[4] and np.all(np.diff(e) > 0) for e in ref["elites"])


def test_find_seed_reproduces_a_fixture_seed():
    case = eref.PLAN_CASES[0]
    assert eref.find_seed(case) == case[-1]
