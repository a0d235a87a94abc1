"""CPU: batched MPPI on the host -- the three new C entries (names, the sizing query, the argument checks
that fire before any launch) and mppi_plan_batch's / BatchedMPPIPlanner's host side. No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mbrl_cem.h")
F32 = np.float32
NEW = ("mbrl_mppi_update_batch", "mbrl_mppi_batch_workspace_bytes", "mbrl_mppi_plan_batch")


def _params(**kw):
    from mbrl_amd import _lib
    d = dict(N=256, H=4, iterations=2, update_sigma=0, temperature=1.0, alpha=0.0, lo=-1.0, hi=1.0, init_mu=0.0,
             init_sigma=0.5, seed=7)
    d.update(kw)
    return _lib.MppiParams(*[d[f] for f, _ in _lib.MppiParams._fields_])


def test_header_exported_list_and_library_agree_on_the_new_names():
    from mbrl_amd import _lib
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name) and name + "(" in text, name
        assert getattr(lib, name).argtypes is not None
    assert lib.mbrl_abi_version() == 13          # additive within v13


BAD_PARAMS = [dict(N=0), dict(H=0), dict(iterations=0), dict(temperature=0.0), dict(temperature=float("nan")),
              dict(temperature=float("inf"))]


def test_sizing_query():
    from mbrl_amd import _lib
    lib = _lib.load()
    size = lib.mbrl_mppi_batch_workspace_bytes
    good = _params()
    for sh in (_lib.MlpShape(17, 6, 512, 3, 1), _lib.MlpShape(5, 1, 256, 2, 5), _lib.MlpShape(24, 6, 512, 3, 1, 1)):
        need = [size(ctypes.byref(sh), ctypes.byref(good), B) for B in (1, 2, 3, 8, 64)]
        # monotone in B (flat while the single plan's layout, which the answer never goes below, is the larger)
        assert all(x > 0 for x in need) and all(x <= y for x, y in zip(need, need[1:])) and need[-1] > need[0], need
        assert need[0] >= lib.mbrl_mppi_workspace_bytes(ctypes.byref(sh), ctypes.byref(good))
        # the B N proposals ([H][B N][a], twice where the update draws) and the per-candidate start states fit
        assert need[4] > 64 * 256 * (2 * 4 * sh.action_dim + sh.state_dim) * 4
        for B in (0, -1):
            assert size(ctypes.byref(sh), ctypes.byref(good), B) == 0
        for bad in BAD_PARAMS:
            assert size(ctypes.byref(sh), ctypes.byref(_params(**bad)), 2) == 0, bad
    sh = _lib.MlpShape(17, 6, 512, 3, 1)
    assert size(None, ctypes.byref(good), 2) == 0 and size(ctypes.byref(sh), None, 2) == 0
    assert size(ctypes.byref(_lib.MlpShape(0, 6, 512, 3, 1)), ctypes.byref(good), 2) == 0


def test_plan_batch_argument_checks_return_the_stated_codes_without_a_device():
    from mbrl_amd import _lib
    lib = _lib.load()
    sh = _lib.MlpShape(17, 6, 512, 3, 1)
    p = _params()
    B = 3
    need = lib.mbrl_mppi_batch_workspace_bytes(ctypes.byref(sh), ctypes.byref(p), B)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)     # non-NULL dummies: the checks fire before anything is read or launched

    def call(shape=ctypes.byref(sh), packed=ptr, s0=ptr, B=B, params=ctypes.byref(p), actions=ptr, states=ptr, ws=ptr,
             nbytes=need):
        return lib.mbrl_mppi_plan_batch(shape, packed, None, None, s0, B, params, None, None, ptr, ptr, actions, states,
                                        None, None, None, None, ws, nbytes, None)
    for kw in (dict(packed=None), dict(s0=None), dict(params=None), dict(actions=None), dict(states=None),
               dict(ws=None), dict(B=0), dict(B=-2)) + tuple(dict(params=ctypes.byref(_params(**b))) for b in BAD_PARAMS):
        assert call(**kw) == _lib.MBRL_EINVAL, kw
        assert lib.mbrl_last_error(), kw
    assert call(shape=ctypes.byref(_lib.MlpShape(0, 6, 512, 3, 1))) == _lib.MBRL_EUNSUPPORTED
    assert call(nbytes=need - 1) == _lib.MBRL_EWORKSPACE and b"workspace" in lib.mbrl_last_error()
    assert call(nbytes=0) == _lib.MBRL_EWORKSPACE
    big = 1 << 40                               # (a size no check may trust: the limits come first)
    assert call(B=65536, nbytes=big) == _lib.MBRL_EUNSUPPORTED and b"65535" in lib.mbrl_last_error()
    assert call(params=ctypes.byref(_params(N=32769)), nbytes=big) == _lib.MBRL_EUNSUPPORTED
    assert b"32768" in lib.mbrl_last_error()
    assert call(B=65535, params=ctypes.byref(_params(N=32768)), nbytes=big) == _lib.MBRL_EUNSUPPORTED   # B N
    assert b"B*N" in lib.mbrl_last_error()


def test_update_batch_argument_checks_return_the_stated_codes_without_a_device():
    from mbrl_amd import _lib
    lib = _lib.load()
    buf, other = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    ptr, ptr2 = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(other, ctypes.c_void_p)
    sp = _lib.Sampler(1, 0, 0, ptr, ptr, -1.0, 1.0)

    def call(costs=ptr, E=1, N=8, B=2, actions=ptr, sampler=ctypes.byref(sp), H=2, a=3, lam=1.0, mu_out=ptr, sg_out=ptr,
             nxt=None):
        return lib.mbrl_mppi_update_batch(costs, E, N, B, actions, sampler, H, a, lam, 0.0, 0, mu_out, sg_out, None,
                                          None, None, nxt, None)
    bad = [dict(costs=None), dict(actions=None), dict(sampler=None), dict(mu_out=None), dict(sg_out=None), dict(N=0),
           dict(E=0), dict(H=0), dict(a=0), dict(lam=0.0), dict(lam=-2.0), dict(lam=float("nan")), dict(lam=float("inf")),
           dict(nxt=ptr), dict(B=0), dict(B=-1)]
    for kw in bad:
        assert call(**kw) == _lib.MBRL_EINVAL, kw
        assert lib.mbrl_last_error(), kw
    nosp = _lib.Sampler(1, 0, 0, None, ptr, -1.0, 1.0)
    assert call(sampler=ctypes.byref(nosp)) == _lib.MBRL_EINVAL
    assert call(N=32769) == _lib.MBRL_EUNSUPPORTED and b"32768" in lib.mbrl_last_error()
    assert call(a=65) == _lib.MBRL_EUNSUPPORTED
    assert call(B=65536) == _lib.MBRL_EUNSUPPORTED and b"65535" in lib.mbrl_last_error()
    assert call(B=65535, N=32768, nxt=ptr2) == _lib.MBRL_EUNSUPPORTED and b"B*N" in lib.mbrl_last_error()


def test_mppi_plan_batch_refuses_on_the_host_before_looking_for_a_device():
    from mbrl_amd import mppi_plan_batch
    from mbrl_amd.planners import BatchedMPPIPlanner
    s0 = torch.zeros(2, 5)
    prev = np.zeros((4, 2), F32)
    for entry in (mppi_plan_batch, BatchedMPPIPlanner.plan_batch):
        with pytest.raises(NotImplementedError, match="distributed"):
            entry(s0, None, None, None, 4, distributed=True)
        with pytest.raises(NotImplementedError, match="noise_beta"):
            entry(s0, None, None, None, 4, noise_beta=1.0)
        with pytest.raises(NotImplementedError, match="noise_mix"):
            entry(s0, None, None, None, 4, noise_mix=np.eye(4, dtype=F32))
        with pytest.raises(ValueError, match="entries for 2"):
            entry(s0, None, None, None, 4, [None])
        with pytest.raises(ValueError, match="entries for 2"):
            entry(s0, None, None, None, 4, [(None, prev)] * 3)
        with pytest.raises(ValueError, match="temperature"):
            entry(s0, None, None, None, 4, temperature=0.0)
        with pytest.raises(ValueError, match="no action row left"):      # the per-row shift, also on the host
            entry(s0, None, None, None, 4, [(None, prev[:1]), None])


def test_batched_planner_attributes_and_the_single_planner_still_refuses():
    from mbrl_amd import BatchedMPPIPlanner, MPPIPlanner
    assert issubclass(BatchedMPPIPlanner, MPPIPlanner) and BatchedMPPIPlanner.warm_starts is True
    assert BatchedMPPIPlanner.plan is MPPIPlanner.plan
    assert not getattr(BatchedMPPIPlanner, "plan_memo", False)       # the service hands it no memos
    assert BatchedMPPIPlanner.defaults is MPPIPlanner.defaults
    with pytest.raises(NotImplementedError):
        MPPIPlanner.plan_batch(None, None, None, None, 5)
