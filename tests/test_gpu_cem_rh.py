"""GPU: the receding-horizon CEM plan (mbrl_cem_plan_rh: csrc/cem_rh.hip and its loop in plan.hip) and
CEMPlanner's warm_start / keep_elites / carry kwargs, against the NumPy restatement
(tests/cem_rh_reference.py).

Bars, at every iteration of every fixture case: costs within 1e-5 relative of the restatement's; the elite
and the best index sets identical (tests/test_cem_rh_host.py asserts that the fixtures' K-th and Kc-th
return gaps exceed 1e-4, so costs within the bar cannot reorder them); mu, sigma, the kept rows and the
carry bit for bit. keep == 0 without rows is mbrl_cem_plan bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import cem_rh_reference as rh
from oracle import cem as ocem

from test_gpu_parity import build, device_problem

pytestmark = pytest.mark.gpu
F32 = np.float32
LO, HI = -1.0, 1.0
RTOL = 1e-5
DEV = "cuda:0"


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).tobytes()


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(DEV)


def _params(p, N, H, K, I, keep):
    from mbrl_amd import _lib
    cem = _lib.CemParams(N, H, K, I, 0.1, LO, HI, 0.0, 0.5, 0, p["rng_seed"] & 0xFFFFFFFFFFFFFFFF)
    return _lib.CemRhParams(cem, keep, 0)


def c_plan_rh(prob, p, N, H, K, I, keep=0, init_mu_rows=None, init_sigma_rows=None, carry_in=None, record=True,
              expect=0, ws_bytes=None, make_ws=None, alloc=None):
    """mbrl_cem_plan_rh through ctypes. Returns the outputs and records as device tensors; with `expect`
    nonzero, asserts that return code instead (the argument checks). make_ws(nbytes) -> the uint8 workspace and
    alloc(*shape, dt=) -> an output tensor replace the private allocations (tests/workspace_cases.py)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    md = prob.mdesc
    a, s, E = md["a"], md["s"], md["E"]
    params = _params(p, N, H, K, I, keep)
    need = lib.mbrl_cem_rh_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params))
    dev = torch.device(DEV)
    ws = make_ws(need) if make_ws else torch.empty(max(need if ws_bytes is None else ws_bytes, 256), dtype=torch.uint8,
                                                   device=dev)
    e = alloc or (lambda *sh, dt=torch.float32: torch.full(sh, -7, dtype=dt, device=dev))  # noqa: E731
    out = dict(mu=e(H, a), sigma=e(H, a), actions=e(H, a), states=e(H, s))
    Kc = max(keep, 0)
    if Kc:
        out.update(carry=e(Kc, H, a), carry_returns=e(Kc))
    if record:
        out.update(costs=e(I, E, N), returns=e(I, N), elites=e(I, K, dt=torch.int64))
        if Kc:
            out.update(kept_hist=e(I + 1, Kc, H, a))
    g = lambda k: _lib.ptr(out.get(k))  # noqa: E731
    s0 = _dev(p["s0"])
    ins = [_dev(init_mu_rows), _dev(init_sigma_rows), _dev(carry_in)]
    rc = lib.mbrl_cem_plan_rh(*prob.refs, _lib.ptr(s0), ctypes.byref(params), *[_lib.ptr(x) for x in ins], g("mu"),
                              g("sigma"), g("actions"), g("states"), g("carry"), g("carry_returns"), g("costs"),
                              g("returns"), g("elites"), g("kept_hist"), None, _lib.ptr(ws),
                              ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, lib.mbrl_last_error())
        for k, v in out.items():          # refused before any launch: nothing was written
            assert bool((v == -7).all()), k
        return None
    _lib.check(rc, "mbrl_cem_plan_rh")
    return out


def _rel(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)))


def _check_against_restatement(got, ref, I, K, Kc, tag):
    """The issue's asserts for one recorded plan, iteration by iteration; prints the figures first."""
    kept = got["kept_hist"].cpu().numpy() if Kc else None
    for it in range(I):
        c = got["costs"][it].cpu().numpy()
        err = _rel(c, ref["costs"][it])
        print(f"cem-rh {tag} it={it}: cost rel err {err:.3g}")
        assert err < RTOL, (tag, it, err)
        assert np.array_equal(got["elites"][it].cpu().numpy(), ref["elites"][it]), (tag, it)
        if Kc:
            assert _bits(kept[it]) == _bits(ref["kept"][it]), (tag, it)
            # the best set, from the GPU's own returns (ascending index: the kept rows' order)
            r = got["returns"][it].cpu().numpy()
            assert np.array_equal(ocem.select_elites(r, Kc), ref["best"][it]), (tag, it)
    assert _bits(got["mu"]) == _bits(ref["mu_out"]) and _bits(got["sigma"]) == _bits(ref["sigma_out"]), tag
    assert _bits(got["actions"]) == _bits(ref["final_actions"]), tag
    assert _rel(got["states"].cpu().numpy(), ref["final_states"]) < RTOL, tag
    if Kc:
        assert _bits(kept[I]) == _bits(ref["kept"][I]) and _bits(got["carry"]) == _bits(ref["carry"]), tag
        # the carry's returns are the GPU's own returns of the best rows
        r = got["returns"][I - 1].cpu().numpy()
        assert _bits(got["carry_returns"]) == _bits(r[ref["best"][I - 1]]), tag


@pytest.mark.parametrize("case", rh.CASES, ids=rh.case_id)
def test_plan_against_the_restatement(case):
    W, L, a, N, E, Kc, inputs, _ = case
    H, K, I = rh.SMALL["H"], rh.SMALL["K"], rh.SMALL["I"]
    p, kw = rh.make_case(case)
    ref = rh.plan(p, N, H, K, I, **kw)
    got = c_plan_rh(device_problem(p), p, N, H, K, I, **kw)
    _check_against_restatement(got, ref, I, K, Kc, rh.case_id(case))


def test_keep_zero_without_rows_is_the_plain_plan_bit_for_bit():
    """The cheetah golden problem cut to N = 512, H = 6: the same launches, so the same bits, records too."""
    from mbrl_amd import CEMPlanner
    N, H, K, I = 512, 6, 51, 3
    p = ocem.synth_problem(3, N=N, H=H)
    _, model_fn, cost_fn, sample_action = build(p)
    plain = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H, num_candidates=N,
                                     num_elites=K, num_iterations=I, seed=p["rng_seed"], record=True,
                                     return_device=True)
    got = c_plan_rh(device_problem(p), p, N, H, K, I, keep=0)
    for k in ("mu", "sigma", "actions", "states", "costs", "returns", "elites"):
        assert torch.equal(plain[k], got[k]), k
    # ... and where the plan runs select / refit / draw as separate launches (the same bits, as for the plain plan)
    from mbrl_amd import _lib
    with _lib.option("unfused_update", 1):
        got_u = c_plan_rh(device_problem(p), p, N, H, K, I, keep=0)
    for k in ("mu", "sigma", "actions", "states", "costs", "returns", "elites"):
        assert torch.equal(plain[k], got_u[k]), k


def test_a_kept_optimum_survives_the_plan():
    """carry_in's row 0 is the restatement's best row after 5 cold iterations: candidate 0 is among the
    elites of iteration 0 and the row comes back in carry_out bit for bit (nothing the plan draws in three
    iterations from the cold distribution beats it)."""
    N, H, K, I, Kc = 64, 3, 8, 3, 3
    p = ocem.synth_problem(2, seed=7110, W=64, L=1, a=5, N=N, H=H)
    cold = rh.plan(p, N, H, K, 5, keep=1, final=False)
    opt = cold["carry"][0]
    rng = np.random.default_rng(1)
    carry_in = np.concatenate([opt[None], rng.uniform(-1, 1, (Kc - 1, H, 5)).astype(F32)], 0)
    ref = rh.plan(p, N, H, K, I, keep=Kc, carry_in=carry_in)
    assert rh.case_gaps(ref, K, Kc) > rh.GAP_MIN
    got = c_plan_rh(device_problem(p), p, N, H, K, I, keep=Kc, carry_in=carry_in)
    _check_against_restatement(got, ref, I, K, Kc, "kept optimum")
    assert 0 in got["elites"][0].cpu().numpy()
    carry = got["carry"].cpu().numpy()
    assert any(_bits(row) == _bits(opt) for row in carry)
    assert float(got["carry_returns"].min()) <= float(got["returns"][0][0])


def test_a_nan_kept_row_sorts_last_and_is_dropped():
    N, H, K, I, Kc = 64, 3, 8, 3, 3
    p = ocem.synth_problem(2, seed=7101, W=64, L=1, a=5, N=N, H=H)
    rng = np.random.default_rng(2)
    carry_in = rng.uniform(-1, 1, (Kc, H, 5)).astype(F32)
    carry_in[1, 2, 3] = np.nan
    ref = rh.plan(p, N, H, K, I, keep=Kc, carry_in=carry_in)
    assert np.isnan(ref["returns"][0][1]) and np.isfinite(np.delete(ref["returns"][0], 1)).all()
    got = c_plan_rh(device_problem(p), p, N, H, K, I, keep=Kc, carry_in=carry_in)
    r0 = got["returns"][0].cpu().numpy()
    assert np.isnan(r0[1]) and np.isfinite(np.delete(r0, 1)).all()
    assert 1 not in got["elites"][0].cpu().numpy()
    assert np.array_equal(ocem.select_elites(r0, Kc), ref["best"][0]) and 1 not in ref["best"][0]
    kept = got["kept_hist"].cpu().numpy()
    assert _bits(kept[0]) == _bits(carry_in)                      # (row 0 of the record: carry_in as given)
    assert np.isfinite(kept[1:]).all() and np.isfinite(got["carry"].cpu().numpy()).all()
    assert np.isfinite(got["mu"].cpu().numpy()).all() and np.isfinite(got["sigma"].cpu().numpy()).all()
    assert _bits(got["mu"]) == _bits(ref["mu_out"]) and _bits(got["carry"]) == _bits(ref["carry"])


def _planner_problem(N=64, H=3, a=5):
    p = ocem.synth_problem(2, seed=7102, W=64, L=1, a=a, N=N, H=H)
    _, model_fn, cost_fn, sample_action = build(p)
    return p, model_fn, cost_fn, sample_action


def test_planner_kwargs_equal_the_c_level_plan():
    from mbrl_amd import CEMPlanner, cem_shift_carry
    N, H, K, I, Kc = 64, 3, 8, 3, 3
    p, model_fn, cost_fn, sample_action = _planner_problem(N, H)
    rng = np.random.default_rng(3)
    prev_actions = rng.uniform(-1.3, 1.3, (H, 5)).astype(F32)
    prev_sigma = rng.uniform(0.1, 0.6, (H, 5)).astype(F32)
    carry = cem_shift_carry(rng.uniform(-1.2, 1.2, (Kc, H, 5)).astype(F32), 1)
    kw = dict(num_candidates=N, num_elites=K, num_iterations=I, seed=p["rng_seed"], record=True, return_device=True)
    res = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H,
                                   initial_trajectory=(None, torch.from_numpy(prev_actions)), warm_start=True,
                                   keep_elites=Kc, carry=torch.from_numpy(carry), warm_std="keep",
                                   prev_sigma=prev_sigma, **kw)
    from mbrl_amd.planners import mppi_warm_start_rows
    rows = mppi_warm_start_rows(prev_actions, H, 1, LO, HI)
    sig = np.concatenate([prev_sigma[1:], prev_sigma[-1:]], 0)
    got = c_plan_rh(device_problem(p), p, N, H, K, I, keep=Kc, init_mu_rows=rows, init_sigma_rows=sig, carry_in=carry)
    for k in ("mu", "sigma", "actions", "states", "costs", "returns", "elites", "carry", "carry_returns", "kept_hist"):
        assert torch.equal(res[k], got[k]), k
    assert res["carry"].shape == (Kc, H, 5) and res["kept_hist"].shape == (I + 1, Kc, H, 5)
    # without record: the carry, no history; a fraction of num_elites resolves to the same count
    kw.update(record=False)
    res2 = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H,
                                    initial_trajectory=(None, torch.from_numpy(prev_actions)), warm_start=True,
                                    keep_elites=0.4, carry=torch.from_numpy(carry), warm_std="keep",
                                    prev_sigma=prev_sigma, **kw)
    assert "kept_hist" not in res2 and torch.equal(res2["carry"], res["carry"]) and torch.equal(res2["mu"], res["mu"])


def test_planner_defaults_are_the_plain_plan_bit_for_bit():
    from mbrl_amd import CEMPlanner
    N, H = 64, 3
    p, model_fn, cost_fn, sample_action = _planner_problem(N, H)
    s0 = torch.from_numpy(p["s0"])
    kw = dict(num_candidates=N, num_iterations=3, seed=p["rng_seed"])
    traj = (None, torch.full((H, 5), 0.3))
    states, actions = CEMPlanner.plan(s0, model_fn, cost_fn, sample_action, H, initial_trajectory=traj, **kw)
    s2, a2 = CEMPlanner.plan(s0, model_fn, cost_fn, sample_action, H, initial_trajectory=traj, warm_start=False, shift=1,
                             warm_std=None, keep_elites=0, carry=None, **kw)
    assert torch.equal(states, s2) and torch.equal(actions, a2)
    d = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, initial_trajectory=traj, warm_start=False,
                                 keep_elites=0, **kw)
    assert "carry" not in d and torch.equal(d["actions"], actions)
    # switched on, the previous plan matters
    s3, a3 = CEMPlanner.plan(s0, model_fn, cost_fn, sample_action, H, initial_trajectory=traj, warm_start=True, **kw)
    assert not torch.equal(a3, actions)


def test_mpc_policy_warm_starts_from_the_shifted_previous_plan():
    from mbrl_amd import CEMPlanner, MPCPolicy
    H = 6
    p = ocem.synth_problem(3, N=256, H=H)
    _, model_fn, cost_fn, sample_action = build(p)
    seen = []

    class Recording(CEMPlanner):
        @staticmethod
        def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
            res = CEMPlanner.plan_detailed(initial_state, model, cost, sample_action, horizon, initial_trajectory,
                                           record=True, **kwargs)
            seen.append(res)
            return res["states"], res["actions"]

    pol = MPCPolicy(model_fn, cost_fn, Recording, sample_action, H, num_candidates=256, num_iterations=2, seed=5,
                    warm_start=True, keep_elites=4)
    obs = torch.from_numpy(p["s0"])
    a0 = pol.get_action({"timestep": 0, "observation": obs})
    a1 = pol.get_action({"timestep": 1, "observation": seen[0]["states"][0]})
    first = seen[0]["actions"].numpy()
    assert np.array_equal(a0.numpy(), first[0]) and a1.shape == (6,)
    want = np.concatenate([first[1:], first[-1:]], 0)
    # the second plan's initial mean is the first plan's shifted, clipped actions (CEM records no mu_hist:
    # record=True returns the rows the plan started from as init_mu) ...
    assert "init_mu" not in seen[0] and np.array_equal(seen[1]["init_mu"].cpu().numpy(), want)
    # ... and the plan used them: iteration 0's proposals are the plain draw around them
    from oracle.philox import cem_actions
    A0 = cem_actions(want, np.full((H, 6), 0.5, F32), LO, HI, 5, 0, np.arange(256))
    ref_c = ocem.rollout(p["model"], p["norm"], p["cost"], seen[0]["states"][0].numpy(), A0)
    got_c = seen[1]["costs"][0].cpu().numpy()
    assert _rel(got_c, ref_c) < RTOL
    cold_A0 = cem_actions(np.zeros((H, 6), F32), np.full((H, 6), 0.5, F32), LO, HI, 5, 0, np.arange(256))
    cold_c = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], cold_A0)
    assert _rel(seen[0]["costs"][0].cpu().numpy(), cold_c) < RTOL     # the episode's first plan starts cold
    assert seen[1]["carry"].shape == (4, H, 6)
    pol.get_action({"timestep": 0, "observation": obs})                 # a new episode forgets the plan
    assert torch.equal(seen[2]["costs"][0], seen[0]["costs"][0])


def test_generic_path_refuses_the_new_kwargs():
    from mbrl_amd import CEMPlanner, fused
    p, model_fn, cost_fn, sample_action = _planner_problem()
    wrapped = lambda s, a: model_fn(s, a)  # noqa: E731
    assert fused.describe_model(wrapped) is None
    s0 = torch.from_numpy(p["s0"])
    with pytest.raises(NotImplementedError, match="keep_elites"):
        CEMPlanner.plan(s0, wrapped, cost_fn, sample_action, 3, num_candidates=64, seed=1, keep_elites=2)
    with pytest.raises(NotImplementedError, match="warm_start"):
        CEMPlanner.plan(s0, wrapped, cost_fn, sample_action, 3, num_candidates=64, seed=1, warm_start=True,
                        initial_trajectory=(None, torch.zeros(3, 5)))


@pytest.mark.parametrize("what,code", [("keep>K", "EINVAL"), ("carry_without_keep", "EINVAL"),
                                       ("small_workspace", "EINVAL"), ("N=32769", "EUNSUPPORTED"),
                                       ("keep<0", "EINVAL"), ("null_outputs", "EINVAL")])
def test_argument_checks_return_before_any_launch(what, code):
    from mbrl_amd import _lib
    lib = _lib.load()
    N, H, K, I = 64, 3, 8, 2
    p = ocem.synth_problem(2, seed=7103, W=64, L=1, a=5, N=N, H=H)
    prob = device_problem(p)
    expect = getattr(_lib, "MBRL_" + code)
    if what == "keep>K":
        assert lib.mbrl_cem_rh_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(_params(p, N, H, K, I, K + 1))) == 0
        c_plan_rh(prob, p, N, H, K, I, keep=K + 1, expect=expect, ws_bytes=1 << 20)
    elif what == "keep<0":
        c_plan_rh(prob, p, N, H, K, I, keep=-1, expect=expect, ws_bytes=1 << 20)
    elif what == "carry_without_keep":
        c_plan_rh(prob, p, N, H, K, I, keep=0, carry_in=np.zeros((1, H, 5), F32), expect=expect)
    elif what == "small_workspace":
        need = lib.mbrl_cem_rh_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(_params(p, N, H, K, I, 3)))
        assert need > lib.mbrl_cem_rh_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(_params(p, N, H, K, I, 0)))
        c_plan_rh(prob, p, N, H, K, I, keep=3, expect=expect, ws_bytes=need - 256)
    elif what == "N=32769":
        c_plan_rh(prob, p, 32769, 1, K, 1, keep=3, expect=expect, record=False)
    else:
        dev = torch.device(DEV)
        params = _params(p, N, H, K, I, 0)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        rc = lib.mbrl_cem_plan_rh(*prob.refs, _lib.ptr(_dev(p["s0"])), ctypes.byref(params), *([None] * 14),
                                  _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
        assert rc == expect
    assert b"cem_plan_rh" in lib.mbrl_last_error() or b"CEM params" in lib.mbrl_last_error()
