"""The rollout's whole shape envelope on the GPU: every case of tests/rollout_cases.py, whose coverage of the
fp32 instances, fallbacks and refusals tests/test_rollout_dispatch_model.py proves on the CPU.

Accepted cases go through fused.rollout (mbrl_rollout_cost) against oracle.cem.rollout at the suite's bars:
costs within test_gpu_parity.RTOL, states within rtol = atol = 1e-4. Cases with N >= 8192 must in addition
equal, bit for bit, the same candidates rolled out as shards of at most 2048 (the README's promise that costs
do not depend on the tile height), and are compared with the oracle on their first 64 candidates. Whole
CEM plans, an MPPI plan and the plain single-workgroup trajectory kernel (the shapes past both the register
and the cooperative kernel's budgets) run at T = 16 and wide-input shapes at the fuzz test's bars; the
single-trajectory kernels' own instance envelope -- every traj_reg_kernel and traj_coop_kernel instance,
both cooperative grids, the hop modes -- is tests/test_gpu_traj_envelope.py. Refused cases must return MBRL_EUNSUPPORTED with the message the dispatch model predicts,
launch nothing (sentinel-filled outputs untouched, a sampled call's actions_out included), and make the
Python planners raise.

This is what pins the LDS half of the dispatch model: a shape it calls refused is refused with the byte count
it computes, and a shape it calls accepted (some within 2 KiB of the 160 KiB line) runs and matches.

Tolerance at W = 1024. RTOL was set at dot products of length 512; the oracle itself is float32. For every
accepted case the oracle was evaluated in float64 (rollout_cases.rollout_f64, asserted on the CPU by
test_float32_oracle_is_within_a_tenth_of_the_bar_of_float64): with H in 1..3 the float32 oracle's worst
relative distance from float64 is 2.2e-7 (r2_t8_humanoid_L3; 1.7e-7 at W = 1024, t16_generic_L2), under
RTOL / 10 = 1e-6 everywhere, so a miss of RTOL on the GPU is the kernel's and not the bar's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.philox import cem_actions

import mppi_reference as mref
import rollout_cases as rc
import rollout_dispatch_model as rdm
from test_gpu_parity import DEV, RTOL, build, device_problem, rel_err

pytestmark = pytest.mark.gpu
SMALL = [c for c in rc.ACCEPTED if c.N <= 64]
LARGE = [c for c in rc.ACCEPTED if c.N >= rdm.R2_MIN_N]
SENTINEL = -12345.5
SAMPLE_OFFSET = 4096 + 5


@functools.lru_cache(maxsize=None)
def _problem(cid):
    c = rc.by_id(cid)
    return ocem.synth_problem(c.cid, N=c.N, H=c.H, **c.over)


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """(s0, actions, oracle costs [E, n], oracle states [E, H, n, s]) on the first n <= 64 candidates."""
    c, p = rc.by_id(cid), _problem(cid)
    a, n = p["cfg"]["a"], min(c.N, rc.ORACLE_ROWS)
    if c.mode == "sampled":
        mu, sg = _sampled_distribution(c.H, a)
        A = cem_actions(mu, sg, -1, 1, p["rng_seed"], 1, np.arange(SAMPLE_OFFSET, SAMPLE_OFFSET + c.N))
        s0 = p["s0"]
    else:
        s0, A = rc.given_inputs(c, p)
    s0n = s0[:n] if s0.ndim == 2 else s0
    costs, states = ocem.rollout(p["model"], p["norm"], p["cost"], s0n, np.ascontiguousarray(A[:, :n]), store_states=True)
    for x in (s0, A, costs, states):
        x.setflags(write=False)
    return s0, A, costs, states


def _sampled_distribution(H, a):
    rng = np.random.default_rng(H * 100 + a)
    return rng.uniform(-0.3, 0.3, (H, a)).astype(np.float32), rng.uniform(0.2, 0.6, (H, a)).astype(np.float32)


def _run(case, prob, s0, A, tile, lo=0, hi=None):
    """Costs [E, n] and states [E, H, n, s] of candidates [lo, hi) under MBRL_OPT_ROLLOUT_TILE = tile."""
    from mbrl_amd import _lib, fused
    hi = A.shape[1] if hi is None else hi
    p = _problem(case.id)
    E, s, n = p["cfg"]["E"], p["cfg"]["s"], hi - lo
    states = torch.full((E, case.H, n, s), SENTINEL, dtype=torch.float32, device=DEV)
    s0_d = torch.from_numpy(np.array(s0[lo:hi] if s0.ndim == 2 else s0)).to(DEV)   # a copy: the reference is read-only
    with _lib.option("rollout_tile", tile):
        costs = fused.rollout(prob, s0_d, n, case.H, actions=torch.from_numpy(np.array(A[:, lo:hi])).to(DEV),
                              s0_per_candidate=s0.ndim == 2, states_out=states)
    torch.cuda.synchronize()
    return costs, states


def _check_against_oracle(case, costs, states, ref_costs, ref_states):
    n = ref_costs.shape[1]
    err = rel_err(costs[:, :n], ref_costs)
    print(f"envelope {case.id}: {rc.run_outcome(case)} cost rel err {err:.3g}")
    assert err < RTOL, (case.id, err)
    assert np.allclose(states[:, :, :n].cpu().numpy(), ref_states, rtol=1e-4, atol=1e-4), case.id


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_accepted_shape_matches_the_oracle(case):
    from mbrl_amd import fused
    assert isinstance(rc.run_outcome(case), rdm.Instance)
    p = _problem(case.id)
    prob = device_problem(p)
    s0, A, ref_costs, ref_states = _reference(case.id)
    if case.mode != "sampled":
        costs, states = _run(case, prob, s0, A, rc.forced_tile(case))
    else:
        from mbrl_amd import _lib
        E, s, a = p["cfg"]["E"], p["cfg"]["s"], p["cfg"]["a"]
        mu, sg = _sampled_distribution(case.H, a)
        mu_d, sg_d = torch.from_numpy(mu).to(DEV), torch.from_numpy(sg).to(DEV)   # the sampler holds their addresses
        sp = fused.make_sampler(p["rng_seed"], 1, mu_d, sg_d, -1.0, 1.0)
        acts = torch.full((case.H, case.N, a), SENTINEL, dtype=torch.float32, device=DEV)
        states = torch.full((E, case.H, case.N, s), SENTINEL, dtype=torch.float32, device=DEV)
        with _lib.option("rollout_tile", rc.forced_tile(case)):
            costs = fused.rollout(prob, torch.from_numpy(np.array(s0)).to(DEV), case.N, case.H, sampler=sp, n_offset=SAMPLE_OFFSET,
                                  actions_out=acts, states_out=states)
        torch.cuda.synchronize()
        assert np.array_equal(acts.cpu().numpy(), A)           # the in-call draw at n_offset
    _check_against_oracle(case, costs, states, ref_costs, ref_states)


@pytest.mark.parametrize("case", LARGE, ids=[c.id for c in LARGE])
def test_large_n_tiles_match_smaller_shards_bitwise_and_the_oracle(case):
    """test_gpu_m8.py's test_32_candidate_tiles_match_smaller_shards_bitwise scheme at the generic, reward-head
    and T = 1, 2, 4 shapes, and at the shapes that fall back to 16-candidate tiles."""
    out = rc.run_outcome(case)
    assert isinstance(out, rdm.Instance) and (out.R == 2 or out.fallback in ("lds", "actions"))
    prob = device_problem(_problem(case.id))
    s0, A, ref_costs, ref_states = _reference(case.id)
    full, states = _run(case, prob, s0, A, 16)
    parts = []
    for lo in range(0, case.N, 2048):
        hi = min(case.N, lo + 2048)
        parts.append(_run(case, prob, s0, A, 8 if (hi - lo) % 2 == 0 else 16, lo, hi)[0])
    assert torch.equal(full, torch.cat(parts, dim=1)), case.id
    _check_against_oracle(case, full, states, ref_costs, ref_states)


# ------------------------------------------------------------------------------------------------ whole plans
PLANS = [("t16_ring", 3, dict(W=1024, L=2), 100, 3, 2, 10, 0.1),
         ("t16_generic", 3, dict(W=1000, L=3, **rc.GENERIC), 65, 2, 2, 7, 0.0),
         ("wide_input", 3, rc.WIDE_90, 100, 3, 2, 10, 0.5)]


@pytest.mark.parametrize("name,cid,over,N,H,I,K,alpha", PLANS, ids=[p[0] for p in PLANS])
def test_cem_plan_at_envelope_shapes_against_the_oracle(name, cid, over, N, H, I, K, alpha):
    """test_gpu_fuzz.py's whole-plan check and bars where the fuzz does not go: W > 512 and 16 K0C > Wpad (the
    final states come from the plain single-workgroup trajectory kernel at all three)."""
    from mbrl_amd import CEMPlanner, fused
    p = ocem.synth_problem(cid, N=N, H=H, **over)
    cfg = p["cfg"]
    assert rdm.trajectory_kernel(cfg["s"], cfg["a"], cfg["W"], cfg["L"], H=H) == "plain"
    _, model_fn, cost_fn, sample_action = build(p)
    md = fused.describe_model(model_fn)
    assert md is not None and fused.describe_cost(cost_fn, md["s"], md) is not None, "fused path not taken"
    res = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H,
                                   num_candidates=N, num_elites=K, alpha=alpha, num_iterations=I,
                                   seed=p["rng_seed"], record=True)
    ref = ocem.cem_plan(p, N=N, H=H, K=K, alpha=alpha, num_iterations=I)
    for it in range(I):
        assert rel_err(res["returns"][it], ref["returns"][it]) < RTOL, (name, it)
        assert np.array_equal(res["elites"][it].cpu().numpy(), ref["elites"][it]), (name, it)
    assert np.array_equal(res["mu"].cpu().numpy(), ref["mu"][-1])
    assert np.array_equal(res["sigma"].cpu().numpy(), ref["sigma"][-1])
    assert np.array_equal(res["actions"].numpy(), ref["final_actions"])
    assert np.allclose(res["states"].numpy(), ref["final_states"], rtol=1e-4, atol=1e-4)


TRAJ = [("s90", 3, dict(s=90, a=6, L=2), 4), ("s_plus_a_100", 3, dict(s=60, a=40, L=2), 3),
        ("W1024", 3, dict(W=1024, L=2), 4), ("W1024_humanoid_E2", 5, dict(W=1024, E=2), 3),
        ("wide_input", 3, rc.WIDE_90, 3)]


@pytest.mark.parametrize("name,cid,over,H", TRAJ, ids=[t[0] for t in TRAJ])
def test_trajectory_past_the_cooperative_budgets_matches_the_oracle(name, cid, over, H):
    """mbrl_trajectory where both traj_reg_supported and traj_coop_supported refuse (s > 80, s + a > 96 at
    W = 512; every W > 512): the plain single-workgroup kernel, per member and member mean."""
    from mbrl_amd import fused
    p = ocem.synth_problem(cid, N=1, H=H, **over)
    a, s, E = p["cfg"]["a"], p["cfg"]["s"], p["cfg"]["E"]
    assert rdm.trajectory_kernel(s, a, p["cfg"]["W"], p["cfg"]["L"], E, H=H) == "plain"
    acts = np.random.default_rng(cid + H).uniform(-1, 1, size=(H, a)).astype(np.float32)
    prob = device_problem(p)
    members = torch.full((E, H, s), SENTINEL, dtype=torch.float32, device=DEV)
    st = fused.trajectory(prob, torch.from_numpy(p["s0"]).to(DEV), torch.from_numpy(acts).to(DEV), H, member_states=members)
    torch.cuda.synchronize()
    _, ref = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], acts[:, None, :], store_states=True)
    assert np.allclose(members.cpu().numpy(), ref[:, :, 0, :], rtol=1e-4, atol=1e-4)
    assert np.allclose(st.cpu().numpy(), np.mean(ref[:, :, 0, :], axis=0, dtype=np.float32), rtol=1e-4, atol=1e-4)


def test_mppi_plan_at_w1024_from_the_gpus_own_records():
    """test_gpu_mppi.py's plan check (each iteration's draw, costs and update from the GPU's own records,
    against tests/mppi_reference.py) at W = 1024."""
    from mbrl_amd import fused
    from test_gpu_mppi import F32, HI, LO, _check_update, _plan
    N, H, I, lam, alpha, upd = 200, 3, 2, 2.0, 0.1, True
    p = ocem.synth_problem(3, N=N, H=H, W=1024, L=2)
    a = p["cfg"]["a"]
    res = _plan(p, H, num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=upd)
    torch.cuda.synchronize()
    mu_h, sg_h = res["mu_hist"].cpu().numpy(), res["sigma_hist"].cpu().numpy()
    for i in range(I):
        A = cem_actions(mu_h[i], sg_h[i], LO, HI, p["rng_seed"], i, np.arange(N))
        got_c = res["costs"][i].cpu().numpy()
        ref_c = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A)
        assert rel_err(got_c, ref_c) < RTOL, i
        ref = mref.update(got_c, A, mu_h[i], sg_h[i], lam, alpha, upd)
        got = dict(mu=mu_h[i + 1], sigma=sg_h[i + 1], weights=res["weights"][i].cpu().numpy(), returns=ref["returns"],
                   stats=np.array([ref["beta"], ref["eta"]], F32))
        _check_update(got, ref, N, mu_h[i], sg_h[i], upd, f"envelope W=1024 it={i}")
    assert torch.equal(res["mu"], res["mu_hist"][I]) and torch.equal(res["actions"], res["mu"].clamp(LO, HI))
    _, states = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], res["actions"].cpu().numpy()[:, None, :],
                             store_states=True)
    assert np.allclose(res["states"].cpu().numpy(), states[0, :, 0, :], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("sampled", [False, True], ids=["given", "sampled"])
@pytest.mark.parametrize("case", rc.REFUSED, ids=[c.id for c in rc.REFUSED])
def test_refused_shape_returns_unsupported_and_touches_nothing(case, sampled):
    """The exact code and message from mbrl_rollout_cost, and no launch: costs, states_out and (for a
    sampled call, whose draw would come first) actions_out keep their sentinel."""
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    s, a, W, L, E, reward = rc.shape_of(case)
    want = rc.outcome(case)
    assert isinstance(want, rdm.Refusal) and want.fragment == case.fragment
    shape = _lib.MlpShape(s, a, W, L, E, reward, 0)
    nbytes = lib.mbrl_mlp_packed_bytes(ctypes.byref(shape))
    assert (nbytes == 0) == (rdm.geometry(s, a, W, L, E, reward) is None)
    packed = torch.zeros(max(nbytes, 4096) // 4, dtype=torch.float32, device=DEV)   # sized as a real pack
    N, H = case.N, case.H
    s0 = torch.zeros(s, device=DEV)
    acts = torch.zeros((H, N, a), device=DEV)
    outs = [torch.full(sh, SENTINEL, device=DEV) for sh in ((E, N), (E, H, N, s), (H, N, a))]
    cost = _lib.Cost(_lib.MBRL_COST_GOAL_STATE, 0, 0, 0, None, None, 0.0, 0.0)
    mu, sg = torch.zeros((H, a), device=DEV), torch.full((H, a), 0.5, device=DEV)
    sp = fused.make_sampler(1, 0, mu, sg, -1.0, 1.0)
    rcode = lib.mbrl_rollout_cost(ctypes.byref(shape), _lib.ptr(packed), None, ctypes.byref(cost), _lib.ptr(s0), 0,
                                  None if sampled else _lib.ptr(acts), ctypes.byref(sp) if sampled else None, N, H, 0,
                                  _lib.ptr(outs[0]), _lib.ptr(outs[2]), _lib.ptr(outs[1]), _lib.stream_handle(torch.device(DEV)))
    msg = lib.mbrl_last_error().decode()
    torch.cuda.synchronize()
    assert rcode == _lib.MBRL_EUNSUPPORTED == want.code, (rcode, msg)
    assert case.fragment in msg, msg
    for o in outs:
        assert bool((o == SENTINEL).all()), case.id


@pytest.mark.parametrize("case", rc.REFUSED, ids=[c.id for c in rc.REFUSED])
def test_planners_raise_on_a_refused_shape(case):
    """CEMPlanner (every refusal) and MPPIPlanner raise RuntimeError with the library's reason rather than
    returning numbers; W = 1025 and L = 5 are refused by the Python layer's pack."""
    from mbrl_amd import CEMPlanner, MPPIPlanner
    p = ocem.synth_problem(case.cid, N=case.N, H=case.H, **case.over)
    _, model_fn, cost_fn, sample_action = build(p)
    frag = "unsupported MLP shape for the HIP path" if "MLP shape" in case.fragment else case.fragment
    for planner, kw in ((CEMPlanner, dict(num_elites=4)), (MPPIPlanner, dict(temperature=1.0))):
        with pytest.raises(RuntimeError) as ei:
            planner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, case.H,
                                  num_candidates=case.N, num_iterations=1, seed=1, **kw)
        assert frag in str(ei.value).replace("\\", ""), str(ei.value)
