"""GPU: every kernel family under the normaliser-flag subsets and cost parameters of tests/flag_cases.py
(whose CPU test shows that a kernel ignoring one flag, weight or alpha would miss these bars; the one
exception, rew_std in the gradient-descent backward, is named at test_gd_kernels and covered by
tests/test_gpu_gd_grad.py), against the CPU
oracle -- itself pinned on these branches by tests/test_oracle_flags.py -- and, for the
gradient-descent kernels, against the reference's autograd host loop. A cleared flag's
statistics pointer is really NULL on the device (asserted in device_problem), which is what
fused.describe_norm makes of a model partial that binds no such normaliser.

Which epilogue instance each rollout family runs, read from plan.hip rollout_impl and rollout.hip
launch_rollout (K0C / NOT = the even-rounded 16-chunks of s + a / s; RING needs both in {2, 6}):
  rollout_cid2       MBRL_OPT_ROLLOUT_TILE 16: rollout_kernel<T 4, R 1, 2, 2, 8 waves>, RING + EREG
  rollout_ring_ereg  tile 16: rollout_kernel<8, 1, 2, 2, 8> with the half-group seam, RING + EREG
  rollout_ring_wide  tile 16: s = 67 -> K0C = NOT = 6: RING, state slots from LDS (no EREG), E = 5
  rollout_nonring    s = 40, a = 6 -> K0C = NOT = 4: rollout_kernel<8, 1, 0, 0, 8>, the generic epilogue
                     (no 8- / 4-candidate stream exists for it, so no option is needed)
  rollout_r2         N = 8200 >= 8192: R = 2 on 8 waves (aliased partials), RING without EREG
  rollout_tiles_*    tile 8 / 4 / 16: rollout_m8_kernel, rollout_m4_kernel, rollout_kernel (bit-equal)
  rollout_pair       MBRL_OPT_ROLLOUT_PAIR 1 + DEBUG_PAIR_ABORT 2 in a plan: rollout_kernel<8, 1, 2, 2, 8, PAIR>
  rollout_split      precision f16x3 / f16x6: rollout_split_kernel (the fp32 redo behind it finds nothing
                     to redo: test_flag_cases.py keeps every operand below 2048)
  rollout_reward     reward head (no small-tile stream): rollout_kernel<8, 1, 2, 2, 8>, reward epilogue
Without the tile option cid 2 at N = 33 and cid 3 at N = 300 would run rollout_m8_kernel (fewer
16-candidate tiles than half the CUs)."""
import functools
from contextlib import ExitStack

import numpy as np
import pytest
import torch

import flag_cases as fc
from oracle import cem as ocem

from test_gpu_parity import DEV, RTOL, rel_err

pytestmark = pytest.mark.gpu
assert RTOL == fc.RTOL


@functools.lru_cache(maxsize=None)
def case(family, variant):
    """(problem, given actions, oracle costs [E, N], oracle states [E, H, N, s]); shared, never written."""
    p = fc.problem(family, variant)
    A = fc.actions(p)
    costs, states = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A, store_states=True)
    for x in (A, costs, states):
        x.setflags(write=False)
    return p, A, costs, states


closures = fc.closures    # build() binding only the normalisers this problem's flags name


def device_problem(p, precision="f32"):
    """A DeviceProblem of its own (never the cache's) for the closures of `p`: recognised by the fused
    path with exactly p's flags and NULL statistics; has_state / has_action go into the C cost struct."""
    from mbrl_amd import _lib, fused
    _, model_fn, cost_fn, _ = closures(p)
    md = fused.describe_model(model_fn)
    assert md is not None, "model closure not recognised"
    cd = fused.describe_cost(cost_fn, md["s"], md)
    assert cd is not None, "cost closure not recognised"
    n = md["norm"]
    for k in ocem.NORM_FLAGS:
        assert bool(n[k]) == ocem.norm_flag(p["norm"], k), k
    obs_null, act_null = fc.null_stats(p)
    assert (n["obs_mean"] is None, n["obs_std"] is None) == (obs_null, obs_null)
    assert (n["act_mean"] is None, n["act_std"] is None) == (act_null, act_null)
    prob = fused.DeviceProblem(md, cd, torch.device(DEV), _lib.precision_code(precision))
    assert (prob.norm.obs_mean is None, prob.norm.act_mean is None) == (obs_null, act_null)
    c = p["cost"]
    if c.get("kind") != "reward":
        assert np.array_equal(cd["weights"].numpy(), c["weights"]) and cd["alpha_state"] == c["alpha_state"] \
            and cd["alpha_action"] == c["alpha_action"]
        if "has_state" in c or "has_action" in c:
            prob.cost = _lib.Cost(_lib.MBRL_COST_GOAL_STATE, int(c.get("has_state", True)),
                                  int(c.get("has_action", True)), 0, _lib.ptr(prob._cost_t[0]),
                                  _lib.ptr(prob._cost_t[1]), c["alpha_state"], c["alpha_action"])
    norm_ref = fused.ctypes_ref(prob.norm) if p["norm"] is not None else None     # norm == NULL
    prob.refs = (fused.ctypes_ref(prob.shape), _lib.ptr(prob.packed), norm_ref, fused.ctypes_ref(prob.cost))
    return prob


def rollout(prob, p, A, opts=()):
    """mbrl_rollout_cost through ctypes with prob.refs (so norm may be NULL): (costs [E, N], states)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    H, N, _ = A.shape
    E, s = p["cfg"]["E"], p["cfg"]["s"]
    s0 = torch.from_numpy(p["s0"]).to(DEV)
    acts = torch.from_numpy(np.array(A)).to(DEV)          # (a copy: the shared case is read-only)
    costs = torch.full((E, N), float("nan"), dtype=torch.float32, device=DEV)
    states = torch.full((E, H, N, s), float("nan"), dtype=torch.float32, device=DEV)
    with ExitStack() as stack:
        for name, value in dict(opts).items():
            stack.enter_context(_lib.option(name, value))
        _lib.check(lib.mbrl_rollout_cost(*prob.refs, _lib.ptr(s0), 0, _lib.ptr(acts), None, N, H, 0, _lib.ptr(costs),
                                         None, _lib.ptr(states), _lib.stream_handle(torch.device(DEV))),
                   "mbrl_rollout_cost")
        torch.cuda.synchronize()
    return costs, states


def check_rollout(costs, states, ref_costs, ref_states, variant, what=""):
    err = rel_err(costs, ref_costs)
    d = float(np.max(np.abs(states.cpu().numpy() - ref_states)))
    print(f"{what} {variant}: returns rel_err {err:.3e} (bar {RTOL:g}), states max abs {d:.3e} (bar 1e-4)")
    assert err < RTOL
    assert np.allclose(states.cpu().numpy(), ref_states, rtol=1e-4, atol=1e-4)
    if variant == "no_cost":
        assert not costs.cpu().numpy().any()       # both terms dropped: exactly 0


# ------------------------------------------------------------------------------------------------ a. rollout
TILE16 = (("rollout_tile", 16),)
ROLLOUT_OPTS = {"rollout_cid2": TILE16, "rollout_ring_ereg": TILE16, "rollout_ring_wide": TILE16,
                "rollout_nonring": (), "rollout_r2": (), "rollout_reward": ()}


@pytest.mark.parametrize("family,variant", fc.pairs(*ROLLOUT_OPTS))
def test_rollout_kernel_epilogues(family, variant):
    p, A, ref_costs, ref_states = case(family, variant)
    costs, states = rollout(device_problem(p), p, A, ROLLOUT_OPTS[family])
    check_rollout(costs, states, ref_costs, ref_states, variant, family)


@pytest.mark.parametrize("family,variant", fc.pairs("rollout_tiles_cid2", "rollout_tiles_cid3"))
def test_small_tiles_match_16_bitwise_and_the_oracle(family, variant):
    """rollout_m8_kernel, rollout_m4_kernel and the 16-candidate kernel: the same bits under every
    normaliser subset and a non-default cost, and the oracle bars."""
    p, A, ref_costs, ref_states = case(family, variant)
    prob = device_problem(p)
    c16, s16 = rollout(prob, p, A, {"rollout_tile": 16})
    for m in (8, 4):
        c, s = rollout(prob, p, A, {"rollout_tile": m})
        assert torch.equal(c, c16) and torch.equal(s, s16), m
    check_rollout(c16, s16, ref_costs, ref_states, variant, family)


@pytest.mark.parametrize("precision", ["f16x3", "f16x6"])
@pytest.mark.parametrize("family,variant", fc.pairs("rollout_split"))
def test_split_rollout(family, variant, precision):
    """rollout_split_kernel at test_gpu_f16x3.py's bars (the exact-fp32 ones). Had the split kernel
    declined the shape, rollout_impl would run the fp32 kernels instead (for this N the 8-candidate
    tiles, bit-equal to every other fp32 tile height): the split states must differ from those bits."""
    p, A, ref_costs, ref_states = case(family, variant)
    costs, states = rollout(device_problem(p, precision), p, A)
    check_rollout(costs, states, ref_costs, ref_states, variant, f"{family} {precision}")
    _, f32_states = rollout(device_problem(p), p, A)      # (the states: without the state term the costs
    assert not torch.equal(states, f32_states), \
        "the fp32 kernel's bits: rollout_split_kernel did not run"   # are a function of the actions alone)


def _plan_on(prob, p, I, opts=()):
    """mbrl_cem_plan on a DeviceProblem (planners._cem_fused_single: what CEMPlanner runs once the
    closures are described), recording every iteration."""
    from mbrl_amd import CEMPlanner, _lib, env, planners
    cfg = p["cfg"]
    sample_action = env.sample_action_fn(env.BoundedActionSpec(cfg["a"], -1.0, 1.0))
    st = CEMPlanner._settings_build(sample_action, cfg["H"], dict(num_candidates=cfg["N"], num_iterations=I,
                                                                   seed=p["rng_seed"], record=True, return_device=True))
    with ExitStack() as stack:
        for name, value in dict(opts).items():
            stack.enter_context(_lib.option(name, value))
        res = planners._cem_fused_single(prob, torch.from_numpy(p["s0"]).to(DEV), st)
        torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("family,variant", fc.pairs("rollout_pair"))
def test_pair_rollout_in_a_plan(family, variant):
    """The column-split pair kernel's own results (no redo launch behind it) in a one-iteration plan:
    the returns against the oracle's rollout of the same draw, and the plan bit for bit against
    16-candidate tiles."""
    from oracle.philox import cem_actions
    p = fc.problem(family, variant)
    cfg = p["cfg"]
    N, H, a = cfg["N"], cfg["H"], cfg["a"]
    prob = device_problem(p)
    pair = _plan_on(prob, p, 1, {"rollout_pair": 1, "debug_pair_abort": 2})
    m16 = _plan_on(prob, p, 1, {"rollout_tile": 16, "rollout_pair": 2})
    for k in ("costs", "returns", "elites", "mu", "sigma", "actions", "states"):
        assert torch.equal(pair[k], m16[k]), k
    A = cem_actions(np.zeros((H, a), np.float32), np.full((H, a), 0.5, np.float32), -1, 1, p["rng_seed"], 0, np.arange(N))
    ref = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A)
    err = rel_err(pair["costs"][0], ref)
    print(f"{family} {variant}: returns rel_err {err:.3e} (bar {RTOL:g})")
    assert err < RTOL


# ------------------------------------------------------------------------------------------------ b. trajectory
def trajectory(prob, p, acts, opts=(), make_ws=None, alloc=None):
    """fused.trajectory (the wrapper the planners' shard path uses), or for norm == NULL, which has no
    Python spelling, mbrl_trajectory through ctypes: (member-mean states [H, s], member states [E, H, s]).
    make_ws(nbytes) -> the uint8 workspace and alloc(*shape, dt=) -> an output tensor: the ctypes call on
    them, whatever the norm (tests/workspace_cases.py)."""
    from mbrl_amd import _lib, fused
    H = acts.shape[0]
    E, s = p["cfg"]["E"], p["cfg"]["s"]
    s0 = torch.from_numpy(p["s0"]).to(DEV)
    a_d = torch.from_numpy(np.array(acts)).to(DEV)
    e = alloc or (lambda *sh, dt=torch.float32: torch.full(sh, float("nan"), dtype=dt, device=DEV))  # noqa: E731
    members = e(E, H, s)
    with ExitStack() as stack:
        for name, value in dict(opts).items():
            stack.enter_context(_lib.option(name, value))
        if p["norm"] is not None and make_ws is None:
            states = fused.trajectory(prob, s0, a_d, H, member_states=members)
        else:
            lib = _lib.load()
            shape, packed, norm_ref, _ = prob.refs
            assert (norm_ref is None) == (p["norm"] is None)
            states = e(H, s)
            need = lib.mbrl_trajectory_workspace_bytes(shape, H)
            ws = make_ws(need) if make_ws else torch.empty(need, dtype=torch.uint8, device=DEV)
            _lib.check(lib.mbrl_trajectory(shape, packed, norm_ref, _lib.ptr(s0), _lib.ptr(a_d), H, _lib.ptr(states),
                                           _lib.ptr(members), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_handle(torch.device(DEV))), "mbrl_trajectory")
        torch.cuda.synchronize()
    return states, members


# traj_reg: cid 2 (Wpad 256, one hidden hand-off) -> traj_reg_kernel. traj_coop: cid 3 (W = 512, L = 3)
# -> traj_coop_kernel, the kernel that read NULL statistics before this change. traj_plain: W = 300
# (Wpad 320 > 256: not register-resident; W != Wpad: not cooperative) -> traj_kernel ungated; cid 3 at
# W = 50, L = 2 would be taken by traj_reg_kernel (Wpad 64, K0 = 23 <= 32). traj_fallback: the
# cooperative kernel gives up (MBRL_OPT_DEBUG_TRAJ_ABORT) and the gated traj_kernel computes the states.
TRAJ_OPTS = {"traj_reg": (), "traj_coop": (), "traj_plain": (), "traj_fallback": (("debug_traj_abort", 1),),
             "traj_ensemble": ()}


@pytest.mark.parametrize("family,variant", fc.pairs(*TRAJ_OPTS))
def test_trajectory_kernels(family, variant):
    p, A, _, ref_states = case(family, variant)
    states, members = trajectory(device_problem(p), p, A[:, 0, :], TRAJ_OPTS[family])
    ref = ref_states[:, :, 0, :]
    d = float(np.max(np.abs(members.cpu().numpy() - ref)))
    print(f"{family} {variant}: states max abs {d:.3e} (bar 1e-4)")
    assert np.allclose(members.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    assert np.allclose(states.cpu().numpy(), np.mean(ref, axis=0, dtype=np.float32), rtol=1e-4, atol=1e-4)


def test_flag_without_statistics_is_refused_before_any_launch():
    """A set flag whose statistics pointer is NULL: MBRL_EINVAL with the message from mbrl_trajectory,
    mbrl_rollout_cost and mbrl_gd_plan, and nothing is launched (the outputs keep their fill)."""
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    p, A, _, _ = case("traj_coop", "norm:all")
    prob = device_problem(p)
    shape, packed, _, cost = prob.refs
    H, N, a = A.shape
    s = p["cfg"]["s"]
    dev = torch.device(DEV)
    s0 = torch.from_numpy(p["s0"]).to(DEV)
    acts = torch.from_numpy(np.array(A)).to(DEV)          # (a copy: the shared case is read-only)
    t = prob._norm_t
    bad = [(_lib.Norm(None, None, _lib.ptr(t[2]), _lib.ptr(t[3]), None, None, 1, 0, 0, 0), "state normalisation"),
           (_lib.Norm(_lib.ptr(t[0]), None, _lib.ptr(t[2]), _lib.ptr(t[3]), None, None, 0, 1, 0, 0), "state normalisation"),
           (_lib.Norm(_lib.ptr(t[0]), _lib.ptr(t[1]), None, None, None, None, 0, 0, 1, 0), "action normalisation")]
    for norm, msg in bad:
        out = torch.full((H + 1, s), 7.0, dtype=torch.float32, device=DEV)
        costs = torch.full((1, N), 7.0, dtype=torch.float32, device=DEV)
        ws = torch.empty(max(lib.mbrl_trajectory_workspace_bytes(shape, H), lib.mbrl_gd_workspace_bytes(shape, H)),
                         dtype=torch.uint8, device=DEV)
        rcs = [lib.mbrl_trajectory(shape, packed, fused.ctypes_ref(norm), _lib.ptr(s0), _lib.ptr(acts), H,
                                   _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))]
        msgs = [lib.mbrl_last_error().decode()]
        rcs.append(lib.mbrl_rollout_cost(shape, packed, fused.ctypes_ref(norm), cost, _lib.ptr(s0), 0, _lib.ptr(acts),
                                         None, N, H, 0, _lib.ptr(costs), None, None, _lib.stream_handle(dev)))
        msgs.append(lib.mbrl_last_error().decode())
        rcs.append(lib.mbrl_gd_plan(shape, packed, fused.ctypes_ref(norm), cost, _lib.ptr(s0), _lib.ptr(acts), H, 2, 0.0,
                                    0.01, _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)))
        msgs.append(lib.mbrl_last_error().decode())
        torch.cuda.synchronize()
        assert rcs == [_lib.MBRL_EINVAL] * 3, rcs
        assert all(msg in m and "requested without" in m for m in msgs), msgs
        assert bool((out == 7.0).all()) and bool((costs == 7.0).all())
        assert np.array_equal(acts.cpu().numpy(), A)
    nocost = _lib.Cost(_lib.MBRL_COST_GOAL_STATE, 1, 1, 0, None, None, 0.4, 0.25)
    out = torch.full((H + 1, s), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.mbrl_gd_workspace_bytes(shape, H), dtype=torch.uint8, device=DEV)
    rc = lib.mbrl_gd_plan(shape, packed, prob.refs[2], fused.ctypes_ref(nocost), _lib.ptr(s0), _lib.ptr(acts), H, 2, 0.0,
                          0.01, _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
    assert rc == _lib.MBRL_EINVAL and "state cost without weights/goal" in lib.mbrl_last_error().decode()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ c. whole plans
def _check_plan(res, ref, I):
    for it in range(I):
        err = rel_err(res["returns"][it], ref["returns"][it])
        print(f"iteration {it}: returns rel_err {err:.3e} (bar {RTOL:g})")
        assert err < RTOL, it
        assert np.array_equal(res["elites"][it].cpu().numpy(), ref["elites"][it]), it
    assert np.array_equal(res["mu"].cpu().numpy(), ref["mu"][-1])
    assert np.array_equal(res["sigma"].cpu().numpy(), ref["sigma"][-1])
    assert np.array_equal(res["actions"].cpu().numpy(), ref["final_actions"])
    assert np.allclose(res["states"].cpu().numpy(), ref["final_states"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("family,variant", fc.pairs(*fc.PLAN_FAMILIES))
def test_cem_plan_with_a_normaliser_subset(family, variant):
    """CEMPlanner.plan_detailed on closures that bind a subset of the normalisers. plan_cid3 (W = 512,
    only normalize_action: obs statistics NULL) ends in traj_coop_kernel, the path that read address 0."""
    from mbrl_amd import CEMPlanner, fused
    p = fc.problem(family, variant)
    cfg = p["cfg"]
    module, model_fn, cost_fn, sample_action = closures(p)
    assert fused.describe(model_fn, cost_fn, torch.device(DEV))[0] is not None, "fused path not taken"
    I = fc.PLAN_ITERATIONS
    res = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, cfg["H"],
                                   num_candidates=cfg["N"], num_iterations=I, seed=p["rng_seed"], record=True)
    assert fused._PACKED.get(module) is not None
    ref, gaps = fc.plan_gaps(p)
    assert min(gaps) > fc.TIE_GAP
    _check_plan(res, ref, I)


def test_mppi_plan_with_a_normaliser_subset():
    from mbrl_amd import MPPIPlanner, fused
    p = fc.problem("plan_cid3", "norm:na")
    cfg = p["cfg"]
    _, model_fn, cost_fn, sample_action = closures(p)
    assert fused.describe(model_fn, cost_fn, torch.device(DEV))[0] is not None, "fused path not taken"
    res = MPPIPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, cfg["H"],
                                    num_candidates=cfg["N"], num_iterations=1, temperature=1.0, seed=p["rng_seed"],
                                    record=True)
    acts = res["actions"].cpu().numpy()
    _, states = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], acts[:, None, :], store_states=True)
    assert np.allclose(res["states"].cpu().numpy(), states[0, :, 0, :], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("family,variant", fc.pairs("forward"))
def test_dynamics_forward_with_a_normaliser_subset(family, variant):
    from mbrl_amd import fused
    p = fc.problem(family, variant)
    cfg = p["cfg"]
    module, model_fn, _, _ = closures(p)
    assert set(model_fn.keywords) == fc.norm_keys(p)
    rng = np.random.default_rng(5)
    s = (3 * rng.standard_normal((cfg["N"], cfg["s"]))).astype(np.float32)
    a = rng.uniform(-1, 1, (cfg["N"], cfg["a"])).astype(np.float32)
    with torch.no_grad():
        out = model_fn(torch.from_numpy(s).to(DEV), torch.from_numpy(a).to(DEV))
    ref = ocem.dynamics_step(p["model"][0], p["norm"], s, a)
    assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    assert fused._PACKED.get(module) is not None, "forward did not take the HIP path"


# ------------------------------------------------------------------------------------------------ d. gradient descent
GD_ITERS = fc.GD_ITERS
GD_MODES = {"default": (), "gd_single": (("gd_single", 1),), "debug_gd_abort": (("debug_gd_abort", 1),)}
_GD_REF = {}


def _gd_reference(family, variant, monkeypatch):
    """The reference's host loop (autograd on the very callables, on the CPU; gd.describe forced to
    decline as in test_gd_host_loop_matches_reference). A dropped cost term is a closure without it."""
    key = (family, variant)
    if key not in _GD_REF:
        from mbrl_amd import GradientDescentPlanner, gd
        p, A, _, _ = case(family, variant)
        _, model_fn, cost_fn, _ = closures(p)
        c = p["cost"]
        if not c.get("has_state", True):
            action_cost = cost_fn.keywords["action_cost"]
            cost_fn = lambda s, a: action_cost(a)                  # noqa: E731
        elif not c.get("has_action", True):
            state_cost = cost_fn.keywords["state_cost"]
            cost_fn = lambda s, a: state_cost(s)                   # noqa: E731
        monkeypatch.setattr(gd, "describe", lambda model, cost, dev: (None, None))
        H = A.shape[0]
        init = ([], [torch.from_numpy(A[i, 0:1].copy()) for i in range(H)])
        states, actions = GradientDescentPlanner.plan(torch.from_numpy(p["s0"]), model_fn, cost_fn, None, H, init,
                                                      num_iterations=GD_ITERS, stop_condition=0.0)
        monkeypatch.undo()
        _GD_REF[key] = (torch.cat(states).numpy(), torch.cat(actions).numpy())
    return _GD_REF[key]


@pytest.mark.parametrize("mode", list(GD_MODES))
@pytest.mark.parametrize("family,variant", fc.pairs("gd_coop", "gd_narrow", "gd_reward"))
def test_gd_kernels(family, variant, mode, monkeypatch):
    """gd.plan_fused (the cooperative kernel where it applies, the one-workgroup kernel, the gated
    fallback) against plain-torch autograd. has_state_cost / has_action_cost = 0 have no Python
    spelling: those go through a raw mbrl_gd_plan call on a DeviceProblem whose cost struct drops the term.

    What these outputs can show is asserted on the CPU (test_flag_cases.py, the same host loop on every
    mutant): each state / action normaliser, the weights, both alphas and both cost switches. They
    cannot show unnormalize_reward: rew_std only scales the gradient, and Adam's step does not depend on
    that scale, so "rew:ur" and "rew:none" expect the same actions and states, and the GD kernels'
    rew_std factor is not covered here (flag_cases.GD_BLIND) but in tests/test_gpu_gd_grad.py."""
    from mbrl_amd import _lib, gd
    ref_states, ref_actions = _gd_reference(family, variant, monkeypatch)
    p, A, _, _ = case(family, variant)
    H = A.shape[0]
    dev = torch.device(DEV)
    acts = [torch.from_numpy(A[i, 0:1].copy()) for i in range(H)]
    s0 = torch.from_numpy(p["s0"])
    with ExitStack() as stack:
        for name, value in GD_MODES[mode]:
            stack.enter_context(_lib.option(name, value))
        if "has_state" in p["cost"] or "has_action" in p["cost"]:
            prob = device_problem(p)
            lib = _lib.load()
            s0_d = s0.to(DEV)
            a_d = torch.cat(acts, 0).to(DEV).contiguous()
            st = torch.empty((H + 1, p["cfg"]["s"]), dtype=torch.float32, device=DEV)
            need = lib.mbrl_gd_workspace_bytes(prob.refs[0], H)
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            _lib.check(lib.mbrl_gd_plan(*prob.refs, _lib.ptr(s0_d), _lib.ptr(a_d), H, GD_ITERS, 0.0, 0.01, _lib.ptr(st),
                                        None, _lib.ptr(ws), need, _lib.stream_handle(dev)), "mbrl_gd_plan")
        else:
            _, model_fn, cost_fn, _ = closures(p)
            mdesc, cdesc = gd.describe(model_fn, cost_fn, dev)
            assert mdesc is not None and cdesc is not None and gd.fused_supported(mdesc, cdesc, dev)
            assert fc.norm_keys(p) == {k for k in ocem.NORM_FLAGS if mdesc["norm"][k]}
            st, a_d, n = gd.plan_fused(s0, mdesc, cdesc, acts, H, GD_ITERS, 0.0, dev)
            assert int(n.item()) == GD_ITERS
        torch.cuda.synchronize()
    st, ac = st.cpu().numpy(), a_d.cpu().numpy()
    print(f"{family} {variant} {mode}: actions max abs {np.max(np.abs(ac - ref_actions)):.3e}, "
          f"states max abs {np.max(np.abs(st - ref_states)):.3e}")
    assert np.allclose(ac, ref_actions, **fc.GD_ACTION_TOL), np.max(np.abs(ac - ref_actions))
    assert np.allclose(st, ref_states, **fc.GD_STATE_TOL), np.max(np.abs(st - ref_states))
