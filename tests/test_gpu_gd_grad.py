"""GPU: mbrl_gd_grad -- the gradient one iteration of the gradient-descent planner consumes, out of
the very kernels and dispatch of mbrl_gd_plan_batch (gd_plan_kernel, gd_coop_kernel) -- against the
float64 autograd gradient of tests/gd_grad_reference.py, at the cases of tests/gd_grad_cases.py.

The plan tests (test_gd.py, test_gpu_flags.py) compare actions after N Adam steps, and Adam divides
the gradient's scale out: a backward pass that lost 1 / act_std, applied rew_std twice or dropped a
whole-gradient factor in the reduce-scatter would pass them all. Here

    e(x) = max |x - g64| / max |g64|,     e(gpu) <= bar(case) = 8 x max(e(grad32), median e(grad32)),

where grad32 is the same chain evaluated in float32 on the CPU: the bar is the float32 restatement's
own distance to float64, never the kernel's. The kernels are float32 evaluations of that chain in
other summation orders (K slices through LDS, wave reductions, the reduce-scatter), so their error is
of the same kind and size without being equal: hence the 8. tests/test_gd_grad_host.py shows on the
CPU that every single wrong backward factor misses these bars at least tenfold, and that no ReLU of
a case can change side between the precisions."""
import functools
from contextlib import ExitStack

import numpy as np
import pytest
import torch

import gd_grad_cases as gc
import gd_grad_reference as ref
from oracle import cem as ocem

from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
LR = 0.01


@functools.lru_cache(maxsize=None)
def device_problem(name):
    from test_gpu_flags import device_problem as build
    return build(gc.problem(name))


def run_grad(name, opts=(), plans=None):
    """mbrl_gd_grad on the case's plans (all, or the listed ones in one call) under the options:
    (states [B, H + 1, s], grad [B, H, a]) as NumPy. The given actions must come back untouched."""
    S0, A = gc.inputs(name)
    if plans is not None:
        S0, A = S0[list(plans)], A[list(plans)]
    return grad_call(device_problem(name), S0, A, opts)


def grad_call(prob, S0, A, opts=(), make_ws=None, alloc=None):
    """mbrl_gd_grad on start states S0 [B, s] and sequences A [B, H, a]. make_ws(nbytes) -> the uint8 workspace
    and alloc(*shape, dt=) -> an output tensor replace the private allocations (tests/workspace_cases.py)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    B, H, a = A.shape
    s0 = torch.from_numpy(np.array(S0)).to(DEV)
    acts = torch.from_numpy(np.array(A)).to(DEV)
    e = alloc or (lambda *sh, dt=torch.float32: torch.full(sh, float("nan"), dtype=dt, device=DEV))  # noqa: E731
    grad, states = e(B, H, a), e(B, H + 1, S0.shape[1])
    need = lib.mbrl_gd_batch_workspace_bytes(prob.refs[0], H, B)
    ws = make_ws(need) if make_ws else torch.empty(need, dtype=torch.uint8, device=DEV)
    with ExitStack() as stack:
        for opt, value in opts:
            stack.enter_context(_lib.option(opt, value))
        _lib.check(lib.mbrl_gd_grad(*prob.refs, _lib.ptr(s0), _lib.ptr(acts), B, H, _lib.ptr(grad), _lib.ptr(states),
                                    _lib.ptr(ws), need, _lib.stream_handle(torch.device(DEV))), "mbrl_gd_grad")
        torch.cuda.synchronize()
    assert np.array_equal(acts.cpu().numpy(), A), "mbrl_gd_grad wrote to its actions"
    return states.cpu().numpy(), grad.cpu().numpy()


def check_grad(name, grad, what, plans=None, factor=gc.BAR_FACTOR):
    g64 = gc.g64(name) if plans is None else gc.g64(name)[list(plans)]
    e, bar = ref.err(grad, g64), gc.bar(name, factor)
    print(f"{name} {what}: e(gpu) {e:.3e}, e(grad32) {gc.e32(name):.3e}, ratio {e / gc.e32(name):.2f}, bar {bar:.3e}")
    assert np.all(np.isfinite(grad))
    assert e <= bar, f"{name} {what}: e(gpu) = {e:.3e} > bar = {bar:.3e}"
    return e


def check_states(name, states, plans=None):
    """states_out against the oracle's rollout of the given actions, at test_trajectory_states_match_oracle's bars."""
    p = gc.problem(name)
    S0, A = gc.inputs(name)
    for i, b in enumerate(range(A.shape[0]) if plans is None else plans):
        _, st = ocem.rollout(p["model"], p["norm"], p["cost"], S0[b], A[b][:, None, :], store_states=True)
        assert np.array_equal(states[i, 0], S0[b])
        assert np.allclose(states[i, 1:], st[0, :, 0, :], rtol=1e-4, atol=1e-4), (name, b)


@pytest.mark.parametrize("name", gc.NAMES)
def test_gradient_matches_float64_autograd(name):
    """Every case through the default dispatch: the cooperative kernel where gd_coop_supported accepts the
    shape (gd_grad_cases.coop_expected restates it), else the one-workgroup kernel."""
    states, grad = run_grad(name)
    check_states(name, states)
    check_grad(name, grad, "coop" if gc.coop_expected(name) else "single")


@pytest.mark.parametrize("name", [n for n in gc.NAMES if gc.coop_expected(n)])
def test_one_workgroup_kernel_on_the_cooperative_shapes(name):
    """MBRL_OPT_GD_SINGLE: the one-workgroup kernel meets the same bar on every cooperative case, and the
    two kernels agree within 2 x bar (not bit for bit: their summation orders differ)."""
    states, grad = run_grad(name, (("gd_single", 1),))
    check_states(name, states)
    check_grad(name, grad, "gd_single")
    _, coop = run_grad(name)
    d = ref.err(grad, coop) * float(np.max(np.abs(coop)) / np.max(np.abs(gc.g64(name))))
    print(f"{name}: coop vs gd_single {d:.3e} (2 x bar {2 * gc.bar(name):.3e})")
    assert d <= 2 * gc.bar(name)


@pytest.mark.parametrize("hop", gc.HOP_VALUES)
@pytest.mark.parametrize("name", gc.HOP_CASES)
def test_every_hand_off_mode(name, hop):
    states, grad = run_grad(name, (("gd_hop", hop),))
    check_states(name, states)
    check_grad(name, grad, f"gd_hop={hop}")


@pytest.mark.parametrize("name", gc.ABORT_CASES)
def test_gated_fallback_produces_the_gradient(name):
    """MBRL_OPT_DEBUG_GD_ABORT: the cooperative kernel gives up at once; the one-workgroup kernel gated on
    its status word must write the gradient and the states (both NaN-filled before the call)."""
    states, grad = run_grad(name, (("debug_gd_abort", 1),))
    check_states(name, states)
    check_grad(name, grad, "debug_gd_abort")
    _, single = run_grad(name, (("gd_single", 1),))
    assert np.array_equal(grad, single)        # the fallback is the one-workgroup kernel


@pytest.mark.parametrize("name", gc.SEAM_CASES)
def test_the_seam_is_the_plans_gradient(name):
    """mbrl_gd_plan with one iteration and no stop test from the same inputs: its states are
    mbrl_gd_grad's bit for bit, and its actions are the Adam step on mbrl_gd_grad's gradient. The first
    step of Adam is a0 - lr g / (|g| + eps) (m / (1 - b1) = g, v / (1 - b2) = g^2); the kernel reaches it
    through some eight float32 roundings of a step of size lr, 5e-9 at most, so the bar is one float32
    ulp at the magnitude of the subtraction's operands, and no finer than the ulp of 1 / 16 (7.5e-9)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    prob = device_problem(name)
    S0, A = gc.inputs(name)
    H, s = A.shape[1], S0.shape[1]
    states, grad = run_grad(name, plans=[0])
    acts = torch.from_numpy(np.array(A[0])).to(DEV)
    s0 = torch.from_numpy(np.array(S0[0])).to(DEV)
    st = torch.full((H + 1, s), float("nan"), dtype=torch.float32, device=DEV)
    iters = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = lib.mbrl_gd_workspace_bytes(prob.refs[0], H)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.mbrl_gd_plan(*prob.refs, _lib.ptr(s0), _lib.ptr(acts), H, 1, 0.0, LR, _lib.ptr(st), _lib.ptr(iters),
                                _lib.ptr(ws), need, _lib.stream_handle(torch.device(DEV))), "mbrl_gd_plan")
    torch.cuda.synchronize()
    assert int(iters.item()) == 1
    assert np.array_equal(st.cpu().numpy(), states[0])
    g = grad[0].astype(np.float64)
    a0 = A[0].astype(np.float64)
    want = a0 - float(np.float32(LR)) * g / (np.abs(g) + 1e-8)
    got = acts.cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.maximum(np.maximum(np.abs(a0), np.abs(want)), 1.0 / 16).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(got - want) / ulp))
    print(f"{name}: plan step vs a0 - lr g / (|g| + eps): {worst:.3f} ulp")
    assert np.all(np.abs(got - want) <= ulp), worst
    assert float(np.max(np.abs(got - a0))) > 0.5 * LR       # the plan did step


@pytest.mark.parametrize("name,mode", [("batch_b11", "coop"), ("batch_b3", "coop"), ("batch_b3", "gd_single"),
                                       ("batch_b3", "debug_gd_abort")])
def test_batch_equals_single_calls(name, mode):
    """One call for B plans (B = 11 at Wpad 512: two groups of cooperative grids) is bit for bit the B
    calls for one plan each, through the cooperative kernel, the one-workgroup kernel and the gated fallback."""
    opts = gc.BATCH_MODES[mode]
    states, grad = run_grad(name, opts)
    check_grad(name, grad, f"batch {mode}")
    for b in range(gc.CASES[name]["B"]):
        s1, g1 = run_grad(name, opts, plans=[b])
        assert np.array_equal(states[b], s1[0]) and np.array_equal(grad[b], g1[0]), b


@pytest.mark.parametrize("name", ["batch_b3", "single_w16_l3"])
def test_python_entry_is_the_abi_call(name):
    """gd.grad_fused on the described closures returns what the raw call returns, and leaves its inputs alone."""
    import flag_cases as fc
    from mbrl_amd import gd
    p = gc.problem(name)
    S0, A = gc.inputs(name)
    _, model_fn, cost_fn, _ = fc.closures(p)
    dev = torch.device(DEV)
    mdesc, cdesc = gd.describe(model_fn, cost_fn, dev)
    assert mdesc is not None and gd.fused_supported(mdesc, cdesc, dev)
    acts = torch.from_numpy(np.array(A))
    st, g = gd.grad_fused(torch.from_numpy(np.array(S0)), mdesc, cdesc, acts, A.shape[1], dev)
    torch.cuda.synchronize()
    states, grad = run_grad(name)
    assert st.shape == states.shape and g.shape == grad.shape
    assert np.array_equal(st.cpu().numpy(), states) and np.array_equal(g.cpu().numpy(), grad)
    assert np.array_equal(acts.numpy(), A)


def test_refusals_are_codes_and_launch_nothing():
    """Argument checks as mbrl_gd_plan_batch's, plus the NULL grad_out: the outputs keep their fill."""
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    name = "coop_w64_l3"
    prob = device_problem(name)
    shape, packed, norm, cost = prob.refs
    S0, A = gc.inputs(name)
    _, H, a = A.shape
    s0 = torch.from_numpy(np.array(S0[0])).to(DEV)
    acts = torch.from_numpy(np.array(A[0])).to(DEV)
    grad = torch.full((H, a), 7.0, dtype=torch.float32, device=DEV)
    states = torch.full((H + 1, S0.shape[1]), 7.0, dtype=torch.float32, device=DEV)
    need = lib.mbrl_gd_batch_workspace_bytes(shape, H, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = _lib.stream_handle(torch.device(DEV))
    args = lambda **kw: [kw.get(k, v) for k, v in dict(  # noqa: E731
        shape=shape, packed=packed, norm=norm, cost=cost, s0=_lib.ptr(s0), actions=_lib.ptr(acts), B=1, H=H,
        grad=_lib.ptr(grad), states=_lib.ptr(states), ws=_lib.ptr(ws), need=need, stream=st).items()]
    assert lib.mbrl_gd_grad(*args(grad=None)) == _lib.MBRL_EINVAL
    assert lib.mbrl_gd_grad(*args(states=None)) == _lib.MBRL_EINVAL
    assert lib.mbrl_gd_grad(*args(H=0)) == _lib.MBRL_EINVAL
    assert lib.mbrl_gd_grad(*args(B=0)) == _lib.MBRL_EINVAL
    assert lib.mbrl_gd_grad(*args(need=need - 1)) == _lib.MBRL_EWORKSPACE
    goal = _lib.Cost(_lib.MBRL_COST_GOAL_STATE, 1, 1, 0, None, None, 0.4, 0.25)     # a reward-head model's cost is MODEL_REWARD
    assert lib.mbrl_gd_grad(*args(cost=fused.ctypes_ref(goal))) == _lib.MBRL_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all()) and bool((states == 7.0).all())
    assert lib.mbrl_gd_grad(*args()) == _lib.MBRL_OK
    torch.cuda.synchronize()
    assert not bool((grad == 7.0).any())
