"""GPU: the batched receding-horizon CEM plan (mbrl_cem_plan_rh_batch: the problem dimension of
csrc/cem_rh.hip and the staged refit, its loop in plan.hip), cem_plan_batch_rh and RecedingHorizonCEMPlanner
behind the planner service, against the NumPy restatement (tests/cem_rh_batch_reference.py).

Bars, per problem and per iteration of every fixture batch, the single plan's: costs within 1e-5 relative of
the restatement's; the elite and the best index sets identical (tests/test_cem_rh_batch_host.py asserts that
every problem's K-th and Kc-th return gaps exceed 1e-4); mu, sigma, the kept rows, the carry and the final
actions bit for bit; the carry's returns the GPU's own returns at the best indices; final states within 1e-5.
B = 1 and problem 0 of any batch are mbrl_cem_plan_rh bit for bit; keep == 0 without rows is
mbrl_cem_plan_batch bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cem_rh_batch_reference as br
import cem_rh_reference as rh
from oracle import cem as ocem

from test_gpu_cem_rh import _bits, _check_against_restatement, _dev, _params, _rel, c_plan_rh
from test_gpu_parity import build, device_problem

pytestmark = pytest.mark.gpu
F32 = np.float32
LO, HI = -1.0, 1.0
RTOL = 1e-5
DEV = "cuda:0"
H, K, I = br.SMALL["H"], br.SMALL["K"], br.SMALL["I"]
OUTPUTS = ("mu", "sigma", "actions", "states", "carry", "carry_returns")
RECORDS = ("costs", "returns", "elites", "kept_hist")


def c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=0, ins=None, flags="given", record=True, expect=0, ws_bytes=None,
                    B=None, null=(), ws_size=None, make_ws=None, alloc=None):
    """mbrl_cem_plan_rh_batch through ctypes. ins: br.stack_inputs' dict (its flags are passed unless
    flags=None). Returns the outputs and records as device tensors; with `expect` nonzero, asserts that return
    code and that nothing was written. null: names among packed / s0 / actions / states / workspace passed as
    NULL; ws_size: the bytes to allocate when the query cannot size the call. make_ws(nbytes) -> the uint8 workspace and
    alloc(*shape, dt=) -> an output tensor replace the private allocations (tests/workspace_cases.py)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    md = prob.mdesc
    a, s, E = md["a"], md["s"], md["E"]
    B = len(s0s) if B is None else B
    Bo = max(B, 1)
    params = _params(p, N, H, K, I, keep)
    need = lib.mbrl_cem_rh_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), B)
    dev = torch.device(DEV)
    ws = make_ws(need) if make_ws else torch.empty(max(ws_size or (need if ws_bytes is None else ws_bytes), 256),
                                                   dtype=torch.uint8, device=dev)
    e = alloc or (lambda *sh, dt=torch.float32: torch.full(sh, -7, dtype=dt, device=dev))  # noqa: E731
    out = dict(mu=e(Bo, H, a), sigma=e(Bo, H, a), actions=e(Bo, H, a), states=e(Bo, H, s))
    Kc = max(keep, 0)
    if Kc:
        out.update(carry=e(Bo, Kc, H, a), carry_returns=e(Bo, Kc))
    if record:
        out.update(costs=e(I, E, Bo * N), returns=e(I, Bo, N), elites=e(I, Bo, K, dt=torch.int64))
        if Kc:
            out.update(kept_hist=e(I + 1, Bo, Kc, H, a))
    g = lambda k: None if k in null else _lib.ptr(out.get(k))  # noqa: E731
    ins = ins or {}
    s0 = _dev(np.asarray(s0s, F32))
    fl = ins.get("flags") if isinstance(flags, str) else flags
    fl_d = None if fl is None else torch.from_numpy(np.ascontiguousarray(fl, dtype=np.int32)).to(DEV)
    ptrs = [_dev(ins.get(k)) for k in ("init_mu_rows", "init_sigma_rows", "carry_in")]
    refs = list(prob.refs)
    if "packed" in null:
        refs[1] = None
    rc = lib.mbrl_cem_plan_rh_batch(*refs, None if "s0" in null else _lib.ptr(s0), B, ctypes.byref(params),
                                    *[_lib.ptr(x) for x in ptrs], _lib.ptr(fl_d), g("mu"), g("sigma"), g("actions"),
                                    g("states"), g("carry"), g("carry_returns"), g("costs"), g("returns"), g("elites"),
                                    g("kept_hist"), None if "workspace" in null else _lib.ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, lib.mbrl_last_error())
        for k, v in out.items():          # refused before any launch: nothing was written
            assert bool((v == -7).all()), k
        return None
    _lib.check(rc, "mbrl_cem_plan_rh_batch")
    return out


def problem_of(got, b, N):
    """Problem b of a batched result in the single plan's shapes (what c_plan_rh returns)."""
    one = {k: got[k][b] for k in OUTPUTS if k in got}
    if "costs" in got:
        one.update(costs=got["costs"][:, :, b * N:(b + 1) * N], returns=got["returns"][:, b], elites=got["elites"][:, b])
    if "kept_hist" in got:
        one["kept_hist"] = got["kept_hist"][:, b]
    return one


def assert_same_bits(x, y, tag, keys=OUTPUTS + RECORDS):
    for k in keys:
        assert (k in x) == (k in y), (tag, k)
        if k in x:
            assert _bits(x[k].contiguous()) == _bits(y[k].contiguous()), (tag, k)


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_batch_against_the_restatement(case):
    W, L, a, N, E, Kc, inputs, _ = case
    p, s0s, kws = br.make_case(case)
    refs = br.cached_plans(case)
    got = c_plan_rh_batch(device_problem(p), p, s0s, N, H, K, I, keep=Kc, ins=br.stack_inputs(kws, H, a, Kc))
    for b, ref in enumerate(refs):
        _check_against_restatement(problem_of(got, b, N), ref, I, K, Kc, f"{br.case_id(case)} problem {b}")


def _single_plan_problem(keep, with_inputs, a=5, N=64, seed=7301):
    p = ocem.synth_problem(2, seed=seed, W=64, L=1, a=a, N=N, H=H)
    rng = np.random.default_rng(seed)
    s0s = np.stack([p["s0"]] + [(p["s0"] + rng.normal(0, 0.2, 5)).astype(F32) for _ in range(2)])
    kws = []
    for b in range(3):
        kw = {}
        if with_inputs:
            kw = dict(init_mu_rows=rng.uniform(-1.3, 1.3, (H, a)).astype(F32),
                      init_sigma_rows=rng.uniform(0.1, 0.6, (H, a)).astype(F32))
            if keep:
                kw["carry_in"] = rng.uniform(-1.2, 1.2, (keep, H, a)).astype(F32)
        kws.append(kw)
    return p, s0s, kws


@pytest.mark.parametrize("a", [5, 8], ids=["scalar", "vector"])
@pytest.mark.parametrize("with_inputs", [False, True], ids=["cold", "inputs"])
@pytest.mark.parametrize("keep", [0, 3])
def test_one_problem_and_problem_zero_are_the_single_plan_bit_for_bit(keep, with_inputs, a):
    """Outputs, carry and records: B = 1 (flags NULL and flags given) and problem 0 of a B = 3 batch."""
    N = 100
    p, s0s, kws = _single_plan_problem(keep, with_inputs, a=a, N=N)
    prob = device_problem(p)
    single = c_plan_rh(prob, p, N, H, K, I, keep=keep, **kws[0])
    one = br.stack_inputs(kws[:1], H, a, keep)
    for flags in (None, "given"):
        got = c_plan_rh_batch(prob, p, s0s[:1], N, H, K, I, keep=keep, ins=one, flags=flags)
        assert_same_bits(problem_of(got, 0, N), single, f"B=1 flags={flags}")
    got3 = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=keep, ins=br.stack_inputs(kws, H, a, keep))
    assert_same_bits(problem_of(got3, 0, N), single, "B=3 problem 0")
    assert not torch.equal(got3["mu"][1], got3["mu"][0])


@pytest.mark.parametrize("unfused", [0, 1], ids=["fused", "unfused"])
def test_keep_zero_without_rows_is_the_plain_batch_bit_for_bit(unfused):
    from mbrl_amd import _lib
    lib = _lib.load()
    N = 100
    p, s0s, _ = _single_plan_problem(0, False, N=N)
    prob = device_problem(p)
    a, s = prob.mdesc["a"], prob.mdesc["s"]
    params = _params(p, N, H, K, I, 0)
    dev = torch.device(DEV)
    with _lib.option("unfused_update", unfused):
        need = lib.mbrl_cem_plan_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params.cem), 3)
        assert lib.mbrl_cem_rh_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), 3) == need
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        plain = dict(mu=torch.empty(3, H, a, device=dev), sigma=torch.empty(3, H, a, device=dev),
                     actions=torch.empty(3, H, a, device=dev), states=torch.empty(3, H, s, device=dev))
        _lib.check(lib.mbrl_cem_plan_batch(*prob.refs, _lib.ptr(_dev(s0s)), 3, ctypes.byref(params.cem),
                                           *[_lib.ptr(plain[k]) for k in ("mu", "sigma", "actions", "states")],
                                           _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)), "mbrl_cem_plan_batch")
        torch.cuda.synchronize()
        for record in (False, True):
            got = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=0, record=record)
            assert_same_bits(got, plain, f"record={record}", keys=("mu", "sigma", "actions", "states"))


def test_a_cleared_flag_bit_plans_as_if_the_pointer_were_null():
    """Every pointer given for every problem; the flags alone decide. Problem b with a bit clear equals the
    restatement of that problem alone, planned at candidate offset b N without that input."""
    a, N, Kc = 5, 100, 3
    p, s0s, kws = _single_plan_problem(Kc, True, a=a, N=N, seed=7302)
    flags = np.array([br.FLAG_SIGMA | br.FLAG_CARRY, br.FLAG_MU | br.FLAG_CARRY, br.FLAG_MU | br.FLAG_SIGMA], np.int32)
    names = ("init_mu_rows", "init_sigma_rows", "carry_in")
    seen = [{n: kws[b][n] for j, n in enumerate(names) if flags[b] >> j & 1} for b in range(3)]
    refs = br.plan_batch(p, s0s, N, H, K, I, Kc, seen)
    assert min(rh.case_gaps(r, K, Kc) for r in refs) > br.GAP_MIN
    ins = br.stack_inputs(kws, H, a, Kc)
    assert ins["flags"].tolist() == [7, 7, 7]
    prob = device_problem(p)
    got = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=Kc, ins=ins, flags=flags)
    for b, ref in enumerate(refs):
        _check_against_restatement(problem_of(got, b, N), ref, I, K, Kc, f"cleared bits, problem {b}")
    assert not got["kept_hist"][0, 2].any() and _bits(got["kept_hist"][0, 0]) == _bits(kws[0]["carry_in"])
    # all bits clear: the batch without any pointer, bit for bit
    cold = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=Kc)
    zero = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=Kc, ins=ins, flags=np.zeros(3, np.int32))
    assert_same_bits(zero, cold, "flags all clear")
    # a set bit whose pointer is NULL is ignored
    ones = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=Kc, ins=dict(flags=np.full(3, 7, np.int32)))
    assert_same_bits(ones, cold, "bits without pointers")


def test_a_nan_carry_row_sorts_last_in_its_problem_and_touches_no_other():
    a, N, Kc = 5, 64, 3
    p, s0s, kws = _single_plan_problem(Kc, True, a=a, N=N, seed=7303)
    prob = device_problem(p)
    clean = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=Kc, ins=br.stack_inputs(kws, H, a, Kc))
    kws[1]["carry_in"][1, 2, 3] = np.nan
    ref = br.plan_problem(p, s0s[1], 1, N, H, K, I, keep=Kc, **kws[1])
    assert np.isnan(ref["returns"][0][1]) and np.isfinite(np.delete(ref["returns"][0], 1)).all()
    got = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=Kc, ins=br.stack_inputs(kws, H, a, Kc))
    r0 = got["returns"][0, 1].cpu().numpy()
    assert np.isnan(r0[1]) and np.isfinite(np.delete(r0, 1)).all()
    assert 1 not in got["elites"][0, 1].cpu().numpy()
    assert np.array_equal(ocem.select_elites(r0, Kc), ref["best"][0]) and 1 not in ref["best"][0]
    kept = got["kept_hist"][:, 1].cpu().numpy()
    assert _bits(kept[0]) == _bits(kws[1]["carry_in"])            # (row 0 of the record: carry_in as given)
    assert np.isfinite(kept[1:]).all() and np.isfinite(got["carry"].cpu().numpy()).all()
    assert _bits(got["mu"][1]) == _bits(ref["mu_out"]) and _bits(got["carry"][1]) == _bits(ref["carry"])
    for b in (0, 2):
        assert_same_bits(problem_of(got, b, N), problem_of(clean, b, N), f"problem {b} beside the NaN")
        assert np.isfinite(got["returns"][:, b].cpu().numpy()).all()


REFUSALS = [("B=0", "EINVAL"), ("K>N", "EINVAL"), ("iterations=0", "EINVAL"), ("keep>K", "EINVAL"), ("keep<0", "EINVAL"),
            ("carry_without_keep", "EINVAL"), ("null_packed", "EINVAL"), ("null_s0", "EINVAL"),
            ("null_actions", "EINVAL"), ("null_states", "EINVAL"), ("null_workspace", "EINVAL"),
            ("small_workspace", "EWORKSPACE"), ("N=32769", "EUNSUPPORTED"), ("B*N", "EUNSUPPORTED"),
            ("staged_refit", "EUNSUPPORTED")]


@pytest.mark.parametrize("what,code", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_argument_checks_return_before_any_launch(what, code):
    from mbrl_amd import _lib
    lib = _lib.load()
    N, I2 = 64, 2
    a = 48 if what == "staged_refit" else 5
    p = ocem.synth_problem(2, seed=7304, W=64, L=1, a=a, N=N, H=H)
    prob = device_problem(p)
    s0s = np.stack([p["s0"]] * 2)
    expect = getattr(_lib, "MBRL_" + code)
    query = lambda *args, B=2: lib.mbrl_cem_rh_batch_workspace_bytes(  # noqa: E731
        ctypes.byref(prob.shape), ctypes.byref(_params(p, *args)), B)
    run = functools.partial(c_plan_rh_batch, prob, p, s0s, expect=expect)
    if what == "B=0":
        assert query(N, H, K, I2, 3, B=0) == 0
        run(N, H, K, I2, keep=3, B=0, ws_size=1 << 20)
    elif what == "K>N":
        assert query(N, H, N + 1, I2, 3) == 0
        run(N, H, N + 1, I2, keep=3, ws_size=1 << 20)
    elif what == "iterations=0":
        assert query(N, H, K, 0, 3) == 0
        run(N, H, K, 0, keep=3, ws_size=1 << 20, record=False)
    elif what == "keep>K":
        assert query(N, H, K, I2, K + 1) == 0
        run(N, H, K, I2, keep=K + 1, ws_size=1 << 20)
    elif what == "keep<0":
        assert query(N, H, K, I2, -1) == 0
        run(N, H, K, I2, keep=-1, ws_size=1 << 20)
    elif what == "carry_without_keep":
        run(N, H, K, I2, keep=0, ins=dict(carry_in=np.zeros((2, 1, H, a), F32)))
    elif what.startswith("null_"):
        run(N, H, K, I2, keep=3, null=(what[5:],))
    elif what == "small_workspace":
        need = query(N, H, K, I2, 3)
        assert need > query(N, H, K, I2, 0) > 0
        run(N, H, K, I2, keep=3, ws_bytes=need - 256)
        run(N, H, K, I2, keep=0, ws_bytes=query(N, H, K, I2, 0) - 256)
    elif what == "N=32769":
        run(32769, 1, K, 1, keep=3, record=False, ws_size=1 << 20)
    elif what == "B*N":
        assert 32768 * 32768 > (2 ** 31 - 1) // 2
        c_plan_rh_batch(prob, p, np.zeros((32768, 5), F32), 32768, 1, K, 1, keep=3, record=False, ws_size=1 << 20,
                        expect=expect)
    else:   # 344 chunks of 32 elites x 48 dimensions x 4 bytes > 64 KiB: more than the staged refit's LDS
        Kbig = 32 * 343 + 1
        assert (Kbig + 31) // 32 * a * 4 > 64 * 1024
        run(16384, 1, Kbig, 1, keep=3, record=False, ws_size=1 << 20)
        # (keep == 0 does not stage: the same K x a is only refused where the batched refit itself refuses it)
    msg = lib.mbrl_last_error()
    # (the params checks are the single plan's, under its name)
    assert b"cem_plan_rh" in msg or b"CEM params" in msg or b"B*N" in msg or b"refit" in msg, msg


# ---- the Python entry: two consecutive control steps
TWO_STEP_SEED = 12     # (searched on the CPU: both steps' gaps exceed GAP_MIN; asserted below)


def two_step_restatement(seed):
    """Three problems, two control steps with warm_std="keep": step 2 plans from the restatement's own first
    predicted state with the previous plan's actions, sigma and carry shifted; problem 1 starts over (cold)."""
    from mbrl_amd.planners import cem_shift_carry, mppi_warm_start_rows
    a, N, Kc = 5, 64, 3
    p = ocem.synth_problem(2, seed=7400 + seed, W=64, L=1, a=a, N=N, H=H)
    rng = np.random.default_rng(seed)
    s0s = np.stack([p["s0"]] + [(p["s0"] + rng.normal(0, 0.2, 5)).astype(F32) for _ in range(2)])
    step1 = br.plan_batch(p, s0s, N, H, K, I, Kc, [{}, {}, {}])
    s1s = np.stack([r["final_states"][0] for r in step1]).astype(F32)
    kws = [dict(init_mu_rows=mppi_warm_start_rows(r["final_actions"], H, 1, LO, HI),
                init_sigma_rows=mppi_warm_start_rows(r["sigma_out"], H, 1, 0.0, np.inf),
                carry_in=cem_shift_carry(r["carry"], 1, LO, HI)) for r in step1]
    kws[1] = {}
    step2 = br.plan_batch(p, s1s, N, H, K, I, Kc, kws, seed=p["rng_seed"] + 1)
    return p, s0s, s1s, step1, step2


def test_cem_plan_batch_rh_two_control_steps_equal_the_restatement():
    from mbrl_amd import cem_plan_batch_rh, cem_shift_carry
    a, N, Kc = 5, 64, 3
    p, s0s, s1s, step1, step2 = two_step_restatement(TWO_STEP_SEED)
    assert min(rh.case_gaps(r, K, Kc) for r in step1 + step2) > br.GAP_MIN
    _, model_fn, cost_fn, sample_action = build(p)
    kw = dict(num_candidates=N, num_elites=K, num_iterations=I, warm_start=True, warm_std="keep", keep_elites=Kc)

    def check(res, refs, tag):
        assert res["carry"].shape == (3, Kc, H, a) and res["carry_returns"].shape == (3, Kc)
        for b, ref in enumerate(refs):
            for k, r in (("mu", "mu_out"), ("sigma", "sigma_out"), ("actions", "final_actions"), ("carry", "carry")):
                assert _bits(res[k][b]) == _bits(ref[r]), (tag, b, k)
            assert _rel(res["states"][b].numpy(), ref["final_states"]) < RTOL, (tag, b)
            assert _rel(res["carry_returns"][b].numpy().astype(np.float64), ref["carry_returns"]) < RTOL, (tag, b)

    r1 = cem_plan_batch_rh(torch.from_numpy(s0s), model_fn, cost_fn, sample_action, H, seed=p["rng_seed"], **kw)
    assert not r1["mu"].is_cuda and "costs" not in r1
    check(r1, step1, "step 1")
    inits = [(None, r1["actions"][b]) for b in range(3)]
    carries = [cem_shift_carry(r1["carry"][b], 1, LO, HI) for b in range(3)]
    sigmas = [r1["sigma"][b] for b in range(3)]
    inits[1] = carries[1] = sigmas[1] = None
    r2 = cem_plan_batch_rh(torch.from_numpy(s1s), model_fn, cost_fn, sample_action, H, inits, carries, sigmas,
                           seed=p["rng_seed"] + 1, record=True, return_device=True, **kw)
    assert r2["mu"].is_cuda and r2["kept_hist"].shape == (I + 1, 3, Kc, H, a) and r2["costs"].shape == (I, 1, 3 * N)
    assert not r2["kept_hist"][0, 1].any()                       # the problem that started over has no kept_0
    check({k: v.cpu() for k, v in r2.items()}, step2, "step 2")
    for b, ref in enumerate(step2):
        assert np.array_equal(r2["elites"][:, b].cpu().numpy(), np.stack(ref["elites"])), b
    # closures the fused path does not recognise are refused, as the single plan refuses them
    with pytest.raises(NotImplementedError, match="fused path"):
        cem_plan_batch_rh(torch.from_numpy(s0s), lambda s, a_: model_fn(s, a_), cost_fn, sample_action, H, seed=1, **kw)


def test_gpu_planner_service_serves_receding_horizon_cem_batches():
    """Workers step environments; the parent plans every lockstep round with one
    RecedingHorizonCEMPlanner.plan_batch (mbrl_cem_plan_rh_batch), each rollout warm-started from its own
    previous plan and memo: every round's served actions equal a direct plan_batch call given the same
    observations, trajectories and memos."""
    import standin_env as se
    from mbrl_amd import MPCPolicy, RecedingHorizonCEMPlanner, data, fused, models, parallel
    from mbrl_amd import env as menv
    from mbrl_amd import env_wrappers as ew
    torch.manual_seed(0)
    m = models.Model(5, 1, hidden_units=256, n_hidden=2)
    ds = data.TransitionsDataset.from_statistics({"observations": {"mean": torch.zeros(5), "std": torch.ones(5)},
                                                  "actions": {"mean": torch.zeros(1), "std": torch.ones(1)}})
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(5), torch.zeros(5)), models.CoshLoss())
    sample_action = functools.partial(ew.EnvWrapper._sample_action, action_spec=menv.BoundedActionSpec(1))
    model_fn = functools.partial(m, **ds.normalizers())
    assert fused.describe_model(model_fn) is not None
    kw = dict(num_candidates=256, seed=11)
    pol = MPCPolicy(model_fn, cost, RecedingHorizonCEMPlanner, sample_action, 10, **kw)
    batches = []
    rs = parallel.get_rollouts_parallel("linear", "run", True, 3, dict(num_steps=4, get_action=pol.get_action),
                                        num_workers=2, env_factory=se.make_env,
                                        on_batch=lambda i, o, a: batches.append((list(i), o, a)))
    assert all(idx == sorted(idx) for idx, _, _ in batches) and {i for idx, _, _ in batches for i in idx} == {0, 1, 2}
    answers = {i: [] for i in range(3)}
    last, memos = {}, {}
    warm_rounds = []
    for n, (idx, obs, acts) in enumerate(batches):
        inits = [None if not answers[i] else (last[i][0][1:], last[i][1][0:]) for i in idx]
        ms = [None if not answers[i] else memos[i] for i in idx]
        if all(x is not None for x in ms):
            warm_rounds.append(n)
        states, ref, new = RecedingHorizonCEMPlanner.plan_batch(obs, model_fn, cost, sample_action, 10,
                                                                initial_trajectories=inits, memos=ms, **kw)
        assert torch.equal(ref[:, 0].reshape(len(idx), -1), acts)
        for b, i in enumerate(idx):
            answers[i].append(acts[b])
            last[i] = (list(states[b].split(1, 0)), list(ref[b].split(1, 0)))
            memos[i] = new[b]
            assert new[b]["carry"].shape == (max(1, int(0.3 * 25)), 10, 1) and new[b]["sigma"].shape == (10, 1)
    assert len(warm_rounds) == len(batches) - 2          # (rollouts 0 and 1 start together, rollout 2 alone)
    # the memos mattered: a warm round planned cold gives other actions
    idx, obs, acts = batches[warm_rounds[0]]
    _, cold, _ = RecedingHorizonCEMPlanner.plan_batch(obs, model_fn, cost, sample_action, 10, **kw)
    assert not torch.equal(cold[:, 0].reshape(len(idx), -1), acts)
    for i, r in enumerate(rs):
        assert len(r) == 4
        assert all(torch.equal(torch.as_tensor(x).reshape(-1), y) for x, y in zip(r.actions[:-1], answers[i]))
