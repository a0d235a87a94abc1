"""GPU: coloured-noise proposals (csrc/cem_noise.hip: mbrl_sample_actions_mixed, mbrl_cem_plan_rh_mixed,
mbrl_cem_plan_rh_batch_mixed and their loops in plan.hip) and the planners' noise_beta / noise_mix kwargs,
against the NumPy restatement (tests/cem_rh_reference.py plan / mixed_actions; fixtures: tests/cem_noise_reference.py).

Bars: the mixed draw bit for bit; the plans at tests/test_gpu_cem_rh.py's bars -- costs within 1e-5 relative,
elite and best index sets identical (tests/test_cem_noise_host.py asserts the fixtures' return gaps), mu,
sigma, kept rows, carry and proposals bit for bit. An identity mix is the white plan (array_equal); a NULL mix
is the existing entry bit for bit."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import cem_noise_reference as nr
import cem_rh_batch_reference as br
import cem_rh_reference as rh
from oracle import cem as ocem

from test_gpu_cem_rh import _bits, _check_against_restatement, _dev, _params, c_plan_rh
from test_gpu_cem_rh_batch import assert_same_bits, c_plan_rh_batch, problem_of
from test_gpu_parity import build, device_problem

pytestmark = pytest.mark.gpu
F32 = np.float32
LO, HI = -1.0, 1.0
DEV = "cuda:0"
K, I = nr.SMALL["K"], nr.SMALL["I"]
PLAN_KEYS = ("mu", "sigma", "actions", "states", "costs", "returns", "elites")


def _dense_mix(H, seed=5):
    return np.random.default_rng(seed).normal(0.0, 1.0 / np.sqrt(H), (H, H)).astype(F32)


def c_sample_mixed(mu, sg, mix, H, a, N, n_offset, it, seed, misalign=False, expect=0):
    """mbrl_sample_actions_mixed through ctypes: the [H, N, a] draw as a host array. misalign: the output
    starts 4 bytes into its allocation (no 16-byte stores)."""
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    dev = torch.device(DEV)
    mu_d, sg_d = _dev(mu), _dev(sg)
    buf = torch.full((H * N * a + 1,), -7.0, dtype=torch.float32, device=dev)
    out = buf[1:] if misalign else buf[:-1]
    sp = fused.make_sampler(seed, it, mu_d, sg_d, LO, HI)
    rc = lib.mbrl_sample_actions_mixed(ctypes.byref(sp), _lib.ptr(_dev(mix)), H, a, N, n_offset, _lib.ptr(out),
                                       _lib.stream_handle(dev))
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool((buf == -7).all()), (rc, lib.mbrl_last_error())
        return None
    _lib.check(rc, "mbrl_sample_actions_mixed")
    guard = buf[0] if misalign else buf[-1]
    assert float(guard) == -7.0
    return out.cpu().numpy().reshape(H, N, a)


def _draw_case(H, a, N, off, it, mix, tag, misaligned=False):
    rng = np.random.default_rng(1000 * H + 10 * a + N % 7)
    mu = rng.uniform(-0.5, 0.5, (H, a)).astype(F32)
    sg = rng.uniform(0.1, 0.9, (H, a)).astype(F32)
    seed = 0x1234_5678_9ABC + a + it
    ref = nr.mixed_actions(mu, sg, LO, HI, seed, it, off + np.arange(N), mix)
    assert _bits(c_sample_mixed(mu, sg, mix, H, a, N, off, it, seed)) == _bits(ref), (tag, H, a, N, off, it)
    if misaligned:
        got = c_sample_mixed(mu, sg, mix, H, a, N, off, it, seed, misalign=True)
        assert _bits(got) == _bits(ref), (tag, H, a, N, off, it, "misaligned")


@pytest.mark.parametrize("H", [1, 2, 3, 20, 63, 64])
def test_mixed_draw_is_the_restatement_bit_for_bit(H):
    """The whole product a in {1, 5, 8, 48} x N in {1, 100, 1000} x n_offset in {0, 4099} x iteration in {0, 3},
    with a beta = 1 matrix; a random dense matrix at every a too (N = 100: the scalar and the 16-byte stores);
    a = 8 also from an output 4 bytes off its alignment (the scalar stores at a multiple of 4)."""
    beta, dense = nr.beta_mix(H), _dense_mix(H)
    for a in (1, 5, 8, 48):
        for N, off, it in itertools.product((1, 100, 1000), (0, 4099), (0, 3)):
            _draw_case(H, a, N, off, it, beta, "beta", misaligned=(a == 8 and off == 0))
        _draw_case(H, a, 100, 4099, 3, dense, "dense", misaligned=(a == 8))


def test_every_offset_and_iteration_pairing_of_the_draw():
    H, a, N = 20, 5, 100
    mix = nr.beta_mix(H)
    mu, sg = np.zeros((H, a), F32), np.full((H, a), 0.5, F32)
    for off, it in itertools.product((0, 4099), (0, 3)):
        ref = nr.mixed_actions(mu, sg, LO, HI, 11, it, off + np.arange(N), mix)
        assert _bits(c_sample_mixed(mu, sg, mix, H, a, N, off, it, 11)) == _bits(ref), (off, it)


def _tile_width(pairs):
    """csrc/cem_noise.hip noise_launch's pairs per tile on this device, restated."""
    want = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    return 64 if pairs >= 64 * want else (32 if pairs >= 32 * want else 16)


@pytest.mark.parametrize("H,a,N,P,lds_kib,tiles_per_group", [
    (20, 5, 8200, 32, 11.6, 1),      # 16400 pairs: 32-pair tiles, the scalar stores
    (20, 8, 8197, 32, 11.6, 1),      # 16394 pairs: 32-pair tiles, 16-byte stores, a partial last tile
    (64, 48, 2735, 64, 80.0, 1),     # 32820 pairs: 64-pair tiles at the H limit, 80 KiB of LDS (raised limit), partial
    (50, 21, 5462, 64, 59.8, 1),     # 32772 pairs: humanoid's H and a on 64-pair tiles
    (2, 48, 60000, 64, 2.0, 2),      # 720000 pairs: 11250 tiles on the 8192-workgroup grid, 3058 workgroups run two
], ids=["P32-scalar", "P32-vector-partial", "P64-H64-80KiB", "P64-humanoid", "two-tiles-per-workgroup"])
def test_wide_tiles_and_the_tile_loop_are_the_restatement_bit_for_bit(H, a, N, P, lds_kib, tiles_per_group):
    """The tile widths and launch shapes the small grid above never reaches (it runs 16-pair tiles, one per
    workgroup): 32- and 64-pair tiles with their row strides of 8 and 4, the dynamic-LDS limit raised above
    64 KiB, and workgroups that own more than one tile. The expected configuration is asserted from the
    launcher's rule on this device, so the case cannot silently fall back to 16-pair tiles."""
    pairs = N * ((a + 3) // 4)
    assert _tile_width(pairs) == P, (pairs, _tile_width(pairs))
    assert abs((4 * ((H * H + 3) & ~3) + 16 * H * P) / 1024 - lds_kib) < 0.06
    assert (-(-pairs // P) > 8192) == (tiles_per_group > 1)
    _draw_case(H, a, N, 4099, 3, nr.beta_mix(H), f"P={P}", misaligned=(a == 8))


def test_null_mix_is_the_white_draw_and_a_long_horizon_is_refused():
    from mbrl_amd import _lib, fused
    H, a, N = 20, 8, 100
    mu, sg = np.zeros((H, a), F32), np.full((H, a), 0.5, F32)
    white = torch.empty((H, N, a), dtype=torch.float32, device=DEV)
    fused.sample_actions(fused.make_sampler(3, 1, _dev(mu), _dev(sg), LO, HI), H, a, N, 7, white)
    assert _bits(c_sample_mixed(mu, sg, None, H, a, N, 7, 1, 3)) == _bits(white)
    assert _bits(c_sample_mixed(mu, sg, np.eye(H, dtype=F32), H, a, N, 7, 1, 3)) == _bits(white)
    mu, sg = np.zeros((65, a), F32), np.full((65, a), 0.5, F32)
    c_sample_mixed(mu, sg, np.eye(65, dtype=F32), 65, a, N, 0, 0, 3, expect=_lib.MBRL_EUNSUPPORTED)


def c_plan_mixed(prob, p, N, H, K, I, mix, keep=0, init_mu_rows=None, init_sigma_rows=None, carry_in=None,
                 record=True, expect=0, ws_bytes=None, null=(), make_ws=None, alloc=None):
    """mbrl_cem_plan_rh_mixed through ctypes (c_plan_rh's shapes; the proposals of the last iteration are not
    recorded by the ABI). With `expect` nonzero: asserts that code and that nothing was written. make_ws(nbytes) -> the uint8 workspace and
    alloc(*shape, dt=) -> an output tensor replace the private allocations (tests/workspace_cases.py)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    md = prob.mdesc
    a, s, E = md["a"], md["s"], md["E"]
    params = _params(p, N, H, K, I, keep)
    need = lib.mbrl_cem_rh_mixed_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), 1)
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
    g = lambda k: None if k in null else _lib.ptr(out.get(k))  # noqa: E731
    s0 = _dev(p["s0"])
    ins = [_dev(init_mu_rows), _dev(init_sigma_rows), _dev(carry_in), _dev(mix)]
    refs = list(prob.refs)
    if "packed" in null:
        refs[1] = None
    rc = lib.mbrl_cem_plan_rh_mixed(*refs, None if "s0" in null else _lib.ptr(s0), ctypes.byref(params),
                                    *[_lib.ptr(x) for x in ins], g("mu"), g("sigma"), g("actions"), g("states"),
                                    g("carry"), g("carry_returns"), g("costs"), g("returns"), g("elites"),
                                    g("kept_hist"), None, None if "workspace" in null else _lib.ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, lib.mbrl_last_error())
        for k, v in out.items():
            assert bool((v == -7).all()), k
        return None
    _lib.check(rc, "mbrl_cem_plan_rh_mixed")
    return out


@pytest.mark.parametrize("case", nr.CASES, ids=nr.case_id)
def test_mixed_plan_against_the_restatement(case):
    W, L, a, N, E, Kc, inputs, H, _ = case
    p, mix, kw = nr.make_case(case)
    ref = nr.cached(nr.case_plan, case, final=True)
    got = c_plan_mixed(device_problem(p), p, N, H, K, I, mix, **kw)
    _check_against_restatement(got, ref, I, K, Kc, nr.case_id(case))
    # the proposals themselves, bit for bit: every iteration's, redrawn from the restatement's distribution
    mus, sgs = [ref["mu0"]] + ref["mu"][:-1], [ref["sigma0"]] + ref["sigma"][:-1]
    for it in range(I):
        drawn = c_sample_mixed(mus[it], sgs[it], mix, H, a, N, 0, it, p["rng_seed"])
        slots = Kc if (it > 0 or "carry" in inputs) else 0
        assert _bits(drawn[:, slots:]) == _bits(ref["actions"][it][:, slots:]), (nr.case_id(case), it)


def _cross_problem(a=5, N=100, H=12, seed=7601):
    return ocem.synth_problem(2, seed=seed, W=64, L=1, a=a, N=N, H=H)


def _inputs(keep, H, a, seed=3):
    rng = np.random.default_rng(seed)
    kw = dict(init_mu_rows=rng.uniform(-1.3, 1.3, (H, a)).astype(F32),
              init_sigma_rows=rng.uniform(0.1, 0.6, (H, a)).astype(F32))
    if keep:
        kw["carry_in"] = rng.uniform(-1.2, 1.2, (keep, H, a)).astype(F32)
    return kw


@pytest.mark.parametrize("a", [5, 8], ids=["scalar", "vector"])
@pytest.mark.parametrize("keep", [0, 3])
def test_identity_and_null_mix_are_the_white_plan(keep, a):
    """Identity mix: array_equal to mbrl_cem_plan_rh (keep > 0: outputs, carry and records) and, with keep == 0
    and no rows, to mbrl_cem_plan. NULL mix: mbrl_cem_plan_rh bit for bit (forwarded)."""
    N, H = 100, 12
    p = _cross_problem(a, N, H)
    prob = device_problem(p)
    kw = _inputs(keep, H, a)
    white = c_plan_rh(prob, p, N, H, K, I, keep=keep, **kw)
    ident = c_plan_mixed(prob, p, N, H, K, I, np.eye(H, dtype=F32), keep=keep, **kw)
    null = c_plan_mixed(prob, p, N, H, K, I, None, keep=keep, **kw)
    for k in white:
        assert torch.equal(white[k], ident[k]), k
    assert_same_bits(null, white, "NULL mix")
    if keep == 0:
        from mbrl_amd import CEMPlanner
        _, model_fn, cost_fn, sample_action = build(p)
        plain = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H,
                                         num_candidates=N, num_elites=K, num_iterations=I, seed=p["rng_seed"],
                                         record=True, return_device=True)
        cold = c_plan_mixed(prob, p, N, H, K, I, np.eye(H, dtype=F32), keep=0)
        for k in PLAN_KEYS:
            assert torch.equal(plain[k], cold[k]), k


def test_mixed_plan_equals_its_step_by_step_equivalent():
    """keep = 0, I = 2: mbrl_sample_actions_mixed -> mbrl_rollout_cost -> mbrl_select_elites -> the refit of the
    gathered rows (oracle.cem.refit over the drawn rows: the refit kernel is bit-exact to it), bit for bit."""
    from mbrl_amd import fused
    N, H, a, I2 = 100, 12, 5, 2
    p = _cross_problem(a, N, H)
    prob = device_problem(p)
    mix = nr.beta_mix(H)
    got = c_plan_mixed(prob, p, N, H, K, I2, mix, keep=0)
    mu, sg = np.zeros((H, a), F32), np.full((H, a), 0.5, F32)
    s0 = _dev(p["s0"])
    for it in range(I2):
        A = c_sample_mixed(mu, sg, mix, H, a, N, 0, it, p["rng_seed"])
        A_d = _dev(A)
        costs = fused.rollout(prob, s0, N, H, actions=A_d)
        assert torch.equal(costs, got["costs"][it]), it
        rets = torch.empty(N, dtype=torch.float32, device=DEV)
        elites = fused.select(costs, K, returns_out=rets)
        assert torch.equal(elites, got["elites"][it]) and torch.equal(rets, got["returns"][it]), it
        el = elites.cpu().numpy()
        mu, sg = ocem.refit(mu, sg, np.ascontiguousarray(A[:, el, :].transpose(1, 0, 2)), 0.1)
    assert _bits(got["mu"]) == _bits(mu) and _bits(got["sigma"]) == _bits(sg)


def test_a_kept_optimum_survives_the_mixed_plan():
    N, H, Kc = 64, 3, 3
    p = ocem.synth_problem(2, seed=7110, W=64, L=1, a=5, N=N, H=H)
    mix = nr.beta_mix(H)
    cold = rh.plan(p, N, H, K, 5, keep=1, final=False)
    opt = cold["carry"][0]
    rng = np.random.default_rng(1)
    carry_in = np.concatenate([opt[None], rng.uniform(-1, 1, (Kc - 1, H, 5)).astype(F32)], 0)
    ref = nr.plan(p, N, H, K, I, mix=mix, keep=Kc, carry_in=carry_in)
    assert rh.case_gaps(ref, K, Kc) > nr.GAP_MIN
    got = c_plan_mixed(device_problem(p), p, N, H, K, I, mix, keep=Kc, carry_in=carry_in)
    _check_against_restatement(got, ref, I, K, Kc, "kept optimum, mixed")
    assert 0 in got["elites"][0].cpu().numpy()
    assert any(_bits(row) == _bits(opt) for row in got["carry"].cpu().numpy())
    assert float(got["carry_returns"].min()) <= float(got["returns"][0][0])


def test_a_nan_kept_row_sorts_last_in_the_mixed_plan():
    N, H, Kc = 64, 3, 3
    p = ocem.synth_problem(2, seed=7101, W=64, L=1, a=5, N=N, H=H)
    mix = nr.beta_mix(H)
    rng = np.random.default_rng(2)
    carry_in = rng.uniform(-1, 1, (Kc, H, 5)).astype(F32)
    carry_in[1, 2, 3] = np.nan
    ref = nr.plan(p, N, H, K, I, mix=mix, keep=Kc, carry_in=carry_in)
    assert np.isnan(ref["returns"][0][1]) and np.isfinite(np.delete(ref["returns"][0], 1)).all()
    got = c_plan_mixed(device_problem(p), p, N, H, K, I, mix, keep=Kc, carry_in=carry_in)
    r0 = got["returns"][0].cpu().numpy()
    assert np.isnan(r0[1]) and np.isfinite(np.delete(r0, 1)).all()
    assert 1 not in got["elites"][0].cpu().numpy()
    assert np.array_equal(ocem.select_elites(r0, Kc), ref["best"][0]) and 1 not in ref["best"][0]
    kept = got["kept_hist"].cpu().numpy()
    assert _bits(kept[0]) == _bits(carry_in)
    assert np.isfinite(kept[1:]).all() and np.isfinite(got["carry"].cpu().numpy()).all()
    assert _bits(got["mu"]) == _bits(ref["mu_out"]) and _bits(got["carry"]) == _bits(ref["carry"])


def c_plan_batch_mixed(prob, p, s0s, N, H, K, I, mix, keep=0, ins=None, record=True, expect=0, ws_bytes=None,
                       make_ws=None, alloc=None):
    """mbrl_cem_plan_rh_batch_mixed through ctypes (c_plan_rh_batch's shapes; make_ws / alloc as c_plan_rh's)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    md = prob.mdesc
    a, s, E = md["a"], md["s"], md["E"]
    B = len(s0s)
    params = _params(p, N, H, K, I, keep)
    need = lib.mbrl_cem_rh_mixed_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), B)
    dev = torch.device(DEV)
    ws = make_ws(need) if make_ws else torch.empty(max(need if ws_bytes is None else ws_bytes, 256), dtype=torch.uint8,
                                                   device=dev)
    e = alloc or (lambda *sh, dt=torch.float32: torch.full(sh, -7, dtype=dt, device=dev))  # noqa: E731
    out = dict(mu=e(B, H, a), sigma=e(B, H, a), actions=e(B, H, a), states=e(B, H, s))
    if keep:
        out.update(carry=e(B, keep, H, a), carry_returns=e(B, keep))
    if record:
        out.update(costs=e(I, E, B * N), returns=e(I, B, N), elites=e(I, B, K, dt=torch.int64))
        if keep:
            out.update(kept_hist=e(I + 1, B, keep, H, a))
    g = lambda k: _lib.ptr(out.get(k))  # noqa: E731
    ins = ins or {}
    s0 = _dev(np.asarray(s0s, F32))
    fl = ins.get("flags")
    fl_d = None if fl is None else torch.from_numpy(np.ascontiguousarray(fl, dtype=np.int32)).to(DEV)
    ptrs = [_dev(ins.get(k)) for k in ("init_mu_rows", "init_sigma_rows", "carry_in")]
    rc = lib.mbrl_cem_plan_rh_batch_mixed(*prob.refs, _lib.ptr(s0), B, ctypes.byref(params),
                                          *[_lib.ptr(x) for x in ptrs], _lib.ptr(fl_d), _lib.ptr(_dev(mix)), g("mu"),
                                          g("sigma"), g("actions"), g("states"), g("carry"), g("carry_returns"),
                                          g("costs"), g("returns"), g("elites"), g("kept_hist"), _lib.ptr(ws),
                                          ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, lib.mbrl_last_error())
        for k, v in out.items():
            assert bool((v == -7).all()), k
        return None
    _lib.check(rc, "mbrl_cem_plan_rh_batch_mixed")
    return out


@pytest.mark.parametrize("case", nr.BATCH_CASES, ids=nr.batch_case_id)
def test_mixed_batch_against_the_restatement(case):
    W, L, a, N, E, Kc, inputs, H, _ = case
    p, s0s, mix, kws = nr.make_batch_case(case)
    refs = nr.cached(nr.batch_case_plans, case, final=True)
    got = c_plan_batch_mixed(device_problem(p), p, s0s, N, H, K, I, mix, keep=Kc, ins=br.stack_inputs(kws, H, a, Kc))
    for b, ref in enumerate(refs):
        _check_against_restatement(problem_of(got, b, N), ref, I, K, Kc, f"{nr.batch_case_id(case)} problem {b}")


def test_mixed_batch_on_32_pair_tiles_against_the_restatement():
    """B N ceil(a / 4) = 20480 pairs: the first launch and every draw take 32-pair tiles, 640 of them."""
    case = nr.WIDE_BATCH_CASE
    W, L, a, N, E, Kc, inputs, H, _ = case
    assert _tile_width(len(inputs) * N * ((a + 3) // 4)) == 32
    p, s0s, mix, kws = nr.make_batch_case(case)
    refs = nr.cached(nr.batch_case_plans, case, final=True)
    got = c_plan_batch_mixed(device_problem(p), p, s0s, N, H, K, I, mix, keep=Kc, ins=br.stack_inputs(kws, H, a, Kc))
    for b, ref in enumerate(refs):
        _check_against_restatement(problem_of(got, b, N), ref, I, K, Kc, f"{nr.batch_case_id(case)} problem {b}")


@pytest.mark.parametrize("keep", [0, 3])
def test_one_problem_and_problem_zero_are_the_single_mixed_plan(keep):
    N, H, a = 100, 12, 8
    p = _cross_problem(a, N, H)
    prob = device_problem(p)
    mix = nr.beta_mix(H)
    rng = np.random.default_rng(9)
    s0s = np.stack([p["s0"]] + [(p["s0"] + rng.normal(0, 0.2, 5)).astype(F32) for _ in range(2)])
    kws = [_inputs(keep, H, a, seed=20 + b) for b in range(3)]
    single = c_plan_mixed(prob, p, N, H, K, I, mix, keep=keep, **kws[0])
    one = c_plan_batch_mixed(prob, p, s0s[:1], N, H, K, I, mix, keep=keep, ins=br.stack_inputs(kws[:1], H, a, keep))
    assert_same_bits(problem_of(one, 0, N), single, "B=1")
    three = c_plan_batch_mixed(prob, p, s0s, N, H, K, I, mix, keep=keep, ins=br.stack_inputs(kws, H, a, keep))
    assert_same_bits(problem_of(three, 0, N), single, "B=3 problem 0")
    # a NULL mix is the existing batched entry, bit for bit
    white = c_plan_rh_batch(prob, p, s0s, N, H, K, I, keep=keep, ins=br.stack_inputs(kws, H, a, keep))
    null = c_plan_batch_mixed(prob, p, s0s, N, H, K, I, None, keep=keep, ins=br.stack_inputs(kws, H, a, keep))
    assert_same_bits(null, white, "NULL mix batch")


def _planner_problem(N=64, H=12, a=5):
    p = ocem.synth_problem(2, seed=7602, W=64, L=1, a=a, N=N, H=H)
    _, model_fn, cost_fn, sample_action = build(p)
    return p, model_fn, cost_fn, sample_action


def test_planner_kwargs_equal_the_c_level_calls():
    from mbrl_amd import CEMPlanner, RecedingHorizonCEMPlanner
    from mbrl_amd.planners import colored_noise_mix
    N, H, a = 64, 12, 5
    p, model_fn, cost_fn, sample_action = _planner_problem(N, H, a)
    prob = device_problem(p)
    mix = colored_noise_mix(H, 1.0)
    s0 = torch.from_numpy(p["s0"])
    kw = dict(num_candidates=N, num_elites=K, num_iterations=I, seed=p["rng_seed"], record=True, return_device=True)
    want = c_plan_mixed(prob, p, N, H, K, I, mix, keep=0)
    for noise in (dict(noise_beta=1.0), dict(noise_mix=mix)):
        res = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, **noise, **kw)
        for k in PLAN_KEYS:
            assert torch.equal(res[k], want[k]), (k, noise.keys())
    res = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, noise_beta=1.0, keep_elites=3, **kw)
    want3 = c_plan_mixed(prob, p, N, H, K, I, mix, keep=3)
    for k in PLAN_KEYS + ("carry", "carry_returns", "kept_hist"):
        assert torch.equal(res[k], want3[k]), k
    # defaults (and noise_beta = 0) are the plain plan bit for bit
    plain = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, **kw)
    zero = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, noise_beta=0.0, noise_mix=None, **kw)
    for k in PLAN_KEYS:
        assert torch.equal(plain[k], zero[k]), k
    assert not torch.equal(plain["actions"], want["actions"])
    # the batched planner: B = 2 first control steps (no memos), keep_elites resolved from its default fraction
    s0s = torch.stack([s0, s0 + 0.1])
    bkw = dict(num_candidates=N, num_elites=K, num_iterations=I, seed=p["rng_seed"], return_device=True)
    st, ac, memos = RecedingHorizonCEMPlanner.plan_batch(s0s, model_fn, cost_fn, sample_action, H, noise_beta=1.0, **bkw)
    Kc = max(1, int(0.3 * K))
    wantb = c_plan_batch_mixed(prob, p, s0s.numpy(), N, H, K, I, mix, keep=Kc, record=False)
    assert torch.equal(ac, wantb["actions"]) and torch.equal(st, wantb["states"])
    assert torch.equal(memos[1]["carry"], wantb["carry"][1].cpu())
    st0, ac0, _ = RecedingHorizonCEMPlanner.plan_batch(s0s, model_fn, cost_fn, sample_action, H, **bkw)
    whiteb = c_plan_rh_batch(prob, p, s0s.numpy(), N, H, K, I, keep=Kc, record=False)
    assert torch.equal(ac0, whiteb["actions"]) and not torch.equal(ac0, ac)


def test_generic_path_refuses_the_noise_kwargs():
    from mbrl_amd import CEMPlanner, fused
    p, model_fn, cost_fn, sample_action = _planner_problem()
    wrapped = lambda s, a: model_fn(s, a)  # noqa: E731
    assert fused.describe_model(wrapped) is None
    s0 = torch.from_numpy(p["s0"])
    with pytest.raises(NotImplementedError, match="noise_beta"):
        CEMPlanner.plan(s0, wrapped, cost_fn, sample_action, 12, num_candidates=64, seed=1, noise_beta=1.0)
    with pytest.raises(NotImplementedError, match="noise_mix"):
        CEMPlanner.plan(s0, wrapped, cost_fn, sample_action, 12, num_candidates=64, seed=1,
                        noise_mix=np.eye(12, dtype=F32))


@pytest.mark.parametrize("what", ["null_outputs", "null_packed", "null_s0", "null_workspace", "H=65",
                                  "workspace_one_byte_short", "carry_without_keep"])
def test_argument_checks_return_before_any_launch(what):
    from mbrl_amd import _lib
    lib = _lib.load()
    N, H = 64, 12
    p = _cross_problem(5, N, H)
    prob = device_problem(p)
    mix = nr.beta_mix(H)
    if what.startswith("null_"):
        c_plan_mixed(prob, p, N, H, K, 2, mix, null=({"outputs": ("actions", "states")}.get(what[5:], (what[5:],))),
                     expect=_lib.MBRL_EINVAL)
    elif what == "H=65":
        p65 = ocem.synth_problem(2, seed=7601, W=64, L=1, a=5, N=N, H=65)
        params = _params(p65, N, 65, K, 2, 0)
        assert lib.mbrl_cem_rh_mixed_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), 1) == 0
        c_plan_mixed(prob, p65, N, 65, K, 2, np.eye(65, dtype=F32), expect=_lib.MBRL_EUNSUPPORTED, ws_bytes=1 << 22)
        s0s = np.stack([p65["s0"]] * 2)
        c_plan_batch_mixed(prob, p65, s0s, N, 65, K, 2, np.eye(65, dtype=F32), expect=_lib.MBRL_EUNSUPPORTED,
                           ws_bytes=1 << 23)
    elif what == "workspace_one_byte_short":
        for keep in (0, 3):
            params = _params(p, N, H, K, 2, keep)
            need = lib.mbrl_cem_rh_mixed_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), 2)
            assert need > lib.mbrl_cem_rh_batch_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), 2) \
                or keep > 0
            c_plan_batch_mixed(prob, p, np.stack([p["s0"]] * 2), N, H, K, 2, mix, keep=keep,
                               expect=_lib.MBRL_EWORKSPACE, ws_bytes=need - 1)
            need1 = lib.mbrl_cem_rh_mixed_workspace_bytes(ctypes.byref(prob.shape), ctypes.byref(params), 1)
            c_plan_mixed(prob, p, N, H, K, 2, mix, keep=keep, expect=_lib.MBRL_EINVAL, ws_bytes=need1 - 1)
    else:
        c_plan_mixed(prob, p, N, H, K, 2, mix, keep=0, carry_in=np.zeros((1, H, 5), F32), expect=_lib.MBRL_EINVAL)
        c_plan_batch_mixed(prob, p, np.stack([p["s0"]] * 2), N, H, K, 2, mix, keep=0,
                           ins=dict(carry_in=np.zeros((2, 1, H, 5), F32)), expect=_lib.MBRL_EINVAL)
