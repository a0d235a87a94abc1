"""GPU: the split-operand rollout (precision F16X3 / F16X6, csrc/rollout_f16x3.hip) over its whole shape
envelope -- every case of tests/split_cases.py, which tests/test_rollout_dispatch_model.py proves to reach
each of the 24 reachable instantiations of rollout_split_kernel, both tile heights, every depth, padded
widths, every action slot and the parity-bumped layer-0 chunk.

An accepted case meets the suite's fp32 bars against the float32 oracle (returns within RTOL, states within
rtol = atol = 1e-4) and, against the float64 rollout,

    e(gpu) <= bar_P(case) = K_P x max(e32(case), median e32),     e(x) = max |x - x64| / max |x64|,

with K_P from split_cases.py: the bar is the float32 oracle's own distance to float64 and a factor measured on
the CPU from an emulation of the split arithmetic, never the kernel's output. tests/test_split_host.py shows
that an F16X3 kernel without x0 w1 or x1 w0 misses every case's bar tenfold. Its states must also differ in
bits from the F32 problem's: the split kernel ran. A declined case must be the F32 problem's result bit for
bit. The third-piece cases hold F16X6 (and F32) to 2 ulp of float64 where F16X3 is hundreds of ulp away; the
per-member and per-tile redo paths are checked to hand exactly the flagged member or tile to the fp32 kernel.
Every printed line gives the case, e(gpu), e32, their ratio and the bar.

On the MI355X the table's worst e(gpu) / e32 is 1.83 (c11_t4_l1, F16X3) and the range-edge tile's 2.36, against
bars of 8 x. The cases c11_t4_l1 and c11_t4_l1_r2 (L = 1 at T = 4, H = 3) are the ones that found the weight
ring's prefetch reading past a two-slot step (rollout_f16x3.hip load_slot): returns off by 2.7 % before the fix."""
import functools

import numpy as np
import pytest
import torch

import split_cases as sc
import split_reference as sref
from oracle import cem as ocem
from oracle.philox import cem_actions
from test_gpu_flags import device_problem
from test_gpu_parity import DEV, RTOL, rel_err

pytestmark = pytest.mark.gpu
PRECISIONS = {"f16x3": 2, "f16x6": 3}
REDO_MARK = 0x7FC0DEAD
ACC_IDS = [c.id for c in sc.ACCEPTED]
R2_IDS = [c.id for c in sc.ACCEPTED if c.id in sc.TILE32 and sc.outcome(c, 2).R == 2]


def run(prob, p, s0, A, H, N, tile=0, sampled=False):
    """mbrl_rollout_cost on (s0, A) under MBRL_OPT_SPLIT_TILE = tile: (costs [E, N], states [E, H, N, s]) as
    NumPy. sampled: the call draws the actions itself (at SAMPLE_OFFSET) and must draw exactly A."""
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    E, s, a = p["cfg"]["E"], p["cfg"]["s"], p["cfg"]["a"]
    s0_d = torch.from_numpy(np.array(s0)).to(DEV)
    costs = torch.full((E, N), float("nan"), dtype=torch.float32, device=DEV)
    states = torch.full((E, H, N, s), float("nan"), dtype=torch.float32, device=DEV)
    acts = torch.from_numpy(np.array(A)).to(DEV)
    stream = _lib.stream_handle(torch.device(DEV))
    with _lib.option("split_tile", tile):
        if sampled:
            mu, sg = sc.sampled_distribution(H, a)
            mu_d, sg_d = torch.from_numpy(mu).to(DEV), torch.from_numpy(sg).to(DEV)
            sp = fused.make_sampler(p["rng_seed"], 1, mu_d, sg_d, -1.0, 1.0)
            drawn = torch.full((H, N, a), float("nan"), dtype=torch.float32, device=DEV)
            rcode = lib.mbrl_rollout_cost(*prob.refs, _lib.ptr(s0_d), int(s0.ndim == 2), None, fused.ctypes_ref(sp), N, H,
                                          sc.SAMPLE_OFFSET, _lib.ptr(costs), _lib.ptr(drawn), _lib.ptr(states), stream)
        else:
            rcode = lib.mbrl_rollout_cost(*prob.refs, _lib.ptr(s0_d), int(s0.ndim == 2), _lib.ptr(acts), None, N, H, 0,
                                          _lib.ptr(costs), None, _lib.ptr(states), stream)
        _lib.check(rcode, "mbrl_rollout_cost")
        torch.cuda.synchronize()
    if sampled:
        assert np.array_equal(drawn.cpu().numpy(), A), "the in-call draw at n_offset"
    return costs.cpu().numpy(), states.cpu().numpy()


@functools.lru_cache(maxsize=None)
def f32_result(cid):
    """The F32 problem's (costs, states) of a table case: what a declined shape must reproduce."""
    c, p = sc.by_id(cid), sc.problem(cid)
    s0, A = sc.inputs(cid)
    return run(device_problem(p), p, s0, A, c.H, c.N, 0, c.mode == "sampled")


def check_bar(what, states, s64, e32, bar):
    e = sref.err(states, s64)
    print(f"{what}: e(gpu) {e:.3e}, e32 {e32:.3e}, ratio {e / e32 if e32 else float('inf'):.2f}, bar {bar:.3e}")
    assert np.all(np.isfinite(states))
    assert e <= bar, f"{what}: e(gpu) = {e:.3e} > bar = {bar:.3e}"


def check_case(cid, precision, costs, states, what):
    c32, s32, s64 = sc.reference(cid)
    assert rel_err(costs, c32) < RTOL, (cid, precision, rel_err(costs, c32))
    assert np.allclose(states, s32, rtol=1e-4, atol=1e-4), (cid, precision)
    assert not np.any(costs.view(np.uint32) == REDO_MARK)
    check_bar(f"{cid} {precision} {what}", states, s64, sc.e32(cid), sc.bar(cid, PRECISIONS[precision]))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cid", ACC_IDS)
def test_accepted_case_meets_the_split_bar(cid, precision):
    c, p = sc.by_id(cid), sc.problem(cid)
    out = sc.outcome(c, PRECISIONS[precision])
    assert out.kind == "split"
    s0, A = sc.inputs(cid)
    costs, states = run(device_problem(p, precision), p, s0, A, c.H, c.N, sc.tile_of(c), c.mode == "sampled")
    check_case(cid, precision, costs, states, "T=%d R=%d K0S=%d NOS=%d TS=%d" % (out.T, out.R, out.K0S, out.NOS, out.TS))
    assert not np.array_equal(states, f32_result(cid)[1]), "the fp32 kernel's bits: rollout_split_kernel did not run"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cid", R2_IDS)
def test_both_tile_heights_meet_the_bar(cid, precision):
    """split_tile 16 and 32 on the R = 2 cases (their summation orders may differ: no bit equality asked)."""
    c, p = sc.by_id(cid), sc.problem(cid)
    s0, A = sc.inputs(cid)
    prob = device_problem(p, precision)
    for tile in (16, 32):
        costs, states = run(prob, p, s0, A, c.H, c.N, tile, c.mode == "sampled")
        check_case(cid, precision, costs, states, f"split_tile={tile}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cid", [c.id for c in sc.DECLINED])
def test_declined_case_is_the_f32_problem_bit_for_bit(cid, precision):
    from mbrl_amd import _lib
    c, p = sc.by_id(cid), sc.problem(cid)
    assert sc.outcome(c, PRECISIONS[precision]).kind == "f32"
    s0, A = sc.inputs(cid)
    if cid in sc.REFUSED:           # no kernel takes the shape: the same refusal at either precision
        for prec in ("f32", precision):
            with pytest.raises(RuntimeError, match="too large"):
                run(device_problem(p, prec), p, s0, A, c.H, c.N, sc.tile_of(c))
            assert _lib.load().mbrl_last_error().decode()
        return
    costs, states = run(device_problem(p, precision), p, s0, A, c.H, c.N, sc.tile_of(c), c.mode == "sampled")
    c32, s32 = f32_result(cid)
    assert np.array_equal(costs.view(np.int32), c32.view(np.int32)) and np.array_equal(states.view(np.int32), s32.view(np.int32))
    ref_c, ref_s, _ = sc.reference(cid)
    assert rel_err(costs, ref_c) < RTOL and np.allclose(states, ref_s, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ third piece
@pytest.mark.parametrize("name", sc.THIRD)
def test_third_piece_is_carried_by_f16x6_and_lost_by_f16x3(name):
    p, s0, A = sc.third_problem(name)
    _, _, s64 = sc.third_reference(name)
    got = {}
    for precision in ("f32", "f16x6", "f16x3"):
        got[precision] = run(device_problem(p, precision), p, s0, A, 1, sc.N)[1]
        print(f"third piece {name} {precision}: {sref.ulps(got[precision], s64):.1f} ulp of float64, "
              f"e {sref.err(got[precision], s64):.3e}")
    assert sref.ulps(got["f32"], s64) <= sc.THIRD_ULPS
    assert sref.ulps(got["f16x6"], s64) <= sc.THIRD_ULPS
    assert sref.ulps(got["f16x3"], s64) > sc.THIRD_ULPS
    check_bar(f"third piece {name} f16x3", got["f16x3"], s64, 0.0, sc.third_bar(name, 2))


# ------------------------------------------------------------------------------------------------ redo paths
def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_out_of_range_weight_flags_its_member_alone(precision):
    """E = 3, one weight of member 1 at 40000: the pack flags member 1's stream, whose candidates the fp32 redo
    pass computes (bit for bit the F32 problem's), while members 0 and 2 stay in the split kernel."""
    H = 2
    p = ocem.synth_problem(3, N=sc.N, H=H, E=3, L=2)
    p["model"][1][1][0][7, 11] = 40000.0
    a = p["cfg"]["a"]
    A = cem_actions(np.zeros((H, a), np.float32), np.full((H, a), 0.5, np.float32), -1, 1, 9, 0, np.arange(sc.N))
    c32, s32 = run(device_problem(p), p, p["s0"], A, H, sc.N)
    costs, states = run(device_problem(p, precision), p, p["s0"], A, H, sc.N)
    assert not np.any(costs.view(np.uint32) == REDO_MARK)
    assert np.array_equal(_bits(costs[1]), _bits(c32[1])) and np.array_equal(_bits(states[1]), _bits(s32[1]))
    _, s64 = sref.rollout_f64(p, A)
    _, o32 = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A, store_states=True)
    for e in (0, 2):
        base = max(sref.err(o32[e], s64[e]), sc.median_e32())
        check_bar(f"member {e} {precision}", states[e], s64[e], sref.err(o32[e], s64[e]), sc.K_BAR[PRECISIONS[precision]] * base)
        assert not np.array_equal(_bits(states[e]), _bits(s32[e])), f"member {e} left the split kernel"


def _edge_check(p, s0, A, H, precision, hot_tile, what):
    """hot_tile None: every tile stays in the split kernel. Else that 16-candidate tile, and only it, holds the
    F32 problem's bits."""
    c32, s32 = run(device_problem(p), p, s0, A, H, sc.N)
    costs, states = run(device_problem(p, precision), p, s0, A, H, sc.N)
    assert not np.any(costs.view(np.uint32) == REDO_MARK)
    _, s64 = sref.rollout_f64(p, A, s0)
    _, o32 = ocem.rollout(p["model"], p["norm"], p["cost"], s0, A, store_states=True)
    for tile in range((sc.N + 15) // 16):
        rows = slice(16 * tile, min(16 * tile + 16, sc.N))
        same = np.array_equal(_bits(states[:, :, rows]), _bits(s32[:, :, rows]))
        if tile == hot_tile:
            assert same and np.array_equal(_bits(costs[:, rows]), _bits(c32[:, rows])), f"{what}: tile {tile} not redone in fp32"
        else:
            assert not same, f"{what}: tile {tile} left the split kernel"
            e32 = sref.err(o32[:, :, rows], s64[:, :, rows])
            check_bar(f"{what} {precision} tile {tile}", states[:, :, rows], s64[:, :, rows], e32,
                      sc.K_BAR[PRECISIONS[precision]] * max(e32, sc.median_e32()))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
def test_activation_range_edge(over, precision):
    """A start state of candidate 20 that normalises to just under 2048 stays in the split kernel; just over,
    its 16-candidate tile (candidates 16..31) and only that tile is the F32 result."""
    H = 2
    p = ocem.synth_problem(3, N=sc.N, H=H, L=2)
    a, nm = p["cfg"]["a"], p["norm"]
    A = cem_actions(np.zeros((H, a), np.float32), np.full((H, a), 0.5, np.float32), -1, 1, 5, 0, np.arange(sc.N))
    s0 = np.tile(p["s0"], (sc.N, 1)).astype(np.float32)
    target = np.float32(2048.5 if over else 2047.5)
    s0[20, 3] = target * nm["obs_std"][3] + nm["obs_mean"][3]
    z = np.float32((s0[20, 3] - nm["obs_mean"][3]) / nm["obs_std"][3])
    assert (z >= 2048) == over and abs(float(z) - 2048) < 1, z
    _edge_check(p, s0, A, H, precision, 1 if over else None, f"activation {float(z):.2f}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
def test_weight_range_edge(over, precision):
    """A layer-1 weight just under 128 stays in the split kernel; 128 itself hands every tile to the fp32 kernel."""
    H = 2
    p = ocem.synth_problem(3, N=sc.N, H=H, L=2)
    p["model"][0][1][0][7, 11] = np.float32(128.0) if over else np.nextafter(np.float32(128.0), np.float32(0))
    a = p["cfg"]["a"]
    A = cem_actions(np.zeros((H, a), np.float32), np.full((H, a), 0.5, np.float32), -1, 1, 5, 0, np.arange(sc.N))
    s0 = np.tile(p["s0"], (sc.N, 1)).astype(np.float32)
    if not over:
        return _edge_check(p, s0, A, H, precision, None, "weight 127.99999")
    c32, s32 = run(device_problem(p), p, s0, A, H, sc.N)
    costs, states = run(device_problem(p, precision), p, s0, A, H, sc.N)
    assert np.array_equal(_bits(costs), _bits(c32)) and np.array_equal(_bits(states), _bits(s32))
