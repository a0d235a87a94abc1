"""The case table of the single-trajectory envelope tests (test_traj_cases_host.py on the CPU,
test_gpu_traj_envelope.py on the GPU): model shapes, horizons and options chosen so that mbrl_trajectory
reaches every instance launch_traj_reg and launch_traj_coop list (csrc/traj.hip: 20 of traj_reg_kernel, 8 of
traj_coop_kernel on both of its grids and under every MBRL_OPT_TRAJ_HOP value) and the plain kernel gated and
ungated, with each dispatch threshold of traj_impl (csrc/plan.hip) met from both sides.

A Case names a synthetic problem (oracle.cem.synth_problem(CID, **shape)), H, the traj_hop options it runs
under and whether MBRL_OPT_DEBUG_TRAJ_ABORT is set; `want` is the instance the case was built to reach, as
rollout_dispatch_model.trajectory_instance spells it at traj_hop = 0 (the model computes it; the host test
checks the two agree, so a case that drifts off its branch fails on the CPU). `about` says what the case is
there for. Shapes are as small as the edge allows: E <= 3 unless the case is about E, H <= 6 unless it is about
H (the reg / coop line on H a is met at H near 1000 and 664: the only way to the two narrowest K0R = 32
cooperative instances).

Inputs are drawn as tests/test_gpu_envelope.py draws them for its trajectories: the problem's s0 and
uniform(-1, 1) actions from default_rng(CID + H)."""
import collections
import functools

import numpy as np

import rollout_dispatch_model as rdm
from rollout_dispatch_model import Coop, Plain, Reg

CID = 3                  # the synthetic problem family (seed 1003); every dim below overrides the config's
HOPS = (0, 1, 2, 3)      # MBRL_OPT_TRAJ_HOP values

# D: the float32 oracle's worst absolute distance from the same rollout in float64 over this table, rounded up
# (tests/test_traj_cases_host.py computes it, prints it and fails if a case exceeds it). The GPU test compares
# with float64 at TIGHT = 32 D -- D already holds one float32 evaluation's rounding at these dot lengths; the
# factor leaves room for another summation order and FMA contraction over L + 1 layers and H contractive steps
# -- and at HARD, the suite's rtol = atol = 1e-4.
D = 1.5e-7                # measured 1.42e-7 (plain_L1_W512: one dot of length 512 per state)
TIGHT = 32 * D
HARD = 1e-4

Case = collections.namedtuple("Case", "id shape H hops abort want about")


def _c(id, s, a, W, L, H, want, about, E=1, hops=(0,), abort=0):
    return Case(id, dict(s=s, a=a, W=W, L=L, E=E), H, tuple(hops), abort, want, about)


def _reg(wp, nhl, k0r):
    return Reg("reg", wp, nhl, k0r)


def _coop(k0r, wi, grid="xcd", hop=rdm.TRAJ_HOP_DEFAULT):
    return Coop("coop", k0r, 2 if k0r == 32 else 5, wi, grid, hop)


# The reg / coop line: H a <= 16384 - 192 - 2 Wpad. a = 16 at Wpad 64 and a = 24 at Wpad 128 divide the limit,
# so the longest register-resident horizon fills the 64 KiB exactly and one step more is cooperative.
LINE_64 = dict(s=4, a=16, W=64, L=2)        # 16 * 1004 = 16064 = 16384 - 192 - 128
LINE_128 = dict(s=4, a=24, W=128, L=2)      # 24 * 664 = 15936 = 16384 - 192 - 256
H_LINE_64, H_LINE_128 = rdm.reg_max_steps(16, 64), rdm.reg_max_steps(24, 128)

REG = (
    # ---- Wpad 64
    _c("r64_n0_k8_s1_W8", 1, 1, 8, 1, 3, _reg(64, 0, 8), "s = 1, W = 8 < Wpad: the r < W / k < W guards, no hidden layer"),
    _c("r64_n0_k32_s17_W33", 17, 3, 33, 1, 2, _reg(64, 0, 32), "W = 33 < Wpad, the second output-row block"),
    _c("r64_n1_k8_K0_8", 4, 4, 64, 2, 4, _reg(64, 1, 8), "K0 = 8: the last shape of the K0R = 8 instance, W = Wpad"),
    _c("r64_n1_k32_K0_9", 4, 5, 64, 2, 4, _reg(64, 1, 32), "K0 = 9: the first shape of the K0R = 32 instance"),
    _c("r64_n2_k8_W33", 5, 2, 33, 3, 3, _reg(64, 2, 8), "two hidden layers at W < Wpad"),
    _c("r64_n2_k32_s16", 16, 6, 64, 3, 3, _reg(64, 2, 32), "s = 16: the first output-row block full, the second empty"),
    _c("r64_n2_k32_s17", 17, 6, 64, 3, 3, _reg(64, 2, 32), "s = 17: one row in the second output-row block"),
    _c("r64_n3_k8_W8", 3, 1, 8, 4, 3, _reg(64, 3, 8), "three hidden layers at W = 8"),
    _c("r64_n3_k32_K0_32", 31, 1, 64, 4, 2, _reg(64, 3, 32), "K0 = 32 with the largest s that admits (s = 31, a = 1)"),
    # ---- Wpad 128
    _c("r128_n0_k8_H1", 6, 2, 100, 1, 1, _reg(128, 0, 8), "H = 1, W = 100 < Wpad"),
    _c("r128_n0_k32", 17, 6, 128, 1, 3, _reg(128, 0, 32), "W = Wpad, s = 17"),
    _c("r128_n1_k8", 2, 3, 128, 2, 3, _reg(128, 1, 8), "W = Wpad"),
    _c("r128_n1_k32_s31_W100", 31, 1, 100, 2, 2, _reg(128, 1, 32), "K0 = 32, s = 31 at W < Wpad"),
    _c("r128_n2_k8_E3", 7, 1, 100, 3, 3, _reg(128, 2, 8), "E = 3 with the member mean", E=3),
    _c("r128_n2_k32_s16", 16, 3, 128, 3, 3, _reg(128, 2, 32), "s = 16"),
    _c("r128_n3_k8_s1", 1, 2, 128, 4, 3, _reg(128, 3, 8), "s = 1 under three hidden layers"),
    _c("r128_n3_k32_W100", 17, 15, 100, 4, 2, _reg(128, 3, 32), "K0 = 32 from a = 15, W < Wpad"),
    # ---- Wpad 256
    _c("r256_n0_k8_W200", 5, 3, 200, 1, 3, _reg(256, 0, 8), "K0 = 8, W = 200 < Wpad"),
    _c("r256_n0_k32", 17, 6, 256, 1, 3, _reg(256, 0, 32), "W = Wpad, s = 17"),
    _c("r256_n1_k8", 4, 4, 256, 2, 3, _reg(256, 1, 8), "K0 = 8, W = Wpad"),
    _c("r256_n1_k32_W200_E3", 5, 4, 200, 2, 4, _reg(256, 1, 32), "K0 = 9, W = 200, E = 3 with the member mean", E=3),
    # ---- the longest register-resident horizons
    _c("line64_reg", H=H_LINE_64, want=_reg(64, 1, 32), about="H a = 16064: exactly the 64 KiB of traj_reg_supported", **LINE_64),
    _c("line128_reg", H=H_LINE_128, want=_reg(128, 1, 32), about="H a = 15936: exactly the 64 KiB at Wpad 128", **LINE_128),
)

COOP = (
    # ---- one step past the reg limit: the only routes to <32, 2, 2> and <32, 2, 4>
    _c("line64_coop", H=H_LINE_64 + 1, want=_coop(32, 2), about="one step past the reg limit at Wpad 64", hops=HOPS, **LINE_64),
    _c("line128_coop", H=H_LINE_128 + 1, want=_coop(32, 4), about="one step past the reg limit at Wpad 128", **LINE_128),
    # ---- K0R = 32 at W = 256 (reg stops at one hidden layer) and W = 512
    _c("c32_w8_L3", 17, 6, 256, 3, 4, _coop(32, 8), "K0R = 32 at W = 256, L = 3", hops=HOPS),
    _c("c32_w8_L4_E5", 5, 2, 256, 4, 3, _coop(32, 8), "L = 4; E = 5: the per-XCD grid with three idle slots", E=5, hops=HOPS),
    _c("c32_w8_L3_E9", 6, 2, 256, 3, 3, _coop(32, 8, "pe", 0), "E = 9 forces the (P, E) grid at K0R = 32", E=9, hops=HOPS),
    _c("c32_w16_s31", 31, 1, 512, 2, 3, _coop(32, 16), "W = 512, K0 = 32, L = 2"),
    # ---- K0R = 96 at every width
    _c("c96_w2_s33", 33, 1, 64, 2, 4, _coop(96, 2), "s = 33: the first s past the reg and K0R = 32 budgets", hops=HOPS),
    _c("c96_w2_s33_E5", 33, 1, 64, 2, 3, _coop(96, 2), "E = 5: the per-XCD grid with idle slots at K0R = 96", E=5, hops=HOPS),
    _c("c96_w2_L3_E9", 40, 3, 64, 3, 3, _coop(96, 2, "pe", 0), "E = 9 forces the (P, E) grid at K0R = 96", E=9, hops=HOPS),
    _c("c96_w4_K0_33", 20, 13, 128, 3, 3, _coop(96, 4), "K0 = 33 > 32 with s <= 32, L = 3"),
    _c("c96_w4_E8", 33, 2, 128, 2, 3, _coop(96, 4), "E = 8: the per-XCD grid full", E=8, hops=HOPS),
    _c("c96_w8_s65_L4", 65, 6, 256, 4, 3, _coop(96, 8), "s = 65: one row in SM = 5's last block; L = 4"),
    _c("c96_w16_s80_K0_96", 80, 16, 512, 2, 3, _coop(96, 16), "K0 = 96 exactly at s = 80: SM = 5's last row"),
)

PLAIN = (
    # ---- the other edges of the cooperative budget, from the refused side
    _c("plain_W100", 40, 3, 100, 2, 3, Plain("plain", False), "W != Wpad past the reg budget"),
    _c("plain_L1_W512", 17, 6, 512, 1, 3, Plain("plain", False), "L = 1 at W = 512"),
    _c("plain_PE_1028", 33, 1, 64, 2, 2, Plain("plain", False), "P E = 4 * 257 = 1028 > 1024", E=257),
    # ---- MBRL_OPT_DEBUG_TRAJ_ABORT = 1
    _c("abort_reg_shape", 4, 5, 64, 2, 4, Plain("plain", True), "a reg shape: the gated kernel behind an aborted coop", abort=1),
    _c("abort_c96_narrow", 33, 1, 64, 2, 4, Plain("plain", True), "a K0R = 96 narrow shape, E = 3", E=3, abort=1),
    _c("abort_coop_refused", 40, 3, 100, 2, 3, Plain("plain", False), "a shape coop refuses: plain runs ungated", abort=1),
)

CASES = REG + COOP + PLAIN
HOP_CASES = tuple(c for c in COOP if c.hops == HOPS)

# (accepted-side id, other-side id or None where the other side is host-only, the threshold)
BOUNDARIES = (
    ("r64_n1_k8_K0_8", "r64_n1_k32_K0_9", "K0 <= 8"),
    ("r64_n2_k32_s16", "r64_n2_k32_s17", "the second output-row block (s > 16)"),
    ("line64_reg", "line64_coop", "H a at Wpad 64"),
    ("line128_reg", "line128_coop", "H a at Wpad 128"),
    ("r64_n3_k32_K0_32", "c96_w4_K0_33", "K0 <= 32"),
    ("r128_n1_k32_s31_W100", "c96_w2_s33", "s <= 32"),
    ("c96_w16_s80_K0_96", None, "s <= 80, K0 <= 96 (past them: tests/test_gpu_envelope.py s90, s_plus_a_100)"),
    ("c96_w4_E8", "c32_w8_L3_E9", "E <= 8"),
    (None, "plain_PE_1028", "P E <= 1024 (the accepted side is never launched: see HOST_ONLY)"),
)

# Static dispatch edges the GPU never sees from this side: a cooperative grid at the 1024-workgroup capacity
# is not launched on a shared machine. (shape, H, instance at traj_hop = 0)
HOST_ONLY = (
    (dict(s=33, a=1, W=64, L=2, E=256), 2, _coop(96, 2, "pe", 0)),      # P E = 1024: accepted
    (dict(s=33, a=1, W=64, L=2, E=257), 2, Plain("plain", False)),      # 1028: refused
    (dict(s=17, a=6, W=512, L=2, E=32), 2, _coop(32, 16, "pe", 0)),     # 32 * 32 = 1024
    (dict(s=17, a=6, W=512, L=2, E=33), 2, Plain("plain", False)),
)

# One two-iteration CEM plan per family: (case id, N, K)
PLANS = (("r128_n2_k8_E3", 64, 8), ("c96_w2_s33", 48, 6), ("line64_coop", 32, 4))


def by_id(cid):
    for c in CASES:
        if c.id == cid:
            return c
    raise KeyError(cid)


def instance(case, traj_hop=0):
    sh = case.shape
    return rdm.trajectory_instance(sh["s"], sh["a"], sh["W"], sh["L"], sh["E"], H=case.H, traj_hop=traj_hop,
                                   debug_abort=case.abort)


@functools.lru_cache(maxsize=None)
def problem(cid):
    """The oracle problem of a case (shared, never written)."""
    from oracle import cem as ocem
    c = by_id(cid)
    return ocem.synth_problem(CID, N=1, H=c.H, **c.shape)


@functools.lru_cache(maxsize=None)
def actions(cid):
    c = by_id(cid)
    acts = np.random.default_rng(CID + c.H).uniform(-1, 1, size=(c.H, c.shape["a"])).astype(np.float32)
    acts.setflags(write=False)
    return acts


def mean_f32(members):
    """The member mean as the library and the oracle define it: (m_0 + m_1 + ...) / E, sequential in float32."""
    acc = members[0].astype(np.float32)
    for e in range(1, members.shape[0]):
        acc = (acc + members[e].astype(np.float32)).astype(np.float32)
    return (acc / np.float32(members.shape[0])).astype(np.float32) if members.shape[0] > 1 else acc


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(float64 member states [E, H, s], float32-oracle member states [E, H, s]) of a case; read-only."""
    from oracle import cem as ocem
    import rollout_cases as rc
    p, acts = problem(cid), actions(cid)
    A = np.ascontiguousarray(acts[:, None, :])
    _, s64 = rc.rollout_f64(p, p["s0"], A, store_states=True)
    _, s32 = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A, store_states=True)
    s64, s32 = np.ascontiguousarray(s64[:, :, 0, :]), np.ascontiguousarray(s32[:, :, 0, :])
    for x in (s64, s32):
        x.setflags(write=False)
    return s64, s32
