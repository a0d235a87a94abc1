"""The case table of the split-operand rollout tests (precision F16X3 / F16X6, csrc/rollout_f16x3.hip):
test_rollout_dispatch_model.py and test_split_host.py on the CPU, test_gpu_split_envelope.py on the GPU.

A Case names a synthetic problem (oracle.cem.synth_problem(cid, **over)), N and H, as rollout_cases.py does;
`built_for` holds the fields of rollout_dispatch_model.split_kernel's outcome the case was written to reach
(checked on the CPU for P = 2 and P = 3, so a case that drifts off its branch fails there). TILE32 lists the
cases run under MBRL_OPT_SPLIT_TILE = 32: the request for 32-candidate workgroups (R = 2) that N >= 8192
would make. Every case has N = 40 -- three 16-candidate tiles or two 32-candidate tiles, the last one partial --
and H in {1, 2, 3}: H = 1 runs step<0> alone, H = 2 both ring phases, H = 3 the wrap of the weight ring into a
third step. `mode` is how the GPU test feeds a case: "given" actions, "per_cand" (s0_per_candidate),
"sampled" (an in-call draw at n_offset > 0).

The bar of a case, for P pieces (test_split_host.py measures what it is built from):

    bar_P(case) = K_P x max(e32(case), median e32),      e(x) = max |x - x64| / max |x64| over the states,

e32 being e of the float32 oracle. K_P = 4 x the worst ratio e(emulation, P) / max(e32, median e32) over the
table, and never below 8: the emulation (split_reference.emulate_split) sums each Linear as NumPy does, the
kernel over K slices on 8 waves and LDS partial sums, which the 4 allows for; 8 is what test_gpu_gd_grad.py
grants a kernel for the same reason. Measured on the CPU (test_split_host.py asserts the constants follow):

    worst ratio P = 2: 1.80 (c11_t8_l1)     -> K_2 = max(8, 7.2) = 8
    worst ratio P = 3: 1.31 (c11_t4_l3)     -> K_3 = max(8, 5.3) = 8

so both precisions are held to the float32 oracle's own distance from float64, eightfold. Nothing here comes
from a kernel's output.

The third-piece cases (THIRD) are exact by construction and tell F16X6 from F16X3; see third_problem()."""
import collections
import functools

import numpy as np

import rollout_dispatch_model as rdm
import split_reference as sref
from oracle import cem as ocem
from oracle.philox import cem_actions

N = 40
SAMPLE_OFFSET = 4096 + 5
WORST_RATIO = {2: 1.80, 3: 1.31}         # measured by test_split_host.py (see above)
MARGIN, FLOOR = 4.0, 8.0
K_BAR = {P: max(FLOOR, MARGIN * r) for P, r in WORST_RATIO.items()}      # 8 and 8
MUTANT_FACTOR = 10.0
THIRD_ULPS = 2.0

Case = collections.namedtuple("Case", "id cid over N H mode built_for")
TILE32 = set()

C22, C31, C31_BUMP, C33 = dict(s=40, a=8), dict(s=20, a=48), dict(s=24, a=16), dict(s=67, a=21)


def _c(id, cid, over, H, mode="given", tile=0, **built_for):
    if tile == 32:
        TILE32.add(id)
    return Case(id, cid, over, N, H, mode, built_for)


def _s(T, R, K0S, NOS, **kw):
    return dict(kind="split", T=T, R=R, K0S=K0S, NOS=NOS, **kw)


ACCEPTED = (
    # ---- (1, 1): cartpole at W = 256 (T = 4), cheetah at W = 512 (T = 8); both tile heights; every depth
    _c("c11_t4", 2, dict(), 3, **_s(4, 1, 1, 1)),
    _c("c11_t4_r2", 2, dict(), 2, "per_cand", 32, **_s(4, 2, 1, 1)),
    _c("c11_t8", 3, dict(), 2, "sampled", **_s(8, 1, 1, 1)),
    _c("c11_t8_r2", 3, dict(), 3, tile=32, **_s(8, 2, 1, 1)),
    _c("c11_t4_l1", 2, dict(L=1), 3, **_s(4, 1, 1, 1)),
    _c("c11_t4_l1_r2", 2, dict(L=1), 3, "per_cand", 32, **_s(4, 2, 1, 1)),
    _c("c11_t4_l3", 2, dict(L=3), 2, "sampled", **_s(4, 1, 1, 1)),
    _c("c11_t4_l4", 2, dict(L=4), 1, tile=32, **_s(4, 2, 1, 1)),
    _c("c11_t8_l1", 3, dict(L=1), 3, "per_cand", **_s(8, 1, 1, 1)),
    _c("c11_t8_l2", 3, dict(L=2), 2, tile=32, **_s(8, 2, 1, 1)),
    _c("c11_t8_l4", 3, dict(L=4), 1, "sampled", **_s(8, 1, 1, 1)),
    # ---- (2, 2): R = 1 only, a forced split_tile = 32 falls back to 16-candidate tiles
    _c("c22_t4", 3, dict(W=256, L=2, **C22), 3, "per_cand", 32, **_s(4, 1, 2, 2)),
    _c("c22_t8", 3, dict(**C22), 2, **_s(8, 1, 2, 2)),
    # ---- (3, 1): three real layer-0 chunks (a = 48: the third action slot), and K0S bumped from 2 to 3
    _c("c31_t4", 3, dict(W=256, L=2, **C31), 2, **_s(4, 1, 3, 1)),
    _c("c31_t4_r2", 3, dict(W=256, L=2, **C31), 3, "sampled", 32, **_s(4, 2, 3, 1)),
    _c("c31_t8", 3, dict(**C31), 3, "per_cand", **_s(8, 1, 3, 1)),
    _c("c31_t8_r2_lds", 3, dict(**C31), 2, tile=32, **_s(8, 1, 3, 1)),     # the redo pass's 32 rows do not fit
    _c("c31_bump_t4", 3, dict(W=256, L=2, **C31_BUMP), 3, "sampled", **_s(4, 1, 3, 1)),
    _c("c31_bump_t4_r2", 3, dict(W=256, L=3, **C31_BUMP), 2, tile=32, **_s(4, 2, 3, 1)),
    _c("c31_bump_t8", 3, dict(**C31_BUMP), 1, **_s(8, 1, 3, 1)),
    _c("c31_bump_t8_r2", 3, dict(L=2, **C31_BUMP), 3, "per_cand", 32, **_s(8, 2, 3, 1)),
    # ---- (3, 3): humanoid's dims, one of them an ensemble
    _c("c33_t4", 5, dict(W=256, L=2, E=1), 3, **_s(4, 1, 3, 3)),
    _c("c33_t8_e2", 5, dict(E=2), 2, "per_cand", **_s(8, 1, 3, 3)),
    # ---- widths off the tile grid
    _c("w129", 3, dict(W=129, L=2), 3, tile=32, **_s(4, 2, 1, 1)),
    _c("w200", 3, dict(W=200, L=3), 2, "per_cand", **_s(4, 1, 1, 1)),
    _c("w257", 3, dict(W=257, L=2), 3, **_s(8, 1, 1, 1)),
    _c("w300", 3, dict(W=300, L=3), 2, "sampled", 32, **_s(8, 2, 1, 1)),
    # ---- action slots: a = 16 fills the first, 17 starts the second, 32 fills it, 33 starts the third
    _c("a16", 2, dict(a=16), 2, **_s(4, 1, 1, 1)),
    _c("a17", 3, dict(s=5, a=17, L=2), 3, "sampled", 32, **_s(8, 2, 1, 1)),
    _c("a32", 2, dict(a=32), 3, tile=32, **_s(4, 2, 3, 1)),
    _c("a33", 3, dict(s=5, a=33, L=2), 2, "per_cand", **_s(8, 1, 3, 1)),
    # ---- an ensemble with (1, 1)
    _c("e2_c11", 3, dict(E=2, L=2), 3, "per_cand", 32, **_s(8, 2, 1, 1)),
)

DECLINED = (
    _c("no_k0s4", 3, dict(s=40, a=30), 2, kind="f32", reason="shape class (4, 2)"),      # K0S 3 bumped to 4
    _c("no_s100", 3, dict(s=100, W=256, L=2), 2, "per_cand", kind="f32", reason="shape class (4, 4)"),
    _c("no_a49", 3, dict(a=49), 2, kind="f32", reason="refused"),
    _c("no_w128", 3, dict(W=128), 3, kind="f32", reason="T = 2"),
    _c("no_w600", 3, dict(W=600, L=2), 2, "sampled", kind="f32", reason="T = 16"),
    _c("no_reward", 6, dict(), 2, tile=32, kind="f32", reason="reward head"),
)
# R = 2 requests turned down (the case runs the split kernel on 16-candidate tiles): by rollout_split_supported
# (more than one output chunk) and by the redo pass's rollout_lds_bytes(X, 32) check
R2_DECLINED = ("c22_t4", "c31_t8_r2_lds")
REFUSED = ("no_a49",)      # mbrl_rollout_cost refuses the shape at either precision


def by_id(cid):
    for c in ACCEPTED + DECLINED:
        if c.id == cid:
            return c
    raise KeyError(cid)


def shape_of(case):
    cfg = dict(ocem.CONFIGS[case.cid])
    cfg.update(case.over)
    return cfg["s"], cfg["a"], cfg["W"], cfg["L"], cfg["E"], int(bool(cfg.get("reward")))


def tile_of(case):
    return 32 if case.id in TILE32 else 0


def outcome(case, P):
    """The dispatch model's outcome for the case as the GPU test runs it."""
    return rdm.split_kernel(*shape_of(case), N=case.N, P=P, split_tile=tile_of(case))


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def problem(cid):
    c = by_id(cid)
    return ocem.synth_problem(c.cid, N=c.N, H=c.H, **c.over)


def sampled_distribution(H, a):
    rng = np.random.default_rng(H * 100 + a)
    return rng.uniform(-0.3, 0.3, (H, a)).astype(np.float32), rng.uniform(0.2, 0.6, (H, a)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(s0 [s] or [N, s], actions [H, N, a]) of a case, read-only. A sampled case's actions are the draw
    the kernel call makes itself: iteration 1 of the problem's seed at SAMPLE_OFFSET."""
    c, p = by_id(cid), problem(cid)
    a = p["cfg"]["a"]
    if c.mode == "sampled":
        mu, sg = sampled_distribution(c.H, a)
        A = cem_actions(mu, sg, -1, 1, p["rng_seed"], 1, np.arange(SAMPLE_OFFSET, SAMPLE_OFFSET + c.N))
    else:
        A = cem_actions(np.zeros((c.H, a), np.float32), np.full((c.H, a), 0.5, np.float32), -1, 1, 11, 0,
                        np.arange(c.N))
    s0 = p["s0"]
    if c.mode == "per_cand":
        rng = np.random.default_rng(len(c.id))
        s0 = (s0[None, :] + 0.25 * rng.standard_normal((c.N, s0.size))).astype(np.float32)
    for x in (s0, A):
        x.setflags(write=False)
    return s0, A


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(float32 oracle costs, states, float64 states) of a case, read-only."""
    p = problem(cid)
    s0, A = inputs(cid)
    c32, s32 = ocem.rollout(p["model"], p["norm"], p["cost"], s0, A, store_states=True)
    _, s64 = sref.rollout_f64(p, A, s0)
    for x in (c32, s32, s64):
        x.setflags(write=False)
    return c32, s32, s64


@functools.lru_cache(maxsize=None)
def e32(cid):
    _, s32, s64 = reference(cid)
    return sref.err(s32, s64)


@functools.lru_cache(maxsize=None)
def median_e32():
    return float(np.median([e32(c.id) for c in ACCEPTED]))


def base(cid):
    return max(e32(cid), median_e32())


def bar(cid, P):
    return K_BAR[P] * base(cid)


@functools.lru_cache(maxsize=None)
def emulated(cid, P, drop=None):
    """States of the emulation with P pieces, optionally without the product `drop` = (i, j)."""
    keep = None if drop is None else [t for t in sref.terms(P) if t != drop]
    s0, A = inputs(cid)
    return sref.emulate_split(problem(cid), A, P, keep, s0)[1]


# ------------------------------------------------------------------------------------------------ third piece
# Two exact cases, cartpole's shape (s = 5, a = 1, W = 256, L = 2, H = 1), no normalisers, zero biases. Every
# hidden unit has one nonzero weight, so nothing accumulates; every value on the way is a float32 number and
# every product is exact in float32, so float64, float32 and a correct F16X6 agree to the bit. Output row d is
# the difference of two hidden units that carry nearly equal values (h_a - h_b, exact by Sterbenz). A single
# Linear cannot lose more than 2 ulp of its own output to a dropped third-order product (|x1 w1|, |x0 w2|,
# |x2 w0| <= 2^-22 |x w|), so that alone would never pass a 2 ulp bar; the difference lifts such a loss to
# hundreds of ulp of the state. Only h_a carries the probed product (else the loss would cancel). The last state
# is h_a alone, so that max |x64| -- what e() divides by -- is the size of the hidden values and F16X3's own
# bar keeps its meaning. Activations
# stay in [16, 2048) and the probing weights in [1, 128), where a third piece is a normal float16
# (rollout_f16x3.hip's header).
#   "carry": weights are signed powers of two, inputs 24-bit mantissas (h_a and h_b from neighbouring input
#            columns): F16X3, and an F16X6 without x2 w0, lose each input's last bits.
#   "cross": per state one probe: "x1w1", a layer-0 weight 1 + 2^-11 under 12-bit inputs 16 (1 + j 2^-11);
#            "x0w2", a weight 64 (1 + 2^-12 + 2^-23) under power-of-two inputs (its 24-bit product then goes
#            through layer 1 as a carry); and one "carry" as above.
THIRD = ("carry", "cross")
THIRD_CATCHES = {"carry": {(2, 0)}, "cross": {(1, 1), (0, 2), (2, 0)}}
_PROBES = {"carry": ("carry",) * 5, "cross": ("x1w1", "x0w2", "carry", "x1w1", "x0w2")}
_COLUMNS = {"carry": ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5)), "cross": ((0, 0), (1, 1), (2, 3), (4, 4), (5, 5))}
_UA, _UB = (7, 58, 109, 160, 211), (30, 73, 116, 159, 202)          # layer-0 units of h_a, h_b per state d
_VA, _VB = (100, 131, 162, 193, 224), (3, 50, 97, 144, 191)         # layer-1 units


@functools.lru_cache(maxsize=None)
def third_problem(name):
    """(problem, s0 [N, 5], actions [1, N, 1]) of a third-piece case, read-only."""
    f32 = np.float32
    p = ocem.synth_problem(2, N=N, H=1, has_action_cost=False,       # (cosh of an action of 16 overflows)
                           norm_flags=dict(normalize_state=False, unnormalize_state=False, normalize_action=False))
    s, a, W = 5, 1, 256
    rng = np.random.default_rng(7 if name == "carry" else 8)
    w0, w1, w2 = np.zeros((W, s + a)), np.zeros((W, W)), np.zeros((s, W))
    for r in range(W):                          # the idle units: one signed power of two each
        w0[r, r % (s + a)] = -2.0 ** int(rng.integers(-3, 3))
        w1[r, (r * 5 + 1) % W] = 2.0 ** int(rng.integers(-3, 1)) * (1 if r % 2 else -1)     # (inputs reach 1024)
    n = np.arange(N)
    x = np.zeros((N, s + a))
    head = 16 * (1 + rng.integers(0, 512, N) * 2.0 ** -10)          # shared by a candidate's columns
    for d in range(s):
        probe, (ca, cb) = _PROBES[name][d], _COLUMNS[name][d]
        if probe == "carry":
            wa, wb, gain = 1.0, 1.0, 2.0
            for c in (ca, cb):                                       # 24-bit mantissas, the last bit set
                x[:, c] = head + 16 * (c * 2.0 ** -11 + (2 * rng.integers(0, 2 ** 11, N) + 1) * 2.0 ** -23)
        elif probe == "x1w1":
            wa, wb, gain = 1 + 2.0 ** -11, 1 + 2.0 ** -8, 2.0
            x[:, ca] = 16 * (1 + (2 * ((n + d) % 16) + 1) * 2.0 ** -11)
        else:
            wa, wb, gain = 64 * (1 + 2.0 ** -12 + 2.0 ** -23), 64 * (1 + 2.0 ** -9 + 2.0 ** -12), 2.0 ** -6
            x[:, ca] = np.where((n + d) % 2, 16.0, 8.0)
        for u, v, c, w, sign in ((_UA[d], _VA[d], ca, wa, 1.0), (_UB[d], _VB[d], cb, wb, -1.0)):
            w0[u], w1[v] = 0.0, 0.0
            w0[u, c], w1[v, u], w2[d, v] = w, gain, sign if (d < s - 1 or sign > 0) else 0.0
    x32, (w0, w1, w2) = x.astype(f32), (m.astype(f32) for m in (w0, w1, w2))
    assert np.array_equal(x32, x)
    p["model"] = [[(w0, np.zeros(W, f32)), (w1, np.zeros(W, f32)), (w2, np.zeros(s, f32))]]
    s0 = np.ascontiguousarray(x32[:, :s])
    A = np.ascontiguousarray(x32[None, :, s:])
    for arr in (s0, A, w0, w1, w2):
        arr.setflags(write=False)
    return p, s0, A


def third_bar(name, P):
    """The bar of section "bar_P" for a third-piece case: its e32 is 0, so K_P x the table's median e32."""
    return K_BAR[P] * max(sref.err(third_reference(name)[1], third_reference(name)[2]), median_e32())


@functools.lru_cache(maxsize=None)
def third_reference(name):
    """(float32 oracle costs, states, float64 states) of a third-piece case."""
    p, s0, A = third_problem(name)
    c32, s32 = ocem.rollout(p["model"], p["norm"], p["cost"], s0, A, store_states=True)
    _, s64 = sref.rollout_f64(p, A, s0)
    return c32, s32, s64
