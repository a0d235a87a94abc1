"""The cases of tests/test_gpu_gd_grad.py (mbrl_gd_grad against the float64 autograd gradient of
tests/gd_grad_reference.py) as plain data plus CPU helpers: no GPU import. One forward / backward
pass each, at the smallest shapes that reach each path of gd.hip:

  one-workgroup kernel   W in {16, 50, 100} (W != Wpad) x L in {1, 2, 3}; W = 300; W = 512 with L = 4
                         (the cooperative kernel's weight slices no longer fit its LDS); s + a = 6 (not a
                         multiple of 4: the K0p padding of the saved layer inputs) and s + a = 33 (past the
                         cooperative kernel's K0 <= 32); H in {1, 2, 7, 16}; goal-state and reward-head models.
                         Every cooperative case below is also run under MBRL_OPT_GD_SINGLE.
  cooperative kernel     W in {64, 128, 256, 512} x L in {2, 3, 4} (512 x 4 excepted, above); s + a in
                         {2, 23, 32}, s = 1; H in {1, 5, 12}; goal-state and reward-head models; every
                         MBRL_OPT_GD_HOP value; MBRL_OPT_DEBUG_GD_ABORT (the gated fallback).
  flags                  flag_cases.GD_VARIANTS, norm == NULL, no_state_cost, no_action_cost on a
                         cooperative and a one-workgroup shape; flag_cases.REWARD on a reward-head model.
  batches                B in {1, 3, 11} at W = 512, L = 3 (11 plans need two groups), distinct start
                         states and sequences.
  zero unit              a layer-0 unit whose pre-activation is exactly 0 in every precision and
                         summation order (zero bias, one non-zero weight on an action coordinate that is 0):
                         ReLU' there is 0, and a kernel masking with >= 0 would let a gradient through.

Every problem is flag_cases._sharpen'ed (statistics far from the identity). The seeds were searched on
the CPU (tests/test_gd_grad_host.py asserts the conditions, for every case): the smallest float64
|pre-activation| is at least MARGIN_FACTOR x the largest float32-vs-float64 pre-activation difference,
so no ReLU changes side between the precisions, and every applicable mutant of gd_grad_reference moves
the gradient by at least MUTANT_FACTOR x the case's bar. (The search asked for 2.5 x MARGIN_FACTOR, the
first seed from 1 upwards that gave it: another CPU's float32 mat-vec rounds a little differently.)"""
import functools

import numpy as np

import flag_cases as fc
import gd_grad_reference as ref
from oracle import cem as ocem

MARGIN_FACTOR = 100.0
BAR_FACTOR = 8.0        # bar(case) = BAR_FACTOR x max(e(grad32 of the case), median e(grad32) over all cases)
MUTANT_FACTOR = 10.0
HOP_VALUES = (0, 1, 2, 3)   # what mbrl_set_option accepts for MBRL_OPT_GD_HOP


def _c(cid, H, seed, variant=None, B=1, zero=False, **over):
    return dict(cid=cid, H=H, seed=seed, variant=variant, B=B, zero=zero, over=over)


CASES = {
    # ---- one-workgroup kernel (the cooperative kernel refuses these shapes)
    "single_w16_l1": _c(2, 1, 1, W=16, L=1),
    "single_w16_l2": _c(3, 2, 1, W=16, L=2),
    "single_w16_l3": _c(6, 7, 1, W=16, L=3),
    "single_w50_l1": _c(6, 16, 1, W=50, L=1),
    "single_w50_l2": _c(2, 7, 1, W=50, L=2),
    "single_w50_l3": _c(3, 16, 1, W=50, L=3),
    "single_w100_l1": _c(3, 2, 1, W=100, L=1),
    "single_w100_l2": _c(6, 1, 1, W=100, L=2),
    "single_w100_l3": _c(2, 16, 1, W=100, L=3),
    "single_w300_goal": _c(3, 7, 1, W=300, L=2),
    "single_w300_reward": _c(6, 2, 1, W=300, L=2),
    "single_k33_goal": _c(3, 2, 1, s=27, a=6, W=64, L=2),
    "single_k33_reward": _c(6, 7, 1, s=27, a=6, W=128, L=2),
    "single_w512_l4": _c(3, 1, 1, W=512, L=4),
    # ---- cooperative kernel
    "coop_w64_l2": _c(3, 12, 1, s=1, a=1, W=64, L=2),
    "coop_w64_l3": _c(6, 5, 1, W=64, L=3),
    "coop_w64_l4": _c(3, 1, 1, s=26, a=6, W=64, L=4),
    "coop_w128_l2": _c(6, 5, 1, s=20, a=12, W=128, L=2),
    "coop_w128_l3": _c(6, 12, 1, s=1, a=1, W=128, L=3),
    "coop_w128_l4": _c(3, 12, 1, W=128, L=4),
    "coop_w256_l2": _c(6, 1, 1, W=256, L=2),
    "coop_w256_l3": _c(3, 12, 1, W=256, L=3),
    "coop_w256_l4": _c(3, 5, 1, s=1, a=5, W=256, L=4),
    "coop_w512_l2": _c(6, 5, 1, W=512, L=2),
    "coop_w512_l3": _c(3, 5, 1, W=512, L=3),
    # ---- batches (distinct start states and sequences per plan)
    "batch_b1": _c(3, 2, 1, B=1, W=512, L=3),
    "batch_b3": _c(3, 2, 1, B=3, W=512, L=3),
    "batch_b11": _c(3, 2, 1, B=11, W=512, L=3),
    # ---- a unit that is exactly 0
    "zero_unit_coop": _c(3, 5, 1, variant="norm:ns+us", zero=True, W=64, L=2),
    "zero_unit_single": _c(6, 5, 1, variant="rew:ur", zero=True, W=50, L=2),
}
# ---- flags: the gd families of flag_cases (shapes as there)
FLAG_SHAPES = {"coop": (3, 6, dict(W=256, L=3)), "narrow": (3, 5, dict(W=50, L=2)), "reward": (6, 5, dict(W=64, L=2))}
GOAL_FLAGS = fc.GD_VARIANTS + ["norm_null", "no_state_cost", "no_action_cost"]
for _fam, (_cid, _H, _over) in FLAG_SHAPES.items():
    for _v in (fc.REWARD if _fam == "reward" else GOAL_FLAGS):
        CASES[f"flags_{_fam}_{_v.replace(':', '_').replace('+', '_')}"] = _c(_cid, _H, 1, variant=_v, **_over)

# the seeds the CPU search settled on (default 1: the first seed tried)
SEEDS = {"single_w50_l3": 5, "single_w100_l3": 9, "single_w300_goal": 6, "single_w300_reward": 2, "single_w512_l4": 4,
         "coop_w128_l2": 2, "coop_w128_l3": 2, "coop_w128_l4": 6, "coop_w256_l3": 23, "coop_w512_l2": 7,
         "coop_w512_l3": 8, "batch_b1": 2, "batch_b3": 22, "batch_b11": 344, "zero_unit_coop": 2,
         "flags_coop_norm_na": 3, "flags_coop_norm_us": 6, "flags_coop_norm_ns": 4, "flags_coop_weights_alphas": 3,
         "flags_coop_norm_null": 64, "flags_coop_no_state_cost": 3, "flags_coop_no_action_cost": 3,
         "flags_narrow_norm_na": 2, "flags_narrow_norm_ns": 2, "flags_narrow_norm_null": 2}
for _name, _seed in SEEDS.items():
    CASES[_name]["seed"] = _seed

NAMES = list(CASES)
# the option runs of the GPU test: (case, option, value)
HOP_CASES = ("coop_w128_l4", "coop_w256_l2")
ABORT_CASES = ("coop_w64_l3", "coop_w256_l3", "flags_reward_rew_ur_sn")
SEAM_CASES = ("coop_w256_l3", "single_w50_l3", "coop_w64_l3")     # one coop, one single, one reward
BATCH_MODES = {"coop": (), "gd_single": (("gd_single", 1),), "debug_gd_abort": (("debug_gd_abort", 1),)}


def coop_expected(name):
    """gd.hip gd_coop_supported restated: whether mbrl_gd_grad runs this case on the cooperative kernel
    (without MBRL_OPT_GD_SINGLE)."""
    p = problem(name)
    cfg, H = p["cfg"], CASES[name]["H"]
    s, a, W, L = cfg["s"], cfg["a"], cfg["W"], cfg["L"]
    if L < 2 or W not in (64, 128, 256, 512) or s + a > 32 or s > 32:
        return False
    al4 = lambda n: (n + 3) & ~3  # noqa: E731
    passes = 2 if cfg.get("reward") else 1
    floats = 2 * (L - 1) * 16 * (W + 32) + 32 + 4 * W + 64 + 8 * 32 + 3 * al4(H * a) + al4(H * a) \
        + al4((H + 1) * s) + 4 + al4(passes * H * (W // 32 + L - 1))
    return floats * 4 <= 160 * 1024


@functools.lru_cache(maxsize=None)
def problem(name):
    """The oracle problem of a case (shared: do not write to it). "norm_null": p["norm"] is None and the
    statistics stay under p["stats"], as flag_cases.problem."""
    c = CASES[name]
    kw = dict(fc.VARIANTS[c["variant"]]) if c["variant"] else {}
    p = fc._sharpen(ocem.synth_problem(c["cid"], seed=c["seed"], N=1, H=c["H"], **kw, **c["over"]))
    if c["variant"] == "norm_null":
        p["stats"], p["norm"] = p["norm"], None
    if c["zero"]:
        # unit 3 of layer 0 sees only action coordinate 0, whose normalised value inputs() holds at
        # exactly 0: its pre-activation is w * 0 + 0 in every pass and precision
        s = p["cfg"]["s"]
        w, b = p["model"][0][0]
        w, b = w.copy(), b.copy()
        keep = w[3, s]
        assert keep != 0
        w[3, :] = 0
        w[3, s] = keep
        b[3] = 0
        p["model"] = [[(w, b)] + list(p["model"][0][1:])]
        p["zero_unit"] = (3, 0)
    return p


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(start states [B, s], action sequences [B, H, a]) of a case; plan 0 starts at the problem's s0."""
    c, p = CASES[name], problem(name)
    cfg = p["cfg"]
    rng = np.random.default_rng(7000 + c["seed"])
    S0 = np.stack([p["s0"]] + [(fc.S0_SCALE * rng.standard_normal(cfg["s"])).astype(np.float32)
                               for _ in range(c["B"] - 1)])
    A = rng.uniform(-0.5, 0.5, (c["B"], c["H"], cfg["a"])).astype(np.float32)
    if c["zero"]:    # (a - act_mean) / act_std is exactly 0 at a = act_mean
        A[:, :, 0] = p["norm"]["act_mean"][0] if ocem.norm_flag(p["norm"], "normalize_action") else 0
    S0.setflags(write=False)
    A.setflags(write=False)
    return S0, A


def _per_plan(name, fn):
    S0, A = inputs(name)
    p = problem(name)
    return np.stack([fn(p, A[b], s0=S0[b]) for b in range(A.shape[0])])


@functools.lru_cache(maxsize=None)
def g64(name):
    g = _per_plan(name, ref.grad64)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def states64(name):
    return _per_plan(name, ref.states64)


@functools.lru_cache(maxsize=None)
def e32(name):
    """e(grad32) of a case: the float32 CPU restatement's own error to float64."""
    return ref.err(_per_plan(name, ref.grad32), g64(name))


@functools.lru_cache(maxsize=None)
def median_e32():
    return float(np.median([e32(n) for n in NAMES]))


def bar(name, factor=BAR_FACTOR):
    return factor * max(e32(name), median_e32())


def margin(name):
    """(smallest float64 |pre-activation|, largest float32-vs-float64 difference) over the case's plans."""
    S0, A = inputs(name)
    p = problem(name)
    pairs = [ref.min_preact_margin(p, A[b], s0=S0[b]) for b in range(A.shape[0])]
    return min(m for m, _ in pairs), max(d for _, d in pairs)


def mutant_errors(name):
    """{label: e(mutant)} for the mutants applicable to the case."""
    p = problem(name)
    return {label: ref.err(_per_plan(name, functools.partial(ref.mutant_grad64, label=label)), g64(name))
            for label in ref.applicable(p, CASES[name]["H"])}
