"""Coloured-noise proposals (include/mbrl_cem.h mbrl_sample_actions_mixed, mbrl_cem_plan_rh_mixed,
mbrl_cem_plan_rh_batch_mixed): the fixtures of the mixed plans. TEST INFRASTRUCTURE ONLY: the checker for
csrc/cem_noise.hip and the mixed plan loops. The restatement itself is cem_rh_reference's -- plan, proposals,
mixed_actions and mixed_normals with a mix, re-exported here; DESIGN.md "Coloured-noise proposals" is
normative: with z[u] the white normals of Philox counter (n, u, i, d >> 2) and C the plan's [H, H] float32 mix,
    e[t] = (..((C[t][0] z[0]) + C[t][1] z[1]) + ..) + C[t][H-1] z[H-1]
every product rounded to float32 before it is added, the additions sequential in u; the action is
clip(mu[t] + sigma[t] e[t]). mix = None is the white plan."""
import cem_rh_batch_reference as br
import cem_rh_reference as rh
from cem_rh_reference import clip_keep_nan, closed_loop, gaps, mixed_actions, mixed_normals, proposals  # noqa: F401

F32 = rh.F32
GAP_MIN = rh.GAP_MIN


def plan(problem, N, H, K, I, **kw):
    """cem_rh_reference.plan (its keywords: mix, and b / s0 for problem b of a batch)."""
    return rh.plan(problem, N, H, K, I, **kw)


def beta_mix(H, beta=1.0):
    from mbrl_amd.planners import colored_noise_mix
    return colored_noise_mix(H, beta)


# ---------------------------------------------------------------------------------------------
# The GPU test's fixture problems (tests/test_gpu_cem_noise.py), shared with the host test that asserts their
# gap condition (tests/test_cem_noise_host.py). s = 5, K = 8, I = 3, a beta = 1 mix.
# (W, L, a, N, E, Kc, inputs, H, seed): every value of every axis -- H = 3 and 12 -- each input combination, and a
# seed at which every iteration's K-th and Kc-th return gaps exceed GAP_MIN on the restatement (find_seed).
# ---------------------------------------------------------------------------------------------
SMALL = dict(s=5, K=8, I=3)
CASES = [
    (64, 1, 1, 64, 1, 0, (), 3, 2),
    (64, 1, 5, 100, 2, 0, ("mu",), 12, 0),
    (256, 2, 8, 64, 1, 0, ("sigma",), 12, 1),
    (256, 2, 1, 100, 2, 0, ("mu", "sigma"), 3, 1),
    (64, 1, 8, 100, 1, 1, (), 12, 0),
    (64, 1, 5, 64, 2, 1, ("carry",), 3, 1),
    (256, 2, 1, 64, 1, 3, ("mu", "sigma", "carry"), 12, 0),
    (256, 2, 5, 100, 1, 3, ("mu",), 3, 0),
    (64, 1, 8, 64, 2, 3, ("carry",), 12, 0),
    (256, 2, 8, 100, 2, 8, ("mu", "sigma", "carry"), 3, 0),
    (64, 1, 5, 100, 1, 8, ("sigma",), 12, 0),
    (256, 2, 5, 64, 2, 8, (), 3, 0),
    (64, 1, 1, 100, 1, 3, ("sigma",), 3, 11),
    (256, 2, 1, 100, 2, 1, ("mu", "sigma", "carry"), 12, 0),
    (256, 2, 8, 64, 1, 1, ("mu",), 3, 0),
    (64, 1, 1, 64, 2, 8, ("carry",), 12, 2),
]


def case_id(case):
    W, L, a, N, E, Kc, inputs, H, _ = case
    return f"W{W}-L{L}-a{a}-N{N}-E{E}-Kc{Kc}-H{H}-" + ("+".join(inputs) or "none")


def make_case(case):
    """(problem, mix, kwargs of plan()) of one fixture case, as cem_rh_reference.make_case builds them."""
    p, kw = rh.make_case(case[:7] + case[8:], H=case[7], seed0=7600)
    return p, beta_mix(case[7]), kw


def case_plan(case, final=False):
    p, mix, kw = make_case(case)
    return plan(p, case[3], case[7], SMALL["K"], SMALL["I"], mix=mix, final=final, **kw)


def case_gap(case):
    return rh.case_gaps(case_plan(case), SMALL["K"], case[5])


def find_seed(case, limit=400, gap=case_gap):
    """The first seed at which the case's smallest gap exceeds GAP_MIN (how the tables' seeds were found)."""
    for seed in range(limit):
        if gap(case[:-1] + (seed,)) > GAP_MIN:
            return seed
    raise RuntimeError(f"no seed below {limit} for {case[:-1]}")


# The batched fixture (mbrl_cem_plan_rh_batch_mixed): (W, L, a, N, E, Kc, per-problem inputs, H, seed) with "m",
# "s", "c" naming the inputs a problem is given and "" a problem that plans cold, as cem_rh_batch_reference's
# table: B = 1, 2 and 5 twice each, with all, no and mixed per-problem inputs.
BATCH_CASES = [
    (64, 1, 5, 100, 1, 3, ("msc",), 12, 0),
    (256, 2, 1, 64, 2, 0, ("",), 3, 4),
    (64, 1, 8, 100, 1, 1, ("", "mc"), 3, 0),
    (256, 2, 5, 64, 1, 8, ("msc", "msc"), 12, 0),
    (64, 1, 8, 64, 2, 3, ("c", "", "msc", "s", "m"), 3, 4),
    (256, 2, 1, 100, 1, 0, ("", "", "", "", ""), 12, 11),
]


# One more batch, wide enough that the first launch and the draw take 32-pair tiles on a 256-CU device
# (B N ceil(a / 4) = 20480 pairs >= 32 x 2 x 256; csrc/cem_noise.hip noise_launch): the fixtures above all run
# 16-pair tiles.
WIDE_BATCH_CASE = (64, 1, 8, 2048, 1, 3, ("msc", "", "c", "s", "m"), 3, 55)


def batch_case_id(case):
    W, L, a, N, E, Kc, inputs, H, _ = case
    return f"W{W}-L{L}-a{a}-N{N}-E{E}-Kc{Kc}-H{H}-B{len(inputs)}-" + "+".join(x or "0" for x in inputs)


def make_batch_case(case):
    """(problem, s0s [B, s], mix, kws) of one fixture batch, as cem_rh_batch_reference.make_case builds them."""
    p, s0s, kws = rh.make_batch(case[:7] + case[8:], H=case[7], seed0=7900)
    return p, s0s, beta_mix(case[7]), kws


def batch_case_plans(case, final=False):
    p, s0s, mix, kws = make_batch_case(case)
    return br.plan_batch(p, s0s, case[3], case[7], SMALL["K"], SMALL["I"], case[5], kws, mix=mix, final=final)


def batch_case_gap(case):
    return min(rh.case_gaps(res, SMALL["K"], case[5]) for res in batch_case_plans(case))


_PLANS = {}


def cached(fn, case, **kw):
    """fn(case, **kw), computed once per session and shared (read only) by the tests that need it."""
    key = (fn.__name__, case, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = fn(case, **kw)
    return _PLANS[key]
