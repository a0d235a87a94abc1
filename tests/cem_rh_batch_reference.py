"""Batched receding-horizon CEM (include/mbrl_cem.h mbrl_cem_plan_rh_batch) restated in NumPy: ONE problem of
a batch is cem_rh_reference.plan with its own initial state and candidate indices b N + arange(N) for the
proposal RNG. TEST INFRASTRUCTURE ONLY: the checker for the problem dimension of csrc/cem_rh.hip, the staged
refit and the batched plan loop.

A batch is B such plans that share the model, the cost and the CEM settings and differ in their initial
state, their optional inputs (an absent input = that problem's flag bit clear) and their candidate offset."""
import numpy as np

import cem_rh_reference as rh

F32 = np.float32
FLAG_MU, FLAG_SIGMA, FLAG_CARRY = 1, 2, 4
SMALL = rh.SMALL
GAP_MIN = rh.GAP_MIN


def plan_problem(problem, s0, b, N, H, K, I, **kw):
    """Problem b of a batch: cem_rh_reference.plan on initial state s0 with Philox candidate indices
    b N + arange(N) (its keywords; b == 0 and s0 == problem["s0"]: the single plan)."""
    return rh.plan(problem, N, H, K, I, s0=s0, b=b, **kw)


def plan_batch(problem, s0s, N, H, K, I, keep, kws, seed=None, final=True, mix=None):
    """The B plans of a batch: kws[b] holds problem b's optional inputs (cem_rh_reference.plan's keywords)."""
    return [plan_problem(problem, s0s[b], b, N, H, K, I, keep=keep, seed=seed, final=final, mix=mix, **kws[b])
            for b in range(len(kws))]


def stack_inputs(kws, H, a, Kc):
    """The batch's device inputs from per-problem keywords: dict(init_mu_rows, init_sigma_rows [B, H, a],
    carry_in [B, Kc, H, a], each None when no problem has it, and flags int32 [B]). A problem without an
    input gets filler that must not be read (values a plan would visibly react to)."""
    B = len(kws)
    out, flags = {}, np.zeros(B, np.int32)
    for k, bit, shape, fill in (("init_mu_rows", FLAG_MU, (H, a), 0.77), ("init_sigma_rows", FLAG_SIGMA, (H, a), 0.33),
                                ("carry_in", FLAG_CARRY, (Kc, H, a), -0.6)):
        if all(kw.get(k) is None for kw in kws):
            out[k] = None
            continue
        out[k] = np.stack([np.full(shape, fill, F32) if kw.get(k) is None else np.asarray(kw[k], F32) for kw in kws])
        flags |= np.array([0 if kw.get(k) is None else bit for kw in kws], np.int32)
    out["flags"] = flags
    return out


# ---------------------------------------------------------------------------------------------
# The GPU test's fixture batches (tests/test_gpu_cem_rh_batch.py), shared with the host test that asserts
# their gap condition (tests/test_cem_rh_batch_host.py). The single plan's small shapes: s = 5, H = 3, K = 8,
# I = 3. (W, L, a, N, E, Kc, per-problem inputs, seed): every value of every axis -- B = 1, 2, 3, 5 is the
# length of the inputs tuple; "m", "s", "c" name the inputs a problem is given (mean rows, sigma rows,
# carry), "" a problem that plans cold (all its flag bits clear). N = 100: the B N = 300 or 500 candidates
# align to neither the 8- nor the 16-candidate tiles, so tiles straddle problems. Each seed was found by a
# search on the CPU (find_seed): every problem's K-th and Kc-th return gaps exceed GAP_MIN at every
# iteration of the restatement, ten times the 1e-5 return bar.
# ---------------------------------------------------------------------------------------------
CASES = [
    (64, 1, 1, 64, 1, 0, ("",), 4),                              # B = 1, nothing given
    (256, 2, 5, 100, 2, 0, ("ms", "ms", "ms"), 1),               # keep == 0 with rows: the first launch alone differs
    (64, 1, 8, 100, 1, 1, ("", "mc"), 1),                        # problem 0 cold, a later one warm with carry
    (256, 2, 1, 64, 2, 3, ("msc", "", "m"), 64),                 # problem 0 warm with carry, later ones cold
    (64, 1, 5, 100, 1, 3, ("msc",) * 5, 1),                      # all given
    (256, 2, 8, 64, 1, 8, ("", ""), 1),                          # Kc = K, none given
    (64, 1, 8, 64, 2, 8, ("c", "", "msc", "s", "m"), 5),
    (256, 2, 5, 100, 1, 1, ("msc",), 0),                         # B = 1, all given
    (64, 1, 1, 100, 2, 3, ("msc", "msc"), 12),
    (256, 2, 8, 100, 2, 0, ("m", "", "s", "ms", ""), 6),         # keep == 0, mixed rows
    (64, 1, 5, 64, 1, 1, ("", "", ""), 0),
    (256, 2, 1, 100, 1, 8, ("", "c", "msc"), 23),
]


def case_id(case):
    W, L, a, N, E, Kc, inputs, _ = case
    return f"W{W}-L{L}-a{a}-N{N}-E{E}-Kc{Kc}-B{len(inputs)}-" + "+".join(x or "0" for x in inputs)


make_case = rh.make_batch   # (problem, s0s [B, s], kws) of one fixture batch


def case_plans(case):
    """The restatement's B plans of a fixture batch."""
    W, L, a, N, E, Kc, inputs, _ = case
    p, s0s, kws = make_case(case)
    return plan_batch(p, s0s, N, SMALL["H"], SMALL["K"], SMALL["I"], Kc, kws)


def case_gap(case):
    """The smallest K-th / Kc-th return gap over the batch's problems and iterations."""
    Kc = case[5]
    return min(rh.case_gaps(res, SMALL["K"], Kc) for res in case_plans(case))


def find_seed(case, limit=400):
    """The first seed at which case_gap exceeds GAP_MIN (how the table's seeds were found)."""
    for seed in range(limit):
        c = case[:-1] + (seed,)
        if case_gap(c) > GAP_MIN:
            return seed
    raise RuntimeError(f"no seed below {limit} for {case_id(case)}")


_PLANS = {}


def cached_plans(case):
    """case_plans, computed once per session and shared (read only) by the tests that need it."""
    if case not in _PLANS:
        _PLANS[case] = case_plans(case)
    return _PLANS[case]
