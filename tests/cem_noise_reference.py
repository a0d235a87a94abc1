"""Coloured-noise proposals (include/mbrl_cem.h mbrl_sample_actions_mixed, mbrl_cem_plan_rh_mixed,
mbrl_cem_plan_rh_batch_mixed) restated in NumPy from the oracle's own pieces -- oracle.philox.cem_normals for the
white normals, oracle.cem for the rollout, selection and refit -- and cem_rh_reference's helpers. TEST
INFRASTRUCTURE ONLY: the checker for csrc/cem_noise.hip and the mixed plan loops.

Semantics (normative, DESIGN.md "Coloured-noise proposals"): with z[u] the white normals of Philox counter
(n, u, i, d >> 2) and C the plan's [H, H] float32 mix,
    e[t] = (..((C[t][0] z[0]) + C[t][1] z[1]) + ..) + C[t][H-1] z[H-1]
every product rounded to float32 before it is added, the additions sequential in u; the action is
clip(mu[t] + sigma[t] e[t]). Everything else is cem_rh_reference.plan's: kept slots, the two selections, the
refit, the kept rows. mix = None is the plain path (that module's functions, called as they are)."""
import numpy as np

import cem_rh_reference as rh
from cem_rh_reference import clip_keep_nan, gaps  # noqa: F401  (gaps: re-exported for the tests)
from oracle import cem as ocem
from oracle.philox import cem_actions, cem_normals

F32 = np.float32
GAP_MIN = rh.GAP_MIN


def mixed_normals(mix, seed, it, n_idx, H, a):
    """e[t, j, d] for candidates n_idx[j]: float32 [H, len(n_idx), a]. mix None: the white normals."""
    z = cem_normals(seed, it, n_idx, H, a)
    if mix is None:
        return z
    C = np.asarray(mix, F32)
    assert C.shape == (H, H)
    e = np.empty_like(z)
    for t in range(H):
        acc = (C[t, 0] * z[0]).astype(F32)
        for u in range(1, H):
            acc = (acc + (C[t, u] * z[u]).astype(F32)).astype(F32)
        e[t] = acc
    return e


def mixed_actions(mu, sigma, lo, hi, seed, it, n_idx, mix=None):
    """oracle.philox.cem_actions with the mixed noise (mix None: that function itself)."""
    if mix is None:
        return cem_actions(mu, sigma, lo, hi, seed, it, n_idx)
    mu, sigma = np.asarray(mu, F32), np.asarray(sigma, F32)
    H, a = mu.shape
    eps = mixed_normals(mix, seed, it, n_idx, H, a)
    x = (mu[:, None, :] + (sigma[:, None, :] * eps).astype(F32)).astype(F32)
    return np.minimum(np.maximum(x, F32(lo)), F32(hi)).astype(F32)


def proposals(mu, sigma, lo, hi, seed, it, N, kept=None, mix=None, b=0):
    """Iteration `it`'s proposals [H, N, a] of problem b (candidate indices b N + arange(N)): the mixed draw
    with slots [0, Kc) replaced by clip(kept)."""
    if mix is None and b == 0:
        return rh.proposals(mu, sigma, lo, hi, seed, it, N, kept)
    A = mixed_actions(mu, sigma, lo, hi, seed, it, b * N + np.arange(N), mix)
    if kept is not None and len(kept):
        A[:, :len(kept), :] = clip_keep_nan(kept, lo, hi).transpose(1, 0, 2)
    return A


def plan(problem, N, H, K, I, *, mix=None, keep=0, init_mu_rows=None, init_sigma_rows=None, carry_in=None, b=0,
         s0=None, final=True):
    """cem_rh_reference.plan with a mix: the same outputs. b, s0: problem b of a batch (its Philox candidate
    indices are b N + arange(N), its initial state s0), as cem_rh_batch_reference.plan_problem. mix None with
    b == 0 and no s0 calls cem_rh_reference.plan itself."""
    if mix is None and b == 0 and s0 is None:
        return rh.plan(problem, N, H, K, I, keep=keep, init_mu_rows=init_mu_rows, init_sigma_rows=init_sigma_rows,
                       carry_in=carry_in, final=final)
    d = ocem.CEM_DEFAULTS
    alpha, lo, hi = d["alpha"], d["lo"], d["hi"]
    a = problem["cfg"]["a"]
    Kc = int(keep)
    assert 0 <= Kc <= K and (carry_in is None or Kc > 0)
    s0 = np.asarray(problem["s0"] if s0 is None else s0, F32)
    mu = np.zeros((H, a), F32) if init_mu_rows is None else \
        np.clip(np.asarray(init_mu_rows, F32), F32(lo), F32(hi)).astype(F32)
    sigma = np.full((H, a), F32((hi - lo) / 4.0), F32) if init_sigma_rows is None else \
        np.asarray(init_sigma_rows, F32).copy()
    kept = None if carry_in is None else np.asarray(carry_in, F32).reshape(Kc, H, a)
    out = dict(costs=[], returns=[], elites=[], best=[], actions=[], mu=[], sigma=[], mu0=mu, sigma0=sigma,
               kept=[np.zeros((Kc, H, a), F32) if kept is None else kept.copy()])
    for it in range(I):
        A = proposals(mu, sigma, lo, hi, problem["rng_seed"], it, N, kept if Kc else None, mix, b)
        costs = ocem.rollout(problem["model"], problem["norm"], problem["cost"], s0, A)
        ret = ocem.ensemble_returns(costs)
        elites = ocem.select_elites(ret, K)
        best = ocem.select_elites(ret, Kc) if Kc else np.zeros(0, np.int64)
        mu, sigma = ocem.refit(mu, sigma, np.ascontiguousarray(A[:, elites, :].transpose(1, 0, 2)), alpha)
        kept = np.ascontiguousarray(A[:, best, :].transpose(1, 0, 2))
        for k, v in dict(costs=costs, returns=ret, elites=elites, best=best, actions=A, mu=mu, sigma=sigma).items():
            out[k].append(v)
        out["kept"].append(kept.copy())
    out.update(mu_out=mu, sigma_out=sigma, carry=kept, carry_returns=out["returns"][-1][out["best"][-1]],
               final_actions=np.clip(mu, F32(lo), F32(hi)).astype(F32))
    if final:
        _, states = ocem.rollout(problem["model"], problem["norm"], problem["cost"], s0,
                                 out["final_actions"][:, None, :], store_states=True)
        out["final_states"] = np.mean(states[:, :, 0, :], axis=0, dtype=F32) if len(problem["model"]) > 1 \
            else states[0, :, 0, :]
    return out


def plan_batch(problem, s0s, N, H, K, I, keep, kws, mix, final=True):
    """The B plans of a batch, per problem: kws[b] holds problem b's optional inputs."""
    return [plan(problem, N, H, K, I, mix=mix, keep=keep, b=b, s0=s0s[b], final=final, **kws[b])
            for b in range(len(kws))]


def closed_loop(problem, steps, N, H, K, I, *, mix=None, keep=0, warm=False, shift=1, seed0=0):
    """cem_rh_reference.closed_loop with a mix (the same protocol and the same per-step seeds)."""
    from mbrl_amd.planners import cem_shift_carry, mppi_warm_start_rows
    p = dict(problem)
    s = np.asarray(problem["s0"], F32)
    lo, hi = ocem.CEM_DEFAULTS["lo"], ocem.CEM_DEFAULTS["hi"]
    rows = carry = None
    total = 0.0
    for step in range(steps):
        p["s0"], p["rng_seed"] = s, seed0 + step
        res = plan(p, N, H, K, I, mix=mix, keep=keep, init_mu_rows=rows, carry_in=carry, final=False)
        act = res["final_actions"]
        if warm:
            rows = mppi_warm_start_rows(act, H, shift, lo, hi)
            carry = cem_shift_carry(res["carry"], shift, lo, hi) if keep else None
        s = ocem.dynamics_step(problem["model"][0], problem["norm"], s[None, :], act[:1])[0]
        total += float(ocem.goal_state_cost(s[None, :], act[:1], problem["cost"])[0])
    return total


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
    W, L, a, N, E, Kc, inputs, H, seed = case
    p = ocem.synth_problem(2, seed=7600 + seed, W=W, L=L, a=a, E=E, N=N, H=H)
    rng = np.random.default_rng(seed)
    kw = dict(keep=Kc)
    if "mu" in inputs:
        kw["init_mu_rows"] = rng.uniform(-1.3, 1.3, (H, a)).astype(F32)
    if "sigma" in inputs:
        kw["init_sigma_rows"] = rng.uniform(0.1, 0.6, (H, a)).astype(F32)
    if "carry" in inputs:
        kw["carry_in"] = rng.uniform(-1.2, 1.2, (Kc, H, a)).astype(F32)
    return p, beta_mix(H), kw


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
    W, L, a, N, E, Kc, inputs, H, seed = case
    p = ocem.synth_problem(2, seed=7900 + seed, W=W, L=L, a=a, E=E, N=N, H=H)
    rng = np.random.default_rng(seed)
    B = len(inputs)
    s0s = np.stack([p["s0"]] + [(p["s0"] + rng.normal(0.0, 0.2, p["s0"].shape)).astype(F32) for _ in range(B - 1)])
    kws = []
    for given in inputs:
        kw = {}
        if "m" in given:
            kw["init_mu_rows"] = rng.uniform(-1.3, 1.3, (H, a)).astype(F32)
        if "s" in given:
            kw["init_sigma_rows"] = rng.uniform(0.1, 0.6, (H, a)).astype(F32)
        if "c" in given:
            assert Kc > 0
            kw["carry_in"] = rng.uniform(-1.2, 1.2, (Kc, H, a)).astype(F32)
        kws.append(kw)
    return p, s0s.astype(F32), beta_mix(H), kws


def batch_case_plans(case, final=False):
    p, s0s, mix, kws = make_batch_case(case)
    return plan_batch(p, s0s, case[3], case[7], SMALL["K"], SMALL["I"], case[5], kws, mix, final=final)


def batch_case_gap(case):
    return min(rh.case_gaps(res, SMALL["K"], case[5]) for res in batch_case_plans(case))


_PLANS = {}


def cached(fn, case, **kw):
    """fn(case, **kw), computed once per session and shared (read only) by the tests that need it."""
    key = (fn.__name__, case, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = fn(case, **kw)
    return _PLANS[key]
