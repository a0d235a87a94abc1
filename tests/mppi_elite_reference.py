"""NumPy restatement of MPPI over the K best (include/mbrl_cem.h "MPPI over the K best") for the tests:
tests/mppi_reference.py's update with a mask.

The elite set is the stable top-K of the float32 member-mean returns (oracle.cem.select_elites: np.argsort(kind=
"stable")[:K], ascending index); a candidate is valid iff it is an elite and its return is finite; beta is the
minimum over the valid returns and every other weight is 0. The sums still run over all N candidates -- the zero
weights take part as zeros -- so `update_f32` is mppi_reference's canonical order unchanged, and with update_sigma
the new sigma is clamped to [sigma_min, sigma_max]. `update` has float64 exponentials and sums; `plan` drives whole
plans; the fixtures' seeds are picked so that the reference's own K-th and (K+1)-th returns are far enough apart
(`find_seed`) for a device plan to select the same set.
"""
import numpy as np

import mppi_reference as mref
from oracle import cem as ocem
from oracle.philox import cem_actions

F32 = np.float32
GAP_MIN = 1e-4   # least relative gap between the K-th and the (K+1)-th return at every iteration of a fixture


def elite_set(r, K):
    """The K smallest (r_n, n) pairs, NaN last, as ascending candidate indices (int64)."""
    return ocem.select_elites(r, K)


def valid_mask(r, K):
    """n is valid iff it is an elite and r_n is finite."""
    m = np.zeros(r.shape, bool)
    m[elite_set(r, K)] = True
    return m & np.isfinite(r)


def weights_of(costs, lam, K):
    """(returns f32, beta f32, weights f64, elites): w_n = exp(-x_n) for valid n, else 0; beta over the valid."""
    r = mref.returns_of(costs)
    ok = valid_mask(r, K)
    el = elite_set(r, K)
    if not ok.any():
        return r, F32(np.nan), np.zeros(r.shape, np.float64), el
    b = F32(np.min(r[ok]))
    beta = F32(0.0) if b == 0 else b
    x = np.full(r.shape, np.inf, F32)
    with np.errstate(all="ignore"):
        x[ok] = ((r[ok] - beta).astype(F32) / F32(lam)).astype(F32)
    w = np.where(ok, np.exp(-x.astype(np.float64)), 0.0)
    return r, beta, w, el


def clamp(sg, sigma_min, sigma_max):
    return np.minimum(np.maximum(sg, sg.dtype.type(sigma_min)), sg.dtype.type(sigma_max))


def update(costs, actions, mu, sigma, lam, alpha, update_sigma, K, sigma_min=0.0, sigma_max=np.inf):
    """mppi_reference.update with the mask and the clamp (float64 exponentials and sums). Adds `elites`; `var` is
    the smoothed variance BEFORE the clamp, `sigma` after it (the clamp bounds as float32 values)."""
    mu, sigma = np.asarray(mu, F32), np.asarray(sigma, F32)
    r, beta, w, el = weights_of(costs, lam, K)
    out = dict(returns=r, beta=beta, weights=w, elites=el)
    if np.isnan(beta):
        out.update(eta=0.0, m=None, v=None, mu=mu.astype(np.float64), sigma=sigma.astype(np.float64),
                   var=(sigma.astype(np.float64) ** 2 if update_sigma else None), unchanged=True)
        return out
    A = np.asarray(actions, F32).astype(np.float64)
    eta = w.sum()
    m = np.einsum("n,tnd->td", w, A) / eta
    a_ = float(F32(alpha))
    oma = float(F32(1) - F32(alpha))
    mu_new = a_ * mu.astype(np.float64) + oma * m
    v = var = None
    sg_new = sigma.astype(np.float64)
    if update_sigma:
        v = np.einsum("n,tnd->td", w, (A - m[:, None, :]) ** 2) / eta
        var = a_ * sigma.astype(np.float64) ** 2 + oma * v
        sg_new = clamp(np.sqrt(var), float(F32(sigma_min)), float(F32(sigma_max)))
    out.update(eta=eta, m=m, v=v, mu=mu_new, var=var, sigma=sg_new, unchanged=False)
    return out


def update_f32(costs, actions, mu, sigma, lam, alpha, update_sigma, K, sigma_min=0.0, sigma_max=np.inf):
    """mppi_reference.update_f32 with the mask and the clamp: float32 in the device's order. (mu', sigma')."""
    mu, sigma = np.asarray(mu, F32), np.asarray(sigma, F32)
    r, beta, w64, _ = weights_of(costs, lam, K)
    if np.isnan(beta):
        return mu.copy(), sigma.copy()
    w = w64.astype(F32)
    A = np.asarray(actions, F32)
    H = A.shape[0]
    eta = mref.canonical_sum(w)
    a_, oma = F32(alpha), F32(1) - F32(alpha)
    mu_new, sg_new = np.empty_like(mu), sigma.copy()
    for t in range(H):
        m = (mref.canonical_sum((w[:, None] * A[t]).astype(F32)) / eta).astype(F32)
        mu_new[t] = ((a_ * mu[t]).astype(F32) + (oma * m).astype(F32)).astype(F32)
        if update_sigma:
            df = (A[t] - m).astype(F32)
            v = (mref.canonical_sum((w[:, None] * (df * df).astype(F32)).astype(F32)) / eta).astype(F32)
            var = ((a_ * (sigma[t] * sigma[t]).astype(F32)).astype(F32) + (oma * v).astype(F32)).astype(F32)
            sg_new[t] = clamp(np.sqrt(var).astype(F32), sigma_min, sigma_max)
    return mu_new, sg_new


def boundary_gap(r, K):
    """Relative gap between the K-th and the (K+1)-th smallest return (inf when K == N or one is not finite)."""
    s = np.sort(np.asarray(r, F32))
    if K >= s.shape[0] or not (np.isfinite(s[K - 1]) and np.isfinite(s[K])):
        return np.inf
    return float((np.float64(s[K]) - np.float64(s[K - 1])) / max(abs(np.float64(s[K])), abs(np.float64(s[K - 1])), 1.0))


def plan(problem, N, H, I, lam, K, alpha=0.0, update_sigma=False, sigma_min=0.0, sigma_max=np.inf, lo=-1.0, hi=1.0,
         init_rows=None, sigma_rows=None):
    """mppi_reference.plan with the restricted update; also records each iteration's elites and boundary gap."""
    a = problem["cfg"]["a"]
    mu = np.zeros((H, a), F32) if init_rows is None else np.clip(np.asarray(init_rows, F32), F32(lo), F32(hi))
    sigma = np.full((H, a), F32((hi - lo) / 4.0), F32) if sigma_rows is None else np.asarray(sigma_rows, F32).copy()
    out = dict(costs=[], weights=[], elites=[], gaps=[], mu_hist=[mu], sigma_hist=[sigma])
    for it in range(I):
        A = cem_actions(mu, sigma, lo, hi, problem["rng_seed"], it, np.arange(N))
        costs = ocem.rollout(problem["model"], problem["norm"], problem["cost"], problem["s0"], A)
        u = update(costs, A, mu, sigma, lam, alpha, update_sigma, K, sigma_min, sigma_max)
        mu, sigma = u["mu"].astype(F32), u["sigma"].astype(F32)
        out["costs"].append(costs)
        out["weights"].append(u["weights"])
        out["elites"].append(u["elites"])
        out["gaps"].append(boundary_gap(u["returns"], K))
        out["mu_hist"].append(mu)
        out["sigma_hist"].append(sigma)
    out["actions"] = np.clip(mu, F32(lo), F32(hi)).astype(F32)
    return out


# Plan-level fixtures: (config id, N, H, I, K, lambda, alpha, update_sigma, sigma_min, sigma_max, problem seed).
# The seeds are the first at which the reference plan's smallest boundary gap is at least GAP_MIN (find_seed).
PLAN_CASES = [
    (3, 300, 4, 2, 30, 2.0, 0.1, True, 0.05, 0.4, 22),
    (5, 128, 3, 2, 12, 1.5, 0.0, True, 0.0, np.inf, 191),    # an ensemble
    (6, 128, 3, 2, 12, 1.5, 0.0, True, 0.0, np.inf, 0),      # the reward head
]


def case_problem(case):
    cid, N, H = case[:3]
    return ocem.synth_problem(cid, N=N, H=H, seed=2000 + case[-1])


def case_plan(case):
    cid, N, H, I, K, lam, alpha, upd, smin, smax, _ = case
    return plan(case_problem(case), N, H, I, lam, K, alpha=alpha, update_sigma=upd, sigma_min=smin, sigma_max=smax)


def case_gap(case):
    return min(case_plan(case)["gaps"])


def find_seed(case, limit=400):
    """The first seed at which the case's smallest boundary gap reaches GAP_MIN (how the table's seeds were found)."""
    for seed in range(limit):
        if case_gap(case[:-1] + (seed,)) >= GAP_MIN:
            return seed
    raise RuntimeError(f"no seed below {limit} for {case[:-1]}")
