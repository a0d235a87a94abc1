"""NumPy restatement of the MPPI update (include/mbrl_cem.h "MPPI", DESIGN.md "MPPI") for the tests.

The returns, beta and x_n = (r_n - beta) / lambda are float32 with the device's operations, so they
match it bit for bit; the exponentials and the sums are float64 (`update`). `update_f32` is the same
update in float32 in the documented summation order (`canonical_sum`), with the chain length of that
order counted as it runs; `chain_depth` is the closed form D the test tolerance is built on.
`plan` drives whole plans with oracle.philox's proposals and oracle.cem's rollout and cost.
"""
import numpy as np

from oracle import cem as ocem
from oracle.philox import cem_actions

F32 = np.float32
CHUNK = ocem.ELITE_CHUNK   # 32
U = 2.0 ** -24             # float32 unit roundoff


def returns_of(costs):
    """Member-mean returns, as the selection forms them (sequential in e, / E; costs[0] when E == 1)."""
    return ocem.ensemble_returns(np.asarray(costs, F32))


def beta_of(r):
    """Minimum over the finite returns (a zero of either sign is +0.0); NaN when none is finite."""
    ok = np.isfinite(r)
    if not ok.any():
        return F32(np.nan)
    b = F32(np.min(r[ok]))
    return F32(0.0) if b == 0 else b


def exponents(r, beta, lam):
    """x_n = (r_n - beta) / lambda in float32 (one subtraction, one division); inf where r_n is invalid."""
    ok = np.isfinite(r)
    x = np.full(r.shape, np.inf, F32)
    with np.errstate(all="ignore"):
        x[ok] = ((r[ok] - beta).astype(F32) / F32(lam)).astype(F32)
    return x


def weights_of(costs, lam):
    """(returns f32, beta f32, weights f64): w_n = exp(-x_n) for valid n, else 0."""
    r = returns_of(costs)
    beta = beta_of(r)
    if np.isnan(beta):
        return r, beta, np.zeros(r.shape, np.float64)
    x = exponents(r, beta, lam)
    w = np.where(np.isfinite(r), np.exp(-x.astype(np.float64)), 0.0)
    return r, beta, w


def update(costs, actions, mu, sigma, lam, alpha, update_sigma):
    """Steps 1-6 with float64 exponentials and sums. actions [H, N, a]; mu, sigma [H, a] float32.
    Returns dict(returns, beta, eta, weights, m, v, mu, var, sigma): mu / var / sigma are the smoothed
    results in float64 (var = sigma ** 2 before the square root; None without update_sigma)."""
    mu, sigma = np.asarray(mu, F32), np.asarray(sigma, F32)
    r, beta, w = weights_of(costs, lam)
    out = dict(returns=r, beta=beta, weights=w)
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
        sg_new = np.sqrt(var)
    out.update(eta=eta, m=m, v=v, mu=mu_new, var=var, sigma=sg_new, unchanged=False)
    return out


def canonical_sum(x, track=None):
    """The documented order over axis 0 in float32: chunks of 32 consecutive entries summed
    sequentially, then the chunk partials again in chunks of 32, until one value is left. A last,
    short chunk sums its real entries only. track (a one-element list) receives the number of
    additions on the longest dependent chain."""
    x = np.asarray(x, F32)
    depth = np.zeros(x.shape[0], np.int64)
    while True:
        n = x.shape[0]
        parts, pdepth = [], []
        for c0 in range(0, n, CHUNK):
            acc, d = x[c0].copy(), depth[c0]
            for i in range(c0 + 1, min(c0 + CHUNK, n)):
                acc = (acc + x[i]).astype(F32)
                d = max(d, depth[i]) + 1
            parts.append(acc)
            pdepth.append(d)
        x, depth = np.stack(parts), np.asarray(pdepth)
        if x.shape[0] == 1:
            break
    if track is not None:
        track[0] = int(depth[0])
    return x[0]


def chain_depth(N):
    """D: additions on the longest dependent chain of canonical_sum over N entries (<= 93 for N <= 32768)."""
    D, n = 0, int(N)
    while True:
        D += min(n, CHUNK) - 1
        n = (n + CHUNK - 1) // CHUNK
        if n == 1:
            return D


def mu_bound(N, lo, hi):
    """|mu_out - reference| <= (D + 8) 2^-24 max(|lo|, |hi|): D additions of the documented order; 8 for
    the exp allowance, the product, the division and the smoothing."""
    return (chain_depth(N) + 8) * U * max(abs(lo), abs(hi))


def var_bound(N, lo, hi):
    """The same bound for the smoothed variance (before the square root), scaled by (hi - lo)^2."""
    return (chain_depth(N) + 8) * U * (hi - lo) ** 2


def update_f32(costs, actions, mu, sigma, lam, alpha, update_sigma):
    """The update in float32 in the device's order (its expf replaced by the correctly rounded
    exponential). Returns (mu', sigma')."""
    mu, sigma = np.asarray(mu, F32), np.asarray(sigma, F32)
    r, beta, w64 = weights_of(costs, lam)
    if np.isnan(beta):
        return mu.copy(), sigma.copy()
    w = w64.astype(F32)
    A = np.asarray(actions, F32)
    H, N, a = A.shape
    eta = canonical_sum(w)
    a_, oma = F32(alpha), F32(1) - F32(alpha)
    mu_new, sg_new = np.empty_like(mu), sigma.copy()
    for t in range(H):
        m = (canonical_sum((w[:, None] * A[t]).astype(F32)) / eta).astype(F32)
        mu_new[t] = ((a_ * mu[t]).astype(F32) + (oma * m).astype(F32)).astype(F32)
        if update_sigma:
            df = (A[t] - m).astype(F32)
            v = (canonical_sum((w[:, None] * (df * df).astype(F32)).astype(F32)) / eta).astype(F32)
            var = ((a_ * (sigma[t] * sigma[t]).astype(F32)).astype(F32) + (oma * v).astype(F32)).astype(F32)
            sg_new[t] = np.sqrt(var).astype(F32)
    return mu_new, sg_new


def warm_rows(prev_actions, H, shift, lo, hi):
    """Hand-written warm start: drop `shift` rows, repeat the last, clip."""
    rows = [np.asarray(r, F32) for r in prev_actions][shift:]
    while len(rows) < H:
        rows.append(rows[-1])
    return np.clip(np.stack(rows[:H]), F32(lo), F32(hi)).astype(F32)


def plan(problem, N, H, I, lam, alpha=0.0, update_sigma=False, lo=-1.0, hi=1.0, init_rows=None):
    """Whole MPPI plan on an oracle.cem.synth_problem: oracle.philox proposals, oracle.cem rollout and
    cost, `update` (float64 sums; the carried mu / sigma are rounded to float32 each iteration)."""
    a = problem["cfg"]["a"]
    mu = np.zeros((H, a), F32) if init_rows is None else np.clip(np.asarray(init_rows, F32), F32(lo), F32(hi))
    sigma = np.full((H, a), F32((hi - lo) / 4.0), F32)
    out = dict(costs=[], weights=[], mu_hist=[mu], sigma_hist=[sigma])
    for it in range(I):
        A = cem_actions(mu, sigma, lo, hi, problem["rng_seed"], it, np.arange(N))
        costs = ocem.rollout(problem["model"], problem["norm"], problem["cost"], problem["s0"], A)
        u = update(costs, A, mu, sigma, lam, alpha, update_sigma)
        mu, sigma = u["mu"].astype(F32), u["sigma"].astype(F32)
        out["costs"].append(costs)
        out["weights"].append(u["weights"])
        out["mu_hist"].append(mu)
        out["sigma_hist"].append(sigma)
    actions = np.clip(mu, F32(lo), F32(hi)).astype(F32)
    _, states = ocem.rollout(problem["model"], problem["norm"], problem["cost"], problem["s0"], actions[:, None, :],
                             store_states=True)
    out["actions"] = actions
    out["states"] = np.mean(states[:, :, 0, :], axis=0, dtype=F32) if len(problem["model"]) > 1 else states[0, :, 0, :]
    return out
