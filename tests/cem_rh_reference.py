"""Receding-horizon CEM (warm start and elite carry-over; include/mbrl_cem.h mbrl_cem_plan_rh, its batched
form mbrl_cem_plan_rh_batch and their _mixed forms with coloured noise) restated ONCE in NumPy from the
oracle's own pieces -- oracle.cem.rollout / ensemble_returns / select_elites / refit and oracle.philox.cem_actions
/ cem_normals. TEST INFRASTRUCTURE ONLY: the checker for csrc/cem_rh.hip, csrc/cem_noise.hip and the plan loop.
cem_rh_batch_reference and cem_noise_reference hold the batched and the mixed fixtures and call plan() here.

Semantics (normative, DESIGN.md "Receding-horizon CEM"):
  * mu0[t] = clip(init_mu_rows[t]) or init_mu; sigma0[t] = init_sigma_rows[t] or init_sigma.
  * Iteration i, candidate n < Kc takes clip(kept_i[n]) when a kept set exists (i >= 1, or i == 0 with
    carry_in = kept_0); every other candidate is the plain draw, Philox counter (n, t, i, d >> 2). The counter
    space does not move: candidates n >= Kc are what the plain plan draws from the same mu / sigma.
  * After the rollout: elites = stable top-K (NaN last, ascending index), best = stable top-Kc of the same
    returns; refit over the elites' action rows; kept_{i+1}[j] = the action rows of best[j].
  * Problem b of a batch is this plan from its own s0 with Philox candidate indices b N + n.
  * With a mix C [H, H] the draw's noise is e[t] = (..((C[t][0] z[0]) + C[t][1] z[1]) + ..) + C[t][H-1] z[H-1] over
    the white normals z[u] of counter (n, u, i, d >> 2), every product and sum rounded to float32 (DESIGN.md
    "Coloured-noise proposals").
A NaN in a kept row stays NaN through the clip, so the row's return is NaN and it sorts last."""
import numpy as np

from oracle import cem as ocem
from oracle.philox import cem_actions, cem_normals

F32 = np.float32


def clip_keep_nan(x, lo, hi):
    """clip that hands a NaN through (np.minimum / np.maximum propagate it)."""
    return np.minimum(np.maximum(np.asarray(x, F32), F32(lo)), F32(hi)).astype(F32)


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
    """Iteration `it`'s proposals [H, N, a] of problem b (Philox candidate indices b N + arange(N)): the draw
    (mixed where a mix is given) with slots [0, Kc) replaced by clip(kept)."""
    A = mixed_actions(mu, sigma, lo, hi, seed, it, b * N + np.arange(N), mix)
    if kept is not None and len(kept):
        A[:, :len(kept), :] = clip_keep_nan(kept, lo, hi).transpose(1, 0, 2)
    return A


def plan(problem, N, H, K, I, *, keep=0, init_mu_rows=None, init_sigma_rows=None, carry_in=None, alpha=None,
         lo=None, hi=None, init_sigma=None, final=True, mix=None, b=0, s0=None, seed=None):
    """The whole plan on an oracle.cem.synth_problem: the one restatement of the single, the batched and the
    mixed plans. mix: the [H, H] noise mix (None: white). b, s0, seed: problem b of a batch -- its Philox
    candidate indices are b N + arange(N), its initial state s0 -- and the plan's Philox seed (defaults: the
    problem's own). Returns per-iteration lists costs, returns, elites, best, actions (the proposals), mu,
    sigma; kept ([I + 1] sets, kept[0] = carry_in or zeros); the outputs mu_out, sigma_out, carry,
    carry_returns, final_actions and (final=True) final_states."""
    d = ocem.CEM_DEFAULTS
    alpha = d["alpha"] if alpha is None else alpha
    lo = d["lo"] if lo is None else lo
    hi = d["hi"] if hi is None else hi
    a = problem["cfg"]["a"]
    Kc = int(keep)
    assert 0 <= Kc <= K and (carry_in is None or Kc > 0)
    s0 = problem["s0"] if s0 is None else np.asarray(s0, F32)
    seed = problem["rng_seed"] if seed is None else seed
    if init_mu_rows is None:
        mu = np.zeros((H, a), F32)
    else:
        mu = np.clip(np.asarray(init_mu_rows, F32), F32(lo), F32(hi)).astype(F32)
    if init_sigma_rows is None:
        sigma = np.full((H, a), F32((hi - lo) / 4.0) if init_sigma is None else F32(init_sigma), F32)
    else:
        sigma = np.asarray(init_sigma_rows, F32).copy()
    kept = None if carry_in is None else np.asarray(carry_in, F32).reshape(Kc, H, a)
    out = dict(costs=[], returns=[], elites=[], best=[], actions=[], mu=[], sigma=[], mu0=mu, sigma0=sigma,
               kept=[np.zeros((Kc, H, a), F32) if kept is None else kept.copy()])
    for it in range(I):
        A = proposals(mu, sigma, lo, hi, seed, it, N, kept if Kc else None, mix, b)
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


def gaps(ret, ks):
    """The relative gap between the k-th and (k + 1)-th smallest return for each k in ks (0 < k < N):
    what lets a test demand identical index sets from costs that agree to 1e-5."""
    srt = np.sort(np.asarray(ret, np.float64))
    return [float((srt[k] - srt[k - 1]) / max(abs(srt[k - 1]), 1.0)) for k in ks if 0 < k < len(srt)]


def closed_loop(problem, steps, N, H, K, I, *, keep=0, warm=False, shift=1, seed0=0, mix=None):
    """`steps` control steps with the synthetic model as its own environment (member 0): plan, apply the
    first action, pay goal_state_cost at the state reached. warm: the next plan starts from the previous
    plan's actions and carry, each shifted by `shift` (last row repeated). Each step plans with its own
    Philox seed (seed0 + step); mix: every plan's noise mix. Returns the summed realised cost (float64 sum of
    the float32 costs)."""
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


# ---------------------------------------------------------------------------------------------
# The GPU test's fixture problems (tests/test_gpu_cem_rh.py), shared with the host test that asserts
# their gap condition (tests/test_cem_rh_host.py). Small shapes: s = 5, H = 3, K = 8, I = 3.
# (W, L, a, N, E, Kc, inputs, seed): every value of every axis, each input combination -- "mu", "sigma",
# "carry" name the optional inputs given -- and a seed at which every iteration's K-th and Kc-th return
# gaps exceed GAP_MIN on the restatement (searched once; the host test asserts it).
# ---------------------------------------------------------------------------------------------
GAP_MIN = 1e-4     # ten times the project's 1e-5 return bar
SMALL = dict(s=5, H=3, K=8, I=3)
CASES = [
    (64, 1, 1, 64, 1, 0, (), 24),
    (64, 1, 5, 100, 2, 0, ("mu",), 2),
    (256, 2, 8, 64, 1, 0, ("sigma",), 5),
    (256, 2, 1, 100, 2, 0, ("mu", "sigma"), 1),
    (64, 1, 8, 100, 1, 1, (), 1),
    (64, 1, 5, 64, 2, 1, ("carry",), 2),
    (256, 2, 1, 64, 1, 3, ("mu", "sigma", "carry"), 12),
    (256, 2, 5, 100, 1, 3, ("mu",), 2),
    (64, 1, 8, 64, 2, 3, ("carry",), 3),
    (256, 2, 8, 100, 2, 8, ("mu", "sigma", "carry"), 1),
    (64, 1, 5, 100, 1, 8, ("sigma",), 4),
    (256, 2, 5, 64, 2, 8, (), 2),
    (64, 1, 1, 100, 1, 3, ("sigma",), 250),
    (256, 2, 1, 100, 2, 1, ("mu", "sigma", "carry"), 1),
    (256, 2, 8, 64, 1, 1, ("mu",), 3),
    (64, 1, 1, 64, 2, 8, ("carry",), 13),
]


def case_id(case):
    W, L, a, N, E, Kc, inputs, _ = case
    return f"W{W}-L{L}-a{a}-N{N}-E{E}-Kc{Kc}-" + ("+".join(inputs) or "none")


def draw_inputs(rng, H, a, Kc, mu, sigma, carry):
    """A problem's optional inputs (plan()'s keywords), those asked for, drawn in this order from rng: some mean
    and carry entries lie outside the bounds."""
    kw = {}
    if mu:
        kw["init_mu_rows"] = rng.uniform(-1.3, 1.3, (H, a)).astype(F32)
    if sigma:
        kw["init_sigma_rows"] = rng.uniform(0.1, 0.6, (H, a)).astype(F32)
    if carry:
        assert Kc > 0
        kw["carry_in"] = rng.uniform(-1.2, 1.2, (Kc, H, a)).astype(F32)
    return kw


def make_case(case, H=SMALL["H"], seed0=7000):
    """(problem, kwargs of plan()) of one fixture case: the synthetic cartpole problem with the case's
    shape, and its optional inputs drawn from the case seed."""
    W, L, a, N, E, Kc, inputs, seed = case
    p = ocem.synth_problem(2, seed=seed0 + seed, W=W, L=L, a=a, E=E, N=N, H=H)
    kw = draw_inputs(np.random.default_rng(seed), H, a, Kc, *(k in inputs for k in ("mu", "sigma", "carry")))
    return p, dict(keep=Kc, **kw)


def make_batch(case, H=SMALL["H"], seed0=7300):
    """(problem, s0s [B, s], kws) of one fixture batch -- inputs: per problem a string of "m", "s", "c" for the
    inputs it is given: the synthetic cartpole problem with the case's shape (problem 0 starts from its s0, the
    others from perturbed copies) and each problem's optional inputs drawn from the case seed."""
    W, L, a, N, E, Kc, inputs, seed = case
    p = ocem.synth_problem(2, seed=seed0 + seed, W=W, L=L, a=a, E=E, N=N, H=H)
    rng = np.random.default_rng(seed)
    B = len(inputs)
    s0s = np.stack([p["s0"]] + [(p["s0"] + rng.normal(0.0, 0.2, p["s0"].shape)).astype(F32) for _ in range(B - 1)])
    return p, s0s.astype(F32), [draw_inputs(rng, H, a, Kc, *(k in given for k in "msc")) for given in inputs]


def case_gaps(res, K, Kc):
    """The smallest K-th and Kc-th return gap over a plan's iterations."""
    return min(min(gaps(r, [k for k in (K, Kc) if k]), default=np.inf) for r in res["returns"])
