"""The sampled rows of the control loop (include/mbrl_cem.h mbrl_rollout_cost_ts_rows, mbrl_cem_plan_ts_rh and its
batch), restated in NumPy. TEST INFRASTRUCTURE ONLY; no GPU import.

  * members(): the RESAMPLED mode's member draw, e(q, t) = (uint64(w.x) * E) >> 32 with w = Philox4x32-10 of counter
    (0, t, q, (iteration << 8) | 0xFF) keyed by the halves of noise_seed (oracle.philox), and its single-mistake
    mutants.
  * restate(): tests/rollout_ts_reference.py's restatement of the nine steps (its normals, model input, bounded
    log-variance and cost, imported) with the member of step 2 drawn per step, at float64 (the reference) or float32
    (the chain that sets the bar). Q rows in all: states [Q][H][N][s], costs [Q][N].
  * plan_given_costs(): the receding-horizon plan of tests/cem_rh_reference.py (its proposals, and
    oracle.cem.ensemble_returns / select_elites / refit) with every iteration's costs supplied from outside instead of
    computed: what the selections, the kept rows and the refit must give from the costs the GPU recorded.
The bars are rollout_ts_reference's: 8 x max(the float32 chain's error of the case, the ten cases' median)."""
import functools

import numpy as np

import rollout_ts_reference as ref
from cem_rh_reference import proposals
from oracle import cem as ocem
from oracle import philox

F32 = np.float32
MEMBER_GROUP = 0xFF        # the group byte of the member draw's counter; the state noise uses j >> 2 < 158
NOISE_GROUPS = 158
MEMBER_MUTANTS = ("member_q_mod_E", "draw_ignores_t", "draw_ignores_q", "draw_ignores_iteration")


def member_counters(iteration, Q, H, mutant=None):
    """The draw's counters, uint32 [Q][H][4]."""
    q, t = np.meshgrid(np.arange(Q, dtype=np.uint32), np.arange(H, dtype=np.uint32), indexing="ij")
    if mutant == "draw_ignores_t":
        t = np.zeros_like(t)
    if mutant == "draw_ignores_q":
        q = np.zeros_like(q)
    it = 0 if mutant == "draw_ignores_iteration" else int(iteration)
    word3 = np.full_like(q, (np.uint32(it) << np.uint32(8)) | np.uint32(MEMBER_GROUP))
    return np.stack([np.zeros_like(q), t, q, word3], axis=-1)


def member_words(seed, iteration, Q, H, mutant=None):
    """w.x of the draw, uint32 [Q][H]."""
    return philox.philox4x32_10(member_counters(iteration, Q, H, mutant), philox.seed_key(seed))[..., 0]


def members(seed, iteration, Q, H, E, mutant=None):
    """e(q, t), int32 [Q][H]."""
    if mutant == "member_q_mod_E":
        return np.repeat((np.arange(Q, dtype=np.int32) % E)[:, None], H, axis=1)
    w = member_words(seed, iteration, Q, H, mutant).astype(np.uint64)
    return ((w * np.uint64(E)) >> np.uint64(32)).astype(np.int32)


def noise_counter_collides(iteration, Q, H, s):
    """Whether any member-draw counter equals a state-noise counter (n + n_offset, t, q, (iteration << 8) | g),
    g < ceil(s / 4), for ANY n + n_offset: the last word alone decides it."""
    groups = (s + 3) // 4
    assert groups <= NOISE_GROUPS
    word3 = member_counters(iteration, Q, H)[..., 3]
    noise3 = (np.uint32(iteration) << np.uint32(8)) | np.arange(groups, dtype=np.uint32)
    return bool(np.isin(word3, noise3).any())


def restate(prob, Q, dtype=np.float64, mutant=None, **override):
    """dict(states [Q][H][N][s], costs [Q][N], members [Q][H], pre: per (q, t, l) the hidden pre-activations) of the
    problem (rollout_ts_reference.problem(name), fields replaced by `override`) in RESAMPLED mode with Q rows, at
    `dtype`."""
    p = dict(prob, **override)
    c = p["case"]
    E, H, N, s = len(p["members"]), p["actions"].shape[0], p["actions"].shape[1], c.s
    norm = ref._norm_as(p["norm"], dtype)
    lo, hi = (np.asarray(b, dtype) for b in p["bounds"])
    actions = np.asarray(p["actions"], dtype)
    s0 = np.asarray(p["s0"], dtype)
    scale = dtype(np.float32(p["noise_scale"]))
    n_idx = np.arange(N, dtype=np.int64) + int(p["n_offset"])
    mem = members(p["noise_seed"], p["iteration"], Q, H, E, mutant)
    layers = [[(np.asarray(w, dtype), np.asarray(b, dtype)) for w, b in m] for m in p["members"]]
    unnorm = ocem.norm_flag(norm, "unnormalize_state")
    states = np.zeros((Q, H, N, s), dtype)
    costs = np.zeros((Q, N), dtype)
    pre = {}
    for q in range(Q):
        eps = ref.normals(p["noise_seed"], p["iteration"], q, n_idx, H, s).astype(dtype)
        st = np.broadcast_to(s0, (N, s)).copy()
        total = np.zeros(N, dtype)
        for t in range(H):
            x = ref._model_input(norm, st, actions[t], dtype)
            member = layers[mem[q, t]]
            for l, (w, b) in enumerate(member[:-1]):
                pre[(q, t, l)] = (x @ w.T + b).astype(dtype)
                x = np.maximum(pre[(q, t, l)], dtype(0))
            wh, bh = member[-1]
            m = (x @ wh[:s].T + bh[:s]).astype(dtype)
            raw = (x @ wh[s:].T + bh[s:]).astype(dtype)
            lv = ref.bounded_logvar(raw, lo, hi).astype(dtype)
            sd = (np.exp(dtype(0.5) * lv).astype(dtype) * scale).astype(dtype)
            z = (m + (sd * eps[t]).astype(dtype)).astype(dtype)
            st = ((z * norm["obs_std"]).astype(dtype) + norm["obs_mean"]).astype(dtype) if unnorm else z
            states[q, t] = st
            total = (total + ref._cost(st, actions[t], p["cost"], dtype)).astype(dtype)
        costs[q] = total
    return dict(states=states, costs=costs, members=mem, pre=pre)


# The RESAMPLED bar table: the issue's N x E x Q on the two (s, a), W, L pairs, H = 4. Every problem is a case of
# rollout_ts_reference's first table with its N, E and seed replaced, so the floor of the bar (that table's median
# e32) is the existing one.
BASES = {(17, 6): "n17_e2p3", (5, 12): "n40_e5p4_state"}
BAR_GRID = [(N, E, Q) for N in (1, 17, 40) for E in (2, 5) for Q in (1, 3, 7)]


def grid_base(N, E, Q):
    """The two shapes alternate over the grid, so that every N, E and Q meets both."""
    return list(BASES.values())[(BAR_GRID.index((N, E, Q))) % 2]


_GRID_REFS = {}


@functools.lru_cache(maxsize=None)
def grid_problem(N, E, Q):
    """The problem of one grid point (shared: do not write to it): the base case with its N and E, at most two hidden
    layers, drawn as rollout_ts_reference draws an envelope case -- seeds tried in a fixed order until no ReLU lies on
    different sides in the float32 and the float64 chain, so that e32 is rounding alone."""
    base = ref.CASES[grid_base(N, E, Q)]
    c = base._replace(N=N, E=E, P=1, L=min(base.L, 2), offset=tuple(e for e in base.offset if e < E))
    for k in range(ref.SEED_TRIES):
        p = ref._draw(c, 6100 + 100 * BAR_GRID.index((N, E, Q)) + k)
        r64, r32 = restate(p, Q, np.float64), restate(p, Q, np.float32)
        if ref.same_sides(r64, r32):
            _GRID_REFS[(N, E, Q)] = (r64, r32)
            return p
    raise AssertionError(f"{(N, E, Q)}: no seed in {ref.SEED_TRIES} keeps every ReLU on one side")


def grid_refs(N, E, Q):
    grid_problem(N, E, Q)
    return _GRID_REFS[(N, E, Q)]


@functools.lru_cache(maxsize=None)
def grid_bars(N, E, Q):
    """(bar, e32) per tensor: rollout_ts_reference.bars' rule with this problem's own float32 chain."""
    r64, r32 = grid_refs(N, E, Q)
    own = {k: ref.err(r32[k], r64[k]) for k in ref.KINDS}
    floor = {k: float(np.median([ref.e32(n)[k] for n in ref.NAMES])) for k in ref.KINDS}
    return {k: ref.BAR_FACTOR * max(own[k], floor[k]) for k in ref.KINDS}, own


def plan_given_costs(cost_hist, N, H, a, K, *, keep, seed, alpha, lo, hi, init_sigma, init_mu_rows=None,
                     init_sigma_rows=None, carry_in=None, b=0):
    """cem_rh_reference.plan with iteration i's costs cost_hist[i] ([Q][N], this problem's columns) given instead of
    rolled out. Per-iteration lists actions (the proposals), returns, elites, best, mu, sigma; kept ([I + 1] sets);
    the outputs mu_out, sigma_out, carry, carry_returns, final_actions."""
    Kc = int(keep)
    mu = np.zeros((H, a), F32) if init_mu_rows is None else np.clip(np.asarray(init_mu_rows, F32), F32(lo), F32(hi))
    sigma = np.full((H, a), F32(init_sigma), F32) if init_sigma_rows is None else np.asarray(init_sigma_rows, F32).copy()
    kept = None if carry_in is None else np.asarray(carry_in, F32).reshape(Kc, H, a)
    out = dict(actions=[], returns=[], elites=[], best=[], mu=[], sigma=[],
               kept=[np.zeros((Kc, H, a), F32) if kept is None else kept.copy()])
    for it, costs in enumerate(cost_hist):
        A = proposals(mu, sigma, lo, hi, seed, it, N, kept if Kc else None, None, b)
        ret = ocem.ensemble_returns(np.asarray(costs, F32))
        elites = ocem.select_elites(ret, K)
        best = ocem.select_elites(ret, Kc) if Kc else np.zeros(0, np.int64)
        mu, sigma = ocem.refit(mu, sigma, np.ascontiguousarray(A[:, elites, :].transpose(1, 0, 2)), alpha)
        kept = np.ascontiguousarray(A[:, best, :].transpose(1, 0, 2))
        for k, v in dict(actions=A, returns=ret, elites=elites, best=best, mu=mu, sigma=sigma).items():
            out[k].append(v)
        out["kept"].append(kept.copy())
    out.update(mu_out=mu, sigma_out=sigma, carry=kept, carry_returns=out["returns"][-1][out["best"][-1]],
               final_actions=np.clip(mu, F32(lo), F32(hi)).astype(F32))
    return out
