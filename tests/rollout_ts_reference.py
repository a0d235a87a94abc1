"""The trajectory-sampling rollout of include/mbrl_cem.h (mbrl_rollout_cost_ts), restated in NumPy at float64 (the
reference) and float32 (the same chain: it sets the bars), with the single-mistake mutants of the host test and
the case table the CPU and the GPU tests share. No GPU import.

The normals are oracle.philox's (bit-exact float32 at either dtype); the float32 chain goes through
oracle.cem.model_input and goal_state_cost themselves, the float64 chain through the same expressions at float64.
Row q = e * P + p is particle p of member e; states [Q][H][N][s], costs [Q][N]."""
import collections
import functools

import numpy as np

from oracle import cem as ocem
from oracle import philox

BAR_FACTOR = 8.0        # bar = BAR_FACTOR x max(e32 of the case's tensor, the table's median of it)
MUTANT_FACTOR = 10.0
KINDS = ("states", "costs")
MUTANTS = ("exp_lv", "raw_lv", "no_particle", "no_iteration", "t_n_swapped", "noise_after_unnorm", "noise_not_fed_back",
           "member_q_mod_E")

Case = collections.namedtuple("Case", "s a W L N H E P norm per_cand offset iteration n_offset noise state_cost "
                                      "action_cost")


def _c(s, a, W, L, N, H, E, P, norm="all", per_cand=False, offset=(), iteration=0, n_offset=0, noise=1.0,
       state_cost=True, action_cost=True):
    return Case(s, a, W, L, N, H, E, P, norm, per_cand, tuple(offset), iteration, n_offset, noise, state_cost,
                action_cost)


# norm: "all" (the three flags), "state" (normalize_state and unnormalize_state), "flags_off" (statistics given,
# no flag set), None (norm == NULL). offset: the members whose parameters sit 4 bytes off a 16-byte boundary.
CASES = {
    "n17_e2p3": _c(17, 6, 64, 2, 17, 4, 2, 3, iteration=3),
    "n40_e5p4_state": _c(5, 12, 33, 3, 40, 4, 5, 4, norm="state", offset=(1,), per_cand=True),
    "n16_h1_l1_off": _c(16, 1, 256, 1, 16, 1, 1, 1, norm="flags_off"),
    "n1_s33_null": _c(33, 2, 33, 2, 1, 4, 2, 3, norm=None, n_offset=5),
    "w1024": _c(17, 6, 1024, 2, 17, 1, 1, 1),
    "no_state_cost": _c(5, 12, 64, 2, 40, 4, 2, 3, state_cost=False, per_cand=True),
    "no_action_cost": _c(17, 6, 64, 1, 16, 4, 1, 1, action_cost=False, iteration=1, n_offset=16),
    "no_cost_half_noise": _c(16, 1, 33, 3, 17, 4, 2, 3, state_cost=False, action_cost=False, noise=0.5),
    "seam": _c(17, 6, 64, 2, 17, 4, 2, 3, norm=None, per_cand=True, noise=0.0),
    "seam_l3_e5": _c(5, 12, 33, 3, 40, 4, 5, 4, norm=None, per_cand=True, noise=0.0, offset=(2,)),
}
NAMES = list(CASES)
DIMENSIONS = dict(N=(1, 16, 17, 40), H=(1, 4), sa=((17, 6), (5, 12), (16, 1), (33, 2)), W=(33, 64, 256, 1024),
                  L=(1, 2, 3), EP=((1, 1), (2, 3), (5, 4)), norm=("all", "state", "flags_off", None))


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def bounded_logvar(raw, lo, hi):
    u = hi - softplus(hi - raw)
    return lo + softplus(u - lo)


def normals(seed, iteration, q, n_idx, H, s, swap_tn=False):
    """eps [H][len(n_idx)][s] of row q: element j & 3 of the two Box-Muller pairs of Philox4x32-10 at counter
    (n, t, q, (iteration << 8) | (j >> 2)), key = the halves of seed."""
    n_idx = np.asarray(n_idx, dtype=np.uint32)
    G = (s + 3) // 4
    T, Nn, Gg = np.meshgrid(np.arange(H, dtype=np.uint32), n_idx, np.arange(G, dtype=np.uint32), indexing="ij")
    word3 = (np.uint32(iteration) << np.uint32(8)) | Gg
    first, second = (T, Nn) if swap_tn else (Nn, T)
    ctr = np.stack([first, second, np.full_like(T, np.uint32(q)), word3], axis=-1)
    w = philox.philox4x32_10(ctr, philox.seed_key(seed))
    z0, z1 = philox.box_muller_f32(w[..., 0], w[..., 1])
    z2, z3 = philox.box_muller_f32(w[..., 2], w[..., 3])
    return np.ascontiguousarray(np.stack([z0, z1, z2, z3], axis=-1).reshape(H, len(n_idx), 4 * G)[..., :s])


def _norm_as(norm, dtype):
    if norm is None:
        return None
    return {k: (np.asarray(v, dtype) if isinstance(v, np.ndarray) else v) for k, v in norm.items()}


def _model_input(norm, st, ac, dtype):
    if dtype == np.float32:
        return ocem.model_input(norm, st, ac)
    if ocem.norm_flag(norm, "normalize_action"):
        ac = (ac - norm["act_mean"]) / norm["act_std"]
    if ocem.norm_flag(norm, "normalize_state"):
        st = (st - norm["obs_mean"]) / norm["obs_std"]
    return np.concatenate([st, ac], axis=1)


def _cost(st, ac, cost, dtype):
    if dtype == np.float32:
        return ocem.goal_state_cost(st, ac, cost)
    sc = ac_term = np.zeros(st.shape[:-1], dtype)
    if cost.get("has_state", True):
        al = np.float64(np.float32(cost["alpha_state"]))
        x = (st - cost["goal"].astype(dtype)) * cost["weights"].astype(dtype)
        sc = np.sum(np.sqrt(x * x + al * al) - al, axis=-1)
    if cost.get("has_action", True):
        aa = np.float64(np.float32(cost["alpha_action"]))
        ac_term = aa * aa * np.mean(np.cosh(ac / aa) - 1.0, axis=-1)
    return sc + ac_term


def restate(prob, dtype=np.float64, mutant=None, **override):
    """dict(states [Q][H][N][s], costs [Q][N], pre: per (q, t, l) the hidden pre-activations [N][W]) of the
    problem (problem(name), fields replaced by `override`) at `dtype`."""
    p = dict(prob, **override)
    c = p["case"]
    E, P, H, N, s = len(p["members"]), p["P"], p["actions"].shape[0], p["actions"].shape[1], c.s
    norm = _norm_as(p["norm"], dtype)
    lo, hi = (np.asarray(b, dtype) for b in p["bounds"])
    actions = np.asarray(p["actions"], dtype)
    s0 = np.asarray(p["s0"], dtype)
    scale = dtype(np.float32(p["noise_scale"]))
    n_idx = np.arange(N) + p["n_offset"]
    states = np.zeros((E * P, H, N, s), dtype)
    costs = np.zeros((E * P, N), dtype)
    pre = {}
    for q in range(E * P):
        e = q % E if mutant == "member_q_mod_E" else q // P
        layers = [(np.asarray(w, dtype), np.asarray(b, dtype)) for w, b in p["members"][e]]
        q_ctr = (q // P) * P if mutant == "no_particle" else q
        eps = normals(p["noise_seed"], 0 if mutant == "no_iteration" else p["iteration"], q_ctr, n_idx, H, s,
                      swap_tn=mutant == "t_n_swapped").astype(dtype)
        st = np.broadcast_to(s0, (N, s)).copy()
        total = np.zeros(N, dtype)
        for t in range(H):
            x = _model_input(norm, st, actions[t], dtype)
            for l, (w, b) in enumerate(layers[:-1]):
                z = (x @ w.T + b).astype(dtype)
                pre[(q, t, l)] = z
                x = np.maximum(z, dtype(0))
            # (the head's halves as two products: the mean's is then oracle.cem.mlp_forward's own expression on the
            # mean rows, so that BLAS blocks it the same way and the float32 chain equals the oracle's bit for bit)
            wh, bh = layers[-1]
            m = (x @ wh[:s].T + bh[:s]).astype(dtype)
            raw = (x @ wh[s:].T + bh[s:]).astype(dtype)
            lv = raw if mutant == "raw_lv" else bounded_logvar(raw, lo, hi).astype(dtype)
            sd = (np.exp(lv if mutant == "exp_lv" else dtype(0.5) * lv).astype(dtype) * scale).astype(dtype)
            noise = (sd * eps[t]).astype(dtype)
            unnorm = ocem.norm_flag(norm, "unnormalize_state")
            back = lambda v: ((v * norm["obs_std"]).astype(dtype) + norm["obs_mean"]).astype(dtype) if unnorm else v  # noqa: E731
            if mutant == "noise_after_unnorm":
                nxt = (back(m) + noise).astype(dtype)
            else:
                nxt = back((m + noise).astype(dtype))
            states[q, t] = nxt
            total = (total + _cost(nxt, actions[t], p["cost"], dtype)).astype(dtype)
            st = back(m) if mutant == "noise_not_fed_back" else nxt
        costs[q] = total
    return dict(states=states, costs=costs, pre=pre)


def applicable(name):
    """The mutants that change this case's result by construction."""
    c = CASES[name]
    noisy = c.noise > 0
    out = []
    for m in MUTANTS:
        ok = noisy
        if m == "no_particle":
            ok = noisy and c.P > 1
        elif m == "no_iteration":
            ok = noisy and c.iteration != 0
        elif m == "t_n_swapped":
            ok = noisy and (c.H > 1 or c.N > 1 or c.n_offset != 0)
        elif m == "noise_after_unnorm":
            ok = noisy and c.norm in ("all", "state")
        elif m == "noise_not_fed_back":
            ok = noisy and c.H > 1
        elif m == "member_q_mod_E":
            ok = c.E > 1 and c.P > 1        # (another member's mean: it shows without noise too)
        if ok:
            out.append(m)
    return out


def err(x, ref):
    """Tensor-relative: max |x - ref| / max |ref| (0 / 0 = 0)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    top = float(np.max(np.abs(ref)))
    d = float(np.max(np.abs(x - ref)))
    return d / top if top > 0 else (0.0 if d == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def problem(name):
    c = CASES[name]
    seed = 4200 + NAMES.index(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    dims = [c.s + c.a] + [c.W] * c.L + [2 * c.s]
    lo = (-6.0 + 0.25 * rng.random(c.s)).astype(np.float32)
    hi = (-1.0 + 0.25 * rng.random(c.s)).astype(np.float32)
    # the raw log-variances in three regimes, dimension by dimension: below min, between the bounds, above max
    regime = np.array([-9.0, -3.5, 2.0], np.float32)[np.arange(c.s) % 3]
    members = []
    for _ in range(c.E):
        layers = []
        for fi, fo in zip(dims[:-1], dims[1:]):
            bound = 1.0 / np.sqrt(fi)
            layers.append((rng.uniform(-bound, bound, (fo, fi)).astype(np.float32),
                           rng.uniform(-bound, bound, fo).astype(np.float32)))
        layers[-1][1][c.s:] += regime
        members.append(layers)
    norm = None
    if c.norm is not None:
        norm = ocem.synth_norm(seed, c.s, c.a)
        on = dict(all=(True, True, True), state=(True, True, False), flags_off=(False, False, False))[c.norm]
        norm.update(normalize_state=on[0], unnormalize_state=on[1], normalize_action=on[2])
    cost = dict(weights=ocem.synth_weights(seed, c.s), goal=rng.standard_normal(c.s).astype(np.float32),
                alpha_state=0.4, alpha_action=0.25, has_state=c.state_cost, has_action=c.action_cost)
    s0 = rng.standard_normal((c.N, c.s) if c.per_cand else c.s).astype(np.float32)
    actions = rng.uniform(-1, 1, (c.H, c.N, c.a)).astype(np.float32)
    return dict(case=c, members=members, bounds=(lo, hi), norm=norm, cost=cost, s0=s0, actions=actions, P=c.P,
                noise_seed=seed * 7919 + 11, iteration=c.iteration, n_offset=c.n_offset, noise_scale=c.noise)


@functools.lru_cache(maxsize=None)
def ref64(name):
    return restate(problem(name), np.float64)


@functools.lru_cache(maxsize=None)
def ref32(name):
    return restate(problem(name), np.float32)


@functools.lru_cache(maxsize=None)
def e32(name):
    r64, r32 = ref64(name), ref32(name)
    return {k: err(r32[k], r64[k]) for k in KINDS}


@functools.lru_cache(maxsize=None)
def bars(name):
    own = e32(name)
    return {k: BAR_FACTOR * max(own[k], float(np.median([e32(n)[k] for n in NAMES]))) for k in KINDS}


def errors(name, got):
    r64 = ref64(name)
    return {k: err(got[k], r64[k]) for k in KINDS}
