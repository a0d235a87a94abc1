"""The trajectory-sampling rollout of include/mbrl_cem.h (mbrl_rollout_cost_ts), restated in NumPy at float64 (the
reference) and float32 (the same chain: it sets the bars), with the single-mistake mutants of the host test and
the two case tables the CPU and the GPU tests share: CASES (the ten cases whose e32 median sets the floor of every
bar) and ENVELOPE (the ends of what the entry accepts; judged against the same floor, never part of it). No GPU
import.

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
KEY_MUTANTS = ("seed_high_dropped", "no_n_offset", "group_is_dimension", "pairs_swapped", "iteration_unshifted")
MUTANTS = ("exp_lv", "raw_lv", "no_particle", "no_iteration", "t_n_swapped", "noise_after_unnorm", "noise_not_fed_back",
           "member_q_mod_E") + KEY_MUTANTS
SEED64 = (0x9E3779B9 << 32) | 0x7F4A7C15     # both key words set
SEED_TRIES = 50

Case = collections.namedtuple("Case", "s a W L N H E P norm per_cand offset iteration n_offset noise state_cost "
                                      "action_cost seed cost_null lv zero_w")


def _c(s, a, W, L, N, H, E, P, norm="all", per_cand=False, offset=(), iteration=0, n_offset=0, noise=1.0,
       state_cost=True, action_cost=True, seed=None, cost_null=False, lv="regimes", zero_w=False):
    return Case(s, a, W, L, N, H, E, P, norm, per_cand, tuple(offset), iteration, n_offset, noise, state_cost,
                action_cost, seed, cost_null, lv, zero_w)


# seed: noise_seed (None: the problem seed * 7919 + 11, below 2^32). cost_null: cost == NULL. lv: "regimes" (below),
# "pm1e4" (+-1e4 on top, dimensions alternating: both softplus calls saturate), "equal" (min_logvar == max_logvar).
# zero_w: every weight 0, so the head's biases are the mean and the raw log-variance of every step.
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

# The ends of the entry's envelope. L + 1 odd: the LDS buffers swap roles from step to step; even: they do not.
ENVELOPE = {
    # W on both sides of one 16-wide tile
    "w1": _c(5, 2, 1, 2, 17, 4, 2, 2), "w15": _c(5, 2, 15, 2, 17, 4, 2, 2),
    "w16": _c(5, 2, 16, 2, 17, 4, 2, 2), "w17": _c(5, 2, 17, 2, 17, 4, 2, 2),
    # s + a at the edges of layer 0's 16-deep chunks, H = 4: the seam rewrites them
    "sa15_1": _c(15, 1, 33, 1, 17, 4, 2, 2), "sa16_1": _c(16, 1, 17, 2, 17, 4, 2, 2, norm="state"),
    "sa1_15": _c(1, 15, 33, 1, 17, 4, 2, 2), "sa3_29": _c(3, 29, 16, 2, 17, 4, 2, 2),
    "sa4_29": _c(4, 29, 33, 1, 17, 4, 2, 2, per_cand=True),
    # an action tail of several chunks, and s + a = 1024: the entry's limit
    "a48": _c(1, 48, 33, 2, 17, 4, 2, 2), "a1023": _c(1, 1023, 16, 1, 2, 2, 1, 2),
    # one partly filled noise group, and a head of exactly one and of two blocks of output neurons
    "s1": _c(1, 1, 17, 2, 17, 4, 2, 2), "s2": _c(2, 1, 33, 1, 17, 4, 2, 2), "s3": _c(3, 1, 17, 2, 17, 4, 2, 2, norm=None),
    "s4": _c(4, 1, 33, 1, 17, 4, 2, 2), "s8": _c(8, 1, 17, 2, 17, 4, 2, 2, norm="flags_off"),
    "s9": _c(9, 1, 33, 1, 17, 4, 2, 2),
    # 2 s wider than W rounded up and than the padded layer-0 input: raw log-variances survive beyond the seam
    "s40_w16": _c(40, 2, 16, 2, 17, 4, 2, 2), "s24_w33": _c(24, 1, 33, 1, 17, 4, 2, 2),
    "l8": _c(5, 2, 33, 8, 17, 4, 2, 2),
    # MBRL_TRAIN_MAX_MEMBERS members, MBRL_TS_MAX_ROWS rows
    "e8p32": _c(5, 2, 16, 1, 17, 2, 8, 32, offset=(3,), seed=SEED64), "e1p256": _c(5, 2, 16, 2, 17, 2, 1, 256),
    # the largest head two LDS buffers hold: 2 x 16 x (1264 + 4) x 4 bytes <= 160 KiB
    "s632_n1": _c(632, 1, 16, 1, 1, 2, 1, 2), "s632_n17": _c(632, 1, 16, 1, 17, 2, 1, 2),
    "shared_s0": _c(17, 6, 33, 2, 40, 4, 2, 2),
    # the key and counter words at their ends
    "key_seed": _c(5, 2, 33, 2, 17, 4, 2, 2, seed=SEED64),
    "key_iteration": _c(9, 2, 33, 1, 17, 4, 2, 2, iteration=(1 << 24) - 1),
    "key_n_offset": _c(5, 2, 33, 2, 17, 4, 2, 2, n_offset=(1 << 31) - 9),
    # the log-variance head at its ends
    "lv_pm1e4": _c(5, 2, 33, 2, 17, 4, 2, 2, lv="pm1e4"), "lv_equal": _c(5, 2, 33, 1, 17, 4, 2, 2, lv="equal"),
    "noise_1e-30": _c(5, 2, 33, 2, 17, 4, 2, 2, noise=1e-30), "noise_1e3": _c(5, 2, 33, 1, 17, 4, 2, 2, noise=1e3),
    "cost_null": _c(5, 2, 33, 2, 17, 4, 2, 2, cost_null=True),
    # zero weights: the states are m + sd * eps, the noise itself (the moment test reads them)
    "moments": _c(8, 1, 16, 1, 4096, 2, 1, 4, norm=None, zero_w=True, seed=SEED64, iteration=5, n_offset=3, noise=0.75),
}
ENV_NAMES = list(ENVELOPE)
ALL = dict(CASES, **ENVELOPE)
ALL_NAMES = NAMES + ENV_NAMES


def case(name):
    return ALL[name]


def _any(pred):
    return lambda cs: any(pred(c) for c in cs)


def _each(values, key):
    return lambda cs: {key(c) for c in cs} >= set(values)


# One entry per row of the envelope: what the table must hold for the row to be there.
ENVELOPE_ROWS = {
    "W on both sides of one tile": _each([1, 15, 16, 17], lambda c: c.W if (c.s, c.a, c.L, c.H) == (5, 2, 2, 4) else None),
    "s + a at chunk edges, H = 4": _each([(15, 1), (16, 1), (1, 15), (3, 29), (4, 29)],
                                         lambda c: (c.s, c.a) if c.H == 4 else None),
    "a long action tail": lambda cs: any((c.s, c.a) == (1, 48) for c in cs) and any(
        (c.s, c.a, c.W, c.L, c.N, c.H) == (1, 1023, 16, 1, 2, 2) for c in cs),
    "small and block-edge s": lambda cs: {c.s for c in cs if c.a == 1 and c.H == 4} >= {1, 2, 3, 4, 8, 9} and any(
        c.a == 1 and c.s in (1, 2, 3, 4, 8, 9) and c.norm in (None, "flags_off") for c in cs),
    "2s > W and 2s > padded s + a": _each([(40, 2, 16), (24, 1, 33)], lambda c: (c.s, c.a, c.W)),
    "deepest trunk": _any(lambda c: (c.L, c.W, c.E, c.P) == (8, 33, 2, 2)),
    "most members and rows": lambda cs: {(c.E, c.P) for c in cs if (c.N, c.H, c.W) == (17, 2, 16)} >= {(8, 32), (1, 256)}
    and any(c.E * c.P == 256 and c.offset for c in cs),
    "largest head": _each([1, 17], lambda c: c.N if (c.s, c.a, c.W, c.L, c.H) == (632, 1, 16, 1, 2) else None),
    "shared s0 across several tiles": _any(lambda c: c.N == 40 and not c.per_cand),
    "key words at their ends": lambda cs: any(c.seed == SEED64 and not c.zero_w and c.E * c.P < 256 for c in cs) and any(
        c.iteration == (1 << 24) - 1 and c.s >= 5 for c in cs) and any(
        c.n_offset == (1 << 31) - 9 and c.N == 17 for c in cs),
    "log-variance head at its ends": lambda cs: {c.lv for c in cs} >= {"pm1e4", "equal"} and
    {c.noise for c in cs} >= {1e-30, 1e3},
    "cost == NULL": _any(lambda c: c.cost_null),
    "the noise itself": _any(lambda c: c.zero_w and (c.W, c.N, c.H, c.E, c.P) == (16, 4096, 2, 1, 4)),
    "both parities of L + 1": lambda cs: {(c.L + 1) % 2 for c in cs if c.H == 4} == {0, 1},
    "small": lambda cs: all((c.N <= 40 and c.H <= 4) or c.zero_w for c in cs),
}
DIMENSIONS = dict(N=(1, 16, 17, 40), H=(1, 4), sa=((17, 6), (5, 12), (16, 1), (33, 2)), W=(33, 64, 256, 1024),
                  L=(1, 2, 3), EP=((1, 1), (2, 3), (5, 4)), norm=("all", "state", "flags_off", None))


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def bounded_logvar(raw, lo, hi):
    u = hi - softplus(hi - raw)
    return lo + softplus(u - lo)


def normals(seed, iteration, q, n_idx, H, s, swap_tn=False, mutant=None):
    """eps [H][len(n_idx)][s] of row q: element j & 3 of the two Box-Muller pairs of Philox4x32-10 at counter
    (n mod 2^32, t, q, (iteration << 8) | (j >> 2)), key = the halves of seed. n_idx: n + n_offset as integers of
    any width."""
    n_idx = (np.asarray(n_idx, dtype=np.int64) % (1 << 32)).astype(np.uint32)
    G = s if mutant == "group_is_dimension" else (s + 3) // 4
    T, Nn, Gg = np.meshgrid(np.arange(H, dtype=np.uint32), n_idx, np.arange(G, dtype=np.uint32), indexing="ij")
    word3 = (np.uint32(iteration) << np.uint32(0 if mutant == "iteration_unshifted" else 8)) | Gg
    first, second = (T, Nn) if swap_tn else (Nn, T)
    ctr = np.stack([first, second, np.full_like(T, np.uint32(q)), word3], axis=-1)
    w = philox.philox4x32_10(ctr, philox.seed_key(seed & 0xFFFFFFFF if mutant == "seed_high_dropped" else seed))
    z0, z1 = philox.box_muller_f32(w[..., 0], w[..., 1])
    z2, z3 = philox.box_muller_f32(w[..., 2], w[..., 3])
    z = np.stack([z2, z3, z0, z1] if mutant == "pairs_swapped" else [z0, z1, z2, z3], axis=-1)
    if mutant == "group_is_dimension":       # one Philox call per dimension j, element j & 3 of it
        return np.ascontiguousarray(z[:, :, np.arange(s), np.arange(s) & 3])
    return np.ascontiguousarray(z.reshape(H, len(n_idx), 4 * G)[..., :s])


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
    n_idx = np.arange(N, dtype=np.int64) + (0 if mutant == "no_n_offset" else int(p["n_offset"]))
    states = np.zeros((E * P, H, N, s), dtype)
    costs = np.zeros((E * P, N), dtype)
    pre = {}
    for q in range(E * P):
        e = q % E if mutant == "member_q_mod_E" else q // P
        layers = [(np.asarray(w, dtype), np.asarray(b, dtype)) for w, b in p["members"][e]]
        q_ctr = (q // P) * P if mutant == "no_particle" else q
        eps = normals(p["noise_seed"], 0 if mutant == "no_iteration" else p["iteration"], q_ctr, n_idx, H, s,
                      swap_tn=mutant == "t_n_swapped", mutant=mutant if mutant in KEY_MUTANTS else None).astype(dtype)
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
    """The mutants that change this case's result by construction. An envelope case is held to the key and counter
    mutants only (the older ones are judged on the first table), and only where its noise is of the states' size."""
    c = ALL[name]
    noisy = c.noise > 0 if name in CASES else c.noise >= 0.5
    out = []
    for m in MUTANTS if name in CASES else KEY_MUTANTS:
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
        elif m == "seed_high_dropped":
            ok = noisy and c.seed is not None and c.seed >= 1 << 32
        elif m == "no_n_offset":
            ok = noisy and c.n_offset != 0
        elif m == "group_is_dimension":
            ok = noisy and c.s >= 2         # (dimension 0 is element 0 of group 0 either way)
        elif m == "iteration_unshifted":
            ok = noisy and c.iteration != 0
        if ok:
            out.append(m)
    return out


def err(x, ref):
    """Tensor-relative: max |x - ref| / max |ref| (0 / 0 = 0)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    top = float(np.max(np.abs(ref)))
    d = float(np.max(np.abs(x - ref)))
    return d / top if top > 0 else (0.0 if d == 0 else float("inf"))


def _draw(c, seed):
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
        if c.lv == "pm1e4":
            layers[-1][1][c.s:] += np.float32(1e4) * (1 - 2 * (np.arange(c.s) % 2)).astype(np.float32)
        if c.zero_w:
            for w, _b in layers:
                w[...] = 0
        members.append(layers)
    if c.lv == "equal":
        hi = lo.copy()
    norm = None
    if c.norm is not None:
        norm = ocem.synth_norm(seed, c.s, c.a)
        on = dict(all=(True, True, True), state=(True, True, False), flags_off=(False, False, False))[c.norm]
        norm.update(normalize_state=on[0], unnormalize_state=on[1], normalize_action=on[2])
    cost = dict(weights=ocem.synth_weights(seed, c.s), goal=rng.standard_normal(c.s).astype(np.float32),
                alpha_state=0.4, alpha_action=0.25, has_state=c.state_cost and not c.cost_null,
                has_action=c.action_cost and not c.cost_null)
    s0 = rng.standard_normal((c.N, c.s) if c.per_cand else c.s).astype(np.float32)
    actions = rng.uniform(-1, 1, (c.H, c.N, c.a)).astype(np.float32)
    return dict(case=c, members=members, bounds=(lo, hi), norm=norm, cost=cost, cost_null=c.cost_null, s0=s0,
                actions=actions, P=c.P, noise_seed=seed * 7919 + 11 if c.seed is None else c.seed, iteration=c.iteration,
                n_offset=c.n_offset, noise_scale=c.noise)


def same_sides(r64, r32):
    """Whether every hidden pre-activation lies on one side of its ReLU in float32 and in float64."""
    return r64["pre"].keys() == r32["pre"].keys() and bool(r64["pre"]) and all(
        np.array_equal(r64["pre"][k] > 0, r32["pre"][k] > 0) for k in r64["pre"])


_REFS = {}


@functools.lru_cache(maxsize=None)
def problem(name):
    """The case's problem (shared: do not write to it). A case of the first table is drawn from its one seed. For an
    envelope case seeds are tried in a fixed order, SEED_TRIES at the most, until no ReLU lies on different sides in
    the float32 and the float64 chain, so that e32 is rounding alone."""
    if name in CASES:
        return _draw(CASES[name], 4200 + NAMES.index(name))
    for k in range(SEED_TRIES):
        p = _draw(ENVELOPE[name], 5200 + 100 * ENV_NAMES.index(name) + k)
        r64, r32 = restate(p, np.float64), restate(p, np.float32)
        if same_sides(r64, r32):
            _REFS[name] = (r64, r32)
            return dict(p, seed_tries=k + 1)
    raise AssertionError(f"{name}: no seed in {SEED_TRIES} keeps every ReLU on one side in float32 and float64")


@functools.lru_cache(maxsize=None)
def ref64(name):
    p = problem(name)
    return _REFS[name][0] if name in _REFS else restate(p, np.float64)


@functools.lru_cache(maxsize=None)
def ref32(name):
    p = problem(name)
    return _REFS[name][1] if name in _REFS else restate(p, np.float32)


@functools.lru_cache(maxsize=None)
def e32(name):
    r64, r32 = ref64(name), ref32(name)
    return {k: err(r32[k], r64[k]) for k in KINDS}


@functools.lru_cache(maxsize=None)
def bars(name):
    """(an envelope case against its own e32 and the first table's median: the ten bars never move)"""
    own = e32(name)
    return {k: BAR_FACTOR * max(own[k], float(np.median([e32(n)[k] for n in NAMES]))) for k in KINDS}


def errors(name, got):
    r64 = ref64(name)
    return {k: err(got[k], r64[k]) for k in KINDS}
