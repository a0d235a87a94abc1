"""The case table of the rollout shape-envelope tests (test_rollout_dispatch_model.py on the CPU,
test_gpu_envelope.py on the GPU): model shapes and candidate counts chosen so that every fp32 rollout
instance launch_rollout can pick is reached, with each LDS-driven fallback and each refusal beside it.

A Case names a synthetic problem (oracle.cem.synth_problem(cid, **over)), N and H; `built_for` says which
fields of the dispatch model's outcome the case was written to reach (the model computes the outcome; a
test checks the two agree, so a case that drifts off its branch fails on the CPU). `mode` is how the GPU
test feeds it: "given" actions, "per_cand" (s0_per_candidate), "sampled" (an in-call draw at n_offset > 0).

HUMANOID / GENERIC / WIDE_* are the state and action dims the cases share: humanoid's 67 / 21 gives the ring
shape K0C = NOT = 6; 30 / 8 gives K0C = 4, which no ring instance has (the generic K0C_T = 0 kernel); the wide
inputs have 16 K0C > Wpad, so the LDS row stride comes from the input and not from W.

rollout_f64() is the float64 evaluation of the oracle's rollout that sizes H (test_rollout_dispatch_model.py,
the tolerance argument in test_gpu_envelope.py's docstring)."""
import collections

import numpy as np

import rollout_dispatch_model as rdm

HUMANOID = dict(s=67, a=21)
GENERIC = dict(s=30, a=8)
WIDE_90 = dict(s=90, a=30, W=16, L=2)
WIDE_200 = dict(s=200, a=40, W=8, L=1)
ORACLE_ROWS = 64          # candidates compared with the oracle where N is large

Case = collections.namedtuple("Case", "id cid over N H mode built_for")
Refused = collections.namedtuple("Refused", "id cid over N H fragment")


def _c(id, cid, over, N, H, mode="given", **built_for):
    return Case(id, cid, over, N, H, mode, built_for)


ACCEPTED = (
    # ---- T = 16 (512 < W <= 1024): ring 2/2 at every depth, unpadded widths, generic, ring 6/6, reward head
    _c("t16_ring22_L1", 3, dict(W=1024, L=1), 40, 3, T=16, R=1, NW=8, K0C_T=2, NOT_T=2, part_alias=False),
    _c("t16_ring22_L2", 3, dict(W=1024, L=2), 40, 3, T=16, K0C_T=2, part_alias=False, lds_bytes=160640),
    _c("t16_ring22_L3", 3, dict(W=1024, L=3), 33, 2, T=16, K0C_T=2, part_alias=True),
    _c("t16_W513", 3, dict(W=513, L=2), 17, 2, T=16, K0C_T=2),
    _c("t16_W1000", 3, dict(W=1000, L=3), 40, 2, "sampled", T=16, K0C_T=2, part_alias=True),
    _c("t16_generic_L2", 3, dict(W=1024, L=2, **GENERIC), 40, 2, T=16, K0C_T=0, part_alias=False, lds_bytes=161920),
    _c("t16_generic_L3", 3, dict(W=1024, L=3, **GENERIC), 21, 2, "per_cand", T=16, K0C_T=0, part_alias=True),
    _c("t16_humanoid_L3_E2", 5, dict(W=1024, L=3, E=2), 40, 2, T=16, K0C_T=6, NOT_T=6, part_alias=True),
    _c("t16_reward", 6, dict(W=1024), 40, 2, T=16, K0C_T=2, reward=1),
    _c("t16_reward_generic", 6, dict(W=600, L=1, **GENERIC), 19, 2, T=16, K0C_T=0, reward=1),
    # ---- 16-candidate tiles (R = 1) of the narrower instances, ring and generic
    _c("r1_t1_ring", 2, dict(W=50), 40, 3, T=1, R=1, NW=4, K0C_T=2),
    _c("r1_t2_ring", 3, dict(W=128, L=2), 40, 2, T=2, R=1, NW=8, K0C_T=2),
    _c("r1_t2_generic", 3, dict(W=100, L=3, **GENERIC), 40, 2, T=2, R=1, K0C_T=0),
    _c("r1_t4_ring", 2, dict(), 40, 3, T=4, R=1, K0C_T=2, kernel="m16"),
    _c("r1_t4_generic", 3, dict(W=200, L=2, **GENERIC), 40, 2, T=4, R=1, K0C_T=0),
    _c("r1_t8_ring", 3, dict(L=2), 40, 2, T=8, R=1, K0C_T=2, GS=True, kernel="m16"),
    _c("r1_t8_generic", 3, dict(L=3, **GENERIC), 40, 2, T=8, R=1, K0C_T=0, part_alias=True),
    _c("r1_t8_reward", 6, dict(), 40, 2, T=8, R=1, K0C_T=2, reward=1),
    # ---- 32-candidate tiles (R = 2, N >= 8192)
    _c("r2_t1_ring", 2, dict(W=50), 8192, 2, T=1, R=2, NW=4, K0C_T=2),
    _c("r2_t1_generic", 3, dict(W=64, L=2, **GENERIC), 8200, 2, T=1, R=2, NW=4, K0C_T=0),
    _c("r2_t2_ring", 3, dict(W=128, L=2), 8192, 2, T=2, R=2, NW=4, K0C_T=2),
    _c("r2_t2_generic_L3", 3, dict(W=128, L=3, **GENERIC), 8192, 2, T=2, R=2, NW=4, K0C_T=0, part_alias=False),
    _c("r2_t4_cartpole_ring", 2, dict(), 8192, 2, T=4, R=2, NW=4, K0C_T=2),
    _c("r2_t4_generic", 3, dict(W=256, L=2, **GENERIC), 8200, 2, T=4, R=2, NW=4, K0C_T=0),
    _c("r2_t8_ring", 4, dict(), 8192, 2, T=8, R=2, NW=8, K0C_T=2, part_alias=True),
    _c("r2_t8_generic_L2", 3, dict(L=2, **GENERIC), 8192, 2, T=8, R=2, NW=4, K0C_T=0, part_alias=False,
       lds_bytes=161280),
    _c("r2_t8_generic_L3", 3, dict(L=3, **GENERIC), 8200, 2, T=8, R=2, NW=8, K0C_T=0, part_alias=True),
    _c("r2_t8_humanoid_L3", 5, dict(E=1), 8192, 1, T=8, R=2, NW=4, K0C_T=6, part_alias=True),
    _c("r2_reward_W512", 6, dict(), 8192, 2, T=8, R=2, NW=4, K0C_T=2, reward=1, lds_bytes=158912),
    _c("r2_reward_W128", 6, dict(W=128), 8200, 2, T=2, R=2, NW=4, K0C_T=2, reward=1),
    _c("r2_a24", 3, dict(a=24, L=3), 8192, 1, T=8, R=2, fallback=None),
    # ---- N >= 8192 that falls back to 16-candidate tiles
    _c("fb_humanoid_L2", 5, dict(L=2, E=1), 8192, 1, T=8, R=1, NW=8, K0C_T=6, fallback="lds"),
    _c("fb_humanoid_L4", 5, dict(L=4, E=1), 8192, 1, T=8, R=1, NW=8, K0C_T=6, fallback="lds"),
    _c("fb_a25", 3, dict(a=25, L=3), 8192, 1, T=8, R=1, fallback="actions"),
    _c("a48_N8192", 3, dict(a=48, L=3), 8192, 1, T=8, R=1, K0C_T=6, NOT_T=2, fallback="actions"),
    _c("a48_N40", 3, dict(a=48, L=3), 40, 2, T=8, R=1, K0C_T=6, NOT_T=2, kernel="m16"),
    # ---- input wider than the hidden layer
    _c("wide_s90", 3, WIDE_90, 40, 3, "per_cand", T=1, R=1, NW=4, K0C_T=0),
    _c("wide_s200", 3, WIDE_200, 40, 2, T=1, R=1, NW=4, K0C_T=0, lds_bytes=114304),
)

REFUSED = (
    Refused("no_a49", 3, dict(a=49, W=64, L=2), 40, 2, "action_dim 49 too large (max 48)"),
    Refused("no_W1025", 3, dict(W=1025), 40, 2, "unsupported MLP shape"),
    Refused("no_L5", 3, dict(W=64, L=5), 40, 2, "unsupported MLP shape"),
    Refused("no_W1024_L4", 3, dict(W=1024, L=4), 40, 2, "LDS footprint 168832 B exceeds 160 KiB"),
    Refused("no_humanoid_W1024_L2", 5, dict(W=1024, L=2, E=1), 40, 2, "LDS footprint 199680 B exceeds 160 KiB"),
    Refused("no_s500", 3, dict(s=500, a=12, W=64, L=2), 40, 2, "LDS footprint 242400 B exceeds 160 KiB"),
)

# Pairs on opposite sides of the 160 KiB line: (accepted id, refused id, what differs)
LINE = (
    ("t16_ring22_L2", "no_W1024_L4", "two more hidden layers' biases"),
    ("t16_ring22_L3", "no_W1024_L4", "L = 3 aliases the partials, L = 4 cannot"),
    ("t16_humanoid_L3_E2", "no_humanoid_W1024_L2", "L = 3 aliases the partials, L = 2 cannot"),
)


def by_id(cid):
    for c in ACCEPTED + REFUSED:
        if c.id == cid:
            return c
    raise KeyError(cid)


def shape_of(case):
    """(s, a, W, L, E, reward) of a case: the config's values under the case's overrides."""
    from oracle import cem as ocem
    cfg = dict(ocem.CONFIGS[case.cid])
    cfg.update(case.over)
    return cfg["s"], cfg["a"], cfg["W"], cfg["L"], cfg["E"], int(bool(cfg.get("reward")))


def outcome(case, **kw):
    """The dispatch model's outcome for a case as mbrl_rollout_cost runs it at auto settings."""
    return rdm.dispatch(*shape_of(case), N=case.N, **kw)


def forced_tile(case):
    """The MBRL_OPT_ROLLOUT_TILE value the GPU test sets: 16 where the 8-candidate branch would otherwise
    take the case (its instances have their own tests, test_gpu_m8.py), else 0."""
    return 16 if getattr(outcome(case), "kernel", None) == "m8" else 0


def run_outcome(case):
    """The outcome as the GPU test runs the case (forced_tile applied)."""
    return outcome(case, rollout_tile=forced_tile(case))


# ------------------------------------------------------------------------------------------------
def rollout_f64(problem, s0, actions, store_states=False):
    """oracle.cem.rollout's arithmetic (the problem's normaliser flags, both cost terms, unit or given weights,
    or the reward head) in float64 from the same float32 inputs: costs [E, N], and with store_states the
    states [E, H, N, s] as well."""
    from oracle import cem as ocem
    nm, cost = problem["norm"], problem["cost"]
    f = lambda x: np.asarray(x, dtype=np.float64)
    on = lambda k: ocem.norm_flag(nm, k)  # noqa: E731
    H, N, _ = actions.shape
    out, states = [], []
    for layers in problem["model"]:
        def mlp(x):
            for w, b in layers[:-1]:
                x = np.maximum(x @ f(w).T + f(b), 0.0)
            return x @ f(layers[-1][0]).T + f(layers[-1][1])

        def inp(st, t):
            an = (f(actions[t]) - f(nm["act_mean"])) / f(nm["act_std"]) if on("normalize_action") else f(actions[t])
            sn = (st - f(nm["obs_mean"])) / f(nm["obs_std"]) if on("normalize_state") else st
            return np.concatenate([sn, an], axis=1)
        st = np.broadcast_to(f(s0), (N, f(s0).shape[-1])).copy()
        ns = st.shape[1]
        total = np.zeros(N)
        member = []
        for t in range(H):
            st = mlp(inp(st, t))[:, :ns]
            if on("unnormalize_state"):
                st = st * f(nm["obs_std"]) + f(nm["obs_mean"])
            member.append(st)
            if cost.get("kind") == "reward":
                r = mlp(inp(st, t))[:, ns]
                total += r * f(nm["rew_std"])[0] + f(nm["rew_mean"])[0] if on("unnormalize_reward") else r
            else:
                x = (st - f(cost["goal"])) * f(cost["weights"])
                sc = np.sum(np.sqrt(x * x + cost["alpha_state"] ** 2) - cost["alpha_state"], axis=-1)
                aa = cost["alpha_action"]
                total += sc + aa * aa * np.mean(np.cosh(f(actions[t]) / aa) - 1.0, axis=-1)
        out.append(total)
        states.append(np.stack(member))
    return (np.stack(out), np.stack(states)) if store_states else np.stack(out)


def given_inputs(case, problem):
    """(s0 [s] or [N, s], actions [H, N, a]) of a "given" / "per_cand" case: the suite's usual draw."""
    from oracle.philox import cem_actions
    a = problem["cfg"]["a"]
    H, N = case.H, case.N
    A = cem_actions(np.zeros((H, a), np.float32), np.full((H, a), 0.5, np.float32), -1, 1, 11, 0, np.arange(N))
    s0 = problem["s0"]
    if case.mode == "per_cand":
        rng = np.random.default_rng(len(case.id))
        s0 = (s0[None, :] + 0.25 * rng.standard_normal((N, s0.size))).astype(np.float32)
    return s0, A
