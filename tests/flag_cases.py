"""The model / cost parameter variants every kernel family is run under (tests/test_gpu_flags.py), as
plain data plus oracle-only helpers: no GPU import. tests/test_flag_cases.py checks on the oracle alone
that each (family, variant) pair can tell a wrong kernel from a right one (see there).

A variant names the keyword switches of oracle.cem.synth_problem:
  * "norm:<subset>"  the eight on/off subsets of normalize_state / unnormalize_state / normalize_action
                     (ns / us / na). A cleared flag's statistics pointer is NULL on the device whenever
                     no other flag needs it (fused.describe_norm): null_stats() says which.
  * "norm_null"      norm == NULL at the C entry (all flags 0); no Python spelling.
  * "weights_alphas" non-unit SmoothAbsLoss weights (one exact zero) with alpha_state 0.7, alpha_action 0.13
  * "no_state_cost" / "no_action_cost" / "no_cost"   has_state_cost / has_action_cost = 0 (C structs only)
  * "rew:<subset>"   reward-head models: unnormalize_reward (ur) x state normalisation (sn = ns and us)
  * "ns+weights"     a whole-plan variant: only normalize_state, with the weights_alphas cost
"""
import numpy as np

from oracle import cem as ocem
from oracle.philox import cem_actions

RTOL = 1e-5            # returns, by rel_err (test_gpu_parity.RTOL)
STATE_BAR = 1e-4       # states
MOVE_RETURNS = 1000 * RTOL      # what a wrong flag / weight / alpha must move the oracle's returns by
MOVE_STATES = 100 * STATE_BAR   # ... and, for a normaliser flag, the final states
RANGE_BAR = 2048.0     # the split kernels' operand range (|x| >= 2048 is redone in fp32)
WEIGHT_BAR = 128.0
TIE_GAP = 1e-5         # K-th to (K+1)-th return, relative: above it the elite bar cannot meet a tie

STATE_FLAGS = ("normalize_state", "unnormalize_state", "normalize_action")
ALPHA_STATE, ALPHA_ACTION = 0.7, 0.13


def _flags(ns, us, na, ur=False):
    return dict(normalize_state=bool(ns), unnormalize_state=bool(us), normalize_action=bool(na),
                unnormalize_reward=bool(ur))


NORM_SUBSETS = {"none": _flags(0, 0, 0), "na": _flags(0, 0, 1), "us": _flags(0, 1, 0), "ns": _flags(1, 0, 0),
                "ns+us": _flags(1, 1, 0), "ns+na": _flags(1, 0, 1), "us+na": _flags(0, 1, 1), "all": _flags(1, 1, 1)}
_WA = dict(random_weights=True, alpha_state=ALPHA_STATE, alpha_action=ALPHA_ACTION)

VARIANTS = {f"norm:{k}": dict(norm_flags=v) for k, v in NORM_SUBSETS.items()}
VARIANTS.update({
    "norm_null": dict(norm_flags=_flags(0, 0, 0)),          # problem() then drops the dict: norm is None
    "weights_alphas": dict(_WA),
    "no_state_cost": dict(has_state_cost=False),
    "no_action_cost": dict(has_action_cost=False),
    "no_cost": dict(has_state_cost=False, has_action_cost=False),
    "ns+weights": dict(_WA, norm_flags=_flags(1, 0, 0)),
    "rew:ur+sn": dict(norm_flags=_flags(1, 1, 1, 1)), "rew:ur": dict(norm_flags=_flags(0, 0, 1, 1)),
    "rew:sn": dict(norm_flags=_flags(1, 1, 1, 0)), "rew:none": dict(norm_flags=_flags(0, 0, 1, 0)),
})

EIGHT = [f"norm:{k}" for k in NORM_SUBSETS]
COST_VARIANTS = ["weights_alphas", "no_state_cost", "no_action_cost", "no_cost"]
FIVE = ["norm:na", "norm:us", "norm:ns", "weights_alphas", "no_state_cost"]
REWARD = ["rew:ur+sn", "rew:ur", "rew:sn", "rew:none"]
GD_VARIANTS = ["norm:na", "norm:us", "norm:ns", "weights_alphas"]

# family -> (config id, synth_problem shape overrides incl. N and H, variants). The kernel instance each
# rollout family runs (read from plan.hip rollout_impl / rollout.hip launch_rollout) is named in
# test_gpu_flags.py next to the option that selects it.
FAMILIES = {
    # ---- mbrl_rollout_cost with given actions
    "rollout_cid2": (2, dict(N=33, H=4), EIGHT + ["norm_null"] + COST_VARIANTS),
    "rollout_ring_ereg": (3, dict(N=300, H=3), FIVE),
    "rollout_ring_wide": (5, dict(N=40, H=2), FIVE),
    "rollout_nonring": (3, dict(N=40, H=2, s=40), FIVE),
    "rollout_r2": (4, dict(N=8200, H=2), FIVE),
    "rollout_tiles_cid2": (2, dict(N=9, H=5), EIGHT + ["weights_alphas", "no_state_cost"]),
    "rollout_tiles_cid3": (3, dict(N=300, H=3), EIGHT + ["weights_alphas", "no_state_cost"]),
    "rollout_pair": (4, dict(N=2048, H=2), FIVE),
    "rollout_split": (3, dict(N=300, H=3), FIVE),
    "rollout_reward": (6, dict(N=300, H=3), REWARD),
    # ---- mbrl_trajectory (one action sequence: N = 1)
    "traj_reg": (2, dict(N=1, H=6), EIGHT),
    "traj_coop": (3, dict(N=1, H=4), EIGHT + ["norm_null"]),
    "traj_plain": (3, dict(N=1, H=4, W=300, L=2), EIGHT),
    "traj_fallback": (3, dict(N=1, H=4), EIGHT),
    "traj_ensemble": (5, dict(N=1, H=2, E=2), ["norm:na"]),
    # ---- whole plans and DynamicsModel.forward
    "plan_cid3": (3, dict(N=257, H=4), ["norm:na"]),
    "plan_cid2": (2, dict(N=128, H=5), ["ns+weights"]),
    "forward": (4, dict(N=77, H=1), ["norm:us", "norm:none"]),
    # ---- mbrl_gd_plan (one action sequence)
    "gd_coop": (3, dict(N=1, H=6, W=256, L=3), GD_VARIANTS + ["no_state_cost", "no_action_cost"]),
    "gd_narrow": (3, dict(N=1, H=5, W=50, L=2), GD_VARIANTS),
    "gd_reward": (6, dict(N=1, H=5, W=64, L=2), REWARD),
}
# families whose GPU test compares states only (mbrl_trajectory and DynamicsModel.forward return no
# cost): their sensitivity condition is the one on the states
STATES_ONLY = ("traj_reg", "traj_coop", "traj_plain", "traj_fallback", "traj_ensemble", "forward")
PLAN_ITERATIONS = 2
PLAN_FAMILIES = ("plan_cid3", "plan_cid2")


def pairs(*families):
    """[(family, variant)] of the named families (all when none is named), for parametrize."""
    return [(f, v) for f in (families or FAMILIES) for v in FAMILIES[f][2]]


# synth_problem's draws are mild: start states ~ N(0, 1), statistics near the identity (mean within
# 0.5, std in [0.5, 2]) and nn.Linear-law weights whose outputs barely depend on their inputs, so over
# the few steps of these cases a wrong flag would move the returns by less than the bar that has to
# catch it. The table's problems therefore scale the start state and the means (the action means
# most: one action sequence has to show a wrong normalize_action), square the stds and
# apply a gain to every weight matrix (biases kept); test_flag_cases.py asserts the result is
# sensitive enough and still inside the split kernels' range.
S0_SCALE, MEAN_SCALE, ACT_MEAN_SCALE, STD_POWER, WEIGHT_GAIN = 3.0, 3.0, 12.0, 2.0, 1.5


def _sharpen(p):
    f32 = np.float32
    p["s0"] = (p["s0"] * f32(S0_SCALE)).astype(f32)
    n = p["norm"]
    for k in ("obs", "act", "rew"):
        if n.get(k + "_mean") is not None:
            n[k + "_mean"] = (n[k + "_mean"] * f32(ACT_MEAN_SCALE if k == "act" else MEAN_SCALE)).astype(f32)
            n[k + "_std"] = (n[k + "_std"] ** f32(STD_POWER)).astype(f32)
    p["model"] = [[((w * f32(WEIGHT_GAIN)).astype(f32), b) for w, b in layers] for layers in p["model"]]
    return p


def problem(family, variant):
    """The oracle problem of a (family, variant) pair. "norm_null": p["norm"] is None and the
    statistics stay under p["stats"] (for the mutants below)."""
    cid, over, variants = FAMILIES[family]
    assert variant in variants, (family, variant)
    p = _sharpen(ocem.synth_problem(cid, **VARIANTS[variant], **over))
    if variant == "norm_null":
        p["stats"], p["norm"] = p["norm"], None
    return p


def norm_keys(p):
    """The TransitionsDataset.normalizers() keywords the model closure binds for this problem."""
    return {k for k in ocem.NORM_FLAGS if ocem.norm_flag(p["norm"], k)}


def null_stats(p):
    """Which statistics pointers the device problem must hold as NULL: (obs, act)."""
    f = lambda k: ocem.norm_flag(p["norm"], k)  # noqa: E731
    return (not (f("normalize_state") or f("unnormalize_state")), not f("normalize_action"))


def actions(p, seed=11):
    """The given actions of a family: [H, N, a], the proposal law of the first CEM iteration."""
    cfg = p["cfg"]
    H, N, a = cfg["H"], cfg["N"], cfg["a"]
    return cem_actions(np.zeros((H, a), np.float32), np.full((H, a), 0.5, np.float32), -1, 1, seed, 0, np.arange(N))


def rel_err(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(x - ref) / np.maximum(np.abs(ref), 1.0)))


def evaluate(p, A):
    """(ensemble returns [N], states [E, H, N, s]) of the oracle."""
    costs, states = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A, store_states=True)
    return ocem.ensemble_returns(costs), states


def mutants(p):
    """[(label, problem, moves_states)]: the problems a kernel with ONE wrong branch would compute --
    each normaliser flag flipped; for a non-default cost, the weights replaced by ones, each alpha put
    back to its default, a dropped term put back."""
    out = []
    base = p["norm"] if p["norm"] is not None else p["stats"]
    c = p["cost"]
    reward = c.get("kind") == "reward"
    default_cost = reward or (np.all(c["weights"] == 1) and c["alpha_state"] == ocem.SMOOTH_ABS_ALPHA
                              and c["alpha_action"] == ocem.COSH_ALPHA and c.get("has_state", True)
                              and c.get("has_action", True))
    # The flags are flipped wherever the variant chose a subset of them. A pure cost variant runs with
    # every normaliser on, which the existing suite pins (and with the state term dropped no state
    # normaliser can move a return).
    subset = not all(ocem.norm_flag(p["norm"], k) for k in STATE_FLAGS)
    flags = STATE_FLAGS + (("unnormalize_reward",) if reward else ()) if default_cost or subset else ()
    for k in flags:
        n = dict(base)
        n[k] = not ocem.norm_flag(p["norm"], k)
        out.append((f"{k} flipped", dict(p, norm=n), k != "unnormalize_reward"))
    if reward:
        return out
    if not np.all(c["weights"] == 1):
        out.append(("unit weights", dict(p, cost=dict(c, weights=np.ones_like(c["weights"]))), False))
    if c["alpha_state"] != ocem.SMOOTH_ABS_ALPHA:
        out.append(("default alpha_state", dict(p, cost=dict(c, alpha_state=ocem.SMOOTH_ABS_ALPHA)), False))
    if c["alpha_action"] != ocem.COSH_ALPHA:
        out.append(("default alpha_action", dict(p, cost=dict(c, alpha_action=ocem.COSH_ALPHA)), False))
    for k in ("has_state", "has_action"):
        if not c.get(k, True):
            out.append((f"{k} put back", dict(p, cost=dict(c, **{k: True})), False))
    return out


# ---- the gradient-descent families: the GPU test compares the optimised actions and the last
# rollout's states with the reference's host loop, so their sensitivity condition is on those outputs
GD_FAMILIES = ("gd_coop", "gd_narrow", "gd_reward")
GD_ITERS = 8
GD_ACTION_TOL = dict(rtol=1e-4, atol=1e-5)     # test_gd_device_matches_reference's bars
GD_STATE_TOL = dict(rtol=1e-4, atol=1e-4)
MOVE_GD_ACTIONS = 1e-3    # |actions| <= 1, so the action bar is at most 1.1e-4: a mutant must move them 9 x that
# NOT visible in those outputs: unnormalize_reward. rew_std only scales the gradient and rew_mean has
# none, and an Adam step does not depend on the gradient's scale (up to its eps = 1e-8), so a GD kernel
# that ignored unnorm_r / rew_std would return the same actions and states. test_flag_cases.py asserts
# exactly that on the host loop; "rew:ur" / "rew:none" (and "rew:ur+sn" / "rew:sn") expect the same
# outputs. The GD kernels' rew_std factor is covered where the gradient itself is compared
# (tests/test_gpu_gd_grad.py, cases "flags_reward_*"), the rollout kernels' reward unnormalisation by
# family rollout_reward (it compares the returns).
GD_BLIND = ("unnormalize_reward flipped",)


def closures(p):
    """test_gpu_parity.build binding only the normalisers this problem's flags name (none for
    norm == NULL): (module, model_fn, cost_fn, sample_action). CPU torch; imported on use."""
    from test_gpu_parity import build
    q = p if p["norm"] is not None else dict(p, norm=p["stats"])
    return build(q, norm_keys=norm_keys(p))


def gd_host_loop(p, A):
    """The reference's gradient-descent loop (mbrl_amd.gd.plan_generic: plain torch autograd on the
    closures, on the CPU) from the action sequence A[:, 0]: (states [H + 1, s], actions [H, a]). A
    dropped cost term is a closure without it."""
    import torch
    from mbrl_amd import gd
    _, model_fn, cost_fn, _ = closures(p)
    c = p["cost"]
    if not c.get("has_state", True):
        action_cost = cost_fn.keywords["action_cost"]
        cost_fn = lambda s, a: action_cost(a)                  # noqa: E731
    elif not c.get("has_action", True):
        state_cost = cost_fn.keywords["state_cost"]
        cost_fn = lambda s, a: state_cost(s)                   # noqa: E731
    H = A.shape[0]
    init = ([], [torch.from_numpy(A[i, 0:1].copy()) for i in range(H)])
    states, actions = gd.plan_generic(torch.from_numpy(p["s0"]), model_fn, cost_fn, None, H, init, GD_ITERS, 0.0)
    return states.numpy(), actions.numpy()


def magnitudes(p, A):
    """(largest |state| or |layer input| over the rollout, every member, every layer incl. the reward
    pass; largest |weight| or |bias|): non-finite values come back as inf."""
    worst = 0.0

    def see(x):
        nonlocal worst
        worst = max(worst, float(np.max(np.abs(x))) if np.all(np.isfinite(x)) else np.inf)

    def layer_inputs(layers, x):
        see(x)
        for w, b in layers[:-1]:
            x = np.maximum(x @ w.T + b, np.float32(0))
            see(x)

    H, N, _ = A.shape
    for layers in p["model"]:
        st = np.broadcast_to(p["s0"], (N, p["s0"].shape[0])).astype(np.float32)
        for t in range(H):
            layer_inputs(layers, ocem.model_input(p["norm"], st, A[t]))
            st = ocem.dynamics_step(layers, p["norm"], st, A[t])
            see(st)
            if p["cost"].get("kind") == "reward":
                layer_inputs(layers, ocem.model_input(p["norm"], st, A[t]))
    wmax = max(float(np.max(np.abs(x))) for layers in p["model"] for wb in layers for x in wb)
    return worst, wmax


def plan_gaps(p, iterations=PLAN_ITERATIONS):
    """(the oracle's plan, per iteration the relative gap between the K-th and (K+1)-th return)."""
    cfg = p["cfg"]
    ref = ocem.cem_plan(p, N=cfg["N"], H=cfg["H"], num_iterations=iterations)
    K = max(1, int(cfg["N"] * ocem.CEM_DEFAULTS["elite_frac"]))
    gaps = []
    for r in ref["returns"]:
        srt = np.sort(r.astype(np.float64))
        gaps.append(float((srt[K] - srt[K - 1]) / max(abs(srt[K - 1]), 1.0)))
    return ref, gaps
