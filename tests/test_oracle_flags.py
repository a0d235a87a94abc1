"""The oracle's per-flag normalisation and cost switches (oracle/cem.py norm_flag, has_state /
has_action, arbitrary weights and alphas) against the project's own torch classes in float64 on the
CPU: Model / ModelWithReward .forward with the chosen subset of TransitionsDataset.normalizers(), and
SmoothAbsLoss / CoshLoss with the same weights and alphas. This pins the branches that
tests/golden/ does not reach (its fixtures run every normaliser, unit weights, default alphas), so the
oracle can be the reference of tests/test_gpu_flags.py. Bars: returns 1e-5 by rel_err, states 1e-4."""
import functools

import numpy as np
import pytest
import torch

import flag_cases as fc
from oracle import cem as ocem

N, H = 32, 4
GOAL_VARIANTS = fc.EIGHT + ["norm_null"] + fc.COST_VARIANTS + ["ns+weights"]


def _f64(x):
    return torch.from_numpy(np.asarray(x, np.float64))


def _torch_rollout(p, A):
    """(returns [N], states [H, N, s]) of member 0 through the torch classes, float64."""
    from mbrl_amd import data, models
    cfg = p["cfg"]
    s, a, reward = cfg["s"], cfg["a"], bool(cfg.get("reward"))
    layers = p["model"][0]
    if reward:
        m = models.ModelWithReward(s, a, hidden_units=cfg["W"], n_hidden=cfg["L"]).double()
        (*trunk, (hw, hb)) = layers
        layers = trunk + [(hw[:s], hb[:s]), (hw[s:], hb[s:])]
    else:
        m = models.Model(s, a, hidden_units=cfg["W"], n_hidden=cfg["L"]).double()
    with torch.no_grad():
        for lin, (w, b) in zip(m.linears(), layers):
            lin.weight.copy_(_f64(w))
            lin.bias.copy_(_f64(b))
    stats = p["norm"] if p["norm"] is not None else p["stats"]
    ds = data.TransitionsDataset.from_statistics(
        {name: {"mean": _f64(stats[k + "_mean"]), "std": _f64(stats[k + "_std"])}
         for name, k in (("observations", "obs"), ("actions", "act"), ("rewards", "rew")) if k + "_mean" in stats})
    keys = fc.norm_keys(p)
    kw = {k: v for k, v in ds.normalizers(reward=reward).items() if k in keys}
    assert set(kw) == keys
    fwd = functools.partial(m, **kw)
    c = p["cost"]
    if not reward:
        state_cost = models.SmoothAbsLoss(_f64(c["weights"]), _f64(c["goal"]), c["alpha_state"])
        action_cost = models.CoshLoss(c["alpha_action"])
    st = _f64(np.broadcast_to(p["s0"], (A.shape[1], s)))
    total = torch.zeros(A.shape[1], dtype=torch.float64)
    states = []
    with torch.no_grad():
        for t in range(A.shape[0]):
            at = _f64(A[t])
            if reward:
                st = fwd(st, at)[0]
                total = total + fwd(st, at)[1].reshape(-1)
            else:
                st = fwd(st, at)
                if c.get("has_state", True):
                    total = total + state_cost(st)
                if c.get("has_action", True):
                    total = total + action_cost(at)
            states.append(st)
    return total.numpy(), torch.stack(states).numpy()


def _problem(cid, variant):
    p = fc._sharpen(ocem.synth_problem(cid, N=N, H=H, **fc.VARIANTS[variant]))
    if variant == "norm_null":
        p["stats"], p["norm"] = p["norm"], None
    return p


@pytest.mark.parametrize("cid,variant", [(c, v) for c in (2, 3) for v in GOAL_VARIANTS] + [(6, v) for v in fc.REWARD])
def test_oracle_switches_match_float64_torch(cid, variant):
    p = _problem(cid, variant)
    assert (p["cfg"]["s"], p["cfg"]["a"]) == ((5, 1) if cid == 2 else (17, 6))
    A = fc.actions(p)
    costs, states = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A, store_states=True)
    ref_ret, ref_states = _torch_rollout(p, A)
    assert fc.rel_err(costs[0], ref_ret) < fc.RTOL
    assert float(np.max(np.abs(states[0] - ref_states))) < fc.STATE_BAR
    if variant == "no_cost":
        assert not costs.any() and not ref_ret.any()


def test_cem_plan_honours_the_switches():
    """cem_plan and its final trajectory go through the same rollout: a flag changes both."""
    base = _problem(2, "norm:all")
    ref = ocem.cem_plan(base, N=64, H=H, num_iterations=1)
    for variant in ("norm:na", "weights_alphas", "no_state_cost"):
        got = ocem.cem_plan(_problem(2, variant), N=64, H=H, num_iterations=1)
        assert fc.rel_err(got["returns"][0], ref["returns"][0]) >= fc.MOVE_RETURNS, variant
    got = ocem.cem_plan(_problem(2, "norm:na"), N=64, H=H, num_iterations=1)
    assert float(np.max(np.abs(got["final_states"] - ref["final_states"]))) >= fc.MOVE_STATES


def test_absent_switches_are_todays_problem():
    """synth_problem without the new keywords is unchanged, and an explicit all-on dict equals it."""
    p = ocem.synth_problem(3, N=8, H=2)
    assert set(p["norm"]) == {"obs_mean", "obs_std", "act_mean", "act_std"} and "has_state" not in p["cost"]
    assert np.all(p["cost"]["weights"] == 1) and p["cost"]["alpha_state"] == 0.4 and p["cost"]["alpha_action"] == 0.25
    q = ocem.synth_problem(3, N=8, H=2, norm_flags=fc.NORM_SUBSETS["all"], has_state_cost=True, has_action_cost=True)
    A = fc.actions(p)
    assert np.array_equal(ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A),
                          ocem.rollout(q["model"], q["norm"], q["cost"], q["s0"], A))
