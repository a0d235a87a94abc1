"""The half-group layer hand-offs of the 8-wave ring rollout (rollout_kernel GS, DESIGN.md §3.1;
mbrl_set_option(MBRL_OPT_ROLLOUT_GROUP_SEAM, 1 on / 2 off)) against the full-barrier seams. The MFMA
and summation orders are the same, so costs and states must agree BIT FOR BIT. Every case forces
16-row tiles (MBRL_OPT_ROLLOUT_TILE = 16: small N would otherwise take the 8-candidate kernel, which
has no such seam), so both runs go through rollout_kernel's 8-wave ring instances."""
import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.philox import cem_actions

from test_gpu_parity import DEV, build, device_problem

pytestmark = pytest.mark.gpu

CASES = [
    pytest.param(3, 16, 3, {}, id="cheetah-one-tile"),                 # W=512, s=17, a=6, L=3
    pytest.param(3, 17, 3, {}, id="cheetah-two-tiles-one-ragged"),
    pytest.param(3, 16, 3, dict(L=2), id="L2-only-the-layer0-seam"),
    pytest.param(3, 16, 3, dict(L=4), id="L4-both-ping-pong-directions"),
    pytest.param(3, 16, 3, dict(W=256), id="W256-narrower-ring-instance"),
    pytest.param(4, 8192, 2, {}, id="walker-32-candidate-tiles"),      # s=24: the R = 2, 8-wave instance
    pytest.param(6, 16, 2, {}, id="reward-head-two-passes-per-step"),
]


def _rollout(prob, p, N, H, A, seam):
    from mbrl_amd import _lib, fused
    E, s = p["cfg"]["E"], p["cfg"]["s"]
    states = torch.empty((E, H, N, s), dtype=torch.float32, device=DEV)
    with _lib.option("rollout_tile", 16), _lib.option("rollout_group_seam", seam):
        costs = fused.rollout(prob, torch.from_numpy(p["s0"]).to(DEV), N, H, actions=torch.from_numpy(A).to(DEV),
                              states_out=states)
    torch.cuda.synchronize()
    return costs, states


@pytest.mark.parametrize("cid,N,H,over", CASES)
def test_group_seam_rollout_equals_full_barrier_bitwise(cid, N, H, over):
    p = ocem.synth_problem(cid, N=N, H=H, **over)
    a = p["cfg"]["a"]
    A = cem_actions(np.zeros((H, a), np.float32), np.full((H, a), 0.5, np.float32), -1, 1, 5, 0, np.arange(N))
    prob = device_problem(p)
    c_off, s_off = _rollout(prob, p, N, H, A, 2)
    c_on, s_on = _rollout(prob, p, N, H, A, 1)
    assert bool(torch.isfinite(c_off).all())
    assert torch.equal(c_on, c_off), float((c_on - c_off).abs().max())
    assert torch.equal(s_on, s_off)


def test_group_seam_plan_equals_full_barrier_plan():
    """One whole recorded CEM plan (cheetah, N=64, H=3, I=2) with the seam forced off and on."""
    from mbrl_amd import CEMPlanner, _lib
    p = ocem.synth_problem(3, N=64, H=3)
    _, model_fn, cost_fn, sample_action = build(p)
    out = {}
    for seam in (2, 1):
        with _lib.option("rollout_tile", 16), _lib.option("rollout_group_seam", seam):
            out[seam] = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, 3,
                                                 num_candidates=64, num_iterations=2, seed=p["rng_seed"],
                                                 record=True)
    for k in ("returns", "elites", "mu", "sigma", "actions", "states"):
        assert torch.equal(out[1][k], out[2][k]), k
