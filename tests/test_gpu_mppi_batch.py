"""GPU: batched MPPI -- the update for B problems in one launch (mbrl_mppi_update_batch), the batched plan
(mbrl_mppi_plan_batch, mppi_plan_batch) and BatchedMPPIPlanner behind the planner service.

The batched update must equal mbrl_mppi_update on contiguous copies of each problem's slices byte for byte,
and the batched plan its step-by-step equivalent per problem (sample_actions with n_offset = b N -> rollout on
s0[b] -> mppi_update, then the trajectory), also byte for byte; problem 0 of a batch and a B = 1 batch are
MPPIPlanner.plan_detailed byte for byte. Against the NumPy reference (tests/mppi_reference.py) the bars are
test_gpu_mppi.py's (_check_update), and costs within 1e-5 relative."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mppi_reference as mref
import standin_env as se
from oracle import cem as ocem
from oracle.philox import cem_actions

from test_gpu_mppi import _check_update, _costs, _run_update
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
F32 = np.float32
LO, HI = -1.0, 1.0

# (B, N, a, H, E) -> each problem's cost kind (an all-NaN problem beside finite ones wherever B > 1) and the
# batch's temperature; a = 30 and 50 take the kernel's 16- and 8-chunk tiles, N = 1025 a second level-2 group
UPDATE_CASES = {
    (1, 33, 6, 1, 1): (["normal"], 1.0),
    (3, 31, 6, 2, 5): (["special", "allnan", "dupmin"], 2.0),
    (4, 1025, 21, 2, 1): (["normal", "allnan", "spread", "dupmin"], 1e-6),
    (2, 4094, 30, 1, 5): (["allnan", "special"], 1e6),
    (5, 1000, 50, 1, 1): (["dupmin", "spread", "normal", "allnan", "special"], 0.5),
}


def _update_inputs(case):
    B, N, a, H, E = case
    kinds, lam = UPDATE_CASES[case]
    rng = np.random.default_rng(B * 7919 + N * 131 + a * 17 + H + E)
    c = np.concatenate([_costs(k, E, N, lam, rng) for k in kinds], 1)                    # [E][B N]
    A = np.clip(rng.normal(0.1, 0.6, (H, B * N, a)), LO, HI).astype(F32)
    mu = rng.uniform(-0.3, 0.3, (B, H, a)).astype(F32)
    sg = rng.uniform(0.05, 0.6, (B, H, a)).astype(F32)
    return kinds, lam, c, A, mu, sg


def _run_batch(c, A, mu, sg, B, lam, alpha, upd, it, seed):
    from mbrl_amd import fused
    dev = torch.device("cuda", 0)
    H, BN, a = A.shape
    N = BN // B
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    costs, acts, mu_d, sg_d = t(c), t(A), t(mu), t(sg)
    full = lambda *sh: torch.full(sh, -7.0, dtype=torch.float32, device=dev)  # noqa: E731
    out = dict(mu=full(B, H, a), sigma=full(B, H, a), weights=full(B, N), returns=full(B, N), stats=full(B, 2),
               next=full(H, BN, a))
    sp = fused.make_sampler(seed, it, mu_d, sg_d, LO, HI)
    fused.mppi_update_batch(costs, acts, sp, B, H, a, lam, alpha, upd, out["mu"], out["sigma"], weights_out=out["weights"],
                            returns_out=out["returns"], stats_out=out["stats"], next_actions=out["next"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("upd", [False, True])
@pytest.mark.parametrize("case", list(UPDATE_CASES), ids=lambda c: "B%d-N%d-a%d-H%d-E%d" % c)
def test_update_batch_equals_the_single_update_per_problem(case, upd):
    from mbrl_amd import fused
    B, N, a, H, E = case
    kinds, lam, c, A, mu, sg = _update_inputs(case)
    alpha, it, seed = 0.1, 1, 0x1234567890ABCDEF
    got = _run_batch(c, A, mu, sg, B, lam, alpha, upd, it, seed)
    for b, kind in enumerate(kinds):
        cb, Ab = c[:, b * N:(b + 1) * N], A[:, b * N:(b + 1) * N]
        one = _run_update(cb, Ab, mu[b], sg[b], lam, alpha, upd, it=it, seed=seed)
        for k in ("mu", "sigma", "weights", "returns", "stats"):
            assert got[k][b].cpu().numpy().tobytes() == one[k].tobytes(), (b, kind, k)
        if kind == "allnan":      # unchanged bit for bit, while its neighbours update
            assert got["mu"][b].cpu().numpy().tobytes() == mu[b].tobytes(), b
            assert got["sigma"][b].cpu().numpy().tobytes() == sg[b].tobytes(), b
            assert not got["weights"][b].any() and np.isnan(got["stats"][b, 0].item()), b
        else:
            assert got["mu"][b].cpu().numpy().tobytes() != mu[b].tobytes(), b
        want = torch.empty((H, N, a), dtype=torch.float32, device=got["next"].device)
        fused.sample_actions(fused.make_sampler(seed, it + 1, got["mu"][b].contiguous(), got["sigma"][b].contiguous(),
                                                LO, HI), H, a, N, b * N, want)
        torch.cuda.synchronize()
        assert torch.equal(got["next"][:, b * N:(b + 1) * N], want), (b, kind)
    if case == (3, 31, 6, 2, 5):   # and against the reference, at the single update's bars
        for b in range(B):
            cb, Ab = c[:, b * N:(b + 1) * N], A[:, b * N:(b + 1) * N]
            ref = mref.update(cb, Ab, mu[b], sg[b], lam, alpha, upd)
            one = {k: got[k][b].cpu().numpy() for k in ("mu", "sigma", "weights", "returns", "stats")}
            _check_update(one, ref, N, mu[b], sg[b], upd, f"batch problem {b} ({kinds[b]}) upd={int(upd)}")


# ------------------------------------------------------------------------------------------------
# whole plans
# ------------------------------------------------------------------------------------------------
def _starts(p, B, seed=1):
    """B start states: the problem's own first, then perturbed ones."""
    rng = np.random.default_rng(seed)
    s0 = np.stack([p["s0"]] + [(p["s0"] + 0.1 * rng.standard_normal(p["s0"].shape)).astype(F32) for _ in range(B - 1)])
    return s0.astype(F32)


def _plan_batch(p, s0s, H, rows=None, **kw):
    from mbrl_amd import mppi_plan_batch
    _, model_fn, cost_fn, sample_action = build(p)
    inits = None if rows is None else [None if r is None else (None, torch.from_numpy(r)) for r in rows]
    kw.setdefault("shift", 0)
    return mppi_plan_batch(torch.from_numpy(s0s), model_fn, cost_fn, sample_action, H, initial_trajectories=inits,
                           seed=p["rng_seed"], record=True, return_device=True, **kw)


def _step_by_step(p, res, s0s, rows, N, H, I, lam, alpha, upd):
    """Every problem of the batched plan `res` against sample_actions(n_offset = b N) -> rollout on s0[b] ->
    mppi_update per iteration and the trajectory: bit for bit."""
    from mbrl_amd import fused
    a, B = p["cfg"]["a"], s0s.shape[0]
    _, model_fn, cost_fn, _ = build(p)
    dev = res["mu"].device
    _, _, prob = fused.describe_problem(model_fn, cost_fn, dev, 0)
    acts = torch.empty((H, N, a), dtype=torch.float32, device=dev)
    for b in range(B):
        s0 = torch.from_numpy(s0s[b]).to(dev)
        mu = torch.zeros((H, a), dtype=torch.float32, device=dev)
        if rows is not None and rows[b] is not None:
            mu = torch.from_numpy(np.clip(rows[b], F32(LO), F32(HI))).to(dev)
        sg = torch.full((H, a), 0.5, dtype=torch.float32, device=dev)
        assert torch.equal(mu, res["mu_hist"][0, b]) and torch.equal(sg, res["sigma_hist"][0, b]), b
        for it in range(I):
            sp = fused.make_sampler(p["rng_seed"], it, mu, sg, LO, HI)
            fused.sample_actions(sp, H, a, N, b * N, acts)
            costs = fused.rollout(prob, s0, N, H, actions=acts)
            assert torch.equal(costs, res["costs"][it][:, b * N:(b + 1) * N]), (b, it)
            mu_n, sg_n = torch.empty_like(mu), torch.empty_like(sg)
            fused.mppi_update(costs, acts, sp, H, a, lam, alpha, upd, mu_n, sg_n)
            mu, sg = mu_n, sg_n
            assert torch.equal(mu, res["mu_hist"][it + 1, b]) and torch.equal(sg, res["sigma_hist"][it + 1, b]), (b, it)
        actions = mu.clamp(LO, HI).contiguous()
        states = fused.trajectory(prob, s0, actions, H)
        torch.cuda.synchronize()
        assert torch.equal(mu, res["mu"][b]) and torch.equal(sg, res["sigma"][b]), b
        assert torch.equal(actions, res["actions"][b]) and torch.equal(states, res["states"][b]), b


# (cid, B, N, H, I, upd, problem overrides, whether the update draws the next proposals)
PLAN_CASES = [
    pytest.param(3, 3, 300, 4, 2, True, {}, True, id="fused-draw-N300"),            # N no multiple of 32
    pytest.param(3, 2, 1000, 5, 3, True, {}, True, id="draw-slices"),               # S > 1
    pytest.param(5, 2, 256, 3, 2, True, {}, True, id="ensemble-E5"),
    pytest.param(6, 2, 256, 3, 2, False, {}, True, id="reward-head-classic"),
    pytest.param(5, 2, 11000, 2, 2, True, dict(E=1), False, id="above-draw-limit-rollout-side-draw"),
    pytest.param(5, 2, 6000, 2, 2, True, dict(E=1), True, id="below-draw-limit-update-draws"),
]


@pytest.mark.parametrize("cid,B,N,H,I,upd,over,update_draws", PLAN_CASES)
def test_plan_batch_equals_its_step_by_step_equivalent(cid, B, N, H, I, upd, over, update_draws):
    p = ocem.synth_problem(cid, N=N, H=H, **over)
    a, lam, alpha = p["cfg"]["a"], 1.5, 0.1
    # the branch the plan takes: the update draws the next proposals while N ceil(a / 4) <= 65536
    assert (N * ((a + 3) // 4) <= 65536) == update_draws
    s0s = _starts(p, B)
    res = _plan_batch(p, s0s, H, num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=upd)
    assert res["costs"].shape == (I, len(p["model"]), B * N) and res["weights"].shape == (I, B, N)
    assert res["mu_hist"].shape == (I + 1, B, H, a) and res["states"].shape == (B, H, p["cfg"]["s"])
    _step_by_step(p, res, s0s, None, N, H, I, lam, alpha, upd)


def test_plan_batch_with_mixed_warm_start_flags():
    """Rows for problems 0 and 2 (some outside the bounds), none for problem 1."""
    cid, B, N, H, I = 3, 3, 300, 4, 2
    p = ocem.synth_problem(cid, N=N, H=H)
    rng = np.random.default_rng(9)
    rows = [rng.uniform(-1.4, 1.4, (H, 6)).astype(F32), None, rng.uniform(-1.4, 1.4, (H, 6)).astype(F32)]
    assert all((np.abs(r) > 1).any() for r in rows if r is not None)
    s0s = _starts(p, B)
    res = _plan_batch(p, s0s, H, rows=rows, num_candidates=N, num_iterations=I, temperature=1.5, alpha=0.1,
                      update_sigma=True)
    assert not res["mu_hist"][0, 1].any()
    assert np.array_equal(res["mu_hist"][0, 2].cpu().numpy(), np.clip(rows[2], F32(LO), F32(HI)))
    _step_by_step(p, res, s0s, rows, N, H, I, 1.5, 0.1, True)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_problem_zero_and_a_batch_of_one_are_the_single_plan(warm):
    from mbrl_amd import MPPIPlanner
    N, H, I, B = 300, 4, 2, 3
    p = ocem.synth_problem(3, N=N, H=H)
    _, model_fn, cost_fn, sample_action = build(p)
    rng = np.random.default_rng(4)
    row = rng.uniform(-1.3, 1.3, (H, 6)).astype(F32) if warm else None
    kw = dict(num_candidates=N, num_iterations=I, temperature=1.5, alpha=0.1, update_sigma=True)
    single = MPPIPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H,
                                       initial_trajectory=None if row is None else (None, torch.from_numpy(row)),
                                       seed=p["rng_seed"], record=True, return_device=True, shift=0, **kw)
    s0s = _starts(p, B)
    for nb in (B, 1):
        rows = None if row is None else [row] + [None] * (nb - 1)
        res = _plan_batch(p, s0s[:nb], H, rows=rows, **kw)
        torch.cuda.synchronize()
        for k in ("states", "actions", "mu", "sigma"):
            assert torch.equal(res[k][0], single[k]), (nb, k)
        assert torch.equal(res["costs"][:, :, :N], single["costs"]), nb
        for k in ("weights", "mu_hist", "sigma_hist"):
            assert torch.equal(res[k][:, 0], single[k]), (nb, k)


def test_plan_batch_against_the_reference_from_its_own_records():
    cid, B, N, H, I, lam, alpha, upd = 3, 2, 300, 4, 2, 2.0, 0.1, True
    p = ocem.synth_problem(cid, N=N, H=H)
    s0s = _starts(p, B)
    res = _plan_batch(p, s0s, H, num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=upd)
    torch.cuda.synchronize()
    mu_h, sg_h = res["mu_hist"].cpu().numpy(), res["sigma_hist"].cpu().numpy()
    costs, weights = res["costs"].cpu().numpy(), res["weights"].cpu().numpy()
    for b in range(B):
        for i in range(I):
            A = cem_actions(mu_h[i, b], sg_h[i, b], LO, HI, p["rng_seed"], i, b * N + np.arange(N))
            got_c = costs[i][:, b * N:(b + 1) * N]
            ref_c = ocem.rollout(p["model"], p["norm"], p["cost"], s0s[b], A)
            err = float(np.max(np.abs(got_c - ref_c) / np.maximum(np.abs(ref_c), 1.0)))
            print(f"mppi-batch-plan problem {b} it={i}: cost rel err {err:.3g}")
            assert err < 1e-5, (b, i, err)
            ref = mref.update(got_c, A, mu_h[i, b], sg_h[i, b], lam, alpha, upd)
            got = dict(mu=mu_h[i + 1, b], sigma=sg_h[i + 1, b], weights=weights[i, b], returns=ref["returns"],
                       stats=np.array([ref["beta"], ref["eta"]], F32))
            _check_update(got, ref, N, mu_h[i, b], sg_h[i, b], upd, f"batch plan problem {b} it={i}")
    assert torch.equal(res["actions"], res["mu"].clamp(LO, HI))


def test_planner_service_serves_batched_mppi_with_warm_starts():
    """Workers step stand-in environments; the parent answers every lockstep round with one
    BatchedMPPIPlanner.plan_batch, each rollout warm-started from its own previous plan."""
    from mbrl_amd import BatchedMPPIPlanner, MPCPolicy, data, fused, models, mppi_plan_batch, parallel
    from mbrl_amd import env as menv
    from mbrl_amd import env_wrappers as ew
    torch.manual_seed(0)
    m = models.Model(5, 1, hidden_units=256, n_hidden=2)
    ds = data.TransitionsDataset.from_statistics({"observations": {"mean": torch.zeros(5), "std": torch.ones(5)},
                                                  "actions": {"mean": torch.zeros(1), "std": torch.ones(1)}})
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(5), torch.zeros(5)), models.CoshLoss())
    sample_action = functools.partial(ew.EnvWrapper._sample_action, action_spec=menv.BoundedActionSpec(1))
    model_fn = functools.partial(m, **ds.normalizers())
    assert fused.describe_model(model_fn) is not None
    H, kw = 10, dict(num_candidates=256, num_iterations=2, seed=11)
    pol = MPCPolicy(model_fn, cost, BatchedMPPIPlanner, sample_action, H, **kw)
    batches = []
    rs = parallel.get_rollouts_parallel("linear", "run", True, 3, dict(num_steps=4, get_action=pol.get_action),
                                        num_workers=2, env_factory=se.make_env,
                                        on_batch=lambda i, o, a: batches.append((list(i), o, a)))
    prev, steps, warm_rounds = {}, {i: 0 for i in range(3)}, 0
    answers = {i: [] for i in range(3)}
    for idx, obs, acts in batches:
        inits = [None if steps[i] == 0 else (prev[i][0][1:], prev[i][1]) for i in idx]
        res = mppi_plan_batch(obs, model_fn, cost, sample_action, H, initial_trajectories=inits, record=True, **kw)
        assert torch.equal(res["actions"][:, 0].reshape(len(idx), -1), acts)
        for b, i in enumerate(idx):
            if steps[i] == 0:
                assert not res["mu_hist"][0, b].any()
            else:             # the previous plan shifted by one step, its last row repeated
                last = prev[i][1]
                assert torch.equal(res["mu_hist"][0, b], torch.cat([last[1:], last[-1:]], 0)), (i, steps[i])
                warm_rounds += 1
            prev[i] = (res["states"][b], res["actions"][b])
            steps[i] += 1
            answers[i].append(acts[b])
    assert warm_rounds >= 3       # every rollout was warm-started at least once
    for i, r in enumerate(rs):
        assert len(r) == 4
        assert all(torch.equal(torch.as_tensor(x).reshape(-1), y) for x, y in zip(r.actions[:-1], answers[i]))


def test_limits_are_refused_before_any_launch():
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    N, H = 64, 3
    p = ocem.synth_problem(3, N=N, H=H)
    _, model_fn, cost_fn, _ = build(p)
    dev = torch.device("cuda", 0)
    _, _, prob = fused.describe_problem(model_fn, cost_fn, dev, 0)
    a, s = p["cfg"]["a"], p["cfg"]["s"]
    canary = lambda *sh: torch.full(sh, 123.5, dtype=torch.float32, device=dev)  # noqa: E731
    outs = [canary(2, H, a), canary(2, H, a), canary(2, H, a), canary(2, H, s)]
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    s0 = torch.zeros((65536, s), dtype=torch.float32, device=dev)

    def plan(B, n):
        params = _lib.MppiParams(n, H, 1, 0, 1.0, 0.0, LO, HI, 0.0, 0.5, 7)
        return lib.mbrl_mppi_plan_batch(*prob.refs, _lib.ptr(s0), B, ctypes.byref(params), None, None,
                                        *[_lib.ptr(x) for x in outs], None, None, None, None, _lib.ptr(ws), 1 << 40,
                                        _lib.stream_handle(dev))
    assert plan(65536, N) == _lib.MBRL_EUNSUPPORTED and b"65535" in lib.mbrl_last_error()
    assert plan(2, 32769) == _lib.MBRL_EUNSUPPORTED and b"32768" in lib.mbrl_last_error()
    # the update alone: the same limits
    costs, acts = torch.zeros((1, 2 * N), device=dev), torch.zeros((H, 2 * N, a), device=dev)
    mu, sg = torch.zeros((2, H, a), device=dev), torch.ones((2, H, a), device=dev)
    sp = fused.make_sampler(1, 0, mu, sg, LO, HI)

    def update(B, n):
        return lib.mbrl_mppi_update_batch(_lib.ptr(costs), 1, n, B, _lib.ptr(acts), ctypes.byref(sp), H, a, 1.0, 0.0, 0,
                                          _lib.ptr(outs[0]), _lib.ptr(outs[1]), None, None, None, None,
                                          _lib.stream_handle(dev))
    assert update(65536, N) == _lib.MBRL_EUNSUPPORTED
    assert update(2, 32769) == _lib.MBRL_EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((x == 123.5).all()) for x in outs)
