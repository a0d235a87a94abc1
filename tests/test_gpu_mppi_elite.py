"""GPU: MPPI over the K best -- mbrl_mppi_update_elite / _batch (csrc/mppi.hip), mbrl_mppi_plan_elite / _batch and
the planners' num_elites / min_std / max_std / warm_std kwargs.

Update level (costs given as arrays, so the elite set is exact): the elite list equals np.argsort(kind="stable")[:K]
in ascending index; returns and beta equal the NumPy restatement (tests/mppi_elite_reference.py) bit for bit. The
restatement's exponential is the device's expf, which NumPy does not have, so "weights and eta bit-equal to the
restatement" is asserted in the form that can be bit-exact: the weights are exactly 0 outside the valid elites and
bit-equal to mbrl_mppi_update's weights on the masked returns (invalid -> NaN: the restatement "with a mask", run
through the existing kernel), eta is bit-equal to mppi_reference.canonical_sum of those float32 weights, and with the
neutral clamp mu' and sigma' equal that masked classic update byte for byte. Beside that the weights stay within
test_gpu_mppi.py's 2 ulp of float32(exp(float64)), mu' within mppi_reference.mu_bound of the float64 restatement and
the smoothed variance within var_bound (the project's bars, unchanged). Two runs give identical bits; the clamp is
exact on either side. Identities, the fused draw, the batch against the single update and whole plans against their
step-by-step equivalents are byte for byte."""
import functools

import numpy as np
import pytest
import torch

import mppi_elite_reference as eref
import mppi_reference as mref
import standin_env as se
from oracle import cem as ocem

from test_gpu_mppi import _check_update, _costs, _run_update
from test_gpu_mppi_batch import _starts
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
F32 = np.float32
LO, HI = -1.0, 1.0
INF = float("inf")
OUT = ("mu", "sigma", "weights", "returns", "stats")


def _elite_costs(kind, E, N, K, lam, rng):
    """Cost arrays for an update with K elites: `ties` puts an exact tie across the K boundary (members equal, so the
    member mean keeps it), `fewfinite` leaves fewer than K finite returns, `allnan` none."""
    if kind == "ties":
        c = np.tile((100.0 + np.floor(4.0 * rng.standard_normal(N)) * F32(0.5 * lam)).astype(F32), (E, 1))
        order = np.argsort(c[0], kind="stable")
        if K < N:
            c[:, order[K]] = c[:, order[K - 1]]
        return c
    if kind == "fewfinite":
        c = np.full((E, N), np.nan, F32)
        c[:, rng.permutation(N)[:N // 2]] = np.inf
        fin = rng.permutation(N)[:K // 2]
        c[:, fin] = (100.0 + 3.0 * lam * rng.standard_normal((E, len(fin)))).astype(F32)
        return c
    return _costs(kind, E, N, lam, rng)


def _run_elite(c, A, mu, sg, K, lam, alpha, upd, smin=0.0, smax=INF, it=0, seed=11, next_shape=None, off=0):
    from mbrl_amd import fused
    dev = torch.device("cuda", 0)
    H, N, a = A.shape
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    costs, acts, mu_d, sg_d = t(c), t(A), t(mu), t(sg)
    mu_o, sg_o = torch.full_like(mu_d, 7.0), torch.full_like(sg_d, 7.0)
    w, r = (torch.full((N,), -1.0, dtype=torch.float32, device=dev) for _ in range(2))
    st = torch.full((2,), -1.0, dtype=torch.float32, device=dev)
    nxt = torch.empty(next_shape, dtype=torch.float32, device=dev) if next_shape else None
    sp = fused.make_sampler(seed, it, mu_d, sg_d, LO, HI)
    el = fused.mppi_update_elite(costs, acts, sp, K, H, a, lam, alpha, upd, mu_o, sg_o, sigma_min=smin, sigma_max=smax,
                                 weights_out=w, returns_out=r, stats_out=st, next_actions=nxt, draw_offset=off)
    torch.cuda.synchronize()
    out = dict(mu=mu_o.cpu().numpy(), sigma=sg_o.cpu().numpy(), weights=w.cpu().numpy(), returns=r.cpu().numpy(),
               stats=st.cpu().numpy(), elites=el.cpu().numpy())
    if nxt is not None:
        out.update(next=nxt, mu_d=mu_o, sg_d=sg_o)
    return out


def _same(x, y, keys=OUT):
    return [k for k in keys if x[k].tobytes() != y[k].tobytes()]


def _ks(N):
    return sorted({1, min(2, N), max(1, N // 10), max(1, N - 1), N})


KINDS = ("normal", "fewfinite", "allnan", "special")
UPDATE_CASES = [(N, K, a, E) for N in (1, 31, 32, 33, 1024, 1025, 4094) for K in _ks(N) for a in (1, 6, 21, 50)
                for E in (1, 5)]


@functools.lru_cache(maxsize=None)
def _actions(N, a, H=2):
    """One proposal / distribution set per (N, a), shared by the cases (left unchanged)."""
    rng = np.random.default_rng(N * 131 + a * 17)
    A = np.clip(rng.normal(0.1, 0.6, (H, N, a)), LO, HI).astype(F32)
    mu, sg = rng.uniform(-0.3, 0.3, (H, a)).astype(F32), rng.uniform(0.05, 0.6, (H, a)).astype(F32)
    return A, mu, sg


@pytest.mark.parametrize("N,K,a,E", UPDATE_CASES)
def test_update_against_the_restatement(N, K, a, E):
    i = UPDATE_CASES.index((N, K, a, E))
    rng = np.random.default_rng(1000 + i)
    A, mu, sg = _actions(N, a)
    lam, alpha = (1.0, 0.5, 30.0)[i % 3], (0.0, 0.1)[i % 2]
    for kind in ("ties", KINDS[i % 4]):
        upd = bool((i + (kind == "ties")) % 2)
        tag = f"N={N} K={K} a={a} E={E} {kind} upd={int(upd)} lam={lam:g}"
        c = _elite_costs(kind, E, N, K, lam, rng)
        got = _run_elite(c, A, mu, sg, K, lam, alpha, upd)
        ref = eref.update(c, A, mu, sg, lam, alpha, upd, K)
        r = ref["returns"]
        want_el = np.sort(np.argsort(r, kind="stable")[:K])
        assert np.array_equal(got["elites"], want_el) and np.array_equal(ref["elites"], want_el), tag
        if kind == "ties" and K < N:
            s = np.sort(r)
            assert s[K - 1] == s[K], tag                      # the tie does straddle the boundary
        valid = eref.valid_mask(r, K)
        if kind == "fewfinite":
            assert valid.sum() == K // 2 < K, tag
        assert not got["weights"][~valid].any(), tag          # exactly 0 outside the valid elites
        # the project's bars against the float64 restatement (returns and beta bit for bit inside)
        _check_update(got, ref, N, mu, sg, upd, tag)
        # bit for bit: the classic kernel on the masked returns is the restatement with the device's expf
        masked = np.where(valid, r, F32(np.nan)).astype(F32)[None, :]
        classic = _run_update(masked, A, mu, sg, lam, alpha, upd)
        assert _same(got, classic, ("mu", "sigma", "weights", "stats")) == [], tag
        if not ref["unchanged"]:
            assert got["stats"][1].tobytes() == mref.canonical_sum(got["weights"]).tobytes(), tag
        again = _run_elite(c, A, mu, sg, K, lam, alpha, upd)
        assert _same(got, again, OUT + ("elites",)) == [], tag


@pytest.mark.parametrize("N,K,a", [(33, 2, 6), (1025, 102, 21), (4094, 4093, 50)])
def test_the_clamp_is_applied_exactly_on_either_side(N, K, a):
    rng = np.random.default_rng(N)
    A, mu, sg = _actions(N, a)
    c = _elite_costs("normal", 1, N, K, 1.0, rng)
    free = _run_elite(c, A, mu, sg, K, 1.0, 0.1, True)
    lo, hi = float(np.median(free["sigma"])), float(free["sigma"].max())
    assert free["sigma"].min() < lo < hi
    for smin, smax in ((lo, INF), (0.0, lo), (lo, lo), (lo, hi), (0.0, hi), (hi, INF), (2.0, 3.0)):
        got = _run_elite(c, A, mu, sg, K, 1.0, 0.1, True, smin, smax)
        assert got["sigma"].tobytes() == np.clip(free["sigma"], F32(smin), F32(smax)).tobytes(), (smin, smax)
        assert _same(got, free, ("mu", "weights", "returns", "stats", "elites")) == [], (smin, smax)
    classic = _run_elite(c, A, mu, sg, K, 1.0, 0.1, False, 2.0, 3.0)      # without update_sigma: copied unclamped
    assert classic["sigma"].tobytes() == sg.tobytes()
    nan = _run_elite(np.full((1, N), np.nan, F32), A, mu, sg, K, 1.0, 0.1, True, 2.0, 3.0)   # nothing valid: copied
    assert nan["sigma"].tobytes() == sg.tobytes() and nan["mu"].tobytes() == mu.tobytes()


@pytest.mark.parametrize("upd", [False, True])
@pytest.mark.parametrize("N,a,E,kind", [(1, 1, 1, "normal"), (33, 6, 5, "dupmin"), (1025, 21, 1, "special"),
                                        (4094, 50, 5, "normal"), (1000, 6, 1, "allnan"), (4094, 6, 1, "spread")])
def test_all_candidates_elite_is_the_classic_update_byte_for_byte(N, a, E, kind, upd):
    rng = np.random.default_rng(N + a)
    A, mu, sg = _actions(N, a)
    c = _costs(kind, E, N, 1.0, rng)
    got = _run_elite(c, A, mu, sg, N, 1.0, 0.1, upd)
    want = _run_update(c, A, mu, sg, 1.0, 0.1, upd)
    assert _same(got, want) == []
    assert np.array_equal(got["elites"], np.arange(N))


@pytest.mark.parametrize("N,a,E", [(1, 1, 1), (33, 6, 5), (1025, 21, 1), (4094, 50, 5)])
def test_one_elite_without_smoothing_returns_the_best_row(N, a, E):
    rng = np.random.default_rng(N * 3 + a)
    A, mu, sg = _actions(N, a)
    c = _costs("dupmin", E, N, 1.0, rng)
    got = _run_elite(c, A, mu, sg, 1, 0.7, 0.0, True)
    best = int(np.argsort(mref.returns_of(c), kind="stable")[0])
    assert got["elites"].tolist() == [best]
    assert np.array_equal(got["mu"], A[:, best])            # ==: +-0 compare equal
    assert not got["sigma"].any() and got["stats"][1] == 1.0 and np.count_nonzero(got["weights"]) == 1


def test_next_proposals_equal_sample_actions():
    from mbrl_amd import fused
    rng = np.random.default_rng(3)
    N, K, H, a, off, cnt, it, seed = 1000, 100, 2, 6, 37, 901, 2, 0x1234567890ABCDEF
    A, mu, sg = _actions(N, a)
    c = _costs("normal", 1, N, 1.0, rng)
    got = _run_elite(c, A, mu, sg, K, 1.0, 0.1, True, 0.2, 0.45, it=it, seed=seed, next_shape=(H, cnt, a), off=off)
    want = torch.empty_like(got["next"])
    fused.sample_actions(fused.make_sampler(seed, it + 1, got["mu_d"], got["sg_d"], LO, HI), H, a, cnt, off, want)
    torch.cuda.synchronize()
    assert torch.equal(got["next"], want)
    plain = _run_elite(c, A, mu, sg, K, 1.0, 0.1, True, 0.2, 0.45, it=it, seed=seed)    # the draw changes nothing else
    assert _same(got, plain, OUT + ("elites",)) == []


# ------------------------------------------------------------------------------------------------
# the batched update
# ------------------------------------------------------------------------------------------------
BATCH_CASES = {
    (1, 33, 3, 6, 1): ["ties"],
    (2, 31, 31, 1, 5): ["special", "allnan"],
    (3, 1025, 102, 21, 1): ["ties", "allnan", "fewfinite"],
    (4, 4094, 409, 50, 5): ["allnan", "normal", "ties", "special"],
    (5, 1000, 1, 6, 1): ["dupmin", "fewfinite", "normal", "allnan", "ties"],
}


@pytest.mark.parametrize("upd", [False, True])
@pytest.mark.parametrize("case", list(BATCH_CASES), ids=lambda c: "B%d-N%d-K%d-a%d-E%d" % c)
def test_update_batch_equals_the_single_update_per_problem(case, upd):
    from mbrl_amd import fused
    B, N, K, a, E = case
    kinds = BATCH_CASES[case]
    H, lam, alpha, it, seed, smin, smax = 2, 1.5, 0.1, 1, 0x1234567890ABCDEF, 0.2, 0.5
    rng = np.random.default_rng(B * 7919 + N)
    c = np.concatenate([_elite_costs(k, E, N, K, lam, rng) for k in kinds], 1)                    # [E][B N]
    A = np.clip(rng.normal(0.1, 0.6, (H, B * N, a)), LO, HI).astype(F32)
    mu, sg = rng.uniform(-0.3, 0.3, (B, H, a)).astype(F32), rng.uniform(0.05, 0.6, (B, H, a)).astype(F32)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    full = lambda *sh: torch.full(sh, -7.0, dtype=torch.float32, device=dev)  # noqa: E731
    got = dict(mu=full(B, H, a), sigma=full(B, H, a), weights=full(B, N), returns=full(B, N), stats=full(B, 2))
    nxt = full(H, B * N, a)
    mu_d, sg_d = t(mu), t(sg)
    el = fused.mppi_update_elite_batch(t(c), t(A), fused.make_sampler(seed, it, mu_d, sg_d, LO, HI), K, B, H, a, lam, alpha,
                                       upd, got["mu"], got["sigma"], sigma_min=smin, sigma_max=smax,
                                       weights_out=got["weights"], returns_out=got["returns"], stats_out=got["stats"],
                                       next_actions=nxt)
    torch.cuda.synchronize()
    assert el.shape == (B, K)
    for b, kind in enumerate(kinds):
        cb, Ab = c[:, b * N:(b + 1) * N], A[:, b * N:(b + 1) * N]
        one = _run_elite(cb, Ab, mu[b], sg[b], K, lam, alpha, upd, smin, smax, it=it, seed=seed)
        for k in OUT:
            assert got[k][b].cpu().numpy().tobytes() == one[k].tobytes(), (b, kind, k)
        assert np.array_equal(el[b].cpu().numpy(), one["elites"]), (b, kind)       # indices local to the problem
        if kind == "allnan":      # unchanged bit for bit, while its neighbours update
            assert got["mu"][b].cpu().numpy().tobytes() == mu[b].tobytes(), b
            assert got["sigma"][b].cpu().numpy().tobytes() == sg[b].tobytes(), b
        want = torch.empty((H, N, a), dtype=torch.float32, device=dev)
        fused.sample_actions(fused.make_sampler(seed, it + 1, got["mu"][b].contiguous(), got["sigma"][b].contiguous(),
                                                LO, HI), H, a, N, b * N, want)
        torch.cuda.synchronize()
        assert torch.equal(nxt[:, b * N:(b + 1) * N], want), (b, kind)


# ------------------------------------------------------------------------------------------------
# whole plans
# ------------------------------------------------------------------------------------------------
def _plan(p, H, rows=None, **kw):
    from mbrl_amd import MPPIPlanner
    _, model_fn, cost_fn, sample_action = build(p)
    init = None if rows is None else (None, torch.from_numpy(rows))
    kw.setdefault("shift", 0)
    return MPPIPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H,
                                     initial_trajectory=init, seed=p["rng_seed"], record=True, return_device=True, **kw)


def _plan_batch(p, s0s, H, rows=None, sigmas=None, **kw):
    from mbrl_amd import mppi_plan_batch
    _, model_fn, cost_fn, sample_action = build(p)
    inits = None if rows is None else [None if r is None else (None, torch.from_numpy(r)) for r in rows]
    kw.setdefault("shift", 0)
    return mppi_plan_batch(torch.from_numpy(s0s), model_fn, cost_fn, sample_action, H, initial_trajectories=inits,
                           prev_sigmas=sigmas, seed=p["rng_seed"], record=True, return_device=True, **kw)


def _step_by_step(p, res, s0s, rows, sigmas, N, K, H, I, lam, alpha, upd, smin, smax):
    """Every problem of the plan `res` ([B] leading axes; a single plan is passed with them added) against
    sample_actions(n_offset = b N) -> rollout -> mppi_update_elite per iteration and the trajectory: bit for bit."""
    from mbrl_amd import fused
    a, B = p["cfg"]["a"], s0s.shape[0]
    _, model_fn, cost_fn, _ = build(p)
    dev = res["mu"].device
    _, _, prob = fused.describe_problem(model_fn, cost_fn, dev, 0)
    acts = torch.empty((H, N, a), dtype=torch.float32, device=dev)
    for b in range(B):
        s0 = torch.from_numpy(s0s[b]).to(dev)
        mu = torch.zeros((H, a), dtype=torch.float32, device=dev)
        sg = torch.full((H, a), 0.5, dtype=torch.float32, device=dev)
        if rows is not None and rows[b] is not None:
            mu = torch.from_numpy(np.clip(rows[b], F32(LO), F32(HI))).to(dev)
            if sigmas is not None and sigmas[b] is not None:
                sg = torch.from_numpy(sigmas[b]).to(dev)
        assert torch.equal(mu, res["mu_hist"][0, b]) and torch.equal(sg, res["sigma_hist"][0, b]), b
        for it in range(I):
            sp = fused.make_sampler(p["rng_seed"], it, mu, sg, LO, HI)
            fused.sample_actions(sp, H, a, N, b * N, acts)
            costs = fused.rollout(prob, s0, N, H, actions=acts)
            assert torch.equal(costs, res["costs"][it][:, b * N:(b + 1) * N]), (b, it)
            mu_n, sg_n = torch.empty_like(mu), torch.empty_like(sg)
            w = torch.empty(N, dtype=torch.float32, device=dev)
            el = fused.mppi_update_elite(costs, acts, sp, K, H, a, lam, alpha, upd, mu_n, sg_n, sigma_min=smin,
                                         sigma_max=smax, weights_out=w)
            mu, sg = mu_n, sg_n
            assert torch.equal(el, res["elites"][it, b]) and torch.equal(w, res["weights"][it, b]), (b, it)
            assert torch.equal(mu, res["mu_hist"][it + 1, b]) and torch.equal(sg, res["sigma_hist"][it + 1, b]), (b, it)
        actions = mu.clamp(LO, HI).contiguous()
        states = fused.trajectory(prob, s0, actions, H)
        torch.cuda.synchronize()
        assert torch.equal(mu, res["mu"][b]) and torch.equal(sg, res["sigma"][b]), b
        assert torch.equal(actions, res["actions"][b]) and torch.equal(states, res["states"][b]), b


def _as_batch(res):
    """A single plan's records with the problem axis of the batched ones."""
    out = {k: res[k][None] for k in ("mu", "sigma", "actions", "states")}
    out.update({k: res[k][:, None] for k in ("weights", "mu_hist", "sigma_hist", "elites")}, costs=res["costs"])
    return out


# (cid, N, K, H, I, problem overrides, sigma rows, whether the update draws the next proposals)
SINGLE_CASES = [
    pytest.param(3, 1000, 100, 5, 3, {}, False, True, id="draw-slices"),
    pytest.param(3, 300, 1, 4, 2, {}, True, True, id="K1-sigma-rows"),
    pytest.param(5, 300, 300, 3, 2, {}, False, True, id="ensemble-K=N"),
    pytest.param(6, 256, 25, 3, 2, {}, True, True, id="reward-head-sigma-rows"),
    pytest.param(5, 11000, 1100, 2, 2, dict(E=1), False, False, id="above-draw-limit"),
    pytest.param(5, 6000, 600, 2, 2, dict(E=1), True, True, id="below-draw-limit-sigma-rows"),
]


@pytest.mark.parametrize("cid,N,K,H,I,over,with_sigma,update_draws", SINGLE_CASES)
def test_plan_equals_its_step_by_step_equivalent(cid, N, K, H, I, over, with_sigma, update_draws):
    p = ocem.synth_problem(cid, N=N, H=H, **over)
    a, lam, alpha, smin, smax = p["cfg"]["a"], 1.5, 0.1, 0.1, 0.45
    assert (N * ((a + 3) // 4) <= 65536) == update_draws
    rng = np.random.default_rng(N + K)
    rows = sig = None
    kw = {}
    if with_sigma:
        rows, sig = rng.uniform(-1.3, 1.3, (H, a)).astype(F32), rng.uniform(0.05, 0.7, (H, a)).astype(F32)
        kw = dict(warm_std="keep", prev_sigma=sig)
    res = _plan(p, H, rows=rows, num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=True,
                num_elites=K, min_std=smin, max_std=smax, **kw)
    assert res["elites"].shape == (I, K) and res["elites"].dtype == torch.int64
    _step_by_step(p, _as_batch(res), p["s0"][None], None if rows is None else [rows], None if sig is None else [sig],
                  N, K, H, I, lam, alpha, True, smin, smax)
    sg = res["sigma_hist"][1:]
    assert bool((sg >= F32(smin)).all()) and bool((sg <= F32(smax)).all())


def test_plan_batch_with_mixed_input_flags_and_problem_zero_is_the_single_plan():
    """Problem 0: mean and sigma rows; 1: cold; 2: mean rows only; 3: both. Then problem 0 of the batch and a batch
    of one against the single plan, byte for byte."""
    cid, B, N, K, H, I, lam, alpha, smin, smax = 3, 4, 300, 30, 4, 2, 1.5, 0.1, 0.1, 0.45
    p = ocem.synth_problem(cid, N=N, H=H)
    rng = np.random.default_rng(9)
    mk = lambda: rng.uniform(-1.4, 1.4, (H, 6)).astype(F32)  # noqa: E731
    sk = lambda: rng.uniform(0.05, 0.7, (H, 6)).astype(F32)  # noqa: E731
    rows, sigmas = [mk(), None, mk(), mk()], [sk(), None, None, sk()]
    s0s = _starts(p, B)
    kw = dict(num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=True, num_elites=K,
              min_std=smin, max_std=smax, warm_std="keep")
    res = _plan_batch(p, s0s, H, rows=rows, sigmas=sigmas, **kw)
    assert res["elites"].shape == (I, B, K)
    assert not res["mu_hist"][0, 1].any() and bool((res["sigma_hist"][0, 1] == 0.5).all())
    assert bool((res["sigma_hist"][0, 2] == 0.5).all())
    assert np.array_equal(res["sigma_hist"][0, 3].cpu().numpy(), sigmas[3])
    _step_by_step(p, res, s0s, rows, sigmas, N, K, H, I, lam, alpha, True, smin, smax)
    single = _plan(p, H, rows=rows[0], prev_sigma=sigmas[0], **kw)
    one = _plan_batch(p, s0s[:1], H, rows=rows[:1], sigmas=sigmas[:1], **kw)
    torch.cuda.synchronize()
    for tag, r in (("problem 0", res), ("B = 1", one)):
        for k in ("states", "actions", "mu", "sigma"):
            assert torch.equal(r[k][0], single[k]), (tag, k)
        assert torch.equal(r["costs"][:, :, :N], single["costs"]), tag
        for k in ("weights", "mu_hist", "sigma_hist", "elites"):
            assert torch.equal(r[k][:, 0], single[k]), (tag, k)


@pytest.mark.parametrize("cid,B,N,K,H,I,over", [(5, 2, 256, 25, 3, 2, {}), (6, 3, 256, 256, 3, 2, {}),
                                                (5, 2, 11000, 1100, 2, 2, dict(E=1))],
                         ids=["ensemble", "reward-head-K=N", "above-draw-limit"])
def test_plan_batch_equals_its_step_by_step_equivalent(cid, B, N, K, H, I, over):
    p = ocem.synth_problem(cid, N=N, H=H, **over)
    s0s = _starts(p, B)
    res = _plan_batch(p, s0s, H, num_candidates=N, num_iterations=I, temperature=1.5, alpha=0.1, update_sigma=True,
                      num_elites=K, min_std=0.1, max_std=0.45)
    _step_by_step(p, res, s0s, None, None, N, K, H, I, 1.5, 0.1, True, 0.1, 0.45)


@pytest.mark.parametrize("case", eref.PLAN_CASES, ids=lambda c: "cfg%d-N%d-K%d" % (c[0], c[1], c[4]))
def test_plan_against_the_restatement_with_identical_elite_sets(case):
    """On a fixture whose elite boundary is clear (tests/test_mppi_elite_host.py asserts the gap on the CPU): the
    device plan selects the reference plan's sets, and each iteration's update meets the MPPI bars on the device's
    own costs."""
    from oracle.philox import cem_actions
    cid, N, H, I, K, lam, alpha, upd, smin, smax, _ = case
    p = eref.case_problem(case)
    ref_plan = eref.case_plan(case)
    res = _plan(p, H, num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=upd, num_elites=K,
                min_std=smin, max_std=None if smax == INF else smax)
    torch.cuda.synchronize()
    mu_h, sg_h = res["mu_hist"].cpu().numpy(), res["sigma_hist"].cpu().numpy()
    for i in range(I):
        assert np.array_equal(res["elites"][i].cpu().numpy(), ref_plan["elites"][i]), i
        A = cem_actions(mu_h[i], sg_h[i], LO, HI, p["rng_seed"], i, np.arange(N))
        got_c = res["costs"][i].cpu().numpy()
        ref_c = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A)
        err = float(np.max(np.abs(got_c - ref_c) / np.maximum(np.abs(ref_c), 1.0)))
        print(f"mppi-elite-plan cid={cid} it={i}: cost rel err {err:.3g}, reference gap {ref_plan['gaps'][i]:.3g}")
        assert err < 1e-5, (i, err)
        ref = eref.update(got_c, A, mu_h[i], sg_h[i], lam, alpha, upd, K)          # (var: before the clamp)
        free = np.sqrt(ref["var"])
        inside = (free > smin) & (free < smax)
        got_sg = np.where(inside, sg_h[i + 1], free.astype(F32))                   # clamped entries checked below
        got = dict(mu=mu_h[i + 1], sigma=got_sg, weights=res["weights"][i].cpu().numpy(), returns=ref["returns"],
                   stats=np.array([ref["beta"], ref["eta"]], F32))
        _check_update(got, ref, N, mu_h[i], sg_h[i], upd, f"elite plan cid={cid} it={i}")
        assert np.all(sg_h[i + 1][free < smin * (1 - 1e-6)] == F32(smin)), i
        assert np.all(sg_h[i + 1][free > smax * (1 + 1e-6)] == F32(smax)), i
    assert torch.equal(res["actions"], res["mu"].clamp(LO, HI))


def test_num_elites_none_is_todays_plan_byte_for_byte():
    N, H, I = 300, 4, 2
    p = ocem.synth_problem(3, N=N, H=H)
    kw = dict(num_candidates=N, num_iterations=I, temperature=1.5, alpha=0.1, update_sigma=True)
    base = _plan(p, H, **kw)
    none = _plan(p, H, num_elites=None, min_std=0.0, max_std=None, **kw)
    full = _plan(p, H, num_elites=N, **kw)                    # K = N, the neutral clamp: the same bits, other entry
    assert "elites" not in none and full["elites"].shape == (I, N)
    for k in ("states", "actions", "mu", "sigma", "costs", "weights", "mu_hist", "sigma_hist"):
        assert torch.equal(base[k], none[k]) and torch.equal(base[k], full[k]), k
    cut = _plan(p, H, num_elites=30, **kw)
    assert not torch.equal(cut["mu"], base["mu"])
    assert int((cut["weights"] != 0).sum(1).max()) <= 30


def test_generic_path_runs_the_restricted_update():
    from mbrl_amd import MPPIPlanner, fused
    N, H, K = 400, 3, 40
    p = ocem.synth_problem(3, N=N, H=H)
    _, model_fn, cost_fn, sample_action = build(p)
    wrapped = lambda s, a: model_fn(s, a)  # noqa: E731
    assert fused.describe_model(wrapped) is None
    kw = dict(num_candidates=N, num_iterations=2, temperature=1.0e4, update_sigma=True, seed=p["rng_seed"], record=True,
              return_device=True, num_elites=K, min_std=0.3, max_std=0.45)
    gn = MPPIPlanner.plan_detailed(torch.from_numpy(p["s0"]), wrapped, cost_fn, sample_action, H, **kw)
    torch.cuda.synchronize()
    assert gn["elites"].shape == (2, K) and int((gn["weights"] != 0).sum(1).max()) == K
    for i in range(2):
        want = np.sort(np.argsort(gn["costs"][i][0].cpu().numpy(), kind="stable")[:K])
        assert np.array_equal(gn["elites"][i].cpu().numpy(), want)
    assert bool((gn["sigma_hist"][1:] >= F32(0.3)).all()) and bool((gn["sigma_hist"][1:] <= F32(0.45)).all())


def test_planner_service_passes_the_kwargs_through():
    """Served actions equal direct mppi_plan_batch calls with the same previous plans and the same kwargs."""
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
    H, kw = 10, dict(num_candidates=256, num_iterations=2, seed=11, update_sigma=True, num_elites=25, min_std=0.2,
                     max_std=0.6, warm_std=0.4)
    pol = MPCPolicy(model_fn, cost, BatchedMPPIPlanner, sample_action, H, **kw)
    batches = []
    rs = parallel.get_rollouts_parallel("linear", "run", True, 3, dict(num_steps=3, get_action=pol.get_action),
                                        num_workers=2, env_factory=se.make_env,
                                        on_batch=lambda i, o, a: batches.append((list(i), o, a)))
    prev, steps, warm = {}, {i: 0 for i in range(3)}, 0
    for idx, obs, acts in batches:
        inits = [None if steps[i] == 0 else (prev[i][0][1:], prev[i][1]) for i in idx]
        res = mppi_plan_batch(obs, model_fn, cost, sample_action, H, initial_trajectories=inits, record=True, **kw)
        assert torch.equal(res["actions"][:, 0].reshape(len(idx), -1), acts)
        assert res["elites"].shape == (2, len(idx), 25)
        assert bool((res["sigma"] >= F32(0.2)).all()) and bool((res["sigma"] <= F32(0.6)).all())
        for b, i in enumerate(idx):
            want = 0.5 if steps[i] == 0 else 0.4           # warm_std applies to warm-started problems only
            assert bool((res["sigma_hist"][0, b] == F32(want)).all()), (i, steps[i])
            warm += steps[i] > 0
            prev[i] = (res["states"][b], res["actions"][b])
            steps[i] += 1
    assert warm >= 3 and len(rs) == 3
