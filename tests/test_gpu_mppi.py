"""GPU: the MPPI update kernel (csrc/mppi.hip), mbrl_mppi_plan and MPPIPlanner.

The update alone runs on synthetic costs and actions (no model, so large N is quick) against the
NumPy reference (tests/mppi_reference.py): returns and beta bit for bit, weights within 2 ulp of
float32(exp(float64)), mu within (D + 8) 2^-24 max(|lo|, |hi|) and the smoothed variance within
(D + 8) 2^-24 (hi - lo)^2, D the chain length of the documented summation order. Whole plans are
checked iteration by iteration from the GPU's own records, against their step-by-step equivalent
(bit for bit), with a warm start, through MPCPolicy and on the generic path.

Largest errors measured over the update parametrisation on an MI355X (as fractions of the bound):
see DESIGN.md "MPPI"."""
import ctypes

import numpy as np
import pytest
import torch

import mppi_reference as mref
from oracle import cem as ocem
from oracle.philox import cem_actions

from test_gpu_parity import build

pytestmark = pytest.mark.gpu
F32 = np.float32
LO, HI = -1.0, 1.0


def _costs(kind, E, N, lam, rng):
    lam = float(lam)
    if kind == "normal":
        c = (100.0 + 3.0 * lam * rng.standard_normal((E, N))).astype(F32)
    elif kind == "equal":
        c = np.full((E, N), 42.5, F32)
    elif kind == "spread":       # steps of 1e6 lambda: all but the minimum underflow to 0
        c = np.tile((1e6 * lam * rng.permutation(N)).astype(F32), (E, 1))
    elif kind == "dupmin":
        c = (100.0 + 3.0 * lam * np.abs(rng.standard_normal((E, N)))).astype(F32)
        c[:, rng.integers(0, N, min(N, 3))] = F32(100.0)
    elif kind == "special":      # a few NaN, +inf and -inf entries among normal ones
        c = (100.0 + 3.0 * lam * rng.standard_normal((E, N))).astype(F32)
        if N >= 8:
            idx = rng.choice(N, 6, replace=False)
            c[0, idx[0]], c[-1, idx[1]] = np.nan, np.nan
            c[0, idx[2]], c[-1, idx[3]] = np.inf, np.inf
            c[0, idx[4]], c[-1, idx[5]] = -np.inf, -np.inf
        else:
            c[0, 0] = np.nan if N > 1 else c[0, 0]
    elif kind == "allnan":
        c = np.full((E, N), np.nan, F32)
    else:
        raise ValueError(kind)
    return c


# (N, a, H, E, update_sigma, alpha, costs, lambda): every value of each axis, the corners, every cost
# distribution and temperature; a = 30 and 50 take the kernel's 16- and 8-chunk tiles
UPDATE_CASES = [
    (1, 1, 1, 1, False, 0.0, "normal", 1.0),
    (1, 21, 7, 5, True, 0.0, "normal", 1e6),
    (1, 1, 1, 1, True, 0.1, "allnan", 1.0),
    (31, 6, 7, 5, True, 0.1, "normal", 1.0),
    (33, 21, 1, 1, True, 0.0, "equal", 1.0),
    (33, 6, 1, 5, True, 0.1, "dupmin", 1e-6),
    (1000, 6, 7, 1, False, 0.1, "normal", 1e-6),
    (1000, 6, 1, 1, True, 0.1, "allnan", 1.0),
    (1024, 1, 1, 5, True, 0.1, "spread", 1.0),
    (1025, 6, 7, 1, True, 0.0, "dupmin", 1.0),
    (1025, 1, 7, 1, False, 0.0, "equal", 1e6),
    (4094, 21, 1, 5, True, 0.1, "special", 1.0),
    (4094, 6, 7, 5, True, 0.0, "spread", 1e6),
    (16381, 6, 7, 1, True, 0.1, "normal", 1e6),
    (16381, 21, 1, 1, False, 0.1, "special", 1.0),
    (32768, 21, 7, 5, True, 0.1, "normal", 1.0),
    (32768, 21, 7, 5, False, 0.0, "special", 1e-6),
    (1500, 30, 2, 1, True, 0.1, "normal", 1.0),
    (1500, 50, 2, 5, True, 0.0, "special", 1.0),
]


def _run_update(c, A, mu, sg, lam, alpha, upd, it=0, seed=11, next_shape=None, off=0):
    from mbrl_amd import fused
    dev = torch.device("cuda", 0)
    H, N, a = A.shape
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    costs, acts, mu_d, sg_d = t(c), t(A), t(mu), t(sg)
    mu_o, sg_o = torch.full_like(mu_d, 7.0), torch.full_like(sg_d, 7.0)
    w = torch.full((N,), -1.0, dtype=torch.float32, device=dev)
    r = torch.full((N,), -1.0, dtype=torch.float32, device=dev)
    st = torch.full((2,), -1.0, dtype=torch.float32, device=dev)
    nxt = torch.empty(next_shape, dtype=torch.float32, device=dev) if next_shape else None
    sp = fused.make_sampler(seed, it, mu_d, sg_d, LO, HI)
    fused.mppi_update(costs, acts, sp, H, a, lam, alpha, upd, mu_o, sg_o, weights_out=w, returns_out=r, stats_out=st,
                      next_actions=nxt, draw_offset=off)
    torch.cuda.synchronize()
    out = dict(mu=mu_o.cpu().numpy(), sigma=sg_o.cpu().numpy(), weights=w.cpu().numpy(), returns=r.cpu().numpy(),
               stats=st.cpu().numpy())
    if nxt is not None:
        out["next"] = nxt
        out["mu_d"], out["sg_d"] = mu_o, sg_o
    return out


def _ulp_dist(x, y):
    """Distance in float32 steps between non-negative arrays."""
    return np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64))


def _check_update(got, ref, N, mu, sg, upd, tag):
    """The issue's asserts for one update; prints the measured figures before asserting."""
    assert np.array_equal(got["returns"], ref["returns"], equal_nan=True), tag
    assert np.array_equal(got["stats"][:1], np.array([ref["beta"]], F32), equal_nan=True), tag
    if ref["unchanged"]:
        assert got["mu"].tobytes() == mu.tobytes() and got["sigma"].tobytes() == sg.tobytes(), tag
        assert not got["weights"].any() and got["stats"][1] == 0.0, tag
        return 0.0, 0.0
    wref = ref["weights"].astype(F32)
    ulp = int(_ulp_dist(got["weights"], wref).max())
    eta_err = abs(float(got["stats"][1]) - ref["eta"]) / ref["eta"]
    mu_err = float(np.max(np.abs(got["mu"].astype(np.float64) - ref["mu"]))) / mref.mu_bound(N, LO, HI)
    var_err = 0.0
    if upd:
        var_err = float(np.max(np.abs(got["sigma"].astype(np.float64) ** 2 - ref["var"]))) / mref.var_bound(N, LO, HI)
    print(f"mppi-err {tag}: weights {ulp} ulp, eta rel {eta_err:.3g}, mu {mu_err:.4f} of bound, "
          f"var {var_err:.4f} of bound (D = {mref.chain_depth(N)})")
    assert ulp <= 2, tag
    assert got["weights"].max() == 1.0 and got["stats"][1] >= 1.0, tag
    assert mu_err <= 1.0, (tag, mu_err)
    if upd:
        assert var_err <= 1.0, (tag, var_err)
    else:
        assert got["sigma"].tobytes() == sg.tobytes(), tag
    return mu_err, var_err


@pytest.mark.parametrize("N,a,H,E,upd,alpha,kind,lam", UPDATE_CASES)
def test_update_kernel_against_the_reference(N, a, H, E, upd, alpha, kind, lam):
    rng = np.random.default_rng(N * 131 + a * 17 + H + E)
    c = _costs(kind, E, N, lam, rng)
    A = np.clip(rng.normal(0.1, 0.6, (H, N, a)), LO, HI).astype(F32)
    mu = rng.uniform(-0.3, 0.3, (H, a)).astype(F32)
    sg = rng.uniform(0.05, 0.6, (H, a)).astype(F32)
    got = _run_update(c, A, mu, sg, lam, alpha, upd)
    ref = mref.update(c, A, mu, sg, lam, alpha, upd)
    _check_update(got, ref, N, mu, sg, upd, f"N={N} a={a} H={H} E={E} upd={int(upd)} alpha={alpha} {kind} lam={lam:g}")
    again = _run_update(c, A, mu, sg, lam, alpha, upd)
    for k in ("mu", "sigma", "weights", "returns", "stats"):
        assert got[k].tobytes() == again[k].tobytes(), k


def test_next_proposals_equal_sample_actions():
    """A draw range that the slices do not divide evenly: bit-equal to mbrl_sample_actions from the
    returned mu_out / sigma_out."""
    from mbrl_amd import fused
    rng = np.random.default_rng(3)
    N, H, a, off, cnt, it, seed = 1000, 7, 6, 37, 901, 2, 0x1234567890ABCDEF
    c = _costs("normal", 1, N, 1.0, rng)
    A = np.clip(rng.normal(0.0, 0.6, (H, N, a)), LO, HI).astype(F32)
    mu, sg = rng.uniform(-0.3, 0.3, (H, a)).astype(F32), rng.uniform(0.05, 0.6, (H, a)).astype(F32)
    got = _run_update(c, A, mu, sg, 1.0, 0.1, True, it=it, seed=seed, next_shape=(H, cnt, a), off=off)
    want = torch.empty_like(got["next"])
    fused.sample_actions(fused.make_sampler(seed, it + 1, got["mu_d"], got["sg_d"], LO, HI), H, a, cnt, off, want)
    torch.cuda.synchronize()
    assert torch.equal(got["next"], want)
    ref = cem_actions(got["mu"], got["sigma"], LO, HI, seed, it + 1, off + np.arange(cnt))
    assert np.array_equal(want.cpu().numpy(), ref)
    plain = _run_update(c, A, mu, sg, 1.0, 0.1, True, it=it, seed=seed)     # the draw changes no other output
    assert plain["mu"].tobytes() == got["mu"].tobytes() and plain["sigma"].tobytes() == got["sigma"].tobytes()


def test_range_limit_is_unsupported():
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    N, H, a = 32769, 1, 1
    costs = torch.zeros((1, N), device=dev)
    acts = torch.zeros((H, N, a), device=dev)
    mu, sg = torch.zeros((H, a), device=dev), torch.ones((H, a), device=dev)
    sp = fused.make_sampler(1, 0, mu, sg, LO, HI)
    rc = lib.mbrl_mppi_update(_lib.ptr(costs), 1, N, _lib.ptr(acts), ctypes.byref(sp), H, a, 1.0, 0.0, 0,
                              _lib.ptr(torch.empty_like(mu)), _lib.ptr(torch.empty_like(sg)), None, None, None, None,
                              0, 0, _lib.stream_handle(dev))
    assert rc == _lib.MBRL_EUNSUPPORTED


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


@pytest.mark.parametrize("cid,N,H,I,upd,alpha", [(3, 1000, 5, 3, True, 0.1), (5, 256, 4, 2, False, 0.0),
                                                  (6, 256, 4, 2, True, 0.0)])
def test_plan_iterations_from_the_gpus_own_records(cid, N, H, I, upd, alpha):
    from mbrl_amd import fused
    p = ocem.synth_problem(cid, N=N, H=H)
    a, lam = p["cfg"]["a"], 2.0
    res = _plan(p, H, num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=upd)
    torch.cuda.synchronize()
    mu_h, sg_h = res["mu_hist"].cpu().numpy(), res["sigma_hist"].cpu().numpy()
    assert mu_h.shape == (I + 1, H, a) and not mu_h[0].any() and np.all(sg_h[0] == F32(0.5))
    dev = res["mu_hist"].device
    for i in range(I):
        A = cem_actions(mu_h[i], sg_h[i], LO, HI, p["rng_seed"], i, np.arange(N))
        drawn = torch.empty((H, N, a), dtype=torch.float32, device=dev)
        fused.sample_actions(fused.make_sampler(p["rng_seed"], i, res["mu_hist"][i].contiguous(),
                                                res["sigma_hist"][i].contiguous(), LO, HI), H, a, N, 0, drawn)
        assert np.array_equal(drawn.cpu().numpy(), A), i
        got_c = res["costs"][i].cpu().numpy()
        ref_c = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A)
        err = float(np.max(np.abs(got_c - ref_c) / np.maximum(np.abs(ref_c), 1.0)))
        print(f"mppi-plan cid={cid} it={i}: cost rel err {err:.3g}")
        assert err < 1e-5, (i, err)
        ref = mref.update(got_c, A, mu_h[i], sg_h[i], lam, alpha, upd)
        got = dict(mu=mu_h[i + 1], sigma=sg_h[i + 1], weights=res["weights"][i].cpu().numpy(), returns=ref["returns"],
                   stats=np.array([ref["beta"], ref["eta"]], F32))
        _check_update(got, ref, N, mu_h[i], sg_h[i], upd, f"plan cid={cid} it={i}")
    assert torch.equal(res["mu"], res["mu_hist"][I]) and torch.equal(res["sigma"], res["sigma_hist"][I])
    assert torch.equal(res["actions"], res["mu"].clamp(LO, HI))
    _, states = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], res["actions"].cpu().numpy()[:, None, :],
                             store_states=True)
    ref_s = np.mean(states[:, :, 0, :], axis=0, dtype=F32) if len(p["model"]) > 1 else states[0, :, 0, :]
    got_s = res["states"].cpu().numpy()
    assert float(np.max(np.abs(got_s - ref_s) / np.maximum(np.abs(ref_s), 1.0))) < 1e-5


# N ceil(a / 4) above the fused draw's 65536 limit (the rollout draws), and below it (the update draws)
@pytest.mark.parametrize("cid,N,H,I,over", [(5, 32768, 2, 1, dict(E=1)), (3, 1000, 5, 3, {}), (5, 300, 3, 2, {})])
def test_plan_equals_its_step_by_step_equivalent(cid, N, H, I, over):
    from mbrl_amd import fused
    p = ocem.synth_problem(cid, N=N, H=H, **over)
    a, lam, alpha = p["cfg"]["a"], 1.5, 0.1
    res = _plan(p, H, num_candidates=N, num_iterations=I, temperature=lam, alpha=alpha, update_sigma=True)
    _, model_fn, cost_fn, _ = build(p)
    dev = res["mu"].device
    _, _, prob = fused.describe_problem(model_fn, cost_fn, dev, 0)
    s0 = torch.from_numpy(p["s0"]).to(dev)
    mu = torch.zeros((H, a), dtype=torch.float32, device=dev)
    sg = torch.full((H, a), 0.5, dtype=torch.float32, device=dev)
    acts = torch.empty((H, N, a), dtype=torch.float32, device=dev)
    for it in range(I):
        sp = fused.make_sampler(p["rng_seed"], it, mu, sg, LO, HI)
        fused.sample_actions(sp, H, a, N, 0, acts)
        costs = fused.rollout(prob, s0, N, H, actions=acts)
        assert torch.equal(costs, res["costs"][it]), it
        mu_n, sg_n = torch.empty_like(mu), torch.empty_like(sg)
        fused.mppi_update(costs, acts, sp, H, a, lam, alpha, True, mu_n, sg_n)
        mu, sg = mu_n, sg_n
        assert torch.equal(mu, res["mu_hist"][it + 1]) and torch.equal(sg, res["sigma_hist"][it + 1]), it
    actions = mu.clamp(LO, HI).contiguous()
    states = fused.trajectory(prob, s0, actions, H)
    torch.cuda.synchronize()
    assert torch.equal(mu, res["mu"]) and torch.equal(sg, res["sigma"])
    assert torch.equal(actions, res["actions"]) and torch.equal(states, res["states"])


def test_warm_start_rows_become_the_initial_mean():
    p = ocem.synth_problem(3, N=512, H=5)
    rng = np.random.default_rng(9)
    rows = rng.uniform(-1.4, 1.4, (5, 6)).astype(F32)           # some outside the bounds
    clipped = np.clip(rows, F32(LO), F32(HI))
    warm = _plan(p, 5, rows=rows, num_candidates=512, num_iterations=2, temperature=1.0)
    assert np.array_equal(warm["mu_hist"][0].cpu().numpy(), clipped)
    same = _plan(p, 5, rows=clipped, num_candidates=512, num_iterations=2, temperature=1.0)
    for k in ("mu", "sigma", "actions", "states", "costs", "weights", "mu_hist", "sigma_hist"):
        assert torch.equal(warm[k], same[k]), k
    # iteration 0's proposals are drawn around those rows (the fused first launch)
    A = cem_actions(clipped, np.full((5, 6), 0.5, F32), LO, HI, p["rng_seed"], 0, np.arange(512))
    ref_c = ocem.rollout(p["model"], p["norm"], p["cost"], p["s0"], A)
    got_c = warm["costs"][0].cpu().numpy()
    assert float(np.max(np.abs(got_c - ref_c) / np.maximum(np.abs(ref_c), 1.0))) < 1e-5
    cold = _plan(p, 5, num_candidates=512, num_iterations=2, temperature=1.0)
    assert not cold["mu_hist"][0].any() and not torch.equal(cold["mu"], warm["mu"])


def test_mpc_policy_warm_starts_from_the_shifted_previous_plan():
    from mbrl_amd import MPCPolicy, MPPIPlanner
    p = ocem.synth_problem(3, N=256, H=6)
    _, model_fn, cost_fn, sample_action = build(p)
    seen = []

    class Recording(MPPIPlanner):
        @staticmethod
        def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
            res = MPPIPlanner.plan_detailed(initial_state, model, cost, sample_action, horizon, initial_trajectory,
                                            record=True, **kwargs)
            seen.append(res)
            return res["states"], res["actions"]

    pol = MPCPolicy(model_fn, cost_fn, Recording, sample_action, 6, num_candidates=256, num_iterations=1,
                    temperature=1.0, seed=5)
    obs = torch.from_numpy(p["s0"])
    a0 = pol.get_action({"timestep": 0, "observation": obs})
    a1 = pol.get_action({"timestep": 1, "observation": seen[0]["states"][0]})
    first = seen[0]["actions"].numpy()
    assert np.array_equal(a0.numpy(), first[0]) and a1.shape == (6,)
    assert not seen[0]["mu_hist"][0].cpu().numpy().any()
    want = np.concatenate([first[1:], first[-1:]], 0)
    assert np.array_equal(seen[1]["mu_hist"][0].cpu().numpy(), want)
    pol.get_action({"timestep": 0, "observation": obs})          # a new episode forgets the plan
    assert not seen[2]["mu_hist"][0].cpu().numpy().any()


def test_generic_path_matches_the_fused_path():
    """A closure recognition rejects runs the callables on device tensors and the same HIP update. The
    two paths' costs may differ by the project's 1e-5 relative bar, i.e. by up to 1e-5 |J| / lambda in
    the exponent; the temperature is set so that this stays under one float32 unit roundoff
    (lambda >= 1e-5 |J| 2^24, |J| < 60 here), and the means then agree within the update bound."""
    from mbrl_amd import MPPIPlanner, fused
    N, H, lam = 400, 4, 1.0e4
    p = ocem.synth_problem(3, N=N, H=H)
    module, model_fn, cost_fn, sample_action = build(p)
    wrapped = lambda s, a: model_fn(s, a)  # noqa: E731
    assert fused.describe_model(wrapped) is None
    kw = dict(num_candidates=N, num_iterations=1, temperature=lam, update_sigma=True, seed=p["rng_seed"], record=True,
              return_device=True)
    s0 = torch.from_numpy(p["s0"])
    fz = MPPIPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, **kw)
    gn = MPPIPlanner.plan_detailed(s0, wrapped, cost_fn, sample_action, H, **kw)
    torch.cuda.synchronize()
    cf, cg = fz["costs"][0].cpu().numpy(), gn["costs"][0].cpu().numpy()
    rel = float(np.max(np.abs(cf - cg) / np.maximum(np.abs(cf), 1.0)))
    assert np.abs(cf).max() < 60.0
    assert torch.equal(fz["mu_hist"][0], gn["mu_hist"][0])
    dmu = float(np.max(np.abs(fz["mu"].cpu().numpy().astype(np.float64) - gn["mu"].cpu().numpy())))
    print(f"mppi-generic: cost rel diff {rel:.3g}, mu diff {dmu / mref.mu_bound(N, LO, HI):.4f} of bound")
    assert rel < 1e-5
    assert dmu <= mref.mu_bound(N, LO, HI)
    # each path's update against the reference on its own costs and the shared proposals
    A = cem_actions(np.zeros((H, 6), F32), np.full((H, 6), 0.5, F32), LO, HI, p["rng_seed"], 0, np.arange(N))
    for tag, res, c in (("fused", fz, cf), ("generic", gn, cg)):
        ref = mref.update(c, A, np.zeros((H, 6), F32), np.full((H, 6), 0.5, F32), lam, 0.0, True)
        got = dict(mu=res["mu"].cpu().numpy(), sigma=res["sigma"].cpu().numpy(), weights=res["weights"][0].cpu().numpy(),
                   returns=ref["returns"], stats=np.array([ref["beta"], ref["eta"]], F32))
        _check_update(got, ref, N, None, None, True, tag)
    assert gn["states"].shape == fz["states"].shape == (H, 17)


def test_distributed_is_not_implemented():
    from mbrl_amd import MPPIPlanner
    p = ocem.synth_problem(3, N=64, H=3)
    _, model_fn, cost_fn, sample_action = build(p)
    with pytest.raises(NotImplementedError):
        MPPIPlanner.plan(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, 3, distributed=True)
