"""GPU: trajectory-sampling rollouts (csrc/rollout_ts.hip: mbrl_rollout_cost_ts, mbrl_cem_plan_ts) and
CEMPlanner(particles=P) on top of them.

Accuracy: over tests/rollout_ts_reference.py's two tables (the ten cases and the envelope), states_out and costs
against the float64 restatement at the project's bar -- the tensor-relative error within 8 x max(the float32 CPU
chain's error on that tensor, the first table's median of it). Everything else is equality byte for byte: against mbrl_eval_members_open_loop without
noise, across N, tile positions, neighbours, members, particle counts, NULL outputs and prior output bytes, and
the whole plan against its step-by-step equivalent. measure_all() returns what profiles/rollout_ts/errors.json
holds."""
import collections
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import rollout_ts_reference as ref
from test_gpu_holdout import _filled
from test_gpu_train_ensemble import DEV, _Data, _dataset, _offset_like, _P

pytestmark = pytest.mark.gpu
NAN = float("nan")
EINVAL, EUNSUPPORTED = -1, -2


class _Null:
    """A missing array: its pointer is NULL."""

    def data_ptr(self):
        return None


def _t(x):
    if x is None:
        return _Null()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)


@functools.lru_cache(maxsize=None)
def device_members(name):
    """Per member the device tensors (w0, b0, w1, ..) of the case, the listed members 4 bytes off alignment."""
    c, p = ref.case(name), ref.problem(name)
    out = []
    for e, layers in enumerate(p["members"]):
        params = [_t(x) for wb in layers for x in wb]
        if e in c.offset:
            params = [_offset_like(t) for t in params]
        assert all((t.data_ptr() % 16 == 4) == (e in c.offset) for t in params)
        out.append(params)
    return out


def _table(members, s, a, W, L):
    from mbrl_amd import _lib
    tms = (_lib.TrainModel * len(members))()
    for tm, params in zip(tms, members):
        tm.state_dim, tm.action_dim, tm.hidden, tm.n_hidden, tm.reward_head, tm.horizon = s, a, W, L, 0, 1
        for i in range(len(params) // 2):
            tm.weight[i], tm.bias[i] = params[2 * i].data_ptr(), params[2 * i + 1].data_ptr()
    return tms


def _norm_struct(norm, keep):
    from mbrl_amd import _lib
    if norm is None:
        return None
    ts = [_t(norm[k]) for k in ("obs_mean", "obs_std", "act_mean", "act_std")]
    keep += ts
    return _lib.Norm(*[t.data_ptr() for t in ts], None, None, int(norm["normalize_state"]),
                     int(norm["unnormalize_state"]), int(norm["normalize_action"]), 0)


def _cost_struct(cost, keep):
    from mbrl_amd import _lib
    w, g = _t(cost["weights"]), _t(cost["goal"])
    keep += [w, g]
    return _lib.Cost(_lib.MBRL_COST_GOAL_STATE, int(cost["has_state"]), int(cost["has_action"]), 0, w.data_ptr(),
                     g.data_ptr(), cost["alpha_state"], cost["alpha_action"])


def run_ts(name, members=None, with_states=True, fill="nan", raw=False, **override):
    """mbrl_rollout_cost_ts on the case (fields of its problem replaced by `override`; members: device tensors
    instead of the case's): dict(states [Q][H][N][s] or None, costs [Q][N]) as NumPy. raw: (rc, states, costs) as
    device tensors instead, whatever rc is."""
    from mbrl_amd import _lib
    lib = _lib.load()
    c, p = ref.case(name), dict(ref.problem(name), **override)
    members = device_members(name) if members is None else members
    E, P = len(members), p["P"]
    H, N = p["actions"].shape[:2]
    keep = []
    lo, hi = _t(p["bounds"][0]), _t(p["bounds"][1])
    bounds = _lib.NllBounds(lo.data_ptr(), hi.data_ptr())
    norm, cost = _norm_struct(p["norm"], keep), _cost_struct(p["cost"], keep)
    s0, actions = _t(p["s0"]), _t(p["actions"])
    ts = _lib.TsParams(P, p["iteration"], p["noise_seed"], p["noise_scale"])
    Q = max(E * P, 1)
    states = _filled((Q, H, N, c.s), fill) if with_states else None
    costs = _filled((Q, N), fill)
    rc = lib.mbrl_rollout_cost_ts(_table(members, c.s, c.a, c.W, c.L), E, ctypes.byref(bounds),
                                  None if norm is None else ctypes.byref(norm),
                                  None if p.get("cost_null") else ctypes.byref(cost), _P(s0), int(np.ndim(p["s0"]) == 2),
                                  _P(actions), N, H, ctypes.c_int32(p["n_offset"]), ctypes.byref(ts), _P(costs),
                                  None if states is None else _P(states), _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    if raw:
        return rc, states, costs
    _lib.check(rc, "mbrl_rollout_cost_ts")
    return dict(states=None if states is None else states.cpu().numpy(), costs=costs.cpu().numpy())


@functools.lru_cache(maxsize=None)
def default_run(name):
    return run_ts(name)


def _same(x, y):
    return all((x[k] is None or y[k] is None or x[k].tobytes() == y[k].tobytes()) for k in ref.KINDS)


def _shares(name):
    got = default_run(name)
    assert all(np.all(np.isfinite(v)) for v in got.values()), name
    e, bar = ref.errors(name, got), ref.bars(name)
    return {k: (e[k], ref.e32(name)[k], bar[k]) for k in ref.KINDS}


def measure_all():
    """Per case of both tables and tensor: e(gpu), the float32 CPU chain's e32, the bar and e(gpu) / bar; and the
    largest share of the first table and of the envelope."""
    out = {n: {k: dict(e_gpu=v[0], e32=v[1], bar=v[2], share=v[0] / v[2] if v[2] else 0.0) for k, v in _shares(n).items()}
           for n in ref.ALL_NAMES}
    out["largest_share_of_the_bar"] = max(t["share"] for n in ref.NAMES for t in out[n].values())
    out["largest_envelope_share_of_the_bar"] = max(t["share"] for n in ref.ENV_NAMES for t in out[n].values())
    return out


@pytest.mark.parametrize("name", ref.ALL_NAMES)
def test_rollout_ts_matches_float64(name):
    failures = []
    for k, (e, own, bar) in _shares(name).items():
        print(f"RATIO {name} {k}: e(gpu) {e:.3e}, e32 {own:.3e}, bar {bar:.3e}")
        if not e <= bar:
            failures.append(f"{k}: e(gpu) = {e:.3e} > bar = {bar:.3e}")
    assert not failures, f"{name}: " + "; ".join(failures)


@pytest.mark.parametrize("name", ["seam", "seam_l3_e5"])
def test_without_noise_the_states_are_the_open_loop_evaluations(name):
    """noise_scale = 0, norm == NULL, s0 per candidate: states_out[e P + p][t][n] is mbrl_eval_members_open_loop's
    pred_out[e][n][t] on a dataset of the same start states and actions (the head's mean rows bound as a head of s
    rows at the same pointers), and the P rows of a member are equal."""
    from mbrl_amd import _lib
    lib = _lib.load()
    c, p = ref.CASES[name], ref.problem(name)
    got = default_run(name)["states"]
    states = np.zeros((c.N, c.H, c.s), np.float32)
    states[:, 0] = p["s0"]
    actions = np.ascontiguousarray(p["actions"].transpose(1, 0, 2))           # [N][H][a], in that memory order
    data = _Data(c.s, c.a, c.H, c.N, 0, arrays=dict(states=states, actions=actions, next_states=np.zeros_like(states),
                                                    rewards=np.zeros((c.N, c.H))))
    tms = _table(device_members(name), c.s, c.a, c.W, c.L)
    for tm in tms:
        tm.horizon = c.H
    rows = torch.arange(c.N, device=DEV)
    row_err, pred = _filled((c.E, c.N, c.H), "nan"), _filled((c.E, c.N, c.H, c.s), "nan")
    _lib.check(lib.mbrl_eval_members_open_loop(tms, c.E, ctypes.byref(data.c), _P(rows), c.N, _P(row_err), None, _P(pred),
                                               None, _lib.stream_handle(DEV)), "mbrl_eval_members_open_loop")
    torch.cuda.synchronize()
    want = pred.cpu().numpy().transpose(0, 2, 1, 3)                  # [E][H][N][s]
    for q in range(c.E * c.P):
        assert got[q].tobytes() == np.ascontiguousarray(want[q // c.P]).tobytes(), q


BIG = "n40_e5p4_state"      # N = 40 (three tiles, the last one partial), E = 5, P = 4, s0 per candidate, H = 4


def _slice(name, lo, hi):
    p = ref.problem(name)
    if np.ndim(p["s0"]) == 1:
        return dict(actions=np.ascontiguousarray(p["actions"][:, lo:hi]), n_offset=p["n_offset"] + lo)
    return dict(s0=p["s0"][lo:hi], actions=np.ascontiguousarray(p["actions"][:, lo:hi]), n_offset=p["n_offset"] + lo)


_SLICES = [(BIG, 0, 17), (BIG, 16, 40), (BIG, 23, 24), (BIG, 5, 40), (BIG, 39, 40), ("e8p32", 5, 17), ("e1p256", 16, 17),
           ("s632_n17", 3, 17), ("a48", 0, 16), ("key_n_offset", 8, 17)]


@pytest.mark.parametrize("name, lo, hi", _SLICES,
                         ids=[f"{lo}-{hi}" if n == BIG else f"{n}-{lo}-{hi}" for n, lo, hi in _SLICES])
def test_a_candidate_does_not_depend_on_n_or_its_tile_position(name, lo, hi):
    """Candidates [lo, hi) alone, with n_offset = lo, are the full call's columns: another N, another position in
    the tile, other neighbours; n_offset = k on [k, N) is the tail of the full call (key_n_offset: past 2^31)."""
    full, part = default_run(name), run_ts(name, **_slice(name, lo, hi))
    assert part["states"].tobytes() == np.ascontiguousarray(full["states"][:, :, lo:hi]).tobytes()
    assert part["costs"].tobytes() == np.ascontiguousarray(full["costs"][:, lo:hi]).tobytes()


def test_a_non_finite_neighbour_changes_nothing_else():
    p = ref.problem(BIG)
    s0 = p["s0"].copy()
    s0[22], s0[33, 1] = NAN, np.inf
    got, full = run_ts(BIG, s0=s0), default_run(BIG)
    others = [n for n in range(40) if n not in (22, 33)]
    assert np.all(np.isnan(got["states"][:, :, 22])) and np.all(np.isnan(got["costs"][:, 22]))
    for k in ref.KINDS:
        assert np.ascontiguousarray(got[k][..., others, :] if k == "states" else got[k][:, others]).tobytes() == \
            np.ascontiguousarray(full[k][..., others, :] if k == "states" else full[k][:, others]).tobytes(), k


def test_a_member_does_not_depend_on_the_other_members():
    c, mems = ref.CASES[BIG], device_members(BIG)
    poisoned = [params if e == 3 else [torch.full_like(t, NAN) for t in params] for e, params in enumerate(mems)]
    got, full = run_ts(BIG, members=poisoned), default_run(BIG)
    rows = slice(3 * c.P, 4 * c.P)
    assert all(got[k][rows].tobytes() == full[k][rows].tobytes() for k in ref.KINDS)
    assert np.all(np.isnan(got["costs"][:3 * c.P]))


def test_a_row_depends_on_its_index_and_member_not_on_the_particle_count():
    """Rows 0 .. 5 of (m0, m0) at P = 3 are rows 0 .. 5 of (m0) at P = 6: the same q on the same member."""
    name = "n17_e2p3"
    m0 = device_members(name)[0]
    two, one = run_ts(name, members=[m0, m0], P=3), run_ts(name, members=[m0], P=6)
    assert _same(two, one)
    # a different q, iteration or noise_seed changes the states
    assert two["states"][0].tobytes() != two["states"][3].tobytes() != two["states"][1].tobytes()
    p = ref.problem(name)
    base = default_run(name)
    for change in (dict(iteration=p["iteration"] + 1), dict(noise_seed=p["noise_seed"] + 1)):
        other = run_ts(name, **change)
        assert all(other["states"][q].tobytes() != base["states"][q].tobytes() for q in range(6)), change


@pytest.mark.parametrize("name", [BIG, "n1_s33_null", "w1024", "no_cost_half_noise", "e8p32", "e1p256", "s632_n17", "a48",
                                  "a1023"])
def test_prior_output_bytes_and_a_null_states_out_never_matter(name):
    base = default_run(name)
    assert all(np.all(np.isfinite(v)) for v in base.values())          # NaN-filled outputs were fully written
    assert _same(base, run_ts(name, fill="ff")) and _same(base, run_ts(name))
    assert base["costs"].tobytes() == run_ts(name, with_states=False)["costs"].tobytes()


def test_a_null_cost_is_zero_cost_and_the_states_of_both_flags_off():
    got, flags_off = default_run("cost_null"), run_ts("cost_null", cost_null=False)
    assert got["costs"].tobytes() == np.zeros_like(got["costs"]).tobytes()       # exactly +0.0
    assert _same(got, flags_off) and np.all(np.isfinite(got["states"]))


def _bad_calls():
    p = ref.problem("n17_e2p3")
    norm = dict(p["norm"])
    yield "particles < 1", EINVAL, dict(P=0)
    yield "rows above MBRL_TS_MAX_ROWS", EINVAL, dict(P=129)
    yield "negative noise_scale", EINVAL, dict(noise_scale=-1.0)
    yield "NaN noise_scale", EINVAL, dict(noise_scale=NAN)
    yield "infinite noise_scale", EINVAL, dict(noise_scale=float("inf"))
    yield "iteration 2^24", EINVAL, dict(iteration=1 << 24)
    yield "negative iteration", EINVAL, dict(iteration=-1)
    yield "negative n_offset", EINVAL, dict(n_offset=-1)
    yield "state cost without weights", EINVAL, dict(cost=dict(p["cost"], weights=None))
    yield "normaliser without statistics", EINVAL, dict(norm=dict(norm, obs_mean=None))
    yield "action normaliser without statistics", EINVAL, dict(norm=dict(norm, act_std=None))


@pytest.mark.parametrize("label, code, change", list(_bad_calls()), ids=[b[0] for b in _bad_calls()])
def test_argument_errors_return_their_code_and_leave_the_outputs_untouched(label, code, change):
    rc, states, costs = run_ts("n17_e2p3", raw=True, **change)
    assert rc == code, (label, rc)
    assert bool(torch.isnan(states).all()) and bool(torch.isnan(costs).all())


def test_struct_level_argument_errors():
    """The errors run_ts cannot express: NULL pointers, E, the members' shape, the cost kind, the LDS envelope."""
    from mbrl_amd import _lib
    lib = _lib.load()
    name = "n17_e2p3"
    c, p = ref.CASES[name], ref.problem(name)
    mems = device_members(name)
    keep = []
    lo, hi = _t(p["bounds"][0]), _t(p["bounds"][1])
    s0, actions = _t(p["s0"]), _t(p["actions"])
    states, costs = _filled((6, c.H, c.N, c.s), "nan"), _filled((6, c.N), "nan")
    st = _lib.stream_handle(DEV)

    def call(tms=None, E=2, bounds=(lo, hi), cost_kind=0, s0_=s0, actions_=actions, ts=(3, 0, 1, 1.0), costs_=costs, N=c.N,
             H=c.H):
        tms = _table(mems, c.s, c.a, c.W, c.L) if tms is None else tms
        b = None if bounds is None else _lib.NllBounds(*[None if t is None else t.data_ptr() for t in bounds])
        cost = _cost_struct(p["cost"], keep)
        cost.kind = cost_kind
        tsp = None if ts is None else _lib.TsParams(*ts)
        opt = lambda t: None if t is None else _P(t)   # noqa: E731
        return lib.mbrl_rollout_cost_ts(tms, E, None if b is None else ctypes.byref(b), None, ctypes.byref(cost), opt(s0_), 0,
                                        opt(actions_), N, H, 0, None if tsp is None else ctypes.byref(tsp), opt(costs_),
                                        _P(states), st)
    assert call() == 0
    torch.cuda.synchronize()
    states.fill_(NAN), costs.fill_(NAN)
    reward = _table(mems, c.s, c.a, c.W, c.L)
    reward[0].reward_head = reward[1].reward_head = 1
    differs = _table(mems, c.s, c.a, c.W, c.L)
    differs[1].hidden = c.W + 1
    no_action = _table(mems, c.s + c.a, 0, c.W, c.L)
    null_layer = _table(mems, c.s, c.a, c.W, c.L)
    null_layer[1].bias[c.L] = None
    wide = _table(mems, 640, c.a, c.W, c.L)                      # 2 s = 1280: 32 x 1284 floats exceed 160 KiB
    # the largest head is s = 632 (the s632 cases run it): 2 x 16 x (1264 + 4) x 4 = 162304 <= 160 KiB = 163840 bytes;
    # s = 633 rounds 2 s = 1266 up to 1280 columns: 2 x 16 x 1284 x 4 = 164352
    s633 = _table(mems, 633, 1, 16, 1)
    deep = _table(mems, c.s, c.a, c.W, 9)                        # n_hidden <= MBRL_TRAIN_MAX_LAYERS - 2 = 8 (case l8)
    for label, rc, want in (
            ("NULL bounds", call(bounds=None), EINVAL), ("NULL bound array", call(bounds=(lo, None)), EINVAL),
            ("NULL s0", call(s0_=None), EINVAL), ("NULL actions", call(actions_=None), EINVAL),
            ("NULL ts", call(ts=None), EINVAL), ("NULL costs", call(costs_=None), EINVAL),
            ("E = 0", call(E=0), EINVAL), ("E above MBRL_TRAIN_MAX_MEMBERS", call(E=9), EINVAL),
            ("N = 0", call(N=0), EINVAL), ("H = 0", call(H=0), EINVAL),
            ("reward head", call(tms=reward), EINVAL), ("member shapes differ", call(tms=differs), EINVAL),
            ("action_dim < 1", call(tms=no_action), EINVAL), ("NULL layer", call(tms=null_layer), EINVAL),
            ("MODEL_REWARD", call(cost_kind=1), EINVAL), ("unknown cost kind", call(cost_kind=7), EUNSUPPORTED),
            ("beyond the LDS envelope", call(tms=wide), EUNSUPPORTED), ("s = 633", call(tms=s633), EUNSUPPORTED),
            ("n_hidden = 9", call(tms=deep), EUNSUPPORTED)):
        assert rc == want, (label, rc, lib.mbrl_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(states).all()) and bool(torch.isnan(costs).all())


# ---- the plan entry and CEMPlanner(particles=P)
LO, HI = -1.0, 1.0


def _prob_ensemble(E, s, a, W, L, seed):
    from mbrl_amd import models
    torch.manual_seed(seed)
    ens = models.EnsembleModel([models.ProbabilisticModel(s, a, hidden_units=W, n_hidden=L, min_logvar=-5.0,
                                                          max_logvar=-1.0) for _ in range(E)]).to(DEV)
    with torch.no_grad():                       # raw log-variances below, between and above the bounds
        for m in ens.members:
            m.linears()[-1].bias[s:] += torch.tensor([-8.0, -3.0, 2.0], device=DEV)[torch.arange(s) % 3]
    return ens


def _closures(ens, s, a, seed=5):
    import functools as ft
    from mbrl_amd import data, env, models
    g = torch.Generator().manual_seed(seed)
    stats = {"observations": {"mean": torch.rand(s, generator=g) - 0.5, "std": torch.rand(s, generator=g) * 1.5 + 0.5},
             "actions": {"mean": torch.rand(a, generator=g) - 0.5, "std": torch.rand(a, generator=g) * 1.5 + 0.5}}
    ds = data.TransitionsDataset.from_statistics(stats)
    model_fn = ft.partial(ens, **ds.normalizers())
    cost_fn = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(s), torch.randn(s, generator=g), 0.4),
                                     models.CoshLoss(0.25))
    return model_fn, cost_fn, env.sample_action_fn(env.BoundedActionSpec(a, LO, HI)), torch.randn(s, generator=g)


_Plan = collections.namedtuple("_Plan", "N H I K E P s a W L pseed unfused", defaults=(2, 2, 5, 12, 33, 2, 123456789, 0))
PLANS = {
    # N ceil(a / 4) below the fused draw's 65536 limit (the update draws the next proposals) and above it (a draw launch)
    "300-3-3": _Plan(300, 3, 3, 30), "30000-2-2": _Plan(30000, 2, 2, 3000),
    # Q = 256 rows through the fused update, and through the selection and the refit
    "q256": _Plan(64, 2, 2, 6, E=8, P=32, s=3, a=17, W=16, L=1),
    "q256_unfused": _Plan(64, 2, 2, 6, E=8, P=32, s=3, a=17, W=16, L=1, unfused=1),
    "k1": _Plan(300, 3, 2, 1, E=3), "k_is_n": _Plan(64, 2, 2, 64, E=3),
    # the plan's deepest trunk: its final trajectory runs on the packed members, which hold four hidden layers
    "l4_w17": _Plan(64, 2, 2, 6, W=17, L=4),
    "seed64": _Plan(64, 2, 2, 6, pseed=ref.SEED64),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_plan_equals_its_step_by_step_equivalent(plan):
    from mbrl_amd import _lib
    with _lib.option("unfused_update", PLANS[plan].unfused):
        _plan_equals_its_step_by_step_equivalent(*PLANS[plan][:-1])


def _plan_equals_its_step_by_step_equivalent(N, H, I, K, E, P, s, a, W, L, pseed):
    from mbrl_amd import CEMPlanner, fused, planners
    alpha, seed = 0.1, 77
    ens = _prob_ensemble(E, s, a, W, L, seed=3)
    model_fn, cost_fn, sample, s0 = _closures(ens, s, a)
    kw = dict(num_candidates=N, num_iterations=I, num_elites=K, seed=seed, particles=P, particle_noise=0.75, device=str(DEV))
    res = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, H, particle_seed=pseed, record=True, return_device=True,
                                   **kw)
    assert res["costs"].shape == (I, E * P, N) and res["returns"].shape == (I, N) and res["elites"].shape == (I, K)
    _, _, prob = fused.describe_problem(model_fn, cost_fn, DEV, 0)
    s0d = s0.to(DEV)
    mu = torch.zeros((H, a), dtype=torch.float32, device=DEV)
    sg = torch.full((H, a), 0.5, dtype=torch.float32, device=DEV)
    acts = torch.empty((H, N, a), dtype=torch.float32, device=DEV)
    for it in range(I):
        sp = fused.make_sampler(seed, it, mu, sg, LO, HI)
        fused.sample_actions(sp, H, a, N, 0, acts)
        costs = fused.rollout_ts(prob, s0d, acts, particles=P, noise_seed=pseed, noise_scale=0.75, iteration=it)
        assert torch.equal(costs, res["costs"][it]), it
        mu_n, sg_n, rets = torch.empty_like(mu), torch.empty_like(sg), torch.empty(N, device=DEV)
        elites = fused.select(costs, K, returns_out=rets)
        fused.refit(sp, H, a, elites, alpha, mu_n, sg_n)
        mu_u, sg_u, rets_u = torch.empty_like(mu), torch.empty_like(sg), torch.empty_like(rets)
        fused_elites = fused.cem_update(costs, K, sp, H, a, alpha, mu_u, sg_u, returns_out=rets_u)
        if fused_elites is not None:             # (None: the shape exceeds the one-launch update)
            assert torch.equal(fused_elites, elites) and torch.equal(rets_u, rets)
            assert torch.equal(mu_u, mu_n) and torch.equal(sg_u, sg_n)
        assert torch.equal(elites, res["elites"][it]) and torch.equal(rets, res["returns"][it]), it
        mu, sg = mu_n, sg_n
    actions = mu.clamp(LO, HI).contiguous()
    states = fused.trajectory(prob, s0d, actions, H)
    torch.cuda.synchronize()
    assert torch.equal(mu, res["mu"]) and torch.equal(sg, res["sigma"])
    assert torch.equal(actions, res["actions"]) and torch.equal(states, res["states"])
    # the derived noise key, and host tensors by default
    auto = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, H, **kw)
    same = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, H, particle_seed=planners._ts_seed(seed), **kw)
    assert not auto["actions"].is_cuda and torch.equal(auto["actions"], same["actions"])
    assert K == N or not torch.equal(auto["mu"].cpu(), res["mu"].cpu())   # (K = N: every candidate is an elite)
    if pseed >> 32:                             # the key's second word reaches the plan's noise
        low = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, H, particle_seed=pseed & 0xFFFFFFFF, record=True, **kw)
        assert not torch.equal(low["costs"][0].cpu(), res["costs"][0].cpu())
        assert not torch.equal(low["mu"].cpu(), res["mu"].cpu())


def test_a_trunk_deeper_than_the_packed_members_is_refused_by_the_plan():
    """mbrl_rollout_cost_ts runs n_hidden = 8 (case l8); the plan also needs the packed members for its final
    trajectory, and those hold at most four hidden layers."""
    from mbrl_amd import CEMPlanner
    ens = _prob_ensemble(2, 5, 12, 17, 8, seed=3)
    model_fn, cost_fn, sample, s0 = _closures(ens, 5, 12)
    with pytest.raises(RuntimeError, match="unsupported MLP shape"):
        CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, 2, num_candidates=64, num_iterations=1, seed=1, particles=2,
                                 device=str(DEV))


_Q6, _Q256 = (5, 12, 3, 2, 300, 3, 30, 33, 2), (3, 17, 8, 32, 64, 2, 6, 16, 1)


@pytest.mark.parametrize("unfused, s, a, E, P, N, H, K, W, L", [(0, *_Q6), (1, *_Q6), (0, *_Q256), (1, *_Q256)],
                         ids=["0", "1", "q256-0", "q256-1"])
def test_the_plan_does_not_depend_on_its_workspaces_prior_bytes(unfused, s, a, E, P, N, H, K, W, L):
    """mbrl_cem_plan_ts with exactly mbrl_cem_ts_workspace_bytes bytes holding zeros, 0xFF and NaNs: every output and
    record the same bytes, with the fused update and with separate select and refit launches."""
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    I = 2
    ens = _prob_ensemble(E, s, a, W, L, seed=6)
    model_fn, cost_fn, _, s0 = _closures(ens, s, a)
    _, _, prob = fused.describe_problem(model_fn, cost_fn, DEV, 0)
    table = fused.ts_members(ens, DEV)
    cem = _lib.CemParams(N, H, K, I, 0.1, LO, HI, 0.0, 0.5, 0, 31)
    tsp = fused.ts_params(P, 0, 17, 1.0)
    s0d = s0.to(DEV)
    runs = []
    with _lib.option("unfused_update", unfused):
        need = lib.mbrl_cem_ts_workspace_bytes(prob.refs[0], ctypes.byref(cem), ctypes.byref(tsp))
        assert need > 0
        for fill in (0x00, 0xFF, "nan"):
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            ws.view(torch.float32)[:need // 4].fill_(NAN) if fill == "nan" else ws.fill_(fill)
            outs = [_filled(sh, "nan") for sh in ((H, a), (H, a), (H, a), (H, s), (I, E * P, N), (I, N))]
            elites = torch.full((I, K), -1, dtype=torch.int64, device=DEV)
            _lib.check(lib.mbrl_cem_plan_ts(prob.refs[0], prob.refs[1], *table.refs, prob.refs[2], prob.refs[3], _P(s0d),
                                            ctypes.byref(cem), ctypes.byref(tsp), *[_P(x) for x in outs], _P(elites), _P(ws),
                                            need, _lib.stream_handle(DEV)), "mbrl_cem_plan_ts")
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(x).all()) for x in outs) and int(elites.min()) >= 0
            runs.append([x.cpu().numpy().tobytes() for x in outs + [elites]])
    assert runs[0] == runs[1] == runs[2]


def test_particles_zero_is_the_plan_without_the_kwarg_and_noise_zero_is_the_mean_plan():
    from mbrl_amd import CEMPlanner
    s, a, H = 5, 12, 3
    ens = _prob_ensemble(2, s, a, 33, 2, seed=4)
    model_fn, cost_fn, sample, s0 = _closures(ens, s, a)
    kw = dict(num_candidates=300, num_iterations=2, seed=9, record=True, device=str(DEV))
    plain = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, H, **kw)
    zero = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, H, particles=0, particle_noise=3.0, particle_seed=1, **kw)
    assert plain.keys() == zero.keys()
    assert all(plain[k].cpu().numpy().tobytes() == zero[k].cpu().numpy().tobytes() for k in plain)
    # without noise every particle is its member's mean rollout: the elites of the deterministic plan, whose
    # returns differ only by the two kernels' rounding
    quiet = CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, H, particles=1, particle_noise=0.0, **kw)
    assert quiet["costs"].shape == plain["costs"].shape
    assert torch.allclose(quiet["costs"][0].cpu(), plain["costs"][0].cpu(), rtol=1e-5, atol=1e-5)


def test_plan_after_train_members_uses_the_new_weights():
    from mbrl_amd import CEMPlanner, env, models
    s, a, W = 6, 2, 48
    ds = _dataset(s, a, 1, 300, seed=8)
    ens = _prob_ensemble(2, s, a, W, 2, seed=1)
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(s), torch.zeros(s), 0.4), models.CoshLoss(0.25))
    sample = env.sample_action_fn(env.BoundedActionSpec(a, LO, HI))
    s0 = torch.linspace(-1, 1, s)

    def plan(module):
        res = CEMPlanner.plan_detailed(s0, module, cost, sample, 5, num_candidates=256, num_iterations=2, seed=3,
                                       particles=3, record=True, device=str(DEV))
        return [res[k].detach().cpu().clone() for k in ("actions", "mu", "sigma", "costs")]
    before = plan(ens)
    ens.train_members(ds, [torch.optim.Adam(m.parameters(), lr=3e-3) for m in ens.members], batch_size=64,
                      num_epochs=3, seed=2, loss="nll")
    after = plan(ens)
    fresh = _prob_ensemble(2, s, a, W, 2, seed=7)
    fresh.load_state_dict(copy.deepcopy(ens.state_dict()))
    want = plan(fresh)
    assert all(torch.equal(x, y) for x, y in zip(after, want))
    assert not any(torch.equal(x, y) for x, y in zip(after, before))


def test_particles_refuse_models_and_callables_the_sampled_plan_cannot_run():
    from mbrl_amd import CEMPlanner, env, models
    s, a = 5, 2
    ens = _prob_ensemble(2, s, a, 33, 2, seed=2)
    model_fn, cost_fn, sample, s0 = _closures(ens, s, a)
    kw = dict(num_candidates=64, num_iterations=1, seed=1, particles=2, device=str(DEV))
    wrapped = lambda st, ac: model_fn(st, ac)  # noqa: E731
    with pytest.raises(NotImplementedError, match="particles=2"):
        CEMPlanner.plan_detailed(s0, wrapped, cost_fn, sample, 3, **kw)
    torch.manual_seed(0)
    plain = models.EnsembleModel([models.Model(s, a, hidden_units=33) for _ in range(2)]).to(DEV)
    with pytest.raises(NotImplementedError, match="particles"):
        CEMPlanner.plan_detailed(s0, plain, cost_fn, sample, 3, **kw)
    with pytest.raises(NotImplementedError, match="particles"):
        CEMPlanner.plan_detailed(s0, ens.members[0], cost_fn, sample, 3, **kw)
    with torch.no_grad():
        ens.members[1].max_logvar += 0.5
    with pytest.raises(NotImplementedError, match="bounds"):
        CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample, 3, **kw)
