"""GPU: sampled rows for the control loop -- mbrl_rollout_cost_ts_rows (the per-step member draw, members_out),
mbrl_cem_plan_ts_rh and its batch (csrc/rollout_ts.hip on plan.hip's receding-horizon loop) and
TrajectorySamplingCEMPlanner on top of them.

Accuracy: the RESAMPLED rollout against tests/ts_rh_reference.py's float64 restatement at rollout_ts_reference's bar,
members_out against its integers exactly. Everything else is equality byte for byte: FIXED against
mbrl_rollout_cost_ts, the independence properties, every plan against its chain -- each iteration's recorded costs
against the rows entry on the restated proposals, and the selections, kept rows and refit against the given-costs
restatement fed those costs. measure_all() returns what profiles/cem_ts_rh/errors.json holds."""
import copy
import ctypes
import itertools

import numpy as np
import pytest
import torch

import rollout_ts_reference as ref
import ts_rh_reference as trh
from test_gpu_holdout import _filled
from test_gpu_rollout_ts import (HI, LO, _closures, _cost_struct, _norm_struct, _prob_ensemble, _t, _table, default_run,
                                 device_members)
from test_gpu_train_ensemble import DEV, _dataset, _offset_like, _P

pytestmark = pytest.mark.gpu
NAN = float("nan")
FIXED, RESAMPLED = 0, 1


def _dev_members(p):
    out = []
    for e, layers in enumerate(p["members"]):
        params = [_t(x) for wb in layers for x in wb]
        out.append([_offset_like(t) for t in params] if e in p["case"].offset else params)
    return out


def run_rows(p, members, mode, particles, with_states=True, with_members=True, fill="nan", raw=False, **override):
    """mbrl_rollout_cost_ts_rows on the problem (fields replaced by `override`): dict(states, costs, members) as
    NumPy; raw: (rc, states, costs, members) as device tensors, whatever rc is."""
    from mbrl_amd import _lib
    lib = _lib.load()
    p = dict(p, **override)
    c = p["case"]
    E = len(members)
    H, N = p["actions"].shape[:2]
    Q = particles if mode == RESAMPLED else E * particles
    Qa = min(max(Q, 1), 512)
    keep = []
    lo, hi = _t(p["bounds"][0]), _t(p["bounds"][1])
    bounds = _lib.NllBounds(lo.data_ptr(), hi.data_ptr())
    norm, cost = _norm_struct(p["norm"], keep), _cost_struct(p["cost"], keep)
    s0, actions = _t(p["s0"]), _t(p["actions"])
    rows = _lib.TsRows(_lib.TsParams(particles, p["iteration"], p["noise_seed"], p["noise_scale"]), mode, 0)
    states = _filled((Qa, H, N, c.s), fill) if with_states else None
    costs = _filled((Qa, N), fill)
    mem = torch.full((Qa, H), -1, dtype=torch.int32, device=DEV) if with_members else None
    rc = lib.mbrl_rollout_cost_ts_rows(_table(members, c.s, c.a, c.W, c.L), E, ctypes.byref(bounds),
                                       None if norm is None else ctypes.byref(norm),
                                       None if p.get("cost_null") else ctypes.byref(cost), _P(s0),
                                       int(np.ndim(p["s0"]) == 2), _P(actions), N, H, ctypes.c_int32(p["n_offset"]),
                                       ctypes.byref(rows), _P(costs), None if states is None else _P(states),
                                       None if mem is None else _P(mem), _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    if raw:
        return rc, states, costs, mem
    _lib.check(rc, "mbrl_rollout_cost_ts_rows")
    return dict(states=None if states is None else states.cpu().numpy(), costs=costs.cpu().numpy(),
                members=None if mem is None else mem.cpu().numpy())


def _same(x, y, kinds=ref.KINDS):
    return all(x[k] is None or y[k] is None or x[k].tobytes() == y[k].tobytes() for k in kinds)


# ---- the rows entry
@pytest.mark.parametrize("name", ["n17_e2p3", "n40_e5p4_state", "n1_s33_null"])
def test_fixed_mode_is_rollout_cost_ts_byte_for_byte(name):
    c = ref.CASES[name]
    got = run_rows(ref.problem(name), device_members(name), FIXED, c.P)
    assert _same(got, default_run(name))
    assert np.array_equal(got["members"], np.repeat((np.arange(c.E * c.P) // c.P)[:, None], c.H, axis=1))


@pytest.mark.parametrize("E", [1, 2, 5, 8])
def test_members_out_is_the_restated_draw_exactly(E):
    for Q, H in itertools.product((1, 3, 7), (1, 4, 9)):
        p = ref._draw(ref._c(5, 2, 16, 1, 3, H, E, 1, iteration=2 + Q, seed=ref.SEED64 + H), 6900 + E)
        got = run_rows(p, _dev_members(p), RESAMPLED, Q, with_states=False)
        want = trh.members(p["noise_seed"], p["iteration"], Q, H, E)
        assert got["members"].dtype == np.int32 and np.array_equal(got["members"], want), (E, Q, H)


_GRID_RUNS = {}


def grid_run(g):
    if g not in _GRID_RUNS:
        p = trh.grid_problem(*g)
        _GRID_RUNS[g] = run_rows(p, _dev_members(p), RESAMPLED, g[2])
    return _GRID_RUNS[g]


def _shares(g):
    got, r64 = grid_run(g), trh.grid_refs(*g)[0]
    assert all(np.all(np.isfinite(got[k])) for k in ref.KINDS), g
    bars, own = trh.grid_bars(*g)
    return {k: (ref.err(got[k], r64[k]), own[k], bars[k]) for k in ref.KINDS}


def measure_all():
    """Per grid point and tensor: e(gpu), the float32 CPU chain's e32, the bar and e(gpu) / bar; and the worst ratio."""
    out = {"N%d_E%d_Q%d" % g: {k: dict(e_gpu=v[0], e32=v[1], bar=v[2], share=v[0] / v[2]) for k, v in _shares(g).items()}
           for g in trh.BAR_GRID}
    out["largest_share_of_the_bar"] = max(t["share"] for v in list(out.values()) for t in v.values())
    return out


@pytest.mark.parametrize("g", trh.BAR_GRID, ids=lambda g: "N%d-E%d-Q%d" % g)
def test_resampled_rows_match_float64(g):
    assert np.array_equal(grid_run(g)["members"], trh.grid_refs(*g)[0]["members"])
    failures = []
    for k, (e, own, bar) in _shares(g).items():
        print(f"RATIO {g} {k}: e(gpu) {e:.3e}, e32 {own:.3e}, bar {bar:.3e}")
        if not e <= bar:
            failures.append(f"{k}: e(gpu) = {e:.3e} > bar = {bar:.3e}")
    assert not failures, f"{g}: " + "; ".join(failures)


def test_resampled_with_one_member_is_fixed_with_q_particles():
    name = "no_action_cost"                     # E = 1
    p, mems = ref.problem(name), device_members(name)
    for Q in (1, 3):
        got, want = run_rows(p, mems, RESAMPLED, Q), run_rows(p, mems, FIXED, Q)
        assert _same(got, want) and np.all(got["members"] == 0)


def test_resampled_over_identical_member_copies_is_fixed():
    name = "n17_e2p3"
    p, m0 = ref.problem(name), device_members(name)[0]
    got, want = run_rows(p, [m0, m0], RESAMPLED, 6), run_rows(p, [m0, m0], FIXED, 3)
    assert _same(got, want)
    assert set(np.unique(got["members"])) == {0, 1}            # (the draw did pick both copies)


BIG = (40, 5, 7)       # N = 40: three tiles, the last one partial; s0 per candidate


def _slice(p, lo, hi):
    return dict(s0=p["s0"][lo:hi], actions=np.ascontiguousarray(p["actions"][:, lo:hi]), n_offset=p["n_offset"] + lo)


@pytest.mark.parametrize("lo, hi", [(0, 17), (16, 40), (23, 24), (39, 40)])
def test_a_resampled_candidate_does_not_depend_on_n_or_its_tile_position(lo, hi):
    p, full = trh.grid_problem(*BIG), grid_run(BIG)
    assert np.ndim(p["s0"]) == 2
    part = run_rows(p, _dev_members(p), RESAMPLED, BIG[2], **_slice(p, lo, hi))
    assert part["states"].tobytes() == np.ascontiguousarray(full["states"][:, :, lo:hi]).tobytes()
    assert part["costs"].tobytes() == np.ascontiguousarray(full["costs"][:, lo:hi]).tobytes()
    assert np.array_equal(part["members"], full["members"])


def test_a_non_finite_neighbour_and_null_outputs_change_nothing_else():
    p, full = trh.grid_problem(*BIG), grid_run(BIG)
    mems = _dev_members(p)
    s0 = p["s0"].copy()
    s0[22], s0[33, 1] = NAN, np.inf
    got = run_rows(p, mems, RESAMPLED, BIG[2], s0=s0)
    others = [n for n in range(40) if n not in (22, 33)]
    assert np.all(np.isnan(got["costs"][:, 22]))
    assert np.ascontiguousarray(got["states"][..., others, :]).tobytes() == \
        np.ascontiguousarray(full["states"][..., others, :]).tobytes()
    assert np.ascontiguousarray(got["costs"][:, others]).tobytes() == np.ascontiguousarray(full["costs"][:, others]).tobytes()
    for kw in (dict(with_states=False), dict(with_members=False), dict(with_states=False, with_members=False),
               dict(fill="ff")):
        assert _same(run_rows(p, mems, RESAMPLED, BIG[2], **kw), full, ("states", "costs", "members")), kw


def test_a_member_a_row_never_ran_does_not_reach_the_row():
    g = (17, 5, 3)
    p, full = trh.grid_problem(*g), grid_run(g)
    mems = _dev_members(p)
    seen = 0
    for q in range(g[2]):
        ran = set(full["members"][q].tolist())
        if len(ran) == 5:
            continue
        seen += 1
        poisoned = [params if e in ran else [torch.full_like(t, NAN) for t in params] for e, params in enumerate(mems)]
        got = run_rows(p, poisoned, RESAMPLED, g[2])
        assert got["states"][q].tobytes() == full["states"][q].tobytes()
        assert got["costs"][q].tobytes() == full["costs"][q].tobytes()
        for r in range(g[2]):                   # a row that did run a poisoned member shows it
            if not set(full["members"][r].tolist()) <= ran:
                assert np.all(np.isnan(got["costs"][r])), (q, r)
    assert seen >= 1


def test_another_iteration_seed_or_row_changes_the_member_sequence():
    p = ref._draw(ref._c(5, 2, 16, 1, 3, 9, 5, 1, iteration=3), 6950)
    mems = _dev_members(p)
    base = run_rows(p, mems, RESAMPLED, 7)["members"]
    assert len({tuple(r) for r in base}) == 7
    for change in (dict(iteration=4), dict(noise_seed=p["noise_seed"] + 1), dict(noise_seed=p["noise_seed"] | (1 << 40))):
        assert not np.array_equal(run_rows(p, mems, RESAMPLED, 7, **change)["members"], base), change


def _bad_rows():
    yield "unknown member_mode", 2, 3, {}
    yield "negative member_mode", -1, 3, {}
    yield "resampled particles < 1", RESAMPLED, 0, {}
    yield "resampled rows above MBRL_TS_MAX_ROWS", RESAMPLED, 257, {}
    yield "fixed rows above MBRL_TS_MAX_ROWS", FIXED, 129, {}
    yield "negative noise_scale", RESAMPLED, 3, dict(noise_scale=-1.0)
    yield "iteration 2^24", RESAMPLED, 3, dict(iteration=1 << 24)
    yield "negative n_offset", RESAMPLED, 3, dict(n_offset=-1)
    yield "state cost without weights", RESAMPLED, 3, dict(cost=dict(ref.problem("n17_e2p3")["cost"], weights=None))


@pytest.mark.parametrize("label, mode, particles, change", list(_bad_rows()), ids=[b[0] for b in _bad_rows()])
def test_rows_argument_errors_return_einval_and_leave_the_outputs_untouched(label, mode, particles, change):
    name = "n17_e2p3"
    rc, states, costs, mem = run_rows(ref.problem(name), device_members(name), mode, particles, raw=True, **change)
    assert rc == -1, (label, rc)
    assert bool(torch.isnan(states).all()) and bool(torch.isnan(costs).all()) and bool((mem == -1).all())


def test_the_resampled_row_bound_is_on_the_rows_themselves_and_null_rows_are_refused():
    from mbrl_amd import _lib
    lib = _lib.load()
    name = "n17_e2p3"                           # E = 2: 256 rows would be 128 particles in FIXED mode
    got = run_rows(ref.problem(name), device_members(name), RESAMPLED, 256, with_states=False)
    assert np.all(np.isfinite(got["costs"])) and got["members"].min() >= 0 and got["members"].max() <= 1
    assert lib.mbrl_rollout_cost_ts_rows(None, 2, None, None, None, None, 0, None, 1, 1, 0, None, None, None, None,
                                         None) == _lib.MBRL_EINVAL


# ---- the plans
ALPHA, ISIG, PSEED, NOISE = 0.1, 0.5, (7 << 32) | 99, 0.75
MODES = {"fixed": (FIXED, 2, 2, 17, 6, 64, 2), "resampled": (RESAMPLED, 3, 5, 5, 12, 33, 1)}   # mode, P, E, s, a, W, L


def _setup(mode_name, seed=3):
    from mbrl_amd import fused
    mode, P, E, s, a, W, L = MODES[mode_name]
    ens = _prob_ensemble(E, s, a, W, L, seed=seed)
    model_fn, cost_fn, sample, s0 = _closures(ens, s, a)
    _, _, prob = fused.describe_problem(model_fn, cost_fn, DEV, 0)
    table = fused.ts_members(ens, DEV)
    Q = P if mode == RESAMPLED else E * P
    return dict(ens=ens, model_fn=model_fn, cost_fn=cost_fn, sample=sample, s0=s0, prob=prob, table=table, mode=mode,
                P=P, E=E, s=s, a=a, Q=Q)


def call_plan(S, s0, N, H, K, I, keep, seed, *, B=None, mu_rows=None, sigma_rows=None, carry=None, flags=None, fill="nan",
              raw=False, rows=None, ws_bytes=None, null=(), shape=None, cost=None):
    """mbrl_cem_plan_ts_rh (B None) or its batch on setup S with every record on: the outputs as NumPy (raw: rc and
    the device tensors)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    prob, table, a, s, Q = S["prob"], S["table"], S["a"], S["s"], S["Q"]
    nb = 1 if B is None else B
    lead = () if B is None else (B,)
    rp = _lib.CemRhParams(_lib.CemParams(N, H, K, I, ALPHA, LO, HI, 0.0, ISIG, 0, seed), keep, 0)
    rows = _lib.TsRows(_lib.TsParams(S["P"], 12345, PSEED, NOISE), S["mode"], 0) if rows is None else rows
    shape_ref = prob.refs[0] if shape is None else ctypes.byref(shape)
    need = lib.mbrl_cem_ts_rh_workspace_bytes(prob.refs[0], ctypes.byref(rp), ctypes.byref(rows), nb)
    if raw and need == 0:
        need = 1 << 20
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ws.view(torch.float32)[:need // 4].fill_(NAN) if fill == "nan" else ws.fill_(0xFF)
    Kc = max(keep, 1) if raw else keep
    sh = dict(mu=(*lead, H, a), sigma=(*lead, H, a), actions=(*lead, H, a), states=(*lead, H, s),
              carry=(*lead, Kc, H, a), carry_returns=(*lead, Kc), costs=(I, Q, nb * N), returns=(I, *lead, N),
              kept_hist=(I + 1, *lead, Kc, H, a))
    out = {k: _filled(v, fill) for k, v in sh.items() if (raw or keep or not k.startswith(("carry", "kept")))}
    out["elites"] = torch.full((I, *lead, K), -1, dtype=torch.int64, device=DEV)
    ins = [None if x is None else _t(x) for x in (mu_rows, sigma_rows, carry)]
    fl = None if flags is None else torch.tensor(flags, dtype=torch.int32, device=DEV)
    s0d = _t(s0)
    g = lambda k: None if (k in null or k not in out) else _P(out[k])   # noqa: E731
    head = [shape_ref, None if "packed" in null else prob.refs[1], *(table.refs if "members" not in null else (None, None)),
            prob.refs[2], prob.refs[3] if cost is None else ctypes.byref(cost), None if "s0" in null else _P(s0d)]
    mid = [ctypes.byref(rp), ctypes.byref(rows), *[None if x is None else _P(x) for x in ins]]
    tail = [g("mu"), g("sigma"), g("actions"), g("states"), g("carry"), g("carry_returns"), g("costs"), g("returns"),
            g("elites"), g("kept_hist"), None if "ws" in null else _P(ws), need if ws_bytes is None else ws_bytes,
            _lib.stream_handle(DEV)]
    if B is None:
        rc = lib.mbrl_cem_plan_ts_rh(*head, *mid, *tail)
    else:
        rc = lib.mbrl_cem_plan_ts_rh_batch(*head, B, *mid, None if fl is None else _P(fl), *tail)
    torch.cuda.synchronize()
    if raw:
        return rc, out
    _lib.check(rc, "mbrl_cem_plan_ts_rh")
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_keep_zero_fixed_without_rows_is_cem_plan_ts():
    from mbrl_amd import _lib
    lib = _lib.load()
    S = _setup("fixed")
    N, H, K, I, seed = 64, 4, 8, 3, 31
    prob, table = S["prob"], S["table"]
    got = call_plan(S, S["s0"], N, H, K, I, 0, seed)
    cem = _lib.CemParams(N, H, K, I, ALPHA, LO, HI, 0.0, ISIG, 0, seed)
    tsp = _lib.TsParams(S["P"], 0, PSEED, NOISE)
    need = lib.mbrl_cem_ts_workspace_bytes(prob.refs[0], ctypes.byref(cem), ctypes.byref(tsp))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    outs = [_filled(sh, "nan") for sh in ((H, S["a"]), (H, S["a"]), (H, S["a"]), (H, S["s"]), (I, S["Q"], N), (I, N))]
    elites = torch.full((I, K), -1, dtype=torch.int64, device=DEV)
    s0d = S["s0"].to(DEV)
    _lib.check(lib.mbrl_cem_plan_ts(prob.refs[0], prob.refs[1], *table.refs, prob.refs[2], prob.refs[3], _P(s0d),
                                    ctypes.byref(cem), ctypes.byref(tsp), *[_P(x) for x in outs], _P(elites), _P(ws),
                                    need, _lib.stream_handle(DEV)), "mbrl_cem_plan_ts")
    torch.cuda.synchronize()
    for k, x in zip(("mu", "sigma", "actions", "states", "costs", "returns"), outs):
        assert got[k].tobytes() == x.cpu().numpy().tobytes(), k
    assert np.array_equal(got["elites"], elites.cpu().numpy())


def _check_chain(S, got, s0, N, H, K, I, keep, seed, b=0, B=None, **inputs):
    """Problem b of `got` (B None: the single plan) against its chain."""
    from mbrl_amd import fused
    a = S["a"]
    pick = (lambda x, axis=0: x) if B is None else (lambda x, axis=0: np.take(x, b, axis=axis))
    costs = [np.ascontiguousarray(got["costs"][i][:, b * N:(b + 1) * N]) for i in range(I)]
    want = trh.plan_given_costs(costs, N, H, a, K, keep=keep, seed=seed, alpha=ALPHA, lo=LO, hi=HI, init_sigma=ISIG, b=b,
                                **inputs)
    s0d = _t(s0)
    for i in range(I):
        acts = _t(want["actions"][i])
        rolled = fused.rollout_ts(S["prob"], s0d, acts, particles=S["P"], noise_seed=PSEED, noise_scale=NOISE, iteration=i,
                                  n_offset=b * N, member_mode=S["mode"])
        assert rolled.cpu().numpy().tobytes() == costs[i].tobytes(), ("costs", i)
        assert pick(got["returns"][i]).tobytes() == want["returns"][i].tobytes(), ("returns", i)
        assert np.array_equal(pick(got["elites"][i]), want["elites"][i]), ("elites", i)
    if keep:
        for i in range(I + 1):
            assert pick(got["kept_hist"][i]).tobytes() == want["kept"][i].tobytes(), ("kept", i)
        assert pick(got["carry"]).tobytes() == want["carry"].tobytes()
        assert pick(got["carry_returns"]).tobytes() == want["carry_returns"].tobytes()
    assert pick(got["mu"]).tobytes() == want["mu_out"].tobytes() and pick(got["sigma"]).tobytes() == want["sigma_out"].tobytes()
    assert pick(got["actions"]).tobytes() == want["final_actions"].tobytes()
    states = fused.trajectory(S["prob"], s0d, _t(pick(got["actions"])), H)
    torch.cuda.synchronize()
    assert pick(got["states"]).tobytes() == states.cpu().numpy().tobytes()


def _inputs(rng, H, a, keep, mu, sigma, carry):
    kw = {}
    if mu:
        kw["init_mu_rows"] = rng.uniform(-1.3, 1.3, (H, a)).astype(np.float32)
    if sigma:
        kw["init_sigma_rows"] = rng.uniform(0.1, 0.6, (H, a)).astype(np.float32)
    if carry:
        kw["carry_in"] = rng.uniform(-1.2, 1.2, (keep, H, a)).astype(np.float32)
    return kw


_SETUPS = {}


def _cached_setup(mode_name):
    if mode_name not in _SETUPS:
        _SETUPS[mode_name] = _setup(mode_name)
    return _SETUPS[mode_name]


@pytest.mark.parametrize("mode_name, N, keep", list(itertools.product(MODES, (40, 64), (0, 3))))
def test_the_plan_equals_its_chain(mode_name, N, keep):
    S = _cached_setup(mode_name)
    H, K, I = 4, 8, 3
    rng = np.random.default_rng(N + keep)
    for mu, sigma, carry in itertools.product((False, True), (False, True), (False, True) if keep else (False,)):
        kw = _inputs(rng, H, S["a"], keep, mu, sigma, carry)
        seed = 100 + 4 * mu + 2 * sigma + carry
        got = call_plan(S, S["s0"], N, H, K, I, keep, seed, mu_rows=kw.get("init_mu_rows"),
                        sigma_rows=kw.get("init_sigma_rows"), carry=kw.get("carry_in"))
        assert all(np.all(np.isfinite(v)) for v in got.values())
        _check_chain(S, got, S["s0"], N, H, K, I, keep, seed, **kw)


@pytest.mark.parametrize("mode_name, B", list(itertools.product(MODES, (1, 3))))
def test_the_batch_is_the_single_plan_and_every_problem_passes_its_chain(mode_name, B):
    S = _cached_setup(mode_name)
    N, H, K, I, keep, seed = 40, 4, 8, 3, 3, 55
    a, s = S["a"], S["s"]
    rng = np.random.default_rng(B)
    s0s = np.stack([S["s0"].numpy()] + [rng.standard_normal(s).astype(np.float32) for _ in range(B - 1)])
    given = ["msc", "", "m"][:B]                # problem 1: every pointer given, every flag clear
    kws = [_inputs(rng, H, a, keep, True, True, True) for _ in range(B)]
    flags = [sum(bit for ch, bit in zip("msc", (1, 2, 4)) if ch in gv) for gv in given]
    stack = lambda k: np.stack([kw[k] for kw in kws])   # noqa: E731
    got = call_plan(S, s0s, N, H, K, I, keep, seed, B=B, mu_rows=stack("init_mu_rows"),
                    sigma_rows=stack("init_sigma_rows"), carry=stack("carry_in"), flags=flags)
    used = [{k: kw[k] for k, ch in (("init_mu_rows", "m"), ("init_sigma_rows", "s"), ("carry_in", "c")) if ch in gv}
            for kw, gv in zip(kws, given)]
    single = call_plan(S, s0s[0], N, H, K, I, keep, seed, mu_rows=used[0].get("init_mu_rows"),
                       sigma_rows=used[0].get("init_sigma_rows"), carry=used[0].get("carry_in"))
    for k in ("mu", "sigma", "actions", "states", "carry", "carry_returns"):
        assert got[k][0].tobytes() == single[k].tobytes(), k
    for k in ("returns", "elites", "kept_hist"):
        assert np.ascontiguousarray(got[k][:, 0]).tobytes() == single[k].tobytes(), k
    assert np.ascontiguousarray(got["costs"][:, :, :N]).tobytes() == single["costs"].tobytes()
    if B == 1:
        assert got["costs"].tobytes() == single["costs"].tobytes()
    for b in range(B):
        _check_chain(S, got, s0s[b], N, H, K, I, keep, seed, b=b, B=B, **used[b])


@pytest.mark.parametrize("B", [None, 3])
def test_the_plans_do_not_depend_on_prior_workspace_or_output_bytes(B):
    S = _cached_setup("resampled")
    rng = np.random.default_rng(5)
    s0 = S["s0"].numpy() if B is None else rng.standard_normal((B, S["s"])).astype(np.float32)
    for keep in (0, 3):
        runs = [call_plan(S, s0, 40, 4, 8, 2, keep, 9, B=B, fill=fill) for fill in ("nan", "ff")]
        assert all(np.all(np.isfinite(v)) for v in runs[0].values())
        assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in runs[0])


def test_every_plan_refusal_returns_its_code_before_any_launch():
    from mbrl_amd import _lib
    S = _cached_setup("fixed")
    EINVAL, EUNSUP, EWS = _lib.MBRL_EINVAL, _lib.MBRL_EUNSUPPORTED, _lib.MBRL_EWORKSPACE
    s0, s0s = S["s0"].numpy(), np.zeros((2, S["s"]), np.float32)
    rows = lambda P, mode, noise=NOISE: _lib.TsRows(_lib.TsParams(P, 0, PSEED, noise), mode, 0)   # noqa: E731
    carry = np.zeros((1, 4, S["a"]), np.float32)
    f16 = type(S["prob"].shape).from_buffer_copy(S["prob"].shape)
    f16.precision = 1
    reward = _lib.Cost(_lib.MBRL_COST_MODEL_REWARD, 0, 0, 0, None, None, 0.0, 0.0)
    cases = [
        ("keep above K", EINVAL, dict(keep=9)), ("negative keep", EINVAL, dict(keep=-1)),
        ("carry with keep == 0", EINVAL, dict(keep=0, carry=carry)), ("NULL s0", EINVAL, dict(null=("s0",))),
        ("NULL packed", EINVAL, dict(null=("packed",))), ("NULL members", EINVAL, dict(null=("members",))),
        ("NULL actions_out", EINVAL, dict(null=("actions",))), ("NULL states_out", EINVAL, dict(null=("states",))),
        ("NULL workspace", EINVAL, dict(null=("ws",))), ("unknown member_mode", EINVAL, dict(rows=rows(2, 7))),
        ("particles < 1", EINVAL, dict(rows=rows(0, FIXED))), ("fixed rows above 256", EINVAL, dict(rows=rows(129, FIXED))),
        ("resampled rows above 256", EINVAL, dict(rows=rows(257, RESAMPLED))),
        ("negative noise_scale", EINVAL, dict(rows=rows(2, FIXED, -1.0))), ("K above N", EINVAL, dict(K=41)),
        ("N above 32768", EUNSUP, dict(N=32769)), ("an f16 precision", EUNSUP, dict(shape=f16)),
        ("a reward-head cost", EINVAL, dict(cost=reward)), ("single: small workspace", EINVAL, dict(ws_bytes=1024)),
        ("batch: small workspace", EWS, dict(B=2, ws_bytes=1024)), ("batch: B < 1", EINVAL, dict(B=0)),
        ("batch: NULL s0", EINVAL, dict(B=2, null=("s0",))),
    ]
    for label, code, kw in cases:
        kw = dict(dict(N=40, K=8, keep=1), **kw)
        B = kw.pop("B", None)
        N, K, keep = kw.pop("N"), kw.pop("K"), kw.pop("keep")
        rc, out = call_plan(S, s0 if B is None else s0s[:max(B, 1)], N, 4, K, 2, keep, 3, B=B, raw=True, **kw)
        assert rc == code, (label, rc, _lib.load().mbrl_last_error())
        assert all(bool(torch.isnan(v).all()) for k, v in out.items() if k != "elites") and bool((out["elites"] == -1).all()), label


# ---- TrajectorySamplingCEMPlanner
def _kw(S, **more):
    return dict(dict(num_candidates=64, num_elites=8, num_iterations=3, seed=21, init_std=ISIG, particles=S["P"],
                     particle_mode="fixed" if S["mode"] == FIXED else "resampled", particle_noise=NOISE, particle_seed=PSEED,
                     device=str(DEV)), **more)


@pytest.mark.parametrize("mode_name", list(MODES))
def test_plan_detailed_returns_the_c_plan(mode_name):
    from mbrl_amd import TrajectorySamplingCEMPlanner as TS, planners
    S = _cached_setup(mode_name)
    H, a = 4, S["a"]
    rng = np.random.default_rng(2)
    prev = torch.from_numpy(rng.uniform(-1.2, 1.2, (H, a)).astype(np.float32))
    carry = rng.uniform(-1.2, 1.2, (2, H, a)).astype(np.float32)       # keep_elites = 0.3 of 8 elites: 2 rows
    res = TS.plan_detailed(S["s0"], S["model_fn"], S["cost_fn"], S["sample"], H, (None, prev), record=True, carry=carry,
                           warm_std=0.3, **_kw(S))
    rows = planners.mppi_warm_start_rows(prev, H, 1, LO, HI)
    want = call_plan(S, S["s0"].numpy(), 64, H, 8, 3, 2, 21, mu_rows=rows, sigma_rows=np.full((H, a), 0.3, np.float32),
                     carry=carry)
    assert res["costs"].shape == (3, S["Q"], 64) and not res["actions"].is_cuda
    for k in ("mu", "sigma", "actions", "states", "carry", "carry_returns", "costs", "returns", "elites", "kept_hist"):
        assert res[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert np.array_equal(res["init_mu"].numpy(), rows)
    # the defaults: a first control step plans cold, with kept rows
    cold = TS.plan_detailed(S["s0"], S["model_fn"], S["cost_fn"], S["sample"], H, **_kw(S))
    base = call_plan(S, S["s0"].numpy(), 64, H, 8, 3, 2, 21)
    assert cold["actions"].numpy().tobytes() == base["actions"].tobytes() and cold["carry"].shape == (2, H, a)


def test_mpc_policy_steps_are_plans_from_the_shifted_trajectories():
    from mbrl_amd import MPCPolicy, TrajectorySamplingCEMPlanner as TS
    S = _cached_setup("resampled")
    H = 4
    pol = MPCPolicy(S["model_fn"], S["cost_fn"], TS, S["sample"], H, **_kw(S))
    rng = np.random.default_rng(8)
    obs = [torch.from_numpy(rng.standard_normal(S["s"]).astype(np.float32)) for _ in range(3)]
    last = None
    for t, o in enumerate(obs):
        act = pol.get_action(dict(timestep=t, observation=o))
        init = None if last is None else (last[0][1:], last[1])
        direct = TS.plan(o, S["model_fn"], S["cost_fn"], S["sample"], H, init, **_kw(S))
        assert torch.equal(pol.last_trajectory[0], direct[0]) and torch.equal(pol.last_trajectory[1], direct[1])
        assert torch.equal(act, direct[1][0])
        if last is not None:                    # the warm start is used: a cold plan differs
            cold = TS.plan(o, S["model_fn"], S["cost_fn"], S["sample"], H, **_kw(S))
            assert not torch.equal(cold[1], direct[1])
        last = direct


def test_plan_batch_with_memos_is_the_batched_call_with_the_shifted_carry_and_sigma():
    from mbrl_amd import TrajectorySamplingCEMPlanner as TS, planners
    S = _cached_setup("fixed")
    H, B, a = 4, 3, S["a"]
    rng = np.random.default_rng(4)
    s0s = torch.from_numpy(rng.standard_normal((B, S["s"])).astype(np.float32))
    kw = _kw(S, warm_std="keep")
    args = (S["model_fn"], S["cost_fn"], S["sample"], H)
    st1, ac1, memos = TS.plan_batch(s0s, *args, **kw)
    first = call_plan(S, s0s.numpy(), 64, H, 8, 3, 2, 21, B=B)
    assert ac1.numpy().tobytes() == first["actions"].tobytes() and st1.numpy().tobytes() == first["states"].tobytes()
    assert all(m["carry"].numpy().tobytes() == first["carry"][b].tobytes() for b, m in enumerate(memos))
    # the second control step: problem 1 restarts (no trajectory, no memo)
    inits = [(st1[b][1:], ac1[b]) if b != 1 else None for b in range(B)]
    memos2 = [m if b != 1 else None for b, m in enumerate(memos)]
    s1s = torch.from_numpy(rng.standard_normal((B, S["s"])).astype(np.float32))
    st2, ac2, _ = TS.plan_batch(s1s, *args, initial_trajectories=inits, memos=memos2, **kw)
    mu_rows = np.stack([planners.mppi_warm_start_rows(ac1[b], H, 1, LO, HI) for b in range(B)])
    sg_rows = np.stack([planners.mppi_warm_start_rows(memos[b]["sigma"], H, 1, 0.0, np.inf) for b in range(B)])
    carry = np.stack([planners.cem_shift_carry(memos[b]["carry"], 1, LO, HI) for b in range(B)])
    second = call_plan(S, s1s.numpy(), 64, H, 8, 3, 2, 21, B=B, mu_rows=mu_rows, sigma_rows=sg_rows, carry=carry,
                       flags=[7, 0, 7])
    assert ac2.numpy().tobytes() == second["actions"].tobytes() and st2.numpy().tobytes() == second["states"].tobytes()


def test_a_plan_after_train_members_uses_the_new_weights():
    from mbrl_amd import TrajectorySamplingCEMPlanner as TS, env, models
    s, a, W = 6, 2, 48
    ds = _dataset(s, a, 1, 300, seed=8)
    ens = _prob_ensemble(2, s, a, W, 2, seed=1)
    cost = models.goal_state_cost(models.SmoothAbsLoss(torch.ones(s), torch.zeros(s), 0.4), models.CoshLoss(0.25))
    sample = env.sample_action_fn(env.BoundedActionSpec(a, LO, HI))
    s0 = torch.linspace(-1, 1, s)

    def plan(module):
        res = TS.plan_detailed(s0, module, cost, sample, 4, num_candidates=64, num_iterations=2, seed=3, particles=3,
                               particle_mode="resampled", record=True, device=str(DEV))
        return [res[k].detach().cpu().clone() for k in ("actions", "mu", "sigma", "costs", "carry")]
    before = plan(ens)
    ens.train_members(ds, [torch.optim.Adam(m.parameters(), lr=3e-3) for m in ens.members], batch_size=64,
                      num_epochs=3, seed=2, loss="nll")
    after = plan(ens)
    fresh = _prob_ensemble(2, s, a, W, 2, seed=7)
    fresh.load_state_dict(copy.deepcopy(ens.state_dict()))
    want = plan(fresh)
    assert all(torch.equal(x, y) for x, y in zip(after, want))
    assert not any(torch.equal(x, y) for x, y in zip(after, before))
