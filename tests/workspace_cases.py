"""The table of tests/test_gpu_workspace_independence.py: one or more cases per exported function of
include/mbrl_cem.h that takes a `void* workspace` (tests/test_workspace_cases.py derives that list from the
header and asserts every name has a case). Importing this module needs no GPU; running a case does.

A case is `run(make_ws, alloc=None) -> dict[str, Tensor or ndarray]`. It obtains its workspace only through
make_ws(nbytes) -- nbytes is exactly what the entry's size query returned, and that is the ws_bytes passed --
and every output and record array the call can write through alloc(*shape, dt=torch.float32) (None: plain
tensors), and returns all of them: records on, histories, carries, iteration counts, losses. Nothing is NULL
that the call could write.

Shapes, the smallest at which the workspace-resident machinery is live (asserted with
tests/rollout_dispatch_model.py in tests/test_workspace_cases.py, which needs no GPU):
  narrow   s 4, a 1, W 64, L 2, N 64, H 4, K 8: the register trajectory, no pair area
  pair     s 17, a 6, W 512, L 3, N 17, H 3, K 4 under MBRL_OPT_ROLLOUT_PAIR = 1: two 16-candidate tiles on four
           column-split workgroups, the cooperative trajectory; also with DEBUG_PAIR_ABORT = 1 (the gated redo
           reads its gate word from the workspace) and DEBUG_TRAJ_ABORT = 1 (the gated trajectory fallback).
           Entries that take no pair area (batches, mixed plans) run the shape as "wide": the cooperative
           trajectory with its own memset
  ens      narrow with E = 3: the member scratch and the member mean
  plain    s 90, a 6, W 64, L 2: neither the register nor the cooperative trajectory kernel takes it
Every plan runs with the fused update and under MBRL_OPT_UNFUSED_UPDATE = 1 (separate select and refit scratch);
mbrl_cem_plan also under MBRL_OPT_UPDATE_SPLIT = 2 (the two-launch update) and = 1 (never split). Batches are
B = 3. The sharded plan runs under MBRL_OPT_SHARD_EMULATE = 1 (comm == NULL) as one rank and as both ranks of two
(narrow: 32 per rank; pair: 17 per rank).
gd: W 64, L 2, H 3, B 1 and 3, the cooperative kernel, the one-workgroup kernel (GD_SINGLE) and the gated
fallback (DEBUG_GD_ABORT). Training: s 5, a 2, W 64, horizon 2, batch 130 -- L 2 takes the fused three-launch
step (260 rows), L 3 and L 1 the multi-launch layout -- both model kinds; ensembles of E = 2.

The single-model mbrl_train_grads / mbrl_train_epoch are the documented exception (include/mbrl_cem.h: the
caller zeroes the workspace once): their case (`zeroed_once`) runs grads, an epoch of three batches with the
last one short, and grads again on ONE workspace obtained once, or with fresh=True on a new one per call, and
reports the status word after each call. The GPU test gives them zeroed workspaces only."""
import ctypes
import functools
from collections import namedtuple
from contextlib import ExitStack

import numpy as np

F32 = np.float32
LO, HI = -1.0, 1.0
DEV = "cuda:0"
B = 3

SHAPES = {
    "narrow": dict(cid=2, over=dict(s=4, a=1, W=64, L=2, E=1), N=64, H=4, K=8),
    "pair": dict(cid=3, over=dict(s=17, a=6, W=512, L=3, E=1), N=17, H=3, K=4),
    "ens": dict(cid=2, over=dict(s=4, a=1, W=64, L=2, E=3), N=64, H=4, K=8),
    "plain": dict(cid=3, over=dict(s=90, a=6, W=64, L=2, E=1), N=64, H=3, K=8),
}
SHAPES["wide"] = SHAPES["pair"]
I = 2                       # iterations of every plan
TRAJECTORY = {"narrow": "reg", "pair": "coop", "wide": "coop", "ens": "reg", "plain": "plain"}

Case = namedtuple("Case", "entries run zeroed_once")
CASES = {}


def _add(name, entries, fn, opts=(), zeroed_once=False):
    """Registers fn(ctx) under `name`; `opts` are MBRL_OPT_* switches held for the whole call, size query included."""
    def run(make_ws, alloc=None, **kw):
        import torch
        from mbrl_amd import _lib
        default = lambda *sh, dt=torch.float32: torch.full(sh, -7, dtype=dt, device=DEV)  # noqa: E731
        with ExitStack() as stack:
            for k, v in opts:
                stack.enter_context(_lib.option(k, v))
            out = fn(_Ctx(make_ws, alloc or default), **kw)
            torch.cuda.synchronize()
        return out
    assert name not in CASES, name
    CASES[name] = Case(tuple(entries), run, zeroed_once)


_Ctx = namedtuple("_Ctx", "make_ws alloc")


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(oracle problem, DeviceProblem) of a shape; shared, never written."""
    from oracle import cem as ocem
    from test_gpu_parity import device_problem
    sh = SHAPES[shape]
    p = ocem.synth_problem(sh["cid"], seed=9100 + len(shape), N=sh["N"], H=sh["H"], **sh["over"])
    return p, device_problem(p)


def _dims(shape):
    sh = SHAPES[shape]
    o = sh["over"]
    return sh["N"], sh["H"], sh["K"], o["s"], o["a"], o["E"]


def _dev(x, dt=None):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt or F32)).to(DEV)


def _s0s(p, n=B):
    rng = np.random.default_rng(5)
    return np.stack([p["s0"]] + [(p["s0"] + rng.normal(0, 0.2, p["s0"].shape)).astype(F32) for _ in range(n - 1)])


def _rows(shape, batch=None, keep=0, seed=3):
    """Warm-start rows, sigma rows and (keep > 0) a carry, for one plan or stacked for `batch` plans."""
    _, H, _, _, a, _ = _dims(shape)
    rng = np.random.default_rng(seed)
    lead = () if batch is None else (batch,)
    kw = dict(init_mu_rows=rng.uniform(-1.3, 1.3, lead + (H, a)).astype(F32),
              init_sigma_rows=rng.uniform(0.1, 0.6, lead + (H, a)).astype(F32))
    if keep:
        kw["carry_in"] = rng.uniform(-1.2, 1.2, lead + (keep, H, a)).astype(F32)
    return kw


def _mix(H):
    return np.random.default_rng(5).normal(0.0, 1.0 / np.sqrt(H), (H, H)).astype(F32)


def _call(name, rc):
    from mbrl_amd import _lib
    _lib.check(rc, name)


def _stream():
    import torch
    from mbrl_amd import _lib
    return _lib.stream_handle(torch.device(DEV))


# ------------------------------------------------------------------------------------------------ select, refit
def _select(ctx, N=300, K=30, E=3):
    import torch
    from mbrl_amd import _lib
    lib = _lib.load()
    costs = _dev(np.random.default_rng(1).standard_normal((E, N)))
    out = dict(elites=ctx.alloc(K, dt=torch.int64), returns=ctx.alloc(N))
    ws = ctx.make_ws(lib.mbrl_select_workspace_bytes(N))
    _call("mbrl_select_elites", lib.mbrl_select_elites(_lib.ptr(costs), E, N, K, _lib.MBRL_NAN_LAST, _lib.ptr(out["elites"]),
                                                        _lib.ptr(out["returns"]), _lib.ptr(ws), ws.numel(), _stream()))
    return out


def _refit(ctx, H=4, a=5, K=9, N=64):
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    rng = np.random.default_rng(2)
    mu, sg = _dev(rng.uniform(-0.5, 0.5, (H, a))), _dev(rng.uniform(0.1, 0.9, (H, a)))
    elites = _dev(np.sort(rng.choice(N, K, replace=False)), np.int64)
    sp = fused.make_sampler(77, 1, mu, sg, LO, HI)
    out = dict(mu=ctx.alloc(H, a), sigma=ctx.alloc(H, a))
    ws = ctx.make_ws(lib.mbrl_refit_workspace_bytes(H, a, K))
    _call("mbrl_cem_refit", lib.mbrl_cem_refit(ctypes.byref(sp), H, a, _lib.ptr(elites), K, 0.1, _lib.ptr(out["mu"]),
                                                _lib.ptr(out["sigma"]), _lib.ptr(ws), ws.numel(), _stream()))
    return out


_add("select", ["mbrl_select_elites"], _select)
_add("select_small", ["mbrl_select_elites"], functools.partial(_select, N=17, K=4, E=1))
_add("refit", ["mbrl_cem_refit"], _refit)


# ------------------------------------------------------------------------------------------------ trajectory
def _trajectory(ctx, shape):
    from test_gpu_flags import trajectory
    p, prob = problem(shape)
    _, H, _, _, a, _ = _dims(shape)
    acts = np.random.default_rng(4).uniform(-1, 1, (H, a)).astype(F32)
    states, members = trajectory(prob, p, acts, make_ws=ctx.make_ws, alloc=ctx.alloc)
    return dict(states=states, members=members)


for _shape in ("narrow", "wide", "ens", "plain"):
    _add(f"trajectory_{_shape}", ["mbrl_trajectory"], functools.partial(_trajectory, shape=_shape))
_add("trajectory_wide_traj_abort", ["mbrl_trajectory"], functools.partial(_trajectory, shape="wide"),
     (("debug_traj_abort", 1),))


# ------------------------------------------------------------------------------------------------ CEM plans
def _cem_params(p, N, H, K):
    from mbrl_amd import _lib
    return _lib.CemParams(N, H, K, I, 0.1, LO, HI, 0.0, 0.5, 0, p["rng_seed"] & 0xFFFFFFFFFFFFFFFF)


def _cem_plan(ctx, shape):
    import torch
    from mbrl_amd import _lib
    lib = _lib.load()
    p, prob = problem(shape)
    N, H, K, s, a, E = _dims(shape)
    params = _cem_params(p, N, H, K)
    e = ctx.alloc
    out = dict(mu=e(H, a), sigma=e(H, a), actions=e(H, a), states=e(H, s), costs=e(I, E, N), returns=e(I, N),
               elites=e(I, K, dt=torch.int64))
    ws = ctx.make_ws(lib.mbrl_cem_workspace_bytes(prob.refs[0], ctypes.byref(params)))
    g = lambda k: _lib.ptr(out[k])  # noqa: E731
    _call("mbrl_cem_plan", lib.mbrl_cem_plan(*prob.refs, _lib.ptr(_dev(p["s0"])), ctypes.byref(params), g("mu"), g("sigma"),
                                              g("actions"), g("states"), g("costs"), g("returns"), g("elites"), None,
                                              _lib.ptr(ws), ws.numel(), _stream()))
    return out


def _cem_plan_batch(ctx, shape):
    from mbrl_amd import _lib
    lib = _lib.load()
    p, prob = problem(shape)
    N, H, K, s, a, E = _dims(shape)
    params = _cem_params(p, N, H, K)
    e = ctx.alloc
    out = dict(mu=e(B, H, a), sigma=e(B, H, a), actions=e(B, H, a), states=e(B, H, s))
    ws = ctx.make_ws(lib.mbrl_cem_plan_batch_workspace_bytes(prob.refs[0], ctypes.byref(params), B))
    g = lambda k: _lib.ptr(out[k])  # noqa: E731
    _call("mbrl_cem_plan_batch", lib.mbrl_cem_plan_batch(*prob.refs, _lib.ptr(_dev(_s0s(p))), B, ctypes.byref(params), g("mu"),
                                                          g("sigma"), g("actions"), g("states"), _lib.ptr(ws), ws.numel(),
                                                          _stream()))
    return out


def _cem_plan_sharded(ctx, shape, nranks):
    """Every rank of `nranks`, one call each on a workspace of its own, under MBRL_OPT_SHARD_EMULATE = 1
    (comm == NULL)."""
    import torch
    from mbrl_amd import _lib
    lib = _lib.load()
    p, prob = problem(shape)
    Nl, H, K, s, a, E = _dims(shape)
    N = Nl * nranks if shape == "pair" else Nl          # (narrow: 64 over two ranks, 32 each)
    params = _cem_params(p, N, H, K)
    e = ctx.alloc
    res = {}
    for rank in range(nranks):
        out = dict(mu=e(H, a), sigma=e(H, a), actions=e(H, a), states=e(H, s), costs=e(I, E, N), returns=e(I, N),
                   elites=e(I, K, dt=torch.int64))
        ws = ctx.make_ws(lib.mbrl_cem_plan_sharded_workspace_bytes(prob.refs[0], ctypes.byref(params), nranks))
        g = lambda k: _lib.ptr(out[k])  # noqa: E731
        _call("mbrl_cem_plan_sharded",
              lib.mbrl_cem_plan_sharded(*prob.refs, _lib.ptr(_dev(p["s0"])), ctypes.byref(params), None, nranks, rank, g("mu"),
                                        g("sigma"), g("actions"), g("states"), g("costs"), g("returns"), g("elites"), None,
                                        _lib.ptr(ws), ws.numel(), _stream()))
        torch.cuda.synchronize()
        res.update({f"rank{rank}.{k}": v for k, v in out.items()})
    return res


def _cem_plan_rh(ctx, shape, keep, mixed=False):
    p, prob = problem(shape)
    N, H, K, s, a, E = _dims(shape)
    kw = dict(keep=keep, make_ws=ctx.make_ws, alloc=ctx.alloc, **_rows(shape, keep=keep))
    if mixed:
        from test_gpu_cem_noise import c_plan_mixed
        return c_plan_mixed(prob, p, N, H, K, I, _mix(H), **kw)
    from test_gpu_cem_rh import c_plan_rh
    return c_plan_rh(prob, p, N, H, K, I, **kw)


def _cem_plan_rh_batch(ctx, shape, keep, mixed=False):
    p, prob = problem(shape)
    N, H, K, s, a, E = _dims(shape)
    ins = _rows(shape, batch=B, keep=keep)
    ins["flags"] = np.array([7, 0, 3 if keep else 1], np.int32)     # problem 1 plans cold, problem 2 without its carry
    kw = dict(keep=keep, ins=ins, make_ws=ctx.make_ws, alloc=ctx.alloc)
    if mixed:
        from test_gpu_cem_noise import c_plan_batch_mixed
        return c_plan_batch_mixed(prob, p, _s0s(p), N, H, K, I, _mix(H), **kw)
    from test_gpu_cem_rh_batch import c_plan_rh_batch
    return c_plan_rh_batch(prob, p, _s0s(p), N, H, K, I, **kw)


PAIR = (("rollout_pair", 1),)
UNFUSED = (("unfused_update", 1),)
# (suffix, shape, options): the shapes an entry with a pair area runs, and the ones an entry without one runs
PAIRED_SHAPES = [("narrow", "narrow", ()), ("pair", "pair", PAIR), ("pair_abort", "pair", PAIR + (("debug_pair_abort", 1),)),
                 ("traj_abort", "pair", PAIR + (("debug_traj_abort", 1),)), ("ens", "ens", ()), ("plain", "plain", ())]
UNPAIRED_SHAPES = [("narrow", "narrow", ()), ("wide", "wide", ()), ("traj_abort", "wide", (("debug_traj_abort", 1),)),
                   ("ens", "ens", ())]


def _add_plans(prefix, entries, fn, shapes, **kw):
    for suffix, shape, opts in shapes:
        for tag, more in (("", ()), ("_unfused", UNFUSED)):
            _add(f"{prefix}_{suffix}{tag}", entries, functools.partial(fn, shape=shape, **kw), opts + more)


_add_plans("cem_plan", ["mbrl_cem_plan"], _cem_plan, PAIRED_SHAPES)
for _v in (1, 2):
    _add(f"cem_plan_narrow_update_split{_v}", ["mbrl_cem_plan"], functools.partial(_cem_plan, shape="narrow"),
         (("update_split", _v),))
    _add(f"cem_plan_pair_update_split{_v}", ["mbrl_cem_plan"], functools.partial(_cem_plan, shape="pair"),
         PAIR + (("update_split", _v),))
_add_plans("cem_plan_batch", ["mbrl_cem_plan_batch"], _cem_plan_batch, UNPAIRED_SHAPES)
# (comm == NULL needs MBRL_OPT_SHARD_EMULATE at any rank count; one rank has no peers and no emulation buffers)
_EMULATED = [(x, y, z + (("shard_emulate", 1),)) for x, y, z in PAIRED_SHAPES[:4]]
_add_plans("cem_plan_sharded_1rank", ["mbrl_cem_plan_sharded"], _cem_plan_sharded, _EMULATED, nranks=1)
_add_plans("cem_plan_sharded_2ranks", ["mbrl_cem_plan_sharded"], _cem_plan_sharded, _EMULATED[:2], nranks=2)
for _keep in (0, 3):
    _add_plans(f"cem_plan_rh_keep{_keep}", ["mbrl_cem_plan_rh"], _cem_plan_rh, PAIRED_SHAPES[:4], keep=_keep)
    _add_plans(f"cem_plan_rh_batch_keep{_keep}", ["mbrl_cem_plan_rh_batch"], _cem_plan_rh_batch, UNPAIRED_SHAPES[:3],
               keep=_keep)
    _add_plans(f"cem_plan_rh_mixed_keep{_keep}", ["mbrl_cem_plan_rh_mixed"], _cem_plan_rh, PAIRED_SHAPES[:2] + PAIRED_SHAPES[3:4],
               keep=_keep, mixed=True)
    _add_plans(f"cem_plan_rh_batch_mixed_keep{_keep}", ["mbrl_cem_plan_rh_batch_mixed"], _cem_plan_rh_batch,
               UNPAIRED_SHAPES[:2], keep=_keep, mixed=True)


# ------------------------------------------------------------------------------------------------ MPPI
def _mppi_params(p, N, H, K=None):
    from mbrl_amd import _lib
    mp = _lib.MppiParams(N, H, I, 1, 0.7, 0.1, LO, HI, 0.0, 0.5, p["rng_seed"] & 0xFFFFFFFFFFFFFFFF)
    return mp if K is None else _lib.MppiEliteParams(mp, K, 0, 0.05, 0.8)


def _mppi_plan(ctx, shape, elite=False, batch=False):
    """mbrl_mppi_plan / _plan_elite / _plan_batch / _plan_elite_batch with warm-start rows and every record."""
    import torch
    from mbrl_amd import _lib
    lib = _lib.load()
    p, prob = problem(shape)
    N, H, K, s, a, E = _dims(shape)
    params = _mppi_params(p, N, H, K if elite else None)
    pref = ctypes.byref(params)
    nb = B if batch else 1
    lead = (B,) if batch else ()
    e = ctx.alloc
    out = dict(mu=e(*lead, H, a), sigma=e(*lead, H, a), actions=e(*lead, H, a), states=e(*lead, H, s),
               costs=e(I, E, nb * N), weights=e(I, *lead, N), mu_hist=e(I + 1, *lead, H, a), sigma_hist=e(I + 1, *lead, H, a))
    if elite:
        out["elites"] = e(I, *lead, K, dt=torch.int64)
    rows = _rows(shape, batch=B if batch else None)
    mu_rows, sg_rows = _dev(rows["init_mu_rows"]), _dev(rows["init_sigma_rows"])
    flags = _dev(np.array([3, 0, 1], np.int32), np.int32) if batch else None
    s0 = _dev(_s0s(p) if batch else p["s0"])
    g = lambda k: _lib.ptr(out[k])  # noqa: E731
    outs = [g(k) for k in ("mu", "sigma", "actions", "states", "costs", "weights", "mu_hist", "sigma_hist")]
    if elite:
        ws = ctx.make_ws(lib.mbrl_mppi_elite_workspace_bytes(prob.refs[0], pref, nb))
        tail = (_lib.ptr(ws), ws.numel(), _stream())
        if batch:
            _call("mbrl_mppi_plan_elite_batch",
                  lib.mbrl_mppi_plan_elite_batch(*prob.refs, _lib.ptr(s0), B, pref, _lib.ptr(mu_rows), _lib.ptr(sg_rows),
                                                 _lib.ptr(flags), *outs, g("elites"), *tail))
        else:
            _call("mbrl_mppi_plan_elite",
                  lib.mbrl_mppi_plan_elite(*prob.refs, _lib.ptr(s0), pref, _lib.ptr(mu_rows), _lib.ptr(sg_rows), *outs,
                                           g("elites"), None, *tail))
    elif batch:
        ws = ctx.make_ws(lib.mbrl_mppi_batch_workspace_bytes(prob.refs[0], pref, B))
        _call("mbrl_mppi_plan_batch",
              lib.mbrl_mppi_plan_batch(*prob.refs, _lib.ptr(s0), B, pref, _lib.ptr(mu_rows), _lib.ptr(flags), *outs,
                                       _lib.ptr(ws), ws.numel(), _stream()))
    else:
        ws = ctx.make_ws(lib.mbrl_mppi_workspace_bytes(prob.refs[0], pref))
        _call("mbrl_mppi_plan",
              lib.mbrl_mppi_plan(*prob.refs, _lib.ptr(s0), pref, _lib.ptr(mu_rows), *outs, None, _lib.ptr(ws), ws.numel(),
                                 _stream()))
    return out


_add_plans("mppi_plan", ["mbrl_mppi_plan"], _mppi_plan, PAIRED_SHAPES)
_add_plans("mppi_plan_elite", ["mbrl_mppi_plan_elite"], _mppi_plan, PAIRED_SHAPES[:5], elite=True)
_add_plans("mppi_plan_batch", ["mbrl_mppi_plan_batch"], _mppi_plan, UNPAIRED_SHAPES, batch=True)
_add_plans("mppi_plan_elite_batch", ["mbrl_mppi_plan_elite_batch"], _mppi_plan, UNPAIRED_SHAPES[:3], elite=True, batch=True)


def _mppi_update_elite(ctx, batch, list_in_ws, N=100, K=7, H=3, a=5, E=2):
    """The two-launch update; list_in_ws: elite_idx_out == NULL, so the list lives behind the selection's keys
    (the returned dict then has no `elites`: the ABI gives the caller no array for it)."""
    import torch
    from mbrl_amd import _lib, fused
    lib = _lib.load()
    nb = B if batch else 1
    lead = (B,) if batch else ()
    rng = np.random.default_rng(8)
    costs = _dev(rng.standard_normal((E, nb * N)))
    acts = _dev(rng.uniform(-1, 1, (H, nb * N, a)))
    mu, sg = _dev(rng.uniform(-0.5, 0.5, lead + (H, a))), _dev(rng.uniform(0.1, 0.9, lead + (H, a)))
    sp = fused.make_sampler(31, 1, mu, sg, LO, HI)
    e = ctx.alloc
    out = dict(mu=e(*lead, H, a), sigma=e(*lead, H, a), weights=e(*lead, N), returns=e(*lead, N), stats=e(*lead, 2),
               next_actions=e(H, nb * N, a))
    if not list_in_ws:
        out["elites"] = e(*lead, K, dt=torch.int64)
    need = lib.mbrl_select_workspace_bytes(nb * N) + (((8 * nb * K + 255) // 256) * 256 if list_in_ws else 0)
    ws = ctx.make_ws(need)
    g = lambda k: _lib.ptr(out.get(k))  # noqa: E731
    head = (_lib.ptr(costs), E, N, K)
    mid = (_lib.ptr(acts), ctypes.byref(sp), H, a, 0.7, 0.1, 1, 0.05, 0.8, g("mu"), g("sigma"), g("elites"), g("weights"),
           g("returns"), g("stats"), g("next_actions"))
    if batch:
        _call("mbrl_mppi_update_elite_batch",
              lib.mbrl_mppi_update_elite_batch(*head, B, *mid, _lib.ptr(ws), ws.numel(), _stream()))
    else:
        _call("mbrl_mppi_update_elite", lib.mbrl_mppi_update_elite(*head, *mid, 0, N, _lib.ptr(ws), ws.numel(), _stream()))
    return out


for _batch, _name in ((False, "mbrl_mppi_update_elite"), (True, "mbrl_mppi_update_elite_batch")):
    for _in_ws in (False, True):
        _add(f"{_name[5:]}{'_list_in_ws' if _in_ws else ''}", [_name],
             functools.partial(_mppi_update_elite, batch=_batch, list_in_ws=_in_ws))


# ------------------------------------------------------------------------------------------------ gradient descent
GD = dict(cid=3, over=dict(s=17, a=6, W=64, L=2), H=3)


@functools.lru_cache(maxsize=None)
def gd_problem():
    from oracle import cem as ocem
    from test_gpu_parity import device_problem
    p = ocem.synth_problem(GD["cid"], seed=9200, N=1, H=GD["H"], **GD["over"])
    return p, device_problem(p)


def _gd_inputs(nb):
    p, _ = gd_problem()
    rng = np.random.default_rng(6)
    return _s0s(p, nb)[:nb], rng.uniform(-0.8, 0.8, (nb, GD["H"], GD["over"]["a"])).astype(F32)


def _gd_grad(ctx, nb):
    from test_gpu_gd_grad import grad_call
    S0, A = _gd_inputs(nb)
    states, grad = grad_call(gd_problem()[1], S0, A, make_ws=ctx.make_ws, alloc=ctx.alloc)
    return dict(states=states, grad=grad)


def _gd_plan(ctx, nb, batch):
    """mbrl_gd_plan (nb == 1, batch False) or mbrl_gd_plan_batch: four Adam iterations, no stop test."""
    import torch
    from mbrl_amd import _lib
    lib = _lib.load()
    _, prob = gd_problem()
    S0, A = _gd_inputs(nb)
    H, s, a = GD["H"], GD["over"]["s"], GD["over"]["a"]
    lead = (nb,) if batch else ()
    out = dict(actions=ctx.alloc(*lead, H, a), states=ctx.alloc(*lead, H + 1, s), iterations=ctx.alloc(nb, dt=torch.int32))
    out["actions"].copy_(_dev(A).reshape(out["actions"].shape))     # in: the initial sequences
    s0 = _dev(S0)
    if batch:
        ws = ctx.make_ws(lib.mbrl_gd_batch_workspace_bytes(prob.refs[0], H, nb))
        _call("mbrl_gd_plan_batch",
              lib.mbrl_gd_plan_batch(*prob.refs, _lib.ptr(s0), _lib.ptr(out["actions"]), nb, H, 4, 0.0, 0.01,
                                     _lib.ptr(out["states"]), _lib.ptr(out["iterations"]), _lib.ptr(ws), ws.numel(), _stream()))
    else:
        ws = ctx.make_ws(lib.mbrl_gd_workspace_bytes(prob.refs[0], H))
        _call("mbrl_gd_plan",
              lib.mbrl_gd_plan(*prob.refs, _lib.ptr(s0), _lib.ptr(out["actions"]), H, 4, 0.0, 0.01, _lib.ptr(out["states"]),
                               _lib.ptr(out["iterations"]), _lib.ptr(ws), ws.numel(), _stream()))
    return out


GD_MODES = (("coop", ()), ("single", (("gd_single", 1),)), ("gd_abort", (("debug_gd_abort", 1),)))
for _mode, _opts in GD_MODES:
    _add(f"gd_plan_{_mode}", ["mbrl_gd_plan"], functools.partial(_gd_plan, nb=1, batch=False), _opts)
    for _nb in (1, B):
        _add(f"gd_plan_batch_b{_nb}_{_mode}", ["mbrl_gd_plan_batch"], functools.partial(_gd_plan, nb=_nb, batch=True), _opts)
        _add(f"gd_grad_b{_nb}_{_mode}", ["mbrl_gd_grad"], functools.partial(_gd_grad, nb=_nb), _opts)


# ------------------------------------------------------------------------------------------------ training
TRAIN = dict(s=5, a=2, W=64, horizon=2, batch=130, T=300)
TRAIN_ROWS = 2 * TRAIN["batch"] + 37      # an epoch of three batches, the last one short


def _rehome(mem, alloc):
    """The member's tensors moved into alloc's memory: parameters and Adam state keep their values (in / out),
    the gradients keep alloc's fill (the calls overwrite them)."""
    mem.params = [alloc(*t.shape).copy_(t) for t in mem.params]
    mem.m = [alloc(*t.shape).copy_(t) for t in mem.m]
    mem.v = [alloc(*t.shape).copy_(t) for t in mem.v]
    mem.grads = [alloc(*t.shape) for t in mem.grads]
    return mem


def _train_setup(ctx, L, reward, E):
    import test_gpu_train_ensemble as te
    t = TRAIN
    data = te._Data(t["s"], t["a"], t["horizon"], t["T"], seed=50 + L)
    mems = [_rehome(te._Member(t["s"], t["a"], t["W"], L, reward, t["horizon"], seed=60 + 10 * L + e), ctx.alloc)
            for e in range(E)]
    rng = np.random.default_rng(70 + L)
    idx = rng.integers(0, t["T"], size=(E, t["batch"]), dtype=np.int64)
    orders = rng.integers(0, t["T"], size=(1, E, TRAIN_ROWS), dtype=np.int64)
    return te, data, mems, idx, orders


def _member_out(prefix, mem, out):
    for kind in ("params", "grads", "m", "v"):
        for i, x in enumerate(getattr(mem, kind)):
            out[f"{prefix}{kind}{i}"] = x.clone()


def _train_single(ctx, L, reward, fresh=False):
    """grads, an epoch (three batches, the last short), grads again: on one workspace obtained once, or
    (fresh) a new one per call. Reports every call's outputs and the status word after it."""
    from mbrl_amd import _lib
    lib = _lib.load()
    te, data, (mem,), idx, orders = _train_setup(ctx, L, reward, 1)
    tm = _lib.TrainModel()
    mem.fill(tm)
    batch = TRAIN["batch"]
    at = lib.mbrl_train_status_offset(ctypes.byref(tm), batch)
    held = []

    def make_ws(n):
        if fresh or not held:
            held.append(ctx.make_ws(n))
        assert held[-1].numel() == n
        return held[-1]

    out = {}
    rows = _dev(idx[0], np.int64)
    for step in ("grads1", "epoch", "grads2"):
        if step == "epoch":
            out[f"{step}.losses"] = te._single_epochs(mem, data, orders[:, 0], batch, make_ws=make_ws, alloc=ctx.alloc)[0]
        else:
            out[f"{step}.loss"] = te._grads_single(mem, data, rows, make_ws=make_ws, alloc=ctx.alloc)
        _member_out(f"{step}.", mem, out)
        out[f"{step}.status"] = held[-1][at:at + 4].clone()
    return out


def _train_ensemble(ctx, L, reward, epoch, E=2):
    te, data, mems, idx, orders = _train_setup(ctx, L, reward, E)
    out = {}
    if epoch:
        out["losses"] = te._ensemble_epochs(mems, data, orders, TRAIN["batch"], make_ws=ctx.make_ws, alloc=ctx.alloc)[0]
    else:
        out["loss"] = te._grads_ensemble(mems, data, _dev(idx, np.int64), make_ws=ctx.make_ws, alloc=ctx.alloc)
    for e, mem in enumerate(mems):
        _member_out(f"member{e}.", mem, out)
    return out


for _L, _reward in ((2, 0), (2, 1), (3, 0), (1, 1)):
    _tag = f"l{_L}_{'reward' if _reward else 'state'}"
    _add(f"train_single_{_tag}", ["mbrl_train_grads", "mbrl_train_epoch"],
         functools.partial(_train_single, L=_L, reward=_reward), zeroed_once=True)
    _add(f"train_grads_ensemble_{_tag}", ["mbrl_train_grads_ensemble"],
         functools.partial(_train_ensemble, L=_L, reward=_reward, epoch=False))
    _add(f"train_epoch_ensemble_{_tag}", ["mbrl_train_epoch_ensemble"],
         functools.partial(_train_ensemble, L=_L, reward=_reward, epoch=True))


def entries_covered():
    return {e for c in CASES.values() for e in c.entries}
