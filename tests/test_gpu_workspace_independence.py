"""GPU: no call's result depends on the bytes its workspace held before, and no call writes outside its
workspace or its outputs. The cases are tests/workspace_cases.py's: every exported function with a `void*
workspace`, at the smallest shapes where its workspace-resident machinery (pair flags, hand-off granules,
gates, status words, member scratch, padded partials) is live.

  a. two runs on zero-filled workspaces are byte-equal in every returned array (no entry needed an exception:
     nothing here is compared at a tolerance);
  b. the workspace filled with 0xFF (NaN floats, all-ones flags and epochs), 0xA5 (a negative float), 0x01 (small
     plausible flags, epochs and tickets, a set status bit), 0x7F (another NaN) and the leftovers of the pair
     shape's CEM plan (real high-epoch flags and granules, tiled to the length asked for): every returned array
     byte-equal to the zero-filled run. The single-model training pair is zeroed once by contract: there the
     sequence grads, epoch, grads on one zeroed workspace must equal the same calls on fresh zeroed
     workspaces, with the status word 0 after each;
  c. the workspace is exactly the size query's bytes, starts at a 4096-byte multiple and has 4096 guard bytes
     on each side; every output array lies in the same slab with guard bands around it and is pre-filled with
     a NaN payload no computation produces. After the call every guard byte is intact (this is checked on every
     run of a. and b. too) and no output element keeps the payload (no exception was needed);
  d. the Python planners on cached workspaces (planners._workspace) dirtied with 0xFF before each use, and a
     small plan that reuses the buffer a larger plan of another shape left behind, against clean runs."""
import functools
import threading

import numpy as np
import pytest
import torch

import workspace_cases as wc

pytestmark = pytest.mark.gpu
DEV = wc.DEV
GUARD, BAND = 0xC3, 4096
SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload; as int64 halves or int32 no index or count either
PATTERNS = {"ff": 0xFF, "a5": 0xA5, "01": 0x01, "7f": 0x7F}


class Arena:
    """One device slab starting at a 4096-byte multiple, filled with GUARD; every block taken from it has at
    least BAND guard bytes before it and BAND right behind its last byte."""

    def __init__(self, capacity=48 << 20):
        raw = torch.empty(capacity + 4096, dtype=torch.uint8, device=DEV)
        off = (-raw.data_ptr()) % 4096
        self.slab = raw[off:off + capacity]
        self.pos, self.blocks = 0, []
        self.slab.fill_(GUARD)

    def reset(self):
        if self.blocks:
            self.slab[:self.pos + BAND].fill_(GUARD)
        self.pos, self.blocks = 0, []

    def _take(self, nbytes, align):
        start = (self.pos + BAND + align - 1) // align * align
        assert start + nbytes + BAND <= self.slab.numel(), "arena too small"
        self.blocks.append((start, start + nbytes))
        self.pos = start + nbytes
        block = self.slab[start:start + nbytes]
        assert block.data_ptr() % align == 0
        return block

    def workspace(self, nbytes, fill):
        assert nbytes > 0, "the size query refused the case"
        ws = self._take(nbytes, 4096)
        if isinstance(fill, int):
            ws.fill_(fill)
        else:                                    # leftovers, tiled to the length
            reps = -(-nbytes // fill.numel())
            ws.copy_(fill.repeat(reps)[:nbytes])
        return ws

    def output(self, *shape, dt=torch.float32):
        n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        block = self._take(n, 256)
        block.view(torch.int32).fill_(SENTINEL)
        return block.view(dt).view(*shape)

    def damaged(self):
        """The guard gaps that no longer hold GUARD everywhere: [(gap start, gap end, first bad offset)]."""
        bad, prev = [], 0
        for start, end in self.blocks + [(self.pos + BAND, None)]:
            gap = self.slab[prev:start]
            wrong = (gap != GUARD).nonzero()
            if wrong.numel():
                bad.append((prev, start, int(wrong[0])))
            prev = end
        return bad


@functools.lru_cache(maxsize=None)
def arena():
    return Arena()


def _host(out):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def run_case(name, fill, **kw):
    """The case on workspaces pre-filled with `fill`, outputs in the arena: (host outputs, damaged guard gaps,
    names of the outputs that still hold a sentinel element)."""
    ar = arena()
    ar.reset()
    out = _host(wc.CASES[name].run(lambda n: ar.workspace(n, fill), ar.output, **kw))
    torch.cuda.synchronize()
    stale = [k for k, v in out.items() if v.size and (v.view(np.int32) == np.int32(SENTINEL)).any()]
    return out, ar.damaged(), stale


@functools.lru_cache(maxsize=None)
def zero_run(name):
    """The reference of a case, computed once: the run on zero-filled workspaces."""
    return run_case(name, 0)


@functools.lru_cache(maxsize=None)
def leftovers():
    """What the pair shape's CEM plan leaves in its workspace (pair flags and granules at their last epochs, the
    cooperative trajectory's granules, the proposals)."""
    kept = []

    def make_ws(n):
        kept.append(torch.zeros(n, dtype=torch.uint8, device=DEV))
        return kept[-1]

    wc.CASES["cem_plan_pair"].run(make_ws)
    torch.cuda.synchronize()
    assert len(kept) == 1 and bool(kept[0].any())
    return kept[0]


def assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


FILLED = [n for n, c in wc.CASES.items() if not c.zeroed_once]
ZEROED_ONCE = [n for n, c in wc.CASES.items() if c.zeroed_once]


@pytest.mark.parametrize("name", list(wc.CASES))
def test_a_two_zero_filled_runs_are_byte_equal(name):
    first, _, _ = zero_run(name)
    again, damaged, _ = run_case(name, 0)
    assert not damaged, damaged
    assert_same(again, first, name)
    assert all(np.isfinite(v).all() for v in first.values() if v.dtype == np.float32), name


@pytest.mark.parametrize("pattern", list(PATTERNS) + ["leftovers"])
@pytest.mark.parametrize("name", FILLED)
def test_b_prior_bytes_do_not_reach_the_result(name, pattern):
    want, _, _ = zero_run(name)
    fill = leftovers() if pattern == "leftovers" else PATTERNS[pattern]
    got, damaged, stale = run_case(name, fill)
    assert not damaged, damaged
    assert not stale, stale
    assert_same(got, want, (name, pattern))


@pytest.mark.parametrize("name", ZEROED_ONCE)
def test_b_single_model_training_on_a_workspace_zeroed_once(name):
    """grads, an epoch of three batches (the last short), grads on one zeroed workspace against the same calls
    on freshly zeroed workspaces; the status word stays 0."""
    reused, damaged, stale = zero_run(name)
    fresh, damaged_f, _ = run_case(name, 0, fresh=True)
    assert not damaged and not damaged_f and not stale
    assert_same(reused, fresh, name)
    for step in ("grads1", "epoch", "grads2"):
        assert reused[f"{step}.status"].tobytes() == bytes(4), (name, step)
    assert reused["epoch.losses"].shape == (3, 3)
    assert reused["grads1.params0"].tobytes() != reused["epoch.params0"].tobytes()      # the epoch did train


@pytest.mark.parametrize("name", list(wc.CASES))
def test_c_guard_bands_are_intact_and_every_output_is_written(name):
    _, damaged, stale = zero_run(name)
    assert not damaged, f"{name}: bytes written outside the workspace or an output: {damaged}"
    assert not stale, f"{name}: outputs with elements the call never wrote: {stale}"


def test_c_the_arena_notices_a_stray_byte():
    """The check itself: one byte written right behind a workspace, and one right before an output."""
    ar = Arena(1 << 16)
    ws = ar.workspace(300, 0)
    out = ar.output(5, 3)
    assert ws.data_ptr() % 4096 == 0 and ws.numel() == 300 and not ar.damaged()
    ar.slab[ar.blocks[0][1]] = 0
    assert ar.damaged() == [(ar.blocks[0][1], ar.blocks[1][0], 0)]
    ar.slab[ar.blocks[0][1]] = GUARD
    ar.slab[ar.blocks[1][0] - 1] = 1
    assert len(ar.damaged()) == 1 and bool((out.view(torch.int32) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ d. the Python path
def _closures(shape):
    from test_gpu_parity import build
    p, _ = wc.problem(shape)
    _, model_fn, cost_fn, sample_action = build(p)
    return p, model_fn, cost_fn, sample_action


def _filled_workspaces(monkeypatch, real, value):
    """planners._workspace wrapped: every buffer it hands out is first filled with `value`, all of it."""
    from mbrl_amd import planners
    calls = []

    def filled(key, nbytes, device):
        buf = real(key, nbytes, device)
        buf.fill_(value)
        calls.append(key)
        return buf

    monkeypatch.setattr(planners, "_workspace", filled)
    return calls


def _same_results(got, want, what):
    keys = [k for k in want if torch.is_tensor(want[k])]
    assert keys and set(keys) <= set(got), what
    for k in keys:
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (what, k)


def _python_plans(shape):
    """name -> thunk returning a dict of tensors, each through planners._workspace."""
    from mbrl_amd import CEMPlanner, MPPIPlanner, planners
    p, model_fn, cost_fn, sample_action = _closures(shape)
    N, H, K, s, a, E = wc._dims(shape)
    s0 = torch.from_numpy(p["s0"])
    kw = dict(num_candidates=N, num_iterations=wc.I, seed=p["rng_seed"], record=True, return_device=True)
    rows = wc._rows(shape, keep=3)
    prev = (None, torch.from_numpy(rows["init_mu_rows"]))

    def batch():
        states, actions = CEMPlanner.plan_batch(torch.from_numpy(wc._s0s(p)), model_fn, cost_fn, sample_action, H,
                                                num_candidates=N, num_elites=K, num_iterations=wc.I, seed=p["rng_seed"])
        return dict(states=states, actions=actions)

    def stepwise():
        _, prob = wc.problem(shape)
        st = dict(N=N, K=K, H=H, I=wc.I, E=E, a=a, alpha=0.1, lo=-1.0, hi=1.0, init_std=0.5, seed=p["rng_seed"],
                  record=True, events=None)

        class OneRank(planners._FusedShardOps):
            def all_gather(self, out_flat, local):
                out_flat.copy_(local.reshape(-1))

        ops = OneRank(prob, s0.to(DEV), st)
        ops._fused_update = False                 # select and refit as their own calls, on _sel_ws / _refit_ws
        return planners.cem_sharded_protocol(ops, st, 1, 0)

    return {
        "cem": lambda: CEMPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, num_elites=K, **kw),
        "cem_warm_keep": lambda: CEMPlanner.plan_detailed(
            s0, model_fn, cost_fn, sample_action, H, num_elites=K, initial_trajectory=prev, warm_start=True, keep_elites=3,
            carry=torch.from_numpy(rows["carry_in"]), **kw),
        "cem_batch": batch,
        "mppi": lambda: MPPIPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, temperature=0.7, **kw),
        "mppi_elites": lambda: MPPIPlanner.plan_detailed(s0, model_fn, cost_fn, sample_action, H, temperature=0.7,
                                                         num_elites=K, **kw),
        "stepwise": stepwise,
    }


PYTHON_PLANS = ("cem", "cem_warm_keep", "cem_batch", "mppi", "mppi_elites", "stepwise")


@pytest.mark.parametrize("shape,opts", [("narrow", ()), ("pair", wc.PAIR), ("ens", ())], ids=["narrow", "pair", "ens"])
@pytest.mark.parametrize("which", PYTHON_PLANS)
def test_d_python_planners_on_dirtied_cached_workspaces(which, shape, opts, monkeypatch):
    """The unwrapped call (whatever the cached buffers hold by now), the call on buffers zeroed before each
    use and the call on buffers filled with 0xFF before each use: the same bytes."""
    from contextlib import ExitStack
    from mbrl_amd import _lib, planners
    plans = _python_plans(shape)
    real = planners._workspace
    with ExitStack() as stack:
        for k, v in opts:
            stack.enter_context(_lib.option(k, v))
        plain = plans[which]()
        torch.cuda.synchronize()
        _filled_workspaces(monkeypatch, real, 0)
        clean = plans[which]()
        torch.cuda.synchronize()
        calls = _filled_workspaces(monkeypatch, real, 0xFF)
        dirty = plans[which]()
        torch.cuda.synchronize()
    assert calls, "the plan took no workspace from planners._workspace"
    _same_results(dirty, clean, (which, shape, "0xFF against zeroed"))
    _same_results(plain, clean, (which, shape, "unwrapped against zeroed"))


def _in_fresh_thread(fn):
    """fn() in a new thread (its planners._workspace cache starts empty); its result, or its exception re-raised."""
    box = {}

    def body():
        try:
            box["out"] = fn()
        except BaseException as e:  # noqa: BLE001 (handed to the caller's thread)
            box["err"] = e

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "err" in box:
        raise box["err"]
    return box["out"]


def test_d_a_small_plan_reuses_the_buffer_of_a_larger_plan_of_another_shape():
    """The narrow plan right after the pair-shape plan on one thread's cached buffer (same key, same stream: the
    smaller need is served by the larger buffer, pair flags and granules still in it) against the narrow plan
    run first in a fresh thread. Both run in threads of their own, whose thread-local caches start empty, so
    what earlier tests left in this thread's cache (other streams, other devices' keys) plays no part."""
    from mbrl_amd import CEMPlanner, _lib, planners

    def plan(shape):
        p, model_fn, cost_fn, sample_action = _closures(shape)
        N, H, K, _, _, _ = wc._dims(shape)
        res = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, H, num_candidates=N,
                                       num_elites=K, num_iterations=wc.I, seed=p["rng_seed"], record=True,
                                       return_device=True)
        torch.cuda.synchronize()
        return res

    def cem_buffers():
        return [(v.data_ptr(), v.numel()) for k, v in planners._WS.bufs.items() if k[0] == "cem"]

    def pair_then_narrow():
        assert getattr(planners._WS, "bufs", None) is None          # a fresh thread: nothing cached yet
        with _lib.option("rollout_pair", 1):
            plan("pair")
        big = cem_buffers()
        assert len(big) == 1, big
        reused = plan("narrow")
        assert cem_buffers() == big, (cem_buffers(), big)           # the narrow plan ran in the pair plan's buffer
        return reused, big[0][1]

    def narrow_first():
        first = plan("narrow")
        small = cem_buffers()
        assert len(small) == 1, small
        return first, small[0][1]

    first, small = _in_fresh_thread(narrow_first)
    reused, big = _in_fresh_thread(pair_then_narrow)
    assert small < big, (small, big)                                # a smaller need, served by the larger buffer
    _same_results(reused, first, "narrow after pair")
