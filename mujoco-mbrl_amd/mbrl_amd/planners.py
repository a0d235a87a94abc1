"""Planners with the reference's static `plan()` API (/root/reference/src/mbrl/planners.py:14-25).

    plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs)
        -> (states [H, s], actions [H, a])

The class itself (not an instance) is what agents pass around (experiment.py:15-26, agents.py:48),
kwargs are read as kwargs.get(name, Cls.defaults[name]) (planners.py:141,153-155), and
`initial_trajectory` is accepted and ignored exactly as the reference's random-shooting planner
ignores it (planners.py:166-187).

RandomShootingPlanner -- the reference's planner (planners.py:140-216), same sampling call and
    argmin semantics, rollout + cost + argmin on the GPU.
CEMPlanner            -- the CEM hot path of BASELINE.json: I iterations of
    Philox proposal -> persistent MFMA rollout -> stable top-K -> alpha-smoothed Gaussian refit.
    With torch.distributed initialised and distributed=True, candidates are sharded over ranks:
    one RCCL all-gather of the per-candidate returns per iteration; every rank then runs the same
    deterministic selection and refit (the refit regenerates elite actions from the counter RNG,
    so no moment collective is needed and the result is bit-identical for any rank count).
    noise_beta / noise_mix give the proposals noise correlated along the horizon (colored_noise_mix; the
    third iCEM ingredient), on the receding-horizon path.
RecedingHorizonCEMPlanner -- CEMPlanner with warm start and elite carry-over on by default; its plan_batch
    (mbrl_cem_plan_rh_batch) keeps each problem's kept rows between control steps through memos.
MPPIPlanner           -- CEM's loop with a softmax-weighted refit over every candidate in place of
    the elite cut (mbrl_mppi_plan), warm-started from the previous plan.
BatchedMPPIPlanner    -- MPPIPlanner with a plan_batch (mppi_plan_batch, mbrl_mppi_plan_batch): B warm-started
    plans in shared launches, the class a served policy uses.
GradientDescentPlanner -- the reference's Adam loop on one action sequence (planners.py:28-137).

All four take the fused path when fused.describe_* (gd.describe) recognise the model / cost closures;
otherwise the user's callables run on device tensors (reference semantics, planners.py:199-210), with
selection / refit / the weighted update still in the HIP extension (gradient descent: gd.plan_generic).
What the CEM and MPPI paths share is written once: _common_settings, _plan_params, _layout /
_device_outputs / _stage_in / _stage_out (the one output buffer, on the device or in mapped host
staging), _cem_record_buffers, _mark, _finish and _generic_plan (the loop over opaque callables).
"""
import contextlib
import functools
import threading
import warnings

import numpy as np
import torch

from . import _lib, fused


class ModelPlanner:
    """planners.py:14-25."""

    @staticmethod
    def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        raise NotImplementedError


def _device(kwargs):
    dev = kwargs.get("device")
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("mbrl_amd planners need a ROCm GPU (torch.cuda.is_available() is False)")
        dev = torch.device("cuda", torch.cuda.current_device())
    return torch.device(dev)


_NULL_CTX = contextlib.nullcontext()


def _on_device(dev):
    """torch.cuda.device(dev), or a no-op when dev is already the current device (the common case:
    the context manager's enter and exit are a few microseconds of every plan's host turn)."""
    if dev.index is not None and torch._C._cuda_getDevice() == dev.index:
        return _NULL_CTX
    return torch.cuda.device(dev)


def _to_host(x, keep_device):
    return x if keep_device else x.cpu()


def _finish(res, keep):
    """The tail of plan_detailed: states and actions to the host (unless `keep`), in ONE device-to-host
    copy where the path left them side by side in res["_both"] (_device_outputs)."""
    both = res.pop("_both", None)
    if both is not None and not keep:
        host = both.cpu()
        H, s = res["states"].shape
        res["states"], res["actions"] = host[:H * s].view(H, s), host[H * s:].view(H, -1)
    else:
        res["states"], res["actions"] = _to_host(res["states"], keep), _to_host(res["actions"], keep)
    return res


def _common_settings(defaults, sample_action, horizon, kwargs):
    """What CEMPlanner and MPPIPlanner read alike: bounds (action_bounds, else the sampler's action_spec,
    else (-1, 1)), init_std (default (hi - lo) / 4 in float32), seed (None: ONE draw from the global
    NumPy RNG, like the reference's sampler), alpha, the switches, the timing hooks and the precision."""
    g = lambda k: kwargs.get(k, defaults[k])  # noqa: E731
    bounds = g("action_bounds")
    sdesc = fused.describe_sampler(sample_action) if sample_action is not None else None
    if bounds is None:
        bounds = (sdesc[0], sdesc[1]) if sdesc is not None else (-1.0, 1.0)
    lo, hi = float(bounds[0]), float(bounds[1])
    init_std = g("init_std")
    init_std = float(np.float32(hi - lo) / np.float32(4.0)) if init_std is None else float(init_std)
    seed = g("seed")
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
    return dict(H=int(horizon), alpha=float(g("alpha")), lo=lo, hi=hi, init_std=init_std, seed=seed,
                keep=bool(g("return_device")), record=bool(kwargs.get("record", False)),
                events=kwargs.get("rollout_events"), plan_events=kwargs.get("plan_events"),
                adim=sdesc[2] if sdesc else None, precision=_lib.precision_code(g("precision")))


def _generic_costs(model, cost, s0, actions, H, N):
    """planners.py:199-210 with the caller's callables. actions [H, N, a] on the GPU.

    The callables are opaque: they run on GPU tensors when they accept them, else (their own
    parameters live on the host, e.g. a cost closing over CPU goal tensors as the reference's
    agents build them) on host copies of the inputs. Returns costs [1, N] (sequential sum over t)
    and states [H, N, s] on the GPU; selection and refit stay in the HIP extension."""
    dev = actions.device
    s = s0.shape[0]

    def call(fn, *args):
        try:
            return fn(*args).to(dev)
        except RuntimeError as e:
            if "device" not in str(e):
                raise
            return fn(*[x.cpu() for x in args]).to(dev)

    states = torch.empty((H, N, s), dtype=torch.float32, device=dev)
    cur = s0.unsqueeze(0).repeat_interleave(N, dim=0)
    with torch.no_grad():
        for t in range(H):
            cur = call(model, cur, actions[t])
            states[t] = cur
        c = call(cost, states.reshape(H * N, s), actions.reshape(H * N, -1)).reshape(H, N)
        total = c[0].clone()
        for t in range(1, H):
            total = total + c[t]
    return total.reshape(1, N).contiguous(), states


class GradientDescentPlanner(ModelPlanner):
    """planners.py:28-137: Adam(lr=0.01) on one action sequence through the learned dynamics, on the
    GPU for recognised closures (mbrl_amd/gd.py), else the reference's loop on the given callables.
    Returns lists of H+1 states [1, s] and H actions [1, a], as the reference does."""
    defaults = dict(num_iterations=40, stop_condition=0.002)
    # plans start from the previous plan of the same episode (MPCPolicy's initial_trajectory,
    # agents.py:40-55): the planner service passes those to plan_batch (parallel._answer)
    warm_starts = True

    @staticmethod
    def _setup(model, cost, kwargs):
        """The kwargs, and gd.describe's view of the closures (None without a GPU or when not recognised)."""
        from . import gd
        d = GradientDescentPlanner.defaults
        num_iterations = int(kwargs.get("num_iterations", d["num_iterations"]))
        stop_condition = float(kwargs.get("stop_condition", d["stop_condition"]))
        dev = mdesc = cdesc = None
        if torch.cuda.is_available():
            dev = _device(kwargs)
            mdesc, cdesc = gd.describe(model, cost, dev)
        return gd, num_iterations, stop_condition, dev, mdesc, cdesc

    @staticmethod
    def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        gd, num_iterations, stop_condition, dev, mdesc, cdesc = GradientDescentPlanner._setup(model, cost, kwargs)
        H = int(horizon)
        if mdesc is not None:
            if initial_trajectory is None:
                # planners.py:94: the nominal sequence (its states are not used for a deterministic model)
                action_list = list(sample_action(batch_size=H).split(1, dim=0))
            else:
                action_list = initial_trajectory[1]
            with torch.cuda.device(dev):
                states, actions = gd.plan_device(initial_state, mdesc, cdesc, action_list, H, num_iterations,
                                                 stop_condition, dev)
        else:
            states, actions = gd.plan_generic(initial_state, model, cost, sample_action, H, initial_trajectory,
                                              num_iterations, stop_condition)
        keep = kwargs.get("return_device", False)
        states, actions = _to_host(states, keep), _to_host(actions, keep)
        return list(states.split(1, 0)), list(actions.split(1, 0))

    @staticmethod
    def plan_batch(initial_states, model, cost, sample_action, horizon, initial_trajectories=None, **kwargs):
        """B independent plans, one per row of initial_states [B, s] (parallel environments), each
        what plan() returns for that row. Row b starts from initial_trajectories[b][1] or, where that
        (or the whole list) is None, from sample_action(batch_size=horizon), drawn in row order (as
        B plan() calls would draw). Recognised closures run in shared launches (mbrl_gd_plan_batch: the
        cooperative grids of up to 256 / (Wpad / 16) plans at once); others run plan() per row.
        Returns (states [B, H+1, s], actions [B, H, a])."""
        gd, num_iterations, stop_condition, dev, mdesc, cdesc = GradientDescentPlanner._setup(model, cost, kwargs)
        H, B = int(horizon), int(initial_states.shape[0])
        inits = [None if initial_trajectories is None else initial_trajectories[b] for b in range(B)]
        keep = kwargs.get("return_device", False)
        if mdesc is not None and gd.fused_supported(mdesc, cdesc, dev) and num_iterations > 0:
            starts = [torch.cat(list(sample_action(batch_size=H).split(1, dim=0)), 0) if init is None
                      else torch.cat([x.reshape(1, -1) for x in init[1]], 0) for init in inits]
            with torch.cuda.device(dev):
                states, actions, _ = gd.plan_fused_batch(initial_states, mdesc, cdesc, torch.stack(starts), H,
                                                         num_iterations, stop_condition, dev)
            return _to_host(states, keep), _to_host(actions, keep)
        # per row, in row order; a row without a warm start draws its sequence inside its own plan(),
        # so a model that uses torch's RNG sees exactly the stream of B plan() calls
        outs = [GradientDescentPlanner.plan(initial_states[b], model, cost, sample_action, H,
                                            initial_trajectory=None if inits[b] is None else (None, list(inits[b][1])),
                                            **dict(kwargs, return_device=True)) for b in range(B)]
        states = torch.stack([torch.cat(o[0], 0).reshape(H + 1, -1) for o in outs])
        actions = torch.stack([torch.cat(o[1], 0).reshape(H, -1) for o in outs])
        return _to_host(states, keep), _to_host(actions, keep)


def _rs_host(initial_state, model, cost, sample_action, H, N):
    """RandomShootingPlanner on a host without a GPU (BASELINE configs[0]: the reference's own CPU
    random-shooting path): the reference's a2 loop on the caller's callables, as written
    (/root/reference/src/mbrl/planners.py:189-216: one sample_action(N * H) draw, time-major rows
    t * N + n, H model calls, one cost call, view(H, N).sum(0)), then np.argmin (first index on ties,
    :184). Returns (states [H, s], actions [H, a]) of the chosen candidate."""
    s = initial_state.shape[0]
    with torch.no_grad():
        state_list = torch.zeros((N * H, s))
        action_list = sample_action(batch_size=N * H)
        for t in range(H):
            states = (initial_state.unsqueeze(dim=0).repeat_interleave(N, dim=0) if t == 0
                      else state_list[(t - 1) * N:t * N])
            state_list[t * N:(t + 1) * N] = model(states, action_list[t * N:(t + 1) * N])
        costs = cost(state_list, action_list).view(H, N).sum(0).detach().numpy()
    i = int(np.argmin(costs))
    return state_list.view(H, N, -1)[:, i], action_list.view(H, N, -1)[:, i]


class RandomShootingPlanner(ModelPlanner):
    """planners.py:140-216 on the GPU; on a host without one (torch.cuda.is_available() False), the
    reference's own CPU loop on the given callables (_rs_host: BASELINE configs[0] is this planner on
    CPU). With a GPU the HIP path always runs (and raises if the extension is missing)."""
    defaults = dict(num_trajectories=1000)

    @staticmethod
    def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        _noise_refuse(kwargs, "RandomShootingPlanner")
        kw = dict(kwargs)
        num_trajectories = kw.pop("num_trajectories", RandomShootingPlanner.defaults["num_trajectories"])
        return RandomShootingPlanner._plan(initial_state, model, cost, sample_action, horizon, initial_trajectory,
                                           num_trajectories, **kw)

    @staticmethod
    def _plan(initial_state, model, cost, sample_action, horizon, initial_trajectory, num_trajectories, **kwargs):
        N, H = int(num_trajectories), int(horizon)
        if kwargs.get("device") is None and not torch.cuda.is_available():
            return _rs_host(initial_state, model, cost, sample_action, H, N)
        dev = _device(kwargs)
        # planners.py:200: one draw of N*H actions from the caller's sampler (host RNG), time-major
        action_list = sample_action(batch_size=N * H)
        a = action_list.shape[1]
        with torch.cuda.device(dev):
            acts = action_list.to(device=dev, dtype=torch.float32).reshape(H, N, a).contiguous()
            s0 = initial_state.to(device=dev, dtype=torch.float32).contiguous()
            mdesc, cdesc, prob = fused.describe_problem(model, cost, dev,
                                                        _lib.precision_code(kwargs.get("precision", "f32")))
            if mdesc is not None and cdesc is not None and mdesc["E"] == 1 and mdesc["a"] == a:
                states = torch.empty((1, H, N, mdesc["s"]), dtype=torch.float32, device=dev)
                costs = fused.rollout(prob, s0, N, H, actions=acts, states_out=states)
                states = states[0]
            else:
                costs, states = _generic_costs(model, cost, s0, acts, H, N)
            idx = fused.select(costs, 1, nan_policy=_lib.MBRL_NAN_FIRST)   # np.argmin, planners.py:184
            i = idx[0]
            out_states = states[:, i]
            out_actions = acts[:, i]
            keep = kwargs.get("return_device", False)
            return _to_host(out_states, keep), _to_host(out_actions, keep)


    @staticmethod
    def plan_batch(initial_states, model, cost, sample_action, horizon, **kwargs):
        """B plans, one per row of initial_states [B, s] (parallel environments), each what plan()
        returns for that row: row b's N x H proposals are the b-th sample_action(batch_size=N*H)
        draw (row order, as B plan() calls would draw). Recognised closures roll all B*N candidates
        out in one launch (per-candidate start states), then take each row's np.argmin.
        Returns (states [B, H, s], actions [B, H, a])."""
        _noise_refuse(kwargs, "RandomShootingPlanner.plan_batch")
        kw = dict(kwargs)
        N = int(kw.pop("num_trajectories", RandomShootingPlanner.defaults["num_trajectories"]))
        H, B = int(horizon), int(initial_states.shape[0])
        keep = kw.get("return_device", False)
        dev = _device(kw)
        with torch.cuda.device(dev):
            mdesc, cdesc = fused.describe(model, cost, dev)
            fusable = mdesc is not None and cdesc is not None and mdesc["E"] == 1
            # recognised closures use no RNG, so all B draws can come first; unrecognised ones (a model
            # may draw from torch's RNG) interleave each row's draw with its plan, as B plan() calls do
            draws = [sample_action(batch_size=N * H) for _ in range(B)] if fusable else None
            if not fusable or mdesc["a"] != draws[0].shape[1]:
                outs = []
                for b in range(B):
                    sampler = sample_action
                    if draws is not None:
                        it = iter([draws[b]])
                        sampler = lambda batch_size, it=it: next(it)  # noqa: E731
                    outs.append(RandomShootingPlanner._plan(initial_states[b], model, cost, sampler, H, None, N,
                                                            **dict(kw, return_device=True)))
                return (_to_host(torch.stack([o[0] for o in outs]), keep),
                        _to_host(torch.stack([o[1] for o in outs]), keep))
            a = draws[0].shape[1]
            prob = fused.device_problem(mdesc, cdesc, dev, _lib.precision_code(kw.get("precision", "f32")))
            acts = torch.cat([d.to(device=dev, dtype=torch.float32).reshape(H, N, a) for d in draws], 1).contiguous()
            s0 = initial_states.to(device=dev, dtype=torch.float32).reshape(B, 1, -1).expand(B, N, -1)
            s0 = s0.reshape(B * N, -1).contiguous()
            states = torch.empty((1, H, B * N, mdesc["s"]), dtype=torch.float32, device=dev)
            costs = fused.rollout(prob, s0, B * N, H, actions=acts, s0_per_candidate=True, states_out=states)
            best = torch.stack([fused.select(costs[:, b * N:(b + 1) * N].contiguous(), 1,
                                             nan_policy=_lib.MBRL_NAN_FIRST)[0] for b in range(B)])  # np.argmin
            cols = best + torch.arange(B, device=dev) * N
            out_states = states[0][:, cols].transpose(0, 1)
            out_actions = acts[:, cols].transpose(0, 1)
            return _to_host(out_states.contiguous(), keep), _to_host(out_actions.contiguous(), keep)


class CEMPlanner(ModelPlanner):
    """Cross-entropy method over action sequences (not in the reference).

    kwargs (defaults): num_candidates (1000), num_elites (None -> num_candidates // 10),
    num_iterations (5), alpha (0.1), seed (None -> drawn from the global NumPy RNG, like the
    reference's sampler), init_std (None -> (hi - lo) / 4), action_bounds (None -> from
    sample_action's action_spec, else (-1, 1)), distributed (False), return_device (False),
    precision ("f32": exact fp32 MFMA; "f16x6" / "f16x3": fp32 emulated on the f16 matrix cores
    with 33 / 22 significant operand bits, see include/mbrl_cem.h). Timing hooks (bench.py):
    rollout_events (per-iteration event pairs around the rollout launch), plan_events (one pair
    recorded on the plan's stream just before and just after the C call that enqueues the plan).
    Returns the final Gaussian mean (clipped) and its predicted states (ensemble mean).

    Receding horizon (mbrl_cem_plan_rh; the two iCEM ingredients, all off by default -- the defaults plan
    exactly as above, bit for bit):
    warm_start (False): honour `initial_trajectory` -- its action rows after dropping the first `shift`
        (1) and repeating the last to keep `horizon` rows, clipped to the bounds, are the initial mean
        (mppi_warm_start_rows), so MPCPolicy(..., warm_start=True) plans from the previous plan's tail.
    warm_std (None): the initial std of a warm-started plan. None: init_std on every row; a float: that
        value; "keep": the previous plan's sigma shifted like the mean, given as plan_detailed(...,
        prev_sigma=) (every entry finite and > 0, checked here on the host: the C call cannot).
    keep_elites (0): Kc, the best rows kept from each iteration into the next one's candidate slots
        [0, Kc) -- an int, or a float in (0, 1) as a fraction of num_elites (rounded down, at least 1).
    carry (None): a [Kc, H, a] tensor, the previous plan's result["carry"] shifted (cem_shift_carry), which
        fills those slots in iteration 0.
    With keep_elites > 0 plan_detailed also returns carry [Kc, H, a] and carry_returns [Kc] (record=True:
    kept_hist [I + 1, Kc, H, a]; record=True also returns the rows a warm-started plan began from as
    init_mu / init_sigma). These kwargs raise NotImplementedError with distributed=True, in
    plan_batch and with callables the fused path does not recognise. B such plans at once, each with its own
    warm start and carry: cem_plan_batch_rh and RecedingHorizonCEMPlanner.plan_batch.

    Coloured noise (mbrl_cem_plan_rh_mixed; the third iCEM ingredient, off by default): the proposal noise of a
    candidate is correlated along the horizon instead of white.
    noise_beta (0.0): the exponent of the noise's power-law spectrum, in [0, 4] (colored_noise_mix(horizon,
        beta); 0 is white and passes no matrix at all: the existing plan, bit for bit).
    noise_mix (None): an explicit [horizon, horizon] mixing matrix instead (any temporal correlation; rows of
        unit norm keep sigma's meaning). Every entry finite, checked on the host. Naming both raises ValueError.
    Either routes the plan to the receding-horizon path (the unfused update), with or without a warm start
    or kept rows; horizon <= 64. The same refusals as the receding-horizon kwargs apply, and MPPIPlanner and
    RandomShootingPlanner refuse them too.

    Trajectory sampling (mbrl_cem_plan_ts; PETS' TS-inf, off by default): every candidate is rolled out as
    `particles` sampled particles per ensemble member and scored by the mean over all of them.
    particles (0): P. 0 is the plan above, byte for byte. P >= 1 needs an EnsembleModel of ProbabilisticModels
        with equal log-variance bounds on the fused path and the goal-state cost; each particle stays on its
        member and draws every next state from the member's predicted Gaussian (include/mbrl_cem.h).
    particle_noise (1.0): the factor on the predicted standard deviation (0: the mean rollout on every particle).
    particle_seed (None -> derived from seed): the key of the particles' noise.
    plan_detailed(record=True) returns costs as [I, E * P, N]. The final predicted states stay the deterministic
    member mean of the final actions. A negative value raises ValueError; with particles >= 1, distributed=True,
    plan_batch, the receding-horizon and coloured-noise kwargs, a precision other than "f32", a CPU device and
    callables or models the fused path does not recognise raise NotImplementedError."""
    defaults = dict(num_candidates=1000, num_elites=None, num_iterations=5, alpha=0.1, seed=None, init_std=None,
                    action_bounds=None, distributed=False, return_device=False, precision="f32",
                    warm_start=False, shift=1, warm_std=None, keep_elites=0, carry=None, noise_beta=0.0,
                    noise_mix=None, particles=0, particle_noise=1.0, particle_seed=None)

    @staticmethod
    def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        res = CEMPlanner.plan_detailed(initial_state, model, cost, sample_action, horizon, initial_trajectory,
                                       **kwargs)
        return res["states"], res["actions"]

    @staticmethod
    def plan_batch(initial_states, model, cost, sample_action, horizon, **kwargs):
        """B plans at once, one per row of initial_states [B, s] (see cem_plan_batch)."""
        _rh_refuse(kwargs, "CEMPlanner.plan_batch")
        _noise_refuse(kwargs, "CEMPlanner.plan_batch")
        _ts_refuse(kwargs, "CEMPlanner.plan_batch")
        return cem_plan_batch(initial_states, model, cost, sample_action, horizon, **kwargs)

    _SETTINGS = {}
    _HOOKS = ("rollout_events", "plan_events", "carry", "prev_sigma", "noise_mix")   # per-plan values: not settings

    @staticmethod
    def _settings(sample_action, horizon, kwargs):
        """The plan's settings; with an explicit seed the dict is built once per (sampler, horizon,
        kwargs) and reused (part of every plan's host turn). The timing hooks (fresh lists per plan in
        bench.py) stay out of the key and are set on a copy."""
        if kwargs.get("seed") is not None:
            try:
                key = (id(sample_action), horizon,
                       tuple((k, v) for k, v in kwargs.items() if k not in CEMPlanner._HOOKS))
                hit = CEMPlanner._SETTINGS.get(key)
            except TypeError:          # an unhashable kwargs value: no caching
                key, hit = None, None
            if hit is None or hit[0] is not sample_action:
                hit = (sample_action, CEMPlanner._settings_build(sample_action, horizon, kwargs))
                if key is not None:
                    if len(CEMPlanner._SETTINGS) > 64:
                        CEMPlanner._SETTINGS.clear()
                    CEMPlanner._SETTINGS[key] = hit
            st = hit[1]
            ev, pev = kwargs.get("rollout_events"), kwargs.get("plan_events")
            if ev is not st["events"] or pev is not st["plan_events"]:
                st = dict(st, events=ev, plan_events=pev)
            return st
        return CEMPlanner._settings_build(sample_action, horizon, kwargs)

    @staticmethod
    def _settings_build(sample_action, horizon, kwargs):
        d = CEMPlanner.defaults
        g = lambda k: kwargs.get(k, d[k])  # noqa: E731
        N = int(g("num_candidates"))
        K = g("num_elites")
        K = max(1, N // 10) if K is None else int(K)
        st = _common_settings(d, sample_action, horizon, kwargs)
        if not 1 <= K <= N:
            raise ValueError(f"need 1 <= num_elites ({K}) <= num_candidates ({N})")
        st.update(N=N, K=K, I=int(g("num_iterations")), distributed=bool(g("distributed")))
        return st

    @staticmethod
    def plan_detailed(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        """plan() plus diagnostics: dict(states, actions, mu, sigma[, costs, returns, elites per iteration]
        [, carry, carry_returns[, kept_hist]])."""
        # (a plan that names no particle kwarg takes the paths below with nothing added to its host turn)
        ts = _ts_inputs(kwargs) if any(k in kwargs for k in _TS_KWARGS) else None
        if kwargs.get("distributed", False):
            _rh_refuse(kwargs, "CEMPlanner with distributed=True")   # (before anything needs a device)
            _noise_refuse(kwargs, "CEMPlanner with distributed=True")
        noise = _noise_inputs(kwargs, int(horizon)) if any(k in kwargs for k in _NOISE_KWARGS) else None
        dev = _device(kwargs)
        st = CEMPlanner._settings(sample_action, horizon, kwargs)
        # (the settings dict does not carry the receding-horizon kwargs: a plan that names none of them
        # takes the plain path with nothing added to its host turn)
        rh = _rh_inputs(st, initial_trajectory, kwargs) if any(k in kwargs for k in _RH_KWARGS) else None
        rh = _rh_with_noise(rh, noise)
        with _on_device(dev):
            mdesc, cdesc, prob = fused.describe_problem(model, cost, dev, st["precision"])
            ws = None
            if st["distributed"] and torch.distributed.is_available() and torch.distributed.is_initialized() \
                    and torch.distributed.get_world_size() > 1:
                ws = torch.distributed.get_world_size()
            if rh is not None and (mdesc is None or cdesc is None):
                _rh_refuse(kwargs, "CEMPlanner with callables the fused path does not recognise")
                _noise_refuse(kwargs, "CEMPlanner with callables the fused path does not recognise")
            if ts is not None and (mdesc is None or cdesc is None):
                raise NotImplementedError(f"CEMPlanner with callables the fused path does not recognise: particles="
                                          f"{ts['P']} is not implemented (trajectory sampling runs on the fused path)")
            if mdesc is not None and cdesc is not None:
                if ts is not None:
                    res = _cem_fused_ts(prob, initial_state, st, ts)
                elif rh is not None:
                    res = _cem_fused_rh(prob, initial_state, st, rh)
                elif ws is None:
                    res = _cem_fused_single(prob, initial_state, st)
                else:
                    res = _cem_fused_sharded(prob, initial_state, st, ws)
                if res.pop("_host", False):      # host staging: the results are host tensors already
                    return res
            else:
                a = st["adim"]
                if a is None:
                    a = sample_action(batch_size=1).shape[1]
                res = _cem_generic(model, cost, initial_state.to(device=dev, dtype=torch.float32).contiguous(), st,
                                   a, dev)
            return _finish(res, st["keep"])


_RH_KWARGS = ("warm_start", "warm_std", "keep_elites", "carry")


def _rh_refuse(kwargs, where):
    """NotImplementedError naming the first receding-horizon kwarg that is switched on: `where` (sharded
    plans, the plain batched entries, the generic path) has no receding-horizon form."""
    d = CEMPlanner.defaults
    for k in _RH_KWARGS:
        v = kwargs.get(k, d[k])
        if v is not None and v is not False and not (k == "keep_elites" and not isinstance(v, bool) and v == 0):
            raise NotImplementedError(f"{where}: {k}={v!r} is not implemented (receding-horizon CEM plans are "
                                      "single-GPU, fused-path plans; batched: cem_plan_batch_rh)")


_TS_KWARGS = ("particles", "particle_noise", "particle_seed")


def _ts_values(kwargs):
    """(particles, particle_noise, particle_seed) of kwargs, checked: ValueError for a negative, fractional or
    non-finite value, before any work."""
    d = CEMPlanner.defaults
    P, noise, seed = (kwargs.get(k, d[k]) for k in _TS_KWARGS)
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or P < 0:
        raise ValueError(f"particles={P!r}: need an integer >= 0")
    if isinstance(noise, bool) or not np.isfinite(noise) or noise < 0:
        raise ValueError(f"particle_noise={noise!r}: need a finite number >= 0")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0):
        raise ValueError(f"particle_seed={seed!r}: need None or an integer >= 0")
    return int(P), float(noise), None if seed is None else int(seed)


def _ts_refuse(kwargs, where):
    """NotImplementedError naming `particles` where it is switched on: `where` has no trajectory-sampling form."""
    if any(k in kwargs for k in _TS_KWARGS):
        P = _ts_values(kwargs)[0]
        if P >= 1:
            raise NotImplementedError(f"{where}: particles={P} is not implemented (trajectory-sampling CEM plans "
                                      "are single-GPU, single-problem, fused-path plans: CEMPlanner.plan)")


def _ts_inputs(kwargs):
    """The checked particle kwargs of CEMPlanner.plan_detailed as dict(P, noise, seed), or None with particles=0
    (today's plan). With P >= 1, every kwarg the sampled plan has no form for raises NotImplementedError naming it,
    before anything needs a device."""
    P, noise, seed = _ts_values(kwargs)
    if P == 0:
        return None
    where = f"CEMPlanner with particles={P}"
    if kwargs.get("distributed", False):
        raise NotImplementedError(f"{where}: distributed=True is not implemented")
    _rh_refuse(kwargs, where)
    _noise_refuse(kwargs, where)
    precision = kwargs.get("precision", CEMPlanner.defaults["precision"])
    if precision != "f32":
        raise NotImplementedError(f"{where}: precision={precision!r} is not implemented (the sampled rollout is fp32)")
    dev = kwargs.get("device")
    if dev is not None and torch.device(dev).type != "cuda":
        raise NotImplementedError(f"{where}: device={str(dev)!r} is not implemented (the sampled rollout is a HIP "
                                  "kernel)")
    return dict(P=P, noise=noise, seed=seed)


def _ts_seed(seed):
    """particle_seed=None: a key derived from the plan's seed (splitmix64's first output), so that the particles'
    noise is not the proposals' Philox stream."""
    m = (1 << 64) - 1
    z = (int(seed) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


_NOISE_KWARGS = ("noise_beta", "noise_mix")
NOISE_MAX_H = 64    # include/mbrl_cem.h: a mix with a longer horizon is MBRL_EUNSUPPORTED


def _noise_refuse(kwargs, where):
    """NotImplementedError naming the coloured-noise kwarg that is switched on: `where` has no coloured form."""
    beta, mix = kwargs.get("noise_beta", 0.0), kwargs.get("noise_mix")
    for k, v, on in (("noise_beta", beta, beta is not None and beta != 0), ("noise_mix", mix, mix is not None)):
        if on:
            shown = f"array{tuple(np.shape(v))}" if k == "noise_mix" else repr(v)
            raise NotImplementedError(f"{where}: {k}={shown} is not implemented (coloured-noise proposals are "
                                      "single-GPU, fused-path receding-horizon CEM plans: CEMPlanner.plan, "
                                      "cem_plan_batch_rh)")


def colored_noise_mix(H, beta):
    """The [H, H] float32 matrix that turns H white normals into noise with a power-law spectrum
    S(f) ~ f^(-beta) along the horizon: colorednoise.powerlaw_psd_gaussian's synthesis (Timmer & Koenig 1995)
    written as a matrix, built in float64. Frequencies f_k = k / H, k = 1 .. H // 2, scales s_k = f_k^(-beta / 2)
    and s_0 = s_1; column 0 is sqrt(2) s_0, columns 2k - 1 / 2k are 2 s_k cos / -2 s_k sin of 2 pi k t / H for
    k < ceil(H / 2), and an even H's last column is sqrt(2) s_{H/2} (-1)^t. One scalar then gives every row unit
    Euclidean norm, the DC term included (colorednoise leaves it out), so each step's noise is marginally
    N(0, 1) and sigma keeps its meaning. beta = 0 is an orthogonal matrix (white noise); H = 1 is [[1]]."""
    H, beta = int(H), float(beta)
    if H < 1:
        raise ValueError(f"colored_noise_mix: H={H} must be >= 1")
    if not (np.isfinite(beta) and 0.0 <= beta <= 4.0):
        raise ValueError(f"colored_noise_mix: beta must be finite and in [0, 4], got {beta}")
    if H == 1:
        return np.ones((1, 1), np.float32)
    return _colored_noise_mix64(H, beta).astype(np.float32)


def _colored_noise_mix64(H, beta):
    """colored_noise_mix before the cast (float64; H >= 2)."""
    t = np.arange(H, dtype=np.float64)
    k = np.arange(1, H // 2 + 1, dtype=np.float64)
    s = np.concatenate([[0.0], (k / H) ** (-beta / 2.0)])
    s[0] = s[1]
    C = np.zeros((H, H), np.float64)
    C[:, 0] = np.sqrt(2.0) * s[0]
    for kk in range(1, (H + 1) // 2):
        C[:, 2 * kk - 1] = 2.0 * s[kk] * np.cos(2.0 * np.pi * kk * t / H)
        C[:, 2 * kk] = -2.0 * s[kk] * np.sin(2.0 * np.pi * kk * t / H)
    if H % 2 == 0:
        C[:, H - 1] = np.sqrt(2.0) * s[H // 2] * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    norms = np.sqrt((C * C).sum(1))
    assert np.allclose(norms, norms[0], rtol=1e-12, atol=0.0), "colored_noise_mix: rows of unequal norm"
    return C / norms[0]


def _noise_inputs(kwargs, H):
    """The noise mix of a plan with these kwargs (host only): None for white noise (noise_beta == 0 and no
    matrix), else (key, matrix) -- float32 [H, H], C-contiguous, every entry finite -- with `key` what the
    device copy is cached under (the exponent, or the matrix's bytes)."""
    beta, mix = kwargs.get("noise_beta", 0.0), kwargs.get("noise_mix")
    beta = 0.0 if beta is None else float(beta)
    if mix is not None and beta != 0.0:
        raise ValueError("give noise_beta or noise_mix, not both")
    if mix is None:
        if not (np.isfinite(beta) and 0.0 <= beta <= 4.0):
            raise ValueError(f"noise_beta must be finite and in [0, 4], got {beta}")
        if beta == 0.0:
            return None
        _noise_horizon(H)
        return _beta_noise(H, beta)
    m = mix.detach().cpu().numpy() if isinstance(mix, torch.Tensor) else np.asarray(mix)
    if m.shape != (H, H):
        raise ValueError(f"noise_mix must be [horizon={H}, horizon={H}], got {m.shape}")
    m = np.ascontiguousarray(m, dtype=np.float32)
    if not np.isfinite(m).all():
        raise ValueError("noise_mix must be finite")
    _noise_horizon(H)
    return ("mix", H, m.tobytes()), m


@functools.lru_cache(maxsize=16)
def _beta_noise(H, beta):
    """_noise_inputs' answer for a power-law mix, built once per (H, beta): the matrix is read-only."""
    m = colored_noise_mix(H, beta)
    m.setflags(write=False)
    return ("beta", H, beta), m


def _noise_horizon(H):
    if H > NOISE_MAX_H:
        raise ValueError(f"coloured-noise proposals need horizon <= {NOISE_MAX_H}, got {H}")


def _rh_with_noise(rh, noise):
    """The receding-horizon inputs of a plan (or None) with its noise mix (or None): a mix alone still takes
    the receding-horizon path, with no rows and nothing kept."""
    if noise is None:
        return rh
    if rh is None:
        rh = dict(mu_rows=None, sigma_rows=None, carry=None, Kc=0)
    return dict(rh, mix=noise)


_MIX_DEVICE = {}


def _noise_mix_device(noise, dev):
    """The device copy of a plan's noise mix (_noise_inputs), kept per (matrix, device)."""
    key = noise[0] + (str(dev),)
    hit = _MIX_DEVICE.get(key)
    if hit is None:
        if len(_MIX_DEVICE) > 16:
            _MIX_DEVICE.clear()
        hit = _MIX_DEVICE[key] = torch.from_numpy(noise[1].copy()).to(dev)   # (a cached matrix is read-only)
    return hit


def _rh_settings(kwargs, K):
    """The receding-horizon settings of a plan with K elites: warm_start, shift, warm_std (None, a float > 0
    or "keep") and Kc, keep_elites resolved to a count in [0, K]."""
    d = CEMPlanner.defaults
    g = lambda k: kwargs.get(k, d[k])  # noqa: E731
    ke = g("keep_elites")
    if isinstance(ke, bool) or ke is None:
        raise ValueError(f"keep_elites must be a count or a fraction in (0, 1), got {ke!r}")
    if isinstance(ke, float) and not ke.is_integer():
        if not 0.0 < ke < 1.0:
            raise ValueError(f"a fractional keep_elites must lie in (0, 1), got {ke}")
        Kc = max(1, int(ke * K))
    else:
        Kc = int(ke)
    if not 0 <= Kc <= K:
        raise ValueError(f"need 0 <= keep_elites ({Kc}) <= num_elites ({K})")
    warm_std = g("warm_std")
    if warm_std is not None and warm_std != "keep":
        warm_std = float(warm_std)
        if not (warm_std > 0.0 and np.isfinite(warm_std)):
            raise ValueError(f"warm_std must be finite and > 0, got {warm_std}")
    shift = int(g("shift"))
    if shift < 0:
        raise ValueError(f"shift must be >= 0, got {shift}")
    return dict(warm_start=bool(g("warm_start")), shift=shift, warm_std=warm_std, Kc=Kc)


def cem_shift_carry(carry, shift, lo=-1.0, hi=1.0):
    """The kept rows of one plan ([Kc, H, a], its result["carry"]) as the next control step's `carry`: what
    mppi_warm_start_rows does to the mean, for every kept row -- the first `shift` steps dropped, the last
    step repeated to keep H, clipped to [lo, hi]. Host only; float32 [Kc, H, a]."""
    x = carry.detach().cpu().numpy() if isinstance(carry, torch.Tensor) else np.asarray(carry)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 3:
        raise ValueError(f"carry must be [Kc, H, a], got shape {x.shape}")
    H = x.shape[1]
    if x.shape[0] == 0:
        return x.copy()
    return np.stack([mppi_warm_start_rows(row, H, shift, lo, hi) for row in x])


def _rh_inputs(st, initial_trajectory, kwargs):
    """The receding-horizon inputs of one plan as host arrays, dict(mu_rows, sigma_rows, carry) with None for
    what is absent, and Kc -- or None when nothing is switched on (the plan then takes the plain path untouched)."""
    rs = _rh_settings(kwargs, st["K"])
    H, Kc = st["H"], rs["Kc"]
    carry = kwargs.get("carry")
    if carry is not None and Kc == 0:
        raise ValueError("carry given with keep_elites == 0")
    rows = sig = None
    if rs["warm_start"] and initial_trajectory is not None:
        rows = mppi_warm_start_rows(initial_trajectory[1], H, rs["shift"], st["lo"], st["hi"])
        ws = rs["warm_std"]
        if ws == "keep":
            prev = kwargs.get("prev_sigma")
            if prev is None:
                raise ValueError('warm_std="keep" needs the previous plan\'s sigma: plan_detailed(..., prev_sigma=)')
            sig = mppi_warm_start_rows(prev, H, rs["shift"], 0.0, np.inf)
        elif ws is not None:
            sig = np.full(rows.shape, ws, np.float32)
        if sig is not None:
            if sig.shape != rows.shape:
                raise ValueError(f"prev_sigma gives {sig.shape} rows, the warm start {rows.shape}")
            if not (np.isfinite(sig).all() and (sig > 0).all()):   # MBRL_EINVAL of mbrl_cem_plan_rh, made here
                raise ValueError("initial sigma rows must be finite and > 0")
    if carry is not None:
        c = carry.detach().cpu().numpy() if isinstance(carry, torch.Tensor) else carry
        carry = np.ascontiguousarray(c, dtype=np.float32)
        if carry.ndim != 3 or carry.shape[:2] != (Kc, H):
            raise ValueError(f"carry must be [keep_elites={Kc}, horizon={H}, a], got {carry.shape}")
    if rows is None and carry is None and Kc == 0:
        return None
    return dict(mu_rows=rows, sigma_rows=sig, carry=carry, Kc=Kc)


def cem_plan_batch(initial_states, model, cost, sample_action, horizon, **kwargs):
    """B independent CEM plans in shared launches (mbrl_cem_plan_batch): one per row of
    initial_states [B, s], e.g. the observations of B parallel environments (parallel.py:20-52
    runs one planner per worker process; here one GPU serves them all). kwargs as CEMPlanner.plan;
    num_candidates / num_elites are per problem. Problem b draws its proposals as candidates
    [b*N, (b+1)*N) of one Philox stream. Returns (states [B, H, s], actions [B, H, a]).

    Closures the fused path does not recognise fall back to one CEMPlanner.plan per row."""
    _rh_refuse(kwargs, "cem_plan_batch")
    _noise_refuse(kwargs, "cem_plan_batch")
    _ts_refuse(kwargs, "cem_plan_batch")
    dev = _device(kwargs)
    st = CEMPlanner._settings(sample_action, horizon, kwargs)
    B = int(initial_states.shape[0])
    with torch.cuda.device(dev):
        mdesc, cdesc, prob = fused.describe_problem(model, cost, dev, st["precision"])
        if mdesc is None or cdesc is None:
            outs = [CEMPlanner.plan(initial_states[b], model, cost, sample_action, horizon,
                                    **dict(kwargs, seed=st["seed"], return_device=True)) for b in range(B)]
            states, actions = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
        else:
            lib = _lib.load()
            H, a, s = st["H"], mdesc["a"], mdesc["s"]
            params = _cem_params(st, int(st["seed"]) & 0xFFFFFFFFFFFFFFFF)
            need = lib.mbrl_cem_plan_batch_workspace_bytes(fused.ctypes_ref(prob.shape), fused.ctypes_ref(params), B)
            ws = _workspace(("cem_batch", str(dev)), need, dev)
            s0 = initial_states.to(device=dev, dtype=torch.float32).reshape(B, s).contiguous()
            actions = torch.empty((B, H, a), dtype=torch.float32, device=dev)
            states = torch.empty((B, H, s), dtype=torch.float32, device=dev)
            _lib.check(lib.mbrl_cem_plan_batch(*prob.refs, _lib.ptr(s0), B, fused.ctypes_ref(params), None, None,
                                               _lib.ptr(actions), _lib.ptr(states), _lib.ptr(ws), ws.numel(),
                                               _lib.stream_handle(dev)), "mbrl_cem_plan_batch")
        keep = st["keep"]
        return _to_host(states, keep), _to_host(actions, keep)


RH_FLAG_MU, RH_FLAG_SIGMA, RH_FLAG_CARRY = 1, 2, 4   # mbrl_cem_plan_rh_batch's input_flags bits


def _per_row(x, B, name):
    """A per-problem argument as a list of B entries (None: B Nones)."""
    if x is None:
        return [None] * B
    x = list(x)
    if len(x) != B:
        raise ValueError(f"{name} has {len(x)} entries for {B} initial states")
    return x


def _rh_batch_inputs(st, B, initial_trajectories, carries, prev_sigmas, kwargs, a=None):
    """The receding-horizon inputs of B plans as host arrays (host only, no device): each row built and
    checked by _rh_inputs (the single plan's rules -- warm-start rows, sigma rows finite and > 0, the carry's
    shape), then stacked. dict(mu_rows, sigma_rows [B, H, a], carry [B, Kc, H, a], each None when no row has
    it; flags int32 [B], bit RH_FLAG_* set where row b has that input, None when nothing is given; Kc).
    A row without an input holds filler the flags switch off (zeros; ones for sigma). a: the action
    dimension every given row must have (None: the first given row's)."""
    Kc = _rh_settings(kwargs, st["K"])["Kc"]
    inits = _per_row(initial_trajectories, B, "initial_trajectories")
    carries = _per_row(carries, B, "carries")
    sigmas = _per_row(prev_sigmas, B, "prev_sigmas")
    rows = []
    for b in range(B):
        kw = dict(kwargs, carry=carries[b], prev_sigma=sigmas[b])
        rows.append(_rh_inputs(st, inits[b], kw) or dict(mu_rows=None, sigma_rows=None, carry=None))
    given = [x for r in rows for x in (r["mu_rows"], r["sigma_rows"], r["carry"]) if x is not None]
    if a is None and given:
        a = given[0].shape[-1]
    for b, r in enumerate(rows):
        for k in ("mu_rows", "sigma_rows", "carry"):
            if r[k] is not None and r[k].shape[-1] != a:
                raise ValueError(f"row {b}: {k} has {r[k].shape[-1]} action dims, expected {a}")
    H = st["H"]
    out = dict(Kc=Kc, flags=None)
    flags = np.zeros(B, np.int32)
    for k, bit, shape, fill in (("mu_rows", RH_FLAG_MU, (H, a), 0.0), ("sigma_rows", RH_FLAG_SIGMA, (H, a), 1.0),
                                ("carry", RH_FLAG_CARRY, (Kc, H, a), 0.0)):
        if all(r[k] is None for r in rows):
            out[k] = None
            continue
        out[k] = np.stack([np.full(shape, fill, np.float32) if r[k] is None else r[k] for r in rows])
        flags |= np.array([0 if r[k] is None else bit for r in rows], np.int32)
    if given:
        out["flags"] = flags
    return out


def _rh_call_inputs(lib, rh, a, dev, noise, batched):
    """What the single and the batched receding-horizon call share: the rows' action-dimension check, the
    upload of the mean rows, sigma rows, carry and (batched) flags -- an absent one stays None -- and the choice
    of sizer and entry by the noise mix (one matrix serves all B problems). Returns (the uploaded tensors, the
    entry's input pointers, sizer, entry)."""
    keys = ("mu_rows", "sigma_rows", "carry") + (("flags",) if batched else ())
    for k in keys[:3]:
        if rh[k] is not None and rh[k].shape[-1] != a:
            raise ValueError(f"{k} has {rh[k].shape[-1]} action dims, the model {a}")
    tensors = [None if rh[k] is None else torch.from_numpy(np.ascontiguousarray(rh[k])).to(dev) for k in keys]
    ins = tuple(_lib.ptr(t) for t in tensors)
    entry = "mbrl_cem_plan_rh_batch" if batched else "mbrl_cem_plan_rh"
    if noise is None:
        sizer = lib.mbrl_cem_rh_batch_workspace_bytes if batched else lib.mbrl_cem_rh_workspace_bytes
        return tensors, ins, sizer, getattr(lib, entry)
    ins += (_lib.ptr(_noise_mix_device(noise, dev)),)
    return tensors, ins, lib.mbrl_cem_rh_mixed_workspace_bytes, getattr(lib, entry + "_mixed")


def cem_plan_batch_rh(initial_states, model, cost, sample_action, horizon, initial_trajectories=None, carries=None,
                      prev_sigmas=None, **kwargs):
    """B independent receding-horizon CEM plans in shared launches (mbrl_cem_plan_rh_batch): cem_plan_batch
    with each problem's own warm start and kept rows, so one GPU planner serves B environments that are each
    somewhere in their own episode. kwargs as CEMPlanner.plan, including warm_start, shift, warm_std and
    keep_elites (per problem). initial_trajectories, carries (each [Kc, H, a], already shifted:
    cem_shift_carry) and prev_sigmas (warm_std="keep") are lists of B entries; a None entry plans that problem
    without that input (its first control step). Problem b draws its proposals as candidates [b*N, (b+1)*N)
    of one Philox stream.

    Returns a dict: states [B, H, s], actions, mu, sigma [B, H, a]; with keep_elites > 0 also carry
    [B, Kc, H, a] and carry_returns [B, Kc]; record=True adds costs [I, E, B*N], returns [I, B, N], elites
    [I, B, K] and (keep_elites > 0) kept_hist [I + 1, B, Kc, H, a]. Host tensors unless return_device.
    The per-row host checks (sigma rows finite and > 0, the carry's shape) raise ValueError before anything
    touches the device; closures the fused path does not recognise raise NotImplementedError."""
    if kwargs.get("distributed", False):
        raise NotImplementedError("cem_plan_batch_rh: distributed=True is not implemented")
    _ts_refuse(kwargs, "cem_plan_batch_rh")
    noise = _noise_inputs(kwargs, int(horizon))
    for k, lists in (("carry", "carries"), ("prev_sigma", "prev_sigmas")):
        if kwargs.get(k) is not None:
            raise TypeError(f"cem_plan_batch_rh takes per-problem lists ({lists}=...), not {k}=")
    kwargs = {k: v for k, v in kwargs.items() if k not in ("carry", "prev_sigma")}
    st = CEMPlanner._settings(sample_action, horizon, kwargs)
    B = int(initial_states.shape[0])
    if B < 1:
        raise ValueError("cem_plan_batch_rh needs at least one initial state")
    rh = _rh_batch_inputs(st, B, initial_trajectories, carries, prev_sigmas, kwargs)
    dev = _device(kwargs)
    with torch.cuda.device(dev):
        mdesc, cdesc, prob = fused.describe_problem(model, cost, dev, st["precision"])
        if mdesc is None or cdesc is None:
            raise NotImplementedError("cem_plan_batch_rh: callables the fused path does not recognise are not "
                                      "implemented (receding-horizon CEM plans are fused-path plans)")
        lib = _lib.load()
        N, K, H, I, Kc = st["N"], st["K"], st["H"], st["I"], rh["Kc"]
        a, s, E = mdesc["a"], mdesc["s"], mdesc["E"]
        _held, ins, sizer, call = _rh_call_inputs(lib, rh, a, dev, noise, True)   # (the uploads, held to the call)
        params = _lib.CemRhParams(_cem_params(st, int(st["seed"]) & 0xFFFFFFFFFFFFFFFF), Kc, 0)
        need = sizer(fused.ctypes_ref(prob.shape), fused.ctypes_ref(params), B)
        if need == 0:
            _lib.check(_lib.MBRL_EINVAL, sizer.__name__)
        ws = _workspace(("cem_rh_batch", str(dev)), need, dev)
        s0 = initial_states.to(device=dev, dtype=torch.float32).reshape(B, s).contiguous()
        e = lambda *sh, dt=torch.float32: torch.empty(sh, dtype=dt, device=dev)  # noqa: E731
        out = dict(states=e(B, H, s), actions=e(B, H, a), mu=e(B, H, a), sigma=e(B, H, a))
        rec = st["record"]
        if Kc:
            out.update(carry=e(B, Kc, H, a), carry_returns=e(B, Kc))
        if rec:
            out.update(costs=e(I, E, B * N), returns=e(I, B, N), elites=e(I, B, K, dt=torch.int64))
            if Kc:
                out.update(kept_hist=e(I + 1, B, Kc, H, a))
        g = lambda k: _lib.ptr(out.get(k))  # noqa: E731
        _lib.check(call(*prob.refs, _lib.ptr(s0), B, fused.ctypes_ref(params), *ins, g("mu"), g("sigma"), g("actions"),
                        g("states"), g("carry"), g("carry_returns"), g("costs"), g("returns"), g("elites"),
                        g("kept_hist"), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)), call.__name__)
        return {k: _to_host(v, st["keep"]) for k, v in out.items()}


class RecedingHorizonCEMPlanner(CEMPlanner):
    """CEMPlanner with the receding-horizon kwargs switched on -- warm_start=True and keep_elites=0.3 (a
    fraction of num_elites) unless the caller says otherwise -- and a batched form that keeps each
    problem's kept rows between control steps, so the planner service (parallel.get_rollouts_parallel) warm-
    starts every rollout it serves.

    plan() is CEMPlanner.plan with those defaults. plan_batch() answers B problems with one
    cem_plan_batch_rh call and hands back one memo per problem: that plan's carry and sigma, unshifted. The
    caller gives a problem's memo back at its next control step (None at its first), and plan_batch shifts
    it: the carry with cem_shift_carry, the sigma (used with warm_std="keep") with mppi_warm_start_rows."""
    rh_defaults = dict(warm_start=True, keep_elites=0.3)
    # the planner service passes each rollout's previous plan (initial_trajectories) and its memo (memos)
    warm_starts = True
    plan_memo = True

    @staticmethod
    def _kwargs(kwargs):
        return dict(RecedingHorizonCEMPlanner.rh_defaults, **kwargs)

    @staticmethod
    def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        return CEMPlanner.plan(initial_state, model, cost, sample_action, horizon, initial_trajectory,
                               **RecedingHorizonCEMPlanner._kwargs(kwargs))

    @staticmethod
    def _memo_inputs(memos, B, shift, lo, hi):
        """(carries, prev_sigmas) for cem_plan_batch_rh from B memos (host only): a memo's carry shifted by
        cem_shift_carry; its sigma as it is (the warm start shifts it with the mean). None stays None."""
        memos = _per_row(memos, B, "memos")
        carries = [None if m is None or m.get("carry") is None else cem_shift_carry(m["carry"], shift, lo, hi)
                   for m in memos]
        return carries, [None if m is None else m.get("sigma") for m in memos]

    @staticmethod
    def plan_batch(initial_states, model, cost, sample_action, horizon, initial_trajectories=None, memos=None,
                   **kwargs):
        """B plans at once; returns (states [B, H, s], actions [B, H, a], memos) -- memos[b] = dict(carry
        [Kc, H, a] or None, sigma [H, a]) of problem b's plan, host tensors, to pass back at its next step."""
        kw = RecedingHorizonCEMPlanner._kwargs(kwargs)
        st = CEMPlanner._settings(sample_action, horizon, kw)
        rs = _rh_settings(kw, st["K"])
        B = int(initial_states.shape[0])
        carries, sigmas = RecedingHorizonCEMPlanner._memo_inputs(memos, B, rs["shift"], st["lo"], st["hi"])
        if rs["Kc"] == 0:
            carries = None
        res = cem_plan_batch_rh(initial_states, model, cost, sample_action, horizon, initial_trajectories, carries,
                                sigmas if rs["warm_std"] == "keep" else None, **kw)
        carry = res["carry"].cpu() if "carry" in res else None
        sigma = res["sigma"].cpu()
        out = [dict(carry=None if carry is None else carry[b], sigma=sigma[b]) for b in range(B)]
        return res["states"], res["actions"], out


def _ts_rh_inputs(kwargs):
    """The checked particle kwargs of TrajectorySamplingCEMPlanner as dict(P, noise, seed, mode): ValueError for a
    bad particle_mode or particle value, NotImplementedError naming every kwarg the sampled plans have no form for,
    before anything needs a device."""
    mode = kwargs.get("particle_mode", TrajectorySamplingCEMPlanner.ts_defaults["particle_mode"])
    if not isinstance(mode, str) or mode not in _lib.TS_MEMBER_MODES:
        raise ValueError(f"particle_mode={mode!r}: need one of {sorted(_lib.TS_MEMBER_MODES)}")
    P, noise, seed = _ts_values(kwargs)
    if P < 1:
        raise ValueError(f"particles={P!r}: TrajectorySamplingCEMPlanner needs an integer >= 1")
    where = f"TrajectorySamplingCEMPlanner with particles={P}"
    if kwargs.get("distributed", False):
        raise NotImplementedError(f"{where}: distributed=True is not implemented")
    _noise_refuse(kwargs, where)
    precision = kwargs.get("precision", CEMPlanner.defaults["precision"])
    if precision != "f32":
        raise NotImplementedError(f"{where}: precision={precision!r} is not implemented (the sampled rollout is fp32)")
    dev = kwargs.get("device")
    if dev is not None and torch.device(dev).type != "cuda":
        raise NotImplementedError(f"{where}: device={str(dev)!r} is not implemented (the sampled rollout is a HIP "
                                  "kernel)")
    return dict(P=P, noise=noise, seed=seed, mode=mode)


def _cem_ts_rh(kwargs, st, ts, rh, initial_states, model, cost, B):
    """One C-ABI call: mbrl_cem_plan_ts_rh (B None: initial_states [s]) or mbrl_cem_plan_ts_rh_batch (initial_states
    [B, s]). rh: _rh_inputs' / _rh_batch_inputs' dict. Returns the result dict on the device: states, actions, mu,
    sigma, with kept rows carry and carry_returns, with record=True costs ([I, Q, N] or [I, Q, B N]), returns, elites
    and kept_hist."""
    dev = _device(kwargs)
    batched = B is not None
    with _on_device(dev):
        mdesc, cdesc, prob = fused.describe_problem(model, cost, dev, st["precision"])
        if mdesc is None or cdesc is None:
            raise NotImplementedError(f"CEMPlanner with callables the fused path does not recognise: particles="
                                      f"{ts['P']} is not implemented (trajectory sampling runs on the fused path)")
        lib = _lib.load()
        resampled = ts["mode"] == "resampled"
        table = _ts_table(prob, ts["P"], resampled)
        N, K, H, I, Kc = st["N"], st["K"], st["H"], st["I"], rh["Kc"]
        a, s = mdesc["a"], mdesc["s"]
        Q = ts["P"] if resampled else table.E * ts["P"]
        nb = B if batched else 1
        _held, ins, _, _ = _rh_call_inputs(lib, rh, a, dev, None, batched)   # (the uploads, held to the call)
        seed = int(st["seed"]) & 0xFFFFFFFFFFFFFFFF
        rows = fused.ts_rows(ts["P"], 0, _ts_seed(seed) if ts["seed"] is None else ts["seed"], ts["noise"], ts["mode"])
        pkey = ("ts_rh", ts["P"], ts["mode"], nb, N, H, K, I, Kc, st["alpha"], st["lo"], st["hi"], st["init_std"], seed)
        _, pref, need = _plan_params(prob, pkey, lambda: _lib.CemRhParams(_cem_params(st, seed), Kc, 0),
                                     lib.mbrl_cem_ts_rh_workspace_bytes, fused.ctypes_ref(rows), nb)
        if need == 0:
            _lib.check(_lib.MBRL_EINVAL, "mbrl_cem_ts_rh_workspace_bytes")
        ws = _workspace(("cem_ts_rh", str(dev)), need, dev)
        lead = (B,) if batched else ()
        s0 = initial_states.to(device=dev, dtype=torch.float32).reshape(*lead, s).contiguous()
        e = lambda *sh, dt=torch.float32: torch.empty(sh, dtype=dt, device=dev)  # noqa: E731
        if batched:
            out = dict(states=e(B, H, s), actions=e(B, H, a), mu=e(B, H, a), sigma=e(B, H, a))
        else:
            out = _device_outputs(dev, H, s, a)
        rec = st["record"]
        if Kc:
            out.update(carry=e(*lead, Kc, H, a), carry_returns=e(*lead, Kc))
        if rec:
            out.update(costs=e(I, Q, nb * N), returns=e(I, *lead, N), elites=e(I, *lead, K, dt=torch.int64))
            if Kc:
                out.update(kept_hist=e(I + 1, *lead, Kc, H, a))
        g = lambda k: _lib.ptr(out.get(k))  # noqa: E731
        shape_ref, packed, norm_ref, cost_ref = prob.refs
        head = (shape_ref, packed, *table.refs, norm_ref, cost_ref, _lib.ptr(s0)) + ((B,) if batched else ())
        call = lib.mbrl_cem_plan_ts_rh_batch if batched else lib.mbrl_cem_plan_ts_rh
        pev = st["plan_events"]
        _mark(pev, 0)
        _lib.check(call(*head, pref, fused.ctypes_ref(rows), *ins, g("mu"), g("sigma"), g("actions"), g("states"),
                        g("carry"), g("carry_returns"), g("costs"), g("returns"), g("elites"), g("kept_hist"),
                        _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)), call.__name__)
        _mark(pev, 1)
        return out


class TrajectorySamplingCEMPlanner(ModelPlanner):
    """CEM on sampled ensemble particles for the control loop (mbrl_cem_plan_ts_rh, mbrl_cem_plan_ts_rh_batch):
    CEMPlanner(particles=P)'s sampled rollout with the receding-horizon inputs CEMPlanner refuses beside it -- warm
    start, kept rows, batches -- and PETS' second propagation mode.

    kwargs: CEMPlanner's own (num_candidates, num_elites, num_iterations, alpha, seed, init_std, action_bounds,
    return_device, record) and, with CEMPlanner's meaning and checks, warm_start (True here), shift, warm_std,
    keep_elites (0.3 here), carry, particle_noise and particle_seed.
    particles (1): P >= 1.
    particle_mode ("fixed"): "fixed" rolls every candidate out as P particles per member, each on its member for the
        whole horizon (TS-inf: E * P rows); "resampled" as P rows in all, each drawing its member afresh at every
        step (TS-1: the row count no longer depends on the ensemble's size). Anything else raises ValueError.
    The model and cost requirements are CEMPlanner(particles=P)'s; distributed=True, the coloured-noise kwargs, a
    precision other than "f32" and a CPU device raise NotImplementedError.

    plan_detailed returns dict(states, actions, mu, sigma[, carry, carry_returns]); record=True adds costs
    [I, Q, N], returns, elites and kept_hist. plan_batch answers B problems with one call and hands back one memo per
    problem, exactly as RecedingHorizonCEMPlanner.plan_batch does."""
    ts_defaults = dict(particles=1, particle_mode="fixed", warm_start=True, keep_elites=0.3)
    # the planner service passes each rollout's previous plan (initial_trajectories) and its memo (memos)
    warm_starts = True
    plan_memo = True

    @staticmethod
    def _kwargs(kwargs):
        return dict(TrajectorySamplingCEMPlanner.ts_defaults, **kwargs)

    @staticmethod
    def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        res = TrajectorySamplingCEMPlanner.plan_detailed(initial_state, model, cost, sample_action, horizon,
                                                         initial_trajectory, **kwargs)
        return res["states"], res["actions"]

    @staticmethod
    def plan_detailed(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        kw = TrajectorySamplingCEMPlanner._kwargs(kwargs)
        ts = _ts_rh_inputs(kw)
        st = CEMPlanner._settings(sample_action, horizon, kw)
        rh = _rh_inputs(st, initial_trajectory, kw) or dict(mu_rows=None, sigma_rows=None, carry=None, Kc=0)
        res = _cem_ts_rh(kw, st, ts, rh, initial_state, model, cost, None)
        if st["record"]:
            for k, src in (("init_mu", "mu_rows"), ("init_sigma", "sigma_rows")):
                if rh[src] is not None:
                    res[k] = torch.from_numpy(rh[src])
        return _finish(res, st["keep"])

    @staticmethod
    def plan_batch(initial_states, model, cost, sample_action, horizon, initial_trajectories=None, memos=None,
                   **kwargs):
        """B plans at once; returns (states [B, H, s], actions [B, H, a], memos) -- memos[b] = dict(carry
        [Kc, H, a] or None, sigma [H, a]) of problem b's plan, host tensors, to pass back at its next step."""
        res = TrajectorySamplingCEMPlanner.plan_batch_detailed(initial_states, model, cost, sample_action, horizon,
                                                               initial_trajectories, memos, **kwargs)
        B = int(initial_states.shape[0])
        carry = res["carry"].cpu() if "carry" in res else None
        sigma = res["sigma"].cpu()
        out = [dict(carry=None if carry is None else carry[b], sigma=sigma[b]) for b in range(B)]
        return res["states"], res["actions"], out

    @staticmethod
    def plan_batch_detailed(initial_states, model, cost, sample_action, horizon, initial_trajectories=None, memos=None,
                            **kwargs):
        """plan_batch's one call as its result dict (cem_plan_batch_rh's layouts, costs [I, Q, B N])."""
        kw = TrajectorySamplingCEMPlanner._kwargs(kwargs)
        ts = _ts_rh_inputs(kw)
        for k in ("carry", "prev_sigma"):
            if kw.get(k) is not None:
                raise TypeError(f"TrajectorySamplingCEMPlanner.plan_batch takes per-problem memos, not {k}=")
        kw = {k: v for k, v in kw.items() if k not in ("carry", "prev_sigma")}
        st = CEMPlanner._settings(sample_action, horizon, kw)
        rs = _rh_settings(kw, st["K"])
        B = int(initial_states.shape[0])
        if B < 1:
            raise ValueError("TrajectorySamplingCEMPlanner.plan_batch needs at least one initial state")
        carries, sigmas = RecedingHorizonCEMPlanner._memo_inputs(memos, B, rs["shift"], st["lo"], st["hi"])
        rh = _rh_batch_inputs(st, B, initial_trajectories, carries if rs["Kc"] else None,
                              sigmas if rs["warm_std"] == "keep" else None, kw)
        res = _cem_ts_rh(kw, st, ts, rh, initial_states, model, cost, B)
        return {k: _to_host(v, st["keep"]) for k, v in res.items()}


_WS = threading.local()


def _workspace(key, nbytes, device):
    """Scratch for `key` owned by this thread and the current stream of `device`. A plan enqueues on
    the current stream and reuses its scratch in stream order; another thread, or this thread on
    another stream, gets a buffer of its own, so plans in flight never share scratch (the flags,
    epochs and proposals of one plan are not overwritten by another's launches)."""
    bufs = getattr(_WS, "bufs", None)
    if bufs is None:
        bufs = _WS.bufs = {}
    idx = device.index if device.index is not None else torch.cuda.current_device()
    k = key + (torch._C._cuda_getCurrentRawStream(idx),)
    buf = bufs.get(k)
    if buf is None or buf.numel() < nbytes or buf.device != device:
        if buf is None and len(bufs) > 16:
            bufs.clear()
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        bufs[k] = buf
    return buf


_STAGING = threading.local()
# plan() with host inputs / outputs goes through mapped pinned staging (_cem_plan_host); False: the
# device-buffer path with a host-to-device copy of s0 and a device-to-host copy of the results (A/B)
HOST_STAGING = True


def _staging(dev, n):
    """This thread's mapped pinned host buffer of >= n floats for plans on `dev` (_lib.HostStaging)."""
    bufs = getattr(_STAGING, "bufs", None)
    if bufs is None:
        bufs = _STAGING.bufs = {}
    buf = bufs.get(str(dev))
    if buf is None or buf.n < n:
        buf = bufs[str(dev)] = _lib.HostStaging(max(n, 256))
    return buf


def _layout(H, s, a):
    """The plan's output buffer, in floats: states [H, s] at 0, then the offsets of actions, mu and sigma
    ([H, a] each) and the length H (s + 3 a). States and actions lie side by side, so that one copy hands
    both to the host (_finish); host staging keeps s0 behind the outputs."""
    return H * s, H * (s + a), H * (s + 2 * a), H * (s + 3 * a)


def _stage_in(dev, s0, H, s, a):
    """s0 (a host tensor) into this thread's staging buffer, behind the outputs. Returns the buffer's host
    array and the device addresses the C call takes: (s0, mu, sigma, actions, states)."""
    o_act, o_mu, o_sg, o_s0 = _layout(H, s, a)
    stage = _staging(dev, o_s0 + s)
    x = s0.detach() if s0.requires_grad else s0
    stage.array[o_s0:o_s0 + s] = (x.numpy().reshape(-1) if x.dtype == torch.float32
                                  else x.reshape(-1).to(torch.float32).numpy())
    return stage.array, stage.cached_at((H, s, a), (o_s0, o_mu, o_sg, o_act, 0))


def _stage_out(arr, H, s, a):
    """The finished plan's outputs as host tensors over ONE copy of the staging array (NumPy views wrapped
    once each: ~2.4x cheaper than torch views). "_host": nothing is left for plan_detailed to bring back."""
    o_act, o_mu, o_sg, end = _layout(H, s, a)
    x = arr[:end].copy()
    return dict(states=torch.from_numpy(x[:o_act].reshape(H, s)), actions=torch.from_numpy(x[o_act:o_mu].reshape(H, a)),
                mu=torch.from_numpy(x[o_mu:o_sg].reshape(H, a)), sigma=torch.from_numpy(x[o_sg:].reshape(H, a)),
                _host=True)


def _device_outputs(dev, H, s, a):
    """One device allocation in _layout's order, as the result dict: states, actions, mu, sigma and
    "_both", the stretch that holds states and actions."""
    o_act, o_mu, o_sg, end = _layout(H, s, a)
    buf = torch.empty(end, dtype=torch.float32, device=dev)
    both = buf[:o_mu]
    return dict(states=both[:o_act].view(H, s), actions=both[o_act:].view(H, a), mu=buf[o_mu:o_sg].view(H, a),
                sigma=buf[o_sg:].view(H, a), _both=both)


def _output_ptrs(out):
    """The device addresses of _device_outputs' tensors in the C calls' order: mu, sigma, actions, states."""
    return _lib.ptr(out["mu"]), _lib.ptr(out["sigma"]), _lib.ptr(out["actions"]), _lib.ptr(out["states"])


def _cem_record_buffers(dev, rec, I, E, N, K):
    """record=True: every iteration's costs [I, E, N], returns [I, N] and elites [I, K]; else Nones."""
    shapes = ((I, E, N), torch.float32), ((I, N), torch.float32), ((I, K), torch.int64)
    return [torch.empty(sh, dtype=dt, device=dev) if rec else None for sh, dt in shapes]


def _plan_params(prob, key, make_params, workspace_bytes, *extra):
    """(params struct, its ctypes reference, workspace bytes) for the settings in `key`, built once per
    problem and kept in prob.plan_cache (host turn). workspace_bytes(shape, params, *extra) is the
    library's query; its answer 0 (settings refused: the caller raises) is not kept."""
    hit = prob.plan_cache.get(key)
    if hit is None:
        params = make_params()
        need = workspace_bytes(fused.ctypes_ref(prob.shape), fused.ctypes_ref(params), *extra)
        if need == 0:
            return params, fused.ctypes_ref(params), 0
        if len(prob.plan_cache) > 64:
            prob.plan_cache.clear()
        hit = prob.plan_cache[key] = (params, fused.ctypes_ref(params), need)
    return hit


def _mark(pev, i):
    """Record event i of the plan_events pair around the C call (bench.py's device span), if asked for."""
    if pev is not None:
        pev[i].record()


_EVENT_ARRAYS = {}


def _events(st, I):
    events = st["events"]
    if events is None:
        return None
    handles = tuple((e.cuda_event if pair is not None else None) for pair in events for e in (pair or (None, None)))
    arr = _EVENT_ARRAYS.get(handles)
    if arr is None:
        if len(_EVENT_ARRAYS) > 16:
            _EVENT_ARRAYS.clear()
        arr = _EVENT_ARRAYS[handles] = (_lib.c_void_p * (2 * I))(*handles)
    return arr


def _cem_params(st, seed):
    return _lib.CemParams(st["N"], st["H"], st["K"], st["I"], st["alpha"], st["lo"], st["hi"], 0.0, st["init_std"], 0,
                          seed)


def _cem_plan_host(lib, prob, initial_state, st, params, ws, pref):
    """mbrl_cem_plan with host staging (_lib.HostStaging): the plan's first launch reads the initial
    state from mapped host memory and its last launches write states, actions, mu and sigma there, so
    no copy launch precedes or follows the plan; one stream sync, then host tensors."""
    dev = prob.device
    md = prob.mdesc
    H, a, s = st["H"], md["a"], md["s"]
    arr, (p_s0, p_mu, p_sg, p_act, p_st) = _stage_in(dev, initial_state, H, s, a)
    pev = st["plan_events"]
    _mark(pev, 0)
    _lib.check(lib.mbrl_cem_plan(*prob.refs, p_s0, pref, p_mu, p_sg, p_act, p_st, None, None, None,
                                 _events(st, params.iterations), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)),
               "mbrl_cem_plan")
    _mark(pev, 1)
    torch.cuda.current_stream(dev).synchronize()
    return _stage_out(arr, H, s, a)


def _cem_fused_single(prob, initial_state, st):
    """One C-ABI call: mbrl_cem_plan (every iteration stream-ordered, no host sync)."""
    lib = _lib.load()
    dev = prob.device
    md = prob.mdesc
    N, K, H, I = st["N"], st["K"], st["H"], st["I"]
    a, s, E = md["a"], md["s"], md["E"]
    pkey = (N, H, K, I, st["alpha"], st["lo"], st["hi"], st["init_std"], int(st["seed"]) & 0xFFFFFFFFFFFFFFFF)
    params, pref, need = _plan_params(prob, pkey, lambda: _cem_params(st, pkey[-1]), lib.mbrl_cem_workspace_bytes)
    ws = _workspace(("cem", str(dev)), need, dev)
    rec = st["record"]
    if HOST_STAGING and not st["keep"] and not rec and not initial_state.is_cuda:
        return _cem_plan_host(lib, prob, initial_state, st, params, ws, pref)
    s0 = initial_state.to(device=dev, dtype=torch.float32).contiguous()
    out = _device_outputs(dev, H, s, a)
    cost_hist, ret_hist, elite_hist = _cem_record_buffers(dev, rec, I, E, N, K)
    ev_arr = _events(st, I)
    pev = st["plan_events"]
    _mark(pev, 0)
    _lib.check(lib.mbrl_cem_plan(*prob.refs, _lib.ptr(s0), pref, *_output_ptrs(out), _lib.ptr(cost_hist),
                                 _lib.ptr(ret_hist), _lib.ptr(elite_hist), ev_arr, _lib.ptr(ws), ws.numel(),
                                 _lib.stream_handle(dev)), "mbrl_cem_plan")
    _mark(pev, 1)
    if rec:
        out.update(costs=cost_hist, returns=ret_hist, elites=elite_hist)
    return out


def _ts_table(prob, P, resampled=False):
    """The sampled plans' model and cost requirements: the goal-state cost, an EnsembleModel of ProbabilisticModels
    (fused.ts_members raises NotImplementedError for any other model) and at most TS_MAX_ROWS rows -- E * P of them,
    or P where every row draws its member per step. Returns the member table."""
    where = f"CEMPlanner with particles={P}"
    if prob.mdesc.get("reward") or prob.cdesc["kind"] != _lib.MBRL_COST_GOAL_STATE:
        raise NotImplementedError(f"{where}: only the goal-state cost is implemented")
    table = fused.ts_members(prob.mdesc["module"], prob.device)
    if resampled and P > _lib.TS_MAX_ROWS:
        raise NotImplementedError(f"{where}: {P} resampled rows exceed {_lib.TS_MAX_ROWS} rows")
    if not resampled and table.E * P > _lib.TS_MAX_ROWS:
        raise NotImplementedError(f"{where}: {table.E} members x {P} particles exceed {_lib.TS_MAX_ROWS} rows")
    return table


def _cem_fused_ts(prob, initial_state, st, ts):
    """One C-ABI call: mbrl_cem_plan_ts, the plan on ts["P"] sampled particles per member. record=True returns the
    costs as [I, E * P, N]."""
    lib = _lib.load()
    dev = prob.device
    md = prob.mdesc
    P = ts["P"]
    table = _ts_table(prob, P)
    N, K, H, I = st["N"], st["K"], st["H"], st["I"]
    a, s, Q = md["a"], md["s"], table.E * P
    seed = int(st["seed"]) & 0xFFFFFFFFFFFFFFFF
    tsp = fused.ts_params(P, 0, _ts_seed(seed) if ts["seed"] is None else ts["seed"], ts["noise"])
    pkey = ("ts", P, N, H, K, I, st["alpha"], st["lo"], st["hi"], st["init_std"], seed)
    params, pref, need = _plan_params(prob, pkey, lambda: _cem_params(st, seed), lib.mbrl_cem_ts_workspace_bytes,
                                      fused.ctypes_ref(tsp))
    if need == 0:
        raise RuntimeError(f"mbrl_cem_ts_workspace_bytes: {lib.mbrl_last_error().decode()}")
    ws = _workspace(("cem_ts", str(dev)), need, dev)
    s0 = initial_state.to(device=dev, dtype=torch.float32).contiguous()
    out = _device_outputs(dev, H, s, a)
    cost_hist, ret_hist, elite_hist = _cem_record_buffers(dev, st["record"], I, Q, N, K)
    shape_ref, packed, norm_ref, cost_ref = prob.refs
    pev = st["plan_events"]
    _mark(pev, 0)
    _lib.check(lib.mbrl_cem_plan_ts(shape_ref, packed, *table.refs, norm_ref, cost_ref, _lib.ptr(s0), pref,
                                    fused.ctypes_ref(tsp), *_output_ptrs(out), _lib.ptr(cost_hist), _lib.ptr(ret_hist),
                                    _lib.ptr(elite_hist), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)),
               "mbrl_cem_plan_ts")
    _mark(pev, 1)
    if st["record"]:
        out.update(costs=cost_hist, returns=ret_hist, elites=elite_hist)
    return out


def _cem_fused_rh(prob, initial_state, st, rh):
    """One C-ABI call: mbrl_cem_plan_rh, or mbrl_cem_plan_rh_mixed where the plan has a noise mix (every
    iteration stream-ordered, no host sync). rh: _rh_inputs, with "mix" from _rh_with_noise."""
    lib = _lib.load()
    dev = prob.device
    md = prob.mdesc
    N, K, H, I, Kc = st["N"], st["K"], st["H"], st["I"], rh["Kc"]
    a, s, E = md["a"], md["s"], md["E"]
    noise = rh.get("mix")
    (rows_d, sig_d, _carry_d), ins, sizer, call = _rh_call_inputs(lib, rh, a, dev, noise, False)   # (held to the call)
    pkey = ("rh" if noise is None else "rh_mixed", N, H, K, I, Kc, st["alpha"], st["lo"], st["hi"], st["init_std"],
            int(st["seed"]) & 0xFFFFFFFFFFFFFFFF)
    _, pref, need = _plan_params(prob, pkey, lambda: _lib.CemRhParams(_cem_params(st, pkey[-1]), Kc, 0), sizer,
                                 *(() if noise is None else (1,)))
    if need == 0:
        _lib.check(_lib.MBRL_EINVAL, sizer.__name__)
    ws = _workspace(("cem_rh", str(dev)), need, dev)
    s0 = initial_state.to(device=dev, dtype=torch.float32).contiguous()
    out = _device_outputs(dev, H, s, a)
    rec = st["record"]
    cost_hist, ret_hist, elite_hist = _cem_record_buffers(dev, rec, I, E, N, K)
    carry_out = carry_ret = kept_hist = None
    if Kc:
        carry_out = torch.empty((Kc, H, a), dtype=torch.float32, device=dev)
        carry_ret = torch.empty((Kc,), dtype=torch.float32, device=dev)
        kept_hist = torch.empty((I + 1, Kc, H, a), dtype=torch.float32, device=dev) if rec else None
    pev = st["plan_events"]
    _mark(pev, 0)
    _lib.check(call(*prob.refs, _lib.ptr(s0), pref, *ins, *_output_ptrs(out), _lib.ptr(carry_out), _lib.ptr(carry_ret),
                    _lib.ptr(cost_hist), _lib.ptr(ret_hist), _lib.ptr(elite_hist), _lib.ptr(kept_hist), _events(st, I),
                    _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)), call.__name__)
    _mark(pev, 1)
    if rec:
        out.update(costs=cost_hist, returns=ret_hist, elites=elite_hist)
        if Kc:
            out.update(kept_hist=kept_hist)
        if rows_d is not None:       # the rows the plan started from (already clipped on the host)
            out.update(init_mu=rows_d)
        if sig_d is not None:
            out.update(init_sigma=sig_d)
    if Kc:
        out.update(carry=carry_out, carry_returns=carry_ret)
    return out


def cem_sharded_protocol(ops, st, world, rank):
    """Host protocol of the sharded CEM plan, independent of where the math runs.

    Rank r of G owns global candidates [r*N/G, (r+1)*N/G). Per iteration: local proposal draw +
    rollout (proposals keyed by the GLOBAL candidate index) -> one all-gather of the [E, N/G] local
    costs -> every rank runs the same deterministic select + refit on the full [E, N] costs. The
    refit regenerates the elites' actions from the counter RNG, so no moment collective is needed
    and mu / sigma are bit-identical on every rank and for every G.

    ops: .device; .rollout(it, mu, sigma, n_offset, n_local, costs_out[E, n_local], events) (events: None
    or a (start, end) pair to record around the rollout kernel alone);
    .all_gather(out_flat[G*E*n_local], local[E, n_local]); .select(costs[E, N], K, returns_out) -> elites;
    .refit(it, mu, sigma, elites, mu_out, sigma_out); .trajectory(actions[H, a]) -> states[H, s]; optionally
    .update(it, mu, sigma, costs, K, returns_out, mu_out, sigma_out, draw_next, n_offset, n_local) -> elites
    or None: select + refit (+ this rank's next proposals) at once, None when it does not apply.
    The fused path binds them to the HIP extension + RCCL; tests bind them to the CPU oracle + gloo."""
    N, K, H, I, E, a = st["N"], st["K"], st["H"], st["I"], st["E"], st["a"]
    if N % world:
        raise ValueError(f"num_candidates {N} must divide evenly over {world} ranks")
    Nl = N // world
    dev = ops.device
    mu = torch.zeros((H, a), dtype=torch.float32, device=dev)
    sigma = torch.full((H, a), st["init_std"], dtype=torch.float32, device=dev)
    mu_n, sigma_n = torch.empty_like(mu), torch.empty_like(sigma)
    local = torch.empty((E, Nl), dtype=torch.float32, device=dev)
    gathered = torch.empty(world * E * Nl, dtype=torch.float32, device=dev)
    rec = st["record"]
    hist = dict(costs=[], returns=[], elites=[])
    events = st["events"]
    for it in range(I):
        ops.rollout(it, mu, sigma, rank * Nl, Nl, local, None if events is None else events[it])
        ops.all_gather(gathered, local)
        # candidate r*Nl + j lives at gathered[r, :, j]
        costs = gathered.view(world, E, Nl).permute(1, 0, 2).reshape(E, N) if world > 1 else gathered.view(E, N)
        rets = torch.empty(N, dtype=torch.float32, device=dev) if rec else None
        upd = getattr(ops, "update", None)
        elites = None if upd is None else upd(it, mu, sigma, costs, K, rets, mu_n, sigma_n, it + 1 < I, rank * Nl, Nl)
        if elites is None:
            elites = ops.select(costs, K, rets)
            ops.refit(it, mu, sigma, elites, mu_n, sigma_n)
        mu, mu_n = mu_n, mu
        sigma, sigma_n = sigma_n, sigma
        if rec:
            hist["costs"].append(costs.clone())
            hist["returns"].append(rets)
            hist["elites"].append(elites)
    actions = mu.clamp(st["lo"], st["hi"]).contiguous()
    states = ops.trajectory(actions)
    out = dict(states=states, actions=actions, mu=mu, sigma=sigma)
    if rec:
        out.update({k: torch.stack(v) for k, v in hist.items()})
    return out


class _FusedShardOps:
    """cem_sharded_protocol bound to the HIP extension (C ABI) and torch.distributed (RCCL)."""

    def __init__(self, prob, s0, st):
        self.prob, self.s0, self.st, self.device = prob, s0, st, prob.device
        H, a, N, K = st["H"], prob.mdesc["a"], st["N"], st["K"]
        lib = _lib.load()
        self._acts = None
        self._drawn = None      # (iteration, n_offset, n_local) whose proposals self._acts holds
        self._fused_update = True
        self._sel_ws = _workspace(("sel", str(self.device)), lib.mbrl_select_workspace_bytes(N), self.device)
        self._refit_ws = _workspace(("refit", str(self.device)), lib.mbrl_refit_workspace_bytes(H, a, K), self.device)
        self._traj_ws = _workspace(("traj", str(self.device)),
                                   lib.mbrl_trajectory_workspace_bytes(fused.ctypes_ref(prob.shape), H), self.device)

    def _sampler(self, it, mu, sigma):
        return fused.make_sampler(self.st["seed"], it, mu, sigma, self.st["lo"], self.st["hi"])

    def rollout(self, it, mu, sigma, n_offset, n_local, costs_out, events=None):
        H, a = self.st["H"], self.prob.mdesc["a"]
        if self._acts is None or self._acts.shape[1] != n_local:
            self._acts = torch.empty((H, n_local, a), dtype=torch.float32, device=self.device)
            self._drawn = None
        # proposal draw (unless the last update drew this shard already), then the rollout kernel
        # alone between the events (bench.py's roofline)
        if self._drawn != (it, n_offset, n_local):
            fused.sample_actions(self._sampler(it, mu, sigma), H, a, n_local, n_offset, self._acts)
        self._drawn = None
        if events is not None:
            events[0].record()
        fused.rollout(self.prob, self.s0, n_local, H, actions=self._acts, costs=costs_out)
        if events is not None:
            events[1].record()

    def all_gather(self, out_flat, local):
        import torch.distributed as dist
        if dist.get_backend() == "gloo":
            # host-staged for gloo (CPU rehearsals of the sharded path on a shared GPU); RCCL gathers
            # device memory directly
            host = torch.empty(out_flat.shape, dtype=out_flat.dtype)
            dist.all_gather_into_tensor(host, local.reshape(-1).cpu())
            out_flat.copy_(host)
        else:
            dist.all_gather_into_tensor(out_flat, local.reshape(-1))

    def update(self, it, mu, sigma, costs, K, returns_out, mu_out, sigma_out, draw_next, n_offset, n_local):
        """mbrl_cem_update: selection, refit and (draw_next) this rank's proposals of iteration it + 1 in
        one launch, bit-identical to select + refit + sample_actions; None where it does not apply."""
        if not self._fused_update:
            return None
        H, a = self.st["H"], self.prob.mdesc["a"]
        nxt = self._acts if (draw_next and self._acts is not None and self._acts.shape[1] == n_local) else None
        if costs.stride(-1) != 1 or not costs.is_contiguous():
            costs = costs.contiguous()
        el = fused.cem_update(costs, K, self._sampler(it, mu, sigma), H, a, self.st["alpha"], mu_out, sigma_out,
                              returns_out=returns_out, next_actions=nxt, draw_offset=n_offset)
        if el is None:
            self._fused_update = False
            return None
        self._drawn = (it + 1, n_offset, n_local) if nxt is not None else None
        return el

    def select(self, costs, K, returns_out):
        return fused.select(costs, K, returns_out=returns_out, workspace=self._sel_ws)

    def refit(self, it, mu, sigma, elites, mu_out, sigma_out):
        fused.refit(self._sampler(it, mu, sigma), self.st["H"], self.prob.mdesc["a"], elites, self.st["alpha"],
                    mu_out, sigma_out, workspace=self._refit_ws)

    def trajectory(self, actions):
        return fused.trajectory(self.prob, self.s0, actions, self.st["H"], workspace=self._traj_ws)


# RCCL process groups run the sharded plan as ONE C call per plan (mbrl_cem_plan_sharded: the
# all-gather is a step on the plan's stream); False, or a gloo group, runs cem_sharded_protocol's
# per-iteration Python loop (the same plan bit for bit)
SHARDED_NATIVE = True
_COMMS = {}


def _rccl_comm(dev, world, rank):
    """The library's RCCL communicator for this process group (created once, collectively: rank 0's
    unique id is broadcast through torch.distributed, then every rank joins)."""
    import ctypes
    import torch.distributed as dist
    key = (str(dev), world, rank, id(dist.distributed_c10d._get_default_group()))
    comm = _COMMS.get(key)
    if comm is None:
        lib = _lib.load()
        obj = [None]
        if rank == 0:
            buf = ctypes.create_string_buffer(_lib.MBRL_COMM_ID_BYTES)
            _lib.check(lib.mbrl_comm_unique_id(buf), "mbrl_comm_unique_id")
            obj[0] = buf.raw
        dist.broadcast_object_list(obj, src=0)
        comm = ctypes.c_void_p()
        rc = lib.mbrl_comm_init(ctypes.c_char_p(obj[0]), world, rank, ctypes.byref(comm))
        # every rank learns whether every rank joined: if one could not, all of them take the
        # per-iteration protocol over torch.distributed instead (the same plan, bit for bit)
        ok = torch.tensor([1 if rc == 0 else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            if rc == 0:
                lib.mbrl_comm_destroy(comm)
            msg = lib.mbrl_last_error() if rc else b"another rank"
            warnings.warn(f"mbrl_amd: RCCL communicator unavailable ({msg.decode(errors='replace')}); "
                          "sharded plans use the torch.distributed protocol")
            comm = False
        _COMMS[key] = comm
    return comm


_OWN_COMM = object()


def _cem_sharded_native(prob, s0, st, world, rank, comm=_OWN_COMM):
    """mbrl_cem_plan_sharded: this rank's shard of the plan, every iteration's all-gather included, in
    one C-ABI call on the current stream (the result is the single-GPU plan's, on every rank).
    comm: the library's RCCL communicator for the default group (default), or None under
    _lib.option("shard_emulate", 1 or 2), where the call fills every rank's slot itself (tests, timing).
    s0 on the host with neither records nor device outputs asked for: the plan reads s0 from and writes
    its outputs to mapped host staging (as _cem_plan_host); the call returns after the plan completed
    (it synchronises once for the peers' status words when world > 1), so no copy launch follows it.
    A failure on any rank raises RuntimeError on every rank (MBRL_EPEER on the healthy ones); the
    communicator stays usable."""
    lib = _lib.load()
    dev = prob.device
    md = prob.mdesc
    N, K, H, I = st["N"], st["K"], st["H"], st["I"]
    a, s, E = md["a"], md["s"], md["E"]
    pkey = ("sharded", world, N, H, K, I, st["alpha"], st["lo"], st["hi"], st["init_std"],
            int(st["seed"]) & 0xFFFFFFFFFFFFFFFF, lib.mbrl_get_option(_lib.OPTIONS["shard_emulate"]))
    _, pref, need = _plan_params(prob, pkey, lambda: _cem_params(st, pkey[10]),
                                 lib.mbrl_cem_plan_sharded_workspace_bytes, world)
    if need == 0:
        raise ValueError(f"num_candidates {N} must divide evenly over {world} ranks")
    ws = _workspace(("cem_sharded", str(dev)), need, dev)
    if comm is _OWN_COMM:
        comm = _rccl_comm(dev, world, rank)
    rec = st["record"]
    staged = HOST_STAGING and not st["keep"] and not rec and not s0.is_cuda
    if staged:
        arr, (p_s0, p_mu, p_sg, p_act, p_st) = _stage_in(dev, s0, H, s, a)
    else:
        s0 = s0.to(device=dev, dtype=torch.float32).contiguous()
        out = _device_outputs(dev, H, s, a)
        p_s0, (p_mu, p_sg, p_act, p_st) = _lib.ptr(s0), _output_ptrs(out)
    cost_hist, ret_hist, elite_hist = _cem_record_buffers(dev, rec, I, E, N, K)
    pev = st.get("plan_events")
    _mark(pev, 0)
    rc = lib.mbrl_cem_plan_sharded(*prob.refs, p_s0, pref, comm, world, rank, p_mu, p_sg, p_act, p_st,
                                   _lib.ptr(cost_hist), _lib.ptr(ret_hist), _lib.ptr(elite_hist), _events(st, I),
                                   _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
    # a failure after the argument checks still joined every all-gather of the plan, and every rank
    # learns of it (include/mbrl_cem.h): the communicator stays in step with the other ranks and is kept
    _lib.check(rc, "mbrl_cem_plan_sharded")
    _mark(pev, 1)
    if staged:
        if world == 1:     # (with peers the call has synchronised already)
            torch.cuda.current_stream(dev).synchronize()
        return _stage_out(arr, H, s, a)
    if rec:
        out.update(costs=cost_hist, returns=ret_hist, elites=elite_hist)
    return out


def _cem_fused_sharded(prob, s0, st, world):
    import torch.distributed as dist
    if SHARDED_NATIVE and dist.get_backend() == "nccl" and _rccl_comm(prob.device, world, dist.get_rank()):
        return _cem_sharded_native(prob, s0, st, world, dist.get_rank())
    st = dict(st, E=prob.mdesc["E"], a=prob.mdesc["a"])
    return cem_sharded_protocol(_FusedShardOps(prob, s0.to(device=prob.device, dtype=torch.float32).contiguous(), st),
                                st, world, dist.get_rank())


def _generic_plan(model, cost, s0, st, a, dev, mu, update, hist):
    """A sampling plan with opaque callables, from the initial mean `mu`: per iteration the HIP proposal
    draw, the callables on device tensors (_generic_costs), then the planner's own HIP
    update(sampler, costs, actions, mu_out, sigma_out); at the end the clipped mean and its predicted
    states. record=True: each iteration's costs and the dict `update` returned go into `hist`'s lists."""
    N, H, I = st["N"], st["H"], st["I"]
    sigma = torch.full((H, a), st["init_std"], dtype=torch.float32, device=dev)
    mu_n, sigma_n = torch.empty_like(mu), torch.empty_like(sigma)
    acts = torch.empty((H, N, a), dtype=torch.float32, device=dev)
    rec = st["record"]
    for it in range(I):
        sp = fused.make_sampler(st["seed"], it, mu, sigma, st["lo"], st["hi"])
        fused.sample_actions(sp, H, a, N, 0, acts)
        costs, _ = _generic_costs(model, cost, s0, acts, H, N)
        kept = update(sp, costs, acts, mu_n, sigma_n)
        mu, mu_n = mu_n, mu
        sigma, sigma_n = sigma_n, sigma
        if rec:
            hist["costs"].append(costs.clone())
            for k, v in kept.items():
                hist[k].append(v)
    actions = mu.clamp(st["lo"], st["hi"]).contiguous()
    _, states = _generic_costs(model, cost, s0, actions.view(H, 1, a), H, 1)
    out = dict(states=states[:, 0, :], actions=actions, mu=mu, sigma=sigma)
    if rec:
        out.update({k: torch.stack(v) for k, v in hist.items()})
    return out


def _cem_generic(model, cost, s0, st, a, dev):
    """CEM with opaque callables: HIP proposal draw, the callables on device tensors, HIP select/refit."""
    N, K, H = st["N"], st["K"], st["H"]

    def update(sp, costs, acts, mu_out, sigma_out):
        rets = torch.empty(N, dtype=torch.float32, device=dev)
        elites = fused.select(costs, K, returns_out=rets)
        fused.refit(sp, H, a, elites, st["alpha"], mu_out, sigma_out)
        return dict(returns=rets, elites=elites)
    return _generic_plan(model, cost, s0, st, a, dev, torch.zeros((H, a), dtype=torch.float32, device=dev), update,
                         dict(costs=[], returns=[], elites=[]))


# ------------------------------------------------------------------------------------------------
# MPPI
# ------------------------------------------------------------------------------------------------
def mppi_warm_start_rows(actions, horizon, shift, lo, hi):
    """The initial mean an MPPI plan starts from, given the previous plan's actions (host only, no
    device): rows [shift:] of `actions` (a [T, a] tensor / array, or a list of [1, a] / [a] rows as the
    gradient-descent planner returns them), the last row repeated to keep `horizon` rows (or cut to
    them), clipped to [lo, hi]. float32 [horizon, a]."""
    if isinstance(actions, (list, tuple)):
        actions = [np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32).reshape(1, -1)
                   for x in actions]
        rows = np.concatenate(actions, 0) if actions else np.zeros((0, 0), np.float32)
    else:
        x = actions.detach().cpu() if isinstance(actions, torch.Tensor) else actions
        rows = np.asarray(x, dtype=np.float32)
        rows = rows.reshape(rows.shape[0], -1) if rows.ndim >= 1 else rows.reshape(1, 1)
    H, shift = int(horizon), int(shift)
    if shift < 0:
        raise ValueError(f"shift must be >= 0, got {shift}")
    rows = rows[shift:]
    if rows.shape[0] == 0:
        raise ValueError(f"initial_trajectory has no action row left after dropping {shift}")
    if rows.shape[0] < H:
        rows = np.concatenate([rows, np.repeat(rows[-1:], H - rows.shape[0], 0)], 0)
    return np.clip(rows[:H], np.float32(lo), np.float32(hi)).astype(np.float32)


class MPPIPlanner(ModelPlanner):
    """Model-predictive path integral control (the information-theoretic update; not in the reference):
    I iterations of Philox proposal -> persistent MFMA rollout -> softmax-weighted refit, in which every
    candidate n contributes with weight exp(-(J_n - J_min) / temperature) (no elite cut), in the HIP
    extension (mbrl_mppi_plan; csrc/mppi.hip).

    kwargs (defaults): num_candidates (1000), num_iterations (1), temperature (1.0), alpha (0.0: the
    smoothing of CEMPlanner), update_sigma (False: classic MPPI keeps sigma; True refits it from the
    weighted variance), init_std (None -> (hi - lo) / 4), action_bounds (None -> from sample_action's
    action_spec, else (-1, 1)), seed (None -> drawn from the global NumPy RNG), shift (1),
    return_device (False), precision ("f32"), record (False).

    Warm start: `initial_trajectory` is honoured. Its action rows, after dropping the first `shift`
    and repeating the last to keep `horizon` rows, clipped to the bounds, are the initial mean
    (mppi_warm_start_rows), so MPCPolicy gets receding-horizon behaviour with one or two iterations per
    control step; shift=0 takes the rows as given, None starts from a zero mean.

    plan returns (predicted states of the clipped final mean, the clipped final mean); plan_detailed
    adds mu, sigma and, with record=True, costs [I, E, N], weights [I, N], mu_hist / sigma_hist
    [I + 1, H, a] (row 0 the initial distribution). distributed=True and this class's plan_batch are not
    implemented (NotImplementedError); the batched form is mppi_plan_batch / BatchedMPPIPlanner.

    MPPI over the K best (mbrl_mppi_plan_elite; the TD-MPC-style update, all off by default -- the defaults call
    exactly the entry above, bit for bit):
    num_elites (None): K in [1, num_candidates]. Only the K best candidates of an iteration (the stable top-K of
        the returns, ties to the lower index) are softmax-weighted; every other weight is 0. K = num_candidates
        is the classic update; a large temperature with K < N is CEM's elite mean.
    min_std (0.0), max_std (None -> +inf): with update_sigma the refitted sigma is clamped to [min_std, max_std],
        which keeps a warm-started episode from collapsing (or blowing up) the proposal width.
    warm_std (None): the initial std of a warm-started plan, as CEMPlanner's: None (init_std on every row), a
        float > 0, or "keep": the previous plan's sigma shifted like the mean (mppi_warm_start_rows(prev, H,
        shift, 0, inf)), given as plan_detailed(..., prev_sigma=); every entry finite and > 0, checked on the host.
    Naming min_std, max_std or warm_std without num_elites takes the same path with K = num_candidates.
    record=True then also returns elites [I, K] (int64, ascending candidate index per iteration). Bad values raise
    ValueError on the host before any device is looked for; warm_std with callables the fused path does not
    recognise is not implemented."""
    defaults = dict(num_candidates=1000, num_iterations=1, temperature=1.0, alpha=0.0, update_sigma=False,
                    init_std=None, action_bounds=None, seed=None, shift=1, return_device=False, precision="f32",
                    distributed=False)
    # the kwargs of the elite-restricted update, beside `defaults` (which other code may compare against)
    elite_defaults = dict(num_elites=None, min_std=0.0, max_std=None, warm_std=None)
    warm_starts = True

    @staticmethod
    def plan(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        res = MPPIPlanner.plan_detailed(initial_state, model, cost, sample_action, horizon, initial_trajectory,
                                        **kwargs)
        return res["states"], res["actions"]

    @staticmethod
    def plan_batch(initial_states, model, cost, sample_action, horizon, **kwargs):
        raise NotImplementedError("MPPIPlanner.plan_batch: batched MPPI plans are not implemented; call plan() per "
                                  "row, or use CEMPlanner.plan_batch")

    @staticmethod
    def _settings_build(sample_action, horizon, kwargs):
        d = MPPIPlanner.defaults
        g = lambda k: kwargs.get(k, d[k])  # noqa: E731
        if g("distributed"):
            raise NotImplementedError("MPPIPlanner: distributed=True (sharded MPPI) is not implemented; "
                                      "use CEMPlanner for multi-GPU plans")
        N, I = int(g("num_candidates")), int(g("num_iterations"))
        st = _common_settings(d, sample_action, horizon, kwargs)
        temperature = float(g("temperature"))
        if not (temperature > 0.0 and np.isfinite(temperature)):
            raise ValueError(f"temperature must be finite and > 0, got {temperature}")
        if N < 1 or I < 1:
            raise ValueError(f"need num_candidates ({N}) >= 1 and num_iterations ({I}) >= 1")
        st.update(N=N, I=I, temperature=temperature, update_sigma=bool(g("update_sigma")), shift=int(g("shift")))
        return st

    @staticmethod
    def _settings_full(sample_action, horizon, kwargs):
        """_settings_build's dict and, under "elite", the elite-restricted update's settings (_elite_settings)."""
        st = MPPIPlanner._settings_build(sample_action, horizon, kwargs)
        return dict(st, elite=MPPIPlanner._elite_settings(kwargs, st["N"]))

    @staticmethod
    def _elite_settings(kwargs, N):
        """dict(K, min_std, max_std, warm_std) of the elite-restricted update, or None when none of its kwargs
        is named (the plan then calls the classic entry untouched). Host only."""
        e = MPPIPlanner.elite_defaults
        ne, lo, hi, ws = (kwargs.get(k, e[k]) for k in ("num_elites", "min_std", "max_std", "warm_std"))
        if isinstance(ne, bool) or (ne is not None and int(ne) != ne):
            raise ValueError(f"num_elites must be an integer count, got {ne!r}")
        if ne is not None and not 1 <= int(ne) <= N:
            raise ValueError(f"need 1 <= num_elites ({int(ne)}) <= num_candidates ({N})")
        lo = float(lo)
        hi = float("inf") if hi is None else float(hi)
        if not (lo >= 0.0 and np.isfinite(lo)):
            raise ValueError(f"min_std must be finite and >= 0, got {lo}")
        if not hi >= lo:
            raise ValueError(f"max_std ({hi}) must be >= min_std ({lo})")
        if ws is not None and ws != "keep":
            ws = float(ws)
            if not (ws > 0.0 and np.isfinite(ws)):
                raise ValueError(f"warm_std must be finite and > 0, got {ws}")
        if ne is None and lo == 0.0 and hi == float("inf") and ws is None:
            return None
        return dict(K=N if ne is None else int(ne), min_std=lo, max_std=hi, warm_std=ws)

    @staticmethod
    def _sigma_rows(st, rows, prev_sigma):
        """The initial sigma rows of a warm-started plan (`rows`: its mean rows, or None) under warm_std, or
        None. Host only; finite and > 0 is checked here, as the C call cannot."""
        el = st["elite"]
        if el is None or el["warm_std"] is None or rows is None:
            return None
        if el["warm_std"] == "keep":
            if prev_sigma is None:
                raise ValueError('warm_std="keep" needs the previous plan\'s sigma: plan_detailed(..., prev_sigma=)')
            sig = mppi_warm_start_rows(prev_sigma, st["H"], st["shift"], 0.0, np.inf)
        else:
            sig = np.full(rows.shape, el["warm_std"], np.float32)
        if sig.shape != rows.shape:
            raise ValueError(f"prev_sigma gives {sig.shape} rows, the warm start {rows.shape}")
        if not (np.isfinite(sig).all() and (sig > 0).all()):
            raise ValueError("initial sigma rows must be finite and > 0")
        return sig

    @staticmethod
    def plan_detailed(initial_state, model, cost, sample_action, horizon, initial_trajectory=None, **kwargs):
        """plan() plus diagnostics: dict(states, actions, mu, sigma[, costs, weights, mu_hist, sigma_hist])."""
        _noise_refuse(kwargs, "MPPIPlanner")
        st = MPPIPlanner._settings_full(sample_action, horizon, kwargs)
        rows = None
        if initial_trajectory is not None:
            rows = mppi_warm_start_rows(initial_trajectory[1], st["H"], st["shift"], st["lo"], st["hi"])
        sig = MPPIPlanner._sigma_rows(st, rows, kwargs.get("prev_sigma"))
        dev = _device(kwargs)
        with _on_device(dev):
            mdesc, cdesc, prob = fused.describe_problem(model, cost, dev, st["precision"])
            if mdesc is not None and cdesc is not None:
                if rows is not None and rows.shape[1] != mdesc["a"]:
                    raise ValueError(f"initial_trajectory actions have {rows.shape[1]} dims, the model {mdesc['a']}")
                res = _mppi_fused_single(prob, initial_state, st, rows, sig)
            else:
                if st["elite"] is not None and st["elite"]["warm_std"] is not None:
                    raise NotImplementedError("MPPIPlanner: warm_std needs closures the fused path recognises")
                a = st["adim"] if rows is None else rows.shape[1]
                if a is None:
                    a = sample_action(batch_size=1).shape[1]
                res = _mppi_generic(model, cost, initial_state.to(device=dev, dtype=torch.float32).contiguous(), st,
                                    a, dev, rows)
            return _finish(res, st["keep"])


def _mppi_elite_params(st, mppi):
    el = st["elite"]
    return _lib.MppiEliteParams(mppi, el["K"], 0, el["min_std"], el["max_std"])


def _mppi_fused_single(prob, initial_state, st, rows, sig=None):
    """One C-ABI call: mbrl_mppi_plan, or mbrl_mppi_plan_elite with the elite-restricted settings (every
    iteration stream-ordered, no host sync)."""
    lib = _lib.load()
    dev = prob.device
    md = prob.mdesc
    N, H, I = st["N"], st["H"], st["I"]
    a, s, E = md["a"], md["s"], md["E"]
    el = st["elite"]
    pkey = ("mppi", N, H, I, st["update_sigma"], st["temperature"], st["alpha"], st["lo"], st["hi"], st["init_std"],
            int(st["seed"]) & 0xFFFFFFFFFFFFFFFF)

    def make_params():
        return _lib.MppiParams(N, H, I, int(st["update_sigma"]), st["temperature"], st["alpha"], st["lo"], st["hi"],
                               0.0, st["init_std"], pkey[-1])
    if el is not None:
        return _mppi_elite_single(lib, prob, initial_state, st, rows, sig, pkey, make_params)
    _, pref, need = _plan_params(prob, pkey, make_params, lib.mbrl_mppi_workspace_bytes)
    if need == 0:
        _lib.check(_lib.MBRL_EINVAL, "mbrl_mppi_workspace_bytes")
    ws = _workspace(("mppi", str(dev)), need, dev)
    s0 = initial_state.to(device=dev, dtype=torch.float32).contiguous()
    rows_d = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    out = _device_outputs(dev, H, s, a)
    rec = st["record"]
    cost_hist, w_hist, mu_hist, sg_hist = [torch.empty(sh, dtype=torch.float32, device=dev) if rec else None
                                           for sh in ((I, E, N), (I, N), (I + 1, H, a), (I + 1, H, a))]
    pev = st["plan_events"]
    _mark(pev, 0)
    _lib.check(lib.mbrl_mppi_plan(*prob.refs, _lib.ptr(s0), pref, _lib.ptr(rows_d), *_output_ptrs(out),
                                  _lib.ptr(cost_hist), _lib.ptr(w_hist), _lib.ptr(mu_hist), _lib.ptr(sg_hist),
                                  _events(st, I), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)), "mbrl_mppi_plan")
    _mark(pev, 1)
    if rec:
        out.update(costs=cost_hist, weights=w_hist, mu_hist=mu_hist, sigma_hist=sg_hist)
    return out


def _mppi_elite_single(lib, prob, initial_state, st, rows, sig, pkey, make_params):
    """mbrl_mppi_plan_elite: the plan above with the selection before each update, the clamp and sigma rows."""
    dev = prob.device
    md = prob.mdesc
    N, H, I = st["N"], st["H"], st["I"]
    a, s, E = md["a"], md["s"], md["E"]
    el = st["elite"]
    K = el["K"]
    ekey = ("mppi_elite", K, el["min_std"], el["max_std"]) + pkey[1:]
    _, pref, need = _plan_params(prob, ekey, lambda: _mppi_elite_params(st, make_params()),
                                 lib.mbrl_mppi_elite_workspace_bytes, 1)
    if need == 0:
        _lib.check(_lib.MBRL_EINVAL, "mbrl_mppi_elite_workspace_bytes")
    ws = _workspace(("mppi_elite", str(dev)), need, dev)
    s0 = initial_state.to(device=dev, dtype=torch.float32).contiguous()
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    rows_d, sig_d = up(rows), up(sig)
    out = _device_outputs(dev, H, s, a)
    rec = st["record"]
    cost_hist, w_hist, mu_hist, sg_hist = [torch.empty(sh, dtype=torch.float32, device=dev) if rec else None
                                           for sh in ((I, E, N), (I, N), (I + 1, H, a), (I + 1, H, a))]
    el_hist = torch.empty((I, K), dtype=torch.int64, device=dev) if rec else None
    pev = st["plan_events"]
    _mark(pev, 0)
    _lib.check(lib.mbrl_mppi_plan_elite(*prob.refs, _lib.ptr(s0), pref, _lib.ptr(rows_d), _lib.ptr(sig_d),
                                        *_output_ptrs(out), _lib.ptr(cost_hist), _lib.ptr(w_hist), _lib.ptr(mu_hist),
                                        _lib.ptr(sg_hist), _lib.ptr(el_hist), _events(st, I), _lib.ptr(ws), ws.numel(),
                                        _lib.stream_handle(dev)), "mbrl_mppi_plan_elite")
    _mark(pev, 1)
    if rec:
        out.update(costs=cost_hist, weights=w_hist, mu_hist=mu_hist, sigma_hist=sg_hist, elites=el_hist)
    return out


def _mppi_generic(model, cost, s0, st, a, dev, rows):
    """MPPI with opaque callables: HIP proposal draw, the callables on device tensors, then the HIP
    weighted update (mbrl_mppi_update), as selection and refit stay in the extension for CEM."""
    N, H = st["N"], st["H"]
    rec = st["record"]
    if rows is None:
        mu = torch.zeros((H, a), dtype=torch.float32, device=dev)
    else:
        mu = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)

    el = st["elite"]

    def update(sp, costs, acts, mu_out, sigma_out):
        wts = torch.empty(N, dtype=torch.float32, device=dev) if rec else None
        kept = {}
        if el is None:
            fused.mppi_update(costs, acts, sp, H, a, st["temperature"], st["alpha"], st["update_sigma"], mu_out,
                              sigma_out, weights_out=wts)
        else:
            kept["elites"] = fused.mppi_update_elite(costs, acts, sp, el["K"], H, a, st["temperature"], st["alpha"],
                                                     st["update_sigma"], mu_out, sigma_out, sigma_min=el["min_std"],
                                                     sigma_max=el["max_std"], weights_out=wts)
        return dict(kept, weights=wts, mu_hist=mu_out.clone(), sigma_hist=sigma_out.clone()) if rec else None
    sigma0 = torch.full((H, a), st["init_std"], dtype=torch.float32, device=dev)     # (row 0 of sigma_hist)
    hist = dict(costs=[], weights=[], mu_hist=[mu.clone()], sigma_hist=[sigma0])
    if el is not None:
        hist["elites"] = []
    return _generic_plan(model, cost, s0, st, a, dev, mu, update, hist)


def mppi_plan_batch(initial_states, model, cost, sample_action, horizon, initial_trajectories=None, prev_sigmas=None,
                    **kwargs):
    """B independent MPPI plans in shared launches (mbrl_mppi_plan_batch): one per row of initial_states
    [B, s], each with its own warm start, so one GPU planner serves B environments that are each somewhere in
    their own episode. kwargs as MPPIPlanner.plan; num_candidates is per problem. initial_trajectories is a list
    of B entries, each None (that problem starts from a zero mean: its first control step) or (states, actions)
    of its previous plan, shifted per row with mppi_warm_start_rows. Problem b draws its proposals as
    candidates [b*N, (b+1)*N) of one Philox stream; problem 0 is MPPIPlanner.plan_detailed bit for bit.

    Returns a dict: states [B, H, s], actions, mu, sigma [B, H, a]; record=True adds costs [I, E, B*N],
    weights [I, B, N] and mu_hist / sigma_hist [I + 1, B, H, a]. Host tensors unless return_device.
    distributed, noise_beta and noise_mix are refused as MPPIPlanner refuses them, and a list that is not B
    long raises ValueError, before anything touches the device. Closures the fused path does not recognise
    fall back to one MPPIPlanner plan per row.

    num_elites, min_std, max_std and warm_std as MPPIPlanner's (mbrl_mppi_plan_elite_batch: one segmented selection
    and one update launch per iteration whatever B is); prev_sigmas (warm_std="keep") is a list of B entries, the
    previous plan's sigma of each warm-started problem (a None entry: that problem starts from init_std). record=True then adds elites [I, B, K] (local indices)."""
    _noise_refuse(kwargs, "mppi_plan_batch")
    st = MPPIPlanner._settings_full(sample_action, horizon, kwargs)
    B = int(initial_states.shape[0])
    if B < 1:
        raise ValueError("mppi_plan_batch needs at least one initial state")
    inits = _per_row(initial_trajectories, B, "initial_trajectories")
    rows = [None if x is None else mppi_warm_start_rows(x[1], st["H"], st["shift"], st["lo"], st["hi"]) for x in inits]
    if "prev_sigma" in kwargs:
        raise ValueError("mppi_plan_batch takes prev_sigmas, one entry per problem, not prev_sigma")
    el = st["elite"]
    # with a prev_sigmas list, a warm-started problem whose entry is None starts from init_std (mixed flags)
    skip = prev_sigmas is not None and el is not None and el["warm_std"] == "keep"
    sigs = [None if skip and ps is None else MPPIPlanner._sigma_rows(st, r, ps)
            for r, ps in zip(rows, _per_row(prev_sigmas, B, "prev_sigmas"))]
    dev = _device(kwargs)
    keep, rec = st["keep"], st["record"]
    with torch.cuda.device(dev):
        mdesc, cdesc, prob = fused.describe_problem(model, cost, dev, st["precision"])
        if mdesc is None or cdesc is None:
            kw = dict(kwargs, seed=st["seed"], return_device=True)
            outs = [MPPIPlanner.plan_detailed(initial_states[b], model, cost, sample_action, horizon, inits[b], **kw)
                    for b in range(B)]
            out = {k: torch.stack([o[k] for o in outs]) for k in ("states", "actions", "mu", "sigma")}
            if rec:
                hists = ("weights", "mu_hist", "sigma_hist") + (("elites",) if el is not None else ())
                out.update(costs=torch.cat([o["costs"] for o in outs], 2),
                           **{k: torch.stack([o[k] for o in outs], 1) for k in hists})
            return {k: _to_host(v, keep) for k, v in out.items()}
        lib = _lib.load()
        N, H, I = st["N"], st["H"], st["I"]
        a, s, E = mdesc["a"], mdesc["s"], mdesc["E"]
        for b, r in enumerate(rows):
            if r is not None and r.shape[1] != a:
                raise ValueError(f"row {b}: initial_trajectory actions have {r.shape[1]} dims, the model {a}")
        rows_d = flags_d = None
        if any(r is not None for r in rows):
            stacked = np.stack([np.zeros((H, a), np.float32) if r is None else r for r in rows])
            rows_d = torch.from_numpy(np.ascontiguousarray(stacked)).to(dev)
            flags_d = torch.tensor([0 if r is None else RH_FLAG_MU for r in rows], dtype=torch.int32).to(dev)
        params = _lib.MppiParams(N, H, I, int(st["update_sigma"]), st["temperature"], st["alpha"], st["lo"], st["hi"],
                                 0.0, st["init_std"], int(st["seed"]) & 0xFFFFFFFFFFFFFFFF)
        s0 = initial_states.to(device=dev, dtype=torch.float32).reshape(B, s).contiguous()
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)  # noqa: E731
        out = dict(states=e(B, H, s), actions=e(B, H, a), mu=e(B, H, a), sigma=e(B, H, a))
        if rec:
            out.update(costs=e(I, E, B * N), weights=e(I, B, N), mu_hist=e(I + 1, B, H, a), sigma_hist=e(I + 1, B, H, a))
        g = lambda k: _lib.ptr(out.get(k))  # noqa: E731
        if el is not None:
            sig_d = None
            if any(x is not None for x in sigs):
                stacked = np.stack([np.ones((H, a), np.float32) if x is None else x for x in sigs])
                sig_d = torch.from_numpy(np.ascontiguousarray(stacked)).to(dev)
                flags = [(0 if r is None else RH_FLAG_MU) | (0 if x is None else RH_FLAG_SIGMA) for r, x in zip(rows, sigs)]
                flags_d = torch.tensor(flags, dtype=torch.int32).to(dev)
            eparams = _mppi_elite_params(st, params)
            need = lib.mbrl_mppi_elite_workspace_bytes(fused.ctypes_ref(prob.shape), fused.ctypes_ref(eparams), B)
            if need == 0:
                _lib.check(_lib.MBRL_EINVAL, "mbrl_mppi_elite_workspace_bytes")
            ws = _workspace(("mppi_elite_batch", str(dev)), need, dev)
            if rec:
                out["elites"] = torch.empty((I, B, el["K"]), dtype=torch.int64, device=dev)
            _lib.check(lib.mbrl_mppi_plan_elite_batch(*prob.refs, _lib.ptr(s0), B, fused.ctypes_ref(eparams),
                                                      _lib.ptr(rows_d), _lib.ptr(sig_d), _lib.ptr(flags_d), g("mu"),
                                                      g("sigma"), g("actions"), g("states"), g("costs"), g("weights"),
                                                      g("mu_hist"), g("sigma_hist"), g("elites"), _lib.ptr(ws),
                                                      ws.numel(), _lib.stream_handle(dev)), "mbrl_mppi_plan_elite_batch")
            return {k: _to_host(v, keep) for k, v in out.items()}
        need = lib.mbrl_mppi_batch_workspace_bytes(fused.ctypes_ref(prob.shape), fused.ctypes_ref(params), B)
        if need == 0:
            _lib.check(_lib.MBRL_EINVAL, "mbrl_mppi_batch_workspace_bytes")
        ws = _workspace(("mppi_batch", str(dev)), need, dev)
        _lib.check(lib.mbrl_mppi_plan_batch(*prob.refs, _lib.ptr(s0), B, fused.ctypes_ref(params), _lib.ptr(rows_d),
                                            _lib.ptr(flags_d), g("mu"), g("sigma"), g("actions"), g("states"),
                                            g("costs"), g("weights"), g("mu_hist"), g("sigma_hist"), _lib.ptr(ws),
                                            ws.numel(), _lib.stream_handle(dev)), "mbrl_mppi_plan_batch")
        return {k: _to_host(v, keep) for k, v in out.items()}


class BatchedMPPIPlanner(MPPIPlanner):
    """MPPIPlanner with a batched form, so the planner service (parallel.get_rollouts_parallel) answers a whole
    round of requests with one mppi_plan_batch call and warm-starts every rollout it serves from that rollout's
    own previous plan. plan() is MPPIPlanner.plan."""
    # the planner service passes each rollout's previous plan (initial_trajectories)
    warm_starts = True

    @staticmethod
    def plan_batch(initial_states, model, cost, sample_action, horizon, initial_trajectories=None, **kwargs):
        """B plans at once; returns (states [B, H, s], actions [B, H, a]). num_elites, min_std, max_std and a
        numeric warm_std pass through (mppi_plan_batch); warm_std="keep" needs prev_sigmas, which the planner
        service does not carry for this planner."""
        res = mppi_plan_batch(initial_states, model, cost, sample_action, horizon, initial_trajectories, **kwargs)
        return res["states"], res["actions"]
