"""CPU: batched receding-horizon CEM on the host -- the gap condition that lets the GPU test
(tests/test_gpu_cem_rh_batch.py) demand identical index sets from every problem of every fixture batch, the
batched restatement (tests/cem_rh_batch_reference.py) against the single plan's, cem_plan_batch_rh's per-row
input building and host checks, RecedingHorizonCEMPlanner's memo shifting and the planner service's memo
protocol. No GPU."""
import numpy as np
import pytest
import torch

import cem_rh_batch_reference as br
import cem_rh_reference as rh

F32 = np.float32
H, K, I = br.SMALL["H"], br.SMALL["K"], br.SMALL["I"]


def test_fixture_table_covers_every_axis():
    cases = br.CASES
    assert {(c[0], c[1]) for c in cases} == {(64, 1), (256, 2)}
    assert {c[2] for c in cases} == {1, 5, 8} and {c[3] for c in cases} == {64, 100}
    assert {c[4] for c in cases} == {1, 2} and {c[5] for c in cases} == {0, 1, 3, 8}
    assert {len(c[6]) for c in cases} == {1, 2, 3, 5}
    full = lambda Kc: "msc" if Kc else "ms"  # noqa: E731
    assert any(all(x == full(c[5]) for x in c[6]) for c in cases)           # all given
    assert any(all(x == "" for x in c[6]) for c in cases)                   # none given
    # mixed per-problem flags: problem 0 cold and a later one warm with carry, and the other way round
    assert any(c[6][0] == "" and any("c" in x for x in c[6][1:]) for c in cases)
    assert any("c" in c[6][0] and any(x == "" for x in c[6][1:]) for c in cases)


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_fixture_gaps_exceed_ten_times_the_return_bar(case):
    Kc = case[5]
    for b, res in enumerate(br.cached_plans(case)):
        gap = rh.case_gaps(res, K, Kc)
        print(f"{br.case_id(case)} problem {b}: smallest gap {gap:.3g}")
        assert gap > br.GAP_MIN, (b, gap)


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_problem_zero_of_the_restatement_is_the_single_plans(case):
    W, L, a, N, E, Kc, inputs, _ = case
    p, s0s, kws = br.make_case(case)
    assert np.array_equal(s0s[0], p["s0"])
    ref = rh.plan(p, N, H, K, I, keep=Kc, **kws[0])
    got = br.cached_plans(case)[0]
    for k in ("costs", "returns", "elites", "best", "actions", "mu", "sigma", "kept"):
        for x, y in zip(got[k], ref[k]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), k
    for k in ("mu_out", "sigma_out", "carry", "carry_returns", "final_actions", "final_states"):
        assert got[k].tobytes() == ref[k].tobytes(), k


def test_a_later_problem_draws_from_its_own_counters():
    """Problem b > 0 with problem 0's state and inputs still differs: its candidates are b N + n."""
    case = br.CASES[10]
    W, L, a, N, E, Kc, inputs, _ = case
    p, s0s, kws = br.make_case(case)
    p0 = br.plan_problem(p, p["s0"], 0, N, H, K, I, keep=Kc, final=False)
    p1 = br.plan_problem(p, p["s0"], 1, N, H, K, I, keep=Kc, final=False)
    from oracle.philox import cem_actions
    assert np.array_equal(p1["actions"][0], cem_actions(p1["mu0"], p1["sigma0"], -1.0, 1.0, p["rng_seed"], 0,
                                                        N + np.arange(N)))
    assert not np.array_equal(p0["actions"][0], p1["actions"][0])


# ---- cem_plan_batch_rh's host side
def _settings(**kw):
    from mbrl_amd.planners import CEMPlanner
    kw = dict(dict(num_candidates=64, num_elites=8, num_iterations=3, seed=5), **kw)
    return CEMPlanner._settings(None, H, kw), kw


def test_batch_inputs_are_built_per_row_with_flag_bits():
    from mbrl_amd.planners import (RH_FLAG_CARRY, RH_FLAG_MU, RH_FLAG_SIGMA, _rh_batch_inputs, cem_shift_carry,
                                   mppi_warm_start_rows)
    assert (RH_FLAG_MU, RH_FLAG_SIGMA, RH_FLAG_CARRY) == (br.FLAG_MU, br.FLAG_SIGMA, br.FLAG_CARRY) == (1, 2, 4)
    a, Kc = 2, 3
    rng = np.random.default_rng(0)
    prev = [rng.uniform(-1.5, 1.5, (H, a)).astype(F32) for _ in range(3)]
    sig = [rng.uniform(0.1, 0.6, (H, a)).astype(F32) for _ in range(3)]
    car = [cem_shift_carry(rng.uniform(-1.2, 1.2, (Kc, H, a)).astype(F32), 1) for _ in range(3)]
    st, kw = _settings(warm_start=True, warm_std="keep", keep_elites=Kc)
    # row 0: its first control step (nothing); row 1: everything; row 2: a warm start without a carry
    got = _rh_batch_inputs(st, 3, [None, (None, torch.from_numpy(prev[1])), (None, prev[2])], [None, car[1], None],
                           [None, sig[1], sig[2]], kw)
    assert got["Kc"] == Kc and got["flags"].dtype == np.int32
    assert got["flags"].tolist() == [0, RH_FLAG_MU | RH_FLAG_SIGMA | RH_FLAG_CARRY, RH_FLAG_MU | RH_FLAG_SIGMA]
    assert got["mu_rows"].shape == (3, H, a) and got["sigma_rows"].shape == (3, H, a)
    assert got["carry"].shape == (3, Kc, H, a) and got["mu_rows"].dtype == np.float32
    for b in (1, 2):
        assert np.array_equal(got["mu_rows"][b], mppi_warm_start_rows(prev[b], H, 1, -1.0, 1.0))
        assert np.array_equal(got["sigma_rows"][b], mppi_warm_start_rows(sig[b], H, 1, 0.0, np.inf))
    assert np.array_equal(got["carry"][1], car[1])
    assert np.isfinite(got["sigma_rows"][0]).all() and (got["sigma_rows"][0] > 0).all()   # (filler, flagged off)
    # nothing given at all: no pointers, no flags; the keep count still resolves
    none = _rh_batch_inputs(st, 2, None, None, None, kw)
    assert none["mu_rows"] is None and none["sigma_rows"] is None and none["carry"] is None and none["flags"] is None
    assert none["Kc"] == Kc
    # warm_start off: a given trajectory is ignored, a carry still counts
    st0, kw0 = _settings(keep_elites=Kc)
    only = _rh_batch_inputs(st0, 2, [(None, prev[0]), None], [None, car[1]], None, kw0)
    assert only["mu_rows"] is None and only["flags"].tolist() == [0, RH_FLAG_CARRY]
    # a fractional keep_elites is a fraction of num_elites
    stf, kwf = _settings(keep_elites=0.3)
    assert _rh_batch_inputs(stf, 1, None, None, None, kwf)["Kc"] == 2


def test_host_checks_raise_value_error_before_any_device_work():
    from mbrl_amd.planners import _rh_batch_inputs, cem_plan_batch_rh
    a, Kc = 2, 3
    ok_sig, prev = np.full((H, a), 0.3, F32), np.zeros((H, a), F32)
    st, kw = _settings(warm_start=True, warm_std="keep", keep_elites=Kc)
    s0 = torch.zeros(2, 5)
    for bad in (0.0, -0.1, np.nan, np.inf):
        sig = ok_sig.copy()
        sig[1, 0] = bad
        with pytest.raises(ValueError, match="finite and > 0"):
            _rh_batch_inputs(st, 2, [(None, prev), (None, prev)], None, [ok_sig, sig], kw)
        with pytest.raises(ValueError, match="finite and > 0"):    # the public entry: raised before it needs a GPU
            cem_plan_batch_rh(s0, None, None, None, H, [(None, prev), (None, prev)], None, [ok_sig, sig], **kw)
    for shape in ((Kc - 1, H, a), (Kc, H + 1, a), (Kc * H, a)):
        with pytest.raises(ValueError, match="carry must be"):
            cem_plan_batch_rh(s0, None, None, None, H, None, [None, np.zeros(shape, F32)], None, **kw)
    with pytest.raises(ValueError, match="action dims"):          # rows that disagree on the action dimension
        _rh_batch_inputs(st, 2, None, [np.zeros((Kc, H, a), F32), np.zeros((Kc, H, a + 1), F32)], None, kw)
    with pytest.raises(ValueError, match="entries for 2"):
        cem_plan_batch_rh(s0, None, None, None, H, [None], None, None, **kw)
    with pytest.raises(ValueError, match="keep_elites == 0"):
        cem_plan_batch_rh(s0, None, None, None, H, None, [np.zeros((1, H, a), F32), None], None, num_candidates=64)
    with pytest.raises(ValueError, match="prev_sigma"):           # warm_std="keep" without that row's sigma
        cem_plan_batch_rh(s0, None, None, None, H, [(None, prev), None], None, None, **kw)
    with pytest.raises(NotImplementedError, match="distributed"):
        cem_plan_batch_rh(s0, None, None, None, H, distributed=True)
    with pytest.raises(TypeError, match="carries"):
        cem_plan_batch_rh(s0, None, None, None, H, carry=np.zeros((Kc, H, a), F32), **kw)


def test_receding_horizon_planner_attributes_and_memo_shifting():
    from mbrl_amd import CEMPlanner, RecedingHorizonCEMPlanner, cem_shift_carry
    P = RecedingHorizonCEMPlanner
    assert issubclass(P, CEMPlanner) and P.warm_starts is True and P.plan_memo is True
    assert not hasattr(CEMPlanner, "warm_starts") and not hasattr(CEMPlanner, "plan_memo")
    assert P._kwargs({}) == dict(warm_start=True, keep_elites=0.3)
    assert P._kwargs(dict(keep_elites=0, seed=1)) == dict(warm_start=True, keep_elites=0, seed=1)
    rng = np.random.default_rng(1)
    carry = torch.from_numpy(rng.uniform(-1.4, 1.4, (2, H, 3)).astype(F32))
    sigma = torch.from_numpy(rng.uniform(0.1, 0.5, (H, 3)).astype(F32))
    carries, sigmas = P._memo_inputs([None, dict(carry=carry, sigma=sigma), dict(carry=None, sigma=sigma)], 3, 1,
                                     -1.0, 1.0)
    assert carries[0] is None and sigmas[0] is None and carries[2] is None and sigmas[2] is sigma
    assert np.array_equal(carries[1], cem_shift_carry(carry, 1, -1.0, 1.0))
    want = np.clip(np.concatenate([carry.numpy()[:, 1:], carry.numpy()[:, -1:]], 1), -1.0, 1.0)
    assert np.array_equal(carries[1], want) and sigmas[1] is sigma     # (the warm start shifts sigma with the mean)
    assert np.array_equal(P._memo_inputs([dict(carry=carry, sigma=sigma)], 1, 2, -0.5, 0.5)[0][0],
                          cem_shift_carry(carry, 2, -0.5, 0.5))
    with pytest.raises(ValueError, match="entries for 2"):
        P._memo_inputs([None], 2, 1, -1.0, 1.0)
    assert P._memo_inputs(None, 2, 1, -1.0, 1.0) == ([None, None], [None, None])


# ---- the planner service's memo protocol (parallel._answer), with stand-in planners
class _Conn:
    def __init__(self):
        self.sent = []

    def send(self, x):
        self.sent.append(x)


class _Policy:
    model = cost = sample_action = None
    horizon = 4

    def __init__(self, planner):
        self.planner = planner
        self.plan_kwargs = dict(marker=7)


def _round(parallel, policy, requests, conns, last, memos):
    """One _answer round; requests: worker -> (rollout index, timestep)."""
    pending = {w: (i, t, None, np.full(3, 10.0 * i + t, F32)) for w, (i, t) in requests.items()}
    parallel._answer(policy, pending, conns, {}, None, last, memos)


def test_service_hands_each_rollout_its_own_memo_back():
    from mbrl_amd import parallel
    calls = []

    class Memo:
        plan_memo = True
        warm_starts = True

        @staticmethod
        def plan_batch(obs, model, cost, sample_action, horizon, initial_trajectories=None, memos=None, **kw):
            B = obs.shape[0]
            assert kw == dict(marker=7) and len(memos) == B and len(initial_trajectories) == B
            calls.append((obs.clone(), list(memos), list(initial_trajectories)))
            n = len(calls)
            states, actions = torch.zeros(B, horizon, 3), obs[:, :1].reshape(B, 1, 1).repeat(1, horizon, 2) + n
            # the memo names the rollout (from its observation's tens digit) and the round it was made in
            return states, actions, [dict(rollout=int(obs[b, 0]) // 10, round=n) for b in range(B)]

    pol = _Policy(Memo)
    conns = {w: _Conn() for w in range(3)}
    last, memos = {}, {}
    # round 1: rollouts 0, 1 at timestep 0 (answered in rollout order whatever the worker order)
    _round(parallel, pol, {1: (0, 0), 0: (1, 0)}, conns, last, memos)
    assert calls[-1][1] == [None, None] and calls[-1][2] == [None, None]
    assert calls[-1][0][:, 0].tolist() == [0.0, 10.0]
    # round 2: both at timestep 1 -> each gets the memo it returned in round 1
    _round(parallel, pol, {1: (0, 1), 0: (1, 1)}, conns, last, memos)
    assert calls[-1][1] == [dict(rollout=0, round=1), dict(rollout=1, round=1)]
    assert all(x is not None for x in calls[-1][2])
    # round 3: rollout 1 goes on (timestep 2), worker 1 starts rollout 2 at timestep 0 -> None for it
    _round(parallel, pol, {1: (2, 0), 0: (1, 2)}, conns, last, memos)
    assert calls[-1][1] == [dict(rollout=1, round=2), None] and calls[-1][2][1] is None
    # round 4: rollout 2 alone at timestep 1: its own memo, from round 3
    _round(parallel, pol, {1: (2, 1)}, conns, last, memos)
    assert calls[-1][1] == [dict(rollout=2, round=3)]
    # a rollout index that starts again (timestep 0) forgets its memo
    _round(parallel, pol, {2: (1, 0)}, conns, last, memos)
    assert calls[-1][1] == [None]
    # every worker got its action: row 0 of its problem's plan
    assert len(conns[0].sent) == 3 and len(conns[1].sent) == 4 and len(conns[2].sent) == 1
    assert conns[1].sent[0].tolist() == [1.0, 1.0]          # rollout 0, round 1: obs 0 + 1


def test_service_calls_planners_without_plan_memo_as_before():
    from mbrl_amd import parallel
    seen = []

    class Plain:
        @staticmethod
        def plan_batch(obs, model, cost, sample_action, horizon, **kw):
            seen.append(dict(kw))
            B = obs.shape[0]
            return torch.zeros(B, horizon, 3), torch.ones(B, horizon, 2)

    class Warm(Plain):
        warm_starts = True

    conns = {0: _Conn(), 1: _Conn()}
    for planner in (Plain, Warm):
        last, memos = {}, {}
        for t in (0, 1):
            _round(parallel, _Policy(planner), {0: (0, t), 1: (1, t)}, conns, last, memos)
        assert memos == {}
    assert all("memos" not in kw for kw in seen)
    assert [sorted(kw) for kw in seen] == [["marker"], ["marker"], ["initial_trajectories", "marker"],
                                           ["initial_trajectories", "marker"]]
    # and without the new argument at all (the call as it was before memos existed)
    pending = {0: (0, 0, None, np.zeros(3, F32))}
    parallel._answer(_Policy(Plain), pending, conns, {}, None, {})
