"""The single-trajectory kernels over their whole instance envelope on the GPU: every case of
tests/traj_cases.py, whose coverage of the 20 traj_reg_kernel and 8 traj_coop_kernel instances, both
cooperative grids, the four MBRL_OPT_TRAJ_HOP values and each dispatch threshold
tests/test_traj_cases_host.py proves on the CPU.

Every case calls the raw mbrl_trajectory (test_gpu_flags.trajectory) on a workspace of its own, exactly the
size query's bytes and pre-filled with the byte 0xA5, and on outputs pre-filled with a NaN payload.

Values. Per-member states against the float64 rollout (rollout_cases.rollout_f64) at two bars: the suite's
rtol = atol = 1e-4, and the tight absolute bar traj_cases.TIGHT = 32 D = 4.8e-6, D = 1.5e-7 being the float32
oracle's own worst distance from float64 over the table (asserted on the CPU). The member mean must equal,
bit for bit, (m_0 + m_1 + ...) / E summed sequentially in float32 over the GPU's own member states (the
oracle's definition), and meet the same two bars against the float64 mean.

Which kernel ran is observed, not only modelled. The workspace begins with the hand-off block (E * 2 * Wpad
u64 granules {tag, value}, then the status word): after a register or an ungated plain case it still holds
0xA5 everywhere; after a cooperative case the status word is 0 and the granules of the two parity buffers of
every member carry the tags of the last two phases, H (L - 1) and H (L - 1) - 1, each in the buffer of its
parity (the cooperative kernel finished every phase, and the fallback behind it left at its gate: it would
not have changed the granules, but the states are the cooperative kernel's, see the hop test); after an
abort case (MBRL_OPT_DEBUG_TRAJ_ABORT) the status word is set, every tag is still the memset's 0 and the
states, now the gated plain kernel's, still match.

Hop modes. The states under traj_hop 1, 2 and 3 equal those under 0 bit for bit, on both grids, at K0R = 32
and 96, at E = 1, 5, 8 and 9 (include/mbrl_cem.h promises "same results").

Plans. A two-iteration CEMPlanner.plan_detailed at N <= 64 on a register shape, a narrow K0R = 96
cooperative shape and the shape one step past the register kernel's H a limit: the plan's states equal, bit
for bit, a standalone mbrl_trajectory of the returned actions (the plan's pre-zeroed hand-off block against
the standalone call's memset).

Measured on an MI355X (max abs error against float64 over all members, steps and state dims; every
instance's figure is in profiles/traj_envelope/errors.json, written by measure_all() below). Worst per family:
  traj_reg_kernel   1.56e-7  (<256, 0, 32>, r256_n0_k32; 9.0e-8 after 1004 steps, line64_reg)
  traj_coop_kernel  1.07e-7  (<96, 5, 4> on the full per-XCD grid, c96_w4_E8; 8.8e-8 after 1005 steps, line64_coop,
                              the same figure under every hop option; 9.9e-8 after 665 steps, line128_coop)
  traj_kernel       1.28e-7  (plain_PE_1028, 257 members)
All of them are the size of D, about 3 % of the tight bar: no instance sits between the tight bar and 1e-4,
so none needs an explanation from its summation order.

What the tests notice, tried once on libraries with one in-bounds index mistake each (never committed): a
hidden-layer column shifted by one in traj_reg_kernel<128, 2, 8> alone fails r128_n2_k8_E3 and nothing else;
an output-layer column shifted in traj_coop_kernel<96, 5, 2> alone fails the three c96_w2_* cases and their
hop tests and nothing else; two rows swapped in the cooperative kernel's slice staging (shared by the eight
instances) fails all 13 cooperative cases and the 8 hop tests, no register or plain case; a shifted column
in traj_kernel's output layer fails the three plain and the three abort cases only. Zeroing a `k < W` / `r < W`
guard is not such a mistake: the pack zero-pads what those guards skip and the activations past W are exact
zeros, so the result does not change (the guards keep the loads inside the member's weights). The plan test
compares two runs of one library bit for bit, so it notices a difference between the plan's path and the
standalone call's, not a mistake both share.
"""
import functools
import json

import numpy as np
import pytest
import torch

import rollout_dispatch_model as rdm
import traj_cases as tc
from test_gpu_flags import trajectory
from test_gpu_parity import DEV, build, device_problem

pytestmark = pytest.mark.gpu
WS_BYTE = 0xA5
OUT_SENTINEL = 0x7FC5A5A5        # a quiet NaN with a payload no computation produces


@functools.lru_cache(maxsize=None)
def _packed(cid):
    """The case's DeviceProblem, packed once."""
    return device_problem(tc.problem(cid))


def _alloc(*shape, dt=torch.float32):
    t = torch.empty(shape, dtype=dt, device=DEV)
    t.view(torch.int32).fill_(OUT_SENTINEL)
    return t


def run(case, hop=0, acts=None):
    """mbrl_trajectory on a 0xA5-filled workspace of exactly the size query's bytes and sentinel-filled
    outputs: (mean states [H, s], member states [E, H, s], the workspace's bytes afterwards), on the host."""
    held = []

    def make_ws(n):
        assert n > 0, "the size query refused the case"
        held.append(torch.full((n,), WS_BYTE, dtype=torch.uint8, device=DEV))
        return held[-1]

    opts = {"traj_hop": hop}
    if case.abort:
        opts["debug_traj_abort"] = 1
    acts = tc.actions(case.id) if acts is None else acts
    states, members = trajectory(_packed(case.id), tc.problem(case.id), acts, opts, make_ws=make_ws, alloc=_alloc)
    assert len(held) == 1
    out = states.cpu().numpy(), members.cpu().numpy(), held[0].cpu().numpy()
    for x in out[:2]:
        assert not (x.view(np.int32) == np.int32(OUT_SENTINEL)).any(), (case.id, "an output element was never written")
    return out


def check_workspace(case, inst, ws):
    """What the hand-off block at the head of the workspace says about the kernels that ran."""
    E, L, H = case.shape["E"], case.shape["L"], case.H
    Wp = rdm.geometry(case.shape["s"], case.shape["a"], case.shape["W"], L, E)["Wpad"]
    xb = E * 2 * Wp * 8                                     # take_traj_scratch: the granules, then 16 status bytes
    assert xb % 256 == 0 and ws.size == xb + 256 + -(-E * H * case.shape["s"] * 4 // 256) * 256, (case.id, ws.size)
    head, status, rest = ws[:xb], ws[xb:xb + 16].view(np.uint32), ws[xb + 16:]
    assert (rest == WS_BYTE).all(), case.id                 # member_states_out was given: the scratch is not used
    if inst.kernel == "reg" or (inst.kernel == "plain" and not inst.gated):
        assert (head == WS_BYTE).all() and (ws[xb:xb + 16] == WS_BYTE).all(), (case.id, "a cooperative launch ran")
        return
    tags = (head.view(np.uint64) >> np.uint64(32)).astype(np.int64).reshape(E, 2, Wp)
    if inst.kernel == "plain":                              # the aborted cooperative launch in front of the gate
        assert status[0] != 0 and not status[1:].any(), (case.id, status)
        assert not tags.any(), case.id
        return
    assert not status.any(), (case.id, status)
    last = H * (L - 1) - 1                                  # the last phase; its epoch is last + 1
    want = {last & 1: last + 1, (last - 1) & 1: last}
    for parity in (0, 1):
        assert (tags[:, parity, :] == want[parity]).all(), (case.id, parity, want[parity], np.unique(tags[:, parity, :]))


def check_values(case, states, members):
    """The max abs error of the member states against float64, after the bars."""
    s64, _ = tc.reference(case.id)
    err = float(np.max(np.abs(members.astype(np.float64) - s64)))
    E = case.shape["E"]
    mean = tc.mean_f32(members) if E > 1 else members[0]
    mean_err = float(np.max(np.abs(states.astype(np.float64) - np.mean(s64, axis=0))))
    print(f"traj envelope {case.id}: {tuple(tc.instance(case))} member max abs err {err:.3g}, mean {mean_err:.3g} "
          f"(tight {tc.TIGHT:.3g}, hard {tc.HARD:g})")
    assert np.allclose(members, s64, rtol=tc.HARD, atol=tc.HARD), (case.id, err)
    assert np.allclose(states, np.mean(s64, axis=0), rtol=tc.HARD, atol=tc.HARD), (case.id, mean_err)
    assert states.tobytes() == mean.tobytes(), (case.id, "the member mean is not the sequential float32 mean")
    assert err <= tc.TIGHT and mean_err <= tc.TIGHT, (case.id, err, mean_err, tc.TIGHT)
    return err


def check_case(case, hop=0):
    inst = tc.instance(case, hop)
    states, members, ws = run(case, hop)
    check_workspace(case, inst, ws)
    return check_values(case, states, members), members


@pytest.mark.parametrize("case", tc.CASES, ids=[c.id for c in tc.CASES])
def test_every_instance_matches_float64_and_leaves_its_mark_in_the_workspace(case):
    assert tc.instance(case) == case.want
    check_case(case)


@pytest.mark.parametrize("case", tc.HOP_CASES, ids=[c.id for c in tc.HOP_CASES])
def test_hop_modes_are_bitwise_equal(case):
    """MBRL_OPT_TRAJ_HOP 1 (the (P, E) grid), 2 (the per-XCD grid) and 3 (the roll call) against 0: the same
    bits, each with the bars and the workspace marks of its own run."""
    _, base = check_case(case, 0)
    for hop in (1, 2, 3):
        assert tc.instance(case, hop).grid == ("pe" if hop == 1 or case.shape["E"] > 8 else "xcd")
        _, members = check_case(case, hop)
        assert members.tobytes() == base.tobytes(), (case.id, hop)


@pytest.mark.parametrize("cid,N,K", tc.PLANS, ids=[p[0] for p in tc.PLANS])
def test_plan_states_equal_a_standalone_trajectory_of_its_actions(cid, N, K):
    """CEMPlanner.plan_detailed (two iterations): its final states against mbrl_trajectory of the actions it
    returned, bit for bit -- the plan's hand-off block zeroed by its first launch against the memset path."""
    from mbrl_amd import CEMPlanner, fused
    case, p = tc.by_id(cid), tc.problem(cid)
    _, model_fn, cost_fn, sample_action = build(p)
    md = fused.describe_model(model_fn)
    assert md is not None and fused.describe_cost(cost_fn, md["s"], md) is not None, "fused path not taken"
    res = CEMPlanner.plan_detailed(torch.from_numpy(p["s0"]), model_fn, cost_fn, sample_action, case.H,
                                   num_candidates=N, num_elites=K, num_iterations=2, seed=p["rng_seed"], record=True)
    acts = np.ascontiguousarray(res["actions"].cpu().numpy())
    assert acts.shape == (case.H, case.shape["a"]) and np.abs(acts).max() <= 1.0 and np.abs(acts).max() > 0.0
    states, members, ws = run(case, 0, acts)
    check_workspace(case, tc.instance(case), ws)
    got = np.ascontiguousarray(res["states"].cpu().numpy())
    assert got.shape == states.shape and np.isfinite(got).all()
    assert got.tobytes() == states.tobytes(), (cid, float(np.max(np.abs(got - states))))


def measure_all(path):
    """Every case (every hop option of the hop cases) once more, its max abs error against float64 into `path`
    as JSON: what profiles/traj_envelope/errors.json holds."""
    out = {"device": torch.cuda.get_device_name(0), "D": tc.D, "tight_bar": tc.TIGHT, "hard_bar": tc.HARD, "cases": {}}
    for case in tc.CASES:
        for hop in case.hops:
            err, _ = check_case(case, hop)
            inst = tc.instance(case, hop)
            out["cases"][case.id if hop == 0 else f"{case.id}@hop{hop}"] = dict(
                instance=[inst.kernel] + [x if not isinstance(x, bool) else int(x) for x in inst[1:]], H=case.H,
                E=case.shape["E"], max_abs_err=err, over_tight_bar=err / tc.TIGHT)
    fam = {}
    for v in out["cases"].values():
        k = v["instance"][0]
        fam[k] = max(fam.get(k, 0.0), v["max_abs_err"])
    out["worst_per_family"] = fam
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    return out
