"""CPU checks of the open-loop training tests' own yardsticks: the written-out backward pass against float64
autograd, the forward chain against tests/open_loop_reference.py, horizon 1 against the one-step gradient, the
case table's coverage and the single-mistake mutants."""
import numpy as np
import pytest
import torch

import open_loop_reference as olref
import train_grad_reference as tref
import train_open_loop_cases as tc
import train_open_loop_reference as ref

QUICK = ["h1_b17", "h3_b15", "s17_a0", "s5_a12", "l3", "a0_plain", "repeats"]


@pytest.mark.parametrize("name", QUICK)
def test_written_out_backward_is_float64_autograd(name):
    p = tc.problem(name)
    loss, grads, pred = ref.autograd64(p["members"][0], p["data"], p["rows"][0], tc.shape_of(name))
    mine = tc.g64(name)
    assert np.allclose(mine["loss"], loss, rtol=1e-12, atol=0)
    assert np.allclose(mine["pred"], pred, rtol=1e-12, atol=1e-14)
    for x, y in zip(mine["grads"], grads):
        assert np.max(np.abs(x - y)) <= 1e-12 * max(np.max(np.abs(y)), 1e-300)


@pytest.mark.parametrize("name", QUICK)
def test_forward_chain_is_the_open_loop_evaluation(name):
    p = tc.problem(name)
    want = olref.evaluate(p["members"][0], p["data"], p["rows"][0], tc.shape_of(name), torch.float64)
    mine = tc.g64(name)
    assert np.allclose(mine["row_err"], np.asarray(want["row_err"], np.float64), rtol=1e-12, atol=1e-300)
    assert np.allclose(mine["pred"], np.asarray(want["pred"], np.float64), rtol=1e-12, atol=1e-14)


def test_horizon_one_is_the_one_step_gradient():
    name = "h1_b17"
    p = tc.problem(name)
    _, grads = tref.autograd64(p["members"][0], p["data"], p["rows"][0], tc.shape_of(name))
    for x, y in zip(tc.g64(name)["grads"], grads):
        assert np.max(np.abs(x - y)) <= 1e-12 * np.max(np.abs(y))


def test_table_reaches_every_listed_value():
    cs = list(tc.CASES.values())
    assert {1, 2, 3, 7, 30} <= {c.H for c in cs}
    assert any(c.H == 30 and c.W <= 64 for c in cs)
    assert {1, 15, 16, 17, 33, 257} <= {c.B for c in cs}
    assert {(15, 2), (16, 1), (17, 0), (5, 12), (33, 48)} <= {(c.s, c.a) for c in cs}
    assert any(c.s > c.W for c in cs) and any(c.s == 1 for c in cs)
    assert {(r, a) for r in (0, 1) for a in (0, 1, 6)} <= {(c.reward, c.a) for c in cs}
    assert {1, 2, 3, 8} <= {c.L for c in cs}
    assert {1, 33, 64, 255, 256, 520, 1024} <= {c.W for c in cs}
    assert {1, 2, 5, 8} <= {c.E for c in cs}
    assert any(c.rows == "repeat" for c in cs) and any(c.offset and c.E >= 2 for c in cs)
    assert 20 <= len(cs) <= 32


@pytest.mark.parametrize("name", tc.NAMES)
def test_no_relu_changes_side_between_float32_and_float64(name):
    p, c = tc.problem(name), tc.CASES[name]
    for e in range(c.E):
        z64, z32 = tc.g64(name, e)["pre"], tc.g32(name, e)["pre"]
        assert np.array_equal(z64 > 0, z32 > 0)
        assert float(np.min(np.abs(z64))) >= p["tau"] / 1.0000001 or float(np.min(np.abs(z64))) >= \
            tc.TAU_FACTOR * float(np.max(np.abs(z32 - z64)))


@pytest.mark.parametrize("name", [n for n in tc.NAMES if tc.CASES[n].H >= 2])
def test_every_mutant_misses_the_bars_tenfold(name):
    c = tc.CASES[name]
    misses = tc.mutant_misses(name)
    assert set(misses) == set(ref.applicable(tc.shape_of(name), c.B)) and "detached feedback" in misses
    for label, ratio in misses.items():
        assert ratio >= tc.MUTANT_FACTOR, (name, label, ratio)


def test_at_least_six_mutants_apply_somewhere():
    seen = set()
    for n in tc.NAMES:
        c = tc.CASES[n]
        seen |= set(ref.applicable(tc.shape_of(n), c.B))
    assert len(seen) >= 6 and seen == set(ref.MUTANTS)
    assert tc.MUTANT_FACTOR >= 10
