"""CPU: what the bars of tests/test_gpu_split_envelope.py are made of (tests/split_cases.py,
tests/split_reference.py). Conditions on the chosen shapes and seeds, asserted -- the GPU is not involved.

  * the worst ratio e(emulation, P) / max(e32, median e32) over the table, for P = 2 and P = 3, is what
    split_cases.WORST_RATIO records (up to another CPU's float32 matrix product), and K_P follows from it;
  * for P = 2 the emulation without x0 w1, and without x1 w0, misses every case's bar at least tenfold;
  * no ReLU input of a case lies on different sides of 0 in float32 and float64. (test_gd_grad_host.py asks
    for min |z| >= 100 x max |z32 - z64|, for the one action sequence of a gradient case. A case here has
    40 x W x L x H pre-activations -- up to 2.5e5 -- whose smallest is of the size of the float32 difference
    itself, so no seed can give that margin; what the bars need is asserted unit by unit instead: no sign
    differs, so the float32 oracle and the float64 reference follow the same linear pieces.)
  * the third-piece cases: float32 and the P = 3 emulation within 2 ulp of float64 on every state (they are
    exact), the P = 2 emulation and every third-order mutant a case is built to catch outside it, and every
    third-order product caught by some case."""
import numpy as np
import pytest

import split_cases as sc
import split_reference as sref

IDS = [c.id for c in sc.ACCEPTED]


def _ratio(cid, P):
    return sref.err(sc.emulated(cid, P), sc.reference(cid)[2]) / sc.base(cid)


def test_measured_ratios_give_the_recorded_bar_factors():
    for P in (2, 3):
        ratios = {cid: _ratio(cid, P) for cid in IDS}
        worst = max(ratios, key=ratios.get)
        print(f"P = {P}: worst e(emulation) / max(e32, median e32) = {ratios[worst]:.2f} ({worst}); "
              f"recorded {sc.WORST_RATIO[P]:.2f}, K_{P} = {sc.K_BAR[P]:g}")
        assert sc.K_BAR[P] == max(sc.FLOOR, sc.MARGIN * sc.WORST_RATIO[P])
        assert sc.MARGIN * ratios[worst] <= sc.K_BAR[P], (P, worst, ratios[worst])
        assert 0.5 * sc.WORST_RATIO[P] <= ratios[worst] <= 1.25 * sc.WORST_RATIO[P], (P, worst, ratios[worst])
    assert 5e-8 < sc.median_e32() < 5e-7
    for cid in IDS:                     # every bar is far inside the suite's state bar of 1e-4
        assert sc.bar(cid, 2) < 1e-5 and np.max(np.abs(sc.reference(cid)[2])) < 4.0


@pytest.mark.parametrize("cid", IDS)
def test_single_term_mutants_miss_the_bar_tenfold(cid):
    s64 = sc.reference(cid)[2]
    assert sref.err(sc.emulated(cid, 2), s64) <= sc.bar(cid, 2) / sc.MARGIN
    assert sref.err(sc.emulated(cid, 3), s64) <= sc.bar(cid, 3) / sc.MARGIN
    for drop in ((0, 1), (1, 0)):
        e = sref.err(sc.emulated(cid, 2, drop), s64)
        assert e >= sc.MUTANT_FACTOR * sc.bar(cid, 2), f"{sref.name(drop)} dropped: e = {e:.3e}, bar {sc.bar(cid, 2):.3e}"


@pytest.mark.parametrize("cid", IDS)
def test_no_relu_input_changes_sign_between_the_precisions(cid):
    s0, A = sc.inputs(cid)
    lo, d, flips = sref.relu_margin(sc.problem(cid), A, s0)
    assert flips == 0, f"{flips} units change side (min |z64| {lo:.2e}, max |z32 - z64| {d:.2e})"


def test_emulation_is_the_oracle_where_nothing_is_dropped():
    """The emulation differs from the float32 oracle only inside the Linears: its costs follow its states."""
    cid = "c11_t4"
    s0, A = sc.inputs(cid)
    costs, states = sref.emulate_split(sc.problem(cid), A, 3, None, s0)
    c32, s32, _ = sc.reference(cid)
    assert np.allclose(states, s32, rtol=0, atol=1e-6) and np.allclose(costs, c32, rtol=1e-6)
    assert sref.terms(2) == ((0, 0), (0, 1), (1, 0)) and len(sref.terms(3)) == 6


@pytest.mark.parametrize("name", sc.THIRD)
def test_third_piece_cases_tell_six_products_from_three(name):
    p, s0, A = sc.third_problem(name)
    _, s32, s64 = sc.third_reference(name)
    assert np.all(s64 != 0) and sref.ulps(s32, s64) <= sc.THIRD_ULPS
    full = sref.emulate_split(p, A, 3, None, s0)[1]
    assert sref.ulps(full, s64) <= sc.THIRD_ULPS
    two = sref.emulate_split(p, A, 2, None, s0)[1]
    assert sref.ulps(two, s64) > sc.MUTANT_FACTOR * sc.THIRD_ULPS
    assert sref.err(two, s64) <= sc.third_bar(name, 2)           # ... while F16X3 still meets its own bar
    for drop in ((0, 2), (1, 1), (2, 0)):
        got = sref.emulate_split(p, A, 3, [t for t in sref.terms(3) if t != drop], s0)[1]
        u = sref.ulps(got, s64)
        if drop in sc.THIRD_CATCHES[name]:
            assert u > sc.MUTANT_FACTOR * sc.THIRD_ULPS, (name, sref.name(drop), u)
        else:
            assert u == 0, (name, sref.name(drop), u)            # the product is zero in this case


def test_every_third_order_product_is_caught():
    assert set().union(*sc.THIRD_CATCHES.values()) == {(0, 2), (1, 1), (2, 0)}
    for name in sc.THIRD:                    # operands where a third piece is a normal float16
        p, s0, A = sc.third_problem(name)
        assert 8 <= np.min(np.abs(s0)) and np.max(np.abs(s0)) < 2048 and np.max(np.abs(A)) < 2048
