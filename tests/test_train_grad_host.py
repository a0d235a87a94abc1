"""CPU: the float64 reference of tests/test_gpu_train_grad.py (train_grad_reference), its case table and
the restatement of the training sources' dispatch (train_grad_cases). The hand-written backward pass is
autograd's; the table reaches every value of every dispatch dimension and both sides of every boundary,
named; no ReLU of any case can change side between float32 and float64 (the rejection sampling held, and
redrew at most a tenth of a case's transitions); and every case tells every applicable single mistake of
a tiled backward pass from a right one, by ten times its bar on the tile-relative metric. These are
conditions on the table, asserted -- not measurements."""
import os
import re

import numpy as np
import pytest
import torch

import train_grad_cases as tc
import train_grad_reference as ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mujoco-mbrl_amd", "csrc")


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("name", tc.NAMES)
def test_reference_is_autograd_of_the_documented_loss(name):
    """The layer-by-layer backward pass against torch autograd of one MSELoss per horizon step and head,
    both float64: equal to float64 rounding (they sum in different orders)."""
    p = tc.problem(name)
    loss, grads = ref.autograd64(p["params"], p["data"], p["rows"], tc.shape_of(name))
    got = tc.g64(name)
    assert abs(got["loss"][0] - loss) <= 1e-12 * abs(loss)
    assert abs(got["loss"][1] + got["loss"][2] - got["loss"][0]) <= 1e-15 * abs(loss)
    for label, x, y in zip(tc.tensor_names(name), got["grads"], grads):
        assert x.shape == y.shape and max(ref.err(x, y)) <= 1e-10, (label, ref.err(x, y))


def test_tile_metric_sees_what_the_tensor_metric_dilutes():
    """A fault confined to the partial tile of a [40][70] gradient whose entries there are small."""
    rng = np.random.default_rng(0)
    g = rng.standard_normal((40, 70))
    g[32:, 64:] *= 1e-3
    g[39, 69] = 5e-3            # the tile's largest entry
    x = g.copy()
    x[39, 69] *= 1.5
    whole, tile = ref.err(x, g)
    assert whole < 1e-3 and tile > 0.05
    # a tile that is exactly zero in the reference: skipped, unless x holds anything there
    g[:32, 32:64] = 0
    x = g.copy()
    assert ref.err(x, g) == (0.0, 0.0)
    x[3, 40] = 1e-30
    assert ref.err(x, g)[1] == float("inf")
    assert ref.err(np.zeros(5), np.zeros(5)) == (0.0, 0.0) and ref.err(np.ones(5), np.zeros(5))[0] == float("inf")
    assert ref.loss_err([1.0, 1.0, 0.0], [1.0, 1.0, 0.0]) == [0.0, 0.0, 0.0]
    assert ref.loss_err([1.0, 1.0, 1e-9], [1.0, 1.0, 0.0])[2] == float("inf")


# ------------------------------------------------------------------------------------------------ stability
@pytest.mark.parametrize("name", tc.NAMES)
def test_no_relu_can_change_side_between_the_precisions(name):
    p, c = tc.problem(name), tc.CASES[name]
    every = np.arange(p["T"])
    z64 = ref.preacts(p["params"], p["data"], every, tc.shape_of(name), torch.float64)
    z32 = ref.preacts(p["params"], p["data"], every, tc.shape_of(name), torch.float32)
    tau = tc.TAU_FACTOR * float(np.max(np.abs(z32 - z64)))
    assert tau == p["tau"] and 0 < tau < 1e-3
    assert float(np.min(np.abs(z64))) >= tau
    assert np.array_equal(np.sign(z32), np.sign(z64))
    assert p["redrawn"] <= tc.REDRAW_CAP * p["T"], (p["redrawn"], p["T"])
    # the batch's own pre-activations are rows of the same table
    assert float(np.min(np.abs(tc.g64(name)["pre"]))) >= tau
    assert np.array_equal(np.sign(tc.g32(name)["pre"]), np.sign(tc.g64(name)["pre"]))
    assert tc.g64(name)["pre"].shape == (c.L, c.B * c.H, c.W)


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("name", tc.NAMES)
def test_every_applicable_mutant_misses_the_bar_tenfold(name):
    misses = tc.mutant_misses(name)
    assert misses, "no mutant applies"
    for e, b in zip(tc.e32(name), tc.bars(name)):
        assert 0 <= e[0] < 1e-3 and 0 <= e[1] < 1e-3 and 0 < b[0] < 1e-2 and 0 < b[1] < 1e-2
    for e, b, l in zip(tc.e32_loss(name), tc.loss_bars(name), tc.g64(name)["loss"]):
        assert e < 1e-5 and 0 < b < 1e-4 and (l > 0 or e == 0)
    for label, miss in misses.items():
        assert miss >= tc.MUTANT_FACTOR, f"{label}: misses its bar by {miss:.3g} x < {tc.MUTANT_FACTOR:g} x"


def test_every_mutant_is_caught_by_some_case():
    caught = {label: [n for n in tc.NAMES if label in ref.applicable(tc.shape_of(n), tc.CASES[n].B)]
              for label in ref.MUTANTS}
    for label, names in caught.items():
        assert names, label
    assert set(caught["dW_0 columns >= 64 dropped"]) == {n for n in tc.NAMES if tc.CASES[n].s + tc.CASES[n].a > 64}
    assert len(caught["dW_0 columns >= 64 dropped"]) >= 5
    assert caught["dW_0 column K0-1 dropped"] == tc.NAMES
    p = tc.problem("l3")
    base = tc.g64("l3")
    for label in ref.applicable(tc.shape_of("l3"), tc.CASES["l3"].B):   # the forward of a mutant is the reference's
        m = ref.loss_and_grads(p["params"], p["data"], p["rows"], tc.shape_of("l3"), torch.float64, mutant=label)
        assert np.array_equal(m["loss"], base["loss"]) and np.array_equal(m["pre"], base["pre"]), label
        assert any(not np.array_equal(x, y) for x, y in zip(m["grads"], base["grads"])), label


# ------------------------------------------------------------------------------------------------ coverage
def _keys(cus=tc.MI355X_CUS):
    return {n: tc.dispatch(n, cus) for n in tc.NAMES}


def _launches(keys, prefix):
    return [l for k in keys.values() for l in k.launches if l.name.startswith(prefix)]


def test_table_reaches_every_value_of_every_dispatch_dimension():
    keys = _keys()
    assert {k.fold_nw for k in keys.values()} == {0, 4, 8, 16}
    # the fold with its input rows staged in LDS and read from memory, at every wave count
    assert {(k.fold_nw, k.fold_input) for k in keys.values()} == \
        {(0, None)} | {(nw, src) for nw in (4, 8, 16) for src in ("lds", "global")}
    fused = [k.fused for k in keys.values() if k.fused]
    assert {(f.layout, f.nw, f.kch) for f in fused} == {("fo", nw, kch) for nw in (4, 16) for kch in (2, 4)}
    for flag in ("vec0", "vec1", "veca", "vecb"):
        assert {getattr(f, flag) for f in fused} == {True, False}, flag
    # the two-launch F / O under MBRL_OPT_TRAIN_FO, the same four instantiations
    split = [tc.dispatch(n, opts={"train_fo": 1}).fused for n in tc.NAMES if keys[n].fused]
    assert {(f.layout, f.nw, f.kch) for f in split} == {("split", nw, kch) for nw in (4, 16) for kch in (2, 4)}
    # launch_waves: the layer-0 forward has K = s + a < 256 in every case (4 waves); the others 4 / 16; the
    # backward launches 4 / 8 / 16, the output layer's and a hidden layer's alike, and dW_0's own launch
    assert {l.nw for l in _launches(keys, "fwd0")} == {4}
    assert {l.nw for l in _launches(keys, "fwd") if l.name != "fwd0"} == {4, 16}
    assert {l.nw for l in _launches(keys, "out")} == {4, 16}
    out_bwd = [k.launches[-1 - (tc.CASES[n].L - (1 if k.fold_nw else 0))] for n, k in keys.items() if not k.fused]
    assert all(l.name.startswith("bwd") for l in out_bwd) and {l.nw for l in out_bwd} == {4, 8, 16}
    assert {l.nw for l in _launches(keys, "bwd1")} == {4, 8, 16}
    assert {l.nw for l in _launches(keys, "bwd0")} == {4, 16}     # (8 needs R in (128, 256): the fold takes those)
    assert {l.nw for l in _launches({n: tc.dispatch(n, opts={"train_no_fold": 1}) for n in tc.NAMES}, "bwd0")} == {4, 8, 16}
    # the tile height: both outcomes of the tmx rule on the device's 256 CUs, for the output layer's launch
    # and a hidden layer's, fused and not; and on a small device
    assert {l.tmx for l in out_bwd} == {1, 2}
    assert {k.launches[-1].tmx for k in keys.values() if k.fused} == {1, 2}
    assert {l.tmx for n, k in keys.items() if not k.fused for l in k.launches if l.name == "bwd1"} == {1, 2}
    small = _keys(tc.SMALL_CUS)
    assert {l.tmx for l in _launches(small, "bwd")} == {1, 2}
    assert sum(small[n] != keys[n] for n in tc.NAMES) >= 5
    assert all(l.tmx == 1 for l in _launches(small, "bwd0") + _launches(small, "fwd") + _launches(small, "out"))
    # every OP_DIRECT operand with float4 loads and without
    assert {l.vec_b for l in _launches(keys, "fwd0")} == {True, False}
    for prefix in ("fwd1", "fwd2", "out", "bwd1", "bwd2"):
        assert {l.vec_a for l in _launches(keys, prefix)} == {True, False}, prefix
    for prefix in ("fwd1", "fwd2", "out"):
        assert {l.vec_b for l in _launches(keys, prefix)} == {True, False}, prefix
    # ... cleared by the pointer alone (W % 4 == 0 and K0 % 4 == 0), in all Linears and in the reward head only
    for n in tc.NAMES:
        c = tc.CASES[n]
        if c.align != "aligned":
            assert c.W % 4 == 0 and (c.s + c.a) % 4 == 0 and c.reward, n
            aligned = tc.train_dispatch(c.s, c.a, c.W, c.L, c.reward, c.H, c.B, tc.MI355X_CUS)
            assert aligned != keys[n], n
            flags = lambda k: [l.vec_b for l in k.launches if l.vec_b is not None] + \
                ([k.fused.vec0, k.fused.vec1, k.fused.vecb] if k.fused else [])  # noqa: E731  (the weights' flags)
            assert all(flags(aligned)) and not all(flags(keys[n])), n
    mixed = keys["offset_reward_w"]
    assert [l.name for l in mixed.launches if l.vec_b is False] == ["out"]
    assert {tc.CASES[n].align for n in tc.NAMES} == {"aligned", "offset", "reward_w"}
    assert any(keys[n].fused for n in tc.NAMES if tc.CASES[n].align == "offset")
    assert any(not keys[n].fused for n in tc.NAMES if tc.CASES[n].align == "offset")
    # every forced layout changes some case's key (the GPU test runs exactly those pairs), XCD order included
    for opt in tc.LAYOUTS:
        assert sum(opt in tc.layouts_for(n) for n in tc.NAMES) >= 2, opt
    assert any(l.xcd for n in tc.NAMES for l in tc.dispatch(n, opts={"train_xcd": 1}).launches)
    assert not any(l.xcd for k in keys.values() for l in k.launches)


def test_ensemble_dispatch_and_its_vec_downgrade():
    for n in tc.ENSEMBLE_CASES:
        c = tc.CASES[n]
        k = tc.dispatch(n, ensemble=True)
        assert k.fold_nw == 0 and k.fused is None and len(k.launches) == 2 * c.L + 2, n
    ens = {n: tc.CASES[n] for n in tc.ENSEMBLE_CASES}
    assert any(c.s + c.a > 64 for c in ens.values()) and any(c.L == 8 for c in ens.values())
    assert any(c.s + c.reward == 33 for c in ens.values()) and any(c.a == 0 for c in ens.values())
    assert {c.align for c in ens.values()} >= {"offset", "reward_w"}
    # member 0 aligned, its partner not: direct() says vec, :1793 takes it back
    for n in ("offset_l3", "offset_reward_w"):
        c = tc.CASES[n]
        args = (c.s, c.a, c.W, c.L, c.reward, c.H, c.B, tc.MI355X_CUS)
        alone = tc.train_dispatch(*args, ensemble=True)
        mixed = tc.train_dispatch(*args, ensemble=True, misaligned_any=tc.misaligned(n))
        assert all(l.vec_b for l in alone.launches if l.vec_b is not None)
        assert mixed != alone and mixed == tc.train_dispatch(*args, ensemble=True, misaligned=tc.misaligned(n))


# (boundary, the case on its accepted side, the case past it, what must differ: key -> value)
BOUNDARIES = [
    ("FUSED_WMAX: W = 512 / 520", "w512_fused", "w520", lambda k: k.fused is not None),
    ("W = 512 / 520 with R = 512: fused at 16 bands", "r512_fused", "w520", lambda k: k.fused is not None),
    ("fused waves: W = 255 / 256", "w255_fused", "w256_k33_fused", lambda k: k.fused.nw == 4),
    ("KCH: K0 = 32 / 33", "k32_fused", "w256_k33_fused", lambda k: k.fused.kch == 2),
    ("FUSED_K0MAX: K0 = 64 / 65", "k64_fused", "k65_l2", lambda k: k.fused is not None),
    ("FOLD_K0MAX: K0 = 64 / 65", "k64_fused", "k65_l2", lambda k: k.fold_input == "lds"),
    ("J = 32 / 33 with the reward column", "j32_reward_fused", "j33", lambda k: k.fused is not None),
    ("R = 64 / 65: no fold / 4 waves", "r65", "r64", lambda k: k.fold_nw == 4),
    ("R = 128 / 129: 4 / 8 waves", "r128", "r129", lambda k: k.fold_nw == 4),
    ("R = 255 / 256: 8 waves / no fold", "r255", "r256", lambda k: k.fold_nw == 8),
    ("R = 257 / 256: 16 waves / no fold", "r257", "r256", lambda k: k.fold_nw == 16),
    ("R = 512 / 513: 16 waves / no fold", "r512", "r513", lambda k: k.fold_nw == 16),
    ("R = 512 / 513: fused / not", "r512_fused", "r513", lambda k: k.fused is not None),
]
SIDES = {"w512_fused": ("W", 512), "w520": ("W", 520), "w255_fused": ("W", 255), "w256_k33_fused": ("W", 256),
         "k32_fused": ("K0", 32), "k64_fused": ("K0", 64), "k65_l2": ("K0", 65), "j32_reward_fused": ("J", 32),
         "j33": ("J", 33), "r64": ("R", 64), "r65": ("R", 65), "r128": ("R", 128), "r129": ("R", 129),
         "r255": ("R", 255), "r256": ("R", 256), "r257": ("R", 257), "r512": ("R", 512), "r513": ("R", 513),
         "r512_fused": ("R", 512)}


@pytest.mark.parametrize("what,inside,outside,holds", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_both_sides_of_every_boundary(what, inside, outside, holds):
    keys = _keys()
    assert holds(keys[inside]) and not holds(keys[outside]), what
    for n, (dim, value) in SIDES.items():
        c = tc.CASES[n]
        assert {"W": c.W, "K0": c.s + c.a, "J": c.s + c.reward, "R": c.B * c.H}[dim] == value, n
    assert tc.CASES["w256_k33_fused"].s + tc.CASES["w256_k33_fused"].a == 33


def test_table_covers_what_the_issue_names():
    C = tc.CASES.values()
    assert 35 <= len(tc.CASES) <= 45
    assert {c.L for c in C} >= {1, 2, 3, 5, 8}
    assert sum(c.a == 0 for c in C) >= 2 and any(c.a == 0 and tc.dispatch(n).fused for n, c in tc.CASES.items())
    assert {(c.s, c.reward) for c in C} >= {(1, 0), (31, 1), (32, 0), (32, 1), (64, 1)}
    assert {c.W for c in C} >= {1, 33, 255, 256, 512, 520, 1024}
    assert all((c.L, c.B * c.H) == (1, 64) for c in C if c.W == 1024)
    foldk = {(c.s + c.a, c.B * c.H) for n, c in tc.CASES.items() if c.L == 3 and tc.dispatch(n).fold_input == "global"}
    assert {k for k, _ in foldk} == {65, 88} and {r for _, r in foldk} == {100, 200, 300}
    assert {c.H for c in C} == {1, 2, 3}
    for H in (2, 3):
        assert {c.B * c.H for c in C if c.H == H} & {64, 128, 129, 255, 256, 512}, H
    assert sum(c.B == 1 for c in C) >= 2 and any(c.B == 1 and c.H == 3 for c in C)
    rep = [n for n, c in tc.CASES.items() if c.rows == "repeat"]
    assert len(rep) >= 4
    for n in rep:
        p = tc.problem(n)
        assert p["T"] - 1 in p["rows"] and len(set(p["rows"].tolist())) < len(p["rows"])
    for n in tc.NAMES:
        p, c = tc.problem(n), tc.CASES[n]
        assert len(p["rows"]) == c.B <= p["T"] and p["rows"].min() >= 0 and p["rows"].max() < p["T"]
        other = tc.other_rows(n)
        assert len(other) == c.B and other.max() < p["T"] and (c.B == 1 or not np.array_equal(other, p["rows"]))
        assert c.L + 1 + c.reward <= 10                  # MBRL_TRAIN_MAX_LAYERS
    assert any(c.L == 8 and c.reward for c in C)         # all ten Linears of the ABI


def test_model_constants_are_the_sources():
    """A change of a threshold in launch_train_grads fails here, and sends its author to train_dispatch."""
    src = ""
    for name in ("mbrl_train.h", "train.hip", "train_fused.hip", "train_api.hip"):   # the training sources, together
        with open(os.path.join(CSRC, name)) as f:
            src += f.read()

    def one(pattern):
        assert len(re.findall(pattern, src)) == 1, pattern

    one(r"constexpr int TT = 32;")
    one(r"constexpr int FOLD_K0MAX = 64;")
    one(r"constexpr int FUSED_WMAX = 512;")
    one(r"constexpr int FUSED_K0MAX = 64;")
    one(r"constexpr int FUSED_MAX_BANDS = 16;")
    one(r"const int nw = R >= 256 \? 16 : R > 128 \? 8 : 4, chunks = \(R \+ 15\) / 16, per = \(chunks \+ nw - 1\) / nw;\n"
        r"    return per == 2 \? nw : 0;")
    one(r"return t\.split == 0 && t\.L == 2 && fold_nw > 0 && J <= TT && K0 <= FUSED_K0MAX && t\.W <= FUSED_WMAX;")
    one(r"return kmax >= 256 \? 16 : \(kmax > 128 && grad_rows\) \? 8 : 4;")
    one(r"int tmx = \(l >= 1 && tiles32 > device_cu_count\(\) && \(n_out >= 256 \|\| R >= 256\)\) \? 2 : 1;")
    one(r"if \(t\.tile == 32 \|\| \(t\.tile == 64 && l >= 1 && \(n_out >= 256 \|\| R >= 256\)\)\) tmx = t\.tile / 32;")
    one(r"L\.xcd = L\.xcd && \(tiles_m0 % \(8 \* \(2 / TMX\)\) == 0\);")
    one(r"o\.vec = \(ld % 4 == 0\) && \(\(reinterpret_cast<uintptr_t>\(p0\) \| reinterpret_cast<uintptr_t>\(o\.p1\)\) & 15\) == 0;")
    one(r"if \(KIND == 0 && !vec\) G\.d\[0\]\.B\.vec = 0;")
    one(r"const bool xstage = !PLAIN && O\.mode == EPI_MASK && O\.fold && O\.fold_k0 <= FOLD_K0MAX;")
    one(r"K0 <= FOLD_K0MAX \? xs\[r - m0\]\[kk\] : O\.fold_x\[\(int64_t\)r \* K0 \+ kk\]")
    one(r"const int l_end = fold_nw \? 1 : 0;")
    one(r"const int kch = F\.K0 <= 32 \? 2 : 4;")
    one(r"const int nw = F\.W >= 256 \? 16 : 4;")
    one(r"K0 <= 32 \?")     # no second selection on either threshold
    one(r"W >= 256 \?")
