"""The cases of tests/test_gpu_train_grad.py (mbrl_train_grads and its ensemble / epoch siblings against
the float64 gradient of tests/train_grad_reference.py) as plain data plus CPU helpers, and a restatement
of launch_train_grads' dispatch (train_dispatch) so that tests/test_train_grad_host.py can show on the
CPU that every reachable branch has a case. No GPU import.

Largest e(gpu) / max(e32, median e32) per tensor kind over the table -- how much of BAR_FACTOR = 8 is
used -- in the default dispatch on an MI355X, tensor-relative / tile-relative, and in brackets the largest
plain e(gpu) / e32 (large only where the float32 restatement happened to land almost on float64):
    dW_0       0.69 / 0.99   (1.52 / 1.52)        db_0       1.93 / 1.53   (7.72 / 7.72, s1)
    dW_hidden  1.34 / 1.34   (1.47 / 1.43)        db_hidden  2.06 / 2.03   (3.70 / 3.47)
    dW_out     1.03 / 0.99   (2.10 / 2.10)        db_out     1.34 / 1.07   (3.42 / 3.42)
    dW_rew     2.03 / 1.85   (2.03 / 1.85)        db_rew     4.04 / 3.22   (114 / 114, j32_reward_fused)
    losses     3.26          (1587, l8_fold's total, whose e32 is 4e-11)
Every forced layout, ensemble and epoch run is byte-equal to the default one, so these are their figures too.
"""
import collections
import functools

import numpy as np
import torch

import train_grad_reference as ref
from gd_grad_cases import BAR_FACTOR, MUTANT_FACTOR

TAU_FACTOR = 32.0       # tau = TAU_FACTOR x max |z32 - z64| of the case: no |z64| of the data set lies below it
REDRAW_CAP = 0.10       # at most this share of a case's transitions was redrawn

# ------------------------------------------------------------------------------------------------
# Part one: the training sources' dispatch, restated (csrc/train.hip unless a comment names mbrl_train.h,
# train_fused.hip or train_api.hip; functions are cited by name).
TT = 32                 # mbrl_train.h  C tile edge
FOLD_K0MAX = 64         # train.hip  the dW_0 fold stages its input rows in LDS up to this K0
FUSED_WMAX = 512        # mbrl_train.h
FUSED_K0MAX = 64        # mbrl_train.h
FUSED_MAX_BANDS = 16    # mbrl_train.h
OPTIONS = ("train_no_fold", "train_split", "train_fo", "train_xcd", "train_tile")

# One GEMM launch: which layer's, the waves per workgroup (launch_waves), the C tile height in 32-row units
# (tmx; 1 for the forward launches), whether the XCD order survives launch_gemm's bijection test, and the
# vec flag of each OP_DIRECT operand (A, B; None where the operand is not OP_DIRECT).
Launch = collections.namedtuple("Launch", "name nw tmx xcd vec_a vec_b")
# The fused step's F / O: one launch ("fo") or two ("split"), their waves, the layer-0 chunks per wave, and
# the four load-path flags (w0, w1, act1, w_out).
Fused = collections.namedtuple("Fused", "layout nw kch vec0 vec1 veca vecb")
Key = collections.namedtuple("Key", "fold_nw fold_input fused launches")


def _ceil(x, y):
    return -(-x // y)


def fold_waves(R, L, fold):
    """fold_waves. The waves of the separate dW_0 launch when the fold reproduces it, else 0."""
    if not fold or L < 1:
        return 0
    nw = 16 if R >= 256 else 8 if R > 128 else 4
    per = _ceil(_ceil(R, 16), nw)
    return nw if per == 2 else 0


def fused_step(s, a, W, L, reward, R, fold_nw, split):
    """fused_step (both overloads)."""
    J, K0 = s + (1 if reward else 0), s + a
    return (not split and L == 2 and fold_nw > 0 and J <= TT and K0 <= FUSED_K0MAX and W <= FUSED_WMAX
            and _ceil(R, TT) <= FUSED_MAX_BANDS)


def launch_waves(products):
    """launch_waves. products: [(K, is_weight_gradient)]."""
    kmax = max(k for k, _ in products)
    grad_rows = any(g and k == kmax for k, g in products)
    return 16 if kmax >= 256 else 8 if (kmax > 128 and grad_rows) else 4


def train_dispatch(s, a, W, L, reward, H, B, cu_count, opts=None, misaligned=(), ensemble=False, misaligned_any=None):
    """The dispatch key of one mbrl_train_grads call (ensemble: of mbrl_train_grads_ensemble's launches).
    opts: {option name: value} of OPTIONS; misaligned: the Linears (0 .. L, L + 1 = the reward head) whose
    weight is not 16-byte aligned -- for an ensemble member 0's, which direct() sees, with misaligned_any
    those of any member (launch_gemm_any; default: member 0's)."""
    opts = dict(opts or {})
    assert set(opts) <= set(OPTIONS), opts
    R, K0, J = B * H, s + a, s + (1 if reward else 0)
    tiles_r, tiles_w = _ceil(R, TT), _ceil(W, TT)
    tile = opts.get("train_tile", 0)
    fold = not opts.get("train_no_fold", 0)                   # train_shape (train_api.hip)
    split = opts.get("train_split", 0) == 1                   # train_shape
    xcd_opt = opts.get("train_xcd", 0) == 1                   # train_shape
    fo = opts.get("train_fo", 0) != 1                         # train_shape; launch_train_grads
    if ensemble:                                              # ensemble_shape (train_api.hip)
        fold, split, xcd_opt = False, True, False
    bad0 = set(misaligned)                                    # what direct() sees
    bad = bad0 | set(misaligned_any or ())
    wvec = lambda ld, seen, *layers: ld % 4 == 0 and not (set(layers) & seen)   # noqa: E731  direct()
    out_layers = (L, L + 1) if reward else (L,)
    fold_nw = fold_waves(R, L, fold)
    fused = fused_step(s, a, W, L, reward, R, fold_nw, split)
    fused_key = None
    launches = []

    def add(name, nw, tmx, m0, vec_a, vec_b, kind0=False):
        # launch_gemm: the XCD order needs whole groups of 8 64-row bands of product 0; launch_gemm_any: never in an ensemble
        xcd = xcd_opt and _ceil(m0, TT * tmx) % (8 * (2 // tmx)) == 0
        if kind0 and ensemble:                    # launch_gemm_any: one load path for all members
            vec_b = vec_b and not (set(kind0) & bad)
        launches.append(Launch(name, nw, tmx, xcd, vec_a, vec_b))

    if fused:
        # launch_train_fused (train_fused.hip): the wave count of the separate launches whose K is W; K0's chunks
        fused_key = Fused("fo" if fo else "split", 16 if W >= 256 else 4, 2 if K0 <= 32 else 4,
                          wvec(K0, bad0, 0),              # fused_fwd vec0
                          wvec(W, bad0, 1),               # fused_fwd vec1
                          W % 4 == 0,                     # fused_out veca (act1 lies in the workspace: aligned)
                          wvec(W, bad0, *out_layers))     # fused_out vecb
    else:
        for l in range(L):                                    # launch_train_grads: the forward loop
            K = K0 if l == 0 else W
            add(f"fwd{l}", launch_waves([(K, False)]), 1, R, None if l == 0 else W % 4 == 0, wvec(K, bad0, l), kind0=(l,))
        add("out", launch_waves([(W, False)]), 1, R, W % 4 == 0, wvec(W, bad0, *out_layers), kind0=out_layers)   # launch_train_grads: the output layer
    l_end = 1 if fold_nw else 0                               # launch_train_grads
    for l in range(L - 1 if fused else L, l_end - 1, -1):     # launch_train_grads: the backward loop
        n_out, n_in = (J if l == L else W), (K0 if l == 0 else W)
        tiles32 = (tiles_r * tiles_w if l >= 1 else 0) + _ceil(n_out, TT) * _ceil(n_in, TT)          # launch_train_grads
        big = l >= 1 and (n_out >= 256 or R >= 256)
        tmx = 2 if (big and tiles32 > cu_count) else 1        # launch_train_grads
        if tile == 32 or (tile == 64 and big):                # launch_train_grads
            tmx = tile // 32
        products = ([(n_out, False)] if l >= 1 else []) + [(R, True)]
        nw = launch_waves(products)
        assert tmx == 1 or nw == 16                           # launch_at_waves
        add(f"bwd{l}", nw, tmx, R if l >= 1 else n_out, (n_out % 4 == 0) if l >= 1 else None, None)   # launch_train_grads
    fold_input = None if not fold_nw else "lds" if K0 <= FOLD_K0MAX else "global"      # gemm_tile xstage, fold_dw0
    return Key(fold_nw, fold_input, fused_key, tuple(launches))


# ------------------------------------------------------------------------------------------------
# Part two: the case table. rows: "seq" (0 .. B - 1), "perm" (a permutation's first B of T = B + 5),
# "repeat" (drawn with replacement, one index three times, T - 1 among them). align: "aligned",
# "offset" (every parameter and gradient tensor a view 4 bytes into a larger buffer), "reward_w" (only
# the reward head's weight).
Case = collections.namedtuple("Case", "kind s a W L reward H B rows align")


def _c(kind, s, a, W, L, reward, H, B, rows="perm", align="aligned"):
    return Case(kind, s, a, W, L, reward, H, B, rows, align)


CASES = {
    # ---- depth: L in {1, 2, 3, 5, 8}; dh[l % 2] and act[0..7] past depth 4
    "l1_w33": _c("depth", 5, 2, 33, 1, 0, 1, 7),
    "l1_w1024": _c("depth", 6, 2, 1024, 1, 0, 1, 64),
    "l3": _c("depth", 7, 3, 48, 3, 1, 1, 40, rows="repeat"),
    "l5_fold": _c("depth", 6, 2, 40, 5, 0, 1, 70),
    "l8_fold": _c("depth", 5, 2, 36, 8, 1, 1, 100),
    "l8_h2": _c("depth", 5, 3, 33, 8, 0, 2, 20),
    # ---- action_dim = 0 (actions == NULL)
    "a0_fused": _c("a0", 6, 0, 64, 2, 0, 1, 96),
    "a0_l3": _c("a0", 5, 0, 32, 3, 1, 2, 25, rows="repeat"),
    # ---- smallest sizes
    "s1": _c("small", 1, 1, 16, 2, 0, 1, 33),
    "w1": _c("small", 3, 1, 1, 1, 0, 1, 20),
    "b1": _c("small", 5, 2, 20, 2, 1, 1, 1, rows="seq"),
    "b1_h3": _c("small", 4, 1, 24, 3, 0, 3, 1, rows="seq"),
    # ---- the output tile seam: J = 32 with and without the reward column, J = 33, J = 65
    "j32_reward_fused": _c("seam", 31, 3, 64, 2, 1, 1, 96),
    "j32_fused": _c("seam", 32, 2, 64, 2, 0, 1, 70),
    "j33": _c("seam", 32, 1, 64, 2, 1, 1, 96),
    "j65": _c("seam", 64, 4, 40, 2, 1, 1, 50),
    # ---- W: 255 / 256 (fused 4 / 16 waves), 512 / 520 (FUSED_WMAX); K0: 32 / 33 (KCH), 64 / 65
    "w255_fused": _c("width", 9, 3, 255, 2, 1, 1, 100),
    "w256_k33_fused": _c("width", 30, 3, 256, 2, 0, 1, 130),
    "k32_fused": _c("width", 28, 4, 100, 2, 0, 1, 200, rows="repeat"),
    "w512_fused": _c("width", 17, 6, 512, 2, 1, 1, 257),
    "w520": _c("width", 8, 2, 520, 2, 0, 1, 65),
    "k64_fused": _c("width", 32, 32, 96, 2, 0, 1, 65),
    "k65_l2": _c("width", 32, 33, 96, 2, 0, 1, 65),
    # ---- the fold with K0 > 64 (global input reads), L = 3
    "fold_k65_r100": _c("foldk", 50, 15, 64, 3, 0, 1, 100),
    "fold_k88_r200": _c("foldk", 64, 24, 48, 3, 1, 2, 100),
    "fold_k65_r300": _c("foldk", 45, 20, 40, 3, 1, 3, 100, rows="repeat"),
    "fold_k88_r300": _c("foldk", 60, 28, 40, 3, 0, 1, 300),
    # ---- R = B H on each side of every row boundary
    "r64": _c("rows", 4, 2, 40, 2, 0, 2, 32),
    "r65": _c("rows", 4, 2, 40, 2, 0, 1, 65),
    "r128": _c("rows", 4, 2, 40, 3, 1, 2, 64),
    "r129": _c("rows", 4, 2, 40, 3, 1, 3, 43),
    "r255": _c("rows", 6, 1, 48, 2, 1, 3, 85),
    "r256": _c("rows", 6, 1, 48, 2, 1, 2, 128),
    "r257": _c("rows", 6, 1, 48, 3, 0, 1, 257),
    "r512": _c("rows", 5, 2, 64, 3, 0, 2, 256),
    "r512_fused": _c("rows", 5, 2, 512, 2, 1, 2, 256),
    "r513": _c("rows", 5, 2, 480, 2, 1, 1, 513),
    # ---- operands at 4-byte offsets (W % 4 == 0 and K0 % 4 == 0: the pointer alone clears vec)
    "offset_fused": _c("align", 6, 2, 64, 2, 1, 1, 96, align="offset"),
    "offset_l3": _c("align", 6, 2, 64, 3, 1, 1, 40, align="offset"),
    "offset_reward_w": _c("align", 6, 2, 64, 3, 1, 1, 40, align="reward_w"),
}
NAMES = list(CASES)
LAYOUTS = (("train_no_fold", 1), ("train_split", 1), ("train_fo", 1), ("train_xcd", 1), ("train_tile", 32), ("train_tile", 64))
ENSEMBLE_CASES = ("fold_k65_r100", "fold_k88_r200", "l8_fold", "j33", "a0_fused", "a0_l3", "offset_l3", "offset_reward_w")
MI355X_CUS = 256
SMALL_CUS = 8           # the CPU test's second CU count: tmx = 2 at small shapes too


def shape_of(name):
    c = CASES[name]
    return (c.s, c.a, c.W, c.L, c.reward, c.H)


def misaligned(name):
    """The Linears whose weight pointer is not 16-byte aligned under the case's alignment policy."""
    c = CASES[name]
    return {"aligned": (), "offset": tuple(range(c.L + 1 + c.reward)), "reward_w": (c.L + 1,)}[c.align]


def dispatch(name, cu_count=MI355X_CUS, opts=None, **kw):
    c = CASES[name]
    return train_dispatch(c.s, c.a, c.W, c.L, c.reward, c.H, c.B, cu_count, opts, misaligned(name), **kw)


def layouts_for(name, cu_count=MI355X_CUS):
    """The forced layouts that change the case's dispatch key."""
    base = dispatch(name, cu_count)
    return [(o, v) for o, v in LAYOUTS if dispatch(name, cu_count, {o: v}) != base]


def _draw(g, n, s, a, H):
    return dict(states=torch.randn((n, H, s), generator=g).numpy(),
                actions=torch.rand((n, H, a), generator=g).mul(2).sub(1).numpy(),
                next_states=torch.randn((n, H, s), generator=g).numpy(),
                rewards=torch.randn((n, H), generator=g).numpy())


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(params, data, rows, T, tau, redrawn) of a case (shared: do not write to it). The parameters are
    torch's default Linear initialisation; the transitions are drawn as tests/test_gpu_train_ensemble.py's
    _Data draws them, and every transition with a float64 pre-activation (any layer, any horizon step)
    within tau = TAU_FACTOR x max |z32 - z64| of zero is drawn again until none is left: a ReLU that falls
    on different sides in float32 and float64 changes a whole mask entry, which no tolerance covers."""
    c = CASES[name]
    shape = shape_of(name)
    g = torch.Generator().manual_seed(1000 + NAMES.index(name))
    dims = [(c.W, c.s + c.a)] + [(c.W, c.W)] * (c.L - 1) + [(c.s, c.W)] + ([(1, c.W)] if c.reward else [])
    params = []
    for fo, fi in dims:
        bound = 1.0 / fi ** 0.5
        params.append(torch.rand((fo, fi), generator=g).mul(2 * bound).sub(bound).numpy())
        params.append(torch.rand((fo,), generator=g).mul(2 * bound).sub(bound).numpy())
    T = c.B if c.rows == "seq" else c.B + 5
    data = _draw(g, T, c.s, c.a, c.H)
    every = np.arange(T)
    redrawn = set()
    for _ in range(100):
        z64 = ref.preacts(params, data, every, shape, torch.float64)
        z32 = ref.preacts(params, data, every, shape, torch.float32)
        tau = TAU_FACTOR * float(np.max(np.abs(z32 - z64)))
        near = np.abs(z64).reshape(c.L, T, c.H, c.W).min(axis=(0, 2, 3)) < tau
        if not near.any():
            break
        bad = np.flatnonzero(near)
        redrawn.update(int(i) for i in bad)
        fresh = _draw(g, len(bad), c.s, c.a, c.H)
        for k in data:
            data[k][bad] = fresh[k]
    else:
        raise AssertionError(f"{name}: the redraws did not settle")
    rng = np.random.default_rng(NAMES.index(name))
    if c.rows == "seq":
        rows = np.arange(c.B)
    elif c.rows == "perm":
        rows = rng.permutation(T)[:c.B]
    else:
        rows = rng.integers(0, T, size=c.B)
        rows[0] = T - 1
        rows[1:4] = rows[4]
    rows = rows.astype(np.int64)
    for v in list(data.values()) + params + [rows]:
        v.setflags(write=False)
    return dict(params=params, data=data, rows=rows, T=T, tau=tau, redrawn=len(redrawn))


def other_rows(name):
    """A second member's rows for the ensemble test: another draw with replacement."""
    c, p = CASES[name], problem(name)
    return np.random.default_rng(500 + NAMES.index(name)).integers(0, p["T"], size=c.B).astype(np.int64)


@functools.lru_cache(maxsize=None)
def g64(name, other=False):
    p = problem(name)
    return ref.loss_and_grads(p["params"], p["data"], other_rows(name) if other else p["rows"], shape_of(name), torch.float64)


@functools.lru_cache(maxsize=None)
def g32(name):
    p = problem(name)
    return ref.loss_and_grads(p["params"], p["data"], p["rows"], shape_of(name), torch.float32)


def tensor_names(name):
    c = CASES[name]
    layers = [str(l) for l in range(c.L)] + ["out"] + (["rew"] if c.reward else [])
    return [f"d{k}_{l}" for l in layers for k in ("W", "b")]


def tensor_kind(label):
    """dW_0 / db_0, the hidden layers', the state head's, the reward head's."""
    k, l = label.split("_")
    return f"{k}_{'hidden' if l.isdigit() and l != '0' else l}"


def errors(name, grads):
    """[(tensor-relative, tile-relative)] of a list of gradients against the case's g64."""
    return [ref.err(x, y) for x, y in zip(grads, g64(name)["grads"])]


@functools.lru_cache(maxsize=None)
def e32(name):
    """[(tensor-relative, tile-relative)] per tensor of the float32 restatement's own error to float64."""
    return errors(name, g32(name)["grads"])


@functools.lru_cache(maxsize=None)
def e32_loss(name):
    return ref.loss_err(g32(name)["loss"], g64(name)["loss"])


@functools.lru_cache(maxsize=None)
def medians():
    """(median tensor-relative e32, median tile-relative e32, median loss e32) over every tensor (every
    non-zero loss) of every case of the table."""
    es = [e for n in NAMES for e in e32(n)]
    ls = [e for n in NAMES for e, l in zip(e32_loss(n), g64(n)["loss"]) if l != 0]
    return float(np.median([e[0] for e in es])), float(np.median([e[1] for e in es])), float(np.median(ls))


def bars(name, factor=BAR_FACTOR):
    """[(tensor-relative bar, tile-relative bar)] per tensor: factor x max(the case's e32, the table's median)."""
    m = medians()
    return [(factor * max(e[0], m[0]), factor * max(e[1], m[1])) for e in e32(name)]


def loss_bars(name, factor=BAR_FACTOR):
    return [factor * max(e, medians()[2]) for e in e32_loss(name)]


def mutant_misses(name):
    """{label: the largest tile-relative error / bar over the case's tensors} of every applicable mutant."""
    p, c = problem(name), CASES[name]
    out = {}
    for label in ref.applicable(shape_of(name), c.B):
        m = ref.loss_and_grads(p["params"], p["data"], p["rows"], shape_of(name), torch.float64, mutant=label)
        out[label] = max(e[1] / b[1] for e, b in zip(errors(name, m["grads"]), bars(name)))
    return out
