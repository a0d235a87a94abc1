"""The cases of tests/test_gpu_holdout.py (mbrl_eval_members against the float64 restatement of
tests/holdout_reference.py) as plain data plus CPU helpers. No GPU import.

The kernel's row tile is 16 positions p = r * horizon + h of one member (csrc/eval.hip EVAL_TM), its only
tile height: at horizon 1 the R of 15 / 16 / 17 and 31 / 32 / 33 lie on both sides of a tile edge, and the
horizon 2 and 3 cases put the edge inside a transition (R = 16 at horizon 2 is 32 positions, R = 17 at
horizon 3 is 51). The four waves of a workgroup split a layer's 16-neuron blocks four at a time, so W = 1,
33, 64, 255, 256, 520 and 1024 leave one, a partial and several full passes per wave; a layer's weights are
read 16 bytes at a time when K % 4 == 0 and the pointer allows it, else one by one (align "offset": that
member's parameters lie 4 bytes into a larger buffer, beside aligned members).

rows: "seq" (0 .. R - 1), "perm" (unsorted: a permutation's first R of T = R + 5), "repeat" (drawn with
replacement, unsorted, one index three times, T - 1 among them)."""
import collections
import functools

import numpy as np
import torch

import holdout_reference as href
import train_grad_reference as tref
from gd_grad_cases import BAR_FACTOR
from train_grad_cases import _draw

Case = collections.namedtuple("Case", "s a W L reward H E R rows offset")


def _c(s, a, W, L, reward, H, E, R, rows="perm", offset=()):
    return Case(s, a, W, L, reward, H, E, R, rows, tuple(offset))


CASES = {
    # ---- R on each side of every tile edge (horizon 1)
    "r1": _c(5, 1, 64, 2, 0, 1, 1, 1, rows="seq"),
    "r15": _c(5, 1, 33, 2, 1, 1, 2, 15),
    "r16": _c(5, 6, 64, 1, 0, 1, 2, 16),
    "r17": _c(5, 6, 64, 2, 1, 1, 1, 17, rows="repeat"),
    "r31": _c(17, 6, 64, 2, 0, 1, 2, 31),
    "r32": _c(17, 6, 33, 3, 1, 1, 1, 32),
    "r33": _c(1, 1, 64, 2, 0, 1, 2, 33, rows="repeat"),
    "r63": _c(5, 1, 64, 2, 0, 1, 1, 63),
    "r65_a0": _c(5, 0, 64, 2, 1, 1, 2, 65),
    "r257": _c(17, 6, 64, 2, 0, 1, 5, 257, rows="repeat"),
    # ---- horizon 2 and 3: the tile edge inside a transition
    "h2_r16": _c(5, 1, 33, 2, 0, 2, 2, 16),
    "h3_r17": _c(5, 6, 64, 2, 1, 3, 1, 17),
    "h2_r1": _c(5, 1, 64, 3, 0, 2, 1, 1, rows="seq"),
    "h3_r257": _c(1, 1, 33, 1, 0, 3, 2, 257, rows="repeat"),
    # ---- widths and depths
    "w1": _c(5, 1, 1, 1, 0, 1, 2, 17),
    "w33_l8": _c(5, 6, 33, 8, 1, 1, 1, 33),
    "w255": _c(17, 6, 255, 2, 0, 1, 2, 33),
    "w256": _c(17, 6, 256, 2, 1, 1, 2, 31),
    "w520": _c(5, 1, 520, 2, 0, 1, 1, 33),
    "w1024": _c(17, 6, 1024, 1, 0, 1, 2, 17),
    "w1024_l2": _c(5, 1, 1024, 2, 1, 2, 1, 15),
    "l8_w64": _c(5, 1, 64, 8, 0, 1, 2, 32),
    "l3_w256": _c(33, 6, 256, 3, 1, 1, 1, 65),
    # ---- wide inputs: s + a = 81, 65, 88; no actions
    "s33_a48": _c(33, 48, 64, 2, 0, 1, 2, 33),
    "k65": _c(17, 48, 64, 2, 1, 1, 1, 17),
    "k88": _c(40, 48, 64, 2, 0, 1, 2, 33),
    "s33_a0": _c(33, 0, 64, 2, 1, 1, 2, 16),
    "s33_a0_w1": _c(33, 0, 1, 1, 0, 1, 1, 15),
    "s1_a0": _c(1, 0, 33, 2, 0, 1, 1, 31),
    # ---- members
    "e5": _c(5, 1, 64, 2, 0, 1, 5, 33),
    "e8": _c(5, 6, 33, 2, 1, 2, 8, 17),
    "e8_w256": _c(17, 6, 256, 2, 0, 1, 8, 63),
    "s17_h3_e5": _c(17, 1, 255, 3, 1, 3, 5, 65, rows="repeat"),
    # ---- a member at 4-byte-offset parameters beside aligned ones (K % 4 == 0 past layer 0: the pointer decides)
    "offset_first": _c(5, 1, 64, 2, 1, 1, 2, 33, offset=(0,)),
    "offset_mid": _c(6, 2, 64, 3, 0, 1, 5, 32, offset=(2,)),
    "offset_last": _c(6, 2, 64, 2, 1, 1, 2, 17, rows="repeat", offset=(1,)),
}
NAMES = list(CASES)

# the values the table must reach (tests/test_holdout_host.py)
REACH = dict(W={1, 33, 64, 255, 256, 520, 1024}, L={1, 2, 3, 8}, s={1, 5, 17, 33}, a={0, 1, 6, 48}, K0={65, 88},
             H={1, 2, 3}, reward={0, 1}, E={1, 2, 5, 8}, R={1, 15, 16, 17, 31, 32, 33, 63, 65, 257},
             rows={"perm", "repeat"})


def shape_of(name):
    c = CASES[name]
    return (c.s, c.a, c.W, c.L, c.reward, c.H)


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(params [E] lists, data, rows, T) of a case (shared: do not write to it): torch's default Linear
    initialisation per member, transitions drawn as tests/train_grad_cases.py draws them."""
    c = CASES[name]
    g = torch.Generator().manual_seed(7000 + NAMES.index(name))
    dims = [(c.W, c.s + c.a)] + [(c.W, c.W)] * (c.L - 1) + [(c.s, c.W)] + ([(1, c.W)] if c.reward else [])
    params = []
    for _ in range(c.E):
        member = []
        for fo, fi in dims:
            bound = 1.0 / fi ** 0.5
            member.append(torch.rand((fo, fi), generator=g).mul(2 * bound).sub(bound).numpy())
            member.append(torch.rand((fo,), generator=g).mul(2 * bound).sub(bound).numpy())
        params.append(member)
    T = c.R if c.rows == "seq" else c.R + 5
    data = _draw(g, T, c.s, c.a, c.H)
    rng = np.random.default_rng(NAMES.index(name))
    if c.rows == "seq":
        rows = np.arange(c.R)
    elif c.rows == "perm":
        rows = rng.permutation(T)[:c.R]
    else:
        rows = rng.integers(0, T, size=c.R)
        rows[0] = T - 1
        rows[1:4] = rows[4]
    rows = rows.astype(np.int64)
    for v in list(data.values()) + [p for m in params for p in m] + [rows]:
        v.setflags(write=False)
    return dict(params=params, data=data, rows=rows, T=T)


@functools.lru_cache(maxsize=None)
def ref(name, e, dtype=torch.float64):
    p = problem(name)
    return href.evaluate(p["params"][e], p["data"], p["rows"], shape_of(name), dtype)


KINDS = ("row_err", "row_rew_err")


def errors(name, e, got):
    """{kind: tensor-relative error} of member e's row_err / row_rew_err (train_grad_reference.err) and
    {"loss": [3 relative errors]} against the float64 restatement."""
    r64 = ref(name, e)
    out = {k: tref.err(got[k], r64[k])[0] for k in KINDS if r64[k] is not None}
    if got.get("loss") is not None:
        out["loss"] = tref.loss_err(got["loss"], r64["loss"])
    return out


@functools.lru_cache(maxsize=None)
def e32(name, e):
    """The float32 restatement's own error to float64."""
    return errors(name, e, ref(name, e, torch.float32))


@functools.lru_cache(maxsize=None)
def medians():
    """{kind: the median e32 over every member of every case}; "loss" over every non-zero loss entry."""
    out = {}
    for k in KINDS:
        out[k] = float(np.median([e32(n, e)[k] for n in NAMES for e in range(CASES[n].E) if k in e32(n, e)]))
    out["loss"] = float(np.median([x for n in NAMES for e in range(CASES[n].E)
                                   for x, l in zip(e32(n, e)["loss"], ref(n, e)["loss"]) if l != 0]))
    return out


def bars(name, e, factor=BAR_FACTOR):
    """The project's native-gradient bar (tests/train_grad_cases.py bars): factor x max(the float32
    restatement's error on this tensor, the table's median of it)."""
    m, own = medians(), e32(name, e)
    out = {k: factor * max(own[k], m[k]) for k in KINDS if k in own}
    out["loss"] = [factor * max(x, m["loss"]) for x in own["loss"]]
    return out
