"""The case table of mbrl_train_grads_open_loop's tests: the smallest shapes that reach each hazard of the
forward kernel's seam, the backward kernel's carry and the position-summed weight gradients. No GPU import.

A case is E members of one shape, each on its own rows of one dataset. Member 0 is the member the float64
comparison's bars are computed for on the CPU (g64 / g32); the GPU test compares every member."""
import collections
import functools

import numpy as np
import torch

import train_grad_reference as tref
import train_open_loop_reference as ref
from gd_grad_cases import BAR_FACTOR, MUTANT_FACTOR

TAU_FACTOR = 32.0       # every |z64| of a case lies above TAU_FACTOR x max |z32 - z64|: no ReLU changes side

ALIVE = 0.2             # at least this share of every hidden layer's (row, unit) entries is active at every step

Case = collections.namedtuple("Case", "s a W L reward H B E rows offset")


def _c(s, a, W, L, reward, H, B, E=1, rows="draw", offset=False):
    return Case(s, a, W, L, reward, H, B, E, rows, offset)


CASES = {
    # the horizon: 1 (mbrl_train_grads_ensemble's gradient), 2, 3, 7 and the planners' 30
    "h1_b17": _c(5, 2, 33, 2, 1, 1, 17, E=2),
    "h2_b16": _c(5, 2, 33, 2, 0, 2, 16),
    "h3_b15": _c(5, 2, 33, 2, 1, 3, 15),
    "h7_b33": _c(5, 2, 33, 2, 1, 7, 33),
    "h30_w64": _c(17, 6, 64, 2, 0, 30, 17),
    # the batch on both sides of the 16-row tile, and one row
    "b1": _c(4, 1, 33, 2, 1, 3, 1),
    "b257": _c(3, 1, 17, 1, 1, 2, 257),
    # the seam: (s, a) around the 16-deep chunk, s > W, s = 1
    "s15_a2": _c(15, 2, 33, 2, 1, 3, 17),
    "s16_a1": _c(16, 1, 33, 1, 1, 3, 16),
    "s17_a0": _c(17, 0, 33, 2, 1, 3, 17),
    "s5_a12": _c(5, 12, 33, 3, 0, 3, 17),
    "s33_a48": _c(33, 48, 64, 2, 1, 2, 17),
    "s_above_w": _c(40, 3, 17, 2, 0, 3, 17),
    "s1": _c(1, 1, 33, 2, 1, 3, 17),
    # both heads at a = 0, 1, 6
    "a0_plain": _c(6, 0, 33, 2, 0, 3, 17),
    "a1_plain": _c(6, 1, 33, 2, 0, 3, 17),
    "a6_reward": _c(17, 6, 33, 2, 1, 3, 17),
    # depth and width
    "l1": _c(5, 2, 64, 1, 1, 3, 17),
    "l3": _c(5, 2, 33, 3, 1, 3, 17),
    "l8": _c(5, 2, 33, 8, 0, 2, 17),
    "w1": _c(3, 1, 1, 2, 1, 3, 17),
    "w255": _c(5, 2, 255, 2, 0, 2, 17),
    "w256": _c(5, 2, 256, 2, 1, 2, 17),
    "w520": _c(5, 2, 520, 2, 0, 2, 15),
    "w1024": _c(5, 2, 1024, 1, 1, 2, 15),
    # members: 2, 5, 8; repeated rows; parameters and gradients 4 bytes off beside aligned ones
    "e5": _c(17, 6, 64, 2, 0, 3, 33, E=5),
    "e8": _c(5, 2, 33, 2, 1, 2, 17, E=8),
    "repeats": _c(5, 2, 33, 2, 1, 3, 33, E=2, rows="repeat"),
    "offset": _c(5, 2, 36, 2, 1, 3, 17, E=2, offset=True),
}
NAMES = list(CASES)


def shape_of(name):
    c = CASES[name]
    return (c.s, c.a, c.W, c.L, c.reward, c.H)


def _draw(seed, c):
    g = torch.Generator().manual_seed(seed)
    dims = [(c.W, c.s + c.a)] + [(c.W, c.W)] * (c.L - 1) + [(c.s, c.W)] + ([(1, c.W)] if c.reward else [])
    members = []
    for _ in range(c.E):
        params = []
        for fo, fi in dims:
            bound = 1.0 / fi ** 0.5
            params.append(torch.rand((fo, fi), generator=g).mul(2 * bound).sub(bound).numpy())
            params.append(torch.rand((fo,), generator=g).mul(2 * bound).sub(bound).numpy())
        members.append(params)
    T = c.B + 5
    data = dict(states=torch.randn((T, c.H, c.s), generator=g).numpy(),
                actions=torch.rand((T, c.H, c.a), generator=g).mul(2).sub(1).numpy(),
                next_states=torch.randn((T, c.H, c.s), generator=g).numpy(),
                rewards=torch.randn((T, c.H), generator=g).numpy())
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, T, size=(c.E, c.B)).astype(np.int64)
    if c.rows == "repeat":
        rows[0, 1:9] = rows[0, 0]
        rows[1, :] = 3
    return members, data, rows, T


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(members [E][params], data, rows [E][B], T, tau, seed) of a case (shared: do not write to it). Seeds
    are tried in order until no hidden pre-activation of any member, row and step lies within tau =
    TAU_FACTOR x max |z32 - z64| of zero: a ReLU on different sides in float32 and float64 changes a whole
    mask entry, and in an open-loop chain everything after it, which no tolerance covers. A draw in which a
    hidden layer is (nearly) dead is passed over too: no gradient would flow through the feedback."""
    c = CASES[name]
    for k in range(50):
        seed = 7000 + 100 * NAMES.index(name) + k
        members, data, rows, T = _draw(seed, c)
        tau, ok = 0.0, True
        for e in range(c.E):
            z64 = ref.loss_and_grads(members[e], data, rows[e], shape_of(name), torch.float64)["pre"]
            z32 = ref.loss_and_grads(members[e], data, rows[e], shape_of(name), torch.float32)["pre"]
            t = TAU_FACTOR * float(np.max(np.abs(z32 - z64)))
            tau = max(tau, t)
            ok = ok and float(np.min(np.abs(z64))) >= t and np.array_equal(z32 > 0, z64 > 0)
            ok = ok and float((z64 > 0).mean(axis=(2, 3)).min()) >= ALIVE     # (no dead layer: the carry is not zero)
        if ok:
            break
    else:
        raise AssertionError(f"{name}: no seed keeps every ReLU on one side")
    for v in list(data.values()) + [p for m in members for p in m] + [rows]:
        v.setflags(write=False)
    return dict(members=members, data=data, rows=rows, T=T, tau=tau, seed=seed)


@functools.lru_cache(maxsize=None)
def g64(name, e=0):
    p = problem(name)
    return ref.loss_and_grads(p["members"][e], p["data"], p["rows"][e], shape_of(name), torch.float64)


@functools.lru_cache(maxsize=None)
def g32(name, e=0):
    p = problem(name)
    return ref.loss_and_grads(p["members"][e], p["data"], p["rows"][e], shape_of(name), torch.float32)


def tensor_names(name):
    c = CASES[name]
    layers = [str(l) for l in range(c.L)] + ["out"] + (["rew"] if c.reward else [])
    return [f"d{k}_{l}" for l in layers for k in ("W", "b")]


def errors(name, grads, e=0):
    """[(tensor-relative, tile-relative)] (train_grad_reference.err) of gradients against member e's g64."""
    return [tref.err(x, y) for x, y in zip(grads, g64(name, e)["grads"])]


@functools.lru_cache(maxsize=None)
def e32(name, e=0):
    return errors(name, g32(name, e)["grads"], e)


@functools.lru_cache(maxsize=None)
def medians():
    """(median tensor-relative, median tile-relative) float32 error over every tensor of member 0 of every case."""
    es = [x for n in NAMES for x in e32(n)]
    return float(np.median([x[0] for x in es])), float(np.median([x[1] for x in es]))


def bars(name, e=0, factor=BAR_FACTOR):
    """[(tensor-relative bar, tile-relative bar)] per tensor of member e: factor x max(the member's own float32
    error, the table's median) -- tests/train_grad_cases.py's rule."""
    m = medians()
    return [(factor * max(x[0], m[0]), factor * max(x[1], m[1])) for x in e32(name, e)]


def mutant_misses(name):
    """{label: the largest tile-relative error / bar over member 0's tensors} of every applicable mutant."""
    p, c = problem(name), CASES[name]
    out = {}
    for label in ref.applicable(shape_of(name), c.B):
        m = ref.loss_and_grads(p["members"][0], p["data"], p["rows"][0], shape_of(name), torch.float64, mutant=label)
        out[label] = max(x[1] / b[1] for x, b in zip(errors(name, m["grads"]), bars(name)))
    return out


__all__ = ["CASES", "NAMES", "BAR_FACTOR", "MUTANT_FACTOR", "problem", "g64", "g32", "bars", "errors",
           "mutant_misses", "shape_of", "tensor_names"]
