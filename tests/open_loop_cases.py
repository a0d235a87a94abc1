"""The cases of tests/test_gpu_open_loop.py (mbrl_eval_members_open_loop against the float64 restatement of
tests/open_loop_reference.py) as plain data plus CPU helpers. No GPU import.

The kernel's tile is 16 rows r of one member (csrc/eval.hip EVAL_TM), each run through all H steps by one
workgroup: R = 1, 15, 16, 17, 33 and 257 lie on both sides of a tile edge. Between two steps the workgroup
rewrites the input columns from s on: the (s, a) of the seam cases put the boundaries s, s + reward, s + a and
their 16-column blocks in every order -- (15, 2): the actions straddle the output layer's last block;
(16, 1) and (17, 0): the reward head's column is the first or the only one to rewrite; (5, 12): the actions
spill into a block only hidden layers wrote; (33, 48): s + a > W. Both parities of L alternate which of the two
buffers holds the outputs. Parameters and data are drawn as tests/holdout_cases.py draws them (its seeds
offset), rows likewise.

No case had to change its seed for the ReLU condition of tests/test_open_loop_host.py."""
import collections
import functools

import numpy as np
import torch

import open_loop_reference as oref
import train_grad_reference as tref
from gd_grad_cases import BAR_FACTOR
from train_grad_cases import _draw

Case = collections.namedtuple("Case", "s a W L reward H E R rows offset seed")


def _c(s, a, W, L, reward, H, E, R, rows="perm", offset=(), seed=0):
    return Case(s, a, W, L, reward, H, E, R, rows, tuple(offset), seed)


CASES = {
    # ---- horizons, R on each side of a tile edge, the seam's (s, a)
    "h1_r1": _c(5, 1, 64, 2, 0, 1, 1, 1, rows="seq"),
    "h1_r33": _c(17, 6, 64, 2, 1, 1, 2, 33, rows="repeat"),
    "h2_r15_s15_a2": _c(15, 2, 64, 2, 0, 2, 2, 15),
    "h3_r16_s16_a1": _c(16, 1, 64, 1, 1, 3, 2, 16),
    "h7_r17_s17_a0": _c(17, 0, 64, 2, 1, 7, 1, 17, rows="repeat"),
    "h30_w64": _c(17, 6, 64, 2, 0, 30, 2, 33),
    "h3_r257_s5_a12": _c(5, 12, 64, 3, 0, 3, 5, 257, rows="repeat"),
    "s33_a48": _c(33, 48, 64, 2, 1, 2, 2, 33),
    "s33_a0_w1": _c(33, 0, 1, 1, 0, 2, 1, 15),
    "s1_a1": _c(1, 1, 33, 2, 0, 3, 2, 17),
    "s1_a0": _c(1, 0, 64, 2, 1, 2, 1, 16),
    "a1_rew0": _c(16, 1, 64, 2, 0, 2, 1, 17),
    "a6_rew": _c(17, 6, 64, 2, 1, 3, 1, 33),
    # ---- depths and widths
    "l8_w33": _c(5, 1, 33, 8, 1, 2, 2, 17),
    "l3_w255": _c(17, 6, 255, 3, 0, 2, 2, 16),
    "w256": _c(17, 6, 256, 2, 1, 3, 2, 17),
    "w520": _c(5, 1, 520, 2, 0, 2, 1, 33),
    "w1024_h2": _c(17, 6, 1024, 1, 0, 2, 1, 17),
    "w1": _c(5, 1, 1, 1, 0, 2, 2, 17),
    # ---- members
    "e8": _c(5, 6, 33, 2, 1, 2, 8, 17),
    "e5_h7": _c(17, 6, 64, 2, 0, 7, 5, 33, rows="repeat"),
    # ---- a member at 4-byte-offset parameters beside aligned ones
    "offset_mid": _c(6, 2, 64, 3, 0, 2, 5, 33, offset=(2,)),
    "offset_first": _c(5, 1, 64, 2, 1, 3, 2, 17, offset=(0,)),
}
NAMES = list(CASES)

# the values the table must reach (tests/test_open_loop_host.py)
REACH = dict(H={1, 2, 3, 7, 30}, R={1, 15, 16, 17, 33, 257}, rows={"perm", "repeat"},
             seam={(15, 2), (16, 1), (17, 0), (5, 12), (33, 48)}, L={1, 2, 3, 8},
             W={1, 33, 64, 255, 256, 520, 1024}, E={1, 2, 5, 8},
             reward_at_a={(0, 0), (1, 0), (0, 1), (1, 1), (0, 6), (1, 6)})


def shape_of(name):
    c = CASES[name]
    return (c.s, c.a, c.W, c.L, c.reward, c.H)


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(params [E] lists, data, rows, T) of a case (shared: do not write to it), drawn as
    tests/holdout_cases.py problem() draws."""
    c = CASES[name]
    g = torch.Generator().manual_seed(9000 + 100 * c.seed + NAMES.index(name))
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
def ref(name, e, dtype=torch.float64, mutant=None):
    p = problem(name)
    return oref.evaluate(p["params"][e], p["data"], p["rows"], shape_of(name), dtype, mutant)


KINDS = ("row_err", "row_rew_err", "pred")


def errors(name, e, got):
    """{kind: tensor-relative error (train_grad_reference.err) of member e's row_err / row_rew_err / pred} and
    {"loss": [3 relative errors]} against the float64 restatement; kinds `got` lacks are left out."""
    r64 = ref(name, e)
    out = {k: tref.err(np.asarray(got[k]).reshape(len(r64[k]), -1), r64[k].reshape(len(r64[k]), -1))[0]
           for k in KINDS if r64[k] is not None and got.get(k) is not None}
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
    """tests/holdout_cases.py bars, per tensor: factor x max(the float32 restatement's error on this tensor, the
    table's median of it)."""
    m, own = medians(), e32(name, e)
    out = {k: factor * max(own[k], m[k]) for k in KINDS if k in own}
    out["loss"] = [factor * max(x, m["loss"]) for x in own["loss"]]
    return out
