"""The Gaussian negative log-likelihood of include/mbrl_cem.h (mbrl_train_grads_nll), restated in torch on the
package's ProbabilisticModel at any dtype -- float64 is the reference, a float32 CPU run of the same chain sets
the bars -- with its row values, its autograd gradients and the single-mistake mutants of the host test, and the
case table the CPU and the GPU tests share. No GPU import.

Positions are p = b * H + h; a case is E members of one shape, each on its own rows of one dataset."""
import collections
import functools

import numpy as np
import torch

import train_grad_reference as tref
from gd_grad_cases import BAR_FACTOR, MUTANT_FACTOR

TAU_FACTOR = 32.0       # every ReLU and softplus argument lies above TAU_FACTOR x max |f32 - f64| of the case

MUTANTS = ("exp_plus", "no_lv", "no_sigmoid", "bounds_swapped", "rows_swapped", "scale_b", "dr_shift")

Case = collections.namedtuple("Case", "s a W L H B E rows offset")


def _c(s, a, W, L, H, B, E=1, rows="draw", offset=False):
    return Case(s, a, W, L, H, B, E, rows, offset)


CASES = {
    # the batch on both sides of the 16-position tile (B * H positions), and one row
    "b1": _c(8, 1, 33, 2, 3, 1),
    "b15_s1": _c(1, 1, 33, 2, 3, 15),
    "b16_s8": _c(8, 6, 64, 2, 1, 16, E=2),          # 2 s = 16: one whole block of output neurons
    "b17_s9": _c(9, 0, 33, 3, 3, 17),               # 2 s = 18: a second block of two; no actions
    "b33_s17": _c(17, 6, 64, 2, 3, 33, E=5),
    "s33_l1": _c(33, 1, 33, 1, 1, 17),              # 2 s = 66 > W
    "w1": _c(8, 1, 1, 2, 3, 17),
    "w256": _c(9, 6, 256, 2, 1, 17),
    "l8": _c(8, 1, 33, 8, 1, 17, E=8),
    "w1024": _c(8, 1, 1024, 1, 1, 15),              # the LDS limit of the hidden width
    "repeats": _c(8, 1, 33, 2, 3, 33, E=2, rows="repeat"),
    "offset": _c(9, 6, 36, 2, 3, 17, E=2, offset=True),
}
NAMES = list(CASES)
DIMENSIONS = dict(B=(1, 15, 16, 17, 33), s=(1, 8, 9, 17, 33), a=(0, 1, 6), W=(1, 33, 64, 256, 1024), L=(1, 2, 3, 8),
                  H=(1, 3), E=(1, 2, 5, 8))


def shape_of(name):
    c = CASES[name]
    return (c.s, c.a, c.W, c.L, c.H)


def softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def loss_and_grads(params, bounds, data, rows, shape, dtype, mutant=None):
    """One member on rows [B]: dict(loss (nll, mse, mean_lv), row_nll / row_err / row_lv [B][H], grads (params'
    order), pre [L][P][W] hidden pre-activations, sp [2][P][s] the two softplus arguments)."""
    s, a, W, L, H = shape
    B = len(rows)
    w = [torch.tensor(np.asarray(p), dtype=dtype, requires_grad=True) for p in params]
    lo, hi = (torch.tensor(np.asarray(b), dtype=dtype) for b in bounds)
    idx = torch.as_tensor(np.array(rows))
    st, ac, ns = (torch.tensor(np.asarray(data[k]), dtype=dtype)[idx] for k in ("states", "actions", "next_states"))
    x = torch.cat([st.reshape(B * H, s), ac.reshape(B * H, a)], dim=1)
    y = ns.reshape(B * H, s)
    pre = []
    for l in range(L):
        z = x @ w[2 * l].T + w[2 * l + 1]
        pre.append(z.detach().numpy())
        x = torch.relu(z)
    out = x @ w[2 * L].T + w[2 * L + 1]
    m, r = (out[:, s:], out[:, :s]) if mutant == "rows_swapped" else (out[:, :s], out[:, s:])
    if mutant == "bounds_swapped":
        a1, u = r - lo, lo + softplus(r - lo)
        a2 = hi - u
        lv = hi - softplus(a2)
    else:
        a1 = hi - r
        u = hi - softplus(a1)
        if mutant == "no_sigmoid":          # the factor sigmoid(max - r) dropped from dr: u's value, r's slope
            u = r + (u - r).detach()
        a2 = u - lo
        lv = lo + softplus(a2)
    d2 = (m - y) ** 2
    w2 = d2 * torch.exp(lv if mutant == "exp_plus" else -lv)
    elem = w2 if mutant == "no_lv" else w2 + lv
    denom = B if mutant == "scale_b" else B * s
    row = [v.sum(1).reshape(B, H) for v in (elem, d2, lv)]
    loss = [(v.sum(0) / denom).sum() for v in row]
    if mutant == "dr_shift":                # row j's dr taken from row j + 1 (the last one from row 0)
        g_out = torch.autograd.grad(loss[0], out, retain_graph=True)[0]
        g_out = torch.cat([g_out[:, :s], torch.roll(g_out[:, s:], -1, dims=1)], dim=1)
        grads = torch.autograd.grad(out, w, grad_outputs=g_out)
    else:
        grads = torch.autograd.grad(loss[0], w)
    return dict(loss=np.array([float(v.detach()) for v in loss]), row_nll=row[0].detach().numpy(),
                row_err=row[1].detach().numpy(), row_lv=row[2].detach().numpy(),
                grads=[g.numpy() for g in grads], pre=np.stack(pre),
                sp=np.stack([a1.detach().numpy(), a2.detach().numpy()]))


def applicable(shape):
    """The mutants that change this shape's gradient (one state dimension has no neighbour row and one scale)."""
    s = shape[0]
    return [m for m in MUTANTS if s > 1 or m not in ("scale_b", "dr_shift")]


def _draw(seed, c):
    g = torch.Generator().manual_seed(seed)
    dims = [(c.W, c.s + c.a)] + [(c.W, c.W)] * (c.L - 1) + [(2 * c.s, c.W)]
    members = []
    for _ in range(c.E):
        params = []
        for fo, fi in dims:
            bound = 1.0 / fi ** 0.5
            params.append(torch.rand((fo, fi), generator=g).mul(2 * bound).sub(bound).numpy())
            params.append(torch.rand((fo,), generator=g).mul(2 * bound).sub(bound).numpy())
        # the raw log-variances in three regimes, dimension by dimension: below min, between the bounds, above max
        regime = np.array([-7.0, -2.0, 3.0], np.float32)[np.arange(c.s) % 3]
        params[-1] = params[-1].copy()
        params[-1][c.s:] += regime
        members.append(params)
    lo = (-4.0 + 0.25 * torch.rand(c.s, generator=g)).numpy()
    hi = (0.5 + 0.25 * torch.rand(c.s, generator=g)).numpy()
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
    return members, (lo, hi), data, rows, T


def sides_agree(v32, v64):
    """(ok, tau): no entry of v64 within tau = TAU_FACTOR x max |v32 - v64| of zero, every sign equal."""
    tau = TAU_FACTOR * float(np.max(np.abs(v32 - v64)))
    return float(np.min(np.abs(v64))) >= tau and np.array_equal(v32 > 0, v64 > 0), tau


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(members [E][params], bounds, data, rows [E][B], T, seed) of a case (shared: do not write to it). Seeds
    are tried in order until no hidden pre-activation and no softplus argument of any member and position lies
    within tau of zero (sides_agree): a ReLU on different sides in float32 and float64 changes a whole mask
    entry, which no tolerance covers."""
    c = CASES[name]
    for k in range(50):
        seed = 9000 + 100 * NAMES.index(name) + k
        members, bounds, data, rows, T = _draw(seed, c)
        ok = True
        for e in range(c.E):
            r64 = loss_and_grads(members[e], bounds, data, rows[e], shape_of(name), torch.float64)
            r32 = loss_and_grads(members[e], bounds, data, rows[e], shape_of(name), torch.float32)
            ok = ok and sides_agree(r32["pre"], r64["pre"])[0] and sides_agree(r32["sp"], r64["sp"])[0]
        if ok:
            break
    else:
        raise AssertionError(f"{name}: no seed keeps every ReLU and softplus argument on one side")
    for v in list(data.values()) + [p for m in members for p in m] + [rows, *bounds]:
        v.setflags(write=False)
    return dict(members=members, bounds=bounds, data=data, rows=rows, T=T, seed=seed)


@functools.lru_cache(maxsize=None)
def g64(name, e=0, mutant=None):
    p = problem(name)
    return loss_and_grads(p["members"][e], p["bounds"], p["data"], p["rows"][e], shape_of(name), torch.float64, mutant)


@functools.lru_cache(maxsize=None)
def g32(name, e=0):
    p = problem(name)
    return loss_and_grads(p["members"][e], p["bounds"], p["data"], p["rows"][e], shape_of(name), torch.float32)


ROWS = ("row_nll", "row_err", "row_lv")


def tensor_names(name):
    c = CASES[name]
    return [f"d{k}_{l}" for l in [str(l) for l in range(c.L)] + ["head"] for k in ("W", "b")] + list(ROWS)


def values(result):
    """What the comparisons look at: the gradients, then the three row arrays."""
    return list(result["grads"]) + [result[k] for k in ROWS]


def errors(name, vals, e=0):
    """[(tensor-relative, tile-relative)] (train_grad_reference.err) of values() against member e's g64."""
    return [tref.err(x, y) for x, y in zip(vals, values(g64(name, e)))]


@functools.lru_cache(maxsize=None)
def e32(name, e=0):
    return errors(name, values(g32(name, e)), e)


@functools.lru_cache(maxsize=None)
def medians():
    """(median tensor-relative, median tile-relative) float32 error over every tensor of member 0 of every case."""
    es = [x for n in NAMES for x in e32(n)]
    return float(np.median([x[0] for x in es])), float(np.median([x[1] for x in es]))


def bars(name, e=0, factor=BAR_FACTOR):
    """[(tensor-relative bar, tile-relative bar)] per value of member e: factor x max(the member's own float32
    error, the table's median) -- tests/train_grad_cases.py's rule."""
    m = medians()
    return [(factor * max(x[0], m[0]), factor * max(x[1], m[1])) for x in e32(name, e)]


def mutant_misses(name):
    """{label: the largest tile-relative error / bar over member 0's values} of every applicable mutant."""
    out = {}
    for label in applicable(shape_of(name)):
        vals = values(g64(name, 0, label))
        out[label] = max(x[1] / b[1] for x, b in zip(errors(name, vals), bars(name)))
    return out


__all__ = ["CASES", "NAMES", "DIMENSIONS", "MUTANTS", "BAR_FACTOR", "MUTANT_FACTOR", "problem", "g64", "g32", "bars",
           "errors", "values", "mutant_misses", "shape_of", "tensor_names", "loss_and_grads", "applicable"]
