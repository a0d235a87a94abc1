"""The gradient mbrl_train_grads computes, restated on the CPU in torch: the documented per-batch loss
(models.py: MSELoss of the predicted next state, plus MSELoss of the reward head for ModelWithReward,
summed over the horizon steps) on rows `rows` of the stacked transitions (repeats allowed), and its
gradient with respect to every Linear. No GPU import.

    X      = [states[rows], actions[rows]]               [R = B H][s + a], row r = transition rows[r / H], step r % H
    z_l    = x_l W_l^T + b_l,  x_{l+1} = relu(z_l)        l = 0 .. L - 1
    Y      = x_L [W_out; w_rew]^T + [b_out; b_rew]        [R][J], J = s (+ 1)
    loss   = sum (Y_s - next_states)^2 / (B s)  +  sum (y_r - rewards)^2 / B

The backward pass is written out layer by layer (and tests/test_train_grad_host.py holds it to autograd),
so that mutants() can put exactly one thing wrong while every forward value stays the same.
dtype = float64 is the reference g64; dtype = float32 is the restatement g32 (plain torch CPU matmuls,
not the kernel's summation order), whose distance to g64 sets every bar."""
import numpy as np
import torch

TILE = 32      # the kernels' C tile edge: the tile-relative metric's tiles

# label -> what is wrong
MUTANTS = {
    "2/(B s) -> 2/B": "the state columns' dY scale loses the 1 / s",
    "head scales swapped": "the reward scale 2 / B on the state columns and 2 / (B s) on the reward column",
    "last batch row dropped": "row R - 1 contributes to no gradient",
    "dW_0 column K0-1 dropped": "the last input column of the layer-0 weight gradient is not written",
    "dW_0 columns >= 64 dropped": "the layer-0 weight gradient past its 64th input column is not written",
    "mask of the other parity": "dH_{L-2} is masked with layer L - 2's neighbour (the other dh ping-pong slot)",
    "db last row tile missing": "db_0 sums every 32-row tile of dH_0 but the last",
    "steps h > 0 dropped": "only horizon step 0 of every transition contributes",
    "reward column dropped from dH": "dH_{L-1} = dY_s W_out without the reward head's share",
}


def applicable(shape, B):
    """The labels of MUTANTS that change this shape's gradient."""
    s, a, W, L, reward, H = shape
    R = B * H
    out = ["dW_0 column K0-1 dropped"]
    if s >= 2:
        out.append("2/(B s) -> 2/B")
    if s >= 2 and reward:
        out.append("head scales swapped")
    if R >= 2:
        out.append("last batch row dropped")
    if s + a > 64:
        out.append("dW_0 columns >= 64 dropped")
    if L >= 2:
        out.append("mask of the other parity")
    if R > TILE:
        out.append("db last row tile missing")
    if H >= 2:
        out.append("steps h > 0 dropped")
    if reward:
        out.append("reward column dropped from dH")
    return out


def _t(x, dtype):
    return torch.from_numpy(np.array(x, np.float32)).to(dtype)


def batch(data, rows, shape, dtype):
    """(X [R][s + a], next states [R][s], rewards [R]) of the batch's rows, in `dtype`."""
    s, a, W, L, reward, H = shape
    rows = np.asarray(rows, np.int64)
    R = len(rows) * H
    X = np.concatenate([data["states"][rows].reshape(R, s), data["actions"][rows].reshape(R, a)], axis=1)
    return _t(X, dtype), _t(data["next_states"][rows].reshape(R, s), dtype), _t(data["rewards"][rows].reshape(R), dtype)


def preacts(params, data, rows, shape, dtype):
    """Every hidden layer's pre-activations [L][R][W] as float64 NumPy."""
    L = shape[3]
    P = [_t(p, dtype) for p in params]
    x = batch(data, rows, shape, dtype)[0]
    out = []
    for l in range(L):
        z = x @ P[2 * l].T + P[2 * l + 1]
        out.append(z.double().numpy())
        x = torch.relu(z)
    return np.stack(out)


def loss_and_grads(params, data, rows, shape, dtype, mutant=None):
    """params: [W_0, b_0, ..., W_out, b_out(, w_rew, b_rew)] as float32 arrays; data: dict of the stacked
    transitions (states / actions / next_states [T][H][.], rewards [T][H]); rows: the batch's transitions.
    Returns dict(loss=[total, state, reward], grads=[one per parameter], pre=[L][R][W]), float64 NumPy,
    every operation carried out in `dtype`."""
    assert mutant is None or mutant in MUTANTS, mutant
    s, a, W, L, reward, H = shape
    B = len(rows)
    R = B * H
    P = [_t(p, dtype) for p in params]
    assert len(P) == 2 * (L + 1 + reward)
    X, Ts, Tr = batch(data, rows, shape, dtype)
    xs, zs = [X], []
    for l in range(L):
        z = xs[-1] @ P[2 * l].T + P[2 * l + 1]
        zs.append(z)
        xs.append(torch.relu(z))
    h = xs[-1]
    Ys = h @ P[2 * L].T + P[2 * L + 1]
    ds = Ys - Ts
    loss_s = torch.sum(ds * ds) / (B * s)
    scale_s, scale_r = 2.0 / (B * s), 2.0 / B
    if mutant == "2/(B s) -> 2/B":
        scale_s = 2.0 / B
    if mutant == "head scales swapped":
        scale_s, scale_r = scale_r, scale_s
    dY = ds * scale_s
    Wout = P[2 * L]
    loss_r = torch.zeros((), dtype=dtype)
    if reward:
        dr = (h @ P[2 * L + 2].T + P[2 * L + 3]).reshape(R) - Tr
        loss_r = torch.sum(dr * dr) / B
        dY = torch.cat([dY, (dr * scale_r).reshape(R, 1)], dim=1)
        Wout = torch.cat([Wout, P[2 * L + 2]], dim=0)
    if mutant == "last batch row dropped":
        dY = dY.clone()
        dY[R - 1] = 0
    if mutant == "steps h > 0 dropped":
        dY = dY * (torch.arange(R) % H == 0).to(dtype).reshape(R, 1)
    grads = [None] * len(P)
    dWout, dbout = dY.T @ h, dY.sum(0)
    grads[2 * L], grads[2 * L + 1] = dWout[:s], dbout[:s]
    if reward:
        grads[2 * L + 2], grads[2 * L + 3] = dWout[s:], dbout[s:]
    masks = [(z > 0).to(dtype) for z in zs]
    if mutant == "reward column dropped from dH":
        dH = (dY[:, :s] @ Wout[:s]) * masks[L - 1]
    else:
        dH = (dY @ Wout) * masks[L - 1]
    for l in range(L - 1, -1, -1):
        grads[2 * l], grads[2 * l + 1] = dH.T @ xs[l], dH.sum(0)
        if l == 0 and mutant == "db last row tile missing":
            grads[1] = dH[:TILE * ((R - 1) // TILE)].sum(0)
        if l > 0:
            m = masks[l - 1]
            if mutant == "mask of the other parity" and l == L - 1:
                m = masks[l]        # layer L - 2's dH masked with layer L - 1's signs
            dH = (dH @ P[2 * l]) * m
    if mutant == "dW_0 column K0-1 dropped":
        grads[0] = grads[0].clone()
        grads[0][:, s + a - 1] = 0
    if mutant == "dW_0 columns >= 64 dropped":
        grads[0] = grads[0].clone()
        grads[0][:, 64:] = 0
    return dict(loss=np.array([float(loss_s + loss_r), float(loss_s), float(loss_r)]),
                grads=[g.double().numpy().copy() for g in grads],
                pre=np.stack([z.double().numpy() for z in zs]))


def autograd64(params, data, rows, shape):
    """(loss, gradients) of the same loss by torch autograd in float64, written as the package's training
    loop writes it: one MSELoss per horizon step and head, summed."""
    s, a, W, L, reward, H = shape
    ps = [_t(p, torch.float64).requires_grad_(True) for p in params]
    rows = np.array(rows, np.int64)
    D = lambda k: torch.from_numpy(np.array(data[k], np.float64))  # noqa: E731
    mse = torch.nn.MSELoss()
    total = 0.0
    for hstep in range(H):
        x = torch.cat([D("states")[rows, hstep], D("actions")[rows, hstep]], dim=1)
        for l in range(L):
            x = torch.relu(x @ ps[2 * l].T + ps[2 * l + 1])
        total = total + mse(x @ ps[2 * L].T + ps[2 * L + 1], D("next_states")[rows, hstep])
        if reward:
            total = total + mse(x @ ps[2 * L + 2].T + ps[2 * L + 3], D("rewards")[rows, hstep].reshape(-1, 1))
    return float(total.detach()), [g.numpy() for g in torch.autograd.grad(total, ps)]


def err(x, g64):
    """(tensor-relative, tile-relative) error of one tensor.
    tensor-relative: max |x - g64| / max |g64| (gd_grad_reference.err's).
    tile-relative:   the largest, over the 32 x 32 tiles of the tensor (a bias is one row), of
                     max |x - g64| in the tile / max |g64| in the tile. A tile whose g64 is all zero (a unit
                     no row of the batch activates) is skipped, but x must be exactly 0 there: inf otherwise.
    A tensor whose g64 is all zero has tensor-relative error 0 if x is all zero, else inf."""
    x, g64 = np.atleast_2d(np.asarray(x, np.float64)), np.atleast_2d(np.asarray(g64, np.float64))
    assert x.shape == g64.shape, (x.shape, g64.shape)
    d = np.abs(x - g64)
    top = float(np.max(np.abs(g64)))
    whole = float(np.max(d)) / top if top > 0 else (0.0 if not np.any(x) else float("inf"))
    M, N = g64.shape
    tm, tn = -(-M // TILE), -(-N // TILE)
    pad = lambda v: np.pad(v, ((0, tm * TILE - M), (0, tn * TILE - N))).reshape(tm, TILE, tn, TILE)  # noqa: E731
    dmax, gmax, xmax = (pad(v).max(axis=(1, 3)) for v in (d, np.abs(g64), np.abs(x)))
    if np.any((gmax == 0) & (xmax != 0)):
        return whole, float("inf")
    live = gmax > 0
    tile = float(np.max(dmax[live] / gmax[live])) if live.any() else 0.0
    return whole, tile


def loss_err(x, l64):
    """|x - l64| / |l64| per entry of [total, state, reward]; an exactly zero reference (no reward head) asks
    for an exactly zero x (inf otherwise)."""
    out = []
    for xv, lv in zip(np.asarray(x, np.float64), np.asarray(l64, np.float64)):
        out.append(abs(xv - lv) / abs(lv) if lv != 0 else (0.0 if xv == 0 else float("inf")))
    return out
