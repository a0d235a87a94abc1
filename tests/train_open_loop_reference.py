"""The gradient mbrl_train_grads_open_loop computes, restated on the CPU in torch. No GPU import.

Per member, over the batch's transitions i = rows[b], b < B, with x_0 = states[i][0], for h = 0 .. H - 1:

    (s^_{h+1}, r^_h) = the member's forward pass on (x_h, actions[i][h])
    x_{h+1}          = s^_{h+1}                    fed back as it is: not detached, clamped or renormalised
    loss = sum_h [ sum (s^_{h+1} - next_states[i][h])^2 / (B s)  +  sum (r^_h - rewards[i][h])^2 / B ]

autograd64 unrolls that on the package's Model / ModelWithReward linears and takes torch autograd in float64.
loss_and_grads writes the backward pass out step by step (backpropagation through time; the host test holds
it to autograd64), so that a mutant can put exactly one thing wrong while every forward value stays the same;
dtype = float32 is the same chain in float32 on the CPU, whose distance to float64 sets every bar."""
import numpy as np
import torch

TILE_ROWS = 16     # rows of the batch per workgroup of the kernels

# label -> what is wrong
MUTANTS = {
    "detached feedback": "carry = 0: the fed-back state is treated as data (teacher forcing in disguise)",
    "carry on the reward column": "the carry's first column is also added to the reward column of g_out",
    "carry from the action columns": "the carry is the last s columns of delta_0 W_0 instead of the first s",
    "dW_0 from the true states": "dW_0 is built from the dataset's states[i][h] instead of the fed-back x_h",
    "mask of step h + 1": "delta_0 of step h is masked with step h + 1's layer-0 activations",
    "no carry in rows 8-15": "rows 8 .. 15 of every 16-row tile of the batch get no carry",
}


def applicable(shape, B):
    s, a, W, L, reward, H = shape
    if H < 2:
        return []
    out = ["detached feedback", "dW_0 from the true states", "mask of step h + 1"]
    if reward:
        out.append("carry on the reward column")
    if a >= 1:
        out.append("carry from the action columns")
    if B > 8:
        out.append("no carry in rows 8-15")
    return out


def _t(x, dtype):
    return torch.from_numpy(np.array(x, np.float32)).to(dtype)


def model_of(params, shape, dtype=torch.float64):
    """The package's Model / ModelWithReward with these parameters, in `dtype`."""
    from mbrl_amd.models import Model, ModelWithReward
    s, a, W, L, reward, H = shape
    m = ModelWithReward(s, a, hidden_units=W, n_hidden=L) if reward else Model(s, a, hidden_units=W, n_hidden=L)
    m = m.to(dtype)
    with torch.no_grad():
        for i, lin in enumerate(m.linears()):
            lin.weight.copy_(_t(params[2 * i], dtype))
            lin.bias.copy_(_t(params[2 * i + 1], dtype))
    return m


def autograd64(params, data, rows, shape):
    """(loss [total, state, reward], gradients in params' order, predictions [B][H][s]) by autograd in float64
    through the package's linears."""
    s, a, W, L, reward, H = shape
    m = model_of(params, shape)
    lins = m.linears()
    rows = np.array(rows, np.int64)
    D = lambda k: torch.from_numpy(np.array(data[k], np.float64))  # noqa: E731
    mse = torch.nn.MSELoss()
    x = D("states")[rows, 0]
    ls, lr, preds = 0.0, torch.zeros((), dtype=torch.float64), []
    for h in range(H):
        z = torch.cat([x, D("actions")[rows, h]], dim=1)
        for lin in lins[:L]:
            z = torch.relu(lin(z))
        x = lins[L](z)
        preds.append(x)
        ls = ls + mse(x, D("next_states")[rows, h])
        if reward:
            lr = lr + mse(lins[L + 1](z), D("rewards")[rows, h].reshape(-1, 1))
    total = ls + lr
    ps = [t for lin in lins for t in (lin.weight, lin.bias)]
    grads = torch.autograd.grad(total, ps)
    return (np.array([float(total.detach()), float(ls.detach()), float(lr.detach())]), [g.numpy() for g in grads],
            torch.stack(preds, dim=1).detach().numpy())


def loss_and_grads(params, data, rows, shape, dtype, mutant=None):
    """dict(loss [3], grads, pred [B][H][s], row_err [B][H], pre [H][L][B][W]) as float64 NumPy, every
    operation carried out in `dtype`; the backward pass written out."""
    assert mutant is None or mutant in MUTANTS, mutant
    s, a, W, L, reward, H = shape
    rows = np.array(rows, np.int64)
    B = len(rows)
    P = [_t(p, dtype) for p in params]
    assert len(P) == 2 * (L + 1 + reward)
    St, Ac, Ns, Rw = (_t(data[k][rows], dtype) for k in ("states", "actions", "next_states", "rewards"))
    Wcat = torch.cat([P[2 * L], P[2 * L + 2]], dim=0) if reward else P[2 * L]
    bcat = torch.cat([P[2 * L + 1], P[2 * L + 3]], dim=0) if reward else P[2 * L + 1]
    x = St[:, 0]
    X0, acts, pre, dYs, preds, row_err = [], [], [], [], [], []
    loss_s, loss_r = torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype)
    for h in range(H):
        cur = torch.cat([x, Ac[:, h]], dim=1)
        X0.append(cur)
        hs, zs = [], []
        for l in range(L):
            z = cur @ P[2 * l].T + P[2 * l + 1]
            cur = torch.relu(z)
            zs.append(z)
            hs.append(cur)
        y = cur @ Wcat.T + bcat
        ds = y[:, :s] - Ns[:, h]
        loss_s = loss_s + torch.sum(ds * ds) / (B * s)
        dY = ds * (2.0 / (B * s))
        if reward:
            dr = y[:, s] - Rw[:, h]
            loss_r = loss_r + torch.sum(dr * dr) / B
            dY = torch.cat([dY, (dr * (2.0 / B)).reshape(B, 1)], dim=1)
        acts.append(hs)
        pre.append(torch.stack(zs))
        dYs.append(dY)
        row_err.append(torch.sum(ds * ds, dim=1))
        x = y[:, :s]
        preds.append(x)
    grads = [torch.zeros_like(p) for p in P]
    carry = torch.zeros((B, s), dtype=dtype)
    no_carry = (torch.arange(B) % TILE_ROWS >= 8).reshape(B, 1)
    for h in range(H - 1, -1, -1):
        g = dYs[h].clone()
        if mutant == "no carry in rows 8-15":
            carry = torch.where(no_carry, torch.zeros_like(carry), carry)
        g[:, :s] += carry
        if mutant == "carry on the reward column" and reward:
            g[:, s] += carry[:, 0]
        top = acts[h][L - 1]
        dWo, dbo = g.T @ top, g.sum(0)
        grads[2 * L] += dWo[:s]
        grads[2 * L + 1] += dbo[:s]
        if reward:
            grads[2 * L + 2] += dWo[s:]
            grads[2 * L + 3] += dbo[s:]
        other = mutant == "mask of step h + 1" and h + 1 < H
        d = (g @ Wcat) * ((acts[h + 1][0] if other and L == 1 else top) > 0).to(dtype)
        for l in range(L - 1, 0, -1):
            grads[2 * l] += d.T @ acts[h][l - 1]
            grads[2 * l + 1] += d.sum(0)
            d = (d @ P[2 * l]) * ((acts[h + 1][0] if other and l == 1 else acts[h][l - 1]) > 0).to(dtype)
        x0 = X0[h]
        if mutant == "dW_0 from the true states":
            x0 = torch.cat([St[:, h], Ac[:, h]], dim=1)
        grads[0] += d.T @ x0
        grads[1] += d.sum(0)
        back = d @ P[0]
        carry = back[:, s + a - s:] if mutant == "carry from the action columns" else back[:, :s]
        if mutant == "detached feedback":
            carry = torch.zeros_like(carry)
    return dict(loss=np.array([float(loss_s + loss_r), float(loss_s), float(loss_r)]),
                grads=[g.double().numpy().copy() for g in grads],
                pred=torch.stack(preds, dim=1).double().numpy(),
                row_err=torch.stack(row_err, dim=1).double().numpy(),
                pre=torch.stack(pre).double().numpy())
