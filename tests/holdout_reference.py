"""What mbrl_eval_members computes and the rule EnsembleModel.fit_members follows, restated on the CPU. No
GPU import.

    X      = [states[rows], actions[rows]]          [R H][s + a], row r H + h = transition rows[r], step h
    x_{l+1} = relu(x_l W_l^T + b_l)                  l = 0 .. L - 1
    Y      = x_L [W_out; w_rew]^T + [b_out; b_rew]
    row_err[r][h]     = sum_j (Y_j - next_states[rows[r]][h][j])^2
    row_rew_err[r][h] = (y_rew - rewards[rows[r]][h])^2
    loss   = (state + reward, state, reward),  state = sum_h (sum_r row_err[r][h]) / (R s),
                                               reward = sum_h (sum_r row_rew_err[r][h]) / R

dtype = float64 is the reference; dtype = float32 is the same chain in plain torch CPU float32, whose
distance to float64 sets every bar (tests/train_grad_cases.py's construction). tests/test_holdout_host.py
holds evaluate() to the package's own modules in float64.

rule() is the keep-best and early-stop rule on a table of held-out losses, in NumPy."""
import numpy as np
import torch

import train_grad_reference as tref


def evaluate(params, data, rows, shape, dtype):
    """params: [W_0, b_0, ..., W_out, b_out(, w_rew, b_rew)] float32 arrays of one member; data: the stacked
    transitions (train_grad_reference.batch's); rows: dataset rows (repeats allowed). Returns
    dict(row_err [R][H], row_rew_err [R][H] or None, loss [3]) as float64 NumPy, every operation in `dtype`."""
    s, a, W, L, reward, H = shape
    R = len(rows)
    P = [torch.from_numpy(np.array(p, np.float32)).to(dtype) for p in params]
    assert len(P) == 2 * (L + 1 + reward)
    x, Ts, Tr = tref.batch(data, rows, shape, dtype)
    for l in range(L):
        x = torch.relu(x @ P[2 * l].T + P[2 * l + 1])
    d = x @ P[2 * L].T + P[2 * L + 1] - Ts
    row_err = (d * d).sum(1).reshape(R, H)
    state = sum(row_err[:, h].sum() / (R * s) for h in range(H))
    row_rew, rew = None, torch.zeros((), dtype=dtype)
    if reward:
        dr = (x @ P[2 * L + 2].T + P[2 * L + 3]).reshape(R * H) - Tr
        row_rew = (dr * dr).reshape(R, H)
        rew = sum(row_rew[:, h].sum() / R for h in range(H))
    return dict(row_err=row_err.double().numpy().copy(),
                row_rew_err=None if row_rew is None else row_rew.double().numpy().copy(),
                loss=np.array([float(state + rew), float(state), float(rew)]))


def rule(val_loss, patience=None, check_every=1):
    """val_loss [epochs][E]: the members' held-out losses after each epoch of a run that never stops early.
    Per member, epoch k is a new best when its loss is below the best so far (start: +inf; a NaN is never
    better), else the member's stale count grows by one. With a patience, after each epoch k with
    (k + 1) % check_every == 0 the run stops when every member's stale count is >= patience.
    Returns dict(best_loss [E] float32, best_epoch [E] (-1: never), stale [E], epochs_run)."""
    val = np.asarray(val_loss, np.float32)
    E = val.shape[1]
    best = np.full(E, np.inf, np.float32)
    at = np.full(E, -1, np.int64)
    stale = np.zeros(E, np.int64)
    ran = 0
    for k in range(val.shape[0]):
        for e in range(E):
            if val[k, e] < best[e]:
                best[e], at[e], stale[e] = val[k, e], k, 0
            else:
                stale[e] += 1
        ran = k + 1
        if patience is not None and (k + 1) % check_every == 0 and stale.min() >= patience:
            break
    return dict(best_loss=best, best_epoch=at, stale=stale, epochs_run=ran)
