"""What mbrl_eval_members_open_loop computes, restated on the CPU at a chosen dtype. No GPU import.

    x_0       = states[rows[r]][0]
    (s^, r^)  = tests/holdout_reference.py's forward pass on [x_h, actions[rows[r]][h]]     h = 0 .. H - 1
    x_{h+1}   = s^                                  (the state head's values, fed back as they are)
    row_err[r][h]     = sum_j (s^_j - next_states[rows[r]][h][j])^2
    row_rew_err[r][h] = (r^ - rewards[rows[r]][h])^2
    pred[r][h]        = s^
    loss              = holdout_reference's: (state + reward, state, reward) over these row errors

states[.][h] for h >= 1 is never read. At horizon 1 this is holdout_reference.evaluate (tests/test_open_loop_host.py
holds the two equal, and this one to the package's Model / ModelWithReward._forward in float64).

mutant: one single mistake of the step seam, for tests/test_open_loop_host.py to show that the bars see it:
    "teacher"      x_h = the dataset's states[rows[r]][h] at h >= 1 (teacher forcing: what mbrl_eval_members does)
    "stale"        at h >= 1 the input columns s + reward .. s + a - 1 keep what the kernel's buffer held instead of
                   step h's actions: zeros up to the output layer's last 16-column block, beyond it the hidden
                   activations of layer L - 2 (at L = 1: the previous input), which shared that buffer
    "reward_col"   at h >= 1 input column s holds r^_{h-1} (the reward head's output lies there after the output
                   layer) instead of the first action. At a = 0 column s meets no weight of layer 0 -- the
                   kernel's layer masks k >= s + a -- so there the mistake changes nothing finite; on the GPU a
                   non-finite r^ would (0 x inf), and tests/test_gpu_open_loop.py has that case.
    "prev_action"  step h >= 1 uses actions[rows[r]][h - 1]
    "prev_target"  step h >= 1 takes its errors against next_states / rewards of step h - 1
    "half_tile"    rows r with r % 16 >= 8 (the second half of a 16-row tile) are teacher forced"""
import numpy as np
import torch

MUTANTS = ("teacher", "stale", "reward_col", "prev_action", "prev_target", "half_tile")


def _t(x, dtype):
    return torch.from_numpy(np.array(x, np.float32)).to(dtype)


def applies(mutant, shape, R):
    """Whether the mistake can change a result of a case of this shape at all."""
    s, a, W, L, reward, H = shape
    if H < 2:
        return False
    if mutant == "stale":
        return a > reward
    if mutant == "reward_col":
        return bool(reward) and a >= 1
    if mutant == "prev_action":
        return a >= 1
    if mutant == "half_tile":
        return R > 8
    return True


def evaluate(params, data, rows, shape, dtype, mutant=None):
    """params, data, rows, shape as holdout_reference.evaluate's. Returns dict(row_err [R][H], row_rew_err [R][H]
    or None, pred [R][H][s], loss [3]) as float64 NumPy and preacts: per step the hidden layers' pre-activations
    [H][L][R][W]; every operation in `dtype`."""
    s, a, W, L, reward, H = shape
    rows = np.asarray(rows, np.int64)
    R = len(rows)
    P = [_t(p, dtype) for p in params]
    assert len(P) == 2 * (L + 1 + reward)
    S, A, NS, RW = (_t(data[k][rows], dtype) for k in ("states", "actions", "next_states", "rewards"))
    second_half = torch.from_numpy((np.arange(R) % 16) >= 8)
    x = S[:, 0]
    errs, rews, preds, pre = [], [], [], []
    stale = rew_prev = None
    for h in range(H):
        act = A[:, h - 1] if (mutant == "prev_action" and h >= 1) else A[:, h]
        if h >= 1 and mutant == "stale":
            act = act.clone()
            first_kept = -(-(s + reward) // 16) * 16
            for k in range(s + reward, s + a):
                act[:, k - s] = stale[:, k] if (k >= first_kept and k < stale.shape[1]) else 0
        if h >= 1 and mutant == "reward_col":
            act = act.clone()
            act[:, 0] = rew_prev
        inp = torch.cat([x, act], dim=1)
        hidden, z_all = [inp], []
        y = inp
        for l in range(L):
            z = y @ P[2 * l].T + P[2 * l + 1]
            z_all.append(z.double().numpy())
            y = torch.relu(z)
            hidden.append(y)
        pre.append(np.stack(z_all))
        out = y @ P[2 * L].T + P[2 * L + 1]
        t = h - 1 if (mutant == "prev_target" and h >= 1) else h
        d = out - NS[:, t]
        errs.append((d * d).sum(1))
        if reward:
            r_hat = (y @ P[2 * L + 2].T + P[2 * L + 3]).reshape(R)
            dr = r_hat - RW[:, t]
            rews.append(dr * dr)
            rew_prev = r_hat
        preds.append(out)
        stale = hidden[L - 1]               # what the output buffer held before the output layer wrote it
        x = out
        if h + 1 < H:
            if mutant == "teacher":
                x = S[:, h + 1]
            elif mutant == "half_tile":
                x = torch.where(second_half[:, None], S[:, h + 1], out)
    row_err = torch.stack(errs, dim=1)
    state = sum(row_err[:, h].sum() / (R * s) for h in range(H))
    row_rew, rew = None, torch.zeros((), dtype=dtype)
    if reward:
        row_rew = torch.stack(rews, dim=1)
        rew = sum(row_rew[:, h].sum() / R for h in range(H))
    return dict(row_err=row_err.double().numpy().copy(),
                row_rew_err=None if row_rew is None else row_rew.double().numpy().copy(),
                pred=torch.stack(preds, dim=1).double().numpy().copy(),
                loss=np.array([float(state + rew), float(state), float(rew)]),
                preacts=np.stack(pre))
