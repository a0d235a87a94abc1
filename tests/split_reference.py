"""Host-side references of the split-operand rollout tests (tests/split_cases.py, test_split_host.py,
test_gpu_split_envelope.py): the float64 rollout, a NumPy emulation of the F16X3 / F16X6 arithmetic and the
error measure the bars are written in.

emulate_split restates the header comment of mujoco-mbrl_amd/csrc/rollout_f16x3.hip, not the kernel: every
Linear scales its activations by 2^4 and its weights by 2^8, splits each into P float16 pieces by exact float32
differences (x0 = f16(x), x1 = f16(x - x0), x2 = f16(x - x0 - x1)), forms the products x_i w_j with i + j < P,
adds them into one float32 accumulator in order of significance and unscales by 2^-12. Everything between the
Linears (normalisers, bias, ReLU, cost) is the float32 oracle's. `keep` names the products kept -- leaving one
out builds the kernel that forgot it.

    e(x) = max |x - x64| / max |x64|   over every recorded state of a case,

the measure of test_gpu_gd_grad.py, on states."""
import numpy as np

import rollout_cases as rc
from oracle import cem as ocem

F32 = np.float32
X_SCALE, W_SCALE = F32(16.0), F32(256.0)        # mbrl_internal.h MBRL_SPLIT_X_SCALE / _W_SCALE
SPLIT_LIMIT = 32768.0                           # |scaled operand| from here on: redone in fp32


def terms(P):
    """The kept products (i, j) = x_i w_j, in the order of their significance."""
    return tuple((i, d - i) for d in range(P) for i in range(d + 1))


def name(term):
    return "x%dw%d" % term


def split(x, P):
    """P float16 pieces of a float32 array, as float32 arrays."""
    x = np.asarray(x, F32)
    assert np.all(np.abs(x) < SPLIT_LIMIT), "operand outside the split range"
    out = []
    for _ in range(P):
        h = x.astype(np.float16).astype(F32)
        out.append(h)
        x = (x - h).astype(F32)
    return out


def split_linear(x, w, P, keep):
    """x [N, K] @ w [out, K]^T by split operands: float32."""
    xs, ws = split(x * X_SCALE, P), split(w * W_SCALE, P)
    acc = np.zeros((x.shape[0], w.shape[0]), F32)
    for i, j in terms(P):
        if (i, j) in keep:
            acc = (acc + xs[i] @ ws[j].T).astype(F32)     # f16 x f16 products are exact in float32
    return (acc * F32(1.0 / (16.0 * 256.0))).astype(F32)


def emulate_split(problem, actions, P, keep=None, s0=None):
    """(costs [E, N], states [E, H, N, s]) of oracle.cem.rollout with every Linear computed by split_linear.
    keep: the products kept, a subset of terms(P) (None: all of them)."""
    keep = set(terms(P) if keep is None else keep)
    assert keep <= set(terms(P))
    nm, cost = problem["norm"], problem["cost"]
    s0 = problem["s0"] if s0 is None else s0
    H, N, _ = actions.shape
    costs, states = [], []
    for layers in problem["model"]:
        st = np.broadcast_to(np.asarray(s0, F32), (N, np.shape(s0)[-1])).copy()
        total = np.zeros(N, F32)
        member = []
        for t in range(H):
            x = ocem.model_input(nm, st, actions[t])
            for w, b in layers[:-1]:
                x = np.maximum(split_linear(x, w, P, keep) + b, F32(0))
            w, b = layers[-1]
            st = (split_linear(x, w, P, keep) + b).astype(F32)[:, :st.shape[1]]
            if ocem.norm_flag(nm, "unnormalize_state"):
                st = (st * nm["obs_std"] + nm["obs_mean"]).astype(F32)
            total = (total + ocem.goal_state_cost(st, actions[t], cost)).astype(F32)
            member.append(st)
        costs.append(total)
        states.append(np.stack(member))
    return np.stack(costs), np.stack(states)


def rollout_f64(problem, actions, s0=None):
    """(costs [E, N], states [E, H, N, s]) in float64 from the float32 inputs (rollout_cases.rollout_f64)."""
    return rc.rollout_f64(problem, problem["s0"] if s0 is None else s0, actions, store_states=True)


def err(x, x64):
    """e(x) = max |x - x64| / max |x64|."""
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    return float(np.max(np.abs(x - x64)) / np.max(np.abs(x64)))


def ulps(x, x64):
    """The largest |x - x64| in float32 ulps of x64's binade."""
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    ulp = np.spacing(np.maximum(np.abs(x64), np.finfo(F32).tiny).astype(F32)).astype(np.float64)
    return float(np.max(np.abs(x - x64) / ulp))


def relu_margin(problem, actions, s0=None):
    """(min |z64|, max |z32 - z64|, sign changes) over every hidden pre-activation of the rollout, each
    precision along its own trajectory: gd_grad_reference.min_preact_margin's pair, and the number of
    units whose pre-activation lies on different sides of 0 in float32 and float64."""
    nm = problem["norm"]
    s0 = problem["s0"] if s0 is None else s0
    H, N, _ = actions.shape
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    on = lambda k: ocem.norm_flag(nm, k)  # noqa: E731
    lo, d, flips = np.inf, 0.0, 0
    for layers in problem["model"]:
        s32 = np.broadcast_to(np.asarray(s0, F32), (N, np.shape(s0)[-1])).copy()
        s64 = f(s32)
        for t in range(H):
            x32 = ocem.model_input(nm, s32, actions[t])
            an = (f(actions[t]) - f(nm["act_mean"])) / f(nm["act_std"]) if on("normalize_action") else f(actions[t])
            sn = (s64 - f(nm["obs_mean"])) / f(nm["obs_std"]) if on("normalize_state") else s64
            x64 = np.concatenate([sn, an], axis=1)
            for w, b in layers[:-1]:
                z32, z64 = (x32 @ w.T + b).astype(F32), x64 @ f(w).T + f(b)
                lo, d = min(lo, float(np.min(np.abs(z64)))), max(d, float(np.max(np.abs(z32 - z64))))
                flips += int(np.sum((z32 > 0) != (z64 > 0)))
                x32, x64 = np.maximum(z32, F32(0)), np.maximum(z64, 0.0)
            s32 = ocem.dynamics_step(layers, nm, s32, actions[t])
            s64 = (x64 @ f(layers[-1][0]).T + f(layers[-1][1]))[:, :s64.shape[1]]
            if on("unnormalize_state"):
                s64 = s64 * f(nm["obs_std"]) + f(nm["obs_mean"])
    return lo, d, flips
