"""NumPy fp32 restatement of the gradient-clipping order of csrc/grad_clip.hip (include/mbrl_cem.h mbrl_grad_norm,
DESIGN.md §7.5), the derived accuracy bar, the clipped Adam step, and the table of cases the host and GPU tests share.

Per member, over its gradient tensors in table order:
  - a tensor is cut into chunks of 1024 consecutive elements, the last one padded with zeros;
  - lane t of 256 forms ((g[4t]^2 + g[4t+1]^2) + g[4t+2]^2) + g[4t+3]^2, each square rounded to fp32 first, and the
    256 lane values meet in the pairwise tree v[t] += v[t + d], d = 128, .. 1;
  - the member's P chunk partials, tensor ascending and chunk ascending, are reduced as mbrl_eval_members reduces
    its loss: lane t of 1024 adds partials t, t + 1024, .. ascending, then the pairwise tree d = 512, .. 1;
  - norm = sqrt(sum) in fp32, q = max_norm / (norm + 1e-6), coef = 1 if q > 1 else q (a NaN q stays NaN).
Every operation below is a NumPy float32 operation: one IEEE rounding each, nothing contracted."""
import numpy as np
import torch

F = np.float32
CHUNK, LANES, FINISH = 1024, 256, 1024
EPS = F(1e-6)
U = 2.0 ** -24          # fp32 unit roundoff


def _tree(v, width):
    """v[..., t] += v[..., t + d] for d = width / 2, .. 1 (in place): the sum in v[..., 0]."""
    d = width // 2
    while d >= 1:
        v[..., :d] += v[..., d:2 * d]
        d //= 2
    return v[..., 0]


def chunk_partials(g, pad=0.0):
    """The partial of each 1024-element chunk of one tensor ([] for an empty one). pad: what the padding of the last
    chunk holds -- zeros in the real order; the tests' mutant passes something else."""
    g = np.asarray(g, F).reshape(-1)
    if g.size == 0:
        return np.zeros(0, F)
    n = -(-g.size // CHUNK)
    x = np.full(n * CHUNK, pad, F)
    x[:g.size] = g
    x = x.reshape(n, LANES, 4)
    with np.errstate(all="ignore"):
        sq = x * x
        v = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
        return _tree(v, LANES).copy()


def reduce_partials(p):
    lanes = np.zeros(FINISH, F)
    with np.errstate(all="ignore"):
        for k in range(0, p.size, FINISH):
            part = p[k:k + FINISH]
            lanes[:part.size] += part
        return F(_tree(lanes, FINISH))


def member_partials(grads):
    return np.concatenate([chunk_partials(g) for g in grads] + [np.zeros(0, F)])


def sumsq(grads):
    return reduce_partials(member_partials(grads))


def norm(grads):
    with np.errstate(all="ignore"):
        return F(np.sqrt(sumsq(grads)))


def coef(nrm, max_norm, eps=EPS):
    with np.errstate(all="ignore"):
        q = F(max_norm) / (F(nrm) + eps)
    return F(1.0) if q > 1 else F(q)


def scaled(grads, c):
    """What Adam consumes: g * coef, one rounded fp32 product per element."""
    with np.errstate(all="ignore"):
        return [np.asarray(g, F) * F(c) for g in grads]


def norm_bar(numels):
    """The relative bar on the norm, from the order alone. All terms are non-negative, so the relative error of the
    sum is at most (longest chain of dependent additions + 1) * 2^-24 -- the + 1 is the square's own rounding: 3
    additions in a lane, 8 tree levels in a chunk, ceil(P / 1024) - 1 additions in a finishing lane, 10 tree levels
    there. The square root halves that and adds one rounding."""
    P = sum(-(-n // CHUNK) for n in numels)
    chain = 3 + 8 + max(-(-P // FINISH) - 1, 0) + 10
    return 0.5 * (chain + 1) * U + U


def norm64(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads)))


def adam_step(params, grads, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam's CPU step number `step` (1-based) on these gradients -- the arithmetic mbrl_adam_step holds
    bit for bit (tests/test_gpu_train_adam.py). Returns the new (params, exp_avg, exp_avg_sq) as NumPy arrays."""
    ps = [torch.from_numpy(np.array(p, F)).requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=True)
    for p, g, mm, vv in zip(ps, grads, m, v):
        p.grad = torch.from_numpy(np.array(g, F))
        opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(np.array(mm, F)),
                            exp_avg_sq=torch.from_numpy(np.array(vv, F)))
    opt.step()
    return ([p.detach().numpy() for p in ps], [opt.state[p]["exp_avg"].numpy() for p in ps],
            [opt.state[p]["exp_avg_sq"].numpy() for p in ps])


def clipped_step(params, grads, m, v, step, max_norm, **kw):
    """One member's clipped step: (norm, coef, (params, exp_avg, exp_avg_sq))."""
    nrm = norm(grads)
    c = coef(nrm, max_norm)
    return nrm, c, adam_step(params, scaled(grads, c), m, v, step, **kw)


# ---- the cases: per member a list of numels, a scale and what to plant; one max_norm per case
BIG = 1024 * 1024
CASES = {
    # every numel seam in one member, beside a small one whose norm stays within max_norm
    "seams": dict(members=[[0, 1, 3, 1023, 1024, 1025, 4099], [3, 1025]], scales=[1.0, 1e-3], max_norm=2.0),
    "e1": dict(members=[[4099, 17]], scales=[1.0], max_norm=0.5),
    "e5": dict(members=[[1025, 3, 64]] * 5, scales=[1e-2, 1.0, 30.0, 1e-3, 5.0], max_norm=3.0),
    # a small norm: eps = 1e-6 is a visible part of norm + eps
    "tiny": dict(members=[[1023, 5], [1024]], scales=[1e-6, 3e-6], max_norm=1e-5),
    "zero": dict(members=[[1025, 3], [7]], scales=[0.0, 1.0], max_norm=1.0),
    "inf_norm": dict(members=[[1025, 3], [7]], scales=[10.0, 100.0], max_norm=float("inf")),
    # E * count on both sides of the 64-tensor table limit
    "e8_c8": dict(members=[[33, 1, 1025, 0, 7, 1024, 3, 2049]] * 8, scales=[2.0 ** (e - 4) for e in range(8)],
                  max_norm=20.0),
    "e8_c10": dict(members=[[33, 1, 1025, 0, 7, 1024, 3, 2049, 5, 1023]] * 8, scales=[2.0 ** (e - 4) for e in range(8)],
                   max_norm=20.0),
    # P on both sides of 1024: one 1024 x 1024 tensor (1024 chunks) and small ones, beside small members
    "p1024": dict(members=[[3, 1025], [BIG, 0], [17]], scales=[1.0, 1e-2, 1.0], max_norm=5.0),
    "p1025": dict(members=[[3, 1025], [BIG, 3], [17]], scales=[1.0, 1e-2, 1.0], max_norm=5.0),
    # non-finite members beside finite ones
    "nan": dict(members=[[1025, 3], [1025, 3], [64]], scales=[1.0, 1.0, 1.0], max_norm=1.0, plant={1: float("nan")}),
    "inf": dict(members=[[1025, 3], [1025, 3], [64]], scales=[1.0, 1.0, 1.0], max_norm=1.0, plant={0: float("inf")}),
}
NAMES = list(CASES)


def gradients(name):
    """The case's gradients: [member][tensor] fp32 arrays, seeded by the name; a planted value goes to element 2 of
    the member's last non-empty tensor."""
    c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    out = []
    for e, (numels, scale) in enumerate(zip(c["members"], c["scales"])):
        gs = [(rng.standard_normal(n) * scale).astype(F) for n in numels]
        if e in c.get("plant", {}):
            [g for g in gs if g.size > 2][-1][2] = c["plant"][e]
        out.append(gs)
    return out
