"""The case table of the selection-branch tests (test_select_model.py on the CPU, test_gpu_select_branches.py
on the GPU): inputs built so that select_branch_model's predictions do not depend on a random draw
landing well.

Keys are built in exact integer ulps. Positive float32 bits are monotone in the key, so
r = (int32(0x42F00000) + u).view(float32) for integer offsets u >= 0 gives keys whose differences are
exactly u (u < 2**27 keeps every value finite and positive). Rows with E = 5 members use five equal
copies of r with u a multiple of 8: r then has three spare mantissa bits, 2r .. 5r are exact and the
member mean is r again.

Every constructor is deterministic from its seed. A row keeps its returns r [N]; costs() gives [E, N]."""
import collections
import functools
import zlib

import numpy as np

import select_branch_model as sbm

BASE = 0x42F00000                      # 120.0f
T = 7                                  # copies of the K-th value in the tie rows
SHAPES = {1: (1, 63, 65, 1000, 1024), 2: (1025, 2047, 2048), 4: (2052, 4094, 4096),
          8: (4097, 4100, 8190, 8192), 16: (8196, 16381, 16384), 32: (16388, 32765, 32768)}
FAMILIES = ("flat", "wide_only", "rank64", "list_radix", "all_radix", "nan_kth", "odd", "nan_first")

Row = collections.namedtuple("Row", "id family kpt N E K nan_policy r")
Row.costs = lambda self: np.tile(self.r, (self.E, 1))


def ulp(u, step=1):
    u = np.asarray(u, dtype=np.int64) * step
    assert u.min() >= 0 and u.max() < 2 ** 27
    return (np.int32(BASE) + u.astype(np.int32)).view(np.float32)


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _shuffle_with_ends(rng, vals, flag=None):
    """vals in random order, with vals[0] and vals[1] (the range's two ends) at candidates 3 and 5, where
    the tie rows do not write."""
    order = rng.permutation(vals.size)
    for src, dst in ((0, 3), (1, 5)):
        j = int(np.nonzero(order == src)[0][0])
        order[j], order[dst] = order[dst], order[j]
    return (vals[order], None) if flag is None else (vals[order], flag[order])


def tie_positions(N, kpt):
    """Candidate 0, candidate N - 1, both sides of a wave boundary (64 KPT w - 1, 64 KPT w + 1, and the
    boundary itself), and two keys of one lane's float4 group (8 and 10)."""
    w = (N - 2) // (64 * kpt)
    b = 64 * kpt * w if w >= 1 else N // 2
    pos = [0, N - 1, b - 1, b, b + 1, 8, 10]
    assert len(set(pos)) == T and not {3, 5} & set(pos) and max(pos) < N
    return np.array(pos)


def _with_ties(u, v, N, kpt):
    """T copies of v placed; K to take all keys equal to v, and K to cut after the third."""
    u = u.copy()
    u[tie_positions(N, kpt)] = v
    below, equal = int((u < v).sum()), int((u == v).sum())
    assert equal >= T
    return u, below + equal, below + 3


def spread(rng, N, bits=24):
    """Offsets uniform over [0, 2**bits), both ends present."""
    vals = rng.integers(0, 1 << bits, N)
    vals[0], vals[1] = 0, (1 << bits) - 1
    return _shuffle_with_ends(rng, vals)[0]


def bucketed(rng, N, C, s, equal=False, B=200):
    """rem = 11 + s and a bucket width of 2**s (ends at 0 and 2**(11+s) - 1); C keys inside bucket B,
    uniform over it (or all equal), the rest spread over the other buckets. Returns the offsets and
    the cluster's flags."""
    nb = N - C
    assert nb >= 2 and N >= 6
    bins = rng.integers(0, 2047, nb)
    bins += bins >= B
    bg = (bins << s) + rng.integers(0, 1 << s, nb)
    bg[0], bg[1] = 0, (1 << (11 + s)) - 1
    low = np.full(C, rng.integers(0, 1 << s)) if equal else rng.integers(0, 1 << s, C)
    vals = np.concatenate([bg, (B << s) + low])
    return _shuffle_with_ends(rng, vals, np.arange(N) >= nb)


def _cluster_rows(u, cl, N, kpt, ties):
    """(tag, offsets, K): the K-th key an eighth of the way into the cluster; with ties, T copies of it."""
    c = np.sort(u[cl])
    v = int(c[c.size // 8])
    out = [("", u, int((u < c[0]).sum()) + max(1, c.size // 8))]
    if ties:
        ut, k_all, k_cut = _with_ties(u, v, N, kpt)
        out += [("-ties_all", ut, k_all), ("-ties_cut", ut, k_cut)]
    return out


def _family_rows(family, N, kpt, step):
    """(tag, returns, K, nan_policy) of one family at one N; step = 8 for the E = 5 rows."""
    NL = sbm.NAN_LAST
    rows = []
    if family == "flat":
        r = np.full(N, 3.5, dtype=np.float32)
        rows.append(("equal-all", r, N, NL))
        if N >= 8:
            rows.append(("equal-cut", r, N // 8, NL))
            z = np.where(_rng(family, N).random(N) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            rows += [("zeros-all", z, N, NL), ("zeros-cut", z, N // 8 + 1, NL)]
    elif family == "wide_only" and N >= 63:
        for m in (3, 11):
            u = spread(_rng(family, N, m), N, m)
            v = np.sort(u)[N // 10]
            k_all = int((u <= v).sum())
            rows.append(("m%d-all" % m, ulp(u, step), k_all, NL))
            if int((u == v).sum()) >= 2:
                rows.append(("m%d-cut" % m, ulp(u, step), k_all - 1, NL))
    elif family == "rank64" and N >= 63:
        u = spread(_rng(family, N), N)
        rows.append(("spread", ulp(u, step), N // 10 + 1, NL))
        ut, k_all, k_cut = _with_ties(u, int(np.sort(u)[N // 10]), N, kpt)
        rows += [("ties_all", ulp(ut, step), k_all, NL), ("ties_cut", ulp(ut, step), k_cut, NL)]
    elif family == "list_radix":
        for C in (100, 1500):
            for s in (5, 8, 13):
                if N < C + 16:
                    continue
                u, cl = bucketed(_rng(family, N, C, s), N, C, s)
                ties = (C, s) in ((100, 13), (1500, 5))
                rows += [("C%d-s%d%s" % (C, s, tag), ulp(uu, step), K, NL)
                         for tag, uu, K in _cluster_rows(u, cl, N, kpt, ties)]
        if N >= 116:
            u, cl = bucketed(_rng(family, N, "equal"), N, 100, 13, equal=True)
            rows.append(("C100-s13-equal", ulp(u, step), int((u < u[cl][0]).sum()) + 12, NL))
    elif family == "all_radix" and N - 8 > sbm.SEL_LIST:
        C = N - 8
        for s in (8, 13):
            u, cl = bucketed(_rng(family, N, s), N, C, s)
            rows += [("s%d-mixed%s" % (s, tag), ulp(uu, step), K, NL)
                     for tag, uu, K in _cluster_rows(u, cl, N, kpt, s == 13)]
        u, cl = bucketed(_rng(family, N, "equal"), N, C, 13, equal=True)
        below = int((u < u[cl][0]).sum())
        rows += [("s13-equal-cut", ulp(u, step), below + C // 8, NL), ("s13-equal-all", ulp(u, step), below + C, NL)]
    elif family == "nan_kth" and N >= 63:
        rng = _rng(family, N)
        base = ulp(spread(rng, N), step)
        for tag, cnt in (("tenth", max(4, N // 10)), ("heavy", N - N // 10)):
            r = base.copy()
            r[rng.choice(N, cnt, replace=False)] = np.nan
            if tag == "tenth":
                rows += [("tenth-cut", r, N - 3, NL), ("tenth-all", r, N, NL)]
            else:
                rows.append(("heavy-cut", r, N - cnt + 5, NL))
    elif family == "odd" and N >= 63 and step == 1:
        rng = _rng(family, N)
        r = (rng.standard_normal(N) * 100).astype(np.float32)
        r[rng.choice(N, 6, replace=False)] = np.repeat(np.float32([-np.inf, np.inf]), 3)
        rows += [("inf-low", r, 2, NL), ("inf-mid", r, N // 10 + 1, NL), ("inf-high", r, N - 1, NL)]
        # float32 subnormals of both signs (|bits| < 2**23), with -0.0 and +0.0 among them
        b = rng.integers(1, 1 << 23, N).astype(np.uint32) | (rng.integers(0, 2, N).astype(np.uint32) << 31)
        b[rng.choice(N, N // 8, replace=False)] &= np.uint32(0x80000000)
        r = b.view(np.float32)
        neg = int((r < 0).sum())
        rows += [("subnormal-zero", r, neg + 2, NL), ("subnormal-pos", r, neg + N // 8 + N // 16, NL),
                 ("subnormal-neg", r, max(1, neg // 2), NL)]
        r = rng.standard_normal(N).astype(np.float32)
        r[rng.choice(N, 5, replace=False)] = np.float32([0.0, -0.0, 0.0, -0.0, 0.0])
        rows.append(("mixed-sign", r, int((r < 0).sum()) + 3, NL))
    elif family == "nan_first" and N >= 63:
        rng = _rng(family, N)
        r = rng.standard_normal(N).astype(np.float32)
        r[rng.choice(N, max(2, N // 10), replace=False)] = np.nan
        rows.append(("argmin", r, 1, sbm.NAN_FIRST))
    return rows


# the rows that also run with E = 5 members (offsets scaled by 8): the member-sum load in each layout
E5_TAGS = {"flat": ("equal-cut",), "rank64": ("spread", "ties_cut"), "list_radix": ("C100-s8",),
           "all_radix": ("s13-mixed",), "nan_kth": ("tenth-cut", "heavy-cut"), "wide_only": ("m11-all",)}


@functools.lru_cache(maxsize=None)
def rows(kpt=None, family=None):
    """The table, or its rows of one (KPT, family). Only feasible rows are listed (all_radix needs a
    bucket above SEL_LIST, list_radix room for its cluster, a single candidate can only be flat)."""
    if kpt is None:
        return tuple(r for k in SHAPES for f in FAMILIES for r in rows(k, f))
    out = []
    for N in SHAPES[kpt]:
        for E, step in ((1, 1), (5, 8)):
            for tag, r, K, pol in _family_rows(family, N, kpt, step):
                if E == 5 and tag not in E5_TAGS.get(family, ()):
                    continue
                rid = "%s-%s-N%d-E%d-K%d" % (family, tag, N, E, K)
                out.append(Row(rid, family, kpt, N, E, int(K), pol, np.ascontiguousarray(r, dtype=np.float32)))
    return tuple(out)


def groups():
    """(KPT, family) pairs that have rows: the GPU test's ids."""
    return [(k, f) for k in SHAPES for f in FAMILIES if rows(k, f)]
