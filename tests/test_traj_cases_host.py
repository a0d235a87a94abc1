"""CPU checks of the single-trajectory case table (tests/traj_cases.py) and of the dispatch model it leans
on (rollout_dispatch_model.trajectory_instance): every case lands on the instance it was built for, the table
reaches all 20 traj_reg_kernel and all 8 traj_coop_kernel instances, both cooperative grids and the four
MBRL_OPT_TRAJ_HOP values, each dispatch threshold is met from both sides, the thresholds the model copies are
the ones in the sources, and the float32 oracle stays within traj_cases-wide distance D of the same rollout
in float64 -- the D from which tests/test_gpu_traj_envelope.py takes its tight bar.
No GPU: the table is run on one by tests/test_gpu_traj_envelope.py."""
import os
import re

import numpy as np

import rollout_dispatch_model as rdm
import traj_cases as tc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mujoco-mbrl_amd", "csrc")


def _shape(c):
    sh = c.shape
    return sh["s"], sh["a"], sh["W"], sh["L"], sh["E"]


def test_every_case_lands_where_it_was_built_to():
    ids = [c.id for c in tc.CASES]
    assert len(set(ids)) == len(ids)
    for c in tc.CASES:
        assert tc.instance(c) == c.want, (c.id, tc.instance(c), c.want)
        s, a, W, L, E = _shape(c)
        assert rdm.trajectory_kernel(s, a, W, L, E, H=c.H) == \
            rdm.trajectory_instance(s, a, W, L, E, H=c.H).kernel                   # the old spelling agrees
        assert c.hops in ((0,), tc.HOPS) and (c.want.kernel == "coop" or c.hops == (0,)), c.id
        # small unless the case is about E or H
        assert E <= 3 or "E = %d" % E in c.about or "P E" in c.about, c.id
        assert c.H <= 6 or c.id.startswith("line"), c.id
    for sh, H, want in tc.HOST_ONLY:
        assert rdm.trajectory_instance(sh["s"], sh["a"], sh["W"], sh["L"], sh["E"], H=H) == want, sh


def test_table_reaches_every_instance_grid_and_hop_option():
    reg = {(i.WP, i.NHL, i.K0R) for i in map(tc.instance, tc.REG)}
    assert reg == rdm.REG_INSTANCES and len(reg) == 20
    coop = {(i.K0R, i.SM, i.WI) for i in map(tc.instance, tc.COOP)}
    assert coop == rdm.COOP_INSTANCES and len(coop) == 8
    assert all(tc.instance(c).kernel == "coop" for c in tc.COOP) and all(tc.instance(c).kernel == "reg" for c in tc.REG)
    # launch_traj_reg / launch_traj_coop list exactly these
    with open(os.path.join(CSRC, "traj.hip")) as f:
        traj = f.read()
    widths = {int(w): int(wi) for w, wi in re.findall(r"case (\d+): return launch_coop_variant<K0R, SM, (\d+)>", traj)}
    assert widths == {64: 2, 128: 4, 256: 8, 512: 16}
    budgets = re.findall(r"launch_coop_width<(\d+), (\d+)>\(A, E, xchg, status, stream\)", traj)
    assert {(int(k), int(m), wi) for k, m in budgets for wi in widths.values()} == rdm.COOP_INSTANCES
    assert sorted(int(w) for w in re.findall(r"case (\d+): return launch_reg_w<\1>", traj)) == [64, 128, 256]
    assert len(re.findall(r"case [0-3]: (?:if constexpr \(WP <= 128\) )?return launch_reg_k0<WP, [0-3]>", traj)) == 4
    assert len(re.findall(r"if constexpr \(WP <= 128\) return launch_reg_k0<WP, [23]>", traj)) == 2
    # hop options: every cooperative grid / hop_mode the options can produce, at both register budgets
    seen = {(i.K0R, i.grid, i.hop) for c in tc.HOP_CASES for i in (tc.instance(c, h) for h in c.hops)}
    for k0r in (32, 96):
        assert {(g, h) for k, g, h in seen if k == k0r} == {("pe", 0), ("xcd", 1), ("xcd", 2)}, k0r
    for k0r in (32, 96):        # E = 5 (idle XCD slots) and E = 9 (the (P, E) grid under every option)
        es = {c.shape["E"] for c in tc.HOP_CASES if tc.instance(c).K0R == k0r}
        assert es >= {5, 9}, (k0r, es)
    assert any(c.shape["E"] == 8 for c in tc.HOP_CASES)
    for c in tc.HOP_CASES:
        grids = [tc.instance(c, h).grid for h in tc.HOPS]
        assert grids == (["pe"] * 4 if c.shape["E"] > rdm.XCD_MAX_E else ["xcd", "pe", "xcd", "xcd"]), c.id
        assert [tc.instance(c, h).hop for h in tc.HOPS] == ([0] * 4 if c.shape["E"] > 8 else [2, 0, 1, 2]), c.id
    # the hand-off tags the GPU test reads need two phases at least (a lone phase leaves the roll call's granules)
    assert all(c.H * (c.shape["L"] - 1) >= 2 for c in tc.COOP)
    assert {c.shape["L"] for c in tc.COOP} == {2, 3, 4}
    # plain: ungated and gated, the abort hook at a reg shape, a K0R = 96 narrow shape and a shape coop refuses
    assert {(tc.instance(c).gated, c.abort) for c in tc.PLAIN} == {(False, 0), (True, 1), (False, 1)}
    ab = {c.id: c for c in tc.PLAIN if c.abort}
    s, a, W, L, E = _shape(ab["abort_reg_shape"])
    assert rdm.trajectory_instance(s, a, W, L, E, H=4).kernel == "reg"
    s, a, W, L, E = _shape(ab["abort_c96_narrow"])
    assert rdm.trajectory_instance(s, a, W, L, E, H=4) == tc._coop(96, 2)
    s, a, W, L, E = _shape(ab["abort_coop_refused"])
    assert rdm.trajectory_instance(s, a, W, L, E, H=3) == rdm.Plain("plain", False)


def test_every_listed_edge_is_in_the_table():
    reg = {c.id: c for c in tc.REG}
    sh = lambda c: (c.shape["s"], c.shape["a"], c.shape["W"], c.shape["L"], c.shape["E"], c.H)  # noqa: E731
    at = lambda wp: [c for c in tc.REG if tc.instance(c).WP == wp]  # noqa: E731
    # W < Wpad and W = Wpad at each WP
    assert {c.shape["W"] for c in at(64)} >= {8, 33, 64}
    assert {c.shape["W"] for c in at(128)} >= {100, 128} and {c.shape["W"] for c in at(256)} >= {200, 256}
    assert any(sh(c)[0] + sh(c)[1] == 8 for c in tc.REG) and any(sh(c)[0] + sh(c)[1] == 9 for c in tc.REG)
    assert any(sh(c)[:2] == (31, 1) for c in tc.REG)                               # K0 = 32 at the largest s
    assert {1, 16, 17} <= {c.shape["s"] for c in tc.REG}
    assert any(c.H == 1 for c in tc.REG) and any(c.shape["E"] == 3 for c in tc.REG)
    assert len(reg) == len(tc.REG)
    # both sides of each boundary, and the two sides differ where they should
    for ok_id, other_id, what in tc.BOUNDARIES:
        for i in (ok_id, other_id):
            assert i is None or tc.by_id(i), what
    k8, k9 = tc.by_id("r64_n1_k8_K0_8"), tc.by_id("r64_n1_k32_K0_9")
    assert (tc.instance(k8).K0R, tc.instance(k9).K0R) == (8, 32) and sh(k9)[1] - sh(k8)[1] == 1
    assert sh(k8)[0] + sh(k8)[1] == rdm.REG_K0_SPLIT
    s16, s17 = tc.by_id("r64_n2_k32_s16"), tc.by_id("r64_n2_k32_s17")
    assert tc.instance(s16) == tc.instance(s17) and (sh(s16)[0], sh(s17)[0]) == (16, 17)
    # the reg / coop line on H a: exactly at the limit, and one step past it, at Wpad 64 and 128
    for wp, reg_id, coop_id, wi in ((64, "line64_reg", "line64_coop", 2), (128, "line128_reg", "line128_coop", 4)):
        r, c = tc.by_id(reg_id), tc.by_id(coop_id)
        assert r.shape == c.shape and c.H == r.H + 1 and r.shape["W"] == wp
        assert r.H * r.shape["a"] == 16384 - 192 - 2 * wp                          # the issue's formula, met exactly
        assert 4 * (rdm.REG_FIXED_FLOATS + 2 * wp + r.H * r.shape["a"]) == rdm.REG_LDS_LIMIT
        assert tc.instance(r) == rdm.Reg("reg", wp, 1, 32) and tc.instance(c) == tc._coop(32, wi)
    # <32, 2, 2> and <32, 2, 4> have no other route: below the line the register kernel takes every such shape
    for s in range(1, 33):
        for a in range(1, 33 - s):
            for W in (64, 128):
                for L in (2, 3, 4):
                    assert rdm.trajectory_instance(s, a, W, L, H=6).kernel == "reg"
    # coop: every width per budget, the listed s and K0, each L, E = 5 / 8 / 9
    c96 = [c for c in tc.COOP if tc.instance(c).K0R == 96]
    assert {c.shape["W"] for c in c96} == {64, 128, 256, 512}
    assert {33, 65, 80} <= {c.shape["s"] for c in c96}
    assert any(sh(c)[:2] == (80, 16) for c in c96)                                  # K0 = 96 exactly
    assert any(sh(c)[0] <= 32 < sh(c)[0] + sh(c)[1] for c in c96)                   # K0 > 32 alone
    c32 = [c for c in tc.COOP if tc.instance(c).K0R == 32 and c.shape["W"] == 256]
    assert {c.shape["L"] for c in c32} == {3, 4}
    assert {5, 8, 9} <= {c.shape["E"] for c in tc.COOP}
    # the refused side of the coop budget
    pl = {c.id: sh(c) for c in tc.PLAIN}
    assert pl["plain_W100"][2] == 100 and pl["plain_L1_W512"][2:4] == (512, 1)
    assert pl["plain_PE_1028"][4] * (pl["plain_PE_1028"][2] // 16) == 1028
    # each is one step from a cooperative shape
    assert rdm.trajectory_instance(40, 3, 128, 2, H=3).kernel == "coop"
    assert rdm.trajectory_instance(17, 6, 512, 2, H=3).kernel == "coop"
    assert rdm.trajectory_instance(33, 1, 64, 2, 256, H=2).kernel == "coop"
    for _, N, K in tc.PLANS:
        assert N <= 64 and K <= N
    assert [tc.instance(tc.by_id(i)).kernel for i, _, _ in tc.PLANS] == ["reg", "coop", "coop"]
    assert tc.instance(tc.by_id(tc.PLANS[1][0])).K0R == 96 and tc.PLANS[2][0] == "line64_coop"


def test_trajectory_model_constants_are_the_sources():
    """Each threshold trajectory_instance copies stands exactly once in the host code, as the model has it."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    traj, plan, host = src("traj.hip"), src("plan.hip"), src("mbrl_host.h")
    k0r = one(traj, r"if \(K0 <= (\d+) && A\.s <= (\d+)\) return (\d+);\n    if \(K0 <= (\d+) && A\.s <= (\d+)\) return (\d+);")
    assert tuple(int(x) for x in k0r) == (32, 32, 32, 96, 80, 96)
    assert tuple((k, s) for k, s, _ in rdm.COOP_BUDGETS) == ((32, 32), (96, 80))
    sm = one(traj, r"return coop_k0r\(A\) == 32 \? launch_coop_width<32, (\d)>\(A, E, xchg, status, stream\)\n"
                   r"\s*: launch_coop_width<96, (\d)>\(A, E, xchg, status, stream\);")
    assert tuple(int(x) for x in sm) == tuple(m for _, _, m in rdm.COOP_BUDGETS)
    for _, max_s, m in rdm.COOP_BUDGETS:
        assert 16 * m >= max_s
    rmh = one(traj, r"inline int reg_max_hidden\(int Wp\) \{ return Wp <= 64 \? (\d) : \(Wp <= 128 \? (\d) : "
                    r"\(Wp <= 256 \? (\d) : (\d)\)\); \}")
    assert [int(x) for x in rmh] == [rdm._reg_max_hidden(w) for w in (64, 128, 256, 512)]
    assert int(one(traj, r"if \(A\.Wpad > (\d+) \|\| A\.L - 1 > reg_max_hidden\(A\.Wpad\) \|\| K0 > 32 \|\| A\.s > 32\) "
                         r"return false;")) == rdm.REG_MAX_W
    assert int(one(traj, r"if \(K0 <= (\d+)\)\n\s*hipLaunchKernelGGL\(\(traj_reg_kernel<WP, NHL, 8>\)")) == rdm.REG_K0_SPLIT
    one(traj, r"else\n\s*hipLaunchKernelGGL\(\(traj_reg_kernel<WP, NHL, 32>\)")
    kib = one(traj, r"return \(size_t\)\(32 \+ 2 \* A\.Wpad \+ 32 \+ 128 \+ A\.H \* A\.a\) \* sizeof\(float\) <= (\d+) \* 1024;")
    assert int(kib) * 1024 == rdm.REG_LDS_LIMIT and rdm.REG_FIXED_FLOATS == 32 + 32 + 128
    one(traj, r"const size_t lds = \(size_t\)\(32 \+ 2 \* WP \+ 32 \+ 128 \+ A\.H \* A\.a\) \* sizeof\(float\);")
    assert int(one(traj, r"\.total <= (\d+) \* 1024;")) * 1024 == rdm.COOP_LDS_LIMIT
    grid = one(traj, r"if \(k0r == 0 \|\| A\.L < 2 \|\| A\.W != A\.Wpad \|\| A\.Wpad > COOP_MAX_W \|\| P \* E > (\d+)\) return false;")
    assert int(grid) == rdm.COOP_MAX_GRID
    assert int(one(traj, r"constexpr int COOP_ROWS = (\d+);")) == rdm.COOP_ROWS
    assert int(one(traj, r"if \(A\.hop_mode >= 1 && E <= (\d+) && xcd_fits\) \{")) == rdm.XCD_MAX_E
    assert int(one(host, r"constexpr int kTrajHopDefault = (\d+);")) == rdm.TRAJ_HOP_DEFAULT
    one(plan, r"T\.hop_mode = hop == 0 \? kTrajHopDefault : hop - 1;")
    one(plan, r"if \(traj_reg_supported\(T\) && opt\(MBRL_OPT_DEBUG_TRAJ_ABORT\) == 0\)")
    one(plan, r"ts\.xchg_bytes = \(size_t\)g\.E \* 2 \* g\.Wpad \* 8;")
    # the cooperative kernel's LDS map, block by block
    one(traj, r"m\.rs = W \+ 32;")
    one(traj, r"m\.slices = o; o \+= \(size_t\)\(L - 1\) \* COOP_ROWS \* m\.rs;\n\s*m\.x0 = o;\s+o \+= al4\(K0R > s \+ a \? K0R : s \+ a\);"
              r"\n\s*m\.hA = o;\s+o \+= Wp;\n\s*m\.hB = o;\s+o \+= Wp;\n\s*m\.out = o;\s+o \+= al4\(s\);")


def test_model_agrees_with_a_brute_force_reading_of_the_host_code():
    """trajectory_instance against the conditions written out once more, straight from traj_impl's order of
    questions, over a grid of shapes around every threshold."""
    n = 0
    for s in (1, 8, 16, 17, 31, 32, 33, 64, 65, 80, 81):
        for a in (1, 2, 8, 15, 16, 17, 24, 28):
            for W in (8, 33, 64, 100, 128, 200, 256, 300, 512, 513):
                for L in (1, 2, 3, 4):
                    for E, H in ((1, 3), (8, 3), (9, 3), (64, 3), (65, 2), (1, 600), (1, 1100)):
                        got = rdm.trajectory_instance(s, a, W, L, E, H=H)
                        Wp = 64 * rdm.geometry(s, a, W, L, E)["T"]
                        K0 = s + a
                        nhl_ok = L - 1 <= (3 if Wp <= 128 else 1)
                        if Wp <= 256 and nhl_ok and K0 <= 32 and s <= 32 and H * a <= 16384 - 192 - 2 * Wp:
                            want = ("reg", Wp, L - 1, 8 if K0 <= 8 else 32)
                        elif ((K0 <= 32 and s <= 32) or (K0 <= 96 and s <= 80)) and L >= 2 and W == Wp and Wp <= 512 \
                                and Wp // 16 * E <= 1024 and rdm._coop_lds_bytes(s, a, W, Wp, L, H, 32 if K0 <= 32 and s <= 32 else 96) <= 150 * 1024:
                            k = 32 if K0 <= 32 and s <= 32 else 96
                            want = ("coop", k, 2 if k == 32 else 5, Wp // 32) + (("xcd", 2) if E <= 8 else ("pe", 0))
                        else:
                            want = ("plain", False)
                        assert tuple(got) == want, ((s, a, W, L, E, H), got, want)
                        n += 1
    assert n > 9000


def test_float32_oracle_is_within_D_of_float64_and_D_is_a_tenth_of_the_tight_bar():
    """The GPU test compares with the float64 rollout at 32 D (tc.TIGHT) and at the suite's 1e-4. D bounds the
    float32 oracle's own distance from float64 over the whole table, horizons of 1005 steps included (the
    synthetic models are contractive: the distance does not grow with H), so a float32 evaluation in another
    summation order has room under the tight bar and a wrong column does not. States stay O(1), so absolute
    distances mean something."""
    worst, big = {}, 0.0
    for c in tc.CASES:
        s64, s32 = tc.reference(c.id)
        assert s64.shape == s32.shape == (c.shape["E"], c.H, c.shape["s"]) and np.all(np.isfinite(s64))
        worst[c.id] = float(np.max(np.abs(s32.astype(np.float64) - s64)))
        big = max(big, float(np.max(np.abs(s64))))
        assert 1e-3 < float(np.max(np.abs(s64))) < 10.0, (c.id, float(np.max(np.abs(s64))))
        # the states move: a kernel that stops early, or repeats a step, is far outside the bar
        if c.H > 1:
            assert float(np.max(np.abs(s64[:, -1] - s64[:, 0]))) > 100 * tc.TIGHT, c.id
    d = max(worst.values())
    print("float32 oracle vs float64, worst abs distance D = %.3g (tc.D = %.3g, tight bar %.3g, largest |state| %.3g); "
          "per case: %s" % (d, tc.D, tc.TIGHT, big,
                            ", ".join("%s %.2g" % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1])[:8])))
    assert d <= tc.D, worst
    assert tc.TIGHT == 32 * tc.D and d < tc.TIGHT / 10
    assert tc.TIGHT < tc.HARD / 4            # the tight bar is well inside the suite's rtol = atol = 1e-4
