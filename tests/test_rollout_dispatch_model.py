"""CPU checks of the rollout dispatch model (tests/rollout_dispatch_model.py) and its case table
(tests/rollout_cases.py): every case lands on the branch it was built for, the table reaches every fp32
instance launch_rollout lists (REQUIRED below, written from the launcher's structure), the geometry half of
the model equals the library's (mbrl_mlp_packed_bytes is host-only), neighbouring cases sit on opposite
sides of the 160 KiB line, the model's constants are the ones in the sources, and the float32 oracle is
close enough to float64 at every case's H for the suite's bars to judge the kernel and not the oracle.
tests/test_gpu_envelope.py runs the same table on the GPU, which pins the LDS half."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import cem as ocem

import rollout_cases as rc
import rollout_dispatch_model as rdm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mujoco-mbrl_amd", "csrc")
RTOL = 1e-5            # test_gpu_parity.RTOL (that module needs no GPU to import, but marks itself gpu)


def _outcomes():
    return [(c, rc.run_outcome(c)) for c in rc.ACCEPTED]


def test_every_case_lands_where_it_was_built_to():
    ids = [c.id for c in rc.ACCEPTED + rc.REFUSED]
    assert len(set(ids)) == len(ids)
    for c, out in _outcomes():
        assert isinstance(out, rdm.Instance), (c.id, out)
        for k, v in c.built_for.items():
            assert getattr(out, k) == v, (c.id, k, getattr(out, k), v)
        assert out.lds_bytes <= rdm.LDS_LIMIT, c.id
        assert 1 <= c.H <= 4 and (c.N <= 64 or c.N >= rdm.R2_MIN_N), c.id
    for c in rc.REFUSED:
        out = rc.outcome(c)
        assert isinstance(out, rdm.Refusal) and out.code == rdm.MBRL_EUNSUPPORTED, (c.id, out)
        assert out.fragment == c.fragment, (c.id, out.fragment)


# ------------------------------------------------------------------------------------------------
# The coverage condition: each entry is a dict of Instance fields some accepted case must carry together.
# From launch_rollout: every (T, R) of MBRL_CASE, each as a ring and as the generic instance; from
# launch_rollout_t: both wave counts where the launcher can ask for either (R = 2 needs 8 pw <= lda for 8
# waves, which only Wpad = 512 offers; R = 1 has one wave count per T); from rollout_impl: the partials
# aliased and not, the reward head on and off at either tile height and at T = 16, each fallback.
REQUIRED = [dict(kernel="m16", T=T, R=R) for T, R in rdm.CASES]
REQUIRED += [dict(T=T, R=R, K0C_T=0) for T, R in rdm.CASES]
REQUIRED += [dict(T=T, R=R, K0C_T=2) for T, R in rdm.CASES]
REQUIRED += [dict(T=16, K0C_T=6, NOT_T=6), dict(T=8, K0C_T=6, NOT_T=2), dict(T=8, R=2, K0C_T=6, NOT_T=6)]
REQUIRED += [dict(T=8, R=2, NW=4, K0C_T=0), dict(T=8, R=2, NW=8, K0C_T=0),
             dict(T=8, R=2, NW=4, K0C_T=2), dict(T=8, R=2, NW=8, K0C_T=2)]
REQUIRED += [dict(T=16, part_alias=a, K0C_T=k, reward=0) for a in (False, True) for k in (0, 2)]
REQUIRED += [dict(R=2, part_alias=a) for a in (False, True)]
REQUIRED += [dict(R=R, reward=w) for R in (1, 2) for w in (0, 1)]
REQUIRED += [dict(T=16, reward=1, K0C_T=0), dict(T=16, reward=1, K0C_T=2), dict(R=2, reward=1, K0C_T=2, T=8),
             dict(R=2, reward=1, T=2)]
REQUIRED += [dict(fallback="lds"), dict(fallback="actions"), dict(R=2, fallback=None)]
REQUIRED += [dict(T=8, R=1, GS=True)]
REQUIRED_REFUSALS = ("action_dim", "unsupported MLP shape", "LDS footprint")
REQUIRED_MODES = ("given", "per_cand", "sampled")


def _unreached(outcomes):
    return [req for req in REQUIRED if not any(all(getattr(o, k) == v for k, v in req.items()) for o in outcomes)]


def test_table_reaches_every_instance_fallback_and_refusal():
    outs = [o for _, o in _outcomes()]
    assert not _unreached(outs), "unreached: %s" % _unreached(outs)
    assert {(o.T, o.R) for o in outs} == set(rdm.CASES)
    for frag in REQUIRED_REFUSALS:
        assert any(frag in c.fragment for c in rc.REFUSED), frag
    # the two refusals of make_geometry (width, depth) separately
    assert {rc.shape_of(c)[2] > 1024 for c in rc.REFUSED if "MLP shape" in c.fragment} == {True, False}
    assert {c.mode for c in rc.ACCEPTED} >= set(REQUIRED_MODES)
    assert any(rc.shape_of(c)[4] > 1 for c in rc.ACCEPTED)                       # an ensemble
    assert any(c.mode == "per_cand" and c.H > 1 for c in rc.ACCEPTED)
    # wide input: the row stride comes from the input
    wide = [c for c in rc.ACCEPTED if 16 * rdm.geometry(*rc.shape_of(c))["K0C"] > rdm.geometry(*rc.shape_of(c))["Wpad"]]
    assert len(wide) >= 2
    # unpadded widths at T = 16, action dims over the whole new range
    assert any(rc.shape_of(c)[2] not in (64, 128, 256, 512, 1024) and o.T == 16 for c, o in _outcomes())
    assert {rc.shape_of(c)[1] for c in rc.ACCEPTED} >= {24, 25, 30, 40, 48}


# what the issue lists by name: deleting one fails here even where another case reaches the same instance
LISTED = ("t16_ring22_L1", "t16_ring22_L2", "t16_ring22_L3", "t16_W513", "t16_W1000", "t16_generic_L2",
          "t16_generic_L3", "t16_humanoid_L3_E2", "t16_reward", "r2_t1_ring", "r2_t1_generic", "r2_t2_generic_L3",
          "r2_t4_cartpole_ring", "r2_t4_generic", "r2_t8_generic_L2", "r2_t8_generic_L3", "r2_reward_W512",
          "r2_reward_W128", "fb_humanoid_L2", "fb_humanoid_L4", "fb_a25", "r2_a24", "wide_s90", "wide_s200",
          "a48_N40", "a48_N8192", "no_a49", "no_W1025", "no_L5", "no_W1024_L4", "no_humanoid_W1024_L2", "no_s500")


def test_every_listed_case_is_in_the_table():
    have = {c.id for c in rc.ACCEPTED + rc.REFUSED}
    assert not [i for i in LISTED if i not in have]


def test_coverage_condition_notices_a_deleted_case():
    """Dropping any one case that alone reaches a requirement leaves it unreached: the condition is not
    satisfied by accident (checked for the cases the requirement list was written around)."""
    full = _outcomes()
    for victim in ("t16_generic_L2", "t16_humanoid_L3_E2", "r2_t1_generic", "r2_t2_generic_L3", "r2_t4_generic",
                   "r2_t8_generic_L2", "r2_reward_W128", "t16_reward_generic", "r2_t8_humanoid_L3"):
        rest = [o for c, o in full if c.id != victim]
        assert len(rest) == len(full) - 1 and _unreached(rest), victim


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mbrl_amd import _lib
    return _lib, _lib.load()


def _library_stride(lib, s, a, W, L, E, reward):
    _lib, h = lib
    sh = _lib.MlpShape(s, a, W, L, E, reward, 0)
    nbytes = h.mbrl_mlp_packed_bytes(ctypes.byref(sh))
    return nbytes, (nbytes // (4 * E) if nbytes else 0)


def test_member_stride_equals_the_librarys(lib):
    """make_geometry's every piece (T, K0C, NOT, the stream, bias, plain, split, m8 and m4 regions) adds up
    to the member stride, so one number pins the geometry half of the model to the C++."""
    shapes = [rc.shape_of(c) for c in rc.ACCEPTED + rc.REFUSED]
    rng = np.random.default_rng(20260)
    for _ in range(400):
        shapes.append((int(rng.integers(1, 260)), int(rng.integers(1, 60)),
                       int(rng.choice([1, 8, 63, 64, 65, 128, 129, 200, 256, 257, 512, 513, 777, 1024, 1025, 1500])),
                       int(rng.integers(1, 6)), int(rng.integers(1, 4)), int(rng.integers(0, 2))))
    shapes += [(1025 * 16, 1, 8, 1, 1, 0), (1, 1, 1, 1, 1, 0), (2049, 3, 1024, 4, 1, 1)]
    refused = 0
    for sh in shapes:
        g = rdm.geometry(*sh)
        nbytes, stride = _library_stride(lib, *sh)
        if g is None:
            refused += 1
            assert nbytes == 0, sh
        else:
            assert stride == g["member_stride"] and nbytes == 4 * sh[4] * g["member_stride"], (sh, stride, g)
    assert refused >= 20


def test_neighbouring_cases_straddle_the_lds_line():
    for ok_id, no_id, _why in rc.LINE:
        ok, no = rc.run_outcome(rc.by_id(ok_id)), rc.outcome(rc.by_id(no_id))
        assert isinstance(ok, rdm.Instance) and isinstance(no, rdm.Refusal), (ok_id, no_id)
        assert ok.lds_bytes <= rdm.LDS_LIMIT < no.lds_bytes and no.lds_bytes - ok.lds_bytes <= 48 * 1024
    # the closest accepted shape sits within 2 % of the limit, so a few words more in lds_map refuse it
    assert max(o.lds_bytes for _, o in _outcomes()) == 161920 and rdm.LDS_LIMIT - 161920 < 2048
    # a 32-row map past the line falls back instead: humanoid's at L = 2
    g = rdm.geometry(67, 21, 512, 2)
    assert rdm.lds_need_bytes(g, 32, 4, False) > 200000 > rdm.LDS_LIMIT >= rdm.lds_need_bytes(g, 16, 8, False)


def test_trajectory_kernel_budgets():
    """Which single-trajectory kernel runs: register-resident, cooperative, or the plain single-workgroup
    kernel past the cooperative kernel's budgets (s > 80 or s + a > 96) and for every W > 512."""
    tk = rdm.trajectory_kernel
    assert tk(5, 1, 256, 2, H=20) == "reg" and tk(17, 6, 512, 3, H=30) == "coop" and tk(67, 21, 512, 3, H=50) == "coop"
    assert tk(80, 16, 512, 2, H=4) == "coop"
    assert tk(81, 6, 512, 2, H=4) == "plain" and tk(60, 37, 512, 2, H=4) == "plain" and tk(90, 6, 512, 2, H=4) == "plain"
    assert tk(17, 6, 1024, 2, H=4) == "plain" and tk(17, 6, 513, 2, H=4) == "plain" and tk(17, 6, 500, 2, H=4) == "plain"
    assert tk(90, 30, 16, 2, H=4) == "plain" and tk(17, 6, 512, 1, H=4) == "plain"


def test_model_constants_are_the_sources():
    """A change of a threshold in the host code fails here, and sends its author to the model."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    hdr, plan, roll, traj = src("mbrl_internal.h"), src("plan.hip"), src("rollout.hip"), src("traj.hip")
    assert int(one(hdr, r"constexpr int MAX_LAYERS = (\d+);")) == rdm.MAX_LAYERS
    assert int(one(hdr, r"if \(T > (\d+)\) return false;")) == rdm.MAX_T
    one(hdr, r"g->K0C = round_even\(\(s \+ a \+ 15\) / 16\);")
    one(hdr, r"g->NOT = round_even\(\(g->so \+ 15\) / 16\);")
    one(hdr, r"g->lda = \(g->Wpad > k0 \? g->Wpad : k0\) \+ 4;")
    one(hdr, r"g->pw = 16 \* g->NOT \+ 4;")
    one(hdr, r"L\.part = A\.part_alias \? L\.act2 : take\(\(size_t\)\(A\.nw > 4 \? A\.nw : 4\) \* M \* A\.pw\);")
    assert int(one(hdr, r"const size_t floor_bytes = (\d+) \* 1024;")) * 1024 == rdm.LDS_FLOOR
    assert len(re.findall(r"> 160 \* 1024", plan)) >= 3 and rdm.LDS_LIMIT == 160 * 1024
    one(plan, r"if \(16 \* g\.a > 768\) return fail\(MBRL_EUNSUPPORTED, \"action_dim %d too large \(max 48\)\", g\.a\);")
    one(plan, r"int R = \(N >= 2 \* 16 \* 256 && g\.T <= 8\) \? 2 : 1;")
    one(plan, r"if \(16 \* R \* g\.a > 768\) R = 1;")
    one(plan, r"A\.nw = \(R == 1 && g\.T >= 2\) \? 8 : 4;")
    one(plan, r"return !reward && g\.L >= 3 && \(g\.L & 1\) && \(size_t\)\(nw > 4 \? nw : 4\) \* g\.pw <= \(size_t\)g\.lda;")
    one(plan, r"if \(R == 2 && g\.T >= 2 && !A\.reward && g\.L >= 3 && \(g\.L & 1\) && \(size_t\)8 \* g\.pw <= \(size_t\)g\.lda\) A\.nw = 8;")
    one(plan, r"bool use8 = \(size_t\)\(\(N \+ 15\) / 16\) \* g\.E \* 2 <= \(size_t\)device_cu_count\(\);")
    one(plan, r"const bool gs_auto = g\.T == 8 && g\.K0C == 2 && g\.NOT == 2;")
    ladder = one(roll, r"\n    (MBRL_CASE\(1, 1\)[^#]*)#undef MBRL_CASE")
    assert tuple((int(t), int(r)) for t, r in re.findall(r"MBRL_CASE\((\d+), (\d+)\)", ladder)) == rdm.CASES
    rings = re.findall(r"if \(A\.K0C == (\d) && A\.NOT == (\d)\) return launch_rollout_tr<T, R, \1, \2, NW>", roll)
    assert tuple((int(k), int(n)) for k, n in rings) == rdm.RING_SHAPES
    one(roll, r"if constexpr \(4 \* T / NW <= 8\) \{")
    one(roll, r"constexpr int NW = \(T >= 2 && R == 1\) \? 8 : 4;")
    assert int(one(traj, r"constexpr int COOP_MAX_W = (\d+);")) == rdm.COOP_MAX_W
    one(traj, r"if \(K0 <= 32 && A\.s <= 32\) return 32;\n    if \(K0 <= 96 && A\.s <= 80\) return 96;")
    one(traj, r"if \(A\.Wpad > 256 \|\| A\.L - 1 > reg_max_hidden\(A\.Wpad\) \|\| K0 > 32 \|\| A\.s > 32\) return false;")
    one(traj, r"\.total <= 150 \* 1024;")


# ------------------------------------------------------------------------------------------------
def test_float32_oracle_is_within_a_tenth_of_the_bar_of_float64():
    """The GPU bar is RTOL against the float32 oracle. At W = 1024 a dot product is twice as long as where
    that bar was set, so H is chosen per case such that the oracle's own rounding (its distance from the
    same rollout in float64) stays under RTOL / 10: a miss on the GPU is then the kernel's."""
    worst = {}
    for c in rc.ACCEPTED:
        p = ocem.synth_problem(c.cid, N=c.N, H=c.H, **c.over)
        n = min(c.N, rc.ORACLE_ROWS)
        if c.mode == "sampled":
            continue            # same shape family as t16_ring22_L3 (drawn actions, same H or shorter)
        s0, A = rc.given_inputs(c, p)
        A = np.ascontiguousarray(A[:, :n])
        s0 = s0[:n] if s0.ndim == 2 else s0
        c32 = ocem.rollout(p["model"], p["norm"], p["cost"], s0, A).astype(np.float64)
        c64 = rc.rollout_f64(p, s0, A)
        assert np.all(np.isfinite(c64))
        worst[c.id] = float(np.max(np.abs(c32 - c64) / np.maximum(np.abs(c64), 1.0)))
    bad = {k: v for k, v in worst.items() if not v < RTOL / 10}
    print("float32 oracle vs float64, worst relative distance per case:",
          ", ".join("%s %.2g" % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1])[:8]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ split kernels
# The 28 instantiations launch_rollout_split lists: (T, R, P, K0S, NOS), R = 2 only where NOS = 1.
SPLIT_LISTED = {(T, R, P, k, n) for T in rdm.SPLIT_T for P in (2, 3) for k, n in rdm.SPLIT_SHAPES
                for R in ((1, 2) if n == 1 else (1,))}
# NOS = 3 needs s > 64, and then s + a > 64 gives K0S = 3: a goal-state model cannot have (K0S, NOS) = (1, 3)
SPLIT_UNREACHABLE = {(T, 1, P, 1, 3) for T in rdm.SPLIT_T for P in (2, 3)}


def _inst(o):
    return (o.T, o.R, o.P, o.K0S, o.NOS)


def test_split_model_reaches_24_of_the_28_listed_instantiations():
    """s in 1..100, a in 0..50, W in {129, 256, 257, 512}, L in 1..4, N = 40, split_tile 0 /
    32, both precisions: every listed instantiation but the four (1, 3) ones is reached, and nothing else.
    (1, 3) stays listed in launch_rollout_split; it is dead code for goal-state models."""
    import split_cases as sc
    assert len(SPLIT_LISTED) == 28
    reached, ts = set(), set()
    for s in range(1, 101):
        for a in range(0, 51):
            for W in (129, 256, 257, 512):
                for L in range(1, 5):
                    for P in (2, 3):
                        for N, tile in ((sc.N, 0), (sc.N, 32)):      # (N >= 8192 asks what split_tile = 32 asks)
                            o = rdm.split_kernel(s, a, W, L, N=N, P=P, split_tile=tile)
                            if o.kind == "split":
                                reached.add(_inst(o))
                                ts.add((o.R, o.P, o.K0S, o.NOS, o.TS))
                                assert o.lds_bytes <= rdm.LDS_LIMIT
                            else:
                                assert o.reason != "refused" or a == 0 or a > rdm.SPLIT_MAX_A, (s, a, W, L)
    assert reached == SPLIT_LISTED - SPLIT_UNREACHABLE and len(reached) == 24
    assert {t[-1] for t in ts} == {1, 2} and all(TS == 2 for R, P, k, n, TS in ts if P == 2)
    # N >= 8192 asks for R = 2 by itself, split_tile = 16 overrides it
    assert rdm.split_kernel(17, 6, 512, 3, N=8192, P=2).R == 2 and rdm.split_kernel(17, 6, 512, 3, N=8191, P=2).R == 1
    assert rdm.split_kernel(17, 6, 512, 3, N=8192, P=2, split_tile=16).R == 1
    for sh in ((17, 6, 512, 3), (49, 49, 512, 2), (500, 12, 64, 2), (67, 21, 512, 2), (5, 1, 1025, 2)):
        refused = isinstance(rdm.dispatch(*sh, N=sc.N), rdm.Refusal)
        assert (rdm.split_kernel(*sh, N=sc.N, P=3) == rdm.F32("f32", "refused")) == refused, sh


def test_every_split_case_lands_where_it_was_built_to_and_the_table_reaches_every_instantiation():
    import split_cases as sc
    ids = [c.id for c in sc.ACCEPTED + sc.DECLINED]
    assert len(set(ids)) == len(ids)
    hit = set()
    for c in sc.ACCEPTED + sc.DECLINED:
        assert c.N == sc.N and c.H in (1, 2, 3), c.id
        for P in (2, 3):
            o = sc.outcome(c, P)
            for k, v in c.built_for.items():
                assert getattr(o, k) == v, (c.id, P, k, getattr(o, k), v)
            if o.kind == "split":
                hit.add(_inst(o))
    assert hit == SPLIT_LISTED - SPLIT_UNREACHABLE, sorted(SPLIT_LISTED - SPLIT_UNREACHABLE - hit)
    # dropping a case that alone reaches an instantiation leaves it unreached
    for victim in ("c22_t4", "c33_t4", "c31_bump_t8_r2"):
        rest = {_inst(sc.outcome(c, P)) for c in sc.ACCEPTED if c.id != victim for P in (2, 3)}
        assert rest < hit, victim
    # what the table promises beside the instantiations
    acc = sc.ACCEPTED
    assert {c.mode for c in acc} == {"given", "per_cand", "sampled"} and {c.H for c in acc} == {1, 2, 3}
    depth = lambda T: {sc.shape_of(c)[3] for c in acc if sc.outcome(c, 2).T == T and sc.outcome(c, 2).K0S == 1}  # noqa: E731
    assert depth(4) == {1, 2, 3, 4} and depth(8) == {1, 2, 3, 4}
    assert {sc.shape_of(c)[2] for c in acc} >= {129, 200, 257, 300} and {sc.shape_of(c)[1] for c in acc} >= {16, 17, 32, 33, 48}
    assert any(sc.shape_of(c)[4] == 2 and sc.outcome(c, 2).NOS == 1 for c in acc)
    assert any(sc.shape_of(c)[4] == 2 and sc.outcome(c, 2).NOS == 3 for c in acc)
    # the parity bump: 32 K0S covers a whole chunk more than s + a needs
    bumped = [c for c in acc if 32 * sc.outcome(c, 2).K0S - sum(sc.shape_of(c)[:2]) >= 32]
    assert {c.id for c in bumped} >= {"c31_bump_t4", "c31_bump_t4_r2", "c31_bump_t8", "c31_bump_t8_r2"}
    # the weight ring of one step is two slots (L = 1, T = 4, two tiles per slot): the prefetch wraps twice
    assert any(sc.shape_of(c)[3] == 1 and sc.outcome(c, 2).T == 4 and c.H == 3 for c in acc)
    # R = 2 requests turned down keep the split kernel on 16-candidate tiles; each reason is there
    for cid in sc.R2_DECLINED:
        assert sc.tile_of(sc.by_id(cid)) == 32 and sc.outcome(sc.by_id(cid), 2).R == 1
    g = rdm.geometry(20, 48, 512, 3)
    assert rdm._split_refusal(g, 2, 3) is None and rdm.lds_launch_bytes(g, 32, 4, False) > rdm.LDS_LIMIT
    assert {c.built_for["reason"] for c in sc.DECLINED} >= {"shape class (4, 2)", "refused", "T = 2", "T = 16", "reward head"}
    assert any(sc.shape_of(c)[0] == 100 for c in sc.DECLINED)


def test_split_model_constants_are_the_sources():
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(text, pattern):
        assert len(re.findall(pattern, text)) == 1, pattern

    hdr, plan, split = src("mbrl_internal.h"), src("plan.hip"), src("rollout_f16x3.hip")
    one(hdr, r"g->split_ok = \(T == 4 \|\| T == 8\) \? 1 : 0;")
    one(hdr, r"g->K0S = \(s \+ a \+ 31\) / 32;\n    g->NOS = g->NOT / 2;\n    if \(\(g->K0S \+ g->NOS\) & 1\) g->K0S \+= 1;")
    one(hdr, r"g->CS = g->K0S \+ \(L - 1\) \* 2 \* T \+ g->NOS;")
    one(plan, r"S\.sr = P \* \(g\.Wpad > 32 \* g\.K0S \? g\.Wpad : 32 \* g\.K0S\) \+ 8;")
    one(plan, r"int RS = N >= 256 \* 32 \? 2 : 1;")
    one(plan, r"if \(const int o = opt\(MBRL_OPT_SPLIT_TILE\)\) RS = o == 32 \? 2 : 1;")
    one(plan, r"X\.nw = RS == 1 && g\.T >= 2 \? 8 : 4;")
    one(plan, r"if \(RS == 2 && \(!rollout_split_supported\(S, g\.T, 2, P\) \|\| rollout_lds_bytes\(X, 32\) > 160 \* 1024\)\) \{")
    shapes = re.findall(r"X\((\d), (\d)\)", re.search(r"#define MBRL_SPLIT_SHAPES\(X\)(.*)", split).group(1))
    assert tuple((int(k), int(n)) for k, n in shapes) == rdm.SPLIT_SHAPES
    one(split, r"constexpr int SW = 8;") and one(split, r"constexpr int SMAXA = 3;")
    one(split, r"if \(R != 1 && !\(R == 2 && A\.NOT == 2\)\) return false;")
    one(split, r"if \(A\.reward \|\| \(T != 4 && T != 8\) \|\| A\.a > 16 \* SMAXA\) return false;")
    one(split, r"if \(rollout_split_lds_bytes\(A, R\) > 160 \* 1024\) return false;")
    one(split, r"constexpr int split_ts\(\) \{ return \(P == 2 \|\| \(R == 1 && K0S <= 2 && NOS <= 2\)\) \? 2 : 1; \}")
    one(split, r"o \+= \(bytes \+ 15\) & ~\(size_t\)15;")
    one(split, r"L\.y = R == 1 \? static_cast<_Float16\*>\(take\(M \* A\.sr \* 2\)\) : L\.x;")
    one(split, r"L\.part = static_cast<float\*>\(take\(\(size_t\)SW \* M \* A\.pw \* 4\)\);")
    assert rdm.SPLIT_WAVES == 8 and rdm.SPLIT_MAX_A == 48 and rdm.SPLIT_R2_MIN_N == 8192
