"""CPU checks of the selection-branch model (tests/select_branch_model.py) and its case table
(tests/select_cases.py): the model's elites are the stable argsort's for every row, the table reaches
every feasible combination of select_reg_body's branches listed in REQUIRED -- through the select entry
and, separately, through the update entry -- and the model's constants are the ones in cem.hip.
tests/test_gpu_select_branches.py runs the same rows on the GPU."""
import os
import re

import numpy as np
import pytest

from oracle import cem as ocem

import select_branch_model as sbm
import select_cases
from test_gpu_fused_update import _fused_k_cap

CEM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mujoco-mbrl_amd", "csrc", "cem.hip")


@pytest.fixture(scope="module")
def traced():
    """(row, labels) for every row; the model's elites are checked against the oracle on the way."""
    out = []
    for row in select_cases.rows():
        c = row.costs()
        ret = ocem.ensemble_returns(c)
        assert np.array_equal(ret, row.r, equal_nan=True), row.id      # five equal members: the mean is exact
        elites, labels = sbm.select_model(ret, row.K, row.nan_policy, row.E)
        if row.nan_policy == sbm.NAN_FIRST:
            assert row.K == 1 and int(elites[0]) == ocem.rs_argmin(ret), row.id
        else:
            assert np.array_equal(elites, ocem.select_elites(ret, row.K)), row.id
        out.append((row, labels))
    return out


def test_model_elites_equal_stable_argsort(traced):
    assert len(traced) == len(select_cases.rows()) > 0
    assert len({row.id for row, _ in traced}) == len(traced)


def test_families_land_where_they_were_built_to(traced):
    """Each constructor takes the narrowing it is named for (at E = 1; the E = 5 rows scale the offsets
    by 8 and may narrow differently)."""
    for row, labels in traced:
        if row.E == 1 and row.family in ("flat", "wide_only", "rank64", "list_radix", "all_radix"):
            assert "narrow_" + row.family in labels, (row.id, sorted(labels))


def test_order_key_edges():
    f = np.float32
    tiny = np.float32(1e-45)                                 # the smallest subnormal
    r = np.array([-np.inf, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, np.inf, np.nan], dtype=f)
    k = sbm.order_key(r)
    assert k[3] == k[4] and list(k[:3]) == sorted(k[:3]) and list(k[4:]) == sorted(k[4:])
    assert k[2] < k[3] < k[5] and k[8] == 0xFFFFFFFF and sbm.order_key(r, sbm.NAN_FIRST)[8] == 0
    assert [sbm.kpt_for(n) for n in (1, 1024, 1025, 2048, 2049, 4097, 8193, 16385, 32768)] == \
        [1, 1, 2, 2, 4, 8, 16, 32, 32]


# ------------------------------------------------------------------------------------------------
# The coverage condition. Each entry is a set of labels that some row of the table must carry together.
# It is written from the kernel's structure, not from the table: a (KPT, layout) pair, the narrowings
# possible at its sizes, ties taken and cut, the compactions the kernel can choose at that KPT, the loads
# and wave variants, the arms of the 8-bit passes.
PAIRS = [("kpt1", "single"), ("kpt2", "single"), ("kpt4", "vec"), ("kpt4", "single"), ("kpt8", "vec"),
         ("kpt8", "single"), ("kpt16", "vec"), ("kpt16", "single"), ("kpt32", "vec"), ("kpt32", "single")]
# a bucket above SEL_LIST = 2048 keys needs N > 2048: from KPT = 4
NARROW = {"kpt1": ("narrow_flat", "narrow_wide_only", "narrow_rank64", "narrow_list_radix"),
          "kpt2": ("narrow_flat", "narrow_wide_only", "narrow_rank64", "narrow_list_radix"),
          "kpt4": ("narrow_flat", "narrow_wide_only", "narrow_rank64", "narrow_list_radix", "narrow_all_radix"),
          "kpt8": ("narrow_flat", "narrow_wide_only", "narrow_rank64", "narrow_list_radix", "narrow_all_radix"),
          "kpt16": ("narrow_flat", "narrow_wide_only", "narrow_rank64", "narrow_list_radix", "narrow_all_radix"),
          "kpt32": ("narrow_flat", "narrow_wide_only", "narrow_rank64", "narrow_list_radix", "narrow_all_radix")}
BITMAP_KPTS = ("kpt8", "kpt16", "kpt32")
WAVES = ("waves_all_full", "waves_some_partial")

REQUIRED = [frozenset(p) for p in PAIRS]
REQUIRED += [frozenset(p + (n,)) for p in PAIRS for n in NARROW[p[0]]]
REQUIRED += [frozenset(p + (n, t)) for p in PAIRS for n in NARROW[p[0]] for t in ("ties_all_taken", "ties_cut")]
# packed counts at every KPT in the layouts it has; from KPT = 8 the bitmaps, and packed counts because
# the ties are cut and because the K-th key is the padding key (cut, and with every NaN taken)
REQUIRED += [frozenset((k, "compact_packed_" + l)) for k, l in PAIRS]
REQUIRED += [frozenset((k, c)) for k in BITMAP_KPTS for c in ("compact_bitmap_vec", "compact_bitmap_ballot")]
REQUIRED += [frozenset((k, c, why)) for k in BITMAP_KPTS for c in ("compact_packed_vec", "compact_packed_single")
             for why in ("ties_cut", "kth_is_pad_key")]
REQUIRED += [frozenset((k, l, "kth_is_pad_key", "ties_all_taken")) for k, l in PAIRS if k in BITMAP_KPTS]
REQUIRED += [frozenset(("compact_packed_vec", b)) for b in ("beany_some", "beany_none")]
REQUIRED += [frozenset((ld, w)) for ld in ("load_e1vec", "load_general", "load_general_vec", "load_general_single")
             for w in WAVES]
REQUIRED += [frozenset((n, r)) for n in ("narrow_list_radix", "narrow_all_radix")
             for r in ("radix_short_last_digit", "radix_mixed", "radix_clustered")]
# two trips of the list loop need more than 1024 listed keys: from KPT = 2
REQUIRED += [frozenset((k, "narrow_list_radix", "list_two_trips")) for k in ("kpt2", "kpt4", "kpt8", "kpt16", "kpt32")]
REQUIRED += [frozenset(("narrow_wide_only", "wide_short")), frozenset(("narrow_wide_only",))]
REQUIRED += [frozenset(("kth_is_pad_key", w)) for w in WAVES]
REQUIRED += [frozenset(("nan_first",))]

# cem_update_kernel keeps the K elite indices and the refit's rows in LDS next to the selection: at
# KPT = 32, K = N is beyond _fused_k_cap (at N = 32768 beyond the kernel's LDS itself), and only K = N
# gives these.
UPDATE_EXEMPT = {
    frozenset(("kpt32", "vec", "narrow_flat", "ties_all_taken")): "all keys equal and all taken is K = N",
    frozenset(("kpt32", "single", "narrow_flat", "ties_all_taken")): "all keys equal and all taken is K = N",
    frozenset(("kpt32", "vec", "kth_is_pad_key", "ties_all_taken")): "every NaN taken is K = N",
    frozenset(("kpt32", "single", "kth_is_pad_key", "ties_all_taken")): "every NaN taken is K = N",
}
# mbrl_cem_update has no nan_policy argument: it selects with NAN_LAST
UPDATE_NO_SUCH_ARGUMENT = {frozenset(("nan_first",))}


def _unreached(label_sets, exempt=()):
    return [sorted(req) for req in REQUIRED if req not in exempt and not any(req <= ls for ls in label_sets)]


def test_table_reaches_every_required_combination_through_select(traced):
    missing = _unreached([labels for _, labels in traced])
    assert not missing, "unreached through mbrl_select_elites: %s" % missing


def test_table_reaches_every_required_combination_through_update(traced):
    inside = [labels for row, labels in traced
              if row.nan_policy == sbm.NAN_LAST and row.K <= _fused_k_cap(row.N, 1)]
    missing = _unreached(inside, set(UPDATE_EXEMPT) | UPDATE_NO_SUCH_ARGUMENT)
    assert not missing, "unreached through mbrl_cem_update: %s" % missing
    # the exemptions are K = N beyond the update's LDS, and nothing else: inside the cap they are unreached,
    # and the select entry reaches them with K = N rows only
    for req in UPDATE_EXEMPT:
        assert req in REQUIRED and not any(req <= ls for ls in inside), sorted(req)
        hits = [row for row, labels in traced if req <= labels]
        assert hits and all(row.K == row.N > _fused_k_cap(row.N, 1) for row in hits), sorted(req)
        assert not sbm.update_fits(32768, 32768, 1)


def test_fused_k_cap_is_inside_the_kernels(traced):
    """_fused_k_cap (the bound the update tests clamp K with) never admits a shape update_kpt() refuses."""
    for row, _ in traced:
        assert sbm.update_fits(row.N, min(row.K, _fused_k_cap(row.N, 1)), 1), row.id


def test_model_constants_are_the_kernels():
    """A kernel change that moves a threshold fails here, and sends its author to the model."""
    src = open(CEM_HIP).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (pattern, m)
        return m[0]

    assert int(one(r"constexpr int SEL_WIDE_BITS = (\d+),")) == sbm.SEL_WIDE_BITS == 11
    assert int(one(r"constexpr int SEL_LIST = (\d+);")) == sbm.SEL_LIST == 2048
    assert int(one(r"if \(bsz <= (\d+)u\) \{")) == sbm.RANK_MAX == 64
    assert int(one(r"if \(KPT >= (\d+) && eqn == kk && prefix != kpad\) \{")) == sbm.BITMAP_KPT == 8
    ladder = one(r"\n    ((?:MBRL_SEL\(\d+\) ?)+)\n#undef MBRL_SEL")
    assert tuple(int(k) for k in re.findall(r"\d+", ladder)) == sbm.KPT_LADDER == (1, 2, 4, 8, 16, 32)
    one(r"#define MBRL_SEL\(KPT\)\s*\\\n    if \(N <= 1024 \* \(KPT\)\) \{")
    one(r"const bool vec = KPT >= 4 && \(N & 3\) == 0 && \(member_stride & 3\) == 0;")
    one(r"const int wb = min\(SEL_WIDE_BITS, rem\), wshift = rem - wb;")
    one(r"if \(rem > 0 && bsz <= \(uint32_t\)SEL_LIST\) \{")
    one(r"const int db = min\(8, rem\), shift = rem - db;")
    # update_fits(): sel_words(), the 160 KiB bound of update_kpt()
    one(r"constexpr int SEL_HIST_WORDS = 2 \* 16 \* 257;")
    one(r"sel_words\(int\) \{ return SEL_HIST_WORDS \+ SEL_WIDE_BINS \+ SEL_LIST \+ 4; \}")
    one(r"return update_lds_words\(kpt, a, K\) \* 4 \+ 1024 <= 160 \* 1024 \? kpt : 0;")
