"""Every branch of the register-resident selection (cem.hip select_reg_body<KPT>) on the GPU, bit for bit
against NumPy's stable argsort: the rows of tests/select_cases.py through mbrl_select_elites
(select_reg_kernel) and through mbrl_cem_update (cem_update_kernel), each launched twice.

Which branches a row takes is what tests/select_branch_model.py predicts for it; that the table reaches
every feasible combination is tests/test_select_model.py's condition, checked on the CPU. Each test here
prints the labels predicted for its rows, so the log records what was claimed to run. The selection
inside cem_select_regen_kernel (the split update) is reached only through whole plans and is not driven
by this table: test_gpu_fused_update.py::test_split_update_plan_equals_one_launch_update covers it."""
import numpy as np
import pytest
import torch

from oracle import cem as ocem
from oracle.philox import cem_actions

import select_branch_model as sbm
import select_cases
from test_gpu_fused_update import _fused_k_cap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, ITERATION, ALPHA = 0x5E1EC7, 2, 0.1
MU = np.float32([[0.125]])             # H = 1, a = 1
SIGMA = np.float32([[0.375]])


def _select_twice(fused, costs, row):
    out = []
    for _ in range(2):
        ret = torch.full((row.N,), -7.0, dtype=torch.float32, device=DEV)
        el = fused.select(costs, row.K, nan_policy=row.nan_policy, returns_out=ret)
        out.append((el.cpu().numpy(), ret.cpu().numpy()))
    return out


def _update_twice(fused, costs, row):
    mu_d, sg_d = torch.from_numpy(MU).to(DEV), torch.from_numpy(SIGMA).to(DEV)
    sp = fused.make_sampler(SEED, ITERATION, mu_d, sg_d, -1.0, 1.0)
    out = []
    for _ in range(2):
        ret = torch.full((row.N,), -7.0, dtype=torch.float32, device=DEV)
        mu_o, sg_o = torch.full_like(mu_d, -7.0), torch.full_like(sg_d, -7.0)
        el = fused.cem_update(costs, row.K, sp, 1, 1, ALPHA, mu_o, sg_o, returns_out=ret)
        torch.cuda.synchronize()
        out.append(None if el is None else (el.cpu().numpy(), ret.cpu().numpy(), mu_o.cpu().numpy(), sg_o.cpu().numpy()))
    return out


def _same_bytes(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _returns_equal(x, ref):
    """Bit for bit (the sign of zero included), a NaN equal to any NaN."""
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(x), nan) and _same_bytes(np.where(nan, np.float32(0), x), np.where(nan, np.float32(0), ref))


@pytest.mark.parametrize("kpt,family", select_cases.groups(), ids=lambda v: str(v))
def test_select_branches_bit_exact(kpt, family):
    from mbrl_amd import fused
    for row in select_cases.rows(kpt, family):
        c = row.costs()
        ret = ocem.ensemble_returns(c)
        _, labels = sbm.select_model(ret, row.K, row.nan_policy, row.E)
        print("%s: %s" % (row.id, " ".join(sorted(labels))))
        costs = torch.from_numpy(c).to(DEV)

        # the select entry
        (el, r1), (el2, r2) = _select_twice(fused, costs, row)
        assert _returns_equal(r1, ret), row.id
        if row.nan_policy == sbm.NAN_FIRST:
            assert int(el[0]) == ocem.rs_argmin(ret), row.id
        else:
            ref_el = ocem.select_elites(ret, row.K)
            assert np.array_equal(el, ref_el), row.id
        assert _same_bytes(el, el2) and _same_bytes(r1, r2), row.id
        if row.nan_policy != sbm.NAN_LAST:
            continue                                      # mbrl_cem_update selects with NAN_LAST only

        # the update entry: inside _fused_k_cap it must run; beyond it, exactly where update_kpt() says
        first, second = _update_twice(fused, costs, row)
        if row.K > _fused_k_cap(row.N, 1) and not sbm.update_fits(row.N, row.K, 1):
            assert first is None and second is None, row.id
            continue
        assert first is not None and second is not None, row.id
        el, r1, mu1, sg1 = first
        assert _returns_equal(r1, ret), row.id
        assert np.array_equal(el, ref_el), row.id
        A = cem_actions(MU, SIGMA, -1.0, 1.0, SEED, ITERATION, ref_el)
        m2, s2 = ocem.refit(MU, SIGMA, np.ascontiguousarray(A.transpose(1, 0, 2)), ALPHA)
        assert np.array_equal(mu1, m2) and np.array_equal(sg1, s2), row.id
        assert all(_same_bytes(x, y) for x, y in zip(first, second)), row.id
