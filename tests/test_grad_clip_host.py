"""The gradient-clipping order on the CPU: tests/grad_clip_reference.py (the NumPy fp32 restatement the GPU tests hold
mbrl_grad_norm to bit for bit) against float64 and torch.nn.utils.clip_grad_norm_ at a bar derived from the order,
the coefficient rules, and single-mistake mutants that the bar or the byte comparison must catch."""
import numpy as np
import pytest
import torch

import grad_clip_reference as ref

F = np.float32


def _finite(name):
    return "plant" not in ref.CASES[name]


def _bits(x):
    return np.asarray(x, F).view(np.int32)


@pytest.mark.parametrize("name", ref.NAMES)
def test_norm_is_within_the_derived_bar_of_float64(name):
    for e, grads in enumerate(ref.gradients(name)):
        got, want = float(ref.norm(grads)), ref.norm64(grads)
        bar = ref.norm_bar(ref.CASES[name]["members"][e])
        if not np.isfinite(want):
            assert not np.isfinite(got)
            continue
        print(f"{name} member {e}: norm {got:.9g}  float64 {want:.9g}  rel {abs(got - want) / max(want, 1e-300):.3e}"
              f"  bar {bar:.3e}")
        assert abs(got - want) <= bar * want, (name, e, got, want, bar)


def test_the_bar_comes_from_the_order():
    """3 + 8 + 10 dependent additions and the square's rounding below 1024 partials; one more addition per further
    1024 partials in a finishing lane."""
    assert ref.norm_bar([1]) == 0.5 * 22 * ref.U + ref.U
    assert ref.norm_bar([ref.BIG]) == ref.norm_bar([1])                      # P = 1024: one partial per lane
    assert ref.norm_bar([ref.BIG, 3]) == 0.5 * 23 * ref.U + ref.U            # P = 1025: lane 0 adds two
    assert ref.norm_bar([0, 0]) == ref.norm_bar([1])


@pytest.mark.parametrize("name", ref.NAMES)
def test_agrees_with_torch_clip_grad_norm(name):
    """The returned norm and the scaled gradients of torch.nn.utils.clip_grad_norm_ on the CPU, within the bar.
    torch runs on float64 copies of the gradients: its own fp32 sum over the 2^20 elements of p1024 is 1.3e-5 off
    float64, 18 bars, where the restatement is 3e-8 off -- the bar is the order's, not torch's summation's."""
    max_norm = ref.CASES[name]["max_norm"]
    for e, grads in enumerate(ref.gradients(name)):
        ps = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in grads]
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g.astype(np.float64))
        tn = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        nrm = ref.norm(grads)
        c = ref.coef(nrm, max_norm)
        bar = ref.norm_bar(ref.CASES[name]["members"][e])
        if not np.isfinite(tn):
            # a NaN gradient: NaN norm, NaN coef, every element NaN. An inf one under a finite max_norm: inf norm,
            # coef = max_norm / inf = 0, so inf * 0 = NaN where the inf was and 0 elsewhere -- in torch and here
            assert np.isnan(float(nrm)) == np.isnan(tn) and not np.isfinite(float(nrm))
            for p, g in zip(ps, ref.scaled(grads, c)):
                assert np.array_equal(g, p.grad.numpy().astype(F), equal_nan=True), (name, e)
            continue
        assert abs(float(nrm) - tn) <= bar * tn, (name, e, float(nrm), tn)
        worst = 0.0
        for p, g in zip(ps, ref.scaled(grads, c)):
            t = p.grad.numpy()
            if t.size:
                worst = max(worst, float(np.max(np.abs(g - t) / np.maximum(np.abs(t), 1e-300))))
            assert np.all(np.abs(g - t) <= bar * np.abs(t)), (name, e, worst)
        print(f"{name} member {e}: norm rel {abs(float(nrm) - tn) / max(tn, 1e-300):.3e}  gradients rel {worst:.3e}"
              f"  bar {bar:.3e}")


def test_coefficient_rules():
    g = ref.gradients("seams")
    n1 = ref.norm(g[1])
    assert float(n1) < 2.0 and _bits(ref.coef(n1, 2.0)) == _bits(1.0)                  # within bounds: exactly 1
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ref.scaled(g[1], ref.coef(n1, 2.0)), g[1]))
    n0 = ref.norm(g[0])
    assert float(n0) > 2.0 and 0 < float(ref.coef(n0, 2.0)) < 1                        # beyond: it clips
    z = ref.gradients("zero")[0]
    assert float(ref.norm(z)) == 0.0 and _bits(ref.coef(ref.norm(z), 1.0)) == _bits(1.0)
    for grads in ref.gradients("inf_norm"):
        assert _bits(ref.coef(ref.norm(grads), float("inf"))) == _bits(1.0)            # +inf never clips
    assert np.isnan(ref.coef(ref.norm(ref.gradients("nan")[1]), 1.0))
    # an inf gradient: inf / inf = NaN under max_norm = +inf; under a finite max_norm q = max_norm / inf = 0, as in
    # torch, and the member's step then sees inf * 0 = NaN where the inf was
    bad = ref.gradients("inf")[0]
    assert np.isinf(ref.norm(bad)) and np.isnan(ref.coef(ref.norm(bad), float("inf")))
    assert _bits(ref.coef(ref.norm(bad), 1.0)) == _bits(0.0)
    assert any(bool(np.isnan(g).any()) for g in ref.scaled(bad, ref.coef(ref.norm(bad), 1.0)))
    assert _bits(ref.coef(ref.norm(ref.gradients("nan")[0]), 1.0)) != _bits(float("nan"))   # its neighbour is finite


# ---- single-mistake mutants: each misses the bar or the byte comparison somewhere in the table
def _norm_of(partials):
    with np.errstate(all="ignore"):
        return F(np.sqrt(ref.reduce_partials(partials)))


def _misses_bar(name, e, got):
    grads = ref.gradients(name)[e]
    want = ref.norm64(grads)
    return abs(float(got) - want) > ref.norm_bar(ref.CASES[name]["members"][e]) * want


def _finite_members():
    return [(name, e) for name in ref.NAMES if _finite(name) for e in range(len(ref.CASES[name]["members"]))]


def test_mutant_padding_read_as_garbage():
    hit = [(n, e) for n, e in _finite_members()
           if _misses_bar(n, e, _norm_of(np.concatenate([ref.chunk_partials(g, pad=1e-3) for g in ref.gradients(n)[e]])))]
    assert hit, "garbage in the padding went unnoticed"


def test_mutant_one_tensors_partials_dropped():
    hit = []
    for n, e in _finite_members():
        grads = [g for g in ref.gradients(n)[e] if g.size]
        if len(grads) > 1 and _misses_bar(n, e, _norm_of(ref.member_partials(grads[:-1]))):
            hit.append((n, e))
    assert hit


def test_mutant_norm_per_tensor():
    hit = []
    for n, e in _finite_members():
        grads, max_norm = ref.gradients(n)[e], ref.CASES[n]["max_norm"]
        want = ref.scaled(grads, ref.coef(ref.norm(grads), max_norm))
        got = [ref.scaled([g], ref.coef(ref.norm([g]), max_norm))[0] for g in grads]
        if any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want)):
            hit.append((n, e))
    assert hit


def test_mutant_eps_left_out():
    hit = [(n, e) for n, e in _finite_members()
           if _bits(ref.coef(ref.norm(ref.gradients(n)[e]), ref.CASES[n]["max_norm"], eps=F(0.0))) !=
           _bits(ref.coef(ref.norm(ref.gradients(n)[e]), ref.CASES[n]["max_norm"]))]
    assert ("tiny", 0) in hit


def test_mutant_coef_after_weight_decay():
    """Scaling g + wd * p in place of g: another step wherever the member clips and weight decay is on."""
    name, e, wd = "e1", 0, 1e-2
    grads = ref.gradients(name)[e]
    rng = np.random.default_rng(5)
    params = [rng.standard_normal(g.shape).astype(F) for g in grads]
    m = [np.zeros_like(g) for g in grads]
    v = [np.zeros_like(g) for g in grads]
    nrm, c, want = ref.clipped_step(params, grads, m, v, 1, ref.CASES[name]["max_norm"], weight_decay=wd)
    assert 0 < float(c) < 1
    late = [(g + F(wd) * p) * c for g, p in zip(grads, params)]
    got = ref.adam_step(params, late, m, v, 1)
    assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[0], want[0]))
    same = ref.adam_step(params, ref.scaled(grads, c), m, v, 1, weight_decay=wd)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(same[0], want[0]))


def test_mutant_members_coefficients_swapped():
    hit = []
    for name in ref.NAMES:
        if not _finite(name) or len(ref.CASES[name]["members"]) < 2:
            continue
        coefs = [ref.coef(ref.norm(g), ref.CASES[name]["max_norm"]) for g in ref.gradients(name)]
        if _bits(coefs[0]) != _bits(coefs[1]):
            hit.append(name)
    assert "seams" in hit and "e5" in hit
