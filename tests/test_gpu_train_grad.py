"""GPU: mbrl_train_grads (csrc/train.hip) over the whole dispatch of launch_train_grads against the float64
gradient of tests/train_grad_reference.py, at the cases of tests/train_grad_cases.py.

tests/test_gpu_train_native.py compares with float32 autograd on the same GPU at a chosen tolerance, and
its bitwise tests show the layouts equal to each other, not that any of them is right. Here, for every
weight and bias gradient x of every case, under two metrics (train_grad_reference.err),

    tensor-relative  max |x - g64| / max |g64|
    tile-relative    max over the 32 x 32 tiles of  max |x - g64| in the tile / max |g64| in the tile

    e(gpu) <= bar(case, tensor) = 8 x max(e32 of that tensor, the table's median e32),

where e32 is the error of the same chain evaluated in float32 on the CPU: the bar is the float32
restatement's own distance to float64, never the kernel's. The three losses are held to the same
construction. tests/test_train_grad_host.py shows on the CPU that the table reaches every branch of the
dispatch, that no ReLU of a case can change side between the precisions, and that every single mistake of
a tiled backward pass misses these bars at least tenfold."""
import ctypes
import functools
from contextlib import ExitStack

import numpy as np
import pytest
import torch

import train_grad_cases as tc
import train_grad_reference as ref
from test_gpu_train_ensemble import (DEV, _assert_member_equal, _Data, _grads_ensemble, _grads_single, _Member,
                                     _single_epochs)

pytestmark = pytest.mark.gpu
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def cu_count():
    """The device's CU count (what launch_train_grads' tmx rule compares with); an MI355X's where there is
    no device, so that the module still collects."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else tc.MI355X_CUS


@functools.lru_cache(maxsize=None)
def device_data(name):
    c, p = tc.CASES[name], tc.problem(name)
    return _Data(c.s, c.a, c.H, p["T"], 0, arrays=p["data"])


def member(name, values=None, seed=0, aligned=False):
    """A member with the case's parameters (or `values`, or a seeded draw when values is False) under the
    case's alignment policy; gradients filled with NaN."""
    c, p = tc.CASES[name], tc.problem(name)
    n = 2 * (c.L + 1 + c.reward)
    off_p, off_g = {"aligned": ((), ()), "offset": (range(n), range(n)), "reward_w": ((2 * (c.L + 1),), ())}[
        "aligned" if aligned else c.align]
    mem = _Member(c.s, c.a, c.W, c.L, c.reward, c.H, seed, values=None if values is False else (values or p["params"]),
                  offset_params=off_p, offset_grads=off_g)
    for i in tc.misaligned(name) if not aligned else ():
        assert mem.params[2 * i].data_ptr() % 16 == 4
    for g in mem.grads:
        g.fill_(NAN)
    return mem


def status_word(mem, batch, ws):
    from mbrl_amd import _lib
    tm = _lib.TrainModel()
    mem.fill(tm)
    off = _lib.load().mbrl_train_status_offset(ctypes.byref(tm), batch)
    return int(ws[off:off + 4].view(torch.int32).item())


def run_grads(name, opts=()):
    """mbrl_train_grads on the case under the options: (loss [3], gradients, the status word), NumPy.
    Gradients and loss are NaN before the call."""
    from mbrl_amd import _lib
    p = tc.problem(name)
    mem = member(name)
    before = [q.clone() for q in mem.params]
    rows = torch.from_numpy(np.array(p["rows"])).to(DEV)
    kept = []
    with ExitStack() as stack:
        for opt, value in opts:
            stack.enter_context(_lib.option(opt, value))
        loss = _grads_single(mem, device_data(name), rows,
                             make_ws=lambda n: kept.append(torch.zeros(n, dtype=torch.uint8, device=DEV)) or kept[0],
                             alloc=lambda *sh: torch.full(sh, NAN, device=DEV))
        status = status_word(mem, len(p["rows"]), kept[0])
    assert all(torch.equal(x, y) for x, y in zip(mem.params, before)), "mbrl_train_grads wrote to the parameters"
    return loss.cpu().numpy(), [g.cpu().numpy() for g in mem.grads], status


@functools.lru_cache(maxsize=None)
def default_run(name):
    return run_grads(name)


def check_against_float64(name, loss, grads, what):
    """Print e(gpu), e32 and their ratio per tensor and metric, then hold every figure to its bar."""
    assert all(np.all(np.isfinite(g)) for g in grads) and np.all(np.isfinite(loss)), f"{name} {what}: not finite"
    e32, bars, med = tc.e32(name), tc.bars(name), tc.medians()
    failures = []
    for label, e, e0, b in zip(tc.tensor_names(name), tc.errors(name, grads), e32, bars):
        for k, metric in enumerate(("tensor", "tile")):
            print(f"RATIO {name} {what} {tc.tensor_kind(label)} {label} {metric}: e(gpu) {e[k]:.3e}, e32 {e0[k]:.3e}, "
                  f"ratio {e[k] / e0[k] if e0[k] else float('inf'):.2f}, of max(e32, median) {e[k] / max(e0[k], med[k]):.2f}, "
                  f"bar {b[k]:.3e}")
            if not e[k] <= b[k]:
                failures.append(f"{label} {metric}: e(gpu) = {e[k]:.3e} > bar = {b[k]:.3e}")
    l64 = tc.g64(name)["loss"]
    for label, e, e0, b in zip(("total", "state", "reward"), ref.loss_err(loss, l64), tc.e32_loss(name), tc.loss_bars(name)):
        print(f"RATIO {name} {what} loss loss_{label} rel: e(gpu) {e:.3e}, e32 {e0:.3e}, "
              f"ratio {e / e0 if e0 else float('inf'):.2f}, of max(e32, median) {e / max(e0, med[2]):.2f}, bar {b:.3e}")
        if not e <= b:
            failures.append(f"loss {label}: e(gpu) = {e:.3e} > bar = {b:.3e}")
    assert not failures, f"{name} {what}: " + "; ".join(failures)


@pytest.mark.parametrize("name", tc.NAMES)
def test_default_dispatch_matches_float64(name):
    loss, grads, status = default_run(name)
    assert status == 0, "a bounded in-launch wait timed out"
    check_against_float64(name, loss, grads, "default")


LAYOUT_RUNS = [(n, o, v) for n in tc.NAMES for o, v in tc.layouts_for(n, cu_count())]


@pytest.mark.parametrize("name,opt,value", LAYOUT_RUNS)
def test_forced_layout_is_bitwise_the_default(name, opt, value):
    """Every case under every forced layout that changes its dispatch key (train_grad_cases.layouts_for:
    the others would pass vacuously and are left out): byte-equal to the default run."""
    assert tc.dispatch(name, cu_count(), {opt: value}) != tc.dispatch(name, cu_count())
    loss, grads, status = run_grads(name, ((opt, value),))
    loss0, grads0, _ = default_run(name)
    assert status == 0
    assert all(np.all(np.isfinite(g)) for g in grads)
    assert loss.tobytes() == loss0.tobytes(), (loss, loss0)
    for label, x, y in zip(tc.tensor_names(name), grads, grads0):
        assert x.tobytes() == y.tobytes(), (label, float(np.max(np.abs(x - y))))


def test_forced_layouts_cover_every_option():
    assert {(o, v) for _, o, v in LAYOUT_RUNS} == set(tc.LAYOUTS)


@pytest.mark.parametrize("name", tc.ENSEMBLE_CASES)
def test_ensemble_is_bitwise_each_member_alone(name):
    """mbrl_train_grads_ensemble with E = 2, other rows and other parameters for the second member:
    byte-equal to mbrl_train_grads per member, and the case's member within its float64 bars. In the
    alignment cases the misaligned member's partner has aligned tensors, in either order: with the aligned
    one first, direct() chooses float4 loads and the launcher takes them back for all members."""
    p = tc.problem(name)
    idx = np.stack([p["rows"], tc.other_rows(name)])
    for flip in ((False, True) if tc.CASES[name].align != "aligned" else (False,)):
        mems = [member(name), member(name, values=False, seed=77, aligned=True)]
        order = [1, 0] if flip else [0, 1]
        mems, rows = [mems[i] for i in order], np.ascontiguousarray(idx[order])
        clones = [m.clone() for m in mems]
        didx = torch.from_numpy(rows).to(DEV)
        loss = _grads_ensemble(mems, device_data(name), didx, alloc=lambda *sh: torch.full(sh, NAN, device=DEV))
        for e, c in enumerate(clones):
            l1 = _grads_single(c, device_data(name), didx[e], alloc=lambda *sh: torch.full(sh, NAN, device=DEV))
            _assert_member_equal(mems[e], c, f"{name} flip {flip} member {e}")
            assert torch.equal(loss[e], l1), (e, loss[e], l1)
            assert all(bool(torch.isfinite(g).all()) for g in mems[e].grads)
        e = order.index(0)
        check_against_float64(name, loss[e].cpu().numpy(), [g.cpu().numpy() for g in mems[e].grads], f"ensemble{int(flip)}")


def test_epochs_at_the_wide_input_fold_are_bitwise_the_separate_launch():
    """mbrl_train_epoch with the in-launch Adam table at s + a = 70 > FOLD_K0MAX: batches of 100, 100 and
    37 rows (the fold with its input read from memory and fold_sum's Adam step, then a short batch without
    the fold), three epochs. Parameters, Adam state, last gradients and every loss are bit for bit what
    train_no_fold = 1 gives."""
    from mbrl_amd import _lib
    s, a, W, L, H, batch, rows, epochs = 50, 20, 64, 3, 1, 100, 237, 3
    assert tc.train_dispatch(s, a, W, L, 0, H, batch, cu_count()).fold_input == "global"
    assert tc.train_dispatch(s, a, W, L, 0, H, rows % batch, cu_count()).fold_nw == 0
    data = _Data(s, a, H, rows, seed=11)
    orders = np.stack([np.random.default_rng(k).permutation(rows) for k in range(epochs)]).astype(np.int64)
    start = _Member(s, a, W, L, 0, H, seed=5)
    out = {}
    for no_fold in (0, 1):
        mem = start.clone()
        kept = []
        with _lib.option("train_no_fold", no_fold):
            losses = _single_epochs(mem, data, orders, batch,
                                    make_ws=lambda n: kept.append(torch.zeros(n, dtype=torch.uint8, device=DEV)) or kept[0])
            assert status_word(mem, batch, kept[0]) == 0
        assert bool(torch.isfinite(losses).all()) and losses.shape == (epochs, 3, 3)
        out[no_fold] = (mem, losses)
    _assert_member_equal(out[0][0], out[1][0], "fold vs no fold")
    assert torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][0].params[0], start.params[0])            # it did train
    assert float(out[0][1][-1, 0, 0]) < float(out[0][1][0, 0, 0])             # and the loss went down
