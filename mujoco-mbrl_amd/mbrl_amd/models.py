"""Dynamics models and costs with the reference's API (/root/reference/src/mbrl/models.py).

`DynamicsModel.forward(state, action, normalize_action=None, normalize_state=None,
unnormalize_state=None)` keeps the reference contract (models.py:13-29). On CUDA tensors with
autograd off it runs the one-step batch through the same HIP rollout kernel the planners use
(H = 1, per-row start states); otherwise (training, CPU tensors) it is plain PyTorch, exactly the
reference's arithmetic.
"""
import contextlib
import ctypes
import functools
import threading
import weakref

import numpy as np
import torch
import torch.nn as nn

from .optim import AdamStep


def _epoch_order(dataset):
    """The row order DataLoader(dataset, batch_size, sampler=TransitionsSampler(dataset)) visits
    (models.py:61-63), as an int64 array of row indices into dataset.stacked().

    TransitionsSampler (data.py:271-285) np.random.shuffle()s the list of (rollout, start) pairs.
    NumPy's legacy shuffle draws j = random_interval(i) for i = n-1 .. 1 and swaps x[i], x[j] on
    every path (the list path and the 1-D array path alike), so shuffling arange(n) in place yields
    the same permutation of positions and leaves the global RNG in the same state -- without
    building and hashing n tuples per epoch (16 ms for 10k transitions, more than the GPU's
    20 training steps of that epoch)."""
    order = np.arange(dataset.num_transitions(), dtype=np.int64)
    np.random.shuffle(order)
    return order


def _epoch_batches(dataset, batch_size):
    """_epoch_order split into the DataLoader's batches (the last one may be short)."""
    order = _epoch_order(dataset)
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def _device_of(module):
    return next(module.parameters()).device


def _batch_loss(dataset, ins, outs, idx, step_loss, n_parts):
    bi = [x.index_select(0, idx) for x in ins]
    bo = [x.index_select(0, idx) for x in outs]
    loss, parts = 0, [0] * n_parts
    for h in range(dataset.horizon):
        for k, term in enumerate(step_loss([x[:, h] for x in bi], [x[:, h] for x in bo])):
            parts[k] = parts[k] + term
            loss = loss + term
    return loss, parts


class _GraphStep:
    """A full-size batch's zero_grad + gather + forward + loss + backward captured once in a HIP
    graph (through torch.cuda.CUDAGraph) and replayed per batch; optimizer.step() stays outside the
    graph so any optimizer works unchanged. The warm-up before capture only touches .grad (zeroed
    after), never the parameters, so training follows exactly the eager sequence of updates."""

    def __init__(self, model, dataset, ins, outs, batch_size, step_loss, n_parts):
        dev = _device_of(model)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.idx = torch.zeros(batch_size, dtype=torch.long, device=dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                loss, _ = _batch_loss(dataset, ins, outs, self.idx, step_loss, n_parts)
                loss.backward()
            del loss                      # drop the warm-up autograd graph before capturing
        torch.cuda.current_stream(dev).wait_stream(side)
        grads = [p.grad for p in self.params if p.grad is not None]
        if grads:
            torch._foreach_zero_(grads)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            if grads:                     # zero_grad() as the graph's first node: backward accumulates
                torch._foreach_zero_(grads)
            self.loss, self.parts = _batch_loss(dataset, ins, outs, self.idx, step_loss, n_parts)
            self.loss.backward()
        # the replay accumulates into exactly these tensors; an eager step in between (the last,
        # partial batch: optimizer.zero_grad() sets .grad to None) must not orphan them
        self.grads = [p.grad for p in self.params]

    def run(self, rows):
        self.idx.copy_(rows)
        for p, g in zip(self.params, self.grads):
            p.grad = g
        self.graph.replay()
        return self.loss, self.parts


# train_model's device path for the reference's MLP models under the default MSELoss: the batch
# gradient from mbrl_train_grads (csrc/train.hip) instead of autograd. False: autograd in a HIP graph.
NATIVE_TRAINING = True

# model -> (binding key, _NativeGrads) of its last native train_model call (_NativeGrads.cached)
_NATIVE_CACHE = weakref.WeakKeyDictionary()
# ensemble -> (binding key, _NativeEnsemble) of its last native train_members call
_NATIVE_ENS_CACHE = weakref.WeakKeyDictionary()

_LIB_OVERRIDE = None


@contextlib.contextmanager
def native_library(lib):
    """Within the block, train_model / train_members bind their native training calls to `lib`
    (_lib.load_other: another build of the extension with the same structs) instead of the loaded
    library -- the A/B hook of tools/train_ensemble_bench.py. Objects cached for one library are not
    reused for another."""
    global _LIB_OVERRIDE
    saved, _LIB_OVERRIDE = _LIB_OVERRIDE, lib
    try:
        yield
    finally:
        _LIB_OVERRIDE = saved


def _native_lib():
    from . import _lib
    return _LIB_OVERRIDE if _LIB_OVERRIDE is not None else _lib.load()


class _NativeGrads:
    """mbrl_train_grads for Model (noise None) / ModelWithReward with MSELoss(reduction='mean'):
    per batch, one C call that gathers the batch, runs the forward pass and the loss gradient, and
    overwrites every Linear's .grad (what zero_grad + backward leave). The loss values come back
    as device scalars (total, state, reward) for the writer."""

    def __init__(self, model, ins, outs, horizon, batch_size, reward):
        from . import _lib
        self.lib = _native_lib()
        dev = _device_of(model)
        lins = model.linears()
        self.params = [t for lin in lins for t in (lin.weight, lin.bias)]
        self.grads = [torch.zeros_like(t) for t in self.params]
        m = _lib.TrainModel()
        m.state_dim, m.action_dim, m.hidden = model.state_dim, model.action_dim, model.hidden_units
        m.n_hidden, m.reward_head, m.horizon = model.n_hidden, int(reward), int(horizon)
        for i, lin in enumerate(lins):
            m.weight[i], m.bias[i] = lin.weight.data_ptr(), lin.bias.data_ptr()
            m.weight_grad[i], m.bias_grad[i] = self.grads[2 * i].data_ptr(), self.grads[2 * i + 1].data_ptr()
        (states, actions), (rewards, next_states) = ins, outs
        self.keep = [x.contiguous() for x in (states, actions, next_states, rewards)]
        d = _lib.TrainData()
        d.states, d.actions, d.next_states, d.rewards = [x.data_ptr() for x in self.keep]
        d.transitions = states.shape[0]
        self.model, self.data = m, d
        need = self.lib.mbrl_train_workspace_bytes(ctypes.byref(m), int(batch_size))
        if need == 0:
            _lib.check(-1, "mbrl_train_workspace_bytes")
        # zeroed once: the fused step's sticky status word lives in it (mbrl_train_status_offset)
        self.ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        self.status_at = int(self.lib.mbrl_train_status_offset(ctypes.byref(m), int(batch_size)))
        self.loss = torch.zeros(3, dtype=torch.float32, device=dev)
        self.ptrs = [t.data_ptr() for t in self.params]
        self.dev = dev
        self._lib = _lib

    @classmethod
    def cached(cls, model, ins, outs, horizon, batch_size, reward):
        """The object of the model's previous train_model call when nothing it binds has changed (the
        parameter and gradient storage, the stacked transitions, the batch size), else a new one. A
        call then starts its first launch without allocating and zeroing the gradients and the
        workspace (host time the GPU idles through at the start of every call,
        tools/train_startup.py). Rebuilt when a non-contiguous input would need a fresh contiguous
        copy."""
        key = (str(_device_of(model)), int(horizon), int(batch_size), bool(reward), id(_LIB_OVERRIDE),
               tuple(t.data_ptr() for lin in model.linears() for t in (lin.weight, lin.bias)),
               tuple((x.data_ptr(), tuple(x.shape), x.is_contiguous()) for x in (*ins, *outs)))
        hit = _NATIVE_CACHE.get(model)
        if hit is not None and hit[0] == key:
            return hit[1]
        obj = cls(model, ins, outs, horizon, batch_size, reward)
        if all(x.is_contiguous() for x in (*ins, *outs)):
            _NATIVE_CACHE[model] = (key, obj)
        else:
            _NATIVE_CACHE.pop(model, None)
        return obj

    @staticmethod
    def forget(model):
        """Drop the model's cached object (after a failed status check: its sticky word is set)."""
        _NATIVE_CACHE.pop(model, None)

    @staticmethod
    def supported(model, dataset, ins, outs, criterion, probabilistic=False):
        """False / True (the reward head) when the native entries take the model, else None. probabilistic: the
        caller's entry reads a ProbabilisticModel (the NLL entries its whole head, the evaluation its mean rows)."""
        if not NATIVE_TRAINING or type(criterion) is not torch.nn.MSELoss or criterion.reduction != "mean":
            return None
        if type(model) is Model:
            if model.noise is not None:
                return None
            reward = False
        elif type(model) is ProbabilisticModel and probabilistic:
            reward = False
        elif type(model) is ModelWithReward:
            reward = True
        else:
            return None
        if model.n_hidden < 1 or model.n_hidden + 2 > 10 or len(ins) != 2 or len(outs) != 2:
            return None
        # train.hip computes Linear-ReLU chains and never calls the module: a replaced activation or
        # a hook would make it train a different function than the model computes
        if type(model.activation_fn) is not nn.ReLU or any(
                m._forward_hooks or m._forward_pre_hooks or m._backward_hooks for m in model.modules()):
            return None
        params = list(model.parameters())
        if len(params) != 2 * len(model.linears()):
            return None
        if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.requires_grad for p in params):
            return None
        (states, actions), (rewards, next_states) = ins, outs
        T, H = states.shape[0], dataset.horizon
        want = [(states, model.state_dim), (actions, model.action_dim), (next_states, model.state_dim)]
        if any(tuple(x.shape) != (T, H, w) or x.dtype != torch.float32 for x, w in want):
            return None
        if rewards.numel() != T * H:
            return None
        return reward

    def epoch(self, order, batch_size, adam):
        """One epoch over the device row order `order`: every batch's gradient and Adam step from one
        mbrl_train_epoch call. Returns the per-batch losses [batches, 3] (device), or None when the
        optimizer's state does not allow it (the caller then steps per batch)."""
        for p, g in zip(self.params, self.grads):
            if p.grad is not g:
                p.grad = g
        if [p.data_ptr() for p in self.params] != self.ptrs:
            raise RuntimeError("model parameters moved during training")
        rows = int(order.shape[0])
        steps = (rows + batch_size - 1) // batch_size
        plan = adam.epoch_plan(self.params, steps)
        if plan is None:
            return None
        table, hp, ss, bc = plan
        losses = torch.empty((steps, 3), dtype=torch.float32, device=self.dev)
        self._lib.check(self.lib.mbrl_train_epoch(ctypes.byref(self.model), ctypes.byref(self.data),
                                                  ctypes.c_void_p(order.data_ptr()), rows, int(batch_size), table,
                                                  len(self.params), ctypes.byref(hp), ss, bc,
                                                  ctypes.c_void_p(losses.data_ptr()),
                                                  ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(),
                                                  self._lib.stream_handle(self.dev)), "mbrl_train_epoch")
        adam.epoch_done(self.params)
        return losses

    def check_status(self):
        """Raise if an in-launch wait of the fused step timed out (the workgroup dispatch order its
        Adam placement relies on was not kept): the parameters may then be off. Never expected. The
        word is sticky (set by any launch since the workspace was zeroed), so one read after the last
        epoch of a train_model call covers every epoch of it: no per-epoch copy or kernel."""
        word = int(self.ws[self.status_at:self.status_at + 4].view(torch.int32).item())
        if word & 1:
            raise RuntimeError("mbrl_amd: a fused training step's bounded wait timed out (status word "
                               f"{word:#x}); the parameters of that step may be wrong")

    def run(self, idx):
        """The batch gradient for the rows `idx` (int64, on the device) into p.grad."""
        for p, g in zip(self.params, self.grads):
            if p.grad is not g:
                p.grad = g
        if [p.data_ptr() for p in self.params] != self.ptrs:
            raise RuntimeError("model parameters moved during training")
        self._lib.check(self.lib.mbrl_train_grads(ctypes.byref(self.model), ctypes.byref(self.data),
                                                  ctypes.c_void_p(idx.data_ptr()), int(idx.shape[0]),
                                                  ctypes.c_void_p(self.loss.data_ptr()),
                                                  ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(),
                                                  self._lib.stream_handle(self.dev)), "mbrl_train_grads")
        loss = self.loss.clone()          # the buffer is reused by the next batch; the writer keeps these
        return loss[0], [loss[1], loss[2]]


def _train_loop(model, dataset, optimizer, batch_size, num_epochs, step_loss, writer, tags, criterion=None,
                order_fn=None, iter0=0, max_grad_norm=None, norm_tag=None):
    """models.py:53-93 / 165-217 on the model's device: per batch, the loss summed over the horizon
    steps, zero_grad, backward, step -- the reference's order of operations. Batches are gathered
    from device-resident transitions (TransitionsDataset.stacked) instead of per-sample collation;
    on a GPU the full-size batches replay one captured graph (_GraphStep), and a plain Adam steps
    through mbrl_adam_step (optim.AdamStep: one launch, torch's arithmetic bit for bit).
    order_fn (EnsembleModel.train_members): epoch k visits the rows order_fn(k) instead of a shuffle
    drawn from the global RNG, batch by batch (no whole-epoch device call: its order ring draws), and
    the writer's batch index goes on from iter0 (the batches a shared-launch part of the call ran).
    max_grad_norm (train_members): torch.nn.utils.clip_grad_norm_ over the model's parameters between the
    gradient and the step, batch by batch; the writer gets the pre-clip norm under norm_tag."""
    dev = _device_of(model)
    if dev.type == "cuda":
        with torch.cuda.device(dev):       # launches and workspaces on the model's GPU
            return _train_loop_on(dev, model, dataset, optimizer, batch_size, num_epochs, step_loss, writer, tags,
                                  criterion, order_fn, iter0, max_grad_norm, norm_tag)
    return _train_loop_on(dev, model, dataset, optimizer, batch_size, num_epochs, step_loss, writer, tags, criterion,
                          order_fn, iter0, max_grad_norm, norm_tag)


def _train_loop_on(dev, model, dataset, optimizer, batch_size, num_epochs, step_loss, writer, tags, criterion,
                   order_fn=None, iter0=0, max_grad_norm=None, norm_tag=None):
    if dataset.num_transitions() == 0:    # the reference's DataLoader yields no batch
        model.train_iterations += 1
        return
    _, ins, outs = dataset.stacked(dev)
    n_parts = len(tags)
    graph = native = None
    if dev.type == "cuda":
        reward = _NativeGrads.supported(model, dataset, ins, outs, criterion)
        if reward is not None:
            native = _NativeGrads.cached(model, ins, outs, dataset.horizon, batch_size, reward)
    if native is None and dev.type == "cuda" and dataset.num_transitions() >= batch_size:
        try:
            graph = _GraphStep(model, dataset, ins, outs, batch_size, step_loss, n_parts)
        except RuntimeError:           # capture unsupported for this model / criterion: stay eager
            graph = None
            for p in model.parameters():
                p.grad = None
    fast = AdamStep.maybe(optimizer) if dev.type == "cuda" else None
    # parameters the optimizer steps that the native gradient call does not overwrite each batch
    own = set() if native is None else {id(p) for p in native.params}
    extra = [p for g in optimizer.param_groups for p in g["params"] if id(p) not in own] if native is not None else []
    num_iters = iter0
    whole = native is not None and fast is not None and order_fn is None and max_grad_norm is None
    if whole and num_epochs > 0:
        # The device path issues the epochs back to back with no host round trip between them (a
        # per-epoch copy of the row order from pageable memory waited for the previous epoch to drain).
        # Epoch k + 1's order is drawn while epoch k runs -- the same np.random draws in the same order
        # (nothing else in this loop draws from the global RNG) -- into a ring of pinned rows and copied
        # on a side stream that the training stream waits on before epoch k + 1 (the copy lands while
        # epoch k computes). The sticky status word is read once, after the last epoch.
        ring = _order_ring(dev, dataset.num_transitions())
        main = torch.cuda.current_stream(dev)
        ring.draw(0)
        ring.copy(0, main)
    epoch_losses = []
    for ep in range(num_epochs):
        if whole:
            host, order = ring.rows(ep)
            if ep >= 1:
                ring.copied[ep % ring.K].wait(main)   # epoch ep's order has landed
        else:
            host = _epoch_order(dataset) if order_fn is None else order_fn(ep)
            order = torch.from_numpy(host).to(dev)
        losses = native.epoch(order, batch_size, fast) if whole else None
        if whole and ep + 1 < num_epochs:
            ring.draw(ep + 1)
            ring.copy(ep + 1, ring.side)
        if losses is not None:            # the whole epoch in one call; the writer gets its values after
            ring.consumed[ep % ring.K].record(main)   # the ring row is free once this epoch has run
            epoch_losses.append(losses)
            continue
        num_iters = _write_epoch_losses(epoch_losses, writer, tags, n_parts, model, num_iters)
        epoch_losses = []
        for i in range(0, len(host), batch_size):
            idx = order[i:i + batch_size]
            if native is not None:
                for p in extra:               # optimizer.zero_grad() for what the native call does not write
                    p.grad = None
                loss, parts = native.run(idx)
                parts = parts[:n_parts]
            elif graph is not None and idx.shape[0] == batch_size:
                loss, parts = graph.run(idx)
            else:
                optimizer.zero_grad()
                loss, parts = _batch_loss(dataset, ins, outs, idx, step_loss, n_parts)
                loss.backward(retain_graph=True)
            if max_grad_norm is not None:
                norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
            if fast is None or not fast.step():
                optimizer.step()
            num_iters += 1
            if writer is not None and max_grad_norm is not None and norm_tag is not None:
                writer.add_scalar(norm_tag.format(model.train_iterations), norm, num_iters)
            if writer is not None:
                for tag, val in zip(tags, parts if n_parts > 1 else [loss]):
                    writer.add_scalar(tag.format(model.train_iterations), val, num_iters)
                if n_parts > 1:
                    writer.add_scalar("loss/total/{}".format(model.train_iterations), loss, num_iters)
        if whole:
            ring.consumed[ep % ring.K].record(torch.cuda.current_stream(dev))
    num_iters = _write_epoch_losses(epoch_losses, writer, tags, n_parts, model, num_iters)
    if graph is not None:
        for p in model.parameters():      # release the graph-pool grads; the eager path re-allocates
            p.grad = None
    # (the native path leaves the last batch's gradients in .grad, as the reference's loop does)
    try:
        if native is not None:
            native.check_status()
    except RuntimeError:
        _NativeGrads.forget(model)        # the workspace's sticky status word is set: start afresh
        raise
    model.train_iterations += 1


class _OrderRing:
    """K pinned host rows and K device rows of n row indices, a copy stream and per-row events, reused
    by every train_model call on datasets of n transitions: epoch e's order lives in row e % K. The
    host draws into a pinned row only once the copy that last read it has finished (`copied`), and
    enqueues the copy into a device row only once the epoch that last read it has run (`consumed`),
    so the host may run up to ~K epochs ahead -- ~17 ms of 2x512 training at K = 16,
    room for a garbage-collector pause of the host thread -- and no call allocates (a pinned
    allocation costs milliseconds, a new stream's first use ~6 ms of queue set-up). Rows hold
    `cap` indices, n rounded up to a power of two, and an epoch uses the first n: the dataset of an
    MBRL loop grows every episode, and it reuses one ring until it doubles. K shrinks with the
    capacity (16 rows up to 131k, 4 from 524k on: a longer epoch is a longer lead), so the ring
    holds at most 16 MB of pinned memory up to 524k indices and 4 rows beyond."""

    def __init__(self, dev, cap):
        self.cap = cap
        self.n = cap
        self.K = max(4, min(16, (1 << 21) // max(cap, 1)))
        self.pinned = torch.empty((self.K, cap), dtype=torch.int64, pin_memory=True)
        self.host = self.pinned.numpy()
        self.arange = np.arange(cap, dtype=np.int64)
        self.dev = torch.empty((self.K, cap), dtype=torch.int64, device=dev)
        self.side = torch.cuda.Stream(dev)
        with torch.cuda.stream(self.side):          # set up the side stream's queue here, once
            self.dev[:1].copy_(self.pinned[:1], non_blocking=True)
        self.side.synchronize()
        from . import _lib
        self.copied = [_lib.StreamEvent() for _ in range(self.K)]      # fence-free: a torch.cuda.Event
        self.consumed = [_lib.StreamEvent() for _ in range(self.K)]    # record idles the GPU ~5.5 us
        # a host wait on an event that is still pending takes a slow first-use path (~2 ms, measured
        # on the first long train_model call of a process, tools/train_after_load.py): take it here
        for r in range(self.K):
            with torch.cuda.stream(self.side):
                self.dev[r].copy_(self.pinned[r], non_blocking=True)
                self.copied[r].record(self.side)
            self.copied[r].synchronize()

    def draw(self, e, fill=None):
        """Epoch e's order (models._epoch_order's draws: NumPy's shuffle of arange(n), in place), or
        what fill(row) writes into the pinned row (train_members: the members' orders, end to end)."""
        r = e % self.K
        self.copied[r].synchronize()                # the copy that last read this pinned row is done
        row = self.host[r, :self.n]
        if fill is not None:
            fill(row)
            return
        np.copyto(row, self.arange[:self.n])
        np.random.shuffle(row)                      # (in place on the view: the draws of a fresh arange(n))

    def copy(self, e, stream):
        r = e % self.K
        # the epoch that last read this device row must have run: the host checks (it is K epochs
        # back, so this rarely waits) -- a wait of the side stream on the training stream's event cost
        # the training stream 20-45 us per epoch (tools/train_epoch_plumbing.py)
        self.consumed[r].synchronize()              # (an event never recorded is complete)
        with torch.cuda.stream(stream):
            self.dev[r, :self.n].copy_(self.pinned[r, :self.n], non_blocking=True)
            self.copied[r].record(stream)

    def rows(self, e):
        r = e % self.K
        return self.host[r, :self.n], self.dev[r, :self.n]


_ORDER_RINGS = {}


def _order_ring(dev, n):
    # one ring per thread: two threads training at once must not share pinned rows
    cap = 1 << max(10, (max(n, 1) - 1).bit_length())
    key = (str(dev), cap, threading.get_ident())
    ring = _ORDER_RINGS.get(key)
    if ring is None:
        if len(_ORDER_RINGS) > 8:
            _ORDER_RINGS.clear()
        ring = _ORDER_RINGS[key] = _OrderRing(dev, cap)
    ring.n = n                  # (the previous call's epochs were all enqueued before this one draws)
    return ring


def _write_epoch_losses(epoch_losses, writer, tags, n_parts, model, num_iters):
    """The writer's per-batch values of whole-epoch device calls (in batch order), after the epochs ran."""
    for losses in epoch_losses:
        if writer is None:
            num_iters += losses.shape[0]
            continue
        for row in losses.cpu().tolist():
            num_iters += 1
            parts = [row[1], row[2]][:n_parts]
            for tag, val in zip(tags, parts if n_parts > 1 else [row[0]]):
                writer.add_scalar(tag.format(model.train_iterations), val, num_iters)
            if n_parts > 1:
                writer.add_scalar("loss/total/{}".format(model.train_iterations), row[0], num_iters)
    return num_iters


class DynamicsModel(nn.Module):
    """models.py:8-93."""

    def __init__(self):
        super().__init__()
        self.train_iterations = 0

    def train_model(self, dataset, optimizer, batch_size=512, num_epochs=50, criterion=None, writer=None):
        """models.py:53-93 (state_only / obs_only data modes: inputs (s, a), outputs (r, s')). On an
        EnsembleModel this fits the member mean; EnsembleModel.train_members trains each member on its
        own bootstrap order."""
        criterion = criterion or torch.nn.MSELoss()

        def step_loss(inp, out):
            (states, actions), (_, next_states) = inp, out
            return [criterion(self.forward(states, actions, normalize_action=None, normalize_state=None,
                                           unnormalize_state=None), next_states)]
        _train_loop(self, dataset, optimizer, batch_size, num_epochs, step_loss, writer, ["loss/state/{}"],
                    criterion)

    def evaluate_model(self, dataset, batch_size, criterion=None):
        """models.py:30-51: one criterion value per batch and horizon step."""
        criterion = criterion or torch.nn.MSELoss()
        dev = _device_of(self)
        if dataset.num_transitions() == 0:
            return []
        _, ins, outs = dataset.stacked(dev)
        evals = []
        with torch.no_grad():
            for rows in _epoch_batches(dataset, batch_size):
                idx = torch.from_numpy(rows).to(dev)
                bi = [x.index_select(0, idx) for x in ins]
                bo = [x.index_select(0, idx) for x in outs]
                for h in range(dataset.horizon):
                    hat = self.forward(bi[0][:, h], bi[1][:, h], normalize_action=None, normalize_state=None,
                                       unnormalize_state=None)
                    evals.append(np.asarray(criterion(hat, bo[1][:, h]).cpu()))
        return evals

    def forward(self, state, action, normalize_action=None, normalize_state=None, unnormalize_state=None):
        if state.is_cuda and not torch.is_grad_enabled() and getattr(self, "noise", None) is None:
            from . import fused
            out = fused.try_forward(self, state, action, normalize_action, normalize_state, unnormalize_state)
            if out is not None:
                return out
        if normalize_action:
            action = normalize_action(action)
        if normalize_state:
            state = normalize_state(state)
        x = torch.cat([state, action], dim=1)
        out = self._forward(x)
        if unnormalize_state:
            out = unnormalize_state(out)
        return out


class Model(DynamicsModel):
    """models.py:96-110 generalised to `n_hidden` Linear-ReLU layers (default 2 = the reference).

    Layers are named linear1 .. linear{n_hidden+1} so an n_hidden=2 state_dict loads into the
    reference's Model and vice versa."""

    def __init__(self, state_dim, action_dim, hidden_units=50, noise=None, n_hidden=2):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.hidden_units, self.n_hidden = hidden_units, n_hidden
        dims = [state_dim + action_dim] + [hidden_units] * n_hidden + [state_dim]
        for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
            setattr(self, f"linear{i + 1}", nn.Linear(fi, fo))
        self.activation_fn = nn.ReLU()
        self.noise = noise

    def linears(self):
        m = self._modules   # the registered submodules (what getattr resolves to), without its overhead
        return [m[f"linear{i + 1}"] for i in range(self.n_hidden + 1)]

    def _forward(self, x):
        lins = self.linears()
        for lin in lins[:-1]:
            x = self.activation_fn(lin(x))
        x = lins[-1](x)
        return x if self.noise is None else x + torch.randn_like(x) * self.noise


class LinearModel(DynamicsModel):
    """models.py:113-122: one Linear from (s, a) to s, plus optional Gaussian noise (experiment.py:41's
    "lin" model). The fused kernels need a hidden layer, so the planners run this model through its
    callable and train_model through autograd."""

    def __init__(self, state_dim, action_dim, noise=None):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.linear1 = nn.Linear(state_dim + action_dim, state_dim)
        self.noise = noise

    def _forward(self, x):
        x = self.linear1(x)
        return x if self.noise is None else x + torch.randn_like(x) * self.noise


def _softplus(x):
    """max(x, 0) + log1p(exp(-|x|)): the form csrc/train_nll.hip evaluates."""
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def bounded_logvar(raw, min_logvar, max_logvar):
    """The PETS bound on a raw log-variance: max - softplus(max - raw), then min + softplus(. - min)."""
    u = max_logvar - _softplus(max_logvar - raw)
    return min_logvar + _softplus(u - min_logvar)


def gaussian_nll(mean, logvar, target):
    """The project's Gaussian NLL of one horizon step: sum_{b, j} [(m - y)^2 exp(-lv) + lv] / (B s), MSELoss's scale
    (mbrl_cem.h, mbrl_train_grads_nll: the constant and the factor 1/2 of the density are left out)."""
    return (((mean - target) ** 2) * torch.exp(-logvar) + logvar).sum() / mean.numel()


class _MeanRows:
    """The mean rows of a ProbabilisticModel's head as the nn.Linear the packer and the evaluation read: weight
    [s, W] and bias [s] are views of the head's first s rows (the same storage, so the same pointers)."""

    def __init__(self, head, s):
        self._head, self._s = head, s

    @property
    def _parameters(self):                # (fused._param_key: the live Parameters' pointers and versions)
        return self._head._parameters

    @property
    def weight(self):
        return self._head.weight[:self._s]

    @property
    def bias(self):
        return self._head.bias[:self._s]


class ProbabilisticModel(DynamicsModel):
    """A PETS-style probabilistic member (not in the reference): Model's trunk of `n_hidden` Linear-ReLU layers and
    one head Linear(hidden_units -> 2 * state_dim) whose rows [0, s) are the predicted mean and rows [s, 2 s) the
    raw log-variance, bounded per dimension by bounded_logvar(raw, min_logvar, max_logvar). The bounds are [s]
    float32 buffers: not parameters, and not trained here. No reward head and no noise injection: forward() and
    the planners use the mean (EnsembleModel.train_members(loss="nll") trains both halves)."""

    def __init__(self, state_dim, action_dim, hidden_units=200, n_hidden=2, min_logvar=-10.0, max_logvar=0.5):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.hidden_units, self.n_hidden = hidden_units, n_hidden
        dims = [state_dim + action_dim] + [hidden_units] * n_hidden + [2 * state_dim]
        for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
            setattr(self, f"linear{i + 1}", nn.Linear(fi, fo))
        self.activation_fn = nn.ReLU()
        self.noise = None
        self.register_buffer("min_logvar", torch.full((state_dim,), float(min_logvar), dtype=torch.float32))
        self.register_buffer("max_logvar", torch.full((state_dim,), float(max_logvar), dtype=torch.float32))

    def linears(self):
        m = self._modules
        return [m[f"linear{i + 1}"] for i in range(self.n_hidden + 1)]

    def mean_linears(self):
        """The layers of the deterministic model this one is for the planners and the held-out MSE: the trunk and
        the head's mean rows."""
        lins = self.linears()
        return lins[:-1] + [_MeanRows(lins[-1], self.state_dim)]

    def _head(self, x):
        lins = self.linears()
        for lin in lins[:-1]:
            x = self.activation_fn(lin(x))
        return lins[-1](x)

    def _forward(self, x):
        return self._head(x)[..., :self.state_dim]

    def _dist(self, x):
        """(mean, bounded log-variance) of the concatenated (state, action) rows x, in the space the model is
        trained in."""
        out = self._head(x)
        s = self.state_dim
        return out[..., :s], bounded_logvar(out[..., s:], self.min_logvar, self.max_logvar)

    def predict_dist(self, state, action, normalize_action=None, normalize_state=None, unnormalize_state=None):
        """forward()'s arguments; returns (mean, logvar): forward()'s mean and the bounded per-dimension
        log-variance of the normalised next state (it is not rescaled by unnormalize_state)."""
        if normalize_action:
            action = normalize_action(action)
        if normalize_state:
            state = normalize_state(state)
        mean, logvar = self._dist(torch.cat([state, action], dim=1))
        if unnormalize_state:
            mean = unnormalize_state(mean)
        return mean, logvar


class EnsembleModel(DynamicsModel):
    """PETS-style ensemble of E `Model`s, or of E `ProbabilisticModel`s (not in the reference; BASELINE.json config 5).

    The CEM planner rolls every member out on the same actions and scores a candidate by the mean
    of the members' returns. Called directly, forward() returns the member-mean next state."""

    def __init__(self, members):
        super().__init__()
        self.members = nn.ModuleList(members)
        m0 = self.members[0]
        for m in self.members:
            if not isinstance(m, (Model, ProbabilisticModel)) or type(m) is not type(m0) or \
                    (m.state_dim, m.action_dim, m.hidden_units, m.n_hidden) != \
                    (m0.state_dim, m0.action_dim, m0.hidden_units, m0.n_hidden):
                raise ValueError("EnsembleModel members must be Models (or ProbabilisticModels) of one shape")
        self.state_dim, self.action_dim = m0.state_dim, m0.action_dim
        self.hidden_units, self.n_hidden = m0.hidden_units, m0.n_hidden
        self.noise = None

    def _forward(self, x):
        return torch.stack([m._forward(x) for m in self.members]).mean(0)

    def train_members(self, dataset, optimizers, batch_size=512, num_epochs=50, bootstrap=True, seed=0,
                      criterion=None, writer=None, loss="one_step", max_grad_norm=None):
        """Train every member on its own view of `dataset`: the bootstrap training a PETS-style
        ensemble's diversity comes from (train_model, inherited, fits the member MEAN with one optimizer
        and one data order, so every member sees the same signal).

        optimizers: a list of E optimizers, one per member over that member's parameters, or a factory
        member -> optimizer. Member e's epoch k visits the rows member_order(seed, e, k, n, bootstrap):
        with bootstrap=True n draws WITH replacement, a fresh resample every epoch (each epoch then sees
        ~63% of the rows, and over the epochs every member sees all of them in its own proportions --
        the per-epoch form of the bootstrap; a resample fixed per member would be k-independent);
        with bootstrap=False a permutation. The draws come from np.random.default_rng([seed, e, k]): the
        global NumPy RNG is not touched. Each member minimises train_model's loss for a Model (the
        criterion of its predicted next state, summed over the horizon steps).

        On a GPU, members the native gradient supports (train_model's test) with plain Adam optimizers
        of equal betas, eps and weight decay train together: one mbrl_train_epoch_ensemble call per
        epoch, the members on a grid axis of shared launches, each member's result bit-identical to that
        member trained alone by mbrl_train_epoch on its order. Anything else -- CPU, `noise` on a
        member, another optimizer or criterion -- trains the members one after another on the same
        orders -- as do more than 8 members (MBRL_TRAIN_MAX_MEMBERS) or a member listed twice. Writer
        tags: loss/state/member{e}/{iteration}. train_iterations counts one per call on the ensemble and
        on each member. Returns the number of epochs that ran in the shared launches (0: member by
        member).

        loss: "one_step" (the default) is the teacher-forced loss above. "open_loop" trains on the loss
        evaluate_members(open_loop=True) measures: from states[i, 0] the member's own prediction is fed back
        as the next state for the dataset's `horizon` steps, the criterion of every step's prediction against
        next_states[i, h] is summed, and the gradient runs through the fed-back predictions (backpropagation
        through time); states[i, h] for h >= 1 is not read. Orders, hook, writer tags and the return value are
        the same; the shared launches are one mbrl_train_epoch_open_loop call per epoch
        (csrc/train_open_loop.hip) under the same support test, and the fallback feeds m._forward its own
        output in torch. Any other string is a ValueError before any work.

        max_grad_norm: None (the default: exactly the calls above), or a positive float -- each member's gradient
        is clipped to that global L2 norm between the gradient and the Adam step of every batch, as
        torch.nn.utils.clip_grad_norm_(m.parameters(), max_grad_norm) does (float("inf") clips nothing and only
        records). The shared launches become mbrl_train_epoch_ensemble_clipped / mbrl_train_epoch_open_loop_clipped
        (csrc/grad_clip.hip: two launches more per batch) under the same support test; the fallbacks call
        clip_grad_norm_. With a writer each batch's pre-clip norm goes to grad_norm/member{e}/{iteration}; the
        native path keeps the norms on the device through the epoch and copies them out with the losses. Anything
        but None or a positive number is a ValueError before any work.

        loss="nll" (an ensemble of ProbabilisticModels; any other member type is a ValueError): each member
        minimises the Gaussian negative log-likelihood of next_states[i, h] under its predicted mean and bounded
        log-variance, teacher forced, summed over the horizon steps on MSELoss's scale (gaussian_nll;
        include/mbrl_cem.h, mbrl_train_grads_nll). The shared launches are one mbrl_train_epoch_nll(_clipped) call
        per epoch (csrc/train_nll.hip) when the members' bounds are equal; the fallback is the same loss under
        autograd. `criterion` is not used. The writer gets the NLL under loss/state/member{e}/{iteration}."""
        if loss not in ("one_step", "open_loop", "nll"):
            raise ValueError(f'train_members: loss must be "one_step", "open_loop" or "nll", got {loss!r}')
        max_grad_norm = _check_max_grad_norm("train_members", max_grad_norm)
        open_loop = loss == "open_loop"
        members = list(self.members)
        _check_nll_members("train_members", members, loss)
        opts = [optimizers(m) for m in members] if callable(optimizers) else list(optimizers)
        if len(opts) != len(members):
            raise ValueError(f"train_members needs one optimizer per member ({len(members)}), got {len(opts)}")
        criterion = criterion or torch.nn.MSELoss()
        n = dataset.num_transitions()
        first = 0
        if n > 0 and num_epochs > 0 and _device_of(self).type == "cuda":
            with torch.cuda.device(_device_of(self)):
                first = _train_members_native(self, members, opts, dataset, batch_size, num_epochs, bootstrap, seed,
                                              criterion, writer, open_loop=open_loop, max_grad_norm=max_grad_norm,
                                              nll=loss == "nll")
        if loss != "one_step" and n > 0 and first < num_epochs:
            torch_epochs = _train_open_loop_torch if open_loop else _train_nll_torch
            for e, (m, opt) in enumerate(zip(members, opts)):
                if first > 0:
                    m.train_iterations -= 1
                torch_epochs(m, e, dataset, opt, batch_size, num_epochs - first, criterion, writer,
                             lambda k, e=e: member_order(seed, e, first + k, n, bootstrap),
                             first * ((n + batch_size - 1) // batch_size), max_grad_norm)
                m.train_iterations += 1
        elif first < num_epochs or n == 0 or num_epochs <= 0:
            for e, (m, opt) in enumerate(zip(members, opts)):
                def step_loss(inp, out, m=m):
                    (states, actions), (_, next_states) = inp, out
                    return [criterion(m.forward(states, actions, normalize_action=None, normalize_state=None,
                                                unnormalize_state=None), next_states)]
                if first > 0:                 # (the native epochs counted this call already)
                    m.train_iterations -= 1
                _train_loop(m, dataset, opt, batch_size, num_epochs - first, step_loss, writer,
                            [f"loss/state/member{e}/{{}}"], criterion,
                            order_fn=lambda k, e=e: member_order(seed, e, first + k, n, bootstrap),
                            iter0=first * ((n + batch_size - 1) // batch_size), max_grad_norm=max_grad_norm,
                            norm_tag=f"grad_norm/member{e}/{{}}")
        self.train_iterations += 1
        return first

    def evaluate_members(self, dataset, rows=None, open_loop=False, predictions=False, nll=False):
        """Every member's error on rows `rows` of dataset.stacked() (default: all of them; indices may repeat):
        dict(loss [E], per_step [E, horizon], row_err [E, R, horizon]) on the ensemble's device, with
            row_err[e, r, h] = sum_j (member e's predicted next state - next_states[rows[r], h])_j ** 2,
            per_step[e, h]   = sum_r row_err[e, r, h] / (R * state_dim)    (MSELoss of step h),
            loss[e]          = sum_h per_step[e, h]: train_members' loss of a batch made of these rows.
        open_loop=False: the member predicts from the dataset's true states[rows[r], h] at every step (teacher
        forcing). open_loop=True: from states[rows[r], 0] only, its own prediction being fed back as the
        next state for the dataset's `horizon` steps, as a planner's rollout does (the stacked next_states[i, h]
        and states[i, h + 1] are one sample under one normalisation, so the prediction is fed back as it
        is); predictions=True (open loop only) adds pred [E, R, horizon, state_dim], the fed-back states.
        On a GPU, when train_members' support test passes for every member, one mbrl_eval_members /
        mbrl_eval_members_open_loop call (csrc/eval.hip) with no host synchronisation -- pass `rows` as a
        device tensor to keep its upload out as well; otherwise (CPU, `noise`, more than 8 members) the same
        definitions in torch. ProbabilisticModel members are evaluated on their mean (the head's first s rows).

        nll=True (ProbabilisticModel members, teacher forced only): the Gaussian negative log-likelihood
        train_members(loss="nll") minimises. The dict then holds row_nll [E, R, horizon] = sum_j [(m - y)^2
        exp(-lv) + lv], per_step and loss from row_nll on the same scale, row_err as above, and mse [E] and
        mean_logvar [E]: the same sums of row_err and of sum_j lv (mbrl_eval_members_nll, csrc/train_nll.hip, or
        the same definitions in torch)."""
        if predictions and not open_loop:
            raise ValueError("evaluate_members returns predictions of an open-loop evaluation only (open_loop=True)")
        if nll and open_loop:
            raise ValueError("evaluate_members: the NLL is teacher forced (nll=True excludes open_loop=True)")
        members = list(self.members)
        _check_nll_members("evaluate_members", members, "nll" if nll else None)
        dev = _device_of(self)
        _, ins, outs = dataset.stacked(dev)
        rows = _holdout_rows(dataset, dev, rows)
        R, H = int(rows.shape[0]), dataset.horizon
        if R < 1:
            raise ValueError("evaluate_members needs at least one row")
        if nll:
            return _evaluate_members_nll(members, dataset, ins, outs, rows, dev)
        pred = None
        if _NativeEval.supported(members, dataset, ins, outs):
            with torch.cuda.device(dev):
                row_err = torch.empty((len(members), R, H), dtype=torch.float32, device=dev)
                loss3 = torch.empty((len(members), 3), dtype=torch.float32, device=dev)
                if open_loop:
                    if predictions:
                        pred = torch.empty((len(members), R, H, self.state_dim), dtype=torch.float32, device=dev)
                    _NativeEval(members, ins, outs, H).run_open_loop(rows, row_err, loss3, pred)
                else:
                    _NativeEval(members, ins, outs, H).run(rows, row_err, loss3)
            loss = loss3[:, 0]
        else:
            if open_loop:
                row_err, pred = _eval_members_open_loop_torch(members, ins, outs, rows)
            else:
                row_err = _eval_members_torch(members, ins, outs, rows)
            loss = None
        per_step = row_err.sum(1) / (R * self.state_dim)
        out = dict(loss=per_step.sum(1) if loss is None else loss, per_step=per_step, row_err=row_err)
        if predictions:
            out["pred"] = pred
        return out

    def fit_members(self, dataset, holdout, optimizers, batch_size=512, max_epochs=50, patience=None, check_every=1,
                    restore_best=True, bootstrap=True, seed=0, criterion=None, writer=None, holdout_loss="one_step",
                    train_loss="one_step", max_grad_norm=None):
        """train_members with a held-out set: the same epochs (orders, shared launches and fallback rules
        are train_members'), and after each epoch every member's loss on all rows of `holdout` (a
        TransitionsDataset of the same dimensions and normalisation; evaluate_members' loss) and a snapshot
        of each member's parameters whenever its loss is below all its earlier ones (a NaN never is). On the
        native path the evaluation and the snapshots are two C calls enqueued on the training stream
        (mbrl_eval_members or mbrl_eval_members_open_loop, mbrl_keep_best); with patience=None the host never
        waits between epochs.

        holdout_loss: "one_step" scores a member by evaluate_members(holdout), "open_loop" by
        evaluate_members(holdout, open_loop=True): its own predictions fed back over the holdout's horizon,
        which may be longer than the training dataset's (30 against 1, say: the planning horizon). Keep-best,
        patience, restore_best, the report and elite(k) then act on that loss. Any other string is a
        ValueError before any work.

        train_loss: train_members' `loss` for the epochs: "one_step" or "open_loop" (with
        holdout_loss="open_loop" the members are trained on, and picked by, the loss a planner's rollout
        meets). Any other string is a ValueError before any work.

        "nll" for either (ProbabilisticModel members; any other member type is a ValueError): the epochs minimise,
        or the members are scored and kept by, the Gaussian negative log-likelihood (train_members(loss="nll"),
        evaluate_members(nll=True)); val_loss then holds the NLL.

        max_grad_norm: train_members' per-member gradient clipping for the epochs (None: none).

        patience: after each epoch k with (k + 1) % check_every == 0 the host reads the members' `stale`
        counts (epochs since the member's best) and stops when every member's is >= patience
        (tests/holdout_reference.py restates the rule in NumPy). restore_best: at the end each member's parameters become its
        snapshot, by an in-place copy (the planners' cached weight packs are refreshed as after
        train_members); a member whose loss was never finite has no snapshot and keeps its last weights. The optimizers' state stays at the last epoch's: it is not snapshotted, so training
        on from restored weights starts with moments that belong to later weights.

        Returns, and keeps as self.holdout_report, dict(val_loss [epochs_run, E], best_loss [E],
        best_epoch [E] (CPU tensors), epochs_run, native_epochs: the epochs that trained in the shared
        launches, native_eval: whether the held-out losses came from the C entry, holdout_loss). Writer tags: train_members', and loss/holdout/member{e}/{iteration} per epoch."""
        if holdout_loss not in ("one_step", "open_loop", "nll"):
            raise ValueError('fit_members: holdout_loss must be "one_step", "open_loop" or "nll", '
                             f'got {holdout_loss!r}')
        if train_loss not in ("one_step", "open_loop", "nll"):
            raise ValueError(f'fit_members: train_loss must be "one_step", "open_loop" or "nll", got {train_loss!r}')
        max_grad_norm = _check_max_grad_norm("fit_members", max_grad_norm)
        open_loop = train_loss == "open_loop"
        members = list(self.members)
        _check_nll_members("fit_members", members, train_loss)
        _check_nll_members("fit_members", members, holdout_loss)
        opts = [optimizers(m) for m in members] if callable(optimizers) else list(optimizers)
        if len(opts) != len(members):
            raise ValueError(f"fit_members needs one optimizer per member ({len(members)}), got {len(opts)}")
        if patience is not None and (patience < 1 or check_every < 1):
            raise ValueError("fit_members needs patience >= 1 and check_every >= 1")
        criterion = criterion or torch.nn.MSELoss()
        n, dev = dataset.num_transitions(), _device_of(self)
        max_epochs = max(int(max_epochs), 0) if n > 0 else 0
        iteration = [m.train_iterations for m in members]
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            tracker = _Holdout(members, holdout, max_epochs, open_loop=holdout_loss == "open_loop",
                               nll=holdout_loss == "nll")
            stopped = []

            def after_epoch(k):
                tracker.record(k)
                if tracker.stop(k, patience, check_every):
                    stopped.append(k)
                return bool(stopped)
            first = 0
            if max_epochs > 0 and dev.type == "cuda":
                first = _train_members_native(self, members, opts, dataset, batch_size, max_epochs, bootstrap, seed,
                                              criterion, writer, after_epoch=after_epoch, open_loop=open_loop,
                                              max_grad_norm=max_grad_norm, nll=train_loss == "nll")
            batches = (n + batch_size - 1) // max(batch_size, 1)
            for k in range(tracker.epochs, 0 if stopped else max_epochs):
                for e, (m, opt) in enumerate(zip(members, opts)):
                    def step_loss(inp, out, m=m):
                        (states, actions), (_, next_states) = inp, out
                        return [criterion(m.forward(states, actions, normalize_action=None, normalize_state=None,
                                                    unnormalize_state=None), next_states)]
                    m.train_iterations = iteration[e]         # (one call's worth of epochs: one iteration)
                    if train_loss != "one_step":
                        (_train_open_loop_torch if open_loop else _train_nll_torch)(
                            m, e, dataset, opt, batch_size, 1, criterion, writer,
                            lambda _, e=e, k=k: member_order(seed, e, k, n, bootstrap), k * batches, max_grad_norm)
                        continue
                    _train_loop(m, dataset, opt, batch_size, 1, step_loss, writer, [f"loss/state/member{e}/{{}}"],
                                criterion, order_fn=lambda _, e=e, k=k: member_order(seed, e, k, n, bootstrap),
                                iter0=k * batches, max_grad_norm=max_grad_norm, norm_tag=f"grad_norm/member{e}/{{}}")
                if after_epoch(k):
                    break
            ran = tracker.epochs
            best_epoch = tracker.best_epoch.detach().cpu().to(torch.int64)      # (the call's first host read)
            if restore_best:
                with torch.no_grad():
                    for params, snaps, at in zip(tracker.params, tracker.snaps, best_epoch.tolist()):
                        if at >= 0:                   # (a member whose loss was never finite stays where it is)
                            torch._foreach_copy_(params, snaps)
            val = tracker.val[:ran, :, 0].detach().cpu()
            report = dict(val_loss=val, best_loss=tracker.best_loss.detach().cpu(), best_epoch=best_epoch,
                          epochs_run=ran, native_epochs=first, native_eval=tracker.native is not None,
                          holdout_loss=holdout_loss)
        if writer is not None:
            for k, row in enumerate(val.tolist()):
                for e, v in enumerate(row):
                    writer.add_scalar(f"loss/holdout/member{e}/{iteration[e]}", v, k + 1)
        for m, it in zip(members, iteration):
            m.train_iterations = it + 1
        self.train_iterations += 1
        self.holdout_report = report
        return report

    def elite(self, k, report=None):
        """An EnsembleModel over the k members with the lowest best_loss of `report` (default: the last
        fit_members'), ties to the lower index, in member order (elite_indices). The members are shared, not
        copied: the planners then roll out k members, and training either ensemble trains the same weights."""
        report = report if report is not None else getattr(self, "holdout_report", None)
        if report is None:
            raise ValueError("elite needs a report: call fit_members first or pass one")
        best = np.asarray(torch.as_tensor(report["best_loss"]).cpu().numpy(), np.float64)
        E = len(self.members)
        if best.shape != (E,) or not 1 <= k <= E:
            raise ValueError(f"elite needs 1 <= k <= {E} and one best_loss per member")
        keep = sorted(np.argsort(best, kind="stable")[:k].tolist())     # (NaNs sort last)
        out = EnsembleModel([self.members[i] for i in keep])
        out.elite_indices = keep
        return out


def _check_max_grad_norm(what, max_grad_norm):
    """None, or the positive float train_members / fit_members clip to (inf allowed); anything else a ValueError."""
    if max_grad_norm is None:
        return None
    if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not max_grad_norm > 0:
        raise ValueError(f"{what}: max_grad_norm must be None or a positive number, got {max_grad_norm!r}")
    return float(max_grad_norm)


def _check_nll_members(what, members, loss):
    """The NLL needs a log-variance: ProbabilisticModel members only."""
    if loss == "nll" and not all(isinstance(m, ProbabilisticModel) for m in members):
        raise ValueError(f'{what}: the "nll" loss needs an ensemble of ProbabilisticModel members')


def member_order(seed, e, k, n, bootstrap=True):
    """The rows member e visits in epoch k of EnsembleModel.train_members (int64 [n]): n draws with
    replacement (bootstrap) or a permutation, from np.random.default_rng([seed, e, k])."""
    rng = np.random.default_rng([int(seed), int(e), int(k)])
    if bootstrap:
        return rng.integers(0, n, size=n, dtype=np.int64)
    return rng.permutation(n).astype(np.int64, copy=False)


class _NativeEnsemble:
    """mbrl_train_epoch_ensemble for E supported members: per member the gradient buffers and
    mbrl_train_model of _NativeGrads, one dataset, one workspace of E member slices."""

    WORKSPACE, EPOCH = "mbrl_train_ensemble_workspace_bytes", "mbrl_train_epoch_ensemble"
    CLIPPED = "mbrl_train_epoch_ensemble_clipped"

    def __init__(self, members, ins, outs, horizon, batch_size):
        from . import _lib
        self._lib, self.lib = _lib, _native_lib()
        self.dev = _device_of(members[0])
        self.E = len(members)
        self.params, self.grads = [], []
        self.models = (_lib.TrainModel * self.E)()
        for e, model in enumerate(members):
            lins = model.linears()
            params = [t for lin in lins for t in (lin.weight, lin.bias)]
            grads = [torch.zeros_like(t) for t in params]
            m = self.models[e]
            m.state_dim, m.action_dim, m.hidden = model.state_dim, model.action_dim, model.hidden_units
            m.n_hidden, m.reward_head, m.horizon = model.n_hidden, 0, int(horizon)
            for i, lin in enumerate(lins):
                m.weight[i], m.bias[i] = lin.weight.data_ptr(), lin.bias.data_ptr()
                m.weight_grad[i], m.bias_grad[i] = grads[2 * i].data_ptr(), grads[2 * i + 1].data_ptr()
            self.params.append(params)
            self.grads.append(grads)
        (states, actions), (rewards, next_states) = ins, outs
        self.keep = [x.contiguous() for x in (states, actions, next_states, rewards)]
        self.data = _lib.TrainData()
        d = self.data
        d.states, d.actions, d.next_states, d.rewards = [x.data_ptr() for x in self.keep]
        d.transitions = states.shape[0]
        need = getattr(self.lib, self.WORKSPACE)(self.models, self.E, int(batch_size))
        if need == 0:
            _lib.check(-1, self.WORKSPACE)
        self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        self.ptrs = [t.data_ptr() for params in self.params for t in params]
        self.clip_ws = None

    @classmethod
    def cached(cls, owner, members, ins, outs, horizon, batch_size):
        """The object of the ensemble's previous train_members call while nothing it binds has changed
        (_NativeGrads.cached's rule): a call then allocates no gradients, workspace or tables."""
        key = (cls.EPOCH, str(_device_of(members[0])), int(horizon), int(batch_size), id(_LIB_OVERRIDE),
               tuple(t.data_ptr() for m in members for lin in m.linears() for t in (lin.weight, lin.bias)),
               tuple((x.data_ptr(), tuple(x.shape), x.is_contiguous()) for x in (*ins, *outs)))
        hit = _NATIVE_ENS_CACHE.get(owner)
        if hit is not None and hit[0] == key:
            return hit[1]
        obj = cls(members, ins, outs, horizon, batch_size)
        if all(x.is_contiguous() for x in (*ins, *outs)):
            _NATIVE_ENS_CACHE[owner] = (key, obj)
        else:
            _NATIVE_ENS_CACHE.pop(owner, None)
        return obj

    def _extra_args(self):
        """What the entry takes between the stream and the clip struct."""
        return ()

    def epoch(self, orders, rows, batch_size, adams):
        """One epoch of every member over the device orders [E * rows]. Returns the losses
        [batches, E, 3] (device), or None when an optimizer's state does not allow the whole-epoch
        call or the optimizers' hyper-parameters differ (nothing has been launched then)."""
        return self._epoch(orders, rows, batch_size, adams, None)

    def epoch_clipped(self, orders, rows, batch_size, adams, max_norm):
        """epoch() through the clipped entry: returns (losses, norms [batches, E] (device): each batch's pre-clip
        gradient norm per member), or None as epoch() does."""
        return self._epoch(orders, rows, batch_size, adams, max_norm)

    def _epoch(self, orders, rows, batch_size, adams, max_norm):
        for params, grads in zip(self.params, self.grads):
            for p, g in zip(params, grads):
                if p.grad is not g:
                    p.grad = g
        if [t.data_ptr() for params in self.params for t in params] != self.ptrs:
            raise RuntimeError("model parameters moved during training")
        steps = (rows + batch_size - 1) // batch_size
        plans = [adam.epoch_plan(params, steps) for adam, params in zip(adams, self.params)]
        if any(pl is None for pl in plans):
            return None
        hp = plans[0][1]
        fields = [f for f, _ in hp._fields_]
        if any(getattr(pl[1], f) != getattr(hp, f) for pl in plans for f in fields):
            return None
        count = len(self.params[0])
        table = (self._lib.AdamTensor * (self.E * count))()
        for e, pl in enumerate(plans):
            for i in range(count):
                src, dst = pl[0][i], table[e * count + i]
                dst.param, dst.grad, dst.exp_avg, dst.exp_avg_sq, dst.numel = \
                    src.param, src.grad, src.exp_avg, src.exp_avg_sq, src.numel
        # [batches][E * count], member-major within a batch
        ss = np.stack([np.ctypeslib.as_array(pl[2]).reshape(steps, count) for pl in plans], axis=1)
        bc = np.stack([np.ctypeslib.as_array(pl[3]).reshape(steps, count) for pl in plans], axis=1)
        ss, bc = np.ascontiguousarray(ss, np.float32), np.ascontiguousarray(bc, np.float32)
        losses = torch.empty((steps, self.E, 3), dtype=torch.float32, device=self.dev)
        args = (self.models, self.E, ctypes.byref(self.data), ctypes.c_void_p(orders.data_ptr()), int(rows),
                int(batch_size), table, count, ctypes.byref(hp), ctypes.c_void_p(ss.ctypes.data),
                ctypes.c_void_p(bc.ctypes.data), ctypes.c_void_p(losses.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()),
                self.ws.numel(), self._lib.stream_handle(self.dev))
        args += self._extra_args()
        if max_norm is None:
            self._lib.check(getattr(self.lib, self.EPOCH)(*args), self.EPOCH)
        else:
            if self.clip_ws is None:
                need = self.lib.mbrl_grad_clip_workspace_bytes(table, self.E, count)
                if need == 0:
                    self._lib.check(-1, "mbrl_grad_clip_workspace_bytes")
                self.clip_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            norms = torch.empty((steps, self.E), dtype=torch.float32, device=self.dev)
            clip = self._lib.GradClip(max_norm=max_norm, norms=norms.data_ptr(), workspace=self.clip_ws.data_ptr(),
                                      ws_bytes=self.clip_ws.numel())
            self._lib.check(getattr(self.lib, self.CLIPPED)(*args, ctypes.byref(clip)), self.CLIPPED)
        for adam, params in zip(adams, self.params):
            adam.epoch_done(params)
        return losses if max_norm is None else (losses, norms)


class _NativeEnsembleOpenLoop(_NativeEnsemble):
    """mbrl_train_epoch_open_loop: the same members, tables and orders, the open-loop loss (csrc/train_open_loop.hip)."""

    WORKSPACE, EPOCH = "mbrl_train_open_loop_workspace_bytes", "mbrl_train_epoch_open_loop"
    CLIPPED = "mbrl_train_epoch_open_loop_clipped"


class _NativeEnsembleNll(_NativeEnsemble):
    """mbrl_train_epoch_nll: ProbabilisticModel members (each head one [2 s, W] tensor), the Gaussian NLL
    (csrc/train_nll.hip). The entry takes one pair of bounds for all members: member 0's buffers, read live."""

    WORKSPACE, EPOCH = "mbrl_train_nll_workspace_bytes", "mbrl_train_epoch_nll"
    CLIPPED = "mbrl_train_epoch_nll_clipped"

    def __init__(self, members, ins, outs, horizon, batch_size):
        super().__init__(members, ins, outs, horizon, batch_size)
        self.bound_t = (members[0].min_logvar, members[0].max_logvar)
        self.bounds = self._lib.NllBounds(self.bound_t[0].data_ptr(), self.bound_t[1].data_ptr())
        if members[0].action_dim == 0:
            self.data.actions = None

    @staticmethod
    def bounds_shared(members):
        m0 = members[0]
        return all(b.dtype == torch.float32 and b.is_contiguous() and b.device == m.linear1.weight.device
                   for m in members for b in (m.min_logvar, m.max_logvar)) and \
            all(torch.equal(m.min_logvar, m0.min_logvar) and torch.equal(m.max_logvar, m0.max_logvar)
                for m in members[1:])

    def _extra_args(self):
        if (self.bounds.min_logvar, self.bounds.max_logvar) != tuple(t.data_ptr() for t in self.bound_t):
            raise RuntimeError("the log-variance bounds moved during training")
        return (ctypes.byref(self.bounds),)


def _nll_batch_loss(m, states, actions, next_states, idx, horizon):
    """train_members(loss="nll")'s loss of one batch in torch: gaussian_nll of every step, summed."""
    st, ac, ns = (x.index_select(0, idx) for x in (states, actions, next_states))
    loss = 0
    for h in range(horizon):
        mean, logvar = m._dist(torch.cat([st[:, h], ac[:, h]], dim=1))
        loss = loss + gaussian_nll(mean, logvar, ns[:, h])
    return loss


def _train_nll_torch(m, e, dataset, opt, batch_size, num_epochs, criterion, writer, order_fn, iter0,
                     max_grad_norm=None):
    """train_members(loss="nll") for one member in torch (_train_open_loop_torch's loop, teacher forced, the
    Gaussian NLL; `criterion` is not used). It is the baseline tools/train_nll_bench.py times."""
    dev = _device_of(m)
    _, ins, outs = dataset.stacked(dev)
    (states, actions), (_, next_states) = ins, outs
    fast = AdamStep.maybe(opt) if dev.type == "cuda" else None
    it = iter0
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        for k in range(num_epochs):
            order = torch.from_numpy(order_fn(k)).to(dev)
            for i in range(0, int(order.shape[0]), batch_size):
                opt.zero_grad()
                loss = _nll_batch_loss(m, states, actions, next_states, order[i:i + batch_size], dataset.horizon)
                loss.backward()
                if max_grad_norm is not None:
                    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), max_grad_norm)
                if fast is None or not fast.step():
                    opt.step()
                it += 1
                if writer is not None:
                    writer.add_scalar(f"loss/state/member{e}/{m.train_iterations}", loss, it)
                    if max_grad_norm is not None:
                        writer.add_scalar(f"grad_norm/member{e}/{m.train_iterations}", norm, it)


def _train_open_loop_torch(m, e, dataset, opt, batch_size, num_epochs, criterion, writer, order_fn, iter0,
                           max_grad_norm=None):
    """train_members(loss="open_loop") for one member in torch: per batch the criterion of every step's prediction
    against next_states[i, h], summed, with m._forward fed its own output from states[i, 0] on; autograd runs
    through the fed-back predictions. A plain Adam steps through mbrl_adam_step on a GPU (optim.AdamStep).
    max_grad_norm: clip_grad_norm_ between backward() and the step; the writer gets the pre-clip norm."""
    dev = _device_of(m)
    _, ins, outs = dataset.stacked(dev)
    (states, actions), (_, next_states) = ins, outs
    fast = AdamStep.maybe(opt) if dev.type == "cuda" else None
    it = iter0
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        for k in range(num_epochs):
            order = torch.from_numpy(order_fn(k)).to(dev)
            for i in range(0, int(order.shape[0]), batch_size):
                idx = order[i:i + batch_size]
                opt.zero_grad()
                x, loss = states.index_select(0, idx)[:, 0], 0
                ac, ns = actions.index_select(0, idx), next_states.index_select(0, idx)
                for h in range(dataset.horizon):
                    x = m._forward(torch.cat([x, ac[:, h]], dim=1))
                    loss = loss + criterion(x, ns[:, h])
                loss.backward()
                if max_grad_norm is not None:
                    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), max_grad_norm)
                if fast is None or not fast.step():
                    opt.step()
                it += 1
                if writer is not None:
                    writer.add_scalar(f"loss/state/member{e}/{m.train_iterations}", loss, it)
                    if max_grad_norm is not None:
                        writer.add_scalar(f"grad_norm/member{e}/{m.train_iterations}", norm, it)


def _train_members_native(owner, members, opts, dataset, batch_size, num_epochs, bootstrap, seed, criterion, writer,
                          after_epoch=None, open_loop=False, max_grad_norm=None, nll=False):
    """The epochs of train_members the shared launches can take, from the first: returns how many ran
    (0: not supported here; the caller trains the rest member by member). Orders are staged as
    _train_loop_on stages them: epoch k + 1's rows are drawn into a pinned ring row while epoch k
    runs and copied on the side stream, with no host round trip between epochs.
    after_epoch (fit_members): called with k once epoch k is enqueued; a true result ends the epochs.
    max_grad_norm: the epochs go through the clipped entry; the norms stay on the device beside the losses until
    the writer reads both after the last epoch."""
    from . import _lib
    dev = _device_of(members[0])
    E = len(members)
    if E > _lib.TRAIN_MAX_MEMBERS or len({id(m) for m in members}) != E:
        return 0
    _, ins, outs = dataset.stacked(dev)
    if any(_NativeGrads.supported(m, dataset, ins, outs, criterion, probabilistic=nll) is not False for m in members):
        return 0
    if nll and not _NativeEnsembleNll.bounds_shared(members):
        return 0
    adams = [AdamStep.maybe(opt) for opt in opts]
    if any(a is None for a in adams):
        return 0
    n = dataset.num_transitions()
    kind = _NativeEnsembleNll if nll else _NativeEnsembleOpenLoop if open_loop else _NativeEnsemble
    native = kind.cached(owner, members, ins, outs, dataset.horizon, batch_size)
    ring = _order_ring(dev, E * n)
    main = torch.cuda.current_stream(dev)

    def fill(k):
        def write(row):
            for e in range(E):
                row[e * n:(e + 1) * n] = member_order(seed, e, k, n, bootstrap)
        return write
    ring.draw(0, fill(0))
    ring.copy(0, main)
    epoch_losses, epoch_norms, done = [], [], 0
    for ep in range(num_epochs):
        _, order = ring.rows(ep)
        if ep >= 1:
            ring.copied[ep % ring.K].wait(main)       # epoch ep's orders have landed
        if max_grad_norm is None:
            losses = native.epoch(order, n, batch_size, adams)
        else:
            losses = native.epoch_clipped(order, n, batch_size, adams, max_grad_norm)
        if losses is None:
            break
        if max_grad_norm is not None:
            losses, norms = losses
            epoch_norms.append(norms)
        if ep + 1 < num_epochs:
            ring.draw(ep + 1, fill(ep + 1))
            ring.copy(ep + 1, ring.side)
        ring.consumed[ep % ring.K].record(main)       # the ring row is free once this epoch has run
        epoch_losses.append(losses)
        done += 1
        if after_epoch is not None and after_epoch(ep):
            break
    if writer is not None:
        it = 0
        for losses in epoch_losses:
            for row in losses.cpu().tolist():
                it += 1
                for e, m in enumerate(members):
                    writer.add_scalar(f"loss/state/member{e}/{m.train_iterations}", row[e][0], it)
        it = 0
        for norms in epoch_norms:
            for row in norms.cpu().tolist():
                it += 1
                for e, m in enumerate(members):
                    writer.add_scalar(f"grad_norm/member{e}/{m.train_iterations}", row[e], it)
    if done:
        for m in members:
            m.train_iterations += 1
    return done


def _eval_members_torch(members, ins, outs, rows):
    """mbrl_eval_members' definitions in torch (CPU, or members the native call does not take): the squared
    error of every member's own _forward per row and horizon step, row_err [E, R, horizon]."""
    (states, actions), (_, next_states) = ins, outs
    with torch.no_grad():
        st, ac, ns = (x.index_select(0, rows) for x in (states, actions, next_states))
        R, H = st.shape[0], st.shape[1]
        x = torch.cat([st.reshape(R * H, -1), ac.reshape(R * H, -1)], dim=1)
        target = ns.reshape(R * H, -1)
        return torch.stack([((m._forward(x) - target) ** 2).sum(1).reshape(R, H) for m in members])


def _eval_members_nll_torch(members, ins, outs, rows):
    """mbrl_eval_members_nll's definitions in torch: (row_nll, row_err, row_lv), each [E, R, horizon]."""
    (states, actions), (_, next_states) = ins, outs
    with torch.no_grad():
        st, ac, ns = (x.index_select(0, rows) for x in (states, actions, next_states))
        R, H = st.shape[0], st.shape[1]
        x = torch.cat([st.reshape(R * H, -1), ac.reshape(R * H, -1)], dim=1)
        target = ns.reshape(R * H, -1)
        out = [[], [], []]
        for m in members:
            mean, lv = m._dist(x)
            d2 = (mean - target) ** 2
            for acc, v in zip(out, (d2 * torch.exp(-lv) + lv, d2, lv)):
                acc.append(v.sum(1).reshape(R, H))
        return tuple(torch.stack(v) for v in out)


def _evaluate_members_nll(members, dataset, ins, outs, rows, dev):
    """evaluate_members(nll=True): the native entry where it takes the members, else torch."""
    E, R, H, s = len(members), int(rows.shape[0]), dataset.horizon, members[0].state_dim
    if _NativeEval.supported(members, dataset, ins, outs) and _NativeEnsembleNll.bounds_shared(members):
        with torch.cuda.device(dev):
            row = torch.empty((3, E, R, H), dtype=torch.float32, device=dev)
            loss3 = torch.empty((E, 3), dtype=torch.float32, device=dev)
            _NativeEval(members, ins, outs, H).run_nll(rows, row, loss3)
        row_nll, row_err, row_lv = row[0], row[1], row[2]
        loss, mse, mean_lv = loss3[:, 0], loss3[:, 1], loss3[:, 2]
    else:
        row_nll, row_err, row_lv = _eval_members_nll_torch(members, ins, outs, rows)
        loss, mse, mean_lv = ((v.sum(1) / (R * s)).sum(1) for v in (row_nll, row_err, row_lv))
    per_step = row_nll.sum(1) / (R * s)
    return dict(loss=loss, per_step=per_step, row_err=row_err, row_nll=row_nll, mse=mse, mean_logvar=mean_lv)


def _eval_members_open_loop_torch(members, ins, outs, rows):
    """mbrl_eval_members_open_loop's definitions in torch: from states[rows, 0] every member's own _forward is
    fed back as the next state, horizon times. Returns (row_err [E, R, horizon], pred [E, R, horizon, s])."""
    (states, actions), (_, next_states) = ins, outs
    with torch.no_grad():
        st, ac, ns = (x.index_select(0, rows) for x in (states, actions, next_states))
        errs, preds = [], []
        for m in members:
            x, steps = st[:, 0], []
            for h in range(st.shape[1]):
                x = m._forward(torch.cat([x, ac[:, h]], dim=1))
                steps.append(x)
            pred = torch.stack(steps, dim=1)
            preds.append(pred)
            errs.append(((pred - ns) ** 2).sum(2))
        return torch.stack(errs), torch.stack(preds)


class _NativeEval:
    """mbrl_eval_members / mbrl_eval_members_open_loop for E supported members on one dataset: the members' live weights and biases (no
    gradients), the stacked transitions, no workspace."""

    def __init__(self, members, ins, outs, horizon):
        from . import _lib
        self._lib, self.lib = _lib, _native_lib()
        self.dev = _device_of(members[0])
        self.E, self.horizon = len(members), int(horizon)
        self.members0 = members[0]
        # (a ProbabilisticModel's head is read through the same pointers: its mean rows are its first s rows)
        self.params = [[t for lin in m.linears() for t in (lin.weight, lin.bias)] for m in members]
        self.models = (_lib.TrainModel * self.E)()
        for m, model, params in zip(self.models, members, self.params):
            m.state_dim, m.action_dim, m.hidden = model.state_dim, model.action_dim, model.hidden_units
            m.n_hidden, m.reward_head, m.horizon = model.n_hidden, 0, self.horizon
            for i in range(len(params) // 2):
                m.weight[i], m.bias[i] = params[2 * i].data_ptr(), params[2 * i + 1].data_ptr()
        (states, actions), (rewards, next_states) = ins, outs
        self.keep = [x.contiguous() for x in (states, actions, next_states, rewards)]
        d = self.data = _lib.TrainData()
        d.states, d.actions, d.next_states, d.rewards = [x.data_ptr() for x in self.keep]
        if members[0].action_dim == 0:
            d.actions = None
        d.transitions = states.shape[0]
        self.ptrs = [t.data_ptr() for params in self.params for t in params]

    @staticmethod
    def supported(members, dataset, ins, outs):
        """train_members' own test, member by member (a member may be listed twice here)."""
        from . import _lib
        if _device_of(members[0]).type != "cuda" or len(members) > _lib.TRAIN_MAX_MEMBERS:
            return False
        mse = torch.nn.MSELoss()
        return all(_NativeGrads.supported(m, dataset, ins, outs, mse, probabilistic=True) is False for m in members)

    def run(self, rows, row_err, loss):
        """Enqueue the evaluation of the device rows `rows` into row_err [E, R, horizon] and loss [E, 3]."""
        if [t.data_ptr() for params in self.params for t in params] != self.ptrs:
            raise RuntimeError("model parameters moved during evaluation")
        P = ctypes.c_void_p
        self._lib.check(self.lib.mbrl_eval_members(self.models, self.E, ctypes.byref(self.data), P(rows.data_ptr()),
                                                   int(rows.shape[0]), P(row_err.data_ptr()), None, P(loss.data_ptr()),
                                                   self._lib.stream_handle(self.dev)), "mbrl_eval_members")

    def run_nll(self, rows, row, loss):
        """mbrl_eval_members_nll on ProbabilisticModel members of equal bounds (member 0's are passed): row
        [3, E, R, horizon] receives row_nll, row_err and row_lv, loss [E, 3] (nll, mse, mean_lv)."""
        if [t.data_ptr() for params in self.params for t in params] != self.ptrs:
            raise RuntimeError("model parameters moved during evaluation")
        P = ctypes.c_void_p
        bounds = self._lib.NllBounds(self.members0.min_logvar.data_ptr(), self.members0.max_logvar.data_ptr())
        self._lib.check(self.lib.mbrl_eval_members_nll(
            self.models, self.E, ctypes.byref(self.data), P(rows.data_ptr()), int(rows.shape[0]), ctypes.byref(bounds),
            P(row[0].data_ptr()), P(row[1].data_ptr()), P(row[2].data_ptr()), P(loss.data_ptr()),
            self._lib.stream_handle(self.dev)), "mbrl_eval_members_nll")

    def run_open_loop(self, rows, row_err, loss, pred=None):
        """The same with the members' predictions fed back (mbrl_eval_members_open_loop); pred: [E, R, horizon, s]
        or None."""
        if [t.data_ptr() for params in self.params for t in params] != self.ptrs:
            raise RuntimeError("model parameters moved during evaluation")
        P = ctypes.c_void_p
        self._lib.check(self.lib.mbrl_eval_members_open_loop(
            self.models, self.E, ctypes.byref(self.data), P(rows.data_ptr()), int(rows.shape[0]), P(row_err.data_ptr()),
            None, None if pred is None else P(pred.data_ptr()), P(loss.data_ptr()), self._lib.stream_handle(self.dev)),
            "mbrl_eval_members_open_loop")


def _holdout_rows(dataset, dev, rows):
    if rows is None:
        return torch.arange(dataset.num_transitions(), dtype=torch.int64, device=dev)
    return torch.as_tensor(rows, dtype=torch.int64).to(dev).contiguous().reshape(-1)


class _Holdout:
    """fit_members' per-epoch work: the members' losses on the held-out rows, the best loss so far and the
    snapshot of each member's parameters at its best epoch. On the native path (mbrl_eval_members and
    mbrl_keep_best on the training stream) the host reads nothing unless a patience asks for `stale`."""

    def __init__(self, members, holdout, max_epochs, open_loop=False, nll=False):
        self.members, self.open_loop, self.nll = members, open_loop, nll
        dev = self.dev = _device_of(members[0])
        _, self.ins, self.outs = holdout.stacked(dev)
        self.rows = _holdout_rows(holdout, dev, None)
        E, R, H = len(members), int(self.rows.shape[0]), holdout.horizon
        if R < 1:
            raise ValueError("fit_members needs a holdout with at least one transition")
        self.state_dim = members[0].state_dim
        self.params = [list(m.parameters()) for m in members]
        # (written by a member's first finite loss; a member that never has one is not restored)
        self.snaps = [[torch.empty_like(p) for p in params] for params in self.params]
        self.val = torch.full((max(max_epochs, 1), E, 3), float("nan"), dtype=torch.float32, device=dev)
        self.best_loss = torch.full((E,), float("inf"), dtype=torch.float32, device=dev)
        self.best_epoch = torch.full((E,), -1, dtype=torch.int32, device=dev)
        self.stale = torch.zeros(E, dtype=torch.int32, device=dev)
        self.epochs = 0
        self.native = None
        if _NativeEval.supported(members, holdout, self.ins, self.outs) and \
                (not nll or _NativeEnsembleNll.bounds_shared(members)):
            from . import _lib
            self.native = _NativeEval(members, self.ins, self.outs, H)
            self.row_err = torch.empty((3, E, R, H) if nll else (E, R, H), dtype=torch.float32, device=dev)
            count = len(self.params[0])
            self.table = (_lib.CopyTensor * (E * count))()
            for e in range(E):
                for i, (p, snap) in enumerate(zip(self.params[e], self.snaps[e])):
                    t = self.table[e * count + i]
                    t.src, t.dst, t.numel = p.data_ptr(), snap.data_ptr(), p.numel()
            self.count = count

    def record(self, k):
        """Epoch k has been enqueued (or has run): evaluate, keep the best."""
        E = len(self.members)
        if self.native is not None:
            nat, P = self.native, ctypes.c_void_p
            if self.nll:
                nat.run_nll(self.rows, self.row_err, self.val[k])
            elif self.open_loop:
                nat.run_open_loop(self.rows, self.row_err, self.val[k])
            else:
                nat.run(self.rows, self.row_err, self.val[k])
            nat._lib.check(nat.lib.mbrl_keep_best(P(self.val[k].data_ptr()), 3, E, int(k), P(self.best_loss.data_ptr()),
                                                  P(self.best_epoch.data_ptr()), P(self.stale.data_ptr()), self.table,
                                                  self.count, nat._lib.stream_handle(self.dev)), "mbrl_keep_best")
        else:
            if self.nll:
                row_err = _eval_members_nll_torch(self.members, self.ins, self.outs, self.rows)[0]
            elif self.open_loop:
                row_err = _eval_members_open_loop_torch(self.members, self.ins, self.outs, self.rows)[0]
            else:
                row_err = _eval_members_torch(self.members, self.ins, self.outs, self.rows)
            state = (row_err.sum(1) / (row_err.shape[1] * self.state_dim)).sum(1)
            self.val[k, :, 0] = state
            self.val[k, :, 1] = state
            self.val[k, :, 2] = 0
            better = state < self.best_loss
            self.best_loss = torch.where(better, state, self.best_loss)
            self.best_epoch = torch.where(better, torch.full_like(self.best_epoch, k), self.best_epoch)
            self.stale = torch.where(better, torch.zeros_like(self.stale), self.stale + 1)
            with torch.no_grad():
                for e in np.flatnonzero(better.cpu().numpy()):
                    for p, snap in zip(self.params[e], self.snaps[e]):
                        snap.copy_(p)
        self.epochs = k + 1

    def stop(self, k, patience, check_every):
        if patience is None or (k + 1) % check_every != 0:
            return False
        return int(self.stale.min().item()) >= patience      # (the one host read a patience costs)


class ModelWithReward(nn.Module):
    """models.py:125-163: a shared Linear-ReLU trunk, state head and reward head. `n_hidden`
    generalises the reference's 2-layer trunk. Layers are linear1..linear{n_hidden} (trunk),
    linear{n_hidden+1} (state head) and linear{n_hidden+2} (reward head). n_hidden=2 gives the
    reference's names, so state_dicts load both ways.

    The planners take RewardAgent's wiring (agents.py:342-362) on the fused path: the model closure
    compose(partial(model, ...), itemgetter(0)) and the cost closure compose(partial(model, ...),
    itemgetter(1)). The cost is the unnormalised reward head at (s_{t+1}, a_t)."""

    def __init__(self, state_dim, action_dim, hidden_units=200, n_hidden=2):
        super().__init__()
        self.train_iterations = 0
        self.state_dim, self.action_dim = state_dim, action_dim
        self.hidden_units, self.n_hidden = hidden_units, n_hidden
        dims = [state_dim + action_dim] + [hidden_units] * n_hidden
        for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
            setattr(self, f"linear{i + 1}", nn.Linear(fi, fo))
        setattr(self, f"linear{n_hidden + 1}", nn.Linear(hidden_units, state_dim))
        setattr(self, f"linear{n_hidden + 2}", nn.Linear(hidden_units, 1))
        self.activation_fn = nn.ReLU()

    def linears(self):
        """Trunk layers, state head, reward head (the packing order of mbrl_mlp_pack)."""
        m = self._modules
        return [m[f"linear{i + 1}"] for i in range(self.n_hidden + 2)]

    def _forward(self, x):
        lins = self.linears()
        for lin in lins[:self.n_hidden]:
            x = self.activation_fn(lin(x))
        return lins[-2](x), lins[-1](x)

    def train_model(self, dataset, optimizer, batch_size=512, num_epochs=50, criterion=None, writer=None):
        """models.py:165-217: state loss + reward loss per horizon step."""
        criterion = criterion or torch.nn.MSELoss()

        def step_loss(inp, out):
            (states, actions), (rewards, next_states) = inp, out
            s_hat, r_hat = self.forward(states, actions, normalize_action=None, normalize_state=None,
                                        unnormalize_state=None, unnormalize_reward=None)
            return [criterion(s_hat, next_states), criterion(r_hat, rewards.reshape(-1, 1))]
        _train_loop(self, dataset, optimizer, batch_size, num_epochs, step_loss, writer,
                    ["loss/state/{}", "loss/reward/{}"], criterion)

    def forward(self, state, action, normalize_state=None, unnormalize_state=None, normalize_action=None,
                unnormalize_reward=None):
        if normalize_action:
            action = normalize_action(action)
        if normalize_state:
            state = normalize_state(state)
        x = torch.cat([state, action], dim=1)
        state, reward = self._forward(x)
        if unnormalize_reward:
            reward = unnormalize_reward(reward)
        if unnormalize_state:
            state = unnormalize_state(state)
        return state, reward


class CostModel(nn.Module):
    """models.py:220-234: a learned cost of (state, action), two ReLU layers and a scalar head."""

    def __init__(self, state_dim, action_dim, hidden_units=70):
        super().__init__()
        self.linear1 = nn.Linear(state_dim + action_dim, hidden_units)
        self.linear2 = nn.Linear(hidden_units, hidden_units)
        self.linear3 = nn.Linear(hidden_units, 1)
        self.activation_fn = nn.ReLU()

    def forward(self, state, action):
        x = torch.cat((state, action), -1)
        x = self.activation_fn(self.linear1(x))
        x = self.activation_fn(self.linear2(x))
        return self.linear3(x)


class StateCost(nn.Module):
    goal_state = None

    def set_goal_state(self, goal_state):
        self.goal_state = goal_state


class SmoothAbsLoss(StateCost):
    """models.py:244-259: sum_d sqrt((w_d (x_d - g_d))^2 + alpha^2) - alpha."""

    def __init__(self, weights, goal_state, alpha=0.4):
        super().__init__()
        self.alpha = alpha
        self.weights = weights
        self.goal_state = goal_state

    def forward(self, x):
        x = x - self.goal_state
        return torch.sum(torch.sqrt((x * self.weights) ** 2 + self.alpha ** 2) - self.alpha, dim=-1)


class QuadraticCost(StateCost):
    """models.py:275-288: (x - g) . L(x - g) with a learned Linear L on the state. The reference's
    forward reads `self.goalState`, an attribute it never sets, so it raises AttributeError; this
    restatement computes what the code spells out with the goal it stores (`goal_state`)."""

    def __init__(self, dim, goal_state):
        super().__init__()
        self.linear = nn.Linear(dim, dim)
        self.goal_state = goal_state

    def forward(self, x):
        d = x - self.goal_state
        return torch.dot(d, self.linear(d))


class CoshLoss(nn.Module):
    """models.py:262-272: alpha^2 * mean_d(cosh(a_d / alpha) - 1)."""

    def __init__(self, alpha=0.25):
        super().__init__()
        self.alpha = alpha

    def forward(self, x):
        return (self.alpha ** 2) * torch.mean(torch.cosh(x / self.alpha) - 1, dim=-1)


def state_action_cost(state, action, state_cost, action_cost):
    """agents.py:182-183."""
    return state_cost(state) + action_cost(action)


def compose(a, b):
    """agents.py:300-304."""
    def ab(*args, **kwargs):
        return b(a(*args, **kwargs))
    return ab


def goal_state_cost(state_cost, action_cost):
    """The cost GoalStateAgent hands the planner (agents.py:231)."""
    return functools.partial(state_action_cost, state_cost=state_cost, action_cost=action_cost)
