"""Gradient sinks: the protocol by which a backward pass writes a parameter's gradient straight into its gradient-arena slice.

dp.GradArena.attach binds a float32 slice of one flat buffer to every parameter (`_goat_sink`, also its .grad) and bumps
ARENA_EPOCH at the start of a step.  A backward pass then, IN THIS ORDER,
  1. looks the slices up (`_sink` / `_sink_cat`) — which lands a queued write of the slice first (wgrad_queue.WgradQueue),
  2. asks whether it is the first writer of the step (`_first_touch`) — which stamps the epoch and clears the unwritten slices of a
     mixed set — and either overwrites / clears the slice or accumulates,
  3. for every parameter it will hand to autograd as an ordinary gradient instead, clears a stale slice (`_prep_fallback`).
`small_sinks` is that sequence for kernels that add into all their (small) parameters at once; hipops.linear_wgrad is the one for
the weight-gradient GEMMs (it lives beside `wgrad` because it launches through hipops.gemm).  torch only: nothing here launches a
hand-written kernel, so the protocol runs on CPU tensors (tests/test_shadows_sinks.py).
"""
import torch

from .wgrad_queue import WgradQueue


def _sink(param, keep_queued=False):
    """Gradient-arena slice bound to `param` (dp.GradArena.attach), or None.  When it is bound — i.e. still the
    object behind param.grad — backward passes accumulate the parameter's gradient straight into it and return
    None to autograd (no temporary, no zero-fill, no `grad += dW` kernel).  Setting param.grad = None (or to any
    other tensor) silently restores the ordinary autograd path.
    keep_queued: the caller is about to queue ANOTHER weight-gradient problem for this slice on this stream and the two may be merged
    (WgradQueue.mergeable): a queued write of the same stream then stays queued."""
    if param is None:
        return None
    if WgradQueue.pending_ids and id(param) in WgradQueue.pending_ids:
        if not (keep_queued and WgradQueue.pending_ids[id(param)] == torch.cuda.current_stream().cuda_stream):
            WgradQueue.flush_param(id(param))      # a queued write of this slice must land before anything else touches it
    s = param.__dict__.get('_goat_sink')
    return s if (s is not None and param.grad is s) else None


def _sink_cat(params, keep_queued=False):
    """One [sum(rows), ...] view over the arena slices of several parameters if they are adjacent in the arena
    (query/key/value weights of a block), else None."""
    sinks = [_sink(p, keep_queued) for p in params]
    if any(t is None for t in sinks):
        return None
    for a, b in zip(sinks, sinks[1:]):
        if a.data_ptr() + a.numel() * a.element_size() != b.data_ptr() or a.shape[1:] != b.shape[1:]:
            return None
    s0 = sinks[0]
    return torch.as_strided(s0, (sum(t.shape[0] for t in sinks),) + tuple(s0.shape[1:]), s0.stride())


ARENA_EPOCH = [0]       # bumped by dp.GradArena.zero(): a sink's first use in a step overwrites / clears its slice


def _first_touch(*params):
    """True if none of `params` has been written through its sink yet in this step (marks them written).
    Small parameters (`_goat_prezero`: biases, LayerNorm, ...) are cleared by GradArena.zero() at the start of the step:
    they never count as a first touch — writers just accumulate.  Mixed states among the others (some written, some
    not) cannot be served by one kernel launch: the unwritten slices are cleared here and the call is an accumulation."""
    cur = ARENA_EPOCH[0]
    params = [p for p in params if not p.__dict__.get('_goat_prezero')]
    if not params:
        return False
    seen = [p.__dict__.get('_goat_epoch') == cur for p in params]
    for p, was in zip(params, seen):
        p.__dict__['_goat_epoch'] = cur
        if not was and any(seen):
            p.__dict__['_goat_sink'].zero_()
    return not any(seen)


def _prep_fallback(*params):
    """A Function is about to return ordinary gradients for `params` (autograd will add them into .grad): if a
    .grad is an arena slice nobody has written yet in this step it still holds the previous step's values."""
    for p in params:
        t = _sink(p)
        if t is not None and _first_touch(p):
            t.zero_()


def small_sinks(params):
    """All-or-nothing form for a kernel that ADDS the gradients of its few small parameters in one launch.
    Every parameter has a bound sink -> the list of sinks, each cleared if this is its first write of the step (the kernel then adds
    into them and the Function returns None for the parameters).  Otherwise -> None, after _prep_fallback(*params): the caller hands
    the kernel zero-filled temporaries and returns them to autograd.  Either way every bound slice has been cleared on its first
    touch, in the order of `params`, when this returns."""
    sinks = [_sink(p) for p in params]
    if any(s is None for s in sinks):
        _prep_fallback(*params)
        return None
    for p, s in zip(params, sinks):
        if _first_touch(p):
            s.zero_()
    return sinks
