"""Row kernels between the GEMMs: LayerNorm with its fused residual / dropout variants, dropout (+ residual), the gradient fan-in
(add_n, fanout) and range fills.  Kernels: csrc/layernorm.hip, csrc/dropout_act.hip, csrc/glue.hip."""
import ctypes
import os

import torch

from . import _lib
from ._plumbing import _dt, _need_gpu, _rows, launch
from .gradsink import _first_touch, _prep_fallback, _sink
from .rng import RngState
from .wgrad_queue import LnReduceQueue


# ----------------------------------------------------------------------------- LayerNorm / dropout
LN_DETERMINISTIC = os.environ.get('GOAT_LN_DETERMINISTIC', '0') == '1'
LN_ATOMIC_MAX_ROWS = int(os.environ.get('GOAT_LN_ATOMIC_MAX_ROWS', '4096'))


class _LnFn(torch.autograd.Function):
    """y = LayerNorm(residual + dropout_p(x)) (P/model/Bert_backbone.py:306-310).
    fork=True returns y twice (two autograd outputs over one buffer): one for the next sub-layer's first Linear, one for
    the next LayerNorm's residual input.  Their gradients then reach backward() separately and the kernel sums them on
    load (goat_ln_bwd's dy2), which replaces the elementwise add autograd would otherwise launch for the shared tensor."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, p, fork=False, fork_in=False, z_out=False, p_out=0.0, post_add=None):
        _need_gpu(x)
        ctx.set_materialize_grads(False)
        if fork_in and (fork or residual is not None):
            raise ValueError('fork_in is for the plain LayerNorm(x) of a pre-LN block')
        if z_out and (fork or fork_in or residual is None):
            raise ValueError('z_out returns the pre-norm sum residual + dropout(x): it needs a residual')
        ctx.fork_in, ctx.z_out = fork_in, z_out
        H = x.shape[-1]
        x2 = _rows(x)
        r2 = _rows(residual) if residual is not None else None
        M = x2.shape[0]
        y = torch.empty_like(x2)
        need_z = (r2 is not None) or p > 0
        z = torch.empty_like(x2) if need_z else None
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        rstd = torch.empty(M, dtype=torch.float32, device=x.device)
        seed, off, dev = RngState.draw(p, x2.numel())
        off_out = 0
        if p_out > 0:                        # dropout on the output: a second counter range of the same stream
            s2, off_out, d2 = RngState.next(x2.numel())
            if p > 0:
                assert s2 == seed
            seed, dev = s2, d2
        pa = None
        if post_add is not None:             # y = dropout_out(LayerNorm(z) + post_add)
            pa = _rows(post_add, x2.dtype)
        ctx.has_post = pa is not None
        launch('goat_ln_fwd_do', _dt(x2), x2, r2, gamma, beta, eps, p, seed, off, dev, y, z, mean, rstd, M, H, p_out, off_out, pa)
        ctx.save_for_backward(z if z is not None else x2, gamma, mean, rstd)
        ctx.rng = (p, seed, off, dev)
        ctx.out_drop = (p_out, off_out)
        ctx.has_res = residual is not None
        ctx.gb = (gamma, beta)
        ctx.shape = x.shape
        yv = y.view(x.shape)
        if z_out:       # second output: the pre-norm sum z = residual + dropout(x), the hidden state of a pre-LN stack; the gradient it
            return yv, z.view(x.shape)      # collects behind this LayerNorm comes back to THIS node (GOAT_LN_ADD_BEFORE)
        if fork_in:     # second output: x itself for the skip connection; its gradient comes back to THIS node (dx_add of the kernel)
            return yv, x.view_as(x)
        return (yv, yv.view_as(yv)) if fork else yv

    @staticmethod
    def backward(ctx, dy, dyb=None):
        dskip = None
        if ctx.fork_in or ctx.z_out:
            dskip, dyb = dyb, None
            if dy is None and ctx.fork_in:     # only the skip connection carried a gradient
                return dskip, None, None, None, None, None, None, None, None, None, None
        z, gamma, mean, rstd = ctx.saved_tensors
        if dy is None:
            if ctx.z_out:                      # the normalised output went unused: only the pre-norm sum carried a gradient
                dy = torch.zeros(ctx.shape, dtype=z.dtype, device=z.device)
            else:
                dy, dyb = dyb, None
        p, seed, off, dev = ctx.rng
        H = z.shape[-1]
        dy2 = _rows(dy)
        if dskip is not None:
            dskip = _rows(dskip, z.dtype)
        if dyb is not None:
            dyb = _rows(dyb, dy2.dtype)
        M = z.shape[0]
        dx = torch.empty_like(z)
        dres = torch.empty_like(z) if (ctx.has_res and p > 0) else None
        # gradient of the summand behind the norm: the (masked) dy — without output dropout it IS dy: handed on as such, no copy
        post_alias = ctx.has_post and ctx.out_drop[0] == 0.0 and dyb is None
        dpost = torch.empty_like(z) if (ctx.has_post and not post_alias) else None
        sg, sb = _sink(ctx.gb[0]), _sink(ctx.gb[1])
        sunk = sg is not None and sb is not None
        if not sunk:
            _prep_fallback(*ctx.gb)
        dg = sg if sunk else torch.empty(H, dtype=torch.float32, device=z.device)
        db = sb if sunk else torch.empty(H, dtype=torch.float32, device=z.device)
        # LN_DETERMINISTIC: per-block partials in a workspace + a second (reduction) launch; default: the blocks add their column
        # partials to dgamma / dbeta with float atomics (43 fewer launches per step; summation order is not reproducible)
        # (measured, scripts/ln_bench.py: atomics 15.8 vs 16.7 us at 3840 rows and one launch fewer; 26.3 vs 22.2 us at 8640 rows)
        acc = int(sunk and not _first_touch(*ctx.gb))
        defer = acc == 1 and LnReduceQueue.enabled and M >= LnReduceQueue.MIN_ROWS
        if defer:       # arena slices (pre-zeroed, accumulating): leave the column partials behind, one reduction per backward pass
            nparts = _lib.lib().goat_ln_bwd_nparts(M)
            ws = torch.empty(nparts * 2 * H, dtype=torch.float32, device=z.device)
            acc = 2
        else:
            ws = torch.empty(_lib.lib().goat_ln_bwd_ws_floats(H), dtype=torch.float32, device=z.device) if (LN_DETERMINISTIC or M > LN_ATOMIC_MAX_ROWS) else None
        launch('goat_ln_bwd_do', _dt(z), dy2, dyb, z, gamma, mean, rstd, p, seed, off, dev, dx, dres, dg, db, ws, M, H,
               acc | (4 if (ctx.z_out and dskip is not None) else 0), dskip, ctx.out_drop[0], ctx.out_drop[1], dpost)
        if defer:
            LnReduceQueue.push(ws, dg, db, nparts, H)
        if sunk:
            dg = db = None
        dxv = dx.view(ctx.shape)
        if ctx.has_res:
            dr = dres.view(ctx.shape) if dres is not None else dxv
        else:
            dr = None
        return dxv, dr, dg, db, None, None, None, None, None, None, (dy2.view(ctx.shape) if post_alias else (dpost.view(ctx.shape) if dpost is not None else None))


def layer_norm(x, gamma, beta, eps, residual=None, p=0.0, fork=False, fork_in=False, z_out=False, p_out=0.0, post_add=None):
    """fork_in=True (pre-LN blocks): returns (LayerNorm(x), x) — use the second output for the skip connection; the gradient it
    receives is added inside the LayerNorm backward kernel instead of by an autograd add.
    z_out=True (pre-LN blocks, with residual): returns (LayerNorm(z), z) with z = residual + dropout_p(x) — the residual junction in
    FRONT of the LayerNorm and the LayerNorm in one launch per direction; z continues as the block's hidden state and the gradient
    it collects later joins inside this LayerNorm's backward kernel.
    p_out: dropout on the LayerNorm's output in the same launch (the embedding blocks' dropout(LayerNorm(e)));
    post_add: a summand added behind the norm and in front of that dropout: dropout(LayerNorm(z) + post_add)."""
    return _LnFn.apply(x, residual, gamma, beta, float(eps), float(p), bool(fork), bool(fork_in), bool(z_out), float(p_out), post_add)


# ----------------------------------------------------------------------------- gradient fan-in / fills (csrc/glue.hip)
FANOUT = os.environ.get('GOAT_NO_FANOUT', '0') != '1'        # (diagnostics: A/B against the autograd engine's pairwise adds)


def add_n(tensors, out=None):
    """out = sum(tensors) (same shape / dtype, contiguous), float32 accumulation, one launch (goat_add_n)."""
    ts = [t.contiguous() for t in tensors]
    out = torch.empty_like(ts[0]) if out is None else out
    while len(ts) > 8:                       # (never on the GOAT paths: at most 7 consumers)
        head = add_n(ts[:8])
        ts = [head] + ts[8:]
    arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    launch('goat_add_n', _dt(ts[0]), arr, len(ts), out, ts[0].numel())
    return out


class _FanoutFn(torch.autograd.Function):
    """n autograd handles on ONE buffer; backward = the sum of the handles' gradients in one launch."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [g for g in grads if g is not None]
        if not gs:
            return None, None
        if len(gs) == 1:
            return gs[0], None
        dt = gs[0].dtype
        gs = [g if g.dtype == dt else g.to(dt) for g in gs]
        return add_n(gs), None


def fanout(x, n):
    """A tensor with n consumers: returns n handles on x's buffer, one per consumer.  Their gradients meet in ONE goat_add_n launch
    (float32 accumulation) instead of n - 1 pairwise `add` kernels issued by the autograd engine as the gradients trickle in."""
    if n <= 1 or not FANOUT or not (torch.is_tensor(x) and x.requires_grad and x.is_cuda):
        return [x] * max(n, 1)
    return list(_FanoutFn.apply(x, n))


def fanout_tree(obj, n):
    """fanout() over every tensor of a nested list / tuple / dict: -> list of n objects of the same structure (the K|V projections of an
    instruction, read by every step of a navigation episode: their gradients meet in one launch per tensor instead of T - 1 adds)."""
    if torch.is_tensor(obj):
        return fanout(obj, n)
    if isinstance(obj, dict):
        parts = {k: fanout_tree(v, n) for k, v in obj.items()}
        return [{k: parts[k][i] for k in obj} for i in range(n)]
    if isinstance(obj, (list, tuple)):
        parts = [fanout_tree(v, n) for v in obj]
        return [type(obj)(p[i] for p in parts) for i in range(n)]
    return [obj] * n


def zero_ranges(tensors):
    """clear up to 16 contiguous tensors (16-byte aligned, sizes multiples of 16 bytes) per launch (goat_zero_ranges)."""
    ts = [t for t in tensors if t.numel()]
    for i in range(0, len(ts), 16):
        grp = ts[i:i + 16]
        if any((t.data_ptr() & 15) or ((t.numel() * t.element_size()) & 15) or not t.is_contiguous() or not t.is_cuda for t in grp):
            for t in grp:
                t.zero_()
            continue
        ptrs = (ctypes.c_void_p * len(grp))(*[t.data_ptr() for t in grp])
        nb = (ctypes.c_int64 * len(grp))(*[t.numel() * t.element_size() for t in grp])
        launch('goat_zero_ranges', ptrs, nb, len(grp))


class _DropAddFn(torch.autograd.Function):
    """y = residual + dropout_p(x)."""

    @staticmethod
    def forward(ctx, x, residual, p):
        _need_gpu(x)
        xc = x.contiguous()
        rc = None
        if residual is not None:
            rc = residual.contiguous()
        y = torch.empty_like(xc)
        seed, off, dev = RngState.draw(p, xc.numel())
        launch('goat_dropout_add_fwd', _dt(xc), xc, rc, y, xc.numel(), p, seed, off, dev)
        ctx.rng = (p, seed, off, dev)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed, off, dev = ctx.rng
        dyc = dy.contiguous()
        if p > 0:
            dx = torch.empty_like(dyc)
            launch('goat_dropout_bwd', _dt(dyc), dyc, dx, dyc.numel(), p, seed, off, dev)
        else:
            dx = dyc
        return dx, (dyc if ctx.has_res else None), None


def dropout_add(x, residual, p):
    if p <= 0 and residual is None:
        return x
    return _DropAddFn.apply(x, residual, float(p))


def dropout(x, p):
    return dropout_add(x, None, p)
