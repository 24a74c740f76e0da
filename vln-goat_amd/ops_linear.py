"""The Linear family on top of the GEMM dispatcher: Linear (+ activation), the Linear(H, 1) row dot, the two-GEMM FFN, the tied
decoder + cross-entropy of the MLM head, and the projections that share one GEMM (multi_linear, linear_bank)."""
import os

import torch

from ._lib import EPI_GELU, EPI_MUL_DGELU, EPI_MUL_DRELU, EPI_NONE, EPI_RELU
from ._plumbing import _dt, _epc, _need_gpu, _rows, launch
from .gradsink import _first_touch, _prep_fallback, _sink, small_sinks
from .ops_gemm import gemm, linear_wgrad, wgrad
from .rng import RngState
from .shadows import _bias_padded, _cat_bias, _shadow, _shadow_cat, _shadow_rows_padded

_ACT_EPI = {None: EPI_NONE, 'none': EPI_NONE, 'gelu': EPI_GELU, 'relu': EPI_RELU}
_ACT_DEPI = {'gelu': EPI_MUL_DGELU, 'relu': EPI_MUL_DRELU}


def _pad_k(x, e):
    K = x.shape[1]
    pad = (-K) % e
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
    return x, pad


SMALLK_WGRAD = os.environ.get('GOAT_NO_SMALLK', '0') != '1'       # (diagnostics: A/B of the short-input weight-gradient kernel)


class _LinearFn(torch.autograd.Function):
    """y = act(x @ W^T + b)   (F.linear + activation; P/model/Bert_backbone.py:302,348-357,362)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, out_dtype):
        _need_gpu(x)
        x2 = x.reshape(-1, x.shape[-1])
        if not x2.is_contiguous() and not (x2.dim() == 2 and x2.stride(1) == 1 and x2.stride(0) % 8 == 0 and x2.data_ptr() % 16 == 0
                                           and x2.dtype == torch.bfloat16 and x2.shape[1] % 64 == 0
                                           and x2.shape[0] * x2.stride(0) * 2 < (1 << 31)):      # (the GEMM's operand window spans rows * lda: < 2 GiB)
            x2 = x2.contiguous()          # (a row-strided view — the [CLS] rows hidden[:, 0] of a pooler — goes to the GEMM as it is: lda = its row stride)
        Kw = weight.shape[1]
        if x2.shape[1] == Kw:
            x2, pad = _pad_k(x2, _epc(x2))
            prepad = False
        else:
            # input already K-padded with zero columns to the GEMM's 16-byte chunk (train_step.prepare_position_features: the 7- / 14-wide
            # position features are cast and padded ONCE per batch on the host instead of by two launches per Linear and step)
            pad = (-Kw) % _epc(x2)
            if x2.shape[1] != Kw + pad:
                raise ValueError('linear: input width %d matches neither the weight (%d) nor its padded width (%d)' % (x2.shape[1], Kw, Kw + pad))
            prepad = True
        w = _shadow(weight, x2.dtype, False, pad)
        N = w.shape[0]
        out = torch.empty((x2.shape[0], N), dtype=out_dtype or x2.dtype, device=x2.device)
        aux = None
        epi = _ACT_EPI[act]
        if epi != EPI_NONE and (ctx.needs_input_grad[0] or weight.requires_grad):
            aux = torch.empty_like(out)
        gemm(x2, w, out, bias=bias.detach() if bias is not None else None, epi=epi, aux=aux)
        ctx.save_for_backward(x2, aux)
        ctx.weight, ctx.bias, ctx.has_bias, ctx.act, ctx.pad, ctx.xshape, ctx.prepad = weight, bias, bias is not None, act, pad, x.shape, prepad
        return out.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, aux = ctx.saved_tensors
        weight = ctx.weight
        dy2 = _rows(dy, x2.dtype)
        if ctx.act not in (None, 'none'):
            dy2 = act_bwd(dy2, aux, ctx.act)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            w = _shadow(weight, x2.dtype, False, ctx.pad)  # [N, Kp]
            dx = torch.empty_like(x2)
            gemm(dy2, w, dx, ta=False, tb=True)        # dx[M,Kp] = dy[M,N] @ W[N,Kp]
            if ctx.pad and not ctx.prepad:
                dx = dx[:, :x2.shape[1] - ctx.pad]
            dx = dx.reshape(ctx.xshape)
        if SMALLK_WGRAD and ctx.pad and x2.shape[1] - ctx.pad <= 16 and (ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])):
            # short-input Linear (7- / 14-wide position features, K padded to a 16-byte chunk for the GEMM): one kernel adds the
            # weight and bias gradients straight into the arena slices (otherwise: padded GEMM into a temporary, slice copy, grad += dW)
            K = x2.shape[1] - ctx.pad
            sinks = small_sinks((weight, ctx.bias) if ctx.has_bias else (weight,))
            if sinks is not None:
                dwt, dbt = sinks[0], (sinks[1] if ctx.has_bias else None)
            else:
                dwt = torch.zeros(weight.shape, dtype=torch.float32, device=dy2.device)
                dbt = torch.zeros(weight.shape[0], dtype=torch.float32, device=dy2.device) if ctx.has_bias else None
            launch('goat_wgrad_smallk', _dt(dy2), dy2, dy2.stride(0), x2, x2.stride(0), dy2.shape[0], dy2.shape[1], K, dwt, dwt.stride(0), dbt)
            if sinks is None:
                dw, db = dwt, dbt
        elif ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            if ctx.pad:           # K-padded input: dW comes out padded — through a temporary, never into the sink
                _prep_fallback(weight, ctx.bias)
                dw, db = wgrad(dy2, x2, ctx.has_bias)
                dw = dw[:, :x2.shape[1] - ctx.pad].contiguous()
            else:
                dw, db = linear_wgrad(dy2, x2, (weight,), (ctx.bias,), ctx.has_bias)
        return dx, dw, db, None, None


class _RowDotFn(torch.autograd.Function):
    """y[..., 0] = x[..., :] . w + b for a Linear(H, 1) (the last layer of ClsPrediction, P/model/pretrain_goat.py:27-38) without the GEMM
    machinery: goat_rowdot_fwd / _bwd (one wave per row; dW / db by block partials + atomics straight into the arena slices)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x)
        x2 = _rows(x)
        M, H = x2.shape
        y = torch.empty(M, dtype=x2.dtype, device=x2.device)
        launch('goat_rowdot_fwd', _dt(x2), x2, weight, bias, y, M, H)
        ctx.save_for_backward(x2)
        ctx.weight, ctx.bias, ctx.xshape = weight, bias, x.shape
        return y.view(*x.shape[:-1], 1)

    @staticmethod
    def backward(ctx, dy):
        x2, = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        M, H = x2.shape
        dy2 = dy.reshape(-1)
        if dy2.dtype != x2.dtype:
            dy2 = dy2.to(x2.dtype)
        dy2 = dy2.contiguous()
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        need_w = ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2])
        dw = db = dwt = dbt = None
        if need_w:
            sinks = small_sinks((weight, bias) if bias is not None else (weight,))
            if sinks is not None:
                dwt, dbt = sinks[0], (sinks[1] if bias is not None else None)
            else:
                buf = torch.zeros(H + 1, dtype=torch.float32, device=x2.device)
                dwt, dbt = buf[:H], (buf[H:] if bias is not None else None)
                dw, db = dwt.view(weight.shape), (dbt.view(bias.shape) if bias is not None else None)
        launch('goat_rowdot_bwd', _dt(x2), x2, weight, dy2, dx, dwt, dbt, M, H)
        return (dx.view(ctx.xshape) if dx is not None else None), dw, db


ROWDOT = os.environ.get('GOAT_NO_ROWDOT', '0') != '1'        # (diagnostics: Linear(H, 1) through the GEMM path again)


def linear(x, weight, bias=None, act=None, out_dtype=None):
    if (ROWDOT and weight.shape[0] == 1 and act in (None, 'none') and out_dtype is None and x.is_cuda and x.shape[-1] == weight.shape[1]
            and weight.shape[1] % 8 == 0 and weight.shape[1] <= 1024 and weight.dtype == torch.float32 and weight.is_contiguous()
            and (bias is None or bias.dtype == torch.float32) and x.dtype in (torch.float32, torch.bfloat16)):
        return _RowDotFn.apply(x, weight, bias)
    return _LinearFn.apply(x, weight, bias, act, out_dtype)


def act_bwd(dy, u, act, p=0.0, rng=(0, 0, None)):
    """dx = dropmask_p(dy) * act'(u)  (goat_act_bwd)."""
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    launch('goat_act_bwd', _dt(dy), dy, u, dx, dy.numel(), _ACT_EPI[act], p, rng[0], rng[1], rng[2])
    return dx


class _FfnFn(torch.autograd.Function):
    """y = dropout_p(act(x @ W1^T + b1)) @ W2^T + b2.  With p == 0 (BERT blocks: BertIntermediate +
    BertOutput.dense, P/model/Bert_backbone.py:345-368) the activation derivative is fused into the dgrad
    GEMM epilogue; with p > 0 (panorama encoder FFN, P/model/transformer.py:179) one elementwise kernel
    applies mask and derivative."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act, p):
        _need_gpu(x)
        x2 = _rows(x)
        W1 = _shadow(w1, x2.dtype)
        W2 = _shadow(w2, x2.dtype)
        M, F_ = x2.shape[0], W1.shape[0]
        u = torch.empty((M, F_), dtype=x2.dtype, device=x2.device)
        h = torch.empty_like(u)
        rng = RngState.draw(p, h.numel())
        gemm(x2, W1, h, bias=b1.detach(), epi=_ACT_EPI[act], aux=u)
        if p > 0:
            launch('goat_dropout_add_fwd', _dt(h), h, None, h, h.numel(), p, rng[0], rng[1], rng[2])
        y = torch.empty((M, W2.shape[0]), dtype=x2.dtype, device=x2.device)
        gemm(h, W2, y, bias=b2.detach())
        ctx.save_for_backward(x2, u, h)
        ctx.w1, ctx.w2, ctx.act, ctx.xshape, ctx.p, ctx.rng = w1, w2, act, x.shape, p, rng
        ctx.b1, ctx.b2 = b1, b2
        return y.view(*x.shape[:-1], W2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, u, h = ctx.saved_tensors
        dy2 = _rows(dy)
        W2 = _shadow(ctx.w2, x2.dtype)  # [H, F]
        du = torch.empty_like(u)
        if ctx.p > 0:
            gemm(dy2, W2, du, tb=True)
            du = act_bwd(du, u, ctx.act, ctx.p, ctx.rng)
        else:
            gemm(dy2, W2, du, tb=True, epi=_ACT_DEPI[ctx.act], aux=u)
        dw2, db2 = linear_wgrad(dy2, h, (ctx.w2,), (ctx.b2,))
        W1 = _shadow(ctx.w1, x2.dtype)  # [F, H]
        dx = torch.empty_like(x2)
        gemm(du, W1, dx, tb=True)
        dw1, db1 = linear_wgrad(du, x2, (ctx.w1,), (ctx.b1,))
        return dx.view(ctx.xshape), dw1, db1, dw2, db2, None, None


def ffn(x, w1, b1, w2, b2, act='gelu', p=0.0):
    return _FfnFn.apply(x, w1, b1, w2, b2, act, float(p))


# ----------------------------------------------------------------------------- tied decoder + cross-entropy (MLM)
def _ce_rows_fwd(logits, ld, n_valid, targets):
    """loss[m], lse[m] (float32) of the float32 logits[m, :n_valid] at leading dimension ld against targets[m] (goat_ce_fwd)."""
    M = logits.shape[0]
    loss = torch.empty(M, dtype=torch.float32, device=logits.device)
    lse = torch.empty(M, dtype=torch.float32, device=logits.device)
    launch('goat_ce_fwd', logits, ld, M, n_valid, targets, loss, lse)
    return loss, lse


def _ce_rows_bwd(logits, ld, n_valid, targets, lse, dloss, dtype):
    """-> dl[M, ld] in `dtype`: the gradient of the logits for the loss gradient dloss[M] (goat_ce_bwd; lse from _ce_rows_fwd)."""
    M = logits.shape[0]
    dl = torch.empty((M, ld), dtype=dtype, device=logits.device)
    launch('goat_ce_bwd', _dt(dl), logits, ld, M, n_valid, targets, lse, dloss.float().contiguous(), dl, ld)
    return dl


class _DecoderCeFn(torch.autograd.Function):
    """loss[m] = CE(h[m] @ W^T + b, target[m])  — BertLMPredictionHead.decoder + F.cross_entropy
    (P/model/Bert_backbone.py:826-829, P/model/pretrain_goat.py:210-216).  The vocabulary dimension is padded
    to a multiple of 64 (zero weight rows) so the logits GEMM, its dgrad (contraction over the vocabulary,
    split-K) and its wgrad all run on the LDS-DMA kernel; cross-entropy forward/backward are two row kernels
    that never materialise a softmax."""

    @staticmethod
    def forward(ctx, h, weight, bias, targets):
        _need_gpu(h)
        h2 = _rows(h)
        M, K = h2.shape
        N = weight.shape[0]
        Np = (N + 63) // 64 * 64
        W = _shadow_rows_padded(weight, h2.dtype, Np)
        Nl = W.shape[0]
        bpad = _bias_padded(bias, Nl)
        logits = torch.empty((M, Nl), dtype=torch.float32, device=h.device)
        gemm(h2, W, logits, bias=bpad)
        tg = targets.contiguous()
        loss, lse = _ce_rows_fwd(logits, Nl, N, tg)
        ctx.save_for_backward(h2, logits, lse, tg)
        ctx.weight, ctx.bias, ctx.N, ctx.hshape = weight, bias, N, h.shape
        return loss

    @staticmethod
    def backward(ctx, dloss):
        h2, logits, lse, tg = ctx.saved_tensors
        weight, N = ctx.weight, ctx.N
        M, K = h2.shape
        Nl = logits.shape[1]
        dl = _ce_rows_bwd(logits, Nl, N, tg, lse, dloss, h2.dtype)
        if h2.dtype == torch.bfloat16:
            W = _shadow_rows_padded(weight, h2.dtype, Nl)
            dh32 = torch.zeros((M, K), dtype=torch.float32, device=h2.device)
            gemm(dl, W, dh32, tb=True, split_k=8, split_opts=(4, 6, 8, 12, 16))     # contraction over the vocabulary
            dh = dh32.to(h2.dtype)
        else:
            dh = torch.empty_like(h2)
            gemm(dl, _shadow_rows_padded(weight, h2.dtype, Nl), dh, tb=True)
        # (not through linear_wgrad: whether the weight is sunk decides which columns of dl are the problem, before anything else happens)
        w_sink = _sink(weight)
        if w_sink is not None:      # the tied word-embedding table: accumulate next to the embedding scatter-add
            b_sink = _sink(ctx.bias)
            first = _first_touch(weight)
            b_first = b_sink is not None and _first_touch(ctx.bias)
            if b_sink is None:
                _prep_fallback(ctx.bias)
            dw, db = wgrad(dl[:, :N], h2, True, w_sink, b_sink, first, b_first, [id(weight), id(ctx.bias)])
            return dh.view(ctx.hshape), None, db, None
        _prep_fallback(weight, ctx.bias)
        dw, db = wgrad(dl, h2, True)
        return dh.view(ctx.hshape), dw[:N], db[:N], None


def decoder_cross_entropy(h, weight, bias, targets):
    return _DecoderCeFn.apply(h, weight, bias, targets)


# ----------------------------------------------------------------------------- fused multi-weight projection
def _cat_fwd(x, ws, bs):
    """-> (x2, out): the rows of x and out[rows, sum of the W_i's rows] = x2 @ cat(W_i)^T + cat(b_i), one GEMM over the concatenated shadows."""
    _need_gpu(x)
    x2 = _rows(x)
    W = _shadow_cat(ws, x2.dtype)
    b = _cat_bias(bs)
    out = torch.empty((x2.shape[0], W.shape[0]), dtype=x2.dtype, device=x2.device)
    gemm(x2, W, out, bias=b)
    return x2, out


def _cat_dgrad(dy2, x2, ws, xshape):
    """dx = dy2 @ cat(W_i), one dgrad over the concatenated contraction, shaped like the input."""
    W = _shadow_cat(ws, x2.dtype)
    dx = torch.empty_like(x2)
    gemm(dy2, W, dx, tb=True)
    return dx.view(xshape)


def _split_grads(dw, db, ws):
    """(dw, db) as linear_wgrad returns them for the run `ws` -> (a list per weight, a list per bias): row blocks, or None for what went
    into a sink."""
    sizes = [w.shape[0] for w in ws]
    none = [None] * len(ws)
    return (list(torch.split(dw, sizes, 0)) if dw is not None else none), (list(torch.split(db, sizes, 0)) if db is not None else none)


class _MultiLinearFn(torch.autograd.Function):
    """y = x @ cat(W_i)^T + cat(b_i): one GEMM for the separate query/key/value Linears of a BERT block
    (P/model/Bert_backbone.py:210,231-232).  Gradients are returned per original parameter."""

    @staticmethod
    def forward(ctx, x, *wb):
        n = len(wb) // 2
        ws, bs = wb[:n], wb[n:]
        x2, out = _cat_fwd(x, ws, bs)
        ctx.save_for_backward(x2)
        ctx.ws, ctx.bs, ctx.xshape = ws, bs, x.shape
        return out.view(*x.shape[:-1], out.shape[1])

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        dy2 = _rows(dy)
        dx = _cat_dgrad(dy2, x2, ctx.ws, ctx.xshape) if ctx.needs_input_grad[0] else None
        dws, dbs = _split_grads(*linear_wgrad(dy2, x2, ctx.ws, ctx.bs), ctx.ws)
        return (dx,) + tuple(dws) + tuple(dbs)


def multi_linear(x, weights, biases):
    return _MultiLinearFn.apply(x, *weights, *biases)


class _GradSlots:
    """One [rows, n * width] gradient buffer shared by the n output views of a projection bank: the consumer of view i (an attention
    backward) writes its gradient straight into columns [i * width, (i + 1) * width) and hands that view back to autograd."""

    def __init__(self, out, n, lead):
        self.buf = torch.empty_like(out)
        self.n, self.width, self.lead = n, out.shape[1] // n, lead

    def view(self, i):
        return self.buf.view(*self.lead, self.buf.shape[1])[..., i * self.width:(i + 1) * self.width]


class _LinearBankFn(torch.autograd.Function):
    """y = x @ cat(W_j)^T + cat(b_j) for the projections of SEVERAL modules that read one activation — the key | value projections of
    every cross-attention layer of the cross-modal encoders on the sequence they all attend to (P/model/Bert_backbone.py:765-781: the same
    `kv_embeds` goes to every layer; P/model/vilmodel_goat.py:501-504,631-647) — as ONE GEMM [rows, n * width] instead of one per layer,
    and in backward ONE dgrad over the concatenated contraction (K = n * width) instead of n dgrads and an n-way add.
    Returns n views [..., width] of the one result (row stride n * width); hipops.attention reads them through strides and writes the
    gradient of view i into its columns of one shared buffer (_GradSlots) — no copies on either side."""

    @staticmethod
    def forward(ctx, x, n, *wb):
        m = len(wb) // 2
        ws, bs = wb[:m], wb[m:]
        x2, out = _cat_fwd(x, ws, bs)
        ctx.save_for_backward(x2)
        ctx.ws, ctx.bs, ctx.xshape, ctx.n = ws, bs, x.shape, n
        need = any(ctx.needs_input_grad)          # (grad mode is off inside forward: the flags say whether a backward pass can come)
        ctx.slots = _GradSlots(out, n, x.shape[:-1]) if need else None
        width = out.shape[1] // n
        full = out.view(*x.shape[:-1], out.shape[1])
        return tuple(full[..., i * width:(i + 1) * width] for i in range(n))

    @staticmethod
    def backward(ctx, *grads):
        (x2,) = ctx.saved_tensors
        ws, n, slots = ctx.ws, ctx.n, ctx.slots
        width = slots.width
        for i, g in enumerate(grads):          # a gradient that is not already in its slot (another producer than attention, a fan-out sum)
            dst = slots.view(i)
            if g is None:
                dst.zero_()
            elif g.data_ptr() != dst.data_ptr() or g.stride() != dst.stride():
                dst.copy_(g)
        dy2 = slots.buf
        dx = _cat_dgrad(dy2, x2, ws, ctx.xshape) if ctx.needs_input_grad[0] else None
        # weight gradients: one problem per run of parameters that are adjacent in the gradient arena (the key | value pair of a layer),
        # reading its columns of the shared gradient buffer through the leading dimension
        per = len(ws) // n
        dws, dbs = [], []
        for i in range(n):
            wi, bi = ws[i * per:(i + 1) * per], ctx.bs[i * per:(i + 1) * per]
            dw, db = _split_grads(*linear_wgrad(dy2[:, i * width:(i + 1) * width], x2, wi, bi), wi)
            dws += dw
            dbs += db
        return (dx, None) + tuple(dws) + tuple(dbs)


LINEAR_BANK = os.environ.get('GOAT_NO_KV_BANK', '0') != '1'       # (diagnostics: A/B against one projection per layer)


def linear_bank(x, groups):
    """groups: n lists of (weight, bias) pairs — the projections of n modules that read x (e.g. [(key, value)] per cross-attention layer).
    -> n views [..., sum of the group's rows] of ONE GEMM result, each carrying `_goat_grad_slot` for its consumer's backward."""
    n = len(groups)
    ws = [w for g in groups for (w, _) in g]
    bs = [b for g in groups for (_, b) in g]
    outs = _LinearBankFn.apply(x, n, *ws, *bs)
    fn = outs[0].grad_fn
    slots = getattr(fn, 'slots', None) if fn is not None else None
    if slots is not None:
        for i, o in enumerate(outs):
            o._goat_grad_slot = (slots, i)
    return list(outs)
