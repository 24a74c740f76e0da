"""Attention: masked multi-head attention on packed projections (training; short and key-streaming kernels) and the KV-cached
decode step with its word selection (inference only; csrc/decode.hip)."""
import math

import torch

from ._plumbing import _dt, _inference_only, _need_gpu, _ptr, launch
from .rng import RngState


ATTN_SHORT_MAXLK = 256      # goat_attn_fwd / goat_attn_bwd (score row-block in registers; the tuned, captured path)
ATTN_MAXLK = 512            # goat_attn_long_fwd / goat_attn_long_bwd (key-streaming forward)


def _attn_entry(Lk):
    """Name stem of the pair of library entry points serving Lk keys (stem + '_fwd' / '_bwd'): the long pair only above the short
    pair's limit, so nothing changes below it."""
    if Lk > ATTN_MAXLK:
        raise ValueError('attention over %d keys: the kernels serve at most %d (max_position_embeddings - 2 of the text encoder)'
                         % (Lk, ATTN_MAXLK))
    return 'goat_attn_long' if Lk > ATTN_SHORT_MAXLK else 'goat_attn'


def _attn_layout(a, b):
    """(pointer, row stride, batch stride) of q, k and v, nine C arguments in a row, and the sizes (B, Lq, Lk, H): of the packed
    projections as _AttnFn takes them, or of gradient buffers laid out like them (b: rows at its own leading dimension)."""
    B, Lq, W = a.shape
    if b is None:
        H = W // 3
        return (_ptr(a), W, Lq * W, _ptr(a, H), W, Lq * W, _ptr(a, 2 * H), W, Lq * W), (B, Lq, Lq, H)
    Lk, ld = b.shape[1], b.stride(1)
    return (_ptr(a), W, Lq * W, _ptr(b), ld, Lk * ld, _ptr(b, W), ld, Lk * ld), (B, Lq, Lk, W)


class _AttnFn(torch.autograd.Function):
    """Masked MHA on packed projections.
    mode 'self' : a = qkv [B,L,3H]              (q|k|v)
    mode 'cross': a = q [B,Lq,H], b = kv [B,Lk,2H]   (k|v)
    kmask: float32 [B,Lk] additive (0 / -10000 / -inf) or None; bias: float32 [B,Lq,Lk] or None."""

    @staticmethod
    def forward(ctx, a, b, kmask, bias, nh, p):
        _need_gpu(a)
        a = a.contiguous()
        slot = None
        if b is not None:
            # a view of a projection bank (linear_bank): rows at the bank's leading dimension; its gradient goes into the bank's buffer
            # (read through its strides; the FIRST consumer of the view claims the slot — a second reader of the same view, e.g. the steps of
            # an eager episode that share one projection of the instruction, gets a buffer of its own and autograd adds the two)
            if b.dim() == 3 and b.stride(2) == 1 and b.stride(0) == b.shape[1] * b.stride(1) and b.stride(1) % 8 == 0 and b.data_ptr() % 16 == 0:
                slot = b.__dict__.pop('_goat_grad_slot', None)
            else:
                b = b.contiguous()
        ctx.slot = slot
        qkv, (B, Lq, Lk, H) = _attn_layout(a, b)
        assert H == nh * 64, 'head_dim must be 64'
        name = _attn_entry(Lk)
        o = torch.empty((B, Lq, H), dtype=a.dtype, device=a.device)
        lse = torch.empty((B, nh, Lq), dtype=torch.float32, device=a.device)
        if kmask is not None:
            kmask = kmask.contiguous().float()
        if bias is not None:
            bias = bias.contiguous().float()
        seed, off, dev = RngState.draw(p, B * nh * Lq * Lk)
        scale = 1.0 / math.sqrt(64.0)
        launch(name + '_fwd', _dt(a), *qkv, o, H, Lq * H, kmask, bias, lse, B, nh, Lq, Lk, scale, p, seed, off, dev,
               what='%s_fwd(Lq=%d,Lk=%d)' % (name, Lq, Lk))
        ctx.save_for_backward(a, b, kmask, bias, o, lse)
        ctx.cfg = (nh, p, seed, off, dev, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        a, b, kmask, bias, o, lse = ctx.saved_tensors
        nh, p, seed, off, dev, scale = ctx.cfg
        do = do.contiguous()
        da = torch.empty_like(a)
        db = None
        if b is not None:
            db = ctx.slot[0].view(ctx.slot[1]) if ctx.slot is not None else torch.empty(b.shape, dtype=b.dtype, device=b.device)
        qkv, (B, Lq, Lk, H) = _attn_layout(a, b)
        dqkv, _ = _attn_layout(da, db)
        dbias = None
        if bias is not None and ctx.needs_input_grad[3]:
            dbias = torch.zeros_like(bias)
        name = _attn_entry(Lk)
        launch(name + '_bwd', _dt(a), *qkv, o, H, Lq * H, do, H, Lq * H, *dqkv, kmask, bias, lse, dbias, B, nh, Lq, Lk, scale, p, seed, off, dev,
               what='%s_bwd(Lq=%d,Lk=%d)' % (name, Lq, Lk))
        return da, db, None, dbias, None, None


def attention(a, b, kmask, bias, nh, p):
    return _AttnFn.apply(a, b, kmask, bias, int(nh), float(p))


# ----------------------------------------------------------------------------- KV-cached decoding (inference only; csrc/decode.hip)
DECODE_MAXL = 512           # goat_attn_decode_fwd: rows of a K|V cache


class DecodeState:
    """The loop state of a KV-cached decode, all in device memory at fixed addresses (goat_decode_select writes it, a captured step
    reads it): words int64 [B, Lmax], kmask float32 [B, Lmax] (-1e9 where the word is <PAD>, else 0), ended uint8 [B],
    end_step int32 [B] (the step at which the row emitted <EOS>, -1 before), pos int32 [1] (the column of the newest word),
    n_live int32 [1] (rows not yet ended)."""

    def __init__(self, B, Lmax, device):
        if not 2 <= Lmax <= DECODE_MAXL:
            raise ValueError('DecodeState: %d columns; the decode kernels serve 2..%d' % (Lmax, DECODE_MAXL))
        self.B, self.Lmax = int(B), int(Lmax)
        self.words = torch.zeros(B, Lmax, dtype=torch.int64, device=device)
        self.kmask = torch.zeros(B, Lmax, dtype=torch.float32, device=device)
        self.ended = torch.zeros(B, dtype=torch.uint8, device=device)
        self.end_step = torch.full((B,), -1, dtype=torch.int32, device=device)
        self.pos = torch.zeros(1, dtype=torch.int32, device=device)
        self.n_live = torch.full((1,), B, dtype=torch.int32, device=device)

    def reset(self, first, pad):
        """Start a new batch of sentences: column 0 = `first` (an int or int64 [B]), everything else as after construction."""
        self.words.fill_(pad)
        self.words[:, 0] = first
        self.kmask.zero_()
        self.kmask[:, 0].masked_fill_(self.words[:, 0] == pad, -1e9)
        self.ended.zero_()
        self.end_step.fill_(-1)
        self.pos.zero_()
        self.n_live.fill_(self.B)


def attn_decode(q, kv_new, cache, kmask, pos, nh, p=0.0):
    """One KV-cached attention step (goat_attn_decode_fwd): with t = pos[0] ON THE DEVICE, cache[:, t] = kv_new and then single-query
    attention of q over the keys 0..t.  q [B, nh*64] (or [B, 1, nh*64]); kv_new [B, 2*nh*64] (K|V); cache [B, Lmax, 2*nh*64] (updated in
    place; the last dimension dense); kmask float32 [B, Lmax] additive or None; pos int32 [1].  -> o, shaped like q.  Inference only."""
    _inference_only('attn_decode', q, kv_new, cache, kmask, pos)
    H = int(nh) * 64
    B, Lmax = cache.shape[0], cache.shape[1]
    if q.numel() != B * H or kv_new.numel() != B * 2 * H or cache.dim() != 3 or cache.shape[2] != 2 * H:
        raise ValueError('attn_decode: q %s / kv_new %s / cache %s do not fit %d heads of 64' % (tuple(q.shape), tuple(kv_new.shape), tuple(cache.shape), nh))
    if not (q.dtype == kv_new.dtype == cache.dtype):
        raise ValueError('attn_decode: q, kv_new and cache must share one dtype')
    if cache.stride(2) != 1:
        raise ValueError('attn_decode: the cache rows must be dense')
    if pos.dtype != torch.int32 or pos.numel() != 1:
        raise ValueError('attn_decode: pos is one int32 on the device')
    if kmask is not None and (kmask.dtype != torch.float32 or tuple(kmask.shape) != (B, Lmax) or not kmask.is_contiguous()):
        raise ValueError('attn_decode: kmask is a contiguous float32 [B, Lmax]')
    for name, t in (('q', q), ('kv_new', kv_new), ('kmask', kmask), ('pos', pos)):
        if t is not None and t.device != cache.device:
            raise ValueError('attn_decode: %s is on %s, the cache on %s' % (name, t.device, cache.device))
    qc = q.contiguous()
    kvc = kv_new.contiguous()
    o = torch.empty_like(qc)
    p = float(p)
    seed, off, dev = RngState.draw(p, B * nh * Lmax)
    launch('goat_attn_decode_fwd', _dt(qc), qc, kvc, cache, cache.stride(1), cache.stride(0), o, kmask, pos, B, int(nh), Lmax, 1.0 / math.sqrt(64.0),
           p, seed, off, dev, what='goat_attn_decode_fwd(B=%d,nh=%d,Lmax=%d)' % (B, nh, Lmax))
    return o


def decode_select(logits, state, unk, eos, pad, sampling=False, n_valid=None):
    """The next word of every row and the loop state in one launch (goat_decode_select): with t = state.pos[0] on the device, row b's
    word — arg-max of logits[b, :n_valid] without the column `unk` (ties: lowest index), or a categorical draw when `sampling`, or `pad`
    if the row has ended — goes to state.words[b, t + 1]; kmask, ended, end_step, n_live follow and pos advances by one.
    logits: float32 [B, ld] with n_valid <= ld valid columns (default: all).  Inference only."""
    _inference_only('decode_select', logits, state.words)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError('decode_select: logits are float32 [B, ld] with dense rows')
    B, ld = logits.shape
    V = ld if n_valid is None else int(n_valid)
    if B != state.B:
        raise ValueError('decode_select: %d rows of logits for a state of %d' % (B, state.B))
    if not 2 <= V <= ld:
        raise ValueError('decode_select: %d valid columns of %d (at least 2, at most the row length)' % (V, ld))
    want = (('words', torch.int64, (B, state.Lmax)), ('kmask', torch.float32, (B, state.Lmax)), ('ended', torch.uint8, (B,)),
            ('end_step', torch.int32, (B,)), ('pos', torch.int32, (1,)), ('n_live', torch.int32, (1,)))
    for name, dtype, shape in want:
        t = getattr(state, name)
        if t.device != logits.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError('decode_select: state.%s must be a contiguous %s %s on %s' % (name, dtype, list(shape), logits.device))
    seed, off, dev = RngState.draw(1.0 if sampling else 0.0, B * V)
    launch('goat_decode_select', logits, logits.stride(0), B, V, state.Lmax, int(unk), int(eos), int(pad), 1 if sampling else 0, seed, off, dev,
           state.pos, state.words, state.kmask, state.ended, state.end_step, state.n_live, what='goat_decode_select(B=%d,V=%d)' % (B, V))
