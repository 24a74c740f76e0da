"""Inputs of the encoders: the embedding tables (with the data-parallel sparse-gradient hook), the panorama view fusion and the
segment-mean gather of the graph map."""
import os

import torch

from ._plumbing import _dt, _need_gpu, launch
from .gradsink import _first_touch, _sink, small_sinks
from .ops_gemm import colsum


PANO_SINK = os.environ.get('GOAT_NO_PANO_SINK', '0') != '1'


class _PanoFusionFn(torch.autograd.Function):
    """fused[n] = sum_v softmax_v(tanh(x[n,v]·a + a0)) x[n,v]  (P/model/vilmodel_goat.py:354-361)."""

    @staticmethod
    def forward(ctx, x, a_w, a_b):
        _need_gpu(x)
        x = x.contiguous()
        N, V, H = x.shape
        fused = torch.empty((N, H), dtype=x.dtype, device=x.device)
        wsave = torch.empty((N, V), dtype=torch.float32, device=x.device)
        av = a_w.detach().reshape(-1).contiguous()
        launch('goat_pano_fusion_fwd', _dt(x), x, av, a_b, fused, wsave, N, V, H)
        ctx.save_for_backward(x, av, a_b, wsave)
        ctx.wshape = a_w.shape
        ctx.params = (a_w, a_b)
        return fused

    @staticmethod
    def backward(ctx, df):
        x, av, a_b, wsave = ctx.saved_tensors
        N, V, H = x.shape
        df = df.contiguous()
        dx = torch.empty_like(x)
        sinks = small_sinks(ctx.params)      # (bound slices are cleared on first touch whether the kernel then adds into them or not)
        sunk = PANO_SINK and sinks is not None and sinks[0].is_contiguous()
        if sunk:                 # arena slices: the kernel's atomics add straight into them
            da, da0 = sinks[0].view(-1), sinks[1].view(-1)
        else:
            da = torch.zeros(H, dtype=torch.float32, device=x.device)
            da0 = torch.zeros(1, dtype=torch.float32, device=x.device)
        launch('goat_pano_fusion_bwd', _dt(x), x, av, a_b, wsave, df, dx, da, da0, N, V, H)
        if sunk:
            return dx, None, None
        return dx, da.view(ctx.wshape), da0


def pano_fusion(x, a_w, a_b):
    return _PanoFusionFn.apply(x, a_w, a_b)


class _GatherFn(torch.autograd.Function):
    """out[i] = scale[i] * sum_{j in seg i} src[idx[j]]  (index tensors built on the host per batch)."""

    @staticmethod
    def forward(ctx, src, idx, start, scale, n_out, inverse):
        _need_gpu(src)
        src = src.contiguous()
        H = src.shape[-1]
        s2 = src.reshape(-1, H)
        out = torch.empty((n_out, H), dtype=src.dtype, device=src.device)
        launch('goat_gather_segmean_fwd', _dt(s2), s2, s2.shape[0], idx, start, scale, out, n_out, H, None)
        ctx.save_for_backward(idx, start, scale)
        ctx.sshape, ctx.sdtype = src.shape, src.dtype
        ctx.inverse = inverse
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, start, scale = ctx.saved_tensors
        dout = dout.contiguous()
        n_out, H = dout.shape
        rows = 1
        for s in ctx.sshape[:-1]:
            rows *= s
        if ctx.inverse is not None:          # inverse index built on the host with the forward one: the backward pass is a gather too
            inv_idx, inv_start = ctx.inverse[0], ctx.inverse[1]
            inv_w = ctx.inverse[2] if len(ctx.inverse) > 2 else None
            if inv_start.numel() != rows + 1:
                raise ValueError('inverse gather index covers %d rows, the source has %d' % (inv_start.numel() - 1, rows))
            d2 = dout if dout.dtype == ctx.sdtype else dout.to(ctx.sdtype)
            dsrc = torch.empty((rows, H), dtype=ctx.sdtype, device=dout.device)
            launch('goat_gather_segmean_fwd', _dt(d2), d2, n_out, inv_idx, inv_start, None, dsrc, rows, H, inv_w,
                   what='goat_gather_segmean_fwd (inverse)')
            return dsrc.view(ctx.sshape), None, None, None, None, None
        d32 = torch.zeros((rows, H), dtype=torch.float32, device=dout.device)
        launch('goat_gather_segmean_bwd', _dt(dout), dout, idx, start, scale, d32, n_out, H)
        return d32.to(ctx.sdtype).view(ctx.sshape), None, None, None, None, None


def gather_segmean(src, idx, start, scale, n_out, inverse=None):
    """inverse: graphmap.inverse_index(idx, start, scale, n_src) on the device (optional) — the backward pass then gathers instead
    of scatter-adding with float atomics into a zero-filled float32 buffer."""
    return _GatherFn.apply(src, idx, start, scale, int(n_out), inverse)


# ----------------------------------------------------------------------------- embedding tables
_EMBED_ERR = {}


def _embed_err(dev):
    t = _EMBED_ERR.get(dev)
    if t is None:
        t = _EMBED_ERR[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def check_embed_errors():
    """Raises if any embedding lookup since the last call saw an id outside its table (synchronises)."""
    for dev, t in _EMBED_ERR.items():
        if int(t.item()):
            t.zero_()
            raise IndexError('embedding id out of range on %s' % (dev,))


class SparseEmbedGrad:
    """Data-parallel hook for the word-embedding table.  In a step whose only gradient of the table comes from the lookups
    (sap, cfp: at most B*L of its 50 265 rows are touched) all-reducing the dense 154 MB table gradient is waste: with
    `sink_list` set (dp.GoatDataParallel.begin_step), _EmbedFn.backward does not scatter into a table listed in `params`
    but hands (d_out rows, ids, table, padding index) over; dp all-gathers rows + ids (5.9 MB per rank) and scatter-adds
    every rank's rows locally (GoatDataParallel.reduce_gradients).  Inactive at world size 1 and in mlm steps (the tied
    decoder makes the table gradient dense)."""
    params = set()          # id(parameter) of the tables handled this way
    sink_list = None        # list to append to during this step's backward, or None


class _EmbedFn(torch.autograd.Function):
    """out = word[ids] (+ type[type_ids or 0]) (+ pos[arange(L)]) in one pass; backward scatters into f32 table
    gradients (P/model/Bert_backbone.py:98-113).  Replaces three F.embedding calls and torch's sort-based
    embedding backward."""

    @staticmethod
    def forward(ctx, ids, word, type_tab, type_ids, pos_tab, out_dtype, word_pad, pos_pad):
        _need_gpu(word)
        ids = ids.contiguous()
        if ids.dtype != torch.int64:
            ids = ids.long()
        if type_ids is not None:
            type_ids = type_ids.long().contiguous()
        V, H = word.shape
        rows = ids.numel()
        L = ids.shape[-1]
        if pos_tab is not None and L > pos_tab.shape[0]:
            raise IndexError('sequence length %d exceeds the position table (%d rows)' % (L, pos_tab.shape[0]))
        out = torch.empty(tuple(ids.shape) + (H,), dtype=out_dtype, device=word.device)
        launch('goat_embed_fwd', _dt(out), word, ids, type_tab, type_ids, pos_tab, L, out, rows, H, V, _embed_err(word.device))
        ctx.tabs = (word, type_tab, pos_tab)
        ctx.save_for_backward(ids, type_ids)
        ctx.meta = (V, H, L, None if type_tab is None else type_tab.shape[0], None if pos_tab is None else pos_tab.shape[0],
                    -1 if word_pad is None else int(word_pad), -1 if pos_pad is None else int(pos_pad))
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, type_ids = ctx.saved_tensors
        V, H, L, TV, P, word_pad, pos_pad = ctx.meta
        dout = dout.contiguous()
        d2 = dout.view(-1, H)
        rows = d2.shape[0]
        need_w, need_t, need_p = ctx.needs_input_grad[1], TV is not None and ctx.needs_input_grad[2], \
            P is not None and ctx.needs_input_grad[4]
        dev = dout.device
        sw, st_, sp = (_sink(t) for t in ctx.tabs)
        if need_w and sw is not None and SparseEmbedGrad.sink_list is not None and id(ctx.tabs[0]) in SparseEmbedGrad.params:
            SparseEmbedGrad.sink_list.append((d2, ids, ctx.tabs[0], word_pad))      # exchanged and scattered by dp after backward
            need_w = False
        for t, sk, need in zip(ctx.tabs, (sw, st_, sp), (need_w, need_t, need_p)):
            if sk is not None and need and _first_touch(t):
                sk.zero_()              # first writer of this slice in the step: clear it (scatter-adds follow)
        dword = (sw if sw is not None else torch.zeros((V, H), dtype=torch.float32, device=dev)) if need_w else None
        dtab = (st_ if st_ is not None else torch.zeros((TV, H), dtype=torch.float32, device=dev)) if need_t else None
        dpos = (sp if sp is not None else torch.zeros((P, H), dtype=torch.float32, device=dev)) if need_p else None
        if need_w or (need_t and type_ids is not None):
            launch('goat_embed_bwd', _dt(d2), d2, ids, type_ids, L, dword, dtab if type_ids is not None else None, None, rows, H, V, word_pad, pos_pad)
        if need_p:
            # position ids are arange(L) for every sample: d pos[:L] = column sums of dout viewed as [rows/L, L*H]
            # (the padding row, if any, is skipped: nn.Embedding(padding_idx) gives it no gradient)
            flat, of = d2.view(rows // L, L * H), dpos.view(-1)
            if 0 <= pos_pad < L:
                if pos_pad > 0:
                    colsum(flat[:, :pos_pad * H], out=of[:pos_pad * H])
                if pos_pad + 1 < L:
                    colsum(flat[:, (pos_pad + 1) * H:], out=of[(pos_pad + 1) * H:L * H])
            else:
                colsum(flat, out=of[:L * H])
        if need_t and type_ids is None:
            colsum(d2, out=dtab[0])            # every token has type 0: one column sum instead of `rows` atomics per column
        return (None, None if (dword is sw or dword is None) else dword, None if dtab is st_ else dtab, None,
                None if dpos is sp else dpos, None, None, None)


def embedding_scatter_add(dword, rows, ids, word_pad=-1):
    """dword[ids[r], :] += rows[r, :] (float32 table gradient, atomics) — goat_embed_bwd on the word table only."""
    rows = rows.contiguous()
    ids = ids.reshape(-1).contiguous()
    launch('goat_embed_bwd', _dt(rows), rows, ids, None, 1, dword, None, None, rows.shape[0], rows.shape[1], dword.shape[0],
           -1 if word_pad is None else int(word_pad), -1)


def embedding(ids, word, type_tab=None, type_ids=None, pos_tab=None, out_dtype=None, word_pad=None, pos_pad=None):
    return _EmbedFn.apply(ids, word, type_tab, type_ids, pos_tab, out_dtype or word.dtype, word_pad, pos_pad)
