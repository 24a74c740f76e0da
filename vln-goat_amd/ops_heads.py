"""Heads and losses behind the encoders: per-row cross-entropy, the causal-learning heads (attention pooling, door gate, dictionary
expectation), the SAP tail, the CFP contrastive tail (mix + InfoNCE), and the validation statistics of the pre-training tasks."""
import ctypes

import torch

from ._lib import GOAT_BF16, GOAT_F32
from ._plumbing import _dt, _inference_only, _need_gpu, _ptr, _rows, launch
from .gradsink import small_sinks
from .ops_linear import _ce_rows_bwd, _ce_rows_fwd


class _CeRowsFn(torch.autograd.Function):
    """loss[m] = logsumexp(logits[m, :]) - logits[m, target[m]] (float32; a negative target = ignored row, loss 0): F.cross_entropy(reduction=
    'none', ignore_index=-100) on the action logits of a navigation step (M/r2r/agent.py:614-616) as one launch per direction
    (goat_ce_fwd / _bwd) instead of log_softmax + nll_loss and their two backward kernels.  Masked actions carry -inf logits."""

    @staticmethod
    def forward(ctx, logits, targets):
        lg = logits.float().contiguous()
        N = lg.shape[1]
        tg = targets.to(torch.int64).contiguous()
        loss, lse = _ce_rows_fwd(lg, N, N, tg)
        ctx.save_for_backward(lg, tg, lse)
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lg, tg, lse = ctx.saved_tensors
        N = lg.shape[1]
        dl = _ce_rows_bwd(lg, N, N, tg, lse, dloss, torch.float32)
        return (dl if ctx.in_dtype == torch.float32 else dl.to(ctx.in_dtype)), None


def cross_entropy_rows(logits, targets, ignore_index=-100):
    """per-row cross-entropy; rows whose target is NEGATIVE are ignored by the kernel (loss 0, zero gradient): `ignore_index` must be
    negative, and is what the torch route below (row widths that are no multiple of 4: goat_ce_* reads 16-byte pieces) is told.
    A target >= the row width is a caller bug: torch raises, the kernel returns NaN for that row (it never reads out of bounds)."""
    if ignore_index >= 0:
        raise ValueError('cross_entropy_rows ignores negative targets only (ignore_index = %d)' % ignore_index)
    _need_gpu(logits)
    if logits.shape[1] % 4:
        return torch.nn.functional.cross_entropy(logits.float(), targets, reduction='none', ignore_index=ignore_index)
    return _CeRowsFn.apply(logits, targets)


# ----------------------------------------------------------------------------- causal-learning heads
class _AttnPoolFn(torch.autograd.Function):
    """out = tanh(sum_l softmax_l(tanh(x_l)·w) x_l), all slots, no padding mask (P/model/pretrain_goat.py:502-515)."""

    @staticmethod
    def forward(ctx, x, w, smask=None):
        _need_gpu(x)
        x = x.contiguous()
        B, L, H = x.shape
        wv = w.detach().reshape(-1).float().contiguous()
        out = torch.empty((B, H), dtype=torch.float32, device=x.device)
        attn = torch.empty((B, L), dtype=torch.float32, device=x.device)
        ws = torch.empty(B * L, dtype=torch.float32, device=x.device)
        if smask is not None:
            assert smask.shape == (B, L) and smask.dtype == torch.float32 and smask.is_contiguous()
        launch('goat_attn_pool_fwd', _dt(x), x, wv, out, attn, ws, B, L, H, smask)
        ctx.save_for_backward(x, wv, attn, out)
        ctx.wshape = w.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wv, attn, out = ctx.saved_tensors
        B, L, H = x.shape
        dout = dout.float().contiguous()
        dx = torch.empty_like(x)
        dw = torch.zeros(H, dtype=torch.float32, device=x.device)
        ws = torch.empty(B * L, dtype=torch.float32, device=x.device)
        launch('goat_attn_pool_bwd', _dt(x), x, wv, attn, out, dout, dx, dw, ws, B, L, H)
        return dx, dw.view(ctx.wshape), None


def attn_pool(x, w, smask=None):
    """smask: optional float32 [B, L] of 0 / -inf added to the scores (slots beyond the batch's own padded width in a
    shape-bucketed static batch); masked slots get weight 0 and a zero gradient."""
    return _AttnPoolFn.apply(x, w, smask)


class _DoorGateFn(torch.autograd.Function):
    """s = sigmoid(Linear_a(aug) + Linear_o(ori)) per token; out = s*aug + (1-s)*ori (P/model/vilmodel_goat.py:137-143)."""

    @staticmethod
    def forward(ctx, aug, ori, wa, ba, wo, bo):
        _need_gpu(aug)
        H = aug.shape[-1]
        a2 = _rows(aug)
        o2 = _rows(ori, a2.dtype)
        wav, wov = wa.detach().reshape(-1).contiguous(), wo.detach().reshape(-1).contiguous()
        rows = a2.shape[0]
        out = torch.empty_like(a2)
        gate = torch.empty(rows, dtype=torch.float32, device=a2.device)
        launch('goat_door_gate_fwd', _dt(a2), a2, o2, wav, wov, ba.detach(), bo.detach(), out, gate, rows, H)
        ctx.save_for_backward(a2, o2, wav, wov, gate)
        ctx.shapes = (aug.shape, ori.shape, ori.dtype, wa.shape, wo.shape)
        ctx.params = (wa, ba, wo, bo)
        return out.view(aug.shape)

    @staticmethod
    def backward(ctx, dout):
        a2, o2, wav, wov, gate = ctx.saved_tensors
        ashape, oshape, odtype, washape, woshape = ctx.shapes
        rows, H = a2.shape
        d2 = _rows(dout, a2.dtype)
        daug, dori = torch.empty_like(a2), torch.empty_like(a2)
        sinks = small_sinks(ctx.params)
        if sinks is not None:
            # gradient arena: the four gate parameters are small (cleared by GradArena.zero at the start of the step, never a first touch) —
            # the kernel's atomics add straight into their slices; a gate used in every step of an episode would otherwise cost a zero fill,
            # a clone and four AccumulateGrad adds per use
            launch('goat_door_gate_bwd', _dt(a2), a2, o2, wav, wov, gate, d2, daug, dori, sinks[0], sinks[2], sinks[1], rows, H, sinks[3])
            return daug.view(ashape), dori.view(oshape).to(odtype), None, None, None, None
        buf = torch.zeros(2 * H + 1, dtype=torch.float32, device=a2.device)
        launch('goat_door_gate_bwd', _dt(a2), a2, o2, wav, wov, gate, d2, daug, dori, buf, _ptr(buf, H), _ptr(buf, 2 * H), rows, H, None)
        db = buf[2 * H:]          # both biases receive the same gradient (distinct tensors: autograd may keep them as .grad)
        return daug.view(ashape), dori.view(oshape).to(odtype), buf[:H].view(washape), db, buf[H:2 * H].view(woshape), db.clone()


def door_gate(aug_lin, ori_lin, aug, ori):
    """aug_lin / ori_lin: the two Linear(H,1) modules of the gate (their weights [1,H] and biases [1])."""
    return _DoorGateFn.apply(aug, ori, aug_lin.weight, aug_lin.bias, ori_lin.weight, ori_lin.bias)


class _DictWsumFn(torch.autograd.Function):
    """out[b,1,:] = sum_k p[b,k] z[b,k,:] (BACL type_1 confounder expectation, P/model/vilmodel_goat.py:115-118)."""

    @staticmethod
    def forward(ctx, z, p, out_dtype):
        _need_gpu(z)
        zf = z.float().contiguous()
        pf = p.float().reshape(p.shape[0], p.shape[1]).contiguous()
        B, K, H = zf.shape
        out = torch.empty((B, 1, H), dtype=out_dtype, device=z.device)
        launch('goat_dict_wsum_fwd', _dt(out), zf, pf, out, B, K, H)
        ctx.save_for_backward(zf, pf)
        ctx.meta = (z.dtype, p.shape, p.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        zf, pf = ctx.saved_tensors
        zdtype, pshape, pdtype = ctx.meta
        B, K, H = zf.shape
        d2 = _rows(dout)
        dz = torch.empty_like(zf) if ctx.needs_input_grad[0] else None
        dp = torch.empty_like(pf) if ctx.needs_input_grad[1] else None
        launch('goat_dict_wsum_bwd', _dt(d2), d2, zf, pf, dz, dp, B, K, H)
        return (dz.to(zdtype) if dz is not None else None, dp.view(pshape).to(pdtype) if dp is not None else None, None)


def dict_weighted_sum(z, p, out_dtype):
    return _DictWsumFn.apply(z, p, out_dtype)


# ----------------------------------------------------------------------------- SAP logits / loss
def _u8(t):
    """bool / uint8 mask -> contiguous byte tensor (a view for bool: same storage)."""
    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


class _SapFuseFn(torch.autograd.Function):
    """Tail of the single-action-prediction head in one launch per direction (goat_sap_fuse_fwd / _bwd; formulas in include/goat_hip.h;
    P/model/pretrain_goat.py:375-413, M/models/vilmodel_GOAT.py:803-839).  -> (gl, ll, fused, loss); loss is None without labels."""

    @staticmethod
    def forward(ctx, gs, ls, fwl, fw_sigmoid, gvis, gvalid, glens, lmask, lmask_is_valid, M, add_stop, ga, la):
        _need_gpu(gs)
        ctx.set_materialize_grads(False)
        B, G = gs.shape
        W = ls.shape[1]
        dt = gs.dtype
        gs = gs.contiguous()
        ls = ls.to(dt).contiguous()
        ctx.fw_shape = None if fwl is None else fwl.shape
        fwl = None if fwl is None else fwl.reshape(B).to(dt).contiguous()
        gvis, gvalid, lmask = _u8(gvis), _u8(gvalid), _u8(lmask)
        glens = None if glens is None else glens.to(torch.int64).contiguous()
        M = None if M is None else M.float().contiguous()
        ga = None if ga is None else ga.to(torch.int64).contiguous()
        la = None if la is None else la.to(torch.int64).contiguous()
        dev = gs.device
        gl = torch.empty((B, G), dtype=torch.float32, device=dev)
        ll = torch.empty((B, W), dtype=torch.float32, device=dev)
        fused = torch.empty((B, G), dtype=torch.float32, device=dev)
        labels = ga is not None
        loss = torch.empty(B, dtype=torch.float32, device=dev) if labels else None
        lse = torch.empty((B, 3), dtype=torch.float32, device=dev) if labels else None
        ctx.cfg = (_dt(gs), int(bool(fw_sigmoid)), int(bool(lmask_is_valid)), int(bool(add_stop)), B, G, W)
        launch('goat_sap_fuse_fwd', ctx.cfg[0], gs, ls, fwl, ctx.cfg[1], gvis, gvalid, glens, lmask, ctx.cfg[2], M, ctx.cfg[3], ga, la, gl, ll, fused,
               loss, lse, B, G, W)
        ctx.opt = (fwl, gvis, gvalid, glens, lmask, M, ga, la, lse)
        ctx.save_for_backward(gs, ls, gl, ll, fused)
        return gl, ll, fused, loss

    @staticmethod
    def backward(ctx, dgl, dll, dfused, dloss):
        gs, ls, gl, ll, fused = ctx.saved_tensors
        fwl, gvis, gvalid, glens, lmask, M, ga, la, lse = ctx.opt
        dtc, fw_sig, lvalid, add_stop, B, G, W = ctx.cfg
        f = lambda t: None if t is None else t.float().contiguous()
        dgl, dll, dfused, dloss = f(dgl), f(dll), f(dfused), f(dloss)
        dgs, dls = torch.empty_like(gs), torch.empty_like(ls)
        dfw = torch.empty_like(fwl) if fwl is not None else None
        launch('goat_sap_fuse_bwd', dtc, gs, ls, fwl, fw_sig, gvis, gvalid, glens, lmask, lvalid, M, add_stop, ga, la, gl, ll, fused, lse, dloss, dgl,
               dll, dfused, dgs, dls, dfw, B, G, W)
        return dgs, dls, (None if dfw is None else dfw.view(ctx.fw_shape)), None, None, None, None, None, None, None, None, None, None


def sap_fuse(gs, ls, fwl=None, fw_sigmoid=True, gvis=None, gvalid=None, glens=None, lmask=None, lmask_is_valid=False, M=None,
             add_stop=False, labels=None):
    """gs [B,G] / ls [B,W] head scores, fwl [B] or [B,1] fusion logit (None: weight 0.5) -> (global logits, local logits, fused logits,
    loss [B] or None), all float32.  labels = (global_act_labels, local_act_labels) adds the three cross-entropies."""
    ga, la = labels if labels is not None else (None, None)
    return _SapFuseFn.apply(gs, ls, fwl, fw_sigmoid, gvis, gvalid, glens, lmask, lmask_is_valid, M, add_stop, ga, la)


# ----------------------------------------------------------------------------- CFP contrastive losses
class _InfoNceFn(torch.autograd.Function):
    """loss[i] = sum_{x in gmap, vp, fused} 1/2 [CE(x_loc[i]·txt_all^T/tau, t0+i) + CE(txt_loc[i]·x_all^T/tau, t0+i)]
    (P/model/pretrain_goat.py:519-534) in one forward and one backward launch (goat_infonce_fwd / _bwd).  `*_all` are the
    candidates of every data-parallel rank (the same tensors as `*_loc` on one rank)."""

    @staticmethod
    def forward(ctx, g_loc, v_loc, f_loc, t_loc, g_all, v_all, f_all, t_all, target0, temperature):
        for t in (g_loc, v_loc, f_loc, t_loc, g_all, v_all, f_all, t_all):
            _need_gpu(t)
        ins = [t.float().contiguous() for t in (g_loc, v_loc, f_loc, t_loc, g_all, v_all, f_all, t_all)]
        Bl, H = ins[0].shape
        Ba = ins[4].shape[0]
        loss = torch.zeros(Bl, dtype=torch.float32, device=ins[0].device)
        prob = torch.empty((6, Bl, Ba), dtype=torch.float32, device=ins[0].device)
        xl = (ctypes.c_void_p * 3)(*[_ptr(t) for t in ins[0:3]])
        xa = (ctypes.c_void_p * 3)(*[_ptr(t) for t in ins[4:7]])
        launch('goat_infonce_fwd', xl, xa, ins[3], ins[7], loss, prob, Bl, Ba, H, int(target0), float(temperature))
        ctx.save_for_backward(prob, *ins)
        ctx.same = tuple(a is b for a, b in zip((g_loc, v_loc, f_loc, t_loc), (g_all, v_all, f_all, t_all)))
        ctx.cfg = (Bl, Ba, H, int(target0), float(temperature))
        return loss

    @staticmethod
    def backward(ctx, dloss):
        prob, *ins = ctx.saved_tensors
        Bl, Ba, H, target0, temperature = ctx.cfg
        dev = prob.device
        dloc = torch.zeros((4, Bl, H), dtype=torch.float32, device=dev)
        need_all = [not s for s in ctx.same]
        dall = torch.zeros((4, Ba, H), dtype=torch.float32, device=dev) if any(need_all) else None
        gl = [dloc[k] for k in range(4)]
        ga = [(dall[k] if need_all[k] else dloc[k]) for k in range(4)]      # same tensor passed as loc and all: one gradient buffer
        xl = (ctypes.c_void_p * 3)(*[_ptr(t) for t in ins[0:3]])
        xa = (ctypes.c_void_p * 3)(*[_ptr(t) for t in ins[4:7]])
        dxl = (ctypes.c_void_p * 3)(*[_ptr(t) for t in gl[0:3]])
        dxa = (ctypes.c_void_p * 3)(*[_ptr(t) for t in ga[0:3]])
        launch('goat_infonce_bwd', xl, xa, ins[3], ins[7], dloss.float().contiguous(), prob, dxl, dxa, gl[3], ga[3], Bl, Ba, H, target0, temperature)
        return tuple(gl) + tuple((ga[k] if need_all[k] else None) for k in range(4)) + (None, None)


def _cfp_mix_fwd(go, vo, fwl):
    B, H = go.shape
    fo = torch.empty_like(go)
    fw = torch.empty(B, dtype=torch.float32, device=go.device)
    launch('goat_cfp_mix_fwd', _dt(fwl), go, vo, fwl, fo, fw, B, H)
    return fo, fw


def _cfp_mix_bwd(go, vo, fw, dfo, dgo, dvo, fwl_dtype, accumulate):
    B, H = go.shape
    dfwl = torch.empty(B, dtype=fwl_dtype, device=go.device)
    launch('goat_cfp_mix_bwd', GOAT_BF16 if fwl_dtype == torch.bfloat16 else GOAT_F32, go, vo, fw, dfo, dgo, dvo, dfwl, B, H, int(accumulate))
    return dfwl


class _CfpMixFn(torch.autograd.Function):
    """fo = go * sigmoid(fwl) + vo * (1 - sigmoid(fwl))  (float32 [B,H] pooled vectors, fusion logit [B] / [B,1] in the compute dtype):
    the fused CFP vector of P/model/pretrain_goat.py:486-499 in one launch per direction."""

    @staticmethod
    def forward(ctx, go, vo, fwl):
        go, vo = go.float().contiguous(), vo.float().contiguous()
        f1 = fwl.reshape(-1).contiguous()
        fo, fw = _cfp_mix_fwd(go, vo, f1)
        ctx.save_for_backward(go, vo, fw)
        ctx.fshape, ctx.fdtype = fwl.shape, f1.dtype
        return fo

    @staticmethod
    def backward(ctx, dfo):
        go, vo, fw = ctx.saved_tensors
        dgo, dvo = torch.empty_like(go), torch.empty_like(vo)
        dfwl = _cfp_mix_bwd(go, vo, fw, dfo.float().contiguous(), dgo, dvo, ctx.fdtype, False)
        return dgo, dvo, dfwl.view(ctx.fshape)


_MEAN_SEED = {}


def backward_mean(loss_vec, scale=1.0):
    """`(loss_vec.mean() * scale).backward()` as the trainer spells it (P/train_r2r_goat.py:333-338), minus the autograd engine's seed
    launches: the mean is still computed (one launch: trainers log it; returned detached), the backward pass starts from a cached
    constant vector scale / n instead of ones_like + div (+ mul) kernels."""
    n = loss_vec.numel()
    key = (n, float(scale), loss_vec.device, loss_vec.dtype)
    g = _MEAN_SEED.get(key)
    if g is None:
        g = _MEAN_SEED[key] = torch.full((n,), float(scale) / n, dtype=loss_vec.dtype, device=loss_vec.device)
    m = loss_vec.detach().mean()
    torch.autograd.backward(loss_vec, grad_tensors=g.view_as(loss_vec))
    return m


def cfp_mix(go, vo, fwl):
    return _CfpMixFn.apply(go, vo, fwl)


class _CfpTailFn(torch.autograd.Function):
    """loss = InfoNCE(go, vo, fo, to) with fo = mix(go, vo, fwl) — the whole CFP tail behind the three pooled vectors as ONE autograd node
    (single rank: candidates = the batch's own vectors): two launches per direction, and the gradients of go / vo from the loss and from
    the fused vector meet inside the backward kernels instead of in autograd-engine adds."""

    @staticmethod
    def forward(ctx, go, vo, fwl, to, temperature):
        go, vo, to = go.float().contiguous(), vo.float().contiguous(), to.float().contiguous()
        f1 = fwl.reshape(-1).contiguous()
        fo, fw = _cfp_mix_fwd(go, vo, f1)
        Bl, H = go.shape
        loss = torch.zeros(Bl, dtype=torch.float32, device=go.device)
        prob = torch.empty((6, Bl, Bl), dtype=torch.float32, device=go.device)
        xs = (ctypes.c_void_p * 3)(_ptr(go), _ptr(vo), _ptr(fo))
        launch('goat_infonce_fwd', xs, xs, to, to, loss, prob, Bl, Bl, H, 0, float(temperature))
        ctx.save_for_backward(go, vo, fo, to, fw, prob)
        ctx.fshape, ctx.fdtype, ctx.temperature = fwl.shape, f1.dtype, float(temperature)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        go, vo, fo, to, fw, prob = ctx.saved_tensors
        Bl, H = go.shape
        d = torch.zeros((4, Bl, H), dtype=torch.float32, device=go.device)          # dgo | dvo | dfo | dto, accumulated by the kernels
        xs = (ctypes.c_void_p * 3)(_ptr(go), _ptr(vo), _ptr(fo))
        dx = (ctypes.c_void_p * 3)(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]))
        launch('goat_infonce_bwd', xs, xs, to, to, dloss.float().contiguous(), prob, dx, dx, d[3], d[3], Bl, Bl, H, 0, ctx.temperature)
        dfwl = _cfp_mix_bwd(go, vo, fw, d[2], d[0], d[1], ctx.fdtype, True)
        return d[0], d[1], dfwl.view(ctx.fshape), d[3], None


def cfp_tail(go, vo, fwl, to, temperature):
    return _CfpTailFn.apply(go, vo, fwl, to, temperature)


def infonce(g_loc, v_loc, f_loc, t_loc, g_all, v_all, f_all, t_all, target0, temperature):
    return _InfoNceFn.apply(g_loc, v_loc, f_loc, t_loc, g_all, v_all, f_all, t_all, target0, temperature)


# ----------------------------------------------------------------------------- validation statistics (csrc/valstats.hip)
def val_rows(logits, row_loss, row_hit, labels=None, soft=None):
    """goat_val_rows: per-row loss and hit of logits [M, N] against hard labels (int64 [M]; negative = ignored row) or soft targets
    (float32 [M, N]) into row_loss float32 [M] / row_hit int32 [M].  Rows may be strided (a column slice of a wider matrix is read in
    place); anything else is made float32 and row-contiguous first.  -> the labels as the kernel read them (for val_reduce), or None."""
    if (labels is None) == (soft is None):
        raise ValueError('val_rows: exactly one of labels / soft')
    _inference_only('val_rows', logits, labels, soft, row_loss, row_hit)
    M, N = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1 or logits.stride(0) < N:
        logits = logits.float().contiguous()
    if labels is not None:
        labels = labels.to(torch.int64).contiguous()
        if labels.shape != (M,):
            raise ValueError('val_rows: %d labels for %d rows' % (labels.numel(), M))
    else:
        if soft.shape != (M, N):
            raise ValueError('val_rows: soft targets %s for logits %s' % (tuple(soft.shape), (M, N)))
        if soft.dtype != torch.float32 or soft.stride(1) != 1 or soft.stride(0) < N:
            soft = soft.float().contiguous()
    if row_loss.dtype != torch.float32 or row_hit.dtype != torch.int32 or row_loss.numel() < M or row_hit.numel() < M \
            or not (row_loss.is_contiguous() and row_hit.is_contiguous()):
        raise ValueError('val_rows: row_loss float32 [>= M] and row_hit int32 [>= M], contiguous')
    launch('goat_val_rows', logits, logits.stride(0), M, N, labels, soft, 0 if soft is None else soft.stride(0), row_loss, row_hit,
           what='goat_val_rows(M=%d,N=%d)' % (M, N))
    return labels


def val_cfp(go, vo, fo, to, temperature, row_loss, row_hit):
    """goat_val_cfp: row_loss / row_hit [3 * B] (modality-major: gmap, vp, fused) of the three image/text problems of validate_cfp"""
    _inference_only('val_cfp', go, vo, fo, to, row_loss, row_hit)
    ins = [t.float().contiguous() for t in (go, vo, fo, to)]
    B, H = ins[0].shape
    if any(t.shape != (B, H) for t in ins):
        raise ValueError('val_cfp: four [B, H] operands, got %s' % [tuple(t.shape) for t in ins])
    if row_loss.dtype != torch.float32 or row_hit.dtype != torch.int32 or row_loss.numel() < 3 * B or row_hit.numel() < 3 * B \
            or not (row_loss.is_contiguous() and row_hit.is_contiguous()):
        raise ValueError('val_cfp: row_loss float32 [>= 3 B] and row_hit int32 [>= 3 B], contiguous')
    xs = (ctypes.c_void_p * 3)(*[_ptr(t) for t in ins[:3]])
    launch('goat_val_cfp', xs, ins[3], B, H, float(temperature), row_loss, row_hit, what='goat_val_cfp(B=%d,H=%d)' % (B, H))


def val_reduce(row_loss, row_hit, labels, acc):
    """goat_val_reduce: acc (float64 [3], a slot of a wider accumulator) += (sum of row_loss, sum of row_hit, rows with label >= 0)"""
    _inference_only('val_reduce', row_loss, row_hit, labels, acc)
    M = row_loss.numel()
    if acc.dtype != torch.float64 or acc.numel() != 3 or not acc.is_contiguous() or row_hit.numel() != M or (labels is not None and labels.numel() != M):
        raise ValueError('val_reduce: acc float64 [3]; row_loss, row_hit and labels of one length')
    launch('goat_val_reduce', row_loss, row_hit, labels, M, acc, what='goat_val_reduce(M=%d)' % M)
