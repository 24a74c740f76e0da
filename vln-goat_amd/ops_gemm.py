"""The GEMM dispatcher: raw launches (goat_gemm_nt, goat_transpose, goat_colsum), gemm() with its autotuner / profile hooks and split-K
rules, and the weight-gradient GEMM through the gradient-sink protocol (wgrad, linear_wgrad).  Kernels: csrc/gemm*.hip."""
import os

import torch

from . import tuning
from ._lib import EPI_ACCUM, EPI_NONE
from ._plumbing import _dt, _epc, call, cargs, launch
from .gradsink import _first_touch, _prep_fallback, _sink, _sink_cat
from .tuning import _TUNED, _heuristic_cfg, _launch_gemm_bf16, _tune_gemm, load_tuned, stage_name, tile_name
from .wgrad_queue import WgradQueue


# ----------------------------------------------------------------------------- raw kernels
# (PROFILE — bench.py's per-launch HIP-event timing — lives in tuning.py beside the autotuner state; `hipops.PROFILE` is an alias)
def _profile_start():
    """(tuning.PROFILE is a list) -> (start, stop) timing events of one launch, `start` recorded: the head of its tuning.PROFILE entry
    (start, stop, flops, shape key, (C symbol, its arguments for a replay, the tensors they point into))."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0, e1


def gemm_nt(a, b, out, bias=None, epi=EPI_NONE, aux=None, split_k=1):
    """out[M,N] = epi(a[M,K] @ b[N,K]^T + bias)."""
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and out.shape[0] == M and out.shape[1] == N
    ev = _profile_start() if tuning.PROFILE is not None else None
    args = cargs(_dt(a), _dt(out), a, a.stride(0), b, b.stride(0), out, out.stride(0), M, N, K, bias, epi, aux,
                 aux.stride(0) if aux is not None else 0, split_k)
    call('goat_gemm_nt', args, what='goat_gemm_nt(M=%d,N=%d,K=%d)' % (M, N, K))
    if ev is not None:
        ev[1].record()
        tuning.PROFILE.append(ev + (2.0 * M * N * K, (M, N, K, epi, split_k, str(a.dtype)), ('goat_gemm_nt', args, (a, b, out, bias, aux))))
    return out


def transpose_pad(x, colsum=None):
    """x[R,C] -> out[C, ld] with ld = R rounded up to the 16-byte chunk, padding zero-filled."""
    R, C = x.shape
    e = _epc(x)
    ld = (R + e - 1) // e * e
    out = torch.empty((C, ld), dtype=x.dtype, device=x.device)
    launch('goat_transpose', _dt(x), x, x.stride(0), out, ld, R, C, colsum)
    return out


def _split_k(n_out_tiles, k_tiles, target=384):
    return max(1, min(k_tiles, int(round(float(target) / max(1, n_out_tiles)))))


def colsum(x, out=None):
    """float32 column sums of x[R,C] (bias gradient)."""
    R, C = x.shape
    if out is None:
        out = torch.zeros(C, dtype=torch.float32, device=x.device)
    launch('goat_colsum', _dt(x), x, x.stride(0), R, C, out)
    return out


# (Dropout inside the FFN GEMM epilogues — round 2's goat_gemm_bf16_dropout — measured 6.25 vs 6.22 ms per step: removed in round 3.)
def gemm(a, b, out, ta=False, tb=False, bias=None, epi=EPI_NONE, aux=None, split_k=1, colsum_out=None, split_opts=None,
         accumulate=False, zero_first=False):
    """out[M,N] = epi(op(a) @ op(b)^T + bias); ta: a is [Kc,M] (else [M,Kc]); tb: b is [Kc,N] (else [N,Kc]).
    bf16 -> pipelined LDS-DMA kernel (goat_gemm_bf16) whenever its layout rules hold; otherwise (f32 parity
    path, odd contraction lengths) explicit transposes + goat_gemm_nt.
    split_opts: candidate split-K factors the autotuner may choose from (the caller must have zero-filled
    `out` if any of them is > 1); returns `out`.
    accumulate: out (float32) += product — split-K launches add atomically anyway, unsplit ones use the
    read-modify-write epilogue GOAT_EPI_ACCUM (gradient-arena sinks).
    zero_first: `out` holds stale data: clear it here if (and only if) the launch ends up split (atomics)."""
    Kc = a.shape[0] if ta else a.shape[1]
    M = a.shape[1] if ta else a.shape[0]
    N = b.shape[1] if tb else b.shape[0]
    assert (b.shape[0] if tb else b.shape[1]) == Kc and out.shape[0] == M and out.shape[1] == N
    if M == 0 or N == 0:          # empty problem (e.g. an MRC batch without masked rows): the reference returns an empty tensor
        return out
    if Kc == 0:
        return out if accumulate else out.zero_()
    fast = (a.dtype == torch.bfloat16 and not (ta and not tb) and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0
            and ((ta and tb) or Kc % 64 == 0) and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            and a.stride(1) == 1 and b.stride(1) == 1)
    if not fast:
        if accumulate:       # f32 parity path / odd shapes: product into a temporary, then one add
            tmp = torch.zeros_like(out) if split_k > 1 else torch.empty_like(out)
            gemm(a, b, tmp, ta, tb, bias, epi, aux, split_k, colsum_out, None, False)
            return out.add_(tmp)
        if zero_first and split_k > 1:
            out.zero_()
        if colsum_out is not None:
            colsum(a, colsum_out)
        if ta:
            a = transpose_pad(a)
            if tb:
                b = transpose_pad(b)
            elif b.shape[1] != a.shape[1]:
                b = torch.nn.functional.pad(b, (0, a.shape[1] - b.shape[1]))
        elif tb:
            b = transpose_pad(b)
            if b.shape[1] != a.shape[1]:
                a = torch.nn.functional.pad(a, (0, b.shape[1] - a.shape[1]))
        if split_k > 1:
            bk = 64 if a.dtype == torch.bfloat16 else 32
            split_k = max(2, min(split_k, (a.shape[1] + bk - 1) // bk))
        return gemm_nt(a, b, out, bias, epi, aux, split_k)
    key = (ta, tb, M, N, Kc, epi, out.dtype == torch.float32, split_k, bias is not None)
    cfg = _TUNED.get(key)
    if cfg is None:
        if tuning.AUTOTUNE and not torch.cuda.is_current_stream_capturing() and tuning.PROFILE is None:
            cfg = _tune_gemm(key, a, b, out, ta, tb, M, N, Kc, bias, epi, aux, split_opts or (split_k,), colsum_out)
        else:
            cfg = _heuristic_cfg(ta, tb, M, N, Kc, split_k) + (split_k,)
            tuning.STATS['gemm_heuristic'] += 1          # a launch on a configuration nobody measured (tests assert a captured step has none)
            if len(tuning.STATS_LOG) < 256:
                tuning.STATS_LOG.append(('gemm', key, bool(torch.cuda.is_current_stream_capturing())))
            if os.environ.get('GOAT_GEMM_CFG_LOG'):      # (diagnostics: shapes that run on the heuristic, e.g. first seen inside a capture)
                import sys
                print('[gemm cfg] heuristic %s capturing=%s autotune=%s' % (key, torch.cuda.is_current_stream_capturing(), tuning.AUTOTUNE), file=sys.stderr)
    else:
        tuning.STATS['gemm_tuned'] += 1
    bm, nstage, split_cfg = cfg
    # a split launch accumulates with atomics: only allowed when the caller zero-filled `out` (split requested / split_opts
    # given), asked for the clear (zero_first) or accumulates anyway.  A tuned entry with split > 1 must never be applied to a
    # buffer the caller left uninitialised (found by the full-size gradient pins of round 2).
    may_split = split_k > 1 or split_opts is not None or zero_first or accumulate
    split_k = split_cfg if may_split else 1
    if zero_first and split_k > 1:
        out.zero_()
    if accumulate and split_k == 1:
        assert epi == EPI_NONE and out.dtype == torch.float32 and bias is None
        epi = EPI_ACCUM
    ev = _profile_start() if tuning.PROFILE is not None else None
    args = _launch_gemm_bf16(a, b, out, ta, tb, M, N, Kc, bias, epi, aux, split_k, bm, nstage, colsum_out)
    if ev is not None:
        ev[1].record()
        tuning.PROFILE.append(ev + (2.0 * M * N * Kc, (M, N, Kc, epi, split_k, 'v2 t%d%d %s %s' % (ta, tb, tile_name(bm), stage_name(nstage))),
                                    ('goat_gemm_bf16', args, (a, b, out, bias, aux, colsum_out))))
    return out


def wgrad(dy, x, want_bias, w_sink=None, b_sink=None, first=False, b_first=False, defer_ids=None):
    """dW[N,K] (f32) = dy[M,N]^T @ x[M,K] ; db[N] (f32) = colsum(dy), fused into the same kernel.
    One zero-fill covers both outputs (split-K partial tiles and the bias sums are accumulated atomically).
    With sinks (gradient-arena slices) the results are accumulated in place — deferred into a grouped launch when
    possible (WgradQueue) — and (None, None) is returned.  (Measured and dropped: running each weight-gradient GEMM on a
    second stream next to the dgrad chain was slower, 9.9 vs 9.3 ms per step.)"""
    M, N = dy.shape
    K = x.shape[1]
    # default (bm 64, split) from scripts/wgrad_sweep.py; the autotuner may pick another split (output is zero-filled)
    tiles = ((N + 63) // 64) * ((K + 127) // 128)
    kt = (M + 63) // 64
    if tiles < 128:
        split = max(1, min(int(round(250.0 / tiles)), kt // 8))
    else:
        split = max(1, min(int(round(500.0 / tiles)), kt // 24))
    nb = N if want_bias else 0
    tunable = tuning.AUTOTUNE and dy.dtype == torch.bfloat16
    if w_sink is not None:
        # gradient-arena slice.  First use in this step: clear it right here (the fill leaves the lines in the
        # Infinity Cache for the split-K atomics) or, unsplit, simply overwrite it; later uses accumulate.
        db = b_sink
        if want_bias and db is None:
            db = torch.zeros(N, dtype=torch.float32, device=dy.device)
        elif want_bias and b_first:
            db.zero_()
        if (defer_ids is not None and WgradQueue.enabled and dy.dtype == torch.bfloat16 and (b_sink is not None or not want_bias)
                and dy.stride(1) == 1 and x.stride(1) == 1 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0
                and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and w_sink.is_contiguous()
                and not torch.is_grad_enabled()):
            WgradQueue.push(dy, x, w_sink, db if want_bias else None, defer_ids, accumulate=not first)
            return None, None
        for i in (defer_ids or ()):
            WgradQueue.flush_param(i)           # (a write left queued for merging must land before this direct one)
        gemm(dy, x, w_sink, ta=True, tb=True, split_k=split, colsum_out=db if want_bias else None,
             split_opts=(1, 2, 3, 4, 6, 8) if tunable else None, accumulate=not first, zero_first=first)
        return None, (db if (want_bias and b_sink is None) else None)
    if split > 1 or tunable:
        buf = torch.zeros(N * K + nb, dtype=torch.float32, device=dy.device)
        dw = buf[:N * K].view(N, K)
        db = buf[N * K:] if want_bias else None
        split = max(split, 2) if not tunable else split
    else:
        dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
        db = torch.zeros(N, dtype=torch.float32, device=dy.device) if want_bias else None
    gemm(dy, x, dw, ta=True, tb=True, split_k=split, colsum_out=db,
         split_opts=(1, 2, 3, 4, 6, 8) if tunable else None)
    return dw, db


def linear_wgrad(dy, x, weights, biases, want_bias=True):
    """wgrad() of a Linear's weight — or of a run of weights whose outputs are concatenated in dy — through the gradient-sink protocol
    (gradsink.py), in its fixed order: look the sinks up (a queued write of a slice lands first unless the two problems may be merged),
    stamp first touches, clear the stale slices of whatever falls back to autograd, launch or queue.  A bias is only sunk when its
    weight is.  -> (dw, db) as wgrad returns them: None for what went into a sink.  biases: one per weight (None: no bias)."""
    keep = WgradQueue.mergeable(dy.shape[0], dy.shape[1], x.shape[1])      # small (BPTT-step) problems of one weight are merged into one
    if len(weights) == 1:
        w_sink = _sink(weights[0], keep)
        b_sink = _sink(biases[0], keep) if w_sink is not None else None
    else:
        w_sink = _sink_cat(weights, keep)
        b_sink = _sink_cat(biases, keep) if w_sink is not None else None
    if w_sink is None:
        _prep_fallback(*weights, *biases)
        return wgrad(dy, x, want_bias)
    first = _first_touch(*weights)
    b_first = b_sink is not None and _first_touch(*biases)
    if b_sink is None:
        _prep_fallback(*biases)
    return wgrad(dy, x, want_bias, w_sink, b_sink, first, b_first, [id(t) for t in weights] + [id(t) for t in biases if t is not None])


if not os.environ.get('GOAT_RETUNE'):       # (GOAT_RETUNE=1: start from an empty table and time every shape again)
    load_tuned()
