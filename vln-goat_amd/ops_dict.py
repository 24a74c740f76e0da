"""Inference-only device pipelines of the causal dictionaries: k-means (front door; csrc/kmeans.hip) and the running per-slot means
(back door; csrc/zdict.hip).  No backward pass: tensors that require grad are refused."""
import torch

from ._lib import GOAT_BF16, GOAT_F32
from ._plumbing import _dt, _epc, _inference_only, launch


# ----------------------------------------------------------------------------- k-means / dictionary pick (inference only; csrc/kmeans.hip)
KMEANS_MAXK = 256           # goat_kmeans_*: clusters


def _kmeans_x(what, x, K):
    """-> (N, D) of a feature table the goat_kmeans_* entry points take: float32 / bfloat16 [N, D] with dense 16-byte aligned rows."""
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[0] < 1:
        raise ValueError('%s: x is [N, D] with dense rows and N >= 1, got %s' % (what, tuple(x.shape)))
    N, D = x.shape
    if D < 8 or D % 8 or not 1 <= int(K) <= KMEANS_MAXK:
        raise ValueError('%s: D = %d must be a multiple of 8 and K = %d within 1..%d' % (what, D, K, KMEANS_MAXK))
    if x.stride(0) < D or x.stride(0) % _epc(x) or x.data_ptr() & 15:
        raise ValueError('%s: the rows of x must be 16-byte aligned (row stride %d)' % (what, x.stride(0)))
    return N, D


def _kmeans_i32(what, name, t, n, ref):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous() or t.device != ref.device:
        raise ValueError('%s: %s is a contiguous int32 [%d] on %s' % (what, name, n, ref.device))


def kmeans_assign(x, centres, labels=None, mind2=None, changed=None):
    """Nearest centre of every row (goat_kmeans_assign), exact float32: labels[i] = argmin_k ||x_i - c_k||² (ties: lowest k).
    x [N, D] float32 / bfloat16; centres float32 [K, D] contiguous.  `labels` int32 [N] is rewritten in place when given (and *changed,
    int32 [1], grows by the number of rows whose label moved); mind2 float32 [N] receives the squared distances.  -> (labels, mind2)."""
    _inference_only('kmeans_assign', x, centres, labels, mind2, changed)
    K = centres.shape[0]
    N, D = _kmeans_x('kmeans_assign', x, K)
    if centres.dtype != torch.float32 or tuple(centres.shape) != (K, D) or not centres.is_contiguous() or centres.device != x.device:
        raise ValueError('kmeans_assign: centres are a contiguous float32 [K, %d] on %s' % (D, x.device))
    if labels is None:
        labels = torch.full((N,), -1, dtype=torch.int32, device=x.device)
    if mind2 is None:
        mind2 = torch.empty(N, dtype=torch.float32, device=x.device)
    _kmeans_i32('kmeans_assign', 'labels', labels, N, x)
    if mind2.dtype != torch.float32 or mind2.numel() != N or not mind2.is_contiguous() or mind2.device != x.device:
        raise ValueError('kmeans_assign: mind2 is a contiguous float32 [%d] on %s' % (N, x.device))
    if changed is not None:
        _kmeans_i32('kmeans_assign', 'changed', changed, 1, x)
    launch('goat_kmeans_assign', _dt(x), x, x.stride(0), centres, labels, mind2, changed, N, D, K,
           what='goat_kmeans_assign(N=%d,D=%d,K=%d)' % (N, D, K))
    return labels, mind2


def kmeans_csr(labels, K):
    """labels int32 [N] -> (start int32 [K+1], order int32 [N]): the members of cluster k are order[start[k]:start[k+1]], ascending
    (goat_kmeans_csr, a stable counting sort on the device).  Labels outside [0, K) are skipped; the tail of `order` is -1 then."""
    _inference_only('kmeans_csr', labels)
    N = labels.numel()
    if N < 1 or not 1 <= int(K) <= KMEANS_MAXK:
        raise ValueError('kmeans_csr: N = %d >= 1 and K = %d within 1..%d' % (N, K, KMEANS_MAXK))
    _kmeans_i32('kmeans_csr', 'labels', labels, N, labels)
    start = torch.empty(int(K) + 1, dtype=torch.int32, device=labels.device)
    order = torch.full((N,), -1, dtype=torch.int32, device=labels.device)
    launch('goat_kmeans_csr', labels, start, order, N, int(K), what='goat_kmeans_csr(N=%d,K=%d)' % (N, K))
    return start, order


def kmeans_centres(x, order, start, centres):
    """centres[k] = mean of the rows of cluster k (goat_kmeans_centres; float32, bitwise reproducible), in place; the row of an empty
    cluster keeps its value.  -> centres."""
    _inference_only('kmeans_centres', x, order, start, centres)
    K = centres.shape[0]
    N, D = _kmeans_x('kmeans_centres', x, K)
    if centres.dtype != torch.float32 or tuple(centres.shape) != (K, D) or not centres.is_contiguous() or centres.device != x.device:
        raise ValueError('kmeans_centres: centres are a contiguous float32 [K, %d] on %s' % (D, x.device))
    _kmeans_i32('kmeans_centres', 'order', order, N, x)
    _kmeans_i32('kmeans_centres', 'start', start, K + 1, x)
    launch('goat_kmeans_centres', _dt(x), x, x.stride(0), order, start, centres, N, D, K,
           what='goat_kmeans_centres(N=%d,D=%d,K=%d)' % (N, D, K))
    return centres


def kmeans_pick(x, order, start, out, picked=None, seed=0, offset=0, rng_dev=None):
    """One uniformly drawn member per cluster, copied for every sample (goat_kmeans_pick): out [B, K, D] (the dtype of x, contiguous,
    rewritten in place) gets out[b, k] = x[picked[k]]; an empty cluster gives picked[k] = -1 and zeros.  The draw is a function of
    (seed + rng_dev[0], offset + k); rng_dev is a uint64-sized device counter (int64 [1]) or None.  -> picked int32 [K]."""
    _inference_only('kmeans_pick', x, order, start, out, picked, rng_dev)
    if out.dim() != 3:
        raise ValueError('kmeans_pick: out is [B, K, D], got %s' % (tuple(out.shape),))
    B, K, D = out.shape
    N, Dx = _kmeans_x('kmeans_pick', x, K)
    if Dx != D or B < 1 or out.dtype != x.dtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError('kmeans_pick: out is a contiguous %s [B >= 1, K, %d] on %s' % (x.dtype, Dx, x.device))
    _kmeans_i32('kmeans_pick', 'order', order, N, x)
    _kmeans_i32('kmeans_pick', 'start', start, K + 1, x)
    if picked is None:
        picked = torch.empty(K, dtype=torch.int32, device=x.device)
    _kmeans_i32('kmeans_pick', 'picked', picked, K, x)
    if rng_dev is not None and (rng_dev.dtype != torch.int64 or rng_dev.numel() != 1 or rng_dev.device != x.device):
        raise ValueError('kmeans_pick: rng_dev is one int64 on %s' % (x.device,))
    launch('goat_kmeans_pick', _dt(x), x, x.stride(0), order, start, out, picked, N, D, K, B, int(seed) & 0xFFFFFFFFFFFFFFFF,
           int(offset) & 0xFFFFFFFFFFFFFFFF, rng_dev, what='goat_kmeans_pick(N=%d,D=%d,K=%d,B=%d)' % (N, D, K, B))
    return picked


# ----------------------------------------------------------------------------- running per-slot means (inference only; csrc/zdict.hip)
DICT_PIECE = 64             # goat_dict_accumulate: rows of a slot summed in plain float32 before a compensated fold
DICT_MAXK = 65535           # goat_dict_*: slots


class DictState:
    """The running state of goat_dict_accumulate: sum and comp float32 [K, D] (sum + comp is the compensated total of every row a slot
    was given), count int32 [K]."""

    def __init__(self, K, D, device):
        if not 1 <= int(K) <= DICT_MAXK or int(D) < 8 or int(D) % 8:
            raise ValueError('DictState: K = %d within 1..%d and D = %d a multiple of 8' % (K, DICT_MAXK, D))
        self.K, self.D = int(K), int(D)
        self.sum = torch.zeros(self.K, self.D, dtype=torch.float32, device=device)
        self.comp = torch.zeros(self.K, self.D, dtype=torch.float32, device=device)
        self.count = torch.zeros(self.K, dtype=torch.int32, device=device)

    def zero(self):
        self.sum.zero_()
        self.comp.zero_()
        self.count.zero_()
        return self


def _dict_state(what, state, ref=None):
    K, D = state.K, state.D
    for name, t, dtype, shape in (('sum', state.sum, torch.float32, (K, D)), ('comp', state.comp, torch.float32, (K, D)),
                                  ('count', state.count, torch.int32, (K,))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != state.sum.device:
            raise ValueError('%s: state.%s must be a contiguous %s %s on %s' % (what, name, dtype, list(shape), state.sum.device))
    if ref is not None and ref.device != state.sum.device:
        raise ValueError('%s: the state is on %s, the tensors on %s' % (what, state.sum.device, ref.device))
    return K, D


def dict_accumulate(x, rows, start, state):
    """Add picked rows of x to the running per-slot sums (goat_dict_accumulate).  x: float32 / bfloat16 [R, D], possibly a strided 2-D
    view (dense 16-byte aligned rows); rows int32 [P]: row indices into x grouped by slot; start int32 [K+1]: slot k owns
    rows[start[k]:start[k+1]].  state (DictState) is updated in place: per launch a slot's rows are summed in float32 in pieces of
    DICT_PIECE and folded into (sum, comp) with a compensated step; count grows by the rows used.  Indices outside [0, R) are skipped
    and not counted.  Bitwise reproducible.  -> state."""
    _inference_only('dict_accumulate', x, rows, start, state.sum, state.comp, state.count)
    K, D = _dict_state('dict_accumulate', state, x)
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[0] < 1 or x.shape[1] != D:
        raise ValueError('dict_accumulate: x is [R >= 1, %d] with dense rows, got %s' % (D, tuple(x.shape)))
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('dict_accumulate: x is float32 or bfloat16, got %s' % x.dtype)
    R = x.shape[0]
    if x.stride(0) < D or x.stride(0) % _epc(x) or x.data_ptr() & 15:
        raise ValueError('dict_accumulate: the rows of x must be 16-byte aligned (row stride %d)' % x.stride(0))
    P = rows.numel()
    if P < 1:
        raise ValueError('dict_accumulate: rows is empty')
    _kmeans_i32('dict_accumulate', 'rows', rows, P, x)
    _kmeans_i32('dict_accumulate', 'start', start, K + 1, x)
    launch('goat_dict_accumulate', _dt(x), x, x.stride(0), R, rows, start, state.sum, state.comp, state.count, P, D, K,
           what='goat_dict_accumulate(R=%d,D=%d,K=%d,P=%d)' % (R, D, K, P))
    return state


def dict_finish(state, feats=None, out=None, out_pz=None):
    """The means and the slot probabilities of a DictState (goat_dict_finish): feats float32 [K, D] = (sum + comp) / count; the same
    values in the dtype of `out` in every out[b] of out [B, K, D]; out_pz [B, K] (or [B, K, 1]) = count / total count, the total formed
    on the device.  Any of the three may be None; out and out_pz share one dtype (float32 / bfloat16) and one B.  A slot that was given
    no rows comes out as zeros."""
    _inference_only('dict_finish', state.sum, state.comp, state.count, feats, out, out_pz)
    K, D = _dict_state('dict_finish', state, next((t for t in (feats, out, out_pz) if t is not None), None))
    dev = state.sum.device
    if feats is not None and (feats.dtype != torch.float32 or tuple(feats.shape) != (K, D) or not feats.is_contiguous() or feats.device != dev):
        raise ValueError('dict_finish: feats is a contiguous float32 [%d, %d] on %s' % (K, D, dev))
    B, dtype = None, None
    if out is not None:
        if out.dim() != 3 or tuple(out.shape[1:]) != (K, D) or out.shape[0] < 1 or not out.is_contiguous() or out.device != dev:
            raise ValueError('dict_finish: out is a contiguous [B >= 1, %d, %d] on %s, got %s' % (K, D, dev, tuple(out.shape)))
        B, dtype = out.shape[0], out.dtype
    if out_pz is not None:
        shape = tuple(out_pz.shape)
        if len(shape) not in (2, 3) or shape[0] < 1 or shape[1:] not in ((K,), (K, 1)) or not out_pz.is_contiguous() or out_pz.device != dev:
            raise ValueError('dict_finish: out_pz is a contiguous [B >= 1, %d] or [B, %d, 1] on %s, got %s' % (K, K, dev, shape))
        if B is not None and (shape[0] != B or out_pz.dtype != dtype):
            raise ValueError('dict_finish: out %s %s and out_pz %s %s must share B and the dtype' % (tuple(out.shape), dtype, shape, out_pz.dtype))
        B, dtype = shape[0], out_pz.dtype
    if dtype is not None and dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('dict_finish: out / out_pz are float32 or bfloat16, got %s' % dtype)
    launch('goat_dict_finish', GOAT_BF16 if dtype == torch.bfloat16 else GOAT_F32, state.sum, state.comp, state.count, feats, out, out_pz,
           B or 1, D, K, what='goat_dict_finish(B=%d,D=%d,K=%d)' % (B or 1, D, K))
