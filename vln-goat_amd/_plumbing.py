"""Pointer / dtype / stream / row-matrix helpers and the one launch path into the C ABI, shared by the modules that call it (the op
families behind hipops, tuning, wgrad_queue, optim)."""
import torch

from . import _lib
from ._lib import GOAT_BF16, GOAT_F32


def _dt(t):
    if t.dtype == torch.float32:
        return GOAT_F32
    if t.dtype == torch.bfloat16:
        return GOAT_BF16
    raise RuntimeError('libgoat_hip supports float32 / bfloat16, got %s' % t.dtype)


def _epc(t):
    return 4 if t.dtype == torch.float32 else 8


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError('GOAT HIP ops need tensors on the GPU (no CPU fallback in the product path)')


def _inference_only(what, *tensors):
    for t in tensors:
        if t is not None and t.requires_grad:
            raise RuntimeError('%s is inference-only (no backward pass): got a tensor that requires grad — call it under '
                               'torch.no_grad() on detached tensors' % what)
    for t in tensors:
        if t is not None:
            _need_gpu(t)


def _ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def _rows(x, dtype=None):
    """x[..., H] as a contiguous [rows, H] matrix, cast to `dtype` (if given) before it is made contiguous."""
    x2 = x.reshape(-1, x.shape[-1])
    if dtype is not None and x2.dtype != dtype:
        x2 = x2.to(dtype)
    return x2.contiguous()


# The per-argument test of cargs / launch, cheapest case first: plain values by exact type, tensors by exact type, and only then
# isinstance() (a tensor subclass; ctypes arrays and structs fall through it).  isinstance() against torch.Tensor goes through the
# tensor metaclass and costs more than everything else in the loop, and the eager step makes several hundred launches.
_PLAIN = frozenset({int, float, type(None)})
_TENSOR = frozenset({torch.Tensor, torch.nn.Parameter})


def cargs(*args):
    """The arguments of a C-ABI call as ctypes takes them: a tensor becomes its data pointer; None (a null pointer), ints (a pointer with
    an element offset is the int `_ptr(t, off)`), floats, ctypes arrays and ctypes structs stay as they are."""
    return tuple([a if type(a) in _PLAIN else a.data_ptr() if (type(a) in _TENSOR or isinstance(a, torch.Tensor)) else a for a in args])


def call(symbol, ctuple, what=None):
    """launch() for arguments that are converted already (ctuple = cargs(...)): the GEMM wrappers launch from the very tuple they keep
    in the tuning.PROFILE record."""
    st = getattr(_lib.lib(), symbol)(_stream(), *ctuple)
    if st:
        _lib.check(st, what or symbol)


def launch(symbol, *args, what=None):
    """Run `symbol` of libgoat_hip.so on the current torch stream with cargs(*args); a non-zero status raises, naming `what` (a label
    with the shapes in it) or the symbol.  Every stream-taking entry point is called through here or through call(), except: the queries
    that return a value instead of a status (goat_version, goat_ln_bwd_nparts, goat_ln_bwd_ws_floats, goat_wgrad_balanced_ws_bytes), and
    WgradQueue._run, whose callers want the raw status (the tuner tries configurations the library may reject).
    (cargs' comprehension is written out here: a nested call per launch costs as much as converting five arguments.)"""
    st = getattr(_lib.lib(), symbol)(_stream(), *[a if type(a) in _PLAIN else a.data_ptr() if (type(a) in _TENSOR or isinstance(a, torch.Tensor)) else a
                                                  for a in args])
    if st:
        _lib.check(st, what or symbol)
