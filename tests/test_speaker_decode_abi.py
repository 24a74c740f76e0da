"""KV-cached decoding, the part that needs no GPU: goat_attn_decode_fwd / goat_decode_select are declared, exported and bound, reject
bad arguments before any launch (no kernel runs: every call below fails validation), and the hipops wrappers are inference-only."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE = -1, -2


def _lib():
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _aligned(nbytes=1024):
    buf = (ctypes.c_char * (nbytes + 16))()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_decode_entry_points_are_declared_exported_and_bound():
    lib = _lib()
    txt = open(os.path.join(ROOT, 'include', 'goat_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    h = lib.lib()
    for name in ('goat_attn_decode_fwd', 'goat_decode_select'):
        assert re.search(r'\bint\s+%s\s*\(' % name, txt), name
        assert hasattr(h, name) and name in lib.SIGNATURES
    assert h.goat_version() >= 103
    assert 'decode.hip' in lib.SOURCES


def _attn(h, p, dtype=1, Q=True, cache=True, pos=True, Lmax=16, c_rs=512, c_bs=512 * 16):
    return h.goat_attn_decode_fwd(None, dtype, p if Q else None, p, p if cache else None, c_rs, c_bs, p, None, p if pos else None,
                                  1, 4, Lmax, 0.125, 0.0, 0, 0, None)


def test_attn_decode_argument_validation_without_gpu():
    h = _lib().lib()
    keep, p = _aligned()
    assert _attn(h, p, Q=False) == E_ARG
    assert _attn(h, p, cache=False) == E_ARG
    assert _attn(h, p, pos=False) == E_ARG
    assert _attn(h, p, dtype=7) == E_ARG
    assert _attn(h, p, Lmax=0) == E_SHAPE
    assert _attn(h, p, Lmax=513) == E_SHAPE
    assert _attn(h, p, c_rs=516) == E_SHAPE            # bf16: 516 elements are not a multiple of the 8-element chunk
    assert _attn(h, p, c_bs=512 * 16 + 4) == E_SHAPE
    assert _attn(h, p + 8) == E_SHAPE                  # base not 16-byte aligned
    del keep


def _select(h, p, logits=True, words=True, V=8, ld=64):
    return h.goat_decode_select(None, p if logits else None, ld, 2, V, 8, 3, 2, 0, 0, 0, 0, None, p, p if words else None, p, p, p, p)


def test_decode_select_argument_validation_without_gpu():
    h = _lib().lib()
    keep, p = _aligned()
    assert _select(h, p, logits=False) == E_ARG
    assert _select(h, p, words=False) == E_ARG
    assert _select(h, p, V=1) == E_SHAPE
    assert _select(h, p, V=65, ld=64) == E_SHAPE
    del keep


def test_attn_decode_refuses_cpu_tensors_and_grad():
    from vln_goat_amd import hipops
    q, kv, cache = torch.zeros(2, 256), torch.zeros(2, 512), torch.zeros(2, 8, 512)
    pos = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.attn_decode(q, kv, cache, None, pos, 4, 0.0)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.attn_decode(q.clone().requires_grad_(), kv, cache, None, pos, 4, 0.0)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.attn_decode(q, kv.clone().requires_grad_(), cache, None, pos, 4, 0.0)
    state = hipops.DecodeState(2, 8, 'cpu')
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.decode_select(torch.zeros(2, 64), state, 3, 2, 0)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.decode_select(torch.zeros(2, 64, requires_grad=True), state, 3, 2, 0)
