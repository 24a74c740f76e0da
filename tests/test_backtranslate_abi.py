"""Back-translation on the device, the part that needs no GPU: goat_retok_rows / goat_scale_cols are declared, exported and bound,
reject bad arguments before any launch (no kernel runs: every call below fails validation), and the hipops wrappers are
inference-only and GPU-only."""
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


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib()
    txt = open(os.path.join(ROOT, 'include', 'goat_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    h = lib.lib()
    for name in ('goat_retok_rows', 'goat_scale_cols'):
        assert re.search(r'\bint\s+%s\s*\(' % name, txt), name
        assert hasattr(h, name) and name in lib.SIGNATURES
    assert h.goat_version() >= 106
    assert 'backtrans.hip' in lib.SOURCES
    from vln_goat_amd import hipops, ops_text
    assert hipops.retok_rows is ops_text.retok_rows and hipops.scale_cols is ops_text.scale_cols


def _retok(h, p, null=None, width=4, ldw=8, B=2, V=9, max_len=6, ldo=8):
    a = {k: p for k in ('words', 'ended', 'end_step', 'pos', 'n_live', 'first_start', 'first_ids', 'rest_start', 'rest_ids', 'out_ids', 'out_mask',
                        'lens', 'status')}
    if null:
        a[null] = None
    return h.goat_retok_rows(None, a['words'], ldw, a['ended'], a['end_step'], a['pos'], a['n_live'], width, B, V, 7, 2, 0, a['first_start'],
                             a['first_ids'], a['rest_start'], a['rest_ids'], 0, 2, 1, max_len, a['out_ids'], a['out_mask'], ldo, a['lens'], a['status'])


def test_retok_rows_argument_validation_without_gpu():
    h = _lib().lib()
    keep, p = _aligned()
    for name in ('words', 'first_start', 'first_ids', 'rest_start', 'rest_ids', 'out_ids', 'out_mask', 'lens', 'status'):
        assert _retok(h, p, null=name) == E_ARG, name
    for name in ('ended', 'end_step', 'pos', 'n_live'):          # the decode state is read only to derive the width
        assert _retok(h, p, null=name, width=0) == E_ARG, name
    assert _retok(h, p, ldw=513) == E_SHAPE
    assert _retok(h, p, ldw=0) == E_SHAPE
    assert _retok(h, p, width=513, ldw=512) == E_SHAPE
    assert _retok(h, p, width=-1) == E_SHAPE
    assert _retok(h, p, max_len=9, ldo=8) == E_SHAPE
    assert _retok(h, p, max_len=1) == E_SHAPE
    assert _retok(h, p, max_len=513, ldo=600) == E_SHAPE
    assert _retok(h, p, B=0) == E_SHAPE
    assert _retok(h, p, B=1025) == E_SHAPE
    assert _retok(h, p, V=0) == E_SHAPE
    del keep


def _scale(h, p, dtype=1, x=True, out=True, noise=True, rows=4, ld=16, D=8):
    return h.goat_scale_cols(None, dtype, p if x else None, p if out else None, p if noise else None, rows, ld, D)


def test_scale_cols_argument_validation_without_gpu():
    h = _lib().lib()
    keep, p = _aligned()
    assert _scale(h, p, x=False) == E_ARG
    assert _scale(h, p, out=False) == E_ARG
    assert _scale(h, p, noise=False) == E_ARG
    assert _scale(h, p, dtype=7) == E_ARG
    assert _scale(h, p, rows=0) == E_SHAPE
    assert _scale(h, p, D=0) == E_SHAPE
    assert _scale(h, p, ld=7, D=8) == E_SHAPE
    assert _scale(h, p + 1) == E_SHAPE                 # a bf16 base at an odd address
    assert _scale(h, p + 2, dtype=0) == E_SHAPE        # a float32 base that is not 4-byte aligned
    del keep


class _Table:
    V = 4
    first_start = rest_start = torch.zeros(5, dtype=torch.int32)
    first_ids = rest_ids = torch.zeros(1, dtype=torch.int32)


def test_wrappers_refuse_cpu_tensors_and_grad():
    from vln_goat_amd import hipops
    x, noise = torch.zeros(3, 16), torch.ones(8)
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.scale_cols(x, noise)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.scale_cols(x.clone().requires_grad_(), noise)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.scale_cols(x, noise.clone().requires_grad_())
    words = torch.zeros(2, 8, dtype=torch.int64)
    ids, masks = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.retok_rows(words, _Table, ids, masks, 7, 2, 0, 0, 2, width=4)
    state = hipops.DecodeState(2, 8, 'cpu')
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.retok_rows(state.words, _Table, ids, masks, 7, 2, 0, 0, 2, state=state)


def test_device_navigator_text_argument_is_checked_by_name():
    import inspect
    from vln_goat_amd import navdev
    for fn in (navdev.DeviceNavigator.begin, navdev.DeviceNavigator.walk):
        assert inspect.signature(fn).parameters['text'].default == 'host'
