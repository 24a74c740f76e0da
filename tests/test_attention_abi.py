"""Argument checking of the four attention entry points (goat_attn_fwd / goat_attn_bwd for Lk <= 256, goat_attn_long_fwd /
goat_attn_long_bwd for Lk <= 512), through ctypes and without a GPU: dummy non-null pointers, a null stream, and every case is one
that an entry point answers BEFORE it launches anything.

The checks run in this order and the first that fails decides the code:
    1. a required pointer is null                                   -> GOAT_E_ARG   (-1)
    2. B, nh, Lq or Lk <= 0, or Lk above the entry point's limit     -> GOAT_E_SHAPE (-2)
    3. dtype is neither GOAT_F32 (0) nor GOAT_BF16 (1)               -> GOAT_E_ARG
    4. a checked operand whose row or batch stride is no multiple of the 16-byte chunk (8 bf16 / 4 f32 elements), or whose base
       is not 16-byte aligned                                        -> GOAT_E_SHAPE
Checked operands: Q, K, V in every entry point; O, dO, dQ in both backward passes; O in the LONG forward only (its kernel stores
four elements at a time; the short forward's general kernels store single elements).  dK and dV are checked by no entry point.

What an entry point ACCEPTS cannot be asserted here, because an accepted call launches.  The two asymmetries (O in the short
forward, dK / dV in the backward passes) therefore appear as pairs: the long forward rejects a misaligned O on that ground alone,
and the same O given to the short forward gets as far as a later row of the table (Lk = 257) without changing its answer.
"""
import ctypes
import os

import pytest

E_ARG, E_SHAPE = -1, -2
F32, BF16 = 0, 1

FWD_OPERANDS = ('Q', 'K', 'V', 'O')
BWD_OPERANDS = ('Q', 'K', 'V', 'O', 'dO', 'dQ', 'dK', 'dV')
FWD_REQUIRED = ('Q', 'K', 'V', 'O', 'lse')
BWD_REQUIRED = BWD_OPERANDS + ('lse',)
# entry point -> (operands, required pointers, operands whose strides / base the entry checks, Lk limit, an Lk it serves)
ENTRIES = {
    'goat_attn_fwd': (FWD_OPERANDS, FWD_REQUIRED, ('Q', 'K', 'V'), 256, 64),
    'goat_attn_long_fwd': (FWD_OPERANDS, FWD_REQUIRED, ('Q', 'K', 'V', 'O'), 512, 300),
    'goat_attn_bwd': (BWD_OPERANDS, BWD_REQUIRED, ('Q', 'K', 'V', 'O', 'dO', 'dQ'), 256, 64),
    'goat_attn_long_bwd': (BWD_OPERANDS, BWD_REQUIRED, ('Q', 'K', 'V', 'O', 'dO', 'dQ'), 512, 300),
}

_BUF = (ctypes.c_char * 256)()
PTR = (ctypes.addressof(_BUF) + 15) & ~15          # a 16-byte aligned address inside _BUF, never dereferenced


def _cases():
    """(id, entry point, overrides of the valid call, expected code)"""
    out = []
    for name, (operands, required, checked, limit, lk) in ENTRIES.items():
        def add(tag, over, want, name=name):
            out.append(pytest.param(name, over, want, id='%s-%s' % (name[5:], tag)))
        for ptr in required:
            add('null_%s' % ptr, {ptr: None}, E_ARG)
        for dim in ('B', 'nh', 'Lq', 'Lk'):
            add('%s_zero' % dim, {dim: 0}, E_SHAPE)
            add('%s_negative' % dim, {dim: -3}, E_SHAPE)
        add('Lk_over_limit', {'Lk': limit + 1}, E_SHAPE)
        add('dtype_2', {'dtype': 2}, E_ARG)
        for op in checked:
            add('%s_rs_bf16' % op, {'dtype': BF16, op + '_rs': 68}, E_SHAPE)          # a multiple of 4, not of 8
            add('%s_rs_f32' % op, {'dtype': F32, op + '_rs': 66}, E_SHAPE)
            add('%s_bs_bf16' % op, {'dtype': BF16, op + '_bs': 4100}, E_SHAPE)
            add('%s_bs_f32' % op, {'dtype': F32, op + '_bs': 4098}, E_SHAPE)
            add('%s_base_off_16_bytes' % op, {op: PTR + 8}, E_SHAPE)
        # first failing check wins
        add('null_and_bad_dtype', {'Q': None, 'dtype': 2}, E_ARG)
        add('null_and_bad_shape', {required[-1]: None, 'Lk': 0}, E_ARG)
        add('bad_shape_and_bad_dtype', {'Lk': limit + 1, 'dtype': 2}, E_SHAPE)
        add('bad_dtype_and_bad_stride', {'dtype': 2, 'Q_rs': 63}, E_ARG)
    # the forward asymmetry: O alone makes the long forward refuse; the short forward's checks pass it on to the next one that stops it
    for over in ({'O_rs': 68}, {'O_bs': 4100}, {'O': PTR + 8}):
        tag = {'O_rs': 'O_rs', 'O_bs': 'O_bs', 'O': 'O_base'}[next(iter(over))]
        out.append(pytest.param('goat_attn_long_fwd', dict(over, dtype=BF16), E_SHAPE, id='attn_long_fwd-rejects_%s' % tag))
        out.append(pytest.param('goat_attn_fwd', dict(over, dtype=BF16, Lk=257), E_SHAPE, id='attn_fwd-%s_then_Lk_257' % tag))
    # dK / dV are in no entry check: a short backward with such strides is answered by its Lk limit as if they were aligned
    for op in ('dK', 'dV'):
        out.append(pytest.param('goat_attn_bwd', {'dtype': BF16, op + '_rs': 68, 'Lk': 257}, E_SHAPE, id='attn_bwd-%s_rs_then_Lk_257' % op))
    return out


def _call(h, name, over):
    operands, _, _, _, lk = ENTRIES[name]
    v = {'dtype': BF16, 'kmask': None, 'bias': None, 'lse': PTR, 'dbias': None, 'B': 2, 'nh': 3, 'Lq': 40, 'Lk': lk}
    for op in operands:
        v[op], v[op + '_rs'], v[op + '_bs'] = PTR, 192, 192 * 512
    unknown = set(over) - set(v)
    assert not unknown, unknown
    v.update(over)
    args = [None, v['dtype']]
    for op in operands:
        args += [v[op], v[op + '_rs'], v[op + '_bs']]
    args += [v['kmask'], v['bias'], v['lse']]
    if len(operands) == 8:
        args.append(v['dbias'])
    args += [v['B'], v['nh'], v['Lq'], v['Lk'], 0.125, 0.0, 0, 0, None]
    return getattr(h, name)(*args)


@pytest.fixture(scope='module')
def lib():
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize('name,over,want', _cases())
def test_attention_entry_checks(lib, name, over, want):
    assert _call(lib, name, over) == want
