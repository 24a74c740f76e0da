"""C-ABI checks of the long-sequence attention entry points that need no GPU: goat_attn_long_fwd / goat_attn_long_bwd are declared,
exported and bound, reject bad arguments before any launch, and goat_attn_fwd keeps its Lk <= 256 contract."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('goat_attn_long_fwd', 'goat_attn_long_bwd')


def _lib():
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _aligned():
    buf = (ctypes.c_char * 256)()
    return buf, ctypes.addressof(buf) & ~15


def test_long_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'goat_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\bint\s+(goat_[a-z0-9_]+)\s*\(', txt))
    lib = _lib()
    h = lib.lib()
    for n in NAMES:
        assert n in declared, '%s is not declared in include/goat_hip.h' % n
        assert hasattr(h, n), 'libgoat_hip.so does not export %s' % n
        assert n in lib.SIGNATURES
    assert lib.SIGNATURES['goat_attn_long_fwd'] == lib.SIGNATURES['goat_attn_fwd']
    assert lib.SIGNATURES['goat_attn_long_bwd'] == lib.SIGNATURES['goat_attn_bwd']
    assert h.goat_version() >= 102


def _fwd(h, dtype, Q, q_rs, Lk, p):
    return h.goat_attn_long_fwd(None, dtype, Q, q_rs, 64, p, 64, 64, p, 64, 64, p, 64, 64, None, None, p, 1, 1, 4, Lk, 0.125, 0.0, 0, 0, None)


def _bwd(h, dtype, Q, q_rs, Lk, p):
    return h.goat_attn_long_bwd(None, dtype, Q, q_rs, 64, p, 64, 64, p, 64, 64, p, 64, 64, p, 64, 64, p, 64, 64, p, 64, 64, p, 64, 64,
                                None, None, p, None, 1, 1, 4, Lk, 0.125, 0.0, 0, 0, None)


def test_long_entry_points_validate_before_any_launch():
    h = _lib().lib()
    buf, p = _aligned()
    for call in (_fwd, _bwd):
        assert call(h, 1, p, 64, 513, p) == -2          # Lk > 512
        assert call(h, 1, None, 64, 300, p) == -1       # null Q
        assert call(h, 7, p, 64, 300, p) == -1          # bad dtype
        assert call(h, 1, p, 63, 300, p) == -2          # bf16 row stride that is no multiple of 8 elements
        assert call(h, 1, p, 64, 0, p) == -2


def test_short_entry_point_keeps_its_limit():
    h = _lib().lib()
    buf, p = _aligned()
    assert h.goat_attn_fwd(None, 1, p, 64, 64, p, 64, 64, p, 64, 64, p, 64, 64, None, None, p, 1, 1, 4, 300, 0.125,
                           0.0, 0, 0, None) == -2
