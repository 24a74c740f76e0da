"""No-GPU part of the loss-head suite (tests/test_loss_heads_gpu.py): goat_ce_fwd / goat_ce_bwd / goat_sap_fuse_fwd / goat_sap_fuse_bwd refuse
one step beyond every limit with GOAT_E_SHAPE and every required pointer left NULL with GOAT_E_ARG (dummy aligned pointers, nothing is
launched: the entry points validate before any launch); the reference conditions and the sensitivity condition of the module hold for
every case of every table, and the tables reach every dispatch branch."""
import ctypes

import pytest

GOAT_E_ARG, GOAT_E_SHAPE = -1, -2
F32, BF16 = 0, 1


@pytest.fixture(scope='module')
def h():
    from vln_goat_amd import _lib
    return _lib.lib()


_BUF = (ctypes.c_char * 512)()
P = (ctypes.addressof(_BUF) + 15) & ~15          # a 16-byte-aligned dummy pointer (never dereferenced)


def _null_each(fn, args, required, what):
    """with every required pointer (positions in `args`, the stream left out) NULL in turn: GOAT_E_ARG"""
    for i in required:
        a = list(args)
        a[i] = None
        assert fn(None, *a) == GOAT_E_ARG, '%s: argument %d NULL' % (what, i)


def test_ce_limits(h):
    fwd = lambda x, ld, M, N: h.goat_ce_fwd(None, x, ld, M, N, P, P, P)
    assert fwd(P, 1024, 7, 1027) == GOAT_E_SHAPE        # ld < N
    assert fwd(P, 1030, 7, 1027) == GOAT_E_SHAPE        # ld % 4
    assert fwd(P + 4, 1028, 7, 1027) == GOAT_E_SHAPE    # logits not 16-byte aligned
    assert fwd(P, 1028, 0, 1027) == GOAT_E_SHAPE
    assert fwd(P, 1028, 7, 0) == GOAT_E_SHAPE
    for dt in (F32, BF16):
        bwd = lambda ld, M, N, ldo: h.goat_ce_bwd(None, dt, P, ld, M, N, P, P, P, P, ldo)
        assert bwd(1024, 7, 1027, 1028) == GOAT_E_SHAPE     # ld < N
        assert bwd(1028, 7, 1027, 1026) == GOAT_E_SHAPE     # ld_out < N
        assert bwd(1028, 0, 1027, 1028) == GOAT_E_SHAPE
        assert bwd(1028, 7, 0, 1028) == GOAT_E_SHAPE
    _null_each(h.goat_ce_fwd, (P, 1028, 7, 1027, P, P, P), (0, 4, 5, 6), 'ce fwd')
    _null_each(h.goat_ce_bwd, (F32, P, 1028, 7, 1027, P, P, P, P, 1028), (1, 5, 6, 7, 8), 'ce bwd')


def _sap_fwd(dt=F32, B=2, G=8128, W=64, **kw):
    a = dict(gs=P, ls=P, fwl=P, gl=P, ll=P, fused=P, loss=P, lse=P)
    a.update(kw)
    return (dt, a['gs'], a['ls'], a['fwl'], 1, P, P, P, P, 0, None, 1, P, P, a['gl'], a['ll'], a['fused'], a['loss'], a['lse'], B, G, W)


def _sap_bwd(dt=F32, B=2, G=8128, W=64, **kw):
    a = dict(gs=P, ls=P, fwl=P, gl=P, ll=P, fused=P, lse=P, dloss=P, dgs=P, dls=P, dfwl=P)
    a.update(kw)
    return (dt, a['gs'], a['ls'], a['fwl'], 1, P, P, P, P, 0, None, 1, P, P, a['gl'], a['ll'], a['fused'], a['lse'], a['dloss'], P, P, P, a['dgs'], a['dls'],
            a['dfwl'], B, G, W)


def test_sap_limits(h):
    for fn, args in ((h.goat_sap_fuse_fwd, _sap_fwd), (h.goat_sap_fuse_bwd, _sap_bwd)):
        for dt in (F32, BF16):
            assert fn(None, *args(dt, G=8129)) == GOAT_E_SHAPE          # (2 G + 2 W) * 4 > 64 KiB
            assert fn(None, *args(dt, G=8128, W=65)) == GOAT_E_SHAPE
            assert fn(None, *args(dt, B=0)) == GOAT_E_SHAPE
            assert fn(None, *args(dt, G=0)) == GOAT_E_SHAPE
            assert fn(None, *args(dt, W=0)) == GOAT_E_SHAPE
        assert fn(None, *args(7)) == GOAT_E_ARG                           # neither GOAT_F32 nor GOAT_BF16
        for name in ('gs', 'ls', 'gl', 'll', 'fused'):
            assert fn(None, *args(**{name: None})) == GOAT_E_ARG, name
    assert h.goat_sap_fuse_fwd(None, *_sap_fwd(lse=None)) == GOAT_E_ARG       # loss without lse
    assert h.goat_sap_fuse_bwd(None, *_sap_bwd(lse=None)) == GOAT_E_ARG       # dloss without lse
    assert h.goat_sap_fuse_bwd(None, *_sap_bwd(dfwl=None)) == GOAT_E_ARG      # fwl without dfwl
    assert h.goat_sap_fuse_bwd(None, *_sap_bwd(dgs=None)) == GOAT_E_ARG
    assert h.goat_sap_fuse_bwd(None, *_sap_bwd(dls=None)) == GOAT_E_ARG


def test_reference_and_sensitivity_conditions_hold_for_every_case():
    """the float64 reference rounded once to the output dtype inside a quarter of the bound, no row scale below 1e-6 of the largest, float32
    on the CPU inside a quarter of the bound; a dropped edge column moves the loss and is a gradient entry of at least 4 bounds"""
    import test_loss_heads_gpu as lh
    assert lh.check_all_inputs() == lh.N_CASES


def test_tables_reach_every_dispatch_branch():
    import test_loss_heads_gpu as lh
    br = lh.branches()
    assert len(br) >= 150
    missing = [k for k, v in br.items() if not v]
    assert not missing, missing
