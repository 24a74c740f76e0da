"""No-GPU part of the small-kernel suite (tests/test_small_kernels_gpu.py): every limit its case tables stop at is refused one step beyond
with GOAT_E_SHAPE, every required pointer left NULL gives GOAT_E_ARG (dummy aligned pointers, nothing is launched: the entry points
validate before any launch), the reference conditions of the module hold for every case of every table, and the tables reach every
dispatch branch."""
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
P3 = (ctypes.c_void_p * 3)(P, P, P)


def _null_each(fn, args, required, what):
    """with every required pointer (positions in `args`, the stream left out) NULL in turn: GOAT_E_ARG"""
    for i in required:
        a = list(args)
        a[i] = None
        assert fn(None, *a) == GOAT_E_ARG, '%s: argument %d NULL' % (what, i)


def test_pool_limits(h):
    fwd = lambda L, H: h.goat_attn_pool_fwd(None, F32, P, P, P, P, P, 2, L, H, None)
    bwd = lambda L, H: h.goat_attn_pool_bwd(None, F32, P, P, P, P, P, P, P, P, 2, L, H)
    for f in (fwd, bwd):
        assert f(513, 768) == GOAT_E_SHAPE          # POOL_MAXL = 512
        assert f(512, 6) == GOAT_E_SHAPE            # H % 4
        assert f(0, 768) == GOAT_E_SHAPE
    _null_each(h.goat_attn_pool_fwd, (F32, P, P, P, P, P, 2, 512, 768, None), (1, 2, 3, 4, 5), 'pool fwd')
    _null_each(h.goat_attn_pool_bwd, (F32, P, P, P, P, P, P, P, P, 2, 512, 768), range(1, 9), 'pool bwd')


def test_door_limits(h):
    for dt in (F32, BF16):
        assert h.goat_door_gate_bwd(None, dt, P, P, P, P, P, P, P, P, P, P, P, 4, 1025, None) == GOAT_E_SHAPE      # 64 * DOOR_MAXC = 1024
        assert h.goat_door_gate_bwd(None, dt, P, P, P, P, P, P, P, P, P, P, P, 0, 1024, None) == GOAT_E_SHAPE
        assert h.goat_door_gate_fwd(None, dt, P, P, P, P, P, P, P, P, 4, 0) == GOAT_E_SHAPE
    _null_each(h.goat_door_gate_fwd, (F32, P, P, P, P, P, P, P, P, 4, 1024), range(1, 9), 'door fwd')
    _null_each(h.goat_door_gate_bwd, (F32, P, P, P, P, P, P, P, P, P, P, P, 4, 1024, None), range(1, 12), 'door bwd')      # dbias2 may be NULL


def test_rowdot_limits(h):
    for dt in (F32, BF16):
        assert h.goat_rowdot_bwd(None, dt, P, P, P, P, P, P, 4, 1032) == GOAT_E_SHAPE       # MAXC full at 1024
        assert h.goat_rowdot_bwd(None, dt, P, P, P, P, P, P, 4, 1020) == GOAT_E_SHAPE       # H % 8
        assert h.goat_rowdot_fwd(None, dt, P, P, P, P, 4, 1020) == GOAT_E_SHAPE
        assert h.goat_rowdot_fwd(None, dt, P, P, P, P, 0, 1024) == GOAT_E_SHAPE
        # a bias gradient without a weight gradient has no kernel form: refused, with or without dx
        assert h.goat_rowdot_bwd(None, dt, P, P, P, P, None, P, 4, 1024) == GOAT_E_ARG
        assert h.goat_rowdot_bwd(None, dt, P, P, P, None, None, P, 4, 1024) == GOAT_E_ARG
        assert h.goat_rowdot_bwd(None, dt, P, P, P, None, None, None, 4, 1024) == 0         # nothing asked for: nothing launched
    _null_each(h.goat_rowdot_fwd, (F32, P, P, None, P, 4, 1024), (1, 2, 4), 'rowdot fwd')                 # the bias may be NULL
    _null_each(h.goat_rowdot_bwd, (F32, P, P, P, P, P, P, 4, 1024), (1, 2, 3), 'rowdot bwd')


def test_pano_limits(h):
    for dt in (F32, BF16):
        assert h.goat_pano_fusion_fwd(None, dt, P, P, P, P, P, 3, 65, 768) == GOAT_E_SHAPE      # V <= 64
        assert h.goat_pano_fusion_bwd(None, dt, P, P, P, P, P, P, P, P, 3, 65, 768) == GOAT_E_SHAPE
        assert h.goat_pano_fusion_fwd(None, dt, P, P, P, P, P, 3, 0, 768) == GOAT_E_SHAPE
    _null_each(h.goat_pano_fusion_fwd, (F32, P, P, P, P, P, 3, 64, 768), range(1, 6), 'pano fwd')
    _null_each(h.goat_pano_fusion_bwd, (F32, P, P, P, P, P, P, P, P, 3, 64, 768), range(1, 9), 'pano bwd')


def test_wgrad_smallk_limits(h):
    call = lambda dt, x, ld_x, K: h.goat_wgrad_smallk(None, dt, P, 128, x, ld_x, 64, 128, K, P, K, P)
    for dt, epc in ((F32, 4), (BF16, 8)):
        assert call(dt, P, 24, 17) == GOAT_E_SHAPE           # SK_MAXK = 16
        assert call(dt, P, 24, 0) == GOAT_E_SHAPE
        assert call(dt, P, 8, 9) == GOAT_E_SHAPE             # ld_x < kp (12 float32, 16 bf16)
        assert call(dt, P, 16 + epc // 2, 5) == GOAT_E_SHAPE  # ld_x % epc
        assert call(dt, P + 8, 16, 5) == GOAT_E_SHAPE        # x not 16-byte aligned
    _null_each(h.goat_wgrad_smallk, (F32, P, 128, P, 16, 64, 128, 5, P, 5, None), (1, 3, 8), 'wgrad_smallk')       # dbias may be NULL


def test_infonce_limits(h):
    fwd = lambda Bl, Ba, H, t0, tau: h.goat_infonce_fwd(None, P3, P3, P, P, P, P, Bl, Ba, H, t0, tau)
    bwd = lambda Bl, Ba, H, t0, tau: h.goat_infonce_bwd(None, P3, P3, P, P, P, P, P3, P3, P, P, Bl, Ba, H, t0, tau)
    for f in (fwd, bwd):
        assert f(33, 130, 68, 98, 0.07) == GOAT_E_SHAPE       # target0 + Bl > Ba
        assert f(131, 130, 68, 0, 0.07) == GOAT_E_SHAPE
        assert f(33, 130, 66, 64, 0.07) == GOAT_E_SHAPE       # H % 4
        assert f(33, 130, 68, 64, 0.0) == GOAT_E_SHAPE        # temperature <= 0
        assert f(33, 130, 68, 64, -0.07) == GOAT_E_SHAPE
        assert f(33, 130, 68, -1, 0.07) == GOAT_E_SHAPE
    _null_each(h.goat_infonce_fwd, (P3, P3, P, P, P, P, 33, 130, 68, 64, 0.07), range(6), 'infonce fwd')
    _null_each(h.goat_infonce_bwd, (P3, P3, P, P, P, P, P3, P3, P, P, 33, 130, 68, 64, 0.07), range(6), 'infonce bwd')
    hole = (ctypes.c_void_p * 3)(P, None, P)
    assert h.goat_infonce_fwd(None, hole, P3, P, P, P, P, 33, 130, 68, 64, 0.07) == GOAT_E_ARG


def test_gather_and_embed_limits(h):
    for dt, bad in ((F32, 6), (BF16, 12)):                    # H % epc
        assert h.goat_gather_segmean_fwd(None, dt, P, 50, P, P, None, P, 9, bad, None) == GOAT_E_SHAPE
        assert h.goat_gather_segmean_bwd(None, dt, P, P, P, None, P, 9, bad) == GOAT_E_SHAPE
        assert h.goat_embed_fwd(None, dt, P, P, None, None, None, 1, P, 8, bad, 3, None) == GOAT_E_SHAPE
        assert h.goat_embed_bwd(None, dt, P, P, None, 1, P, None, None, 600, bad, 3, -1, -1) == GOAT_E_SHAPE
    assert h.goat_gather_segmean_fwd(None, F32, P, 50, P, P, None, P, 0, 8, None) == GOAT_E_SHAPE
    assert h.goat_embed_bwd(None, F32, P, P, None, 1, P, None, None, 0, 8, 3, -1, -1) == GOAT_E_SHAPE
    _null_each(h.goat_gather_segmean_fwd, (F32, P, 50, P, P, None, P, 9, 8, None), (1, 3, 4, 6), 'gather fwd')       # scale, tok_w may be NULL
    _null_each(h.goat_gather_segmean_bwd, (F32, P, P, P, None, P, 9, 8), (1, 2, 3, 5), 'gather bwd')
    _null_each(h.goat_embed_fwd, (F32, P, P, None, None, None, 1, P, 8, 8, 3, None), (1, 2, 7), 'embed fwd')
    _null_each(h.goat_embed_bwd, (F32, P, P, None, 1, P, None, None, 600, 8, 3, -1, -1), (1, 2), 'embed bwd')


def test_dict_wsum_cfp_mix_and_colsum_arguments(h):
    _null_each(h.goat_dict_wsum_fwd, (F32, P, P, P, 3, 5, 257), (1, 2, 3), 'dict_wsum fwd')
    _null_each(h.goat_dict_wsum_bwd, (F32, P, P, P, P, P, 3, 5, 257), (1, 2, 3), 'dict_wsum bwd')                  # dz, dp may each be NULL
    _null_each(h.goat_cfp_mix_fwd, (F32, P, P, P, P, P, 3, 257), range(1, 6), 'cfp_mix fwd')
    _null_each(h.goat_cfp_mix_bwd, (F32, P, P, P, P, P, P, P, 3, 257, 1), range(1, 8), 'cfp_mix bwd')
    _null_each(h.goat_colsum, (F32, P, 136, 33, 130, P), (1, 5), 'colsum')
    assert h.goat_dict_wsum_fwd(None, F32, P, P, P, 3, 0, 257) == GOAT_E_SHAPE
    assert h.goat_cfp_mix_fwd(None, F32, P, P, P, P, P, 3, 0) == GOAT_E_SHAPE
    assert h.goat_colsum(None, F32, P, 1, 0, 1, P) == GOAT_E_SHAPE


def test_reference_conditions_hold_for_every_case():
    """the float64 reference rounded once to the output dtype inside a quarter of the bound; no row scale below 1e-6 of the largest"""
    import test_small_kernels_gpu as sk
    assert sk.check_all_inputs() == sum(len(t) for _, t, _, _ in sk.FAMILIES)


def test_tables_reach_every_dispatch_branch():
    import test_small_kernels_gpu as sk
    br = sk.branches()
    assert len(br) >= 90
    missing = [k for k, v in br.items() if not v]
    assert not missing, missing
