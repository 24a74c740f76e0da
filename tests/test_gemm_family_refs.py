"""No-GPU part of the GEMM family suite (tests/test_gemm_family_gpu.py): the conditions on its float64 references hold for every case of every
table, the tables reach what they are meant to reach, and every entry of its refusal tables is refused with GOAT_E_ARG by the entry point
itself (dummy aligned pointers, nothing is launched: goat_gemm_bf16 and goat_wgrad_grouped validate before any launch)."""
import ctypes

import pytest

import test_gemm_family_gpu as gf

_BUF = (ctypes.c_char * 512)()
P = (ctypes.addressof(_BUF) + 15) & ~15          # a 16-byte-aligned dummy pointer (never dereferenced)


@pytest.fixture(scope='module')
def h():
    from vln_goat_amd import _lib
    return _lib.lib()


def test_reference_conditions_hold_for_every_case():
    """every reference finite, no S zero, float32 on the CPU inside a quarter of F, no aux between 0 and the smallest normal; prints the
    worst float32-CPU error / F of every family"""
    res = gf.check_all_inputs(verbose=True)
    assert set(res) == {'gemm_bf16', 'wgrad_grouped', 'wgrad_balanced', 'gemm_nt'} and all(n > 0 for n, _ in res.values())


def test_tables_reach_what_they_are_meant_to():
    missing = [k for k, v in gf.table_properties().items() if not v]
    assert not missing, missing


def _gemm_bf16(h, bm, ns, ta, tb, run, M=125, N=123):
    Kc = 64
    f32 = run in ('f32', 'accum', 'split2', 'split3')
    epi = dict(accum=gf.EPI_ACCUM, gelu=gf.EPI_GELU, relu=gf.EPI_RELU, dgelu=gf.EPI_MUL_DGELU, drelu=gf.EPI_MUL_DRELU).get(run, gf.EPI_NONE)
    bias = P if run in ('bf16', 'f32', 'gelu', 'relu') else None
    aux = P if run in ('gelu', 'relu', 'dgelu', 'drelu') else None
    split = int(run[5:]) if run.startswith('split') else 1
    return h.goat_gemm_bf16(None, ta, tb, 0 if f32 else 1, P, 136, P, 136, P, 136, M, N, Kc, bias, epi, aux, 136, split, bm, ns, None)


def test_refused_layouts_are_refused_by_the_entry(h):
    for bm, ns, ta, tb in sorted(gf.REFUSED_LAYOUT):
        for run in gf.RUNS:
            assert _gemm_bf16(h, bm, ns, ta, tb, run) == gf.GOAT_E_ARG, (gf.cfg_name(bm, ns), ta, tb, run)


def test_refused_runs_are_refused_by_the_entry(h):
    n = 0
    for bm, ns, ta, tb in gf.GEMM_TABLE:
        if (bm, ns, ta, tb) in gf.REFUSED_LAYOUT:
            continue
        for run in gf.RUNS:
            if gf.expected_status(bm, ns, ta, tb, run):
                assert _gemm_bf16(h, bm, ns, ta, tb, run) == gf.GOAT_E_ARG, (gf.cfg_name(bm, ns), ta, tb, run)
                n += 1
    wgrad_layout = sum(1 for p in gf.GEMM_TABLE if p[2] and p not in gf.REFUSED_LAYOUT)
    assert wgrad_layout == 18 and n == 5 * 2 * 4 + wgrad_layout * 4          # the persistent loop on two layouts; the weight-gradient layout


def test_expected_status_equals_the_query(h):
    """the GPU suite's table of refusals and the library's own table (goat_gemm_bf16_query) agree on every (configuration, layout, run)"""
    for bm, ns, ta, tb in gf.GEMM_TABLE:
        for run in gf.RUNS:
            f32 = run in ('f32', 'accum', 'split2', 'split3')
            epi = dict(accum=gf.EPI_ACCUM, gelu=gf.EPI_GELU, relu=gf.EPI_RELU, dgelu=gf.EPI_MUL_DGELU, drelu=gf.EPI_MUL_DRELU).get(run, gf.EPI_NONE)
            split = int(run[5:]) if run.startswith('split') else 1
            assert h.goat_gemm_bf16_query(ta, tb, 0 if f32 else 1, epi, split, bm, ns) == gf.expected_status(bm, ns, ta, tb, run), (gf.cfg_name(bm, ns), ta, tb, run)


def test_grouped_tables_equal_the_query(h):
    for bm, ns in gf.GROUPED_CONFIGS:
        assert h.goat_wgrad_grouped_query(bm, ns) == 0, (hex(bm), hex(ns))
    for bm, ns in gf.GROUPED_REFUSED:
        assert h.goat_wgrad_grouped_query(bm, ns) == gf.GOAT_E_ARG, (hex(bm), hex(ns))


def test_grouped_refusals_are_refused_by_the_entry(h):
    from vln_goat_amd import _lib
    arr = (_lib.WgradProblem * 1)()
    q = arr[0]
    q.dy, q.ld_dy, q.x, q.ld_x, q.dw, q.ld_dw, q.dbias = P, 136, P, 136, P, 136, None
    q.rows, q.n_out, q.n_in, q.accumulate = 65, 129, 127, 0
    for bm, ns in gf.GROUPED_REFUSED:
        assert h.goat_wgrad_grouped(None, ctypes.addressof(arr), 1, bm, ns) == gf.GOAT_E_ARG, (hex(bm), hex(ns))
    for bm in (64, 128, gf.T(192, 256)):
        assert h.goat_wgrad_balanced_ws_bytes(bm) < 0
        assert h.goat_wgrad_grouped_balanced(None, ctypes.addressof(arr), 1, bm, P, 1 << 30) == gf.GOAT_E_ARG
