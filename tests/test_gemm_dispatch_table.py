"""The GEMM configuration table (csrc/gemm_tiles.hpp) decides what the parent commit's scattered dispatch ladders decided: over the whole
sweep of tests/golden/gemm_dispatch_parent.json (recorded from the parent's library by scripts/record_gemm_dispatch.py) the two query
functions accept exactly the recorded configurations.  Only the queries are called — no pointer, no device — so this runs anywhere."""
import json
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOAT_E_ARG = -1


@pytest.fixture(scope='module')
def rec():
    with open(os.path.join(HERE, 'golden', 'gemm_dispatch_parent.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def h():
    from vln_goat_amd import _lib
    return _lib.lib()


def test_gemm_bf16_query_equals_the_recorded_decisions(h, rec):
    s = rec['sweep']
    accepted = {tuple(x) for x in rec['gemm_bf16_accepted']}
    n, wrong = 0, []
    for t in s['tiles']:
        for ns in s['nstages']:
            for ta, tb in s['layouts']:
                for dt in s['dtypes']:
                    for epi in s['epilogues']:
                        for split in s['splits']:
                            n += 1
                            key = (ta, tb, dt, epi, split, t, ns)
                            st = h.goat_gemm_bf16_query(*key)
                            if st != (0 if key in accepted else GOAT_E_ARG):
                                wrong.append((key, st))
    assert n == 16016 and len(accepted) > 500 and not wrong, wrong[:10]


def test_wgrad_queries_equal_the_recorded_decisions(h, rec):
    s = rec['sweep']
    accepted = {tuple(x) for x in rec['wgrad_grouped_accepted']}
    assert len(accepted) > 10
    for t in s['tiles']:
        for ns in s['nstages']:
            assert h.goat_wgrad_grouped_query(t, ns) == (0 if (t, ns) in accepted else GOAT_E_ARG), (hex(t), hex(ns))
        assert (h.goat_wgrad_balanced_ws_bytes(t) > 0) == (t in rec['wgrad_balanced_accepted']), hex(t)
    assert len(rec['wgrad_balanced_accepted']) == 3


def test_tile_candidates_are_the_recorded_lists_in_order(rec, monkeypatch):
    from vln_goat_amd import tuning
    monkeypatch.setattr(tuning, 'N_CU', 256)
    monkeypatch.setattr(tuning, '_N_CU_READ', [True])
    assert tuning.USE_PP and tuning.USE_PERSIST
    assert len(rec['tile_candidates']) > 100
    for (ta, tb, M, N), want in rec['tile_candidates']:
        assert [list(c) for c in tuning._tile_candidates(bool(ta), bool(tb), M, N)] == want, (ta, tb, M, N)


def test_python_flags_are_the_headers():
    from vln_goat_amd import tuning
    with open(os.path.join(HERE, '..', 'include', 'goat_hip.h')) as f:
        defs = {m.group(1): int(m.group(2), 16) for m in re.finditer(r'#define GOAT_GEMM_(\w+) (0x[0-9A-Fa-f]+)', f.read())}
    assert defs == {'8WAVES': tuning.EIGHT_WAVES, 'PP': tuning.PINGPONG, 'PERSIST': tuning.PERSIST}
    assert tuning.BALANCED & (tuning.EIGHT_WAVES | tuning.PINGPONG | tuning.PERSIST | 0xFF) == 0       # Python only: clear of the C flags and the ring depth


def test_balanced_fits_is_the_entry_points_rule(h, rec, monkeypatch):
    """WgradQueue._balanced_fits (which groups the tuner offers to goat_wgrad_grouped_balanced) against the entry point itself.  Called with a
    NULL workspace the entry never reaches a launch: GOAT_E_SHAPE for a group with fewer K-tile iterations than compute units, else GOAT_E_ARG
    for the workspace.  Dummy operand pointers, never read."""
    import ctypes
    import torch
    from vln_goat_amd import _lib, tuning
    from vln_goat_amd.wgrad_queue import WgradQueue
    if not torch.cuda.is_available():
        monkeypatch.setattr(tuning, 'N_CU', 256)         # what the library assumes without a device
        monkeypatch.setattr(tuning, '_N_CU_READ', [True])
    ncu = tuning.n_cu()
    buf = (ctypes.c_char * 512)()
    P = (ctypes.addressof(buf) + 15) & ~15
    groups = [[(64 * k - 63, 1, 1)] for k in (ncu - 1, ncu, ncu + 1)] + [[(65, 129, 127)] * 48, [(200, 700, 900)] * 6, [(1, 513, 257)] * 40, [(129, 300, 260)] * 21]
    seen = set()
    for t in rec['wgrad_balanced_accepted']:
        for g in groups:
            arr = (_lib.WgradProblem * len(g))()
            for q, (rows, n_out, n_in) in zip(arr, g):
                q.dy, q.ld_dy, q.x, q.ld_x, q.dw, q.ld_dw, q.dbias = P, (n_out + 7) // 8 * 8, P, (n_in + 7) // 8 * 8, P, n_in, None
                q.rows, q.n_out, q.n_in, q.accumulate = rows, n_out, n_in, 0
            st = h.goat_wgrad_grouped_balanced(None, ctypes.addressof(arr), len(g), t, None, 0)
            assert st in (-1, -2), (hex(t), g[0], st)
            items = [(torch.empty(rows, n_out, device='meta'), torch.empty(rows, n_in, device='meta')) for rows, n_out, n_in in g]
            assert WgradQueue._balanced_fits(items, t) == (st == -1), (hex(t), g[0], len(g), st)
            seen.add(st)
    assert seen == {-1, -2}
