"""Record which configurations the bf16 GEMM entry points of a library accept -> tests/golden/gemm_dispatch_parent.json.

    GOAT_HIP_LIB=/path/to/libgoat_hip.so python scripts/record_gemm_dispatch.py [out.json]

Run on a machine WITHOUT a GPU, against a library built from the commit whose decisions are to be pinned (the recorded file is the
parent's of the dispatch fold).  Every entry point validates before it touches the device: a refused configuration returns GOAT_E_ARG,
an accepted one goes on to hipFuncSetAttribute, which fails with HIP's "no device" status — nothing is ever launched, and the
operand pointers (host memory) are never read.  With a device present the accepted launches WOULD run on host pointers, so the script
exits at once when it sees one.  It also records tuning._tile_candidates of the same checkout for every distinct (ta, tb, M, N) of
tuned_gfx950.json (N_CU pinned to 256, the MI355X value).  tests/test_gemm_dispatch_table.py compares the query functions with the file."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: libgoat_hip.so then finds the HIP runtime torch loaded)

GOAT_E_ARG = -1
TILES = [64, 96, 128, 256, 128 | 256 << 16, 192 | 256 << 16, 256 | 192 << 16, 256 | 256 << 16, 192 | 192 << 16, 64 | 256 << 16, 32]
NSTAGES = [1, 2, 3, 4, 5, 0x102, 0x103, 0x104, 0x202, 0x203, 0x302, 0x402, 0x602]
LAYOUTS = [(0, 0), (0, 1), (1, 1), (1, 0)]
DTYPES = [0, 1]                 # GOAT_F32, GOAT_BF16
EPILOGUES = range(7)
SPLITS = [1, 2]
M = N = 64
KC = 128


def sweep():
    return [(ta, tb, dt, epi, split, t, ns) for t in TILES for ns in NSTAGES for ta, tb in LAYOUTS for dt in DTYPES for epi in EPILOGUES for split in SPLITS]


def main():
    lib_path = os.environ.get('GOAT_HIP_LIB')
    if not lib_path:
        sys.exit('set GOAT_HIP_LIB to the library to record')
    h = ctypes.CDLL(lib_path)
    n_dev = ctypes.c_int(0)
    h.hipGetDeviceCount(ctypes.byref(n_dev))
    if torch.cuda.is_available() or n_dev.value != 0:
        sys.exit('a HIP device is present: an accepted configuration would be LAUNCHED on host pointers.  Run this where there is none.')
    from vln_goat_amd import _lib, tuning

    h.goat_gemm_bf16.argtypes = _lib.SIGNATURES['goat_gemm_bf16']
    h.goat_wgrad_grouped.argtypes = _lib.SIGNATURES['goat_wgrad_grouped']
    h.goat_wgrad_grouped_balanced.argtypes = _lib.SIGNATURES['goat_wgrad_grouped_balanced']
    h.goat_wgrad_balanced_ws_bytes.argtypes = [ctypes.c_int]
    buf = (ctypes.c_char * (1 << 16))()
    P = (ctypes.addressof(buf) + 255) & ~255

    gemm = []
    for ta, tb, dt, epi, split, t, ns in sweep():
        aux = P if epi in (3, 4) else None
        st = h.goat_gemm_bf16(None, ta, tb, dt, P, 136, P, 136, P, 136, M, N, KC, None, epi, aux, 136, split, t, ns, None)
        assert st == GOAT_E_ARG or st > 0, (st, ta, tb, dt, epi, split, hex(t), hex(ns))       # refused, or stopped by "no device"
        if st != GOAT_E_ARG:
            gemm.append([ta, tb, dt, epi, split, t, ns])

    arr = (_lib.WgradProblem * 1)()
    q = arr[0]
    q.dy, q.ld_dy, q.x, q.ld_x, q.dw, q.ld_dw, q.dbias = P, 136, P, 136, P, 136, None
    q.rows, q.n_out, q.n_in, q.accumulate = 65, 129, 127, 0
    grouped, balanced = [], []
    for t in TILES:
        for ns in NSTAGES:
            st = h.goat_wgrad_grouped(None, ctypes.addressof(arr), 1, t, ns)
            assert st == GOAT_E_ARG or st > 0, (st, hex(t), hex(ns))
            if st != GOAT_E_ARG:
                grouped.append([t, ns])
        refused = h.goat_wgrad_grouped_balanced(None, ctypes.addressof(arr), 1, t, P, 1 << 16) == GOAT_E_ARG
        assert refused == (h.goat_wgrad_balanced_ws_bytes(t) < 0), hex(t)
        if not refused:
            balanced.append(t)

    tuning.N_CU, tuning._N_CU_READ[0] = 256, True
    with open(tuning.TUNED_FILE) as f:
        shapes = sorted({tuple(json.loads(k)[:4]) for k in json.load(f)})
    cands = [[list(s), [list(c) for c in tuning._tile_candidates(bool(s[0]), bool(s[1]), s[2], s[3])]] for s in shapes]

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'gemm_dispatch_parent.json')
    with open(out, 'w') as f:
        json.dump({'sweep': dict(tiles=TILES, nstages=NSTAGES, layouts=LAYOUTS, dtypes=DTYPES, epilogues=list(EPILOGUES), splits=SPLITS),
                   'gemm_bf16_accepted': gemm, 'wgrad_grouped_accepted': grouped, 'wgrad_balanced_accepted': balanced,
                   'tile_candidates': cands}, f, separators=(',', ':'))
    print('goat_gemm_bf16: %d accepted of %d; goat_wgrad_grouped: %d of %d; balanced: %s; %d shapes of tile candidates -> %s' % (
        len(gemm), len(sweep()), len(grouped), len(TILES) * len(NSTAGES), ['%dx%d' % (t & 0xFFFF, (t >> 16) or 128) for t in balanced], len(cands), out))


if __name__ == '__main__':
    main()
