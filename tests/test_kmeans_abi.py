"""The k-means / dictionary-pick entry points (csrc/kmeans.hip), the part that needs no GPU: they are declared, exported and bound,
reject bad arguments before any launch (no kernel runs: every call below fails validation), and the hipops wrappers are
inference-only."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE = -1, -2
NAMES = ('goat_kmeans_assign', 'goat_kmeans_csr', 'goat_kmeans_centres', 'goat_kmeans_pick')


def _lib():
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _aligned(nbytes=1024):
    buf = (ctypes.c_char * (nbytes + 16))()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_kmeans_entry_points_are_declared_exported_and_bound():
    lib = _lib()
    txt = open(os.path.join(ROOT, 'include', 'goat_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    h = lib.lib()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % name, txt), name
        assert hasattr(h, name) and name in lib.SIGNATURES
    assert h.goat_version() >= 104
    assert 'kmeans.hip' in lib.SOURCES


def _assign(h, p, dtype=0, X=True, C=True, labels=True, ld=16, N=4, D=16, K=3, xoff=0):
    return h.goat_kmeans_assign(None, dtype, p + xoff if X else None, ld, p if C else None, p if labels else None, None, None, N, D, K)


def test_assign_argument_validation_without_gpu():
    h = _lib().lib()
    keep, p = _aligned()
    assert _assign(h, p, X=False) == E_ARG
    assert _assign(h, p, C=False) == E_ARG
    assert _assign(h, p, labels=False) == E_ARG
    assert _assign(h, p, dtype=7) == E_ARG
    assert _assign(h, p, K=0) == E_SHAPE
    assert _assign(h, p, K=257) == E_SHAPE
    assert _assign(h, p, D=12, ld=12) == E_SHAPE
    assert _assign(h, p, D=0, ld=16) == E_SHAPE
    assert _assign(h, p, ld=8) == E_SHAPE                  # ld_x < D
    assert _assign(h, p, N=0) == E_SHAPE
    assert _assign(h, p, xoff=8) == E_SHAPE                # base not 16-byte aligned
    assert _assign(h, p, dtype=1, ld=20) == E_SHAPE        # bf16: 20 elements are not a multiple of the 8-element chunk
    del keep


def test_csr_centres_pick_argument_validation_without_gpu():
    h = _lib().lib()
    keep, p = _aligned()
    assert h.goat_kmeans_csr(None, None, p, p, 4, 3) == E_ARG
    assert h.goat_kmeans_csr(None, p, None, p, 4, 3) == E_ARG
    assert h.goat_kmeans_csr(None, p, p, None, 4, 3) == E_ARG
    assert h.goat_kmeans_csr(None, p, p, p, 0, 3) == E_SHAPE
    assert h.goat_kmeans_csr(None, p, p, p, 4, 0) == E_SHAPE
    assert h.goat_kmeans_csr(None, p, p, p, 4, 257) == E_SHAPE

    def centres(dtype=0, X=p, order=p, start=p, C=p, ld=16, N=4, D=16, K=3):
        return h.goat_kmeans_centres(None, dtype, X, ld, order, start, C, N, D, K)
    assert centres(X=None) == E_ARG
    assert centres(order=None) == E_ARG
    assert centres(start=None) == E_ARG
    assert centres(C=None) == E_ARG
    assert centres(dtype=2) == E_ARG
    assert centres(K=0) == E_SHAPE
    assert centres(K=257) == E_SHAPE
    assert centres(D=12, ld=12) == E_SHAPE
    assert centres(ld=8) == E_SHAPE
    assert centres(X=p + 8) == E_SHAPE
    assert centres(C=p + 4) == E_SHAPE

    def pick(dtype=0, X=p, order=p, start=p, out=p, picked=p, ld=16, N=4, D=16, K=3, B=2):
        return h.goat_kmeans_pick(None, dtype, X, ld, order, start, out, picked, N, D, K, B, 0, 0, None)
    assert pick(X=None) == E_ARG
    assert pick(out=None) == E_ARG
    assert pick(picked=None) == E_ARG
    assert pick(dtype=-1) == E_ARG
    assert pick(K=0) == E_SHAPE
    assert pick(K=257) == E_SHAPE
    assert pick(D=12, ld=12) == E_SHAPE
    assert pick(ld=8) == E_SHAPE
    assert pick(B=0) == E_SHAPE
    assert pick(X=p + 8) == E_SHAPE
    assert pick(out=p + 8) == E_SHAPE
    del keep


def test_kmeans_wrappers_refuse_cpu_tensors_and_grad():
    from vln_goat_amd import hipops
    x, c = torch.zeros(4, 16), torch.zeros(3, 16)
    labels = torch.zeros(4, dtype=torch.int32)
    start, order = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    out = torch.zeros(2, 3, 16)
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.kmeans_assign(x, c)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.kmeans_assign(x.clone().requires_grad_(), c)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.kmeans_assign(x, c.clone().requires_grad_())
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.kmeans_csr(labels, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.kmeans_centres(x, order, start, c)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.kmeans_centres(x.clone().requires_grad_(), order, start, c)
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.kmeans_pick(x, order, start, out)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.kmeans_pick(x.clone().requires_grad_(), order, start, out)


def test_frontdoor_is_exported_and_refuses_cpu_tables():
    import vln_goat_amd
    from vln_goat_amd import frontdoor
    for name in ('TIM_TSV_FIELDNAMES', 'read_tim_tsv', 'write_tim_tsv', 'extract_front_features', 'DeviceKMeans', 'KMeansPicker'):
        assert getattr(vln_goat_amd, name) is getattr(frontdoor, name)
    with pytest.raises(RuntimeError, match='GPU'):
        frontdoor.DeviceKMeans(2, init=torch.zeros(2, 16)).fit(torch.zeros(8, 16))
    with pytest.raises(ValueError):
        frontdoor.DeviceKMeans(257)
