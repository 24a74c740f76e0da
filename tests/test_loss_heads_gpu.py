"""The loss heads — goat_ce_fwd / goat_ce_bwd (csrc/ce.hip; cross_entropy_rows and decoder_cross_entropy of hipops) and goat_sap_fuse_fwd /
goat_sap_fuse_bwd (csrc/causal.hip; hipops.sap_fuse) — at every width, padding, tail, mask spelling and NULL pointer, against float64
references on the CPU, with the method and the helpers of tests/test_small_kernels_gpu.py (read its docstring first).

Reference: float64, from the operands as the kernel receives them (bf16 scores and logits upcast from their bf16 values; the decoder weight
rounded to the compute dtype first); the ce backward from the closed form of include/goat_hip.h, the decoder and SAP backward by float64
autograd.  Nothing a kernel wrote enters a reference.

Bound: _tol(dtype) times the row scale ('row' for [rows, N] outputs, 'vec' for loss, lse, dfwl and parameter gradients), with conditions
a. b. c. of the small-kernels docstring asserted on the CPU.  Outputs the kernels compute and store in float32 from operands that are exact
in float32 (loss and lse of every ce call, the decoder loss among them: its logits leave the GEMM in float32; gl, ll, fused, loss, lse of
sap) are held to the float32 bound 1e-3 in the bf16 cases as well: the bf16 bound there would only hide the float32 arithmetic behind a
storage rounding that does not happen.  What the 'vec' scale does to lse of ce: every case with M = 7 has the rows shifted by +1000 and
-1000, so the scale of lse is about 1000 and its bound about 1.0 absolute, wider than one dropped plateau column (log(12/11) = 0.09).
The lse figures (and "lse unchanged" of the ignored rows) therefore show only that lse is the row's value to 1e-3 of 1000; a dropped
summand is caught by loss, whose scale the shifted rows leave alone (lse - x[t] cancels the shift), and by dlogits, not by lse.

Special values: -inf logits (masked slots), +inf losses (a label on a masked slot) and NaN rows (a label past the row) are part of the
contract: O(..., special=True) compares them exactly, sign included, and keeps them out of the scales.

Sensitivity (ce_ready / sap_ready, on the float64 reference alone, before any launch): the loose float32 bound only bites where one summand
matters.  Every ce and sap case has edge-plateau rows: a set E of at most 12 edge columns (ce: columns 0-3, the 8 columns around 1024 — and
2048 at N = 2049 —, the last full 4-group and the scalar tail; sap: slots 0, 63, 64, 65, 127, 128 and the last, at most 4 per sample) raised
to one common height PLATEAU above the largest other logit, the label inside E.  Asserted: removing any single column of E from the softmax
moves the row's loss by at least 4 times the bound applied to that loss, and the column's own gradient entry is at least 4 times the bound
of its gradient row (not where the gradient row is exactly zero: N = 1, a one-slot plateau).  Wide rows split E over two rows (ce) or over
the samples (sap).  In sap the condition can only be asserted in a sample with a label on that side and a finite loss, so more than 3
edges are dealt out over exactly those samples (global: plain, ragged, la < 0; local: ragged, ga < 0; sap_plateaus), and sap_ready
asserts for every case that the slots it was asserted for cover all of sap_edges(G) and all of sap_edges(W).  A case with lse but
neither a loss output nor dloss has no bound on a loss or on a label's gradient: there the same is asserted of the lse of gl and of ll
against the bound of lse (not of fused, whose edges M takes off their common height).  Only the 'neither' cases are exempt: without lse no output sums over the slots (gl, ll, fused and the
gradients of dgl, dll, dfused are slot-wise, and every slot of them is compared).
A sap case whose random fusion matrix cancels an edge's gradient entry is redrawn (`salt`), on the CPU.  The decoder cases reach the
same two kernels behind a GEMM, where no logit can be placed: they carry no plateau and no sensitivity condition.

ce rows (CE_KINDS), M = 7: flat; two edge-plateau rows; the flat row shifted by +1000 and by -1000; a third of the columns -inf (edge columns
among them) with the label on a finite column; the same with the label on a -inf column (loss +inf).  The ignored targets are a second
launch over the same logits with the targets of rows 0 and 4 replaced by -1 and -100 (loss exactly 0.0, lse unchanged, the gradient row
exactly 0.0), so that all nine kinds run in every case with M = 7.

sap samples (SAP_ROLES), B = 6, as far as the mask spelling of the case allows: plain; ragged map, visited slots, masked local slots; ga on
a masked slot (loss +inf); ga < 0; la < 0 (with add_stop and an lmask: local slot 0 masked in the ga < 0 sample); everything masked and
both labels negative (all logits -inf, loss and gradients exactly 0.0).  The local row of the plain sample is flat (its global row is a plateau).

Every figure is printed (`FIG family dtype case output[@variant] worst error / row scale`) before it is asserted, every miss reported."""
import itertools
import math
import sys

import pytest
import torch

from test_small_kernels_gpu import (BF16, DEV, F32, NAN, O, Outs, _dedup, _dn, _gen, _sd, _tol, check, check_inputs, conditioned, nan_in, row_scale)

pytestmark = pytest.mark.gpu

INF = float('inf')
PLATEAU = 10.0          # height of the edge columns above the largest other logit of the row
SENS = 4.0              # a dropped edge column moves the loss / is a gradient entry of at least SENS bounds
MAX_SALT = 16


@pytest.fixture(scope='module')
def ops():
    from vln_goat_amd import hipops
    return hipops


def _f32_conditions(c, names, what):
    """conditions a. and c. at the float32 bound for outputs stored in float32 whatever the case's dtype"""
    check_inputs(F32, {n: c['outs'][n] for n in names if n in c['outs']}, what)
    for n in names:
        if n in c['outs']:
            assert c['f32_cpu'][n] <= 0.25 * _tol(F32), '%s %s: float32 on the CPU is %.3e of the scale off the float64 reference' % (what, n, c['f32_cpu'][n])


def _drop_moves(logits, col):
    """|change of logsumexp(logits)| when column `col` leaves the softmax (float64; inf when it is the only finite one)"""
    p = float(torch.exp(logits[col] - torch.logsumexp(logits, 0)))
    return INF if p >= 1.0 else -math.log1p(-p)


# ================================================================================================ goat_ce_fwd / goat_ce_bwd
CE_NS = (1, 3, 4, 5, 8, 1020, 1023, 1024, 1025, 1027, 1028, 2049, 50265)
CE_KINDS = ('flat', 'plateau-a', 'plateau-b', 'up1000', 'down1000', 'masked', 'label-masked')
CE_IGNORED = ((0, -1), (4, -100))           # (row, target) of the second launch


def ce_edges(N):
    """columns 0-3, the 8 columns around 1024 (and 2048 below 4096: 256 threads x 4 columns a trip), the last full 4-group, the scalar tail"""
    n4 = 4 * (N >> 2)
    e = set(range(min(4, N))) | set(range(max(n4 - 4, 0), N))
    for k in ((1024, 2048) if N < 4096 else (1024,)):
        e |= {col for col in range(k - 4, k + 4) if col < N}
    return sorted(e)


def ce_plateaus(N):
    e = ce_edges(N)
    pa, pb = (e, e) if len(e) <= 12 else (e[0::2], e[1::2])
    assert len(pa) <= 12 and len(pb) <= 12
    return pa, pb


def ce_rows(N, M, in_dt, g):
    """-> logits [M, N] (float32 holding values of in_dt), targets, {row: edge columns}"""
    kinds = CE_KINDS if M == len(CE_KINDS) else ('plateau-a',) * M
    pa, pb = ce_plateaus(N)
    x = torch.randn(M, N, generator=g)
    tgt = torch.randint(0, N, (M,), generator=g)
    pick = torch.rand(M, generator=g)
    edges = {}
    for m, kind in enumerate(kinds):
        if kind.startswith('plateau'):
            e = pa if kind.endswith('a') else pb
            x[m, e] = float(x[m].max()) + PLATEAU
            tgt[m] = e[-1] if kind.endswith('a') else e[0]
            edges[m] = e
        elif kind == 'up1000':
            x[m] = x[0] + 1000.0
            tgt[m] = tgt[0]
        elif kind == 'down1000':
            x[m] = x[0] - 1000.0
            tgt[m] = tgt[0]
        elif kind in ('masked', 'label-masked') and N >= 2:
            dead = torch.zeros(N, dtype=torch.bool)
            dead[1::3] = True
            dead[ce_edges(N)[0::2]] = True
            if bool(dead.all()):
                dead[N - 1] = False
            x[m, dead] = -INF
            cols = (~dead if kind == 'masked' else dead).nonzero().flatten()
            tgt[m] = cols[-1] if kind == 'label-masked' else cols[int(pick[m] * len(cols))]
    return x.to(in_dt).float(), tgt, edges


def ce_reference(x, tgt, dloss, N, width, rdt):
    """lse = logsumexp(x[m, :N]); loss = lse - x[m, t]; dlogits = (exp(x - lse) - [n == t]) dloss, zeros in [N, width); t < 0: loss 0 and a
    zero row; t >= N: NaN loss and NaN in [0, N) -> loss, lse, dlogits"""
    xr, dl = x.to(rdt), dloss.to(rdt)
    M = x.shape[0]
    lse = torch.logsumexp(xr, 1)
    p = torch.exp(xr - lse[:, None])
    loss, d = torch.zeros(M, dtype=rdt), torch.zeros(M, width, dtype=rdt)
    for m in range(M):
        t = int(tgt[m])
        if t < 0:
            continue
        if t >= N:
            loss[m], d[m, :N] = NAN, NAN
            continue
        loss[m] = lse[m] - xr[m, t]
        d[m, :N] = p[m] * dl[m]
        d[m, t] -= dl[m]
    return loss, lse, d


def ce_outs(x, tgt, dloss, N, width, dto, rdt):
    loss, lse, d = ce_reference(x, tgt, dloss, N, width, rdt)
    exact = torch.zeros(x.shape[0], width, dtype=torch.bool)
    exact[:, N:] = True
    exact[tgt < 0] = True
    exact[(d == 0).all(1)] = True          # one finite column carrying the label (N = 1; N = 3 with two masked): exp(0) - 1, exact zeros
    return dict(loss=O(loss, 'vec', F32, (tgt < 0) | (N == 1), special=True), lse=O(lse, 'vec', F32), dl=O(d, 'row', dto, exact, special=True))


def _ce_build(name, dto, in_dt, N, M, width, mode, bump, rdt, ignored=CE_IGNORED):
    g = _gen(_sd(name), in_dt == BF16, N, M, _sd(mode), bump)
    x, tgt, edges = ce_rows(N, M, in_dt, g)
    if mode == 'labels':       # labels outside the row next to ordinary rows
        tgt = torch.tensor([N, N + 1, 2 ** 31, 2 ** 32 + 3, -2 ** 32 + 3, 3, int(tgt[6])])
        edges = {}
    c = dict(x=x, tgt=tgt, edges=edges, dloss=torch.rand(M, generator=g) + 0.5)
    c['outs'] = ce_outs(x, tgt, c['dloss'], N, width, dto, rdt)
    if mode == 'kinds' and M > 1:
        c['tgt_ign'] = tgt.clone()
        for m, v in ignored:
            c['tgt_ign'][m] = v
        c['outs_ign'] = ce_outs(x, c['tgt_ign'], c['dloss'], N, width, dto, rdt)
    return c


def ce_ready(c, N, dto, what):
    """the float32 conditions of loss and lse, and the sensitivity condition of the module docstring"""
    _f32_conditions(c, ('loss', 'lse'), what)
    if 'outs_ign' in c:
        check_inputs(dto, c['outs_ign'], what + ' ignored')
    x, o = c['x'].double(), c['outs']
    bound = _tol(F32) * float(row_scale(o['loss']))
    worst = INF
    for m, e in c['edges'].items():
        drow = o['dl']['ref'][m]
        gbound = _tol(dto) * float(drow.abs().max())
        for col in e:
            moved = _drop_moves(x[m], col)
            assert moved >= SENS * bound, '%s: row %d without column %d moves the loss by %.3e, the bound is %.3e' % (what, m, col, moved, bound)
            worst = min(worst, moved / bound if bound else INF)
            if N > 1:
                assert abs(float(drow[col])) >= SENS * gbound, '%s: gradient entry (%d, %d) is %.3e, the bound of its row is %.3e' % (
                    what, m, col, abs(float(drow[col])), gbound)
                worst = min(worst, abs(float(drow[col])) / gbound)
    return worst


def _r(n, q):
    return (n + q - 1) // q * q


def _ce_table():
    """(dtype_out, N, ld, ld_out, M, mode)"""
    t = []
    for dto in (F32, BF16):
        for N in CE_NS:
            for ld in _dedup((_r(N, 4), _r(N, 64))):
                t += [(dto, N, ld, ldo, 7, 'kinds') for ldo in _dedup((N, ld, ld + 8))]
        t.append((dto, 1027, 1028, 1036, 1, 'kinds'))
    return t


CE_TABLE = _ce_table()
CE_LABEL_TABLE = [(dto, 1027, ld, ldo, 7, 'labels') for dto in (F32, BF16) for ld, ldo in ((1028, 1027), (1088, 1096))]


def _ce_id(c):
    return '%s-N%d-ld%d-ldo%d-M%d' % (_dn(c[0]), c[1], c[2], c[3], c[4])


@conditioned
def ce_case(dto, N, ld, ld_out, M, mode, bump, rdt):
    return _ce_build('ce', dto, F32, N, M, ld_out, mode, bump, rdt)


def _ce_direct(ops, c, case, tgt, outs, tag, miss):
    """both kernels by direct calls: the logits a view into a NaN buffer with NaN padding columns, the outputs NaN inside sentinel pads"""
    dto, N, ld, ld_out, M = case[:5]
    cid = _ce_id(case)
    xp = torch.full((M, ld), NAN)
    xp[:, :N] = c['x']
    xd, td = nan_in(xp), tgt.to(DEV)
    o = Outs()
    loss, lse = o.new('loss', (M,), F32), o.new('lse', (M,), F32)
    ops.launch('goat_ce_fwd', xd, ld, M, N, td, loss, lse)
    dl = o.new('dl', (M, ld_out), dto)
    ops.launch('goat_ce_bwd', ops._dt(dl), xd, ld, M, N, td, lse, nan_in(c['dloss']), dl, ld_out)
    got = o.collect(cid, miss)
    miss += check('ce', F32, cid, outs, dict(loss=got['loss'], lse=got['lse']), tag=tag)
    miss += check('ce', dto, cid, outs, dict(dl=got['dl']), tag=tag)


@pytest.mark.parametrize('case', CE_TABLE, ids=_ce_id)
def test_ce_direct(ops, case):
    """N = 1: loss and gradient exactly 0 (their references are all zero: compared for equality)"""
    c, cid = ce_case(*case), _ce_id(case)
    check_inputs(case[0], c['outs'], cid)
    ce_ready(c, case[1], case[0], cid)
    miss = []
    _ce_direct(ops, c, case, c['tgt'], c['outs'], '', miss)
    if 'outs_ign' in c:
        _ce_direct(ops, c, case, c['tgt_ign'], c['outs_ign'], '@ignored', miss)
    assert not miss, miss


@pytest.mark.parametrize('case', CE_LABEL_TABLE, ids=_ce_id)
def test_ce_labels_outside_the_row(ops, case):
    """targets N, N + 1, 2^31, 2^32 + 3 (NaN loss, NaN in dlogits[m, :N], zeros in the padding: compared at their 64-bit width in both
    directions) and -2^32 + 3 (negative: an ignored row) next to two ordinary rows; the moat and the sentinels stay intact"""
    c, cid = ce_case(*case), _ce_id(case)
    check_inputs(case[0], c['outs'], cid)
    _f32_conditions(c, ('loss', 'lse'), cid)
    assert int(torch.isnan(c['outs']['loss']['spec']).sum()) == 4 and bool(c['outs']['dl']['zero'][4].all())
    miss = []
    _ce_direct(ops, c, case, c['tgt'], c['outs'], '@labels', miss)
    assert not miss, miss


# ---------------------------------------------------------------- hipops.cross_entropy_rows
CER_TABLE = [(dt, N) for dt in (F32, BF16) for N in (4, 60, 64, 1028, 37)]
def cer_is_kernel(N):
    """cross_entropy_rows: goat_ce_* for row widths that are a multiple of 4, torch otherwise"""
    return N % 4 == 0


def cer_ignored(N):
    """(row, target) of the second call: any negative target on the kernel route; the torch route (N % 4) knows ignore_index = -100 only"""
    return ((0, -1), (4, -100)) if cer_is_kernel(N) else ((0, -100), (4, -100))


@conditioned
def cer_case(dt, N, bump, rdt):
    return _ce_build('ce-rows', dt, dt, N, 7, N, 'kinds', bump, rdt, cer_ignored(N))


@pytest.mark.parametrize('case', CER_TABLE, ids=lambda c: '%s-N%d' % (_dn(c[0]), c[1]))
def test_cross_entropy_rows(ops, case):
    """logits given in float32 and in bf16, the gradient through autograd in the dtype of the logits"""
    dt, N = case
    c, cid = cer_case(*case), '%s-N%d' % (_dn(dt), N)
    check_inputs(dt, c['outs'], cid)
    ce_ready(c, N, dt, cid)
    miss = []
    for tgt, outs, tag in ((c['tgt'], c['outs'], ''), (c['tgt_ign'], c['outs_ign'], '@ignored')):
        x = c['x'].to(dt).to(DEV).requires_grad_(True)
        loss = ops.cross_entropy_rows(x, tgt.to(DEV))
        loss.backward(c['dloss'].to(DEV))
        torch.cuda.synchronize()
        assert loss.dtype == F32 and x.grad.dtype == dt
        miss += check('ce-rows', F32, cid, outs, dict(loss=loss), tag=tag)
        miss += check('ce-rows', dt, cid, outs, dict(dl=x.grad), tag=tag)
    assert not miss, miss


# ---------------------------------------------------------------- hipops.decoder_cross_entropy
DEC_TABLE = [(dt, M, K, N) for dt in (F32, BF16) for M, K, N in ((5, 64, 130), (9, 768, 1000), (3, 64, 50265))]


def _dec_id(c):
    return '%s-M%d-K%d-N%d' % (_dn(c[0]), c[1], c[2], c[3])


@conditioned
def dec_case(dt, M, K, N, bump, rdt):
    """loss[m] = CE(h[m] . Wq^T + b, t[m]) with Wq the weight rounded to the compute dtype; targets of -100 are ignored rows"""
    g = _gen(_sd('decoder'), dt == BF16, M, K, N, bump)
    c = dict(h=torch.randn(M, K, generator=g).to(dt), w=torch.randn(N, K, generator=g) * 0.05, b=torch.randn(N, generator=g) * 0.1,
             tgt=torch.randint(0, N, (M,), generator=g), dloss=torch.rand(M, generator=g) + 0.5,
             base=dict(dw=torch.randn(N, K, generator=g), db=torch.randn(N, generator=g)))
    c['tgt'][1] = -100
    if M > 4:
        c['tgt'][M - 1] = -100
    h, w, b = (t.to(rdt).clone().requires_grad_(True) for t in (c['h'], c['w'].to(dt), c['b']))
    live = c['tgt'] >= 0
    loss = torch.zeros(M, dtype=rdt)
    loss[live] = torch.nn.functional.cross_entropy((h @ w.T + b)[live], c['tgt'][live], reduction='none')
    loss.backward(c['dloss'].to(rdt))
    c['outs'] = dict(loss=O(loss, 'vec', F32, ~live), dh=O(h.grad, 'row', dt, ~live[:, None]), dw=O(w.grad, 'vec', F32), db=O(b.grad, 'vec', F32))
    return c


@pytest.mark.parametrize('sunk', [False, True], ids=['grad', 'sink'])
@pytest.mark.parametrize('case', DEC_TABLE, ids=_dec_id)
def test_decoder_cross_entropy(ops, case, sunk):
    """plain .grad, and weight and bias bound to gradient sinks on a non-zero base (the protocol of test_linear_short_input_weight_gradient):
    sink - base against the same reference"""
    dt, M, K, N = case
    c, cid = dec_case(*case), _dec_id(case)
    check_inputs(dt, c['outs'], cid)
    _f32_conditions(c, ('loss',), cid)
    h = c['h'].to(DEV).requires_grad_(True)
    w, b = torch.nn.Parameter(c['w'].to(DEV)), torch.nn.Parameter(c['b'].to(DEV))
    if sunk:
        for prm, base in ((w, c['base']['dw']), (b, c['base']['db'])):
            prm.grad = base.to(DEV)
            prm.__dict__['_goat_sink'] = prm.grad
            prm.__dict__['_goat_prezero'] = True          # "cleared at step start": the kernels only ever add
    try:
        loss = ops.decoder_cross_entropy(h, w, b, c['tgt'].to(DEV))
        loss.backward(c['dloss'].to(DEV))
        torch.cuda.synchronize()
    finally:
        for prm in (w, b):
            prm.__dict__.pop('_goat_sink', None)
            prm.__dict__.pop('_goat_prezero', None)
    tag = '@sink' if sunk else ''
    miss = check('decoder', F32, cid, c['outs'], dict(loss=loss), tag=tag)       # float32 logits out of the GEMM, float32 loss: the float32 bound
    miss += check('decoder', dt, cid, c['outs'], dict(dh=h.grad, dw=w.grad, db=b.grad), c['base'] if sunk else None, tag)
    assert not miss, miss


# ================================================================================================ goat_sap_fuse_fwd / goat_sap_fuse_bwd
SAP_DIMS = ((1, 1), (1, 5), (23, 38), (63, 65), (64, 64), (65, 63), (129, 1), (150, 71), (200, 130))
SAP_ROLES = ('plain', 'ragged', 'ga-masked', 'ga-negative', 'la-negative', 'all-masked')
MASKS = ('none', 'vis+lens', 'vis+valid', 'all')
LMASKS = ('null', 'masked', 'valid')
MATS = ('null', 'binary', 'real')
FWLS = ('null', 'sigmoid', 'raw')
FOUTS = ('loss+lse', 'lse', 'neither')
UPS = ('dloss', 'dgl+dll+dfused', 'all', 'dloss+dfused')
SAP_LDS = (8128, 64)              # (2 G + 2 W) * 4 = 64 KiB exactly
SAP_BAD = lambda n: (n, n + 1, 2 ** 31, 2 ** 32 + 2, -2 ** 32 + 2)


def sap_edges(n):
    return sorted({s for s in (0, 63, 64, 65, 127, 128, n - 1) if 0 <= s < n})


SAP_CARRIERS = dict(g=('plain', 'ragged', 'la-negative'), l=('ragged', 'ga-negative'))      # the roles with a finite loss and a label on that side


def sap_plateaus(n, roles, side):
    """-> the edge slots of every sample.  Up to 3 edges: all of them in every sample.  More: dealt out over the carriers of the side, the
    samples whose role keeps a label on that side and a finite loss, so that the condition is asserted for every edge (sap_ready checks
    the union); the first local carrier, ragged, gets slot 0, which the ga-negative sample masks under add_stop.  The other samples (their
    loss is +inf or has no term of that side) get the slots of one carrier."""
    e = sap_edges(n)
    if len(e) <= 3:
        return [list(e) for _ in roles]
    carriers = [b for b, role in enumerate(roles) if role in SAP_CARRIERS[side]]
    nc = len(carriers)
    return [e[carriers.index(b)::nc] if b in carriers else e[b % nc::nc] for b in range(len(roles))]


def _sap_table():
    """(dtype, G, W, mask spelling, lmask, add_stop, M, fwl, forward outputs, upstream, kind): every (mask, lmask, add_stop) triple three
    times per dtype, the other axes cycled against them with different strides (branches() checks what that reaches)"""
    t = []
    trip = list(itertools.product(MASKS, LMASKS, (0, 1)))
    for dt in (F32, BF16):
        for rep in range(3):
            for i, (mk, lm, st) in enumerate(trip):
                j = rep * len(trip) + i
                fout = FOUTS[(j + j // 3) % 3]
                up = UPS[1] if fout == 'neither' else UPS[(j + j // 4) % 4]
                t.append((dt,) + SAP_DIMS[(2 * j + rep) % 9] + (mk, lm, st, MATS[(j + j // 3 + rep) % 3], FWLS[(j // 2 + rep) % 3], fout, up, 'roles'))
    return t


SAP_TABLE = _sap_table()
SAP_LDS_TABLE = [(dt,) + SAP_LDS + ('vis+lens', 'masked', 1, 'null', 'sigmoid', 'loss+lse', 'all', 'lds') for dt in (F32, BF16)]
SAP_LABEL_TABLE = [(dt, G, W, 'vis+lens', 'masked', 1, 'binary', 'sigmoid', 'loss+lse', 'all', 'labels') for dt in (F32, BF16) for G, W in ((23, 38), (65, 63))]


def _sap_id(c):
    return '%s-G%d-W%d-%s-l%s-s%d-M%s-f%s-%s-%s' % ((_dn(c[0]),) + tuple(c[1:10]))


def _sap_inputs(dt, G, W, mk, lm, st, mm, fk, up, kind, g):
    """the operands as the kernels receive them (CPU tensors; masks as bool, True = masked for `lmd`)"""
    roles = {'roles': SAP_ROLES, 'lds': SAP_ROLES[:2], 'labels': ('plain',) * 12}[kind]
    B = len(roles)
    gs, ls = torch.randn(B, G, generator=g), torch.randn(B, W, generator=g)
    fwl = None
    if fk == 'sigmoid':
        fwl = torch.randn(B, generator=g).clamp(-1.5, 1.5).to(dt)
    elif fk == 'raw':
        fwl = (torch.rand(B, generator=g) * 0.6 + 0.2).to(dt)              # drawn in (0, 1)
    fw = torch.full((B,), 0.5, dtype=torch.float64) if fwl is None else torch.sigmoid(fwl.double()) if fk == 'sigmoid' else fwl.double()
    eg, ew = sap_plateaus(G, roles, 'g'), sap_plateaus(W, roles, 'l')
    vis, valid = torch.zeros(B, G, dtype=torch.bool), torch.ones(B, G, dtype=torch.bool)
    lens = torch.full((B,), G, dtype=torch.int64)
    lmd = torch.zeros(B, W, dtype=torch.bool)
    ga = torch.tensor([e[-1] for e in eg])
    la = torch.tensor([e[0] for e in ew])
    u = torch.rand(B, G, generator=g), torch.rand(B, W, generator=g), torch.rand(B, 2, generator=g)
    if kind == 'roles' and W > 1:                        # the plain sample keeps a flat local row: on plateaus alone dfwl = dl (E_p[ls] - ls[la]) cancels
        ew[0] = []
        la[0] = int(u[2][0, 0] * W)
    for b, role in enumerate(roles):
        gm, lmk = mk != 'none', lm != 'null'
        if role == 'ragged':
            if gm:
                vis[b] = u[0][b] < 0.25
                vis[b, eg[b]] = False
                lo = max(eg[b]) + 1
                cut = [lo + int(float(u[2][b, k]) * (G - lo + 1)) for k in range(2)]
                if mk in ('vis+lens', 'all'):
                    lens[b] = cut[0]
                if mk in ('vis+valid', 'all'):
                    valid[b, cut[1]:] = False
            if lmk:
                lmd[b] = u[1][b] < 0.3
                lmd[b, ew[b]] = False
        elif role == 'ga-masked' and gm and G > len(eg[b]):
            ga[b] = [s for s in range(G) if s not in eg[b]][-1]
            vis[b, ga[b]] = True
        elif role == 'ga-negative':
            ga[b] = -1
            if lmk and st and W > 1:                     # add_stop reads local slot 0: masked here
                ew[b] = [s for s in ew[b] if s != 0]
                if len(ew[b]) == 1 and W > 2:            # (a one-slot plateau among live slots: 1 - p cancels in float32, for any kernel)
                    ew[b] = [W - 2, W - 1]
                la[b] = ew[b][0]
                lmd[b, 0] = True
        elif role == 'la-negative':
            la[b] = -1
        elif role == 'all-masked':
            ga[b], la[b] = -100, -7
            if mk == 'vis+lens':
                lens[b] = 0
            elif mk == 'vis+valid':
                valid[b] = False
            elif mk == 'all':
                vis[b] = True
            if lmk:
                lmd[b] = True
    if kind == 'labels':                                 # labels outside the range next to ordinary ones: they contribute nothing
        for i, (bg, bw) in enumerate(zip(SAP_BAD(G), SAP_BAD(W))):
            ga[i], la[5 + i] = bg, bw
    for b in range(B):
        gs[b, eg[b]] = float(gs[b].max()) + PLATEAU / float(fw[b])
        if ew[b]:
            ls[b, ew[b]] = float(ls[b].max()) + PLATEAU / float(1 - fw[b])
    M = None if mm == 'null' else (torch.rand(B, G, W, generator=g) < 0.3).float() if mm == 'binary' else torch.rand(B, G, W, generator=g)
    amp = 0.01 if 'dloss' in up or up == 'all' else 1.0
    d = dict(dloss=torch.rand(B, generator=g) + 0.5, dgl=amp * torch.randn(B, G, generator=g), dll=amp * torch.randn(B, W, generator=g),
             dfused=amp * torch.randn(B, G, generator=g))
    want = dict(zip(UPS, (('dloss',), ('dgl', 'dll', 'dfused'), ('dloss', 'dgl', 'dll', 'dfused'), ('dloss', 'dfused'))))[up]
    gmask = vis.clone()
    if mk in ('vis+valid', 'all'):
        gmask |= ~valid
    if mk in ('vis+lens', 'all'):
        gmask |= torch.arange(G)[None] >= lens[:, None]
    return dict(B=B, gs=gs.to(dt), ls=ls.to(dt), fwl=fwl, vis=vis, valid=valid, lens=lens, lmd=lmd, M=M, ga=ga, la=la, eg=eg, ew=ew, gmask=gmask,
                up={k: (v if k in want else None) for k, v in d.items()})


def sap_reference(c, G, W, lm, st, fk, rdt):
    """the formulas of include/goat_hip.h in `rdt`, the backward by autograd -> {name: tensor}"""
    B = c['B']
    gs, ls = c['gs'].to(rdt).clone().requires_grad_(True), c['ls'].to(rdt).clone().requires_grad_(True)
    fwl = None if c['fwl'] is None else c['fwl'].to(rdt).clone().requires_grad_(True)
    fw = torch.full((B,), 0.5, dtype=rdt) if fwl is None else torch.sigmoid(fwl) if fk == 'sigmoid' else fwl
    ninf = torch.full((), -INF, dtype=rdt)
    lmd = c['lmd'] if lm != 'null' else torch.zeros_like(c['lmd'])
    gl = torch.where(c['gmask'], ninf, gs * fw[:, None])
    lraw = ls * (1 - fw[:, None])
    ll = torch.where(lmd, ninf, lraw)
    fused = gl
    if c['M'] is not None:
        fused = fused + torch.bmm(c['M'].to(rdt), torch.where(lmd, torch.zeros((), dtype=rdt), lraw)[:, :, None])[:, :, 0]
    if st:
        fused = fused + torch.cat([ll[:, :1], torch.zeros(B, G - 1, dtype=rdt)], 1)
    with torch.no_grad():
        lse = torch.stack([torch.logsumexp(t, 1) for t in (gl, ll, fused)], 1)
    terms = []
    for b in range(B):
        t = torch.zeros((), dtype=rdt)
        if 0 <= int(c['ga'][b]) < G:
            a = int(c['ga'][b])
            t = t + (torch.logsumexp(gl[b], 0) - gl[b, a]) + (torch.logsumexp(fused[b], 0) - fused[b, a])
        if 0 <= int(c['la'][b]) < W:
            t = t + torch.logsumexp(ll[b], 0) - ll[b, int(c['la'][b])]
        terms.append(t)
    loss = torch.stack(terms)
    roots = [(t, c['up'][k].to(rdt)) for t, k in ((loss, 'dloss'), (gl, 'dgl'), (ll, 'dll'), (fused, 'dfused')) if c['up'][k] is not None and t.requires_grad]
    torch.autograd.backward([t for t, _ in roots], [d for _, d in roots])
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    r = dict(gl=gl, ll=ll, fused=fused, loss=loss, lse=lse, dgs=z(gs), dls=z(ls))
    if fwl is not None:
        r['dfwl'] = z(fwl)
    return {k: v.detach() for k, v in r.items()}


def sap_build(dt, G, W, mk, lm, st, mm, fk, fout, up, kind, salt, bump, rdt):
    g = _gen(_sd('sap'), dt == BF16, G, W, MASKS.index(mk), LMASKS.index(lm), st, MATS.index(mm), FWLS.index(fk), UPS.index(up), _sd(kind), salt, bump)
    c = _sap_inputs(dt, G, W, mk, lm, st, mm, fk, up, kind, g)
    r = sap_reference(c, G, W, lm, st, fk, rdt)
    labelled = ((c['ga'] >= 0) & (c['ga'] < G)) | ((c['la'] >= 0) & (c['la'] < W))
    lmd = c['lmd'] if lm != 'null' else torch.zeros_like(c['lmd'])
    none_g, none_l = r['dgs'].abs().amax(1, keepdim=True) == 0, r['dls'].abs().amax(1, keepdim=True) == 0      # rows no gradient reaches: exact zeros
    outs = dict(gl=O(r['gl'], 'row', F32, special=True), ll=O(r['ll'], 'row', F32, special=True), fused=O(r['fused'], 'row', F32, special=True),
                dgs=O(r['dgs'], 'row', dt, c['gmask'] | none_g), dls=O(r['dls'], 'row', dt, lmd | none_l))
    if fout == 'loss+lse':
        outs['loss'] = O(r['loss'], 'vec', F32, ~labelled, special=True)
    if fout != 'neither':
        outs['lse'] = O(r['lse'], 'vec', F32, special=True)
    if 'dfwl' in r:
        outs['dfwl'] = O(r['dfwl'], 'vec', dt, (none_g & none_l)[:, 0])
    c['outs'], c['probe'] = outs, r
    return c


def sap_ready(c, case, what):
    """the float32 conditions of the float32 outputs, and the sensitivity condition of the module docstring -> the smallest margin"""
    dt, G, W = case[:3]
    up = case[9]
    _f32_conditions(c, ('gl', 'll', 'fused', 'loss', 'lse'), what)
    r, o = c['probe'], c['outs']
    worst = INF
    with_loss = 'loss' in o
    bound = _tol(F32) * float(row_scale(o['loss'])) if with_loss else 0.0
    lse_alone = 'lse' in o and not with_loss and up == UPS[1]
    lbound = _tol(F32) * float(row_scale(o['lse'])) if lse_alone else 0.0
    held = dict(dgs=set(), dls=set())                   # the slots for which the condition was asserted, per side, over the samples
    for b in range(c['B']):
        sides = []
        if 0 <= int(c['ga'][b]) < G and int(c['ga'][b]) in c['eg'][b]:
            sides.append((c['eg'][b], (r['gl'][b], r['fused'][b]), 'dgs'))
        if 0 <= int(c['la'][b]) < W and int(c['la'][b]) in c['ew'][b]:
            sides.append((c['ew'][b], (r['ll'][b],), 'dls'))
        if not math.isfinite(float(r['loss'][b])):       # ga on a masked slot: no carrier of either side (sap_plateaus)
            continue
        for e, rows, dname in sides:
            grow = o[dname]['ref'][b]
            gbound = _tol(dt) * float(grow.abs().max())
            for s in e:
                if with_loss:
                    moved = sum(_drop_moves(t.double(), s) for t in rows)
                    assert moved >= SENS * bound, '%s: sample %d without slot %d of %s moves the loss by %.3e, the bound is %.3e' % (what, b, s, dname, moved, bound)
                    worst = min(worst, moved / bound if bound else INF)
                if up != UPS[1] and len(e) > 1:
                    assert abs(float(grow[s])) >= SENS * gbound, '%s: %s entry (%d, %d) is %.3e, the bound of its row is %.3e' % (
                        what, dname, b, s, abs(float(grow[s])), gbound)
                    worst = min(worst, abs(float(grow[s])) / gbound)
                if lse_alone:                            # no loss and no dloss: the lse of the sample are the only sums over the slots
                    moved = _drop_moves(rows[0].double(), s)         # (of gl and of ll: M takes the edges of fused off their common height)
                    assert moved >= SENS * lbound, '%s: sample %d without slot %d of %s moves its lse by %.3e, the bound is %.3e' % (what, b, s, dname, moved, lbound)
                    worst = min(worst, moved / lbound)
                held[dname].add(s)                       # (a one-slot row under dloss alone: softmax 1, gradient exactly zero, nothing to drop)
    if 'lse' in o:                                       # 'neither': no output sums over the slots (gl, ll, fused and the gradients of dgl, dll, dfused are slot-wise)
        for dname, n in (('dgs', G), ('dls', W)):
            lost = sorted(set(sap_edges(n)) - held[dname])
            assert not lost, '%s: the sensitivity condition was asserted for no sample at the edge slots %s of %s' % (what, lost, dname)
    return worst


@conditioned
def _sap_conditioned(dt, G, W, mk, lm, st, mm, fk, fout, up, kind, salt, bump, rdt):
    return sap_build(dt, G, W, mk, lm, st, mm, fk, fout, up, kind, salt, bump, rdt)


_SAP_CACHE = {}


def sap_case(*case):
    """the conditioned case whose sensitivity condition holds too (the draw is moved on by `salt`; CPU work on the references alone)"""
    if case not in _SAP_CACHE:
        why = None
        for salt in range(MAX_SALT):
            c = _sap_conditioned(*case, salt)
            try:
                c = dict(c, margin=sap_ready(c, case, _sap_id(case)), salt=salt)
            except AssertionError as ex:
                why = str(ex)
                continue
            _SAP_CACHE[case] = c
            break
        else:
            raise AssertionError('no draw among %d meets the sensitivity condition: %s' % (MAX_SALT, why))
    return _SAP_CACHE[case]


def _sap_device(c, case):
    """-> the optional arguments of both entry points, as the case spells them"""
    dt, G, W, mk, lm, st, mm, fk = case[:8]
    u8 = lambda t: t.to(torch.uint8).to(DEV)
    return dict(gvis=u8(c['vis']) if mk != 'none' else None, gvalid=u8(c['valid']) if mk in ('vis+valid', 'all') else None,
                glens=c['lens'].to(DEV) if mk in ('vis+lens', 'all') else None,
                lmask=None if lm == 'null' else u8(c['lmd'] if lm == 'masked' else ~c['lmd']), lvalid=int(lm == 'valid'),
                M=None if c['M'] is None else nan_in(c['M']), ga=c['ga'].to(DEV), la=c['la'].to(DEV))


def _sap_run(ops, case, miss):
    dt, G, W, mk, lm, st, mm, fk, fout, up, kind = case
    c, cid = sap_case(*case), _sap_id(case)
    B, outs = c['B'], c['outs']
    check_inputs(dt, outs, cid)
    a = _sap_device(c, case)

    def split(got, tag):
        f32 = {k: v for k, v in got.items() if k in ('gl', 'll', 'fused', 'loss', 'lse')}
        return check('sap', F32, cid, outs, f32, tag=tag) + check('sap', dt, cid, outs, {k: v for k, v in got.items() if k not in f32}, tag=tag)

    if fout != 'lse':                  # hipops.sap_fuse gives loss and lse together or not at all
        gs, ls = c['gs'].to(DEV).requires_grad_(True), c['ls'].to(DEV).requires_grad_(True)
        fwl = None if c['fwl'] is None else c['fwl'].to(DEV).requires_grad_(True)
        res = ops.sap_fuse(gs, ls, fwl, fw_sigmoid=fk != 'raw', gvis=a['gvis'], gvalid=a['gvalid'], glens=a['glens'], lmask=a['lmask'],
                           lmask_is_valid=bool(a['lvalid']), M=None if c['M'] is None else c['M'].to(DEV), add_stop=bool(st),
                           labels=(a['ga'], a['la']) if fout == 'loss+lse' else None)
        roots = [(t, c['up'][k].to(DEV)) for t, k in zip(res, ('dgl', 'dll', 'dfused', 'dloss')) if c['up'][k] is not None]
        torch.autograd.backward([t for t, _ in roots], [d for _, d in roots])
        torch.cuda.synchronize()
        got = dict(gl=res[0], ll=res[1], fused=res[2], dgs=gs.grad, dls=ls.grad)
        if fout == 'loss+lse':
            got['loss'] = res[3]
        if fwl is not None:
            got['dfwl'] = fwl.grad
        miss += split(got, '')
    gs, ls = nan_in(c['gs']), nan_in(c['ls'])
    fwl = None if c['fwl'] is None else nan_in(c['fwl'])
    labels = fout != 'neither'
    o = Outs()
    gl, ll, fused = o.new('gl', (B, G), F32), o.new('ll', (B, W), F32), o.new('fused', (B, G), F32)
    loss = o.new('loss', (B,), F32) if fout == 'loss+lse' else None
    lse = o.new('lse', (B, 3), F32) if labels else None
    ga, la = (a['ga'], a['la']) if labels else (None, None)
    code = ops._dt(gs)
    ops.launch('goat_sap_fuse_fwd', code, gs, ls, fwl, int(fk != 'raw'), a['gvis'], a['gvalid'], a['glens'], a['lmask'], a['lvalid'], a['M'], st, ga, la,
               gl, ll, fused, loss, lse, B, G, W)
    d = {k: None if v is None else nan_in(v) for k, v in c['up'].items()}
    dgs, dls = o.new('dgs', (B, G), dt), o.new('dls', (B, W), dt)
    dfwl = o.new('dfwl', (B,), dt) if fwl is not None else None
    ops.launch('goat_sap_fuse_bwd', code, gs, ls, fwl, int(fk != 'raw'), a['gvis'], a['gvalid'], a['glens'], a['lmask'], a['lvalid'], a['M'], st, ga, la,
               gl, ll, fused, lse, d['dloss'], d['dgl'], d['dll'], d['dfused'], dgs, dls, dfwl, B, G, W)
    miss += split(o.collect(cid, miss), '@direct')


@pytest.mark.parametrize('case', SAP_TABLE, ids=_sap_id)
def test_sap_fuse(ops, case):
    """through hipops.sap_fuse (where its form exists: loss and lse together or neither), then by direct calls inside pads"""
    miss = []
    _sap_run(ops, case, miss)
    assert not miss, miss


@pytest.mark.parametrize('case', SAP_LDS_TABLE, ids=_sap_id)
def test_sap_fuse_at_the_lds_limit(ops, case):
    """G = 8128, W = 64: the four LDS rows of the forward fill 64 KiB exactly; G = 8129 is refused (tests/test_loss_heads_abi.py)"""
    assert (2 * case[1] + 2 * case[2]) * 4 == 64 * 1024
    miss = []
    _sap_run(ops, case, miss)
    assert not miss, miss


@pytest.mark.parametrize('case', SAP_LABEL_TABLE, ids=_sap_id)
def test_sap_labels_outside_the_range(ops, case):
    """ga in (G, G + 1, 2^31, 2^32 + 2, -2^32 + 2) with la valid, the same for la with ga valid, two ordinary samples: a label >= G (>= W) at
    its 64-bit width and a negative label contribute nothing to the loss or to a gradient"""
    c = sap_case(*case)
    assert c['ga'][:5].tolist() == list(SAP_BAD(case[1])) and c['la'][5:10].tolist() == list(SAP_BAD(case[2]))
    miss = []
    _sap_run(ops, case, miss)
    assert not miss, miss


# ================================================================================================ the tables as a whole (no GPU)
def _lane_class(n):
    return 'one trip' if n < 64 else 'exactly 64' if n == 64 else '65' if n == 65 else 'more than 128' if n > 128 else 'two trips'


def check_all_inputs(verbose=False):
    """conditions a. b. c. and the sensitivity condition over every case of every table -> number of cases"""
    n = 0

    def say(name, cid, c, margin):
        if verbose:
            print('ok %s %s  seed bump %d%s  smallest sensitivity margin %s bounds  float32 on the CPU / row scale: %s' % (
                name, cid, c['bump'], ' salt %d' % c['salt'] if 'salt' in c else '', 'n/a' if margin is None else '%.1f' % margin,
                ' '.join('%s %.1e' % kv for kv in sorted(c['f32_cpu'].items()))))

    for case in CE_TABLE + CE_LABEL_TABLE:
        c, cid = ce_case(*case), _ce_id(case)
        check_inputs(case[0], c['outs'], cid)
        say('ce', cid, c, ce_ready(c, case[1], case[0], cid))
        n += 1
    for case in CER_TABLE:
        c, cid = cer_case(*case), '%s-N%d' % (_dn(case[0]), case[1])
        check_inputs(case[0], c['outs'], cid)
        say('ce-rows', cid, c, ce_ready(c, case[1], case[0], cid))
        n += 1
    for case in DEC_TABLE:
        c = dec_case(*case)
        check_inputs(case[0], c['outs'], _dec_id(case))
        _f32_conditions(c, ('loss',), _dec_id(case))
        say('decoder', _dec_id(case), c, None)
        n += 1
    for case in SAP_TABLE + SAP_LDS_TABLE + SAP_LABEL_TABLE:
        c = sap_case(*case)
        check_inputs(case[0], c['outs'], _sap_id(case))
        say('sap', _sap_id(case), c, c['margin'])
        n += 1
    return n


N_CASES = len(CE_TABLE) + len(CE_LABEL_TABLE) + len(CER_TABLE) + len(DEC_TABLE) + len(SAP_TABLE) + len(SAP_LDS_TABLE) + len(SAP_LABEL_TABLE)


def branches():
    """every dispatch branch, loop boundary and NULL test of the four entry points -> whether a case of the tables reaches it"""
    b = {}
    for dto in (F32, BF16):
        d = _dn(dto)
        ce = [c for c in CE_TABLE if c[0] == dto]
        for N in CE_NS:
            b['ce N=%d %s' % (N, d)] = any(c[1] == N for c in ce)
        b['ce scalar tail ' + d] = any(c[1] % 4 for c in ce)
        b['ce no vector group ' + d] = any(c[1] < 4 for c in ce)
        b['ce second trip of the block ' + d] = any(c[1] > 1024 for c in ce)
        b['ce tail in the second trip ' + d] = any(c[1] > 1024 and c[1] % 4 for c in ce)
        b['ce ld = N ' + d] = any(c[2] == c[1] for c in ce)
        b['ce ld > N ' + d] = any(c[2] > c[1] for c in ce)
        b['ce ld %% 64 ' + d] = any(c[2] % 64 == 0 and c[2] > _r(c[1], 4) for c in ce)
        b['ce ld_out = N ' + d] = any(c[3] == c[1] for c in ce)
        b['ce ld_out = ld > N ' + d] = any(c[3] == c[2] > c[1] for c in ce)
        b['ce ld_out > ld ' + d] = any(c[3] > c[2] for c in ce)
        b['ce ld_out %% 4 ' + d] = any(c[3] % 4 for c in ce)
        b['ce M = 1 ' + d] = any(c[4] == 1 for c in ce)
        b['ce labels outside the row ' + d] = any(c[0] == dto for c in CE_LABEL_TABLE)
        b['ce-rows kernel route ' + d] = {4, 60, 64, 1028} <= {c[1] for c in CER_TABLE if c[0] == dto and cer_is_kernel(c[1])}
        b['ce-rows torch route ' + d] = any(c[0] == dto and not cer_is_kernel(c[1]) for c in CER_TABLE)
        b['decoder padded vocabulary ' + d] = any(c[0] == dto and c[3] % 64 for c in DEC_TABLE)
        sap = [c for c in SAP_TABLE if c[0] == dto]
        for pos, axis, name in ((3, MASKS, 'mask'), (4, LMASKS, 'lmask'), (5, (0, 1), 'add_stop'), (6, MATS, 'M'), (7, FWLS, 'fwl'), (8, FOUTS, 'outputs'),
                                (9, UPS, 'upstream')):
            for v in axis:
                b['sap %s %s %s' % (name, v, d)] = any(c[pos] == v for c in sap)
        for dims in SAP_DIMS:
            b['sap G=%d W=%d %s' % (dims + (d,))] = any(c[1:3] == dims for c in sap)
        for trip in itertools.product(MASKS, LMASKS, (0, 1)):
            b['sap triple %s %s %d %s' % (trip + (d,))] = any(c[3:6] == trip for c in sap)
        for cls in ('one trip', 'exactly 64', '65', 'more than 128'):
            b['sap G %s %s' % (cls, d)] = any(_lane_class(c[1]) == cls for c in sap)
        for cls in ('one trip', 'exactly 64', '65', 'more than 128'):
            b['sap W %s %s' % (cls, d)] = any(_lane_class(c[2]) == cls for c in sap)
        # both sides of each NULL test of sap_fwd_kernel / sap_bwd_kernel
        null = dict(gvis=lambda c: c[3] == 'none', gvalid=lambda c: c[3] in ('none', 'vis+lens'), glens=lambda c: c[3] in ('none', 'vis+valid'),
                    lmask=lambda c: c[4] == 'null', M=lambda c: c[6] == 'null', fwl=lambda c: c[7] == 'null', loss=lambda c: c[8] != 'loss+lse',
                    lse=lambda c: c[8] == 'neither', ga=lambda c: c[8] == 'neither', dloss=lambda c: c[9] == UPS[1], dgl=lambda c: c[9] in (UPS[0], UPS[3]),
                    dll=lambda c: c[9] in (UPS[0], UPS[3]), dfused=lambda c: c[9] == UPS[0])
        for name, is_null in null.items():
            b['sap %s NULL %s' % (name, d)] = any(is_null(c) for c in sap)
            b['sap %s given %s' % (name, d)] = any(not is_null(c) for c in sap)
        b['sap fw_sigmoid = 0 ' + d] = any(c[7] == 'raw' for c in sap)
        b['sap lmask_is_valid ' + d] = any(c[4] == 'valid' for c in sap)
        b['sap add_stop with a masked local slot 0 ' + d] = any(c[5] == 1 and c[4] != 'null' and c[2] > 1 for c in sap)
        b['sap M with add_stop ' + d] = any(c[5] == 1 and c[6] != 'null' for c in sap)
        b['sap gvalid together with glens ' + d] = any(c[3] == 'all' for c in sap)
        b['sap dloss together with dgl dll dfused ' + d] = any(c[9] == 'all' for c in sap)
        b['sap loss NULL with lse ' + d] = any(c[8] == 'lse' and c[9] != UPS[1] for c in sap)
        b['sap LDS limit ' + d] = any(c[0] == dto and (2 * c[1] + 2 * c[2]) * 4 == 64 * 1024 and c[6] == 'null' for c in SAP_LDS_TABLE)
        b['sap labels outside the range ' + d] = any(c[0] == dto for c in SAP_LABEL_TABLE)
        b['sap table size ' + d] = len(sap) <= 80
    return b


def test_tables_reach_every_dispatch_branch():
    missing = [k for k, v in branches().items() if not v]
    assert not missing, missing


if __name__ == '__main__':
    if sys.argv[1:] == ['--check-inputs']:
        print('%d cases: the reference and sensitivity conditions hold' % check_all_inputs(verbose=True))
        missing = [k for k, v in branches().items() if not v]
        print('branches not reached: %s' % (missing or 'none'))
        sys.exit(1 if missing else 0)
    sys.exit('usage: python tests/test_loss_heads_gpu.py --check-inputs')
