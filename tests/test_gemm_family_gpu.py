"""The GEMM family (csrc/gemm2.hip, gemm3.hip, gemm5.hip, gemm2_tile.hpp, gemm5_tile.hpp, gemm_epilogue.hpp, gemm.hip) against float64
references on the CPU, element by element: goat_gemm_bf16 on every (tile, ring depth, main loop) and operand layout, goat_wgrad_grouped,
goat_wgrad_grouped_balanced and goat_gemm_nt.

Operands: drawn on the CPU from a seeded generator; rows of A [M, Kc] and of B [N, Kc] are scaled by random powers of two in [2^-6, 2^6]
(exact in bf16), so that a row of small magnitude has to be right on its own account.  Every operand (and bias, and saved pre-activation
that a kernel reads) is a view into a NaN-filled buffer with ld = roundup(extent, 8) + 8, starting 16 bytes into its row, with one whole
guard row behind the last row: the kernels' buffer descriptors cover rows x ld elements from the base pointer, and whatever they are
entitled to read lies inside the allocation.  A transposed A [Kc, ld] therefore always has M < ld: NaN columns are in the fetched tile.

Outputs (C, saved pre-activation, dW, dbias, colsum): views into a buffer of 7.0 with 16 guard elements in front and behind, two guard
rows above and below and ld > N (ld a multiple of 8 for the first problem size of a tile, odd for the second: 16-byte stores with an
element-wise tail, and element-wise stores throughout).  An output the kernel must write completely starts as NaN; one it adds into
starts from a random base of magnitude about 1 (colsum / dbias: once from zero, once from a base).  Afterwards every position outside
the view equals 7.0 bitwise and every position inside is finite.

References: float64 on the CPU from the operands as the kernel receives them; the saved pre-activation of the x act' epilogues is a bf16
tensor made here (with 0.0, -0.0, values inside (-4, 4) and beyond +-4).  Nothing a kernel wrote enters a reference.

Bounds, element-wise and derived (S = sum_k |a_k||b_k| in float64, u = 2^-23, q = one rounding of the stored type: 2^-8 bf16, u float32):
    float32 results (plain, + bias, EPI_ACCUM / split-K onto a base)   F  = (Kc + 8) u (S + |bias| + |base|)
    colsum / dbias                                                     (Kc + 8) u (sum_k |a_k| + |base|)
    bf16 result or saved pre-activation                                Bq = F + q (|ref| + F)
    activation output act(u)                                           L Bq + fit(|u| + Bq) + q (|act(u)| + L Bq + fit)
    x act'                                                             |act'(aux)| F + (|acc| + F) dfit(aux) + q |ref| + u |ref|
F is any-order float32 summation with either rounding mode, at a factor of two.  ReLU: L = 1, no fit; GELU: L = 1.13 and the fit bounds
of tests/test_gelu_fit.py (gelu_fast / dgelu_fast for goat_gemm_bf16, gelu_f / dgelu_f for goat_gemm_nt).  x ReLU' is compared for
equality with 0 where aux <= 0.  Conditions on the references (check_inputs: device-free, run over the whole table by
tests/test_gemm_family_refs.py and by `python tests/test_gemm_family_gpu.py --check-inputs`): every reference finite and no S zero; the
same products in float32 torch on the CPU inside a quarter of F at every element; no generated aux strictly between 0 and the smallest
bf16 normal.

Refusals are an explicit table (REFUSED_LAYOUT, REFUSED_RUN, GROUPED_REFUSED): a refused combination returns GOAT_E_ARG and writes nothing,
an accepted one must not raise — an instantiation that vanished from a build fails the test.

The persistent loop (nstage | 0x400) walks at most one tile per workgroup on these shapes; its many-tile behaviour stays with
test_hip_ops.test_gemm_bf16_persistent_matches_one_workgroup_per_tile (bit equality with the ping-pong loop).

Every figure is printed (`FIG family config case output worst error / bound`) before it is asserted; all misses of a case are collected.

Figures of one MI355X run (worst error / bound): float32 results 0.056 (goat_gemm_bf16, Kc = 1, and the grouped launch), 0.12 (goat_gemm_nt
float32, K = 4), 0.003 (balanced launch); x GELU' in float32 0.14.  bf16 results, saved pre-activations and activation outputs reach 0.99
and must be expected to: round-to-nearest moves a value just above a power of two by 2^-9 * 2^e = 2^-8 |v| (1 - O(2^-8)) when it sits
half-way between two bf16 values, which is the whole q (|ref| + F) term — the margin of a bf16 output is F, not a factor.

Defect this module found (fixed in csrc/gemm2.hip and csrc/gemm.hip): split_k > 1 on a contraction of one K-tile (Kc <= 64; goat_gemm_nt
K <= 64 bf16 / 32 float32) was clamped to an unsplit launch that OVERWROTE C instead of adding into it (cases K64 / K1 split2, split3
of test_gemm_bf16, K4 / K8 / K40 of test_gemm_nt)."""
import ctypes
import functools
import re
import sys

import pytest
import torch

from test_gelu_fit import dgelu64, dgelu_f_err, dgelu_fit_err, gelu64, gelu_f_err, gelu_fit_err

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PAD, GUARD_ROWS, SENT, NAN = 16, 2, 7.0, float('nan')
U, UB = 2.0 ** -23, 2.0 ** -8
L_GELU = 1.13                   # max |gelu'| = 1.129
GOAT_E_ARG, GOAT_E_SHAPE = -1, -2
EPI_NONE, EPI_GELU, EPI_RELU, EPI_MUL_DGELU, EPI_MUL_DRELU, EPI_ACCUM = 0, 1, 2, 3, 4, 5
BK = 64


def T(rows, cols=128):
    return rows if cols == 128 else rows | cols << 16


def tile_dims(bm):
    return bm & 0xFFFF, (bm >> 16) or 128


def loop_of(ns):
    return 'persistent' if ns & 0x400 else 'ping-pong' if ns & 0x200 else 'lockstep8' if ns & 0x100 else 'lockstep'


def cfg_name(bm, ns):
    return '%dx%d/%d/%s' % (tile_dims(bm) + (ns & 0xFF, loop_of(ns)))


def _dn(dt):
    return 'bf16' if dt == BF16 else 'f32'


def _q(dt):
    return UB if dt == BF16 else U


def _up8(n):
    return (n + 7) // 8 * 8


@pytest.fixture(scope='module')
def ops():
    from vln_goat_amd import hipops
    return hipops


# ================================================================================================ operands and float64 references
def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _scaled(g, rows, cols, dt):
    """rows of a random matrix times random powers of two in [2^-6, 2^6]: exact in `dt`"""
    x = torch.randn(rows, cols, generator=g).to(dt)
    e = torch.randint(-6, 7, (rows, 1), generator=g).float()
    y = (x.float() * torch.pow(2.0, e)).to(dt)
    assert torch.equal(y.float(), x.float() * torch.pow(2.0, e))
    return y


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, Kc, dt=BF16):
    """operands (logical, K-contiguous: A [M, Kc], B [N, Kc]), bias, bases, a saved pre-activation, and every float64 reference of
    C = A . B^T; built once per size and shared by layouts and configurations, never modified"""
    g = _gen(M, N, Kc, dt == BF16)
    A, B = _scaled(g, M, Kc, dt), _scaled(g, N, Kc, dt)
    aux = (torch.randn(M, N, generator=g) * 3.0).to(dt)
    plant = torch.tensor([0.0, -0.0, 5.0, -7.5, 100.0, -300.0, 0.5, -3.96875, 4.0, -4.0], dtype=dt)
    aux.view(-1)[:min(plant.numel(), aux.numel())] = plant[:aux.numel()]
    c = dict(M=M, N=N, Kc=Kc, dt=dt, A=A, B=B, aux=aux, bias=torch.randn(N, generator=g), base=torch.randn(M, N, generator=g),
             cbase=torch.randn(M, generator=g))
    a, b = A.double(), B.double()
    c['ref'], c['S'] = a @ b.T, a.abs() @ b.abs().T
    c['asum'], c['aabs'] = a.sum(1), a.abs().sum(1)
    return c


def F_of(c, extra=0.0):
    return (c['Kc'] + 8) * U * (c['S'] + extra)


def Bq_of(F, ref, q):
    return F + q * (ref.abs() + F)


def colsum_bound(c, base=0.0):
    return (c['Kc'] + 8) * U * (c['aabs'] + base)


def act64(kind, u):
    return gelu64(u) if kind == 'gelu' else u.clamp_min(0.0)


def dact64(kind, a):
    return dgelu64(a) if kind == 'gelu' else (a > 0).double()


def act_bound(kind, u, Bq, q, fit):
    L, fe = (L_GELU, fit(u.abs() + Bq)) if kind == 'gelu' else (1.0, 0.0)
    return L * Bq + fe + q * (act64(kind, u).abs() + L * Bq + fe)


def dact_bound(kind, c, q, dfit):
    a, F = c['aux'].double(), F_of(c)
    ref = c['ref'] * dact64(kind, a)
    fe = dfit(a) if kind == 'gelu' else 0.0
    return ref, dact64(kind, a).abs() * F + (c['ref'].abs() + F) * fe + q * ref.abs() + U * ref.abs()


def check_inputs(c, what):
    """conditions a. b. c. of the module docstring on one case -> worst float32-CPU error / F"""
    for k in ('ref', 'S', 'asum', 'aabs'):
        assert bool(torch.isfinite(c[k]).all()), '%s: %s not finite' % (what, k)
    assert bool((c['S'] > 0).all()) and bool((c['aabs'] > 0).all()), '%s: a zero S' % what
    a32, b32 = c['A'].float(), c['B'].float()
    worst = 0.0
    for got, ref, bound in ((a32 @ b32.T, c['ref'], F_of(c)), (a32 @ b32.T + c['bias'], c['ref'] + c['bias'].double(), F_of(c, c['bias'].double().abs())),
                            (a32.sum(1), c['asum'], colsum_bound(c))):
        worst = max(worst, float(((got.double() - ref).abs() / bound).max()))
    assert worst <= 0.25, '%s: float32 on the CPU is %.3f of F off the float64 reference' % (what, worst)
    a = c['aux'].float()
    assert not bool(((a > 0) & (a < 2.0 ** -126)).any()), '%s: an aux value between 0 and the smallest bf16 normal' % what
    assert bool((a == 0).any()) and bool((a.abs() > 4).any()) or a.numel() < 8, '%s: aux lacks a zero or a value beyond the clamp' % what
    return worst


# ================================================================================================ memory around a launch
def place_in(t):
    """CPU tensor [rows, ext] or [n] -> device view into a NaN-filled buffer: ld = roundup(ext, 8) + 8, the view 16 bytes into its row,
    one guard row behind the last"""
    if t.dim() == 1:
        return place_in(t.view(1, -1))[0]
    rows, ext = t.shape
    off = 16 // t.element_size()
    buf = torch.full((rows + 1, _up8(ext) + 8), NAN, dtype=t.dtype, device=DEV)
    v = buf[:rows, off:off + ext]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and v.stride(0) % 8 == 0
    return v


def operands(c, ta, tb):
    return place_in(c['A'].T.contiguous() if ta else c['A']), place_in(c['B'].T.contiguous() if tb else c['B'])


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


class Out:
    """one output inside its sentinel bands; init: CPU tensor the kernel adds onto, None: NaN (the kernel must write every element)"""

    def __init__(self, rows, cols, dtype, ld, init=None):
        assert ld > cols
        self.shape, self.ld, self.off = (rows, cols), ld, PAD + GUARD_ROWS * ld
        self.buf = torch.full((2 * PAD + (rows + 2 * GUARD_ROWS) * ld,), SENT, dtype=dtype, device=DEV)
        self.v = self.buf.as_strided((rows, cols), (ld, 1), self.off)
        self.v.copy_(init.view(rows, cols) if init is not None else torch.full((rows, cols), NAN))
        self.before = self.buf.clone()

    def vec(self):
        return self.v[0]

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(self.before))

    def collect(self, label, miss):
        """-> the view on the CPU; the bands must read 7.0 bitwise"""
        b = self.buf.cpu()
        got = b.as_strided(self.shape, (self.ld, 1), self.off).clone()
        b.as_strided(self.shape, (self.ld, 1), self.off).fill_(SENT)
        if not torch.equal(_bits(b), _bits(torch.full_like(b, SENT))):
            miss.append('%s: %d guard elements were written' % (label, int((b != SENT).sum())))
        return got


def out_ld(cols, odd):
    return _up8(cols) + 8 + (1 if odd else 0)


def compare(label, got, ref, bound, miss, zero=None):
    """got against the float64 reference, element by element in units of the bound; zero: positions that must be exactly 0"""
    if not bool(torch.isfinite(got).all()):
        print('FIG %s nan' % label)
        miss.append('%s: %d values not finite' % (label, int((~torch.isfinite(got)).sum())))
        return
    ratio = (got.double().reshape(ref.shape) - ref).abs() / bound
    if zero is not None:
        ratio = torch.where(zero, torch.zeros_like(ratio), ratio)          # (the bound is 0 there: compared for equality instead)
        bad = (got.reshape(ref.shape) != 0) & zero
        if bool(bad.any()):
            miss.append('%s: %d positions that must be exactly 0 are not, first %s' % (label, int(bad.sum()), bad.nonzero()[0].tolist()))
    worst = float(ratio.max())
    print('FIG %s %.3e' % (label, worst))
    if not worst <= 1.0:
        miss.append('%s: error / bound %.3e at %s (%d elements over)' % (label, worst, (ratio == ratio.max()).nonzero()[0].tolist(), int((ratio > 1).sum())))


def status_of(fn, *args):
    """the status a hipops launch helper raised with, 0 when it did not raise"""
    try:
        fn(*args)
    except RuntimeError as ex:
        m = re.search(r'status (-?\d+)', str(ex))
        assert m, ex
        return int(m.group(1))
    return 0


# ================================================================================================ a. goat_gemm_bf16, every configuration
PP_TILES = (T(128), T(256), T(128, 256), T(192, 256), T(256, 256))
CONFIGS = ([(64, 2), (64, 3), (64, 4), (128, 2), (128, 3), (128, 4), (256, 2), (256, 3), (128, 0x102), (128, 0x103), (128, 0x104),
            (96, 2), (96, 3), (96, 4), (T(128, 256), 2), (T(128, 256), 3), (T(192, 256), 2), (T(256, 192), 2), (T(256, 256), 2),
            (T(192, 192), 2), (T(192, 192), 3)] + [(t, 0x202) for t in PP_TILES]          # the 26 of test_gemm_bf16_every_tile_configuration
           + [(t, 0x602) for t in PP_TILES])                                                # ... and the persistent loop
LAYOUTS = ((0, 0), (0, 1), (1, 1))
# (tile, nstage, trans_a, trans_b) goat_gemm_bf16 refuses with GOAT_E_ARG: a transposed side needs a power-of-two tile width, the 96- and
# 192-row tiles take K-contiguous A only, the persistent loop takes K-contiguous A
REFUSED_LAYOUT = frozenset(
    [(T(256, 192), 2, 0, 1), (T(192, 192), 2, 0, 1), (T(192, 192), 3, 0, 1),
     (T(256, 192), 2, 1, 1), (T(192, 192), 2, 1, 1), (T(192, 192), 3, 1, 1),
     (96, 2, 1, 1), (96, 3, 1, 1), (96, 4, 1, 1), (T(192, 256), 2, 1, 1), (T(192, 256), 0x202, 1, 1)]
    + [(t, 0x602, 1, 1) for t in PP_TILES])
RUNS = ('bf16', 'f32', 'accum', 'split2', 'split3', 'gelu', 'relu', 'dgelu', 'drelu')
# (what, run) refused with GOAT_E_ARG on an accepted (configuration, layout): the persistent loop has bf16 results, unsplit; the weight-
# gradient layout (transposed A) has no activation epilogues
REFUSED_RUN = frozenset([('persistent', r) for r in ('f32', 'accum', 'split2', 'split3')] + [('trans_a', r) for r in ('gelu', 'relu', 'dgelu', 'drelu')])


def expected_status(bm, ns, ta, tb, run):
    if (bm, ns, ta, tb) in REFUSED_LAYOUT:
        return GOAT_E_ARG
    if (loop_of(ns), run) in REFUSED_RUN or (ta and ('trans_a', run) in REFUSED_RUN):
        return GOAT_E_ARG
    return 0


def tile_sizes(bm):
    """(M, N, odd ld): one tile with three dead rows and five dead columns; four tiles, three of them with one valid row and / or column"""
    rows, cols = tile_dims(bm)
    return ((rows - 3, cols - 5, False), (rows + 1, cols + 1, True))


def contractions(ta, tb):
    """K-contiguous operands need whole K-tiles: one (fewer than any ring depth, fewer than the two phases of the ping-pong loop) and
    three; both transposed: any length"""
    return (1, 72, 200) if ta and tb else (64, 192)


GEMM_TABLE = [(bm, ns, ta, tb) for bm, ns in CONFIGS for ta, tb in LAYOUTS]


def _gemm_id(p):
    return '%s-t%d%d' % (cfg_name(p[0], p[1]), p[2], p[3])


def launch_gemm(ops, c, a, b, ta, tb, bm, ns, run, odd, colsum=None):
    """one launch of `run` -> (status, {name: Out}, aux input or None)"""
    M, N, Kc = c['M'], c['N'], c['Kc']
    ld = out_ld(N, odd)
    adds = run == 'accum' or run.startswith('split')
    odt = F32 if run == 'f32' or adds else BF16
    outs = dict(C=Out(M, N, odt, ld, c['base'] if adds else None))
    bias = place_in(c['bias']) if run in ('bf16', 'f32', 'gelu', 'relu') else None
    epi = dict(accum=EPI_ACCUM, gelu=EPI_GELU, relu=EPI_RELU, dgelu=EPI_MUL_DGELU, drelu=EPI_MUL_DRELU).get(run, EPI_NONE)
    aux = None
    if run in ('gelu', 'relu'):
        outs['aux'] = Out(M, N, BF16, ld)
        aux = outs['aux'].v
    elif run in ('dgelu', 'drelu'):
        aux = place_in(c['aux'])
    if colsum is not None:
        outs['colsum'] = Out(1, M, F32, M + 8, c['cbase'] if colsum == 'base' else torch.zeros(M))
    split = int(run[5:]) if run.startswith('split') else 1
    st = status_of(ops._launch_gemm_bf16, a, b, outs['C'].v, bool(ta), bool(tb), M, N, Kc, bias, epi, aux, split, bm, ns,
                   outs['colsum'].vec() if colsum is not None else None)
    torch.cuda.synchronize()
    return st, outs


def expectations(c, run, odt_in=BF16, fits=(gelu_fit_err, dgelu_fit_err)):
    """{output: (reference, bound, positions that must be exactly zero or None)} of one run"""
    bias = c['bias'].double()
    if run in ('bf16', 'f32', 'gelu', 'relu'):
        u, Fb = c['ref'] + bias, F_of(c, bias.abs())
        if run == 'f32':
            return dict(C=(u, Fb, None))
        q = _q(odt_in)
        Bq = Bq_of(Fb, u, q)
        if run == 'bf16':
            return dict(C=(u, Bq, None))
        return dict(aux=(u, Bq, None), C=(act64(run, u), act_bound(run, u, Bq, q, fits[0]), None))
    if run in ('dgelu', 'drelu'):
        kind = run[1:]
        ref, bound = dact_bound(kind, c, _q(odt_in), fits[1])
        return dict(C=(ref, bound, (c['aux'].float() <= 0) if kind == 'relu' else None))
    base = c['base'].double()
    return dict(C=(c['ref'] + base, F_of(c, base.abs()), None))


def check_run(label, c, run, outs, miss, colsum=None, **kw):
    for name, (ref, bound, zero) in expectations(c, run, **kw).items():
        compare('%s %s:%s' % (label, run, name), outs[name].collect('%s %s:%s' % (label, run, name), miss), ref, bound, miss, zero)
    if colsum is not None:
        base = c['cbase'].double() if colsum == 'base' else 0.0
        lab = '%s %s:colsum@%s' % (label, run, colsum)
        compare(lab, outs['colsum'].collect(lab, miss), (c['asum'] + base).view(1, -1), colsum_bound(c, abs(base)).view(1, -1), miss)


@pytest.mark.parametrize('p', GEMM_TABLE, ids=_gemm_id)
def test_gemm_bf16(ops, p):
    bm, ns, ta, tb = p
    miss = []
    for M, N, odd in tile_sizes(bm):
        for Kc in contractions(ta, tb):
            c = gemm_case(M, N, Kc)
            label = 'gemm_bf16 %s t%d%d-M%d-N%d-K%d' % (cfg_name(bm, ns), ta, tb, M, N, Kc)
            a, b = operands(c, ta, tb)
            for run in RUNS:
                want = expected_status(bm, ns, ta, tb, run)
                colsum = {'f32': 'zero', 'accum': 'base'}.get(run) if ta and want == 0 else None
                st, outs = launch_gemm(ops, c, a, b, ta, tb, bm, ns, run, odd, colsum)
                if st != want:
                    miss.append('%s %s: status %d, the table says %d' % (label, run, st, want))
                elif want:
                    miss += ['%s %s: refused, yet %s was written' % (label, run, k) for k, o in outs.items() if not o.untouched()]
                else:
                    check_run(label, c, run, outs, miss, colsum)
            if (bm, ns, ta, tb) in REFUSED_LAYOUT:
                break                       # (one contraction is enough to see a refusal)
    assert not miss, miss


LOOPS = ((128, 2), (128, 0x102), (T(128, 256), 2), (128, 0x202))       # lockstep 4-wave, lockstep 8-wave, wide 8-wave, ping-pong


@pytest.mark.parametrize('cfg', LOOPS, ids=lambda c: cfg_name(*c))
@pytest.mark.parametrize('ta,tb', [(0, 0), (1, 1)])
def test_gemm_bf16_empty_trailing_split_and_clamp(ops, cfg, ta, tb):
    """Kc = 320 is five K-tiles: split_k = 4 gives two per split and a fourth split with nothing to do (the kernels return early there);
    split_k = 9 is clamped to five"""
    bm, ns = cfg
    M, N, odd = tile_sizes(bm)[1]
    c, miss = gemm_case(M, N, 320), []
    a, b = operands(c, ta, tb)
    for split in (4, 9):
        label = 'gemm_bf16 %s t%d%d-M%d-N%d-K320' % (cfg_name(bm, ns), ta, tb, M, N)
        st, outs = launch_gemm(ops, c, a, b, ta, tb, bm, ns, 'split%d' % split, odd)
        assert st == 0, (label, split, st)
        check_run(label, c, 'split%d' % split, outs, miss)
    assert not miss, miss


# ================================================================================================ b. c. the grouped weight gradients
GROUPED_CONFIGS = ((64, 3), (128, 2), (128, 0x102), (128, 0x103), (256, 2), (T(128, 256), 3), (T(256, 256), 2), (256, 0x202), (T(128, 256), 0x202),
                   (T(256, 256), 0x202))            # as test_hip_ops.test_wgrad_grouped
# (tile, nstage) goat_wgrad_grouped refuses with GOAT_E_ARG: tiles that are no power of two on either side, the 128 x 128 ping-pong tile,
# ring depths the tile has no room for, the persistent flag
GROUPED_REFUSED = ((96, 2), (T(192, 256), 2), (T(256, 192), 2), (T(192, 192), 2), (128, 0x202), (T(192, 256), 0x202), (256, 4), (T(256, 256), 3),
                   (128, 0x302), (64, 5))
BALANCED_TILES = (T(256, 256), T(128, 256), T(256))
GROUPED_TABLE = [(bm, ns, n) for bm, ns in GROUPED_CONFIGS for n in (1, 5)] + [(128, 2, 48)]
ROWS = (1, 63, 64, 65, 200)


def group_problems(bm, n):
    """rows in ROWS; n_out, n_in one below or one above a tile edge, or 8; accumulate and dbias mixed within the launch"""
    rt, ct = tile_dims(bm)
    if n == 1:
        return [dict(rows=65, n_out=rt + 1, n_in=ct - 1, acc=0, db=1)]
    return [dict(rows=ROWS[i % 5], n_out=(rt - 1, rt + 1, 8)[(i + i // 5) % 3], n_in=(ct + 1, 8, ct - 1)[(i + i // 3) % 3], acc=(i + i // 5) % 2, db=int(i % 3 != 1))
            for i in range(n)]


def balanced_problems(bm, target):
    """three problems (four tiles, two tiles, one tile) whose K-tile iterations, tiles x ceil(rows / 64), sum to `target`"""
    rt, ct = tile_dims(bm)
    k1 = max(1, target // 8)
    rem = target - 4 * k1
    k2 = max(1, (rem - 1) // 2)
    k3 = rem - 2 * k2
    assert k3 >= 1
    return [dict(rows=64 * k1 - 1, n_out=rt + 1, n_in=ct + 1, acc=0, db=1), dict(rows=64 * (k2 - 1) + 1, n_out=rt + 1, n_in=ct - 5, acc=1, db=0),
            dict(rows=64 * k3, n_out=8, n_in=8, acc=1, db=1)]


def iterations(bm, probs):
    rt, ct = tile_dims(bm)
    return sum(((q['n_out'] + rt - 1) // rt) * ((q['n_in'] + ct - 1) // ct) * ((q['rows'] + BK - 1) // BK) for q in probs)


def _case_of(q):
    return gemm_case(q['n_out'], q['n_in'], q['rows'])


class Group:
    """the argument array of a grouped launch: dY [rows, n_out] and X [rows, n_in] row-strided in NaN-filled buffers, dW with ld = n_in + 8"""

    def __init__(self, probs, db_from):
        from vln_goat_amd import _lib
        self.probs, self.db_from = probs, db_from
        self.arr = (_lib.WgradProblem * len(probs))()
        self.keep, self.outs = [], []
        for i, q in enumerate(probs):
            c = _case_of(q)
            dy, x = operands(c, 1, 1)
            dw = Out(q['n_out'], q['n_in'], F32, q['n_in'] + 8, c['base'] if q['acc'] else None)
            db = Out(1, q['n_out'], F32, q['n_out'] + 8, c['cbase'] if db_from == 'base' else torch.zeros(q['n_out'])) if q['db'] else None
            r = self.arr[i]
            r.dy, r.ld_dy, r.x, r.ld_x, r.dw, r.ld_dw = dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.v.data_ptr(), dw.ld
            r.dbias = db.vec().data_ptr() if db is not None else None
            r.rows, r.n_out, r.n_in, r.accumulate = q['rows'], q['n_out'], q['n_in'], q['acc']
            self.keep.append((dy, x))
            self.outs.append((dw, db))

    def addr(self):
        return ctypes.addressof(self.arr)

    def untouched(self):
        return all(dw.untouched() and (db is None or db.untouched()) for dw, db in self.outs)

    def check(self, label, miss):
        """-> the collected results (for bit comparison between launches)"""
        got = []
        for i, (q, (dw, db)) in enumerate(zip(self.probs, self.outs)):
            c = _case_of(q)
            lab = '%s p%d-r%d-o%d-i%d-acc%d' % (label, i, q['rows'], q['n_out'], q['n_in'], q['acc'])
            base = c['base'].double() if q['acc'] else 0.0
            got.append(dw.collect(lab + ' dW', miss))
            compare(lab + ' dW', got[-1], c['ref'] + base, F_of(c, abs(base)), miss)
            if db is not None:
                base = c['cbase'].double() if self.db_from == 'base' else 0.0
                got.append(db.collect(lab + ' dbias', miss))
                compare('%s dbias@%s' % (lab, self.db_from), got[-1], (c['asum'] + base).view(1, -1), colsum_bound(c, abs(base)).view(1, -1), miss)
        return got


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('p', GROUPED_TABLE, ids=lambda p: '%s-n%d' % (cfg_name(p[0], p[1]), p[2]))
def test_wgrad_grouped(ops, p):
    from vln_goat_amd import _lib
    bm, ns, n = p
    miss = []
    for db_from in ('zero', 'base'):
        g = Group(group_problems(bm, n), db_from)
        st = _lib.lib().goat_wgrad_grouped(_stream(), g.addr(), n, bm, ns)
        torch.cuda.synchronize()
        assert st == 0, st
        g.check('wgrad_grouped %s n%d' % (cfg_name(bm, ns), n), miss)
    assert not miss, miss


def test_wgrad_grouped_refusals(ops):
    from vln_goat_amd import _lib
    g = Group(group_problems(128, 5), 'base')
    for bm, ns in GROUPED_REFUSED:
        assert _lib.lib().goat_wgrad_grouped(_stream(), g.addr(), 5, bm, ns) == GOAT_E_ARG, (hex(bm), hex(ns))
    torch.cuda.synchronize()
    assert g.untouched()


@pytest.mark.parametrize('bm', BALANCED_TILES, ids=lambda bm: '%dx%d' % tile_dims(bm))
def test_wgrad_grouped_balanced(ops, bm):
    """The smallest group the entry accepts: one K-tile iteration more than the device has compute units (pp_launch_group_sk refuses fewer
    iterations than workgroups), so a share is one or two K-tiles and nearly every tile is cut and summed through the workspace.  The
    flag words are zero afterwards, a second launch reproduces the first bit for bit, and one iteration fewer than the CU count is
    refused with GOAT_E_SHAPE, nothing written."""
    from vln_goat_amd import _lib
    L = _lib.lib()
    G = torch.cuda.get_device_properties(0).multi_processor_count
    probs = balanced_problems(bm, G + 1)
    assert iterations(bm, probs) == G + 1
    nb = L.goat_wgrad_balanced_ws_bytes(bm)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    miss, first = [], None
    for db_from in ('zero', 'base', 'base'):
        g = Group(probs, db_from)
        st = L.goat_wgrad_grouped_balanced(_stream(), g.addr(), len(probs), bm, ws.data_ptr(), nb)
        torch.cuda.synchronize()
        assert st == 0, st
        got = g.check('wgrad_balanced %dx%d G%d' % (tile_dims(bm) + (G,)), miss)
        if int(ws[-G * 32:].view(torch.int32).abs().sum()) != 0:
            miss.append('flag words not zero after the launch')
        if db_from == 'base':
            if first is not None and not all(torch.equal(_bits(x), _bits(y)) for x, y in zip(first, got)):
                miss.append('the second launch does not reproduce the first bit for bit')
            first = got
    few = balanced_problems(bm, G - 1)
    assert iterations(bm, few) == G - 1
    g = Group(few, 'base')
    st = L.goat_wgrad_grouped_balanced(_stream(), g.addr(), len(few), bm, ws.data_ptr(), nb)
    torch.cuda.synchronize()
    if st != GOAT_E_SHAPE or not g.untouched():
        miss.append('one iteration fewer than the CU count: status %d (GOAT_E_SHAPE expected), outputs untouched: %s' % (st, g.untouched()))
    assert not miss, miss


# ================================================================================================ d. goat_gemm_nt
NT_SPLITS = (2, 3, 4, 5)
NT_TABLE = ([(F32, M, N, K) for M, N in ((125, 129), (129, 125)) for K in (4, 36, 100)]
            + [(BF16, M, N, K) for M, N in ((125, 129), (129, 125)) for K in (8, 40, 104)] + [(BF16, 129, 125, 296)])


def nt_k_tiles(dt, K):
    bk = 64 if dt == BF16 else 32
    return (K + bk - 1) // bk


def nt_has_empty_trailing_split(dt, K, split):
    kt = nt_k_tiles(dt, K)
    split = max(min(split, kt), 2)
    per = (kt + split - 1) // split
    return per * (split - 1) >= kt


@pytest.mark.parametrize('p', NT_TABLE, ids=lambda p: '%s-M%d-N%d-K%d' % ((_dn(p[0]),) + p[1:]))
def test_gemm_nt(ops, p):
    """the 128 x 128 tile of the round-1 kernel (float32 parity path, bf16 contractions that are no multiple of 64): plain + bias, bf16 in
    with float32 out, GELU / ReLU with saved pre-activation, x GELU' / x ReLU', split-K onto a base (split_k beyond the K-tiles, and
    K-tile counts that leave the last split empty: float32 K = 100 with 3, bf16 K = 296 with 4)"""
    dt, M, N, K = p
    c, miss = gemm_case(M, N, K, dt), []
    label = 'gemm_nt %s M%d-N%d-K%d' % (_dn(dt), M, N, K)
    a, b = operands(c, 0, 0)
    fits = (gelu_f_err, dgelu_f_err)
    plan = [('bf16', dt), ('gelu', dt), ('relu', dt), ('dgelu', dt), ('drelu', dt)] + [('split%d' % s, F32) for s in NT_SPLITS]
    if dt == BF16:
        plan.append(('f32', F32))
    for run, odt in plan:
        ld = out_ld(N, odd=(M > N))
        outs = dict(C=Out(M, N, odt, ld, c['base'] if run.startswith('split') else None))
        bias = place_in(c['bias']) if run in ('bf16', 'f32', 'gelu', 'relu') else None
        epi = dict(bf16=EPI_NONE, f32=EPI_NONE, gelu=EPI_GELU, relu=EPI_RELU, dgelu=EPI_MUL_DGELU, drelu=EPI_MUL_DRELU).get(run, EPI_NONE)
        aux = None
        if run in ('gelu', 'relu'):
            outs['aux'] = Out(M, N, dt, ld)
            aux = outs['aux'].v
        elif run in ('dgelu', 'drelu'):
            aux = place_in(c['aux'])
        st = status_of(ops.gemm_nt, a, b, outs['C'].v, bias, epi, aux, int(run[5:]) if run.startswith('split') else 1)
        torch.cuda.synchronize()
        assert st == 0, (label, run, st)
        # (run 'bf16' is "the input type out": the name of the plain + bias run of expectations())
        check_run(label, c, 'f32' if run == 'bf16' and dt == F32 else run, outs, miss, odt_in=dt, fits=fits)
    assert not miss, miss


# ================================================================================================ the tables, device-free
def case_keys():
    """{family: every (M, N, Kc, dtype) its tests build}; the balanced launch at 256 compute units"""
    k = dict(gemm_bf16=set(), wgrad_grouped=set(), wgrad_balanced=set(), gemm_nt=set())
    for bm, ns, ta, tb in GEMM_TABLE:
        if (bm, ns, ta, tb) not in REFUSED_LAYOUT:
            k['gemm_bf16'] |= {(M, N, Kc, BF16) for M, N, _ in tile_sizes(bm) for Kc in contractions(ta, tb)}
    k['gemm_bf16'] |= {tile_sizes(bm)[1][:2] + (320, BF16) for bm, _ in LOOPS}
    for bm, ns, n in GROUPED_TABLE:
        k['wgrad_grouped'] |= {(q['n_out'], q['n_in'], q['rows'], BF16) for q in group_problems(bm, n)}
    for bm in BALANCED_TILES:
        k['wgrad_balanced'] |= {(q['n_out'], q['n_in'], q['rows'], BF16) for t in (255, 257) for q in balanced_problems(bm, t)}
    k['gemm_nt'] = {(M, N, K, dt) for dt, M, N, K in NT_TABLE}
    return k


def check_all_inputs(verbose=False):
    """conditions a. b. c. over every case of every table -> {family: (cases, worst float32-CPU error / F)}"""
    res = {}
    for fam, keys in case_keys().items():
        worst = 0.0
        for key in sorted(keys, key=lambda t: t[:3] + (t[3] == BF16,)):
            worst = max(worst, check_inputs(gemm_case(*key), '%s %s' % (fam, key[:3])))
        res[fam] = (len(keys), worst)
        print('REF %s: %d cases, worst float32-CPU error / F %.3f' % (fam, len(keys), worst))
    gemm_case.cache_clear()
    return res


def table_properties():
    """what the tables must reach, by name"""
    b = {}
    b['every configuration on every layout'] = len(GEMM_TABLE) == 31 * 3
    b['refused layouts are table entries'] = all(p in GEMM_TABLE for p in REFUSED_LAYOUT)
    b['one K-tile below every ring depth'] = 64 in contractions(0, 0) and 64 in contractions(0, 1)
    b['a contraction of one element'] = 1 in contractions(1, 1)
    b['gemm_nt empty trailing split f32'] = any(nt_has_empty_trailing_split(F32, K, s) and nt_k_tiles(F32, K) > 2 for dt, _, _, K in NT_TABLE if dt == F32 for s in NT_SPLITS)
    b['gemm_nt empty trailing split bf16'] = any(nt_has_empty_trailing_split(BF16, K, s) and nt_k_tiles(BF16, K) > 2 for dt, _, _, K in NT_TABLE if dt == BF16 for s in NT_SPLITS)
    for n in (1, 5, 48):
        b['grouped launch of %d' % n] = any(p[2] == n for p in GROUPED_TABLE)
    pr = group_problems(128, 5)
    b['accumulate mixed'] = {q['acc'] for q in pr} == {0, 1}
    b['dbias mixed'] = {q['db'] for q in pr} == {0, 1}
    b['every row count'] = {q['rows'] for q in pr} == set(ROWS)
    for bm in BALANCED_TILES:
        b['balanced %#x iterations' % bm] = all(iterations(bm, balanced_problems(bm, t)) == t for t in (63, 64, 255, 257, 303, 305))
    return b


if __name__ == '__main__':
    if sys.argv[1:] == ['--check-inputs']:
        res = check_all_inputs(verbose=True)
        missing = [k for k, v in table_properties().items() if not v]
        print('%d cases: the reference conditions hold; table properties not met: %s' % (sum(n for n, _ in res.values()), missing or 'none'))
        sys.exit(1 if missing else 0)
    sys.exit('usage: python tests/test_gemm_family_gpu.py --check-inputs')
