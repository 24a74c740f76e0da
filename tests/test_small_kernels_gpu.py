"""The small non-GEMM kernels of csrc/causal.hip (attention pooling, door gate, dict_wsum, cfp_mix, InfoNCE, rowdot) and of csrc/embed.hip / csrc/linear_aux.hip
(panorama fusion, short-K weight gradient, gather / segment mean, embedding tables, column sums) at every dispatch branch, width and tail,
against float64 references on the CPU.  (The SAP pair of causal.hip and the cross-entropy kernels: tests/test_loss_heads_gpu.py, with these helpers.)

Reference: float64, from the operands as the kernel receives them (a bf16 input upcast from its bf16 value; the Linear(H, 1) weight of rowdot
rounded to the activation dtype first), written from the comment block above each kernel; backward references by float64 autograd on the
CPU.  Nothing a kernel wrote enters a reference.

Bound: test_hip_ops._tol (1e-3 on the float32 path, 2e-2 on the bf16 path) times the largest |reference| of the ROW the element belongs to
('row': the last dimension — an output row of a [rows, H] tensor, a sample of a [B, L] / [B, K] one; 'vec': the whole tensor — 1-D parameter
gradients, scalars, and the 1-D row results loss[Bl], gate[rows], y[M], dfwl[B], which are one number per row).  Two conditions on the
references, asserted on the CPU before anything runs (check_inputs; `python tests/test_small_kernels_gpu.py --check-inputs` and
tests/test_small_kernels_abi.py run them over the whole table without a device):
  a. the reference rounded once to the kernel's output dtype sits inside a quarter of the bound at every element;
  b. no row scale is below 1e-6 of the tensor's largest;
  c. the same formula evaluated in float32 torch on the CPU sits inside a quarter of the row-scaled bound as well.  A row of one element
     (H = 1, K = 1) is a sum that may cancel — s aug + (1 - s) ori of the door gate does in some of 2051 rows — and float32 arithmetic
     alone then misses the bound by the factor a float32 kernel misses it by.  Such inputs are not used: the generator seed of a case
     is moved on until a. b. c. hold (conditioned(); `--check-inputs` prints the seed bump and the float32-CPU figures of every case).
Positions a kernel must not touch, or must write as exact zeros (padding rows of a table, rows no segment names, masked slots, the gradients
of a one-slot softmax), are compared for equality at every position — with the base they started from, or with 0.0 — and take no part in
the row scales.  No output of this module uses the per-tensor fall-back scale or a floored row scale.

Direct calls (launch('goat_...')): every output is a view into a larger buffer with PAD elements of 7.0 in front of and behind it, which must
read 7.0 afterwards; every floating-point input is a view into a NaN-filled buffer of the same layout and every output is checked finite;
an output the kernel must write completely starts as NaN.  Outputs the kernels add into atomically run twice: from zero and from a random
base of magnitude about 1 (`got - base` against the same bound).

Every figure is printed (`FIG family dtype case output[@variant] worst error / row scale`) before it is asserted, every miss reported."""
import ctypes
import functools
import itertools
import math
import sys

import pytest
import torch

from test_hip_ops import _tol

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16, F32 = torch.bfloat16, torch.float32
PAD = 16            # sentinel elements on either side of every direct-call output (a 16-byte chunk is 8 bf16 / 4 float32 elements)
SENT = 7.0
NAN = float('nan')
GOAT_E_ARG = -1


def _dn(dt):
    return 'bf16' if dt == BF16 else 'f32'


def _epc(dt):
    return 8 if dt == BF16 else 4


def _gen(*key):
    """a generator seeded by the case and its seed bump (conditioned() moves the bump on until the reference conditions hold)"""
    s = 0
    for k in key:
        s = (s * 1000003 + (hash(k) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _sd(name):
    """stable integer of a family name (str hashes change between processes)"""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@pytest.fixture(scope='module')
def ops():
    from vln_goat_amd import hipops
    return hipops


# ================================================================================================ references, conditions, comparison
def O(ref, kind, odt, zero=None, special=False):
    """one output: float64 reference, 'row' | 'vec' scale, the dtype the kernel stores it in, bool mask of positions compared for equality.
    special: positions where the reference is -inf, +inf or NaN are part of the contract (a masked logit, the loss of a label on a masked
    slot, a poisoned row): the kernel's value must be the same special value, sign included; they take no part in the scales.  Without
    it a non-finite reference is refused (check_inputs) and a non-finite kernel value is a miss (check), as ever."""
    ref = ref.detach().double()
    spec = None
    if special and not bool(torch.isfinite(ref).all()):
        spec = ref.clone()
        ref = torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref))
    if zero is None and ref.numel() and not bool(ref.any()):
        zero = torch.ones_like(ref, dtype=torch.bool)         # (the gradients behind a one-slot softmax: exact zeros)
    if zero is not None:
        zero = zero.expand_as(ref).clone()
    return dict(ref=ref, kind=kind, odt=odt, zero=zero, spec=spec)


def _nonfinite(o):
    """positions whose reference is a special value (None: none, the default)"""
    return None if o.get('spec') is None else ~torch.isfinite(o['spec'])


def _live(o):
    live = torch.ones_like(o['ref'], dtype=torch.bool) if o['zero'] is None else ~o['zero']
    return live if _nonfinite(o) is None else live & ~_nonfinite(o)


def row_scale(o):
    a = o['ref'].abs() * _live(o)
    if o['kind'] == 'vec' or a.dim() < 2:
        return a.max() if a.numel() else a.sum()
    return a.amax(-1, keepdim=True)


def _same_special(spec, got):
    """got carries spec's special values at spec's non-finite positions, and only there -> bool"""
    if got is None:
        return False
    nf = ~torch.isfinite(spec)
    if not torch.equal(nf, ~torch.isfinite(got.double())):
        return False
    a, b = spec[nf], got.double()[nf]
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def check_inputs(dt, outs, what):
    """conditions a. and b. of the module docstring, on the references alone"""
    tol = _tol(dt)
    for name, o in outs.items():
        ref, live, scale = o['ref'], _live(o), row_scale(o)
        assert bool(torch.isfinite(ref).all()), '%s %s: reference not finite' % (what, name)
        assert bool((ref[~live] == 0).all()), '%s %s: a position compared for equality has a non-zero reference' % (what, name)
        if not bool(live.any()):
            continue
        once = ref.to(o['odt']).double()
        bad = ((once - ref).abs() > 0.25 * tol * scale) & live
        assert not bool(bad.any()), '%s %s: storage rounding alone takes more than a quarter of the bound at %d elements' % (what, name, int(bad.sum()))
        rows = scale[live.any(-1, keepdim=True)] if scale.dim() else scale.reshape(1)
        assert bool((rows >= 1e-6 * scale.max()).all()), '%s %s: a row scale is below 1e-6 of the largest (%.3e of %.3e): another seed' % (
            what, name, float(rows.min()), float(scale.max()))


MAX_BUMP = 64


def conditioned(build):
    """build(*case, bump, rdt) -> the case with references computed in `rdt`.  The case is built in float64 and again, from the same
    operands, in float32; the generator seed is moved on (bump 0, 1, ...) until conditions a. b. c. of the module docstring hold.  All of
    this is CPU work on the references: nothing a kernel computed enters the choice."""
    @functools.lru_cache(maxsize=None)
    def case(*key):
        dt = key[0] if isinstance(key[0], torch.dtype) else F32
        why = None
        for bump in range(MAX_BUMP):
            c = build(*key, bump=bump, rdt=torch.float64)
            try:
                for k in ('outs', 'outs32'):
                    if k in c:
                        check_inputs(dt, c[k], '%s%r bump %d' % (build.__name__, key[1:], bump))
                c['f32_cpu'] = check_conditioning(dt, c['outs'], build(*key, bump=bump, rdt=torch.float32)['outs'], build.__name__)
            except AssertionError as ex:
                why = str(ex)
                continue
            c['bump'] = bump
            return c
        raise AssertionError('no seed among %d meets the reference conditions: %s' % (MAX_BUMP, why))
    case.__name__ = build.__name__
    return case


def check_conditioning(dt, outs, outs_f32, what):
    """condition c.: the same formula evaluated in float32 torch on the CPU sits inside a quarter of the row-scaled bound at every element
    (otherwise a row is ill-conditioned — a one-element row s aug + (1 - s) ori that cancels, say — and the case cannot tell a kernel error
    from float32 arithmetic) -> {output: worst float32-CPU error / row scale}"""
    tol, figs = _tol(dt), {}
    for name, o in outs.items():
        scale, live = row_scale(o), _live(o)
        if _nonfinite(o) is not None or _nonfinite(outs_f32[name]) is not None:
            assert o.get('spec') is not None and _same_special(o['spec'], outs_f32[name].get('spec')), \
                '%s %s: float32 on the CPU has other special values than the float64 reference' % (what, name)
        err = ((outs_f32[name]['ref'] - o['ref']).abs() / scale.clamp_min(1e-300)) * live
        figs[name] = float(err.max()) if err.numel() else 0.0
        assert figs[name] <= 0.25 * tol, '%s %s: float32 on the CPU is %.3e of the row scale off the float64 reference: another seed' % (what, name, figs[name])
    return figs


def check(group, dt, cid, outs, got, base=None, tag=''):
    """every got[name] against outs[name]; with `base`, got - base -> the misses.  Every figure is printed; a test gathers the misses of all
    its runs (the hipops call, the direct calls, the pads) and asserts once at its end, so that one miss does not hide the next."""
    tol, misses = _tol(dt), []
    for name, g in got.items():
        o = outs[name]
        ref, live, scale = o['ref'], _live(o), row_scale(o)
        g = g.detach().cpu().reshape(ref.shape)
        b = base[name].reshape(ref.shape) if base is not None and name in base else None
        label = '%s %s %s %s%s' % (group, _dn(dt), cid, name, tag)
        nf = _nonfinite(o)
        if nf is not None:                                       # special values: the same value with its sign, exactly; then out of the way
            gs = torch.where(nf, g.double(), torch.full_like(ref, float('inf')))
            ws = torch.where(nf, o['spec'], torch.full_like(ref, float('inf')))
            bad = ~((gs == ws) | (torch.isnan(gs) & torch.isnan(ws)))
            if bool(bad.any()):
                i = bad.nonzero()[0].tolist()
                misses.append('%s: %d positions differ from the special value of the reference, first %s: %r for %r' % (
                    label, int(bad.sum()), i, float(g[tuple(i)]), float(o['spec'][tuple(i)])))
            g = torch.where(nf, torch.zeros_like(g), g)
        if not bool(torch.isfinite(g).all()):
            print('FIG %s nan' % label)
            misses.append('%s: %d values not finite' % (label, int((~torch.isfinite(g)).sum())))
            continue
        delta = g.double() - (b.double() if b is not None else 0.0)
        err = ((delta - ref).abs() / scale.clamp_min(1e-300)) * live
        worst = float(err.max()) if err.numel() else 0.0
        print('FIG %s %.3e' % (label, worst))
        if not worst < tol:
            misses.append('%s: error / row scale %.3e (bound %.0e) at %s' % (label, worst, tol, (err == err.max()).nonzero()[0].tolist()))
        if o['zero'] is not None:
            want = b if b is not None else torch.zeros_like(g)
            bad = (g != want) & o['zero']
            if bool(bad.any()):
                misses.append('%s: %d positions the kernel must leave %s differ, first %s' % (
                    label, int(bad.sum()), 'as they were' if b is not None else 'exactly 0.0', bad.nonzero()[0].tolist()))
    return misses


# ================================================================================================ memory around a direct call
def moat(t, fill):
    """CPU tensor -> (buffer, view holding t) on the device: PAD elements of `fill` in front of and behind the view"""
    n = t.numel()
    buf = torch.full((n + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    v = buf[PAD:PAD + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return buf, v


def nan_in(t):
    """a floating-point input as a view into a NaN-filled buffer"""
    return moat(t.contiguous(), NAN)[1]


class Outs:
    """the outputs of a direct call, each inside sentinel pads"""

    def __init__(self):
        self.bufs = {}

    def new(self, name, shape, dtype, base=None):
        """base: CPU tensor the kernel adds onto; None: NaN, the kernel must write every element"""
        init = base.to(dtype) if base is not None else torch.full(tuple(shape), NAN, dtype=dtype)
        self.bufs[name] = moat(init, SENT)
        return self.bufs[name][1]

    def collect(self, what, miss, names=None):
        torch.cuda.synchronize()
        bad = [n for n, (buf, v) in self.bufs.items() if not bool((buf[:PAD] == SENT).all() and (buf[-PAD:] == SENT).all())]
        if bad:
            miss.append('%s: the pads around %s were written' % (what, bad))
        return {n: v.cpu() for n, (buf, v) in self.bufs.items() if names is None or n in names}


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _dedup(t):
    return list(dict.fromkeys(t))


# ================================================================================================ panorama fusion
PANO_N = 3


def pano_limit(dt):
    return 1024 if dt == BF16 else 768


def pano_is_register(dt, H):
    """goat_pano_fusion_fwd / _bwd: the register pair for whole chunks, H <= 64 * EPC * MC (MC 2 bf16, 3 float32) and PF_NW * H floats of LDS"""
    return H % _epc(dt) == 0 and H <= 64 * _epc(dt) * (2 if dt == BF16 else 3) and 8 * H * 4 <= 64 * 1024


def _pano_table():
    t = []
    for dt in (F32, BF16):
        e, lim = _epc(dt), pano_limit(dt)
        t += [(dt, V, 768) for V in (1, 8, 9, 36, 63, 64)]                 # wave w owns slots w, w + 8, ...: one, full first trip, partial, full
        t += [(dt, 9, H) for H in (e, 64 * e - e, 64 * e + e, lim)]        # one chunk; a partly filled first / second chunk trip; the register limit
        t += [(dt, V, lim + e) for V in (1, 9, 64)]                        # generic pair by the H rule
        t.append((dt, 9, 772 if dt == BF16 else 70))                       # generic pair by H % EPC
    return _dedup(t)


PANO_TABLE = _pano_table()


def _pano_id(c):
    return '%s-V%d-H%d' % (_dn(c[0]), c[1], c[2])


@conditioned
def pano_case(dt, V, H, bump, rdt):
    """score_v = tanh(x_v . a + a0); w = softmax_v(score); fused = sum_v w_v x_v"""
    g = _gen(_sd('pano'), dt == BF16, V, H, bump)
    N = PANO_N
    c = dict(x=_randn(g, N, V, H).to(dt), a=_randn(g, H) / math.sqrt(H), a0=torch.tensor([0.1]), df=_randn(g, N, H).to(dt),
             base=dict(da=_randn(g, H), da0=_randn(g, 1)))
    x, a, a0 = (c[k].to(rdt).clone().requires_grad_(True) for k in ('x', 'a', 'a0'))
    w = torch.softmax(torch.tanh(x @ a + a0), 1)
    fused = (w.unsqueeze(-1) * x).sum(1)
    fused.backward(c['df'].to(rdt))
    c['outs'] = dict(fused=O(fused, 'row', dt), dx=O(x.grad, 'row', dt), da=O(a.grad, 'vec', F32), da0=O(a0.grad, 'vec', F32))
    return c


@pytest.mark.parametrize('case', PANO_TABLE, ids=_pano_id)
def test_pano_fusion(ops, case):
    """through hipops.pano_fusion (gradients from zero), then by direct calls inside pads with da / da0 added onto a non-zero base.  The
    last row of the last panorama ends at the pad: a store one chunk past a row lands there."""
    dt, V, H = case
    c, cid, N = pano_case(*case), _pano_id(case), PANO_N
    miss = []
    check_inputs(dt, c['outs'], cid)
    x = c['x'].to(DEV).requires_grad_(True)
    aw, ab = torch.nn.Parameter(c['a'].view(1, H).to(DEV)), torch.nn.Parameter(c['a0'].to(DEV))
    f = ops.pano_fusion(x, aw, ab)
    f.backward(c['df'].to(DEV))
    torch.cuda.synchronize()
    miss += check('pano', dt, cid, c['outs'], dict(fused=f, dx=x.grad, da=aw.grad, da0=ab.grad))
    xd, ad, a0d, dfd = (nan_in(c[k]) for k in ('x', 'a', 'a0', 'df'))
    o = Outs()
    fused, wsave = o.new('fused', (N, H), dt), o.new('wsave', (N, V), F32)
    ops.launch('goat_pano_fusion_fwd', ops._dt(xd), xd, ad, a0d, fused, wsave, N, V, H)
    dx, da, da0 = o.new('dx', (N, V, H), dt), o.new('da', (H,), F32, c['base']['da']), o.new('da0', (1,), F32, c['base']['da0'])
    ops.launch('goat_pano_fusion_bwd', ops._dt(xd), xd, ad, a0d, wsave, dfd, dx, da, da0, N, V, H)
    miss += check('pano', dt, cid, c['outs'], o.collect(cid, miss, ('fused', 'dx', 'da', 'da0')), c['base'], '@base')
    assert not miss, miss


# ================================================================================================ short-K weight gradient
def sk_rows_per_block(rows):
    """goat_wgrad_smallk: SK_ROWS 128 from 2048 rows on, 32 below"""
    return 128 if rows >= 2048 else 32


def sk_kp(dt, K):
    return (K + _epc(dt) - 1) // _epc(dt) * _epc(dt)


def _sk_table():
    """(dtype, K, rows, N, with dbias, ld_dw - K, ld_x - kp): every K at both row regimes, every N and rows per dtype"""
    t = []
    for dt in (F32, BF16):
        for i, K in enumerate((1, 4, 5, 8, 9, 12, 13, 16)):
            t.append((dt, K, (1, 31, 33, 2047)[i % 4], (1, 127, 129, 768)[(i + i // 4) % 4], i % 3 != 0, 3 * (i % 2), _epc(dt) * ((i + 1) % 2)))
            t.append((dt, K, (2048, 2100)[i % 2], (129, 1, 768, 127)[(i + i // 4) % 4], i % 3 != 1, 3 * ((i + 1) % 2), _epc(dt) * (i % 2)))
    return t


SK_TABLE = _sk_table()


def _sk_id(c):
    return '%s-K%d-r%d-N%d-b%d-lw%d-lx%d' % ((_dn(c[0]),) + tuple(int(v) for v in c[1:]))


@conditioned
def sk_case(dt, K, rows, N, bias, gap_w, gap_x, bump, rdt):
    """dW[n, k] = sum_r dy[r, n] x[r, k]; dbias[n] = sum_r dy[r, n]"""
    g = _gen(_sd('smallk'), dt == BF16, K, rows, N, bump)
    c = dict(dy=_randn(g, rows, N).to(dt), x=_randn(g, rows, K).to(dt), base_dw=_randn(g, N, K + gap_w), base_db=_randn(g, N))
    outs = dict(dw=O(c['dy'].to(rdt).T @ c['x'].to(rdt), 'row', F32))
    if bias:
        outs['dbias'] = O(c['dy'].to(rdt).sum(0), 'vec', F32)
    c['outs'] = outs
    return c


def _sk_launch(ops, case, c, from_base, miss):
    dt, K, rows, N, bias, gap_w, gap_x = case
    kp = sk_kp(dt, K)
    ld_x, ld_dw = kp + gap_x, K + gap_w
    xp = torch.full((rows, ld_x), NAN, dtype=dt)          # columns K .. kp - 1 are multiplied: zeros, as in production; NaN beyond kp only
    xp[:, :kp] = 0
    xp[:, :K] = c['x']
    w0 = c['base_dw'].clone()                              # the gap columns K .. ld_dw - 1 keep their base values in both runs
    if not from_base:
        w0[:, :K] = 0
    o = Outs()
    dw = o.new('dwfull', (N, ld_dw), F32, w0)
    db = o.new('dbias', (N,), F32, c['base_db'] if from_base else torch.zeros(N)) if bias else None
    ops.launch('goat_wgrad_smallk', ops._dt(xp), nan_in(c['dy']), N, nan_in(xp), ld_x, rows, N, K, dw, ld_dw, db)
    got = o.collect(_sk_id(case), miss)
    full = got.pop('dwfull')
    if not torch.equal(full[:, K:], w0[:, K:]):
        miss.append('%s: columns >= K of a dW row were written' % _sk_id(case))
    got['dw'] = full[:, :K]
    return got


@pytest.mark.parametrize('case', SK_TABLE, ids=_sk_id)
def test_wgrad_smallk(ops, case):
    dt, cid = case[0], _sk_id(case)
    c = sk_case(*case)
    miss = []
    check_inputs(dt, c['outs'], cid)
    miss += check('smallk', dt, cid, c['outs'], _sk_launch(ops, case, c, False, miss))
    miss += check('smallk', dt, cid, c['outs'], _sk_launch(ops, case, c, True, miss), dict(dw=c['base_dw'][:, :case[1]], dbias=c['base_db']), '@base')
    assert not miss, miss


SK_LINEAR = (100, 768, 7)


@conditioned
def sk_linear_case(dt, bump, rdt):
    rows, N, K = SK_LINEAR
    g = _gen(_sd('smallk-linear'), dt == BF16, bump)
    c = dict(x=_randn(g, rows, K).to(dt), w=_randn(g, N, K) * 0.3, b=_randn(g, N) * 0.1, dy=_randn(g, rows, N).to(dt))
    c['outs'] = dict(dw=O(c['dy'].to(rdt).T @ c['x'].to(rdt), 'row', F32), dbias=O(c['dy'].to(rdt).sum(0), 'vec', F32))
    return c


@pytest.mark.parametrize('dt', [F32, BF16], ids=_dn)
def test_wgrad_smallk_through_linear(ops, dt):
    """the 7-wide position Linear: hipops.linear pads K for its GEMM and hands the weight / bias gradients to goat_wgrad_smallk"""
    c = sk_linear_case(dt)
    miss = []
    check_inputs(dt, c['outs'], 'linear')
    assert ops.SMALLK_WGRAD
    w, b = torch.nn.Parameter(c['w'].to(DEV)), torch.nn.Parameter(c['b'].to(DEV))
    ops.linear(c['x'].to(DEV), w, b).backward(c['dy'].to(DEV))
    torch.cuda.synchronize()
    miss += check('smallk', dt, 'linear-r%d-N%d-K%d' % SK_LINEAR, c['outs'], dict(dw=w.grad, dbias=b.grad))
    assert not miss, miss


# ================================================================================================ InfoNCE
TAU = float(torch.tensor(0.07, dtype=F32))          # the production temperature, as the kernel receives it
NCE_TABLE = [(Bl, Ba, t0, H, form) for H in (68, 260) for Bl, Ba, t0, form in
             ((130, 130, 0, 'one'), (130, 130, 0, 'dp'), (33, 130, 64, 'dp'), (1, 65, 64, 'dp'), (64, 64, 0, 'one'), (64, 64, 0, 'dp'))]
NCE_NAMES = ('g', 'v', 'f', 't')


def _nce_id(c):
    return 'Bl%d-Ba%d-t%d-H%d-%s' % c


@conditioned
def nce_case(Bl, Ba, t0, H, form, bump, rdt):
    """loss_i = sum over x in (g, v, f) of 1/2 [CE(x_loc[i] . t_all^T / tau, t0 + i) + CE(t_loc[i] . x_all^T / tau, t0 + i)]; 'one': loc and all
    are the same tensors (one rank: both roles of a tensor add into one gradient), 'dp': distinct tensors, loc = rows t0 .. t0 + Bl of all"""
    g = _gen(_sd('infonce'), Bl, Ba, t0, H, bump)
    full = [torch.nn.functional.normalize(_randn(g, Ba, H), dim=1) for _ in range(4)]
    c = dict(all=full, loc=[t[t0:t0 + Bl].clone() for t in full], w=torch.rand(Bl, generator=g) + 0.5,
             base={'d%s_%s' % (n, r): _randn(g, Bl if r == 'loc' else Ba, H) for n in NCE_NAMES for r in ('loc', 'all')})
    ra = [t.to(rdt).clone().requires_grad_(True) for t in full]
    rl = ra if form == 'one' else [t.to(rdt).clone().requires_grad_(True) for t in c['loc']]
    tgt = torch.arange(Bl) + t0
    ce = torch.nn.functional.cross_entropy
    loss = sum(0.5 * (ce(rl[k] @ ra[3].T / TAU, tgt, reduction='none') + ce(rl[3] @ ra[k].T / TAU, tgt, reduction='none')) for k in range(3))
    (loss * c['w'].to(rdt)).sum().backward()
    outs = dict(loss=O(loss, 'vec', F32))
    for k, n in enumerate(NCE_NAMES):
        if form == 'dp':
            outs['d%s_loc' % n] = O(rl[k].grad, 'row', F32)
        outs['d%s_all' % n] = O(ra[k].grad, 'row', F32)
    c['outs'] = outs
    return c


def _nce_ops(ops, c, form):
    al = [t.to(DEV).requires_grad_(True) for t in c['all']]
    lo = al if form == 'one' else [t.to(DEV).requires_grad_(True) for t in c['loc']]
    loss = ops.infonce(lo[0], lo[1], lo[2], lo[3], al[0], al[1], al[2], al[3], c['t0'], TAU)
    (loss * c['w'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = dict(loss=loss)
    for k, n in enumerate(NCE_NAMES):
        if form == 'dp':
            got['d%s_loc' % n] = lo[k].grad
        got['d%s_all' % n] = al[k].grad
    return got


@pytest.mark.parametrize('case', NCE_TABLE, ids=_nce_id)
def test_infonce(ops, case):
    """float32 only, as the kernel is.  Ba > 64: the softmax loops and the similarity row take further trips; H = 68 / 260: the 64-column
    tail tile of the backward, the second 256-float trip of the forward.  One rank: twice, bit-equal (a fixed summation order is promised)."""
    Bl, Ba, t0, H, form = case
    c, cid = dict(nce_case(*case), t0=t0), _nce_id(case)
    miss = []
    check_inputs(F32, c['outs'], cid)
    got = _nce_ops(ops, c, form)
    miss += check('infonce', F32, cid, c['outs'], got)
    if form == 'one':
        again = _nce_ops(ops, c, form)
        for n in got:
            assert torch.equal(got[n], again[n]), '%s %s: two runs of one process differ' % (cid, n)
    elif Bl == 33:
        # direct calls: every d* added onto a non-zero base
        ins = {r: [nan_in(t) for t in c[r]] for r in ('loc', 'all')}
        o = Outs()
        loss, prob = o.new('loss', (Bl,), F32, torch.zeros(Bl)), o.new('prob', (6, Bl, Ba), F32)
        arr = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts[:3]])
        ops.launch('goat_infonce_fwd', arr(ins['loc']), arr(ins['all']), ins['loc'][3], ins['all'][3], loss, prob, Bl, Ba, H, t0, TAU)
        d = {r: [o.new('d%s_%s' % (n, r), c['base']['d%s_%s' % (n, r)].shape, F32, c['base']['d%s_%s' % (n, r)]) for n in NCE_NAMES] for r in ('loc', 'all')}
        ops.launch('goat_infonce_bwd', arr(ins['loc']), arr(ins['all']), ins['loc'][3], ins['all'][3], nan_in(c['w']), prob, arr(d['loc']), arr(d['all']),
                   d['loc'][3], d['all'][3], Bl, Ba, H, t0, TAU)
        got = o.collect(cid, miss)
        got.pop('prob')
        miss += check('infonce', F32, cid, c['outs'], got, c['base'], '@base')
    assert not miss, miss


# ================================================================================================ embedding tables
ES_MAXV, ES_MIN_ROWS, EMB_MAX_BLOCKS = 64, 512, 8192


def emb_bwd_branch(vocab, rows):
    """goat_embed_bwd on the word table alone: LDS accumulation for tables of at most 64 rows from 512 token rows on; otherwise one wave per
    token row with atomics, in at most 8192 blocks of 4 waves"""
    if vocab <= ES_MAXV and rows >= ES_MIN_ROWS:
        return 'small'
    return 'atomic-capped' if (rows + 3) // 4 > EMB_MAX_BLOCKS else 'atomic'


def _emb_bwd_table():
    t = []
    for dt in (F32, BF16):
        for (iv, vocab), (ir, rows) in itertools.product(enumerate((1, 3, 64)), enumerate((512, 513, 767))):
            t.append((dt, vocab, rows, (8, 72, 768)[(iv + ir) % 3]))
        t += [(dt, 65, 600, 72), (dt, 64, 511, 72), (dt, 70, 33000, 8)]
    return t


EMB_BWD_TABLE = _emb_bwd_table()


def _emb_bwd_id(c):
    return '%s-v%d-r%d-H%d' % (_dn(c[0]), c[1], c[2], c[3])


@conditioned
def emb_bwd_case(dt, vocab, rows, H, bump, rdt):
    """dword[ids[r]] += dout[r] for 0 <= ids[r] < vocab, ids[r] != pad"""
    g = _gen(_sd('embed-bwd'), dt == BF16, vocab, rows, H, bump)
    ids = torch.randint(0, vocab, (rows,), generator=g)
    ids[5] = ids[17] = ids[300] = vocab          # out of range: skipped by both kernels
    ids[40] = -1
    pad = 1 if vocab > 1 else -1                  # the padding row inside the table
    c = dict(ids=ids, pad=pad, dout=_randn(g, rows, H).to(dt), base=dict(dword=_randn(g, vocab, H)))
    use = (ids >= 0) & (ids < vocab) & (ids != pad)
    ref = torch.zeros(vocab, H, dtype=rdt).index_add_(0, ids[use], c['dout'].to(rdt)[use])
    named = torch.zeros(vocab, dtype=torch.bool)
    named[ids[use]] = True
    c['outs'] = dict(dword=O(ref, 'row', F32, ~named[:, None]))
    return c


@pytest.mark.parametrize('case', EMB_BWD_TABLE, ids=_emb_bwd_id)
def test_embedding_scatter_add(ops, case):
    """hipops.embedding_scatter_add into a table inside pads, from zero and onto a base; rows nobody names (the padding row among them)
    keep their bits"""
    dt, vocab, rows, H = case
    c, cid = emb_bwd_case(*case), _emb_bwd_id(case)
    miss = []
    check_inputs(dt, c['outs'], cid)
    dout, ids = nan_in(c['dout']), c['ids'].to(DEV)
    for base in (None, c['base']):
        o = Outs()
        dword = o.new('dword', (vocab, H), F32, base['dword'] if base else torch.zeros(vocab, H))
        ops.embedding_scatter_add(dword, dout, ids, word_pad=c['pad'])
        miss += check('embed', dt, cid, c['outs'], o.collect(cid, miss), base, '@base' if base else '')
    ops.check_embed_errors()
    assert not miss, miss


EMB_FWD_TABLE = [(dt, H) for dt in (F32, BF16) for H in (8, 72, 768)]


@conditioned
def emb_fwd_case(dt, H, bump, rdt):
    """out[b, l] = word[ids[b, l]] + type[tids[b, l]] + pos[l]; the gradient of word row `pad` and of position row `pad` is zero"""
    g = _gen(_sd('embed-fwd'), dt == BF16, H, bump)
    B, L, V, P, pad = 3, 5, 11, 7, 1
    c = dict(word=_randn(g, V, H), typ=_randn(g, 2, H), pos=_randn(g, P, H), ids=torch.randint(0, V, (B, L), generator=g),
             tids=torch.randint(0, 2, (B, L), generator=g), dout=_randn(g, B, L, H).to(dt), pad=pad)
    c['ids'][:, -1] = pad
    c['ids'][0, :2] = 4
    ids, tids, d = c['ids'], c['tids'], c['dout'].to(rdt)
    out = c['word'].to(rdt)[ids] + c['typ'].to(rdt)[tids] + c['pos'].to(rdt)[:L][None]
    use = (ids != pad).reshape(-1)
    dword = torch.zeros(V, H, dtype=rdt).index_add_(0, ids.reshape(-1)[use], d.reshape(-1, H)[use])
    named = torch.zeros(V, dtype=torch.bool)
    named[ids.reshape(-1)[use]] = True
    dtyp = torch.zeros(2, H, dtype=rdt).index_add_(0, tids.reshape(-1), d.reshape(-1, H))
    dpos = torch.zeros(P, H, dtype=rdt)
    dpos[:L] = d.sum(0)
    dpos[pad] = 0
    live = torch.zeros(P, dtype=torch.bool)
    live[:L] = True
    live[pad] = False
    c['outs'] = dict(out=O(out, 'row', dt), dword=O(dword, 'row', F32, ~named[:, None]), dtype=O(dtyp, 'row', F32), dpos=O(dpos, 'row', F32, ~live[:, None]))
    return c


@pytest.mark.parametrize('case', EMB_FWD_TABLE, ids=lambda c: '%s-H%d' % (_dn(c[0]), c[1]))
def test_embedding_forward_and_table_gradients(ops, case):
    """hipops.embedding with all three tables (the position gradient is a column sum over dout viewed [B, L * H] with ld > C, split around
    the padding position); from the word table alone the float32 lookup is a copy"""
    dt, H = case
    c, cid = emb_fwd_case(*case), '%s-H%d' % (_dn(dt), H)
    miss = []
    check_inputs(dt, c['outs'], cid)
    word, typ, pos = (torch.nn.Parameter(c[k].to(DEV)) for k in ('word', 'typ', 'pos'))
    ids = c['ids'].to(DEV)
    out = ops.embedding(ids, word, typ, c['tids'].to(DEV), pos, out_dtype=dt, word_pad=c['pad'], pos_pad=c['pad'])
    out.backward(c['dout'].to(DEV))
    alone = ops.embedding(ids, word, out_dtype=dt)
    torch.cuda.synchronize()
    ops.check_embed_errors()
    miss += check('embed', dt, cid, c['outs'], dict(out=out, dword=word.grad, dtype=typ.grad, dpos=pos.grad))
    if dt == F32:
        assert torch.equal(alone.cpu(), c['word'][c['ids']]), '%s: the word-table lookup is not a copy' % cid
    assert not miss, miss


# ================================================================================================ gather / segment mean
GATHER_MAX_BLOCKS = 4096


def gather_is_capped(dt, n_out, H):
    """goat_gather_segmean_fwd / _bwd: one thread per (output row, chunk), at most 4096 blocks of 256"""
    return (n_out * (H // _epc(dt)) + 255) // 256 > GATHER_MAX_BLOCKS


GATHER_SRC = 50
_MIXED = ((), (3,), (4, -1, 4, 7), (49, 0), (-1, 5), (1, 2, 3, 5), (10,), (-1,), (11, 12), ())      # empty first and last; -1 between valid entries


def _gather_segs(kind):
    if kind == 'copy':
        return tuple((i * 7 % GATHER_SRC,) for i in range(12))
    if kind == 'cap':
        return tuple((i % GATHER_SRC, -1, (i + 1) % GATHER_SRC) if i % 97 == 0 else (i % GATHER_SRC,) for i in range(6000))
    return _MIXED


def _gather_table():
    """(dtype, H, segments, scale, tok_w)"""
    t = []
    for dt in (F32, BF16):
        for H in (_epc(dt), 768):
            t += [(dt, H, 'mixed', True, False), (dt, H, 'mixed', False, False), (dt, H, 'mixed', True, True), (dt, H, 'copy', False, False)]
    t.append((F32, 768, 'cap', True, False))
    return t


GATHER_TABLE = _gather_table()


def _gather_id(c):
    return '%s-H%d-%s-%s%s' % (_dn(c[0]), c[1], c[2], 'scale' if c[3] else 'noscale', '-tokw' if c[4] else '')


@conditioned
def gather_case(dt, H, kind, with_scale, with_tokw, bump, rdt):
    """out[i] = scale[i] * sum over j in segment i with idx[j] >= 0 of tok_w[j] * src[idx[j]]; the atomic backward (no tok_w) adds
    scale[i] * dout[i] into dsrc[idx[j]]"""
    g = _gen(_sd('gather'), dt == BF16, H, _sd(kind), with_scale, with_tokw, bump)
    segs = _gather_segs(kind)
    n_out = len(segs)
    idx = torch.tensor([i for s in segs for i in s], dtype=torch.int32)
    start = torch.tensor([0] + list(itertools.accumulate(len(s) for s in segs)), dtype=torch.int32)
    seg_of = torch.repeat_interleave(torch.arange(n_out), start[1:].long() - start[:-1].long())
    valid = idx >= 0
    cnt = torch.zeros(n_out).index_add_(0, seg_of[valid], torch.ones(int(valid.sum())))
    c = dict(src=_randn(g, GATHER_SRC, H).to(dt), dout=_randn(g, n_out, H).to(dt), idx=idx, start=start, n_out=n_out,
             scale=(1.0 / cnt.clamp_min(1)) if with_scale else None, tok_w=(torch.rand(idx.numel(), generator=g) + 0.5) if with_tokw else None,
             base=dict(dsrc=_randn(g, GATHER_SRC, H)))
    sc = c['scale'].to(rdt) if with_scale else torch.ones(n_out, dtype=rdt)
    tw = c['tok_w'].to(rdt) if with_tokw else torch.ones(idx.numel(), dtype=rdt)
    si, sg = idx[valid].long(), seg_of[valid]
    out = torch.zeros(n_out, H, dtype=rdt).index_add_(0, sg, c['src'].to(rdt)[si] * tw[valid][:, None]) * sc[:, None]
    dsrc = torch.zeros(GATHER_SRC, H, dtype=rdt).index_add_(0, si, (c['dout'].to(rdt) * sc[:, None])[sg])
    named = torch.zeros(GATHER_SRC, dtype=torch.bool)
    named[si] = True
    c['outs'] = dict(out=O(out, 'row', dt, (cnt == 0)[:, None]), dsrc=O(dsrc, 'row', dt, ~named[:, None]))
    c['outs32'] = dict(dsrc=O(dsrc, 'row', F32, ~named[:, None]))
    return c


@pytest.mark.parametrize('case', GATHER_TABLE, ids=_gather_id)
def test_gather_segmean(ops, case):
    """without tok_w through hipops.gather_segmean: the forward, the atomic backward and the inverse-index backward against the same float64
    reference; then by direct calls inside pads (tok_w on the forward; the atomic backward onto a base, rows no segment names untouched).
    One source per segment without scale is a copy."""
    from vln_goat_amd import graphmap
    dt, H, kind, with_scale, with_tokw = case
    c, cid = gather_case(*case), _gather_id(case)
    n_out = c['n_out']
    miss = []
    check_inputs(dt, c['outs'], cid)
    idx, start = c['idx'].to(DEV), c['start'].to(DEV)
    scale = c['scale'].to(DEV) if with_scale else None
    if not with_tokw:
        src = c['src'].to(DEV).requires_grad_(True)
        out = ops.gather_segmean(src, idx, start, scale, n_out)
        out.backward(c['dout'].to(DEV))
        inv = tuple(t.to(DEV) for t in graphmap.inverse_index(c['idx'], c['start'], c['scale'], GATHER_SRC) if t is not None)
        src2 = c['src'].to(DEV).requires_grad_(True)
        ops.gather_segmean(src2, idx, start, scale, n_out, inv).backward(c['dout'].to(DEV))
        torch.cuda.synchronize()
        miss += check('gather', dt, cid, c['outs'], dict(out=out, dsrc=src.grad))
        miss += check('gather', dt, cid, c['outs'], dict(dsrc=src2.grad), tag='@inverse')
        if kind == 'copy':
            assert torch.equal(out.detach().cpu(), c['src'][c['idx'].long()]), '%s: one source per segment is not a copy' % cid
    o = Outs()
    out = o.new('out', (n_out, H), dt)
    srcd, doutd = nan_in(c['src']), nan_in(c['dout'])
    ops.launch('goat_gather_segmean_fwd', ops._dt(srcd), srcd, GATHER_SRC, idx, start, nan_in(c['scale']) if with_scale else None, out, n_out, H,
               nan_in(c['tok_w']) if with_tokw else None)
    miss += check('gather', dt, cid, c['outs'], o.collect(cid, miss), tag='@direct')
    if not with_tokw:
        o = Outs()
        dsrc = o.new('dsrc', (GATHER_SRC, H), F32, c['base']['dsrc'])
        ops.launch('goat_gather_segmean_bwd', ops._dt(doutd), doutd, idx, start, nan_in(c['scale']) if with_scale else None, dsrc, n_out, H)
        miss += check('gather', dt, cid, c['outs32'], o.collect(cid, miss), c['base'], '@base')
    assert not miss, miss


# ================================================================================================ door gate
DOOR_TABLE = [(dt, rows, H) for dt in (F32, BF16) for rows, H in
              ((1, 1024), (5, 63), (1024, 65), (1029, 768), (2051, 1), (2051, 1024), (5, 65), (1029, 63))]


def door_bwd_is_capped(rows):
    """goat_door_gate_bwd: at most 256 blocks of 4 waves; beyond 1024 rows a wave keeps partials over several rows"""
    return (rows + 3) // 4 > 256


def _door_id(c):
    return '%s-r%d-H%d' % (_dn(c[0]), c[1], c[2])


@conditioned
def door_case(dt, rows, H, bump, rdt):
    """s = sigmoid(aug . wa + ba + ori . wo + bo); out = s aug + (1 - s) ori; both biases receive the same gradient"""
    g = _gen(_sd('door'), dt == BF16, rows, H, bump)
    c = dict(aug=_randn(g, rows, H).to(dt), ori=_randn(g, rows, H).to(dt), wa=_randn(g, H) / math.sqrt(H), wo=_randn(g, H) / math.sqrt(H),
             ba=torch.tensor([0.2]), bo=torch.tensor([-0.1]), dout=_randn(g, rows, H).to(dt),
             base=dict(dwa=_randn(g, H), dwo=_randn(g, H), dbias=_randn(g, 1), dbias2=_randn(g, 1)))
    aug, ori, wa, wo, ba = (c[k].to(rdt).clone().requires_grad_(True) for k in ('aug', 'ori', 'wa', 'wo', 'ba'))
    s = torch.sigmoid(aug @ wa + ba + ori @ wo + c['bo'].to(rdt))
    out = s[:, None] * aug + (1 - s[:, None]) * ori
    out.backward(c['dout'].to(rdt))
    c['outs'] = dict(out=O(out, 'row', dt), gate=O(s, 'vec', F32), daug=O(aug.grad, 'row', dt), dori=O(ori.grad, 'row', dt),
                     dwa=O(wa.grad, 'vec', F32), dwo=O(wo.grad, 'vec', F32), dbias=O(ba.grad, 'vec', F32), dbias2=O(ba.grad, 'vec', F32))
    return c


@pytest.mark.parametrize('case', DOOR_TABLE, ids=_door_id)
def test_door_gate(ops, case):
    """through the autograd function (gradients from zero), then by direct calls inside pads: dbias2 NULL from zero, dbias2 set onto a base"""
    dt, rows, H = case
    c, cid = door_case(*case), _door_id(case)
    miss = []
    check_inputs(dt, c['outs'], cid)
    aug, ori = c['aug'].to(DEV).requires_grad_(True), c['ori'].to(DEV).requires_grad_(True)
    prm = [torch.nn.Parameter(c[k].to(DEV).view(s)) for k, s in (('wa', (1, H)), ('ba', (1,)), ('wo', (1, H)), ('bo', (1,)))]
    out = ops._DoorGateFn.apply(aug, ori, *prm)
    out.backward(c['dout'].to(DEV))
    torch.cuda.synchronize()
    miss += check('door', dt, cid, c['outs'], dict(out=out, daug=aug.grad, dori=ori.grad, dwa=prm[0].grad, dbias=prm[1].grad, dwo=prm[2].grad, dbias2=prm[3].grad))
    ins = {k: nan_in(c[k]) for k in ('aug', 'ori', 'wa', 'wo', 'ba', 'bo', 'dout')}
    code = ops._dt(ins['aug'])
    for base in (None, c['base']):
        o = Outs()
        outd, gate = o.new('out', (rows, H), dt), o.new('gate', (rows,), F32)
        ops.launch('goat_door_gate_fwd', code, ins['aug'], ins['ori'], ins['wa'], ins['wo'], ins['ba'], ins['bo'], outd, gate, rows, H)
        daug, dori = o.new('daug', (rows, H), dt), o.new('dori', (rows, H), dt)
        acc = {k: o.new(k, c['base'][k].shape, F32, base[k] if base else torch.zeros_like(c['base'][k]))
               for k in (('dwa', 'dwo', 'dbias', 'dbias2') if base else ('dwa', 'dwo', 'dbias'))}
        ops.launch('goat_door_gate_bwd', code, ins['aug'], ins['ori'], ins['wa'], ins['wo'], gate, ins['dout'], daug, dori, acc['dwa'], acc['dwo'],
                   acc['dbias'], rows, H, acc.get('dbias2'))
        miss += check('door', dt, cid, c['outs'], o.collect(cid, miss), base, '@base' if base else '@direct')
    assert not miss, miss


# ================================================================================================ rowdot
ROWDOT_TABLE = [(dt, M, H, bias) for dt in (F32, BF16) for M, H, bias in
                ((1, 8, True), (3, 1016, False), (513, 1024, True), (2051, 8, False), (2051, 1024, True), (513, 1016, True), (3, 1024, False))]


def rowdot_bwd_is_capped(M):
    """goat_rowdot_bwd: at most 128 blocks of 4 waves"""
    return (M + 3) // 4 > 128


def _rowdot_id(c):
    return '%s-M%d-H%d-%s' % (_dn(c[0]), c[1], c[2], 'bias' if c[3] else 'nobias')


@conditioned
def rowdot_case(dt, M, H, bias, bump, rdt):
    """y[m] = x[m] . w + b with w rounded to the activation dtype; dx[m] = dy[m] w; dw = sum_m dy[m] x[m]; db = sum_m dy[m]"""
    g = _gen(_sd('rowdot'), dt == BF16, M, H, bump)
    c = dict(x=_randn(g, M, H).to(dt), w=_randn(g, H) / math.sqrt(H), b=torch.tensor([0.3]), dy=_randn(g, M).to(dt),
             base=dict(dw=_randn(g, H), db=_randn(g, 1)))
    x, dy, wq = c['x'].to(rdt), c['dy'].to(rdt), c['w'].to(dt).to(rdt)
    outs = dict(y=O(x @ wq + (c['b'].to(rdt) if bias else 0.0), 'vec', dt), dx=O(dy[:, None] * wq[None], 'row', dt), dw=O(dy @ x, 'vec', F32))
    if bias:
        outs['db'] = O(dy.sum().reshape(1), 'vec', F32)
    c['outs'] = outs
    return c


@pytest.mark.parametrize('case', ROWDOT_TABLE, ids=_rowdot_id)
def test_rowdot(ops, case):
    """through hipops.linear (one output column), then by direct calls inside pads: dx only; dw (and db) only, onto a base; and the entry
    point refuses a bias gradient without a weight gradient (the kernel has no such form)"""
    dt, M, H, bias = case
    c, cid = rowdot_case(*case), _rowdot_id(case)
    miss = []
    check_inputs(dt, c['outs'], cid)
    x = c['x'].to(DEV).requires_grad_(True)
    w = torch.nn.Parameter(c['w'].view(1, H).to(DEV))
    b = torch.nn.Parameter(c['b'].to(DEV)) if bias else None
    assert ops.ROWDOT
    y = ops.linear(x, w, b)
    assert y.shape == (M, 1)
    y.backward(c['dy'].view(M, 1).to(DEV))
    torch.cuda.synchronize()
    got = dict(y=y, dx=x.grad, dw=w.grad)
    if bias:
        got['db'] = b.grad
    miss += check('rowdot', dt, cid, c['outs'], got)
    xd, wd, dyd = nan_in(c['x']), nan_in(c['w']), nan_in(c['dy'])
    code = ops._dt(xd)
    o = Outs()
    yd, dx = o.new('y', (M,), dt), o.new('dx', (M, H), dt)
    ops.launch('goat_rowdot_fwd', code, xd, wd, nan_in(c['b']) if bias else None, yd, M, H)
    ops.launch('goat_rowdot_bwd', code, xd, wd, dyd, dx, None, None, M, H)
    miss += check('rowdot', dt, cid, c['outs'], o.collect(cid, miss), tag='@dx-only')
    o = Outs()
    dw = o.new('dw', (H,), F32, c['base']['dw'])
    db = o.new('db', (1,), F32, c['base']['db']) if bias else None
    ops.launch('goat_rowdot_bwd', code, xd, wd, dyd, None, dw, db, M, H)
    miss += check('rowdot', dt, cid, c['outs'], o.collect(cid, miss), c['base'], '@dw-only-base')
    lone = torch.full((1,), SENT, device=DEV)
    st = ops._lib.lib().goat_rowdot_bwd(torch.cuda.current_stream().cuda_stream, code, xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), None, None,
                                        lone.data_ptr(), M, H)
    torch.cuda.synchronize()
    assert st == GOAT_E_ARG and float(lone) == SENT
    assert not miss, miss


# ================================================================================================ attention pooling
POOL_B = 2
POOL_TABLE = [(dt, L, H, mask) for dt in (F32, BF16) for L, H, mask in
              ((1, 4, False), (3, 260, False), (255, 256, False), (256, 768, False), (257, 260, False), (512, 4, False), (512, 768, True),
               (257, 256, False))]


def pool_bwd_is_wide(L):
    """goat_attn_pool_bwd: one slot per thread up to 256 slots, slots strided over the block beyond"""
    return L > 256


def _pool_id(c):
    return '%s-L%d-H%d%s' % (_dn(c[0]), c[1], c[2], '-mask' if c[3] else '')


@conditioned
def pool_case(dt, L, H, mask, bump, rdt):
    """a = softmax_l(tanh(x_l) . w + slot mask); out = tanh(sum_l a_l x_l); a masked slot has weight 0 and a zero gradient"""
    g = _gen(_sd('pool'), dt == BF16, L, H, bump)
    B = POOL_B
    c = dict(x=_randn(g, B, L, H).to(dt), w=_randn(g, H) / math.sqrt(H), dout=_randn(g, B, H), base=dict(dw=_randn(g, H)), smask=None)
    dead = torch.zeros(B, L, dtype=torch.bool)
    if mask:                                                       # -inf in both halves of a 512-slot row
        dead[0, [3, 100, 255, 256, 300, 511]] = True
        dead[1, 200:300] = True
        c['smask'] = torch.zeros(B, L).masked_fill(dead, float('-inf'))
    x, w = c['x'].to(rdt).clone().requires_grad_(True), c['w'].to(rdt).clone().requires_grad_(True)
    score = torch.tanh(x) @ w
    if mask:
        score = score + c['smask'].to(rdt)
    a = torch.softmax(score, 1)
    out = torch.tanh((a.unsqueeze(-1) * x).sum(1))
    out.backward(c['dout'].to(rdt))
    c['outs'] = dict(out=O(out, 'row', F32), attn=O(a, 'row', F32, dead if mask else None), dx=O(x.grad, 'row', dt, dead[..., None] if mask else None),
                     dw=O(w.grad, 'vec', F32))
    return c


@pytest.mark.parametrize('case', POOL_TABLE, ids=_pool_id)
def test_attn_pool(ops, case):
    """through hipops.attn_pool, then by direct calls inside pads with dw added onto a base.  H = 4 / 260: a (second) 256-column slab with
    one live quad; L = 256 / 257: either side of the switch between the two backward kernels."""
    dt, L, H, mask = case
    c, cid, B = pool_case(*case), _pool_id(case), POOL_B
    miss = []
    check_inputs(dt, c['outs'], cid)
    x, w = c['x'].to(DEV).requires_grad_(True), torch.nn.Parameter(c['w'].view(1, H).to(DEV))
    out = ops.attn_pool(x, w, c['smask'].to(DEV) if mask else None)
    out.backward(c['dout'].to(DEV))
    torch.cuda.synchronize()
    miss += check('pool', dt, cid, c['outs'], dict(out=out, dx=x.grad, dw=w.grad))
    xd, wd, doutd = nan_in(c['x']), nan_in(c['w']), nan_in(c['dout'])
    code = ops._dt(xd)
    o = Outs()
    outd, attn, ws = o.new('out', (B, H), F32), o.new('attn', (B, L), F32), o.new('ws', (B * L,), F32)
    ops.launch('goat_attn_pool_fwd', code, xd, wd, outd, attn, ws, B, L, H, c['smask'].to(DEV) if mask else None)
    dx, dw, ws2 = o.new('dx', (B, L, H), dt), o.new('dw', (H,), F32, c['base']['dw']), o.new('ws2', (B * L,), F32)
    ops.launch('goat_attn_pool_bwd', code, xd, wd, attn, outd, doutd, dx, dw, ws2, B, L, H)
    miss += check('pool', dt, cid, c['outs'], o.collect(cid, miss, ('out', 'attn', 'dx', 'dw')), c['base'], '@base')
    assert not miss, miss


# ================================================================================================ dict_wsum, cfp_mix
WSUM_B = 3
WSUM_TABLE = [(dt, K, H) for dt in (F32, BF16) for K, H in ((1, 768), (3, 255), (4, 1), (5, 257), (39, 768), (39, 255), (5, 1), (3, 257), (1, 1), (4, 768))]


def _wsum_id(c):
    return '%s-K%d-H%d' % (_dn(c[0]), c[1], c[2])


@conditioned
def wsum_case(dt, K, H, bump, rdt):
    """out[b] = sum_k p[b, k] z[b, k]; dz[b, k] = p[b, k] dout[b]; dp[b, k] = z[b, k] . dout[b]"""
    g = _gen(_sd('wsum'), dt == BF16, K, H, bump)
    B = WSUM_B
    c = dict(z=_randn(g, B, K, H), p=torch.softmax(_randn(g, B, K), 1), dout=_randn(g, B, 1, H).to(dt))
    z, p, d = c['z'].to(rdt), c['p'].to(rdt), c['dout'].to(rdt)
    c['outs'] = dict(out=O((p[..., None] * z).sum(1, keepdim=True), 'row', dt), dz=O(p[..., None] * d, 'row', F32), dp=O((z * d).sum(-1), 'row', F32))
    return c


@pytest.mark.parametrize('case', WSUM_TABLE, ids=_wsum_id)
def test_dict_wsum(ops, case):
    """through hipops.dict_weighted_sum with both, dz only and dp only; by direct calls inside pads; K = 1 with p = 1 is a copy"""
    dt, K, H = case
    c, cid, B = wsum_case(*case), _wsum_id(case), WSUM_B
    miss = []
    check_inputs(dt, c['outs'], cid)
    for tag, need_z, need_p in (('', True, True), ('@dz-only', True, False), ('@dp-only', False, True)):
        z, p = c['z'].to(DEV).requires_grad_(need_z), c['p'].to(DEV).requires_grad_(need_p)
        out = ops.dict_weighted_sum(z, p, dt)
        out.backward(c['dout'].to(DEV))
        torch.cuda.synchronize()
        assert (z.grad is not None) == need_z and (p.grad is not None) == need_p
        got = dict(out=out)
        if need_z:
            got['dz'] = z.grad
        if need_p:
            got['dp'] = p.grad
        miss += check('wsum', dt, cid, c['outs'], got, tag=tag)
    zd, pd, dd = nan_in(c['z']), nan_in(c['p']), nan_in(c['dout'])
    o = Outs()
    out, dz, dp = o.new('out', (B, 1, H), dt), o.new('dz', (B, K, H), F32), o.new('dp', (B, K), F32)
    ops.launch('goat_dict_wsum_fwd', ops._dt(out), zd, pd, out, B, K, H)
    ops.launch('goat_dict_wsum_bwd', ops._dt(dd), dd, zd, pd, dz, dp, B, K, H)
    miss += check('wsum', dt, cid, c['outs'], o.collect(cid, miss), tag='@direct')
    if K == 1 and dt == F32:
        one = ops.dict_weighted_sum(c['z'].to(DEV), torch.ones(B, 1, device=DEV), F32)
        assert torch.equal(one.cpu(), c['z']), '%s: p = 1 over one slot is not a copy' % cid
    assert not miss, miss


MIX_TABLE = [(dt, H) for dt in (F32, BF16) for H in (1, 255, 257, 768)]


@conditioned
def mix_case(dt, H, bump, rdt):
    """w = sigmoid(fwl); fo = go w + vo (1 - w); dgo = dfo w; dvo = dfo (1 - w); dfwl = w (1 - w) sum_h dfo (go - vo)"""
    g = _gen(_sd('mix'), dt == BF16, H, bump)
    B = WSUM_B
    c = dict(go=_randn(g, B, H), vo=_randn(g, B, H), fwl=_randn(g, B).to(dt), dfo=_randn(g, B, H), base=dict(dgo=_randn(g, B, H), dvo=_randn(g, B, H)))
    go, vo, dfo = c['go'].to(rdt), c['vo'].to(rdt), c['dfo'].to(rdt)
    w = torch.sigmoid(c['fwl'].to(rdt))[:, None]
    c['outs'] = dict(fo=O(go * w + vo * (1 - w), 'row', F32), fw=O(w[:, 0], 'vec', F32), dgo=O(dfo * w, 'row', F32), dvo=O(dfo * (1 - w), 'row', F32),
                     dfwl=O((w * (1 - w) * (dfo * (go - vo)).sum(1, keepdim=True))[:, 0], 'vec', dt))
    return c


@pytest.mark.parametrize('case', MIX_TABLE, ids=lambda c: '%s-H%d' % (_dn(c[0]), c[1]))
def test_cfp_mix(ops, case):
    """through hipops.cfp_mix, then by direct calls inside pads with accumulate = 0 and accumulate = 1 onto a base"""
    dt, H = case
    c, cid, B = mix_case(*case), '%s-H%d' % (_dn(dt), H), WSUM_B
    miss = []
    check_inputs(dt, c['outs'], cid)
    go, vo, fwl = (c[k].to(DEV).requires_grad_(True) for k in ('go', 'vo', 'fwl'))
    fo = ops.cfp_mix(go, vo, fwl)
    fo.backward(c['dfo'].to(DEV))
    torch.cuda.synchronize()
    miss += check('mix', dt, cid, c['outs'], dict(fo=fo, dgo=go.grad, dvo=vo.grad, dfwl=fwl.grad))
    god, vod, fwld, dfod = (nan_in(c[k]) for k in ('go', 'vo', 'fwl', 'dfo'))
    for base in (None, c['base']):
        o = Outs()
        fod, fw = o.new('fo', (B, H), F32), o.new('fw', (B,), F32)
        ops.launch('goat_cfp_mix_fwd', ops._dt(fwld), god, vod, fwld, fod, fw, B, H)
        dgo, dvo, dfwl = o.new('dgo', (B, H), F32, base and base['dgo']), o.new('dvo', (B, H), F32, base and base['dvo']), o.new('dfwl', (B,), dt)
        ops.launch('goat_cfp_mix_bwd', ops._dt(fwld), god, vod, fw, dfod, dgo, dvo, dfwl, B, H, 1 if base else 0)
        miss += check('mix', dt, cid, c['outs'], o.collect(cid, miss), base, '@accumulate' if base else '@direct')
    assert not miss, miss


# ================================================================================================ column sums
COLSUM_TABLE = [(dt, R, C, ld) for dt in (F32, BF16) for R, C, ld in ((1, 1, 1), (31, 65, 65), (33, 64, 200), (4097, 130, 136))]


def colsum_grid(R, C):
    """goat_colsum: 64 columns per block; up to 1024 / column blocks row strips, none shorter than 32 rows -> (column blocks, row strips)"""
    cb = (C + 63) // 64
    rb = max(1, min((1024 + cb - 1) // cb, (R + 31) // 32))
    rpb = (R + rb - 1) // rb
    return cb, (R + rpb - 1) // rpb


def _colsum_id(c):
    return '%s-R%d-C%d-ld%d' % (_dn(c[0]), c[1], c[2], c[3])


@conditioned
def colsum_case(dt, R, C, ld, bump, rdt):
    g = _gen(_sd('colsum'), dt == BF16, R, C, ld, bump)
    c = dict(x=_randn(g, R, C).to(dt), base=dict(colsum=_randn(g, C)))
    c['outs'] = dict(colsum=O(c['x'].to(rdt).sum(0), 'vec', F32))
    return c


@pytest.mark.parametrize('case', COLSUM_TABLE, ids=_colsum_id)
def test_colsum(ops, case):
    """direct calls, the columns C .. ld - 1 of every row NaN; from zero and onto a base"""
    dt, R, C, ld = case
    c, cid = colsum_case(*case), _colsum_id(case)
    miss = []
    check_inputs(dt, c['outs'], cid)
    xp = torch.full((R, ld), NAN, dtype=dt)
    xp[:, :C] = c['x']
    xd = nan_in(xp)
    for base in (None, c['base']):
        o = Outs()
        out = o.new('colsum', (C,), F32, base['colsum'] if base else torch.zeros(C))
        ops.launch('goat_colsum', ops._dt(xd), xd, ld, R, C, out)
        miss += check('colsum', dt, cid, c['outs'], o.collect(cid, miss), base, '@base' if base else '')
    assert not miss, miss


# ================================================================================================ the tables as a whole (no GPU)
FAMILIES = (('pano', PANO_TABLE, pano_case, _pano_id), ('smallk', SK_TABLE, sk_case, _sk_id),
            ('smallk-linear', [(F32,), (BF16,)], sk_linear_case, lambda c: _dn(c[0])),
            ('infonce', NCE_TABLE, nce_case, _nce_id), ('embed-bwd', EMB_BWD_TABLE, emb_bwd_case, _emb_bwd_id),
            ('embed-fwd', EMB_FWD_TABLE, emb_fwd_case, lambda c: '%s-H%d' % (_dn(c[0]), c[1])), ('gather', GATHER_TABLE, gather_case, _gather_id),
            ('door', DOOR_TABLE, door_case, _door_id), ('rowdot', ROWDOT_TABLE, rowdot_case, _rowdot_id), ('pool', POOL_TABLE, pool_case, _pool_id),
            ('wsum', WSUM_TABLE, wsum_case, _wsum_id), ('mix', MIX_TABLE, mix_case, lambda c: '%s-H%d' % (_dn(c[0]), c[1])),
            ('colsum', COLSUM_TABLE, colsum_case, _colsum_id))


def check_all_inputs(verbose=False):
    """conditions a. and b. over every case of every table -> number of cases"""
    n = 0
    for name, table, build, ident in FAMILIES:
        for case in table:
            c = build(*case)
            dt = case[0] if isinstance(case[0], torch.dtype) else F32
            check_inputs(dt, c['outs'], '%s %s' % (name, ident(case)))
            if 'outs32' in c:
                check_inputs(dt, c['outs32'], '%s %s' % (name, ident(case)))
            n += 1
            if verbose:
                print('ok %s %s  seed bump %d  float32 on the CPU / row scale: %s' % (
                    name, ident(case), c['bump'], ' '.join('%s %.1e' % kv for kv in sorted(c['f32_cpu'].items()))))
    return n


def branches():
    """every dispatch branch of the entry points -> whether a case of the tables reaches it (the rules restated from csrc/)"""
    b = {}
    for dt in (F32, BF16):
        d = _dn(dt)
        pano = [c for c in PANO_TABLE if c[0] == dt]
        b['pano register ' + d] = any(pano_is_register(dt, H) for _, V, H in pano)
        b['pano generic by width ' + d] = any(not pano_is_register(dt, H) and H % _epc(dt) == 0 for _, V, H in pano)
        b['pano generic by chunk ' + d] = any(not pano_is_register(dt, H) and H % _epc(dt) for _, V, H in pano)
        b['pano register limit ' + d] = any(pano_is_register(dt, H) and not pano_is_register(dt, H + _epc(dt)) for _, V, H in pano)
        for V in (1, 8, 9, 63, 64):
            b['pano register V=%d %s' % (V, d)] = any(v == V and pano_is_register(dt, H) for _, v, H in pano)
        sk = [c for c in SK_TABLE if c[0] == dt]
        for kp in ((8, 16) if dt == BF16 else (4, 8, 12, 16)):
            for rpb in (32, 128):
                b['smallk KP %d SK_ROWS %d %s' % (kp, rpb, d)] = any(sk_kp(dt, c[1]) == kp and sk_rows_per_block(c[2]) == rpb for c in sk)
        b['smallk odd N ' + d] = any(c[3] % 2 for c in sk)
        b['smallk N %% 128 ' + d] = any(c[3] % 128 for c in sk)
        b['smallk dead rows in the last batch ' + d] = all(any(c[2] % 8 and sk_rows_per_block(c[2]) == rpb for c in sk) for rpb in (32, 128))
        b['smallk no dbias ' + d] = any(not c[4] for c in sk)
        b['smallk ld_dw > K ' + d] = any(c[5] for c in sk)
        b['smallk ld_x > kp ' + d] = any(c[6] for c in sk)
        emb = [c for c in EMB_BWD_TABLE if c[0] == dt]
        for br in ('small', 'atomic', 'atomic-capped'):
            b['embed backward %s %s' % (br, d)] = any(emb_bwd_branch(c[1], c[2]) == br for c in emb)
        b['embed backward small at 64 rows ' + d] = any(emb_bwd_branch(c[1], c[2]) == 'small' and emb_bwd_branch(c[1] + 1, c[2]) == 'atomic' for c in emb)
        b['embed backward small at 512 tokens ' + d] = any(emb_bwd_branch(c[1], c[2]) == 'small' and emb_bwd_branch(c[1], c[2] - 1) == 'atomic' for c in emb)
        b['embed backward atomic at 511 tokens ' + d] = any(emb_bwd_branch(c[1], c[2]) == 'atomic' and emb_bwd_branch(c[1], c[2] + 1) == 'small' for c in emb)
        b['embed backward rows %% 256 ' + d] = any(emb_bwd_branch(c[1], c[2]) == 'small' and c[2] % 256 for c in emb)
        b['embed backward H %% 64 ' + d] = any(emb_bwd_branch(c[1], c[2]) == 'small' and c[3] % 64 for c in emb)
        b['gather uncapped ' + d] = any(c[0] == dt and not gather_is_capped(dt, len(_gather_segs(c[2])), c[1]) for c in GATHER_TABLE)
        for capped in (False, True):
            b['door backward capped=%d %s' % (capped, d)] = any(c[0] == dt and door_bwd_is_capped(c[1]) == capped for c in DOOR_TABLE)
            b['rowdot backward capped=%d %s' % (capped, d)] = any(c[0] == dt and rowdot_bwd_is_capped(c[1]) == capped for c in ROWDOT_TABLE)
            b['pool backward wide=%d %s' % (capped, d)] = any(c[0] == dt and pool_bwd_is_wide(c[1]) == capped for c in POOL_TABLE)
        b['pool backward at the switch ' + d] = {256, 257} <= {c[1] for c in POOL_TABLE if c[0] == dt}
        b['door DOOR_MAXC full ' + d] = any(c[0] == dt and c[2] == 64 * 16 for c in DOOR_TABLE)
        b['rowdot MAXC full ' + d] = any(c[0] == dt and c[2] == 1024 for c in ROWDOT_TABLE)
        b['colsum one row strip ' + d] = any(c[0] == dt and colsum_grid(c[1], c[2])[1] == 1 for c in COLSUM_TABLE)
        b['colsum several row strips ' + d] = any(c[0] == dt and colsum_grid(c[1], c[2])[1] > 1 for c in COLSUM_TABLE)
        b['colsum ld > C ' + d] = any(c[0] == dt and c[3] > c[2] for c in COLSUM_TABLE)
    b['gather capped f32'] = any(gather_is_capped(c[0], len(_gather_segs(c[2])), c[1]) for c in GATHER_TABLE)
    b['infonce second softmax trip'] = any(c[1] > 64 for c in NCE_TABLE)
    b['infonce one trip'] = any(c[1] <= 64 for c in NCE_TABLE)
    b['infonce backward tail tile'] = any(c[3] % 64 for c in NCE_TABLE)
    b['infonce forward second 256-float trip'] = any(c[3] > 256 for c in NCE_TABLE)
    b['infonce one rank'] = any(c[4] == 'one' for c in NCE_TABLE)
    b['infonce target offset'] = any(c[2] > 0 for c in NCE_TABLE)
    return b


def test_tables_reach_every_dispatch_branch():
    missing = [k for k, v in branches().items() if not v]
    assert not missing, missing


if __name__ == '__main__':
    if sys.argv[1:] == ['--check-inputs']:
        print('%d cases: the reference conditions hold' % check_all_inputs(verbose=True))
        missing = [k for k, v in branches().items() if not v]
        print('branches not reached: %s' % (missing or 'none'))
        sys.exit(1 if missing else 0)
    sys.exit('usage: python tests/test_small_kernels_gpu.py --check-inputs')
