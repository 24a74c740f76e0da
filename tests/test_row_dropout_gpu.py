"""The training-mode dropout paths of csrc/dropout_act.hip and csrc/layernorm.hip (outside attention) — goat_dropout_add_fwd / goat_dropout_bwd, goat_act_bwd (and
hipops.ffn with p > 0 on top of them), goat_ln_fwd_do / goat_ln_bwd_do in their generic forms and the bf16 768-wide backward — against
float64 references on the upcast operands whose dropout masks come from helpers.flat_keep_mask, the host restatement of
GoatRng::keep(offset + i, goat_thr16(p)).  No reference is built from anything a kernel wrote: a mask that forward and backward get
wrong in the same way (a wrong counter in a partial chunk group, offset_out taken for offset, a lost high counter word) fails here.

Counter layout through hipops: after ops.manual_seed(S) the first dropout range starts at counter 0, the next at the previous numel
rounded up to 8; hipops.layer_norm draws the input mask (p) first, then the output mask (p_out).

Values: test_hip_ops._close (max error / max reference below 1e-3 float32, 2e-2 bf16); the direct dropout calls are held elementwise to
one storage rounding over two float32 operations.  Zero patterns are compared at EVERY position; that a kept position cannot read as
zero is asserted on the reference (|ref| >= 1e-6 max |ref| at every kept position — the generator seeds were chosen so that it holds).
Every figure is printed (`FIG group dtype tensor value`) before it is asserted."""
import ctypes
import functools
import math

import pytest
import torch

from helpers import flat_keep_mask
from test_hip_ops import _close

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SEED = 1234
BF16, F32 = torch.bfloat16, torch.float32
GOAT_E_SHAPE = -2
BIG = 2 ** 33 + 8            # a counter whose pair index no longer fits 32 bits: GoatRng::pair_bits adds its __umul24 term from here on


def _dn(dtype):
    return 'bf16' if dtype == BF16 else 'f32'


@pytest.fixture(scope='module')
def ops():
    from vln_goat_amd import hipops
    return hipops


@pytest.fixture()
def rng_state(ops):
    """the process-wide dropout counter state, put back after the test"""
    saved = (ops.RngState.seed, ops.RngState.base, ops.RngState.counter, ops.RngState.dev)
    ops.RngState.dev = None
    yield ops.RngState
    ops.RngState.seed, ops.RngState.base, ops.RngState.counter, ops.RngState.dev = saved


def host_keep(seed, offset, n, p, shape=None):
    """CPU bool tensor of the documented keep bits of counters offset .. offset + n - 1 (all True for p == 0: the kernels draw nothing)"""
    k = torch.ones(n, dtype=torch.bool) if p == 0 else torch.from_numpy(flat_keep_mask(seed, offset, n, p))
    return k.view(shape) if shape is not None else k


def p32(p):
    """the probability as the kernels receive it (a C float)"""
    return float(torch.tensor(p, dtype=torch.float32))


def assert_kept_not_tiny(ref, keep, what):
    """a kept position must not be able to read as zero: |ref| >= 1e-6 max |ref| wherever the mask keeps"""
    a = ref.abs()
    assert bool((a[keep] >= 1e-6 * a.max()).all()), '%s: a kept reference value is below 1e-6 of the largest (choose another generator seed)' % what


def fig(group, dtype, name, got, ref):
    err = float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-6))
    print('FIG %s %s %s %.3e' % (group, _dn(dtype), name, err))
    return err


def check_close(group, dtype, pairs, what):
    """every (name, got, float64 reference) by test_hip_ops._close; the figures are printed first, every miss is reported"""
    misses = []
    for name, g, r in pairs:
        assert (g is None) == (r is None), (what, name)
        if g is None:
            continue
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        assert bool(torch.isfinite(g).all()), '%s %s: not finite' % (what, name)
        fig(group, dtype, name, g, r)
        try:
            _close(g, r, dtype, '%s %s' % (what, name))
        except AssertionError as ex:
            misses.append(str(ex).splitlines()[0])
    assert not misses, misses


def check_zero_pattern(got, keep, what):
    """got == 0 exactly where the host mask drops and nowhere else"""
    bad = (got.cpu() == 0) != ~keep
    assert not bool(bad.any()), '%s: zeros differ from the documented mask at %d of %d positions, first %s' % (
        what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())


# ================================================================================================ a. goat_dropout_add_fwd / goat_dropout_bwd
PAD = 16       # sentinel elements behind every output: a vector store past n would land there


def _launch_dropout(ops, bwd, x, res, alias, p, seed, offset, dev):
    """one direct launch -> (result [n], the PAD elements behind it).  alias: the result overwrites x's own buffer."""
    n = x.numel()
    buf = torch.full((n + PAD,), 7.0, dtype=x.dtype, device=DEV)
    if alias:
        buf[:n] = x
        src = buf[:n]
    else:
        src = x
    y = buf[:n]
    dt = ops._dt(x)
    if bwd:
        ops.launch('goat_dropout_bwd', dt, src, y, n, p, seed, offset, dev)
    else:
        ops.launch('goat_dropout_add_fwd', dt, src, res, y, n, p, seed, offset, dev)
    torch.cuda.synchronize()
    return buf[:n].cpu(), buf[n:].cpu()


def _dropout_ref(x, res, keep, p):
    ref = x.double() * keep / (1.0 - p32(p))
    return ref + res.double() if res is not None else ref


def _check_dropout(dtype, got, tail, x, res, keep, p, what):
    """elementwise |got - ref| <= u |ref| + 2^-22 (|x| / (1 - p) + |res|), u = 2^-8 (bf16) / 2^-23 (float32): one storage rounding over
    at most two float32 operations (scale, add; possibly contracted).  Without a residual also the exact zero pattern."""
    assert bool((tail == 7.0).all()), '%s: wrote behind the end of the tensor' % what
    ref = _dropout_ref(x, res, keep, p)
    u = 2.0 ** -8 if dtype == BF16 else 2.0 ** -23
    bound = u * ref.abs() + 2.0 ** -22 * (x.double().abs() / (1.0 - p32(p)) + (res.double().abs() if res is not None else 0.0))
    over = (got.double() - ref).abs() - bound
    rel = float(((got.double() - ref).abs() / ref.abs().max().clamp_min(1e-6)).max())
    print('FIG dropout %s %s %.3e' % (_dn(dtype), 'y' if res is not None else 'y_nores', rel))
    assert not bool((over > 0).any()), '%s: %d of %d elements exceed the rounding bound, worst by %.3e at %d' % (
        what, int((over > 0).sum()), over.numel(), float(over.max()), int(over.argmax()))
    if res is None:
        assert_kept_not_tiny(ref, keep, what)
        check_zero_pattern(got, keep, what)


DROP_N = (1, 3, 7, 8, 9, 4099)
DROP_OFFSETS = (0, 8 * 5, 8 * 5 + 3, BIG)      # 0, 8 k, 8 k + 3 (the odd path of keep_bits), past 2^33


@pytest.mark.parametrize('offset', DROP_OFFSETS, ids=['off0', 'off8k', 'off8k+3', 'off2^33+8'])
@pytest.mark.parametrize('n', DROP_N)
@pytest.mark.parametrize('dtype', [F32, BF16], ids=_dn)
def test_dropout_direct_every_tail_offset_and_alias(ops, dtype, n, offset):
    """forward with and without residual, with and without y aliasing x, p in {0, 0.1}; the backward kernel, out of place and in place.
    n < 8 (bf16) / 4 (float32) runs the scalar tail alone, 9 and 4099 one resp. many vector chunks plus a tail."""
    g = torch.Generator().manual_seed(100 + n)
    x = torch.randn(n, generator=g).to(dtype)
    res = torch.randn(n, generator=g).to(dtype)
    xd, rd = x.to(DEV), res.to(DEV)
    for p in (0.0, 0.1):
        keep = host_keep(SEED, offset, n, p)
        for with_res in (False, True):
            for alias in (False, True):
                what = 'dropout fwd %s n=%d off=%d p=%g res=%d alias=%d' % (_dn(dtype), n, offset, p, with_res, alias)
                got, tail = _launch_dropout(ops, False, xd, rd if with_res else None, alias, p, SEED, offset, None)
                _check_dropout(dtype, got, tail, x, res if with_res else None, keep, p, what)
        for alias in (False, True):
            got, tail = _launch_dropout(ops, True, xd, None, alias, p, SEED, offset, None)
            _check_dropout(dtype, got, tail, x, None, keep, p, 'dropout bwd %s n=%d off=%d p=%g alias=%d' % (_dn(dtype), n, offset, p, alias))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=_dn)
def test_dropout_direct_device_counter_is_added_to_the_seed(ops, dtype):
    """a non-NULL rng_dev holding 5 == seed + 5 with NULL, forward and backward; both are the host mask of seed + 5"""
    n, p, offset = 4099, 0.1, 8 * 5
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, generator=g).to(dtype)
    xd = x.to(DEV)
    dev = torch.tensor([5], dtype=torch.int64, device=DEV)
    keep = host_keep(SEED + 5, offset, n, p)
    assert not torch.equal(keep, host_keep(SEED, offset, n, p))
    for bwd in (False, True):
        with_dev, t1 = _launch_dropout(ops, bwd, xd, None, False, p, SEED, offset, dev)
        plain, t2 = _launch_dropout(ops, bwd, xd, None, False, p, SEED + 5, offset, None)
        _check_dropout(dtype, with_dev, t1, x, None, keep, p, 'dropout rng_dev bwd=%d' % bwd)
        _check_dropout(dtype, plain, t2, x, None, keep, p, 'dropout seed + 5 bwd=%d' % bwd)
        assert torch.equal(with_dev, plain)
    assert int(dev.item()) == 5


BIG_N = 2048 * 256 * 8 + 8 * 300 + 5        # bf16: the grid caps at 2048 blocks of 256 threads of 8 elements; 300 chunks of a second trip, then a tail of 5
BIG_WIN = 65536


def _big_windows():
    # (the tensor ends 2405 elements into the second trip: the middle window ends 2048 elements into it and overlaps the last one)
    return (0, 2048 * 256 * 8 + 2048 - BIG_WIN, BIG_N - BIG_WIN)


def _big_case():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(BIG_N, generator=g).to(BF16)
    res = torch.randn(BIG_N, generator=g).to(BF16)
    # counter 2^33 falls 1000 elements in front of the start of the second grid-stride trip, inside the middle window
    offset = 2 ** 33 - 2048 * 256 * 8 + 1000
    return x, res, offset


def test_dropout_direct_second_grid_stride_trip_and_tail(ops):
    """bf16, n = 2048 * 256 * 8 + 8 * 300 + 5: three 64 Ki-element windows (start, around the first element of the second trip, end with
    the scalar tail) against host masks made per window through flat_keep_mask(s, o, n, p)[k:] == flat_keep_mask(s, o + k, n - k, p)."""
    x, res, offset = _big_case()
    assert offset % 8 == 0
    p = 0.1
    xd, rd = x.to(DEV), res.to(DEV)
    for with_res, alias in ((False, False), (True, True)):
        got, tail = _launch_dropout(ops, False, xd, rd if with_res else None, alias, p, SEED, offset, None)
        for w0 in _big_windows():
            sl = slice(w0, w0 + BIG_WIN)
            keep = host_keep(SEED, offset + w0, BIG_WIN, p)
            _check_dropout(BF16, got[sl], tail, x[sl], res[sl] if with_res else None, keep, p, 'dropout big window %d res=%d' % (w0, with_res))


# ================================================================================================ b. goat_act_bwd
def _dact(u, act):
    if act == 'relu':
        return (u > 0).double()
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


ACT_OFFSETS = {5: 8 * 5 + 3, 4099: BIG}


@pytest.mark.parametrize('n', [5, 4099])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('act', ['gelu', 'relu'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=_dn)
def test_act_bwd_direct(ops, dtype, act, p, n):
    """dx = dy keep / (1 - p) act'(u) with the erf-GELU derivative in float64; exact zeros at every dropped position (and, for relu,
    wherever u <= 0).  n = 5 is the scalar tail alone (at an odd offset), 4099 vector chunks plus a tail at a counter past 2^33."""
    offset = ACT_OFFSETS[n]
    g = torch.Generator().manual_seed(200 + n)
    dy = torch.randn(n, generator=g).to(dtype)
    u = torch.randn(n, generator=g).to(dtype)
    keep = host_keep(SEED, offset, n, p)
    got = ops.act_bwd(dy.to(DEV), u.to(DEV), act, p, (SEED, offset, None))
    torch.cuda.synchronize()
    ref = dy.double() * keep / (1.0 - p32(p)) * _dact(u.double(), act)
    what = 'act_bwd %s %s p=%g n=%d' % (_dn(dtype), act, p, n)
    check_close('act_bwd', dtype, [('dx', got, ref)], what)
    zero = ~keep | ((u <= 0) if act == 'relu' else torch.zeros(n, dtype=torch.bool))
    assert bool((got.cpu()[zero] == 0).all()), '%s: %d non-zero values at dropped positions' % (what, int((got.cpu()[zero] != 0).sum()))
    if act == 'relu':
        assert_kept_not_tiny(ref, ~zero, what)
        check_zero_pattern(got, ~zero, what)


# ================================================================================================ c. hipops.ffn with dropout
@pytest.mark.parametrize('act', ['gelu', 'relu'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=_dn)
def test_ffn_with_dropout_autograd(ops, rng_state, dtype, act):
    """the panorama encoder FFN: in-place dropout on h = act(x W1^T + b1), then mask times act' in one kernel on the way back — float64
    autograd with the host mask of the [M, F] range at counter 0"""
    M, H, F_, p = 37, 128, 256, 0.1
    g = torch.Generator().manual_seed(23)
    x = torch.randn(M, H, generator=g).to(dtype)
    w1, b1 = torch.randn(F_, H, generator=g) * 0.1, torch.randn(F_, generator=g) * 0.1
    w2, b2 = torch.randn(H, F_, generator=g) * 0.1, torch.randn(H, generator=g) * 0.1
    dy = torch.randn(M, H, generator=g).to(dtype)
    xd = x.to(DEV).requires_grad_(True)
    prm = [torch.nn.Parameter(t.to(DEV)) for t in (w1, b1, w2, b2)]
    ops.manual_seed(SEED)
    y = ops.ffn(xd, prm[0], prm[1], prm[2], prm[3], act, p)
    assert rng_state.counter == M * F_
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    keep = host_keep(SEED, 0, M * F_, p, (M, F_))
    xr = x.double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    wq = [pr[0].to(dtype).double(), pr[2].to(dtype).double()] if dtype == BF16 else [pr[0], pr[2]]      # the kernels see bf16-rounded weights
    pre = xr @ wq[0].T + pr[1]
    h = torch.relu(pre) if act == 'relu' else 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    yr = (h * keep / (1.0 - p32(p))) @ wq[1].T + pr[3]
    yr.backward(dy.double())
    pairs = [('y', y.detach(), yr.detach()), ('dx', xd.grad, xr.grad)]
    pairs += [(n, q.grad, r.grad) for n, q, r in zip(('dw1', 'db1', 'dw2', 'db2'), prm, pr)]
    check_close('ffn', dtype, pairs, 'ffn %s %s' % (_dn(dtype), act))


# ================================================================================================ d. hipops.layer_norm
LN_P, LN_P_OUT, LN_EPS = 0.2, 0.25, 1e-12
# form -> what hipops.layer_norm is given; `outs` = autograd outputs that receive an upstream gradient
FORMS = {
    'plain': dict(),
    'res_p': dict(res=True, p=LN_P),
    'res_p_fork': dict(res=True, p=LN_P, fork=True),
    'zout_p': dict(res=True, p=LN_P, z_out=True),
    'fork_in': dict(fork_in=True),
    'p_out': dict(p_out=LN_P_OUT),
    'p_out_post': dict(p_out=LN_P_OUT, post=True),
    'res_p_p_out': dict(res=True, p=LN_P, p_out=LN_P_OUT),
}
# every register shape of the dispatch (MAXC 1, 2, 3, 4, 8 at 64 chunks of 8 bf16 / 4 float32 elements per MAXC), widths whose last
# 64-chunk group is partial (520 bf16, 264 float32, 1032), the one-row-in-flight form (MAXC > 3) and, for bf16 4096, the raised
# dynamic-LDS attribute of the backward
# (float32 1024 is MAXC 4 there: 1032 already needs five chunk groups and lands on 8)
WIDTHS = {BF16: (8, 256, 512, 520, 768, 1032, 2048, 4096), F32: (4, 256, 264, 512, 768, 1024, 1032, 2048)}
PARTIAL = {BF16: 520, F32: 264}
ROWS = (1, 5, 9, 37)          # a forward block covers 4 rows, a backward block 8: below one block, a partial second one, several


def _ln_table():
    """(dtype, form, M, H, variant).  variant: 'default' | 'generic' (GOAT_LN_BWD_GENERIC=1: bf16 768 on the generic backward) |
    'deterministic' (hipops.LN_DETERMINISTIC: per-block partials + reduction launch) | 'counter33' (RngState.counter preset to 2^33 + 8)"""
    t = []
    for dt in (BF16, F32):
        for H in WIDTHS[dt]:
            for M in (5, 37):
                for form in ('res_p_fork', 'p_out_post'):
                    t.append((dt, form, M, H, 'default'))
        for form in FORMS:
            for H in (256, PARTIAL[dt], 768):
                t.append((dt, form, 9, H, 'default'))
        for H in (WIDTHS[dt][0], 768, WIDTHS[dt][-1]):
            t.append((dt, 'res_p_p_out', 1, H, 'default'))
            t.append((dt, 'zout_p', 1, H, 'default'))
        t.append((dt, 'res_p_fork', 4101, 256, 'default'))         # M > LN_ATOMIC_MAX_ROWS: workspace path; the grid caps at 512 blocks, the row loop wraps
        t.append((dt, 'res_p_p_out', 9, 768, 'deterministic'))
        t.append((dt, 'zout_p', 1, PARTIAL[dt], 'deterministic'))
        t.append((dt, 'res_p_p_out', 9, PARTIAL[dt], 'counter33'))
        t.append((dt, 'zout_p', 37, 768, 'counter33'))
    t += [(dt, form, M, H, 'generic') for dt, form, M, H, v in list(t) if dt == BF16 and H == 768 and v in ('default', 'counter33')]
    return t


LN_TABLE = _ln_table()


def check_ln_table(table=None):
    """table-level coverage the issue asks for (also run without a GPU by test_dropout_mask_host.py)"""
    table = LN_TABLE if table is None else table
    assert len(set(table)) == len(table)
    have = set(table)
    for dt in (BF16, F32):
        for H in WIDTHS[dt]:
            for M in (5, 37):
                for form in ('res_p_fork', 'p_out_post'):
                    assert (dt, form, M, H, 'default') in have, (dt, form, M, H)
        for form in FORMS:
            for H in (256, PARTIAL[dt], 768):
                assert (dt, form, 9, H, 'default') in have, (dt, form, H)
        assert {M for d, f, M, H, v in table if d == dt} >= set(ROWS)
        assert {H for d, f, M, H, v in table if d == dt} == set(WIDTHS[dt])
        assert any(d == dt and M > 4096 and H == 256 for d, f, M, H, v in table)
        assert any(d == dt and (M, H, v) == (9, 768, 'deterministic') for d, f, M, H, v in table)
        assert any(d == dt and v == 'counter33' for d, f, M, H, v in table)
        # MAXC 1, 2, 3, 4, 8 of csrc/layernorm.hip's ln_maxc
        epc = 8 if dt == BF16 else 4
        maxc = {min(m for m in (1, 2, 3, 4, 8) if m >= (H // epc + 63) // 64) for H in WIDTHS[dt]}
        assert maxc == {1, 2, 3, 4, 8}, maxc
    # every bf16 768 case of the default build runs on the generic backward as well
    d768 = {(f, M) for d, f, M, H, v in table if d == BF16 and H == 768 and v == 'default'}
    g768 = {(f, M) for d, f, M, H, v in table if d == BF16 and H == 768 and v == 'generic'}
    assert d768 <= g768 and {f for f, M in d768} == set(FORMS)


def _ln_id(c):
    dt, form, M, H, variant = c
    return '%s-%s-%dx%d-%s' % (_dn(dt), form, M, H, variant)


# generator seeds moved on until every kept reference value of the case stands clear of zero (ln_reference_conditions)
LN_SEED_BUMP = {('bf16', 'p_out_post', 37, 2048): 1, ('bf16', 'res_p_fork', 4101, 256): 9, ('f32', 'res_p_fork', 37, 1032): 1,
                ('f32', 'res_p_fork', 4101, 256): 6, ('f32', 'zout_p', 37, 768): 1}


def _ln_seed(dt, form, M, H):
    return 10007 * H + 101 * M + 10 * list(FORMS).index(form) + (1 if dt == BF16 else 0) + 1000003 * LN_SEED_BUMP.get((_dn(dt), form, M, H), 0)


def _r8(n):
    return (n + 7) & ~7


@functools.lru_cache(maxsize=None)
def ln_case(dt, form, M, H, counter0=0):
    """operands (CPU, in the storage dtype) and float64 references of one case: computed once, shared by the variants that run it"""
    f = FORMS[form]
    p, p_out = f.get('p', 0.0), f.get('p_out', 0.0)
    g = torch.Generator().manual_seed(_ln_seed(dt, form, M, H))
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(x=rn(M, H).to(dt), gamma=1 + 0.1 * rn(H), beta=0.1 * rn(H), d1=rn(M, H).to(dt), d2=rn(M, H).to(dt))
    c['res'] = rn(M, H).to(dt) if f.get('res') else None
    c['post'] = (2 + rn(M, H)).to(dt) if f.get('post') else None
    off = counter0
    c['keep_in'] = host_keep(SEED, off, M * H, p, (M, H))
    off += _r8(M * H) if p > 0 else 0
    c['keep_out'] = host_keep(SEED, off, M * H, p_out, (M, H))
    c['counter_end'] = off + (_r8(M * H) if p_out > 0 else 0)
    x = c['x'].double().requires_grad_(True)
    gamma, beta = c['gamma'].double().requires_grad_(True), c['beta'].double().requires_grad_(True)
    res = c['res'].double().requires_grad_(True) if c['res'] is not None else None
    post = c['post'].double().requires_grad_(True) if c['post'] is not None else None
    z = x * c['keep_in'] / (1.0 - p32(p))
    if res is not None:
        z = z + res
    yn = torch.nn.functional.layer_norm(z, (H,), gamma, beta, LN_EPS)
    if post is not None:
        yn = yn + post
    y = yn * c['keep_out'] / (1.0 - p32(p_out))
    d1, d2 = c['d1'].double(), c['d2'].double()
    if f.get('fork'):
        y.backward(d1 + d2)
    elif f.get('z_out'):
        torch.autograd.backward([y, z], [d1, d2])
    elif f.get('fork_in'):
        torch.autograd.backward([y, x * 1.0], [d1, d2])
    else:
        y.backward(d1)
    c['ref'] = dict(y=y.detach(), z=z.detach() if f.get('z_out') else None, dx=x.grad, dres=res.grad if res is not None else None,
                    dgamma=gamma.grad, dbeta=beta.grad, dpost=post.grad if post is not None else None)
    return c


def ln_run(ops, dt, form, c, gamma=None, beta=None):
    """the production call and its backward -> the tensors named as the reference names them"""
    f = FORMS[form]
    x = c['x'].to(DEV).requires_grad_(True)
    gamma = c['gamma'].to(DEV).requires_grad_(True) if gamma is None else gamma
    beta = c['beta'].to(DEV).requires_grad_(True) if beta is None else beta
    res = c['res'].to(DEV).requires_grad_(True) if c['res'] is not None else None
    post = c['post'].to(DEV).requires_grad_(True) if c['post'] is not None else None
    out = ops.layer_norm(x, gamma, beta, LN_EPS, residual=res, p=f.get('p', 0.0), fork=f.get('fork', False), fork_in=f.get('fork_in', False),
                         z_out=f.get('z_out', False), p_out=f.get('p_out', 0.0), post_add=post)
    outs = list(out) if isinstance(out, tuple) else [out]
    torch.autograd.backward(outs, [c['d1'].to(DEV), c['d2'].to(DEV)][:len(outs)])
    torch.cuda.synchronize()
    return dict(y=outs[0].detach(), z=outs[1].detach() if f.get('z_out') else None, dx=x.grad, dres=res.grad if res is not None else None,
                dgamma=gamma.grad, dbeta=beta.grad, dpost=post.grad if post is not None else None)


LN_NAMES = ('y', 'z', 'dx', 'dres', 'dgamma', 'dbeta', 'dpost')


def ln_reference_conditions(dt, form, M, H, c):
    """what the zero-pattern checks rest on, on the references alone (no GPU)"""
    f, what = FORMS[form], _ln_id((dt, form, M, H, 'ref'))
    if f.get('p', 0.0) > 0:
        assert_kept_not_tiny(c['ref']['dx'], c['keep_in'], what + ' dx')
    if f.get('p_out', 0.0) > 0:
        assert_kept_not_tiny(c['ref']['y'], c['keep_out'], what + ' y')


def ln_check(dt, form, M, H, c, got, what, skip=()):
    ln_reference_conditions(dt, form, M, H, c)
    f = FORMS[form]
    misses = []
    try:
        check_close('layer_norm', dt, [(n, got[n], c['ref'][n]) for n in LN_NAMES if n not in skip], what)
    except AssertionError as ex:
        misses.append(str(ex))
    # the input mask: dx is zero exactly at its dropped positions (no form with p > 0 joins a skip gradient behind the dropout split:
    # z_out's second gradient joins in FRONT of it)
    if f.get('p', 0.0) > 0:
        try:
            check_zero_pattern(got['dx'], c['keep_in'], what + ' dx against the input mask')
        except AssertionError as ex:
            misses.append(str(ex))
    if f.get('p_out', 0.0) > 0:
        try:
            check_zero_pattern(got['y'], c['keep_out'], what + ' y against the output mask')
        except AssertionError as ex:
            misses.append(str(ex))
    assert not misses, misses


@pytest.mark.parametrize('case', LN_TABLE, ids=[_ln_id(c) for c in LN_TABLE])
def test_layer_norm_forms_widths_rows(ops, rng_state, monkeypatch, case):
    dt, form, M, H, variant = case
    counter0 = BIG if variant == 'counter33' else 0
    if variant == 'generic':
        monkeypatch.setenv('GOAT_LN_BWD_GENERIC', '1')
        # the same operands and reference as the default run; a counter33 case keeps its counter
        counter0 = BIG if (dt, form, M, H, 'counter33') in LN_TABLE else 0
    else:
        monkeypatch.delenv('GOAT_LN_BWD_GENERIC', raising=False)
    if variant == 'deterministic':
        monkeypatch.setattr(ops, 'LN_DETERMINISTIC', True)
    else:
        assert not ops.LN_DETERMINISTIC
        assert (M > ops.LN_ATOMIC_MAX_ROWS) == (M == 4101)
    c = ln_case(dt, form, M, H, counter0)
    ops.manual_seed(SEED)
    rng_state.counter = counter0
    assert rng_state.seed == SEED and rng_state.dev is None
    got = ln_run(ops, dt, form, c)
    assert rng_state.counter == c['counter_end']
    ln_check(dt, form, M, H, c, got, _ln_id(case))


def test_ln_table_covers_every_width_and_form():
    check_ln_table()


@pytest.mark.parametrize('deferred', [False, True], ids=['accumulate', 'deferred'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=_dn)
def test_layer_norm_sunk_gamma_beta_add_onto_a_nonzero_base(ops, rng_state, monkeypatch, dtype, deferred):
    """gamma / beta bound to pre-zeroed gradient-arena slices that already hold another writer's sum: the backward accumulates onto it —
    with float atomics at this row count, and (LnReduceQueue.MIN_ROWS lowered) by leaving column partials for the one batched reduction
    at the end of the backward pass."""
    form, M, H = 'res_p_fork', 37, 512
    c = ln_case(dtype, form, M, H)
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(H, generator=g), torch.randn(H, generator=g)]
    gamma, beta = c['gamma'].to(DEV).requires_grad_(True), c['beta'].to(DEV).requires_grad_(True)
    sinks = [b.to(DEV) for b in base]
    for prm, snk in zip((gamma, beta), sinks):
        prm.grad = snk
        prm.__dict__['_goat_sink'] = snk
        prm.__dict__['_goat_prezero'] = True
    assert ops.LnReduceQueue.enabled and M < ops.LnReduceQueue.MIN_ROWS
    if deferred:
        monkeypatch.setattr(ops.LnReduceQueue, 'MIN_ROWS', 1)
    ops.manual_seed(SEED)
    try:
        got = ln_run(ops, dtype, form, c, gamma, beta)
        assert not ops.LnReduceQueue.items            # flushed by the end-of-backward callback
        torch.cuda.synchronize()
    finally:
        for prm in (gamma, beta):
            prm.__dict__.pop('_goat_sink', None)
            prm.__dict__.pop('_goat_prezero', None)
    assert gamma.grad is sinks[0] and beta.grad is sinks[1]
    what = 'layer_norm sunk %s %s' % (_dn(dtype), 'deferred' if deferred else 'accumulate')
    ln_check(dtype, form, M, H, c, got, what, skip=('dgamma', 'dbeta'))
    added = [('dgamma', sinks[0].double().cpu() - base[0].double(), c['ref']['dgamma']), ('dbeta', sinks[1].double().cpu() - base[1].double(), c['ref']['dbeta'])]
    check_close('layer_norm', dtype, added, what + ' (sink - base)')


# ================================================================================================ e. entry checks
@pytest.mark.parametrize('dtype,H', [(BF16, 12), (F32, 6), (BF16, 4104), (F32, 2052)], ids=['bf16-12', 'f32-6', 'bf16-4104', 'f32-2052'])
def test_layer_norm_entry_points_refuse_widths_they_cannot_serve(ops, dtype, H):
    """H not a multiple of the 16-byte chunk, or beyond 64 * 8 chunks: GOAT_E_SHAPE from both directions and nothing written"""
    from vln_goat_amd import _lib
    M = 2
    lib, st, dt = _lib.lib(), torch.cuda.current_stream().cuda_stream, ops._dt(torch.empty(0, dtype=dtype))
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    x = torch.ones(M, H, dtype=dtype, device=DEV)
    gamma, beta = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    outs = [torch.full((M, H), 7.0, dtype=dtype, device=DEV) for _ in range(2)]
    stats = [torch.full((M,), 7.0, device=DEV) for _ in range(2)]
    grads = [torch.full((H,), 7.0, device=DEV) for _ in range(2)]
    assert lib.goat_ln_fwd_do(st, dt, vp(x), None, vp(gamma), vp(beta), 1e-5, 0.0, 0, 0, None, vp(outs[0]), vp(outs[1]), vp(stats[0]), vp(stats[1]),
                              M, H, 0.0, 0, None) == GOAT_E_SHAPE
    assert lib.goat_ln_bwd_do(st, dt, vp(x), None, vp(x), vp(gamma), vp(gamma[:M]), vp(gamma[:M]), 0.0, 0, 0, None, vp(outs[0]), vp(outs[1]),
                              vp(grads[0]), vp(grads[1]), None, M, H, 0, None, 0.0, 0, None) == GOAT_E_SHAPE
    torch.cuda.synchronize()
    for t in outs + stats + grads:
        assert bool((t == 7.0).all()), 'an entry point that returned GOAT_E_SHAPE wrote to one of its outputs'
