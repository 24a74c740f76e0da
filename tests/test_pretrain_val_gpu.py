"""goat_val_rows / goat_val_cfp / goat_val_reduce (csrc/valstats.hip), pretrain_eval.ValStats and the validate_* loops on the device.

Kernel cases: float64 numpy references built from the float32 operands as the kernel receives them; nothing a kernel wrote enters a
reference.  Hits and row counts are compared for equality.  A loss sum is bounded by test_hip_ops._tol(float32) = 1e-3 times
sum_rows max(|logsumexp64|, |x_label|, 1); a single row_loss by the same figure times its own row's scale.  Row scale of the forms without
a label logit: soft rows use sum_n t_n |x_n| (the expectation the loss subtracts) in the place of |x_label|; a CFP row is the mean of its
two cross-entropies, so its scale is the mean of their two scales.  As condition c. of tests/test_small_kernels_gpu.py requires, the same
formula in float32 torch on the CPU must sit within a quarter of the bound; for CFP the top two image-to-text scores of every row of a
random case must be at least 1e-3 x the row's largest |score| apart, so that no hit depends on float32 rounding: the seed is moved on
until both hold (conditioned_cfp), and both are asserted before anything runs on the device.

Direct calls: every logit matrix is a view into a NaN-filled buffer (padding columns ld > N and the floats around the matrix are NaN: a
read past a row poisons its loss), every output sits between sentinel pads that must read back unchanged.

Model level: the model's own `compute_loss=False` outputs are recorded while validate_* runs and the reference's formulas are evaluated
on them in float64 torch on the CPU (the forward itself is pinned by tests/test_model_parity_gpu.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import CASES, build_case, case_tasks
from test_hip_ops import _tol

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL = _tol(torch.float32)
PAD = 16
SENT = 7
NAN = float('nan')
NINF = -float('inf')


# ================================================================================================ memory around a direct call
def moat(shape, dtype, fill):
    """-> (buffer, view of `shape` filled with `fill`) on the device, PAD sentinel elements on either side of the view"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device=DEV)
    v = buf[PAD:PAD + n].view(shape)
    v.fill_(fill)
    return buf, v


def pads_intact(*bufs):
    return all(bool((b[:PAD] == SENT).all() and (b[-PAD:] == SENT).all()) for b in bufs)


def nan_matrix(x, ld, off):
    """x float32 CPU [M, N] -> a device view [M, N] with row stride ld, `off` floats past a 16-byte boundary, inside NaN"""
    M, N = x.shape
    buf = torch.full((2 * PAD + off + M * ld,), NAN, dtype=torch.float32, device=DEV)
    v = buf[PAD + off:PAD + off + M * ld].view(M, ld)[:, :N]
    v.copy_(x)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * (off % 4)
    return v


# ================================================================================================ references
def hard_ref(x, labels):
    """x float32 [M, N], labels int64 [M] (CPU tensors) -> float64 per-row loss, bool hit, bool counted, per-row scale"""
    x64, lab = x.double().numpy(), labels.numpy()
    M, N = x64.shape
    with np.errstate(all='ignore'):
        m = x64.max(1)
        lse = m + np.log(np.exp(x64 - m[:, None]).sum(1))
    counted = lab >= 0
    inrange = counted & (lab < N)
    xl = np.where(inrange, x64[np.arange(M), np.clip(lab, 0, N - 1)], NAN)
    loss = np.where(counted, lse - xl, 0.0)
    am = np.where(np.isnan(x64).any(1), -1, np.argmax(np.where(np.isnan(x64), NINF, x64), 1))      # numpy: the first of the maxima
    hit = inrange & (am == lab)
    scale = np.where(counted, np.maximum(np.maximum(np.abs(lse), np.abs(xl)), 1.0), 0.0)
    return loss, hit, counted, scale


def hard_f32(x, labels):
    """the same formula in float32 torch on the CPU, summed over the counted rows"""
    keep = labels >= 0
    xs, ls = x[keep], labels[keep]
    return float((torch.logsumexp(xs, 1) - xs.gather(1, ls[:, None]).squeeze(1)).sum())


def soft_ref(x, t):
    x64, t64 = x.double().numpy(), t.double().numpy()
    m = x64.max(1)
    lse = m + np.log(np.exp(x64 - m[:, None]).sum(1))
    with np.errstate(all='ignore'):
        terms = np.where(t64 > 0, t64 * (np.log(t64) - (x64 - lse[:, None])), 0.0)
    loss = terms.sum(1)
    hit = np.argmax(x64, 1) == np.argmax(t64, 1)
    scale = np.maximum(np.maximum(np.abs(lse), (t64 * np.abs(x64)).sum(1)), 1.0)
    return loss, hit, scale


def check_condition_c(f32_sum, ref_sum, bound, what):
    assert abs(f32_sum - ref_sum) <= 0.25 * bound, '%s: float32 on the CPU is %.3e off the float64 sum, a quarter of the bound is %.3e' % (
        what, abs(f32_sum - ref_sum), 0.25 * bound)


def check_rows(what, got_loss, got_hit, loss, hit, scale, miss):
    """per-row outputs: losses within TOL x the row's scale (rows of scale 0 — ignored ones — exactly 0), hits equal"""
    gl, gh = got_loss.cpu().double().numpy(), got_hit.cpu().numpy()
    err = np.abs(gl - loss)
    bad = ~(err <= TOL * scale)
    print('FIG %s row_loss worst error / row scale %.3e' % (what, float(np.max(err / np.maximum(scale, 1e-300) * (scale > 0), initial=0.0))))
    if bad.any():
        miss.append('%s: %d row losses outside the bound, first row %d: %r vs %r' % (what, int(bad.sum()), int(bad.argmax()), gl[bad.argmax()], loss[bad.argmax()]))
    if not (gh == hit.astype(np.int32)).all():
        miss.append('%s: hits differ at rows %s' % (what, np.nonzero(gh != hit.astype(np.int32))[0][:8].tolist()))


def check_sums(what, acc_row, loss_sum, hits, rows, bound, miss):
    a = acc_row.cpu().tolist()
    print('FIG %s loss sum error %.3e bound %.3e' % (what, abs(a[0] - loss_sum), bound))
    if not abs(a[0] - loss_sum) <= bound:
        miss.append('%s: loss sum %r vs %r, bound %.3e' % (what, a[0], loss_sum, bound))
    if a[1] != float(hits) or a[2] != float(rows):
        miss.append('%s: (hits, rows) = (%r, %r), reference (%d, %d)' % (what, a[1], a[2], hits, rows))


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


@pytest.fixture(scope='module')
def ops():
    from vln_goat_amd import hipops
    return hipops


# ================================================================================================ hard rows: shapes
HARD_M = (1, 3, 5, 257)
HARD_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)      # 1024 / 1025: the switch from a wave per row to a block per row


@functools.lru_cache(maxsize=None)
def hard_case(M, N):
    g = _gen(11, M, N)
    x = torch.randn(M, N, generator=g) * 3.0
    labels = torch.randint(0, N, (M,), generator=g)
    lift = torch.rand(M, generator=g) < 0.5                     # about half of the rows are hits
    x[lift, labels[lift]] += 12.0
    loss, hit, counted, scale = hard_ref(x, labels)
    bound = TOL * float(scale.sum())
    check_condition_c(hard_f32(x, labels), float(loss.sum()), bound, 'hard M=%d N=%d' % (M, N))
    return dict(x=x, labels=labels, loss=loss, hit=hit, scale=scale, bound=bound)


def run_hard_direct(ops, c, ld, off, what, miss):
    M, N = c['x'].shape
    xv = nan_matrix(c['x'], ld, off)
    lb, rl = moat((M,), torch.float32, NAN)
    hb, rh = moat((M,), torch.int32, -5)
    ab, acc = moat((3, 3), torch.float64, 5.0)
    acc[1].zero_()
    labels = c['labels'].to(DEV)
    used = ops.val_rows(xv, rl, rh, labels=labels)
    ops.val_reduce(rl, rh, used, acc[1])
    torch.cuda.synchronize()
    if not pads_intact(lb, hb, ab):
        miss.append('%s: a sentinel pad was written' % what)
    if not bool((acc[0] == 5.0).all() and (acc[2] == 5.0).all()):
        miss.append('%s: a neighbouring accumulator slot was written' % what)
    check_rows(what, rl, rh, c['loss'], c['hit'], c['scale'], miss)
    check_sums(what, acc[1], float(c['loss'].sum()), int(c['hit'].sum()), M, c['bound'], miss)


@pytest.mark.parametrize('N', HARD_N)
def test_hard_rows_every_width_stride_and_base(ops, N):
    cases = [hard_case(M, N) for M in HARD_M]                   # (references and their conditions first: CPU only)
    miss = []
    for M, c in zip(HARD_M, cases):
        for ld in (N, N + 3):
            for off in (0, 1):
                run_hard_direct(ops, c, ld, off, 'hard M=%d N=%d ld=%d off=%d' % (M, N, ld, off), miss)
    assert not miss, '\n'.join(miss)


def test_hard_rows_vocabulary_width(ops):
    c = hard_case(3, 50265)
    miss = []
    run_hard_direct(ops, c, 50265, 0, 'hard M=3 N=50265', miss)
    run_hard_direct(ops, c, 50268, 1, 'hard M=3 N=50265 ld=50268 off=1', miss)
    assert not miss, '\n'.join(miss)


# ================================================================================================ hard rows: planted contents
@functools.lru_cache(maxsize=None)
def planted_case(N):
    g = _gen(13, N)
    M = 12
    x = torch.randn(M, N, generator=g) * 2.0
    labels = torch.randint(80, N - 80, (M,), generator=g)
    far = 75 + N // 2
    # rows 0 / 1: an exact tie of the maximum in two distant columns (other lanes, other waves); the lowest index is the label / is not
    x[0, 75] = x[0, far] = 40.0
    labels[0] = 75
    x[1, 75] = x[1, far] = 40.0
    labels[1] = far
    # rows 2 / 3: the tie inside one 16-byte piece
    x[2, 100] = x[2, 102] = 40.0
    labels[2] = 100
    x[3, 100] = x[3, 102] = 40.0
    labels[3] = 102
    # rows 4 / 5: 70 leading / 70 trailing -inf columns (more than a wave's width); row 6 both, and the maximum right behind the stretch
    x[4, :70] = NINF
    x[5, -70:] = NINF
    x[6, :70] = NINF
    x[6, -70:] = NINF
    x[6, 70] = 30.0
    labels[6] = 70
    # rows 7 / 9: ignored (label -1), their logits NaN: an ignored row is not read
    x[7] = NAN
    x[9] = NAN
    labels[7] = labels[9] = -1
    # row 10: every column but one is -inf
    x[10] = NINF
    x[10, 90] = -3.0
    labels[10] = 90
    loss, hit, counted, scale = hard_ref(x, labels)
    assert hit[0] and not hit[1] and hit[2] and not hit[3] and hit[6] and hit[10] and not counted[7] and not counted[9]
    assert np.isfinite(loss).all() and loss[7] == 0.0 and abs(loss[10]) == 0.0
    bound = TOL * float(scale.sum())
    check_condition_c(hard_f32(x, labels), float(loss.sum()), bound, 'planted N=%d' % N)
    return dict(x=x, labels=labels, loss=loss, hit=hit, counted=counted, scale=scale, bound=bound)


@pytest.mark.parametrize('N', [200, 1500])                      # a wave per row; a block per row
def test_hard_rows_ties_masked_stretches_and_ignored_rows(ops, N):
    from vln_goat_amd import pretrain_eval
    c = planted_case(N)
    miss = []
    M = c['x'].shape[0]
    for ld, off in ((N, 0), (N + 3, 1)):
        xv = nan_matrix(c['x'], ld, off)
        lb, rl = moat((M,), torch.float32, NAN)
        hb, rh = moat((M,), torch.int32, -5)
        ab, acc = moat((3,), torch.float64, 0.0)
        used = ops.val_rows(xv, rl, rh, labels=c['labels'].to(DEV))
        ops.val_reduce(rl, rh, used, acc)
        torch.cuda.synchronize()
        what = 'planted N=%d ld=%d off=%d' % (N, ld, off)
        if not pads_intact(lb, hb, ab):
            miss.append('%s: a sentinel pad was written' % what)
        check_rows(what, rl, rh, c['loss'], c['hit'], c['scale'], miss)
        check_sums(what, acc, float(c['loss'].sum()), int(c['hit'].sum()), int(c['counted'].sum()), c['bound'], miss)
    # in slots of their own: an all -inf row, a label >= N, a NaN logit — each a NaN sum; the good slot beside them stays finite
    g = _gen(17, N)
    base = torch.randn(3, N, generator=g)
    lab = torch.tensor([3, 5, 7])
    good = hard_ref(base, lab)
    st = pretrain_eval.ValStats(('good', 'all_inf', 'past', 'nan'), DEV)
    st.add_rows('good', base.to(DEV), labels=lab.to(DEV))
    x = base.clone()
    x[1] = NINF
    st.add_rows('all_inf', x.to(DEV), labels=lab.to(DEV))
    st.add_rows('past', base.to(DEV), labels=torch.tensor([3, N, 7]).to(DEV))
    x = base.clone()
    x[2, N - 2] = NAN
    x[2, 7] = 50.0                                              # (the argmax is the label, and the hit is 0 all the same)
    st.add_rows('nan', x.to(DEV), labels=lab.to(DEV))
    r = st.read()
    if not (abs(r['good'][0] - float(good[0].sum())) <= TOL * float(good[3].sum()) and r['good'][1:] == (float(good[1].sum()), 3.0)):
        miss.append('good slot: %r' % (r['good'],))
    for name, hits in (('all_inf', float(good[1][[0, 2]].sum())), ('past', float(good[1][[0, 2]].sum())), ('nan', float(good[1][[0, 1]].sum()))):
        if not (np.isnan(r[name][0]) and r[name][1] == hits and r[name][2] == 3.0):
            miss.append('%s slot: %r, wanted (nan, %r, 3.0)' % (name, r[name], hits))
    assert not miss, '\n'.join(miss)


# ================================================================================================ soft rows
SOFT_N = (100, 1000, 1001, 1025)                                # 1025: a block per row


@functools.lru_cache(maxsize=None)
def soft_case(N):
    g = _gen(19, N)
    M = 37
    x = torch.randn(M, N, generator=g) * 2.0
    p = torch.rand(M, N, generator=g) ** 4
    p[torch.rand(M, N, generator=g) < 0.3] = 0.0               # exact zeros
    p[:, 0] += 1e-3                                             # (no all-zero row)
    t = (p / p.sum(1, keepdim=True)).float()
    top = t.argmax(1)
    x[torch.arange(M), top] += torch.where(torch.rand(M, generator=g) < 0.5, 12.0, 0.0)      # about half of the rows are hits
    # rows 0 / 1: a tie of the target's maximum in two distant columns; the logits' argmax is the lower / the upper one
    hi = N - 7
    t[0, 5] = t[0, hi] = t[0].max() * 2
    t[1, 5] = t[1, hi] = t[1].max() * 2
    x[0, 5], x[1, hi] = 30.0, 30.0
    assert bool((t == 0).any())
    loss, hit, scale = soft_ref(x, t)
    assert hit[0] and not hit[1]
    bound = TOL * float(scale.sum())
    f32 = float(F.kl_div(F.log_softmax(x, dim=-1), t, reduction='sum'))
    check_condition_c(f32, float(loss.sum()), bound, 'soft N=%d' % N)
    return dict(x=x, t=t, loss=loss, hit=hit, scale=scale, bound=bound)


@pytest.mark.parametrize('N', SOFT_N)
def test_soft_rows(ops, N):
    c = soft_case(N)
    M = c['x'].shape[0]
    miss = []
    for (ld, off), (ldt, offt) in (((N, 0), (N, 0)), ((N + 3, 1), (N + 3, 1)), ((N, 0), (N + 1, 2))):      # the last: rows at different offsets
        xv, tv = nan_matrix(c['x'], ld, off), nan_matrix(c['t'], ldt, offt)
        lb, rl = moat((M,), torch.float32, NAN)
        hb, rh = moat((M,), torch.int32, -5)
        ab, acc = moat((3,), torch.float64, 0.0)
        assert ops.val_rows(xv, rl, rh, soft=tv) is None
        ops.val_reduce(rl, rh, None, acc)
        torch.cuda.synchronize()
        what = 'soft N=%d ld=%d off=%d ldt=%d offt=%d' % (N, ld, off, ldt, offt)
        if not pads_intact(lb, hb, ab):
            miss.append('%s: a sentinel pad was written' % what)
        check_rows(what, rl, rh, c['loss'], c['hit'], c['scale'], miss)
        check_sums(what, acc, float(c['loss'].sum()), int(c['hit'].sum()), M, c['bound'], miss)
    assert not miss, '\n'.join(miss)


# ================================================================================================ accumulation
def test_accumulation_slots_and_bitwise_repeats():
    from vln_goat_amd import pretrain_eval
    a, b = hard_case(257, 257), hard_case(5, 4099)
    s = soft_case(1001)
    st = pretrain_eval.ValStats(('left', 'both', 'right', 'once', 'again', 'soft1', 'soft2'), DEV)
    xa, la = a['x'].to(DEV), a['labels'].to(DEV)
    xb, lb = b['x'].to(DEV), b['labels'].to(DEV)
    st.add_rows('both', xa, labels=la)
    st.add_rows('both', xb, labels=lb)                          # two calls into one slot add up (and the workspace is reused)
    st.add_rows('once', xa, labels=la)
    st.add_rows('again', xa, labels=la)
    xs, ts = s['x'].to(DEV), s['t'].to(DEV)
    st.add_rows('soft1', xs, soft=ts)
    st.add_rows('soft2', xs, soft=ts)
    st.add_rows('both', xa[:0], labels=la[:0])                  # an empty selection launches nothing
    acc = st.acc.cpu()
    r = st.read()
    assert r['left'] == (0.0, 0.0, 0.0) and r['right'] == (0.0, 0.0, 0.0)          # the neighbours of 'both'
    want = float(a['loss'].sum()) + float(b['loss'].sum())
    assert abs(r['both'][0] - want) <= a['bound'] + b['bound']
    assert r['both'][1:] == (float(a['hit'].sum() + b['hit'].sum()), 262.0)
    assert torch.equal(acc[3], acc[4]) and torch.equal(acc[5], acc[6])             # the same call twice: the same bits
    st2 = pretrain_eval.ValStats(('x',), DEV)                   # ... and from a fresh object with a fresh workspace
    st2.add_rows('x', xa, labels=la)
    assert torch.equal(st2.acc.cpu()[0], acc[3])


# ================================================================================================ CFP
CFP_B = (1, 2, 3, 48, 65, 130)
CFP_H = (64, 100, 768)
TAU = 0.5


def cfp_ref(xs, txt, tau):
    """xs: three float32 [B, H], txt float32 [B, H] -> float64 loss [3, B], hit [3, B], scale [3, B], smallest relative top-two gap"""
    B = txt.shape[0]
    t64 = txt.double().numpy()
    loss, hit, scale, gap = np.zeros((3, B)), np.zeros((3, B), bool), np.zeros((3, B)), np.inf
    idx = np.arange(B)
    for k, x in enumerate(xs):
        s = x.double().numpy() @ t64.T / tau
        sc = []
        for sim in (s, s.T):
            m = sim.max(1)
            lse = m + np.log(np.exp(sim - m[:, None]).sum(1))
            loss[k] += 0.5 * (lse - sim[idx, idx])
            sc.append(np.maximum(np.maximum(np.abs(lse), np.abs(sim[idx, idx])), 1.0))
        scale[k] = 0.5 * (sc[0] + sc[1])
        hit[k] = np.argmax(s, 1) == idx
        if B > 1:
            top = np.sort(s, 1)
            gap = min(gap, float(((top[:, -1] - top[:, -2]) / np.abs(s).max(1)).min()))
    return loss, hit, scale, gap


def cfp_f32(xs, txt, tau):
    tgt = torch.arange(txt.shape[0])
    out = []
    for x in xs:
        sim = (x @ txt.T) / tau
        out.append(float((F.cross_entropy(sim, tgt, reduction='sum') + F.cross_entropy(sim.T, tgt, reduction='sum')) / 2.0))
    return out


@functools.lru_cache(maxsize=None)
def conditioned_cfp(B, H):
    """the seed is moved on until the top two image-to-text scores of every row are 1e-3 x the row scale apart and float32 on the CPU
    sits within a quarter of the bound (CPU work on the references only)"""
    why = None
    for bump in range(64):
        g = _gen(23, B, H, bump)
        txt = torch.randn(B, H, generator=g) / H ** 0.25
        xs = []
        for k in range(3):
            x = torch.randn(B, H, generator=g) / H ** 0.25
            pull = (torch.rand(B, 1, generator=g) < 0.6).float()                   # most rows lean towards their own text: hits and misses
            xs.append((x + pull * txt).contiguous())
        loss, hit, scale, gap = cfp_ref(xs, txt, TAU)
        bounds = TOL * scale.sum(1)
        f32 = cfp_f32(xs, txt, TAU)
        if gap < 1e-3:
            why = 'top-two gap %.3e' % gap
            continue
        if any(abs(f32[k] - loss[k].sum()) > 0.25 * bounds[k] for k in range(3)):
            why = 'float32 on the CPU outside a quarter of the bound'
            continue
        return dict(xs=xs, txt=txt, loss=loss, hit=hit, scale=scale, bounds=bounds, gap=gap, bump=bump)
    raise AssertionError('no seed among 64 meets the CFP conditions: %s' % why)


def run_cfp(ops, c, tau, what, miss):
    B, H = c['txt'].shape
    lb, rl = moat((3 * B,), torch.float32, NAN)
    hb, rh = moat((3 * B,), torch.int32, -5)
    ab, acc = moat((3, 3), torch.float64, 0.0)
    ops.val_cfp(c['xs'][0].to(DEV), c['xs'][1].to(DEV), c['xs'][2].to(DEV), c['txt'].to(DEV), tau, rl, rh)
    for k in range(3):
        ops.val_reduce(rl[k * B:(k + 1) * B], rh[k * B:(k + 1) * B], None, acc[k])
    torch.cuda.synchronize()
    if not pads_intact(lb, hb, ab):
        miss.append('%s: a sentinel pad was written' % what)
    check_rows(what, rl, rh, c['loss'].reshape(-1), c['hit'].reshape(-1), c['scale'].reshape(-1), miss)
    for k in range(3):
        check_sums('%s k=%d' % (what, k), acc[k], float(c['loss'][k].sum()), int(c['hit'][k].sum()), B, float(c['bounds'][k]), miss)


@pytest.mark.parametrize('H', CFP_H)
def test_cfp_every_batch_size(ops, H):
    cases = [conditioned_cfp(B, H) for B in CFP_B]
    assert all(c['gap'] >= 1e-3 for c in cases)
    assert any(c['hit'].any() for c in cases) and any((~c['hit']).any() for c in cases)
    miss = []
    for B, c in zip(CFP_B, cases):
        run_cfp(ops, c, TAU, 'cfp B=%d H=%d bump=%d' % (B, H, c['bump']), miss)
    assert not miss, '\n'.join(miss)


def test_cfp_exact_scores_and_a_planted_tie(ops):
    """small integers over 8 and tau = 1/4: every dot product is exact in float32 in any order, so the planted tie (two identical text
    rows) is a tie on the device too and must resolve to the lower index"""
    B, H, tau = 9, 64, 0.25
    g = _gen(29)
    txt = torch.randint(-4, 5, (B, H), generator=g).float() / 8.0
    txt[6] = txt[2]                                             # text 2 and text 6 score alike against every vector
    xs = [torch.randint(-4, 5, (B, H), generator=g).float() / 8.0 for _ in range(3)]
    for x in xs:
        x[2] = 2.0 * txt[2]                                     # rows 2 and 6 both score highest against texts 2 and 6
        x[6] = 2.0 * txt[2]
    loss, hit, scale, _ = cfp_ref(xs, txt, tau)
    for x in xs:
        s = x.double().numpy() @ txt.double().numpy().T / tau
        assert (s == (x @ txt.T / tau).double().numpy()).all()                     # exact in float32
        assert s[2].argmax() == 2 and s[6].argmax() == 2 and s[6, 2] == s[6, 6] == s[6].max()
    assert hit[:, 2].all() and not hit[:, 6].any()
    c = dict(xs=xs, txt=txt, loss=loss, hit=hit, scale=scale, bounds=TOL * scale.sum(1))
    f32 = cfp_f32(xs, txt, tau)
    for k in range(3):
        check_condition_c(f32[k], float(loss[k].sum()), float(c['bounds'][k]), 'cfp exact k=%d' % k)
    miss = []
    run_cfp(ops, c, tau, 'cfp exact', miss)
    assert not miss, '\n'.join(miss)


# ================================================================================================ model level
MODEL_CASES = ('pretrain_small_ragged', 'pretrain_r2r_mrc', 'pretrain_reverie_small')


class Recorder(torch.nn.Module):
    """hands the model's outputs through and keeps a CPU copy of each, by task, in call order"""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.seen = {}

    def forward(self, batch, task, compute_loss=True):
        assert compute_loss is False and not self.model.training and not torch.is_grad_enabled()
        out = self.model(batch, task=task, compute_loss=compute_loss)
        keep = tuple(None if o is None else o.detach().cpu() for o in (out if isinstance(out, tuple) else (out,)))
        self.seen.setdefault(task, []).append(keep)
        return out


@functools.lru_cache(maxsize=None)
def model_case(name):
    from vln_goat_amd import synth
    cfg, model, _ = build_case(name)
    bkw = CASES[name][1]
    batches = [synth.make_pretrain_batch(**dict(bkw, seed=bkw['seed'] + 100 * k)) for k in range(3)]
    batches[1]['txt_labels'].fill_(-1)                          # the empty mlm selection
    model = model.to(DEV).eval()
    return cfg, model, batches, [synth.batch_to(b, DEV) for b in batches]


def _ce64(scores, labels):
    """-> (float64 loss sum, hits, rows, sum of row scales) of F.cross_entropy(reduction='sum') / argmax == labels on the CPU"""
    s = scores.double()
    lse = torch.logsumexp(s, 1)
    xl = s.gather(1, labels[:, None]).squeeze(1)
    scale = torch.maximum(torch.maximum(lse.abs(), xl.abs()), torch.ones_like(lse))
    return (float(F.cross_entropy(s, labels, reduction='sum')), int((s.max(dim=-1)[1] == labels).sum()), labels.numel(), float(scale.sum()))


def _close(got, want, scale_sum, count, what):
    print('FIG %s %r vs %r (bound %.3e)' % (what, got, want, TOL * scale_sum / count))
    assert abs(got - want) <= TOL * scale_sum / count, what


@pytest.mark.parametrize('name', MODEL_CASES)
def test_validate_loops_against_the_reference_formulas(name):
    from vln_goat_amd import pretrain_eval
    cfg, model, cpu_batches, batches = model_case(name)
    rec = Recorder(model).eval()
    tasks = case_tasks(name)
    assert set(tasks) >= {'mlm', 'sap', 'cfp'} and (name != 'pretrain_reverie_small' or {'og', 'mrc'} <= set(tasks))

    log = pretrain_eval.validate_mlm(rec, batches)
    tot = [0.0, 0, 0, 0.0]
    assert [o[0].shape[0] for o in rec.seen['mlm']].count(0) == 1          # one batch without a masked token
    for b, (scores,) in zip(cpu_batches, rec.seen['mlm']):
        labels = b['txt_labels'][b['txt_labels'] != -1]
        if labels.numel():
            tot = [a + v for a, v in zip(tot, _ce64(scores, labels))]
    assert set(log) == {'loss', 'acc', 'tok_per_s'} and log['acc'] == tot[1] / tot[2] and log['tok_per_s'] > 0
    _close(log['loss'], tot[0] / tot[2], tot[3], tot[2], name + ' mlm loss')

    log = pretrain_eval.validate_sap(rec, batches)
    tots = {k: [0.0, 0, 0, 0.0] for k in 'glf'}
    for gl, ll, fl, ga, la in rec.seen['sap']:
        for k, (sc, lab) in zip('glf', ((gl, ga), (ll, la), (fl, ga))):    # the fused row against the global labels
            tots[k] = [a + v for a, v in zip(tots[k], _ce64(sc, lab))]
    assert set(log) == {'gloss', 'lloss', 'floss', 'gacc', 'lacc', 'facc', 'tok_per_s'}
    n = tots['g'][2]
    assert n == sum(len(b['global_act_labels']) for b in cpu_batches)
    for k in 'glf':
        assert log[k + 'acc'] == tots[k][1] / n, k
        _close(log[k + 'loss'], tots[k][0] / n, tots[k][3], n, '%s sap %sloss' % (name, k))

    log = pretrain_eval.validate_cfp(rec, batches, cfg.cfp_temperature)
    tots = {k: [0.0, 0, 0.0] for k in 'glf'}
    n = 0
    for go, vo, fo, to in rec.seen['cfp']:
        loss, hit, scale, gap = cfp_ref([go, vo, fo], to, cfg.cfp_temperature)
        assert gap > 1e-6                                       # (no hit of this batch hangs on float32 rounding)
        n += to.shape[0]
        for j, k in enumerate('glf'):
            tots[k] = [tots[k][0] + float(loss[j].sum()), tots[k][1] + int(hit[j].sum()), tots[k][2] + float(scale[j].sum())]
    assert set(log) == {'gloss', 'lloss', 'floss', 'gacc', 'lacc', 'facc', 'tok_per_s'}
    for k in 'glf':
        assert log[k + 'acc'] == tots[k][1] / n, k
        _close(log[k + 'loss'], tots[k][0] / n, tots[k][2], n, '%s cfp %sloss' % (name, k))

    if 'mrc' in tasks:
        log = pretrain_eval.validate_mrc(rec, batches)
        tot, hits, n_feat, scale_sum = 0.0, 0, 0, 0.0
        for b, (vl, vt, _, _) in zip(cpu_batches, rec.seen['mrc']):
            tot += float(F.kl_div(F.log_softmax(vl.double(), dim=-1), vt.double(), reduction='sum'))
            hits += int((vl.max(dim=-1)[1] == vt.max(dim=-1)[1]).sum())
            n_feat += int(b['vp_view_mrc_masks'].sum())
            scale_sum += float(soft_ref(vl, vt)[2].sum())
        assert set(log) == {'loss', 'acc', 'feat_per_s'} and log['acc'] == hits / n_feat and log['feat_per_s'] > 0
        _close(log['loss'], tot / n_feat, scale_sum, n_feat, name + ' mrc loss')

    if 'og' in tasks:
        log = pretrain_eval.validate_og(rec, batches)
        tot = [0.0, 0, 0, 0.0]
        for b, (scores,) in zip(cpu_batches, rec.seen['og']):
            assert bool(torch.isinf(scores).any())              # masked object slots carry -inf
            tot = [a + v for a, v in zip(tot, _ce64(scores, b['obj_labels']))]
        assert set(log) == {'loss', 'acc', 'tok_per_s'} and log['acc'] == tot[1] / tot[2]
        _close(log['loss'], tot[0] / tot[2], tot[3], tot[2], name + ' og loss')


@pytest.mark.parametrize('training', [True, False])
def test_validate_over_all_tasks(training):
    from vln_goat_amd import pretrain_eval
    name = 'pretrain_reverie_small'
    cfg, model, _, batches = model_case(name)
    tasks = case_tasks(name)
    loaders = {t: batches for t in tasks}
    keys = {'mlm': ('loss', 'acc', 'tok_per_s'), 'og': ('loss', 'acc', 'tok_per_s'), 'mrc': ('loss', 'acc', 'feat_per_s'),
            'sap': ('gloss', 'lloss', 'floss', 'gacc', 'lacc', 'facc', 'tok_per_s'), 'cfp': ('gloss', 'lloss', 'floss', 'gacc', 'lacc', 'facc', 'tok_per_s')}
    model.train(training)
    try:
        logs, best, flag = pretrain_eval.validate(model, loaders, setname='_unseen', max_metrix=0.0, tem=cfg.cfp_temperature)
        assert model.training is training
        assert set(logs) == {'val_unseen_%s_%s' % (t, k) for t in tasks for k in keys[t]}
        assert all(np.isfinite(v) for v in logs.values())
        facc = logs['val_unseen_sap_facc']
        assert flag is True and best == facc                    # facc >= 0.0
        assert pretrain_eval.validate(model, {'sap': batches}, setname='_unseen', max_metrix=facc, tem=cfg.cfp_temperature)[1:] == (facc, True)
        assert pretrain_eval.validate(model, {'sap': batches}, setname='_unseen', max_metrix=facc + 0.5, tem=cfg.cfp_temperature)[1:] == (facc + 0.5, False)
        logs2, best2, flag2 = pretrain_eval.validate(model, {'sap': batches}, setname='_seen', max_metrix=0.0)
        assert (best2, flag2) == (0.0, False) and logs2['val_seen_sap_facc'] == facc          # the same figure, bit for bit, on a second pass
        with pytest.raises(ValueError):
            pretrain_eval.validate(model, {'itm': batches})
        assert model.training is training
    finally:
        model.eval()
