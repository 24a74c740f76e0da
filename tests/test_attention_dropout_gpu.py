"""goat_attn_fwd / goat_attn_bwd WITH dropout, through hipops.attention, on every kernel family of the short pair (Lk <= 256): odd and
even key counts, cross shapes, key masks (-10000 and -inf), the bias and its gradient, fully masked samples and the device-side seed
bump.

Two independent checks per case:
  * the dropout bits the forward drew (recovered through one-hot V) are EXACTLY helpers.attn_keep_mask — the documented function of
    (seed + *rng_dev, offset, b, h, q, key) and the dtype, restated on the host in integer arithmetic;
  * O, dQ, dK, dV and dbias match float64 autograd of softmax(scale QK^T + kmask + bias) * keep / (1 - p) @ V built from THAT host mask
    (not from what the forward drew: a mask that both directions get wrong in the same way would fail here).
Tolerance: test_hip_ops._close (max error / max reference: 1e-3 float32, 2e-2 bf16), the figure the p = 0.3 tests there hold."""
import pytest
import torch

from helpers import attn_keep_mask
from test_hip_ops import _close

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SEED = 1234
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope='module')
def ops():
    from vln_goat_amd import hipops
    return hipops


@pytest.fixture()
def rng_state(ops):
    """the process-wide dropout counter state, put back after the test"""
    saved = (ops.RngState.seed, ops.RngState.base, ops.RngState.counter, ops.RngState.dev)
    yield ops.RngState
    ops.RngState.seed, ops.RngState.base, ops.RngState.counter, ops.RngState.dev = saved


def bwd_family(dtype, Lq, Lk):
    """The backward kernel that serves [Lq, Lk]: the dispatch of goat_attn_bwd (csrc/attention.hip) and goat_attn2_bwd (csrc/attention2.hip)
    restated.  float32 always streams; bf16 takes the shared-dS kernel (template per dS-stride class) while its LDS image fits 160 KiB,
    then the role kernel (multi-role form when there are more tiles than waves, on 8 waves or as few as 6), then streams."""
    if dtype == F32:
        return 'stream'
    nqt, nkt = (Lq + 31) // 32, (Lk + 31) // 32
    tile = 32 * 72 * 2
    dss = 40 if nkt == 1 else 72 if nkt == 2 else 104 if nkt == 3 else 168 if nkt <= 5 else 264
    if (2 * nqt + 2 * nkt) * tile + nqt * 32 * dss * 2 + (2 * nqt + nkt) * 128 <= 160 * 1024:
        return 'shared%d' % dss
    nwv = min(nqt + nkt, 8)
    sm0 = (2 * nqt + 2 * nkt) * tile + (2 * nqt + nkt) * 128
    sm = sm0 + (nwv * tile if nqt + nkt > 8 else 0)
    while sm > 160 * 1024 and nqt + nkt > 8 and nwv > 6:
        nwv -= 1
        sm = sm0 + nwv * tile
    if sm > 160 * 1024:
        return 'stream'
    return ('multi%d' if nqt + nkt > 8 else 'roles%d') % nwv


class Case:
    """Operands of one attention problem (self-attention when Lq == Lk, else cross), its runs on the GPU and its float64 reference.
    mask: None | 'm1e4' | 'inf' (ragged key lengths, masked keys at -10000 / -inf); dead: this sample has -inf on EVERY key."""

    def __init__(self, ops, dtype, Lq, Lk, nh=3, p=0.3, mask=None, use_bias=False, B=2, dead=None):
        self.ops, self.dtype, self.Lq, self.Lk, self.nh, self.p, self.B = ops, dtype, Lq, Lk, nh, p, B
        self.H = H = nh * 64
        self.self_attn = Lq == Lk
        g = torch.Generator().manual_seed(Lq * 1000 + Lk)
        self.q = (torch.randn(B, Lq, H, generator=g) * 0.5).to(DEV, dtype)
        self.k = (torch.randn(B, Lk, H, generator=g) * 0.5).to(DEV, dtype)
        self.v = (torch.randn(B, Lk, H, generator=g) * 0.5).to(DEV, dtype)
        self.do = torch.randn(B, Lq, H, generator=g).to(DEV, dtype)
        self.bias = (torch.randn(B, Lq, Lk, generator=g) * 0.5).to(DEV) if use_bias else None
        self.kmask = None
        if mask is not None or dead is not None:
            klens = torch.tensor([max(1, Lk - 3), max(1, (Lk + 1) // 2), max(1, Lk - 1)][:B])
            if dead is not None:
                klens[dead] = 0
            fill = -10000.0 if mask == 'm1e4' else float('-inf')
            self.kmask = torch.zeros(B, Lk).masked_fill(~(torch.arange(Lk)[None, :] < klens[:, None]), fill).to(DEV)
        # keys whose probabilities can be seen (a masked key has probability 0 whatever its dropout bit)
        self.visible = (self.kmask == 0) if self.kmask is not None else torch.ones(B, Lk, dtype=torch.bool, device=DEV)

    def _call(self, q, k, v, bias, seed=SEED):
        """one production call; the seed is set in front of it, so a dropout call draws at offset 0"""
        self.ops.manual_seed(seed)
        assert self.ops.RngState.seed == seed and self.ops.RngState.counter == 0
        if self.self_attn:
            a, b = torch.cat([q, k, v], -1).requires_grad_(True), None
        else:
            a, b = q.clone().requires_grad_(True), torch.cat([k, v], -1).requires_grad_(True)
        return a, b, self.ops.attention(a, b, self.kmask, bias, self.nh, self.p)

    def run(self):
        """-> O, dQ, dK, dV, dbias of the kernels"""
        bias = self.bias.clone().requires_grad_(True) if self.bias is not None else None
        a, b, o = self._call(self.q, self.k, self.v, bias)
        o.backward(self.do)
        torch.cuda.synchronize()
        H = self.H
        if self.self_attn:
            dq, dk, dv = a.grad.split(H, -1)
        else:
            dq, (dk, dv) = a.grad, b.grad.split(H, -1)
        return o.detach(), dq, dk, dv, (bias.grad if bias is not None else None)

    def drawn_mask(self):
        """bool [B, nh, Lq, Lk]: the forward's keep bits, from calls on one-hot V (O[q, d] != 0 <=> probability (q, 64 j + d) kept)."""
        B, nh, Lq, Lk = self.B, self.nh, self.Lq, self.Lk
        keep = torch.zeros(B, nh, Lq, Lk, dtype=torch.bool, device=DEV)
        with torch.no_grad():
            for j in range((Lk + 63) // 64):
                n = min(64, Lk - 64 * j)
                onehot = torch.zeros(B, Lk, nh, 64, device=DEV, dtype=self.dtype)
                onehot[:, 64 * j + torch.arange(n), :, torch.arange(n)] = 1
                _, _, o = self._call(self.q, self.k, onehot.view(B, Lk, self.H), self.bias)
                keep[:, :, :, 64 * j:64 * j + n] = (o.detach().view(B, Lq, nh, 64).permute(0, 2, 1, 3)[..., :n] != 0)
        return keep

    def host_mask(self, seed=SEED):
        if self.p == 0:
            return torch.ones(self.B, self.nh, self.Lq, self.Lk, dtype=torch.bool, device=DEV)
        return torch.from_numpy(attn_keep_mask(self.dtype, seed, 0, self.B, self.nh, self.Lq, self.Lk, self.p)).to(DEV)

    def reference(self, keep):
        """float64 autograd on the upcast operands -> O, dQ, dK, dV, dbias, the smallest probability of a visible key.  A row without
        keys (every score -inf) is a row of zeros."""
        B, nh = self.B, self.nh
        q, k, v = (x.double().requires_grad_(True) for x in (self.q, self.k, self.v))
        bias = self.bias.double().requires_grad_(True) if self.bias is not None else None

        def sp(x):
            return x.view(B, x.shape[1], nh, 64).permute(0, 2, 1, 3)
        s = sp(q) @ sp(k).transpose(-1, -2) / 8.0
        if self.kmask is not None:
            s = s + self.kmask.double()[:, None, None, :]
        if bias is not None:
            s = s + bias[:, None]
        empty = (s == float('-inf')).all(-1, keepdim=True)
        pr = torch.softmax(torch.where(empty, torch.zeros_like(s), s), -1) * (~empty)
        vis = self.visible[:, None, None, :].expand_as(pr)
        pmin = float(pr.detach()[vis & ~empty.expand_as(pr)].min()) if bool((vis & ~empty).any()) else 1.0
        o = ((pr * keep / (1.0 - self.p)) @ sp(v)).permute(0, 2, 1, 3).reshape(B, self.Lq, self.H)
        o.backward(self.do.double())
        return o.detach(), q.grad, k.grad, v.grad, (bias.grad if bias is not None else None), pmin


NAMES = ('O', 'dQ', 'dK', 'dV', 'dbias')


def one_key_bounds(case, o_ref):
    """Lk = 1: the softmax over one key is the constant 1, so the float64 dQ, dK and dbias are identically zero and max error / max
    reference has no scale.  What a correct bf16 kernel leaves there is rounding: dS = P (dP keep / (1 - p) - D) with D = sum_d dO_d O'_d
    from the STORED output O', while dP keep / (1 - p) = sum_d dO_d O_d exactly, so |dS| <= sum_d |dO_d| |O_d - O'_d|.  O' carries two bf16
    roundings (the probability fragment of the MFMA and the stored result: 2^-9 relative each), hence |dS| <= 2^-8 sum_d |dO_d| |O_d|;
    (1 + 2^-7) on top covers the bf16 roundings of dS and of the stored gradients and the float32 arithmetic in between.  dQ = dS scale K,
    dK = sum_q dS_q scale Q_q, dbias = sum_h dS follow elementwise.  (A dropped probability has O = O' = 0: exact zeros.)"""
    assert case.Lk == 1 and case.dtype == BF16
    B, Lq, nh, H = case.B, case.Lq, case.nh, case.H
    u = 2.0 ** -8 * (1 + 2.0 ** -7)
    e = u * (case.do.double().abs() * o_ref.abs()).view(B, Lq, nh, 64).sum(-1, keepdim=True)      # [B, Lq, nh, 1]
    k, q = case.k.double().abs().view(B, 1, nh, 64), case.q.double().abs().view(B, Lq, nh, 64)
    return {'dQ': (e * k / 8.0).reshape(B, Lq, H), 'dK': (e * q / 8.0).sum(1, keepdim=True).reshape(B, 1, H), 'dbias': e.sum(2)}


def check_values(case, got, ref, what):
    """every tensor against its float64 reference by test_hip_ops._close; the figures are printed, every miss is reported"""
    misses = []
    for name, g, r in zip(NAMES, got, ref):
        assert (g is None) == (r is None), name
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), '%s %s: not finite' % (what, name)
        if name in ('dQ', 'dK', 'dbias') and case.Lk == 1:
            assert not bool(r.any())
            bound = one_key_bounds(case, ref[0])[name]
            over = g.double().abs() - bound
            print('%s %s: reference identically 0, max |got| = %.3e, max (|got| - bound) = %.3e' % (what, name, float(g.abs().max()), float(over.max())))
            if bool((over > 0).any()):
                misses.append('%s: |got| exceeds the rounding bound by %.3e' % (name, float(over.max())))
            continue
        err = float((g.double() - r).abs().max() / r.abs().max().clamp_min(1e-6))
        print('%s %s: max err / scale = %.3e' % (what, name, err))
        try:
            _close(g, r, case.dtype, '%s %s' % (what, name))
        except AssertionError as ex:
            misses.append(str(ex).splitlines()[0])
    assert not misses, misses


def check_mask(case, drawn, host, pmin):
    # (every visible probability is far above the smallest bf16 / float32 normal, so a kept one cannot read as 0)
    assert pmin > 1e-6, pmin
    vis = case.visible[:, None, None, :].expand_as(drawn)
    bad = (drawn != host) & vis
    assert not bool(bad.any()), 'dropout bits differ from the documented hash at %d of %d visible positions, first (b, h, q, key) = %s' % (
        int(bad.sum()), int(vis.sum()), bad.nonzero()[0].tolist())


# ------------------------------------------------------------------------------------------------ a. anchor: a path the suite already runs
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_mask_restatement_on_the_64_by_64_anchor(ops, dtype):
    """L = 64 self-attention is what test_hip_ops' dropout tests run: a disagreement HERE is an error of helpers.attn_keep_mask, not of a
    kernel."""
    c = Case(ops, dtype, 64, 64)
    host = c.host_mask()
    check_mask(c, c.drawn_mask(), host, c.reference(host)[-1])
    assert abs(1.0 - host.float().mean().item() - 0.3) < 0.02


# ------------------------------------------------------------------------------------------------ b. the dispatch matrix
# (family of the bf16 backward, Lq, Lk, key mask, bias with gradient, nh, p).  Every dS-stride class of the shared kernel, both forms of
# the multi-role kernel and the streaming fallback see no mask, -10000, -inf and the bias gradient; odd and even Lk wherever both exist.
MATRIX = [
    ('shared40', 31, 31, None, True, 3, 0.3), ('shared40', 40, 17, 'm1e4', False, 3, 0.3), ('shared40', 7, 32, 'inf', True, 3, 0.3),
    ('shared40', 1, 1, None, False, 3, 0.3), ('shared40', 5, 1, None, True, 3, 0.3),
    ('shared72', 63, 63, 'inf', False, 3, 0.3), ('shared72', 80, 37, 'm1e4', True, 3, 0.3), ('shared72', 50, 64, None, False, 12, 0.3),
    ('shared104', 81, 81, None, True, 3, 0.3), ('shared104', 80, 80, 'm1e4', False, 3, 0.3), ('shared104', 23, 95, 'inf', True, 3, 0.3),
    ('shared168', 129, 129, 'm1e4', True, 3, 0.3), ('shared168', 37, 159, 'inf', False, 3, 0.3), ('shared168', 37, 160, None, True, 3, 0.1),
    ('shared264', 23, 199, 'inf', True, 3, 0.3), ('shared264', 60, 200, None, False, 3, 0.3), ('shared264', 96, 255, 'm1e4', True, 3, 0.3),
    ('shared264', 1, 161, None, False, 3, 0.3),
    ('multi8', 180, 180, None, True, 3, 0.3), ('multi8', 191, 191, 'inf', False, 3, 0.3), ('multi8', 130, 255, 'm1e4', True, 3, 0.3),
    ('multi6', 199, 199, 'inf', True, 3, 0.3), ('multi6', 199, 200, None, False, 3, 0.3), ('multi6', 224, 224, 'm1e4', False, 3, 0.3),
    ('stream', 255, 255, 'm1e4', True, 3, 0.3), ('stream', 200, 255, 'inf', False, 3, 0.3), ('stream', 200, 254, None, True, 3, 0.3),
]
# float32: the streaming kernels on the 64-bit counter stream, whatever the shape
MATRIX_F32 = [('stream', 31, 31, None, True, 3, 0.3), ('stream', 80, 37, 'm1e4', False, 3, 0.3), ('stream', 129, 129, 'inf', True, 3, 0.3),
              ('stream', 23, 199, None, False, 3, 0.3), ('stream', 255, 255, 'm1e4', True, 3, 0.3)]


def _matrix_id(dtype, m):
    fam, Lq, Lk, mask, use_bias, nh, p = m
    return '%s-%s-%dx%d-%s%s-nh%d-p%g' % ('bf16' if dtype == BF16 else 'f32', fam, Lq, Lk, mask or 'nomask', '-dbias' if use_bias else '', nh, p)


_ALL = [(BF16, m) for m in MATRIX] + [(F32, m) for m in MATRIX_F32]


@pytest.mark.parametrize('dtype,m', _ALL, ids=[_matrix_id(d, m) for d, m in _ALL])
def test_dropout_bits_values_and_gradients(ops, dtype, m):
    fam, Lq, Lk, mask, use_bias, nh, p = m
    assert bwd_family(dtype, Lq, Lk) == fam
    c = Case(ops, dtype, Lq, Lk, nh=nh, p=p, mask=mask, use_bias=use_bias)
    host = c.host_mask()
    ref = c.reference(host)
    check_mask(c, c.drawn_mask(), host, ref[-1])
    check_values(c, c.run(), ref[:5], _matrix_id(dtype, m))


def test_matrix_covers_every_family_with_every_operand_mix():
    by = {}
    for fam, Lq, Lk, mask, use_bias, nh, p in MATRIX:
        e = by.setdefault(fam, dict(masks=set(), bias=False, odd=False, even=False))
        e['masks'].add(mask)
        e['bias'] |= use_bias
        e['odd' if Lk & 1 else 'even'] = True
    assert set(by) == {'shared40', 'shared72', 'shared104', 'shared168', 'shared264', 'multi8', 'multi6', 'stream'}
    for fam, e in by.items():
        assert e['masks'] == {None, 'm1e4', 'inf'} and e['bias'] and e['odd'] and e['even'], fam


# ------------------------------------------------------------------------------------------------ c. a sample without keys
DEAD = [(BF16, 36, 36), (BF16, 180, 180), (BF16, 255, 255), (BF16, 37, 80), (F32, 36, 36), (F32, 37, 80)]


@pytest.mark.parametrize('use_bias', [False, True], ids=['nobias', 'dbias'])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('dtype,Lq,Lk', DEAD, ids=['%s-%s-%dx%d' % ('bf16' if d == BF16 else 'f32', bwd_family(d, a, b), a, b) for d, a, b in DEAD])
def test_sample_with_every_key_masked_gives_exact_zeros(ops, dtype, Lq, Lk, p, use_bias):
    """goat_hip.h: "Rows whose keys are all -inf produce zeros" — outputs and every gradient of that sample, also under dropout and with a
    bias on top of the -inf; its neighbours in the batch (ragged -inf masks) are untouched by it."""
    dead = 1
    c = Case(ops, dtype, Lq, Lk, p=p, mask='inf', use_bias=use_bias, B=3, dead=dead)
    got, ref = c.run(), c.reference(c.host_mask())
    for name, g in zip(NAMES, got):
        if g is not None:
            assert bool(torch.isfinite(g).all()), name
            assert bool((g[dead] == 0).all()), '%s of the sample without keys: %d nonzero' % (name, int((g[dead] != 0).sum()))
    check_values(c, got, ref[:5], 'dead sample %dx%d p=%g' % (Lq, Lk, p))


# ------------------------------------------------------------------------------------------------ d. the device-side seed bump
BUMP = [(BF16, 63, 63), (BF16, 180, 180), (BF16, 255, 255), (F32, 31, 31)]


@pytest.mark.parametrize('dtype,Lq,Lk', BUMP, ids=['%s-%s-%dx%d' % ('bf16' if d == BF16 else 'f32', bwd_family(d, a, b), a, b) for d, a, b in BUMP])
def test_device_counter_is_added_to_the_seed(ops, rng_state, dtype, Lq, Lk):
    """seed + *rng_dev is what lets a replayed graph draw fresh masks: forward and backward of every family must read it."""
    bump = 0x9E3779B1
    c = Case(ops, dtype, Lq, Lk)
    rng_state.dev = torch.tensor([bump], dtype=torch.int64, device=DEV)
    host, unbumped = c.host_mask(SEED + bump), c.host_mask(SEED)
    assert not torch.equal(host, unbumped)
    ref = c.reference(host)
    drawn = c.drawn_mask()
    check_mask(c, drawn, host, ref[-1])
    assert not torch.equal(drawn, unbumped)
    check_values(c, c.run(), ref[:5], 'device counter %dx%d' % (Lq, Lk))
