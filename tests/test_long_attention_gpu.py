"""Attention and CFP pooling over 257-512 keys (RxR-length instructions): the key-streaming forward of csrc/attention_long.hip and the
strided pooling passes, against the float32 PyTorch references of tests/test_hip_ops.py (same tolerances: 1e-3 float32, 2e-2 bf16,
relative to the reference's maximum)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
B, NH, H = 3, 3, 192


def _tol(dtype):
    return 1e-3 if dtype == torch.float32 else 2e-2


def _close(got, ref, dtype, what=''):
    got, ref = got.float().cpu(), ref.float().cpu()
    scale = ref.abs().max().clamp_min(1e-6)
    err = (got - ref).abs().max() / scale
    assert err < _tol(dtype), '%s: max err / scale = %.3e' % (what, err)


def _attn_ref(q, k, v, kmask, bias, nh):
    B, Lq, H = q.shape

    def sp(x):
        return x.view(x.shape[0], x.shape[1], nh, 64).permute(0, 2, 1, 3)
    s = sp(q) @ sp(k).transpose(-1, -2) / 8.0
    if kmask is not None:
        s = s + kmask[:, None, None, :]
    if bias is not None:
        s = s + bias[:, None]
    p = torch.softmax(s, -1)
    return (p @ sp(v)).permute(0, 2, 1, 3).reshape(B, Lq, H)


@pytest.fixture(scope='module')
def ops():
    from vln_goat_amd import hipops
    return hipops


def _inputs(Lq, Lk, mode, dtype, g):
    if mode == 'self':
        a = (torch.randn(B, Lq, 3 * H, generator=g) * 0.7).to(DEV, dtype).requires_grad_(True)
        return a, None
    a = (torch.randn(B, Lq, H, generator=g) * 0.7).to(DEV, dtype).requires_grad_(True)
    b = (torch.randn(B, Lk, 2 * H, generator=g) * 0.7).to(DEV, dtype).requires_grad_(True)
    return a, b


def _check_against_reference(ops, dtype, Lq, Lk, mode, kmask, use_bias, g):
    bias = (torch.randn(B, Lq, Lk, generator=g) * 0.5).to(DEV).requires_grad_(True) if use_bias else None
    a, b = _inputs(Lq, Lk, mode, dtype, g)
    o = ops.attention(a, b, kmask, bias, NH, 0.0)
    af = a.detach().float().requires_grad_(True)
    bf = None
    if mode == 'self':
        q, k, v = af.split(H, -1)
    else:
        bf = b.detach().float().requires_grad_(True)
        q = af
        k, v = bf.split(H, -1)
    biasf = bias.detach().clone().requires_grad_(True) if use_bias else None
    ref = _attn_ref(q, k, v, kmask, biasf, NH)
    do = torch.randn(B, Lq, H, generator=g).to(DEV)
    o.backward(do.to(dtype))
    ref.backward(do.to(dtype).float())
    for t in (o, a.grad) + ((b.grad,) if b is not None else ()) + ((bias.grad,) if use_bias else ()):
        assert torch.isfinite(t).all()
    _close(o, ref, dtype, 'attn out')
    _close(a.grad, af.grad, dtype, 'attn da')
    if b is not None:
        _close(b.grad, bf.grad, dtype, 'attn db')
    if use_bias:
        _close(bias.grad, biasf.grad, dtype, 'attn dbias')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('Lq,Lk,mode,use_bias,inf', [
    (257, 257, 'self', False, False),       # first length over the old limit: a one-key tail tile
    (300, 300, 'self', False, True),        # klens [Lk, Lk // 2, Lk - 3]: whole trailing tiles at -inf
    (512, 512, 'self', True, False),        # the maximum, with dbias
    (37, 300, 'cross', False, False),
    (5, 511, 'cross', False, False),
    (33, 289, 'cross', True, False),
    (300, 23, 'cross', False, False)])      # long queries over short keys (the existing kernels)
def test_long_attention_fwd_bwd(ops, dtype, Lq, Lk, mode, use_bias, inf):
    g = torch.Generator().manual_seed(Lq * 131 + Lk)
    klens = torch.tensor([Lk, max(1, Lk // 2), max(1, Lk - 3)])
    valid = torch.arange(Lk)[None, :] < klens[:, None]
    kmask = torch.zeros(B, Lk).masked_fill(~valid, float('-inf') if inf else -10000.0).to(DEV)
    _check_against_reference(ops, dtype, Lq, Lk, mode, kmask, use_bias, g)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('mode,Lq', [('self', 300), ('cross', 37)])
def test_long_attention_leading_masked_tiles(ops, dtype, mode, Lq):
    """kmask = -inf on keys 0..69 of one sample: the running maximum is still -inf after the first two key tiles."""
    Lk = 300
    g = torch.Generator().manual_seed(77 + Lq)
    kmask = torch.zeros(B, Lk)
    kmask[1, :70] = float('-inf')
    _check_against_reference(ops, dtype, Lq, Lk, mode, kmask.to(DEV), False, g)


def _raw_call(ops, a, b, kmask, do):
    """goat_attn_long_fwd / goat_attn_long_bwd with the arguments hipops._AttnFn builds (p = 0)."""
    from vln_goat_amd import _lib
    h = _lib.lib()
    pt, st, dt = ops._ptr, ops._stream, ops._dt
    if b is None:
        Bn, Lq, H3 = a.shape
        Hh, Lk = H3 // 3, Lq
        q, k, v = (a, 0, H3, Lq * H3), (a, Hh, H3, Lq * H3), (a, 2 * Hh, H3, Lq * H3)
    else:
        Bn, Lq, Hh = a.shape
        Lk, ldb = b.shape[1], b.stride(1)
        q, k, v = (a, 0, Hh, Lq * Hh), (b, 0, ldb, Lk * ldb), (b, Hh, ldb, Lk * ldb)
    nh = Hh // 64
    o = torch.empty((Bn, Lq, Hh), dtype=a.dtype, device=a.device)
    lse = torch.empty((Bn, nh, Lq), dtype=torch.float32, device=a.device)
    scale = 1.0 / math.sqrt(64.0)
    rc = h.goat_attn_long_fwd(st(), dt(a), pt(q[0], q[1]), q[2], q[3], pt(k[0], k[1]), k[2], k[3], pt(v[0], v[1]), v[2], v[3],
                              pt(o), Hh, Lq * Hh, pt(kmask), None, pt(lse), Bn, nh, Lq, Lk, scale, 0.0, 0, 0, None)
    assert rc == 0
    da = torch.empty_like(a)
    db = torch.empty_like(b) if b is not None else None
    if b is None:
        dq, dk, dv = (da, 0, H3, Lq * H3), (da, Hh, H3, Lq * H3), (da, 2 * Hh, H3, Lq * H3)
    else:
        dq, dk, dv = (da, 0, Hh, Lq * Hh), (db, 0, ldb, Lk * ldb), (db, Hh, ldb, Lk * ldb)
    rc = h.goat_attn_long_bwd(st(), dt(a), pt(q[0], q[1]), q[2], q[3], pt(k[0], k[1]), k[2], k[3], pt(v[0], v[1]), v[2], v[3],
                              pt(o), Hh, Lq * Hh, pt(do), Hh, Lq * Hh,
                              pt(dq[0], dq[1]), dq[2], dq[3], pt(dk[0], dk[1]), dk[2], dk[3], pt(dv[0], dv[1]), dv[2], dv[3],
                              pt(kmask), None, pt(lse), None, Bn, nh, Lq, Lk, scale, 0.0, 0, 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    return o, lse, da, db


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('Lq,Lk,mode', [(80, 80, 'self'), (60, 200, 'cross')])
def test_long_entry_points_agree_with_the_short_ones(ops, dtype, Lq, Lk, mode):
    """Below 257 keys hipops.attention runs goat_attn_fwd / goat_attn_bwd; the long pair, called directly on the same problem,
    must give the same output, lse and gradients."""
    from vln_goat_amd import _lib
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    klens = torch.tensor([Lk, max(1, Lk // 2), max(1, Lk - 3)])
    kmask = torch.zeros(B, Lk).masked_fill(~(torch.arange(Lk)[None, :] < klens[:, None]), -10000.0).to(DEV)
    a, b = _inputs(Lq, Lk, mode, dtype, g)
    do = torch.randn(B, Lq, H, generator=g).to(DEV, dtype)
    o = ops.attention(a, b, kmask, None, NH, 0.0)
    o.backward(do)
    # the short forward's lse: call it once more through the ABI with the same arguments
    o2, lse2, da2, db2 = _raw_call(ops, a.detach(), b.detach() if b is not None else None, kmask, do)
    lse = torch.empty_like(lse2)
    if b is None:
        q, k, v = (a, 0, 3 * H, Lq * 3 * H), (a, H, 3 * H, Lq * 3 * H), (a, 2 * H, 3 * H, Lq * 3 * H)
    else:
        q, k, v = (a, 0, H, Lq * H), (b, 0, 2 * H, Lk * 2 * H), (b, H, 2 * H, Lk * 2 * H)
    o1 = torch.empty_like(o2)
    rc = _lib.lib().goat_attn_fwd(ops._stream(), ops._dt(a), ops._ptr(q[0], q[1]), q[2], q[3], ops._ptr(k[0], k[1]), k[2], k[3],
                                  ops._ptr(v[0], v[1]), v[2], v[3], ops._ptr(o1), H, Lq * H, ops._ptr(kmask), None, ops._ptr(lse),
                                  B, NH, Lq, Lk, 0.125, 0.0, 0, 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(o1, o.detach())
    _close(o2, o.detach(), dtype, 'out')
    _close(lse2, lse, dtype, 'lse')
    _close(da2, a.grad, dtype, 'da')
    if b is not None:
        _close(db2, b.grad, dtype, 'db')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('L', [257, 320])
def test_long_attention_dropout_backward_uses_the_forward_mask(ops, dtype, L):
    """tests/test_hip_ops.py's dropout check over the old limit: the mask is recovered from forward calls on one-hot V
    (O[q, d] != 0 <=> probability (q, 64 j + d) kept); a torch reference with that mask gives the expected output and gradients;
    equal seeds give equal bits."""
    Bd, p = 2, 0.3
    g = torch.Generator().manual_seed(L)
    qk = (torch.randn(Bd, L, 2 * H, generator=g) * 0.5).to(DEV, dtype)
    v = (torch.randn(Bd, L, H, generator=g) * 0.7).to(DEV, dtype)
    keep = torch.zeros(Bd, NH, L, L, dtype=torch.bool, device=DEV)
    for j in range((L + 63) // 64):
        onehot = torch.zeros(Bd, L, NH, 64, device=DEV, dtype=dtype)
        n = min(64, L - 64 * j)
        onehot[:, 64 * j + torch.arange(n), :, torch.arange(n)] = 1
        ops.manual_seed(1234)
        o = ops.attention(torch.cat([qk, onehot.view(Bd, L, H)], -1), None, None, None, NH, p)
        keep[:, :, :, 64 * j:64 * j + n] = (o.view(Bd, L, NH, 64).permute(0, 2, 1, 3)[..., :n] != 0)
    rate = 1.0 - keep.float().mean().item()
    print('L %d %s: drop rate %.4f' % (L, dtype, rate))
    assert abs(rate - p) < 0.02, rate
    a = torch.cat([qk, v], -1).requires_grad_(True)
    ops.manual_seed(1234)
    o = ops.attention(a, None, None, None, NH, p)
    do = torch.randn(Bd, L, H, generator=g).to(DEV, dtype)
    o.backward(do)
    af = a.detach().float().requires_grad_(True)

    def sp(x):
        return x.view(Bd, L, NH, 64).permute(0, 2, 1, 3)
    qf, kf, vf = af.split(H, -1)
    pr = torch.softmax(sp(qf) @ sp(kf).transpose(-1, -2) / 8.0, -1) * keep / (1.0 - p)
    ref = (pr @ sp(vf)).permute(0, 2, 1, 3).reshape(Bd, L, H)
    ref.backward(do.float())
    _close(o, ref, dtype, 'attn dropout out')
    _close(a.grad, af.grad, dtype, 'attn dropout grads')
    g1 = a.grad.clone()
    a.grad = None
    ops.manual_seed(1234)
    o2 = ops.attention(a, None, None, None, NH, p)
    o2.backward(do)
    assert torch.equal(o, o2)
    assert torch.equal(g1, a.grad)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('L', [257, 300, 512])
def test_attn_pool_long(ops, dtype, L):
    """tanh-attention pooling of the CFP heads over more slots than one block has threads."""
    Bp, Hp = 5, 768
    g = torch.Generator().manual_seed(41)
    x = (torch.randn(Bp, L, Hp, generator=g) * 0.7).to(DEV, dtype).requires_grad_(True)
    w = torch.nn.Parameter((torch.rand(Hp, 1, generator=g) * 0.2 - 0.1).to(DEV))
    out = ops.attn_pool(x, w)
    dout = torch.randn(Bp, Hp, generator=g).to(DEV)
    out.backward(dout)
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)
    a = torch.softmax(torch.matmul(torch.tanh(xr), wr), 1)
    ref = torch.tanh(torch.sum(xr * a, 1))
    ref.backward(dout)
    assert out.dtype == torch.float32
    _close(out, ref, dtype, 'attn_pool')
    _close(x.grad, xr.grad, dtype, 'attn_pool dx')
    _close(w.grad, wr.grad, dtype, 'attn_pool dw')


def test_attention_over_512_keys_is_a_value_error(ops):
    a = torch.zeros(1, 4, 64, device=DEV)
    b = torch.zeros(1, 513, 128, device=DEV)
    with pytest.raises(ValueError, match='512'):
        ops.attention(a, b, None, None, 1, 0.0)
