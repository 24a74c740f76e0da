"""Shared test helpers: golden cases, oracle runs, gradient fingerprints."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# must match tests/golden/make_golden_pretrain.py
CASES = {
    'pretrain_small_fixed': (dict(num_l_layers=2, num_top_layer=2, num_pano_layers=2, vocab_size=1000),
                             dict(B=4, T=5, L=80, seed=1, vocab_size=1000, style='survey')),
    'pretrain_small_ragged': (dict(num_l_layers=2, num_top_layer=2, num_pano_layers=2, vocab_size=1000),
                              dict(B=4, T=[1, 3, 5, 2], L=[80, 33, 20, 57], seed=2, vocab_size=1000, style='rich',
                                   ragged_views=True)),
    'pretrain_config1': (dict(num_l_layers=2, num_top_layer=2, num_pano_layers=2),
                         dict(B=4, T=5, L=80, seed=3, style='survey')),
    # REVERIE/SOON object branch (objects appended to every panorama), OG head, MRC on views and objects
    'pretrain_reverie_small': (dict(num_l_layers=2, num_top_layer=2, num_pano_layers=2, vocab_size=1000, name='REVERIE',
                                    obj_feat_size=768, image_prob_size=100, obj_prob_size=100, obj_name_vocab_size=45,
                                    use_obj_name=True, pretrain_tasks=['mlm', 'mrc', 'sap', 'og', 'cfp']),
                               dict(B=4, T=[2, 4, 1, 3], L=[40, 33, 20, 57], seed=5, vocab_size=1000, style='rich',
                                    ragged_views=True, objects=6, mrc=True, prob_size=100)),
    # MRC head on an R2R batch (views only; separate object classifier configured but unused)
    'pretrain_r2r_mrc': (dict(num_l_layers=2, num_top_layer=2, num_pano_layers=2, vocab_size=1000, image_prob_size=100,
                              obj_prob_size=50, pretrain_tasks=['mlm', 'mrc', 'sap', 'cfp']),
                         dict(B=3, T=[3, 1, 2], L=[30, 24, 16], seed=6, vocab_size=1000, style='survey', mrc=True,
                              prob_size=100)),
    # BACL-txt in pre-training (do_back_txt): type_2 + door, and type_1 with dictionary->text cross-attention
    'pretrain_bacl_type2_door': (dict(num_l_layers=2, num_top_layer=2, num_pano_layers=2, vocab_size=1000, do_back_txt=True,
                                      do_back_txt_type='type_2', do_add_method='door', do_front_txt=True),
                                 dict(B=3, T=[2, 1, 3], L=[30, 24, 16], seed=8, vocab_size=1000, style='rich', zdict=(35, 39))),
    'pretrain_bacl_type1_xattn': (dict(num_l_layers=2, num_top_layer=2, num_pano_layers=2, vocab_size=1000, do_back_txt=True,
                                       do_back_txt_type='type_1', z_cross_attn=True),
                                  dict(B=3, T=[2, 1, 3], L=[30, 24, 16], seed=9, vocab_size=1000, style='survey', zdict=(35, 39))),
    # ---- full-size pins: BASELINE.json configs[1] / configs[4] at the sizes bench.py times them -------------
    # config 2: full R2R model (6/3/2 layers, vocab 50 265), per-rank batch 48, T=5, 36 views, L=80
    'pretrain_config2_full': (dict(), dict(B=48, T=5, L=80, seed=100, style='survey')),
    # config 5 shape: REVERIE model (object tokens, OG head, name embeddings), L=160, per-rank batch 32, up to 20 objects
    'pretrain_config5_reverie_full': (dict(name='REVERIE', obj_feat_size=768, image_prob_size=1000, obj_prob_size=1000,
                                           obj_name_vocab_size=45, use_obj_name=True,
                                           pretrain_tasks=['mlm', 'mrc', 'sap', 'og', 'cfp']),
                                      dict(B=32, T=5, L=160, seed=105, style='survey', objects=20, mrc=True, prob_size=1000)),
}
FULL_SIZE = ('pretrain_config2_full', 'pretrain_config5_reverie_full')


def case_tasks(name):
    return tuple(CASES[name][0].get('pretrain_tasks', ('mlm', 'sap', 'cfp')))
WEIGHT_SEED = 7


def load_golden(name):
    path = os.path.join(ROOT, 'tests', 'golden', name + '.npz')
    return dict(np.load(path, allow_pickle=False))


def build_case(name):
    """-> (config, product model (CPU, seeded), batch (CPU))."""
    from vln_goat_amd import config as gcfg, pretrain_model, synth
    cfg_over, bkw = CASES[name]
    cfg = gcfg.make_config(**cfg_over)
    model = pretrain_model.GlocalTextPathCMTPreTraining(cfg)
    sd = synth.seeded_state_dict(model, seed=WEIGHT_SEED)
    model.load_state_dict(sd)
    model.tie_weights()
    batch = synth.make_pretrain_batch(**bkw)
    return cfg, model, batch


def fingerprint(grad):
    if grad is None:
        return np.zeros(9, dtype=np.float32)
    flat = grad.detach().float().reshape(-1).cpu()
    first = torch.zeros(8)
    first[:min(8, flat.numel())] = flat[:8]
    return np.concatenate([[float(flat.double().norm())], first.numpy()]).astype(np.float32)


# ---- seeded random projections of a gradient tensor (VERDICT r4 #5a) -------------------------------------------------------------
# The fingerprint above pins the L2 norm and the first 8 elements: a wrong element past index 8 that preserves the norm to 2e-3 would
# pass.  NPROJ inner products <g, r_j> with fixed pseudo-random vectors r_j in [-1, 1) cover EVERY element for 4 more numbers per
# tensor.  r_j[i] is an integer hash of (i, j) — exact in numpy (uint64) and in torch (int64, on any device), so the generator (CPU,
# imported reference) and the GPU tests build bit-identical vectors without storing or transferring them.
NPROJ = 4


def _proj_hash(idx, j, xp):
    """idx: int64 / uint64 array of element indices -> values in [-1, 1) (float64).  32-bit multiply-xorshift, all arithmetic mod 2^32."""
    m = 0xFFFFFFFF
    x = (idx * 2654435761 + (j + 1) * 40503) & m
    x = x ^ (x >> 15)
    x = (x * 0x2C1B3C6D) & m
    x = x ^ (x >> 12)
    x = (x * 0x297A2D39) & m
    x = x ^ (x >> 15)
    return x


def proj_vector_np(n, j):
    x = _proj_hash(np.arange(n, dtype=np.uint64), j, np)
    return (x & np.uint64(0xFFFF)).astype(np.float64) / 32768.0 - 1.0


def projections(grad):
    """[NPROJ] float64: <grad.flatten(), r_j> accumulated in float64 (zeros for a missing gradient).  Works for numpy arrays and for
    torch tensors on any device (the hash runs where the tensor lives)."""
    out = np.zeros(NPROJ, dtype=np.float64)
    if grad is None:
        return out
    if torch.is_tensor(grad):
        flat = grad.detach().reshape(-1).double()
        idx = torch.arange(flat.numel(), dtype=torch.int64, device=flat.device)
        for j in range(NPROJ):
            r = (_proj_hash(idx, j, torch) & 0xFFFF).double() / 32768.0 - 1.0
            out[j] = float((flat * r).sum())
        return out
    flat = np.asarray(grad, dtype=np.float64).reshape(-1)
    for j in range(NPROJ):
        out[j] = float(np.dot(flat, proj_vector_np(flat.size, j)))
    return out


def check_projections(got, ref, norm, tol, what=''):
    """|<g, r_j> - reference| <= tol * ||g_ref|| for every j (an elementwise error e moves a projection by <e, r_j> ~ 0.58 ||e||)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max()
    assert err <= tol * float(norm) + 1e-9, (what, err, float(norm), list(got), list(ref))


def oracle_run(cfg, sd, batch, task, autocast_bf16=False):
    """Runs the oracle with autograd; returns (loss_vec, {name: grad}) for the parameter tensors in sd.
    autocast_bf16: the same restatement under stock torch.autocast(bfloat16) on the CPU — the yardstick the GPU tests use
    for what bf16 rounding alone does to each gradient tensor."""
    from oracle import goat_oracle
    if autocast_bf16:
        with torch.autocast('cpu', dtype=torch.bfloat16):
            return oracle_run(cfg, sd, batch, task)
    leaves = {}
    for k, v in sd.items():
        if v.is_floating_point():
            leaves[k] = v.clone().requires_grad_(True)
        else:
            leaves[k] = v
    leaves['mlm_head.predictions.decoder.weight'] = leaves['bert.embeddings.word_embeddings.weight']
    loss_vec = goat_oracle.forward(cfg, leaves, batch, task, compute_loss=True)
    loss_vec.mean().backward()
    grads = {k: v.grad for k, v in leaves.items() if torch.is_tensor(v) and v.requires_grad}
    return loss_vec.detach(), grads


# ---- host restatement of the pre-training update ---------------------------------------------------------------------------------
# clip_grad_norm_(max_norm) + the reference's AdamW (P/optim/adamw.py:53-110) in torch CPU ops.  tests/test_adamw_restatement.py pins it to
# tests/golden/adamw_trace.npz bit for bit; the GPU tests use it where the trace has no case (chunk boundaries, tails, views).
# torch's own composite ops (add_ with alpha, addcmul_, addcdiv_) fuse their multiply-add on some CPUs' vector kernels and not on others',
# so each is written out as the single roundings the trace holds: _fma where it fused (exact product and sum in float64, one rounding to
# float32 — the float64 sum's own rounding is 2^29 times finer), plain float32 ops elsewhere.
# The square root goes through float64 as well: torch's float32 sqrt is the correctly rounded one on some hosts and up to an ulp off on
# others (an EPYC 9575F differed from the trace in a sixth of the elements); the float64 root rounded to float32 is correct on all.
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def clip_adamw_step(params, grads, state, lr, weight_decay, betas=(0.9, 0.98), eps=1e-6, max_norm=5.0, norm=None):
    """One update, in place.  params: {name: float32 CPU tensor}; grads: {name: gradient} for the tensors that got one (the others are
    skipped: no moment update, no decay, their step count stays); state: {name: {'step', 'exp_avg', 'exp_avg_sq'}}, filled on first use;
    lr: this step's learning rate; weight_decay: {name: value}; norm: the total gradient norm as a float32 value if the caller has it
    (the order of a float32 sum of squares is torch's business and differs between CPUs), else computed here as clip_grad_norm_ does.
    -> the total gradient norm before clipping."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    grads = {n: grads[n] for n in params if n in grads}
    if norm is None:
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads.values()]))
    norm = torch.as_tensor(norm, dtype=torch.float32)
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)                    # clamp(max_norm / (norm + 1e-6), max = 1), multiplied in always
    b1, b2 = betas
    for n, g in grads.items():
        g = g * coef
        p = params[n]
        st = state.setdefault(n, {'step': 0, 'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)})
        st['step'] += 1                                       # the parameter's own count: a skipped step makes its bias correction lag
        m, v, t = st['exp_avg'], st['exp_avg_sq'], st['step']
        m.copy_(_fma(g, f32(1.0 - b1), m * f32(b1)))                         # exp_avg.mul_(beta1).add_(grad, alpha = 1 - beta1)
        v.copy_(_fma(g * f32(1.0 - b2), g, v * f32(b2)))                     # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        denom = v.double().sqrt().float() + f32(eps)                         # exp_avg_sq.sqrt().add_(eps)
        step_size = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        p.copy_(p + (f32(-step_size) * m) / denom)                           # p.addcdiv_(exp_avg, denom, value = -step_size)
        if weight_decay[n] > 0.0:
            p.copy_(_fma(f32(-lr * weight_decay[n]), p, p))                  # p.add_(p, alpha = -lr * weight_decay): decoupled, after the update
    return float(norm)


# ---- host restatement of the attention dropout mask ------------------------------------------------------------------------------
# Source of truth: HeadRng / GoatRng / goat_thr16 in csrc/common.hpp and AttnMask in csrc/attn_tile.hpp.  Integer arithmetic only, so
# the result is exact: the GPU tests compare the bits a kernel drew with it and build their float64 references from it.
_M32 = np.uint64(0xFFFFFFFF)
_MIX = np.uint64(0xD6E8FEB86659FD93)
_GOLD = 0x9E3779B97F4A7C15


def _mix64(x):
    """x: uint64 array -> {x ^= x >> 32; x *= MIX} twice, then x ^= x >> 32 (mod 2^64)."""
    s = np.uint64(32)
    x = x ^ (x >> s)
    x = x * _MIX
    x = x ^ (x >> s)
    x = x * _MIX
    return x ^ (x >> s)


def _mul32(x, c):
    return (x * np.uint64(c)) & _M32


def _thr16(p):
    """goat_thr16: (uint32_t)(p * 65536.0f + 0.5f) in float32"""
    return np.uint64(int(np.float32(np.float32(p) * np.float32(65536.0) + np.float32(0.5))))


def _goat_rng_keep(seed, ctr, thr16):
    """GoatRng(seed).keep(ctr, thr16) for a uint64 array of counters (any shape, any parity) -> bool array of that shape."""
    with np.errstate(over='ignore'):
        kk = _mix64(np.array([(seed * _GOLD + 0x632BE59BD9B4E019) & (2 ** 64 - 1)], dtype=np.uint64))[0]
        k0, k1 = kk & _M32, kk >> np.uint64(32)
        pair = ctr >> np.uint64(1)
        # __umul24(q >> 32, 0x9E3779): the low 24 bits of each operand, the low 32 bits of their product (zero below counter 2^33)
        hi24 = _mul32((pair >> np.uint64(32)) & np.uint64(0xFFFFFF), 0x9E3779 & 0xFFFFFF)
        x = (((pair & _M32) ^ k0) + hi24) & _M32
        x = x ^ (x >> np.uint64(16))
        x = _mul32(x, 0x7FEB352D)
        x = (x + k1) & _M32
        x = x ^ (x >> np.uint64(15))
        x = _mul32(x, 0x846CA68B)
        x = x ^ (x >> np.uint64(16))
    half = np.where((ctr & np.uint64(1)) != 0, x >> np.uint64(16), x & np.uint64(0xFFFF))
    return half >= thr16


def flat_keep_mask(seed, offset, n, p):
    """bool [n]: GoatRng(seed).keep(offset + i, goat_thr16(p)) for i < n — the mask of every row kernel of csrc/dropout_act.hip and csrc/layernorm.hip (dropout,
    activation backward, LayerNorm input and output dropout), for BOTH dtypes: element i of the flat tensor owns counter offset + i
    (mod 2^64).  `seed` is the effective one (the call's seed + *rng_dev); any offset parity, counters of any size."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    with np.errstate(over='ignore'):
        ctr = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    return _goat_rng_keep(seed, ctr, _thr16(p))


def attn_keep_mask(dtype, seed, offset, B, nh, Lq, Lk, p):
    """bool [B, nh, Lq, Lk]: True where goat_attn_fwd / goat_attn_bwd keep probability (b, h, q, key) under (seed, offset), `seed`
    being the effective one (the call's seed + *rng_dev).  dtype: torch.bfloat16 (HeadRng: a 32-bit key per (b, h), one hash per pair of
    q * Lk + key) or torch.float32 (GoatRng: one flat 64-bit counter stream from `offset`, as flat_keep_mask)."""
    thr16 = _thr16(p)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    bh = np.arange(B * nh, dtype=np.uint64)[:, None]
    idx = np.arange(Lq * Lk, dtype=np.uint64)[None, :]
    if dtype == torch.float32:
        with np.errstate(over='ignore'):
            ctr = np.uint64(offset) + bh * np.uint64(Lq * Lk) + idx
        return _goat_rng_keep(seed, ctr, thr16).reshape(B, nh, Lq, Lk)
    with np.errstate(over='ignore'):
        if dtype == torch.bfloat16:
            x0 = np.uint64((seed + _GOLD * (offset + 1)) & (2 ** 64 - 1))
            k = _mix64(x0 ^ (bh * _MIX)) & _M32
            x = (idx >> np.uint64(1)) ^ k
            x = _mul32(x, 0x7FEB352D)
            x = x ^ (x >> np.uint64(15))
            x = _mul32(x, 0x846CA68B)
            x = x ^ (x >> np.uint64(16))
        else:
            raise ValueError(dtype)
    half = np.where((idx & np.uint64(1)) != 0, x >> np.uint64(16), x & np.uint64(0xFFFF))
    return (half >= thr16).reshape(B, nh, Lq, Lk)
