"""KV-cached, graph-replayed decoding of the speaker on the GPU: goat_attn_decode_fwd and goat_decode_select against plain torch,
the device-side position under graph replay, the dropout statistics, IncrementalDecoder pinned to the reference's golden logits
(tests/golden/speaker_small.npz), and infer_batch_cached against the unchanged prefix form infer_batch.

Tolerances.  Attention outputs: tests/test_hip_ops.py's bounds for attention outputs in the same dtype — max error over the largest
|reference| entry below 1e-3 (float32) / 2e-2 (bfloat16); the reference is float64.  Golden logits: tests/test_speaker.py's bound for
the full forward, 1e-3 (float32) / 2e-2 (bfloat16) times max(1, max|ref|).  Everything else is exact (bitwise or integer)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
DEV = 'cuda'
POSITIONS = (0, 1, 31, 32, 63, 64, 65, 255, 256, 511)      # the wave and tile edges of the kernel's layouts
VOCAB, FEAT = 300, 768 + 128


def _tol(dtype):
    return 1e-3 if dtype == torch.float32 else 2e-2


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


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


# ------------------------------------------------------------------------------------------------ goat_attn_decode_fwd
def _decode_case(nh, dtype, t, Lmax=512, B=3, seed=0):
    """q, kv_new, a cache whose rows >= t are NaN (row t is written by the call, the tail must never be read), kmask whose tail is NaN:
    row 1 has every visible key at -1e9, row 2 every third key."""
    g = torch.Generator().manual_seed(1000 * nh + t + seed)
    H = nh * 64
    q = (torch.randn(B, H, generator=g) * 0.7).to(DEV, dtype)
    kv = (torch.randn(B, 2 * H, generator=g) * 0.7).to(DEV, dtype)
    cache = (torch.randn(B, Lmax, 2 * H, generator=g) * 0.7).to(DEV, dtype)
    cache[:, t:] = float('nan')
    kmask = torch.zeros(B, Lmax)
    kmask[1, :t + 1] = -1e9
    kmask[2, 1:t + 1:3] = -1e9
    kmask[:, t + 1:] = float('nan')
    return q, kv, cache, kmask.to(DEV)


def _decode_ref(q, kv, cache, kmask, t, nh):
    """float64: plain softmax over the first t + 1 keys; masked keys are REMOVED (score -inf), a row with every key masked is the
    mean of its V rows."""
    B, H = q.shape
    full = cache.double().clone()
    full[:, t] = kv.double()
    k = full[:, :t + 1, :H].reshape(B, t + 1, nh, 64)
    v = full[:, :t + 1, H:].reshape(B, t + 1, nh, 64)
    s = torch.einsum('bhd,bkhd->bhk', q.double().reshape(B, nh, 64), k) / math.sqrt(64.0)
    masked = (kmask[:, :t + 1] < -1e8)                                  # [B, t + 1]
    allm = masked.all(1)
    s = s.masked_fill((masked & ~allm[:, None])[:, None, :], float('-inf'))
    p = torch.softmax(s, -1)
    p = torch.where(allm[:, None, None], torch.full_like(p, 1.0 / (t + 1)), p)
    return torch.einsum('bhk,bkhd->bhd', p, v).reshape(B, H)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('nh', [4, 12])
def test_attn_decode_matches_float64_torch(ops, dtype, nh):
    worst = 0.0
    for t in POSITIONS:
        q, kv, cache, kmask = _decode_case(nh, dtype, t)
        before = cache.clone()
        pos = torch.tensor([t], dtype=torch.int32, device=DEV)
        o = ops.attn_decode(q, kv, cache, kmask, pos, nh, 0.0)
        assert o.shape == q.shape and bool(torch.isfinite(o.float()).all()), t
        ref = _decode_ref(q, kv, before, kmask, t, nh)
        err = float((o.double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err < _tol(dtype), (t, err)
        # the all-masked row is the mean of its V rows (row t being kv_new)
        full = before.double().clone()
        full[:, t] = kv.double()
        mean_v = full[1, :t + 1, nh * 64:].mean(0)
        assert float((o[1].double() - mean_v).abs().max()) < _tol(dtype) * float(ref.abs().max()), t
        # the cache: row t is kv_new bit for bit, every other row (the NaN tail included) is bit-unchanged
        assert torch.equal(_bits(cache[:, t]), _bits(kv)), t
        keep = torch.ones(cache.shape[1], dtype=torch.bool, device=DEV)
        keep[t] = False
        assert torch.equal(_bits(cache[:, keep]), _bits(before[:, keep])), t
        assert int(pos.item()) == t
    print('attn_decode parity %s nh=%d: max err / max|ref| over positions %s = %.3e (bound %.0e)'
          % (str(dtype).replace('torch.', ''), nh, POSITIONS, worst, _tol(dtype)))


def test_attn_decode_without_mask_and_strided_cache(ops):
    """kmask None, and a cache that is a column view of a wider buffer (row stride 2 * its width)."""
    nh, t, dtype = 4, 37, torch.bfloat16
    q, kv, cache, kmask = _decode_case(nh, dtype, t, Lmax=40)
    wide = torch.full((3, 40, 4 * nh * 64), float('nan'), dtype=dtype, device=DEV)
    view = wide[:, :, 2 * nh * 64:]
    view.copy_(cache)
    pos = torch.tensor([t], dtype=torch.int32, device=DEV)
    o = ops.attn_decode(q, kv, view, None, pos, nh, 0.0)
    ref = _decode_ref(q, kv, cache, torch.zeros_like(kmask), t, nh)
    assert float((o.double() - ref).abs().max() / ref.abs().max()) < _tol(dtype)
    assert torch.equal(_bits(view[:, t]), _bits(kv)) and bool(torch.isnan(wide[:, :, :2 * nh * 64].float()).all())


def test_attn_decode_reads_the_position_on_the_device(ops):
    """One captured call, replayed five times across a wave edge with `pos` advanced on the device and q / kv_new refreshed by copy_ into
    the static inputs: every replay equals the eager call at that position bit for bit (output and cache)."""
    nh, dtype, t0, Lmax = 4, torch.bfloat16, 29, 48
    q0, kv0, cache0, kmask = _decode_case(nh, dtype, t0, Lmax=Lmax)
    kmask = torch.zeros_like(kmask)
    kmask[2, 1::3] = -1e9
    cache0 = torch.nan_to_num(cache0, nan=0.25)
    sq, skv, scache = q0.clone(), kv0.clone(), cache0.clone()
    pos = torch.tensor([t0], dtype=torch.int32, device=DEV)
    ops.attn_decode(sq, skv, cache0.clone(), kmask, pos, nh, 0.0)          # warm-up on a scratch cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph(g):
        so = ops.attn_decode(sq, skv, scache, kmask, pos, nh, 0.0)
    ecache = cache0.clone()
    for i in range(5):
        t = t0 + i
        q, kv, _, _ = _decode_case(nh, dtype, t, Lmax=Lmax, seed=77)
        sq.copy_(q)
        skv.copy_(kv)
        g.replay()
        eo = ops.attn_decode(q, kv, ecache, kmask, torch.tensor([t], dtype=torch.int32, device=DEV), nh, 0.0)
        assert int(pos.item()) == t
        assert torch.equal(_bits(so), _bits(eo)), t
        assert torch.equal(_bits(scache), _bits(ecache)), t
        pos.add_(1)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_attn_decode_dropout_is_unbiased_and_reproducible(ops, rng_state, dtype):
    """p = 0.5, t = 63, zero scores, V rows the 64 one-hot vectors: output component d is the (dropped-out) probability of key d."""
    B, nh, t, p = 3, 4, 63, 0.5
    H = nh * 64
    q = torch.zeros(B, H, dtype=dtype, device=DEV)
    cache = torch.zeros(B, 64, 2 * H, dtype=dtype, device=DEV)
    cache[:, :, H:] = torch.eye(64, dtype=dtype, device=DEV).repeat(1, nh).unsqueeze(0)
    kv = cache[:, t].clone()
    pos = torch.tensor([t], dtype=torch.int32, device=DEV)

    def draw():
        return ops.attn_decode(q, kv, cache, None, pos, nh, p).float()

    ops.manual_seed(1234)
    o1 = draw()
    o2 = draw()
    ops.manual_seed(1234)
    o3 = draw()
    kept = 1.0 / (64 * (1 - p))
    assert bool(((o1 == 0) | ((o1 - kept).abs() < 1e-6)).all())
    n = o1.numel()
    share = float((o1 == 0).float().mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print('attn_decode dropout %s: share of zeros %.4f over %d components (p = %.2f, 5 sigma = %.4f)' % (dtype, share, n, p, 5 * sigma))
    assert abs(share - p) <= 5 * sigma
    assert torch.equal(o1, o3)                      # same (seed, offset): same bits
    assert not torch.equal(o1, o2)                  # a second draw: other bits
    # the mask is per (sample, head, key), not shared
    assert not torch.equal(o1[0, :64], o1[0, 64:128]) and not torch.equal(o1[0], o1[1])


# ------------------------------------------------------------------------------------------------ goat_decode_select
def _expected_word(logits, V, unk):
    x = logits[:, :V].clone()
    x[:, unk] = float('-inf')
    mx = x.max(1, keepdim=True).values
    cols = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == mx, cols, torch.full_like(cols, V)).min(1).values         # the LOWEST index among the maxima


@pytest.mark.parametrize('V', [2, 300, 2049])
def test_decode_select_greedy(ops, V):
    ld = (V + 63) // 64 * 64
    B, Lmax, t = 6, 8, 4
    pad, unk, eos = (0, 1, 5) if V == 2 else (0, 3, 2)              # (V = 2: <EOS> is outside the vocabulary and never emitted)
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(B, ld, generator=g)
    logits[:, V:] = 1e9                                             # padding columns must never be read
    if V > 2:
        logits[1, 7] = logits[1, V - 1] = 50.0                      # a tie: the lowest index wins
        logits[2, unk] = 60.0                                       # <UNK> holds the maximum: the second best is chosen
        logits[2, 11] = 40.0
        logits[4, eos] = 45.0                                       # this row emits <EOS>
    logits = logits.to(DEV)
    st = ops.DecodeState(B, Lmax, DEV)
    st.words.fill_(-7)
    st.kmask.fill_(5.0)
    st.pos.fill_(t)
    st.ended[3] = 1
    st.end_step[3] = 1
    st.n_live.fill_(-1)
    ops.decode_select(logits, st, unk, eos, pad, sampling=False, n_valid=V)
    want = _expected_word(logits, V, unk)
    want[3] = pad
    if V > 2:
        assert want.tolist()[1:5] == [7, 11, pad, eos]
        nomask = logits[:, :V].clone()
        nomask[:, unk] = float('-inf')
        assert torch.equal(want[[0, 5]], nomask.argmax(1)[[0, 5]])                    # rows without ties: torch.argmax
    assert torch.equal(st.words[:, t + 1], want)
    assert torch.equal(st.kmask[:, t + 1], torch.where(want == pad, -1e9, 0.0).float())
    cols = [c for c in range(Lmax) if c != t + 1]
    assert bool((st.words[:, cols] == -7).all()) and bool((st.kmask[:, cols] == 5.0).all())
    ended = [0, 0, 0, 1, int(V > 2), 0]
    assert st.ended.tolist() == ended
    assert st.end_step.tolist() == [-1, -1, -1, 1, t if V > 2 else -1, -1]
    assert int(st.pos.item()) == t + 1
    assert int(st.n_live.item()) == B - sum(ended)


def test_decode_select_sampling_follows_the_softmax(ops, rng_state):
    V, ld, n, unk = 8, 64, 20000, 3
    row = torch.tensor([0.3, -1.2, 1.1, 5.0, 0.0, 2.0, -0.4, 0.9])
    logits = torch.full((n, ld), 1e9)
    logits[:, :V] = row
    logits = logits.to(DEV)
    st = ops.DecodeState(n, 2, DEV)
    ops.manual_seed(99)
    ops.decode_select(logits, st, unk, 100, 101, sampling=True, n_valid=V)
    first = st.words[:, 1].clone()
    st.pos.zero_()
    ops.decode_select(logits, st, unk, 100, 101, sampling=True, n_valid=V)
    assert not torch.equal(first, st.words[:, 1])                   # the next offset: another draw
    x = row.clone()
    x[unk] = float('-inf')
    prob = torch.softmax(x.double(), 0)
    freq = torch.bincount(first.cpu(), minlength=V).double() / n
    assert freq.numel() == V and float(freq[unk]) == 0.0            # <UNK> is never drawn
    for w in range(V):
        sigma = math.sqrt(float(prob[w]) * (1 - float(prob[w])) / n)
        print('decode_select sampling: word %d frequency %.4f, softmax %.4f, 5 sigma %.4f' % (w, float(freq[w]), float(prob[w]), 5 * sigma))
        assert abs(float(freq[w]) - float(prob[w])) <= 5 * sigma, w
    assert int(st.n_live.item()) == n


# ------------------------------------------------------------------------------------------------ pinned to the reference
def _golden_model():
    import make_golden_speaker as mg
    from vln_goat_amd import speaker
    cfg = speaker.default_config(speaker_dropout=0.0, featdropout=0.0)
    torch.manual_seed(0)
    m = speaker.Transpeaker(FEAT, 512, 256, VOCAB, cfg)
    m.load_state_dict(mg.seeded_state(m.state_dict()))
    return m.cuda().eval(), mg


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_incremental_decoder_matches_reference_golden(dtype):
    """IncrementalDecoder driven teacher-forced over the fixture's instructions (rows of 12, 9 and 6 tokens with <PAD> tails): the
    projection logits of every step against the IMPORTED REFERENCE's, with and without the context mask; then greedy decoding."""
    import vln_goat_amd
    from vln_goat_amd import speaker
    z = np.load(os.path.join(HERE, 'golden', 'speaker_small.npz'))
    m, mg = _golden_model()
    can, img, insts, ctx_mask = mg.inputs()
    can, img, insts = torch.from_numpy(can).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(insts).cuda()
    B, L = insts.shape
    vln_goat_amd.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            _, enc = m.encoder(can, img, True)
        dec = speaker.IncrementalDecoder(m, B, L, enc.shape[1])
        for tag, cm in (('nomask', None), ('ctxmask', torch.from_numpy(ctx_mask).cuda())):
            dec.start(enc, insts[:, 0], 0, cm)
            steps = []
            for s in range(L):
                dec.step(unk=3, eos=2, pad=0)
                steps.append(dec.logits.clone())
                if s + 1 < L:
                    dec.force(insts[:, s + 1])
            logits = torch.stack(steps, 1).cpu().numpy()
            ref = z[tag + '_logits']
            err = float(np.abs(logits - ref).max())
            print('IncrementalDecoder %s %s: max |logits - reference| = %.3e (bound %.3e)'
                  % (str(dtype).replace('torch.', ''), tag, err, _tol(dtype) * max(1.0, np.abs(ref).max())))
            assert err <= _tol(dtype) * max(1.0, np.abs(ref).max()), tag
            assert torch.equal(dec.state.words[:, :L], insts)
        if dtype == torch.float32:
            words = speaker.infer_batch_cached(m, can, img, bos=1, eos=2, pad=0, unk=3, max_decode=10, already_dropfeat=True)
            assert np.array_equal(words.cpu().numpy(), z['greedy_words'])
    finally:
        vln_goat_amd.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ the prefix form
SMALL = dict(B=8, T=3, F=64, hidden=64, word=64, vocab=12, max_decode=32, seed=4, scale=1.0)     # (seed / scale: see _small_case)


def _small_case(batch_seed=0):
    """A seeded small speaker (2 layers, 2 heads, vocabulary 12) and a batch of random features.  The seed and the weight scale were
    chosen so that the unchanged infer_batch ends its rows at several different steps before max_decode; the test asserts that."""
    from vln_goat_amd import speaker
    c = SMALL
    cfg = speaker.default_config(h_dim=c['hidden'], wemb=c['word'], proj_hidden=128, speaker_layer_num=2, speaker_head_num=2,
                                 speaker_dropout=0.0, featdropout=0.0, image_feat_size=48)
    torch.manual_seed(c['seed'])
    m = speaker.Transpeaker(c['F'], c['hidden'], c['word'], c['vocab'], cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.mul_(c['scale'])
    g = torch.Generator().manual_seed(100 + batch_seed)
    can = torch.randn(c['B'], c['T'], c['F'], generator=g).cuda()
    img = torch.randn(c['B'], c['T'], 36, c['F'], generator=g).cuda()
    return m.cuda().eval(), can, img


def _end_steps(words, eos):
    """per row the column of its first <EOS> (or -1)"""
    hit = (words == eos)
    first = torch.where(hit.any(1), hit.float().argmax(1), torch.full((words.shape[0],), -1, device=words.device))
    return first.tolist()


def test_infer_batch_cached_equals_the_prefix_form():
    from vln_goat_amd import speaker
    m, can, img = _small_case()
    md = SMALL['max_decode']
    kw = dict(bos=1, eos=2, pad=0, unk=3, max_decode=md)
    want = speaker.infer_batch(m, can, img, **kw)
    ends = _end_steps(want, 2)
    print('prefix form: rows end at columns %s of %d' % (ends, want.shape[1]))
    # the precondition: early stopping is exercised — every row ends, at two or more different steps, all before max_decode
    assert min(ends) > 0 and len(set(ends)) >= 2 and want.shape[1] < md + 1, ends
    for check_every in (1, 8):
        got = speaker.infer_batch_cached(m, can, img, check_every=check_every, **kw)
        assert got.dtype == torch.int64 and torch.equal(got, want), check_every
    # a case that never ends: <EOS> outside the vocabulary, both forms run to max_decode
    kw['eos'] = 100
    full = speaker.infer_batch(m, can, img, **kw)
    assert full.shape[1] == md + 1
    assert torch.equal(speaker.infer_batch_cached(m, can, img, **kw), full)


def test_one_decoder_serves_two_batches_and_eager_equals_replay():
    from vln_goat_amd import speaker
    m, can, img = _small_case()
    _, can2, img2 = _small_case(batch_seed=1)
    c = SMALL
    kw = dict(bos=1, eos=2, pad=0, unk=3, max_decode=c['max_decode'])
    replayed = speaker.IncrementalDecoder(m, c['B'], c['max_decode'], c['T'])
    eager = speaker.IncrementalDecoder(m, c['B'], c['max_decode'], c['T'], use_graph=False)
    for a, b in ((can, img), (can2, img2)):
        want = speaker.infer_batch(m, a, b, **kw)
        got = speaker.infer_batch_cached(m, a, b, decoder=replayed, **kw)
        assert torch.equal(got, want)
        assert torch.equal(speaker.infer_batch_cached(m, a, b, decoder=eager, **kw), got)       # eager stepping == graph replay
    assert len(replayed._graphs) == 1 and not eager._graphs                                     # one capture served both batches
    assert not torch.equal(speaker.infer_batch(m, can, img, **kw), speaker.infer_batch(m, can2, img2, **kw))
    with pytest.raises(ValueError):
        speaker.infer_batch_cached(m, can[:4], img[:4], decoder=replayed, **kw)
