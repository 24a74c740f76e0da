"""Sampled decoding through IncrementalDecoder / infer_batch_cached (sampling=True) at dropout 0.

A captured step bakes in the (seed, offset) the word choice was given at capture; what makes a REPLAY draw new Gumbel noise is the device
counter the step bumps.  The model here has a zero projection, so the logits are the same (all zero) for every row at every step and
every word is a draw from the uniform distribution over the vocabulary without <UNK>: if the noise did not change from step to step,
every column of `words` after the capture would repeat the one before it.

Bounds.  Two independent columns of B = 64 draws over 11 words coincide with probability 11^-64; the pooled word frequencies over
n = B x max_decode independent draws lie within 5 sigma of 1/11, sigma = sqrt(q (1 - q) / n) (the bound of the kernel's own sampling test)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, F, VOCAB, MAX_DECODE = 64, 3, 64, 12, 32
BOS, EOS, PAD, UNK = 1, 100, 0, 3          # <EOS> outside the vocabulary: no row ends, every step draws for every row


@pytest.fixture(scope='module')
def case():
    from vln_goat_amd import speaker
    cfg = speaker.default_config(h_dim=64, wemb=64, proj_hidden=128, speaker_layer_num=2, speaker_head_num=2,
                                 speaker_dropout=0.0, featdropout=0.0, image_feat_size=48)
    torch.manual_seed(4)
    m = speaker.Transpeaker(F, 64, 64, VOCAB, cfg)
    with torch.no_grad():
        m.projection.weight.zero_()
    g = torch.Generator().manual_seed(100)
    can = torch.randn(B, T, F, generator=g).cuda()
    img = torch.randn(B, T, 36, F, generator=g).cuda()
    return m.cuda().eval(), can, img


@pytest.fixture()
def rng_state():
    """the process-wide dropout counter state, put back after the test"""
    from vln_goat_amd import hipops as ops
    saved = (ops.RngState.seed, ops.RngState.base, ops.RngState.counter, ops.RngState.dev)
    ops.manual_seed(7)
    yield ops.RngState
    ops.RngState.seed, ops.RngState.base, ops.RngState.counter, ops.RngState.dev = saved


def _check_draws(words, tag):
    assert words.shape == (B, MAX_DECODE + 1) and bool((words[:, 0] == BOS).all())
    drawn = words[:, 1:]
    assert int(drawn.min()) >= 0 and int(drawn.max()) < VOCAB and not bool((drawn == UNK).any())
    same = [s for s in range(MAX_DECODE - 1) if torch.equal(drawn[:, s], drawn[:, s + 1])]
    assert not same, '%s: steps %s repeat the draw of the step before for every row' % (tag, same)
    n, q = drawn.numel(), 1.0 / (VOCAB - 1)
    sigma = math.sqrt(q * (1 - q) / n)
    freq = torch.bincount(drawn.reshape(-1).cpu(), minlength=VOCAB).double() / n
    for w in range(VOCAB):
        if w != UNK:
            print('%s: word %d frequency %.4f, uniform %.4f, 5 sigma %.4f' % (tag, w, float(freq[w]), q, 5 * sigma))
            assert abs(float(freq[w]) - q) <= 5 * sigma, (tag, w)


@pytest.mark.parametrize('use_graph', [True, False])
def test_sampled_decoding_draws_new_noise_at_every_step(case, rng_state, use_graph):
    from vln_goat_amd import hipops, speaker
    m, can, img = case
    outer = hipops.RngState.dev
    dec = speaker.IncrementalDecoder(m, B, MAX_DECODE, T, use_graph=use_graph)
    kw = dict(bos=BOS, eos=EOS, pad=PAD, unk=UNK, max_decode=MAX_DECODE, sampling=True, decoder=dec)
    first = speaker.infer_batch_cached(m, can, img, **kw)
    _check_draws(first, 'graph replay' if use_graph else 'eager')
    second = speaker.infer_batch_cached(m, can, img, **kw)             # the same decoder (and graph), the same logits: other words
    _check_draws(second, 'second batch')
    assert not torch.equal(first, second)
    assert len(dec._graphs) == (1 if use_graph else 0)
    assert hipops.RngState.dev is outer                                 # the decoder's counter does not stay installed


def test_decoder_accepts_a_counter_of_the_caller(case, rng_state):
    from vln_goat_amd import speaker
    m, can, img = case
    ctr = torch.zeros(1, dtype=torch.int64, device='cuda')
    dec = speaker.IncrementalDecoder(m, B, MAX_DECODE, T, rng_dev=ctr)
    speaker.infer_batch_cached(m, can, img, bos=BOS, eos=EOS, pad=PAD, unk=UNK, max_decode=MAX_DECODE, sampling=True, decoder=dec)
    assert int(ctr.item()) == MAX_DECODE * 0x9E3779B1                   # one bump per step, eager or replayed
    with pytest.raises(ValueError):
        speaker.IncrementalDecoder(m, B, MAX_DECODE, T, rng_dev=torch.zeros(1, dtype=torch.int32, device='cuda'))
