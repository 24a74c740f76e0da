"""helpers.attn_keep_mask — the host restatement of the attention dropout bits (HeadRng / GoatRng in csrc/common.hpp, AttnMask in
csrc/attn_tile.hpp) — against pins from a C++ transcription of the two structs compiled for the host.  The GPU tests
(test_attention_dropout_gpu.py) compare the kernels with it; this file keeps the restatement itself from drifting.

helpers.flat_keep_mask — GoatRng::keep(offset + i, goat_thr16(p)), the mask of every row kernel (test_row_dropout_gpu.py) — is pinned the
same way: FLAT_PIN was printed by a host C++ transcription of GoatRng and goat_thr16 (__umul24 written as the product of the low 24 bits
of each operand, mod 2^32), compiled outside the repository and not committed.  It covers offset 0, an odd offset, a range that
straddles counter 2^33 (where the high word of the pair index first becomes non-zero), 2^33 + 8, 2^40 + 3 and a counter whose high pair
word exceeds 24 bits."""
import numpy as np
import pytest
import torch

from helpers import attn_keep_mask, flat_keep_mask

# seed 1234, offset 0, B 2, nh 3, Lq 5, Lk 7, p 0.3; flattened in (b, h, q, key) order
PIN = {
    torch.bfloat16: '1111010111110101110111110101111100101011111111111000101011001110011101110101101010101111101101110101001010110111110101110'
                    '11100011101010111010011110111110110001111111101111110010111011111111111010110101101110111',
    torch.float32: '1110111011101010011110100101101011110010001010111101111111011111011111111011110111001111000010010110110111010101101110000'
                   '11110101101010111011111100011111101111111111111010101000101011111111101100011101011101110',
}


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_mask_matches_the_pinned_bits(dtype):
    m = attn_keep_mask(dtype, 1234, 0, 2, 3, 5, 7, 0.3)
    assert m.shape == (2, 3, 5, 7) and m.dtype == np.bool_
    assert ''.join('1' if v else '0' for v in m.reshape(-1)) == PIN[dtype]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_heads_samples_offsets_and_seeds_draw_their_own_masks(dtype):
    m = attn_keep_mask(dtype, 1234, 0, 2, 3, 33, 65, 0.3).reshape(6, -1)
    for i in range(6):
        for j in range(i + 1, 6):
            # two independent masks of 2145 elements agree on 0.58 of them (0.7^2 + 0.3^2), +- 0.011
            assert 0.5 < (m[i] == m[j]).mean() < 0.66, (i, j)
    other = attn_keep_mask(dtype, 1234, 8, 2, 3, 33, 65, 0.3).reshape(6, -1)
    assert 0.5 < (m == other).mean() < 0.66
    other = attn_keep_mask(dtype, 1235, 0, 2, 3, 33, 65, 0.3).reshape(6, -1)
    assert 0.5 < (m == other).mean() < 0.66


def test_float32_heads_continue_one_counter_stream():
    """GoatRng: head bh of an [Lq, Lk] problem starts where head bh - 1 ended, and `offset` shifts the whole stream."""
    m = attn_keep_mask(torch.float32, 77, 0, 2, 3, 5, 7, 0.3).reshape(-1)
    flat = attn_keep_mask(torch.float32, 77, 0, 1, 1, 1, 2 * 3 * 5 * 7, 0.3).reshape(-1)
    assert np.array_equal(m, flat)
    shifted = attn_keep_mask(torch.float32, 77, 8, 1, 1, 1, 2 * 3 * 5 * 7 - 8, 0.3).reshape(-1)
    assert np.array_equal(flat[8:], shifted)


def test_drop_rate():
    m = attn_keep_mask(torch.bfloat16, 99, 8, 4, 12, 33, 65, 0.1)
    assert m.size == 102960 and int((~m).sum()) == 10269          # 0.0997378


def test_threshold_edges():
    assert attn_keep_mask(torch.bfloat16, 1, 0, 1, 2, 9, 9, 0.0).all()
    # thr16 = 65536 > every 16-bit half
    assert not attn_keep_mask(torch.float32, 1, 0, 1, 2, 9, 9, 1.0).any()


# (seed, offset, n, p) -> keep bits of counters offset .. offset + n - 1
FLAT_PIN = {
    (1234, 0, 96, 0.3): '111011101110101001111010010110101111001000101011110111111101111101111111101111011100111100001001',
    (1234, 13, 96, 0.1): '111111111101111111111111110111111111111111111111111011111111011110111111111001110111110110111011',
    (77, 2 ** 33 - 5, 96, 0.3): '111011001011110110101011011000111101101111011111000100110101111111111000111111011011111101110000',
    (77, 2 ** 33 + 8, 96, 0.2): '111111011110110001111011011110111110001101111011111111110011111110111111111011100001111011110011',
    (77, 2 ** 40 + 3, 96, 0.25): '100001111101010111111111111111011111111111010011101010111111100111110111011011110011111110111111',
    (2 ** 63 - 1, 2 ** 57 + 8, 96, 0.1): '111011111100111111101111101111111111111111111111111111111111111111111111111111101111111111111111',
}


@pytest.mark.parametrize('key', list(FLAT_PIN), ids=['seed%d-off%d-p%g' % (k[0], k[1], k[3]) for k in FLAT_PIN])
def test_flat_mask_matches_the_pinned_bits(key):
    m = flat_keep_mask(*key)
    assert m.shape == (key[2],) and m.dtype == np.bool_
    assert ''.join('1' if v else '0' for v in m) == FLAT_PIN[key]


@pytest.mark.parametrize('offset', [0, 8, 13, 2 ** 33 - 5, 2 ** 33 + 8, 2 ** 40 + 3])
def test_flat_mask_is_one_counter_stream(offset):
    """flat_keep_mask(s, o, n, p)[k:] == flat_keep_mask(s, o + k, n - k, p) for even and odd k: the identity by which the GPU tests
    make the mask of a window of a large tensor."""
    n = 301
    full = flat_keep_mask(99, offset, n, 0.2)
    for k in (1, 2, 7, 8, 150, 299):
        assert np.array_equal(full[k:], flat_keep_mask(99, offset + k, n - k, 0.2)), k


@pytest.mark.parametrize('offset', [0, 8, 13, 2 ** 33 - 5, 2 ** 33 + 8, 2 ** 40 + 3])
def test_flat_mask_is_the_float32_attention_stream(offset):
    n = 211
    flat = flat_keep_mask(1234, offset, n, 0.3)
    assert np.array_equal(flat, attn_keep_mask(torch.float32, 1234, offset, 1, 1, 1, n, 0.3).reshape(-1))


def test_flat_mask_high_counter_word_changes_the_bits():
    """the __umul24 term: counters 2^33 apart share the low pair word and must still draw unrelated masks"""
    a, b = flat_keep_mask(5, 8, 4096, 0.3), flat_keep_mask(5, 2 ** 33 + 8, 4096, 0.3)
    assert 0.5 < (a == b).mean() < 0.66          # independent masks agree on 0.58 of 4096 elements, +- 0.008
    # 2^24 << 33 apart: the 24-bit multiply no longer sees the difference (documented behaviour of __umul24, period 2^57)
    assert np.array_equal(a, flat_keep_mask(5, 2 ** 57 + 8, 4096, 0.3))


def test_flat_mask_drop_rate_and_threshold_edges():
    m = flat_keep_mask(99, 2 ** 33 + 8, 100000, 0.1)
    assert abs((~m).mean() - 0.1) < 0.004         # 4 sigma of 100 000 draws
    assert flat_keep_mask(1, 3, 77, 0.0).all()
    assert not flat_keep_mask(1, 3, 77, 1.0).any()


def test_row_dropout_case_table_covers_every_width_and_form():
    """the case table of test_row_dropout_gpu.py (a GPU module): its coverage conditions hold wherever the suite runs"""
    import test_row_dropout_gpu
    test_row_dropout_gpu.check_ln_table()
