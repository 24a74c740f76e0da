"""helpers.attn_keep_mask — the host restatement of the attention dropout bits (HeadRng / GoatRng in csrc/common.hpp, AttnMask in
csrc/attn_tile.hpp) — against pins from a C++ transcription of the two structs compiled for the host.  The GPU tests
(test_attention_dropout_gpu.py) compare the kernels with it; this file keeps the restatement itself from drifting."""
import numpy as np
import pytest
import torch

from helpers import attn_keep_mask

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
