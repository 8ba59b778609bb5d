"""The visibility bitsets of a forward (int64 [T, max_slots / 64]: bit s % 64 of word s // 64 = slot s visible) are packed in one place,
`model.pack_vis_bits`; the torch wrapper the tests use and the host-mask path both go through it.  Pinned here to a bit-by-bit loop."""
import numpy as np
import pytest
import torch

from atspeed_amd.model import pack_vis_bits, vis_bits_from_bool


@pytest.mark.parametrize("T,S,max_slots", [(1, 1, 64), (3, 63, 64), (6, 64, 128), (9, 100, 256), (5, 130, 512), (4, 511, 512)])
def test_shared_packing_equals_a_bit_by_bit_loop(T, S, max_slots):
    rng = np.random.default_rng(1000 * T + S)
    vis = rng.random((T, S)) < 0.5
    if S >= 64:
        vis[0, 63] = True                                  # the sign bit of word 0
        vis[-1, :64] = True                                # a full word: -1
    want = np.zeros((T, max_slots // 64), dtype=np.int64)
    for r in range(T):
        for w in range(max_slots // 64):
            word = 0
            for b in range(64):
                if 64 * w + b < S and vis[r, 64 * w + b]:
                    word |= 1 << b
            want[r, w] = word - (1 << 64) if word >> 63 else word
    got = pack_vis_bits(vis, max_slots)
    assert got.dtype == np.int64 and got.shape == want.shape and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want)
    t = vis_bits_from_bool(torch.from_numpy(vis), max_slots)
    assert t.dtype == torch.int64 and t.is_contiguous() and np.array_equal(t.numpy(), want)
