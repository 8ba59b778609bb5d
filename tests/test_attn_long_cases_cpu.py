"""tests/attn_long_cases.py without a GPU: every visibility edge and every placed query row the GPU tests rely on is present (by count), the
placed rows have the softmax they were placed for, and the numpy reference is torch's float64 softmax attention."""
import numpy as np
import pytest
import torch

from tests import attn_long_cases as LC, segs_cases as SC

SHAPES = [(4, 64), (2, 128)]


def test_existing_fixtures_keep_their_values():
    assert (SC.MAX_SLOTS, SC.LAYERS, SC.VIS_WORDS) == (256, 2, 4)
    assert SC.vis_words(np.ones((3, 70), dtype=bool)).shape == (3, 4)


def test_long7_shape():
    sg = LC.table("long7", 32)
    assert sg["max_slots"] == 2048 and sg["vis_words"] == 32
    assert list(zip(sg["n_tok"], sg["n_slots"])) == [(40, 2048), (64, 2047), (33, 1985), (65, 577), (20, 1536), (130, 1473), (1, 2048)]
    assert sg["total_tok"] == 353 and sg["total_tok"] & 1
    for s, n in zip(sg["segs"], sg["n_slots"]):
        assert s["vis"].shape[1] == n and s["bits"].shape[1] == 2048
        assert np.array_equal(s["bits"][:, :n], s["vis"])
        assert LC.bit_words(s["bits"]).shape == (s["vis"].shape[0], 32)
    w = LC.bit_words(sg["segs"][2]["bits"])                     # bit j of word w = slot 64 w + j
    assert ((w[32] >> np.uint64(600 % 64)) & np.uint64(1))[600 // 64] == 1 and not w[32, :8].any()


def test_long7_edges_by_count():
    sg = LC.table("long7", 32)
    segs, ns = sg["segs"], sg["n_slots"]
    only_last = [(i, r) for i, s in enumerate(segs) for r in range(s["vis"].shape[0]) if s["vis"][r].sum() == 1 and s["vis"][r, ns[i] - 1]]
    assert only_last == [(1, 40), (2, 7), (3, 64), (5, 129)]
    blind = LC.blind_rows(sg)
    assert blind.sum() == 2 and list(np.flatnonzero(blind)) == [sg["row0"][2] + 5, sg["row0"][4] + 3]
    high = [(i, r) for i, s in enumerate(segs) for r in range(s["vis"].shape[0]) if s["vis"][r].any() and not s["vis"][r, :512].any()]
    assert high == [(1, 40), (2, 7), (2, 32), (3, 64), (5, 70), (5, 129)]
    assert segs[2]["vis"][32].sum() > 100 and segs[5]["vis"][70].sum() > 100        # (two of them see many slots there, not one)
    # a segment in which nobody sees tiles 8 .. 12 but somebody sees tiles 7 and 13
    lap = [i for i, s in enumerate(segs) if ns[i] > 13 * 64 and not s["vis"][:, 512: 832].any() and s["vis"][:, 448: 512].any() and s["vis"][:, 832: 896].any()]
    assert lap == [4]
    # a wave group (16 and 32 rows) that sees exactly tiles 3, 7, 11, ...: one per lap of the four-stage ring
    tiles_of = lambda v: set(np.flatnonzero(v.any(0)) // 64)
    for rows in (slice(0, 16), slice(16, 32), slice(0, 32)):
        assert tiles_of(segs[5]["vis"][rows]) == {3, 7, 11, 15, 19, 23}
    assert len(tiles_of(segs[5]["vis"][32:64])) == 24
    # a second wave group that sees nothing in tile 0, which the first one needs
    assert not segs[1]["vis"][32:, :64].any() and segs[1]["vis"][:16, :64].any(1).all() and segs[1]["vis"][32:].any(1).all()
    # stale set bits at slots >= n_slots: in the last word, and in later words
    last_word = sum(int(s["bits"][:, ns[i]: 64 * LC._tiles(ns[i])].sum()) for i, s in enumerate(segs))
    later = sum(int(s["bits"][:, 64 * LC._tiles(ns[i]):].sum()) for i, s in enumerate(segs))
    assert last_word == 64 * 1 + 33 * 63 + 65 * 63 + 65 * 63 and later == 65 * 22 * 64 + 1 * 8 * 64 + 65 * 8 * 64
    # the tree segment: the prefix, then every fourth ancestor up to the row itself, the last in the segment's last slot
    v = segs[0]["vis"]
    assert v[:, :LC.TREE_PREFIX].all() and not v[:, LC.TREE_PREFIX: 2008].any()
    assert [int(x) for x in np.flatnonzero(v[39, 2008:])] == list(range(3, 40, 4)) and v[39, 2047]


def test_one_row_sees_every_slot():
    """the scalar kernel keeps a slot list and the probabilities of 64 vis_words slots per wave, 4 waves: only a row of the fourth head that
    sees more than 1920 slots (head_dim 32) uses the part of that allocation beyond 64 KiB"""
    sg = LC.table("long7", 32)
    assert sg["segs"][6]["vis"].shape == (1, 2048) and sg["segs"][6]["vis"].all()
    assert max(int(s["vis"].sum(1).max()) for s in sg["segs"][:6]) < 1920


def test_form16_rule():
    """tests/test_segs_gpu.py::_form16: the ring's LDS limit beside its workgroup limit; the defaults are what they were"""
    from tests.test_segs_gpu import _form16
    assert [_form16(2, 2, 128, 128, w) for w in (4, 8, 23, 24, 32)] == ["ring", "ring", "ring", "staged", "staged"]
    assert _form16(2, 2, 64, 128, 32) == "ring" and _form16(2, 4, 128, 64, 32) == "ring" and _form16(2, 4, 64, 64, 32) == "ring"
    assert _form16(8, 4, 64) == "ring" and _form16(8, 33, 64) == "staged" and _form16(6, 43, 128) == "staged" and _form16(1, 1, 256) == "staged"
    assert _form16(8, 32, 64) == "ring" and _form16(10, 26, 64, 64, 32) == "staged"


def test_cross_tables():
    a, b = LC.table("cross", 23), LC.table("cross", 24)
    assert (a["n_tok"], a["n_slots"], a["max_slots"]) == ([128, 70], [1472, 1472], 1472)
    assert (b["n_tok"], b["n_slots"], b["max_slots"]) == ([128, 70], [1536, 1473], 1536)
    assert b["segs"][1]["bits"][:, 1473:].all() and not LC.blind_rows(a).any() and not LC.blind_rows(b).any()


def test_placed_kinds_cover_first_and_last_groups():
    sg = LC.table("long7", 32)
    for kind in LC.KINDS:
        where = [(i, r) for i, r, k, _ in LC.PLACED if k == kind]
        assert any(LC.first_group(r) for i, r in where), kind
        assert any(LC.last_group(r, sg["n_tok"][i]) and r >= 32 * ((sg["n_tok"][i] - 1) // 32) for i, r in where), kind
    rows = [(i, r) for i, r, _, _ in LC.PLACED]
    assert len(set(rows)) == len(rows)
    blind = LC.blind_rows(sg)
    assert not any(blind[sg["row0"][i] + r] for i, r in rows)
    for i, r, kind, ss in LC.PLACED:
        nt = LC._tiles(sg["n_slots"][i])
        if kind == "last":
            assert ss[0] // 64 == nt - 1
        if kind == "first":
            assert ss[0] // 64 == 0
        if kind == "twin":
            assert ss[0] // 64 != ss[1] // 64
    assert any(s >= 512 for _, _, k, ss in LC.PLACED for s in ss)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n_heads,head_dim", SHAPES)
def test_placed_rows_have_their_softmax(n_heads, head_dim, dtype):
    """q = 0: uniform, the reference is the mean of the visible v; q = 8 k[s]: max p > 1 - 1e-6 (a twin: two equal p that sum to it);
    q = -8 k[s]: p[s] vanishes.  Inputs are values of the format."""
    layer, H = 1, n_heads * head_dim
    sg, _, kc, vc = LC.inputs("long7", 32, "peaked", n_heads, head_dim, dtype)
    q = LC.placed_q("long7", 32, "peaked", n_heads, head_dim, dtype, layer)
    ref, mag = LC.ref64("long7", 32, "peaked", n_heads, head_dim, dtype, layer)
    assert np.array_equal(SC.to_dtype64(q, dtype), q)
    assert all(np.array_equal(SC.to_dtype64(k[layer], dtype), k[layer].astype(np.float64)) for k in kc)
    for i, r, kind, ss in LC.PLACED:
        p = LC.softmax_probs(sg, q, kc, i, n_heads, head_dim, layer)[:, r]              # [heads][n_slots]
        vis = sg["segs"][i]["vis"][r]
        row = int(sg["row0"][i]) + r
        assert all(vis[s] for s in ss)
        if kind == "zero":
            assert np.allclose(p[:, vis], 1.0 / vis.sum(), rtol=1e-14, atol=0) and vis.sum() > 50
            want = vc[i][layer, : sg["n_slots"][i]].astype(np.float64)[vis].mean(0)
            assert np.allclose(ref[row], want, rtol=0, atol=1e-14)
        elif kind in ("last", "first"):
            assert (p.max(-1) > 1 - 1e-6).all() and (p.argmax(-1) == ss[0]).all(), (i, r, kind, float(p.max(-1).min()))
        elif kind == "twin":
            assert (p[:, ss[0]] == p[:, ss[1]]).all() and (p[:, ss[0]] + p[:, ss[1]] > 1 - 1e-6).all(), (i, r)
        else:
            assert (p[:, ss[0]] < 1e-30).all() and (p.sum(-1) > 1 - 1e-12).all()
            assert vis.sum() > 1
    assert max(sg["segs"][i]["vis"][r].sum() for i, r, k, _ in LC.PLACED if k == "zero") > 1900      # the mean counts keys up to 2048
    # unit-normal rows are flat: no probability near one among many visible keys
    p = LC.softmax_probs(sg, q, kc, 0, n_heads, head_dim, layer)[:, 20]
    assert p.max() < 0.5


@pytest.mark.parametrize("family", ["normal", "peaked"])
@pytest.mark.parametrize("n_heads,head_dim", SHAPES)
def test_reference_is_torch_softmax_in_float64(n_heads, head_dim, family):
    layer, H = 0, n_heads * head_dim
    sg, _, kc, vc = LC.inputs("long7", 32, family, n_heads, head_dim, "bf16")
    q = LC.placed_q("long7", 32, family, n_heads, head_dim, "bf16", layer)
    ref, mag = LC.ref64("long7", 32, family, n_heads, head_dim, "bf16", layer)
    blind = LC.blind_rows(sg)
    assert not ref[blind].any() and not mag[blind].any() and (mag[~blind] > 0).all()
    for i in range(sg["n"]):
        T, S, r0 = sg["n_tok"][i], sg["n_slots"][i], int(sg["row0"][i])
        qt = torch.from_numpy(q[r0: r0 + T, :H]).view(T, n_heads, head_dim).transpose(0, 1)
        k = torch.from_numpy(kc[i][layer, :S]).double().view(S, n_heads, head_dim).transpose(0, 1)
        v = torch.from_numpy(vc[i][layer, :S]).double().view(S, n_heads, head_dim).transpose(0, 1)
        sc = (qt @ k.transpose(1, 2)) / head_dim ** 0.5
        sc = sc.masked_fill(~torch.from_numpy(sg["segs"][i]["vis"])[None], float("-inf"))
        p = torch.softmax(sc, -1)
        want = (p @ v).transpose(0, 1).reshape(T, H).numpy()
        wmag = (p @ v.abs()).transpose(0, 1).reshape(T, H).numpy()
        keep = ~blind[r0: r0 + T]
        assert np.abs(ref[r0: r0 + T][keep] - want[keep]).max() < 1e-13
        assert np.abs(mag[r0: r0 + T][keep] - wmag[keep]).max() < 1e-13
