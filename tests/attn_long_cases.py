"""Attention cases at long caches and peaked scores, built on the CPU from seeds alone (a plain module like tests/segs_cases.py): segment tables
of up to 2048 slots (32 visibility words, 32 K/V tiles of 64 keys) with placed visibility edges, two input families, and the per-segment
fp64 softmax attention of each.  tests/test_attn_long_cases_cpu.py checks, without a GPU, that every edge and every placed row is present;
tests/test_attn_long_gpu.py runs the kernels on them.

Wave groups: a wave owns 16 or 32 consecutive query rows of a segment.  `first group` below means rows < 16 (the first wave of both families),
`last group` rows >= 32 * ((n_tok - 1) // 32) that also lie in the last 16-row group, i.e. rows >= 16 * ((n_tok - 1) // 16).

Values are those of the tested format.  The caches are held in float32, which holds every bf16 / fp16 / fp32 value exactly, and are widened to
fp64 where the reference reads them (a 33-head cache set in fp64 would take a gigabyte); q is held in fp64."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import segs_cases as SC

LAYERS = SC.LAYERS
# (n_tok, n_slots) of long7: 32 full tiles | last tile short by one | 32nd tile holds one slot | ten tiles, the last holds one slot, the second
# 64-row tile one row | 24 tiles | three 64-row tiles, 24th tile holds one slot | one row.  353 rows: odd, the packed output has a pad row.
LONG_TOK = [40, 64, 33, 65, 20, 130, 1]
LONG_SLOTS = [2048, 2047, 1985, 577, 1536, 1473, 2048]
CROSS_TOK = [128, 70]
CROSS_SLOTS = [24 * 64, 24 * 64 - 63]
TREE_PREFIX = 1900                       # the tree segment: every row sees this prefix, then its ancestors
VICTIM = {"long7": 2, "cross": 1}        # the segment whose cache the isolation check fills with huge values


def _tiles(s):
    return (s + 63) // 64


def _long_vis(i, vis, stale):
    """the placed edges of long7, written relative to the segment's n_slots so that a table clipped to fewer words keeps them"""
    t, s = vis.shape
    if i == 0:                                            # the tree shape of test_attn_short_gpu._short_vis case 1: a prefix, then every 4th ancestor
        pre, base = min(TREE_PREFIX, s - t), s - t        # (the ancestors' slots are the segment's last t: they end in the last tile)
        vis[:] = False
        vis[:, :pre] = True
        for r in range(t):
            for a in range(r % 4, r + 1, 4):
                vis[r, base + a] = True
    if i == 1:
        vis[32:, :64] = False; vis[32:, 64] = True        # the second wave group sees nothing in tile 0, which the first one needs
        vis[40] = False; vis[40, s - 1] = True            # a row that sees only slot n_slots - 1, next to a stale bit
        stale[:, s:] = True                               # stale bits in the last word (slot 2047 of long7)
    if i == 2:
        vis[5] = False                                    # a row that sees nothing
        vis[7] = False; vis[7, s - 1] = True              # only the one slot of the last tile
        vis[32, :512] = False; vis[32, 600] = True        # the single row of the second wave group sees only words >= 8
        stale[:, s:] = True                               # bits 1 .. 63 of the last word
    if i == 3:
        vis[64] = False; vis[64, s - 1] = True            # the one row of the second 64-row tile sees only the one slot of the last key tile
        stale[:, s:] = True                               # the rest of the last word and every later word
    if i == 4:
        vis[:, 8 * 64: 13 * 64] = False                   # nobody sees tiles 8 .. 12: a whole ring lap plus one
        vis[3] = False                                    # ... and one row nothing
        stale[3, s:] = True                               # (its words past n_slots are set all the same)
    if i == 5:
        lap = (np.arange(s) // 64) % 4 == 3
        vis[:32, ~lap] = False                            # the first wave group sees exactly one tile per ring lap: tiles 3, 7, 11, ...
        vis[:32, s - 1] = True                            # (the last of them holds one slot)
        vis[70, :512] = False; vis[70, 8 * 64 + 5] = True # a row in the second 64-row tile that sees only words >= 8
        vis[129] = False; vis[129, s - 1] = True          # the last row sees only the last slot
        stale[::2, s:] = True
    if i == 6:
        vis[:] = True                                     # the one row sees every slot: the scalar kernel's slot list and probabilities are full,
                                                          # up to the last byte of the dynamic LDS its fourth wave is given


@functools.lru_cache(maxsize=None)
def table(name: str, vis_words: int = 32):
    """long7 / cross as a segment set in the format of segs_cases.segments, at max_slots = 64 vis_words (slot counts clipped to it).  Per segment:
    vis bool [n_tok][n_slots] (the truth) and bits bool [n_tok][max_slots] (what the kernel is handed: vis plus stale set bits at slots >= n_slots,
    which must never be seen)."""
    max_slots = 64 * vis_words
    tok, slots = (LONG_TOK, LONG_SLOTS) if name == "long7" else (CROSS_TOK, CROSS_SLOTS)
    slots = [min(s, max_slots) for s in slots]
    rng = np.random.default_rng({"long7": 3207, "cross": 2423}[name] + vis_words)
    segs = []
    for i, (t, s) in enumerate(zip(tok, slots)):
        vis = rng.random((t, s)) < 0.3
        vis[:, 0] = True
        stale = np.zeros((t, max_slots), dtype=bool)
        if name == "long7":
            _long_vis(i, vis, stale)
        else:
            stale[:, s:] = True
        stale[:, :s] = False
        bits = stale.copy()
        bits[:, :s] = vis
        z = np.zeros(t, dtype=np.int32)
        segs.append(dict(ids=z, pos=z, slots=z, vis=vis, bits=bits))
    row0 = np.concatenate([[0], np.cumsum(tok)])
    return dict(name=name, n=len(segs), segs=segs, n_tok=list(tok), n_slots=slots, n_logit=[0] * len(segs), row0=row0, total_tok=int(row0[-1]),
                max_slots=max_slots, vis_words=vis_words)


def bit_words(bits: np.ndarray) -> np.ndarray:
    """bool [T][64 W] -> uint64 [T][W], bit j of word w = slot 64 w + j"""
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little").view(np.uint64)


# ------------------------------------------------------------------ placed query rows of the `peaked` family
# (segment, row, kind, slots): zero: q = 0; last / first: q = 8 k[s], s in the last / first key tile; twin: q = 8 k[s0] with k[s1] = k[s0] in
# another tile; neg: q = -8 k[s].  Each kind once in a first wave group (row < 16) and once in a last one.  Slots of long7 at 32 words.
PLACED = [
    (0, 2, "zero", ()), (0, 6, "last", (2048 - 40 + 2,)), (0, 9, "first", (17,)), (0, 12, "twin", (100, 1850)), (0, 14, "neg", (5,)),
    (0, 33, "zero", ()), (0, 34, "last", (2048 - 40 + 34,)), (0, 36, "first", (40,)), (0, 37, "twin", (700, 2048 - 40 + 1)), (0, 38, "neg", (1000,)),
    (4, 17, "twin", (500, 840)), (4, 18, "zero", ()),               # the twins on either side of the tiles 8 .. 12 nobody sees
    (5, 1, "last", (1472,)), (5, 3, "zero", ()), (5, 128, "neg", (700,)),
    (1, 50, "last", (2046,)),                                       # next to the stale bit of slot 2047
    (6, 0, "first", (3,)),                                          # the only row of its wave: no maximum moves after tile 0 (the rescale is skipped)
]
KINDS = ("zero", "last", "first", "twin", "neg")


def first_group(row):
    return row < 16


def last_group(row, n_tok):
    return row >= 16 * ((n_tok - 1) // 16)


@functools.lru_cache(maxsize=None)
def _normal(name: str, vis_words: int, n_heads: int, head_dim: int, dtype: str):
    sg = table(name, vis_words)
    rng = np.random.default_rng(9100 + 17 * n_heads + head_dim + vis_words)
    H, ms = n_heads * head_dim, sg["max_slots"]

    cast32 = lambda x: torch.from_numpy(x).to(SC.TORCH[dtype]).float().numpy()
    q = cast32(rng.standard_normal((sg["total_tok"], 3 * H), dtype=np.float32)).astype(np.float64)
    kc = [cast32(rng.standard_normal((LAYERS, ms, H), dtype=np.float32)) for _ in range(sg["n"])]
    vc = [cast32(rng.standard_normal((LAYERS, ms, H), dtype=np.float32)) for _ in range(sg["n"])]
    return sg, q, kc, vc


@functools.lru_cache(maxsize=None)
def inputs(name: str, vis_words: int, family: str, n_heads: int, head_dim: int, dtype: str):
    """(sg, q, kc, vc): the table, q [total_tok][3 H] (fp64) and per-segment caches [LAYERS][max_slots][H] (float32), every element a value of
    `dtype`.  `normal`: unit-normal.  `peaked`: the same numbers; the slots the rows of PLACED name are made visible to them and a twin's second
    K row is a copy of its first (in both layers).  The placed q rows depend on the layer whose K row they follow: `placed_q`."""
    assert family in ("normal", "peaked")
    sg, q, kc, vc = _normal(name, vis_words, n_heads, head_dim, dtype)
    if family == "peaked":
        assert name == "long7" and vis_words == 32, "the placed rows name slots of long7 at 32 words"
        sg = dict(sg, segs=[dict(s, vis=s["vis"].copy(), bits=s["bits"].copy()) for s in sg["segs"]])
        kc = list(kc)
        for i, r, kind, ss in PLACED:
            for s in ss:
                assert s < sg["n_slots"][i]
                sg["segs"][i]["vis"][r, s] = sg["segs"][i]["bits"][r, s] = True
            if kind == "twin":
                kc[i] = kc[i].copy()                  # (the caches without a twin are shared with `normal`)
                kc[i][:, ss[1]] = kc[i][:, ss[0]]
    return sg, q, kc, vc


def placed_q(name, vis_words, family, n_heads, head_dim, dtype, layer):
    """q of `inputs` for a launch on `layer`: in `peaked` the placed rows are 0, 8 k or -8 k of that layer's K row (exact in the format: a power
    of two times a value of it, far from overflow)"""
    sg, q, kc, _ = inputs(name, vis_words, family, n_heads, head_dim, dtype)
    if family == "normal":
        return q
    q = q.copy()
    H = n_heads * head_dim
    for i, r, kind, ss in PLACED:
        row = int(sg["row0"][i]) + r
        if kind == "zero":
            q[row, :H] = 0.0
        else:
            q[row, :H] = (-8.0 if kind == "neg" else 8.0) * kc[i][layer, ss[0]].astype(np.float64)
    return q


def softmax_probs(sg, q, kc, i, n_heads, head_dim, layer):
    """fp64 probabilities [heads][n_tok][n_slots] of segment i: softmax of q k^T / sqrt(head_dim) over the visible slots; a row that sees nothing
    gets zeros"""
    T, S, r0, H = sg["n_tok"][i], sg["n_slots"][i], int(sg["row0"][i]), n_heads * head_dim
    qs = q[r0: r0 + T, :H].reshape(T, n_heads, head_dim).transpose(1, 0, 2)
    k = kc[i][layer, :S].astype(np.float64).reshape(S, n_heads, head_dim).transpose(1, 2, 0)
    sc = np.where(sg["segs"][i]["vis"][None], np.matmul(qs, k) / np.sqrt(head_dim), -np.inf)
    mx = sc.max(-1, keepdims=True)
    p = np.exp(sc - np.where(np.isfinite(mx), mx, 0.0))
    return p / np.maximum(p.sum(-1, keepdims=True), 1e-300)


@functools.lru_cache(maxsize=None)
def ref64(name: str, vis_words: int, family: str, n_heads: int, head_dim: int, dtype: str, layer: int):
    """the per-segment fp64 softmax attention over that segment's own cache, layer and visibility, as segs_cases.attn_ref64: the result
    [total_tok][H] and mag = sum_s p_s |v_s| per element.  Rows that see nothing are zero in both."""
    sg, _, kc, vc = inputs(name, vis_words, family, n_heads, head_dim, dtype)
    q = placed_q(name, vis_words, family, n_heads, head_dim, dtype, layer)
    H = n_heads * head_dim
    out = np.zeros((sg["total_tok"], H))
    mag = np.zeros_like(out)
    for i in range(sg["n"]):
        T, S, r0 = sg["n_tok"][i], sg["n_slots"][i], int(sg["row0"][i])
        p = softmax_probs(sg, q, kc, i, n_heads, head_dim, layer)
        v = vc[i][layer, :S].astype(np.float64).reshape(S, n_heads, head_dim).transpose(1, 0, 2)
        out[r0: r0 + T] = np.matmul(p, v).transpose(1, 0, 2).reshape(T, H)
        mag[r0: r0 + T] = np.matmul(p, np.abs(v)).transpose(1, 0, 2).reshape(T, H)
    out.setflags(write=False); mag.setflags(write=False)
    return out, mag


def blind_rows(sg):
    """bool [total_tok]: the rows that see nothing"""
    return ~np.concatenate([s["vis"].any(1) for s in sg["segs"]])


def n_visible(sg):
    """visible keys per row [total_tok]"""
    return np.concatenate([s["vis"].sum(1) for s in sg["segs"]])
