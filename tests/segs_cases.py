"""Inputs and fp64 references of tests/test_segs_gpu.py, built on the CPU from seeds alone (a plain module like tests/guard.py), so that
tests/test_rounding_cpu.py can check -- without a GPU -- that the cases keep their near ties under the cap of tests/rounding.py."""
from __future__ import annotations

import functools

import numpy as np
import torch

MAX_SLOTS, LAYERS, VIS_WORDS = 256, 2, 4
MAX_POS = 256                      # rows of the cos / sin tables the tests supply
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def to_dtype64(x, name):
    """fp values -> values of the format (torch's cast) as fp64"""
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(TORCH[name]).double().numpy()


@functools.lru_cache(maxsize=None)
def segments(name: str) -> dict:
    """ragged5 / many32: per-segment numpy arrays ids, pos, slots (a permutation: row != slot), vis (bool [n_tok][n_slots]) and the counts"""
    rng = np.random.default_rng({"ragged5": 501, "many32": 3201}[name])
    if name == "ragged5":
        n_tok, n_slots, n_logit = [1, 63, 64, 65, 130], [1, 70, 64, 129, 200], [1, 5, 0, 65, 7]
    else:
        n_tok = [int(v) for v in rng.integers(9, 31, 32)]
        n_slots = [t + int(v) for t, v in zip(n_tok, rng.integers(0, 21, 32))]
        n_logit = [int(rng.integers(1, t + 1)) for t in n_tok]
        n_logit[5] = 0                 # a segment without logit rows between two that have some: it shares its logit_row0 with the next one
        n_logit[17] = n_logit[18] = 0  # ... and two in a row
    segs = []
    for i, (t, s) in enumerate(zip(n_tok, n_slots)):
        slots = rng.permutation(s)[:t] if s >= t else rng.permutation(MAX_SLOTS)[:t]
        if t > 1 and np.array_equal(slots, np.arange(t)):
            slots = slots[::-1].copy()
        vis = rng.random((t, s)) < 0.3
        vis[:, 0] = True
        pos = np.arange(t)
        ids = rng.integers(0, 1000, t)
        segs.append(dict(ids=ids.astype(np.int32), pos=pos.astype(np.int32), slots=slots.astype(np.int32), vis=vis))
    if name == "ragged5":
        segs[0]["vis"][:] = True                                          # a single row that sees its one slot
        segs[4]["vis"][3] = False; segs[4]["vis"][3, 199] = True          # one row sees only the last slot of its segment
        segs[3]["vis"][7, 64:] = False                                    # one row sees nothing beyond the first 64 slots
        segs[4]["pos"][[10, 11, 12]] = 9                                  # tree tokens: repeated positions
        segs[3]["pos"][[20, 21]] = 19
        segs[1]["pos"][5] = -1
        segs[2]["pos"][6] = MAX_POS - 1
        segs[3]["pos"][8] = MAX_POS
        segs[4]["pos"][100] = MAX_POS + 7
        segs[1]["ids"][3] = -3                                            # the id clamp: -> 0 and vocab - 1
        segs[4]["ids"][64] = 1000 + 5
    else:
        segs[2]["ids"][0] = -3
        segs[30]["ids"][1] = 1000 + 5
        segs[7]["pos"][2] = -1
        segs[9]["pos"][3] = MAX_POS + 7
    row0 = np.concatenate([[0], np.cumsum(n_tok)])
    return dict(name=name, n=len(segs), segs=segs, n_tok=n_tok, n_slots=n_slots, n_logit=n_logit, row0=row0, total_tok=int(row0[-1]),
                total_logit=int(sum(n_logit)), vocab=1000)


def vis_words(vis: np.ndarray) -> np.ndarray:
    """bool [T][S] -> uint64 [T][VIS_WORDS], bit j of word w = slot 64 w + j"""
    full = np.zeros((vis.shape[0], VIS_WORDS * 64), dtype=np.uint8)
    full[:, : vis.shape[1]] = vis
    return np.packbits(full, axis=1, bitorder="little").view(np.uint64)


def clamp_pos(pos):
    return np.clip(pos, 0, MAX_POS - 1)


# ------------------------------------------------------------------ RoPE
@functools.lru_cache(maxsize=None)
def rope_tables(head_dim: int):
    """fp32 cos / sin [MAX_POS][head_dim / 2], theta 10000 (the values themselves are arbitrary inputs of the kernel under test)"""
    inv = 10000.0 ** (-np.arange(head_dim // 2, dtype=np.float64) * 2 / head_dim)
    ang = np.arange(MAX_POS, dtype=np.float64)[:, None] * inv[None]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rope_qkv(seg_name: str, n_heads: int, head_dim: int, dtype: str):
    """unit-normal qkv [total_tok][3 H] as values of the format (fp64)"""
    sg = segments(seg_name)
    rng = np.random.default_rng(7000 + 13 * n_heads + head_dim)
    return to_dtype64(rng.standard_normal((sg["total_tok"], 3 * n_heads * head_dim)), dtype)


# The rotary pair in fp32 is one product rounded (at most 2^-24 |x1 s|) and one fused multiply-add rounded (at most 2^-24 of the result): at most
# 2^-23 of the operands' magnitude |x0 c| + |x1 s| in all.  Its near-tie band is that, not rounding.REL of the VALUE: under cancellation the value
# is small against its operands and the error is not.  (Where the magnitude is below 8 |value| -- nearly everywhere -- this band is the narrower.)
ROPE_REL = 2.0 ** -23


def rope_rotate64(x64, pos_all, n_heads, head_dim):
    """HF rotate-half on [T][H] fp64 values (pairs (i, i + head_dim / 2) of every head) with the fp32 tables' values; returns the rotated values
    and the operands' magnitude |x0 c| + |x1 s| per element (the scale of the fp32 evaluation error)"""
    cos, sin = rope_tables(head_dim)
    ps = clamp_pos(pos_all)
    c = cos[ps].astype(np.float64)[:, None, :]
    s = sin[ps].astype(np.float64)[:, None, :]
    half = head_dim // 2
    x = x64.reshape(x64.shape[0], n_heads, head_dim)
    x0, x1 = x[..., :half], x[..., half:]
    out = np.concatenate([x0 * c - x1 * s, x1 * c + x0 * s], axis=-1)
    mag = np.concatenate([np.abs(x0 * c) + np.abs(x1 * s), np.abs(x1 * c) + np.abs(x0 * s)], axis=-1)
    return out.reshape(x64.shape), mag.reshape(x64.shape)


def all_pos(sg):
    return np.concatenate([s["pos"] for s in sg["segs"]])


@functools.lru_cache(maxsize=None)
def rope_slabs(seg_name: str, n_heads: int, head_dim: int, dtype: str, splits: int):
    """fp32 slabs [splits][T][3 H] and what the kernel makes of them first: the sequential float32 sum in ascending slab order (starting from
    0, as the kernel's accumulator does), rounded to the 16-bit format (fp64 values)"""
    sg = segments(seg_name)
    rng = np.random.default_rng(7100 + splits)
    slabs = (rng.standard_normal((splits, sg["total_tok"], 3 * n_heads * head_dim)) / np.sqrt(splits)).astype(np.float32)
    acc = np.zeros(slabs.shape[1:], dtype=np.float32)
    for z in range(splits):
        acc = acc + slabs[z]
    return slabs, to_dtype64(acc, dtype)


# ------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def attn_inputs(seg_name: str, n_heads: int, head_dim: int, dtype: str):
    """unit-normal q (the first H of 3 H columns) and per-segment K / V caches [LAYERS][MAX_SLOTS][H], as values of the format (fp64)"""
    sg = segments(seg_name)
    rng = np.random.default_rng(9000 + 17 * n_heads + head_dim)
    H = n_heads * head_dim
    q = to_dtype64(rng.standard_normal((sg["total_tok"], 3 * H)), dtype)
    kc = [to_dtype64(rng.standard_normal((LAYERS, MAX_SLOTS, H)), dtype) for _ in range(sg["n"])]
    vc = [to_dtype64(rng.standard_normal((LAYERS, MAX_SLOTS, H)), dtype) for _ in range(sg["n"])]
    return q, kc, vc


@functools.lru_cache(maxsize=None)
def attn_ref64(seg_name: str, n_heads: int, head_dim: int, dtype: str, layer: int):
    """per segment: softmax(q k^T / sqrt(dh) over the visible slots) v in fp64 over that segment's own cache, layer and visibility (the formula of
    test_kernels_gpu.py::test_tree_attention); returns the result [T][H] and sum_s p_s |v_s| per element"""
    sg = segments(seg_name)
    q, kc, vc = attn_inputs(seg_name, n_heads, head_dim, dtype)
    H = n_heads * head_dim
    out = np.zeros((sg["total_tok"], H))
    mag = np.zeros_like(out)
    for i, s in enumerate(sg["segs"]):
        T, S = sg["n_tok"][i], sg["n_slots"][i]
        qs = q[sg["row0"][i]: sg["row0"][i] + T, :H].reshape(T, n_heads, head_dim)
        k = kc[i][layer, :S].reshape(S, n_heads, head_dim)
        v = vc[i][layer, :S].reshape(S, n_heads, head_dim)
        sc = np.einsum("thd,shd->hts", qs, k) / np.sqrt(head_dim)
        sc = np.where(s["vis"][None], sc, -np.inf)
        p = np.exp(sc - sc.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out[sg["row0"][i]: sg["row0"][i] + T] = np.einsum("hts,shd->thd", p, v).reshape(T, H)
        mag[sg["row0"][i]: sg["row0"][i] + T] = np.einsum("hts,shd->thd", p, np.abs(v)).reshape(T, H)
    return out, mag


# ------------------------------------------------------------------ residual + norm tail
def norm_ref64(h64, w64, eps, dtype):
    """HF LlamaRMSNorm on the stored h (values of the format, fp64): round(w * round(h * rsqrt(mean(h^2) + eps))).  Returns the fp64 value in
    front of each rounding step: inner = h * rs, outer = w * round(inner), and outer_alt = w * (the other neighbour of inner) where inner is a
    near tie (else = outer)."""
    from tests import rounding
    h64 = np.asarray(h64, dtype=np.float64)
    rs = 1.0 / np.sqrt((h64 * h64).mean(-1, keepdims=True) + float(np.float32(eps)))
    inner = h64 * rs
    if rounding.fmt(dtype) == "fp32":
        return inner, w64 * inner, w64 * inner
    r = rounding.round_to(inner, dtype)
    tie = rounding.near_tie(inner, dtype)
    lo, hi, _ = rounding._floor_ceil(inner, dtype)
    other = np.where(r == lo, hi, lo)
    return inner, w64 * r, np.where(tie, w64 * other, w64 * r)


# the residual + norm cases: (form, m, n, k); the form is what plan_gemm takes with the default switches and a 64 MB workspace, asserted through
# atspeed_gemm_path_counters: tiled = LDS-tiled split (5), wdma_split (3), ring_split (4), kcut (4), panel_split (10), ring (0)
NORM_N = [768, 1002, 4096, 4104, 8192, 8200]
RESID_NORM_16 = ([("tiled", 8, n, 512) for n in NORM_N] +
                 [("wdma_split", 33, 4096, 2560), ("wdma_split", 33, 4104, 2560), ("wdma_split", 33, 8192, 1536), ("wdma_split", 33, 8200, 1536),
                  ("ring_split", 33, 8192, 256), ("ring_split", 33, 8200, 256),
                  ("kcut", 257, 4096, 2048),
                  ("panel_split", 257, 4104, 8192), ("panel_split", 257, 8192, 2048), ("panel_split", 257, 8200, 2048),
                  ("ring", 513, 8192, 128), ("ring", 513, 8200, 128), ("ring", 1153, 4096, 128), ("ring", 1153, 4104, 128)])
PATH_OF_FORM = {"tiled": 5, "wdma_split": 3, "ring_split": 4, "kcut": 4, "panel_split": 10, "ring": 0}


def resid_inputs(m, n, k, dtype, seed=0):
    """a [m][k] ~ N(0, 1), w [n][k] ~ N(0, 1 / k), residual [m][n] ~ N(0, 1), norm weight [n] = 1 + N(0, 0.1): values of the format (fp32 arrays)"""
    rng = np.random.default_rng(1234 + seed)
    t = TORCH[dtype]
    cast = lambda x: torch.from_numpy(x.astype(np.float32)).to(t)
    return (cast(rng.standard_normal((m, k), dtype=np.float32)), cast(rng.standard_normal((n, k), dtype=np.float32) / np.float32(np.sqrt(k))),
            cast(rng.standard_normal((m, n), dtype=np.float32)), cast(1 + 0.1 * rng.standard_normal(n, dtype=np.float32)))
