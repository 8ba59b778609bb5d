"""Placed operands for the projection GEMMs, the edge table of their dispatch, and the judge (a plain module like tests/attn_long_cases.py; torch
and numpy on the CPU, no GPU and no library).  tests/test_gemm_cases_cpu.py proves the cases and the judge; tests/test_gemm_placed_gpu.py runs
the kernels on them.

Placed operands.  One operand of a launch holds a single non-zero per row, the other is dense.  Every output element is then ONE product of two
values of the format -- exact in fp32 -- plus exact zeros from every other k-step, ring stage, split part and slab, so the fp32 result is known
bit for bit whatever the summation order, and every 16-bit epilogue is a stated function of it (common.h: round_elt, resid_add, swiglu).
  weight selector (`W`):      W[n] = beta_n at k = kappa(n), A dense.  kappa runs over every k of [0, K); N < K takes ceil(K / N) launches.
  activation selector (`A`):  A[i] = alpha_i at k = kappa'(i), W dense.  kappa' takes every k of the first and the last 128 of K (hence every
                              residue mod 128) and one k of every aligned 64-k chunk: every part of every K split of gemm.hip is a whole
                              number of 64-k tiles (the LDS-tiled kernel: BK = 64 / 32, at least four per part) or of 128- / 256-k units, so
                              every part of every plan holds a selected k.  ceil(len(targets) / M) launches.
Dense rows are scaled by 2^((row mod 13) - 6), so a leak between rows, or a scale of the neighbouring row, is a gross error in the smaller row.
SwiGLU launches keep |gate| <= 8 (beta < 4, dense values < 2, row scales 2^((row mod 13) // 2 - 6) <= 1): above that the judge's band would
have to cover __expf's error growth.  One dense row is all zero (exact zeros out, or exactly h under the residual epilogue).  Dense values and
row scales are integer hashes of (row, column, seed), evaluated alike on any torch device and, for the expected values, only at the selected k:
the reference is a gather of M x N elements, not a matmul.
W8A8: e4m3 codes, one scale vector powers of two, the other general fp32 values (variant `a`: sx = 2^.., sw general; `b`: the other way round):
the result is fl32(acc * general) * 2^.. in whichever order a kernel multiplies.  W4A8: e2m1 codes under varied E8M0 block scales (one block
of scale byte 0 and zero codes), e4m3 activations, sx powers of two.  (An e4m3 x e2m1 product times 2^e has 6 mantissa bits: it IS a 16-bit value,
so W4A8 pins reads, scales and locations, and the roundings only under RESID's sum and SwiGLU.)  W8A8 SwiGLU launches keep the dense codes normal
and the scales within 2^-9 .. 1: a tiny gate would make silu(g) u the product g u / 2, whose exact ties would all count as near ties.
No ring form takes a K of fewer k-steps than its four stages (K % 128 == 0: four steps of 32 at the least), so the table holds none.

Expected values from the exact p (tests/rounding.py), per epilogue: F32: p (bit for bit).  STORE: round_to(p), bit for bit (exact ties go to
even).  RESID: round_to(h + round_to(p)) (16 bit; |exponent(h) - exponent(p)| <= 12 keeps the fp32 sum exact), fl32(h + p) (fp32), bit for
bit.  SWIGLU: silu(round_to(g)) * round_to(u) under rounding.assert_rounded at rounding.REL / rounding.CAP (16 bit), relative error <= REL
(fp32); outputs in the interleaved 16-row gate / up groups of atspeed_amd.model._interleave_gate_up.

The edge table (TABLE): one row per (form, shape, epilogues, types, the launch counter that must be 1), derived by hand from the planner
predicates of atspeed_amd/csrc/gemm.hip; `why` starts with the predicates the row sits on (before the colon) and names the constant."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from tests import rounding as RD

STORE, F32, RESID, SWIGLU = 0, 1, 2, 3
EPI = {"S": STORE, "F": F32, "R": RESID, "G": SWIGLU}
EPI_NAME = {STORE: "store", F32: "f32", RESID: "resid", SWIGLU: "swiglu"}
DT = {"b": "bf16", "h": "fp16", "f": "fp32"}
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
# atspeed_gemm_path_counters (internal.h: ATS_PATH_*)
RING, RING_SK, WDMA, WDMA_SPLIT, RING_SPLIT, TILED, FP8_RING, FP8_WDMA, FP8_WDMA_SPLIT, PANEL, PANEL_SPLIT, FP8_RING_SPLIT, FP4 = range(13)
N_COUNTERS = 13
DEFAULT_SWITCHES = dict(gemm_sk=1, gemm_panel=1, gemm_kcut=2, gemm_sk_g=0, gemm_force_mt=0)      # the library's defaults, pinned by every case


class Row(NamedTuple):
    form: str        # the form the row pins (the K-cut sub-form and the split-K tail have their own names)
    m: int
    n: int
    k: int
    epis: str        # of S F R G
    dtypes: str      # of b h f
    counter: int     # the one launch counter that must read 1
    why: str         # "predicate[, predicate]: the constant and the side of it"
    ws: bool         # with the 64 MB workspace
    sw: tuple        # switches other than the defaults

    @property
    def fam(self):
        return "f32" if self.dtypes == "f" else "w8a8" if self.form.startswith("fp8") else "w4a8" if self.form == "fp4" else "g16"


def R(form, m, n, k, epis, dtypes, counter, why, ws=True, **sw):
    return Row(form, m, n, k, epis, dtypes, counter, why, ws, tuple(sorted(sw.items())))


# ------------------------------------------------------------------ the edge table
# Defaults: gemm_sk = 1 (cost model), gemm_panel = 1, gemm_kcut = 2.  t128 / t192 = tiles of 128 / 192 weight rows; tn = 256-wide weight tiles
# of the ring kernels, tm128 / tm256 = token tiles; fill = tiles * 100 / 256 of the last round.
TABLE = [
    # ---- the LDS-tiled kernel, 16 bit: what no other form takes (m < 33, n < 2048, K off the 64 / 128 grid)
    R("tiled", 1, 128, 128, "SR", "b", TILED, "make_plan: one tile of bm = 16, one row, two k-tiles (ktiles / 4 = 0: no split)"),
    R("tiled", 16, 384, 352, "SG", "b", TILED, "make_plan: m <= 16 is bm = 16; K % 64 != 0, the last k-tile is half empty"),
    R("tiled", 17, 384, 352, "S", "h", TILED, "make_plan: m = 17 is bm = 32, its last 15 rows padding"),
    R("tiled", 32, 200, 96, "R", "b", TILED, "make_plan: m <= 32 is bm = 32, a full tile; K = 96, a k-tile and a half; last weight tile 72 wide"),
    R("tiled", 33, 200, 96, "F", "b", TILED, "make_plan: m = 33 is bm = 64"),
    R("tiled", 64, 136, 512, "SR", "bh", TILED, "make_plan: m <= 64 is bm = 64 and target_wgs = 768; last weight tile 8 wide; 8 k-tiles, 2 parts"),
    R("tiled", 65, 136, 512, "S", "b", TILED, "make_plan: m = 65 is bm = 128 and target_wgs = 512"),
    R("tiled", 7, 250, 768, "SFR", "b", TILED, "make_plan, reduce_splits: 3 parts and n % 4 != 0, the element-wise reduce pass (V = 1)"),
    R("tiled", 5, 128, 448, "F", "b", TILED, "make_plan: 7 k-tiles, max_splits = ktiles / 4 = 1: the last K without a split"),
    R("tiled", 1, 128, 4096, "F", "b", TILED, "make_plan: 64 k-tiles, the cap of 16 parts"),
    R("tiled", 20, 4096, 768, "S", "b", TILED, "plan_gemm: 3 slabs fit the workspace"),
    R("tiled", 20, 4096, 768, "SR", "b", TILED, "plan_gemm: no workspace, p.tiled.splits = 1 and k_per_split = K", ws=False),
    R("tiled", 129, 1024, 512, "SG", "b", TILED, "make_plan, wdma_split_count: n < 2048 stays here; a second token tile of one row"),
    R("tiled", 256, 1024, 256, "R", "h", TILED, "make_plan: two full 128-row token tiles"),
    R("tiled", 257, 640, 1376, "SG", "b", TILED, "big_kernel_applies: K % 128 != 0 at 257 rows; third token tile of one row"),
    R("tiled", 129, 16384, 192, "S", "b", TILED, "make_plan: bn = 64 from n = 16384 at m > 128 (K < 256 keeps ring_split_count away)"),
    R("tiled", 129, 16256, 192, "S", "b", TILED, "make_plan: n < 16384 keeps bn = 128"),
    R("tiled", 513, 9728, 576, "F", "b", TILED, "make_plan: 380 tiles, below 75 % of target_wgs = 512: 2 parts of 9 k-tiles"),
    R("tiled", 513, 9856, 576, "F", "b", TILED, "make_plan: 385 tiles, tiles * 4 >= target_wgs * 3: no split"),
    # ---- the LDS-tiled kernel, fp32 engine (BK = 32)
    R("tiled32", 1, 128, 128, "S", "f", TILED, "make_plan: one tile, one row, 4 k-tiles"),
    R("tiled32", 16, 136, 100, "SG", "f", TILED, "make_plan: bm = 16 full; K % 32 != 0; last weight tile 8 wide (SwiGLU: n = 160)"),
    R("tiled32", 17, 136, 100, "F", "f", TILED, "make_plan: m = 17 is bm = 32"),
    R("tiled32", 64, 250, 512, "SR", "f", TILED, "make_plan, reduce_splits: bm = 64 full, 4 parts, n % 4 != 0"),
    R("tiled32", 65, 256, 512, "G", "f", TILED, "make_plan: m = 65 is bm = 128"),
    R("tiled32", 129, 256, 96, "SR", "f", TILED, "make_plan: second token tile of one row, 3 k-tiles"),
    R("tiled32", 300, 8192, 256, "F", "f", TILED, "plan_gemm: dtype == ATSPEED_F32 takes no ring form whatever the shape"),
    # ---- ring kernel, split into slabs (one user's wide projections: 33-512 rows, n >= 8192)
    R("ring_split", 32, 8192, 256, "S", "b", TILED, "ring_split_count: m < min_m = 33 stays with the LDS-tiled kernel"),
    R("ring_split", 33, 8192, 256, "SFRG", "bh", RING_SPLIT, "ring_split_count: min_m = 33, min_n = 8192, the smallest K = 256: 2 parts of one 128-k unit (four ring stages)"),
    R("ring_split", 128, 8192, 384, "S", "b", RING_SPLIT, "ring_split_count, launch_slabs: 128 rows, the 128-row tile full; K = 256 + 128, 3 parts"),
    R("ring_split", 129, 8192, 256, "R", "b", RING_SPLIT, "launch_slabs: m > 128 takes the 256-row tile, 127 rows of it padding"),
    R("ring_split", 256, 8192, 256, "S", "h", RING_SPLIT, "launch_slabs: the 256-row tile full"),
    R("ring_split", 257, 8192, 256, "F", "b", RING_SPLIT, "ring_split_count: second 256-row token tile of one row (t256 = 64: 4 parts wanted, 2 units there)"),
    R("ring_split", 512, 8192, 256, "S", "b", RING_SPLIT, "ring_split_count: max_m = 512, two full token tiles"),
    R("ring_split", 513, 8192, 256, "S", "b", RING, "ring_split_count, ring_fills: m > max_m = 512; t128 = 160 fills 62 %: the ring kernel"),
    R("ring_split", 40, 8184, 256, "S", "b", TILED, "ring_split_count: n < min_n = 8192"),
    R("ring_split", 40, 8200, 256, "SR", "b", RING_SPLIT, "ring_split_count: tn = 33, the last weight tile 8 wide"),
    R("ring_split", 40, 8198, 256, "SF", "b", RING_SPLIT, "ring_split_count, reduce_splits: n % 4 != 0, the element-wise reduce pass"),
    R("ring_split", 100, 8192, 1024, "SG", "b", RING_SPLIT, "ring_split_count, wdma_split_count: s = min(256 / 32, units = 8) = 8 parts, the most at a small shape (K < 1536 keeps the weight-streaming split away)"),
    R("ring_split", 40, 8192, 256, "S", "b", TILED, "plan_gemm: no workspace for the slabs", ws=False),
    # ---- weight-streaming kernel, no split (33-256 rows, 150-256 tiles)
    R("wdma", 32, 19200, 512, "S", "b", TILED, "wdma_applies: m < min_m = 33"),
    R("wdma", 33, 19200, 512, "SFG", "bh", WDMA, "wdma_applies, launch_wdma: min_m = 33, t128 = 150, the smallest K = 512; <64, 128, 6>"),
    R("wdma", 64, 19200, 640, "S", "b", WDMA, "launch_wdma: m <= 64, the 64-row tile full; K = 512 + 128"),
    R("wdma", 65, 19200, 512, "F", "b", WDMA, "launch_wdma: m = 65 takes <128, 128, 4>"),
    R("wdma", 128, 19200, 512, "G", "b", WDMA, "launch_wdma: m <= 128, the tile full"),
    R("wdma", 129, 19200, 512, "S", "h", WDMA, "launch_wdma: m = 129 takes <256, 128, 3> with 8 waves"),
    R("wdma", 256, 19200, 576, "SF", "b", WDMA, "wdma_applies: max_m = 256, the tile full; K % 64 == 0 but not % 128"),
    R("wdma", 257, 19200, 512, "S", "b", RING, "wdma_applies, ring_fills: m > max_m; t128 = 225 fills 87 %"),
    R("wdma", 40, 19080, 512, "SF", "b", WDMA, "wdma_applies: t128 = 150 with a last tile 8 wide"),
    R("wdma", 40, 19074, 512, "S", "b", WDMA, "wdma_applies: t128 = 150, a last tile 2 wide, n % 4 != 0"),
    R("wdma", 40, 19072, 512, "S", "b", RING_SPLIT, "wdma_applies, ring_split_count: t128 = 149 < 150"),
    R("wdma", 40, 19072, 576, "S", "b", TILED, "wdma_applies, ring_split_count: t128 = 149 and K % 128 != 0"),
    R("wdma", 40, 32768, 512, "S", "b", WDMA, "wdma_applies: t128 = 256, the last one-round grid of 128-row tiles"),
    R("wdma", 40, 32769, 512, "F", "b", WDMA, "wdma_applies, launch_wdma: t128 = 257, ok192 (171 tiles of 192): <64, 192, 4>, last tile 1 wide"),
    R("wdma", 100, 32859, 576, "SF", "b", WDMA, "launch_wdma: <128, 192, 3> (the lm_head's shape)"),
    R("wdma", 129, 32769, 512, "S", "b", RING_SPLIT, "wdma_applies: 129-256 rows take 128-row tiles only (t128 = 257)"),
    R("wdma", 40, 19200, 448, "S", "b", TILED, "wdma_applies: K < 512"),
    R("wdma", 40, 19200, 512, "R", "b", RING_SPLIT, "wdma_applies: no residual epilogue; ring_split_count takes it"),
    # ---- weight-streaming kernel, split in K
    R("wdma_split", 32, 12288, 1024, "S", "b", TILED, "wdma_split_count: m < min_m = 33"),
    R("wdma_split", 33, 12288, 1024, "SFRG", "bh", WDMA_SPLIT, "wdma_split_count: min_m = 33; t128 = 96, s = min(2, 16 / 8) = 2"),
    R("wdma_split", 64, 12288, 1088, "S", "b", WDMA_SPLIT, "launch_wdma_split: <64, 6> full; K % 64 == 0 but not % 128, 17 k-tiles over 2 parts"),
    R("wdma_split", 65, 12288, 1024, "R", "b", WDMA_SPLIT, "launch_wdma_split: m = 65 takes <128, 4>"),
    R("wdma_split", 128, 12288, 1024, "S", "h", WDMA_SPLIT, "wdma_split_count: min_tiles = 8 up to 128 rows"),
    R("wdma_split", 129, 12288, 1024, "S", "b", RING_SPLIT, "wdma_split_count: min_tiles = 16 above 128 rows, 16 / 16 = 1 part: the ring split"),
    R("wdma_split", 129, 12288, 2048, "SR", "b", WDMA_SPLIT, "wdma_split_count, launch_wdma_split: 32 / 16 = 2 parts; <256, 3, 4>"),
    R("wdma_split", 256, 12288, 2048, "F", "b", WDMA_SPLIT, "wdma_split_count: m <= 256, the tile full"),
    R("wdma_split", 257, 12288, 2048, "S", "b", PANEL_SPLIT, "wdma_split_count, panel_applies: m > 256; t128 = 96 >= 64: the panel split"),
    R("wdma_split", 40, 2048, 5120, "SR", "b", WDMA_SPLIT, "wdma_split_count: n = 2048, t128 = 16; 80 / 8 = 10 parts give 160 >= 150 workgroups"),
    R("wdma_split", 40, 2040, 5120, "S", "b", TILED, "wdma_split_count: n < 2048"),
    R("wdma_split", 40, 4096, 2560, "S", "b", WDMA_SPLIT, "wdma_split_count: t128 = 32, 40 / 8 = 5 parts, 160 workgroups"),
    R("wdma_split", 40, 4096, 2496, "S", "b", TILED, "wdma_split_count: 39 / 8 = 4 parts, t128 * s = 128 < 150"),
    R("wdma_split", 40, 12168, 1024, "SF", "b", WDMA_SPLIT, "wdma_split_count: last weight tile 8 wide"),
    R("wdma_split", 40, 12290, 1024, "S", "b", WDMA_SPLIT, "wdma_split_count, reduce_splits: n % 4 != 0 (t128 = 97)"),
    R("wdma_split", 40, 12288, 1024, "S", "b", TILED, "plan_gemm: no workspace for the slabs", ws=False),
    # ---- panel form, unsplit (257-352 rows, 129-256 panels)
    R("panel", 256, 19200, 2048, "S", "b", WDMA, "panel_applies: m < 257"),
    R("panel", 257, 19200, 2048, "SFRG", "bh", PANEL, "panel_applies, panel_split_count: m = 257, t128 = 150: one round; the smallest K = 2048"),
    R("panel", 352, 19200, 2176, "S", "b", PANEL, "panel_applies: one round of panels up to m = 352; K = 2048 + 128"),
    R("panel", 353, 19200, 2048, "S", "b", RING, "panel_applies, ring_fills: m > 352 without split; t128 = 225"),
    R("panel", 384, 19200, 2048, "SR", "b", PANEL, "panel_applies: gemm_panel = 2, the 384-row tile full", gemm_panel=2),
    R("panel", 385, 19200, 2048, "S", "b", RING_SPLIT, "panel_applies, ring_fills, ring_split_count: m > 384 even when forced; t128 = 300 fills 58 % of two rounds: one slab", gemm_panel=2),
    R("panel", 300, 19080, 2048, "SF", "b", PANEL, "panel_applies: last panel 8 wide"),
    R("panel", 300, 16512, 2048, "S", "b", PANEL, "panel_split_count: t128 = 129, 256 / 129 = 1 part"),
    R("panel", 300, 32768, 2048, "S", "b", PANEL, "panel_applies: t128 = 256"),
    R("panel", 300, 32769, 2048, "S", "b", RING, "panel_applies: t128 = 257 > 256"),
    R("panel", 300, 19200, 1920, "S", "b", RING, "panel_applies: K < 2048"),
    # ---- panel form, split in K
    R("panel_split", 257, 8192, 2048, "SFRG", "bh", PANEL_SPLIT, "panel_applies, panel_split_count: t128 = 64, the least that splits by default; min(256 / 64, 16 / 4) = 4 parts"),
    R("panel_split", 384, 8192, 2048, "S", "b", PANEL_SPLIT, "panel_applies: the split form runs up to 384 rows, the tile full"),
    R("panel_split", 385, 8192, 2048, "S", "b", RING_SPLIT, "panel_applies, ring_split_count: m > 384"),
    R("panel_split", 300, 8064, 2048, "S", "b", TILED, "panel_applies: t128 = 63 < 64 at K < 8192"),
    R("panel_split", 300, 16384, 2048, "SR", "b", PANEL_SPLIT, "panel_split_count: t128 = 128, 2 parts (129 panels run unsplit)"),
    R("panel_split", 320, 2048, 2048, "SR", "b", PANEL_SPLIT, "panel_applies: gemm_panel = 2, t128 = 16, the fewest panels; 4 parts", gemm_panel=2, gemm_kcut=0),
    R("panel_split", 320, 2040, 2048, "S", "b", PANEL_SPLIT, "panel_applies: forced, last panel 120 wide", gemm_panel=2, gemm_kcut=0),
    R("panel_split", 320, 1920, 2048, "S", "b", TILED, "panel_applies: t128 = 15 < 16 even when forced", gemm_panel=2, gemm_kcut=0),
    R("panel_split", 320, 4096, 2560, "SF", "b", PANEL_SPLIT, "panel_split_count: units / 4 = 5 parts at K = 2560 (4 at 2048)", gemm_panel=2, gemm_kcut=0),
    R("panel_split", 300, 8192, 2048, "S", "b", TILED, "plan_gemm, big_kernel_applies: no workspace; a panel shape never takes the ring kernel", ws=False),
    # ---- K-cut sub-form of the ring split (257-1100 rows, 1024 <= n <= 4096, K >= 2048)
    R("kcut", 256, 1024, 2048, "S", "b", TILED, "kcut_split_count: m < 257"),
    R("kcut", 257, 1024, 2048, "SFR", "bh", RING_SPLIT, "kcut_split_count, cut_split_count: m = 257, n = 1024, K = 2048: t128 = 12, min(21, 16 / 4) = 4 parts; third token tile of one row"),
    R("kcut", 384, 1024, 2048, "S", "b", RING_SPLIT, "cut_split_count: three full 128-row token tiles"),
    R("kcut", 385, 1024, 2048, "R", "b", RING_SPLIT, "cut_split_count: fourth token tile of one row"),
    R("kcut", 512, 1024, 2560, "S", "h", RING_SPLIT, "kcut_split_count: 20 units / 4 = 5 parts at K = 2560"),
    R("kcut", 513, 1024, 2048, "F", "b", RING_SPLIT, "cut_split_count: fifth token tile of one row"),
    R("kcut", 1100, 1024, 2048, "S", "b", RING_SPLIT, "kcut_split_count: the last m = 1100"),
    R("kcut", 1101, 1024, 2048, "S", "b", TILED, "kcut_split_count, ring_fills: m > 1100, t128 = 36 fills nothing"),
    R("kcut", 300, 1020, 2048, "S", "b", TILED, "kcut_split_count: n < 1024"),
    R("kcut", 300, 4100, 2048, "S", "b", TILED, "kcut_split_count, panel_applies: n > 4096; t128 = 33 < 64"),
    R("kcut", 1024, 4096, 2048, "S", "b", RING_SPLIT, "cut_split_count: t128 = 128, two parts of 128-row tiles just fit a round"),
    R("kcut", 1025, 4096, 2048, "SR", "b", RING_SPLIT, "cut_split_count: t128 = 144 > 128: 256-row tiles, t256 = 80, 3 parts"),
    R("kcut", 300, 1024, 1920, "S", "b", TILED, "kcut_split_count: K < 2048"),
    R("kcut", 300, 4096, 2048, "S", "b", RING_SPLIT, "kcut_split_count: gemm_kcut = 1 where the panel form does not apply (t128 = 32)", gemm_kcut=1),
    R("kcut", 300, 8192, 2048, "S", "b", PANEL_SPLIT, "kcut_split_count: n > 4096 leaves the panel split alone"),
    R("kcut", 300, 1024, 2048, "S", "b", TILED, "plan_gemm: no workspace for the slabs", ws=False),
    # ---- ring kernel, one launch
    R("ring", 513, 7688, 256, "SFRG", "bh", RING, "ring_fills: t128 = 31 x 5 = 155 fills 60 %; last weight tile 8 wide (SwiGLU: n = 7680 + 32)"),
    R("ring", 513, 7680, 256, "S", "b", TILED, "ring_fills: t128 = 150 fills 58 %, and sk_any_plan has no plan at K = 256"),
    R("ring", 513, 7690, 128, "SF", "b", RING, "big_kernel_applies: the smallest K = 128, one lap of the four ring stages; n % 4 != 0"),
    R("ring", 640, 7936, 256, "S", "h", RING, "ring_fills: five full 128-row token tiles"),
    R("ring", 1100, 4608, 256, "SR", "b", RING, "ring_fills: t128 = 18 x 9 = 162"),
    # ---- ring kernel with the split-K tail
    R("ring_sk", 257, 4096, 1024, "SFR", "bh", RING_SK, "sk_plan_s, big_kernel_applies: gemm_sk = 2; t128 = 48 = sk_min_tiles, U = 8 = 4 S", gemm_sk=2, gemm_panel=0, gemm_kcut=0),
    R("ring_sk", 257, 4096, 896, "S", "b", TILED, "sk_plan_s: U = 7 < 4 S, no plan", gemm_sk=2, gemm_panel=0, gemm_kcut=0),
    R("ring_sk", 257, 3840, 1024, "S", "b", TILED, "big_kernel_applies: t128 = 45 < sk_min_tiles = 48", gemm_sk=2, gemm_panel=0, gemm_kcut=0),
    R("ring_sk", 384, 4160, 1024, "SG", "b", RING_SK, "sk_plan_s: three full token tiles, tn = 17, last weight tile 64 wide", gemm_sk=2, gemm_panel=0, gemm_kcut=0),
    R("ring_sk", 513, 4096, 1024, "S", "b", RING_SK, "sk_plan_s: R = 80 tiles of 128 rows x 2 parts, fifth token tile of one row", gemm_sk=2, gemm_panel=0, gemm_kcut=0),
    R("ring_sk", 513, 4352, 4096, "SR", "b", RING_SK, "sk_cost_us, big_choose: gemm_sk = 1, the cost model by itself: 85 tiles of 128 rows x 2 parts at K = 4096"),
    R("ring_sk", 513, 4352, 2560, "S", "b", TILED, "sk_cost_us, big_kernel_applies: at K = 2560 the seam costs more than it saves on 85 tiles, no plan, and the grid fills 33 %"),
    # ---- W8A8 weight-streaming kernel, no split
    R("fp8_wdma", 1, 16, 512, "S", "b", FP8_WDMA, "wdma8_applies: m = 1, n = 16, K = 512, the least of each"),
    R("fp8_wdma", 32, 128, 512, "SG", "b", FP8_WDMA, "launch_wdma8, wdma8_bn64: <32, 8, 64> full"),
    R("fp8_wdma", 33, 128, 640, "S", "b", FP8_WDMA, "launch_wdma8: m = 33 takes <64, 8, 64>; K = 512 + 128"),
    R("fp8_wdma", 64, 136, 512, "S", "b", FP8_WDMA, "launch_wdma8, wdma8_bn64: n % 64 != 0 takes 128-row tiles, <64, 6>; last tile 8 wide"),
    R("fp8_wdma", 65, 136, 512, "F", "b", FP8_WDMA, "launch_wdma8: m = 65 takes <128, 4>"),
    R("fp8_wdma", 128, 128, 512, "S", "b", FP8_WDMA, "launch_wdma8: <128, 6, 64> full"),
    R("fp8_wdma", 129, 128, 512, "F", "b", FP8_WDMA, "launch_wdma8: m = 129 takes <256, 4, 64> with 8 waves"),
    R("fp8_wdma", 256, 200, 512, "SG", "b", FP8_WDMA, "wdma8_applies, launch_wdma8: m = 256, <256, 3> full (SwiGLU: n = 224)"),
    R("fp8_wdma", 257, 128, 512, "S", "b", FP8_RING, "wdma8_applies, mx_split_count: m > 256; one 256-k unit, no cut"),
    R("fp8_wdma", 32, 200, 512, "S", "b", FP8_WDMA, "launch_wdma8: <32, 6> on 128-row tiles"),
    R("fp8_wdma", 40, 16384, 1024, "S", "b", FP8_WDMA, "wdma8_bn64, wdma8_split_count: n = 16384, 256 tiles of 64 rows, no split"),
    R("fp8_wdma", 40, 16448, 1024, "S", "b", FP8_WDMA, "wdma8_bn64, wdma8_split_count: n > 16384 takes 129 tiles of 128 rows, 256 / 129 = 1 part"),
    R("fp8_wdma", 40, 8256, 1024, "S", "b", FP8_WDMA, "wdma8_split_count: 129 tiles of 64 rows, 1 part"),
    R("fp8_wdma", 40, 1024, 896, "S", "b", FP8_WDMA, "wdma8_split_count: 7 k-tiles / 4 = 1 part"),
    R("fp8_wdma", 40, 128, 256, "S", "b", FP8_RING, "wdma8_applies: K < 512 takes the ring kernel (K % 256 == 0)"),
    R("fp8_wdma", 40, 1024, 1024, "SG", "b", FP8_WDMA, "plan_fp8: no workspace, one part per tile", ws=False),
    # ---- W8A8 weight-streaming kernel, split
    R("fp8_wdma_split", 40, 8192, 1024, "S", "b", FP8_WDMA_SPLIT, "wdma8_split_count: 128 tiles of 64 rows, min(2, 8 / 4) = 2 parts"),
    R("fp8_wdma_split", 32, 1024, 1024, "SFRG", "b", FP8_WDMA_SPLIT, "wdma8_split_count: K = 1024, the least that splits; <32, 8, 64> full"),
    R("fp8_wdma_split", 33, 1000, 1024, "S", "b", FP8_WDMA_SPLIT, "launch_wdma8: 128-row tiles, <64, 6>, the last 104 wide"),
    R("fp8_wdma_split", 64, 1024, 2560, "S", "b", FP8_WDMA_SPLIT, "wdma8_split_count: 20 k-tiles / 4 = 5 parts"),
    R("fp8_wdma_split", 65, 1024, 2048, "R", "b", FP8_WDMA_SPLIT, "wdma8_split_count: 4 parts; m = 65 takes <128, 6, 64>"),
    R("fp8_wdma_split", 128, 1000, 1024, "F", "b", FP8_WDMA_SPLIT, "launch_wdma8: <128, 4> full"),
    R("fp8_wdma_split", 129, 1024, 1024, "S", "b", FP8_WDMA_SPLIT, "launch_wdma8: m = 129 takes <256, 4, 64>"),
    R("fp8_wdma_split", 256, 1000, 1024, "SR", "b", FP8_WDMA_SPLIT, "launch_wdma8: <256, 3> full"),
    R("fp8_wdma_split", 40, 1024, 512, "R", "b", FP8_WDMA_SPLIT, "plan_fp8: the residual epilogue goes through slabs, one part per tile if need be"),
    R("fp8_wdma_split", 40, 1024, 512, "R", "b", FP8_RING, "plan_fp8: no room for slabs and K % 256 == 0: the ring kernel's own residual epilogue", ws=False),
    # ---- W8A8 ring kernel
    R("fp8_ring", 257, 1024, 512, "SFRG", "b", FP8_RING, "mx_split_count: (K / 256) / 2 = 1 part; second token tile of one row"),
    R("fp8_ring", 384, 1024, 768, "S", "b", FP8_RING, "mx_split_count: K = 768, still 1 part; three full 128-row tiles"),
    R("fp8_ring", 385, 1024, 512, "F", "b", FP8_RING, "launch_big_fp8, big_use_256_rows: fourth 128-row token tile of one row"),
    R("fp8_ring", 513, 1024, 1024, "SR", "b", FP8_RING, "mx_split_count: K < 8192 cuts up to 512 rows only"),
    R("fp8_ring", 300, 1022, 1024, "S", "b", FP8_RING, "plan_fp8: n % 4 != 0 leaves no slabs"),
    R("fp8_ring", 300, 1024, 1024, "S", "b", FP8_RING, "plan_fp8: no workspace", ws=False),
    R("fp8_ring", 513, 7688, 256, "S", "b", FP8_RING, "ring_fills, mx_split_count: t128 = 155 fills 60 %; the smallest K = 256; last weight tile 8 wide"),
    # ---- W8A8 ring kernel cut in K
    R("fp8_ring_split", 257, 1024, 1024, "SFRG", "b", FP8_RING_SPLIT, "mx_split_count, cut_split_count: m = 257, K = 1024: 2 parts of two 256-k units"),
    R("fp8_ring_split", 384, 1024, 2048, "S", "b", FP8_RING_SPLIT, "mx_split_count: 4 parts"),
    R("fp8_ring_split", 385, 1024, 2560, "R", "b", FP8_RING_SPLIT, "mx_split_count: 5 parts of 10 units; fourth token tile of one row"),
    R("fp8_ring_split", 512, 1024, 1024, "S", "b", FP8_RING_SPLIT, "mx_split_count: the last m at K < 8192"),
    R("fp8_ring_split", 600, 1024, 8192, "S", "b", FP8_RING_SPLIT, "mx_split_count: K >= 8192 cuts above 512 rows; t128 = 20, 12 parts"),
    R("fp8_ring_split", 512, 8192, 1024, "S", "b", FP8_RING_SPLIT, "mx_split_count, cut_split_count: t256 = 64, the most; t128 = 128, 2 parts"),
    # ---- W4A8
    R("fp4", 1, 64, 256, "S", "b", FP4, "w4a8_mi, w4a8_split_count: one row, one tile, one 256-k tile"),
    R("fp4", 32, 72, 256, "SR", "b", FP4, "w4a8_mi: MI = 1 full; last weight tile 8 wide"),
    R("fp4", 33, 72, 512, "S", "h", FP4, "w4a8_mi: m = 33 is MI = 2; K = 256 + 256"),
    R("fp4", 64, 200, 512, "G", "b", FP4, "w4a8_mi: MI = 2 full (SwiGLU: n = 224)"),
    R("fp4", 65, 200, 256, "S", "b", FP4, "w4a8_mi: m = 65 is MI = 4"),
    R("fp4", 128, 200, 256, "R", "h", FP4, "w4a8_mi: the 128-row tile full"),
    R("fp4", 129, 200, 256, "F", "b", FP4, "w4a8_mi: second token tile of one row"),
    R("fp4", 257, 64, 256, "S", "b", FP4, "w4a8_mi: third token tile of one row"),
    R("fp4", 40, 200, 2048, "SFRG", "bh", FP4, "w4a8_split_count: 8 k-tiles / 4 = 2 parts (SwiGLU: n = 224)"),
    R("fp4", 40, 200, 1792, "S", "b", FP4, "w4a8_split_count: 7 k-tiles / 4 = 1 part"),
    R("fp4", 300, 200, 3072, "SR", "b", FP4, "w4a8_split_count: 12 tiles over 3 parts of 4 k-tiles"),
    R("fp4", 40, 202, 2048, "S", "b", FP4, "ats_gemm_w4a8: n % 4 != 0 leaves no slabs"),
    R("fp4", 40, 200, 2048, "SR", "b", FP4, "ats_gemm_w4a8: no workspace, the epilogue in the kernel", ws=False),
    R("fp4", 8, 16384, 2048, "S", "b", FP4, "w4a8_split_count: 256 tiles, no split"),
    R("fp4", 8, 16320, 2048, "S", "b", FP4, "w4a8_split_count: 255 tiles, 2 parts"),
]


def out_n(row, epi):
    """the N a launch of (row, epi) runs: SwiGLU needs N % 32 == 0, so the row's n is raised to the next multiple of 32 (same tile counts)"""
    return (row.n + 31) // 32 * 32 if epi == SWIGLU else row.n


def case_id(row, epi, dt):
    sw = "".join(f"-{k[5:]}{v}" for k, v in row.sw)
    return f"{row.form}-{row.m}x{row.n}x{row.k}-{EPI_NAME[epi]}-{dt}{'' if row.ws else '-nows'}{sw}"


def cases():
    """every (row, epilogue, format) of the table"""
    return [(r, EPI[e], DT[d]) for r in TABLE for e in r.epis for d in r.dtypes]


# ------------------------------------------------------------------ hashed values
def _mix(r, c, seed):
    """32 well-mixed bits of (r, c, seed): int64 tensors, the same on every device"""
    x = (r * 0x9E3779B1 + c * 0x85EBCA77 + (seed * 0x27D4EB2F + 0x165667B1)) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x = x ^ (x >> 12)
    x = (x * 0x297A2D39) & 0xFFFFFFFF
    return x ^ (x >> 15)


def _val(h, mant, elo, ehi, odd=False):
    """+-(1 + man / 2^mant) 2^e, e in [elo, ehi], as float32 (exact); odd: the mantissa's last bit set (never a power of two)"""
    sign = 1 - 2 * (h & 1)
    e = (h >> 1) % (ehi - elo + 1) + elo
    man = (h >> 9) & ((1 << mant) - 1)
    if odd:
        man = man | 1
    return torch.ldexp((sign * ((1 << mant) + man)).to(torch.float32), (e - mant).to(torch.int32))


def _row_exp(r, swiglu):
    return (r % 13) // 2 - 6 if swiglu else r % 13 - 6


MANT = {"bf16": 7, "fp16": 10, "fp32": 7}          # the fp32 engine's operands hold bf16 values, so that its products stay exact
E4M3 = torch.tensor([(-1.0) ** (c >> 7) * ((c & 7) / 8 * 2.0 ** -6 if (c >> 3) & 15 == 0 else (1 + (c & 7) / 8) * 2.0 ** (((c >> 3) & 15) - 7)) for c in range(256)],
                    dtype=torch.float32)
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float32)


def _stride(K):
    s = max(1, int(K * 0.618)) | 1
    while np.gcd(s, K) != 1:
        s += 2
    return s


def kappa_w(N, K, pas):
    """the weight selector's k of rows 0 .. N-1 in launch `pas`: a permutation of (n + pas N) mod K"""
    j = (np.arange(N, dtype=np.int64) + pas * N) % K
    return (j * _stride(K) + K // 3) % K


def n_pass_w(N, K):
    return (K + N - 1) // N


@functools.lru_cache(maxsize=None)
def _targets(K):
    """the k the activation selector must take: the first and last 128 of K and one of every aligned 64-k chunk"""
    c = np.arange((K + 63) // 64, dtype=np.int64)
    t = np.concatenate([np.arange(min(128, K)), np.arange(max(K - 128, 0), K), np.minimum(c * 64 + (c * 37 + 11) % 64, K - 1)])
    _, first = np.unique(t, return_index=True)
    return t[np.sort(first)]


def n_pass_a(M, K):
    return (len(_targets(K)) + M - 1) // M


def kappa_a(M, K, pas):
    """the activation selector's k of rows 0 .. M-1 in launch `pas`: the targets in order, then a permutation of [0, K)"""
    t = _targets(K)
    j = np.arange(M, dtype=np.int64) + pas * M
    return np.where(j < len(t), t[np.minimum(j, len(t) - 1)], ((j - len(t)) * _stride(K) + K // 5) % K)


# ------------------------------------------------------------------ one launch
class Launch:
    """the operands of one launch of (row, epi, dt): selector `sel` ('W' / 'A'), launch number `pas`, scale variant `var` ('a' / 'b', W8A8)"""

    def __init__(self, row, epi, dt, sel, pas, var="a"):
        self.row, self.epi, self.dt, self.sel, self.pas, self.var = row, epi, dt, sel, pas, var
        self.fam, self.m, self.n, self.k = row.fam, row.m, out_n(row, epi), row.k
        self.swiglu = epi == SWIGLU
        self.seed = 1 + pas + (100 if sel == "A" else 0)
        self.kappa = kappa_w(self.n, self.k, pas) if sel == "W" else kappa_a(self.m, self.k, pas)
        rows = self.m if sel == "W" else self.n                     # rows of the DENSE operand
        self.zero_row = rows // 2 if rows >= 3 else -1
        self.name = f"{case_id(row, epi, dt)} {sel}{pas}{var if self.fam == 'w8a8' else ''}"
        self._acc = self._h = None                                  # built once per launch, dropped with it
        self.dev = "cpu"                                            # where the gathers below run: integer hashes and exact products, the same on any device

    # -- values (float32 tensors on the index tensors' device), before the row scales of the 8- and 4-bit families
    def _kap(self, r):
        return torch.from_numpy(self.kappa).to(r.device)[r]

    def _hot16(self, r):
        return _val(_mix(r, r * 0 + 7, self.seed + 50), MANT[self.dt], -3, 1 if self.swiglu else 2, odd=True)

    def _dense16(self, r, k):
        v = _val(_mix(r, k, self.seed), MANT[self.dt], -3, 0)
        return torch.where(r == self.zero_row, torch.zeros_like(v), torch.ldexp(v, _row_exp(r, self.swiglu).to(torch.int32) + 0 * k.to(torch.int32)))

    def _hot8(self, r):                                             # e4m3 codes, exponent field 4 .. 10, mantissa 1 .. 7
        h = _mix(r, r * 0 + 7, self.seed + 50)
        return ((h & 1) << 7) | ((4 + (h >> 1) % 7) << 3) | (1 + (h >> 9) % 7)

    def _dense8(self, r, k):                                        # W8A8: any e4m3 code but NaN; W4A8 activations: normal, < 16 (< 8: SwiGLU)
        h = _mix(r, k, self.seed)
        if self.fam == "w4a8":
            c = ((h & 1) << 7) | ((4 + (h >> 1) % (6 if self.swiglu else 7)) << 3) | ((h >> 9) & 7)
        elif self.swiglu:                                           # normal, in [1 / 4, 32): a tiny gate makes silu(g) u the tie-rich product g u / 2
            c = ((h & 1) << 7) | ((5 + (h >> 1) % 7) << 3) | ((h >> 9) & 7)
        else:
            c = h & 0xFF
            c = torch.where((c & 0x7F) == 0x7F, c - 1, c)
        return torch.where(r == self.zero_row, torch.zeros_like(c), c + 0 * k)

    def _zero_blk(self, n, blk):                                    # W4A8: the block of scale byte 0 and zero codes
        nz = self.n // 2 + 1 if self.n >= 3 else 0
        kz = int(self.kappa[nz]) // 32 if self.sel == "W" else -1
        return (n == nz) & (blk == (kz + 1) % (self.k // 32))

    def _scale4(self, n, blk):                                      # E8M0 bytes: 2^-4 .. 2^2 (2^-10 .. 2^-4: SwiGLU)
        sb = 127 + (n * 5 + blk * 3) % 7 - (10 if self.swiglu else 4)
        return torch.where(self._zero_blk(n, blk), torch.zeros_like(sb), sb)

    def _codes4(self, n, k):                                        # e2m1 codes of W
        if self.sel == "W":
            h = _mix(n, n * 0 + 7, self.seed + 50)
            c = torch.where(k == self._kap(n), (1 + (h >> 1) % 7) | ((h & 1) << 3), torch.zeros_like(h) + 0 * k)
        else:
            c = _mix(n, k, self.seed) & 15
            c = torch.where((c == 8) | (n == self.zero_row), torch.zeros_like(c), c)
        return torch.where(self._zero_blk(n, k // 32), torch.zeros_like(c), c)

    def a_codes(self, i, k):
        """e4m3 codes of A (W8A8, W4A8)"""
        return torch.where(k == self._kap(i), self._hot8(i) + 0 * k, torch.zeros_like(k + i)) if self.sel == "A" else self._dense8(i, k)

    def w_codes(self, n, k):
        """e4m3 codes of W (W8A8)"""
        return torch.where(k == self._kap(n), self._hot8(n) + 0 * k, torch.zeros_like(k + n)) if self.sel == "W" else self._dense8(n, k)

    def a_vals(self, i, k):
        if self.fam in ("w8a8", "w4a8"):
            return E4M3.to(i.device)[self.a_codes(i, k)]
        return torch.where(k == self._kap(i), self._hot16(i) + 0 * k, torch.zeros((), device=i.device)) if self.sel == "A" else self._dense16(i, k)

    def w_vals(self, n, k):
        if self.fam == "w8a8":
            return E4M3.to(n.device)[self.w_codes(n, k)]
        if self.fam == "w4a8":
            return torch.ldexp(E2M1.to(n.device)[self._codes4(n, k)], (self._scale4(n, k // 32) - 127).to(torch.int32))
        return torch.where(k == self._kap(n), self._hot16(n) + 0 * k, torch.zeros((), device=n.device)) if self.sel == "W" else self._dense16(n, k)

    # -- scale vectors (numpy float32)
    def _general(self, r, e):
        h = _mix(torch.from_numpy(r), torch.from_numpy(r) * 0 + 11, self.seed + 70).numpy()
        return np.ldexp(1.0 + (h & 0x7FFFFF) / 2.0 ** 23, e).astype(np.float32)

    def sx(self):
        i = np.arange(self.m, dtype=np.int64)
        if self.fam == "w8a8" and self.var == "b":
            return self._general(i, -1)                                                   # [0.5, 1)
        if self.fam == "w8a8" and self.swiglu:
            return np.ldexp(1.0, (i % 13) // 4 - 3).astype(np.float32)                   # |acc| < 450: |gate| < 450 * 2^-6
        return np.ldexp(1.0, _row_exp(i, self.swiglu)).astype(np.float32)

    def sw(self):
        n = np.arange(self.n, dtype=np.int64)
        if self.var == "b":
            return np.ldexp(1.0, (n % 13) // 4 - 9 if self.swiglu else n % 13 - 28).astype(np.float32)
        return self._general(n, (-8 if self.swiglu else -17) + (n % 2).astype(np.int64))  # [2^-17, 2^-15) ([2^-8, 2^-6): SwiGLU)

    # -- what the kernel is handed
    def operands(self, device="cpu"):
        """dict of tensors on `device`: a [M][K], w [N][K] in the family's storage (16 bit / fp32 values; e4m3 bytes; w: packed e2m1 nibbles and
        wsc [N][K / 32] scale bytes), sx / sw where the family has them"""
        I = torch.arange(self.m, device=device)[:, None]
        Nn = torch.arange(self.n, device=device)[:, None]
        Kk = torch.arange(self.k, device=device)[None, :]
        if self.fam in ("g16", "f32"):
            return dict(a=self.a_vals(I, Kk).to(TORCH[self.dt]), w=self.w_vals(Nn, Kk).to(TORCH[self.dt]))
        ops = dict(a=self.a_codes(I, Kk).to(torch.uint8), sx=torch.from_numpy(self.sx()).to(device))
        if self.fam == "w8a8":
            ops.update(w=self.w_codes(Nn, Kk).to(torch.uint8), sw=torch.from_numpy(self.sw()).to(device))
        else:
            c = self._codes4(Nn, Kk)
            ops.update(w=(c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8),
                       wsc=self._scale4(Nn, torch.arange(self.k // 32, device=device)[None, :]).to(torch.uint8))
        return ops

    def dense_float(self):
        """(A, W) as float32 CPU matrices of the dequantised values without sx / sw (the teeth checks' wrong kernels multiply these)"""
        I, Nn, Kk = torch.arange(self.m)[:, None], torch.arange(self.n)[:, None], torch.arange(self.k)[None, :]
        return self.a_vals(I, Kk) + torch.zeros(self.m, self.k), self.w_vals(Nn, Kk) + torch.zeros(self.n, self.k)

    # -- the exact result
    def k_of(self):
        """int64 [M][N]: the one k whose product an output element is"""
        return np.broadcast_to(self.kappa[None, :] if self.sel == "W" else self.kappa[:, None], (self.m, self.n))

    def acc64(self):
        """fp64 [M][N]: the one product a_i[k] w_n[k] of each element (exact in fp32: test_gemm_cases_cpu.py)"""
        if self._acc is None:
            self._acc = self._acc64()
        return self._acc

    def _acc64(self):
        I, Nn = torch.arange(self.m, device=self.dev)[:, None], torch.arange(self.n, device=self.dev)[None, :]
        kk = torch.from_numpy(np.array(self.k_of())).to(self.dev)
        return (self.a_vals(I + 0 * Nn, kk).double() * self.w_vals(Nn + 0 * I, kk).double()).cpu().numpy() + 0.0       # (a sum of +0 and -0 is +0)

    def exact(self):
        """fp64 [M][N]: the value the kernel's fp32 result must hold before its epilogue"""
        p = self.acc64()
        if self.fam == "w8a8":
            gen, two = (self.sw()[None, :], self.sx()[:, None]) if self.var == "a" else (self.sx()[:, None], self.sw()[None, :])
            return (p.astype(np.float32) * gen).astype(np.float64) * two          # fl32(acc * general) * 2^e
        if self.fam == "w4a8":
            return p * self.sx()[:, None].astype(np.float64)
        return p

    def resid(self):
        """fp64 [M][N] values of the format: random h with |exponent(h) - exponent(p)| <= 12 (fp16: kept normal and below 2^15)"""
        if self._h is None:
            self._h = self._resid()
        return self._h

    def _resid(self):
        p = self.exact()
        ep = np.where(p == 0, 0, np.frexp(p)[1] - 1)
        I, Nn = torch.arange(self.m, device=self.dev)[:, None], torch.arange(self.n, device=self.dev)[None, :]
        h = _mix(I + 0 * Nn, Nn + 0 * I, self.seed + 90).cpu().numpy()
        mant = 23 if self.dt == "fp32" else MANT[self.dt]
        e = ep + (h >> 1) % 25 - 12
        if self.dt == "fp16":
            e = np.clip(e, -14, 14)
        man = (h >> 6) & ((1 << mant) - 1)
        return np.ldexp((1 - 2 * (h & 1)) * ((1 << mant) + man).astype(np.float64), (e - mant).astype(np.int64))


def launches(row, epi, dt):
    """the launches of one case: the weight selector until kappa has covered [0, K) (W8A8: in both scale variants), then the activation
    selector until kappa' has taken every target (W8A8: the variants in turn)"""
    n, out = out_n(row, epi), []
    for pas in range(n_pass_w(n, row.k)):
        out += [Launch(row, epi, dt, "W", pas, v) for v in ("ab" if row.fam == "w8a8" else "a")]
    out += [Launch(row, epi, dt, "A", pas, "ab"[pas % 2] if row.fam == "w8a8" else "a") for pas in range(n_pass_a(row.m, row.k))]
    return out


# ------------------------------------------------------------------ expected values and the judge
def silu64(g):
    return g / (1.0 + np.exp(-g))


def gate_up(p):
    """[M][N] in interleaved 16-row groups -> gate, up [M][N / 2]"""
    v = p.reshape(p.shape[0], p.shape[1] // 32, 2, 16)
    return v[:, :, 0].reshape(p.shape[0], -1), v[:, :, 1].reshape(p.shape[0], -1)


def expected(L: Launch):
    """fp64 array of the launch's expected output (SWIGLU: the fp64 reference the judge rounds)"""
    p, dt = L.exact(), L.dt
    rnd = (lambda x: x.astype(np.float32).astype(np.float64)) if dt == "fp32" else (lambda x: RD.round_to(x, dt))
    if L.epi == F32:
        return p.astype(np.float32).astype(np.float64)
    if L.epi == STORE:
        return rnd(p)
    if L.epi == RESID:
        return rnd(L.resid() + (p if dt == "fp32" else rnd(p)))
    g, u = gate_up(p)
    return silu64(g) * u if dt == "fp32" else silu64(rnd(g)) * rnd(u)


def _bits(x, dt):
    x = np.asarray(x, dtype=np.float64)
    if dt == "fp32":
        return x.astype(np.float32).view(np.uint32)
    return torch.from_numpy(x).to(TORCH[dt]).view(torch.int16).numpy().view(np.uint16)


def blame(L: Launch, i, j):
    """where the product of output element (i, j) comes from: the text of a failure message"""
    cols = [j] if L.epi != SWIGLU else [32 * (j // 16) + j % 16, 32 * (j // 16) + 16 + j % 16]
    what = []
    for n in cols:
        k = int(L.k_of()[i, n])
        what.append(f"n={n} k={k} (k-step {k // 32}, ring stage {(k // 32) % 4}, 64-k tile {k // 64}, 128-k unit {k // 128} of {(L.k + 127) // 128}, "
                    f"16-byte chunk {k % 64 // 8 if L.fam in ('g16', 'f32') else k % 128 // 16})")
    return f"row i={i} {' / '.join(what)}, selector {L.sel}, exact fp32 value(s) {[float(L.exact()[i, n]) for n in cols]!r}"


def judge(L: Launch, got):
    """got: the kernel's output [M][N] ([M][N / 2]: SwiGLU) as a float array.  Raises AssertionError naming the first wrong element."""
    out_dt = "fp32" if L.epi == F32 else L.dt
    want = expected(L)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (L.name, got.shape, want.shape)
    if L.epi == SWIGLU:
        if L.dt == "fp32":
            bad = ~(np.abs(got - want) <= RD.REL * np.abs(want))
            rule = f"silu(g) u within {RD.REL:.3e} relative"
        else:
            try:
                RD.assert_rounded(got, want, L.dt, name=L.name)
                return
            except AssertionError as e:
                if "near ties" in str(e) and "not the rounded" not in str(e):
                    raise
                band = RD.REL * np.abs(want)
                bad = ~((got >= RD.round_to(want - band, L.dt)) & (got <= RD.round_to(want + band, L.dt)))
                rule = "round_to(silu(round_to(g)) round_to(u))"
    else:
        bad = _bits(got, out_dt) != _bits(want, out_dt)
        rule = {F32: "p", STORE: "round_to(p)", RESID: "round_to(h + round_to(p))" if L.dt != "fp32" else "fl32(h + p)"}[L.epi]
    if bad.any():
        i, j = (int(x) for x in np.argwhere(bad)[0])
        extra = f", h {float(L.resid()[i, j])!r}" if L.epi == RESID else ""
        raise AssertionError(f"{L.name}: {int(bad.sum())} of {bad.size} elements differ from {rule}; first at ({i}, {j}): got {got[i, j]!r} "
                             f"(bits {int(_bits(got[i, j], out_dt)):#x}), expected {want[i, j]!r} (bits {int(_bits(want[i, j], out_dt)):#x}){extra}; "
                             f"{blame(L, i, j)}")
