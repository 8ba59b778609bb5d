"""tests/gemm_cases.py proved on the CPU, without a GPU or the library: the selectors cover what they claim, every product is exact in fp32,
the conditions the expected values rest on hold, the table is sane -- and the judge has teeth: the output of each wrong kernel of the list
below is rejected, that of a correct fp32 emulation in another summation order passes.

Exact ties (`STORE`): a product of two bf16 values has 16 mantissa bits and of two fp16 values 22, so ties of the 16-bit rounding are common
and asserted present in every 16-bit STORE case.  The 8- and 4-bit families cannot promise them: an e4m3 x e2m1 product has 6 mantissa bits (it
IS a bf16 / fp16 value), and a W8A8 value is fl32(acc * scale), a tie once in 2^16 elements."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gemm_cases as GC
from tests import rounding as RD

CASES = GC.cases()
IDS = [GC.case_id(*c) for c in CASES]
GEMM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "atspeed_amd", "csrc", "gemm.hip")
FULL = 1_200_000          # a case of more output elements than this (all launches together) is checked on the first launch of each selector and variant,
# the rows whose predicate needs K > 2560: make_plan's cap of 16 parts (64 k-tiles), wdma_split_count at n = 2048 (80 k-tiles for 10 parts) and just
# below it, mx_split_count above 512 rows (K >= 8192), the one K at which sk_cost_us takes a tail by itself at a small shape, and w4a8_split_count's
# third part (12 k-tiles of 256)
DEEP_K = {(1, 128, 4096), (40, 2048, 5120), (40, 2040, 5120), (600, 1024, 8192), (513, 4352, 4096), (300, 200, 3072)}
BAND = 600_000            # ... and on its first BAND / N rows: values are hashes of (row, column, seed), the same whatever M is


# ------------------------------------------------------------------ the table
def test_table_is_sane():
    assert len(set(IDS)) == len(IDS), "two rows pin the same case"
    assert {r.counter for r in GC.TABLE} == set(range(GC.N_COUNTERS)), "every counted form appears as some row's expected counter"
    assert 100 <= len(GC.TABLE) <= 200
    forms = {r.form for r in GC.TABLE}
    assert forms == {"tiled", "tiled32", "ring_split", "wdma", "wdma_split", "panel", "panel_split", "kcut", "ring", "ring_sk", "fp8_wdma", "fp8_wdma_split",
                     "fp8_ring", "fp8_ring_split", "fp4"}
    for r in GC.TABLE:
        assert r.n <= 33000 and set(r.epis) <= set("SFRG") and set(r.dtypes) <= set("bhf"), r
        assert r.k <= 2560 or (r.m, r.n, r.k) in DEEP_K, r
        if r.fam in ("w8a8",):
            assert r.dtypes == "b", "the W8A8 entry point is bf16"
    # each form's own counter is pinned with every epilogue it has and, where it has them, both 16-bit types
    own = {"tiled": GC.TILED, "ring_split": GC.RING_SPLIT, "wdma": GC.WDMA, "wdma_split": GC.WDMA_SPLIT, "panel": GC.PANEL, "panel_split": GC.PANEL_SPLIT,
           "kcut": GC.RING_SPLIT, "ring": GC.RING, "ring_sk": GC.RING_SK, "fp8_wdma": GC.FP8_WDMA, "fp8_wdma_split": GC.FP8_WDMA_SPLIT, "fp8_ring": GC.FP8_RING,
           "fp8_ring_split": GC.FP8_RING_SPLIT, "fp4": GC.FP4, "tiled32": GC.TILED}
    no_epi = {"wdma": "R", "kcut": "G", "fp8_wdma": "R"}                 # wdma_applies / kcut_split_count / plan_fp8 send these elsewhere
    for form, c in own.items():
        rows = [r for r in GC.TABLE if r.form == form and r.counter == c]
        assert set("".join(r.epis for r in rows)) == set("SFRG") - set(no_epi.get(form, "")), form
        if rows[0].fam in ("g16", "w4a8"):
            assert set("".join(r.dtypes for r in rows)) == set("bh"), form


def test_every_row_names_predicates_of_gemm_hip():
    src = open(GEMM_HIP).read()
    for r in GC.TABLE:
        head, _, rest = r.why.partition(":")
        assert rest.strip(), r
        for name in head.split(","):
            name = name.strip()
            assert re.fullmatch(r"[a-z_0-9]+", name), (name, r)
            assert re.search(rf"\b{name}\(", src), f"{name} is no function of gemm.hip ({r})"


# ------------------------------------------------------------------ the selectors
@pytest.mark.parametrize("n,k", sorted({(GC.out_n(r, e), r.k) for r, e, _ in CASES}))
def test_weight_selector_covers_k(n, k):
    seen = np.zeros(k, dtype=bool)
    for pas in range(GC.n_pass_w(n, k)):
        kap = GC.kappa_w(n, k, pas)
        assert kap.shape == (n,) and kap.min() >= 0 and kap.max() < k
        seen[kap] = True
        if n > 1 and k > 64:
            assert np.abs(np.diff(kap)).min() > 8, "neighbouring rows select neighbouring k"
    assert seen.all()


@pytest.mark.parametrize("m,k", sorted({(r.m, r.k) for r in GC.TABLE}))
def test_activation_selector_meets_its_conditions(m, k):
    kap = np.concatenate([GC.kappa_a(m, k, pas) for pas in range(GC.n_pass_a(m, k))])
    assert kap.min() >= 0 and kap.max() < k
    hit = np.zeros(k, dtype=bool)
    hit[kap] = True
    assert hit[: min(128, k)].all() and hit[max(0, k - 128):].all(), "the first and the last 128 of K"
    assert len(set((kap % 128).tolist())) == min(128, k), "every residue of k mod 128"
    for c in range((k + 63) // 64):
        assert hit[64 * c: 64 * c + 64].any(), f"no k in the 64-k chunk {c}: a part of a K split may hold none"


# ------------------------------------------------------------------ the values
def _checked_launches(row, epi, dt):
    ls = GC.launches(row, epi, dt)
    if sum(L.m * L.n for L in ls) <= FULL:
        return ls
    first = {}
    for L in GC.launches(row._replace(m=min(row.m, max(40, BAND // row.n))), epi, dt):
        first.setdefault((L.sel, L.var), L)
    return list(first.values())


@pytest.mark.parametrize("row,epi,dt", CASES, ids=IDS)
def test_products_are_exact_and_the_conditions_hold(row, epi, dt):
    ties = elems = 0
    for L in _checked_launches(row, epi, dt):
        p = L.acc64()
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p), f"{L.name}: a product is not exact in fp32"
        v = L.exact()
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v) and np.isfinite(v).all()
        nz = np.abs(v[v != 0])
        assert nz.size and nz.min() >= 2.0 ** -100, "no result near the subnormals of fp32"
        zr = L.zero_row
        if zr >= 0:
            assert not (v[zr] if L.sel == "W" else v[:, zr]).any(), "the all-zero row"
        if L.fam in ("w8a8", "w4a8"):                             # (the dense e4m3 codes include +-0, the dense e2m1 codes 0 twice in 16)
            assert (v == 0).mean() <= 0.25 + 1.0 / max(min(L.m, L.n), 3)
        else:
            assert (np.count_nonzero(v, axis=1) > 0).sum() >= L.m - 1 and (np.count_nonzero(v, axis=0) > 0).sum() >= L.n - 1
        if L.fam in ("g16", "f32"):
            mant = np.frexp(np.abs(nz))[0]
            assert (mant != 0.5).mean() > 0.99, "the selected values are no powers of two"
        if L.fam == "w8a8":                                       # one scale vector powers of two, the other not
            two, gen = (L.sx(), L.sw()) if L.var == "a" else (L.sw(), L.sx())
            assert (np.frexp(two)[0] == 0.5).all() and (np.frexp(gen)[0] != 0.5).mean() > 0.99 and len(set(two[:13].tolist())) >= min(4, two.size)
        if epi == GC.RESID:
            h = L.resid()
            rp = v if dt == "fp32" else RD.round_to(v, dt)
            assert np.array_equal(RD.round_to(h, dt) if dt != "fp32" else h.astype(np.float32).astype(np.float64), h), "h holds values of the format"
            gap = np.abs((np.frexp(h)[1] - np.frexp(v)[1])[v != 0])
            assert gap.max() <= 12, f"{L.name}: |exponent(h) - exponent(p)| = {gap.max()}"
            s = h + rp
            if dt != "fp32":
                assert np.array_equal(s.astype(np.float32).astype(np.float64), s), "the fp32 sum h + round_to(p) is exact"
                assert np.isfinite(RD.round_to(s, dt)).all()
        if epi == GC.SWIGLU:
            g, u = GC.gate_up(v)
            assert np.abs(g).max() <= 8.0, f"{L.name}: |gate| = {np.abs(g).max()}"
            if dt != "fp32":
                share = float(RD.near_tie(GC.expected(L), dt).mean())
                assert share <= RD.CAP, f"{L.name}: {share:.4%} near ties"
        if epi == GC.STORE and L.fam == "g16":
            lo, _, u = RD._floor_ceil(v, dt)
            ties += int((v == lo + 0.5 * u).sum())
            elems += v.size
    if epi == GC.STORE and row.fam == "g16":
        assert ties > 0, f"no exact tie among {elems} products"


# ------------------------------------------------------------------ the judge has teeth
CHUNK = {"g16": 8, "f32": 4, "w8a8": 16, "w4a8": 16}             # elements of A in a 16-byte chunk


def _kernel(L, wrong=None):
    """the output a kernel would give: fp32 sums over 32-k steps from the LAST step to the first, the scales applied as (acc sx) sw, the
    epilogue in fp32 (torch on the CPU) -- correct, or wrong in the one way named"""
    A, W = L.dense_float()
    K, dt = L.k, L.dt
    if wrong == "k_shift":
        A = torch.roll(A, CHUNK[L.fam], 1)
    if wrong == "stale_stage":
        s = next(int(k) // 32 for k in L.kappa if k >= 32)
        A = A.clone()
        A[:, 32 * s: 32 * s + 32] = A[:, 32 * s - 32: 32 * s]
    k_end = K - K // 4 if wrong == "drop_last_part" else K
    acc = torch.zeros(L.m, L.n)
    for k0 in range((k_end - 1) // 32 * 32, -1, -32):
        acc += A[:, k0: min(k0 + 32, k_end)] @ W[:, k0: min(k0 + 32, k_end)].T
    if L.fam in ("w8a8", "w4a8"):
        sx = torch.from_numpy(L.sx())
        acc = acc * (torch.roll(sx, 1) if wrong == "sx_row" else sx)[:, None]
    if L.fam == "w8a8":
        sw = torch.from_numpy(L.sw())
        acc = acc * (torch.roll(sw, -1) if wrong == "sw_row" else sw)[None, :]
    td = GC.TORCH[dt]
    if L.epi == GC.F32:
        out = acc
    elif L.epi == GC.STORE:
        out = acc.to(td)
        if wrong == "truncate":
            lo, hi, _ = RD._floor_ceil(acc.double().numpy(), dt)
            out = torch.from_numpy(np.where(acc.numpy() >= 0, lo, hi))
    elif L.epi == GC.RESID:
        h = torch.from_numpy(L.resid()).to(td).float()
        out = (h + acc).to(td) if wrong == "resid_once" or dt == "fp32" else (h + acc.to(td).float()).to(td)
    else:
        g, u = (torch.from_numpy(np.ascontiguousarray(x)) for x in GC.gate_up(acc.numpy()))
        if wrong != "swiglu_unrounded":
            g, u = g.to(td).float(), u.to(td).float()
        out = (g / (1 + torch.exp(-g)) * u).to(td)
    out = out.double().numpy()
    return np.roll(out, 1, axis=0) if wrong == "row_off" else out


def _teeth_row(form, counter, dtype="b"):
    rows = [r for r in GC.TABLE if r.form == form and r.counter == counter and dtype in r.dtypes and r.m >= 32]
    return min(rows, key=lambda r: r.m * r.n * r.k)


TEETH = [  # (row, format, what the family's wrong kernels are tried on)
    (_teeth_row("tiled", GC.TILED), "bf16"), (_teeth_row("tiled", GC.TILED, "h"), "fp16"), (_teeth_row("tiled32", GC.TILED, "f"), "fp32"),
    (_teeth_row("fp8_wdma_split", GC.FP8_WDMA_SPLIT), "bf16"), (_teeth_row("fp8_ring_split", GC.FP8_RING_SPLIT), "bf16"),
    (_teeth_row("fp4", GC.FP4), "bf16"), (_teeth_row("fp4", GC.FP4, "h"), "fp16"),
    (_teeth_row("ring_split", GC.RING_SPLIT), "bf16"), (_teeth_row("kcut", GC.RING_SPLIT, "h"), "fp16"),
]


def _rejected(L, wrong):
    try:
        GC.judge(L, _kernel(L, wrong))
    except AssertionError as e:
        assert "k-step" in str(e) and "ring stage" in str(e) and "bits" in str(e), "the message names the place and the bits"
        return True
    return False


@pytest.mark.parametrize("row,dt", TEETH, ids=[f"{r.form}-{r.m}x{r.n}x{r.k}-{d}" for r, d in TEETH])
def test_the_judge_rejects_every_wrong_kernel_and_accepts_a_correct_one(row, dt):
    epis = [GC.STORE, GC.RESID, GC.SWIGLU, GC.F32]
    for epi in epis:
        W0 = GC.Launch(row, epi, dt, "W", 0)
        A_last = GC.Launch(row, epi, dt, "A", GC.n_pass_a(row.m, row.k) - 1, "b")
        for L in (W0, A_last):
            GC.judge(L, _kernel(L))                                # a correct kernel in another summation order passes
        wrongs = ["k_shift", "stale_stage", "drop_last_part", "row_off"]
        if dt != "fp32" and row.fam != "w4a8":                      # (an e4m3 x e2m1 product times 2^e IS a 16-bit value: nothing to round)
            wrongs += {GC.STORE: ["truncate"], GC.RESID: ["resid_once"], GC.SWIGLU: ["swiglu_unrounded"], GC.F32: []}[epi]
        if row.fam in ("w8a8", "w4a8"):
            wrongs.append("sx_row")
        if row.fam == "w8a8":
            wrongs.append("sw_row")
        for wrong in wrongs:
            assert _rejected(W0, wrong), f"{W0.name}: a kernel wrong by `{wrong}` passes the judge"
        for wrong in ("k_shift", "row_off") + (("sx_row",) if row.fam != "g16" and row.fam != "f32" else ()) + (("sw_row",) if row.fam == "w8a8" else ()):
            assert _rejected(A_last, wrong), f"{A_last.name}: a kernel wrong by `{wrong}` passes the judge"


def test_a_wrong_scale_variant_is_told_apart():
    """W8A8 variant `b` (sw powers of two, sx general) against variant `a`'s result: the two pin both scale vectors' indices"""
    row = _teeth_row("fp8_wdma_split", GC.FP8_WDMA_SPLIT)
    a, b = GC.Launch(row, GC.STORE, "bf16", "W", 0, "a"), GC.Launch(row, GC.STORE, "bf16", "W", 0, "b")
    GC.judge(b, _kernel(b))
    with pytest.raises(AssertionError):
        GC.judge(b, _kernel(a))
