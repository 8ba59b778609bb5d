"""Guard-band tests: strides, halos and workspace edges of every kernel (tests/guard.py).

tests/test_kernels_gpu.py holds the kernels' arithmetic to fp64 / bit-exact references, always on dense operands straight from the torch
allocator.  Here every case runs the SAME call twice -- once on such dense buffers, once on operands carved out of an `Arena`: 16 bytes past
a 256-byte boundary, rows further apart than they are wide, NaN in every input byte outside the stated extent (halos, row gaps, pad rows,
weight rows >= n, cache slots >= n_slots, logit columns >= vocab), seeded random bytes around every output and after `workspace_bytes` --
and asserts (1) no guard byte changed, (2) the result is the dense call's bit for bit and, for the GEMMs, `atspeed_gemm_path_counters`
shows the same, intended form for both calls.  No case needed the fall-back to the fp64 tolerance: the strides used here (lda % 8 == 0)
change no form.  Nothing here can fault: every halo is allocated memory at least one tile (256 rows) deep."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib
from tests import guard
from tests.guard import Arena
from tests.mxfp4_ref import dequant_mxfp4

DEV = "cuda"
EPI_NAME = {0: "store", 1: "f32", 2: "resid", 3: "swiglu"}
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
# atspeed_gemm_path_counters
RING, RING_SK, WDMA, WDMA_SPLIT, RING_SPLIT, TILED, FP8_RING, FP8_WDMA, FP8_WDMA_SPLIT, PANEL, PANEL_SPLIT, FP8_RING_KCUT, W4A8 = range(13)
WS_BYTES = 128 << 20


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _st():
    return _lib.stream_ptr()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, std=1.0, dtype=torch.float32):
    return (torch.randn(shape, generator=g, device=DEV) * std).to(dtype)


def _counters(lib, reset=False):
    out = (C.c_int64 * 16)()
    lib.atspeed_gemm_path_counters(out, 16, 1 if reset else 0)
    return list(out)


def _up(x, q):
    return (x + q - 1) // q * q


def _out_geometry(n, epi, dtype):
    """(columns, dtype, gapped row stride) of a GEMM output: the gap is a multiple of 8 (16-bit) / 4 (fp32) elements and of no 64"""
    cols = n // 2 if epi == _lib.EPI_SWIGLU else n
    odt = torch.float32 if (epi == _lib.EPI_F32 or dtype == torch.float32) else dtype
    return cols, odt, (_up(cols, 4) + 20 if odt == torch.float32 else _up(cols, 8) + 40)


# ------------------------------------------------------------------ atspeed_gemm: one shape per form the counters distinguish
SK_SW = dict(gemm_sk=2, gemm_panel=0, gemm_kcut=0)
PANEL_SW = dict(gemm_panel=2, gemm_kcut=0)
# form, counter, switches that force it (as the form's own test in test_kernels_gpu.py does), (m, n, k), epilogues, 16-bit types
G16_FORMS = [
    ("ring", RING, dict(gemm_sk=0), (4200, 8200, 256), (0, 1, 2), "both"),             # ragged m and n, 16-byte stores straddling N
    ("ring", RING, dict(gemm_sk=0), (4200, 8480, 256), (3,), "both"),                  # SwiGLU needs N % 32 == 0: ffn 4240
    ("ring_sk_tail", RING_SK, SK_SW, (400, 4096, 4096), (0, 1, 2, 3), "both"),
    ("ring_sk_tail", RING_SK, SK_SW, (700, 32859, 2048), (1,), "bf16"),
    ("wstream", WDMA, {}, (121, 32859, 768), (0, 1), "both"),                          # (the form has no residual epilogue)
    ("wstream", WDMA, {}, (110, 22016, 512), (3,), "both"),
    ("wstream_split", WDMA_SPLIT, {}, (100, 12288, 1024), (0, 1, 2, 3), "both"),
    ("wstream_split", WDMA_SPLIT, {}, (100, 12296, 1024), (0, 1, 2), "bf16"),         # 97 tiles of 128 weight rows, the last one 8 rows wide
    ("ring_split", RING_SPLIT, {}, (129, 8448, 256), (0, 1, 2, 3), "both"),
    ("ring_split", RING_SPLIT, {}, (256, 9000, 384), (0, 1, 2), "bf16"),
    ("kcut", RING_SPLIT, {}, (320, 4096, 4096), (0, 1, 2), "both"),                    # (SwiGLU never takes the K-cut form)
    ("kcut", RING_SPLIT, {}, (1099, 1028, 2304), (0,), "bf16"),
    ("tiled", TILED, {}, (20, 4096, 768), (0, 1, 2, 3), "both"),
    ("tiled", TILED, {}, (5, 200, 96), (0, 1, 2), "bf16"),
    ("panel", PANEL, PANEL_SW, (320, 22016, 4096), (0, 1, 2, 3), "both"),
    ("panel", PANEL, PANEL_SW, (320, 22024, 4096), (0, 1, 2), "bf16"),                 # 173 panels, the last one 8 rows wide
    ("panel_split", PANEL_SPLIT, PANEL_SW, (320, 4096, 4096), (0, 1, 2, 3), "both"),
    ("panel_split", PANEL_SPLIT, PANEL_SW, (320, 4104, 4096), (0, 1), "bf16"),
]
# fp32 runs on the LDS-tiled kernel only; 96 / 352 / 1376: a K tail inside a tile
F32_SHAPES = [(5, 200, 96), (16, 384, 352), (257, 640, 1376)]


def _g16_cases():
    out = []
    for form, idx, sw, (m, n, k), epis, types in G16_FORMS:
        for dt in ((torch.bfloat16, torch.float16) if types == "both" else (torch.bfloat16,)):
            for e in epis:
                out.append(pytest.param(form, idx, sw, m, n, k, e, dt, id=f"{form}-{m}x{n}x{k}-{EPI_NAME[e]}-{DT_NAME[dt]}"))
    for m, n, k in F32_SHAPES:
        for e in (0, 1, 2, 3):
            if e != 3 or n % 32 == 0:
                out.append(pytest.param("tiled", TILED, {}, m, n, k, e, torch.float32, id=f"tiled-{m}x{n}x{k}-{EPI_NAME[e]}-fp32"))
    return out


@pytest.mark.parametrize("form,idx,sw,m,n,k,epi,dtype", _g16_cases())
def test_gemm_guard_bands(lib, form, idx, sw, m, n, k, epi, dtype):
    """atspeed_gemm, every 16-bit form x epilogue x {bf16, fp16} and fp32 on the LDS-tiled kernel: lda = k + 40 (fp32: + 20), ldc gapped,
    NaN after row m of a, after column k of every row of a and after row n of w, random bytes around c and after workspace_bytes."""
    g = _gen(m + n + k + epi)
    code = _lib.dtype_code(dtype)
    a = _randn((m, k), g, 1.0, dtype)
    w = _randn((n, k), g, 0.05, dtype)
    cols, odt, ldc = _out_geometry(n, epi, dtype)
    base = _randn((m, cols), g, 1.0, odt) if epi == _lib.EPI_RESID else None
    ws0 = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
    c0 = base.clone() if base is not None else torch.zeros(m, cols, dtype=odt, device=DEV)
    ar = Arena(DEV, seed=epi)
    av = ar.input("a", a, ld=k + (20 if dtype == torch.float32 else 40))
    wv = ar.input("w", w)
    cv = ar.output("c", m, cols, odt, ld=ldc, init=base)
    wsv = ar.workspace("workspace", WS_BYTES)
    ar.snapshot()
    with _lib.switches(**sw):
        _counters(lib, reset=True)
        _lib.check(lib.atspeed_gemm(a.data_ptr(), w.data_ptr(), c0.data_ptr(), m, n, k, k, cols, code, epi, ws0.data_ptr(), WS_BYTES, _st()))
        cnt0 = _counters(lib, reset=True)
        _lib.check(lib.atspeed_gemm(av.ptr, wv.ptr, cv.ptr, m, n, k, av.ld, ldc, code, epi, wsv.ptr, WS_BYTES, _st()))
        cnt1 = _counters(lib)
        torch.cuda.synchronize()
    assert cnt0[idx] == 1 and sum(cnt0[:13]) == 1, (form, cnt0)
    assert cnt1 == cnt0, ("the strides changed the form", cnt0, cnt1)
    ar.check()
    guard.assert_same("c", cv.t, c0)


# ------------------------------------------------------------------ packed operands: the pad row of an odd row count
def _pack(lib, t):
    rows, cols = t.shape
    out = torch.zeros((rows + 1) // 2 * 2, cols, dtype=t.dtype, device=DEV)
    _lib.check(lib.atspeed_pack_rows(t.data_ptr(), out.data_ptr(), rows, cols * t.element_size(), _st()))
    return out


def _packed_input(ar, name, packed, rows, kind=None):
    """a packed operand of `rows` rows as an Arena input: an odd count's pad row is poisoned"""
    v = ar.input(name, packed, kind=kind)
    if rows % 2:
        v.add_guard(guard.packed_row_offsets(rows, packed.shape[1] * packed.element_size()), guard.POISON[v.kind])
    return v


def _packed_swiglu_out(ar, m, cols, gap, odt):
    """the packed output of a SwiGLU epilogue, m odd: rows ld = cols + gap elements apart (gap: 0 or 32), the pad row and the gap are guard bytes"""
    assert m % 2 == 1 and cols % 32 == 0 and gap % 32 == 0
    ld = cols + gap
    cv = ar.output("c", m + 1, ld, odt)
    cv.add_guard(guard.packed_row_offsets(m, ld * 2))
    if gap:
        cv.add_guard(guard.packed_gap_offsets(m, cols * 2, ld * 2))
    return cv, ld


def _assert_packed_swiglu(lib, cv, ld, c0, m, cols):
    """rows 0 .. m - 1, columns 0 .. cols - 1 of the packed arena output against the dense packed call's"""
    u1 = torch.empty(m, ld, dtype=c0.dtype, device=DEV)
    u0 = torch.empty(m, cols, dtype=c0.dtype, device=DEV)
    _lib.check(lib.atspeed_unpack_rows(cv.ptr, u1.data_ptr(), m, ld * 2, _st()))
    _lib.check(lib.atspeed_unpack_rows(c0.data_ptr(), u0.data_ptr(), m, cols * 2, _st()))
    torch.cuda.synchronize()
    guard.assert_same("c", u1[:, :cols], u0)


@pytest.mark.parametrize("m,n,k,epi,gap", [(121, 32859, 256, 1, 0), (225, 22016, 512, 3, 0), (225, 22016, 512, 3, 32), (33, 16384, 576, 0, 0), (777, 4096, 1024, 2, 0),
                                          (321, 22016, 4096, 3, 0), (321, 22016, 4096, 3, 32)], ids=lambda v: str(v))
def test_gemm_packed_pad_rows(lib, m, n, k, epi, gap):
    """atspeed_gemm_packed with an odd m (and an odd n: 32859): the poisoned pad row of a (and of w) reaches no output row < m; the
    SwiGLU epilogue's packed output keeps its pad row untouched and, with ldc = N / 2 + 32, its row gap too."""
    g = _gen(m + n)
    a = _randn((m, k), g, 1.0, torch.bfloat16)
    w = _randn((n, k), g, 0.05, torch.bfloat16)
    ap, wp = _pack(lib, a), _pack(lib, w)
    cols, odt, ldc = _out_geometry(n, epi, torch.bfloat16)
    me = (m + 1) // 2 * 2
    ws0 = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
    ar = Arena(DEV)
    av, wv = _packed_input(ar, "a", ap, m), _packed_input(ar, "w", wp, n)
    wsv = ar.workspace("workspace", WS_BYTES)
    if epi == _lib.EPI_SWIGLU:
        c0 = torch.zeros(me, cols, dtype=odt, device=DEV)
        cv, ld1 = _packed_swiglu_out(ar, m, cols, gap, odt)
        ld0 = cols
    else:
        base = _randn((m, cols), g, 1.0, odt) if epi == _lib.EPI_RESID else None
        c0 = base.clone() if base is not None else torch.zeros(m, cols, dtype=odt, device=DEV)
        cv = ar.output("c", m, cols, odt, ld=ldc, init=base)
        ld0, ld1 = cols, ldc
    ar.snapshot()
    _counters(lib, reset=True)
    _lib.check(lib.atspeed_gemm_packed(ap.data_ptr(), wp.data_ptr(), c0.data_ptr(), m, n, k, ld0, epi, ws0.data_ptr(), WS_BYTES, _st()))
    cnt0 = _counters(lib, reset=True)
    _lib.check(lib.atspeed_gemm_packed(av.ptr, wv.ptr, cv.ptr, m, n, k, ld1, epi, wsv.ptr, WS_BYTES, _st()))
    cnt1 = _counters(lib)
    torch.cuda.synchronize()
    assert cnt0 == cnt1 and sum(cnt0[:13]) == 1, (cnt0, cnt1)
    ar.check()
    if epi == _lib.EPI_SWIGLU:
        _assert_packed_swiglu(lib, cv, ld1, c0, m, cols)
    else:
        guard.assert_same("c", cv.t, c0)


def _quant(lib, x):
    m, k = x.shape
    q = torch.empty(m, k, dtype=torch.uint8, device=DEV)
    s = torch.empty(m, dtype=torch.float32, device=DEV)
    _lib.check(lib.atspeed_quant_rows_fp8(x.data_ptr(), m, k, q.data_ptr(), s.data_ptr(), _st()))
    return q, s


def _fp8_operands(lib, m, n, k, seed):
    g = _gen(seed)
    xq, sx = _quant(lib, _randn((m, k), g, 1.5, torch.bfloat16))
    wq, sw = _quant(lib, _randn((n, k), g, 0.05, torch.bfloat16))
    return g, xq, sx, wq, sw


@pytest.mark.parametrize("m,n,k,epi,gap", [(901, 2752, 512, 3, 0), (901, 2752, 512, 3, 32), (121, 22016, 4096, 3, 32), (121, 4096, 4096, 2, 0), (1301, 1024, 1280, 0, 0),
                                          (33, 2304, 768, 1, 0)], ids=lambda v: str(v))
def test_gemm_fp8_packed_pad_rows(lib, m, n, k, epi, gap):
    """atspeed_gemm_fp8_packed with an odd m: the pad row of xq holds the e4m3 NaN, sx[m] the fp32 NaN; the packed SwiGLU output as in
    test_gemm_packed_pad_rows"""
    g, xq, sx, wq, sw = _fp8_operands(lib, m, n, k, m + n)
    xp, wp = _pack(lib, xq), _pack(lib, wq)
    cols, odt, ldc = _out_geometry(n, epi, torch.bfloat16)
    me = m + 1
    ws0 = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
    ar = Arena(DEV)
    xv, wv = _packed_input(ar, "xq", xp, m, "e4m3"), _packed_input(ar, "wq", wp, n, "e4m3")
    sxv, swv = ar.input("sx", sx), ar.input("sw", sw)
    wsv = ar.workspace("workspace", WS_BYTES)
    if epi == _lib.EPI_SWIGLU:
        c0 = torch.zeros(me, cols, dtype=odt, device=DEV)
        cv, ld1 = _packed_swiglu_out(ar, m, cols, gap, odt)
        ld0 = cols
    else:
        base = _randn((m, cols), g, 1.0, odt) if epi == _lib.EPI_RESID else None
        c0 = base.clone() if base is not None else torch.zeros(m, cols, dtype=odt, device=DEV)
        cv = ar.output("c", m, cols, odt, ld=ldc, init=base)
        ld0, ld1 = cols, ldc
    ar.snapshot()
    _counters(lib, reset=True)
    _lib.check(lib.atspeed_gemm_fp8_packed(xp.data_ptr(), sx.data_ptr(), wp.data_ptr(), sw.data_ptr(), c0.data_ptr(), m, n, k, ld0, epi, ws0.data_ptr(), WS_BYTES, _st()))
    cnt0 = _counters(lib, reset=True)
    _lib.check(lib.atspeed_gemm_fp8_packed(xv.ptr, sxv.ptr, wv.ptr, swv.ptr, cv.ptr, m, n, k, ld1, epi, wsv.ptr, WS_BYTES, _st()))
    cnt1 = _counters(lib)
    torch.cuda.synchronize()
    assert cnt0 == cnt1 and sum(cnt0[:13]) == 1, (cnt0, cnt1)
    ar.check()
    if epi == _lib.EPI_SWIGLU:
        _assert_packed_swiglu(lib, cv, ld1, c0, m, cols)
    else:
        guard.assert_same("c", cv.t, c0)


# ------------------------------------------------------------------ atspeed_gemm_fp8
FP8_FORMS = [
    ("fp8_ring", FP8_RING, (900, 2752, 512), (0, 1, 2, 3), False),                     # (no workspace: the plain grid)
    ("fp8_ring", FP8_RING, (1543, 1000, 256), (0, 1, 2), False),
    ("fp8_wstream", FP8_WDMA, (33, 2304, 768), (0, 1, 3), True),                       # (its residual epilogue always goes through slabs)
    ("fp8_wstream", FP8_WDMA, (77, 1000, 512), (0, 1), True),
    ("fp8_wstream_split", FP8_WDMA_SPLIT, (100, 4096, 4096), (0, 1, 2, 3), True),
    ("fp8_ring_kcut", FP8_RING_KCUT, (300, 4096, 4096), (0, 1, 2, 3), True),
]


@pytest.mark.parametrize("form,idx,m,n,k,epi,use_ws", [pytest.param(f, i, *s, e, u, id=f"{f}-{s[0]}x{s[1]}x{s[2]}-{EPI_NAME[e]}")
                                                       for f, i, s, es, u in FP8_FORMS for e in es])
def test_gemm_fp8_guard_bands(lib, form, idx, m, n, k, epi, use_ws):
    """atspeed_gemm_fp8: e4m3 NaN after row m of xq and row n of wq, NaN after sx[m - 1] and sw[n - 1], gapped ldc"""
    g, xq, sx, wq, sw = _fp8_operands(lib, m, n, k, m + n + epi)
    cols, odt, ldc = _out_geometry(n, epi, torch.bfloat16)
    base = _randn((m, cols), g, 1.0, odt) if epi == _lib.EPI_RESID else None
    c0 = base.clone() if base is not None else torch.zeros(m, cols, dtype=odt, device=DEV)
    nb = WS_BYTES if use_ws else 0
    ws0 = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
    ar = Arena(DEV, seed=epi)
    xv, wv = ar.input("xq", xq, kind="e4m3"), ar.input("wq", wq, kind="e4m3")
    sxv, swv = ar.input("sx", sx), ar.input("sw", sw)
    cv = ar.output("c", m, cols, odt, ld=ldc, init=base)
    wsv = ar.workspace("workspace", nb)
    ar.snapshot()
    _counters(lib, reset=True)
    _lib.check(lib.atspeed_gemm_fp8(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), c0.data_ptr(), m, n, k, cols, epi,
                                    ws0.data_ptr() if use_ws else None, nb, _st()))
    cnt0 = _counters(lib, reset=True)
    _lib.check(lib.atspeed_gemm_fp8(xv.ptr, sxv.ptr, wv.ptr, swv.ptr, cv.ptr, m, n, k, ldc, epi, wsv.ptr if use_ws else None, nb, _st()))
    cnt1 = _counters(lib)
    torch.cuda.synchronize()
    assert cnt0[idx] == 1 and sum(cnt0[:13]) == 1, (form, cnt0)
    assert cnt1 == cnt0
    ar.check()
    guard.assert_same("c", cv.t, c0)


def test_gemm_fp8_residual_without_room_for_slabs_is_refused_before_any_launch(lib):
    """atspeed_hip.h: epilogue 2, K % 256 != 0 and too little workspace -> ATSPEED_ERR_CAPACITY; nothing was written"""
    m, n, k = 100, 4096, 640
    g, xq, sx, wq, sw = _fp8_operands(lib, m, n, k, 5)
    ar = Arena(DEV)
    cv = ar.output("c", m, n, torch.bfloat16, ld=n + 40, init=_randn((m, n), g, 1.0, torch.bfloat16))
    wsv = ar.workspace("workspace", 4096)
    ar.snapshot()
    for ptr, nb in ((wsv.ptr, 4096), (None, 0)):
        rc = lib.atspeed_gemm_fp8(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), cv.ptr, m, n, k, cv.ld, 2, ptr, nb, _st())
        assert rc == _lib.ERR_CAPACITY
    torch.cuda.synchronize()
    ar.check()
    assert torch.equal(cv.buf, cv.saved) and torch.equal(wsv.buf, wsv.saved)


# ------------------------------------------------------------------ atspeed_gemm_w4a8
def _w4_operands(lib, m, n, k, seed):
    g = _gen(seed)
    xq, sx = _quant(lib, _randn((m, k), g, 1.5, torch.bfloat16))
    wq = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, device=DEV, generator=g)          # two e2m1 codes per byte
    sc = torch.randint(118, 124, (n, k // 32), dtype=torch.uint8, device=DEV, generator=g)       # scale bytes around 2^-6
    return g, xq, sx, wq, sc


def _w4_call(lib, xq, sx, wq, sc, c, m, n, k, ldc, epi, ws, nb):
    return lib.atspeed_gemm_w4a8(xq, sx, wq, sc, c, m, n, k, ldc, epi, _lib.ATSPEED_BF16, 0, ws, nb, _st())


@pytest.mark.parametrize("epi", [0, 1, 2, 3], ids=lambda e: EPI_NAME[e])
@pytest.mark.parametrize("m", [31, 33, 63, 65, 255, 257])
@pytest.mark.parametrize("k,split", [(4096, True), (512, False)], ids=["w4a8_split", "w4a8_unsplit"])
def test_gemm_w4a8_guard_bands(lib, k, split, m, epi):
    """atspeed_gemm_w4a8 at a size cut in K (fp32 slabs in the workspace) and one that is not, m on both sides of the 32 / 64 / 256-row
    tile heights: 0x77 nibbles and 0xFF scale bytes after weight row n, e4m3 NaN after row m of xq, NaN after sx[m - 1], gapped ldc"""
    n = 224
    g, xq, sx, wq, sc = _w4_operands(lib, m, n, k, m + k + epi)
    cols, odt, ldc = _out_geometry(n, epi, torch.bfloat16)
    base = _randn((m, cols), g, 1.0, odt) if epi == _lib.EPI_RESID else None
    c0 = base.clone() if base is not None else torch.zeros(m, cols, dtype=odt, device=DEV)
    nb = 16 << 20
    ws0 = torch.empty(nb, dtype=torch.uint8, device=DEV)
    ar = Arena(DEV, seed=epi)
    xv, sxv = ar.input("xq", xq, kind="e4m3"), ar.input("sx", sx)
    wv, scv = ar.input("wq", wq, kind="mxfp4"), ar.input("wscale", sc, kind="e8m0")
    cv = ar.output("c", m, cols, odt, ld=ldc, init=base)
    wsv = ar.workspace("workspace", nb)
    ar.snapshot()
    _counters(lib, reset=True)
    _lib.check(_w4_call(lib, xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sc.data_ptr(), c0.data_ptr(), m, n, k, cols, epi, ws0.data_ptr(), nb))
    _lib.check(_w4_call(lib, xv.ptr, sxv.ptr, wv.ptr, scv.ptr, cv.ptr, m, n, k, ldc, epi, wsv.ptr, nb))
    cnt = _counters(lib)
    torch.cuda.synchronize()
    assert cnt[W4A8] == 2 and sum(cnt[:13]) == 2, cnt
    assert bool((wsv.buf != wsv.saved).any()) == split, "this size was meant to run the other form"
    ar.check()
    guard.assert_same("c", cv.t, c0)


# ------------------------------------------------------------------ atspeed_lmhead_lse
@pytest.mark.parametrize("rows,vocab,hidden,fused", [(700, 32859, 512, 1), (90, 32859, 256, 0)], ids=["fused", "small_path"])
def test_lmhead_lse_guard_bands(lib, rows, vocab, hidden, fused):
    """atspeed_lmhead_lse, the fused path and the small one: weight rows >= vocab are NaN, the logit columns vocab .. ld - 1 (ld =
    roundup64(vocab)) and everything after workspace_bytes stay untouched, lse and the logits are the dense call's bits"""
    g = _gen(rows)
    x = _randn((rows, hidden), g, 1.0, torch.bfloat16)
    w = _randn((vocab, hidden), g, 0.08, torch.bfloat16)
    ld = _up(vocab, 64)
    nb = 64 << 20
    ws0 = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lg0 = torch.zeros(rows, ld, dtype=torch.float32, device=DEV)
    lse0 = torch.empty(rows, dtype=torch.float32, device=DEV)
    ar = Arena(DEV)
    xv, wv = ar.input("x", x), ar.input("w", w)
    lgv = ar.output("logits", rows, vocab, torch.float32, ld=ld)
    lsev = ar.output("lse", 1, rows, torch.float32)
    wsv = ar.workspace("workspace", nb)
    ar.snapshot()
    f0, f1 = C.c_int32(-1), C.c_int32(-1)
    _counters(lib, reset=True)
    _lib.check(lib.atspeed_lmhead_lse(x.data_ptr(), w.data_ptr(), lg0.data_ptr(), lse0.data_ptr(), rows, vocab, hidden, ld, None, ws0.data_ptr(), nb, C.byref(f0), _st()))
    cnt0 = _counters(lib, reset=True)
    _lib.check(lib.atspeed_lmhead_lse(xv.ptr, wv.ptr, lgv.ptr, lsev.ptr, rows, vocab, hidden, ld, None, wsv.ptr, nb, C.byref(f1), _st()))
    cnt1 = _counters(lib)
    torch.cuda.synchronize()
    assert f0.value == f1.value == fused and cnt0 == cnt1, (f0.value, f1.value, cnt0, cnt1)
    ar.check()
    guard.assert_same("lse", lsev.t, lse0.view(1, rows))
    guard.assert_same("logits", lgv.t, lg0[:, :vocab])
    assert not bool(torch.isnan(lse0).any())


# ------------------------------------------------------------------ workspace ladder
def _ref64(a, w):
    return a.double() @ w.double().T


def _fp8_float(q):
    return q.cpu().view(torch.float8_e4m3fn).to(torch.float64)


def _ladder_16(lib, m, n, k):
    g = _gen(m + n)
    a, w = _randn((m, k), g, 1.0, torch.bfloat16), _randn((n, k), g, 0.05, torch.bfloat16)
    ref = _ref64(a, w).cpu()
    tol = 1e-2 * float(ref.abs().max())                                   # test_gemm_store_and_f32, 16-bit store

    def call(c, ws, nb):
        return lib.atspeed_gemm(a.data_ptr(), w.data_ptr(), c.ptr, m, n, k, k, c.ld, _lib.ATSPEED_BF16, 0, ws, nb, _st())
    return call, ref, tol


def _ladder_fp8(lib, m, n, k):
    g, xq, sx, wq, sw = _fp8_operands(lib, m, n, k, m + n)
    ref = (_fp8_float(xq) @ _fp8_float(wq).T) * sx.cpu().double()[:, None] * sw.cpu().double()[None, :]
    tol = 2e-2 * float(ref.abs().max())                                   # test_gemm_fp8, 16-bit outputs

    def call(c, ws, nb):
        return lib.atspeed_gemm_fp8(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), c.ptr, m, n, k, c.ld, 0, ws, nb, _st())
    return call, ref, tol


def _ladder_w4(lib, m, n, k):
    g, xq, sx, wq, sc = _w4_operands(lib, m, n, k, m + n)
    q = wq.cpu().numpy()
    codes = np.stack((q & 15, q >> 4), -1).reshape(n, k)                  # low nibble = even element
    wd = torch.from_numpy(dequant_mxfp4(codes, sc.cpu().numpy()).astype(np.float64))
    xa = _fp8_float(xq)
    s = sx.cpu().double()[:, None]
    ref = (xa @ wd.T) * s
    bound = (xa.abs() @ wd.abs().T) * s
    tol = (k / 128 + 16) * 2.0 ** -24 * bound + 2.0 ** -8 * ref.abs() + 1e-30      # test_gemm_w4a8_matches_the_exact_product, bf16 store

    def call(c, ws, nb):
        return _w4_call(lib, xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sc.data_ptr(), c.ptr, m, n, k, c.ld, 0, ws, nb)
    return call, ref, tol


LADDER = [
    ("wstream_split", _ladder_16, WDMA_SPLIT, {}, (100, 12288, 1024)),
    ("ring_split", _ladder_16, RING_SPLIT, {}, (129, 8448, 256)),
    ("kcut", _ladder_16, RING_SPLIT, {}, (320, 4096, 4096)),
    ("panel_split", _ladder_16, PANEL_SPLIT, PANEL_SW, (320, 4096, 4096)),
    ("fp8_wstream_split", _ladder_fp8, FP8_WDMA_SPLIT, {}, (100, 4096, 4096)),
    ("fp8_ring_kcut", _ladder_fp8, FP8_RING_KCUT, {}, (300, 4096, 4096)),
    ("w4a8_split", _ladder_w4, None, {}, (65, 224, 4096)),
    ("tiled_split", _ladder_16, None, {}, (20, 4096, 768)),              # the LDS-tiled kernel's own split: no counter of its own either
]


@pytest.mark.parametrize("form,make,idx,sw,shape", LADDER, ids=[l[0] for l in LADDER])
def test_workspace_ladder(lib, form, make, idx, sw, shape):
    """workspace_bytes = 0, 1, 2, 4, 8, ... x (m n 4) up to the first size at which the split form runs and one step beyond, then once more
    with the largest size and a workspace pointer 8 bytes off 16-byte alignment.  At every step: the bytes from workspace_bytes on and
    around c are untouched, the result is within the form's existing fp64 tolerance whatever form ran, and WHERE the split form ran
    (the counters; W4A8 and the LDS-tiled kernel, whose counter covers both forms: the workspace was written) the slabs it left are
    inside workspace_bytes.  That last statement IS the guard on the bytes from workspace_bytes on (ar.check()): the slab count computed
    from the written extent below only reports it in slabs and cannot fail where that guard holds.  The planner is not restated: the
    test watches what ran."""
    m, n, k = shape
    slab = m * n * 4
    call, ref, tol = make(lib, m, n, k)
    seen, mult = None, 0
    while True:
        ar = Arena(DEV, seed=mult)
        cv = ar.output("c", m, n, torch.bfloat16, ld=_up(n, 8) + 40)
        nb = mult * slab
        wsv = ar.workspace("workspace", nb, halo_bytes=2 * slab)
        ar.snapshot()
        with _lib.switches(**sw):
            _counters(lib, reset=True)
            _lib.check(call(cv, wsv.ptr, nb))
            cnt = _counters(lib)
            torch.cuda.synchronize()
        _ladder_asserts(form, ar, cv, wsv, nb, slab, cnt, idx, ref, tol, mult)
        if seen is None and _ran_split(cnt, idx, wsv):
            seen = mult
        last = mult
        if seen is not None and mult > seen:
            break
        assert mult <= 512, f"{form}: no workspace size made the split form run"
        mult = 1 if mult == 0 else mult * 2
    assert seen is not None and seen >= 1
    # the workspace pointer 8 bytes off 16-byte alignment, at the largest size of the ladder
    ar = Arena(DEV, seed=999)
    cv = ar.output("c", m, n, torch.bfloat16, ld=_up(n, 8) + 40)
    nb = last * slab
    wsv = ar.workspace("workspace", nb, align_mod=24, halo_bytes=2 * slab)
    assert wsv.ptr % 16 == 8
    ar.snapshot()
    with _lib.switches(**sw):
        _counters(lib, reset=True)
        _lib.check(call(cv, wsv.ptr, nb))
        cnt = _counters(lib)
        torch.cuda.synchronize()
    _ladder_asserts(form + " (workspace 8 bytes off 16)", ar, cv, wsv, nb, slab, cnt, idx, ref, tol, last)


def _ran_split(cnt, idx, wsv):
    return bool((wsv.buf != wsv.saved).any()) if idx is None else cnt[idx] == 1


def _ladder_asserts(form, ar, cv, wsv, nb, slab, cnt, idx, ref, tol, mult):
    ar.check()
    err = (cv.t.double().cpu() - ref).abs()
    assert bool((err <= tol).all()), (form, mult, float(err.max()), cnt)
    if _ran_split(cnt, idx, wsv):
        changed = (wsv.buf != wsv.saved).nonzero()
        assert changed.numel(), (form, "a split form that left nothing in the workspace", cnt)
        extent = int(changed[-1]) - wsv.off + 1
        parts = (extent + slab - 1) // slab
        assert parts >= 1 and parts * slab <= nb, (form, mult, parts, nb)


# ------------------------------------------------------------------ tree attention
def _attn_inputs(T, S, heads, dh, dtype, seed, max_slots):
    from atspeed_amd.model import vis_bits_from_bool
    g = _gen(seed)
    H = heads * dh
    q = _randn((T, 3 * H), g, 1.0, dtype)
    kc = _randn((S, H), g, 1.0, dtype)
    vc = _randn((S, H), g, 1.0, dtype)
    vis = torch.rand(T, S, generator=torch.Generator().manual_seed(seed)) < 0.25
    vis[:, 0] = True
    if S > 100:
        vis[5] = False; vis[5, S - 1] = True
        vis[T - 1, : S - 3] = False; vis[T - 1, S - 3:] = True
    bits = vis_bits_from_bool(vis, max_slots).to(DEV)
    return q, kc, vc, vis, bits


def _attn_pair(lib, T, S, heads, dh, dtype, qtile, rpw):
    max_slots = 512
    H = heads * dh
    q, kc, vc, _, bits = _attn_inputs(T, S, heads, dh, dtype, T + S, max_slots)
    code = _lib.dtype_code(dtype)
    # dense: full-size caches whose slots >= S hold finite random data, as in test_kernels_gpu.py
    g = _gen(1)
    kd = torch.cat((kc, _randn((max_slots - S, H), g, 1.0, dtype)))
    vd = torch.cat((vc, _randn((max_slots - S, H), g, 1.0, dtype)))
    out0 = torch.zeros(T, H, dtype=dtype, device=DEV)
    ar = Arena(DEV)
    qv = ar.input("q", q, ld=3 * H + 40)
    kv, vv = ar.input("kcache", kc), ar.input("vcache", vc)              # S rows: slot S and everything after it is NaN
    bv = ar.input("vis_bits", bits)
    ov = ar.output("out", T, H, dtype)
    ar.snapshot()

    def call(qp, ldq, kp, vp, bp, op):
        if qtile is None:
            return lib.atspeed_tree_attention(qp, ldq, kp, vp, bp, max_slots // 64, op, T, S, heads, dh, code, _st())
        return lib.atspeed_tree_attention_tiled(qp, ldq, kp, vp, bp, max_slots // 64, op, T, S, heads, dh, code, qtile, rpw, _st())
    _lib.check(call(q.data_ptr(), 3 * H, kd.data_ptr(), vd.data_ptr(), bits.data_ptr(), out0.data_ptr()))
    _lib.check(call(qv.ptr, qv.ld, kv.ptr, vv.ptr, bv.ptr, ov.ptr))
    torch.cuda.synchronize()
    ar.check()
    guard.assert_same("out", ov.t, out0)
    assert not bool(torch.isnan(out0.float()).any())


@pytest.mark.parametrize("rpw", [16, 32])
@pytest.mark.parametrize("qtile", [64, 128, 256])
@pytest.mark.parametrize("heads,dh,T,S", [(12, 64, 200, 330), (8, 128, 37, 64), (32, 128, 300, 470)], ids=["12x64-T200-S330", "8x128-T37-S64", "32x128-T300-S470"])
def test_tree_attention_mfma_guard_bands(lib, heads, dh, T, S, qtile, rpw):
    """the MFMA kernels at every query-tile height and both rows_per_wave, T ragged against 64 / 128 / 256: ldq = 3 H + 40 with NaN in
    the gap and after row T, cache slots >= n_slots NaN, out in an arena"""
    _attn_pair(lib, T, S, heads, dh, torch.bfloat16, qtile, rpw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: DT_NAME[d])
@pytest.mark.parametrize("T", [23, 150])
def test_tree_attention_scalar_guard_bands(lib, dtype, T):
    """head_dim 32: the scalar kernel in all three types, through atspeed_tree_attention's own choice"""
    _attn_pair(lib, T, 150, 4, 32, dtype, None, None)


@pytest.mark.parametrize("qtile,rpw", [(None, None), (64, 16), (128, 32), (256, 16), (256, 32)], ids=["auto", "64x16", "128x32", "256x16", "256x32"])
@pytest.mark.parametrize("dtype,heads,dh", [(torch.bfloat16, 12, 64), (torch.float32, 4, 32), (torch.float16, 4, 32)], ids=["bf16_mfma", "fp32_scalar", "fp16_scalar"])
def test_tree_attention_invisible_slots_below_n_slots_are_never_seen(lib, dtype, heads, dh, qtile, rpw):
    """slots below n_slots that no row sees, filled with the type's largest finite value (K and V), change no output bit against the
    same slots filled with zeros.  (Non-finite values there are NOT required to be harmless: atspeed_hip.h, atspeed_tree_attention.)"""
    if qtile is not None and dtype != torch.bfloat16:
        qtile, rpw = None, None                                           # (the scalar kernel takes no tiling)
    T, S, max_slots = 200, 330, 512
    H = heads * dh
    q, kc, vc, vis, _ = _attn_inputs(T, S, heads, dh, dtype, 77, max_slots)
    from atspeed_amd.model import vis_bits_from_bool
    hidden = torch.zeros(S, dtype=torch.bool)
    hidden[torch.tensor([1, 63, 64, 100, 255, 256, S - 2])] = True       # tile edges and interior
    vis[:, hidden] = False
    bits = vis_bits_from_bool(vis, max_slots).to(DEV)
    code = _lib.dtype_code(dtype)
    outs = []
    for fill in (0.0, float(torch.finfo(dtype).max)):
        k2, v2 = kc.clone(), vc.clone()
        k2[hidden.to(DEV)] = fill; v2[hidden.to(DEV)] = fill
        kd = torch.cat((k2, torch.zeros(max_slots - S, H, dtype=dtype, device=DEV)))
        vd = torch.cat((v2, torch.zeros(max_slots - S, H, dtype=dtype, device=DEV)))
        out = torch.zeros(T, H, dtype=dtype, device=DEV)
        if qtile is None:
            _lib.check(lib.atspeed_tree_attention(q.data_ptr(), 3 * H, kd.data_ptr(), vd.data_ptr(), bits.data_ptr(), max_slots // 64, out.data_ptr(), T, S, heads, dh, code, _st()))
        else:
            _lib.check(lib.atspeed_tree_attention_tiled(q.data_ptr(), 3 * H, kd.data_ptr(), vd.data_ptr(), bits.data_ptr(), max_slots // 64, out.data_ptr(), T, S, heads, dh,
                                                        code, qtile, rpw, _st()))
        torch.cuda.synchronize()
        outs.append(out)
    guard.assert_same("out", outs[1], outs[0])
    assert not bool(torch.isnan(outs[0].float()).any())


# ------------------------------------------------------------------ row kernels
def _pair(ar_outs, dense_outs):
    for v, d in zip(ar_outs, dense_outs):
        guard.assert_same(v.name, v.t, d.reshape(v.rows, v.cols))


@pytest.mark.parametrize("hidden", [100, 11008])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: DT_NAME[d])
def test_rmsnorm_guard_bands(lib, dtype, hidden):
    rows = 37
    g = _gen(hidden)
    x, w = _randn((rows, hidden), g, 2.0, dtype), (1 + _randn((hidden,), g, 0.1)).to(dtype)
    y0 = torch.empty_like(x)
    ar = Arena(DEV)
    xv, wv, yv = ar.input("x", x), ar.input("w", w), ar.output("y", rows, hidden, dtype)
    ar.snapshot()
    code = _lib.dtype_code(dtype)
    _lib.check(lib.atspeed_rmsnorm(x.data_ptr(), w.data_ptr(), y0.data_ptr(), rows, hidden, 1e-6, code, _st()))
    _lib.check(lib.atspeed_rmsnorm(xv.ptr, wv.ptr, yv.ptr, rows, hidden, 1e-6, code, _st()))
    torch.cuda.synchronize()
    ar.check()
    _pair([yv], [y0])


@pytest.mark.parametrize("with_y", [True, False], ids=["y", "y_null"])
@pytest.mark.parametrize("hidden", [768, 4096, 8192])
def test_rmsnorm_quant_fp8_guard_bands(lib, hidden, with_y):
    rows = 37
    g = _gen(hidden)
    x, w = _randn((rows, hidden), g, 2.0, torch.bfloat16), (1 + _randn((hidden,), g, 0.1)).to(torch.bfloat16)
    y0 = torch.empty_like(x); q0 = torch.empty(rows, hidden, dtype=torch.uint8, device=DEV); s0 = torch.empty(rows, device=DEV)
    ar = Arena(DEV)
    xv, wv = ar.input("x", x), ar.input("w", w)
    yv = ar.output("y", rows, hidden, torch.bfloat16)
    qv, sv = ar.output("q", rows, hidden, torch.uint8), ar.output("scale", 1, rows, torch.float32)
    ar.snapshot()
    _lib.check(lib.atspeed_rmsnorm_quant_fp8(x.data_ptr(), w.data_ptr(), y0.data_ptr(), q0.data_ptr(), s0.data_ptr(), rows, hidden, 1e-6, _st()))
    _lib.check(lib.atspeed_rmsnorm_quant_fp8(xv.ptr, wv.ptr, yv.ptr if with_y else None, qv.ptr, sv.ptr, rows, hidden, 1e-6, _st()))
    torch.cuda.synchronize()
    ar.check()
    _pair([qv, sv], [q0, s0])
    if with_y:
        _pair([yv], [y0])
    else:
        assert torch.equal(yv.buf, yv.saved)


@pytest.mark.parametrize("rows,cols", [(37, 1152), (9, 12352), (51, 11008)])
def test_quant_rows_fp8_and_packed_guard_bands(lib, rows, cols):
    """atspeed_quant_rows_fp8 and _packed (odd rows; 12352 columns: the one-row fallback): the packed input's pad row is NaN, the packed
    output's pad row and scale[rows] are guard bytes"""
    g = _gen(rows + cols)
    x = _randn((rows, cols), g, 3.0, torch.bfloat16)
    q0, s0 = _quant(lib, x)
    ar = Arena(DEV)
    xv = ar.input("x", x)
    qv, sv = ar.output("q", rows, cols, torch.uint8), ar.output("scale", 1, rows, torch.float32)
    xp = _pack(lib, x)
    re = xp.shape[0]
    xpv = _packed_input(ar, "x_packed", xp, rows)
    qpv = ar.output("q_packed", re, cols, torch.uint8)
    qpv.add_guard(guard.packed_row_offsets(rows, cols))
    spv = ar.output("scale_packed", 1, rows, torch.float32)
    ar.snapshot()
    _lib.check(lib.atspeed_quant_rows_fp8(xv.ptr, rows, cols, qv.ptr, sv.ptr, _st()))
    _lib.check(lib.atspeed_quant_rows_fp8_packed(xpv.ptr, rows, cols, qpv.ptr, spv.ptr, _st()))
    torch.cuda.synchronize()
    ar.check()
    _pair([qv, sv, spv], [q0, s0, s0])
    q1 = torch.empty(rows, cols, dtype=torch.uint8, device=DEV)
    _lib.check(lib.atspeed_unpack_rows(qpv.ptr, q1.data_ptr(), rows, cols, _st()))
    torch.cuda.synchronize()
    guard.assert_same("q_packed", q1, q0)


@pytest.mark.parametrize("rows,cols,dt", [(7, 96, torch.bfloat16), (33, 256, torch.uint8), (63, 4096, torch.bfloat16)])
def test_pack_and_unpack_rows_guard_bands(lib, rows, cols, dt):
    """atspeed_pack_rows writes the even-rounded destination (the pad row: zeros, as the header says) and nothing else; atspeed_unpack_rows
    reads no pad row (NaN) and writes `rows` rows"""
    src = (torch.arange(rows * cols, dtype=torch.int32, device=DEV) % 251).reshape(rows, cols).to(dt)
    rb = cols * src.element_size()
    re = (rows + 1) // 2 * 2
    ar = Arena(DEV)
    sv = ar.input("src", src, kind="bf16" if dt == torch.bfloat16 else "e4m3")
    pv = ar.output("packed", re, cols, dt)
    ar.snapshot()
    _lib.check(lib.atspeed_pack_rows(sv.ptr, pv.ptr, rows, rb, _st()))
    torch.cuda.synchronize()
    ar.check()
    guard.assert_same("packed", pv.t, _pack(lib, src))
    pad = pv.payload_bytes()[guard.packed_row_offsets(rows, rb).to(DEV)]
    assert not bool(pad.any()), "the pad row of an odd row count is zeroed"
    ar2 = Arena(DEV)
    pin = _packed_input(ar2, "packed", pv.t.clone(), rows, "bf16" if dt == torch.bfloat16 else "e4m3")
    uv = ar2.output("unpacked", rows, cols, dt)
    ar2.snapshot()
    _lib.check(lib.atspeed_unpack_rows(pin.ptr, uv.ptr, rows, rb, _st()))
    torch.cuda.synchronize()
    ar2.check()
    guard.assert_same("unpacked", uv.t, src)


@pytest.mark.parametrize("rows,V", [(1, 32859), (40, 33014), (3, 1000), (2, 7)])
def test_lse_log_softmax_guard_bands(lib, rows, V):
    """atspeed_lse_rows / atspeed_log_softmax_rows: the padding columns V .. ld - 1 of the logits are NaN (a finite padding value hides
    under a max), the log-softmax output has gapped rows"""
    ld = _up(V, 64)
    g = _gen(V)
    x = _randn((rows, V), g, 3.0)
    x[0, 5] = 40.0
    dense = torch.zeros(rows, ld, device=DEV); dense[:, :V] = x
    lse0 = torch.empty(rows, device=DEV); ls0 = torch.empty(rows, V, device=DEV)
    _lib.check(lib.atspeed_lse_rows(dense.data_ptr(), rows, V, ld, lse0.data_ptr(), _st()))
    _lib.check(lib.atspeed_log_softmax_rows(dense.data_ptr(), ld, lse0.data_ptr(), rows, V, ls0.data_ptr(), V, _st()))
    ar = Arena(DEV)
    xv = ar.input("logits", x, ld=ld)
    lv = ar.output("lse", 1, rows, torch.float32)
    ov = ar.output("log_softmax", rows, V, torch.float32, ld=_up(V, 4) + 20)
    ar.snapshot()
    _lib.check(lib.atspeed_lse_rows(xv.ptr, rows, V, ld, lv.ptr, _st()))
    _lib.check(lib.atspeed_log_softmax_rows(xv.ptr, ld, lv.ptr, rows, V, ov.ptr, ov.ld, _st()))
    torch.cuda.synchronize()
    ar.check()
    _pair([lv, ov], [lse0, ls0])
    ref = torch.logsumexp(x.double(), -1)
    np.testing.assert_allclose(lse0.double().cpu().numpy(), ref.cpu().numpy(), atol=2e-6 * float(ref.abs().max()) + 1e-6, rtol=0)


@pytest.mark.parametrize("rows,vocab,k", [(1, 32859, 20), (40, 32859, 40), (7, 300, 5), (3, 16384 + 5, 1)])
def test_row_topk_and_free_expand_guard_bands(lib, rows, vocab, k):
    """atspeed_row_topk and atspeed_beam_expand_prune_free with k < ATSPEED_MAX_BEAMS: NaN padding columns, the k-entry outputs' tails and
    the candidate scratch's surroundings are guard bytes"""
    ld = _up(vocab, 64)
    MB = _lib.MAX_BEAMS
    g = _gen(rows + vocab)
    logits = _randn((rows, vocab), g, 3.0)
    logits[0, : min(vocab, 50)] = float("-inf")
    beam = -torch.rand(rows, generator=g, device=DEV) * 5
    lse = torch.logsumexp(logits.double(), -1).float()
    dense = torch.full((rows, ld), 7.0, device=DEV); dense[:, :vocab] = logits
    tk0 = torch.empty(rows, MB, dtype=torch.int32, device=DEV)
    ws0 = torch.empty(rows * MB, dtype=torch.int32, device=DEV)
    o0 = [torch.empty(k, dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.int32, torch.int32)]
    _lib.check(lib.atspeed_row_topk(dense.data_ptr(), rows, vocab, ld, k, tk0.data_ptr(), _st()))
    _lib.check(lib.atspeed_beam_expand_prune_free(dense.data_ptr(), ld, lse.data_ptr(), beam.data_ptr(), rows, vocab, k, ws0.data_ptr(), *[o.data_ptr() for o in o0], _st()))
    ar = Arena(DEV)
    xv, lv, bv = ar.input("logits", logits, ld=ld), ar.input("lse", lse), ar.input("beam_score", beam)
    tkv = ar.output("row_topk", rows, MB, torch.int32)
    wsv = ar.output("row_cand_ws", rows, MB, torch.int32)
    ov = [ar.output(nm, 1, k, dt) for nm, dt in (("out_score", torch.float32), ("out_parent", torch.int32), ("out_token", torch.int32), ("out_flat", torch.int32))]
    ar.snapshot()
    _lib.check(lib.atspeed_row_topk(xv.ptr, rows, vocab, ld, k, tkv.ptr, _st()))
    _lib.check(lib.atspeed_beam_expand_prune_free(xv.ptr, ld, lv.ptr, bv.ptr, rows, vocab, k, wsv.ptr, *[o.ptr for o in ov], _st()))
    torch.cuda.synchronize()
    ar.check()
    _pair([tkv] + ov, [tk0] + o0)


@pytest.mark.parametrize("rows,k", [(20, 20), (40, 7), (1, 1)])
def test_beam_expand_prune_guard_bands(lib, rows, k):
    """atspeed_beam_expand_prune over a two-node automaton, k < ATSPEED_MAX_BEAMS: NaN padding columns and NaN after lse / beam_score /
    beam_node's last entry, the five k-entry outputs' tails are guard bytes"""
    V = 32859
    ld = _up(V, 64)
    g = _gen(rows * 64 + k)
    toks = sorted(set(torch.randint(0, V, (300,), generator=torch.Generator().manual_seed(k)).tolist()) | {0, V - 1})
    row_ptr = np.array([0, len(toks), len(toks)], np.int32); tok = np.array(toks, np.int32); nxt = np.ones(len(toks), np.int32)
    fsm = C.c_void_p()
    _lib.check(lib.atspeed_fsm_create(row_ptr.ctypes.data, tok.ctypes.data, nxt.ctypes.data, 2, len(toks), V, C.byref(fsm)))
    try:
        logits = _randn((rows, V), g, 2.5)
        beam = -torch.rand(rows, generator=g, device=DEV) * 5
        node = torch.zeros(rows, dtype=torch.int32, device=DEV)
        lse = torch.logsumexp(logits.double(), -1).float()
        dense = torch.zeros(rows, ld, device=DEV); dense[:, :V] = logits
        dts = (torch.float32, torch.int32, torch.int32, torch.int32, torch.int32)
        o0 = [torch.empty(k, dtype=dt, device=DEV) for dt in dts]
        _lib.check(lib.atspeed_beam_expand_prune(dense.data_ptr(), ld, lse.data_ptr(), beam.data_ptr(), node.data_ptr(), rows, fsm, k, *[o.data_ptr() for o in o0], _st()))
        ar = Arena(DEV)
        xv, lv, bv, nv = ar.input("logits", logits, ld=ld), ar.input("lse", lse), ar.input("beam_score", beam), ar.input("beam_node", node)
        ov = [ar.output(nm, 1, k, dt) for nm, dt in zip(("out_score", "out_parent", "out_token", "out_node", "out_flat"), dts)]
        ar.snapshot()
        _lib.check(lib.atspeed_beam_expand_prune(xv.ptr, ld, lv.ptr, bv.ptr, nv.ptr, rows, fsm, k, *[o.ptr for o in ov], _st()))
        torch.cuda.synchronize()
        ar.check()
        _pair(ov, o0)
        assert int(o0[4][0]) >= 0
    finally:
        lib.atspeed_fsm_destroy(fsm)


@pytest.mark.parametrize("packed", [0, 1], ids=["row_major", "packed"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: DT_NAME[d])
def test_quant_weights_mxfp4_guard_bands(lib, dtype, packed):
    """atspeed_quant_weights_mxfp4 with an odd row count in both layouts: NaN after the last row (packed: in the pad row), exactly
    rows x k / 2 nibble bytes and rows x k / 32 scale bytes written"""
    rows, k = 37, 512
    g = _gen(rows + packed)
    w = _randn((rows, k), g, 0.05, dtype)
    src = _pack(lib, w) if packed else w
    q0 = torch.empty(rows, k // 2, dtype=torch.uint8, device=DEV); s0 = torch.empty(rows, k // 32, dtype=torch.uint8, device=DEV)
    code = _lib.dtype_code(dtype)
    _lib.check(lib.atspeed_quant_weights_mxfp4(src.data_ptr(), rows, k, code, packed, q0.data_ptr(), s0.data_ptr(), _st()))
    ar = Arena(DEV)
    wv = _packed_input(ar, "w", src, rows) if packed else ar.input("w", src)
    qv, sv = ar.output("q", rows, k // 2, torch.uint8), ar.output("scales", rows, k // 32, torch.uint8)
    ar.snapshot()
    _lib.check(lib.atspeed_quant_weights_mxfp4(wv.ptr, rows, k, code, packed, qv.ptr, sv.ptr, _st()))
    torch.cuda.synchronize()
    ar.check()
    _pair([qv, sv], [q0, s0])


def test_assemble_sequences_guard_bands(lib):
    n, k, L = 9, 20, 4
    g = torch.Generator().manual_seed(3)
    lens = [int(x) for x in torch.randint(1, 200, (n,), generator=g)]
    prompts = torch.cat([torch.randint(0, 32000, (p,), generator=g, dtype=torch.int32) for p in lens]).to(DEV)
    toks = torch.randint(32000, 32859, (n * k * L,), generator=g, dtype=torch.int32).to(DEV)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = k * (int(off[-1]) + n * L)
    r0 = torch.full((total,), -1, dtype=torch.int64, device=DEV)
    _lib.check(lib.atspeed_assemble_sequences(prompts.data_ptr(), off.ctypes.data, toks.data_ptr(), n, k, L, r0.data_ptr(), _st()))
    ar = Arena(DEV)
    pv, tv = ar.input("prompts", prompts), ar.input("toks", toks)
    ov = ar.output("out", 1, total, torch.int64)
    ar.snapshot()
    _lib.check(lib.atspeed_assemble_sequences(pv.ptr, off.ctypes.data, tv.ptr, n, k, L, ov.ptr, _st()))
    torch.cuda.synchronize()
    ar.check()
    _pair([ov], [r0])
    assert int(r0.min()) >= 0
