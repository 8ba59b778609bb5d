"""Every GEMM form at the edges of its dispatch, bit for bit on placed operands (tests/gemm_cases.py; proved on the CPU by
tests/test_gemm_cases_cpu.py).  One case per (table row, epilogue, format): each of its launches -- the weight selector until its k have
covered [0, K), then the activation selector until it has taken every target -- builds the operands on the device, resets
atspeed_gemm_path_counters, calls atspeed_gemm / atspeed_gemm_fp8 / atspeed_gemm_w4a8 with the 64 MB workspace the other GEMM tests use (or
none, where the row says so), asserts that exactly the row's counter reads 1, and hands the output to gemm_cases.judge: F32, STORE and RESID
bit for bit, SWIGLU under rounding.assert_rounded at rounding.REL / rounding.CAP (16 bit) or within REL relative (fp32 engine).  A failure
names the first wrong element, the k its product comes from, the k-step, ring stage, k-tile, unit and 16-byte chunk that k lies in, and the
bits got and expected.  The output buffer starts as a poison value, so an element never written fails like a wrong one.  The gathers of the
expected values (integer hashes, exact products of values of at most 11 bits) run on the device too; tests/rounding.py rounds them in numpy.
Run with -m gpu on the MI355X box."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib
from tests import gemm_cases as GC

CASES = GC.cases()
POISON = 7.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


@pytest.fixture(scope="module")
def work():
    return torch.empty(64 << 20, dtype=torch.uint8, device="cuda")


def _counters(lib, reset=False):
    out = (C.c_int64 * 16)()
    lib.atspeed_gemm_path_counters(out, 16, 1 if reset else 0)
    return list(out)[: GC.N_COUNTERS]


def _launch(lib, L, work):
    """one launch of the case: the output as a float64 numpy array, and the launch counters it left"""
    ops = L.operands("cuda")
    m, n, k, epi = L.m, L.n, L.k, L.epi
    td = GC.TORCH[L.dt]
    if epi == GC.RESID:
        c = torch.from_numpy(L.resid()).to(td).cuda()
    else:
        c = torch.full((m, n // 2 if epi == GC.SWIGLU else n), POISON, dtype=torch.float32 if epi == GC.F32 else td, device="cuda")
    ldc = c.stride(0)
    wp, wb = (work.data_ptr(), work.numel()) if L.row.ws else (None, 0)
    st = _lib.stream_ptr()
    _counters(lib, reset=True)
    if L.fam in ("g16", "f32"):
        rc = lib.atspeed_gemm(ops["a"].data_ptr(), ops["w"].data_ptr(), c.data_ptr(), m, n, k, k, ldc, _lib.dtype_code(td), epi, wp, wb, st)
    elif L.fam == "w8a8":
        rc = lib.atspeed_gemm_fp8(ops["a"].data_ptr(), ops["sx"].data_ptr(), ops["w"].data_ptr(), ops["sw"].data_ptr(), c.data_ptr(), m, n, k, ldc, epi, wp, wb, st)
    else:
        rc = lib.atspeed_gemm_w4a8(ops["a"].data_ptr(), ops["sx"].data_ptr(), ops["w"].data_ptr(), ops["wsc"].data_ptr(), c.data_ptr(), m, n, k, ldc, epi,
                                   _lib.dtype_code(td), 0, wp, wb, st)
    _lib.check(rc)
    torch.cuda.synchronize()
    return c.double().cpu().numpy(), _counters(lib)


@pytest.mark.parametrize("row,epi,dt", CASES, ids=[GC.case_id(*c) for c in CASES])
def test_placed_operands_bit_for_bit(lib, work, row, epi, dt):
    want = [int(i == row.counter) for i in range(GC.N_COUNTERS)]
    with _lib.switches(**{**GC.DEFAULT_SWITCHES, **dict(row.sw)}):
        for L in GC.launches(row, epi, dt):
            L.dev = "cuda"
            got, cnt = _launch(lib, L, work)
            assert cnt == want, f"{L.name}: launch counters {cnt}, expected counter {row.counter} alone ({row.why})"
            GC.judge(L, got)


def test_the_device_builds_the_operands_and_gathers_of_the_cpu():
    """the hashes are integer arithmetic and the products exact: one small launch of every family built on both devices"""
    for form, epi, dt in (("tiled", GC.RESID, "fp16"), ("tiled32", GC.STORE, "fp32"), ("fp8_wdma_split", GC.SWIGLU, "bf16"), ("fp4", GC.STORE, "bf16")):
        row = min((r for r in GC.TABLE if r.form == form and r.m >= 16), key=lambda r: r.m * r.n * r.k)
        for sel in "WA":
            a, b = GC.Launch(row, epi, dt, sel, 0, "b"), GC.Launch(row, epi, dt, sel, 0, "b")
            b.dev = "cuda"
            assert np.array_equal(a.exact(), b.exact()) and (epi != GC.RESID or np.array_equal(a.resid(), b.resid()))
            oa, ob = a.operands("cpu"), b.operands("cuda")
            for key in oa:
                assert torch.equal(oa[key], ob[key].cpu()), (form, sel, key)
