"""The 4-bit target without a GPU: the numpy restatement of the MXFP4 rule (tests/mxfp4_ref.py) on its corner cases, the C ABI of the new
calls (declared and exported), and the CLI's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from atspeed_amd import _lib
from tests.mxfp4_ref import E2M1, dequant_mxfp4, e2m1_codes, pack_nibbles, quant_mxfp4, unpack_nibbles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP4_ABI = ("atspeed_llama_enable_fp4", "atspeed_llama_fp4_counters", "atspeed_quant_weights_mxfp4", "atspeed_gemm_w4a8")


def _block(vals, fill=0.0):
    b = np.full(32, fill, dtype=np.float32)
    b[: len(vals)] = vals
    return b[None, :]


def test_ties_go_to_the_even_mantissa():
    # amax 6 -> X = floor(log2 6) - 2 = 0: scale 1, the values are the grid itself
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for sign in (1.0, -1.0):
        codes, sb = quant_mxfp4(_block([6.0] + [sign * t for t in ties]))
        assert sb[0, 0] == 127
        got = dequant_mxfp4(codes, sb)[0, 1:8]
        assert got.tolist() == [sign * w if w else 0.0 for w in want]
    assert e2m1_codes(np.array([0.25, -0.25], np.float32)).tolist() == [0, 0]     # rounds to zero: +0, no sign bit
    # just off the ties: nearest
    codes, sb = quant_mxfp4(_block([6.0, 0.26, 0.74, 1.26, 1.74, 2.51, 3.49, 5.01]))
    assert dequant_mxfp4(codes, sb)[0, 1:8].tolist() == [0.5, 0.5, 1.5, 1.5, 3.0, 3.0, 6.0]


def test_saturation_at_six():
    codes, sb = quant_mxfp4(_block([7.9, -7.5, 5.5]))
    assert sb[0, 0] == 127                                     # floor(log2 7.9) = 2
    assert dequant_mxfp4(codes, sb)[0, :3].tolist() == [6.0, -6.0, 6.0]
    assert codes[0, 0] == 7 and codes[0, 1] == 15


def test_zero_blocks_get_byte_zero_and_zero_elements():
    w = np.zeros((3, 64), np.float32)
    w[1, 40] = 3.0                                             # block 1 of row 1 is not zero
    codes, sb = quant_mxfp4(w)
    assert sb[0].tolist() == [0, 0] and sb[2].tolist() == [0, 0] and sb[1].tolist() == [0, 126]     # floor(log2 3) - 2 = -1
    assert not codes[0].any() and not codes[2].any() and not codes[1, :32].any()
    w = np.full((1, 32), -0.0, np.float32)
    codes, sb = quant_mxfp4(w)
    assert sb[0, 0] == 0 and not codes.any()


def test_blocks_whose_amax_is_an_exact_power_of_two():
    for p in (-20, -3, 0, 1, 7):
        amax = 2.0 ** p
        codes, sb = quant_mxfp4(_block([amax, -amax / 2, amax / 8]))
        assert sb[0, 0] == 127 + p - 2                         # amax / 2^X = 4 exactly
        assert codes[0, 0] == 6 and codes[0, 1] == 8 | 4 and codes[0, 2] == 1
        assert dequant_mxfp4(codes, sb)[0, :3].tolist() == [amax, -amax / 2, amax / 8]
    codes, sb = quant_mxfp4(_block([2.0 ** -140]))            # X clamps at -127
    assert sb[0, 0] == 0 and codes[0, 0] == e2m1_codes(np.array([np.ldexp(2.0 ** -140, 127)], np.float32))[0]


def test_representable_values_round_trip():
    rng = np.random.default_rng(3)
    for X in (-9, -1, 0, 4):
        grid = np.concatenate((E2M1, -E2M1[1:]))
        vals = rng.choice(grid, size=(5, 96)).astype(np.float32)
        vals[:, ::32] = 6.0                                    # every block's amax is 6: X comes back as given
        w = np.ldexp(vals, X).astype(np.float32)
        codes, sb = quant_mxfp4(w)
        assert (sb == 127 + X).all()
        np.testing.assert_array_equal(dequant_mxfp4(codes, sb), w)
        np.testing.assert_array_equal(unpack_nibbles(pack_nibbles(codes)), codes)
    assert pack_nibbles(np.array([[1, 2, 15, 0]], np.uint8)).tolist() == [[0x21, 0x0F]]     # low nibble = even k


def _declared():
    text = open(os.path.join(ROOT, "include", "atspeed_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(atspeed_[a-z0-9_]+)\s*\(", text))


def test_fp4_abi_is_declared_bound_and_exported():
    names = _declared()
    assert all(n in names for n in FP4_ABI), sorted(set(FP4_ABI) - names)
    assert all(n in _lib.SIGNATURES for n in FP4_ABI)
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in FP4_ABI)
    loaded = _lib.load()
    assert b"0.2" in loaded.atspeed_version()
    # host-side refusals need no device: null arguments
    assert loaded.atspeed_llama_enable_fp4(None, None) == _lib.ERR_INVALID
    assert loaded.atspeed_llama_fp4_counters(None, None, None, 0) == _lib.ERR_INVALID
    assert loaded.atspeed_gemm_w4a8(None, None, None, None, None, 1, 64, 256, 64, 0, _lib.ATSPEED_BF16, 0, None, 0, None) == _lib.ERR_INVALID
    assert loaded.atspeed_quant_weights_mxfp4(None, 1, 256, _lib.ATSPEED_F32, 0, None, None, None) == _lib.ERR_INVALID


def test_cli_refuses_fp4_with_fp32_and_with_fp8():
    from atspeed_amd.inference import parse
    base = ["--data_path", "unused"]
    assert parse(base + ["--target_fp4"]).target_fp4
    assert parse(base + ["--target_fp4", "--dtype", "fp16"]).target_fp4
    assert not parse(base).target_fp4
    with pytest.raises(SystemExit):
        parse(base + ["--target_fp4", "--dtype", "fp32"])
    with pytest.raises(SystemExit):
        parse(base + ["--target_fp4", "--target_fp8"])
