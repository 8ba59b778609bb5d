"""Test helper: a numpy restatement of the 4-bit target's weight format (OCP MXFP4, atspeed_llama_enable_fp4; INTEGRATION.md "4-bit target")
and a W4A8 `RefLlama`.

Each row of K is cut into blocks of 32 consecutive k.  A block's scale byte is 127 + X, X = clamp(floor(log2(amax)) - 2, -127, 127); its
elements are e2m1(v / 2^X) rounded to nearest on {0, .5, 1, 1.5, 2, 3, 4, 6} with ties to the even mantissa, saturating at 6.  A value that
rounds to 0 is +0 (code 0); an all-zero block has byte 0 and zero elements.  Codes: bit 3 sign, 0..7 the grid in order.  Storage: [rows][K / 2]
bytes, element k in byte k / 2, low nibble = even k; scales [rows][K / 32].
"""
import numpy as np
import torch

from oracle.llama_ref import RefLlama, quant_rows_e4m3

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)


def e2m1_codes(y: np.ndarray) -> np.ndarray:
    """Codes of values already divided by their block scale: round to nearest, ties to the even mantissa, saturate at 6."""
    a = np.abs(y)
    c = ((a > 0.25).astype(np.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0)).astype(np.uint8)
    return np.where((c != 0) & (y < 0), c | 8, c).astype(np.uint8)


def quant_mxfp4(w: np.ndarray):
    """w [rows, K] (the 16-bit values as float32) -> (codes uint8 [rows, K], scale bytes uint8 [rows, K / 32])."""
    w = np.asarray(w, dtype=np.float32)
    rows, K = w.shape
    assert K % 32 == 0
    blk = w.reshape(rows, K // 32, 32)
    amax = np.abs(blk).max(-1)
    _, e = np.frexp(amax)                                  # amax = f 2^e, f in [0.5, 1): floor(log2(amax)) = e - 1
    X = np.clip(e.astype(np.int32) - 1 - 2, -127, 127)
    nz = amax > 0
    y = np.ldexp(blk, -X[..., None]).astype(np.float32)    # exact: a power-of-two scaling
    codes = np.where(nz[..., None], e2m1_codes(y), 0).astype(np.uint8)
    sb = np.where(nz, 127 + X, 0).astype(np.uint8)
    return codes.reshape(rows, K), sb


def pack_nibbles(codes: np.ndarray) -> np.ndarray:
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack_nibbles(q: np.ndarray) -> np.ndarray:
    out = np.empty((q.shape[0], q.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2] = q & 15
    out[:, 1::2] = q >> 4
    return out


def dequant_mxfp4(codes: np.ndarray, sb: np.ndarray) -> np.ndarray:
    """float32 [rows, K]: e2m1 value x 2^(byte - 127) (exact in float32)."""
    v = E2M1[codes & 7] * np.where(codes & 8, -1.0, 1.0).astype(np.float32)
    rows, K = codes.shape
    s = np.ldexp(np.float32(1.0), sb.astype(np.int32) - 127).astype(np.float32)
    return (v.reshape(rows, K // 32, 32) * s[..., None]).reshape(rows, K).astype(np.float32)


class RefLlamaW4A8(RefLlama):
    """RefLlama whose four layer projections are W4A8: MXFP4 weights quantised from the (16-bit-valued) weights, per-token e4m3
    activations with an fp32 scale (the W8A8 oracle's quant_rows_e4m3), products exact, fp32 sum, the token scale on the sum."""

    def __init__(self, dims, state_dict, max_slots: int = 1024):
        super().__init__(dims, state_dict, max_slots=max_slots)
        self.w4 = {}
        for l in range(self.d.n_layers):
            for pj in self.PROJ:
                name = f"model.layers.{l}.{pj}.weight"
                self.w4[name] = torch.from_numpy(dequant_mxfp4(*quant_mxfp4(self.w[name].numpy())))

    def _proj(self, x: torch.Tensor, name: str) -> torch.Tensor:
        xq, sx = quant_rows_e4m3(x)
        return (xq @ self.w4[name].T) * sx[:, None]
