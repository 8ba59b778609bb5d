"""Test helper: references for the unmerged LoRA target (atspeed_llama_set_lora).

* `LoraRefLlama` / `LoraRefLlamaW4A8`: the oracle's Llama with peft's forward restated on top of its projections,
  `result + scaling * (x @ A.T) @ B.T` for the adapted q / k / v projections, whatever arithmetic the base projection runs in
  (fp32, fp64, W8A8, W4A8): the adapter itself is never quantised.
* `shrink_ref64` / `expand_ref64`: the kernels' rule (csrc/common.h "LoRA side path") in fp64 on the same input values -- the value in
  front of the kernel's roundings -- each with the error bound that follows from the rule.

    xn  = round(w * round(x * rsqrt(mean(x^2) + eps)))
    u   = round(sum_k xn[k] A[j][k])
    d   = round(sum_j u[j] B[c][j])
    y   = round(base + round(scaling * d))           then the rotary pair on y (q, k), one more rounding

`round` = to the engine's 16-bit type; the fp32 engine rounds nothing.
"""
from __future__ import annotations

from typing import Dict, Mapping, Tuple

import numpy as np
import torch

from atspeed_amd import lora as L
from oracle.llama_ref import RefLlama
from tests import rounding as R
from tests.mxfp4_ref import RefLlamaW4A8


class _LoraMixin:
    """`set_lora(adapter)`: adapter = atspeed_amd.lora.Adapter (fp32 CPU tensors).  `tensors_as(dtype)` rounds A and B to the values a 16-bit
    engine holds."""

    _lora: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
    _lora_scaling: float = 0.0

    def set_lora(self, adapter: "L.Adapter", as_dtype: torch.dtype = torch.float32):
        self._lora = {}
        for l, lw in enumerate(adapter.layers):
            for m, (a, b) in lw.items():
                self._lora[f"model.layers.{l}.self_attn.{m}_proj.weight"] = (a.to(as_dtype).to(torch.float32), b.to(as_dtype).to(torch.float32))
        self._lora_scaling = float(np.float32(adapter.scaling))       # the library takes the scaling as a float
        return self

    def clear_lora(self):
        self._lora = {}
        return self

    def _proj(self, x: torch.Tensor, name: str) -> torch.Tensor:
        y = super()._proj(x, name)
        ab = self._lora.get(name)
        if ab is None:
            return y
        a, b = (t.to(x.dtype) for t in ab)
        return y + self._lora_scaling * ((x @ a.T) @ b.T)


class LoraRefLlama(_LoraMixin, RefLlama):
    pass


class LoraRefLlamaW4A8(_LoraMixin, RefLlamaW4A8):
    pass


def merged_state_dict(sd: Mapping, adapter: "L.Adapter") -> Dict[str, torch.Tensor]:
    """W + scaling * B A for every adapted projection, in fp64 (what a merge would store, before any rounding)"""
    out = {k: (torch.from_numpy(np.asarray(v)) if isinstance(v, np.ndarray) else v).to(torch.float64) for k, v in sd.items()}
    s = float(np.float32(adapter.scaling))
    for l, lw in enumerate(adapter.layers):
        for m, (a, b) in lw.items():
            k = f"model.layers.{l}.self_attn.{m}_proj.weight"
            out[k] = out[k] + s * (b.double() @ a.double())
    return out


# ------------------------------------------------------------------ the kernels' rule in fp64
def rnd(x64, dtype: str):
    return np.asarray(x64, dtype=np.float64) if dtype == "fp32" else R.round_to(x64, dtype)


def half_ulp(x64, dtype: str):
    return np.zeros_like(np.asarray(x64, dtype=np.float64)) if dtype == "fp32" else 0.5 * R.ulp(x64, dtype)


TIE_REL = 2.0 ** -21


def rounded_within(x64, e, dtype: str):
    """bound on |round(v) - x| for a v within e of x: e plus half a spacing AT v's magnitude, which may lie in the binade above x's"""
    return e + half_ulp(np.abs(x64) + e, dtype)


def shrink_ref64(h64, w64, a64, eps: float, dtype: str):
    """sum_k xn[k] A[j][k] in fp64 from values of the format -- the value in front of u's rounding: two ROUNDED values can differ by a whole
    spacing when what they round is almost equal, a rounded value is within half a spacing of what it rounds -- and the bound on a kernel that
    sums the same products in fp32 in ANY order and rounds once:
    |got - ref| <= 1/2 ulp16(ref) + H 2^-24 sum_k |xn[k] A[j][k]|  (each of the at most H - 1 partial sums and the H products' accumulation rounds
    once, relative 2^-24 of a partial sum that is at most the sum of the magnitudes; the 16-bit term is the final rounding and is absent in
    fp32).  "The same products" needs one more term in 16 bits: xn is rounded twice on its way (x * rs, then w * that), and the kernel forms
    x * rs from ITS fp32 row statistic, as rmsnorm_kernel does, not from the fp64 one: a sum of H squares, a reciprocal square root and the
    product, a few fp32 roundings -- TIE_REL = 2^-21 (eight of them) covers it.  Where the fp64 value of x * rs lies within TIE_REL of a
    rounding boundary the kernel's value may be the other neighbour, and such a k adds |w| ulp(x rs) |A[j][k]| for that step and
    ulp(w round(x rs)) |A[j][k]| for the second step, which then rounds another value.  (The second step alone cannot flip: the product of two
    16-bit values is exact in fp32.)  Returns (ref, bound, number of near-tie elements): their share must stay small (rounding.CAP over a
    case), so that the term cannot excuse a wrong kernel."""
    h64 = np.asarray(h64, dtype=np.float64)
    rs = 1.0 / np.sqrt((h64 * h64).mean(-1, keepdims=True) + float(np.float32(eps)))
    inner = h64 * rs
    outer = w64 * rnd(inner, dtype)
    xn = rnd(outer, dtype)
    acc = xn @ a64.T
    mag = np.abs(xn) @ np.abs(a64).T
    ref = acc
    e = h64.shape[1] * 2.0 ** -24 * mag
    if dtype == "fp32":
        return ref, e, 0
    tie = R.near_tie(inner, dtype, TIE_REL)
    e = e + (tie * (np.abs(w64) * R.ulp(inner, dtype) + R.ulp(outer, dtype))) @ np.abs(a64).T
    return ref, rounded_within(ref, e, dtype), int(tie.sum())


def expand_ref64(base64, u64, b64, scaling: float, dtype: str):
    """base + scaling * sum_j u[j] B[c][j] in fp64, UNROUNDED (see shrink_ref64), for one module from the projection's values base64, the
    kernel's OWN u (values of the format) and B [H][r16]; and the bound on the kernel's y = round(base + round(scaling * round(fp32 sum))):
    each rounding puts its result within half a spacing of what it rounds, so the three half-ulps add up at each step's magnitude -- d
    (times |scaling| on its way to y), scaling * d, y -- plus |scaling| r16 2^-24 sum_j |u_j B_cj| for the fp32 sum in any order."""
    acc = u64 @ b64.T
    mag = np.abs(u64) @ np.abs(b64).T
    y = base64 + scaling * acc
    r16 = b64.shape[1]
    e_d = rounded_within(acc, r16 * 2.0 ** -24 * mag, dtype)
    e_sd = rounded_within(scaling * acc, abs(scaling) * e_d, dtype)
    return y, rounded_within(y, e_sd, dtype)
