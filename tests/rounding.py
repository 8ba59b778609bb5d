"""Rounding of fp64 reference values to the engine's number formats (test infrastructure, a plain module like tests/guard.py; numpy on the CPU).

The kernels compute in fp32 from 16-bit (or fp32) inputs and round once or twice to 16 bits; a test's reference is fp64 on the same input
values.  The two can disagree only where the fp64 value lies within the fp32 evaluation error of a rounding boundary, i.e. of the midpoint of
two neighbouring values of the format.  `assert_rounded` therefore asks for the nearest-even rounding of the reference, bit for bit, on every
element that is not such a near tie, accepts either neighbour on the near ties, and fails when near ties are more than a stated share of the
case (so that "near tie" cannot become the excuse of a wrong kernel).  tests/test_rounding_cpu.py checks this module against torch's casts."""
from __future__ import annotations

import numpy as np

# format -> (explicit mantissa bits, exponent of the smallest normal value, largest finite value)
FORMATS = {
    "bf16": (7, -126, float.fromhex("0x1.fep127")),
    "fp16": (10, -14, 65504.0),
    "fp32": (23, -126, float.fromhex("0x1.fffffep127")),
}
REL = 2.0 ** -20        # near-tie band: a handful of fp32 roundings of 2^-24 each
CAP = 0.005             # near ties may be at most this share of a case's elements (a condition, not a measurement)


def fmt(dtype) -> str:
    """'bf16' / 'fp16' / 'fp32' from a name or a torch dtype"""
    s = str(dtype)
    for name, keys in (("bf16", ("bf16", "bfloat16")), ("fp16", ("fp16", "float16", "half")), ("fp32", ("fp32", "float32"))):
        if any(s == k or s == "torch." + k for k in keys):
            return name
    raise TypeError(f"no such format: {dtype}")


def ulp(x64, dtype) -> np.ndarray:
    """spacing of the format's values in the binade of x (the subnormal spacing below the smallest normal value, also for 0)"""
    p, emin, _ = FORMATS[fmt(dtype)]
    x = np.abs(np.asarray(x64, dtype=np.float64))
    e = np.frexp(x)[1].astype(np.int64) - 1                 # floor(log2 |x|); frexp(0) gives exponent 0, clipped below
    e = np.where(x == 0, emin, np.maximum(e, emin))
    return np.ldexp(1.0, (e - p).astype(np.int64))


def _floor_ceil(x64, dtype):
    """the format's neighbours lo <= x <= hi of x (equal when x is a value of the format), unbounded in range"""
    x = np.asarray(x64, dtype=np.float64)
    u = ulp(x, dtype)
    q = x / u                                               # exact: u is a power of two
    return np.floor(q) * u, np.ceil(q) * u, u


def round_to(x64, dtype) -> np.ndarray:
    """x rounded to the nearest value of the format, ties to the even mantissa; overflow gives +-inf.  Returned as fp64."""
    x = np.asarray(x64, dtype=np.float64)
    u = ulp(x, dtype)
    r = np.rint(x / u) * u                                  # rint: ties to even; x / u and the product are exact
    big = FORMATS[fmt(dtype)][2]
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(r) > big, np.sign(x) * np.inf, r)


def near_tie(x64, dtype, rel=REL, mag64=None) -> np.ndarray:
    """True where x lies within rel * mag of the midpoint between two neighbouring values of the format.  mag defaults to |x|; an expression
    whose fp32 evaluation error scales with its operands rather than with its value (a difference of products: the rotary pair) passes the
    operands' magnitude, e.g. |x0 c| + |x1 s|."""
    x = np.asarray(x64, dtype=np.float64)
    lo, _, u = _floor_ceil(x, dtype)
    mag = np.abs(x) if mag64 is None else np.asarray(mag64, dtype=np.float64)
    return np.abs(x - (lo + 0.5 * u)) <= rel * mag


def _matches(got, ref64, dtype, band):
    """got is the rounding of SOME value within `band` of the reference: away from a midpoint that is round_to(ref64) itself, at a near tie either
    neighbour (and, where cancellation leaves a value so small that the band spans more than one spacing of the format, the values in between)"""
    return (got >= round_to(ref64 - band, dtype)) & (got <= round_to(ref64 + band, dtype))


def assert_rounded(got, ref64, dtype, rel=REL, cap=CAP, mag64=None, alt64=None, name="result"):
    """got (values of the format, any float array) against the fp64 reference: every element that is not a near tie equals round_to(ref64)
    exactly, a near tie may be either neighbour, and near ties are at most `cap` of the elements.  alt64: a second, equally valid reference
    for results of TWO rounding steps -- where the first step was a near tie the kernel may have continued from the other neighbour, and
    alt64 holds the reference continued from that one (equal to ref64 elsewhere); those elements count as near ties.  rel = 0: the kernel
    evaluates the expression exactly in fp32 (a product of two 16-bit values), so nothing is a near tie and an exact tie rounds to even.
    Returns the share of near ties."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    none = np.zeros(ref.shape, dtype=bool)
    band = lambda x: rel * (np.abs(x) if mag64 is None else np.asarray(mag64, dtype=np.float64))
    tie = near_tie(ref, dtype, rel, mag64) if rel > 0 else none
    ok = _matches(got, ref, dtype, band(ref))
    if alt64 is not None:
        alt = np.asarray(alt64, dtype=np.float64)
        differs = alt != ref
        ok |= differs & _matches(got, alt, dtype, band(alt))
        tie = tie | differs
    share = float(tie.mean()) if tie.size else 0.0
    if not ok.all():
        idx = tuple(int(i) for i in np.argwhere(~ok)[0])
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.size} elements are not the rounded reference; first at {idx}: got {got[idx]!r}, "
                             f"reference {ref[idx]!r} -> {float(round_to(ref[idx], dtype))!r} ({fmt(dtype)}, near tie: {bool(tie[idx])})")
    assert share <= cap, f"{name}: {share:.4%} of the elements are near ties (cap {cap:.2%}): the case cannot tell a wrong rounding from a tie"
    return share
