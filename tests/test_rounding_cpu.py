"""tests/rounding.py against torch's own casts, and the near-tie share of every case of tests/test_segs_gpu.py that uses assert_rounded, computed
from the fp64 references alone (no GPU): a case whose near ties exceeded the cap could not tell a wrong rounding from a tie."""
import numpy as np
import pytest
import torch

from tests import rounding as R
from tests import segs_cases as SC

FMTS = ["bf16", "fp16", "fp32"]


def _torch_round(x64, name):
    return torch.from_numpy(np.asarray(x64, dtype=np.float64)).to(SC.TORCH[name]).double().numpy()


def _values(name):
    """random values over the format's range, its boundary values and the exact midpoints of neighbours (ties)"""
    p, emin, big = R.FORMATS[name]
    rng = np.random.default_rng(11)
    x = [rng.standard_normal(20000), rng.standard_normal(20000) * 1e-3, np.ldexp(rng.standard_normal(5000), rng.integers(emin - p - 3, emin + 4, 5000)),
         np.ldexp(1 + rng.random(5000), rng.integers(100, 128 if name != "fp16" else 16, 5000) if name != "fp16" else rng.integers(10, 16, 5000))]
    g = min(p, 10)                                                                      # (fp32: every 2^13-th value of the binade)
    grid = np.ldexp(np.arange(2 ** g, 2 ** (g + 1) + 1, dtype=np.float64), -g)          # every value of one binade, and the next power of two
    grid = np.concatenate([grid, grid[:-1] + np.ldexp(1.0, -p)]) if g < p else grid     # ... and their upper neighbours
    for e in (0, emin, emin + 1, -3, 5):
        g = np.ldexp(grid, e)
        x += [g, (g[:-1] + g[1:]) / 2, np.nextafter((g[:-1] + g[1:]) / 2, np.inf), np.nextafter((g[:-1] + g[1:]) / 2, -np.inf)]
    sub = np.ldexp(np.arange(0, 40, dtype=np.float64), emin - p)                        # subnormals and their midpoints
    x += [sub, sub + np.ldexp(0.5, emin - p), np.array([0.0, big, big * (1 + 2.0 ** -(p + 2)), big * (1 + 2.0 ** -(p + 1)), big * 2])]
    x = np.concatenate(x)
    return np.concatenate([x, -x])


@pytest.mark.parametrize("name", FMTS)
def test_round_to_equals_the_torch_cast(name):
    # torch casts fp64 to a 16-bit type THROUGH fp32 (two roundings: 1 + 2^-8 + 2^-52 becomes 1.0 in bf16), so the comparison is made on
    # fp32-representable inputs, where its cast rounds once; fp64 inputs a hair past a midpoint are checked directly below
    x = _values(name)
    with np.errstate(all="ignore"):
        x32 = x.astype(np.float32).astype(np.float64)
        assert np.array_equal(R.round_to(x32, name), _torch_round(x32, name))
    lo = _torch_round(np.random.default_rng(2).standard_normal(3000), name)
    hi = lo + R.ulp(np.where(lo >= 0, lo, np.nextafter(lo, 0)), name)
    hi = np.where(R.round_to(hi, name) == hi, hi, lo)                       # (keeps lo where the step crossed zero's binade oddly: then no check)
    mid = (lo + hi) / 2
    ok = hi > lo
    assert np.array_equal(R.round_to(np.nextafter(mid, np.inf), name)[ok], hi[ok]) and np.array_equal(R.round_to(np.nextafter(mid, -np.inf), name)[ok], lo[ok])
    assert np.array_equal(R.round_to(x, SC.TORCH[name]), R.round_to(x, name))          # a torch dtype names the format too


@pytest.mark.parametrize("name", FMTS)
def test_ulp_is_the_distance_to_the_next_value(name):
    p, emin, big = R.FORMATS[name]
    x = np.abs(_torch_round(np.random.default_rng(3).standard_normal(5000) * 3, name))
    x = np.concatenate([x, np.ldexp(1.0, np.arange(emin - 2, 15)), [0.0]])
    nxt = torch.nextafter(torch.from_numpy(x).to(SC.TORCH[name]), torch.tensor(float("inf"), dtype=SC.TORCH[name])).double().numpy()
    assert np.array_equal(R.ulp(x, name), nxt - x)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_near_tie_and_assert_rounded(name):
    p, emin, _ = R.FORMATS[name]
    lo = _torch_round(np.random.default_rng(5).standard_normal(4000), name)
    hi = torch.nextafter(torch.from_numpy(lo).to(SC.TORCH[name]), torch.tensor(float("inf"), dtype=SC.TORCH[name])).double().numpy()
    mid = (lo + hi) / 2
    inside = mid + 0.5 * R.REL * np.abs(mid)
    outside = mid + 4 * R.REL * np.abs(mid) + np.ldexp(1.0, emin - p - 30)
    assert R.near_tie(mid, name).all() and R.near_tie(inside, name).all() and not R.near_tie(outside, name).any()
    assert not R.near_tie(lo + 0.25 * (hi - lo), name).any()
    # a wider band through the operands' magnitude
    assert R.near_tie(outside, name, mag64=64 * np.abs(mid)).all()
    x = np.concatenate([lo + 0.3 * (hi - lo), inside[:10]])                     # 10 near ties in 4010 elements: under the cap
    good = R.round_to(x, name)
    assert R.assert_rounded(good, x, name) == pytest.approx(10 / 4010)
    either = good.copy(); either[-10:] = lo[:10]                               # a near tie may be either neighbour
    R.assert_rounded(either, x, name)
    bad = good.copy(); bad[7] = hi[7]                                          # ... anything else must be the nearest value
    with pytest.raises(AssertionError, match="not the rounded reference"):
        R.assert_rounded(bad, x, name)
    far = good.copy(); far[-1] = hi[9] + (hi[9] - lo[9])                       # ... and a near tie not a third value
    with pytest.raises(AssertionError, match="not the rounded reference"):
        R.assert_rounded(far, x, name)
    with pytest.raises(AssertionError, match="near ties"):
        R.assert_rounded(R.round_to(inside, name), inside, name)               # all ties: over the cap
    # two rounding steps: where the first was a near tie, the continuation from the other neighbour is accepted and counted as a tie
    alt = x.copy(); alt[:5] = x[:5] * 1.5
    two = good.copy(); two[:5] = R.round_to(alt[:5], name)
    with pytest.raises(AssertionError):
        R.assert_rounded(two, x, name)
    assert R.assert_rounded(two, x, name, alt64=alt) == pytest.approx(15 / 4010)
    # rel = 0: an exactly evaluated expression has no near ties, an exact tie rounds to even
    assert R.assert_rounded(R.round_to(mid, name), mid, name, rel=0) == 0
    with pytest.raises(AssertionError, match="not the rounded reference"):
        R.assert_rounded(np.where(R.round_to(mid, name) == lo, hi, lo), mid, name, rel=0)


# ------------------------------------------------------------------ the cases of tests/test_segs_gpu.py stay under the cap
ROPE_SHAPES = [(4, 32), (12, 64), (2, 128), (3, 24)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n_heads,head_dim", ROPE_SHAPES)
def test_rope_cases_stay_under_the_near_tie_cap(n_heads, head_dim, dtype):
    sg = SC.segments("ragged5")
    H = n_heads * head_dim
    qkv = SC.rope_qkv("ragged5", n_heads, head_dim, dtype)
    srcs = [qkv]
    if head_dim % 16 == 0:
        srcs += [SC.rope_slabs("ragged5", n_heads, head_dim, dtype, s)[1] for s in (1, 3, 4, 6)]
    for src in srcs:
        for part in (src[:, :H], src[:, H: 2 * H]):
            ref, mag = SC.rope_rotate64(part, SC.all_pos(sg), n_heads, head_dim)
            assert R.near_tie(ref, dtype, SC.ROPE_REL, mag).mean() <= R.CAP


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("form,m,n,k", SC.RESID_NORM_16)
def test_norm_cases_stay_under_the_near_tie_cap(form, m, n, k, dtype):
    """h as the fp64 product + residual rounded once (the GPU test takes the h the kernel stored: the same values up to its last bit), on the
    first 64 rows of a case: the share is a property of the rows' distribution, and the GPU test checks the cap again on every call"""
    a, w, r, nw = SC.resid_inputs(m, n, k, dtype)
    a, r = a[:64], r[:64]
    h = R.round_to(r.double().numpy() + R.round_to(a.double().numpy() @ w.double().numpy().T, dtype), dtype)
    inner, outer, alt = SC.norm_ref64(h, nw.double().numpy(), 1e-5, dtype)
    share = (alt != outer).mean()              # the second step, a product of two 16-bit values, is exact in fp32: only the first step has near ties
    assert share <= R.CAP, share


def test_segment_fixtures_have_the_edges_the_gpu_tests_rely_on():
    r5, m32 = SC.segments("ragged5"), SC.segments("many32")
    assert r5["n_tok"] == [1, 63, 64, 65, 130] and r5["n_slots"] == [1, 70, 64, 129, 200] and r5["total_tok"] == 323
    assert m32["n"] == 32 and all(9 <= t <= 30 for t in m32["n_tok"]) and m32["n_logit"][5] == 0 and m32["n_logit"][4] > 0 and m32["n_logit"][6] > 0
    assert (m32["total_tok"] + 127) // 128 <= 32 and 32 * 16 >= 512            # 32 query tiles of 128 rows x 16 heads: the 32-rows-per-wave kernel
    for sg in (r5, m32):
        for i, s in enumerate(sg["segs"]):
            assert len(set(s["slots"].tolist())) == sg["n_tok"][i] and s["slots"].max() < SC.MAX_SLOTS and s["vis"].any(1).all()
            assert sg["n_tok"][i] == 1 or not np.array_equal(s["slots"], np.arange(sg["n_tok"][i]))
    pos = SC.all_pos(r5)
    assert {-1, SC.MAX_POS - 1, SC.MAX_POS, SC.MAX_POS + 7} <= set(pos.tolist()) and len(pos) - len(set(pos.tolist())) >= 3
    w = SC.vis_words(r5["segs"][4]["vis"])
    assert w.shape == (130, 4) and int(w[3, 3]) == 1 << (199 - 192) and not w[3, :3].any()
