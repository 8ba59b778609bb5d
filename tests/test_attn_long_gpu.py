"""Every attention kernel form at long caches and peaked scores (tests/attn_long_cases.py): tables of up to 2048 slots -- 32 visibility words,
32 K/V tiles, eight laps of the four-stage ring -- and query rows placed so that one key dominates, in the last tile (everything before it is
rescaled by about 0), in the first (the maximum never moves again), twice, or negatively, besides the unit-normal inputs every other
attention test uses.  Each launch goes through every check of tests/test_segs_gpu.py::_check_attention: the fp64 bound relative to
sum_s p_s |v_s| (which does not grow with the key count), poison past total_tok, the lock-step launch against one launch per segment where
both take the same form, the packed output, and a victim segment of huge values that changes no bit elsewhere.  Rows that see nothing must be
exact zeros.  Which 16-rows-per-wave form a launch takes is tests/test_segs_gpu.py::_form16's rule (workgroups, and the ring's LDS: head_dim
128 at 128-row tiles leaves the ring at 24 visibility words); the 32-rows-per-wave forms are told apart by the launch counters.

Bounds: ATTN_C and EPS of tests/test_segs_gpu.py as they stand; the fp32 scalar kernel at 2048 keys has its own entry (LONG_C).  Inputs and
fp64 references are built once per module.  Run with -m gpu on the MI355X box."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib, synth
from atspeed_amd.model import HipLlama, vis_bits_from_bool
from oracle.llama_ref import RefLlama
from tests import attn_long_cases as LC
from tests.guard import assert_same
from tests.test_attn_short_gpu import ONE_BUF, TWO_BUF
from tests.test_segs_gpu import ATTN_C, EPS, TD, Segs, _attention, _caches, _check_attention, _counters, _form16, _poisoned, _st, lib  # noqa: F401
from tests.test_tail_rows_gpu import _check_against_oracle, _lse

FAMILIES = ["normal", "peaked"]
MFMA_SHAPES = [(4, 64), (2, 128)]
N_BLIND = {"long7": 2, "cross": 0}                 # the rows the builder made see nothing
# tree_attn_kernel<float> sums n_vis terms one after the other, so the cap of 8 that ATTN_C["scalar32"] stands at (measured at 200 keys) cannot
# hold at 2048: twice the worst ratio measured on `normal` against the fp64 reference (8.316 at 2 heads x 128 and 32 words:
# profiles/segs_attention_error.txt).  test_scalar32_at_long_caches keeps it below the worst case of the arithmetic.
LONG_C = {"scalar32": 16.63}


def _device(sg):
    """the device side of a table of attn_long_cases: the visibility words include the stale bits at slots >= n_slots"""
    S = Segs.__new__(Segs)
    S.sg = sg
    z = [torch.zeros(t, dtype=torch.int32, device="cuda") for t in sg["n_tok"]]
    S.ids = S.pos = S.slots = z
    S.vis = [torch.from_numpy(LC.bit_words(s["bits"]).view(np.int64)).cuda() for s in sg["segs"]]
    S.kc = S.vc = None
    return S


def _case(name, words, family, n_heads, head_dim, dtype, layer, c=None):
    sg, _, kc, vc = LC.inputs(name, words, family, n_heads, head_dim, dtype)
    ref, mag = LC.ref64(name, words, family, n_heads, head_dim, dtype, layer)
    case = dict(S=_device(sg), q=LC.placed_q(name, words, family, n_heads, head_dim, dtype, layer), kc=kc, vc=vc, ref=ref, mag=mag,
                blind=LC.blind_rows(sg), victim=LC.VICTIM[name])
    assert int(case["blind"].sum()) == N_BLIND[name]
    if c is not None:
        case["c"] = c
    return case


def _run(lib, family, n_heads, head_dim, dtype, layer, qtile, rpw, packed, form, name="long7", words=32, c=None):
    case = _case(name, words, family, n_heads, head_dim, dtype, layer, c)
    return _check_attention(lib, f"{name}/{words}w/{family}", n_heads, head_dim, dtype, layer, qtile, rpw, packed, form, max_slots=64 * words,
                            vis_words=words, case=case)


def _n_qtiles(name, qtile):
    return sum((t + qtile - 1) // qtile for t in LC.table(name)["n_tok"])


# ------------------------------------------------------------------ 16 rows per wave
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("qtile", [64, 128])
@pytest.mark.parametrize("n_heads,head_dim", MFMA_SHAPES)
def test_rows16_at_32_words(lib, n_heads, head_dim, qtile, layer, family):
    """tree_attn_mfma_kernel<DH, NW, 4> through eight laps of its ring; (2, 128) at 128-row tiles is the register-STAGED form here: four tiles of
    head_dim 128 and 128 rows x 32 visibility words do not fit the ring's LDS"""
    form = _form16(_n_qtiles("long7", qtile), n_heads, qtile, head_dim, 32)
    assert form == ("staged" if (head_dim, qtile) == (128, 128) else "ring")
    _run(lib, family, n_heads, head_dim, "bf16", layer, qtile, 16, 1, "rows16" if form == "ring" else "staged16")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("qtile", [64, 128])
def test_rows16_staged_by_grid(lib, qtile, family):
    """33 heads of 64: 10 tiles of 64 rows and 8 of 128 give 330 and 264 workgroups, above the ring's 256"""
    assert _n_qtiles("long7", qtile) * 33 > 256 and _form16(_n_qtiles("long7", qtile), 33, qtile, 64, 32) == "staged"
    _run(lib, family, 33, 64, "bf16", 1, qtile, 16, 1, "staged16")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_heads,head_dim", MFMA_SHAPES)
def test_rows16_256_row_tile(lib, n_heads, head_dim, family):
    """the 256-row tile (16 waves, always register-staged) through atspeed_tree_attention_tiled on the 130-row segment of 1473 slots"""
    i, layer, td, H = 5, 1, torch.bfloat16, n_heads * head_dim
    case = _case("long7", 32, family, n_heads, head_dim, "bf16", layer)
    sg = case["S"].sg
    r0, t, s = int(sg["row0"][i]), sg["n_tok"][i], sg["n_slots"][i]
    q = torch.from_numpy(case["q"][r0: r0 + t]).to(td).cuda()
    kc, vc = (torch.from_numpy(a[i][layer]).to(td).cuda() for a in (case["kc"], case["vc"]))
    out = _poisoned((t + 3, H), td)
    _lib.check(lib.atspeed_tree_attention_tiled(q.data_ptr(), 3 * H, kc.data_ptr(), vc.data_ptr(), case["S"].vis[i].data_ptr(), 32, out.data_ptr(), t, s,
                                                n_heads, head_dim, _lib.ATSPEED_BF16, 256, 16, _st()))
    torch.cuda.synchronize()
    err = np.abs(out[:t].double().cpu().numpy() - case["ref"][r0: r0 + t])
    ratio = float((err / (EPS["bf16"] * case["mag"][r0: r0 + t])).max())
    print(f"256-row tile long7 segment {i} {family} heads={n_heads} dh={head_dim}: max|err|={err.max():.3e} worst |err| / (eps sum p|v|) = {ratio:.3f}")
    assert err.max() <= 3e-2
    assert ratio <= ATTN_C["staged16"], (ratio, ATTN_C["staged16"])
    assert_same("rows past n_tokens", out[t:].cpu(), _poisoned((3, H), td).cpu())


# ------------------------------------------------------------------ 32 rows per wave
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("qtile", [64, 128, 256])
@pytest.mark.parametrize("n_heads,head_dim", MFMA_SHAPES)
def test_rows32_at_32_words(lib, n_heads, head_dim, qtile, family):
    """tree_attn32_kernel single-buffered (64-row tiles) and double-buffered (128, 256) over words 8 .. 31 and keys beyond 512, told apart by the
    launch counters; the 64-row launch equals the 128-row one bit for bit (the 32-row wave groups are the same partition of a segment in both
    tilings: tests/test_attn_short_gpu.py)"""
    case = _case("long7", 32, family, n_heads, head_dim, "bf16", 1)
    S, td, H = case["S"], torch.bfloat16, n_heads * head_dim
    q = torch.from_numpy(case["q"]).to(td).cuda()
    S.kc, S.vc = _caches(S.sg, H, td, case["kc"]), _caches(S.sg, H, td, case["vc"])
    c0 = _counters(lib)
    out = _attention(lib, S, q, H, n_heads, head_dim, td, 1, qtile, 32, 0, max_slots=2048, vis_words=32)
    c1 = _counters(lib)
    assert (c1[ONE_BUF] - c0[ONE_BUF], c1[TWO_BUF] - c0[TWO_BUF]) == ((1, 0) if qtile == 64 else (0, 1))
    if qtile == 64:
        wide = _attention(lib, S, q, H, n_heads, head_dim, td, 1, 128, 32, 0, max_slots=2048, vis_words=32)
        assert_same("64-row single-buffered vs 128-row double-buffered", out.cpu(), wide.cpu())
    _check_attention(lib, f"long7/32w/{family}", n_heads, head_dim, "bf16", 1, qtile, 32, 1, "rows32", max_slots=2048, vis_words=32, case=case)


@pytest.mark.parametrize("rpw,n_heads,head_dim,qtile,form", [(16, 2, 128, 64, "rows16"), (32, 4, 64, 128, "rows32")])
def test_fp16(lib, rpw, n_heads, head_dim, qtile, form):
    """the fp16 flavour of each MFMA family on the placed rows (an fp16 p keeps 11 bits where bf16 keeps 8: eps is 2^-11)"""
    _run(lib, "peaked", n_heads, head_dim, "fp16", 1, qtile, rpw, 0, form)


# ------------------------------------------------------------------ the ring's LDS boundary
@pytest.mark.parametrize("words,qtile,form", [(23, 128, "ring"), (24, 128, "staged"), (24, 64, "ring")])
def test_ring_lds_boundary(lib, words, qtile, form):
    """head_dim 128: four tiles take 139264 of the 163776 bytes a workgroup may ask for, so 128-row tiles keep the ring up to 23 visibility
    words and take the register-staged form from 24 on (max_slots >= 1536); 64-row tiles stay.  Each side against fp64 (the forms round
    differently: no bit identity across them)."""
    assert _form16(_n_qtiles("cross", qtile), 2, qtile, 128, words) == form
    _run(lib, "normal", 2, 128, "bf16", 1, qtile, 16, 1, "rows16" if form == "ring" else "staged16", name="cross", words=words)


# ------------------------------------------------------------------ the scalar kernel
@pytest.mark.parametrize("family", FAMILIES)
def test_scalar16_at_32_words(lib, family):
    """tree_attn_kernel<fp16>, head_dim 32: 16 * (32 + 128 * 32) = 66048 bytes of dynamic LDS, above 64 KiB"""
    _run(lib, family, 4, 32, "fp16", 1, 0, 0, 0, "scalar16")


def _check_fp32_rows(name, got, ref, mag, n_vis, head_dim, c):
    """per row against the worst case of the arithmetic: n_vis + head_dim + 32 fp32 roundings (the sequential sums of n_vis probabilities and of
    n_vis products, the head_dim products of a score, the exponential and the division)"""
    keep = n_vis > 0
    ratio = (np.abs(got - ref)[keep] / (EPS["fp32"] * mag[keep])).max(1)
    worst_case = (n_vis[keep] + head_dim + 32).astype(np.float64)
    assert (ratio <= worst_case).all(), (name, float((ratio / worst_case).max()))
    assert c < float(worst_case.max()), (name, c, float(worst_case.max()))


@pytest.mark.parametrize("n_heads,head_dim,words", [(4, 32, 32), (4, 128, 31), (4, 128, 32), (2, 128, 32)])
def test_scalar32_at_long_caches(lib, n_heads, head_dim, words):
    """tree_attn_kernel<float> (the fp32 parity mode): head_dim 32 at 32 words (66048 bytes of LDS), head_dim 128 at 31 words (exactly 65536) and
    at 32 (67584).  Four heads: the fourth wave's slot list and probabilities are the last of the allocation, and the one row of the last
    segment sees every slot, so the bytes beyond 64 KiB are written and read.  (2, 128) is the engine test's shape and the worst ratio measured.
    Unit-normal inputs only."""
    case = _case("long7", words, "normal", n_heads, head_dim, "fp32", 1, c=LONG_C["scalar32"])
    ratio, out = _check_attention(lib, f"long7/{words}w/normal", n_heads, head_dim, "fp32", 1, 0, 0, 0, "scalar32", max_slots=64 * words, vis_words=words,
                                  case=case)
    T = case["S"].sg["total_tok"]
    _check_fp32_rows(f"scalar32 dh={head_dim} {words}w", out[:T].double().cpu().numpy(), case["ref"], case["mag"], LC.n_visible(case["S"].sg), head_dim,
                     LONG_C["scalar32"])


@pytest.mark.parametrize("i", [0, 6])
def test_scalar32_one_segment_at_2048_slots(lib, i):
    """atspeed_tree_attention (one segment, everything automatic) in fp32 at 2048 slots: the 40 rows of the tree segment, and the one row that
    sees every slot"""
    layer, n_heads, head_dim, td = 1, 4, 32, torch.float32
    H = n_heads * head_dim
    case = _case("long7", 32, "normal", n_heads, head_dim, "fp32", layer)
    sg = case["S"].sg
    r0, t, s = int(sg["row0"][i]), sg["n_tok"][i], sg["n_slots"][i]
    assert s == 2048
    q = torch.from_numpy(case["q"][r0: r0 + t]).to(td).cuda()
    kc, vc = (torch.from_numpy(a[i][layer]).cuda() for a in (case["kc"], case["vc"]))
    out = _poisoned((t + 3, H), td)
    _lib.check(lib.atspeed_tree_attention(q.data_ptr(), 3 * H, kc.data_ptr(), vc.data_ptr(), case["S"].vis[i].data_ptr(), 32, out.data_ptr(), t, s, n_heads,
                                          head_dim, _lib.dtype_code(td), _st()))
    torch.cuda.synchronize()
    got, ref, mag = out[:t].double().cpu().numpy(), case["ref"][r0: r0 + t], case["mag"][r0: r0 + t]
    err = np.abs(got - ref)
    ratio = float((err / (EPS["fp32"] * mag)).max())
    print(f"one segment fp32 {t} x 2048 heads={n_heads} dh={head_dim}: max|err|={err.max():.3e} worst |err| / (eps sum p|v|) = {ratio:.3f}")
    assert err.max() <= 2e-5
    assert ratio <= LONG_C["scalar32"], (ratio, LONG_C["scalar32"])
    _check_fp32_rows("one segment", got, ref, mag, sg["segs"][i]["vis"].sum(1), head_dim, LONG_C["scalar32"])
    assert_same("rows past n_tokens", out[t:].cpu(), _poisoned((3, H), td).cpu())


# ------------------------------------------------------------------ the engine at max_slots = 2048
V, HIDDEN, HEADS, FFN, SLOTS = 384, 256, 2, 512, 2048            # the tiny dims of tests/test_tail_rows_gpu.py: 2 heads of 128
N1, N2, PREFIX, BRANCHES = 150, 20, 30, 4


def _rounds():
    """a tree over the whole arena: 150 tokens at slots spread over [0, 2048), slot 2047 among them -- a causal prefix of 30, then four branches
    (token r follows token r - 4) -- and a second round of 20 tokens, five more per branch, that sees the prefix and its branch"""
    g = torch.Generator().manual_seed(2048)
    pool = torch.randperm(SLOTS - 1, generator=g)[: N1 + N2 - 1].to(torch.int32)
    slots1 = torch.cat((pool[:70], torch.tensor([SLOTS - 1], dtype=torch.int32), pool[70: N1 - 1]))
    slots2 = pool[N1 - 1:]
    assert slots1.numel() == N1 and slots2.numel() == N2 and int(slots1.max()) == SLOTS - 1 and int(slots1.min()) < 64
    anc1 = lambda r: list(range(min(r, PREFIX - 1) + 1)) + list(range(PREFIX + (r - PREFIX) % BRANCHES, r + 1, BRANCHES) if r >= PREFIX else [])
    vis1 = torch.zeros(N1, SLOTS, dtype=torch.bool)
    for r in range(N1):
        vis1[r, slots1[anc1(r)].long()] = True
    pos1 = torch.tensor([r if r < PREFIX else PREFIX + (r - PREFIX) // BRANCHES for r in range(N1)], dtype=torch.int32)
    vis2 = torch.zeros(N2, SLOTS, dtype=torch.bool)
    for j in range(N2):
        vis2[j, slots1[anc1(N1 - BRANCHES + j % BRANCHES)].long()] = True
        vis2[j, slots2[list(range(j % BRANCHES, j + 1, BRANCHES))].long()] = True
    pos2 = torch.tensor([int(pos1[-1]) + 1 + j // BRANCHES for j in range(N2)], dtype=torch.int32)
    ids1 = torch.randint(3, V, (N1,), generator=g).to(torch.int32)
    ids2 = torch.randint(3, V, (N2,), generator=g).to(torch.int32)
    assert not torch.equal(vis1[:, slots1.long()], torch.tril(torch.ones(N1, N1, dtype=torch.bool)))       # a tree, not a causal mask
    return (ids1, pos1, slots1, vis1, 40), (ids2, pos2, slots2, vis2, N2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_engine_at_2048_slots(dtype):
    """a model created with max_slots = 2048 (32 visibility words in every attention launch; in fp32 the scalar kernel at 67584 bytes of LDS):
    both rounds against the fp32 oracle under the bounds of tests/test_tail_rows_gpu.py"""
    dims = synth.LlamaDims(V, HIDDEN, 2, HEADS, FFN)
    sd = synth.synthetic_state_dict(dims, 31, std=0.05, head_std=0.1)
    m = HipLlama.from_state_dict(dims, sd, TD[dtype], max_slots=SLOTS, max_tokens=512, max_logit_rows=128)
    ref = RefLlama(m.dims, m.export_state_dict(), max_slots=SLOTS)
    for what, (ids, pos, slots, vis, n_logit) in zip(("150 tokens over the arena", "the round behind them"), _rounds()):
        want = ref.forward(ids, pos, slots, vis, n_logit_rows=n_logit)
        got = m.forward_raw(ids.cuda(), pos.cuda(), slots.cuda(), vis_bits_from_bool(vis, SLOTS).cuda(), SLOTS, n_logit).clone()
        _check_against_oracle(f"max_slots 2048: {what}", dtype, got, _lse(m, n_logit), want)
