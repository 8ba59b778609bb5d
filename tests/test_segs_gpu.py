"""The kernels behind the segment table -- embedding gather, logit-row gather, row info, RoPE + KV scatter, multi-segment tree attention -- and the
fused residual + RMSNorm tail of the residual projections, each called alone through its low-level entry point and compared with an fp64
reference on the same input values (tests/segs_cases.py builds inputs and references on the CPU; tests/rounding.py states how a 16-bit result
may differ from a rounded fp64 value).  Whole forwards exercise these kernels too, but only against themselves or at a few percent of
max |logit|.  Run with -m gpu on the MI355X box."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib
from tests import guard, rounding as R, segs_cases as SC
from tests.guard import assert_same

TD = SC.TORCH
POISON16, POISON32 = 0x7FC1, 0x7FC00001          # NaNs no kernel writes


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    l = _lib.load()
    assert l.atspeed_device_count() >= 1
    return l


def _st():
    return _lib.stream_ptr()


def _poisoned(shape, dtype):
    """a device tensor of `dtype` whose every element is a NaN pattern of the test's own"""
    if dtype == torch.float32:
        return torch.full(shape, POISON32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, POISON16, dtype=torch.int16, device="cuda").view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Segs:
    """the device side of a fixture of tests/segs_cases.py and the ATSPEED_SEGMENTS argument list"""

    def __init__(self, name, kc=None, vc=None):
        self.sg = sg = SC.segments(name)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
        self.ids = [dev(s["ids"], np.int32) for s in sg["segs"]]
        self.pos = [dev(s["pos"], np.int32) for s in sg["segs"]]
        self.slots = [dev(s["slots"], np.int32) for s in sg["segs"]]
        self.vis = [torch.from_numpy(SC.vis_words(s["vis"]).view(np.int64)).cuda() for s in sg["segs"]]
        self.kc, self.vc = kc, vc

    def args(self, n_logit=None):
        n = self.sg["n"]
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts]) if ts is not None else None
        cnt = lambda v: (C.c_int32 * n)(*v)
        self._keep = [arr(self.ids), arr(self.pos), arr(self.slots), arr(self.vis), arr(self.kc), arr(self.vc), cnt(self.sg["n_tok"]), cnt(self.sg["n_slots"]),
                      cnt(self.sg["n_logit"] if n_logit is None else n_logit)]
        return [n] + self._keep


# ------------------------------------------------------------------ a. embed / gather / row_info
@pytest.mark.parametrize("hidden", [64, 768])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("seg_name", ["ragged5", "many32"])
def test_embed_gather_row_info(lib, seg_name, dtype, hidden):
    """embed_segs_kernel, gather_logit_rows_kernel and row_info_kernel against numpy indexing, bit for bit: the three binary searches over the table
    (many32 holds segments WITHOUT logit rows, which share their logit_row0 with the next segment), the id clamp (-3 -> row 0, vocab + 5 -> the last
    row) and the position clamp; rows past the totals keep their poison."""
    S = Segs(seg_name)
    sg, td, code = S.sg, TD[dtype], _lib.dtype_code(TD[dtype])
    T, L, V = sg["total_tok"], sg["total_logit"], sg["vocab"]
    table = torch.from_numpy(np.random.default_rng(1).standard_normal((V, hidden)).astype(np.float32)).to(td).cuda()
    out = _poisoned((T + 3, hidden), td)
    _lib.check(lib.atspeed_segs_embed(table.data_ptr(), hidden, V, code, out.data_ptr(), *S.args(), _st()))
    ids = np.clip(np.concatenate([s["ids"] for s in sg["segs"]]), 0, V - 1)
    assert_same("embed", out[:T].cpu(), table.cpu()[torch.from_numpy(ids).long()])
    assert_same("embed rows past total_tok", out[T:].cpu(), _poisoned((3, hidden), td).cpu())

    h = out[:T].contiguous()
    gath = _poisoned((L + 3, hidden), td)
    _lib.check(lib.atspeed_segs_gather_logit_rows(h.data_ptr(), hidden, code, gath.data_ptr(), *S.args(), _st()))
    rows = np.concatenate([np.arange(sg["row0"][i] + sg["n_tok"][i] - sg["n_logit"][i], sg["row0"][i] + sg["n_tok"][i]) for i in range(sg["n"])])
    assert len(rows) == L
    assert_same("gather_logit_rows", gath[:L].cpu(), h.cpu()[torch.from_numpy(rows).long()])
    assert_same("gather rows past total_logit", gath[L:].cpu(), _poisoned((3, hidden), td).cpu())

    if dtype == "fp32" and hidden == 64:                      # (row_info has no type and no width)
        kc = [0x1000 * (i + 1) for i in range(sg["n"])]
        vc = [0x7000000 + 0x1000 * i for i in range(sg["n"])]
        info = torch.full((T + 3, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        a = S.args()
        a[5], a[6] = (C.c_void_p * sg["n"])(*kc), (C.c_void_p * sg["n"])(*vc)        # never dereferenced by this kernel
        _lib.check(lib.atspeed_segs_row_info(info.data_ptr(), SC.MAX_POS, *a, _st()))
        rec = info.cpu().numpy()
        want = np.zeros((T, 6), dtype=np.int32)
        seg_of = np.repeat(np.arange(sg["n"]), sg["n_tok"])
        want.view(np.int64)[:, 0] = np.array(kc)[seg_of]
        want.view(np.int64)[:, 1] = np.array(vc)[seg_of]
        want[:, 4] = SC.clamp_pos(SC.all_pos(sg))
        want[:, 5] = np.concatenate([s["slots"] for s in sg["segs"]])
        assert np.array_equal(rec[:T], want), np.argwhere(rec[:T] != want)[:4]
        assert (rec[T:] == 0x5A5A5A5A).all()


# ------------------------------------------------------------------ b. RoPE + KV scatter
def _caches(sg, H, td, values=None, max_slots=SC.MAX_SLOTS):
    """per segment [LAYERS][max_slots][H]: poison, or the given values (numpy arrays that hold values of the format)"""
    if values is None:
        return [_poisoned((SC.LAYERS, max_slots, H), td) for _ in range(sg["n"])]
    return [torch.from_numpy(v).to(td).cuda() for v in values]


def _check_rope(sg, name, dtype, n_heads, head_dim, layer, src64, q_out, kcs, vcs, check_kv_cols_of=None):
    """q rows of q_out, and rows [layer][slot] of the caches, against the fp64 rotation of src64 [T][3 H] (values of the format)"""
    H = n_heads * head_dim
    pos = SC.all_pos(sg)
    for part, nm in ((0, "q"), (1, "k")):
        ref, mag = SC.rope_rotate64(src64[:, part * H: (part + 1) * H], pos, n_heads, head_dim)
        if part == 0:
            got = q_out[:, :H].double().cpu().numpy()
        else:
            got = np.concatenate([kcs[i][layer].double().cpu().numpy()[s["slots"]] for i, s in enumerate(sg["segs"])])
        if dtype == "fp32":
            err = np.abs(got - ref)
            assert (err <= 4 * 2.0 ** -24 * mag).all(), (name, nm, float((err / mag).max()))
        else:
            R.assert_rounded(got, ref, dtype, SC.ROPE_REL, R.CAP, mag64=mag, name=f"{name} rotated {nm}")
    v_got = torch.cat([vcs[i][layer][torch.from_numpy(s["slots"]).long().cuda()] for i, s in enumerate(sg["segs"])])
    assert_same(f"{name} v at cache[layer][slot]", v_got.cpu(), torch.from_numpy(src64[:, 2 * H:]).to(TD[dtype]))
    # every cache row no token names, and the whole other layer, keep their poison
    for i, s in enumerate(sg["segs"]):
        untouched = np.ones(SC.MAX_SLOTS, dtype=bool)
        untouched[s["slots"]] = False
        for c in (kcs[i], vcs[i]):
            b = _bits(c).cpu().numpy()
            want = POISON32 if dtype == "fp32" else POISON16
            assert (b[1 - layer] == want).all() and (b[layer][untouched] == want).all(), (name, "a cache row no token names was written", i)


ROPE_SHAPES = [(4, 32), (12, 64), (2, 128), (3, 24)]       # (3, 24): head_dim % 16 != 0, the scalar kernel also in 16 bits


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("n_heads,head_dim", ROPE_SHAPES)
def test_rope_kv(lib, n_heads, head_dim, dtype, layer):
    """rope_kv_segs_kernel<T> (fp32; 16-bit with head_dim 24) and rope_kv_segs_vec_kernel on ragged5: rotated q in place and rotated k at
    cache[layer][slot] = the fp64 rotate-half of the same values with the same fp32 table values, rounded once; v bit-exact; the k / v columns of qkv
    unchanged; positions -1, MAX_POS and MAX_POS + 7 take table rows 0 and MAX_POS - 1 (the reference clamps); nothing else in the caches is touched."""
    S = Segs("ragged5")
    sg, td, H = S.sg, TD[dtype], n_heads * head_dim
    src = SC.rope_qkv("ragged5", n_heads, head_dim, dtype)
    qkv = torch.from_numpy(src).to(td).cuda()
    before = qkv.clone()
    S.kc, S.vc = _caches(sg, H, td), _caches(sg, H, td)
    cos, sin = (torch.from_numpy(t).cuda() for t in SC.rope_tables(head_dim))
    loff = layer * SC.MAX_SLOTS * H * qkv.element_size()
    _lib.check(lib.atspeed_segs_rope_kv(qkv.data_ptr(), None, 0, cos.data_ptr(), sin.data_ptr(), loff, n_heads, head_dim, SC.MAX_POS, _lib.dtype_code(td),
                                        *S.args(), _st()))
    torch.cuda.synchronize()
    _check_rope(sg, "rope", dtype, n_heads, head_dim, layer, src, qkv, S.kc, S.vc)
    assert_same("k and v columns of qkv", qkv[:, H:].cpu(), before[:, H:].cpu())


@pytest.mark.parametrize("splits", [1, 3, 4, 6])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n_heads,head_dim", ROPE_SHAPES[:3])
def test_rope_kv_slabs(lib, n_heads, head_dim, dtype, splits):
    """rope_kv_segs_slab_kernel: the slabs summed in ascending order in fp32 (numpy's sequential float32 sum is that order), rounded to 16 bits, then
    rotated -- the same assertions, and bit-identical to the non-slab call on the pre-summed, pre-rounded qkv."""
    S = Segs("ragged5")
    sg, td, H, layer = S.sg, TD[dtype], n_heads * head_dim, 1
    slabs, summed = SC.rope_slabs("ragged5", n_heads, head_dim, dtype, splits)
    d_slabs = torch.from_numpy(slabs).cuda()
    qkv = _poisoned((sg["total_tok"], 3 * H), td)
    S.kc, S.vc = _caches(sg, H, td), _caches(sg, H, td)
    cos, sin = (torch.from_numpy(t).cuda() for t in SC.rope_tables(head_dim))
    loff = layer * SC.MAX_SLOTS * H * 2
    tail = (cos.data_ptr(), sin.data_ptr(), loff, n_heads, head_dim, SC.MAX_POS, _lib.dtype_code(td))
    _lib.check(lib.atspeed_segs_rope_kv(qkv.data_ptr(), d_slabs.data_ptr(), splits, *tail, *S.args(), _st()))
    torch.cuda.synchronize()
    _check_rope(sg, "rope slabs", dtype, n_heads, head_dim, layer, summed, qkv, S.kc, S.vc)
    assert (_bits(qkv[:, H:]).cpu().numpy() == POISON16).all(), "the slab form writes only the q columns of qkv"
    S2 = Segs("ragged5")
    S2.kc, S2.vc = _caches(sg, H, td), _caches(sg, H, td)
    qkv2 = torch.from_numpy(summed).to(td).cuda()
    _lib.check(lib.atspeed_segs_rope_kv(qkv2.data_ptr(), None, 0, *tail, *S2.args(), _st()))
    torch.cuda.synchronize()
    assert_same("slab form q vs separate pass", qkv[:, :H].cpu(), qkv2[:, :H].cpu())
    for i in range(sg["n"]):
        assert_same(f"slab form k cache {i}", S.kc[i].view(-1, H).cpu(), S2.kc[i].view(-1, H).cpu())
        assert_same(f"slab form v cache {i}", S.vc[i].view(-1, H).cpu(), S2.vc[i].view(-1, H).cpu())


# ------------------------------------------------------------------ c. multi-segment attention
# |err| <= c * eps * sum_s p_s |v_s| per element, eps = 2^-8 (bf16) / 2^-11 (fp16) / 2^-24 (fp32): c per kernel form = twice the worst ratio measured
# against the fp64 reference on these cases (profiles/segs_attention_error.txt), capped at 8
# (measured worst ratios: rows32 1.43, rows16 1.13, staged16 1.195 (on the build before the attention refactor), scalar16 0.82, scalar32 6.23 -- the fp32 scalar kernel's fast exponential and sequential
# fp32 sums over up to 200 slots are several fp32 roundings against an eps of ONE fp32 rounding; twice its ratio exceeds the cap, so it stands at 8)
ATTN_C = {"rows32": 2.86, "rows16": 2.26, "staged16": 2.39, "scalar16": 1.64, "scalar32": 8.0}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -24}


def _form16(n_qtiles, n_heads, qtile, head_dim=64, vis_words=SC.VIS_WORDS):
    """which 16-rows-per-wave kernel a launch takes (attn.hip, ats_tree_attention_segs): the LDS-DMA ring up to 256 workgroups and 128-row tiles
    while its four K / V tiles and the tile's visibility words fit the kernel's dynamic LDS (AttnTile<DH>::lds_ring <= kAttnLdsCap: head_dim 128
    at 128-row tiles up to 23 words), else the register-staged form.  Bit-identity between the lock-step launch and the per-segment launches is
    asserted only where both take the same."""
    tile = 64 * head_dim * 2 + 64 * (head_dim * 2 + 32)             # AttnTile<DH>::TILE: a K tile and a V tile of padded rows
    ring_lds = 4 * tile + qtile * vis_words * 8
    return "ring" if qtile <= 128 and n_qtiles * n_heads <= 256 and ring_lds <= 160 * 1024 - 64 else "staged"


def _attention(lib, S, q, H, n_heads, head_dim, td, layer, qtile, rpw, packed, rows_extra=3, max_slots=SC.MAX_SLOTS, vis_words=SC.VIS_WORDS):
    sg = S.sg
    T = sg["total_tok"]
    Tp = (T + 1) // 2 * 2
    out = _poisoned((Tp + rows_extra, H), td)
    loff = layer * max_slots * H * q.element_size()
    _lib.check(lib.atspeed_segs_tree_attention(q.data_ptr(), 3 * H, loff, vis_words, out.data_ptr(), H, n_heads, head_dim, _lib.dtype_code(td), qtile, rpw,
                                               packed, *S.args(), _st()))
    torch.cuda.synchronize()
    return out


def _check_attention(lib, seg_name, n_heads, head_dim, dtype, layer, qtile, rpw, packed, form, max_slots=SC.MAX_SLOTS, vis_words=SC.VIS_WORDS, case=None):
    """case (tests/test_attn_long_gpu.py): a dict in place of the fixture of tests/segs_cases.py -- S (the device side of its table), q, kc, vc
    (numpy, values of the format), ref, mag, victim, blind (bool per row: the rows that see nothing, which must be exact zeros and stay out of
    the ratio) and, where the bound on the ratio is not ATTN_C[form], c.  Returns the worst ratio and the output."""
    S = Segs(seg_name) if case is None else case["S"]
    sg, td, H, T = S.sg, TD[dtype], n_heads * head_dim, S.sg["total_tok"]
    if case is None:
        q64, kc64, vc64 = SC.attn_inputs(seg_name, n_heads, head_dim, dtype)
        ref, mag = SC.attn_ref64(seg_name, n_heads, head_dim, dtype, layer)
        blind, bound, victim = np.zeros(T, dtype=bool), ATTN_C[form], 2 if seg_name == "ragged5" else 11
    else:
        q64, kc64, vc64, ref, mag, blind, victim = (case[k] for k in ("q", "kc", "vc", "ref", "mag", "blind", "victim"))
        bound = case.get("c", ATTN_C[form])
    q = torch.from_numpy(q64).to(td).cuda()
    S.kc, S.vc = _caches(sg, H, td, kc64), _caches(sg, H, td, vc64)
    out = _attention(lib, S, q, H, n_heads, head_dim, td, layer, qtile, rpw, 0, max_slots=max_slots, vis_words=vis_words)
    got = out[:T].double().cpu().numpy()
    err = np.abs(got - ref)
    assert (got[blind] == 0).all(), "a row that sees nothing returns zeros"
    ratio = float((err[~blind] / (EPS[dtype] * mag[~blind])).max())
    print(f"segs attention {seg_name} heads={n_heads} dh={head_dim} {dtype} layer={layer} qtile={qtile} rows_per_wave={rpw} form={form}: "
          f"max|err|={err.max():.3e} worst |err| / (eps sum p|v|) = {ratio:.3f}")
    # 1. the project's tolerance for this operation on unit-normal inputs; 2. the scale-aware bound
    assert err.max() <= (2e-5 if dtype == "fp32" else 3e-2)
    assert ratio <= bound, (ratio, bound)
    # 5. rows past total_tok keep their poison
    assert_same("rows past total_tok", out[T:].cpu(), _poisoned((out.shape[0] - T, H), td).cpu())
    # 3. the lock-step launch equals one launch per segment with the same tiling (the same kernel on the same tiles)
    if dtype == "bf16" and qtile:
        esz = 2
        same_form = rpw == 32 or all(_form16(sum((t + qtile - 1) // qtile for t in sg["n_tok"]), n_heads, qtile, head_dim, vis_words) ==
                                     _form16((t + qtile - 1) // qtile, n_heads, qtile, head_dim, vis_words) for t in sg["n_tok"])
        if same_form:
            one = torch.zeros(T, H, dtype=td, device="cuda")
            for i in range(sg["n"]):
                r0, t = int(sg["row0"][i]), sg["n_tok"][i]
                _lib.check(lib.atspeed_tree_attention_tiled(q.data_ptr() + r0 * 3 * H * esz, 3 * H, S.kc[i][layer].data_ptr(), S.vc[i][layer].data_ptr(),
                                                            S.vis[i].data_ptr(), vis_words, one.data_ptr() + r0 * H * esz, t, sg["n_slots"][i], n_heads, head_dim,
                                                            _lib.ATSPEED_BF16, qtile, rpw, _st()))
            torch.cuda.synchronize()
            assert_same("lock-step vs one launch per segment", out[:T].cpu(), one.cpu())
    # 4. packed output = atspeed_pack_rows of the row-major output; the pad row of an odd total_tok is not written
    if packed:
        pk = _attention(lib, S, q, H, n_heads, head_dim, td, layer, qtile, rpw, 1, rows_extra=2, max_slots=max_slots, vis_words=vis_words)
        Tp = (T + 1) // 2 * 2
        want = torch.empty(Tp, H, dtype=td, device="cuda")
        _lib.check(lib.atspeed_pack_rows(out[:T].contiguous().data_ptr(), want.data_ptr(), T, H * 2, _st()))
        torch.cuda.synchronize()
        gb, wb = pk[:Tp].contiguous().view(torch.uint8).reshape(-1), want.view(torch.uint8).reshape(-1).clone()
        if T & 1:
            pad = guard.packed_row_offsets(T, H * 2).cuda()
            assert (gb[pad].view(torch.int16) == POISON16).all(), "the pad row of the packed output was written"
            wb[pad] = gb[pad]
        assert torch.equal(gb, wb), "packed output differs from atspeed_pack_rows of the row-major output"
        assert (_bits(pk[Tp:]) == POISON16).all()
    # 5. another segment's cache filled with large finite values changes no bit of the other segments' rows
    big = 3.0e38 if dtype != "fp16" else 60000.0
    S.kc[victim], S.vc[victim] = torch.full_like(S.kc[victim], big), torch.full_like(S.vc[victim], -big)
    out2 = _attention(lib, S, q, H, n_heads, head_dim, td, layer, qtile, rpw, 0, max_slots=max_slots, vis_words=vis_words)
    keep = np.ones(T, dtype=bool)
    keep[sg["row0"][victim]: sg["row0"][victim + 1]] = False
    keep = torch.from_numpy(keep).cuda()
    assert_same("rows of the other segments", out2[:T][keep].cpu(), out[:T][keep].cpu())
    return ratio, out


@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("rpw", [16, 32])
@pytest.mark.parametrize("qtile", [64, 128])
@pytest.mark.parametrize("n_heads,head_dim", [(4, 64), (2, 128)])
def test_tree_attention_segs(lib, n_heads, head_dim, qtile, rpw, layer, packed):
    """ats_tree_attention_segs in its lock-step form on ragged5: five segments with their own caches, n_slots and visibility words, row0 != 0, ragged
    last tiles (63 / 65 / 130 rows), the qtile_seg / qtile_idx lookup, a layer offset, the packed output o_proj reads -- per element against the fp64
    softmax attention of each segment over its own cache."""
    _check_attention(lib, "ragged5", n_heads, head_dim, "bf16", layer, qtile, rpw, packed, "rows32" if rpw == 32 else "rows16")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_tree_attention_segs_scalar(lib, dtype):
    """tree_attn_kernel<T> (head_dim 32: no MFMA form) over the same segments"""
    _check_attention(lib, "ragged5", 4, 32, dtype, 1, 0, 0, 0, "scalar32" if dtype == "fp32" else "scalar16")


@pytest.mark.parametrize("n_heads,head_dim,qtile", [(33, 64, 64), (43, 64, 128), (43, 128, 128)], ids=["64x4w", "64x8w", "128x8w"])
def test_tree_attention_segs_staged(lib, n_heads, head_dim, qtile):
    """the register-staged 16-rows-per-wave form at 64- and 128-row tiles, which only grids above 256 workgroups take (attn.hip,
    ats_tree_attention_segs): ragged5 has 8 tiles of 64 rows and 6 of 128, so 33 and 43 heads give 264 and 258 workgroups.  (Its 256-row tile,
    and head_dim 128 at 64-row tiles, are reached by test_kernels_gpu.py::test_tree_attention_every_tiling.)"""
    _check_attention(lib, "ragged5", n_heads, head_dim, "bf16", 1, qtile, 16, 1, "staged16")


def test_tree_attention_segs_many32(lib):
    """32 segments of 9-30 rows, everything automatic: ats_seg_finish's `n >= 16` rule gives 128-row tiles, and 32 tiles x 16 heads = 512 workgroups the
    32-rows-per-wave kernel"""
    _check_attention(lib, "many32", 16, 64, "bf16", 1, 0, 0, 1, "rows32")


# ------------------------------------------------------------------ d. residual + norm tail
def _counters(lib, reset=False):
    out = (C.c_int64 * 16)()
    lib.atspeed_gemm_path_counters(out, 16, 1 if reset else 0)
    return list(out)


def _pack(lib, t):
    rows, rb = t.shape[0], t.shape[1] * t.element_size()
    dst = torch.zeros((rows + 1) // 2 * 2, t.shape[1], dtype=t.dtype, device="cuda")
    _lib.check(lib.atspeed_pack_rows(t.contiguous().data_ptr(), dst.data_ptr(), rows, rb, _st()))
    return dst


def _unpack(lib, t, rows):
    dst = torch.zeros(rows, t.shape[1], dtype=t.dtype, device="cuda")
    _lib.check(lib.atspeed_unpack_rows(t.data_ptr(), dst.data_ptr(), rows, t.shape[1] * t.element_size(), _st()))
    return dst


def _check_xn(name, xn, h, nw, eps, dtype):
    """xn against the fp64 norm of the h the call STORED (the kernel takes its statistics from the stored, rounded h): round(w * round(h * rs))"""
    inner, outer, alt = SC.norm_ref64(h.double().cpu().numpy(), nw.double().cpu().numpy(), eps, dtype)
    got = xn.double().cpu().numpy()
    if dtype == "fp32":
        # fp32 results are not rounded to a coarser format: the bound is the worst case of the fp32 evaluation -- the sum of squares (8 sequential
        # terms per thread, 6 shuffle steps, 16 partials: 30 roundings, halved by the square root), the mean, eps, rsqrt and two products: 24 x 2^-24
        assert (np.abs(got - outer) <= 24 * 2.0 ** -24 * np.abs(outer)).all(), (name, float((np.abs(got - outer) / np.abs(outer)).max()))
        return
    # first step h * rs: near ties at rounding.REL (alt = the continuation from the other neighbour); second step w * round(.): a product of two
    # 16-bit values, exact in fp32, so no tolerance at all
    R.assert_rounded(got, outer, dtype, rel=0, cap=R.CAP, alt64=alt, name=name)


CASES_16 = [(f, m, n, k, dt, pk) for (f, m, n, k) in SC.RESID_NORM_16 for dt in ("bf16", "fp16") for pk in ((0, 1) if n % 32 == 0 else (0,))]
CASES_32 = [("tiled", 8, n, 512, "fp32", 0) for n in SC.NORM_N]


@pytest.mark.parametrize("form,m,n,k,dtype,packed", CASES_16 + CASES_32)
def test_gemm_resid_norm(lib, form, m, n, k, dtype, packed):
    """ats_gemm_resid_norm: every GEMM form that leaves slabs or applies the residual itself (the smallest shapes plan_gemm gives each, the path
    asserted) x the tail's forms -- NPT 4 / 8 (n <= 4096 / <= 8192), V = 1 (n = 1002), the unfused norm kernels (n = 8200, and behind the plain ring
    kernel), packed xn.  h equals atspeed_gemm(epilogue 2) bit for bit; xn is the fp64 norm of that stored h; nothing outside h [m][n], xn and the
    workspace is written."""
    td, code = TD[dtype], _lib.dtype_code(TD[dtype])
    a, w, r, nw = SC.resid_inputs(m, n, k, dtype)
    fused = form != "ring" and n <= 8192                      # the norm kernels behind the GEMM read h densely: a row gap only where the reduce pass is fused
    eps, ldh, ws_bytes = 1e-5, n + 8 if fused else n, 64 << 20
    if dtype == "fp32":
        assert form == "tiled"
    ar = guard.Arena("cuda", seed=m + n)
    nwv = ar.input("norm_w", nw)
    if packed:
        av, wv = _pack(lib, a.cuda()), _pack(lib, w.cuda())
        a_ptr, w_ptr, lda = av.data_ptr(), wv.data_ptr(), k
    else:
        avv, wvv = ar.input("a", a, ld=k + 8), ar.input("w", w)
        a_ptr, w_ptr, lda = avv.ptr, wvv.ptr, k + 8
    hv = ar.output("h", m, n, td, ld=ldh, init=r)
    xrows = (m + 1) // 2 * 2 if packed else m
    xv = ar.output("xn", xrows, n, td)
    wsv = ar.workspace("workspace", ws_bytes, halo_bytes=4 * m * n)
    ar.snapshot()
    _counters(lib, reset=True)
    _lib.check(lib.atspeed_gemm_resid_norm(a_ptr, w_ptr, hv.ptr, m, n, k, lda, ldh, code, nwv.ptr, xv.ptr, eps, wsv.ptr, ws_bytes, packed, _st()))
    torch.cuda.synchronize()
    cnt = _counters(lib)
    assert cnt[SC.PATH_OF_FORM[form]] == 1 and sum(cnt) == 1, (form, cnt)
    if packed and m & 1:                                       # the pad row of a packed xn is not written
        xv.add_guard(guard.packed_row_offsets(m, n * 2))
    ar.check()
    # 1. h: the same plan, slabs and sum order as the plain residual GEMM
    h2 = r.clone().cuda()
    ws2 = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    if packed:                                                 # (packed operands give the row-major call's bits: test_gemm_packed_equals_row_major_bit_for_bit)
        ad, wd = a.cuda(), w.cuda()
        a_ptr, w_ptr, lda = ad.data_ptr(), wd.data_ptr(), k
    _lib.check(lib.atspeed_gemm(a_ptr, w_ptr, h2.data_ptr(), m, n, k, lda, n, code, 2, ws2.data_ptr(), ws_bytes, _st()))
    torch.cuda.synchronize()
    h = hv.t.clone()
    assert_same("h vs atspeed_gemm epilogue 2", h.cpu(), h2.cpu())
    # 2. xn from the stored h
    xn = _unpack(lib, xv.t.contiguous(), m) if packed else xv.t
    _check_xn(f"xn {form} {m}x{n}x{k} {dtype} packed={packed}", xn, h, nw, eps, dtype)


def _fp8_operands(lib, m, n, k, dtype, packed=0):
    a, w, r, nw = SC.resid_inputs(m, n, k, "bf16")            # the e4m3 quantiser's entry point reads bf16
    xq, wq = torch.empty(m, k, dtype=torch.uint8, device="cuda"), torch.empty(n, k, dtype=torch.uint8, device="cuda")
    sx, sw = torch.empty(m, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    ad, wd = a.cuda(), w.cuda()
    if packed:                                                # (m, n even here: no pad rows)
        _lib.check(lib.atspeed_quant_rows_fp8_packed(_pack(lib, ad).data_ptr(), m, k, xq.data_ptr(), sx.data_ptr(), _st()))
        _lib.check(lib.atspeed_quant_rows_fp8_packed(_pack(lib, wd).data_ptr(), n, k, wq.data_ptr(), sw.data_ptr(), _st()))
    else:
        _lib.check(lib.atspeed_quant_rows_fp8(ad.data_ptr(), m, k, xq.data_ptr(), sx.data_ptr(), _st()))
        _lib.check(lib.atspeed_quant_rows_fp8(wd.data_ptr(), n, k, wq.data_ptr(), sw.data_ptr(), _st()))
    torch.cuda.synchronize()
    return xq, sx, wq, sw, wd, r.to(TD[dtype]), nw.to(TD[dtype])


def _e4m3_ref(xn, s):
    """the e4m3 bytes of xn [m][n] with per-row scales s, on the CPU: e4m3(clamp(x * (1 / s), +-448)) in float32, nearest even (torch's cast)"""
    y = (xn.float().cpu() * (1.0 / s.float().cpu())[:, None]).clamp(-448.0, 448.0)
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def _check_quant_tail(lib, name, call, m, n, dtype, r, nw, eps, fused, h_check=None):
    """the assertions on a W8A8 / W4A8 residual projection.  call(h, ldh, xn, q, s, ws, ws_bytes) makes the call; `fused`: the reduce pass carries
    the norm (h may then have a row gap).  Returns the h, xn, q_out, s_out of the guarded call and its workspace view."""
    td, ws_bytes = TD[dtype], 64 << 20
    ldh = n + 8 if fused else n
    ar = guard.Arena("cuda", seed=n)
    hv = ar.output("h", m, n, td, ld=ldh, init=r)
    xv, qv, sv = ar.output("xn", m, n, td), ar.output("q_out", m, n, torch.uint8), ar.output("s_out", 1, m, torch.float32)
    wsv = ar.workspace("workspace", ws_bytes, halo_bytes=4 * m * n)
    ar.snapshot()
    call(hv.ptr, ldh, xv.ptr, qv.ptr, sv.ptr, wsv.ptr, ws_bytes)
    ar.check()                                                # h's row gap and rows >= m, xn, q_out, s_out and the workspace: nothing outside them written
    h = hv.t.clone()
    if h_check is not None:
        h_check(h)
    _check_xn(name, xv.t, h, nw, eps, dtype)
    # s_out: the scale rule in float32; q_out: an e4m3 reference of the CPU's on the xn the same call wrote (both 16-bit types), and for bf16 the
    # project's own quantiser too
    amax = xv.t.float().abs().amax(1).cpu().numpy()
    want = np.where(amax > 0, amax * np.float32(1.0 / 448.0), np.float32(1)).astype(np.float32)
    assert np.array_equal(sv.t.cpu().numpy()[0], want)
    assert_same(f"{name} q_out vs e4m3(xn / s_out) on the CPU", qv.t.cpu(), _e4m3_ref(xv.t, sv.t[0]))
    if dtype == "bf16":
        q2, s2 = torch.empty(m, n, dtype=torch.uint8, device="cuda"), torch.empty(m, dtype=torch.float32, device="cuda")
        _lib.check(lib.atspeed_quant_rows_fp8(xv.t.contiguous().data_ptr(), m, n, q2.data_ptr(), s2.data_ptr(), _st()))
        torch.cuda.synchronize()
        assert_same(f"{name} q_out vs atspeed_quant_rows_fp8(xn)", qv.t.cpu(), q2.cpu())
        assert_same(f"{name} s_out", sv.t.cpu(), s2[None].cpu())
    # without q_out: the same xn; without xn (where the e4m3 form does not need it): the same q_out / s_out
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

    def run(xn, q, s):
        h_ = r.clone().cuda()
        call(h_.data_ptr(), n, xn, q, s, ws.data_ptr(), ws_bytes)
        return h_
    x3 = torch.empty(m, n, dtype=td, device="cuda")
    h3 = run(x3.data_ptr(), None, None)
    assert_same(f"{name} xn of a call without q_out", x3.cpu(), xv.t.cpu())
    assert_same(f"{name} h of a call without q_out", h3.cpu(), h.cpu())
    q4, s4 = torch.empty(m, n, dtype=torch.uint8, device="cuda"), torch.empty(1, m, dtype=torch.float32, device="cuda")
    if n <= 8192:
        run(None, q4.data_ptr(), s4.data_ptr())
        assert_same(f"{name} q_out of a call without xn", q4.cpu(), qv.t.cpu())
        assert_same(f"{name} s_out of a call without xn", s4.cpu(), sv.t.cpu())
    else:   # beyond the norm + e4m3 kernel's 8192 columns the e4m3 rows are made from xn: a call without xn is refused before it writes anything
        h5 = r.clone().cuda()
        with pytest.raises(_lib.AtSpeedError):
            call(h5.data_ptr(), n, None, q4.data_ptr(), s4.data_ptr(), ws.data_ptr(), ws_bytes)
        torch.cuda.synchronize()
        assert_same(f"{name} h of a refused call", h5.cpu(), r.cpu())
    return h, xv.t, qv.t, sv.t, wsv


def _fp8_h_check(name, xq, sx, wq, sw, r, k, dtype):
    """h of the W8A8 projection against r + the dequantised product in fp64.  Two roundings to the 16-bit type, each half an ulp (2^-8 of the value
    in bf16, 2^-11 in fp16): the projection's, then the sum's; the fp32 accumulation of k products at its worst case, k 2^-24 of sum |x w|."""
    deq = lambda q, s_: q.cpu().view(torch.float8_e4m3fn).double() * s_.cpu().double()[:, None]
    x64, w64 = deq(xq, sx), deq(wq, sw)
    proj, mag = x64 @ w64.T, (x64.abs().float() @ w64.abs().float().T).double() * (1 + 2.0 ** -10)      # (mag: a bound's factor, float32 will do)
    ref = r.double() + proj
    u = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    tol = u * (proj.abs() + ref.abs()) * (1 + 2 * u) + k * 2.0 ** -24 * mag

    def check(h):
        err = (h.double().cpu() - ref).abs()
        assert bool((err <= tol).all()), (name, float((err / tol).max()))
    return check


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k", [(8, 768, 1024), (8, 4096, 1024), (8, 4104, 1024), (8, 8192, 1024), (8, 8200, 1024), (300, 4096, 4096)])
def test_gemm_fp8_resid_norm(lib, m, n, k, dtype):
    """ats_gemm_fp8_resid_norm: the QUANT form of the tail behind the W8A8 weight-streaming split (NPT 4 / 8) and the ring kernel cut in K, and the
    8200-column case where no fused form exists.  Found here: with q_out and more than 8192 columns the call used to be refused by the norm + e4m3
    kernel AFTER the GEMM had updated h; it now makes the e4m3 rows from xn, and is refused up front when xn is missing.  Found here too (300 x 4096
    x 4096 in fp16): the tail with and without the e4m3 rows gave xn that differed in isolated elements -- in the fp16 build the compiler had folded
    h * rs and its rounding into one v_fma_mixlo_f16 in one instantiation and kept v_mul_f32 + v_cvt_f16_f32 in the other; the norm kernels now
    share common.h norm_scale, which keeps the fp32 product apart from its conversion."""
    xq, sx, wq, sw, _, r, nw = _fp8_operands(lib, m, n, k, dtype)
    eps, code, nwd = 1e-5, _lib.dtype_code(TD[dtype]), nw.cuda()

    def call(h, ldh, xn, q, s, ws, ws_bytes):
        _lib.check(lib.atspeed_gemm_fp8_resid_norm(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), h, m, n, k, ldh, code, nwd.data_ptr(),
                                                   xn, q, s, eps, ws, ws_bytes, 0, _st()))
        torch.cuda.synchronize()
    _counters(lib, reset=True)
    h, *_ = _check_quant_tail(lib, f"fp8 {m}x{n}x{k} {dtype}", call, m, n, dtype, r, nw, eps, fused=n <= 8192,
                              h_check=_fp8_h_check(f"fp8 h {m}x{n}x{k} {dtype}", xq, sx, wq, sw, r, k, dtype))
    cnt = _counters(lib)
    assert cnt[11 if m > 256 else 8] == sum(cnt) and sum(cnt) >= 2, cnt
    if dtype == "bf16":                                       # h: the same slabs and sum order as atspeed_gemm_fp8's residual epilogue
        h2, ws = r.clone().cuda(), torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        _lib.check(lib.atspeed_gemm_fp8(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), h2.data_ptr(), m, n, k, n, 2, ws.data_ptr(), ws.numel(), _st()))
        torch.cuda.synchronize()
        assert_same("h vs atspeed_gemm_fp8 epilogue 2", h.cpu(), h2.cpu())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [4096, 8256])
def test_gemm_fp8_resid_norm_packed(lib, n, dtype):
    """packed = 1: xq, wq, xn and q_out in the packed operand layout, behind the fused QUANT tail (4096 columns) and behind the norm kernels + the
    quantiser (8256 > 8192 columns).  Every output equals atspeed_pack_rows of the row-major call's; for bf16 q_out / s_out also equal
    atspeed_quant_rows_fp8_packed of the packed xn."""
    m, k, eps, code, ws_bytes = 8, 1024, 1e-5, _lib.dtype_code(TD[dtype]), 64 << 20
    outs = []
    for pk in (0, 1):
        xq, sx, wq, sw, _, r, nw = _fp8_operands(lib, m, n, k, dtype, packed=pk)
        nwd = nw.cuda()
        ar = guard.Arena("cuda", seed=n + pk)
        hv = ar.output("h", m, n, TD[dtype], init=r)
        xv, qv, sv = ar.output("xn", m, n, TD[dtype]), ar.output("q_out", m, n, torch.uint8), ar.output("s_out", 1, m, torch.float32)
        wsv = ar.workspace("workspace", ws_bytes, halo_bytes=4 * m * n)
        ar.snapshot()
        _lib.check(lib.atspeed_gemm_fp8_resid_norm(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), hv.ptr, m, n, k, n, code, nwd.data_ptr(),
                                                   xv.ptr, qv.ptr, sv.ptr, eps, wsv.ptr, ws_bytes, pk, _st()))
        torch.cuda.synchronize()
        ar.check()
        outs.append((hv.t.clone(), xv.t.clone(), qv.t.clone(), sv.t.clone()))
    (h0, x0, q0, s0), (h1, x1, q1, s1) = outs
    assert_same("h packed vs row-major", h1.cpu(), h0.cpu())
    assert_same("s_out packed vs row-major", s1.cpu(), s0.cpu())
    assert_same("xn packed vs atspeed_pack_rows(row-major xn)", x1.cpu(), _pack(lib, x0).cpu())
    assert_same("q_out packed vs atspeed_pack_rows(row-major q_out)", q1.cpu(), _pack(lib, q0).cpu())
    if dtype == "bf16":
        q2, s2 = torch.empty(m, n, dtype=torch.uint8, device="cuda"), torch.empty(m, dtype=torch.float32, device="cuda")
        _lib.check(lib.atspeed_quant_rows_fp8_packed(x1.contiguous().data_ptr(), m, n, q2.data_ptr(), s2.data_ptr(), _st()))
        torch.cuda.synchronize()
        assert_same("q_out vs atspeed_quant_rows_fp8_packed(xn)", q1.cpu(), q2.cpu())
        assert_same("s_out vs atspeed_quant_rows_fp8_packed(xn)", s1.cpu(), s2[None].cpu())


@pytest.mark.parametrize("fn", ["fp8", "w4a8"])
def test_resid_norm_packed_refused_before_h(lib, fn):
    """Found here: packed e4m3 rows need whole 64-byte blocks (n % 64 == 0); 8224 columns (n % 32 == 0 only) used to be refused by the quantiser
    AFTER the projection had updated h.  The call is now refused before its first launch: h keeps every bit."""
    m, n, k = 8, 8224, 1024
    xq, sx, wq, sw, wd, r, nw = _fp8_operands(lib, m, n, k, "bf16", packed=1)
    if fn == "w4a8":                                          # operands of the size a call that is NOT refused would read: MXFP4 weights and their scales
        wq, sw = torch.empty(n, k // 2, dtype=torch.uint8, device="cuda"), torch.empty(n, k // 32, dtype=torch.uint8, device="cuda")
        _lib.check(lib.atspeed_quant_weights_mxfp4(_pack(lib, wd).data_ptr(), n, k, _lib.ATSPEED_BF16, 1, wq.data_ptr(), sw.data_ptr(), _st()))
    nwd, h = nw.cuda(), r.clone().cuda()
    xn, q, s = torch.empty(m, n, dtype=torch.bfloat16, device="cuda"), torch.empty(m, n, dtype=torch.uint8, device="cuda"), torch.empty(m, dtype=torch.float32, device="cuda")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    f = lib.atspeed_gemm_fp8_resid_norm if fn == "fp8" else lib.atspeed_gemm_w4a8_resid_norm
    with pytest.raises(_lib.AtSpeedError):
        _lib.check(f(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), h.data_ptr(), m, n, k, n, _lib.ATSPEED_BF16, nwd.data_ptr(),
                     xn.data_ptr(), q.data_ptr(), s.data_ptr(), 1e-5, ws.data_ptr(), ws.numel(), 1, _st()))
    torch.cuda.synchronize()
    assert_same("h of a refused call", h.cpu(), r.cpu())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [768, 4096, 4104, 8192, 8200])
def test_gemm_w4a8_resid_norm(lib, n, dtype):
    """ats_gemm_w4a8_resid_norm: the same tail behind the W4A8 kernel's split form, on both sides of the NPT 4 / 8 boundary (4096 / 4104), at the
    last fused width (8192) and beyond it (8200: the projection runs unsplit, the norm kernels follow)"""
    m, k = 8, 2048
    xq, sx, _, _, wd, r, nw = _fp8_operands(lib, m, n, k, dtype)
    wq, wsc = torch.empty(n, k // 2, dtype=torch.uint8, device="cuda"), torch.empty(n, k // 32, dtype=torch.uint8, device="cuda")
    _lib.check(lib.atspeed_quant_weights_mxfp4(wd.data_ptr(), n, k, _lib.ATSPEED_BF16, 0, wq.data_ptr(), wsc.data_ptr(), _st()))
    eps, code, nwd = 1e-5, _lib.dtype_code(TD[dtype]), nw.cuda()

    def call(h, ldh, xn, q, s, ws, ws_bytes):
        _lib.check(lib.atspeed_gemm_w4a8_resid_norm(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), wsc.data_ptr(), h, m, n, k, ldh, code,
                                                    nwd.data_ptr(), xn, q, s, eps, ws, ws_bytes, 0, _st()))
        torch.cuda.synchronize()
    _counters(lib, reset=True)
    h, _, _, _, wsv = _check_quant_tail(lib, f"w4a8 {m}x{n}x{k} {dtype}", call, m, n, dtype, r, nw, eps, fused=n <= 8192)
    cnt = _counters(lib)
    assert cnt[12] == sum(cnt) and sum(cnt) >= 2, cnt           # the W4A8 kernel, every call
    # the split form leaves its slabs in the workspace (then the fused tail ran: h had a row gap, which the norm kernels refuse); the unsplit one
    # beyond 8192 columns does not touch it
    assert torch.equal(wsv.buf, wsv.saved) == (n > 8192)
    h2 = r.clone().cuda()
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    # (beyond 8192 columns, where the slabs could not be summed by the fused tail, the projection runs unsplit: the plain call without a workspace)
    ws2, ws2_bytes = (ws.data_ptr(), ws.numel()) if n <= 8192 else (None, 0)
    _lib.check(lib.atspeed_gemm_w4a8(xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), wsc.data_ptr(), h2.data_ptr(), m, n, k, n, 2, code, 0, ws2, ws2_bytes, _st()))
    torch.cuda.synchronize()
    assert_same("h vs atspeed_gemm_w4a8 epilogue 2", h.cpu(), h2.cpu())
