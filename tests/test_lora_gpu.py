"""The unmerged LoRA target on the GPU (atspeed_llama_set_lora): the two kernels alone through their entry points against
the fp64 restatement of their rule (tests/lora_ref.py), then whole forwards and decodes of adapted models against the LoRA reference --
fp32 at the existing 1e-3 bar, bf16 / fp16 at the Llama-7B width at the existing 16-bit bar, W8A8 and W4A8 bases at their tests' own bars --
and the on / off switch.  Every comparison with an adapter first asserts, on the CPU side, that the adapter changes what is compared: a run
that ignores the adapter cannot pass.  Run with -m gpu on the MI355X box."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import atspeed_amd
from atspeed_amd import _lib, lora as L, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, last_trace, release_decoders, target_generate
from atspeed_amd.model import HipLlama, vis_bits_from_bool
from oracle import beamsd_ref as R
from oracle.llama_ref import RefLlama
from tests import guard, lora_ref as LR, segs_cases as SC
from tests.golden.cases import CASES, build_case_inputs
from tests.guard import assert_same

TD = SC.TORCH
SCORE_TOL = 1e-3                                   # the fp32 bar (tests/test_bssd_gpu.py, BASELINE north star)
BF16_MAX_TOL, BF16_MEAN_TOL = 0.04, 0.006          # the 16-bit bar (tests/test_fulldims_gpu.py), relative to max |logit|
FP8_VS_NOISE = 0.85                                # the quantised-base bar (tests/test_fp8_gpu.py, tests/test_fp4_gpu.py)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _st():
    return _lib.stream_ptr()


def _fmt(x, dtype):
    """fp values -> (values of the format as fp64 numpy, the device tensor's CPU twin)"""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(TD[dtype])
    return t.double().numpy(), t


# ------------------------------------------------------------------ 1. the shrink kernel alone
SHRINK_ROWS = (1, 17, 64, 130)                     # one partly filled 16-row workgroup, 16 + 1, four whole ones, 8 + a tail


def _a_cat(rng, rank, hidden, dtype, modules=("q", "v")):
    """the library's stacked A: [3 R16][hidden], rows j < rank of an adapted module's third hold values, everything else is zero"""
    r16 = (rank + 15) // 16 * 16
    a = np.zeros((3 * r16, hidden), dtype=np.float32)
    for k, m in enumerate("qkv"):
        if m in modules:
            a[k * r16: k * r16 + rank] = rng.standard_normal((rank, hidden)) / np.sqrt(hidden)
    return r16, a


@pytest.mark.parametrize("rank", [4, 8, 16, 24, 40, 64])
@pytest.mark.parametrize("hidden", [256, 768, 4096])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_lora_shrink_kernel(lib, dtype, hidden, rank):
    """lora_shrink_mfma_kernel<3|6|9|12> (16-bit; every hidden here is a multiple of 128) and lora_shrink_kernel<float>, rows 1 / 17 / 64 / 130:
    within 1/2 ulp16 + H 2^-24 sum|terms| of the fp64 chain on the same values (LR.shrink_ref64 states the bound; it holds for any summation
    order; an element of xn that the fp64 chain rounds at a near tie may be the other neighbour), two runs bit-identical, nothing outside [rows][3 R16] written, inputs untouched, pad columns and the absent module exactly +0."""
    td, code = TD[dtype], _lib.dtype_code(TD[dtype])
    rng = np.random.default_rng(1000 * rank + hidden)
    r16, a32 = _a_cat(rng, rank, hidden, dtype)
    a64, a_t = _fmt(a32, dtype)
    w64, w_t = _fmt(1 + 0.1 * rng.standard_normal(hidden), dtype)
    ties = 0
    for rows in SHRINK_ROWS:
        h64, h_t = _fmt(rng.standard_normal((rows, hidden)) * (0.5 + rng.random((rows, 1)) * 3), dtype)
        ar = guard.Arena("cuda", seed=rows)
        vh, vw, va = ar.input("h", h_t.cuda()), ar.input("norm_w", w_t.cuda()), ar.input("a_cat", a_t.cuda())
        outs = []
        for run in range(2):
            vu = ar.output(f"u{run}", rows, 3 * r16, td)
            outs.append(vu)
        ar.snapshot()
        for vu in outs:
            _lib.check(lib.atspeed_lora_shrink(vh.ptr, vw.ptr, va.ptr, vu.ptr, rows, hidden, 3 * r16, 1e-6, code, _st()))
        torch.cuda.synchronize()
        ar.check()
        assert_same(f"shrink run 2 vs run 1 ({dtype} H={hidden} r={rank} rows={rows})", outs[1].t.cpu(), outs[0].t.cpu())
        got = outs[0].t.double().cpu().numpy()
        ref, bound, n_tie = LR.shrink_ref64(h64, w64, a64, 1e-6, dtype)
        ties += n_tie
        err = np.abs(got - ref)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"shrink {dtype} H={hidden} rank={rank} rows={rows}: worst |err| / bound {worst:.3f}")
        assert (err <= bound).all(), (dtype, hidden, rank, rows, worst, np.argwhere(err > bound)[:3].tolist())
        zero_cols = np.ones(3 * r16, dtype=bool)
        for k in (0, 2):
            zero_cols[k * r16: k * r16 + rank] = False
        bits = outs[0].t.contiguous().view(torch.int32 if dtype == "fp32" else torch.int16).cpu().numpy()
        assert (bits[:, zero_cols] == 0).all(), "a pad column or the absent module's column is not exactly +0"
        assert np.abs(got[:, ~zero_cols]).min() > 0
    share = ties / (sum(SHRINK_ROWS) * hidden)
    assert share <= LR.R.CAP, f"{share:.3%} of xn are near ties of a 16-bit rounding: the case cannot tell a wrong kernel from a tie"


def test_lora_shrink_lane_map_with_exact_integers(lib):
    """the MFMA kernel's operand and accumulator maps, without any tolerance: small integers and a unit norm weight make every product and
    sum exact in bf16 / fp32, so u must equal the integer matrix product bit for bit -- a lane, a k-group or a tile in the wrong place shows.
    Rows hold +-c with c a power of two, so that x * rsqrt(mean x^2) = +-1 up to rsqrt's rounding, which the 16-bit rounding removes."""
    H, rank, rows = 512, 40, 37
    r16 = 48
    rng = np.random.default_rng(5)
    sign = rng.choice([-1.0, 1.0], size=(rows, H))
    h = sign * (2.0 ** rng.integers(-2, 3, size=(rows, 1)))
    a = np.zeros((3 * r16, H))
    for k in range(3):
        a[k * r16: k * r16 + rank] = rng.integers(-1, 2, size=(rank, H))              # -1, 0, 1: sums stay below 2^9, exact in bf16
    for dtype in ("bf16", "fp16"):
        td = TD[dtype]
        u = torch.full((rows, 3 * r16), 777.0, dtype=td, device="cuda")
        dev = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32)).to(td).cuda()
        hd, wd, ad = dev(h), dev(np.ones(H)), dev(a)
        _lib.check(lib.atspeed_lora_shrink(hd.data_ptr(), wd.data_ptr(), ad.data_ptr(), u.data_ptr(), rows, H, 3 * r16, 0.0, _lib.dtype_code(td), _st()))
        want = sign @ a.T
        assert np.abs(want).max() <= 256 and np.array_equal(u.double().cpu().numpy(), want), dtype


# ------------------------------------------------------------------ 2. expand + RoPE + scatter alone
SEG_TOK, SEG_SLOTS = (37, 23), (50, 23)


class TwoSegs:
    """two segments with their own positions (tree tokens: repeats; one beyond the table) and slots (permutations: row != slot)"""

    def __init__(self, H, td):
        rng = np.random.default_rng(77)
        self.n_tok = list(SEG_TOK)
        self.pos = [np.arange(5, 5 + SEG_TOK[0]), np.arange(100, 100 + SEG_TOK[1])]
        self.pos[0][[10, 11, 12]] = 14
        self.pos[1][3] = SC.MAX_POS + 7
        self.slots = [rng.permutation(SEG_SLOTS[0])[: SEG_TOK[0]], rng.permutation(SC.MAX_SLOTS)[: SEG_TOK[1]]]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()
        self.d_pos, self.d_slots = [dev(p) for p in self.pos], [dev(s) for s in self.slots]
        self.H, self.td = H, td
        self.total = sum(self.n_tok)

    def caches(self):
        fill = torch.full((SC.LAYERS, SC.MAX_SLOTS, self.H), 3.0, dtype=self.td, device="cuda")
        return [fill.clone() for _ in range(2)], [fill.clone() for _ in range(2)]

    def args(self, kc, vc):
        arr = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
        cnt = lambda v: (C.c_int32 * 2)(*v)
        self._keep = [None, arr(self.d_pos), arr(self.d_slots), None, arr(kc), arr(vc), cnt(self.n_tok), cnt(SEG_SLOTS), cnt([0, 0])]
        return [2] + self._keep

    def all_pos(self):
        return np.concatenate(self.pos)

    def gather(self, caches, layer):
        """the cache rows the tokens named, in row order: [total][H] fp64"""
        return np.concatenate([caches[i][layer].double().cpu().numpy()[self.slots[i]] for i in range(2)])


@pytest.mark.parametrize("modules", [("q", "v"), ("q", "k", "v"), ("v",)], ids=lambda m: "".join(m))
@pytest.mark.parametrize("n_heads,head_dim,r16,scaling", [(12, 64, 16, 2.0), (32, 128, 48, 0.5)])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_lora_rope_kv_kernel(lib, dtype, n_heads, head_dim, r16, scaling, modules):
    """lora_rope_kv_segs_vec_kernel (16-bit) / lora_rope_kv_segs_kernel<float> at layer 1 of two segments.  Without any tolerance: with B = 0 the
    q columns and both caches equal atspeed_segs_rope_kv's bit for bit, and with a real B every module that is NOT adapted still does.  The
    adapted modules: within the bound of LR.expand_ref64 (continued from the u this call was given; scaling is a power of two, so that the
    scaled product is exact and the bound's steps are the rule's roundings alone), carried through the rotation -- |c| e0 + |s| e1, the fp32
    evaluation of the pair (SC.ROPE_REL of its operands) and the rotated value's own half ulp.  fp32 has no 16-bit steps; its bound keeps the
    sums' fp32 terms and 2^-23 of |base| + |scaling d| for the two fp32 operations of the add."""
    td, code, H, layer = TD[dtype], _lib.dtype_code(TD[dtype]), n_heads * head_dim, 1
    S = TwoSegs(H, td)
    T = S.total
    rng = np.random.default_rng(31 * n_heads + len(modules))
    qkv64, qkv_t = _fmt(rng.standard_normal((T, 3 * H)), dtype)
    u32 = np.zeros((T, 3 * r16), dtype=np.float32)
    rank = r16 - 8                                                        # pad columns of u and B are zero, as the library lays them out
    for k in range(3):
        u32[:, k * r16: k * r16 + rank] = rng.standard_normal((T, rank))
    u64, u_t = _fmt(u32, dtype)
    b64, b_dev = {}, {}
    for m in "qkv":
        b32 = np.zeros((H, r16), dtype=np.float32)
        b32[:, :rank] = rng.standard_normal((H, rank)) * 0.3
        b64[m], t = _fmt(b32, dtype)
        b_dev[m] = t.cuda()
    zero_b = torch.zeros(H, r16, dtype=td, device="cuda")
    cos, sin = (torch.from_numpy(t).cuda() for t in SC.rope_tables(head_dim))
    loff = layer * SC.MAX_SLOTS * H * qkv_t.element_size()
    tail = (cos.data_ptr(), sin.data_ptr(), loff, n_heads, head_dim, SC.MAX_POS, code)
    u_dev = u_t.cuda()

    def run(bs):
        q = qkv_t.clone().cuda()
        kc, vc = S.caches()
        if bs is None:
            _lib.check(lib.atspeed_segs_rope_kv(q.data_ptr(), None, 0, *tail, *S.args(kc, vc), _st()))
        else:
            ptr = [b.data_ptr() if b is not None else None for b in bs]
            _lib.check(lib.atspeed_segs_lora_rope_kv(q.data_ptr(), u_dev.data_ptr(), *ptr, r16, scaling, *tail, *S.args(kc, vc), _st()))
        torch.cuda.synchronize()
        return q, kc, vc

    plain = run(None)
    zero = run([zero_b if m in modules else None for m in "qkv"])
    real = run([b_dev[m] if m in modules else None for m in "qkv"])
    for name, other in (("B = 0", zero), ("real B", real)):
        mods = "qkv" if name == "B = 0" else [m for m in "qkv" if m not in modules]
        assert_same(f"{name}: k and v columns of qkv", other[0][:, H:].cpu(), qkv_t[:, H:])
        if "q" in mods:
            assert_same(f"{name}: q", other[0][:, :H].cpu(), plain[0][:, :H].cpu())
        for m, idx in (("k", 1), ("v", 2)):
            if m in mods:
                for i in range(2):
                    assert_same(f"{name}: {m} cache {i}", other[idx][i].view(-1, H).cpu(), plain[idx][i].view(-1, H).cpu())
    for i in range(2):                                                    # the other layer and rows no token names: untouched
        for c in (real[1][i], real[2][i]):
            untouched = np.ones(SC.MAX_SLOTS, dtype=bool)
            untouched[S.slots[i]] = False
            v = c.double().cpu().numpy()
            assert (v[1 - layer] == 3.0).all() and (v[layer][untouched] == 3.0).all()
    pos = S.all_pos()
    for k, m in enumerate("qkv"):
        if m not in modules:
            continue
        base = qkv64[:, k * H: (k + 1) * H]
        y, e_y = LR.expand_ref64(base, u64[:, k * r16: (k + 1) * r16], b64[m], scaling, dtype)
        if dtype == "fp32":
            e_y = e_y + 2.0 ** -23 * (np.abs(base) + np.abs(y - base))
        assert float(np.abs(y - base).mean()) > 0.1, "the adapter's term must be visible against the base"
        if m == "v":
            got, ref, bound = S.gather(real[2], layer), y, e_y
        else:
            ref, mag = SC.rope_rotate64(y, pos, n_heads, head_dim)
            _, carried = SC.rope_rotate64(e_y, pos, n_heads, head_dim)            # |e0 c| + |e1 s|: the operands' errors through the pair
            bound = LR.rounded_within(ref, carried + SC.ROPE_REL * mag, dtype)
            got = real[0][:, :H].double().cpu().numpy() if m == "q" else S.gather(real[1], layer)
        err = np.abs(got - ref)
        print(f"expand {dtype} {n_heads}x{head_dim} {''.join(modules)} module {m}: worst |err| / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (m, float((err / bound).max()), np.argwhere(err > bound)[:3].tolist())


def test_lora_rope_kv_scalar_kernel_in_16_bits(lib):
    """head_dim 24 (not a multiple of 16) takes the scalar template in bf16 too: B = 0 equals the plain pass bit for bit, a real B moves q"""
    n_heads, head_dim, r16, td = 3, 24, 16, torch.bfloat16
    H = n_heads * head_dim
    S = TwoSegs(H, td)
    rng = np.random.default_rng(9)
    qkv = torch.from_numpy(rng.standard_normal((S.total, 3 * H)).astype(np.float32)).to(td)
    u = torch.from_numpy(rng.standard_normal((S.total, 3 * r16)).astype(np.float32)).to(td).cuda()
    b = torch.from_numpy((rng.standard_normal((H, r16)) * 0.3).astype(np.float32)).to(td).cuda()
    cos, sin = (torch.from_numpy(t).cuda() for t in SC.rope_tables(head_dim))
    tail = (cos.data_ptr(), sin.data_ptr(), 0, n_heads, head_dim, SC.MAX_POS, _lib.dtype_code(td))
    res = []
    for bq in (None, torch.zeros_like(b), b):
        q = qkv.clone().cuda()
        kc, vc = S.caches()
        if bq is None:
            _lib.check(lib.atspeed_segs_rope_kv(q.data_ptr(), None, 0, *tail, *S.args(kc, vc), _st()))
        else:
            _lib.check(lib.atspeed_segs_lora_rope_kv(q.data_ptr(), u.data_ptr(), bq.data_ptr(), None, None, r16, 2.0, *tail, *S.args(kc, vc), _st()))
        torch.cuda.synchronize()
        res.append((q.cpu(), [c.cpu() for c in kc], [c.cpu() for c in vc]))
    assert_same("scalar B = 0: q", res[1][0], res[0][0])
    for i in range(2):
        assert_same("scalar: k cache", res[2][1][i].view(-1, H), res[0][1][i].view(-1, H))
        assert_same("scalar: v cache", res[2][2][i].view(-1, H), res[0][2][i].view(-1, H))
    assert float((res[2][0][:, :H].float() - res[0][0][:, :H].float()).abs().mean()) > 0.1


# ------------------------------------------------------------------ 3. fp32 engine at small dims
def _adapter(dims, seed, r=8, alpha=16, modules=("q", "v"), std=0.1, rslora=False):
    return L.from_tensors(synth.synthetic_lora(dims, seed, r=r, modules=modules, std=std), dims.n_layers, dims.hidden, r, alpha, rslora)


def _tree_inputs(P, B, V, g, hide=5):
    """tests/test_fulldims_gpu.py's packed-verify-like forward: a prompt, then B tree tokens that see the prompt (minus one slot) and themselves"""
    ids = torch.cat((torch.randint(3, 32000, (P,), generator=g), torch.randint(32000, V, (B,), generator=g))).to(torch.int32)
    T = P + B
    vis = torch.zeros(T, T, dtype=torch.bool)
    vis[:P, :P] = torch.tril(torch.ones(P, P, dtype=torch.bool))
    vis[P:, :P] = True
    vis[P:, P:] = torch.eye(B, dtype=torch.bool)
    vis[P:, hide] = False
    pos = torch.cat((torch.arange(P), torch.full((B,), P))).to(torch.int32)
    return ids, pos, torch.arange(T, dtype=torch.int32), vis


@pytest.mark.parametrize("modules,r,rslora", [(("q", "v"), 8, False), (("q", "k", "v"), 40, True)], ids=["qv_r8", "qkv_r40_rslora"])
def test_fp32_forward_with_adapter_matches_the_lora_reference(modules, r, rslora):
    """Llama-68M-like dims (768 / 12 heads x 64 / 2 layers; hidden % 128 == 0 but fp32: the scalar kernels): a tree-mask forward, then a second
    forward that reads the K / V the first one cached (a wrong v or k in the cache shows only there), both <= 1e-3 of the LoRA reference --
    whose logits the adapter moves by far more than that."""
    V = synth.TINY.vocab_size
    dims = synth.LlamaDims(V, 768, 2, 12, 3072)
    sd = synth.synthetic_state_dict(dims, 5, std=0.03, head_std=0.1)
    ad = _adapter(dims, 6, r=r, modules=modules, std=0.05, rslora=rslora)
    m = HipLlama.from_state_dict(dims, sd, torch.float32, max_slots=256, max_tokens=256, max_logit_rows=128).load_lora(ad)
    assert m.lora.modules == modules and m.lora.r == r and abs(m.lora.scaling - (16 / np.sqrt(r) if rslora else 16 / r)) < 1e-12
    ref, plain = LR.LoraRefLlama(dims, sd, max_slots=256).set_lora(ad), RefLlama(dims, sd, max_slots=256)
    g = torch.Generator().manual_seed(3)
    ids, pos, slots, vis = _tree_inputs(40, 30, V, g)
    m.lora_launches(reset=True)
    got1 = m.forward_raw(ids.cuda(), pos.cuda(), slots.cuda(), vis_bits_from_bool(vis, 256).cuda(), 70, 31).cpu()
    assert m.lora_launches() == 2 * dims.n_layers and m.rope_fused_launches() == 0
    want1, base1 = ref.forward(ids, pos, slots, vis, n_logit_rows=31), plain.forward(ids, pos, slots, vis, n_logit_rows=31)
    assert float((want1 - base1).abs().max()) > 100 * SCORE_TOL
    assert float((got1 - want1).abs().max()) <= SCORE_TOL
    # second forward: 12 new tokens at slots 70.. that see all 70 cached slots (minus one) and themselves
    n2 = 12
    ids2 = torch.randint(32000, V, (n2,), generator=g).to(torch.int32)
    pos2 = torch.full((n2,), 41, dtype=torch.int32)
    slots2 = torch.arange(70, 70 + n2, dtype=torch.int32)
    vis2 = torch.zeros(n2, 70 + n2, dtype=torch.bool)
    vis2[:, :70] = True
    vis2[:, 9] = False
    vis2[:, 70:] = torch.eye(n2, dtype=torch.bool)
    got2 = m.forward_raw(ids2.cuda(), pos2.cuda(), slots2.cuda(), vis_bits_from_bool(vis2, 256).cuda(), 70 + n2, n2).cpu()
    want2 = ref.forward(ids2, pos2, slots2, vis2, n_logit_rows=n2)
    print(f"fp32 + adapter {modules} r={r}: max err {float((got1 - want1).abs().max()):.2e} / {float((got2 - want2).abs().max()):.2e}, "
          f"adapter moves the logits by {float((want1 - base1).abs().max()):.3f}")
    assert float((got2 - want2).abs().max()) <= SCORE_TOL


GOLDEN_LORA = ("k20_dk40_sigma01", "k8_dk16_trie", "k20_dk40_sigma01_s7")     # position mask, strict trie, K = 20 / DK = 40 with another seed


@pytest.mark.parametrize("name", GOLDEN_LORA)
def test_fp32_bssd_with_adapted_target_equals_the_oracle_on_the_lora_reference(name):
    """three golden recipes with a rank-8 q / v adapter on the target: the oracle's own item list WITH the adapter differs from its list
    WITHOUT (asserted; adapter std 0.1 leaves the oracle's smallest decision margin at >= 2e-4, far above fp32 noise at these dims), and the
    engine reproduces the list with: token ids, per-round n_matches and the draft's candidate ids exactly, scores <= 1e-3; target_generate
    likewise (the lossless property)."""
    case = [c for c in CASES if c["name"] == name][0]
    ci = build_case_inputs(case)
    ad = _adapter(ci["target_dims"], 77, std=0.1)
    rd = RefLlama(ci["draft_dims"], ci["draft_sd"])
    args = (ci["prompt"], case["gamma"], case["max_new_tokens"], case["K"], case["DK"], ci["fn"])
    without = R.BSSD(RefLlama(ci["target_dims"], ci["target_sd"]), rd, *args)
    ref = R.BSSD(LR.LoraRefLlama(ci["target_dims"], ci["target_sd"]).set_lora(ad), RefLlama(ci["draft_dims"], ci["draft_sd"]), *args)
    P = len(ci["prompt"])
    assert ref["beam_sequence"][:, P:].tolist() != without["beam_sequence"][:, P:].tolist(), "the adapter must change the oracle's items"
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **kw).load_lora(ad)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **kw)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}
    out = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    assert out["beam_sequence"][:, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()
    np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
    assert (out["n_run"], out["total_accept_steps"]) == (ref["n_run"], ref["total_accept_steps"])
    tr = last_trace(tgt, drf)
    assert [r["n_matches"] for r in tr] == [r["n_matches"] for r in ref["rounds"]]
    for r, g in zip(tr, ref["rounds"]):
        for ids, gids in zip(r["draft_ids"], g["draft_ids"]):
            assert [x for x in ids if x >= 0] == gids
    tg = target_generate(tgt, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    rtg = R.target_generate(LR.LoraRefLlama(ci["target_dims"], ci["target_sd"]).set_lora(ad), ci["prompt"], case["max_new_tokens"], case["K"], ci["fn"])
    assert tg["beam_sequence"][:, P:].cpu().tolist() == rtg["beam_sequence"][:, P:].tolist()
    np.testing.assert_allclose(tg["beam_scores"].cpu().numpy(), rtg["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
    assert torch.equal(tg["beam_sequence"], out["beam_sequence"])
    release_decoders(tgt, drf)


def test_fp32_batch_and_session_with_adapter_equal_the_single_calls():
    """the adapter belongs to the model: BSSD_batch of 4 users and BSSD_batch(..., lanes=2) give each user's single BSSD result, and the
    session allocates nothing after its creation (lora_u and the adapter copies exist since load_lora)"""
    case = [c for c in CASES if c["name"] == "k20_dk40_sigma01"][0]
    ci = build_case_inputs(case)
    ad = _adapter(ci["target_dims"], 77, std=0.1)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **kw).load_lora(ad)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **kw)
    users = [synth.synthetic_prompt(18 + 5 * u, 900 + u) for u in range(3)] + [ci["prompt"]]
    inputs = [{"input_ids": torch.from_numpy(p)[None].cuda()} for p in users]
    a = (case["gamma"], case["max_new_tokens"])
    single = [BSSD(tgt, drf, inp, *a, prefix_allowed_tokens_fn=ci["fn"]) for inp in inputs]
    tgt.lora_launches(reset=True)
    bat = BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=ci["fn"])
    assert tgt.lora_launches() > 0
    ses = BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=ci["fn"], lanes=2)
    for what, outs in (("batch", bat), ("lanes=2", ses)):
        assert len(outs) == 4
        for u, (s, o) in enumerate(zip(single, outs)):
            assert torch.equal(s["beam_sequence"], o["beam_sequence"]), (what, u)
            np.testing.assert_allclose(s["beam_scores"].cpu().numpy(), o["beam_scores"].cpu().numpy(), atol=1e-4, rtol=0)
            assert (s["n_run"], s["total_accept_steps"], s["accept_steps"]) == (o["n_run"], o["total_accept_steps"], o["accept_steps"]), (what, u)
    c = ses[0]["session_counters"]
    assert c["allocs_after_create"] == 0 and c["users_retired"] == 4, c
    release_decoders(tgt, drf)


# ------------------------------------------------------------------ 4. 16-bit and quantised bases at the Llama-7B width
H7, F7, HEADS7, LAYERS7 = 4096, 11008, 32, 2
FULL_STD = 0.03          # adapter std at this width: moves the reference's logits by more than 3 x the 16-bit bar (asserted below)


def _err(got, want):
    scale = float(want.abs().max())
    e = (got - want).abs()
    return float(e.max()) / scale, float(e.mean()) / scale


def _full(dtype, seed=2025, head_std=0.02):
    V = synth.BEAUTY.vocab_size
    dims = synth.LlamaDims(V, H7, LAYERS7, HEADS7, F7)
    m = HipLlama.from_synthetic(dims, seed, std=0.02, head_std=head_std, dtype=dtype, max_slots=512, max_tokens=512, max_logit_rows=448)
    return dims, m, _adapter(dims, 78, std=FULL_STD)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16bit_forward_with_adapter_at_llama7b_width(dtype):
    """hidden 4096 / ffn 11008 / 32 x 128, 2 layers, rank-8 q / v adapter: one 228-token tree forward (small-M kernels) and a 12-sequence
    lock-step batch (ring GEMM; without an adapter its qkv projection carries RoPE in the epilogue) against the LoRA reference on the weight
    and adapter values the device holds, at the existing 16-bit bar; the reference's logits with and without the adapter differ by more than
    3 x that bar; no fused RoPE launch, and 2 adapter launches per layer per forward."""
    dims, m, ad = _full(dtype)
    V = dims.vocab_size
    sd = m.export_state_dict()
    m.load_lora(ad)
    ref, plain = LR.LoraRefLlama(dims, sd, max_slots=512).set_lora(ad, dtype), RefLlama(dims, sd, max_slots=512)
    g = torch.Generator().manual_seed(11)
    ids, pos, slots, vis = _tree_inputs(108, 120, V, g)
    m.lora_launches(reset=True), m.rope_fused_launches(reset=True)
    got = m.forward_raw(ids.cuda(), pos.cuda(), slots.cuda(), vis_bits_from_bool(vis, 512).cuda(), 228, 24).float().cpu()
    assert m.lora_launches(reset=True) == 2 * LAYERS7 and m.rope_fused_launches() == 0
    want, base = ref.forward(ids, pos, slots, vis, n_logit_rows=24), plain.forward(ids, pos, slots, vis, n_logit_rows=24)
    d_max, d_mean = _err(base, want)
    e_max, e_mean = _err(got, want)
    print(f"{dtype} + adapter, 228 tokens: max err {e_max:.4f} mean {e_mean:.5f}; the adapter moves the reference by max {d_max:.4f} mean {d_mean:.5f}")
    assert d_max > 3 * BF16_MAX_TOL and d_mean > 3 * BF16_MEAN_TOL
    assert e_max < BF16_MAX_TOL and e_mean < BF16_MEAN_TOL
    seqs, refs = [], []
    for i in range(12):
        P, B = 70 + 6 * i, 60
        s = _tree_inputs(P, B, V, g, hide=3 + i)
        seqs.append((s[0], s[1], s[2], vis_bits_from_bool(s[3], 512), P + B, 8))
        refs.append(s)
    outs = m.forward_raw_batch(seqs)
    torch.cuda.synchronize()
    assert m.lora_launches() == 2 * LAYERS7 and m.rope_fused_launches() == 0
    for i in (0, 11):
        want, base = ref.forward(*refs[i], n_logit_rows=8), plain.forward(*refs[i], n_logit_rows=8)
        e_max, e_mean = _err(outs[i].float().cpu(), want)
        d_max, d_mean = _err(base, want)
        print(f"{dtype} + adapter, batched sequence {i}: max err {e_max:.4f} mean {e_mean:.5f}; adapter moves max {d_max:.4f} mean {d_mean:.5f}")
        assert d_max > 3 * BF16_MAX_TOL and d_mean > 3 * BF16_MEAN_TOL
        assert e_max < BF16_MAX_TOL and e_mean < BF16_MEAN_TOL


def _judge(got, want_q, want_32, label):
    """the quantised-base bar of tests/test_fp8_gpu.py / test_fp4_gpu.py: closer to the quantised LoRA reference than FP8_VS_NOISE x the scheme's
    own noise (mean) and than its worst case (max), and closer to it than to the unquantised LoRA reference"""
    scale = float(want_q.abs().max())
    eq, e32, qn = (got - want_q).abs(), (got - want_32).abs(), (want_q - want_32).abs()
    print(f"{label}: vs quantised LoRA reference max {float(eq.max()) / scale:.4f} mean {float(eq.mean()) / scale:.4f}; vs unquantised mean "
          f"{float(e32.mean()) / scale:.4f}; scheme noise mean {float(qn.mean()) / scale:.4f} max {float(qn.max()) / scale:.4f}")
    assert float(eq.mean()) < FP8_VS_NOISE * float(qn.mean()) and float(eq.max()) < float(qn.max())
    assert float(eq.mean()) < float(e32.mean())


def _seq(g, V, T, hole=7):
    ids = torch.cat((torch.randint(3, 32000, (T - 30,), generator=g), torch.randint(32000, V, (30,), generator=g))).to(torch.int32)
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
    vis[10:, hole] = False                                        # tree mask, not plain causal
    pos = torch.arange(T, dtype=torch.int32)
    return ids, pos, pos.clone(), vis


def test_fp8_base_with_16bit_adapter():
    """enable_fp8() + adapter at the Llama-7B width: one user at 228 tokens (weight-streaming W8A8 kernels; without an adapter RoPE rides in
    the qkv epilogue) and the batched path (32 x 100 tokens: the W8A8 ring kernels) against the LoRA reference with w8a8=True under
    test_fp8_gpu.py's bar, every projection counted as fp8 (`other == 0`), the adapter moving the W8A8 reference by more than the scheme's own
    noise; and loading the adapter AFTER enable_fp8() gives the same bits as loading it before."""
    dims, m, ad = _full(torch.bfloat16, seed=31, head_std=0.05)
    V = dims.vocab_size
    sd = m.export_state_dict()
    ref8 = LR.LoraRefLlama(dims, sd, max_slots=512, w8a8=True).set_lora(ad, torch.bfloat16)
    ref32 = LR.LoraRefLlama(dims, sd, max_slots=512).set_lora(ad, torch.bfloat16)
    m.load_lora(ad)                                              # before the base is quantised (the CLI's order)
    m.enable_fp8()
    g = torch.Generator().manual_seed(6)
    one = _seq(g, V, 228)
    dev = lambda s, rows: (s[0].cuda(), s[1].cuda(), s[2].cuda(), vis_bits_from_bool(s[3], 512).cuda(), s[0].numel(), rows)
    m.fp8_counters(reset=True), m.lora_launches(reset=True), m.rope_fused_launches(reset=True)
    got = m.forward_raw(*dev(one, 6)).float().cpu()
    torch.cuda.synchronize()
    assert all(c["fp8"] == LAYERS7 and c["other"] == 0 for c in m.fp8_counters(reset=True).values())
    assert m.lora_launches(reset=True) == 2 * LAYERS7 and m.rope_fused_launches() == 0
    want8, want32 = ref8.forward(*one, n_logit_rows=6), ref32.forward(*one, n_logit_rows=6)
    base8 = ref8.clear_lora().forward(*one, n_logit_rows=6)
    ref8.set_lora(ad, torch.bfloat16)
    assert float((want8 - base8).abs().mean()) > float((want8 - want32).abs().mean()), "the adapter must move the W8A8 reference by more than the scheme's noise"
    _judge(got, want8, want32, "W8A8 + adapter, one user, 228 tokens")
    seqs = [_seq(g, V, 100, hole=7 + i % 9) for i in range(32)]
    outs = m.forward_raw_batch([(s[0], s[1], s[2], vis_bits_from_bool(s[3], 512), 100, 6) for s in seqs])
    torch.cuda.synchronize()
    assert all(c["fp8"] == LAYERS7 and c["other"] == 0 for c in m.fp8_counters().values())
    assert m.lora_launches() == 2 * LAYERS7 and m.rope_fused_launches() == 0
    for i in (0, 31):
        _judge(outs[i].float().cpu(), ref8.forward(*seqs[i], n_logit_rows=6), ref32.forward(*seqs[i], n_logit_rows=6), f"W8A8 + adapter, batched sequence {i}")
    # the same adapter loaded again, now after enable_fp8(): the same bits
    m.unload_lora()
    m.load_lora(ad)
    again = m.forward_raw(*dev(one, 6)).float().cpu()
    assert_same("adapter loaded after enable_fp8 vs before", again, got)


def test_fp4_base_with_16bit_adapter():
    """enable_fp4() + adapter, one user at 121 tokens, fp16 (the reference's checkpoint type), under test_fp4_gpu.py's bar"""
    dims, m, ad = _full(torch.float16, seed=41, head_std=0.05)
    V = dims.vocab_size
    sd = m.export_state_dict()
    ref4 = LR.LoraRefLlamaW4A8(dims, sd, max_slots=512).set_lora(ad, torch.float16)
    ref32 = LR.LoraRefLlama(dims, sd, max_slots=512).set_lora(ad, torch.float16)
    m.enable_fp4()
    m.load_lora(ad)
    g = torch.Generator().manual_seed(9)
    s = _seq(g, V, 121)
    m.fp4_counters(reset=True), m.lora_launches(reset=True)
    got = m.forward_raw(s[0].cuda(), s[1].cuda(), s[2].cuda(), vis_bits_from_bool(s[3], 512).cuda(), 121, 6).float().cpu()
    torch.cuda.synchronize()
    assert all(c["fp4"] == LAYERS7 and c["other"] == 0 for c in m.fp4_counters().values())
    assert m.lora_launches() == 2 * LAYERS7
    _judge(got, ref4.forward(*s, n_logit_rows=6), ref32.forward(*s, n_logit_rows=6), "W4A8 + adapter, one user, 121 tokens")


# ------------------------------------------------------------------ 5. composition and the on / off switch
def _small_pair(dtype=torch.bfloat16):
    """tests/test_bssd_gpu.py::test_bssd_bf16_is_lossless_against_own_target_generate's pair"""
    V = synth.BEAUTY.vocab_size
    tdims, ddims = synth.LlamaDims(V, 512, 2, 8, 1376), synth.LlamaDims(V, 256, 2, 4, 704)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_synthetic(tdims, 11, std=0.03, head_std=0.2, dtype=dtype, num_beams=20, **kw)
    drf = HipLlama.from_synthetic(ddims, 12, std=0.03, head_std=0.2, dtype=dtype, num_beams=40, **kw)
    return tgt, drf


def test_bf16_bssd_with_adapter_is_lossless_against_own_target_generate():
    """the criterion of test_bssd_bf16_is_lossless_against_own_target_generate with an adapted target -- and the adapter changes the items"""
    tgt, drf = _small_pair()
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    prompts = [synth.synthetic_prompt(60 + 17 * u, 100 + u) for u in range(2)]
    before = [target_generate(tgt, {"input_ids": torch.from_numpy(p)[None].cuda()}, 4, prefix_allowed_tokens_fn=fn) for p in prompts]
    tgt.load_lora(_adapter(tgt.dims, 79, std=0.1))
    for prompt, b0 in zip(prompts, before):
        inputs = {"input_ids": torch.from_numpy(prompt)[None].cuda()}
        a = BSSD(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn)
        b = target_generate(tgt, inputs, 4, prefix_allowed_tokens_fn=fn)
        sa, sb = a["beam_scores"].cpu().numpy(), b["beam_scores"].cpu().numpy()
        np.testing.assert_allclose(sa, sb, atol=5e-2, rtol=0)
        ta, tb = a["beam_sequence"][:, len(prompt):].cpu().tolist(), b["beam_sequence"][:, len(prompt):].cpu().tolist()
        if np.abs(np.diff(sb)).min() > 5e-2:
            assert ta == tb
        assert len({tuple(x) for x in ta} & {tuple(x) for x in tb}) >= 18
        assert tb != b0["beam_sequence"][:, len(prompt):].cpu().tolist(), "the adapter must change the engine's items"
    release_decoders(tgt, drf)


def test_unload_restores_the_model_bit_for_bit_and_counters_follow():
    """A model without an adapter keeps lora_launches == 0 and its fused RoPE epilogue; with one the counters swap; after unload_lora() the
    logits are bit-identical to a model that never had an adapter and the fused-RoPE counter advances again.  A second adapter replaces the first."""
    V = synth.BEAUTY.vocab_size
    dims = synth.LlamaDims(V, 1024, 2, 8, 2816)                   # head_dim 128, hidden % 256 == 0: the batched qkv projection fuses RoPE
    make = lambda: HipLlama.from_synthetic(dims, 7, std=0.03, head_std=0.1, dtype=torch.bfloat16, max_slots=512, max_tokens=512, max_logit_rows=448)
    never, m = make(), make()
    g = torch.Generator().manual_seed(4)
    seqs = []
    for i in range(16):                                           # 1824 tokens: 15 x 12 tiles of 128 x 256 fill 70 % of a round of the chip, so the ring kernel takes the qkv projection
        s = _tree_inputs(60 + 4 * (i % 8), 40, V, g, hide=3 + i % 8)
        seqs.append((s[0], s[1], s[2], vis_bits_from_bool(s[3], 512), s[0].numel(), 4))
    want = never.forward_raw_batch(seqs, return_all=True).clone()
    assert never.lora_launches() == 0 and never.rope_fused_launches(reset=True) == dims.n_layers and never.lora is None
    ad_a, ad_b = _adapter(dims, 80, std=0.1), _adapter(dims, 81, r=16, modules=("q", "k", "v"), std=0.1)
    m.load_lora(ad_a)
    m.rope_fused_launches(reset=True)
    with_a = m.forward_raw_batch(seqs, return_all=True).clone()
    assert m.lora_launches(reset=True) == 2 * dims.n_layers and m.rope_fused_launches() == 0
    assert float((with_a - want).abs().max()) > 0.05 * float(want.abs().max())
    m.load_lora(ad_b)                                             # replaces the first
    assert m.lora.r == 16 and m.lora.modules == ("q", "k", "v")
    with_b = m.forward_raw_batch(seqs, return_all=True).clone()
    assert not torch.equal(with_b, with_a)
    m.load_lora(ad_a)
    assert_same("the first adapter again", m.forward_raw_batch(seqs, return_all=True), with_a)
    m.unload_lora()
    m.unload_lora()                                               # a no-op without an adapter
    m.lora_launches(reset=True), m.rope_fused_launches(reset=True)
    assert_same("after unload_lora vs a model that never had an adapter", m.forward_raw_batch(seqs, return_all=True), want)
    assert m.lora_launches() == 0 and m.rope_fused_launches() == dims.n_layers and m.lora is None


def test_set_lora_refusals(lib):
    V = synth.TINY.vocab_size
    dims = synth.LlamaDims(V, 256, 1, 4, 512)
    m = HipLlama.from_synthetic(dims, 1, dtype=torch.bfloat16, max_slots=256, max_tokens=256, max_logit_rows=64)
    a = torch.zeros(8, 256, dtype=torch.bfloat16, device="cuda")
    lay = (_lib.LoraLayer * 1)()
    assert lib.atspeed_llama_set_lora(m._handle, 8, 2.0, lay, _st()) == _lib.ERR_INVALID and b"no module" in lib.atspeed_last_error()
    lay[0].a_q = a.data_ptr()
    assert lib.atspeed_llama_set_lora(m._handle, 8, 2.0, lay, _st()) == _lib.ERR_INVALID and b"one half" in lib.atspeed_last_error()
    lay[0].b_q = a.data_ptr()
    assert lib.atspeed_llama_set_lora(m._handle, 65, 2.0, lay, _st()) == _lib.ERR_INVALID and b"rank 65" in lib.atspeed_last_error()
    assert lib.atspeed_llama_set_lora(m._handle, 8, float("nan"), lay, _st()) == _lib.ERR_INVALID
    assert m.lora_launches() == 0 and lib.atspeed_llama_lora_launches(None, 0) == -1
    with pytest.raises(NotImplementedError):
        m.load_lora(synth.synthetic_lora(dims, 2, r=65), r=65, lora_alpha=16)


def test_graph_captured_before_load_lora_is_dropped():
    """graphs on: a decode shape captured and replayed without an adapter must, after load_lora, give what the ungraphed adapted model gives
    (set / clear drop the model's captured graphs: a replay would run the launch sequence of before)"""
    tgt, drf = _small_pair()
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    inp = {"input_ids": torch.from_numpy(synth.synthetic_prompt(64, 77))[None].cuda()}
    ad = _adapter(tgt.dims, 79, std=0.1)
    with _lib.switches(graphs=1):
        plain = [BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn) for _ in range(3)]      # second sight captures, third replays
        tgt.load_lora(ad)
        graphed = [BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn) for _ in range(3)]
        torch.cuda.synchronize()
    eager = BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn)
    assert not torch.equal(eager["beam_sequence"], plain[0]["beam_sequence"]), "the adapter must change the items"
    for o in graphed:
        assert torch.equal(o["beam_sequence"], eager["beam_sequence"]) and torch.equal(o["beam_scores"], eager["beam_scores"])
    with _lib.switches(graphs=1):
        tgt.unload_lora()
        back = BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn)
    assert torch.equal(back["beam_sequence"], plain[0]["beam_sequence"]) and torch.equal(back["beam_scores"], plain[0]["beam_scores"])
    release_decoders(tgt, drf)
