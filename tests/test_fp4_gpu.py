"""The 4-bit target (W4A8: OCP MXFP4 weights x per-token e4m3 activations on v_mfma_scale_f32_16x16x128_f8f6f4) against its restatements:
the quantiser bit for bit against tests/mxfp4_ref.py, the GEMM against the exact product in fp64, the forward and BSSD against a W4A8
RefLlama (tests/mxfp4_ref.RefLlamaW4A8), the engine's counters, refusals and the graph key."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import atspeed_amd
from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, release_decoders, target_generate, target_generate_batch
from atspeed_amd.model import HipLlama, vis_bits_from_bool
from oracle import beamsd_ref as R
from oracle.llama_ref import RefLlama
from tests.mxfp4_ref import dequant_mxfp4, pack_nibbles, quant_mxfp4

FP8_VS_NOISE = 0.85                        # the W8A8 tests' bar (tests/test_fp8_gpu.py), against the W4A8 scheme's own noise
H7, F7, HEADS7 = 4096, 11008, 32
DT = {torch.bfloat16: _lib.ATSPEED_BF16, torch.float16: _lib.ATSPEED_F16}


def _stream():
    return _lib.stream_ptr(0)


def _quant_dev(w16: torch.Tensor, packed: bool):
    """the library's quantiser on a [rows, K] 16-bit CUDA tensor -> (nibbles uint8 [rows, K / 2], scales uint8 [rows, K / 32]) on the host"""
    lib = _lib.load()
    rows, K = w16.shape
    src = w16.contiguous()
    if packed:
        ev = rows + (rows & 1)
        pad = torch.zeros(ev, K, dtype=w16.dtype, device="cuda")
        pad[:rows] = w16
        src = torch.empty_like(pad)
        _lib.check(lib.atspeed_pack_rows(pad.data_ptr(), src.data_ptr(), ev, 2 * K, _stream()))
    q = torch.empty(rows, K // 2, dtype=torch.uint8, device="cuda")
    s = torch.empty(rows, K // 32, dtype=torch.uint8, device="cuda")
    _lib.check(lib.atspeed_quant_weights_mxfp4(src.data_ptr(), rows, K, DT[w16.dtype], int(packed), q.data_ptr(), s.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return q.cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_quantiser_is_bit_equal_to_the_numpy_rule(dtype):
    g = torch.Generator().manual_seed(1)
    rows, K = 37, 512                                             # odd row count
    w = (torch.randn(rows, K, generator=g) * 0.05).to(dtype)
    w[:, 7] *= 40                                                 # an outlier column: the other elements of its blocks go to 0
    # crafted blocks: ties (scale 1: amax 6), saturation (amax 7.9), zero blocks, exact powers of two, a tiny block
    tie = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, 0.0] * 2)
    w[0, 0:32] = tie.to(dtype)
    w[1, 32:64] = torch.tensor([7.9, -7.5, 5.5, 6.5] * 8).to(dtype)
    w[2, :] = 0
    w[3, 64:96] = torch.tensor([2.0 ** -5, -(2.0 ** -6), 2.0 ** -8, 0.0] * 8).to(dtype)
    w[4, 96:128] = torch.tensor([2.0 ** 3] * 32).to(dtype)
    w[5, 128:160] = (torch.arange(32) - 16).to(dtype) * 2.0 ** -14
    want_c, want_s = quant_mxfp4(w.float().numpy())
    want_q = pack_nibbles(want_c)
    for packed in (False, True):
        q, s = _quant_dev(w.cuda(), packed)
        np.testing.assert_array_equal(s, want_s)
        np.testing.assert_array_equal(q, want_q)
    assert want_s[2].tolist() == [0] * (K // 32) and not want_q[2].any()
    assert dequant_mxfp4(want_c, want_s)[0, :8].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]


def _rand_e4m3(g, m, K):
    v = torch.randn(m, K, generator=g) * 40
    return v.clamp(-448, 448).to(torch.float8_e4m3fn)


def _rand_w4(g, n, K):
    """random MXFP4 weights: codes [n, K] and scale bytes around 2^-6"""
    codes = torch.randint(0, 16, (n, K), generator=g).numpy().astype(np.uint8)
    sb = torch.randint(118, 124, (n, K // 32), generator=g).numpy().astype(np.uint8)
    sb[0, 0] = 0                                                  # an all-zero-scale block
    return codes, sb


def _exact(xq, sx, codes, sb):
    """(xq @ dequant(W).T) * sx in fp64, and the bound sum |a b| * sx for the fp32 summation error"""
    a = xq.float().double().numpy()
    w = dequant_mxfp4(codes, sb).astype(np.float64)
    s = sx.double().numpy()[:, None]
    return (a @ w.T) * s, (np.abs(a) @ np.abs(w).T) * s


@pytest.mark.parametrize("K", [4096, 11008])
def test_gemm_w4a8_matches_the_exact_product(K):
    lib = _lib.load()
    g = torch.Generator().manual_seed(K)
    n = 200                                                       # 3 tiles of 64 weight rows + a tail of 8
    codes, sb = _rand_w4(g, n, K)
    wq = torch.from_numpy(pack_nibbles(codes)).cuda()
    ws_ = torch.from_numpy(sb).cuda()
    work = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    ms = (1, 16, 33, 121, 228, 256, 257, 600, 1100) if K == 4096 else (1, 60, 228, 300)
    for m in ms:
        xq = _rand_e4m3(g, m, K)
        sx = torch.rand(m, generator=g) * 0.01 + 1e-3
        ref, bound = _exact(xq, sx, codes, sb)
        tol = (K / 128 + 16) * 2.0 ** -24 * bound + 1e-30
        xd, sxd = xq.view(torch.uint8).cuda(), sx.cuda()
        for ws_bytes in (work.numel(), 0):                       # split into slabs + the reduce pass / the epilogue in the kernel
            wp = work.data_ptr() if ws_bytes else None
            c = torch.empty(m, n, dtype=torch.float32, device="cuda")
            _lib.check(lib.atspeed_gemm_w4a8(xd.data_ptr(), sxd.data_ptr(), wq.data_ptr(), ws_.data_ptr(), c.data_ptr(), m, n, K, n, 1,
                                             _lib.ATSPEED_BF16, 0, wp, ws_bytes, _stream()))
            err = np.abs(c.cpu().double().numpy() - ref)
            assert (err <= tol).all(), (m, ws_bytes, float((err / (bound + 1e-30)).max()))
            if m not in (1, 228, 1100) and K == 4096:
                continue
            for dtype in (torch.bfloat16, torch.float16):
                u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
                c16 = torch.empty(m, n, dtype=dtype, device="cuda")
                _lib.check(lib.atspeed_gemm_w4a8(xd.data_ptr(), sxd.data_ptr(), wq.data_ptr(), ws_.data_ptr(), c16.data_ptr(), m, n, K, n, 0,
                                                 DT[dtype], 0, wp, ws_bytes, _stream()))
                got = c16.cpu().double().numpy()
                assert (np.abs(got - ref) <= tol + u * np.abs(ref)).all(), ("store", m, dtype)
                h0 = (torch.randn(m, n, generator=g) * float(np.abs(ref).mean() + 1e-3)).to(dtype)
                h = h0.cuda()
                _lib.check(lib.atspeed_gemm_w4a8(xd.data_ptr(), sxd.data_ptr(), wq.data_ptr(), ws_.data_ptr(), h.data_ptr(), m, n, K, n, 2,
                                                 DT[dtype], 0, wp, ws_bytes, _stream()))
                want = h0.double().numpy() + ref
                assert (np.abs(h.cpu().double().numpy() - want) <= tol + u * (np.abs(ref) + np.abs(want))).all(), ("resid", m, dtype)
    # SwiGLU (N % 32 == 0: gate rows 32b..32b+15, up rows 32b+16..32b+31) and operands in the packed layout, at a split and an unsplit size
    n2 = 192
    codes2, sb2 = _rand_w4(g, n2, K)
    wq2, ws2 = torch.from_numpy(pack_nibbles(codes2)).cuda(), torch.from_numpy(sb2).cuda()
    for m in (33, 600):
        xq = _rand_e4m3(g, m, K)
        sx = torch.rand(m, generator=g) * 0.01 + 1e-3
        ref, bound = _exact(xq, sx, codes2, sb2)
        r16 = torch.from_numpy(ref).to(torch.bfloat16).double()
        gate = r16.view(m, n2 // 32, 2, 16)[:, :, 0].reshape(m, -1)
        up = r16.view(m, n2 // 32, 2, 16)[:, :, 1].reshape(m, -1)
        want = (gate * torch.sigmoid(gate) * up).numpy()
        ev = m + (m & 1)
        xpad = torch.zeros(ev, K, dtype=torch.uint8, device="cuda")
        xpad[:m] = xq.view(torch.uint8).cuda()
        xpk = torch.empty_like(xpad)
        _lib.check(lib.atspeed_pack_rows(xpad.data_ptr(), xpk.data_ptr(), ev, K, _stream()))
        for packed in (0, 1):
            for ws_bytes in (work.numel(), 0):
                out = torch.zeros(ev, n2 // 2, dtype=torch.bfloat16, device="cuda")
                src = xpk if packed else xpad
                _lib.check(lib.atspeed_gemm_w4a8(src.data_ptr(), sx.cuda().data_ptr(), wq2.data_ptr(), ws2.data_ptr(), out.data_ptr(), m, n2, K,
                                                 n2 // 2, 3, _lib.ATSPEED_BF16, packed, work.data_ptr() if ws_bytes else None, ws_bytes, _stream()))
                if packed:
                    un = torch.empty_like(out)
                    _lib.check(lib.atspeed_unpack_rows(out.data_ptr(), un.data_ptr(), ev, n2, _stream()))
                    out = un
                got = out[:m].cpu().double().numpy()
                assert np.allclose(got, want, rtol=2 ** -6, atol=1e-3 * float(np.abs(want).max())), ("swiglu", m, packed, ws_bytes)


def _model(dims, seed, dtype, **kw):
    return HipLlama.from_synthetic(dims, seed, std=0.02, head_std=0.05, dtype=dtype, max_slots=512, max_tokens=512, max_logit_rows=448, **kw)


def _seq(g, V, T, hole=7):
    ids = torch.randint(3, V, (T,), generator=g).to(torch.int32)
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
    if T > 12:
        vis[10:, hole] = False                                    # tree mask, not plain causal
    pos = torch.arange(T, dtype=torch.int32)
    return ids, pos, vis


def _judge(got, ref4, ref32, host, rows, label):
    want4 = ref4.forward(*host, n_logit_rows=rows)
    want32 = ref32.forward(*host, n_logit_rows=rows)
    scale = float(want4.abs().max())
    e4, e32, qn = (got - want4).abs(), (got - want32).abs(), (want4 - want32).abs()
    print(f"{label}: W4A8 engine vs W4A8 oracle max {float(e4.max()) / scale:.4f} mean {float(e4.mean()) / scale:.4f}; vs fp32 oracle mean "
          f"{float(e32.mean()) / scale:.4f}; scheme noise mean {float(qn.mean()) / scale:.4f} max {float(qn.max()) / scale:.4f}")
    assert float(e4.mean()) < FP8_VS_NOISE * float(qn.mean()) and float(e4.max()) < float(qn.max())
    assert float(e4.mean()) < float(e32.mean())


@pytest.mark.parametrize("width,dtype", [("small", torch.bfloat16), ("llama7b", torch.bfloat16), ("llama7b", torch.float16)],
                         ids=["small", "llama7b_width", "llama7b_width_fp16"])
def test_fp4_forward_logits_match_the_w4a8_oracle(width, dtype):
    from tests.mxfp4_ref import RefLlamaW4A8
    V = synth.BEAUTY.vocab_size
    dims = synth.LlamaDims(V, 512, 2, 4, 1536) if width == "small" else synth.LlamaDims(V, H7, 3, HEADS7, F7)
    m = _model(dims, 41, dtype)
    sd = m.export_state_dict()
    ref4, ref32 = RefLlamaW4A8(dims, sd, max_slots=512), RefLlama(dims, sd, max_slots=512)
    m.enable_fp4()
    L = dims.n_layers
    g = torch.Generator().manual_seed(9)
    Ts = (20, 60, 121, 228) if (width, dtype) == ("llama7b", torch.bfloat16) else (121,)
    for T in Ts:                                                  # one user per forward
        ids, pos, vis = _seq(g, V, T)
        rows = min(T, 6)
        m.fp4_counters(reset=True)
        got = m.forward_raw(ids.cuda(), pos.cuda(), pos.clone().cuda(), vis_bits_from_bool(vis, 512).cuda(), T, rows).float().cpu()
        torch.cuda.synchronize()
        assert all(c["fp4"] == L and c["other"] == 0 for c in m.fp4_counters().values())
        _judge(got, ref4, ref32, (ids, pos, pos, vis), rows, f"{width} {dtype} T={T}")
    if width == "small":                                          # one batched forward above 256 tokens: 3 users x 100
        seqs, host = [], []
        for i in range(3):
            ids, pos, vis = _seq(g, V, 100, hole=7 + i)
            seqs.append((ids, pos, pos.clone(), vis_bits_from_bool(vis, 512), 100, 6))
            host.append((ids, pos, pos, vis))
        m.fp4_counters(reset=True)
        outs = m.forward_raw_batch(seqs)
        torch.cuda.synchronize()
        assert all(c["fp4"] == L and c["other"] == 0 for c in m.fp4_counters().values())
        for i in range(3):
            _judge(outs[i].float().cpu(), ref4, ref32, host[i], 6, f"batched 300 tokens, user {i}")


def test_fp4_forward_past_the_fused_norm_width_matches_the_w4a8_oracle():
    """hidden 8448 = 33 x 256 > 8192, where no fused norm + e4m3 quantisation exists: the first norm and both residual projections leave 16-bit
    rows and qkv / gate_up quantise them themselves.  Two layers ("down feeds the next layer's norm" and the last layer's down), ffn 512.  One
    40-token sequence alone and beside two fillers in a 300-token forward: all four projections W4A8 in both layers, its logit rows against
    the W4A8 oracle with this file's bar."""
    from tests.mxfp4_ref import RefLlamaW4A8
    dims = synth.LlamaDims(synth.TINY.vocab_size, 8448, 2, 66, 512)
    m = _model(dims, 43, torch.bfloat16)
    sd = m.export_state_dict()
    ref4, ref32 = RefLlamaW4A8(dims, sd, max_slots=512), RefLlama(dims, sd, max_slots=512)
    m.enable_fp4()
    g = torch.Generator().manual_seed(10)
    seqs, host = [], []
    for T in (40, 130, 130):
        ids, pos, vis = _seq(g, dims.vocab_size, T)
        seqs.append((ids, pos, pos.clone(), vis_bits_from_bool(vis, 512), T, 6))
        host.append((ids, pos, pos, vis))
    want4 = ref4.forward(*host[0], n_logit_rows=6)
    want32 = ref32.forward(*host[0], n_logit_rows=6)
    scale, qn = float(want4.abs().max()), (want4 - want32).abs()
    for label, batch in (("40 tokens", seqs[:1]), ("300 tokens", seqs)):
        m.fp4_counters(reset=True)
        got = m.forward_raw_batch(batch)[0].float().cpu()
        torch.cuda.synchronize()
        cnt = m.fp4_counters()
        assert all(c["fp4"] == dims.n_layers and c["other"] == 0 for c in cnt.values()), (label, cnt)
        e4, e32 = (got - want4).abs(), (got - want32).abs()
        print(f"hidden 8448, {label}: W4A8 engine vs W4A8 oracle max {float(e4.max()) / scale:.4f} mean {float(e4.mean()) / scale:.4f}; vs fp32 oracle "
              f"mean {float(e32.mean()) / scale:.4f}; scheme noise mean {float(qn.mean()) / scale:.4f} max {float(qn.max()) / scale:.4f}")
        assert float(e4.mean()) < FP8_VS_NOISE * float(qn.mean()) and float(e4.max()) < float(qn.max()), label
        assert float(e4.mean()) < float(e32.mean()), label


def test_fp4_one_user_bssd_peaked_matches_the_w4a8_oracle():
    """the fp8 tests' `peaked` recipe (residual branches scaled by 3e-4, head rows 3 x wider) at the Llama-7B width, one user"""
    from tests.mxfp4_ref import RefLlamaW4A8
    V = synth.BEAUTY.vocab_size
    layers = 2
    tdims = synth.LlamaDims(V, H7, layers, HEADS7, F7)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448, resid_scale=3e-4)
    tgt = HipLlama.from_synthetic(tdims, 31, std=0.02, head_std=0.06, dtype=torch.bfloat16, num_beams=20, **kw)
    ddims = synth.LlamaDims(V, 256, 2, 4, 704)
    drf = HipLlama.from_synthetic(ddims, 32, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=40, **kw)
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    P = 96
    prompt = synth.synthetic_prompt(P, 411)
    tgt.enable_fp4()
    tgt.fp4_counters(reset=True)
    f4 = BSSD(tgt, drf, {"input_ids": torch.from_numpy(prompt)[None].cuda()}, 4, 4, prefix_allowed_tokens_fn=fn)
    cnt = tgt.fp4_counters()
    assert all(c["other"] == 0 and c["fp4"] == layers * f4["n_target_forwards"] for c in cnt.values()), cnt
    assert f4["n_valid"] == 20 and bool(torch.isfinite(f4["beam_scores"]).all())
    ref = R.BSSD(RefLlamaW4A8(tdims, tgt.export_state_dict(), max_slots=512), RefLlama(ddims, drf.export_state_dict(), max_slots=512),
                 prompt, 4, 4, 20, 40, fn)
    want = {tuple(x) for x in ref["beam_sequence"][:, P:].tolist()}
    got = {tuple(x) for x in f4["beam_sequence"][:, P:].cpu().tolist()}
    print("one-user W4A8 engine vs W4A8 oracle: top-20 overlap", len(want & got) / 20.0)
    assert len(want & got) >= 18
    release_decoders(tgt, drf)


def _small_pair(dtype=torch.bfloat16):
    V = synth.BEAUTY.vocab_size
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448, resid_scale=3e-4)
    tgt = HipLlama.from_synthetic(synth.LlamaDims(V, 512, 2, 4, 1536), 21, std=0.02, head_std=0.06, dtype=dtype, num_beams=20, **kw)
    drf = HipLlama.from_synthetic(synth.LlamaDims(V, 256, 2, 4, 704), 22, std=0.03, head_std=0.2, dtype=dtype, num_beams=40, **kw)
    return tgt, drf


def test_fp4_lock_step_batches_run_fully_in_fp4_and_agree_with_one_user_calls():
    tgt, drf = _small_pair()
    tgt.enable_fp4()
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    U, P = 16, 64
    inputs = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(P, 500 + u))[None].cuda()} for u in range(U)]
    tgt.fp4_counters(reset=True)
    outs = BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn)
    gen = target_generate_batch(tgt, inputs, 4, prefix_allowed_tokens_fn=fn)
    cnt = tgt.fp4_counters()
    assert all(c["other"] == 0 and c["fp4"] > 0 for c in cnt.values()), cnt
    for u in range(U):
        one = BSSD(tgt, drf, inputs[u], 4, 4, prefix_allowed_tokens_fn=fn)
        a = {tuple(x) for x in outs[u]["beam_sequence"][:, P:].cpu().tolist()}
        b = {tuple(x) for x in one["beam_sequence"][:, P:].cpu().tolist()}
        assert len(a & b) >= 18, (u, len(a & b))
        one_g = target_generate(tgt, inputs[u], 4, prefix_allowed_tokens_fn=fn)
        a = {tuple(x) for x in gen[u]["beam_sequence"][:, P:].cpu().tolist()}
        b = {tuple(x) for x in one_g["beam_sequence"][:, P:].cpu().tolist()}
        assert len(a & b) >= 18, ("target_generate", u, len(a & b))
    assert all(c["other"] == 0 for c in tgt.fp4_counters().values())
    release_decoders(tgt, drf)


def test_fp4_refusals_and_repeated_enable():
    lib = _lib.load()
    V = synth.BEAUTY.vocab_size
    small = synth.LlamaDims(V, 256, 1, 4, 512)
    m32 = _model(small, 1, torch.float32)
    with pytest.raises(_lib.AtSpeedError, match="bf16 or fp16"):
        m32.enable_fp4()
    m8 = _model(small, 2, torch.bfloat16)
    m8.enable_fp8()
    with pytest.raises(_lib.AtSpeedError, match="8-bit target"):
        m8.enable_fp4()
    m4 = _model(small, 3, torch.float16)
    m4.enable_fp4()
    m4.enable_fp4()                                               # a second call is a no-op
    with pytest.raises(_lib.AtSpeedError, match="4-bit target"):
        m4.enable_fp8()
    bad = _model(synth.LlamaDims(V, 320, 1, 5, 512), 4, torch.bfloat16)
    assert lib.atspeed_llama_enable_fp4(bad._handle, _lib.stream_ptr(0)) == _lib.ERR_INVALID
    assert b"multiples of 256" in lib.atspeed_last_error()
    g = torch.Generator().manual_seed(2)
    ids, pos, vis = _seq(g, V, 30)
    out = m4.forward_raw(ids.cuda(), pos.cuda(), pos.clone().cuda(), vis_bits_from_bool(vis, 512).cuda(), 30, 2)
    assert bool(torch.isfinite(out).all())
    assert all(c["fp4"] == 1 and c["other"] == 0 for c in m4.fp4_counters().values())


def test_fp4_after_graphs_captured_in_16_bits():
    """graphs on: the decoder's recurring 16-bit forwards are captured (second sight) and replayed; after enable_fp4 the same shapes must run
    the W4A8 projections (the weight scheme is part of the graph key), so the counters advance for every target forward"""
    tgt, drf = _small_pair()
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    inp = {"input_ids": torch.from_numpy(synth.synthetic_prompt(64, 77))[None].cuda()}
    with _lib.switches(graphs=1):
        for _ in range(3):
            BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn)
        tgt.enable_fp4()
        tgt.fp4_counters(reset=True)
        f4 = [BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn) for _ in range(2)]
        torch.cuda.synchronize()
        cnt = tgt.fp4_counters()
    # every forward of the first fp4 call runs eagerly (new key); the second may replay the graphs captured in fp4
    assert all(c["other"] == 0 and c["fp4"] >= 2 * f4[0]["n_target_forwards"] for c in cnt.values()), cnt
    assert torch.equal(f4[0]["beam_sequence"], f4[1]["beam_sequence"])
    release_decoders(tgt, drf)
