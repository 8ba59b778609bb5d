"""BASELINE config 5 (Llama target verification in fp8 on the CDNA4 matrix cores) against ITS OWN oracle: `oracle.llama_ref.RefLlama(w8a8=True)`
restates the W8A8 scheme (OCP e4m3, weights per output row, activations per token, fp32 accumulate) on the CPU.  The reference's 8-bit
target is bitsandbytes LLM.int8 (`code/inference.py:88`), third-party, unpinned and absent offline: config 5 is "parity unpinned"
against the reference and pinned to this restatement.

Shapes are chosen so that `ats_gemm_fp8_applies` holds for ALL FOUR layer projections in EVERY forward (the r1 test only reached
gate_up in the first round), and the engine's own counters (`atspeed_llama_fp8_counters`) assert it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import atspeed_amd
from atspeed_amd import synth
from atspeed_amd.beamSD import BSSD_batch, release_decoders
from atspeed_amd.model import HipLlama, vis_bits_from_bool
from oracle import beamsd_ref as R
from oracle.llama_ref import RefLlama

H, F, HEADS, LAYERS = 2048, 5632, 16, 2          # every projection fills >= 60 % of a round of 256 CUs from ~2.5 k tokens on
# Tolerance.  e4m3 keeps 3 mantissa bits: the scheme's own noise (W8A8 oracle against the fp32 oracle on the same weights) is ~3.5 % (mean)
# and ~20 % (max) of the largest |logit| at these dims.  The engine quantises bf16-rounded activations, the oracle fp32 ones: a value
# within 2^-9 of an e4m3 rounding boundary (step 2^-4) takes the neighbouring code, so ~3 % of all codes differ by one step and the two
# implementations differ by a fixed fraction of that noise (expected ~0.6 x, by the flip-rate argument).  The bar: closer to the W8A8
# oracle than FP8_VS_NOISE x the scheme's noise, and closer to it than to the fp32 oracle.
FP8_VS_NOISE = 0.85


def _fill(t):
    return t * 100 // (((t + 255) // 256) * 256)


def _fp8_applies(m, n, k):                        # gemm.hip: ats_gemm_fp8_applies, the ring kernel's rule (m <= 256 takes the weight-streaming form)
    tn = (n + 255) // 256
    return m >= 512 and k % 256 == 0 and (_fill(tn * ((m + 255) // 256)) >= 60 or _fill(tn * ((m + 127) // 128)) >= 60)


PROJ_SHAPES = ((3 * H, H), (H, H), (2 * F, H), (H, F))
# config 5 at its real width: the Llama-7B layer (hidden 4096, ffn 11008, 32 heads x 128: K = 4096 and K = 11008 projections, the fused
# qkv + RoPE epilogue of the fp8 ring kernel), a few layers deep so that the CPU W8A8 oracle finishes in seconds
H7, F7, HEADS7 = 4096, 11008, 32


# past hidden 8192 there is no fused norm + e4m3 quantisation: every quantised consumer of a norm gets 16-bit rows and quantises them itself.
# 8448 = 33 x 256 is the first such width enable_fp8 takes; two layers reach both "down feeds the next layer's norm" and the last layer's down;
# ffn 512 is the smallest with which all four projections are W8A8 shapes at one-user sizes (the weight-streaming form wants K >= 512)
WIDE = synth.LlamaDims(synth.TINY.vocab_size, 8448, 2, 66, 512)


def _target(dtype=torch.bfloat16, V=synth.BEAUTY.vocab_size, width="small", layers=LAYERS, **kw):
    dims = {"small": synth.LlamaDims(V, H, layers, HEADS, F), "llama7b": synth.LlamaDims(V, H7, layers, HEADS7, F7), "wide": WIDE}[width]
    return dims, HipLlama.from_synthetic(dims, 31, std=0.03 if width == "small" else 0.02, head_std=0.2 if width == "small" else 0.05, dtype=dtype,
                                         max_slots=512, max_tokens=512, max_logit_rows=448, **kw)


@pytest.mark.parametrize("width,layers,dtype", [("small", LAYERS, torch.bfloat16), ("llama7b", 3, torch.bfloat16), ("llama7b", 3, torch.float16)],
                         ids=["hidden2048", "llama7b_width", "llama7b_width_fp16"])
def test_fp8_forward_logits_match_the_w8a8_oracle(width, layers, dtype):
    """fp16: the reference's dtype combination (inference.py:75-91: fp16 checkpoints, 8-bit target) -- the e4m3 copies come from the fp16 weight
    values, the activations between the W8A8 projections are fp16; the oracle is RefLlama(w8a8=True) on those fp16-valued weights."""
    dims, m = _target(dtype=dtype, width=width, layers=layers)
    LAYERS_ = layers
    sd = m.export_state_dict()                                    # the 16-bit weight values the device holds (and quantises)
    ref8, ref32 = RefLlama(dims, sd, max_slots=512, w8a8=True), RefLlama(dims, sd, max_slots=512)
    m.enable_fp8()
    g = torch.Generator().manual_seed(5)
    V = dims.vocab_size
    seqs, host = [], []
    for i in range(32):                                           # 32 x 100 tokens = 3200 rows: fp8 applies to all four projections
        T = 100
        ids = torch.cat((torch.randint(3, 32000, (T - 30,), generator=g), torch.randint(32000, V, (30,), generator=g))).to(torch.int32)
        vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
        vis[40:, 7 + i % 9] = False                               # a hidden slot: tree mask, not plain causal
        pos = torch.arange(T, dtype=torch.int32)
        seqs.append((ids, pos, pos.clone(), vis_bits_from_bool(vis, 512), T, 6))
        host.append((ids, pos, pos, vis))
    shapes = PROJ_SHAPES if width == "small" else ((3 * H7, H7), (H7, H7), (2 * F7, H7), (H7, F7))
    assert all(_fp8_applies(3200, n, k) for n, k in shapes)
    m.fp8_counters(reset=True)
    m.rope_fused_launches(reset=True)
    outs = m.forward_raw_batch(seqs)
    torch.cuda.synchronize()
    cnt = m.fp8_counters()
    assert all(c["fp8"] == LAYERS_ and c["other"] == 0 for c in cnt.values()), cnt
    if width == "llama7b":
        assert m.rope_fused_launches() == LAYERS_                 # head_dim 128: RoPE + the KV scatter ride in the fp8 qkv projection's epilogue
    worst = []
    for i in (0, 13, 31):
        want8 = ref8.forward(*host[i], n_logit_rows=6)
        want32 = ref32.forward(*host[i], n_logit_rows=6)
        got = outs[i].float().cpu()
        scale = float(want8.abs().max())
        e8, e32 = (got - want8).abs(), (got - want32).abs()
        qn = (want8 - want32).abs()                               # the quantisation noise of the scheme itself, on this sequence
        worst.append((float(e8.max()) / scale, float(e8.mean()) / scale, float(e32.mean()) / scale, float(qn.mean()) / scale, float(qn.max()) / scale))
    print("fp8 engine vs W8A8 oracle (max, mean), vs fp32 oracle (mean), W8A8-vs-fp32 oracle (mean, max), relative to max|logit|:", worst)
    for e8_max, e8_mean, e32_mean, qn_mean, qn_max in worst:
        assert e8_mean < FP8_VS_NOISE * qn_mean and e8_max < qn_max
        assert e8_mean < e32_mean, "the W8A8 oracle must explain the fp8 engine better than the unquantised one"


def test_fp8_forward_past_the_fused_norm_width_matches_the_w8a8_oracle():
    """hidden 8448 > 8192: the first norm and both residual projections leave 16-bit rows and qkv / gate_up quantise them themselves (every
    other model of the suite takes its e4m3 rows from the fused norm).  One 40-token sequence alone (the one-user kernels) and beside two
    fillers in a 300-token forward (257-511 tokens: the ring kernel for every K % 256 == 0): all four projections W8A8 in both layers, its
    logit rows against the W8A8 oracle with this file's bar."""
    dims, m = _target(width="wide")
    sd = m.export_state_dict()
    ref8, ref32 = RefLlama(dims, sd, max_slots=512, w8a8=True), RefLlama(dims, sd, max_slots=512)
    m.enable_fp8()
    g = torch.Generator().manual_seed(8)
    seqs, host = [], []
    for T in (40, 130, 130):
        ids = torch.randint(3, dims.vocab_size, (T,), generator=g).to(torch.int32)
        vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
        vis[20:, 7] = False                                       # a hidden slot: tree mask, not plain causal
        pos = torch.arange(T, dtype=torch.int32)
        seqs.append((ids, pos, pos.clone(), vis_bits_from_bool(vis, 512), T, 6))
        host.append((ids, pos, pos, vis))
    want8 = ref8.forward(*host[0], n_logit_rows=6)
    want32 = ref32.forward(*host[0], n_logit_rows=6)
    scale, qn = float(want8.abs().max()), (want8 - want32).abs()
    for label, batch in (("40 tokens", seqs[:1]), ("300 tokens", seqs)):
        m.fp8_counters(reset=True)
        got = m.forward_raw_batch(batch)[0].float().cpu()
        torch.cuda.synchronize()
        cnt = m.fp8_counters()
        assert all(c["fp8"] == dims.n_layers and c["other"] == 0 for c in cnt.values()), (label, cnt)
        e8, e32 = (got - want8).abs(), (got - want32).abs()
        print(f"hidden 8448, {label}: fp8 engine vs W8A8 oracle max {float(e8.max()) / scale:.4f} mean {float(e8.mean()) / scale:.4f}; vs fp32 oracle "
              f"mean {float(e32.mean()) / scale:.4f}; scheme noise mean {float(qn.mean()) / scale:.4f} max {float(qn.max()) / scale:.4f}")
        assert float(e8.mean()) < FP8_VS_NOISE * float(qn.mean()) and float(e8.max()) < float(qn.max()), label
        assert float(e8.mean()) < float(e32.mean()), label


def test_fp8_bssd_runs_every_projection_in_fp8_in_every_round_and_matches_the_w8a8_oracle():
    U, P = 144, 64
    rounds = [U * (P + 120), U * 100, U * 60, U * 20]
    assert all(_fp8_applies(mm, n, k) for mm in rounds for n, k in PROJ_SHAPES)       # also the final single step (20 tokens per user)
    V = synth.BEAUTY.vocab_size
    tdims, tgt = _target(num_beams=20)
    ddims = synth.LlamaDims(V, 256, 2, 4, 704)
    drf = HipLlama.from_synthetic(ddims, 32, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=40, max_slots=512, max_tokens=512, max_logit_rows=448)
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    prompts = [synth.synthetic_prompt(P, 300 + u) for u in range(U)]
    inputs = [{"input_ids": torch.from_numpy(p)[None].cuda()} for p in prompts]
    bf = BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn)
    tgt.enable_fp8()
    tgt.fp8_counters(reset=True)
    f8 = BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn)
    cnt = tgt.fp8_counters()
    n_fwd = max(o["n_target_forwards"] for o in f8)
    assert all(o["n_target_forwards"] == n_fwd for o in f8)                           # unrelated random weights: no step accepted, 3 rounds + 1
    assert all(c["other"] == 0 and c["fp8"] == LAYERS * n_fwd for c in cnt.values()), cnt
    assert all(o["n_valid"] == 20 and bool(torch.isfinite(o["beam_scores"]).all()) for o in f8)
    # a few users against the oracle with the W8A8 target (fp32 draft on the draft's bf16 weight values)
    rt = RefLlama(tdims, tgt.export_state_dict(), max_slots=512, w8a8=True)
    rd = RefLlama(ddims, drf.export_state_dict(), max_slots=512)
    overlap8, overlap_bf, dscore = [], [], []
    for u in (0, 71, 143):
        ref = R.BSSD(rt, rd, prompts[u], 4, 4, 20, 40, fn)
        want = {tuple(x) for x in ref["beam_sequence"][:, P:].tolist()}
        got8 = {tuple(x) for x in f8[u]["beam_sequence"][:, P:].cpu().tolist()}
        gotb = {tuple(x) for x in bf[u]["beam_sequence"][:, P:].cpu().tolist()}
        overlap8.append(len(want & got8) / 20.0)
        overlap_bf.append(len(want & gotb) / 20.0)
        dscore.append(abs(float(f8[u]["beam_scores"][0]) - float(ref["beam_scores"][0])))
        assert f8[u]["n_run"] == ref["n_run"] and f8[u]["total_accept_steps"] == ref["total_accept_steps"]
    print("fp8 engine vs W8A8 oracle: top-20 overlap", overlap8, "(bf16 engine vs the same oracle:", overlap_bf, ") best-score diff", dscore)
    assert np.mean(overlap8) >= 0.5
    release_decoders(tgt, drf)


@pytest.mark.parametrize("width", ["small", "llama7b"], ids=["hidden2048", "llama7b_width"])
def test_fp8_accept_length_drift_on_an_aligned_pair(width):
    """Accepted length of the fp8 target against the bf16 target on weights where acceptance is non-trivial (draft and target share a
    bigram table, residual branches scaled: HipLlama.from_synthetic(align_to=...)): the drift config 5 reports, with a bound.  The
    residual scale is the first of a short list at which the bf16 pair accepts a mixed number of steps.  llama7b_width: a full-width
    (hidden 4096 / ffn 11008, 4 layers) target against the Llama-68M-shaped draft, i.e. bench.py's aligned pair with fewer layers."""
    U, P = (144, 64) if width == "small" else (64, 64)
    V = synth.BEAUTY.vocab_size
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    kw = dict(dtype=torch.bfloat16, max_slots=512, max_tokens=512, max_logit_rows=448)
    inputs = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(P, 900 + u))[None].cuda()} for u in range(U)]
    mean_acc = lambda outs: sum(o["total_accept_steps"] for o in outs) / max(1, sum(o["n_run"] for o in outs))
    seen = {}
    ddims = synth.LlamaDims(V, 256, 2, 4, 704) if width == "small" else synth.llama_68m(V)
    tdims = synth.LlamaDims(V, H, LAYERS, HEADS, F) if width == "small" else synth.llama_7b(V, 4)
    for rs in ((3e-4, 5e-4, 1e-3) if width == "small" else (3e-5, 1e-4, 3e-4, 1e-3)):
        drf = HipLlama.from_synthetic(ddims, 32, std=0.02, head_std=0.02, num_beams=40, resid_scale=rs, **kw)
        tgt = HipLlama.from_synthetic(tdims, 31, std=0.02, head_std=0.02, num_beams=20, resid_scale=rs, align_to=drf, **kw)
        a_bf = mean_acc(BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn))
        seen[rs] = [a_bf]
        if 0.2 < a_bf < 2.8:
            tgt.enable_fp8()
            a_f8 = mean_acc(BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn))
            seen[rs].append(a_f8)
        release_decoders(tgt, drf)
        del tgt, drf
        if len(seen[rs]) == 2:
            break
    print("mean accepted steps per verification by residual scale, [bf16 target, fp8 target]:", seen)
    mixed = [v for v in seen.values() if len(v) == 2]
    assert mixed, f"no residual scale gave mixed acceptance: {seen}"
    assert abs(mixed[0][1] - mixed[0][0]) <= 0.5


# ------------------------------------------------------------------ config 5 in the reference's own regime: ONE user per call (round 5)
@pytest.mark.parametrize("T,dtype", [(121, torch.bfloat16), (228, torch.bfloat16), (20, torch.bfloat16), (228, torch.float16), (60, torch.float16)],
                         ids=["121", "228", "20", "228_fp16", "60_fp16"])
def test_fp8_one_user_forward_at_llama7b_width_matches_the_w8a8_oracle(T, dtype):
    """VERDICT r4 missing #1: the reference's 8-bit target runs every forward at batch 1 (inference.py:86-91, beamSD.py:221: T = 228 for the
    first verification, K + dl * DK = 60-140 later, K = 20 for the final step); here m < 512 used to fall back to bf16 silently.  One
    sequence at hidden 4096 / ffn 11008 / 32 heads x 128 through the weight-streaming W8A8 kernels (gemm_wdma_kernel<..., F8>): every layer
    projection counted as fp8, logits against the W8A8 oracle with the batched path's tolerance."""
    from atspeed_amd import _lib
    import ctypes as C
    layers = 3
    dims, m = _target(dtype=dtype, width="llama7b", layers=layers)
    sd = m.export_state_dict()
    ref8, ref32 = RefLlama(dims, sd, max_slots=512, w8a8=True), RefLlama(dims, sd, max_slots=512)
    m.enable_fp8()
    g = torch.Generator().manual_seed(6)
    V = dims.vocab_size
    ids = torch.cat((torch.randint(3, 32000, (max(T - 30, 1),), generator=g), torch.randint(32000, V, (T - max(T - 30, 1),), generator=g))).to(torch.int32)
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
    if T > 12:
        vis[10:, 7] = False                                       # tree mask, not plain causal
    pos = torch.arange(T, dtype=torch.int32)
    rows = min(T, 6)
    m.fp8_counters(reset=True)
    cnt = (C.c_int64 * 16)()
    _lib.load().atspeed_gemm_path_counters(cnt, 16, 1)
    got = m.forward_raw(ids.cuda(), pos.cuda(), pos.clone().cuda(), vis_bits_from_bool(vis, 512).cuda(), T, rows).float().cpu()
    torch.cuda.synchronize()
    fc = m.fp8_counters()
    assert all(c["fp8"] == layers and c["other"] == 0 for c in fc.values()), fc
    _lib.load().atspeed_gemm_path_counters(cnt, 16, 0)
    assert cnt[7] == 2 * layers and cnt[8] == 2 * layers and cnt[6] == 0, list(cnt)  # gate_up and qkv without split; o_proj, down cut in K; no ring launch
    want8 = ref8.forward(ids, pos, pos, vis, n_logit_rows=rows)
    want32 = ref32.forward(ids, pos, pos, vis, n_logit_rows=rows)
    scale = float(want8.abs().max())
    e8, e32, qn = (got - want8).abs(), (got - want32).abs(), (want8 - want32).abs()
    print(f"T={T}: fp8 one-user engine vs W8A8 oracle max {float(e8.max()) / scale:.4f} mean {float(e8.mean()) / scale:.4f}; vs fp32 oracle mean "
          f"{float(e32.mean()) / scale:.4f}; scheme noise mean {float(qn.mean()) / scale:.4f} max {float(qn.max()) / scale:.4f}")
    assert float(e8.mean()) < FP8_VS_NOISE * float(qn.mean()) and float(e8.max()) < float(qn.max())
    assert float(e8.mean()) < float(e32.mean())


@pytest.mark.parametrize("recipe,dtype", [("flat", torch.bfloat16), ("peaked", torch.bfloat16), ("peaked", torch.float16)], ids=["flat", "peaked", "peaked_fp16"])
def test_fp8_one_user_bssd_runs_every_projection_of_every_forward_in_fp8(recipe, dtype):
    """A ONE-user BSSD call (the reference's loop, inference.py:162-176) with the fp8 target at the Llama-7B width: every layer projection of
    every target forward -- first verification, later rounds, final single step -- is counted as fp8 (`other == 0`), and the oracle with a
    W8A8 target agrees on n_run / accepted steps and on most of the top-20.  `flat`: the random-init recipe of the other tests, whose flat logits put
    most of the top-20 within the scheme's own noise (overlap >= 8 of 20 is all that can be asked).  `peaked` (round 6, VERDICT r5 weak #1c): the recipe
    of tests/test_decisions_gpu.py's verifiable headline regime -- residual branches scaled by 3e-4, head rows 3 x wider, draft and target still
    unrelated -- where the candidates stand clear of the quantisation noise: at least 18 of the oracle's 20 items, in bf16 and in the reference's fp16."""
    from atspeed_amd.beamSD import BSSD
    V = synth.BEAUTY.vocab_size
    layers = 2
    extra = dict(resid_scale=3e-4) if recipe == "peaked" else {}
    if recipe == "peaked":
        tdims = synth.LlamaDims(V, H7, layers, HEADS7, F7)
        tgt = HipLlama.from_synthetic(tdims, 31, std=0.02, head_std=0.06, dtype=dtype, num_beams=20, max_slots=512, max_tokens=512, max_logit_rows=448, **extra)
    else:
        tdims, tgt = _target(dtype=dtype, width="llama7b", layers=layers, num_beams=20)
    ddims = synth.LlamaDims(V, 256, 2, 4, 704)
    drf = HipLlama.from_synthetic(ddims, 32, std=0.03, head_std=0.2, dtype=dtype, num_beams=40, max_slots=512, max_tokens=512, max_logit_rows=448, **extra)
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    P = 96
    prompt = synth.synthetic_prompt(P, 411)
    inp = {"input_ids": torch.from_numpy(prompt)[None].cuda()}
    bf = BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn)
    tgt.enable_fp8()
    tgt.fp8_counters(reset=True)
    f8 = BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn)
    cnt = tgt.fp8_counters()
    assert all(c["other"] == 0 and c["fp8"] == layers * f8["n_target_forwards"] for c in cnt.values()), cnt
    assert f8["n_valid"] == 20 and bool(torch.isfinite(f8["beam_scores"]).all())
    ref = R.BSSD(RefLlama(tdims, tgt.export_state_dict(), max_slots=512, w8a8=True), RefLlama(ddims, drf.export_state_dict(), max_slots=512),
                 prompt, 4, 4, 20, 40, fn)
    want = {tuple(x) for x in ref["beam_sequence"][:, P:].tolist()}
    got8 = {tuple(x) for x in f8["beam_sequence"][:, P:].cpu().tolist()}
    gotb = {tuple(x) for x in bf["beam_sequence"][:, P:].cpu().tolist()}
    print("one-user fp8 engine vs W8A8 oracle: top-20 overlap", len(want & got8) / 20.0, "(bf16 engine:", len(want & gotb) / 20.0, ")")
    assert f8["n_run"] == ref["n_run"] and f8["total_accept_steps"] == ref["total_accept_steps"]
    assert len(want & got8) >= (18 if recipe == "peaked" else 8)
    release_decoders(tgt, drf)
