"""End-to-end GPU parity: HipLlama forward vs the oracle Llama (fp32 logits within 1e-3) and
BSSD / target_generate vs the golden vectors produced by the REAL reference (token ids,
per-round n_matches and draft candidate ids bit-exact; scores within 1e-3)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import atspeed_amd
from atspeed_amd import synth
from atspeed_amd.beamSD import BSSD, last_trace, release_decoders, target_generate
from atspeed_amd.model import HipLlama, vis_bits_from_bool
from oracle import beamsd_ref as R
from oracle.llama_ref import RefLlama
from tests.golden.cases import CASES, build_case_inputs

LOGIT_TOL = 1e-3    # BASELINE.json north star: fp32 logits within 1e-3
SCORE_TOL = 1e-3


def test_forward_fp32_logits_match_oracle_with_tree_mask():
    ci = build_case_inputs(CASES[0])
    dims = ci["target_dims"]
    m = HipLlama.from_state_dict(dims, ci["target_sd"], torch.float32, max_slots=256, max_tokens=256, max_logit_rows=128)
    ref = RefLlama(dims, ci["target_sd"])
    P, B = 24, 7
    ids0 = torch.from_numpy(ci["prompt"])
    inp = R._causal_inputs(ids0)
    l_ref0 = ref.forward(inp.ids, inp.pos, inp.slots, inp.vis)
    i32 = lambda t: t.to(torch.int32).cuda()
    l0 = m.forward_raw(i32(inp.ids), i32(inp.pos), i32(inp.slots), vis_bits_from_bool(inp.vis, 256).cuda(), P, P)
    np.testing.assert_allclose(l0.cpu().numpy(), l_ref0.numpy(), atol=LOGIT_TOL, rtol=0)
    assert float((l0.cpu() - l_ref0).abs().max()) < 1e-4          # in practice ~1e-5
    # second forward: B tree tokens over the cached prompt, one prompt slot hidden
    ids1 = torch.randint(32000, dims.vocab_size, (B,), generator=torch.Generator().manual_seed(1))
    vis1 = torch.cat((torch.ones(B, P, dtype=torch.bool), torch.eye(B, dtype=torch.bool)), 1)
    vis1[:, 5] = False
    l_ref1 = ref.forward(ids1, torch.full((B,), P), torch.arange(P, P + B), vis1, n_logit_rows=3)
    l1 = m.forward_raw(i32(ids1), i32(torch.full((B,), P)), i32(torch.arange(P, P + B)), vis_bits_from_bool(vis1, 256).cuda(), P + B, 3)
    np.testing.assert_allclose(l1.cpu().numpy(), l_ref1.numpy(), atol=LOGIT_TOL, rtol=0)


# head_dim 64 and 128 with >= 512 attention workgroups (the lock-step kernels); hidden 3072: the one-sequence forwards take the split-K
# ring GEMM for qkv (N = 9216) with the slab-summing RoPE, the batched one the plain ring GEMM + reduce-free RoPE
@pytest.mark.parametrize("hidden,heads,n_seq", [(768, 12, 48), (768, 6, 96), (3072, 24, 24)])
def test_batched_forward_equals_per_sequence_forwards_bf16(hidden, heads, n_seq):
    """`forward_raw_batch` (one segment and KV arena per sequence: the engine's lock-step form, 128-row query tiles, 32-rows-per-wave
    attention with LDS-DMA, ring GEMMs over all rows) against the same sequences one per forward (small-grid kernels): bf16 logits agree
    to bf16 noise, and both are tree forwards (a hidden prompt slot, ragged lengths)."""
    V = 32000 + 256
    dims = synth.LlamaDims(V, hidden, 2, heads, 1536)
    m = HipLlama.from_synthetic(dims, 77, dtype=torch.bfloat16, max_slots=256, max_tokens=256, max_logit_rows=256, device=torch.device("cuda", 0))
    g = torch.Generator().manual_seed(3)
    seqs = []
    for i in range(n_seq):
        T = 64 if i < 2 else int(torch.randint(9, 70, (1,), generator=g))      # 33+ tokens: the split-K mode of one-sequence forwards
        ids = torch.randint(3, V, (T,), generator=g).to(torch.int32)
        vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
        if T > 12:
            vis[8:, 3] = False                                     # a hidden slot: not plain causal attention
        seqs.append((ids, torch.arange(T, dtype=torch.int32), torch.arange(T, dtype=torch.int32), vis_bits_from_bool(vis, 256), T, 4))
    outs = m.forward_raw_batch(seqs)
    torch.cuda.synchronize()
    for i in (0, 1, n_seq // 2, n_seq - 1):
        ids, pos, slots, bits, T, nl = seqs[i]
        one = m.forward_raw(ids.cuda(), pos.cuda(), slots.cuda(), bits.cuda(), T, nl)
        a, b = outs[i].float().cpu().numpy(), one.float().cpu().numpy()
        assert a.shape == b.shape == (4, V)
        scale = float(np.abs(b).max())
        np.testing.assert_allclose(a, b, atol=0.03 * scale, rtol=0)
        assert float(np.abs(a - b).mean()) < 0.004 * scale


def _models(ci, case, dtype=torch.float32):
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    t = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], dtype, num_beams=case["K"], **kw)
    d = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], dtype, num_beams=case["DK"], **kw)
    return t, d


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_bssd_and_target_generate_equal_reference(case, bssd_golden):
    gold = bssd_golden[case["name"]]
    ci = build_case_inputs(case)
    tgt, drf = _models(ci, case)
    P = len(ci["prompt"])
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}
    procs = ci["procs"] or None          # extra logits processors (the LogitsProcessorList argument of beamSD.py:465,549)
    tg = target_generate(tgt, inputs, case["max_new_tokens"], logits_processor=procs, prefix_allowed_tokens_fn=ci["fn"])
    assert tg["beam_sequence"].shape == (case["K"], P + case["max_new_tokens"]) and tg["beam_sequence"].dtype == torch.int64
    assert (tg["beam_sequence"][:, :P].cpu() == torch.from_numpy(ci["prompt"])[None]).all()
    assert tg["beam_sequence"][:, P:].cpu().tolist() == gold["tg_tokens"]
    np.testing.assert_allclose(tg["beam_scores"].cpu().numpy(), gold["tg_scores"], atol=SCORE_TOL, rtol=0)
    out = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], logits_processor=procs, prefix_allowed_tokens_fn=ci["fn"])
    for key in ("beam_sequence", "beam_scores", "n_run", "total_accept_steps", "total_accept_tokens", "ave_accept_tokens",
                "draft_time_cost", "target_time_cost", "verify_time_cost", "time_cost"):
        assert key in out                                                 # keys consumed at inference.py:179-187
    # lossless: identical to plain beam search (also pins the case the reference itself cannot run)
    assert out["beam_sequence"][:, P:].cpu().tolist() == gold["tg_tokens"]
    np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), gold["tg_scores"], atol=SCORE_TOL, rtol=0)
    if "reference_error" in gold:
        return
    assert out["beam_sequence"][:, P:].cpu().tolist() == gold["bssd_tokens"]
    np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), gold["bssd_scores"], atol=SCORE_TOL, rtol=0)
    assert out["n_run"] == gold["n_run"]
    assert out["total_accept_steps"] == gold["total_accept_steps"]
    assert out["total_accept_tokens"] == gold["total_accept_tokens"]
    assert out["ave_accept_tokens"] == pytest.approx(gold["ave_accept_tokens"])
    if procs:                            # host path (Python callables per step): real stage times, no device trace
        assert out["accept_steps"] == [r["n_matches"] for r in gold["rounds"]]
        assert out["draft_time_cost"] > 0 and out["target_time_cost"] > 0 and out["verify_time_cost"] > 0
        return
    tr = last_trace(tgt, drf)
    assert [r["n_matches"] for r in tr] == [r["n_matches"] for r in gold["rounds"]]
    assert [r["draft_len"] for r in tr] == [r["draft_len"] for r in gold["rounds"]]
    for r, g in zip(tr, gold["rounds"]):
        for ids, gids, n in zip(r["draft_ids"], g["draft_ids"], g["step_len"][1:]):
            assert [x for x in ids if x >= 0] == gids                    # step_len = number of real beams
            assert len(gids) == n


def test_bssd_bf16_is_lossless_against_own_target_generate():
    """bf16 engine: BSSD must reproduce the engine's own plain beam search (same kernels, same
    rounding) — the lossless property of the greedy branch, at the 68M-like / wider dims."""
    V = synth.BEAUTY.vocab_size
    tdims = synth.LlamaDims(V, 512, 2, 8, 1376)
    ddims = synth.LlamaDims(V, 256, 2, 4, 704)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_synthetic(tdims, 11, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=20, **kw)
    drf = HipLlama.from_synthetic(ddims, 12, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=40, **kw)
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    for u in range(3):
        prompt = synth.synthetic_prompt(60 + 17 * u, 100 + u)
        inputs = {"input_ids": torch.from_numpy(prompt)[None].cuda()}
        a = BSSD(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn)
        b = target_generate(tgt, inputs, 4, prefix_allowed_tokens_fn=fn)
        sa, sb = a["beam_scores"].cpu().numpy(), b["beam_scores"].cpu().numpy()
        np.testing.assert_allclose(sa, sb, atol=5e-2, rtol=0)
        ta, tb = a["beam_sequence"][:, len(prompt):].cpu().tolist(), b["beam_sequence"][:, len(prompt):].cpu().tolist()
        # identical item sets unless two beams are closer than the bf16 noise
        gaps = np.abs(np.diff(sb))
        if gaps.min() > 5e-2:
            assert ta == tb
        assert len({tuple(x) for x in ta} & {tuple(x) for x in tb}) >= 18


@pytest.mark.parametrize("name", ["k20_dk40_sigma01_s7", "k20_dk40_nomask", "k8_dk16_chain"])
def test_bssd_batch_equals_sequential_calls(name, bssd_golden):
    """Interleaved multi-user decoding (one stream per user) must give exactly the per-user results."""
    from atspeed_amd.beamSD import BSSD_batch
    case = [c for c in CASES if c["name"] == name][0]       # position mask, no mask at all (row top-k + free expand), chained whole-sentence trie
    ci = build_case_inputs(case)
    tgt, drf = _models(ci, case)
    users = [synth.synthetic_prompt(18 + 5 * u, 900 + u) for u in range(5)]
    if case["mask"] == "chain":                              # the whole-sentence trie only knows its own prompt
        users = [ci["prompt"]] * 5
    users[2] = ci["prompt"]                                  # one user is the golden case itself
    inputs = [{"input_ids": torch.from_numpy(p)[None].cuda()} for p in users]
    seq = [BSSD(tgt, drf, inp, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"]) for inp in inputs]
    bat = BSSD_batch(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    assert len(bat) == len(seq)
    for a, b in zip(seq, bat):
        assert torch.equal(a["beam_sequence"], b["beam_sequence"])
        np.testing.assert_allclose(a["beam_scores"].cpu().numpy(), b["beam_scores"].cpu().numpy(), atol=1e-4, rtol=0)
        assert (a["n_run"], a["total_accept_steps"], a["accept_steps"]) == (b["n_run"], b["total_accept_steps"], b["accept_steps"])
    gold = bssd_golden[case["name"]]
    P = len(ci["prompt"])
    assert bat[2]["beam_sequence"][:, P:].cpu().tolist() == gold["bssd_tokens"]
    assert [bat[2]["n_run"], bat[2]["total_accept_steps"]] == [gold["n_run"], gold["total_accept_steps"]]
    # a second batch on the same lanes (state reuse) gives the same answer
    bat2 = BSSD_batch(tgt, drf, inputs[::-1], case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    for a, b in zip(seq[::-1], bat2):
        assert torch.equal(a["beam_sequence"], b["beam_sequence"])


def test_games_strict_trie_many_users_batch():
    """BASELINE config 3 shape (Games vocabulary, strict item trie, many users per batch) on small models: every user
    of a 48-user lock-step batch must equal its own single-user decode, a few users are checked against the oracle,
    and every recommended item must be a real item of the index (the trie allows nothing else)."""
    from atspeed_amd.beamSD import BSSD_batch
    from atspeed_amd.generation_trie import SuffixTrieConstraint, Trie
    vocab = synth.GAMES
    V = vocab.vocab_size
    tdims = synth.LlamaDims(V, 256, 2, 4, 704)
    ddims = synth.LlamaDims(V, 128, 2, 2, 352)
    tsd = synth.synthetic_state_dict(tdims, 21, std=0.05, head_std=0.3)
    dsd = synth.synthetic_state_dict(ddims, 22, std=0.05, head_std=0.3)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_state_dict(tdims, tsd, torch.float32, num_beams=20, **kw)
    drf = HipLlama.from_state_dict(ddims, dsd, torch.float32, num_beams=40, **kw)
    items = synth.synthetic_items(vocab)
    item_set = {tuple(int(t) for t in it) for it in items}
    fn = SuffixTrieConstraint(Trie([[1] + [int(t) for t in it] + [2] for it in items]), synth.RESPONSE_SEP, 1)
    n_users = 48
    prompts = [synth.synthetic_prompt(20 + (7 * u) % 40, 5000 + u) for u in range(n_users)]
    inputs = [{"input_ids": torch.from_numpy(p)[None].cuda()} for p in prompts]
    bat = BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn)
    assert len(bat) == n_users
    for u in (0, 7, 23, 47):
        one = BSSD(tgt, drf, inputs[u], 4, 4, prefix_allowed_tokens_fn=fn)
        assert torch.equal(one["beam_sequence"], bat[u]["beam_sequence"])
        assert (one["n_run"], one["accept_steps"]) == (bat[u]["n_run"], bat[u]["accept_steps"])
    for u in (3, 31):
        ref = R.BSSD(RefLlama(tdims, tsd), RefLlama(ddims, dsd), prompts[u], 4, 4, 20, 40, fn)
        P = len(prompts[u])
        nv = bat[u]["n_valid"]
        assert bat[u]["beam_sequence"][:nv, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()[:nv]
        assert bat[u]["n_run"] == ref["n_run"] and bat[u]["total_accept_steps"] == ref["total_accept_steps"]
    for u in range(n_users):
        P = len(prompts[u])
        toks = bat[u]["beam_sequence"][: bat[u]["n_valid"], P:].cpu().tolist()
        assert bat[u]["n_valid"] >= 1
        assert all(tuple(t) in item_set for t in toks), "a beam left the item trie"
        assert len({tuple(t) for t in toks}) == len(toks), "duplicate items in one user's beams"
        sc = bat[u]["beam_scores"][: bat[u]["n_valid"]].cpu().numpy()
        assert np.all(np.diff(sc) <= 1e-6), "beams must be sorted by score"


def test_mask_free_search_many_users_batch_bf16():
    """`prefix_allowed_tokens_fn=None` at batch scale on the bf16 engine: 48 users in lock step (ring GEMMs, the lm_head's fused normaliser
    with EVERY logit tile stored, `row_topk_kernel` over all logit rows of a round) against the same engine one user at a time (small-M
    kernels, plain lm_head + streaming LSE): same n_run / accept_steps, item sets equal up to bf16 near-ties (scores agree to bf16 noise), and
    two users in fp32 against the oracle bit for bit."""
    from atspeed_amd.beamSD import BSSD_batch
    V = synth.GAMES.vocab_size
    tdims = synth.LlamaDims(V, 256, 2, 4, 704)
    ddims = synth.LlamaDims(V, 128, 2, 2, 352)
    tsd = synth.synthetic_state_dict(tdims, 21, std=0.05, head_std=0.3)
    dsd = synth.perturbed_state_dict(synth.synthetic_state_dict(ddims, 22, std=0.05, head_std=0.3), 23, 0.0)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    n_users = 48
    prompts = [synth.synthetic_prompt(20 + (7 * u) % 40, 6000 + u) for u in range(n_users)]
    inputs = [{"input_ids": torch.from_numpy(p)[None].cuda()} for p in prompts]
    for dtype in (torch.float32, torch.bfloat16):
        tgt = HipLlama.from_state_dict(tdims, tsd, dtype, num_beams=20, **kw)
        drf = HipLlama.from_state_dict(ddims, dsd, dtype, num_beams=40, **kw)
        bat = BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=None)
        assert len(bat) == n_users and all(o["n_valid"] == 20 for o in bat)
        for u in (0, 7, 23, 47):
            one = BSSD(tgt, drf, inputs[u], 4, 4, prefix_allowed_tokens_fn=None)
            P = len(prompts[u])
            a = {tuple(x) for x in one["beam_sequence"][:, P:].cpu().tolist()}
            b = {tuple(x) for x in bat[u]["beam_sequence"][:, P:].cpu().tolist()}
            if dtype == torch.float32:
                assert torch.equal(one["beam_sequence"], bat[u]["beam_sequence"])
                assert (one["n_run"], one["accept_steps"]) == (bat[u]["n_run"], bat[u]["accept_steps"])
            else:
                assert len(a & b) >= 17, (u, len(a & b))
                np.testing.assert_allclose(np.sort(one["beam_scores"].cpu().numpy()), np.sort(bat[u]["beam_scores"].cpu().numpy()), atol=0.15, rtol=0)
        if dtype == torch.float32:
            for u in (3, 31):
                ref = R.BSSD(RefLlama(tdims, tsd), RefLlama(ddims, dsd), prompts[u], 4, 4, 20, 40, None)
                P = len(prompts[u])
                assert bat[u]["beam_sequence"][:, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()
                assert (bat[u]["n_run"], bat[u]["total_accept_steps"]) == (ref["n_run"], ref["total_accept_steps"])
                np.testing.assert_allclose(bat[u]["beam_scores"].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
        release_decoders(tgt, drf)


def test_api_errors():
    ci = build_case_inputs(CASES[0])
    tgt, drf = _models(ci, CASES[0])
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}
    with pytest.raises(TypeError):       # separator absent: the reference's fn returns None -> TypeError in HF
        BSSD(tgt, drf, {"input_ids": torch.tensor([[1, 5, 6, 7]]).cuda()}, 4, 4, prefix_allowed_tokens_fn=ci["fn"])
    tgt.generation_config.do_sample = True
    with pytest.raises(atspeed_amd._lib.AtSpeedError):        # mask-free search is greedy only
        BSSD(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=None)
    tgt.generation_config.temperature = 0.0
    with pytest.raises(atspeed_amd._lib.AtSpeedError):
        BSSD(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=ci["fn"])
    tgt.generation_config.temperature = 1.0
    tgt.generation_config.do_sample = False
    # the reference's post-top-k id filter (beamSD.py:80-86) is hard-coded for item tokens >= 32000: an automaton over ordinary tokens
    # loses every beam to it (the reference then dies on a shape mismatch); here the call says so, and the thresholds
    # can be set per automaton
    low = atspeed_amd.PositionSetConstraint({0: [5, 6, 7, 8, 9], 1: [10, 11, 12], 2: [2]}, synth.RESPONSE_SEP)
    tgt.generation_config.num_beams, keep = 3, tgt.generation_config.num_beams
    try:
        with pytest.raises(atspeed_amd._lib.AtSpeedError) as ei:
            target_generate(tgt, inputs, 2, prefix_allowed_tokens_fn=low)
        assert ei.value.status == atspeed_amd._lib.ERR_FILTERED
        low2 = atspeed_amd.PositionSetConstraint({0: [5, 6, 7, 8, 9], 1: [10, 11, 12], 2: [2]}, synth.RESPONSE_SEP, id_filter=(0, 2))
        o = target_generate(tgt, inputs, 2, prefix_allowed_tokens_fn=low2)
        assert o["n_valid"] == 3 and set(o["beam_sequence"][:, -2].cpu().tolist()) <= {5, 6, 7, 8, 9}
    finally:
        tgt.generation_config.num_beams = keep
    # position-set mask exhausted (5th generated token after EOS): HF raises ValueError on the empty list
    with pytest.raises((ValueError, KeyError)):
        target_generate(tgt, inputs, 6, prefix_allowed_tokens_fn=ci["fn"])


def test_capacity_limits_are_reported_not_faulted():
    """Sizes beyond the handles' limits must come back as status codes (AtSpeedError), never as a device fault."""
    from atspeed_amd._lib import AtSpeedError
    case = CASES[0]
    ci = build_case_inputs(case)
    kw = dict(max_slots=128, max_tokens=128, max_logit_rows=128)
    t = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=20, **kw)
    d = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=40, **kw)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}
    with pytest.raises(AtSpeedError) as e:           # 24 + 3*40 tokens need 144 KV slots > 128
        BSSD(t, d, inputs, 4, 4, prefix_allowed_tokens_fn=ci["fn"])
    assert e.value.status == -3
    t.generation_config.num_beams = 65               # > ATSPEED_MAX_BEAMS
    with pytest.raises(AtSpeedError):
        target_generate(t, inputs, 4, prefix_allowed_tokens_fn=ci["fn"])
    t.generation_config.num_beams = 20
    d.generation_config.num_beams = 10               # draft beams < target beams
    with pytest.raises(AtSpeedError):
        BSSD(t, d, inputs, 4, 4, prefix_allowed_tokens_fn=ci["fn"])
    d.generation_config.num_beams = 40
    with pytest.raises(AtSpeedError):                # gamma beyond ATSPEED_MAX_GAMMA
        BSSD(t, d, inputs, 9, 4, prefix_allowed_tokens_fn=ci["fn"])
    long_prompt = synth.synthetic_prompt(600, 1)
    with pytest.raises(AtSpeedError):                # prompt longer than the decoder was built for
        target_generate(t, {"input_ids": torch.from_numpy(long_prompt)[None].cuda()}, 4, prefix_allowed_tokens_fn=ci["fn"])
    # and the handles still work afterwards
    t2 = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=5, max_slots=256, max_tokens=256, max_logit_rows=128)
    out = target_generate(t2, inputs, 4, prefix_allowed_tokens_fn=ci["fn"])
    assert out["beam_sequence"].shape == (5, len(ci["prompt"]) + 4)


def test_max_beams_and_long_generation():
    """K = DK = 64 (ATSPEED_MAX_BEAMS) and 7 generated positions on the tiny models: lossless vs plain beam search."""
    case = [c for c in CASES if c["name"] == "k20_dk40_new7_gamma2"][0]
    ci = build_case_inputs(case)
    kw = dict(max_slots=1024, max_tokens=640, max_logit_rows=512)
    t = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=64, **kw)
    d = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=64, **kw)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}
    a = BSSD(t, d, inputs, 3, 7, prefix_allowed_tokens_fn=ci["fn"])
    b = target_generate(t, inputs, 7, prefix_allowed_tokens_fn=ci["fn"])
    assert a["beam_sequence"].shape == (64, len(ci["prompt"]) + 7)
    assert torch.equal(a["beam_sequence"], b["beam_sequence"])
    np.testing.assert_allclose(a["beam_scores"].cpu().numpy(), b["beam_scores"].cpu().numpy(), atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["k20_dk40_sigma01_s7", "k20_dk40_sigma0", "k5_dk10_indep", "k20_dk40_trie", "k6_dk12_new7_gamma3_s9"])
def test_arbitrary_python_mask_callable(name, bssd_golden):
    """A plain closure (no compile()) takes the host-mask path: same answers as the reference."""
    case = [c for c in CASES if c["name"] == name][0]
    gold = bssd_golden[name]
    ci = build_case_inputs(case)
    tgt, drf = _models(ci, case)
    con = ci["fn"]
    calls = []
    def closure(batch_id, sentence):                  # what BaseDataset.get_prefix_allowed_tokens_fn returns (data.py:96-104)
        calls.append(batch_id)
        return con(batch_id, sentence)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}
    P = len(ci["prompt"])
    tg = target_generate(tgt, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=closure)
    nv = len(gold["tg_tokens"])
    assert tg["beam_sequence"][:, P:].cpu().tolist() == gold["tg_tokens"]
    np.testing.assert_allclose(tg["beam_scores"].cpu().numpy(), gold["tg_scores"], atol=SCORE_TOL, rtol=0)
    out = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=closure)
    assert out["beam_sequence"][:, P:].cpu().tolist() == gold["bssd_tokens"]
    np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), gold["bssd_scores"], atol=SCORE_TOL, rtol=0)
    assert (out["n_run"], out["total_accept_steps"]) == (gold["n_run"], gold["total_accept_steps"])
    assert out["accept_steps"] == [r["n_matches"] for r in gold["rounds"]]
    assert calls and set(calls) == {0} and nv > 0
    # the CSV columns inference.py:183-187 reads: wall-clock stage times as the reference's Timer measures them, not zeros
    assert out["draft_time_cost"] > 0 and out["target_time_cost"] > 0 and out["verify_time_cost"] > 0
    assert out["draft_time_cost"] + out["target_time_cost"] + out["verify_time_cost"] <= out["time_cost"]


def test_python_mask_callable_errors():
    ci = build_case_inputs(CASES[0])
    tgt, drf = _models(ci, CASES[0])
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}
    with pytest.raises(ValueError):                   # HF: empty allowed list
        target_generate(tgt, inputs, 2, prefix_allowed_tokens_fn=lambda b, s: [])
    with pytest.raises(TypeError):                    # the reference's fn returns None when "Response:" is absent
        target_generate(tgt, inputs, 2, prefix_allowed_tokens_fn=lambda b, s: None)


def test_aligned_synthetic_pair_brackets_acceptance():
    """HipLlama.from_synthetic(align_to=..): with the layers' residual writes scaled to ~0 a narrow draft and a wide target
    share one bigram table, so every draft step is accepted (n_run=1, 3 steps: SURVEY.md 8c property iii); a large
    scale decouples them.  Both stay lossless against target_generate on the same target."""
    V = synth.TINY.vocab_size
    fn = atspeed_amd.PositionSetConstraint(synth.TINY.allowed_tokens(), synth.RESPONSE_SEP)
    ddims = synth.LlamaDims(V, 96, 2, 3, 256)
    tdims = synth.LlamaDims(V, 128, 3, 4, 352)
    kw = dict(dtype=torch.float32, max_slots=512, max_tokens=512, max_logit_rows=448)
    prompt = synth.synthetic_prompt(30, 77)
    inputs = {"input_ids": torch.from_numpy(prompt)[None].cuda()}
    seen = {}
    for rs in (1e-6, 1.0):
        d = HipLlama.from_synthetic(ddims, 5, num_beams=40, resid_scale=rs, **kw)
        t = HipLlama.from_synthetic(tdims, 6, num_beams=20, resid_scale=rs, align_to=d, **kw)
        out = BSSD(t, d, inputs, 4, 4, prefix_allowed_tokens_fn=fn)
        tg = target_generate(t, inputs, 4, prefix_allowed_tokens_fn=fn)
        assert torch.equal(out["beam_sequence"], tg["beam_sequence"])
        np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), tg["beam_scores"].cpu().numpy(), atol=SCORE_TOL, rtol=0)
        seen[rs] = (out["n_run"], out["total_accept_steps"])
    assert seen[1e-6] == (1, 3)
    assert seen[1.0][1] < 3 and seen[1.0][0] > 1


def test_harness_end_to_end_on_a_tiny_dataset():
    """dataset -> prompts -> BSSD (lock-step batches) -> items -> ranking metrics (atspeed_amd.harness):
    under the strict trie every returned beam is an item, beam-SD returns target_generate's ranking, and the aligned
    weight pair accepts every draft step."""
    from atspeed_amd.harness import ItemIndex, SeqRecTestData, run_inference
    rng = np.random.default_rng(3)
    # >= DK distinct first-level codes: fewer finite candidates than beams is the regime where the reference itself breaks
    idx = {str(i): [f"<a_{rng.integers(48)}>", f"<b_{rng.integers(8)}>", f"<c_{rng.integers(8)}>", f"<d_{rng.integers(8)}>"] for i in range(300)}
    ix = ItemIndex(idx)
    assert len(ix.allowed_tokens()[0]) >= 20
    train = {u: rng.integers(0, 300, size=rng.integers(1, 12)).tolist() for u in range(12)}
    valid = {u: rng.integers(0, 300, size=1).tolist() for u in range(12)}
    test = {u: (rng.integers(0, 300, size=1).tolist() if u % 4 else []) for u in range(12)}
    data = SeqRecTestData(ix, train, valid, test)
    assert len(data) == 9
    V = ix.vocab_size
    kw = dict(dtype=torch.float32, max_slots=512, max_tokens=512, max_logit_rows=448)
    d = HipLlama.from_synthetic(synth.LlamaDims(V, 96, 2, 3, 256), 5, num_beams=20, resid_scale=1e-6, **kw)
    t = HipLlama.from_synthetic(synth.LlamaDims(V, 128, 3, 4, 352), 6, num_beams=10, resid_scale=1e-6, align_to=d, **kw)
    strict = data.strict_trie_fn()
    res = run_inference(t, d, data, gamma=4, max_new_tokens=4, users_per_batch=4, prefix_allowed_tokens_fn=strict, baseline=True)
    assert len(res.predictions) == 9 and all(len(p) == 10 for p in res.predictions)
    assert all(i >= 0 for p in res.predictions for i in p)               # strict trie: every beam names an item
    assert all(len(set(p)) == len(p) for p in res.predictions)           # distinct beams -> distinct items
    assert res.counters()["mean_accept_len"] == 3.0
    assert all(set(r) >= {"speedup", "generalBS_time_cost", "overhead"} for r in res.rows)
    from atspeed_amd.harness import CodeTokenEncoder, encode_prompt
    enc = CodeTokenEncoder(ix)
    for u, pred in zip(data.users, res.predictions):
        ids = torch.from_numpy(encode_prompt(data, u, None, enc))[None].cuda()
        tg = target_generate(t, {"input_ids": ids}, 4, prefix_allowed_tokens_fn=strict)
        assert [ix.decode(g) for g in tg["beam_sequence"][:, ids.shape[1]:].cpu().tolist()] == pred
    m = res.metrics(ix, topN=(1, 5, 10, 20))
    assert m["topN"] == [1, 5, 10] and all(0.0 <= x <= 1.0 for key in ("precision", "recall", "ndcg", "mrr") for x in m[key])
    # decoder="beam": the plain lock-step beam search of the target returns the same items (the method is lossless)
    res_b = run_inference(t, d, data, gamma=4, max_new_tokens=4, users_per_batch=4, prefix_allowed_tokens_fn=strict, decoder="beam")
    assert res_b.predictions == res.predictions and all(r["n_run"] == 0 for r in res_b.rows)
    # the position-set mask (what inference.py really uses) may compose code tuples that are no item
    res2 = run_inference(t, d, data, users_per_batch=9)
    assert len(res2.predictions) == 9 and any(i == -1 for p in res2.predictions for i in p)


def test_inference_cli_on_generated_dataset(tmp_path):
    """`python -m atspeed_amd.inference` end to end: dataset files in the reference's formats (index JSON + sequential_*.txt),
    2-layer Llama-7B-dims target / Llama-68M-dims draft with aligned synthetic weights, summary JSON with timing and metrics."""
    import json
    from atspeed_amd import inference
    rng = np.random.default_rng(5)
    root = tmp_path / "data" / "toys"
    root.mkdir(parents=True)
    idx = {str(i): [f"<a_{rng.integers(64)}>", f"<b_{rng.integers(16)}>", f"<c_{rng.integers(16)}>", f"<d_{rng.integers(16)}>"] for i in range(500)}
    (root / "toys.LCRec-1e-3lr.json").write_text(json.dumps(idx))
    for name, n_lo, n_hi in (("train", 2, 25), ("valid", 1, 2), ("test", 0, 2)):
        lines = []
        for u in range(1, 21):
            items = rng.integers(1, 501, size=rng.integers(n_lo, n_hi)).tolist()
            lines.append(" ".join(str(x) for x in [u] + items))
        (root / f"sequential_{name}.txt").write_text("\n".join(lines) + "\n")
    out = inference.main(["--data_path", str(tmp_path / "data"), "--dataset", "toys", "--target_layers", "2", "--aligned", "3e-6",
                          "--run_beam_sizes", "[5, 20]", "--users_per_batch", "8", "--strict_trie", "--baseline",
                          "--output_dir", str(tmp_path / "AnaResult")])
    assert [r["beam_size"] for r in out] == [5, 20]
    for r in out:
        assert r["users"] > 0 and r["items_per_s"] > 0 and r["mean_accept_len"] == 3.0
        assert r["metrics"]["users"] == r["users"] and len(r["metrics"]["recall"]) == len(r["metrics"]["topN"])
        assert {"draft_time_cost", "target_time_cost", "verify_time_cost", "total_time_cost", "speedup"} <= set(r["timing_mean_rank0"])
    assert len(list((tmp_path / "AnaResult" / "toys").glob("timing_mean_*.json"))) == 2
    # --dtype: the engine's fp16 flavour -- the reference's own type, inference.py:75-100 -- is reachable from the CLI; same decoder, same columns
    out16 = inference.main(["--data_path", str(tmp_path / "data"), "--dataset", "toys", "--target_layers", "2", "--aligned", "3e-6", "--dtype", "fp16",
                            "--run_beam_sizes", "[5]", "--users_per_batch", "8", "--strict_trie", "--output_dir", str(tmp_path / "AnaResult16")])
    assert out16[0]["users"] == out[0]["users"] and out16[0]["mean_accept_len"] == 3.0
    # config 5 in the reference's own loop: --target_fp8 with ONE user per call (inference.py:86-91,162-176) through the W8A8 weight-streaming kernels
    out8 = inference.main(["--data_path", str(tmp_path / "data"), "--dataset", "toys", "--target_layers", "2", "--aligned", "3e-6", "--target_fp8",
                           "--run_beam_sizes", "[20]", "--users_per_batch", "1", "--strict_trie", "--output_dir", str(tmp_path / "AnaResult8u1")])
    assert out8[0]["users"] == out[1]["users"] and out8[0]["mean_accept_len"] >= 2.5 and out8[0]["items_per_s"] > 0
    # the reference's own dtype combination (inference.py:75-91: fp16 checkpoints, 8-bit target): the fp16 flavour with W8A8 target projections
    out816 = inference.main(["--data_path", str(tmp_path / "data"), "--dataset", "toys", "--target_layers", "2", "--aligned", "3e-6", "--dtype", "fp16",
                             "--target_fp8", "--run_beam_sizes", "[20]", "--users_per_batch", "1", "--strict_trie", "--output_dir", str(tmp_path / "AnaResult8f16")])
    assert out816[0]["users"] == out[1]["users"] and out816[0]["mean_accept_len"] >= 2.5 and out816[0]["items_per_s"] > 0
    with pytest.raises(SystemExit):                                                  # the e4m3 copies are made of 16-bit weights: refused before anything is loaded
        inference.main(["--data_path", str(tmp_path / "data"), "--dataset", "toys", "--target_layers", "2", "--dtype", "fp32", "--target_fp8",
                        "--run_beam_sizes", "[5]", "--output_dir", str(tmp_path / "AnaResult8")])


def test_target_generate_batch_equals_single_calls(bssd_golden):
    from atspeed_amd.beamSD import target_generate_batch
    case = next(c for c in CASES if c["name"] == "k20_dk40_trie")
    ci = build_case_inputs(case)
    tgt, _ = _models(ci, case)
    rng = np.random.default_rng(2)
    prompts = [ci["prompt"]] + [np.concatenate([rng.integers(3, 31000, size=n), ci["prompt"][-6:]]) for n in (5, 40, 17)]
    inputs = [{"input_ids": torch.from_numpy(p.astype(np.int64))[None].cuda()} for p in prompts]
    outs = target_generate_batch(tgt, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    for inp, o in zip(inputs, outs):
        one = target_generate(tgt, inp, case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
        assert torch.equal(o["beam_sequence"], one["beam_sequence"])
        np.testing.assert_allclose(o["beam_scores"].cpu().numpy(), one["beam_scores"].cpu().numpy(), atol=SCORE_TOL, rtol=0)
    gold = bssd_golden[case["name"]]
    P = len(ci["prompt"])
    assert outs[0]["beam_sequence"][:, P:].cpu().tolist() == gold["tg_tokens"]   # the real reference's output


def test_teacher_data_tensors_match_the_oracle_forward():
    """generate_teacher_data: beams from the lock-step constrained search; the packed tree-mask forward
    returns, for the label and for every beam, the logits a plain causal forward over prompt ++ sequence gives (oracle Llama)."""
    from atspeed_amd.harness import CodeTokenEncoder, ItemIndex, SeqRecTestData, encode_prompt
    from atspeed_amd.teacher import generate_teacher_data
    rng = np.random.default_rng(4)
    idx = {str(i): [f"<a_{rng.integers(40)}>", f"<b_{rng.integers(8)}>", f"<c_{rng.integers(8)}>", f"<d_{rng.integers(8)}>"] for i in range(200)}
    ix = ItemIndex(idx)
    train = {u: rng.integers(0, 200, size=rng.integers(2, 9)).tolist() for u in range(3)}
    data = SeqRecTestData(ix, train, {u: [] for u in range(3)}, {u: [int(rng.integers(200))] for u in range(3)})
    dims = synth.LlamaDims(ix.vocab_size, 128, 2, 4, 352)
    sd = synth.synthetic_state_dict(dims, 11, std=0.05, head_std=0.1)
    m = HipLlama.from_state_dict(dims, sd, torch.float32, max_slots=512, max_tokens=512, max_logit_rows=512, num_beams=10)
    ref = RefLlama(dims, sd, max_slots=512)
    enc = CodeTokenEncoder(ix)
    prompts = [encode_prompt(data, u, None, enc) for u in data.users]
    labels = [list(ix.item_codes[u.labels[0]]) + [2] for u in data.users]
    out = generate_teacher_data(m, prompts, labels, data.strict_trie_fn(), beam_size=10, max_new_token=5, users_per_batch=2)
    for p, lab, tl, to, tol in zip(prompts, labels, out["teacher_logits"], out["teacher_output"], out["teacher_output_logits"]):
        assert to.shape == (10, 5) and tl.shape == (5, ix.vocab_size) and tol.shape == (10, 5, ix.vocab_size - 32000)
        assert all(ix.decode(b[:4]) >= 0 and b[4] == 2 for b in to.tolist())              # strict trie: item codes, then EOS
        for seq, got in [(lab, tl)] + [(b, torch.cat([torch.zeros(5, 32000), g], 1)) for b, g in zip(to.tolist()[:3], tol[:3])]:
            full = torch.from_numpy(np.concatenate([p, np.asarray(seq[:-1], dtype=np.int64)]))
            inp = R._causal_inputs(full)
            want = ref.forward(inp.ids, inp.pos, inp.slots, inp.vis)[len(p) - 1:]
            cols = slice(32000, None) if got is not tl else slice(None)
            np.testing.assert_allclose(got[:, cols].numpy(), want[:, cols].numpy(), atol=LOGIT_TOL, rtol=0)
    # samples scored one per forward give what the batched forward (one segment and KV arena per sample) gave
    one = generate_teacher_data(m, prompts, labels, data.strict_trie_fn(), beam_size=10, max_new_token=5, users_per_batch=3, score_batch=1)
    for k in ("teacher_logits", "teacher_output_logits"):
        for a, b in zip(out[k], one[k]):
            np.testing.assert_allclose(a.numpy(), b.numpy(), atol=LOGIT_TOL, rtol=0)
    assert all(torch.equal(a, b) for a, b in zip(out["teacher_output"], one["teacher_output"]))


# ------------------------------------------------------------------ sampling branch
def _sampling_pair(name, temperature):
    case = next(c for c in CASES if c["name"] == name)
    ci = build_case_inputs(case)
    tgt, drf = _models(ci, case)
    for m in (tgt, drf):
        m.generation_config.do_sample = True
        m.generation_config.temperature = temperature
    return case, ci, tgt, drf, RefLlama(ci["target_dims"], ci["target_sd"]), RefLlama(ci["draft_dims"], ci["draft_sd"])


@pytest.mark.parametrize("name,temperature", [("k10_dk40_sigma01", 1.3), ("k20_dk40_sigma01_s7", 1.0), ("k5_dk10_indep", 1.0),
                                              ("k20_dk40_sigma0", 0.7), ("k20_dk40_trie", 1.0)])
def test_sampling_bssd_makes_the_oracles_decisions(name, temperature):
    """do_sample: the device draws from the same counter-based streams as oracle/beamsd_sample_ref.py (HashRng), whose torch-RNG
    twin is pinned seed for seed to the real reference.  Same sampled beams and per-round n_matches for every seed whose
    closest decision margin is above fp32 noise; scores within 1e-3."""
    from oracle import beamsd_sample_ref as S
    case, ci, tgt, drf, rt, rd = _sampling_pair(name, temperature)
    P = len(ci["prompt"])
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}
    checked = 0
    acc = []
    for seed in range(40, 52):
        rng = S.HashRng(seed)
        ref = S.BSSD_sample(rt, rd, ci["prompt"], case["gamma"], case["max_new_tokens"], case["K"], case["DK"], ci["fn"], temperature, rng)
        out = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        acc.append(out["total_accept_steps"])
        nv = out["n_valid"]                          # fewer finite candidates than beams (strict trie): dead slots sort last
        same = nv == ref["beam_sequence"].shape[0] and out["beam_sequence"][:nv, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()
        if rng.min_margin < 1e-4 and not same:
            continue                                   # a draw decided by less than fp32 rounding: not comparable
        checked += 1
        assert same, (name, seed, rng.min_margin)
        assert out["accept_steps"] == [r["n_matches"] for r in ref["rounds"]] and out["n_run"] == ref["n_run"]
        np.testing.assert_allclose(out["beam_scores"][:nv].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
        assert (np.diff(out["beam_scores"][:nv].cpu().numpy()) <= 0).all()     # beamSD.py:529-531: sorted best first
    assert checked >= 10
    # same seed twice -> same result; another seed -> (almost surely) another
    a = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=7)
    b = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=7)
    assert torch.equal(a["beam_sequence"], b["beam_sequence"])


def test_sampled_walk_that_accepts_every_block_feeds_the_draft_its_last_block():
    """do_sample with draft == target at K 6, DK 12, gamma 2, 7 new tokens: for each of these seeds a round before the last accepts both draft
    blocks, so the sampled walk writes the draft's re-ingest inputs (its own last block ++ the new beams, beamSD.py:402-416) and the next
    round's draft steps run on them.  Same beams, rounds and accepted steps as oracle/beamsd_sample_ref.py, under the rule of the test above."""
    from oracle import beamsd_sample_ref as S
    temperature = 1.0
    case = dict(next(c for c in CASES if c["name"] == "k6_dk12_new7_gamma2_s5"), sigma=0.0)
    ci = build_case_inputs(case)
    tgt, drf = _models(ci, case)
    for m in (tgt, drf):
        m.generation_config.do_sample = True
        m.generation_config.temperature = temperature
    rt, rd = RefLlama(ci["target_dims"], ci["target_sd"]), RefLlama(ci["draft_dims"], ci["draft_sd"])
    P = len(ci["prompt"])
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}
    checked = 0
    for seed in range(40, 44):
        rng = S.HashRng(seed)
        ref = S.BSSD_sample(rt, rd, ci["prompt"], case["gamma"], case["max_new_tokens"], case["K"], case["DK"], ci["fn"], temperature, rng)
        out = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        nv = out["n_valid"]
        same = nv == ref["beam_sequence"].shape[0] and out["beam_sequence"][:nv, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()
        if rng.min_margin < 1e-4 and not same:
            continue                                   # a draw decided by less than fp32 rounding: not comparable
        checked += 1
        assert same, (seed, rng.min_margin)
        assert out["accept_steps"] == [r["n_matches"] for r in ref["rounds"]] and out["n_run"] == ref["n_run"]
        assert case["gamma"] in out["accept_steps"][:-1]                          # a walk that accepted every block, and a round after it
        np.testing.assert_allclose(out["beam_scores"][:nv].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
    assert checked >= 3


@pytest.mark.parametrize("name,temperature", [("k10_dk40_sigma01", 1.3), ("k20_dk40_sigma0", 0.7), ("k5_dk10_indep", 1.0)])
def test_sampling_with_a_host_side_mask_or_processor_samples_what_the_device_path_samples(name, temperature):
    """do_sample with an arbitrary Python mask callable or extra logits processors (legal in the reference: beamSD.py:293-369 with any
    `logits_processor`; NotImplementedError through round 3): the host path draws from the device's counter-based streams, so a closure that
    wraps the compilable constraint -- and the same with an identity processor appended -- returns exactly the device path's sampled beams,
    rounds and accepted steps for the same seed (scores within 1e-3)."""
    case, ci, tgt, drf, rt, rd = _sampling_pair(name, temperature)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}
    closure = lambda b, sent: ci["fn"](b, sent)                   # no .compile(): served by hostmask.py
    same_b = same_p = same_t = 0
    seeds = list(range(60, 70))
    for seed in seeds:
        dev = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        host = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=closure, seed=seed)
        proc = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], logits_processor=[lambda ids, sc: sc + 0.0],
                    prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        nv = dev["n_valid"]
        for other, tag in ((host, "b"), (proc, "p")):
            ok = (other["beam_sequence"].shape[0] == nv and torch.equal(other["beam_sequence"], dev["beam_sequence"][:nv])
                  and other["accept_steps"] == dev["accept_steps"] and other["n_run"] == dev["n_run"])
            if ok:
                np.testing.assert_allclose(other["beam_scores"].cpu().numpy(), dev["beam_scores"][:nv].cpu().numpy(), atol=SCORE_TOL, rtol=0)
                assert (np.diff(other["beam_scores"].cpu().numpy()) <= 0).all()
            if tag == "b":
                same_b += ok
            else:
                same_p += ok
        d_t = target_generate(tgt, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        h_t = target_generate(tgt, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=closure, seed=seed)
        same_t += bool(h_t["beam_sequence"].shape[0] == d_t["n_valid"] and torch.equal(h_t["beam_sequence"], d_t["beam_sequence"][: d_t["n_valid"]]))
    print(f"[{name}] host-mask sampling equals the device path on {same_b} / {same_p} / {same_t} of {len(seeds)} seeds (closure / processor / target_generate)")
    # a draw decided by less than fp32 rounding may differ between the host's and the device's softmax: at most one seed in ten
    assert same_b >= len(seeds) - 1 and same_p >= len(seeds) - 1 and same_t >= len(seeds) - 1
    # repeatable
    a = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=closure, seed=7)
    b = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=closure, seed=7)
    assert torch.equal(a["beam_sequence"], b["beam_sequence"])
    for m in (tgt, drf):
        m.generation_config.do_sample = False


def test_sampling_target_generate_and_batches():
    from atspeed_amd.beamSD import BSSD_batch, target_generate_batch
    from oracle import beamsd_sample_ref as S
    name, temperature = "k10_dk40_sigma01", 1.3
    case, ci, tgt, drf, rt, rd = _sampling_pair(name, temperature)
    P = len(ci["prompt"])
    rng0 = np.random.default_rng(1)
    prompts = [ci["prompt"]] + [np.concatenate([rng0.integers(3, 31000, size=n), ci["prompt"][-6:]]) for n in (9, 30)]
    inputs = [{"input_ids": torch.from_numpy(p.astype(np.int64))[None].cuda()} for p in prompts]
    # plain sampled beam search (beamSD.py:544-595 with do_sample)
    for seed in (3, 4, 5):
        rng = S.HashRng(seed)
        ref = S.target_generate_sample(rt, prompts[0], case["max_new_tokens"], case["K"], ci["fn"], temperature, rng)
        out = target_generate(tgt, inputs[0], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        if rng.min_margin >= 1e-4:
            assert out["beam_sequence"][:, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()
    # batches: user u draws from stream seed + u, i.e. equals the single call with that seed
    outs = BSSD_batch(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=100)
    tgs = target_generate_batch(tgt, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=200)
    for u, (inp, o, t) in enumerate(zip(inputs, outs, tgs)):
        one = BSSD(tgt, drf, inp, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=100 + u)
        assert torch.equal(o["beam_sequence"], one["beam_sequence"]) and o["accept_steps"] == one["accept_steps"]
        one_t = target_generate(tgt, inp, case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"], seed=200 + u)
        assert torch.equal(t["beam_sequence"], one_t["beam_sequence"])
    # greedy again on the same decoders once do_sample is off
    for m in (tgt, drf):
        m.generation_config.do_sample = False
    g = BSSD(tgt, drf, inputs[0], case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    tg = target_generate(tgt, inputs[0], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    assert torch.equal(g["beam_sequence"], tg["beam_sequence"])


def test_release_decoders_frees_and_recreates():
    from atspeed_amd.beamSD import _Decoder, release_decoders
    case = CASES[0]
    ci = build_case_inputs(case)
    tgt, drf = _models(ci, case)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}
    a = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    n_before = len(_Decoder._cache)
    assert release_decoders(tgt, drf) >= 1 and len(_Decoder._cache) < n_before
    b = BSSD(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    assert torch.equal(a["beam_sequence"], b["beam_sequence"])
