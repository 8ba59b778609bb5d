"""Prompt prefixes (include/atspeed_hip.h "prompt prefixes") on the GPU: the copy kernel alone with guard bands, the fp32
engine behind a prefix against the reference's golden vectors, batches and sessions whose users name different prefixes or none, the
refusals, the 16-bit / W8A8 / per-user-adapter forwards behind a scattered prefix, sampling, and the harness."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib, synth
from atspeed_amd import lora as L
from atspeed_amd.beamSD import (BSSD, BSSD_batch, BSSDSession, _Decoder, last_trace, release_decoders, target_generate,
                                target_generate_batch)
from atspeed_amd.model import HipLlama, PromptPrefix, vis_bits_from_bool
from oracle.llama_ref import RefLlama
from tests.golden.cases import CASES, build_case_inputs

SCORE_TOL = 1e-3
DEV = "cuda:0"
KW = dict(max_slots=512, max_tokens=512, max_logit_rows=448)


# ------------------------------------------------------------------ 1. the copy kernel alone
SENTINEL = 0xA5
HALO = 4096


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _copy_case(lp, row_bytes, layers, users, max_slots=128):
    """scatter, then gather, at one shape: every byte of every buffer is compared with what the contract says it holds"""
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(lp * 1000 + row_bytes + layers + users)
    arena = layers * max_slots * row_bytes
    store_bytes = layers * lp * row_bytes
    rnd = lambda n: torch.randint(0, 256, (n,), dtype=torch.uint8, device=DEV, generator=g)
    stores = [torch.cat((torch.full((HALO,), SENTINEL, dtype=torch.uint8, device=DEV), rnd(store_bytes),
                         torch.full((HALO,), SENTINEL, dtype=torch.uint8, device=DEV))) for _ in range(2)]
    # every user's K and V arena inside ONE sentinel-filled buffer: halo | arena | halo per (user, K / V)
    stride = HALO + arena + HALO
    buf = torch.full((users * 2, stride), SENTINEL, dtype=torch.uint8, device=DEV)
    ka = [buf[2 * u, HALO:HALO + arena] for u in range(users)]
    va = [buf[2 * u + 1, HALO:HALO + arena] for u in range(users)]
    st = _lib.stream_ptr(torch.device(DEV))
    _lib.check(lib.atspeed_kv_rows_scatter(stores[0][HALO:].data_ptr(), stores[1][HALO:].data_ptr(), _ptrs(ka), _ptrs(va), users, lp, layers,
                                           row_bytes, max_slots, st))
    want = torch.full_like(buf, SENTINEL)
    for kv in range(2):
        rows = stores[kv][HALO:HALO + store_bytes].view(layers, lp * row_bytes)
        w = want[kv::2, HALO:HALO + arena].view(users, layers, max_slots * row_bytes)        # rows >= lp, the next layer, the halos keep the sentinel
        w[:, :, :lp * row_bytes] = rows[None]
    assert torch.equal(buf, want), f"scatter lp={lp} row_bytes={row_bytes} layers={layers} users={users}"
    # gather: a random arena pair -> a sentinel-filled store
    src = [rnd(arena), rnd(arena)]
    keep = [s.clone() for s in src]
    out = [torch.full((HALO + store_bytes + HALO,), SENTINEL, dtype=torch.uint8, device=DEV) for _ in range(2)]
    _lib.check(lib.atspeed_kv_rows_gather(out[0][HALO:].data_ptr(), out[1][HALO:].data_ptr(), src[0].data_ptr(), src[1].data_ptr(), lp, layers,
                                          row_bytes, max_slots, st))
    for kv in range(2):
        assert torch.equal(src[kv], keep[kv])
        assert bool((out[kv][:HALO] == SENTINEL).all()) and bool((out[kv][HALO + store_bytes:] == SENTINEL).all())
        got = out[kv][HALO:HALO + store_bytes].view(layers, lp * row_bytes)
        assert torch.equal(got, src[kv].view(layers, max_slots * row_bytes)[:, :lp * row_bytes]), f"gather lp={lp} row_bytes={row_bytes}"


@pytest.mark.parametrize("hidden,esz", [(64, 4), (768, 2), (4096, 2)], ids=["h64_fp32", "h768_16bit", "h4096_16bit"])
def test_copy_kernel_guard_bands(hidden, esz):
    """fp32 / bf16 / fp16 differ for this kernel in the row's bytes alone (it moves 16-byte pieces): hidden 64 fp32 = 256-byte rows, 768 and
    4096 in a 16-bit type = 1536- and 8192-byte rows"""
    for lp in (1, 7, 36, 64):
        for layers in (1, 3):
            for users in (1, 5):
                _copy_case(lp, hidden * esz, layers, users)


def test_copy_kernel_guard_bands_256_users():
    for lp in (1, 36):
        _copy_case(lp, 768 * 2, 1, 256)


def test_copy_kernel_refuses_bad_shapes():
    lib = _lib.load()
    t = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = _ptrs([t])
    assert lib.atspeed_kv_rows_scatter(t.data_ptr(), t.data_ptr(), p, p, 1, 129, 1, 64, 128, None) == _lib.ERR_INVALID       # more rows than slots
    assert lib.atspeed_kv_rows_scatter(t.data_ptr(), t.data_ptr(), p, p, 1, 0, 1, 64, 128, None) == _lib.ERR_INVALID
    assert lib.atspeed_kv_rows_scatter(t.data_ptr(), t.data_ptr(), p, p, 1, 4, 1, 24, 128, None) == _lib.ERR_INVALID         # rows of 24 bytes
    assert lib.atspeed_kv_rows_scatter(t.data_ptr(), t.data_ptr(), p, p, 257, 4, 1, 64, 128, None) == _lib.ERR_CAPACITY


# ------------------------------------------------------------------ 2. fp32 engine against the golden vectors
def _case(name):
    return [c for c in CASES if c["name"] == name][0]


@functools.lru_cache(maxsize=2)
def _world(name, dtype=torch.float32):
    case = _case(name)
    ci = build_case_inputs(case)
    t = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], dtype, num_beams=case["K"], **KW)
    d = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], dtype, num_beams=case["DK"], **KW)
    return case, ci, t, d


def _inp(prompt):
    return {"input_ids": torch.from_numpy(np.asarray(prompt, dtype=np.int64))[None].to(DEV)}


def _decoder_kv(tgt, drf, draft):
    """the K and V arena of lane 0's decoder as [layers, max_slots, hidden] tensors of the model's type (atspeed_decoder_kv_copy)"""
    lib = _lib.load()
    dec = _Decoder.cached(tgt, drf)
    m = drf if draft else tgt
    n = int(lib.atspeed_decoder_kv_bytes(dec.handle, 1 if draft else 0))
    k, v = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    _lib.check(lib.atspeed_decoder_kv_copy(dec.handle, 1 if draft else 0, 0, k.data_ptr(), v.data_ptr(), _lib.stream_ptr(torch.device(DEV))))
    shape = (m.dims.n_layers, m.max_slots, m.dims.hidden)
    return k.view(m.dtype).view(shape), v.view(m.dtype).view(shape)


GOLDEN_CASES = ["k20_dk40_sigma01", "k20_dk40_trie", "k6_dk12_new7_gamma2_s5", "k20_dk40_sigma0", "k5_dk10_indep"]


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_fp32_engine_behind_a_prefix_equals_the_golden_vectors(name, bssd_golden):
    case, ci, tgt, drf = _world(name)
    gold = bssd_golden[name]
    prompt, P, fn = ci["prompt"], len(ci["prompt"]), ci["fn"]
    a = (case["gamma"], case["max_new_tokens"])
    dl = min(case["gamma"], case["max_new_tokens"] - 1)
    plain = BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn)
    plain_trace = last_trace(tgt, drf)
    for lp in (1, 8, P - 1):
        pre = PromptPrefix(tgt, drf, prompt[:lp])
        assert pre.length == lp and pre.ids == tuple(int(t) for t in prompt[:lp]) and not pre.stale
        assert pre.info()["bytes"] == 2 * tgt.dims.n_layers * lp * tgt.dims.hidden * 4 + 4 * lp
        assert pre.read()[2].tolist() == [int(t) for t in prompt[:lp]] and pre.read(True)[2].tolist() == [int(t) for t in prompt[:lp]]
        # ---- BSSD
        tgt.forward_log(1), drf.forward_log(1)
        out = BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, prefix=pre)
        tlog, dlog = tgt.forward_log(0), drf.forward_log(0)
        assert dlog[0][0] == P - lp, (lp, dlog[:2])                       # the draft's first forward: the suffix rows alone
        assert tlog[0][0] == P - lp + dl * case["DK"], (lp, tlog[:2])      # the target's first (packed) forward: suffix rows + the draft blocks
        assert out["beam_sequence"].shape == (case["K"], P + case["max_new_tokens"])
        assert (out["beam_sequence"][:, :P].cpu() == torch.from_numpy(prompt)[None]).all()
        assert out["beam_sequence"][:, P:].cpu().tolist() == gold["tg_tokens"]
        np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), gold["tg_scores"], atol=SCORE_TOL, rtol=0)
        assert torch.equal(out["beam_sequence"], plain["beam_sequence"])
        assert (out["n_run"], out["total_accept_steps"], out["accept_steps"]) == (plain["n_run"], plain["total_accept_steps"], plain["accept_steps"])
        tr = last_trace(tgt, drf)
        assert tr == plain_trace
        if "reference_error" not in gold:
            assert out["beam_sequence"][:, P:].cpu().tolist() == gold["bssd_tokens"]
            np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), gold["bssd_scores"], atol=SCORE_TOL, rtol=0)
            assert out["n_run"] == gold["n_run"] and out["total_accept_steps"] == gold["total_accept_steps"]
            assert [r["n_matches"] for r in tr] == [r["n_matches"] for r in gold["rounds"]]
            for r, g in zip(tr, gold["rounds"]):
                for ids, gids in zip(r["draft_ids"], g["draft_ids"]):
                    assert [x for x in ids if x >= 0] == gids
        # slots [0, lp) of both arenas hold the prefix store bit for bit
        for draft in (False, True):
            pk, pv, _ = pre.read(draft)
            ak, av = _decoder_kv(tgt, drf, draft)
            assert torch.equal(ak[:, :lp].contiguous().view(torch.uint8), pk.view(torch.uint8)), (lp, draft)
            assert torch.equal(av[:, :lp].contiguous().view(torch.uint8), pv.view(torch.uint8)), (lp, draft)
        assert pre.info()["users_served"] == 1 and pre.info(True)["users_served"] == 1
        # ---- target_generate: the target's half alone counts
        tgt.forward_log(1)
        tg = target_generate(tgt, _inp(prompt), case["max_new_tokens"], prefix_allowed_tokens_fn=fn, prefix=pre)
        tlog = tgt.forward_log(0)
        assert tlog[0][0] == P - lp and len(tlog) == case["max_new_tokens"]
        assert tg["beam_sequence"][:, P:].cpu().tolist() == gold["tg_tokens"]
        np.testing.assert_allclose(tg["beam_scores"].cpu().numpy(), gold["tg_scores"], atol=SCORE_TOL, rtol=0)
        assert pre.info()["users_served"] == 2 and pre.info(True)["users_served"] == 1
    # a later call without a prefix prefills the whole prompt again: the cached decoder does not keep the prefix
    tgt.forward_log(1)
    again = target_generate(tgt, _inp(prompt), case["max_new_tokens"], prefix_allowed_tokens_fn=fn)
    assert tgt.forward_log(0)[0][0] == P and again["beam_sequence"][:, P:].cpu().tolist() == gold["tg_tokens"]
    release_decoders(tgt, drf)


# ------------------------------------------------------------------ 3. batch and session: two prefixes and users without one
def _six_users():
    head_a = synth.synthetic_prompt(12, 4001)[:8]
    head_b = synth.synthetic_prompt(12, 4002)[:8]
    tails = [synth.synthetic_prompt(14 + 5 * u, 4100 + u)[1:] for u in range(6)]       # without their BOS; they end with the Response separator
    heads = [head_a, head_b, head_a, None, head_b, None]
    prompts = [np.concatenate((h, t)) if h is not None else np.concatenate(([1], t)) for h, t in zip(heads, tails)]
    return head_a, head_b, heads, prompts


def _same(what, single, outs, bssd=True, atol=SCORE_TOL):
    for u, (s, o) in enumerate(zip(single, outs)):
        assert torch.equal(s["beam_sequence"], o["beam_sequence"]), (what, u)
        np.testing.assert_allclose(s["beam_scores"].cpu().numpy(), o["beam_scores"].cpu().numpy(), atol=atol, rtol=0)
        if bssd:
            assert (s["n_run"], s["total_accept_steps"], s["accept_steps"]) == (o["n_run"], o["total_accept_steps"], o["accept_steps"]), (what, u)


def test_batch_and_session_with_two_prefixes_and_users_without_one():
    case, ci, tgt, drf = _world("k20_dk40_sigma01")
    fn, a = ci["fn"], (case["gamma"], case["max_new_tokens"])
    head_a, head_b, heads, prompts = _six_users()
    inputs = [_inp(p) for p in prompts]
    single = [BSSD(tgt, drf, inp, *a, prefix_allowed_tokens_fn=fn) for inp in inputs]
    single_tg = [target_generate(tgt, inp, a[1], prefix_allowed_tokens_fn=fn) for inp in inputs]
    pa, pb = PromptPrefix(tgt, drf, head_a), PromptPrefix(tgt, drf, head_b)
    prefixes = [None if h is None else (pa if h is head_a else pb) for h in heads]
    # lock step
    tgt.forward_log(1)
    bat = BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=fn, prefixes=prefixes)
    first = tgt.forward_log(0)[0][0]
    dl = min(case["gamma"], case["max_new_tokens"] - 1)
    assert first == sum(len(p) - (8 if h is not None else 0) for p, h in zip(prompts, heads)) + 6 * dl * case["DK"]
    _same("BSSD_batch(prefixes=)", single, bat)
    assert all(o["status"] == 0 for o in bat)
    assert (pa.users_served, pb.users_served, pa.info(True)["users_served"]) == (2, 2, 2)
    # two lanes
    ses = BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=fn, prefixes=prefixes, lanes=2)
    _same("BSSD_batch(lanes=2)", single, ses)
    c = ses[0]["session_counters"]
    assert c["allocs_after_create"] == 0 and c["users_retired"] == 6, c
    assert (pa.users_served, pb.users_served) == (4, 4)
    # a session with interleaved submits: three users, a round, the other three while the first are decoding
    with BSSDSession(tgt, drf, 2, *a, prefix_allowed_tokens_fn=fn) as s:
        tickets = [s.submit(inputs[u], prefix=prefixes[u]) for u in range(3)]
        done = s.step()
        tickets += [s.submit(inputs[u], prefix=prefixes[u]) for u in range(3, 6)]
        done += s.drain()
        got = dict(done)
        _same("BSSDSession", single, [got[t] for t in tickets])
        assert all(got[t]["status"] == 0 for t in tickets)
        c = s.counters()
        assert c["allocs_after_create"] == 0 and c["users_retired"] == 6, c
    assert (pa.users_served, pb.users_served) == (6, 6)
    # plain beam search in lock step; one prefix for a sub-list through prefix=
    tgb = target_generate_batch(tgt, inputs, a[1], prefix_allowed_tokens_fn=fn, prefixes=prefixes)
    _same("target_generate_batch(prefixes=)", single_tg, tgb, bssd=False)
    both = target_generate_batch(tgt, [inputs[0], inputs[2]], a[1], prefix_allowed_tokens_fn=fn, prefix=pa)
    _same("target_generate_batch(prefix=)", [single_tg[0], single_tg[2]], both, bssd=False)
    assert (pa.users_served, pb.users_served, pa.info(True)["users_served"]) == (10, 8, 6)
    with pytest.raises(ValueError):
        BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=fn, prefixes=prefixes[:5])
    with pytest.raises(ValueError):
        BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=fn, prefix=pa, prefixes=prefixes)
    release_decoders(tgt, drf)


# ------------------------------------------------------------------ 4. refusals
def test_a_prompt_that_differs_from_its_prefix_ends_alone():
    case, ci, tgt, drf = _world("k20_dk40_sigma01")
    fn, a = ci["fn"], (case["gamma"], case["max_new_tokens"])
    head_a, _, _, prompts = _six_users()
    pa = PromptPrefix(tgt, drf, head_a)
    users = [prompts[0], prompts[2].copy(), prompts[2]]
    users[1][5] += 1                                                  # one token of the prefix differs
    inputs = [_inp(p) for p in users]
    single = [BSSD(tgt, drf, inputs[u], *a, prefix_allowed_tokens_fn=fn) for u in (0, 2)]
    warm = BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=fn)            # fills the buffers the next call's torch.empty hands back
    del warm
    bat = BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=fn, prefix=pa)
    _same("others", single, [bat[0], bat[2]])
    P1 = len(users[1])
    assert bat[1]["status"] == _lib.ERR_INVALID and bat[1]["n_valid"] == 0 and bat[0]["status"] == 0 and bat[2]["status"] == 0
    assert bool(torch.isinf(bat[1]["beam_scores"]).all()) and bool((bat[1]["beam_scores"] < 0).all())
    assert bool((bat[1]["beam_sequence"][:, P1:] == 0).all())
    tgb = target_generate_batch(tgt, inputs, a[1], prefix_allowed_tokens_fn=fn, prefix=pa)
    assert [o["status"] for o in tgb] == [0, _lib.ERR_INVALID, 0]
    assert bool(torch.isinf(tgb[1]["beam_scores"]).all()) and bool((tgb[1]["beam_sequence"][:, P1:] == 0).all())
    assert torch.equal(tgb[0]["beam_sequence"], target_generate(tgt, inputs[0], a[1], prefix_allowed_tokens_fn=fn)["beam_sequence"])
    ses = BSSD_batch(tgt, drf, inputs, *a, prefix_allowed_tokens_fn=fn, prefix=pa, lanes=2)
    assert [o["status"] for o in ses] == [0, _lib.ERR_INVALID, 0] and bool(torch.isinf(ses[1]["beam_scores"]).all())
    _same("session others", single, [ses[0], ses[2]])
    for call in (lambda: BSSD(tgt, drf, inputs[1], *a, prefix_allowed_tokens_fn=fn, prefix=pa),
                 lambda: target_generate(tgt, inputs[1], a[1], prefix_allowed_tokens_fn=fn, prefix=pa)):
        with pytest.raises(_lib.AtSpeedError) as e:                   # the one-user calls return the error
            call()
        assert e.value.status == _lib.ERR_INVALID and "prefix" in e.value.message
    release_decoders(tgt, drf)


def test_refusals_before_anything_launches(monkeypatch):
    case, ci, tgt, drf = _world("k20_dk40_sigma01")
    fn, a = ci["fn"], (case["gamma"], case["max_new_tokens"])
    prompt, P = ci["prompt"], len(ci["prompt"])
    lib = _lib.load()
    other = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **KW)
    p_other, full, full_t = PromptPrefix(other, drf, prompt[:8]), PromptPrefix(tgt, drf, prompt), PromptPrefix(tgt, None, prompt)
    half, good = PromptPrefix(tgt, None, prompt[:8]), PromptPrefix(tgt, drf, prompt[:8])
    tgt.forward_log(1), drf.forward_log(1)                                            # from here on nothing may be launched
    with pytest.raises(ValueError, match="at least"):                                 # Lp = P: no suffix row for the first logits
        BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, prefix=full)
    with pytest.raises(ValueError, match="other models"):
        BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, prefix=p_other)
    with pytest.raises(ValueError, match="draft"):                                    # the target's half alone does not serve beam-SD
        BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, prefix=half)
    with pytest.raises(NotImplementedError):                                          # a mask that cannot compile() itself: the host path
        BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=lambda b, ids: fn(b, ids), prefix=good)
    with pytest.raises(NotImplementedError):
        target_generate(tgt, _inp(prompt), a[1], prefix_allowed_tokens_fn=lambda b, ids: fn(b, ids), prefix=half)
    # the library's own checks, behind the front end's: a prefix of another model on the decoder, Lp = P in a generate call
    dec = _Decoder.get(tgt, drf, P)
    assert lib.atspeed_decoder_set_prefix(dec.handle, p_other.handle(), None) == _lib.ERR_INVALID
    monkeypatch.setattr("atspeed_amd.beamSD._prefix_list", lambda prefix, prefixes, n, *rest: None if prefix is None else [prefix] * n)
    with pytest.raises(_lib.AtSpeedError) as e:
        BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, prefix=full)
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.AtSpeedError) as e:
        target_generate(tgt, _inp(prompt), a[1], prefix_allowed_tokens_fn=fn, prefix=full_t)
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.AtSpeedError) as e:                       # the target's half alone, past the front end: the library wants both or neither
        BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, prefix=half)
    assert e.value.status == _lib.ERR_INVALID
    assert tgt.forward_log(0) == [] and drf.forward_log(0) == [], "a refused call launched a forward"
    release_decoders(tgt, drf, other)


def _adapter(dims, seed, r=8, alpha=16, modules=("q", "v"), std=0.1):
    return L.from_tensors(synth.synthetic_lora(dims, seed, r=r, modules=modules, std=std), dims.n_layers, dims.hidden, r, alpha)


def test_staleness_follows_the_arithmetic_that_made_the_prefix(monkeypatch):
    V = synth.TINY.vocab_size
    dims = synth.LlamaDims(V, 256, 1, 4, 512)
    m = HipLlama.from_synthetic(dims, 9, dtype=torch.bfloat16, num_beams=4, **KW)
    fn = None                                                         # a mask-free search: every token is a candidate
    prompt = synth.synthetic_prompt(20, 77)
    pre = PromptPrefix(m, None, prompt[:8])
    ok = target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pre)
    assert ok["beam_sequence"].shape[0] == 4 and not pre.stale
    # resident adapters: an unrelated slot comes and goes, the prefix (slot 0) stays good; a prefix built under a slot dies with that slot
    m.add_lora(_adapter(dims, 70), "a")
    assert not pre.stale
    pa = PromptPrefix(m, None, prompt[:8], adapter="a")
    m.add_lora(_adapter(dims, 71), "b")
    assert not pa.stale and not pre.stale
    target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pa, adapter="a")
    with pytest.raises(ValueError, match="adapter"):                  # the user's adapter differs from the prefix's
        target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pa, adapter="b")
    with pytest.raises(ValueError, match="adapter"):
        target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pa)
    m.remove_lora("a")
    assert pa.stale and not pre.stale
    m.add_lora(_adapter(dims, 72), "a")                               # the same slot, another adapter: still stale
    assert pa.stale
    with pytest.raises(ValueError, match="stale"):
        target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pa, adapter="a")
    m.remove_lora("a"), m.remove_lora("b")
    target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pre)
    # quantised copies change every projection: stale, and the library refuses it on its own too
    m.enable_fp8()
    assert pre.stale
    with pytest.raises(ValueError, match="stale"):
        target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pre)
    monkeypatch.setattr("atspeed_amd.beamSD._prefix_list", lambda prefix, prefixes, n, *rest: None if prefix is None else [prefix] * n)
    with pytest.raises(_lib.AtSpeedError) as e:
        target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pre)
    assert e.value.status == _lib.ERR_INVALID and "stale" in e.value.message
    release_decoders(m)


# ------------------------------------------------------------------ 5. 16-bit and quantised modes, forward level
def _shared_head_seqs(n_seq, T, lp, V, max_slots, n_logit, seed):
    """n_seq sequences of T tokens that share their first lp tokens, as (full-prompt entries, suffix entries) of forward_raw_batch: the
    suffix rows carry positions and slots lp .., see the whole causal past, one slot hidden (a tree mask)"""
    g = torch.Generator().manual_seed(seed)
    head = torch.randint(3, V, (lp,), generator=g).to(torch.int32)
    full, suffix = [], []
    for i in range(n_seq):
        ids = torch.cat((head, torch.randint(3, V, (T - lp,), generator=g).to(torch.int32)))
        vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
        vis[lp + 4:, 2 + i % 5] = False
        pos = torch.arange(T, dtype=torch.int32)
        bits = vis_bits_from_bool(vis, max_slots)
        full.append((ids, pos, pos.clone(), bits, T, n_logit))
        suffix.append((ids[lp:].contiguous(), pos[lp:].contiguous(), pos[lp:].clone(), bits[lp:].contiguous(), T, n_logit))
    return head, full, suffix


@pytest.mark.parametrize("dtype,hidden,heads,ffn", [(torch.bfloat16, 768, 12, 1536), (torch.float16, 768, 12, 1536), (torch.bfloat16, 4096, 32, 11008)],
                         ids=["bf16", "fp16", "bf16_llama7b_width"])
def test_16bit_forward_behind_a_scattered_prefix(dtype, hidden, heads, ffn):
    """hidden 768 / 12 heads / 2 layers, 48 sequences: the logits of the suffix rows behind a scattered prefix against the same rows of the
    full-prompt forward, at the bar test_batched_forward_equals_per_sequence_forwards_bf16 holds two kernel routes of the same values to.
    llama7b_width: the Llama-7B layer (head_dim 128), where the batched forward writes K / V from the qkv projection's fused RoPE epilogue and
    the prefix's own one-user forward does not."""
    V = 32000 + 256
    dims = synth.LlamaDims(V, hidden, 2, heads, ffn)
    m = HipLlama.from_synthetic(dims, 77, dtype=dtype, max_slots=256, max_tokens=256, max_logit_rows=256, device=torch.device(DEV))
    lp, T, n = 36, 70, 48
    head, full, suffix = _shared_head_seqs(n, T, lp, V, 256, 4, 3)
    pre = PromptPrefix(m, None, head)
    pre.to_batch_arenas(n)                                            # first: the arenas hold nothing else yet
    m.forward_log(1), m.rope_fused_launches(reset=True)
    got = [o.float().cpu().numpy() for o in m.forward_raw_batch(suffix)]
    assert m.forward_log(0)[0][0] == n * (T - lp)
    assert (m.rope_fused_launches() == 2) == (hidden == 4096)
    want = [o.float().cpu().numpy() for o in m.forward_raw_batch(full)]
    assert pre.users_served == n
    worst = [0.0, 0.0]
    for a, b in zip(got, want):
        scale = float(np.abs(b).max())
        assert a.shape == b.shape == (4, V)
        worst = [max(worst[0], float(np.abs(a - b).max()) / scale), max(worst[1], float(np.abs(a - b).mean()) / scale)]
    print(f"prefix route vs full route, relative to max|logit|: worst max {worst[0]:.4f}, worst mean {worst[1]:.5f}")
    assert worst[0] <= 0.03 and worst[1] <= 0.004


def _fp8_applies(m, n, k):                        # tests/test_fp8_gpu.py's restatement of the fp8 ring kernel's rule (gemm.hip: ats_gemm_fp8_applies)
    fill = lambda t: t * 100 // (((t + 255) // 256) * 256)
    tn = (n + 255) // 256
    return m >= 512 and k % 256 == 0 and (fill(tn * ((m + 255) // 256)) >= 60 or fill(tn * ((m + 127) // 128)) >= 60)


def test_w8a8_forward_behind_a_scattered_prefix():
    """bf16 W8A8 at the shape of tests/test_fp8_gpu.py (hidden 2048, 2 layers; enough rows for every projection of both forwards to take the
    fp8 kernels, which the counters assert).  The bar is that file's bar for two routes to the same W8A8 values, measured here against the
    scheme's own noise on these inputs (W8A8 oracle against the fp32 oracle): mean below 0.85 x its mean, max below its max."""
    H, F, HEADS, LAYERS = 2048, 5632, 16, 2
    V = synth.BEAUTY.vocab_size
    dims = synth.LlamaDims(V, H, LAYERS, HEADS, F)
    m = HipLlama.from_synthetic(dims, 31, std=0.03, head_std=0.2, dtype=torch.bfloat16, **KW)
    sd = m.export_state_dict()
    m.enable_fp8()
    lp, T, n = 36, 100, 40                                            # 4000 full-prompt rows, 2560 suffix rows: both fill every projection's grid
    assert all(_fp8_applies(rows, nn, kk) for rows in (n * T, n * (T - lp)) for nn, kk in ((3 * H, H), (H, H), (2 * F, H), (H, F)))
    head, full, suffix = _shared_head_seqs(n, T, lp, V, 512, 6, 5)
    pre = PromptPrefix(m, None, head)
    pre.to_batch_arenas(n)
    m.fp8_counters(reset=True)
    got = [o.float().cpu() for o in m.forward_raw_batch(suffix)]
    cnt = m.fp8_counters(reset=True)
    assert all(c["fp8"] == LAYERS and c["other"] == 0 for c in cnt.values()), cnt
    want = [o.float().cpu() for o in m.forward_raw_batch(full)]
    cnt = m.fp8_counters()
    assert all(c["fp8"] == LAYERS and c["other"] == 0 for c in cnt.values()), cnt
    ref8, ref32 = RefLlama(dims, sd, max_slots=512, w8a8=True), RefLlama(dims, sd, max_slots=512)
    figures = []
    for i in (0, 31):
        ids, pos, slots, _, _, _ = full[i]
        vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
        vis[lp + 4:, 2 + i % 5] = False
        want8 = ref8.forward(ids, pos, slots, vis, n_logit_rows=6)
        want32 = ref32.forward(ids, pos, slots, vis, n_logit_rows=6)
        scale = float(want8.abs().max())
        qn = (want8 - want32).abs() / scale                           # the scheme's own noise on this sequence
        d = (got[i] - want[i]).abs() / scale
        e8 = (got[i] - want8).abs() / scale
        figures.append((float(d.mean()), float(d.max()), float(e8.mean()), float(e8.max()), float(qn.mean()), float(qn.max())))
    print("W8A8, relative to max|logit|: prefix route vs full route (mean, max), prefix route vs W8A8 oracle (mean, max), scheme noise (mean, max):", figures)
    for d_mean, d_max, e8_mean, e8_max, qn_mean, qn_max in figures:
        assert d_mean < 0.85 * qn_mean and d_max < qn_max
        assert e8_mean < 0.85 * qn_mean and e8_max < qn_max          # and the prefix route meets the fp8 test's own bar against the oracle


def test_16bit_forward_with_a_prefix_per_adapter():
    """add_lora twice, one prefix per adapter, four users [a, a, b, b] in one forward behind their scattered prefixes: each user's suffix
    logits against its own full-prompt forward under its adapter, at the 16-bit bar; the adapters move the logits by more than the bar"""
    V = 32000 + 256
    dims = synth.LlamaDims(V, 768, 2, 12, 1536)
    m = HipLlama.from_synthetic(dims, 77, dtype=torch.bfloat16, num_beams=4, max_slots=256, max_tokens=256, max_logit_rows=256, device=torch.device(DEV))
    m.add_lora(_adapter(dims, 70, std=0.3), "a").add_lora(_adapter(dims, 71, std=0.3), "b")
    lp, T = 36, 70
    head, full, suffix = _shared_head_seqs(4, T, lp, V, 256, 4, 9)
    names = ["a", "a", "b", "b"]
    pa, pb = PromptPrefix(m, None, head, adapter="a"), PromptPrefix(m, None, head, adapter="b")
    assert not torch.equal(pa.read()[1][0], pb.read()[1][0]), "the adapters change V, so the two prefixes differ"
    pa.to_batch_arenas(2, first=0)
    pb.to_batch_arenas(2, first=2)
    got = [o.float().cpu().numpy() for o in m.forward_raw_batch(suffix, adapters=names)]
    for u in range(4):
        own = m.forward_raw_batch([full[u]], adapters=[names[u]])[0].float().cpu().numpy()
        scale = float(np.abs(own).max())
        assert float(np.abs(got[u] - own).max()) <= 0.03 * scale and float(np.abs(got[u] - own).mean()) <= 0.004 * scale, u
    fn = None
    prompt = np.concatenate((head.numpy().astype(np.int64), synth.synthetic_prompt(12, 5)[1:]))
    with pytest.raises(ValueError, match="adapter"):
        target_generate(m, _inp(prompt), 2, prefix_allowed_tokens_fn=fn, prefix=pa, adapter="b")
    release_decoders(m)


def test_sampling_with_a_prefix_draws_the_same_beams():
    case, ci, tgt, drf = _world("k20_dk40_sigma01")
    fn, a = ci["fn"], (case["gamma"], case["max_new_tokens"])
    prompt = ci["prompt"]
    pre = PromptPrefix(tgt, drf, prompt[:8])
    try:
        for m in (tgt, drf):
            m.generation_config.do_sample = True
        plain = BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, seed=3)
        behind = BSSD(tgt, drf, _inp(prompt), *a, prefix_allowed_tokens_fn=fn, seed=3, prefix=pre)
        assert torch.equal(plain["beam_sequence"], behind["beam_sequence"])
        np.testing.assert_allclose(plain["beam_scores"].cpu().numpy(), behind["beam_scores"].cpu().numpy(), atol=SCORE_TOL, rtol=0)
        assert (plain["n_run"], plain["accept_steps"]) == (behind["n_run"], behind["accept_steps"])
    finally:
        for m in (tgt, drf):
            m.generation_config.do_sample = False
    release_decoders(tgt, drf)


# ------------------------------------------------------------------ 6. the harness
class WordTokenizer:
    """a tokenizer stand-in over the prompt TEXT (the reference's template): BOS, one id per whitespace-separated word, the Response separator"""

    def encode(self, text):
        ids = [3 + zlib.crc32(w.encode()) % 31000 for w in text.split()[:-1]]              # the last word is "Response:"
        return [1] + [t + 1 if t == synth.RESPONSE_SEP[0] else t for t in ids] + list(synth.RESPONSE_SEP)


def test_harness_share_prefix_returns_the_same_predictions_and_builds_one_prefix():
    from atspeed_amd.harness import ItemIndex, SeqRecTestData, common_prefix, encode_prompt, run_inference
    rng = np.random.default_rng(3)
    idx = {str(i): [f"<a_{rng.integers(48)}>", f"<b_{rng.integers(8)}>", f"<c_{rng.integers(8)}>", f"<d_{rng.integers(8)}>"] for i in range(300)}
    ix = ItemIndex(idx)
    train = {u: rng.integers(0, 300, size=rng.integers(1, 12)).tolist() for u in range(12)}
    valid = {u: rng.integers(0, 300, size=1).tolist() for u in range(12)}
    test = {u: (rng.integers(0, 300, size=1).tolist() if u % 4 else []) for u in range(12)}
    data = SeqRecTestData(ix, train, valid, test)
    tok = WordTokenizer()
    header = common_prefix([encode_prompt(data, u, tok).tolist() for u in data.users])
    assert len(header) >= 8
    V = ix.vocab_size
    kw = dict(dtype=torch.float32, max_slots=512, max_tokens=512, max_logit_rows=448)
    d = HipLlama.from_synthetic(synth.LlamaDims(V, 96, 2, 3, 256), 5, num_beams=20, resid_scale=1.0, **kw)
    t = HipLlama.from_synthetic(synth.LlamaDims(V, 128, 3, 4, 352), 6, num_beams=10, resid_scale=1.0, align_to=d, **kw)
    for extra in (dict(), dict(decoder="beam"), dict(stream_lanes=3)):
        base = run_inference(t, d, data, gamma=4, max_new_tokens=4, users_per_batch=4, tokenizer=tok, **extra)
        t.forward_log(1)
        shr = run_inference(t, d, data, gamma=4, max_new_tokens=4, users_per_batch=4, tokenizer=tok, share_prefix=True, **extra)
        log = t.forward_log(0)
        assert base.prefixes_built == 0 and shr.prefixes_built == 1 and shr.prefix_users == 9, (extra, shr.prefixes_built)
        assert log[0][0] == len(header), log[:2]                      # the run's first target forward makes the prefix: the template's header
        assert shr.predictions == base.predictions and shr.uids == base.uids and len(shr.predictions) == 9
        assert shr.metrics(ix) == base.metrics(ix)
        np.testing.assert_allclose(np.asarray(shr.scores), np.asarray(base.scores), atol=SCORE_TOL, rtol=0)
        assert [r["n_run"] for r in shr.rows] == [r["n_run"] for r in base.rows]
    release_decoders(t, d)
