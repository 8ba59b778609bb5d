"""Beam-SD sessions (`BSSDSession`, `BSSD_batch(..., lanes=N)`, `run_inference(..., stream_lanes=N)`): a fixed set of lanes, a queue of users,
each free lane refilled at the next round boundary.  Every user must equal its own `BSSD` call, whichever lane it lands on and whoever
shares its rounds; the lanes must really be refilled (round counter = the admission simulation, below the chunked count); nothing may be
allocated after the session was created."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import atspeed_amd
from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, BSSDSession, release_decoders
from atspeed_amd.generation_trie import Trie, prefix_allowed_tokens_fn
from atspeed_amd.model import HipLlama
from tests.golden.cases import CASES, build_case_inputs

CASE = "k6_dk12_new7_gamma3_s9"          # gamma 3, 7 new tokens, K 6, DK 12: users stay 3 to 7 rounds
N_USERS, LANES = 24, 4
# loop iterations of the lock-step engine per user of the 24 prompts below, from the CPU oracle's n_run (rounds = n_run + 1)
ORACLE_ROUNDS = [7, 6, 4, 5, 5, 5, 3, 4, 6, 7, 6, 4, 4, 4, 5, 3, 5, 5, 5, 5, 5, 6, 7, 5]
SCORE_TOL = 1e-4                          # the bound of test_bssd_batch_equals_sequential_calls: the GEMM tiling depends on who shares a forward


def _inputs(prompts):
    return [{"input_ids": torch.from_numpy(np.asarray(p, dtype=np.int64))[None].cuda()} for p in prompts]


def rounds_of(result) -> int:
    """The engine's rule (DESIGN.md "Sessions"): a user takes part in one round per verification (n_run) and in one more, which is its final
    single step (beamSD.py:505-509) or, when the last verification already produced the last token, the export of its beams."""
    return int(result["n_run"]) + 1


def refilled_rounds(need, lanes: int) -> int:
    """Rounds a session of `lanes` lanes runs for users needing need[u] rounds, in submission order, each free lane refilled at the boundary."""
    queue, busy, rounds = list(need), [], 0
    while queue or busy:
        while queue and len(busy) < lanes:
            busy.append(queue.pop(0))
        rounds += 1
        busy = [r - 1 for r in busy if r > 1]
    return rounds


def chunked_rounds(need, chunk: int) -> int:
    return sum(max(need[i:i + chunk]) for i in range(0, len(need), chunk))


def assert_same_user(single, other, what=""):
    assert torch.equal(single["beam_sequence"], other["beam_sequence"]), what
    np.testing.assert_allclose(single["beam_scores"].cpu().numpy(), other["beam_scores"].cpu().numpy(), atol=SCORE_TOL, rtol=0, err_msg=str(what))
    assert (single["n_run"], single["total_accept_steps"], single["accept_steps"]) == (other["n_run"], other["total_accept_steps"], other["accept_steps"]), what


@pytest.fixture(scope="module")
def stream_run():
    """Models of the golden case, the 24 prompts + the golden case's own prompt as user 24, every user's single BSSD call (the reference of
    all tests here, computed once) and ONE run of the 25 users through a 4-lane session."""
    case = [c for c in CASES if c["name"] == CASE][0]
    ci = build_case_inputs(case)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **kw)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **kw)
    prompts = [synth.synthetic_prompt(18 + 5 * (u % 7), 900 + u) for u in range(N_USERS)] + [ci["prompt"]]
    inputs = _inputs(prompts)
    args = (case["gamma"], case["max_new_tokens"])
    single = [BSSD(tgt, drf, inp, *args, prefix_allowed_tokens_fn=ci["fn"]) for inp in inputs]
    ses = BSSD_batch(tgt, drf, inputs, *args, prefix_allowed_tokens_fn=ci["fn"], lanes=LANES)
    yield dict(case=case, ci=ci, tgt=tgt, drf=drf, prompts=prompts, inputs=inputs, args=args, single=single, ses=ses)
    release_decoders(tgt, drf)


def test_every_user_of_a_session_equals_its_single_call(stream_run, bssd_golden):
    r = stream_run
    assert len(r["ses"]) == N_USERS + 1
    for u, (a, b) in enumerate(zip(r["single"], r["ses"])):
        assert_same_user(a, b, f"user {u}")
        assert b["status"] == 0 and b["rounds_in_lane"] == rounds_of(a) and 0 <= b["lane"] < LANES
        for key in ("total_accept_tokens", "ave_accept_tokens", "draft_time_cost", "target_time_cost", "verify_time_cost", "time_cost",
                    "n_valid", "n_target_forwards", "n_draft_forwards", "rounds_queued"):
            assert key in b
        assert (b["n_target_forwards"], b["n_draft_forwards"]) == (a["n_target_forwards"], a["n_draft_forwards"])     # per user, not per round
    gold, P, g = bssd_golden[CASE], len(r["ci"]["prompt"]), r["ses"][N_USERS]
    assert g["beam_sequence"][:, P:].cpu().tolist() == gold["bssd_tokens"]
    np.testing.assert_allclose(g["beam_scores"].cpu().numpy(), gold["bssd_scores"], atol=1e-3, rtol=0)
    assert [g["n_run"], g["total_accept_steps"]] == [gold["n_run"], gold["total_accept_steps"]]
    assert g["accept_steps"] == [x["n_matches"] for x in gold["rounds"]]


def test_lanes_are_refilled(stream_run):
    r = stream_run
    need = [rounds_of(o) for o in r["ses"]]
    print("rounds per user", need)
    assert need[:N_USERS] == ORACLE_ROUNDS                   # what the CPU oracle gave for these prompts
    assert max(need) - min(need) >= 2                        # unequal users: equal ones would pass everything below trivially
    c = r["ses"][0]["session_counters"]
    print("session counters", c)
    assert c["rounds"] == refilled_rounds(need, LANES)
    assert c["rounds"] < chunked_rounds(need, LANES)
    assert refilled_rounds(need[:N_USERS], LANES) == 31 and chunked_rounds(need[:N_USERS], LANES) == 36
    assert c["allocs_after_create"] == 0
    assert c["users_admitted"] == c["users_retired"] == N_USERS + 1 and c["lane_rounds"] == sum(need)
    assert c["lanes_occupied"] == 0 and c["queued"] == 0 and c["n_lanes"] == LANES
    assert max(o["n_target_forwards"] for o in r["ses"]) <= c["target_forwards"] <= c["rounds"]     # one packed forward per round that needs one
    assert sum(o["n_draft_forwards"] for o in r["ses"]) >= c["draft_forwards"] >= max(o["n_draft_forwards"] for o in r["ses"])
    assert c["arena_reserved"] == 0 and c["arena_failed"] == 0      # fp32 models take no split-K arena
    # in submission order: user u waits exactly until a lane is free
    assert [o["rounds_queued"] for o in r["ses"][:LANES]] == [0] * LANES
    assert all(b["rounds_queued"] >= a["rounds_queued"] for a, b in zip(r["ses"], r["ses"][1:]))


def test_users_that_arrive_while_others_decode(stream_run):
    r = stream_run
    fn = r["ci"]["fn"]
    with BSSDSession(r["tgt"], r["drf"], LANES, *r["args"], prefix_allowed_tokens_fn=fn) as ses:
        assert ses.step() == [] and ses.counters()["rounds"] == 0           # nothing queued, no lane occupied: nothing happens
        tickets = [ses.submit(inp) for inp in r["inputs"][:6]]
        got = ses.step() + ses.step()
        assert ses.counters()["rounds"] == 2 and ses.counters()["lanes_occupied"] == LANES
        tickets += [ses.submit(inp) for inp in r["inputs"][6:12]]
        got += ses.drain()
        assert ses.step() == []
        c = ses.counters()
    assert tickets == list(range(1, 13))
    assert sorted(t for t, _ in got) == tickets                             # every ticket once
    for t, res in got:
        assert_same_user(r["single"][t - 1], res, f"ticket {t}")
    assert c["users_admitted"] == c["users_retired"] == 12 and c["allocs_after_create"] == 0
    assert [res["rounds_queued"] for t, res in sorted(got)[:LANES]] == [0] * LANES


def test_one_lane_all_lanes_and_an_overlong_prompt(stream_run):
    r = stream_run
    fn, users = r["ci"]["fn"], [0, 1, 2, 6, 24]
    ins = [r["inputs"][u] for u in users]
    need = [rounds_of(r["single"][u]) for u in users]
    one = BSSD_batch(r["tgt"], r["drf"], ins, *r["args"], prefix_allowed_tokens_fn=fn, lanes=1)
    for u, o in zip(users, one):
        assert_same_user(r["single"][u], o, f"lanes=1 user {u}")
    assert one[0]["session_counters"]["rounds"] == sum(need)                # one user after the other
    lock = BSSD_batch(r["tgt"], r["drf"], ins, *r["args"], prefix_allowed_tokens_fn=fn)
    assert [rounds_of(o) for o in lock] == need
    with BSSDSession(r["tgt"], r["drf"], 8, *r["args"], prefix_allowed_tokens_fn=fn) as ses:       # 8 lanes, 5 users: three lanes stay empty
        tickets = [ses.submit(inp) for inp in ins]
        wide = dict(ses.drain())
        c = ses.counters()
    for t, a in zip(tickets, lock):
        assert_same_user(a, wide[t], "lanes >= users")
        assert wide[t]["rounds_queued"] == 0 and wide[t]["lane"] == t - 1
    # everybody starts in round 1, as in the lock-step call, whose loop runs until its slowest user is done
    assert c["n_lanes"] == 8 and c["rounds"] == max(rounds_of(o) for o in lock) and c["lane_rounds"] == sum(need)
    clamped = BSSD_batch(r["tgt"], r["drf"], ins, *r["args"], prefix_allowed_tokens_fn=fn, lanes=8)  # the list call takes no more lanes than users
    assert clamped[0]["session_counters"]["n_lanes"] == len(users) and clamped[0]["session_counters"]["rounds"] == max(need)
    with BSSDSession(r["tgt"], r["drf"], 2, *r["args"], prefix_allowed_tokens_fn=fn, max_prompt=40) as ses:
        t1 = ses.submit(r["inputs"][0])
        long_prompt = np.concatenate([synth.synthetic_prompt(30, 5)[:-len(synth.RESPONSE_SEP)], synth.synthetic_prompt(30, 6)])
        with pytest.raises(_lib.AtSpeedError) as ei:
            ses.submit(_inputs([long_prompt])[0])
        assert ei.value.status == _lib.ERR_CAPACITY and "max_prompt" in ei.value.message
        t2 = ses.submit(r["inputs"][1])
        got = dict(ses.drain())
        assert (t1, t2) == (1, 2) and sorted(got) == [1, 2]
        assert_same_user(r["single"][0], got[1])
        assert_same_user(r["single"][1], got[2])
    with pytest.raises(ValueError):
        BSSDSession(r["tgt"], r["drf"], 2, *r["args"], prefix_allowed_tokens_fn=lambda b, s: [2])       # a host-side mask
    with pytest.raises(ValueError):
        BSSDSession(r["tgt"], r["drf"], 2, *r["args"], prefix_allowed_tokens_fn=fn, logits_processor=[lambda i, s: s])
    with pytest.raises(ValueError):
        BSSDSession(r["tgt"], r["drf"], 2, *r["args"], prefix_allowed_tokens_fn=fn, trace_decisions=True)
    other = atspeed_amd.PositionSetConstraint(r["ci"]["fn"].allowed_tokens, synth.RESPONSE_SEP)          # an equal automaton, but not the same one
    with BSSDSession(r["tgt"], r["drf"], 2, *r["args"], prefix_allowed_tokens_fn=fn) as ses:
        ses.submit(r["inputs"][0])
        ses.fn = other
        with pytest.raises(ValueError):
            ses.submit(r["inputs"][1])


def test_library_drain_and_its_capacity_check(stream_run):
    """atspeed_session_drain itself (BSSDSession.drain is one call of it): with too little room for the pending users it is refused before
    anything is launched -- nobody admitted, no round -- and the session goes on; with room every ticket comes back once."""
    import ctypes as C
    r = stream_run
    lib = _lib.load()
    with BSSDSession(r["tgt"], r["drf"], 3, *r["args"], prefix_allowed_tokens_fn=r["ci"]["fn"]) as ses:
        tickets = [ses.submit(inp) for inp in r["inputs"][:7]]
        small, n = (_lib.SessionDone * 6)(), C.c_int32(-1)
        assert lib.atspeed_session_drain(ses._owner.ptr, small, 6, C.byref(n)) == _lib.ERR_CAPACITY and n.value == 0
        assert b"7 users pending" in lib.atspeed_last_error()
        assert lib.atspeed_session_round(ses._owner.ptr, small, 2, C.byref(n)) == _lib.ERR_CAPACITY and n.value == 0     # 3 lanes can finish 3
        c = ses.counters()
        assert (c["rounds"], c["users_admitted"], c["queued"], c["lanes_occupied"]) == (0, 0, 7, 0)
        first = ses.step()                                   # one round through the library, then the rest in ONE drain call
        assert first == [] and ses.counters()["rounds"] == 1
        got = ses.drain()
        c = ses.counters()
        assert ses.drain() == [] and ses.step() == []
    assert sorted(t for t, _ in got) == tickets == list(range(1, 8))
    for t, res in got:
        assert_same_user(r["single"][t - 1], res, f"ticket {t}")
    need = [rounds_of(r["single"][u]) for u in range(7)]
    assert c["rounds"] == refilled_rounds(need, 3) and c["users_retired"] == 7 and c["allocs_after_create"] == 0
    finish = got_round(need, 3)
    assert [finish[t - 1] for t, _ in got] == sorted(finish)            # records come in the order the users finished


def got_round(need, lanes: int):
    """The round in which each user of `need` finishes under the admission rule."""
    queue, busy, rounds, out = list(enumerate(need)), [], 0, [0] * len(need)
    while queue or busy:
        while queue and len(busy) < lanes:
            busy.append(list(queue.pop(0)))
        rounds += 1
        for b in busy:
            b[1] -= 1
            if b[1] == 0:
                out[b[0]] = rounds
        busy = [b for b in busy if b[1] > 0]
    return out


def test_a_prompt_that_could_run_out_of_kv_slots_is_refused_at_submit(stream_run):
    """A session refuses at submit what could exhaust the KV slots inside a round (prompt + (max_new_tokens - 1) x DK > max_slots), where it
    costs nobody else a round; the session stays usable, and a prompt just inside the bound is decoded like its single call."""
    r = stream_run
    fn, dk, new = r["ci"]["fn"], r["case"]["DK"], r["case"]["max_new_tokens"]
    limit = 512 - (new - 1) * dk                              # max_slots of the fixture's models
    inside, outside = _inputs([synth.synthetic_prompt(limit, 31), synth.synthetic_prompt(limit + 1, 32)])
    with BSSDSession(r["tgt"], r["drf"], 2, *r["args"], prefix_allowed_tokens_fn=fn, max_prompt=512) as ses:
        t1 = ses.submit(r["inputs"][3])
        with pytest.raises(_lib.AtSpeedError) as ei:
            ses.submit(outside)
        assert ei.value.status == _lib.ERR_CAPACITY and "KV slots" in ei.value.message
        t2 = ses.submit(inside)
        got = dict(ses.drain())
        assert (t1, t2) == (1, 2) and sorted(got) == [1, 2] and ses.counters()["users_admitted"] == 2
    assert_same_user(r["single"][3], got[1])
    assert_same_user(BSSD(r["tgt"], r["drf"], inside, *r["args"], prefix_allowed_tokens_fn=fn), got[2])
    with pytest.raises(_lib.AtSpeedError):                   # the list call says the same, before it decodes anybody
        BSSD_batch(r["tgt"], r["drf"], [r["inputs"][0], outside], *r["args"], prefix_allowed_tokens_fn=fn, lanes=2)


def test_sampling_seeds_follow_users_not_lanes(stream_run):
    r = stream_run
    fn, n = r["ci"]["fn"], 10
    for m in (r["tgt"], r["drf"]):
        m.generation_config.do_sample, m.generation_config.temperature = True, 1.0
    try:
        ses = BSSD_batch(r["tgt"], r["drf"], r["inputs"][:n], *r["args"], prefix_allowed_tokens_fn=fn, lanes=LANES, seed=100)
        for u, o in enumerate(ses):
            one = BSSD(r["tgt"], r["drf"], r["inputs"][u], *r["args"], prefix_allowed_tokens_fn=fn, seed=100 + u)
            assert_same_user(one, o, f"sampled user {u}")
        assert len({o["lane"] for o in ses}) == LANES and ses[0]["session_counters"]["allocs_after_create"] == 0
    finally:
        for m in (r["tgt"], r["drf"]):
            m.generation_config.do_sample = False


def test_a_filtered_user_frees_its_lane_and_harms_nobody():
    """The prompts and the trie of test_a_filtered_user_does_not_abort_the_lock_step_batch, repeated to 9 users on 2 lanes: every third user
    loses all beams of its first step to the id filter."""
    case = [c for c in CASES if c["name"] == "k5_dk10_indep"][0]
    ci = build_case_inputs(case)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448, device="cuda:0")
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **kw)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **kw)
    pa, pb, pc = [1, 50, 51, 52], [1, 60, 61], [1, 70, 71, 72, 73]
    items = [[32000 + i, 32064 + (3 * i) % 64, 32128 + (5 * i) % 64, 32192 + (7 * i) % 64, 2] for i in range(24)]
    seqs = [pa + it for it in items] + [pc + it for it in items[:12]] + [pb + [7 + i, 8, 9, 10, 2] for i in range(6)]
    fn = prefix_allowed_tokens_fn(Trie(seqs))
    three = [{"input_ids": torch.tensor([p], dtype=torch.int64).cuda()} for p in (pa, pb, pc)]
    ones = {u: BSSD(tgt, drf, three[u], 4, 4, prefix_allowed_tokens_fn=fn) for u in (0, 2)}
    for _ in range(2):           # twice: the second run's result buffers are the first run's blocks, a filtered user must not keep what they held
        res = BSSD_batch(tgt, drf, three * 3, 4, 4, prefix_allowed_tokens_fn=fn, lanes=2)
    assert [o["status"] for o in res] == [0, _lib.ERR_FILTERED, 0] * 3
    for u, o in enumerate(res):
        if u % 3 == 1:
            assert o["n_valid"] == 0 and bool(torch.isneginf(o["beam_scores"]).all()) and int(o["beam_sequence"][:, len(pb):].abs().sum()) == 0
            assert o["rounds_in_lane"] == 1
            continue
        one = ones[u % 3]
        nv = one["n_valid"]
        assert o["n_valid"] == nv >= 1 and torch.equal(o["beam_sequence"][:nv], one["beam_sequence"][:nv])
        np.testing.assert_allclose(o["beam_scores"][:nv].cpu().numpy(), one["beam_scores"][:nv].cpu().numpy(), atol=SCORE_TOL, rtol=0)
        assert (o["n_run"], o["accept_steps"]) == (one["n_run"], one["accept_steps"])
    c = res[0]["session_counters"]
    assert c["users_retired"] == 9 and c["allocs_after_create"] == 0
    release_decoders(tgt, drf)


def test_bf16_session_against_single_calls():
    """bf16 at the dims of test_bssd_bf16_is_lossless_against_own_target_generate, 32 users on 8 lanes, under that test's rule: scores within
    5e-2, identical items where the smallest score gap exceeds 5e-2, at least 18 of 20 items otherwise."""
    V = synth.BEAUTY.vocab_size
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_synthetic(synth.LlamaDims(V, 512, 2, 8, 1376), 11, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=20, **kw)
    drf = HipLlama.from_synthetic(synth.LlamaDims(V, 256, 2, 4, 704), 12, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=40, **kw)
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    prompts = [synth.synthetic_prompt(40 + 17 * (u % 5), 100 + u) for u in range(32)]
    inputs = _inputs(prompts)
    ses = BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn, lanes=8)
    assert len(ses) == 32
    for p, inp, a in zip(prompts, inputs, ses):
        b = BSSD(tgt, drf, inp, 4, 4, prefix_allowed_tokens_fn=fn)
        sa, sb = a["beam_scores"].cpu().numpy(), b["beam_scores"].cpu().numpy()
        np.testing.assert_allclose(sa, sb, atol=5e-2, rtol=0)
        ta, tb = a["beam_sequence"][:, len(p):].cpu().tolist(), b["beam_sequence"][:, len(p):].cpu().tolist()
        if np.abs(np.diff(sb)).min() > 5e-2:
            assert ta == tb
        assert len({tuple(x) for x in ta} & {tuple(x) for x in tb}) >= 18
    c = ses[0]["session_counters"]
    print("bf16 session counters", c)
    assert c["users_retired"] == 32 and c["allocs_after_create"] == 0 and c["arena_failed"] == 0
    # 8 lanes x (longest prompt 108 + 4 x 40) tokens: the worst round passes 257 tokens, so create reserved the split-K arena
    assert c["arena_reserved"] == 1 and tgt.sk_arena_bytes() > 0
    release_decoders(tgt, drf)


def test_harness_stream_lanes_returns_the_default_predictions():
    """run_inference(stream_lanes=4) on the tiny dataset of test_harness_end_to_end_on_a_tiny_dataset."""
    from atspeed_amd.harness import ItemIndex, SeqRecTestData, run_inference
    rng = np.random.default_rng(3)
    idx = {str(i): [f"<a_{rng.integers(48)}>", f"<b_{rng.integers(8)}>", f"<c_{rng.integers(8)}>", f"<d_{rng.integers(8)}>"] for i in range(300)}
    ix = ItemIndex(idx)
    train = {u: rng.integers(0, 300, size=rng.integers(1, 12)).tolist() for u in range(12)}
    valid = {u: rng.integers(0, 300, size=1).tolist() for u in range(12)}
    test = {u: (rng.integers(0, 300, size=1).tolist() if u % 4 else []) for u in range(12)}
    data = SeqRecTestData(ix, train, valid, test)
    V = ix.vocab_size
    kw = dict(dtype=torch.float32, max_slots=512, max_tokens=512, max_logit_rows=448)
    d = HipLlama.from_synthetic(synth.LlamaDims(V, 96, 2, 3, 256), 5, num_beams=20, resid_scale=1.0, **kw)
    t = HipLlama.from_synthetic(synth.LlamaDims(V, 128, 3, 4, 352), 6, num_beams=10, resid_scale=1.0, align_to=d, **kw)
    strict = data.strict_trie_fn()
    for fn in (strict, None):                # the strict trie, then the position-set mask inference.py uses
        base = run_inference(t, d, data, gamma=4, max_new_tokens=4, users_per_batch=4, prefix_allowed_tokens_fn=fn)
        ses = run_inference(t, d, data, gamma=4, max_new_tokens=4, users_per_batch=4, prefix_allowed_tokens_fn=fn, stream_lanes=4)
        assert ses.predictions == base.predictions and ses.uids == base.uids and len(ses.predictions) == 9
        assert [r["n_run"] for r in ses.rows] == [r["n_run"] for r in base.rows]
        assert [r["total_accept_steps"] for r in ses.rows] == [r["total_accept_steps"] for r in base.rows]
        np.testing.assert_allclose(np.asarray(ses.scores), np.asarray(base.scores), atol=SCORE_TOL, rtol=0)
    with pytest.raises(ValueError):
        run_inference(t, d, data, decoder="beam", stream_lanes=4)
    release_decoders(t, d)
