"""Staged verification (DESIGN.md "Staged verification", switch `verify_staged`): a greedy lock-step round forwards the round inputs first and
then one draft block per phase, only for the users whose verify walk is still alive.  Decisions come from the same walk on logits of the same
math, so a staged run must equal the packed run: tokens, accepted steps and counters exactly, scores within 1e-3 (the GEMM's M differs).
Small fp32 models from tests/golden; the packed run of the shared users is computed once."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, BSSDSession, release_decoders
from atspeed_amd.model import HipLlama
from tests.golden.cases import CASES, build_case_inputs
from tests.round_ref import expected_draft_log, expected_log

KW = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
SCORE_TOL = 1e-3
MIX_CASE = "k6_dk12_new7_gamma3_s9"       # gamma 3, 7 new tokens, K 6, DK 12 (the models of tests/test_stream_gpu.py)
# six of that file's prompts, by the CPU oracle's accepted steps per round: 0 and 3 stop at step 0 of their first rounds ([0,0,0,0,0,0] and
# [0,0,2,0]), 6 and 7 stop mid-walk ([2,2] and [2,0,1]), 15 and 2 have a round that accepts every block ([1,3]: 3 of 3; [2,1,1]: the last 1 of 1)
MIX_USERS = [0, 3, 6, 7, 15, 2]
MIX_ORACLE = [[0, 0, 0, 0, 0, 0], [0, 0, 2, 0], [2, 2], [2, 0, 1], [1, 3], [2, 1, 1]]


def _case(name):
    return [c for c in CASES if c["name"] == name][0]


def _models(case, ci):
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **KW)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **KW)
    return tgt, drf


def _inputs(prompts):
    return [{"input_ids": torch.from_numpy(np.asarray(p, dtype=np.int64))[None].cuda()} for p in prompts]


def _threshold() -> int:
    v = C.c_int32(0)
    _lib.check(_lib.load().atspeed_get_switch(b"verify_staged_tokens", C.byref(v)))
    return int(v.value)


def _logged(tgt, drf, inputs, gamma, new, fn, mode, switches=None, **kw):
    """One BSSD_batch call with the switch at `mode` -> (results, the target's forward log [(tokens, logit rows)])."""
    with _lib.switches(verify_staged=mode, **(switches or {})):
        tgt.forward_log(1)
        outs = BSSD_batch(tgt, drf, inputs, gamma, new, prefix_allowed_tokens_fn=fn, **kw)
        log = tgt.forward_log(0)
    return outs, [tuple(int(x) for x in e) for e in log]


def assert_same_user(a, b, what=""):
    """everything the golden tests compare, staged (b) against packed (a)"""
    assert torch.equal(a["beam_sequence"], b["beam_sequence"]), what
    np.testing.assert_allclose(a["beam_scores"].cpu().numpy(), b["beam_scores"].cpu().numpy(), atol=SCORE_TOL, rtol=0, err_msg=str(what))
    for key in ("n_run", "total_accept_steps", "accept_steps", "n_valid", "n_target_forwards", "n_draft_forwards"):
        assert a[key] == b[key], (what, key, a[key], b[key])


@pytest.fixture(scope="module")
def mix():
    """The mixed batch's models and six users, their packed run (switch 0) and their staged run (switch 2), each once."""
    case = _case(MIX_CASE)
    ci = build_case_inputs(case)
    tgt, drf = _models(case, ci)
    prompts = [synth.synthetic_prompt(18 + 5 * (u % 7), 900 + u) for u in range(24)]
    inputs = _inputs(prompts)
    args = (case["gamma"], case["max_new_tokens"])
    six = [inputs[u] for u in MIX_USERS]
    drf.forward_log(1)
    packed, plog = _logged(tgt, drf, six, *args, ci["fn"], 0)
    pdlog = [tuple(int(x) for x in e) for e in drf.forward_log(1)]         # the draft's forwards of the packed call; the log starts again
    staged, slog = _logged(tgt, drf, six, *args, ci["fn"], 2)
    sdlog = [tuple(int(x) for x in e) for e in drf.forward_log(0)]
    yield dict(case=case, ci=ci, tgt=tgt, drf=drf, prompts=prompts, inputs=inputs, args=args, packed=packed, plog=plog, staged=staged, slog=slog,
               pdlog=pdlog, sdlog=sdlog)
    release_decoders(tgt, drf)


@pytest.mark.parametrize("name", ["k20_dk40_sigma01_s7", "k8_dk16_trie"])
def test_golden_cases_forced_staged(name, bssd_golden):
    case, gold = _case(name), bssd_golden[name]
    ci = build_case_inputs(case)
    tgt, drf = _models(case, ci)
    one = _inputs([ci["prompt"]])
    args = (case["gamma"], case["max_new_tokens"])
    packed, plog = _logged(tgt, drf, one, *args, ci["fn"], 0)
    staged, slog = _logged(tgt, drf, one, *args, ci["fn"], 2)
    g, P = staged[0], len(ci["prompt"])
    assert g["beam_sequence"][:, P:].cpu().tolist() == gold["bssd_tokens"]
    np.testing.assert_allclose(g["beam_scores"].cpu().numpy(), gold["bssd_scores"], atol=SCORE_TOL, rtol=0)
    assert g["accept_steps"] == [x["n_matches"] for x in gold["rounds"]]
    assert [g["n_run"], g["total_accept_steps"]] == [gold["n_run"], gold["total_accept_steps"]]
    assert g["n_target_forwards"] == packed[0]["n_target_forwards"] == len(plog)
    assert_same_user(packed[0], g, name)
    # the run really was staged: every verification round starts with a forward of the round inputs alone
    want, _, passes, _ = expected_log([P], [g["accept_steps"]], *args, case["K"], case["DK"], True)
    assert slog == want and len(slog) > len(plog) and g["n_target_passes"] == passes[0] == len(slog)
    assert packed[0]["n_target_passes"] == packed[0]["n_target_forwards"]
    release_decoders(tgt, drf)


def test_mixed_batch_forwards_exactly_the_pending_users_blocks(mix):
    r = mix
    k, dk, (gamma, new) = r["case"]["K"], r["case"]["DK"], r["args"]
    acc = [o["accept_steps"] for o in r["packed"]]
    assert acc == MIX_ORACLE                                              # the engine's fp32 decisions are the CPU oracle's
    lens = [len(r["prompts"][u]) for u in MIX_USERS]
    _, _, _, dls = expected_log(lens, acc, gamma, new, k, dk, True)
    first = [(a[0], d[0]) for a, d in zip(acc, dls)]
    assert sum(1 for a, d in first if a == 0) >= 2 and sum(1 for a, d in first if 0 < a < d) >= 2       # stop at step 0 / mid-walk
    assert sum(1 for a, d in zip(acc, dls) if any(x == y > 0 for x, y in zip(a, d))) >= 2                # a round that accepts every block
    for u, (a, b) in enumerate(zip(r["packed"], r["staged"])):
        assert_same_user(a, b, f"user {MIX_USERS[u]}")
    want_p, _, passes_p, _ = expected_log(lens, acc, gamma, new, k, dk, False)
    want_s, segs_s, passes_s, _ = expected_log(lens, acc, gamma, new, k, dk, True)
    print("packed log", r["plog"], "\nstaged log", r["slog"])
    assert r["plog"] == want_p and [o["n_target_passes"] for o in r["packed"]] == passes_p
    assert r["slog"] == want_s                                            # per phase exactly the still-pending users' block rows
    assert [o["n_target_passes"] for o in r["staged"]] == passes_s and sum(passes_s) == sum(segs_s)
    assert sum(t for t, _ in r["slog"]) < sum(t for t, _ in r["plog"])    # rejected blocks were never forwarded


def test_mixed_batch_forward_logs_are_the_round_rules(mix):
    """Every forward of the six users' call, both models, packed and forced staged, against the restatement of the round rule
    (tests/round_ref.py): the draft's steps are the same forwards in both runs (step 0: the round inputs, or dk + k rows after a round that
    accepted every block; step i: dk rows per user that drafts more than i blocks), and the packed target log holds, per round, every
    user's round inputs and draft blocks."""
    r = mix
    k, dk, (gamma, new) = r["case"]["K"], r["case"]["DK"], r["args"]
    lens = [len(r["prompts"][u]) for u in MIX_USERS]
    want_d, _ = expected_draft_log(lens, MIX_ORACLE, gamma, new, k, dk)
    want_p, _, _, _ = expected_log(lens, MIX_ORACLE, gamma, new, k, dk, False)
    print("draft log, packed call", r["pdlog"], "\ndraft log, staged call", r["sdlog"], "\nwant", want_d)
    assert r["pdlog"] == want_d and r["sdlog"] == want_d
    assert r["plog"] == want_p


@pytest.mark.parametrize("name,gamma,new,want_dl", [("k5_dk10_indep", 3, 4, [3, 2, 1, 0]), ("k20_dk40_new7_gamma2", 2, 7, [2, 2, 0])])
def test_last_rounds(name, gamma, new, want_dl):
    """gamma' = min(gamma, max_new_tokens - generated - 1) shrinks to 0 (the closing one_step) with an unrelated draft; with draft == target
    every block is accepted and the draft re-ingests its own last block (beamSD.py:402-416)."""
    case = _case(name)
    ci = build_case_inputs(case)
    tgt, drf = _models(case, ci)
    one = _inputs([ci["prompt"]])
    packed, plog = _logged(tgt, drf, one, gamma, new, ci["fn"], 0)
    staged, slog = _logged(tgt, drf, one, gamma, new, ci["fn"], 2)
    acc = packed[0]["accept_steps"]
    want, _, passes, dls = expected_log([len(ci["prompt"])], [acc], gamma, new, case["K"], case["DK"], True)
    assert dls[0] == want_dl, (acc, dls)
    if name == "k20_dk40_new7_gamma2":
        assert acc == [2, 2]                                              # fully accepted rounds
    assert_same_user(packed[0], staged[0], name)
    assert slog == want and staged[0]["n_target_passes"] == passes[0]
    release_decoders(tgt, drf)


def test_unread_slots_stay_unwritten(mix):
    """One staged round of a user that stops at step 0: the KV slots of its draft blocks still hold the sentinel (the packed round writes
    them).  Slots [0, P) are the prompt's, [P, P + gamma' x DK) the draft blocks'."""
    r = mix
    lib, u = _lib.load(), MIX_USERS[0]
    assert MIX_ORACLE[0][0] == 0
    P, dk, (gamma, new) = len(r["prompts"][u]), r["case"]["DK"], r["args"]
    dims = r["ci"]["target_dims"]
    written = {}
    for mode in (2, 0):
        with _lib.switches(verify_staged=mode), BSSDSession(r["tgt"], r["drf"], 1, gamma, new, prefix_allowed_tokens_fn=r["ci"]["fn"]) as ses:
            ses.submit(r["inputs"][u])
            dec = ses._decs[0].handle
            nbytes = int(lib.atspeed_decoder_kv_bytes(dec, 0))
            assert nbytes == dims.n_layers * KW["max_slots"] * dims.hidden * 4
            sentinel = torch.full((nbytes // 4,), -12345.0, dtype=torch.float32, device="cuda")
            kbuf, vbuf = torch.empty_like(sentinel), torch.empty_like(sentinel)
            st = _lib.stream_ptr(sentinel.device)
            _lib.check(lib.atspeed_decoder_kv_copy(dec, 0, 1, sentinel.data_ptr(), sentinel.data_ptr(), st))
            assert ses.step() == [] and ses.counters()["rounds"] == 1
            _lib.check(lib.atspeed_decoder_kv_copy(dec, 0, 0, kbuf.data_ptr(), vbuf.data_ptr(), st))
            torch.cuda.synchronize()
            c = ses.counters()
        rows = [(b.view(dims.n_layers, KW["max_slots"], dims.hidden) != -12345.0).any(dim=2).all(dim=0).cpu().numpy() for b in (kbuf, vbuf)]
        assert (rows[0] == rows[1]).all()
        written[mode] = np.flatnonzero(rows[0]).tolist()
        assert c["target_forwards"] == 1 and c["target_passes"] == 1      # stopped at step 0: phase 0 was the round's only pass
    assert written[2] == list(range(P))                                   # the prompt's slots and nothing else
    assert written[0] == list(range(P + gamma * dk))                      # the packed round wrote every draft block


def test_session_with_staging(mix):
    """Four lanes with refill, every round staged: each user equals its single call (which is never staged), nothing is allocated after create."""
    r = mix
    users = list(range(12))
    single = [BSSD(r["tgt"], r["drf"], r["inputs"][u], *r["args"], prefix_allowed_tokens_fn=r["ci"]["fn"]) for u in users]
    with _lib.switches(verify_staged=2):
        ses = BSSD_batch(r["tgt"], r["drf"], [r["inputs"][u] for u in users], *r["args"], prefix_allowed_tokens_fn=r["ci"]["fn"], lanes=4)
    for u, (a, b) in enumerate(zip(single, ses)):
        assert_same_user(a, b, f"user {u}")
        assert b["status"] == 0 and b["n_target_passes"] >= b["n_target_forwards"] == a["n_target_passes"]
    c = ses[0]["session_counters"]
    print("session counters", c)
    assert c["allocs_after_create"] == 0 and c["users_retired"] == len(users)
    assert c["target_passes"] > c["target_forwards"] and c["target_forwards"] <= c["rounds"]
    assert len({o["lane"] for o in ses}) == 4 and max(o["rounds_queued"] for o in ses) > 0            # lanes were refilled


def test_sampling_ignores_the_switch(mix):
    r = mix
    six = [r["inputs"][u] for u in MIX_USERS]
    for m in (r["tgt"], r["drf"]):
        m.generation_config.do_sample, m.generation_config.temperature = True, 1.0
    try:
        a, alog = _logged(r["tgt"], r["drf"], six, *r["args"], r["ci"]["fn"], 0, seed=100)
        b, blog = _logged(r["tgt"], r["drf"], six, *r["args"], r["ci"]["fn"], 2, seed=100)
    finally:
        for m in (r["tgt"], r["drf"]):
            m.generation_config.do_sample = False
    assert alog == blog
    for x, y in zip(a, b):
        assert torch.equal(x["beam_sequence"], y["beam_sequence"]) and torch.equal(x["beam_scores"], y["beam_scores"])      # bit for bit
        assert (x["n_run"], x["accept_steps"], x["n_target_passes"]) == (y["n_run"], y["accept_steps"], y["n_target_passes"])


def test_auto_threshold(mix):
    """Switch 1 (the default) stages a round only when its packed forward would exceed T* tokens.  The rule's second condition (enough rows
    expected to be skipped, test_auto_follows_the_accepted_steps) is taken out here with `verify_staged_pass_tokens` 0."""
    only_t_star = dict(verify_staged_pass_tokens=0)
    r = mix
    v = C.c_int32(-1)
    _lib.check(_lib.load().atspeed_get_switch(b"verify_staged", C.byref(v)))
    t_star = _threshold()
    k, dk, (gamma, new) = r["case"]["K"], r["case"]["DK"], r["args"]
    assert v.value == 1 and t_star > 0
    # under T*: the six users' first round packs sum(P) + 6 x gamma x DK tokens
    lens = [len(r["prompts"][u]) for u in MIX_USERS]
    assert sum(lens) + len(lens) * gamma * dk <= t_star
    outs, log = _logged(r["tgt"], r["drf"], [r["inputs"][u] for u in MIX_USERS], *r["args"], r["ci"]["fn"], 1, only_t_star)
    assert log == r["plog"]
    # over T* in the first round only: so many users that sum(P) + n x gamma x DK > T*; later rounds (K + gamma' x DK tokens per user) that
    # fall under T* run packed again
    per_user = 18 + gamma * dk
    n = t_star // per_user + 2
    assert n <= 256, f"T* = {t_star} cannot be passed by one lock-step batch of these users"
    many = [r["inputs"][u % 24] for u in range(n)]
    lens = [len(r["prompts"][u % 24]) for u in range(n)]
    packed, plog = _logged(r["tgt"], r["drf"], many, *r["args"], r["ci"]["fn"], 0)
    auto, alog = _logged(r["tgt"], r["drf"], many, *r["args"], r["ci"]["fn"], 1, only_t_star)
    assert plog[0][0] > t_star
    assert alog[0] == (sum(lens), n) and alog[0] != plog[0]               # round 1 begins with phase 0: the prompts alone, one logit row each
    acc = [o["accept_steps"] for o in packed]
    want_p, _, _, _ = expected_log(lens, acc, gamma, new, k, dk, False)
    want, _, passes, _ = expected_log(lens, acc, gamma, new, k, dk, True, t_star)
    assert plog == want_p and alog == want and [o["n_target_passes"] for o in auto] == passes
    for a, b in zip(packed, auto):
        assert_same_user(a, b)


@pytest.mark.parametrize("name,gamma,new", [("k5_dk10_indep", 3, 4), ("k20_dk40_new7_gamma2", 2, 7)])
def test_auto_follows_the_accepted_steps(name, gamma, new):
    """Above T* (set to 0 here) the default rule stages a round when the target's recent walks say that rows will be skipped: a target that has
    decoded nothing yet is staged; after rounds that rejected at step 0 every round is (no phase is added, every draft block is skipped); after
    rounds that accepted every block none is (nothing to skip, each phase would cost a pass over the weights)."""
    case = _case(name)
    ci = build_case_inputs(case)
    tgt, drf = _models(case, ci)
    one = _inputs([ci["prompt"]])
    P, args = len(ci["prompt"]), (gamma, new, case["K"], case["DK"])
    above = dict(verify_staged_tokens=0)
    first, flog = _logged(tgt, drf, one, gamma, new, ci["fn"], 1, above)
    again, alog = _logged(tgt, drf, one, gamma, new, ci["fn"], 1, above)
    acc = first[0]["accept_steps"]
    want_s, _, _, dls = expected_log([P], [acc], *args, True)
    want_p, _, _, _ = expected_log([P], [acc], *args, False)
    assert flog[0] == (P, 1)                                              # no history: the first round opens with phase 0
    if name == "k5_dk10_indep":
        assert acc == [0, 0, 0] and flog == alog == want_s
    else:
        assert acc == [2, 2] and dls[0] == [2, 2, 0] and alog == want_p
        assert flog == want_s[:3] + want_p[1:]                            # round 1 in three phases, then packed: round 1 accepted everything
    assert_same_user(first[0], again[0], name)
    release_decoders(tgt, drf)
