"""All per-user options in ONE call (item filter, resident adapter, prompt prefix; beamSD.py "per-user options") on the GPU: six users of the
fp32 golden trie case, each with its own mix of the three, through every entry point that takes them -- the lock-step batch, a session of
two lanes, the beam path, and the chunked form of both batch calls -- against the user's own one-user call with its adapter and filter and
WITHOUT its prefix.  Each option alone is pinned to the oracle by test_item_filter_gpu.py, test_lora_multi_gpu.py and test_prefix_gpu.py;
here: no option is dropped or handed to the wrong user when all travel together, and nothing stays on the cached decoders afterwards."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import beamSD, lora as L, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, BSSDSession, release_decoders, target_generate, target_generate_batch
from atspeed_amd.model import HipLlama, PromptPrefix
from tests.golden.cases import CASES, build_case_inputs

SCORE_TOL = 1e-3                                   # tests/test_prefix_gpu.py: a prefix against the full prefill
KW = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
N = 6
ADAPTERS = ["a", None, "a", "b", None, None]
OPENING = ["a", "b", "a", None, "b", None]         # which 8-token opening the prompt starts with
NAMES_PREFIX = [True, True, True, False, False, False]     # user 4 opens with head_b and does not name the prefix


def _adapter(dims, seed):
    return L.from_tensors(synth.synthetic_lora(dims, seed, r=8, modules=("q", "v"), std=0.1), dims.n_layers, dims.hidden, 8, 16)


def _gen(out, P):
    return out["beam_sequence"][:, P:].cpu().tolist()


def build_world():
    """models, users, their options as every entry point takes them, and the one-user calls everything is compared with"""
    case =[c for c in CASES if c["name"] == "k20_dk40_trie"][0]
    ci = build_case_inputs(case)
    fn, a = ci["fn"], (case["gamma"], case["max_new_tokens"])
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **KW)
    tgt.add_lora(_adapter(ci["target_dims"], 77), "a").add_lora(_adapter(ci["target_dims"], 78), "b")
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **KW)
    heads = {"a": synth.synthetic_prompt(12, 4001)[:8], "b": synth.synthetic_prompt(12, 4002)[:8]}
    tails = [synth.synthetic_prompt(14 + 5 * u, 4100 + u)[1:] for u in range(N)]          # without their BOS; they end with the Response separator
    prompts = [np.concatenate((heads[o], t)) if o else np.concatenate(([synth.BOS_ID], t)) for o, t in zip(OPENING, tails)]
    inputs = [{"input_ids": torch.from_numpy(p.astype(np.int64))[None].cuda()} for p in prompts]
    P = [len(p) for p in prompts]
    items = [[int(t) for t in it] for it in ci["items"]]
    # the plain calls (nothing named), then each user under its adapter alone: the filters are made from those
    plain = [BSSD(tgt, drf, inp, *a, prefix_allowed_tokens_fn=fn) for inp in inputs]
    adapted = [BSSD(tgt, drf, inp, *a, prefix_allowed_tokens_fn=fn, adapter=ad) for inp, ad in zip(inputs, ADAPTERS)]
    uniq = sorted({tuple(it) for it in items})
    pick = np.random.default_rng(7).choice(len(uniq), size=2 * case["DK"] + 5, replace=False)
    exclude = [_gen(adapted[0], P[0])[:3], None, None, _gen(adapted[3], P[3])[:3], None, None]
    allow = [None, [list(uniq[i]) for i in sorted(pick)], None, None, None, None]
    one = [dict(adapter=ADAPTERS[u], exclude_items=exclude[u], allow_items=allow[u]) for u in range(N)]
    single = [BSSD(tgt, drf, inputs[u], *a, prefix_allowed_tokens_fn=fn, **one[u]) for u in range(N)]
    single_tg = [target_generate(tgt, inputs[u], a[1], prefix_allowed_tokens_fn=fn, **one[u]) for u in range(N)]
    pa, pb = PromptPrefix(tgt, drf, heads["a"], adapter="a"), PromptPrefix(tgt, drf, heads["b"])
    prefixes = [(pa if o == "a" else pb) if named else None for o, named in zip(OPENING, NAMES_PREFIX)]
    return dict(case=case, fn=fn, a=a, tgt=tgt, drf=drf, inputs=inputs, P=P, items=items, plain=plain, adapted=adapted, single=single,
                single_tg=single_tg, pa=pa, pb=pb, prefixes=prefixes, exclude=exclude, allow=allow,
                dl=min(case["gamma"], case["max_new_tokens"] - 1),
                suffix=[p - (8 if pre is not None else 0) for p, pre in zip(P, prefixes)])


@pytest.fixture(scope="module")
def world():
    w = build_world()
    yield w
    release_decoders(w["tgt"], w["drf"])


def _batch_kw(w, exclude=None):
    return dict(prefix_allowed_tokens_fn=w["fn"], exclude_items=exclude or w["exclude"], allow_items=w["allow"], adapters=ADAPTERS,
                prefixes=w["prefixes"])


def _same(what, single, outs, bssd=True):
    for u, (s, o) in enumerate(zip(single, outs)):
        assert torch.equal(s["beam_sequence"], o["beam_sequence"]), (what, u)
        np.testing.assert_allclose(s["beam_scores"].cpu().numpy(), o["beam_scores"].cpu().numpy(), atol=SCORE_TOL, rtol=0, err_msg=f"{what} user {u}")
        if bssd:
            assert (s["n_run"], s["total_accept_steps"], s["accept_steps"]) == (o["n_run"], o["total_accept_steps"], o["accept_steps"]), (what, u)


def _served(w):
    return w["pa"].info()["users_served"], w["pb"].info()["users_served"], w["pa"].info(True)["users_served"], w["pb"].info(True)["users_served"]


def _nothing_kept(w, what):
    """a plain batch of the same users on the same cached decoders: the plain single calls, every whole prompt prefilled"""
    w["tgt"].forward_log(1)
    outs = BSSD_batch(w["tgt"], w["drf"], w["inputs"], *w["a"], prefix_allowed_tokens_fn=w["fn"])
    first = w["tgt"].forward_log(0)[0][0]
    assert first == sum(w["P"]) + N * w["dl"] * w["case"]["DK"], (what, first)
    _same(f"plain batch after {what}", w["plain"], outs)


def test_the_reference_calls_show_every_option(world):
    """a run that drops an option cannot equal these: the filters move users 0, 1 and 3, the adapter moves users 0 and 2"""
    w = world
    for u in (0, 1, 3):
        assert _gen(w["single"][u], w["P"][u]) != _gen(w["adapted"][u], w["P"][u]), u
    for u in (0, 3):
        assert not any(row in w["exclude"][u] for row in _gen(w["single"][u], w["P"][u])), u
    assert all(row in w["allow"][1] for row in _gen(w["single"][1], w["P"][1])[:w["single"][1]["n_valid"]])
    for u in (0, 2):
        assert _gen(w["adapted"][u], w["P"][u]) != _gen(w["plain"][u], w["P"][u]), u
    for u in (4, 5):
        assert torch.equal(w["single"][u]["beam_sequence"], w["plain"][u]["beam_sequence"])
    _same("BSSD against target_generate", w["single_tg"], w["single"], bssd=False)      # lossless under every mix


def _session(w):
    with BSSDSession(w["tgt"], w["drf"], 2, *w["a"], prefix_allowed_tokens_fn=w["fn"]) as s:
        sub = lambda u: s.submit(w["inputs"][u], exclude_items=w["exclude"][u], allow_items=w["allow"][u], adapter=ADAPTERS[u], prefix=w["prefixes"][u])
        tickets = [sub(u) for u in range(3)]
        done = s.step()
        tickets += [sub(u) for u in range(3, N)]
        done += s.drain()
        got = dict(done)
        assert all(got[t]["status"] == 0 for t in tickets)
        c = s.counters()
        assert c["allocs_after_create"] == 0 and c["users_retired"] == N, c
    return [got[t] for t in tickets]


PATHS =["lock_step", "lanes2", "session", "beam", "lock_step_chunked", "beam_chunked"]


@pytest.mark.parametrize("path", PATHS)
def test_six_users_with_their_own_mix_of_options(world, path, monkeypatch):
    w = world
    tgt, drf, a = w["tgt"], w["drf"], w["a"]
    bssd = not path.startswith("beam")
    if path.endswith("chunked"):
        monkeypatch.setattr(beamSD, "MAX_USERS_PER_CALL", 4)                         # two chunks: every per-user list is sliced
    before = _served(w)
    tgt.forward_log(1)
    if path in ("lock_step", "lock_step_chunked"):
        outs = BSSD_batch(tgt, drf, w["inputs"], *a, **_batch_kw(w))
    elif path == "lanes2":
        outs = BSSD_batch(tgt, drf, w["inputs"], *a, lanes=2, **_batch_kw(w))
        c = outs[0]["session_counters"]
        assert c["allocs_after_create"] == 0 and c["users_retired"] == N, c
    elif path == "session":
        outs = _session(w)
    else:
        outs = target_generate_batch(tgt, w["inputs"], a[1], **_batch_kw(w))
    log = tgt.forward_log(0)
    monkeypatch.undo()
    _same(path, w["single"] if bssd else w["single_tg"], outs, bssd=bssd)
    assert all(o["status"] == 0 for o in outs)
    # the first target forward holds the suffix rows alone (and, packed with them, the draft blocks of a beam-SD round)
    n_first = {"lock_step": N, "beam": N, "lock_step_chunked": 4, "beam_chunked": 4}.get(path)
    if n_first is not None:
        assert log[0][0] == sum(w["suffix"][:n_first]) + (n_first * w["dl"] * w["case"]["DK"] if bssd else 0), (path, log[:2])
    after = _served(w)
    assert tuple(x - y for x, y in zip(after, before)) == ((2, 1, 2, 1) if bssd else (2, 1, 0, 0)), (path, before, after)
    _nothing_kept(w, path)


def test_a_call_that_raises_during_set_up_leaves_nothing_behind(world):
    """user 3 excludes every item: refused before anything is launched, with adapters and prefixes of the other users already checked"""
    w = world
    w["tgt"].forward_log(1), w["drf"].forward_log(1)
    exclude = list(w["exclude"])
    exclude[3] = w["items"]
    with pytest.raises(ValueError, match="user 3"):
        BSSD_batch(w["tgt"], w["drf"], w["inputs"], *w["a"], **_batch_kw(w, exclude))
    assert w["tgt"].forward_log(0) == [] and w["drf"].forward_log(0) == [], "a refused call launched a forward"
    _nothing_kept(w, "a call that raised")


def test_a_chunked_call_whose_second_chunk_raises_leaves_nothing_behind(world, monkeypatch):
    """chunks of 4: users 0 .. 3 run, then user 5 (the second chunk's user 1, named by its place in the whole list) excludes every item"""
    w = world
    monkeypatch.setattr(beamSD, "MAX_USERS_PER_CALL", 4)
    exclude = list(w["exclude"])
    exclude[5] = w["items"]
    with pytest.raises(ValueError, match="user 5"):
        BSSD_batch(w["tgt"], w["drf"], w["inputs"], *w["a"], **_batch_kw(w, exclude))
    monkeypatch.undo()
    _nothing_kept(w, "a chunked call whose second chunk raised")
