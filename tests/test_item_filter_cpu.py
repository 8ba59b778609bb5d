"""Per-user item filters, the parts that need no GPU: the numpy restatement (tests/item_filter_ref.py) against a brute force over the
sequences of a nested-dict trie, the refusals of the Python layer and of the command line, the harness' history lists, and the oracle
under the test's filter closure against the golden recorded from the reference (tests/golden/gen_item_filter_golden.py)."""
import itertools
import json
import os

import numpy as np
import pytest

from atspeed_amd import beamSD, harness, inference
from atspeed_amd.generation_trie import PositionSetConstraint, SuffixTrieConstraint, Trie, WholeSentenceTrieConstraint
from tests import item_filter_ref as F

SEP = (13, 14)


def _random_trie(rng, depth=4, fan=(3, 2, 3, 2), drop=0.25):
    """item sequences of `depth` tokens (+ an EOS = 2 below each), some branches missing so that subtrees differ in size"""
    items = [q for q in itertools.product(*[range(100 * (d + 1), 100 * (d + 1) + fan[d]) for d in range(depth)]) if rng.random() > drop]
    return [list(q) + [2] for q in items]


def _brute_force(seqs, listed, mode):
    """the blocked PREFIXES by the definition read over sequences, with no automaton: (set of prefixes, unknown count, status)"""
    full = {tuple(q) for q in seqs}
    nodes = {q[:i] for q in full for i in range(len(q) + 1)}
    known = [tuple(q) for q in listed if tuple(q) in nodes]
    unknown = len(listed) - len(known)

    blocked = set()
    if mode == F.BLOCK:
        # an end node; or a node every root-to-leaf sequence through which meets an end node strictly below it
        for p in nodes:
            if p in known or all(any(len(q) > len(p) and leaf[:len(q)] == q for q in known) for leaf in full if leaf[:len(p)] == p):
                blocked.add(p)
        status = F.ERR_CONSTRAINT if () in blocked else 0
    else:
        def on_path(p):
            return any(q[:len(p)] == p for q in known)
        for p in nodes:
            if p and on_path(p[:-1]) and p[:-1] not in known and not on_path(p):
                blocked.add(p)
        status = F.ERR_CONSTRAINT if not known else 0
    return blocked, unknown, status


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("mode", [F.BLOCK, F.ALLOW])
def test_restatement_equals_brute_force(seed, mode):
    rng = np.random.default_rng(seed)
    seqs = _random_trie(rng)
    row_ptr, tok, nxt, prefixes = F.csr_from_sequences(seqs)
    items = [q[:-1] for q in seqs]
    picks = [items[i] for i in rng.choice(len(items), size=max(1, len(items) // (2 if seed % 2 else 4)), replace=False)]
    listed = [list(q) for q in picks]
    listed += [list(items[0]) + [2]]                                   # with the EOS
    listed += [list(items[1][:2])]                                     # ends at an interior node
    listed += [list(items[2][:1]), list(items[2])]                     # a prefix of another listed sequence
    listed += [[999], list(items[0][:2]) + [998]]                      # unknown: no edge at the start node / deeper
    if seed == 5 and mode == F.BLOCK:
        listed = [list(q) for q in items]                              # everything: the closure reaches the start node
    words, unknown, status = F.node_mask(row_ptr, tok, nxt, 0, listed, mode)
    want, want_unknown, want_status = _brute_force(seqs, listed, mode)
    got = {prefixes[n] for n in range(len(prefixes)) if F.is_blocked(words, n)}
    assert got == want
    assert (unknown, status) == (want_unknown, want_status)
    assert len(words) == F.n_words(len(prefixes)) and int(words[-1]) >> (len(prefixes) & 31 or 32) == 0      # no bit at or above n_nodes
    if seed == 5 and mode == F.BLOCK:
        assert status == F.ERR_CONSTRAINT and F.is_blocked(words, 0)


def test_restatement_edge_cases():
    row_ptr, tok, nxt, prefixes = F.csr_from_sequences([[5, 6, 2], [5, 7, 2], [8, 9, 2]])
    w, unk, st = F.node_mask(row_ptr, tok, nxt, 0, [], F.BLOCK)
    assert not w.any() and (unk, st) == (0, 0)                          # block mode, no sequences: all bits 0
    w, unk, st = F.node_mask(row_ptr, tok, nxt, 0, [[77]], F.ALLOW)
    assert not w.any() and (unk, st) == (1, F.ERR_CONSTRAINT)           # allow mode, nothing known
    for bad in ([[]], [[5] * (F.MAX_NEW_TOKENS + 1)]):
        with pytest.raises(ValueError):
            F.node_mask(row_ptr, tok, nxt, 0, bad, F.BLOCK)
    # both items under 5 blocked: the closure blocks node (5,), not the start node
    w, _, st = F.node_mask(row_ptr, tok, nxt, 0, [[5, 6], [5, 7]], F.BLOCK)
    assert {prefixes[n] for n in range(len(prefixes)) if F.is_blocked(w, n)} == {(5,), (5, 6), (5, 7)} and st == 0
    # another start node: the same sequences are walked from there
    n5 = prefixes.index((5,))
    w, unk, _ = F.node_mask(row_ptr, tok, nxt, n5, [[6], [5, 6]], F.BLOCK)
    assert {prefixes[n] for n in range(len(prefixes)) if F.is_blocked(w, n)} == {(5, 6)} and unk == 1
    # allow: the end node wins over a longer sequence through it -- its own children stay free
    w, _, _ = F.node_mask(row_ptr, tok, nxt, 0, [[5], [5, 6, 2]], F.ALLOW)
    assert {prefixes[n] for n in range(len(prefixes)) if F.is_blocked(w, n)} == {(8,)}


def test_filter_closure_is_the_restatement():
    """the closure the golden generator wraps around the reference's mask = a walk of the automaton minus the blocked edges"""
    rng = np.random.default_rng(11)
    seqs = _random_trie(rng)
    trie = Trie([[1] + q for q in seqs])
    fn = SuffixTrieConstraint(trie, SEP, 1)
    fsm = fn.compile([3, 4, 13, 14])
    items = [q[:-1] for q in seqs]
    for mode, listed in ((F.BLOCK, [items[0], items[3], items[4][:3]] + [q for q in items if q[0] == items[-1][0]]),
                         (F.ALLOW, [items[0], items[5], items[7][:2]])):
        words, _, _ = F.node_mask(fsm.row_ptr, fsm.tok, fsm.nxt, fsm.start, listed, mode)
        wrapped = F.closure(fn, SEP, **({"exclude": listed} if mode == F.BLOCK else {"allow": listed}))
        todo, seen = [()], 0
        while todo:
            gen = todo.pop()
            node = fsm.walk(fsm.start, gen)
            want = [int(t) for t, c in zip(fsm.allowed(node), fsm.nxt[fsm.row_ptr[node]: fsm.row_ptr[node + 1]]) if not F.is_blocked(words, int(c))]
            assert sorted(wrapped(0, [3, 4, 13, 14] + list(gen))) == want, (mode, gen)
            todo += [gen + (t,) for t in want]
            seen += 1
        assert seen > 10


class _Model:
    """enough of a HipLlama for the argument checks that come before any device work"""


def _fake_models(monkeypatch):
    monkeypatch.setattr(beamSD, "_mode", lambda seed, *models: (False, 1.0, 0, 0, 1.0))
    return _Model(), _Model()


def test_loader_refusals(monkeypatch):
    tgt, drf = _fake_models(monkeypatch)
    inputs = {"input_ids": None}
    trie = Trie([[1, 5, 6, 2]])
    with pytest.raises(ValueError, match="mutually exclusive"):
        beamSD.BSSD(tgt, drf, inputs, 2, 4, prefix_allowed_tokens_fn=SuffixTrieConstraint(trie, SEP), exclude_items=[[5]], allow_items=[[5]])
    with pytest.raises(ValueError, match="mutually exclusive"):
        beamSD.target_generate_batch(tgt, [inputs, inputs], 4, prefix_allowed_tokens_fn=SuffixTrieConstraint(trie, SEP),
                                     exclude_items=[[[5]], None], allow_items=[[[5]], None])
    with pytest.raises(ValueError, match="per user"):
        beamSD.BSSD_batch(tgt, drf, [inputs, inputs], 2, 4, prefix_allowed_tokens_fn=SuffixTrieConstraint(trie, SEP), exclude_items=[[[5]]])
    # the host path: a closure, or an extra logits processor
    with pytest.raises(NotImplementedError):
        beamSD.BSSD(tgt, drf, inputs, 2, 4, prefix_allowed_tokens_fn=lambda b, s: [5], exclude_items=[[5]])
    with pytest.raises(NotImplementedError):
        beamSD.target_generate(tgt, inputs, 4, logits_processor=[lambda i, s: s], prefix_allowed_tokens_fn=SuffixTrieConstraint(trie, SEP),
                               allow_items=[[5]])


@pytest.mark.parametrize("fn", [PositionSetConstraint({0: [5], 1: [2]}, SEP), None, "chained"])
def test_wrong_constraint_type_is_refused(fn):
    if fn == "chained":
        a = Trie([[1, 5, 0]])
        a.append(Trie([[6, 2]]), 0)
        fn = WholeSentenceTrieConstraint(a)
    with pytest.raises(ValueError, match="exclude_items / allow_items need"):
        beamSD._check_filter_constraint(fn, "BSSD")
    beamSD._check_filter_constraint(SuffixTrieConstraint(Trie([[1, 5, 2]]), SEP), "BSSD")
    beamSD._check_filter_constraint(WholeSentenceTrieConstraint(Trie([[1, 5, 2]])), "BSSD")


def test_filter_specs():
    S = beamSD._filter_specs
    assert S(1, None, None, False, "x") is None
    assert S(3, [None, None, None], None, True, "x") is None
    assert S(1, [(5, 6)], None, False, "x") == [(0, [[5, 6]])]
    assert S(1, [], None, False, "x") == [(0, [])]                       # an empty block list is a filter (with all bits 0), None is none
    assert S(2, [[[5]], None], [None, [[6]]], True, "x") == [(0, [[5]]), (1, [[6]])]


def test_parse_refuses_exclude_history_without_strict_trie(capsys):
    with pytest.raises(SystemExit):
        inference.parse(["--data_path", "x", "--exclude_history"])
    assert "--strict_trie" in capsys.readouterr().err
    assert inference.parse(["--data_path", "x", "--exclude_history", "--strict_trie"]).exclude_history
    assert not inference.parse(["--data_path", "x"]).exclude_history


def test_test_user_keeps_the_uncut_history():
    ix = harness.ItemIndex({str(i): [f"<a_{i % 3}>", f"<b_{i}>"] for i in range(8)})
    data = harness.SeqRecTestData(ix, {0: [0, 1, 2, 3, 4]}, {0: [5]}, {0: [6]}, max_his_len=2)
    u = data.users[0]
    assert u.history == [4, 5] and u.full_history == [0, 1, 2, 3, 4, 5] and u.labels == [6]
    assert harness.TestUser(1, [2], [3]).full_history == []              # the field is defaulted


# ---------------------------------------------------------------------------------------------- the golden: the reference under the closure
def _filter_golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "item_filter_golden.json")) as f:
        return {c["name"]: c for c in json.load(f)}


def test_golden_holds_the_six_cases_above_the_margin():
    from tests.golden import item_filter_cases as IC
    gold = _filter_golden()
    assert sorted(gold) == sorted(IC.case_id(b, k) for b, k in IC.all_cases())
    for c in gold.values():
        assert c["min_margin"] > IC.MIN_MARGIN and c["bssd_tokens"] == c["tg_tokens"]            # decided above fp32 noise, and lossless
        if c["kind"] == "allow_pick":
            assert c["seed"] == IC.ALLOW_SEED[c["base"]]


@pytest.mark.parametrize("base", ["k8_dk16_trie", "k20_dk40_trie"])
def test_oracle_under_the_closure_equals_the_reference_under_it(base, bssd_golden):
    """oracle.BSSD / target_generate with the test's closure against what the REAL reference gave with it: ids, n_matches, step_len and
    draft ids exact, scores within 1e-3"""
    from atspeed_amd import synth
    from oracle import beamsd_ref as R
    from oracle.llama_ref import RefLlama
    from tests.golden import item_filter_cases as IC
    gold = _filter_golden()
    case = IC.base_case(base)
    ci = IC.build_case_inputs(case)
    rt, rd = RefLlama(ci["target_dims"], ci["target_sd"]), RefLlama(ci["draft_dims"], ci["draft_sd"])
    P = len(ci["prompt"])
    plain = bssd_golden[base]["tg_tokens"]
    for kind in IC.KINDS:
        g = gold[IC.case_id(base, kind)]
        lists = IC.filter_lists(base, kind, ci["items"], plain)
        fn = F.closure(ci["fn"], synth.RESPONSE_SEP, **lists)
        tg = R.target_generate(rt, ci["prompt"], case["max_new_tokens"], case["K"], fn)
        assert tg["beam_sequence"][:, P:].tolist() == g["tg_tokens"]
        np.testing.assert_allclose(tg["beam_scores"].numpy(), g["tg_scores"], atol=1e-3, rtol=0)
        out = R.BSSD(rt, rd, ci["prompt"], case["gamma"], case["max_new_tokens"], case["K"], case["DK"], fn)
        assert out["beam_sequence"][:, P:].tolist() == g["bssd_tokens"]
        np.testing.assert_allclose(out["beam_scores"].numpy(), g["bssd_scores"], atol=1e-3, rtol=0)
        assert [r["n_matches"] for r in out["rounds"]] == [r["n_matches"] for r in g["rounds"]]
        assert [r["step_len"] for r in out["rounds"]] == [r["step_len"] for r in g["rounds"]]
        assert [r["draft_ids"] for r in out["rounds"]] == [r["draft_ids"] for r in g["rounds"]]
        # what the filter must do to the list
        assert g["tg_tokens"] != plain
        if kind == "block_top3":
            assert lists["exclude"] == plain[:3] and not any(row in plain[:3] for row in g["tg_tokens"])
        elif kind == "block_first_code":
            assert len(lists["exclude"]) > 1 and not any(row[0] == plain[0][0] for row in g["tg_tokens"])
        else:
            assert len(lists["allow"]) == 2 * case["DK"] + 5 and all(row in lists["allow"] for row in g["tg_tokens"])
