"""Per-user item filters on the device (include/atspeed_hip.h "item filters"): the builder kernel against the numpy restatement bit for
bit, the step and cutoff kernels alone under a filter, and the engine -- BSSD, target_generate, batches, sessions, sampling, bf16 --
against the golden recorded from the reference under the same filter closure, against the oracle and against its own unfiltered and
one-user calls."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, BSSDSession, last_trace, target_generate, target_generate_batch
from atspeed_amd.model import HipLlama
from oracle import beamsd_ref as R
from oracle.llama_ref import RefLlama
from tests import item_filter_ref as F
from tests.golden import item_filter_cases as IC

SCORE_TOL = 1e-3
V = 6000


# ---------------------------------------------------------------------------------------------- library objects
class Automaton:
    def __init__(self, row_ptr, tok, nxt, vocab=V):
        self.row_ptr, self.tok, self.nxt = (np.ascontiguousarray(a, np.int32) for a in (row_ptr, tok, nxt))
        self.n_nodes = len(self.row_ptr) - 1
        tok_arg = self.tok if len(self.tok) else np.zeros(1, np.int32)
        nxt_arg = self.nxt if len(self.nxt) else np.zeros(1, np.int32)
        self.h = _lib.Handle.create("atspeed_fsm_destroy", _lib.load().atspeed_fsm_create, self.row_ptr.ctypes.data, tok_arg.ctypes.data,
                                    nxt_arg.ctypes.data, self.n_nodes, len(self.tok), vocab)

    @classmethod
    def of(cls, seqs, vocab=V):
        row_ptr, tok, nxt, prefixes = F.csr_from_sequences(seqs)
        a = cls(row_ptr, tok, nxt, vocab)
        a.prefixes = prefixes
        return a


def build_masks(a: Automaton, starts, lists, mode, expect=0):
    """one create call for len(starts) users -> (handle, words [users][W], unknown, status)"""
    lib = _lib.load()
    toks, soff, uoff = [], [0], [0]
    for seqs in lists:
        for q in seqs:
            toks += [int(t) for t in q]
            soff.append(len(toks))
        uoff.append(len(soff) - 1)
    a_tok = np.asarray(toks if toks else [0], np.int32)
    a_soff, a_uoff, a_start = np.asarray(soff, np.int32), np.asarray(uoff, np.int32), np.asarray(starts, np.int32)
    n = len(starts)
    unknown, status = np.full(n, -99, np.int32), np.full(n, -99, np.int32)
    h = _lib.Handle("atspeed_node_masks_destroy")
    rc = lib.atspeed_node_masks_create(a.h.ptr, n, a_start.ctypes.data, a_tok.ctypes.data, a_soff.ctypes.data, a_uoff.ctypes.data, mode,
                                       unknown.ctypes.data, status.ctypes.data, _lib.stream_ptr(torch.device("cuda", 0)), C.byref(h.ptr))
    assert rc == expect, (rc, lib.atspeed_last_error())
    if rc != 0:
        return None, None, None, None
    W = F.n_words(a.n_nodes)
    words = np.full((n, W), 0xDEADBEEF, np.uint32)
    for u in range(n):
        _lib.check(lib.atspeed_node_masks_read(h.ptr, u, words[u].ctypes.data, W))
    return h, words, unknown, status


def check_builder(a: Automaton, starts, lists, mode):
    h, words, unknown, status = build_masks(a, starts, lists, mode)
    for u, (st, seqs) in enumerate(zip(starts, lists)):
        w, unk, stat = F.node_mask(a.row_ptr, a.tok, a.nxt, st, seqs, mode)
        assert np.array_equal(words[u], w), (u, [n for n in range(a.n_nodes) if F.is_blocked(words[u], n) != F.is_blocked(w, n)][:20])
        assert (int(unknown[u]), int(status[u])) == (unk, stat), u
    return h, words, status


# ---------------------------------------------------------------------------------------------- 1. builder = restatement
@pytest.mark.parametrize("n", [31, 32, 33, 64, 65])
def test_builder_word_edges(n):
    """a root with n - 1 leaf children: the last node id sits below, at and above a word edge"""
    a = Automaton.of([[t] for t in range(n - 1)])
    assert a.n_nodes == n
    for keep in (0, n - 2):
        _, words, status = check_builder(a, [0], [[[t] for t in range(n - 1) if t != keep]], F.BLOCK)
        assert status[0] == 0 and sum(F.is_blocked(words[0], x) for x in range(n)) == n - 2
    _, words, status = check_builder(a, [0], [[[t] for t in range(n - 1)]], F.BLOCK)        # everything: the closure reaches the start node
    assert status[0] == _lib.ERR_CONSTRAINT and all(F.is_blocked(words[0], x) for x in range(n))
    assert int(words[0][-1]) >> ((n & 31) or 32) == 0                                       # bits at or above n_nodes are 0


def _trie_3222():
    return [[10 + a, 20 + b, 30 + c, 40 + d] for a, b, c, d in itertools.product(range(3), range(2), range(2), range(2))]


def test_builder_closure_levels():
    leaves = _trie_3222()
    a = Automaton.of(leaves)
    assert a.n_nodes == 46
    under = lambda *pre: [q for q in leaves if q[:len(pre)] == list(pre)]
    for listed, closed in ((under(10, 20, 30), (10, 20, 30)), (under(11, 21), (11, 21)), (under(12), (12,))):
        _, words, status = check_builder(a, [0], [listed], F.BLOCK)
        got = {a.prefixes[x] for x in range(46) if F.is_blocked(words[0], x)}
        want = {tuple(q[:i]) for q in listed for i in range(len(closed), 5)}
        assert got == want and closed in got and status[0] == 0
    _, words, status = check_builder(a, [0], [leaves], F.BLOCK)
    assert all(F.is_blocked(words[0], x) for x in range(46)) and status[0] == _lib.ERR_CONSTRAINT


def test_builder_many_sequences_shuffled_with_duplicates_and_unknowns():
    """a root with 1500 children (more than a workgroup has threads) of 2 leaves each; 3000 listed sequences"""
    leaves = [[c, 2000 + j] for c in range(1500) for j in range(2)]
    a = Automaton.of(leaves)
    rng = np.random.default_rng(3)
    listed = [leaves[i] for i in rng.integers(0, len(leaves), size=2993)]            # with replacement: duplicates, and pairs left half open
    listed += [[1500, 2000], [7, 2002], [5999], [3, 2000, 1], [1499, 1999], [0, 0], [2000]]
    listed = [listed[i] for i in rng.permutation(len(listed))]
    assert len(listed) == 3000 and len({tuple(q) for q in listed}) < 2993
    for mode in (F.BLOCK, F.ALLOW):
        _, words, status = check_builder(a, [0], [listed], mode)
        assert status[0] == 0
    closed = [c for c in range(1500) if [c, 2000] in listed and [c, 2001] in listed]
    _, words, _ = check_builder(a, [0], [listed], F.BLOCK)
    assert len(closed) > 100 and all(F.is_blocked(words[0], a.prefixes.index((c,))) for c in closed[:50])


def test_builder_users_start_nodes_interior_ends_prefixes_and_empty_lists():
    leaves = _trie_3222()
    a = Automaton.of(leaves)
    n11 = a.prefixes.index((11,))
    # two users with different start nodes, the second one's sequences relative to its node; a third user without sequences
    starts = [0, n11, 0]
    lists = [[[10, 20, 30, 40], [12, 21], [11, 20, 31, 41], [10, 99]],            # a leaf, an interior end node, a leaf, an unknown
             [[20, 30], [21, 31, 40], [21, 31, 41], [11, 20]],                    # interior, two leaves that close (21, 31); unknown from here
             []]
    _, words, status = check_builder(a, starts, lists, F.BLOCK)
    assert not words[2].any() and status[2] == 0                                  # block mode, no sequences: all bits 0
    assert F.is_blocked(words[1], a.prefixes.index((11, 21, 31))) and not F.is_blocked(words[0], a.prefixes.index((11, 21, 31)))
    # allow mode: interior end nodes, and a sequence that is a prefix of another -- the end node wins: its children stay free
    lists = [[[10, 20], [10, 20, 30, 41], [12, 21, 31, 40]], [[20], [21, 30, 40]]]
    _, words, status = check_builder(a, [0, n11], lists, F.ALLOW)
    assert not F.is_blocked(words[0], a.prefixes.index((10, 20, 31))) and F.is_blocked(words[0], a.prefixes.index((10, 21)))
    assert F.is_blocked(words[0], a.prefixes.index((11,))) and F.is_blocked(words[0], a.prefixes.index((10, 20, 30, 40)))
    # allow mode with nothing known
    _, words, status = check_builder(a, [0], [[[99], [10, 98]]], F.ALLOW)
    assert status[0] == _lib.ERR_CONSTRAINT and not words[0].any()


def test_builder_refuses_bad_sequences():
    a = Automaton.of(_trie_3222())
    build_masks(a, [0], [[[]]], F.BLOCK, expect=_lib.ERR_INVALID)
    build_masks(a, [0], [[[10] * (_lib.MAX_NEW_TOKENS + 1)]], F.BLOCK, expect=_lib.ERR_INVALID)
    build_masks(a, [46], [[[10]]], F.BLOCK, expect=_lib.ERR_INVALID)
    build_masks(a, [0], [[[10]]], 2, expect=_lib.ERR_INVALID)


@pytest.fixture(scope="module")
def fixture_trie():
    case = IC.base_case("k8_dk16_trie")
    ci = IC.build_case_inputs(case)
    fsm = ci["fn"].compile([int(t) for t in ci["prompt"]])
    return case, ci, fsm


def test_builder_on_the_fixture_trie_both_modes_twice(fixture_trie):
    case, ci, fsm = fixture_trie
    a = Automaton(fsm.row_ptr, fsm.tok, fsm.nxt, ci["target_dims"].vocab_size)
    items = [[int(t) for t in it] for it in ci["items"]]
    first = items[0][0]
    listed = items[5:60] + [it for it in items if it[0] == first] + [it + [synth.EOS_ID] for it in items[100:110]] + [[31999]]
    for mode in (F.BLOCK, F.ALLOW):
        _, w1, s1 = check_builder(a, [fsm.start], [listed], mode)
        _, w2, s2 = check_builder(a, [fsm.start], [listed[::-1]], mode)              # the bits are a function of the set, not of the order
        assert np.array_equal(w1, w2) and s1[0] == s2[0] == 0 and w1.any()


# ---------------------------------------------------------------------------------------------- 2. the step kernel alone
def _two_level(n_mid=4, n_leaf=6):
    return [[100 + m, 1000 + 10 * m + j] for m in range(n_mid) for j in range(n_leaf)]


def _expand_masked(a: Automaton, masks, user, logits: np.ndarray, bscore, nodes, k):
    lib = _lib.load()
    n = len(nodes)
    dev = torch.device("cuda", 0)
    lg = torch.from_numpy(logits).to(dev).contiguous()
    lse = torch.empty(n, dtype=torch.float32, device=dev)
    bs = torch.tensor(bscore, dtype=torch.float32, device=dev)
    nd = torch.tensor(nodes, dtype=torch.int32, device=dev)
    o_s = torch.full((64,), float("nan"), dtype=torch.float32, device=dev)
    o_p, o_t, o_n, o_f = (torch.full((64,), -7, dtype=torch.int32, device=dev) for _ in range(4))
    st = _lib.stream_ptr(dev)
    _lib.check(lib.atspeed_lse_rows(lg.data_ptr(), n, V, V, lse.data_ptr(), st))
    _lib.check(lib.atspeed_beam_expand_prune_masked(lg.data_ptr(), V, lse.data_ptr(), bs.data_ptr(), nd.data_ptr(), n, a.h.ptr, k, o_s.data_ptr(),
                                                    o_p.data_ptr(), o_t.data_ptr(), o_n.data_ptr(), o_f.data_ptr(), masks.ptr if masks else None,
                                                    user, st))
    torch.cuda.synchronize()
    return lse.cpu().numpy(), o_s.cpu().numpy()[:k], o_p.cpu().numpy()[:k], o_t.cpu().numpy()[:k], o_n.cpu().numpy()[:k], o_f.cpu().numpy()[:k]


def _expand_ref(a: Automaton, words, logits, lse, bscore, nodes, k):
    """numpy top-k over the unblocked candidates by (score desc, flat id asc); the score expression is the kernel's, in fp32"""
    cand = []
    for r, nd in enumerate(nodes):
        if not bscore[r] > -np.inf:
            continue
        for e in range(a.row_ptr[nd], a.row_ptr[nd + 1]):
            if words is not None and F.is_blocked(words, int(a.nxt[e])):
                continue
            t = int(a.tok[e])
            sc = np.float32(np.float32(logits[r, t] - np.float32(lse[r])) + np.float32(bscore[r]))
            if sc > -np.inf:
                cand.append((-float(sc), r * V + t, float(sc), int(a.nxt[e])))
    cand.sort()
    flat = [c[1] for c in cand[:k]] + [-1] * max(0, k - len(cand))
    return flat, [c[2] for c in cand[:k]], [c[3] for c in cand[:k]]


def test_step_kernel_under_a_filter():
    leaves = _two_level()
    a = Automaton.of(leaves)
    mid = [a.prefixes.index((100 + m,)) for m in range(4)]
    rng = np.random.default_rng(9)
    logits = rng.standard_normal((4, V)).astype(np.float32)
    bscore = [-0.5, -1.25, -0.75, -2.0]
    k = 8
    lse, _, _, _, _, plain = _expand_masked(a, None, 0, logits, bscore, mid, k)
    best = int(plain[0])
    br, bt = best // V, best % V
    cases = {
        "the best candidate blocked": [[100 + br, bt]],
        "one live row wholly blocked beside live ones": [[101, 1010 + j] for j in range(6)],
        "fewer than k survivors": [q for q in leaves if q not in ([100, 1003], [102, 1021], [103, 1035])],
    }
    for what, listed in cases.items():
        h, words, _, status = build_masks(a, [0], [listed], F.BLOCK)
        _, o_s, o_p, o_t, o_n, o_f = _expand_masked(a, h, 0, logits, bscore, mid, k)
        flat, sc, nodes = _expand_ref(a, words[0], logits, lse, bscore, mid, k)
        assert o_f.tolist() == flat, what                                           # ids exact and in order, the tail flat -1
        nv = len(sc)
        assert np.array_equal(o_s[:nv], np.asarray(sc, np.float32)) and o_n[:nv].tolist() == nodes, what
        assert all(o_s[nv:] == -np.inf), what
        assert (o_p[:nv] * V + o_t[:nv]).tolist() == flat[:nv], what
        if what.startswith("the best"):
            assert best not in flat and flat != plain.tolist()
        if what.startswith("one live"):
            assert 1 not in o_p[:nv].tolist() and nv == k
        if what.startswith("fewer"):
            assert nv == 3 and flat[3:] == [-1] * 5


def test_step_kernel_tie_between_a_blocked_and_an_unblocked_candidate():
    a = Automaton.of(_two_level())
    mid = [a.prefixes.index((100 + m,)) for m in range(4)]
    rng = np.random.default_rng(10)
    logits = rng.standard_normal((4, V)).astype(np.float32)
    logits[0, 1002] = logits[0, 1004] = np.float32(9.0)                               # two children of row 0 tie for the best score
    bscore = [-0.5, -1.25, -0.75, -2.0]
    lse, _, _, _, _, plain = _expand_masked(a, None, 0, logits, bscore, mid, 3)
    assert plain[:2].tolist() == [1002, 1004]                                         # unfiltered: lowest flat id first
    h, words, _, _ = build_masks(a, [0], [[[100, 1002]]], F.BLOCK)
    _, o_s, _, _, _, o_f = _expand_masked(a, h, 0, logits, bscore, mid, 3)
    flat, sc, _ = _expand_ref(a, words[0], logits, lse, bscore, mid, 3)
    assert o_f.tolist() == flat and flat[0] == 1004 and 1002 not in flat and np.array_equal(o_s, np.asarray(sc, np.float32))
    # masks of another automaton are refused
    other = Automaton.of(_two_level())
    lib = _lib.load()
    x = torch.zeros(4, V, device="cuda")
    y = torch.zeros(64, device="cuda")
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert lib.atspeed_beam_expand_prune_masked(x.data_ptr(), V, y.data_ptr(), y.data_ptr(), z.data_ptr(), 4, other.h.ptr, 3, y.data_ptr(), z.data_ptr(),
                                                z.data_ptr(), z.data_ptr(), z.data_ptr(), h.ptr, 0, None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------------------------- 3. the cutoff kernel alone
def _cutoffs(a: Automaton, masks, logits, nodes, temperature, top_k, top_p, min_keep):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n = len(nodes)
    lg = torch.from_numpy(logits).to(dev).contiguous()
    lse = torch.empty(n, dtype=torch.float32, device=dev)
    nd = torch.tensor(nodes, dtype=torch.int32, device=dev)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(lib.atspeed_lse_rows(lg.data_ptr(), n, V, V, lse.data_ptr(), st))
    _lib.check(lib.atspeed_warp_cutoffs_masked(lg.data_ptr(), V, lse.data_ptr(), n, a.h.ptr, nd.data_ptr(), float(temperature), int(top_k),
                                               float(top_p), int(min_keep), out.data_ptr(), masks.ptr if masks else None, 0, st))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_cutoff_kernel_under_a_filter_equals_the_kernel_on_the_filtered_automaton():
    """a row of at most 1024 children (sorted in LDS) and one of 1500 (radix select): the masked kernel = the unmasked kernel on a CSR from
    which the blocked edges were removed"""
    rng = np.random.default_rng(4)
    small = np.sort(rng.choice(np.arange(100, V), size=700, replace=False))
    big = np.sort(rng.choice(np.arange(100, V), size=1500, replace=False))
    a = Automaton.of([[1, int(t)] for t in small] + [[2, int(t)] for t in big])
    n1, n2 = a.prefixes.index((1,)), a.prefixes.index((2,))
    listed = [[1, int(t)] for t in rng.choice(small, size=200, replace=False)] + [[2, int(t)] for t in rng.choice(big, size=330, replace=False)]
    logits = (rng.standard_normal((2, V)) * np.asarray([[2.0], [8.0]])).astype(np.float32)
    # the best entries of both rows are among the blocked ones: the cutoffs must move
    listed += [[1, int(small[np.argmax(logits[0, small])])], [2, int(big[np.argmax(logits[1, big])])]]
    h, words, _, status = build_masks(a, [0], [listed], F.BLOCK)
    assert status[0] == 0
    rp, tok, nxt = F.filtered_csr(a.row_ptr, a.tok, a.nxt, words[0])
    cut = Automaton(rp, tok, nxt)
    assert rp[n2 + 1] - rp[n2] == 1500 - 331 > 1024 and rp[n1 + 1] - rp[n1] == 700 - 201
    moved = 0
    for top_k, top_p, min_keep in ((50, 1.0, 2), (8, 0.9, 2), (0, 0.5, 2), (0, 0.9, 1), (1, 1.0, 1)):
        got = _cutoffs(a, h, logits, [n1, n2], 1.3, top_k, top_p, min_keep)
        want = _cutoffs(cut, None, logits, [n1, n2], 1.3, top_k, top_p, min_keep)
        assert np.array_equal(got, want) and np.isfinite(got).all(), (top_k, top_p, got, want)
        moved += int((got != _cutoffs(a, None, logits, [n1, n2], 1.3, top_k, top_p, min_keep)).sum())
    assert moved >= 5


# ---------------------------------------------------------------------------------------------- engine fixtures
def _golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "item_filter_golden.json")) as f:
        return {c["name"]: c for c in json.load(f)}


class _Pair:
    """models, prompt and filter lists of one base case, built once"""

    def __init__(self, name, dtype=torch.float32):
        self.case = IC.base_case(name)
        self.ci = IC.build_case_inputs(self.case)
        kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
        self.tgt = HipLlama.from_state_dict(self.ci["target_dims"], self.ci["target_sd"], dtype, num_beams=self.case["K"], **kw)
        self.drf = HipLlama.from_state_dict(self.ci["draft_dims"], self.ci["draft_sd"], dtype, num_beams=self.case["DK"], **kw)
        self.inputs = {"input_ids": torch.from_numpy(self.ci["prompt"])[None].cuda()}
        self.P = len(self.ci["prompt"])
        self.items = [[int(t) for t in it] for it in self.ci["items"]]

    def lists(self, kind, bssd_golden):
        return IC.filter_lists(self.case["name"], kind, self.ci["items"], bssd_golden[self.case["name"]]["tg_tokens"])

    def kw(self, lists):
        return {"exclude_items": lists["exclude"]} if "exclude" in lists else {"allow_items": lists["allow"]}

    def gen(self, out):
        return out["beam_sequence"][:, self.P:].cpu().tolist()

    def other_inputs(self, n):
        rng0 = np.random.default_rng(1)
        prompts = [self.ci["prompt"]] + [np.concatenate([rng0.integers(3, 31000, size=m), self.ci["prompt"][-6:]]) for m in (9, 30, 17, 5, 23)[:n - 1]]
        return [{"input_ids": torch.from_numpy(p.astype(np.int64))[None].cuda()} for p in prompts]


_pairs = {}


def pair_of(name, dtype=torch.float32):
    if (name, dtype) not in _pairs:
        _pairs[(name, dtype)] = _Pair(name, dtype)
    return _pairs[(name, dtype)]


# ---------------------------------------------------------------------------------------------- 4. fp32 engine against the golden
@pytest.mark.parametrize("base,kind", IC.all_cases(), ids=[IC.case_id(b, k) for b, k in IC.all_cases()])
def test_engine_equals_the_reference_under_the_same_filter(base, kind, bssd_golden):
    gold = _golden()[IC.case_id(base, kind)]
    p = pair_of(base)
    case, lists = p.case, p.lists(kind, bssd_golden)
    kw = p.kw(lists)
    tg = target_generate(p.tgt, p.inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=p.ci["fn"], **kw)
    assert p.gen(tg) == gold["tg_tokens"]
    np.testing.assert_allclose(tg["beam_scores"].cpu().numpy(), gold["tg_scores"], atol=SCORE_TOL, rtol=0)
    out = BSSD(p.tgt, p.drf, p.inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=p.ci["fn"], **kw)
    assert p.gen(out) == gold["bssd_tokens"] == gold["tg_tokens"]                          # BSSD == target_generate under the filter
    np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), gold["bssd_scores"], atol=SCORE_TOL, rtol=0)
    assert out["n_run"] == gold["n_run"] and out["total_accept_steps"] == gold["total_accept_steps"]
    tr = last_trace(p.tgt, p.drf)
    assert [r["n_matches"] for r in tr] == [r["n_matches"] for r in gold["rounds"]]
    for r, g in zip(tr, gold["rounds"]):
        for ids, gids, n in zip(r["draft_ids"], g["draft_ids"], g["step_len"][1:]):
            assert [x for x in ids if x >= 0] == gids and len(gids) == n
    # the filter did something, and what it should
    plain = bssd_golden[base]["tg_tokens"]
    assert gold["tg_tokens"] != plain
    if "exclude" in lists:
        assert not any(row in lists["exclude"] for row in gold["tg_tokens"])
    else:
        assert all(row in lists["allow"] for row in gold["tg_tokens"])
    # the same closure through the build's own host path gives the same ids
    closure = F.closure(p.ci["fn"], synth.RESPONSE_SEP, **lists)
    host = target_generate(p.tgt, p.inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=closure)
    assert p.gen(host) == gold["tg_tokens"][:host["n_valid"]] and host["n_valid"] == case["K"]
    if kind == "block_top3" and base == "k8_dk16_trie":
        hb = BSSD(p.tgt, p.drf, p.inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=closure)
        assert p.gen(hb) == gold["bssd_tokens"] and hb["n_run"] == gold["n_run"]


# ---------------------------------------------------------------------------------------------- 5. batches and sessions
def _same_user(a, b, P_a=None):
    assert torch.equal(a["beam_sequence"], b["beam_sequence"])
    np.testing.assert_allclose(a["beam_scores"].cpu().numpy(), b["beam_scores"].cpu().numpy(), atol=SCORE_TOL, rtol=0)
    assert a["n_valid"] == b["n_valid"]
    if "n_run" in a and "n_run" in b:
        assert a["n_run"] == b["n_run"] and a["accept_steps"] == b["accept_steps"]


def test_batch_of_four_users_each_equals_its_own_call(bssd_golden):
    p = pair_of("k8_dk16_trie")
    case, fn = p.case, p.ci["fn"]
    g, L = case["gamma"], case["max_new_tokens"]
    inputs = p.other_inputs(4)
    block, allow = p.lists("block_first_code", bssd_golden)["exclude"], p.lists("allow_pick", bssd_golden)["allow"]
    excl, allw = [block, None, None, []], [None, allow, None, None]
    outs = BSSD_batch(p.tgt, p.drf, inputs, g, L, prefix_allowed_tokens_fn=fn, exclude_items=excl, allow_items=allw)
    singles = [BSSD(p.tgt, p.drf, inputs[0], g, L, prefix_allowed_tokens_fn=fn, exclude_items=block),
               BSSD(p.tgt, p.drf, inputs[1], g, L, prefix_allowed_tokens_fn=fn, allow_items=allow),
               BSSD(p.tgt, p.drf, inputs[2], g, L, prefix_allowed_tokens_fn=fn),
               BSSD(p.tgt, p.drf, inputs[3], g, L, prefix_allowed_tokens_fn=fn, exclude_items=[])]
    for o, s in zip(outs, singles):
        _same_user(o, s)
    plain = BSSD_batch(p.tgt, p.drf, inputs, g, L, prefix_allowed_tokens_fn=fn)               # the decoders kept no filter
    _same_user(outs[2], plain[2])
    _same_user(outs[3], plain[3])                                                            # None and the empty list = unfiltered
    assert not torch.equal(outs[0]["beam_sequence"], plain[0]["beam_sequence"])
    assert not torch.equal(outs[1]["beam_sequence"], plain[1]["beam_sequence"])
    first = block[0][0]
    assert not (outs[0]["beam_sequence"][:, inputs[0]["input_ids"].shape[1]] == first).any()
    # the same lists through a session of two lanes, and through the plain beam search of the target
    laned = BSSD_batch(p.tgt, p.drf, inputs, g, L, prefix_allowed_tokens_fn=fn, exclude_items=excl, allow_items=allw, lanes=2)
    for o, s in zip(laned, outs):
        _same_user(o, s)
    assert laned[0]["session_counters"]["allocs_after_create"] == 0
    tgs = target_generate_batch(p.tgt, inputs, L, prefix_allowed_tokens_fn=fn, exclude_items=excl, allow_items=allw)
    for o, s in zip(tgs, outs):
        assert torch.equal(o["beam_sequence"], s["beam_sequence"])                            # lossless under every filter


def test_session_masks_follow_users_not_lanes(bssd_golden):
    p = pair_of("k8_dk16_trie")
    case, fn = p.case, p.ci["fn"]
    g, L = case["gamma"], case["max_new_tokens"]
    inputs = p.other_inputs(6)
    rng = np.random.default_rng(2)
    filt = [dict(exclude_items=[p.items[i] for i in rng.choice(len(p.items), size=150, replace=False)]) for _ in range(3)]
    filt += [dict(allow_items=[p.items[i] for i in rng.choice(len(p.items), size=60, replace=False)]) for _ in range(2)] + [dict()]
    singles = [BSSD(p.tgt, p.drf, inp, g, L, prefix_allowed_tokens_fn=fn, **f) for inp, f in zip(inputs, filt)]
    assert len({tuple(map(tuple, p.gen(s))) for s in singles}) >= 5                            # distinct filters, distinct results
    with BSSDSession(p.tgt, p.drf, 2, g, L, prefix_allowed_tokens_fn=fn) as ses:
        tickets = [ses.submit(inp, **f) for inp, f in zip(inputs, filt)]
        done = dict(ses.drain())
        assert ses.counters()["allocs_after_create"] == 0
        lanes = [done[t]["lane"] for t in tickets]
    assert sorted(set(lanes)) == [0, 1]
    for t, s in zip(tickets, singles):
        _same_user(done[t], s)


# ---------------------------------------------------------------------------------------------- 6. fewer survivors than K
def test_fewer_survivors_than_beams(bssd_golden):
    p = pair_of("k8_dk16_trie")
    case, fn = p.case, p.ci["fn"]
    allow, seen = [], set()
    for it in p.items:                                                                        # five items with distinct first codes
        if it[0] not in seen:
            seen.add(it[0])
            allow.append(it)
        if len(allow) == 5:
            break
    L, K = case["max_new_tokens"], case["K"]
    assert K == 8
    closure = F.closure(fn, synth.RESPONSE_SEP, allow=allow)
    ref = R.target_generate(RefLlama(p.ci["target_dims"], p.ci["target_sd"]), p.ci["prompt"], L, 5, closure)    # a beam as wide as the candidate set is exhaustive
    want = ref["beam_sequence"][:, p.P:].tolist()
    assert sorted(want) == sorted(allow)
    for out in (target_generate(p.tgt, p.inputs, L, prefix_allowed_tokens_fn=fn, allow_items=allow),
                BSSD(p.tgt, p.drf, p.inputs, case["gamma"], L, prefix_allowed_tokens_fn=fn, allow_items=allow)):
        assert out["n_valid"] == 5
        assert p.gen(out)[:5] == want
        sc = out["beam_scores"].cpu().numpy()
        np.testing.assert_allclose(sc[:5], ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
        # the rest is "not a beam", the build's rule for a pick without a candidate: score -inf, pick token 0 (behind the prefix of beam 0)
        assert np.all(sc[5:] == -np.inf) and not out["beam_sequence"][5:, -1].any()


# ---------------------------------------------------------------------------------------------- 7. sampling
@pytest.mark.parametrize("top_k,top_p", [(None, None), (8, 0.9)])
def test_sampling_under_a_block_list_makes_the_oracles_decisions(top_k, top_p, bssd_golden, monkeypatch):
    """oracle/beamsd_sample_ref.py with the filter closure and HashRng, seed for seed: draws are keyed by flat id, so absent candidates shift
    nothing.  A seed whose closest draw is decided by less than 1e-4 (fp32 rounding of the summed scores; HashRng.min_margin, the rule of
    tests/test_warpers_gpu.py) is compared only if it agrees."""
    from oracle import beamsd_sample_ref as S
    p = pair_of("k8_dk16_trie")
    case, fn = p.case, p.ci["fn"]
    lists = p.lists("block_first_code", bssd_golden)
    closure = F.closure(fn, synth.RESPONSE_SEP, **lists)
    T = 1.3
    if top_k:
        from transformers import TopKLogitsWarper, TopPLogitsWarper
        warpers = [TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=2), TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=2)]
        plain = S._tempered

        def warped(logits, seqs, beam_size, f, temperature):
            rows = plain(logits, seqs, beam_size, f, temperature)
            for w in warpers:
                rows = w(None, rows)
            return rows
        monkeypatch.setattr(S, "_tempered", warped)
    rt, rd = RefLlama(p.ci["target_dims"], p.ci["target_sd"]), RefLlama(p.ci["draft_dims"], p.ci["draft_sd"])
    g, L = case["gamma"], case["max_new_tokens"]
    try:
        for m in (p.tgt, p.drf):
            m.generation_config.do_sample, m.generation_config.temperature = True, T
            m.generation_config.top_k, m.generation_config.top_p = top_k, top_p
        checked = 0
        first = lists["exclude"][0][0]
        for seed in (40, 41, 42, 43):
            rng = S.HashRng(seed)
            ref = S.BSSD_sample(rt, rd, p.ci["prompt"], g, L, case["K"], case["DK"], closure, T, rng)
            out = BSSD(p.tgt, p.drf, p.inputs, g, L, prefix_allowed_tokens_fn=fn, seed=seed, exclude_items=lists["exclude"])
            nv = out["n_valid"]
            assert not (out["beam_sequence"][:nv, p.P] == first).any()
            same = nv == ref["beam_sequence"].shape[0] and out["beam_sequence"][:nv, p.P:].cpu().tolist() == ref["beam_sequence"][:, p.P:].tolist()
            if rng.min_margin < 1e-4 and not same:
                continue
            checked += 1
            assert same, (seed, rng.min_margin)
            assert out["accept_steps"] == [r["n_matches"] for r in ref["rounds"]] and out["n_run"] == ref["n_run"]
            np.testing.assert_allclose(out["beam_scores"][:nv].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
        assert checked >= 3
    finally:
        for m in (p.tgt, p.drf):
            m.generation_config.do_sample = False
            m.generation_config.top_k = m.generation_config.top_p = None


# ---------------------------------------------------------------------------------------------- 8. set, then clear
def test_a_decoder_that_lost_its_mask_is_unfiltered_and_a_blocked_start_node_is_refused(bssd_golden):
    p = pair_of("k20_dk40_trie")
    case, fn = p.case, p.ci["fn"]
    g, L = case["gamma"], case["max_new_tokens"]
    before = BSSD(p.tgt, p.drf, p.inputs, g, L, prefix_allowed_tokens_fn=fn)
    filtered = BSSD(p.tgt, p.drf, p.inputs, g, L, prefix_allowed_tokens_fn=fn, **p.kw(p.lists("block_top3", bssd_golden)))
    after = BSSD(p.tgt, p.drf, p.inputs, g, L, prefix_allowed_tokens_fn=fn)
    assert not torch.equal(filtered["beam_sequence"], before["beam_sequence"])
    assert torch.equal(after["beam_sequence"], before["beam_sequence"]) and torch.equal(after["beam_scores"], before["beam_scores"])   # the bits
    assert p.gen(before) == bssd_golden[case["name"]]["tg_tokens"]
    for call in (lambda **kw: BSSD(p.tgt, p.drf, p.inputs, g, L, prefix_allowed_tokens_fn=fn, **kw),
                 lambda **kw: target_generate(p.tgt, p.inputs, L, prefix_allowed_tokens_fn=fn, **kw)):
        with pytest.raises(ValueError, match="user 0"):
            call(exclude_items=p.items)                                               # every item: the start node ends up blocked
        with pytest.raises(ValueError, match="user 0"):
            call(allow_items=[[5, 6, 7, 8]])                                          # nothing the trie knows
    with pytest.raises(ValueError, match="user 1"):
        BSSD_batch(p.tgt, p.drf, [p.inputs, p.inputs], g, L, prefix_allowed_tokens_fn=fn, exclude_items=[None, p.items])
    again = BSSD(p.tgt, p.drf, p.inputs, g, L, prefix_allowed_tokens_fn=fn)
    assert torch.equal(again["beam_sequence"], before["beam_sequence"])


# ---------------------------------------------------------------------------------------------- 9. bf16 engine
def test_bf16_bssd_equals_its_own_target_generate_under_a_block_list(bssd_golden):
    p = pair_of("k8_dk16_trie", torch.bfloat16)
    case, fn = p.case, p.ci["fn"]
    plain = target_generate(p.tgt, p.inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=fn)
    block = p.gen(plain)[:3] + [it for it in p.items if it[0] == p.gen(plain)[3][0]]
    tg = target_generate(p.tgt, p.inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=fn, exclude_items=block)
    out = BSSD(p.tgt, p.drf, p.inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=fn, exclude_items=block)
    assert p.gen(out) == p.gen(tg) and out["n_valid"] == tg["n_valid"] == case["K"]
    np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), tg["beam_scores"].cpu().numpy(), atol=0.05, rtol=0)
    assert not any(row in block for row in p.gen(tg)) and p.gen(tg) != p.gen(plain)
