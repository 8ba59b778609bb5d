"""The two kernels behind atspeed_score_items, each alone (include/atspeed_hip.h "scoring candidates"): the tree builder against the numpy
restatement tests/score_tree_ref.py bit for bit, and the path-score kernel on placed logits whose terms are exactly summable in fp32."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib
from tests import score_tree_ref as T

V = 6000
DEV = torch.device("cuda", 0)
SENT = -7777                                  # what every output array holds before the launch


class Automaton:
    def __init__(self, row_ptr, tok, nxt, vocab=V):
        self.row_ptr, self.tok, self.nxt = (np.ascontiguousarray(a, np.int32) for a in (row_ptr, tok, nxt))
        self.n_nodes = len(self.row_ptr) - 1
        self.h = _lib.Handle.create("atspeed_fsm_destroy", _lib.load().atspeed_fsm_create, self.row_ptr.ctypes.data, self.tok.ctypes.data,
                                    self.nxt.ctypes.data, self.n_nodes, len(self.tok), vocab)


def trie_of(seqs):
    return Automaton(*T.csr_from_sequences(seqs))


def build(a: Automaton, prompts, starts, lists, max_slots=512, caps=None, guard=3):
    """one launch for len(prompts) users, their row ranges back to back (user u's holds caps[u] rows; default: two more than it needs) -> per
    user dict(ids, pos, slot, vis, pred_row, known, n_rows, unknown, status, tail), `tail` = the `guard` rows behind the last range"""
    lib, n, W = _lib.load(), len(prompts), max_slots // 64
    toks = [int(t) for seqs in lists for q in seqs for t in q]
    soff = np.concatenate([[0], np.cumsum([len(q) for seqs in lists for q in seqs])]).astype(np.int32)
    uoff = np.concatenate([[0], np.cumsum([len(seqs) for seqs in lists])]).astype(np.int32)
    if caps is None:
        caps = [T.n_rows(len(p), seqs) + 2 for p, seqs in zip(prompts, lists)]
    roff = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)
    n_seq, R = int(uoff[-1]), int(roff[-1]) + guard
    dev = lambda x, dt: torch.tensor(np.asarray(x), dtype=dt, device=DEV)
    d_prompts = [dev(p, torch.int32) for p in prompts]
    d_tok, d_soff = dev(toks, torch.int32), dev(soff, torch.int32)
    ids, pos, slot = (torch.full((R,), SENT, dtype=torch.int32, device=DEV) for _ in range(3))
    vis = torch.full((R, W), SENT, dtype=torch.int64, device=DEV)
    pred = torch.full((n_seq, T.LMAX), SENT, dtype=torch.int32, device=DEV)
    known = torch.full((n_seq,), SENT, dtype=torch.int32, device=DEV)
    res = torch.full((3, n), SENT, dtype=torch.int32, device=DEV)
    a_prompt = (C.c_void_p * n)(*[t.data_ptr() for t in d_prompts])
    a_len = np.asarray([len(p) for p in prompts], np.int32)
    a_start = np.asarray(starts, np.int32)
    _lib.check(lib.atspeed_score_tree_build(a.h.ptr, n, a_prompt, a_len.ctypes.data, a_start.ctypes.data, d_tok.data_ptr(), len(toks),
                                            d_soff.data_ptr(), uoff.ctypes.data, max_slots, roff.ctypes.data, ids.data_ptr(), pos.data_ptr(),
                                            slot.data_ptr(), vis.data_ptr(), pred.data_ptr(), known.data_ptr(), res[0].data_ptr(),
                                            res[1].data_ptr(), res[2].data_ptr(), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    ids, pos, slot, vis, pred, known, res = (x.cpu().numpy() for x in (ids, pos, slot, vis, pred, known, res))
    outs, end = [], int(roff[-1])
    for u in range(n):
        r0, r1, s0, s1 = int(roff[u]), int(roff[u + 1]), int(uoff[u]), int(uoff[u + 1])
        outs.append(dict(ids=ids[r0:r1], pos=pos[r0:r1], slot=slot[r0:r1], vis=vis[r0:r1], pred_row=pred[s0:s1], known=known[s0:s1],
                         n_rows=int(res[0, u]), unknown=int(res[1, u]), status=int(res[2, u]), tail=(ids[end:], pos[end:], slot[end:], vis[end:])))
    return outs


def check(a: Automaton, prompts, starts, lists, max_slots=512, caps=None):
    outs = build(a, prompts, starts, lists, max_slots, caps)
    for u, (o, p, st, seqs) in enumerate(zip(outs, prompts, starts, lists)):
        ref = T.layout(p, seqs, max_slots, None if caps is None else caps[u])
        assert (o["n_rows"], o["status"]) == (ref["n_rows"], ref["status"]), u
        want_known = [int(T.is_known(a.row_ptr, a.tok, a.nxt, st, q)) for q in seqs]
        assert o["known"].tolist() == want_known and o["unknown"] == len(seqs) - sum(want_known), u
        if ref["status"] == T.ERR_INVALID:
            continue
        R = len(ref["ids"])
        for name in ("ids", "pos", "slot", "vis"):
            got = o[name].view(np.uint64) if name == "vis" else o[name]
            assert np.array_equal(got[:R], ref[name]), (u, name)
            assert (o[name][R:] == SENT).all(), (u, name, "rows past the count are untouched")
        assert np.array_equal(o["pred_row"], ref["pred_row"]), u
        for t in o["tail"]:
            assert (t == SENT).all(), "the guard rows behind the last range are untouched"
    return outs


PROMPT = list(range(200, 207))
ITEMS = [[10 + a, 20 + b, 30 + c, 40 + d] for a in range(3) for b in range(2) for c in range(2) for d in range(2)]


def test_single_candidate_of_length_1_has_no_tree_rows():
    a = trie_of(ITEMS)
    o = check(a, [PROMPT], [0], [[[11]]])[0]
    assert o["n_rows"] == len(PROMPT) and o["pred_row"][0, 0] == len(PROMPT) - 1 and o["known"][0] == 1


def test_mixed_lengths_prefixes_and_sharing():
    a = trie_of(ITEMS + [[10, 20, 30, 40, 50]])
    lists = [[10], [10, 20], [10, 20, 30, 40], [10, 20, 30, 40, 50], [11, 21], [12, 20, 31, 41]]       # 1, 2, 4, 5; proper prefixes of successors
    check(a, [PROMPT], [0], [lists])
    check(a, [PROMPT], [0], [[[1, 2], [1, 2, 3], [1, 2, 3, 4], [1, 2, 4]]])                              # all unknown: the layout does not care
    shared = [[10, 20, 30, 40 + d, 50 + e] for d in range(2) for e in range(3)]                         # a 3-token prefix shared by all
    o = check(trie_of(shared), [PROMPT], [0], [shared])[0]
    assert o["n_rows"] == len(PROMPT) + 3 + 2
    none = [[t, 50 + t, 60 + t] for t in range(10)]                                                     # nothing shared
    o = check(trie_of(none), [PROMPT], [0], [none])[0]
    assert o["n_rows"] == len(PROMPT) + 20


def test_600_candidates_carry_across_passes():
    """more sequences than the workgroup has threads, with prefixes that straddle the pass boundaries: the owner of a depth comes from an
    earlier pass"""
    rng = np.random.default_rng(5)
    pool = {tuple(int(t) for t in (rng.integers(0, 3), rng.integers(0, 5), rng.integers(0, 9), rng.integers(0, 9))) for _ in range(2000)}
    seqs = [list(q) for q in sorted(pool)][:600]
    assert len(seqs) == 600 and seqs[255][:2] == seqs[256][:2] and seqs[511][:2] == seqs[512][:2]
    a = trie_of(seqs[::2])                                                                              # every other one is unknown
    o = check(a, [PROMPT], [0], [seqs])[0]
    assert o["unknown"] == 300 and o["n_rows"] == 101
    deep = [[1] * 14 + [t // 16, t % 16] for t in range(300)]                                           # 14 shared depths carried into the second pass
    check(trie_of(deep), [PROMPT], [0], [deep])


def test_rows_straddle_word_edges_and_fill_max_slots_exactly():
    seqs = [[t, 1, 2] for t in range(40)]                                                               # 80 tree rows
    a = trie_of(seqs)
    o = check(a, [list(range(60))], [0], [seqs], max_slots=256)[0]                                      # rows 60 .. 139: slots 63 / 64 and 127 / 128
    assert o["n_rows"] == 140
    exact = check(a, [list(range(10))], [0], [seqs[:27]], max_slots=64)[0]                              # 10 + 54 = 64 = max_slots
    assert exact["n_rows"] == 64 and exact["status"] == 0
    over = check(a, [list(range(10))], [0], [seqs], max_slots=64, caps=[64])[0]                         # 90 rows: the 64 that fit, ERR_CAPACITY
    assert over["n_rows"] == 90 and over["status"] == _lib.ERR_CAPACITY
    short = check(a, [list(range(10))], [0], [seqs], max_slots=512, caps=[33])[0]                       # the caller's range is the bound
    assert short["status"] == _lib.ERR_CAPACITY


def test_unsorted_and_duplicate_lists_are_refused():
    a = trie_of(ITEMS)
    for bad in ([[11, 20], [10, 20]], [[10, 20], [10, 20]], [[10, 20, 30], [10, 20]], [[10], [11], [10]]):
        o = build(a, [PROMPT], [0], [bad])[0]
        assert o["status"] == _lib.ERR_INVALID, bad
    check(a, [PROMPT], [0], [[[11, 20], [10, 20]]])


def test_position_set_automaton_rows_are_not_merged():
    """one node per depth: the prefixes (1, 3) and (2, 3) reach the same node and still own a row each"""
    a = Automaton(*T.position_set_csr([[1, 2], [3, 4], [5, 6], [7]]))
    seqs = [[1, 3, 5, 7], [1, 3, 6, 7], [2, 3, 5, 7], [2, 4, 5, 7], [2, 4, 9, 7]]
    o = check(a, [PROMPT], [0], [seqs])[0]
    assert o["n_rows"] == len(PROMPT) + 3 + 1 + 3 + 2 + 1 and o["unknown"] == 1
    assert o["known"].tolist() == [1, 1, 1, 1, 0]
    o = check(a, [PROMPT], [1], [[[3, 5, 7], [4, 6]]])[0]                                               # a start node below the root
    assert o["unknown"] == 0


def test_unknown_sequences_keep_their_rows():
    a = trie_of(ITEMS)
    seqs = [[10, 20, 30, 40], [10, 20, 99, 40], [10, 21, 31, 41], [77]]
    o = check(a, [PROMPT], [0], [seqs])[0]
    assert o["known"].tolist() == [1, 0, 1, 0] and o["unknown"] == 2
    assert o["n_rows"] == check(trie_of(seqs), [PROMPT], [0], [seqs])[0]["n_rows"]


def test_two_users_one_launch():
    a = trie_of(ITEMS)
    n11 = 2                                                                                             # breadth-first: root 0, then 10, 11, 12
    big = [q for q in ITEMS if q[0] != 12] + [[12, 20], [12, 21, 31]]
    lists = [sorted(big), [[20, 30, 40], [20, 31], [21, 99]]]
    outs = check(a, [PROMPT, list(range(300, 333))], [0, n11], lists)
    assert outs[0]["n_rows"] != outs[1]["n_rows"] and outs[1]["unknown"] == 1


# ---------------------------------------------------------------------------------------------- path scores
def test_path_scores_bit_for_bit_on_placed_rows():
    """logits and normalisers are small multiples of 2^-10: every term and every partial sum is exact in fp32, so the expected sums (numpy,
    in token order) must be met bit for bit.  ld > vocab; unknown sequences, a row out of range and a token out of range give -inf."""
    lib = _lib.load()
    rng = np.random.default_rng(9)
    rows, vocab, ld = 37, 300, 320
    logits = (rng.integers(-4096, 4096, size=(rows, ld)) / 1024.0).astype(np.float32)
    logits[:, vocab:] = np.nan                                                                          # the pad columns are never read
    lse = (rng.integers(0, 8192, size=rows) / 1024.0).astype(np.float32)
    lens = [1, 2, 4, 5, 16, 3, 2, 4]
    seqs = [[int(t) for t in rng.integers(0, vocab, size=n)] for n in lens]
    pred = np.full((len(seqs), T.LMAX), -1, np.int32)
    for s, q in enumerate(seqs):
        pred[s, :len(q)] = rng.integers(0, rows - 5, size=len(q))
    base = np.asarray([0, 5, 0, 1, 2, 0, 0, 0], np.int32)
    known = np.asarray([1, 1, 1, 0, 1, 1, 1, 1], np.int32)
    pred[5, 1] = rows                                                                                   # a row the buffers do not have
    seqs[6][0] = vocab                                                                                  # a pad column
    want = np.zeros(len(seqs), np.float32)
    for s, q in enumerate(seqs):
        acc = np.float32(0)
        for d, t in enumerate(q):
            r = int(base[s]) + int(pred[s, d])
            if s in (5, 6):
                continue
            acc = np.float32(acc + np.float32(logits[r, t] - lse[r]))
        want[s] = acc if known[s] and s not in (5, 6) else -np.inf
    toks = np.asarray([t for q in seqs for t in q], np.int32)
    soff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    t_logits, t_lse, t_tok, t_off, t_pred, t_base, t_known = map(d, (logits, lse, toks, soff, pred, base, known))
    out = torch.full((len(seqs) + 2,), 123.0, dtype=torch.float32, device=DEV)
    _lib.check(lib.atspeed_path_scores(t_logits.data_ptr(), ld, t_lse.data_ptr(), rows, vocab, t_tok.data_ptr(), t_off.data_ptr(), t_pred.data_ptr(),
                                       t_base.data_ptr(), t_known.data_ptr(), len(seqs), out.data_ptr(), _lib.stream_ptr(DEV)))
    got = out.cpu().numpy()
    assert np.array_equal(got[:len(seqs)].view(np.uint32), want.view(np.uint32)), (got, want)
    assert (got[len(seqs):] == 123.0).all()
    assert np.isneginf(want[[3, 5, 6]]).all() and np.isfinite(want[[0, 1, 2, 4, 7]]).all()
    # seq_base NULL = 0
    _lib.check(lib.atspeed_path_scores(t_logits.data_ptr(), ld, t_lse.data_ptr(), rows, vocab, t_tok.data_ptr(), t_off.data_ptr(), t_pred.data_ptr(),
                                       None, t_known.data_ptr(), len(seqs), out.data_ptr(), _lib.stream_ptr(DEV)))
    got0 = out.cpu().numpy()
    assert got0[0] == want[0] and got0[2] == want[2]
