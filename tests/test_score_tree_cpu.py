"""tests/score_tree_ref.py against brute force: every row's visible set is the prompt plus its own prefix, every token is predicted by the row
whose (prompt ++ prefix) precedes it, rows are numbered in (sequence, depth) order and no prefix owns two rows."""
import itertools

import numpy as np
import pytest

from tests import score_tree_ref as T


def _visible(vis_row):
    return {64 * w + b for w, word in enumerate(vis_row) for b in range(64) if (int(word) >> b) & 1}


def check_brute_force(prompt, seqs, max_slots=512):
    lay = T.layout(prompt, seqs, max_slots)
    P = len(prompt)
    assert lay["status"] == T.OK
    R = lay["n_rows"]
    # what each row stands for: its whole input sequence, prompt ++ prefix
    content = {r: tuple(prompt[: r + 1]) for r in range(P)}
    for r in range(P, R):
        seen = sorted(_visible(lay["vis"][r]))
        assert seen[:P] == list(range(P)) and seen[-1] == r and lay["slot"][r] == r
        anc = seen[P:]
        assert [int(lay["pos"][a]) for a in anc] == list(range(P, P + len(anc))), "a row sees one row per depth of its prefix, in order"
        content[r] = tuple(prompt) + tuple(int(lay["ids"][a]) for a in anc)
    for r in range(P):
        assert _visible(lay["vis"][r]) == set(range(r + 1)) and lay["pos"][r] == r and lay["slot"][r] == r and lay["ids"][r] == prompt[r]
    assert len(set(content.values())) == R, "no prefix owns two rows"
    # exactly the proper non-empty prefixes of the items have tree rows
    want = {tuple(prompt) + tuple(q[:d + 1]) for q in seqs for d in range(len(q) - 1)}
    assert {content[r] for r in range(P, R)} == want
    for s, q in enumerate(seqs):
        for d in range(T.LMAX):
            pr = int(lay["pred_row"][s, d])
            if d >= len(q):
                assert pr == -1
            else:
                assert content[pr] == tuple(prompt) + tuple(q[:d]), (s, d)
    # (sequence, depth) order: the first appearance of each prefix, in list order
    first = []
    for q in seqs:
        for d in range(len(q) - 1):
            key = tuple(prompt) + tuple(q[:d + 1])
            if key not in first:
                first.append(key)
    assert [content[r] for r in range(P, R)] == first
    return lay


CASES = {
    "single_len1": [[7]],
    "single_len5": [[7, 8, 9, 10, 11]],
    "mixed_lengths": [[3], [4, 1], [4, 2, 6, 1], [4, 2, 6, 2, 9], [5, 1, 1, 1], [5, 2]],
    "proper_prefix_then_extension": [[1, 2], [1, 2, 3], [1, 2, 3, 4], [1, 2, 4]],
    "prefix_chain_from_len1": [[1], [1, 2], [1, 2, 3]],
    "shared_3": [[9, 8, 7, t, u] for t in range(3) for u in range(2)],
    "no_sharing": [[t, 50 + t, 60 + t] for t in range(10)],
    "sibling_after_deep": [[1, 2, 3, 4, 5], [1, 3], [1, 3, 1], [2]],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_brute_force(name):
    seqs = CASES[name]
    assert T.strictly_ascending(seqs)
    check_brute_force(list(range(100, 107)), seqs)


def test_layout_random_lists_and_word_edges():
    rng = np.random.default_rng(11)
    for trial in range(40):
        n = int(rng.integers(1, 80))
        pool = {tuple(int(t) for t in rng.integers(0, 4, size=int(rng.integers(1, 7)))) for _ in range(n)}
        seqs = [list(q) for q in sorted(pool)]
        P = int(rng.choice([1, 2, 60, 63, 64, 65]))
        lay = check_brute_force(list(rng.integers(0, 1000, size=P)), seqs, max_slots=1024)
        assert lay["n_rows"] == P + len({q[:d + 1] for q in pool for d in range(len(q) - 1)})


def test_every_item_of_a_full_trie_shares_its_levels():
    seqs = [list(q) for q in itertools.product(range(3), range(4), range(2), range(5))]
    lay = check_brute_force([1, 2, 3], seqs)
    assert lay["n_rows"] == 3 + 3 + 12 + 24              # one row per interior trie node; the 120 leaves need none


def test_order_violations_and_capacity():
    assert T.layout([1], [[2, 1], [1, 5]], 64)["status"] == T.ERR_INVALID
    assert T.layout([1], [[1, 5], [1, 5]], 64)["status"] == T.ERR_INVALID
    assert T.layout([1], [[1, 5, 2], [1, 5]], 64)["status"] == T.ERR_INVALID         # an extension before its prefix
    seqs = [[t, 1, 2] for t in range(40)]
    full = T.layout(list(range(10)), seqs, 64, cap=200)
    assert full["n_rows"] == 90 and full["status"] == T.ERR_CAPACITY and len(full["ids"]) == 64
    exact = T.layout(list(range(10)), seqs[:27], 64)
    assert exact["n_rows"] == 64 and exact["status"] == T.OK
    ref = T.layout(list(range(10)), seqs, 128)
    assert np.array_equal(full["ids"], ref["ids"][:64]) and np.array_equal(full["pred_row"], ref["pred_row"])


def test_known_walk():
    row_ptr, tok, nxt = T.csr_from_sequences([[1, 2, 3], [1, 4], [5]])
    assert T.is_known(row_ptr, tok, nxt, 0, [1, 2]) and T.is_known(row_ptr, tok, nxt, 0, [5])
    assert not T.is_known(row_ptr, tok, nxt, 0, [1, 3]) and not T.is_known(row_ptr, tok, nxt, 0, [5, 1])
    rp, tk, nx = T.position_set_csr([[1, 2], [3, 4], [9]])
    assert T.is_known(rp, tk, nx, 0, [2, 3, 9]) and T.is_known(rp, tk, nx, 1, [4, 9]) and not T.is_known(rp, tk, nx, 0, [3])
