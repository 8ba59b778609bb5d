"""numpy restatement of the packed layout of a scored item list (include/atspeed_hip.h "scoring candidates"): the prompt's causal rows, then
one row per NEW prefix of the sorted item list.  The builder kernel (scan.hip, score_tree_kernel) must equal this bit for bit; this file is
checked against brute force by tests/test_score_tree_cpu.py."""
from __future__ import annotations

import numpy as np

LMAX = 16                                   # ATSPEED_MAX_NEW_TOKENS
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -3


def strictly_ascending(seqs) -> bool:
    """lexicographic, a proper prefix before its extensions, no duplicates (Python's tuple order)"""
    t = [tuple(int(x) for x in q) for q in seqs]
    return all(a < b for a, b in zip(t, t[1:]))


def shared_depths(prev, seq) -> int:
    """e(s) = min(lcp(s), len(s - 1) - 1): the leading depths of `seq` whose rows earlier sequences own.  The predecessor owns no row for
    its LAST token (nothing is predicted from it), so a sequence that continues its predecessor owns that depth itself."""
    if prev is None:
        return 0
    lcp = 0
    while lcp < min(len(prev), len(seq)) and int(prev[lcp]) == int(seq[lcp]):
        lcp += 1
    return max(0, min(lcp, len(prev) - 1))


def n_rows(P: int, seqs) -> int:
    rows, prev = P, None
    for q in seqs:
        rows += max(0, len(q) - 1 - shared_depths(prev, q))
        prev = q
    return rows


def find_edge(row_ptr, tok, node: int, t: int) -> int:
    lo, hi = int(row_ptr[node]), int(row_ptr[node + 1])
    i = lo + int(np.searchsorted(tok[lo:hi], t))
    return i if i < hi and int(tok[i]) == t else -1


def is_known(row_ptr, tok, nxt, start: int, seq) -> bool:
    node = start
    for t in seq:
        e = find_edge(row_ptr, tok, node, int(t))
        if e < 0:
            return False
        node = int(nxt[e])
    return True


def layout(prompt, seqs, max_slots: int, cap: int = None):
    """-> dict(ids, pos, slot [rows] int32, vis [rows][max_slots / 64] uint64, pred_row [len(seqs)][LMAX] int32 (-1 past a sequence's end),
    n_rows, status).  `cap`: rows the caller's arrays hold (default: exactly enough, at most max_slots); rows at or past min(cap, max_slots)
    are not produced and the status is ERR_CAPACITY.  An order violation gives ERR_INVALID and only n_rows / status are defined."""
    P, W = len(prompt), max_slots // 64
    total = n_rows(P, seqs)
    if not strictly_ascending(seqs):
        return dict(n_rows=total, status=ERR_INVALID)
    cap = min(total if cap is None else cap, max_slots)
    R = min(total, cap)
    ids, pos, slot = (np.zeros(R, np.int32) for _ in range(3))
    vis = np.zeros((R, W), np.uint64)
    pred = np.full((len(seqs), LMAX), -1, np.int32)

    def set_bits(r, bits):
        for s in bits:
            vis[r, s >> 6] |= np.uint64(1) << np.uint64(s & 63)

    for r in range(min(P, R)):
        ids[r], pos[r], slot[r] = int(prompt[r]), r, r
        set_bits(r, range(r + 1))
    owner = {}                               # depth -> row that owns the current prefix of that depth
    nxt_row, prev = P, None
    for s, q in enumerate(seqs):
        e = shared_depths(prev, q)
        for d in list(owner):
            if d >= e:
                del owner[d]
        for d in range(e, len(q) - 1):
            owner[d] = nxt_row
            if nxt_row < R:
                ids[nxt_row], pos[nxt_row], slot[nxt_row] = int(q[d]), P + d, nxt_row
                set_bits(nxt_row, list(range(P)) + [owner[a] for a in range(d + 1) if owner[a] < R])
            nxt_row += 1
        for d in range(len(q)):
            pred[s, d] = P - 1 if d == 0 else owner[d - 1]
        prev = q
    assert nxt_row == total
    return dict(ids=ids, pos=pos, slot=slot, vis=vis, pred_row=pred, n_rows=total, status=OK if total <= cap else ERR_CAPACITY)


def csr_from_sequences(seqs):
    """a trie over `seqs` as the automaton's CSR arrays (breadth-first ids, children ascending) -> (row_ptr, tok, nxt)"""
    kids = [{}]
    for q in seqs:
        node = 0
        for t in q:
            t = int(t)
            if t not in kids[node]:
                kids[node][t] = len(kids)
                kids.append({})
            node = kids[node][t]
    order, newid = [0], {0: 0}
    for n in order:
        for t in sorted(kids[n]):
            newid[kids[n][t]] = len(order)
            order.append(kids[n][t])
    row_ptr, tok, nxt = [0], [], []
    for n in order:
        for t in sorted(kids[n]):
            tok.append(t)
            nxt.append(newid[kids[n][t]])
        row_ptr.append(len(tok))
    return np.asarray(row_ptr, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32)


def position_set_csr(levels):
    """one node per depth: node d allows levels[d] and leads to node d + 1 (the last node has no children)"""
    row_ptr, tok, nxt = [0], [], []
    for d, allowed in enumerate(levels):
        for t in sorted(int(x) for x in allowed):
            tok.append(t)
            nxt.append(d + 1)
        row_ptr.append(len(tok))
    row_ptr.append(len(tok))
    return np.asarray(row_ptr, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32)
