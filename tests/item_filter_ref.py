"""Numpy restatement of the per-user item filter (include/atspeed_hip.h "item filters") over a CSR automaton `(row_ptr, tok, nxt)` and a
start node: what `atspeed_node_masks_create` must build bit for bit, and the candidate rule the kernels apply.

A filter is a list of token sequences walked from the user's start node.  A sequence with a token that has no edge is UNKNOWN (ignored,
counted); the END NODE of a known sequence is the node it leads to (not necessarily a leaf).  The result is a bitset over node ids,
ceil(n_nodes / 32) uint32 words, bit 1 = blocked, bits at or above n_nodes 0.
  block: B = the end nodes, then the closure bottom-up along the listed paths: a node on a listed path (start node included) all of whose
         children are in B is in B.
  allow: K = every node on a known path (start node included), E = the end nodes; a node is blocked iff it is a child of a node in K \\ E
         and is not itself in K.
  status: ERR_CONSTRAINT (-4) when the start node ends up blocked (block) or no sequence is known (allow), else 0.
An empty sequence or one longer than MAX_NEW_TOKENS is invalid (ValueError here, ATSPEED_ERR_INVALID in the library).
A candidate (row, child edge e) is absent iff bit nxt[e] is set.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

BLOCK, ALLOW = 0, 1
MAX_NEW_TOKENS = 16
ERR_CONSTRAINT = -4


def n_words(n_nodes: int) -> int:
    return (n_nodes + 31) // 32


def walk(row_ptr, tok, nxt, start: int, seq: Sequence[int]):
    """[start, node after token 0, ...] or None when a token has no edge"""
    path, node = [int(start)], int(start)
    for t in seq:
        lo, hi = int(row_ptr[node]), int(row_ptr[node + 1])
        j = lo + int(np.searchsorted(tok[lo:hi], t))
        if j >= hi or int(tok[j]) != int(t):
            return None
        node = int(nxt[j])
        path.append(node)
    return path


def children(row_ptr, nxt, node: int) -> List[int]:
    return [int(c) for c in nxt[int(row_ptr[node]): int(row_ptr[node + 1])]]


def node_mask(row_ptr, tok, nxt, start: int, seqs: Sequence[Sequence[int]], mode: int) -> Tuple[np.ndarray, int, int]:
    """(words uint32 [ceil(n_nodes / 32)], unknown count, status)"""
    n_nodes = len(row_ptr) - 1
    for q in seqs:
        if len(q) == 0 or len(q) > MAX_NEW_TOKENS:
            raise ValueError(f"a filter sequence holds 1 .. {MAX_NEW_TOKENS} tokens, not {len(q)}")
    paths = [walk(row_ptr, tok, nxt, start, q) for q in seqs]
    unknown = sum(p is None for p in paths)
    paths = [p for p in paths if p is not None]
    blocked = set()
    if mode == BLOCK:
        blocked = {p[-1] for p in paths}
        on_path = {}                                   # depth -> proper ancestors of an end node at that depth
        for p in paths:
            for d, node in enumerate(p[:-1]):
                on_path.setdefault(d, set()).add(node)
        for d in sorted(on_path, reverse=True):        # deepest first: below the start node the automaton is a tree
            for node in on_path[d]:
                ch = children(row_ptr, nxt, node)
                if ch and all(c in blocked for c in ch):
                    blocked.add(node)
        status = ERR_CONSTRAINT if int(start) in blocked else 0
    else:
        kept = {node for p in paths for node in p}
        ends = {p[-1] for p in paths}
        for node in kept - ends:
            blocked |= {c for c in children(row_ptr, nxt, node) if c not in kept}
        status = ERR_CONSTRAINT if not paths else 0
    words = np.zeros(n_words(n_nodes), np.uint32)
    for node in blocked:
        words[node >> 5] |= np.uint32(1) << np.uint32(node & 31)
    return words, unknown, status


def is_blocked(words: np.ndarray, node: int) -> bool:
    return bool((int(words[node >> 5]) >> (node & 31)) & 1)


def filtered_csr(row_ptr, tok, nxt, words: np.ndarray):
    """the automaton without the edges that lead to a blocked node (same node ids): what a filtered walk sees"""
    keep = np.asarray([not is_blocked(words, int(c)) for c in nxt], bool)
    rp = np.zeros(len(row_ptr), np.int32)
    for n in range(len(row_ptr) - 1):
        rp[n + 1] = rp[n] + int(keep[int(row_ptr[n]): int(row_ptr[n + 1])].sum())
    return rp, np.ascontiguousarray(tok[keep], np.int32), np.ascontiguousarray(nxt[keep], np.int32)


def csr_from_sequences(seqs: Sequence[Sequence[int]]):
    """(row_ptr, tok, nxt, prefixes): the trie of `seqs` as a CSR automaton, node ids breadth first from the root (node 0), children by
    ascending token; prefixes[n] = the token tuple that leads to node n"""
    tree = {}
    for q in seqs:
        level = tree
        for t in q:
            level = level.setdefault(int(t), {})
    prefixes, levels, row_ptr, tok, nxt = [()], [tree], [0], [], []
    i = 0
    while i < len(levels):
        for t in sorted(levels[i]):
            tok.append(t)
            nxt.append(len(levels))
            levels.append(levels[i][t])
            prefixes.append(prefixes[i] + (t,))
        row_ptr.append(len(tok))
        i += 1
    return np.asarray(row_ptr, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32), prefixes


def closure(fn, sep, exclude=None, allow=None):
    """A `prefix_allowed_tokens_fn(batch_id, sentence)` closure around the mask function `fn` that applies a filter the way a user of the
    reference would write it: the children `fn` allows, minus those whose subtree holds no permitted item.  `exclude` / `allow`: lists of
    generated-token sequences (items' code tokens; an item listed without its EOS also covers the EOS below it), every one of them a path
    `fn` knows.  Works on what `fn` returns only, so it serves the reference's own mask functions and this build's alike."""
    assert (exclude is None) != (allow is None)
    listed = [tuple(int(t) for t in q) for q in (exclude if exclude is not None else allow)]

    def suffix(sentence):
        s = [int(x) for x in (sentence.tolist() if hasattr(sentence, "tolist") else sentence)]
        m = len(sep)
        for end in range(m, len(s) + 1):
            if s[end - m: end] == list(sep):
                return s, s[end:]
        raise ValueError("separator not found")

    memo = {}

    def on_path(prefix) -> bool:
        return any(q[:len(prefix)] == prefix for q in listed)

    def alive(s, gen) -> bool:
        """does a permitted continuation exist at or below the generated prefix `gen` (`s` = the whole sentence that ends with it)?"""
        key = tuple(gen)
        if key not in memo:
            if exclude is not None:
                if key in listed:
                    memo[key] = False
                elif not on_path(key):                               # nothing listed below: untouched
                    memo[key] = True
                else:
                    ch = fn(0, s)
                    memo[key] = (not ch) or any(alive(s + [c], gen + [c]) for c in ch)
            else:                                                    # blocked iff the parent is in K \ E and the node is not in K
                parent = key[:-1]
                memo[key] = not (on_path(parent) and parent not in listed and not on_path(key))
        return memo[key]

    def wrapped(batch_id, sentence):
        s, gen = suffix(sentence)
        return [c for c in fn(batch_id, s) if alive(s + [c], gen + [c])]

    return wrapped
