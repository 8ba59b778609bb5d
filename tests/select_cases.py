"""Placed and tied inputs for the selection and LSE kernels of atspeed_amd/csrc/scan.hip, with their references.

numpy and torch on the CPU only; nothing here touches the library.  tests/test_select_cpu.py checks that every case is what it claims
(and that the geometry restated below is still the kernel's), tests/test_select_gpu.py runs the cases through the C ABI.

Value rule of the selection cases: logits and beam scores are dyadic rationals, multiples of 2^-6 below 2^10 in magnitude, and lse = 0
is passed in, so (logit - lse) + beam score is exact in fp32 and the expected scores are known bit for bit.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

# ------------------------------------------------------------------ geometry the placements rely on (scan.hip; drift guard in test_select_cpu.py)
THREADS = 1024                 # kScanThreads
SLOTS = 16                     # kCPT: candidate slots per thread
LANES = 64
LEAD = 4                       # kTopkLead
WAVES = THREADS // LANES
CHUNK = THREADS * SLOTS        # candidates of one expand / columns of one row_topk chunk
MAX_BEAMS = 64
LSE_U = 8                      # 16-byte loads per thread and chunk of lse_rows_kernel
NEG_INF = float("-inf")


def thread_of(c):
    return c % THREADS


def slot_of(c):
    return (c % CHUNK) // THREADS


def wave_of(c):
    return (c % THREADS) // LANES


def chunk_of(col):
    return col // CHUNK


def lse_threads(rows):
    return 256 if rows >= 1024 else 512


def lse_chunk(nt):
    return nt * LSE_U * 4


def lse_split(vocab, nt):
    """How lse_rows_kernel<nt> walks a row: full double-buffered chunks, floats of the partial chunk, scalars of the tail."""
    nv4 = vocab // 4
    n_full = nv4 // (nt * LSE_U)
    return {"n_full": n_full, "partial": (nv4 - n_full * nt * LSE_U) * 4, "tail": vocab - nv4 * 4}


# ------------------------------------------------------------------ references
def select_ref(scores, k):
    """The k best entries of `scores` (indexed by flat id) by (score desc, flat id asc); scores compare as VALUES (-0.0 == +0.0), -inf is
    no candidate; padded with -1.  The rule of oracle.beamsd_ref.topk_desc_stable, restated over numpy."""
    s = np.asarray(scores, np.float64).reshape(-1) + 0.0            # + 0.0: one zero
    ids = np.flatnonzero(s > -np.inf)
    best = ids[np.lexsort((ids, -s[ids]))][:k]
    out = np.full(k, -1, np.int64)
    out[: len(best)] = best
    return out


def lse_ref(x):
    """fp64 logsumexp of every row (a row of -inf gives -inf)."""
    return torch.logsumexp(torch.as_tensor(x).double(), -1).numpy()


def is_dyadic(a):
    """multiples of 2^-6 below 2^10 in magnitude (-inf allowed: a dead beam, a masked entry)"""
    a = np.asarray(a, np.float64)
    f = a[np.isfinite(a)]
    return bool(np.all(np.isneginf(a) | np.isfinite(a)) and np.all(f * 64 == np.round(f * 64)) and np.all(np.abs(f) < 1024))


def score32(logit, bscore):
    """what the kernels evaluate, in fp32: (logit - lse) + beam score with lse = 0"""
    return (np.asarray(logit, np.float32) - np.float32(0)) + np.asarray(bscore, np.float32)


# ------------------------------------------------------------------ atspeed_beam_expand_prune over hand-made automata
@dataclass
class ExpandCase:
    name: str
    vocab: int
    k: int
    logits: np.ndarray            # [rows, vocab] fp32
    bscore: np.ndarray            # [rows] fp32, -inf = dead beam
    node: np.ndarray              # [rows] int32
    row_ptr: np.ndarray
    tok: np.ndarray
    nxt: np.ndarray
    n_nodes: int
    claims: dict = field(default_factory=dict)

    @property
    def rows(self):
        return len(self.bscore)

    def children(self, r):
        n = int(self.node[r])
        return self.tok[self.row_ptr[n]: self.row_ptr[n + 1]]

    def candidates(self):
        """(row, token) of every candidate in expand order: live rows in order, children of the row's node ascending.  Candidate c sits on
        thread c % 1024, slot c // 1024."""
        r = [np.full(len(self.children(q)), q) for q in range(self.rows) if self.bscore[q] > NEG_INF]
        t = [self.children(q) for q in range(self.rows) if self.bscore[q] > NEG_INF]
        return (np.concatenate(r), np.concatenate(t)) if r else (np.zeros(0, np.int64), np.zeros(0, np.int64))

    def flat_scores(self):
        """fp32 score of every flat id r * vocab + t, -inf where (r, t) is no candidate"""
        out = np.full(self.rows * self.vocab, NEG_INF, np.float32)
        r, t = self.candidates()
        out[r * self.vocab + t] = score32(self.logits[r, t], self.bscore[r])
        return out

    def expected(self):
        fs = self.flat_scores()
        flat = select_ref(fs, self.k)
        live = flat >= 0
        f = flat[live]
        parent, token = f // self.vocab, f % self.vocab
        node = []
        for p, t in zip(parent, token):
            n = int(self.node[p])
            e = int(self.row_ptr[n] + np.searchsorted(self.children(p), t))
            node.append(int(self.nxt[e]))
        return {"flat": flat.tolist(), "parent": parent.tolist(), "token": token.tolist(), "node": node, "score": fs[f]}


def _background(n, seed):
    """n distinct losing scores in [-100 - n/64, -100]"""
    return -100.0 - np.random.default_rng(seed).permutation(n) / 64.0


def _winner_scores(n, seed):
    """n distinct winning scores in [100, 100 + n/64), in no particular order"""
    return 100.0 + np.random.default_rng(seed).permutation(n) / 64.0


def _beam_scores(rows, dead=()):
    bs = -0.25 - ((np.arange(rows) * 37) % 129) / 64.0
    bs[list(dead)] = NEG_INF
    return bs


def _expand_case(name, degs, sc, k, claims, dead=(), vocab=1000, seed=1):
    """Row r sits on its own node r with degs[r] children (a seeded ascending subset of the vocabulary); sc[c] is the intended score of
    candidate c in expand order (live rows only).  Tokens the node does not allow carry logit 900, the children of a dead row 500: neither
    may ever be picked."""
    rng = np.random.default_rng(seed)
    rows = len(degs)
    n_nodes = max(rows + 3, 16)                                          # a few empty nodes: out_node has somewhere to point
    kids = [np.sort(rng.choice(vocab, d, replace=False)) for d in degs]
    row_ptr = np.zeros(n_nodes + 1, np.int64)
    row_ptr[1: rows + 1] = np.cumsum(degs)
    row_ptr[rows + 1:] = row_ptr[rows]
    tok = np.concatenate(kids)
    nxt = (np.arange(len(tok)) * 5 + 1) % n_nodes
    bs = _beam_scores(rows, dead)
    logits = np.full((rows, vocab), 900.0)
    c = 0
    for r in range(rows):
        if r in dead:
            logits[r, kids[r]] = 500.0
            continue
        logits[r, kids[r]] = np.asarray(sc[c: c + degs[r]]) - bs[r]
        c += degs[r]
    assert c == len(sc), (name, c, len(sc))
    return ExpandCase(name, vocab, k, logits.astype(np.float32), bs.astype(np.float32), np.arange(rows, dtype=np.int32),
                      row_ptr.astype(np.int32), tok.astype(np.int32), nxt.astype(np.int32), n_nodes, claims)


def _place(total, winners, seed):
    """background scores with the candidates `winners` raised to distinct winning scores"""
    sc = _background(total, seed)
    sc[np.asarray(winners)] = _winner_scores(len(winners), seed + 1)
    return sc


@functools.lru_cache(maxsize=None)
def expand_cases():
    cases = []
    # k below, at and just above the lead count, and at the beam limit: one node of 256 children (waves 0-3, slot 0); the five best sit in
    # wave 2, so at k = 5 the k-th key is the fifth of its wave while the four above it are lead keys
    for k in (1, 2, 3, 4, 5, 63, 64):
        sc = _background(256, 10)
        sc[[131, 145, 158, 172, 191]] = [103.0, 101.5, 104.25, 100.0, 102.0]
        cl = {"live": 256, "winner_slots": [0]}
        if k <= 5:
            cl["winner_waves"] = [2]
        cases.append(_expand_case(f"k_sweep[{k}]", [256], sc, k, cl))
    full = [256] * 64
    # all 64 winners in one wave, one per lane, over all slots
    for w in (0, 7, 15):
        win = [((5 * l + w) % SLOTS) * THREADS + LANES * w + l for l in range(LANES)]
        cases.append(_expand_case(f"one_wave[{w}]", full, _place(CHUNK, win, 20 + w), 64,
                                  {"live": CHUNK, "winner_waves": [w], "max_per_thread": 1, "winner_slots": list(range(SLOTS))}))
    # exactly four winners per wave: the 64 lead keys ARE the answer, the bound equals the 64th key
    win = [((3 * w + i) % SLOTS) * THREADS + LANES * w + (17 * i + 5 * w) % LANES for w in range(WAVES) for i in range(LEAD)]
    cases.append(_expand_case("four_per_wave", full, _place(CHUNK, win, 30), 64,
                              {"live": CHUNK, "per_wave": [4] * WAVES, "bound_is_kth": True}))
    # the 64th key is the FIFTH of its wave and the 63 above it are all lead keys (wave 14 holds three winners, wave 15 five): the bound
    # lies below the k-th key, and a bound one rank too high loses it
    win = [((3 * w + i) % SLOTS) * THREADS + LANES * w + (17 * i + 5 * w) % LANES
           for w in range(WAVES) for i in range({14: 3, 15: 5}.get(w, 4))]
    sc = _place(CHUNK, win, 31)
    w15 = [c for c in win if wave_of(c) == 15]
    sc[w15[2]] = 99.0                                                    # lowest winner: the fifth key of wave 15
    cases.append(_expand_case("kth_is_fifth_of_wave", full, sc, 64,
                              {"live": CHUNK, "per_wave": [4] * 14 + [3, 5], "bound_is_kth": False, "kth_wave_rank": 4}))
    # fewer lead keys than k: no bound at all
    cases.append(_expand_case("no_bound", [2, 3], np.array([-3.0, 4.5, 1.25, -7.0, 2.0]), 20, {"live": 5, "n": 5}))
    # one thread owns two winners (slots s and s + 1)
    win = [c + d for c in (5, 70, 700, 1023) for d in (0, THREADS)]
    cases.append(_expand_case("two_slots_one_thread", [256] * 10, _place(2560, win, 40), 8,
                              {"live": 2560, "max_per_thread": 2, "winner_slots": [0, 1], "winner_waves": [0, 1, 10, 15]}))
    # every slot of every thread taken; the winners in the last slot, the very last candidate among them
    win = [15 * THREADS + t for t in list(range(0, 1024, 27)) + [1023]]
    cases.append(_expand_case("full", full, _place(CHUNK, win, 50), len(win), {"live": CHUNK, "winner_slots": [15], "last_candidate_wins": True}))
    # one score everywhere: flat ids ascending.  k = 40 < 50 children: row 0's lowest tokens; 25 children: all of row 0, then row 1's first
    cases.append(_expand_case("plateau", [50] * 20, np.full(1000, 2.5), 40, {"live": 1000, "tie_ranks": list(range(40)), "winner_rows": [0]}))
    cases.append(_expand_case("plateau_two_rows", [25] * 20, np.full(500, 2.5), 40,
                              {"live": 500, "tie_ranks": list(range(40)), "winner_rows": [0, 1]}))
    # k-th and (k+1)-th equal, in different rows: the lower flat id (row 2) wins although row 5's token is the smaller one
    degs = [100] * 8
    sc = _background(800, 60)
    top = [30, 410, 777, 150, 620, 333, 55, 701, 505]                     # nine distinct winners ...
    sc[top] = 100.0 + np.arange(9, 0, -1)
    sc[2 * 100 + 99] = 90.0                                               # ... the tenth: row 2's last child
    sc[5 * 100 + 0] = 90.0                                                # and, equal, row 5's first
    cases.append(_expand_case("tie_at_k", degs, sc, 10, {"live": 800, "tie_ranks": [9], "kth_row": 2, "next_row": 5}))
    # two equal scores inside the top k in different waves and slots
    sc = _background(2048, 70)
    sc[[300, 1500, 9, 2047, 600, 1100]] = [110.0, 109.0, 108.0, 105.0, 104.0, 103.0]
    sc[70] = 107.0                                                        # wave 1, slot 0 (row 0)
    sc[THREADS + 900] = 107.0                                             # wave 14, slot 1 (row 7)
    cases.append(_expand_case("tie_across_waves", [256] * 8, sc, 8, {"live": 2048, "tie_ranks": [3], "tie_waves": [1, 14], "tie_slots": [0, 1]}))
    # dead beams between live ones: their children are no candidates and take no candidate index
    degs = [100 + 13 * r for r in range(12)]
    dead = (0, 3, 4, 9, 11)
    live_degs = [d for r, d in enumerate(degs) if r not in dead]
    off = np.concatenate(([0], np.cumsum(live_degs)))
    win = [int(off[i]) for i in range(len(live_degs))] + [int(off[i + 1]) - 1 for i in range(len(live_degs))] + [1024, 1023]
    cases.append(_expand_case("dead_rows", degs, _place(int(off[-1]), win, 80), 16,
                              {"live": int(off[-1]), "dead_rows": list(dead), "n": 16}, dead=dead))
    # a single live row, the last of 64
    cases.append(_expand_case("one_live_of_64", full, _place(256, [0, 100, 255, 64, 63, 128], 90), 20,
                              {"live": 256, "dead_rows": list(range(63)), "winner_rows": [63]}, dead=tuple(range(63))))
    return cases


# ------------------------------------------------------------------ atspeed_row_topk / atspeed_beam_expand_prune_free
V3 = 2 * CHUNK + 5             # the smallest vocabulary with three chunks (the last one ragged)
V1 = CHUNK                     # exactly one


@dataclass
class TopkCase:
    name: str
    vocab: int
    k: int
    rows: np.ndarray              # [n, vocab] fp32
    claims: dict = field(default_factory=dict)

    def expected(self):
        out = np.full((len(self.rows), MAX_BEAMS), -1, np.int64)
        for r, row in enumerate(self.rows):
            out[r, : self.k] = select_ref(row, self.k)
        return out


def _row_bg(vocab):
    col = np.arange(vocab)
    return -200.0 - ((col * 7919) % 8192) / 64.0


def _boundary_cols(vocab):
    """both sides of every chunk boundary and the last column; a vocabulary of one chunk has slot boundaries (columns 1023 | 1024) instead"""
    if vocab > 2 * CHUNK:
        return [CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, vocab - 1]
    return [THREADS - 1, THREADS, vocab - THREADS - 1, vocab - THREADS, vocab - 1]


def _topk_rows(vocab):
    """name -> (row, k, claims); shared by the row_topk cases and the rows of the mask-free expand"""
    last = chunk_of(vocab - 1)
    chunks = list(range(last + 1))
    rows = {}
    r = _row_bg(vocab)
    b = _boundary_cols(vocab)
    r[b] = 50.0 + ((np.arange(len(b)) * 3) % len(b))                     # not monotone in the column
    rows["boundary"] = (r, 5, {"winner_col_set": b})
    for k in (5, 20):
        r = _row_bg(vocab)
        r[vocab - 5:] = [7.0, 9.0, 8.0, 6.0, 10.0]
        rows[f"last_chunk_only[{k}]"] = (r, k, {"best_cols": list(range(vocab - 5, vocab)), "best_chunks": [last]})
    col = np.arange(vocab)
    rows["ramp_desc"] = (500.0 - col / 64.0, 20, {"winner_cols": list(range(20))})
    rows["ramp_asc"] = (-100.0 + col / 64.0, 20, {"winner_col_set": list(range(vocab - 20, vocab)), "winner_chunks": sorted({chunk_of(vocab - 20), last})})
    rows["all_equal"] = (np.full(vocab, -3.5), 20, {"winner_cols": list(range(20)), "tie_ranks": list(range(20))})
    rows["all_equal[64]"] = (np.full(vocab, -3.5), 64, {"winner_cols": list(range(64)), "tie_ranks": list(range(64))})
    k = 6
    r = _row_bg(vocab)
    if last == 2:
        pl = [3, 1030, CHUNK - 1, CHUNK, CHUNK + 2048 + 7, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 2, vocab - 1]
    else:
        pl = [3, 1030, 2048 + 7, 5000, 8191, 8192, 12000, vocab - 2, vocab - 1]
    r[pl] = 12.0
    rows["plateau"] = (r, k, {"winner_cols": pl[:k], "plateau_chunks": chunks, "tie_ranks": list(range(k))})
    r = np.full(vocab, NEG_INF)
    ff = [vocab - 5, vocab - 3, vocab - 1]
    r[ff] = [1.0, 3.0, 2.0]
    rows["few_finite"] = (r, 20, {"finite": 3, "winner_chunks": [last]})
    rows["all_neg_inf"] = (np.full(vocab, NEG_INF), 20, {"finite": 0})
    # new keys and carried keys meet inside wave 0: the carried j-th best rides on thread j, the later chunk's winners on threads < k
    k = 20
    r = _row_bg(vocab)
    first = [17 * i + 3 + THREADS * (i % SLOTS) for i in range(k)]        # chunk 0, all over it
    r[first] = 60.0 + 2.0 * np.arange(k)                                   # 60, 62, ..
    later = [last * CHUNK + t for t in range(k)] if last else []
    if vocab == V3:
        later = [CHUNK + t for t in range(0, k, 2)] + [2 * CHUNK + t for t in range(5)]
    r[later] = 61.0 + 2.0 * np.arange(len(later))                          # 61, 63, ..: interleaved with the carried ones
    rows["wave0_competition"] = (r, k, {"later_threads_below_k": True} if later else {})
    return rows


@functools.lru_cache(maxsize=None)
def topk_cases():
    cases = []
    for vocab in (V3, V1):
        for name, (row, k, claims) in _topk_rows(vocab).items():
            cases.append(TopkCase(f"{name}-V{vocab}", vocab, k, row[None].astype(np.float32), claims))
        # +0.0 at a higher column than -0.0, everything else negative: equal values, the lower column first.  Row 1: the same across a chunk
        # boundary where there is one, where the carried -0.0 meets a new +0.0
        rows = np.tile(-1.0 - (np.arange(vocab) % 512) / 64.0, (2, 1))
        rows[0, 3], rows[0, 10] = -0.0, 0.0
        hi = CHUNK + 7 if vocab > CHUNK + 7 else 5000
        rows[1, 5], rows[1, hi] = -0.0, 0.0
        cases.append(TopkCase(f"signed_zeros-V{vocab}", vocab, 2, rows.astype(np.float32), {"zeros": [[3, 10], [5, hi]]}))
    return cases


@dataclass
class FreeCase:
    name: str
    vocab: int
    k: int
    rows: np.ndarray              # [n, vocab] fp32
    bscore: np.ndarray            # [n] fp32
    claims: dict = field(default_factory=dict)

    def flat_scores(self):
        return score32(self.rows, self.bscore[:, None]).reshape(-1)

    def expected(self):
        fs = self.flat_scores()
        flat = select_ref(fs, self.k)
        f = flat[flat >= 0]
        return {"flat": flat.tolist(), "parent": (f // self.vocab).tolist(), "token": (f % self.vocab).tolist(), "score": fs[f]}


@functools.lru_cache(maxsize=None)
def free_cases():
    cases = []
    for vocab in (V3, V1):
        t = _topk_rows(vocab)
        names = ["boundary", "last_chunk_only[20]", "wave0_competition", "all_equal", "plateau", "few_finite", "all_neg_inf", "ramp_asc"]
        rows = np.stack([t[n][0] for n in names])
        # row 3 is dead; the others are shifted so that their best entries interleave: 52.5 .. 48.5 (row 0), 50, 48, 46 (row 2), nine times
        # 47.5 (row 4), 47.25 and 46.25 (row 5); the ramp of row 7 starts at 43.5, just below the 20th
        bs = np.array([-1.5, -0.75, -48.0, NEG_INF, 35.5, 44.25, -1.0, 43.5 - float(rows[7].max())])
        # a tie between a token of row 0 and a token of row 1: row 1 gets an entry that scores what row 0's best does
        rows[1, 777] = float(rows[0].max()) + bs[0] - bs[1]
        for k in (5, 20):
            ties = [0] if k == 5 else [0] + list(range(8, 16))
            cases.append(FreeCase(f"mixed[{k}]-V{vocab}", vocab, k, rows.astype(np.float32), bs.astype(np.float32),
                                  {"dead_rows": [3], "tie_ranks": ties, "tie_rows": [0, 1]}))
        # signed zeros with k = 1: the row's single candidate is what row_topk ranks first
        z = topk_cases()[[c.name for c in topk_cases()].index(f"signed_zeros-V{vocab}")].rows
        cases.append(FreeCase(f"signed_zeros-V{vocab}", vocab, 1, z, np.array([-1.5, -3.0], np.float32), {"zeros": True}))
    return cases


# ------------------------------------------------------------------ atspeed_lse_rows
LSE_FAMILIES = ("a", "b_full", "b_partial", "b_tail", "c", "d", "e", "f", "g")
LSE_CONST = 1.5                # family (c)
LSE_EXACT = ("c", "f", "g")    # closed-form answers: no measured factor


def lse_vocabs(nt):
    ch = lse_chunk(nt)
    out = []
    for n in (1, 2, 3):
        out += [(f"{n}c", n * ch), (f"{n}c+1", n * ch + 1), (f"{n}c+3", n * ch + 3), (f"{n}c+4", n * ch + 4), (f"{n}c+4nt+2", n * ch + 4 * nt + 2)]
    return out + [("c-1", ch - 1), ("7", 7), ("3", 3)]


@dataclass
class LseCase:
    name: str
    nt: int
    rows: int
    vocab: int
    ld: int
    families: list                # per row
    x: torch.Tensor               # [rows, ld] fp32, NaN in the padding columns
    ref: np.ndarray               # [rows] fp64
    claims: dict


def lse_case(vname, vocab, rows, families, seed=0):
    """Row r holds family families[r % len]:
    a N(0, 3); b_* the same with +40 at the first column of the last full chunk / inside the partial chunk / at V - 1 in the scalar tail
    (where the vocabulary has no such region the row stays family a); c every entry 1.5; d 1e4 + N(0, 1); e N(0, 3) with -inf on about
    30 % of the entries, on every load of thread 5 in chunk 0 and on the whole scalar tail; f -inf but one entry; g -inf."""
    nt = lse_threads(rows)
    ch = lse_chunk(nt)
    sp = lse_split(vocab, nt)
    ld = (vocab + 3) // 4 * 4 + (64 if vname == "2c+3" else 0)
    g = torch.Generator().manual_seed(1000 + seed)
    base = torch.randn(rows, vocab, generator=g)
    x = base * 3.0
    fam = [families[r % len(families)] for r in range(rows)]
    place = {"b_full": (sp["n_full"] - 1) * ch if sp["n_full"] else None,
             "b_partial": sp["n_full"] * ch + sp["partial"] // 2 if sp["partial"] else None,
             "b_tail": vocab - 1 if sp["tail"] else None}
    n4 = vocab - sp["tail"]
    thread5 = [4 * (u * nt + 5) + j for u in range(LSE_U) for j in range(4)] if sp["n_full"] else []
    for r, f in enumerate(fam):
        if f in place:
            if place[f] is None:
                fam[r] = "a"
            else:
                x[r, place[f]] = 40.0
        elif f == "c":
            x[r] = LSE_CONST
        elif f == "d":
            x[r] = 1.0e4 + base[r]
        elif f == "e":
            x[r, torch.rand(vocab, generator=g) < 0.3] = NEG_INF
            x[r, thread5] = NEG_INF
            x[r, n4:] = NEG_INF
        elif f == "f":
            cols = [c for c in (0, place["b_full"], place["b_partial"], place["b_tail"], (r * 7919) % vocab) if c is not None]
            keep = cols[(r // len(families)) % len(cols)]
            v = float(x[r, keep])
            x[r] = NEG_INF
            x[r, keep] = v
        elif f == "g":
            x[r] = NEG_INF
    full = torch.full((rows, ld), float("nan"))
    full[:, :vocab] = x
    claims = dict(sp, nt=nt, planted={k: v for k, v in place.items() if v is not None})
    return LseCase(f"nt{nt}-rows{rows}-{vname}", nt, rows, vocab, ld, fam, full, lse_ref(x), claims)


def lse_bound(ref):
    """the project's LSE tolerance (tests/test_kernels_gpu.py::test_lse_rows), per row"""
    return 2e-6 * np.abs(ref) + 1e-6


# ------------------------------------------------------------------ atspeed_lmhead_lse: a dominant logit in a chosen column
# (rows, vocab, hidden).  300 rows: the shape of a first batched forward; its tile grid is too thin for the fused epilogue, so the plain GEMM +
# atspeed_lse_rows answer.  2100 rows: the same vocabulary on the fused path, where tiles without a token of the automaton are never written.
LMHEAD_SHAPES = ((300, 5000, 256), (2100, 5000, 256))
LMHEAD_FUSED = {300: 0, 2100: 1}
LMHEAD_FSM_TOKENS = (2, 300, 4400, 4700, 4999)  # as test_lmhead_lse_fused_epilogue: tiles 0, 1, 17, 18 and the tail tile 19


def lmhead_plants(rows):
    """(row, column): a stored tile, tile 10 which the automaton does not store, the last column; first row, first row of the second
    256-row tile, last row"""
    return ((0, 0), (256, 2600), (rows - 1, 4999))


def plant_dominant(x, w, plants):
    """w with row `col` replaced by x[r] * (40 / |x[r]|^2) for every (r, col): row r's logit at col is then about 40"""
    w = w.clone()
    for r, col in plants:
        xr = x[r].double()
        w[col] = (xr * (40.0 / float(xr @ xr))).to(w.dtype)
    return w
