"""Inputs for the sampled beam step and the two verify walks of atspeed_amd/csrc/scan.hip (atspeed_beam_sample_step, atspeed_verify_walk).

numpy on the CPU only; nothing here touches the library.  tests/walk_ref.py is the reference, tests/test_walk_cpu.py checks that every case
is what it claims, tests/test_walk_gpu.py runs the cases through the C ABI.

Two families.
  placed   the value rule of tests/select_cases.py: logits and beam scores are multiples of 2^-6 below 2^10, lse = 0 is passed in and the
           temperature is 1, 0.5 or 2, so every tempered cumulative score is exact in fp32 and scores are compared bit for bit.  Automata are
           hand-made layered graphs (layered_fsm).
  natural  random fp32 logits, lse = the fp32 rounding of the true fp64 LSE, one temperature that is no power of two (1.3).  The same inputs
           go through the oracle (tests/test_walk_cpu.py).
A case names the branches it exists for in `claims`; the seeds below were searched (search() at the end of this file) until the reference alone
reaches those branches with every decision margin at or above 1e-4.  The draft side of a walk -- blocks and tables -- is made by the
reference's own step on the draft's logits, so a walk's inputs are what a round would hand it.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from tests import walk_ref as R

NEG = -np.inf
NAT_LO, NAT_VOCAB = 32000, 32200      # natural family: item tokens as the oracle knows them
MARGIN = 1e-4                  # tests/test_bssd_gpu.py's figure for "above fp32 noise"
STEP_BRANCHES = ("multi_slot", "full_16384", "dead_beam", "blocked_edge", "cutoff", "filter_drop", "short_block", "table")
SAMPLED_WALK_BRANCHES = ("all_accepted", "bonus", "dnext", "n_acc_eq_k", "n_acc_gt_k", "subset_reorders", "reject_some", "reject_none_accepted",
                         "zero_mass_fallback", "short_draft_block", "resample_short", "short_result", "parent_not_hit", "draft_pick_removed",
                         "cutoff", "blocked_edge_mid_list", "dl0", "hit_not_identity")
GREEDY_WALK_BRANCHES = ("all_accepted", "reject_step0", "reject_middle", "target_none", "tie", "signed_zero", "target_order_differs",
                        "hit_not_identity", "staged_gaps", "pending", "free_mode", "vtrace", "dl0", "dnext")
OUTPUT_BRANCHES = ("vis_straddle", "distinct_parent_vis", "seq_full", "k64")


# ------------------------------------------------------------------ automata
def layered_fsm(vocab, layers, seed, n_sink=6, tok_lo=0):
    """layers[d] = the degrees of the nodes of depth d.  Child j of node x of layer d carries a token of a seeded ascending subset of the
    vocabulary (of [tok_lo, vocab): the oracle's one-step search keeps item tokens, ids >= 32000, only) and leads to node (7 j + x) mod |layer d + 1| of the next layer; below the last layer lie n_sink nodes without children."""
    rng = np.random.default_rng(seed)
    base = np.concatenate(([0], np.cumsum([len(L) for L in layers]))).astype(int)
    n_nodes = int(base[-1]) + n_sink
    row_ptr, tok, nxt = [0], [], []
    for d, L in enumerate(layers):
        m_next = len(layers[d + 1]) if d + 1 < len(layers) else n_sink
        for x, deg in enumerate(L):
            tok += (tok_lo + np.sort(rng.choice(vocab - tok_lo, deg, replace=False))).tolist()
            nxt += [int(base[d + 1]) + (7 * j + x) % m_next for j in range(deg)]
            row_ptr.append(len(tok))
    row_ptr += [len(tok)] * n_sink
    return R.Fsm(np.asarray(row_ptr, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32), n_nodes, vocab), base


def path_to(fsm, start, target):
    """tokens of a path start -> target (breadth first)"""
    prev = {start: None}
    todo = [start]
    while todo:
        n = todo.pop(0)
        if n == target:
            out = []
            while prev[n] is not None:
                n, t = prev[n]
                out.append(t)
            return out[::-1]
        for e in range(*fsm.kids(n)):
            c = int(fsm.nxt[e])
            if c not in prev:
                prev[c] = (n, int(fsm.tok[e]))
                todo.append(c)
    raise ValueError((start, target))


def _block(fsm, nodes):
    """block `nodes` for the case's one user; mask_seqs = the sequences from node 0 that atspeed_node_masks_create takes (block mode)"""
    fsm.blocked = np.zeros(fsm.n_nodes, bool)
    fsm.blocked[list(nodes)] = True
    return [path_to(fsm, 0, n) for n in nodes]


def dyadic(rng, shape, lo, hi):
    """multiples of 2^-6 in [lo, hi)"""
    return (rng.integers(int(lo * 64), int(hi * 64), shape) / 64.0).astype(np.float32)


def true_lse32(x):
    x = x.astype(np.float64)
    m = x.max(-1)
    return (m + np.log(np.exp(x - m[..., None]).sum(-1))).astype(np.float32)


# ------------------------------------------------------------------ the sampled step
@dataclass
class StepCase:
    name: str
    family: str
    fsm: R.Fsm
    logits: np.ndarray
    lse: np.ndarray
    bscore: np.ndarray
    node: np.ndarray
    k: int
    T: float
    seed: int
    round: int
    step: int
    cutoff: Optional[np.ndarray] = None
    filter_ids: bool = False
    mask_seqs: Optional[list] = None
    claims: tuple = ()

    @property
    def sub(self):
        return R.rng_sub(self.seed, R.P_STEP, self.round, self.step, 1)      # as HashRng.begin(P_STEP, round, step, model 1)

    def expected(self, rules=()):
        return R.step_sample_ref(self.fsm, self.logits, self.lse, self.bscore, self.node, self.k, self.T, self.sub, self.cutoff,
                                 self.filter_ids, rules)


def step_case(name, seed, degs, k, T, claims, vocab=300, dead=(), block=(), cut=None, filter_min=0, natural=False):
    rng = np.random.default_rng(seed)
    n = len(degs)
    vocab = NAT_VOCAB if natural else vocab
    fsm, base = layered_fsm(vocab, [list(degs), [3] * 11], 1000 + seed, tok_lo=NAT_LO if natural else 0)
    mask_seqs = _block(fsm, [int(base[1]) + b for b in block]) if block else None
    if filter_min or natural:
        fsm.filter_min, fsm.filter_eos = filter_min or NAT_LO, 2
    if natural:
        logits = (rng.standard_normal((n, vocab)) * 2.0).astype(np.float32)
        lse = true_lse32(logits)
        bscore = (-rng.random(n) * 3.0).astype(np.float32)
    else:
        logits = dyadic(rng, (n, vocab), -2, 2)
        lse = np.zeros(n, np.float32)
        bscore = dyadic(rng, n, -3, 0)
    bscore[list(dead)] = NEG
    cutoff = None
    if cut is not None:
        cutoff = np.full(n, NEG, np.float32)
        cutoff[::2] = cut                                     # every other row has a cutoff
    return StepCase(name, "natural" if natural else "placed", fsm, logits, lse, bscore, np.arange(n, dtype=np.int32), k, T, seed, 3, 1, cutoff,
                    filter_min > 0 or natural, mask_seqs, tuple(claims))


@functools.lru_cache(maxsize=None)
def step_cases():
    c = [
        step_case("small", 11, [9, 14, 5], 5, 1.0, ("table",)),
        # more than 1024 candidates: a thread holds more than one slot; a dead beam in the middle takes no candidate index
        step_case("multi_slot_dead", 23, [256] * 10, 8, 0.5, ("multi_slot", "dead_beam", "table"), dead=(4,)),
        # every slot of every thread: 64 rows x 256 children
        step_case("full_16384", 31, [256] * 64, 64, 2.0, ("multi_slot", "full_16384", "table")),
        # edges into blocked nodes, rows with a cutoff, and the id filter dropping picks: the block shrinks, -1 at its end
        step_case("masked_cut_filtered", 40, [40, 33, 40, 25, 40, 18], 12, 1.0, ("blocked_edge", "cutoff", "filter_drop", "short_block", "table"),
                  block=(1, 4, 8), cut=-0.75, filter_min=150),
        step_case("fewer_candidates_than_k", 51, [3, 2], 8, 2.0, ("short_block", "table")),
        step_case("natural", 60, [30, 41, 17, 28], 10, 1.3, ("table",), natural=True),
        step_case("natural_wide", 61, [200] * 12, 20, 1.3, ("multi_slot", "table"), natural=True),
    ]
    return c


# ------------------------------------------------------------------ walks
@dataclass
class WalkCase:
    name: str
    family: str
    w: R.WalkIn
    claims: tuple
    draft: list = field(default_factory=list)        # sampled: per draft step dict(logits, lse, bscore, node, k, sub, filter_ids)
    mask_seqs: Optional[list] = None
    draft_margins: dict = field(default_factory=dict)
    aux: dict = field(default_factory=dict)

    def expected(self, rules=()):
        return R.walk_ref(self.w, rules)


def _cur_rows(rng, n_prompt, nb, dl, dk, W, slot0):
    n0 = n_prompt + nb
    rows = n0 + dl * dk
    ids = rng.integers(0, 1000, rows).astype(np.int32)
    pos = np.concatenate((np.arange(n_prompt), np.full(nb, n_prompt), np.repeat(n_prompt + 1 + np.arange(dl), dk))).astype(np.int32)
    slot = (slot0 + np.arange(rows)).astype(np.int32)
    vis = np.zeros((rows, W), np.uint64)
    lim = min(slot0, 64 * W)                                 # bits of slots below slot0 only: a new row's own bit is never set beforehand
    for r in range(rows):
        bits = int(rng.integers(1, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 62)
        bits &= (1 << lim) - 1
        for wd in range(W):
            vis[r, wd] = np.uint64((bits >> (64 * wd)) & 0xFFFFFFFFFFFFFFFF)
    return dict(ids=ids, pos=pos, slot=slot, vis=vis), n0


def _seq(rng, n):
    return rng.integers(1, 30000, (n, R.LMAX)).astype(np.int32)


def _greedy_step(fsm, logits, lse, bscore, node, k, vocab=0, row_cand=None, n_row_cand=0):
    """the draft's greedy step: the k best candidates by (score desc, flat id asc)"""
    n = len(bscore)
    rows = np.arange(n)
    c = R.expand(fsm, node, rows, rows, bscore.astype(np.float64), logits, lse, 1.0, None, False, R.Rec(), vocab, row_cand, n_row_cand)
    ids = np.flatnonzero((c["flat"] >= 0) & (c["sc"] > NEG))
    sc = c["sc"][ids] + 0.0
    order = np.lexsort((c["flat"][ids], -sc))[:k]
    V = fsm.vocab if fsm is not None else vocab
    picks = []
    for q in order:
        fl = int(c["flat"][ids][q])
        nd = 0
        if fsm is not None:
            e = fsm.edge(node[fl // V], fl % V)
            nd = int(fsm.nxt[e])
        picks.append((float(sc[q]), fl // V, fl % V, nd, fl))
    picks += [R.NONE_PICK] * (k - len(picks))
    return R._pick_arrays(picks)


def _row_topk(logits, kk):
    """atspeed_row_topk: the kk best columns of every row (value desc, column asc), padded with -1 to MAXB"""
    out = np.full((len(logits), R.MAXB), -1, np.int32)
    for r, row in enumerate(logits):
        ok = np.flatnonzero(row > NEG)
        best = ok[np.lexsort((ok, -row[ok].astype(np.float64)))][:kk]
        out[r, : len(best)] = best
    return out


def walk_case(name, seed, claims, *, sample, nb, k, dk, dl, layers, vocab=200, T=1.0, tnoise=0.0, noise_steps=None, filter_min=0, cut=None,
              block=(), W=1, slot0=8, gen_len0=1, n_prompt=3, gaps=None, blocks_ready=None, free=False, vtrace=False, natural=False,
              grid=64, zeros=False, rnd=2):
    """One walk.  The draft runs dl steps from the nb round beams on its own logits (sampled: reference step with tables; greedy: dk best);
    the target's logits are the draft's plus `tnoise` (per step: noise_steps[i]) times a dyadic disturbance, laid out block after block at
    blk_row0 (gaps = extra rows in front of every draft block: a staged layout)."""
    rng = np.random.default_rng(seed)
    fsm, base, mask_seqs = None, None, None
    vocab = NAT_VOCAB if natural else vocab
    if natural:
        filter_min = NAT_LO
    if not free:
        fsm, base = layered_fsm(vocab, layers, 2000 + seed, tok_lo=NAT_LO if natural else 0)
        if block:
            mask_seqs = _block(fsm, [int(base[d]) + x for d, x in block])
        if filter_min:
            fsm.filter_min, fsm.filter_eos = filter_min, 2
    m0 = len(layers[0]) if not free else 1
    node0 = (np.arange(nb) % m0).astype(np.int32)

    def draw(shape):
        if natural:
            return (rng.standard_normal(shape) * 2.0).astype(np.float32)
        return (rng.integers(-2 * grid, 2 * grid + 1, shape) / float(grid)).astype(np.float32)

    bs0 = (-rng.random(nb) * 2.0).astype(np.float32) if natural else (-(rng.permutation(128)[:nb] + 1) / 64.0).astype(np.float32)
    blk = [dict(score=bs0, node=node0, flat=np.arange(nb, dtype=np.int32) * 0, seq=_seq(rng, nb))]
    dlog, dlse, draft, dtab, dmargins = [], [], [], [], {}
    n_row_cand = k if free else 0
    for i in range(dl):
        n = nb if i == 0 else dk
        lg = draw((n, vocab))
        if zeros and i == 0:                                  # a -0.0 / +0.0 pair on top of step 0: rows 0 and 1, their first children
            lg[:] = -np.abs(lg) - 1.0
            blk[0]["score"][:2] = (-0.0, 0.0)
            lg[0, fsm.tok[fsm.kids(node0[0])[0]]] = -0.0
            lg[1, fsm.tok[fsm.kids(node0[1])[0]]] = 0.0
        ls = true_lse32(lg) if natural else np.zeros(n, np.float32)
        bsc, nd = blk[i]["score"], blk[i]["node"]
        if sample:
            sub = R.rng_sub(seed, R.P_STEP, rnd, i, 1)
            o = R.step_sample_ref(fsm, lg, ls, bsc, nd, dk, T, sub, None, filter_min > 0)
            draft.append(dict(logits=lg, lse=ls, bscore=bsc, node=nd, k=dk, sub=sub, filter_ids=filter_min > 0, expected=o))
            dtab.append(dict(score=o["tab_score"], off=o["tab_off"], lse=o["tab_lse"]))
            for kind, v in o["margins"].items():
                dmargins[kind] = min(dmargins.get(kind, np.inf), v)
        elif free:
            o = _greedy_step(None, lg, ls, bsc, nd, dk, vocab, _row_topk(lg, dk), dk)
        else:
            o = _greedy_step(fsm, lg, ls, bsc, nd, dk)
        blk.append(dict(score=o["score"].astype(np.float32), node=o["node"], flat=o["flat"], parent=o["parent"], tok=o["tok"], seq=_seq(rng, dk)))
        dlog.append(lg); dlse.append(ls)
    # the target's rows: block i at blk_row0[i]
    sizes = [nb] + [dk] * dl
    row0, at = [], 0
    for i, s in enumerate(sizes):
        at += (gaps or 0) if i > 0 else 0
        row0.append(at)
        at += s
    tl = np.full((at, vocab), np.nan, np.float32)
    for i, s in enumerate(sizes):
        src = dlog[i] if i < dl else draw((s, vocab))
        amp = (noise_steps or {}).get(i, tnoise)
        dist = draw((s, vocab)) * np.float32(amp) if amp else 0
        if amp and not natural:
            dist = np.round(dist * 64.0) / 64.0                # the disturbance is dyadic too
        tl[row0[i]: row0[i] + s] = src + dist if amp else src      # (src + 0 would turn a -0.0 into +0.0)
    tlse = np.zeros(at, np.float32)
    if natural:
        fin = ~np.isnan(tl[:, 0])
        tlse[fin] = true_lse32(tl[fin])
    cutoff = None
    if cut is not None:
        cutoff = np.full(at, NEG, np.float32)
        cutoff[::2] = cut
    cur, n0 = _cur_rows(rng, n_prompt, nb, dl, dk, W, slot0)
    w = R.WalkIn(fsm=fsm, blk=blk, nb=nb, dl=dl, k=k, dk=dk, gen_len0=gen_len0, logits=tl, lse=tlse, blk_row0=row0,
                 blocks_ready=dl + 1 if blocks_ready is None else blocks_ready, cur=cur, n0=n0, W=W, sample=sample, T=T, seed=seed, round=rnd,
                 dtab=dtab, cutoff=cutoff, vtrace=vtrace, vocab=vocab if free else 0, row_cand=_row_topk(np.nan_to_num(tl, nan=NEG), k) if free else None,
                 n_row_cand=n_row_cand)
    return WalkCase(name, "natural" if natural else "placed", w, tuple(claims), draft, mask_seqs, dmargins, dict(dlog=dlog, dlse=dlse))


L3 = [[12, 9, 14, 11], [10, 13, 8, 12, 9, 11], [12, 10, 9, 13, 11], [9, 12, 10]]       # four layers: walks of up to three draft blocks


@functools.lru_cache(maxsize=None)
def sampled_walk_cases():
    S = dict(sample=True)
    return [
        # target == draft: every draft pick whose parent was kept is accepted (p >= q), so every step is accepted and the bonus draw follows
        walk_case("all_accepted", 103, ("all_accepted", "bonus", "dnext", "n_acc_gt_k", "subset_reorders", "hit_not_identity", "parent_not_hit", "seq_full"),
                  nb=4, k=4, dk=12, dl=2, layers=L3, gen_len0=14, **S),
        walk_case("n_acc_eq_k", 111, ("n_acc_eq_k",), nb=3, k=5, dk=8, dl=1, layers=L3, tnoise=0.5, T=0.5, **S),
        walk_case("reject_some", 120, ("reject_some", "hit_not_identity"), nb=3, k=5, dk=8, dl=2, layers=L3, noise_steps={1: 1.0}, T=2.0, **S),
        walk_case("reject_none_accepted", 131, ("reject_none_accepted",), nb=2, k=4, dk=4, dl=1, layers=L3, tnoise=4.0, **S),
        # step 0, target and draft given the same rows, the draft's block cut short by the id filter: every live pick is accepted (p == q),
        # fewer than k of them, and the residual has no mass
        walk_case("zero_mass_fallback", 140, ("zero_mass_fallback", "short_draft_block", "reject_some"), nb=3, k=6, dk=8, dl=1, layers=L3,
                  filter_min=120, **S),
        # a node of three children, k = 6: the resample runs out of candidates
        walk_case("resample_short", 151, ("resample_short", "short_result", "short_draft_block"), nb=1, k=6, dk=6, dl=1, layers=[[3], [4, 4, 4]],
                  tnoise=2.0, **S),
        walk_case("target_cutoff", 162, ("draft_pick_removed", "cutoff"), nb=3, k=4, dk=8, dl=1, layers=L3, cut=0.25, tnoise=0.25, **S),
        # a blocked edge in the middle of child lists, at a rejecting step: the residual reads the draft's table through child indices
        walk_case("blocked_mid_list", 174, ("blocked_edge_mid_list", "reject_some"), nb=3, k=5, dk=8, dl=1, layers=L3, block=((1, 2), (1, 4)),
                  tnoise=1.0, **S),
        walk_case("dl0", 180, ("dl0", "bonus"), nb=4, k=6, dk=6, dl=0, layers=L3, T=0.5, **S),
        walk_case("straddle", 190, ("vis_straddle", "distinct_parent_vis"), nb=3, k=6, dk=8, dl=1, layers=L3, tnoise=1.0, W=2, slot0=55, **S),
        walk_case("k64", 200, ("multi_slot",), nb=64, k=64, dk=64, dl=1, layers=[[40] * 8, [30] * 9, [5] * 4], vocab=128, W=4, slot0=20, **S),
        walk_case("natural_accept", 210, ("all_accepted", "bonus"), nb=3, k=3, dk=9, dl=2, layers=L3, T=1.3, natural=True, **S),
        walk_case("natural_reject", 220, ("reject_some",), nb=3, k=5, dk=8, dl=2, layers=L3, T=1.3, natural=True, noise_steps={1: 0.6}, **S),
    ]


@functools.lru_cache(maxsize=None)
def greedy_walk_cases():
    G = dict(sample=False)
    return [
        walk_case("all_accepted", 300, ("all_accepted", "dnext", "vtrace"), nb=3, k=4, dk=8, dl=3, layers=L3, vtrace=True, **G),
        walk_case("order_differs", 310, ("all_accepted", "target_order_differs", "hit_not_identity"), nb=3, k=4, dk=8, dl=2, layers=L3, tnoise=0.05, **G),
        walk_case("reject_step0", 320, ("reject_step0",), nb=3, k=4, dk=6, dl=2, layers=L3, tnoise=2.0, **G),
        walk_case("reject_middle", 333, ("reject_middle", "hit_not_identity"), nb=3, k=4, dk=8, dl=3, layers=L3, noise_steps={0: 0.05, 1: 2.0}, vtrace=True, **G),
        walk_case("target_none", 340, ("target_none", "short_result"), nb=1, k=6, dk=6, dl=1, layers=[[4], [3, 3, 3, 3]], **G),
        walk_case("ties", 350, ("tie", "all_accepted"), nb=3, k=5, dk=10, dl=2, layers=L3, grid=1, **G),
        walk_case("signed_zeros", 360, ("signed_zero", "tie"), nb=3, k=3, dk=6, dl=1, layers=L3, zeros=True, **G),
        walk_case("staged_gaps", 370, ("staged_gaps", "all_accepted"), nb=3, k=4, dk=8, dl=2, layers=L3, gaps=5, **G),
        walk_case("pending", 380, ("pending",), nb=3, k=4, dk=8, dl=2, layers=L3, blocks_ready=1, vtrace=True, **G),
        walk_case("free_mode", 390, ("free_mode", "all_accepted"), nb=3, k=4, dk=8, dl=2, layers=L3, free=True, **G),
        walk_case("dl0", 400, ("dl0",), nb=4, k=6, dk=6, dl=0, layers=L3, **G),
        walk_case("straddle_full", 410, ("vis_straddle", "distinct_parent_vis", "seq_full", "all_accepted"), nb=3, k=6, dk=8, dl=2, layers=L3,
                  W=2, slot0=39, gen_len0=14, **G),
        walk_case("k64", 420, ("multi_slot", "all_accepted"), nb=64, k=64, dk=64, dl=1, layers=[[40] * 8, [30] * 9, [5] * 4], vocab=128, W=4,
                  slot0=20, **G),
        walk_case("natural_accept", 430, ("all_accepted",), nb=3, k=4, dk=8, dl=2, layers=L3, natural=True, **G),
        walk_case("natural_reject", 440, ("reject_middle",), nb=3, k=4, dk=8, dl=2, layers=L3, natural=True, noise_steps={1: 1.5}, **G),
    ]


def case_margins(c, out):
    """every kind's smallest margin over the walk and the draft steps that made its inputs"""
    m = dict(out["margins"])
    for kind, v in getattr(c, "draft_margins", {}).items():
        m[kind] = min(m[kind], v)
    return m


def score_bound(logit, lse, T, score):
    """natural family: three fp32 roundings of (logit - lse) / T + score, doubled"""
    d = np.abs(np.asarray(logit, np.float64) - lse)
    return 2.0 * 2.0 ** -24 * (d + d / T + np.abs(score))


def search(build, seed0, tries=60):
    """how the seeds above were found: the first seed from seed0 on whose case reaches its claims with every margin at or above MARGIN in the
    reference alone.  `build(seed)` returns the case, e.g. lambda s: walk_case("reject_some", s, ("reject_some",), sample=True, ...)"""
    for seed in range(seed0, seed0 + tries):
        c = build(seed)
        out = c.expected()
        m = case_margins(c, out) if isinstance(c, WalkCase) else out["margins"]
        if all(b in out["branches"] for b in c.claims) and min(m.values()) >= MARGIN and out["status"] == 0:
            return seed
    return None
