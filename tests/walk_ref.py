"""fp64 restatement, over plain numpy arrays, of the decision half of atspeed_amd/csrc/scan.hip that only whole runs reached: one sampled
beam step (beam_step_body with `sample`) and one verify walk, greedy (verify_walk_body) or sampled (verify_sample_body), with the outputs
both walks share (verify_outputs).  It follows oracle/beamsd_ref.py::verify, oracle/beamsd_sample_ref.py::verify_sample / one_step_sample and
HashRng; tests/test_walk_cpu.py pins it to them on the natural cases of tests/walk_cases.py.

numpy on the CPU only (atspeed_amd.synth is numpy too); nothing here touches the library.  Every function returns, beside its arrays,
  margins   the smallest margin of every KIND of decision it took:
              gumbel   gap between neighbouring noisy keys where a draw cuts (an ordered draw: between all neighbours it returns in order)
              accept   |log(u q) - log p| of an accept test
              sign     |p - q| / max(p, q) wherever the sign of p - q decides (residual weights)
              greedy   score gap at a greedy cut or between ordered greedy picks, exact ties left out (they are decided by flat id)
  branches  the names of the branches it went through, in first-visit order.
`rules` names WRONG rules (tests/test_walk_cpu.py tells each apart from the right one; profiles/walk_mutations.txt predicts with them what a
mutated kernel gets wrong).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from atspeed_amd import synth

MAXB, LMAX, GAMMA, MAX_CAND = 64, 16, 8, 16384
NEG = -np.inf
P_STEP, P_ACCEPT, P_PERM, P_RESID, P_BONUS = 1, 2, 3, 4, 5
PENDING = -1
ERR_CAPACITY, ERR_CONSTRAINT, ERR_FILTERED = -3, -4, -6
NONE_PICK = (NEG, 0, 0, 0, -1)          # score, parent, token, node, flat of "no beam"

WRONG_RULES = ("accept_swapped", "residual_keeps_taken", "subset_largest", "fallback_uniform", "no_fallback", "vis_word0", "base_no_cnt")
# Rules that change no output (tests/test_walk_cpu.py::test_an_equivalent_rule_changes_nothing):
#   accept_strict  `u q < p` for `u q <= p` differs only where u q == p exactly.  u < 1, so that needs q == 0: a draft pick whose probability
#                  underflowed.  No case whose margins clear can hold one (the fp64 reference would not underflow where fp32 does).
#   draft_order, hit_by_flat
#                  the ORDER of the rows a step expands (the accepted set left in draft order in the sampled walk; hit[] ranked by flat id
#                  instead of draft position in the greedy one) is not observable: a candidate's flat id, its parent and its table index come
#                  from the row's position in the draft's block (brow), never from the row's index in the expand, the row's score travels with
#                  it (hit[] and sbh[] take the same rank), every selection is keyed by (score or noisy key, flat id), and the result of a
#                  step that goes on is overwritten by the step after it.  Only the order of the fp32 sums of a block LSE changes.
EQUIVALENT_RULES = ("accept_strict", "draft_order", "hit_by_flat")


# ------------------------------------------------------------------ the counter-based generator (common.h ats_rng_sub / ats_u01 / ats_gumbel)
def rng_sub(seed: int, purpose: int, rnd: int, step: int, tag: int) -> int:
    ctr = (purpose & 0xFF) | ((rnd & 0xFF) << 8) | ((step & 0xFF) << 16) | ((tag & 0xFF) << 24)
    return int(synth.hash_u32(np.array([ctr], dtype=np.uint64), int(seed) & 0xFFFFFFFF)[0])


def hashes(ids, sub: int) -> np.ndarray:
    return synth.hash_u32(np.asarray(ids, dtype=np.uint64), sub)


def u01(ids, sub: int) -> np.ndarray:
    return ((hashes(ids, sub) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(ids, sub: int) -> np.ndarray:
    return -np.log(-np.log(u01(ids, sub)))


# ------------------------------------------------------------------ inputs
@dataclass
class Fsm:
    row_ptr: np.ndarray
    tok: np.ndarray
    nxt: np.ndarray
    n_nodes: int
    vocab: int
    blocked: Optional[np.ndarray] = None      # [n_nodes] bool: an edge into a blocked node is no candidate
    filter_min: int = 0                       # post-top-k id filter of the one-step search: keep tok >= filter_min or tok == filter_eos
    filter_eos: int = -1

    def kids(self, node):
        return int(self.row_ptr[node]), int(self.row_ptr[node + 1])

    def edge(self, node, tok):
        e0, e1 = self.kids(node)
        j = int(np.searchsorted(self.tok[e0:e1], tok))
        return e0 + j if j < e1 - e0 and self.tok[e0 + j] == tok else -1


@dataclass
class WalkIn:
    """what atspeed_verify_walk is given; logits are dense [rows, vocab] here, the test pads them to a leading dimension"""
    fsm: Optional[Fsm]
    blk: list                                  # blocks 0 .. dl: dict(score f32 [n], node i32 [n], flat i32 [n], seq i32 [n, LMAX])
    nb: int
    dl: int
    k: int
    dk: int
    gen_len0: int
    logits: np.ndarray
    lse: np.ndarray
    blk_row0: list
    blocks_ready: int
    cur: dict                                  # ids, pos, slot i32 [rows], vis uint64 [rows, W]
    n0: int
    W: int
    sample: bool = False
    T: float = 1.0
    seed: int = 0
    round: int = 0
    dtab: list = field(default_factory=list)   # per draft step: dict(score f64 [cand], off i32 [rows + 1], lse f64)
    cutoff: Optional[np.ndarray] = None        # f32 per logits row
    vtrace: bool = False
    vocab: int = 0                             # free mode (fsm None)
    row_cand: Optional[np.ndarray] = None      # [rows, MAXB] i32
    n_row_cand: int = 0


class Rec:
    def __init__(self):
        self.margins = {"gumbel": np.inf, "accept": np.inf, "sign": np.inf, "greedy": np.inf}
        self.branches: List[str] = []

    def m(self, kind, v):
        self.margins[kind] = min(self.margins[kind], float(v))

    def b(self, name, cond=True):
        if cond and name not in self.branches:
            self.branches.append(name)


# ------------------------------------------------------------------ candidate enumeration (cand_rows / cand_at / expand_candidates / expand_and_select)
def expand(w_fsm, node, brow, lrow, bscore, logits, lse, T, cutoff, sampled, rec, vocab=0, row_cand=None, n_row_cand=0):
    """Candidates in expand order: live rows in order, children of the row's node ascending (free mode: the row's row_cand entries).
    Returns r, j, tok, flat, sc (fp64; -inf = absent: cut off, blocked, or a padded row_cand entry), off [rows + 1] and a status."""
    n = len(node)
    V = w_fsm.vocab if w_fsm is not None else vocab
    R, J, TK, SC = [], [], [], []
    off = np.zeros(n + 1, np.int64)
    status = 0
    for r in range(n):
        off[r + 1] = off[r]
        live = bscore[r] > NEG
        if w_fsm is not None:
            e0, e1 = w_fsm.kids(node[r])
            toks = w_fsm.tok[e0:e1].astype(np.int64)
        else:
            toks = row_cand[lrow[r], :n_row_cand].astype(np.int64)
        if live and len(toks) == 0:
            status = ERR_CONSTRAINT
        if not live:
            rec.b("dead_beam")
            continue
        off[r + 1] = off[r] + len(toks)
        ok = toks >= 0
        s = np.full(len(toks), NEG)
        s[ok] = (logits[lrow[r], toks[ok]].astype(np.float64) - float(lse[lrow[r]])) / T
        sc = s + float(bscore[r])
        if sampled and cutoff is not None:
            cut = s < float(cutoff[lrow[r]])
            rec.b("cutoff", bool(cut.any()))
            sc[cut] = NEG
        if w_fsm is not None and w_fsm.blocked is not None:
            blk = w_fsm.blocked[w_fsm.nxt[e0:e1]]
            rec.b("blocked_edge", bool(blk.any()))
            rec.b("blocked_edge_mid_list", len(blk) > 2 and bool(blk[1:-1].any()))
            sc[blk] = NEG
        sc[~ok] = NEG
        R.append(np.full(len(toks), r)); J.append(np.arange(len(toks))); TK.append(toks); SC.append(sc)
    if not R:
        z = np.zeros(0, np.int64)
        return dict(r=z, j=z, tok=z, flat=z, sc=np.zeros(0), off=off, status=status)
    r, j, tok, sc = np.concatenate(R), np.concatenate(J), np.concatenate(TK), np.concatenate(SC)
    if len(r) > MAX_CAND:
        status = ERR_CAPACITY
    rec.b("multi_slot", len(r) > 1024)
    rec.b("full_16384", len(r) == MAX_CAND)
    flat = np.asarray(brow, np.int64)[r] * V + tok
    flat[tok < 0] = -1
    return dict(r=r, j=j, tok=tok, flat=flat, sc=sc, off=off, status=status)


def sample_topn(flat, logw, n, sub, rec, ordered):
    """sample_topn: the n largest logw + Gumbel(hash(flat)) among the finite weights, key desc, flat id asc; -1 = none.  `ordered`: the
    caller keeps the order of the draws, so every gap between neighbours counts, not the cut alone"""
    ids = np.flatnonzero((flat >= 0) & (logw > NEG))
    keys = logw[ids] + gumbel(flat[ids], sub)
    order = np.lexsort((flat[ids], -keys))
    ks = keys[order]
    top = ks[: n + 1]
    if ordered and len(top) > 1:
        rec.m("gumbel", np.min(top[:-1] - top[1:]))
    elif len(ks) > n and n > 0:
        rec.m("gumbel", ks[n - 1] - ks[n])
    out = np.full(n, -1, np.int64)
    sel = flat[ids][order[:n]]
    out[: len(sel)] = sel
    return out


def lse64(v):
    v = v[v > NEG]
    if len(v) == 0:
        return NEG
    m = v.max()
    return m + np.log(np.sum(np.exp(v - m)))


def pick_of_flat(fl, fsm, node, brow, lrow, bscore, logits, lse, T, cutoff):
    """pick_of_flat: the pick with its TRUE tempered cumulative score; rows describe the expand it belongs to"""
    if fl < 0:
        return NONE_PICK
    parent, tok = int(fl) // fsm.vocab, int(fl) % fsm.vocab
    rr = [q for q in range(len(brow)) if brow[q] == parent]
    if not rr:
        return (NEG, parent, tok, 0, int(fl))
    r = rr[0]
    s = (float(logits[lrow[r], tok]) - float(lse[lrow[r]])) / T
    score = s + float(bscore[r])
    e = fsm.edge(node[r], tok)
    nd = int(fsm.nxt[e]) if e >= 0 else 0
    if e < 0 or (cutoff is not None and s < float(cutoff[lrow[r]])):
        score = NEG
    if e >= 0 and fsm.blocked is not None and fsm.blocked[fsm.nxt[e]]:
        score = NEG
    return (score, parent, tok, nd, int(fl))


# ------------------------------------------------------------------ one sampled beam step
def step_sample_ref(fsm, logits, lse, bscore, node, k, T, sub, cutoff=None, filter_ids=False, rules=()):
    """beam_step_body with a.sample (one_step_sample of the oracle): k draws without replacement from softmax of the tempered cumulative
    scores, the draft's table, the post-top-k id filter.  Outputs of k entries; table = every candidate in expand order."""
    rec = Rec()
    n = len(bscore)
    rows = np.arange(n)
    c = expand(fsm, node, rows, rows, bscore, logits, lse, T, cutoff, True, rec)
    rec.b("table")
    draws = sample_topn(c["flat"], c["sc"], k, sub, rec, ordered=True)
    picks = [pick_of_flat(f, fsm, node, rows, rows, bscore, logits, lse, T, cutoff) for f in draws]
    status = c["status"]
    if filter_ids:
        ok = [p[4] >= 0 and (p[2] >= fsm.filter_min or p[2] == fsm.filter_eos) for p in picks]
        had = sum(p[4] >= 0 for p in picks)
        rec.b("filter_drop", had > sum(ok))
        if had > 0 and sum(ok) == 0:
            status = ERR_FILTERED
        picks = [p for p, o in zip(picks, ok) if o] + [NONE_PICK] * (k - sum(ok))
    rec.b("short_block", any(p[4] < 0 for p in picks))
    out = _pick_arrays(picks)
    out.update(tab_score=c["sc"].copy(), tab_off=c["off"].astype(np.int32), tab_lse=lse64(c["sc"]), n_valid=int(np.sum(out["flat"] >= 0)),
               status=status, margins=rec.margins, branches=rec.branches, n_cand=len(c["sc"]))
    return out


def _pick_arrays(picks):
    return dict(score=np.array([p[0] for p in picks], np.float64), parent=np.array([p[1] for p in picks], np.int32),
                tok=np.array([p[2] for p in picks], np.int32), node=np.array([p[3] for p in picks], np.int32),
                flat=np.array([p[4] for p in picks], np.int32))


# ------------------------------------------------------------------ what both walks share
def _step_rows(w: WalkIn, i, hit, sbh):
    """verify_step_rows: the rows step i expands"""
    if i == 0:
        brow = np.arange(w.nb)
        bscore = w.blk[0]["score"][: w.nb].astype(np.float64)
    else:
        brow = np.asarray(hit, np.int64)
        bscore = np.asarray(sbh, np.float64)
    node = w.blk[i]["node"][brow]
    lrow = w.blk_row0[i] + brow
    return node, brow, lrow, bscore


def _outputs(w: WalkIn, picks, nm, status, rec, rules):
    """verify_outputs: new round beams, next target inputs, the draft's re-ingest inputs, the mailbox"""
    k, dk, W = w.k, w.dk, w.W
    cnt = w.nb if nm == 0 else dk
    rowbase = w.n0 - w.nb if nm == 0 else w.n0 + (nm - 1) * dk
    base_next = int(w.cur["slot"][rowbase]) + (0 if "base_no_cnt" in rules else cnt)
    gen_len = w.gen_len0 + nm
    res = _pick_arrays(picks)
    seq = np.zeros((k, LMAX), np.int32)
    src = w.blk[nm].get("seq")
    for j, p in enumerate(picks):
        if src is not None:
            seq[j, :gen_len] = src[p[1], :gen_len]
        if gen_len < LMAX:
            seq[j, gen_len] = p[2]
    res["seq"] = seq
    res["seq_written"] = min(gen_len + 1, LMAX)             # words of every row the walk writes
    rec.b("seq_full", gen_len == LMAX)
    rec.b("k64", k == MAXB and dk == MAXB and w.nb == MAXB)

    def block(slot0):
        ids = res["tok"].copy()
        pos = (w.cur["pos"][rowbase + res["parent"]] + 1).astype(np.int32)
        slot = (slot0 + np.arange(k)).astype(np.int32)
        vis = w.cur["vis"][rowbase + res["parent"]].copy()
        for j in range(k):
            s = slot0 + j
            wd = 0 if "vis_word0" in rules else s >> 6
            if wd < W:
                vis[j, wd] |= np.uint64(1) << np.uint64(s & 63)
        return dict(ids=ids, pos=pos, slot=slot, vis=vis)

    nxt = block(base_next)
    rec.b("vis_straddle", W >= 2 and base_next < 64 <= base_next + k - 1)
    par = [p[1] for p in picks if p[4] >= 0]
    rows = {pp: w.cur["vis"][rowbase + pp].tobytes() for pp in set(par)}
    rec.b("distinct_parent_vis", len(rows) >= 2 and len(set(rows.values())) == len(rows))
    dnext = None
    if nm == w.dl and w.dl > 0:
        rec.b("dnext")
        lo = slice(rowbase, rowbase + dk)
        dnext = {f: np.concatenate((w.cur[f][lo], nxt[f])) for f in ("ids", "pos", "slot", "vis")}
    n_valid = int(np.sum(res["flat"] >= 0))
    rec.b("short_result", n_valid < k)
    return dict(res=res, next=nxt, dnext=dnext, n_matches=nm, n_valid=n_valid, status=status, base_next=base_next)


# ------------------------------------------------------------------ the greedy walk
def walk_greedy_ref(w: WalkIn, rules=()):
    """verify_walk_body (oracle.beamsd_ref.verify): the target's k best of every step must all be among the draft's dk of the next block"""
    rec = Rec()
    nm, status = 0, 0
    hit = sbh = None
    trace = []                                             # per step taken: (score f64 [k], parent [k], token or -1 [k])
    decisions = []
    picks = [NONE_PICK] * w.k
    for i in range(w.dl + 1):
        if i >= w.blocks_ready:
            rec.b("pending")
            return dict(pending=True, n_matches=PENDING, status=status, trace=trace, decisions=decisions, margins=rec.margins,
                        branches=rec.branches)
        node, brow, lrow, bscore = _step_rows(w, i, hit, sbh)
        rec.b("hit_not_identity", i > 0 and list(brow) != list(range(len(brow))))
        rec.b("staged_gaps", i > 0 and w.blk_row0[i] != w.nb + (i - 1) * w.dk)
        c = expand(w.fsm, node, brow, lrow, bscore, w.logits, w.lse, 1.0, None, False, rec, w.vocab, w.row_cand, w.n_row_cand)
        rec.b("free_mode", w.fsm is None)
        status = c["status"] or status
        ids = np.flatnonzero((c["flat"] >= 0) & ((c["sc"] > NEG) | np.isnan(c["sc"])))
        sc = c["sc"][ids]
        rec.b("signed_zero", bool(np.any((sc == 0) & np.signbit(sc))) and bool(np.any((sc == 0) & ~np.signbit(sc))))
        sc = sc + 0.0                                      # a -0.0 takes +0.0's key and comes out as +0.0
        order = np.lexsort((c["flat"][ids], -sc))
        top = sc[order[: w.k + 1]]
        gaps = top[:-1] - top[1:]
        rec.b("tie", bool(np.any(gaps == 0)))
        if np.any(gaps > 0):
            rec.m("greedy", gaps[gaps > 0].min())
        sel = order[: w.k]
        picks = []
        for q in sel:
            fl = int(c["flat"][ids][q])
            parent, tok = fl // (w.fsm.vocab if w.fsm else w.vocab), fl % (w.fsm.vocab if w.fsm else w.vocab)
            nd = 0
            if w.fsm is not None:
                r = [x for x in range(len(brow)) if brow[x] == parent][0]
                e = w.fsm.edge(node[r], tok)
                nd = int(w.fsm.nxt[e]) if e >= 0 else 0
            picks.append((float(sc[q]), parent, tok, nd, fl))
        rec.b("target_none", len(picks) < w.k)
        picks += [NONE_PICK] * (w.k - len(picks))
        trace.append((np.array([p[0] for p in picks]), np.array([p[1] for p in picks]), np.array([p[2] if p[4] >= 0 else -1 for p in picks])))
        rec.b("vtrace", w.vtrace)
        if i == w.dl:
            rec.b("all_accepted")
            rec.b("dl0", w.dl == 0)
            break
        df = list(w.blk[i + 1]["flat"][: w.dk])
        pos = [df.index(p[4]) if p[4] >= 0 and p[4] in df else -1 for p in picks]
        decisions.append(dict(step=i, target=[p[4] for p in picks], pos=pos))
        if min(pos) < 0:
            rec.b("reject_step0", i == 0)
            rec.b("reject_middle", 0 < i < w.dl)
            break
        key = [p[4] for p in picks] if "hit_by_flat" in rules else pos
        rank = np.argsort(np.argsort(key, kind="stable"), kind="stable")
        hit, sbh = [0] * w.k, [0.0] * w.k
        for j in range(w.k):
            hit[rank[j]], sbh[rank[j]] = pos[j], picks[j][0]
        rec.b("target_order_differs", pos != sorted(pos))
        nm += 1
    out = _outputs(w, picks, nm, status, rec, rules)
    out.update(pending=False, trace=trace, decisions=decisions, margins=rec.margins, branches=rec.branches)
    return out


# ------------------------------------------------------------------ the sampled walk
def walk_sample_ref(w: WalkIn, rules=()):
    """verify_sample_body (oracle.beamsd_sample_ref.verify_sample with HashRng)"""
    rec = Rec()
    k, dk, T, fsm = w.k, w.dk, w.T, w.fsm
    nm, status = 0, 0
    hit = sbh = None
    decisions = []
    fin = np.full(k, -1, np.int64)
    for i in range(w.dl + 1):
        node, brow, lrow, bscore = _step_rows(w, i, hit, sbh)
        rec.b("hit_not_identity", i > 0 and list(brow) != list(range(len(brow))))
        c = expand(fsm, node, brow, lrow, bscore, w.logits, w.lse, T, w.cutoff, True, rec)
        status = c["status"] or status
        if i == w.dl:                                                      # bonus draw from the target
            fin = sample_topn(c["flat"], c["sc"], k, rng_sub(w.seed, P_BONUS, w.round, i, 0), rec, ordered=True)
            rec.b("bonus")
            rec.b("dl0", w.dl == 0)
            rec.b("all_accepted", w.dl > 0)
            decisions.append(dict(step=i, bonus=fin.tolist()))
            break
        Lt, Ld = lse64(c["sc"]), float(w.dtab[i]["lse"])
        d_flat = w.blk[i + 1]["flat"][:dk].astype(np.int64)
        d_score = w.blk[i + 1]["score"][:dk].astype(np.float64)
        u = u01(np.arange(dk), rng_sub(w.seed, P_ACCEPT, w.round, i, 0))
        d_h = hashes(np.arange(dk), rng_sub(w.seed, P_PERM, w.round, i, 0))
        acc = np.zeros(dk, bool)
        d_sc = np.full(dk, NEG)
        rec.b("short_draft_block", bool(np.any(d_flat < 0)))
        for d in range(dk):
            if d_flat[d] < 0:
                continue
            t = pick_of_flat(d_flat[d], fsm, node, brow, lrow, bscore, w.logits, w.lse, T, w.cutoff)
            rec.b("parent_not_hit", i >= 1 and t[1] not in list(brow))
            rec.b("draft_pick_removed", t[1] in list(brow) and t[0] == NEG)
            p = np.exp(t[0] - Lt) if t[0] > NEG else 0.0
            q = np.exp(d_score[d] - Ld)
            if "accept_swapped" in rules:
                acc[d] = u[d] * p <= q
            elif "accept_strict" in rules:
                acc[d] = u[d] * q < p
            else:
                acc[d] = u[d] * q <= p
            if p > 0:
                rec.m("accept", abs(np.log(u[d] * q) - np.log(p)))
            d_sc[d] = t[0]
        n_acc = int(acc.sum())
        if n_acc >= k:
            rec.b("n_acc_eq_k", n_acc == k)
            rec.b("n_acc_gt_k", n_acc > k)
            a_pos = np.flatnonzero(acc)
            hh = d_h[a_pos].astype(np.int64)
            order = np.lexsort((a_pos, -hh if "subset_largest" in rules else hh))
            chosen = np.sort(a_pos[order[:k]])                            # draft positions, ascending
            if "draft_order" not in rules:
                chosen = chosen[np.argsort(d_flat[chosen], kind="stable")]   # result in ascending flat id
            rec.b("subset_reorders", list(chosen) != sorted(chosen))
            hit, sbh, fin = chosen.tolist(), d_sc[chosen].tolist(), d_flat[chosen].copy()
            decisions.append(dict(step=i, accepted=acc.tolist(), chosen=hit, ids=fin.tolist()))
            nm += 1
            continue
        rec.b("reject_some", 0 < n_acc < k)
        rec.b("reject_none_accepted", n_acc == 0)
        taken = set(d_flat[acc].tolist())
        live = (c["flat"] >= 0) & (c["sc"] > NEG)
        logw = np.full(len(c["sc"]), NEG)
        pr = np.zeros(len(c["sc"]))
        tot = 0.0
        dts, dto = w.dtab[i]["score"], w.dtab[i]["off"]
        for x in np.flatnonzero(live):
            q = np.exp(float(dts[dto[brow[c["r"][x]]] + c["j"][x]]) - Ld)
            p = np.exp(c["sc"][x] - Lt)
            if int(c["flat"][x]) in taken and "residual_keeps_taken" not in rules:
                continue
            pr[x] = p
            if p != q:
                rec.m("sign", abs(p - q) / max(p, q))
            if p - q > 0:
                logw[x] = np.log(p - q)
                tot += p - q
        if tot == 0.0:
            rec.b("zero_mass_fallback")
            if "no_fallback" not in rules:
                if "fallback_uniform" in rules:
                    logw = np.where(pr > 0, 0.0, NEG)
                else:
                    logw = np.where(pr > 0, np.log(np.where(pr > 0, pr, 1.0)), NEG)
        drawn = sample_topn(c["flat"], logw, k - n_acc, rng_sub(w.seed, P_RESID, w.round, i, 0), rec, ordered=False)
        rec.b("resample_short", bool(np.any(drawn < 0)))
        allf = np.concatenate((d_flat[acc], np.where(drawn < 0, 0x7FFFFFFF, drawn)))
        allf = np.sort(allf, kind="stable")
        fin = np.where(allf == 0x7FFFFFFF, -1, allf)
        decisions.append(dict(step=i, accepted=acc.tolist(), drawn=drawn.tolist(), ids=fin.tolist()))
        break
    # picks of the final set, in the row space of the last step's expand
    picks = [pick_of_flat(f, fsm, node, brow, lrow, bscore, w.logits, w.lse, T, w.cutoff) for f in fin]
    out = _outputs(w, picks, nm, status, rec, rules)
    out.update(pending=False, decisions=decisions, margins=rec.margins, branches=rec.branches)
    return out


def walk_ref(w: WalkIn, rules=()):
    return walk_sample_ref(w, rules) if w.sample else walk_greedy_ref(w, rules)
