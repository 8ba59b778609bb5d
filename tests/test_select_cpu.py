"""The cases of tests/select_cases.py are what they say, their reference alone satisfies every condition the GPU tests assert, and the geometry
they restate is still the one of atspeed_amd/csrc/scan.hip.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import beamsd_ref as R
from tests import select_cases as S

EXPAND = {c.name: c for c in S.expand_cases()}
TOPK = {c.name: c for c in S.topk_cases()}
FREE = {c.name: c for c in S.free_cases()}


def _tie_ranks(sorted_scores, k):
    """ranks i < k whose score equals the next one's (i = k - 1: the k-th against the first loser)"""
    s = np.asarray(sorted_scores, np.float64)
    return [i for i in range(min(k, len(s) - 1)) if s[i] == s[i + 1]]


def _sorted_scores(scores, n):
    ids = S.select_ref(scores, n)
    return np.asarray(scores, np.float64).reshape(-1)[ids[ids >= 0]]


# ------------------------------------------------------------------ drift guard
def test_geometry_is_still_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "atspeed_amd", "csrc", "scan.hip")).read()
    assert re.search(r"constexpr int kScanThreads = (\d+);", src).group(1) == str(S.THREADS)
    assert re.search(r"constexpr int kCPT = (\d+);", src).group(1) == str(S.SLOTS)
    assert re.search(r"constexpr int kTopkLead = (\d+);", src).group(1) == str(S.LEAD)
    assert re.search(r"constexpr int U = (\d+),", src).group(1) == str(S.LSE_U)
    assert "constexpr int kScanWaves = kScanThreads / 64;" in src and S.LANES == 64
    assert "constexpr int kMaxCand = kScanThreads * kCPT;" in src and S.CHUNK == S.THREADS * S.SLOTS
    assert "const int nt = n_rows >= 1024 ? 256 : 512;" in src
    assert (S.lse_threads(1023), S.lse_threads(1024)) == (512, 256)
    assert "int c = tid + i * kScanThreads;" in src                      # candidate c: thread c % 1024, slot c // 1024
    assert "keys[kCPT] = tid < kk ? best[tid] : 0;" in src               # the carried j-th best rides on thread j
    from atspeed_amd import _lib
    assert _lib.MAX_BEAMS == S.MAX_BEAMS


# ------------------------------------------------------------------ expand + prune
def _expand_properties(c):
    rows, toks = c.candidates()
    fs = c.flat_scores()
    exp = c.expected()
    flat = np.array(exp["flat"])
    n = int((flat >= 0).sum())
    cand_flat = rows * c.vocab + toks
    index_of = {int(f): i for i, f in enumerate(cand_flat)}
    win = np.array([index_of[int(f)] for f in flat[:n]], dtype=np.int64)             # candidate indices of the winners
    per_wave = np.bincount(S.wave_of(win), minlength=S.WAVES).tolist() if n else [0] * S.WAVES
    scores = fs[cand_flat].astype(np.float64)
    # the lead keys: the LEAD best of every wave (score desc, flat asc); the bound is the k-th best of them
    lead = []
    for w in range(S.WAVES):
        mine = np.flatnonzero(S.wave_of(np.arange(len(cand_flat))) == w)
        order = mine[np.lexsort((cand_flat[mine], -scores[mine]))][: min(S.LEAD, c.k)]
        lead += [(-scores[i], int(cand_flat[i])) for i in order]
    lead.sort()
    p = {"live": len(cand_flat), "n": n, "winner_waves": sorted(set(S.wave_of(win).tolist())), "winner_slots": sorted(set(S.slot_of(win).tolist())),
         "per_wave": per_wave, "max_per_thread": int(np.bincount(S.thread_of(win)).max()) if n else 0,
         "tie_ranks": _tie_ranks(_sorted_scores(fs, c.k + 1), c.k), "winner_rows": sorted(set(exp["parent"])),
         "dead_rows": [r for r in range(c.rows) if c.bscore[r] == S.NEG_INF],
         "last_candidate_wins": bool(n and len(cand_flat) - 1 in win.tolist()),
         "bound_is_kth": len(lead) >= c.k and n == c.k and lead[c.k - 1][1] == int(flat[c.k - 1])}
    if n:
        kth = int(win[-1])                                                             # rank of the k-th key inside its own wave (0 = its best)
        same = np.flatnonzero(S.wave_of(np.arange(len(cand_flat))) == S.wave_of(kth))
        p["kth_wave_rank"] = int(sum((scores[i], -cand_flat[i]) > (scores[kth], -cand_flat[kth]) for i in same))
    if c.name == "tie_at_k":
        p["kth_row"] = exp["parent"][-1]
        p["next_row"] = int(S.select_ref(fs, c.k + 1)[-1] // c.vocab)
        assert c.children(p["next_row"])[0] < exp["token"][-1]                        # a rule "lower token first" would pick the other one
    if c.name == "tie_across_waves":
        i = p["tie_ranks"][0]
        p["tie_waves"] = sorted(S.wave_of(win[i: i + 2]).tolist())
        p["tie_slots"] = sorted(S.slot_of(win[i: i + 2]).tolist())
    return p


@pytest.mark.parametrize("name", list(EXPAND))
def test_expand_case_is_what_it_claims(name):
    c = EXPAND[name]
    assert c.claims, "a case claims at least one property"
    p = _expand_properties(c)
    for key, want in c.claims.items():
        assert p[key] == want, (key, p[key], want)
    assert p["live"] <= S.CHUNK and c.rows <= S.MAX_BEAMS and 1 <= c.k <= S.MAX_BEAMS
    # the automaton is one atspeed_fsm_create accepts: children strictly ascending, edges inside the node table
    assert c.row_ptr[0] == 0 and c.row_ptr[-1] == len(c.tok) and len(c.row_ptr) == c.n_nodes + 1
    for n in range(c.n_nodes):
        kids = c.tok[c.row_ptr[n]: c.row_ptr[n + 1]]
        assert np.all(np.diff(kids) > 0) and np.all((kids >= 0) & (kids < c.vocab))
    assert np.all((c.nxt >= 0) & (c.nxt < c.n_nodes)) and len(set(c.nxt.tolist())) > 1
    # the logits of forbidden tokens (900) and of dead rows' children (500) would win if the kernel took them for candidates; none is expected
    exp = c.expected()
    assert float(np.max(exp["score"])) < 400.0 and float(c.logits.max()) == 900.0


@pytest.mark.parametrize("name", list(EXPAND))
def test_expand_case_values_are_exact_and_reference_agrees(name):
    c = EXPAND[name]
    assert S.is_dyadic(c.logits) and S.is_dyadic(c.bscore)
    rows, toks = c.candidates()
    exact = c.logits[rows, toks].astype(np.float64) + c.bscore[rows].astype(np.float64)
    assert np.array_equal(S.score32(c.logits[rows, toks], c.bscore[rows]).astype(np.float64), exact)
    fs = torch.from_numpy(c.flat_scores())
    vals, idx = R.topk_desc_stable(fs, c.k)
    want = [int(i) if v > S.NEG_INF else -1 for v, i in zip(vals.tolist(), idx.tolist())]
    assert c.expected()["flat"] == want + [-1] * (c.k - len(want))
    assert np.array_equal(c.expected()["score"], vals[vals > S.NEG_INF].numpy())


def test_expand_k_sweep_and_wave_cases_are_complete():
    assert {c.k for c in EXPAND.values() if c.name.startswith("k_sweep")} == {1, 2, 3, 4, 5, 63, 64}
    assert {"one_wave[0]", "one_wave[7]", "one_wave[15]", "four_per_wave", "no_bound", "two_slots_one_thread", "full", "plateau", "tie_at_k",
            "tie_across_waves", "dead_rows", "one_live_of_64"} <= set(EXPAND)
    for w in (0, 7, 15):                                                               # one winner per lane, every other candidate finite
        c = EXPAND[f"one_wave[{w}]"]
        rows, toks = c.candidates()
        idx = {int(f): i for i, f in enumerate(rows * c.vocab + toks)}
        win = np.array([idx[f] for f in c.expected()["flat"]])
        assert sorted((S.thread_of(win) % S.LANES).tolist()) == list(range(S.LANES))
        assert np.all(np.isfinite(c.flat_scores()[rows * c.vocab + toks]))


# ------------------------------------------------------------------ row_topk and the mask-free expand
def _topk_properties(c, r):
    row = c.rows[r]
    want = c.expected()[r, : c.k]
    win = want[want >= 0]
    p = {"finite": int(np.isfinite(row).sum()), "winner_cols": win.tolist(), "winner_col_set": sorted(win.tolist()), "winner_chunks": sorted(set(S.chunk_of(win).tolist())),
         "tie_ranks": _tie_ranks(_sorted_scores(row, c.k + 1), c.k)}
    best = S.select_ref(row, 5)
    p["best_cols"] = sorted(best[best >= 0].tolist())
    p["best_chunks"] = sorted(set(S.chunk_of(best[best >= 0]).tolist()))
    top = np.flatnonzero(row == np.max(row)) if p["finite"] else np.zeros(0, np.int64)
    p["plateau_chunks"] = sorted(set(S.chunk_of(top).tolist()))
    later = win[S.chunk_of(win) > 0]
    p["later_threads_below_k"] = bool(len(later) and np.all(S.thread_of(later) < c.k) and np.any(S.chunk_of(win) == 0))
    return p


@pytest.mark.parametrize("name", list(TOPK))
def test_topk_case_is_what_it_claims(name):
    c = TOPK[name]
    assert c.vocab in (S.V3, S.V1) and len(c.rows) <= 8 and c.rows.shape[1] == c.vocab
    assert (S.chunk_of(S.V3 - 1), S.chunk_of(S.V3 - 6), S.chunk_of(S.V1 - 1)) == (2, 1, 0)       # three chunks, the last of 5 columns; one
    if "zeros" in c.claims:
        for r, (neg, pos) in enumerate(c.claims["zeros"]):
            row = c.rows[r]
            assert neg < pos and np.signbit(row[neg]) and row[neg] == 0 and not np.signbit(row[pos]) and row[pos] == 0
            assert np.all(np.delete(row, [neg, pos]) < 0)
            assert c.expected()[r, :2].tolist() == [neg, pos]
        return
    p = _topk_properties(c, 0)
    for key, want in c.claims.items():
        assert p[key] == want, (key, p[key], want)
    assert S.is_dyadic(c.rows)


@pytest.mark.parametrize("name", list(TOPK))
def test_topk_reference_agrees_with_oracle(name):
    c = TOPK[name]
    for r, row in enumerate(c.rows):
        vals, idx = R.topk_desc_stable(torch.from_numpy(row), c.k)
        want = [int(i) for v, i in zip(vals.tolist(), idx.tolist()) if v > S.NEG_INF]
        assert c.expected()[r].tolist() == want + [-1] * (S.MAX_BEAMS - len(want))


def test_topk_cases_are_complete():
    for v in (S.V3, S.V1):
        assert {f"{n}-V{v}" for n in ("boundary", "last_chunk_only[5]", "last_chunk_only[20]", "ramp_desc", "ramp_asc", "all_equal", "plateau",
                                     "few_finite", "all_neg_inf", "signed_zeros", "wave0_competition")} <= set(TOPK)
    c = TOPK[f"wave0_competition-V{S.V3}"]                                            # carried and new keys alternate in the answer
    chunks = S.chunk_of(c.expected()[0, : c.k])
    assert set(chunks.tolist()) == {0, 1, 2} and np.count_nonzero(np.diff(chunks)) >= 10
    c = TOPK[f"last_chunk_only[20]-V{S.V3}"]                                          # the five best in the last chunk, the rest from earlier ones
    assert S.chunk_of(c.expected()[0, :5]).tolist() == [2] * 5 and set(S.chunk_of(c.expected()[0, 5:20]).tolist()) <= {0, 1}


@pytest.mark.parametrize("name", list(FREE))
def test_free_case_is_exact_tied_and_agrees_with_oracle(name):
    c = FREE[name]
    assert len(c.rows) <= 8 and S.is_dyadic(c.rows) and S.is_dyadic(c.bscore)
    fs = c.flat_scores()
    exact = (c.rows.astype(np.float64) + c.bscore.astype(np.float64)[:, None]).reshape(-1)
    ok = np.isfinite(exact)
    assert np.array_equal(fs.astype(np.float64)[ok], exact[ok]) and np.all(np.isneginf(fs[~ok]))
    exp = c.expected()
    vals, idx = R.topk_desc_stable(torch.from_numpy(fs), c.k)
    assert exp["flat"] == [int(i) if v > S.NEG_INF else -1 for v, i in zip(vals.tolist(), idx.tolist())]
    if "tie_ranks" in c.claims:
        assert _tie_ranks(_sorted_scores(fs, c.k + 1), c.k) == c.claims["tie_ranks"]
        assert exp["parent"][:2] == c.claims["tie_rows"] and exp["score"][0] == exp["score"][1]
        assert [r for r in range(len(c.rows)) if c.bscore[r] == S.NEG_INF] == c.claims["dead_rows"]
        assert not set(c.claims["dead_rows"]) & set(exp["parent"])
    # the k best pairs lie among each row's k best columns: what the two-stage kernel relies on
    for f in exp["flat"]:
        if f >= 0:
            assert f % c.vocab in S.select_ref(c.rows[f // c.vocab], c.k).tolist()


# ------------------------------------------------------------------ LSE
@pytest.mark.parametrize("nt", [512, 256])
def test_lse_vocabularies_cover_every_loop_shape(nt):
    ch = S.lse_chunk(nt)
    assert ch == nt * 8 * 4
    shapes = {name: S.lse_split(v, nt) for name, v in S.lse_vocabs(nt)}
    assert len(shapes) == 18 and max(v for _, v in S.lse_vocabs(nt)) == 3 * ch + 4 * nt + 2
    for n in (1, 2, 3):
        assert shapes[f"{n}c"] == {"n_full": n, "partial": 0, "tail": 0}
        assert shapes[f"{n}c+1"] == {"n_full": n, "partial": 0, "tail": 1}               # a scalar tail after an empty partial chunk
        assert shapes[f"{n}c+3"] == {"n_full": n, "partial": 0, "tail": 3}
        assert shapes[f"{n}c+4"] == {"n_full": n, "partial": 4, "tail": 0}               # one vector, thread 0 alone
        assert shapes[f"{n}c+4nt+2"] == {"n_full": n, "partial": 4 * nt, "tail": 2}      # one vector per thread
    assert shapes["c-1"] == {"n_full": 0, "partial": ch - 4, "tail": 3}
    assert shapes["7"] == {"n_full": 0, "partial": 4, "tail": 3} and shapes["3"] == {"n_full": 0, "partial": 0, "tail": 3}


@pytest.mark.parametrize("vname,rows", [("3c+4nt+2", 3), ("2c+3", 3), ("1c", 3), ("7", 3), ("3", 1), ("c-1", 1)])
def test_lse_case_is_what_it_claims(vname, rows):
    nt = S.lse_threads(rows)
    vocab = dict(S.lse_vocabs(nt))[vname]
    fams = S.LSE_FAMILIES
    for g0 in range(0, len(fams), rows):
        c = S.lse_case(vname, vocab, rows, fams[g0: g0 + rows])
        sp = S.lse_split(vocab, nt)
        assert c.nt == 512 and {k: c.claims[k] for k in sp} == sp
        assert c.ld == (vocab + 3) // 4 * 4 + (64 if vname == "2c+3" else 0) and c.x.shape == (rows, c.ld)
        assert bool(torch.isnan(c.x[:, vocab:]).all()) and not bool(torch.isnan(c.x[:, :vocab]).any())
        assert not bool(torch.isposinf(c.x[:, :vocab]).any())
        x = c.x[:, :vocab].numpy()
        for r, f in enumerate(c.families):
            if f.startswith("b_"):
                col = c.claims["planted"][f]
                assert int(np.argmax(x[r])) == col and x[r, col] == 40.0
                lo, hi = {"b_full": ((sp["n_full"] - 1) * S.lse_chunk(nt), sp["n_full"] * S.lse_chunk(nt)),
                          "b_partial": (sp["n_full"] * S.lse_chunk(nt), vocab - sp["tail"]), "b_tail": (vocab - sp["tail"], vocab)}[f]
                assert lo <= col < hi
            elif f == "c":
                assert np.all(x[r] == S.LSE_CONST) and abs(c.ref[r] - (S.LSE_CONST + np.log(vocab))) < 1e-12
            elif f == "d":
                assert abs(float(np.mean(x[r])) - 1e4) < 5.0
            elif f == "e":
                assert np.all(np.isneginf(x[r, vocab - sp["tail"]:]))
                if sp["n_full"]:
                    assert all(np.all(np.isneginf(x[r, 4 * (u * nt + 5): 4 * (u * nt + 5) + 4])) for u in range(S.LSE_U))
                assert np.isneginf(c.ref[r]) == bool(np.all(np.isneginf(x[r])))
            elif f == "f":
                assert int(np.isfinite(x[r]).sum()) == 1 and c.ref[r] == float(x[r][np.isfinite(x[r])][0])
            elif f == "g":
                assert np.all(np.isneginf(x[r])) and np.isneginf(c.ref[r])
        assert np.all(np.isfinite(c.ref) | np.isneginf(c.ref))


def test_lse_1024_row_case_holds_every_family():
    vname, vocab = S.lse_vocabs(256)[4]                                                # 1c+4nt+2: every region exists
    c = S.lse_case(vname, vocab, 1024, S.LSE_FAMILIES)
    assert c.nt == 256 and c.claims["n_full"] == 1 and set(c.families) == set(S.LSE_FAMILIES)
    assert max(v for _, v in S.lse_vocabs(256)) <= 3 * S.lse_chunk(256) + 4 * 256 + 2
    kept = {int(np.flatnonzero(np.isfinite(c.x[r, :vocab].numpy()))[0]) for r, f in enumerate(c.families) if f == "f"}
    assert {0, c.claims["planted"]["b_partial"], vocab - 1} <= kept                    # the single finite entry visits every region


# ------------------------------------------------------------------ lm_head
@pytest.mark.parametrize("rows,vocab,hidden", S.LMHEAD_SHAPES)
def test_lmhead_plants_dominate_their_rows(rows, vocab, hidden):
    from atspeed_amd import synth
    x = torch.from_numpy(synth.hash_normal(rows * hidden, 61, 1.0).reshape(rows, hidden)).to(torch.bfloat16)
    w = torch.from_numpy(synth.hash_normal(vocab * hidden, 62, 0.08).reshape(vocab, hidden)).to(torch.bfloat16)
    plants = S.lmhead_plants(rows)
    w2 = S.plant_dominant(x, w, plants)
    stored = {t // 256 for t in S.LMHEAD_FSM_TOKENS}
    assert [col // 256 in stored for _, col in plants] == [True, False, True]
    assert [col for _, col in plants][::2] == [0, vocab - 1] and [r for r, _ in plants] == [0, 256, rows - 1]
    logits = x.double() @ w2.double().T
    for r, col in plants:
        rest = torch.cat((logits[r, :col], logits[r, col + 1:]))
        assert abs(float(logits[r, col]) - 40.0) < 0.5 and float(rest.max()) < 20.0
        assert float(torch.logsumexp(logits[r], -1)) - float(torch.logsumexp(rest, -1)) > 15.0      # the planted tile carries the normaliser
