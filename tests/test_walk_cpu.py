"""The cases of tests/walk_cases.py are what they claim, and tests/walk_ref.py is the oracle's rule: no GPU, nothing touches the library.

  * placed cases obey the value rule (multiples of 2^-6 below 2^10, lse = 0, temperature 1 / 0.5 / 2), so their scores are exact in fp32;
  * every case reaches the branches it names, every branch the issue lists is named by some placed case, and the smallest margin of every
    kind of decision -- Gumbel key gaps, accept tests, signs of p - q, greedy score gaps -- is at least 1e-4 in the reference alone.  That is
    a condition on the CASES (tests/test_walk_gpu.py excuses nothing at run time), not a tolerance on the kernels;
  * on the natural family the reference makes the decisions of oracle.beamsd_ref.verify / oracle.beamsd_sample_ref.verify_sample /
    one_step_sample on the same inputs;
  * a restatement with a wrong rule is told apart from the right one by at least one case.
"""
import numpy as np
import pytest
import torch

from oracle import beamsd_ref as OG
from oracle import beamsd_sample_ref as OS
from tests import select_cases as S
from tests import walk_cases as W
from tests import walk_ref as R

STEP = {c.name: c for c in W.step_cases()}
SWALK = {c.name: c for c in W.sampled_walk_cases()}
GWALK = {c.name: c for c in W.greedy_walk_cases()}
ALL = [("step", c) for c in STEP.values()] + [("sampled", c) for c in SWALK.values()] + [("greedy", c) for c in GWALK.values()]
IDS = [f"{k}-{c.name}" for k, c in ALL]


@pytest.fixture(scope="module")
def expected():
    return {(k, c.name): c.expected() for k, c in ALL}


def _arrays(kind, c):
    if kind == "step":
        return [c.logits, c.bscore], [c.lse], c.T
    w = c.w
    fin = w.logits[~np.isnan(w.logits)]                   # the rows between staged blocks are NaN: no walk may read them
    return [fin, w.blk[0]["score"]], [w.lse], w.T


@pytest.mark.parametrize("kind,c", ALL, ids=IDS)
def test_case_is_what_it_claims(kind, c, expected):
    out = expected[(kind, c.name)]
    vals, lses, T = _arrays(kind, c)
    if c.family == "placed":
        assert all(S.is_dyadic(v) for v in vals), "value rule: multiples of 2^-6 below 2^10"
        assert all(np.all(x == 0) for x in lses) and T in (1.0, 0.5, 2.0)
        if kind != "step":                                  # the draft's cumulative tempered scores: multiples of 2^-8 below 2^15, exact in fp32
            for b in c.w.blk[1:]:
                f = b["score"][np.isfinite(b["score"])].astype(np.float64)
                assert np.all(f * 256 == np.round(f * 256)) and np.all(np.abs(f) < 2 ** 15)
    else:
        assert T == 1.3 or kind == "greedy"
    missing = [b for b in c.claims if b not in out["branches"]]
    assert not missing, (c.name, missing, out["branches"])
    m = W.case_margins(c, out) if kind != "step" else out["margins"]
    low = {k: v for k, v in m.items() if v < W.MARGIN}
    assert not low, (c.name, low)
    assert out["status"] == 0


def test_every_listed_branch_is_claimed_by_a_placed_case():
    def claimed(cases):
        return {b for c in cases if c.family == "placed" for b in c.claims}
    assert set(W.STEP_BRANCHES) <= claimed(STEP.values())
    walks = claimed(SWALK.values()) | claimed(GWALK.values())
    assert set(W.SAMPLED_WALK_BRANCHES) <= claimed(SWALK.values()) | {"k64"}, set(W.SAMPLED_WALK_BRANCHES) - claimed(SWALK.values())
    assert set(W.GREEDY_WALK_BRANCHES) <= claimed(GWALK.values()), set(W.GREEDY_WALK_BRANCHES) - claimed(GWALK.values())
    assert set(W.OUTPUT_BRANCHES) - {"k64"} <= walks
    # k = dk = nb = 64: the reference names the branch itself, both walks have the case
    assert "k64" in SWALK["k64"].expected()["branches"] and "k64" in GWALK["k64"].expected()["branches"]
    # the table is written for EVERY candidate in expand order: one entry per child of every live row
    for c in STEP.values():
        o = c.expected()
        live = [r for r in range(len(c.bscore)) if c.bscore[r] > -np.inf]
        assert o["n_cand"] == sum(c.fsm.kids(c.node[r])[1] - c.fsm.kids(c.node[r])[0] for r in live) == o["tab_off"][-1]


def test_geometry_and_constants_are_still_the_kernels():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "atspeed_hip.h")).read()
    com = open(os.path.join(root, "atspeed_amd", "csrc", "common.h")).read()
    assert int(re.search(r"#define ATSPEED_MAX_BEAMS (\d+)", hdr).group(1)) == R.MAXB
    assert int(re.search(r"#define ATSPEED_MAX_NEW_TOKENS (\d+)", hdr).group(1)) == R.LMAX
    assert int(re.search(r"#define ATSPEED_MAX_GAMMA (\d+)", hdr).group(1)) == R.GAMMA
    assert "ATS_RNG_STEP = 1, ATS_RNG_ACCEPT = 2, ATS_RNG_PERM = 3, ATS_RNG_RESID = 4, ATS_RNG_BONUS = 5" in com
    assert (R.P_STEP, R.P_ACCEPT, R.P_PERM, R.P_RESID, R.P_BONUS) == (OS.P_STEP, OS.P_ACCEPT, OS.P_PERM, OS.P_RESID, OS.P_BONUS)
    rng = OS.HashRng(77)
    rng.begin(OS.P_RESID, 3, 2, 1)
    assert rng.sub == R.rng_sub(77, R.P_RESID, 3, 2, 1)
    ids = np.arange(50)
    np.testing.assert_array_equal(rng._u01(ids).astype(np.float64), R.u01(ids, rng.sub))


# ------------------------------------------------------------------ the oracle on the natural family
class _Rows:
    """a model whose forward returns given logits rows"""

    def __init__(self, logits):
        self.logits = torch.from_numpy(np.ascontiguousarray(logits))

    def forward(self, ids, pos, slots, vis, n_logit_rows):
        return self.logits[-n_logit_rows:]


def _fn(fsm):
    """prefix_allowed_tokens_fn of the automaton: a beam's sequence is [the node it sits on]"""
    def fn(batch, seq):
        e0, e1 = fsm.kids(int(seq[-1]))
        return fsm.tok[e0:e1].tolist()
    return fn


def _inputs(cur, lo, hi, W):
    vis = np.zeros((hi - lo, 64 * W), bool)
    for r in range(lo, hi):
        for s in range(64 * W):
            vis[r - lo, s] = (int(cur["vis"][r, s >> 6]) >> (s & 63)) & 1
    t = lambda a: torch.from_numpy(a[lo:hi].astype(np.int64))
    return OG.StepInputs(ids=t(cur["ids"]), pos=t(cur["pos"]), slots=t(cur["slot"]), vis=torch.from_numpy(vis))


def _vis_bits(words, width):
    return [[(int(row[s >> 6]) >> (s & 63)) & 1 for s in range(width)] for row in words]


def _dummy_inputs(n):
    return OG.StepInputs(ids=torch.zeros(n, dtype=torch.long), pos=torch.zeros(n, dtype=torch.long), slots=torch.arange(n),
                         vis=torch.eye(n, dtype=torch.bool))


@pytest.mark.parametrize("name", [n for n, c in STEP.items() if c.family == "natural"])
def test_step_ref_makes_the_oracles_draws(name):
    c = STEP[name]
    out = c.expected()
    n = len(c.bscore)
    rng = OS.HashRng(c.seed)
    rng.begin(OS.P_STEP, c.round, c.step, 1)
    o = OS.one_step_sample(_Rows(c.logits), _dummy_inputs(n), c.k, torch.from_numpy(c.bscore), torch.from_numpy(c.node.astype(np.int64))[:, None],
                           _fn(c.fsm), c.T, rng)
    assert o["seq_tokens"].tolist() == out["flat"].tolist()
    assert o["beam_indices"].tolist() == out["parent"].tolist() and o["beam_tokens"].tolist() == out["tok"].tolist()
    np.testing.assert_allclose(o["beam_scores"].double().numpy(), out["score"], rtol=0, atol=2e-5)
    # the table is the oracle's distribution: probs = softmax over every (row, token), candidates in expand order
    probs = o["probs"].double().numpy()
    V = c.fsm.vocab
    flat = np.concatenate([r * V + c.fsm.tok[slice(*c.fsm.kids(c.node[r]))].astype(np.int64) for r in range(n)])
    np.testing.assert_allclose(np.exp(out["tab_score"] - out["tab_lse"]), probs[flat], rtol=1e-4, atol=1e-9)
    assert abs(probs.sum() - probs[flat].sum()) < 1e-6


def _oracle_draft(c, sampled):
    """the draft side of a natural walk case through the oracle's own step; asserts it is the case's blocks"""
    w = c.w
    fn = _fn(w.fsm)
    d = {"step_len": [w.nb], "step_seq_tokens": [], "step_beam_sequence": [torch.from_numpy(w.blk[0]["node"].astype(np.int64))[:, None]],
         "step_beam_indices": [], "step_inputs": [], "step_probs": []}
    rng = OS.HashRng(w.seed)
    for i in range(w.dl):
        n = w.nb if i == 0 else w.dk
        bs = torch.from_numpy(w.blk[i]["score"])
        seqs = d["step_beam_sequence"][i]
        lg = c.aux["dlog"][i]
        if sampled:
            rng.begin(OS.P_STEP, w.round, i, 1)
            o = OS.one_step_sample(_Rows(lg), _dummy_inputs(n), w.dk, bs, seqs, fn, w.T, rng)
            ids = o["seq_tokens"]
            d["step_probs"].append(o["probs"])
        else:
            ids = OG.expand_and_prune(torch.from_numpy(lg), bs, seqs, w.dk, fn)[0]
        assert ids.tolist() == w.blk[i + 1]["flat"].tolist(), "the case's draft block is the oracle's"
        d["step_len"].append(len(ids))
        d["step_seq_tokens"].append(ids)
        d["step_beam_indices"].append(ids // w.fsm.vocab)
        d["step_beam_sequence"].append(torch.from_numpy(w.blk[i + 1]["node"].astype(np.int64))[:, None])
        lo = w.n0 + i * w.dk
        d["step_inputs"].append(_inputs(w.cur, lo, lo + w.dk, w.W))
    return d, fn


def _check_oracle_outputs(w, out, v):
    k = w.k
    assert v["n_matches"] == out["n_matches"]
    np.testing.assert_allclose(v["beam_scores"].double().numpy(), out["res"]["score"], rtol=0, atol=5e-5)
    for name, got, want in (("next", out["next"], v["target_inputs"]), ("dnext", out["dnext"], v["draft_inputs"])):
        if got is None:
            assert want is v["target_inputs"]               # no re-ingest block: the draft gets the target's inputs
            continue
        assert got["ids"].tolist() == want.ids.tolist() and got["pos"].tolist() == want.pos.tolist() and got["slot"].tolist() == want.slots.tolist()
        width = want.vis.shape[1]
        assert width == out["base_next"] + k
        assert _vis_bits(got["vis"], width) == want.vis.long().tolist()
        assert all(int(x) >> max(0, width - 64 * i) == 0 for row in got["vis"] for i, x in enumerate(row) if width < 64 * (i + 1))


@pytest.mark.parametrize("name", [n for n, c in SWALK.items() if c.family == "natural"])
def test_sampled_walk_ref_makes_the_oracles_decisions(name):
    c = SWALK[name]
    w, out = c.w, c.expected()
    d, fn = _oracle_draft(c, True)
    tin = _inputs(w.cur, 0, w.n0, w.W)
    target = {"next_token_scores": torch.from_numpy(w.logits), "packed": _inputs(w.cur, 0, len(w.cur["ids"]), w.W)}
    rng = OS.HashRng(w.seed)
    v = OS.verify_sample(tin, d, target, w.k, torch.from_numpy(w.blk[0]["score"]), None, fn, w.T, rng, w.round)
    assert len(v["trace"]) == len(out["decisions"])
    for t, dec in zip(v["trace"], out["decisions"]):
        if t.get("bonus"):
            assert t["ids"] == dec["bonus"]
        else:
            assert t["accepted"] == sum(dec["accepted"]) and t["ids"] == dec["ids"]
    assert [int(x) for x in out["res"]["flat"]] == v["trace"][-1]["ids"]
    _check_oracle_outputs(w, out, v)


@pytest.mark.parametrize("name", [n for n, c in GWALK.items() if c.family == "natural"])
def test_greedy_walk_ref_makes_the_oracles_decisions(name):
    c = GWALK[name]
    w, out = c.w, c.expected()
    d, fn = _oracle_draft(c, False)
    tin = _inputs(w.cur, 0, w.n0, w.W)
    target = {"next_token_scores": torch.from_numpy(w.logits), "packed": _inputs(w.cur, 0, len(w.cur["ids"]), w.W)}
    v = OG.verify(tin, d, target, w.k, torch.from_numpy(w.blk[0]["score"]), None, fn)
    assert len(v["trace"]) == len(out["trace"])
    V = w.fsm.vocab
    for t, (sc, par, tok) in zip(v["trace"], out["trace"]):
        assert t["target_ids"] == (par * V + tok).tolist()
        np.testing.assert_allclose(np.array(t["target_scores"]), sc, rtol=0, atol=5e-5)
    _check_oracle_outputs(w, out, v)


# ------------------------------------------------------------------ wrong rules are told apart
def _same(a, b):
    if a.get("pending") or b.get("pending"):
        return a.get("pending") == b.get("pending")
    if a["n_matches"] != b["n_matches"] or a["n_valid"] != b["n_valid"]:
        return False
    for part in ("res", "next", "dnext"):
        x, y = a[part], b[part]
        if (x is None) != (y is None):
            return False
        if x is not None and any(not np.array_equal(x[f], y[f]) for f in x if f != "seq_written"):
            return False
    return True


@pytest.mark.parametrize("rule", R.WRONG_RULES)
def test_a_wrong_rule_is_told_apart(rule):
    cases = list(SWALK.values()) + list(GWALK.values())
    caught = [c.name for c in cases if not _same(c.expected(), c.expected((rule,)))]
    print(rule, "caught by", caught)
    assert caught, rule


@pytest.mark.parametrize("rule", R.EQUIVALENT_RULES)
def test_an_equivalent_rule_changes_nothing(rule):
    assert all(_same(c.expected(), c.expected((rule,))) for c in list(SWALK.values()) + list(GWALK.values()))
