"""Sampling-mode warpers on the device: the cutoff kernel (`atspeed_warp_cutoffs`) against tests/warp_ref.py, and the sampled BSSD /
target_generate with `top_k` / `top_p` against the host path (transformers' own warpers on the host rows) and against the oracle with the
same warpers patched in.  Every kernel comparison runs on rows that are unambiguous at both boundaries (margins asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib
from atspeed_amd.beamSD import BSSD, BSSD_batch, _Decoder, _DeviceFSM, target_generate
from atspeed_amd.model import HipLlama
from oracle.llama_ref import RefLlama
from tests import warp_ref as W
from tests.golden.cases import CASES, build_case_inputs

SCORE_TOL = 1e-3
MARGIN = 1e-4
V = 6000
# children per automaton node: a strict trie's 1-5, the position-set mask's 256, the sizes around the in-LDS sort's 1024 and two lists
# that take the radix select (>= 4099)
DEGS = (1, 2, 3, 4, 5, 50, 51, 256, 257, 1024, 1025, 4099, 5000)
WARPERS = [(50, 1.0, 2), (8, 0.9, 2), (0, 0.5, 2), (0, 0.9, 2), (2, 0.1, 2), (1, 1.0, 1), (1, 0.1, 1)]


class _Automaton:
    """node i has DEGS[i] children (ascending token ids drawn from the vocabulary)"""

    def __init__(self):
        rng = np.random.default_rng(5)
        self.toks = [np.sort(rng.choice(V, size=d, replace=False)).astype(np.int32) for d in DEGS]
        row_ptr = np.zeros(len(DEGS) + 1, np.int32)
        row_ptr[1:] = np.cumsum(DEGS)
        tok = np.concatenate(self.toks)
        nxt = np.zeros(len(tok), np.int32)
        self.h = _lib.Handle.create("atspeed_fsm_destroy", _lib.load().atspeed_fsm_create, row_ptr.ctypes.data, tok.ctypes.data, nxt.ctypes.data,
                                    len(DEGS), len(tok), V)


@pytest.fixture(scope="module")
def automaton():
    return _Automaton()


def _logit_row(deg: int, kind: str, seed: int) -> np.ndarray:
    """one row of V logits.  "peaky": N(0, scale^2), the scale growing with the child count (a flat row of thousands of entries has
    cumulative probabilities closer than 1e-4 to each other, so none can be unambiguous); "plateau": 28 % of the tokens on a high plateau
    of about 7e-4 probability each, so a nucleus of more than 1024 entries still has cumulative sums several 1e-4 apart"""
    rng = np.random.default_rng(seed)
    if kind == "plateau":
        x = rng.standard_normal(V).astype(np.float32) * np.float32(0.1) - np.float32(12.0)
        hi = rng.choice(V, size=(V * 28) // 100, replace=False)
        x[hi] += np.float32(18.0)
        return x
    return (rng.standard_normal(V) * (2.0 if deg <= 300 else 8.0)).astype(np.float32)


def _scores(logits: np.ndarray, lse: np.ndarray, toks: np.ndarray, r: int, temperature: float) -> np.ndarray:
    """(logit - lse) / temperature in fp32: the expression of expand_candidates"""
    return ((logits[r, toks] - np.float32(lse[r])) / np.float32(temperature)).astype(np.float32)


def _cutoffs(automaton, logits: np.ndarray, nodes, temperature, top_k, top_p, min_keep):
    lib = _lib.load()
    n = len(nodes)
    lg = torch.from_numpy(logits).cuda().contiguous()
    lse = torch.empty(n, dtype=torch.float32, device="cuda")
    nd = torch.tensor(list(nodes), dtype=torch.int32, device="cuda")
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    st = _lib.stream_ptr(lg.device)
    _lib.check(lib.atspeed_lse_rows(lg.data_ptr(), n, V, V, lse.data_ptr(), st))
    _lib.check(lib.atspeed_warp_cutoffs(lg.data_ptr(), V, lse.data_ptr(), n, automaton.h.ptr, nd.data_ptr(), float(temperature), int(top_k),
                                        float(top_p), int(min_keep), out.data_ptr(), st))
    torch.cuda.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def _build_rows(automaton, plan, temperature, top_k, top_p, min_keep):
    """`plan` = [(node, kind, tie)]: per row the first seed whose scores (with a CPU normaliser) clear both margins; never the outcome"""
    rows = []
    for r, (node, kind, tie) in enumerate(plan):
        toks = automaton.toks[node]
        for seed in range(60):
            x = _logit_row(DEGS[node], kind, 7919 * r + 100 * node + seed)
            if tie:                                     # an exact tie between the k'-th and (k'+1)-th largest children
                order = toks[np.argsort(-x[toks], kind="stable")]
                x[order[tie]] = x[order[tie - 1]]
            lse = np.float32(np.log(np.exp(x.astype(np.float64) - x.max()).sum()) + x.max())
            gk, gp = W.margins(_scores(x[None], [lse], toks, 0, temperature), top_k, top_p, min_keep, tie_at_k=bool(tie))
            if gk >= 1.2 * MARGIN and gp >= 1.2 * MARGIN:
                break
        else:
            raise AssertionError(f"no unambiguous row for node {node} ({DEGS[node]} children), {kind}, top_k={top_k} top_p={top_p}")
        rows.append(x)
    return np.stack(rows)


def _check(automaton, plan, temperature, top_k, top_p, min_keep):
    logits = _build_rows(automaton, plan, temperature, top_k, top_p, min_keep)
    nodes = [p[0] for p in plan]
    cut, lse = _cutoffs(automaton, logits, nodes, temperature, top_k, top_p, min_keep)
    for r, (node, kind, tie) in enumerate(plan):
        s = _scores(logits, lse, automaton.toks[node], r, temperature)
        gk, gp = W.margins(s, top_k, top_p, min_keep, tie_at_k=bool(tie))
        assert gk >= MARGIN and gp >= MARGIN, ("boundary precondition", r, node, gk, gp)       # with the DEVICE's normaliser
        got, want = s >= cut[r], W.survivors(s, top_k, top_p, min_keep)
        assert np.array_equal(got, want), (r, DEGS[node], kind, top_k, top_p, min_keep, int(got.sum()), int(want.sum()), float(cut[r]),
                                           W.cutoff(s, top_k, top_p, min_keep))
    return cut


@pytest.mark.parametrize("top_k,top_p,min_keep", WARPERS)
def test_cutoff_kernel_keeps_the_reference_survivors(automaton, top_k, top_p, min_keep):
    """every node kind twice in ONE launch (rows of different nodes side by side), two temperatures; then a first step: one source row"""
    plan = [(i, "peaky", 0) for i in range(len(DEGS))] + [(i, "peaky", 0) for i in reversed(range(len(DEGS)))]
    if top_p < 1.0:
        plan += [(len(DEGS) - 1, "plateau", 0), (len(DEGS) - 2, "plateau", 0)]        # a nucleus of more than 1024 entries: several runs
    for temperature in (1.0, 1.3):
        _check(automaton, plan, temperature, top_k, top_p, min_keep)
    for node in (0, 7, 11):
        _check(automaton, [(node, "peaky", 0)], 0.7, top_k, top_p, min_keep)


def test_plateau_rows_reach_the_multi_run_walk(automaton):
    """the plateau rows are what they are meant to be: more survivors than one 1024-entry run holds"""
    logits = _build_rows(automaton, [(12, "plateau", 0)], 1.0, 0, 0.9, 2)
    cut, lse = _cutoffs(automaton, logits, [12], 1.0, 0, 0.9, 2)
    s = _scores(logits, lse, automaton.toks[12], 0, 1.0)
    assert (s >= cut[0]).sum() > 1024 and np.array_equal(s >= cut[0], W.survivors(s, 0, 0.9, 2))


@pytest.mark.parametrize("top_k", [2, 50])
def test_an_exact_tie_at_the_kth_value_survives_on_the_device(automaton, top_k):
    plan = [(i, "peaky", top_k) for i, d in enumerate(DEGS) if d > top_k]
    cut = _check(automaton, plan, 1.0, top_k, 1.0, 2)
    logits = _build_rows(automaton, plan, 1.0, top_k, 1.0, 2)
    _, lse = _cutoffs(automaton, logits, [p[0] for p in plan], 1.0, top_k, 1.0, 2)
    for r, (node, _, _) in enumerate(plan):
        assert (_scores(logits, lse, automaton.toks[node], r, 1.0) >= cut[r]).sum() == top_k + 1


def test_both_warpers_off_cut_nothing(automaton):
    rng = np.random.default_rng(3)
    nodes = list(range(len(DEGS)))
    logits = (rng.standard_normal((len(nodes), V)) * 2).astype(np.float32)
    for top_k, top_p in ((0, 1.0), (0, 1.5)):
        cut, _ = _cutoffs(automaton, logits, nodes, 1.3, top_k, top_p, 2)
        assert np.all(np.isneginf(cut))
    cut, _ = _cutoffs(automaton, logits, nodes, 1.3, 50, 1.0, 2)                       # fewer children than k': the k'-th largest is -inf
    assert all(np.isneginf(cut[i]) == (DEGS[i] < 50) for i in nodes)


def test_bad_arguments_are_refused(automaton):
    lib = _lib.load()
    x = torch.zeros(4, V, device="cuda")
    y = torch.zeros(4, device="cuda")
    nd = torch.zeros(4, dtype=torch.int32, device="cuda")
    for temperature, top_k, top_p, min_keep in ((0.0, 5, 1.0, 2), (1.0, -1, 1.0, 2), (1.0, 5, 0.0, 2), (1.0, 5, 0.9, 0)):
        assert lib.atspeed_warp_cutoffs(x.data_ptr(), V, y.data_ptr(), 4, automaton.h.ptr, nd.data_ptr(), temperature, top_k, top_p, min_keep,
                                        y.data_ptr(), None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------------------------- end to end
NAME, TEMPERATURE = "k10_dk40_sigma01", 1.3
E2E_WARPERS = [(50, None), (8, 0.9), (None, 0.5)]
SEEDS = list(range(40, 52))


@pytest.fixture(scope="module")
def pair():
    case = next(c for c in CASES if c["name"] == NAME)
    ci = build_case_inputs(case)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **kw)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **kw)
    for m in (tgt, drf):
        m.generation_config.do_sample = True
        m.generation_config.temperature = TEMPERATURE
    yield case, ci, tgt, drf
    for m in (tgt, drf):
        m.generation_config.do_sample = False


def _set(tgt, drf, top_k, top_p):
    for m in (tgt, drf):
        m.generation_config.top_k, m.generation_config.top_p = top_k, top_p


def _same(dev, other):
    """tokens, n_run and accepted steps identical, scores within the project's 1e-3 (the host path returns the finite beams only)"""
    nv = dev["n_valid"]
    assert other["beam_sequence"].shape[0] == nv and torch.equal(other["beam_sequence"], dev["beam_sequence"][:nv])
    if "n_run" in dev:
        assert other["n_run"] == dev["n_run"] and other["accept_steps"] == dev["accept_steps"]
    np.testing.assert_allclose(other["beam_scores"].cpu().numpy(), dev["beam_scores"][:nv].cpu().numpy(), atol=SCORE_TOL, rtol=0)


@pytest.mark.parametrize("top_k,top_p", E2E_WARPERS)
def test_device_path_samples_what_the_host_path_samples(pair, top_k, top_p):
    """a closure that wraps the compilable constraint is served by hostmask.py, which warps the host rows with transformers' own
    TopKLogitsWarper / TopPLogitsWarper: for the same seed the device path (cutoff kernel + sampled step kernels) returns its beams.
    With top_k = 8 this fails where the setting is ignored."""
    case, ci, tgt, drf = pair
    _set(tgt, drf, top_k, top_p)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}
    closure = lambda b, sent: ci["fn"](b, sent)
    g, L = case["gamma"], case["max_new_tokens"]
    warped = []
    for seed in SEEDS:
        dev = BSSD(tgt, drf, inputs, g, L, prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        _same(dev, BSSD(tgt, drf, inputs, g, L, prefix_allowed_tokens_fn=closure, seed=seed))
        _same(target_generate(tgt, inputs, L, prefix_allowed_tokens_fn=ci["fn"], seed=seed),
              target_generate(tgt, inputs, L, prefix_allowed_tokens_fn=closure, seed=seed))
        warped.append(dev["beam_sequence"])
    # the setting is honoured, not ignored by both paths alike: 10 beams drawn from at most 8 (or a nucleus of) candidates per row are not
    # the beams drawn from all 256
    _set(tgt, drf, None, None)
    plain = [BSSD(tgt, drf, inputs, g, L, prefix_allowed_tokens_fn=ci["fn"], seed=seed)["beam_sequence"] for seed in SEEDS]
    assert sum(not torch.equal(a, b) for a, b in zip(warped, plain)) >= len(SEEDS) // 2


@pytest.mark.parametrize("top_k,top_p", E2E_WARPERS)
def test_batch_of_three_users_samples_what_the_host_path_samples(pair, top_k, top_p):
    """the same comparison through BSSD_batch (the multi-job form of the cutoff launch): three users with prompts of their own, every user
    of every seed against the host path's call for that user's stream"""
    case, ci, tgt, drf = pair
    _set(tgt, drf, top_k, top_p)
    rng0 = np.random.default_rng(1)
    prompts = [ci["prompt"]] + [np.concatenate([rng0.integers(3, 31000, size=n), ci["prompt"][-6:]]) for n in (9, 30)]
    inputs = [{"input_ids": torch.from_numpy(p.astype(np.int64))[None].cuda()} for p in prompts]
    closure = lambda b, sent: ci["fn"](b, sent)
    g, L = case["gamma"], case["max_new_tokens"]
    for seed in SEEDS:
        outs = BSSD_batch(tgt, drf, inputs, g, L, prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        for u, (inp, o) in enumerate(zip(inputs, outs)):                       # user u draws from stream seed + u
            _same(o, BSSD(tgt, drf, inp, g, L, prefix_allowed_tokens_fn=closure, seed=seed + u))


@pytest.mark.parametrize("top_k,top_p", [(8, 0.9), (50, None)])
def test_device_makes_the_oracles_decisions_with_the_warpers(pair, top_k, top_p, monkeypatch):
    """oracle/beamsd_sample_ref.py with transformers' warpers applied after its `_tempered` (patched from here): the device makes the same
    decisions -- tokens and per-round n_matches, scores within 1e-3 -- for every seed whose closest draw is decided by more than fp32
    rounding (HashRng.min_margin, as for the temperature alone).  With top_k = 8 this fails where the setting is ignored."""
    from transformers import TopKLogitsWarper, TopPLogitsWarper
    from oracle import beamsd_sample_ref as S
    case, ci, tgt, drf = pair
    _set(tgt, drf, top_k, top_p)
    warpers = [TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=2)] + ([TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=2)] if top_p else [])
    plain = S._tempered

    def warped(logits, seqs, beam_size, fn, temperature):
        rows = plain(logits, seqs, beam_size, fn, temperature)
        for w in warpers:
            rows = w(None, rows)
        return rows
    monkeypatch.setattr(S, "_tempered", warped)
    rt, rd = RefLlama(ci["target_dims"], ci["target_sd"]), RefLlama(ci["draft_dims"], ci["draft_sd"])
    P = len(ci["prompt"])
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}
    g, L = case["gamma"], case["max_new_tokens"]
    checked = 0
    for seed in SEEDS:
        rng = S.HashRng(seed)
        ref = S.BSSD_sample(rt, rd, ci["prompt"], g, L, case["K"], case["DK"], ci["fn"], TEMPERATURE, rng)
        out = BSSD(tgt, drf, inputs, g, L, prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        nv = out["n_valid"]
        same = nv == ref["beam_sequence"].shape[0] and out["beam_sequence"][:nv, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()
        if rng.min_margin < 1e-4 and not same:
            continue
        checked += 1
        assert same, (seed, rng.min_margin)
        assert out["accept_steps"] == [r["n_matches"] for r in ref["rounds"]] and out["n_run"] == ref["n_run"]
        np.testing.assert_allclose(out["beam_scores"][:nv].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
    assert checked >= 10
    checked = 0
    for seed in SEEDS:                                                          # the same rule and the same floor for plain sampled beam search
        rng = S.HashRng(seed)
        ref = S.target_generate_sample(rt, ci["prompt"], L, case["K"], ci["fn"], TEMPERATURE, rng)
        out = target_generate(tgt, inputs, L, prefix_allowed_tokens_fn=ci["fn"], seed=seed)
        nv = out["n_valid"]
        same = nv == ref["beam_sequence"].shape[0] and out["beam_sequence"][:nv, P:].cpu().tolist() == ref["beam_sequence"][:, P:].tolist()
        if rng.min_margin < 1e-4 and not same:
            continue
        checked += 1
        assert same, (seed, rng.min_margin)
        np.testing.assert_allclose(out["beam_scores"][:nv].cpu().numpy(), ref["beam_scores"].numpy(), atol=SCORE_TOL, rtol=0)
    assert checked >= 10


def test_warpers_off_change_nothing_and_launch_nothing(pair):
    """top_k = top_p = None: three sampled calls before and after an explicit atspeed_decoder_set_warpers(..., 0, 1.0, 2) are bit-identical,
    and neither they nor a greedy call launch the cutoff kernel; with top_k set every sampled step does."""
    case, ci, tgt, drf = pair
    lib = _lib.load()
    _set(tgt, drf, None, None)
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}
    g, L = case["gamma"], case["max_new_tokens"]
    calls = [lambda s: BSSD(tgt, drf, inputs, g, L, prefix_allowed_tokens_fn=ci["fn"], seed=s),
             lambda s: target_generate(tgt, inputs, L, prefix_allowed_tokens_fn=ci["fn"], seed=s),
             lambda s: BSSD_batch(tgt, drf, [inputs, inputs], g, L, prefix_allowed_tokens_fn=ci["fn"], seed=s)[1]]
    n0 = lib.atspeed_warp_cutoff_launches()
    before = [c(11 + i) for i, c in enumerate(calls)]
    for target, draft in ((tgt, drf), (tgt, None)):
        for lane in (0, 1):
            try:
                _lib.check(lib.atspeed_decoder_set_warpers(_Decoder.cached(target, draft, lane).handle, 0, 1.0, 2))
            except KeyError:
                pass
    after = [c(11 + i) for i, c in enumerate(calls)]
    for a, b in zip(before, after):
        assert torch.equal(a["beam_sequence"], b["beam_sequence"]) and torch.equal(a["beam_scores"], b["beam_scores"])
    for m in (tgt, drf):
        m.generation_config.do_sample = False
    _set(tgt, drf, 8, 0.9)                                                        # greedy: the warpers are not looked at
    BSSD(tgt, drf, inputs, g, L, prefix_allowed_tokens_fn=ci["fn"])
    target_generate(tgt, inputs, L, prefix_allowed_tokens_fn=ci["fn"])
    assert lib.atspeed_warp_cutoff_launches() == n0
    for m in (tgt, drf):
        m.generation_config.do_sample = True
    target_generate(tgt, inputs, L, prefix_allowed_tokens_fn=ci["fn"], seed=3)
    assert lib.atspeed_warp_cutoff_launches() == n0 + L                           # one launch per sampled step
    h = _Decoder.cached(tgt, None).handle
    assert lib.atspeed_decoder_set_warpers(h, -1, 1.0, 2) == _lib.ERR_INVALID and lib.atspeed_decoder_set_warpers(h, 0, 0.0, 2) == _lib.ERR_INVALID


def test_from_hf_inherits_top_k_50_and_samples_with_it():
    """an HF LlamaForCausalLM's generation config defaults to top_k = 50: `from_hf` carries it over, and a sampled step on the model's own
    logits keeps 50 of the candidates (91 at the first position) the position-set mask allows for the row"""
    import atspeed_amd
    from atspeed_amd import synth
    from tests.test_from_hf_gpu import V as VH, _hf
    hf = _hf(torch.float16, 5)
    hf.generation_config.num_beams = 4
    m = HipLlama.from_hf(hf, max_slots=256, max_tokens=256, max_logit_rows=128)
    assert m.generation_config.top_k == 50 and m.generation_config.top_p in (None, 1.0)
    m.generation_config.do_sample = True
    fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    prompt = synth.synthetic_prompt(40, 3)
    inputs = {"input_ids": torch.from_numpy(prompt)[None].cuda()}
    lib = _lib.load()
    n0 = lib.atspeed_warp_cutoff_launches()
    out = target_generate(m, inputs, 4, prefix_allowed_tokens_fn=fn, seed=1)
    assert lib.atspeed_warp_cutoff_launches() == n0 + 4 and out["n_valid"] == 4
    # the kernel entry on the model's own first-step row: of the start node's children 50 survive
    from atspeed_amd.hostmask import _causal, _forward
    fsm = fn.compile(prompt.tolist())
    logits, lse = _forward(m, _causal(prompt), 1)
    nd = torch.tensor([fsm.start], dtype=torch.int32, device="cuda")
    cut = torch.empty(1, dtype=torch.float32, device="cuda")
    _lib.check(lib.atspeed_warp_cutoffs(logits.data_ptr(), m.logits_ld, lse.data_ptr(), 1, _DeviceFSM.get(fsm, VH).handle, nd.data_ptr(), 1.0,
                                        m.generation_config.top_k, 1.0, 2, cut.data_ptr(), _lib.stream_ptr(m.device)))
    toks = np.asarray(fsm.tok[fsm.row_ptr[fsm.start]: fsm.row_ptr[fsm.start + 1]])
    s = (logits[0].float().cpu().numpy()[toks] - lse.cpu().numpy()[0]).astype(np.float32)
    kept = int((s >= cut.item()).sum())
    assert len(toks) > 50 and 50 <= kept <= 50 + int((s == np.sort(s)[-50]).sum()) - 1            # more than 50 only through ties at the 50th
