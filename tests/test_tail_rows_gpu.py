"""Row-pruned tail of the last layer (switch `tail_rows_tokens`): where at most half of a forward's
rows get logits, the last layer's o_proj / post-attention norm / gate_up / SwiGLU / down run over the logit rows alone; qkv, RoPE, the KV scatter
and the attention run over every row.  The switch at 0 forces the pruned form wherever the rule allows it, at NEVER the full one.

The pruned form is compared with the fp32 oracle (oracle/llama_ref.py on exactly the weight values the device holds), never with the other
form.  Bounds, each taken from the existing test of the same comparison:
  fp32  logits and LSE within 1e-3 absolute: tests/test_bssd_gpu.py:18 (LOGIT_TOL), asserted at :33 (observed there < 1e-4);
  bf16  max error < 0.04 and mean error < 0.006 of max |logit|: tests/test_fulldims_gpu.py:28-29 (BF16_MAX_TOL / BF16_MEAN_TOL), asserted at :206 / :225;
  fp16  a quarter of the bf16 bounds: tests/test_from_hf_gpu.py:20 (F16_MAX_TOL / F16_MEAN_TOL), asserted at :92.
  16-bit LSE: |lse(a) - lse(b)| <= max |a - b|, so the maximum bound of the logits holds for it as well.
  scores of two forms of one decode: 1e-3, tests/test_staged_verify_gpu.py:19 (SCORE_TOL), asserted at :59.
Tiny models (hidden 256, 2 heads of 128 so that the fused RoPE epilogue applies, ffn 512, 384 tokens); the oracle's logits of a case are computed
once per dtype and layer count and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, release_decoders, target_generate_batch
from atspeed_amd.model import HipLlama, vis_bits_from_bool
from oracle.llama_ref import RefLlama
from tests.golden.cases import CASES, build_case_inputs
from tests.guard import assert_same

NEVER = 1 << 30
V, HIDDEN, HEADS, FFN, SLOTS = 384, 256, 2, 512, 512
LOGIT_TOL = 1e-3
BF16_MAX_TOL, BF16_MEAN_TOL = 0.04, 0.006
F16_MAX_TOL, F16_MEAN_TOL = BF16_MAX_TOL / 4, BF16_MEAN_TOL / 4
SCORE_TOL = 1e-3
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# (n_tok, n_logit) per segment.  mixed: T = 280 (the full form's projections take the ring family), R = 56 (the compact ones the small-M
# family), logit rows at odd and at even rows of the packed layout, a segment without logit rows, one that is all logit rows.  mixed_odd: the
# same with one logit row less, R = 55: the compact operands end in a pad row.  wide: T = 700, R = 260 >= 257: the compact side is a ring
# launch too.
CASES_SEGS = {"mixed": [(1, 1), (5, 1), (70, 1), (33, 33), (40, 0), (131, 20)],
              "mixed_odd": [(1, 1), (5, 1), (70, 1), (33, 33), (40, 0), (131, 19)],
              "wide": [(150, 60), (150, 60), (150, 60), (150, 60), (100, 20)]}
NEW = 20                                       # tokens per segment of the second round


def _segments(case):
    """per segment: ids, pos, slots, vis (bool [n_tok, n_tok]) of a causal prompt with one hidden slot; then the second round's NEW tokens"""
    g = torch.Generator().manual_seed(17 + len(CASES_SEGS[case]))
    first, second = [], []
    for n, nl in CASES_SEGS[case]:
        ids = torch.randint(3, V, (n,), generator=g).to(torch.int32)
        vis = torch.tril(torch.ones(n, n, dtype=torch.bool))
        if n > 12:
            vis[8:, 3] = False
        first.append((ids, torch.arange(n, dtype=torch.int32), torch.arange(n, dtype=torch.int32), vis, n, nl))
        ids2 = torch.randint(3, V, (NEW,), generator=g).to(torch.int32)
        vis2 = torch.cat((torch.ones(NEW, n, dtype=torch.bool), torch.tril(torch.ones(NEW, NEW, dtype=torch.bool))), 1)
        if n > 12:
            vis2[:, 3] = False
        second.append((ids2, torch.arange(n, n + NEW, dtype=torch.int32), torch.arange(n, n + NEW, dtype=torch.int32), vis2, n + NEW, NEW))
    return first, second


def _bits(seqs):
    return [(i, p, s, vis_bits_from_bool(v, SLOTS), ns, nl) for i, p, s, v, ns, nl in seqs]


_MODELS, _ORACLE = {}, {}


def _model(dtype, layers):
    """one model per (dtype, layer count) for the whole module: fp32 weights of one seed, converted by value"""
    key = (dtype, layers)
    if key not in _MODELS:
        dims = synth.LlamaDims(V, HIDDEN, layers, HEADS, FFN)
        sd = synth.synthetic_state_dict(dims, 31, std=0.05, head_std=0.1)
        _MODELS[key] = HipLlama.from_state_dict(dims, sd, DTYPES[dtype], max_slots=SLOTS, max_tokens=512, max_logit_rows=128)
    return _MODELS[key]


def _oracle(dtype, layers, case):
    """(logits of the first forward, logits of the second round), each [R, V] fp32, from one RefLlama per segment on the device's weight values"""
    key = (dtype, layers, case)
    if key not in _ORACLE:
        m = _model(dtype, layers)
        sd = m.export_state_dict()
        first, second = _segments(case)
        a, b = [], []
        for s1, s2 in zip(first, second):
            ref = RefLlama(m.dims, sd, max_slots=SLOTS)
            a.append(ref.forward(s1[0], s1[1], s1[2], s1[3], n_logit_rows=s1[5]))
            b.append(ref.forward(s2[0], s2[1], s2[2], s2[3], n_logit_rows=s2[5]))
        _ORACLE[key] = (torch.cat(a), torch.cat(b))
    return _ORACLE[key]


def _read(m, what, index, nbytes, dtype=torch.uint8):
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().atspeed_llama_read(m._handle, what, index, out.data_ptr(), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.view(dtype).cpu()


def _lse(m, rows):
    return _read(m, 1, 0, 4 * rows, torch.float32)


def _check_against_oracle(what, dtype, got, got_lse, want):
    got, want_lse = got.float().cpu(), torch.logsumexp(want.double(), 1).float()
    err, err_lse = (got - want).abs(), (got_lse - want_lse).abs()
    scale = float(want.abs().max())
    print(f"{what} [{dtype}]: max |logit err| {float(err.max()):.3e} mean {float(err.mean()):.3e} max |lse err| {float(err_lse.max()):.3e} of max |logit| {scale:.3f}")
    if dtype == "fp32":
        assert float(err.max()) < LOGIT_TOL and float(err_lse.max()) < LOGIT_TOL
        return
    max_tol, mean_tol = (BF16_MAX_TOL, BF16_MEAN_TOL) if dtype == "bf16" else (F16_MAX_TOL, F16_MEAN_TOL)
    assert float(err.max()) < max_tol * scale and float(err.mean()) < mean_tol * scale
    assert float(err_lse.max()) < max_tol * scale


def _rows_run(m, fn):
    """fn() under the GEMM brackets -> rows each projection kind ran over"""
    m.profile(1)
    out = fn()
    torch.cuda.synchronize()
    return out, {k: v["rows"] for k, v in m.profile(0).items()}


# ------------------------------------------------------------------ 1. + 3. logits of the pruned form and of the round behind it, against the oracle
@pytest.mark.parametrize("dtype,layers,case", [("fp32", 2, "mixed"), ("bf16", 2, "mixed"), ("fp16", 2, "mixed"), ("bf16", 1, "mixed"),
                                               ("fp32", 1, "mixed"), ("bf16", 2, "mixed_odd"), ("fp16", 2, "mixed_odd"), ("fp32", 2, "mixed_odd"),
                                               ("bf16", 2, "wide"), ("fp32", 2, "wide")])
def test_pruned_logits_and_the_next_round_match_the_oracle(dtype, layers, case):
    """The pruned forward's logits and LSE meet the oracle bound of the dtype; so do those of a second forward of NEW tokens per segment that
    attend to the slots the pruned prefill wrote (what a wrong front / back split would break without the first forward showing it).  1 layer:
    the last layer is also the first, its input norm comes from the embedding."""
    m = _model(dtype, layers)
    first, second = _segments(case)
    T, R = sum(s[4] for s in first), sum(s[5] for s in first)
    want1, want2 = _oracle(dtype, layers, case)
    with _lib.switches(tail_rows_tokens=NEVER):
        full = m.forward_raw_batch(_bits(first), return_all=True).clone()
    with _lib.switches(tail_rows_tokens=0):
        got1, rows = _rows_run(m, lambda: m.forward_raw_batch(_bits(first), return_all=True).clone())
        lse1 = _lse(m, R)
        assert rows["qkv"] == layers * T and rows["o_proj"] == rows["gate_up"] == rows["down"] == (layers - 1) * T + R, rows   # the pruned form ran
        got2 = m.forward_raw_batch(_bits(second), return_all=True).clone()
        lse2 = _lse(m, NEW * len(second))
    print(f"pruned against full [{dtype}, {layers} layers, {case}]: max |d logit| {float((got1 - full).abs().max()):.3e}")
    _check_against_oracle(f"pruned prefill T={T} R={R}", dtype, got1, lse1, want1)
    _check_against_oracle("the round behind it", dtype, got2, lse2, want2)


# ------------------------------------------------------------------ 2. the caches
@pytest.mark.parametrize("dtype,layers", [("bf16", 2), ("fp32", 2), ("bf16", 1)])
def test_kv_caches_are_bit_identical(dtype, layers):
    """K and V of every layer, the last included, byte for byte what the full forward leaves; slots no token wrote stay zero (the arenas are
    zero-filled when created and this model has run nothing else)."""
    dims = synth.LlamaDims(V, HIDDEN, layers, HEADS, FFN)
    m = HipLlama.from_state_dict(dims, synth.synthetic_state_dict(dims, 31, std=0.05, head_std=0.1), DTYPES[dtype], max_slots=SLOTS, max_tokens=512,
                                 max_logit_rows=128)
    first, _ = _segments("mixed")
    esz = 4 if dtype == "fp32" else 2
    nbytes = layers * SLOTS * HIDDEN * esz
    arenas = lambda: [(_read(m, 2, i, nbytes), _read(m, 3, i, nbytes)) for i in range(len(first))]
    with _lib.switches(tail_rows_tokens=0):
        m.forward_raw_batch(_bits(first))
        pruned = arenas()
    with _lib.switches(tail_rows_tokens=NEVER):
        m.forward_raw_batch(_bits(first))
        full = arenas()
    for i, ((pk_, pv), (fk, fv)) in enumerate(zip(pruned, full)):
        assert torch.equal(pk_, fk) and torch.equal(pv, fv), f"segment {i}"
        n = first[i][4]
        for name, a in (("K", pk_), ("V", pv)):
            a = a.view(layers, SLOTS, HIDDEN * esz)
            assert not bool(a[:, n:].any()), f"segment {i}: {name} slots past the {n} written ones were touched"
            assert bool(a[layers - 1, :n].any(dim=1).all()), f"segment {i}: a written {name} slot of the last layer is all zero"


# ------------------------------------------------------------------ 4. decisions end to end
def test_decisions_are_those_of_the_full_form():
    """BSSD_batch (every round staged, so that phase 0 of round 1 is a prefill with one logit row per user) and target_generate_batch on the six
    users of tests/test_staged_verify_gpu.py's mixed batch (fp32 golden models, clear margins): tokens, accepted steps and forward counts are
    identical between the two forms, scores within SCORE_TOL."""
    case = [c for c in CASES if c["name"] == "k6_dk12_new7_gamma3_s9"][0]
    ci = build_case_inputs(case)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **kw)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **kw)
    prompts = [synth.synthetic_prompt(18 + 5 * (u % 7), 900 + u) for u in (0, 3, 6, 7, 15, 2)]
    inputs = [{"input_ids": torch.from_numpy(np.asarray(p, dtype=np.int64))[None].cuda()} for p in prompts]
    res = {}
    try:
        for name, sw in (("pruned", 0), ("full", NEVER)):
            with _lib.switches(tail_rows_tokens=sw, verify_staged=2):
                tgt.forward_log(1)
                sd = BSSD_batch(tgt, drf, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
                log = tgt.forward_log(0)
                tg = target_generate_batch(tgt, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
            res[name] = (sd, tg, [tuple(int(x) for x in e) for e in log])
    finally:
        release_decoders(tgt, drf)
    assert res["pruned"][2] == res["full"][2]
    assert any(2 * r <= t and r > 0 for t, r in res["pruned"][2]), res["pruned"][2]       # a forward the rule prunes was among them
    for which in (0, 1):
        for u, (a, b) in enumerate(zip(res["full"][which], res["pruned"][which])):
            assert torch.equal(a["beam_sequence"], b["beam_sequence"]), (which, u)
            d = float((a["beam_scores"] - b["beam_scores"]).abs().max())
            print(f"{'BSSD_batch' if which == 0 else 'target_generate_batch'} user {u}: max |d score| {d:.3e}")
            assert d <= SCORE_TOL
            for key in ("n_run", "total_accept_steps", "accept_steps", "n_target_forwards", "n_draft_forwards"):
                if key in a or key in b:
                    assert a[key] == b[key], (which, u, key, a[key], b[key])


# ------------------------------------------------------------------ 5. graph replay
def test_graph_replay_keeps_the_two_forms_apart():
    """`graphs` on: a pruned forward of a recurring shape, captured at its second call and replayed at its third, equals the directly launched
    pruned forward bit for bit; a full forward with the same (T, R, n) does not pick up the pruned graph.  At these sizes the two forms give the
    same logits bit for bit (every output row of a projection is summed in the same order whatever M is), so what tells them apart is the
    residual-stream buffer: the full form leaves the last layer's output there, the pruned one the stream in front of the last o_proj."""
    m = _model("bf16", 2)
    lib = _lib.load()
    T, R = 280, 55
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, V, (T,), generator=g).to(torch.int32).cuda()
    pos = torch.arange(T, dtype=torch.int32).cuda()
    vis = vis_bits_from_bool(torch.tril(torch.ones(T, T, dtype=torch.bool)), SLOTS)
    vis = vis.cuda()

    def run():
        _lib.check(lib.atspeed_llama_forward(m._handle, ids.data_ptr(), pos.data_ptr(), pos.data_ptr(), vis.data_ptr(), T, T, R, None, _lib.stream_ptr()))
        return (_read(m, 0, 0, 4 * R * m.logits_ld, torch.int32).view(R, m.logits_ld)[:, :V].contiguous(), _read(m, 1, 0, 4 * R, torch.int32),
                _read(m, 4, 0, 2 * T * HIDDEN, torch.int16))

    direct = {}
    for name, sw in (("pruned", 0), ("full", NEVER)):
        with _lib.switches(tail_rows_tokens=sw, graphs=0):
            direct[name] = run()
    print("graph test: logits of the two forms identical:", torch.equal(direct["pruned"][0], direct["full"][0]))
    assert not torch.equal(direct["pruned"][2], direct["full"][2]), "the two forms leave the same residual stream: this test could not tell their graphs apart"
    for name, sw in (("pruned", 0), ("full", NEVER)):       # pruned first: its graph exists when the full form arrives with the same (T, R, n)
        with _lib.switches(tail_rows_tokens=sw, graphs=1):
            for call in range(3):                           # direct, captured + launched, replayed
                lo, ls, h = run()
                assert torch.equal(lo, direct[name][0]) and torch.equal(ls, direct[name][1]) and torch.equal(h, direct[name][2]), (name, call)


# ------------------------------------------------------------------ 6. the gather alone
@pytest.mark.parametrize("dtype,packed", [("bf16", 0), ("bf16", 1), ("fp32", 0)])       # (the fp32 parity mode has no packed operands)
@pytest.mark.parametrize("case", ["mixed", "mixed_odd"])
def test_gather_guard_band(case, dtype, packed):
    """gather_tail_rows_kernel: rows < R of both outputs are the source rows exactly, in the row-major and in the packed layout, for an odd
    R (55) and an even one (56); rows >= R, the pad row of the odd count included, keep their sentinel."""
    lib = _lib.load()
    td = DTYPES[dtype]
    segs = CASES_SEGS[case]
    n_tok = [s[0] for s in segs]
    nl = [s[1] for s in segs]
    T, R, n = sum(n_tok), sum(nl), len(segs)
    assert R == (56 if case == "mixed" else 55)
    Te, cap = T + (T & 1), R + 5 + ((R + 5) & 1)
    gen = torch.Generator().manual_seed(2)
    h = torch.randn(Te, HIDDEN, generator=gen).to(td).cuda()
    att = torch.randn(Te, HIDDEN, generator=gen).to(td).cuda()
    sentinel = lambda: torch.full((cap, HIDDEN), 0x7FC1, dtype=torch.int16, device="cuda").view(td) if td != torch.float32 else \
        torch.full((cap, HIDDEN), 0x7FC00001, dtype=torch.int32, device="cuda").view(td)
    pack = lambda t, back=False: _pack(lib, t, back)
    att_in = pack(att) if packed else att
    h_out, att_out = sentinel(), sentinel()
    if packed:
        att_out = pack(att_out)                # a packed buffer whose every row is the sentinel
    cnt = lambda v: (C.c_int32 * n)(*v)
    _lib.check(lib.atspeed_segs_gather_tail_rows(h.data_ptr(), att_in.data_ptr(), HIDDEN, _lib.dtype_code(td), packed, h_out.data_ptr(), att_out.data_ptr(),
                                                 n, None, None, None, None, None, None, cnt(n_tok), cnt([1] * n), cnt(nl), _lib.stream_ptr()))
    torch.cuda.synchronize()
    if packed:
        att_out = pack(att_out, back=True)
    row0 = np.concatenate([[0], np.cumsum(n_tok)])
    rows = torch.from_numpy(np.concatenate([np.arange(row0[i] + n_tok[i] - nl[i], row0[i] + n_tok[i]) for i in range(n)])).long()
    assert any(int(r) & 1 for r in rows) and any(not int(r) & 1 for r in rows)
    want_tail = sentinel()[R:].cpu()
    assert_same("h rows", h_out[:R].cpu(), h.cpu()[rows])
    assert_same("att rows", att_out[:R].cpu(), att.cpu()[rows])
    assert_same("h rows past R", h_out[R:].cpu(), want_tail)
    assert_same("att rows past R", att_out[R:].cpu(), want_tail)


def _pack(lib, t, back):
    out = torch.empty_like(t)
    fn = lib.atspeed_unpack_rows if back else lib.atspeed_pack_rows
    _lib.check(fn(t.data_ptr(), out.data_ptr(), t.shape[0], t.shape[1] * t.element_size(), _lib.stream_ptr()))
    return out


# ------------------------------------------------------------------ 7. below the threshold nothing changes
def test_default_leaves_small_forwards_alone(bssd_golden):
    """The library's default: a one-user forward gives the bits of the full form (both run the unpruned body), and a golden BSSD case its pinned
    tokens."""
    m = _model("bf16", 2)
    T, R = 100, 1
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(3, V, (T,), generator=g).to(torch.int32).cuda()
    pos = torch.arange(T, dtype=torch.int32).cuda()
    vis = vis_bits_from_bool(torch.tril(torch.ones(T, T, dtype=torch.bool)), SLOTS).cuda()
    default, rows = _rows_run(m, lambda: m.forward_raw(ids, pos, pos, vis, T, R).clone())
    assert rows["o_proj"] == rows["qkv"] == 2 * T, rows
    with _lib.switches(tail_rows_tokens=NEVER):
        full = m.forward_raw(ids, pos, pos, vis, T, R).clone()
    with _lib.switches(tail_rows_tokens=0):
        pruned, rows = _rows_run(m, lambda: m.forward_raw(ids, pos, pos, vis, T, R).clone())
    assert rows["o_proj"] == T + R, rows                     # (the switch does reach this forward)
    assert_same("default against the full form", default.cpu(), full.cpu())
    case = [c for c in CASES if c["name"] == "k20_dk40_sigma01_s7"][0]
    gold = bssd_golden[case["name"]]
    ci = build_case_inputs(case)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    tgt = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=case["K"], **kw)
    drf = HipLlama.from_state_dict(ci["draft_dims"], ci["draft_sd"], torch.float32, num_beams=case["DK"], **kw)
    P = len(ci["prompt"])
    out = BSSD(tgt, drf, {"input_ids": torch.from_numpy(ci["prompt"])[None].cuda()}, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=ci["fn"])
    release_decoders(tgt, drf)
    assert out["beam_sequence"][:, P:].cpu().tolist() == gold["bssd_tokens"]
    np.testing.assert_allclose(out["beam_scores"].cpu().numpy(), gold["bssd_scores"], atol=SCORE_TOL, rtol=0)
    assert out["n_run"] == gold["n_run"] and out["total_accept_steps"] == gold["total_accept_steps"]
