"""The single-buffered 64-row form of the 32-rows-per-wave attention kernel (tree_attn32_kernel<DH, 2, 1>) and the rule
that selects it (ats_seg_finish, switch `attn_short`).

Bare kernel: atspeed_segs_tree_attention at explicit 64-row tiles against the fp64 softmax attention of each segment under the bound of
tests/test_segs_gpu.py (ATTN_C["rows32"]), and BIT FOR BIT against the same inputs through the 128-row double-buffered launch: the 32-row wave
groups are the same partition of a segment in both tilings, so every skip decision and every sum is the same.  The rule: tables with
qtile_rows = 0, told apart by the library's launch counters (13 = single-buffered, 14 = double-buffered).  Engine: a lock-step batch decodes
the same with the switch at 0 and at 1.  Inputs and references are built once per module.  Run with -m gpu on the MI355X box."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD_batch, release_decoders
from atspeed_amd.generation_trie import PositionSetConstraint
from atspeed_amd.model import HipLlama
from tests import guard, segs_cases as SC
from tests.guard import assert_same
from tests.test_segs_gpu import ATTN_C, EPS, POISON16, TD, Segs, _attention, _bits, _caches, _counters, _poisoned, _st, lib  # noqa: F401

ONE_BUF, TWO_BUF = 13, 14            # atspeed_gemm_path_counters: launches of tree_attn32_kernel by tile buffers


def _table(n_tok, n_slots, seed, vis_of=None):
    """a segment set in the format of segs_cases.segments: random visibility (0.3, slot 0 always), vis_of(i, vis) edits segment i's in place"""
    rng = np.random.default_rng(seed)
    segs = []
    for i, (t, s) in enumerate(zip(n_tok, n_slots)):
        vis = rng.random((t, s)) < 0.3
        vis[:, 0] = True
        if vis_of:
            vis_of(i, vis)
        z = np.zeros(t, dtype=np.int32)
        segs.append(dict(ids=z, pos=z, slots=z, vis=vis))
    row0 = np.concatenate([[0], np.cumsum(n_tok)])
    return dict(n=len(segs), segs=segs, n_tok=list(n_tok), n_slots=list(n_slots), n_logit=[0] * len(segs), row0=row0, total_tok=int(row0[-1]))


def _device(sg):
    S = Segs.__new__(Segs)
    S.sg = sg
    z = [torch.zeros(t, dtype=torch.int32, device="cuda") for t in sg["n_tok"]]
    S.ids = S.pos = S.slots = z
    S.vis = [torch.from_numpy(SC.vis_words(s["vis"]).view(np.int64)).cuda() for s in sg["segs"]]
    S.kc = S.vc = None
    return S


# ------------------------------------------------------------------ the bare kernel
# rows 1, 20, 32, 33, 40, 64 x slots 1, 64, 65, 128, 129, 170 -- every pair of a full / ragged wave with a full / ragged last key tile
SHORT_TOK = [1, 20, 32, 33, 40, 64, 64, 21, 64]            # (an odd total: the packed output has a pad row)
SHORT_SLOTS = [1, 129, 64, 65, 170, 128, 170, 170, 129]


def _short_vis(i, vis):
    t, s = vis.shape
    if i == 0:
        vis[:] = True                                     # one row, one slot
    if i == 1:                                            # the tree shape: a prefix of 100 slots, then a row's ancestors (every 4th row above it) and itself
        vis[:] = False
        vis[:, :100] = True
        for r in range(t):
            for a in range(r % 4, r + 1, 4):
                vis[r, 100 + a] = True
    if i == 3:
        vis[5] = False                                    # a row that sees nothing at all
    if i == 4:
        vis[:, 64:128] = False                            # a middle key tile that no row of the segment sees
    if i == 5:
        vis[32:, :64] = False; vis[32:, 64] = True        # the second wave sees nothing in tile 0, which the first wave needs
    if i == 6:
        vis[:32, 128:] = False                            # the first wave sees nothing in the last (ragged) tile, which the second needs
        vis[40] = False; vis[40, 169] = True              # a row that sees only the segment's last slot
    if i == 7:
        vis[:, :128] = False; vis[:, 128] = True          # a segment whose first two tiles nobody sees
        vis[19] = False                                   # ... and one row nothing


@functools.lru_cache(maxsize=None)
def _short_case(n_heads, head_dim, dtype):
    """the table, its inputs as values of the format (fp64) and the fp64 reference of layer 1: (sg, q, kc, vc, ref, mag)"""
    sg = _table(SHORT_TOK, SHORT_SLOTS, 6400 + head_dim, _short_vis)
    rng = np.random.default_rng(6500 + n_heads)
    H = n_heads * head_dim
    q = SC.to_dtype64(rng.standard_normal((sg["total_tok"], 3 * H)), dtype)
    kc = [SC.to_dtype64(rng.standard_normal((SC.LAYERS, SC.MAX_SLOTS, H)), dtype) for _ in range(sg["n"])]
    vc = [SC.to_dtype64(rng.standard_normal((SC.LAYERS, SC.MAX_SLOTS, H)), dtype) for _ in range(sg["n"])]
    ref, mag = np.zeros((sg["total_tok"], H)), np.zeros((sg["total_tok"], H))
    for i, s in enumerate(sg["segs"]):
        T, Sn, r0 = sg["n_tok"][i], sg["n_slots"][i], int(sg["row0"][i])
        qs = q[r0: r0 + T, :H].reshape(T, n_heads, head_dim)
        k, v = kc[i][1, :Sn].reshape(Sn, n_heads, head_dim), vc[i][1, :Sn].reshape(Sn, n_heads, head_dim)
        sc = np.where(s["vis"][None], np.einsum("thd,shd->hts", qs, k) / np.sqrt(head_dim), -np.inf)
        mx = np.where(np.isfinite(sc.max(-1, keepdims=True)), sc.max(-1, keepdims=True), 0.0)
        p = np.exp(sc - mx)
        p /= np.maximum(p.sum(-1, keepdims=True), 1e-300)                 # a row that sees nothing: all zeros
        ref[r0: r0 + T] = np.einsum("hts,shd->thd", p, v).reshape(T, H)
        mag[r0: r0 + T] = np.einsum("hts,shd->thd", p, np.abs(v)).reshape(T, H)
    return sg, q, kc, vc, ref, mag


@pytest.mark.parametrize("n_heads,head_dim,dtype", [(2, 128, "bf16"), (4, 64, "bf16"), (2, 128, "fp16")])
def test_single_buffered_tiles(lib, n_heads, head_dim, dtype):
    """64-row tiles on the 32-rows-per-wave kernel: fp64 reference, bit identity with the 128-row launch, poison past total_tok, packed output"""
    sg, q64, kc64, vc64, ref, mag = _short_case(n_heads, head_dim, dtype)
    td, H, T = TD[dtype], n_heads * head_dim, sg["total_tok"]
    S = _device(sg)
    q = torch.from_numpy(q64).to(td).cuda()
    S.kc, S.vc = _caches(sg, H, td, kc64), _caches(sg, H, td, vc64)
    c0 = _counters(lib)
    out = _attention(lib, S, q, H, n_heads, head_dim, td, 1, 64, 32, 0)
    c1 = _counters(lib)
    assert (c1[ONE_BUF] - c0[ONE_BUF], c1[TWO_BUF] - c0[TWO_BUF]) == (1, 0)
    got = out[:T].double().cpu().numpy()
    err = np.abs(got - ref)
    blind = ~np.concatenate([s["vis"].any(1) for s in sg["segs"]])
    assert blind.sum() == 2 and (got[blind] == 0).all(), "a row that sees nothing returns zeros"
    ratio = float((err[~blind] / (EPS[dtype] * mag[~blind])).max())
    print(f"single-buffered attention heads={n_heads} dh={head_dim} {dtype}: max|err|={err.max():.3e} worst |err| / (eps sum p|v|) = {ratio:.3f}")
    assert err.max() <= 3e-2
    assert ratio <= ATTN_C["rows32"], (ratio, ATTN_C["rows32"])
    assert_same("rows past total_tok", out[T:].cpu(), _poisoned((out.shape[0] - T, H), td).cpu())
    wide = _attention(lib, S, q, H, n_heads, head_dim, td, 1, 128, 32, 0)
    c2 = _counters(lib)
    assert (c2[ONE_BUF] - c1[ONE_BUF], c2[TWO_BUF] - c1[TWO_BUF]) == (0, 1)
    assert_same("64-row single-buffered vs 128-row double-buffered", out.cpu(), wide.cpu())
    if dtype == "bf16":                                   # (the packed operand is bf16's)
        pk = _attention(lib, S, q, H, n_heads, head_dim, td, 1, 64, 32, 1, rows_extra=2)
        Tp = (T + 1) // 2 * 2
        want = torch.empty(Tp, H, dtype=td, device="cuda")
        _lib.check(lib.atspeed_pack_rows(out[:T].contiguous().data_ptr(), want.data_ptr(), T, H * 2, _st()))
        torch.cuda.synchronize()
        gb, wb = pk[:Tp].contiguous().view(torch.uint8).reshape(-1), want.view(torch.uint8).reshape(-1).clone()
        assert T & 1
        pad = guard.packed_row_offsets(T, H * 2).cuda()
        assert (gb[pad].view(torch.int16) == POISON16).all(), "the pad row of the packed output was written"
        wb[pad] = gb[pad]
        assert torch.equal(gb, wb), "packed output differs from atspeed_pack_rows of the row-major output"
        assert (_bits(pk[Tp:]) == POISON16).all()


# ------------------------------------------------------------------ the rule
@functools.lru_cache(maxsize=None)
def _rule_table(kind):
    rng = np.random.default_rng(7700)
    tok = [int(v) for v in rng.integers(1, 65, 32)]
    tok[3], tok[9] = 64, 20
    if kind == "n16":
        tok = tok[:16]
    elif kind == "n16_one65":
        tok = tok[:16]; tok[11] = 65
    elif kind == "n15":
        tok = tok[:15]
    elif kind == "n15_long":
        tok = [100 + t for t in tok[:15]]
    slots = [min(SC.MAX_SLOTS, t + int(v)) for t, v in zip(tok, rng.integers(0, 140, 32))]
    return _table(tok, slots, 7701)


# (table, switch, the tile height the rule gives, the counter that moves)
RULE = [("n16", 1, 64, ONE_BUF), ("n32", 1, 64, ONE_BUF), ("n16_one65", 1, 128, TWO_BUF), ("n15", 1, 64, ONE_BUF), ("n15_long", 1, 128, TWO_BUF),
        ("n16", 0, 128, TWO_BUF), ("n32", 0, 128, TWO_BUF), ("n15", 0, 64, ONE_BUF)]


@pytest.mark.parametrize("kind,switch,height,counter", RULE)
def test_rule(lib, kind, switch, height, counter):
    """qtile_rows = 0: at least 16 segments of at most 64 rows take 64-row tiles; one segment of 65 rows, or the switch at 0, keeps 128; fewer
    than 16 segments take what they took (64 unless half of them exceed 96 rows).  Told by the counters and equal to the explicit launch."""
    sg = _rule_table(kind)
    n_heads, head_dim, td = 4, 64, torch.bfloat16
    H = n_heads * head_dim
    S = _device(sg)
    g = torch.Generator().manual_seed(7702)
    q = torch.randn(sg["total_tok"], 3 * H, generator=g).to(td).cuda()
    S.kc = [torch.randn(SC.LAYERS, SC.MAX_SLOTS, H, generator=g).to(td).cuda() for _ in range(sg["n"])]
    S.vc = [torch.randn(SC.LAYERS, SC.MAX_SLOTS, H, generator=g).to(td).cuda() for _ in range(sg["n"])]
    with _lib.switches(attn_short=switch):
        c0 = _counters(lib)
        auto = _attention(lib, S, q, H, n_heads, head_dim, td, 0, 0, 32, 0)
        c1 = _counters(lib)
        other = ONE_BUF + TWO_BUF - counter
        assert (c1[counter] - c0[counter], c1[other] - c0[other]) == (1, 0), (kind, switch)
        assert_same("the rule's launch vs the explicit one", auto.cpu(), _attention(lib, S, q, H, n_heads, head_dim, td, 0, height, 32, 0).cpu())
        # everything automatic (the kernel family too: 16 rows per wave at these grids) is the explicit launch at the same height
        assert_same("automatic vs explicit", _attention(lib, S, q, H, n_heads, head_dim, td, 0, 0, 0, 0).cpu(),
                    _attention(lib, S, q, H, n_heads, head_dim, td, 0, height, 0, 0).cpu())


# ------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def pair():
    """a bf16 pair of 16 heads x 64 whose lock-step batches of 32 users reach the 32-rows-per-wave kernel (512 workgroups), weights aligned so that
    verification accepts draft blocks"""
    V = synth.BEAUTY.vocab_size
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448)
    drf = HipLlama.from_synthetic(synth.LlamaDims(V, 1024, 2, 16, 1408), 52, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=40, resid_scale=3e-5, **kw)
    tgt = HipLlama.from_synthetic(synth.LlamaDims(V, 1024, 2, 16, 2752), 51, std=0.03, head_std=0.2, dtype=torch.bfloat16, num_beams=20, resid_scale=3e-5,
                                  align_to=drf, **kw)
    fn = PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    inputs = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(30 + 7 * (u % 5), 300 + u))[None].cuda()} for u in range(32)]
    yield tgt, drf, fn, inputs
    release_decoders(tgt, drf)


@pytest.mark.parametrize("graphs", [0, 1])
def test_engine_lock_step(lib, pair, graphs):
    """BSSD_batch of 32 users, every round staged (20-row round inputs, 40-row blocks): tokens, scores and every counter are the same with the
    switch at 0 and at 1, and only the run at 1 launches the single-buffered form"""
    tgt, drf, fn, inputs = pair
    runs, launched = [], []
    for short in (0, 1):
        with _lib.switches(attn_short=short, verify_staged=2, graphs=graphs):
            c0 = _counters(lib)
            runs.append(BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn))
            torch.cuda.synchronize()
            c1 = _counters(lib)
            launched.append((c1[ONE_BUF] - c0[ONE_BUF], c1[TWO_BUF] - c0[TWO_BUF]))
    print("attention launches (single-buffered, double-buffered) with attn_short 0 / 1:", launched)
    if not graphs:                                        # (a replayed graph launches without passing the counters)
        assert launched[0][0] == 0 and launched[0][1] > 0 and launched[1][0] > 0
    assert sum(sum(o["accept_steps"]) for o in runs[0]) > 0, "no draft block was accepted: no phase beyond the first ran"
    for u, (a, b) in enumerate(zip(runs[0], runs[1])):
        assert torch.equal(a["beam_sequence"], b["beam_sequence"]), u
        assert torch.equal(a["beam_scores"], b["beam_scores"]), u
        for key in ("n_run", "total_accept_steps", "accept_steps", "n_valid", "n_target_forwards", "n_draft_forwards", "n_target_passes"):
            assert a[key] == b[key], (u, key, a[key], b[key])
