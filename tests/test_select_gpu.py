"""The selection and LSE kernels of atspeed_amd/csrc/scan.hip on the placed and tied inputs of tests/select_cases.py, through the C ABI:
which wave, slot and chunk holds which winner is chosen, equal scores are everywhere, and the expected scores are exact (dyadic values,
lse = 0), so ids, order and score bits are all pinned.  tests/test_select_cpu.py checks the cases themselves."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib, synth
from tests import select_cases as S

EXPAND = {c.name: c for c in S.expand_cases()}
TOPK = {c.name: c for c in S.topk_cases()}
FREE = {c.name: c for c in S.free_cases()}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    l = _lib.load()
    assert l.atspeed_device_count() >= 1
    return l


def _st():
    return _lib.stream_ptr()


def _padded(rows, fill=float("nan")):
    """[n, vocab] -> device [n, ld], ld the next multiple of 64, the padding columns NaN: a kernel that read one would select it"""
    rows = torch.as_tensor(rows)
    ld = (rows.shape[1] + 63) // 64 * 64
    out = torch.full((rows.shape[0], ld), fill)
    out[:, : rows.shape[1]] = rows
    return out.cuda(), ld


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _check_picks(got, exp, k, node=True):
    """got: (score, parent, token, node, flat) device tensors of k entries"""
    flat = exp["flat"]
    n = sum(f >= 0 for f in flat)
    o_s, o_p, o_t, o_n, o_f = (g.cpu() if g is not None else None for g in got)
    assert o_f.tolist() == flat                                           # ids in order, -1 past the live count
    assert o_p[:n].tolist() == exp["parent"] and o_t[:n].tolist() == exp["token"]
    if node:
        assert o_n[:n].tolist() == exp["node"]
    assert torch.equal(_bits(o_s[:n]), _bits(torch.from_numpy(np.ascontiguousarray(exp["score"], np.float32))))      # score bits, no tolerance


# ------------------------------------------------------------------ expand + prune through hand-made automata
@pytest.mark.parametrize("name", list(EXPAND))
def test_expand_prune_placed(lib, name):
    c = EXPAND[name]
    lg, ld = _padded(c.logits)
    lse = torch.zeros(c.rows, device="cuda")
    bs, nd = torch.from_numpy(c.bscore).cuda(), torch.from_numpy(c.node).cuda()
    with _lib.Handle.create("atspeed_fsm_destroy", lib.atspeed_fsm_create, c.row_ptr.ctypes.data, c.tok.ctypes.data, c.nxt.ctypes.data,
                            c.n_nodes, len(c.tok), c.vocab) as fsm:
        runs = []
        for _ in range(2):
            o_s = torch.full((c.k,), 7.0, device="cuda")
            o_p, o_t, o_n, o_f = (torch.full((c.k,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
            _lib.check(lib.atspeed_beam_expand_prune(lg.data_ptr(), ld, lse.data_ptr(), bs.data_ptr(), nd.data_ptr(), c.rows, fsm.ptr, c.k,
                                                     o_s.data_ptr(), o_p.data_ptr(), o_t.data_ptr(), o_n.data_ptr(), o_f.data_ptr(), _st()))
            torch.cuda.synchronize()
            runs.append((o_s, o_p, o_t, o_n, o_f))
    _check_picks(runs[0], c.expected(), c.k)
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))                            # the second call answers the same, bit for bit


# ------------------------------------------------------------------ row top-k and the mask-free expand
@pytest.mark.parametrize("name", list(TOPK))
def test_row_topk_placed(lib, name):
    c = TOPK[name]
    lg, ld = _padded(c.rows)
    n = len(c.rows)
    runs = []
    for _ in range(2):
        out = torch.full((n, _lib.MAX_BEAMS), -7, dtype=torch.int32, device="cuda")
        _lib.check(lib.atspeed_row_topk(lg.data_ptr(), n, c.vocab, ld, c.k, out.data_ptr(), _st()))
        torch.cuda.synchronize()
        runs.append(out.cpu())
    assert runs[0].tolist() == c.expected().tolist()                      # whole rows: the -1 fill up to ATSPEED_MAX_BEAMS included
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("name", list(FREE))
def test_free_expand_placed(lib, name):
    c = FREE[name]
    lg, ld = _padded(c.rows)
    n = len(c.rows)
    lse = torch.zeros(n, device="cuda")
    bs = torch.from_numpy(c.bscore).cuda()
    runs = []
    for _ in range(2):
        ws = torch.full((n * _lib.MAX_BEAMS,), -7, dtype=torch.int32, device="cuda")
        o_s = torch.full((c.k,), 7.0, device="cuda")
        o_p, o_t, o_f = (torch.full((c.k,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        _lib.check(lib.atspeed_beam_expand_prune_free(lg.data_ptr(), ld, lse.data_ptr(), bs.data_ptr(), n, c.vocab, c.k, ws.data_ptr(),
                                                      o_s.data_ptr(), o_p.data_ptr(), o_t.data_ptr(), o_f.data_ptr(), _st()))
        torch.cuda.synchronize()
        runs.append((o_s, o_p, o_t, None, o_f))
    _check_picks(runs[0], c.expected(), c.k, node=False)
    for a, b in zip(*runs):
        assert a is None or torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ LSE
# Allowed |err| / (2e-6 |ref| + 1e-6) per family of tests/select_cases.lse_case.  1.0 = the project's bound as it stands, and no family
# needed more: the worst ratios measured on an MI355X over all 36 vocabularies were a 0.052, b 0.000, d 0.024, e 0.077 (both kernel forms).
# A family that exceeds 1 on a correct kernel gets twice its measured worst ratio, 8 at most, with the reason written here.  c, f and g have
# closed-form answers and are held to those instead (c came within 0.40 of its 1e-6 + 2^-23 |ref|).
LSE_FACTOR = {"a": 1.0, "b_full": 1.0, "b_partial": 1.0, "b_tail": 1.0, "d": 1.0, "e": 1.0}


def _run_lse(lib, c):
    xd = c.x.cuda()
    runs = []
    for _ in range(2):
        out = torch.full((c.rows,), 7.0, device="cuda")
        _lib.check(lib.atspeed_lse_rows(xd.data_ptr(), c.rows, c.vocab, c.ld, out.data_ptr(), _st()))
        torch.cuda.synchronize()
        runs.append(out.cpu())
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    return runs[0].double().numpy()


def _check_lse(c, got):
    """per row against the fp64 reference; prints the worst |err| / bound of every family before it asserts"""
    x = c.x[:, : c.vocab]
    worst, bad = {}, []
    for r, fam in enumerate(c.families):
        ref = c.ref[r]
        if np.isneginf(ref):                                              # g, or e on a vocabulary that is all scalar tail
            ok, ratio = np.isneginf(got[r]), 0.0
        elif fam == "f":                                                  # one finite entry: that entry, exactly
            ok, ratio = got[r] == float(x[r][torch.isfinite(x[r])][0]), 0.0
        elif fam == "c":
            ratio = abs(got[r] - ref) / (1e-6 + 2.0 ** -23 * abs(ref))
            ok = ratio <= 1.0
        else:
            ratio = abs(got[r] - ref) / S.lse_bound(ref)
            ok = ratio <= LSE_FACTOR[fam]
        worst[fam] = max(worst.get(fam, 0.0), float(ratio)) if np.isfinite(got[r]) or np.isneginf(ref) else float("inf")
        if not ok:
            bad.append((r, fam, float(got[r]), float(ref)))
    print(c.name, "worst |err| / bound:", " ".join(f"{f}={v:.3f}" for f, v in sorted(worst.items())))
    assert not bad, bad[:8]


@pytest.mark.parametrize("vname,vocab", S.lse_vocabs(512), ids=[n for n, _ in S.lse_vocabs(512)])
def test_lse_rows_512_threads(lib, vname, vocab):
    """fewer than 1024 rows: lse_rows_kernel<512>, rows = 3 with three families per launch, then rows = 1 with one"""
    fams = S.LSE_FAMILIES
    for g0 in range(0, len(fams), 3):
        c = S.lse_case(vname, vocab, 3, fams[g0: g0 + 3], seed=g0)
        assert c.nt == 512
        _check_lse(c, _run_lse(lib, c))
    for i, f in enumerate(fams):
        c = S.lse_case(vname, vocab, 1, [f], seed=10 + i)
        _check_lse(c, _run_lse(lib, c))


@pytest.mark.parametrize("vname,vocab", S.lse_vocabs(256), ids=[n for n, _ in S.lse_vocabs(256)])
def test_lse_rows_256_threads(lib, vname, vocab):
    """1024 rows: lse_rows_kernel<256>; row r holds family r % 9, so every family meets every loop shape"""
    c = S.lse_case(vname, vocab, 1024, S.LSE_FAMILIES)
    assert c.nt == 256
    _check_lse(c, _run_lse(lib, c))


# ------------------------------------------------------------------ fused lm_head + LSE: a dominant logit in a tile that is not stored
@pytest.mark.parametrize("rows,vocab,hidden", S.LMHEAD_SHAPES)
def test_lmhead_lse_dominant_unstored_tile(lib, rows, vocab, hidden):
    """operands of test_kernels_gpu.py::test_lmhead_lse_fused_epilogue; three rows get a logit of about 40 in column 0, in a column of a tile the
    automaton does not store, and in the last column: the (max, sum) partial of that tile must reach the normaliser whether or not the tile is
    written.  300 rows take the plain GEMM + atspeed_lse_rows (a grid of 40 tiles is too thin for the fused epilogue), 2100 the fused path."""
    x = torch.from_numpy(synth.hash_normal(rows * hidden, 61, 1.0).reshape(rows, hidden)).to(torch.bfloat16)
    w = torch.from_numpy(synth.hash_normal(vocab * hidden, 62, 0.08).reshape(vocab, hidden)).to(torch.bfloat16)
    plants = S.lmhead_plants(rows)
    w = S.plant_dominant(x, w, plants)
    ref_lse = torch.logsumexp(x.double() @ w.double().T, dim=1)
    assert all(ref_lse[r] > 39.0 for r, _ in plants)
    x, w = x.cuda(), w.cuda()
    ld = (vocab + 63) // 64 * 64
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    toks = np.array(S.LMHEAD_FSM_TOKENS, np.int32)
    row_ptr, nxt = np.array([0, len(toks), len(toks)], np.int32), np.ones(len(toks), np.int32)
    with _lib.Handle.create("atspeed_fsm_destroy", lib.atspeed_fsm_create, row_ptr.ctypes.data, toks.ctypes.data, nxt.ctypes.data, 2, len(toks),
                            vocab) as fsm:
        for use_fsm in (False, True):
            SENT = -12345.0
            logits = torch.full((rows, ld), SENT, dtype=torch.float32, device="cuda")
            lse = torch.empty(rows, dtype=torch.float32, device="cuda")
            fused = C.c_int32(-1)
            _lib.check(lib.atspeed_lmhead_lse(x.data_ptr(), w.data_ptr(), logits.data_ptr(), lse.data_ptr(), rows, vocab, hidden, ld,
                                              fsm.ptr if use_fsm else None, ws.data_ptr(), ws.numel(), C.byref(fused), _st()))
            torch.cuda.synchronize()
            assert fused.value == S.LMHEAD_FUSED[rows]
            np.testing.assert_allclose(lse.cpu().double().numpy(), ref_lse.numpy(), atol=2e-4, rtol=0)
            for r, col in plants:
                stored = not (use_fsm and fused.value) or col // 256 in {t // 256 for t in S.LMHEAD_FSM_TOKENS}
                assert (float(logits[r, col]) != SENT) == stored          # on the fused path the dominant tile really is unwritten
