"""The sampled beam step and the two verify walks of atspeed_amd/csrc/scan.hip on the cases of tests/walk_cases.py, through their bare
entry points (atspeed_beam_sample_step, atspeed_verify_walk) against the fp64 reference tests/walk_ref.py.

Every operand is a tests/guard.py arena view: inputs sit in NaN / INT_MAX poison, every output buffer starts as seeded random bytes and is
compared WHOLE with "what it held before, with the documented rows and words replaced by the reference's": a pending walk writes
n_matches alone (and the trace of the steps it took), dnext is untouched unless every block was accepted, nothing past k entries, past the
written prefix of a suffix row or outside a buffer changes.  Decisions, ids, parents, nodes, suffixes, ids / pos / slot / vis of next and
dnext, the mailbox and the trace are exact; scores are exact to the bit on the placed family and within
2 * 2^-24 * (|logit - lse| + |logit - lse| / T + |score|) of fp64 on the natural one; tab_lse is within select_cases.lse_bound.  Nothing is
excused at run time: tests/test_walk_cpu.py proves that every case's decision margins clear 1e-4 in the reference alone.

A sampled walk reads the draft's tables.  They are made here by the step kernel itself on the draft's inputs (and checked), as a round makes
them: the zero-mass fallback needs p == q to the bit, i.e. the draft's block LSE and the walk's formed by the same code.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib
from tests import guard
from tests import select_cases as S
from tests import walk_cases as W
from tests import walk_ref as R

STEP = {c.name: c for c in W.step_cases()}
SWALK = {c.name: c for c in W.sampled_walk_cases()}
GWALK = {c.name: c for c in W.greedy_walk_cases()}
MAXB, LMAX, GAMMA = R.MAXB, R.LMAX, R.GAMMA


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    l = _lib.load()
    assert l.atspeed_device_count() >= 1
    return l


def _st():
    return _lib.stream_ptr()


def _t(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


class Automaton:
    """the case's automaton (and its one user's filter) as library handles"""

    def __init__(self, lib, fsm, mask_seqs):
        self.fsm = _lib.Handle.create("atspeed_fsm_destroy", lib.atspeed_fsm_create, fsm.row_ptr.ctypes.data, fsm.tok.ctypes.data,
                                      fsm.nxt.ctypes.data, fsm.n_nodes, len(fsm.tok), fsm.vocab)
        if fsm.filter_min > 0:
            _lib.check(lib.atspeed_fsm_set_id_filter(self.fsm.ptr, fsm.filter_min, fsm.filter_eos))
        self.masks = None
        if mask_seqs:
            toks = np.asarray([t for q in mask_seqs for t in q], np.int32)
            soff = np.asarray(np.concatenate(([0], np.cumsum([len(q) for q in mask_seqs]))), np.int32)
            uoff, start = np.asarray([0, len(mask_seqs)], np.int32), np.zeros(1, np.int32)
            unknown, status = np.full(1, -99, np.int32), np.full(1, -99, np.int32)
            self.masks = _lib.Handle.create("atspeed_node_masks_destroy", lib.atspeed_node_masks_create, self.fsm.ptr, 1, start.ctypes.data,
                                            toks.ctypes.data, soff.ctypes.data, uoff.ctypes.data, _lib.MASK_BLOCK, unknown.ctypes.data,
                                            status.ctypes.data, _st())
            assert unknown[0] == 0 and status[0] == 0
            words = np.zeros((fsm.n_nodes + 31) // 32, np.uint32)
            _lib.check(lib.atspeed_node_masks_read(self.masks.ptr, 0, words.ctypes.data, len(words)))
            got = [(int(words[n >> 5]) >> (n & 31)) & 1 for n in range(fsm.n_nodes)]
            assert got == fsm.blocked.astype(int).tolist(), "the filter blocks exactly the case's nodes"

    @property
    def mask_ptr(self):
        return self.masks.ptr if self.masks else None

    @property
    def fsm_addr(self):
        return self.fsm.ptr.value

    @property
    def mask_addr(self):
        return self.masks.ptr.value if self.masks else None

    def close(self):
        if self.masks:
            self.masks.close()
        self.fsm.close()


def _before(v):
    """what an output view's payload held at snapshot()"""
    return v.saved[v.off: v.off + v.nbytes].view(v.dtype).view(v.rows, v.ld)[:, : v.cols].clone()


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64).astype(np.float32))


def _check_scores(name, got, want64, bound, exact):
    """got fp32 tensor, want64 / bound fp64 arrays.  Placed: bit for bit.  Natural: |got - want| <= bound (infinities alike)"""
    got = got.cpu()
    if exact:
        guard.assert_same(name, _bits(got).reshape(1, -1), _bits(_f32(want64)).reshape(1, -1))
        return
    g = got.double().numpy()
    inf = ~np.isfinite(want64)
    assert np.array_equal(g[inf], want64[inf]), name
    err = np.abs(g[~inf] - want64[~inf])
    worst = float((err / bound[~inf]).max()) if err.size else 0.0
    print(f"{name}: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


def _padded_logits(ar, name, logits):
    ld = (logits.shape[1] + 63) // 64 * 64 + 64            # never the vocabulary itself: a row stride taken for it reads NaN
    return ar.input(name, _t(logits), ld=ld), ld


# ------------------------------------------------------------------ the sampled step
def _run_step(lib, c, am, seed=0, table=True, args=None):
    """one call on fresh arenas; returns (arena, views, status code)"""
    ar = guard.Arena("cuda", seed)
    n = len(c.bscore)
    lg, ld = _padded_logits(ar, "logits", c.logits)
    v = dict(lse=ar.input("lse", _t(c.lse)), bs=ar.input("beam_score", _t(c.bscore)), nd=ar.input("beam_node", _t(c.node)))
    cut = ar.input("cutoff", _t(c.cutoff)) if c.cutoff is not None else None
    exp = c.expected()
    o = {f: ar.output(f, 1, MAXB, torch.float32 if f == "score" else torch.int32) for f in ("score", "parent", "tok", "node", "flat")}
    o["tab_score"] = ar.output("tab_score", 1, exp["n_cand"] + 64, torch.float32)
    o["tab_off"] = ar.output("tab_off", 1, MAXB + 1, torch.int32)
    o["tab_lse"] = ar.output("tab_lse", 1, 4, torch.float32)
    o["mail"] = ar.output("mailbox", 1, 4, torch.int32)
    ar.snapshot()
    a = dict(logits=lg.ptr, ld=ld, lse=v["lse"].ptr, bs=v["bs"].ptr, nd=v["nd"].ptr, n=n, fsm=am.fsm.ptr, masks=am.mask_ptr, user=0, k=c.k,
             T=c.T, sub=c.sub, cut=cut.ptr if cut else None, filt=int(c.filter_ids), ts=o["tab_score"].ptr if table else None,
             to=o["tab_off"].ptr if table else None, tl=o["tab_lse"].ptr if table else None, mail=o["mail"].ptr)
    a.update(args or {})
    rc = lib.atspeed_beam_sample_step(a["logits"], a["ld"], a["lse"], a["bs"], a["nd"], a["n"], a["fsm"], a["masks"], a["user"], a["k"], a["T"],
                                      a["sub"], a["cut"], a["filt"], o["score"].ptr, o["parent"].ptr, o["tok"].ptr, o["node"].ptr, o["flat"].ptr,
                                      a["ts"], a["to"], a["tl"], a["mail"], _st())
    torch.cuda.synchronize()
    return ar, o, rc


def _check_step(c, ar, o, exp, table=True):
    ar.check()
    exact = c.family == "placed"
    k, n = c.k, len(c.bscore)
    for f in ("parent", "tok", "node", "flat"):
        want = _before(o[f])
        want[0, :k] = _t(exp[f]).to(want.device)
        guard.assert_same(f, o[f].t, want)
    live = exp["flat"] >= 0
    par, tok = exp["parent"][live], exp["tok"][live]
    bound = np.full(k, np.inf)
    bound[live] = W.score_bound(c.logits[par, tok], c.lse[par].astype(np.float64), c.T, exp["score"][live])
    _check_scores("score", o["score"].t[0, :k], exp["score"], bound, exact)
    want = _before(o["score"])
    want[0, :k] = o["score"].t[0, :k]
    guard.assert_same("score beyond k", o["score"].t, want)
    nc = exp["n_cand"]
    if table:
        # the table: every candidate in expand order, the offsets of the rows, the normaliser
        cr = np.repeat(np.arange(n), np.diff(exp["tab_off"]))
        ct = np.concatenate([c.fsm.tok[slice(*c.fsm.kids(c.node[r]))] for r in range(n) if c.bscore[r] > -np.inf])
        tb = W.score_bound(c.logits[cr, ct], c.lse[cr].astype(np.float64), c.T, np.where(np.isfinite(exp["tab_score"]), exp["tab_score"], 0.0))
        _check_scores("tab_score", o["tab_score"].t[0, :nc], exp["tab_score"], tb, exact)
        want = _before(o["tab_off"])
        want[0, : n + 1] = _t(exp["tab_off"]).to(want.device)
        guard.assert_same("tab_off", o["tab_off"].t, want)
        got_lse = float(o["tab_lse"].t[0, 0])
        assert abs(got_lse - exp["tab_lse"]) <= S.lse_bound(exp["tab_lse"]), (got_lse, exp["tab_lse"])
        for name, cols in (("tab_score", nc), ("tab_lse", 1)):
            want = _before(o[name])
            want[0, :cols] = o[name].t[0, :cols]
            guard.assert_same(name + " beyond its extent", o[name].t, want)
    else:
        for name in ("tab_score", "tab_off", "tab_lse"):
            guard.assert_same(name + " (no table asked for)", o[name].t, _before(o[name]))
    want = _before(o["mail"])
    want[0, 2] = exp["n_valid"]                            # status: written only when there is one to report
    guard.assert_same("mailbox", o["mail"].t, want)


@pytest.mark.parametrize("name", list(STEP))
def test_sampled_step(lib, name):
    c = STEP[name]
    exp = c.expected()
    am = Automaton(lib, c.fsm, c.mask_seqs)
    try:
        runs = []
        for _ in range(2):
            ar, o, rc = _run_step(lib, c, am)
            _lib.check(rc)
            runs.append({f: v.buf.clone() for f, v in o.items()})
        _check_step(c, ar, o, exp)
        for f in runs[0]:
            assert torch.equal(runs[0][f], runs[1][f]), f"{f}: the second call answers other bits"
        ar, o, rc = _run_step(lib, c, am, table=False)    # the same picks without a table
        _lib.check(rc)
        _check_step(c, ar, o, exp, table=False)
    finally:
        am.close()


# ------------------------------------------------------------------ the walks
class WalkRun:
    """one atspeed_verify_walk call on fresh arenas"""

    def __init__(self, lib, c, am, dtab, seed=0, patch=None):
        w = c.w
        ar = self.ar = guard.Arena("cuda", seed)
        a = self.args = _lib.WalkArgs()
        a.struct_size = C.sizeof(_lib.WalkArgs)
        self.keep = []
        for i, b in enumerate(w.blk):
            for f, arr in (("score", b["score"]), ("node", b["node"]), ("flat", b["flat"]), ("seq", b["seq"])):
                v = ar.input(f"blk{i}.{f}", _t(arr))
                getattr(a, "blk_" + f)[i] = v.ptr
        a.nb, a.dl, a.k, a.dk, a.gen_len0 = w.nb, w.dl, w.k, w.dk, w.gen_len0
        lg, a.ld = _padded_logits(ar, "logits", w.logits)
        a.logits, a.lse = lg.ptr, ar.input("lse", _t(w.lse)).ptr
        for i, r0 in enumerate(w.blk_row0):
            a.blk_row0[i] = r0
        a.blocks_ready = w.blocks_ready
        if w.fsm is not None:
            a.fsm, a.masks, a.user = am.fsm_addr, am.mask_addr, 0
        else:
            a.vocab, a.n_row_cand = w.vocab, w.n_row_cand
            a.row_cand = ar.input("row_cand", _t(w.row_cand)).ptr
        a.n0 = w.n0
        for f in ("ids", "pos", "slot", "vis"):
            setattr(a, "cur_" + f, ar.input("cur." + f, _t(w.cur[f])).ptr)
        o = self.out = {}
        for blk, rows in (("next", MAXB), ("dnext", 2 * MAXB)):
            for f in ("ids", "pos", "slot"):
                o[f"{blk}.{f}"] = ar.output(f"{blk}.{f}", 1, rows, torch.int32)
            o[f"{blk}.vis"] = ar.output(f"{blk}.vis", rows, w.W, torch.int64)
            for f in ("ids", "pos", "slot", "vis"):
                setattr(a, f"{blk}_{f}", o[f"{blk}.{f}"].ptr)
        for f in ("score", "node", "parent", "tok", "flat"):
            o["res." + f] = ar.output("res." + f, 1, MAXB, torch.float32 if f == "score" else torch.int32)
            setattr(a, "res_" + f, o["res." + f].ptr)
        o["res.seq"] = ar.output("res.seq", MAXB, LMAX, torch.int32)
        a.res_seq = o["res.seq"].ptr
        o["mail"] = ar.output("mailbox", 1, 4, torch.int32)
        a.mailbox = o["mail"].ptr
        o["vtrace"] = ar.output("vtrace", (GAMMA + 1) * 3, MAXB, torch.int32)
        a.vtrace = o["vtrace"].ptr if w.vtrace else None
        a.vis_words, a.sample, a.temperature, a.seed, a.round = w.W, int(w.sample), w.T, w.seed, w.round
        for i, t in enumerate(dtab):
            a.dtab_score[i], a.dtab_off[i], a.dtab_lse[i] = t["score"].data_ptr(), t["off"].data_ptr(), t["lse"].data_ptr()
        if w.cutoff is not None:
            a.cutoff = ar.input("cutoff", _t(w.cutoff)).ptr
        for f, val in (patch or {}).items():
            if isinstance(val, tuple):
                getattr(a, f)[val[0]] = val[1]
            else:
                setattr(a, f, val)
        ar.snapshot()
        self.rc = lib.atspeed_verify_walk(C.byref(a), _st())
        torch.cuda.synchronize()

    def untouched(self):
        self.ar.check()
        for name, v in self.out.items():
            guard.assert_same(name + " (a refused or pending call writes nothing here)", v.t, _before(v))


def _draft_tables(lib, c, am):
    """the draft's steps through the step kernel: its blocks are the case's, its tables feed the walk"""
    tabs = []
    for i, d in enumerate(c.draft):
        e = d["expected"]
        n = len(d["bscore"])
        lg = torch.full((n, d["logits"].shape[1] + 64), float("nan"))
        lg[:, : d["logits"].shape[1]] = _t(d["logits"])
        lg, ls, bs, nd = lg.cuda(), _t(d["lse"]).cuda(), _t(d["bscore"]).cuda(), _t(d["node"]).cuda()
        o_s = torch.full((MAXB,), 7.0, device="cuda")
        o_p, o_t, o_n, o_f = (torch.full((MAXB,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
        t = dict(score=torch.full((e["n_cand"] + 1,), 7.0, device="cuda"), off=torch.full((MAXB + 1,), -7, dtype=torch.int32, device="cuda"),
                 lse=torch.full((1,), 7.0, device="cuda"))
        _lib.check(lib.atspeed_beam_sample_step(lg.data_ptr(), lg.shape[1], ls.data_ptr(), bs.data_ptr(), nd.data_ptr(), n, am.fsm.ptr, am.mask_ptr,
                                                0, d["k"], c.w.T, d["sub"], None, int(d["filter_ids"]), o_s.data_ptr(), o_p.data_ptr(),
                                                o_t.data_ptr(), o_n.data_ptr(), o_f.data_ptr(), t["score"].data_ptr(), t["off"].data_ptr(),
                                                t["lse"].data_ptr(), None, _st()))
        torch.cuda.synchronize()
        assert o_f[: d["k"]].tolist() == e["flat"].tolist(), f"draft step {i}: the step kernel's block is not the case's"
        assert t["off"][: n + 1].tolist() == e["tab_off"].tolist()
        tabs.append(t)
    return tabs


def _check_walk(c, run, exp):
    w, o = c.w, run.out
    exact = c.family == "placed"
    k, dk, Wd = w.k, w.dk, w.W
    run.ar.check()
    # the trace: the steps the walk took, k picks each
    want = _before(o["vtrace"])
    if w.vtrace:
        for i, (sc, par, tok) in enumerate(exp["trace"]):
            got_bits = o["vtrace"].t[3 * i, :k].clone()
            live = tok >= 0
            lrow = w.blk_row0[i] + par[live]
            tb = np.full(k, np.inf)
            tb[live] = W.score_bound(w.logits[lrow, tok[live]], w.lse[lrow].astype(np.float64), 1.0, sc[live])
            _check_scores(f"trace score step {i}", got_bits.view(torch.float32), np.where(live, sc, -np.inf), tb, exact)
            want[3 * i, :k] = got_bits
            want[3 * i + 1, :k] = _t(par.astype(np.int32)).to(want.device)
            want[3 * i + 2, :k] = _t(tok.astype(np.int32)).to(want.device)
    guard.assert_same("vtrace", o["vtrace"].t, want)
    mail = _before(o["mail"])
    mail[0, 0] = exp["n_matches"]
    if exp["pending"]:
        guard.assert_same("mailbox", o["mail"].t, mail)
        for name, v in o.items():
            if name not in ("mail", "vtrace"):
                guard.assert_same(name + " (a pending walk writes n_matches only)", v.t, _before(v))
        return
    mail[0, 2] = exp["n_valid"]
    guard.assert_same("mailbox", o["mail"].t, mail)
    res = exp["res"]
    for f in ("node", "parent", "tok", "flat"):
        want = _before(o["res." + f])
        want[0, :k] = _t(res[f]).to(want.device)
        guard.assert_same("res." + f, o["res." + f].t, want)
    want = _before(o["res.seq"])
    want[:k, : res["seq_written"]] = _t(res["seq"][:, : res["seq_written"]]).to(want.device)
    guard.assert_same("res.seq", o["res.seq"].t, want)
    # scores: the pick's row of the last step's expand is row `parent` of block n_matches
    nm = exp["n_matches"]
    live = res["flat"] >= 0
    lrow = w.blk_row0[nm] + res["parent"][live]
    lg, ls = w.logits[lrow, res["tok"][live]], w.lse[lrow].astype(np.float64)
    bound = np.full(k, np.inf)
    bound[live] = W.score_bound(lg, ls, w.T, res["score"][live])
    _check_scores("res.score", o["res.score"].t[0, :k], res["score"], bound, exact)
    want = _before(o["res.score"])
    want[0, :k] = o["res.score"].t[0, :k]
    guard.assert_same("res.score beyond k", o["res.score"].t, want)
    for blk, e, r0 in (("next", exp["next"], 0), ("dnext", exp["dnext"], 0)):
        for f in ("ids", "pos", "slot", "vis"):
            v = o[f"{blk}.{f}"]
            want = _before(v)
            if e is not None:
                src = _t(e[f]).to(want.device)
                if f == "vis":
                    want[: len(src)] = src
                else:
                    want[0, : len(src)] = src
            guard.assert_same(f"{blk}.{f}" + ("" if e is not None else " (untouched unless every block was accepted)"), v.t, want)


def _walk_test(lib, c):
    exp = c.expected()
    am = Automaton(lib, c.w.fsm, c.mask_seqs) if c.w.fsm is not None else None
    try:
        dtab = _draft_tables(lib, c, am) if c.w.sample else []
        runs = []
        for _ in range(2):
            run = WalkRun(lib, c, am, dtab)
            _lib.check(run.rc)
            runs.append({f: v.buf.clone() for f, v in run.out.items()})
        _check_walk(c, run, exp)
        for f in runs[0]:
            assert torch.equal(runs[0][f], runs[1][f]), f"{f}: the second call answers other bits"
    finally:
        if am:
            am.close()


@pytest.mark.parametrize("name", list(SWALK))
def test_sampled_walk(lib, name):
    _walk_test(lib, SWALK[name])


@pytest.mark.parametrize("name", list(GWALK))
def test_greedy_walk(lib, name):
    _walk_test(lib, GWALK[name])


# ------------------------------------------------------------------ refusals, before any launch
WALK_REFUSALS = [("k", 0, "CAP"), ("k", 65, "CAP"), ("dk", 0, "CAP"), ("dk", 65, "CAP"), ("nb", 0, "CAP"), ("nb", 65, "CAP"), ("dl", -1, "CAP"),
                 ("dl", GAMMA + 1, "CAP"), ("ld", 0, "INV"), ("ld", -64, "INV"), ("logits", None, "INV"), ("lse", None, "INV"),
                 ("mailbox", None, "INV"), ("res_flat", None, "INV"), ("next_vis", None, "INV"), ("dnext_ids", None, "INV"),
                 ("cur_slot", None, "INV"), ("blk_score", (1, None), "INV"), ("blk_flat", (1, None), "INV"), ("struct_size", 8, "INV"),
                 ("vis_words", 0, "INV"), ("gen_len0", LMAX, "CAP"), ("blocks_ready", 9, "INV")]


@pytest.mark.parametrize("field,value,code", WALK_REFUSALS, ids=[f"{f}={v}" for f, v, _ in WALK_REFUSALS])
def test_walk_refusals(lib, field, value, code):
    c = GWALK["all_accepted"]
    am = Automaton(lib, c.w.fsm, None)
    try:
        run = WalkRun(lib, c, am, [], patch={field: value})
        assert run.rc == {"CAP": _lib.ERR_CAPACITY, "INV": _lib.ERR_INVALID}[code], (run.rc, lib.atspeed_last_error())
        run.untouched()
    finally:
        am.close()


def test_sampled_walk_refusals(lib):
    c = SWALK["reject_some"]
    am = Automaton(lib, c.w.fsm, None)
    try:
        dtab = _draft_tables(lib, c, am)
        for patch in ({"dtab_lse": (0, None)}, {"dtab_score": (1, None)}, {"temperature": 0.0}, {"fsm": None, "vocab": 100}):
            run = WalkRun(lib, c, am, dtab, patch=patch)
            assert run.rc == _lib.ERR_INVALID, (patch, run.rc)
            run.untouched()
    finally:
        am.close()


STEP_REFUSALS = [({"k": 0}, "CAP"), ({"k": 65}, "CAP"), ({"n": 0}, "CAP"), ({"n": 65}, "CAP"), ({"ld": 0}, "INV"), ({"lse": None}, "INV"),
                 ({"logits": None}, "INV"), ({"bs": None}, "INV"), ({"nd": None}, "INV"), ({"fsm": None}, "INV"), ({"T": 0.0}, "INV"),
                 ({"tl": None}, "INV"), ({"ts": None}, "INV")]


@pytest.mark.parametrize("patch,code", STEP_REFUSALS, ids=[str(p) for p, _ in STEP_REFUSALS])
def test_step_refusals(lib, patch, code):
    c = STEP["small"]
    am = Automaton(lib, c.fsm, None)
    try:
        ar, o, rc = _run_step(lib, c, am, args=patch)
        assert rc == {"CAP": _lib.ERR_CAPACITY, "INV": _lib.ERR_INVALID}[code], (rc, lib.atspeed_last_error())
        ar.check()
        for name, v in o.items():
            guard.assert_same(name + " (a refused call writes nothing)", v.t, _before(v))
    finally:
        am.close()
