"""Compatibility path for ARBITRARY `prefix_allowed_tokens_fn(batch_id, sentence) -> List[int]` callables.

The fast path compiles the mask into a device automaton (`generation_trie.ConstraintFSM`).  A callable that
cannot be compiled (any closure, e.g. the one `BaseDataset.get_prefix_allowed_tokens_fn` returns at
`code/data.py:96-104`) is served here the way the reference serves every mask: the function is called on the host
once per beam per step (`code/beamSD.py:60-64,286-291` through HF's `PrefixConstrainedLogitsProcessor`).  All
arithmetic still runs in libatspeed_hip — forwards (`HipLlama.forward_padded`), the full-vocabulary normaliser
(`atspeed_lse_rows`), mask + expand + top-K (`atspeed_beam_expand_prune` over a per-step automaton whose node r
holds row r's allowed list) and the acceptance test (`atspeed_accept`); only the mask lists and the small beam
tables cross PCIe, with one synchronisation per step like the reference.  One user at a time.

Extra logits processors (`BSSD(..., logits_processor=LogitsProcessorList([...]))`, beamSD.py:469-478) are torch callables
`(input_ids [n, len], scores [n, V]) -> scores`, so a step with processors hands them the log-softmax rows as a device tensor
(`_processed_rows`: `atspeed_log_softmax_rows`, then the mask first, as HF's PrefixConstrainedLogitsProcessor does it (scores + (-inf outside
the allowed list)), then the caller's processors in order (HF appends custom processors after its own)) and the library expands the rows they
return (`atspeed_beam_expand_prune_free`: row-wise top-k, then the K best (row, token) pairs; -inf entries are never picked).
The reference's post-top-k id filter (`_keep_ids`) runs whenever the processor list is non-empty (beamSD.py:80), mask or not.
Stage times (`draft/target/verify_time_cost`, the CSV columns inference.py:183-187 reads) are wall clock with a device
synchronisation at the end of each stage, as the reference's Timer measures them (beamSD.py:12-37).

Sampling mode (`generation_config.do_sample`, beamSD.py:65-75,293-321,332-369) with a host-side mask or processors: forwards and the
full-vocabulary log-softmax stay in the library; the tempered, masked rows of a step (<= DK x V fp32, 5 MB) come to the host, where
transformers' own TopKLogitsWarper / TopPLogitsWarper warp them when the config sets `top_k` / `top_p` (`_hf_warpers`) and the draws
are made from the SAME counter-based streams the device kernels use (`_HashRng`: (seed, purpose, round, step, model) -> sub-seed, one hash per
candidate id; scan.hip) -- so a callable that wraps a compilable constraint samples exactly what the device path samples for that seed
(tests/test_bssd_gpu.py).

There is ONE round loop (`_bssd`: draft stage, block packing, target forward, the verify row window, next-round inputs, statistics) and one
step body (`_one_step`).  Greedy and sampling differ in the step function (`_greedy_step` / `_sample_step`: how a step picks its beams) and in
the decision of one verify step (`_greedy_decide` / `_sample_decide`, on a `_VerifyStep`), which the entry points hand to the loop.
"""
from __future__ import annotations

import time
from functools import partial
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, synth
from .model import HipLlama, pack_vis_bits


class _Inputs:
    """Host-side description of one forward: tokens, positions, KV slots and visibility rows (bool [T, S])."""

    def __init__(self, ids, pos, slots, vis):
        self.ids = np.asarray(ids, np.int32)
        self.pos = np.asarray(pos, np.int32)
        self.slots = np.asarray(slots, np.int32)
        self.vis = np.asarray(vis, bool)


def _pad(v: np.ndarray, width: int) -> np.ndarray:
    if v.shape[1] >= width:
        return v[:, :width]
    return np.concatenate((v, np.zeros((v.shape[0], width - v.shape[1]), bool)), axis=1)


def _causal(ids: np.ndarray) -> _Inputs:
    n = len(ids)
    return _Inputs(ids, np.arange(n), np.arange(n), np.tril(np.ones((n, n), bool)))


def _pack(blocks: Sequence[_Inputs]) -> _Inputs:
    """several blocks as the inputs of ONE forward (visibility rows padded to the widest block)"""
    width = max(b.vis.shape[1] for b in blocks)
    return _Inputs(np.concatenate([b.ids for b in blocks]), np.concatenate([b.pos for b in blocks]),
                   np.concatenate([b.slots for b in blocks]), np.concatenate([_pad(b.vis, width) for b in blocks], axis=0))


def _forward(model: HipLlama, inp: _Inputs, n_rows: int):
    """-> (logits [n_rows, ld] device, lse [n_rows] device)."""
    dev = model.device
    with torch.cuda.device(dev):
        ids, pos, slots = (torch.from_numpy(a).to(dev) for a in (inp.ids, inp.pos, inp.slots))
        bits = torch.from_numpy(pack_vis_bits(inp.vis, model.max_slots)).to(dev)
        logits = model.forward_padded(ids, pos, slots, bits, inp.vis.shape[1], n_rows)
        lse = torch.empty(n_rows, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().atspeed_lse_rows(logits.data_ptr(), n_rows, model.dims.vocab_size, model.logits_ld, lse.data_ptr(),
                                                _lib.stream_ptr(dev)))
    return logits, lse


def _allowed_lists(fn: Callable, seqs: np.ndarray) -> List[List[int]]:
    out = []
    for r in range(seqs.shape[0]):
        al = fn(0, torch.from_numpy(seqs[r]))        # batch id 0: _num_beams is poked to the row count (beamSD.py:56,281)
        if len(al) == 0:                              # TypeError when fn returned None, like the HF processor
            raise ValueError("`prefix_allowed_tokens_fn` returned an empty list for batch ID 0."
                             "This means that the constraint is unsatisfiable. Please check your implementation"
                             "of `prefix_allowed_tokens_fn` ")
        out.append(sorted({int(t) for t in al}))
    return out


def _gather_rows(model: HipLlama, logits, lse, row_ids: Sequence[int]):
    """the candidate rows of a forward (verify keeps only hit beams), contiguous"""
    rows = torch.as_tensor(list(row_ids), dtype=torch.int64, device=model.device)
    return logits[rows].contiguous(), lse[rows].contiguous()


def _read_back(o_s, o_p, o_t, o_f):
    """device top-k result -> host arrays (score, parent (row index r), token, flat = r*V + token), only real beams (finite scores)"""
    s, p, t, f = (x.cpu().numpy() for x in (o_s, o_p, o_t, o_f))
    keep = f >= 0
    return s[keep], p[keep].astype(np.int64), t[keep].astype(np.int64), f[keep].astype(np.int64)


def _expand_prune(model: HipLlama, logits, lse, row_ids: Sequence[int], beam_scores: np.ndarray,
                  allowed: List[List[int]], k: int):
    """Mask + add beam scores + top-k on the device (beamSD.py:60-78).  `row_ids[r]` = logits row of candidate row r."""
    lib = _lib.load()
    dev = model.device
    n = len(allowed)
    row_ptr = np.zeros(n + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(a) for a in allowed])
    tok = np.asarray([t for a in allowed for t in a], np.int32)
    nxt = np.zeros(len(tok), np.int32)
    with _lib.Handle.create("atspeed_fsm_destroy", lib.atspeed_fsm_create, row_ptr.ctypes.data, tok.ctypes.data, nxt.ctypes.data, n, len(tok),
                            model.dims.vocab_size) as fsm, torch.cuda.device(dev):
        lg, ls = _gather_rows(model, logits, lse, row_ids)
        bs = torch.from_numpy(np.asarray(beam_scores, np.float32)).to(dev)
        nd = torch.arange(n, dtype=torch.int32, device=dev)
        o_s = torch.empty(k, dtype=torch.float32, device=dev)
        o_p, o_t, o_n, o_f = (torch.empty(k, dtype=torch.int32, device=dev) for _ in range(4))
        _lib.check(lib.atspeed_beam_expand_prune(lg.data_ptr(), model.logits_ld, ls.data_ptr(), bs.data_ptr(), nd.data_ptr(), n, fsm.ptr, k,
                                                 o_s.data_ptr(), o_p.data_ptr(), o_t.data_ptr(), o_n.data_ptr(), o_f.data_ptr(),
                                                 _lib.stream_ptr(dev)))
        return _read_back(o_s, o_p, o_t, o_f)


def _processed_rows(model: HipLlama, logits, lse, row_ids: Sequence[int], seqs: np.ndarray, fn: Optional[Callable],
                    procs: Sequence[Callable]) -> torch.Tensor:
    """log-softmax over the full vocabulary (:58,:285; library) -> prefix mask (:60-64,:286-291; transformers
    PrefixConstrainedLogitsProcessor.__call__: scores + mask) -> processors: device fp32 [n, V].  Call under the model's device."""
    dev = model.device
    V, n = model.dims.vocab_size, len(row_ids)
    lg, ls = _gather_rows(model, logits, lse, row_ids)
    scores = torch.empty(n, V, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().atspeed_log_softmax_rows(lg.data_ptr(), model.logits_ld, ls.data_ptr(), n, V, scores.data_ptr(), V,
                                                    _lib.stream_ptr(dev)))
    if fn is not None:
        mask = torch.full_like(scores, float("-inf"))
        for r, al in enumerate(_allowed_lists(fn, seqs)):
            mask[r, torch.as_tensor(al, dtype=torch.long, device=dev)] = 0
        scores = scores + mask
    if procs:
        ids = torch.from_numpy(np.ascontiguousarray(seqs)).to(dev)
        for proc in procs:
            scores = proc(ids, scores)
    return scores.to(torch.float32)


def _expand_processed(model: HipLlama, logits, lse, row_ids: Sequence[int], beam_scores: np.ndarray, seqs: np.ndarray,
                      fn: Optional[Callable], procs: Sequence[Callable], k: int):
    """The expand of a step WITH extra logits processors (beamSD.py:58-78): processed rows -> + beam scores -> top-k."""
    dev = model.device
    V, n = model.dims.vocab_size, len(row_ids)
    with torch.cuda.device(dev):
        scores = _processed_rows(model, logits, lse, row_ids, seqs, fn, procs).contiguous()
        bs = torch.from_numpy(np.asarray(beam_scores, np.float32)).to(dev)
        zero = torch.zeros(n, dtype=torch.float32, device=dev)
        ws = torch.empty(n * _lib.MAX_BEAMS, dtype=torch.int32, device=dev)
        o_s = torch.empty(k, dtype=torch.float32, device=dev)
        o_p, o_t, o_f = (torch.empty(k, dtype=torch.int32, device=dev) for _ in range(3))
        _lib.check(_lib.load().atspeed_beam_expand_prune_free(scores.data_ptr(), V, zero.data_ptr(), bs.data_ptr(), n, V, k, ws.data_ptr(),
                                                              o_s.data_ptr(), o_p.data_ptr(), o_t.data_ptr(), o_f.data_ptr(),
                                                              _lib.stream_ptr(dev)))
        return _read_back(o_s, o_p, o_t, o_f)


def _expand(model, logits, lse, row_ids, beam_scores, seqs, fn, procs, k):
    if procs:
        return _expand_processed(model, logits, lse, row_ids, beam_scores, seqs, fn, procs, k)
    return _expand_prune(model, logits, lse, row_ids, beam_scores, _allowed_lists(fn, seqs), k)


def _hf_warpers(top_k: int, top_p: float, min_keep: int) -> List[Callable]:
    """what `_get_logits_warper` puts after the temperature for a beam search: transformers' own top-k, then top-p (0 / >= 1 = off)"""
    out: List[Callable] = []
    if top_k or top_p < 1.0:
        from transformers import TopKLogitsWarper, TopPLogitsWarper
        if top_k:
            out.append(TopKLogitsWarper(top_k=int(top_k), min_tokens_to_keep=int(min_keep)))
        if top_p < 1.0:
            out.append(TopPLogitsWarper(top_p=float(top_p), min_tokens_to_keep=int(min_keep)))
    return out


def _tempered_rows(model: HipLlama, logits, lse, row_ids: Sequence[int], seqs: np.ndarray, fn: Optional[Callable], procs: Sequence[Callable],
                   temperature: float, warpers: Sequence[Callable] = ()) -> np.ndarray:
    """processed rows -> temperature warper (:65-66, :293-294) -> top-k / top-p warpers on the host rows -> host fp32 [n, V]"""
    with torch.cuda.device(model.device):
        rows = (_processed_rows(model, logits, lse, row_ids, seqs, fn, procs) / float(temperature)).cpu()
    for w in warpers:
        rows = w(None, rows)
    return rows.numpy()


def _keep_ids(t: np.ndarray, s: Optional[np.ndarray] = None) -> np.ndarray:
    """The id filter after the top-k (beamSD.py:80-86; the Llama vocabulary size and EOS are hard-coded there, and any processor switches
    it on): item codes and EOS stay.  With `s`, the scores of the picks (sampling), a pick must be finite too."""
    keep = (t >= synth.LLAMA_VOCAB) | (t == synth.EOS_ID)
    return keep if s is None else keep & np.isfinite(s)


# ---------------------------------------------------------------------------------------------- random streams of the sampling mode
P_STEP, P_ACCEPT, P_PERM, P_RESID, P_BONUS = 1, 2, 3, 4, 5     # purposes of a random stream (scan.hip)


class _HashRng:
    """The device's counter-based generator (scan.hip / common.h ats_rng_sub): every draw is a pure function of
    (seed, purpose, round, step, model tag, element id).  A draw without replacement = top-n of log w + Gumbel(hash(id)) (Plackett-Luce, the
    law of torch.multinomial's sequential draws), a uniform = ((h >> 9) + 0.5) 2^-23, a random subset = the n smallest hashes."""

    def __init__(self, seed: int):
        self.seed, self.sub = int(seed) & 0xFFFFFFFF, 0

    def begin(self, purpose: int, rnd: int, step: int, model_tag: int = 0):
        ctr = (purpose & 0xFF) | ((rnd & 0xFF) << 8) | ((step & 0xFF) << 16) | ((model_tag & 0xFF) << 24)
        self.sub = int(synth.hash_u32(np.array([ctr], dtype=np.uint64), self.seed)[0])

    def _u01(self, ids: np.ndarray) -> np.ndarray:
        h = synth.hash_u32(ids.astype(np.uint64), self.sub)
        return ((h >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)

    def multinomial_log(self, logw: np.ndarray, n: int) -> np.ndarray:
        ids = np.nonzero(np.isfinite(logw))[0]
        u = self._u01(ids)
        keys = logw[ids].astype(np.float32) + (-np.log(-np.log(u, dtype=np.float32), dtype=np.float32)).astype(np.float32)
        order = np.lexsort((ids, -keys))                 # key desc, id asc
        return ids[order[:n]].astype(np.int64)

    def uniform_ids(self, ids: np.ndarray) -> np.ndarray:
        return self._u01(ids)

    def subset_ids(self, ids: np.ndarray, n: int) -> np.ndarray:
        h = synth.hash_u32(ids.astype(np.uint64), self.sub)
        return np.lexsort((np.arange(len(ids)), h))[:n].astype(np.int64)


def _softmax(x: np.ndarray) -> np.ndarray:
    """softmax over a flat fp32 vector with -inf entries (all -inf -> zeros, as the reference zeroes its NaNs, beamSD.py:319-320)"""
    m = np.max(x) if x.size else -np.inf
    if not np.isfinite(m):
        return np.zeros_like(x, dtype=np.float32)
    e = np.exp((x - m).astype(np.float32), dtype=np.float32)
    return (e / e.sum(dtype=np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- one step
def _one_step(model: HipLlama, inp: _Inputs, k: int, beam_scores: np.ndarray, beam_seq: np.ndarray, pick: Callable) -> Dict:
    """one_step_beam_search (beamSD.py:40-106): forward, `pick(logits, lse, n, seqs)` -> dict(flat, scores, parents, tokens, ...) of the
    new beams, then their sequences and the inputs of the next forward."""
    n = len(beam_scores)
    logits, lse = _forward(model, inp, n)
    o = pick(logits, lse, n, beam_seq[:1] if (n == 1 and k != 1) else beam_seq)    # :61-64
    p, t = o["parents"], o["tokens"]
    m = len(t)
    S = inp.vis.shape[1]
    vis = np.concatenate((inp.vis[-n:][p], np.eye(m, dtype=bool)), axis=1)          # :89
    o["next"] = _Inputs(t, np.full(m, inp.pos[-1] + 1), np.arange(S, S + m), vis)   # :91
    o["seq"] = np.concatenate((beam_seq[p], t[:, None]), axis=1)
    return o


def _greedy_step(model, inp, k, beam_scores, beam_seq, stream, fn, procs) -> Dict:
    """a step that keeps the k best candidates (`stream`, the random stream of the step, is the sampling form's)"""
    def pick(logits, lse, n, seqs):
        s, p, t, f = _expand(model, logits, lse, range(n), beam_scores, seqs, fn, procs, k)
        keep = _keep_ids(t)
        return dict(flat=f[keep], scores=s[keep], parents=p[keep], tokens=t[keep])
    return _one_step(model, inp, k, beam_scores, beam_seq, pick)


def _sample_step(model, inp, k, beam_scores, beam_seq, stream, fn, procs, temperature, rng, warpers=()) -> Dict:
    """a step with do_sample (:65-75): k draws without replacement from softmax of the flattened scores; stream = (round, step, model tag)"""
    V = model.dims.vocab_size

    def pick(logits, lse, n, seqs):
        flat = (_tempered_rows(model, logits, lse, range(n), seqs, fn, procs, temperature, warpers)
                + np.asarray(beam_scores, np.float32)[:, None]).reshape(-1)
        rng.begin(P_STEP, *stream)
        idx = rng.multinomial_log(flat, k)
        s = flat[idx]
        if fn is not None or procs:
            keep = _keep_ids(idx % V, s)
            idx, s = idx[keep], s[keep]
        return dict(flat=idx, scores=s.astype(np.float32), parents=idx // V, tokens=idx % V, probs=_softmax(flat), dist=flat)
    return _one_step(model, inp, k, beam_scores, beam_seq, pick)


def _beam_search(model: HipLlama, prompt: np.ndarray, max_new_tokens: int, step: Callable):
    k = int(model.generation_config.num_beams)
    inp = _causal(prompt)
    scores = np.zeros(1, np.float32)
    seq = np.repeat(prompt[None, :], k, axis=0)
    for g in range(max_new_tokens):                                                 # beamSD.py:579-588
        o = step(model, inp, k, scores, seq, (g, 0, 0))
        inp, scores, seq = o["next"], o["scores"], o["seq"]
    return seq, scores


def _final_sort(seq: np.ndarray, scores: np.ndarray):
    o = np.argsort(-scores, kind="stable")                                          # beamSD.py:529-531, :589-591
    return seq[o], scores[o]


def _sampling_kw(fn, procs, sample, num_beams: int) -> Dict:
    """`sample` = (temperature, seed) or (temperature, seed, top_k, top_p); the warpers' min_tokens_to_keep follows the TARGET's beam count, as
    the reference builds one warper list from the target's config for both models (beamSD.py:479-481)"""
    temperature, seed = sample[:2]
    top_k, top_p = sample[2:] if len(sample) > 2 else (0, 1.0)
    return dict(fn=fn, procs=procs, temperature=temperature, rng=_HashRng(seed), warpers=_hf_warpers(top_k, top_p, 2 if num_beams > 1 else 1))


def target_generate_host_mask(model: HipLlama, prompt: np.ndarray, max_new_tokens: int, fn: Optional[Callable],
                              procs: Sequence[Callable] = (), sample=None) -> Dict:
    """target_generate (beamSD.py:544-595) with the mask function / logits processors on the host; `sample` = (temperature, seed) with
    `generation_config.do_sample`, optionally followed by (top_k, top_p)."""
    if sample is None:
        seq, scores = _beam_search(model, prompt, max_new_tokens, partial(_greedy_step, fn=fn, procs=procs))
    else:
        seq, scores = _final_sort(*_beam_search(model, prompt, max_new_tokens, partial(_sample_step, **_sampling_kw(fn, procs, sample, int(model.generation_config.num_beams)))))
    return dict(beam_sequence=seq, beam_scores=scores)


# ---------------------------------------------------------------------------------------------- the decision of one verify step
class _VerifyStep:
    """One step of the verify walk, as the loop hands it to a decision function `decide(target, logits, lse, k, step, ...)`, which returns
    (scores, parents, tokens, hit') of the step's new beams: hit' = their indices among the draft's next block when that block is accepted,
    None when the walk ends here."""

    def __init__(self, stream, last, rows, seqs, scores, hit, n_draft, drafted):
        self.stream = stream        # (round, step) of the random streams (sampling)
        self.last = last            # the step after the draft's last block: nothing left to judge, its beams are the round's result
        self.rows = rows            # logits rows of the beams that survived so far
        self.seqs = seqs            # their sequences
        self.scores = scores        # and scores
        self.hit = hit              # their indices among the step's `n_draft` draft beams (None at step 0)
        self.n_draft = n_draft
        self.drafted = drafted      # the draft's step whose block is judged (None at the last step)


def _greedy_decide(target, logits, lse, k, step: _VerifyStep, fn, procs):
    """verify, greedy (beamSD.py:242-456): the target's top-k of the step; accepted when the draft's block holds all of them"""
    lib = _lib.load()
    s, p, t, _ = _expand(target, logits, lse, step.rows, step.scores, step.seqs, fn, procs, k)
    parents = step.hit[p] if step.hit is not None else p
    if step.last:
        return s, parents, t, None
    flat = parents * target.dims.vocab_size + t
    d_flat = step.drafted["flat"]
    kk, dd = len(flat), len(d_flat)
    with torch.cuda.device(target.device):                                          # acceptance on the device (:371-380)
        tf = torch.from_numpy(flat.astype(np.int32)).cuda()
        ts = torch.from_numpy(np.asarray(s, np.float32)).cuda()
        df = torch.from_numpy(d_flat.astype(np.int32)).cuda()
        h_out = torch.empty(kk, dtype=torch.int32, device="cuda")
        sb = torch.empty(kk, dtype=torch.float32, device="cuda")
        acc = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.atspeed_accept(tf.data_ptr(), ts.data_ptr(), kk, df.data_ptr(), dd, h_out.data_ptr(), sb.data_ptr(),
                                      acc.data_ptr(), _lib.stream_ptr(target.device)))
        if not (bool(acc.item()) and kk == k):
            return s, parents, t, None
        hit = h_out.cpu().numpy().astype(np.int64)
    pos_of = {int(d): j for j, d in enumerate(d_flat)}
    order = np.argsort(np.asarray([pos_of[int(y)] for y in flat]), kind="stable")    # the next step's rows come in the draft's order
    return s[order], parents, t, hit


def _sample_decide(target, logits, lse, k, step: _VerifyStep, fn, procs, temperature, rng, warpers=()):
    """verify with do_sample (beamSD.py:293-321 distributions, :332-369 accept / resample, :303-309 bonus draw).  One documented deviation,
    as on the device path: with no residual mass left the remaining draws come from the target distribution (the reference resamples
    uniformly over the whole vocabulary, -inf scores included)."""
    V = target.dims.vocab_size
    stream, drafted = step.stream, step.drafted
    bs = _tempered_rows(target, logits, lse, step.rows, step.seqs, fn, procs, temperature, warpers) + np.asarray(step.scores, np.float32)[:, None]
    if step.hit is not None:                                                        # :311-321: into the draft's beam space
        tbs = np.full((step.n_draft, V), -np.inf, dtype=np.float32)
        tbs[step.hit] = bs
        bs = tbs
    bs = bs.reshape(-1)

    def beams(flat_ids, hit_next):
        return bs[flat_ids], flat_ids // V, flat_ids % V, hit_next
    if step.last:                                                                   # :303-309 bonus draw from the target
        rng.begin(P_BONUS, *stream, 0)
        return beams(rng.multinomial_log(bs, k), None)
    probs = _softmax(bs)
    dprobs, d_ids = drafted["probs"], drafted["flat"]
    p_i, q_i = probs[d_ids], dprobs[d_ids]
    rng.begin(P_ACCEPT, *stream, 0)
    r = rng.uniform_ids(np.arange(len(d_ids)))
    acc = (r * q_i) <= p_i                                                          # r <= p / q without the division, as the device tests it
    acc_tokens = d_ids[acc]
    n_acc = int(acc.sum())
    if n_acc >= k:                                                                  # :341-350
        rng.begin(P_PERM, *stream, 0)
        sel = rng.subset_ids(np.nonzero(acc)[0], k)
        seq_tokens = np.sort(acc_tokens[sel])
        pos_of = {int(d): j for j, d in enumerate(d_ids.tolist())}
        return beams(seq_tokens, np.asarray([pos_of[int(y)] for y in seq_tokens.tolist()], dtype=np.int64))
    newp = np.clip(probs - dprobs, 0, None).astype(np.float32)                      # :351-369 reject: resample the missing beams
    newp[acc_tokens] = 0
    if float(newp.sum()) == 0.0:
        newp = probs.copy()
        newp[acc_tokens] = 0
    rng.begin(P_RESID, *stream, 0)
    with np.errstate(divide="ignore"):
        nxt = rng.multinomial_log(np.log(newp, dtype=np.float32), k - n_acc)
    return beams(np.sort(np.concatenate((acc_tokens, nxt))), None)


# ---------------------------------------------------------------------------------------------- the round loop
class _Stage:
    """wall clock of a stage with a device synchronisation at its end (the reference's Timer, beamSD.py:12-37)"""

    def __init__(self, acc: Dict[str, float], key: str, dev):
        self.acc, self.key, self.dev = acc, key, dev

    def __enter__(self):
        self.t0 = time.time()

    def __exit__(self, *exc):
        torch.cuda.synchronize(self.dev)
        self.acc[self.key] += time.time() - self.t0


def _bssd(target: HipLlama, draft: HipLlama, prompt: np.ndarray, gamma: int, max_new_tokens: int, step: Callable, decide: Callable) -> Dict:
    """The rounds of BSSD (beamSD.py:458-542) around a step function and a verify decision."""
    cost = {"draft_time_cost": 0.0, "target_time_cost": 0.0, "verify_time_cost": 0.0}
    k, dk = int(target.generation_config.num_beams), int(draft.generation_config.num_beams)
    cur_len, max_len = len(prompt), len(prompt) + max_new_tokens
    tin = din = _causal(prompt)
    scores = np.zeros(1, np.float32)
    seq = np.repeat(prompt[None, :], k, axis=0)
    accept_steps: List[int] = []
    while cur_len < max_len:
        rnd = len(accept_steps)
        dl = min(gamma, max_len - cur_len - 1)                                      # :504
        if dl == 0:                                                                 # :505-509 (in no stage's sum: the reference breaks before :523-525)
            o = step(target, tin, k, scores, seq, (rnd, 0, 0))
            seq, scores = o["seq"], o["scores"]
            break
        # ---- draft (:108-179)
        steps, inp, d_scores, d_seq = [], din, scores, seq
        step_len, step_seq = [len(scores)], [seq]
        with _Stage(cost, "draft_time_cost", draft.device):
            for i in range(dl):
                o = step(draft, inp, dk, d_scores, d_seq, (rnd, i, 1))
                inp, d_scores, d_seq = o["next"], o["scores"], o["seq"]
                steps.append(o)
                step_len.append(len(d_scores))
                step_seq.append(d_seq)
        # ---- target: one forward over round inputs ++ every draft block (:190-232)
        packed = _pack([tin] + [o["next"] for o in steps])
        with _Stage(cost, "target_time_cost", target.device):
            logits, lse = _forward(target, packed, sum(step_len))
        t_verify = time.time()
        # ---- verify (:242-456): step i judges draft block i + 1 on the rows of block i, until a block is refused or none is left
        lo, hi = 0, step_len[0]
        hit, v_scores = None, scores
        for i in range(dl + 1):
            rows = list(range(lo, hi))
            if i != dl:
                lo, hi = hi, hi + step_len[i + 1]
            seqs = step_seq[i]
            if hit is not None:
                rows, seqs = [rows[h] for h in hit], seqs[hit]
            if i == 0 and len(rows) == 1 and k != 1:
                seqs = seqs[:1]
            v_scores, parents, t, hit = decide(target, logits, lse, k, _VerifyStep((rnd, i), i == dl, rows, seqs, v_scores, hit, step_len[i],
                                                                                   steps[i] if i != dl else None))
            if hit is None:
                break
        nm = i                                                                      # accepted blocks = steps that went on
        seq = np.concatenate((step_seq[nm][parents], t[:, None]), axis=1)           # :383
        scores = np.asarray(v_scores, np.float32)
        # ---- next round's inputs: the new beams over the accepted block's rows
        blk_lo = len(tin.ids) - step_len[0] + sum(step_len[:nm])
        blk_rows = packed.vis[blk_lo: blk_lo + step_len[nm]]
        base = int(packed.slots[blk_lo + step_len[nm] - 1]) + 1
        m = len(t)
        vis = np.concatenate((_pad(blk_rows, base)[parents], np.eye(m, dtype=bool)), axis=1)
        tin = din = _Inputs(t, np.full(m, packed.pos[blk_lo] + 1), np.arange(base, base + m), vis)
        if nm == dl:                                                                # :402-416: the draft re-ingests its last block
            last = steps[dl - 1]["next"]
            din = _Inputs(np.concatenate((last.ids, tin.ids)), np.concatenate((last.pos, tin.pos)),
                          np.concatenate((last.slots, tin.slots)), np.concatenate((_pad(last.vis, base + m), vis), axis=0))
        cur_len += nm + 1
        accept_steps.append(nm)
        torch.cuda.synchronize(target.device)
        cost["verify_time_cost"] += time.time() - t_verify
    n_run, total = len(accept_steps), sum(accept_steps)
    return dict(beam_sequence=seq, beam_scores=scores, n_run=n_run, total_accept_steps=total, total_accept_tokens=total * k,
                ave_accept_tokens=total * k / n_run if n_run else 0.0, accept_steps=accept_steps, **cost)


def bssd_host_mask(target: HipLlama, draft: HipLlama, prompt: np.ndarray, gamma: int, max_new_tokens: int, fn: Optional[Callable],
                   procs: Sequence[Callable] = (), sample=None) -> Dict:
    """BSSD (beamSD.py:458-542) with the mask function / logits processors on the host; `sample` = (temperature, seed) with
    `generation_config.do_sample`."""
    if sample is None:
        kw = dict(fn=fn, procs=procs)
        return _bssd(target, draft, prompt, gamma, max_new_tokens, partial(_greedy_step, **kw), partial(_greedy_decide, **kw))
    kw = _sampling_kw(fn, procs, sample, int(target.generation_config.num_beams))
    out = _bssd(target, draft, prompt, gamma, max_new_tokens, partial(_sample_step, **kw), partial(_sample_decide, **kw))
    out["beam_sequence"], out["beam_scores"] = _final_sort(out["beam_sequence"], out["beam_scores"])
    return out
