"""Restatement of the sampling-mode warpers as ONE cutoff per score row (the rule the device kernel `row_warp_cutoff` and the host path share;
include/atspeed_hip.h, atspeed_warp_cutoffs), in numpy fp32, plus the boundary margins the GPU comparisons require of their inputs.

A row holds tempered log-softmax scores; -inf (masked) and NaN entries are no candidates.
  top-k : k' = max(top_k, min_keep).  With at least k' finite entries, everything strictly below the k'-th largest is cut and ties with it
          survive (transformers: `scores < topk(scores, k')[0][..., -1, None]`); with fewer, the k'-th largest of the full row is -inf and
          nothing is cut.  top_k in (None, 0) = off.
  top-p : on what top-k left, p = softmax(row).  In descending order an entry is kept while the mass strictly above it is below top_p; the
          first min_keep are always kept (transformers removes, ascending, the entries whose cumulative sum is <= 1 - top_p and never the
          last min_keep: the same boundary from the other end).  top_p in (None, >= 1) = off.
The cutoff is the score of the last kept entry; a candidate survives iff its score is at or above it (-inf = nothing cut).
"""
from __future__ import annotations

import numpy as np


def _finite_desc(row: np.ndarray) -> np.ndarray:
    row = np.asarray(row, np.float32)
    return np.sort(row[np.isfinite(row)])[::-1]


def _norm(top_k, top_p):
    return (0 if top_k is None else int(top_k)), (1.0 if top_p is None else min(float(top_p), 1.0))


def _descending_mass(sv: np.ndarray):
    """softmax of a descending run and the fp32 mass strictly above each entry (sequential sum, largest first)"""
    e = np.exp((sv - sv[0]).astype(np.float32), dtype=np.float32)
    p = (e / e.sum(dtype=np.float32)).astype(np.float32)
    before = np.concatenate((np.zeros(1, np.float32), np.cumsum(p, dtype=np.float32)[:-1]))
    return p, before


def cutoff(row: np.ndarray, top_k, top_p, min_keep: int) -> float:
    top_k, top_p = _norm(top_k, top_p)
    s = _finite_desc(row)
    cut = -np.inf
    if len(s) == 0 or (top_k == 0 and top_p >= 1.0):
        return cut
    n_surv = len(s)
    if top_k:
        kk = max(top_k, min_keep)
        if kk <= len(s):
            cut = float(s[kk - 1])
            n_surv = int((s >= s[kk - 1]).sum())
    if top_p < 1.0:
        sv = s[:n_surv]
        _, before = _descending_mass(sv)
        keep = (before < np.float32(top_p)) | (np.arange(n_surv) < min_keep)
        n_keep = n_surv if keep.all() else int(np.argmin(keep))
        cut = float(sv[max(n_keep, 1) - 1])
    return cut


def survivors(row: np.ndarray, top_k, top_p, min_keep: int) -> np.ndarray:
    """bool mask of the entries that stay finite"""
    row = np.asarray(row, np.float32)
    return np.isfinite(row) & (row >= np.float32(cutoff(row, top_k, top_p, min_keep)))


def margins(row: np.ndarray, top_k, top_p, min_keep: int, tie_at_k: bool = False):
    """(gap_k, gap_p) of a row: the distance between the scores on either side of the top-k threshold (with `tie_at_k` the row holds a
    deliberate exact tie at the k'-th value: the gap below the tied group), and the smallest |cumulative probability - (1 - top_p)| of
    transformers' ascending cumulative sum over what top-k left.  inf where a warper is off or has nothing to cut."""
    top_k, top_p = _norm(top_k, top_p)
    s = _finite_desc(row)
    gap_k = gap_p = np.inf
    n_surv = len(s)
    if len(s) and top_k:
        kk = max(top_k, min_keep)
        if kk <= len(s):
            n_surv = int((s >= s[kk - 1]).sum())
            if tie_at_k:
                assert n_surv > kk, "the row has no tie at the k-th value"
                gap_k = float(s[kk - 1] - s[n_surv]) if n_surv < len(s) else np.inf
            elif kk < len(s):
                gap_k = float(s[kk - 1] - s[kk])
    if len(s) and top_p < 1.0:
        sv = s[:n_surv][::-1].astype(np.float32)                       # ascending, as TopPLogitsWarper sorts
        e = np.exp(sv - sv[-1], dtype=np.float32)
        cum = np.cumsum((e / e.sum(dtype=np.float32)).astype(np.float32), dtype=np.float32)
        gap_p = float(np.abs(cum.astype(np.float64) - (1.0 - top_p)).min())
    return gap_k, gap_p


def hf_survivors(row: np.ndarray, top_k, top_p, min_keep: int) -> np.ndarray:
    """the installed transformers' TopKLogitsWarper -> TopPLogitsWarper on the row, in the reference's order; bool mask of finite entries"""
    import torch
    from transformers import TopKLogitsWarper, TopPLogitsWarper
    top_k, top_p = _norm(top_k, top_p)
    x = torch.from_numpy(np.asarray(row, np.float32))[None].clone()
    if top_k:
        x = TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=min_keep)(None, x)
    if top_p < 1.0:
        x = TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=min_keep)(None, x)
    return torch.isfinite(x[0]).numpy()


def score_row(n: int, seed: int, scale: float = 2.0, temperature: float = 1.0, n_masked: int = 0, tie_at: int = 0) -> np.ndarray:
    """a row of tempered log-softmax scores: n entries, `n_masked` of them -inf, optionally an exact tie between the tie_at-th and
    (tie_at + 1)-th largest finite entries"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    m = x.max()
    x = ((x - m) - np.log(np.exp(x - m, dtype=np.float32).sum(dtype=np.float32))).astype(np.float32) / np.float32(temperature)
    if n_masked:
        x[rng.choice(n, size=n_masked, replace=False)] = -np.inf
    if tie_at:
        fin = np.nonzero(np.isfinite(x))[0]
        order = fin[np.argsort(-x[fin], kind="stable")]
        x[order[tie_at]] = x[order[tie_at - 1]]
    return x.astype(np.float32)
