#!/usr/bin/env python3
"""What scoring candidates costs (DESIGN "Scoring candidates"): `score_items_batch` against the path it replaces for this use,
`teacher.score_branches_batch` plus a host-side log-softmax and gather that produce the same numbers.  Llama-7B dims (bf16, 32 layers), the
Beauty-shaped strict trie, 32 users x 100 candidates of 4 codes; packed rows per user before and after prefix sharing.  Two candidate sets:
`random` (100 of the 12 035 items: they share little more than first codes) and `clustered` (100 items under 10 first codes, what a
retriever that works on the code tree returns).

    python tools/score_items_cost.py [users] [candidates] [parent commit] > profiles/score_items_cost.txt
"""
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from atspeed_amd import synth
from atspeed_amd.beamSD import _tree_rows_added, score_items_batch
from atspeed_amd.generation_trie import SuffixTrieConstraint, Trie
from atspeed_amd.model import HipLlama
from atspeed_amd.teacher import score_branches_batch

n_users = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n_cand = int(sys.argv[2]) if len(sys.argv) > 2 else 100
REPS = 3
dev = torch.device("cuda", 0)
vocab = synth.BEAUTY
m = HipLlama.from_synthetic(synth.llama_7b(vocab.vocab_size, 32), 2025, dtype=torch.bfloat16, num_beams=20, max_slots=512, max_tokens=512,
                            max_logit_rows=512, device=dev)
items = sorted({tuple(int(t) for t in it) for it in synth.synthetic_items(vocab)})
fn = SuffixTrieConstraint(Trie([[1] + list(it) + [2] for it in items]), synth.RESPONSE_SEP, 1)
plens = synth.prompt_lengths(n_users, 7)
prompts = [synth.synthetic_prompt(int(plens[u]), 900 + u) for u in range(n_users)]
inputs = [{"input_ids": torch.from_numpy(p.astype(np.int64))[None].to(dev)} for p in prompts]
rng = np.random.default_rng(1)
by_first = {}
for it in items:
    by_first.setdefault(it[0], []).append(it)


def candidates(kind):
    out = []
    for _ in range(n_users):
        if kind == "random":
            pick = [items[i] for i in rng.choice(len(items), size=n_cand, replace=False)]
        else:
            firsts = rng.choice(sorted(by_first), size=10, replace=False)
            pool = [it for f in firsts for it in by_first[int(f)]]
            pick = [pool[i] for i in rng.choice(len(pool), size=min(n_cand, len(pool)), replace=False)]
        out.append([list(q) for q in pick])
    return out


def timed(f):
    f()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


def teacher_path(lists):
    """the same numbers from full-vocabulary logits: one packed forward with a row per branch token, then log-softmax, gather and sum"""
    logits = score_branches_batch(m, prompts, lists)
    out = []
    for brs, lg in zip(lists, logits):
        lp = torch.log_softmax(torch.stack(lg), -1)                                    # [candidates, 4, V]
        idx = torch.tensor(brs, device=dev)
        out.append(lp.gather(-1, idx[..., None])[..., 0].sum(-1))
    return out


commit = sys.argv[3] if len(sys.argv) > 3 else subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                                              cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
print(f"score_items cost on the tree of the commit that follows {commit or '(unknown: not a git checkout, no commit given)'}; {torch.cuda.get_device_name(dev)}")
print(f"Llama-7B dims (32 layers, bf16), Beauty-shaped strict trie ({len(items)} items), {n_users} users x {n_cand} candidates of 4 codes, "
      f"prompts of {int(plens.min())}-{int(plens.max())} tokens; {REPS} timed calls after one warm-up, wall clock with a device synchronisation")
for kind in ("random", "clustered"):
    lists = candidates(kind)
    before = [len(p) + sum(len(q) - 1 for q in l) for p, l in zip(prompts, lists)]
    after = []
    for p, l in zip(prompts, lists):
        rows, prev = len(p), None
        for q in sorted({tuple(q) for q in l}):
            rows += _tree_rows_added(prev, q)
            prev = q
        after.append(rows)
    new, t_new = timed(lambda: score_items_batch(m, inputs, lists, fn))
    old, t_old = timed(lambda: teacher_path(lists))
    diff = max((a - b).abs().max().item() for a, b in zip(new, old))
    print(f"\n[{kind}] packed rows per user: a row per branch token {np.mean(before):.1f} (max {max(before)}), prefix-shared {np.mean(after):.1f} "
          f"(max {max(after)}); forward tokens {sum(before)} -> {sum(after)}")
    print(f"  score_items_batch                           {np.median(t_new):8.1f} ms per call  (runs: {', '.join(f'{t:.1f}' for t in t_new)})")
    print(f"  score_branches_batch + log-softmax + gather {np.median(t_old):8.1f} ms per call  (runs: {', '.join(f'{t:.1f}' for t in t_old)})")
    print(f"  ratio old / new {np.median(t_old) / np.median(t_new):.2f}; largest |difference| of the {sum(len(l) for l in lists)} scores {diff:.4f} "
          f"(bf16, two batch shapes)")
