#!/usr/bin/env python3
"""What resident per-user adapters cost (profiles/lora_multi_cost.txt).

  python3 tools/lora_multi_cost.py [--users N] [--batch U] [--reps R] [--wide]

Full Llama-7B(32L) / Llama-68M dims in bf16, Beauty, K = 20 / DK = 40, gamma 4, random-init weights (acceptance ~ 0), rank-8 q / v adapters,
the way tools/lora_cost.py runs:
  (a) a lock-step BSSD_batch of U users with every user on ONE resident adapter;
  (b) the same batch with four resident adapters dealt round-robin;
  (c) one user per call under a resident adapter.
--wide measures (a) and (c) with the same adapter loaded model-wide (load_lora) instead and touches nothing the resident adapters added, so
the same file runs on the parent commit: the line (a) is compared with.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from atspeed_amd import synth
from atspeed_amd.beamSD import BSSD, BSSD_batch, release_decoders
from atspeed_amd.generation_trie import PositionSetConstraint
from atspeed_amd.model import HipLlama

DEV = torch.device("cuda", 0)
V = synth.BEAUTY.vocab_size


def _prompts(n):
    plens = synth.prompt_lengths(n, 2025)
    return [{"input_ids": torch.from_numpy(synth.synthetic_prompt(int(plens[u]), synth.tensor_seed(2025, f"user{u}")))[None].to(DEV)} for u in range(n)]


def _batch(tag, tgt, drf, many, fn, reps, **kw):
    BSSD_batch(tgt, drf, many, 4, 4, prefix_allowed_tokens_fn=fn, **kw)
    torch.cuda.synchronize()
    tgt.lora_launches(reset=True)
    t0 = time.perf_counter()
    for _ in range(reps):
        BSSD_batch(tgt, drf, many, 4, 4, prefix_allowed_tokens_fn=fn, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    print(f"MARK lock-step batch of {len(many)} users, {tag}: {1e3 * dt:.1f} ms per batch, {len(many) * 20 / dt:.1f} items/s "
          f"({tgt.lora_launches() // reps} adapter launches per batch)", flush=True)


def _one(tag, tgt, drf, one, fn, **kw):
    for p in one[:2]:
        BSSD(tgt, drf, p, 4, 4, prefix_allowed_tokens_fn=fn, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = [BSSD(tgt, drf, p, 4, 4, prefix_allowed_tokens_fn=fn, **kw) for p in one[2:]]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"MARK one user per call, {tag}: {1e3 * dt / len(outs):.2f} ms/user ({len(outs)} users, "
          f"{sum(o['n_target_forwards'] for o in outs)} target forwards)", flush=True)


def main(args):
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=DEV)
    fn = PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    drf = HipLlama.from_synthetic(synth.llama_68m(V), 2026, dtype=torch.bfloat16, num_beams=40, **kw)
    tgt = HipLlama.from_synthetic(synth.llama_7b(V, 32), 2025, dtype=torch.bfloat16, num_beams=20, **kw)
    one, many = _prompts(args.users + 2), _prompts(args.batch)
    lora = lambda seed: synth.synthetic_lora(tgt.dims, seed, r=8, modules=("q", "v"), std=0.02)
    if args.wide:
        tgt.load_lora(lora(78), r=8, lora_alpha=16)
        _batch("model-wide rank-8 q/v adapter (load_lora)", tgt, drf, many, fn, args.reps)
        _one("model-wide rank-8 q/v adapter (load_lora)", tgt, drf, one, fn)
    else:
        names = ["w0", "w1", "w2", "w3"]
        for i, name in enumerate(names):
            tgt.add_lora(lora(78 + i), name, r=8, lora_alpha=16)
        _batch("(a) every user on ONE resident rank-8 q/v adapter", tgt, drf, many, fn, args.reps, adapters=["w0"] * len(many))
        _batch("(b) four resident adapters dealt round-robin", tgt, drf, many, fn, args.reps, adapters=[names[u % 4] for u in range(len(many))])
        _batch("    nobody names one of the four resident adapters", tgt, drf, many, fn, args.reps)
        _one("(c) a resident rank-8 q/v adapter", tgt, drf, one, fn, adapter="w0")
    release_decoders(tgt, drf)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--users", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2)
    main(ap.parse_args())
