#!/usr/bin/env python3
"""A/B of the row-pruned tail of the last layer (switch `tail_rows_tokens`) on prefill-only lock-step batches: full
Llama-7B dims, bf16, Beauty prompts, K=20, ONE new token -- `target_generate_batch` is then one target forward over every user's prompt with
one logit row per user, the shape of phase 0 of a staged round and of every large prefill.  Per batch size the two forms alternate in ONE
process, `reps` times each after a warm-up of each: full = switch at a value no forward exceeds, pruned = switch at 0.  The default of the
switch is read off this table: the smallest forward from which the pruned form is not slower than the full runs' own spread.
usage: python3 tools/tail_rows_ab.py [--users 4,8,16,32,64,128,256] [--reps 5] [--layers 32] [--bssd]
--bssd: time whole BSSD_batch calls of the headline recipe (gamma 4, 4 new tokens, library defaults otherwise) instead."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD_batch, release_decoders, target_generate_batch
from atspeed_amd.generation_trie import PositionSetConstraint
from atspeed_amd.model import HipLlama

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=str, default="4,8,16,32,64,128,256")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--bssd", action="store_true")
args = ap.parse_args()
K, DK, GAMMA, NEW = 20, 40, 4, 4
NEVER = 1 << 30
dev = torch.device("cuda", 0)
V = synth.BEAUTY.vocab_size
fn = PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
sizes = [int(x) for x in args.users.split(",")]
plens = synth.prompt_lengths(max(sizes), 2025)
prompts = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(int(plens[u]), synth.tensor_seed(2025, f"user{u}")))[None].to(dev)} for u in range(max(sizes))]
kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=dev)
t = HipLlama.from_synthetic(synth.llama_7b(V, args.layers), 2025, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=K, **kw)
d = HipLlama.from_synthetic(synth.llama_68m(V), 2026, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=DK, **kw) if args.bssd else None
what = f"BSSD_batch, gamma={GAMMA}, {NEW} new tokens, draft Llama-68M DK={DK}" if args.bssd else "target_generate_batch, 1 new token (one prefill forward)"
print(f"box: {torch.cuda.get_device_name(dev)}; {_lib.load().atspeed_version().decode()}", flush=True)
print(f"workload: {what}; target Llama-7B({args.layers}L) bf16 K={K}; {args.reps} timed calls per form and size, alternating, after one warm-up of each; "
      f"ms = wall time of one call", flush=True)


def run(ps, threshold):
    with _lib.switches(tail_rows_tokens=threshold):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        outs = BSSD_batch(t, d, ps, GAMMA, NEW, prefix_allowed_tokens_fn=fn) if args.bssd else target_generate_batch(t, ps, 1, prefix_allowed_tokens_fn=fn)
        torch.cuda.synchronize(dev)
        return outs, 1e3 * (time.perf_counter() - t0)


for n in sizes:
    ps = prompts[:n]
    forms = (("full", NEVER), ("pruned", 0))
    for _, th in forms:
        run(ps, th)
    walls, outs, log = {name: [] for name, _ in forms}, {}, None
    for rep in range(args.reps):
        for name, th in forms:
            if rep == 0 and name == "pruned":
                t.forward_log(1)
            outs[name], w = run(ps, th)
            walls[name].append(w)
            if rep == 0 and name == "pruned":
                log = t.forward_log(0)
    fm, pm = statistics.median(walls["full"]), statistics.median(walls["pruned"])
    spread = max(walls["full"]) - min(walls["full"])
    same = sum(int(torch.equal(a["beam_sequence"], b["beam_sequence"])) for a, b in zip(outs["full"], outs["pruned"]))
    dmax = max(float((a["beam_scores"] - b["beam_scores"]).abs().max()) for a, b in zip(outs["full"], outs["pruned"]))
    line = f"CELL users {n}: target forwards (tokens, logit rows) {log}"
    for name, _ in forms:
        w = sorted(walls[name])
        line += f"\n     {name:7s} {statistics.median(w):8.3f} ms [{w[0]:.3f} .. {w[-1]:.3f}]"
    line += (f"\n     full - pruned {fm - pm:+.3f} ms ({100 * (fm - pm) / fm:+.2f} %), slowest pruned - fastest full {max(walls['pruned']) - min(walls['full']):+.3f} ms; "
             f"spread of the full runs {spread:.3f} ms; beam_sequence identical {same}/{n}, max |d beam_scores| {dmax:.4f}")
    print(line, flush=True)
release_decoders(*([t, d] if d is not None else [t]))
