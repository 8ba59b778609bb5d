#!/usr/bin/env python3
"""A/B of packed against staged verification (switch `verify_staged`, DESIGN.md "Staged verification") on lock-step batches of 4 .. 256 users:
full Llama-7B / Llama-68M dims, bf16, Beauty prompts, K=20 / DK=40, gamma=4, 4 new tokens -- the headline recipe (unrelated weights: every
verification stops at step 0) and the two draft-aligned brackets of bench.py (resid_scale 3e-6 and 3e-5: most blocks accepted).  Per cell
four modes alternate in ONE process, `reps` times each after a warm-up of each: 0 = packed, 2 = every round staged, `first` = only the
first round staged (switch 1 with the threshold between the first round's packed token count and the later rounds' and no pass cost), so
every cell gives the gain at two round sizes, and `auto` = the library's defaults.  The threshold T* (`verify_staged_tokens`) and the cost of
a phase (`verify_staged_pass_tokens`) are read off this table.
usage: python3 tools/staged_verify_ab.py [--users 4,16,64,256] [--recipes unrelated,3e-6,3e-5] [--reps 3] [--layers 32]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD_batch, release_decoders
from atspeed_amd.generation_trie import PositionSetConstraint
from atspeed_amd.model import HipLlama

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=str, default="4,16,64,256")
ap.add_argument("--recipes", type=str, default="unrelated,3e-6,3e-5")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layers", type=int, default=32)
args = ap.parse_args()
K, DK, GAMMA, NEW = 20, 40, 4, 4
dev = torch.device("cuda", 0)
V = synth.BEAUTY.vocab_size
fn = PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
sizes = [int(x) for x in args.users.split(",")]
n_max = max(sizes)
plens = synth.prompt_lengths(n_max, 2025)
prompts = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(int(plens[u]), synth.tensor_seed(2025, f"user{u}")))[None].to(dev)} for u in range(n_max)]
print(f"box: {torch.cuda.get_device_name(dev)}; {_lib.load().atspeed_version().decode()}", flush=True)
print(f"workload: prompts {int(min(plens))}-{int(max(plens))} tokens, target Llama-7B({args.layers}L) / draft Llama-68M, bf16, K={K} DK={DK} gamma={GAMMA} "
      f"new tokens={NEW}; {args.reps} timed calls per mode and cell, alternating, after one warm-up of each; ms = wall time of one BSSD_batch call", flush=True)


def run(t, d, ps, mode, threshold):
    sw = dict(verify_staged=mode) if threshold is None else dict(verify_staged=mode, verify_staged_tokens=threshold, verify_staged_pass_tokens=0)
    with _lib.switches(**sw):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        outs = BSSD_batch(t, d, ps, GAMMA, NEW, prefix_allowed_tokens_fn=fn)
        torch.cuda.synchronize(dev)
        return outs, 1e3 * (time.perf_counter() - t0)


for recipe in args.recipes.split(","):
    rs = None if recipe == "unrelated" else float(recipe)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=dev)
    d = HipLlama.from_synthetic(synth.llama_68m(V), 2026, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=DK, resid_scale=1.0 if rs is None else rs, **kw)
    t = HipLlama.from_synthetic(synth.llama_7b(V, args.layers), 2025, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=K,
                                resid_scale=1.0 if rs is None else rs, align_to=(d if rs is not None else None), **kw)
    for n in sizes:
        ps = prompts[:n]
        t.forward_log(1)
        base, _ = run(t, d, ps, 0, 0)
        plog = [tok for tok, _ in t.forward_log(0)]                           # packed tokens per round
        cut = (plog[0] + max(plog[1:], default=0)) // 2                       # between the first round's tokens and the largest later round's
        modes = (("packed", 0, 0), ("staged", 2, 0), ("first", 1, cut), ("auto", 1, None))
        for _, m, th in modes[1:]:
            run(t, d, ps, m, th)
        walls = {name: [] for name, _, _ in modes}
        outs, logs = {}, {}
        for rep_i in range(args.reps):
            for name, m, th in modes:
                if rep_i == args.reps - 1:
                    t.forward_log(1)
                outs[name], w = run(t, d, ps, m, th)
                walls[name].append(w)
                if rep_i == args.reps - 1:
                    logs[name] = [tok for tok, _ in t.forward_log(0)]
        acc = sum(o["total_accept_steps"] for o in base) / max(1, sum(o["n_run"] for o in base))
        cell = f"CELL recipe {recipe} users {n}: mean accepted length {acc:.2f}, packed rounds of {plog} tokens"
        for name, _, _ in modes:
            w = sorted(walls[name])
            cell += f"\n     {name:7s} {statistics.median(w):8.2f} ms [{w[0]:.2f} .. {w[-1]:.2f}]  target passes {len(logs[name])}, tokens {sum(logs[name])}"
        pm, spread = statistics.median(walls["packed"]), max(walls["packed"]) - min(walls["packed"])
        same = lambda a, b, key: sum(int(x[key] == y[key]) for x, y in zip(a, b))
        so = outs["staged"]
        seq_same = sum(int(torch.equal(a["beam_sequence"], b["beam_sequence"])) for a, b in zip(base, so))
        dmax = max([float((a["beam_scores"] - b["beam_scores"]).abs().max()) for a, b in zip(base, so) if not torch.equal(a["beam_sequence"], b["beam_sequence"])], default=0.0)
        cell += (f"\n     packed / staged {pm / statistics.median(walls['staged']):.3f}, packed / first {pm / statistics.median(walls['first']):.3f}, packed / auto {pm / statistics.median(walls['auto']):.3f}; spread of the packed runs {spread:.2f} ms"
                 f"\n     staged against packed: identical accept_steps {same(base, so, 'accept_steps')}/{n}, n_run {same(base, so, 'n_run')}/{n}, "
                 f"n_target_forwards {same(base, so, 'n_target_forwards')}/{n}, n_draft_forwards {same(base, so, 'n_draft_forwards')}/{n}, "
                 f"beam_sequence {seq_same}/{n}; max |d beam_scores| over the others {dmax:.4f}")
        print(cell, flush=True)
    release_decoders(t, d)
    del t, d
    torch.cuda.empty_cache()
