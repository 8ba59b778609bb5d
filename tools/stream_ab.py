#!/usr/bin/env python3
"""A/B of a list of users through chunked lock-step batches (BSSD_batch on chunks of `lanes` users, one chunk after the other) and through a
session of the same `lanes` lanes (BSSD_batch(..., lanes=N): each free lane refilled at the next round boundary).  Full Llama-7B /
Llama-68M dims, bf16, Beauty prompts (synth.prompt_lengths), K=20 / DK=40, gamma=4, 4 new tokens.  Three weight recipes: unrelated weights
(every verification accepts nothing: all users take the same rounds, the session cannot gain) and draft-aligned targets with resid_scale
3e-5 and 3e-4 (mixed acceptance).  Per cell the two paths alternate in ONE process, `reps` times each after a warm-up of both.
usage: python3 tools/stream_ab.py [--users 1024] [--lanes 16,64,256] [--recipes unrelated,3e-5,3e-4] [--reps 3] [--layers 32]
Prints, per cell: items/s of both paths (median and range), mean accepted length, the session's rounds and lane occupancy from its
counters, the rounds the chunked path ran (from its users' n_run), and the speed-up the round counts alone predict next to the measured one."""
import argparse
import ctypes as C
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
ap.add_argument("--users", type=int, default=1024)
ap.add_argument("--lanes", type=str, default="16,64,256")
ap.add_argument("--recipes", type=str, default="unrelated,3e-5,3e-4")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layers", type=int, default=32)
args = ap.parse_args()
K, DK, GAMMA, NEW = 20, 40, 4, 4
dev = torch.device("cuda", 0)
V = synth.BEAUTY.vocab_size
fn = PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
plens = synth.prompt_lengths(args.users, 2025)
prompts = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(int(plens[u]), synth.tensor_seed(2025, f"user{u}")))[None].to(dev)}
           for u in range(args.users)]
longest = max(range(args.users), key=lambda u: int(plens[u]))

tf = C.c_double()
scratch = torch.empty(4 << 20, dtype=torch.uint8, device=dev)
_lib.check(_lib.load().atspeed_probe_mfma_bf16(4000, scratch.data_ptr(), scratch.numel(), _lib.stream_ptr(dev), C.byref(tf)))
print(f"box: {torch.cuda.get_device_name(dev)}, MFMA probe (atspeed_probe_mfma_bf16, 16x16x32 bf16, 8 waves/CU) {tf.value:.0f} TFLOP/s; "
      f"{_lib.load().atspeed_version().decode()}", flush=True)
print(f"workload: {args.users} users, prompts {int(min(plens))}-{int(max(plens))} tokens, target Llama-7B({args.layers}L) / draft Llama-68M, bf16, "
      f"K={K} DK={DK} gamma={GAMMA} new tokens={NEW}; {args.reps} timed runs per path and cell, alternating, after one warm-up of each", flush=True)


def timed(call):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    outs = call()
    torch.cuda.synchronize(dev)
    return outs, time.perf_counter() - t0


def rate(walls):
    r = sorted(args.users * K / w for w in walls)
    return statistics.median(r), r[0], r[-1]


for recipe in args.recipes.split(","):
    rs = None if recipe == "unrelated" else float(recipe)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=dev)
    d = HipLlama.from_synthetic(synth.llama_68m(V), 2026, dtype=torch.bfloat16, num_beams=DK, resid_scale=1.0 if rs is None else rs, **kw)
    t = HipLlama.from_synthetic(synth.llama_7b(V, args.layers), 2025, dtype=torch.bfloat16, num_beams=K, resid_scale=1.0 if rs is None else rs,
                                align_to=(d if rs is not None else None), **kw)
    for lanes in (int(x) for x in args.lanes.split(",")):
        chunked = lambda ps: [o for i in range(0, len(ps), lanes) for o in BSSD_batch(t, d, ps[i:i + lanes], GAMMA, NEW, prefix_allowed_tokens_fn=fn)]
        session = lambda ps: BSSD_batch(t, d, ps, GAMMA, NEW, prefix_allowed_tokens_fn=fn, lanes=lanes)
        warm = prompts[:min(args.users, 2 * lanes)] + [prompts[longest]]       # the longest prompt sizes the session's buffers as the full list does
        chunked(warm), session(warm)
        walls = {"chunked": [], "session": []}
        logs = {}
        for rep_i in range(args.reps):
            for name, path in (("chunked", chunked), ("session", session)):
                if rep_i == args.reps - 1:
                    t.forward_log(1)                                          # token counts of the last run's target forwards
                outs, w = timed(lambda: path(prompts))
                walls[name].append(w)
                if rep_i == args.reps - 1:
                    logs[name] = sorted(tok for tok, _ in t.forward_log(0))
                if name == "chunked":
                    co = outs
                else:
                    so = outs
        same = sum(int(torch.equal(a["beam_sequence"], b["beam_sequence"])) for a, b in zip(co, so))
        acc = sum(o["total_accept_steps"] for o in so) / max(1, sum(o["n_run"] for o in so))
        need = [o["n_run"] + 1 for o in co]                                      # rounds a user takes part in (DESIGN.md "Sessions")
        chunk_rounds = sum(max(need[i:i + lanes]) for i in range(0, len(need), lanes))
        c = so[0]["session_counters"]
        (cm, clo, chi), (sm, slo, shi) = rate(walls["chunked"]), rate(walls["session"])
        # device time by stage (hipEvent brackets of every round, shared among its users: their sum is the path's total) and the target forwards' sizes
        stage = lambda outs: " / ".join(f"{sum(o[k] for o in outs):.3f}" for k in ("draft_time_cost", "target_time_cost", "verify_time_cost"))
        sizes = lambda lg: f"{len(lg)} forwards, tokens min {lg[0]} / median {lg[len(lg) // 2]} / max {lg[-1]} / sum {sum(lg)}" if lg else "none"
        print(f"CELL recipe {recipe} lanes {lanes}: chunked {cm:.0f} items/s [{clo:.0f} .. {chi:.0f}], session {sm:.0f} items/s [{slo:.0f} .. {shi:.0f}], "
              f"measured ratio {sm / cm:.3f}; mean accepted length {acc:.3f}, rounds per user {min(need)}-{max(need)}; "
              f"rounds chunked {chunk_rounds} / session {c['rounds']} -> ratio from the counters {chunk_rounds / c['rounds']:.3f}; "
              f"lane occupancy {c['lane_rounds'] / (c['rounds'] * c['n_lanes']):.3f} (chunked {sum(need) / (chunk_rounds * lanes):.3f}), "
              f"target forwards {c['target_forwards']}, draft forwards {c['draft_forwards']}, allocations after create {c['allocs_after_create']}, "
              f"arena reserved {c['arena_reserved']}; identical beam_sequence for {same} of {len(so)} users\n"
              f"     last run, device seconds draft / target / verify: chunked {stage(co)}, session {stage(so)}; wall {walls['chunked'][-1]:.3f} / {walls['session'][-1]:.3f} s\n"
              f"     last run, target forwards: chunked {sizes(logs['chunked'])}; session {sizes(logs['session'])}", flush=True)
    release_decoders(t, d)
    del t, d
    torch.cuda.empty_cache()
