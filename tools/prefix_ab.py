#!/usr/bin/env python3
"""A/B of prompt prefixes (`PromptPrefix`) on the headline shape: full Llama-7B dims, bf16, 256 users in lock step,
`BSSD_batch` (gamma 4, 4 new tokens, K=20, draft Llama-68M DK=40) and `target_generate_batch` (4 new tokens).  Seeded prompts of 66-186
tokens share their first `--prefix_len` tokens.  Per prefix length the two forms -- prefix off, prefix on -- alternate in ONE process,
`reps` calls each after a warm-up of each; a call's time is taken from device events around it (its host work included: the call ends with
its own stream synchronisation).  The scatter launch is timed alone (`atspeed_kv_rows_scatter` into 256 arena pairs) next to a plain
device-to-device copy of the same bytes (torch's contiguous same-type `copy_`: one hipMemcpyAsync) in the same run.
usage: python3 tools/prefix_ab.py [--prefix_len 16,36,64] [--users 256] [--reps 3] [--layers 32] [--out profiles/prefix_cache_ab.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD_batch, release_decoders, target_generate_batch
from atspeed_amd.generation_trie import PositionSetConstraint
from atspeed_amd.model import HipLlama, PromptPrefix

ap = argparse.ArgumentParser()
ap.add_argument("--prefix_len", type=str, default="16,36,64")
ap.add_argument("--users", type=int, default=256)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--out", type=str, default=None, help="append the report to this file as well")
args = ap.parse_args()
K, DK, GAMMA, NEW = 20, 40, 4, 4
dev = torch.device("cuda", 0)
V = synth.BEAUTY.vocab_size
fn = PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
lib = _lib.load()
out_f = open(args.out, "a") if args.out else None


def say(line):
    print(line, flush=True)
    if out_f:
        out_f.write(line + "\n")
        out_f.flush()


kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=dev)
t = HipLlama.from_synthetic(synth.llama_7b(V, args.layers), 2025, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=K, **kw)
d = HipLlama.from_synthetic(synth.llama_68m(V), 2026, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=DK, **kw)
say(f"box: {torch.cuda.get_device_name(dev)}; {lib.atspeed_version().decode()}")
say(f"workload: {args.users} users in lock step, target Llama-7B({args.layers}L) bf16 K={K}, draft Llama-68M DK={DK}, gamma={GAMMA}, {NEW} new tokens; prompts of "
    f"66-186 tokens (seeded) sharing their first Lp tokens; {args.reps} timed calls per form, off / on alternating, after one warm-up of each; ms = device "
    f"events around one call")
lens = 66 + (synth.hash_u32(np.arange(args.users, dtype=np.uint64), synth.tensor_seed(2025, "prefix_ab.len")) % 121).astype(np.int64)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    outs = call()
    e1.record()
    torch.cuda.synchronize(dev)
    return outs, e0.elapsed_time(e1)


def scatter_cell(lp):
    """the scatter launch alone against a plain copy of the same bytes: arenas of 128 slots (the stride changes addresses, not bytes)"""
    n, layers, row_bytes, slots = args.users, args.layers, t.dims.hidden * 2, 128
    arena = layers * slots * row_bytes
    store = [torch.randint(0, 255, (layers * lp * row_bytes,), dtype=torch.uint8, device=dev) for _ in range(2)]
    buf = torch.zeros(2 * n, arena, dtype=torch.uint8, device=dev)
    ptrs = lambda rows: (C.c_void_p * n)(*[buf[r].data_ptr() for r in rows])
    ka, va = ptrs(range(0, 2 * n, 2)), ptrs(range(1, 2 * n, 2))
    moved = 2 * n * layers * lp * row_bytes
    src, dst = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    sc = lambda: _lib.check(lib.atspeed_kv_rows_scatter(store[0].data_ptr(), store[1].data_ptr(), ka, va, n, lp, layers, row_bytes, slots, st))
    sc(), dst.copy_(src)
    ms_s = sorted(timed(sc)[1] for _ in range(5))
    ms_c = sorted(timed(lambda: dst.copy_(src))[1] for _ in range(5))
    say(f"     scatter alone: {moved / 1e9:.2f} GB written to {n} users' K and V arenas ({2 * layers * lp * row_bytes / 1e6:.1f} MB read once): median {ms_s[2]:.3f} ms "
        f"[{ms_s[0]:.3f} .. {ms_s[-1]:.3f}] = {moved / ms_s[2] / 1e6:.0f} GB/s written; device-to-device copy of the same bytes: median {ms_c[2]:.3f} ms "
        f"[{ms_c[0]:.3f} .. {ms_c[-1]:.3f}] = {moved / ms_c[2] / 1e6:.0f} GB/s")
    return ms_s[2]


for lp in [int(x) for x in args.prefix_len.split(",")]:
    head = synth.synthetic_prompt(lp + 8, synth.tensor_seed(2025, "prefix_ab.head"))[:lp]
    prompts = [synth.synthetic_prompt(int(lens[u]), synth.tensor_seed(2025, f"prefix_ab.user{u}")) for u in range(args.users)]
    for p in prompts:
        p[:lp] = head                                                 # (the shortest prompt keeps its Response separator: 66 >= Lp + 2)
    ps = [{"input_ids": torch.from_numpy(p)[None].to(dev)} for p in prompts]
    pre = PromptPrefix(t, d, head)
    rows = int(sum(len(p) for p in prompts))
    say(f"CELL Lp {lp}: prompt rows {rows} ({rows / args.users:.1f} per user), of which the prefix is {lp * args.users} ({100 * lp * args.users / rows:.1f} %); "
        f"prefix store {pre.info()['bytes'] / 1e6:.1f} MB (target) + {pre.info(True)['bytes'] / 1e6:.1f} MB (draft)")
    ms_scatter = scatter_cell(lp)
    for name, call in (("BSSD_batch", lambda p: BSSD_batch(t, d, ps, GAMMA, NEW, prefix_allowed_tokens_fn=fn, prefix=p)),
                       ("target_generate_batch", lambda p: target_generate_batch(t, ps, NEW, prefix_allowed_tokens_fn=fn, prefix=p))):
        forms = (("off", None), ("on", pre))
        for _, p in forms:
            call(p)
        ms, outs = {f: [] for f, _ in forms}, {}
        for rep in range(args.reps):
            for f, p in forms:
                outs[f], w = timed(lambda: call(p))
                ms[f].append(w)
        off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
        spread = max(ms["off"]) - min(ms["off"])
        # the prefix rows come from a one-user forward, the full prompts' from the batch's ring kernels: two 16-bit routes to the same values.
        # These synthetic weights give near-flat scores, so a beam list is decided by that noise: compare the beams both forms returned
        same = sum(int(torch.equal(a["beam_sequence"], b["beam_sequence"])) for a, b in zip(outs["off"], outs["on"]))
        common, dmax = 0, 0.0
        for a, b in zip(outs["off"], outs["on"]):
            sa = {tuple(r[-NEW:]): float(x) for r, x in zip(a["beam_sequence"].tolist(), a["beam_scores"].tolist())}
            sb = {tuple(r[-NEW:]): float(x) for r, x in zip(b["beam_sequence"].tolist(), b["beam_scores"].tolist())}
            both = set(sa) & set(sb)
            common += len(both)
            dmax = max([dmax] + [abs(sa[k] - sb[k]) for k in both])
        line = f"     {name}:"
        for f, _ in forms:
            w = sorted(ms[f])
            line += f" {f} {statistics.median(w):9.3f} ms [{w[0]:.3f} .. {w[-1]:.3f}];"
        say(line + f" off - on {off - on:+.3f} ms ({100 * (off - on) / off:+.2f} %), spread of the off runs {spread:.3f} ms; the scatter launches cost "
            f"~{ms_scatter:.3f} ms (target, measured above) of it; beam lists identical for {same}/{args.users} users, {common / args.users:.1f} of {K} beams in common per user, max |d score| of a common beam {dmax:.4f}")
    pre.close()
release_decoders(t, d)
if out_f:
    out_f.close()
