#!/usr/bin/env python3
"""A/B of the forms of the 32-rows-per-wave attention kernel at the headline's shapes: 256 users, 32 heads x 128, bf16,
the prompt lengths of bench.py (70-184 tokens), through atspeed_segs_tree_attention with an explicit tile height.
  round20   20 query rows per user over prompt + 20 slots (the round inputs of a verification)
  round40   40 query rows per user over prompt + 60 slots (a draft block of a staged phase)
  prefill   the prompt's rows over the prompt's slots, causal
Forms: 64- or 128-row query tiles, the library's buffer count for that height (64: one tile buffer, 128: two) and, on a library built with the
experiment's instantiations (a switch `attn_ab`: bit 0 = the other buffer count, bit 1 = users outermost in the work order), the other
three.  Every form of a shape alternates in ONE process: `--reps` rounds of `--launches` launches each between two events; a launch reads the
caches of another layer than the one before (`--layers` layers of K and V per user, 2 MB each), so a launch's 0.4-0.7 GB of K/V never sits in
the 256 MB last-level cache from the launch before.  Prints the median, minimum and maximum microseconds per launch and the bytes of K/V a
launch fetches (tiles x 64 keys x 512 B per workgroup).
usage: python3 tools/attn_short_ab.py [--users 256] [--reps 7] [--launches 8] [--layers 4]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from atspeed_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--launches", type=int, default=8)
ap.add_argument("--layers", type=int, default=4)
args = ap.parse_args()
N, HEADS, DH, VW = args.users, 32, 128, 4
H, S = HEADS * DH, VW * 64
lib = _lib.load()
dev = torch.device("cuda", 0)
has_ab = lib.atspeed_set_switch(b"attn_ab", 0) == 0
print(f"box: {torch.cuda.get_device_name(dev)}; {lib.atspeed_version().decode()}; experiment switch attn_ab: {'yes' if has_ab else 'no'}")
plens = synth.prompt_lengths(N, 2025)
kc = torch.empty(N, args.layers, S, H, dtype=torch.bfloat16, device=dev).normal_()
vc = torch.empty(N, args.layers, S, H, dtype=torch.bfloat16, device=dev).normal_()
print(f"{N} users, prompts {int(plens.min())}-{int(plens.max())} (mean {plens.mean():.1f}); caches {args.layers} layers x {S} slots x {H} per user: "
      f"{2 * kc.numel() * 2 / 2**30:.2f} GB of K and V, a launch reads one layer of it; {args.reps} x {args.launches} launches per form, alternating")


def shape(name):
    """-> rows per user, slots per user, visibility [rows][slots] per user"""
    rows, slots, vis = [], [], []
    for p in (int(x) for x in plens):
        t, s = {"round20": (20, p + 20), "round40": (40, p + 60), "prefill": (p, p)}[name]
        v = np.zeros((t, S), dtype=np.uint8)
        if name == "prefill":
            v[:, :p] = np.tril(np.ones((p, p), dtype=np.uint8))
        else:
            v[:, : s - t] = 1                                  # everything before the block and the row itself
            v[np.arange(t), s - t + np.arange(t)] = 1
        rows.append(t); slots.append(s); vis.append(np.packbits(v, axis=1, bitorder="little").view(np.uint64))
    return rows, slots, vis


def run_shape(name):
    rows, slots, vis = shape(name)
    T = sum(rows)
    q = torch.empty(T, 3 * H, dtype=torch.bfloat16, device=dev).normal_()        # the qkv buffer of a forward: q is its first H columns
    out = torch.empty((T + 1) // 2 * 2, H, dtype=torch.bfloat16, device=dev)
    visd = [torch.from_numpy(v.view(np.int64)).to(dev) for v in vis]
    arr = lambda ptrs: (C.c_void_p * N)(*ptrs)
    cnt = lambda v: (C.c_int32 * N)(*v)
    segs = [N, None, None, None, arr([v.data_ptr() for v in visd]), arr([kc[u].data_ptr() for u in range(N)]), arr([vc[u].data_ptr() for u in range(N)]),
            cnt(rows), cnt(slots), cnt([0] * N)]
    st = _lib.stream_ptr()

    def launch(qtile, layer):
        _lib.check(lib.atspeed_segs_tree_attention(q.data_ptr(), 3 * H, layer * S * H * 2, VW, out.data_ptr(), H, HEADS, DH, _lib.dtype_code(torch.bfloat16), qtile, 32, 0,
                                                   *segs, st))

    forms = [("64 rows, 1 buffer", 64, 0), ("128 rows, 2 buffers", 128, 0)]
    if has_ab:
        forms += [("64 rows, 2 buffers", 64, 1), ("128 rows, 1 buffer", 128, 1)]
        if name != "prefill":                                  # one query tile per user at either height: the work order applies
            forms += [(f"{label}, users outermost", qt, ab | 2) for label, qt, ab in list(forms)]
    want, us = None, {f[0]: [] for f in forms}
    for rep in range(args.reps + 1):                           # (round 0 warms up and checks the forms against each other)
        for label, qt, ab in forms:
            if has_ab:
                _lib.check(lib.atspeed_set_switch(b"attn_ab", ab))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.launches):
                launch(qt, (rep * args.launches + i) % args.layers)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                us[label].append(1e3 * e0.elapsed_time(e1) / args.launches)
            else:
                launch(qt, 0)
                torch.cuda.synchronize()
                got = out[:T].clone()
                want = got if want is None else want
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{label}: output differs from the first form's"
    if has_ab:
        _lib.check(lib.atspeed_set_switch(b"attn_ab", 0))
    print(f"SHAPE {name}: {T} rows, {sum(slots) / N:.0f} slots per user on average; every form's output bit-identical")
    for label, qt, _ in forms:
        wgs = sum((r + qt - 1) // qt for r in rows) * HEADS
        mb = sum(((r + qt - 1) // qt) * ((s + 63) // 64) for r, s in zip(rows, slots)) * HEADS * 64 * 512 / 1e6
        m = statistics.median(us[label])
        print(f"     {label:40s} {m:8.1f} us [{min(us[label]):.1f} .. {max(us[label]):.1f}]  {wgs} workgroups, {mb:.0f} MB of K/V tiles, {mb / m:.2f} TB/s")


for name in ("round20", "round40", "prefill"):
    run_shape(name)
