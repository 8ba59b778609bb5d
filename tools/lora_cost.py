#!/usr/bin/env python3
"""What the unmerged LoRA target costs and what it buys (profiles/lora_cost.txt, profiles/lora_fp8_merge_vs_side.txt).

  python3 tools/lora_cost.py cost [--no_lora] [--users N] [--batch U] [--reps R]
      Full Llama-7B(32L) / Llama-68M dims, Beauty, K = 20 / DK = 40, random-init weights (acceptance ~ 0): one user per call in bf16 and W8A8
      (ms per user) and one lock-step batch of U users in bf16 (items/s), each without and with a rank-8 q / v adapter on the target.
      --no_lora measures the adapter-free lines only and touches nothing this feature added, so the same file runs on the parent commit.
  python3 tools/lora_cost.py merge [--layers 3] [--ranks 8,64]
      Llama-7B width: the adapter-induced logit shift of a W8A8 and of a W4A8 target, once with the adapter merged into the 16-bit weights
      BEFORE they are quantised and once on the side path, against the same shift of the fp32 engine (weights = the bf16 values, adapter on its
      fp32 side path: the arithmetic tests/test_lora_gpu.py pins to the CPU reference).
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
from atspeed_amd.model import HipLlama, vis_bits_from_bool

DEV = torch.device("cuda", 0)
V = synth.BEAUTY.vocab_size


def _prompts(n):
    plens = synth.prompt_lengths(n, 2025)
    return [{"input_ids": torch.from_numpy(synth.synthetic_prompt(int(plens[u]), synth.tensor_seed(2025, f"user{u}")))[None].to(DEV)} for u in range(n)]


def cost(args):
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=DEV)
    fn = PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
    drf = HipLlama.from_synthetic(synth.llama_68m(V), 2026, dtype=torch.bfloat16, num_beams=40, **kw)
    one, many = _prompts(args.users + 2), _prompts(args.batch)
    for prec in ("bf16", "fp8"):
        tgt = HipLlama.from_synthetic(synth.llama_7b(V, 32), 2025, dtype=torch.bfloat16, num_beams=20, **kw)
        if prec == "fp8":
            tgt.enable_fp8()
        for lora in ((False,) if args.no_lora else (False, True, False)):          # off, on, off again: the adapter-free line twice in one process
            if lora:
                tgt.load_lora(synth.synthetic_lora(tgt.dims, 78, r=8, modules=("q", "v"), std=0.02), r=8, lora_alpha=16)
            elif not args.no_lora:
                tgt.unload_lora()
            tag = f"{prec} {'rank-8 q/v adapter' if lora else 'no adapter'}"
            for p in one[:2]:
                BSSD(tgt, drf, p, 4, 4, prefix_allowed_tokens_fn=fn)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = [BSSD(tgt, drf, p, 4, 4, prefix_allowed_tokens_fn=fn) for p in one[2:]]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            acc = sum(o["total_accept_steps"] for o in outs) / max(1, sum(o["n_run"] for o in outs))
            print(f"MARK one user per call, {tag}: {1e3 * dt / args.users:.2f} ms/user ({args.users} users, accept {acc:.3f}, "
                  f"{sum(o['n_target_forwards'] for o in outs)} target forwards)", flush=True)
            if prec == "bf16":
                BSSD_batch(tgt, drf, many, 4, 4, prefix_allowed_tokens_fn=fn)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    BSSD_batch(tgt, drf, many, 4, 4, prefix_allowed_tokens_fn=fn)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.reps
                print(f"MARK lock-step batch of {args.batch} users, {tag}: {1e3 * dt:.1f} ms per batch, {args.batch * 20 / dt:.1f} items/s", flush=True)
        release_decoders(tgt, drf)
        del tgt


def _forward(m, seq, rows):
    ids, pos, vis = seq
    T = ids.numel()
    return m.forward_raw(ids.to(DEV), pos.to(DEV), pos.clone().to(DEV), vis_bits_from_bool(vis, 512).to(DEV), T, rows).float().clone()


def merge(args):
    dims = synth.llama_7b(V, args.layers)
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=448, device=DEV)
    g = torch.Generator().manual_seed(6)
    T, rows = 228, 64
    ids = torch.cat((torch.randint(3, 32000, (T - 30,), generator=g), torch.randint(32000, V, (30,), generator=g))).to(torch.int32)
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
    vis[10:, 7] = False
    seq = (ids, torch.arange(T, dtype=torch.int32), vis)
    make16 = lambda: HipLlama.from_synthetic(dims, 2025, std=0.02, head_std=0.05, dtype=torch.bfloat16, **kw)
    sd = make16().export_state_dict()                                       # the bf16 weight values, fp32 on the host
    f32 = HipLlama.from_state_dict(dims, sd, torch.float32, **kw)
    base32 = _forward(f32, seq, rows)
    scale = float(base32.abs().max())
    print(f"# {args.layers} layers at hidden 4096 / ffn 11008 / 32 x 128, one 228-token forward, {rows} logit rows; max |logit| {scale:.3f}")
    print("# shift = logits(with adapter) - logits(without), same arithmetic both times; error = |shift - fp32 shift|, relative to mean |fp32 shift|")
    base_q = {}
    for fmt in ("fp8", "fp4"):
        m = make16()
        getattr(m, "enable_" + fmt)()
        base_q[fmt] = _forward(m, seq, rows)
        del m
    for r in args.ranks:
        for std in (0.02, 0.005):
            t = synth.synthetic_lora(dims, 78, r=r, modules=("q", "v"), std=std)
            f32.load_lora(t, r=r, lora_alpha=16)
            want = _forward(f32, seq, rows) - base32
            f32.unload_lora()
            ws = float(want.abs().mean())
            # merged: W + scaling B A in fp32, rounded to bf16 (what a merge tool would save), then quantised by enable_fp8 / enable_fp4
            msd = dict(sd)
            s = 16.0 / r                                                    # alpha / r, as load_lora(..., lora_alpha=16)
            for l in range(dims.n_layers):
                for mod in ("q", "v"):
                    p = f"base_model.model.model.layers.{l}.self_attn.{mod}_proj."
                    a, b = torch.from_numpy(t[p + "lora_A.weight"]).to(torch.bfloat16).float(), torch.from_numpy(t[p + "lora_B.weight"]).to(torch.bfloat16).float()
                    k = f"model.layers.{l}.self_attn.{mod}_proj.weight"
                    msd[k] = sd[k] + s * (b @ a)
            for fmt in ("fp8", "fp4"):
                res = {}
                side = make16()
                getattr(side, "enable_" + fmt)()
                side.load_lora(t, r=r, lora_alpha=16)
                res["side path"] = _forward(side, seq, rows) - base_q[fmt]
                del side
                mg = HipLlama.from_state_dict(dims, msd, torch.bfloat16, **kw)
                getattr(mg, "enable_" + fmt)()
                res["merged, then quantised"] = _forward(mg, seq, rows) - base_q[fmt]
                del mg
                for how, shift in res.items():
                    e = (shift - want).abs()
                    print(f"MARK rank {r} adapter std {std} ({'W8A8' if fmt == 'fp8' else 'W4A8'}, {how}): fp32 shift mean {ws / scale:.4f} of max|logit|; "
                          f"shift error mean {float(e.mean()) / ws:.3f} max {float(e.max()) / ws:.3f} of mean |fp32 shift|", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("cost", "merge"))
    ap.add_argument("--no_lora", action="store_true")
    ap.add_argument("--users", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--ranks", type=lambda s: [int(x) for x in s.split(",")], default=[8, 64])
    a = ap.parse_args()
    (cost if a.mode == "cost" else merge)(a)
