#!/usr/bin/env python3
"""Accepted-length drift of the 8- and 4-bit targets against the bf16 target on an aligned pair (tests/test_fp8_gpu.py
test_fp8_accept_length_drift_on_an_aligned_pair, llama7b_width recipe: 4-layer Llama-7B-wide target aligned to the Llama-68M draft, 64 users,
the first residual scale of the list at which the bf16 pair accepts a mixed number of steps)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import atspeed_amd
from atspeed_amd import synth
from atspeed_amd.beamSD import BSSD_batch, release_decoders
from atspeed_amd.model import HipLlama
V = synth.BEAUTY.vocab_size
fn = atspeed_amd.PositionSetConstraint(synth.BEAUTY.allowed_tokens(), synth.RESPONSE_SEP)
kw = dict(dtype=torch.bfloat16, max_slots=512, max_tokens=512, max_logit_rows=448)
inputs = [{"input_ids": torch.from_numpy(synth.synthetic_prompt(64, 900 + u))[None].cuda()} for u in range(64)]
mean_acc = lambda outs: sum(o["total_accept_steps"] for o in outs) / max(1, sum(o["n_run"] for o in outs))
for rs in (3e-5, 1e-4, 3e-4, 1e-3):
    res = {}
    for prec in ("bf16", "fp8", "fp4"):
        drf = HipLlama.from_synthetic(synth.llama_68m(V), 32, std=0.02, head_std=0.02, num_beams=40, resid_scale=rs, **kw)
        tgt = HipLlama.from_synthetic(synth.llama_7b(V, 4), 31, std=0.02, head_std=0.02, num_beams=20, resid_scale=rs, align_to=drf, **kw)
        if prec == "fp8": tgt.enable_fp8()
        if prec == "fp4": tgt.enable_fp4()
        res[prec] = mean_acc(BSSD_batch(tgt, drf, inputs, 4, 4, prefix_allowed_tokens_fn=fn))
        release_decoders(tgt, drf)
        del tgt, drf
        if prec == "bf16" and not (0.2 < res["bf16"] < 2.8):
            break
    print(f"MARK drift resid_scale {rs:g}: mean accepted steps bf16 {res['bf16']:.3f}" +
          (f" fp8 {res['fp8']:.3f} ({res['fp8'] - res['bf16']:+.3f}) fp4 {res['fp4']:.3f} ({res['fp4'] - res['bf16']:+.3f})" if len(res) == 3 else " (not mixed)"), flush=True)
    if len(res) == 3:
        break
