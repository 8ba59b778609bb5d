"""What the sampling-mode warpers cost: (1) the cutoff kernel alone (`atspeed_warp_cutoffs`, hipEvent-timed) at the row counts of the
bench's lock-step batches, (2) sampled BSSD_batch calls of the bench's model pair with the warpers off / top_k = 50 / top_k = 50 + top_p = 0.9,
interleaved.  The draws differ between the settings, so (2) also prints rounds and accepted steps: compare ms per round, not per batch.

    python tools/sample_warp_cost.py [--streams 256] [--reps 3] [--target-layers 32]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                       # noqa: E402  (the workload pieces of the benchmark)
from atspeed_amd import _lib, synth                                # noqa: E402
from atspeed_amd.beamSD import BSSD_batch, _DeviceFSM             # noqa: E402
from atspeed_amd.model import HipLlama                             # noqa: E402

SETTINGS = [("off", None, None), ("top_k=50", 50, None), ("top_k=50,top_p=0.9", 50, 0.9)]


def kernel_alone(fn, prompt, V, dev, mask_name):
    lib = _lib.load()
    fsm = fn.compile(prompt.tolist())
    n_nodes = len(fsm.row_ptr) - 1
    deg = np.diff(np.asarray(fsm.row_ptr))
    h = _DeviceFSM.get(fsm, V).handle
    st = _lib.stream_ptr(dev)
    print(f"# cutoff kernel alone, {mask_name} mask: {n_nodes} nodes, children per node {int(deg.min())}-{int(deg.max())} (mean {deg.mean():.1f}), V = {V}")
    print("#   rows   top_k  top_p   us per launch (min / median of 20)")
    for rows in (20, 40, 5120, 10240, 25600):
        logits = torch.randn(rows, V, device=dev) * 2
        lse = torch.logsumexp(logits, 1).contiguous()
        inner = np.nonzero(deg >= 1)[0]                               # rows of a step sit on nodes that have children
        nodes = torch.from_numpy(inner[np.arange(rows) % len(inner)].astype(np.int32)).to(dev)
        cut = torch.empty(rows, dtype=torch.float32, device=dev)
        for top_k, top_p in ((50, 1.0), (50, 0.9), (0, 0.9)):
            ts = []
            for i in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(lib.atspeed_warp_cutoffs(logits.data_ptr(), V, lse.data_ptr(), rows, h, nodes.data_ptr(), 1.0, top_k, top_p, 2, cut.data_ptr(), st))
                e1.record()
                e1.synchronize()
                if i >= 3:
                    ts.append(1e3 * e0.elapsed_time(e1))
            print(f"  {rows:6d}   {top_k:5d}  {top_p:5.2f}   {min(ts):8.1f} / {float(np.median(ts)):8.1f}")
        del logits, lse, nodes, cut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--target-layers", type=int, default=32)
    ap.add_argument("--seed", type=int, default=2025)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    vocab = synth.BEAUTY
    V = vocab.vocab_size
    prompts, dprompts = bench.make_prompts(a.streams, 0, a.seed, "beauty", dev)
    for mask in ("position", "trie"):
        kernel_alone(bench.make_mask(vocab, mask), prompts[0], V, dev, mask)

    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=dev)
    d = HipLlama.from_synthetic(synth.llama_68m(V), a.seed + 1, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=40, **kw)
    t = HipLlama.from_synthetic(synth.llama_7b(V, a.target_layers), a.seed, std=0.02, head_std=0.02, dtype=torch.bfloat16, num_beams=20, **kw)
    for m in (t, d):
        m.generation_config.do_sample = True
        m.generation_config.temperature = 1.0
    fn = bench.make_mask(vocab, "position")

    def call(top_k, top_p):
        for m in (t, d):
            m.generation_config.top_k, m.generation_config.top_p = top_k, top_p
        n0 = lib.atspeed_warp_cutoff_launches()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        outs = BSSD_batch(t, d, dprompts, 4, 4, prefix_allowed_tokens_fn=fn, seed=a.seed)
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0)
        rounds = max(o["n_run"] for o in outs)
        acc = sum(o["total_accept_steps"] for o in outs) / max(1, sum(o["n_run"] for o in outs))
        return ms, lib.atspeed_warp_cutoff_launches() - n0, rounds, acc

    for _, k, p in SETTINGS:                                        # decoders, buffers and graphs exist before anything is timed
        call(k, p)
    print(f"# sampled BSSD_batch, {a.streams} users, Llama-7B({a.target_layers}L) bf16 target / Llama-68M draft, beams 20 / 40, gamma 4, 4 new tokens, temperature 1.0")
    print("#   rep  setting               ms per batch   cutoff launches   rounds   accepted steps per round")
    rows = {name: [] for name, _, _ in SETTINGS}
    for rep in range(a.reps):
        order = SETTINGS[rep % 3:] + SETTINGS[:rep % 3]
        for name, k, p in order:
            ms, n, rounds, acc = call(k, p)
            rows[name].append(ms)
            print(f"  {rep:4d}  {name:20s}  {ms:10.1f}   {n:8d}   {rounds:6d}   {acc:.3f}")
    for name, v in rows.items():
        print(f"# {name:20s} mean {np.mean(v):8.1f} ms  (min {min(v):.1f}, max {max(v):.1f})")


if __name__ == "__main__":
    main()
