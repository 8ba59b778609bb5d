#!/usr/bin/env python3
"""What a per-user item filter costs (profiles/item_filter_cost.txt).

  python3 tools/item_filter_cost.py [--batch 256] [--history 20] [--reps 3] [--layers 32] [--kernels_only]
      BASELINE config 3's strict-trie batch -- Games (17 332 items), Llama-68M / Llama-7B dims, K = 20 / DK = 40, random-init bf16 weights,
      `--batch` users in one lock-step BSSD_batch -- once unfiltered and once with `--history` seeded items excluded per user:
      items/s, the draft / verify stage times the library reports (the step and verify kernels run inside them), the builder's time for the
      whole batch (one atspeed_node_masks_create call with its host marshalling), and the step kernel alone (atspeed_beam_expand_prune_masked,
      40 rows at first-level nodes of the Games trie) with and without a filter.
The unfiltered headline (bench.py --gpus 1 --steps 2 --warmup 1) against the parent commit is measured with bench.py itself.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from atspeed_amd import _lib, synth
from atspeed_amd.beamSD import BSSD_batch, _DeviceFSM, _item_filters, _filter_specs
from atspeed_amd.generation_trie import SuffixTrieConstraint, Trie
from atspeed_amd.model import HipLlama

DEV = torch.device("cuda", 0)
GV = synth.GAMES


def _prompts(n):
    plens = synth.prompt_lengths(n, 2025, mean_hist=5.98)
    return [{"input_ids": torch.from_numpy(synth.synthetic_prompt(int(plens[u]), synth.tensor_seed(2025, f"user{u}")))[None].to(DEV)} for u in range(n)]


def _batch(tgt, drf, prompts, fn, reps, **kw):
    BSSD_batch(tgt, drf, prompts, 4, 4, prefix_allowed_tokens_fn=fn, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        outs = BSSD_batch(tgt, drf, prompts, 4, 4, prefix_allowed_tokens_fn=fn, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    return dt, sum(o["draft_time_cost"] for o in outs), sum(o["target_time_cost"] for o in outs), sum(o["verify_time_cost"] for o in outs), outs


def _step_alone(fsm, dfsm, masks, n_rows=40, k=40, reps=50):
    """the step kernel by itself: n_rows beams at first-level nodes (about 70 children each), microseconds per launch"""
    lib = _lib.load()
    V = GV.vocab_size
    ld = (V + 3) // 4 * 4                                   # the LSE kernel reads 16-byte groups: rows 16-byte aligned
    g = torch.Generator().manual_seed(1)
    lg = torch.randn(n_rows, ld, generator=g).to(DEV)
    lse = torch.empty(n_rows, dtype=torch.float32, device=DEV)
    first = fsm.nxt[fsm.row_ptr[fsm.start]: fsm.row_ptr[fsm.start + 1]]
    nd = torch.from_numpy(np.ascontiguousarray(first[:n_rows], np.int32)).to(DEV)
    bs = torch.zeros(n_rows, dtype=torch.float32, device=DEV)
    o_s = torch.empty(64, dtype=torch.float32, device=DEV)
    o = [torch.empty(64, dtype=torch.int32, device=DEV) for _ in range(4)]
    st = _lib.stream_ptr(DEV)
    _lib.check(lib.atspeed_lse_rows(lg.data_ptr(), n_rows, V, ld, lse.data_ptr(), st))

    def launch():
        _lib.check(lib.atspeed_beam_expand_prune_masked(lg.data_ptr(), ld, lse.data_ptr(), bs.data_ptr(), nd.data_ptr(), n_rows, dfsm.handle, k, o_s.data_ptr(),
                                                        o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), masks, 0, st))
    for _ in range(5):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main(a):
    kw = dict(max_slots=512, max_tokens=512, max_logit_rows=384, device=DEV)
    items = synth.synthetic_items(GV)
    fn = SuffixTrieConstraint(Trie([[1] + [int(t) for t in it] + [2] for it in items]), synth.RESPONSE_SEP, 1)
    prompts = _prompts(a.batch)
    rng = np.random.default_rng(7)
    excl = [[[int(t) for t in items[i]] for i in rng.choice(len(items), size=a.history, replace=False)] for _ in range(a.batch)]
    print(f"# Games V={GV.vocab_size}, {len(items)} items, Llama-68M / Llama-7B({a.layers}L) bf16 random init, K=20 DK=40, {a.batch} users per lock-step batch, "
          f"{a.history} items excluded per user, {a.reps} timed batches after one warm-up")
    if not a.kernels_only:
        drf = HipLlama.from_synthetic(synth.llama_68m(GV.vocab_size), 2026, dtype=torch.bfloat16, num_beams=40, **kw)
        tgt = HipLlama.from_synthetic(synth.llama_7b(GV.vocab_size, a.layers), 2025, dtype=torch.bfloat16, num_beams=20, **kw)
    for tag, kwargs in (() if a.kernels_only else (("unfiltered", {}), ("filtered", dict(exclude_items=excl)), ("unfiltered again", {}))):
        dt, d_s, t_s, v_s, outs = _batch(tgt, drf, prompts, fn, a.reps, **kwargs)
        print(f"MARK {tag}: {1e3 * dt:.1f} ms per batch, {a.batch * 20 / dt:.1f} items/s; stage times summed over users: draft {1e3 * d_s:.1f} ms "
              f"(forwards + step kernels), target {1e3 * t_s:.1f} ms, verify {1e3 * v_s:.1f} ms (verify kernels)", flush=True)
    # the builder alone: one create call for the whole batch
    fsms = [fn.compile(p["input_ids"][0].tolist()) for p in prompts]
    dfsm = _DeviceFSM.get(fsms[0], GV.vocab_size)
    specs = _filter_specs(a.batch, excl, None, True, "cost")
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        owners, per_user = _item_filters(dfsm, [f.start for f in fsms], specs, DEV, "cost")
        t_all = time.perf_counter() - t0
    print(f"MARK builder: {a.batch} users x {a.history} sequences, {fsms[0].n_nodes} nodes: {1e3 * t_all:.2f} ms for the create call with its host "
          f"marshalling, copies, the kernel and the synchronisation", flush=True)
    us_plain = _step_alone(fsms[0], dfsm, None)
    us_mask = _step_alone(fsms[0], dfsm, per_user[0][0])
    print(f"MARK step kernel alone, 40 rows at first-level nodes, k=40: {us_plain:.1f} us unfiltered, {us_mask:.1f} us filtered", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--history", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--kernels_only", action="store_true", help="the builder and the step kernel alone: no models, no batches")
    main(ap.parse_args())
