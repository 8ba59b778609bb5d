#!/usr/bin/env python3
"""One user's qkv (N = 3 x 4096, store) and gate_up (N = 2 x 11008, SwiGLU) projections at K = 4096, Llama-7B: kernel time of the 16-bit,
W8A8 and W4A8 forms at M tokens, operands in the packed layout the engine uses (HIP events around 50 launches after 10 warm-ups).
usage: python3 tools/gemm_fp4_ab.py [M ...]   (default 60 228)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from atspeed_amd import _lib
lib = _lib.load()
st = _lib.stream_ptr(0)
K = 4096
ws = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
def timed(fn, reps=50):
    for _ in range(10): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3
for M in [int(x) for x in sys.argv[1:]] or [60, 228]:
    for name, N, epi in (("qkv", 3 * 4096, 0), ("gate_up", 2 * 11008, 3)):
        ldc = N // 2 if epi == 3 else N
        x = (torch.randn(M + (M & 1), K, device="cuda") * 0.5).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)
        xp, wp = torch.empty_like(x), torch.empty_like(w)
        lib.atspeed_pack_rows(x.data_ptr(), xp.data_ptr(), x.shape[0], 2 * K, st)
        lib.atspeed_pack_rows(w.data_ptr(), wp.data_ptr(), N, 2 * K, st)
        c = torch.empty(M + 1, N, dtype=torch.bfloat16, device="cuda")
        xq = torch.empty(x.shape[0], K, dtype=torch.uint8, device="cuda"); sx = torch.empty(x.shape[0], device="cuda")
        wq8 = torch.empty(N, K, dtype=torch.uint8, device="cuda"); sw8 = torch.empty(N, device="cuda")
        _lib.check(lib.atspeed_quant_rows_fp8_packed(xp.data_ptr(), x.shape[0], K, xq.data_ptr(), sx.data_ptr(), st))
        _lib.check(lib.atspeed_quant_rows_fp8_packed(wp.data_ptr(), N, K, wq8.data_ptr(), sw8.data_ptr(), st))
        wq4 = torch.empty(N, K // 2, dtype=torch.uint8, device="cuda"); sw4 = torch.empty(N, K // 32, dtype=torch.uint8, device="cuda")
        _lib.check(lib.atspeed_quant_weights_mxfp4(wp.data_ptr(), N, K, _lib.ATSPEED_BF16, 1, wq4.data_ptr(), sw4.data_ptr(), st))
        t16 = timed(lambda: lib.atspeed_gemm_packed(xp.data_ptr(), wp.data_ptr(), c.data_ptr(), M, N, K, ldc, epi, ws.data_ptr(), ws.numel(), st))
        t8 = timed(lambda: lib.atspeed_gemm_fp8_packed(xq.data_ptr(), sx.data_ptr(), wq8.data_ptr(), sw8.data_ptr(), c.data_ptr(), M, N, K, ldc, epi,
                                                      ws.data_ptr(), ws.numel(), st))
        t4 = timed(lambda: lib.atspeed_gemm_w4a8(xq.data_ptr(), sx.data_ptr(), wq4.data_ptr(), sw4.data_ptr(), c.data_ptr(), M, N, K, ldc, epi,
                                                 _lib.ATSPEED_BF16, 1, ws.data_ptr(), ws.numel(), st))
        wb = N * K
        print(f"{name:8s} M={M:4d}  bf16 {t16:7.1f} us ({2 * wb / t16 / 1e3:5.0f} GB/s)   W8A8 {t8:7.1f} us ({wb / t8 / 1e3:5.0f} GB/s)   "
              f"W4A8 {t4:7.1f} us ({wb * 17 / 32 / t4 / 1e3:5.0f} GB/s weights + scales)", flush=True)
