"""A create call that runs out of device memory halfway returns its error AND gives back what it had allocated until then."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from atspeed_amd import _lib
from atspeed_amd.beamSD import target_generate
from atspeed_amd.model import HipLlama
from tests.golden.cases import CASES, build_case_inputs


def test_failed_llama_create_releases_its_allocations():
    """hidden 256, one layer, 1024 tokens / logit rows, a vocabulary of 2^30: the KV cache and the first six activation buffers are a few MB
    each and fit; the logits buffer ([1280 rows][2^30] fp32 = 5.5 TB) is one request no device can hold, which the allocator refuses at once
    without committing anything.  ONE such call: the error comes back, the out pointer is untouched, the device has as much free memory as
    before, and the library goes on working.  (Before the create functions owned their half-built objects this call lost 18 874 368
    bytes of device memory: the test then fails on the memory assertion.)"""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    cfg = _lib.LlamaConfig(vocab_size=1 << 30, hidden=256, n_layers=1, n_heads=4, ffn=512, rope_theta=10000.0, rms_eps=1e-5,
                           dtype=0, max_slots=1024, max_tokens=1024, max_logit_rows=1024, weight_layout=0)
    # create only records the weight pointers (no kernel reads them before a forward): one small buffer stands for all of them
    w = torch.zeros(1024, dtype=torch.float32, device=dev)
    layers = (_lib.LlamaLayerWeights * 1)(_lib.LlamaLayerWeights(*([w.data_ptr()] * 6)))
    sentinel = 0x5A5A5A5A
    h = C.c_void_p(sentinel)
    torch.cuda.synchronize(dev)
    free_before, _ = torch.cuda.mem_get_info(dev)
    with torch.cuda.device(dev):
        rc = lib.atspeed_llama_create(C.byref(cfg), w.data_ptr(), w.data_ptr(), w.data_ptr(), layers, C.byref(h))
    msg = lib.atspeed_last_error().decode("utf-8", "replace")
    free_after, _ = torch.cuda.mem_get_info(dev)
    print(f"rc {rc}  message {msg!r}  free before {free_before}  after {free_after}  lost {free_before - free_after}")
    assert rc == _lib.ERR_HIP
    assert "hipMalloc" in msg and "failed" in msg
    assert h.value == sentinel                      # no handle, not even a half-built one
    assert free_after >= free_before                # the KV cache and the activation buffers made before the failure are back
    # and a normal model can be created and run afterwards
    ci = build_case_inputs(CASES[0])
    t = HipLlama.from_state_dict(ci["target_dims"], ci["target_sd"], torch.float32, num_beams=5, max_slots=256, max_tokens=256, max_logit_rows=128)
    out = target_generate(t, {"input_ids": torch.from_numpy(ci["prompt"])[None, :].cuda()}, 4, prefix_allowed_tokens_fn=ci["fn"])
    assert out["beam_sequence"].shape == (5, len(ci["prompt"]) + 4)
