"""`HipLlama`: the model object the beam-SD path drives, with weights resident in HBM and the
forward executed by libatspeed_hip (MFMA GEMMs, tree attention, fused norms/RoPE/SwiGLU).

It stands where the reference uses an HF `LlamaForCausalLM` (`code/inference.py:75-100`,
called at `code/beamSD.py:52,221`) and exposes the attributes the path reads from it:
`generation_config.{num_beams,do_sample}` (`beamSD.py:53,482-483`), `.dtype`, `.device`.
PyTorch is plumbing here: it owns the device memory of the weights and provides the stream.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, synth
from . import lora as _lora


def _gen_config(num_beams: int = 1) -> SimpleNamespace:
    return SimpleNamespace(num_beams=num_beams, num_return_sequences=num_beams, do_sample=False,
                           temperature=1.0, max_new_tokens=4, return_dict_in_generate=True)


def _interleave_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[2*ffn, hidden] with rows 32b..32b+15 = gate[16b..], 32b+16..32b+31 = up[16b..] (SwiGLU epilogue layout)."""
    ffn, hidden = gate.shape
    out = torch.empty(2 * ffn, hidden, dtype=gate.dtype, device=gate.device)
    v = out.view(ffn // 16, 2, 16, hidden)
    v[:, 0] = gate.view(ffn // 16, 16, hidden)
    v[:, 1] = up.view(ffn // 16, 16, hidden)
    return out


COMPUTE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _weight_tensors(packed: Dict):
    for k in ("embed", "final_norm", "lm_head"):
        yield k, packed[k]
    for l, lw in enumerate(packed["layers"]):
        for k, t in lw.items():
            yield f"layers.{l}.{k}", t


def engine_dtype_for(checkpoint_dtype: torch.dtype) -> torch.dtype:
    """The arithmetic type a checkpoint of `checkpoint_dtype` runs in: its own.  fp32 -> fp32 (exact-fp32 MFMA, the parity mode), bf16 ->
    bf16, fp16 -> fp16 -- the reference loads both models with `torch_dtype=torch.float16` (code/inference.py:75-100); the engine's fp16
    flavour (v_mfma_f32_16x16x32_f16, fp32 accumulation, the bf16 engine's kernels compiled for IEEE half) keeps every weight bit of such a
    checkpoint.  (Through round 3 an fp16 checkpoint was converted to bf16 BY VALUE: 11-bit significands rounded to 8; `dtype=torch.bfloat16`
    still asks for that.)"""
    if checkpoint_dtype in (torch.float32, torch.float64):
        return torch.float32
    if checkpoint_dtype in (torch.bfloat16, torch.float16):
        return checkpoint_dtype
    raise TypeError(f"no engine dtype for a {checkpoint_dtype} checkpoint (quantised checkpoints must be dequantised first)")


class HipLlama:
    def __init__(self, dims: synth.LlamaDims, packed: Dict, dtype: torch.dtype, device: torch.device,
                 max_slots: int = 512, max_tokens: int = 512, max_logit_rows: int = 384, num_beams: int = 1):
        if device.type != "cuda":
            raise RuntimeError("HipLlama needs a HIP device; atspeed_amd has no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in COMPUTE_DTYPES:
            # the library reads weights as ATSPEED_F32, ATSPEED_BF16 or ATSPEED_F16 bits; anything else would be silently reinterpreted
            raise TypeError(f"HipLlama computes in torch.float32, torch.bfloat16 or torch.float16, not {dtype}: convert the checkpoint "
                            "(HipLlama.from_hf / from_state_dict do, by value) instead of passing its storage dtype")
        for name, t in _weight_tensors(packed):
            if t.dtype != dtype or t.device != device:
                raise TypeError(f"HipLlama: weight {name} is {t.dtype} on {t.device}, the model was declared {dtype} on {device}")
        self.dims = dims
        self._packed = packed          # keeps the weight tensors alive
        self._dtype = dtype
        self._device = device
        self.generation_config = _gen_config(num_beams)
        self.config = SimpleNamespace(vocab_size=dims.vocab_size, hidden_size=dims.hidden, pad_token_id=0, bos_token_id=1,
                                      eos_token_id=2, use_cache=True)
        self.max_slots, self.max_tokens, self.max_logit_rows = max_slots, max_tokens, max_logit_rows
        lib = _lib.load()
        # bf16 / fp16: the projection weights and the lm_head go into the library's packed operand layout (two rows per 128-byte line and 64-byte
        # k-block: full cache lines for every LDS-DMA piece of the GEMMs); ATSPEED_PACK=0 keeps HF's row-major layout (A/B runs, slower)
        self.weights_packed = (dtype in (torch.bfloat16, torch.float16) and dims.hidden % 32 == 0 and dims.ffn % 32 == 0
                               and os.environ.get("ATSPEED_PACK", "1") != "0")
        if self.weights_packed:
            with torch.cuda.device(device):
                for lw in packed["layers"]:
                    for k in ("wqkv", "wo", "wgu", "wd"):
                        lw[k] = self._pack_rows(lw[k])
                packed["lm_head"] = self._pack_rows(packed["lm_head"])
        cfg = _lib.LlamaConfig(dims.vocab_size, dims.hidden, dims.n_layers, dims.n_heads, dims.ffn, dims.rope_theta,
                               dims.rms_eps, _lib.dtype_code(dtype),
                               max_slots, max_tokens, max_logit_rows,
                               _lib.WEIGHTS_PACKED if self.weights_packed else _lib.WEIGHTS_ROW_MAJOR)
        layers = (_lib.LlamaLayerWeights * dims.n_layers)()
        for l, lw in enumerate(packed["layers"]):
            layers[l] = _lib.LlamaLayerWeights(lw["input_norm"].data_ptr(), lw["wqkv"].data_ptr(), lw["wo"].data_ptr(),
                                               lw["post_norm"].data_ptr(), lw["wgu"].data_ptr(), lw["wd"].data_ptr())
        with torch.cuda.device(device):
            self._owner = _lib.Handle.create("atspeed_llama_destroy", lib.atspeed_llama_create, C.byref(cfg), packed["embed"].data_ptr(),
                                             packed["final_norm"].data_ptr(), packed["lm_head"].data_ptr(), layers)
        self.logits_ld = int(lib.atspeed_llama_logits_ld(self._handle))
        self.lora = None               # SimpleNamespace(r, lora_alpha, scaling, modules) while an adapter is loaded (load_lora)
        self.adapters: Dict[str, int] = {}        # resident adapters (add_lora): name -> library slot 1 .. 16
        self.adapter_info: Dict[str, SimpleNamespace] = {}   # name -> SimpleNamespace(r, lora_alpha, scaling, modules)

    @staticmethod
    def _pack_rows(t: torch.Tensor) -> torch.Tensor:
        """row-major [rows, cols] -> the packed operand layout (atspeed_pack_rows); rows rounded up to even."""
        rows, cols = t.shape
        out = torch.empty((rows + 1) // 2 * 2, cols, dtype=t.dtype, device=t.device)
        _lib.check(_lib.load().atspeed_pack_rows(t.data_ptr(), out.data_ptr(), rows, cols * t.element_size(), _lib.stream_ptr(t.device)))
        return out

    @staticmethod
    def _unpack_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
        out = torch.empty(rows, t.shape[1], dtype=t.dtype, device=t.device)
        _lib.check(_lib.load().atspeed_unpack_rows(t.data_ptr(), out.data_ptr(), rows, t.shape[1] * t.element_size(), _lib.stream_ptr(t.device)))
        return out

    # ---- attributes the reference path reads ---------------------------------------
    @property
    def dtype(self) -> torch.dtype:
        return self._dtype

    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def _handle(self) -> C.c_void_p:
        """the library's model object; `_owner` (a `_lib.Handle`) destroys it with this object"""
        return self._owner.ptr

    def eval(self):
        return self

    # ---- construction --------------------------------------------------------------
    @staticmethod
    def _pack(sd: Dict[str, torch.Tensor], dims: synth.LlamaDims) -> Dict:
        def g(name):
            return sd[name]
        layers = []
        for l in range(dims.n_layers):
            p = f"model.layers.{l}."
            layers.append(dict(
                input_norm=g(p + "input_layernorm.weight").contiguous(),
                wqkv=torch.cat((g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"),
                                g(p + "self_attn.v_proj.weight")), 0).contiguous(),
                wo=g(p + "self_attn.o_proj.weight").contiguous(),
                post_norm=g(p + "post_attention_layernorm.weight").contiguous(),
                wgu=_interleave_gate_up(g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")),
                wd=g(p + "mlp.down_proj.weight").contiguous()))
        return dict(embed=g("model.embed_tokens.weight").contiguous(), final_norm=g("model.norm.weight").contiguous(),
                    lm_head=g("lm_head.weight").contiguous(), layers=layers)

    @classmethod
    def from_state_dict(cls, dims: synth.LlamaDims, state_dict: Dict, dtype: torch.dtype = torch.float32,
                        device="cuda", **kw) -> "HipLlama":
        """HF-named tensors (numpy or torch, any float dtype: values are converted through fp32, never reinterpreted) -> device weights
        in `dtype`, which must be torch.float32, torch.bfloat16 or torch.float16."""
        device = torch.device(device)
        if dtype not in COMPUTE_DTYPES:
            raise TypeError(f"HipLlama.from_state_dict: dtype must be torch.float32, torch.bfloat16 or torch.float16, not {dtype}")
        sd = {}
        for k, v in state_dict.items():
            t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()
            sd[k] = t.to(device=device, dtype=torch.float32).to(dtype)
        return cls(dims, cls._pack(sd, dims), dtype, device, **kw)

    @classmethod
    def from_hf(cls, hf_model, dtype: Optional[torch.dtype] = None, device="cuda", **kw) -> "HipLlama":
        """Adapter for an HF `LlamaForCausalLM` (the object the reference loads, inference.py:75-100).  `dtype=None` picks the engine
        dtype from the checkpoint's (`engine_dtype_for`: fp32 -> fp32, bf16 -> bf16, fp16 -> fp16: the reference's `torch_dtype=torch.float16`
        models keep every weight bit); `dtype=torch.float32` computes an fp16 / bf16 checkpoint in fp32, `dtype=torch.bfloat16` converts an
        fp16 one by value.  Anything the kernels do not implement raises instead of approximating."""
        c = hf_model.config
        rp = getattr(c, "rope_parameters", None) or {}
        theta = getattr(c, "rope_theta", None) or (rp.get("rope_theta") if isinstance(rp, dict) else None) or 10000.0
        scaling = getattr(c, "rope_scaling", None) or rp          # transformers 4.41: None or {"type": ...}; 5.x: always a dict with rope_type
        if isinstance(scaling, dict) and (scaling.get("rope_type") or scaling.get("type") or "default") != "default":
            raise NotImplementedError(f"rope scaling {scaling} is not on this path (Llama-68M / Llama-7B use plain RoPE)")
        if getattr(c, "num_key_value_heads", None) not in (None, c.num_attention_heads):
            raise NotImplementedError("grouped-query attention is not on this path (Llama-68M / Llama-7B are MHA)")
        if getattr(c, "attention_bias", False) or getattr(c, "mlp_bias", False):
            raise NotImplementedError("projection biases are not on this path (Llama has none)")
        if getattr(c, "head_dim", None) not in (None, c.hidden_size // c.num_attention_heads):
            raise NotImplementedError("head_dim != hidden_size / num_attention_heads is not on this path")
        dims = synth.LlamaDims(c.vocab_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                               c.intermediate_size, float(theta), float(c.rms_norm_eps))
        sd = {k: v for k, v in hf_model.state_dict().items() if "rotary" not in k}
        if "lm_head.weight" not in sd:                       # tie_word_embeddings
            sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
        m = cls.from_state_dict(dims, sd, engine_dtype_for(hf_model.dtype) if dtype is None else dtype, device, **kw)
        m.generation_config.num_beams = getattr(hf_model.generation_config, "num_beams", 1)
        m.generation_config.do_sample = bool(getattr(hf_model.generation_config, "do_sample", False))
        temp = getattr(hf_model.generation_config, "temperature", None)
        m.generation_config.temperature = 1.0 if temp is None else float(temp)
        # the sampling-mode warpers `_get_logits_warper` reads: an HF config defaults to top_k = 50, top_p = 1.0 (beamSD._warpers)
        # transformers 4.41 holds these defaults in the config itself; 5.x leaves an unset field None and fills the same values in when
        # generating.  Either way None on the HF config means the default, so an unset top_k is 50: set `top_k = 0` for the temperature alone.
        for name, default in (("top_k", 50), ("top_p", 1.0)):
            v = getattr(hf_model.generation_config, name, None)
            setattr(m.generation_config, name, default if v is None else v)
        return m

    @classmethod
    def from_synthetic(cls, dims: synth.LlamaDims, seed: int, std: float = 0.02, head_std: Optional[float] = None,
                       norm_jitter: float = 0.1, dtype: torch.dtype = torch.bfloat16, device="cuda",
                       resid_scale: float = 1.0, align_to: Optional["HipLlama"] = None, round_to_bf16: bool = False,
                       round_to: Optional[torch.dtype] = None, **kw) -> "HipLlama":
        """Weights generated ON THE DEVICE by the same hash recipe as `synth.synthetic_state_dict`
        (bit-identical values), so 7B-sized models need no host generation or PCIe transfer.

        `resid_scale` / `align_to` build the high-acceptance bracket of SURVEY.md 8(d) without checkpoints: with the
        o_proj / down_proj weights scaled by `resid_scale` << 1 a model is close to its own bigram table
        head(norm(embed[tok])); `align_to=draft` copies the draft's embedding / final norm / head into the first
        `draft.hidden` coordinates of this (wider) model, so both models rank next tokens almost alike while every
        kernel still runs on dense weights of the full shapes.

        `round_to_bf16` / `round_to=torch.bfloat16 | torch.float16` (fp32 models): every weight is rounded to the nearest value of that type,
        i.e. the fp32 engine holds EXACTLY the weights of the bf16 / fp16 model of the same seed -- the judge of tests/replay.py and bench.py's
        fp32 accepted-length comparison."""
        device = torch.device(device)
        lib = _lib.load()
        head_std = std if head_std is None else head_std
        if dtype not in COMPUTE_DTYPES:
            raise TypeError(f"HipLlama.from_synthetic: dtype must be torch.float32, torch.bfloat16 or torch.float16, not {dtype}")
        code = _lib.dtype_code(dtype)
        sd: Dict[str, torch.Tensor] = {}
        with torch.cuda.device(device):
            st = _lib.stream_ptr(device)
            for name, shape, kind in synth.weight_specs(dims):
                t = torch.empty(shape, dtype=dtype, device=device)
                s = synth.tensor_seed(seed, name)
                if kind == "norm":
                    scale, add = float(synth.normal_scale(norm_jitter)), 1.0
                else:
                    w_std = synth.weight_std(name, dims, std, head_std)
                    if "o_proj" in name or "down_proj" in name:
                        w_std *= resid_scale
                    scale, add = float(synth.normal_scale(w_std)), 0.0
                _lib.check(lib.atspeed_fill_hash_normal(t.data_ptr(), t.numel(), s, scale, add, code, 0, st))
                sd[name] = t
            if align_to is not None:
                src, hd = align_to._packed, align_to.dims.hidden
                if align_to.dims.vocab_size != dims.vocab_size or hd > dims.hidden:
                    raise ValueError("align_to: same vocabulary and a hidden size <= this model's are required")
                sd["model.embed_tokens.weight"].zero_()
                sd["model.embed_tokens.weight"][:, :hd] = src["embed"]
                sd["lm_head.weight"][:, :hd] = (align_to._unpack_rows(src["lm_head"], dims.vocab_size) if align_to.weights_packed else src["lm_head"])
                # RMS over `hidden` coordinates of which `hd` carry the signal: rescale so norm(x)[:hd] matches the draft's
                sd["model.norm.weight"][:hd] = (src["final_norm"].float() * (hd / dims.hidden) ** 0.5).to(dtype)
            if round_to_bf16 and round_to is None:
                round_to = torch.bfloat16
            if round_to is not None and dtype == torch.float32:
                for t in sd.values():
                    t.copy_(t.to(round_to))
            packed = cls._pack(sd, dims)
            del sd
        return cls(dims, packed, dtype, device, **kw)

    def _enable_quant(self, fmt: str) -> "HipLlama":
        with torch.cuda.device(self._device):
            _lib.check(getattr(_lib.load(), f"atspeed_llama_enable_{fmt}")(self._handle, _lib.stream_ptr(self._device)))
        setattr(self, fmt, True)
        return self

    def _quant_counters(self, fmt: str, reset: bool) -> Dict[str, Dict[str, int]]:
        quant = (C.c_int64 * 4)()
        other = (C.c_int64 * 4)()
        _lib.check(getattr(_lib.load(), f"atspeed_llama_{fmt}_counters")(self._handle, quant, other, 1 if reset else 0))
        return {k: {fmt: int(quant[i]), "other": int(other[i])} for i, k in enumerate(self.GEMM_KINDS[:4])}

    def enable_fp8(self) -> "HipLlama":
        """fp8 (e4m3, W8A8 with per-row scales) layer projections (BASELINE config 5; the place of the reference's `load_in_8bit` target,
        code/inference.py:86-91).  bf16 and fp16 models: the e4m3 copies are made from the model's own 16-bit weight values, the activations
        between the W8A8 projections stay in the model's type (an fp16 checkpoint, the reference's, keeps the fp16 flavour)."""
        return self._enable_quant("fp8")

    def fp8_counters(self, reset: bool = False) -> Dict[str, Dict[str, int]]:
        """Launches of each layer projection that ran as fp8 / as bf16 GEMMs since the last reset (atspeed_llama_fp8_counters)."""
        return self._quant_counters("fp8", reset)

    def enable_fp4(self) -> "HipLlama":
        """4-bit target: OCP MXFP4 layer projections (e2m1 weights with one E8M0 scale per 32 k of a row) against the W8A8 activations
        (per-token e4m3), on the block-scaled MFMA (atspeed_llama_enable_fp4).  bf16 and fp16 models; the copies are made from the model's
        own 16-bit weight values.  Exclusive with enable_fp8.  Opt-in: MXFP4 without rotation or outlier handling costs model quality."""
        return self._enable_quant("fp4")

    def fp4_counters(self, reset: bool = False) -> Dict[str, Dict[str, int]]:
        """Launches of each layer projection that ran as W4A8 / as 16-bit GEMMs since the last reset (atspeed_llama_fp4_counters)."""
        return self._quant_counters("fp4", reset)

    # ---- LoRA adapter beside the base ------------------------------------------------
    def load_lora(self, adapter, r: Optional[int] = None, lora_alpha: Optional[float] = None, use_rslora: bool = False) -> "HipLlama":
        """Run this model with a LoRA adapter on q_proj / k_proj / v_proj WITHOUT merging it (peft's `result + lora_B(lora_A(x)) * scaling`,
        what the reference's `PeftModel.from_pretrained` target computes, code/inference.py:86-100): the adapter stays in the model's 16-bit
        type beside a base that may be 16-bit, W8A8 (`enable_fp8`) or W4A8 (`enable_fp4`), loaded before or after those.

        `adapter`: a peft directory (`adapter_config.json` + `adapter_model.safetensors` / `.bin`), or a dict of peft-named tensors
        (`...layers.{l}.self_attn.{q,k,v}_proj.lora_{A,B}[.default].weight`) together with `r` and `lora_alpha`.  Values are converted to the
        engine dtype through fp32.  A second adapter replaces the first.  NotImplementedError: target modules other than q / k / v,
        `use_dora`, `bias != "none"`, `modules_to_save`, rank > 64."""
        ad = _lora.read(adapter, self.dims.n_layers, self.dims.hidden, r, lora_alpha, use_rslora)
        with torch.cuda.device(self._device):
            arr, keep = self._lora_layers(ad)
            _lib.check(_lib.load().atspeed_llama_set_lora(self._handle, ad.r, ad.scaling, arr, _lib.stream_ptr(self._device)))
        del keep                       # the library holds copies of its own
        self.lora = SimpleNamespace(r=ad.r, lora_alpha=ad.lora_alpha, scaling=ad.scaling, modules=ad.modules)
        return self

    def _lora_layers(self, ad):
        """a loaded adapter's tensors on the device in the engine dtype, as the library's per-layer pointer array (+ the tensors, to keep)"""
        arr = (_lib.LoraLayer * self.dims.n_layers)()
        keep = []
        for l, lw in enumerate(ad.layers):
            for m in _lora.MODULES:
                if m in lw:
                    a, b = (t.to(self._device, torch.float32).to(self._dtype).contiguous() for t in lw[m])
                    keep += [a, b]
                    setattr(arr[l], "a_" + m, a.data_ptr())
                    setattr(arr[l], "b_" + m, b.data_ptr())
        return arr, keep

    def unload_lora(self) -> "HipLlama":
        """Remove the adapter: later forwards are bit for bit those of a model that never had one."""
        _lib.check(_lib.load().atspeed_llama_clear_lora(self._handle))
        self.lora = None
        return self

    # ---- resident adapters, picked per user -------------------------------------------
    def add_lora(self, adapter, name: str, r: Optional[int] = None, lora_alpha: Optional[float] = None, use_rslora: bool = False) -> "HipLlama":
        """Keep one more adapter RESIDENT on this model under `name` (up to 16 at once, each with its own rank and scaling): the users of
        one forward, lock-step batch or session then each run under the adapter they name -- `adapter=` / `adapters=` of BSSD, BSSD_batch,
        target_generate(_batch) and BSSDSession.submit -- or under none.  `adapter`, `r`, `lora_alpha`, `use_rslora` and the refusals are
        `load_lora`'s.  `adapters` maps name -> slot.  A duplicate name is a ValueError; a model-wide `load_lora` adapter and resident
        ones exclude each other (AtSpeedError ERR_INVALID), the 17th is AtSpeedError ERR_CAPACITY."""
        if not isinstance(name, str) or not name:
            raise ValueError(f"add_lora: the adapter's name must be a non-empty string, not {name!r}")
        if name in self.adapters:
            raise ValueError(f"add_lora: an adapter named {name!r} is resident already (slot {self.adapters[name]}): remove_lora it first")
        ad = _lora.read(adapter, self.dims.n_layers, self.dims.hidden, r, lora_alpha, use_rslora)
        self.adapters[name] = self._resident_add(ad)
        self.adapter_info[name] = SimpleNamespace(r=ad.r, lora_alpha=ad.lora_alpha, scaling=ad.scaling, modules=ad.modules)
        return self

    def remove_lora(self, name: str) -> "HipLlama":
        """Free the resident adapter `name`.  No user of a call or session in flight may name it.  With the last one gone the model runs
        bit for bit, and launch for launch, as one that never had an adapter."""
        self._resident_remove(self.adapter_slot(name))
        del self.adapters[name], self.adapter_info[name]
        return self

    def adapter_slot(self, name: Optional[str]) -> int:
        """the library slot of a resident adapter's name; None -> 0 (no adapter).  KeyError (naming the known ones) for an unknown name"""
        if name is None:
            return 0
        try:
            return self.adapters[name]
        except (KeyError, TypeError):
            raise KeyError(f"no resident adapter named {name!r} on this model (add_lora); resident: {sorted(self.adapters)}") from None

    def _resident_add(self, ad) -> int:
        slot = C.c_int32(0)
        with torch.cuda.device(self._device):
            arr, keep = self._lora_layers(ad)
            _lib.check(_lib.load().atspeed_llama_add_lora(self._handle, ad.r, ad.scaling, arr, _lib.stream_ptr(self._device), C.byref(slot)))
        del keep                       # the library holds copies of its own
        return int(slot.value)

    def _resident_remove(self, slot: int) -> None:
        _lib.check(_lib.load().atspeed_llama_remove_lora(self._handle, slot))

    def lora_launches(self, reset: bool = False) -> int:
        """Adapter kernels launched since the last reset: 2 per layer per forward with an adapter, 0 without (atspeed_llama_lora_launches)."""
        return int(_lib.load().atspeed_llama_lora_launches(self._handle, 1 if reset else 0))

    def rope_fused_launches(self, reset: bool = False) -> int:
        """qkv projections that carried RoPE + the KV scatter in their epilogue since the last reset (atspeed_llama_rope_fused_launches)."""
        return int(_lib.load().atspeed_llama_rope_fused_launches(self._handle, 1 if reset else 0))

    def sk_arena_bytes(self) -> int:
        """Bytes of the ring kernel's split-K arena this model owns: 0 until its first forward of >= 257 tokens (atspeed_llama_sk_arena_bytes)."""
        return int(_lib.load().atspeed_llama_sk_arena_bytes(self._handle))

    # ---- measurement hooks --------------------------------------------------------------
    GEMM_KINDS = ("qkv", "o_proj", "gate_up", "down", "lm_head")

    def _profile(self, fn, *args) -> Dict[str, Dict[str, float]]:
        ms = (C.c_double * 5)()
        cnt = (C.c_int64 * 5)()
        rows = (C.c_int64 * 5)()
        _lib.check(fn(self._handle, *args, ms, cnt, rows))
        return {k: dict(ms=ms[i], count=int(cnt[i]), rows=int(rows[i])) for i, k in enumerate(self.GEMM_KINDS)}

    def profile(self, enable: int = -1) -> Dict[str, Dict[str, float]]:
        """hipEvent brackets around the forward's GEMMs (see atspeed_llama_profile)."""
        return self._profile(_lib.load().atspeed_llama_profile, enable)

    def profile_big(self) -> Dict[str, Dict[str, float]]:
        """The brackets of launches with >= 1024 tokens only (one kernel: the 256x256 ring GEMM); read before `profile(0)` resets."""
        return self._profile(_lib.load().atspeed_llama_profile_big)

    def forward_log(self, enable: int = -1):
        """[(tokens, logit rows)] of the forwards run since the log was switched on (atspeed_llama_forward_log); enable as there."""
        lib = _lib.load()
        n = int(lib.atspeed_llama_forward_log(self._handle, -1, None, 0))
        buf = (C.c_int32 * max(2 * n, 2))()
        lib.atspeed_llama_forward_log(self._handle, enable, buf, n)
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]

    def gemm_shape(self, kind: str):
        """(N, K) of a GEMM kind."""
        d = self.dims
        return {"qkv": (3 * d.hidden, d.hidden), "o_proj": (d.hidden, d.hidden), "gate_up": (2 * d.ffn, d.hidden),
                "down": (d.hidden, d.ffn), "lm_head": (d.vocab_size, d.hidden)}[kind]

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """HF-named fp32 CPU tensors (undoing the qkv / gate-up packing): lets bench.py's cpu_baseline run the
        oracle on exactly the weights the device holds."""
        d, pk = self.dims, self._packed
        f = lambda t: t.detach().to("cpu", torch.float32)
        with torch.cuda.device(self._device):
            u = (lambda t, rows: self._unpack_rows(t, rows)) if self.weights_packed else (lambda t, rows: t)
            sd = {"model.embed_tokens.weight": f(pk["embed"]), "model.norm.weight": f(pk["final_norm"]),
                  "lm_head.weight": f(u(pk["lm_head"], d.vocab_size))}
            layers = [{k: (u(v, {"wqkv": 3 * d.hidden, "wo": d.hidden, "wgu": 2 * d.ffn, "wd": d.hidden}[k]) if k in ("wqkv", "wo", "wgu", "wd") else v)
                       for k, v in lw.items()} for lw in pk["layers"]] if self.weights_packed else pk["layers"]
        for l, lw in enumerate(layers):
            p = f"model.layers.{l}."
            qkv = f(lw["wqkv"])
            sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"] = \
                qkv[: d.hidden], qkv[d.hidden: 2 * d.hidden], qkv[2 * d.hidden:]
            gu = f(lw["wgu"]).view(d.ffn // 16, 2, 16, d.hidden)
            sd[p + "mlp.gate_proj.weight"] = gu[:, 0].reshape(d.ffn, d.hidden)
            sd[p + "mlp.up_proj.weight"] = gu[:, 1].reshape(d.ffn, d.hidden)
            sd[p + "self_attn.o_proj.weight"] = f(lw["wo"])
            sd[p + "mlp.down_proj.weight"] = f(lw["wd"])
            sd[p + "input_layernorm.weight"] = f(lw["input_norm"])
            sd[p + "post_attention_layernorm.weight"] = f(lw["post_norm"])
        return sd

    # ---- forward (tests / tools; the decoder calls the C entry point directly) --------
    def forward_padded(self, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, vis_bits: torch.Tensor,
                       n_slots: int, n_logit_rows: int) -> torch.Tensor:
        """The forward call (device tensors as in `forward_raw`): fp32 logits [n_logit_rows, logits_ld] of the last rows, the library's
        padded row stride kept (the row kernels of the host-mask path take `logits_ld`)."""
        T = ids.numel()
        assert vis_bits.shape == (T, self.max_slots // 64) and vis_bits.dtype == torch.int64
        with torch.cuda.device(self._device):
            raw = torch.empty(n_logit_rows * self.logits_ld, dtype=torch.float32, device=self._device)
            _lib.check(_lib.load().atspeed_llama_forward(self._handle, ids.data_ptr(), pos.data_ptr(), slots.data_ptr(),
                                                         vis_bits.data_ptr(), T, n_slots, n_logit_rows, raw.data_ptr(),
                                                         _lib.stream_ptr(self._device)))
        return raw.view(n_logit_rows, self.logits_ld)

    def forward_raw(self, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, vis_bits: torch.Tensor,
                    n_slots: int, n_logit_rows: int) -> torch.Tensor:
        """ids/pos/slots int32 [T]; vis_bits int64 [T, max_slots/64] (bit s of word s//64 = slot s visible).
        Returns fp32 logits [n_logit_rows, vocab] of the last rows."""
        return self.forward_padded(ids, pos, slots, vis_bits, n_slots, n_logit_rows)[:, : self.dims.vocab_size]

    def forward_raw_batch(self, seqs, return_all: bool = False, adapters=None):
        """Several independent sequences in ONE forward.  `seqs`: list of (ids, pos, slots, vis_bits, n_slots, n_logit_rows) with CPU
        tensors shaped as in `forward_raw`.  Returns one fp32 [n_logit_rows, vocab] view per sequence (views of one buffer), or with
        `return_all` the buffer itself, [sum of n_logit_rows, vocab], sequences one after the other.  `adapters`: one resident adapter's
        name (`add_lora`) or None per sequence."""
        n = len(seqs)
        if adapters is not None and len(adapters) != n:
            raise ValueError(f"forward_raw_batch: adapters needs one name (or None) per sequence: {len(adapters)} for {n} sequences")
        ad = np.array([self.adapter_slot(a) for a in adapters] if adapters is not None else [0] * n, dtype=np.int32)
        lib = _lib.load()
        W = self.max_slots // 64
        for ids, pos, slots, vis, _, _ in seqs:
            assert ids.dtype == pos.dtype == slots.dtype == torch.int32 and vis.dtype == torch.int64
            assert vis.shape == (ids.numel(), W)
        nt = np.array([s[0].numel() for s in seqs], dtype=np.int32)
        ns = np.array([s[4] for s in seqs], dtype=np.int32)
        nl = np.array([s[5] for s in seqs], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(nt)]).astype(np.int64)
        with torch.cuda.device(self._device):
            # one upload for all sequences: [ids | pos | slots] as int32 and the bitsets as int64
            ips = torch.cat([torch.cat([s[k] for s in seqs]) for k in range(3)]).to(self._device, non_blocking=True)
            vis = torch.cat([s[3] for s in seqs]).to(self._device, non_blocking=True)
            tot = int(off[-1])
            ptrs = lambda base, stride: (C.c_void_p * n)(*[base + int(o) * stride for o in off[:-1]])
            a_ids, a_pos, a_slot = (ptrs(ips.data_ptr() + k * tot * 4, 4) for k in range(3))
            a_vis = ptrs(vis.data_ptr(), W * 8)
            rows = int(nl.sum())
            raw = torch.empty(rows * self.logits_ld, dtype=torch.float32, device=self._device)
            _lib.check(lib.atspeed_llama_forward_batch_adapters(self._handle, n, a_ids, a_pos, a_slot, a_vis, nt.ctypes.data, ns.ctypes.data,
                                                                nl.ctypes.data, ad.ctypes.data if adapters is not None else None,
                                                                raw.data_ptr(), _lib.stream_ptr(self._device)))
        out = raw.view(rows, self.logits_ld)[:, : self.dims.vocab_size]
        if return_all:
            return out
        r0 = np.concatenate([[0], np.cumsum(nl)])
        return [out[int(r0[i]): int(r0[i + 1])] for i in range(n)]


class PromptPrefix:
    """The K / V rows of a prompt opening that many users share (`include/atspeed_hip.h` "prompt prefixes"), made once by the models' own
    forwards over `ids` and kept on the device: a user that names the prefix (`prefix=` / `prefixes=` of BSSD, BSSD_batch, target_generate(_batch)
    and BSSDSession.submit) gets the rows copied into its KV arenas and prefills only the rest of its prompt.

    `target`, `draft`: the HipLlama models the calls will be made with; `draft=None` builds the target's half alone, which serves
    target_generate(_batch) -- the beam-SD calls need both.  `adapter`: the name of the resident adapter (`target.add_lora`) the users run
    under, None = none (a model-wide `load_lora` adapter is part of the model's arithmetic and needs no name); the draft is never adapted.
    The object holds strong references to its models and owns one library handle per model.

    `stale`: the arithmetic of a model changed after the prefix was built (`enable_fp8` / `enable_fp4`, `load_lora` / `unload_lora`, or
    `remove_lora` / `add_lora` of the prefix's own slot): every call refuses it (ValueError) and a new one has to be built.  Memory per
    prefix and model: 2 x layers x length x hidden elements (`info()["bytes"]`)."""

    def __init__(self, target: "HipLlama", draft: Optional["HipLlama"], ids, adapter: Optional[str] = None):
        for m in (target,) + ((draft,) if draft is not None else ()):
            if not isinstance(m, HipLlama):
                raise TypeError("PromptPrefix: models must be atspeed_amd.HipLlama")
        if torch.is_tensor(ids):
            ids = ids.reshape(-1).tolist()
        self.ids = tuple(int(t) for t in ids)
        self.length = len(self.ids)
        if self.length < 1:
            raise ValueError("PromptPrefix: a prefix holds at least one token")
        self.target, self.draft, self.adapter = target, draft, adapter
        self.slot = target.adapter_slot(adapter)
        lib = _lib.load()
        self._owners = []
        for m, slot in ((target, self.slot), (draft, 0)):
            if m is None:
                self._owners.append(None)
                continue
            with torch.cuda.device(m.device):
                t = torch.tensor(self.ids, dtype=torch.int32, device=m.device)
                self._owners.append(_lib.Handle.create("atspeed_prefix_destroy", lib.atspeed_prefix_create, m._handle, t.data_ptr(), self.length,
                                                       slot, _lib.stream_ptr(m.device)))

    def handle(self, draft: bool = False):
        """the library object of the target's (draft's) half, None when that half was not built"""
        o = self._owners[1 if draft else 0]
        return o.ptr if o is not None else None

    def info(self, draft: bool = False) -> Dict[str, int]:
        """{length, users_served, bytes, stale} of one half (atspeed_prefix_info)"""
        n, served, nbytes = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        st = _lib.load().atspeed_prefix_info(self.handle(draft), C.byref(n), C.byref(served), C.byref(nbytes))
        if st < 0:
            _lib.check(st)
        return {"length": int(n.value), "users_served": int(served.value), "bytes": int(nbytes.value), "stale": bool(st)}

    @property
    def stale(self) -> bool:
        return any(self.info(bool(i))["stale"] for i, o in enumerate(self._owners) if o is not None)

    @property
    def users_served(self) -> int:
        return self.info()["users_served"]

    def read(self, draft: bool = False):
        """(K, V, ids) of one half as tensors: K and V [layers, length, hidden] in the model's type (atspeed_prefix_read; tests)"""
        m = self.draft if draft else self.target
        with torch.cuda.device(m.device):
            k = torch.empty(m.dims.n_layers, self.length, m.dims.hidden, dtype=m._dtype, device=m.device)
            v = torch.empty_like(k)
            ids = torch.empty(self.length, dtype=torch.int32, device=m.device)
            _lib.check(_lib.load().atspeed_prefix_read(self.handle(draft), k.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.stream_ptr(m.device)))
        return k, v, ids

    def to_batch_arenas(self, n: int, first: int = 0, draft: bool = False) -> None:
        """Copy the rows into arenas [first, first + n) of the pool `forward_raw_batch` gives its sequences (atspeed_prefix_to_batch_arenas):
        a following forward whose sequences start at position / slot `length` then sees the prefix as if it had prefilled it."""
        m = self.draft if draft else self.target
        with torch.cuda.device(m.device):
            _lib.check(_lib.load().atspeed_prefix_to_batch_arenas(self.handle(draft), int(first), int(n), _lib.stream_ptr(m.device)))

    def close(self) -> None:
        for o in self._owners:
            if o is not None:
                o.close()


def pack_vis_bits(vis: np.ndarray, max_slots: int) -> np.ndarray:
    """bool [T, S] -> int64 [T, max_slots/64]: bit s % 64 of word s // 64 = slot s visible (slots >= S are not); little-endian hosts."""
    T, S = vis.shape
    full = np.zeros((T, max_slots), bool)
    full[:, :S] = vis
    return np.packbits(full, axis=-1, bitorder="little").view(np.int64)


def vis_bits_from_bool(vis: torch.Tensor, max_slots: int) -> torch.Tensor:
    """bool [T, S] -> int64 [T, max_slots/64] bitset (host helper for tests)."""
    return torch.from_numpy(pack_vis_bits(vis.cpu().numpy(), max_slots))
