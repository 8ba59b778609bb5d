"""LoRA adapters for a `HipLlama` target, read the way peft stores them and kept OUT of the base weights.

The reference never merges: `code/inference.py:86-100` loads the base in 8 bit and wraps it with `PeftModel.from_pretrained`, whose
arguments default to rank 8, alpha 16, `['q_proj', 'v_proj']` (`code/utils.py:121-124`).  This module is the host side of that: it reads
an adapter directory (`adapter_config.json` + `adapter_model.safetensors` or `.bin`) or a dict of tensors, checks that the adapter is one
the kernels implement, and returns per-layer (A, B) pairs.  No GPU and no peft needed here; `HipLlama.load_lora` uploads the result.
"""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

MODULES = ("q", "k", "v")                      # what the engine adapts: the three projections in front of RoPE
MAX_RANK = 64                                  # ATSPEED_LORA_MAX_RANK
# ...layers.{l}.self_attn.{q,k,v}_proj.lora_{A,B}[.adapter name].weight  (peft saves without the adapter name, keeps it in memory)
_KEY = re.compile(r"(?:^|\.)layers\.(\d+)\.(?:([a-z_]+)\.)?([a-z]+)_proj\.lora_([AB])(?:\.[^.]+)?\.weight$")


@dataclass
class Adapter:
    r: int
    lora_alpha: float
    use_rslora: bool
    layers: List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]     # layers[l][module] = (A [r, hidden], B [hidden, r]) fp32 CPU tensors

    @property
    def scaling(self) -> float:
        """peft's `scaling`: alpha / r, or alpha / sqrt(r) with rslora"""
        return self.lora_alpha / math.sqrt(self.r) if self.use_rslora else self.lora_alpha / self.r

    @property
    def modules(self) -> Tuple[str, ...]:
        return tuple(m for m in MODULES if any(m in lw for lw in self.layers))


def _module_of(name: str) -> str:
    return name.split(".")[-1].replace("_proj", "")


def check_config(cfg: Mapping) -> Tuple[int, float, bool]:
    """(r, lora_alpha, use_rslora) of an `adapter_config.json`; NotImplementedError for everything the side path does not compute."""
    if str(cfg.get("peft_type", "LORA")).upper() != "LORA":
        raise NotImplementedError(f"adapter type {cfg.get('peft_type')!r}: only LoRA adapters are on this path")
    if cfg.get("use_dora"):
        raise NotImplementedError("use_dora: weight-decomposed adapters rescale the base weight, the side path only adds")
    if str(cfg.get("bias", "none")) != "none":
        raise NotImplementedError(f"bias={cfg.get('bias')!r}: adapters that train biases are not on this path (Llama projections have none)")
    if cfg.get("modules_to_save"):
        raise NotImplementedError(f"modules_to_save={cfg.get('modules_to_save')}: replaced modules would have to be merged into the checkpoint")
    if cfg.get("rank_pattern") or cfg.get("alpha_pattern"):
        raise NotImplementedError("rank_pattern / alpha_pattern: one rank and one scaling per adapter")
    tm = cfg.get("target_modules") or []
    if isinstance(tm, str):
        raise NotImplementedError(f"target_modules={tm!r}: a regular expression; list the modules (q_proj, k_proj, v_proj)")
    bad = sorted(t for t in tm if _module_of(t) not in MODULES or not t.endswith("_proj"))
    if bad:
        raise NotImplementedError(f"target modules {bad}: only q_proj / k_proj / v_proj are adapted beside the base")
    r = int(cfg["r"])
    if r > MAX_RANK:
        raise NotImplementedError(f"rank {r} > {MAX_RANK}")
    if r < 1:
        raise ValueError(f"rank {r}")
    return r, float(cfg.get("lora_alpha", r)), bool(cfg.get("use_rslora", False))


def from_tensors(tensors: Mapping, n_layers: int, hidden: int, r: int, lora_alpha: float, use_rslora: bool = False) -> Adapter:
    """peft-named tensors (torch or numpy, any float type: converted by value through fp32) -> Adapter.  Both key spellings
    (`lora_A.weight`, `lora_A.default.weight`) are accepted; keys that are no LoRA weights at all are an error, not ignored."""
    if r > MAX_RANK:
        raise NotImplementedError(f"rank {r} > {MAX_RANK}")
    if r < 1:
        raise ValueError(f"rank {r}")
    halves: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
    for key, val in tensors.items():
        mt = _KEY.search(key)
        if mt is None:
            raise NotImplementedError(f"adapter tensor {key!r} is not a lora_A / lora_B weight of a layer projection")
        l, parent, mod, ab = int(mt.group(1)), mt.group(2), mt.group(3), mt.group(4)
        if parent != "self_attn" or mod not in MODULES:
            raise NotImplementedError(f"adapter tensor {key!r}: only self_attn q_proj / k_proj / v_proj are adapted beside the base")
        if not 0 <= l < n_layers:
            raise ValueError(f"adapter tensor {key!r}: the model has {n_layers} layers")
        t = torch.from_numpy(np.ascontiguousarray(val)) if isinstance(val, np.ndarray) else val.detach()
        t = t.to("cpu", torch.float32).contiguous()
        want = (r, hidden) if ab == "A" else (hidden, r)
        if tuple(t.shape) != want:
            raise ValueError(f"adapter tensor {key!r} is {tuple(t.shape)}, expected {want} (rank {r}, hidden {hidden})")
        if halves.setdefault((l, mod), {}).setdefault(ab, t) is not t:
            raise ValueError(f"adapter tensor {key!r}: a second tensor for the same weight")
    layers: List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = [dict() for _ in range(n_layers)]
    for (l, mod), h in halves.items():
        if set(h) != {"A", "B"}:
            raise ValueError(f"layer {l} {mod}_proj: lora_{'B' if 'A' in h else 'A'} is missing")
        layers[l][mod] = (h["A"], h["B"])
    if not halves:
        raise ValueError("the adapter holds no lora_A / lora_B weights")
    return Adapter(r, float(lora_alpha), bool(use_rslora), layers)


def read_peft_dir(path: str, n_layers: int, hidden: int) -> Adapter:
    """A directory as `PeftModel.save_pretrained` writes it."""
    with open(os.path.join(path, "adapter_config.json")) as f:
        cfg = json.load(f)
    r, alpha, rs = check_config(cfg)
    st, bn = os.path.join(path, "adapter_model.safetensors"), os.path.join(path, "adapter_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        tensors = load_file(st, device="cpu")
    elif os.path.exists(bn):
        tensors = torch.load(bn, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{path}: neither adapter_model.safetensors nor adapter_model.bin")
    return from_tensors(tensors, n_layers, hidden, r, alpha, rs)


def read(adapter, n_layers: int, hidden: int, r: Optional[int] = None, lora_alpha: Optional[float] = None, use_rslora: bool = False) -> Adapter:
    """`adapter`: a peft directory (its config gives r / alpha) or a mapping of peft-named tensors with `r` and `lora_alpha` given."""
    if isinstance(adapter, Adapter):
        return adapter
    if isinstance(adapter, (str, os.PathLike)):
        if r is not None or lora_alpha is not None:
            raise ValueError("a peft directory carries its own r / lora_alpha (adapter_config.json)")
        return read_peft_dir(os.fspath(adapter), n_layers, hidden)
    if r is None or lora_alpha is None:
        raise ValueError("a dict of adapter tensors needs r and lora_alpha")
    return from_tensors(adapter, n_layers, hidden, int(r), float(lora_alpha), use_rslora)
