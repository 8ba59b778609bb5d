"""The host side of the unmerged LoRA target, without a GPU: the peft-directory loader (atspeed_amd/lora.py), its refusals, the algebra of
the reference the GPU tests compare with (tests/lora_ref.py), and the CLI flag."""
import json

import numpy as np
import pytest
import torch

from atspeed_amd import lora as L, synth
from tests import lora_ref as LR

DIMS = synth.LlamaDims(vocab_size=320, hidden=64, n_layers=2, n_heads=4, ffn=128)


def _write(tmp_path, tensors, cfg, fmt="safetensors"):
    d = tmp_path / "adapter"
    d.mkdir()
    (d / "adapter_config.json").write_text(json.dumps(cfg))
    tt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(tt, str(d / "adapter_model.safetensors"))
    else:
        torch.save(tt, str(d / "adapter_model.bin"))
    return str(d)


def _cfg(**kw):
    cfg = dict(peft_type="LORA", r=8, lora_alpha=16, target_modules=["q_proj", "v_proj"], bias="none", use_dora=False, use_rslora=False,
               modules_to_save=None, lora_dropout=0.05, task_type="CAUSAL_LM")
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
@pytest.mark.parametrize("spelling", ["plain", "default"])
def test_loader_reads_a_peft_directory(tmp_path, spelling, fmt):
    """both key spellings (peft saves `lora_A.weight`, holds `lora_A.default.weight` in memory), both file formats; the values come back
    exactly, layer by layer and module by module; scaling = alpha / r"""
    t = synth.synthetic_lora(DIMS, 5, r=8, modules=("q", "v"))
    if spelling == "default":
        t = {k.replace(".weight", ".default.weight"): v for k, v in t.items()}
    ad = L.read(_write(tmp_path, t, _cfg(), fmt), DIMS.n_layers, DIMS.hidden)
    assert (ad.r, ad.lora_alpha, ad.use_rslora, ad.scaling, ad.modules) == (8, 16.0, False, 2.0, ("q", "v"))
    for l in range(DIMS.n_layers):
        assert sorted(ad.layers[l]) == ["q", "v"]
        for m in ("q", "v"):
            p = f"base_model.model.model.layers.{l}.self_attn.{m}_proj.lora_"
            sfx = ".default.weight" if spelling == "default" else ".weight"
            a, b = ad.layers[l][m]
            assert a.shape == (8, DIMS.hidden) and b.shape == (DIMS.hidden, 8) and a.dtype == b.dtype == torch.float32
            assert np.array_equal(a.numpy(), t[p + "A" + sfx]) and np.array_equal(b.numpy(), t[p + "B" + sfx])
            assert np.abs(b.numpy()).max() > 0, "synthetic_lora's B must not be zero"


def test_loader_rslora_scaling_and_half_precision_files(tmp_path):
    """use_rslora: alpha / sqrt(r); an fp16 file is converted by value"""
    t = {k: v.astype(np.float16) for k, v in synth.synthetic_lora(DIMS, 6, r=16, modules=("k",)).items()}
    ad = L.read(_write(tmp_path, t, _cfg(r=16, lora_alpha=32, use_rslora=True, target_modules=["k_proj"])), DIMS.n_layers, DIMS.hidden)
    assert ad.scaling == 32 / 4.0 and ad.modules == ("k",)
    a = ad.layers[1]["k"][0]
    assert a.dtype == torch.float32 and np.array_equal(a.numpy(), t["base_model.model.model.layers.1.self_attn.k_proj.lora_A.weight"].astype(np.float32))


def test_loader_takes_a_dict_with_r_and_alpha():
    t = synth.synthetic_lora(DIMS, 7, r=4, modules=("q", "k", "v"))
    ad = L.read(t, DIMS.n_layers, DIMS.hidden, r=4, lora_alpha=8)
    assert ad.scaling == 2.0 and ad.modules == ("q", "k", "v")
    with pytest.raises(ValueError):
        L.read(t, DIMS.n_layers, DIMS.hidden)                     # a dict carries no config
    with pytest.raises(ValueError):
        L.read(t, DIMS.n_layers, DIMS.hidden, r=8, lora_alpha=8)  # shapes say rank 4


@pytest.mark.parametrize("change", [dict(target_modules=["q_proj", "o_proj"]), dict(target_modules=["gate_proj"]), dict(use_dora=True),
                                    dict(bias="all"), dict(bias="lora_only"), dict(modules_to_save=["lm_head"]), dict(r=65),
                                    dict(target_modules="q_proj|v_proj"), dict(rank_pattern={"q_proj": 4}), dict(peft_type="IA3")],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_config_refusals(tmp_path, change):
    """everything the side path does not compute raises NotImplementedError instead of being approximated or ignored"""
    path = _write(tmp_path, synth.synthetic_lora(DIMS, 5, r=8), _cfg(**change))
    with pytest.raises(NotImplementedError):
        L.read(path, DIMS.n_layers, DIMS.hidden)


def test_tensor_refusals():
    t = synth.synthetic_lora(DIMS, 5, r=8)
    q = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"
    with pytest.raises(NotImplementedError):                      # a module outside q / k / v in the tensors although the config did not say so
        L.from_tensors({**t, q.replace("q_proj", "o_proj"): t[q]}, DIMS.n_layers, DIMS.hidden, 8, 16)
    with pytest.raises(NotImplementedError):
        L.from_tensors({**t, "base_model.model.model.layers.0.mlp.up_proj.lora_A.weight": t[q]}, DIMS.n_layers, DIMS.hidden, 8, 16)
    with pytest.raises(NotImplementedError):                      # a saved module that is no LoRA weight
        L.from_tensors({**t, "base_model.model.lm_head.weight": t[q]}, DIMS.n_layers, DIMS.hidden, 8, 16)
    with pytest.raises(NotImplementedError):
        L.from_tensors(synth.synthetic_lora(DIMS, 5, r=65), DIMS.n_layers, DIMS.hidden, 65, 16)
    with pytest.raises(ValueError):                               # half a pair
        L.from_tensors({k: v for k, v in t.items() if k != q}, DIMS.n_layers, DIMS.hidden, 8, 16)
    with pytest.raises(ValueError):                               # a layer the model does not have
        L.from_tensors({k.replace("layers.1.", "layers.2."): v for k, v in t.items()}, DIMS.n_layers, DIMS.hidden, 8, 16)


def _inputs(T=9, S=12):
    rng = np.random.default_rng(3)
    ids = rng.integers(3, DIMS.vocab_size, T)
    vis = np.tril(np.ones((T, S), dtype=bool))
    return ids, np.arange(T), np.arange(T), vis


@pytest.mark.parametrize("modules,rslora", [(("q", "v"), False), (("q", "k", "v"), True), (("v",), False)])
def test_reference_with_adapter_equals_reference_on_merged_weights(modules, rslora):
    """the algebra: x W^T + s (x A^T) B^T == x (W + s B A)^T, in fp64 to 1e-9 of max |logit| -- and the adapter changes the logits at all"""
    sd = synth.synthetic_state_dict(DIMS, 11)
    ad = L.from_tensors(synth.synthetic_lora(DIMS, 12, r=8, modules=modules, std=0.05), DIMS.n_layers, DIMS.hidden, 8, 16, rslora)
    side = LR.LoraRefLlama(DIMS, sd, max_slots=16, dtype=torch.float64).set_lora(ad)
    merged = LR.LoraRefLlama(DIMS, sd, max_slots=16, dtype=torch.float64)
    merged.w.update({k: v for k, v in LR.merged_state_dict(sd, ad).items() if "_proj" in k})
    merged._W = lambda name: merged.w[name].to(torch.float64)              # keep the merged weights in fp64 (no fp32 rounding of the merge)
    plain = LR.LoraRefLlama(DIMS, sd, max_slots=16, dtype=torch.float64)
    a, b, c = (m.forward(*_inputs()) for m in (side, merged, plain))
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= 1e-9 * scale
    assert float((a - c).abs().max()) > 1e-3 * scale
    assert torch.equal(side.clear_lora().forward(*_inputs()), c)


def test_reference_mixin_composes_with_w8a8_and_w4a8():
    """the adapter's term is added in full precision to a quantised base projection: reference(adapter) - reference(no adapter) on one
    projection call equals scaling * (x A^T) B^T, whatever the base arithmetic"""
    d = synth.LlamaDims(vocab_size=320, hidden=256, n_layers=1, n_heads=4, ffn=256)
    sd = synth.synthetic_state_dict(d, 21, bf16=True)
    ad = L.from_tensors(synth.synthetic_lora(d, 22, r=8, modules=("q",)), d.n_layers, d.hidden, 8, 16)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((5, d.hidden)).astype(np.float32))
    a, b = ad.layers[0]["q"]
    want = 2.0 * ((x @ a.T) @ b.T)
    for make in (lambda: LR.LoraRefLlama(d, sd, max_slots=8, w8a8=True), lambda: LR.LoraRefLlamaW4A8(d, sd, max_slots=8)):
        m = make()
        name = "model.layers.0.self_attn.q_proj.weight"
        base = m._proj(x, name)
        got = m.set_lora(ad)._proj(x, name) - base
        assert torch.allclose(got, want, rtol=0, atol=1e-5 * float(base.abs().max()))
        assert torch.equal(m._proj(x, name.replace("q_proj", "k_proj")), m.clear_lora()._proj(x, name.replace("q_proj", "k_proj")))


def test_kernel_rule_restatement_is_consistent():
    """shrink_ref64 / expand_ref64: fp32 applies no rounding (the plain fp64 products), the 16-bit bounds hold at least the final rounding's half
    spacing, and a zero B leaves the base untouched"""
    rng = np.random.default_rng(2)
    h, w, a = rng.standard_normal((3, 64)), 1 + 0.1 * rng.standard_normal(64), rng.standard_normal((48, 64))
    u32, bound32, _ = LR.shrink_ref64(h, w, a, 1e-6, "fp32")
    rs = 1 / np.sqrt((h * h).mean(-1, keepdims=True) + float(np.float32(1e-6)))
    assert np.allclose(u32, (w * h * rs) @ a.T, rtol=1e-12, atol=0) and (bound32 > 0).all()
    for dt in ("bf16", "fp16"):
        u, bound, ties = LR.shrink_ref64(h, w, a, 1e-6, dt)
        assert ties <= 2
        assert (bound >= 0.5 * LR.R.ulp(u, dt)).all()
        base = LR.rnd(rng.standard_normal((3, 32)), dt)
        y, yb = LR.expand_ref64(base, LR.rnd(u[:, :16], dt), np.zeros((32, 16)), 2.0, dt)
        assert np.array_equal(y, base) and (yb >= 0.5 * LR.R.ulp(base, dt)).all()


def test_target_lora_flag_parses():
    from atspeed_amd import inference
    args = inference.parse(["--data_path", "x", "--target_lora", "/some/dir", "--target_fp8"])
    assert args.target_lora == "/some/dir" and args.target_fp8
    assert inference.parse(["--data_path", "x"]).target_lora is None
    args = inference.parse(["--data_path", "x", "--target_lora", "d", "--target_fp4"])
    assert args.target_lora == "d" and args.target_fp4


def test_synthetic_lora_is_seeded_and_named_like_peft():
    a, b = synth.synthetic_lora(DIMS, 5, r=8), synth.synthetic_lora(DIMS, 5, r=8)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert len(a) == DIMS.n_layers * 2 * 2 and all(".self_attn." in k and k.endswith(".weight") for k in a)
    c = synth.synthetic_lora(DIMS, 6, r=8)
    assert not np.array_equal(a[sorted(a)[0]], c[sorted(c)[0]])
