"""Resident LoRA adapters picked per user (HipLlama.add_lora), the host side: the name -> slot bookkeeping through a stub
of the library handle, and every refusal the Python entry points make before any device work -- unknown names, wrong list lengths, the host
path -- plus the ABI records' layout.  No GPU."""
import ctypes as C
from types import SimpleNamespace

import pytest

from atspeed_amd import _lib, beamSD, synth
from atspeed_amd.generation_trie import PositionSetConstraint
from atspeed_amd.model import HipLlama

DIMS = synth.LlamaDims(synth.TINY.vocab_size, 64, 2, 4, 128)
SEP = (13, 14)


class StubLlama(HipLlama):
    """a HipLlama without a device: the two calls that reach the library hand out / take back slots as the library does (lowest free of 1 .. 16)"""

    def __init__(self):
        self.dims, self.adapters, self.adapter_info, self.lora = DIMS, {}, {}, None
        self.used, self.calls = set(), []

    def _resident_add(self, ad):
        free = [s for s in range(1, _lib.LORA_MAX_ADAPTERS + 1) if s not in self.used]
        if not free:
            raise _lib.AtSpeedError(_lib.ERR_CAPACITY, "add_lora: all 16 slots are occupied")
        self.used.add(free[0])
        self.calls.append(("add", free[0], ad.r, ad.scaling, ad.modules))
        return free[0]

    def _resident_remove(self, slot):
        self.used.remove(slot)
        self.calls.append(("remove", slot))


def _tensors(r=8, modules=("q", "v")):
    return synth.synthetic_lora(DIMS, 5, r=r, modules=modules)


def test_names_map_to_slots_and_freed_slots_are_reused():
    m = StubLlama()
    assert m.add_lora(_tensors(), "weekly", r=8, lora_alpha=16) is m
    m.add_lora(_tensors(4, ("q", "k", "v")), "segment-b", r=4, lora_alpha=8, use_rslora=True)
    assert m.adapters == {"weekly": 1, "segment-b": 2}
    assert m.calls[0] == ("add", 1, 8, 2.0, ("q", "v")) and m.calls[1][:3] == ("add", 2, 4) and abs(m.calls[1][3] - 4.0) < 1e-12
    assert m.adapter_info["segment-b"].modules == ("q", "k", "v") and m.adapter_info["weekly"].scaling == 2.0
    assert m.adapter_slot(None) == 0 and m.adapter_slot("weekly") == 1 and m.adapter_slot("segment-b") == 2
    assert m.remove_lora("weekly") is m and m.adapters == {"segment-b": 2} and "weekly" not in m.adapter_info
    m.add_lora(_tensors(), "next", r=8, lora_alpha=16)
    assert m.adapters == {"segment-b": 2, "next": 1} and m.lora is None            # load_lora's record is not touched


def test_add_and_remove_refusals_leave_the_map_as_it_was():
    m = StubLlama()
    m.add_lora(_tensors(), "a", r=8, lora_alpha=16)
    with pytest.raises(ValueError, match="resident already"):
        m.add_lora(_tensors(), "a", r=8, lora_alpha=16)
    for bad in ("", None, 3):
        with pytest.raises(ValueError, match="non-empty string"):
            m.add_lora(_tensors(), bad, r=8, lora_alpha=16)
    with pytest.raises(NotImplementedError):                                      # the loader's refusals are load_lora's: rank > 64
        m.add_lora(synth.synthetic_lora(DIMS, 2, r=65), "big", r=65, lora_alpha=16)
    with pytest.raises(KeyError, match=r"resident: \['a'\]"):
        m.remove_lora("b")
    with pytest.raises(KeyError, match="'zzz'"):
        m.adapter_slot("zzz")
    assert m.adapters == {"a": 1} and m.calls == [("add", 1, 8, 2.0, ("q", "v"))]
    for i in range(15):
        m.add_lora(_tensors(), f"n{i}", r=8, lora_alpha=16)
    with pytest.raises(_lib.AtSpeedError) as e:                                   # the library's refusal of the 17th leaves no name behind
        m.add_lora(_tensors(), "one too many", r=8, lora_alpha=16)
    assert e.value.status == _lib.ERR_CAPACITY and len(m.adapters) == 16 and "one too many" not in m.adapters


def test_adapter_slots_of_a_call():
    S = beamSD._adapter_slots
    tgt = SimpleNamespace(adapters={"a": 1, "b": 5})
    assert S(tgt, None, 1, False, "x") is None and S(tgt, None, 3, True, "x") is None
    assert S(object(), [None, None], 2, True, "x") is None                       # nobody names an adapter: the model is not even looked at
    assert S(tgt, "b", 1, False, "x") == [5]
    assert S(tgt, ["a", None, "b", "a"], 4, True, "x") == [1, 0, 5, 1]
    for bad in (["a"], ["a", "b", None], "a", []):
        with pytest.raises(ValueError, match="one name .or None. per user"):
            S(tgt, bad, 2, True, "BSSD_batch")
    with pytest.raises(KeyError, match=r"'c'.*resident: \['a', 'b'\]"):
        S(tgt, ["a", "c"], 2, True, "x")
    with pytest.raises(KeyError, match=r"resident: \[\]"):
        S(object(), "a", 1, False, "x")


class _Model:
    """enough of a HipLlama for the argument checks that come before any device work"""

    def __init__(self):
        self.adapters = {"a": 1}
        self.generation_config = SimpleNamespace(num_beams=2)
        self.max_tokens, self.device = 64, "cpu"


@pytest.fixture
def models(monkeypatch):
    monkeypatch.setattr(beamSD, "_mode", lambda seed, *models: (False, 1.0, 0, 0, 1.0))
    return _Model(), _Model()


def test_entry_points_refuse_before_any_device_work(models):
    tgt, drf = models
    inputs = {"input_ids": None}
    fn = PositionSetConstraint({0: [5], 1: [2]}, SEP)
    with pytest.raises(KeyError, match="'b'"):
        beamSD.BSSD(tgt, drf, inputs, 2, 4, prefix_allowed_tokens_fn=fn, adapter="b")
    with pytest.raises(KeyError, match="'b'"):
        beamSD.target_generate(tgt, inputs, 4, prefix_allowed_tokens_fn=fn, adapter="b")
    with pytest.raises(KeyError, match="'b'"):
        beamSD.BSSD_batch(tgt, drf, [inputs, inputs], 2, 4, prefix_allowed_tokens_fn=fn, adapters=["a", "b"])
    with pytest.raises(KeyError, match="'b'"):
        beamSD.BSSD_batch(tgt, drf, [inputs, inputs], 2, 4, prefix_allowed_tokens_fn=fn, adapters=[None, "b"], lanes=2)
    with pytest.raises(KeyError, match="'b'"):
        beamSD.target_generate_batch(tgt, [inputs, inputs], 4, prefix_allowed_tokens_fn=fn, adapters=["b", None])
    for lanes in (None, 2):
        with pytest.raises(ValueError, match="per user"):
            beamSD.BSSD_batch(tgt, drf, [inputs, inputs], 2, 4, prefix_allowed_tokens_fn=fn, adapters=["a"], lanes=lanes)
    with pytest.raises(ValueError, match="per user"):
        beamSD.target_generate_batch(tgt, [inputs, inputs], 4, prefix_allowed_tokens_fn=fn, adapters=["a", None, None])
    with pytest.raises(ValueError, match="per user"):
        beamSD.BSSD_batch(tgt, drf, [inputs, inputs], 2, 4, prefix_allowed_tokens_fn=fn, adapters="a")
    ses = beamSD.BSSDSession(tgt, drf, 2, 2, 4, prefix_allowed_tokens_fn=fn)
    with pytest.raises(KeyError, match="'b'"):
        ses.submit(inputs, adapter="b")


def test_the_host_path_refuses_an_adapter_as_it_refuses_item_filters(models):
    tgt, drf = models
    inputs = {"input_ids": None}
    fn = PositionSetConstraint({0: [5], 1: [2]}, SEP)
    with pytest.raises(NotImplementedError, match="device path only"):
        beamSD.BSSD(tgt, drf, inputs, 2, 4, prefix_allowed_tokens_fn=lambda b, s: [5], adapter="a")
    with pytest.raises(NotImplementedError, match="device path only"):
        beamSD.target_generate(tgt, inputs, 4, logits_processor=[lambda i, s: s], prefix_allowed_tokens_fn=fn, adapter="a")
    with pytest.raises(KeyError):                                                 # the name is looked up first, on either path
        beamSD.BSSD(tgt, drf, inputs, 2, 4, prefix_allowed_tokens_fn=lambda b, s: [5], adapter="b")


def test_forward_raw_batch_checks_its_adapter_list_first():
    m = StubLlama()
    m.add_lora(_tensors(), "a", r=8, lora_alpha=16)
    with pytest.raises(ValueError, match="per sequence"):
        m.forward_raw_batch([None, None], adapters=["a"])
    with pytest.raises(KeyError, match="'b'"):
        m.forward_raw_batch([None, None], adapters=["a", "b"])


def test_abi_records_have_the_headers_layout():
    """atspeed_lora_slot: four pointers, int32, float; atspeed_session_user: struct_size first, the adapter last (LP64)"""
    assert C.sizeof(_lib.LoraSlot) == 40 and _lib.LoraSlot.r16.offset == 32 and _lib.LoraSlot.scaling.offset == 36
    U = _lib.SessionUser
    assert U.struct_size.offset == 0 and U.prompt_ids_dev.offset == 8 and U.seed.offset == 24 and U.out_tokens_dev.offset == 32
    assert U.masks.offset == 56 and U.mask_user.offset == 64 and U.adapter.offset == 68 and C.sizeof(U) == 72
    assert _lib.LORA_MAX_ADAPTERS == 16
    for name in ("atspeed_llama_add_lora", "atspeed_llama_remove_lora", "atspeed_llama_lora_slots", "atspeed_llama_forward_batch_adapters",
                 "atspeed_decoder_set_adapter", "atspeed_session_submit_ex", "atspeed_segs_lora_shrink_multi", "atspeed_segs_lora_rope_kv_multi"):
        assert name in _lib.SIGNATURES
