"""ctypes binding of libatspeed_hip.so (C-ABI: include/atspeed_hip.h).

There is no CPU fallback: if the shared library is missing, every HIP-backed entry point
raises ImportError telling the user to build it (`python -c "import __graft_entry__ as g; g.build()"`).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# ATSPEED_LIB: another build of the library (tuning builds under tools/probe); it must exist, there is no fallback
LIB_PATH = os.path.abspath(os.environ["ATSPEED_LIB"]) if os.environ.get("ATSPEED_LIB") else os.path.join(_HERE, "lib", "libatspeed_hip.so")

ATSPEED_F32, ATSPEED_BF16, ATSPEED_F16 = 0, 1, 2
WEIGHTS_ROW_MAJOR, WEIGHTS_PACKED = 0, 1
MAX_BEAMS, MAX_NEW_TOKENS, MAX_GAMMA = 64, 16, 8
LORA_MAX_RANK = 64
LORA_MAX_ADAPTERS = 16
ERR_INVALID, ERR_HIP, ERR_CAPACITY, ERR_CONSTRAINT, ERR_NO_DEVICE, ERR_FILTERED = -1, -2, -3, -4, -5, -6
EPI_STORE, EPI_F32, EPI_RESID, EPI_SWIGLU = 0, 1, 2, 3
MASK_BLOCK, MASK_ALLOW = 0, 1


class LlamaLayerWeights(C.Structure):
    _fields_ = [("input_norm", C.c_void_p), ("wqkv", C.c_void_p), ("wo", C.c_void_p),
                ("post_norm", C.c_void_p), ("wgu", C.c_void_p), ("wd", C.c_void_p)]


class LlamaConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32),
                ("ffn", C.c_int32), ("rope_theta", C.c_float), ("rms_eps", C.c_float), ("dtype", C.c_int32),
                ("max_slots", C.c_int32), ("max_tokens", C.c_int32), ("max_logit_rows", C.c_int32), ("weight_layout", C.c_int32)]


class LoraLayer(C.Structure):
    _fields_ = [("a_q", C.c_void_p), ("b_q", C.c_void_p), ("a_k", C.c_void_p), ("b_k", C.c_void_p), ("a_v", C.c_void_p), ("b_v", C.c_void_p)]


class LoraSlot(C.Structure):
    """atspeed_lora_slot: one resident adapter of one layer as the segmented adapter kernels read it"""
    _fields_ = [("a_cat", C.c_void_p), ("b_q", C.c_void_p), ("b_k", C.c_void_p), ("b_v", C.c_void_p), ("r16", C.c_int32), ("scaling", C.c_float)]


class GenStats(C.Structure):
    _fields_ = [("n_run", C.c_int32), ("total_accept_steps", C.c_int32), ("accept_steps", C.c_int32 * MAX_NEW_TOKENS),
                ("n_valid", C.c_int32), ("n_target_forwards", C.c_int32), ("n_draft_forwards", C.c_int32),
                ("draft_ms", C.c_float), ("target_ms", C.c_float), ("verify_ms", C.c_float), ("total_ms", C.c_float),
                ("status", C.c_int32), ("n_target_passes", C.c_int32)]


class SessionCounters(C.Structure):
    _fields_ = [("rounds", C.c_int64), ("target_forwards", C.c_int64), ("draft_forwards", C.c_int64), ("lane_rounds", C.c_int64),
                ("users_admitted", C.c_int64), ("users_retired", C.c_int64), ("allocs_after_create", C.c_int64),
                ("arena_reserved", C.c_int32), ("arena_failed", C.c_int32), ("n_lanes", C.c_int32), ("lanes_occupied", C.c_int32),
                ("queued", C.c_int64), ("target_passes", C.c_int64)]


class SessionDone(C.Structure):
    _fields_ = [("ticket", C.c_int64), ("lane", C.c_int32), ("status", C.c_int32), ("rounds_queued", C.c_int64),
                ("rounds_in_lane", C.c_int64)]


class SessionUser(C.Structure):
    """atspeed_session_user as it was before prompt prefixes: everything a session's user brings (atspeed_session_submit_ex).  The record is
    versioned by struct_size, so this shorter one stays valid: the library reads the members it does not have as 0"""
    _fields_ = [("struct_size", C.c_size_t), ("prompt_ids_dev", C.c_void_p), ("prompt_len", C.c_int32), ("start_node", C.c_int32),
                ("seed", C.c_uint32), ("out_tokens_dev", C.c_void_p), ("out_scores_dev", C.c_void_p), ("stats_host", C.POINTER(GenStats)),
                ("masks", C.c_void_p), ("mask_user", C.c_int32), ("adapter", C.c_int32)]


class SessionUserPrefix(C.Structure):
    """atspeed_session_user of today's header: SessionUser and the trailing prompt-prefix pair (a user that names a PromptPrefix)"""
    _fields_ = SessionUser._fields_ + [("target_prefix", C.c_void_p), ("draft_prefix", C.c_void_p)]


# every symbol include/atspeed_hip.h declares: (restype, argtypes)
_P, _I, _F, _SZ, _U32, _U64 = C.c_void_p, C.c_int32, C.c_float, C.c_size_t, C.c_uint32, C.c_uint64


class WalkArgs(C.Structure):
    """atspeed_walk_args: one verify walk as device pointers and ints (atspeed_verify_walk)"""
    _fields_ = [("struct_size", _SZ),
                ("blk_score", _P * (MAX_GAMMA + 1)), ("blk_node", _P * (MAX_GAMMA + 1)), ("blk_flat", _P * (MAX_GAMMA + 1)),
                ("blk_seq", _P * (MAX_GAMMA + 1)),
                ("nb", _I), ("dl", _I), ("k", _I), ("dk", _I), ("gen_len0", _I), ("ld", _I), ("logits", _P), ("lse", _P),
                ("blk_row0", _I * (MAX_GAMMA + 1)), ("blocks_ready", _I), ("fsm", _P), ("masks", _P), ("user", _I),
                ("vocab", _I), ("n_row_cand", _I), ("n0", _I), ("row_cand", _P),
                ("cur_ids", _P), ("cur_pos", _P), ("cur_slot", _P), ("cur_vis", _P),
                ("next_ids", _P), ("next_pos", _P), ("next_slot", _P), ("next_vis", _P),
                ("dnext_ids", _P), ("dnext_pos", _P), ("dnext_slot", _P), ("dnext_vis", _P),
                ("res_score", _P), ("res_node", _P), ("res_seq", _P), ("res_parent", _P), ("res_tok", _P), ("res_flat", _P),
                ("mailbox", _P), ("vis_words", _I), ("sample", _I), ("temperature", _F), ("seed", _U32), ("round", _I), ("pad", _I),
                ("dtab_score", _P * MAX_GAMMA), ("dtab_off", _P * MAX_GAMMA), ("dtab_lse", _P * MAX_GAMMA),
                ("cutoff", _P), ("vtrace", _P)]


# ATSPEED_SEGMENTS of the header: n, six host arrays of per-segment device pointers, three host arrays of counts
_SEGS = [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P]
SIGNATURES = {
    "atspeed_version": (C.c_char_p, []),
    "atspeed_last_error": (C.c_char_p, []),
    "atspeed_device_count": (C.c_int, []),
    "atspeed_fill_hash_normal": (C.c_int, [_P, _SZ, _U32, _F, _F, C.c_int, _U64, _P]),
    "atspeed_fsm_create": (C.c_int, [_P, _P, _P, _I, _I, _I, C.POINTER(_P)]),
    "atspeed_fsm_destroy": (None, [_P]),
    "atspeed_fsm_create_free": (C.c_int, [_I, C.POINTER(_P)]),
    "atspeed_fsm_set_id_filter": (C.c_int, [_P, _I, _I]),
    "atspeed_row_topk": (C.c_int, [_P, _I, _I, _I, _I, _P, _P]),
    "atspeed_beam_expand_prune_free": (C.c_int, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "atspeed_trie_flatten": (C.c_int, [_P, _P, _I, _P, _P, _P, C.POINTER(_I), C.POINTER(_I)]),
    "atspeed_llama_create": (C.c_int, [C.POINTER(LlamaConfig), _P, _P, _P, C.POINTER(LlamaLayerWeights), C.POINTER(_P)]),
    "atspeed_llama_destroy": (None, [_P]),
    "atspeed_llama_forward": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "atspeed_llama_forward_batch": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "atspeed_llama_logits": (_P, [_P]),
    "atspeed_llama_read": (C.c_int, [_P, _I, _I, _P, _SZ, _P]),
    "atspeed_probe_mfma_bf16": (C.c_int, [_I, _P, C.c_size_t, _P, _P]),
    "atspeed_probe_hbm_read": (C.c_int, [_P, C.c_size_t, _I, _P, _P, _P]),
    "atspeed_llama_enable_fp8": (C.c_int, [_P, _P]),
    "atspeed_llama_fp8_counters": (C.c_int, [_P, _P, _P, _I]),
    "atspeed_llama_enable_fp4": (C.c_int, [_P, _P]),
    "atspeed_llama_fp4_counters": (C.c_int, [_P, _P, _P, _I]),
    "atspeed_quant_weights_mxfp4": (C.c_int, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "atspeed_gemm_w4a8": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "atspeed_llama_rope_fused_launches": (C.c_int64, [_P, _I]),
    "atspeed_llama_sk_arena_bytes": (C.c_int64, [_P]),
    "atspeed_llama_set_lora": (C.c_int, [_P, _I, _F, C.POINTER(LoraLayer), _P]),
    "atspeed_llama_clear_lora": (C.c_int, [_P]),
    "atspeed_llama_lora_launches": (C.c_int64, [_P, _I]),
    "atspeed_lora_shrink": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _F, _I, _P]),
    "atspeed_segs_lora_rope_kv": (C.c_int, [_P, _P, _P, _P, _P, _I, _F, _P, _P, _SZ, _I, _I, _I, _I] + _SEGS + [_P]),
    "atspeed_llama_add_lora": (C.c_int, [_P, _I, _F, C.POINTER(LoraLayer), _P, C.POINTER(_I)]),
    "atspeed_llama_remove_lora": (C.c_int, [_P, _I]),
    "atspeed_llama_lora_slots": (_I, [_P]),
    "atspeed_llama_forward_batch_adapters": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "atspeed_decoder_set_adapter": (C.c_int, [_P, _I]),
    "atspeed_session_submit_ex": (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),      # SessionUser or SessionUserPrefix, by reference
    "atspeed_segs_lora_shrink_multi": (C.c_int, [_P, _P, C.POINTER(LoraSlot), _I, _P, _I, _F, _I, _P] + _SEGS + [_P]),
    "atspeed_segs_lora_rope_kv_multi": (C.c_int, [_P, _P, C.POINTER(LoraSlot), _I, _P, _P, _SZ, _I, _I, _I, _I, _P] + _SEGS + [_P]),
    "atspeed_quant_rows_fp8": (C.c_int, [_P, _I, _I, _P, _P, _P]),
    "atspeed_quant_rows_fp8_packed": (C.c_int, [_P, _I, _I, _P, _P, _P]),
    "atspeed_gemm_fp8": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "atspeed_llama_profile": (C.c_int, [_P, _I, _P, _P, _P]),
    "atspeed_llama_profile_big": (C.c_int, [_P, _P, _P, _P]),
    "atspeed_llama_forward_log": (C.c_int32, [_P, _I, _P, _I]),
    "atspeed_llama_logits_ld": (_I, [_P]),
    "atspeed_lse_rows": (C.c_int, [_P, _I, _I, _I, _P, _P]),
    "atspeed_log_softmax_rows": (C.c_int, [_P, _I, _P, _I, _I, _P, _I, _P]),
    "atspeed_lmhead_lse": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _SZ, C.POINTER(_I), _P]),
    "atspeed_beam_expand_prune": (C.c_int, [_P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "atspeed_accept": (C.c_int, [_P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "atspeed_decoder_create": (C.c_int, [_P, _P, _I, C.POINTER(_P)]),
    "atspeed_decoder_destroy": (None, [_P]),
    "atspeed_decoder_set_sampling": (C.c_int, [_P, _I, _F, C.c_uint32]),
    "atspeed_decoder_set_warpers": (C.c_int, [_P, _I, _F, _I]),
    "atspeed_warp_cutoffs": (C.c_int, [_P, _I, _P, _I, _P, _P, _F, _I, _F, _I, _P, _P]),
    "atspeed_warp_cutoff_launches": (C.c_int64, []),
    "atspeed_bssd_generate": (C.c_int, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, C.POINTER(GenStats), _P]),
    "atspeed_bssd_generate_batch": (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "atspeed_session_create": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _P, C.POINTER(_P)]),
    "atspeed_session_submit": (C.c_int, [_P, _P, _I, _I, _U32, _P, _P, C.POINTER(GenStats), C.POINTER(C.c_int64)]),
    "atspeed_session_round": (C.c_int, [_P, C.POINTER(SessionDone), _I, C.POINTER(_I)]),
    "atspeed_session_drain": (C.c_int, [_P, C.POINTER(SessionDone), _I, C.POINTER(_I)]),
    "atspeed_session_get_counters": (C.c_int, [_P, C.POINTER(SessionCounters)]),
    "atspeed_session_destroy": (None, [_P]),
    "atspeed_node_masks_create": (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P, C.POINTER(_P)]),
    "atspeed_node_masks_destroy": (None, [_P]),
    "atspeed_node_masks_read": (C.c_int, [_P, _I, _P, _I]),
    "atspeed_decoder_set_node_mask": (C.c_int, [_P, _P, _I]),
    "atspeed_session_submit_masked": (C.c_int, [_P, _P, _I, _I, _U32, _P, _P, C.POINTER(GenStats), _P, _I, C.POINTER(C.c_int64)]),
    "atspeed_beam_expand_prune_masked": (C.c_int, [_P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "atspeed_warp_cutoffs_masked": (C.c_int, [_P, _I, _P, _I, _P, _P, _F, _I, _F, _I, _P, _P, _I, _P]),
    "atspeed_beam_sample_step": (C.c_int, [_P, _I, _P, _P, _P, _I, _P, _P, _I, _I, _F, _U32, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "atspeed_verify_walk": (C.c_int, [C.POINTER(WalkArgs), _P]),
    "atspeed_score_items": (C.c_int, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "atspeed_score_tree_build": (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "atspeed_path_scores": (C.c_int, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P]),
    "atspeed_target_generate": (C.c_int, [_P, _P, _I, _P, _I, _I, _I, _P, _P, C.POINTER(GenStats), _P]),
    "atspeed_target_generate_batch": (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "atspeed_assemble_sequences": (C.c_int, [_P, _P, _P, _I, _I, _I, _P, _P]),
    "atspeed_decoder_trace": (C.c_int, [_P, _P, _I]),
    "atspeed_decoder_set_trace": (C.c_int, [_P, _I]),
    "atspeed_decoder_decisions": (C.c_int64, [_P, _P, C.c_int64]),
    "atspeed_decoder_kv_bytes": (C.c_int64, [_P, _I]),
    "atspeed_decoder_kv_copy": (C.c_int, [_P, _I, _I, _P, _P, _P]),
    "atspeed_prefix_create": (C.c_int, [_P, _P, _I, _I, _P, C.POINTER(_P)]),
    "atspeed_prefix_destroy": (None, [_P]),
    "atspeed_prefix_info": (C.c_int, [_P, C.POINTER(_I), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "atspeed_prefix_read": (C.c_int, [_P, _P, _P, _P, _P]),
    "atspeed_decoder_set_prefix": (C.c_int, [_P, _P, _P]),
    "atspeed_prefix_to_batch_arenas": (C.c_int, [_P, _I, _I, _P]),
    "atspeed_kv_rows_scatter": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "atspeed_kv_rows_gather": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "atspeed_gemm": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "atspeed_gemm_path_counters": (C.c_int, [_P, _I, _I]),
    "atspeed_set_switch": (C.c_int, [C.c_char_p, _I]),
    "atspeed_get_switch": (C.c_int, [C.c_char_p, C.POINTER(_I)]),
    "atspeed_gemm_packed": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "atspeed_gemm_fp8_packed": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "atspeed_pack_rows": (C.c_int, [_P, _P, _I, _I, _P]),
    "atspeed_unpack_rows": (C.c_int, [_P, _P, _I, _I, _P]),
    "atspeed_rmsnorm": (C.c_int, [_P, _P, _P, _I, _I, _F, _I, _P]),
    "atspeed_rmsnorm_quant_fp8": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _F, _P]),
    "atspeed_tree_attention": (C.c_int, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "atspeed_tree_attention_tiled": (C.c_int, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "atspeed_segs_embed": (C.c_int, [_P, _I, _I, _I, _P] + _SEGS + [_P]),
    "atspeed_segs_gather_logit_rows": (C.c_int, [_P, _I, _I, _P] + _SEGS + [_P]),
    "atspeed_segs_gather_tail_rows": (C.c_int, [_P, _P, _I, _I, _I, _P, _P] + _SEGS + [_P]),
    "atspeed_segs_row_info": (C.c_int, [_P, _I] + _SEGS + [_P]),
    "atspeed_segs_rope_kv": (C.c_int, [_P, _P, _I, _P, _P, _SZ, _I, _I, _I, _I] + _SEGS + [_P]),
    "atspeed_segs_tree_attention": (C.c_int, [_P, _I, _SZ, _I, _P, _I, _I, _I, _I, _I, _I, _I] + _SEGS + [_P]),
    "atspeed_gemm_resid_norm": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _F, _P, _SZ, _I, _P]),
    "atspeed_gemm_fp8_resid_norm": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _F, _P, _SZ, _I, _P]),
    "atspeed_gemm_w4a8_resid_norm": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _F, _P, _SZ, _I, _P]),
}

_lib: Optional[C.CDLL] = None


class AtSpeedError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"[atspeed_hip status {status}] {message}")
        self.status = status
        self.message = message


def load() -> C.CDLL:
    """Load the HIP library (after torch, so both share one libamdhip64)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `make -C atspeed_amd/csrc` (or `__graft_entry__.build()`); atspeed_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  -- pulls in torch's libamdhip64.so.7 first so the SONAME resolves to it
    except Exception:  # pragma: no cover - torch is plumbing; the library also loads against /opt/rocm
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> None:
    if status == 0:
        return
    msg = load().atspeed_last_error().decode("utf-8", "replace")
    if status == ERR_CONSTRAINT:
        raise ValueError(msg)          # what HF's PrefixConstrainedLogitsProcessor raises
    raise AtSpeedError(status, msg)


class Handle:
    """Owner of one library object: its `c_void_p` (`ptr`) and the name of the function that destroys it.  `close()`, leaving a `with` block
    and collection all destroy it, at most once between them; at interpreter shutdown, when the library may be gone already, errors are
    swallowed."""

    def __init__(self, destroy: str):
        self.ptr, self._destroy = C.c_void_p(), destroy

    @classmethod
    def create(cls, destroy: str, create_fn, *args) -> "Handle":
        """`create_fn(*args, &ptr)`: every create function of the library takes its out pointer last."""
        h = cls(destroy)
        check(create_fn(*args, C.byref(h.ptr)))
        return h

    def close(self) -> None:
        ptr, self.ptr = self.ptr, None
        if ptr:
            try:
                getattr(load(), self._destroy)(ptr)
            except Exception:
                pass

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class switches:
    """`with _lib.switches(gemm_sk=2, gemm_panel=0): ...` -- set process-wide library switches (atspeed_set_switch) and restore them on exit.
    The environment variables (ATSPEED_GEMM_SK, ...) only give the INITIAL values, read once by the library; tests and sweeps that compare
    two settings in one process go through here.  Every name is read before any is set, so an unknown name changes nothing."""

    def __init__(self, **values: int):
        self.values = values
        self.old = {}

    def __enter__(self):
        lib = load()
        cur = _I(0)
        for name in self.values:
            check(lib.atspeed_get_switch(name.encode(), C.byref(cur)))
            self.old[name] = cur.value
        try:
            for name, v in self.values.items():
                check(lib.atspeed_set_switch(name.encode(), int(v)))
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        lib = load()
        failed = [st for st in [lib.atspeed_set_switch(name.encode(), v) for name, v in self.old.items()] if st != 0]
        if failed:                  # every name has been tried by now: a failure leaves no other switch unrestored
            check(failed[0])
        return False


def dtype_code(dtype) -> int:
    """torch dtype -> the library's atspeed_dtype code (fp32 parity mode, bf16, fp16)."""
    import torch
    try:
        return {torch.float32: ATSPEED_F32, torch.bfloat16: ATSPEED_BF16, torch.float16: ATSPEED_F16}[dtype]
    except KeyError:
        raise TypeError(f"libatspeed_hip computes in torch.float32, torch.bfloat16 or torch.float16, not {dtype}") from None


def stream_ptr(device=None) -> int:
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)
