"""ctypes binding of the C-ABI device backend (``include/nano_mi355x.h``) and of the host C engine
(``include/nano_infer_abi.h``).

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950) into
``nano_amd/lib/libnano_mi355x.so``.  There is no Python or CPU fallback: if the library is missing,
or no gfx950 device is visible when a model is created, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NANO_LIB") or os.path.join(HERE, "lib", "libnano_mi355x.so")     # NANO_LIB: a measurement build (libnano_mi355x_stamps.so)

f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
i8p = np.ctypeslib.ndpointer(dtype=np.int8, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")


class NanoModelDesc(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "arch", "block_size", "vocab_size", "n_layer", "n_embd", "n_head", "n_kv_head", "n_hidden",
        "is_shared_classifier", "head_dim", "quant_type", "group_size")]


class NanoFusedGemvDesc(C.Structure):
    """include/nano_mi355x.h NanoFusedGemvDesc: one fused decode GEMV launch as a step issues it."""
    _fields_ = [("quant", C.c_uint32), ("gs", C.c_uint32), ("kind", C.c_uint32), ("n", C.c_uint32), ("nb", C.c_uint32), ("nseg", C.c_uint32),
                ("rows", C.c_uint32 * 3), ("w", C.c_void_p * 3), ("ws", C.c_void_p * 3), ("x", C.c_void_p), ("norm_w", C.c_void_p),
                ("attn_part", C.c_void_p), ("attn_ml", C.c_void_p), ("attn_nsplit", C.c_uint32), ("attn_n_head", C.c_uint32),
                ("attn_hd", C.c_uint32), ("use_gemm", C.c_uint32), ("ordered", C.c_uint32), ("route_out", C.c_void_p), ("out", C.c_void_p),
                ("out_slots", C.c_uint32), ("out_stride", C.c_uint32), ("tile_max", C.c_void_p), ("tile_slots", C.c_uint32),
                ("tile_pairs", C.c_uint32), ("ntiles_out", C.c_void_p), ("argmax_out", C.c_void_p), ("resid_add", C.c_void_p),
                ("resid_add_stride", C.c_uint32)]


class NanoLoraOpDesc(C.Structure):
    """include/nano_mi355x.h NanoLoraOpDesc: one LoRA side-branch launch (q | k | v, or o) as a step issues it."""
    _fields_ = [(n, C.c_uint32) for n in ("E", "KD", "rank", "alpha", "nb", "S", "v_bstride", "_pad")] + \
               [("x", C.c_void_p), ("norm_w", C.c_void_p), ("a", C.c_void_p * 3), ("b", C.c_void_p * 3), ("pos", C.c_void_p),
                ("q", C.c_void_p), ("kraw", C.c_void_p), ("v", C.c_void_p), ("q_floats", C.c_uint64), ("k_floats", C.c_uint64), ("v_floats", C.c_uint64)]


NANO_LORA_TABLE_MAX = 64
NANO_LORA_NONE = 0xffffffff


class NanoLoraAdapter(C.Structure):
    """include/nano_mi355x.h NanoLoraAdapter: one adapter of a per-row LoRA launch."""
    _fields_ = [("rank", C.c_uint32), ("alpha", C.c_uint32), ("a", C.c_void_p * 3), ("b", C.c_void_p * 3)]


class NanoLoraRowsOpDesc(C.Structure):
    """include/nano_mi355x.h NanoLoraRowsOpDesc: one per-row LoRA side-branch launch (q | k | v, or o) as a step with a LoRA table issues it."""
    _fields_ = [(n, C.c_uint32) for n in ("E", "KD", "nb", "S", "v_bstride", "n_adapters")] + \
               [("x", C.c_void_p), ("norm_w", C.c_void_p), ("adapters", C.POINTER(NanoLoraAdapter)), ("row_adapter", C.c_void_p), ("pos", C.c_void_p),
                ("q", C.c_void_p), ("kraw", C.c_void_p), ("v", C.c_void_p), ("q_floats", C.c_uint64), ("k_floats", C.c_uint64), ("v_floats", C.c_uint64)]


class NanoAttnDecodeDesc(C.Structure):
    """include/nano_mi355x.h NanoAttnDecodeDesc: one decode attention launch (or a prefill chunk's two passes) as a step issues it."""
    _fields_ = [(n, C.c_uint32) for n in ("nb", "n_head", "n_kv_head", "hd", "n_layer", "layer", "S", "range_hint", "nsplit", "rope_qwen3",
                                          "kv_half", "chunk", "want_frag", "pool_rows", "pt_stride")] + \
               [(n, C.c_void_p) for n in ("q", "k", "vraw", "pos", "q_norm", "k_norm", "rope_cos", "rope_sin", "pt_rows", "k_cache", "v_cache",
                                          "out", "xf", "xsf", "plan")]


class NanoQkvAttnFusedDesc(C.Structure):
    """include/nano_mi355x.h NanoQkvAttnFusedDesc: one fused q | k | v + attention launch as a step issues it."""
    _fields_ = [("qkv", C.POINTER(NanoFusedGemvDesc)), ("attn", C.POINTER(NanoAttnDecodeDesc)), ("layer1", C.c_uint32), ("tick0", C.c_uint32),
                ("hand_init", C.c_void_p), ("part_out", C.c_void_p), ("ml_out", C.c_void_p), ("plan_out", C.c_void_p), ("err_out", C.c_void_p)]


class NanoWoW13FusedDesc(C.Structure):
    """include/nano_mi355x.h NanoWoW13FusedDesc: one fused Wo + W1|W3 launch as a step issues it."""
    _fields_ = [("wo", C.POINTER(NanoFusedGemvDesc)), ("w13", C.POINTER(NanoFusedGemvDesc)), ("layer1", C.c_uint32), ("tick0", C.c_uint32),
                ("hand_init", C.c_void_p), ("plan_out", C.c_void_p), ("err_out", C.c_void_p)]


class NanoExactAttnDesc(C.Structure):
    """include/nano_mi355x.h NanoExactAttnDesc: exact mode's attention of one sequence and one layer."""
    _fields_ = [(n, C.c_uint32) for n in ("n_head", "n_kv_head", "hd", "S", "range", "is_causal", "long_form", "_pad")] + \
               [(n, C.c_void_p) for n in ("q", "k_cache", "v_cache", "out")]


# the fields of an attention plan (nano_amd/csrc/kernels.h AttnPlan; xcd: workgroups of a KV head on one XCD)
ATTN_PLAN_FIELDS = ("mode", "lpr", "qv", "kvm", "npt", "w16", "paged", "kv_half", "nsplit", "xcd")


# what nano_hip_f32_gemv_plan reports (nano_amd/csrc/kernels.h F32GemvPlan + route_gemv_slices), and the kernel roles of gemv_common.h
F32_PLAN_FIELDS = ("role", "B", "nv", "upw", "rw", "nw", "grid", "lds_bytes", "launches", "seqs_per_launch", "takes")
F32_PLAN_WORDS = len(F32_PLAN_FIELDS) + 1         # NANO_F32_GEMV_PLAN_WORDS: a last word that is always 0
F32_ROLES = ("generic", "norm_store", "resid", "resid_combine", "norm_swiglu")


# what nano_hip_f32_gemm_plan reports (route_kind + nano_amd/csrc/kernels.h F32GemmPlan, field for field): route is an index into ROUTE_NAMES
F32_GEMM_PLAN_FIELDS = ("route", "sw", "threads", "grid", "lds_bytes", "rt", "nw", "nt", "nu", "upw", "tp", "stage_bytes", "tab_off",
                        "pro_threads", "pro_lds", "xs_floats", "takes")


# what nano_hip_q80_gemv_plan reports (nano_amd/csrc/kernels.h Q80GemvPlan + route_kind + route_gemv_slices): route is an index into
# ROUTE_NAMES, kernel into Q80_KERNELS, role into Q80_ROLES, variant into Q80_VARIANTS
Q80_PLAN_FIELDS = ("route", "kernel", "role", "gs", "B", "nv", "upw", "rw", "nw", "grid", "lds_bytes", "variant", "pre", "launches",
                   "seqs_per_launch", "takes")
Q80_PLAN_WORDS = len(Q80_PLAN_FIELDS) + 1         # NANO_Q80_GEMV_PLAN_WORDS: a last word behind takes, the plan's cw (q80_gemv_plan_cw)
Q80_ROLES = F32_ROLES
Q80_KERNELS = ("none", "slab", "stream")
Q80_VARIANTS = ("plain", "early", "wf", "wfc2", "wfc3", "wfc4")


# what nano_hip_q80_gemm_plan reports (route_kind + nano_amd/csrc/kernels.h Q80GemmPlan, field for field): route is an index into ROUTE_NAMES,
# kernel into Q80_GEMM_KERNELS
Q80_GEMM_PLAN_FIELDS = ("route", "kernel", "tt", "nv", "r", "ms", "tp", "pp", "gs", "sw", "threads", "grid", "lds_bytes", "norm_order",
                        "hh", "ntiles", "tc0", "tc1", "tpw", "full", "nu", "nk", "ttl", "nw", "rounds", "tts", "magic",
                        "nsa", "pre", "a_stage", "a_ws", "b_base", "b_stage", "b_xs", "ks", "ncw", "nss", "tab", "ring", "nl",
                        "waves", "lt", "nhc", "nwaves", "ng", "npass", "takes")
Q80_GEMM_KERNELS = ("none", "g6s", "g6f", "g7", "g7k", "gc", "g2")


# what nano_hip_q4k_gemv_plan reports (nano_amd/csrc/kernels.h Q4kGemvPlan + route_kind + route_gemv_slices): route is an index into
# ROUTE_NAMES, kernel into Q4K_KERNELS, role into Q80_ROLES
Q4K_PLAN_FIELDS = ("route", "kernel", "role", "B", "nv", "ipt", "d", "loop", "rounds", "wg0", "wg1", "wg2", "rw", "nthr", "grid", "lds_bytes",
                   "pre", "quant_rows", "quant_nthr", "quant_nv", "partials", "launches", "seqs_per_launch", "takes")
Q4K_KERNELS = ("none", "slab", "chunk")


# what nano_hip_qkv_attn_fused_plan / nano_hip_wo_w13_fused_plan report (nano_amd/csrc/kernels.h QkvAttnFusedPlan / WoW13FusedPlan): kernel is
# an index into FUSED_KERNELS, role into Q80_ROLES; the word before takes is always 0
QKV_ATTN_FUSED_PLAN_FIELDS = ("kernel", "nv", "upw", "d", "qv", "threads", "n_attn", "ngemv", "lds_bytes", "rw", "wg0", "wg1", "wg2", "rounds",
                              "_zero", "takes")
WO_W13_FUSED_PLAN_FIELDS = ("sig", "threads", "role", "wf", "wfc", "nv_a", "upw_a", "nv_b", "upw_b", "wa", "wb", "lds_bytes", "rw_a", "rw_b",
                            "_zero", "takes", "cw")
FUSED_KERNELS = ("none", "q80_table", "q80_wf", "q4k", "f32")
NANO_DEVERR_HANDOFF = 2


# RouteKind of nano_amd/csrc/kernels.h (what NanoFusedGemvDesc.route_out reports)
ROUTE_NAMES = ("gemv", "gemv_preq", "gemv_sliced", "q4k", "reserved", "frag_g6", "frag_old", "frag_g7", "q4k_gemm", "f32_gemm")


class NanoHipError(RuntimeError):
    pass


class NanoHipTokenScore(C.Structure):
    """include/nano_mi355x.h NanoHipTokenScore: what the model thought of one fed position, for one target token (24 bytes)."""
    _fields_ = [("logprob", C.c_float), ("target_logit", C.c_float), ("max_logit", C.c_float), ("lse", C.c_float),
                ("argmax", C.c_uint32), ("rank", C.c_uint32)]


# the same record as a numpy structured dtype: prefill_score() / op_score_rows() return arrays of it
TOKEN_SCORE_DTYPE = np.dtype([("logprob", "<f4"), ("target_logit", "<f4"), ("max_logit", "<f4"), ("lse", "<f4"), ("argmax", "<u4"), ("rank", "<u4")])
assert TOKEN_SCORE_DTYPE.itemsize == C.sizeof(NanoHipTokenScore)


class NanoHipTopEntry(C.Structure):
    """include/nano_mi355x.h NanoHipTopEntry: one of the k most probable tokens of a row (12 bytes)."""
    _fields_ = [("token", C.c_uint32), ("logit", C.c_float), ("logprob", C.c_float)]


# the same record as a numpy structured dtype: the top-k methods return [rows, k] arrays of it, most probable first
TOP_ENTRY_DTYPE = np.dtype([("token", "<u4"), ("logit", "<f4"), ("logprob", "<f4")])
assert TOP_ENTRY_DTYPE.itemsize == C.sizeof(NanoHipTopEntry) == 12
TOPK_MAX = 32                                                          # NANO_TOPK_MAX


class NanoHipLookupParams(C.Structure):
    """include/nano_mi355x.h NanoHipLookupParams: greedy decode with lookup drafts (max_steps 0 = no limit; stop_token 0xffffffff = none)."""
    _fields_ = [(n, C.c_uint32) for n in ("max_draft", "ngram_max", "ngram_min", "stop_token", "max_steps")]


class NanoHipPoolParams(C.Structure):
    """include/nano_mi355x.h NanoHipPoolParams: text embeddings (pooling POOL_LAST | POOL_MEAN, normalize 0 | 1, dim 0 = n_embd, reserved 0)."""
    _fields_ = [(n, C.c_uint32) for n in ("pooling", "normalize", "dim", "reserved")]


POOL_LAST, POOL_MEAN = 0, 1


def _pooling(pooling) -> int:
    return {"last": POOL_LAST, "mean": POOL_MEAN}[pooling] if isinstance(pooling, str) else int(pooling)


class NanoHipLookupStats(C.Structure):
    """include/nano_mi355x.h NanoHipLookupStats (drafted = steps_verify * max_draft)."""
    _fields_ = [(n, C.c_uint32) for n in ("steps_plain", "steps_verify", "drafted", "accepted", "emitted")]


class NanoHipLookupSeq(C.Structure):
    """include/nano_mi355x.h NanoHipLookupSeq: one sequence of nano_hip_decode_lookup_rows (reserved 0)."""
    _fields_ = [(n, C.c_uint32) for n in ("slot", "n_history", "max_new", "reserved")]


assert C.sizeof(NanoHipLookupSeq) == 16

# the words of the record nano_hip_op_lookup_step returns (nano_amd/csrc/kernels.h LOOKUP_REC_*)
LOOKUP_RECORD_FIELDS = ("emitted", "accepted", "nb_next", "n", "match_len", "match_end", "done", "left")
LOOKUP_NO_STOP = 0xFFFFFFFF


class NanoHipDraftParams(C.Structure):
    """include/nano_mi355x.h NanoHipDraftParams: greedy decode with a draft model (max_rounds 0 = no limit; stop_token 0xffffffff = none)."""
    _fields_ = [(n, C.c_uint32) for n in ("max_draft", "stop_token", "max_rounds", "draft_held")]


class NanoHipDraftStats(C.Structure):
    """include/nano_mi355x.h NanoHipDraftStats (draft_held: what to pass as draft_held when the call is continued)."""
    _fields_ = [(n, C.c_uint32) for n in ("rounds_plain", "rounds_verify", "drafted", "accepted", "emitted", "draft_rows_fed", "draft_held")]


# the words of the record nano_hip_op_draft_round returns (nano_amd/csrc/kernels.h DRAFT_REC_*)
DRAFT_RECORD_FIELDS = ("emitted", "accepted", "nb_next", "n", "dn", "cursor", "done", "left")


PHASE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32)        # nano_hip_phase_fn(env, layer, phase)


_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the native library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NanoHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p

    def fn(name, restype, argtypes):
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
        return f

    fn("nano_hip_device_count", C.c_int, [])
    fn("nano_hip_last_error", C.c_char_p, [])
    fn("nano_hip_device_info", C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64)])
    fn("nano_hip_model_create", C.c_int, [C.POINTER(vp), C.POINTER(NanoModelDesc), vp, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_uint32])
    fn("nano_hip_model_create_ex", C.c_int, [C.POINTER(vp), C.POINTER(NanoModelDesc), vp, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32])
    fn("nano_hip_model_destroy", None, [vp])
    fn("nano_hip_params_bytes", C.c_size_t, [C.POINTER(NanoModelDesc)])
    fn("nano_hip_weight_bytes_per_step", C.c_uint64, [vp])
    fn("nano_hip_forward", C.c_int, [vp, u32p, u32p, C.c_uint32, C.c_uint32, vp, vp])
    fn("nano_hip_decode_greedy", C.c_int, [vp, u32p, u32p, C.c_uint32, C.c_uint32, vp])
    fn("nano_hip_prefill", C.c_int, [vp, C.c_uint32, u32p, C.c_uint32, C.c_uint32])
    fn("nano_hip_prefill_chunk_tokens", C.c_uint32, [vp])
    fn("nano_hip_prefill_score", C.c_int, [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp])
    fn("nano_hip_op_score_rows", C.c_int, [C.c_int, vp, C.c_uint32, C.c_uint32, vp, vp])
    fn("nano_hip_decode_lookup", C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(NanoHipLookupParams), vp, C.POINTER(C.c_uint32), C.POINTER(NanoHipLookupStats)])
    fn("nano_hip_verify_draft", C.c_int, [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_uint32)])
    fn("nano_hip_op_lookup_step", C.c_int, [C.c_int, vp, C.c_uint32, vp, vp, C.c_uint32, C.POINTER(NanoHipLookupParams), C.c_uint32, C.c_uint32, vp, vp, vp])
    fn("nano_hip_decode_draft", C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(NanoHipDraftParams), vp, C.POINTER(C.c_uint32), C.POINTER(NanoHipDraftStats)])
    fn("nano_hip_op_draft_round", C.c_int, [C.c_int, vp, C.c_uint32, vp, vp, C.c_uint32, C.POINTER(NanoHipDraftParams), C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp])
    fn("nano_hip_lora_attach", C.c_int, [vp, C.c_uint32, C.c_uint32, f32p, C.c_size_t])
    fn("nano_hip_lora_enable", C.c_int, [vp, C.c_int])
    fn("nano_hip_forward_sample", C.c_int, [vp, C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(NanoHipSample)])
    fn("nano_hip_op_sample", C.c_int, [vp, f32p, u32p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(NanoHipSample)])
    fn("nano_hip_forward_sample_batch", C.c_int, [vp, u32p, u32p, C.c_uint32, C.POINTER(NanoHipSampleParams), C.POINTER(NanoHipSample)])
    fn("nano_hip_op_sample_batch", C.c_int, [vp, f32p, C.c_uint32, C.POINTER(NanoHipSampleParams), C.POINTER(NanoHipSample)])
    fn("nano_hip_forward_sample_batch_ex", C.c_int, [vp, u32p, u32p, C.c_uint32, C.POINTER(NanoHipSampleParamsEx), C.POINTER(NanoHipSample)])
    fn("nano_hip_op_sample_batch_ex", C.c_int, [vp, f32p, C.c_uint32, C.POINTER(NanoHipSampleParamsEx), C.POINTER(NanoHipSample)])
    fn("nano_hip_sync", C.c_int, [vp])
    fn("nano_hip_set_strict", C.c_int, [vp, C.c_int])
    fn("nano_hip_set_phase_hook", C.c_int, [vp, PHASE_FN, vp])
    fn("nano_hip_set_exact", C.c_int, [vp, C.c_int])
    fn("nano_hip_exact_state", C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)])
    fn("nano_hip_op_exact_rmsnorm", C.c_int, [C.c_int, f32p, f32p, f32p, C.c_uint32])
    fn("nano_hip_op_exact_attention", C.c_int, [C.c_int, C.POINTER(NanoExactAttnDesc)])
    fn("nano_hip_time_classifier", C.c_int, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint64)])
    fn("nano_hip_time_classifier_in_step", C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_float)])
    fn("nano_hip_time_step", C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)])
    fn("nano_hip_membw", C.c_int, [C.c_int, C.c_size_t, C.c_uint32, C.POINTER(C.c_float)])
    fn("nano_hip_read_state", C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, f32p, C.c_size_t])
    fn("nano_hip_op_rmsnorm", C.c_int, [C.c_int, f32p, f32p, f32p, C.c_uint32])
    fn("nano_hip_op_matmul_f32", C.c_int, [C.c_int, f32p, f32p, f32p, C.c_uint32, C.c_uint32])
    fn("nano_hip_op_quantize_q80", C.c_int, [C.c_int, f32p, C.c_uint32, C.c_uint32, i8p, f32p])
    fn("nano_hip_op_matmul_q80", C.c_int, [C.c_int, f32p, i8p, f32p, i8p, f32p, C.c_uint32, C.c_uint32, C.c_uint32])
    fn("nano_hip_op_quantize_q4k", C.c_int, [C.c_int, f32p, C.c_uint32, u8p])
    fn("nano_hip_op_matmul_q4k", C.c_int, [C.c_int, f32p, u8p, u8p, C.c_uint32, C.c_uint32])
    fn("nano_hip_op_rope", C.c_int, [C.c_int, f32p, C.c_uint32, f32p, f32p, C.c_int])
    fn("nano_hip_op_attention", C.c_int, [C.c_int, f32p, f32p, f32p, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32])
    fn("nano_hip_op_swiglu", C.c_int, [C.c_int, f32p, f32p, C.c_uint32])
    fn("nano_hip_op_argmax", C.c_int, [C.c_int, f32p, C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_op_fused_gemv", C.c_int, [C.c_int, C.POINTER(NanoFusedGemvDesc)])
    fn("nano_hip_op_lora_qkv", C.c_int, [C.c_int, C.POINTER(NanoLoraOpDesc)])
    fn("nano_hip_op_lora_o", C.c_int, [C.c_int, C.POINTER(NanoLoraOpDesc)])
    fn("nano_hip_op_attention_decode", C.c_int, [C.c_int, C.POINTER(NanoAttnDecodeDesc)])
    fn("nano_hip_f32_gemv_plan", C.c_int, [C.POINTER(NanoFusedGemvDesc), C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_f32_gemm_plan", C.c_int, [C.POINTER(NanoFusedGemvDesc), C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_q80_gemv_plan", C.c_int, [C.POINTER(NanoFusedGemvDesc), C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_q80_gemm_plan", C.c_int, [C.POINTER(NanoFusedGemvDesc), C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_q4k_gemv_plan", C.c_int, [C.POINTER(NanoFusedGemvDesc), C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_qkv_attn_fused_plan", C.c_int, [C.POINTER(NanoFusedGemvDesc), C.POINTER(NanoAttnDecodeDesc), C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_wo_w13_fused_plan", C.c_int, [C.POINTER(NanoFusedGemvDesc), C.POINTER(NanoFusedGemvDesc), C.c_uint32, C.POINTER(C.c_uint32)])
    fn("nano_hip_op_qkv_attn_fused", C.c_int, [C.c_int, C.POINTER(NanoQkvAttnFusedDesc)])
    fn("nano_hip_op_wo_w13_fused", C.c_int, [C.c_int, C.POINTER(NanoWoW13FusedDesc)])
    fn("nano_hip_kv_release", C.c_int, [vp, C.c_uint32])
    fn("nano_hip_kv_pages", C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)])
    fn("nano_hip_kv_fork", C.c_int, [vp, C.c_uint32, C.c_uint32, u32p, C.c_uint32])
    fn("nano_hip_kv_sharing", C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)])
    fn("nano_prefill_shared", C.c_int, [vp, u32p, C.c_uint32, C.c_uint32])
    # ragged steps.  (Declared where present: NANO_LIB may name an older build, loaded to be measured against this one.)
    for name, args in (("nano_hip_step_rows", [vp, vp, C.c_uint32, vp, vp]),
                       ("nano_hip_rows_plan", [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint32)]),
                       ("nano_hip_rows_addressable", [C.c_uint32] * 4),
                       ("nano_prefill_batch", [vp, vp, u32p, C.c_uint32, vp]),
                       # top-k alternatives
                       ("nano_hip_op_topk_rows", [C.c_int, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
                       ("nano_hip_prefill_score_topk", [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]),
                       ("nano_hip_forward_topk", [vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp]),
                       ("nano_hip_step_rows_score", [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp]),
                       ("nano_score_ids_topk", [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(C.c_double)]),
                       ("nano_forward_batch_topk", [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]),
                       # text embeddings
                       ("nano_hip_step_rows_pool", [vp, vp, C.c_uint32, vp, C.POINTER(NanoHipPoolParams), vp]),
                       ("nano_hip_rows_pool_plan", [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]),
                       ("nano_hip_op_pool_rows", [C.c_int, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.POINTER(NanoHipPoolParams), C.c_uint32, vp]),
                       ("nano_embed_batch", [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
                       # lookup drafts for several sequences
                       ("nano_hip_decode_lookup_rows", [vp, vp, C.c_uint32, vp, C.POINTER(NanoHipLookupParams), vp, vp, vp, C.POINTER(C.c_uint32)]),
                       ("nano_hip_lookup_rows_plan", [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(C.c_uint32)]),
                       ("nano_hip_op_lookup_rows_round", [C.c_int, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.POINTER(NanoHipLookupParams),
                                                          C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]),
                       ("nano_decode_batch_lookup", [vp, vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, vp, vp]),
                       # logit edits
                       ("nano_hip_forward_sample_batch_edit", [vp, u32p, u32p, C.c_uint32, C.POINTER(NanoHipSampleParamsEdit), C.POINTER(NanoHipSample)]),
                       ("nano_hip_op_sample_batch_edit", [vp, f32p, C.c_uint32, C.POINTER(NanoHipSampleParamsEdit), C.POINTER(NanoHipSample)]),
                       ("nano_hip_mask_table_set", [vp, C.c_void_p, C.c_uint32]),
                       ("nano_set_logit_edit", [vp, vp]),
                       ("nano_forward_batch_sample_edit", [vp, u32p, u32p, C.c_uint32, vp, vp, vp, vp, vp]),
                       # KV images
                       ("nano_hip_kv_image_plan", [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
                       ("nano_hip_kv_image_check", [vp, C.c_size_t, vp]),
                       ("nano_hip_kv_save", [vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
                       ("nano_hip_kv_restore", [vp, C.c_uint32, vp, C.c_size_t, C.c_uint32]),
                       ("nano_kv_save", [vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
                       ("nano_kv_restore", [vp, C.c_uint32, vp, C.c_size_t, C.c_uint32]),
                       # LoRA table
                       ("nano_hip_lora_table_set", [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t]),
                       ("nano_hip_lora_table_clear", [vp, C.c_uint32]),
                       ("nano_hip_lora_bind", [vp, vp, vp, C.c_uint32]),
                       ("nano_hip_lora_binding", [vp, C.c_uint32, C.POINTER(C.c_uint32)]),
                       ("nano_hip_op_lora_qkv_rows", [C.c_int, C.POINTER(NanoLoraRowsOpDesc)]),
                       ("nano_hip_op_lora_o_rows", [C.c_int, C.POINTER(NanoLoraRowsOpDesc)]),
                       ("nano_lora_table_load", [vp, C.c_uint32, C.c_char_p]),
                       ("nano_lora_table_load_from_buffer", [vp, C.c_uint32, vp, C.c_size_t]),
                       ("nano_lora_table_free", [vp, C.c_uint32]),
                       ("nano_lora_bind", [vp, vp, vp, C.c_uint32])):
        if hasattr(L, name) or not os.environ.get("NANO_LIB"):
            fn(name, C.c_int, args)
    for name, args in (("nano_hip_kv_image_bytes", [vp, C.c_uint32]), ("nano_kv_image_bytes", [vp, C.c_uint32]),
                       ("nano_hip_lora_param_floats", [C.c_uint32] * 4)):
        if hasattr(L, name) or not os.environ.get("NANO_LIB"):
            fn(name, C.c_size_t, args)
    fn("nano_hip_handoff_state", C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)])
    fn("nano_hip_set_fusion", C.c_int, [vp, C.c_uint32])
    fn("nano_hip_debug_fault", C.c_int, [vp, C.c_uint32])
    fn("nano_hip_background_load", C.c_int, [C.c_int, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32])
    fn("nano_hip_stamps_begin", C.c_int, [vp])
    fn("nano_hip_stamps_read", C.c_int, [vp, vp, u32p, C.c_uint32, C.POINTER(C.c_uint32)])
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise NanoHipError(f"nano_hip error {rc}: {lib().nano_hip_last_error().decode(errors='replace')}")


def row_segs(segs) -> np.ndarray:
    """(slot, pos0, count[, reserved]) rows as the NanoHipRowSeg array the library reads: uint32 [n][4]"""
    s = np.zeros((len(segs), 4), np.uint32)
    for i, g in enumerate(segs):
        s[i, :len(g)] = g
    return s


def rows_plan(segs, cap: int, max_seq_len: int):
    """nano_hip_rows_plan (device-free): how a ragged step cuts its rows into passes of at most cap rows.  Returns
    (row_pass, row_index, row_hint, n_passes), the arrays per row in caller order."""
    s = row_segs(segs)
    rows = int(s[:, 2].astype(np.uint64).sum()) if s.size else 0
    rows = min(rows, len(segs) * max_seq_len)          # (no plan has more; a refused list may claim any number)
    rp, ri, rh = (np.zeros(max(rows, 1), np.uint32) for _ in range(3))
    n = C.c_uint32(0)
    check(lib().nano_hip_rows_plan(s.ctypes.data if s.size else None, s.shape[0], cap, max_seq_len, rp.ctypes.data, ri.ctypes.data, rh.ctypes.data, C.byref(n)))
    return rp[:rows], ri[:rows], rh[:rows], int(n.value)


def rows_pool_plan(segs, cap: int, max_seq_len: int, pooling="last"):
    """nano_hip_rows_pool_plan (device-free): the row map step_rows_pool() builds for its kernel.  Returns (row_seg, row_ordinal), per fed
    row in feeding order (pass after pass, a pass's rows by rows_plan()'s row_index); row_ordinal is 0xffffffff where a row is not pooled."""
    s = row_segs(segs)
    rows = int(s[:, 2].astype(np.uint64).sum()) if s.size else 0
    rows = min(rows, len(segs) * max_seq_len)          # (no plan has more; a refused list may claim any number)
    rs, ro = (np.zeros(max(rows, 1), np.uint32) for _ in range(2))
    check(lib().nano_hip_rows_pool_plan(s.ctypes.data if s.size else None, s.shape[0], cap, max_seq_len, _pooling(pooling), rs.ctypes.data, ro.ctypes.data))
    return rs[:rows], ro[:rows]


class NanoKvImageHeader(C.Structure):
    """include/nano_mi355x.h NanoKvImageHeader: the 64-byte header of a KV image."""
    _fields_ = [(n, C.c_uint32) for n in ("magic", "version", "header_bytes", "format", "n_layer", "kv_dim", "n_pos", "block_rows", "row_bytes",
                                          "reserved0")] + [("payload_bytes", C.c_uint64), ("model_tag", C.c_uint64), ("reserved1", C.c_uint32 * 2)]


assert C.sizeof(NanoKvImageHeader) == 64
KV_IMAGE_PLAN_FIELDS = ("header_bytes", "payload_bytes", "total_bytes", "blocks", "last_rows", "block_stride", "vec_bytes", "_zero")
KV_ALL = 0xFFFFFFFF                                                   # nano_hip_kv_restore's n_pos for "all of the image"


def kv_image_plan(n_layer: int, kv_dim: int, elem_bytes: int, n_pos: int) -> dict:
    """nano_hip_kv_image_plan (device-free): the sizes of the image of n_pos positions of a cache of n_layer layers, kv_dim elements per
    row and elem_bytes (4 FP32, 2 FP16, 1 FP8) per element."""
    out = np.zeros(len(KV_IMAGE_PLAN_FIELDS), np.uint64)
    check(lib().nano_hip_kv_image_plan(n_layer, kv_dim, elem_bytes, n_pos, out.ctypes.data))
    return {k: int(v) for k, v in zip(KV_IMAGE_PLAN_FIELDS, out)}


def kv_image_check(image) -> dict:
    """nano_hip_kv_image_check (device-free): the header's fields of a well-formed image (bytes-like or uint8 array); raises NanoHipError
    with the library's message for anything else."""
    a = np.ascontiguousarray(np.frombuffer(image, np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else image, np.uint8).reshape(-1)
    h = NanoKvImageHeader()
    check(lib().nano_hip_kv_image_check(a.ctypes.data if a.size else None, a.size, C.byref(h)))
    return {n: (list(getattr(h, n)) if n == "reserved1" else int(getattr(h, n))) for n, _ in NanoKvImageHeader._fields_}


def last_error() -> str:
    return lib().nano_hip_last_error().decode(errors="replace")


def device_count() -> int:
    return int(lib().nano_hip_device_count())


def device_info(device: int = 0):
    name = C.create_string_buffer(64)
    mem = C.c_uint64(0)
    cus = lib().nano_hip_device_info(device, name, 64, C.byref(mem))
    if cus < 0:
        check(cus)
    return {"arch": name.value.decode(), "cus": int(cus), "mem_bytes": int(mem.value)}


def membw(device: int = 0, nbytes: int = 1 << 30, iters: int = 10) -> float:
    g = C.c_float(0)
    check(lib().nano_hip_membw(device, nbytes, iters, C.byref(g)))
    return float(g.value)


def background_load(device: int = 0, nbytes: int = 1 << 30, iters: int = 10, xcd_mask: int = 0xff, wgs: int = 2048):
    """A competing streaming reader on the XCDs of xcd_mask (blocks until done: run it in a thread)."""
    check(lib().nano_hip_background_load(device, nbytes, iters, xcd_mask, wgs))


STATE_IDS = {"x": 0, "q": 1, "xba": 2, "hb": 3, "logits": 4, "k": 5, "v": 6}


class NanoHipSample(C.Structure):
    """Result of the device-side sampler (include/nano_mi355x.h NanoHipSample)."""
    _fields_ = [("token", C.c_uint32), ("status", C.c_uint32), ("n_candidates", C.c_uint32), ("n_sorted", C.c_uint32), ("nucleus", C.c_uint32),
                ("top", C.c_uint32 * 6), ("sum_bits", C.c_uint32), ("walked_chunks", C.c_uint32)]


class NanoHipSampleParams(C.Structure):
    """One row of the batched device sampler (include/nano_mi355x.h NanoHipSampleParams)."""
    _fields_ = [("repetition_penalty", C.c_float), ("temperature", C.c_float), ("top_p", C.c_float), ("coin", C.c_float),
                ("history", C.POINTER(C.c_uint32)), ("n_history", C.c_uint32)]


def sample_params(rows):
    """rows: (repetition_penalty, temperature, top_p, coin, history) per row -> (ctypes array, the history arrays it points into:
    keep them alive for the call)"""
    arr = (NanoHipSampleParams * len(rows))()
    keep = []
    for i, (rp, temp, top_p, coin, hist) in enumerate(rows):
        h = np.ascontiguousarray(hist if hist is not None else [], np.uint32).reshape(-1)
        keep.append(h)
        arr[i] = NanoHipSampleParams(rp, temp, top_p, coin, h.ctypes.data_as(C.POINTER(C.c_uint32)) if h.size else None, h.size)
    return arr, keep


class NanoHipSampleParamsEx(C.Structure):
    """A row with top-k truncation in front of the top-p cut (include/nano_mi355x.h NanoHipSampleParamsEx): top_k 0 = off."""
    _fields_ = [("p", NanoHipSampleParams), ("top_k", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def sample_params_ex(rows, top_k):
    """sample_params() with row i's top_k: one int for all rows, or one per row"""
    base, keep = sample_params(rows)
    ks = [int(top_k)] * len(rows) if np.isscalar(top_k) else [int(k) for k in top_k]
    assert len(ks) == len(rows)
    arr = (NanoHipSampleParamsEx * len(rows))()
    for i, k in enumerate(ks):
        arr[i].p = base[i]
        arr[i].top_k = k
    return arr, keep


NANO_BIAS_MAX = 1024


class NanoHipLogitBias(C.Structure):
    """One entry of a row's bias list (include/nano_mi355x.h NanoHipLogitBias)."""
    _fields_ = [("token", C.c_uint32), ("bias", C.c_float)]


class NanoHipSampleParamsEdit(C.Structure):
    """A row with a logit edit (include/nano_mi355x.h NanoHipSampleParamsEdit): a mask per call (allow) or by table id, and a bias list."""
    _fields_ = [("ex", NanoHipSampleParamsEx), ("allow", C.POINTER(C.c_uint32)), ("bias", C.POINTER(NanoHipLogitBias)),
                ("mask_id", C.c_uint32), ("n_bias", C.c_uint32)]


def mask_words(allowed, vocab):
    """ceil(vocab / 32) mask words from a boolean array [vocab] or a list of allowed ids"""
    a = np.asarray(allowed)
    on = np.zeros(-(-vocab // 32) * 32, bool)
    if a.dtype == bool:
        on[:vocab] = a.reshape(-1)
    else:
        on[a.astype(np.int64).reshape(-1)] = True
    return np.packbits(on.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def sample_params_edit(rows, top_k, edits):
    """sample_params_ex() with row i's edit: None, or a dict with any of allow (uint32 mask words), mask_id (int, 1-based),
    bias (a (tokens, values) pair of arrays)"""
    base, keep = sample_params_ex(rows, top_k)
    edits = [None] * len(rows) if edits is None else list(edits)
    assert len(edits) == len(rows)
    arr = (NanoHipSampleParamsEdit * len(rows))()
    for i, e in enumerate(edits):
        arr[i].ex = base[i]
        if not e:
            continue
        if e.get("allow") is not None:
            w = np.ascontiguousarray(e["allow"], np.uint32).reshape(-1)
            keep.append(w)
            arr[i].allow = w.ctypes.data_as(C.POINTER(C.c_uint32))
        arr[i].mask_id = int(e.get("mask_id", 0))
        b = e.get("bias")
        if b is not None and len(b[0]):
            ent = np.zeros(np.size(b[0]), np.dtype([("token", "<u4"), ("bias", "<f4")]))      # NanoHipLogitBias[n]
            ent["token"], ent["bias"] = np.asarray(b[0]).reshape(-1), np.asarray(b[1]).reshape(-1)
            keep.append(ent)
            arr[i].bias = ent.ctypes.data_as(C.POINTER(NanoHipLogitBias))
            arr[i].n_bias = ent.size
    return arr, keep


class DeviceModel:
    """A model resident on one GPU: mirrors what the reference keeps in ``LLM`` (weights + FwdBuffer).
    kv_f16 / kv_paged / kv_fp8: with all three None the library reads NANO_KV_F16 / NANO_KV_FP8 / NANO_KV_PAGED from the environment;
    as soon as one of them is given (False included) the flags are exactly the keywords and the environment is not consulted."""

    def __init__(self, desc: NanoModelDesc, params, params_bytes: int, *, on_device: bool = False,
                 device: int = 0, max_seq_len: int = 512, max_batch: int = 1, kv_f16: Optional[bool] = None,
                 kv_paged: Optional[bool] = None, kv_fp8: Optional[bool] = None):
        self.desc = desc
        self.h = C.c_void_p(None)
        ptr = params if isinstance(params, int) else params.ctypes.data
        if kv_fp8 is not None:       # explicit flags, NANO_HIP_KV_FP8 = 4 among them (with kv_f16: refused by the library)
            check(lib().nano_hip_model_create_ex(C.byref(self.h), C.byref(desc), C.c_void_p(ptr), params_bytes,
                                                 1 if on_device else 0, device, max_seq_len, max_batch,
                                                 (1 if kv_f16 else 0) | (2 if kv_paged else 0) | (4 if kv_fp8 else 0)))
        elif kv_paged is not None:   # explicit flags: NANO_HIP_KV_F16 = 1, NANO_HIP_KV_PAGED = 2
            check(lib().nano_hip_model_create_ex(C.byref(self.h), C.byref(desc), C.c_void_p(ptr), params_bytes,
                                                 1 if on_device else 0, device, max_seq_len, max_batch,
                                                 (1 if kv_f16 else 0) | (2 if kv_paged else 0)))
        elif kv_f16 is None:         # environment default (NANO_KV_F16 / NANO_KV_FP8 / NANO_KV_PAGED)
            check(lib().nano_hip_model_create(C.byref(self.h), C.byref(desc), C.c_void_p(ptr), params_bytes,
                                              1 if on_device else 0, device, max_seq_len, max_batch))
        else:
            check(lib().nano_hip_model_create_ex(C.byref(self.h), C.byref(desc), C.c_void_p(ptr), params_bytes,
                                                 1 if on_device else 0, device, max_seq_len, max_batch, 1 if kv_f16 else 0))
        self.vocab = int(desc.vocab_size)
        self.max_seq_len, self.max_batch, self.device = max_seq_len, max_batch, device

    def close(self):
        if self.h:
            lib().nano_hip_model_destroy(self.h)
            self.h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def weight_bytes_per_step(self) -> int:
        return int(lib().nano_hip_weight_bytes_per_step(self.h))

    def forward(self, tokens: Sequence[int], pos: Sequence[int], is_causal: int = 1, want_logits: bool = True,
                want_argmax: bool = False):
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        p = np.ascontiguousarray(pos, np.uint32).reshape(-1)
        B = t.size
        logits = np.empty((B, self.vocab), np.float32) if want_logits else None
        amax = np.empty(B, np.uint32) if want_argmax else None
        check(lib().nano_hip_forward(self.h, t, p, B, is_causal,
                                     logits.ctypes.data if want_logits else None,
                                     amax.ctypes.data if want_argmax else None))
        return logits, amax

    def decode_greedy(self, tokens: Sequence[int], pos: Sequence[int], steps: int, fetch: bool = True) -> Optional[np.ndarray]:
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        p = np.ascontiguousarray(pos, np.uint32).reshape(-1)
        out = np.empty((steps, t.size), np.uint32) if fetch else None
        check(lib().nano_hip_decode_greedy(self.h, t, p, t.size, steps, out.ctypes.data if fetch else None))
        return out

    def prefill(self, tokens: Sequence[int], pos0: int = 0, slot: int = 0):
        """Batched prefill of one sequence: tokens at positions pos0.. (no logits)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        check(lib().nano_hip_prefill(self.h, slot, t, pos0, t.size))

    def prefill_score(self, tokens: Sequence[int], targets: Optional[Sequence[int]] = None, pos0: int = 0, slot: int = 0) -> np.ndarray:
        """prefill() that also scores every fed position on the device (nano_hip_prefill_score): entry i of the returned
        TOKEN_SCORE_DTYPE array describes the logits of tokens[i] at pos0 + i for targets[i] (None: for that row's own arg-max).
        Perplexity of ids: prefill_score(ids[:-1], ids[1:])."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        g = None if targets is None else np.ascontiguousarray(targets, np.uint32).reshape(-1)
        if g is not None and g.size != t.size:
            raise ValueError(f"{t.size} tokens but {g.size} targets")
        out = np.zeros(t.size, TOKEN_SCORE_DTYPE)
        check(lib().nano_hip_prefill_score(self.h, slot, t.ctypes.data, pos0, t.size, None if g is None else g.ctypes.data, out.ctypes.data))
        return out

    def prefill_score_topk(self, tokens: Sequence[int], k: int, targets: Optional[Sequence[int]] = None, pos0: int = 0, slot: int = 0):
        """prefill_score() plus the k most probable tokens of every fed position (nano_hip_prefill_score_topk).  Returns (scores
        TOKEN_SCORE_DTYPE[len(tokens)], top TOP_ENTRY_DTYPE[len(tokens), k], most probable first); k = 0: (scores, None)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        g = None if targets is None else np.ascontiguousarray(targets, np.uint32).reshape(-1)
        if g is not None and g.size != t.size:
            raise ValueError(f"{t.size} tokens but {g.size} targets")
        out = np.zeros(t.size, TOKEN_SCORE_DTYPE)
        top = np.zeros((t.size, k), TOP_ENTRY_DTYPE) if k else None
        check(lib().nano_hip_prefill_score_topk(self.h, slot, t.ctypes.data, pos0, t.size, None if g is None else g.ctypes.data, k,
                                                out.ctypes.data, top.ctypes.data if k else None))
        return out, top

    def forward_topk(self, tokens: Sequence[int], pos: Sequence[int], k: int, targets: Optional[Sequence[int]] = None):
        """One causal decode step of slots 0 .. B-1 whose logits stay on the device (nano_hip_forward_topk).  Returns (scores
        TOKEN_SCORE_DTYPE[B] for targets -- None: each row's own arg-max --, top TOP_ENTRY_DTYPE[B, k]); k = 0: (scores, None)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        p = np.ascontiguousarray(pos, np.uint32).reshape(-1)
        g = None if targets is None else np.ascontiguousarray(targets, np.uint32).reshape(-1)
        if p.size != t.size or (g is not None and g.size != t.size):
            raise ValueError(f"{t.size} tokens but {p.size} positions / {0 if g is None else g.size} targets")
        out = np.zeros(t.size, TOKEN_SCORE_DTYPE)
        top = np.zeros((t.size, k), TOP_ENTRY_DTYPE) if k else None
        check(lib().nano_hip_forward_topk(self.h, t.ctypes.data, p.ctypes.data, t.size, None if g is None else g.ctypes.data, k,
                                          out.ctypes.data, top.ctypes.data if k else None))
        return out, top

    def step_rows_score(self, segs: Sequence[Sequence[int]], tokens: Sequence[int], k: int, targets: Optional[Sequence[int]] = None):
        """The scoring form of a ragged step (nano_hip_step_rows_score): step_rows() that returns, per row in caller order, what
        prefill_score_topk() per segment returns: (scores TOKEN_SCORE_DTYPE[rows], top TOP_ENTRY_DTYPE[rows, k]); k = 0: (scores, None)."""
        s = row_segs(segs)
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        g = None if targets is None else np.ascontiguousarray(targets, np.uint32).reshape(-1)
        rows = int(s[:, 2].sum()) if s.size else 0
        if t.size != rows or (g is not None and g.size != rows):
            raise ValueError(f"{rows} rows but {t.size} tokens / {0 if g is None else g.size} targets")
        out = np.zeros(max(rows, 1), TOKEN_SCORE_DTYPE)
        top = np.zeros((max(rows, 1), k), TOP_ENTRY_DTYPE) if k else None
        check(lib().nano_hip_step_rows_score(self.h, s.ctypes.data if s.size else None, s.shape[0], t.ctypes.data if t.size else None,
                                             None if g is None else g.ctypes.data, k, out.ctypes.data, top.ctypes.data if k else None))
        return out[:rows], (top[:rows] if k else None)

    def decode_lookup(self, history: Sequence[int], max_new: int, max_draft: int = 7, ngram_max: int = 3, ngram_min: int = 1,
                      stop_token: Optional[int] = None, max_steps: int = 0):
        """Greedy decode of slot 0 with lookup drafts (nano_hip_decode_lookup): slot 0 holds positions 0 .. len(history)-2, history[-1] is
        fed first.  Returns (ids uint32[<= max_new], stats dict of steps_plain / steps_verify / drafted / accepted / emitted)."""
        h = np.ascontiguousarray(history, np.uint32).reshape(-1)
        p = NanoHipLookupParams(max_draft, ngram_max, ngram_min, LOOKUP_NO_STOP if stop_token is None else stop_token, max_steps)
        out = np.zeros(max(max_new, 1), np.uint32)
        n, st = C.c_uint32(0), NanoHipLookupStats()
        check(lib().nano_hip_decode_lookup(self.h, h.ctypes.data if h.size else None, h.size, max_new, C.byref(p), out.ctypes.data, C.byref(n), C.byref(st)))
        return out[:n.value].copy(), {k: int(getattr(st, k)) for k, _ in NanoHipLookupStats._fields_}

    def decode_lookup_rows(self, histories, slots, max_new, max_draft: int = 7, ngram_max: int = 3, ngram_min: int = 1,
                           stop_token: Optional[int] = None, max_steps: int = 0):
        """Greedy decode of several sequences with lookup drafts, one ragged verify pass per round (nano_hip_decode_lookup_rows): slot
        slots[i] holds positions 0 .. len(histories[i])-2, histories[i][-1] is fed first, at most max_new[i] ids are emitted.  Returns
        (list of uint32 id arrays, list of stats dicts as decode_lookup's, rounds)."""
        hs = [np.ascontiguousarray(h, np.uint32).reshape(-1) for h in histories]
        B = len(hs)
        if len(slots) != B or len(max_new) != B:
            raise ValueError(f"{B} histories but {len(slots)} slots / {len(max_new)} max_new")
        seqs = (NanoHipLookupSeq * max(B, 1))(*[NanoHipLookupSeq(int(s), h.size, int(mn), 0) for h, s, mn in zip(hs, slots, max_new)])
        outs = [np.zeros(max(int(mn), 1), np.uint32) for mn in max_new]
        hp = (C.c_void_p * max(B, 1))(*[h.ctypes.data if h.size else None for h in hs])
        op = (C.c_void_p * max(B, 1))(*[o.ctypes.data for o in outs])
        p = NanoHipLookupParams(max_draft, ngram_max, ngram_min, LOOKUP_NO_STOP if stop_token is None else stop_token, max_steps)
        n, st, rounds = np.zeros(max(B, 1), np.uint32), (NanoHipLookupStats * max(B, 1))(), C.c_uint32(0)
        check(lib().nano_hip_decode_lookup_rows(self.h, seqs, B, hp, C.byref(p), op, n.ctypes.data, st, C.byref(rounds)))
        return ([outs[i][:int(n[i])].copy() for i in range(B)],
                [{k: int(getattr(st[i], k)) for k, _ in NanoHipLookupStats._fields_} for i in range(B)], int(rounds.value))

    def decode_draft(self, draft: "DeviceModel", history: Sequence[int], max_new: int, max_draft: int = 4, stop_token: Optional[int] = None,
                     max_rounds: int = 0, draft_held: int = 0):
        """Greedy decode of slot 0 with `draft` as the draft model (nano_hip_decode_draft): this model's slot 0 holds positions
        0 .. len(history)-2, history[-1] is fed first; the draft's slot 0 holds the first draft_held positions and is fed the rest by the
        call.  Returns (ids uint32[<= max_new], stats dict of NanoHipDraftStats' fields; pass stats["draft_held"] on to continue)."""
        h = np.ascontiguousarray(history, np.uint32).reshape(-1)
        p = NanoHipDraftParams(max_draft, LOOKUP_NO_STOP if stop_token is None else stop_token, max_rounds, draft_held)
        out = np.zeros(max(max_new, 1), np.uint32)
        n, st = C.c_uint32(0), NanoHipDraftStats()
        check(lib().nano_hip_decode_draft(self.h, None if draft is None else draft.h, h.ctypes.data if h.size else None, h.size, max_new, C.byref(p),
                                          out.ctypes.data, C.byref(n), C.byref(st)))
        return out[:n.value].copy(), {k: int(getattr(st, k)) for k, _ in NanoHipDraftStats._fields_}

    def verify_draft(self, tokens: Sequence[int], pos0: int = 0, slot: int = 0):
        """prefill() that returns every fed row's arg-max (nano_hip_verify_draft): tokens[0] the last committed id, tokens[1:] a draft.
        Returns (argmax uint32[len(tokens)], n_accepted)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        out = np.zeros(max(t.size, 1), np.uint32)
        a = C.c_uint32(0)
        check(lib().nano_hip_verify_draft(self.h, slot, t.ctypes.data if t.size else None, pos0, t.size, out.ctypes.data, C.byref(a)))
        return out[:t.size], int(a.value)

    def prefill_chunk_tokens(self) -> int:
        """Prompt tokens prefill() feeds per weight read in the model's current mode (64 | 8; strict / exact mode: 1)."""
        return int(lib().nano_hip_prefill_chunk_tokens(self.h))

    def step_rows(self, segs: Sequence[Sequence[int]], tokens: Sequence[int], want_argmax: bool = False) -> Optional[np.ndarray]:
        """A ragged step (nano_hip_step_rows): segs = (slot, pos0, count) triples, tokens = their ids, segment after segment.  Each
        slot's K / V rows are those of prefill() per segment; want_argmax: returns every row's arg-max, caller order (verify_draft's)."""
        s = row_segs(segs)
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        rows = int(s[:, 2].sum()) if s.size else 0
        if t.size != rows:
            raise ValueError(f"{rows} rows but {t.size} tokens")
        out = np.zeros(max(rows, 1), np.uint32) if want_argmax else None
        check(lib().nano_hip_step_rows(self.h, s.ctypes.data if s.size else None, s.shape[0], t.ctypes.data if t.size else None,
                                       out.ctypes.data if want_argmax else None))
        return out[:rows] if want_argmax else None

    def step_rows_pool(self, segs: Sequence[Sequence[int]], tokens: Sequence[int], pooling="last", normalize: bool = True, dim: int = 0) -> np.ndarray:
        """Text embeddings from a ragged step (nano_hip_step_rows_pool): step_rows() that stops in front of the classifier and returns
        one vector per segment, float32 [len(segs), dim or n_embd]: the final-norm hidden state of the segment's last row (pooling "last")
        or the mean over its rows ("mean"), cut to `dim` leading components, then scaled to unit length (normalize)."""
        s = row_segs(segs)
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        rows = int(s[:, 2].sum()) if s.size else 0
        if t.size != rows:
            raise ValueError(f"{rows} rows but {t.size} tokens")
        p = NanoHipPoolParams(_pooling(pooling), int(normalize), dim, 0)
        out = np.zeros((max(s.shape[0], 1), dim or int(self.desc.n_embd)), np.float32)
        check(lib().nano_hip_step_rows_pool(self.h, s.ctypes.data if s.size else None, s.shape[0], t.ctypes.data if t.size else None,
                                            C.byref(p), out.ctypes.data))
        return out[:s.shape[0]]

    def rows_plan(self, segs: Sequence[Sequence[int]], max_seq_len: int):
        """How step_rows() cuts these segments in the model's current mode: rows_plan(segs, prefill_chunk_tokens(), max_seq_len)."""
        return rows_plan(segs, self.prefill_chunk_tokens(), max_seq_len)

    # top_k= on the four helpers below: the default, the int 0, is the entry point without top_k; anything else -- an int >= 1, or one
    # value per row (zeros included) -- goes through the _ex entry point (nano_mi355x.h, "top-k truncation").
    def forward_sample(self, token: int, pos: int, history: Sequence[int], repetition_penalty: float, temperature: float,
                       top_p: float, coin: float, top_k: int = 0) -> NanoHipSample:
        """One decode step of slot 0 + the reference's sampler on the device (infer.c:1156-1189)."""
        if top_k != 0:
            return self.forward_sample_batch([token], [pos], [(repetition_penalty, temperature, top_p, coin, history)], top_k=[top_k])[0]
        h = np.ascontiguousarray(history, np.uint32).reshape(-1)
        r = NanoHipSample()
        check(lib().nano_hip_forward_sample(self.h, token, pos, h, h.size, repetition_penalty, temperature, top_p, coin, C.byref(r)))
        return r

    def op_sample(self, logits: np.ndarray, history: Sequence[int], repetition_penalty: float, temperature: float,
                  top_p: float, coin: float, top_k: int = 0) -> NanoHipSample:
        """The device sampler alone, on host-provided logits (V floats)."""
        l = np.ascontiguousarray(logits, np.float32).reshape(-1)
        assert l.size == self.vocab
        if top_k != 0:
            return self.op_sample_batch(l.reshape(1, -1), [(repetition_penalty, temperature, top_p, coin, history)], top_k=[top_k])[0]
        h = np.ascontiguousarray(history, np.uint32).reshape(-1)
        r = NanoHipSample()
        check(lib().nano_hip_op_sample(self.h, l, h, h.size, repetition_penalty, temperature, top_p, coin, C.byref(r)))
        return r

    def set_mask_table(self, masks) -> None:
        """nano_hip_mask_table_set: masks [n][ceil(V / 32)] uint32 words replace the model's mask table (rows refer to it by
        mask_id = index + 1); None or an empty array frees it."""
        w = np.zeros((0, 0), np.uint32) if masks is None else np.ascontiguousarray(masks, np.uint32)
        n = 0 if w.size == 0 else (1 if w.ndim == 1 else w.shape[0])
        check(lib().nano_hip_mask_table_set(self.h, w.ctypes.data if n else None, n))

    def forward_sample_batch(self, tokens: Sequence[int], pos: Sequence[int], params, top_k=0, edits=None) -> list:
        """One decode step of slots 0..B-1, then row i sampled on the device with params[i] =
        (repetition_penalty, temperature, top_p, coin, history); one NanoHipSample per row.  top_k: one int, or one per row.
        edits: None (the entry points without edits), or one entry per row as sample_params_edit takes them."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        p = np.ascontiguousarray(pos, np.uint32).reshape(-1)
        out = (NanoHipSample * max(t.size, 1))()
        if edits is not None:
            arr, _keep = sample_params_edit(params, top_k, edits)
            check(lib().nano_hip_forward_sample_batch_edit(self.h, t, p, t.size, arr, out))
        elif np.isscalar(top_k) and top_k == 0:
            arr, _keep = sample_params(params)
            check(lib().nano_hip_forward_sample_batch(self.h, t, p, t.size, arr, out))
        else:
            arr, _keep = sample_params_ex(params, top_k)
            check(lib().nano_hip_forward_sample_batch_ex(self.h, t, p, t.size, arr, out))
        return list(out)[:t.size]

    def op_sample_batch(self, logits: np.ndarray, params, top_k=0, edits=None) -> list:
        """The batched device sampler alone, on host logits [B][V]; params, top_k and edits as forward_sample_batch."""
        l = np.ascontiguousarray(logits, np.float32)
        assert l.ndim == 2 and l.shape[1] == self.vocab
        out = (NanoHipSample * max(l.shape[0], 1))()
        if edits is not None:
            arr, _keep = sample_params_edit(params, top_k, edits)
            check(lib().nano_hip_op_sample_batch_edit(self.h, l.reshape(-1), l.shape[0], arr, out))
        elif np.isscalar(top_k) and top_k == 0:
            arr, _keep = sample_params(params)
            check(lib().nano_hip_op_sample_batch(self.h, l.reshape(-1), l.shape[0], arr, out))
        else:
            arr, _keep = sample_params_ex(params, top_k)
            check(lib().nano_hip_op_sample_batch_ex(self.h, l.reshape(-1), l.shape[0], arr, out))
        return list(out)[:l.shape[0]]

    def lora_attach_file(self, path: str):
        """Attach a LoRA module file (reference format: 256-byte header, rank / alpha = words 6 / 7, then FP32 tensors)."""
        raw = np.fromfile(path, dtype=np.uint8)
        hdr = raw[:256].view(np.uint32)
        params = np.ascontiguousarray(raw[256:].view(np.float32))
        check(lib().nano_hip_lora_attach(self.h, int(hdr[6]), int(hdr[7]), params, params.size))

    def lora_enable(self, on: bool):
        check(lib().nano_hip_lora_enable(self.h, 1 if on else 0))

    def lora_table_set_file(self, id: int, path: str):
        """Store a LoRA module file (format as lora_attach_file) as entry `id` of the model's LoRA table (nano_hip_lora_table_set)."""
        raw = np.fromfile(path, dtype=np.uint8)
        hdr = raw[:256].view(np.uint32)
        params = np.ascontiguousarray(raw[256:].view(np.float32))
        check(lib().nano_hip_lora_table_set(self.h, id, int(hdr[6]), int(hdr[7]), params.ctypes.data, params.size))

    def lora_table_clear(self, id: int):
        check(lib().nano_hip_lora_table_clear(self.h, id))

    def lora_bind(self, slots, ids):
        """KV slot slots[i] takes table entry ids[i]; None (or NANO_LORA_NONE) = no module (nano_hip_lora_bind)."""
        s = np.ascontiguousarray(slots, np.uint32)
        i = np.ascontiguousarray([NANO_LORA_NONE if v is None else v for v in ids], np.uint32)
        assert s.ndim == 1 and s.shape == i.shape
        check(lib().nano_hip_lora_bind(self.h, s.ctypes.data, i.ctypes.data, s.size))

    def lora_binding(self, slot: int):
        """the table entry `slot` is bound to, or None"""
        out = C.c_uint32(0)
        check(lib().nano_hip_lora_binding(self.h, slot, C.byref(out)))
        return None if out.value == NANO_LORA_NONE else int(out.value)

    def sync(self):
        check(lib().nano_hip_sync(self.h))

    def set_strict(self, on: bool = True):
        """Strict-parity mode: eager, reference summation order, logits bit-identical to the reference CPU engine."""
        check(lib().nano_hip_set_strict(self.h, 1 if on else 0))

    def set_exact(self, on: bool = True):
        """Exact mode: strict mode's bits (the reference CPU engine's) from steps that are captured once and replayed as HIP graphs."""
        check(lib().nano_hip_set_exact(self.h, 1 if on else 0))

    def exact_state(self) -> dict:
        """{'on', 'graphs' (exact-mode graphs instantiated), 'launches_per_step' (kernel nodes of the last enqueued exact step)}"""
        on, graphs, launches = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().nano_hip_exact_state(self.h, C.byref(on), C.byref(graphs), C.byref(launches)))
        return {"on": bool(on.value), "graphs": int(graphs.value), "launches_per_step": int(launches.value)}

    def set_phase_hook(self, fn=None):
        """fn(layer, phase) at the reference's twelve observation points of a strict-mode forward; None removes it."""
        self._phase_cb = PHASE_FN(lambda env, layer, phase: fn(int(layer), int(phase))) if fn else C.cast(None, PHASE_FN)
        check(lib().nano_hip_set_phase_hook(self.h, self._phase_cb, None))

    def time_classifier(self, batch: int = 1, iters: int = 20):
        ms, nbytes = C.c_float(0), C.c_uint64(0)
        check(lib().nano_hip_time_classifier(self.h, batch, iters, C.byref(ms), C.byref(nbytes)))
        return float(ms.value), int(nbytes.value)

    def time_classifier_in_step(self, batch: int = 1, pos: int = 0, iters: int = 20):
        """(ms per classifier launch measured inside whole decode steps [raw event span], algorithmic bytes per launch,
        ms of an empty event pair)"""
        ms, nbytes, empty = C.c_float(0), C.c_uint64(0), C.c_float(0)
        check(lib().nano_hip_time_classifier_in_step(self.h, batch, pos, iters, C.byref(ms), C.byref(nbytes), C.byref(empty)))
        return float(ms.value), int(nbytes.value), float(empty.value)

    def time_step(self, batch: int = 1, pos: int = 0, iters: int = 20) -> float:
        ms = C.c_float(0)
        check(lib().nano_hip_time_step(self.h, batch, pos, iters, C.byref(ms)))
        return float(ms.value)

    def kv_release(self, slot: int):
        """paged KV cache: give the slot's pages back to the pool"""
        check(lib().nano_hip_kv_release(self.h, slot))

    def kv_pages(self):
        """paged KV cache: (pages in use, pages in the pool)"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        check(lib().nano_hip_kv_pages(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def kv_fork(self, src: int, n_pos: int, dsts: Sequence[int]):
        """Make positions 0..n_pos-1 of every slot in dsts hold slot src's K / V rows (nano_hip_kv_fork): a copy on the contiguous
        cache; on the paged cache the full 64-position pages are shared (copy-on-write) and a partial last block is copied."""
        d = np.ascontiguousarray(dsts, np.uint32).reshape(-1)
        check(lib().nano_hip_kv_fork(self.h, src, n_pos, d, d.size))

    def kv_sharing(self):
        """paged KV cache: (pages with more than one owner, copy-on-write page copies made so far)"""
        a, b = C.c_uint32(0), C.c_uint64(0)
        check(lib().nano_hip_kv_sharing(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def kv_image_bytes(self, n_pos: int) -> int:
        """the size of the KV image of n_pos positions of this model (nano_hip_kv_image_bytes)"""
        return int(lib().nano_hip_kv_image_bytes(self.h, n_pos))

    def kv_save(self, slot: int, n_pos: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """nano_hip_kv_save: the KV image of positions 0..n_pos-1 of `slot` as a uint8 array (64-byte header + the rows, block-major);
        the slot is unchanged.  out: a contiguous uint8 array to write into (a view of its front is returned) instead of a new one."""
        img = np.empty(max(self.kv_image_bytes(n_pos), 64), np.uint8) if out is None else out
        assert img.dtype == np.uint8 and img.flags.c_contiguous
        n = C.c_size_t(0)
        check(lib().nano_hip_kv_save(self.h, slot, n_pos, img.ctypes.data, img.size, C.byref(n)))
        return img[:n.value]

    def kv_restore(self, slot: int, image, n_pos: Optional[int] = None):
        """nano_hip_kv_restore: positions 0..n_pos-1 (None: all) of the image into `slot` of this model, which may be another model opened
        from the same file than the one that saved it."""
        a = np.ascontiguousarray(np.frombuffer(image, np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else image, np.uint8).reshape(-1)
        check(lib().nano_hip_kv_restore(self.h, slot, a.ctypes.data if a.size else None, a.size, KV_ALL if n_pos is None else n_pos))

    def handoff_state(self):
        """(fusion bits in force, re-issues after a hand-off gave up, code bits of the last give-up)"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().nano_hip_handoff_state(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def set_fusion(self, mask: int):
        check(lib().nano_hip_set_fusion(self.h, mask))

    def debug_fault(self, flags: int):
        check(lib().nano_hip_debug_fault(self.h, flags))

    def stamps_begin(self):
        check(lib().nano_hip_stamps_begin(self.h))

    def stamps_read(self, cap: int = 512):
        """(stamps[n_launch, 2048, 8] uint64, kinds[n_launch]) of the steps run since stamps_begin()"""
        out = np.zeros((cap, 2048, 8), np.uint64); kinds = np.zeros(cap, np.uint32); n = C.c_uint32(0)
        check(lib().nano_hip_stamps_read(self.h, out.ctypes.data, kinds, cap, C.byref(n)))
        return out[:n.value], kinds[:n.value]

    def read_state(self, name: str, n: int, slot: int = 0, layer: int = 0, pos: int = 0) -> np.ndarray:
        out = np.empty(n, np.float32)
        check(lib().nano_hip_read_state(self.h, slot, STATE_IDS[name], layer, pos, out, n))
        return out


def desc_from_spec(spec) -> NanoModelDesc:
    """``nano_amd.modelfile.ModelSpec`` -> C struct."""
    return NanoModelDesc(spec.arch, spec.block_size, spec.vocab_size, spec.n_layer, spec.n_embd, spec.n_head,
                         spec.n_kv_head, spec.n_hidden, spec.shared_classifier, spec.head_dim, spec.quant_type,
                         spec.group_size)


def load_model_file(path: str, *, device: int = 0, max_seq_len: int = 512, max_batch: int = 1, kv_f16: Optional[bool] = None,
                    kv_paged: Optional[bool] = None, kv_fp8: Optional[bool] = None) -> DeviceModel:
    """Open a Nano ``.bin`` (header + tokenizer section + parameter blob) and upload it.
    The tokenizer section is skipped: this entry works on token ids."""
    from . import modelfile as mf
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    spec = mf.read_header(bytes(raw[:256]))
    tok_bytes = int(np.frombuffer(bytes(raw[256:260]), "<u4")[0])
    off = 256 + tok_bytes
    params = np.ascontiguousarray(raw[off:])         # private, aligned copy of the blob
    m = DeviceModel(desc_from_spec(spec), params, params.size, device=device, max_seq_len=max_seq_len, max_batch=max_batch, kv_f16=kv_f16, kv_paged=kv_paged, kv_fp8=kv_fp8)
    m.spec = spec
    return m


# ---- single operators ---------------------------------------------------------------------------------
def op_rmsnorm(x, w, device=0):
    x = np.ascontiguousarray(x, np.float32); out = np.empty_like(x)
    check(lib().nano_hip_op_rmsnorm(device, out, x, np.ascontiguousarray(w, np.float32), x.size)); return out


def op_matmul_f32(x, w, device=0):
    d, n = w.shape; out = np.empty(d, np.float32)
    check(lib().nano_hip_op_matmul_f32(device, out, np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32), n, d)); return out


def op_quantize_q80(x, gs, device=0):
    x = np.ascontiguousarray(x, np.float32)
    q = np.empty(x.size, np.int8); s = np.empty(x.size // gs, np.float32)
    check(lib().nano_hip_op_quantize_q80(device, x, x.size, gs, q, s)); return q, s


def op_matmul_q80(xq, xs, wq, ws, n, d, gs, device=0):
    out = np.empty(d, np.float32)
    check(lib().nano_hip_op_matmul_q80(device, out, np.ascontiguousarray(xq), np.ascontiguousarray(xs),
                                       np.ascontiguousarray(wq), np.ascontiguousarray(ws), n, d, gs)); return out


def op_quantize_q4k(x, device=0):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(((x.size + 255) // 256) * 160, np.uint8)
    check(lib().nano_hip_op_quantize_q4k(device, x, x.size, out)); return out


def op_matmul_q4k(x_blocks, w_blocks, n, d, device=0):
    out = np.empty(d, np.float32)
    check(lib().nano_hip_op_matmul_q4k(device, out, np.ascontiguousarray(x_blocks), np.ascontiguousarray(w_blocks), n, d)); return out


_FLAG = np.zeros(1, np.float32)         # stands for "a norm weight / attention partials are given" where only the shape is read


def _fused_shape(quant, kind, n, rows, nb, *, gs=0, norm=False, attn=None, ordered=False, use_gemm=False, resid_add=False) -> NanoFusedGemvDesc:
    """The shape part of a NanoFusedGemvDesc -- all a plan query reads.  norm: False, the address of the norm weight, or True (a query:
    null or not is all that is read, _FLAG stands for the weight); attn: None or (n_head, hd, nsplit[, address of the partials]), _FLAG likewise;
    resid_add: False, True (a query: _FLAG) or (address, stride) of the residual epilogue's addend (kind 1)."""
    d = NanoFusedGemvDesc()
    d.quant, d.gs, d.kind, d.n, d.nb, d.nseg = quant, gs, kind, n, nb, len(rows)
    for i, r in enumerate(rows):
        d.rows[i] = r
    if norm:
        d.norm_w = _FLAG.ctypes.data if norm is True else norm
    if attn is not None:
        d.attn_n_head, d.attn_hd, d.attn_nsplit = attn[:3]
        d.attn_part = attn[3] if len(attn) > 3 else _FLAG.ctypes.data
    if resid_add:
        d.resid_add, d.resid_add_stride = (_FLAG.ctypes.data, rows[0]) if resid_add is True else resid_add
    d.ordered = 1 if ordered else 0
    d.use_gemm = 1 if use_gemm else 0
    return d


def _plan_query(name, fields, words, desc, cus):
    """nano_hip_<name>_plan of a descriptor (a tuple: of the query's two descriptors): `words` output words, the first len(fields) of them named."""
    assert len(fields) <= words
    out = (C.c_uint32 * words)()
    descs = desc if isinstance(desc, tuple) else (desc,)
    check(getattr(lib(), f"nano_hip_{name}_plan")(*(C.byref(d) for d in descs), cus, out))
    return dict(zip(fields, (int(v) for v in out)))


def f32_gemv_plan(kind, n, rows, nb=1, *, norm=False, attn=None, resid_add=False, cus=256):
    """The FP32 launch the router issues for a fused-gemv shape (nano_hip_f32_gemv_plan; needs no GPU).  rows: the row count of each
    weight tensor (kind 2: two equal counts); attn = (n_head, hd, nsplit) for a launch that combines split-attention partials.
    Returns a dict of F32_PLAN_FIELDS; takes == 0: the router refuses the shape and every other entry is 0."""
    return _plan_query("f32_gemv", F32_PLAN_FIELDS, F32_PLAN_WORDS, _fused_shape(0x00, kind, n, rows, nb, norm=bool(norm), attn=attn, resid_add=bool(resid_add)), cus)


def f32_gemm_plan(kind, n, rows, nb=9, *, norm=False, attn=None, cus=256):
    """The FP32 MFMA GEMM launch the router issues for a fused-gemv shape of 9..64 sequences (nano_hip_f32_gemm_plan; needs no GPU);
    arguments as f32_gemv_plan.  Returns a dict of F32_GEMM_PLAN_FIELDS; a shape the GEMM refuses: the sliced route and zeros."""
    return _plan_query("f32_gemm", F32_GEMM_PLAN_FIELDS, len(F32_GEMM_PLAN_FIELDS), _fused_shape(0x00, kind, n, rows, nb, norm=bool(norm), attn=attn), cus)


def q80_gemv_plan(kind, n, rows, nb=1, *, gs=64, norm=False, attn=None, ordered=False, use_gemm=False, resid_add=False, cus=256):
    """The Q80 launch the router issues for a fused-gemv shape (nano_hip_q80_gemv_plan; needs no GPU).  rows: the row count of each
    weight tensor (kind 2: two equal counts); attn = (n_head, hd, nsplit) for a launch that combines split-attention partials.
    Returns a dict of Q80_PLAN_FIELDS; takes == 0: the router refuses the shape and every other entry is 0."""
    d = _fused_shape(0x80, kind, n, rows, nb, gs=gs, norm=bool(norm), attn=attn, ordered=ordered, use_gemm=use_gemm, resid_add=bool(resid_add))
    return _plan_query("q80_gemv", Q80_PLAN_FIELDS, Q80_PLAN_WORDS, d, cus)


def q80_gemv_plan_cw(kind, n, rows, nb=1, *, gs=64, norm=False, attn=None, ordered=False, use_gemm=False, resid_add=False, cus=256):
    """The last word of nano_hip_q80_gemv_plan for the arguments of q80_gemv_plan: 1 when the launch -- a residual launch behind split
    attention -- runs gemv_q80_slab_cw_kernel, the splits' weights made inside each wave; 0: every other launch, the table form included."""
    d = _fused_shape(0x80, kind, n, rows, nb, gs=gs, norm=bool(norm), attn=attn, ordered=ordered, use_gemm=use_gemm, resid_add=bool(resid_add))
    return _plan_query("q80_gemv", Q80_PLAN_FIELDS + ("cw",), Q80_PLAN_WORDS, d, cus)["cw"]


def q80_gemm_plan(kind, n, rows, nb=1, *, gs=64, norm=False, attn=None, ordered=False, use_gemm=False, cus=256):
    """The batched Q80 launch (G6 / G7 / G7K / GC / G2) the router issues for a fused-gemv shape (nano_hip_q80_gemm_plan; needs no GPU);
    arguments as q80_gemv_plan.  Returns a dict of Q80_GEMM_PLAN_FIELDS; a shape whose route ends in the GEMV kernels: the route and zeros."""
    d = _fused_shape(0x80, kind, n, rows, nb, gs=gs, norm=bool(norm), attn=attn, ordered=ordered, use_gemm=use_gemm)
    return _plan_query("q80_gemm", Q80_GEMM_PLAN_FIELDS, len(Q80_GEMM_PLAN_FIELDS), d, cus)


def q4k_gemv_plan(kind, n, rows, nb=1, *, norm=False, attn=None, resid_add=False, cus=256):
    """The Q4K launch the router issues for a fused-gemv shape (nano_hip_q4k_gemv_plan; needs no GPU).  rows: the row count of each
    weight tensor (kind 2: two equal counts); attn = (n_head, hd, nsplit) for a launch that combines split-attention partials.
    Returns a dict of Q4K_PLAN_FIELDS; takes == 0: the router refuses the shape and every other entry is 0."""
    return _plan_query("q4k_gemv", Q4K_PLAN_FIELDS, len(Q4K_PLAN_FIELDS), _fused_shape(0x42, kind, n, rows, nb, norm=bool(norm), attn=attn, resid_add=bool(resid_add)), cus)


def op_fused_gemv(quant, kind, n, weights, x=None, norm_w=None, *, gs=0, nb=1, resid=None, attn=None, use_gemm=False, ordered=False,
                  want_route=False, guard=None, partials=None, want_argmax=False, resid_add=None, device=0):
    """One fused decode GEMV launch exactly as a decode step issues it (nano_hip_op_fused_gemv).
    quant: 0x00 F32 / 0x80 Q80 / 0x42 Q4K; kind: 0 store, 1 residual add, 2 SwiGLU.
    weights: list of (w, ws_or_None, rows) -- F32 float[rows, n]; Q80 int8[rows*n] + float scales; Q4K uint8 blocks (no frame).
    x: [nb, n] fp32; resid: [nb, rows] old residual values (kind 1); attn = (part[nb, nsplit, n], ml[nb, n_head, nsplit, 2], n_head, hd).
    ordered: strict mode (the reference's ascending group order; bit-exact fp32 against the oracle); default: the fast path, whose
    Q80 kernels of group size 64 fold canonically (unit sums of 8 groups, units ascending -- tests/canon.py restates it).
    guard: None, or a float32 array [slots >= nb, stride >= rows_total] that IS the output buffer (slot b's result in [b, :rows_total];
    kind 1: it holds the residual stream there on entry) -- it goes to the device whole and comes back whole, so the caller sees whatever
    a launch wrote beyond its rows or its sequences; the returned out is that array.
    partials: None, or a float32 array [slots >= nb, pairs, 2] that IS the step's arg-max partials buffer: it goes to the device whole and
    comes back whole; the launch is asked for partials exactly where the step's classifier is (route.hip route_partials()) and then
    writes nb x ntiles (max, bits of the first row) pairs densely from the start of the buffer -- partials.reshape(-1, 2)[b * ntiles + t].
    want_argmax: behind the launch, the arg-max kernel as a greedy step builds it (from the partials where the launch wrote them).
    resid_add: None, or a float32 array [nb, stride >= rows] (kind 1): the residual epilogue's addend, out += (W act + resid_add[b, :rows]).
    Returns out[nb, rows_total]; with any of want_route / partials / want_argmax a tuple (out, route name if want_route,
    ntiles if partials is given -- 0: the launch was not asked --, argmax uint32[nb] if want_argmax)."""
    keep = []

    def held(v, dtype=None):
        v = np.ascontiguousarray(v, dtype); keep.append(v)
        return v

    if norm_w is not None:
        norm_w = held(norm_w, np.float32)
    if attn is not None:
        part, ml, n_head, hd = attn
        part, ml = held(part, np.float32), held(ml, np.float32)
    if resid_add is not None:
        resid_add = held(resid_add, np.float32)
        assert resid_add.ndim == 2 and resid_add.shape[0] == nb
    d = _fused_shape(quant, kind, n, [rows for _, _, rows in weights], nb, gs=gs, norm=norm_w is not None and norm_w.ctypes.data,
                     attn=None if attn is None else (n_head, hd, part.shape[-2], part.ctypes.data), ordered=ordered, use_gemm=use_gemm,
                     resid_add=resid_add is not None and (resid_add.ctypes.data, resid_add.shape[1]))
    for i, (w, ws, _) in enumerate(weights):
        d.w[i] = held(w).ctypes.data
        if ws is not None:
            d.ws[i] = held(ws, np.float32).ctypes.data
    rows_total = weights[0][2] if kind == 2 else sum(r for _, _, r in weights)
    if x is not None:
        d.x = held(x, np.float32).ctypes.data
    if attn is not None:
        d.attn_ml = ml.ctypes.data
    if guard is not None:
        assert resid is None and guard.dtype == np.float32 and guard.flags.c_contiguous and guard.ndim == 2
        out = guard
        d.out_slots, d.out_stride = guard.shape
    else:
        out = np.zeros((nb, rows_total), np.float32) if resid is None else np.array(resid, np.float32, copy=True).reshape(nb, rows_total)
    route = C.c_uint32(0xffffffff)
    d.route_out = C.cast(C.pointer(route), C.c_void_p)
    d.out = out.ctypes.data
    ntiles = C.c_uint32(0xffffffff)
    if partials is not None:
        assert partials.dtype == np.float32 and partials.flags.c_contiguous and partials.ndim == 3 and partials.shape[2] == 2
        d.tile_max, d.tile_slots, d.tile_pairs = partials.ctypes.data, partials.shape[0], partials.shape[1]
        d.ntiles_out = C.cast(C.pointer(ntiles), C.c_void_p)
    amax = np.full(nb, 0xffffffff, np.uint32)
    if want_argmax:
        d.argmax_out = amax.ctypes.data
    check(lib().nano_hip_op_fused_gemv(device, C.byref(d)))
    res = (out,)
    if want_route:
        res += (ROUTE_NAMES[route.value] if route.value < len(ROUTE_NAMES) else "?",)
    if partials is not None:
        res += (int(ntiles.value),)
    if want_argmax:
        res += (amax,)
    return res if len(res) > 1 else out


def _lora_desc(E, KD, rank, alpha, x, pairs, keep):
    def held(v, dtype=np.float32):
        v = np.ascontiguousarray(v, dtype); keep.append(v)
        return v
    x = held(x)
    d = NanoLoraOpDesc()
    d.E, d.KD, d.rank, d.alpha, d.nb = E, KD, rank, alpha, x.reshape(-1, E).shape[0]
    d.x = x.ctypes.data
    for i, (A, Bm) in enumerate(pairs):
        d.a[i], d.b[i] = held(A).ctypes.data, held(Bm).ctypes.data
    return d, held


def _inplace(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable
    return a.ctypes.data, a.size


def op_lora_qkv(x, norm_w, pairs, q, kraw, v, pos, *, KD, rank, alpha, S, v_bstride, device=0):
    """One lora_qkv launch as a step issues it (nano_hip_op_lora_qkv).  x [nb, E]; pairs = ((A_q, B_q), (A_k, B_k), (A_v, B_v)), A [rank, E],
    B [E | KD, rank]; q, kraw, v: float32 arrays changed IN PLACE, each going to the device whole and coming back whole -- q holds the nb
    rows of E floats from its start, kraw those of KD, v is a whole cache plane [slots, S, KD] with sequence b's row at flat offset
    b * v_bstride + pos[b] * KD (v_bstride = S * KD: a decode step; 0: a prefill chunk)."""
    keep = []
    x = np.ascontiguousarray(x, np.float32)
    d, held = _lora_desc(x.shape[-1], KD, rank, alpha, x, pairs, keep)
    d.S, d.v_bstride = S, v_bstride
    d.norm_w = held(norm_w).ctypes.data
    d.pos = held(pos, np.uint32).ctypes.data
    (d.q, d.q_floats), (d.kraw, d.k_floats), (d.v, d.v_floats) = _inplace(q), _inplace(kraw), _inplace(v)
    check(lib().nano_hip_op_lora_qkv(device, C.byref(d)))


def op_lora_o(xba, pair, o1, *, rank, alpha, device=0):
    """One lora_o launch as a step issues it (nano_hip_op_lora_o): o1[b] = (alpha / rank) B (A xba[b]).  o1: a float32 array changed IN
    PLACE (the nb rows of E floats from its start are written; it goes to the device whole and comes back whole)."""
    keep = []
    xba = np.ascontiguousarray(xba, np.float32)
    d, _ = _lora_desc(xba.shape[-1], 0, rank, alpha, xba, (pair,), keep)
    d.q, d.q_floats = _inplace(o1)
    check(lib().nano_hip_op_lora_o(device, C.byref(d)))


def lora_param_floats(n_layer, n_embd, kv_dim, rank) -> int:
    """floats of a LoRA module's parameter block (nano_hip_lora_param_floats; no device)"""
    return int(lib().nano_hip_lora_param_floats(n_layer, n_embd, kv_dim, rank))


def _lora_rows_desc(E, KD, x, adapters, row_adapter, keep, n_pairs):
    def held(v, dtype=np.float32):
        v = np.ascontiguousarray(v, dtype); keep.append(v)
        return v
    x = held(x)
    d = NanoLoraRowsOpDesc()
    d.E, d.KD, d.nb, d.n_adapters = E, KD, x.reshape(-1, E).shape[0], len(adapters)
    d.x = x.ctypes.data
    arr = (NanoLoraAdapter * max(len(adapters), 1))()
    for i, (rank, alpha, pairs) in enumerate(adapters):
        arr[i].rank, arr[i].alpha = rank, alpha
        assert len(pairs) == n_pairs
        for j, (A, Bm) in enumerate(pairs):
            arr[i].a[j], arr[i].b[j] = held(A).ctypes.data, held(Bm).ctypes.data
    keep.append(arr)
    d.adapters = arr
    d.row_adapter = held([NANO_LORA_NONE if v is None else v for v in row_adapter], np.uint32).ctypes.data
    return d, held


def op_lora_qkv_rows(x, norm_w, adapters, row_adapter, q, kraw, v, pos, *, KD, S, v_bstride, device=0):
    """One per-row lora_qkv launch as a step with a LoRA table issues it (nano_hip_op_lora_qkv_rows).  adapters = [(rank, alpha, ((A_q, B_q),
    (A_k, B_k), (A_v, B_v)))]; row_adapter[b] = the adapter of row b, or None: that row's q, kraw and v row are left untouched.  The rest as
    op_lora_qkv: q, kraw, v changed IN PLACE, going to the device whole and coming back whole."""
    keep = []
    x = np.ascontiguousarray(x, np.float32)
    d, held = _lora_rows_desc(x.shape[-1], KD, x, adapters, row_adapter, keep, 3)
    d.S, d.v_bstride = S, v_bstride
    d.norm_w = held(norm_w).ctypes.data
    d.pos = held(pos, np.uint32).ctypes.data
    (d.q, d.q_floats), (d.kraw, d.k_floats), (d.v, d.v_floats) = _inplace(q), _inplace(kraw), _inplace(v)
    check(lib().nano_hip_op_lora_qkv_rows(device, C.byref(d)))


def op_lora_o_rows(xba, adapters, row_adapter, o1, *, device=0):
    """One per-row lora_o launch (nano_hip_op_lora_o_rows): adapters = [(rank, alpha, ((A_o, B_o),))]; a row without an adapter gets -0.0 in
    every element of its o1 row.  o1: a float32 array changed IN PLACE."""
    keep = []
    xba = np.ascontiguousarray(xba, np.float32)
    d, _ = _lora_rows_desc(xba.shape[-1], 0, xba, adapters, row_adapter, keep, 1)
    d.q, d.q_floats = _inplace(o1)
    check(lib().nano_hip_op_lora_o_rows(device, C.byref(d)))


def op_attention_decode(q, k, pos, k_cache, v_cache, *, n_head, n_kv_head, hd, n_layer, layer, S, range_hint, rope_cos, rope_sin,
                        rope_qwen3, q_norm=None, k_norm=None, vraw=None, kv_half=False, chunk=False, nsplit=0, want_frag=False,
                        pt_rows=None, pool_rows=0, device=0):
    """One decode attention launch as a step issues it (nano_hip_op_attention_decode); chunk: the two passes of a prefill chunk.
    q [nb, n_head*hd], k [nb, kv_dim] raw rows; pos [nb]; caches float32 (kv_half 1 / True: float16 bit patterns; kv_half 2: uint8 e4m3fn
    bytes, taken and returned as uint8) contiguous [seqs, n_layer, S, kv_dim]
    or paged (pt_rows [seqs, pt_stride], pool_rows) [n_layer, pool_rows, kv_dim]; rope tables [S, hd/2].
    Returns dict(out [nb, n_head*hd], k_cache, v_cache (new arrays, same shape / dtype), plan (one dict; chunk: [pass 1, pass 2]),
    xf / xsf when want_frag)."""
    d = NanoAttnDecodeDesc()
    q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); pos = np.ascontiguousarray(pos, np.uint32)
    nb_ = q.shape[0]
    if int(kv_half) == 2 and (np.asarray(k_cache).dtype != np.uint8 or np.asarray(v_cache).dtype != np.uint8):
        raise TypeError("kv_half=2: the caches are uint8 arrays of e4m3fn bytes")
    cdt = np.uint8 if int(kv_half) == 2 else np.float16 if kv_half else np.float32
    kc = np.array(k_cache, cdt, copy=True, order="C"); vc = np.array(v_cache, cdt, copy=True, order="C")
    rope_cos = np.ascontiguousarray(rope_cos, np.float32); rope_sin = np.ascontiguousarray(rope_sin, np.float32)
    out = np.zeros((nb_, n_head * hd), np.float32)
    plan = np.zeros((2, len(ATTN_PLAN_FIELDS)), np.uint32)
    keep = [q, k, pos, kc, vc, rope_cos, rope_sin, out, plan]
    d.nb, d.n_head, d.n_kv_head, d.hd, d.n_layer, d.layer, d.S = nb_, n_head, n_kv_head, hd, n_layer, layer, S
    d.range_hint, d.nsplit, d.rope_qwen3, d.kv_half, d.chunk, d.want_frag = range_hint, nsplit, int(rope_qwen3), int(kv_half), int(chunk), int(want_frag)
    d.q, d.k, d.pos, d.k_cache, d.v_cache, d.out, d.plan = (x.ctypes.data for x in (q, k, pos, kc, vc, out, plan))
    d.rope_cos, d.rope_sin = rope_cos.ctypes.data, rope_sin.ctypes.data
    if q_norm is not None:
        q_norm = np.ascontiguousarray(q_norm, np.float32); k_norm = np.ascontiguousarray(k_norm, np.float32); keep += [q_norm, k_norm]
        d.q_norm, d.k_norm = q_norm.ctypes.data, k_norm.ctypes.data
    if vraw is not None:
        vraw = np.ascontiguousarray(vraw, np.float32); keep.append(vraw); d.vraw = vraw.ctypes.data
    if pt_rows is not None:
        pt_rows = np.ascontiguousarray(pt_rows, np.uint32); keep.append(pt_rows)
        d.pt_rows, d.pt_stride, d.pool_rows = pt_rows.ctypes.data, pt_rows.shape[-1], pool_rows
    xf = xsf = None
    if want_frag:
        tiles, ng = (nb_ + 15) // 16, n_head * hd // 64
        xf = np.zeros((tiles, ng, 1024), np.int8); xsf = np.zeros((tiles, ng, 16), np.float32); keep += [xf, xsf]
        d.xf, d.xsf = xf.ctypes.data, xsf.ctypes.data
    check(lib().nano_hip_op_attention_decode(device, C.byref(d)))
    plans = [dict(zip(ATTN_PLAN_FIELDS, (int(v) for v in row))) for row in plan]
    res = {"out": out, "k_cache": kc, "v_cache": vc, "plan": plans if chunk else plans[0]}
    if want_frag:
        res["xf"], res["xsf"] = xf, xsf
    return res


def _attn_shape(n_head, n_kv_head, hd, *, range_hint, nsplit=0, rope_qwen3=True, qk_norm=True, n_layer=1, layer=0, S=None) -> NanoAttnDecodeDesc:
    """The shape part of a one-sequence NanoAttnDecodeDesc -- all the fused plan query reads (qk_norm: _FLAG stands for the two weights)."""
    d = NanoAttnDecodeDesc()
    d.nb, d.n_head, d.n_kv_head, d.hd, d.n_layer, d.layer = 1, n_head, n_kv_head, hd, n_layer, layer
    d.S = max(range_hint, 1) if S is None else S
    d.range_hint, d.nsplit, d.rope_qwen3 = range_hint, nsplit, int(bool(rope_qwen3))
    if qk_norm:
        d.q_norm = d.k_norm = _FLAG.ctypes.data
    return d


def qkv_attn_fused_plan(quant, n, n_head, n_kv_head, hd, *, range_hint=64, nsplit=0, gs=None, rope_qwen3=None, qk_norm=None, ordered=False,
                        use_gemm=False, cus=256):
    """The fused q | k | v + attention launch a one-sequence step issues (nano_hip_qkv_attn_fused_plan; needs no GPU) for a projection of row
    length n onto n_head / n_kv_head heads of hd, and decode attention with nsplit splits (0: the step's own choice) over range_hint rows.
    rope_qwen3 / qk_norm default to what the format's models have (Q80, Q4K: Qwen3's; FP32: Nano's plain attention).
    Returns a dict of QKV_ATTN_FUSED_PLAN_FIELDS; takes == 0: the step issues the two plain launches and every other entry is 0."""
    qwen = quant != 0x00
    g = _fused_shape(quant, 0, n, [n_head * hd, n_kv_head * hd, n_kv_head * hd], 1, gs=(64 if quant == 0x80 else 0) if gs is None else gs,
                     norm=True, ordered=ordered, use_gemm=use_gemm)
    a = _attn_shape(n_head, n_kv_head, hd, range_hint=range_hint, nsplit=nsplit, rope_qwen3=qwen if rope_qwen3 is None else rope_qwen3,
                    qk_norm=qwen if qk_norm is None else qk_norm)
    return _plan_query("qkv_attn_fused", QKV_ATTN_FUSED_PLAN_FIELDS, len(QKV_ATTN_FUSED_PLAN_FIELDS), (g, a), cus)


def wo_w13_fused_plan(n_wo, n_embd, n_hidden, *, attn=None, gs=64, ordered=False, cus=256):
    """The fused Wo + W1|W3 launch a one-sequence Q80 step issues (nano_hip_wo_w13_fused_plan; needs no GPU): Wo [n_embd, n_wo], W1 and W3
    [n_hidden, n_embd]; attn = (n_head, hd, nsplit) when Wo combines split-attention partials.
    Returns a dict of WO_W13_FUSED_PLAN_FIELDS; takes == 0: the step issues the two plain launches and every other entry is 0."""
    a = _fused_shape(0x80, 1, n_wo, [n_embd], 1, gs=gs, attn=attn, ordered=ordered)
    b = _fused_shape(0x80, 2, n_embd, [n_hidden, n_hidden], 1, gs=gs, norm=True, ordered=ordered)
    return _plan_query("wo_w13_fused", WO_W13_FUSED_PLAN_FIELDS, len(WO_W13_FUSED_PLAN_FIELDS), (a, b), cus)


def op_qkv_attn_fused(quant, n, weights, x, norm_w, pos, k_cache, v_cache, *, n_head, n_kv_head, hd, S, range_hint, rope_cos, rope_sin,
                      rope_qwen3, q_norm=None, k_norm=None, nsplit=0, gs=0, n_layer=1, layer=0, layer1=1, tick0=0, hand_init=None, device=0):
    """One fused q | k | v + attention launch exactly as a one-sequence step issues it (nano_hip_op_qkv_attn_fused).
    weights: [(wq, ws, rows), (wk, ..), (wv, ..)] as op_fused_gemv takes them; x [n], norm_w [n]; pos: the position; caches float32
    [n_layer, S, kv_dim] (copied; returned whole); hand_init: None or uint64[q_dim + 2 kv_dim] granules (tag << 32 | value bits).
    Returns dict(out [q_dim] head outputs (nsplit > 1: the combined partials), k_cache, v_cache, q [q_dim], k [kv_dim] raw rows as stored,
    part [nsplit, q_dim] and ml [n_head, nsplit, 2] when nsplit > 1, plan (dict of QKV_ATTN_FUSED_PLAN_FIELDS), err (the error word)).
    Raises NanoHipError for a shape the plan refuses (before any launch) and when a consumer gave up its wait."""
    keep = []

    def held(v, dtype=None):
        v = np.ascontiguousarray(v, dtype); keep.append(v)
        return v

    QD, KD = n_head * hd, n_kv_head * hd
    norm_w = held(norm_w, np.float32)
    g = _fused_shape(quant, 0, n, [r for _, _, r in weights], 1, gs=gs, norm=norm_w.ctypes.data)
    for i, (w, ws, _) in enumerate(weights):
        g.w[i] = held(w).ctypes.data
        if ws is not None:
            g.ws[i] = held(ws, np.float32).ctypes.data
    g.x = held(x, np.float32).ctypes.data
    qk = np.zeros(QD + KD, np.float32)
    g.out = qk.ctypes.data
    a = _attn_shape(n_head, n_kv_head, hd, range_hint=range_hint, nsplit=nsplit, rope_qwen3=rope_qwen3, qk_norm=False, n_layer=n_layer, layer=layer, S=S)
    if q_norm is not None:
        a.q_norm, a.k_norm = held(q_norm, np.float32).ctypes.data, held(k_norm, np.float32).ctypes.data
    kc = np.array(k_cache, np.float32, copy=True, order="C"); vc = np.array(v_cache, np.float32, copy=True, order="C")
    assert kc.size == n_layer * S * KD and vc.size == kc.size
    out = np.zeros(QD, np.float32)
    a.pos = held(np.array([pos], np.uint32)).ctypes.data
    a.rope_cos, a.rope_sin = held(rope_cos, np.float32).ctypes.data, held(rope_sin, np.float32).ctypes.data
    a.k_cache, a.v_cache, a.out = kc.ctypes.data, vc.ctypes.data, out.ctypes.data
    part = np.zeros((8, QD), np.float32); ml = np.zeros(n_head * 8 * 2, np.float32)      # room for any split count the launch takes
    plan = np.zeros(len(QKV_ATTN_FUSED_PLAN_FIELDS), np.uint32); err = np.zeros(1, np.uint32)
    d = NanoQkvAttnFusedDesc()
    d.qkv, d.attn, d.layer1, d.tick0 = C.pointer(g), C.pointer(a), layer1, tick0
    if hand_init is not None:
        hand_init = held(hand_init, np.uint64)
        assert hand_init.size == QD + 2 * KD
        d.hand_init = hand_init.ctypes.data
    d.part_out, d.ml_out, d.plan_out, d.err_out = part.ctypes.data, ml.ctypes.data, plan.ctypes.data, err.ctypes.data
    check(lib().nano_hip_op_qkv_attn_fused(device, C.byref(d)))
    p = dict(zip(QKV_ATTN_FUSED_PLAN_FIELDS, (int(v) for v in plan)))
    res = {"out": out, "k_cache": kc, "v_cache": vc, "q": qk[:QD], "k": qk[QD:], "plan": p, "err": int(err[0])}
    ran = p["n_attn"] // n_head if p["takes"] else 0
    if ran > 1:
        res["part"] = part.reshape(-1)[:ran * QD].reshape(ran, QD)
        res["ml"] = ml[:n_head * ran * 2].reshape(n_head, ran, 2)
    return res


def op_wo_w13_fused(n_wo, wo, w1, w3, resid, norm_w, *, x=None, attn=None, gs=64, layer1=1, tick0=0, hand_init=None, device=0):
    """One fused Wo + W1|W3 launch exactly as a one-sequence Q80 step issues it (nano_hip_op_wo_w13_fused).
    wo = (w, ws, n_embd), w1 / w3 = (w, ws, n_hidden) as op_fused_gemv takes them; x [n_wo] the attention output, or attn = (part[nsplit, n_wo],
    ml[n_head, nsplit, 2], n_head, hd); resid [n_embd] the residual stream on entry; norm_w [n_embd] W1|W3's rmsnorm weight;
    hand_init: None or uint64[n_embd] granules.  Returns dict(x [n_embd] the residual stream Wo leaves, hb [n_hidden], plan, err)."""
    keep = []

    def held(v, dtype=None):
        v = np.ascontiguousarray(v, dtype); keep.append(v)
        return v

    E, Hd = wo[2], w1[2]
    assert w3[2] == Hd
    norm_w = held(norm_w, np.float32)
    if attn is not None:
        part, ml, n_head, hd = attn
        part, ml = held(part, np.float32), held(ml, np.float32)
    a = _fused_shape(0x80, 1, n_wo, [E], 1, gs=gs, attn=None if attn is None else (n_head, hd, part.shape[-2], part.ctypes.data))
    b = _fused_shape(0x80, 2, E, [Hd, Hd], 1, gs=gs, norm=norm_w.ctypes.data)
    a.w[0], a.ws[0] = held(wo[0]).ctypes.data, held(wo[1], np.float32).ctypes.data
    for i, t in enumerate((w1, w3)):
        b.w[i], b.ws[i] = held(t[0]).ctypes.data, held(t[1], np.float32).ctypes.data
    if x is not None:
        a.x = held(x, np.float32).ctypes.data
    if attn is not None:
        a.attn_ml = ml.ctypes.data
    xo = np.array(resid, np.float32, copy=True).reshape(E); hb = np.zeros(Hd, np.float32)
    a.out, b.out = xo.ctypes.data, hb.ctypes.data
    plan = np.zeros(len(WO_W13_FUSED_PLAN_FIELDS), np.uint32); err = np.zeros(1, np.uint32)
    d = NanoWoW13FusedDesc()
    d.wo, d.w13, d.layer1, d.tick0 = C.pointer(a), C.pointer(b), layer1, tick0
    if hand_init is not None:
        hand_init = held(hand_init, np.uint64)
        assert hand_init.size == E
        d.hand_init = hand_init.ctypes.data
    d.plan_out, d.err_out = plan.ctypes.data, err.ctypes.data
    check(lib().nano_hip_op_wo_w13_fused(device, C.byref(d)))
    return {"x": xo, "hb": hb, "plan": dict(zip(WO_W13_FUSED_PLAN_FIELDS, (int(v) for v in plan))), "err": int(err[0])}


def op_rope(head, fcr, fci, qwen3, device=0):
    h = np.array(head, np.float32, copy=True)
    check(lib().nano_hip_op_rope(device, h, h.size, np.ascontiguousarray(fcr, np.float32), np.ascontiguousarray(fci, np.float32), int(qwen3))); return h


def op_attention(q, k_cache, v_cache, n_head, n_kv_head, head_dim, device=0):
    rng = k_cache.shape[0]
    out = np.empty(n_head * head_dim, np.float32)
    check(lib().nano_hip_op_attention(device, out, np.ascontiguousarray(q, np.float32), np.ascontiguousarray(k_cache, np.float32),
                                      np.ascontiguousarray(v_cache, np.float32), n_head, n_kv_head, head_dim, rng)); return out


def op_exact_rmsnorm(x, w, device=0):
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
    out = np.empty_like(x)
    check(lib().nano_hip_op_exact_rmsnorm(device, out, x, w, x.size)); return out


def op_exact_attention(q, k_cache, v_cache, n_head, n_kv_head, head_dim, rng=None, is_causal=True, long_form=False, device=0):
    """exact mode's attention (infer.c:842-879) of one sequence: caches [S][kv_dim]; is_causal: rows 0 .. rng - 1, else all S rows;
    long_form: the three-launch form an exact step keeps where att[S] does not fit the one-launch kernel's LDS."""
    q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k_cache, np.float32); v = np.ascontiguousarray(v_cache, np.float32)
    out = np.empty(n_head * head_dim, np.float32)
    d = NanoExactAttnDesc()
    d.n_head, d.n_kv_head, d.hd, d.S = n_head, n_kv_head, head_dim, k.shape[0]
    d.range = k.shape[0] if rng is None else rng
    d.is_causal, d.long_form = int(bool(is_causal)), int(bool(long_form))
    d.q, d.k_cache, d.v_cache, d.out = q.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data
    check(lib().nano_hip_op_exact_attention(device, C.byref(d))); return out


def op_swiglu(hb, hb2, device=0):
    h = np.array(hb, np.float32, copy=True)
    check(lib().nano_hip_op_swiglu(device, h, np.ascontiguousarray(hb2, np.float32), h.size)); return h


def op_score_rows(logits, targets=None, device=0) -> np.ndarray:
    """The row-statistics kernel alone (nano_hip_op_score_rows): logits [rows, V] float32, targets [rows] or None (each row's own
    arg-max); one TOKEN_SCORE_DTYPE entry per row.  Device only: without a GPU this raises."""
    l = np.ascontiguousarray(logits, np.float32)
    if l.ndim != 2:
        raise ValueError("logits must be [rows, V]")
    g = None if targets is None else np.ascontiguousarray(targets, np.uint32).reshape(-1)
    if g is not None and g.size != l.shape[0]:
        raise ValueError(f"{l.shape[0]} rows but {g.size} targets")
    out = np.zeros(l.shape[0], TOKEN_SCORE_DTYPE)
    check(lib().nano_hip_op_score_rows(device, l.ctypes.data, l.shape[0], l.shape[1], None if g is None else g.ctypes.data, out.ctypes.data))
    return out


def op_topk_rows(logits, k, targets=None, device=0):
    """The row statistics and the top-k selection alone (nano_hip_op_topk_rows): logits [rows, V] float32, targets [rows] or None.
    Returns (scores TOKEN_SCORE_DTYPE[rows], top TOP_ENTRY_DTYPE[rows, k], most probable first).  Device only: no host path."""
    l = np.ascontiguousarray(logits, np.float32)
    if l.ndim != 2:
        raise ValueError("logits must be [rows, V]")
    g = None if targets is None else np.ascontiguousarray(targets, np.uint32).reshape(-1)
    if g is not None and g.size != l.shape[0]:
        raise ValueError(f"{l.shape[0]} rows but {g.size} targets")
    out = np.zeros(l.shape[0], TOKEN_SCORE_DTYPE)
    top = np.zeros((l.shape[0], max(k, 1)), TOP_ENTRY_DTYPE)
    check(lib().nano_hip_op_topk_rows(device, l.ctypes.data, l.shape[0], l.shape[1], k, None if g is None else g.ctypes.data,
                                      out.ctypes.data, top.ctypes.data))
    return out, top


def op_pool_rows(x, w_final, seg_count, pooling="last", normalize=True, dim=0, pass_cap=64, device=0, guard=0):
    """The pool kernel alone (nano_hip_op_pool_rows): x [rows, n_embd] float32 residual rows, segment after segment; w_final [n_embd];
    seg_count the segments' row counts.  Returns float32 [n_segs, dim or n_embd].  guard > 0: (out, tail) where tail is `guard` words of
    the output buffer behind the result, filled with 0xa5a5a5a5 before the call.  Device only: no host path."""
    xv = np.ascontiguousarray(x, np.float32)
    if xv.ndim != 2:
        raise ValueError("x must be [rows, n_embd]")
    w = np.ascontiguousarray(w_final, np.float32).reshape(-1)
    c = np.ascontiguousarray(seg_count, np.uint32).reshape(-1)
    if w.size != xv.shape[1]:
        raise ValueError(f"n_embd {xv.shape[1]} but {w.size} weights")
    d = dim or xv.shape[1]
    buf = np.full(c.size * d + guard, 0xA5A5A5A5, np.uint32)
    p = NanoHipPoolParams(_pooling(pooling), int(normalize), dim, 0)
    xp = xv if xv.size else np.zeros((1, xv.shape[1]), np.float32)
    check(lib().nano_hip_op_pool_rows(device, xp.ctypes.data, xv.shape[0], xv.shape[1], w.ctypes.data, c.ctypes.data, c.size, C.byref(p), pass_cap, buf.ctypes.data))
    out = buf[:c.size * d].view(np.float32).reshape(c.size, d)
    return (out, buf[c.size * d:]) if guard else out


def op_lookup_step(history, fed=(), amax=(), *, left, max_draft=7, ngram_max=3, ngram_min=1, stop_token=None, seq_limit=1 << 30, device=0):
    """lookup_step_kernel alone (nano_hip_op_lookup_step): behind a step that fed `fed` and left the row arg-maxes `amax` (both empty: no
    step has run yet).  Returns (record dict of LOOKUP_RECORD_FIELDS, the history with the emitted ids appended, next tokens, next
    positions -- the latter two all 16 words, 0xffffffff from nb_next on)."""
    h = np.ascontiguousarray(history, np.uint32).reshape(-1)
    f = np.ascontiguousarray(fed, np.uint32).reshape(-1)
    g = np.ascontiguousarray(amax, np.uint32).reshape(-1)
    if f.size != g.size:
        raise ValueError(f"{f.size} fed ids but {g.size} arg-maxes")
    buf = np.full(h.size + 16, 0xFFFFFFFF, np.uint32)
    buf[:h.size] = h
    p = NanoHipLookupParams(max_draft, ngram_max, ngram_min, LOOKUP_NO_STOP if stop_token is None else stop_token, 0)
    rec, nt, npos = np.zeros(8, np.uint32), np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    check(lib().nano_hip_op_lookup_step(device, buf.ctypes.data, h.size, f.ctypes.data if f.size else None, g.ctypes.data if g.size else None, f.size,
                                        C.byref(p), left, min(seq_limit, 0xFFFFFFFF), rec.ctypes.data, nt.ctypes.data, npos.ctypes.data))
    r = dict(zip(LOOKUP_RECORD_FIELDS, (int(v) for v in rec)))
    return r, buf[:r["n"]].copy() if h.size <= r["n"] <= buf.size else buf, nt, npos


def lookup_rows_plan(n, nb_next, max_seq_len):
    """nano_hip_lookup_rows_plan (device-free): the pass of a round.  Returns (order of the live sequences, row_start per sequence --
    0xffffffff: dead --, list of (hint, rows) groups)."""
    a = np.ascontiguousarray(n, np.uint32).reshape(-1)
    b = np.ascontiguousarray(nb_next, np.uint32).reshape(-1)
    if a.size != b.size:
        raise ValueError(f"{a.size} lengths but {b.size} row counts")
    B = a.size
    order, start, gh, gr = (np.zeros(max(B, 1), np.uint32) for _ in range(4))
    ng = C.c_uint32(0)
    check(lib().nano_hip_lookup_rows_plan(a.ctypes.data if B else None, b.ctypes.data if B else None, B, max_seq_len, order.ctypes.data, start.ctypes.data,
                                          gh.ctypes.data, gr.ctypes.data, C.byref(ng)))
    live = int(np.count_nonzero(b))
    return order[:live].tolist(), start[:B].tolist(), [(int(gh[g]), int(gr[g])) for g in range(ng.value)]


def op_lookup_rows_round(histories, left, slots, fed=(), amax=(), row_start=None, nb=None, *, max_draft=7, ngram_max=3, ngram_min=1, stop_token=None,
                         seq_limit=1 << 30, max_seq_len=1 << 30, device=0):
    """The two between-rounds launches of lookup_rows.hip alone (nano_hip_op_lookup_rows_round): behind a pass that fed `fed` and left the
    row arg-maxes `amax` (pass order), sequence i's rows being row_start[i] .. row_start[i] + nb[i] (None: no pass has run yet).
    Returns (list of record dicts, list of histories with the emitted ids appended, next tokens, next positions, next slots -- each
    len(histories) * 16 words, 0xffffffff beyond the pass's rows --, row_start per sequence)."""
    hs = [np.ascontiguousarray(h, np.uint32).reshape(-1) for h in histories]
    B = len(hs)
    f = np.ascontiguousarray(fed, np.uint32).reshape(-1)
    g = np.ascontiguousarray(amax, np.uint32).reshape(-1)
    if f.size != g.size:
        raise ValueError(f"{f.size} fed ids but {g.size} arg-maxes")
    rs = np.ascontiguousarray([0xFFFFFFFF] * B if row_start is None else row_start, np.uint32).reshape(-1)
    cnt = np.ascontiguousarray([0] * B if nb is None else nb, np.uint32).reshape(-1)
    nn = np.ascontiguousarray([h.size for h in hs], np.uint32)
    lf = np.ascontiguousarray(left, np.uint32).reshape(-1)
    sl = np.ascontiguousarray(slots, np.uint32).reshape(-1)
    if not (rs.size == cnt.size == lf.size == sl.size == B):
        raise ValueError("one entry per sequence is needed in left, slots, row_start and nb")
    bufs = []
    for h in hs:
        buf = np.full(h.size + 16, 0xFFFFFFFF, np.uint32)
        buf[:h.size] = h
        bufs.append(buf)
    hp = (C.c_void_p * max(B, 1))(*[b.ctypes.data for b in bufs])
    p = NanoHipLookupParams(max_draft, ngram_max, ngram_min, LOOKUP_NO_STOP if stop_token is None else stop_token, 0)
    rec = np.zeros((max(B, 1), 8), np.uint32)
    nt, npos, nsl = (np.zeros(max(B, 1) * 16, np.uint32) for _ in range(3))
    rso = np.zeros(max(B, 1), np.uint32)
    check(lib().nano_hip_op_lookup_rows_round(device, B, hp, nn.ctypes.data, lf.ctypes.data, sl.ctypes.data, f.ctypes.data if f.size else None,
                                              g.ctypes.data if g.size else None, f.size, rs.ctypes.data, cnt.ctypes.data, C.byref(p),
                                              min(seq_limit, 0xFFFFFFFF), min(max_seq_len, 0xFFFFFFFF), rec.ctypes.data, nt.ctypes.data, npos.ctypes.data,
                                              nsl.ctypes.data, rso.ctypes.data))
    recs = [dict(zip(LOOKUP_RECORD_FIELDS, (int(v) for v in rec[i]))) for i in range(B)]
    out_h = [bufs[i][:recs[i]["n"]].copy() if hs[i].size <= recs[i]["n"] <= bufs[i].size else bufs[i] for i in range(B)]
    return recs, out_h, nt, npos, nsl, rso[:B].tolist()


def op_draft_round(history, fed=(), amax=(), *, left, dn=0, max_draft=4, stop_token=None, seq_limit=1 << 30, device=0):
    """draft_round_kernel alone (nano_hip_op_draft_round): its STAGE role on fed[1:], then its ACCEPT role behind a round that fed `fed` and
    left the row arg-maxes `amax` (both empty: no round has run yet); dn = positions the draft held before it.  Returns (record dict of
    DRAFT_RECORD_FIELDS, the history with the emitted ids appended, next tokens, next positions -- the latter two all 16 words: row 0 and
    the next round's positions; next tokens 1 .. len(fed)-1 are what STAGE put there, every other word is 0xffffffff)."""
    h = np.ascontiguousarray(history, np.uint32).reshape(-1)
    f = np.ascontiguousarray(fed, np.uint32).reshape(-1)
    g = np.ascontiguousarray(amax, np.uint32).reshape(-1)
    if f.size != g.size:
        raise ValueError(f"{f.size} fed ids but {g.size} arg-maxes")
    buf = np.full(h.size + 16, 0xFFFFFFFF, np.uint32)
    buf[:h.size] = h
    p = NanoHipDraftParams(max_draft, LOOKUP_NO_STOP if stop_token is None else stop_token, 0, 0)
    rec, nt, npos = np.zeros(8, np.uint32), np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    check(lib().nano_hip_op_draft_round(device, buf.ctypes.data, h.size, f.ctypes.data if f.size else None, g.ctypes.data if g.size else None, f.size,
                                        C.byref(p), left, min(seq_limit, 0xFFFFFFFF), dn, rec.ctypes.data, nt.ctypes.data, npos.ctypes.data))
    r = dict(zip(DRAFT_RECORD_FIELDS, (int(v) for v in rec)))
    return r, buf[:r["n"]].copy() if h.size <= r["n"] <= buf.size else buf, nt, npos


def op_argmax(x, device=0):
    i = C.c_uint32(0)
    x = np.ascontiguousarray(x, np.float32)
    check(lib().nano_hip_op_argmax(device, x, x.size, C.byref(i))); return int(i.value)


# ---- host C engine (include/nano_infer_abi.h) -----------------------------------------------------------
class Engine:
    """The reference's engine API (llm_context_init / generate_next_token / sessions) as implemented by
    the host C code of this library; ids in, ids out (no tokenizer linked in the stand-alone library)."""

    def __init__(self, path: str, max_seq_len: int = 512, rep_pen: float = 1.0, temperature: float = 0.0,
                 top_p: float = 1.0, top_k: int = 0, seed: int = 39, device: int = 0, max_batch: int = 1,
                 lora_path: Optional[str] = None):
        L = lib()
        vp = C.c_void_p
        L.nano_set_device.argtypes = [C.c_int]; L.nano_set_max_batch.argtypes = [C.c_uint32]
        L.llm_context_init.restype = vp
        L.llm_context_init.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64]
        L.llm_context_free.argtypes = [vp]
        L.generate_next_token.restype = C.c_uint32
        L.generate_next_token.argtypes = [vp, u32p, C.c_uint32, C.c_int]
        L.nano_session_init_ids.restype = vp
        L.nano_session_init_ids.argtypes = [vp, u32p, C.c_uint32, C.c_uint32]
        L.nano_session_step_ids.restype = C.c_int32
        L.nano_session_step_ids.argtypes = [vp, vp]
        L.llm_session_free.argtypes = [vp]
        L.nano_forward_batch.restype = C.c_int
        L.nano_forward_batch.argtypes = [vp, u32p, u32p, C.c_uint32, vp, vp]
        L.nano_score_ids.restype = C.c_int
        L.nano_score_ids.argtypes = [vp, u32p, C.c_uint32, vp, vp, C.POINTER(C.c_double)]
        L.nano_forward_batch_sample.restype = C.c_int
        L.nano_forward_batch_sample.argtypes = [vp, u32p, u32p, C.c_uint32, vp, vp, vp, vp]
        L.build_sampler.restype = C.POINTER(SamplerC)
        L.build_sampler.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64]
        L.free_sampler.argtypes = [C.POINTER(SamplerC)]
        L.nano_set_device(device)
        L.nano_set_max_batch(max_batch)
        self.L = L
        self.ctx = L.llm_context_init(path.encode(), lora_path.encode() if lora_path else None, max_seq_len, rep_pen, temperature, top_p, top_k, seed)
        self.max_seq_len = max_seq_len

    def close(self):
        if self.ctx:
            self.L.llm_context_free(self.ctx); self.ctx = None

    def next_token(self, ids: np.ndarray, pos: int, is_prefilling: int) -> int:
        return int(self.L.generate_next_token(self.ctx, ids, pos, is_prefilling))

    def generate(self, prompt: Sequence[int], n_decode: int) -> np.ndarray:
        """Greedy/sampled generation through generate_next_token, like the reference's session loop."""
        n_prompt = len(prompt)
        ids = np.zeros(n_prompt + n_decode + 1, np.uint32)
        ids[:n_prompt] = prompt
        for pos in range(n_prompt - 1):
            self.next_token(ids, pos, 1)
        for i in range(n_decode):
            pos = n_prompt - 1 + i
            ids[pos + 1] = self.next_token(ids, pos, 0)
        return ids[:n_prompt + n_decode]

    def build_sampler(self, vocab_size: int, rep_pen: float, temperature: float, top_p: float, seed: int, top_k: int = 0):
        """A Sampler of the engine (build_sampler); free it with free_sampler.  .contents.rng_state is its generator state."""
        return self.L.build_sampler(vocab_size, rep_pen, temperature, top_p, top_k, seed)

    def free_sampler(self, s):
        self.L.free_sampler(s)

    def forward_batch(self, tokens: Sequence[int], pos: Sequence[int], want_logits: bool = True, vocab: int = 0):
        """nano_forward_batch: one decode step of B sequences; logits [B][vocab] (or arg-max ids)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        p = np.ascontiguousarray(pos, np.uint32).reshape(-1)
        logits = np.empty((t.size, vocab), np.float32) if want_logits else None
        amax = None if want_logits else np.empty(t.size, np.uint32)
        check(self.L.nano_forward_batch(self.ctx, t, p, t.size, logits.ctypes.data if want_logits else None,
                                        None if want_logits else amax.ctypes.data))
        return logits if want_logits else amax

    def score_ids(self, ids: Sequence[int]):
        """nano_score_ids: (logprobs[n - 1] float32, argmax[n - 1] uint32, nll_sum) of ids[1:] given what precedes each."""
        t = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        n = max(t.size - 1, 0)
        lp, am, nll = np.zeros(n, np.float32), np.zeros(n, np.uint32), C.c_double(0.0)
        check(self.L.nano_score_ids(self.ctx, t, t.size, lp.ctypes.data, am.ctypes.data, C.byref(nll)))
        return lp, am, float(nll.value)

    def score_ids_topk(self, ids: Sequence[int], k: int):
        """nano_score_ids_topk: score_ids() plus (top_ids uint32[n - 1, k], top_logprobs float32[n - 1, k]), most probable first."""
        t = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        n = max(t.size - 1, 0)
        lp, am, nll = np.zeros(n, np.float32), np.zeros(n, np.uint32), C.c_double(0.0)
        ti, tl = np.zeros((n, k), np.uint32), np.zeros((n, k), np.float32)
        check(self.L.nano_score_ids_topk(self.ctx, t.ctypes.data, t.size, k, lp.ctypes.data, am.ctypes.data, ti.ctypes.data, tl.ctypes.data, C.byref(nll)))
        return lp, am, float(nll.value), ti, tl

    def forward_batch_topk(self, tokens: Sequence[int], pos: Sequence[int], k: int):
        """nano_forward_batch_topk: one decode step of B sequences -> (top_ids uint32[B, k], top_logprobs float32[B, k], argmax uint32[B])."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        p = np.ascontiguousarray(pos, np.uint32).reshape(-1)
        ti, tl, am = np.zeros((t.size, k), np.uint32), np.zeros((t.size, k), np.float32), np.zeros(t.size, np.uint32)
        check(self.L.nano_forward_batch_topk(self.ctx, t.ctypes.data, p.ctypes.data, t.size, k, ti.ctypes.data, tl.ctypes.data, am.ctypes.data))
        return ti, tl, am

    def prefill_shared(self, prefix: Sequence[int], batch: int):
        """nano_prefill_shared: ingest the prefix once per device and make it positions 0..len(prefix)-1 of sequences 0..batch-1."""
        t = np.ascontiguousarray(prefix, np.uint32).reshape(-1)
        check(self.L.nano_prefill_shared(self.ctx, t, t.size, batch))

    def kv_image_bytes(self, n_pos: int) -> int:
        return int(self.L.nano_kv_image_bytes(self.ctx, n_pos))

    def kv_save(self, slot: int, n_pos: int) -> np.ndarray:
        """nano_kv_save: the KV image of positions 0..n_pos-1 of `slot` of the context's device model (uint8 array)"""
        img = np.empty(max(self.kv_image_bytes(n_pos), 64), np.uint8)
        n = C.c_size_t(0)
        check(self.L.nano_kv_save(self.ctx, slot, n_pos, img.ctypes.data, img.size, C.byref(n)))
        return img[:n.value]

    def kv_restore(self, slot: int, image, n_pos: Optional[int] = None):
        """nano_kv_restore: positions 0..n_pos-1 (None: all) of the image into `slot` of the context's device model"""
        a = np.ascontiguousarray(np.frombuffer(image, np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else image, np.uint8).reshape(-1)
        check(self.L.nano_kv_restore(self.ctx, slot, a.ctypes.data if a.size else None, a.size, KV_ALL if n_pos is None else n_pos))

    def lora_table_load(self, id: int, path: str):
        """nano_lora_table_load: a LoRA module file into entry `id` of the context's LoRA table"""
        check(self.L.nano_lora_table_load(self.ctx, id, path.encode()))

    def lora_table_load_bytes(self, id: int, data: bytes):
        """nano_lora_table_load_from_buffer: the bytes of a LoRA module file into entry `id`"""
        a = np.frombuffer(data, np.uint8)
        check(self.L.nano_lora_table_load_from_buffer(self.ctx, id, a.ctypes.data if a.size else None, a.size))

    def lora_table_free(self, id: int):
        check(self.L.nano_lora_table_free(self.ctx, id))

    def lora_bind(self, slots, ids):
        """nano_lora_bind: sequence slots[i] takes table entry ids[i]; None = no module"""
        s = np.ascontiguousarray(slots, np.uint32)
        i = np.ascontiguousarray([NANO_LORA_NONE if v is None else v for v in ids], np.uint32)
        check(self.L.nano_lora_bind(self.ctx, s.ctypes.data, i.ctypes.data, s.size))

    def prefill_batch(self, prompts: Sequence[Sequence[int]], want_first_ids: bool = True) -> Optional[np.ndarray]:
        """nano_prefill_batch: sequence i ingests prompts[i] from position 0, all in one ragged step per device; returns first_ids
        (the arg-max behind each prompt's last token), or None."""
        ps = [np.ascontiguousarray(p, np.uint32).reshape(-1) for p in prompts]
        ptrs = (C.c_void_p * len(ps))(*[p.ctypes.data if p.size else None for p in ps])
        n = np.array([p.size for p in ps], np.uint32)
        first = np.zeros(max(len(ps), 1), np.uint32) if want_first_ids else None
        check(self.L.nano_prefill_batch(self.ctx, ptrs, n, len(ps), first.ctypes.data if want_first_ids else None))
        return first[:len(ps)] if want_first_ids else None

    def embed_batch(self, texts: Sequence[Sequence[int]], n_embd: int, pooling="last", normalize: bool = True, dim: int = 0) -> np.ndarray:
        """nano_embed_batch: sequence i ingests texts[i] from position 0, all in one pooled ragged step; returns float32
        [len(texts), dim or n_embd], one vector per text (DeviceModel.step_rows_pool says which)."""
        ts = [np.ascontiguousarray(t, np.uint32).reshape(-1) for t in texts]
        ptrs = (C.c_void_p * len(ts))(*[t.ctypes.data if t.size else None for t in ts])
        n = np.array([t.size for t in ts], np.uint32)
        out = np.zeros((max(len(ts), 1), dim or n_embd), np.float32)
        check(self.L.nano_embed_batch(self.ctx, ptrs, n.ctypes.data, len(ts), _pooling(pooling), int(normalize), dim, out.ctypes.data))
        return out[:len(ts)]

    def decode_batch_lookup(self, histories, max_new, max_draft: int = 7, stop_token: Optional[int] = None):
        """nano_decode_batch_lookup: sequence i (slot i) decodes greedily with lookup drafts from histories[i]; returns the list of id arrays."""
        hs = [np.ascontiguousarray(h, np.uint32).reshape(-1) for h in histories]
        B = len(hs)
        outs = [np.zeros(max(int(mn), 1), np.uint32) for mn in max_new]
        hp = (C.c_void_p * max(B, 1))(*[h.ctypes.data if h.size else None for h in hs])
        op = (C.c_void_p * max(B, 1))(*[o.ctypes.data for o in outs])
        nh, mn = np.array([h.size for h in hs], np.uint32), np.ascontiguousarray(max_new, np.uint32)
        n = np.zeros(max(B, 1), np.uint32)
        check(self.L.nano_decode_batch_lookup(self.ctx, hp, nh.ctypes.data, mn.ctypes.data, B, max_draft, LOOKUP_NO_STOP if stop_token is None else stop_token,
                                              op, n.ctypes.data))
        return [outs[i][:int(n[i])].copy() for i in range(B)]

    def set_logit_edit(self, allow=None, bias=None) -> None:
        """nano_set_logit_edit: allow = mask words (or None), bias = (tokens, values) (or None); both None clears the context's edit."""
        if allow is None and bias is None:
            check(self.L.nano_set_logit_edit(self.ctx, None)); return
        e, _keep = logit_edit(allow, bias)
        check(self.L.nano_set_logit_edit(self.ctx, C.cast(C.pointer(e), C.c_void_p)))

    def forward_batch_sample(self, tokens: Sequence[int], pos: Sequence[int], samplers, histories, edits=None) -> np.ndarray:
        """nano_forward_batch_sample: one decode step of B sequences, sequence i sampled with samplers[i] (from build_sampler)
        over histories[i] (the ids its repetition penalty marks); returns the B sampled ids.  edits: None, or per sequence None or
        (allow words or None, (bias tokens, bias values) or None): nano_forward_batch_sample_edit."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        p = np.ascontiguousarray(pos, np.uint32).reshape(-1)
        B = t.size
        hs = [np.ascontiguousarray(h if h is not None else [], np.uint32).reshape(-1) for h in histories]
        sp = (C.POINTER(SamplerC) * B)(*samplers)
        hp = (C.POINTER(C.c_uint32) * B)(*[h.ctypes.data_as(C.POINTER(C.c_uint32)) if h.size else None for h in hs])
        nh = np.array([h.size for h in hs], np.uint32)
        out = np.empty(B, np.uint32)
        if edits is not None:
            arr, keep = (NanoLogitEdit * B)(), []
            for i, e in enumerate(edits):
                if e is not None:
                    arr[i], k = logit_edit(*e); keep.append(k)
            check(self.L.nano_forward_batch_sample_edit(self.ctx, t, p, B, C.cast(sp, C.c_void_p), C.cast(hp, C.c_void_p),
                                                        nh.ctypes.data, C.cast(arr, C.c_void_p), out.ctypes.data))
            return out
        check(self.L.nano_forward_batch_sample(self.ctx, t, p, B, C.cast(sp, C.c_void_p), C.cast(hp, C.c_void_p),
                                               nh.ctypes.data, out.ctypes.data))
        return out

    def run_session(self, prompt: Sequence[int], max_steps: int):
        """nano_session_init_ids + nano_session_step_ids until stop; returns (generated ids, last status)."""
        p = np.ascontiguousarray(prompt, np.uint32)
        s = self.L.nano_session_init_ids(self.ctx, p, p.size, self.max_seq_len)
        assert s, "session init failed"
        out, status = [], 0
        for _ in range(max_steps):
            status = int(self.L.nano_session_step_ids(self.ctx, s))
            sess = C.cast(s, C.POINTER(NanoSession)).contents
            if status == 12 or (status == -10 and not sess.is_prefilling):
                out.append(int(sess.next_token))
            if status < 0:
                break
        self.L.llm_session_free(s)
        return out, status


class NanoLogitEdit(C.Structure):
    """NanoLogitEdit (include/nano_infer_abi.h)."""
    _fields_ = [("allow", C.POINTER(C.c_uint32)), ("bias_tokens", C.POINTER(C.c_uint32)), ("bias_values", C.POINTER(C.c_float)), ("n_bias", C.c_uint32)]


def logit_edit(allow=None, bias=None):
    """(NanoLogitEdit, the arrays it points into) from mask words and a (tokens, values) pair"""
    e, keep = NanoLogitEdit(), []
    if allow is not None:
        w = np.ascontiguousarray(allow, np.uint32).reshape(-1); keep.append(w)
        e.allow = w.ctypes.data_as(C.POINTER(C.c_uint32))
    if bias is not None and len(bias[0]):
        t = np.ascontiguousarray(bias[0], np.uint32).reshape(-1); v = np.ascontiguousarray(bias[1], np.float32).reshape(-1); keep += [t, v]
        e.bias_tokens, e.bias_values, e.n_bias = t.ctypes.data_as(C.POINTER(C.c_uint32)), v.ctypes.data_as(C.POINTER(C.c_float)), t.size
    return e, keep


class SamplerC(C.Structure):
    """Sampler (include/nano_infer_abi.h = reference infer/infer.h)."""
    _fields_ = [("vocab_size", C.c_int), ("probindex", C.c_void_p), ("repetition_penalty", C.c_float), ("temperature", C.c_float),
                ("top_p", C.c_float), ("top_k", C.c_uint32), ("rng_state", C.c_uint64)]


class NanoSession(C.Structure):
    """Nano_Session (include/nano_infer_abi.h = reference infer/infer.h:237-250)."""
    _fields_ = [("prompt", C.c_void_p), ("num_prompt_tokens", C.c_uint32), ("max_seq_len", C.c_uint32),
                ("output_ids", C.POINTER(C.c_uint32)), ("output_count", C.c_uint32), ("output_text", C.c_void_p),
                ("next_token", C.c_uint32), ("pos", C.c_uint32), ("is_prefilling", C.c_int32),
                ("t_0", C.c_uint64), ("t_1", C.c_uint64), ("tps", C.c_float)]
