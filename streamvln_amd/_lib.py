"""ctypes binding of include/streamvln_hip.h (libstreamvln_hip.so, built in-tree by csrc/build.sh).

There is no CPU fallback: a missing library or a failing call raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVLN_LIB: another build of the same engine (tools/ab_lib.sh: A/B of two builds on one GPU box); default = the in-tree library
LIB_PATH = os.environ.get("SVLN_LIB") or os.path.join(_HERE, "libstreamvln_hip.so")

SVLN_BF16, SVLN_F32 = 0, 1
EPI_NONE, EPI_GELU_TANH, EPI_GELU_ERF, EPI_SWIGLU, EPI_ARGMAX = 0, 1, 2, 3, 4


class SvlnConfig(C.Structure):
    _fields_ = [
        ("v_hidden", C.c_int32), ("v_inter", C.c_int32), ("v_heads", C.c_int32), ("v_layers", C.c_int32),
        ("v_patch", C.c_int32), ("v_image", C.c_int32), ("v_eps", C.c_float),
        ("hidden", C.c_int32), ("layers", C.c_int32), ("q_heads", C.c_int32), ("kv_heads", C.c_int32),
        ("head_dim", C.c_int32), ("inter", C.c_int32), ("vocab", C.c_int32),
        ("rope_theta", C.c_float), ("rms_eps", C.c_float),
        ("max_positions", C.c_int32), ("max_envs", C.c_int32), ("max_frames", C.c_int32), ("dtype", C.c_int32),
    ]


class SvlnTurnArgs(C.Structure):
    """svln_turn_args of include/streamvln_hip.h"""
    _fields_ = [
        ("pixels", C.c_void_p), ("n_frames", C.c_int32), ("pixels_on_device", C.c_int32),
        ("env", C.c_int32),
        ("ids", C.c_void_p), ("n_ids", C.c_int32), ("n_memory", C.c_int32),
        ("new_window", C.c_int32), ("new_episode", C.c_int32),
        ("max_new_tokens", C.c_int32),
        ("eos_ids", C.c_void_p), ("n_eos", C.c_int32),
    ]


class SvlnGemmProblem(C.Structure):
    """svln_gemm_problem of include/streamvln_hip.h"""
    _fields_ = [(n, C.c_uint64 if n == "ws_elems" else C.c_int64) for n in (
        "dtype", "epi", "M", "N", "K", "fp8", "has_ws", "ws_elems", "has_zeros", "norm_out", "norm_w", "res", "rope", "rope_nq", "rope_nkv",
        "rope_T", "vitpack", "vit_F", "vit_S", "vit_heads", "vit_head_dim", "force_cfg", "force_split")]


class SvlnGemmLaunch(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tile", "splitk", "fp8", "ntw", "vp", "tile_base", "launch_tiles", "nsplit", "grid", "block",
                                         "lds_bytes", "bm", "bn", "reducer")] + \
               [("reducer_grid", C.c_int32 * 3), ("reducer_block", C.c_int32), ("reduce_too_large", C.c_int32)]


class SvlnGemmPlan(C.Structure):
    """svln_gemm_plan_out of include/streamvln_hip.h"""
    _fields_ = [(n, C.c_int32) for n in ("nt_w", "bn_fast", "n_launches", "fused", "vit_packer")] + [("launch", SvlnGemmLaunch * 2)]


class SvlnDecodeLayerOp(C.Structure):
    """svln_decode_layer_op of include/streamvln_hip.h"""
    _fields_ = [(n, C.c_void_p) for n in ("o_w", "post_norm", "gu_w", "down_w", "next_norm", "next_qkv_w", "next_qkv_b", "part", "kv_len", "skip",
                                          "x", "qkv_out")] + \
               [("gran", C.c_void_p * 4), ("seq", C.c_void_p), ("giveup", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("nsplit", "tiles_per_split", "n_q", "n_kv", "H", "I", "qkv_dim", "cus")] + [("eps", C.c_float)]


class SvlnArgmaxStepOp(C.Structure):
    """svln_argmax_step_op of include/streamvln_hip.h"""
    _fields_ = [(n, C.c_void_p) for n in ("part_val", "part_idx", "part_sum", "part_raw", "part_max", "eos", "ctl_out", "out_ids", "last_token",
                                          "out_top", "scores", "flags")] + \
               [(n, C.c_int32) for n in ("n", "steps", "use_ctl", "pos", "kv_len", "done", "count", "max_new", "n_eos", "flag_bytes", "rows")]


class SvlnDraftSelectOp(C.Structure):
    """svln_draft_select_op of include/streamvln_hip.h"""
    _fields_ = [(n, C.c_void_p) for n in ("k", "fed", "cand", "cand_score", "eos", "ctl_out", "out_ids", "last_token", "scores", "rec",
                                          "stats", "taps")] + \
               [(n, C.c_int32) for n in ("G", "r", "pos", "kv_len", "done", "count", "max_new", "n_eos", "rows", "tap_rows")]


class SvlnDecodeLayerWalkOp(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("elem_size", "K", "nrows", "pair", "first")]


class SvlnDecodeLayerSlot(C.Structure):
    _fields_ = [("load_off", C.c_int64)] + [(n, C.c_int32) for n in ("valid", "row", "pb", "row_done")]


GEMM_TILES = ("skinny", "c64", "c128", "c128L", "c128K2", "c256", "c256n64", "big", "p8", "p8_32")      # svln_gemm_launch.tile
GEMM_FORCE_FP8_SCALED = 0x40000        # force_cfg bit of svln_op_gemm_fp8: the block-scaled MFMA form (svln_set_fp8_scaled_mfma)
GEMM_REDUCERS = (None, "epilogue", "rownorm", "qkv_rope", "vitpack")                                     # svln_gemm_launch.reducer


def gemm_plan(**problem) -> SvlnGemmPlan:
    """svln_gemm_plan for the given svln_gemm_problem fields (the others 0): what the GEMM dispatcher does with the product; no GPU needed"""
    plan = SvlnGemmPlan()
    check(load().svln_gemm_plan(C.byref(SvlnGemmProblem(**problem)), C.byref(plan)))
    return plan


MODE_BITS = ("decode_graph", "persistent", "fp8_decode", "mxfp4_decode", "mxfp4_batched", "fp8_gemm", "fp8_scaled", "packed", "speculative",
             "prefill_draft", "batch_draft", "scores", "topk", "entropy", "sampling", "truncation", "allowed", "penalty", "jobs", "group")

# the Caller enumeration of csrc/modes.h, in order (svln_mode_refusal's `caller` is an index into it)
MODE_CALLERS = ("set_decode_persistent:on", "set_decode_persistent:off", "set_fp8_decode:on", "set_fp8_decode:off", "set_mxfp4_decode:on",
                "set_mxfp4_decode:off", "set_mxfp4_batched:on", "set_mxfp4_batched:off", "set_fp8_gemm:on", "set_fp8_gemm:off", "set_fp8_scaled_mfma",
                "set_speculative:on", "set_speculative:off", "set_prefill_draft:on", "set_prefill_draft:off", "set_batch_draft:on",
                "set_batch_draft:off", "set_token_scores:on", "set_token_scores:off", "top_logprobs:on", "top_logprobs:off", "token_entropy:on",
                "token_entropy:off", "set_sampling:on", "set_sampling:off", "sampling_truncation:on", "sampling_truncation:off",
                "set_allowed_tokens", "set_repetition_penalty", "weight_write", "generate_batch", "generate_group", "generate_beams",
                "generate_forced", "batch_submit_forced", "generate_candidates", "op_gemv_batched_argmax")


class SvlnModeState(C.Structure):
    """svln_mode_state of include/streamvln_hip.h"""
    _fields_ = [(n, C.c_int32) for n in MODE_BITS + ("group_env",)]


class SvlnModeRule(C.Structure):
    """svln_mode_rule_out of include/streamvln_hip.h"""
    _fields_ = [(n, C.c_int32) for n in ("caller", "part", "bit", "must_be_on", "on_no_change")] + \
               [(n, C.c_char_p) for n in ("caller_name", "what", "tail")]


def mode_rules():
    """the engine's mode rule table (csrc/modes.h) in order, as dicts (bit: its MODE_BITS name); no GPU needed"""
    n, nc, nb = C.c_int32(), C.c_int32(), C.c_int32()
    check(load().svln_mode_rule_count(C.byref(n), C.byref(nc), C.byref(nb)))
    assert (nb.value, nc.value) == (len(MODE_BITS), len(MODE_CALLERS)), (nb.value, nc.value)
    out = []
    for i in range(n.value):
        r = SvlnModeRule()
        check(load().svln_mode_rule(i, C.byref(r)))
        out.append({"caller": r.caller, "part": r.part, "bit": MODE_BITS[r.bit], "must_be_on": bool(r.must_be_on),
                    "on_no_change": bool(r.on_no_change), "caller_name": r.caller_name.decode(), "text": (r.what + r.tail).decode()})
    return out


def mode_refusal(caller, on=(), no_change=False, who=None, group_env=0):
    """svln_mode_refusal: None if `caller` (a MODE_CALLERS name or its index) is accepted while the MODE_BITS named in `on` are on, else the engine's message; no GPU needed"""
    st = SvlnModeState(**{b: 1 for b in on}, group_env=group_env)
    buf, refused = C.create_string_buffer(1024), C.c_int32()
    if isinstance(caller, str):
        caller = MODE_CALLERS.index(caller)
    check(load().svln_mode_refusal(int(caller), who.encode() if who else None, C.byref(st), int(no_change), buf, len(buf), C.byref(refused)))
    return buf.value.decode() if refused.value else None


_P, _I, _F, _I64, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_uint64
_PI32, _PI64, _PF, _PD = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_double)

#: every symbol include/streamvln_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "svln_create": (_I, [C.POINTER(SvlnConfig), _I, C.POINTER(_P)]),
    "svln_destroy": (None, [_P]),
    "svln_last_error": (C.c_char_p, []),
    "svln_sync": (_I, [_P]),
    "svln_synth_tensor": (_I, [_P, C.c_char_p, C.c_uint64, _F, _F]),
    "svln_set_tensor": (_I, [_P, C.c_char_p, _P, _I, _I64, _I]),
    "svln_weights_ready": (_I, [_P]),
    "svln_get_tensor_f32": (_I, [_P, C.c_char_p, _PF, _I64]),
    "svln_reset_env": (_I, [_P, _I]),
    "svln_kv_reset": (_I, [_P, _I]),
    "svln_env_state": (_I, [_P, _I, _PI32, _PI32]),
    "svln_kv_free_pages": (_I, [_P, _PI32]),
    "svln_encode_frames": (_I, [_P, _P, _I, _I]),
    "svln_preprocess_frames": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "svln_preprocess_frames_enqueue": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "svln_engine_stream": (_I, [_P, C.POINTER(C.c_void_p)]),
    "svln_preprocess_time": (_I, [_P, _PD, _PI64, _I]),
    "svln_frame_ring": (_I, [_P, _I, _I, _I, C.POINTER(C.c_void_p), _PI64]),
    "svln_frame_ring_wait": (_I, [_P, _I]),
    "svln_turn": (_I, [_P, C.POINTER(SvlnTurnArgs), _PI64, _I, _PI32, _PI32]),
    "svln_append_turn": (_I, [_P, _I, _PI64, _I, _I]),
    "svln_append_turn_at": (_I, [_P, _I, _PI64, _I, _I, _I]),
    "svln_generate_batch": (_I, [_P, _PI32, _I, _I, _PI64, _I, _PI64, _I, _PI32]),
    "svln_batch_submit": (_I, [_P, _I, _I, _PI64, _I, _PI32]),
    "svln_batch_step": (_I, [_P, _PI32, _PI32, _PI32]),
    "svln_batch_result": (_I, [_P, _I, _PI32, _PI64, _I, _PI32]),
    "svln_batch_cancel": (_I, [_P, _I]),
    "svln_set_turn_row_limit": (_I, [_P, _I]),
    "svln_set_repetition_penalty": (_I, [_P, _F]),
    "svln_get_hidden_batch": (_I, [_P, _I, _PF, _I, _PI32]),
    "svln_generate": (_I, [_P, _I, _I, _PI64, _I, _PI64, _I, _PI32]),
    "svln_generate_fixed": (_I, [_P, _I, _I, _PI64]),
    "svln_get_hidden": (_I, [_P, _PF, _I, _PI32]),
    "svln_get_embeds": (_I, [_P, _I, _I, _I, _PF]),
    "svln_get_frame_feats": (_I, [_P, _I, _I, _PF]),
    "svln_get_top2": (_I, [_P, _PF]),
    "svln_set_token_scores": (_I, [_P, _I]),
    "svln_top_logprobs": (_I, [_P, _I]),
    "svln_get_topk": (_I, [_P, _PI32, _PF, _I, _PI32, _PI32]),
    "svln_batch_topk": (_I, [_P, _I, _PI32, _PF, _I, _PI32, _PI32]),
    "svln_generate_batch_topk": (_I, [_P, _I, _PI32, _PF, _I, _PI32, _PI32]),
    "svln_op_gemv_batched_argmax_topk": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _I, _I, _F, _U64, _PI32, _PI32, _PI32, _PF, _PF,
                                              _PI32, _PI32, _PF, _PI32]),
    "svln_op_gemm_argmax_topk": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _I, _I, _F, _U64, _PI32, _PI32, _PI32, _PF, _PF, _PI32,
                                      _PI32, _PF, _PI32]),
    "svln_token_entropy": (_I, [_P, _I]),
    "svln_get_token_entropy": (_I, [_P, _PF, _I, _PI32]),
    "svln_batch_entropy": (_I, [_P, _I, _PF, _I, _PI32]),
    "svln_generate_batch_entropy": (_I, [_P, _I, _PF, _I, _PI32]),
    "svln_op_gemv_argmax_entropy": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _F, _I, _F, _U64, C.c_int32, C.c_int32, _PI32, _PF, _PF, _PF, _PI32, _PF,
                                         _PF, _PF, _PF, _PI32]),
    "svln_op_gemv_batched_argmax_entropy": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _I, _F, _U64, _PI32, _PI32, _PI32, _PF, _PF, _PF, _PI32,
                                                 _PF, _PF, _PF, _PF, _PI32]),
    "svln_op_gemm_argmax_entropy": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _I, _F, _U64, _PI32, _PI32, _PI32, _PF, _PF, _PF, _PI32, _PF,
                                         _PF, _PF, _PF, _PI32]),
    "svln_op_entropy_merge": (_I, [_P, _PF, _PI32, _PF, _PF, _PF, _I, _I, _PF]),
    "svln_get_token_scores": (_I, [_P, _PF, _I, _PI32]),
    "svln_batch_scores": (_I, [_P, _I, _PF, _I, _PI32]),
    "svln_generate_batch_scores": (_I, [_P, _I, _PF, _I, _PI32]),
    "svln_set_sampling": (_I, [_P, _I, _F, _U64]),
    "svln_sampling_truncation": (_I, [_P, _I, _F]),
    "svln_op_truncate": (_I, [_P, _PF, _PI32, _I, _I, _I, _PI32, _PI32, _U64, _F, _I, _F, _PF, _PI32, _PF, _PF, _PF, _PI32, _PF]),
    "svln_set_allowed_tokens": (_I, [_P, _PI64, _I]),
    "svln_get_allowed_logprobs": (_I, [_P, _PF, _I, _PI32, _PI32]),
    "svln_batch_allowed_logprobs": (_I, [_P, _I, _PF, _I, _PI32, _PI32]),
    "svln_generate_batch_allowed_logprobs": (_I, [_P, _I, _PF, _I, _PI32, _PI32]),
    "svln_generate_group": (_I, [_P, _I, _I, _I, _PI64, _I, _PI64, _I, _PI32]),
    "svln_turn_group": (_I, [_P, C.POINTER(SvlnTurnArgs), _I, _PI64, _I, _PI32]),
    "svln_generate_forced": (_I, [_P, _I, _PI64, _I, _PI64, _I, _PF, _PI64, _PF, _PI32]),
    "svln_turn_forced": (_I, [_P, C.POINTER(SvlnTurnArgs), _PI64, _I, _PF, _PI64, _PF, _PI32]),
    "svln_generate_candidates": (_I, [_P, _I, _I, _PI64, _PI32, _PI64, _I, _PF, _PI64, _PF]),
    "svln_turn_candidates": (_I, [_P, C.POINTER(SvlnTurnArgs), _I, _PI64, _PI32, _PF, _PI64, _PF]),
    "svln_generate_candidates_folded": (_I, [_P, _I, _I, _PI64, _PI32, _PI64, _I, _PF, _PI64, _PF]),
    "svln_turn_candidates_folded": (_I, [_P, C.POINTER(SvlnTurnArgs), _I, _PI64, _PI32, _PF, _PI64, _PF]),
    "svln_batch_submit_forced": (_I, [_P, _I, _PI64, _I, _PI64, _I, _PI32]),
    "svln_batch_forced": (_I, [_P, _I, _PF, _PI64, _PF, _I, _PI32]),
    "svln_batch_forced_stats": (_I, [_P, _PI64, _PI64, _PI64, _I]),
    "svln_op_gemv_batched_target": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _PI32, _F, _PI32, _PF, _PF, _PF]),
    "svln_op_gemm_target": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _PI32, _F, _PI32, _PF, _PF, _PF]),
    "svln_op_read_argmax_partials": (_I, [_P, _I, _I, _PF, _PI32, _PF]),
    "svln_group_select": (_I, [_P, _I, _I, _PI32]),
    "svln_group_logprobs": (_I, [_P, _I, _PF, _I, _PI32]),
    "svln_group_dist": (_I, [_P, _I, _PF, _I, _PI32, _PI32]),
    "svln_get_hidden_group": (_I, [_P, _I, _PF, _I, _PI32]),
    "svln_op_kv_page_copy": (_I, [_P, _I, _PI32, _I]),
    "svln_generate_beams": (_I, [_P, _I, _I, _I, _PI64, _I, _PI64, _I, _PI32, _PF]),
    "svln_turn_beams": (_I, [_P, C.POINTER(SvlnTurnArgs), _I, _PI64, _I, _PI32, _PF]),
    "svln_beam_trace": (_I, [_P, _I, _PI32, _PI32, _PI32, _PF, _PI32]),
    "svln_op_beam_page_gather": (_I, [_P, _PI32, _PI32, _I]),
    "svln_op_beam_select": (_I, [_P, _I, _I, _I, _I, _I, _PI32, _I, _PI32, _PF, _PI32, _PF, _PI32, _PF, _PI32, _PI32, _PF, _PI32, _PF, _PI32,
                                 _PI32, _PI32, _PI32]),
    "svln_op_kv_pool_read": (_I, [_P, _I, _I, _I, _PF, _PF]),
    "svln_set_layer_taps": (_I, [_P, _I, _I]),
    "svln_get_layer_taps": (_I, [_P, _PF]),
    "svln_get_layer_probe": (_I, [_P, _I, _PF, _I64, _PI32, _PI32]),
    "svln_set_decode_graph": (_I, [_P, _I]),
    "svln_set_decode_persistent": (_I, [_P, _I]),
    "svln_probe_decode_layer": (_I, [_P, _I, C.POINTER(C.c_uint64), _I, _PI32]),
    "svln_op_decode_layer": (_I, [_P, C.POINTER(SvlnDecodeLayerOp)]),
    "svln_decode_layer_supported": (_I, [_I, _I, _I, _I, _I, _I, _PI32]),
    "svln_decode_layer_walk": (_I, [C.POINTER(SvlnDecodeLayerWalkOp), C.POINTER(SvlnDecodeLayerWalkOp), _I, _I, C.POINTER(SvlnDecodeLayerSlot), _I,
                                    _PI32, _PI64]),
    "svln_set_fp8_decode": (_I, [_P, _I]),
    "svln_set_fp8_gemm": (_I, [_P, _I]),
    "svln_set_fp8_scaled_mfma": (_I, [_P, _I]),
    "svln_set_mxfp4_decode": (_I, [_P, _I]),
    "svln_set_mxfp4_batched": (_I, [_P, _I]),
    "svln_set_packed_decode": (_I, [_P, _I]),
    "svln_packed_stats": (_I, [_P, _PI64, _PI64, _PI64, _PI64]),
    "svln_op_pack_rows": (_I, [_P, _P, _I, _I64, _I, _P, _P, _PI64]),
    "svln_op_unpack_rows": (_I, [_P, _P, _P, _P, _I, _I64, _I, _P]),
    "svln_op_gemv_packed": (_I, [_P, _P, _P, _P, _I, _P, _P, _F, _P, _P, _P, _I, _I, _I, _PI32]),
    "svln_set_speculative": (_I, [_P, _I]),
    "svln_set_draft": (_I, [_P, _I, _PI64, _I]),
    "svln_draft_stats": (_I, [_P, _PI64, _PI64, _PI64, _I]),
    "svln_set_prefill_draft": (_I, [_P, _I]),
    "svln_prefill_draft_stats": (_I, [_P, _PI64, _PI64, _PI64, _I]),
    "svln_generate_drafts": (_I, [_P, _I, _I, _PI64, _PI32, _I, _PI64, _I, _PI64, _I, _PI32, _PI32, _PI32]),
    "svln_turn_drafts": (_I, [_P, C.POINTER(SvlnTurnArgs), _I, _PI64, _PI32, _PI64, _I, _PI32, _PI32, _PI32, _PI32]),
    "svln_drafts_stats": (_I, [_P, _PI64]),
    "svln_op_draft_select": (_I, [_P, C.POINTER(SvlnDraftSelectOp)]),
    "svln_set_batch_draft": (_I, [_P, _I]),
    "svln_batch_draft_stats": (_I, [_P, _PI64, _PI64, _PI64, _PI64, _PI64, _I]),
    "svln_set_memory_prune": (_I, [_P, _I]),
    "svln_op_memory_prune": (_I, [_P, _P, _I, _I, _PI32, _PF]),
    "svln_probe_reset": (_I, [_P]),
    "svln_probe_read": (_I, [_P, _PD, _PI64, _PD]),
    "svln_probe_read_prefill": (_I, [_P, _PD, _PI64, _PD, _PD, _PD]),
    "svln_phase_times": (_I, [_P, _PD, _PD, _PD, _I]),
    "svln_set_feature_cache": (_I, [_P, _I]),
    "svln_feature_cache_stats": (_I, [_P, _PI64, _PI64]),
    "svln_op_gemm": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I]),
    "svln_op_gemm_norm": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _P, _I, _P, _P, _P, _F, _I, _I, _I, _I, _PI32]),
    "svln_op_gemm_norm_q8": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _F, _I, _I, _I, _I, _P, _P, _PI32]),
    "svln_gemm_plan": (_I, [C.POINTER(SvlnGemmProblem), C.POINTER(SvlnGemmPlan)]),
    "svln_mode_refusal": (_I, [_I, C.c_char_p, C.POINTER(SvlnModeState), _I, C.c_char_p, _I, _PI32]),
    "svln_mode_rule_count": (_I, [_PI32, _PI32, _PI32]),
    "svln_mode_rule": (_I, [_I, C.POINTER(SvlnModeRule)]),
    "svln_op_gemv": (_I, [_P, _P, _I, _P, _P, _F, _P, _P, _P, _I, _I, _I, _PI32]),
    "svln_op_gemm_fp8": (_I, [_P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    "svln_op_gemv_batched": (_I, [_P, _P, _I, _P, _I, _P, _F, _P, _P, _I, _P, _I, _I, _I, _I, _I, _PI32]),
    "svln_op_quant_fp8": (_I, [_P, _P, _I64, _I, _P, _P]),
    "svln_op_gemv_fp8": (_I, [_P, _P, _P, _I, _P, _P, _F, _P, _P, _P, _I, _I, _I, _PI32]),
    "svln_op_quant_mxfp4": (_I, [_P, _P, _I64, _I, _P, _P]),
    "svln_op_gemv_mxfp4": (_I, [_P, _P, _P, _I, _P, _P, _F, _P, _P, _P, _I, _I, _I, _PI32]),
    "svln_op_gemv_mxfp4_batched": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _PI32]),
    "svln_op_gemv_mxfp4_batched_argmax_pen": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _PI32]),
    "svln_op_gemv_argmax_scores": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _F, _PI32, _PF]),
    "svln_op_gemv_argmax_topk": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _F, _I, _I, _F, _U64, _I, _I, _PI32, _PF, _PF, _PI32, _PF, _PF, _PF,
                                      _PF, _PI32, _PI32, _PF, _PI32]),
    "svln_op_gemv_batched_argmax_scores": (_I, [_P, _P, _I, _P, _I, _P, _F, _I, _I, _I, _P, _P, _F, _PI32, _PF]),
    "svln_op_gemm_argmax_scores": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _PI32, _PF]),
    "svln_op_gemv_argmax_sample": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _F, _F, _U64, _I, _I, _PI32, _PF]),
    "svln_op_gemv_batched_argmax_sample": (_I, [_P, _P, _I, _P, _I, _P, _F, _I, _I, _I, _P, _P, _F, _F, _U64, _PI32, _PI32, _PI32, _PF]),
    "svln_op_gemm_argmax_sample": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _F, _F, _U64, _PI32, _PI32, _PI32, _PF]),
    "svln_op_gumbel": (_I, [_P, _U64, _I, _I, _I, _I, _PF]),
    "svln_op_subset_argmax": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _PI64, _I, _P, _P, _F, _F, _U64, _PI32, _PI32, _PI32, _PF, _PF, _PF]),
    "svln_op_rmsnorm": (_I, [_P, _P, _P, _P, _I, _I, _F]),
    "svln_op_layernorm": (_I, [_P, _P, _P, _P, _P, _I, _I, _F]),
    "svln_op_rmsnorm_tap": (_I, [_P, _P, _P, _P, _I, _I, _F, _I, _P, _I, _I]),
    "svln_op_rmsnorm_indexed": (_I, [_P, _P, _I, _P, _P, _PI32, _PI32, _P, _I, _I, _I, _F]),
    "svln_op_gather_rows": (_I, [_P, _PI32, _I, _P, _I, _P, _I, _P, _I, _I]),
    "svln_op_gather_rows_ragged": (_I, [_P, _PI32, _I, _P, _I, _P, _I, _I]),
    "svln_op_frame_hash": (_I, [_P, _P, _I, _I64, C.POINTER(C.c_uint64)]),
    "svln_op_attention_llm": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _I, _I]),
    "svln_op_attention_vit": (_I, [_P, _P, _I, _I, _P, _I]),
    "svln_op_attention_decode": (_I, [_P, _I, _P, _I, _I64, _PI32, _P, _P, _I]),
    "svln_op_attention_verify": (_I, [_P, _I, _P, _I, _I, _P, _P, _I]),
    "svln_op_attention_verify_multi": (_I, [_P, _I, _I, _P, _I, _I, _PI32, _P, _PI32, _I, _P, _I]),
    "svln_op_verify_step": (_I, [_P, _I, _PI32, _PI32, _I, _I, _PI64, _I, _PI32, _PI32, _PI64, _PI32]),
    "svln_op_argmax_step": (_I, [_P, C.POINTER(SvlnArgmaxStepOp)]),
    "svln_op_dead_step": (_I, [_P, _I, C.c_char_p, _I, _PI32]),
    "svln_op_kv_read": (_I, [_P, _I, _I, _I, _PF, _PF]),
    "svln_op_llm_qkv_rope": (_I, [_P, _P, _I, _I, _P, _I, _PI32]),
    "svln_op_rope_kv_mirror": (_I, [_P, _P, _I, _I, _I, _PI32, _I]),
    "svln_op_set_pages": (_I, [_P, _I, _PI32, _I]),
    "svln_op_fill_attn_state": (_I, [_P, _F, _I]),
    "svln_op_vit_qkv_attention": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _PI32]),
    "svln_op_fill_vit_state": (_I, [_P, _F, _I]),
    "svln_op_vit_kv_read": (_I, [_P, _PF, _PF]),
    "svln_op_pool": (_I, [_P, _P, _P, _I]),
    "svln_op_patchify": (_I, [_P, _P, _P, _I]),
}

_lib = None


def load():
    """dlopen the engine (no GPU needed to load; compute calls need one)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with streamvln_amd/csrc/build.sh "
                               f"(or __graft_entry__.build()); there is no fallback path")
        # torch first: the engine must share torch's HIP runtime (same libamdhip64 instance) so that device
        # pointers and the GPU context are common to both; loading ours first can bind a second runtime copy.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


class SvlnError(RuntimeError):
    pass


def check(rc: int):
    if rc != 0:
        raise SvlnError(load().svln_last_error().decode("utf-8", "replace"))
