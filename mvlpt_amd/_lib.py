"""ctypes binding of libmvlpt_hip.so (C ABI in include/mvlpt_hip.h).

There is NO CPU fallback: if the shared library is missing (build it with ``make`` or
``python -c 'import __graft_entry__ as g; g.build()'``) importing this module raises, and every
compute call needs a HIP device.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64; it must be loaded FIRST so that libmvlpt_hip.so binds to
# the same HIP runtime instance (two runtimes in one process do not see each other's devices, streams or pointers).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVLPT_HIP_LIB") or os.path.join(_HERE, "libmvlpt_hip.so")   # override: A/B builds of the same ABI

DT_F32, DT_F16, DT_BF16 = 0, 1, 2
LABEL_INT64, LABEL_PROB_F32 = 0, 1
EPI_STORE16, EPI_GELU, EPI_RESID32, EPI_GELUBWD, EPI_STORE32, EPI_GELU_SPLIT, EPI_GELUBWD_SPLIT, EPI_STORE_SPLIT = 0, 1, 2, 3, 4, 5, 6, 7
# kernel families mvlpt_op_gemm_route reports (MVLPT_GEMM_* in the header)
GEMM_BT_128x128_R2, GEMM_BT_128x128_R4, GEMM_BT_256x128_R3, GEMM_BT_256x256_R2, GEMM_PHASED, GEMM_PC, GEMM_PCP = 1, 2, 3, 4, 5, 6, 7
PREC_FAST, PREC_SPLIT_GRAD, PREC_SPLIT_ALL = 0, 1, 2
ACT_QUICKGELU, ACT_GELU = 0, 1                           # MVLPT_ACT_*
ACT_OUT_SINGLE, ACT_OUT_PAIR, ACT_OUT_MIXED = 0, 1, 2    # MVLPT_ACT_OUT_*
ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -3, -4      # MVLPT_ERR_*
NEAREST_MAX_K, NEAREST_MAX_ROWS = 64, 65535 * 8      # MVLPT_NEAREST_MAX_K, MVLPT_NEAREST_MAX_ROWS
TPT_MAX_VIEWS, TPT_MAX_GROUPS, TPT_MAX_CLASSES = 128, 65535, 1 << 20      # MVLPT_TPT_MAX_*
TIP_LOGITS, TIP_TRAIN, TIP_SEARCH = 0, 1, 2               # MVLPT_TIP_* modes of mvlpt_tip_workspace_bytes
TIP_MAX_NB, TIP_MAX_NA, TIP_MAX_CLASSES, TIP_MAX_ROWS = 256, 32, 1 << 20, (1 << 31) - 256      # MVLPT_TIP_MAX_*
EVAL_SORT_TILE, EVAL_MAX_ROWS, EVAL_POINTS, EVAL_FLAG_NONFINITE, EVAL_FLAG_SOFT_TARGET = 4096, 1 << 20, 11, 1, 2      # MVLPT_EVAL_*
TEXT_MIN_L = 3     # MVLPT_TEXT_MIN_L: the smallest sequence length mvlpt_text_encode_tokens accepts


class MvlptArch(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "image_resolution", "patch_size", "vision_width", "vision_layers", "vision_heads",
        "context_length", "text_width", "text_layers", "text_heads", "embed_dim", "compute_dtype")]


class MvlptResNetArch(C.Structure):
    _fields_ = [("image_resolution", C.c_int), ("width", C.c_int), ("layers", C.c_int * 4), ("heads", C.c_int), ("output_dim", C.c_int)]


TEXT_JOB_BYTES = 96     # MVLPT_TEXT_JOB_BYTES


class MvlptTextJob(C.Structure):
    """One text forward (include/mvlpt_hip.h documents the fields); class_lo / class_hi are host arrays, the other pointers device."""
    _fields_ = ([(n, C.c_void_p) for n in ("prefix", "suffix", "ctx", "ctx_deep", "layout", "eot")]
                + [(n, C.POINTER(C.c_int32)) for n in ("class_lo", "class_hi")]
                + [(n, C.c_int32) for n in ("n_ctx", "ctx_per_class", "n_deep", "groups", "n_cls", "L", "save_for_bwd", "reserved")])


assert C.sizeof(MvlptTextJob) == TEXT_JOB_BYTES


class MvlptKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int64), ("ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double), ("busy_ms", C.c_double), ("flops_executed", C.c_double)]


class MvlptImageDesc(C.Structure):
    _fields_ = [("offset", C.c_int64)] + [(n, C.c_int32) for n in (
        "height", "width", "crop_top", "crop_left", "crop_height", "crop_width", "resize_height", "resize_width",
        "out_top", "out_left", "flip", "reserved")]


AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE = 0, 1, 2, 3      # MVLPT_AUG_*
AUG_MAX_HOLES = 4                                                      # MVLPT_AUG_MAX_HOLES


class MvlptAugmentDesc(C.Structure):
    _fields_ = [("n_ops", C.c_int32), ("ops", C.c_int32 * 4), ("factor", C.c_float * 3), ("hue_shift", C.c_int32),
                ("grayscale", C.c_int32), ("n_holes", C.c_int32), ("hole", (C.c_int32 * 4) * AUG_MAX_HOLES)]


# MVLPT_JPEG_ROUTE_*: who decodes a file (0: the device), and the bits of a status word > 0 (MVLPT_JPEG_ST_*)
(JPEG_ROUTE_DEVICE, JPEG_ROUTE_MALFORMED, JPEG_ROUTE_FRAME, JPEG_ROUTE_SCANS, JPEG_ROUTE_COLOUR, JPEG_ROUTE_SAMPLING, JPEG_ROUTE_TABLES,
 JPEG_ROUTE_RESTART, JPEG_ROUTE_SIZE) = range(9)
JPEG_ST_BAD_CODE, JPEG_ST_COEF_INDEX, JPEG_ST_ENDED_EARLY, JPEG_ST_BAD_SIZE = 1, 2, 4, 8
JPEG_MAX_BATCH = 16384


class MvlptJpegInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("height", "width", "components", "h_samp", "v_samp", "restart_interval", "n_segments", "route")]


OPTIM_SGD, OPTIM_ADAM, OPTIM_ADAMW = 0, 1, 2
OPTIM_MAX_SEGS = 1024   # MVLPT_OPTIM_MAX_SEGS


class MvlptOptimSeg(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("active", C.c_int32), ("missed", C.c_int32)]


class MvlptOptimHyper(C.Structure):
    _fields_ = [("kind", C.c_int32), ("nesterov", C.c_int32), ("lr", C.c_double), ("weight_decay", C.c_double), ("momentum", C.c_double),
                ("dampening", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("launch", C.c_int64)]


_vp, _i, _f = C.c_void_p, C.c_int, C.c_float

# name -> (restype, argtypes): every symbol include/mvlpt_hip.h declares
SIGNATURES = {
    "mvlpt_create": (_i, [C.POINTER(MvlptArch), C.POINTER(_vp)]),
    "mvlpt_create_resnet": (_i, [C.POINTER(MvlptArch), C.POINTER(MvlptResNetArch), C.POINTER(_vp)]),
    "mvlpt_destroy": (_i, [_vp]),
    "mvlpt_set_precision": (_i, [_vp, _i]),
    "mvlpt_set_activation": (_i, [_vp, _i]),
    "mvlpt_get_activation": (_i, [_vp, C.POINTER(_i)]),
    "mvlpt_trim": (_i, [_vp]),
    "mvlpt_debug_checksums": (_i, [_vp, _i, C.POINTER(C.c_uint64), _i]),
    "mvlpt_set_ln_fold": (_i, [_vp, _i, _i]),
    "mvlpt_set_resid_packed": (_i, [_vp, _i]),
    "mvlpt_set_vpt_dropout": (_i, [_vp, _vp, _i, _i, _i, _i]),
    "mvlpt_last_error": (C.c_char_p, [_vp]),
    "mvlpt_version": (C.c_char_p, []),
    "mvlpt_stream_create_cus": (_i, [_i, _i, C.POINTER(_vp)]),
    "mvlpt_stream_destroy": (_i, [_vp]),
    "mvlpt_stream_cus": (_i, [_vp]),
    "mvlpt_stream_set_cu_cap": (_i, [_vp, _i]),
    "mvlpt_load_frozen": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _vp]),
    "mvlpt_frozen_ready": (_i, [_vp]),
    "mvlpt_image_fwd": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "mvlpt_image_fwd_begin": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_image_fwd_resume": (_i, [_vp, _vp, _vp]),
    "mvlpt_image_fwd_abandon": (_i, [_vp]),
    "mvlpt_image_bwd": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mvlpt_text_fwd": (_i, [_vp, C.POINTER(MvlptTextJob), _vp, _vp]),
    "mvlpt_text_bwd": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mvlpt_text_workspace_bytes": (_i, [_vp, _i, _i, _i, C.POINTER(C.c_int64)]),
    "mvlpt_set_text_act_ckpt": (_i, [_vp, _i]),
    "mvlpt_set_text_grad_len": (_i, [_vp, _i, _i]),
    "mvlpt_set_text_shared_prefix": (_i, [_vp, _i]),
    "mvlpt_text_act_ckpt_plan": (_i, [_vp, C.POINTER(C.c_int32), _i, C.POINTER(_i)]),
    "mvlpt_text_encode_tokens": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "mvlpt_text_ensemble": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mvlpt_logits_fwd": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _vp]),
    "mvlpt_logits_bwd": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mvlpt_logits_ranged_fwd": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _vp]),
    "mvlpt_logits_ranged_bwd": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mvlpt_cross_entropy": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "mvlpt_op_gemm": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvlpt_op_gemm_ex": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_activation_fwd": (_i, [_i, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "mvlpt_op_activation_bwd": (_i, [_i, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _vp]),
    "mvlpt_op_gemm_route": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "mvlpt_op_gemm_split": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvlpt_op_layernorm_fwd_split": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_layernorm_bwd_split": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_attention32_fwd": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention32_bwd": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_pack_weight_mixed": (_i, [_i, _vp, _i, _i, _i, _vp, C.POINTER(C.c_int), _vp]),
    "mvlpt_op_gemm_mixed": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvlpt_op_cast_mixed": (_i, [_i, _vp, _vp, C.c_int64, _i, _vp]),
    "mvlpt_op_fold_vectors": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_gemm_ln_producer": (_i, [_i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, C.POINTER(C.c_int), _vp]),
    "mvlpt_op_gemm_folded": (_i, [_i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mvlpt_op_fold_weight": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp]),
    "mvlpt_op_respk_pack": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_assemble_packed": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_respk_unpack": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp]),
    "mvlpt_op_gemm_residp": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_int), _vp]),
    "mvlpt_op_layernorm_fwd_mixed": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_layernorm_bwd_mixed": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_attention32_fwd_mixed": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention32_bwd_mixed": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_layernorm_fwd": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_layernorm_bwd": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_attention_fwd": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention_bwd": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention_wide_fwd": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_cast": (_i, [_i, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_op_layernorm_fwd_ex": (_i, [_i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_layernorm_bwd_ex": (_i, [_i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_layernorm_route": (_i, [_i, _i, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "mvlpt_op_gemm_gelubwd_rows": (_i, [_i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_layernorm_bwd_rows": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention_bwd_rows": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention32_fwd_prefix": (_i, [_i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention32_bwd_prefix": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention_fwd_prefix": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_attention_bwd_prefix": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_cast_ex": (_i, [_i, _vp, _vp, C.c_int64, _i, _i, _vp, _vp]),
    "mvlpt_op_cast_to_f32": (_i, [_i, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_op_pack_weight": (_i, [_i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "mvlpt_op_patchify": (_i, [_i, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_patchify_route": (_i, [_i, _i, _i, _i]),
    "mvlpt_op_pack_conv_weight": (_i, [_vp, _i, _i, _i, _i, _vp, C.POINTER(C.c_int), _vp]),
    "mvlpt_op_conv2d": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "mvlpt_op_avgpool2x2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_nchw_to_nhwc8": (_i, [_vp, _i, _vp, _i, _i, _vp]),
    "mvlpt_op_attnpool_tokens": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_attnpool_query": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_assemble_prompts_ranged": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_gather_ctx_grad_ranged": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mvlpt_op_embed_tokens": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_ensemble_features": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_normalize_rows": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "mvlpt_op_sgemm_bt": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "mvlpt_op_grad_scale": (_i, [_vp, C.c_int64, _f, _vp, _vp]),
    "mvlpt_op_optim_step": (_i, [C.POINTER(MvlptOptimHyper), _vp, _vp, _vp, _vp, C.c_int64, _vp, _i, _vp, _vp, _vp]),
    "mvlpt_op_reduce_prompt_rows": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "mvlpt_op_gather_ctx_grad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mvlpt_op_attention_bwd_cls": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_copy_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_overwrite_rows": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "mvlpt_op_overwrite_ctx_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mvlpt_op_gather_zero_ctx_grad": (_i, [_i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mvlpt_op_assemble_tokens": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_op_assemble_prompts": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mvlpt_nearest_workspace_bytes": (_i, [_i, _i, _i, _i, _vp, C.POINTER(C.c_int64)]),
    "mvlpt_op_nearest_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_nearest_tokens": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mvlpt_tpt_workspace_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_int64)]),
    "mvlpt_op_tpt_head_fwd": (_i, [_vp, _vp, _f, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_op_tpt_head_bwd": (_i, [_vp, _f, _i, _i, _i, _i, _i, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_tip_workspace_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int64)]),
    "mvlpt_op_tip_logits": (_i, [_vp, _vp, _vp, _vp, _f, _f, _f, _i, _i, _i, _i, _vp, _vp]),
    "mvlpt_op_tip_train_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _i, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_op_tip_train_bwd": (_i, [_vp, _f, _f, _i, _i, _i, _i, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_op_tip_search": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_int64, _vp]),
    "mvlpt_op_eval_count": (_i, [_vp, C.c_int64, _i, _i, _vp, _i, C.c_int64, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _vp]),
    "mvlpt_op_eval_rank_columns": (_i, [_vp, C.c_int64, _i, _i, _vp, _i, C.c_int64, _vp, _i, C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp,
                                        _vp, C.c_int64, _vp]),
    "mvlpt_eval_workspace_bytes": (_i, [_i, _i, _vp, C.POINTER(C.c_int64)]),
    "mvlpt_softmax_reg_workspace_bytes": (_i, [_i, _i, _i, C.POINTER(C.c_size_t)]),
    "mvlpt_op_softmax_reg_eval": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.c_double, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mvlpt_op_softmax_reg_predict": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mvlpt_preprocess": (_i, [_vp, _vp, C.c_int64, C.POINTER(MvlptImageDesc), _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _i, _vp, _vp]),
    "mvlpt_preprocess_aug": (_i, [_vp, _vp, C.c_int64, C.POINTER(MvlptImageDesc), C.POINTER(MvlptAugmentDesc), _i, _i, _i, _i,
                                  C.POINTER(_f), C.POINTER(_f), _vp, _i, _vp, _vp]),
    "mvlpt_jpeg_probe": (_i, [_vp, C.c_int64, C.POINTER(MvlptJpegInfo)]),
    "mvlpt_jpeg_workspace_bytes": (_i, [C.POINTER(MvlptJpegInfo), _i, C.POINTER(C.c_int64)]),
    "mvlpt_jpeg_decode": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i, _vp, C.c_int64, C.POINTER(C.c_int64), _vp, _vp]),
    "mvlpt_op_jpeg_entropy": (_i, [_vp, C.c_int64, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp]),
    "mvlpt_op_jpeg_idct": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "mvlpt_op_jpeg_colour": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _i, _i, _i, _i, _i, _vp, _vp]),
    "mvlpt_profile_begin": (_i, [_vp, _i]),
    "mvlpt_profile_pause": (_i, [_vp, _i]),
    "mvlpt_profile_end": (_i, [_vp, C.POINTER(MvlptKernelStat), _i]),
}


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.isfile(path):
        raise ImportError(
            f"{path} not found: build the HIP extension first (`make` at the repo root, or "
            "`__graft_entry__.build()`); mvlpt_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    return lib


lib = load_library()


def last_error(handle=None) -> str:
    msg = lib.mvlpt_last_error(handle)
    return msg.decode() if msg else ""


def check(rc: int, handle=None, what: str = "") -> None:
    if rc != 0:
        raise RuntimeError(f"libmvlpt_hip {what} failed (code {rc}): {last_error(handle) or last_error(None)}")
