"""ctypes binding of ``libsamrs_hip.so`` (C ABI: ``include/samrs_hip.h``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every computation happens in
the library.  There is NO fallback: if the shared library is missing, or there is no HIP device,
importing / constructing fails loudly.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .synth import SamConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsamrs_hip.so")

PREC_BF16, PREC_F16 = 0, 1
PRECISIONS = {"bf16": PREC_BF16, "f16": PREC_F16, "fp16": PREC_F16}

ABI_VERSION = 5
POLYGON_EPS_Q_MAX = 16384          # samrs_simplify_polygons: eps_q in sixteenths of a pixel, 1 .. 16384
REGION_MODES = {"holes": 1, "islands": 2, "both": 3}        # enum samrs_region_mode
OVERLAP_RULES = {"logit": 1, "smallest": 2, "priority": 3}  # enum samrs_overlap_rule
# "split" option bits (include/samrs_hip.h): rounding points that run as a two-term operand split
SPLIT_PATCH, SPLIT_NECK, SPLIT_OI, SPLIT_UP, SPLIT_DEFAULT = 1, 2, 4, 8, 15
SPLIT_ATTN, SPLIT_MLP, SPLIT_ATTN_V, SPLIT_LIN2, SPLIT_ALL = 16, 32, 64, 128, 255          # reference-grade bits: set before the weights are loaded
# (64 = the attention-side split restricted to the v third of qkv + proj; option "split_depth" = leading blocks they apply to)

OK, ERR_NOT_SET, ERR_BAD_SHAPE, ERR_BAD_ARG, ERR_HIP, ERR_BAD_WEIGHTS, ERR_CAPACITY, ERR_PRECISION, ERR_RANGE = 0, -1, -2, -3, -4, -5, -6, -7, -8


class samrs_config(C.Structure):
    _fields_ = [
        ("embed_dim", C.c_int32), ("depth", C.c_int32), ("num_heads", C.c_int32),
        ("n_global", C.c_int32), ("global_attn_indexes", C.c_int32 * 8),
        ("img_size", C.c_int32), ("patch_size", C.c_int32), ("window_size", C.c_int32),
        ("out_chans", C.c_int32), ("max_images", C.c_int32), ("max_prompts", C.c_int32),
        ("max_points", C.c_int32), ("precision", C.c_int32),
    ]


_lib = None

# samrs_predict_multi(e, n_images, slots, prompt_offsets, boxes, point_coords, point_labels, n_points, mask_input, multimask,
#                     return_logits, in_hw, orig_hw, masks_out, iou_out, lowres_out, stream)
PREDICT_MULTI_ARGTYPES = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                          C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p,
                          C.c_void_p, C.c_void_p]


def load_library() -> C.CDLL:
    """Loads the in-tree shared library; raises if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SAMRS_LIB_PATH", LIB_PATH)          # A/B builds of the same ABI (tools/, never the tests)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `make -C samrs_amd/csrc` (or __graft_entry__.build()). "
            "samrs_amd has no CPU / PyTorch fallback by design.")
    lib = C.CDLL(path)
    vp, ip, fp = C.c_void_p, C.c_int, C.c_float
    lib.samrs_abi_version.restype = ip
    lib.samrs_create.restype = vp
    lib.samrs_create.argtypes = [C.POINTER(samrs_config), ip, C.c_char_p, ip]
    lib.samrs_destroy.argtypes = [vp]
    lib.samrs_destroy.restype = None
    lib.samrs_last_error.argtypes = [vp]
    lib.samrs_last_error.restype = C.c_char_p
    lib.samrs_load_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), ip]
    lib.samrs_finalize_weights.argtypes = [vp, vp]
    lib.samrs_set_images.argtypes = [vp, vp, ip, ip, ip, ip, vp]
    lib.samrs_set_images_ragged.argtypes = [vp, C.POINTER(vp), C.POINTER(ip), C.POINTER(ip), ip, ip, vp]
    lib.samrs_get_embedding.argtypes = [vp, ip, vp, vp]
    lib.samrs_set_embedding.argtypes = [vp, ip, vp, vp]
    lib.samrs_reset_image.argtypes = [vp, ip]
    lib.samrs_predict.argtypes = [vp, ip, ip, vp, vp, vp, ip, vp, ip, ip, ip, ip, ip, ip, vp, vp, vp, vp]
    lib.samrs_predict_multi.argtypes = PREDICT_MULTI_ARGTYPES
    lib.samrs_paint.argtypes = [vp, vp, vp, ip, ip, ip, vp, vp, vp, vp, ip, vp]
    lib.samrs_debug_encoder_prefix.argtypes = [vp, vp, ip, ip, ip, ip, vp, vp]
    lib.samrs_debug_encoder_prefix.restype = ip
    lib.samrs_debug_time_dominant_kernel.argtypes = [vp, ip]
    lib.samrs_debug_time_dominant_kernel.restype = ip
    lib.samrs_debug_dominant_kernel_time.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
    lib.samrs_debug_dominant_kernel_time.restype = ip
    lib.samrs_resample_pass_u8.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    lib.samrs_resample_pass_u8.restype = ip
    lib.samrs_rbox_mask_prompt.argtypes = [vp, ip, ip, ip, ip, ip, ip, ip, ip, vp, vp]
    lib.samrs_rbox_mask_prompt.restype = ip
    lib.samrs_rbox_mask_prompt_rule.argtypes = [vp, ip, ip, ip, ip, ip, ip, ip, ip, ip, vp, vp]
    lib.samrs_rbox_mask_prompt_rule.restype = ip
    lib.samrs_k_gemm.argtypes = [ip, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_gemm_f32.argtypes = [vp, ip, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_gemm_stats.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, vp]
    lib.samrs_k_gemm_fold.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, vp]
    lib.samrs_k_ln_rowstat.argtypes = [vp, vp, ip, fp, vp]
    lib.samrs_k_ln_fold_weight.argtypes = [ip, vp, vp, vp, vp, vp, vp, vp, ip, ip, vp]
    lib.samrs_k_rowstats_convert.argtypes = [ip, vp, vp, vp, ip, ip, vp]
    lib.samrs_set_option.argtypes = [vp, C.c_char_p, ip]
    lib.samrs_get_option.argtypes = [vp, C.c_char_p, C.POINTER(ip)]
    lib.samrs_rle_encode.argtypes = [vp, vp, ip, ip, ip, vp, C.c_int64, vp, vp, vp]
    lib.samrs_rle_decode.argtypes = [vp, vp, C.c_int64, vp, ip, ip, ip, vp, vp, vp, vp]
    lib.samrs_rle_decode.restype = ip
    lib.samrs_scene_claim.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, ip, vp, vp, vp, vp, ip, vp]
    lib.samrs_scene_resolve.argtypes = [vp, vp, vp, ip, ip, ip, vp, vp]
    lib.samrs_rle_encode_placed.argtypes = [vp, vp, ip, ip, ip, ip, ip, ip, ip, vp, C.c_int64, vp, vp, vp]
    for name in ("samrs_scene_claim", "samrs_scene_resolve", "samrs_rle_encode_placed"):
        getattr(lib, name).restype = ip
    lib.samrs_k_convert_split.argtypes = [ip, vp, vp, vp, C.c_int64, vp]
    lib.samrs_select_best.argtypes = [vp, vp, vp, ip, ip, ip, ip, vp, vp, vp, vp]
    lib.samrs_gt_match.argtypes = [vp, vp, ip, ip, ip, vp, vp, vp, vp, vp, vp]
    lib.samrs_clean_masks.argtypes = [vp, vp, ip, ip, ip, ip, ip, vp, vp, vp]
    lib.samrs_clean_masks.restype = ip
    lib.samrs_k_region_labels.argtypes = [vp, ip, ip, ip, ip, vp, vp]
    lib.samrs_k_region_labels.restype = ip
    lib.samrs_mask_boxes.argtypes = [vp, vp, ip, ip, ip, ip, ip, vp, vp, vp, vp]
    lib.samrs_k_mask_row_extents.argtypes = [vp, ip, ip, ip, vp, vp]
    lib.samrs_k_mask_hull.argtypes = [vp, ip, ip, ip, ip, ip, vp, vp, ip, vp, vp]
    for name in ("samrs_mask_boxes", "samrs_k_mask_row_extents", "samrs_k_mask_hull"):
        getattr(lib, name).restype = ip
    lib.samrs_mask_polygons.argtypes = [vp, vp, ip, ip, ip, ip, ip, ip, vp, C.c_int64, vp, C.c_int64, vp, vp, vp]
    lib.samrs_k_polygon_edges.argtypes = [vp, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp]
    lib.samrs_k_polygon_ranks.argtypes = [vp, ip, ip, ip, ip, vp, vp, vp, vp, vp]
    lib.samrs_k_polygon_scratch_bytes.argtypes = [ip, ip, ip, ip]
    lib.samrs_k_polygon_edge_stride.argtypes = [ip, ip, ip]
    for name in ("samrs_mask_polygons", "samrs_k_polygon_edges", "samrs_k_polygon_ranks"):
        getattr(lib, name).restype = ip
    lib.samrs_k_polygon_scratch_bytes.restype = C.c_int64
    lib.samrs_k_polygon_edge_stride.restype = C.c_int64
    lib.samrs_simplify_polygons.argtypes = [vp, vp, vp, vp, ip, ip, vp, vp]
    lib.samrs_simplify_polygons.restype = ip
    lib.samrs_k_polygon_simplify_scratch_bytes.argtypes = [ip, C.c_int64, C.c_int64]
    lib.samrs_k_polygon_simplify_scratch_bytes.restype = C.c_int64
    lib.samrs_k_polygon_simplify_keep.argtypes = [vp, vp, vp, ip, ip, C.c_int64, C.c_int64, vp, vp, vp, vp]
    lib.samrs_k_polygon_simplify_keep.restype = ip
    lib.samrs_fill_polygons.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, ip, vp, vp, vp, vp]
    lib.samrs_fill_polygons.restype = ip
    lib.samrs_score_masks.argtypes = [vp, vp, ip, ip, ip, ip, ip, fp, vp, vp, vp]
    lib.samrs_filter_masks.argtypes = [vp, vp, ip, ip, ip, vp, vp, fp, fp, fp, vp, vp]
    lib.samrs_resolve_overlaps.argtypes = [vp, vp, ip, ip, ip, ip, vp, ip, ip, vp, vp, vp, vp, vp]
    lib.samrs_mask_pack_bits.argtypes = [vp, vp, ip, ip, ip, vp, vp]
    lib.samrs_label_pack_bits.argtypes = [vp, vp, vp, ip, ip, ip, vp, vp]
    lib.samrs_mask_pair_counts.argtypes = [vp, vp, ip, vp, ip, C.c_int64, vp, vp, vp, vp]
    lib.samrs_coco_match.argtypes = [vp, vp, vp, vp, vp, ip, ip, ip, C.POINTER(C.c_double), ip, C.POINTER(C.c_double), ip, ip,
                                     vp, vp, vp, vp, vp, vp]
    lib.samrs_coco_match_min.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, C.POINTER(C.c_double), ip, C.POINTER(C.c_double), ip, ip,
                                         vp, vp, vp, vp, vp, vp]
    lib.samrs_mask_boundary_bits.argtypes = [vp, vp, ip, ip, ip, ip, vp, vp]
    for name in ("samrs_score_masks", "samrs_filter_masks", "samrs_resolve_overlaps", "samrs_mask_pack_bits", "samrs_label_pack_bits",
                 "samrs_mask_pair_counts", "samrs_coco_match", "samrs_coco_match_min", "samrs_mask_boundary_bits"):
        getattr(lib, name).restype = ip
    lib.samrs_png_encode_labels.argtypes = [vp, vp, ip, ip, ip, vp, vp, C.c_int64, vp, vp, vp]
    lib.samrs_blend_labels.argtypes = [vp, vp, vp, vp, fp, vp, ip, ip, ip, vp]
    lib.samrs_png_encode_rgb.argtypes = [vp, vp, ip, ip, ip, ip, vp, C.c_int64, vp, vp, vp]
    for name in ("samrs_blend_labels", "samrs_png_encode_rgb"):
        getattr(lib, name).restype = ip
    lib.samrs_k_upscaler_fused.argtypes = [ip, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_convert.argtypes = [ip, vp, vp, C.c_int64, vp]
    lib.samrs_k_layernorm.argtypes = [ip, vp, vp, vp, fp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_window_attention.argtypes = [ip, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_window_attention_lo.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, C.c_uint32, vp]
    lib.samrs_k_global_attention.argtypes = [ip, vp, vp, vp, vp, ip, ip, ip, ip, vp]
    lib.samrs_k_postprocess.argtypes = [vp, ip, ip, ip, ip, ip, ip, ip, vp, vp]
    lib.samrs_k_neck_im2col.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.samrs_k_neck_im2col.restype = ip
    lib.samrs_k_gemm_gln.argtypes = [ip, vp, vp, vp, vp, vp, ip, ip, ip, vp, vp, vp]
    lib.samrs_k_upscale2_masks.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_gemm_split3.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
    i64 = C.c_int64
    lib.samrs_k_mx_scale_bytes.argtypes = [ip, ip, ip]
    lib.samrs_k_mx_scale_bytes.restype = i64
    lib.samrs_k_mx4_pack.argtypes = [ip, vp, vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_gemm_mx.argtypes = [ip, vp, vp, vp, vp, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, vp]
    lib.samrs_k_layernorm_mx.argtypes = [ip, vp, vp, vp, fp, vp, ip, ip, vp, vp, vp, vp, vp]
    lib.samrs_k_attention_mx.argtypes = [ip, ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, vp, vp, vp, vp, vp]
    lib.samrs_k_gemm_mx_gelu_mxout.argtypes = [ip, vp, vp, vp, vp, ip, ip, ip, ip, vp, vp, vp, vp, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp]
    for name in ("samrs_k_mx4_pack", "samrs_k_gemm_mx", "samrs_k_layernorm_mx", "samrs_k_attention_mx", "samrs_k_gemm_mx_gelu_mxout"):
        getattr(lib, name).restype = ip
    # decoder kernels, one each (include/samrs_hip_internal.h; tests/test_decoder_kernels_gpu.py)
    lib.samrs_k_prompt_tokens.argtypes = [vp, vp, vp, ip, ip, fp, vp, vp, vp, vp, vp, vp, vp, ip, vp]
    lib.samrs_k_dense_pe.argtypes = [vp, vp, ip, vp]
    lib.samrs_k_mask_embed.argtypes = [vp] * 12 + [ip, ip, vp]
    lib.samrs_k_fill_slot_table.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), ip, vp, vp]
    lib.samrs_k_make_keys.argtypes = [ip, vp, vp, vp, vp, vp, ip, ip, ip, vp, vp]
    lib.samrs_k_token_self_attn.argtypes = [vp, vp, vp, vp, ip, ip, ip, ip, vp]
    lib.samrs_k_t2i_workspace_floats.argtypes = [ip, ip]
    lib.samrs_k_t2i_workspace_floats.restype = i64
    lib.samrs_k_t2i_attention.argtypes = [ip, vp, vp, vp, ip, i64, vp, vp, ip, ip, ip, ip, ip, vp, vp]
    lib.samrs_k_i2t_attention.argtypes = [ip, vp, ip, i64, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    lib.samrs_k_i2t_fused.argtypes = [ip, vp, ip, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, fp, vp, vp, vp, ip, ip, ip, ip, ip, vp, vp]
    lib.samrs_k_group_ln_gelu.argtypes = [ip, vp, vp, vp, fp, vp, i64, ip, ip, vp]
    lib.samrs_k_mask_product.argtypes = [ip, vp, vp, vp, ip, ip, ip, ip, ip, vp]
    for name in ("samrs_k_prompt_tokens", "samrs_k_dense_pe", "samrs_k_mask_embed", "samrs_k_fill_slot_table", "samrs_k_make_keys",
                 "samrs_k_token_self_attn", "samrs_k_t2i_attention", "samrs_k_i2t_attention", "samrs_k_i2t_fused",
                 "samrs_k_group_ln_gelu", "samrs_k_mask_product", "samrs_debug_copy_buffer", "samrs_debug_outlier_columns"):
        getattr(lib, name).restype = ip
    lib.samrs_debug_copy_buffer.argtypes = [vp, C.c_char_p, vp, C.c_size_t, vp]
    lib.samrs_debug_outlier_columns.argtypes = [vp, ip, ip, C.POINTER(C.c_int32)]
    if hasattr(lib, "samrs_debug_gemm_choice"):       # an older build of the same ABI (SAMRS_LIB_PATH: A/B runs) has no such probe
        lib.samrs_debug_gemm_choice.argtypes = [ip] * 10 + [C.POINTER(C.c_int32)]
        lib.samrs_debug_gemm_choice.restype = None
    lib.samrs_get_slot_info.argtypes = [vp, ip, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    # checkpoint audit (samrs_hip.h samrs_audit_*; the two kernels alone: samrs_hip_internal.h)
    lib.samrs_audit_site_count.argtypes = [vp, C.POINTER(ip)]
    lib.samrs_audit_site_name.argtypes = [vp, ip, C.c_char_p, ip, C.POINTER(ip)]
    lib.samrs_audit_read_profile.argtypes = [vp, vp, ip]
    lib.samrs_audit_read_columns.argtypes = [vp, ip, vp, vp, C.POINTER(C.c_int64)]
    lib.samrs_k_range_profile.argtypes = [ip, vp, C.c_long, ip, ip, vp, vp]
    lib.samrs_k_column_stats.argtypes = [ip, vp, ip, ip, ip, vp, vp, vp, vp]
    lib.samrs_k_audit_rows_per_partial.argtypes = []
    for name in ("samrs_audit_site_count", "samrs_audit_site_name", "samrs_audit_read_profile", "samrs_audit_read_columns",
                 "samrs_k_range_profile", "samrs_k_column_stats", "samrs_k_audit_rows_per_partial"):
        getattr(lib, name).restype = ip
    # the outlier-column kernels and the padded-row / EXT-stage GEMM launches, one each (tests/test_outlier_kernels_gpu.py)
    if hasattr(lib, "samrs_k_gemm_ext"):              # an older build of the same ABI (SAMRS_LIB_PATH: A/B runs) has none of them
        lib.samrs_k_gemm_ld.argtypes = [ip, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
        lib.samrs_k_gemm_ext.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, vp]
        lib.samrs_k_layernorm_ext.argtypes = [ip, vp, vp, vp, fp, vp, ip, ip, ip, vp, ip, ip, vp]
        lib.samrs_k_outlier_weight_ext.argtypes = [ip, vp, ip, ip, vp, ip, vp, ip, ip, vp]
        lib.samrs_k_outlier_side_weight.argtypes = [ip, vp, vp, ip, ip, vp, ip, vp, ip, vp, ip, vp, vp]
        lib.samrs_k_outlier_gather.argtypes = [vp, vp, ip, vp, ip, vp, ip, vp]
        lib.samrs_k_outlier_side_gemm.argtypes = [ip, vp, ip, vp, vp, ip, ip, vp, vp]
        lib.samrs_k_weight_norms.argtypes = [vp, ip, ip, vp, vp, vp]
        lib.samrs_k_range_scan.argtypes = [ip, vp, i64, ip, ip, vp, vp]
        for name in ("samrs_k_gemm_ld", "samrs_k_gemm_ext", "samrs_k_layernorm_ext", "samrs_k_outlier_weight_ext", "samrs_k_outlier_side_weight",
                     "samrs_k_outlier_gather", "samrs_k_outlier_side_gemm", "samrs_k_weight_norms", "samrs_k_range_scan"):
            getattr(lib, name).restype = ip
    # the fp32 GEMM batch, image ingest, embedding hand-over and reference-grade GELU, one each (tests/test_token_side_kernels_gpu.py)
    if hasattr(lib, "samrs_k_gemm_f32_batch"):        # an older build of the same ABI (SAMRS_LIB_PATH: A/B runs) has none of them
        lib.samrs_k_gemm_f32_batch.argtypes = [vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, ip, ip, vp]
        lib.samrs_k_patch_im2col.argtypes = [ip, vp, vp, vp, ip, ip, ip, ip, ip, vp]
        lib.samrs_k_transpose_f32.argtypes = [vp, vp, ip, ip, vp]
        lib.samrs_k_gelu_split.argtypes = [ip, vp, vp, vp, i64, vp]
        for name in ("samrs_k_gemm_f32_batch", "samrs_k_patch_im2col", "samrs_k_transpose_f32", "samrs_k_gelu_split"):
            getattr(lib, name).restype = ip
    for name in ("samrs_load_weight", "samrs_finalize_weights", "samrs_set_images", "samrs_set_images_ragged", "samrs_get_embedding",
                 "samrs_set_embedding", "samrs_reset_image", "samrs_predict", "samrs_predict_multi", "samrs_paint", "samrs_k_gemm",
                 "samrs_k_gemm_f32", "samrs_k_convert", "samrs_k_layernorm", "samrs_k_window_attention",
                 "samrs_k_window_attention_lo", "samrs_k_global_attention", "samrs_k_postprocess", "samrs_k_gemm_gln", "samrs_k_upscale2_masks",
                 "samrs_k_gemm_stats", "samrs_k_gemm_fold", "samrs_k_ln_fold_weight", "samrs_k_rowstats_convert", "samrs_k_ln_rowstat",
                 "samrs_set_option", "samrs_get_option", "samrs_rle_encode", "samrs_k_convert_split", "samrs_select_best", "samrs_gt_match",
                 "samrs_png_encode_labels", "samrs_k_upscaler_fused", "samrs_k_gemm_split3", "samrs_get_slot_info"):
        getattr(lib, name).restype = ip
    if lib.samrs_abi_version() != ABI_VERSION:
        raise ImportError("libsamrs_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


# samrs_rle_status (samrs_hip.h): the per-mask status codes of samrs_rle_decode
RLE_STATUS = ("OK", "ABSENT", "RANGE", "BAD_CHAR", "TRUNCATED", "BAD_COUNT", "BAD_SUM")


PNG_RGB_BLOCK_BYTES = 1 << 20      # filtered bytes per deflate block of samrs_png_encode_rgb (SAMRS_PNG_RGB_BLOCK_BYTES in samrs_hip.h)


def png_rgb_bound(h: int, w: int) -> int:
    """The worst-case size samrs_hip.h documents for one file of samrs_png_encode_rgb, rounded up to the 16 bytes files are
    aligned to: 9 bits per filtered byte, 4498 + 9 bits per deflate block, 63 bytes of framing."""
    n = (3 * int(w) + 1) * int(h)
    blocks = -(-n // PNG_RGB_BLOCK_BYTES)
    return (63 + -(-(9 * n + blocks * (4498 + 9)) // 8) + 15) & ~15


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class EngineError(RuntimeError):
    pass


def multi_call_args(slots: Sequence[int], counts: Sequence[int], input_sizes: Sequence[Sequence[int]],
                    original_sizes: Sequence[Sequence[int]], n_rows: int) -> Tuple[List[int], List[int], List[int], List[int]]:
    """Host-side checks of a predict_multi call (nothing touches the device): one slot, prompt count, input size and original
    size per image, counts summing to the rows of the prompt tensors -> (slots, prompt_offsets, in_hw, orig_hw) flat lists."""
    n_img = len(slots)
    if n_img < 1:
        raise ValueError("predict_multi needs at least one image")
    if not (len(counts) == len(input_sizes) == len(original_sizes) == n_img):
        raise ValueError(f"predict_multi: {n_img} slots but {len(counts)} prompt counts, {len(input_sizes)} input sizes and "
                         f"{len(original_sizes)} original sizes")
    offsets = [0]
    for c in counts:
        if int(c) < 0:
            raise ValueError(f"predict_multi: negative prompt count {c}")
        offsets.append(offsets[-1] + int(c))
    if offsets[-1] != n_rows:
        raise ValueError(f"predict_multi: the prompt counts sum to {offsets[-1]} but the prompt tensors have {n_rows} rows")
    in_hw, orig_hw = [], []
    for name, sizes, out in (("input", input_sizes, in_hw), ("original", original_sizes, orig_hw)):
        for hw in sizes:
            if len(hw) != 2:
                raise ValueError(f"predict_multi: every {name} size must be (h, w), got {tuple(hw)}")
            out.extend((int(hw[0]), int(hw[1])))
    return [int(v) for v in slots], offsets, in_hw, orig_hw


def _prompt_rows(boxes, point_coords, mask_input) -> Optional[int]:
    """Batch size of a prompt batch as the shapes state it (None: no prompt), before any conversion."""
    if point_coords is not None:
        return int(point_coords.shape[0]) if point_coords.dim() == 3 else None
    if boxes is not None:
        return boxes.numel() // 4
    if mask_input is not None:
        return int(mask_input.shape[0])
    return None


class PrecisionError(EngineError):
    """``multimask_output=True`` on an embedding that was encoded below the operand-split mode this model's multimask
    outputs need (SAMRS_ERR_PRECISION; ``Engine.get_slot_info``).  Re-encode the image in the engine's default mode
    (``SamPredictor.set_image`` does), or accept the reduced mode with ``engine.set_option("allow_reduced", 1)``."""


class OperandRangeError(EngineError):
    """Option ``range_check`` = 2: the encoder pass of ``set_image`` / ``set_images`` saturated values of an MFMA operand tensor
    (f16 tops out at 65504 and every conversion on the path saturates there; SAMRS_ERR_RANGE).  The checkpoint's activations do
    not fit the f16 operand type: build the model with ``precision="bf16"``."""


class Engine:
    """One engine handle = one GPU's weights + workspaces (``samrs_engine_t``)."""

    def __init__(self, cfg: SamConfig, device: torch.device, precision: str = "f16", max_images: int = 1,
                 max_prompts: int = 64, max_points: int = 4):
        if device.type != "cuda":
            raise EngineError("samrs_amd runs on a HIP device only (torch device type 'cuda'); there is no CPU path")
        if not torch.cuda.is_available():
            raise EngineError("no HIP device visible to PyTorch")
        self.lib = load_library()
        self.cfg = cfg
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        self.precision = precision
        self.max_images, self.max_prompts, self.max_points = max_images, max_prompts, max_points
        c = samrs_config()
        c.embed_dim, c.depth, c.num_heads = cfg.embed_dim, cfg.depth, cfg.num_heads
        c.n_global = len(cfg.global_attn_indexes)
        for i, g in enumerate(cfg.global_attn_indexes):
            c.global_attn_indexes[i] = g
        c.img_size, c.patch_size, c.window_size, c.out_chans = cfg.img_size, cfg.patch_size, cfg.window_size, cfg.out_chans
        c.max_images, c.max_prompts, c.max_points = max_images, max_prompts, max_points
        c.precision = PRECISIONS[precision]
        err = C.create_string_buffer(512)
        with torch.cuda.device(self.device):
            self.handle = self.lib.samrs_create(C.byref(c), self.device.index, err, 512)
        if not self.handle:
            raise EngineError("samrs_create failed: " + err.value.decode())
        self._audit_done = None        # start_audit: called once when the engine has profiled its passes

    # -- error mapping: same exception types / messages as the reference (predictor.py:133-134 ...)
    def _check(self, rc: int) -> None:
        if rc == OK:
            return
        msg = self.lib.samrs_last_error(self.handle).decode()
        if rc == ERR_NOT_SET:
            raise RuntimeError(msg)
        if rc in (ERR_BAD_SHAPE, ERR_BAD_ARG):
            raise AssertionError(msg)
        if rc == ERR_PRECISION:
            raise PrecisionError(msg)
        if rc == ERR_RANGE:
            raise OperandRangeError(msg)
        raise EngineError(f"libsamrs_hip error {rc}: {msg}")

    # -- per-engine options (include/samrs_hip.h: "split", "decoder_fusion", "ln_fold", "gemm_variant")
    def set_option(self, name: str, value: int) -> None:
        self._check(self.lib.samrs_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int()
        self._check(self.lib.samrs_get_option(self.handle, name.encode(), C.byref(v)))
        return v.value

    @contextlib.contextmanager
    def options(self, **values: int):
        """Options in force for the calls made inside the block only (a pipeline's operand-split mode must not outlive the
        pipeline's own calls: the engine is shared with every SamPredictor built on the same model)."""
        old = {k: self.get_option(k) for k in values}
        try:
            for k, v in values.items():
                if v != old[k]:
                    self.set_option(k, v)
            yield self
        finally:
            for k, v in old.items():
                if self.get_option(k) != v:
                    self.set_option(k, v)

    def get_slot_info(self, slot: int = 0) -> Dict[str, int]:
        """{"is_set", "split", "split_depth"} of an embedding slot: the operand-split mode its image was encoded in (-1: the
        embedding was installed by set_embedding)."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.samrs_get_slot_info(self.handle, slot, C.byref(a), C.byref(b), C.byref(c)))
        return {"is_set": int(a.value), "split": int(b.value), "split_depth": int(c.value)}

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.samrs_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Strict load (build_sam.py:103-106): every key / shape of the reference state_dict."""
        for name, t in sd.items():
            a = np.ascontiguousarray(t.detach().to(torch.float32).cpu().numpy())
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.samrs_load_weight(self.handle, name.encode(), a.ctypes.data, shape, a.ndim))
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_finalize_weights(self.handle, _stream()))

    def set_images(self, images_u8: torch.Tensor, slot0: int = 0) -> None:
        """images_u8: uint8 [n, H, W, 3] on this device, long side == img_size."""
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3
        assert images_u8.is_cuda and images_u8.is_contiguous()
        n, h, w, _ = images_u8.shape
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_set_images(self.handle, images_u8.data_ptr(), n, h, w, slot0, _stream()))
        if self._audit_done is not None:
            self._audit_poll()

    def set_images_ragged(self, images_u8, slot0: int = 0) -> None:
        """One encoder pass over tiles of DIFFERENT sizes: a sequence of uint8 [H_i, W_i, 3] device tensors, each with
        long side == img_size (samrs_set_images_ragged)."""
        n = len(images_u8)
        for t in images_u8:
            assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[-1] == 3 and t.is_cuda and t.is_contiguous()
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in images_u8])
        hs = (C.c_int * n)(*[int(t.shape[0]) for t in images_u8])
        ws = (C.c_int * n)(*[int(t.shape[1]) for t in images_u8])
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_set_images_ragged(self.handle, ptrs, hs, ws, n, slot0, _stream()))
        if self._audit_done is not None:
            self._audit_poll()

    def debug_encoder_prefix(self, images_u8: torch.Tensor, n_blocks: int) -> torch.Tensor:
        """Test hook: residual stream [n, 64, 64, D] after patch embed + the first n_blocks blocks."""
        n, h, w, _ = images_u8.shape
        out = torch.empty(n, self.cfg.grid, self.cfg.grid, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_debug_encoder_prefix(self.handle, images_u8.data_ptr(), n, h, w, n_blocks,
                                                            out.data_ptr(), _stream()))
        return out

    def outlier_columns(self, block: int, gemm: int):
        """Test hook: the outlier K-columns the engine picked for block GEMM `gemm` (0 qkv, 1 lin1, 2 lin2, 3 proj) of encoder block `block`."""
        buf = (C.c_int32 * 32)()
        n = self.lib.samrs_debug_outlier_columns(self.handle, block, gemm, buf)
        if n < 0:
            self._check(n)
        return [int(buf[i]) for i in range(n)]

    # -- checkpoint audit (options "range_profile" / "audit_passes"; samrs_amd/audit.py turns the numbers into a report)
    PROFILE_WORDS = 48

    def audit_sites(self) -> List[Tuple[str, int]]:
        """(name, K of the site's column statistics or 0) of every audit site, in data-flow order (samrs_audit_site_name)."""
        n, k = C.c_int(), C.c_int()
        self._check(self.lib.samrs_audit_site_count(self.handle, C.byref(n)))
        buf = C.create_string_buffer(64)
        out = []
        for i in range(n.value):
            self._check(self.lib.samrs_audit_site_name(self.handle, i, buf, 64, C.byref(k)))
            out.append((buf.value.decode(), int(k.value)))
        return out

    def range_profile(self, reset: bool = False) -> np.ndarray:
        """int64 [n_sites, 48]: the profile rows accumulated so far (samrs_audit_read_profile; synchronises the device).  ``reset``
        clears the whole audit state afterwards, column statistics included."""
        rows = np.zeros((len(self.audit_sites()), self.PROFILE_WORDS), dtype=np.int64)
        self._check(self.lib.samrs_audit_read_profile(self.handle, rows.ctypes.data, int(bool(reset))))
        return rows

    def column_stats(self, site) -> Dict[str, object]:
        """{"sumsq" float64 [K], "max_abs" float32 [K], "n_rows"} of one block-GEMM operand site (index or name) after passes profiled
        with ``range_profile`` = 2 (samrs_audit_read_columns); AssertionError (SAMRS_ERR_BAD_ARG) where there is nothing to read."""
        sites = self.audit_sites()
        if isinstance(site, str):
            names = [s[0] for s in sites]
            if site not in names:
                raise KeyError(f"no audit site {site!r}")
            site = names.index(site)
        k = sites[site][1] if 0 <= site < len(sites) else 0
        sumsq, max_abs, n_rows = np.zeros(max(k, 1), np.float64), np.zeros(max(k, 1), np.float32), C.c_int64()
        self._check(self.lib.samrs_audit_read_columns(self.handle, int(site), sumsq.ctypes.data, max_abs.ctypes.data, C.byref(n_rows)))
        return {"sumsq": sumsq, "max_abs": max_abs, "n_rows": int(n_rows.value)}

    def start_audit(self, passes: int, done=None) -> None:
        """Profile the next ``passes`` encoder passes (option ``audit_passes``); ``done(engine)`` is called once, from the
        set_images* call after which the engine has switched the profile off by itself."""
        self.set_option("audit_passes", int(passes))
        self._audit_done = done if passes > 0 else None

    def _audit_poll(self) -> None:
        if self.get_option("audit_passes") == 0:          # a host-side read: no synchronisation
            done, self._audit_done = self._audit_done, None
            done(self)

    def debug_copy_buffer(self, name: str, dst: torch.Tensor) -> torch.Tensor:
        """Test hook: fill `dst` (a contiguous tensor on this engine's device) with the leading dst.numel() elements of the named
        internal decoder buffer (TOK0, DENSE, K0F, KF, KE, Q, HYPER, ...: samrs_hip_internal.h).  The caller picks dtype and shape."""
        if not dst.is_contiguous() or dst.device != torch.device(self.device):
            raise ValueError("debug_copy_buffer: dst must be a contiguous tensor on the engine's device")
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_debug_copy_buffer(self.handle, name.encode(), dst.data_ptr(), dst.numel() * dst.element_size(),
                                                         _stream()))
        return dst

    def time_dominant_kernel(self, enable: bool) -> None:
        self._check(self.lib.samrs_debug_time_dominant_kernel(self.handle, int(enable)))

    def dominant_kernel_time(self):
        """(average ms, launches, N, K) of the MLP lin1+GELU GEMM launches timed since the last call."""
        ms, n, m, nn, kk = C.c_float(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.samrs_debug_dominant_kernel_time(self.handle, C.byref(ms), C.byref(n), C.byref(m), C.byref(nn), C.byref(kk)))
        return ms.value, n.value, nn.value, kk.value

    def get_embedding(self, slot: int = 0) -> torch.Tensor:
        out = torch.empty(1, self.cfg.out_chans, self.cfg.grid, self.cfg.grid, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_get_embedding(self.handle, slot, out.data_ptr(), _stream()))
        return out

    def set_embedding(self, emb: torch.Tensor, slot: int = 0) -> None:
        emb = emb.to(self.device, torch.float32).contiguous()
        assert emb.numel() == self.cfg.out_chans * self.cfg.grid ** 2
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_set_embedding(self.handle, slot, emb.data_ptr(), _stream()))

    def reset_image(self, slot: int = 0) -> None:
        self._check(self.lib.samrs_reset_image(self.handle, slot))

    def _prompt_arrays(self, boxes, point_coords, point_labels, mask_input):
        """The shape contract of one prompt batch -> (boxes, point_coords, point_labels, mask_input) as contiguous device
        tensors of the library's types, and their common batch size."""
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        if point_coords is not None and point_labels is None:
            raise AssertionError("point_labels must be supplied if point_coords is supplied.")
        # shape contract of predictor.py:169-177 / prompt_encoder.py:73-105 -- the library reads raw pointers, so a
        # mis-shaped prompt must be rejected here (the reference fails with a shape error inside the prompt encoder)
        n = None
        if point_coords is not None:
            if point_coords.dim() != 3 or point_coords.shape[-1] != 2:
                raise ValueError(f"point_coords must be BxNx2, got {tuple(point_coords.shape)}")
            n, npts = int(point_coords.shape[0]), int(point_coords.shape[1])
            if tuple(point_labels.shape) != (n, npts):
                raise ValueError(f"point_labels must be BxN = {(n, npts)}, got {tuple(point_labels.shape)}")
            if npts < 1 or npts > self.max_points:
                raise ValueError(f"{npts} points per prompt, but this engine was created with max_points={self.max_points} "
                                 "(hard limit 8: the decoder keeps at most 16 tokens per prompt); pass max_points= to "
                                 "sam_model_registry[...]")
            point_coords = point_coords.to(**f32).contiguous()
            point_labels = point_labels.to(dtype=torch.int32, device=dev).contiguous()
        if boxes is not None:
            if boxes.numel() % 4 != 0 or boxes.shape[-1] != 4:
                raise ValueError(f"boxes must be Bx4, got {tuple(boxes.shape)}")
            boxes = boxes.to(**f32).reshape(-1, 4).contiguous()
            if n is not None and boxes.shape[0] != n:
                raise ValueError(f"boxes has {boxes.shape[0]} rows but the point prompts have {n}")
            n = int(boxes.shape[0])
        if mask_input is not None:
            side = 4 * self.cfg.grid
            if mask_input.dim() != 4 or tuple(mask_input.shape[1:]) != (1, side, side):
                raise ValueError(f"mask_input must be Bx1x{side}x{side}, got {tuple(mask_input.shape)}")
            if n is not None and mask_input.shape[0] != n:
                raise ValueError(f"mask_input has batch {mask_input.shape[0]} but the other prompts have {n}")
            mask_input = mask_input.to(**f32).contiguous()
            n = int(mask_input.shape[0])
        if n is None:
            raise AssertionError("at least one prompt (points, boxes or mask_input) is required")
        return boxes, point_coords, point_labels, mask_input, n

    def predict(self, slot: int, boxes: Optional[torch.Tensor], point_coords: Optional[torch.Tensor],
                point_labels: Optional[torch.Tensor], mask_input: Optional[torch.Tensor], multimask_output: bool,
                return_logits: bool, input_size: Tuple[int, int], original_size: Tuple[int, int],
                want_masks: bool = True) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        boxes, point_coords, point_labels, mask_input, n = self._prompt_arrays(boxes, point_coords, point_labels, mask_input)
        if n < 1:
            raise ValueError("empty prompt batch")
        npts = 0 if point_coords is None else point_coords.shape[1]
        c = 3 if multimask_output else 1
        oh, ow = int(original_size[0]), int(original_size[1])
        masks = None
        if want_masks:
            masks = torch.empty(n, c, oh, ow, dtype=torch.float32 if return_logits else torch.uint8, device=dev)
        iou = torch.empty(n, c, **f32)
        low = torch.empty(n, c, 256, 256, **f32)
        with torch.cuda.device(dev):
            self._check(self.lib.samrs_predict(
                self.handle, slot, n, _ptr(boxes), _ptr(point_coords), _ptr(point_labels), npts, _ptr(mask_input),
                int(bool(multimask_output)), int(bool(return_logits)), int(input_size[0]), int(input_size[1]), oh, ow,
                _ptr(masks), iou.data_ptr(), low.data_ptr(), _stream()))
        if masks is not None and not return_logits:
            masks = masks.view(torch.bool)
        return masks, iou, low

    def predict_multi(self, slots: Sequence[int], counts: Sequence[int], boxes: Optional[torch.Tensor],
                      point_coords: Optional[torch.Tensor], point_labels: Optional[torch.Tensor], mask_input: Optional[torch.Tensor],
                      multimask_output: bool, return_logits: bool, input_sizes: Sequence[Tuple[int, int]],
                      original_sizes: Sequence[Tuple[int, int]], want_masks: bool = True):
        """The prompts of several images in one decoder chain (samrs_predict_multi).  Image i (embedding slot ``slots[i]``;
        slots may repeat) owns the next ``counts[i]`` rows of the prompt tensors, which have the layouts of :meth:`predict`
        and one prompt kind for all images.  Returns per-image lists (masks [n_i, C, H_i, W_i] bool -- fp32 logits with
        return_logits, None without want_masks --, iou [n_i, C], low-res logits [n_i, C, 256, 256]); entry i equals
        ``predict(slots[i], <image i's rows>, ...)`` byte for byte."""
        rows = _prompt_rows(boxes, point_coords, mask_input)
        slots, offsets, in_hw, orig_hw = multi_call_args(slots, counts, input_sizes, original_sizes, rows if rows is not None else 0)
        n_img, counts = len(slots), [offsets[i + 1] - offsets[i] for i in range(len(slots))]
        boxes, point_coords, point_labels, mask_input, n = self._prompt_arrays(boxes, point_coords, point_labels, mask_input)
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        npts = 0 if point_coords is None else point_coords.shape[1]
        c = 3 if multimask_output else 1
        masks = [None] * n_img
        if want_masks:
            masks = [torch.empty(counts[i], c, orig_hw[2 * i], orig_hw[2 * i + 1],
                                 dtype=torch.float32 if return_logits else torch.uint8, device=dev) for i in range(n_img)]
        iou = torch.empty(n, c, **f32)
        low = torch.empty(n, c, 256, 256, **f32)
        if n > 0:
            ia = C.c_int * n_img
            mptr = (C.c_void_p * n_img)(*[m.data_ptr() if m is not None and m.numel() else None for m in masks])
            with torch.cuda.device(dev):
                self._check(self.lib.samrs_predict_multi(
                    self.handle, n_img, ia(*slots), (C.c_int * (n_img + 1))(*offsets), _ptr(boxes), _ptr(point_coords),
                    _ptr(point_labels), npts, _ptr(mask_input), int(bool(multimask_output)), int(bool(return_logits)),
                    (C.c_int * (2 * n_img))(*in_hw), (C.c_int * (2 * n_img))(*orig_hw), mptr, iou.data_ptr(), low.data_ptr(),
                    _stream()))
        if want_masks and not return_logits:
            masks = [m.view(torch.bool) for m in masks]
        return masks, list(torch.split(iou, counts)), list(torch.split(low, counts))

    def rle_encode(self, masks: torch.Tensor, out: torch.Tensor, cursor: torch.Tensor, table: torch.Tensor) -> None:
        """COCO RLE strings of `masks` ([n, H, W] bool / uint8 on this device) appended to the byte buffer `out` (uint8, device)
        behind `cursor` (int64 [1], device, in / out); `table` (int64 [n, 3], device) receives (offset, length, n_counts)
        per mask.  Asynchronous on the current stream; see samrs_rle_encode in samrs_hip.h."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        m = m.reshape(-1, m.shape[-2], m.shape[-1]).contiguous()
        n, h, w = m.shape
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert cursor.dtype == torch.int64 and cursor.is_cuda and table.dtype == torch.int64 and table.is_cuda
        assert table.is_contiguous() and table.numel() >= 3 * n
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_rle_encode(self.handle, m.data_ptr(), n, h, w, out.data_ptr(), out.numel(),
                                                  cursor.data_ptr(), table.data_ptr(), _stream()))

    def rle_decode(self, strings: torch.Tensor, table: torch.Tensor, size: Sequence[int], out: Optional[torch.Tensor] = None,
                   areas_out: Optional[torch.Tensor] = None, status_out: Optional[torch.Tensor] = None):
        """The inverse of :meth:`rle_encode`: `strings` (uint8, device, contiguous; any alignment) and `table` (int64 [n, 3], device:
        (offset, length, ignored) per mask -- what ``rle_encode`` wrote) -> (masks uint8 [n, H, W] of 0 / 1 for `size` = (H, W), areas
        int64 [n], status int32 [n]; ``RLE_STATUS`` names the codes), all on the device.  A mask whose status is not 0 is all zero.
        `out` / `areas_out` / `status_out`: caller-owned contiguous tensors of those shapes and types (slices are fine) instead of
        new ones.  Asynchronous on the current stream; see samrs_rle_decode in samrs_hip.h."""
        h, w = int(size[0]), int(size[1])
        if not (isinstance(strings, torch.Tensor) and strings.dtype == torch.uint8 and strings.is_cuda and strings.is_contiguous() and strings.dim() == 1):
            raise ValueError("strings must be a contiguous uint8 [bytes] tensor on the engine's device")
        if not (isinstance(table, torch.Tensor) and table.dtype == torch.int64 and table.is_cuda and table.is_contiguous()
                and table.dim() == 2 and table.shape[1] == 3):
            raise ValueError("table must be a contiguous int64 [n, 3] tensor on the engine's device")
        n = int(table.shape[0])
        outs = []
        for name, t, shape, dt in (("out", out, (n, h, w), torch.uint8), ("areas_out", areas_out, (n,), torch.int64),
                                   ("status_out", status_out, (n,), torch.int32)):
            if t is None:
                t = torch.empty(shape, dtype=dt, device=self.device)
            elif not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on the engine's device, or None")
            outs.append(t)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_rle_decode(self.handle, _ptr(strings) if n else None, strings.numel(), _ptr(table) if n else None,
                                                  n, h, w, _ptr(outs[0]) if n else None, _ptr(outs[1]) if n else None,
                                                  _ptr(outs[2]) if n else None, _stream()))
        return outs[0], outs[1], outs[2]

    def png_encode(self, maps: torch.Tensor, lut: torch.Tensor, out: torch.Tensor, cursor: torch.Tensor, table: torch.Tensor) -> None:
        """``gray/<stem>.png`` and ``color/<stem>.png`` of the class maps `maps` ([n, H, W] or [H, W] uint8 on this device, 255 =
        unlabeled) through `lut` (uint8 [256, 3], device; ``tile_io.class_lut``), byte-identical with
        :func:`tile_io.write_label_pair`, appended to the byte buffer `out` (uint8, device, 16-byte aligned) behind `cursor` (int64
        [1], device, in / out); `table` (int64 [n, 2, 2], device) receives (offset, length) of the gray and the colour file per
        map, length < 0: did not fit (-length - 1 bytes needed).  Asynchronous on the current stream; see samrs_png_encode_labels
        in samrs_hip.h."""
        m = maps.reshape(-1, maps.shape[-2], maps.shape[-1]).contiguous()
        n, h, w = m.shape
        assert m.dtype == torch.uint8 and m.is_cuda
        assert lut.dtype == torch.uint8 and lut.is_cuda and lut.is_contiguous() and lut.numel() == 768
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert cursor.dtype == torch.int64 and cursor.is_cuda and table.dtype == torch.int64 and table.is_cuda
        assert table.is_contiguous() and table.numel() >= 4 * n
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_png_encode_labels(self.handle, m.data_ptr(), n, h, w, lut.data_ptr(), out.data_ptr(),
                                                         out.numel(), cursor.data_ptr(), table.data_ptr(), _stream()))

    def blend_labels(self, images: torch.Tensor, maps: torch.Tensor, lut: torch.Tensor, alpha: float = 0.4,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """visualize.py's overlay: ``Image.blend(image, lut[map], alpha)`` bit for bit, for `images` ([n, H, W, 3] or [H, W, 3] uint8 on
        this device) and their class maps `maps` ([n, H, W] or [H, W] uint8) through `lut` (uint8 [256, 3], device) -> uint8 of the
        images' shape (`out`, contiguous and not the images themselves, or a new tensor).  0 <= alpha <= 1.  Asynchronous on the
        current stream; see samrs_blend_labels in samrs_hip.h."""
        img = images.reshape(-1, *images.shape[-3:]).contiguous()
        m = maps.reshape(-1, *maps.shape[-2:]).contiguous()
        n, h, w, _ = img.shape
        assert img.dtype == torch.uint8 and img.is_cuda and img.shape[-1] == 3
        assert m.dtype == torch.uint8 and m.is_cuda and tuple(m.shape) == (n, h, w)
        assert lut.dtype == torch.uint8 and lut.is_cuda and lut.is_contiguous() and lut.numel() == 768
        res = out if out is not None else torch.empty_like(img)
        assert res.dtype == torch.uint8 and res.is_cuda and res.is_contiguous() and res.numel() == img.numel()
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_blend_labels(self.handle, img.data_ptr(), m.data_ptr(), lut.data_ptr(), float(alpha),
                                                    res.data_ptr(), n, h, w, _stream()))
        return res if out is not None else res.view(images.shape)

    def png_encode_rgb(self, rgb: torch.Tensor, out: torch.Tensor, cursor: torch.Tensor, table: torch.Tensor, filter: int = -1) -> None:
        """Truecolour PNG files of `rgb` ([n, H, W, 3] or [H, W, 3] uint8 on this device), appended to the byte buffer `out` (uint8,
        device, 16-byte aligned) behind `cursor` (int64 [1], device, in / out); `table` (int64 [n, 2], device) receives (offset,
        length) per image, length < 0: did not fit (-length - 1 bytes needed).  `filter`: 0 .. 4 = that PNG row filter on every row,
        -1 = per row the least sum of absolute filtered values.  ``png_rgb_bound(H, W)`` bytes per image always suffice for data
        whose codes stay under deflate's length limit.  Asynchronous on the current stream; see samrs_png_encode_rgb in samrs_hip.h."""
        x = rgb.reshape(-1, *rgb.shape[-3:]).contiguous()
        n, h, w, _ = x.shape
        assert x.dtype == torch.uint8 and x.is_cuda and x.shape[-1] == 3
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert cursor.dtype == torch.int64 and cursor.is_cuda and table.dtype == torch.int64 and table.is_cuda
        assert table.is_contiguous() and table.numel() >= 2 * n
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_png_encode_rgb(self.handle, x.data_ptr(), n, h, w, int(filter), out.data_ptr(), out.numel(),
                                                      cursor.data_ptr(), table.data_ptr(), _stream()))

    def select_best(self, masks: torch.Tensor, iou: torch.Tensor, best_out: Optional[torch.Tensor] = None,
                    quality_out: Optional[torch.Tensor] = None, areas_out: Optional[torch.Tensor] = None):
        """Best-of-C by predicted IoU on the device (samrs_select_best): masks [n, C, H, W] bool / uint8, iou [n, C] ->
        (best masks uint8 [n, H, W], quality fp32 [n], areas int64 [n]); the outputs may be caller-owned contiguous slices."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        n, c, h, w = m.shape
        assert m.is_contiguous() and iou.is_contiguous() and iou.dtype == torch.float32 and tuple(iou.shape) == (n, c)
        best = best_out if best_out is not None else torch.empty(n, h, w, dtype=torch.uint8, device=self.device)
        qual = quality_out if quality_out is not None else torch.empty(n, dtype=torch.float32, device=self.device)
        areas = areas_out if areas_out is not None else torch.empty(n, dtype=torch.int64, device=self.device)
        assert best.is_contiguous() and qual.is_contiguous() and areas.is_contiguous() and areas.dtype == torch.int64
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_select_best(self.handle, m.data_ptr(), iou.data_ptr(), n, c, h, w, best.data_ptr(),
                                                   qual.data_ptr(), areas.data_ptr(), _stream()))
        return best, qual, areas

    def clean_masks(self, masks: torch.Tensor, min_area: int, mode="both", areas_out=None, changed_out=None):
        """Small islands and holes removed on the device, in place (samrs_clean_masks; ``remove_small_regions`` of
        utils/amg.py:267-291): masks [n, H, W] bool / uint8, contiguous (a contiguous slice such as ``predict(...)[0][:, 0]`` of a
        C = 1 output is fine) -> (masks, areas int64 [n] = pixels set afterwards, changed int64 [n] = pixels whose value changed).
        A region is an 8-connected component and is small below `min_area` pixels; mode "holes" fills the small components of the
        complement, "islands" clears the small components (keeping the largest when all are small; ties: the one whose first
        pixel in row-major order comes first), "both" does holes, then islands.  `areas_out` / `changed_out`: None = a new
        tensor, a caller-owned contiguous int64 [n] slice, or False = not wanted (the library gets NULL and the tuple holds None
        there).  Asynchronous on the current stream."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        if m.dim() != 3 or m.dtype != torch.uint8:
            raise ValueError(f"masks must be bool / uint8 [n, H, W], got {masks.dtype} {tuple(masks.shape)}")
        if not (m.is_cuda and m.is_contiguous()):
            raise ValueError("masks must be a contiguous tensor on the engine's device (they are rewritten in place)")
        code = REGION_MODES.get(mode) if isinstance(mode, str) else int(mode)
        if code is None:
            raise ValueError(f"mode must be one of {sorted(REGION_MODES)}, got {mode!r}")
        n, h, w = m.shape
        outs = []
        for name, t in (("areas_out", areas_out), ("changed_out", changed_out)):
            if t is False:
                t = None
            elif t is None:
                t = torch.empty(n, dtype=torch.int64, device=self.device)
            elif not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and t.numel() == n):
                raise ValueError(f"{name} must be a contiguous int64 [{n}] tensor on the engine's device, None or False")
            outs.append(t)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_clean_masks(self.handle, m.data_ptr(), n, h, w, int(min_area), code, _ptr(outs[0]),
                                                   _ptr(outs[1]), _stream()))
        return masks, outs[0], outs[1]

    def region_labels(self, masks: torch.Tensor, complement: bool = False) -> torch.Tensor:
        """Test hook (samrs_k_region_labels): int32 [n, H, W], every pixel's flattened root = the smallest row-major pixel index of
        its 8-connected component of the set (complement: the unset) pixels, -1 outside that working set."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        assert m.dim() == 3 and m.dtype == torch.uint8 and m.is_cuda and m.is_contiguous()
        n, h, w = m.shape
        out = torch.empty(n, h, w, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_k_region_labels(m.data_ptr(), n, h, w, int(bool(complement)), out.data_ptr(), _stream()))
        return out

    def _masks_u8(self, masks: torch.Tensor) -> torch.Tensor:
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        if m.dim() != 3 or m.dtype != torch.uint8:
            raise ValueError(f"masks must be bool / uint8 [n, H, W], got {masks.dtype} {tuple(masks.shape)}")
        if not (m.is_cuda and m.is_contiguous()):
            raise ValueError("masks must be a contiguous tensor on the engine's device")
        return m

    def mask_boxes(self, masks: torch.Tensor, offset: Sequence[int] = (0, 0), hbox_out=None, rbox_out=None, record_out=None):
        """Where each mask actually is, derived on the device (samrs_mask_boxes): masks [n, H, W] bool / uint8, contiguous, decoded
        in a window whose origin is `offset` = (x0, y0) -> (hbox int32 [n, 4] = xmin, ymin, xmax, ymax inclusive; rbox fp32
        [n, 4, 2] = the corners of the minimum-area rotated rectangle of the set pixels' centres; record int64 [n, 8] = dx, dy, pmin,
        pmax, qmin, qmax, hull vertex count m, twice the hull's area).  The rectangle lies along a hull edge; of several
        equal-area ones the edge that comes first from the top-left set pixel, down the left side, wins.  An empty mask has m = 0
        and all outputs zero.  Each output: None = a new tensor, a caller-owned contiguous slice of that shape and type, or False =
        not wanted (the library gets NULL and the tuple holds None there).  Asynchronous on the current stream."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        outs = []
        for name, t, shape, dt in (("hbox_out", hbox_out, (n, 4), torch.int32), ("rbox_out", rbox_out, (n, 4, 2), torch.float32),
                                   ("record_out", record_out, (n, 8), torch.int64)):
            if t is False:
                t = None
            elif t is None:
                t = torch.empty(shape, dtype=dt, device=self.device)
            elif not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on the engine's device, None or False")
            outs.append(t)
        if n:
            with torch.cuda.device(self.device):
                self._check(self.lib.samrs_mask_boxes(self.handle, m.data_ptr(), n, h, w, int(offset[0]), int(offset[1]), _ptr(outs[0]),
                                                      _ptr(outs[1]), _ptr(outs[2]), _stream()))
        return outs[0], outs[1], outs[2]

    def mask_polygons(self, masks: torch.Tensor, offset: Sequence[int] = (0, 0), max_edges: int = 65536, vertices=None, rings=None,
                      cursor=None, table=None):
        """Each mask's outline as polygons, traced on the device (samrs_mask_polygons): masks [n, H, W] bool / uint8, contiguous,
        decoded in a window whose origin is `offset` = (x0, y0) -> (vertices int32 [V, 2], rings int32 [R, 4], cursor int64 [2],
        table int64 [n, 5]), all on the device.  Vertices are corners of the pixel LATTICE ((x, y) = the top-left corner of pixel
        (row y, col x)), not the pixel centres of ``mask_boxes``: a polygon encloses exactly its pixels' squares.  A ring record is
        (first vertex relative to the mask's first vertex, vertex count, twice the signed area: > 0 outer ring, < 0 hole, the pixel
        index y * W + x of the ring's smallest edge); table[j] = (first ring, ring count, first vertex, vertex count, edge count) with
        absolute firsts.  The masks are placed in order behind `cursor` (first free vertex, first free ring), which moves on: pass
        the same `vertices`, `rings` and `cursor` again to append.  A mask that does not fit either buffer takes no space and has
        firsts -1, ring count -1 - rings needed, vertex count -1 - vertices needed; a mask with more than `max_edges` edges is not
        traced (ring count = vertex count = -1; the edge count is always true).  ``samrs_amd.polygons.rings_of`` reads the result on
        the host.  Omitted buffers are allocated for the worst case (min(max_edges, 2 H W + 4) vertices and a quarter of that in rings
        per mask: 24 bytes per edge of the cap), a fresh cursor is (0, 0).  Asynchronous on the current stream."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        if int(max_edges) < 4:
            raise ValueError(f"max_edges must be at least 4, got {max_edges}")
        if vertices is None:
            vertices = torch.empty(max(1, n) * min(int(max_edges), 2 * h * w + 4), 2, dtype=torch.int32, device=self.device)
        if rings is None:
            rings = torch.empty(max(1, n) * (min(int(max_edges), 2 * h * w + 4) // 4), 4, dtype=torch.int32, device=self.device)
        if cursor is None:
            cursor = torch.zeros(2, dtype=torch.int64, device=self.device)
        if table is None:
            table = torch.empty(n, 5, dtype=torch.int64, device=self.device)
        for name, t, dt, last in (("vertices", vertices, torch.int32, 2), ("rings", rings, torch.int32, 4)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == last):
                raise ValueError(f"{name} must be a contiguous {dt} [k, {last}] tensor on the engine's device")
        if not (isinstance(cursor, torch.Tensor) and cursor.dtype == torch.int64 and cursor.is_cuda and cursor.is_contiguous() and cursor.numel() == 2):
            raise ValueError("cursor must be a contiguous int64 [2] tensor on the engine's device")
        if not (isinstance(table, torch.Tensor) and table.dtype == torch.int64 and table.is_cuda and table.is_contiguous()
                and tuple(table.shape) == (n, 5)):
            raise ValueError(f"table must be a contiguous int64 [{n}, 5] tensor on the engine's device")
        if n:
            with torch.cuda.device(self.device):
                self._check(self.lib.samrs_mask_polygons(self.handle, m.data_ptr(), n, h, w, int(offset[0]), int(offset[1]), int(max_edges),
                                                         vertices.data_ptr(), vertices.shape[0], rings.data_ptr(), rings.shape[0],
                                                         cursor.data_ptr(), table.data_ptr(), _stream()))
        return vertices, rings, cursor, table

    @staticmethod
    def polygon_eps_q(epsilon: float) -> int:
        """The tolerance of ``simplify_polygons`` in sixteenths of a pixel: round(16 * epsilon), which must lie in 1 .. 16384."""
        eps = float(epsilon)
        if not (eps == eps and 0.0 < eps < 1e9):
            raise ValueError(f"polygon epsilon must be a positive number of pixels, got {epsilon}")
        q = int(round(16.0 * eps))
        if not 1 <= q <= POLYGON_EPS_Q_MAX:
            raise ValueError(f"polygon epsilon {epsilon} is {q} sixteenths of a pixel: must lie in 1 .. {POLYGON_EPS_Q_MAX}")
        return q

    def _polygon_buffers(self, table, rings, vertices, cursor=None):
        for name, t, dt, last in (("vertices", vertices, torch.int32, 2), ("rings", rings, torch.int32, 4), ("table", table, torch.int64, 5)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == last):
                raise ValueError(f"{name} must be a contiguous {dt} [k, {last}] tensor on the engine's device")
        if cursor is not None and not (isinstance(cursor, torch.Tensor) and cursor.dtype == torch.int64 and cursor.is_cuda
                                       and cursor.is_contiguous() and cursor.numel() == 2):
            raise ValueError("cursor must be a contiguous int64 [2] tensor on the engine's device")

    def simplify_polygons(self, table: torch.Tensor, rings: torch.Tensor, vertices: torch.Tensor, cursor: torch.Tensor, epsilon: float):
        """The rings that ``mask_polygons`` traced, simplified IN PLACE on the device (samrs_simplify_polygons): Douglas-Peucker on
        every closed ring with distances to the chord segment, in integers, at the tolerance `epsilon` pixels (rounded to sixteenths
        of a pixel, 1/16 .. 1024; ``polygon_eps_q``).  `table` int64 [n, 5]: the rows of the ``mask_polygons`` calls that appended
        behind `cursor` into `vertices` / `rings`, in placement order (``torch.cat`` of their tables; rows that were not traced or
        placed pass through).  The vertices are compacted towards the first placed row's first vertex, ring records and rows get
        their new first vertex and vertex count, cursor[0] moves back to the new end; a ring record keeps the ORIGINAL ring's
        twice-signed area and its pixel index.  Every ring keeps at least 3 vertices, beginning with its first; topology is not
        preserved.  Returns (vertices, rings, cursor, table).  Asynchronous on the current stream."""
        q = self.polygon_eps_q(epsilon)
        self._polygon_buffers(table, rings, vertices, cursor)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_simplify_polygons(self.handle, vertices.data_ptr(), rings.data_ptr(), table.data_ptr(),
                                                         int(table.shape[0]), q, cursor.data_ptr(), _stream()))
        return vertices, rings, cursor, table

    def polygon_simplify_stages(self, table: torch.Tensor, rings: torch.Tensor, vertices: torch.Tensor, eps_q: int):
        """Test hook (samrs_k_polygon_simplify_keep): the listing and the rounds of ``simplify_polygons`` alone -> (keep uint8 [V] = 1
        at every kept vertex (absolute index), kept int32 [R] = kept vertices per ring (absolute ring index; -1: no ring of a placed
        row)).  Changes none of its inputs."""
        self._polygon_buffers(table, rings, vertices)
        n, V, R = int(table.shape[0]), int(vertices.shape[0]), int(rings.shape[0])
        nbytes = int(self.lib.samrs_k_polygon_simplify_scratch_bytes(n, V, R))
        if nbytes < 0:
            raise ValueError("polygon_simplify_stages needs at least one row")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        keep = torch.zeros(V, dtype=torch.uint8, device=self.device)
        kept = torch.zeros(R, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_k_polygon_simplify_keep(vertices.data_ptr(), rings.data_ptr(), table.data_ptr(), n, int(eps_q), V, R,
                                                               scratch.data_ptr(), keep.data_ptr(), kept.data_ptr(), _stream()))
        return keep, kept

    def fill_polygons(self, table: torch.Tensor, rings: torch.Tensor, vertices: torch.Tensor, size: Sequence[int],
                      offset: Sequence[int] = (0, 0), out=None, ref=None, counts_out=None):
        """The rings of the n rows of `table` back to masks, on the device (samrs_fill_polygons): the even-odd fill of each row's rings,
        sampled at the pixel centres of an (H, W) = `size` window whose origin is `offset` = (x0, y0); a centre exactly on an edge
        counts as right of it; integers only.  `table` int64 [n, 5], `rings` int32 [R, 4], `vertices` int32 [V, 2] as
        ``mask_polygons`` writes and ``simplify_polygons`` rewrites them, or as ``samrs_amd.polygons.pack_rings`` builds them from
        any integer polygons (uploaded).  -> (masks uint8 [n, H, W], counts int64 [n, 3] or None).  `out`: the masks' tensor, None to
        allocate one, False for no masks at all (only the counts are taken; nothing of size H W is written).  `ref` bool / uint8
        [n, H, W]: masks to count against; counts[j] = (set pixels of the fill, set pixels of ref[j], set in both), the last two 0
        without `ref`.  `counts_out`: their tensor, None to allocate one when there is something to report (`ref` given or out=False),
        False for none.  A row that is not a set of rings (not traced / not placed, a vertex farther than 2^20 from the origin, ring
        records that do not tile its vertices) fills as empty and has counts[j, 0] == -1.  Asynchronous on the current stream."""
        self._polygon_buffers(table, rings, vertices)
        n, (h, w) = int(table.shape[0]), (int(size[0]), int(size[1]))
        if out is None:
            out = torch.empty(n, h, w, dtype=torch.uint8, device=self.device)
        masks = None if out is False else self._masks_u8(out)
        if masks is not None and tuple(masks.shape) != (n, h, w):
            raise ValueError(f"out must be [{n}, {h}, {w}], got {tuple(masks.shape)}")
        g = None
        if ref is not None:
            g = self._masks_u8(ref)
            if tuple(g.shape) != (n, h, w):
                raise ValueError(f"ref must be [{n}, {h}, {w}], got {tuple(g.shape)}")
        if counts_out is None:
            counts_out = torch.empty(n, 3, dtype=torch.int64, device=self.device) if (g is not None or masks is None) else False
        counts = None if counts_out is False else counts_out
        if counts is not None and not (isinstance(counts, torch.Tensor) and counts.dtype == torch.int64 and counts.is_cuda
                                       and counts.is_contiguous() and tuple(counts.shape) == (n, 3)):
            raise ValueError(f"counts_out must be a contiguous int64 [{n}, 3] tensor on the engine's device")
        if n or (masks is None and counts is None):               # no rows: nothing to do; no output at all: the library says so
            with torch.cuda.device(self.device):
                self._check(self.lib.samrs_fill_polygons(self.handle, vertices.data_ptr(), rings.data_ptr(), table.data_ptr(), n, h, w,
                                                         int(offset[0]), int(offset[1]), None if masks is None else masks.data_ptr(),
                                                         None if g is None else g.data_ptr(),
                                                         None if counts is None else counts.data_ptr(), _stream()))
        return (None if masks is None else out), counts

    def score_masks(self, low: torch.Tensor, input_size: Sequence[int], original_size: Sequence[int], offset: float = 1.0,
                    boxes: Optional[torch.Tensor] = None, counts_out=None) -> torch.Tensor:
        """Threshold counts of every mask at the full output resolution, straight from the low-resolution logits
        (samrs_score_masks): low fp32 [n, 256, 256] or [n, C, 256, 256] (the third output of ``predict``; C is flattened into n),
        contiguous -> counts int64 [n, 4] = n_hi, n_mid, n_lo, n_in: the output pixels whose postprocessed logit is > +offset, > 0,
        > -offset, and > 0 inside the mask's box.  n_mid equals the number of set pixels of the mask ``predict`` returns for the
        same logits and sizes, exactly; stability = n_hi / n_lo (``quality.stability``), share inside the box = n_in / n_mid
        (``quality.inside_fraction``).  `boxes`: fp32 [n, 4] xyxy in the ORIGINAL frame (both corners inclusive), or None (n_in =
        0); for C = 3 repeat each box three times.  `counts_out`: None = a new tensor, or a caller-owned contiguous int64 [n, 4]
        slice.  Nothing of full resolution is written.  Asynchronous on the current stream."""
        if not (isinstance(low, torch.Tensor) and low.dtype == torch.float32 and low.dim() in (3, 4) and tuple(low.shape[-2:]) == (256, 256)):
            raise ValueError("low must be fp32 [n, 256, 256] or [n, C, 256, 256] (the low-resolution logits of predict)")
        if not (low.is_cuda and low.is_contiguous()):
            raise ValueError("low must be a contiguous tensor on the engine's device")
        n = int(low.numel() // (256 * 256))
        offset = float(offset)
        if not (offset >= 0.0 and offset != float("inf")):
            raise ValueError(f"offset must be finite and >= 0, got {offset}")
        if boxes is not None:
            if not (isinstance(boxes, torch.Tensor) and boxes.dtype == torch.float32 and boxes.is_cuda and boxes.is_contiguous()
                    and tuple(boxes.shape) == (n, 4)):
                raise ValueError(f"boxes must be a contiguous fp32 [{n}, 4] tensor on the engine's device, or None")
        if counts_out is None:
            counts_out = torch.empty(n, 4, dtype=torch.int64, device=self.device)
        elif not (isinstance(counts_out, torch.Tensor) and counts_out.dtype == torch.int64 and counts_out.is_cuda
                  and counts_out.is_contiguous() and tuple(counts_out.shape) == (n, 4)):
            raise ValueError(f"counts_out must be a contiguous int64 [{n}, 4] tensor on the engine's device, or None")
        if n:
            with torch.cuda.device(self.device):
                self._check(self.lib.samrs_score_masks(self.handle, low.data_ptr(), n, int(input_size[0]), int(input_size[1]),
                                                       int(original_size[0]), int(original_size[1]), offset, _ptr(boxes),
                                                       counts_out.data_ptr(), _stream()))
        return counts_out

    def filter_masks(self, masks: torch.Tensor, counts: torch.Tensor, iou: Optional[torch.Tensor] = None, min_stability: float = 0.0,
                     min_pred_iou: float = 0.0, min_inside_box: float = 0.0, keep_out=None) -> torch.Tensor:
        """The quality gate on the device (samrs_filter_masks): masks [n, H, W] bool / uint8, contiguous, in / out; counts int64
        [n, 4] from :meth:`score_masks`; iou fp32 [n] (the predicted IoU; needed when min_pred_iou > 0) -> keep uint8 [n].  A
        mask is kept iff every enabled criterion holds (a threshold <= 0 disables its criterion; ``quality.keep_rule`` restates
        the rule): stability n_hi / n_lo >= min_stability (an empty low-threshold mask fails), iou > min_pred_iou, share inside
        the box n_in / n_mid >= min_inside_box (an empty mask passes).  A dropped mask is zeroed in place -- to painting, areas,
        class statistics, ``mask_boxes`` and RLE it is an empty mask --, a kept one is not touched.  `keep_out`: None = a new
        tensor, or a caller-owned contiguous uint8 [n] slice.  Asynchronous on the current stream."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        if not (isinstance(counts, torch.Tensor) and counts.dtype == torch.int64 and counts.is_cuda and counts.is_contiguous()
                and tuple(counts.shape) == (n, 4)):
            raise ValueError(f"counts must be a contiguous int64 [{n}, 4] tensor on the engine's device")
        thr = [float(min_stability), float(min_pred_iou), float(min_inside_box)]
        if any(t != t for t in thr):
            raise ValueError("a threshold is NaN")
        if iou is None:
            if thr[1] > 0:
                raise ValueError("min_pred_iou > 0 needs iou")
        elif not (isinstance(iou, torch.Tensor) and iou.dtype == torch.float32 and iou.is_cuda and iou.is_contiguous() and iou.numel() == n):
            raise ValueError(f"iou must be a contiguous fp32 [{n}] tensor on the engine's device, or None")
        if keep_out is None:
            keep_out = torch.empty(n, dtype=torch.uint8, device=self.device)
        elif not (isinstance(keep_out, torch.Tensor) and keep_out.dtype == torch.uint8 and keep_out.is_cuda and keep_out.is_contiguous()
                  and tuple(keep_out.shape) == (n,)):
            raise ValueError(f"keep_out must be a contiguous uint8 [{n}] tensor on the engine's device, or None")
        if n:
            with torch.cuda.device(self.device):
                self._check(self.lib.samrs_filter_masks(self.handle, m.data_ptr(), n, h, w, counts.data_ptr(), _ptr(iou), thr[0], thr[1],
                                                        thr[2], keep_out.data_ptr(), _stream()))
        return keep_out

    def resolve_overlaps(self, masks: torch.Tensor, rule, low: Optional[torch.Tensor] = None, input_size: Optional[Sequence[int]] = None,
                         original_size: Optional[Sequence[int]] = None, priority: Optional[torch.Tensor] = None, owner_out=None,
                         before_out=None, removed_out=None):
        """One instance per pixel, on the device and in place (samrs_resolve_overlaps): masks [n, H, W] bool / uint8, contiguous, in /
        out -> (masks, owner int32 [H, W] = index of the mask that holds each pixel, -1 where none is set; before int64 [n] = set
        pixels on entry; removed int64 [n] = pixels cleared).  Walking the masks in order, mask j takes a pixel it is set at from
        its holder b iff there is no holder, or P[j] > P[b], or P[j] == P[b] and not v_j < v_b: ties go to the later mask, as
        painting does.  v is the postprocessed logit at the pixel, from `low` fp32 [n, 256, 256] or [n, 1, 256, 256] (the third
        output of ``predict``) for `input_size` -> the masks' size; without `low` the logit term is absent.  `rule`: "logit" (P = 0;
        needs `low`), "smallest" (P = -(the mask's set pixels on entry): the smaller instance wins; `low` breaks equal areas) or
        "priority" (P = `priority`, int64 [n] on the device; `low` breaks equal keys).  The gate is the mask byte, not v > 0: a pixel
        the clean-up filled competes with its negative logit.  Losers' bytes become 0, winners' bytes are not touched.
        `original_size`, when given, must be the masks' (H, W).  Each output: None = a new tensor, a caller-owned contiguous slice
        of that shape and type, or False = not wanted (the library gets NULL and the tuple holds None there).  Asynchronous on the
        current stream."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        code = OVERLAP_RULES.get(rule) if isinstance(rule, str) else int(rule)
        if code not in OVERLAP_RULES.values():
            raise ValueError(f"rule must be one of {sorted(OVERLAP_RULES)}, got {rule!r}")
        if original_size is not None and (int(original_size[0]), int(original_size[1])) != (h, w):
            raise ValueError(f"original_size {tuple(original_size)} is not the masks' size {(h, w)}")
        in_h = in_w = 0
        if low is not None:
            if not (isinstance(low, torch.Tensor) and low.dtype == torch.float32 and low.is_cuda and low.is_contiguous()
                    and tuple(low.shape) in ((n, 256, 256), (n, 1, 256, 256))):
                raise ValueError(f"low must be a contiguous fp32 [{n}, 256, 256] tensor on the engine's device (the low-resolution "
                                 f"logits of predict), or None")
            if input_size is None:
                raise ValueError("low needs input_size, the (h, w) of the input frame the logits were decoded for")
            in_h, in_w = int(input_size[0]), int(input_size[1])
        elif code == OVERLAP_RULES["logit"]:
            raise ValueError('rule "logit" needs low')
        if code == OVERLAP_RULES["priority"]:
            if not (isinstance(priority, torch.Tensor) and priority.dtype == torch.int64 and priority.is_cuda and priority.is_contiguous()
                    and priority.numel() == n):
                raise ValueError(f'rule "priority" needs priority, a contiguous int64 [{n}] tensor on the device')
        else:
            priority = None
        outs = []
        for name, t, shape, dt in (("owner_out", owner_out, (h, w), torch.int32), ("before_out", before_out, (n,), torch.int64),
                                   ("removed_out", removed_out, (n,), torch.int64)):
            if t is False:
                t = None
            elif t is None:
                t = torch.empty(shape, dtype=dt, device=self.device)
            elif not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on the engine's device, None or False")
            outs.append(t)
        if n:
            with torch.cuda.device(self.device):
                self._check(self.lib.samrs_resolve_overlaps(self.handle, m.data_ptr(), n, h, w, code, _ptr(low), in_h, in_w, _ptr(priority),
                                                            _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _stream()))
        elif outs[0] is not None:
            outs[0].fill_(-1)
        return masks, outs[0], outs[1], outs[2]

    def mask_row_extents(self, masks: torch.Tensor) -> torch.Tensor:
        """Test hook (samrs_k_mask_row_extents): int32 [n, H, 3] = first set column, last set column and pixel count of every row,
        (-1, -1, 0) for an empty row."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        out = torch.empty(n, h, 3, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_k_mask_row_extents(m.data_ptr(), n, h, w, out.data_ptr(), _stream()))
        return out

    def polygon_stages(self, masks: torch.Tensor, max_edges: int = 65536):
        """Test hook (samrs_k_polygon_edges, samrs_k_polygon_ranks): the stages of ``mask_polygons`` alone, for one chunk of masks ->
        (counts int32 [n] = edges per mask, ids uint32-as-int64 [n, stride], succ int32 [n, stride], corner uint8 [n, stride],
        leader int32 [n, stride], rank int32 [n, stride]) with stride = min(max_edges, 4 H W); only the first counts[j] entries of mask
        j mean anything, and none where counts[j] > max_edges."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        stride = int(self.lib.samrs_k_polygon_edge_stride(h, w, int(max_edges)))
        nbytes = int(self.lib.samrs_k_polygon_scratch_bytes(n, h, w, int(max_edges)))
        if stride < 0 or nbytes < 0:
            raise ValueError(f"{n} masks of {h} x {w} with max_edges {max_edges}: outside the limits of samrs_mask_polygons")
        dev = self.device
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ids = torch.zeros(n, stride, dtype=torch.int32, device=dev)
        succ, leader, rank = (torch.zeros(n, stride, dtype=torch.int32, device=dev) for _ in range(3))
        corner = torch.zeros(n, stride, dtype=torch.uint8, device=dev)
        counts, counts2 = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        with torch.cuda.device(dev):
            self._check(self.lib.samrs_k_polygon_edges(m.data_ptr(), n, h, w, int(max_edges), scratch.data_ptr(), ids.data_ptr(),
                                                       succ.data_ptr(), corner.data_ptr(), counts.data_ptr(), _stream()))
            self._check(self.lib.samrs_k_polygon_ranks(m.data_ptr(), n, h, w, int(max_edges), scratch.data_ptr(), leader.data_ptr(),
                                                       rank.data_ptr(), counts2.data_ptr(), _stream()))
        assert torch.equal(counts, counts2)
        return counts, ids.to(torch.int64) & 0xFFFFFFFF, succ, corner, leader, rank

    def mask_hull(self, masks: torch.Tensor, offset: Sequence[int] = (0, 0), cap: int = 2048):
        """Test hook (samrs_k_mask_hull): (vertices int32 [n, cap, 2], counts int32 [n]): the ordered strict hull vertices (x, y) of
        every mask in the frame of `offset`; rows past a mask's count are not written."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        ext = torch.empty(n, h, 3, dtype=torch.int32, device=self.device)
        verts = torch.zeros(n, cap, 2, dtype=torch.int32, device=self.device)
        counts = torch.zeros(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_k_mask_hull(m.data_ptr(), n, h, w, int(offset[0]), int(offset[1]), ext.data_ptr(),
                                                   verts.data_ptr(), int(cap), counts.data_ptr(), _stream()))
        return verts, counts

    def gt_match(self, masks: torch.Tensor, label_rgb: torch.Tensor, colors: torch.Tensor, inter_out: Optional[torch.Tensor] = None,
                 gt_area_out: Optional[torch.Tensor] = None, gt_masks_out: Optional[torch.Tensor] = None):
        """HRSC ground-truth matching on the device (samrs_gt_match): masks [n, H, W] bool / uint8, label_rgb uint8 [H, W, 3],
        colors uint8 [n, 3] -> (inter int64 [n], gt_area int64 [n], gt_masks uint8 [n, H, W] 0/1 or None).  Instance j's ground
        truth is the label pixels whose RGB equals colors[j]; pass `gt_masks_out` to receive it (e.g. for `rle_encode`).  The
        outputs may be caller-owned contiguous slices; asynchronous on the current stream."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        if m.dim() != 3:
            raise ValueError(f"masks must be [n, H, W], got {tuple(m.shape)}")
        n, h, w = m.shape
        if tuple(label_rgb.shape) != (h, w, 3) or label_rgb.dtype != torch.uint8:
            raise ValueError(f"label_rgb must be uint8 [{h}, {w}, 3] (the masks' size), got {label_rgb.dtype} {tuple(label_rgb.shape)}")
        if tuple(colors.shape) != (n, 3) or colors.dtype != torch.uint8:
            raise ValueError(f"colors must be uint8 [{n}, 3], got {colors.dtype} {tuple(colors.shape)}")
        for t in (m, label_rgb, colors):
            assert t.is_cuda and t.is_contiguous()
        inter = inter_out if inter_out is not None else torch.empty(n, dtype=torch.int64, device=self.device)
        gta = gt_area_out if gt_area_out is not None else torch.empty(n, dtype=torch.int64, device=self.device)
        for t in (inter, gta):
            assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and t.numel() == n
        if gt_masks_out is not None:
            assert gt_masks_out.dtype == torch.uint8 and gt_masks_out.is_cuda and gt_masks_out.is_contiguous()
            assert gt_masks_out.numel() == n * h * w
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_gt_match(self.handle, m.data_ptr(), n, h, w, label_rgb.data_ptr(), colors.data_ptr(),
                                                inter.data_ptr(), gta.data_ptr(), _ptr(gt_masks_out), _stream()))
        return inter, gta, gt_masks_out

    # -- COCO mask AP (samrs_amd/coco_ap.py): bit planes, pairwise counts, the greedy matching ---------------------------------
    def _out(self, name: str, t, shape, dtype) -> torch.Tensor:
        """A caller-owned contiguous output of that shape and type, or with None a new one."""
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_cuda and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"{name} must be a contiguous {dtype} {list(shape)} tensor on the engine's device, or None")
        return t

    def pack_mask_bits(self, masks: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Bit planes of masks [n, H, W] bool / uint8 (non-zero = set; contiguous, any alignment) on the device
        (samrs_mask_pack_bits) -> int64 [n, words], words = ceil(H W / 64): pixel p in row-major order is bit p % 64 of word p / 64
        (the int64 holds the uint64 bit pattern; ``numpy().view(np.uint64)``), the unused high bits of the last word are zero.
        `out`: a caller-owned contiguous int64 [n, words] slice.  Asynchronous on the current stream."""
        m = self._masks_u8(masks)
        n, h, w = m.shape
        out = self._out("out", out, (n, (h * w + 63) // 64), torch.int64)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_mask_pack_bits(self.handle, m.data_ptr(), n, h, w, out.data_ptr(), _stream()))
        return out

    def pack_label_bits(self, label_rgb: torch.Tensor, colors: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Bit planes of the instances of a label image (samrs_label_pack_bits): label_rgb uint8 [H, W, 3], colors uint8 [n, 3] ->
        int64 [n, words] in ``pack_mask_bits``' layout; instance j = the pixels whose RGB equals colors[j].  The image is read once
        per call and no mask bytes are written."""
        if label_rgb.dim() != 3 or label_rgb.shape[2] != 3 or label_rgb.dtype != torch.uint8:
            raise ValueError(f"label_rgb must be uint8 [H, W, 3], got {label_rgb.dtype} {tuple(label_rgb.shape)}")
        if colors.dim() != 2 or colors.shape[1] != 3 or colors.dtype != torch.uint8:
            raise ValueError(f"colors must be uint8 [n, 3], got {colors.dtype} {tuple(colors.shape)}")
        for t in (label_rgb, colors):
            if not (t.is_cuda and t.is_contiguous()):
                raise ValueError("label_rgb and colors must be contiguous tensors on the engine's device")
        h, w, n = int(label_rgb.shape[0]), int(label_rgb.shape[1]), int(colors.shape[0])
        out = self._out("out", out, (n, (h * w + 63) // 64), torch.int64)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_label_pack_bits(self.handle, label_rgb.data_ptr(), colors.data_ptr(), n, h, w, out.data_ptr(),
                                                       _stream()))
        return out

    def mask_pair_counts(self, a: torch.Tensor, b: torch.Tensor, inter_out=None, area_a_out=None, area_b_out=None):
        """Every plane of `a` against every plane of `b` (samrs_mask_pair_counts): a int64 [na, words], b int64 [nb, words] (bit
        planes of masks of one size) -> (inter int64 [na, nb] = |a_i AND b_j|, area_a int64 [na], area_b int64 [nb]).  Exact integer
        counts.  Each output: None = a new tensor, or a caller-owned contiguous tensor of that shape."""
        for name, t in (("a", a), ("b", b)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == 2 and t.is_cuda and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int64 [n, words] tensor on the engine's device (pack_mask_bits)")
        if a.shape[1] != b.shape[1]:
            raise ValueError(f"a and b hold planes of different sizes: {a.shape[1]} and {b.shape[1]} words")
        na, nb, words = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
        inter = self._out("inter_out", inter_out, (na, nb), torch.int64)
        area_a = self._out("area_a_out", area_a_out, (na,), torch.int64)
        area_b = self._out("area_b_out", area_b_out, (nb,), torch.int64)
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_mask_pair_counts(self.handle, a.data_ptr(), na, b.data_ptr(), nb, words, inter.data_ptr(),
                                                        area_a.data_ptr(), area_b.data_ptr(), _stream()))
        return inter, area_a, area_b

    def mask_boundary_bits(self, planes: torch.Tensor, h: int, w: int, d: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The boundary bands of bit planes (samrs_mask_boundary_bits; the definition is stated there): planes int64 [n, words] of
        h x w masks, from ``pack_mask_bits`` or ``pack_label_bits`` alike -> int64 [n, words], band = M AND NOT (M eroded by the
        (2 d + 1)^2 square, everything outside the image background), tail bits zero.  d: ``coco_ap.boundary_dilation(h, w)``, 1..128.
        `out`: a caller-owned contiguous int64 [n, words] slice that does not overlap `planes`.  Asynchronous on the current stream;
        the call keeps one grown scratch per engine, so such calls must be stream-ordered with each other."""
        h, w, d = int(h), int(w), int(d)
        words = (h * w + 63) // 64 if h > 0 and w > 0 else -1
        if not (isinstance(planes, torch.Tensor) and planes.dtype == torch.int64 and planes.dim() == 2 and planes.is_cuda
                and planes.is_contiguous()) or (words > 0 and planes.shape[1] != words):
            raise ValueError(f"planes must be a contiguous int64 [n, {words}] tensor on the engine's device (pack_mask_bits of {h} x {w} masks)")
        n = int(planes.shape[0])
        out = self._out("out", out, (n, int(planes.shape[1])), torch.int64)
        if n:                                                  # an empty stack has no storage to point at
            with torch.cuda.device(self.device):
                self._check(self.lib.samrs_mask_boundary_bits(self.handle, planes.data_ptr(), n, h, w, d, out.data_ptr(), _stream()))
        return out

    def coco_match(self, inter: torch.Tensor, area_d: torch.Tensor, area_g: torch.Tensor, scores, thresholds=None, area_ranges=None,
                   max_det: int = 100, order_out=None, match_out=None, dt_ignore_out=None, n_valid_out=None, n_kept_out=None,
                   boundary=None):
        """COCOeval.evaluateImg's greedy matching of one image on the device (samrs_coco_match; the rule is stated there and in
        samrs_amd/coco_ap.py): inter int64 [nd, ng], area_d int64 [nd], area_g int64 [ng] (``mask_pair_counts``), scores fp32 [nd]
        on the device, or on the host (a CPU tensor / array: checked for NaN, then uploaded by the library) ->
        (order int32 [max_det], match int32 [A, T, max_det] = ground-truth INDEX or -1, dt_ignore uint8 [A, T, max_det],
        n_valid int32 [A], n_kept int32 [1]) for the T `thresholds` (default: COCO's ten) and A `area_ranges` (default: COCO's
        four).  Ranks past n_kept hold -1 / -1 / 0.  A NaN among device scores yields n_kept = -1.  Asynchronous on the current
        stream; the outputs may be caller-owned contiguous tensors.
        `boundary` = (inter_b, area_db, area_gb), the same counts of the masks' boundary bands (``mask_boundary_bits`` +
        ``mask_pair_counts``): Boundary AP's matching (samrs_coco_match_min), the pair IoU is min(mask IoU, boundary IoU) while
        area ranges and ignore flags stay the masks'.  None (default) makes the plain call."""
        from . import coco_ap
        thr = np.ascontiguousarray(coco_ap.IOU_THRESHOLDS if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        rng = np.ascontiguousarray(coco_ap.AREA_RANGES if area_ranges is None else area_ranges, dtype=np.float64).reshape(-1, 2)
        T, A, max_det = len(thr), len(rng), int(max_det)
        nd, ng = int(area_d.numel()), int(area_g.numel())
        for name, t, shape in (("inter", inter, (nd, ng)), ("area_d", area_d, (nd,)), ("area_g", area_g, (ng,))):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous int64 {list(shape)} tensor on the engine's device")
        if boundary is not None:
            if len(boundary) != 3:
                raise ValueError("boundary must be (inter_b, area_db, area_gb)")
            for name, t, shape in zip(("inter_b", "area_db", "area_gb"), boundary, ((nd, ng), (nd,), (ng,))):
                if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"boundary: {name} must be a contiguous int64 {list(shape)} tensor on the engine's device")
        on_host = not (isinstance(scores, torch.Tensor) and scores.is_cuda)
        if on_host:
            scores = torch.as_tensor(np.ascontiguousarray(np.asarray(scores, dtype=np.float32).reshape(-1)))
        if not (scores.dtype == torch.float32 and scores.is_contiguous() and scores.numel() == nd):
            raise ValueError(f"scores must be a contiguous fp32 [{nd}] tensor or array")
        order = self._out("order_out", order_out, (max_det,), torch.int32)
        match = self._out("match_out", match_out, (A, T, max_det), torch.int32)
        ign = self._out("dt_ignore_out", dt_ignore_out, (A, T, max_det), torch.uint8)
        n_valid = self._out("n_valid_out", n_valid_out, (A,), torch.int32)
        n_kept = self._out("n_kept_out", n_kept_out, (1,), torch.int32)
        dp = C.POINTER(C.c_double)
        counts = [_ptr(inter) if nd and ng else None, _ptr(area_d) if nd else None, _ptr(area_g) if ng else None]
        fn = self.lib.samrs_coco_match
        if boundary is not None:
            counts += [_ptr(boundary[0]) if nd and ng else None, _ptr(boundary[1]) if nd else None, _ptr(boundary[2]) if ng else None]
            fn = self.lib.samrs_coco_match_min
        with torch.cuda.device(self.device):
            self._check(fn(self.handle, *counts, scores.data_ptr() if nd else None, int(on_host), nd, ng,
                           thr.ctypes.data_as(dp), T, rng.ctypes.data_as(dp), A, max_det, order.data_ptr(),
                           match.data_ptr(), ign.data_ptr(), n_valid.data_ptr(), n_kept.data_ptr(), _stream()))
            if on_host and nd:
                torch.cuda.current_stream().synchronize()      # the library reads the host scores on the stream
        return order, match, ign, n_valid, n_kept

    def paint(self, masks: torch.Tensor, labels: torch.Tensor, seg: torch.Tensor,
              class_pixels: Optional[torch.Tensor] = None, class_instances: Optional[torch.Tensor] = None,
              areas_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Ordered painting + areas (+ class statistics) on device; see samrs_paint in samrs_hip.h.  `areas_out`: a caller-owned
        contiguous int64 [n] slice to receive the areas (the pipeline's [batch, max_boxes] table) instead of a new tensor."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        m = m.reshape(-1, m.shape[-2], m.shape[-1]).contiguous()
        n, h, w = m.shape
        labels = labels.to(dtype=torch.int32, device=self.device).contiguous()
        if areas_out is not None:
            assert areas_out.dtype == torch.int64 and areas_out.is_contiguous() and areas_out.numel() == n and areas_out.is_cuda
        areas = areas_out if areas_out is not None else torch.empty(n, dtype=torch.int64, device=self.device)
        ncls = 0 if class_pixels is None else class_pixels.numel()
        with torch.cuda.device(self.device):
            self._check(self.lib.samrs_paint(self.handle, m.data_ptr(), labels.data_ptr(), n, h, w, seg.data_ptr(),
                                             areas.data_ptr(), _ptr(class_pixels), _ptr(class_instances), ncls, _stream()))
        return areas

    # -- scene mode (samrs_amd/scene.py): windows of one large scene composited in the scene's frame ------------------------
    def _check_scene(self, rc: int) -> None:
        """A window that is not inside its scene is a caller's planning error, not a malformed prompt: EngineError."""
        if rc == ERR_BAD_ARG:
            raise EngineError(self.lib.samrs_last_error(self.handle).decode())
        self._check(rc)

    def scene_claim(self, masks: torch.Tensor, ranks: torch.Tensor, window: Sequence[int], order: torch.Tensor,
                    labels: Optional[torch.Tensor] = None, class_pixels: Optional[torch.Tensor] = None,
                    class_instances: Optional[torch.Tensor] = None, areas_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The masks of one predict call ([n, h, w] bool / uint8), all decoded in `window` = (x0, y0, w, h) of the scene whose rank
        map is `order` (int32 [H, W] on this device, initialised to -1): order[p] = max(order[p], ranks[j]) wherever mask j is set
        (`ranks` int32 [n]: the masks' positions in the scene's annotation order).  Areas and class statistics as `paint`; see
        samrs_scene_claim in samrs_hip.h.  Asynchronous on the current stream."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        m = (m if m.dim() == 3 else m.reshape(-1, m.shape[-2], m.shape[-1])).contiguous()
        n, h, w = m.shape
        x0, y0, ww, wh = (int(v) for v in window)
        if (ww, wh) != (w, h):
            raise ValueError(f"window {tuple(window)} does not have the masks' size {w} x {h}")
        assert order.dtype == torch.int32 and order.dim() == 2 and order.is_cuda and order.is_contiguous()
        H, W = int(order.shape[0]), int(order.shape[1])
        ranks = ranks.to(dtype=torch.int32, device=self.device).contiguous()
        assert ranks.numel() == n
        if labels is not None:
            labels = labels.to(dtype=torch.int32, device=self.device).contiguous()
            assert labels.numel() == n
        if areas_out is not None:
            assert areas_out.dtype == torch.int64 and areas_out.is_contiguous() and areas_out.numel() == n and areas_out.is_cuda
        areas = areas_out if areas_out is not None else torch.empty(n, dtype=torch.int64, device=self.device)
        ncls = 0 if class_pixels is None else class_pixels.numel()
        with torch.cuda.device(self.device):
            self._check_scene(self.lib.samrs_scene_claim(self.handle, m.data_ptr(), ranks.data_ptr(), _ptr(labels), n, h, w, x0, y0, H, W,
                                                         order.data_ptr(), areas.data_ptr(), _ptr(class_pixels), _ptr(class_instances),
                                                         ncls, _stream()))
        return areas

    def scene_resolve(self, order: torch.Tensor, labels_by_rank: torch.Tensor, seg: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The scene's class map from its rank map: seg[p] = 255 where order[p] < 0, else the label of annotation order[p]
        (samrs_scene_resolve); `seg`: a caller-owned contiguous uint8 [H, W], or None for a new tensor."""
        assert order.dtype == torch.int32 and order.dim() == 2 and order.is_cuda and order.is_contiguous()
        H, W = int(order.shape[0]), int(order.shape[1])
        lab = labels_by_rank.to(dtype=torch.int32, device=self.device).contiguous()
        if seg is None:
            seg = torch.empty(H, W, dtype=torch.uint8, device=self.device)
        assert seg.dtype == torch.uint8 and seg.is_cuda and seg.is_contiguous() and tuple(seg.shape) == (H, W)
        with torch.cuda.device(self.device):
            self._check_scene(self.lib.samrs_scene_resolve(self.handle, order.data_ptr(), lab.data_ptr() if lab.numel() else None,
                                                           lab.numel(), H, W, seg.data_ptr(), _stream()))
        return seg

    def rle_encode_placed(self, masks: torch.Tensor, window: Sequence[int], size: Sequence[int], out: torch.Tensor,
                          cursor: torch.Tensor, table: torch.Tensor) -> None:
        """`rle_encode` of each mask ([n, h, w] bool / uint8) as if pasted at `window` = (x0, y0, w, h) on an all-zero canvas of
        `size` = (H, W): the strings of ``{"size": [H, W]}``, without the canvas ever existing (samrs_rle_encode_placed)."""
        m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        m = (m if m.dim() == 3 else m.reshape(-1, m.shape[-2], m.shape[-1])).contiguous()
        n, h, w = m.shape
        x0, y0, ww, wh = (int(v) for v in window)
        if (ww, wh) != (w, h):
            raise ValueError(f"window {tuple(window)} does not have the masks' size {w} x {h}")
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert cursor.dtype == torch.int64 and cursor.is_cuda and table.dtype == torch.int64 and table.is_cuda
        assert table.is_contiguous() and table.numel() >= 3 * n
        with torch.cuda.device(self.device):
            self._check_scene(self.lib.samrs_rle_encode_placed(self.handle, m.data_ptr(), n, h, w, x0, y0, int(size[0]), int(size[1]),
                                                               out.data_ptr(), out.numel(), cursor.data_ptr(), table.data_ptr(),
                                                               _stream()))
