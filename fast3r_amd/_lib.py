"""ctypes binding of libf3r_hip.so (the C ABI declared in include/f3r.h).

This is the drop-in boundary: the Python host hands raw device pointers (torch tensors are only the
allocator) to hand-written HIP kernels.  There is NO fallback: if the shared library is missing or a
kernel reports an error, the call raises -- the product path never silently computes with torch ops.
"""
import ctypes
import os

import torch

F3R_F16, F3R_BF16 = 0, 1
F3R_A_PLAIN, F3R_A_CONV3X3 = 0, 1
F3R_EPI_GENERIC, F3R_EPI_QKV, F3R_EPI_CONVT = 0, 1, 2
F3R_ACT_NONE, F3R_ACT_GELU, F3R_ACT_RELU = 0, 1, 2
F3R_SPLIT_NONE, F3R_SPLIT_W2, F3R_SPLIT_X3, F3R_SPLIT_W2F8, F3R_SPLIT_X3F8 = 0, 1, 2, 3, 4
F3R_MAX_SEG = 8
F3R_REAL_F32, F3R_REAL_F64 = 0, 1
F3R_LOSS_DIS, F3R_LOSS_LOG1P = 0, 1
SCENE_TILE = 4096  # F3R_SCENE_TILE: keys per tile of the segmented sort; COLLECT_TILE: entries per tile of collect_points
COLLECT_TILE = 1024
F3R_SKY_CLASSIFY, F3R_SKY_MORPH, F3R_SKY_LABEL = 1, 2, 4
F3R_SKY_EMPTY, F3R_SKY_NO_TOP, F3R_SKY_TOP = 0, 1, 2
SKY_PIX_TILE, SKY_WORD_TILE = 16, 256  # F3R_SKY_PIX_TILE, F3R_SKY_WORD_TILE: words per workgroup of the two kinds of sky kernel
MESH_TILE = 1024  # F3R_MESH_TILE: pixels, or quads, per workgroup of the mesh kernels
F3R_INDEX_I32, F3R_INDEX_I64 = 0, 1
# F3R_CLOUD_TILE: pixels per workgroup of the combine kernels; F3R_CLOUD_SORT_TILE: keys per workgroup of the voxel sort; F3R_CLOUD_FPS_TILE:
# points per tile of the tiled farthest-point path; F3R_CLOUD_FPS_ONE_MAX: the most points its one-workgroup path takes
CLOUD_TILE, CLOUD_SORT_TILE, CLOUD_FPS_TILE, CLOUD_FPS_ONE_MAX = 1024, 2048, 1024, 8192
RENDER_CENTER_PARTS = 1024  # F3R_RENDER_CENTER_PARTS: rows of the scratch f3r_render_center takes
RASTER_SMALL_PIXELS = 64  # F3R_RASTER_SMALL_PIXELS: the largest pixel box a stage-1 thread of the rasteriser draws itself
F3R_FPS_AUTO, F3R_FPS_ONE, F3R_FPS_TILED = 0, 1, 2
MAPS_TILE = 1024  # F3R_MAPS_TILE: pixels per workgroup of the map-picture kernels
F3R_MAPS_LUT, F3R_MAPS_RGB = 0, 1
GTVIEW_CAM_WORDS = 25  # F3R_GTVIEW_CAM_WORDS: floats of a row of the ground-truth views' camera table (the 3 x 3 intrinsics, then the 4 x 4 pose)
F3R_GTVIEW_POSE, F3R_GTVIEW_FINITE_MASK = 1, 2
# F3R_DEPTH_TILE: pixels per workgroup of the depth metrics' error and compaction kernels; F3R_DEPTH_ROW_WORDS: words of a row of their table;
# F3R_DEPTH_OUT_WORDS: fixed words of a result row (the curves follow); F3R_DEPTH_MAX_THRESHOLDS: inlier thresholds of one call
DEPTH_TILE, DEPTH_ROW_WORDS, DEPTH_OUT_WORDS, DEPTH_MAX_THRESHOLDS = 1024, 8, 16, 4
F3R_DEPTH_ALIGN_NONE, F3R_DEPTH_ALIGN_MEDIAN = 0, 1
MATCH_TILE = 2048  # F3R_MATCH_TILE: candidates of a pair's second view per workgroup of the reciprocity kernels
F3R_CLEAN_WORLD, F3R_CLEAN_CAMERA = 0, 1  # f3r_clean_frame: the frame of the points handed to f3r_clean_confidence
F3R_GALIGN_L1, F3R_GALIGN_L2 = 0, 1  # f3r_galign_dist: the distance of f3r_galign_loss_grad

_c_i64, _c_i32, _c_f32, _c_vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p


class GemmArgs(ctypes.Structure):
    """struct f3r_gemm_args (include/f3r.h) -- field order and types must match exactly."""
    _fields_ = [
        ("A", _c_vp), ("W", _c_vp), ("bias", _c_vp),
        ("M", _c_i64), ("N", _c_i32), ("K", _c_i32), ("Kpad", _c_i32), ("lda", _c_i64),
        ("a_mode", _c_i32), ("a_relu", _c_i32),
        ("conv_H", _c_i32), ("conv_W", _c_i32), ("conv_C", _c_i32), ("conv_stride", _c_i32),
        ("conv_OH", _c_i32), ("conv_OW", _c_i32),
        ("epi", _c_i32), ("act", _c_i32),
        ("rowadd", _c_vp), ("rowadd_div", _c_i64),
        ("res_f32", _c_vp), ("ldr_f32", _c_i64),
        ("res_lp", _c_vp), ("ldr_lp", _c_i64),
        ("res_lp2", _c_vp), ("ldr_lp2", _c_i64),
        ("out_f32", _c_vp), ("ldo_f32", _c_i64),
        ("out_lp", _c_vp), ("ldo_lp", _c_i64),
        ("q", _c_vp), ("k", _c_vp), ("vt", _c_vp), ("seq_len", _c_i64), ("ldvt", _c_i64),
        ("rope_cos", _c_vp), ("rope_sin", _c_vp), ("rope_w", _c_i32), ("q_scale", _c_f32),
        ("ct_s", _c_i32), ("ct_h", _c_i32), ("ct_w", _c_i32), ("ct_cout", _c_i32),
        ("dtype", _c_i32), ("rope_mode", _c_i32),
        ("split", _c_i32), ("kernel_sel", _c_i32), ("A_lo", _c_vp),
        ("out_lp_lo", _c_vp), ("res_lp_lo", _c_vp), ("res_lp2_lo", _c_vp), ("out_relu", _c_vp), ("out_relu_lo", _c_vp),
        ("qkv_dq", _c_i32), ("out_lp_f8", _c_i32),
        ("w_scale", _c_vp), ("W_aux", _c_vp),
        ("out_f8", _c_vp), ("out_relu_f8", _c_vp),
        ("fin_w", _c_vp), ("fin_b", _c_vp), ("fin_pts", _c_vp), ("fin_conf", _c_vp),
        ("fin_n_out", _c_i32), ("fin_depth_mode", _c_i32), ("fin_conf_mode", _c_i32), ("fin_vmin", _c_f32), ("fin_vmax", _c_f32), ("reserved0", _c_i32),
    ]


class AttnArgs(ctypes.Structure):
    """struct f3r_attn_args (include/f3r.h)."""
    _fields_ = [
        ("q", _c_vp), ("o", _c_vp),
        ("ldq", _c_i64), ("ldo", _c_i64),
        ("q_batch_stride", _c_i64), ("o_batch_stride", _c_i64),
        ("tq", _c_i64),
        ("batch", _c_i32), ("n_heads", _c_i32), ("n_seg", _c_i32), ("dtype", _c_i32),
        ("k_seg", _c_vp * F3R_MAX_SEG), ("vt_seg", _c_vp * F3R_MAX_SEG),
        ("seg_len", _c_i64 * F3R_MAX_SEG), ("ldvt", _c_i64 * F3R_MAX_SEG),
        ("ldk", _c_i64),
        ("k_batch_stride", _c_i64 * F3R_MAX_SEG), ("vt_batch_stride", _c_i64 * F3R_MAX_SEG),
        ("scale", _c_f32), ("q_prescaled", _c_i32),
        ("st_o", _c_vp), ("st_ml", _c_vp), ("state_in", _c_i32), ("state_out", _c_i32),
        ("kv_group", _c_i32), ("causal", _c_i32), ("q_pos0", _c_i64), ("seg_pos0", _c_i64 * F3R_MAX_SEG),
        ("kernel_sel", _c_i32), ("head_dim", _c_i32),
        ("dbg_counters", _c_vp),
        ("sched_counter", _c_vp),
        ("qk_planes", _c_i32), ("reserve_cus", _c_i32),
    ]


class AttnF32Args(ctypes.Structure):
    """struct f3r_attn_f32_args (include/f3r.h)."""
    _fields_ = [
        ("q", _c_vp), ("k", _c_vp), ("v", _c_vp), ("ldq", _c_i64), ("ldkv", _c_i64),
        ("o_hi", _c_vp), ("o_lo", _c_vp), ("o_f32", _c_vp), ("ldo", _c_i64),
        ("n_seq", _c_i64), ("tq", _c_i64), ("tk", _c_i64), ("q_pos0", _c_i64), ("k_pos0", _c_i64),
        ("n_heads", _c_i32), ("kv_group", _c_i32), ("causal", _c_i32), ("dtype", _c_i32), ("head_dim", _c_i32), ("scale", _c_f32),
    ]


# every symbol include/f3r.h declares: (name, restype, argtypes)
SYMBOLS = {
    "f3r_version": (ctypes.c_int, []),
    "f3r_last_error_string": (ctypes.c_char_p, []),
    "f3r_sizeof": (ctypes.c_size_t, [ctypes.c_int]),
    "f3r_wall_clock_khz": (ctypes.c_int, []),
    "f3r_patchify": (ctypes.c_int, [_c_vp, _c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_interp_bilinear": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp] + [ctypes.c_int] * 9 + [_c_vp]),
    "f3r_interp_bilinear_f8": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp] + [ctypes.c_int] * 9 + [_c_vp]),
    "f3r_layernorm": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, ctypes.c_int, _c_f32, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_layernorm_f8": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_f32, ctypes.c_int, _c_vp]),
    "f3r_gemm": (ctypes.c_int, [ctypes.POINTER(GemmArgs), _c_vp]),
    "f3r_attn_fwd": (ctypes.c_int, [ctypes.POINTER(AttnArgs), _c_vp]),
    "f3r_attn_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(AttnArgs)]),
    "f3r_block_workspace_bytes": (ctypes.c_size_t, [_c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i64, _c_i64, ctypes.POINTER(ctypes.c_size_t)]),
    "f3r_block_workspace_bytes_ex": (ctypes.c_size_t, [_c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i64, _c_i64, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "f3r_upsample2x": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_dpt_final": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_vp, _c_vp, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     _c_f32, _c_f32, ctypes.c_int, _c_vp]),
    "f3r_cast_f32_to_lp": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, ctypes.c_int, _c_vp]),
    "f3r_align_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "f3r_align_local_to_global": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_size_t,
                                                 ctypes.c_int, _c_i64, _c_f32, _c_vp]),
    "f3r_focal_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "f3r_estimate_focal": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          _c_f32, _c_f32, _c_f32, ctypes.c_int, _c_f32, _c_f32, _c_vp]),
    "f3r_nn_index_bytes": (ctypes.c_size_t, [_c_i64]),
    "f3r_nn_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "f3r_nn_build": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, ctypes.c_size_t, _c_vp, ctypes.c_size_t, _c_vp]),
    "f3r_nn_query": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "f3r_estimate_normals": (ctypes.c_int, [_c_vp, _c_vp, ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_recon_stats_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "f3r_recon_stats": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_double, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "f3r_recon_prepare_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, _c_i64]),
    "f3r_recon_prepare": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, ctypes.c_int, _c_i64, _c_f32, _c_f32, _c_vp, _c_vp,
                                         _c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "f3r_resample_u8": (ctypes.c_int, [_c_vp, _c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_vp, _c_vp, ctypes.c_int, _c_vp]),
    "f3r_imgnorm_u8": (ctypes.c_int, [_c_vp, _c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_silu_mul": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_rows_add_f32": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, ctypes.c_int, _c_vp]),
    "f3r_rope2d_f32": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, ctypes.c_int, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_vp]),
    "f3r_attn_f32": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_f32, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_rope_f32": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, ctypes.c_int, _c_i64, ctypes.c_int, ctypes.c_int, _c_vp, _c_vp, _c_vp]),
    "f3r_silu_mul_f32": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_attn_f32_ex": (ctypes.c_int, [ctypes.POINTER(AttnF32Args), _c_vp]),
    "f3r_attn_f32_mfma_workspace": (ctypes.c_int64, [ctypes.POINTER(AttnF32Args)]),
    "f3r_attn_f32_mfma": (ctypes.c_int, [ctypes.POINTER(AttnF32Args), _c_vp, ctypes.c_int64, _c_vp]),
    "f3r_qkv_planes": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int, _c_f32, _c_vp, _c_vp, _c_vp, _c_i64, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_attn_state_finish": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, ctypes.c_int, ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_i64, ctypes.c_int, _c_vp]),
    "f3r_estimate_poses": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_f32, _c_f32,
                                          _c_f32, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_pose_pair_metrics": (ctypes.c_int, [_c_vp, _c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_pose_error_stats": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_vp, _c_vp]),
    "f3r_mv_conf_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "f3r_mv_conf_loss": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _c_vp, ctypes.c_size_t,
                                        _c_vp, _c_vp]),
    "f3r_scene_sort_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "f3r_scene_sort": (ctypes.c_int, [_c_vp, ctypes.c_int, _c_i64, _c_i64, _c_vp, _c_vp, ctypes.c_size_t, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                      _c_vp, _c_vp]),
    "f3r_scene_extent_workspace_bytes": (ctypes.c_size_t, []),
    "f3r_scene_extent": (ctypes.c_int, [_c_vp, _c_i64, ctypes.POINTER(_c_i64), _c_vp, ctypes.c_size_t, _c_vp, _c_vp]),
    "f3r_scene_collect_count": (ctypes.c_int, [_c_vp, ctypes.c_int, _c_i64, _c_vp, _c_vp]),
    "f3r_scene_collect_write": (ctypes.c_int, [_c_vp, ctypes.c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_ply_pack": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_vp, _c_vp]),
    "f3r_color_range": (ctypes.c_int, [_c_vp, _c_i64, ctypes.c_int, _c_vp, _c_vp]),
    "f3r_color_to_u8": (ctypes.c_int, [_c_vp, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _c_vp, _c_vp]),
    "f3r_sky_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "f3r_sky_detect": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_vp,
                                      ctypes.c_size_t, _c_vp, _c_vp, _c_vp]),
    "f3r_mesh_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "f3r_mesh_threshold": (ctypes.c_int, [_c_vp, ctypes.c_int, _c_vp, _c_vp, _c_vp]),
    "f3r_mesh_count": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_i64, _c_i64, _c_i64, _c_vp, ctypes.c_int, _c_vp,
                                      ctypes.c_size_t, _c_vp, _c_vp]),
    "f3r_mesh_write": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_i64, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, _c_vp, ctypes.c_size_t, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_mesh_ply_pack": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_vp, _c_i64, ctypes.c_int, _c_vp, _c_vp]),
    "f3r_cloud_combine_count": (ctypes.c_int, [_c_vp, ctypes.c_int, _c_i64, _c_vp, _c_vp, _c_vp]),
    "f3r_cloud_combine_write": (ctypes.c_int, [_c_vp, ctypes.c_int, _c_i64, _c_vp, _c_vp, ctypes.c_int, _c_vp, _c_vp, _c_vp]),
    "f3r_cloud_bounds": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_vp]),
    "f3r_cloud_voxel_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "f3r_cloud_voxel_sort": (ctypes.c_int, [_c_vp, _c_i64, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.POINTER(ctypes.c_int), _c_vp,
                                            ctypes.c_size_t, _c_vp, _c_vp]),
    "f3r_cloud_voxel_sums": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp, ctypes.c_size_t, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_cloud_fps_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "f3r_cloud_fps": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_vp, ctypes.c_size_t, _c_vp, _c_vp]),
    "f3r_cloud_mark": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp]),
    "f3r_cloud_gather": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "f3r_render_clear": (ctypes.c_int, [_c_vp, ctypes.c_int, ctypes.c_int, _c_vp]),
    "f3r_render_splat": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, _c_i64, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                        _c_vp, _c_vp]),
    "f3r_render_resolve": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _c_vp, _c_vp, _c_vp]),
    "f3r_render_center": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp]),
    "f3r_raster_workspace_bytes": (ctypes.c_size_t, [_c_i64]),
    "f3r_raster_triangles": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64, _c_i64, ctypes.POINTER(ctypes.c_double),
                                            ctypes.c_int, ctypes.c_int, _c_vp, _c_vp, ctypes.c_size_t, _c_i64, _c_vp]),
    "f3r_maps_colorize": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_gtview_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "f3r_gtview_resample": (ctypes.c_int, [_c_vp] + [ctypes.c_int] * 5 + [_c_vp, _c_vp, ctypes.c_int, ctypes.c_int, _c_vp, _c_vp] + [ctypes.c_int] * 9
                            + [_c_vp, _c_vp, _c_vp, ctypes.c_size_t, _c_vp]),
    "f3r_gtview_unproject": (ctypes.c_int, [_c_vp, _c_vp] + [ctypes.c_int] * 5 + [_c_vp, _c_vp] + [ctypes.c_int] * 8 + [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_depth_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int]),
    "f3r_depth_medians": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_i64, ctypes.c_int, ctypes.c_int, _c_f32, _c_vp, _c_i64, _c_vp]),
    "f3r_depth_errors": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                        ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.c_int, _c_vp, ctypes.c_size_t, _c_vp, _c_i64, _c_vp]),
    "f3r_depth_sparsify": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_int, _c_vp, ctypes.c_size_t, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp]),
    "f3r_match_index_bytes": (ctypes.c_size_t, [ctypes.POINTER(_c_i64), ctypes.c_int]),
    "f3r_match_workspace_bytes": (ctypes.c_size_t, [_c_i64, ctypes.c_int]),
    "f3r_match_index": (ctypes.c_int, [_c_vp, _c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, ctypes.c_size_t, _c_vp, ctypes.c_size_t, _c_vp]),
    "f3r_match_search": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, ctypes.POINTER(_c_i32), _c_vp, ctypes.POINTER(_c_i64),
                                        ctypes.c_int, _c_vp, _c_vp, _c_vp]),
    "f3r_match_count": (ctypes.c_int, [_c_vp, _c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, ctypes.POINTER(_c_i32), _c_vp,
                                       ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "f3r_match_write": (ctypes.c_int, [_c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, ctypes.POINTER(_c_i32), _c_vp, ctypes.POINTER(_c_i64),
                                       ctypes.c_int, _c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                       _c_i64, _c_vp]),
    "f3r_clean_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "f3r_clean_confidence": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp,
                                            ctypes.POINTER(_c_i32), _c_i64, ctypes.c_double, _c_f32, ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp,
                                            ctypes.c_size_t, _c_vp]),
    "f3r_galign_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "f3r_galign_loss_grad": (ctypes.c_int, [_c_vp] * 7 + [ctypes.POINTER(_c_i64), ctypes.c_int, _c_vp, ctypes.POINTER(_c_i32), ctypes.c_int, _c_vp,
                                            ctypes.POINTER(_c_i64), _c_vp, ctypes.POINTER(_c_i32), ctypes.c_int] + [_c_vp] * 8
                             + [ctypes.c_size_t, _c_vp]),
}

# entry points added after ABI_VERSION: {symbol: the f3r_version() that first exports it}.  lib() binds one only when the loaded library
# reports that version; entry() is the one place that tells a caller of a later symbol to rebuild an older library.
SYMBOL_SINCE = {name: 420 for name in SYMBOLS if name.startswith("f3r_cloud_")}
SYMBOL_SINCE_430 = {name: 430 for name in SYMBOLS if name.startswith("f3r_render_")}  # the point-splat renderer
# entry points gated by presence, not by version (f3r_version() did not move for them): lib() binds one only when the loaded library exports
# it, and entry() tells the caller of an absent one to rebuild.  The triangle rasteriser
SYMBOL_IF_PRESENT = frozenset(name for name in SYMBOLS if name.startswith("f3r_raster_"))
SYMBOL_IF_PRESENT_MAPS = frozenset(name for name in SYMBOLS if name.startswith("f3r_maps_"))  # the map pictures, gated the same way
SYMBOL_IF_PRESENT_VIEWS = frozenset(name for name in SYMBOLS if name.startswith("f3r_gtview_"))  # the ground-truth views, gated the same way
SYMBOL_IF_PRESENT_DEPTH = frozenset(name for name in SYMBOLS if name.startswith("f3r_depth_"))  # the multi-view depth metrics, gated the same way
SYMBOL_IF_PRESENT_MATCH = frozenset(name for name in SYMBOLS if name.startswith("f3r_match_"))  # view matching, gated the same way
SYMBOL_IF_PRESENT_CLEAN = frozenset(name for name in SYMBOLS if name.startswith("f3r_clean_"))  # confidence cleaning, gated the same way
SYMBOL_IF_PRESENT_GALIGN = frozenset(name for name in SYMBOLS if name.startswith("f3r_galign_"))  # global alignment, gated the same way


def symbol_since(name: str) -> int:
    """the f3r_version() that first exports `name`: the one lookup of lib() and entry() over the tables above (0: ABI_VERSION has it)"""
    return SYMBOL_SINCE.get(name, SYMBOL_SINCE_430.get(name, 0))


def if_present(name: str) -> bool:
    """is `name` gated by presence: the one lookup of lib() and entry() over the seven sets above"""
    return (name in SYMBOL_IF_PRESENT or name in SYMBOL_IF_PRESENT_MAPS or name in SYMBOL_IF_PRESENT_VIEWS or name in SYMBOL_IF_PRESENT_DEPTH
            or name in SYMBOL_IF_PRESENT_MATCH or name in SYMBOL_IF_PRESENT_CLEAN or name in SYMBOL_IF_PRESENT_GALIGN)


LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libf3r_hip.so")
if os.environ.get("F3R_LAB_LIB"):  # measurement builds only (tools/lab: kernels with ablation bits); never set by the product or the tests
    LIB_PATH = os.environ["F3R_LAB_LIB"]
_lib = None


class F3RError(RuntimeError):
    pass


ABI_VERSION = 410  # the oldest f3r_version() lib() accepts; entry points of a later version are listed in SYMBOL_SINCE / SYMBOL_SINCE_430 and reached through entry()


def lib():
    """Load (once) and return the shared library.  Raises loudly if it is missing: there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise F3RError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(fast3r_amd has no CPU / torch fallback)")
        l = ctypes.CDLL(LIB_PATH)

        def bind(name):
            fn = getattr(l, name)  # AttributeError if the .so does not export what the header declares
            fn.restype, fn.argtypes = SYMBOLS[name]

        bind("f3r_version")  # first: an older library lacks later symbols, and "rebuild it" says more than an AttributeError
        if l.f3r_version() < ABI_VERSION:
            raise F3RError(f"{LIB_PATH} is version {l.f3r_version()}, this host code needs >= {ABI_VERSION}: rebuild it (fast3r_amd/csrc/build.sh)")
        for name in SYMBOLS:
            if if_present(name) and not hasattr(l, name):
                continue
            if symbol_since(name) <= l.f3r_version():
                bind(name)
        if l.f3r_sizeof(0) != ctypes.sizeof(GemmArgs) or l.f3r_sizeof(1) != ctypes.sizeof(AttnArgs) or l.f3r_sizeof(2) != ctypes.sizeof(AttnF32Args):
            raise F3RError("fast3r_amd/_lib.py struct layout does not match include/f3r.h "
                           f"(gemm {l.f3r_sizeof(0)} vs {ctypes.sizeof(GemmArgs)}, attn {l.f3r_sizeof(1)} vs {ctypes.sizeof(AttnArgs)}, "
                           f"attn_f32 {l.f3r_sizeof(2)} vs {ctypes.sizeof(AttnF32Args)}): rebuild the library (fast3r_amd/csrc/build.sh)")
        _lib = l
    return _lib


def library_version() -> int:
    return lib().f3r_version()


def entry(name: str):
    """The bound entry point `name` of the loaded library; F3RError if that library predates it (symbol_since)."""
    l = lib()
    have, need = library_version(), symbol_since(name)
    if have < need:
        raise F3RError(f"{LIB_PATH} is version {have}, {name} needs >= {need}: rebuild it (fast3r_amd/csrc/build.sh)")
    if if_present(name) and not hasattr(l, name):
        raise F3RError(f"{LIB_PATH} does not export {name}: rebuild it (fast3r_amd/csrc/build.sh)")
    return getattr(l, name)


def check(status: int, what: str = ""):
    """Map a negative f3r_status onto a Python exception (ValueError for argument errors, like the reference's
    asserts / ValueErrors on bad shapes; RuntimeError for launch failures)."""
    if status == 0:
        return
    msg = lib().f3r_last_error_string().decode(errors="replace")
    if status in (-1, -2):
        raise ValueError(f"{what}: {msg} (f3r_status {status})")
    raise F3RError(f"{what}: {msg} (f3r_status {status})")


def dtype_id(dt: torch.dtype) -> int:
    if dt == torch.float16:
        return F3R_F16
    if dt == torch.bfloat16:
        return F3R_BF16
    raise ValueError(f"fast3r_amd: MFMA operand dtype must be torch.float16 or torch.bfloat16, got {dt}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def require_gpu(t: torch.Tensor, name="tensor"):
    if not t.is_cuda:
        raise F3RError(f"fast3r_amd: {name} lives on {t.device}; the HIP kernels need a ROCm device "
                       "(there is no CPU fallback -- the CPU path is oracle/, test infrastructure only)")


def work_device(t: torch.Tensor, what="tensor"):
    """Where the kernels run for `t`: its own ROCm device, or -- for a CPU tensor, e.g. the preds `inference()` hands back after its
    `to_cpu` (inference_multiview.py:92) -- the current ROCm device (the caller uploads, runs the kernels, and returns results on
    `t.device`).  Still no CPU *compute* path: without a GPU this raises."""
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise F3RError(f"fast3r_amd: {what} lives on {t.device} and no ROCm device is available; the HIP kernels need one "
                       "(there is no CPU fallback -- the CPU path is oracle/, test infrastructure only)")
    return torch.device("cuda", torch.cuda.current_device())
