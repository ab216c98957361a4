"""ctypes binding of libbodyslam_hip.so (include/bodyslam_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every compute call below hands raw
device pointers to the C ABI.  There is NO fallback: if the shared library is missing or a call
fails, an exception is raised (BodySlamHipError) -- the product path never silently computes on
the CPU or through torch ops.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BODYSLAM_HIP_LIB") or os.path.join(_HERE, "libbodyslam_hip.so")      # (the override: A/B runs of two builds in one call)

F32, F16, BF16 = 0, 1, 2
F64 = 3                         # bs_similarity_fit only
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SOFTPLUS, ACT_SOFTPLUS_FAST = 0, 1, 2, 3, 4
OUT_PLAIN, OUT_SHUFFLE, OUT_QKV = 0, 1, 2

_TORCH2BS = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
BS2TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}


class BodySlamHipError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("dtype", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int32), ("conv", C.c_int32),
        ("Hin", C.c_int32), ("Win", C.c_int32), ("Cin", C.c_int32), ("Hout", C.c_int32), ("Wout", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("pad_h", C.c_int32), ("pad_w", C.c_int32),
        ("relu_a", C.c_int32),
        ("bias", C.c_void_p), ("bias_group_rows", C.c_int32), ("act", C.c_int32),
        ("scale", C.c_void_p), ("res", C.c_void_p), ("res_dtype", C.c_int32), ("ldr", C.c_int32), ("res2", C.c_void_p),
        ("out", C.c_void_p), ("out2", C.c_void_p), ("out3", C.c_void_p),
        ("out_dtype", C.c_int32), ("ldo", C.c_int32), ("out_mode", C.c_int32),
        ("out_group_rows", C.c_int32), ("out_group_stride", C.c_int32), ("out_row_offset", C.c_int32),
        ("shuffle_s", C.c_int32), ("shuffle_cout", C.c_int32),
        ("qkv_hidden", C.c_int32), ("qkv_tokens", C.c_int32), ("qkv_sp", C.c_int32), ("q_scale", C.c_float),
        ("tile", C.c_int32), ("seg1", C.c_int32), ("out_split_off", C.c_int32), ("res_split_off", C.c_int32),
        ("f8_seg", C.c_int32), ("f8_scales", C.c_uint32), ("out_f8", C.c_int32), ("res_f8", C.c_int32),
        ("qkv_cls_last", C.c_int32), ("qkv_cls_rows", C.c_int32), ("qkv_patch_row0", C.c_int32), ("f8_wonly_from", C.c_int32), ("out_lo8_rows", C.c_int32),
        ("f8_skip_from", C.c_int32), ("bias2_row0", C.c_int32), ("bias2_group_rows", C.c_int32), ("out_planes_rows", C.c_int32),
        ("bias2", C.c_void_p),
        ("qkv_lo_off", C.c_int32), ("out2_relu", C.c_int32),
    ]


_lib: Optional[C.CDLL] = None

_SIGS = {
    "bs_init": [C.c_int],
    "bs_version": [],
    "bs_gemm": [C.POINTER(GemmDesc), C.c_void_p],
    "bs_gemm_tile": [C.POINTER(GemmDesc)],
    "bs_attention": [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p],
    "bs_attention_table": [C.c_void_p] * 5 + [C.c_int32] * 7 + [C.c_void_p],
    "bs_attention_table_corr": [C.c_void_p] * 8 + [C.c_int32] * 7 + [C.c_void_p],
    "bs_layernorm": [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p],
    "bs_cast": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p],
    "bs_copy_f32": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "bs_cast_split": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p],
    "bs_relu_split": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p],
    "bs_preprocess_patches": [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p],
    "bs_preprocess_image": [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p],
    "bs_fill_rows": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
    "bs_resize_bilinear_nhwc": [C.c_void_p, C.c_void_p] + [C.c_int32] * 8 + [C.c_void_p],
    "bs_upconv_tapsum": [C.c_void_p] * 3 + [C.c_int32] * 9 + [C.c_void_p],
    "bs_upconv_fused": [C.c_void_p] * 4 + [C.c_int32] * 15 + [C.c_void_p],
    "bs_resize_bias_relu_nhwc": [C.c_void_p] * 3 + [C.c_int32] * 8 + [C.c_void_p],
    "bs_col_mean": [C.c_void_p, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p],
    "bs_rank1_bias": [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p],
    "bs_depth_u16_to_m": [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p],
    "bs_engine_load": [C.c_char_p, C.c_void_p],
    "bs_engine_destroy": [C.c_void_p],
    "bs_engine_io": [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p],
    "bs_engine_device_bytes": [C.c_void_p],
    "bs_engine_run": [C.c_void_p, C.c_void_p],
    "bs_engine_upload": [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64],
    "bs_engine_download": [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64],
    "bs_zoedepth_forward": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_cyclepose_forward": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
    "bs_tsdf_frames_upload": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
    "bs_tsdf_touch_batch": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                            C.c_void_p],
    "bs_tsdf_integrate_batch": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p],
    "bs_tsdf_update_batch": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_void_p],
    "bs_odo_prepare": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_odo_pyrdown": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p],
    "bs_odo_sobel": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_odo_accumulate": [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_void_p],
    "bs_odo_step": [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p],
    "bs_odo_p2p_prepare": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p],
    "bs_odo_p2p_target": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_odo_p2p_accumulate": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                              C.c_void_p],
    "bs_odo_p2p_step": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p,
                        C.c_void_p, C.c_void_p],
    "bs_tsdf_extract": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_tsdf_mesh": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32] + [C.c_void_p] * 7,
    "bs_tsdf_raycast": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                        C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_attractor_step": [C.c_void_p] * 4 + [C.c_int32] * 8 + [C.c_void_p],
    "bs_add_resized": [C.c_void_p] * 3 + [C.c_int32] * 7 + [C.c_void_p],
    "bs_mlp2": [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32] * 6 + [C.c_void_p],
    "bs_mlp2_add": [C.c_void_p] * 7 + [C.c_int32] * 10 + [C.c_void_p],
    "bs_projector_level": [C.c_void_p] * 10 + [C.c_int32] * 9 + [C.c_void_p],
    "bs_logbinom_depth": [C.c_void_p] * 8 + [C.c_int32] * 5 + [C.c_float, C.c_float, C.c_int32, C.c_void_p],
    "bs_logbinom_depth_ex": [C.c_void_p] * 7 + [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_float, C.c_float, C.c_int32, C.c_void_p],
    "bs_small_attention": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
    "bs_route_argmax": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p],
    "bs_postprocess_depth": [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p],
    "bs_cyclepose_im2col": [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p],
    "bs_cyclepose_im2col_window": [C.c_void_p] * 3 + [C.c_int32] * 8 + [C.c_void_p],
    "bs_instnorm_relu_nhwc": [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_float, C.c_int32, C.c_void_p],
    "bs_avgpool_nhwc": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
    "bs_cyclepose_head": [C.c_void_p] * 12 + [C.c_int32] * 3 + [C.c_void_p],
    "bs_backproject": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 6,
    "bs_pose_chain": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pose_chain_from": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pixel_to_3d": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_depth_metrics_workspace": [C.c_int32, C.c_int32, C.c_int32],
    "bs_depth_metrics": [C.c_void_p, C.c_void_p] + [C.c_int32] * 3 + [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                                                       C.c_void_p, C.c_void_p],
    "bs_similarity_fit": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_trajectory_metrics": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p],
    # sparse-feature scale path (csrc/sparse_features.hip); `levels` and the other host tables are passed as pointers to numpy arrays
    "bs_orb_pyramid": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_orb_fast": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_orb_select": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_orb_describe": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_orb_match": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_orb_displacement": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_void_p],
    # loop closure (csrc/loop_closure.hip)
    "bs_orb_lift": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_orb_match_pairs": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_loop_register": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                         C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p],
    # pose graph (csrc/posegraph.hip)
    "bs_pg_linearise": [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 8,
    "bs_pg_assemble": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5,
    "bs_pg_solve": [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7,
    "bs_pg_update": [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4,
    # cloud-to-cloud distances (csrc/pointcloud.hip); lo, hi, dims, thresholds and the affine are pointers to host arrays
    "bs_pc_bounds": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_pc_grid_count": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_grid_scatter": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_pc_query_grid": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int32,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_query_brute": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_transform": [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_stats": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    # k nearest neighbours, normals, the mean neighbour distance (csrc/knn.hip); the orientation vector is a pointer to 3 host doubles
    "bs_pc_query_knn": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_normals": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_knn_mean_distance": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p],
    # radius search and DBSCAN (csrc/radius.hip); the index arguments as for bs_pc_query_knn
    "bs_pc_radius_count": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                           C.c_void_p, C.c_void_p],
    "bs_pc_radius_fill": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_radius_sort": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_pc_radius_unpack": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_dbscan_hook": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                          C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_dbscan_compress": [C.c_void_p, C.c_int64, C.c_void_p],
    "bs_pc_dbscan_roots": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_pc_dbscan_labels": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                            C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    # orientation of normals along a minimum spanning tree (csrc/orient.hip); every pointer is a device pointer
    "bs_pc_orient_edges": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_orient_clear": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "bs_pc_orient_select": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_orient_select_hi": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_orient_hook": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_orient_compress": [C.c_void_p, C.c_int64, C.c_void_p],
    "bs_pc_orient_seed": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_pc_orient_flip": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                          C.c_void_p],
    # voxel down-sampling (csrc/voxel.hip); the origin is a pointer to 3 host doubles
    "bs_pc_voxel_assign": [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_voxel_flags": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_voxel_accumulate": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_pc_voxel_finish": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                           C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    # triangle-mesh scene (csrc/mesh_scene.hip); every pointer is a device pointer
    "bs_mesh_records": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_cast_brute": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6,
    "bs_mesh_closest_brute": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int32] +
                             [C.c_void_p] * 6,
    "bs_mesh_grid_count": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p],
    "bs_mesh_grid_scatter": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_mesh_cast_grid": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                          C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 8,
    "bs_mesh_closest_grid": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_int64,
                             C.c_float, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 8,
    "bs_mesh_hits_grid": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                          C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4,
    "bs_mesh_hits_brute": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_hits_unpack": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 5,
    "bs_mesh_sample_weights": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_sample": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64] + [C.c_void_p] * 5,
    # mesh topology and clean-up (csrc/mesh_ops.hip); every pointer is a device pointer
    "bs_mesh_edge_insert": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_edge_flags": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_edge_rows": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6,
    "bs_mesh_cc_hook": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_cc_compress": [C.c_void_p, C.c_int64, C.c_void_p],
    "bs_mesh_cc_roots": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_mesh_cc_clusters": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_orient_hook": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_orient_compress": [C.c_void_p, C.c_int64, C.c_void_p],
    "bs_mesh_orient_check": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_orient_flip": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_segment_sum": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_mesh_triangle_geometry": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_vertex_normals": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_mesh_laplacian_step": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_void_p],
    # is this mesh a solid (csrc/mesh_solid.hip); every pointer is a device pointer
    "bs_mesh_fan_hook": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_fan_compress": [C.c_void_p, C.c_int64, C.c_void_p],
    "bs_mesh_fan_count": [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_solid_records": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_mesh_pairs_grid": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                           C.c_float, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5,
    "bs_mesh_pairs_brute": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] +
                           [C.c_void_p] * 4,
    "bs_mesh_signed_volume": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    # rigid ICP registration (csrc/icp.hip); lo, hi and dims are pointers to host arrays
    "bs_icp_step": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                    C.c_int32, C.c_int64, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_icp_finish": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p],
    # global registration (csrc/global_registration.hip); every pointer is a device pointer
    "bs_fpfh_spfh": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_fpfh_features": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
    "bs_feature_match": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p],
    "bs_gr_hypotheses": [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_gr_score": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p],
    "bs_gr_winner": [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p],
    "bs_gr_winner_fit": [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_void_p],
    "bs_gr_refit_step": [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p],
    "bs_gr_refit_finish": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p],
}
EXPORTS = sorted(list(_SIGS) + ["bs_last_error"])


def load_library() -> C.CDLL:
    """dlopen the in-tree library and declare every prototype.  No GPU is needed for this."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BodySlamHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C bodyslam_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.bs_last_error.restype = C.c_char_p
    lib.bs_last_error.argtypes = []
    lib.bs_engine_device_bytes.restype = C.c_int64
    lib.bs_depth_metrics_workspace.restype = C.c_int64
    _lib = lib
    return lib


_inited_device: Optional[int] = None


def init(device: int = 0) -> None:
    global _inited_device
    lib = load_library()
    if _inited_device == device:
        return
    if not torch.cuda.is_available():
        raise BodySlamHipError("bodyslam_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                               "and there is no CPU fallback")
    check(lib.bs_init(device), "bs_init")
    _inited_device = device


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load_library().bs_last_error().decode(errors="replace")
        raise BodySlamHipError(f"{what} failed with status {status}: {msg}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def dt(t: torch.Tensor) -> int:
    return _TORCH2BS[t.dtype]


def p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------
# thin typed wrappers (argument checking that needs tensor metadata lives here; numeric argument
# validation lives in the C library)
# ---------------------------------------------------------------------------------------------
def make_gemm_desc(A: torch.Tensor, W: torch.Tensor, out: torch.Tensor, *, M: int, N: int, K: int, lda: int,
                   conv=None, relu_a: bool = False, bias: Optional[torch.Tensor] = None, bias_group_rows: int = 0,
                   act: int = ACT_NONE, scale: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                   res2: Optional[torch.Tensor] = None, ldr: int = 0, ldo: Optional[int] = None, out_group=None,
                   shuffle=None, qkv=None, a_offset: int = 0, tile: int = 0, seg1: int = 0, out_split_off: int = 0,
                   res_split_off: int = 0, f8_seg: int = 0, f8_scales=(127, 127, 127, 127), out_f8=None, res_f8: bool = False,
                   f8_wonly_from: int = 0, out_lo8_rows: int = 0, f8_skip_from: int = 0, bias2=None, out_planes_rows: int = 0,
                   out_relu: Optional[torch.Tensor] = None) -> GemmDesc:
    """Fill a bs_gemm_desc.  conv = (Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad_h, pad_w) or None;
    out_group = (rows, stride, offset); shuffle = (s, Cout, Hgrid, Wgrid);
    qkv = (hidden, tokens, Sp, q_scale, out_k, out_vt[, cls_last[, cls_rows[, patch_row0[, lo_off]]]]); a_offset in elements;
    (lo_off > 0: out / out_k / out_vt are allocated twice over and the rounding residuals go lo_off elements behind the values)
    bias2 = (fp32 [groups, N], row0, group_rows)."""
    d = GemmDesc()
    d.A = A.data_ptr() + a_offset * A.element_size()
    d.W = W.data_ptr()
    assert A.dtype == W.dtype and A.dtype in (torch.float16, torch.bfloat16), (A.dtype, W.dtype)
    d.dtype = dt(A)
    d.M, d.N, d.K, d.lda = M, N, K, lda
    if conv is not None:
        d.conv = 1
        (d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.KH, d.KW, d.stride, d.pad_h, d.pad_w) = conv
    d.relu_a = int(relu_a)
    if bias is not None:
        assert bias.dtype == torch.float32
        d.bias = bias.data_ptr()
    d.bias_group_rows = bias_group_rows
    d.act = act
    if scale is not None:
        assert scale.dtype == torch.float32
        d.scale = scale.data_ptr()
    if res is not None:
        d.res = res.data_ptr()
        d.res_dtype = dt(res)
        d.ldr = ldr if ldr else N
    if res2 is not None:
        assert res is not None and res2.dtype == A.dtype
        d.res2 = res2.data_ptr()
    d.out = out.data_ptr()
    d.out_dtype = dt(out)
    d.ldo = N if ldo is None else ldo
    if out_group is not None:
        d.out_group_rows, d.out_group_stride, d.out_row_offset = out_group
    if shuffle is not None:
        d.out_mode = OUT_SHUFFLE
        d.shuffle_s, d.shuffle_cout, d.Hout, d.Wout = shuffle
    if qkv is not None:
        d.out_mode = OUT_QKV
        hidden, tokens, sp, q_scale, out_k, out_vt = qkv[:6]
        d.qkv_cls_last = int(bool(qkv[6])) if len(qkv) > 6 else 0
        d.qkv_cls_rows = int(qkv[7]) if len(qkv) > 7 else 0
        d.qkv_patch_row0 = int(qkv[8]) if len(qkv) > 8 else d.qkv_cls_rows
        d.qkv_lo_off = int(qkv[9]) if len(qkv) > 9 else 0
        d.qkv_hidden, d.qkv_tokens, d.qkv_sp, d.q_scale = hidden, tokens, sp, q_scale
        d.out2 = out_k.data_ptr()
        d.out3 = out_vt.data_ptr()
    d.tile = tile
    d.seg1, d.out_split_off, d.res_split_off = seg1, out_split_off, res_split_off
    d.f8_seg = f8_seg
    d.f8_scales = f8_scales[0] | (f8_scales[1] << 8) | (f8_scales[2] << 16) | (f8_scales[3] << 24)
    d.out_f8 = 0 if out_f8 is None else ((out_f8[0] & 0xff) | ((out_f8[1] & 0xff) << 8))
    d.res_f8 = int(res_f8)
    d.f8_wonly_from = f8_wonly_from
    d.out_lo8_rows = out_lo8_rows
    d.f8_skip_from = f8_skip_from
    d.out_planes_rows = out_planes_rows
    if bias2 is not None:
        b2, row0, grows = bias2
        assert b2.dtype == torch.float32 and b2.shape[-1] == N
        d.bias2, d.bias2_row0, d.bias2_group_rows = b2.data_ptr(), row0, grows
    if out_relu is not None:         # second output: relu(y) in out's (hi16 | hi8 | lo8) format (bs_gemm_desc.out2_relu)
        assert qkv is None and out_f8 is not None and out_relu.dtype == out.dtype and out_relu.numel() == out.numel()
        d.out2 = out_relu.data_ptr()
        d.out2_relu = 1
    return d


def gemm(A: torch.Tensor, W: torch.Tensor, out: torch.Tensor, **kw) -> None:
    d = make_gemm_desc(A, W, out, **kw)
    check(load_library().bs_gemm(C.byref(d), stream_ptr()), "bs_gemm")


def _gemm_bytes(d) -> float:
    rows_in = float(d.M if not d.conv else d.M / max(d.stride * d.stride, 1))
    rows_f8 = 0.0 if d.f8_skip_from < 0 else (rows_in if (d.conv or not d.f8_skip_from) else float(min(d.f8_skip_from, d.M)))
    taps = d.KH * d.KW if d.conv else 1
    a = rows_in * (d.Cin if d.conv else d.K) * 2 + rows_f8 * d.f8_seg
    w = float(d.N) * (d.K * 2 + taps * d.f8_seg)
    if d.out_dtype == F32:
        per_row = [4.0, 4.0, 4.0]
    elif d.out_f8:              # (hi16 | hi8 | lo8): 4 B; without the lo8 plane 3 B; hi16 alone 2 B
        per_row = [4.0, 3.0, 2.0]
    else:
        per_row = [2.0 * (2 if d.out_split_off else 1)] * 3
    full = float(d.M)
    r_planes = float(min(d.out_planes_rows, d.M)) if d.out_planes_rows else full            # rows that keep any plane
    r_lo = float(min(d.out_lo8_rows, d.M)) if d.out_lo8_rows else r_planes                   # rows that keep the lo8 plane
    r_lo = min(r_lo, r_planes)
    out = d.N * (r_lo * per_row[0] + (r_planes - r_lo) * per_row[1] + (full - r_planes) * per_row[2])
    res = float(d.M) * d.N * (4 if (d.res and d.res_dtype == F32) else 0)
    return a + w + out + res


class Plan:
    """A prebuilt sequence of C-ABI calls over static buffers: descriptors and pointer arguments are
    marshalled once, so replaying a forward costs one ctypes call per kernel (and the whole sequence
    can be captured into a HIP graph).  `mark(name, tensor)` records a named intermediate for tests."""

    def __init__(self, device=None):
        # the device whose streams the plan is issued on (an engine passes its own; None = torch's current device at run time)
        self.device = None if device is None else torch.device(device)
        self.calls = []      # (cfunc, args) ; args exclude the trailing stream
        self.names = []
        self.keep = []       # keeps descriptors / tensors alive
        self.keep_descs = [] # the bs_gemm descriptors in call order (engine export)
        self.marks = {}      # call index -> [(name, tensor)]
        self.gemm_info = {}  # call index -> dict(tile, conv, flops, bytes)
        self.stack_info = {} # call index -> dict(name, alg_flops, flops): launches other than bs_gemm that carry matrix-core work of a GEMM / conv
                             # the reference has (the fused up-convolution, the attractor MLPs): timed with the GEMMs for the roofline
        self.events = None   # a list: run() records a HIP event pair around every bs_gemm launch into it (see run_timed)
        self._graph = None   # torch.cuda.CUDAGraph of the captured sequence (capture())

    def gemm(self, name, A, W, out, **kw):
        passes = kw.pop("precision_passes", 1)
        d = make_gemm_desc(A, W, out, **kw)
        kw["precision_passes"] = passes
        self.keep.append((d, A, W, out, kw))
        self.keep_descs.append(d)
        self.calls.append((load_library().bs_gemm, (C.byref(d),)))
        self.names.append(name)
        # bookkeeping for the roofline: which kernel instantiation and how many algorithmic FLOPs
        self.gemm_info[len(self.calls) - 1] = dict(
            name=name, tile=load_library().bs_gemm_tile(C.byref(d)), conv=bool(d.conv),
            # executed work in 16-bit-MFMA-equivalents: an FP8 correction stage covers 128 k in the time of 64
            # (tiles past f8_wonly_from run only the first FP8 half)
            # (tiles past f8_skip_from run none)
            flops=2.0 * d.N * (d.M * d.K + (0 if d.f8_skip_from < 0 else (min(d.f8_skip_from, d.M) if d.f8_skip_from else d.M)) * (d.KH * d.KW if d.conv else 1) * d.f8_seg
                               / (4 if d.f8_wonly_from else 2)),
            # algorithmic FLOPs exclude the extra passes of a split-precision product
            alg_flops=2.0 * d.M * d.N * (d.K / kw.get("precision_passes", 1)),
            # algorithmic HBM bytes: A once (16-bit values + the FP8 planes of the rows that run FP8 stages), W once, the output
            # (+ the fp32 residual read)
            bytes=_gemm_bytes(d))

    def add(self, name, fn_name, *args):
        cargs = []
        for a in args:
            if isinstance(a, torch.Tensor):
                self.keep.append(a)
                cargs.append(a.data_ptr())
            else:
                cargs.append(a)
        self.calls.append((getattr(load_library(), fn_name), tuple(cargs)))
        self.names.append(name)

    def tag_stack(self, alg_flops: float, flops: float):
        """the call added last carries this much matrix-core work (algorithmic / executed in 16-bit-pass equivalents)"""
        self.stack_info[len(self.calls) - 1] = dict(name=self.names[-1], alg_flops=float(alg_flops), flops=float(flops))

    def mark(self, name, tensor, meta=None):
        self.marks.setdefault(len(self.calls), []).append((name, tensor, meta))

    def run_timed(self, events: list):
        """Like run(), with a HIP event pair (recorded on the launch stream) around every bs_gemm launch;
        appends (call_index, start_event, end_event) to `events`."""
        stream = torch.cuda.current_stream(self.device)
        st = stream.cuda_stream
        for i, (fn, args) in enumerate(self.calls):
            if i in self.gemm_info or i in self.stack_info:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = fn(*args, st)
                e1.record(stream)
                events.append((i, e0, e1))
            else:
                rc = fn(*args, st)
            if rc:
                check(rc, self.names[i])

    def capture(self):
        """Capture the whole launch sequence (with the GEMM tail launches the library forks itself) into one HIP graph;
        run() then replays it with a single hipGraphLaunch instead of ~600 ctypes calls.  The buffers are static, so the
        captured pointers stay valid; inputs are copied into them before run() as usual.  Worth it for the reference's
        one-frame-per-call pattern (host time 3.6 ms -> ~0.1 ms per forward; the GPU time does not change)."""
        if self._graph is not None:
            return
        self.run()                              # warm-up: first-use attribute calls, the library's lazy streams and events
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(device=self.device)
        cap.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(cap):
            with torch.cuda.graph(g, stream=cap, capture_error_mode="thread_local"):
                self.run()
        torch.cuda.current_stream(self.device).wait_stream(cap)
        self._graph = g

    def run(self, taps: Optional[dict] = None):
        if taps is None and self.events is not None:      # a caller (bench.py) asked for per-launch HIP events
            return self.run_timed(self.events)
        if taps is None and self._graph is not None and not torch.cuda.is_current_stream_capturing():
            self._graph.replay()
            return
        st = torch.cuda.current_stream(self.device).cuda_stream
        if taps is None:
            for i, (fn, args) in enumerate(self.calls):
                rc = fn(*args, st)
                if rc:
                    check(rc, self.names[i])
            return
        means = taps.get("__site_means__")                # tap mode (tests, the calibration's channel means)
        for i in range(len(self.calls) + 1):
            for (name, t, meta) in self.marks.get(i, []):
                if meta and meta[0] == "chanmean":
                    # the channel means of a product's 16-bit input rows as the launch that follows will read them (the calibration's static
                    # bias correction): only when the caller asks for them, never cloned
                    if means is not None:
                        _, off, M, lda, K = meta
                        means[name] = t.view(-1)[off: off + M * lda].view(M, lda)[:, :K].float().mean(0)
                    continue
                if means is None:               # (a run made for the channel means clones nothing else)
                    taps[name] = (t.clone(), meta)
            if i < len(self.calls):
                fn, args = self.calls[i]
                check(fn(*args, st), self.names[i])


_F8_ON_DEVICE = {}      # device index -> does torch's fp32 -> e4m3 cast on that device give the CPU cast's bytes (checked once per process)


def _f8_pack_device(device):
    """where the weight planes are formed: on `device` when torch's e4m3 cast there reproduces the CPU cast bit for bit (checked once on a
    sample that covers ties, the subnormal range and the saturation bound), else on the host.  One-off weight re-layout, not the compute
    path -- but a ZoeD_NK engine packs 300 M weights, 40 s of an 8-core host against < 1 s on the GPU."""
    if device is None or os.environ.get("BS_PACK_ON_HOST") == "1":       # (the switch: A / B of the two packings)
        return torch.device("cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return torch.device("cpu")
    ok = _F8_ON_DEVICE.get(device.index)
    if ok is None:
        g = torch.Generator().manual_seed(7)
        t = torch.cat([torch.randn(4096, generator=g) * 100.0, torch.randn(4096, generator=g) * 1e-2, torch.linspace(-460.0, 460.0, 4097),
                       torch.arange(0, 4096, dtype=torch.float32) * 2.0 ** -11, torch.tensor([0.0, -0.0, 448.0, -448.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -11])])
        t = t.clamp(-448.0, 448.0)
        try:
            ok = bool(torch.equal(t.to(torch.float8_e4m3fn).view(torch.uint8), t.to(device).to(torch.float8_e4m3fn).view(torch.uint8).cpu()))
        except Exception:
            ok = False
        _F8_ON_DEVICE[device.index] = ok
    return device if ok else torch.device("cpu")


def f8_weight(w: torch.Tensor, dtype, planes: str = "both", device=None) -> tuple:
    """fp32 [N, K] -> ([N, 2K] `dtype`-typed rows of [W_hi16 | W_lo8 | W_hi8] bytes, (sb0, sb1)): the weight side of bs_gemm's
    FP8 correction segment.  W_hi8 = e4m3(W_hi * 2^e_hi), W_lo8 = e4m3((W - W_hi) * 2^e_lo) with per-matrix power-of-two
    scales that put the largest magnitude just under e4m3's 448; sb0 / sb1 are the E8M0 exponents bs_gemm applies to the
    lo / hi plane (127 - e).  planes: "both" (default), "lo" = [W_hi16 | W_lo8] only, "hi_only" = the W_lo8 plane zeroed.
    device: where the planes are formed and returned (_f8_pack_device; default: the host)."""
    import math
    w = w.detach().to(_f8_pack_device(device)).float()
    hi = w.to(dtype)
    lo = w - hi.float()

    def plane(t):
        mx = float(t.abs().max())
        e = 0 if mx == 0.0 else min(int(math.floor(math.log2(448.0 / mx))), 100)
        return (t * (2.0 ** e)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8), e

    hi8, e_hi = plane(hi.float())
    lo8, e_lo = plane(lo)
    hi16 = hi.contiguous().view(torch.uint8).view(w.shape[0], -1)
    if planes == "lo":            # [W_hi16 | W_lo8]: the weight-rounding correction only (bs_gemm f8_seg = K)
        row = torch.cat([hi16, lo8], 1).contiguous()
    elif planes == "hi_only":     # probe: no weight-rounding correction (the W_lo8 plane is zero)
        row = torch.cat([hi16, torch.zeros_like(lo8), hi8], 1).contiguous()
    else:
        row = torch.cat([hi16, lo8, hi8], 1).contiguous()
    return row.view(dtype), (127 - e_lo, 127 - e_hi)


def f8_conv_weight(w_ohwi: torch.Tensor, dtype, device=None) -> tuple:
    """fp32 [O, kh, kw, I] -> the conv-mode counterpart of f8_weight: K order [W_hi16: chunk64, tap, 64][W_lo8: chunk128, tap, 128]
    [W_hi8: chunk128, tap, 128] (the kernel's chunk walk continues from the 16-bit channels through the two FP8 planes)."""
    import math
    w = w_ohwi.detach().to(_f8_pack_device(device)).float()
    O, kh, kw, I = w.shape
    assert I % 128 == 0, I
    hi = w.to(dtype)
    lo = w - hi.float()

    def plane(t):
        mx = float(t.abs().max())
        e = 0 if mx == 0.0 else min(int(math.floor(math.log2(448.0 / mx))), 100)
        q = (t * (2.0 ** e)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        return q.reshape(O, kh, kw, I // 128, 128).permute(0, 3, 1, 2, 4).reshape(O, -1), e

    hi8, e_hi = plane(hi.float())
    lo8, e_lo = plane(lo)
    hi16 = conv_weight(hi).view(torch.uint8).view(O, -1)
    row = torch.cat([hi16, lo8, hi8], 1).contiguous()
    return row.view(dtype), (127 - e_lo, 127 - e_hi)


F8_ACT_HI_EXP, F8_ACT_LO_EXP = 0, 11          # include/bodyslam_hip.h BS_F8_ACT_*_EXP


# ---------------------------------------------------------------------------------------------
def conv_weight(w_ohwi: torch.Tensor) -> torch.Tensor:
    """[O, kh, kw, I] -> the K order bs_gemm's conv mode walks: [O][I/64 chunks][kh][kw][64] flattened to [O, kh*kw*I]."""
    O, kh, kw, I = w_ohwi.shape
    assert I % 64 == 0, I
    return w_ohwi.reshape(O, kh, kw, I // 64, 64).permute(0, 3, 1, 2, 4).reshape(O, -1).contiguous()


def conv_geom(Hin, Win, Cin, KH, KW, stride, pad):
    Hout = (Hin + 2 * pad - KH) // stride + 1
    Wout = (Win + 2 * pad - KW) // stride + 1
    return (Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad, pad)


def attention(q, k, vt, bias, out, B, nh, S, Sp, split=0):
    """split: 0 = rows [B*S, nh*64]; 16 = (hi | lo) 16-bit pairs, 32 = (hi16 | hi8 | lo8) planes, rows [B*S, 2*nh*64]"""
    check(load_library().bs_attention(p(q), p(k), p(vt), p(bias), p(out), B, nh, S, Sp, dt(q) | split, stream_ptr()), "bs_attention")


def attention_table(q, k, vt, table, out, B, nh, hp, wp, Sp, split=0, grouped=0):
    check(load_library().bs_attention_table(p(q), p(k), p(vt), p(table), p(out), B, nh, hp, wp, Sp, int(grouped), dt(q) | split, stream_ptr()),
          "bs_attention_table")


def attention_table_corr(q, k, vt, q_lo, k_lo, vt_lo, table, out, B, nh, hp, wp, Sp, split=0, grouped=0):
    """split-precision operands: x = x16 + x_lo (bs_attention_table_corr)"""
    check(load_library().bs_attention_table_corr(p(q), p(k), p(vt), p(q_lo), p(k_lo), p(vt_lo), p(table), p(out), B, nh, hp, wp, Sp, int(grouped),
                                                 dt(q) | split, stream_ptr()), "bs_attention_table_corr")


def layernorm(x, gamma, beta, out16, out32, rows, cols, eps, dtype=F16):
    check(load_library().bs_layernorm(p(x), p(gamma), p(beta), p(out16), p(out32), rows, cols, eps,
                                      dt(out16) if out16 is not None else dtype, stream_ptr()), "bs_layernorm")


def cast(x, out):
    check(load_library().bs_cast(p(x), p(out), x.numel(), dt(out), stream_ptr()), "bs_cast")


def cast_split(x, out, rows, cols, f8=False):
    """fp32 [rows, cols] -> 16-bit [rows, 2*cols] = (hi | lo),  hi = round16(x), lo = round16(x - hi);
    f8: (hi16 | hi8 | lo8), the operand format of the FP8 correction passes."""
    check(load_library().bs_cast_split(p(x), p(out), rows, cols, dt(out) | (32 if f8 else 0), stream_ptr()), "bs_cast_split")


def relu_split(x, out, rows, cols, f8=False):
    """(hi | lo) [rows, 2*cols] -> re-split relu(hi + lo); f8: the same on (hi16 | hi8 | lo8) rows."""
    check(load_library().bs_relu_split(p(x), p(out), rows, cols, dt(out) | (32 if f8 else 0), stream_ptr()), "bs_relu_split")


def preprocess_patches(frames, out, B, H, W, nh, nw, flip):
    check(load_library().bs_preprocess_patches(p(frames), p(out), B, H, W, nh, nw, int(flip), dt(out), stream_ptr()),
          "bs_preprocess_patches")


def preprocess_image(frames, out, B, H, W, nh, nw, flip):
    check(load_library().bs_preprocess_image(p(frames), p(out), B, H, W, nh, nw, int(flip), stream_ptr()), "bs_preprocess_image")


def fill_rows(x, v, B, rows_per_image, cols):
    check(load_library().bs_fill_rows(p(x), p(v), B, rows_per_image, cols, stream_ptr()), "bs_fill_rows")


def resize_bilinear_nhwc(x, out, B, Hin, Win, Cch, Hout, Wout, align_corners=True, split=False):
    check(load_library().bs_resize_bilinear_nhwc(p(x), p(out), B, Hin, Win, Cch, Hout, Wout, int(align_corners) | (4 if split == 2 else (2 if split else 0)), dt(x),
                                                 stream_ptr()), "bs_resize_bilinear_nhwc")


def depth_u16_to_m(depth_u16: torch.Tensor, depth_scale: float, depth_trunc: float) -> torch.Tensor:
    """int16-stored uint16 depth [..., H, W] on the device -> fp32 metres, values >= depth_trunc -> 0 (include/bodyslam_hip.h)"""
    assert depth_u16.dtype == torch.int16 and depth_u16.is_cuda and depth_u16.is_contiguous()
    out = torch.empty(depth_u16.shape, dtype=torch.float32, device=depth_u16.device)
    check(load_library().bs_depth_u16_to_m(p(depth_u16), depth_u16.numel(), float(depth_scale), float(depth_trunc), p(out), stream_ptr()),
          "bs_depth_u16_to_m")
    return out


def col_mean(A, lda, row0, rows_per_group, groups, row_step, K, out, zero=None):
    """bf16 [groups, K] means over every row_step-th row of each group of the 16-bit matrix A; `zero` (fp32) is cleared as well
    (include/bodyslam_hip.h)"""
    assert out.dtype == torch.bfloat16 and (zero is None or zero.dtype == torch.float32)
    check(load_library().bs_col_mean(p(A), lda, row0, rows_per_group, groups, row_step, K, p(out), p(zero), 0 if zero is None else zero.numel(),
                                     dt(A), stream_ptr()), "bs_col_mean")


def rank1_bias(abar, dw, out):
    """out [G, N] fp32 (zeroed) += abar [G, K] bf16 @ dw [N, K]^T bf16 (include/bodyslam_hip.h)"""
    assert abar.dtype == torch.bfloat16 and dw.dtype == torch.bfloat16 and out.dtype == torch.float32
    G, K = abar.shape
    N = dw.shape[0]
    assert dw.shape[1] == K and tuple(out.shape) == (G, N)
    check(load_library().bs_rank1_bias(p(abar), p(dw), p(out), G, N, K, stream_ptr()), "bs_rank1_bias")


def upconv_tapsum(y, bias, out, B, Hin, Win, Cout, Hout, Wout, align_corners=True, split=False, relu=True):
    """conv3x3(interpolate x2(x)) from the low-resolution tap products y [B, Hin, Win, 9*Cout] fp32 (include/bodyslam_hip.h)"""
    check(load_library().bs_upconv_tapsum(p(y), p(bias), p(out), B, Hin, Win, Cout, Hout, Wout,
                                          int(align_corners) | (4 if split == 2 else (2 if split else 0)), int(relu), dt(out), stream_ptr()),
          "bs_upconv_tapsum")


def upconv_fused(x, w, bias, out, B, Hin, Win, Cin, Cout, mode=0, split=0, relu=True, f8_scales=(127, 127, 127, 127)):
    """relu(conv3x3(interpolate x2, align_corners(x))) in one launch from the low-resolution input (include/bodyslam_hip.h)"""
    check(load_library().bs_upconv_fused(p(x), p(w), p(bias), p(out), B, Hin, Win, Cin, Cout, 2 * Hin, 2 * Win,
                                         1 | (4 if split == 2 else (2 if split else 0)), int(relu), mode, *[int(v) for v in f8_scales], dt(out),
                                         stream_ptr()), "bs_upconv_fused")


def resize_bias_relu_nhwc(x, bias, out, B, Hin, Win, Cch, Hout, Wout, split=False):
    """relu(bilinear(x, align_corners) + bias) on NHWC 16-bit rows / (hi | lo) pairs (include/bodyslam_hip.h)"""
    check(load_library().bs_resize_bias_relu_nhwc(p(x), p(bias), p(out), B, Hin, Win, Cch, Hout, Wout, 1 | (2 if split else 0), dt(out), stream_ptr()),
          "bs_resize_bias_relu_nhwc")


def attractor_step(A, bins_prev, bins_out, route, B, Hp, Wp, H, W, groups, n_bins, n_attr):
    check(load_library().bs_attractor_step(p(A), p(bins_prev), p(bins_out), p(route), B, Hp, Wp, H, W, groups, n_bins, n_attr,
                                           stream_ptr()), "bs_attractor_step")


def mlp2(x, ldx, W1, b1, W2, b2, out, M, K1, N1, N2, act2=ACT_SOFTPLUS_FAST):
    """out = act2(round16(relu(x W1^T + b1)) W2^T + b2) in one launch (include/bodyslam_hip.h: bs_mlp2)"""
    check(load_library().bs_mlp2(p(x), ldx, p(W1), p(b1), p(W2), p(b2), p(out), M, K1, N1, N2, act2, dt(x), stream_ptr()), "bs_mlp2")


def mlp2_add(emb, prev, W1, b1, W2, b2, out, B, Hp, Wp, H, W, K1, N1, N2, act2=ACT_SOFTPLUS_FAST, split=False):
    """bs_add_resized + bs_mlp2 in one launch (include/bodyslam_hip.h: bs_mlp2_add)"""
    check(load_library().bs_mlp2_add(p(emb), p(prev), p(W1), p(b1), p(W2), p(b2), p(out), B, Hp, Wp, H, W, K1, N1, N2, act2,
                                     dt(emb) | (16 if split else 0), stream_ptr()), "bs_mlp2_add")


def projector_level(z, b_c1, emb_prev, Wc2, b_c2, We, b_e, x_out, emb_out, eh_out, B, Hl, Wl, H, W, PM, E, NE):
    """one level of the bins head's projector path in one launch (include/bodyslam_hip.h: bs_projector_level)"""
    check(load_library().bs_projector_level(p(z), p(b_c1), p(emb_prev), p(Wc2), p(b_c2), p(We), p(b_e), p(x_out), p(emb_out), p(eh_out), B, Hl, Wl,
                                            H, W, PM, E, NE, dt(z), stream_ptr()), "bs_projector_level")


def add_resized(x, prev, out, B, Hp, Wp, H, W, Cch, split=False):
    check(load_library().bs_add_resized(p(x), p(prev), p(out), B, Hp, Wp, H, W, Cch, dt(x) | (16 if split else 0), stream_ptr()),
          "bs_add_resized")


def logbinom_depth(last, Eh, bins, w0_last, w2, b2, route, depth, B, H, W, He, We, min_temp, max_temp):
    check(load_library().bs_logbinom_depth(p(last), p(Eh), p(bins), p(w0_last), p(w2), p(b2), p(route), p(depth), B, H, W, He, We,
                                           min_temp, max_temp, dt(last), stream_ptr()), "bs_logbinom_depth")


def small_attention(qkv, out, B, S, nheads):
    check(load_library().bs_small_attention(p(qkv), p(out), B, S, nheads, dt(out), stream_ptr()), "bs_small_attention")


def route_argmax(logits, ld, route, B):
    check(load_library().bs_route_argmax(p(logits), ld, p(route), B, stream_ptr()), "bs_route_argmax")


def postprocess_depth(depth_net, depth_m, depth_u16, B, H, W, nh, nw, flip):
    check(load_library().bs_postprocess_depth(p(depth_net), p(depth_m), p(depth_u16), B, H, W, nh, nw, int(flip), stream_ptr()),
          "bs_postprocess_depth")


def cyclepose_im2col(frames, pairs, out, P, H, W):
    check(load_library().bs_cyclepose_im2col(p(frames), p(pairs), p(out), P, H, W, dt(out), stream_ptr()), "bs_cyclepose_im2col")


def instnorm_relu_nhwc(x, out, out_f32, scratch, P, HW, Cch, eps=1e-5):
    check(load_library().bs_instnorm_relu_nhwc(p(x), p(out), p(out_f32), p(scratch), P, HW, Cch, eps, dt(out), stream_ptr()),
          "bs_instnorm_relu_nhwc")


def avgpool_nhwc(x, out, P, HW, Cch):
    check(load_library().bs_avgpool_nhwc(p(x), p(out), P, HW, Cch, stream_ptr()), "bs_avgpool_nhwc")


def cyclepose_head(pooled, x2, w_skip_pool, w_skip_x2, b_skip, w1, b1, w2, b2, pose7, T, scratch, P, HW, Cch):
    check(load_library().bs_cyclepose_head(p(pooled), p(x2), p(w_skip_pool), p(w_skip_x2), p(b_skip), p(w1), p(b1), p(w2), p(b2),
                                           p(pose7), p(T), p(scratch), P, HW, Cch, stream_ptr()), "bs_cyclepose_head")


def backproject(depth_u16, K4, depth_scale, depth_trunc, poses, xyz, idx, count, scratch, B, H, W):
    Karr = (C.c_double * 4)(*[float(v) for v in K4])
    check(load_library().bs_backproject(p(depth_u16), B, H, W, C.cast(Karr, C.c_void_p), float(depth_scale), float(depth_trunc),
                                        p(poses), p(xyz), p(idx), p(count), p(scratch), stream_ptr()), "bs_backproject")


def pose_chain(t_rel, N, g0, g_abs):
    g0arr = None
    if g0 is not None:
        g0arr = C.cast((C.c_double * 16)(*[float(v) for v in g0]), C.c_void_p)
    check(load_library().bs_pose_chain(p(t_rel), N, g0arr, p(g_abs), stream_ptr()), "bs_pose_chain")


def pose_chain_from(t_rel, N, g0_dev, g_abs):
    """g0_dev: fp64 [16] device tensor (e.g. the last pose of the previous call's output)"""
    check(load_library().bs_pose_chain_from(p(t_rel), N, p(g0_dev), p(g_abs), stream_ptr()), "bs_pose_chain_from")


def pixel_to_3d(uvd, K4, out, n):
    Karr = (C.c_double * 4)(*[float(v) for v in K4])
    check(load_library().bs_pixel_to_3d(p(uvd), n, C.cast(Karr, C.c_void_p), p(out), stream_ptr()), "bs_pixel_to_3d")


DEPTH_SCALE_MEDIAN, DEPTH_SCALE_FIXED = 0, 1
DEPTH_METRICS_FIELDS = 16


def depth_metrics(pred, gt, gt_lo, gt_hi, scale, workspace, out):
    """pred, gt: int16 / uint16 [B, H, W] device tensors (uint16 values); scale None = the per-frame median scale, else the fixed value;
    workspace: uint8 device tensor of at least depth_metrics_workspace(B, H, W) bytes; out: fp64 [B, DEPTH_METRICS_FIELDS]
    (include/bodyslam_hip.h)"""
    B, H, W = pred.shape
    assert tuple(gt.shape) == (B, H, W) and pred.is_contiguous() and gt.is_contiguous()
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, DEPTH_METRICS_FIELDS) and out.is_contiguous()
    mode = DEPTH_SCALE_MEDIAN if scale is None else DEPTH_SCALE_FIXED
    check(load_library().bs_depth_metrics(p(pred), p(gt), B, H, W, float(gt_lo), float(gt_hi), mode, 0.0 if scale is None else float(scale),
                                          p(workspace), workspace.numel() * workspace.element_size(), p(out), stream_ptr()), "bs_depth_metrics")


def depth_metrics_workspace(B: int, H: int, W: int) -> int:
    return int(load_library().bs_depth_metrics_workspace(B, H, W))


TRAJ_EVO, TRAJ_TRAINING = 0, 1
TRAJ_ALIGN_ORIGIN, TRAJ_ALIGN, TRAJ_CORRECT_SCALE, TRAJ_ALL_PAIRS = 1, 2, 4, 8
TRAJ_OK, TRAJ_DEGENERATE, TRAJ_TOO_SHORT, TRAJ_BAD_OFFSETS = 0, 1, 2, 3
TRAJ_FIELDS = 40
SIMILARITY_FIT_WORKSPACE_BYTES = 131136


def similarity_fit(source, target, workspace, out):
    """source, target: [n, 3] contiguous device tensors, both fp32 or both fp64; workspace: uint8 device tensor of at least
    SIMILARITY_FIT_WORKSPACE_BYTES; out: fp64 [16] device tensor (include/bodyslam_hip.h)"""
    n = source.shape[0]
    assert tuple(source.shape) == (n, 3) and tuple(target.shape) == (n, 3) and source.is_contiguous() and target.is_contiguous()
    assert source.dtype == target.dtype and source.dtype in (torch.float32, torch.float64), (source.dtype, target.dtype)
    assert out.dtype == torch.float64 and out.numel() == 16 and out.is_contiguous()
    check(load_library().bs_similarity_fit(p(source), p(target), n, F32 if source.dtype == torch.float32 else F64, p(workspace),
                                           workspace.numel() * workspace.element_size(), p(out), stream_ptr()), "bs_similarity_fit")


def trajectory_metrics(gt, pred, offsets, protocol, delta, flags, out):
    """gt, pred: fp64 [total, 16] (or [total, 4, 4]) contiguous device tensors; offsets: int32 [S + 1] device tensor; out: fp64
    [S, TRAJ_FIELDS] device tensor (include/bodyslam_hip.h)"""
    total = gt.shape[0]
    S = offsets.numel() - 1
    assert gt.dtype == torch.float64 and pred.dtype == torch.float64 and gt.numel() == total * 16 and pred.numel() == total * 16
    assert gt.is_contiguous() and pred.is_contiguous() and offsets.dtype == torch.int32 and offsets.is_contiguous()
    assert out.dtype == torch.float64 and tuple(out.shape) == (S, TRAJ_FIELDS) and out.is_contiguous()
    check(load_library().bs_trajectory_metrics(p(gt), p(pred), p(offsets), S, total, protocol, delta, flags, p(out), stream_ptr()),
          "bs_trajectory_metrics")


PG_LINE_PROCESS, PG_SYSTEM = 1, 2
PG_STAGE_SWEEP, PG_STAGE_REDUCED, PG_STAGE_DENSE_SOLVE, PG_STAGE_BACKSUB, PG_STAGE_ALL = 1, 2, 4, 8, 15
PG_MAX_SEPARATORS, PG_NODE_WORKSPACE, PG_SLOT_FIELDS = 128, 114, 120


def _f64(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float64 and t.is_cuda and t.is_contiguous()), "fp64 contiguous device tensors"


def _i32(*ts):
    for t in ts:
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous(), "int32 contiguous device tensors"


def pg_linearise(X, T, info, src, tgt, unc, mu, flags, lw, z, q, Hss, g, cterm, cost=None):
    """X fp64 [N, 4, 4], T [E, 4, 4], info [E, 6, 6], src / tgt / unc int32 [E]; lw, q, cterm [E], z [E, 6], Hss [E, 6, 6], g [E, 6];
    cost: fp64 [>= 1] or None (include/bodyslam_hip.h)"""
    N, E = X.shape[0], src.numel()
    _f64(X, T, info, lw, z, q, Hss, g, cterm, cost)
    _i32(src, tgt, unc)
    assert X.numel() == N * 16 and T.numel() == E * 16 and info.numel() == E * 36 and tgt.numel() == E and unc.numel() == E
    assert lw.numel() == E and z.numel() == E * 6 and q.numel() == E and cterm.numel() == E
    assert (Hss is None or Hss.numel() == E * 36) and (g is None or g.numel() == E * 6)
    check(load_library().bs_pg_linearise(p(X), N, p(T), p(info), p(src), p(tgt), p(unc), E, float(mu), int(flags), p(lw), p(z), p(q), p(Hss), p(g),
                                         p(cterm), p(cost), stream_ptr()), "bs_pg_linearise")


def pg_assemble(Hss, g, row_ptr, adj, reference_node, D, b, Cc, maxes=None):
    """row_ptr int32 [N + 1], adj int32 [nnz, 3]; D [N, 6, 6], b [N, 6], Cc [N, 6, 6]; maxes fp64 [>= 2] or None"""
    N, E, nnz = row_ptr.numel() - 1, g.numel() // 6, adj.numel() // 3
    _f64(Hss, g, D, b, Cc, maxes)
    _i32(row_ptr, adj)
    assert Hss.numel() == E * 36 and D.numel() == N * 36 and b.numel() == N * 6 and Cc.numel() == N * 36
    check(load_library().bs_pg_assemble(p(Hss), p(g), E, N, p(row_ptr), p(adj), nnz, int(reference_node), p(D), p(b), p(Cc), p(maxes), stream_ptr()),
          "bs_pg_assemble")


def pg_solve(D, b, Cc, Hss, lam, segments, sep_node, node_slot, adjacent, long_edges, stages, node_ws, slots, M, vec, delta, sums=None):
    """the plan arrays are int32 device tensors (posegraph.solve_plan); node_ws [N, PG_NODE_WORKSPACE], slots [max(n_segments, 1), PG_SLOT_FIELDS],
    M [6 S, 6 S], vec [24 S], delta [N, 6]; sums fp64 [>= 2] or None"""
    N, E, S = b.numel() // 6, Hss.numel() // 36, sep_node.numel()
    nseg, nadj, nlong = segments.numel() // 2, adjacent.numel(), long_edges.numel() // 3
    _f64(D, b, Cc, Hss, node_ws, slots, M, vec, delta, sums)
    _i32(segments, sep_node, node_slot, adjacent, long_edges)
    assert D.numel() == N * 36 and Cc.numel() == N * 36 and node_slot.numel() == N and delta.numel() == N * 6
    assert node_ws.numel() >= N * PG_NODE_WORKSPACE and slots.numel() >= nseg * PG_SLOT_FIELDS and M.numel() >= 36 * S * S and vec.numel() >= 24 * S
    check(load_library().bs_pg_solve(p(D), p(b), p(Cc), p(Hss), N, E, float(lam), p(segments), nseg, p(sep_node), S, p(node_slot), p(adjacent), nadj,
                                     p(long_edges), nlong, int(stages), p(node_ws), p(slots), p(M), p(vec), p(delta), p(sums), stream_ptr()), "bs_pg_solve")


def pg_update(X, delta, Xn, terms, xnorm2=None):
    N = X.shape[0]
    _f64(X, delta, Xn, terms, xnorm2)
    assert X.numel() == N * 16 and Xn.numel() == N * 16 and delta.numel() == N * 6 and terms.numel() >= N
    check(load_library().bs_pg_update(p(X), p(delta), N, p(Xn), p(terms), p(xnorm2), stream_ptr()), "bs_pg_update")


PC_MAX_CELLS, PC_MAX_THRESHOLDS, PC_STATS_FIELDS, PC_STATS_WORKSPACE_BYTES = 1 << 24, 8, 16, 163968


def _pts(*ts):
    for t in ts:
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 3, "fp32 contiguous [n, 3] device tensors"


def _host(a, dtype, n):
    """a host array of n `dtype` values as (the array, which must stay alive over the call; its address)"""
    import numpy as np
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    assert a.size == n, (a.size, n)
    return a, a.ctypes.data


def pc_bounds(points, out):
    """points fp32 [n, 3], out int32 / uint32 storage [8], both on the device (include/bodyslam_hip.h)"""
    _pts(points)
    assert out.numel() == 8 and out.element_size() == 4 and out.is_cuda and out.is_contiguous()
    check(load_library().bs_pc_bounds(p(points), points.shape[0], p(out), stream_ptr()), "bs_pc_bounds")


def pc_grid_count(points, lo, hi, cell_size, dims, counts):
    _pts(points)
    _i32(counts)
    (lo_, lo_p), (hi_, hi_p), (d_, d_p) = _host(lo, "float32", 3), _host(hi, "float32", 3), _host(dims, "int32", 3)
    assert counts.numel() >= int(d_[0]) * int(d_[1]) * int(d_[2])
    check(load_library().bs_pc_grid_count(p(points), points.shape[0], lo_p, hi_p, float(cell_size), d_p, p(counts), stream_ptr()), "bs_pc_grid_count")


def pc_grid_scatter(points, lo, hi, cell_size, dims, cursor, records, n_records):
    """cursor int32 [cells] (a copy of the exclusive scan; advanced by the call), records fp32 [>= n_records, 4]"""
    _pts(points)
    _i32(cursor)
    assert records.dtype == torch.float32 and records.is_cuda and records.is_contiguous() and records.dim() == 2 and records.shape[1] == 4
    (lo_, lo_p), (hi_, hi_p), (d_, d_p) = _host(lo, "float32", 3), _host(hi, "float32", 3), _host(dims, "int32", 3)
    assert cursor.numel() >= int(d_[0]) * int(d_[1]) * int(d_[2]) and 0 <= n_records <= records.shape[0]
    check(load_library().bs_pc_grid_scatter(p(points), points.shape[0], lo_p, hi_p, float(cell_size), d_p, p(cursor), int(n_records), p(records),
                                            stream_ptr()), "bs_pc_grid_scatter")


def pc_query_grid(records, n_records, cell_start, lo, hi, cell_size, dims, source, max_distance, shell_cap, dist, index, fallback_list, fallback_count):
    """records fp32 [>= max(n_records, 1), 4] (a tensor of no elements has no address to hand over)"""
    _pts(source)
    _i32(cell_start, index, fallback_list, fallback_count)
    m = source.shape[0]
    (lo_, lo_p), (hi_, hi_p), (d_, d_p) = _host(lo, "float32", 3), _host(hi, "float32", 3), _host(dims, "int32", 3)
    assert records.dtype == torch.float32 and records.is_cuda and records.is_contiguous() and records.dim() == 2 and records.shape[1] == 4
    assert cell_start.numel() == int(d_[0]) * int(d_[1]) * int(d_[2]) + 1 and 0 <= n_records <= records.shape[0]
    assert dist.dtype == torch.float32 and dist.is_cuda and dist.is_contiguous() and dist.numel() == m and index.numel() == m
    assert fallback_list.numel() >= m and fallback_count.numel() >= 1
    check(load_library().bs_pc_query_grid(p(records), p(cell_start), int(n_records), lo_p, hi_p, float(cell_size), d_p, p(source), m,
                                          float(max_distance), int(shell_cap), p(dist), p(index), p(fallback_list), p(fallback_count), stream_ptr()),
          "bs_pc_query_grid")


def pc_query_brute(records, n_records, source, fallback_list, m, max_distance, keys, dist, index):
    """fallback_list: int32 device tensor of m source indices, or None for all m = source.shape[0] sources; keys: int64 [>= m] scratch"""
    _pts(source)
    _i32(index)
    assert records.dtype == torch.float32 and records.is_cuda and records.is_contiguous() and records.dim() == 2 and records.shape[1] == 4
    assert dist.dtype == torch.float32 and dist.is_cuda and dist.is_contiguous() and dist.numel() == source.shape[0] and index.numel() == source.shape[0]
    assert keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous() and keys.numel() >= m and 0 <= n_records <= records.shape[0]
    if fallback_list is None:
        assert m == source.shape[0]
    else:
        _i32(fallback_list)
        assert 1 <= m <= fallback_list.numel()
    check(load_library().bs_pc_query_brute(p(records), int(n_records), p(source), p(fallback_list), int(m), float(max_distance), p(keys), p(dist),
                                           p(index), stream_ptr()), "bs_pc_query_brute")


def pc_transform(source, affine, out):
    """source fp32 / fp64 [n, 3], affine: 12 host doubles (rows of [A | t]), out fp32 [n, 3]"""
    _pts(out)
    assert source.dtype in (torch.float32, torch.float64) and source.is_cuda and source.is_contiguous() and tuple(source.shape) == tuple(out.shape)
    a_, a_p = _host(affine, "float64", 12)
    check(load_library().bs_pc_transform(p(source), F32 if source.dtype == torch.float32 else F64, source.shape[0], a_p, p(out), stream_ptr()),
          "bs_pc_transform")


def pc_stats(dist, thresholds, workspace, out):
    """dist fp32 [n] (device); thresholds: up to PC_MAX_THRESHOLDS host floats; workspace: uint8 device tensor of PC_STATS_WORKSPACE_BYTES;
    out fp64 [PC_STATS_FIELDS] (device)"""
    assert dist.dtype == torch.float32 and dist.is_cuda and dist.is_contiguous() and dist.dim() == 1
    assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and out.numel() == PC_STATS_FIELDS
    n_tau = len(thresholds)
    t_, t_p = _host(thresholds, "float32", n_tau)
    check(load_library().bs_pc_stats(p(dist), dist.numel(), t_p if n_tau else None, n_tau, p(workspace), workspace.numel() * workspace.element_size(),
                                     p(out), stream_ptr()), "bs_pc_stats")


PC_KNN_MAX = 32
PC_ORIENT_AXIS, PC_ORIENT_DIRECTION, PC_ORIENT_CAMERA = 0, 1, 2


def pc_query_knn(records, n_records, cell_start, lo, hi, cell_size, dims, source, k, radius, index, d2, count):
    """the index as for pc_query_grid; source fp32 [m, 3]; radius: a positive float, math.inf = none; index int32 [m, k], d2 fp32 [m, k],
    count int32 [m]: all on the device (include/bodyslam_hip.h)"""
    _pts(source)
    _i32(cell_start, index, count)
    m, k = source.shape[0], int(k)
    (lo_, lo_p), (hi_, hi_p), (d_, d_p) = _host(lo, "float32", 3), _host(hi, "float32", 3), _host(dims, "int32", 3)
    assert records.dtype == torch.float32 and records.is_cuda and records.is_contiguous() and records.dim() == 2 and records.shape[1] == 4
    assert cell_start.numel() == int(d_[0]) * int(d_[1]) * int(d_[2]) + 1 and 0 <= n_records <= records.shape[0]
    assert d2.dtype == torch.float32 and d2.is_cuda and d2.is_contiguous() and d2.numel() == m * k and index.numel() == m * k and count.numel() == m
    check(load_library().bs_pc_query_knn(p(records), p(cell_start), int(n_records), lo_p, hi_p, float(cell_size), d_p, p(source), m, k, float(radius),
                                         p(index), p(d2), p(count), stream_ptr()), "bs_pc_query_knn")


def pc_normals(points, index, count, k, orientation, vector, normals, eigenvalues=None):
    """points fp32 [n, 3], index int32 [n, k] and count int32 [n] (the cloud's query on itself), normals fp32 [n, 3], eigenvalues fp64 [n, 3]
    or None: all on the device; vector: 3 host doubles, or None with PC_ORIENT_AXIS"""
    _pts(points, normals)
    _i32(index, count)
    n, k = points.shape[0], int(k)
    assert tuple(normals.shape) == tuple(points.shape) and index.numel() == n * k and count.numel() == n
    if eigenvalues is not None:
        _f64(eigenvalues)
        assert eigenvalues.numel() == 3 * n
    v_, v_p = (None, None) if vector is None else _host(vector, "float64", 3)
    check(load_library().bs_pc_normals(p(points), n, p(index), p(count), k, int(orientation), v_p, p(normals), p(eigenvalues), stream_ptr()),
          "bs_pc_normals")


def pc_knn_mean_distance(d2, count, k, avg):
    """d2 fp32 [m, k], count int32 [m], avg fp32 [m]: all on the device"""
    _i32(count)
    m, k = count.numel(), int(k)
    for t in (d2, avg):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    assert d2.numel() == m * k and avg.numel() == m
    check(load_library().bs_pc_knn_mean_distance(p(d2), p(count), m, k, p(avg), stream_ptr()), "bs_pc_knn_mean_distance")


PC_RADIUS_OVERRUN = 1


def _pc_index(index):
    """index: (records, n_records, cell_start, lo, hi, cell_size, dims) as for pc_query_knn -> (the leading arguments of a bs_pc_radius_* /
    bs_pc_dbscan_* call, the host arrays that must stay alive over it)"""
    records, n_records, cell_start, lo, hi, cell_size, dims = index
    _i32(cell_start)
    (lo_, lo_p), (hi_, hi_p), (d_, d_p) = _host(lo, "float32", 3), _host(hi, "float32", 3), _host(dims, "int32", 3)
    assert records.dtype == torch.float32 and records.is_cuda and records.is_contiguous() and records.dim() == 2 and records.shape[1] == 4
    assert cell_start.numel() == int(d_[0]) * int(d_[1]) * int(d_[2]) + 1 and 0 <= n_records <= records.shape[0]
    return (p(records), p(cell_start), int(n_records), lo_p, hi_p, float(cell_size), d_p), (lo_, hi_, d_)


def pc_radius_count(index, source, radius, count):
    """index: see _pc_index; source fp32 [m, 3], count int32 [m]: on the device (include/bodyslam_hip.h)"""
    _pts(source)
    _i32(count)
    assert count.numel() == source.shape[0]
    head, alive = _pc_index(index)
    check(load_library().bs_pc_radius_count(*head, p(source), source.shape[0], float(radius), p(count), stream_ptr()), "bs_pc_radius_count")


def pc_radius_fill(index, source, radius, row_start, total, keys, status):
    """row_start int64 [m + 1] (the exclusive scan of the counts, total = its last entry), keys int64 [total], status int32 [1] (zeroed)"""
    _pts(source)
    _i64(row_start, keys)
    _i32(status)
    assert row_start.numel() == source.shape[0] + 1 and keys.numel() == total >= 1 and status.numel() >= 1
    head, alive = _pc_index(index)
    check(load_library().bs_pc_radius_fill(*head, p(source), source.shape[0], float(radius), p(row_start), int(total), p(keys), p(status),
                                           stream_ptr()), "bs_pc_radius_fill")


def pc_radius_sort(keys, row_start, keys_out):
    _i64(keys, row_start, keys_out)
    assert keys.numel() == keys_out.numel() >= 1 and row_start.numel() >= 2 and keys.data_ptr() != keys_out.data_ptr()
    check(load_library().bs_pc_radius_sort(p(keys), p(row_start), row_start.numel() - 1, keys.numel(), p(keys_out), stream_ptr()),
          "bs_pc_radius_sort")


def pc_radius_unpack(keys, index, d2):
    _i64(keys)
    _i32(index)
    assert d2.dtype == torch.float32 and d2.is_cuda and d2.is_contiguous() and keys.numel() == index.numel() == d2.numel() >= 1
    check(load_library().bs_pc_radius_unpack(p(keys), keys.numel(), p(index), p(d2), stream_ptr()), "bs_pc_radius_unpack")


def pc_dbscan_hook(index, points, eps, count, min_points, parent, changed):
    """points fp32 [n, 3] (the cloud the index was built over), count int32 [n] (pc_radius_count of the cloud on itself), parent int32 [n],
    changed int32 [1]"""
    _pts(points)
    _i32(count, parent, changed)
    n = points.shape[0]
    assert count.numel() == n and parent.numel() == n and changed.numel() >= 1
    head, alive = _pc_index(index)
    check(load_library().bs_pc_dbscan_hook(*head, p(points), n, float(eps), p(count), int(min_points), p(parent), p(changed), stream_ptr()),
          "bs_pc_dbscan_hook")


def pc_dbscan_compress(parent):
    _i32(parent)
    check(load_library().bs_pc_dbscan_compress(p(parent), parent.numel(), stream_ptr()), "bs_pc_dbscan_compress")


def pc_dbscan_roots(parent, count, min_points, is_root):
    _i32(parent, count, is_root)
    assert parent.numel() == count.numel() == is_root.numel()
    check(load_library().bs_pc_dbscan_roots(p(parent), p(count), int(min_points), parent.numel(), p(is_root), stream_ptr()), "bs_pc_dbscan_roots")


def pc_dbscan_labels(index, points, eps, count, min_points, parent, rank, n_clusters, labels):
    _pts(points)
    _i32(count, parent, rank, labels)
    n = points.shape[0]
    assert count.numel() == n and parent.numel() == n and rank.numel() == n and labels.numel() == n and 0 <= n_clusters <= n
    head, alive = _pc_index(index)
    check(load_library().bs_pc_dbscan_labels(*head, p(points), n, float(eps), p(count), int(min_points), p(parent), p(rank), int(n_clusters),
                                             p(labels), stream_ptr()), "bs_pc_dbscan_labels")


ORIENT_MAX_ITEMS, ORIENT_NO_KEY = 1 << 30, -1        # (union_parity.h; the 64-bit ~0 as the int64 a torch comparison takes)


def _u8(t, n):
    assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.numel() == n, "uint8 contiguous device tensor"


def pc_orient_edges(points, normals, index, count, keys, valid):
    """points, normals fp32 [n, 3]; index int32 [n, k], count int32 [n] (pc_query_knn of the cloud on itself); keys int64 [n k], valid int32 [n]"""
    _pts(points, normals)
    _i32(index, count, valid)
    _i64(keys)
    n, k = index.shape
    assert points.shape[0] == n and normals.shape[0] == n and count.numel() == n and valid.numel() == n and keys.numel() == n * k
    check(load_library().bs_pc_orient_edges(p(points), p(normals), n, p(index), p(count), k, p(keys), p(valid), stream_ptr()), "bs_pc_orient_edges")


def pc_orient_clear(best, best_hi=None):
    _i64(best)
    if best_hi is not None:
        _i32(best_hi)
        assert best_hi.numel() == best.numel()
    check(load_library().bs_pc_orient_clear(p(best), p(best_hi), best.numel(), stream_ptr()), "bs_pc_orient_clear")


def pc_orient_select(keys, index, word, best, crossing):
    """word int32 [n] (the bits of parent << 1 | parity, below 2^31), best int64 [n] cleared, crossing int32 [1] zeroed"""
    _i64(keys, best)
    _i32(index, word, crossing)
    n, k = index.shape
    assert keys.numel() == n * k and word.numel() == n and best.numel() == n and crossing.numel() >= 1
    check(load_library().bs_pc_orient_select(p(keys), p(index), p(word), n, k, p(best), p(crossing), stream_ptr()), "bs_pc_orient_select")


def pc_orient_select_hi(keys, index, word, best, best_hi):
    _i64(keys, best)
    _i32(index, word, best_hi)
    n, k = index.shape
    assert keys.numel() == n * k and word.numel() == n and best.numel() == n and best_hi.numel() == n
    check(load_library().bs_pc_orient_select_hi(p(keys), p(index), p(word), n, k, p(best), p(best_hi), stream_ptr()), "bs_pc_orient_select_hi")


def pc_orient_hook(normals, word, best, best_hi):
    _pts(normals)
    _i32(word, best_hi)
    _i64(best)
    n = normals.shape[0]
    assert word.numel() == n and best.numel() == n and best_hi.numel() == n
    check(load_library().bs_pc_orient_hook(p(normals), p(word), n, p(best), p(best_hi), stream_ptr()), "bs_pc_orient_hook")


def pc_orient_compress(word):
    _i32(word)
    check(load_library().bs_pc_orient_compress(p(word), word.numel(), stream_ptr()), "bs_pc_orient_compress")


def pc_orient_seed(points, valid, word, seed):
    """seed int64 [n], cleared by pc_orient_clear"""
    _pts(points)
    _i32(valid, word)
    _i64(seed)
    n = points.shape[0]
    assert valid.numel() == n and word.numel() == n and seed.numel() == n
    check(load_library().bs_pc_orient_seed(p(points), p(valid), p(word), n, p(seed), stream_ptr()), "bs_pc_orient_seed")


def pc_orient_flip(normals, valid, word, seed, direction, out, flipped):
    """direction: three floats; out fp32 [n, 3] (not `normals`), flipped uint8 [n]"""
    _pts(normals, out)
    _i32(valid, word)
    _i64(seed)
    n = normals.shape[0]
    _u8(flipped, n)
    assert out.shape[0] == n and valid.numel() == n and word.numel() == n and seed.numel() == n and out.data_ptr() != normals.data_ptr()
    dx, dy, dz = (float(v) for v in direction)
    check(load_library().bs_pc_orient_flip(p(normals), p(valid), p(word), n, p(seed), dx, dy, dz, p(out), p(flipped), stream_ptr()),
          "bs_pc_orient_flip")


PC_VOXEL_AXIS_BITS, PC_VOXEL_EMPTY_KEY, PC_VOXEL_NO_POINT = 21, -1, 0x7fffffff           # (the empty key as the int64 a torch fill_ takes)
PC_VOXEL_TABLE_FULL, PC_VOXEL_OUT_OF_RANGE, PC_VOXEL_BAD_ATTRIBUTE = 1, 2, 4


def _i64(*ts):
    for t in ts:
        assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous(), "int64 contiguous device tensors"


def _voxel_attrs(points, *attrs):
    for a in attrs:
        if a is not None:
            _pts(a)
            assert tuple(a.shape) == tuple(points.shape)


def pc_voxel_assign(points, origin, voxel_size, keys, first, slot_of_point, status):
    """points fp32 [n, 3]; origin: 3 host doubles; keys int64 [slots] filled with PC_VOXEL_EMPTY_KEY, first int32 [slots] filled with
    PC_VOXEL_NO_POINT (slots: a power of two above n), slot_of_point int32 [n], status int32 [1] zeroed: all on the device"""
    _pts(points)
    _i64(keys)
    _i32(first, slot_of_point, status)
    n, slots = points.shape[0], keys.numel()
    assert first.numel() == slots and slot_of_point.numel() == n and status.numel() >= 1
    o_, o_p = _host(origin, "float64", 3)
    check(load_library().bs_pc_voxel_assign(p(points), n, o_p, float(voxel_size), p(keys), p(first), slots, p(slot_of_point), p(status), stream_ptr()),
          "bs_pc_voxel_assign")


def pc_voxel_flags(slot_of_point, first, leader, is_first):
    """slot_of_point, leader, is_first int32 [n], first int32 [slots]: all on the device"""
    _i32(slot_of_point, first, leader, is_first)
    n = slot_of_point.numel()
    assert leader.numel() == n and is_first.numel() == n
    check(load_library().bs_pc_voxel_flags(p(slot_of_point), p(first), first.numel(), n, p(leader), p(is_first), stream_ptr()), "bs_pc_voxel_flags")


def pc_voxel_accumulate(points, colors, normals, origin, shift, leader, rank, sums, counts, first_index, row_of_point, status):
    """points and, or None, colors / normals fp32 [n, 3]; leader, rank (the inclusive scan of is_first), row_of_point int32 [n]; sums int64
    [m, 3 + 3 per attribute] and counts int32 [m], zeroed; first_index int32 [m]; status int32 [1]: all on the device"""
    _pts(points)
    _voxel_attrs(points, colors, normals)
    _i64(sums)
    _i32(leader, rank, counts, first_index, row_of_point, status)
    n, m = points.shape[0], counts.numel()
    terms = 3 + 3 * (colors is not None) + 3 * (normals is not None)
    assert leader.numel() == n and rank.numel() == n and row_of_point.numel() == n and first_index.numel() == m and sums.numel() == m * terms
    o_, o_p = _host(origin, "float64", 3)
    check(load_library().bs_pc_voxel_accumulate(p(points), p(colors), p(normals), n, o_p, int(shift), p(leader), p(rank), m, p(sums), p(counts),
                                                p(first_index), p(row_of_point), p(status), stream_ptr()), "bs_pc_voxel_accumulate")


def pc_voxel_finish(points, colors, normals, sums, counts, first_index, origin, shift, unit_normals, out_points, out_colors, out_normals):
    """the inputs of pc_voxel_accumulate after it; out_points and, with their inputs, out_colors / out_normals fp32 [m, 3] (device)"""
    _pts(points, out_points)
    _voxel_attrs(points, colors, normals)
    _voxel_attrs(out_points, out_colors, out_normals)
    _i64(sums)
    _i32(counts, first_index)
    n, m = points.shape[0], counts.numel()
    terms = 3 + 3 * (colors is not None) + 3 * (normals is not None)
    assert (colors is None) == (out_colors is None) and (normals is None) == (out_normals is None)
    assert out_points.shape[0] == m and first_index.numel() == m and sums.numel() == m * terms
    o_, o_p = _host(origin, "float64", 3)
    check(load_library().bs_pc_voxel_finish(p(points), p(colors), p(normals), n, p(sums), p(counts), p(first_index), m, o_p, int(shift),
                                            int(bool(unit_normals)), p(out_points), p(out_colors), p(out_normals), stream_ptr()), "bs_pc_voxel_finish")


ICP_POINT_TO_POINT, ICP_POINT_TO_PLANE = 0, 1
ICP_ITERATE, ICP_EVALUATE = 0, 1
ICP_RUNNING, ICP_CONVERGED, ICP_MAX_ITERATION, ICP_DEGENERATE = 0, 1, 2, 3
ICP_PARTIAL_FIELDS, ICP_STATE_FIELDS, ICP_LOG_FIELDS, ICP_MAX_ITERATIONS, ICP_BLOCK = 32, 64, 4, 65536, 256


def icp_step(records, n_records, cell_start, lo, hi, cell_size, dims, target, normals, source, max_distance, estimation, mode, state, partial):
    """records / cell_start / lo / hi / cell_size / dims: the index as for pc_query_grid; target fp32 [n, 3] (the points the index was built
    from), normals fp32 [n, 3] or None, source fp32 / fp64 [m, 3], state fp64 [ICP_STATE_FIELDS + ICP_LOG_FIELDS * max_iteration], partial
    fp64 [ceil(m / ICP_BLOCK), ICP_PARTIAL_FIELDS]: all on the device (include/bodyslam_hip.h)"""
    _pts(target)
    _i32(cell_start)
    _f64(state, partial)
    m = source.shape[0]
    assert source.dtype in (torch.float32, torch.float64) and source.is_cuda and source.is_contiguous() and source.dim() == 2 and source.shape[1] == 3
    if normals is not None:
        _pts(normals)
        assert tuple(normals.shape) == tuple(target.shape)
    (lo_, lo_p), (hi_, hi_p), (d_, d_p) = _host(lo, "float32", 3), _host(hi, "float32", 3), _host(dims, "int32", 3)
    assert records.dtype == torch.float32 and records.is_cuda and records.is_contiguous() and records.dim() == 2 and records.shape[1] == 4
    assert cell_start.numel() == int(d_[0]) * int(d_[1]) * int(d_[2]) + 1 and 0 <= n_records <= min(records.shape[0], target.shape[0])
    assert state.numel() >= ICP_STATE_FIELDS + ICP_LOG_FIELDS and partial.numel() >= -(-m // ICP_BLOCK) * ICP_PARTIAL_FIELDS
    check(load_library().bs_icp_step(p(records), p(cell_start), int(n_records), lo_p, hi_p, float(cell_size), d_p, p(target), p(normals),
                                     target.shape[0], p(source), F32 if source.dtype == torch.float32 else F64, m, float(max_distance),
                                     int(estimation), int(mode), p(state), p(partial), stream_ptr()), "bs_icp_step")


def icp_finish(partial, m, lo, hi, estimation, mode, max_iteration, relative_fitness, relative_rmse, state):
    _f64(state, partial)
    (lo_, lo_p), (hi_, hi_p) = _host(lo, "float32", 3), _host(hi, "float32", 3)
    assert partial.numel() >= -(-m // ICP_BLOCK) * ICP_PARTIAL_FIELDS and state.numel() >= ICP_STATE_FIELDS + ICP_LOG_FIELDS * int(max_iteration)
    check(load_library().bs_icp_finish(p(partial), int(m), lo_p, hi_p, int(estimation), int(mode), int(max_iteration), float(relative_fitness),
                                       float(relative_rmse), p(state), stream_ptr()), "bs_icp_finish")


# ---- global registration (csrc/global_registration.hip) ---------------------------------------------------------------------------------
FPFH_DIM, FPFH_ROW, GR_STATE_FIELDS, GR_PARTIAL_FIELDS, GR_BLOCK = 33, 36, 16, 17, 256


def _lists(n, row_start, index, d2, first):
    _i64(row_start)
    _i32(index)
    m = row_start.numel() - 1
    assert d2.dtype == torch.float32 and d2.is_cuda and d2.is_contiguous() and d2.numel() == index.numel()
    assert m >= 1 and 0 <= first and first + m <= n
    return m


def fpfh_spfh(table, row_start, index, d2, first, spfh):
    """table fp32 [n, 8] = (x, y, z, ., nx, ny, nz, .); row_start int64 [m + 1], index int32 [total], d2 fp32 [total]: the sorted radius lists of
    the points first .. first + m - 1; spfh int32 [n, FPFH_ROW]: on the device (include/bodyslam_hip.h)"""
    n = table.shape[0]
    _f32(table, n, 8)
    assert spfh.dtype == torch.int32 and spfh.is_cuda and spfh.is_contiguous() and tuple(spfh.shape) == (n, FPFH_ROW)
    m = _lists(n, row_start, index, d2, first)
    check(load_library().bs_fpfh_spfh(p(table), n, p(row_start), p(index), p(d2), m, int(first), index.numel(), p(spfh), stream_ptr()), "bs_fpfh_spfh")


def fpfh_features(spfh, row_start, index, d2, first, features):
    """spfh int32 [n, FPFH_ROW] (complete: every neighbour's row is read), the lists as for fpfh_spfh, features fp32 [n, FPFH_DIM]"""
    n = spfh.shape[0]
    assert spfh.dtype == torch.int32 and spfh.is_cuda and spfh.is_contiguous() and tuple(spfh.shape) == (n, FPFH_ROW)
    _f32(features, n, FPFH_DIM)
    m = _lists(n, row_start, index, d2, first)
    check(load_library().bs_fpfh_features(p(spfh), n, p(row_start), p(index), p(d2), m, int(first), index.numel(), p(features), stream_ptr()),
          "bs_fpfh_features")


def feature_match(source, target, splits, best):
    """source fp32 [m, FPFH_DIM], target fp32 [n, FPFH_DIM], best int64 [m] filled with -1 (all bits set)"""
    m, n = source.shape[0], target.shape[0]
    _f32(source, m, FPFH_DIM)
    _f32(target, n, FPFH_DIM)
    _i64(best)
    assert best.numel() == m
    check(load_library().bs_feature_match(p(source), m, p(target), n, int(splits), p(best), stream_ptr()), "bs_feature_match")


def _corr(corr):
    _f64(corr)
    assert corr.dim() == 2 and corr.shape[1] == 6
    return corr.shape[0]


def gr_hypotheses(corr, seed, h0, count, edge_length_threshold, tau, fits, valid):
    c = _corr(corr)
    _f64(fits)
    _i32(valid)
    assert fits.numel() >= 12 * count and valid.numel() >= count
    check(load_library().bs_gr_hypotheses(p(corr), c, int(seed), int(h0), int(count), float(edge_length_threshold), float(tau), p(fits), p(valid),
                                          stream_ptr()), "bs_gr_hypotheses")


def gr_score(corr, fits, valid_list, count, splits, tau, score):
    c = _corr(corr)
    _f64(fits)
    _i32(valid_list, score)
    assert fits.numel() >= 12 * count and score.numel() >= count and 1 <= valid_list.numel() <= count
    check(load_library().bs_gr_score(p(corr), c, p(fits), p(valid_list), valid_list.numel(), int(count), int(splits), float(tau), p(score),
                                     stream_ptr()), "bs_gr_score")


def gr_winner(score, count, h0, best):
    _i32(score)
    _i64(best)
    assert score.numel() >= count and best.numel() == 1
    check(load_library().bs_gr_winner(p(score), int(count), int(h0), p(best), stream_ptr()), "bs_gr_winner")


def gr_winner_fit(corr, seed, h, edge_length_threshold, tau, state):
    c = _corr(corr)
    _f64(state)
    assert state.numel() >= GR_STATE_FIELDS
    check(load_library().bs_gr_winner_fit(p(corr), c, int(seed), int(h), float(edge_length_threshold), float(tau), p(state), stream_ptr()),
          "bs_gr_winner_fit")


def gr_refit_step(corr, state, tau, mask, partial):
    c = _corr(corr)
    _f64(state, partial)
    _i32(mask)
    assert mask.numel() == c and partial.numel() >= -(-c // GR_BLOCK) * GR_PARTIAL_FIELDS and state.numel() >= GR_STATE_FIELDS
    check(load_library().bs_gr_refit_step(p(corr), c, p(state), float(tau), p(mask), p(partial), stream_ptr()), "bs_gr_refit_step")


def gr_refit_finish(partial, c, final_round, state):
    _f64(state, partial)
    assert partial.numel() >= -(-c // GR_BLOCK) * GR_PARTIAL_FIELDS and state.numel() >= GR_STATE_FIELDS
    check(load_library().bs_gr_refit_finish(p(partial), int(c), 1 if final_round else 0, p(state), stream_ptr()), "bs_gr_refit_finish")


# ---- triangle-mesh scene (csrc/mesh_scene.hip) ------------------------------------------------------------------------------------------
MESH_MAX_TRIANGLES, MESH_MAX_SAMPLED_TRIANGLES = 1 << 29, 1 << 22


def _f32(t, *shape):
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape, (t.dtype, tuple(t.shape), shape)


def _mesh_records(records, n_triangles):
    assert records.dtype == torch.float32 and records.is_cuda and records.is_contiguous() and records.dim() == 3
    assert tuple(records.shape[1:]) == (3, 4) and 0 <= n_triangles <= records.shape[0]


def mesh_records(vertices, triangles, records, kept):
    """vertices fp32 [V, 3], triangles int32 [T, 3], records fp32 [T, 3, 4], kept int32 [1]: all on the device"""
    _pts(vertices)
    _i32(triangles, kept)
    T = triangles.shape[0]
    assert triangles.dim() == 2 and triangles.shape[1] == 3 and kept.numel() >= 1
    _mesh_records(records, T)
    check(load_library().bs_mesh_records(p(vertices), vertices.shape[0], p(triangles), T, p(records), p(kept), stream_ptr()), "bs_mesh_records")


def _mesh_query(records, n_triangles, rows, width, fallback_list, m, keys, geom_start, geometry_ids, primitive_ids, uvs):
    _mesh_records(records, n_triangles)
    n = rows.shape[0]
    _f32(rows, n, width)
    _f32(uvs, n, 2)
    _i32(geom_start, geometry_ids, primitive_ids)
    assert geometry_ids.numel() == n and primitive_ids.numel() == n and geom_start.numel() >= 1
    assert keys is None or (keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous() and keys.numel() >= m)
    if fallback_list is None:
        assert m == n
    else:
        _i32(fallback_list)
        assert 1 <= m <= fallback_list.numel()


def mesh_cast_brute(records, n_triangles, rays, fallback_list, m, keys, geom_start, t_hit, geometry_ids, primitive_ids, uvs, normals):
    """rays fp32 [n, 6]; fallback_list: int32 device tensor of m ray rows, or None for all m = n rays; keys int64 [>= m] scratch; geom_start
    int32 [n_geom + 1]; the outputs fp32 [n], int32 [n], int32 [n], fp32 [n, 2], fp32 [n, 3]"""
    _mesh_query(records, n_triangles, rays, 6, fallback_list, m, keys, geom_start, geometry_ids, primitive_ids, uvs)
    n = rays.shape[0]
    _f32(t_hit, n)
    _f32(normals, n, 3)
    check(load_library().bs_mesh_cast_brute(p(records), int(n_triangles), p(rays), n, p(fallback_list), int(m), p(keys), p(geom_start),
                                            geom_start.numel() - 1, p(t_hit), p(geometry_ids), p(primitive_ids), p(uvs), p(normals), stream_ptr()),
          "bs_mesh_cast_brute")


def mesh_closest_brute(records, n_triangles, query, fallback_list, m, max_distance, keys, geom_start, points, distance, geometry_ids, primitive_ids,
                       uvs):
    """query fp32 [n, 3]; the outputs fp32 [n, 3], fp32 [n], int32 [n], int32 [n], fp32 [n, 2]; the rest as mesh_cast_brute"""
    _mesh_query(records, n_triangles, query, 3, fallback_list, m, keys, geom_start, geometry_ids, primitive_ids, uvs)
    n = query.shape[0]
    _f32(points, n, 3)
    _f32(distance, n)
    check(load_library().bs_mesh_closest_brute(p(records), int(n_triangles), p(query), n, p(fallback_list), int(m), float(max_distance), p(keys),
                                               p(geom_start), geom_start.numel() - 1, p(points), p(distance), p(geometry_ids), p(primitive_ids),
                                               p(uvs), stream_ptr()), "bs_mesh_closest_brute")


def _mesh_grid(grid):
    """grid: (lo, hi, cell_size, dims, pad) -> the host arrays (kept alive by the caller) and their addresses"""
    lo, hi, h, dims, pad = grid
    return _host(lo, "float32", 3), _host(hi, "float32", 3), float(h), _host(dims, "int32", 3), float(pad)


def mesh_grid_count(records, n_triangles, grid, counts):
    """counts int32 [cells], zeroed: += 1 for every (kept triangle, cell its padded box overlaps)"""
    _mesh_records(records, n_triangles)
    _i32(counts)
    (lo_, lo_p), (hi_, hi_p), h, (d_, d_p), pad = _mesh_grid(grid)
    assert counts.numel() >= int(d_[0]) * int(d_[1]) * int(d_[2])
    check(load_library().bs_mesh_grid_count(p(records), int(n_triangles), lo_p, hi_p, h, d_p, pad, p(counts), stream_ptr()), "bs_mesh_grid_count")


def mesh_grid_scatter(records, n_triangles, grid, cursor, refs):
    """cursor int32 [cells]: a copy of the exclusive scan (advanced by the call); refs int32 [n_refs]"""
    _mesh_records(records, n_triangles)
    _i32(cursor, refs)
    (lo_, lo_p), (hi_, hi_p), h, (d_, d_p), pad = _mesh_grid(grid)
    assert cursor.numel() >= int(d_[0]) * int(d_[1]) * int(d_[2])
    check(load_library().bs_mesh_grid_scatter(p(records), int(n_triangles), lo_p, hi_p, h, d_p, pad, p(cursor), refs.numel(), p(refs), stream_ptr()),
          "bs_mesh_grid_scatter")


def _mesh_index(refs, cell_start, d_, fallback_list, fallback_count, n):
    _i32(refs, cell_start, fallback_list, fallback_count)
    assert cell_start.numel() == int(d_[0]) * int(d_[1]) * int(d_[2]) + 1 and fallback_list.numel() >= n and fallback_count.numel() >= 1


def mesh_cast_grid(records, n_triangles, refs, cell_start, grid, origin_limit, rays, geom_start, t_hit, geometry_ids, primitive_ids, uvs, normals,
                   fallback_list, fallback_count):
    """the outputs of mesh_cast_brute for every ray the walk finishes; the others on fallback_list int32 [>= n] (fallback_count int32 [1])"""
    n = rays.shape[0]
    _mesh_query(records, n_triangles, rays, 6, None, n, None, geom_start, geometry_ids, primitive_ids, uvs)
    _f32(t_hit, n)
    _f32(normals, n, 3)
    (lo_, lo_p), (hi_, hi_p), h, (d_, d_p), pad = _mesh_grid(grid)
    _mesh_index(refs, cell_start, d_, fallback_list, fallback_count, n)
    check(load_library().bs_mesh_cast_grid(p(records), int(n_triangles), p(refs), p(cell_start), lo_p, hi_p, h, d_p, pad, float(origin_limit), p(rays), n,
                                           p(geom_start), geom_start.numel() - 1, p(t_hit), p(geometry_ids), p(primitive_ids), p(uvs), p(normals),
                                           p(fallback_list), p(fallback_count), stream_ptr()), "bs_mesh_cast_grid")


def mesh_closest_grid(records, n_triangles, refs, cell_start, grid, query, max_distance, shell_cap, geom_start, points, distance, geometry_ids,
                      primitive_ids, uvs, fallback_list, fallback_count):
    """the outputs of mesh_closest_brute for every point the walk finishes; the others on fallback_list"""
    n = query.shape[0]
    _mesh_query(records, n_triangles, query, 3, None, n, None, geom_start, geometry_ids, primitive_ids, uvs)
    _f32(points, n, 3)
    _f32(distance, n)
    (lo_, lo_p), (hi_, hi_p), h, (d_, d_p), pad = _mesh_grid(grid)
    _mesh_index(refs, cell_start, d_, fallback_list, fallback_count, n)
    check(load_library().bs_mesh_closest_grid(p(records), int(n_triangles), p(refs), p(cell_start), lo_p, hi_p, h, d_p, pad, p(query), n,
                                              float(max_distance), int(shell_cap), p(geom_start), geom_start.numel() - 1, p(points), p(distance),
                                              p(geometry_ids), p(primitive_ids), p(uvs), p(fallback_list), p(fallback_count), stream_ptr()),
          "bs_mesh_closest_grid")


MESH_HITS_COUNT, MESH_HITS_ANY, MESH_HITS_FILL = 0, 1, 2


def _mesh_hits(rays, mode, out, row_start, keys):
    """the sink of a bs_mesh_hits_* call -> total.  COUNT, ANY: out int32 [n]; FILL: row_start int64 [n + 1], keys int64 [total]"""
    n = rays.shape[0]
    _f32(rays, n, 6)
    assert mode in (MESH_HITS_COUNT, MESH_HITS_ANY, MESH_HITS_FILL)
    if mode == MESH_HITS_FILL:
        _i64(row_start, keys)
        assert row_start.numel() == n + 1 and keys.numel() >= 1
        return keys.numel()
    _i32(out)
    assert out.numel() == n
    return 0


def mesh_hits_grid(records, n_triangles, refs, cell_start, grid, origin_limit, rays, mode, tnear, tfar, out, row_start, keys, fallback_list,
                   fallback_count):
    """every hit of the rays fp32 [n, 6] the walk covers into the sink of `mode` (_mesh_hits); the others on fallback_list int32 [>= n]"""
    _mesh_records(records, n_triangles)
    n = rays.shape[0]
    total = _mesh_hits(rays, mode, out, row_start, keys)
    (lo_, lo_p), (hi_, hi_p), h, (d_, d_p), pad = _mesh_grid(grid)
    _mesh_index(refs, cell_start, d_, fallback_list, fallback_count, n)
    check(load_library().bs_mesh_hits_grid(p(records), int(n_triangles), p(refs), p(cell_start), lo_p, hi_p, h, d_p, pad, float(origin_limit), p(rays), n,
                                           int(mode), float(tnear), float(tfar), p(out), p(row_start), total, p(keys), p(fallback_list),
                                           p(fallback_count), stream_ptr()), "bs_mesh_hits_grid")


def mesh_hits_brute(records, n_triangles, rays, fallback_list, m, mode, tnear, tfar, out, row_start, keys, cursor):
    """the rays of fallback_list (int32, m of them; None: all m = n) against every triangle into the sink of `mode`; cursor int32 [>= m]
    scratch for FILL"""
    _mesh_records(records, n_triangles)
    n = rays.shape[0]
    total = _mesh_hits(rays, mode, out, row_start, keys)
    if fallback_list is None:
        assert m == n
    else:
        _i32(fallback_list)
        assert 1 <= m <= fallback_list.numel()
    if mode == MESH_HITS_FILL:
        _i32(cursor)
        assert cursor.numel() >= m
    check(load_library().bs_mesh_hits_brute(p(records), int(n_triangles), p(rays), n, p(fallback_list), int(m), int(mode), float(tnear), float(tfar),
                                            p(out), p(row_start), total, p(keys), p(cursor), stream_ptr()), "bs_mesh_hits_brute")


def mesh_hits_unpack(records, n_triangles, rays, keys, ray_ids, geom_start, t_hit, geometry_ids, primitive_ids, uvs):
    """keys, ray_ids int64 [total] (sorted rows and the ray of each) -> t_hit fp32, geometry_ids, primitive_ids int32 [total], uvs fp32 [total, 2]"""
    _mesh_records(records, n_triangles)
    _f32(rays, rays.shape[0], 6)
    _i64(keys, ray_ids)
    total = keys.numel()
    _f32(t_hit, total)
    _f32(uvs, total, 2)
    _i32(geom_start, geometry_ids, primitive_ids)
    assert total >= 1 and ray_ids.numel() == total and geometry_ids.numel() == total and primitive_ids.numel() == total and geom_start.numel() >= 2
    check(load_library().bs_mesh_hits_unpack(p(records), int(n_triangles), p(rays), rays.shape[0], p(keys), p(ray_ids), total, p(geom_start),
                                             geom_start.numel() - 1, p(t_hit), p(geometry_ids), p(primitive_ids), p(uvs), stream_ptr()),
          "bs_mesh_hits_unpack")


def mesh_sample_weights(records, area, top, weights):
    """records fp32 [T, 3, 4]; area fp64 [T] and top int64 [1]: scratch; weights int64 [T]"""
    T = records.shape[0]
    _mesh_records(records, T)
    _i64(top, weights)
    assert area.dtype == torch.float64 and area.is_cuda and area.is_contiguous() and area.numel() == T and weights.numel() == T and top.numel() >= 1
    check(load_library().bs_mesh_sample_weights(p(records), T, p(area), p(top), p(weights), stream_ptr()), "bs_mesh_sample_weights")


def mesh_sample(records, cum, triangles, vertex_colors, seed, first, points, colors, normals, index):
    """cum int64 [T]: the inclusive scan of the weights; triangles int32 [T, 3], vertex_colors fp32 [V, 3] and colors fp32 [n, 3]: all three or
    None; points, normals fp32 [n, 3], index int32 [n]"""
    T, n = records.shape[0], points.shape[0]
    _mesh_records(records, T)
    _i64(cum)
    _i32(index)
    _f32(points, n, 3)
    _f32(normals, n, 3)
    assert cum.numel() == T and index.numel() == n and (colors is None) == (vertex_colors is None)
    n_vertices = 1
    if colors is not None:
        _pts(vertex_colors)
        _f32(colors, n, 3)
        _i32(triangles)
        assert tuple(triangles.shape) == (T, 3)
        n_vertices = vertex_colors.shape[0]
    check(load_library().bs_mesh_sample(p(records), T, p(cum), p(triangles) if colors is not None else None, p(vertex_colors), n_vertices,
                                        int(seed), int(first), n, p(points), p(colors), p(normals), p(index), stream_ptr()), "bs_mesh_sample")


# ---- mesh topology and clean-up (csrc/mesh_ops.hip) -------------------------------------------------------------------------------------
MESH_EDGE_EMPTY_KEY, MESH_EDGE_NO_HALF, MESH_EDGE_TABLE_FULL = -1, 0x7fffffff, 1            # (the empty key as the int64 a torch fill_ takes)
MESH_TRIANGLE_VALID, MESH_TRIANGLE_KEPT = 1, 2


def _tri(triangles):
    _i32(triangles)
    assert triangles.dim() == 2 and triangles.shape[1] == 3 and triangles.shape[0] >= 1
    return triangles.shape[0]


def mesh_edge_insert(triangles, n_vertices, keys, first_half, count, forward, slot_of_half, status):
    """triangles int32 [T, 3]; keys int64 [slots] filled with MESH_EDGE_EMPTY_KEY, first_half int32 [slots] filled with MESH_EDGE_NO_HALF, count
    and forward int32 [slots] zeroed (slots: a power of two), slot_of_half int32 [3 T], status int32 [2] zeroed: all on the device"""
    T = _tri(triangles)
    _i64(keys)
    _i32(first_half, count, forward, slot_of_half, status)
    slots = keys.numel()
    assert first_half.numel() == slots and count.numel() == slots and forward.numel() == slots and slot_of_half.numel() == 3 * T and status.numel() >= 2
    check(load_library().bs_mesh_edge_insert(p(triangles), T, int(n_vertices), p(keys), p(first_half), p(count), p(forward), slots, p(slot_of_half),
                                             p(status), stream_ptr()), "bs_mesh_edge_insert")


def mesh_edge_flags(slot_of_half, first_half, leader, is_first):
    """slot_of_half, leader, is_first int32 [3 T], first_half int32 [slots]: all on the device"""
    _i32(slot_of_half, first_half, leader, is_first)
    n = slot_of_half.numel()
    assert leader.numel() == n and is_first.numel() == n
    check(load_library().bs_mesh_edge_flags(p(slot_of_half), p(first_half), first_half.numel(), n, p(leader), p(is_first), stream_ptr()),
          "bs_mesh_edge_flags")


def mesh_edge_rows(triangles, slot_of_half, count, forward, leader, rank, edges, edge_count, edge_forward, edge_first_triangle, edge_of_half):
    """rank int32 [3 T]: the inclusive scan of is_first; edges int32 [E, 2], edge_count / edge_forward / edge_first_triangle int32 [E],
    edge_of_half int32 [3 T]"""
    T = _tri(triangles)
    _i32(slot_of_half, count, forward, leader, rank, edges, edge_count, edge_forward, edge_first_triangle, edge_of_half)
    E = edge_count.numel()
    assert count.numel() == forward.numel() and tuple(edges.shape) == (E, 2) and edge_forward.numel() == E and edge_first_triangle.numel() == E
    assert all(t.numel() == 3 * T for t in (slot_of_half, leader, rank, edge_of_half))
    check(load_library().bs_mesh_edge_rows(p(triangles), T, p(slot_of_half), p(count), p(forward), count.numel(), p(leader), p(rank), E, p(edges),
                                           p(edge_count), p(edge_forward), p(edge_first_triangle), p(edge_of_half), stream_ptr()), "bs_mesh_edge_rows")


def mesh_cc_hook(edge_of_half, edge_first_triangle, parent, changed):
    """edge_of_half int32 [3 T], edge_first_triangle int32 [E], parent int32 [T], changed int32 [1]"""
    _i32(edge_of_half, edge_first_triangle, parent, changed)
    T = parent.numel()
    assert edge_of_half.numel() == 3 * T and changed.numel() >= 1
    check(load_library().bs_mesh_cc_hook(p(edge_of_half), p(edge_first_triangle), T, edge_first_triangle.numel(), p(parent), p(changed), stream_ptr()),
          "bs_mesh_cc_hook")


def mesh_cc_compress(parent):
    _i32(parent)
    check(load_library().bs_mesh_cc_compress(p(parent), parent.numel(), stream_ptr()), "bs_mesh_cc_compress")


def mesh_cc_roots(parent, edge_of_half, is_root):
    _i32(parent, edge_of_half, is_root)
    T = parent.numel()
    assert edge_of_half.numel() == 3 * T and is_root.numel() == T
    check(load_library().bs_mesh_cc_roots(p(parent), p(edge_of_half), T, p(is_root), stream_ptr()), "bs_mesh_cc_roots")


def mesh_cc_clusters(parent, edge_of_half, rank, triangle_clusters, cluster_n_triangles):
    """rank int32 [T]: the inclusive scan of is_root; triangle_clusters int32 [T]; cluster_n_triangles int32 [C] zeroed"""
    _i32(parent, edge_of_half, rank, triangle_clusters, cluster_n_triangles)
    T = parent.numel()
    assert edge_of_half.numel() == 3 * T and rank.numel() == T and triangle_clusters.numel() == T
    check(load_library().bs_mesh_cc_clusters(p(parent), p(edge_of_half), p(rank), T, cluster_n_triangles.numel(), p(triangle_clusters),
                                             p(cluster_n_triangles), stream_ptr()), "bs_mesh_cc_clusters")


def _mesh_links(me, word):
    """me: mesh.MeshEdges -> the leading arguments of a bs_mesh_orient_hook / _check call"""
    _i32(me.edge_of_half, me.edge_count, me.edge_forward, me.edge_first_triangle, word)
    T, E = word.numel(), me.edge_count.numel()
    assert me.edge_of_half.numel() == 3 * T and me.edge_forward.numel() == E and me.edge_first_triangle.numel() == E
    return p(me.edge_of_half), p(me.edge_count), p(me.edge_forward), p(me.edge_first_triangle), T, E


def mesh_orient_hook(me, word, changed):
    """me: mesh.MeshEdges; word int32 [T] (the bits of parent << 1 | parity), changed int32 [1]"""
    _i32(changed)
    check(load_library().bs_mesh_orient_hook(*_mesh_links(me, word), p(word), p(changed), stream_ptr()), "bs_mesh_orient_hook")


def mesh_orient_compress(word):
    _i32(word)
    check(load_library().bs_mesh_orient_compress(p(word), word.numel(), stream_ptr()), "bs_mesh_orient_compress")


def mesh_orient_check(me, word, bad):
    """bad int32 [T] zeroed"""
    _i32(bad)
    assert bad.numel() == word.numel()
    check(load_library().bs_mesh_orient_check(*_mesh_links(me, word), p(word), p(bad), stream_ptr()), "bs_mesh_orient_check")


def mesh_orient_flip(triangles, edge_of_half, word, bad, out, flipped):
    """out int32 [T, 3] (not `triangles`), flipped uint8 [T]"""
    T = _tri(triangles)
    _i32(edge_of_half, word, bad, out)
    _u8(flipped, T)
    assert edge_of_half.numel() == 3 * T and word.numel() == T and bad.numel() == T and tuple(out.shape) == (T, 3)
    assert out.data_ptr() != triangles.data_ptr()
    check(load_library().bs_mesh_orient_flip(p(triangles), p(edge_of_half), p(word), p(bad), T, p(out), p(flipped), stream_ptr()),
          "bs_mesh_orient_flip")


def mesh_segment_sum(values, start, out):
    """values fp64 [n], start int64 [segments + 1], out fp64 [segments]"""
    _f64(values, out)
    _i64(start)
    assert start.numel() == out.numel() + 1 and out.numel() >= 1
    check(load_library().bs_mesh_segment_sum(p(values), values.numel(), p(start), out.numel(), p(out), stream_ptr()), "bs_mesh_segment_sum")


def mesh_triangle_geometry(vertices, triangles, flags=None, normals=None, cross=None, area=None):
    """vertices fp32 [V, 3], triangles int32 [T, 3]; any of flags int32 [T], normals fp32 [T, 3], cross fp64 [T, 3], area fp64 [T]"""
    _pts(vertices)
    T = _tri(triangles)
    _f64(cross, area)
    if flags is not None:
        _i32(flags)
        assert flags.numel() == T
    if normals is not None:
        _f32(normals, T, 3)
    assert (cross is None or tuple(cross.shape) == (T, 3)) and (area is None or area.numel() == T)
    check(load_library().bs_mesh_triangle_geometry(p(vertices), vertices.shape[0], p(triangles), T, p(flags), p(normals), p(cross), p(area),
                                                   stream_ptr()), "bs_mesh_triangle_geometry")


def mesh_vertex_normals(cross, corner_order, vertex_start, normals):
    """cross fp64 [T, 3], corner_order int64 [3 T], vertex_start int64 [V + 1], normals fp32 [V, 3]"""
    _f64(cross)
    _i64(corner_order, vertex_start)
    _pts(normals)
    T, V = cross.shape[0], normals.shape[0]
    assert tuple(cross.shape) == (T, 3) and corner_order.numel() == 3 * T and vertex_start.numel() == V + 1
    check(load_library().bs_mesh_vertex_normals(p(cross), T, p(corner_order), p(vertex_start), V, p(normals), stream_ptr()), "bs_mesh_vertex_normals")


def mesh_laplacian_step(src, nbr_start, nbr, lam, clamp, out):
    """src, out fp32 [V, 3] (distinct), nbr_start int64 [V + 1], nbr int32 [M]"""
    _pts(src, out)
    _i64(nbr_start)
    _i32(nbr)
    V = src.shape[0]
    assert out.shape[0] == V and nbr_start.numel() == V + 1 and src.data_ptr() != out.data_ptr()
    check(load_library().bs_mesh_laplacian_step(p(src), V, p(nbr_start), p(nbr) if nbr.numel() else None, nbr.numel(), float(lam), int(bool(clamp)),
                                                p(out), stream_ptr()), "bs_mesh_laplacian_step")


# ---- is this mesh a solid (csrc/mesh_solid.hip) -----------------------------------------------------------------------------------------
MESH_PAIRS_COUNT, MESH_PAIRS_ANY, MESH_PAIRS_FILL = 0, 1, 2


def mesh_fan_hook(triangles, edge_of_half, edge_first_triangle, parent, changed):
    """triangles int32 [T, 3], edge_of_half int32 [3 T], edge_first_triangle int32 [E], parent int32 [3 T] over the corners, changed int32 [1]"""
    T = _tri(triangles)
    _i32(edge_of_half, edge_first_triangle, parent, changed)
    assert edge_of_half.numel() == 3 * T and parent.numel() == 3 * T and changed.numel() >= 1
    check(load_library().bs_mesh_fan_hook(p(triangles), T, p(edge_of_half), p(edge_first_triangle), edge_first_triangle.numel(), p(parent), p(changed),
                                          stream_ptr()), "bs_mesh_fan_hook")


def mesh_fan_compress(parent):
    _i32(parent)
    check(load_library().bs_mesh_fan_compress(p(parent), parent.numel(), stream_ptr()), "bs_mesh_fan_compress")


def mesh_fan_count(triangles, n_vertices, edge_of_half, parent, count):
    """count int32 [V] zeroed: the corner classes at every vertex"""
    T = _tri(triangles)
    _i32(edge_of_half, parent, count)
    assert edge_of_half.numel() == 3 * T and parent.numel() == 3 * T and count.numel() == n_vertices >= 1
    check(load_library().bs_mesh_fan_count(p(triangles), T, int(n_vertices), p(edge_of_half), p(parent), p(count), stream_ptr()), "bs_mesh_fan_count")


def mesh_solid_records(vertices, triangles, records, kept):
    """vertices fp32 [V, 3], triangles int32 [T, 3], records fp32 [T, 3, 4] (the vertex rows in the fourth lanes), kept int32 [1]"""
    _pts(vertices)
    T = _tri(triangles)
    _i32(kept)
    assert kept.numel() >= 1 and vertices.shape[0] >= 1
    _mesh_records(records, T)
    check(load_library().bs_mesh_solid_records(p(vertices), vertices.shape[0], p(triangles), T, p(records), p(kept), stream_ptr()), "bs_mesh_solid_records")


def _mesh_pairs(q_records, records, mode, out, row_start, keys, any_flag):
    """the sink of a bs_mesh_pairs_* call -> (n_q, n_triangles, total)"""
    n_q, T = q_records.shape[0], records.shape[0]
    _mesh_records(q_records, n_q)
    _mesh_records(records, T)
    assert mode in (MESH_PAIRS_COUNT, MESH_PAIRS_ANY, MESH_PAIRS_FILL) and n_q >= 1 and T >= 1
    total = 0
    if mode == MESH_PAIRS_COUNT:
        _i32(out)
        assert out.numel() == n_q
    elif mode == MESH_PAIRS_ANY:
        _i32(any_flag)
        assert any_flag.numel() >= 1
    else:
        _i64(row_start, keys)
        assert row_start.numel() == n_q + 1 and keys.numel() >= 1
        total = keys.numel()
    return n_q, T, total


def mesh_pairs_grid(q_records, records, refs, cell_start, grid, self_mode, cell_cap, mode, out, row_start, keys, any_flag, fallback_list, fallback_count):
    """the intersecting pairs of the query triangles the walk covers into the sink of `mode`; the others on fallback_list int32 [>= n_q]"""
    n_q, T, total = _mesh_pairs(q_records, records, mode, out, row_start, keys, any_flag)
    (lo_, lo_p), (hi_, hi_p), h, (d_, d_p), pad = _mesh_grid(grid)
    _mesh_index(refs, cell_start, d_, fallback_list, fallback_count, n_q)
    check(load_library().bs_mesh_pairs_grid(p(q_records), n_q, p(records), T, p(refs), refs.numel(), p(cell_start), lo_p, hi_p, h, d_p, pad,
                                            int(bool(self_mode)), int(cell_cap), int(mode), p(out), p(row_start), total, p(keys), p(any_flag),
                                            p(fallback_list), p(fallback_count), stream_ptr()), "bs_mesh_pairs_grid")


def mesh_pairs_brute(q_records, fallback_list, m, records, self_mode, mode, out, row_start, keys, cursor, any_flag):
    """the query triangles of fallback_list (int32, m of them; None: all) against every triangle into the sink of `mode`; cursor int32 [>= m]
    scratch for FILL"""
    n_q, T, total = _mesh_pairs(q_records, records, mode, out, row_start, keys, any_flag)
    if fallback_list is None:
        assert m == n_q
    else:
        _i32(fallback_list)
        assert 1 <= m <= fallback_list.numel()
    if mode == MESH_PAIRS_FILL:
        _i32(cursor)
        assert cursor.numel() >= m
    check(load_library().bs_mesh_pairs_brute(p(q_records), n_q, p(fallback_list), int(m), p(records), T, int(bool(self_mode)), int(mode), p(out),
                                             p(row_start), total, p(keys), p(cursor), p(any_flag), stream_ptr()), "bs_mesh_pairs_brute")


def mesh_signed_volume(vertices, triangles, parent, vol6):
    """parent int32 [T]: bs_mesh_cc_compress' fixed point; vol6 fp64 [T]"""
    _pts(vertices)
    T = _tri(triangles)
    _i32(parent)
    _f64(vol6)
    assert parent.numel() == T and vol6.numel() == T and vertices.shape[0] >= 1
    check(load_library().bs_mesh_signed_volume(p(vertices), vertices.shape[0], p(triangles), T, p(parent), p(vol6), stream_ptr()), "bs_mesh_signed_volume")
