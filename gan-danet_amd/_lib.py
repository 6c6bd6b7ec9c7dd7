"""ctypes binding of libgandanet_hip.so (C ABI: include/gandanet.h).

The product path has NO fallback: if the shared library is missing or a call
fails, this raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libgandanet_hip.so")

PREC_FP32, PREC_BF16, PREC_X3 = 0, 1, 2   # GD_PREC_*: exact f32 MFMA / bf16 operands / split-bf16 (hi + lo, three MFMAs per product)
PAM_BWD_K64_ATOMIC, PAM_BWD_K64_PARTS, PAM_BWD_TWO_KERNEL = 0, 1, 3   # GD_PAM_BWD_* (2 is retired)
ACT_NONE, ACT_RELU, ACT_LEAKY02, ACT_SIGMOID = 0, 1, 2, 3
EVAL_F64, EVAL_SKIP_NAN = 1, 2   # GD_EVAL_*
GUARD_SQNORM, GUARD_NORM, GUARD_COEF, GUARD_OK, GUARD_APPLIED, GUARD_SKIPPED, GUARD_RECORD = range(7)   # GD_GUARD_*
GUARD_CHUNK = 65536              # GD_GUARD_CHUNK
FILTER_F32, FILTER_F64 = 0, 1    # GD_FILTER_*
EDGE_REFLECT, EDGE_INTERIOR = 0, 1   # GD_EDGE_*
FILTER_MAX_RADIUS, SAVGOL_MAX_WINDOW = 64, 33   # GD_FILTER_MAX_RADIUS, GD_SAVGOL_MAX_WINDOW
ZOOM_MIRROR, ZOOM_NEAREST = 0, 1   # GD_ZOOM_*
FREQ_MAX_BINS, FREQ_MAX_TABLE_BYTES = 33, 16 << 20   # GD_FREQ_MAX_BINS, GD_FREQ_MAX_TABLE_BYTES
ZONE_MAX, ZONE_EDGE_CHUNK = 32, 512   # GD_ZONE_MAX, GD_ZONE_EDGE_CHUNK
STL_MAX_T = 2048                 # GD_STL_MAX_T
SKILL_MAPS = ("n", "mean_p", "mean_t", "bias", "rmse", "mae", "std_p", "std_t", "cc", "nse", "kge", "crmsd")   # GD_SKILL_*: bit k of `which`
LSTSQ_MAX_P = 8                  # GD_LSTSQ_MAX_P
TREND_MAX_T = 2048               # GD_TREND_MAX_T
TREND_MAPS = ("n", "s", "var_s", "z", "p", "tau", "slope", "intercept", "slope_lo", "slope_hi")   # GD_TREND_*: plane k of `out`
TREND_SEN, TREND_CI, TREND_CONTINUITY = 1, 2, 4   # GD_TREND_SEN, GD_TREND_CI, GD_TREND_CONTINUITY
CP_MAX_T = 2048                  # GD_CP_MAX_T
CP_MAPS = ("n", "pt_k", "pt_u", "pt_index", "pt_p", "cs_q", "cs_r", "cs_index", "cs_p", "st_index", "st_mean_before", "st_mean_after",
           "st_shift", "st_rss0", "st_rss", "st_f", "tr_index", "tr_slope_before", "tr_slope_after", "tr_intercept_before",
           "tr_intercept_after", "tr_jump", "tr_rss0", "tr_rss", "tr_f")   # GD_CP_*: plane k of `out`
CP_PETTITT, CP_CUSUM, CP_STEP, CP_TREND = 1, 2, 4, 8   # GD_CP_PETTITT, GD_CP_CUSUM, GD_CP_STEP, GD_CP_TREND
LAG_MAX, LAG_MAX_T, LAG_CHUNK = 64, 2048, 32   # GD_LAG_MAX, GD_LAG_MAX_T, GD_LAG_CHUNK
LAG_PLANES = ("best_lag", "best_r", "best_n", "r0")   # GD_LAG_*: plane k of `best`
LAG_SELECT = {"abs": 0, "max": 1, "min": 2}           # GD_LAG_SELECT_*
ACF_KINDS = {"pearson": 0, "standard": 1}             # GD_ACF_*
TC_MAX_T, TC_MAX_B, TC_MAX_Q = 2048, 2048, 8   # GD_TC_MAX_T, GD_TC_MAX_B, GD_TC_MAX_Q
TC_STATS = ("err_var_x", "err_var_y", "err_var_z", "rho2_x", "rho2_y", "rho2_z", "beta_y", "beta_z")   # GD_TC_*: plane k of `stats`
TC_COVS = ("xx", "yy", "zz", "xy", "xz", "yz")   # row k of `cov`
TC_FLAGS = {"masked": 1, "few": 2, "nonpos": 4, "neg_x": 8, "neg_y": 16, "neg_z": 32, "rho2": 64}   # GD_TC_FLAG_*
SSA_MAX_M, SSA_MAX_T, SSA_MAX_RANK, SSA_MAX_ITER, SSA_MAX_SWEEPS, SSA_CHUNK = 64, 2048, 16, 200, 30, 8192   # GD_SSA_MAX_*, GD_SSA_CHUNK
SSA_METHODS = {"bk": 0, "vg": 1}   # GD_SSA_BK, GD_SSA_VG
SSA_MAPS = ("n", "n_gaps", "mean", "sd", "trace", "sweeps", "iterations", "last_change", "flags")   # GD_SSA_*: plane k of `maps`
SSA_FLAGS = {"masked": 1, "few": 2, "constant": 4, "nonfinite": 8, "gaps": 16, "sweeps": 32, "iter": 64}   # GD_SSA_FLAG_*
KM_MAX_T, KM_MAX_K, KM_CHUNK, KM_SLAB = 2048, 64, 64, 1024   # GD_KM_MAX_T, GD_KM_MAX_K, GD_KM_CHUNK, GD_KM_SLAB
ENSV_MAX_M, ENSV_F64, ENSV_FAIR = 32, 1, 2   # GD_ENSV_MAX_M, GD_ENSV_F64, GD_ENSV_FAIR
ENSV_FIELDS = ("n", "tied", "crps", "crps_gauss", "abs_e", "e2", "s2")   # GD_ENSV_*: record slot k; then cover, hist
ENSV_COVER, ENSV_HIST, ENSV_BINS, ENSV_REC = 7, 11, 33, 44   # GD_ENSV_COVER, GD_ENSV_HIST, GD_ENSV_BINS, GD_ENSV_REC
ENSV_METRIC_NAMES = ("crps", "crps_gauss", "mae", "rmse", "spread", "spread_skill")   # GD_ENSV_M_*: metric slot k
ENSV_M_COVER, ENSV_M_RELIABILITY, ENSV_M_TIED, ENSV_M_HIST, ENSV_METRICS = 6, 10, 11, 12, 45
ENSV_LEVELS = (0.5, 0.6826894921370859, 0.9, 0.95)   # the nominal levels of the four coverage counts
EOF_MAX_T, EOF_MAX_K = 256, 16   # GD_EOF_MAX_T, GD_EOF_MAX_K
EOF_CHUNK, EOF_SPLIT_MIN, EOF_SPLIT_MAX = 32, 8, 256   # GD_EOF_CHUNK, GD_EOF_SPLIT_MIN, GD_EOF_SPLIT_MAX (csrc/eof_core.h)
SPEC_MAX_H, SPEC_MAX_W, SPEC_MAX_BINS = 1024, 2048, 1024   # GD_SPEC_MAX_H, GD_SPEC_MAX_W, GD_SPEC_MAX_BINS
SPEC_DETREND = {"none": 0, "mean": 1, "plane": 2}          # GD_SPEC_DETREND_* (csrc/spectra_core.h)
DROUGHT_MAX_T, DROUGHT_MAX_PERIOD, DROUGHT_MAX_N = 2048, 366, 257   # GD_DROUGHT_MAX_T, GD_DROUGHT_MAX_PERIOD, GD_DROUGHT_MAX_N
DROUGHT_ANOMALY, DROUGHT_STANDARDIZED = 0, 1   # GD_DROUGHT_ANOMALY, GD_DROUGHT_STANDARDIZED
DROUGHT_EV_MAPS = ("n_valid", "n_dry", "n_events", "event_steps", "max_duration", "mean_duration", "max_severity", "total_severity",
                   "peak", "longest_start", "worst_start", "last_run")   # GD_DROUGHT_EV_*: bit k of `which`
CCL_TILE_T, CCL_TILE_H, CCL_TILE_W = 4, 8, 32   # GD_CCL_TILE_T, GD_CCL_TILE_H, GD_CCL_TILE_W
CCL_U8, CCL_STRUCT_BITS = 2, 13   # GD_CCL_U8 (the dtype tag of a uint8 cube), GD_CCL_STRUCT_BITS
CCL_NO_TILES, CCL_SEVERITY = 1, 1   # GD_CCL_NO_TILES (gd_ccl_label flags), GD_CCL_SEVERITY (gd_ccl_tracks flags)
CCL_BOUNDS = ("n", "t0", "t1", "h0", "h1", "w0", "w1")   # GD_CCL_B_*: column k of the bounds table
CCL_TRACK = ("count", "area", "severity", "sum_h", "sum_w", "min")   # GD_CCL_TR_*: column k of a track record
CCL_TOTALS = ("volume", "severity", "peak_area", "peak_area_step", "peak", "centroid_t", "centroid_h", "centroid_w")   # GD_CCL_TO_*
NBR_MAX_HW, NBR_MAX_K, NBR_MAX_S = 1 << 20, 8, 32   # GD_NBR_MAX_HW, GD_NBR_MAX_K, GD_NBR_MAX_S
NBR_NORMALIZE = {"window": 0, "valid": 1}            # GD_NBR_WINDOW, GD_NBR_VALID
QM_MAX_T, QM_MAX_N, QM_MAX_Q, QM_MAX_PERIOD, QM_MAX_F, QM_SMALL_N = 2048, 2048, 256, 366, 16, 32   # GD_QM_MAX_*, GD_QM_SMALL_N
QM_LAYOUT_QSM, QM_LAYOUT_SQM = 0, 1                  # GD_QM_LAYOUT_*
QM_ROUTES = {"auto": 0, "small": 1, "long": 2}       # GD_QM_ROUTE_*
QM_KINDS = {"eqm": 0, "qdm": 1}                      # GD_QM_EQM, GD_QM_QDM
QM_EXTRAPOLATE = {"constant": 0, "clip": 1}          # GD_QM_CONSTANT, GD_QM_CLIP

c_fp = C.c_void_p  # device pointers travel as integers


class ConvDesc(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("M", C.c_int), ("Mstore", C.c_int), ("Ck", C.c_int), ("ks", C.c_int),
        ("stride", C.c_int), ("pad", C.c_int), ("transposed", C.c_int),
        ("Hi", C.c_int), ("Wi", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int),
        ("a", c_fp), ("a_bs", C.c_long), ("a_sm", C.c_long), ("a_sc", C.c_long), ("a_st", C.c_long),
        ("x", c_fp), ("x_bs", C.c_long),
        ("in_scale", c_fp), ("in_shift", c_fp), ("in_relu", C.c_int),
        ("y", c_fp), ("y_bs", C.c_long),
        ("out_layout", C.c_int), ("out_bf16", C.c_int), ("ldo", C.c_int),
        ("alpha", c_fp), ("bias", c_fp), ("res", c_fp), ("res_bs", C.c_long),
        ("act", C.c_int), ("accumulate", C.c_int), ("precision", C.c_int),
        ("sub_oy", C.c_int), ("sub_ox", C.c_int), ("sub_step", C.c_int),
    ]


class GemmNTDesc(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("M", C.c_int), ("N", C.c_int), ("kseg", C.c_int), ("klen", C.c_long),
        ("a", c_fp), ("a_bs", C.c_long), ("a_ss", C.c_long), ("lda", C.c_long),
        ("bm", c_fp), ("b_bs", C.c_long), ("b_ss", C.c_long), ("ldb", C.c_long),
        ("im2col", C.c_int), ("ks", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
        ("Hi", C.c_int), ("Wi", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int),
        ("in_scale", c_fp), ("in_shift", c_fp), ("in_relu", C.c_int),
        ("c", c_fp), ("c_bs", C.c_long), ("ldc", C.c_long),
        ("alpha", c_fp), ("bias", c_fp),
        ("accumulate", C.c_int), ("splits", C.c_int), ("precision", C.c_int),
    ]


_i, _l, _f, _p, _sz = C.c_int, C.c_long, C.c_float, c_fp, C.c_size_t

# name -> (restype, argtypes); every symbol declared in include/gandanet.h
SIGNATURES = {
    "gd_version": (_i, []),
    "gd_set_deterministic": (None, [_i]),
    "gd_get_deterministic": (_i, []),
    "gd_set_det_reduce": (_i, [_i]),
    "gd_get_det_reduce": (_i, []),
    "gd_set_split_reduce": (_i, [_i]),
    "gd_get_split_reduce": (_i, []),
    "gd_split_ws_bytes": (_sz, []),
    "gd_last_error": (_i, [C.c_char_p, _i]),
    "gd_sizeof_conv_desc": (_i, []),
    "gd_sizeof_gemm_nt_desc": (_i, []),
    "gd_conv2d": (_i, [C.POINTER(ConvDesc), _p]),
    "gd_gemm_nt": (_i, [C.POINTER(GemmNTDesc), _p]),
    "gd_gemm_nt_ws": (_i, [C.POINTER(GemmNTDesc), _p, _p, _sz]),
    "gd_gemm_nt_plan": (_i, [C.POINTER(GemmNTDesc), _sz, C.POINTER(_i), C.POINTER(_sz)]),
    "gd_conv3x3_ws_bytes": (_sz, [_i, _i]),
    "gd_conv3x3_eligible": (_i, [C.POINTER(ConvDesc)]),
    "gd_conv3x3": (_i, [C.POINTER(ConvDesc), _p, _sz, _p]),
    "gd_conv3x3_wgrad": (_i, [_p, _l, _p, _p, _l, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p]),
    "gd_conv3x3_wgrad_ws": (_i, [_p, _l, _p, _p, _l, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _sz]),
    "gd_conv3x3_wgrad_plan": (_i, [_i, _i, _i, _i, _i, _i, _sz, C.POINTER(_i), C.POINTER(_sz)]),
    "gd_pack_16_split": (_i, [_p, _l, _i, _i, _i, _p, _p, _i, _p, _l, _i, _l, _i, _i, _p, _l, _i, _l, _i, _i, _p]),
    "gd_pack_16_split_masked": (_i, [_p, _l, _i, _i, _i, _p, _p, _i, _p, _l, _i, _l, _i, _i, _p, _l, _i, _l, _i, _i, _p, _l, _p]),
    "gd_split3_weights": (_i, [_p, _l, _l, _l, _p, _p]),
    "gd_bn_stats_ws_floats": (_sz, [_i, _i, _l]),
    "gd_bn_stats": (_i, [_p, _l, _i, _i, _l, _f, _f, _p, _p, _p, _p, _p, _p]),
    "gd_bn_fold": (_i, [_p, _p, _p, _p, _i, _p, _p, _p]),
    "gd_bn_fold_eval": (_i, [_p, _p, _p, _p, _f, _i, _p, _p, _p, _p]),
    "gd_affine_act": (_i, [_p, _l, _p, _p, _i, _i, _l, _i, _p, _l, _p]),
    "gd_bn_act_bwd": (_i, [_p, _l, _p, _l, _p, _p, _p, _p, _p, _i, _i, _l, _i, _i, _p, _p, _p, _l, _i, _p, _p]),
    "gd_bn_stats_local": (_i, [_p, _l, _i, _i, _l, _p, _p, _p]),
    "gd_bn_stats_merge": (_i, [_p, _i, _i, _f, _f, _p, _p, _p, _p, _p]),
    "gd_bn_act_bwd_dx": (_i, [_p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _f, _i, _i, _l, _i, _p, _l, _i, _p]),
    "gd_bicubic_fwd": (_i, [_p, _i, _i, _i, _p, _i, _i, _f, _f, _p]),
    "gd_bicubic_bwd": (_i, [_p, _i, _i, _i, _p, _i, _i, _f, _f, _p]),
    "gd_bilinear_fwd": (_i, [_p, _i, _i, _i, _p, _i, _i, _i, _p, _p]),
    "gd_bilinear_bwd": (_i, [_p, _i, _i, _i, _p, _i, _i, _p]),
    "gd_maxpool2_fwd": (_i, [_p, _i, _i, _i, _p, _p]),
    "gd_maxpool2_bwd": (_i, [_p, _p, _i, _i, _i, _p, _p]),
    "gd_act_fwd": (_i, [_p, _p, _l, _i, _p]),
    "gd_act_bwd": (_i, [_p, _p, _p, _l, _i, _p]),
    "gd_axpby": (_i, [_p, _f, _p, _f, _l, _p]),
    "gd_scale_dev": (_i, [_p, _p, _p, _l, _i, _p]),
    "gd_copy_rows": (_i, [_p, _l, _l, _p, _l, _l, _i, _i, _i, _p]),
    "gd_channel_sum": (_i, [_p, _l, _i, _i, _l, _p, _i, _p, _p]),
    "gd_copy_slab": (_i, [_p, _l, _p, _l, _i, _l, _i, _p]),
    "gd_softmax_rows": (_i, [_p, _p, _l, _i, _f, _p]),
    "gd_softmax_rows_bwd": (_i, [_p, _p, _p, _l, _i, _f, _p]),
    "gd_dot": (_i, [_p, _p, _l, _p, _i, _p, _p]),
    "gd_transpose": (_i, [_p, _p, _i, _i, _i, _p]),
    "gd_add_transpose": (_i, [_p, _p, _i, _i, _p]),
    "gd_bce_logits": (_i, [_p, _l, _f, _p, _p, _p, _p]),
    "gd_bce_logits_target": (_i, [_p, _p, _l, _p, _p, _p, _p, _p]),
    "gd_leaky_fwd": (_i, [_p, _p, _l, _f, _p]),
    "gd_leaky_bwd": (_i, [_p, _p, _p, _l, _f, _p]),
    "gd_mse": (_i, [_p, _p, _l, _p, _p, _p, _p]),
    "gd_l1": (_i, [_p, _p, _l, _p, _p, _p, _p]),
    "gd_tv": (_i, [_p, _i, _i, _i, _i, _f, _p, _p, _p, _p]),
    "gd_ssim": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "gd_ssim_samples": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p]),
    "gd_ssim_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "gd_adamw": (_i, [_p, _p, _p, _p, _l, _i, _f, _f, _f, _f, _f, _f, _p]),
    "gd_pam_flash_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _l, _p, _l, _p, _p, _p, _p]),
    "gd_pam_key_sqnorm_max": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "gd_pam_fwd_shift_ws_bytes": (_sz, [_i, _i]),
    "gd_pam_flash_fwd_shift": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _l, _p, _l, _p, _p, _i, _p, _sz, _p]),
    "gd_pam_flash_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _l, _p, _sz, _p]),
    "gd_pam_bwd_scratch_bytes": (_sz, [_i, _i]),
    "gd_pam_wide_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _l, _p, _l, _p, _p, _p]),
    "gd_pam_wide_scratch_bytes": (_sz, [_i, _i, _i]),
    "gd_pam_wide_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "gd_pam_f32_fwd": (_i, [_p, _l, _p, _l, _p, _l, _i, _i, _i, _i, _i, _p, _p, _l, _p, _l, _p, _p, _p]),
    "gd_pam_f32_bwd": (_i, [_p, _l, _p, _l, _p, _l, _p, _l, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "gd_pam_attn_stats": (_i, [_p, _l, _p, _l, _i, _i, _i, _i, _f, _p, _p, _p, _p]),
    "gd_pam_attn_received": (_i, [_p, _l, _p, _l, _p, _i, _i, _i, _i, _f, _p, _p]),
    "gd_pam_attn_rows": (_i, [_p, _l, _p, _l, _p, _i, _i, _i, _i, _i, _f, _p, _p, _p]),
    "gd_round_to_16": (_i, [_p, _p, _l, _f, _i, _p]),
    "gd_chan_dot": (_i, [_p, _l, _p, _l, _i, _i, _i, _p, _p, _p, _p]),
    "gd_pam_f16_scale": (_i, [_p, _l, _i, _i, _i, _p, _p, _p, _p, _p]),
    "gd_conv3x3_nhwc_pack": (_i, [_p, _i, _i, _i, _p, _sz, _p]),
    "gd_conv3x3_nhwc": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "gd_conv3x3_nhwc_f32out": (_i, [_p, _p, _p, _p, _l, _i, _i, _i, _i, _i, _i, _p]),
    "gd_disc_stem_fwd": (_i, [_p, _i, _i, _i, _i, _p, _p, _i, _f, _p, _i, _p]),
    "gd_disc_stem_wgrad": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p]),
    "gd_disc_stem_wgrad_ws": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p, _sz]),
    "gd_disc_stem_dgrad": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p]),
    "gd_conv3x3_nhwc_s2": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _i, _p]),
    "gd_conv3x3_nhwc_s2_dgrad": (_i, [_p, _p, _p, _f, _p, _i, _i, _i, _i, _i, _i, _p]),
    "gd_nhwc_flatten_fwd": (_i, [_p, _i, _i, _i, _p, _i, _p]),
    "gd_nhwc_flatten_bwd": (_i, [_p, _p, _f, _i, _i, _i, _p, _i, _p]),
    "gd_nhwc_to_nchw16": (_i, [_p, _i, _i, _i, _p, _p, _i, _p]),
    "gd_nhwc_to_nchw16_ws": (_i, [_p, _i, _i, _i, _p, _p, _i, _p, _p, _sz]),
    "gd_nhwc_stem_fwd": (_i, [_p, _i, _i, _i, _i, _p, _p, _i, _i, _p, _i, _p]),
    "gd_nhwc_stem_bwd": (_i, [_p, _i, _i, _i, _i, _p, _i, _p, _i, _p]),
    "gd_nhwc_maxpool2_fwd": (_i, [_p, _i, _i, _i, _i, _p, _i, _p]),
    "gd_nhwc_maxpool2_bwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _i, _p]),
    "gd_nhwc_l1": (_i, [_p, _p, _l, _p, _i, _p, _i, _p]),
    "gd_nhwc_l1_grad": (_i, [_p, _p, _l, _p, _i, _p, _i, _p]),
    "gd_shift_sum9_fwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "gd_shift_sum9_bwd": (_i, [_p, _p, _i, _i, _i, _p]),
    "gd_combine_inputs": (_i, [_p, _i, _i, _i, _f, _p, _i, _i, _i, _f, _p, _i, _i, _i, _p]),
    "gd_hist_match_ws_bytes": (_sz, [_l, _l]),
    "gd_hist_match": (_i, [_p, _p, _i, _l, _l, C.c_double, _p, _p, _sz, _p]),
    "gd_hist_match_host": (_i, [_p, _p, _i, _l, _l, C.c_double, _p]),
    "gd_eval_stats_ws_bytes": (_sz, [_l]),
    "gd_eval_stats": (_i, [_p, _p, _l, _l, _p, C.c_double, C.c_double, _i, _p, _p, _sz, _p]),
    "gd_masked_plane_mean_ws_bytes": (_sz, [_l, _l]),
    "gd_masked_plane_mean": (_i, [_p, _l, _l, _p, _p, _p, _p, _sz, _p]),
    "gd_ensemble_stats": (_i, [_p, _i, _l, _l, _i, _p, _p, _p]),
    "gd_eval_merge_host": (_i, [C.POINTER(C.c_double), _l, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gd_grad_sqnorm_ws_bytes": (_sz, [_l]),
    "gd_grad_sqnorm": (_i, [C.POINTER(_p), C.POINTER(_l), _i, _f, _i, _p, _p, _sz, _p]),
    "gd_guard_finalize": (_i, [_p, C.c_double, _i, _p]),
    "gd_adamw_guarded": (_i, [_p, _p, _p, _p, _p, _l, _p, _f, _f, _f, _f, _f, _f, _f, _p]),
    "gd_gaussian_weights_host": (_i, [C.c_double, C.c_double, C.POINTER(C.c_double), _i]),
    "gd_correlate1d_axis": (_i, [_p, _p, _i, _l, _l, _l, C.POINTER(C.c_double), _i, _i, _p]),
    "gd_savgol_edges_axis": (_i, [_p, _p, _i, _l, _l, _l, _p, _i, _p]),
    "gd_median_nd": (_i, [_p, _p, _i, C.POINTER(C.c_int64), C.POINTER(_i), _p]),
    "gd_fill_prepare": (_i, [_p, C.c_double, _p, _p, _i, _l, _p]),
    "gd_fill_ratio": (_i, [_p, _p, _p, C.c_double, _p, _i, _l, _p]),
    "gd_zoom_axis_ws_bytes": (_sz, [_l, _l, _l, _i, _i]),
    "gd_zoom_axis": (_i, [_p, _p, _i, _i, _l, _l, _l, _l, _i, _i, _p, _sz, _p]),
    "gd_spline_prefilter_axis": (_i, [_p, _p, _i, _l, _l, _l, _p]),
    "gd_restore_units": (_i, [_p, _i, _p, _i, _p, _l, _l, C.c_double, C.c_double, C.c_double, _p, _i, _p]),
    "gd_masked_plane_mean_f64_ws_bytes": (_sz, [_l, _l]),
    "gd_masked_plane_mean_f64": (_i, [_p, _l, _l, _p, _p, _p, _p, _sz, _p]),
    "gd_blend_region": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "gd_channel_moments_ws_bytes": (_sz, [_l, _l]),
    "gd_channel_moments": (_i, [_p, _i, _l, _l, _p, _p, _sz, _p]),
    "gd_scale_from_moments_host": (_i, [C.POINTER(C.c_double), _l, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]),
    "gd_channel_affine": (_i, [_p, _i, _p, _i, _l, _l, _p, _p, _i, _l, _l, _p]),
    "gd_freq_cos_table_host": (_i, [_l, _i, C.POINTER(C.c_double)]),
    "gd_freq_augment_axis": (_i, [_p, _p, _i, _l, _l, _l, _p, _i, _p, _p]),
    "gd_zone_rasterize": (_i, [_p, _l, C.POINTER(_l), _i, _p, _l, _p, _l, _p, _p]),
    "gd_zone_rasterize_host": (_i, [C.POINTER(C.c_double), _l, C.POINTER(_l), _i, C.POINTER(C.c_double), _l, C.POINTER(C.c_double), _l,
                                    C.POINTER(C.c_uint32)]),
    "gd_zone_mean_ws_bytes": (_sz, [_l, _l, _i]),
    "gd_zone_mean": (_i, [_p, _i, _l, _l, _p, _i, _p, _p, _p, _p, _sz, _p]),
    "gd_stl_decompose": (_i, [_p, _i, _l, _l, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "gd_stl_decompose_host": (_i, [_p, _i, _l, _l, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "gd_series_stats": (_i, [_p, _p, _i, _l, _l, _p, _i, _p, _i, _p]),
    "gd_series_stats_host": (_i, [_p, _p, _i, _l, _l, _p, _i, _p, _i]),
    "gd_series_skill": (_i, [_p, _l, _i, _i, _p, _p]),
    "gd_series_skill_host": (_i, [_p, _l, _i, _i, _p]),
    "gd_series_lstsq": (_i, [_p, _i, _l, _l, _p, _i, _p, _p, _p, _p]),
    "gd_series_lstsq_host": (_i, [_p, _i, _l, _l, _p, _i, _p, _p, _p]),
    "gd_harmonic_finalize": (_i, [_p, _i, _l, _i, _i, C.c_double, _p, _p, _p, _p, _p, _p, _p]),
    "gd_block_mean": (_i, [_p, _i, _l, _l, _l, _i, _i, _p, _i, _p, _p, _p]),
    "gd_block_mean_host": (_i, [_p, _i, _l, _l, _l, _i, _i, _p, _i, _p, _p]),
    "gd_trend_test": (_i, [_p, _i, _l, _l, _p, _i, _p, _i, C.c_double, _p, _p]),
    "gd_trend_test_host": (_i, [_p, _i, _l, _l, _p, _i, _p, _i, C.c_double, _p]),
    "gd_change_point": (_i, [_p, _i, _l, _l, _p, _p, _p, _i, _i, _p, _p]),
    "gd_change_point_host": (_i, [_p, _i, _l, _l, _p, _p, _p, _i, _i, _p]),
    "gd_lag_corr": (_i, [_p, _p, _i, _l, _l, _l, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "gd_lag_corr_host": (_i, [_p, _p, _i, _l, _l, _l, _i, _i, _i, _i, _p, _p, _p, _p]),
    "gd_series_acf": (_i, [_p, _i, _l, _l, _i, _i, _i, _p, _p, _p, _p]),
    "gd_series_acf_host": (_i, [_p, _i, _l, _l, _i, _i, _i, _p, _p, _p]),
    "gd_corr_signif": (_i, [_p, _p, _p, _l, _p, _l, _p, _p, _p, _p]),
    "gd_tc_estimate": (_i, [_p, _p, _p, _i, _l, _l, _i, _p, _p, _p, _p, _p, _p]),
    "gd_tc_estimate_host": (_i, [_p, _p, _p, _i, _l, _l, _i, _p, _p, _p, _p, _p]),
    "gd_tc_group": (_i, [_l]),
    "gd_tc_bootstrap_workspace": (_sz, [_l, _l, _l]),
    "gd_tc_bootstrap": (_i, [_p, _p, _p, _i, _l, _l, _p, _l, _i, _p, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "gd_tc_bootstrap_host": (_i, [_p, _p, _p, _i, _l, _l, _p, _l, _i, _p, _i, _p, _p, _p, _p]),
    "gd_ssa_decompose": (_i, [_p, _i, _l, _l, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "gd_ssa_decompose_host": (_i, [_p, _i, _l, _l, _i, _i, _i, _p, _p, _p, _p, _p]),
    "gd_ssa_fill": (_i, [_p, _i, _l, _l, _i, _i, _i, _p, C.c_double, _i, _i, _p, _p, _p, _p]),
    "gd_ssa_fill_host": (_i, [_p, _i, _l, _l, _i, _i, _i, _p, C.c_double, _i, _i, _p, _p, _p]),
    "gd_km_assign": (_i, [_p, _i, _l, _l, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    "gd_km_assign_host": (_i, [_p, _i, _l, _l, _p, _i, _p, _p, _p, _p, _p, _p, _p]),
    "gd_km_update_ws_bytes": (_sz, [_l, _l, _i]),
    "gd_km_update_min_ws_bytes": (_sz, [_l, _i]),
    "gd_km_update": (_i, [_p, _i, _l, _l, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "gd_km_update_host": (_i, [_p, _i, _l, _l, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "gd_km_farthest": (_i, [_p, _l, _p, _i, _p, _p]),
    "gd_km_farthest_host": (_i, [_p, _l, _p, _i, _p]),
    "gd_ens_verify_ws_bytes": (_sz, [_l]),
    "gd_ens_verify": (_i, [_p, _i, _l, _p, _l, _l, _p, C.c_double, _i, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "gd_ens_verify_host": (_i, [_p, _i, _l, _p, _l, _l, _p, C.c_double, _i, _p, _p, _p, _p, _p]),
    "gd_ens_verify_merge_host": (_i, [C.POINTER(C.c_double), _l, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gd_eof_prepare": (_i, [_p, _i, _l, _l, _p, _p, _i, _p, _p, _p]),
    "gd_eof_prepare_host": (_i, [_p, _i, _l, _l, _p, _p, _i, _p, _p]),
    "gd_eof_gram_ws_bytes": (_sz, [_l, _l]),
    "gd_eof_gram": (_i, [_p, _i, _l, _l, _p, _p, _p, _p, _p, _sz, _p]),
    "gd_eof_gram_host": (_i, [_p, _i, _l, _l, _p, _p, _p, _p]),
    "gd_eof_project": (_i, [_p, _i, _l, _l, _p, _p, _p, _i, _p, _i, _p, _p]),
    "gd_eof_project_host": (_i, [_p, _i, _l, _l, _p, _p, _p, _i, _p, _i, _p]),
    "gd_eof_reconstruct": (_i, [_p, _p, _p, _p, _p, _l, _l, _i, _p, _i, _p]),
    "gd_eof_reconstruct_host": (_i, [_p, _p, _p, _p, _p, _l, _l, _i, _p, _i]),
    "gd_spec_twiddle_host": (_i, [_l, _p]),
    "gd_spec_default_bins": (_i, [_l, _l, C.c_double, C.c_double]),
    "gd_spec_bins_host": (_i, [_l, _l, C.c_double, C.c_double, _i, C.c_double, _p, _p, _p]),
    "gd_spec_prepare": (_i, [_p, _i, _l, _l, _l, _p, _p, _p, _i, _p, _p, _p]),
    "gd_spec_prepare_host": (_i, [_p, _i, _l, _l, _l, _p, _p, _p, _i, _p, _p]),
    "gd_spec_power_ws_bytes": (_sz, [_l, _l, _l, _i]),
    "gd_spec_power": (_i, [_p, _i, _l, _l, _l, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _sz, _p]),
    "gd_spec_power_host": (_i, [_p, _i, _l, _l, _l, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p]),
    "gd_spec_cross_ws_bytes": (_sz, [_l, _l, _l, _i]),
    "gd_spec_cross": (_i, [_p, _p, _i, _l, _l, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _sz, _p]),
    "gd_spec_cross_host": (_i, [_p, _p, _i, _l, _l, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p]),
    "gd_drought_clim": (_i, [_p, _i, _l, _l, _i, _i, _l, _l, _p, _p, _p]),
    "gd_drought_clim_host": (_i, [_p, _i, _l, _l, _i, _i, _l, _l, _p, _p]),
    "gd_drought_index": (_i, [_p, _i, _l, _l, _p, _i, _i, _i, _i, _p, _p, _p]),
    "gd_drought_index_host": (_i, [_p, _i, _l, _l, _p, _i, _i, _i, _i, _p, _p]),
    "gd_drought_rank": (_i, [_p, _i, _l, _l, _i, _i, _l, _l, _p, _p, _i, _p, _p]),
    "gd_drought_rank_host": (_i, [_p, _i, _l, _l, _i, _i, _l, _l, _p, _p, _i, _p]),
    "gd_drought_events": (_i, [_p, _i, _l, _l, C.c_double, _i, _i, _p, _p, _p, _p]),
    "gd_drought_events_host": (_i, [_p, _i, _l, _l, C.c_double, _i, _i, _p, _p, _p]),
    "gd_drought_exceed": (_i, [_p, _i, _l, C.c_double, _p, _p]),
    "gd_drought_exceed_host": (_i, [_p, _i, _l, C.c_double, _p]),
    "gd_ccl_ws_bytes": (_sz, [_l]),
    "gd_ccl_label": (_i, [_p, _i, _l, _l, _l, C.c_double, _p, _i, _i, _p, _p]),
    "gd_ccl_label_host": (_i, [_p, _i, _l, _l, _l, C.c_double, _p, _i, _i, _p]),
    "gd_ccl_filter": (_i, [_p, _l, _i, _p, _sz, _p]),
    "gd_ccl_filter_host": (_i, [_p, _l, _i]),
    "gd_ccl_relabel": (_i, [_p, _l, _p, _p, _p, _sz, _p]),
    "gd_ccl_relabel_host": (_i, [_p, _l, _p, _p]),
    "gd_ccl_bounds": (_i, [_p, _l, _l, _l, _i, _p, _p]),
    "gd_ccl_bounds_host": (_i, [_p, _l, _l, _l, _i, _p]),
    "gd_ccl_offsets": (_i, [_p, _i, _p, _p, _sz, _p]),
    "gd_ccl_offsets_host": (_i, [_p, _i, _p]),
    "gd_ccl_tracks": (_i, [_p, _i, _l, _l, _l, C.c_double, _p, _p, _p, _i, _l, _p, _i, _p, _p, _p]),
    "gd_ccl_tracks_host": (_i, [_p, _i, _l, _l, _l, C.c_double, _p, _p, _p, _i, _l, _p, _i, _p, _p]),
    "gd_ccl_totals": (_i, [_p, _p, _p, _i, _p, _p]),
    "gd_ccl_totals_host": (_i, [_p, _p, _p, _i, _p]),
    "gd_nbr_ws_bytes": (_sz, [_l, _l, _i, _l]),
    "gd_nbr_fss": (_i, [_p, _p, _i, _l, _l, _l, _p, _p, _p, _i, _i, _p, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "gd_nbr_fss_host": (_i, [_p, _p, _i, _l, _l, _l, _p, _p, _p, _i, _i, _p, _i, _i, _p, _p, _p]),
    "gd_nbr_fraction": (_i, [_p, _i, _l, _l, _l, _p, _p, _i, _i, _i, _p, _p, _sz, _p]),
    "gd_nbr_fraction_host": (_i, [_p, _i, _l, _l, _l, _p, _p, _i, _i, _i, _p]),
    "gd_qm_quantiles": (_i, [_p, _p, _i, _l, _l, _p, _i, _i, _i, _l, _l, _p, _i, _i, _i, _p, _p, _p]),
    "gd_qm_quantiles_host": (_i, [_p, _p, _i, _l, _l, _p, _i, _i, _i, _l, _l, _p, _i, _i, _i, _p, _p]),
    "gd_qm_apply": (_i, [_p, _i, _l, _l, _l, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "gd_qm_apply_host": (_i, [_p, _i, _l, _l, _l, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "gd_augment_d4": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _f, _p]),
    "gd_bcast_mul": (_i, [_p, _p, _p, _i, _i, _l, _i, _p]),
    "gd_row_dot": (_i, [_p, _p, _p, _l, _l, _p]),
    "gd_chan_maxmean_fwd": (_i, [_p, _p, _p, _i, _i, _l, _p]),
    "gd_chan_maxmean_bwd": (_i, [_p, _p, _p, _i, _i, _l, _p]),
    "gd_comm_unique_id": (_i, [C.c_char_p]),
    "gd_comm_init": (_i, [_i, _i, C.c_char_p]),
    "gd_comm_world": (_i, []),
    "gd_allreduce": (_i, [_p, _sz, _i, _p]),
    "gd_reduce_scatter": (_i, [_p, _p, _sz, _i, _p]),
    "gd_allgather": (_i, [_p, _p, _sz, _i, _p]),
    "gd_comm_destroy": (_i, []),
    "gd_pack_bf16": (_i, [_p, _l, _i, _i, _i, _p, _f, _p, _i, _i, _p, _i, _i, _i, _i, _p]),
    "gd_pack_16": (_i, [_p, _l, _i, _i, _i, _p, _f, _p, _i, _i, _p, _i, _i, _i, _i, _i, _p]),
    "gd_pack_16_affine": (_i, [_p, _l, _i, _i, _i, _p, _p, _i, _p, _i, _i, _p, _i, _i, _i, _p]),
}

_lib = None


class GandanetError(RuntimeError):
    pass


def load() -> C.CDLL:
    """dlopen the library (once) and attach the prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GandanetError(
            f"{LIB_PATH} is missing: the HIP extension is not built (run __graft_entry__.build()). "
            "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    if lib.gd_sizeof_conv_desc() != C.sizeof(ConvDesc) or lib.gd_sizeof_gemm_nt_desc() != C.sizeof(GemmNTDesc):
        raise GandanetError("descriptor struct layout differs between _lib.py and libgandanet_hip.so")
    _lib = lib
    return lib


def last_error() -> str:
    buf = C.create_string_buffer(512)
    load().gd_last_error(buf, 512)
    return buf.value.decode()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise GandanetError(f"{what or 'gandanet call'} failed (rc={rc}): {last_error()}")
