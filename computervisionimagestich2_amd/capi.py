"""ctypes binding of libstitch_hip.so (include/stitch.h) -- the product path.

Two families, mirroring the header:
  * host-buffer calls on numpy arrays of shape (3, H, W) (CImg's planar layout, CImg.h:11787-11793);
  * device-resident calls on torch CUDA(=HIP) tensors, enqueued on torch's current stream.
PyTorch supplies device memory and streams only; every computation is a hand-written HIP kernel in csrc/.
There is no fallback: a missing library or a missing GPU raises.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STITCH_LIB", os.path.join(_HERE, "libstitch_hip.so"))  # STITCH_LIB: A/B builds of the same ABI

# kernel ids of stitch_plan_read_profile -> the HIP kernel symbol each one times (rocprofv3 reports the same names)
KERNELS = ("compose", "seam", "mask", "vv_x_fwd", "vv_x_bwd", "vv_y_fwd", "vv_y_bwd", "decimate", "collapse_top", "collapse",
           "collapse_l0", "vv_xbyf", "vv_x_fwd_src", "coarse")
KERNEL_SYMBOLS = {"compose": "k_src_index (source-fused) / k_compose", "seam": "k_seam", "mask": "k_mask", "vv_x_fwd": "k_vv_x_fwd<T, false, false>", "vv_x_bwd": "k_vv_x_bwd",
                  "vv_y_fwd": "k_vv_y_fwd1 / k_vv_y_fwd", "vv_y_bwd": "k_vv_y_bwd_dec", "decimate": "k_decimate", "collapse_top": "k_blend_top",
                  "collapse": "k_collapse<float, false>", "collapse_l0": "k_collapse<T, true>", "vv_xbyf": "k_vv_xbyf<false, float, 0, false>", "vv_x_fwd_src": "k_vv_x_fwd<T, true, false>",
                  "coarse": "k_coarse"}


class StitchError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"stitch error {code}: {text}")
        self.code = code


OK, ERR_ARG, ERR_EMPTY_MIDROW, ERR_ZERO_OVERLAP, ERR_PYRAMID, ERR_HIP, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5, -6
ERR_NO_MAP, ERR_CAPACITY = -7, -8  # the whole-panorama calls (include/stitch_panorama.h)
CALL_MASK_KEEP = 64  # STITCH_CALL_MASK_KEEP (include/stitch_mask_keep.h): a bit of stitch_plan_call_forms beside the STITCH_FAST_* values 1 .. 32


class BlendOpts(C.Structure):
    """stitch_blend_opts.  Defaults = root variant (ImageProcess.cpp:648-773)."""
    _fields_ = [("sigma", C.c_float), ("blur_kind", C.c_int), ("level_rule", C.c_int), ("seam_rule", C.c_int)]

    def __init__(self, sigma=2.0, blur_kind=0, level_rule=0, seam_rule=0):
        super().__init__(sigma, blur_kind, level_rule, seam_rule)


ROOT_OPTS = dict(sigma=2.0, blur_kind=0, level_rule=0, seam_rule=0)
EX6_OPTS = dict(sigma=2.0, blur_kind=1, level_rule=1, seam_rule=1)


class Seam(C.Structure):
    _fields_ = [("sum_a_x", C.c_int32), ("n_a", C.c_int32), ("sum_ov_x", C.c_int32), ("n_ov", C.c_int32),
                ("ratio", C.c_float), ("ov", C.c_float), ("branch", C.c_int32), ("start", C.c_int32)]

    def as_tuple(self):
        return (self.sum_a_x, self.n_a, self.sum_ov_x, self.n_ov, self.branch, self.start)


class PairDesc(C.Structure):
    """stitch_pair_desc: one independent stitch step of a batch (device pointers)."""
    _fields_ = [("frame", C.c_void_p), ("fw", C.c_int), ("fh", C.c_int), ("p", C.c_double * 8), ("offx", C.c_float),
                ("offy", C.c_float), ("mosaic", C.c_void_p), ("mw", C.c_int), ("mh", C.c_int), ("ox", C.c_int), ("oy", C.c_int),
                ("out", C.c_void_p), ("out_u8", C.c_void_p)]


def _signatures(*rows):
    """Rows of (names, restype, *argtypes) -> {name: (restype, argtypes)}; `stem_*` stands for the twins stem_u8 and stem_f32."""
    return {n: (res, list(args)) for names, res, *args in rows for n in re.sub(r"(\S+)\*", r"\1u8 \1f32", names).split()}


# The signature of every function include/stitch.h declares; tests/test_capi_abi.py holds this table to the header.  Every pointer,
# array and stream parameter is a c_void_p: it takes None, a plain int, byref(...), a ctypes array or structure array, or a c_void_p.
vp, i32, f32, f64, sz, u32 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_uint32
SIGNATURES = _signatures(
    ("stitch_abi_version stitch_init stitch_device_count", i32), ("stitch_last_error", C.c_char_p), ("stitch_trim", None),
    ("stitch_set_device", i32, i32), ("stitch_blend_opts_default", None, vp),
    ("stitch_plan_cache_query", i32, i32, i32, vp, vp), ("stitch_pyramid_levels", i32, i32, i32, i32, vp, vp),
    # the per-pixel path: on host buffers, and the device twin with its stream behind
    ("stitch_project_*", i32, vp, i32, i32, f32, vp), ("stitch_dev_project_*", i32, vp, i32, i32, f32, vp, vp),
    ("stitch_warp_*", i32, vp, i32, i32, vp, f32, f32, vp, i32, i32), ("stitch_dev_warp_*", i32, vp, i32, i32, vp, f32, f32, vp, i32, i32, vp),
    ("stitch_move_*", i32, vp, i32, i32, i32, i32, vp, i32, i32), ("stitch_dev_move_*", i32, vp, i32, i32, i32, i32, vp, i32, i32, vp),
    ("stitch_blend_*", i32, vp, vp, i32, i32, vp, vp, vp), ("stitch_dev_blend_*", i32, vp, vp, vp, vp, vp),
    ("stitch_pair_*", i32, vp, i32, i32, vp, f32, f32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp),
    ("stitch_dev_pair_*", i32, vp, vp, i32, i32, vp, f32, f32, vp, i32, i32, i32, i32, vp, vp), ("stitch_dev_pairs_*", i32, vp, vp, i32, vp),
    ("stitch_equalize_u8", i32, vp, i32, i32, vp), ("stitch_dev_equalize_u8", i32, vp, i32, i32, vp, vp),
    ("stitch_lummix_u8", i32, vp, vp, i32, i32, f64, f64), ("stitch_dev_lummix_u8", i32, vp, vp, i32, i32, f64, f64, vp),
    ("stitch_finish_u8", i32, vp, i32, i32, f64, f64, vp), ("stitch_dev_finish_u8", i32, vp, i32, i32, f64, f64, vp, vp),
    # plans
    ("stitch_plan_create", i32, i32, i32, vp, vp), ("stitch_plan_create_batched", i32, i32, i32, vp, i32, vp),
    ("stitch_plan_destroy", None, vp), ("stitch_plan_workspace_bytes", sz, vp), ("stitch_plan_workspace_base", vp, vp),
    ("stitch_plan_capacity stitch_plan_fused_sweep_levels stitch_plan_fast_paths stitch_plan_coarse_from stitch_plan_clear_fault", i32, vp),
    ("stitch_plan_call_forms stitch_plan_set_profiling stitch_plan_set_profiling_kernel", i32, vp, i32),
    ("stitch_plan_levels", i32, vp, vp, vp), ("stitch_plan_collapse_range", i32, vp, i32, vp, vp, vp), ("stitch_plan_status", i32, vp, vp),
    ("stitch_plan_status_at", i32, vp, i32, vp), ("stitch_plan_set_handoff_spin_limit", i32, vp, C.c_uint),
    ("stitch_plan_read_profile", i32, vp, vp, vp, vp),
    # the callers either side of the path
    ("stitch_gray_u8", i32, vp, i32, i32, vp, vp), ("stitch_dev_gray_u8", i32, vp, i32, i32, vp, vp, vp),
    ("stitch_bmp_parse", i32, vp, sz, vp), ("stitch_bmp_file_bytes", sz, i32, i32),
    ("stitch_bmp_decode_u8", i32, vp, sz, vp), ("stitch_dev_bmp_decode_u8", i32, vp, sz, vp, vp, vp),
    ("stitch_bmp_encode_u8", i32, vp, i32, i32, vp, sz), ("stitch_dev_bmp_encode_u8", i32, vp, i32, i32, vp, sz, vp),
    ("stitch_transfer_u8", i32, vp, i32, i32, vp, i32, i32, vp, vp), ("stitch_dev_transfer_u8", i32, vp, i32, i32, vp, i32, i32, vp, vp, vp),
    ("stitch_project_gray_u8", i32, vp, i32, i32, f32, vp, vp, vp), ("stitch_dev_project_gray_u8", i32, vp, i32, i32, f32, vp, vp, vp, vp),
    ("stitch_canvas_bbox", i32, i32, i32, vp, i32, i32, vp, vp, vp, vp), ("stitch_step_geometry", i32, i32, i32, vp, i32, i32, vp),
    ("stitch_dev_step_*", i32, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, sz, vp, vp, vp),
    ("stitch_map_points", i32, vp, vp, vp, vp, i32, vp, f32, f32), ("stitch_shift_points", i32, vp, vp, vp, vp, i32, i32, i32),
    # one pair split into row bands
    ("stitch_band_create", i32, i32, i32, i32, i32, i32, vp, vp), ("stitch_band_destroy", None, vp),
    ("stitch_band_geometry", i32, vp, i32, vp), ("stitch_band_set_level0", i32, vp, i32), ("stitch_band_levels stitch_band_status", i32, vp, vp),
    ("stitch_band_compose_*", i32, vp, vp, i32, i32, vp, f32, f32, vp, i32, i32, i32, i32, vp), ("stitch_band_reduce_x", i32, vp, i32, vp),
    ("stitch_band_reduce_xy_fwd", i32, vp, i32, vp, vp, vp), ("stitch_band_reduce_y_fwd", i32, vp, i32, i32, vp, vp, vp),
    ("stitch_band_reduce_y_bwd", i32, vp, i32, i32, vp, vp, vp, vp), ("stitch_band_reduce_y_fwd_cols", i32, vp, i32, i32, i32, vp, vp, vp),
    ("stitch_band_reduce_y_bwd_cols", i32, vp, i32, i32, i32, vp, vp, vp, vp), ("stitch_band_rows", i32, vp, i32, i32, i32, i32, vp, i32, vp),
    ("stitch_band_top", i32, vp, vp, vp), ("stitch_band_collapse_*", i32, vp, i32, vp, vp),
    # benchmark frames, quantisation, verification hooks
    ("stitch_dev_synth_*", i32, vp, i32, i32, i32, vp), ("stitch_dev_quantize_u8", i32, vp, vp, sz, vp),
    ("stitch_dev_check_fastdiv", i32, f32, vp, vp), ("stitch_dev_check_collapse_taps", i32, i32, i32, i32, vp, vp),
    # features: matching, RANSAC, SIFT
    ("stitch_match_l1_ratio", i32, vp, i32, vp, i32, f64, vp, vp, vp, vp), ("stitch_dev_match_l1_ratio_many", i32, vp, i32, f64, vp),
    ("stitch_dev_match_l1_ratio", i32, vp, i32, vp, i32, f64, vp, vp, vp, vp, vp), ("stitch_ransac_rand", None, u32, vp, i32),
    ("stitch_ransac", i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp), ("stitch_dev_ransac_many stitch_dev_sift_many", i32, vp, i32, vp, vp),
    ("stitch_sift", i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp), ("stitch_sift_filter", i32, f64, vp),
    ("stitch_sift_expn_table", None, vp), ("stitch_sift_elem", None, f64, vp),
)

# The same for include/stitch_panorama.h, the whole panorama (a header of its own, so a table of its own: SIGNATURES states
# stitch.h and nothing else); tests/test_panorama_host.py holds it to that header.
PANORAMA_SIGNATURES = _signatures(
    ("stitch_panorama_opts_default stitch_panorama_destroy", None, vp),
    ("stitch_feature_order", i32, vp, i32, vp, vp), ("stitch_stitch_order", i32, vp, i32, i32, vp, vp, vp),
    ("stitch_dev_map_points", i32, vp, vp, vp, vp, i32, vp, f32, f32, vp), ("stitch_dev_shift_points", i32, vp, vp, vp, vp, i32, i32, i32, vp),
    ("stitch_dev_pair_maps", i32, vp, vp, f64, vp, vp, vp, vp),
    ("stitch_dev_panorama_from_features_u8", i32, vp, vp, i32, vp, vp, vp), ("stitch_dev_panorama_u8", i32, vp, i32, vp, vp, vp),
    ("stitch_panorama_u8", i32, vp, i32, vp, vp), ("stitch_panorama_info", i32, vp, vp, vp, vp, vp),
    ("stitch_panorama_step_at", i32, vp, i32, vp), ("stitch_panorama_pixels", vp, vp), ("stitch_panorama_step_pixels", vp, vp, i32),
    ("stitch_panorama_copy", i32, vp, i32, vp, sz, i32, vp),
)

# The same for include/stitch_rig.h, a calibrated rig; tests/test_rig_host.py holds it to that header.
RIG_SIGNATURES = _signatures(
    ("stitch_rig_opts_default stitch_rig_destroy", None, vp), ("stitch_rig_create", i32, vp, i32, i32, vp, i32, vp, vp),
    ("stitch_rig_from_panorama", i32, vp, vp, i32, vp, vp), ("stitch_rig_info", i32, vp, vp, vp, vp, vp, vp), ("stitch_rig_step_plan", vp, vp, i32),
    ("stitch_dev_rig_stitch_u8", i32, vp, vp, i32, vp, vp, vp, vp), ("stitch_dev_project_many_u8", i32, vp, vp, i32, i32, i32, f32, vp),
    ("stitch_dev_finish_many_u8", i32, vp, i32, i32, i32, f64, f64, vp),
)

# The same for include/stitch_exposure.h, the colour transfer inside the chain; tests/test_exposure_host.py holds it to that header.
EXPOSURE_SIGNATURES = _signatures(
    ("stitch_exposure_opts_default", None, vp), ("stitch_dev_running_stats_f32", i32, vp, vp, vp, i32, i32, vp, vp, vp, vp),
    ("stitch_dev_transfer_form_u8", i32, vp, i32, i32, vp, i32, i32, vp, vp, i32, i32, vp, vp),
    ("stitch_dev_panorama_exposure_from_features_u8", i32, vp, vp, i32, vp, vp, vp, vp), ("stitch_dev_panorama_exposure_u8", i32, vp, i32, vp, vp, vp, vp),
    ("stitch_panorama_exposure_u8", i32, vp, i32, vp, vp, vp), ("stitch_panorama_exposure_stats", i32, vp, i32, vp),
    ("stitch_panorama_exposure_frame_copy", i32, vp, i32, vp, sz, i32, vp),
)

# The same for include/stitch_rig_exposure.h, the colour transfer in a rig's replay; tests/test_rig_exposure_host.py holds it to that header.
RIG_EXPOSURE_SIGNATURES = _signatures(
    ("stitch_rig_create_exposure", i32, vp, i32, i32, vp, i32, vp, vp, vp), ("stitch_rig_from_panorama_exposure", i32, vp, vp, i32, vp, vp, vp),
    ("stitch_dev_rig_stitch_exposure_u8", i32, vp, vp, i32, vp, vp, vp, vp, vp),
    ("stitch_dev_transfer_many_u8", i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp),
)

# The same for include/stitch_calibrate.h, a rig calibrated from several captures; tests/test_calibrate_host.py holds it to that header.
CALIBRATE_SIGNATURES = _signatures(
    ("stitch_calibrate_opts_default stitch_calibration_destroy", None, vp), ("stitch_dev_calibrate_u8", i32, vp, i32, i32, vp, vp, vp),
    ("stitch_dev_calibrate_from_features_u8", i32, vp, vp, i32, i32, vp, vp, vp), ("stitch_calibrate_u8", i32, vp, i32, i32, vp, vp),
    ("stitch_calibration_info", i32, vp, vp, vp, vp, vp, vp, vp), ("stitch_calibration_step_at", i32, vp, i32, vp),
    ("stitch_calibration_counts", i32, vp, vp, vp), ("stitch_calibration_step_support", i32, vp, i32, vp, vp),
    ("stitch_rig_from_calibration", i32, vp, vp, vp, vp),
)

# The same for include/stitch_rig_seams.h, fixed seams for a rig; tests/test_rig_seams_host.py holds it to that header.
RIG_SEAMS_SIGNATURES = _signatures(
    ("stitch_seam_from_sums", i32, i32, i32, i32, i32, i32, i32, vp), ("stitch_dev_pairs_seamed_*", i32, vp, vp, i32, vp, vp),
    ("stitch_rig_fix_seams stitch_rig_seams", i32, vp, vp, i32), ("stitch_rig_clear_seams", i32, vp),
    ("stitch_dev_rig_geometric_seams", i32, vp, vp, vp), ("stitch_dev_rig_coverage_u8", i32, vp, i32, i32, vp, vp),
    ("stitch_rig_step_canvas", i32, vp, i32, vp, vp),
)

# The same for include/stitch_rig_crop.h, the crop of a rig's output; tests/test_rig_crop_host.py holds it to that header.
RIG_CROP_SIGNATURES = _signatures(
    ("stitch_dev_largest_rect_u8", i32, vp, i32, i32, vp, vp), ("stitch_dev_rig_inscribed_rect", i32, vp, i32, vp, vp),
    ("stitch_rig_set_crop", i32, vp, vp, i32), ("stitch_rig_clear_crop", i32, vp), ("stitch_rig_crop stitch_rig_output_size", i32, vp, vp, vp),
)

# The same for include/stitch_rig_formats.h, a rig's frames and mosaics in camera layouts; tests/test_pixfmt_host.py holds it to that
# header.  (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks the eight.)
RIG_FORMAT_SIGNATURES = _signatures(
    ("stitch_image_bytes", i32, i32, i32, i32, i32, i32, vp, vp),
    ("stitch_dev_unpack_many_u8 stitch_dev_pack_many_u8", i32, i32, i32, vp, vp, i32, vp),
    ("stitch_rig_set_formats", i32, vp, i32, i32, i32), ("stitch_rig_formats", i32, vp, vp, vp, vp), ("stitch_rig_clear_formats", i32, vp),
    ("stitch_dev_rig_stitch_fmt_u8", i32, vp, vp, i32, vp, vp, vp, vp, vp),
)

# The same for include/stitch_rig_formats_yuv.h, the 4:2:2 layouts and NV21 (which the calls above take as further codes) and the query of
# the form a frame index took; tests/test_pixfmt_yuv_host.py holds it to that header.  (Bound where the library exports it, likewise.)
RIG_FORMAT_YUV_SIGNATURES = _signatures(
    ("stitch_rig_input_form", i32, vp, i32, vp),
)

# The same for include/stitch_rig_monitor.h, a rig's alignment monitor; tests/test_rig_monitor_host.py holds it to that header.
# (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks the eight.)
RIG_MONITOR_SIGNATURES = _signatures(
    ("stitch_residual_words", i32, i32), ("stitch_dev_pairs_residual_u8", i32, vp, i32, i32, i32, vp, i32, vp, vp),
    ("stitch_rig_set_monitor", i32, vp, i32), ("stitch_rig_clear_monitor", i32, vp), ("stitch_rig_monitor", i32, vp, vp),
    ("stitch_rig_residuals", i32, vp, vp, sz, vp, vp, vp), ("stitch_dev_rig_residual_domain_u8", i32, vp, i32, i32, vp, vp),
    ("stitch_residual_best_shift", i32, vp, i32, i32, vp, vp),
)

# The same for include/stitch_rig_scale.h, a rig's output scale; tests/test_rig_scale_host.py holds it to that header.
# (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks the four.)
RIG_SCALE_SIGNATURES = _signatures(
    ("stitch_dev_scale_pack_many_u8", i32, i32, i32, vp, i32, i32, vp, vp, i32, vp),
    ("stitch_rig_set_output_scale", i32, vp, i32, i32), ("stitch_rig_clear_output_scale", i32, vp), ("stitch_rig_output_scale", i32, vp, vp, vp),
)
SCALE_MAX_FACTOR = 8  # STITCH_SCALE_MAX_FACTOR

# The same for include/stitch_seam_path.h, path seams; tests/test_seam_path_host.py holds it to that header.
# (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks them.)
SEAM_PATH_SIGNATURES = _signatures(
    ("stitch_seam_path_opts_default", None, vp), ("stitch_plan_create_masked", i32, i32, i32, vp, i32, vp), ("stitch_plan_is_masked", i32, vp),
    ("stitch_dev_pairs_pathed_*", i32, vp, vp, i32, vp, vp, vp),
    ("stitch_dev_pairs_seam_path_u8", i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp),
    ("stitch_rig_set_seam_paths", i32, vp, vp), ("stitch_rig_fix_seam_paths", i32, vp, vp, i32), ("stitch_rig_clear_seam_paths", i32, vp),
    ("stitch_rig_seam_paths", i32, vp, vp, vp), ("stitch_rig_last_seam_paths", i32, vp, i32, i32, vp, i32, vp),
)

# The same for include/stitch_seam_anchor.h, temporally anchored path seams; tests/test_seam_anchor_host.py holds it to that header.
# (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks them.)
SEAM_ANCHOR_SIGNATURES = _signatures(
    ("stitch_dev_pairs_seam_path_anchored_u8", i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
    ("stitch_rig_set_seam_anchor", i32, vp, vp), ("stitch_rig_prime_seam_anchor", i32, vp, vp, i32),
    ("stitch_rig_reset_seam_anchor stitch_rig_clear_seam_anchor", i32, vp), ("stitch_rig_seam_anchor", i32, vp, vp, vp),
    ("stitch_rig_last_seam_moved", i32, vp, i32, i32, vp),
)

# The same for include/stitch_rig_exposure_temporal.h, smoothed or fixed transfer statistics for a rig; tests/test_exposure_temporal_host.py
# holds it to that header.  (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks them.)
RIG_EXPOSURE_TEMPORAL_SIGNATURES = _signatures(
    ("stitch_dev_transfer_given_many_u8", i32, vp, vp, i32, i32, i32, vp, i32, vp), ("stitch_dev_stats_filter_f32", i32, vp, i32, i32, vp, vp, vp, vp),
    ("stitch_rig_set_exposure_smoothing", i32, vp, i32),
    ("stitch_rig_clear_exposure_smoothing stitch_rig_reset_exposure_state stitch_rig_clear_fixed_exposure", i32, vp),
    ("stitch_rig_prime_exposure_state stitch_rig_exposure_state stitch_rig_fix_exposure", i32, vp, vp, i32),
    ("stitch_rig_exposure_smoothing stitch_rig_fixed_exposure", i32, vp, vp, vp), ("stitch_rig_last_used_stats", i32, vp, vp, sz, vp, vp),
)
EXPOSURE_KEEP_MAX = 255  # STITCH_EXPOSURE_KEEP_MAX

# The same for include/stitch_collapse_sides.h, the level-0 collapse that reads one image per column block; tests/test_collapse_sides_host.py
# holds it to that header.  (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks the two.)
COLLAPSE_SIDES_SIGNATURES = _signatures(
    ("stitch_plan_collapse_sides", i32, vp, i32, vp), ("stitch_dev_check_collapse_sides", i32, i32, i32, i32, i32, i32, vp, vp, vp),
)

# The same for include/stitch_src_runs.h, the level-0 index planes kept in 16-byte runs; tests/test_src_runs_host.py holds it to that
# header.  (Bound where the library exports it: an A/B build of an earlier tree, STITCH_LIB, lacks the three.)
SRC_RUNS_SIGNATURES = _signatures(
    ("stitch_plan_src_run_counts", i32, vp, vp), ("stitch_src_run_classes", i32, vp, C.c_float, C.c_float, i32, i32, i32, i32, i32, vp, vp),
    ("stitch_plan_src_runs_fill", i32, vp, i32),
)

_lib = None


def lib():
    """Load libstitch_hip.so; fail loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C computervisionimagestich2_amd/csrc). There is no CPU fallback.")
        try:
            # One HIP runtime per process: torch bundles its own libamdhip64.so.7; loading it first makes the
            # loader bind this library's NEEDED libamdhip64.so.7 to the same copy, so tensors, streams and the
            # kernels below share one runtime (loading /opt/rocm's copy first leaves torch without a device).
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(PANORAMA_SIGNATURES.items()) + list(RIG_SIGNATURES.items()) + list(EXPOSURE_SIGNATURES.items()) \
                + list(RIG_EXPOSURE_SIGNATURES.items()) + list(CALIBRATE_SIGNATURES.items()) + list(RIG_SEAMS_SIGNATURES.items()):
            try:
                f = getattr(L, name)
            except AttributeError:
                raise ImportError(f"{LIB_PATH} does not export {name}: it was built from another include/stitch.h") from None
            f.restype, f.argtypes = res, args
        L.stitch_plan_handoff_counts.restype, L.stitch_plan_handoff_counts.argtypes = i32, [vp, vp]  # include/stitch_handoff.h
        if hasattr(L, "stitch_plan_g_flag_counts"):  # include/stitch_g_flags.h (an A/B build of an earlier tree, STITCH_LIB, lacks it)
            L.stitch_plan_g_flag_counts.restype, L.stitch_plan_g_flag_counts.argtypes = i32, [vp, vp]
        if hasattr(L, "stitch_plan_mask_row_counts"):  # include/stitch_mask_rows.h (likewise)
            L.stitch_plan_mask_row_counts.restype, L.stitch_plan_mask_row_counts.argtypes = i32, [vp, vp]
        if hasattr(L, "stitch_plan_index_counts"):  # include/stitch_index_plane.h (likewise)
            L.stitch_plan_index_counts.restype, L.stitch_plan_index_counts.argtypes = i32, [vp, vp]
        if hasattr(L, "stitch_plan_mask_keep_counts"):  # include/stitch_mask_keep.h (likewise)
            L.stitch_plan_mask_keep_counts.restype, L.stitch_plan_mask_keep_counts.argtypes = i32, [vp, vp]
        # include/stitch_collapse_sides.h, stitch_src_runs.h, stitch_rig_crop.h, stitch_rig_formats.h, stitch_rig_formats_yuv.h, stitch_rig_monitor.h, stitch_seam_path.h, stitch_seam_anchor.h,
        # stitch_rig_exposure_temporal.h, stitch_rig_scale.h (likewise)
        for name, (res, args) in list(COLLAPSE_SIDES_SIGNATURES.items()) + list(SRC_RUNS_SIGNATURES.items()) + list(RIG_CROP_SIGNATURES.items()) + list(RIG_EXPOSURE_TEMPORAL_SIGNATURES.items()) \
                + list(RIG_FORMAT_SIGNATURES.items()) + list(RIG_FORMAT_YUV_SIGNATURES.items()) + list(RIG_MONITOR_SIGNATURES.items()) + list(SEAM_PATH_SIGNATURES.items()) + list(SEAM_ANCHOR_SIGNATURES.items()) + list(RIG_SCALE_SIGNATURES.items()):
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def _chk(rc):
    if rc < 0:
        raise StitchError(rc, lib().stitch_last_error().decode())
    return rc


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _fn(stem, a):
    """The _u8 / _f32 twin of the entry points `stem` for the pixel type of `a`, a numpy array or a torch tensor."""
    sfx = {"uint8": "u8", "float32": "f32"}.get(str(a.dtype).rpartition(".")[2])  # "uint8" / "torch.uint8"
    if sfx is None:
        raise TypeError(f"unsupported pixel type {a.dtype}")
    return getattr(lib(), stem + sfx)


def _img(a):
    a = np.ascontiguousarray(a)
    if a.ndim != 3 or a.shape[0] != 3:
        raise ValueError(f"expected a (3,H,W) planar image, got {a.shape}")
    return a


def _map8(p):
    p = [float(v) for v in p]
    if len(p) != 8:
        raise ValueError("the bilinear map has 8 parameters {H00,H01,H02,H10,H11,H12,H20,H21}")
    return (C.c_double * 8)(*p)


def _opts(opts):
    if opts is None:
        return BlendOpts()
    if isinstance(opts, BlendOpts):
        return opts
    return BlendOpts(**opts)


def _seam_array(seams):
    """Seams as the library takes them, by their four integers: Seam records, or tuples whose first four entries are
    (sum_a_x, n_a, sum_ov_x, n_ov) -- Seam.as_tuple() and the records of a step dict qualify."""
    seams = list(seams)
    arr = (Seam * max(len(seams), 1))()
    for d, sm in zip(arr, seams):
        v = sm.as_tuple() if isinstance(sm, Seam) else tuple(sm)
        d.sum_a_x, d.n_a, d.sum_ov_x, d.n_ov = (int(x) for x in v[:4])
    return arr


def seam_from_sums(sum_a_x, n_a, sum_ov_x, n_ov, seam_rule, cw):
    """stitch_seam_from_sums (host only): the Seam the scan derives from these four integers under seam_rule on a canvas cw wide;
    raises StitchError(ERR_ARG) for integers no middle row of cw columns can give."""
    s = Seam()
    _chk(lib().stitch_seam_from_sums(int(sum_a_x), int(n_a), int(sum_ov_x), int(n_ov), int(seam_rule), int(cw), C.byref(s)))
    return s


def device_count():
    return lib().stitch_device_count()


def plan_cache_query(cw, ch, opts=None):
    """(idle cached workspaces a host-buffer call for this canvas would take under the CURRENT environment's tuning
    switches, fused_sweep_levels of the first) -- stitch_plan_cache_query."""
    fused = C.c_int(-1)
    n = _chk(lib().stitch_plan_cache_query(int(cw), int(ch), C.byref(_opts(opts)), C.byref(fused)))
    return n, fused.value


def trim():
    lib().stitch_trim()


def pyramid_levels(w, h, level_rule=0):
    lw, lh = (C.c_int * 32)(), (C.c_int * 32)()
    n = _chk(lib().stitch_pyramid_levels(int(w), int(h), int(level_rule), lw, lh))
    return n, list(lw[:n]), list(lh[:n])


# ---- host-buffer entry points (numpy) ------------------------------------------------------------------------
def project(src, fov_deg=15.0):
    """Projection::imageProjection (Projection.cpp:20-73)."""
    src = _img(src)
    dst = np.empty_like(src)
    _, h, w = src.shape
    _chk(_fn("stitch_project_", src)(_p(src), w, h, fov_deg, _p(dst)))
    return dst


def warp(src, p, offx, offy, canvas):
    """ImageProcess::warpingImageByHomography (ImageProcess.cpp:596-606); writes into `canvas` in place."""
    src = _img(src)
    assert canvas.flags.c_contiguous and canvas.dtype == src.dtype and canvas.shape[0] == 3
    _chk(_fn("stitch_warp_", src)(_p(src), src.shape[2], src.shape[1], _map8(p), offx, offy, _p(canvas), canvas.shape[2], canvas.shape[1]))
    return canvas


def move(src, ox, oy, canvas):
    """ImageProcess::movingImageByOffset (ImageProcess.cpp:608-620); writes into `canvas` in place."""
    src = _img(src)
    assert canvas.flags.c_contiguous and canvas.dtype == src.dtype and canvas.shape[0] == 3
    _chk(_fn("stitch_move_", src)(_p(src), src.shape[2], src.shape[1], int(ox), int(oy), _p(canvas), canvas.shape[2], canvas.shape[1]))
    return canvas


def blend(a, b, opts=None):
    """ImageProcess::blendTwoImages (ImageProcess.cpp:648-773) -> (out, Seam)."""
    a, b = _img(a), _img(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    out, s = np.empty_like(a), Seam()
    _chk(_fn("stitch_blend_", a)(_p(a), _p(b), a.shape[2], a.shape[1], C.byref(_opts(opts)), _p(out), C.byref(s)))
    return out, s


def pair(frame, p, offx, offy, mosaic, ox, oy, cw, ch, opts=None):
    """One stitch step (ImageProcess.cpp:218-230): warp `frame`, move `mosaic`, blend -> (out, Seam)."""
    frame, mosaic = _img(frame), _img(mosaic)
    assert frame.dtype == mosaic.dtype
    out, s = np.empty((3, ch, cw), frame.dtype), Seam()
    _chk(_fn("stitch_pair_", frame)(_p(frame), frame.shape[2], frame.shape[1], _map8(p), offx, offy, _p(mosaic), mosaic.shape[2],
                                    mosaic.shape[1], int(ox), int(oy), int(cw), int(ch), C.byref(_opts(opts)), _p(out), C.byref(s)))
    return out, s


def equalize(img):
    """equalization::equalization(img, 1) (equalization.cpp:4-25,74-131) -> (equalised copy, 256 Y bins)."""
    img = np.array(_img(img), dtype=np.uint8, copy=True)
    hist = np.zeros(256, np.int32)
    _chk(lib().stitch_equalize_u8(_p(img), img.shape[2], img.shape[1], _p(hist)))
    return img, hist


def lummix(result, equalized, num=19.0, den=20.0):
    """Luminance mix of ImageProcess::matching (ImageProcess.cpp:240-268) -> new array."""
    result = np.array(_img(result), dtype=np.uint8, copy=True)
    equalized = np.ascontiguousarray(equalized, np.uint8)
    _chk(lib().stitch_lummix_u8(_p(result), _p(equalized), result.shape[2], result.shape[1], num, den))
    return result


def finish(result, num=19.0, den=20.0):
    """Tail of matching() in one call (ImageProcess.cpp:237-268): equalise a copy, mix -> (new array, Y bins)."""
    result = np.array(_img(result), dtype=np.uint8, copy=True)
    hist = np.zeros(256, np.int32)
    _chk(lib().stitch_finish_u8(_p(result), result.shape[2], result.shape[1], num, den, _p(hist)))
    return result, hist


def gray(rgb):
    """ImageProcess::toGrayScale + SIFT float staging (ImageProcess.cpp:27-40,47-51) -> (gray uint8 (H,W), float32 (H,W))."""
    rgb = np.ascontiguousarray(_img(rgb), np.uint8)
    _, h, w = rgb.shape
    g, f = np.empty((h, w), np.uint8), np.empty((h, w), np.float32)
    _chk(lib().stitch_gray_u8(_p(rgb), w, h, _p(g), _p(f)))
    return g, f


def project_gray(src, fov_deg=15.0):
    """readFile's per-image chain in one kernel (ImageProcess.cpp:18-20) -> (projected, gray, gray_f32)."""
    src = np.ascontiguousarray(_img(src), np.uint8)
    _, h, w = src.shape
    dst, g, f = np.empty_like(src), np.empty((h, w), np.uint8), np.empty((h, w), np.float32)
    _chk(lib().stitch_project_gray_u8(_p(src), w, h, fov_deg, _p(dst), _p(g), _p(f)))
    return dst, g, f


def transfer(src, tem):
    """transfer::transfer (transfer.cpp:3-13,125-225): l-alpha-beta colour transfer of tem's statistics onto src
    -> (out (3,H,W) uint8, stats float32[12] = mean/sd of src, mean/sd of tem)."""
    src, tem = np.ascontiguousarray(_img(src), np.uint8), np.ascontiguousarray(_img(tem), np.uint8)
    out, st = np.empty_like(src), np.zeros(12, np.float32)
    _chk(lib().stitch_transfer_u8(_p(src), src.shape[2], src.shape[1], _p(tem), tem.shape[2], tem.shape[1], _p(out), _p(st)))
    return out, st


def dev_transfer(d_src, d_tem, out=None, stats=None, stats_form=0, keep_black=False, diag=None):
    """Device-resident colour transfer; out may be d_src itself.  stats_form 1 / 2 form the statistics by scan (the same bits,
    include/stitch_exposure.h), keep_black leaves (0,0,0) source pixels black; diag: optional (6, 4) int32 tensor for the
    scan's counters.  The defaults are stitch_dev_transfer_u8 itself."""
    import torch
    for t in (d_src, d_tem):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape[0] == 3
    out = torch.empty_like(d_src) if out is None else out
    if stats_form == 0 and not keep_black and diag is None:
        _chk(lib().stitch_dev_transfer_u8(_dp(d_src), d_src.shape[2], d_src.shape[1], _dp(d_tem), d_tem.shape[2], d_tem.shape[1], _dp(out),
                                          _dp(stats), _stream()))
    else:
        _chk(lib().stitch_dev_transfer_form_u8(_dp(d_src), d_src.shape[2], d_src.shape[1], _dp(d_tem), d_tem.shape[2], d_tem.shape[1], _dp(out),
                                               _dp(stats), int(stats_form), int(bool(keep_black)), _dp(diag), _stream()))
    return out


STATS_DIAG = ("plain_adds", "spans_o1", "spans_redone", "tiles_serial")  # STITCH_STATS_DIAG counters per plane


def dev_running_stats(planes, form=2, counts=None, want_diag=False):
    """stitch_dev_running_stats_f32: mean and sd of 1 .. 6 float32 device tensors (each flattened, each with its own length) as
    transfer.cpp:128-164 accumulates them, float sums in index order; counts default to the lengths.  form 0: the serial walk,
    1: one workgroup's scan, 2: spans + walk -- the same bits.  Returns (mean, sd) device tensors, with want_diag also an
    (n, 4) int32 tensor of STATS_DIAG counters.  Enqueued on torch's current stream."""
    import torch
    planes = [p.reshape(-1) for p in planes]
    for p in planes:
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError("expected contiguous float32 tensors on the HIP device")
    n = len(planes)
    ptrs = (C.c_void_p * max(n, 1))(*[p.data_ptr() for p in planes])
    lens = (C.c_size_t * max(n, 1))(*[p.numel() for p in planes])
    cnts = (C.c_float * max(n, 1))(*[float(p.numel()) if counts is None else float(counts[i]) for i, p in enumerate(planes)])
    dev = planes[0].device if planes else None
    mean, sd = torch.zeros(max(n, 1), dtype=torch.float32, device=dev), torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
    diag = torch.zeros((max(n, 1), len(STATS_DIAG)), dtype=torch.int32, device=dev) if want_diag else None
    _chk(lib().stitch_dev_running_stats_f32(ptrs, lens, cnts, n, int(form), _dp(mean), _dp(sd), _dp(diag), _stream()))
    return (mean, sd, diag) if want_diag else (mean, sd)


class BmpInfo(C.Structure):
    """stitch_bmp_info: what CImg's loader derives from the 54-byte header (CImg.h:48413-48441)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bpp", C.c_int32), ("top_down", C.c_int32),
                ("data_pos", C.c_uint64), ("stride", C.c_uint64), ("data_bytes", C.c_uint64)]


def bmp_parse(header, file_bytes):
    """Header arithmetic of CImg's load_bmp on the first 54 bytes of a file of `file_bytes` bytes.  Host only."""
    h = np.frombuffer(bytes(header[:54]), np.uint8)
    bi = BmpInfo()
    _chk(lib().stitch_bmp_parse(_p(h), int(file_bytes) if h.size >= 54 else h.size, C.byref(bi)))
    return bi


def bmp_decode(data):
    """Bytes of a 24/32-bit BMP file -> planar (3,H,W) uint8 RGB, as CImg<unsigned char>::load_bmp gives it."""
    buf = np.frombuffer(bytes(data), np.uint8)
    bi = bmp_parse(buf[:54].tobytes(), buf.size)
    out = np.empty((3, bi.height, bi.width), np.uint8)
    _chk(lib().stitch_bmp_decode_u8(_p(buf), buf.size, _p(out)))
    return out


def bmp_encode(img):
    """Planar (3,H,W) uint8 RGB -> the bytes CImg<unsigned char>::save_bmp writes."""
    img = np.ascontiguousarray(_img(img), np.uint8)
    _, h, w = img.shape
    n = lib().stitch_bmp_file_bytes(w, h)
    out = np.empty(n, np.uint8)
    _chk(lib().stitch_bmp_encode_u8(_p(img), w, h, _p(out), n))
    return out.tobytes()


def dev_bmp_decode(d_file, info, out=None):
    """Device-resident file image (1-D uint8 tensor) -> planar (3,H,W) uint8 tensor; `info` from bmp_parse."""
    import torch
    assert d_file.is_cuda and d_file.dtype == torch.uint8 and d_file.is_contiguous()
    out = torch.empty((3, info.height, info.width), dtype=torch.uint8, device=d_file.device) if out is None else out
    _chk(lib().stitch_dev_bmp_decode_u8(_dp(d_file), d_file.numel(), C.byref(info), _dp(out), _stream()))
    return out


def dev_bmp_encode(d_img, out=None):
    """Planar (3,H,W) uint8 tensor -> device-resident file image (1-D uint8 tensor), byte-identical to save_bmp."""
    import torch
    assert d_img.is_cuda and d_img.dtype == torch.uint8 and d_img.is_contiguous() and d_img.shape[0] == 3
    _, h, w = d_img.shape
    n = lib().stitch_bmp_file_bytes(int(w), int(h))
    out = torch.empty(n, dtype=torch.uint8, device=d_img.device) if out is None else out
    _chk(lib().stitch_dev_bmp_encode_u8(_dp(d_img), int(w), int(h), _dp(out), out.numel(), _stream()))
    return out


def canvas_bbox(fw, fh, p_fwd, result_w, result_h):
    """Canvas of one stitch step (ImageProcess.cpp:206-216) -> (min_x, min_y, new_w, new_h).  Host arithmetic."""
    mx, my, nw, nh = C.c_float(), C.c_float(), C.c_int(), C.c_int()
    _chk(lib().stitch_canvas_bbox(int(fw), int(fh), _map8(p_fwd), int(result_w), int(result_h), C.byref(mx), C.byref(my),
                                  C.byref(nw), C.byref(nh)))
    return mx.value, my.value, nw.value, nh.value


class StepGeom(C.Structure):
    """stitch_step_geom: canvas and offsets of one stitch step (ImageProcess.cpp:206-216, :224)."""
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("cw", C.c_int), ("ch", C.c_int), ("ox", C.c_int), ("oy", C.c_int)]


def step_geometry(fw, fh, p_fwd, mw, mh):
    g = StepGeom()
    _chk(lib().stitch_step_geometry(int(fw), int(fh), _map8(p_fwd), int(mw), int(mh), C.byref(g)))
    return g


def dev_step(frame, p_fwd, p_bwd, mosaic, opts=None):
    """One stitch step of matching() from the FORWARD map, device resident (ImageProcess.cpp:206-230): canvas sizing,
    warp, move, blend -> (new mosaic tensor, StepGeom, Seam)."""
    import torch
    frame, mosaic = _timg(frame), _timg(mosaic)
    g = step_geometry(frame.shape[2], frame.shape[1], p_fwd, mosaic.shape[2], mosaic.shape[1])
    out = torch.empty((3, g.ch, g.cw), dtype=frame.dtype, device=frame.device)
    g2, s = StepGeom(), Seam()
    _chk(_fn("stitch_dev_step_", frame)(_dp(frame), frame.shape[2], frame.shape[1], _map8(p_fwd), _map8(p_bwd), _dp(mosaic), mosaic.shape[2],
                                        mosaic.shape[1], C.byref(_opts(opts)), _dp(out), out.numel(), C.byref(g2), C.byref(s), _stream()))
    return out, g2, s


def map_points(x, y, p_fwd, offx, offy):
    """updateFeaturesByHomography (ImageProcess.cpp:622-631) -> (x, y, ix, iy)."""
    x, y = np.array(x, np.float32), np.array(y, np.float32)
    ix, iy = np.empty(x.size, np.int32), np.empty(x.size, np.int32)
    _chk(lib().stitch_map_points(_p(x), _p(y), _p(ix), _p(iy), x.size, _map8(p_fwd), offx, offy))
    return x, y, ix, iy


def shift_points(x, y, ox, oy):
    """updateFeaturesByOffset (ImageProcess.cpp:633-640) -> (x, y, ix, iy)."""
    x, y = np.array(x, np.float32), np.array(y, np.float32)
    ix, iy = np.empty(x.size, np.int32), np.empty(x.size, np.int32)
    _chk(lib().stitch_shift_points(_p(x), _p(y), _p(ix), _p(iy), x.size, int(ox), int(oy)))
    return x, y, ix, iy


def dev_map_points(x, y, p_fwd, offx, offy, want_int=True):
    """map_points on float32 device tensors, IN PLACE, on torch's current stream (no synchronisation) -> (x, y, ix, iy); ix / iy
    are new int32 tensors (None without want_int)."""
    import torch
    x, y = _tvec(x, torch.float32, "x"), _tvec(y, torch.float32, "y")
    if x.numel() != y.numel():
        raise ValueError("x and y differ in length")
    ix, iy = (torch.empty(x.numel(), dtype=torch.int32, device=x.device) for _ in range(2)) if want_int else (None, None)
    _chk(lib().stitch_dev_map_points(_dp(x), _dp(y), _dp(ix), _dp(iy), x.numel(), _map8(p_fwd), offx, offy, _stream()))
    return x, y, ix, iy


def dev_shift_points(x, y, ox, oy, want_int=True):
    """shift_points on float32 device tensors, IN PLACE, on torch's current stream -> (x, y, ix, iy)."""
    import torch
    x, y = _tvec(x, torch.float32, "x"), _tvec(y, torch.float32, "y")
    if x.numel() != y.numel():
        raise ValueError("x and y differ in length")
    ix, iy = (torch.empty(x.numel(), dtype=torch.int32, device=x.device) for _ in range(2)) if want_int else (None, None)
    _chk(lib().stitch_dev_shift_points(_dp(x), _dp(y), _dp(ix), _dp(iy), x.numel(), int(ox), int(oy), _stream()))
    return x, y, ix, iy


# ---- descriptor matching: ImageProcess::getImgPair (ImageProcess.cpp:273-351) -----------------------------------------------
DESCRIPTOR_DIM = 128  # STITCH_DESCRIPTOR_DIM (DESCRIPTOR_SUM, ImageProcess.h:20)
RATIO_THRESHOLD = 0.5  # ImageProcess.h:22


class MatchDesc(C.Structure):
    """stitch_match_desc: one (data, query) set of a batched match (device pointers)."""
    _fields_ = [("db", C.c_void_p), ("query", C.c_void_p), ("n_db", C.c_int32), ("n_query", C.c_int32), ("nn", C.c_void_p),
                ("dist2", C.c_void_p), ("pairs", C.c_void_p), ("count", C.c_void_p)]


def _desc_rows(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != DESCRIPTOR_DIM:
        raise ValueError(f"expected (n, {DESCRIPTOR_DIM}) float32 descriptors, got {a.shape}")
    return a


def match(db, query, ratio=RATIO_THRESHOLD):
    """Exact L1 two-nearest-neighbour search of every `query` row among the `db` rows with the ratio test of getImgPair.
    Returns (pairs, nn, d0, d1): pairs (count, 2) int32 of (db index, query index) in query order; per query the index of
    the nearest row (-1 without data) and the two smallest distances (NaN where there is no such neighbour)."""
    db, query = _desc_rows(db), _desc_rows(query)
    nq = query.shape[0]
    nn = np.empty(nq, np.int32)
    dist2 = np.empty((nq, 2), np.float32)
    pairs = np.empty((max(nq, 1), 2), np.int32)
    count = C.c_int32(0)
    _chk(lib().stitch_match_l1_ratio(_p(db), db.shape[0], _p(query), nq, ratio, _p(nn), _p(dist2), _p(pairs), C.byref(count)))
    return pairs[:count.value].copy(), nn, dist2[:, 0].copy(), dist2[:, 1].copy()


def _tdesc(t):
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == DESCRIPTOR_DIM):
        raise ValueError(f"expected a contiguous (n, {DESCRIPTOR_DIM}) float32 device tensor, got {tuple(t.shape)} {t.dtype}")
    return t


def _match_outputs(db, query, want_dist=True):
    import torch
    nq, dev = query.shape[0], query.device
    return dict(pairs=torch.empty((max(nq, 1), 2), dtype=torch.int32, device=dev), count=torch.zeros(1, dtype=torch.int32, device=dev),
                nn=torch.empty(nq, dtype=torch.int32, device=dev),
                dist2=torch.empty((nq, 2), dtype=torch.float32, device=dev) if want_dist else None)


def _mdesc(db, query, o):
    return MatchDesc(_dp(db), _dp(query), db.shape[0], query.shape[0], _dp(o["nn"]), _dp(o["dist2"]), _dp(o["pairs"]), _dp(o["count"]))


def dev_match(db, query, ratio=RATIO_THRESHOLD, want_dist=True):
    """match() on device tensors, enqueued on torch's current stream (no synchronisation).  Returns a dict of device
    tensors: pairs ((n_query, 2) int32, the first `count` rows valid), count ((1,) int32), nn, dist2 ((n_query, 2) or None)."""
    db, query = _tdesc(db), _tdesc(query)
    o = _match_outputs(db, query, want_dist)
    d = _mdesc(db, query, o)
    _chk(lib().stitch_dev_match_l1_ratio(d.db, d.n_db, d.query, d.n_query, ratio, d.nn, d.dist2, d.pairs, d.count, _stream()))
    return o


def dev_match_many(sets, ratio=RATIO_THRESHOLD, want_dist=True):
    """Many (db, query) pairs of device tensors in one launch sequence; returns one dict per set as dev_match does."""
    sets = [(_tdesc(a), _tdesc(b)) for a, b in sets]
    outs = [_match_outputs(a, b, want_dist) for a, b in sets]
    arr = (MatchDesc * max(len(sets), 1))(*[_mdesc(a, b, o) for (a, b), o in zip(sets, outs)])
    _chk(lib().stitch_dev_match_l1_ratio_many(arr, len(sets), ratio, _stream()))
    return outs

# ---- map estimation: ImageProcess::RANSAC (ImageProcess.cpp:395-529) -----------------------------------------------------
RANSAC_ROUNDS, RANSAC_THRESHOLD, RANSAC_SEED, RANSAC_INFO = 72, 4.0, 666666, 5
RANSAC_OK, RANSAC_TOO_FEW, RANSAC_NO_CONSENSUS, RANSAC_DRAW_CAP = 0, 1, 2, 3


class RansacOpts(C.Structure):
    """stitch_ransac_opts; the defaults are the reference's values."""
    _fields_ = [("rounds", C.c_int32), ("threshold", C.c_float), ("seed", C.c_uint32), ("max_draws", C.c_int32)]

    def __init__(self, rounds=0, threshold=RANSAC_THRESHOLD, seed=RANSAC_SEED, max_draws=0):
        super().__init__(int(rounds), float(threshold), int(seed), int(max_draws))


class RansacDesc(C.Structure):
    """stitch_ransac_desc: one list of a batched estimation (device pointers)."""
    _fields_ = [("src_x", C.c_void_p), ("src_y", C.c_void_p), ("dst_x", C.c_void_p), ("dst_y", C.c_void_p), ("pairs", C.c_void_p),
                ("count", C.c_void_p), ("n_max", C.c_int32), ("mirror", C.c_int32), ("p", C.c_void_p), ("inliers", C.c_void_p),
                ("info", C.c_void_p)]


def ransac_rand(n, seed=RANSAC_SEED):
    """The first n values of rand() after srand(seed) as the library generates them (host hook) -> int32 array."""
    out = np.empty(int(n), np.int32)
    lib().stitch_ransac_rand(int(seed), _p(out), int(n))
    return out


def ransac(src_x, src_y, dst_x, dst_y, mirror=False, opts=None):
    """ImageProcess::RANSAC on one list of pairs (src point i, dst point i) given as host arrays.  Returns (p, inliers, info):
    the 8 doubles of the map src -> dst (NaN when info[0] != RANSAC_OK), the winning inlier indices in increasing order, and
    info = [status, n, winning round, winning count, rand() values consumed]."""
    a = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (src_x, src_y, dst_x, dst_y)]
    n = a[0].size
    if any(v.size != n for v in a):
        raise ValueError("the four coordinate arrays differ in length")
    p, inl, info = np.empty(8, np.float64), np.empty(max(n, 1), np.int32), np.empty(RANSAC_INFO, np.int32)
    o = opts if opts is not None else RansacOpts()
    _chk(lib().stitch_ransac(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), n, int(bool(mirror)), C.byref(o), _p(p), _p(inl), _p(info)))
    return p, inl[:max(int(info[3]), 0)].copy(), info


def _tvec(t, dtype, what):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"expected a contiguous {dtype} device tensor for {what}")
    return t


def dev_ransac_many(lists, opts=None, want_inliers=True):
    """Many lists in one launch sequence on torch's current stream (no synchronisation).  Each entry is a dict of device
    tensors: src_x, src_y, dst_x, dst_y (float32 keypoint coordinates of the two frames) and optionally pairs ((n_max, 2)
    int32 of (src row, dst row), e.g. dev_match's output), count ((1,) int32) and mirror (bool).  Without pairs, pair i is
    (src i, dst i).  Returns (p, info, inliers): (n, 8) float64, (n, 5) int32, and a list of int32 tensors (the winning indices,
    then -1) or None."""
    import torch
    n = len(lists)
    dev = lists[0]["src_x"].device if n else torch.device("cuda", torch.cuda.current_device())
    p = torch.empty((n, 8), dtype=torch.float64, device=dev)
    info = torch.empty((n, RANSAC_INFO), dtype=torch.int32, device=dev)
    descs, inl = [], []
    for i, e in enumerate(lists):
        xy = [_tvec(e[k], torch.float32, k) for k in ("src_x", "src_y", "dst_x", "dst_y")]
        pairs, count = e.get("pairs"), e.get("count")
        if pairs is not None:
            n_max = _tvec(pairs, torch.int32, "pairs").numel() // 2
        else:
            n_max = min(v.numel() for v in xy)
        if count is not None:
            _tvec(count, torch.int32, "count")
        inl.append(torch.empty(n_max, dtype=torch.int32, device=dev) if want_inliers else None)
        descs.append(RansacDesc(_dp(xy[0]), _dp(xy[1]), _dp(xy[2]), _dp(xy[3]), _dp(pairs), _dp(count), n_max, int(bool(e.get("mirror", False))),
                                p.data_ptr() + 64 * i, _dp(inl[-1]), info.data_ptr() + 4 * RANSAC_INFO * i))
    arr = (RansacDesc * max(n, 1))(*descs)
    o = opts if opts is not None else RansacOpts()
    _chk(lib().stitch_dev_ransac_many(arr, n, C.byref(o), _stream()))
    return p, info, (inl if want_inliers else None)


# ---- SIFT: ImageProcess::siftAlgorithm (ImageProcess.cpp:44-99) over vl/sift.c --------------------------------------------
SIFT_OK, SIFT_OVERFLOW, SIFT_STATUS = 0, 1, 4
SIFT_KP_DTYPE = np.dtype([("o", "<i4"), ("ix", "<i4"), ("iy", "<i4"), ("is", "<i4"), ("x", "<f4"), ("y", "<f4"), ("s", "<f4"),
                          ("sigma", "<f4")])  # StitchSiftKeypoint = VlSiftKeypoint after vl_sift_detect


class SiftOpts(C.Structure):
    """StitchSiftOpts; the defaults are the reference's values (octaves < 0: VLFeat's automatic rule)."""
    _fields_ = [("octaves", C.c_int32), ("levels", C.c_int32), ("first_octave", C.c_int32), ("peak_thresh", C.c_double),
                ("edge_thresh", C.c_double), ("norm_thresh", C.c_double), ("magnif", C.c_double), ("window_size", C.c_double)]

    def __init__(self, octaves=4, levels=2, first_octave=0, peak_thresh=0.0, edge_thresh=10.0, norm_thresh=0.0, magnif=3.0,
                 window_size=2.0):
        super().__init__(int(octaves), int(levels), int(first_octave), float(peak_thresh), float(edge_thresh), float(norm_thresh),
                         float(magnif), float(window_size))


class SiftDesc(C.Structure):
    """stitch_sift_desc: one frame of a batched extraction (device pointers)."""
    _fields_ = [("image", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32), ("is_f32", C.c_int32),
                ("keypoints", C.c_void_p), ("kp_cap", C.c_int32), ("feat_cap", C.c_int32), ("feat_kp", C.c_void_p),
                ("feat_angle", C.c_void_p), ("feat_desc", C.c_void_p), ("counts", C.c_void_p), ("status", C.c_void_p)]


def sift(gray, opts=None, kp_cap=8192, feat_cap=None):
    """siftAlgorithm's VLFeat sequence on one (H, W) uint8 gray image given as a host array.  Returns a dict: kp (SIFT_KP_DTYPE
    records in detection order), fkp (keypoint index per feature row), angle (float64), desc ((n, 128) float32, the reference's
    insertion order), status ([status, keypoints found, rows found, octaves run]).  status[0] == SIFT_OVERFLOW: the capacities
    were too small, status[1:3] say what is needed."""
    g = np.ascontiguousarray(gray, dtype=np.uint8)
    if g.ndim != 2:
        raise ValueError("expected an (H, W) gray image")
    feat_cap = 2 * kp_cap if feat_cap is None else feat_cap
    kp = np.zeros(max(kp_cap, 1), SIFT_KP_DTYPE)
    fkp, ang = np.zeros(max(feat_cap, 1), np.int32), np.zeros(max(feat_cap, 1), np.float64)
    desc = np.zeros((max(feat_cap, 1), DESCRIPTOR_DIM), np.float32)
    counts, status = np.zeros(2, np.int32), np.zeros(SIFT_STATUS, np.int32)
    o = opts if opts is not None else SiftOpts()
    _chk(lib().stitch_sift(_p(g), g.shape[1], g.shape[0], C.byref(o), _p(kp), int(kp_cap), _p(fkp), _p(ang), _p(desc), int(feat_cap), _p(counts),
                           _p(status)))
    nk, nf = int(counts[0]), int(counts[1])
    return dict(kp=kp[:nk].copy(), fkp=fkp[:nf].copy(), angle=ang[:nf].copy(), desc=desc[:nf].copy(), status=status)


def dev_sift_many(images, opts=None, kp_cap=8192, feat_cap=None, slack=0, fill=None):
    """Many gray frames -- (H, W) uint8 or float32 device tensors with contiguous rows, sizes may differ -- in one launch sequence
    per 16 frames and octave on torch's current stream (no synchronisation).  kp_cap and feat_cap (default 2 * kp_cap) are one
    number for every frame or a sequence with one per frame.  Returns a list of dicts of device tensors: kp ((kp_cap, 8) int32:
    the StitchSiftKeypoint records, columns 4..7 are float32 bits), fkp, angle, desc, counts ((2,) int32) and status ((4,)
    int32); sift_unpack turns one into host arrays.  The buffers are `slack` records longer than the capacities and, with `fill`,
    hold that byte everywhere before the call (for tests: nothing may be written at or beyond a capacity)."""
    import torch
    n = len(images)
    kcaps = [int(k) for k in kp_cap] if hasattr(kp_cap, "__len__") else [int(kp_cap)] * n
    fcaps = [2 * k for k in kcaps] if feat_cap is None else [int(k) for k in feat_cap] if hasattr(feat_cap, "__len__") else [int(feat_cap)] * n
    if len(kcaps) != n or len(fcaps) != n:
        raise ValueError("one capacity per frame")
    outs, descs = [], []
    for t, kc, fc in zip(images, kcaps, fcaps):
        if not (t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.dtype in (torch.uint8, torch.float32)):
            raise ValueError("expected (H, W) uint8 or float32 device tensors with contiguous rows")
        dev = t.device
        o = dict(kp=torch.empty((max(kc, 1) + slack, 8), dtype=torch.int32, device=dev),
                 fkp=torch.empty(max(fc, 1) + slack, dtype=torch.int32, device=dev),
                 angle=torch.empty(max(fc, 1) + slack, dtype=torch.float64, device=dev),
                 desc=torch.empty((max(fc, 1) + slack, DESCRIPTOR_DIM), dtype=torch.float32, device=dev),
                 head=torch.empty(2 + SIFT_STATUS, dtype=torch.int32, device=dev))
        if fill is not None:
            for k in ("kp", "fkp", "angle", "desc"):
                o[k].view(torch.uint8).fill_(int(fill))
        o["counts"], o["status"] = o["head"][:2], o["head"][2:]
        outs.append(o)
        descs.append(SiftDesc(_dp(t), t.shape[1], t.shape[0], t.stride(0) * t.element_size(), int(t.dtype == torch.float32),
                              _dp(o["kp"]), kc, fc, _dp(o["fkp"]), _dp(o["angle"]), _dp(o["desc"]),
                              _dp(o["head"]), o["head"].data_ptr() + 8))
    arr = (SiftDesc * max(n, 1))(*descs)
    op = opts if opts is not None else SiftOpts()
    _chk(lib().stitch_dev_sift_many(arr, n, C.byref(op), _stream()))
    return outs


def sift_unpack(out):
    """One entry of dev_sift_many as host arrays (this waits for the stream): the dict capi.sift returns."""
    head = out["head"].cpu().numpy()
    nk, nf = int(head[0]), int(head[1])
    kp = out["kp"][:nk].cpu().numpy().view(SIFT_KP_DTYPE).reshape(-1)
    return dict(kp=kp, fkp=out["fkp"][:nf].cpu().numpy(), angle=out["angle"][:nf].cpu().numpy(), desc=out["desc"][:nf].cpu().numpy(),
                status=head[2:].copy())


# ---- the whole panorama: include/stitch_panorama.h ------------------------------------------------------------------------
class FeatureSet(C.Structure):
    """stitch_feature_set: one frame's features in map order (device pointers)."""
    _fields_ = [("d_desc", C.c_void_p), ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("n", C.c_int32)]


class FrameU8(C.Structure):
    """stitch_frame_u8: one planar (3, height, width) frame, not projected."""
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class PanoramaOpts(C.Structure):
    """stitch_panorama_opts; the defaults are stitch_panorama_opts_default's (the reference's values)."""
    _fields_ = [("blend", C.c_void_p), ("sift", C.c_void_p), ("ransac", C.c_void_p), ("ratio", C.c_double), ("match_threshold", C.c_int32),
                ("fov_deg", C.c_float), ("kp_cap", C.c_int32), ("feat_cap", C.c_int32), ("finish", C.c_int32), ("num", C.c_double),
                ("den", C.c_double), ("keep_steps", C.c_int32)]


class PanoramaStep(C.Structure):
    """stitch_panorama_step: what one stitch step used and produced."""
    _fields_ = [("src", C.c_int32), ("dst", C.c_int32), ("p_fwd", C.c_double * 8), ("p_bwd", C.c_double * 8), ("geom", StepGeom), ("seam", Seam),
                ("info", (C.c_int32 * RANSAC_INFO) * 2)]


def feature_order_c(descriptors):
    """stitch_feature_order: the index array of pipeline.feature_order, computed by the library's host code."""
    d = _desc_rows(descriptors)
    idx, kept = np.empty(max(d.shape[0], 1), np.int32), C.c_int(0)
    _chk(lib().stitch_feature_order(_p(d), d.shape[0], _p(idx), C.byref(kept)))
    return idx[:kept.value].copy()


def stitch_order_c(counts, threshold=20):
    """stitch_stitch_order: pipeline.stitch_order by the library's host code -> (start, [(src, dst), ...])."""
    c = np.ascontiguousarray(counts, dtype=np.int32)
    n = c.shape[0]
    if c.ndim != 2 or c.shape[1] != n:
        raise ValueError("expected a square matrix of counts")
    pairs, start, steps = np.zeros((max(n * (n - 1), 1), 2), np.int32), C.c_int(0), C.c_int(0)
    _chk(lib().stitch_stitch_order(_p(c), n, int(threshold), C.byref(start), _p(pairs), C.byref(steps)))
    return start.value, [(int(a), int(b)) for a, b in pairs[:steps.value]]


def _feature_set(desc, x, y):
    import torch
    desc, x, y = _tdesc(desc), _tvec(x, torch.float32, "x"), _tvec(y, torch.float32, "y")
    if not x.numel() == y.numel() == desc.shape[0]:
        raise ValueError("descriptors, x and y differ in length")
    return FeatureSet(_dp(desc), _dp(x), _dp(y), desc.shape[0])


def dev_pair_maps(src, dst, ratio=RATIO_THRESHOLD, opts=None):
    """pipeline.pair_maps without its read-back: src / dst are (descriptors (n, 128), x (n,), y (n,)) float32 device tensors in map
    order -- the frame in the mosaic and the frame to warp.  Both matcher calls, the longer-list rule and both estimations are
    enqueued on torch's current stream.  Returns device tensors (p (2, 8) float64: forward, backward; info (2, 5) int32)."""
    import torch
    a, b = _feature_set(*src), _feature_set(*dst)
    dev = src[0].device
    p = torch.empty((2, 8), dtype=torch.float64, device=dev)
    info = torch.empty((2, RANSAC_INFO), dtype=torch.int32, device=dev)
    o = opts if opts is not None else RansacOpts()
    _chk(lib().stitch_dev_pair_maps(C.byref(a), C.byref(b), float(ratio), C.byref(o), _dp(p), _dp(info), _stream()))
    return p, info


def _panorama_opts(opts, finish, num, den, sift_opts, ransac_opts, kp_cap, feat_cap, keep_steps, ratio, match_threshold, fov_deg, keep):
    o = PanoramaOpts()
    lib().stitch_panorama_opts_default(C.byref(o))
    for obj, field in ((_opts(opts) if opts is not None else None, "blend"), (sift_opts, "sift"), (ransac_opts, "ransac")):
        if obj is not None:
            keep.append(obj)  # the structure must outlive the call
            setattr(o, field, C.addressof(obj))
    o.ratio, o.match_threshold, o.fov_deg = float(ratio), int(match_threshold), float(fov_deg)
    o.kp_cap, o.feat_cap, o.finish, o.num, o.den = int(kp_cap), int(feat_cap or 0), int(bool(finish)), float(num), float(den)
    o.keep_steps = int(bool(keep_steps))
    return o


class ExposureOpts(C.Structure):
    """stitch_exposure_opts (include/stitch_exposure.h)."""
    _fields_ = [("mode", C.c_int32), ("stats_form", C.c_int32), ("keep_black", C.c_int32)]


def _exposure(exposure):
    """None / 0 -> None (the chain as it is); a mode 1 / 2 -> the library's defaults with that mode; a dict(mode=, stats_form=,
    keep_black=) or an ExposureOpts -> as given."""
    if exposure is None or (isinstance(exposure, int) and exposure == 0):
        return None
    if isinstance(exposure, ExposureOpts):
        return exposure
    o = ExposureOpts()
    lib().stitch_exposure_opts_default(C.byref(o))
    if isinstance(exposure, dict):
        for k, v in exposure.items():
            if k not in ("mode", "stats_form", "keep_black"):
                raise ValueError(f"exposure: unknown key {k!r}")
            setattr(o, k, int(v))
    else:
        o.mode = int(exposure)
    return o


def _panorama_result(h, device, return_steps, keep_steps, exposure=None, frame_sizes=None):
    """The handle's mosaic (and steps) as torch tensors / dicts shaped like pipeline.panorama_from_features's; destroys the handle."""
    import torch
    L = lib()
    try:
        w, ht, start, ns = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _chk(L.stitch_panorama_info(h, C.byref(w), C.byref(ht), C.byref(start), C.byref(ns)))
        final = torch.empty((3, ht.value, w.value), dtype=torch.uint8, device=device)
        _chk(L.stitch_panorama_copy(h, -1, _dp(final), final.numel(), 1, _stream()))
        steps = []
        for k in range(ns.value if return_steps else 0):
            s = PanoramaStep()
            _chk(L.stitch_panorama_step_at(h, k, C.byref(s)))
            g = s.geom
            out = None
            if keep_steps:
                out = torch.empty((3, g.ch, g.cw), dtype=torch.uint8, device=device)
                _chk(L.stitch_panorama_copy(h, k, _dp(out), out.numel(), 1, _stream()))
            steps.append(dict(start=start.value, src=s.dst, mosaic_src=s.src, p=np.array(s.p_bwd[:]), p_fwd=np.array(s.p_fwd[:]), offx=g.min_x, offy=g.min_y,
                              ox=g.ox, oy=g.oy, cw=g.cw, ch=g.ch, out=out, seam=s.seam.as_tuple(),
                              info=np.array([list(s.info[0]), list(s.info[1])], np.int64)))
            if exposure is not None and exposure.mode:
                st12 = np.zeros(12, np.float32)
                _chk(L.stitch_panorama_exposure_stats(h, k, _p(st12)))
                steps[-1]["exposure_stats"] = st12
                if keep_steps:
                    fw, fh = frame_sizes[s.dst]
                    steps[-1]["transferred"] = torch.empty((3, fh, fw), dtype=torch.uint8, device=device)
                    _chk(L.stitch_panorama_exposure_frame_copy(h, k, _dp(steps[-1]["transferred"]), 3 * fw * fh, 1, _stream()))
        torch.cuda.current_stream().synchronize()  # the copies have left the handle's buffers
    finally:
        L.stitch_panorama_destroy(h)
    return (final, steps) if return_steps else final


def _frames_u8(frames):
    import torch
    frames = [_timg(f) for f in frames]
    if any(f.dtype != torch.uint8 for f in frames):
        raise TypeError("expected uint8 frames")
    return frames, (FrameU8 * max(len(frames), 1))(*[FrameU8(_dp(f), f.shape[2], f.shape[1]) for f in frames])


def dev_panorama(frames, opts=None, finish=True, num=19.0, den=20.0, return_steps=False, keep_steps=False, sift_opts=None, ransac_opts=None,
                 kp_cap=4096, feat_cap=None, ratio=RATIO_THRESHOLD, match_threshold=20, fov_deg=15.0, exposure=None):
    """The whole of ImageProcess::ImageProcess plus matching() in ONE library call (stitch_dev_panorama_u8): frames is a list of
    (3, H, W) uint8 device tensors (unprojected).  Returns the mosaic as a tensor; with return_steps also a list of dicts with the
    keys of pipeline.panorama_from_features's steps ("src" is the warped frame; "out" the step's mosaic with keep_steps, else
    None).  Runs on torch's current stream and waits for it.  exposure (include/stitch_exposure.h): None is this chain; 1 / 2 or
    dict(mode=, stats_form=, keep_black=) recolours every frame before its step (stitch_dev_panorama_exposure_u8); the steps then
    also hold "exposure_stats" and, with keep_steps, "transferred"."""
    frames, arr = _frames_u8(frames)
    keep, h = [], C.c_void_p()
    o = _panorama_opts(opts, finish, num, den, sift_opts, ransac_opts, kp_cap, feat_cap, keep_steps, ratio, match_threshold, fov_deg, keep)
    if exposure is None:
        _chk(lib().stitch_dev_panorama_u8(arr, len(frames), C.byref(o), _stream(), C.byref(h)))
        return _panorama_result(h, frames[0].device, return_steps, keep_steps)
    e = _exposure(exposure)
    _chk(lib().stitch_dev_panorama_exposure_u8(arr, len(frames), C.byref(o), None if e is None else C.byref(e), _stream(), C.byref(h)))
    return _panorama_result(h, frames[0].device, return_steps, keep_steps, e, [(f.shape[2], f.shape[1]) for f in frames])


def dev_panorama_from_features(frames, features, opts=None, finish=True, num=19.0, den=20.0, return_steps=False, keep_steps=False,
                               ransac_opts=None, ratio=RATIO_THRESHOLD, match_threshold=20, fov_deg=15.0, exposure=None):
    """stitch_dev_panorama_from_features_u8: as dev_panorama, from the frames and per frame (descriptors (n, 128), x, y) float32
    device tensors in map order, which are left unchanged."""
    frames, arr = _frames_u8(frames)
    if len(features) != len(frames):
        raise ValueError("one feature set per frame")
    sets = (FeatureSet * max(len(frames), 1))(*[_feature_set(*f) for f in features])
    keep, h = [], C.c_void_p()
    o = _panorama_opts(opts, finish, num, den, None, ransac_opts, 4096, None, keep_steps, ratio, match_threshold, fov_deg, keep)
    if exposure is None:
        _chk(lib().stitch_dev_panorama_from_features_u8(arr, sets, len(frames), C.byref(o), _stream(), C.byref(h)))
        return _panorama_result(h, frames[0].device, return_steps, keep_steps)
    e = _exposure(exposure)
    _chk(lib().stitch_dev_panorama_exposure_from_features_u8(arr, sets, len(frames), C.byref(o), None if e is None else C.byref(e), _stream(), C.byref(h)))
    return _panorama_result(h, frames[0].device, return_steps, keep_steps, e, [(f.shape[2], f.shape[1]) for f in frames])


def panorama(frames, opts=None, finish=True, num=19.0, den=20.0, sift_opts=None, ransac_opts=None, kp_cap=4096, feat_cap=None,
             ratio=RATIO_THRESHOLD, match_threshold=20, fov_deg=15.0, exposure=None):
    """stitch_panorama_u8: the whole panorama from (3, H, W) uint8 HOST arrays -> the mosaic as a numpy array."""
    frames = [np.ascontiguousarray(_img(f), np.uint8) for f in frames]
    arr = (FrameU8 * max(len(frames), 1))(*[FrameU8(f.ctypes.data, f.shape[2], f.shape[1]) for f in frames])
    keep, h = [], C.c_void_p()
    o = _panorama_opts(opts, finish, num, den, sift_opts, ransac_opts, kp_cap, feat_cap, False, ratio, match_threshold, fov_deg, keep)
    L = lib()
    if exposure is None:
        _chk(L.stitch_panorama_u8(arr, len(frames), C.byref(o), C.byref(h)))
    else:
        e = _exposure(exposure)
        _chk(L.stitch_panorama_exposure_u8(arr, len(frames), C.byref(o), None if e is None else C.byref(e), C.byref(h)))
    try:
        w, ht = C.c_int(), C.c_int()
        _chk(L.stitch_panorama_info(h, C.byref(w), C.byref(ht), None, None))
        out = np.empty((3, ht.value, w.value), np.uint8)
        _chk(L.stitch_panorama_copy(h, -1, _p(out), out.nbytes, 0, None))
    finally:
        L.stitch_panorama_destroy(h)
    return out


# ---- device-resident entry points (torch tensors on the HIP device) --------------------------------------------
def _timg(t):
    if not t.is_cuda or not t.is_contiguous() or t.dim() != 3 or t.shape[0] != 3:
        raise ValueError("expected a contiguous (3,H,W) tensor on the HIP device")
    return t


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev_project(src, fov_deg=15.0, out=None):
    import torch
    src = _timg(src)
    out = torch.empty_like(src) if out is None else out
    _, h, w = src.shape
    _chk(_fn("stitch_dev_project_", src)(_dp(src), w, h, fov_deg, _dp(out), _stream()))
    return out


def dev_project_gray(src, fov_deg=15.0):
    """readFile's per-image chain on the device (ImageProcess.cpp:18-20) -> (projected (3,H,W), gray (H,W) uint8, gray float32)."""
    import torch
    src = _timg(src)
    if src.dtype != torch.uint8:
        raise TypeError("expected a uint8 frame")
    _, h, w = src.shape
    out = torch.empty_like(src)
    g = torch.empty((h, w), dtype=torch.uint8, device=src.device)
    f = torch.empty((h, w), dtype=torch.float32, device=src.device)
    _chk(lib().stitch_dev_project_gray_u8(_dp(src), w, h, fov_deg, _dp(out), _dp(g), _dp(f), _stream()))
    return out, g, f


def dev_warp(src, p, offx, offy, canvas):
    src, canvas = _timg(src), _timg(canvas)
    _chk(_fn("stitch_dev_warp_", src)(_dp(src), src.shape[2], src.shape[1], _map8(p), offx, offy, _dp(canvas), canvas.shape[2], canvas.shape[1],
                                      _stream()))
    return canvas


def dev_move(src, ox, oy, canvas):
    src, canvas = _timg(src), _timg(canvas)
    _chk(_fn("stitch_dev_move_", src)(_dp(src), src.shape[2], src.shape[1], int(ox), int(oy), _dp(canvas), canvas.shape[2], canvas.shape[1],
                                      _stream()))
    return canvas


def dev_equalize(img, hist=None):
    """In place on a uint8 device tensor; `hist` (int32[256] device tensor, optional) receives the Y bins."""
    img = _timg(img)
    _chk(lib().stitch_dev_equalize_u8(_dp(img), img.shape[2], img.shape[1], _dp(hist), _stream()))
    return img


def dev_lummix(result, equalized, num=19.0, den=20.0):
    result, equalized = _timg(result), _timg(equalized)
    _chk(lib().stitch_dev_lummix_u8(_dp(result), _dp(equalized), result.shape[2], result.shape[1], num, den, _stream()))
    return result


def dev_finish(result, num=19.0, den=20.0, hist=None):
    result = _timg(result)
    _chk(lib().stitch_dev_finish_u8(_dp(result), result.shape[2], result.shape[1], num, den, _dp(hist), _stream()))
    return result


def dev_synth(w, h, frame_id, dtype, device=None):
    """Synthetic benchmark frame generated on the device -> (3,h,w) tensor."""
    import torch
    out = torch.empty((3, h, w), dtype=dtype, device=device or torch.device("cuda", torch.cuda.current_device()))
    _chk(_fn("stitch_dev_synth_", out)(_dp(out), int(w), int(h), int(frame_id), _stream()))
    return out


def dev_check_fastdiv(w):
    """stitch_dev_check_fastdiv: (numerators tested, quotients that differ from the IEEE divide) for denominator w."""
    t, m = C.c_ulonglong(), C.c_ulonglong()
    _chk(lib().stitch_dev_check_fastdiv(w, C.byref(t), C.byref(m)))
    return t.value, m.value


def dev_check_collapse_taps(w, h, probe):
    """stitch_dev_check_collapse_taps: (samples compared, samples that differ between k_collapse4's per-lane taps and k_collapse)."""
    t, m = C.c_ulonglong(), C.c_ulonglong()
    _chk(lib().stitch_dev_check_collapse_taps(int(w), int(h), int(probe), C.byref(t), C.byref(m)))
    return t.value, m.value


def src_run_classes(p, offx, offy, fw, fh, cw, ch, px_bytes=4):
    """stitch_src_run_classes, on the host: -> ((outside, no patch, 1..64, general), classes as a (bands, tiles) uint8 array)."""
    import numpy as np
    m = (C.c_double * 8)(*[float(v) for v in p])
    n = (C.c_uint32 * 4)()
    cls = np.zeros(((int(ch) + 63) // 64, (int(cw) + 63) // 64), dtype=np.uint8)
    _chk(lib().stitch_src_run_classes(m, float(offx), float(offy), int(fw), int(fh), int(cw), int(ch), int(px_bytes), n, cls.ctypes.data_as(vp)))
    return tuple(int(v) for v in n), cls


def dev_check_collapse_sides(w, h, probe, branch, seam_x):
    """stitch_dev_check_collapse_sides: (samples compared, samples that differ between k_collapse4's one-sided forms and k_collapse,
    (a-only, b-only, both) column blocks of the k_collapse4 launch)."""
    t, m, n = C.c_ulonglong(), C.c_ulonglong(), (C.c_int * 3)()
    _chk(lib().stitch_dev_check_collapse_sides(int(w), int(h), int(probe), int(branch), int(seam_x), C.byref(t), C.byref(m), n))
    return t.value, m.value, tuple(int(v) for v in n)


def dev_quantize(src, out=None):
    """float mosaic -> unsigned char by truncation (CImg.h:11167-11182, behind ImageProcess.cpp:772)."""
    import torch
    assert src.is_cuda and src.is_contiguous() and src.dtype == torch.float32
    out = torch.empty(src.shape, dtype=torch.uint8, device=src.device) if out is None else out
    _chk(lib().stitch_dev_quantize_u8(_dp(src), _dp(out), src.numel(), _stream()))
    return out


class _Handle:
    """An object of the library behind an opaque pointer; `_destroy` names the function that releases it."""

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan(_Handle):
    """stitch_plan: the device workspace of one canvas size (pyramids, scratch, tables, seam record)."""
    _destroy = "stitch_plan_destroy"

    def __init__(self, cw, ch, opts=None, max_pairs=1, masked=False):
        """masked=True: stitch_plan_create_masked (include/stitch_seam_path.h), the workspace of pairs(paths=..., branches=...)."""
        self._h = C.c_void_p()
        self.cw, self.ch, self.max_pairs, self.masked = int(cw), int(ch), int(max_pairs), bool(masked)
        create = lib().stitch_plan_create_masked if masked else lib().stitch_plan_create_batched
        _chk(create(self.cw, self.ch, C.byref(_opts(opts)), self.max_pairs, C.byref(self._h)))
        lw, lh = (C.c_int * 32)(), (C.c_int * 32)()
        n = _chk(lib().stitch_plan_levels(self._h, lw, lh))
        self.level_w, self.level_h = list(lw[:n]), list(lh[:n])
        self.fused_sweep_levels = lib().stitch_plan_fused_sweep_levels(self._h)

    @property
    def levels(self):
        return len(self.level_w)

    @property
    def coarse_from(self):
        return lib().stitch_plan_coarse_from(self._h)

    @property
    def fast_paths(self):
        """stitch_plan_fast_paths as a set of names."""
        f = lib().stitch_plan_fast_paths(self._h)
        names = ("implicit_mask", "source_fused", "fused_sweep", "zero_tiles", "fused_decimate", "coarse_levels")
        return {n for i, n in enumerate(names) if f & (1 << i)}

    def call_forms(self, n_pairs=1):
        """stitch_plan_call_forms: the per-call forms ("source_fused", "fused_sweep") a call with n_pairs pairs runs."""
        f = lib().stitch_plan_call_forms(self._h, int(n_pairs))
        return {n for b, n in ((2, "source_fused"), (4, "fused_sweep")) if f & b}  # (and CALL_MASK_KEEP: mask_keep_form)

    @property
    def workspace_bytes(self):
        return lib().stitch_plan_workspace_bytes(self._h)

    def collapse_range(self, level):
        """stitch_plan_collapse_range: (xa, xb, per_lane_taps) of the collapse of `level`."""
        xa, xb, g = C.c_int(), C.c_int(), C.c_int()
        _chk(lib().stitch_plan_collapse_range(self._h, int(level), C.byref(xa), C.byref(xb), C.byref(g)))
        return xa.value, xb.value, g.value

    @property
    def workspace_base(self):
        return lib().stitch_plan_workspace_base(self._h) or 0

    def blend(self, a, b, out=None):
        import torch
        a, b = _timg(a), _timg(b)
        assert a.shape == b.shape == (3, self.ch, self.cw)
        out = torch.empty_like(a) if out is None else out
        _chk(_fn("stitch_dev_blend_", a)(self._h, _dp(a), _dp(b), _dp(out), _stream()))
        return out

    def pair(self, frame, p, offx, offy, mosaic, ox, oy, out=None, seam=None):
        """Enqueue warp+move+blend of one pair on torch's current stream; `out` is (3,ch,cw).  seam: as pairs' seams, one record."""
        import torch
        frame, mosaic = _timg(frame), _timg(mosaic)
        if out is None:
            out = torch.empty((3, self.ch, self.cw), dtype=frame.dtype, device=frame.device)
        if seam is not None:
            return self.pairs([(frame, p, offx, offy, mosaic, ox, oy, out)], seams=[seam])[0]
        _chk(_fn("stitch_dev_pair_", frame)(self._h, _dp(frame), frame.shape[2], frame.shape[1], _map8(p), offx, offy, _dp(mosaic),
                                            mosaic.shape[2], mosaic.shape[1], int(ox), int(oy), _dp(out), _stream()))
        return out

    def pairs(self, items, seams=None, paths=None, branches=None):
        """Enqueue n <= max_pairs independent pairs as ONE launch sequence.  items: iterable of
        (frame, p, offx, offy, mosaic, ox, oy, out[, out_u8]) with device tensors; out_u8 (float frames only) receives the
        mosaic as unsigned char as well.  seams (stitch_dev_pairs_seamed_*): one Seam or (sum_a_x, n_a, sum_ov_x, n_ov, ...) tuple
        per item, which replaces that pair's seam scan.  paths, branches (stitch_dev_pairs_pathed_*, a masked plan): per item a
        contiguous int32 device tensor of ch seam columns and its branch, 0 or 1; the blend cuts along them and no seam is scanned.
        Returns the list of `out` tensors."""
        items = list(items)
        if (paths is None) != (branches is None) or (paths is not None and seams is not None):
            raise ValueError("paths come with branches, and without seams")
        if paths is not None:
            import torch
            paths, branches = list(paths), [int(b) for b in branches]
            if len(paths) != len(items) or len(branches) != len(items):
                raise ValueError("one path and one branch per item")
            for t in paths:
                if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.int32 or tuple(t.shape) != (self.ch,):
                    raise ValueError(f"every path is a contiguous ({self.ch},) int32 device tensor")
        if seams is not None:
            seams = list(seams)
            if len(seams) != len(items):
                raise ValueError("one seam per item")
        arr = (PairDesc * len(items))()
        fn = None
        for d, it in zip(arr, items):
            frame, p, offx, offy, mosaic, ox, oy, out = it[:8]
            out8 = it[8] if len(it) > 8 else None
            frame, mosaic, out = _timg(frame), _timg(mosaic), _timg(out)
            assert tuple(out.shape) == (3, self.ch, self.cw) and out.dtype == frame.dtype == mosaic.dtype
            assert frame.dtype == items[0][0].dtype, "one pixel type per batch"
            fn = fn or _fn("stitch_dev_pairs_", frame)
            d.frame, d.fw, d.fh = frame.data_ptr(), frame.shape[2], frame.shape[1]
            d.p = _map8(p)
            d.offx, d.offy = float(offx), float(offy)
            d.mosaic, d.mw, d.mh = mosaic.data_ptr(), mosaic.shape[2], mosaic.shape[1]
            d.ox, d.oy, d.out = int(ox), int(oy), out.data_ptr()
            if out8 is not None:
                import torch
                assert out8.is_cuda and out8.is_contiguous() and out8.dtype == torch.uint8 and tuple(out8.shape) == (3, self.ch, self.cw)
                d.out_u8 = out8.data_ptr()
        if paths is not None:
            _chk(_fn("stitch_dev_pairs_pathed_", items[0][0])(self._h, arr, len(items), _ptr_table(paths), (C.c_int32 * len(items))(*branches), _stream()))
        elif seams is not None:
            _chk(_fn("stitch_dev_pairs_seamed_", items[0][0])(self._h, arr, len(items), _seam_array(seams), _stream()))
        else:
            _chk(fn(self._h, arr, len(items), _stream()))
        return [it[7] for it in items]

    def status(self, index=0):
        """Wait for the last call and return pair `index`'s Seam; raises StitchError for an empty mid row / zero
        overlap of that pair."""
        s = Seam()
        _chk(lib().stitch_plan_status_at(self._h, int(index), C.byref(s)))
        return s

    def clear_fault(self):
        """Acknowledge the fused sweep's sticky time-out report (stitch_plan_clear_fault)."""
        _chk(lib().stitch_plan_clear_fault(self._h))

    def handoff_counts(self):
        """-> (full, zero_marker, mask_tiles_recorded): hand-offs of the fused sweeps since the plan was created, published in full
        and as the one-word zero marker, and level-0 mask tiles recorded instead of stored (stitch_plan_handoff_counts)."""
        out = (C.c_uint64 * 3)()
        _chk(lib().stitch_plan_handoff_counts(self._h, out))
        return tuple(int(v) for v in out)

    def g_flag_counts(self):
        """-> (level 1, level 2): tile columns of the pyramid planes that the plan's last call recorded as all +0 instead of storing
        them (stitch_plan_g_flag_counts)."""
        out = (C.c_uint64 * 2)()
        _chk(lib().stitch_plan_g_flag_counts(self._h, out))
        return tuple(int(v) for v in out)

    def mask_row_counts(self):
        """-> (level 1, level 2): (tile column, band) entries of the mask plane that the plan's last call recorded as repeats of the
        plane's row 0 instead of storing them (stitch_plan_mask_row_counts)."""
        out = (C.c_uint64 * 2)()
        _chk(lib().stitch_plan_mask_row_counts(self._h, out))
        return tuple(int(v) for v in out)

    def index_counts(self):
        """-> (computed, reused, shared): level-0 index planes of the plan's last call -- slots whose plane the call computed, slots
        whose plane stood from an earlier call, pairs that read the plane of an earlier pair of the call (stitch_plan_index_counts)."""
        out = (C.c_uint32 * 3)()
        _chk(lib().stitch_plan_index_counts(self._h, out))
        return tuple(int(v) for v in out)

    def mask_keep_counts(self):
        """-> (computed, stood): slots whose mask planes the plan's last call computed, slots whose mask pyramid stood from an earlier
        call with the same seam record and form (stitch_plan_mask_keep_counts)."""
        out = (C.c_uint32 * 2)()
        _chk(lib().stitch_plan_mask_keep_counts(self._h, out))
        return tuple(int(v) for v in out)

    def mask_keep_form(self, n_pairs=1):
        """A call with n_pairs pairs is of a form under which mask pyramids stand (stitch_plan_call_forms, STITCH_CALL_MASK_KEEP)."""
        return bool(lib().stitch_plan_call_forms(self._h, int(n_pairs)) & CALL_MASK_KEEP)

    def src_run_counts(self):
        """-> (outside, no patch, 1..64 patches, general): 64 x 64 tiles of the index planes the last call's causal x sweep gathered
        through in 16-byte runs, each plane once (stitch_plan_src_run_counts)."""
        out = (C.c_uint32 * 4)()
        _chk(lib().stitch_plan_src_run_counts(self._h, out))
        return tuple(int(v) for v in out)

    def src_runs_fill(self, byte):
        """Test hook: every byte of the plan's run arrays set to `byte` (stitch_plan_src_runs_fill)."""
        _chk(lib().stitch_plan_src_runs_fill(self._h, int(byte)))

    def collapse_sides(self, pair=0):
        """-> (a_only, b_only, both): 256-column blocks of the last call's level-0 collapse of `pair` that read only image a, only
        image b, both (stitch_plan_collapse_sides)."""
        out = (C.c_int * 3)()
        _chk(lib().stitch_plan_collapse_sides(self._h, int(pair), out))
        return tuple(int(v) for v in out)

    def set_handoff_spin_limit(self, polls):
        _chk(lib().stitch_plan_set_handoff_spin_limit(self._h, int(polls)))

    def set_profiling_kernel(self, name):
        _chk(lib().stitch_plan_set_profiling_kernel(self._h, KERNELS.index(name)))

    def set_profiling(self, on):
        _chk(lib().stitch_plan_set_profiling(self._h, int(bool(on))))

    def read_profile(self):
        """-> {kernel: (total_ms, launches, level0_ms)} since profiling was enabled / last read."""
        ms, n, l0 = (C.c_double * len(KERNELS))(), (C.c_int * len(KERNELS))(), (C.c_double * len(KERNELS))()
        _chk(lib().stitch_plan_read_profile(self._h, ms, n, l0))
        return {KERNELS[i]: (ms[i], n[i], l0[i]) for i in range(len(KERNELS))}


class Band(_Handle):
    """stitch_band: this rank's row band of ONE pair split over several GPUs (include/stitch.h, "one pair split into row
    bands").  Computation only; what crosses ranks is moved by pipeline.BandStitcher."""
    _destroy = "stitch_band_destroy"

    def __init__(self, cw, ch, rank, nranks, split_levels, opts=None):
        self._h = C.c_void_p()
        _chk(lib().stitch_band_create(int(cw), int(ch), int(rank), int(nranks), int(split_levels), C.byref(_opts(opts)), C.byref(self._h)))
        self.cw, self.ch, self.rank, self.nranks, self.split_levels = int(cw), int(ch), int(rank), int(nranks), int(split_levels)
        tot = C.c_int()
        lib().stitch_band_levels(self._h, C.byref(tot))
        self.levels = tot.value
        self.geom = []
        for l in range(self.split_levels + 1):
            g = (C.c_int * 6)()
            _chk(lib().stitch_band_geometry(self._h, l, g))
            self.geom.append(dict(w=g[0], rows=g[1], row0=g[2], pitch=g[3], h=g[4], halo=g[5]))

    def compose(self, frame, p, offx, offy, mosaic, ox, oy):
        frame, mosaic = _timg(frame), _timg(mosaic)
        _chk(_fn("stitch_band_compose_", frame)(self._h, _dp(frame), frame.shape[2], frame.shape[1], _map8(p), offx, offy, _dp(mosaic),
                                                mosaic.shape[2], mosaic.shape[1], int(ox), int(oy), _stream()))

    def set_level0(self, source_fused):
        """Level 0 source-fused (default) or materialised (what the one-plane-at-a-time sweeps need); before the next compose."""
        _chk(lib().stitch_band_set_level0(self._h, int(bool(source_fused))))

    def reduce_x(self, level):
        _chk(lib().stitch_band_reduce_x(self._h, int(level), _stream()))

    def reduce_xy_fwd(self, level, resume, state_out):
        """reduce_x + reduce_y_fwd(plane -1) with the anticausal x and causal y sweeps fused (one pass over the level)."""
        _chk(lib().stitch_band_reduce_xy_fwd(self._h, int(level), _dp(resume), _dp(state_out), _stream()))

    def reduce_y_fwd(self, level, plane, resume, state_out):
        _chk(lib().stitch_band_reduce_y_fwd(self._h, int(level), int(plane), _dp(resume), _dp(state_out), _stream()))

    def reduce_y_bwd(self, level, plane, fwd_state, resume, state_out):
        _chk(lib().stitch_band_reduce_y_bwd(self._h, int(level), int(plane), _dp(fwd_state), _dp(resume), _dp(state_out), _stream()))

    def reduce_y_fwd_cols(self, level, x0, x1, resume, state_out):
        _chk(lib().stitch_band_reduce_y_fwd_cols(self._h, int(level), int(x0), int(x1), _dp(resume), _dp(state_out), _stream()))

    def reduce_y_bwd_cols(self, level, x0, x1, fwd_state, resume, state_out):
        _chk(lib().stitch_band_reduce_y_bwd_cols(self._h, int(level), int(x0), int(x1), _dp(fwd_state), _dp(resume), _dp(state_out), _stream()))

    def rows(self, level, kind, first_row, nrows, buf, to_buffer):
        assert buf.is_cuda and buf.is_contiguous() and buf.dtype.is_floating_point and buf.element_size() == 4
        _chk(lib().stitch_band_rows(self._h, int(level), int(kind), int(first_row), int(nrows), _dp(buf), int(bool(to_buffer)), _stream()))

    def top(self, g7):
        assert g7.is_cuda and g7.is_contiguous()
        _chk(lib().stitch_band_top(self._h, _dp(g7), _stream()))

    def collapse(self, level, out=None):
        if level == 0:
            _chk(_fn("stitch_band_collapse_", out)(self._h, 0, _dp(out), _stream()))
        else:
            _chk(lib().stitch_band_collapse_f32(self._h, int(level), None, _stream()))

    def status(self):
        s = Seam()
        _chk(lib().stitch_band_status(self._h, C.byref(s)))
        return s


# ---- a calibrated rig: include/stitch_rig.h ---------------------------------------------------------------------------------
class Panorama(_Handle):
    """stitch_panorama: the result handle of a whole-panorama call, kept open (dev_panorama_handle) -- what Rig.from_panorama reads."""
    _destroy = "stitch_panorama_destroy"

    def __init__(self, h, device):
        self._h, self.device = h, device
        w, ht, start, ns = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _chk(lib().stitch_panorama_info(h, C.byref(w), C.byref(ht), C.byref(start), C.byref(ns)))
        self.width, self.height, self.start, self.n_steps = w.value, ht.value, start.value, ns.value

    def mosaic(self):
        """A copy of the mosaic as a (3, height, width) uint8 tensor, complete when this returns."""
        import torch
        out = torch.empty((3, self.height, self.width), dtype=torch.uint8, device=self.device)
        _chk(lib().stitch_panorama_copy(self._h, -1, _dp(out), out.numel(), 1, _stream()))
        torch.cuda.current_stream().synchronize()
        return out


def dev_panorama_handle(frames, opts=None, finish=True, num=19.0, den=20.0, sift_opts=None, ransac_opts=None, kp_cap=4096, feat_cap=None,
                        ratio=RATIO_THRESHOLD, match_threshold=20, fov_deg=15.0, exposure=None):
    """dev_panorama, but the result stays behind its handle -> Panorama (close() it when done).  exposure: as dev_panorama's."""
    frames, arr = _frames_u8(frames)
    keep, h = [], C.c_void_p()
    o = _panorama_opts(opts, finish, num, den, sift_opts, ransac_opts, kp_cap, feat_cap, False, ratio, match_threshold, fov_deg, keep)
    e = _exposure(exposure)
    if e is None:
        _chk(lib().stitch_dev_panorama_u8(arr, len(frames), C.byref(o), _stream(), C.byref(h)))
    else:
        _chk(lib().stitch_dev_panorama_exposure_u8(arr, len(frames), C.byref(o), C.byref(e), _stream(), C.byref(h)))
    return Panorama(h, frames[0].device)


class RigOpts(C.Structure):
    """stitch_rig_opts; the defaults are stitch_rig_opts_default's."""
    _fields_ = [("blend", C.c_void_p), ("fov_deg", C.c_float), ("finish", C.c_int32), ("num", C.c_double), ("den", C.c_double),
                ("max_sets", C.c_int32)]


def _rig_opts(opts, finish, num, den, max_sets, fov_deg, keep):
    o = RigOpts()
    lib().stitch_rig_opts_default(C.byref(o))
    if opts is not None:
        keep.append(_opts(opts))  # the library copies it during creation
        o.blend = C.addressof(keep[-1])
    o.fov_deg, o.finish, o.num, o.den, o.max_sets = float(fov_deg), int(bool(finish)), float(num), float(den), int(max_sets)
    return o


def rig_steps(steps, start=None):
    """Step dicts -> (start, PanoramaStep array).  The dicts are those of dev_panorama(return_steps=True), pipeline.stitch_chain and
    tests/golden/golden.json: start, src, p, p_fwd, offx, offy, ox, oy, cw, ch.  In them `src` is the frame that is WARPED -- `dst`
    of stitch_panorama_step -- and `p` the backward map; the frame already in the mosaic ("mosaic_src", where a dict has it) goes
    into stitch_panorama_step's src, which no step depends on."""
    steps = list(steps)
    arr = (PanoramaStep * max(len(steps), 1))()
    for d, st in zip(arr, steps):
        d.src, d.dst = int(st.get("mosaic_src", -1)), int(st["src"])
        d.p_fwd, d.p_bwd = _map8(st["p_fwd"]), _map8(st["p"])
        d.geom = StepGeom(float(st["offx"]), float(st["offy"]), int(st["cw"]), int(st["ch"]), int(st["ox"]), int(st["oy"]))
    if start is None:
        start = steps[0]["start"]
    return int(start), arr


class Rect(C.Structure):
    """stitch_rect (include/stitch_rig_crop.h): x0, y0, w, h."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]

    def as_tuple(self):
        return (self.x0, self.y0, self.w, self.h)


CROP_AFTER_FINISH, CROP_BEFORE_FINISH = 1, 2


def _rect(rect):
    return rect if isinstance(rect, Rect) else Rect(*[int(v) for v in rect])


def dev_largest_rect(mask):
    """stitch_dev_largest_rect_u8 on torch's current stream, which it waits for: the largest axis-aligned rectangle of non-zero
    bytes inside a contiguous (h, w) uint8 device tensor, as (x0, y0, w, h) -- the largest area, then the smallest y0, the smallest
    x0, the widest; (0, 0, 0, 0) where nothing is covered."""
    import torch
    if not mask.is_cuda or not mask.is_contiguous() or mask.dim() != 2 or mask.dtype != torch.uint8:
        raise ValueError("expected a contiguous (H, W) uint8 tensor on the HIP device")
    r = Rect()
    _chk(lib().stitch_dev_largest_rect_u8(_dp(mask), mask.shape[1], mask.shape[0], C.byref(r), _stream()))
    return r.as_tuple()


# ---- camera layouts: include/stitch_rig_formats.h ---------------------------------------------------------------------------
PIX_PLANAR, PIX_RGB24, PIX_BGR24, PIX_RGBX32, PIX_BGRX32, PIX_NV12 = range(6)
_PIX_BPP = {PIX_RGB24: 3, PIX_BGR24: 3, PIX_RGBX32: 4, PIX_BGRX32: 4, PIX_NV12: 1}
# include/stitch_rig_formats_yuv.h: the 4:2:2 layouts and NV21, and the forms Rig.input_form answers with
PIX_YUYV, PIX_UYVY, PIX_NV21, PIX_NV16 = range(16, 20)
_PIX_TWO_PLANES = (PIX_NV12, PIX_NV21, PIX_NV16)
_PIX_ALL = tuple(range(6)) + tuple(range(16, 20))
RIG_INPUT_NONE, RIG_INPUT_FUSED, RIG_INPUT_CONVERTED = range(3)


class ImageDesc(C.Structure):
    """stitch_image."""
    _fields_ = [("data", C.c_void_p), ("data2", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32), ("pitch2", C.c_int32)]


def tight_pitches(fmt, w):
    """(pitch, pitch2) of rows without padding; (0, 0) for PIX_PLANAR, which has none."""
    if fmt == PIX_PLANAR:
        return 0, 0
    pairs = 2 * ((w + 1) // 2)
    if fmt in (PIX_YUYV, PIX_UYVY):  # groups of 4 bytes, two pixels each
        return 2 * pairs, 0
    return (w if fmt in _PIX_TWO_PLANES else _PIX_BPP[fmt] * w), (pairs if fmt in _PIX_TWO_PLANES else 0)


def image_bytes(fmt, w, h, pitch=None, pitch2=None):
    """stitch_image_bytes (host only): the extent of each plane in bytes, (bytes, bytes2); a pitch of None is the tight one.  Raises
    StitchError(ERR_ARG) for a bad format, size or pitch."""
    tight = tight_pitches(fmt, w) if fmt in _PIX_ALL else (0, 0)
    b1, b2 = C.c_size_t(), C.c_size_t()
    _chk(lib().stitch_image_bytes(int(fmt), int(w), int(h), int(tight[0] if pitch is None else pitch), int(tight[1] if pitch2 is None else pitch2),
                                  C.byref(b1), C.byref(b2)))
    return b1.value, b2.value


class Image:
    """One image in a layout of include/stitch_rig_formats.h or include/stitch_rig_formats_yuv.h: uint8 device tensors plus pitches.
    `data` (and for PIX_NV12, PIX_NV21 and PIX_NV16 `data2`, the chroma plane) are contiguous uint8 tensors that start at the plane's
    first byte and hold at least image_bytes(...) bytes -- any shape, so a view into a larger buffer gives an odd base; for PIX_PLANAR
    `data` is the dense (3, h, w) tensor of every other call."""

    def __init__(self, fmt, width, height, data, data2=None, pitch=None, pitch2=None):
        tight = tight_pitches(fmt, width)
        self.fmt, self.width, self.height, self.data, self.data2 = int(fmt), int(width), int(height), data, data2
        self.pitch, self.pitch2 = int(tight[0] if pitch is None else pitch), int(tight[1] if pitch2 is None else pitch2)
        need = image_bytes(self.fmt, self.width, self.height, self.pitch, self.pitch2)
        for t, n in ((data, need[0]), (data2, need[1])):
            if n and (t is None or not t.is_cuda or not t.is_contiguous() or str(t.dtype) != "torch.uint8" or t.numel() < n):
                raise ValueError(f"every plane is a contiguous uint8 device tensor of at least {n} bytes")

    @classmethod
    def empty(cls, fmt, width, height, device="cuda", pitch=None, pitch2=None, fill=None):
        """A fresh image of exactly image_bytes(...) bytes per plane (fill: a byte value to set every byte to)."""
        import torch
        tight = tight_pitches(fmt, width)
        pitch, pitch2 = tight[0] if pitch is None else pitch, tight[1] if pitch2 is None else pitch2
        b1, b2 = image_bytes(fmt, width, height, pitch, pitch2)
        make = (lambda n: torch.empty(n, dtype=torch.uint8, device=device)) if fill is None else (lambda n: torch.full((n,), fill, dtype=torch.uint8, device=device))
        data = make(b1).view(3, height, width) if fmt == PIX_PLANAR else make(b1)
        return cls(fmt, width, height, data, make(b2) if b2 else None, pitch, pitch2)

    def desc(self):
        return ImageDesc(self.data.data_ptr(), self.data2.data_ptr() if self.data2 is not None else None, self.width, self.height, self.pitch, self.pitch2)


def _image_array(images):
    return (ImageDesc * max(len(images), 1))(*[im.desc() for im in images])


def _planar_list(planar, w, h):
    import torch
    planar = [_timg(t) for t in planar]
    if any(tuple(t.shape) != (3, h, w) or t.dtype != torch.uint8 for t in planar):
        raise ValueError(f"every planar image is a (3, {h}, {w}) uint8 tensor")
    return planar


def dev_unpack_many(images, matrix=0, out=None):
    """stitch_dev_unpack_many_u8 on torch's current stream, which it waits for: same-size, same-format Images -> dense planar
    (3, h, w) tensors, one launch."""
    import torch
    images = list(images)
    fmt, w, h = images[0].fmt, images[0].width, images[0].height
    if any(im.fmt != fmt for im in images):
        raise ValueError("one format per call")
    if out is None:
        out = [torch.empty((3, h, w), dtype=torch.uint8, device=images[0].data.device) for _ in images]
    out = _planar_list(out, w, h)
    if len(out) != len(images):
        raise ValueError("one planar output per image")
    ptrs = (C.c_void_p * max(len(out), 1))(*[t.data_ptr() for t in out])
    _chk(lib().stitch_dev_unpack_many_u8(fmt, int(matrix), _image_array(images), ptrs, len(images), _stream()))
    return out


def dev_pack_many(planar, fmt=None, matrix=0, out=None, pitch=None, pitch2=None):
    """stitch_dev_pack_many_u8 on torch's current stream, which it waits for: dense planar (3, h, w) tensors -> Images of `fmt`, one
    launch; into `out` (Images; their format is the call's) or fresh images of the given pitches (None: tight)."""
    planar = list(planar)
    _, h, w = planar[0].shape
    planar = _planar_list(planar, w, h)
    if out is None:
        out = [Image.empty(fmt, w, h, planar[0].device, pitch, pitch2) for _ in planar]
    out = list(out)
    fmt = out[0].fmt if fmt is None else fmt
    if len(out) != len(planar) or any(im.fmt != fmt for im in out):
        raise ValueError("one image of the call's format per planar input")
    ptrs = (C.c_void_p * max(len(planar), 1))(*[t.data_ptr() for t in planar])
    _chk(lib().stitch_dev_pack_many_u8(int(fmt), int(matrix), ptrs, _image_array(out), len(planar), _stream()))
    return out


def dev_scale_pack_many(planar, size, fmt=PIX_PLANAR, matrix=0, rect=None, out=None, pitch=None, pitch2=None):
    """stitch_dev_scale_pack_many_u8 on torch's current stream, which it waits for: of every dense planar (3, h, w) tensor the
    rectangle rect = (x0, y0, w, h) (None: the whole image) scaled to size = (ow, oh) by the exact area average of
    include/stitch_rig_scale.h and written as an Image of `fmt`, one launch; into `out` (Images of that size; their format is the
    call's) or fresh images of the given pitches (None: tight).  Returns the Images (PIX_PLANAR: their .data is the (3, oh, ow) tensor)."""
    planar = list(planar)
    _, h, w = planar[0].shape
    planar = _planar_list(planar, w, h)
    ow, oh = int(size[0]), int(size[1])
    if out is None:
        out = [Image.empty(fmt, ow, oh, planar[0].device, pitch, pitch2) for _ in planar]
    out = list(out)
    if len(out) != len(planar) or any(im.fmt != fmt for im in out):
        raise ValueError("one image of the call's format per planar input")
    ptrs = (C.c_void_p * max(len(planar), 1))(*[t.data_ptr() for t in planar])
    _chk(lib().stitch_dev_scale_pack_many_u8(int(fmt), int(matrix), ptrs, w, h, C.byref(_rect(rect)) if rect is not None else None, _image_array(out),
                                             len(planar), _stream()))
    return out


class Rig(_Handle):
    """stitch_rig: the recorded stitch order, maps and canvases of a panorama, replayed on many frame sets -- step k of all the
    sets of a call is one batched launch sequence."""
    _destroy = "stitch_rig_destroy"

    def __init__(self, h):
        self._h = h
        v = [C.c_int() for _ in range(5)]
        _chk(lib().stitch_rig_info(h, *[C.byref(x) for x in v]))
        self.width, self.height, self.n_frames, self.n_steps, self.max_sets = (x.value for x in v)

    @classmethod
    def from_steps(cls, frame_sizes, start, steps, opts=None, finish=True, num=19.0, den=20.0, max_sets=16, fov_deg=15.0, exposure=0, keep_black=True,
                   stats_form=2):
        """stitch_rig_create (host only): frame_sizes = (width, height) of every decoded frame; steps = step dicts as rig_steps
        takes them (`src` is the WARPED frame) or a ready PanoramaStep array; start may be None to take steps[0]["start"].
        exposure 1 / 2 (stitch_rig_create_exposure): every step of the replay first matches the frame's colours to the frame it is
        stitched to (the step's "mosaic_src", which must then be a frame already placed) / to the running mosaic, per set."""
        if isinstance(steps, C.Array):
            arr, n_steps = steps, len(steps)
        else:
            steps = list(steps)
            n_steps = len(steps)
            start, arr = rig_steps(steps, start) if steps else (start, (PanoramaStep * 1)())
        wh = np.ascontiguousarray(np.array(frame_sizes, np.int32).reshape(-1, 2))
        keep, h = [], C.c_void_p()
        o = _rig_opts(opts, finish, num, den, max_sets, fov_deg, keep)
        if exposure:
            e = _exposure(dict(mode=exposure, keep_black=bool(keep_black), stats_form=stats_form))
            _chk(lib().stitch_rig_create_exposure(_p(wh), wh.shape[0], int(start), arr, n_steps, C.byref(o), C.byref(e), C.byref(h)))
        else:
            _chk(lib().stitch_rig_create(_p(wh), wh.shape[0], int(start), arr, n_steps, C.byref(o), C.byref(h)))
        return cls(h)

    @classmethod
    def from_panorama(cls, pano, frames, opts=None, finish=True, num=19.0, den=20.0, max_sets=16, fov_deg=15.0, exposure=0, keep_black=True, stats_form=2,
                      seams=None):
        """stitch_rig_from_panorama: pano is a Panorama (dev_panorama_handle), frames the tensors it was made from (sizes only).
        exposure 1 / 2: stitch_rig_from_panorama_exposure, as from_steps; the handle's own mode is not read.
        seams="recorded": fix_seams from the records of the panorama's own steps."""
        if seams not in (None, "recorded"):
            raise ValueError('seams: None or "recorded"')
        arr = (FrameU8 * max(len(frames), 1))(*[FrameU8(None, f.shape[2], f.shape[1]) for f in frames])
        keep, h = [], C.c_void_p()
        o = _rig_opts(opts, finish, num, den, max_sets, fov_deg, keep)
        if exposure:
            e = _exposure(dict(mode=exposure, keep_black=bool(keep_black), stats_form=stats_form))
            _chk(lib().stitch_rig_from_panorama_exposure(pano._h, arr, len(frames), C.byref(o), C.byref(e), C.byref(h)))
        else:
            _chk(lib().stitch_rig_from_panorama(pano._h, arr, len(frames), C.byref(o), C.byref(h)))
        rig = cls(h)
        if seams == "recorded":
            rec = []
            for k in range(rig.n_steps):
                st = PanoramaStep()
                _chk(lib().stitch_panorama_step_at(pano._h, k, C.byref(st)))
                rec.append(st.seam.as_tuple())
            rig.fix_seams(rec)
        return rig

    @classmethod
    def from_calibration(cls, cal, opts=None, finish=True, num=19.0, den=20.0, max_sets=16, fov_deg=15.0, exposure=0, keep_black=True, stats_form=2):
        """stitch_rig_from_calibration: cal is a Calibration (dev_calibrate); its frame sizes, start and steps make the rig.
        exposure 1 / 2: as from_steps."""
        keep, h = [], C.c_void_p()
        o = _rig_opts(opts, finish, num, den, max_sets, fov_deg, keep)
        e = _exposure(dict(mode=exposure, keep_black=bool(keep_black), stats_form=stats_form)) if exposure else None
        _chk(lib().stitch_rig_from_calibration(cal._h, C.byref(o), None if e is None else C.byref(e), C.byref(h)))
        return cls(h)

    def step_plan(self, k):
        """stitch_rig_step_plan: the address of the batched workspace step k runs on (None before the first stitch call)."""
        return lib().stitch_rig_step_plan(self._h, int(k))

    def fix_seams(self, seams):
        """stitch_rig_fix_seams (host only): one Seam or (sum_a_x, n_a, sum_ov_x, n_ov, ...) tuple per step; every later stitch()
        uses them for every set, and no set fails for its pixels.  Returns self."""
        seams = list(seams)
        _chk(lib().stitch_rig_fix_seams(self._h, _seam_array(seams), len(seams)))
        return self

    def clear_seams(self):
        """stitch_rig_clear_seams: back to content seams.  Returns self."""
        _chk(lib().stitch_rig_clear_seams(self._h))
        return self

    @property
    def seams(self):
        """stitch_rig_seams: the fixed records as Seam tuples, one per step ([] = content seams)."""
        arr = (Seam * max(self.n_steps, 1))()
        n = _chk(lib().stitch_rig_seams(self._h, arr, self.n_steps))
        return [arr[k].as_tuple() for k in range(n)]

    def geometric_seams(self):
        """stitch_dev_rig_geometric_seams on torch's current stream, which it waits for: the seams of the cameras' footprints,
        computed on the device and fixed.  Raises StitchError (ERR_EMPTY_MIDROW / ERR_ZERO_OVERLAP naming the step) where the
        footprints give no seam; the rig then keeps the seams it had.  Returns self."""
        _chk(lib().stitch_dev_rig_geometric_seams(self._h, None, _stream()))
        return self

    def coverage(self, step=-1, which=2, out=None, device=None):
        """stitch_dev_rig_coverage_u8 on torch's current stream: step's canvas as a (ch, cw) uint8 tensor of 0 / 255 -- which = 0 the
        warped frame's footprint, 1 the moved mosaic's, 2 either; step -1 is the last step: the validity mask of the output."""
        import torch
        cw, ch = C.c_int(), C.c_int()
        _chk(lib().stitch_rig_step_canvas(self._h, int(step), C.byref(cw), C.byref(ch)))
        w, h = cw.value, ch.value
        if out is None:
            out = torch.empty((h, w), dtype=torch.uint8, device=device or "cuda")
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= w * h
        _chk(lib().stitch_dev_rig_coverage_u8(self._h, int(step), int(which), _dp(out), _stream()))
        return out

    def inscribed_rect(self, step=-1):
        """stitch_dev_rig_inscribed_rect on torch's current stream, which it waits for: the largest rectangle (x0, y0, w, h) inside
        step's A | B coverage, read from the rig's bit planes (dev_largest_rect's rule); step -1: inside the output's validity mask."""
        r = Rect()
        _chk(lib().stitch_dev_rig_inscribed_rect(self._h, int(step), C.byref(r), _stream()))
        return r.as_tuple()

    def set_crop(self, rect=None, mode=CROP_AFTER_FINISH):
        """stitch_rig_set_crop (host only): every later stitch() writes the rectangle (x0, y0, w, h) of the output canvas alone --
        mode 1 (CROP_AFTER_FINISH) the slice of the finished canvas, mode 2 (CROP_BEFORE_FINISH) the finish pass on the slice of the
        unfinished one.  rect=None takes inscribed_rect() (on the device) and raises ValueError if it is empty.  Returns self."""
        if rect is None:
            rect = self.inscribed_rect()
            if rect[2] < 1 or rect[3] < 1:
                raise ValueError("the output's coverage holds no rectangle")
        _chk(lib().stitch_rig_set_crop(self._h, C.byref(_rect(rect)), int(mode)))
        return self

    def clear_crop(self):
        """stitch_rig_clear_crop: back to the whole canvas.  Returns self."""
        _chk(lib().stitch_rig_clear_crop(self._h))
        return self

    @property
    def crop(self):
        """stitch_rig_crop: ((x0, y0, w, h), mode); mode 0 is no crop, with the whole canvas as the rectangle."""
        r, mode = Rect(), C.c_int()
        _chk(lib().stitch_rig_crop(self._h, C.byref(r), C.byref(mode)))
        return r.as_tuple(), mode.value

    def _out_size(self):
        w, h = C.c_int(), C.c_int()
        _chk(lib().stitch_rig_output_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    @property
    def out_width(self):
        """stitch_rig_output_size: the width of what stitch() writes per set (the crop's, or the canvas's)."""
        return self._out_size()[0]

    @property
    def out_height(self):
        return self._out_size()[1]

    def set_output_scale(self, ow, oh):
        """stitch_rig_set_output_scale (host only): every later stitch() writes ow x oh per set -- the exact area average
        (include/stitch_rig_scale.h) of what it writes without the scale, in the output format; 1 <= ow <= w <= 8 ow and likewise
        for oh against the rig's present output size (the crop's, else the canvas).  Returns self."""
        _chk(lib().stitch_rig_set_output_scale(self._h, int(ow), int(oh)))
        return self

    def clear_output_scale(self):
        """stitch_rig_clear_output_scale: back to the crop's or the canvas's size.  Returns self."""
        _chk(lib().stitch_rig_clear_output_scale(self._h))
        return self

    @property
    def output_scale(self):
        """stitch_rig_output_scale: (ow, oh), or None when no scale is set."""
        if not hasattr(lib(), "stitch_rig_output_scale"):  # an A/B build of an earlier tree, STITCH_LIB
            return None
        w, h = C.c_int(), C.c_int()
        _chk(lib().stitch_rig_output_scale(self._h, C.byref(w), C.byref(h)))
        return (w.value, h.value) if w.value else None

    def set_formats(self, in_fmt, out_fmt, matrix=0):
        """stitch_rig_set_formats (host only): every later stitch() takes its frames as Images of in_fmt and returns Images of
        out_fmt (include/stitch_rig_formats.h, include/stitch_rig_formats_yuv.h); matrix: the Y Cb Cr matrix of both sides.  Returns self."""
        _chk(lib().stitch_rig_set_formats(self._h, int(in_fmt), int(out_fmt), int(matrix)))
        return self

    def clear_formats(self):
        """stitch_rig_clear_formats: planar both ways again.  Returns self."""
        _chk(lib().stitch_rig_clear_formats(self._h))
        return self

    @property
    def formats(self):
        """stitch_rig_formats: (in_fmt, out_fmt, matrix); (0, 0, 0) is every rig that never set one."""
        if not hasattr(lib(), "stitch_rig_formats"):  # an A/B build of an earlier tree, STITCH_LIB
            return 0, 0, 0
        v = [C.c_int() for _ in range(3)]
        _chk(lib().stitch_rig_formats(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def input_form(self, frame):
        """stitch_rig_input_form (host only): how the last completed stitch() with a format set read frame index `frame` --
        RIG_INPUT_NONE (no such call yet, a planar in_fmt, or a frame no step uses), RIG_INPUT_FUSED (the tiled projection staged the
        packed frames itself) or RIG_INPUT_CONVERTED (one conversion launch into planar scratch, then the planar projection)."""
        form = C.c_int()
        _chk(lib().stitch_rig_input_form(self._h, int(frame), C.byref(form)))
        return form.value

    def set_monitor(self, radius):
        """stitch_rig_set_monitor (host only): every later stitch() also measures, per set and step, the residuals of the blend's
        two inputs over the step's overlap under every integer shift within `radius` (0 .. 8; include/stitch_rig_monitor.h);
        residuals() reads them.  Outputs, statuses, seams and statistics stay what they are.  Returns self."""
        _chk(lib().stitch_rig_set_monitor(self._h, int(radius)))
        return self

    def clear_monitor(self):
        """stitch_rig_clear_monitor: no monitor.  Returns self."""
        _chk(lib().stitch_rig_clear_monitor(self._h))
        return self

    @property
    def monitor(self):
        """stitch_rig_monitor: the monitor's radius, or None when none is set."""
        r = C.c_int(-1)
        _chk(lib().stitch_rig_monitor(self._h, C.byref(r)))
        return None if r.value < 0 else r.value

    def residuals(self):
        """stitch_rig_residuals (host only): the records of the last monitored stitch() as an (n_sets, n_steps, words) uint64 numpy
        array -- n, sum_b, then sum_a, sad, ssd per shift; n_sets = 0 when there is none."""
        n_sets, n_steps, radius = C.c_int(), C.c_int(), C.c_int()
        _chk(lib().stitch_rig_residuals(self._h, None, 0, C.byref(n_sets), C.byref(n_steps), C.byref(radius)))
        words = residual_words(radius.value) if radius.value >= 0 else 0
        out = np.zeros((n_sets.value, n_steps.value, words), np.uint64)
        if out.size:
            _chk(lib().stitch_rig_residuals(self._h, _p(out), out.size, None, None, None))
        return out

    def residual_domain(self, step=-1, radius=None, out=None, device=None):
        """stitch_dev_rig_residual_domain_u8 on torch's current stream: the domain the monitor sums step's records over, as a
        (ch, cw) uint8 tensor of 0 / 255 -- the moved mosaic's coverage and the warped frame's, eroded by the shift box of `radius`
        (None: the monitor's).  Does not change the rig's monitor."""
        import torch
        if radius is None:
            radius = self.monitor
            if radius is None:
                raise ValueError("no monitor is set: state the radius")
        cw, ch = C.c_int(), C.c_int()
        _chk(lib().stitch_rig_step_canvas(self._h, int(step), C.byref(cw), C.byref(ch)))
        w, h = cw.value, ch.value
        if out is None:
            out = torch.empty((h, w), dtype=torch.uint8, device=device or "cuda")
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= w * h
        _chk(lib().stitch_dev_rig_residual_domain_u8(self._h, int(step), int(radius), _dp(out), _stream()))
        return out

    def set_seam_paths(self, max_step=2, margin=8):
        """stitch_rig_set_seam_paths (include/stitch_seam_path.h): from now on every stitch() finds, per set and step, the least-cost
        seam column of every row over the step's coverage (steps of at most max_step columns per row, coverage eroded by margin) and
        blends along it, with no host round trip.  The seams stitch() returns are the geometric records.  Returns self."""
        _chk(lib().stitch_rig_set_seam_paths(self._h, C.byref(SeamPathOpts(int(max_step), int(margin)))))
        return self

    def fix_seam_paths(self, paths):
        """stitch_rig_fix_seam_paths: one path per step -- the step's ch seam columns, any integer sequence -- shared by all sets.
        Returns self."""
        rows = [np.ascontiguousarray(np.asarray(p.cpu() if hasattr(p, "cpu") else p).astype(np.int32).reshape(-1)) for p in paths]
        for k, r in enumerate(rows[:self.n_steps]):
            cw, ch = C.c_int(), C.c_int()
            _chk(lib().stitch_rig_step_canvas(self._h, k, C.byref(cw), C.byref(ch)))
            if r.size != ch.value:
                raise ValueError(f"the path of step {k} has {ch.value} rows, got {r.size}")
        _chk(lib().stitch_rig_fix_seam_paths(self._h, (C.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows]), len(rows)))
        return self

    def clear_seam_paths(self):
        """stitch_rig_clear_seam_paths: vertical seams again.  Returns self."""
        _chk(lib().stitch_rig_clear_seam_paths(self._h))
        return self

    @property
    def seam_paths(self):
        """stitch_rig_seam_paths: None, ("found", max_step, margin) or ("fixed",)."""
        mode, o = C.c_int(), SeamPathOpts()
        _chk(lib().stitch_rig_seam_paths(self._h, C.byref(mode), C.byref(o)))
        return None if mode.value == 0 else ("found", o.max_step, o.margin) if mode.value == 1 else ("fixed",)

    def last_seam_paths(self, set=0, step=0):
        """stitch_rig_last_seam_paths (host only): (path, cost) of `set` at `step` in the last stitch() along paths -- an int32 numpy
        array of the step's ch columns and the path's cost (0 for fixed paths)."""
        cost = C.c_uint64()
        ch = _chk(lib().stitch_rig_last_seam_paths(self._h, int(set), int(step), None, 0, None))
        out = np.zeros(ch, np.int32)
        _chk(lib().stitch_rig_last_seam_paths(self._h, int(set), int(step), _p(out), ch, C.byref(cost)))
        return out, cost.value

    def set_seam_anchor(self, weight, cap, policy="set"):
        """stitch_rig_set_seam_anchor (include/stitch_seam_anchor.h): while found paths are set (set_seam_paths) every path also pays
        weight * min(|s - r|, cap) per row for leaving the anchor r -- policy "set": the previous set's path, across sequences and
        calls; "call": the path of the previous call's last set.  weight >= 0, cap >= 1, weight * cap <= 2055.  Returns self."""
        pol = {"set": SEAM_ANCHOR_PER_SET, "call": SEAM_ANCHOR_PER_CALL}.get(policy, policy)
        _chk(lib().stitch_rig_set_seam_anchor(self._h, C.byref(SeamAnchorOpts(int(weight), int(cap), int(pol)))))
        return self

    def prime_seam_anchor(self, paths):
        """stitch_rig_prime_seam_anchor: one path per step -- the step's ch columns, any integers -- becomes the anchor.  Returns self."""
        rows = [np.ascontiguousarray(np.asarray(p.cpu() if hasattr(p, "cpu") else p).astype(np.int32).reshape(-1)) for p in paths]
        for k, r in enumerate(rows[:self.n_steps]):
            cw, ch = C.c_int(), C.c_int()
            _chk(lib().stitch_rig_step_canvas(self._h, k, C.byref(cw), C.byref(ch)))
            if r.size != ch.value:
                raise ValueError(f"the anchor of step {k} has {ch.value} rows, got {r.size}")
        _chk(lib().stitch_rig_prime_seam_anchor(self._h, (C.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows]), len(rows)))
        return self

    def reset_seam_anchor(self):
        """stitch_rig_reset_seam_anchor: forget the anchor, keep the options -- a scene cut.  Returns self."""
        _chk(lib().stitch_rig_reset_seam_anchor(self._h))
        return self

    def clear_seam_anchor(self):
        """stitch_rig_clear_seam_anchor: forget the anchor and the options.  Returns self."""
        _chk(lib().stitch_rig_clear_seam_anchor(self._h))
        return self

    def seam_anchor(self):
        """stitch_rig_seam_anchor: (options, has_anchor) -- options None where none are set, else (weight, cap, "set" | "call")."""
        o, has = SeamAnchorOpts(), C.c_int()
        _chk(lib().stitch_rig_seam_anchor(self._h, C.byref(o), C.byref(has)))
        return (None if o.policy == 0 else (o.weight, o.cap, "set" if o.policy == SEAM_ANCHOR_PER_SET else "call")), bool(has.value)

    def last_seam_moved(self, set=0, step=0):
        """stitch_rig_last_seam_moved (host only): `moved` of `set` at `step` in the last stitch() along paths."""
        moved = C.c_uint64()
        _chk(lib().stitch_rig_last_seam_moved(self._h, int(set), int(step), C.byref(moved)))
        return moved.value

    # ---- temporal exposure: include/stitch_rig_exposure_temporal.h (host only; the rig was made with exposure 1 or 2) ----
    def _records(self, stats, what):
        a = np.ascontiguousarray(np.asarray(stats.cpu() if hasattr(stats, "cpu") else stats, dtype=np.float32))
        if a.size % 12:
            raise ValueError(f"{what}: one record of 12 floats per step")
        return a.reshape(-1, 12)

    def set_exposure_smoothing(self, keep):
        """stitch_rig_set_exposure_smoothing: from the next stitch() on every step's transfer applies filtered statistics
        u = m + (keep / 256) * (p - m), p the step's state, carried from set to set across sequences and calls.  keep 0 .. 255.
        Returns self."""
        _chk(lib().stitch_rig_set_exposure_smoothing(self._h, int(keep)))
        return self

    def clear_exposure_smoothing(self):
        """stitch_rig_clear_exposure_smoothing: forget the option and the state.  Returns self."""
        _chk(lib().stitch_rig_clear_exposure_smoothing(self._h))
        return self

    def reset_exposure_state(self):
        """stitch_rig_reset_exposure_state: forget the state, keep the option -- a scene cut.  Returns self."""
        _chk(lib().stitch_rig_reset_exposure_state(self._h))
        return self

    def prime_exposure_state(self, stats):
        """stitch_rig_prime_exposure_state: (n_steps, 12) float32, one valid record per step, becomes the state.  Returns self."""
        a = self._records(stats, "prime_exposure_state")
        _chk(lib().stitch_rig_prime_exposure_state(self._h, _p(a), a.shape[0]))
        return self

    def exposure_smoothing(self):
        """stitch_rig_exposure_smoothing: (keep, has) -- keep None where no smoothing is set, has a list of one bool per step."""
        keep, has = C.c_int(), (C.c_int32 * max(self.n_steps, 1))()
        _chk(lib().stitch_rig_exposure_smoothing(self._h, C.byref(keep), has))
        return (None if keep.value < 0 else keep.value), [bool(v) for v in has[:self.n_steps]]

    def exposure_state(self):
        """stitch_rig_exposure_state: (n_steps, 12) float32, the state as the last completed stitch() or a later prime left it."""
        out = np.zeros((self.n_steps, 12), np.float32)
        _chk(lib().stitch_rig_exposure_state(self._h, _p(out), self.n_steps))
        return out

    def fix_exposure(self, stats):
        """stitch_rig_fix_exposure: (n_steps, 12) float32, one valid record per step, applied to every set from now on: nothing is
        measured and the smoothing state rests.  Returns self."""
        a = self._records(stats, "fix_exposure")
        _chk(lib().stitch_rig_fix_exposure(self._h, _p(a), a.shape[0]))
        return self

    def clear_fixed_exposure(self):
        """stitch_rig_clear_fixed_exposure: measured statistics again.  Returns self."""
        _chk(lib().stitch_rig_clear_fixed_exposure(self._h))
        return self

    def fixed_exposure(self):
        """stitch_rig_fixed_exposure: None, or the (n_steps, 12) float32 fixed statistics."""
        n = C.c_int()
        _chk(lib().stitch_rig_fixed_exposure(self._h, None, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros((n.value, 12), np.float32)
        _chk(lib().stitch_rig_fixed_exposure(self._h, _p(out), C.byref(n)))
        return out

    def last_used_stats(self):
        """stitch_rig_last_used_stats: (n_sets, n_steps, 12) float32, what the apply passes of the last stitch() with smoothing or
        fixed statistics read (n_sets = 0 where there is none)."""
        n_sets, n_steps = C.c_int(), C.c_int()
        _chk(lib().stitch_rig_last_used_stats(self._h, None, 0, C.byref(n_sets), C.byref(n_steps)))
        out = np.zeros((n_sets.value, n_steps.value, 12), np.float32)
        if out.size:
            _chk(lib().stitch_rig_last_used_stats(self._h, _p(out), out.size, C.byref(n_sets), C.byref(n_steps)))
        return out

    def _stitch_fmt(self, sets, out, return_stats):
        """stitch() of a rig with a format set: stitch_dev_rig_stitch_fmt_u8."""
        in_fmt, out_fmt, _ = self.formats
        sets = [[f if isinstance(f, Image) else Image(PIX_PLANAR, f.shape[2], f.shape[1], _timg(f)) for f in fs] for fs in sets]
        if any(len(fs) != self.n_frames for fs in sets):
            raise ValueError(f"every set has {self.n_frames} frames")
        flat = [f for fs in sets for f in fs]
        if any(f.fmt != in_fmt for f in flat):
            raise ValueError(f"every frame is an Image of format {in_fmt}")
        n_sets = len(sets)
        ow, oh = self._out_size()
        if out is None:
            out = [Image.empty(out_fmt, ow, oh, flat[0].data.device) for _ in range(n_sets)]
        out = [o if isinstance(o, Image) else Image(PIX_PLANAR, o.shape[2], o.shape[1], _timg(o)) for o in out]
        if len(out) != n_sets or any((o.fmt, o.width, o.height) != (out_fmt, ow, oh) for o in out):
            raise ValueError(f"one {ow} x {oh} output Image of format {out_fmt} per set")
        status = (C.c_int32 * max(n_sets, 1))()
        seams = (Seam * max(n_sets * self.n_steps, 1))()
        stats = np.zeros((n_sets, self.n_steps, 12), np.float32) if return_stats else None
        rc = lib().stitch_dev_rig_stitch_fmt_u8(self._h, _image_array(flat), n_sets, _image_array(out), status, seams, _p(stats) if return_stats else None, _stream())
        statuses = list(status[:n_sets])
        seam_rows = [[seams[i * self.n_steps + k].as_tuple() for k in range(self.n_steps)] for i in range(n_sets)]
        self.last_rc = rc
        if rc < 0 and rc not in (ERR_EMPTY_MIDROW, ERR_ZERO_OVERLAP):
            raise StitchError(rc, lib().stitch_last_error().decode())
        return (out, statuses, seam_rows, stats) if return_stats else (out, statuses, seam_rows)

    def stitch(self, sets, out=None, return_stats=False):
        """With a format set (set_formats): stitch_dev_rig_stitch_fmt_u8 -- the frames are Images of in_fmt (a planar side also takes
        plain (3, H, W) tensors), the outputs come back as Images of out_fmt, allocated by image_bytes at tight pitch unless given as
        `out`; everything else as below.

        stitch_dev_rig_stitch_u8 on torch's current stream, which it waits for (with return_stats
        stitch_dev_rig_stitch_exposure_u8, and a fourth result: an (n_sets, n_steps, 12) float32 array of every transfer's
        statistics; the rig must have been made with an exposure mode).  sets: a list of frame sets, each a list of
        n_frames (3, H, W) uint8 device tensors.  Returns (outputs, statuses, seams): one (3, height, width) tensor per set -- with a
        crop set (set_crop) one (3, out_height, out_width) tensor, and `out` is checked against that shape --, each
        set's status (OK, ERR_EMPTY_MIDROW or ERR_ZERO_OVERLAP: a failed set does not raise, the others are valid), and per set the
        Seam tuples of its steps.  self.last_rc keeps the call's return value (the status of the first set that is not OK).
        Anything else -- a bad argument, a failed HIP call, a hand-off time-out -- raises StitchError."""
        import torch
        sets = [list(fs) for fs in sets]
        if self.formats[:2] != (0, 0):
            return self._stitch_fmt(sets, out, return_stats)
        flat = [f for fs in sets for f in fs]
        if any(len(fs) != self.n_frames for fs in sets):
            raise ValueError(f"every set has {self.n_frames} frames")
        flat, arr = _frames_u8(flat)
        n_sets = len(sets)
        # the crop's size while one is set (an A/B build of an earlier tree, STITCH_LIB, has no crop: the canvas)
        ow, oh = self._out_size() if hasattr(lib(), "stitch_rig_output_size") else (self.width, self.height)
        if out is None:
            out = [torch.empty((3, oh, ow), dtype=torch.uint8, device=flat[0].device) for _ in range(n_sets)]
        out = [_timg(o) for o in out]
        if len(out) != n_sets or any(tuple(o.shape) != (3, oh, ow) or o.dtype != torch.uint8 for o in out):
            raise ValueError(f"one (3, {oh}, {ow}) uint8 output per set")
        ptrs = (C.c_void_p * max(n_sets, 1))(*[o.data_ptr() for o in out])
        status = (C.c_int32 * max(n_sets, 1))()
        seams = (Seam * max(n_sets * self.n_steps, 1))()
        stats = np.zeros((n_sets, self.n_steps, 12), np.float32) if return_stats else None
        if return_stats:
            rc = lib().stitch_dev_rig_stitch_exposure_u8(self._h, arr, n_sets, ptrs, status, seams, _p(stats), _stream())
        else:
            rc = lib().stitch_dev_rig_stitch_u8(self._h, arr, n_sets, ptrs, status, seams, _stream())
        statuses = list(status[:n_sets])
        seam_rows = [[seams[i * self.n_steps + k].as_tuple() for k in range(self.n_steps)] for i in range(n_sets)]
        self.last_rc = rc
        if rc < 0 and rc not in (ERR_EMPTY_MIDROW, ERR_ZERO_OVERLAP):
            raise StitchError(rc, lib().stitch_last_error().decode())
        return (out, statuses, seam_rows, stats) if return_stats else (out, statuses, seam_rows)


# ---- a rig calibrated from several captures: include/stitch_calibrate.h -----------------------------------------------------
class CalibrateOpts(C.Structure):
    """stitch_calibrate_opts."""
    _fields_ = [("pano", C.c_void_p), ("pooled_threshold", C.c_int32)]


class Calibration(_Handle):
    """stitch_calibration: one stitch order and one set of steps from several captures of the same cameras (host data).
    start, width, height; steps: dicts with the keys of dev_panorama's steps (`src` is the WARPED camera, "mosaic_src" the one it is
    stitched to, "out" None, "seam" zeros); counts ((n_sets, n, n) int32) and pooled ((n, n)); support ((n_steps, n_sets, 2) int32:
    per step and capture the pairs it put into the chosen pooled list and its inliers of the forward map)."""
    _destroy = "stitch_calibration_destroy"

    def __init__(self, h):
        self._h = h
        L = lib()
        v = [C.c_int() for _ in range(6)]
        _chk(L.stitch_calibration_info(h, *[C.byref(x) for x in v]))
        self.n_sets, self.n, self.start, self.n_steps, self.width, self.height = (x.value for x in v)
        self.counts, self.pooled = np.zeros((self.n_sets, self.n, self.n), np.int32), np.zeros((self.n, self.n), np.int32)
        _chk(L.stitch_calibration_counts(h, _p(self.counts), _p(self.pooled)))
        self.support = np.zeros((self.n_steps, self.n_sets, 2), np.int32)
        self.steps = []
        for k in range(self.n_steps):
            s, pairs, inl = PanoramaStep(), np.zeros(self.n_sets, np.int32), np.zeros(self.n_sets, np.int32)
            _chk(L.stitch_calibration_step_at(h, k, C.byref(s)))
            _chk(L.stitch_calibration_step_support(h, k, _p(pairs), _p(inl)))
            self.support[k, :, 0], self.support[k, :, 1] = pairs, inl
            g = s.geom
            self.steps.append(dict(start=self.start, src=s.dst, mosaic_src=s.src, p=np.array(s.p_bwd[:]), p_fwd=np.array(s.p_fwd[:]), offx=g.min_x,
                                   offy=g.min_y, ox=g.ox, oy=g.oy, cw=g.cw, ch=g.ch, out=None, seam=s.seam.as_tuple(),
                                   info=np.array([list(s.info[0]), list(s.info[1])], np.int64)))


def _calibrate_opts(pooled_threshold, sift_opts, ransac_opts, kp_cap, feat_cap, ratio, match_threshold, fov_deg, keep):
    keep.append(_panorama_opts(None, True, 19.0, 20.0, sift_opts, ransac_opts, kp_cap, feat_cap, False, ratio, match_threshold, fov_deg, keep))
    return CalibrateOpts(C.addressof(keep[-1]), int(pooled_threshold))


def _capture_list(sets):
    sets = [list(fs) for fs in sets]
    if not sets or any(len(fs) != len(sets[0]) for fs in sets):
        raise ValueError("every capture has the same number of cameras")
    return sets


def dev_calibrate(sets, pooled_threshold=0, sift_opts=None, ransac_opts=None, kp_cap=4096, feat_cap=None, ratio=RATIO_THRESHOLD, match_threshold=20,
                  fov_deg=15.0):
    """stitch_dev_calibrate_u8: sets is a list of captures, each a list of the n cameras' (3, H, W) uint8 device tensors
    (unprojected; camera i has one size in every capture).  Returns a Calibration.  Runs on torch's current stream and waits for it.
    pooled_threshold 0: n_sets * match_threshold."""
    sets = _capture_list(sets)
    flat, arr = _frames_u8([f for fs in sets for f in fs])
    keep, h = [], C.c_void_p()
    o = _calibrate_opts(pooled_threshold, sift_opts, ransac_opts, kp_cap, feat_cap, ratio, match_threshold, fov_deg, keep)
    _chk(lib().stitch_dev_calibrate_u8(arr, len(sets), len(sets[0]), C.byref(o), _stream(), C.byref(h)))
    return Calibration(h)


def dev_calibrate_from_features(frame_sizes, features, pooled_threshold=0, ransac_opts=None, ratio=RATIO_THRESHOLD, match_threshold=20):
    """stitch_dev_calibrate_from_features_u8: frame_sizes = (width, height) per camera; features = per capture a list with, per
    camera, (descriptors (n, 128), x, y) float32 device tensors in map order, which are left unchanged."""
    features = _capture_list(features)
    wh = np.ascontiguousarray(np.array(frame_sizes, np.int32).reshape(-1, 2))
    if wh.shape[0] != len(features[0]):
        raise ValueError("one frame size per camera")
    flat = [f for fs in features for f in fs]
    fs = (FeatureSet * len(flat))(*[_feature_set(*f) for f in flat])
    keep, h = [], C.c_void_p()
    o = _calibrate_opts(pooled_threshold, None, ransac_opts, 4096, None, ratio, match_threshold, 15.0, keep)
    _chk(lib().stitch_dev_calibrate_from_features_u8(_p(wh), fs, len(features), len(features[0]), C.byref(o), _stream(), C.byref(h)))
    return Calibration(h)


def calibrate(sets, pooled_threshold=0, sift_opts=None, ransac_opts=None, kp_cap=4096, feat_cap=None, ratio=RATIO_THRESHOLD, match_threshold=20,
              fov_deg=15.0):
    """stitch_calibrate_u8: as dev_calibrate, from (3, H, W) uint8 HOST arrays."""
    sets = [[np.ascontiguousarray(_img(f), np.uint8) for f in fs] for fs in _capture_list(sets)]
    flat = [f for fs in sets for f in fs]
    arr = (FrameU8 * len(flat))(*[FrameU8(f.ctypes.data, f.shape[2], f.shape[1]) for f in flat])
    keep, h = [], C.c_void_p()
    o = _calibrate_opts(pooled_threshold, sift_opts, ransac_opts, kp_cap, feat_cap, ratio, match_threshold, fov_deg, keep)
    _chk(lib().stitch_calibrate_u8(arr, len(sets), len(sets[0]), C.byref(o), C.byref(h)))
    return Calibration(h)


def _ptr_table(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


# ---- a rig's alignment monitor: include/stitch_rig_monitor.h ------------------------------------------------------------------
def residual_words(radius):
    """stitch_residual_words (host only): the words of a record, 2 + 3 * (2 * radius + 1) ** 2; 0 for a radius outside 0 .. 8."""
    return lib().stitch_residual_words(int(radius))


def dev_pairs_residual(pairs, cw, ch, domains, radius):
    """stitch_dev_pairs_residual_u8 on torch's current stream, which it waits for.  pairs: (frame, p, offx, offy, mosaic, ox, oy)
    with (3, H, W) uint8 device tensors -- the inputs of a blend; domains: one (ch, cw) uint8 device mask per pair (non-zero = in the
    domain; the same tensor may serve several pairs).  Returns an (n, words) int64 device tensor of records: n, sum_b, then
    sum_a, sad, ssd per shift, dy-major (every value is below 2^51)."""
    import torch
    pairs, domains = list(pairs), list(domains)
    if len(domains) != len(pairs) or not pairs:
        raise ValueError("one domain per pair, and at least one pair")
    arr = (PairDesc * len(pairs))()
    for d, it in zip(arr, pairs):
        frame, p, offx, offy, mosaic, ox, oy = it[:7]
        frame, mosaic = _timg(frame), _timg(mosaic)
        if frame.dtype != torch.uint8 or mosaic.dtype != torch.uint8:
            raise TypeError("expected uint8 images")
        d.frame, d.fw, d.fh = frame.data_ptr(), frame.shape[2], frame.shape[1]
        d.p = _map8(p)
        d.offx, d.offy = float(offx), float(offy)
        d.mosaic, d.mw, d.mh = mosaic.data_ptr(), mosaic.shape[2], mosaic.shape[1]
        d.ox, d.oy = int(ox), int(oy)
    for m in domains:
        if not m.is_cuda or not m.is_contiguous() or m.dtype != torch.uint8 or tuple(m.shape) != (ch, cw):
            raise ValueError(f"every domain is a contiguous ({ch}, {cw}) uint8 device mask")
    words = residual_words(radius)
    rec = torch.empty((len(pairs), max(words, 1)), dtype=torch.int64, device=pairs[0][0].device)
    _chk(lib().stitch_dev_pairs_residual_u8(arr, len(pairs), int(cw), int(ch), _ptr_table(domains), int(radius), _dp(rec), _stream()))
    return rec


# ---- path seams: include/stitch_seam_path.h -----------------------------------------------------------------------------------
class SeamPathOpts(C.Structure):
    """stitch_seam_path_opts: the step bound K (1 .. 8) and the coverage margin m (0 .. 64) of the finder."""
    _fields_ = [("max_step", C.c_int32), ("margin", C.c_int32)]

    def __init__(self, max_step=2, margin=8):
        super().__init__(max_step, margin)


# ---- temporally anchored path seams: include/stitch_seam_anchor.h ---------------------------------------------------------------
SEAM_ANCHOR_MAX, SEAM_ANCHOR_PER_SET, SEAM_ANCHOR_PER_CALL = 2055, 1, 2


class SeamAnchorOpts(C.Structure):
    """stitch_seam_anchor_opts: the weight w and the cap T of the temporal term w * min(|s - r|, T), and a rig's policy.  No defaults."""
    _fields_ = [("weight", C.c_int32), ("cap", C.c_int32), ("policy", C.c_int32)]


def dev_pairs_seam_path(pairs, cw, ch, cov_a, cov_b, branches, max_step=2, margin=8, anchors=None, weight=None, cap=None):
    """stitch_dev_pairs_seam_path_u8 on torch's current stream, which it waits for.  pairs: (frame, p, offx, offy, mosaic, ox, oy)
    with (3, H, W) uint8 device tensors -- the inputs of a blend; cov_a, cov_b: per pair a (ch, cw) uint8 device mask of where the
    warped frame / the moved mosaic can have data (non-zero = covered; tensors may serve several pairs); branches: per pair 0 or 1.
    Returns (paths, costs): an (n, ch) int32 and an (n,) int64 device tensor -- the least-cost seam column of every row, and its cost.
    anchors (with weight and cap): stitch_dev_pairs_seam_path_anchored_u8 (include/stitch_seam_anchor.h) -- per pair a (ch,) int32
    device tensor or None (that pair is unanchored); returns (paths, costs, moved), moved an (n,) int64 device tensor."""
    import torch
    pairs, cov_a, cov_b, branches = list(pairs), list(cov_a), list(cov_b), [int(b) for b in branches]
    if not pairs or not len(cov_a) == len(cov_b) == len(branches) == len(pairs):
        raise ValueError("two masks and a branch per pair, and at least one pair")
    arr = (PairDesc * len(pairs))()
    for d, it in zip(arr, pairs):
        frame, p, offx, offy, mosaic, ox, oy = it[:7]
        frame, mosaic = _timg(frame), _timg(mosaic)
        if frame.dtype != torch.uint8 or mosaic.dtype != torch.uint8:
            raise TypeError("expected uint8 images")
        d.frame, d.fw, d.fh = frame.data_ptr(), frame.shape[2], frame.shape[1]
        d.p = _map8(p)
        d.offx, d.offy = float(offx), float(offy)
        d.mosaic, d.mw, d.mh = mosaic.data_ptr(), mosaic.shape[2], mosaic.shape[1]
        d.ox, d.oy = int(ox), int(oy)
    for m in cov_a + cov_b:
        if not m.is_cuda or not m.is_contiguous() or m.dtype != torch.uint8 or tuple(m.shape) != (ch, cw):
            raise ValueError(f"every coverage mask is a contiguous ({ch}, {cw}) uint8 device mask")
    dev = pairs[0][0].device
    paths = torch.empty((len(pairs), ch), dtype=torch.int32, device=dev)
    costs = torch.empty((len(pairs),), dtype=torch.int64, device=dev)
    o = SeamPathOpts(int(max_step), int(margin))
    if anchors is not None:
        anchors = list(anchors)
        if weight is None or cap is None or len(anchors) != len(pairs):
            raise ValueError("anchors come with a weight and a cap, one entry (a tensor or None) per pair")
        for a in anchors:
            if a is not None and (not a.is_cuda or not a.is_contiguous() or a.dtype != torch.int32 or a.numel() != ch):
                raise ValueError(f"every anchor is a contiguous ({ch},) int32 device tensor, or None")
        moved = torch.empty((len(pairs),), dtype=torch.int64, device=dev)
        tab = (C.c_void_p * len(pairs))(*[None if a is None else a.data_ptr() for a in anchors])
        _chk(lib().stitch_dev_pairs_seam_path_anchored_u8(arr, len(pairs), int(cw), int(ch), _ptr_table(cov_a), _ptr_table(cov_b), (C.c_int32 * len(pairs))(*branches),
                                                          C.byref(o), tab, C.byref(SeamAnchorOpts(int(weight), int(cap), 0)), _dp(paths), _dp(costs), _dp(moved), _stream()))
        return paths, costs, moved
    _chk(lib().stitch_dev_pairs_seam_path_u8(arr, len(pairs), int(cw), int(ch), _ptr_table(cov_a), _ptr_table(cov_b), (C.c_int32 * len(pairs))(*branches),
                                             C.byref(o), _dp(paths), _dp(costs), _stream()))
    return paths, costs


def residual_best_shift(record, radius, zero_mean=False):
    """stitch_residual_best_shift (host only): (dx, dy) of the shift a record favours -- the least ssd, or with zero_mean the least
    n * ssd - (sum_a - sum_b) ** 2, compared exactly; ties to the shortest shift, then the smallest dy, then the smallest dx.
    Raises StitchError(ERR_ZERO_OVERLAP) for a record with n == 0."""
    rec = np.ascontiguousarray(np.asarray(record.cpu() if hasattr(record, "cpu") else record).astype(np.uint64).reshape(-1))
    if rec.size != residual_words(radius) or not rec.size:
        raise ValueError(f"a record of radius {radius} has {residual_words(radius)} words, got {rec.size}")
    dx, dy = C.c_int(), C.c_int()
    _chk(lib().stitch_residual_best_shift(_p(rec), int(radius), int(bool(zero_mean)), C.byref(dx), C.byref(dy)))
    return dx.value, dy.value


def dev_project_many(srcs, fov_deg=15.0, out=None):
    """stitch_dev_project_many_u8: same-size (3, H, W) uint8 device tensors through ONE projection launch -> list of tensors."""
    import torch
    srcs = [_timg(t) for t in srcs]
    out = [torch.empty_like(t) for t in srcs] if out is None else list(out)
    _, h, w = srcs[0].shape
    if any(tuple(t.shape) != (3, h, w) or t.dtype != torch.uint8 for t in srcs + out) or len(out) != len(srcs):
        raise ValueError("expected uint8 images of one size, and one output per image")
    _chk(lib().stitch_dev_project_many_u8(_ptr_table(srcs), _ptr_table(out), len(srcs), w, h, fov_deg, _stream()))
    return out


def dev_finish_many(results, num=19.0, den=20.0):
    """stitch_dev_finish_many_u8: the finish pass on same-size (3, H, W) uint8 device tensors, in place, in three launches."""
    import torch
    results = [_timg(t) for t in results]
    _, h, w = results[0].shape
    if any(tuple(t.shape) != (3, h, w) or t.dtype != torch.uint8 for t in results):
        raise ValueError("expected uint8 mosaics of one size")
    _chk(lib().stitch_dev_finish_many_u8(_ptr_table(results), len(results), w, h, num, den, _stream()))
    return results


def dev_transfer_many(srcs, tems, out=None, stats_form=2, keep_black=False, want_stats=False, want_diag=False):
    """stitch_dev_transfer_many_u8: the colour transfer of many (source, template) pairs in the launches of one -- all sources of
    one size, all templates of one size, (3, H, W) uint8 device tensors; out[i] may be srcs[i].  Returns the outputs, with
    want_stats also a (count, 12) float32 device tensor, with want_diag also a (count, 6, 4) int32 tensor of STATS_DIAG counters."""
    import torch
    srcs, tems = [_timg(t) for t in srcs], [_timg(t) for t in tems]
    out = [torch.empty_like(t) for t in srcs] if out is None else list(out)
    (_, sh, sw), (_, th, tw) = srcs[0].shape, tems[0].shape
    if any(tuple(t.shape) != (3, sh, sw) or t.dtype != torch.uint8 for t in srcs + out) or any(tuple(t.shape) != (3, th, tw) or t.dtype != torch.uint8 for t in tems) \
            or not len(srcs) == len(tems) == len(out):
        raise ValueError("expected uint8 sources of one size, templates of one size, and one template and one output per source")
    n, dev = len(srcs), srcs[0].device
    stats = torch.zeros((n, 12), dtype=torch.float32, device=dev) if want_stats else None
    diag = torch.zeros((n, 6, len(STATS_DIAG)), dtype=torch.int32, device=dev) if want_diag else None
    _chk(lib().stitch_dev_transfer_many_u8(_ptr_table(srcs), _ptr_table(tems), _ptr_table(out), n, sw, sh, tw, th, int(stats_form), int(bool(keep_black)),
                                           _dp(stats), _dp(diag), _stream()))
    return (out,) + ((stats,) if want_stats else ()) + ((diag,) if want_diag else ()) if (want_stats or want_diag) else out


# ---- temporal exposure: include/stitch_rig_exposure_temporal.h ------------------------------------------------------------------
def dev_transfer_given_many(srcs, stats, out=None, keep_black=False):
    """stitch_dev_transfer_given_many_u8: the colour transfer's apply pass with GIVEN statistics on same-size (3, H, W) uint8 device
    tensors in one launch -- image i recoloured with stats[i], a (count, 12) float32 device tensor; out[i] may be srcs[i].  No
    template and no float plane is involved.  Returns the outputs."""
    import torch
    srcs = [_timg(t) for t in srcs]
    out = [torch.empty_like(t) for t in srcs] if out is None else list(out)
    _, h, w = srcs[0].shape
    if any(tuple(t.shape) != (3, h, w) or t.dtype != torch.uint8 for t in srcs + out) or len(out) != len(srcs):
        raise ValueError("expected uint8 images of one size, and one output per image")
    if not stats.is_cuda or stats.dtype != torch.float32 or not stats.is_contiguous() or tuple(stats.shape) != (len(srcs), 12):
        raise ValueError("expected a contiguous (count, 12) float32 tensor of statistics on the HIP device")
    _chk(lib().stitch_dev_transfer_given_many_u8(_ptr_table(srcs), _ptr_table(out), len(srcs), w, h, _dp(stats), int(bool(keep_black)), _stream()))
    return out


def dev_stats_filter(measured, keep, state, has, out=None):
    """stitch_dev_stats_filter_f32: the first-order filter over the (count, 12) float32 device tensor `measured`, record after record;
    state: (12,) float32 and has: (1,) int32 device tensors, read and rewritten.  Returns the (count, 12) used records (`out`, which
    may be `measured`).  Enqueued on torch's current stream."""
    import torch
    out = torch.empty_like(measured) if out is None else out
    for t, shape, dt in ((measured, None, torch.float32), (out, tuple(measured.shape), torch.float32), (state, (12,), torch.float32), (has, (1,), torch.int32)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise ValueError("expected contiguous device tensors: measured and out (count, 12) float32, state (12,) float32, has (1,) int32")
    if measured.dim() != 2 or measured.shape[1] != 12:
        raise ValueError("measured: (count, 12)")
    _chk(lib().stitch_dev_stats_filter_f32(_dp(measured), measured.shape[0], int(keep), _dp(state), _dp(has), _dp(out), _stream()))
    return out
