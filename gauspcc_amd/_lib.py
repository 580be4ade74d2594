"""ctypes binding of libgauspcc.so (C ABI: include/gauspcc.h).

There is no CPU fallback: importing a symbol from here without the built HIP library,
or calling it without an MI355X, raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GAUSPCC_LIB") or os.path.join(_HERE, "libgauspcc.so")  # env override: kernel-variant experiments (tools/)

_lib = None


class GpccError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libgauspcc error {code}: {msg}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [
        ("num_points", C.c_int64),
        ("num_bytes", C.c_int64),
        ("num_levels", C.c_int32),
        ("flags", C.c_int32),
        ("level_nodes", C.c_int64 * 24),
        ("coded_nodes", C.c_int64),
        ("conv_pairs", C.c_int64),
        ("device_ms", C.c_double),
        ("ideal_bits", C.c_double),
    ]


class Profile(C.Structure):
    _fields_ = [("conv_ms", C.c_double), ("conv_launches", C.c_int64), ("conv_pair_jobs", C.c_int64),
                ("fused_ms", C.c_double), ("fused_launches", C.c_int64), ("fused_pair_jobs", C.c_int64)]


class Stage(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_double), ("bytes", C.c_double), ("brackets", C.c_int64), ("critical_ms", C.c_double)]


class ChainStage(C.Structure):
    """gsac_chain_stage (include/gauspcc.h): one stage of gsac_decode_normal_chain"""
    _fields_ = [(k, C.c_int32) for k in ("ch", "dep_ch", "dh", "lag", "mean_col", "scale_col", "feat_col", "out_col", "out_pitch", "keep_group")] + \
               [(k, C.c_void_p) for k in ("w1", "b1", "w2", "b2", "q_dev", "out_dev", "keep_dev", "bytes")] + \
               [("nbytes", C.c_int64), ("cnt", C.c_void_p), ("min_value", C.c_void_p), ("max_value", C.c_void_p)]


class RateStage(C.Structure):
    """gsac_rate_stage (include/gauspcc.h): one stage of gsac_chain_rate_forward / _backward"""
    _fields_ = [(k, C.c_int32) for k in ("attr", "col", "ch", "mean_col", "scale_col")] + [("res", C.c_void_p)]


GSR_STATE_WORDS = 16                                       # include/gauspcc.h
GPCC_TRAIN_STATE_WORDS = 256                               # include/gauspcc.h
GSR_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)   # gsr_alloc_fn: device memory for the training paths (frame state, backward workspace)

EXPORTS = [
    "gpcc_last_error", "gpcc_version", "gpcc_ctx_create", "gpcc_ctx_destroy", "gpcc_ctx_bytes", "gpcc_ctx_set_container_version", "gpcc_raster_order", "gpcc_voxelise",
    "gpcc_model_create", "gpcc_model_destroy", "gpcc_encode", "gpcc_decode", "gpcc_decode_to", "gpcc_encode_batch", "gpcc_decode_batch", "gpcc_sort_zyx",
    "gpcc_build_octree", "gpcc_conv3d", "gpcc_head_cdf", "gpcc_rc_encode", "gpcc_rc_decode", "gpcc_memcpy_d2d",
    "gpcc_profile_enable", "gpcc_profile_get", "gpcc_profile_stages", "gpcc_debug_trace_enable", "gpcc_debug_trace_get", "gpcc_debug_capture", "gpcc_debug_capture_get", "gpcc_debug_exclusive_scan", "gpcc_debug_launches", "gpcc_device_error_check",
    "gsac_calculate_cdf", "gsac_encode", "gsac_decode", "gsac_encode_u16", "gsac_decode_u16", "gsac_encode_const", "gsac_decode_const", "gsac_host_encode_u16", "gsac_host_decode_u16", "gsac_host_encode_f32", "gsac_host_decode_f32", "gpcc_write_files", "gpcc_read_files", "gsac_encode_gaussian", "gsac_decode_gaussian", "gsac_encode_gaussian_mixed", "gsac_decode_gaussian_mixed", "gsac_calculate_cdf_mixed", "gsac_encode_gaussian_slices", "gsac_decode_gaussian_slices", "gsac_encode_gaussian_mixed_slices", "gsac_decode_gaussian_mixed_slices", "gshac_mlp2", "gshac_mlp2_act", "gsge_forward", "gsge_forward_train", "gsge_backward", "gsr_visible_filter", "gsr_forward", "gsr_forward_train", "gsr_backward", "gsnn_generate", "gsnn_forward_train", "gsnn_backward", "gsnn_noise_forward", "gsnn_noise_backward", "gsnn_noise_forward_b", "gsnn_noise_backward_b", "gsnn_quantise", "gsnn_mean",
    "gpcc_train_frame", "gpcc_train_frame_nodes", "gpcc_train_weights", "gpcc_train_conv", "gpcc_train_wgrad",
    "gpcc_knn", "gpcc_scatter_max", "gpcc_grow_voxels",
    "gpcc_densify_stats", "gpcc_densify_front", "gpcc_densify_finish", "gpcc_compact_rows", "gpcc_expand_rows",
    "gsr_forward_aux", "gsr_forward_train_aux", "gsr_backward_aux",
    "gsr_ssim_forward", "gsr_ssim_backward",
    "gsr_wavelet_l1_forward", "gsr_wavelet_l1_backward", "gsr_haar_forward", "gsr_haar_inverse",
    "gsr_sh_forward", "gsr_sh_backward",
    "gsac_rate_forward", "gsac_rate_backward", "gsac_chain_rate_forward", "gsac_chain_rate_backward",
    "gsge_plane_forward", "gsge_plane_backward", "gsge_plane_rows_forward", "gsge_plane_rows_backward",
    "gsge_msplane_forward", "gsge_msplane_backward",
    "gshac_mlp2_backward", "gshac_mlp2_slab_rows",
    "gsac_arm_encode", "gsac_arm_decode", "gsac_arm_cdf_rows",
    "gsac_normal_cdf_rows", "gsac_encode_normal_streams", "gsac_decode_normal_streams", "gsac_decode_normal_chain",
]
# the tri-plane ARM's entry points: listed apart because tests/test_abi.py matches EXPORTS against the header with a pattern of the
# prefixes above; tests/test_arm_ref_cpu.py checks these against the header and the library
EXPORTS_ARM = ["gsarm_rate_forward", "gsarm_rate_backward"]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C gauspcc_amd/csrc). gauspcc_amd has no CPU fallback."
        )
    # torch first: the library and torch must share ONE HIP runtime (torch ships its own libamdhip64; a process that loads
    # /opt/rocm's copy through this library before torch's ends up with two, and the second finds no device)
    import torch  # noqa: F401

    L = C.CDLL(LIB_PATH)
    vp, i64, i32, u16 = C.c_void_p, C.c_int64, C.c_int, C.c_uint16
    L.gpcc_last_error.restype = C.c_char_p
    L.gpcc_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.gpcc_ctx_destroy.argtypes = [vp]
    L.gpcc_ctx_destroy.restype = None
    L.gpcc_ctx_bytes.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.gpcc_ctx_set_container_version.argtypes = [vp, i32]
    L.gpcc_raster_order.argtypes = [vp, vp, i32, i64, vp, vp]
    L.gpcc_voxelise.argtypes = [vp, vp, i32, i64, C.c_double, C.c_double, C.c_double, i32, vp, vp]
    L.gpcc_model_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.gpcc_model_destroy.argtypes = [vp]
    L.gpcc_model_destroy.restype = None
    L.gpcc_encode.argtypes = [vp, vp, vp, i64, i32, u16, C.POINTER(vp), C.POINTER(i64), C.POINTER(Stats), vp]
    L.gpcc_decode.argtypes = [vp, vp, vp, i64, C.POINTER(vp), C.POINTER(i64), C.POINTER(u16), C.POINTER(Stats), vp]
    L.gpcc_encode_batch.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(i64), i32, i32, C.POINTER(u16), C.POINTER(vp), C.POINTER(i64), C.POINTER(Stats), C.POINTER(i32), vp]
    L.gpcc_decode_batch.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(i64), i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.POINTER(u16), C.POINTER(Stats), C.POINTER(i32), vp]
    L.gpcc_decode_to.argtypes = [vp, vp, vp, i64, vp, i64, C.POINTER(i64), C.POINTER(u16), C.POINTER(Stats), vp]
    L.gpcc_sort_zyx.argtypes = [vp, vp, i64, vp, vp]
    L.gpcc_build_octree.argtypes = [vp, vp, i64, C.POINTER(i32), C.POINTER(i64), vp, vp, i64, vp]
    L.gpcc_conv3d.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, i32, vp, C.POINTER(i64), vp]
    L.gpcc_head_cdf.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.gpcc_rc_encode.argtypes = [vp, vp, i32, vp, i64, i32, C.POINTER(vp), C.POINTER(i64), vp]
    L.gpcc_rc_decode.argtypes = [vp, vp, i32, vp, i64, i64, i32, vp, vp]
    L.gpcc_memcpy_d2d.argtypes = [vp, vp, vp, i64, vp]
    L.gpcc_profile_enable.argtypes = [vp, i32]
    L.gpcc_debug_trace_enable.argtypes = [vp, i32]
    L.gpcc_debug_trace_get.argtypes = [vp, vp, vp, i32]
    L.gpcc_debug_capture.argtypes = [vp, i32]
    L.gpcc_debug_capture_get.restype = C.c_longlong
    L.gpcc_debug_capture_get.argtypes = [vp, i32, vp, C.c_longlong]
    L.gpcc_debug_exclusive_scan.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp]
    L.gpcc_debug_launches.argtypes = [i32]
    L.gpcc_device_error_check.argtypes = [vp]
    L.gpcc_debug_launches.restype = C.c_longlong
    L.gpcc_profile_get.argtypes = [vp, C.POINTER(Profile)]
    L.gpcc_profile_stages.argtypes = [vp, C.POINTER(Stage), i32, C.POINTER(i32)]
    L.gsac_calculate_cdf.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp]
    L.gsac_encode.argtypes = [vp, vp, vp, i32, i64, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), vp]
    L.gsac_decode.argtypes = [vp, vp, vp, i64, vp, i32, i64, i32, vp, vp]
    L.gsac_encode_u16.argtypes = L.gsac_encode.argtypes
    L.gsac_decode_u16.argtypes = L.gsac_decode.argtypes
    L.gsac_encode_const.argtypes = L.gsac_encode.argtypes
    L.gsac_decode_const.argtypes = L.gsac_decode.argtypes
    L.gsac_host_encode_u16.argtypes = [vp, vp, i64, i32, vp, i64, C.POINTER(i64)]
    L.gsac_host_decode_u16.argtypes = [vp, vp, i64, i64, i32, vp]
    L.gsac_host_encode_f32.argtypes = L.gsac_host_encode_u16.argtypes
    L.gsac_host_decode_f32.argtypes = L.gsac_host_decode_u16.argtypes
    L.gpcc_write_files.argtypes = [vp, vp, vp, i32, i32]
    L.gpcc_read_files.argtypes = [vp, i32, i32, C.POINTER(vp), vp]
    fp = C.POINTER(C.c_float)
    L.gsac_encode_gaussian.argtypes = [vp, vp, vp, vp, vp, i64, i32, fp, fp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), vp]
    L.gsac_decode_gaussian.argtypes = [vp, vp, vp, vp, i64, C.c_float, C.c_float, vp, i64, vp, i32, vp, vp]
    L.gsac_encode_gaussian_mixed.argtypes = [vp, vp, vp, vp, vp, i32, vp, i64, i32, fp, fp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), vp]
    L.gsac_decode_gaussian_mixed.argtypes = [vp, vp, vp, vp, i32, vp, i64, C.c_float, C.c_float, vp, i64, vp, i32, vp, vp]
    L.gsac_calculate_cdf_mixed.argtypes = [vp, vp, vp, vp, i32, vp, i64, i32, i32, vp, vp]
    L.gsac_encode_gaussian_slices.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), vp]
    L.gsac_decode_gaussian_slices.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, vp, i32, vp, vp]
    L.gshac_mlp2.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, vp]
    L.gshac_mlp2_act.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, C.c_float, vp, vp]
    L.gsac_encode_gaussian_mixed_slices.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), vp]
    L.gsac_decode_gaussian_mixed_slices.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i64, vp, i32, vp, vp]
    L.gsge_forward.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp]
    L.gsge_forward_train.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp]
    L.gsge_backward.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, i32, i32, i32, i32, vp, vp, GSR_ALLOC, vp, vp]
    f32 = C.c_float
    L.gsr_visible_filter.argtypes = [vp, i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, f32, f32, i32, vp, vp]
    L.gsr_forward.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, f32, f32, i32, vp, vp, C.POINTER(i64), vp]
    L.gsr_forward_train.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, f32, f32, i32, vp, vp, GSR_ALLOC, vp,
                                    C.POINTER(C.c_uint64), C.POINTER(i64), vp]
    L.gsr_backward.argtypes = [vp, C.POINTER(C.c_uint64), i32, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, f32, f32, vp, vp, GSR_ALLOC, vp,
                               vp, vp, vp, vp, vp, vp, vp, vp]
    # the _aux forms: out_invdepth, out_alpha after radii; dL_dinvdepth, dL_dalpha after dL_dout
    L.gsr_forward_aux.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, vp, C.POINTER(i64), vp]
    L.gsr_forward_train_aux.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, vp, GSR_ALLOC, vp,
                                        C.POINTER(C.c_uint64), C.POINTER(i64), vp]
    L.gsr_backward_aux.argtypes = [vp, C.POINTER(C.c_uint64), i32, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, GSR_ALLOC, vp,
                                   vp, vp, vp, vp, vp, vp, vp, vp]
    L.gsnn_generate.argtypes = [vp, i64, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), vp]
    L.gsnn_forward_train.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, GSR_ALLOC, vp, C.POINTER(vp),
                                     C.POINTER(i64), vp]
    L.gsnn_backward.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, GSR_ALLOC, vp, vp]
    st = C.POINTER(C.c_uint64)
    L.gpcc_train_frame.argtypes = [vp, vp, i64, i32, GSR_ALLOC, vp, st, C.POINTER(i32), C.POINTER(i64), vp]
    L.gpcc_train_frame_nodes.argtypes = [vp, st, vp, vp, vp, vp, vp]
    L.gpcc_train_weights.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.gpcc_train_conv.argtypes = [vp, st, i32, vp, vp, vp, i32, vp, vp]
    L.gpcc_train_wgrad.argtypes = [vp, st, i32, vp, vp, GSR_ALLOC, vp, vp, vp]
    L.gpcc_knn.argtypes = [vp, vp, i64, i32, vp, vp, vp, GSR_ALLOC, vp, vp]
    L.gpcc_scatter_max.argtypes = [vp, vp, vp, i64, i64, i64, i32, vp, vp, GSR_ALLOC, vp, vp]
    L.gpcc_grow_voxels.argtypes = [vp, vp, i64, vp, vp, i64, i64, vp, i64, f32, f32, C.POINTER(i64), GSR_ALLOC, vp, vp]
    L.gpcc_densify_stats.argtypes = [vp, i64, i32, vp, vp, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, GSR_ALLOC, vp, vp]
    L.gpcc_densify_front.argtypes = [vp, vp, vp, i64, f32, vp, vp, vp]
    L.gpcc_densify_finish.argtypes = [vp, vp, vp, vp, i64, i32, vp, vp, i64, f32, f32, vp, C.POINTER(i64), GSR_ALLOC, vp, vp]
    L.gpcc_compact_rows.argtypes = [vp, vp, i64, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), GSR_ALLOC, vp, vp]
    L.gpcc_expand_rows.argtypes = [vp, vp, i64, i64, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), GSR_ALLOC, vp, vp]
    dp = C.POINTER(C.c_double)
    L.gsnn_noise_forward.argtypes = [vp, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), dp, vp, i64, C.POINTER(i32), C.POINTER(vp), vp, vp]
    L.gsnn_noise_backward.argtypes = [vp, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), dp, vp, i64, C.POINTER(i32), vp, vp, vp]
    L.gsnn_noise_forward_b.argtypes = [vp, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), dp, vp, i64, C.POINTER(i32), C.c_double, C.POINTER(vp), vp, vp]
    L.gsnn_noise_backward_b.argtypes = [vp, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), dp, vp, i64, C.POINTER(i32), C.c_double, vp, vp, vp]
    L.gsnn_quantise.argtypes = [vp, i64, i32, C.POINTER(vp), C.POINTER(i64), dp, vp, i64, C.POINTER(i32), C.c_double, vp, i32, C.POINTER(vp), vp, vp]
    L.gsnn_mean.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i64), vp, vp, vp]
    L.gsr_ssim_forward.argtypes = [vp, vp, vp, i64, i64, i64, i64, i32, fp, i32, vp, vp, vp, C.c_double, vp, i32, GSR_ALLOC, vp, vp]
    L.gsr_ssim_backward.argtypes = [vp, vp, vp, i64, i64, i64, i64, i32, fp, i32, vp, i32, vp, f32, vp, f32, vp, vp, vp]
    L.gsr_wavelet_l1_forward.argtypes = [vp, vp, vp, i64, i64, i64, dp, vp, vp, GSR_ALLOC, vp, vp]
    L.gsr_wavelet_l1_backward.argtypes = [vp, vp, vp, i64, i64, i64, dp, vp, vp, vp, vp]
    L.gsr_haar_forward.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
    L.gsr_haar_inverse.argtypes = [vp, vp, vp, i64, i64, i64, vp, i64, i64, vp]
    L.gsr_sh_forward.argtypes = [vp, i32, i32, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    L.gsr_sh_backward.argtypes = [vp, i32, i32, i32, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, vp]
    pp, ip, f64 = C.POINTER(vp), C.POINTER(i32), C.c_double
    L.gsac_rate_forward.argtypes = [vp, i32, i64, i64, vp, vp, pp, pp, pp, ip, vp, i32, f64, f64, i32, vp, vp]
    L.gsac_rate_backward.argtypes = [vp, i32, i64, i64, vp, vp, pp, pp, pp, ip, vp, i32, f64, f64, i32, vp, vp, pp, pp, pp, vp, GSR_ALLOC, vp, vp]
    chain = [vp, i64, i32, i32, vp, i64, i32, vp, vp, vp, vp, vp, f64, vp, C.POINTER(RateStage), i32]
    L.gsac_chain_rate_forward.argtypes = chain + [vp, vp]
    L.gsac_chain_rate_backward.argtypes = chain + [vp, vp, vp, vp, vp, pp, vp, vp, vp]
    L.gsge_plane_forward.argtypes = [vp, vp, vp, vp, vp, f64, i64, i32, i32, i32, i32, i32, vp, GSR_ALLOC, vp, vp]
    L.gsge_plane_backward.argtypes = [vp, vp, vp, vp, vp, vp, f64, i64, i32, i32, i32, i32, i32, vp, vp, GSR_ALLOC, vp, vp]
    L.gsge_plane_rows_forward.argtypes = [vp, vp, vp, vp, vp, f64, i64, i32, i32, i32, i32, i32, vp, i32, vp, GSR_ALLOC, vp, vp]
    L.gsge_plane_rows_backward.argtypes = [vp, vp, vp, vp, vp, vp, f64, i64, i32, i32, i32, i32, i32, i32, vp, vp, GSR_ALLOC, vp, vp]
    L.gsge_msplane_forward.argtypes = [vp, vp, i64, i32, pp, i32, ip, ip, i32, i32, i32, vp, vp, vp, vp, vp, vp, GSR_ALLOC, vp, vp]
    L.gsge_msplane_backward.argtypes = [vp, vp, vp, i64, i32, pp, i32, ip, ip, i32, i32, i32, vp, vp, vp, vp, vp, pp, vp, GSR_ALLOC, vp, vp]
    L.gshac_mlp2_backward.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, GSR_ALLOC, vp, vp]
    L.gshac_mlp2_slab_rows.argtypes = [i64, i32, i32, i32]
    L.gshac_mlp2_slab_rows.restype = i64
    L.gsarm_rate_forward.argtypes = [vp, i32, pp, ip, ip, ip, vp, i32, ip, vp, vp, vp, vp, GSR_ALLOC, vp, vp]
    L.gsarm_rate_backward.argtypes = [vp, i32, pp, ip, ip, ip, vp, i32, ip, vp, i32, pp, vp, GSR_ALLOC, vp, vp]
    L.gsac_arm_encode.argtypes = [vp, i32, pp, ip, ip, ip, ip, vp, i32, ip, ip, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64), vp]
    L.gsac_arm_decode.argtypes = [vp, i32, pp, ip, ip, ip, ip, ip, vp, i32, ip, vp, i64, vp, i64, vp]
    L.gsac_arm_cdf_rows.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.gsac_normal_cdf_rows.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp]
    L.gsac_encode_normal_streams.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), vp]
    L.gsac_decode_normal_streams.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp]
    L.gsac_decode_normal_chain.argtypes = [vp, C.POINTER(ChainStage), i32, vp, i32, i64, i32, i32, i32, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise GpccError(rc, lib().gpcc_last_error().decode(errors="replace"))
