"""ctypes binding of include/gpsgs.h.  No fallback: a missing library is an ImportError with build instructions."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPSGS_LIB") or os.path.join(_HERE, "lib", "libgpsgs_hip.so")  # GPSGS_LIB: development (another build of the same library)

GPSGS_OK, GPSGS_E_INVALID, GPSGS_E_WORKSPACE, GPSGS_E_LAUNCH, GPSGS_E_NO_DEVICE, GPSGS_E_INTERNAL = 0, -1, -2, -3, -4, -5
_ERR = {-1: "invalid argument", -2: "workspace too small", -3: "HIP launch failed", -4: "no HIP device",
        -5: "internal self-check failed (debug mode: inconsistent bin lists)"}
GSR_FLAG_DEBUG = 1
GSR_FLAG_NO_LARGE_SORT = 4
GSR_FLAG_TIMING = 2
GSR_FLAG_COMPOSITE_TILES = 8
GSR_FLAG_NO_COLOR_GRAD = 256
GSR_FLAG_WAVE_PRIORITY = 512
GSR_FLAG_ANTIALIAS = 1024
GSR_MAX_FEATURES = 64
STAGES = ("preprocess", "scan", "scatter", "sort", "composite_fwd", "composite_bwd", "preprocess_bwd")


class GsrStrided(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("batch_stride", C.c_int64), ("pixel_stride", C.c_int64), ("channel_stride", C.c_int64)]


class GsrHeader(C.Structure):
    _fields_ = [("num_rendered", C.c_uint64), ("overflow", C.c_uint32), ("max_tile_count", C.c_uint32),
                ("num_busy_wgs", C.c_uint32), ("num_slots", C.c_uint32), ("num_points", C.c_uint32), ("row_overflow", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


class _DepthSlot(C.Union):
    _fields_ = [("out_depth", C.c_void_p), ("dL_ddepth", C.c_void_p)]


class _AlphaSlot(C.Union):
    _fields_ = [("out_alpha", C.c_void_p), ("dL_dalpha", C.c_void_p)]


class GsrViewExt(C.Structure):
    """Optional extras of one view (include/gpsgs.h): device pointer to the {begin, end} row range, work-order hint, (ABI 3) the SH-colour /
    precomputed-covariance inputs of the upstream interface with their gradient outputs, and the opt-in depth / alpha maps: out_depth / out_alpha
    (forward) share their slots with dL_ddepth / dL_dalpha (backward)."""
    _anonymous_ = ("_depth", "_alpha")
    _fields_ = [("row_range", C.c_void_p), ("order_hint", C.c_uint32), ("sh_degree", C.c_uint32), ("sh_coeffs", C.c_uint32), ("bin_capacity", C.c_uint32),
                ("shs", C.c_void_p), ("campos", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("dL_dsh", C.c_void_p), ("dL_dcov3D", C.c_void_p),
                ("_depth", _DepthSlot), ("_alpha", _AlphaSlot)]


class _FeatureMapSlot(C.Union):
    _fields_ = [("out_features", C.c_void_p), ("dL_dfeaturemap", C.c_void_p)]


class GsrFeatures(C.Structure):
    """F-channel feature maps of one view (include/gpsgs.h): channels (0 = none), features [rows, F], out_features [F, H, W] (forward) sharing
    its slot with dL_dfeaturemap (backward, NULL = zero), dL_dfeatures [rows, F] (backward, NULL = not wanted)."""
    _anonymous_ = ("_map",)
    _fields_ = [("channels", C.c_int32), ("reserved0", C.c_uint32), ("features", C.c_void_p), ("_map", _FeatureMapSlot), ("dL_dfeatures", C.c_void_p)]


class GsrContrib(C.Structure):
    """Per-Gaussian contribution statistics of one view (include/gpsgs.h): weight_sum, weight_max (fp32 [rows]) and pixel_count (int32 [rows]),
    each NULL = not wanted; reserved must be NULL."""
    _fields_ = [("weight_sum", C.c_void_p), ("weight_max", C.c_void_p), ("pixel_count", C.c_void_p), ("reserved", C.c_void_p)]


class GsrAbsGrad(C.Structure):
    """Absolute screen-space gradient of one view (include/gpsgs.h): absgrad fp32 [rows, 2], written by gsr_backward_absgrad (NULL = not wanted);
    reserved must be NULL."""
    _fields_ = [("absgrad", C.c_void_p), ("reserved", C.c_void_p)]


class _DistortSlot(C.Union):
    _fields_ = [("out_distort", C.c_void_p), ("dL_ddistort", C.c_void_p)]


class GsrDistort(C.Structure):
    """Depth-distortion map of one view (include/gpsgs.h): out_distort fp32 [H, W] (forward) sharing its slot with dL_ddistort (backward), NULL = not
    wanted; totals fp32 [2, H, W], written by the forward and read by the backward; reserved must be NULL."""
    _anonymous_ = ("_map",)
    _fields_ = [("_map", _DistortSlot), ("totals", C.c_void_p), ("reserved", C.c_void_p * 2)]


vp, i32, i64, f32, sz, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t, C.c_uint
sp, pp = C.POINTER(GsrStrided), C.POINTER(C.c_void_p)
_WS = [i32, i32, i32, i64]   # P, W, H, instance capacity
_FWD = [i32, i32, i32, vp, vp, vp, vp, vp, f32, f32, f32, vp, vp, vp, vp, vp, vp, sz, i64, u32, vp]
_FWD_NOTIFY = _FWD + [vp, u32]
_FWD_EX = _FWD_NOTIFY + [C.POINTER(GsrViewExt)]
_BWD = [i32, i32, i32, vp, vp, vp, vp, vp, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i64, u32, vp]
_BWD_EX = _BWD + [C.POINTER(GsrViewExt)]
_BWD_CAMERA = _BWD_EX + [vp, vp, vp, vp, sz]

# name -> (restype, argtypes) of every symbol include/gpsgs.h declares, one dict per section of the header, in its order.  lib() sets the prototypes from
# PROTOTYPES, their union, so a symbol cannot be listed without one (ctypes' default `int` conversion would truncate a 64-bit device pointer
# silently); tests/test_capi.py holds the union to the header's declarations and to SECTIONS, and checks that every name has its prototype set.
_GSR = {
    "gpsgs_abi_version": (i32, []),
    "gsr_supported_flags": (i32, []),
    "gpsgs_build_info": (C.c_char_p, []),
    "gpsgs_measure_sclk": (i32, [vp, C.POINTER(C.c_double), vp]),
    "gsr_debug_set_wg_trace": (i32, [vp]),
    "gsr_workspace_bytes": (sz, _WS),
    "gsr_workspace_bytes_forward_only": (sz, _WS),
    "gsr_workspace_bytes_ex": (sz, _WS + [u32, i32]),
    "gsr_workspace_bytes_depth_alpha": (sz, _WS + [u32, i32]),
    "gsr_direct_lists_ok": (i32, [i32, i32, u32]),
    "gsr_forward": (i32, _FWD),
    "gsr_forward_notify": (i32, _FWD_NOTIFY),
    "gsr_forward_ex": (i32, _FWD_EX),
    "gsr_backward": (i32, _BWD),
    "gsr_backward_ex": (i32, _BWD_EX),
    "gsr_camera_grad_scratch_bytes": (sz, [i32]),
    "gsr_backward_camera": (i32, _BWD_CAMERA),
    "gsr_workspace_bytes_features": (sz, _WS + [u32, i32, i32]),
    "gsr_forward_features": (i32, _FWD_EX + [C.POINTER(GsrFeatures)]),
    "gsr_backward_features": (i32, _BWD_CAMERA + [C.POINTER(GsrFeatures)]),
    "gsr_workspace_bytes_contrib": (sz, _WS + [u32, i32]),
    "gsr_forward_contrib": (i32, _FWD_EX + [C.POINTER(GsrContrib)]),
    "gsr_workspace_bytes_absgrad": (sz, _WS + [u32]),
    "gsr_backward_absgrad": (i32, _BWD_CAMERA + [C.POINTER(GsrAbsGrad)]),
    "gsr_forward_distort": (i32, _FWD_EX + [C.POINTER(GsrDistort)]),
    "gsr_backward_distort": (i32, _BWD_CAMERA + [C.POINTER(GsrDistort)]),
    "gsr_copy_header_async": (i32, [vp, vp, vp]),
    "gsr_read_header": (i32, [vp, C.POINTER(GsrHeader), vp]),
    "gsr_export_state": (i32, [vp, i32, i32, i32, i64, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gsr_mark_visible": (i32, [i32, vp, vp, vp, vp, vp]),
    "gsr_selftest": (i32, [vp, vp]),
    "gsr_timing_read": (i32, [C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "gsr_debug_count_records": (i32, [vp, sz, i32, i32, i32, i64, u32, vp, vp]),
    "gsr_pack_scratch_bytes": (sz, [i32, i32, i32]),
    "gsr_pack_views": (i32, [i32, i32, i32, sp, sp, sp, sp, sp, sp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gsr_pack_views_backward": (i32, [i32, i32, i32, vp, vp, vp, vp, vp, vp, pp, pp, pp, pp, pp, vp]),
    "gsr_head_supported": (i32, [i32, i32, i32]),
    "gsr_head_tile": (i32, []),
    "gsr_head_scratch_bytes": (sz, [i32, i32, i32, i32, i32]),
    "gsr_head_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, vp, vp]),
    "gsr_head_backward": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp]),
    "fl_scratch_bytes": (sz, [i32, i32, i32]),
    "fl_l1_ssim_forward": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "fl_l1_ssim_backward": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "up_unproject_forward": (i32, [i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "up_unproject_backward": (i32, [i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp]),
    "up_unproject_forward_dev": (i32, [i32, i32, vp, vp, i64, vp, vp, vp, vp, vp]),
    "up_unproject_backward_dev": (i32, [i32, i32, vp, vp, i64, vp, vp, vp, i64, i64, i64, vp, vp]),
    "up_splat_scratch_bytes": (sz, [i32, i32]),
    "up_zsplat": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
    "up_flow2render_dev": (i32, [i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
    "cs_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cs_backward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cv_build_forward": (i32, [vp, vp, pp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cv_build_backward": (i32, [vp, vp, pp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cs_lookup_forward": (i32, [pp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cs_lookup_backward": (i32, [vp, vp, pp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "cu_upsample_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cu_upsample_backward": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "cu_upsample_scratch_bytes": (sz, [i32, i32, i32, i32]),
}
# GroupNorm (tests/test_capi_groupnorm.py cross-checks these names against the header)
_GN = {
    "gn_chunk_elems": (sz, []),
    "gn_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "gn_forward": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp]),
    "gn_backward": (i32, [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
}
# GroupNorm with the ReLU / residual add + ReLU epilogue fused in (the same section; tests/test_capi_groupnorm_epilogue.py)
_GNE = {
    "gne_forward": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp]),
    "gne_backward": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
}
# Stem convolution (the header's last section; tests/test_capi_stemconv.py)
_SC = {
    "sc_supported": (i32, [i32, i32, i32, i32, i32]),
    "sc_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "sc_scratch_bytes": (sz, [i32, i32, i32, i32, i32, i32, i32, i32]),
    "sc_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp]),
    "sc_backward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
}
# 3x3 convolution on the matrix cores (tests/test_capi_conv3x3.py)
_C3 = {
    "c3_supported": (i32, [i32, i32]),
    "c3_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "c3_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "c3_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "c3_backward": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
}
# 1x1 convolution on the matrix cores (tests/test_capi_conv1x1.py)
_C1 = {
    "c1_supported": (i32, [i32, i32, i32]),
    "c1_tile": (i32, [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "c1_scratch_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
    "c1_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "c1_backward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
}
# Residual-block 3x3 convolution, C_in -> C_out, on the matrix cores (tests/test_capi_resconv.py)
_RC = {
    "rc_supported": (i32, [i32, i32]),
    "rc_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "rc_scratch_bytes": (sz, [i32, i32, i32, i32, i32]),
    "rc_forward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "rc_backward": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
}
# Decoder glue, bilinear 2x upsample + concatenation (the header's last section; tests/test_capi_upcat.py).  skips / skip_channels: host arrays
_UC = {
    "uc_supported": (i32, [i32, C.POINTER(i32)]),
    "uc_tile": (i32, [C.POINTER(i32), C.POINTER(i32)]),
    "uc_forward": (i32, [vp, pp, C.POINTER(i32), i32, i32, i32, i32, i32, vp, vp]),
    "uc_backward": (i32, [vp, C.POINTER(i32), i32, i32, i32, i32, i32, vp, vp]),
}
PROTOTYPES = {**_GSR, **_GN, **_GNE, **_SC, **_C3, **_C1, **_RC, **_UC}
SECTIONS = tuple(tuple(s) for s in (_GSR, _GN, _GNE, _SC, _C3, _C1, _RC, _UC))     # each section's names, in header order
SYMBOLS, GN_SYMBOLS, GNE_SYMBOLS, SC_SYMBOLS, C3_SYMBOLS, C1_SYMBOLS, RC_SYMBOLS, UC_SYMBOLS = SECTIONS

_lib = None


def lib():
    """Load libgpsgs_hip.so once.  Raises ImportError (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "gps_gaussian_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C gps-gaussian_amd/csrc`). There is no CPU fallback for this path." % LIB_PATH)
    l = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    if l.gpsgs_abi_version() != 4:
        raise ImportError("gps_gaussian_amd: ABI version mismatch in %s" % LIB_PATH)
    _lib = l
    return l


def check(rc, what):
    if rc != 0:
        raise RuntimeError("gps_gaussian_amd: %s failed: %s (%d)" % (what, _ERR.get(rc, "unknown"), rc))


def measure_sclk_mhz(device=None):
    """Shader clock (MHz) under a few milliseconds of chip-filling VALU load (gpsgs_measure_sclk); synchronises the current stream."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    scratch = torch.zeros((3,), dtype=torch.int64, device=dev)
    mhz = C.c_double(0.0)
    with torch.cuda.device(dev):
        check(lib().gpsgs_measure_sclk(scratch.data_ptr(), C.byref(mhz), torch.cuda.current_stream(dev).cuda_stream), "gpsgs_measure_sclk")
    return float(mhz.value)


def timing_read():
    """Per-stage {name: (total_ms, launches)} of the calls made with GSR_FLAG_TIMING since the last read."""
    ms = (C.c_float * len(STAGES))()
    n = (C.c_int * len(STAGES))()
    check(lib().gsr_timing_read(ms, n), "gsr_timing_read")
    return {name: (float(ms[i]), int(n[i])) for i, name in enumerate(STAGES)}
