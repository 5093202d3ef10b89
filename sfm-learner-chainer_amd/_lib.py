"""ctypes binding of libsfmwarp.so (include/sfmwarp.h).  No torch types cross this boundary:
every tensor is handed over as a raw device pointer plus explicit sizes.

The library is REQUIRED: there is no CPU or PyTorch fallback.  If it is missing, importing
this module raises, and so does every operator of the package.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch ships its own libamdhip64; libsfmwarp.so must bind to that SAME runtime instance (device
# pointers, streams and events are shared with torch), so torch has to be loaded first.  Loading
# /opt/rocm's copy first and torch's afterwards leaves this library without a visible device.
import torch  # noqa: F401

SFM_MAX_SCALES = 8
SFM_MAX_SRC = 8
SFM_RESIZE_MAX_TERMS = 8
SFM_ABI_VERSION = 6
SFM_LAYOUT_PLANAR, SFM_LAYOUT_HWC = 0, 1
SFM_PROJECTION_FAST, SFM_PROJECTION_REFERENCE_ORDER = 0, 1
PROJECTIONS = {None: SFM_PROJECTION_FAST, "fast": SFM_PROJECTION_FAST, "reference_order": SFM_PROJECTION_REFERENCE_ORDER}

SMOOTH_NONE, SMOOTH_SECOND_ORDER, SMOOTH_EDGE_AWARE = 0, 1, 2
SMOOTH_MODES = {None: SMOOTH_NONE, "none": SMOOTH_NONE, "second_order": SMOOTH_SECOND_ORDER,
                "edge_aware": SMOOTH_EDGE_AWARE}



def _setting(table, what, name):
    if name not in table:
        raise ValueError("%s must be one of %s" % (what, sorted(k for k in table if k)))
    return table[name]


def smooth_mode_id(name):
    """SMOOTH_* of a `smooth_mode` argument; anything outside the table is a ValueError"""
    return _setting(SMOOTH_MODES, "smooth_mode", name)


def projection_id(name):
    """SFM_PROJECTION_* of a `projection` argument; anything outside the table is a ValueError"""
    return _setting(PROJECTIONS, "projection", name)


ERR_NULL, ERR_SHAPE, ERR_CONFIG, ERR_WORKSPACE = -1, -2, -3, -4

_FP = C.c_void_p   # device float*


class SfmLossDesc(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("norm_B", C.c_int32), ("n_src", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32 * SFM_MAX_SCALES), ("W", C.c_int32 * SFM_MAX_SCALES),
        ("smooth_reg", C.c_float), ("exp_reg", C.c_float), ("ssim_rate", C.c_float),
        ("smooth_mode", C.c_int32),
        ("tgt", _FP * SFM_MAX_SCALES), ("src", _FP * SFM_MAX_SCALES), ("disp", _FP * SFM_MAX_SCALES),
        ("mask_logits", _FP * SFM_MAX_SCALES), ("intrinsics", _FP), ("pose", _FP * SFM_MAX_SRC),
        ("d_disp", _FP * SFM_MAX_SCALES), ("d_pose", _FP * SFM_MAX_SRC), ("d_mask", _FP * SFM_MAX_SCALES),
        ("d_src", _FP * SFM_MAX_SCALES),
        ("image_layout", C.c_int32),
        ("warped", _FP * SFM_MAX_SCALES),
        ("projection", C.c_int32),
    ]


class SfmWarpPyramidDesc(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("n_src", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32 * SFM_MAX_SCALES), ("W", C.c_int32 * SFM_MAX_SCALES),
        ("image_layout", C.c_int32),
        ("src", _FP * SFM_MAX_SCALES), ("disp", _FP * SFM_MAX_SCALES), ("intrinsics", _FP), ("pose", _FP * SFM_MAX_SRC),
        ("warped", _FP * SFM_MAX_SCALES), ("valid", _FP * SFM_MAX_SCALES),
        ("g_warped", _FP * SFM_MAX_SCALES), ("d_disp", _FP * SFM_MAX_SCALES), ("d_pose", _FP * SFM_MAX_SRC),
    ]


class SfmPhotoErrorDesc(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("n_img", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32 * SFM_MAX_SCALES), ("W", C.c_int32 * SFM_MAX_SCALES),
        ("ssim_rate", C.c_float),
        ("img", _FP * SFM_MAX_SCALES), ("tgt", _FP * SFM_MAX_SCALES), ("err", _FP * SFM_MAX_SCALES),
        ("g_err", _FP * SFM_MAX_SCALES), ("d_img", _FP * SFM_MAX_SCALES),
    ]


MIN_REPROJ_NORM_KEPT, MIN_REPROJ_NORM_ALL = 0, 1
MIN_REPROJ_NORMS = {"kept": MIN_REPROJ_NORM_KEPT, "all": MIN_REPROJ_NORM_ALL}


def min_reproj_norm_id(name):
    """SFM_MIN_REPROJ_NORM_* of a `norm` argument; anything outside the table is a ValueError"""
    return _setting(MIN_REPROJ_NORMS, "norm", name)


class SfmMinReprojDesc(C.Structure):      # include/sfmwarp_min_reproj.h
    _fields_ = [
        ("B", C.c_int32), ("n_err", C.c_int32), ("n_ident", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32 * SFM_MAX_SCALES), ("W", C.c_int32 * SFM_MAX_SCALES),
        ("norm", C.c_int32), ("weight", C.c_float * SFM_MAX_SCALES),
        ("err", _FP * SFM_MAX_SCALES), ("valid", _FP * SFM_MAX_SCALES), ("ident", _FP * SFM_MAX_SCALES),
        ("winner", C.c_void_p * SFM_MAX_SCALES),      # device int8_t*
        ("loss", _FP), ("count", C.c_void_p), ("g_loss", _FP),      # count: device int32_t*
        ("g_err", _FP * SFM_MAX_SCALES),
    ]


DISP_SMOOTH_EDGE_MEAN_ABS, DISP_SMOOTH_EDGE_ABS_MEAN = 0, 1
DISP_SMOOTH_EDGES = {"mean_abs": DISP_SMOOTH_EDGE_MEAN_ABS, "abs_mean": DISP_SMOOTH_EDGE_ABS_MEAN}


def disp_smooth_edge_id(name):
    """SFM_DISP_SMOOTH_EDGE_* of an `edge` argument; anything outside the table is a ValueError"""
    return _setting(DISP_SMOOTH_EDGES, "edge", name)


class SfmDispSmoothDesc(C.Structure):     # include/sfmwarp_disp_smooth.h
    _fields_ = [
        ("B", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32 * SFM_MAX_SCALES), ("W", C.c_int32 * SFM_MAX_SCALES),
        ("normalize", C.c_int32), ("edge", C.c_int32), ("accumulate", C.c_int32), ("weight", C.c_float * SFM_MAX_SCALES),
        ("disp", _FP * SFM_MAX_SCALES), ("img", _FP * SFM_MAX_SCALES),
        ("loss", _FP), ("stats", C.c_void_p), ("g_loss", _FP),      # stats: device double*
        ("g_disp", _FP * SFM_MAX_SCALES),
    ]


class SfmWarpFullResDesc(C.Structure):    # include/sfmwarp_full_res.h
    _fields_ = [
        ("B", C.c_int32), ("n_src", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32), ("W", C.c_int32),
        ("h", C.c_int32 * SFM_MAX_SCALES), ("w", C.c_int32 * SFM_MAX_SCALES),
        ("image_layout", C.c_int32),
        ("src", _FP), ("disp", _FP * SFM_MAX_SCALES), ("intrinsics", _FP), ("pose", _FP * SFM_MAX_SRC),
        ("warped", _FP * SFM_MAX_SCALES), ("valid", _FP * SFM_MAX_SCALES),
        ("g_warped", _FP * SFM_MAX_SCALES), ("d_disp", _FP * SFM_MAX_SCALES), ("d_pose", _FP * SFM_MAX_SRC),
    ]


# include/sfmwarp_conventions.h: the padding of the SSIM window and the upsampling of the full-resolution warp's disparities
SSIM_PAD_ZERO, SSIM_PAD_REFLECT = 0, 1
SSIM_PADDINGS = {"zero": SSIM_PAD_ZERO, "reflect": SSIM_PAD_REFLECT}
UPSAMPLE_ALIGN_CORNERS, UPSAMPLE_HALF_PIXEL = 0, 1
UPSAMPLES = {"align_corners": UPSAMPLE_ALIGN_CORNERS, "half_pixel": UPSAMPLE_HALF_PIXEL}


def ssim_padding_id(name, what="padding"):
    """SFM_SSIM_PAD_* of a `padding` argument; anything outside the table is a ValueError"""
    return _setting(SSIM_PADDINGS, what, name)


def upsample_id(name):
    """SFM_UPSAMPLE_* of an `upsample` argument; anything outside the table is a ValueError"""
    return _setting(UPSAMPLES, "upsample", name)


# include/sfmwarp_pose.h: what a pose holds, the inverse transform per source, and the affine map in front of depth = 1 / disp
POSE_EULER, POSE_AXIS_ANGLE, POSE_MATRIX = 0, 1, 2
POSE_FORMATS = {"euler": POSE_EULER, "axis_angle": POSE_AXIS_ANGLE, "matrix": POSE_MATRIX}


def pose_format_id(name):
    """SFM_POSE_* of a `pose_format` argument; anything outside the table is a ValueError"""
    return _setting(POSE_FORMATS, "pose_format", name)


class SfmPoseConv(C.Structure):
    _fields_ = [("pose_format", C.c_int32), ("invert", C.c_int32 * SFM_MAX_SRC), ("disp_scale", C.c_float), ("disp_shift", C.c_float)]


# include/sfmwarp_depth_consistency.h: the geometry-consistency term of SC-SfMLearner
class SfmDepthConsDesc(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("n_src", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32 * SFM_MAX_SCALES), ("W", C.c_int32 * SFM_MAX_SCALES),
        ("disp", _FP * SFM_MAX_SCALES), ("src_disp", _FP * SFM_MAX_SCALES), ("intrinsics", _FP), ("pose", _FP * SFM_MAX_SRC),
        ("diff", _FP * SFM_MAX_SCALES), ("valid", _FP * SFM_MAX_SCALES),
        ("computed", _FP * SFM_MAX_SCALES), ("projected", _FP * SFM_MAX_SCALES),
        ("g_diff", _FP * SFM_MAX_SCALES), ("d_disp", _FP * SFM_MAX_SCALES), ("d_src_disp", _FP * SFM_MAX_SCALES),
        ("d_pose", _FP * SFM_MAX_SRC),
    ]


# include/sfmwarp_pairwise.h: the masked means of SC-SfMLearner's compute_pairwise_loss
class SfmPairwiseDesc(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("n_src", C.c_int32), ("n_scales", C.c_int32),
        ("H", C.c_int32 * SFM_MAX_SCALES), ("W", C.c_int32 * SFM_MAX_SCALES),
        ("detach_weight", C.c_int32), ("min_count_photo", C.c_int32), ("min_count_geom", C.c_int32),
        ("weight", C.c_float * SFM_MAX_SCALES),
        ("err", _FP * SFM_MAX_SCALES), ("diff", _FP * SFM_MAX_SCALES), ("valid", _FP * SFM_MAX_SCALES),
        ("ident", _FP * SFM_MAX_SCALES), ("cmp", _FP * SFM_MAX_SCALES),
        ("keep", C.c_void_p * SFM_MAX_SCALES),      # device int8_t*
        ("loss", _FP), ("count", C.c_void_p), ("g_loss", _FP),      # count: device int32_t*
        ("g_err", _FP * SFM_MAX_SCALES), ("g_diff", _FP * SFM_MAX_SCALES),
    ]


# SFMWARP_LIB selects another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("SFMWARP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsfmwarp.so")

# every symbol declared in include/sfmwarp.h: name -> (restype, argtypes)
_I, _V, _Z = C.c_int, C.c_void_p, C.c_size_t
SYMBOLS = {
    "sfm_abi_version": (_I, []),
    "sfm_last_error": (C.c_char_p, []),
    "sfm_pose_proj_fwd": (_I, [_FP, _FP, _FP, _I, _V]),
    "sfm_pose_proj_bwd": (_I, [_FP, _FP, _FP, _FP, _I, _V]),
    "sfm_warp_fwd": (_I, [_FP, _FP, _I, _FP, _FP, _FP, _I, _I, _I, _I, _V]),
    "sfm_warp_bwd_workspace_bytes": (_Z, [_I, _I, _I]),
    "sfm_warp_bwd": (_I, [_FP, _FP, _I, _FP, _FP, _FP, _FP, _FP, _FP, _V, _Z, _I, _I, _I, _I, _V]),
    "sfm_sampler_fwd": (_I, [_FP, _FP, _FP, _I, _I, _I, _I, _I, _I, _V]),
    "sfm_sampler_bwd": (_I, [_FP, _FP, _FP, _FP, _FP, _I, _I, _I, _I, _I, _I, _V]),
    "sfm_sampler_interp_fwd": (_I, [_FP, _FP, _FP, _I, _I, _I, _I, _I, _I, _V]),
    "sfm_sampler_interp_bwd": (_I, [_FP, _FP, _FP, _FP, _FP, _I, _I, _I, _I, _I, _I, _V]),
    "sfm_loss_workspace_bytes": (_Z, [C.POINTER(SfmLossDesc)]),
    "sfm_loss_fwd": (_I, [C.POINTER(SfmLossDesc), _FP, _V, _Z, _V]),
    "sfm_loss_bwd": (_I, [C.POINTER(SfmLossDesc), C.c_float, _V, _Z, _V]),
    "sfm_loss_fwd_bwd": (_I, [C.POINTER(SfmLossDesc), _FP, _V, _Z, _V]),
    "sfm_step_fwd": (_I, [_FP, _FP, C.POINTER(SfmLossDesc), _FP, _V, _Z, _V]),
    "sfm_step_fwd_bwd": (_I, [_FP, _FP, C.POINTER(SfmLossDesc), _FP, _V, _Z, _V]),
    "sfm_loss_plan_info": (_I, [C.POINTER(SfmLossDesc), _I, _I, C.POINTER(C.c_int), _I]),
    "sfm_loss_profile_events": (_I, [_V, _V]),
    "sfm_loss_debug_trace": (_I, [_V]),
    "sfm_loss_variant": (_I, [_I]),
    "sfm_resize_fwd": (_I, [_FP, _FP, _I, _I, _I, _I, _I, _I, _V]),
    "sfm_disp_act_fwd": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), _I, _V]),
    "sfm_disp_act_bwd": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), _I, _V]),
    "sfm_scale_arrays": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), _I, _FP, _V]),
    "sfm_augment_fwd": (_I, [_FP, _FP, _FP, _I, _I, _I, _I, _I, _V]),
    "sfm_pyramid_fwd": (_I, [_FP, C.POINTER(C.c_void_p), _I, _I, _I, _I, _I, _V]),
    "sfm_pyramid_variant": (_I, [_I]),
    "sfm_pyramid_hwc_fwd": (_I, [_FP, C.POINTER(C.c_void_p), _I, _I, _I, _I, _I, _V]),
    "sfm_pyramid_pair_hwc_fwd": (_I, [_FP, _FP, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _I, _I, _I, _I, _I, _V]),
    # the backward of sfm_resize_fwd
    "sfm_resize_bwd": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _FP, _I, _I, _I, _I, _V]),
    # the gradient with respect to the camera intrinsics
    "sfm_loss_proj_bwd": (_I, [C.POINTER(SfmLossDesc), _I, _V, _Z, _FP, _FP, _V]),
    "sfm_warp_intrinsics_bwd_workspace_bytes": (_Z, [_I, _I, _I]),
    "sfm_warp_intrinsics_bwd": (_I, [_FP, _FP, _I, _FP, _FP, _FP, _FP, _V, _Z, _I, _I, _I, _I, _V]),
    "sfm_pose_proj_bwd_k": (_I, [_FP, _FP, _FP, _FP, _I, _V]),
    # the differentiable warp of the whole source pyramid
    "sfm_warp_pyramid_fwd": (_I, [C.POINTER(SfmWarpPyramidDesc), _V]),
    "sfm_warp_pyramid_bwd_workspace_bytes": (_Z, [C.POINTER(SfmWarpPyramidDesc)]),
    "sfm_warp_pyramid_bwd": (_I, [C.POINTER(SfmWarpPyramidDesc), _V, _Z, _V]),
    # the per-pixel L1 + SSIM error maps of a warped pyramid
    "sfm_photo_error_fwd": (_I, [C.POINTER(SfmPhotoErrorDesc), _V]),
    "sfm_photo_error_bwd": (_I, [C.POINTER(SfmPhotoErrorDesc), _V]),
}

# every symbol declared in the side header include/sfmwarp_min_reproj.h (to be folded into SYMBOLS together with that header)
EXT_SYMBOLS = {
    "sfm_min_reproj_workspace_bytes": (_Z, [C.POINTER(SfmMinReprojDesc)]),
    "sfm_min_reproj_fwd": (_I, [C.POINTER(SfmMinReprojDesc), _V, _Z, _V]),
    "sfm_min_reproj_bwd": (_I, [C.POINTER(SfmMinReprojDesc), _V]),
}


# every symbol declared in the side header include/sfmwarp_disp_smooth.h (to be folded into SYMBOLS together with that header)
SMOOTH_SYMBOLS = {
    "sfm_disp_smooth_workspace_bytes": (_Z, [C.POINTER(SfmDispSmoothDesc)]),
    "sfm_disp_smooth_fwd": (_I, [C.POINTER(SfmDispSmoothDesc), _V, _Z, _V]),
    "sfm_disp_smooth_bwd": (_I, [C.POINTER(SfmDispSmoothDesc), _V]),
}


# every symbol declared in the side header include/sfmwarp_full_res.h (to be folded into SYMBOLS together with that header)
FULL_RES_SYMBOLS = {
    "sfm_warp_full_res_fwd": (_I, [C.POINTER(SfmWarpFullResDesc), _V]),
    "sfm_warp_full_res_bwd_workspace_bytes": (_Z, [C.POINTER(SfmWarpFullResDesc)]),
    "sfm_warp_full_res_bwd": (_I, [C.POINTER(SfmWarpFullResDesc), _V, _Z, _V]),
}


# every symbol declared in the side header include/sfmwarp_conventions.h (to be folded into SYMBOLS together with that header)
CONV_SYMBOLS = {
    "sfm_photo_error_pad_fwd": (_I, [C.POINTER(SfmPhotoErrorDesc), C.c_int32, _V]),
    "sfm_photo_error_pad_bwd": (_I, [C.POINTER(SfmPhotoErrorDesc), C.c_int32, _V]),
    "sfm_warp_full_res_up_fwd": (_I, [C.POINTER(SfmWarpFullResDesc), C.c_int32, _V]),
    "sfm_warp_full_res_up_bwd_workspace_bytes": (_Z, [C.POINTER(SfmWarpFullResDesc), C.c_int32]),
    "sfm_warp_full_res_up_bwd": (_I, [C.POINTER(SfmWarpFullResDesc), C.c_int32, _V, _Z, _V]),
}


# every symbol declared in the side header include/sfmwarp_pose.h (to be folded into SYMBOLS together with that header)
POSE_SYMBOLS = {
    "sfm_pose_mat_fwd": (_I, [_FP, C.c_int32, C.c_int32, _FP, _I, _V]),
    "sfm_pose_mat_bwd": (_I, [_FP, C.c_int32, C.c_int32, _FP, _FP, _I, _V]),
    "sfm_warp_pyramid_conv_fwd": (_I, [C.POINTER(SfmWarpPyramidDesc), C.POINTER(SfmPoseConv), _V]),
    "sfm_warp_pyramid_conv_bwd_workspace_bytes": (_Z, [C.POINTER(SfmWarpPyramidDesc), C.POINTER(SfmPoseConv)]),
    "sfm_warp_pyramid_conv_bwd": (_I, [C.POINTER(SfmWarpPyramidDesc), C.POINTER(SfmPoseConv), _V, _Z, _V]),
    "sfm_warp_full_res_conv_fwd": (_I, [C.POINTER(SfmWarpFullResDesc), C.c_int32, C.POINTER(SfmPoseConv), _V]),
    "sfm_warp_full_res_conv_bwd_workspace_bytes": (_Z, [C.POINTER(SfmWarpFullResDesc), C.c_int32, C.POINTER(SfmPoseConv)]),
    "sfm_warp_full_res_conv_bwd": (_I, [C.POINTER(SfmWarpFullResDesc), C.c_int32, C.POINTER(SfmPoseConv), _V, _Z, _V]),
}


# every symbol declared in the side header include/sfmwarp_depth_consistency.h (to be folded into SYMBOLS together with that header)
DEPTH_CONS_SYMBOLS = {
    "sfm_depth_consistency_fwd": (_I, [C.POINTER(SfmDepthConsDesc), C.POINTER(SfmPoseConv), _V]),
    "sfm_depth_consistency_bwd_workspace_bytes": (_Z, [C.POINTER(SfmDepthConsDesc), C.POINTER(SfmPoseConv)]),
    "sfm_depth_consistency_bwd": (_I, [C.POINTER(SfmDepthConsDesc), C.POINTER(SfmPoseConv), _V, _Z, _V]),
}


# every symbol declared in the side header include/sfmwarp_pairwise.h (to be folded into SYMBOLS together with that header)
PAIRWISE_SYMBOLS = {
    "sfm_pairwise_workspace_bytes": (_Z, [C.POINTER(SfmPairwiseDesc)]),
    "sfm_pairwise_fwd": (_I, [C.POINTER(SfmPairwiseDesc), _V, _Z, _V]),
    "sfm_pairwise_bwd": (_I, [C.POINTER(SfmPairwiseDesc), _V]),
}


class SfmWarpError(RuntimeError):
    """A launch failed inside libsfmwarp (positive return code = hipError_t)."""


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libsfmwarp.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C sfm-learner-chainer_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SYMBOLS.items()) + list(EXT_SYMBOLS.items()) + list(SMOOTH_SYMBOLS.items()) \
            + list(FULL_RES_SYMBOLS.items()) + list(CONV_SYMBOLS.items()) + list(POSE_SYMBOLS.items()) + list(DEPTH_CONS_SYMBOLS.items()) \
            + list(PAIRWISE_SYMBOLS.items()):
        fn = getattr(lib, name)     # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    got = lib.sfm_abi_version()
    if got != SFM_ABI_VERSION:
        raise ImportError("libsfmwarp.so has ABI version %d, this package expects %d" % (got, SFM_ABI_VERSION))
    return lib


lib = _load()


def last_error() -> str:
    msg = lib.sfm_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(code: int) -> None:
    """Maps the C return convention onto the reference's classes of failure: bad shapes /
    dtypes are TypeError (Chainer's type_check.InvalidType is a TypeError-like check failure),
    inconsistent configuration is ValueError, launch failures are RuntimeError."""
    if code == 0:
        return
    msg = last_error()
    if code in (ERR_NULL, ERR_SHAPE):
        raise TypeError(msg)
    if code in (ERR_CONFIG, ERR_WORKSPACE):
        raise ValueError(msg)
    raise SfmWarpError("%s (code %d)" % (msg, code))
