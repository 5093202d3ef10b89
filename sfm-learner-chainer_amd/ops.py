"""Thin array-level wrappers over the C ABI.  torch.Tensor on a ROCm device is used purely as
the device-array container (allocation, stream, lifetime); all arithmetic happens in
libsfmwarp.so.  Arrays are float32, C-contiguous, NCHW -- the reference's layout.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import SfmDepthConsDesc, SfmDispSmoothDesc, SfmLossDesc, SfmMinReprojDesc, SfmPairwiseDesc, SfmPhotoErrorDesc, SfmWarpFullResDesc, SfmWarpPyramidDesc, check, lib

__all__ = ["pose_proj_fwd", "pose_proj_bwd", "pose_proj_bwd_intrinsics", "warp_fwd", "warp_bwd", "warp_bwd_intrinsics", "sampler_fwd", "sampler_bwd",
           "interp_fwd", "interp_bwd", "resize", "resize_bwd", "pyramid", "disp_act_fwd", "disp_act_bwd", "FusedLoss", "warp_pyramid_fwd",
           "warp_pyramid_bwd", "photo_error_fwd", "photo_error_bwd", "min_reproj_fwd", "min_reproj_bwd",
           "disp_smooth_fwd", "disp_smooth_bwd", "warp_full_res_fwd", "warp_full_res_bwd", "pose_mat_fwd", "pose_mat_bwd",
           "depth_consistency_fwd", "depth_consistency_bwd", "pairwise_fwd", "pairwise_bwd"]

FLOAT32 = (torch.float32,)
FLOATS = (torch.float32, torch.bfloat16, torch.float16)      # what a network puts out, autocast included (torch_api casts them)
_DTYPE_NAMES = {FLOAT32: "float32 (dtype.char == 'f')", FLOATS: "float32, bfloat16 or float16"}


def _dev(t, name, ndim=None, dtypes=FLOAT32):
    """A CUDA(ROCm) tensor of one of `dtypes`, made contiguous; anything else is a type error, as in the
    reference's check_type_forward (spational_transformer_sampler_interp.py:11-24)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor on a ROCm device, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise TypeError("%s: CPU arrays are not supported by this build (GPU-only, no CPU fallback)" % name)
    if t.dtype not in dtypes:
        raise TypeError("%s: expected dtype %s, got %s" % (name, _DTYPE_NAMES[dtypes], t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise TypeError("%s: expected ndim == %d, got %d" % (name, ndim, t.dim()))
    return t.contiguous()


def _devs(ts, name, ndim=None):
    return [_dev(t, "%s[%d]" % (name, k), ndim) for k, t in enumerate(ts)]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _numel_array(ts):
    return (C.c_longlong * len(ts))(*[t.numel() for t in ts])


def _empty(shapes, device):
    return [torch.empty(shape, dtype=torch.float32, device=device) for shape in shapes]


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(index=None):
    """The HIP stream torch currently issues work on for that device, as a raw handle.  (The private accessor
    skips the construction of a torch.cuda.Stream object: it is what torch's own launchers use per call.)"""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device() if index is None else index))
    return C.c_void_p(torch.cuda.current_stream(index).cuda_stream)


def _launch(device, fn, *args):
    """THE call through the C ABI: fn(*args, stream) on the stream torch currently issues work on for `device`, return code
    checked.  The device guard is entered only when `device` is not the current one (a fused step is 15-70 us of GPU time and
    its host side about 7 us: the guard alone, let alone a generator-based context manager, would show)."""
    idx = device.index
    if torch.cuda.current_device() == idx:
        check(fn(*args, _stream(idx)))
    else:
        with torch.cuda.device(idx):
            check(fn(*args, _stream(idx)))


def pose_proj_fwd(pose6, K):
    pose6, K = _dev(pose6, "pose6", 2), _dev(K, "K", 3)
    N = pose6.shape[0]
    if pose6.shape[1] != 6 or tuple(K.shape) != (N, 3, 3):
        raise TypeError("pose6 must be (N,6) and K (N,3,3)")
    out = torch.empty((N, 4, 4), dtype=torch.float32, device=pose6.device)
    _launch(pose6.device, lib.sfm_pose_proj_fwd, _p(pose6), _p(K), _p(out), N)
    return out


def pose_proj_bwd(pose6, K, g_proj):
    pose6, K, g_proj = _dev(pose6, "pose6", 2), _dev(K, "K", 3), _dev(g_proj, "g_proj", 3)
    N = pose6.shape[0]
    out = torch.empty((N, 6), dtype=torch.float32, device=pose6.device)
    _launch(pose6.device, lib.sfm_pose_proj_bwd, _p(pose6), _p(K), _p(g_proj), _p(out), N)
    return out


def _pose_mat_setting(fmt, invert):
    fmt = _lib.pose_format_id(fmt)
    if fmt == _lib.POSE_MATRIX:
        raise ValueError("pose_format must be 'euler' or 'axis_angle' here: a matrix is what this operator returns")
    return fmt, int(bool(invert))


def pose_mat_fwd(pose6, fmt, invert):
    """pose6 (N,6) in the convention `fmt` ("euler": the reference's euler2mat / pose_vec2mat; "axis_angle": Monodepth2's
    rot_from_axisangle and translation) -> T (N,3,4) = [R|t], or [R^T | -R^T t] with `invert` (sfm_pose_mat_fwd)."""
    fmt, invert = _pose_mat_setting(fmt, invert)
    pose6 = _dev(pose6, "pose6", 2)
    N = pose6.shape[0]
    if pose6.shape[1] != 6:
        raise TypeError("pose6 must be (N,6)")
    out = torch.empty((N, 3, 4), dtype=torch.float32, device=pose6.device)
    _launch(pose6.device, lib.sfm_pose_mat_fwd, _p(pose6), fmt, invert, _p(out), N)
    return out


def pose_mat_bwd(pose6, fmt, invert, g_T):
    """The backward of `pose_mat_fwd` for g_T (N,3,4) -> d_pose6 (N,6) (sfm_pose_mat_bwd)."""
    fmt, invert = _pose_mat_setting(fmt, invert)
    pose6, g_T = _dev(pose6, "pose6", 2), _dev(g_T, "g_T", 3)
    N = pose6.shape[0]
    if pose6.shape[1] != 6 or tuple(g_T.shape) != (N, 3, 4) or g_T.device != pose6.device:
        raise TypeError("pose6 must be (N,6) and g_T (N,3,4) on the same device")
    out = torch.empty((N, 6), dtype=torch.float32, device=pose6.device)
    _launch(pose6.device, lib.sfm_pose_mat_bwd, _p(pose6), fmt, invert, _p(g_T), _p(out), N)
    return out


def pose_conv(pose_format="euler", invert=None, depth_affine=None, n_src=None):
    """The SfmPoseConv of three keyword arguments (include/sfmwarp_pose.h), or None where all three are the defaults -- the caller
    then uses the existing symbols.  invert: None or one flag per source; depth_affine: None or (disp_scale, disp_shift).  Anything
    else is a ValueError, raised before a tensor is looked at."""
    if pose_format == "euler" and invert is None and depth_affine is None:
        return None
    fmt = _lib.pose_format_id(pose_format)
    flags = [] if invert is None else [bool(v) for v in invert]
    if n_src is not None and invert is not None and len(flags) != n_src:
        raise ValueError("invert needs one flag per source (%d), got %d" % (n_src, len(flags)))
    if len(flags) > _lib.SFM_MAX_SRC:
        raise ValueError("invert: at most %d sources" % _lib.SFM_MAX_SRC)
    if fmt == _lib.POSE_MATRIX and any(flags):
        raise ValueError("invert with pose_format='matrix': a general 3x4 has no R^T inverse, invert it before the call")
    scale, shift = (1.0, 0.0) if depth_affine is None else (float(depth_affine[0]), float(depth_affine[1]))
    if not (scale - scale == 0.0 and shift - shift == 0.0):
        raise ValueError("depth_affine must be two finite numbers, got %r" % (depth_affine,))
    if fmt == _lib.POSE_EULER and not any(flags) and (scale, shift) == (1.0, 0.0):
        return None
    c = _lib.SfmPoseConv()
    c.pose_format, c.disp_scale, c.disp_shift = fmt, scale, shift
    for i, v in enumerate(flags):
        c.invert[i] = int(v)
    return c


def _pose_shape(conv):
    """the shape of one sample's pose under the conventions `conv`"""
    return (3, 4) if conv is not None and conv.pose_format == _lib.POSE_MATRIX else (6,)


def pose_proj_bwd_intrinsics(pose6, K, g_proj):
    """The K half of `pose_proj_bwd` (sfm_pose_proj_bwd_k): g_proj (N,4,4) -> d_K (N,3,3) = g_proj[:, :3, :] . [R|t]^T."""
    pose6, K, g_proj = _dev(pose6, "pose6", 2), _dev(K, "K", 3), _dev(g_proj, "g_proj", 3)
    N = pose6.shape[0]
    if pose6.shape[1] != 6 or tuple(K.shape) != (N, 3, 3) or tuple(g_proj.shape) != (N, 4, 4):
        raise TypeError("pose6 must be (N,6), K (N,3,3) and g_proj (N,4,4)")
    out = torch.empty((N, 3, 3), dtype=torch.float32, device=pose6.device)
    _launch(pose6.device, lib.sfm_pose_proj_bwd_k, _p(pose6), _p(K), _p(g_proj), _p(out), N)
    return out


def _warp_args(imgs, depth, pose6, K):
    imgs = _dev(imgs, "imgs", 4)
    N, Cc, H, W = imgs.shape
    depth = _dev(depth, "depth")
    if depth.numel() == N * H * W:
        drows = 1
    elif depth.numel() == 3 * N * H * W:
        drows = 3
    else:
        raise TypeError("depthes must be (N,3,H*W) or (N,H*W), got shape %s" % (tuple(depth.shape),))
    pose6, K = _dev(pose6, "poses", 2), _dev(K, "K", 3)
    if tuple(pose6.shape) != (N, 6) or tuple(K.shape) != (N, 3, 3):
        raise TypeError("poses must be (N,6) and K (N,3,3) with N=%d" % N)
    return imgs, depth, drows, pose6, K, N, Cc, H, W


def warp_fwd(imgs, depth, pose6, K):
    """projective_inverse_warp forward.  depth: (N,3,H*W) as in the reference, or (N,H*W) = one
    row of its broadcast (models/base_model.py:82-84)."""
    imgs, depth, drows, pose6, K, N, Cc, H, W = _warp_args(imgs, depth, pose6, K)
    out = torch.empty_like(imgs)
    _launch(imgs.device, lib.sfm_warp_fwd, _p(imgs), _p(depth), drows, _p(pose6), _p(K), _p(out), N, Cc, H, W)
    return out


def warp_bwd(imgs, depth, pose6, K, g_warped, want_d_src=False):
    imgs, depth, drows, pose6, K, N, Cc, H, W = _warp_args(imgs, depth, pose6, K)
    g_warped = _dev(g_warped, "g_warped", 4)
    if g_warped.shape != imgs.shape:
        raise TypeError("g_warped must have the shape of imgs")
    d_depth = torch.empty((N, 3, H * W) if drows == 3 else (N, H * W), dtype=torch.float32, device=imgs.device)
    d_pose = torch.empty((N, 6), dtype=torch.float32, device=imgs.device)
    d_src = torch.zeros_like(imgs) if want_d_src else None
    nbytes = lib.sfm_warp_bwd_workspace_bytes(N, H, W)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=imgs.device)
    _launch(imgs.device, lib.sfm_warp_bwd, _p(imgs), _p(depth), drows, _p(pose6), _p(K), _p(g_warped), _p(d_depth), _p(d_pose),
            _p(d_src), _p(ws), nbytes, N, Cc, H, W)
    return d_depth, d_pose, d_src


def warp_bwd_intrinsics(imgs, depth, pose6, K, g_warped):
    """The output `warp_bwd` does not have (sfm_warp_intrinsics_bwd): d_K (N,3,3), the gradient of projective_inverse_warp with
    respect to K for the upstream gradient g_warped.  No atomics: the same bits on every call."""
    imgs, depth, drows, pose6, K, N, Cc, H, W = _warp_args(imgs, depth, pose6, K)
    g_warped = _dev(g_warped, "g_warped", 4)
    if g_warped.shape != imgs.shape:
        raise TypeError("g_warped must have the shape of imgs")
    d_K = torch.empty((N, 3, 3), dtype=torch.float32, device=imgs.device)
    nbytes = lib.sfm_warp_intrinsics_bwd_workspace_bytes(N, H, W)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=imgs.device)
    _launch(imgs.device, lib.sfm_warp_intrinsics_bwd, _p(imgs), _p(depth), drows, _p(pose6), _p(K), _p(g_warped), _p(d_K), _p(ws),
            nbytes, N, Cc, H, W)
    return d_K


def _sampler_args(x, grid):
    x, grid = _dev(x, "x", 4), _dev(grid, "grid", 4)
    if grid.shape[1] != 2:
        raise TypeError("grid.shape[1] must be 2, got %d" % grid.shape[1])
    if x.shape[0] != grid.shape[0]:
        raise TypeError("x.shape[0] != grid.shape[0] (%d vs %d)" % (x.shape[0], grid.shape[0]))
    N, Cc, H, W = x.shape
    return x, grid, N, Cc, H, W, grid.shape[2], grid.shape[3]


def _sampler(fwd, x, grid):
    x, grid, N, Cc, H, W, oH, oW = _sampler_args(x, grid)
    y = torch.empty((N, Cc, oH, oW), dtype=torch.float32, device=x.device)
    _launch(x.device, fwd, _p(x), _p(grid), _p(y), N, Cc, H, W, oH, oW)
    return y


def _sampler_b(bwd, x, grid, gy, want_gx):
    x, grid, N, Cc, H, W, oH, oW = _sampler_args(x, grid)
    gy = _dev(gy, "gy", 4)
    if tuple(gy.shape) != (N, Cc, oH, oW):
        raise TypeError("gy must be (N,C,oH,oW)")
    ggrid = torch.empty_like(grid)
    gx = torch.zeros_like(x) if want_gx else None
    _launch(x.device, bwd, _p(x), _p(grid), _p(gy), _p(ggrid), _p(gx), N, Cc, H, W, oH, oW)
    return gx, ggrid


def sampler_fwd(x, grid):
    return _sampler(lib.sfm_sampler_fwd, x, grid)


def sampler_bwd(x, grid, gy, want_gx=True):
    return _sampler_b(lib.sfm_sampler_bwd, x, grid, gy, want_gx)


def interp_fwd(x, grid):
    return _sampler(lib.sfm_sampler_interp_fwd, x, grid)


def interp_bwd(x, grid, gy, want_gx=True):
    return _sampler_b(lib.sfm_sampler_interp_bwd, x, grid, gy, want_gx)


def resize(x, out_hw):
    x = _dev(x, "x", 4)
    N, Cc, H, W = x.shape
    oH, oW = int(out_hw[0]), int(out_hw[1])
    y = torch.empty((N, Cc, oH, oW), dtype=torch.float32, device=x.device)
    _launch(x.device, lib.sfm_resize_fwd, _p(x), _p(y), N, Cc, H, W, oH, oW)
    return y


def resize_bwd(gys, in_hw):
    """Backward of `resize` (sfm_resize_bwd): gys, one array (N,C,oh,ow) or a list of 1..8 of them with the same N, C and device,
    each the gradient of a resize of ONE input (N,C,*in_hw) to its own size -> gx (N,C,*in_hw), the sum of their adjoints in one
    launch.  [d_src[s] for s in scales] of a fused loss -> the gradient of the full-resolution frames.  A gather: no atomics, the
    same bits on every call."""
    gys = [gys] if isinstance(gys, torch.Tensor) else list(gys)
    if not 1 <= len(gys) <= _lib.SFM_RESIZE_MAX_TERMS:
        raise TypeError("resize_bwd: 1..%d gradient arrays, got %d" % (_lib.SFM_RESIZE_MAX_TERMS, len(gys)))
    gys = _devs(gys, "gys", 4)
    N, Cc = gys[0].shape[:2]
    for k, g in enumerate(gys):
        if tuple(g.shape[:2]) != (N, Cc) or g.device != gys[0].device:
            raise TypeError("resize_bwd: gys[%d] is %s on %s, gys[0] %s on %s: N, C and the device must agree"
                            % (k, tuple(g.shape), g.device, tuple(gys[0].shape), gys[0].device))
    H, W = int(in_hw[0]), int(in_hw[1])
    gx = torch.empty((N, Cc, H, W), dtype=torch.float32, device=gys[0].device)
    sizes = C.c_int * len(gys)
    _launch(gx.device, lib.sfm_resize_bwd, _ptr_array(gys), sizes(*[g.shape[2] for g in gys]), sizes(*[g.shape[3] for g in gys]),
            len(gys), _p(gx), N, Cc, H, W)
    return gx


def _pyramid_shapes(n_scales, N, G, H, W, tail=()):
    """The shape of every level of a pyramid of `n_scales` scales; a scale count the library does not take is a type error."""
    if not 1 <= n_scales <= _lib.SFM_MAX_SCALES:
        raise TypeError("n_scales must be in [1, %d]" % _lib.SFM_MAX_SCALES)
    return [(N, G, H >> s, W >> s) + tail for s in range(n_scales)]


def pyramid(x, n_scales, out=None):
    """[x, resize(x, (H>>1, W>>1)), ...]: all scales of models/base_model.py:69-72 in one launch.
    `out`: the list an earlier call with the same shapes returned -- scales 1.. are written in place and scale 0 becomes `x`
    (a caller that needs scale 0 at a fixed address copies it)."""
    x = _dev(x, "x", 4)
    N, Cc, H, W = x.shape
    shapes = _pyramid_shapes(n_scales, N, Cc, H, W)
    if out is None:
        outs = [x] + _empty(shapes[1:], x.device)
    elif [tuple(t.shape) for t in out] != shapes:
        raise TypeError("pyramid: `out` does not match the input")
    else:
        outs = [x] + list(out[1:])
    _launch(x.device, lib.sfm_pyramid_fwd, _p(x), _ptr_array(outs), N, Cc, H, W, n_scales)
    return outs


def pyramid_hwc(x, n_scales):
    """The pyramid of `pyramid`, pixel-interleaved for the fused loss (SFM_LAYOUT_HWC): x (N,3G,H,W) planar, G images
    per sample -> [y_s (N,G,H>>s,W>>s,3) for s in 0..n_scales-1], one launch.  Same values as `pyramid`."""
    x = _dev(x, "x", 4)
    N, Cc, H, W = x.shape
    if Cc % 3 != 0:
        raise TypeError("pyramid_hwc: the channel count must be a multiple of 3 (RGB images), got %d" % Cc)
    outs = _empty(_pyramid_shapes(n_scales, N, Cc // 3, H, W, (3,)), x.device)
    _launch(x.device, lib.sfm_pyramid_hwc_fwd, _p(x), _ptr_array(outs), N, Cc // 3, H, W, n_scales)
    return outs


def pyramid_pair_hwc(tgt, src, n_scales, out=None, per_pixel=False):
    """Both pixel-interleaved pyramids of a step in one launch: tgt (N,3,H,W), src (N,3*n_src,H,W) ->
    ([tgt_s (N,1,h,w,3)], [src_s (N,n_src,h,w,3)]) -- the loop head models/base_model.py:69-72.
    `out` = (yt, ys) of an earlier call with the same shapes: written in place instead of allocating.
    `per_pixel`: run the one-thread-per-output-pixel kernel instead of the band kernel (same values bit for bit; A/B tests)."""
    tgt, src = _dev(tgt, "tgt", 4), _dev(src, "src", 4)
    N, Ct, H, W = tgt.shape
    if Ct != 3 or src.shape[0] != N or tuple(src.shape[2:]) != (H, W) or src.shape[1] % 3 != 0 or src.shape[1] == 0:
        raise TypeError("pyramid_pair_hwc: expected tgt (N,3,H,W) and src (N,3*n_src,H,W), got %s and %s" % (tuple(tgt.shape), tuple(src.shape)))
    n_src = src.shape[1] // 3
    t_shapes, s_shapes = _pyramid_shapes(n_scales, N, 1, H, W, (3,)), _pyramid_shapes(n_scales, N, n_src, H, W, (3,))
    given = out is not None
    if given:
        yt, ys = out
        if len(yt) != n_scales or len(ys) != n_scales or tuple(yt[0].shape) != t_shapes[0] or tuple(ys[0].shape) != s_shapes[0]:
            raise TypeError("pyramid_pair_hwc: `out` does not match the inputs")
        if yt[0].device != tgt.device or ys[0].device != tgt.device:
            raise TypeError("pyramid_pair_hwc: `out` lives on %s, the inputs on %s" % (yt[0].device, tgt.device))
    else:
        yt, ys = tuple(_empty(t_shapes, tgt.device)), tuple(_empty(s_shapes, tgt.device))
        out = _PyramidPair((yt, ys))
    # (the pointer arrays of the buffers are built once -- a step is 15-60 us -- and are only reused while `out` still holds the
    #  very arrays they were built from: round-5 advisor finding, a caller that swapped an element used to be written through a
    #  stale pointer)
    key = tuple(t.data_ptr() for t in yt) + tuple(t.data_ptr() for t in ys)
    cached = getattr(out, "_ptrs", None)
    if cached is None or cached[0] != key:
        if given:
            for s in range(n_scales):
                for t, shape in ((yt[s], t_shapes[s]), (ys[s], s_shapes[s])):
                    if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32 or t.device != tgt.device:
                        raise TypeError("pyramid_pair_hwc: `out` scale %d does not match the inputs" % s)
        cached = (key, (_ptr_array(yt), _ptr_array(ys)))
        if isinstance(out, _PyramidPair):
            out._ptrs = cached
    if per_pixel:
        check(lib.sfm_pyramid_variant(1))
    _launch(tgt.device, lib.sfm_pyramid_pair_hwc_fwd, _p(tgt), _p(src), *cached[1], N, n_src, H, W, n_scales)
    return out


class _PyramidPair(tuple):
    """(tgt pyramid, src pyramid) as `pyramid_pair_hwc` returns it -- two TUPLES of arrays; carries the ctypes pointer arrays of its
    buffers, keyed on their addresses, so that a caller that hands it back as `out` does not pay for rebuilding them every step."""


def to_hwc(x):
    """(N,3G,h,w) planar -> (N,G,h,w,3) pixel-interleaved copy (a torch permute; for callers that hold planar pyramids)."""
    N, Cc, h, w = x.shape
    return x.reshape(N, Cc // 3, 3, h, w).permute(0, 1, 3, 4, 2).contiguous()


def disp_act_fwd(xs):
    """[10 * sigmoid(x) + 0.01 for x in xs] in one launch (models/disp_net.py:104-122)."""
    xs = _devs(xs, "xs")
    outs = [torch.empty_like(x) for x in xs]
    _launch(xs[0].device, lib.sfm_disp_act_fwd, _ptr_array(xs), _ptr_array(outs), _numel_array(xs), len(xs))
    return outs


def disp_act_bwd(disps, g_disps):
    disps, g_disps = _devs(disps, "disps"), _devs(g_disps, "g_disps")
    if any(a.shape != b.shape for a, b in zip(disps, g_disps)):
        raise TypeError("g_disps must match disps")
    outs = [torch.empty_like(x) for x in disps]
    _launch(disps[0].device, lib.sfm_disp_act_bwd, _ptr_array(disps), _ptr_array(g_disps), _ptr_array(outs), _numel_array(disps),
            len(disps))
    return outs


# ---------------------------------------------------------------------------------------------------------------------------
# the fused loss: descriptor, workspace, layout -- shared by FusedLoss.bind, torch_api._plan and links.SFMLearnerLoss
# ---------------------------------------------------------------------------------------------------------------------------
# SFM_LAYOUT_HWC forms the byte offset of a gather inside one image exactly in fp32 (include/sfmwarp.h): an image of a scale
# must have fewer than 2^24 / 12 pixels there.  Larger frames take the reference's planar layout (same results).
HWC_MAX_PIXELS = (1 << 24) // 12
_LAYOUTS = {"planar": _lib.SFM_LAYOUT_PLANAR, "hwc": _lib.SFM_LAYOUT_HWC}


def layout_for(H, W):
    """The image layout ("hwc" or "planar") the link and the torch route pick for full-resolution frames of H x W."""
    return "hwc" if H * W < HWC_MAX_PIXELS else "planar"


def _set_scales(d, hw):
    """n_scales, H[] and W[] of any of the four descriptors from hw = [(h, w) of each scale]"""
    d.n_scales = len(hw)
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w


def _one_device(dev, arrays):
    for t in arrays:
        if t.device != dev:
            raise TypeError("every array must live on %s, one is on %s" % (dev, t.device))


def loss_desc(B, norm_B, n_src, hw, settings, layout):
    """An SfmLossDesc with every non-pointer field set.  hw: (h, w) of each scale; settings: (smooth_reg, exp_reg, ssim_rate,
    smooth_mode, projection), the last two as _lib.SMOOTH_* / _lib.SFM_PROJECTION_*; layout: "planar" or "hwc".  (Whether
    there are explainability masks shows in the pointers alone.)"""
    d = SfmLossDesc()
    d.B, d.norm_B, d.n_src = B, norm_B, n_src
    d.smooth_reg, d.exp_reg, d.ssim_rate, d.smooth_mode, d.projection = settings
    d.image_layout = _LAYOUTS[layout]
    _set_scales(d, hw)
    return d


def workspace_bytes(d):
    """sfm_loss_workspace_bytes of a descriptor whose pointers are bound (any non-NULL value); 0 bytes means the library
    refuses the descriptor: a ValueError with its message."""
    nbytes = lib.sfm_loss_workspace_bytes(C.byref(d)) if d.B > 0 else 256
    if nbytes == 0:
        check(lib.sfm_loss_fwd(C.byref(d), None, None, 0, None))   # re-run the validation for its message
        raise ValueError(_lib.last_error() or "invalid loss descriptor")
    return nbytes


def _point(field, arrays):
    """field[k] = the address of arrays[k] (a pointer array of the descriptor); None leaves the entry as it is"""
    for k, t in enumerate(arrays):
        if t is not None:
            field[k] = t.data_ptr()


def _own(buffers, key, k, shape, device):
    """The caller's array `buffers[key][k]` if it gave one, else a fresh one"""
    if buffers.get(key) is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    t = buffers[key] if key == "loss5" else buffers[key][k]
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous() \
            or tuple(t.shape) != tuple(shape):
        raise TypeError("buffers[%r][%d]: expected a contiguous float32 array of shape %s on %s" % (key, k, tuple(shape), device))
    return t


def _owns(buffers, key, shapes, device):
    return [_own(buffers, key, k, shape, device) for k, shape in enumerate(shapes)]


def _d_src_arrays(buffers, want_d_src, shapes, device):
    """(the one allocation behind them or None, [a d_src array or None per scale]).  want_d_src: True, or one flag per scale --
    SfmLossDesc.d_src[s] may be NULL for any scale; buffers["d_srcs"], the caller's arrays, replaces it.  Always planar."""
    given = buffers.get("d_srcs")
    if given is not None:
        return None, [_own(buffers, "d_srcs", s, shape, device) if given[s] is not None else None for s, shape in enumerate(shapes)]
    want = [bool(want_d_src[s] if isinstance(want_d_src, (list, tuple)) else want_d_src) for s in range(len(shapes))]
    if not any(want):
        return None, [None] * len(shapes)
    # the d_src arrays of all bound scales are views of ONE allocation: the library accumulates into them (float atomics), so every
    # backward starts by clearing them -- one fill kernel instead of one per scale
    numel = [shape[0] * shape[1] * shape[2] * shape[3] if on else 0 for shape, on in zip(shapes, want)]
    whole = torch.zeros((sum(numel),), dtype=torch.float32, device=device)
    return whole, [part.view(shape) if on else None for part, shape, on in zip(whole.split(numel), shapes, want)]


def _place_workspace(ws, nbytes, device):
    """(tensor, address, bytes) of the workspace as include/sfmwarp.h states it: sfm_loss_workspace_bytes bytes on a 256-byte
    boundary, content undefined -- the caller's `ws`, all of it, or a fresh allocation (which starts on a 512-byte boundary;
    should an allocator ever hand out less, 256 spare bytes absorb it)"""
    if ws is not None:
        if not isinstance(ws, torch.Tensor) or ws.device != device or not ws.is_contiguous():
            raise TypeError("buffers['ws']: expected a contiguous tensor on %s" % (device,))
        ptr, have = ws.data_ptr(), ws.numel() * ws.element_size()
        if ptr % 256 or have < nbytes:
            raise ValueError("buffers['ws']: need %d bytes on a 256-byte boundary, got %d bytes at offset %d mod 256"
                             % (nbytes, have, ptr % 256))
        return ws, ptr, have
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    if ws.data_ptr() % 256:
        ws = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256, nbytes


# ---------------------------------------------------------------------------------------------------------------------------
# the warp of the whole source pyramid (include/sfmwarp.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _warp_pyramid_desc(src_pyr, disps, poses, K, layout, pose_shape=(6,)):
    """(descriptor with the inputs bound, the arrays it points at, B, n_src, [(h, w)], device) for warp_pyramid_fwd / _bwd"""
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'planar' or 'hwc', got %r" % (layout,))
    hwc = layout == "hwc"
    S, n_src = len(disps), len(poses)
    if len(src_pyr) != S or not 1 <= S <= _lib.SFM_MAX_SCALES or not 1 <= n_src <= _lib.SFM_MAX_SRC:
        raise TypeError("src_pyr and disps need one entry per scale (1..%d), poses one per source (1..%d)"
                        % (_lib.SFM_MAX_SCALES, _lib.SFM_MAX_SRC))
    src_pyr, disps, poses = _devs(src_pyr, "src_pyr", 5 if hwc else 4), _devs(disps, "disps", 4), _devs(poses, "poses", 1 + len(pose_shape))
    K = _dev(K, "intrinsics", 4)
    B, dev = disps[0].shape[0], disps[0].device
    if tuple(K.shape) != (B, S, 3, 3):
        raise TypeError("intrinsics must be (B,%d,3,3), got %s" % (S, tuple(K.shape)))
    hw = [tuple(t.shape[2:]) for t in disps]
    for s, (h, w) in enumerate(hw):
        want = (B, n_src, h, w, 3) if hwc else (B, 3 * n_src, h, w)
        if tuple(src_pyr[s].shape) != want or tuple(disps[s].shape) != (B, 1, h, w):
            raise TypeError("scale %d: expected src %s and disp (B,1,h,w), got %s and %s"
                            % (s, want, tuple(src_pyr[s].shape), tuple(disps[s].shape)))
    for i, t in enumerate(poses):
        if tuple(t.shape) != (B,) + pose_shape:
            raise TypeError("poses[%d] must be %s" % (i, _POSE_SHAPE_NAMES[pose_shape]))
    _one_device(dev, src_pyr + disps + poses + [K])
    d = SfmWarpPyramidDesc()
    d.B, d.n_src, d.image_layout = B, n_src, _LAYOUTS[layout]
    _set_scales(d, hw)
    d.intrinsics = K.data_ptr()
    for field, arrays in ((d.src, src_pyr), (d.disp, disps), (d.pose, poses)):
        _point(field, arrays)
    return d, (src_pyr, disps, poses, K), B, n_src, hw, dev


_POSE_SHAPE_NAMES = {(6,): "(B,6)", (3, 4): "(B,3,4)"}


def _warp_pyramid_calls(conv):
    """(fwd, workspace query, bwd) as callables of the existing signatures: the existing symbols without conventions, those of
    include/sfmwarp_pose.h with `conv` bound otherwise"""
    if conv is None:
        return lib.sfm_warp_pyramid_fwd, lib.sfm_warp_pyramid_bwd_workspace_bytes, lib.sfm_warp_pyramid_bwd
    c = C.byref(conv)
    return (lambda d, *rest: lib.sfm_warp_pyramid_conv_fwd(d, c, *rest),
            lambda d: lib.sfm_warp_pyramid_conv_bwd_workspace_bytes(d, c),
            lambda d, *rest: lib.sfm_warp_pyramid_conv_bwd(d, c, *rest))


def warp_pyramid_fwd(src_pyr, disps, poses, K, layout, want_valid=False, pose_format="euler", invert=None, depth_affine=None):
    """Every scale and source of a step warped in ONE launch (sfm_warp_pyramid_fwd): src_pyr[s] (B,3*n_src,h,w) for layout
    "planar" or (B,n_src,h,w,3) for "hwc" (what `pyramid_hwc` writes), disps[s] (B,1,h,w), poses[i] (B,6), K (B,S,3,3) ->
    [warped_s (B,n_src,3,h,w)], each `warp_fwd` of that (scale, source) with depth 1 / disp bit for bit; with `want_valid` also
    [valid_s (B,n_src,h,w)]: 1.0 where the sample passes both strict tests of models/transform.py:129, else 0.0.
    pose_format, invert, depth_affine: the conventions of include/sfmwarp_pose.h (`pose_conv`); "matrix" takes poses[i] (B,3,4)."""
    conv = pose_conv(pose_format, invert, depth_affine, len(poses))
    fwd = _warp_pyramid_calls(conv)[0]
    d, keep, B, n_src, hw, dev = _warp_pyramid_desc(src_pyr, disps, poses, K, layout, _pose_shape(conv))
    warped = _empty([(B, n_src, 3, h, w) for h, w in hw], dev)
    valid = _empty([(B, n_src, h, w) for h, w in hw], dev) if want_valid else None
    _point(d.warped, warped)
    _point(d.valid, valid or ())
    _launch(dev, fwd, C.byref(d))
    return (warped, valid) if want_valid else warped


def warp_pyramid_bwd(src_pyr, disps, poses, K, layout, g_warped, pose_format="euler", invert=None, depth_affine=None):
    """The backward of `warp_pyramid_fwd` for the upstream gradients g_warped[s] (B,n_src,3,h,w): one launch over the pixels and a
    small fold (sfm_warp_pyramid_bwd) -> ([d_disp_s (B,1,h,w)], [d_pose_i (B,6)]).  No atomics: the same bits on every call.
    Under pose_format="matrix" d_pose_i is (B,3,4): the gradient of the matrix itself."""
    conv = pose_conv(pose_format, invert, depth_affine, len(poses))
    _, query, bwd = _warp_pyramid_calls(conv)
    d, keep, B, n_src, hw, dev = _warp_pyramid_desc(src_pyr, disps, poses, K, layout, _pose_shape(conv))
    if len(g_warped) != len(hw):
        raise TypeError("g_warped needs one entry per scale")
    g_warped = _devs(g_warped, "g_warped", 5)
    for s, (h, w) in enumerate(hw):
        if tuple(g_warped[s].shape) != (B, n_src, 3, h, w) or g_warped[s].device != dev:
            raise TypeError("g_warped[%d] must be (B,n_src,3,h,w) = %s on %s" % (s, (B, n_src, 3, h, w), dev))
    d_disps = _empty([(B, 1, h, w) for h, w in hw], dev)
    d_poses = _empty([(B,) + _pose_shape(conv)] * n_src, dev)
    for field, arrays in ((d.g_warped, g_warped), (d.d_disp, d_disps), (d.d_pose, d_poses)):
        _point(field, arrays)
    nbytes = query(C.byref(d))
    if nbytes == 0:
        check(bwd(C.byref(d), None, 0, None))   # re-run the validation for its message
        raise ValueError(_lib.last_error() or "invalid warp pyramid descriptor")
    ws, ptr, have = _place_workspace(None, nbytes, dev)
    _launch(dev, bwd, C.byref(d), C.c_void_p(ptr), have)
    return d_disps, d_poses


# ---------------------------------------------------------------------------------------------------------------------------
# the geometry-consistency term of SC-SfMLearner (include/sfmwarp_depth_consistency.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _depth_cons_desc(disps, src_disps, poses, K, pose_shape=(6,)):
    """(descriptor with the inputs bound, the arrays it points at, B, n_src, [(h, w)], device) for depth_consistency_fwd / _bwd"""
    S, n_src = len(disps), len(poses)
    if len(src_disps) != S or not 1 <= S <= _lib.SFM_MAX_SCALES or not 1 <= n_src <= _lib.SFM_MAX_SRC:
        raise TypeError("disps and src_disps need one entry per scale (1..%d), poses one per source (1..%d)"
                        % (_lib.SFM_MAX_SCALES, _lib.SFM_MAX_SRC))
    disps, src_disps, poses = _devs(disps, "disps", 4), _devs(src_disps, "src_disps", 4), _devs(poses, "poses", 1 + len(pose_shape))
    K = _dev(K, "intrinsics", 4)
    B, dev = disps[0].shape[0], disps[0].device
    if tuple(K.shape) != (B, S, 3, 3):
        raise TypeError("intrinsics must be (B,%d,3,3), got %s" % (S, tuple(K.shape)))
    hw = [tuple(t.shape[2:]) for t in disps]
    for s, (h, w) in enumerate(hw):
        if tuple(disps[s].shape) != (B, 1, h, w) or tuple(src_disps[s].shape) != (B, n_src, h, w):
            raise TypeError("scale %d: expected disp (B,1,h,w) and src_disp %s, got %s and %s"
                            % (s, (B, n_src, h, w), tuple(disps[s].shape), tuple(src_disps[s].shape)))
    for i, t in enumerate(poses):
        if tuple(t.shape) != (B,) + pose_shape:
            raise TypeError("poses[%d] must be %s" % (i, _POSE_SHAPE_NAMES[pose_shape]))
    _one_device(dev, disps + src_disps + poses + [K])
    d = SfmDepthConsDesc()
    d.B, d.n_src = B, n_src
    _set_scales(d, hw)
    d.intrinsics = K.data_ptr()
    for field, arrays in ((d.disp, disps), (d.src_disp, src_disps), (d.pose, poses)):
        _point(field, arrays)
    return d, (disps, src_disps, poses, K), B, n_src, hw, dev


def _conv_ref(conv):
    return C.byref(conv) if conv is not None else None


def depth_consistency_fwd(disps, src_disps, poses, K, want_valid=False, want_depths=False, pose_format="euler", invert=None,
                          depth_affine=None):
    """The geometry-consistency maps of every scale and source in ONE launch (sfm_depth_consistency_fwd): disps[s] (B,1,h,w) the
    target's disparity, src_disps[s] (B,n_src,h,w) the sources' own, poses[i] (B,6), K (B,S,3,3) -> [diff_s (B,n_src,h,w)]:
    |computed - projected| / (computed + projected) where the sample is in view, exactly 0 elsewhere -- computed the depth of the
    target pixel's 3-D point in the source camera (clamped at 1e-3), projected the source's depth map sampled where it lands, at the
    positions of `warp_pyramid_fwd` bit for bit.  With `want_valid` also [valid_s], with `want_depths` also [computed_s] and
    [projected_s], all (B,n_src,h,w); returned as (diff, valid, computed, projected) without the lists that were not asked for.
    pose_format, invert, depth_affine: the conventions of include/sfmwarp_pose.h (`pose_conv`), the affine map applied to both
    disparities; "matrix" takes poses[i] (B,3,4)."""
    conv = pose_conv(pose_format, invert, depth_affine, len(poses))
    d, keep, B, n_src, hw, dev = _depth_cons_desc(disps, src_disps, poses, K, _pose_shape(conv))
    shapes = [(B, n_src, h, w) for h, w in hw]
    diff = _empty(shapes, dev)
    valid = _empty(shapes, dev) if want_valid else None
    computed, projected = (_empty(shapes, dev), _empty(shapes, dev)) if want_depths else (None, None)
    for field, arrays in ((d.diff, diff), (d.valid, valid), (d.computed, computed), (d.projected, projected)):
        _point(field, arrays or ())
    _launch(dev, lib.sfm_depth_consistency_fwd, C.byref(d), _conv_ref(conv))
    out = (diff,) + ((valid,) if want_valid else ()) + ((computed, projected) if want_depths else ())
    return out if len(out) > 1 else diff


def depth_consistency_bwd(disps, src_disps, poses, K, g_diff, want_d_src_disp=True, ws=None, pose_format="euler", invert=None,
                          depth_affine=None):
    """The backward of `depth_consistency_fwd` for the upstream gradients g_diff[s] (B,n_src,h,w): one launch over the pixels and a
    small fold (sfm_depth_consistency_bwd) -> ([d_disp_s (B,1,h,w)], [d_pose_i (B,6)], [d_src_disp_s (B,n_src,h,w)] or None).
    d_disp and d_pose: no atomics, the same bits on every call, whatever `ws` (the caller's workspace, or None for a fresh one)
    held.  d_src_disp is scattered with float atomics (equal up to the order of the additions); want_d_src_disp=False launches the
    kernel without the scatter.  Under pose_format="matrix" d_pose_i is (B,3,4): the gradient of the matrix itself."""
    conv = pose_conv(pose_format, invert, depth_affine, len(poses))
    d, keep, B, n_src, hw, dev = _depth_cons_desc(disps, src_disps, poses, K, _pose_shape(conv))
    if len(g_diff) != len(hw):
        raise TypeError("g_diff needs one entry per scale")
    g_diff = _devs(g_diff, "g_diff", 4)
    for s, (h, w) in enumerate(hw):
        if tuple(g_diff[s].shape) != (B, n_src, h, w) or g_diff[s].device != dev:
            raise TypeError("g_diff[%d] must be (B,n_src,h,w) = %s on %s" % (s, (B, n_src, h, w), dev))
    d_disps = _empty([(B, 1, h, w) for h, w in hw], dev)
    d_poses = _empty([(B,) + _pose_shape(conv)] * n_src, dev)
    d_src_disps = _empty([(B, n_src, h, w) for h, w in hw], dev) if want_d_src_disp else None      # (the call clears them itself)
    for field, arrays in ((d.g_diff, g_diff), (d.d_disp, d_disps), (d.d_pose, d_poses), (d.d_src_disp, d_src_disps or ())):
        _point(field, arrays)
    nbytes = lib.sfm_depth_consistency_bwd_workspace_bytes(C.byref(d), _conv_ref(conv))
    if nbytes == 0:
        check(lib.sfm_depth_consistency_bwd(C.byref(d), _conv_ref(conv), None, 0, None))   # re-run the validation for its message
        raise ValueError(_lib.last_error() or "invalid depth consistency descriptor")
    ws, ptr, have = _place_workspace(ws, nbytes, dev)
    _launch(dev, lib.sfm_depth_consistency_bwd, C.byref(d), _conv_ref(conv), C.c_void_p(ptr), have)
    return d_disps, d_poses, d_src_disps


# ---------------------------------------------------------------------------------------------------------------------------
# the full-resolution multi-scale warp: every disparity upsampled inside the warp (include/sfmwarp_full_res.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _warp_full_res_desc(src, disps, poses, K, layout, pose_shape=(6,)):
    """(descriptor with the inputs bound, the arrays it points at, B, n_src, (H, W), [(h, w)], device) for warp_full_res_fwd / _bwd"""
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'planar' or 'hwc', got %r" % (layout,))
    hwc = layout == "hwc"
    S, n_src = len(disps), len(poses)
    if not 1 <= S <= _lib.SFM_MAX_SCALES or not 1 <= n_src <= _lib.SFM_MAX_SRC:
        raise TypeError("disps needs one entry per scale (1..%d), poses one per source (1..%d)" % (_lib.SFM_MAX_SCALES, _lib.SFM_MAX_SRC))
    src, disps, poses = _dev(src, "src", 5 if hwc else 4), _devs(disps, "disps", 4), _devs(poses, "poses", 1 + len(pose_shape))
    K = _dev(K, "intrinsics", 3)
    B, dev = src.shape[0], src.device
    H, W = (src.shape[2:4] if hwc else src.shape[2:])
    if tuple(src.shape) != ((B, n_src, H, W, 3) if hwc else (B, 3 * n_src, H, W)):
        raise TypeError("src must be %s for %d poses, got %s" % ("(B,n_src,H,W,3)" if hwc else "(B,3*n_src,H,W)", n_src, tuple(src.shape)))
    if tuple(K.shape) != (B, 3, 3):
        raise TypeError("intrinsics must be (B,3,3), got %s" % (tuple(K.shape),))
    for s, t in enumerate(disps):
        if tuple(t.shape[:2]) != (B, 1):
            raise TypeError("disps[%d] must be (B,1,h,w) = (%d,1,h,w), got %s" % (s, B, tuple(t.shape)))
    for i, t in enumerate(poses):
        if tuple(t.shape) != (B,) + pose_shape:
            raise TypeError("poses[%d] must be %s" % (i, _POSE_SHAPE_NAMES[pose_shape]))
    _one_device(dev, disps + poses + [K])
    hw = [tuple(t.shape[2:]) for t in disps]
    d = SfmWarpFullResDesc()
    d.B, d.n_src, d.n_scales, d.H, d.W, d.image_layout = B, n_src, S, H, W, _LAYOUTS[layout]
    for s, (h, w) in enumerate(hw):
        d.h[s], d.w[s] = h, w
    d.src, d.intrinsics = src.data_ptr(), K.data_ptr()
    for field, arrays in ((d.disp, disps), (d.pose, poses)):
        _point(field, arrays)
    return d, (src, disps, poses, K), B, n_src, (H, W), hw, dev


def _warp_full_res_conv_calls(upsample, conv):
    """`_warp_full_res_calls` under the conventions `conv` (`pose_conv`): without any (None) exactly that; otherwise the entry points
    of include/sfmwarp_pose.h with the upsampling and the conventions bound"""
    if conv is None:
        return _warp_full_res_calls(upsample)
    up, c = _lib.upsample_id(upsample), C.byref(conv)
    return (lambda d, *rest: lib.sfm_warp_full_res_conv_fwd(d, up, c, *rest),
            lambda d: lib.sfm_warp_full_res_conv_bwd_workspace_bytes(d, up, c),
            lambda d, *rest: lib.sfm_warp_full_res_conv_bwd(d, up, c, *rest))


def _warp_full_res_calls(upsample):
    """(fwd, workspace query, bwd) as callables of the existing signatures: the existing symbols for "align_corners", those of
    include/sfmwarp_conventions.h with the value bound for "half_pixel"; an unknown name is a ValueError"""
    if upsample == "align_corners":
        return lib.sfm_warp_full_res_fwd, lib.sfm_warp_full_res_bwd_workspace_bytes, lib.sfm_warp_full_res_bwd
    up = _lib.upsample_id(upsample)
    return (lambda d, *rest: lib.sfm_warp_full_res_up_fwd(d, up, *rest),
            lambda d: lib.sfm_warp_full_res_up_bwd_workspace_bytes(d, up),
            lambda d, *rest: lib.sfm_warp_full_res_up_bwd(d, up, *rest))


def warp_full_res_fwd(src, disps, poses, K, layout, want_valid=False, upsample="align_corners", pose_format="euler", invert=None,
                      depth_affine=None):
    """ONE full-resolution source set warped with the disparity of every scale, each upsampled to (H, W) inside the kernel, in ONE
    launch (sfm_warp_full_res_fwd): src (B,3*n_src,H,W) for layout "planar" or (B,n_src,H,W,3) for "hwc", disps[s] (B,1,h_s,w_s) of any
    sizes, poses[i] (B,6), K (B,3,3) -> [warped_s (B,n_src,3,H,W)]: `warp_pyramid_fwd` at equal sizes on `resize` of each disparity
    (itself where it has the full size), bit for bit; with `want_valid` also [valid_s (B,n_src,H,W)].  upsample="half_pixel": each
    disparity upsampled as F.interpolate(mode="bilinear", align_corners=False) does instead (sfm_warp_full_res_up_fwd).
    pose_format, invert, depth_affine: the conventions of include/sfmwarp_pose.h (`pose_conv`); the affine map acts on the
    upsampled disparity; "matrix" takes poses[i] (B,3,4)."""
    conv = pose_conv(pose_format, invert, depth_affine, len(poses))
    fwd = _warp_full_res_conv_calls(upsample, conv)[0]
    d, keep, B, n_src, (H, W), hw, dev = _warp_full_res_desc(src, disps, poses, K, layout, _pose_shape(conv))
    warped = _empty([(B, n_src, 3, H, W)] * len(hw), dev)
    valid = _empty([(B, n_src, H, W)] * len(hw), dev) if want_valid else None
    _point(d.warped, warped)
    _point(d.valid, valid or ())
    _launch(dev, fwd, C.byref(d))
    return (warped, valid) if want_valid else warped


def warp_full_res_bwd(src, disps, poses, K, layout, g_warped, ws=None, upsample="align_corners", pose_format="euler", invert=None,
                      depth_affine=None):
    """The backward of `warp_full_res_fwd` for the upstream gradients g_warped[s] (B,n_src,3,H,W): one launch over the pixels, one
    that gathers every low-resolution gradient and a small fold (sfm_warp_full_res_bwd) -> ([d_disp_s (B,1,h_s,w_s)], [d_pose_i
    (B,6)]): `warp_pyramid_bwd` at equal sizes followed by `resize_bwd` of each d_disp, bit for bit.  No atomics: the same bits on
    every call, whatever `ws` (the caller's workspace, or None for a fresh one) held.  upsample="half_pixel": the backward of that
    forward (sfm_warp_full_res_up_bwd), each d_disp the adjoint of the half-pixel upsampling; the workspace is the same.
    Under pose_format="matrix" d_pose_i is (B,3,4): the gradient of the matrix itself."""
    conv = pose_conv(pose_format, invert, depth_affine, len(poses))
    _, query, bwd = _warp_full_res_conv_calls(upsample, conv)
    d, keep, B, n_src, (H, W), hw, dev = _warp_full_res_desc(src, disps, poses, K, layout, _pose_shape(conv))
    if len(g_warped) != len(hw):
        raise TypeError("g_warped needs one entry per scale")
    g_warped = _devs(g_warped, "g_warped", 5)
    for s, g in enumerate(g_warped):
        if tuple(g.shape) != (B, n_src, 3, H, W) or g.device != dev:
            raise TypeError("g_warped[%d] must be (B,n_src,3,H,W) = %s on %s" % (s, (B, n_src, 3, H, W), dev))
    d_disps = _empty([(B, 1, h, w) for h, w in hw], dev)
    d_poses = _empty([(B,) + _pose_shape(conv)] * n_src, dev)
    for field, arrays in ((d.g_warped, g_warped), (d.d_disp, d_disps), (d.d_pose, d_poses)):
        _point(field, arrays)
    nbytes = query(C.byref(d))
    if nbytes == 0:
        check(bwd(C.byref(d), None, 0, None))   # re-run the validation for its message
        raise ValueError(_lib.last_error() or "invalid full-resolution warp descriptor")
    ws, ptr, have = _place_workspace(ws, nbytes, dev)
    _launch(dev, bwd, C.byref(d), C.c_void_p(ptr), have)
    return d_disps, d_poses


# ---------------------------------------------------------------------------------------------------------------------------
# the per-pixel photometric error maps of a warped pyramid (include/sfmwarp.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _photo_error_desc(imgs, tgts, ssim_rate):
    """(descriptor with the inputs bound, the arrays it points at, B, n_img, [(h, w)], device) for photo_error_fwd / _bwd"""
    if not isinstance(imgs, (list, tuple)) or not isinstance(tgts, (list, tuple)):
        raise TypeError("imgs and tgts must be lists with one array per scale")
    S = len(imgs)
    if len(tgts) != S or not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("imgs and tgts need one entry per scale (1..%d), got %d and %d" % (_lib.SFM_MAX_SCALES, S, len(tgts)))
    imgs, tgts = _devs(imgs, "imgs", 5), _devs(tgts, "tgts", 4)
    B, n_img = imgs[0].shape[:2]
    dev = imgs[0].device
    if not 1 <= n_img <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d images per sample, got %d" % (_lib.SFM_MAX_SRC, n_img))
    hw = [tuple(t.shape[3:]) for t in imgs]
    for s, (h, w) in enumerate(hw):
        if tuple(imgs[s].shape) != (B, n_img, 3, h, w) or tuple(tgts[s].shape) != (B, 3, h, w):
            raise TypeError("scale %d: expected imgs (B,n_img,3,h,w) = %s and tgts (B,3,h,w), got %s and %s"
                            % (s, (B, n_img, 3, h, w), tuple(imgs[s].shape), tuple(tgts[s].shape)))
    _one_device(dev, imgs + tgts)
    d = SfmPhotoErrorDesc()
    d.B, d.n_img, d.ssim_rate = B, n_img, float(ssim_rate)
    _set_scales(d, hw)
    for field, arrays in ((d.img, imgs), (d.tgt, tgts)):
        _point(field, arrays)
    return d, (imgs, tgts), B, n_img, hw, dev


def _photo_error_calls(padding):
    """(fwd, bwd) as callables of the existing signatures: the existing symbols for "zero", those of include/sfmwarp_conventions.h
    with the value bound for "reflect"; an unknown name is a ValueError"""
    if padding == "zero":
        return lib.sfm_photo_error_fwd, lib.sfm_photo_error_bwd
    pad = _lib.ssim_padding_id(padding)
    return (lambda d, *rest: lib.sfm_photo_error_pad_fwd(d, pad, *rest)), (lambda d, *rest: lib.sfm_photo_error_pad_bwd(d, pad, *rest))


def photo_error_fwd(imgs, tgts, ssim_rate, padding="zero"):
    """The photometric error map of every (scale, image) of a step in ONE launch (sfm_photo_error_fwd): imgs[s] (B,n_img,3,h,w) --
    what `warp_pyramid_fwd` returns, or the planar source pyramid viewed so --, tgts[s] (B,3,h,w) -> [err_s (B,n_img,h,w)],
    err = (1 - ssim_rate) * mean_c |X - Y| + ssim_rate * mean_c compute_ssim(X, Y) of models/base_model.py:126-142 per pixel.  A
    rejection by the library (ssim_rate outside [0,1]) is a ValueError with sfm_last_error() as its message.  padding="reflect": the
    3x3 SSIM window over the image extended by ReflectionPad2d(1) (sfm_photo_error_pad_fwd; every h, w >= 2, else TypeError)."""
    fwd = _photo_error_calls(padding)[0]
    d, keep, B, n_img, hw, dev = _photo_error_desc(imgs, tgts, ssim_rate)
    err = _empty([(B, n_img, h, w) for h, w in hw], dev)
    _point(d.err, err)
    _launch(dev, fwd, C.byref(d))
    return err


def photo_error_bwd(imgs, tgts, ssim_rate, g_err, padding="zero"):
    """The backward of `photo_error_fwd` for the upstream gradients g_err[s] (B,n_img,h,w), ONE launch (sfm_photo_error_bwd) ->
    [d_img_s (B,n_img,3,h,w)].  The targets are constants.  No atomics: the same bits on every call.  `padding` as in the forward."""
    bwd = _photo_error_calls(padding)[1]
    d, keep, B, n_img, hw, dev = _photo_error_desc(imgs, tgts, ssim_rate)
    if not isinstance(g_err, (list, tuple)) or len(g_err) != len(hw):
        raise TypeError("g_err needs one entry per scale")
    g_err = _devs(g_err, "g_err", 4)
    for s, (h, w) in enumerate(hw):
        if tuple(g_err[s].shape) != (B, n_img, h, w) or g_err[s].device != dev:
            raise TypeError("g_err[%d] must be (B,n_img,h,w) = %s on %s" % (s, (B, n_img, h, w), dev))
    d_imgs = _empty([(B, n_img, 3, h, w) for h, w in hw], dev)
    for field, arrays in ((d.g_err, g_err), (d.d_img, d_imgs)):
        _point(field, arrays)
    _launch(dev, bwd, C.byref(d))
    return d_imgs


# ---------------------------------------------------------------------------------------------------------------------------
# the minimum over the sources, the auto-mask and the mean of every scale (include/sfmwarp_min_reproj.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _min_reproj_desc(B, n_err, n_ident, hw, weights, norm):
    """An SfmMinReprojDesc with every non-pointer field set.  norm: "kept" or "all"; weights: one non-negative number per scale"""
    if len(weights) != len(hw) or not 1 <= len(hw) <= _lib.SFM_MAX_SCALES:
        raise TypeError("one weight per scale (1..%d), got %d weights for %d scales" % (_lib.SFM_MAX_SCALES, len(weights), len(hw)))
    d = SfmMinReprojDesc()
    d.B, d.n_err, d.n_ident, d.norm = B, n_err, n_ident, _lib.min_reproj_norm_id(norm)
    _set_scales(d, hw)
    for s, w in enumerate(weights):
        d.weight[s] = float(w)
    return d


def min_reproj_fwd(errs, valids, idents, weights, norm):
    """Per pixel the smallest error over the sources, the auto-mask and the mean of every scale in two launches
    (sfm_min_reproj_fwd): errs[s] (B,n_err,h,w) -- what `photo_error_fwd` returns for the warped pyramid --, valids None or a list
    with (B,n_err,h,w) or None per scale (sources with valid <= 0 at a pixel do not compete), idents None (no auto-mask) or
    [(B,n_ident,h,w)], the errors of the unwarped sources: a pixel is kept where some valid source has a finite error that is
    strictly below every ident.  weights: one per scale; norm: "kept" (the mean over the kept pixels) or "all" (over all pixels).
    -> (loss (S+1,) float32: the mean of each scale and, last, their weighted sum; count (S,) int32: the kept pixels;
    [winner_s (B,h,w) int8]: the index of the source a kept pixel took its error from, else -1).  No atomics: the same bits on
    every call.  A rejection by the library (a negative weight) is a ValueError with sfm_last_error() as its message."""
    if not isinstance(errs, (list, tuple)) or not 1 <= len(errs) <= _lib.SFM_MAX_SCALES:
        raise TypeError("errs must be a list with one array per scale (1..%d)" % _lib.SFM_MAX_SCALES)
    S = len(errs)
    errs = _devs(errs, "errs", 4)
    B, n_err = errs[0].shape[:2]
    dev = errs[0].device
    if not 1 <= n_err <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d error maps per sample, got %d" % (_lib.SFM_MAX_SRC, n_err))
    hw = [tuple(t.shape[2:]) for t in errs]
    valids = [None] * S if valids is None else list(valids)
    if len(valids) != S or (idents is not None and len(idents) != S):
        raise TypeError("valids and idents need one entry per scale")
    valids = [None if t is None else _dev(t, "valids[%d]" % s, 4) for s, t in enumerate(valids)]
    idents = [] if idents is None else _devs(idents, "idents", 4)
    n_ident = idents[0].shape[1] if idents else 0
    if idents and not 1 <= n_ident <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d identity maps per sample, got %d" % (_lib.SFM_MAX_SRC, n_ident))
    for s, (h, w) in enumerate(hw):
        if tuple(errs[s].shape) != (B, n_err, h, w) or (valids[s] is not None and valids[s].shape != errs[s].shape):
            raise TypeError("scale %d: errs and valids must be (B,n_err,h,w) = %s" % (s, (B, n_err, h, w)))
        if idents and tuple(idents[s].shape) != (B, n_ident, h, w):
            raise TypeError("idents[%d] must be (B,n_ident,h,w) = %s, got %s" % (s, (B, n_ident, h, w), tuple(idents[s].shape)))
    _one_device(dev, errs + [t for t in valids if t is not None] + idents)
    d = _min_reproj_desc(B, n_err, n_ident, hw, weights, norm)
    loss = torch.empty((S + 1,), dtype=torch.float32, device=dev)
    count = torch.empty((S,), dtype=torch.int32, device=dev)
    winners = [torch.empty((B, h, w), dtype=torch.int8, device=dev) for h, w in hw]
    for field, arrays in ((d.err, errs), (d.valid, valids), (d.ident, idents), (d.winner, winners)):
        _point(field, arrays)
    d.loss, d.count = loss.data_ptr(), count.data_ptr()
    if B == 0:      # the mean of nothing, as the library defines it for a scale with nothing kept; nothing to launch
        return loss.zero_(), count.zero_(), winners
    nbytes = lib.sfm_min_reproj_workspace_bytes(C.byref(d))
    if nbytes == 0:
        check(lib.sfm_min_reproj_fwd(C.byref(d), None, 0, None))   # re-run the validation for its message
        raise ValueError(_lib.last_error() or "invalid min reprojection descriptor")
    ws, ptr, have = _place_workspace(None, nbytes, dev)
    _launch(dev, lib.sfm_min_reproj_fwd, C.byref(d), C.c_void_p(ptr), have)
    return loss, count, winners


def min_reproj_bwd(winners, count, g_loss, n_err, weights, norm, shapes):
    """The backward of `min_reproj_fwd` for the upstream gradients g_loss (S+1,) of its `loss`, ONE launch (sfm_min_reproj_bwd):
    winners and count as the forward returned them, shapes = [(h, w)] -> [g_err_s (B,n_err,h,w)], c_s at the winning source of a
    kept pixel and 0 everywhere else, c_s = (g_loss[s] + weights[s] * g_loss[S]) / denom[s].  The kernel reads count and g_loss on
    the device: nothing syncs."""
    hw = [tuple(x) for x in shapes]
    S = len(hw)
    if not isinstance(winners, (list, tuple)) or len(winners) != S or not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("winners and shapes need one entry per scale (1..%d)" % _lib.SFM_MAX_SCALES)
    if not 1 <= int(n_err) <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d error maps per sample, got %d" % (_lib.SFM_MAX_SRC, n_err))
    g_loss = _dev(g_loss, "g_loss", 1)
    dev = g_loss.device
    B = winners[0].shape[0] if isinstance(winners[0], torch.Tensor) and winners[0].dim() == 3 else -1
    for s, (t, (h, w)) in enumerate(zip(winners, hw)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int8 or tuple(t.shape) != (B, h, w) or not t.is_contiguous():
            raise TypeError("winners[%d] must be a contiguous int8 array (B,h,w) = %s" % (s, (B, h, w)))
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or tuple(count.shape) != (S,) or not count.is_contiguous():
        raise TypeError("count must be a contiguous int32 array (%d,)" % S)
    if tuple(g_loss.shape) != (S + 1,):
        raise TypeError("g_loss must be (%d,), got %s" % (S + 1, tuple(g_loss.shape)))
    _one_device(dev, list(winners) + [count])
    d = _min_reproj_desc(B, int(n_err), 0, hw, weights, norm)
    g_errs = _empty([(B, int(n_err), h, w) for h, w in hw], dev)
    for field, arrays in ((d.winner, winners), (d.g_err, g_errs)):
        _point(field, arrays)
    d.count, d.g_loss = count.data_ptr(), g_loss.data_ptr()
    _launch(dev, lib.sfm_min_reproj_bwd, C.byref(d))
    return g_errs


# ---------------------------------------------------------------------------------------------------------------------------
# the masked means of SC-SfMLearner's compute_pairwise_loss for every scale and source (include/sfmwarp_pairwise.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _pairwise_desc(errs, diffs, weights, min_counts, detach_weight):
    """(descriptor with err, diff and every setting bound, the arrays it points at, B, n_src, [(h, w)], device) for pairwise_fwd / _bwd"""
    if not isinstance(errs, (list, tuple)) or not isinstance(diffs, (list, tuple)):
        raise TypeError("errs and diffs must be lists with one array per scale")
    S = len(errs)
    if len(diffs) != S or not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("errs and diffs need one entry per scale (1..%d), got %d and %d" % (_lib.SFM_MAX_SCALES, S, len(diffs)))
    if len(weights) != S:
        raise TypeError("one weight per scale (1..%d), got %d weights for %d scales" % (_lib.SFM_MAX_SCALES, len(weights), S))
    errs, diffs = _devs(errs, "errs", 4), _devs(diffs, "diffs", 4)
    B, n_src = errs[0].shape[:2]
    dev = errs[0].device
    if not 1 <= n_src <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d sources, got %d" % (_lib.SFM_MAX_SRC, n_src))
    hw = [tuple(t.shape[2:]) for t in errs]
    for s, (h, w) in enumerate(hw):
        if tuple(errs[s].shape) != (B, n_src, h, w) or diffs[s].shape != errs[s].shape:
            raise TypeError("scale %d: errs and diffs must be (B,n_src,h,w) = %s, got %s and %s"
                            % (s, (B, n_src, h, w), tuple(errs[s].shape), tuple(diffs[s].shape)))
    _one_device(dev, errs + diffs)
    d = SfmPairwiseDesc()
    d.B, d.n_src, d.detach_weight = B, n_src, int(bool(detach_weight))
    d.min_count_photo, d.min_count_geom = (int(v) for v in min_counts)
    _set_scales(d, hw)
    for s, w in enumerate(weights):
        d.weight[s] = float(w)
    for field, arrays in ((d.err, errs), (d.diff, diffs)):
        _point(field, arrays)
    return d, (errs, diffs), B, n_src, hw, dev


def _pairwise_maps(ts, name, errs):
    """None, or one float32 array of the shape of errs[s] per scale"""
    if ts is None:
        return []
    if not isinstance(ts, (list, tuple)) or len(ts) != len(errs):
        raise TypeError("%s needs one entry per scale" % name)
    ts = _devs(ts, name, 4)
    for s, t in enumerate(ts):
        if t.shape != errs[s].shape:
            raise TypeError("%s[%d] must be (B,n_src,h,w) = %s, got %s" % (name, s, tuple(errs[s].shape), tuple(t.shape)))
    return ts


def pairwise_fwd(errs, diffs, valids, idents, cmps, weights, min_counts, detach_weight):
    """Per (scale, source) the mean of err * (1 - diff) and of diff over the kept pixels of the whole batch, and their weighted totals,
    in two launches (sfm_pairwise_fwd): errs[s], diffs[s] (B,n_src,h,w) -- what `photo_error_fwd` returns for the warped pyramid and
    `depth_consistency_fwd` for the same pose --; valids None or a list with (B,n_src,h,w) or None per scale (a pixel with
    valid <= 0 is dropped); idents None (no auto-mask) or [(B,n_src,h,w)], the errors of the unwarped sources: a pixel is kept only
    where cmps[s] (None: errs[s]) is strictly below it.  weights: one per scale; min_counts = (photo, geometry): a mean over at most
    that many pixels is 0; detach_weight: looked at by the backward only.
    -> (loss (2*S*n_src+2,) float32: photo[s*n_src+i], geom[s*n_src+i], photo_total, geom_total; count (S*n_src,) int32: the kept
    pixels; [keep_s (B,n_src,h,w) int8]).  Sums are fp64 in a fixed order, no atomics: the same bits on every call.  A rejection by
    the library (a negative weight or min_count) is a ValueError with sfm_last_error() as its message."""
    d, held, B, n_src, hw, dev = _pairwise_desc(errs, diffs, weights, min_counts, detach_weight)
    errs, S = held[0], len(hw)
    valids = [None] * S if valids is None else list(valids)
    if len(valids) != S:
        raise TypeError("valids needs one entry per scale")
    valids = [None if t is None else _dev(t, "valids[%d]" % s, 4) for s, t in enumerate(valids)]
    for s, t in enumerate(valids):
        if t is not None and t.shape != errs[s].shape:
            raise TypeError("valids[%d] must be (B,n_src,h,w) = %s, got %s" % (s, tuple(errs[s].shape), tuple(t.shape)))
    idents, cmps = _pairwise_maps(idents, "idents", errs), _pairwise_maps(cmps, "cmps", errs)
    if cmps and not idents:
        raise TypeError("cmps without idents: there is nothing to compare them with")
    _one_device(dev, [t for t in valids if t is not None] + idents + cmps)
    loss = torch.empty((2 * S * n_src + 2,), dtype=torch.float32, device=dev)
    count = torch.empty((S * n_src,), dtype=torch.int32, device=dev)
    keeps = [torch.empty((B, n_src, h, w), dtype=torch.int8, device=dev) for h, w in hw]
    for field, arrays in ((d.valid, valids), (d.ident, idents), (d.cmp, cmps), (d.keep, keeps)):
        _point(field, arrays)
    d.loss, d.count = loss.data_ptr(), count.data_ptr()
    if B == 0:      # the mean of nothing, as the library defines it for a pair with nothing kept; nothing to launch
        return loss.zero_(), count.zero_(), keeps
    nbytes = lib.sfm_pairwise_workspace_bytes(C.byref(d))
    if nbytes == 0:
        check(lib.sfm_pairwise_fwd(C.byref(d), None, 0, None))   # re-run the validation for its message
        raise ValueError(_lib.last_error() or "invalid pairwise descriptor")
    ws, ptr, have = _place_workspace(None, nbytes, dev)
    _launch(dev, lib.sfm_pairwise_fwd, C.byref(d), C.c_void_p(ptr), have)
    return loss, count, keeps


def pairwise_bwd(errs, diffs, keeps, count, g_loss, weights, min_counts, detach_weight, want_g_diff=True):
    """The backward of `pairwise_fwd` for the upstream gradients g_loss (2*S*n_src+2,) of its `loss`, ONE launch (sfm_pairwise_bwd):
    keeps and count as the forward returned them -> ([g_err_s (B,n_src,h,w)], [g_diff_s (B,n_src,h,w)] or None without
    `want_g_diff`): g_err = (1 - diff) * cp and g_diff = cg - err * cp (cg alone with `detach_weight`) at a kept pixel, 0 elsewhere,
    cp / cg = (g_loss[photo / geom s,i] + weights[s] * g_loss[photo / geom total]) / max(count, 1), 0 where count <= min_count.
    The kernel reads count and g_loss on the device: nothing syncs."""
    d, held, B, n_src, hw, dev = _pairwise_desc(errs, diffs, weights, min_counts, detach_weight)
    S = len(hw)
    if not isinstance(keeps, (list, tuple)) or len(keeps) != S:
        raise TypeError("keeps needs one entry per scale")
    for s, (t, (h, w)) in enumerate(zip(keeps, hw)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int8 or tuple(t.shape) != (B, n_src, h, w) or not t.is_contiguous():
            raise TypeError("keeps[%d] must be a contiguous int8 array (B,n_src,h,w) = %s" % (s, (B, n_src, h, w)))
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or tuple(count.shape) != (S * n_src,) or not count.is_contiguous():
        raise TypeError("count must be a contiguous int32 array (%d,)" % (S * n_src))
    g_loss = _dev(g_loss, "g_loss", 1)
    if tuple(g_loss.shape) != (2 * S * n_src + 2,):
        raise TypeError("g_loss must be (%d,), got %s" % (2 * S * n_src + 2, tuple(g_loss.shape)))
    _one_device(dev, list(keeps) + [count, g_loss])
    shapes = [(B, n_src, h, w) for h, w in hw]
    g_errs = _empty(shapes, dev)
    g_diffs = _empty(shapes, dev) if want_g_diff else None
    for field, arrays in ((d.keep, keeps), (d.g_err, g_errs), (d.g_diff, g_diffs or ())):
        _point(field, arrays)
    d.count, d.g_loss = count.data_ptr(), g_loss.data_ptr()
    _launch(dev, lib.sfm_pairwise_bwd, C.byref(d))
    return g_errs, g_diffs


# ---------------------------------------------------------------------------------------------------------------------------
# the edge-aware smoothness of the (mean-normalised) disparity of every scale (include/sfmwarp_disp_smooth.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _disp_smooth_desc(disps, tgts, weights, normalize, edge):
    """(descriptor with the inputs and every setting bound, the arrays it points at, B, [(h, w)], device) for disp_smooth_fwd / _bwd"""
    if not isinstance(disps, (list, tuple)) or not isinstance(tgts, (list, tuple)):
        raise TypeError("disps and tgts must be lists with one array per scale")
    S = len(disps)
    if len(tgts) != S or not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("disps and tgts need one entry per scale (1..%d), got %d and %d" % (_lib.SFM_MAX_SCALES, S, len(tgts)))
    if len(weights) != S:
        raise TypeError("one weight per scale (1..%d), got %d weights for %d scales" % (_lib.SFM_MAX_SCALES, len(weights), S))
    disps, tgts = _devs(disps, "disps", 4), _devs(tgts, "tgts", 4)
    B, dev = disps[0].shape[0], disps[0].device
    hw = [tuple(t.shape[2:]) for t in disps]
    for s, (h, w) in enumerate(hw):
        if tuple(disps[s].shape) != (B, 1, h, w) or tuple(tgts[s].shape) != (B, 3, h, w):
            raise TypeError("scale %d: expected disps (B,1,h,w) = %s and tgts (B,3,h,w), got %s and %s"
                            % (s, (B, 1, h, w), tuple(disps[s].shape), tuple(tgts[s].shape)))
    _one_device(dev, disps + tgts)
    d = SfmDispSmoothDesc()
    d.B, d.normalize, d.edge = B, int(bool(normalize)), _lib.disp_smooth_edge_id(edge)
    _set_scales(d, hw)
    for s, w in enumerate(weights):
        d.weight[s] = float(w)
    for field, arrays in ((d.disp, disps), (d.img, tgts)):
        _point(field, arrays)
    return d, (disps, tgts), B, hw, dev


def disp_smooth_fwd(disps, tgts, weights, normalize, edge):
    """The edge-aware smoothness of the disparity of every scale in two launches (sfm_disp_smooth_fwd): disps[s] (B,1,h,w),
    tgts[s] (B,3,h,w) planar, the images whose edges relax the penalty; weights: one per scale; normalize: divide each sample's
    disparity by its own mean + 1e-7 first (Monodepth2) -- done by factoring |M_b| out of the sums, in the same pass; edge:
    "mean_abs" (exp(-mean_c |dI|), Monodepth2) or "abs_mean" (exp(-|mean_c dI|), compute_disp_smooth of models/base_model.py:144-155).
    -> (loss (S+1,) float32: mean_x + mean_y of each scale and, last, their weighted sum; stats (S,B,3) float64: per (scale, sample)
    M_b, X_b, Y_b of the header, which `disp_smooth_bwd` reads).  No atomics: the same bits on every call.  A rejection by the library
    (a negative weight) is a ValueError with sfm_last_error() as its message."""
    d, keep, B, hw, dev = _disp_smooth_desc(disps, tgts, weights, normalize, edge)
    S = len(hw)
    loss = torch.empty((S + 1,), dtype=torch.float32, device=dev)
    stats = torch.empty((S, B, 3), dtype=torch.float64, device=dev)
    d.loss, d.stats = loss.data_ptr(), stats.data_ptr()
    if B == 0:      # the sum over no samples; nothing to launch
        return loss.zero_(), stats
    nbytes = lib.sfm_disp_smooth_workspace_bytes(C.byref(d))
    if nbytes == 0:
        check(lib.sfm_disp_smooth_fwd(C.byref(d), None, 0, None))   # re-run the validation for its message
        raise ValueError(_lib.last_error() or "invalid disparity smoothness descriptor")
    ws, ptr, have = _place_workspace(None, nbytes, dev)
    _launch(dev, lib.sfm_disp_smooth_fwd, C.byref(d), C.c_void_p(ptr), have)
    return loss, stats


def disp_smooth_bwd(disps, tgts, stats, g_loss, weights, normalize, edge, out=None):
    """The backward of `disp_smooth_fwd` for the upstream gradients g_loss (S+1,) of its `loss`, ONE launch (sfm_disp_smooth_bwd):
    stats as the forward returned it -> [g_disp_s (B,1,h,w)].  With `out`, a list of S contiguous float32 arrays (B,1,h,w), the
    gradient is ADDED to them in place (one fp32 addition per element) and they are returned.  The images get no gradient.  The kernel
    reads stats and g_loss on the device: nothing syncs."""
    d, keep, B, hw, dev = _disp_smooth_desc(disps, tgts, weights, normalize, edge)
    S = len(hw)
    g_loss = _dev(g_loss, "g_loss", 1)
    if tuple(g_loss.shape) != (S + 1,):
        raise TypeError("g_loss must be (%d,), got %s" % (S + 1, tuple(g_loss.shape)))
    if not isinstance(stats, torch.Tensor) or stats.dtype != torch.float64 or tuple(stats.shape) != (S, B, 3) or not stats.is_contiguous():
        raise TypeError("stats must be a contiguous float64 array (%d,%d,3)" % (S, B))
    _one_device(dev, [g_loss, stats])
    if out is None:
        g_disps = _empty([(B, 1, h, w) for h, w in hw], dev)
    else:
        if not isinstance(out, (list, tuple)) or len(out) != S:
            raise TypeError("out needs one entry per scale")
        g_disps = list(out)
        for s, (t, (h, w)) in enumerate(zip(g_disps, hw)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (B, 1, h, w) or not t.is_contiguous() \
                    or t.device != dev:
                raise TypeError("out[%d] must be a contiguous float32 array (B,1,h,w) = %s on %s" % (s, (B, 1, h, w), dev))
        d.accumulate = 1
    _point(d.g_disp, g_disps)
    d.stats, d.g_loss = stats.data_ptr(), g_loss.data_ptr()
    _launch(dev, lib.sfm_disp_smooth_bwd, C.byref(d))
    return g_disps


class FusedLoss:
    """One bound instance of the fused multi-scale loss (sfm_loss_fwd / _bwd / _fwd_bwd):
    descriptor + caller-owned workspace and outputs.  Re-usable across steps as long as the
    input tensors keep their addresses (call `bind` again otherwise)."""

    def __init__(self, smooth_reg=0.0, exp_reg=0.0, ssim_rate=0.0, smooth_mode="second_order", projection="fast"):
        """projection: "fast" (SFM_PROJECTION_FAST) or "reference_order" (SFM_PROJECTION_REFERENCE_ORDER: the per-pixel chain of
        models/transform.py:105-108,122-131 in the reference's own rounding sequence; include/sfmwarp.h says what each guarantees)."""
        self.smooth_mode = _lib.smooth_mode_id(smooth_mode)
        self.projection = _lib.projection_id(projection)
        self.smooth_reg = float(smooth_reg or 0.0)
        self.exp_reg = float(exp_reg or 0.0)
        self.ssim_rate = float(ssim_rate or 0.0)
        self.desc = None
        self._keep = None

    def bind(self, tgt_pyr, src_pyr, intrinsics, disps, poses, masks=None, norm_B=None, want_d_src=False, layout="planar",
             want_warped=False, buffers=None, want_d_intrinsics=False, want_d_proj=False):
        """layout: "planar" -- tgt (B,3,h,w), src (B,3*n_src,h,w) as in the reference; "hwc" -- tgt (B,1,h,w,3),
        src (B,n_src,h,w,3) as written by `pyramid_hwc` (the faster layout for these kernels; same results).
        want_warped: `forward` / `forward_backward` also write `self.warped[s]` (B,n_src,3,h,w), the warped source images the
        loss was computed on (curr_proj_img, models/base_model.py:90-94; planar in both layouts).
        want_d_intrinsics / want_d_proj: every gradient call (`backward`, `forward_backward`, `step_from_frames(grad=True)`) is
        followed by ONE small launch (sfm_loss_proj_bwd) that leaves `self.d_intrinsics` (B,S,3,3), the gradient with respect to
        the intrinsics, and / or `self.d_proj` (B,S,n_src,3,4), dL/dPm of every proj_tgt_to_src call -- both scaled by the gy of
        that call.  Off (the default): not one launch or allocation more.
        buffers: optional dict of caller-owned arrays to use instead of allocating -- any of "d_disps", "d_poses", "d_masks",
        "warped" (lists, one array per scale / source), "d_srcs" (one array or None per scale: replaces `want_d_src`; the caller's
        arrays are cleared before every backward like the own ones), "loss5" ((5,) float32) and "ws" (a contiguous device tensor of
        any dtype that starts on a 256-byte boundary; ALL its bytes are handed over as the workspace, and it must hold at least
        sfm_loss_workspace_bytes).  Float arrays need the shapes given above and 4-byte alignment, nothing more."""
        keep = self._check_inputs(tgt_pyr, src_pyr, intrinsics, disps, poses, masks, layout)
        tgt_pyr, src_pyr, intrinsics, disps, poses, masks = keep
        B, n_src, dev = tgt_pyr[0].shape[0], len(poses), tgt_pyr[0].device
        hw = [tuple(t.shape[2:]) for t in disps]
        d = loss_desc(B, int(norm_B if norm_B is not None else B), n_src, hw,
                      (self.smooth_reg, self.exp_reg, self.ssim_rate, self.smooth_mode, self.projection), layout)
        # outputs: the caller's (`buffers`) or fresh ones
        buffers = dict(buffers or {})
        use_masks = self.exp_reg > 0
        d_disps = _owns(buffers, "d_disps", [t.shape for t in disps], dev)
        d_poses = _owns(buffers, "d_poses", [t.shape for t in poses], dev)
        d_masks = _owns(buffers, "d_masks", [t.shape for t in masks], dev) if use_masks else None
        warped = _owns(buffers, "warped", [(B, n_src, 3, h, w) for h, w in hw], dev) if want_warped else None     # always planar
        d_src_all, d_srcs = _d_src_arrays(buffers, want_d_src, [(B, 3 * n_src, h, w) for h, w in hw], dev)
        d.intrinsics = intrinsics.data_ptr()
        for field, arrays in ((d.tgt, tgt_pyr), (d.src, src_pyr), (d.disp, disps), (d.pose, poses), (d.d_disp, d_disps),
                              (d.d_pose, d_poses), (d.d_src, d_srcs), (d.mask_logits, masks if use_masks else ()),
                              (d.d_mask, d_masks or ()), (d.warped, warped or ())):
            _point(field, arrays)
        self.ws, self._ws_ptr, self._ws_bytes = _place_workspace(buffers.get("ws"), workspace_bytes(d), dev)
        self.loss5 = torch.zeros((5,), dtype=torch.float32, device=dev) if buffers.get("loss5") is None \
            else _own(buffers, "loss5", 0, (5,), dev)
        self.desc, self.device = d, dev
        self._desc_ref, self._ws_arg, self._loss5_arg = C.byref(d), C.c_void_p(self._ws_ptr), _p(self.loss5)
        self.d_disps, self.d_poses, self.d_masks, self.warped = d_disps, d_poses, d_masks, warped
        self._d_src_all, self.d_srcs = d_src_all, (d_srcs if any(t is not None for t in d_srcs) else None)
        S = len(hw)
        self.d_intrinsics = torch.empty((B, S, 3, 3), dtype=torch.float32, device=dev) if want_d_intrinsics else None
        self.d_proj = torch.empty((B, S, n_src, 3, 4), dtype=torch.float32, device=dev) if want_d_proj else None
        self._proj_args = (_p(self.d_proj), _p(self.d_intrinsics)) if want_d_intrinsics or want_d_proj else None
        self._keep = keep
        return self

    def _proj_bwd(self, loss):
        """sfm_loss_proj_bwd behind a gradient call (loss: 0 after sfm_loss_bwd, 1 after sfm_loss_fwd_bwd / sfm_step_fwd_bwd)"""
        if self._proj_args is not None:
            _launch(self.device, lib.sfm_loss_proj_bwd, self._desc_ref, loss, self._ws_arg, self._ws_bytes, *self._proj_args)

    def _check_inputs(self, tgt_pyr, src_pyr, intrinsics, disps, poses, masks, layout):
        """bind's arguments as contiguous float32 device arrays of consistent shapes, in the order of `_keep`"""
        if layout not in _LAYOUTS:
            raise ValueError("layout must be 'planar' or 'hwc', got %r" % (layout,))
        hwc = layout == "hwc"
        S = len(disps)
        if not (len(tgt_pyr) == len(src_pyr) == S):
            raise TypeError("tgt_pyr, src_pyr and disps must have one entry per scale")
        if S > _lib.SFM_MAX_SCALES or len(poses) > _lib.SFM_MAX_SRC:
            raise TypeError("at most %d scales and %d sources" % (_lib.SFM_MAX_SCALES, _lib.SFM_MAX_SRC))
        tgt_pyr, src_pyr = _devs(tgt_pyr, "tgt_pyr", 5 if hwc else 4), _devs(src_pyr, "src_pyr", 5 if hwc else 4)
        disps, poses = _devs(disps, "disps", 4), _devs(poses, "poses", 2)
        intrinsics = _dev(intrinsics, "intrinsics", 4)
        B, n_src = tgt_pyr[0].shape[0], len(poses)
        if tuple(intrinsics.shape) != (B, S, 3, 3):
            raise TypeError("intrinsics must be (B,%d,3,3), got %s" % (S, tuple(intrinsics.shape)))
        use_masks = self.exp_reg > 0         # (without the term, `masks` is kept as given and never read)
        if use_masks:
            if masks is None:
                raise ValueError("exp_reg > 0 needs the explainability logits (masks)")
            masks = _devs(masks, "masks", 4)
        for s in range(S):
            h, w = disps[s].shape[2:]
            want = ((B, 1, h, w, 3), (B, n_src, h, w, 3)) if hwc else ((B, 3, h, w), (B, 3 * n_src, h, w))
            if (tuple(tgt_pyr[s].shape), tuple(src_pyr[s].shape)) != want or tuple(disps[s].shape) != (B, 1, h, w):
                raise TypeError("scale %d: expected tgt (B,3,h,w), src (B,3*n_src,h,w) [hwc: (B,1,h,w,3), (B,n_src,h,w,3)], "
                                "disp (B,1,h,w)" % s)
            if use_masks and tuple(masks[s].shape) != (B, n_src, h, w):
                raise TypeError("masks[%d] must be (B,n_src,h,w)" % s)
        for i in range(n_src):
            if tuple(poses[i].shape) != (B, 6):
                raise TypeError("poses[%d] must be (B,6)" % i)
        return tgt_pyr, src_pyr, intrinsics, disps, poses, masks

    def rebind(self, intrinsics, disps, poses, masks=None):
        """Points the bound descriptor at other input arrays of the SAME shapes (the network outputs of the next
        iteration); pyramids, workspace and gradient buffers stay.  Only pointers change: the plan cached inside the
        library for this descriptor shape is found again as long as the addresses repeat."""
        d = self.desc
        old = self._keep
        intrinsics = _dev(intrinsics, "intrinsics", 4)
        disps, poses = _devs(disps, "disps", 4), _devs(poses, "poses", 2)
        if intrinsics.shape != old[2].shape or len(disps) != len(old[3]) or len(poses) != len(old[4]) \
                or any(a.shape != b.shape for a, b in zip(disps, old[3])) or any(a.shape != b.shape for a, b in zip(poses, old[4])):
            raise TypeError("rebind: shapes differ from the bound ones (call bind)")
        if self.exp_reg > 0:
            if masks is None:
                raise ValueError("exp_reg > 0 needs the explainability logits (masks)")
            masks = _devs(masks, "masks", 4)
            if any(a.shape != b.shape for a, b in zip(masks, old[5])):
                raise TypeError("rebind: mask shapes differ from the bound ones (call bind)")
            _point(d.mask_logits, masks)
        else:
            masks = None
        d.intrinsics = intrinsics.data_ptr()
        _point(d.disp, disps)
        _point(d.pose, poses)
        self._keep = (old[0], old[1], intrinsics, disps, poses, masks)
        return self

    def _zero_d_src(self):
        if self.d_srcs is None:
            return
        if self._d_src_all is not None:
            self._d_src_all.zero_()
        else:      # the caller's arrays (bind(buffers=...)): one fill each
            for t in self.d_srcs:
                if t is not None:
                    t.zero_()

    def _loss5(self, out):
        """(the array that receives the five scalars, its pointer argument): `out` if the caller gave one, else self.loss5.  The
        argument objects that never change between calls are built once per bind (a step is 70 us of GPU time: the host side of
        a call has to stay well below)."""
        return (self.loss5, self._loss5_arg) if out is None else (out, C.c_void_p(out.data_ptr()))

    def step_from_frames(self, tgt_full, src_full, grad=True, out=None):
        """One step from the FULL-RESOLUTION frames in one call through the C ABI (sfm_step_fwd_bwd / sfm_step_fwd): both pyramids
        are written into the pixel-interleaved buffers this instance was bound to (layout="hwc"), then the fused loss runs.
        tgt_full (B,3,H,W), src_full (B,3*n_src,H,W): float32, contiguous, on the bound device -- the CALLER vouches for that
        (links.SFMLearnerLoss validates once per set of arrays); nothing is checked here but what the library checks itself."""
        self._zero_d_src()
        loss5, l5 = self._loss5(out)
        _launch(self.device, lib.sfm_step_fwd_bwd if grad else lib.sfm_step_fwd, tgt_full.data_ptr(), src_full.data_ptr(),
                self._desc_ref, l5, self._ws_arg, self._ws_bytes)
        if grad:
            self._proj_bwd(1)
        return loss5

    def forward(self, out=None):
        """`out`: as for forward_backward."""
        loss5, l5 = self._loss5(out)
        _launch(self.device, lib.sfm_loss_fwd, self._desc_ref, l5, self._ws_arg, self._ws_bytes)
        return loss5

    def backward(self, gy=1.0):
        self._zero_d_src()
        _launch(self.device, lib.sfm_loss_bwd, self._desc_ref, float(gy), self._ws_arg, self._ws_bytes)
        self._proj_bwd(0)
        return self.d_disps, self.d_poses, self.d_masks, self.d_srcs

    def forward_backward(self, out=None, variant=0):
        """`out`: optional (5,) float32 device tensor to receive the five scalars instead of `self.loss5`
        (lets a caller keep a log of the steps of a reporting interval and reduce it across ranks once).
        `variant`: development hook (sfm_loss_variant): 3 = the kernels read their header from the argument struct."""
        self._zero_d_src()
        loss5, l5 = self._loss5(out)
        if variant:
            check(lib.sfm_loss_variant(int(variant)))
        _launch(self.device, lib.sfm_loss_fwd_bwd, self._desc_ref, l5, self._ws_arg, self._ws_bytes)
        self._proj_bwd(1)
        return loss5
