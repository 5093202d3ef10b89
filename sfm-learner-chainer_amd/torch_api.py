"""PyTorch autograd route to the fused loss and to the operators.

The reference's networks (DispNet, PoseNet) are Chainer links; on this stack they are `torch.nn` modules whose outputs carry a
grad_fn.  This module hands those outputs to libsfmwarp and the gradients it computes back to torch.autograd:

  sfm_learner_loss / SFMLearnerLoss   the loss of models/base_model.py:48-124 as a function and as a torch.nn.Module
  projective_inverse_warp             models/transform.py:156-193 (ops.warp_fwd / ops.warp_bwd / ops.warp_bwd_intrinsics)
  warp_pyramid                        the warped source images of EVERY (scale, source) of a step, models/base_model.py:69-94, for a
                                      loss of the caller's own (ops.pyramid_hwc, ops.warp_pyramid_fwd / ops.warp_pyramid_bwd)
  warp_full_res                       the full-resolution sources warped with the disparity of EVERY scale, each upsampled inside the
                                      warp: Monodepth2's full-resolution multi-scale (ops.warp_full_res_fwd / ops.warp_full_res_bwd)
  pose_matrix                         a 6-vector (axis-angle or Euler, optionally inverted) -> the rigid 3x4 the warps take with
                                      pose_format="matrix": Monodepth2's transformation_from_parameters (ops.pose_mat_fwd / ops.pose_mat_bwd)
  photometric_error                   alpha * SSIM + (1 - alpha) * L1 per pixel (models/base_model.py:96,126-142) of every (scale, image) of
                                      a step, differentiable w.r.t. the images (ops.photo_error_fwd / ops.photo_error_bwd)
  min_reprojection                    the stage behind it: per pixel the minimum over the sources, the auto-mask against the unwarped
                                      sources and the mean of every scale (ops.min_reproj_fwd / ops.min_reproj_bwd)
  min_reprojection_loss               warp_pyramid -> photometric_error -> min_reprojection as one call and ONE autograd node
  depth_consistency                   SC-SfMLearner's diff_depth of every (scale, source) (ops.depth_consistency_fwd / _bwd)
  pairwise_mean                       the stage behind it and photometric_error: the masked means of compute_pairwise_loss per (scale,
                                      source), with the auto-mask and the mean_on_mask threshold (ops.pairwise_fwd / ops.pairwise_bwd)
  sc_sfm_loss                         SC-SfMLearner's objective, both directions: one autograd node per direction
  multi_scale_intrinsics              datasets/kitti/kitti_raw_transformed.py:76-93, differentiable (plain torch)
  disp_activation                     models/disp_net.py:104-122 (ops.disp_act_fwd / ops.disp_act_bwd)
  resize_images / resize_like         F.resize_images as DispNet's decoder differentiates it, models/disp_net.py:11-14,105,111,117
                                      (ops.resize / ops.resize_bwd)

The loss is custom operators (torch.library), so that FakeTensor and torch.compile can trace it:

  sfmwarp::sfm_learner_loss   ONE fused call computes the five scalars and, when a gradient is wanted, every gradient for gy = 1
                              (sfm_step_fwd_bwd; the planar pyramid + sfm_loss_fwd_bwd for frames of HWC_MAX_PIXELS or more)
  sfmwarp::sfm_learner_loss_k the same call followed by sfm_loss_proj_bwd: also the gradient of the intrinsics (used when they require one)
  sfmwarp::scale_arrays       its backward: those gradients times the upstream gradient, which the kernel reads on the device
                              (sfm_scale_arrays), written out of place

Eagerly the same launches run through a torch.autograd.Function (_LossFunction): the generic argument handling of a Python custom
operator costs more host time per call than a whole step at the reference's batch.  torch.compile traces the operators.

Nothing here reads a device value on the host: a step runs under torch.cuda.graph capture, GradScaler, autocast and
torch.compile (backend="aot_eager" keeps the hot path in libsfmwarp: no generated kernels).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from . import _lib, ops
from ._lib import SfmLossDesc, lib

__all__ = ["sfm_learner_loss", "SFMLearnerLoss", "projective_inverse_warp", "disp_activation", "resize_images", "resize_like",
           "scale_arrays_into", "multi_scale_intrinsics", "warp_pyramid", "photometric_error",
           "min_reprojection", "min_reprojection_loss", "disparity_smoothness", "warp_full_res", "pose_matrix",
           "depth_consistency", "pairwise_mean", "sc_sfm_loss"]

_ALIGN = 64                  # floats: every array inside a per-call buffer starts on a 256-byte boundary
_MAX_ARRAYS = 32             # sfm_scale_arrays


def _round(n):
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def _grad_spans(disps, poses, masks, K=None):
    """[offset0, numel0, offset1, numel1, ...] of the unit-gradient arrays d_disp[s], d_pose[i], d_mask[s] (in that order) and, with
    `K` (the intrinsics, when their gradient is wanted), d_intrinsics behind them inside the one buffer the loss op returns, that
    buffer's length in floats, and the arrays' shapes."""
    spans, off, shapes = [], 0, []
    for t in list(disps) + list(poses) + list(masks) + ([K] if K is not None else []):
        n = t.numel()
        spans += [off, n]
        off += _round(n)
        shapes.append(tuple(t.shape))
    return spans, off, shapes


def _views(buf, spans, shapes):
    """the arrays that lie at `spans` in the flat buffer `buf`"""
    return [buf[o:o + n].view(shape) for o, n, shape in zip(spans[0::2], spans[1::2], shapes)]


# ---------------------------------------------------------------------------------------------------------------------------
# sfm_scale_arrays
# ---------------------------------------------------------------------------------------------------------------------------
def _launch_scale(xp, yp, numel, gy, device):
    n = len(numel)
    ptr = C.c_void_p * n
    ops._launch(device, lib.sfm_scale_arrays, ptr(*xp), ptr(*yp), (C.c_longlong * n)(*numel), n, C.c_void_p(gy.data_ptr()))


def _gy(gy):
    gy = ops._dev(gy, "gy")
    if gy.numel() != 1:
        raise TypeError("gy must hold one element, got shape %s" % (tuple(gy.shape),))
    return gy


def scale_arrays_into(xs, ys, gy):
    """ys[k][...] = xs[k] * gy for up to 32 float32 device arrays in ONE launch (sfm_scale_arrays).  gy: a float32 device tensor of
    one element, read by the kernel (no host sync).  ys[k] may be xs[k] (in place); contiguous arrays of equal sizes only."""
    if len(xs) != len(ys) or not 1 <= len(xs) <= _MAX_ARRAYS:
        raise TypeError("scale_arrays_into: 1..%d arrays and as many outputs, got %d and %d" % (_MAX_ARRAYS, len(xs), len(ys)))
    gy = _gy(gy)
    for k, (x, y) in enumerate(zip(xs, ys)):
        for t, name in ((x, "xs[%d]" % k), (y, "ys[%d]" % k)):
            ops._dev(t, name)
            if not t.is_contiguous():
                raise TypeError("%s: expected a contiguous array" % name)
            if t.device != gy.device:
                raise TypeError("%s lives on %s, gy on %s" % (name, t.device, gy.device))
        if x.numel() != y.numel():
            raise TypeError("xs[%d] has %d elements, ys[%d] %d" % (k, x.numel(), k, y.numel()))
    _launch_scale([x.data_ptr() for x in xs], [y.data_ptr() for y in ys], [x.numel() for x in xs], gy, gy.device)
    return ys


def _check_spans(spans, n):
    """spans = [offset0, numel0, ...]: at most 32 pairs, every span inside a buffer of n elements (before any launch)."""
    if len(spans) % 2 or len(spans) > 2 * _MAX_ARRAYS:
        raise TypeError("scale_arrays: spans must hold at most %d (offset, numel) pairs, got %d values" % (_MAX_ARRAYS, len(spans)))
    for k in range(0, len(spans), 2):
        o, m = spans[k], spans[k + 1]
        if o < 0 or m < 0 or o + m > n:
            raise TypeError("scale_arrays: span %d = (offset %d, numel %d) lies outside x's %d elements" % (k // 2, o, m, n))


def _scaled(x, spans, gy):
    """sfmwarp::scale_arrays on checked arguments (the eager backward calls it directly): one launch, none for no spans."""
    out = torch.empty_like(x)
    if spans:
        xb, yb = x.data_ptr(), out.data_ptr()
        offs = spans[0::2]
        _launch_scale([xb + 4 * o for o in offs], [yb + 4 * o for o in offs], spans[1::2], gy, x.device)
    return out


@torch.library.custom_op("sfmwarp::scale_arrays", mutates_args=())
def _scale_arrays_op(x: Tensor, spans: list[int], gy: Tensor) -> Tensor:
    """x: a flat float32 device buffer that holds up to 32 arrays at spans = [offset0, numel0, offset1, numel1, ...] (floats) ->
    a NEW buffer of x's size whose spans hold x * gy[0], one launch.  Elements outside the spans are not written."""
    _check_spans(spans, x.numel())
    x, gy = ops._dev(x, "x", 1), _gy(gy)
    if gy.device != x.device:
        raise TypeError("scale_arrays: gy lives on %s, x on %s" % (gy.device, x.device))
    return _scaled(x, spans, gy)


@_scale_arrays_op.register_fake
def _(x, spans, gy):
    _check_spans(spans, x.numel())
    return torch.empty_like(x)


# ---------------------------------------------------------------------------------------------------------------------------
# the fused loss
# ---------------------------------------------------------------------------------------------------------------------------
class _Plan:
    """Host-side constants of one configuration (shapes, settings, entry point): the descriptor with everything but the pointers,
    the workspace size and where each array lies in the per-call scratch buffer.  No device memory."""
    __slots__ = ("desc", "hwc", "ws_bytes", "tgt_off", "src_off", "ws_off", "scratch", "spans", "grad_floats")


_PLANS = {}                 # at most _MAX_PLANS configurations, oldest dropped first
_MAX_PLANS = 16
_FAKE = 0x1000             # placeholder pointer for sizing the workspace: never dereferenced
_desc_hook = None           # measurement hook (tools/torch_step_time.py): called with the descriptor bytes of every launch


def _plan(B, H, W, n_src, disps, masks, poses, cfg, K=None):
    """K: the intrinsics when the call also returns their gradient (a span of its own behind the others), else None"""
    S = len(disps)
    shapes = tuple(tuple(t.shape) for t in disps)
    key = (B, H, W, n_src, shapes, len(masks), cfg, K is not None)
    p = _PLANS.get(key)
    if p is not None:
        return p
    p = _Plan()
    layout = ops.layout_for(H, W)
    p.hwc = layout == "hwc"
    d = ops.loss_desc(B, cfg[5], n_src, [shape[2:] for shape in shapes], cfg[:5], layout)
    for s in range(S):
        d.tgt[s] = d.src[s] = d.disp[s] = d.d_disp[s] = _FAKE
        if masks:
            d.mask_logits[s] = d.d_mask[s] = _FAKE
    for i in range(n_src):
        d.pose[i] = d.d_pose[i] = _FAKE
    d.intrinsics = _FAKE
    p.desc, p.ws_bytes = bytes(d), ops.workspace_bytes(d)
    # scratch: the pyramids (hwc: every scale of both; planar: scales 1.. -- scale 0 is the frame itself), then the workspace
    off, p.tgt_off, p.src_off = 0, [], []
    for s in range(S):
        h, w = shapes[s][2], shapes[s][3]
        if p.hwc or s > 0:
            p.tgt_off.append(off)
            off += _round(B * 3 * h * w)
            p.src_off.append(off)
            off += _round(B * 3 * n_src * h * w)
        else:
            p.tgt_off.append(None)
            p.src_off.append(None)
    p.ws_off = off
    p.scratch = off + _round(p.ws_bytes // 4) + _ALIGN    # + the slack to put the workspace on a 256-byte boundary
    p.spans, p.grad_floats, _ = _grad_spans(disps, poses, masks, K)
    if len(_PLANS) >= _MAX_PLANS:
        _PLANS.pop(next(iter(_PLANS)))            # the oldest configuration (e.g. an epoch's last, smaller batch)
    _PLANS[key] = p
    return p


def _run_loss(tgt, src, K, disps, poses, masks, cfg, grad, grad_k=False):
    """grad_k (with grad): one more launch, sfm_loss_proj_bwd, leaves d_intrinsics for gy = 1 in the last span of the buffer"""
    dev = tgt.device
    B, _, H, W = tgt.shape
    n_src = len(poses)
    grad_k = grad and grad_k
    p = _plan(B, H, W, n_src, disps, masks, poses, cfg, K if grad_k else None)
    d = SfmLossDesc.from_buffer_copy(p.desc)
    scratch = torch.empty((p.scratch,), dtype=torch.float32, device=dev)
    base = scratch.data_ptr()
    base += (-base) % 256
    loss5 = torch.empty((5,), dtype=torch.float32, device=dev)
    g = torch.empty((p.grad_floats if grad else 0,), dtype=torch.float32, device=dev)
    gb = g.data_ptr()
    S = len(disps)
    for s in range(S):
        d.disp[s] = disps[s].data_ptr()
        if masks:
            d.mask_logits[s] = masks[s].data_ptr()
        if p.tgt_off[s] is None:
            d.tgt[s], d.src[s] = tgt.data_ptr(), src.data_ptr()
        else:
            d.tgt[s], d.src[s] = base + 4 * p.tgt_off[s], base + 4 * p.src_off[s]
    for i in range(n_src):
        d.pose[i] = poses[i].data_ptr()
    d.intrinsics = K.data_ptr()
    if grad:
        sp = p.spans
        for s in range(S):
            d.d_disp[s] = gb + 4 * sp[2 * s]
            if masks:
                d.d_mask[s] = gb + 4 * sp[2 * (S + n_src + s)]
        for i in range(n_src):
            d.d_pose[i] = gb + 4 * sp[2 * (S + i)]
    else:
        for s in range(S):
            d.d_disp[s] = d.d_mask[s] = None
        for i in range(n_src):
            d.d_pose[i] = None
    if _desc_hook is not None:
        _desc_hook(bytes(d))
    ws = C.c_void_p(base + 4 * p.ws_off)
    l5 = C.c_void_p(loss5.data_ptr())
    if p.hwc:
        fn = lib.sfm_step_fwd_bwd if grad else lib.sfm_step_fwd
        ops._launch(dev, fn, tgt.data_ptr(), src.data_ptr(), C.byref(d), l5, ws, p.ws_bytes)
    else:
        for x, pyr, G in ((tgt, d.tgt, 3), (src, d.src, 3 * n_src)):
            if S > 1:
                ops._launch(dev, lib.sfm_pyramid_fwd, x.data_ptr(), (C.c_void_p * S)(*pyr[:S]), B, G, H, W, S)
        ops._launch(dev, lib.sfm_loss_fwd_bwd if grad else lib.sfm_loss_fwd, C.byref(d), l5, ws, p.ws_bytes)
    if grad_k and B > 0:
        ops._launch(dev, lib.sfm_loss_proj_bwd, C.byref(d), 1, ws, p.ws_bytes, None, C.c_void_p(gb + 4 * p.spans[-2]))
    return loss5, g


def _loss_op_body(grad_k):
    def body(tgt_img: Tensor, src_imgs: Tensor, intrinsics: Tensor, disps: list[Tensor], poses: list[Tensor],
             masks: list[Tensor], smooth_reg: float, exp_reg: float, ssim_rate: float, smooth_mode: int, projection: int,
             norm_batch: int, grad: bool) -> list[Tensor]:
        cfg = (float(smooth_reg), float(exp_reg), float(ssim_rate), int(smooth_mode), int(projection), int(norm_batch))
        loss5, unit = _run_loss(tgt_img, src_imgs, intrinsics, disps, poses, masks, cfg, grad, grad_k)
        return [loss5[0], loss5[1:].clone(), unit]          # (an operator's outputs may not share storage)
    return body


def _register_loss_op(name, grad_k):
    """sfmwarp::<name>: the fused loss on validated arrays: tgt_img (B,3,H,W), src_imgs (B,3*n_src,H,W), intrinsics (B,S,3,3),
    disps[s] (B,1,h,w), poses[i] (B,6), masks[s] (B,n_src,h,w) or no masks (an empty list: no explainability term) -- float32,
    contiguous, one device.  smooth_mode / projection: _lib.SMOOTH_* / _lib.SFM_PROJECTION_*.

    Returns [total (), terms (4,) = (pixel, smooth, exp, ssim), unit_grads]: unit_grads is ONE flat float32 buffer that holds
    d_disp[s], d_pose[i], d_mask[s] -- the gradients of total for gy = 1, in that order, each at an offset rounded up to 64
    floats (_grad_spans) -- when `grad`, else empty.  grad_k (the operator sfm_learner_loss_k, same arguments): d_intrinsics
    (B,S,3,3) follows them, and the backward hands it to `intrinsics`.  (Two operators, not one with a flag: the first keeps its
    signature, and a traced call drops a trailing argument that equals its default.)"""
    op = torch.library.custom_op("sfmwarp::" + name, mutates_args=())(_loss_op_body(grad_k))

    @op.register_fake
    def _(tgt_img, src_imgs, intrinsics, disps, poses, masks, smooth_reg, exp_reg, ssim_rate, smooth_mode, projection, norm_batch,
          grad):
        n = _grad_spans(disps, poses, masks, intrinsics if grad and grad_k else None)[1]
        f = dict(dtype=torch.float32, device=tgt_img.device)
        return [torch.empty((), **f), torch.empty((4,), **f), torch.empty((n if grad else 0,), **f)]

    def setup_context(ctx, inputs, output):
        disps, poses, masks = inputs[3], inputs[4], inputs[5]
        ctx.grad = inputs[12]
        ctx.spans, _, ctx.shapes = _grad_spans(disps, poses, masks, inputs[2] if ctx.grad and grad_k else None)
        ctx.counts = (len(disps), len(poses), len(masks))
        ctx.mark_non_differentiable(output[1], output[2])
        ctx.save_for_backward(output[2])

    def backward(ctx, grads):
        S, n, m = ctx.counts
        (unit,) = ctx.saved_tensors
        if not ctx.grad:        # no prediction required a gradient (only an image or the intrinsics did): none flows anywhere
            return (None, None, None, [None] * S, [None] * n, [None] * m, None, None, None, None, None, None, None)
        gy = grads[0].to(torch.float32)
        views = _views(torch.ops.sfmwarp.scale_arrays(unit, ctx.spans, gy), ctx.spans, ctx.shapes)
        return (None, None, views[S + n + m] if grad_k else None, views[:S], views[S:S + n], views[S + n:S + n + m],
                None, None, None, None, None, None, None)

    op.register_autograd(backward, setup_context=setup_context)
    return op


_loss_op = _register_loss_op("sfm_learner_loss", False)
_loss_k_op = _register_loss_op("sfm_learner_loss_k", True)


class _LossFunction(torch.autograd.Function):
    """The eager form of sfmwarp::sfm_learner_loss + its autograd: the same launches (_run_loss, sfm_scale_arrays), without the
    generic argument handling of a Python custom operator (its per-call host cost exceeds a whole step at the reference's batch).
    torch.compile traces the custom operator instead (sfm_learner_loss)."""

    @staticmethod
    def forward(ctx, tgt, src, K, cfg, grad, grad_k, S, n, *arrays):
        disps, poses, masks = list(arrays[:S]), list(arrays[S:S + n]), list(arrays[S + n:])
        loss5, unit = _run_loss(tgt, src, K, disps, poses, masks, cfg, grad, grad_k)
        terms = loss5[1:]
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)              # (no zero-filled gradient for `terms`: one fill kernel less per step)
        ctx.save_for_backward(unit)                   # (freed by a backward without retain_graph, like any saved tensor)
        ctx.grad, ctx.grad_k = grad, grad and grad_k
        ctx.spans, _, ctx.shapes = _grad_spans(disps, poses, masks, K if ctx.grad_k else None)
        return loss5[0], terms

    @staticmethod
    def backward(ctx, g_total, g_terms):
        (unit,) = ctx.saved_tensors
        if g_total is None or not ctx.grad:     # (not ctx.grad: only an image or the intrinsics required a gradient)
            return (None,) * (8 + len(ctx.shapes) - ctx.grad_k)
        views = _views(_scaled(unit, ctx.spans, _gy(g_total.to(torch.float32))), ctx.spans, ctx.shapes)
        if ctx.grad_k:          # (the last span: d_intrinsics, scaled in the same launch as the others)
            return (None, None, views[-1]) + (None,) * 5 + tuple(views[:-1])
        return (None,) * 8 + tuple(views)


def _dev_float(t, name, ndim=None):
    """A differentiable network output: float32, bfloat16 or float16 on a ROCm device -> float32, contiguous (casts and copies are
    recorded by autograd, so the gradient returns in the input's dtype and layout)."""
    t = ops._dev(t, name, ndim, ops.FLOATS)
    return t if t.dtype == torch.float32 else t.to(torch.float32)


_EULER = ("euler", None, None)


def _pose_conv_args(src_imgs, pose_format, invert, depth_range):
    """The three convention arguments of the warps, checked before any array is: -> (pose_format, invert as a tuple of bools or None,
    (disp_scale, disp_shift) or None), what ops.warp_*'s keyword arguments of the same meaning take.  depth_range = (min_depth,
    max_depth) is Monodepth2's disp_to_depth: depth = 1 / (1/max_depth + (1/min_depth - 1/max_depth) * disp)."""
    if pose_format == "euler" and invert is None and depth_range is None:      # the existing call: nothing to look at
        return _EULER
    fmt = _lib.pose_format_id(pose_format)
    if invert is not None:
        if isinstance(invert, (bool, int, float, torch.Tensor)) or not all(isinstance(v, (bool, int)) and v in (0, 1) for v in invert):
            raise ValueError("invert must be None or a sequence of one boolean per source, got %r" % (invert,))
        invert = tuple(bool(v) for v in invert)
        n_src = src_imgs.shape[1] if isinstance(src_imgs, torch.Tensor) and src_imgs.dim() == 5 else None
        if n_src is not None and len(invert) != n_src:
            raise ValueError("invert needs one boolean per source (%d), got %d" % (n_src, len(invert)))
        if fmt == _lib.POSE_MATRIX and any(invert):
            raise ValueError("invert with pose_format='matrix': a general 3x4 has no R^T inverse -- invert the matrices before the call "
                             "(pose_matrix(..., invert=True) does it for a rigid one)")
    affine = None
    if depth_range is not None:
        try:
            lo, hi = (float(v) for v in depth_range)
        except (TypeError, ValueError):
            raise ValueError("depth_range must be None or (min_depth, max_depth), got %r" % (depth_range,)) from None
        if not (0.0 < lo < hi < float("inf")):
            raise ValueError("depth_range needs 0 < min_depth < max_depth, both finite, got %r" % (depth_range,))
        affine = (1.0 / lo - 1.0 / hi, 1.0 / hi)
    return pose_format, invert, affine


def _pose_kw(pc):
    return dict(pose_format=pc[0], invert=pc[1], depth_affine=pc[2])


def _pose_matrices(pred_poses, B, n_src):
    """pose_format="matrix": a list of n_src (B,3,4) or (B,4,4) tensors, or one (B,n_src,3,4) / (B,n_src,4,4) tensor -> n_src contiguous
    float32 (B,3,4) arrays, rows 0..2 of each (the slice and the cast are recorded by autograd: the gradient returns in the input's
    shape and dtype, a fourth row's is 0)."""
    if isinstance(pred_poses, torch.Tensor):
        t = _dev_float(pred_poses, "pred_poses", 4)
        if tuple(t.shape) not in ((B, n_src, 3, 4), (B, n_src, 4, 4)):
            raise TypeError("pred_poses: expected (B,n_src,3,4) or (B,n_src,4,4) with B, n_src = %d, %d, got %s" % (B, n_src, tuple(t.shape)))
        return [t[:, i, :3].contiguous() for i in range(n_src)]
    poses = list(pred_poses)
    if len(poses) != n_src:
        raise TypeError("src_imgs has %d sources but %d poses were given" % (n_src, len(poses)))
    out = []
    for i, t in enumerate(poses):
        t = _dev_float(t, "pred_poses[%d]" % i, 3)
        if tuple(t.shape) not in ((B, 3, 4), (B, 4, 4)):
            raise TypeError("pred_poses[%d] must be (B,3,4) or (B,4,4) with B = %d, got %s" % (i, B, tuple(t.shape)))
        out.append(t[:, :3].contiguous())
    return out


def _poses(pred_poses, B, n_src, pose_format="euler"):
    """A list of n_src (B,6) tensors (contiguous or not, e.g. h.split(6, 1)) or PoseNet's packed (B,6*n_src) output ->
    n_src contiguous float32 (B,6) arrays.  pose_format="matrix": `_pose_matrices`."""
    if pose_format == "matrix":
        return _pose_matrices(pred_poses, B, n_src)
    if isinstance(pred_poses, torch.Tensor):
        packed = _dev_float(pred_poses, "pred_poses", 2)
        if tuple(packed.shape) != (B, 6 * n_src):
            raise TypeError("pred_poses: expected (B,6*n_src) = (%d,%d), got %s" % (B, 6 * n_src, tuple(packed.shape)))
        return list(packed.view(B, n_src, 6).transpose(0, 1).contiguous().unbind(0))
    poses = list(pred_poses)
    if len(poses) != n_src:
        raise TypeError("src_imgs has %d sources but %d poses were given" % (n_src, len(poses)))
    out = []
    for i, t in enumerate(poses):
        t = _dev_float(t, "pred_poses[%d]" % i, 2)
        if tuple(t.shape) != (B, 6):
            raise TypeError("pred_poses[%d] must be (B,6) = (%d,6), got %s" % (i, B, tuple(t.shape)))
        out.append(t)
    return out


def _masks(pred_maskes, B, n_src, H, W, S):
    """The explainability logits of a loss with exp_reg > 0: S arrays (B,n_src,H>>s,W>>s) -> float32, contiguous"""
    if pred_maskes is None or len(pred_maskes) != S:
        raise ValueError("exp_reg > 0 needs the explainability logits (pred_maskes), one per scale")
    masks = []
    for s, t in enumerate(pred_maskes):
        t = _dev_float(t, "pred_maskes[%d]" % s, 4)
        if tuple(t.shape) != (B, n_src, H >> s, W >> s):
            raise TypeError("pred_maskes[%d] must be (B,n_src,H>>%d,W>>%d), got %s" % (s, s, s, tuple(t.shape)))
        masks.append(t)
    return masks


def _step_inputs(src_imgs, intrinsics, pred_disps, pred_poses, tgt=None, exp_reg=0.0, pred_maskes=None, pose_format="euler"):
    """The inputs of `sfm_learner_loss` (which passes `tgt`, its checked target frames) and of `warp_pyramid` (which does not, and
    takes the intrinsics as constants), checked in the one order both have: src_imgs (B,n_src,3,H,W) -- with `tgt`, that it is
    (B,3,H,W) too --, 1..8 sources, 1..8 scales, intrinsics (B,S,3,3), pred_disps[s] (B,1,H>>s,W>>s), the poses, with exp_reg > 0
    the masks, and last that every array lives on the frames' device.  -> (src, K, disps, poses, masks)"""
    src = ops._dev(src_imgs, "src_imgs", 5)
    B, n_src, c, H, W = src.shape
    if tgt is None:
        if c != 3:
            raise TypeError("src_imgs must be (B,n_src,3,H,W), got %s" % (tuple(src.shape),))
    elif tuple(tgt.shape) != (B, 3, H, W) or c != 3:
        raise TypeError("tgt_img must be (B,3,H,W) and src_imgs (B,n_src,3,H,W), got %s and %s" % (tuple(tgt.shape), tuple(src.shape)))
    if not 1 <= n_src <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d source images, got %d" % (_lib.SFM_MAX_SRC, n_src))
    S = len(pred_disps)
    if not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("1..%d scales, got %d" % (_lib.SFM_MAX_SCALES, S))
    K = ops._dev(intrinsics, "intrinsics", 4)
    if tuple(K.shape) != (B, S, 3, 3):
        raise TypeError("intrinsics must be (B,%d,3,3), got %s" % (S, tuple(K.shape)))
    if tgt is None and K.requires_grad:
        raise TypeError("warp_pyramid does not differentiate the intrinsics: detach them, or warp per (scale, source) with "
                        "projective_inverse_warp, which returns their gradient")
    disps = []
    for s, t in enumerate(pred_disps):
        t = _dev_float(t, "pred_disps[%d]" % s, 4)
        if tuple(t.shape) != (B, 1, H >> s, W >> s):
            raise TypeError("pred_disps[%d] must be (B,1,H>>%d,W>>%d) = %s, got %s" % (s, s, s, (B, 1, H >> s, W >> s), tuple(t.shape)))
        disps.append(t)
    poses = _poses(pred_poses, B, n_src, pose_format)
    masks = _masks(pred_maskes, B, n_src, H, W, S) if exp_reg > 0 else []
    dev = src.device if tgt is None else tgt.device
    for t in [K] + disps + poses + masks:
        if t.device != dev:
            raise TypeError("every array must live on %s, one is on %s" % (dev, t.device))
    return src, K, disps, poses, masks


def sfm_learner_loss(tgt_img, src_imgs, intrinsics, pred_disps, pred_poses, pred_maskes=None, *, smooth_reg, exp_reg=0.,
                     ssim_rate=0., smooth_mode="second_order", projection="fast", norm_batch=None):
    """The loss of SFMLearner.__call__ (models/base_model.py:48-124) with torch.autograd gradients.

    tgt_img (B,3,H,W) and src_imgs (B,n_src,3,H,W): float32 images -- constants, as the reference's `.data` makes them (:71-72): no
      gradient flows to them.
    intrinsics (B,S,3,3) float32: any invertible 3x3 per (sample, scale).  When it requires grad (a learned calibration, e.g. a
      (B,4) focal / centre parameter through `multi_scale_intrinsics`) it receives its gradient WITH the predictions': one more small
      launch (sfm_loss_proj_bwd) behind the fused one, scaled by the upstream gradient in the same launch as the others.  With every
      prediction detached no gradient launch runs and the intrinsics get none either.
    pred_disps: S tensors (B,1,H>>s,W>>s); pred_poses: n_src tensors (B,6) (views such as h.split(6, 1) are fine) or one packed
      (B,6*n_src) tensor; pred_maskes: S explainability logits (B,n_src,H>>s,W>>s), needed iff exp_reg > 0.  Float32, bfloat16 or
      float16 (autocast) on a ROCm device: computed in float32, each gradient returned in its input's dtype.
    smooth_mode: "second_order" (the reference's live form), "edge_aware" or "none"; projection: "fast" or "reference_order"
      (include/sfmwarp.h); norm_batch: the global batch when this call holds a shard of it.

    Returns (total_loss, terms): total_loss a 0-d tensor; terms = (pixel, smooth, exp, ssim), shape (4,).  The fused kernel
    produces the gradient of total_loss only: `terms` is NOT differentiable (report it, do not backpropagate through it).

    With grad mode on and any prediction requiring grad, ONE fused launch computes the loss and its gradients for gy = 1; backward
    scales them by the upstream gradient on the device (so loss scaling, GradScaler and graph capture work, and no call syncs).
    Gradients are per call: several forwards before one backward each keep their own."""
    smooth_mode, projection = _lib.smooth_mode_id(smooth_mode), _lib.projection_id(projection)
    tgt = ops._dev(tgt_img, "tgt_img", 4)
    exp_reg = float(exp_reg or 0.0)
    src, K, disps, poses, masks = _step_inputs(src_imgs, intrinsics, pred_disps, pred_poses, tgt, exp_reg, pred_maskes)
    B, n_src, _, H, W = src.shape
    S = len(disps)
    grad = torch.is_grad_enabled() and any(t.requires_grad for t in disps + poses + masks)
    grad_k = grad and K.requires_grad
    cfg = (float(smooth_reg or 0.0), exp_reg, float(ssim_rate or 0.0), smooth_mode, projection,
           int(norm_batch if norm_batch is not None else B))
    stacked = src.view(B, 3 * n_src, H, W)
    if torch.compiler.is_compiling():
        op = torch.ops.sfmwarp.sfm_learner_loss_k if grad_k else torch.ops.sfmwarp.sfm_learner_loss
        total, terms, _ = op(tgt, stacked, K, disps, poses, masks, *cfg, grad)
        return total, terms
    return _LossFunction.apply(tgt, stacked, K, cfg, grad, grad_k, S, n_src, *disps, *poses, *masks)


class SFMLearnerLoss(torch.nn.Module):
    """The loss half of the reference's SFMLearner link (models/base_model.py:28-124) as a torch.nn.Module: the constructor takes
    the reference's config keys (smooth_reg, exp_reg, ssim_rate, seq_len), forward() the arguments of links.SFMLearnerLoss and
    returns the total loss (0-d, differentiable).  `last_report` holds the five reported scalars of the latest call
    (total_loss, pixel_loss, smooth_loss, exp_loss, ssim_loss: 0-d device tensors -- reading the dict does not sync)."""

    def __init__(self, config, smooth_mode="second_order", projection="fast"):
        super().__init__()
        self.n_sources = config['seq_len'] - 1
        self.smooth_reg = config['smooth_reg']
        self.exp_reg = config['exp_reg']
        self.ssim_rate = config['ssim_rate'] if 'ssim_rate' in config else 0.0     # models/base_model.py:24-25, 39
        self.smooth_mode = smooth_mode
        self.projection = projection
        self._last = None

    def forward(self, tgt_img, src_imgs, intrinsics, inv_intrinsics, pred_disps, pred_poses, pred_maskes=None, norm_batch=None):
        """inv_intrinsics is unused, as in the reference (base_model.py:48)."""
        if isinstance(src_imgs, torch.Tensor) and src_imgs.dim() == 5 and src_imgs.shape[1] != self.n_sources:
            raise TypeError("src_imgs has %d sources, the config's seq_len says %d" % (src_imgs.shape[1], self.n_sources))
        total, terms = sfm_learner_loss(tgt_img, src_imgs, intrinsics, pred_disps, pred_poses, pred_maskes,
                                        smooth_reg=self.smooth_reg, exp_reg=self.exp_reg, ssim_rate=self.ssim_rate,
                                        smooth_mode=self.smooth_mode, projection=self.projection, norm_batch=norm_batch)
        self._last = (total.detach(), terms)
        return total

    @property
    def last_report(self):
        """{'total_loss', 'pixel_loss', 'smooth_loss', 'exp_loss', 'ssim_loss'} of the latest call (models/base_model.py:119-123):
        0-d device tensors, None before the first call."""
        if self._last is None:
            return None
        total, terms = self._last
        return dict(zip(("total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss"), (total,) + tuple(terms.unbind(0))))


# ---------------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------------
class _Warp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, imgs, depthes, poses, K):
        ctx.save_for_backward(imgs, depthes, poses, K)
        return ops.warp_fwd(imgs, depthes, poses, K)

    @staticmethod
    def backward(ctx, g):
        imgs, depthes, poses, K = ctx.saved_tensors
        g = g.contiguous()
        d_depth, d_pose, d_src = ops.warp_bwd(imgs, depthes, poses, K, g, want_d_src=ctx.needs_input_grad[0])
        d_K = ops.warp_bwd_intrinsics(imgs, depthes, poses, K, g) if ctx.needs_input_grad[3] else None
        return d_src, d_depth.view(depthes.shape), d_pose, d_K


def projective_inverse_warp(imgs, depthes, poses, K):
    """models/transform.py:156-193: imgs (N,C,H,W), depthes (N,3,H*W) or (N,H*W), poses (N,6), K (N,3,3), float32 on a ROCm
    device -> the warped images (N,C,H,W).  Gradients flow to imgs, depthes and poses (ops.warp_bwd) and, when it requires one, to K
    (ops.warp_bwd_intrinsics: one more pass over the pixels)."""
    return _Warp.apply(imgs, depthes, poses, K)


class _PoseMatrix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose, fmt, invert):
        ctx.save_for_backward(pose)
        ctx.conv = (fmt, invert)
        return ops.pose_mat_fwd(pose, fmt, invert)

    @staticmethod
    def backward(ctx, g):
        pose, = ctx.saved_tensors
        return ops.pose_mat_bwd(pose, *ctx.conv, g.to(torch.float32).contiguous()), None, None


def pose_matrix(pose, *, pose_format="axis_angle", invert=False):
    """pose (B,6) -> the rigid transform T (B,3,4) = [R|t] as ONE differentiable node (ops.pose_mat_fwd / ops.pose_mat_bwd):
    pose_format="axis_angle": (ax, ay, az, tx, ty, tz), R Monodepth2's rot_from_axisangle (any finite angle); "euler": the reference's
    euler2mat / pose_vec2mat.  invert=True returns [R^T | -R^T t], Monodepth2's transformation_from_parameters(..., invert=True).
    float32, bfloat16 or float16 on a ROCm device, computed in float32, the gradient returned in the input's dtype.

    What it is for: build every source's matrix your own way -- a pose head per source, a fixed stereo baseline, the product of two
    poses (append the row (0,0,0,1) and matmul) -- and hand the result to `warp_pyramid`, `warp_full_res` or
    `min_reprojection_loss` with pose_format="matrix"."""
    if _lib.pose_format_id(pose_format) == _lib.POSE_MATRIX:
        raise ValueError("pose_format must be 'euler' or 'axis_angle': a matrix is what pose_matrix returns")
    if not isinstance(invert, (bool, int)) or invert not in (0, 1):
        raise ValueError("invert must be a boolean, got %r" % (invert,))
    pose = _dev_float(pose, "pose", 2)
    if pose.shape[1] != 6:
        raise TypeError("pose must be (B,6), got %s" % (tuple(pose.shape),))
    return _PoseMatrix.apply(pose, pose_format, bool(invert))


class _WarpPyramid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, K, S, want_valid, pc, *arrays):
        disps, poses = list(arrays[:S]), list(arrays[S:])
        pyr = ops.pyramid_hwc(src, S)
        out = ops.warp_pyramid_fwd(pyr, disps, poses, K, "hwc", want_valid, **_pose_kw(pc))
        warped, valid = out if want_valid else (out, [])
        ctx.save_for_backward(K, *pyr, *disps, *poses)
        ctx.S, ctx.pc = S, pc
        ctx.mark_non_differentiable(*valid)
        ctx.set_materialize_grads(False)              # (a scale the caller's loss does not use: one zero fill here, not one per output)
        return tuple(warped) + tuple(valid)

    @staticmethod
    def backward(ctx, *grads):
        S = ctx.S
        K, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        pyr, disps, poses = list(saved[:S]), list(saved[S:2 * S]), list(saved[2 * S:])
        B, n_src = pyr[0].shape[:2]
        g = [torch.zeros((B, n_src, 3) + tuple(d.shape[2:]), dtype=torch.float32, device=d.device) if gr is None
             else gr.to(torch.float32).contiguous() for gr, d in zip(grads[:S], disps)]
        d_disps, d_poses = ops.warp_pyramid_bwd(pyr, disps, poses, K, "hwc", g, **_pose_kw(ctx.pc))
        return (None, None, None, None, None) + tuple(d_disps) + tuple(d_poses)


def warp_pyramid(src_imgs, intrinsics, pred_disps, pred_poses, *, return_valid=False, pose_format="euler", invert=None, depth_range=None):
    """The warped source images of every scale and every source of a step -- curr_proj_img of models/base_model.py:90-94 for all s
    and i -- as differentiable tensors, for a loss of your own on them (a per-pixel minimum over the sources, auto-masking, a
    robust penalty, a feature loss).  The inputs are those of `sfm_learner_loss`:

    src_imgs (B,n_src,3,H,W) float32: constants, as in the loss -- no gradient flows to them;
    intrinsics (B,S,3,3) float32, any invertible 3x3 per (sample, scale): a constant HERE -- if it requires grad this raises
      TypeError: `projective_inverse_warp`, per (scale, source), is the route that differentiates K;
    pred_disps: S tensors (B,1,H>>s,W>>s); pred_poses: n_src tensors (B,6) or one packed (B,6*n_src) tensor; float32, bfloat16 or
      float16 on a ROCm device, computed in float32, each gradient returned in its input's dtype.

    Returns a list of S tensors (B,n_src,3,H>>s,W>>s): [s][:, i] is projective_inverse_warp of source i at scale s with depth
    1 / disp (bit for bit), exactly 0 where the sample is not in view.  With `return_valid` also the list of S masks (B,n_src,H>>s,W>>s),
    1.0 where the sample passes both strict tests of models/transform.py:129, else 0.0 (not differentiable).

    Two launches forward (the source pyramid, the warp of all scales and sources); backward one launch over the pixels plus a small
    fold, whatever S and n_src are.  Nothing reads a device value on the host: it runs under torch.cuda.graph capture.

    pose_format, invert and depth_range select the pose and depth conventions inside the same launches (include/sfmwarp_pose.h):
    pose_format="axis_angle": pred_poses[i] = (ax, ay, az, tx, ty, tz), R Monodepth2's rot_from_axisangle; "matrix": pred_poses is a
      list of n_src (B,3,4) or (B,4,4) tensors (rows 0..2 are used) or one (B,n_src,3,4) / (B,n_src,4,4) tensor, any 3x4, and the
      gradient is that of the matrix, in the input's shape (`pose_matrix` builds one from a 6-vector, differentiably);
    invert: None or n_src booleans -- source i is warped through [R^T | -R^T t], Monodepth2's invert=True (a ValueError with "matrix");
    depth_range=(min_depth, max_depth): depth = 1 / (1/max_depth + (1/min_depth - 1/max_depth) * disp), Monodepth2's disp_to_depth,
      instead of 1 / disp.
    With the three at their defaults the call is what it was, bit for bit."""
    pc = _pose_conv_args(src_imgs, pose_format, invert, depth_range)
    src, K, disps, poses, _ = _step_inputs(src_imgs, intrinsics, pred_disps, pred_poses, pose_format=pose_format)
    B, n_src, _, H, W = src.shape
    S = len(disps)
    out = _WarpPyramid.apply(src.view(B, 3 * n_src, H, W), K, S, bool(return_valid), pc, *disps, *poses)
    return (list(out[:S]), list(out[S:])) if return_valid else list(out)


class _DepthConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K, S, want_valid, want_depths, pc, *arrays):
        disps, src_disps, poses = list(arrays[:S]), list(arrays[S:2 * S]), list(arrays[2 * S:])
        out = ops.depth_consistency_fwd(disps, src_disps, poses, K, want_valid, want_depths, **_pose_kw(pc))
        out = (out,) if not (want_valid or want_depths) else out
        ctx.save_for_backward(K, *disps, *src_disps, *poses)
        ctx.S, ctx.pc = S, pc
        flat = tuple(t for group in out for t in group)
        ctx.mark_non_differentiable(*flat[S:])
        ctx.set_materialize_grads(False)              # (a scale the caller's loss does not use: one zero fill here, not one per output)
        return flat

    @staticmethod
    def backward(ctx, *grads):
        S = ctx.S
        K, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        disps, src_disps, poses = list(saved[:S]), list(saved[S:2 * S]), list(saved[2 * S:])
        g = [torch.zeros_like(sd) if gr is None else gr.to(torch.float32).contiguous() for gr, sd in zip(grads[:S], src_disps)]
        want = any(ctx.needs_input_grad[5 + S:5 + 2 * S])      # src_disps that do not require grad: the kernel without the scatter
        d_disps, d_poses, d_src = ops.depth_consistency_bwd(disps, src_disps, poses, K, g, want_d_src_disp=want, **_pose_kw(ctx.pc))
        return (None,) * 5 + tuple(d_disps) + (tuple(d_src) if want else (None,) * S) + tuple(d_poses)


def depth_consistency(pred_disps, src_disps, intrinsics, pred_poses, *, return_valid=False, return_depths=False, pose_format="euler",
                      invert=None, depth_range=None):
    """The geometry-consistency term of SC-SfMLearner (Bian et al., NeurIPS 2019: inverse_warp2 and compute_pairwise_loss) for every
    scale and source of a step, as ONE autograd node on this library's warp:

      diff = |computed - projected| / (computed + projected)

    where computed is the depth of the target pixel's 3-D point seen from the source camera (clamped at 1e-3) and projected the
    source frame's own predicted depth, sampled bilinearly where that point lands -- at the positions of `warp_pyramid` with the same
    arguments, bit for bit.  A pixel whose sample is not in view gets exactly 0.

    pred_disps: S tensors (B,1,h_s,w_s), the target frame's disparities (any sizes of at least 3x3 per scale);
    src_disps: S tensors (B,n_src,h_s,w_s), the disparity the SAME network predicts for each source frame;
    intrinsics (B,S,3,3) float32: a constant -- if it requires grad this raises TypeError, as in `warp_pyramid`;
    pred_poses: n_src tensors (B,6) or one packed (B,6*n_src) tensor.  Predictions are float32, bfloat16 or float16 on a ROCm
      device, computed in float32, each gradient returned in its input's dtype.  Gradients flow to pred_disps, src_disps and
      pred_poses; src_disps that do not require grad (detached, or under no_grad) skip the scatter that forms their gradient.

    Returns the list of S tensors diff_s (B,n_src,h_s,w_s), each in [0, 1) for positive disparities.  With `return_valid` also the S
    masks (1.0 where the sample passes both strict in-view tests, else 0.0), with `return_depths` also the S computed and the S
    projected depths: (diff, valid, computed, projected) without the lists not asked for; only diff is differentiable.

    It adds no reduction.  SC-SfMLearner's geometry loss and its self-discovered mask are `pairwise_mean` on the result (and the
    whole objective `sc_sfm_loss`), or two aten lines:
      geometry = sum((d * v).sum() / v.sum().clamp(min=1) for d, v in zip(diff, valid))
      weighted = [err_s * (1 - d) for err_s, d in zip(photometric_error_maps, diff)]

    One launch forward; backward one launch over the pixels plus a small fold, whatever S and n_src are.  Nothing reads a device
    value on the host: it runs under torch.cuda.graph capture.  pose_format, invert and depth_range are those of `warp_pyramid`;
    depth_range acts on both disparities."""
    pc = _pose_conv_args(None, pose_format, invert, depth_range)
    if isinstance(pred_disps, torch.Tensor) or isinstance(src_disps, torch.Tensor):
        raise TypeError("pred_disps and src_disps are lists with one tensor per scale")
    S = len(pred_disps)
    if not 1 <= S <= _lib.SFM_MAX_SCALES or len(src_disps) != S:
        raise TypeError("1..%d scales, and as many src_disps as pred_disps: got %d and %d" % (_lib.SFM_MAX_SCALES, S, len(src_disps)))
    disps = [_dev_float(t, "pred_disps[%d]" % s, 4) for s, t in enumerate(pred_disps)]
    srcs = [_dev_float(t, "src_disps[%d]" % s, 4) for s, t in enumerate(src_disps)]
    B, n_src = srcs[0].shape[:2]
    if not 1 <= n_src <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d sources, got %d" % (_lib.SFM_MAX_SRC, n_src))
    if pc[1] is not None and len(pc[1]) != n_src:
        raise ValueError("invert needs one boolean per source (%d), got %d" % (n_src, len(pc[1])))
    for s, (t, u) in enumerate(zip(disps, srcs)):
        h, w = t.shape[2:]
        if tuple(t.shape) != (B, 1, h, w) or tuple(u.shape) != (B, n_src, h, w):
            raise TypeError("scale %d: pred_disps must be (B,1,h,w) and src_disps (B,n_src,h,w) = %s, got %s and %s"
                            % (s, (B, n_src, h, w), tuple(t.shape), tuple(u.shape)))
    K = ops._dev(intrinsics, "intrinsics", 4)
    if tuple(K.shape) != (B, S, 3, 3):
        raise TypeError("intrinsics must be (B,%d,3,3), got %s" % (S, tuple(K.shape)))
    if K.requires_grad:
        raise TypeError("depth_consistency does not differentiate the intrinsics: detach them")
    poses = _poses(pred_poses, B, n_src, pose_format)
    for t in [K] + srcs + poses:
        if t.device != disps[0].device:
            raise TypeError("every array must live on %s, one is on %s" % (disps[0].device, t.device))
    out = _DepthConsistency.apply(K, S, bool(return_valid), bool(return_depths), pc, *disps, *srcs, *poses)
    groups = [list(out[k:k + S]) for k in range(0, len(out), S)]
    return tuple(groups) if len(groups) > 1 else groups[0]


class _WarpFullRes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, K, S, want_valid, upsample, pc, *arrays):
        disps, poses = list(arrays[:S]), list(arrays[S:])
        hwc = ops.pyramid_hwc(src, 1)[0]
        out = ops.warp_full_res_fwd(hwc, disps, poses, K, "hwc", want_valid, upsample=upsample, **_pose_kw(pc))
        warped, valid = out if want_valid else (out, [])
        ctx.save_for_backward(K, hwc, *disps, *poses)
        ctx.S, ctx.upsample, ctx.pc = S, upsample, pc
        ctx.mark_non_differentiable(*valid)
        ctx.set_materialize_grads(False)              # (a scale the caller's loss does not use: one zero fill here, not one per output)
        return tuple(warped) + tuple(valid)

    @staticmethod
    def backward(ctx, *grads):
        S = ctx.S
        K, hwc, saved = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:]
        disps, poses = list(saved[:S]), list(saved[S:])
        B, n_src, H, W = hwc.shape[:4]
        g = [torch.zeros((B, n_src, 3, H, W), dtype=torch.float32, device=hwc.device) if gr is None
             else gr.to(torch.float32).contiguous() for gr in grads[:S]]
        d_disps, d_poses = ops.warp_full_res_bwd(hwc, disps, poses, K, "hwc", g, upsample=ctx.upsample, **_pose_kw(ctx.pc))
        return (None, None, None, None, None, None) + tuple(d_disps) + tuple(d_poses)


def _full_res_inputs(src_imgs, intrinsics, pred_disps, pred_poses, who, pose_format="euler"):
    """The inputs of `warp_full_res`, checked: src_imgs (B,n_src,3,H,W), 1..8 sources, 1..8 scales, intrinsics (B,3,3) or (B,S,3,3)
    -- of which [:, 0], the full-resolution camera, is used --, a constant, pred_disps[s] (B,1,h_s,w_s) of any size, the poses, and
    last that every array lives on the frames' device.  -> (src, K (B,3,3), disps, poses)"""
    src = ops._dev(src_imgs, "src_imgs", 5)
    B, n_src, c, H, W = src.shape
    if c != 3:
        raise TypeError("src_imgs must be (B,n_src,3,H,W), got %s" % (tuple(src.shape),))
    if not 1 <= n_src <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d source images, got %d" % (_lib.SFM_MAX_SRC, n_src))
    if not isinstance(pred_disps, (list, tuple)) or not 1 <= len(pred_disps) <= _lib.SFM_MAX_SCALES:
        raise TypeError("pred_disps: a list of 1..%d tensors (B,1,h,w)" % _lib.SFM_MAX_SCALES)
    S = len(pred_disps)
    K = ops._dev(intrinsics, "intrinsics")
    if K.requires_grad:
        raise TypeError("%s does not differentiate the intrinsics: detach them, or warp per (scale, source) with "
                        "projective_inverse_warp, which returns their gradient" % who)
    if tuple(K.shape) == (B, S, 3, 3):
        K = K[:, 0].contiguous()
    elif tuple(K.shape) != (B, 3, 3):
        raise TypeError("intrinsics must be (B,3,3) or (B,%d,3,3), got %s" % (S, tuple(K.shape)))
    disps = []
    for s, t in enumerate(pred_disps):
        t = _dev_float(t, "pred_disps[%d]" % s, 4)
        if tuple(t.shape[:2]) != (B, 1):
            raise TypeError("pred_disps[%d] must be (B,1,h,w) = (%d,1,h,w), got %s" % (s, B, tuple(t.shape)))
        disps.append(t)
    poses = _poses(pred_poses, B, n_src, pose_format)
    for t in [K] + disps + poses:
        if t.device != src.device:
            raise TypeError("every array must live on %s, one is on %s" % (src.device, t.device))
    return src, K, disps, poses


def warp_full_res(src_imgs, intrinsics, pred_disps, pred_poses, *, return_valid=False, upsample="align_corners", pose_format="euler",
                  invert=None, depth_range=None):
    """Monodepth2's "full-resolution multi-scale" warp: the disparity of every scale upsampled to the input resolution and the
    FULL-RESOLUTION sources warped with it through the full-resolution camera -- what `resize_images` per scale followed by
    `projective_inverse_warp` per (scale, source) computes, in one launch and without a full-resolution copy of any disparity.

    src_imgs (B,n_src,3,H,W) float32: constants -- no gradient flows to them;
    intrinsics (B,3,3) float32, the full-resolution camera, or the (B,S,3,3) `sfm_learner_loss` takes, of which [:, 0] is used: a
      constant -- if it requires grad this raises TypeError;
    pred_disps: S tensors (B,1,h_s,w_s) of ANY sizes (a scale of size (H, W) is used as it is, every other one is resampled as
      `resize_images` does: align-corners bilinear, the reference's F.resize_images); pred_poses: n_src tensors (B,6) or one packed
      (B,6*n_src) tensor; float32, bfloat16 or float16 on a ROCm device, computed in float32, each gradient returned in its input's dtype.

    Returns a list of S tensors (B,n_src,3,H,W): [s][:, i] is projective_inverse_warp of source i with depth 1 / resize_images(
    pred_disps[s], (H, W)), bit for bit.  With `return_valid` also the list of S masks (B,n_src,H,W), as `warp_pyramid` returns them.

    Two launches forward (the pixel-interleaved copy of the sources, the warp of all scales and sources); backward one launch over
    the pixels, one that gathers the gradient of every low-resolution disparity and a small fold, whatever S and n_src are.  No
    atomics: the same bits on every call.  Nothing reads a device value on the host: it runs under torch.cuda.graph capture.

    upsample="half_pixel" is Monodepth2's own upsampling instead: every resampled disparity is F.interpolate(pred_disps[s], (H, W),
    mode="bilinear", align_corners=False) -- half-pixel centres -- formed inside the same launch, its gradient the adjoint of that map
    in the same gather launch.  The launches, the workspace and the determinism are those of the default; any other name is a ValueError.

    pose_format, invert, depth_range: as in `warp_pyramid`; the depth map acts on the UPSAMPLED disparity, as Monodepth2's
    disp_to_depth(F.interpolate(disp, ...)) does."""
    _lib.upsample_id(upsample)
    pc = _pose_conv_args(src_imgs, pose_format, invert, depth_range)
    src, K, disps, poses = _full_res_inputs(src_imgs, intrinsics, pred_disps, pred_poses, "warp_full_res", pose_format)
    B, n_src, _, H, W = src.shape
    S = len(disps)
    out = _WarpFullRes.apply(src.detach().view(B, 3 * n_src, H, W), K, S, bool(return_valid), upsample, pc, *disps, *poses)
    return (list(out[:S]), list(out[S:])) if return_valid else list(out)


class _PhotoError(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ssim_rate, padding, S, *arrays):
        imgs, tgts = list(arrays[:S]), list(arrays[S:])
        err = ops.photo_error_fwd(imgs, tgts, ssim_rate, padding)
        ctx.save_for_backward(*imgs, *tgts)
        ctx.S, ctx.ssim_rate, ctx.padding = S, ssim_rate, padding
        ctx.set_materialize_grads(False)              # (a scale the caller's loss does not use: one zero fill here, not one per output)
        return tuple(err)

    @staticmethod
    def backward(ctx, *grads):
        S = ctx.S
        imgs, tgts = list(ctx.saved_tensors[:S]), list(ctx.saved_tensors[S:])
        g = [torch.zeros(x.shape[:2] + x.shape[3:], dtype=torch.float32, device=x.device) if gr is None
             else gr.to(torch.float32).contiguous() for gr, x in zip(grads, imgs)]
        d_imgs = ops.photo_error_bwd(imgs, tgts, ctx.ssim_rate, g, ctx.padding)
        return (None, None, None) + tuple(d_imgs) + (None,) * S


def photometric_error(imgs, tgt, *, ssim_rate, padding="zero"):
    """The per-pixel photometric error of every (scale, image) of a step -- ssim_rate * compute_ssim + (1 - ssim_rate) * |.| of
    models/base_model.py:96,126-142 before any mean, averaged over the three channels -- as differentiable maps: the stage between
    `warp_pyramid` and a minimum over the sources, an auto-mask or a robust penalty of your own.

    imgs: a list of S tensors (B,n,3,h_s,w_s), float32, bfloat16 or float16 on a ROCm device (computed in float32, the gradient
      returned in the input's dtype): what `warp_pyramid` returns, or any such list -- the planar source pyramid viewed as
      (B,n,3,h,w) gives the identity-reprojection error that auto-masking compares with;
    tgt: the target frames (B,3,H,W) float32 -- turned into the planar pyramid of `sfm_learner_loss` (ops.pyramid), and then
      h_s, w_s must be H >> s, W >> s -- or a list of S per-scale tensors (B,3,h_s,w_s).  A constant: no gradient flows to it;
    ssim_rate: alpha in [0,1]; 0 is the mean absolute difference alone (no SSIM code runs), 1 the SSIM term alone.

    padding: "zero", the reference's SSIM window -- a zero-padded 3x3 average, divided by 9 at the border too --, or "reflect",
      Monodepth2's: the 3x3 average over the image extended by one pixel of reflection, ReflectionPad2d(1) + AvgPool2d(3, 1), so that
      every window holds nine real values (every h_s, w_s >= 2, else TypeError).  Any other name is a ValueError.

    Returns a list of S maps (B,n,h_s,w_s) in [0,1] for images in [-1,1].  Nothing is masked: the zeros of out-of-view pixels take
    part in their neighbours' windows as in the reference -- `warp_pyramid(..., return_valid=True)` has the mask.

    One launch forward and one backward, whatever S and n are (plus the pyramid launch for a single `tgt`).  The gradient goes to
    `imgs` only; if none of them requires one, nothing is recorded.  Nothing reads a device value on the host: it runs under
    torch.cuda.graph capture."""
    _lib.ssim_padding_id(padding)
    if not isinstance(imgs, (list, tuple)):
        raise TypeError("imgs must be a list of (B,n,3,h,w) tensors, one per scale")
    S = len(imgs)
    if not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("1..%d scales, got %d" % (_lib.SFM_MAX_SCALES, S))
    xs = []
    for s, t in enumerate(imgs):
        t = _dev_float(t, "imgs[%d]" % s, 5)
        if t.shape[2] != 3 or tuple(t.shape[:2]) != tuple(xs[0].shape[:2] if xs else t.shape[:2]):
            raise TypeError("imgs[%d] must be (B,n,3,h,w) with the B and n of imgs[0], got %s" % (s, tuple(t.shape)))
        xs.append(t)
    B, n = xs[0].shape[:2]
    if not 1 <= n <= _lib.SFM_MAX_SRC:
        raise TypeError("1..%d images per sample, got %d" % (_lib.SFM_MAX_SRC, n))
    if isinstance(tgt, (list, tuple)):
        if len(tgt) != S:
            raise TypeError("imgs has %d scales but tgt has %d" % (S, len(tgt)))
        tgts = ops._devs(tgt, "tgt", 4)
    else:
        tgt = ops._dev(tgt, "tgt", 4)
        H, W = tgt.shape[2:]
        for s, t in enumerate(xs):
            if tuple(t.shape[3:]) != (H >> s, W >> s):
                raise TypeError("imgs[%d] must be (B,n,3,H>>%d,W>>%d) = %s for a tgt of %s, got %s"
                                % (s, s, s, (B, n, 3, H >> s, W >> s), tuple(tgt.shape), tuple(t.shape)))
        if tuple(tgt.shape[:2]) != (B, 3):
            raise TypeError("tgt must be (B,3,H,W) = (%d,3,H,W), got %s" % (B, tuple(tgt.shape)))
        tgts = ops.pyramid(tgt.detach(), S)
    for s, (x, y) in enumerate(zip(xs, tgts)):
        if tuple(y.shape) != (B, 3) + tuple(x.shape[3:]):
            raise TypeError("tgt[%d] must be (B,3,h,w) = %s, got %s" % (s, (B, 3) + tuple(x.shape[3:]), tuple(y.shape)))
        if x.device != xs[0].device or y.device != xs[0].device:
            raise TypeError("every array must live on %s" % (xs[0].device,))
    return list(_PhotoError.apply(float(ssim_rate), padding, S, *xs, *[y.detach() for y in tgts]))


def _scale_weights(weights, S):
    """`weights` of min_reprojection / min_reprojection_loss as a tuple of S floats; None: 2**-s, the example of INTEGRATION.md"""
    if weights is None:
        return tuple(2.0 ** -s for s in range(S))
    weights = tuple(float(w) for w in weights)
    if len(weights) != S:
        raise TypeError("weights: one per scale, got %d for %d scales" % (len(weights), S))
    return weights


def _g_loss(S, g_total, g_scales, device):
    """(S+1,) float32: the upstream gradients of (per_scale, total) as sfm_min_reproj_bwd reads them; None is zero.  On the device."""
    total = torch.zeros((1,), dtype=torch.float32, device=device) if g_total is None else g_total.to(torch.float32).reshape(1)
    if g_scales is None:
        return torch.nn.functional.pad(total, (S, 0))
    return torch.cat([g_scales.to(torch.float32).reshape(S), total])


class _MinReproj(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, weights, norm, bound, has_ident, *arrays):
        errs, rest = list(arrays[:S]), list(arrays[S:])
        valids = [rest.pop(0) if on else None for on in bound]
        idents = rest if has_ident else None
        loss, count, winners = ops.min_reproj_fwd(errs, valids, idents, weights, norm)
        ctx.save_for_backward(count, *winners)
        ctx.cfg = (S, errs[0].shape[1], weights, norm, [tuple(e.shape[2:]) for e in errs], len(arrays))
        ctx.mark_non_differentiable(*winners)
        ctx.set_materialize_grads(False)
        return (loss[S], loss[:S]) + tuple(winners)

    @staticmethod
    def backward(ctx, g_total, g_scales, *_):
        S, n_err, weights, norm, hw, n_arrays = ctx.cfg
        if g_total is None and g_scales is None:
            return (None,) * (5 + n_arrays)
        count, winners = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        g_errs = ops.min_reproj_bwd(winners, count, _g_loss(S, g_total, g_scales, count.device), n_err, weights, norm, hw)
        return (None,) * 5 + tuple(g_errs) + (None,) * (n_arrays - S)


def min_reprojection(errs, *, valid=None, ident=None, weights=None, norm="kept"):
    """The last stage of a Monodepth2-style loss on the library's warp: per pixel the smallest error over the sources, the
    auto-mask against the unwarped sources and the mean, every scale in two launches (ops.min_reproj_fwd) and one backward
    (ops.min_reproj_bwd) -- what the examples of INTEGRATION.md spell as where / min / < / where / sum / sum / clamp / divide per scale.

    errs: a list of S tensors (B,n,h_s,w_s) -- what `photometric_error` returns for the list `warp_pyramid` returns; float32,
      bfloat16 or float16 on a ROCm device (computed in float32, the gradient returned in the input's dtype);
    valid: None, or a list of S entries, each (B,n,h_s,w_s) float32 or None -- `warp_pyramid(..., return_valid=True)`: a source with
      valid <= 0 at a pixel does not compete there;
    ident: None (no auto-mask) or a list of S tensors (B,m,h_s,w_s) float32, the errors of the unwarped sources: a pixel counts only
      where its smallest error is strictly below every one of them;
    weights: one per scale, default 2**-s; norm: "kept" -- each scale's mean runs over its kept pixels (at least 1) -- or "all" -- over
      all B*h*w pixels, Monodepth2's own `.mean()`.

    Returns (total, per_scale, winners): total, 0-d, = sum_s weights[s] * per_scale[s]; per_scale (S,), the mean of each scale; both
    differentiable with respect to `errs` ONLY (valid and ident are constants); winners, a list of S int8 maps (B,h_s,w_s): the source a
    kept pixel took its error from, -1 where the pixel is dropped.  A NaN or +inf error never wins.  Sums run in fp64 in a fixed
    order: the same bits on every call.  Nothing reads a device value on the host: it runs under torch.cuda.graph capture."""
    if not isinstance(errs, (list, tuple)):
        raise TypeError("errs must be a list of (B,n,h,w) tensors, one per scale")
    S = len(errs)
    if not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("1..%d scales, got %d" % (_lib.SFM_MAX_SCALES, S))
    xs = [_dev_float(t, "errs[%d]" % s, 4) for s, t in enumerate(errs)]
    valid = [None] * S if valid is None else list(valid)
    if len(valid) != S or (ident is not None and len(ident) != S):
        raise TypeError("valid and ident need one entry per scale (%d)" % S)
    bound = tuple(v is not None for v in valid)
    vs = [ops._dev(v, "valid[%d]" % s, 4).detach() for s, v in enumerate(valid) if v is not None]
    ids = [] if ident is None else [t.detach() for t in ops._devs(ident, "ident", 4)]
    out = _MinReproj.apply(S, _scale_weights(weights, S), norm, bound, ident is not None, *xs, *vs, *ids)
    return out[0], out[1], list(out[2:])


class _DispSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, weights, normalize, edge, *arrays):
        disps, tgts = list(arrays[:S]), list(arrays[S:])
        loss, stats = ops.disp_smooth_fwd(disps, tgts, weights, normalize, edge)
        ctx.save_for_backward(stats, *disps, *tgts)
        ctx.cfg = (S, weights, normalize, edge)
        ctx.set_materialize_grads(False)
        return loss[S], loss[:S]

    @staticmethod
    def backward(ctx, g_total, g_scales):
        S, weights, normalize, edge = ctx.cfg
        if g_total is None and g_scales is None:
            return (None,) * (4 + 2 * S)
        stats, disps, tgts = ctx.saved_tensors[0], list(ctx.saved_tensors[1:1 + S]), list(ctx.saved_tensors[1 + S:])
        g_disps = ops.disp_smooth_bwd(disps, tgts, stats, _g_loss(S, g_total, g_scales, stats.device), weights, normalize, edge)
        return (None,) * 4 + tuple(g_disps) + (None,) * S


def disparity_smoothness(pred_disps, tgt, *, normalize=True, edge="mean_abs", weights=None):
    """The second term of a Monodepth2-style loss: the edge-aware first-order smoothness of the disparity, every scale in two
    launches (ops.disp_smooth_fwd) and one backward (ops.disp_smooth_bwd) -- per scale
        d = disp / (disp.mean((2, 3), keepdim=True) + 1e-7)                                       (with `normalize`)
        mean(|d[..., :, 1:] - d[..., :, :-1]| * exp(-a_x)) + mean(|d[..., 1:, :] - d[..., :-1, :]| * exp(-a_y))
    with a = mean_c |dI_c| for edge "mean_abs" (Monodepth2's get_smooth_loss) or |mean_c dI_c| for "abs_mean" (compute_disp_smooth
    of models/base_model.py:144-155; with normalize=False that function exactly).

    pred_disps: a list of S tensors (B,1,h_s,w_s), float32, bfloat16 or float16 on a ROCm device (computed in float32, each
      gradient returned in its input's dtype); h_s, w_s >= 3;
    tgt: the frames whose edges relax the penalty, (B,3,H,W) float32 -- turned into the planar pyramid of `sfm_learner_loss`
      (ops.pyramid), and then h_s, w_s must be H >> s, W >> s -- or a list of S per-scale tensors (B,3,h_s,w_s).  A constant: no
      gradient flows to it;
    weights: one per scale, default 2**-s.

    Returns (total, per_scale): total, 0-d, = sum_s weights[s] * per_scale[s]; per_scale (S,).  Both are differentiable with respect
    to `pred_disps` ONLY, the path through each sample's mean included; if none of them requires a gradient, nothing is recorded.
    The mean is factored out of the sums (|D(d/M)| = |Dd| / |M|), which run in fp64 in a fixed order: the same bits on every call.
    Nothing reads a device value on the host: it runs under torch.cuda.graph capture."""
    if not isinstance(pred_disps, (list, tuple)):
        raise TypeError("pred_disps must be a list of (B,1,h,w) tensors, one per scale")
    S = len(pred_disps)
    if not 1 <= S <= _lib.SFM_MAX_SCALES:
        raise TypeError("1..%d scales, got %d" % (_lib.SFM_MAX_SCALES, S))
    _lib.disp_smooth_edge_id(edge)
    xs = []
    for s, t in enumerate(pred_disps):
        t = _dev_float(t, "pred_disps[%d]" % s, 4)
        if t.shape[1] != 1 or t.shape[0] != (xs[0].shape[0] if xs else t.shape[0]):
            raise TypeError("pred_disps[%d] must be (B,1,h,w) with the B of pred_disps[0], got %s" % (s, tuple(t.shape)))
        xs.append(t)
    B = xs[0].shape[0]
    if isinstance(tgt, (list, tuple)):
        if len(tgt) != S:
            raise TypeError("pred_disps has %d scales but tgt has %d" % (S, len(tgt)))
        tgts = ops._devs(tgt, "tgt", 4)
    else:
        tgt = ops._dev(tgt, "tgt", 4)
        H, W = tgt.shape[2:]
        for s, t in enumerate(xs):
            if tuple(t.shape[2:]) != (H >> s, W >> s):
                raise TypeError("pred_disps[%d] must be (B,1,H>>%d,W>>%d) = %s for a tgt of %s, got %s"
                                % (s, s, s, (B, 1, H >> s, W >> s), tuple(tgt.shape), tuple(t.shape)))
        if tuple(tgt.shape[:2]) != (B, 3):
            raise TypeError("tgt must be (B,3,H,W) = (%d,3,H,W), got %s" % (B, tuple(tgt.shape)))
        tgts = ops.pyramid(tgt.detach(), S)
    for s, (x, y) in enumerate(zip(xs, tgts)):
        if tuple(y.shape) != (B, 3) + tuple(x.shape[2:]):
            raise TypeError("tgt[%d] must be (B,3,h,w) = %s, got %s" % (s, (B, 3) + tuple(x.shape[2:]), tuple(y.shape)))
        if x.device != xs[0].device or y.device != xs[0].device:
            raise TypeError("every array must live on %s" % (xs[0].device,))
    return _DispSmooth.apply(S, _scale_weights(weights, S), bool(normalize), edge, *xs, *[y.detach() for y in tgts])


class _MinReprojLoss(torch.autograd.Function):
    """warp_pyramid -> photometric_error -> min_reprojection as ONE node: the six launches of the forward and the four of the
    backward run back to back from one `apply`, and autograd's engine visits one node with S + n_src leaves behind it."""

    @staticmethod
    def forward(ctx, tgt, src, K, cfg, S, *arrays):
        ssim_rate, auto_mask, weights, norm, smooth, pad, _, pc = cfg
        disps, poses = list(arrays[:S]), list(arrays[S:])
        B, n_src = src.shape[0], len(poses)
        pyr = ops.pyramid_hwc(src, S)
        warped, valid = ops.warp_pyramid_fwd(pyr, disps, poses, K, "hwc", True, **_pose_kw(pc))
        tgts = ops.pyramid(tgt, S)
        errs = ops.photo_error_fwd(warped, tgts, ssim_rate, pad)
        idents = None
        if auto_mask:     # the identity reprojection: the planar source pyramid is (B,n_src,3,h,w) byte for byte
            idents = ops.photo_error_fwd([p.view(B, n_src, 3, p.shape[2], p.shape[3]) for p in ops.pyramid(src, S)], tgts, ssim_rate, pad)
        loss, count, winners = ops.min_reproj_fwd(errs, valid, idents, weights, norm)
        if smooth is None:
            ctx.save_for_backward(K, count, *pyr, *disps, *poses, *warped, *tgts, *winners)
            ctx.cfg, ctx.pad, ctx.pc = (S, n_src, ssim_rate, weights, norm, None), pad, pc
            return loss[S]
        sm_loss, stats = ops.disp_smooth_fwd(disps, tgts, *smooth)      # on the target pyramid this node holds anyway: the RAW disparities
        ctx.save_for_backward(K, count, *pyr, *disps, *poses, *warped, *tgts, *winners, stats)
        ctx.cfg, ctx.pad, ctx.pc = (S, n_src, ssim_rate, weights, norm, smooth), pad, pc
        return loss[S] + sm_loss[S]

    @staticmethod
    def backward(ctx, g_total):
        S, n_src, ssim_rate, weights, norm, smooth = ctx.cfg
        if g_total is None:
            return (None,) * (5 + S + n_src)
        K, count, rest = ctx.saved_tensors[0], ctx.saved_tensors[1], list(ctx.saved_tensors[2:])
        pyr, disps, poses = rest[:S], rest[S:2 * S], rest[2 * S:2 * S + n_src]
        rest = rest[2 * S + n_src:]
        warped, tgts, winners = rest[:S], rest[S:2 * S], rest[2 * S:3 * S]
        g_loss = _g_loss(S, g_total, None, count.device)
        g_errs = ops.min_reproj_bwd(winners, count, g_loss, n_src, weights, norm, [tuple(t.shape[2:]) for t in disps])
        d_warped = ops.photo_error_bwd(warped, tgts, ssim_rate, g_errs, ctx.pad)
        d_disps, d_poses = ops.warp_pyramid_bwd(pyr, disps, poses, K, "hwc", d_warped, **_pose_kw(ctx.pc))
        if smooth is not None:      # the smoothness gradient is added in place by its kernel: no aten call
            ops.disp_smooth_bwd(disps, tgts, rest[3 * S], g_loss, *smooth, out=d_disps)
        return (None,) * 5 + tuple(d_disps) + tuple(d_poses)


class _MinReprojLossFullRes(torch.autograd.Function):
    """warp_full_res -> photometric_error -> min_reprojection as ONE node, every scale compared with the full-resolution target; the
    smoothness term stays where _MinReprojLoss has it: each disparity at its own size on the target pyramid."""

    @staticmethod
    def forward(ctx, tgt, src, K, cfg, S, *arrays):
        ssim_rate, auto_mask, weights, norm, smooth, pad, up, pc = cfg
        disps, poses = list(arrays[:S]), list(arrays[S:])
        B, n_src = src.shape[0], len(poses)
        H, W = tgt.shape[2:]
        hwc = ops.pyramid_hwc(src, 1)[0]
        warped, valid = ops.warp_full_res_fwd(hwc, disps, poses, K, "hwc", True, upsample=up, **_pose_kw(pc))
        errs = ops.photo_error_fwd(warped, [tgt] * S, ssim_rate, pad)
        idents = None
        if auto_mask:     # the identity reprojection, ONCE: the target and the unwarped sources are the same at every scale
            idents = ops.photo_error_fwd([src.view(B, n_src, 3, H, W)], [tgt], ssim_rate, pad) * S
        loss, count, winners = ops.min_reproj_fwd(errs, valid, idents, weights, norm)
        if smooth is None:
            ctx.save_for_backward(K, count, hwc, tgt, *disps, *poses, *warped, *winners)
            ctx.cfg, ctx.conv, ctx.pc = (S, n_src, ssim_rate, weights, norm, None), (pad, up), pc
            return loss[S]
        tgts = ops.pyramid(tgt, S)
        sm_loss, stats = ops.disp_smooth_fwd(disps, tgts, *smooth)
        ctx.save_for_backward(K, count, hwc, tgt, *disps, *poses, *warped, *winners, stats, *tgts[1:])
        ctx.cfg, ctx.conv, ctx.pc = (S, n_src, ssim_rate, weights, norm, smooth), (pad, up), pc
        return loss[S] + sm_loss[S]

    @staticmethod
    def backward(ctx, g_total):
        S, n_src, ssim_rate, weights, norm, smooth = ctx.cfg
        if g_total is None:
            return (None,) * (5 + S + n_src)
        K, count, hwc, tgt = ctx.saved_tensors[:4]
        rest = list(ctx.saved_tensors[4:])
        disps, poses = rest[:S], rest[S:S + n_src]
        rest = rest[S + n_src:]
        warped, winners = rest[:S], rest[S:2 * S]
        g_loss = _g_loss(S, g_total, None, count.device)
        g_errs = ops.min_reproj_bwd(winners, count, g_loss, n_src, weights, norm, [tuple(tgt.shape[2:])] * S)
        pad, up = ctx.conv
        d_warped = ops.photo_error_bwd(warped, [tgt] * S, ssim_rate, g_errs, pad)
        d_disps, d_poses = ops.warp_full_res_bwd(hwc, disps, poses, K, "hwc", d_warped, upsample=up, **_pose_kw(ctx.pc))
        if smooth is not None:      # the smoothness gradient is added in place by its kernel: no aten call
            ops.disp_smooth_bwd(disps, [tgt] + rest[2 * S + 1:], rest[2 * S], g_loss, *smooth, out=d_disps)
        return (None,) * 5 + tuple(d_disps) + tuple(d_poses)


def min_reprojection_loss(tgt_img, src_imgs, intrinsics, pred_disps, pred_poses, *, ssim_rate, auto_mask=True, weights=None, norm="kept",
                          smooth_weight=0.0, smooth_normalize=True, smooth_edge="mean_abs", full_res=False, ssim_padding="zero",
                          upsample="align_corners", pose_format="euler", invert=None, depth_range=None):
    """The Monodepth2-style loss of INTEGRATION.md ("Your own loss on the library's warp") in one call and ONE autograd node: per
    pixel the smallest ssim_rate * SSIM + (1 - ssim_rate) * L1 error over the warped sources that are in view, averaged per scale
    over the pixels where it is strictly below the error of every UNWARPED source (`auto_mask`; off: over the pixels some source
    sees), the scales added with `weights` (default 2**-s).

    The inputs are those of `sfm_learner_loss`: tgt_img (B,3,H,W) and src_imgs (B,n_src,3,H,W) float32, constants; intrinsics
    (B,S,3,3), a constant HERE as in `warp_pyramid` (TypeError if it requires grad); pred_disps: S tensors (B,1,H>>s,W>>s);
    pred_poses: n_src tensors (B,6) or one packed (B,6*n_src) tensor -- float32, bfloat16 or float16, each gradient returned in its
    input's dtype.  norm: "kept" or "all", as in `min_reprojection`.

    Returns total (0-d).  Forward: the source pyramid, `warp_pyramid`'s launch with its valid masks, the target pyramid,
    `photometric_error`'s launch on the warped pyramid and, with `auto_mask`, on the unwarped one, `min_reprojection`'s two.  Backward:
    one launch each of min_reprojection, photometric_error and the warp, plus the warp's small fold.  The values are those of the three
    stages called one after the other, bit for bit; nothing reads a device value on the host, so the step can be captured in a graph.

    smooth_weight > 0 adds the second term of that objective in the SAME node: smooth_weight * the total of `disparity_smoothness`
    on the target pyramid the node already holds, with `smooth_normalize` and `smooth_edge` as its `normalize` and `edge` and the
    per-scale weights float32(smooth_weight * weights[s]).  Two more launches forward and one aten add of the two totals; one more
    launch backward, which adds its gradient into d_disp in place.  The total and the gradients are those of the two calls added in
    float32, bit for bit.  With smooth_weight == 0 (the default) nothing of this runs and `smooth_normalize` and `smooth_edge` are not looked at.

    full_res=True is Monodepth2's full-resolution multi-scale form, still ONE node: `warp_full_res` instead of `warp_pyramid` (every
    disparity upsampled inside the warp of the full-resolution sources; intrinsics may then also be the full-resolution (B,3,3)
    alone, and pred_disps[s] may have any size unless smooth_weight > 0), `photometric_error` of the S full-resolution warped sets
    against the full-resolution target, the identity error computed once and handed to `min_reprojection` for every scale, and the
    smoothness term unchanged: each disparity at its own size on the target pyramid.  The total and the gradients are those of
    these stages called one after the other, bit for bit.  With full_res=False (the default) the call is what it was.

    ssim_padding="reflect" and upsample="half_pixel" are Monodepth2's own conventions, the `padding` of `photometric_error` -- applied
    to the warped error and to the identity error alike -- and the `upsample` of `warp_full_res`; the smoothness term looks at neither.
    Still one node with the same launches, and still the stages called one after the other with these arguments, bit for bit.
    upsample="half_pixel" without full_res=True raises ValueError (the pyramid form upsamples nothing), as does any unknown name.

    pose_format, invert and depth_range are those of `warp_pyramid` / `warp_full_res` and reach the WARP only: the smoothness term
    keeps reading the raw pred_disps, which is Monodepth2's own split (disp_to_depth in front of the warp, the sigmoid output in the
    smoothness term).  pose_format="axis_angle", invert=[True, False] and depth_range=(0.1, 100.0) are that code's
    transformation_from_parameters and disp_to_depth.  Still one node with the same launches; at their defaults the call is what it was."""
    _lib.ssim_padding_id(ssim_padding, "ssim_padding")
    pc = _pose_conv_args(src_imgs, pose_format, invert, depth_range)
    if _lib.upsample_id(upsample) != _lib.UPSAMPLE_ALIGN_CORNERS and not full_res:
        raise ValueError("upsample=%r needs full_res=True: the pyramid form compares every disparity at its own size" % (upsample,))
    if smooth_weight:       # (0, the default: nothing below is looked at, the call costs what it cost before the term existed)
        smooth_weight = float(smooth_weight)
        if not smooth_weight >= 0.0:
            raise ValueError("smooth_weight must be >= 0, got %r" % (smooth_weight,))
        _lib.disp_smooth_edge_id(smooth_edge)
    tgt = ops._dev(tgt_img, "tgt_img", 4)
    if full_res:
        src, K, disps, poses = _full_res_inputs(src_imgs, intrinsics, pred_disps, pred_poses, "min_reprojection_loss", pose_format)
        B, n_src, _, H, W = src.shape
        if tuple(tgt.shape) != (B, 3, H, W) or tgt.device != src.device:
            raise TypeError("tgt_img must be (B,3,H,W) = %s on %s, got %s on %s" % ((B, 3, H, W), src.device, tuple(tgt.shape), tgt.device))
        for s, t in enumerate(disps):       # (the smoothness term reads the target pyramid at each disparity's own size)
            if smooth_weight and tuple(t.shape[2:]) != (H >> s, W >> s):
                raise TypeError("pred_disps[%d] must be (B,1,H>>%d,W>>%d) = %s with smooth_weight > 0, got %s"
                                % (s, s, s, (B, 1, H >> s, W >> s), tuple(t.shape)))
        node = _MinReprojLossFullRes
    else:
        src, K, disps, poses, _ = _step_inputs(src_imgs, intrinsics, pred_disps, pred_poses, tgt, pose_format=pose_format)
        if K.requires_grad:
            raise TypeError("min_reprojection_loss does not differentiate the intrinsics: detach them")
        B, n_src, _, H, W = src.shape
        node = _MinReprojLoss
    S = len(disps)
    weights = _scale_weights(weights, S)
    smooth = (tuple(smooth_weight * w for w in weights), bool(smooth_normalize), smooth_edge) if smooth_weight else None
    cfg = (float(ssim_rate), bool(auto_mask), weights, norm, smooth, ssim_padding, upsample, pc)
    _lib.min_reproj_norm_id(norm)
    return node.apply(tgt.detach(), src.detach().view(B, 3 * n_src, H, W), K, cfg, S, *disps, *poses)


def _unit_weights(weights, S):
    """`weights` of pairwise_mean / sc_sfm_loss as a tuple of S floats; None: 1.0 each -- SC-SfMLearner adds the scales unweighted
    (NOT the 2**-s of `min_reprojection`)"""
    if weights is None:
        return (1.0,) * S
    weights = tuple(float(w) for w in weights)
    if len(weights) != S:
        raise TypeError("weights: one per scale, got %d for %d scales" % (len(weights), S))
    return weights


def _min_counts(min_count):
    try:
        photo, geom = (int(v) for v in min_count)
    except (TypeError, ValueError):
        raise ValueError("min_count must be (photo, geometry), two integers >= 0, got %r" % (min_count,)) from None
    if photo < 0 or geom < 0:
        raise ValueError("min_count must be (photo, geometry), two integers >= 0, got %r" % (min_count,))
    return photo, geom


def _pairwise_g_loss(n_pairs, g_pt, g_gt, g_p, g_g, device):
    """(2*n_pairs+2,) float32: the upstream gradients in the layout sfm_pairwise_bwd reads; None is zero.  On the device."""
    parts = []
    for g, n in ((g_p, n_pairs), (g_g, n_pairs), (g_pt, 1), (g_gt, 1)):
        parts.append(torch.zeros((n,), dtype=torch.float32, device=device) if g is None else g.to(torch.float32).reshape(n))
    return torch.cat(parts)


class _PairwiseMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, weights, min_count, detach_weight, bound, has_ident, has_cmp, *arrays):
        errs, diffs, rest = list(arrays[:S]), list(arrays[S:2 * S]), list(arrays[2 * S:])
        valids = [rest.pop(0) if on else None for on in bound]
        idents = rest[:S] if has_ident else None
        cmps = rest[S:2 * S] if has_cmp else None
        loss, count, keeps = ops.pairwise_fwd(errs, diffs, valids, idents, cmps, weights, min_count, detach_weight)
        n = errs[0].shape[1]
        ctx.save_for_backward(count, *errs, *diffs, *keeps)
        ctx.cfg = (S, n, weights, min_count, detach_weight, len(arrays))
        ctx.mark_non_differentiable(*keeps)
        ctx.set_materialize_grads(False)
        N = S * n
        return (loss[2 * N], loss[2 * N + 1], loss[:N].view(S, n), loss[N:2 * N].view(S, n)) + tuple(keeps)

    @staticmethod
    def backward(ctx, g_pt, g_gt, g_p, g_g, *_):
        S, n, weights, min_count, detach_weight, n_arrays = ctx.cfg
        if g_pt is None and g_gt is None and g_p is None and g_g is None:
            return (None,) * (7 + n_arrays)
        count, rest = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        errs, diffs, keeps = rest[:S], rest[S:2 * S], rest[2 * S:]
        want = any(ctx.needs_input_grad[7 + S:7 + 2 * S])
        g_loss = _pairwise_g_loss(S * n, g_pt, g_gt, g_p, g_g, count.device)
        g_errs, g_diffs = ops.pairwise_bwd(errs, diffs, keeps, count, g_loss, weights, min_count, detach_weight, want_g_diff=want)
        return (None,) * 7 + tuple(g_errs) + (tuple(g_diffs) if want else (None,) * S) + (None,) * (n_arrays - 2 * S)


def pairwise_mean(errs, diffs, *, valid=None, ident=None, cmp=None, weights=None, min_count=(0, 0), detach_weight=False):
    """The last stage of SC-SfMLearner's compute_pairwise_loss on the library's maps: per (scale, source), over the whole batch, the
    mean of err * (1 - diff) -- the photometric error under the self-discovered mask -- and of diff -- the geometry-consistency loss
    -- over the kept pixels, every scale and source in two launches (ops.pairwise_fwd) and one backward (ops.pairwise_bwd); what
    INTEGRATION.md spells as (e * (1 - d) * v).sum() / v.sum().clamp(min=1) and (d * v).sum() / v.sum().clamp(min=1) per scale.

    errs, diffs: lists of S tensors (B,n,h_s,w_s) -- what `photometric_error` returns for the list `warp_pyramid` returns, and what
      `depth_consistency` returns; float32, bfloat16 or float16 on a ROCm device (computed in float32, each gradient returned in its
      input's dtype);
    valid: None, or a list of S entries, each (B,n,h_s,w_s) float32 or None -- `warp_pyramid(..., return_valid=True)`: a pixel with
      valid <= 0 is dropped;
    ident: None (no auto-mask) or a list of S tensors (B,n,h_s,w_s) float32, the error of UNWARPED source i against the target: a
      pixel is kept only where `cmp` -- None: errs itself -- is strictly below it (a tie or a NaN drops the pixel).  SC-SfMLearner
      compares the channel-mean L1 of the warped and of the unwarped source: photometric_error at ssim_rate=0 as `cmp` and `ident`;
    weights: one per scale; None means 1.0 for every scale, as SC-SfMLearner adds them -- NOT the 2**-s of `min_reprojection`;
    min_count=(photo, geometry): a mean over at most that many pixels is 0, with a zero gradient -- mean_on_mask's
      `mask.sum() > 10000` on a mask expanded to the channels is (3333, 10000) on this library's channel-mean error map; (0, 0) is
      the clamp(min=1) of INTEGRATION.md;
    detach_weight: the weight 1 - diff carries no gradient to `diffs` (the geometry mean still does).

    Returns (photo_total, geom_total, photo, geom, keeps): the totals, 0-d, = sum_s weights[s] * sum_i photo[s, i] (and geom); photo
    and geom (S,n), the mean of each (scale, source); all four differentiable with respect to `errs` and `diffs` ONLY; keeps, a list of
    S int8 maps (B,n,h_s,w_s), 1 where the pixel is kept.  Dropped pixels are excluded by selection: a NaN there changes nothing.
    Sums run in fp64 in a fixed order: the same bits on every call.  Nothing reads a device value on the host: it runs under
    torch.cuda.graph capture."""
    if not isinstance(errs, (list, tuple)) or not isinstance(diffs, (list, tuple)):
        raise TypeError("errs and diffs must be lists of (B,n,h,w) tensors, one per scale")
    S = len(errs)
    if not 1 <= S <= _lib.SFM_MAX_SCALES or len(diffs) != S:
        raise TypeError("1..%d scales, and as many diffs as errs: got %d and %d" % (_lib.SFM_MAX_SCALES, S, len(diffs)))
    min_count = _min_counts(min_count)
    weights = _unit_weights(weights, S)
    xs = [_dev_float(t, "errs[%d]" % s, 4) for s, t in enumerate(errs)]
    ds = [_dev_float(t, "diffs[%d]" % s, 4) for s, t in enumerate(diffs)]
    valid = [None] * S if valid is None else list(valid)
    if len(valid) != S or (ident is not None and len(ident) != S) or (cmp is not None and len(cmp) != S):
        raise TypeError("valid, ident and cmp need one entry per scale (%d)" % S)
    if cmp is not None and ident is None:
        raise TypeError("cmp without ident: there is nothing to compare it with")
    bound = tuple(v is not None for v in valid)
    vs = [ops._dev(v, "valid[%d]" % s, 4).detach() for s, v in enumerate(valid) if v is not None]
    ids = [] if ident is None else [t.detach() for t in ops._devs(ident, "ident", 4)]
    cs = [] if cmp is None else [t.detach() for t in ops._devs(cmp, "cmp", 4)]
    out = _PairwiseMean.apply(S, weights, min_count, bool(detach_weight), bound, ident is not None, cmp is not None, *xs, *ds, *vs, *ids, *cs)
    return out[0], out[1], out[2], out[3], list(out[4:])


_AUTO_MASKS = {False: None, None: None, "error": "error", "l1": "l1"}


class _ScSfmLoss(torch.autograd.Function):
    """warp_pyramid -> photometric_error -> depth_consistency -> pairwise_mean (-> disparity_smoothness) as ONE node: one direction
    of compute_photo_and_geometry_loss for every scale and source."""

    @staticmethod
    def forward(ctx, tgt, src, K, cfg, S, *arrays):
        ssim_rate, auto_mask, with_mask, detach_weight, min_count, weights, geometry_weight, smooth, pad, pc = cfg
        disps, src_disps, poses = list(arrays[:S]), list(arrays[S:2 * S]), list(arrays[2 * S:])
        B, n_src = src.shape[0], len(poses)
        pyr = ops.pyramid_hwc(src, S)
        warped, valid = ops.warp_pyramid_fwd(pyr, disps, poses, K, "hwc", True, **_pose_kw(pc))
        tgts = ops.pyramid(tgt, S)
        errs = ops.photo_error_fwd(warped, tgts, ssim_rate, pad)
        idents = cmps = None
        if auto_mask is not None:     # the identity error: the planar source pyramid is (B,n_src,3,h,w) byte for byte
            plain = [p.view(B, n_src, 3, p.shape[2], p.shape[3]) for p in ops.pyramid(src, S)]
            if auto_mask == "l1":     # SC-SfMLearner's own test: the channel-mean L1 of the warped against that of the unwarped source
                cmps = ops.photo_error_fwd(warped, tgts, 0.0, pad)
                idents = ops.photo_error_fwd(plain, tgts, 0.0, pad)
            else:
                idents = ops.photo_error_fwd(plain, tgts, ssim_rate, pad)
        diffs = ops.depth_consistency_fwd(disps, src_disps, poses, K, **_pose_kw(pc))
        loss, count, keeps = ops.pairwise_fwd(errs, diffs, valid, idents, cmps, weights, min_count, detach_weight)
        N = S * n_src
        photo, geom = loss[2 * N], loss[2 * N + 1]
        saved = [K, count, *pyr, *disps, *src_disps, *poses, *warped, *tgts, *errs, *diffs, *keeps]
        if not with_mask:             # the photometric means of the SAME stage on a zero diff: e * (1.0f - 0.0f) is e, bit for bit
            zeros = [torch.zeros_like(d) for d in diffs]
            loss0, count, keeps = ops.pairwise_fwd(errs, zeros, valid, idents, cmps, weights, min_count, True)
            photo = loss0[2 * N]
            saved += zeros
        total = photo + geometry_weight * geom
        if smooth is not None:        # on the target pyramid this node holds anyway: the RAW disparities
            sm_loss, stats = ops.disp_smooth_fwd(disps, tgts, *smooth)
            saved.append(stats)
            total = total + sm_loss[S]
        ctx.save_for_backward(*saved)
        ctx.cfg, ctx.S, ctx.n_src = cfg, S, n_src
        ctx.set_materialize_grads(False)
        return total, photo, geom

    @staticmethod
    def backward(ctx, g_total, g_photo, g_geom):
        ssim_rate, auto_mask, with_mask, detach_weight, min_count, weights, geometry_weight, smooth, pad, pc = ctx.cfg
        S, n_src = ctx.S, ctx.n_src
        if g_total is None and g_photo is None and g_geom is None:
            return (None,) * (5 + 2 * S + n_src)
        K, count, rest = ctx.saved_tensors[0], ctx.saved_tensors[1], list(ctx.saved_tensors[2:])
        take = lambda k: [rest.pop(0) for _ in range(k)]
        pyr, disps, src_disps, poses = take(S), take(S), take(S), take(n_src)
        warped, tgts, errs, diffs, keeps = take(S), take(S), take(S), take(S), take(S)
        zeros = take(S) if not with_mask else None
        dev, N = count.device, S * n_src
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        gt = None if g_total is None else g_total.to(torch.float32)
        g_pt = zero if gt is None else gt
        g_gt = zero if gt is None else geometry_weight * gt
        if g_photo is not None:
            g_pt = g_pt + g_photo.to(torch.float32)
        if g_geom is not None:
            g_gt = g_gt + g_geom.to(torch.float32)
        if with_mask:
            g_errs, g_diffs = ops.pairwise_bwd(errs, diffs, keeps, count, _pairwise_g_loss(N, g_pt, g_gt, None, None, dev), weights,
                                               min_count, detach_weight)
        else:                         # the two calls of the forward: the photometric one on the zero diff, the geometry one without the weight
            g_errs, _ = ops.pairwise_bwd(errs, zeros, keeps, count, _pairwise_g_loss(N, g_pt, None, None, None, dev), weights, min_count,
                                         True, want_g_diff=False)
            _, g_diffs = ops.pairwise_bwd(errs, diffs, keeps, count, _pairwise_g_loss(N, None, g_gt, None, None, dev), weights, min_count,
                                          True)
        d_warped = ops.photo_error_bwd(warped, tgts, ssim_rate, g_errs, pad)
        d_disps, d_poses = ops.warp_pyramid_bwd(pyr, disps, poses, K, "hwc", d_warped, **_pose_kw(pc))
        want = any(ctx.needs_input_grad[5 + S:5 + 2 * S])      # src_disps that do not require grad: the kernel without the scatter
        c_disps, c_poses, d_src = ops.depth_consistency_bwd(disps, src_disps, poses, K, g_diffs, want_d_src_disp=want, **_pose_kw(pc))
        for a, b in zip(d_disps + d_poses, c_disps + c_poses):      # float32, the warp's first: warp + depth_consistency
            a.add_(b)
        if smooth is not None:        # the smoothness gradient is added in place by its kernel: no aten call
            ops.disp_smooth_bwd(disps, tgts, rest[0], _g_loss(S, gt, None, dev), *smooth, out=d_disps)
        return (None,) * 5 + tuple(d_disps) + (tuple(d_src) if want else (None,) * S) + tuple(d_poses)


def sc_sfm_loss(tgt_img, src_imgs, intrinsics, tgt_disps, src_disps, pred_poses, *, ssim_rate=0.85, geometry_weight=0.5, smooth_weight=0.0,
                auto_mask=False, with_mask=True, detach_weight=False, min_count=(0, 0), weights=None, bidirectional=True,
                ssim_padding="zero", pose_format="euler", invert=None, depth_range=None, smooth_normalize=True, smooth_edge="mean_abs"):
    """SC-SfMLearner's objective (Bian et al., NeurIPS 2019: compute_photo_and_geometry_loss) on this library's warp in one call, ONE
    autograd node per direction:

      total = photo + geometry_weight * geometry (+ smooth),    added in float32 in that order

    with photo the sum over the scales (times weights[s]) and the sources of the mean of err * (1 - diff_depth) over the kept pixels,
    geometry that of diff_depth, err = ssim_rate * SSIM + (1 - ssim_rate) * L1 of `photometric_error`, diff_depth of
    `depth_consistency` and the means of `pairwise_mean`; a pixel is kept where the warp is in view and it passes the auto-mask.

    tgt_img (B,3,H,W), src_imgs (B,n_src,3,H,W) float32: constants; intrinsics (B,S,3,3): a constant (TypeError if it requires grad);
    tgt_disps: S tensors (B,1,H>>s,W>>s), the network on the target frame; src_disps: S tensors (B,n_src,H>>s,W>>s), the SAME network
    on each source frame; pred_poses: n_src tensors (B,6) or one packed (B,6*n_src) tensor.  Predictions are float32, bfloat16 or
    float16, each gradient returned in its input's dtype.

    auto_mask: False; "l1" -- SC-SfMLearner's own test: the pixel is kept where the channel-mean L1 of the warped source is strictly
      below that of the unwarped one (the two error maps at ssim_rate = 0, `cmp` / `ident` of `pairwise_mean`); or "error" -- the
      unwarped error at `ssim_rate` compared against err itself (Monodepth2's form of the test);
    with_mask=False: the photometric term is the plain masked mean of err.  The stage runs twice, once more on a zero diff -- e *
      (1.0f - 0.0f) is e, bit for bit -- and the backward runs its launch twice; the geometry term is unchanged;
    detach_weight, min_count, weights: those of `pairwise_mean`; weights=None adds the scales unweighted;
    smooth_weight > 0 adds smooth_weight * the total of `disparity_smoothness` (per-scale weights float32(smooth_weight * weights[s]),
      `smooth_normalize`, `smooth_edge`) of the TARGET frame on the target pyramid, in the first direction's node;
    ssim_padding, pose_format, invert, depth_range: those of `min_reprojection_loss`; depth_range acts on every disparity.

    One direction, forward: the source pyramid, `warp_pyramid`'s launch with its valid masks, the target pyramid, `photometric_error`'s
    launch (with auto_mask two more, "l1", or one more, "error"), `depth_consistency`'s, `pairwise_mean`'s two, optionally the
    smoothness' two.  Backward: one launch of pairwise_mean, one of photometric_error, the warp's two, depth_consistency's two -- its
    scatter into d_src_disp only where src_disps require grad -- then d_disp and d_pose of the warp and of depth_consistency added in
    float32, the warp's first, and the smoothness gradient added in place by its own launch.  The values are those of the stages called
    one after the other, bit for bit; nothing reads a device value on the host, so the step can be captured in a graph.

    bidirectional=True (the default) adds the second direction of compute_photo_and_geometry_loss as a second node: every source
    becomes the target of a batch of B*n_src samples with ONE reference frame, the original target -- its own src_disps are the target
    disparities, tgt_disps the reference's, the pose of its pair is used with the inversion flag flipped, the intrinsics are repeated.
    The reshapes are plain aten; the three scalars of the two directions are added in float32, the first direction's first.  The
    second direction's means run over the B*n_src pairs TOGETHER (one mean per scale, not one per source), which is the
    count-weighted average of the per-source means the loop of INTEGRATION.md adds up.  It needs one inversion flag for all sources
    (invert=None or all equal: ValueError otherwise) and a 6-vector pose: pose_format="matrix" with bidirectional=True is a
    ValueError -- invert the matrices and call each direction yourself.

    Returns (total, photo, geometry), three 0-d tensors.

    Out of scope: SC-SfMLearner's clamp(0, 1) of the per-channel L1 in front of the channel mean.  `photometric_error` does not have
    it, and it never acts on images in [0, 1]."""
    _lib.ssim_padding_id(ssim_padding, "ssim_padding")
    if isinstance(auto_mask, torch.Tensor) or auto_mask not in _AUTO_MASKS:
        raise ValueError("auto_mask must be False, 'error' or 'l1', got %r" % (auto_mask,))
    auto_mask = _AUTO_MASKS[auto_mask]
    pc = _pose_conv_args(src_imgs, pose_format, invert, depth_range)
    if bidirectional and pose_format == "matrix":
        raise ValueError("pose_format='matrix' with bidirectional=True: invert the matrices and call each direction yourself")
    if bidirectional and pc[1] is not None and len(set(pc[1])) > 1:
        raise ValueError("bidirectional=True needs one inversion flag for all sources, got invert=%r" % (invert,))
    min_count = _min_counts(min_count)
    geometry_weight = float(geometry_weight)
    if smooth_weight:
        smooth_weight = float(smooth_weight)
        if not smooth_weight >= 0.0:
            raise ValueError("smooth_weight must be >= 0, got %r" % (smooth_weight,))
        _lib.disp_smooth_edge_id(smooth_edge)
    tgt = ops._dev(tgt_img, "tgt_img", 4)
    if isinstance(tgt_disps, torch.Tensor) or isinstance(src_disps, torch.Tensor):
        raise TypeError("tgt_disps and src_disps are lists with one tensor per scale")
    src, K, disps, poses, _ = _step_inputs(src_imgs, intrinsics, tgt_disps, pred_poses, tgt, pose_format=pose_format)
    if K.requires_grad:
        raise TypeError("sc_sfm_loss does not differentiate the intrinsics: detach them")
    B, n_src, _, H, W = src.shape
    S = len(disps)
    if len(src_disps) != S:
        raise TypeError("as many src_disps as tgt_disps: got %d and %d" % (len(src_disps), S))
    srcs = []
    for s, t in enumerate(src_disps):
        t = _dev_float(t, "src_disps[%d]" % s, 4)
        if tuple(t.shape) != (B, n_src, H >> s, W >> s) or t.device != tgt.device:
            raise TypeError("src_disps[%d] must be (B,n_src,H>>%d,W>>%d) = %s on %s, got %s"
                            % (s, s, s, (B, n_src, H >> s, W >> s), tgt.device, tuple(t.shape)))
        srcs.append(t)
    weights = _unit_weights(weights, S)
    smooth = (tuple(smooth_weight * w for w in weights), bool(smooth_normalize), smooth_edge) if smooth_weight else None
    head = (float(ssim_rate), auto_mask, bool(with_mask), bool(detach_weight), min_count, weights, geometry_weight)
    tgt, src = tgt.detach(), src.detach()
    out = _ScSfmLoss.apply(tgt, src.view(B, 3 * n_src, H, W), K, head + (smooth, ssim_padding, pc), S, *disps, *srcs, *poses)
    if not bidirectional:
        return out
    # the second direction: sample b * n_src + i is source i of sample b as the target, the original target as its one reference
    M = B * n_src
    flipped = (not (pc[1][0] if pc[1] is not None else False),)
    back = _ScSfmLoss.apply(src.reshape(M, 3, H, W), tgt[:, None].expand(B, n_src, 3, H, W).reshape(M, 3, H, W),
                            K.repeat_interleave(n_src, dim=0), head + (None, ssim_padding, (pc[0], flipped, pc[2])), S,
                            *[t.reshape(M, 1, t.shape[2], t.shape[3]) for t in srcs],
                            *[t.expand(B, n_src, t.shape[2], t.shape[3]).reshape(M, 1, t.shape[2], t.shape[3]) for t in disps],
                            torch.stack(poses, 1).reshape(M, 6))
    return tuple(a + b for a, b in zip(out, back))


def multi_scale_intrinsics(K, n_scales):
    """get_multi_scale_intrinsics, datasets/kitti/kitti_raw_transformed.py:76-93, for a batch and differentiable (plain torch, any
    device): K (B,3,3) -- fx, fy, cx, cy are read from [0,0], [1,1], [0,2], [1,2], as the reference does -- or (B,4) = (fx, fy, cx,
    cy), e.g. a learned parameter -> (B,n_scales,3,3): scale s is [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with the four divided by
    2**s.  What `sfm_learner_loss` takes as `intrinsics`."""
    if not isinstance(K, torch.Tensor) or not K.is_floating_point():
        raise TypeError("multi_scale_intrinsics: expected a floating-point torch.Tensor")
    if K.dim() == 3 and tuple(K.shape[1:]) == (3, 3):
        f = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], dim=1)
    elif K.dim() == 2 and K.shape[1] == 4:
        f = K
    else:
        raise TypeError("multi_scale_intrinsics: K must be (B,3,3) or (B,4) = (fx, fy, cx, cy), got %s" % (tuple(K.shape),))
    if not 1 <= int(n_scales) <= _lib.SFM_MAX_SCALES:
        raise TypeError("n_scales must be in [1, %d]" % _lib.SFM_MAX_SCALES)
    v = torch.stack([f / float(2 ** s) for s in range(int(n_scales))], dim=1)     # (B,S,4); no host array goes to the device
    zero, one = torch.zeros_like(v[..., 0]), torch.ones_like(v[..., 0])
    rows = [v[..., 0], zero, v[..., 2], zero, v[..., 1], v[..., 3], zero, zero, one]
    return torch.stack(rows, dim=-1).reshape(f.shape[0], int(n_scales), 3, 3)


class _DispAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *xs):
        outs = ops.disp_act_fwd(xs)
        ctx.save_for_backward(*outs)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        return tuple(ops.disp_act_bwd(ctx.saved_tensors, [g.contiguous() for g in gs]))


def disp_activation(xs):
    """DispNet's output activation, models/disp_net.py:104-122: [10 * sigmoid(x) + 0.01 for x in xs], all scales in one launch
    (ops.disp_act_fwd; backward ops.disp_act_bwd).  float32, bfloat16 or float16 on a ROCm device (the logits of a network under
    autocast): computed and returned in float32, each gradient returned in its input's dtype."""
    return list(_DispAct.apply(*[_dev_float(x, "xs[%d]" % k) for k, x in enumerate(xs)]))


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_hw):
        ctx.in_hw = tuple(x.shape[2:])
        return ops.resize(x, out_hw)

    @staticmethod
    def backward(ctx, g):
        return ops.resize_bwd(g.contiguous(), ctx.in_hw), None


def resize_images(x, output_shape):
    """F.resize_images(x, (out_H, out_W)), bilinear and align-corners, as DispNet's decoder calls it (models/disp_net.py:105,111,117):
    x (N,C,H,W) -> (N,C,out_H,out_W), sampled at the reference's double linspace positions (ops.resize).  The gradient is that
    map's adjoint, computed as a gather (ops.resize_bwd): no atomics, the same bits on every run.  float32, bfloat16 or float16 on
    a ROCm device: computed and returned in float32, the gradient returned in the input's dtype."""
    return _Resize.apply(_dev_float(x, "x", 4), (int(output_shape[0]), int(output_shape[1])))


def resize_like(inputs, ref):
    """models/disp_net.py:11-14: `inputs` resized to the height and width of `ref`; `inputs` itself when they already agree."""
    if tuple(inputs.shape[2:]) == tuple(ref.shape[2:]):
        return inputs
    return resize_images(inputs, ref.shape[2:])
