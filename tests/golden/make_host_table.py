#!/usr/bin/env python3
"""Writes host_plans.npz and host_rejects.json: what the Python host layer (ops.py, torch_api.py, augment.py) decides without a
device.

host_plans.npz: for a fixed grid of configurations, what torch_api._plan returns under FakeTensorMode -- the descriptor bytes
(every non-pointer field, _FAKE for the pointers), the workspace size, where each pyramid level and the workspace lie in the
per-call scratch buffer, the scratch length, the gradient spans and their total.  A configuration the library refuses (a 16x24
frame has a 2x3 fourth scale) is recorded by the class and text of the exception instead.

host_rejects.json: every refusal of the Python layer that is reachable before the first data_ptr() -- CPU tensors, fake-CUDA
tensors of the wrong dtype, ndim or shape, wrong counts, bad settings -- as [label, exception class, full message].

Nothing is launched and no GPU is needed.  The committed files pin the commit that introduced them;
tests/test_host_table_cpu.py replays both against the package as it is.  Regenerate them only in a change that alters a plan or a
message on purpose, and say why.

usage: python tests/golden/make_host_table.py [out_dir]"""
import importlib
import itertools
import json
import os
import sys

import numpy as np
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PKG = "sfm-learner-chainer_amd"
_lib = importlib.import_module(PKG + "._lib")
ops = importlib.import_module(PKG + ".ops")
ta = importlib.import_module(PKG + ".torch_api")
augment = importlib.import_module(PKG + ".augment")

# ---------------------------------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------------------------------
BATCHES = (1, 4)
FRAMES = ((16, 24), (128, 416), (1024, 1376))      # the last has HWC_MAX_PIXELS pixels or more: planar
N_SRC = (1, 2, 4)
SCALES = (1, 4)
MASKS = (0, 1)
SMOOTH = ("none", "second_order", "edge_aware")
PROJECTIONS = ("fast", "reference_order")
NORM = (1, 4)                                      # norm_batch = B, 4 B
PARAMS = ("B", "frame", "n_src", "S", "masks", "smooth_mode", "projection", "norm")
MAX_SPANS = 2 * (4 + 4 + 4)                        # (offset, numel) of 4 d_disp, 4 d_pose, 4 d_mask
INT_FIELDS = ("ws_bytes", "ws_off", "scratch", "grad_floats")


def grid():
    return list(itertools.product(BATCHES, range(len(FRAMES)), N_SRC, SCALES, MASKS, range(len(SMOOTH)), range(len(PROJECTIONS)), NORM))


def plan(B, frame, n_src, S, masks, smooth, projection, norm):
    """torch_api._plan for one configuration, as sfm_learner_loss would call it"""
    H, W = FRAMES[frame]
    f = dict(dtype=torch.float32, device="cuda")
    ta._PLANS.clear()
    with FakeTensorMode():
        disps = [torch.empty(B, 1, H >> s, W >> s, **f) for s in range(S)]
        poses = [torch.empty(B, 6, **f) for _ in range(n_src)]
        logits = [torch.empty(B, n_src, H >> s, W >> s, **f) for s in range(S)] if masks else []
        cfg = (0.1, 0.2 if masks else 0.0, 0.15, _lib.SMOOTH_MODES[SMOOTH[smooth]], _lib.PROJECTIONS[PROJECTIONS[projection]], B * norm)
        return ta._plan(B, H, W, n_src, disps, logits, poses, cfg)


def plan_tables():
    params = np.array(grid(), np.int16)
    n = len(params)
    t = dict(params=params, desc=np.zeros((n, len(bytes(_lib.SfmLossDesc()))), np.uint8), hwc=np.zeros(n, np.int8),
             tgt_off=np.full((n, max(SCALES)), -1, np.int64), src_off=np.full((n, max(SCALES)), -1, np.int64),
             spans=np.full((n, MAX_SPANS), -1, np.int64), error=np.array([""] * n, dtype="U200"))
    for k in INT_FIELDS:
        t[k] = np.zeros(n, np.int64)
    for k, p in enumerate(params):
        try:
            pl = plan(*(int(v) for v in p))
        except Exception as e:        # the library refused the descriptor
            t["error"][k] = "%s: %s" % (type(e).__name__, e)
            continue
        t["desc"][k] = np.frombuffer(pl.desc, np.uint8)
        t["hwc"][k] = pl.hwc
        for name in ("tgt_off", "src_off"):        # None (planar scale 0: the frame itself) is -1
            t[name][k, :len(getattr(pl, name))] = [-1 if o is None else o for o in getattr(pl, name)]
        t["spans"][k, :len(pl.spans)] = pl.spans
        for name in INT_FIELDS:
            t[name][k] = getattr(pl, name)
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def T(*shape, dtype=torch.float32, device="cuda"):
    return torch.empty(*shape, dtype=dtype, device=device)


def _bind_args(B=2, H=16, W=24, S=2, n=2, hwc=False):
    tgt = [T(B, 1, H >> s, W >> s, 3) if hwc else T(B, 3, H >> s, W >> s) for s in range(S)]
    src = [T(B, n, H >> s, W >> s, 3) if hwc else T(B, 3 * n, H >> s, W >> s) for s in range(S)]
    return [tgt, src, T(B, S, 3, 3), [T(B, 1, H >> s, W >> s) for s in range(S)], [T(B, 6) for _ in range(n)]]


def _loss_args(B=2, H=16, W=24, S=2, n=2, device="cuda"):
    return [T(B, 3, H, W, device=device), T(B, n, 3, H, W, device=device), T(B, S, 3, 3, device=device),
            [T(B, 1, H >> s, W >> s, device=device) for s in range(S)], [T(B, 6, device=device) for _ in range(n)]]


def _with(args, k, v):
    return args[:k] + [v] + args[k + 1:]


def cases():
    """[(label, thunk)]: each thunk, called under FakeTensorMode, must raise"""
    out = []
    add = lambda label, fn: out.append((label, fn))
    F64, I32, CPU = dict(dtype=torch.float64), dict(dtype=torch.int32), dict(device="cpu")

    # the one tensor check, through an operator that does nothing else first
    add("resize: not a tensor", lambda: ops.resize([1.0], (4, 4)))
    add("resize: cpu", lambda: ops.resize(T(1, 3, 8, 8, **CPU), (4, 4)))
    add("resize: float64", lambda: ops.resize(T(1, 3, 8, 8, **F64), (4, 4)))
    add("resize: bfloat16", lambda: ops.resize(T(1, 3, 8, 8, dtype=torch.bfloat16), (4, 4)))
    add("resize: ndim 3", lambda: ops.resize(T(3, 8, 8), (4, 4)))

    add("pose_proj_fwd: pose6 cpu", lambda: ops.pose_proj_fwd(T(2, 6, **CPU), T(2, 3, 3)))
    add("pose_proj_fwd: K ndim", lambda: ops.pose_proj_fwd(T(2, 6), T(2, 9)))
    add("pose_proj_fwd: K float64", lambda: ops.pose_proj_fwd(T(2, 6), T(2, 3, 3, **F64)))
    add("pose_proj_fwd: pose6 (N,5)", lambda: ops.pose_proj_fwd(T(2, 5), T(2, 3, 3)))
    add("pose_proj_fwd: K of another N", lambda: ops.pose_proj_fwd(T(2, 6), T(3, 3, 3)))
    add("pose_proj_bwd: pose6 ndim", lambda: ops.pose_proj_bwd(T(12), T(2, 3, 3), T(2, 4, 4)))
    add("pose_proj_bwd: K cpu", lambda: ops.pose_proj_bwd(T(2, 6), T(2, 3, 3, **CPU), T(2, 4, 4)))
    add("pose_proj_bwd: g_proj ndim", lambda: ops.pose_proj_bwd(T(2, 6), T(2, 3, 3), T(2, 16)))
    add("pose_proj_bwd: g_proj int32", lambda: ops.pose_proj_bwd(T(2, 6), T(2, 3, 3), T(2, 4, 4, **I32)))

    w = lambda imgs=None, depth=None, pose=None, K=None: [T(2, 3, 8, 8) if imgs is None else imgs, T(2, 64) if depth is None else depth,
                                                          T(2, 6) if pose is None else pose, T(2, 3, 3) if K is None else K]
    for name, fn, extra in (("warp_fwd", ops.warp_fwd, []), ("warp_bwd", ops.warp_bwd, [None])):
        g = lambda a, extra=extra: a + ([T(2, 3, 8, 8)] if extra else [])
        add(name + ": imgs cpu", lambda fn=fn, g=g: fn(*g(w(imgs=T(2, 3, 8, 8, **CPU)))))
        add(name + ": imgs ndim 3", lambda fn=fn, g=g: fn(*g(w(imgs=T(3, 8, 8)))))
        add(name + ": depth float64", lambda fn=fn, g=g: fn(*g(w(depth=T(2, 64, **F64)))))
        add(name + ": depth of 2 rows", lambda fn=fn, g=g: fn(*g(w(depth=T(2, 2, 64)))))
        add(name + ": depth of another frame", lambda fn=fn, g=g: fn(*g(w(depth=T(2, 63)))))
        add(name + ": poses ndim", lambda fn=fn, g=g: fn(*g(w(pose=T(12)))))
        add(name + ": poses (N,5)", lambda fn=fn, g=g: fn(*g(w(pose=T(2, 5)))))
        add(name + ": K of another N", lambda fn=fn, g=g: fn(*g(w(K=T(1, 3, 3)))))
        add(name + ": K ndim", lambda fn=fn, g=g: fn(*g(w(K=T(2, 9)))))
    add("warp_bwd: g_warped of another shape", lambda: ops.warp_bwd(*w(), T(2, 3, 8, 7)))
    add("warp_bwd: g_warped ndim", lambda: ops.warp_bwd(*w(), T(2, 3, 64)))
    add("warp_bwd: g_warped cpu", lambda: ops.warp_bwd(*w(), T(2, 3, 8, 8, **CPU)))
    add("warp_bwd: depth of 3 rows, g_warped float64", lambda: ops.warp_bwd(*w(depth=T(2, 3, 64)), T(2, 3, 8, 8, **F64)))

    for name in ("sampler_fwd", "interp_fwd", "sampler_bwd", "interp_bwd"):
        fn = getattr(ops, name)
        g = (lambda a: a + [T(2, 3, 4, 5)]) if name.endswith("bwd") else (lambda a: a)
        add(name + ": x ndim", lambda fn=fn, g=g: fn(*g([T(2, 3, 64), T(2, 2, 4, 5)])))
        add(name + ": x cpu", lambda fn=fn, g=g: fn(*g([T(2, 3, 8, 8, **CPU), T(2, 2, 4, 5)])))
        add(name + ": grid float64", lambda fn=fn, g=g: fn(*g([T(2, 3, 8, 8), T(2, 2, 4, 5, **F64)])))
        add(name + ": grid of 3 channels", lambda fn=fn, g=g: fn(*g([T(2, 3, 8, 8), T(2, 3, 4, 5)])))
        add(name + ": grid of another N", lambda fn=fn, g=g: fn(*g([T(2, 3, 8, 8), T(1, 2, 4, 5)])))
    for name in ("sampler_bwd", "interp_bwd"):
        fn = getattr(ops, name)
        add(name + ": gy of another shape", lambda fn=fn: fn(T(2, 3, 8, 8), T(2, 2, 4, 5), T(2, 3, 5, 4)))
        add(name + ": gy ndim", lambda fn=fn: fn(T(2, 3, 8, 8), T(2, 2, 4, 5), T(2, 3, 20)))
        add(name + ": gy cpu", lambda fn=fn: fn(T(2, 3, 8, 8), T(2, 2, 4, 5), T(2, 3, 4, 5, **CPU)))

    for S in (0, 9):
        add("pyramid: n_scales %d" % S, lambda S=S: ops.pyramid(T(1, 3, 16, 24), S))
        add("pyramid_hwc: n_scales %d" % S, lambda S=S: ops.pyramid_hwc(T(1, 6, 16, 24), S))
        add("pyramid_pair_hwc: n_scales %d" % S, lambda S=S: ops.pyramid_pair_hwc(T(1, 3, 16, 24), T(1, 6, 16, 24), S))
    add("pyramid: x ndim", lambda: ops.pyramid(T(3, 16, 24), 2))
    add("pyramid: x cpu", lambda: ops.pyramid(T(1, 3, 16, 24, **CPU), 2))
    add("pyramid: out of another length", lambda: ops.pyramid(T(1, 3, 16, 24), 2, out=[T(1, 3, 16, 24)]))
    add("pyramid: out of another shape", lambda: ops.pyramid(T(1, 3, 16, 24), 2, out=[T(1, 3, 16, 24), T(1, 3, 8, 11)]))
    add("pyramid_hwc: x float64", lambda: ops.pyramid_hwc(T(1, 6, 16, 24, **F64), 2))
    add("pyramid_hwc: 4 channels", lambda: ops.pyramid_hwc(T(1, 4, 16, 24), 2))
    add("pyramid_hwc: 4 channels, n_scales 9", lambda: ops.pyramid_hwc(T(1, 4, 16, 24), 9))
    pp = ops.pyramid_pair_hwc
    add("pyramid_pair_hwc: tgt cpu", lambda: pp(T(1, 3, 16, 24, **CPU), T(1, 6, 16, 24), 2))
    add("pyramid_pair_hwc: src ndim", lambda: pp(T(1, 3, 16, 24), T(1, 2, 3, 16, 24), 2))
    add("pyramid_pair_hwc: tgt of 6 channels", lambda: pp(T(1, 6, 16, 24), T(1, 6, 16, 24), 2))
    add("pyramid_pair_hwc: src of another N", lambda: pp(T(1, 3, 16, 24), T(2, 6, 16, 24), 2))
    add("pyramid_pair_hwc: src of another frame", lambda: pp(T(1, 3, 16, 24), T(1, 6, 16, 22), 2))
    add("pyramid_pair_hwc: src of 4 channels", lambda: pp(T(1, 3, 16, 24), T(1, 4, 16, 24), 2))
    add("pyramid_pair_hwc: src of 0 channels", lambda: pp(T(1, 3, 16, 24), T(1, 0, 16, 24), 2))
    add("pyramid_pair_hwc: src of 4 channels, n_scales 0", lambda: pp(T(1, 3, 16, 24), T(1, 4, 16, 24), 0))
    yt, ys = lambda: [T(1, 1, 16, 24, 3), T(1, 1, 8, 12, 3)], lambda: [T(1, 2, 16, 24, 3), T(1, 2, 8, 12, 3)]
    add("pyramid_pair_hwc: out of another length", lambda: pp(T(1, 3, 16, 24), T(1, 6, 16, 24), 2, out=(yt()[:1], ys())))
    add("pyramid_pair_hwc: out ys of another length", lambda: pp(T(1, 3, 16, 24), T(1, 6, 16, 24), 2, out=(yt(), ys()[:1])))
    add("pyramid_pair_hwc: out yt[0] planar", lambda: pp(T(1, 3, 16, 24), T(1, 6, 16, 24), 2, out=([T(1, 3, 16, 24), yt()[1]], ys())))
    add("pyramid_pair_hwc: out ys[0] of 3 sources", lambda: pp(T(1, 3, 16, 24), T(1, 6, 16, 24), 2, out=(yt(), [T(1, 3, 16, 24, 3), ys()[1]])))
    add("pyramid_pair_hwc: out on the cpu", lambda: pp(T(1, 3, 16, 24), T(1, 6, 16, 24), 2,
                                                       out=([T(1, 1, 16, 24, 3, **CPU), T(1, 1, 8, 12, 3, **CPU)], ys())))

    add("disp_act_fwd: cpu", lambda: ops.disp_act_fwd([T(1, 1, 4, 4), T(1, 1, 2, 2, **CPU)]))
    add("disp_act_fwd: float16", lambda: ops.disp_act_fwd([T(1, 1, 4, 4, dtype=torch.float16)]))
    add("disp_act_fwd: not a tensor", lambda: ops.disp_act_fwd([None]))
    add("disp_act_bwd: disps int32", lambda: ops.disp_act_bwd([T(1, 1, 4, 4, **I32)], [T(1, 1, 4, 4)]))
    add("disp_act_bwd: g_disps cpu", lambda: ops.disp_act_bwd([T(1, 1, 4, 4)], [T(1, 1, 4, 4, **CPU)]))
    add("disp_act_bwd: g_disps of another shape", lambda: ops.disp_act_bwd([T(1, 1, 4, 4), T(1, 1, 2, 2)], [T(1, 1, 4, 4), T(1, 1, 2, 3)]))

    # FusedLoss
    add("FusedLoss: smooth_mode", lambda: ops.FusedLoss(smooth_mode="third_order"))
    add("FusedLoss: projection", lambda: ops.FusedLoss(projection="exact"))
    add("FusedLoss: smooth_mode and projection", lambda: ops.FusedLoss(smooth_mode="", projection=""))
    bind = lambda args, exp_reg=0.0, **kw: ops.FusedLoss(smooth_reg=0.1, exp_reg=exp_reg).bind(*args, **kw)
    add("bind: layout", lambda: bind(_bind_args(), layout="nhwc"))
    add("bind: layout None", lambda: bind(_bind_args(), layout=None))
    add("bind: one tgt scale short", lambda: bind(_with(_bind_args(), 0, _bind_args()[0][:1])))
    add("bind: one src scale more", lambda: bind(_with(_bind_args(), 1, _bind_args()[1] + [T(2, 6, 4, 6)])))
    add("bind: 9 scales", lambda: bind(_bind_args(H=1024, W=1024, S=9)))
    add("bind: 9 sources", lambda: bind(_bind_args(n=9)))
    add("bind: tgt_pyr[1] cpu", lambda: bind(_with(_bind_args(), 0, [T(2, 3, 16, 24), T(2, 3, 8, 12, **CPU)])))
    add("bind: tgt_pyr planar under hwc", lambda: bind(_bind_args(), layout="hwc"))
    add("bind: tgt_pyr hwc under planar", lambda: bind(_bind_args(hwc=True)))
    add("bind: src_pyr[0] float64", lambda: bind(_with(_bind_args(), 1, [T(2, 6, 16, 24, **F64), T(2, 6, 8, 12)])))
    add("bind: src_pyr[1] ndim under hwc", lambda: bind(_with(_bind_args(hwc=True), 1, [T(2, 2, 16, 24, 3), T(2, 6, 8, 12)]), layout="hwc"))
    add("bind: disps[1] ndim", lambda: bind(_with(_bind_args(), 3, [T(2, 1, 16, 24), T(2, 8, 12)])))
    add("bind: disps[0] not a tensor", lambda: bind(_with(_bind_args(), 3, [None, T(2, 1, 8, 12)])))
    add("bind: poses[1] ndim", lambda: bind(_with(_bind_args(), 4, [T(2, 6), T(12)])))
    add("bind: poses[0] cpu", lambda: bind(_with(_bind_args(), 4, [T(2, 6, **CPU), T(2, 6)])))
    add("bind: intrinsics ndim", lambda: bind(_with(_bind_args(), 2, T(2, 3, 3))))
    add("bind: intrinsics of one scale", lambda: bind(_with(_bind_args(), 2, T(2, 1, 3, 3))))
    add("bind: intrinsics of another B", lambda: bind(_with(_bind_args(), 2, T(1, 2, 3, 3))))
    add("bind: intrinsics float64", lambda: bind(_with(_bind_args(), 2, T(2, 2, 3, 3, **F64))))
    add("bind: exp_reg without masks", lambda: bind(_bind_args(), exp_reg=0.2))
    add("bind: exp_reg without masks, hwc", lambda: bind(_bind_args(hwc=True), exp_reg=0.2, layout="hwc"))
    add("bind: masks[1] ndim", lambda: bind(_bind_args(), exp_reg=0.2, masks=[T(2, 2, 16, 24), T(2, 2, 96)]))
    add("bind: masks[0] cpu", lambda: bind(_bind_args(), exp_reg=0.2, masks=[T(2, 2, 16, 24, **CPU), T(2, 2, 8, 12)]))

    # torch_api.sfm_learner_loss
    L = lambda a, **kw: ta.sfm_learner_loss(*a, **dict(dict(smooth_reg=0.1), **kw))
    add("loss: smooth_mode", lambda: L(_loss_args(), smooth_mode="third_order"))
    add("loss: projection", lambda: L(_loss_args(), projection="exact"))
    add("loss: smooth_mode on cpu tensors", lambda: L(_loss_args(device="cpu"), smooth_mode="x"))
    add("loss: cpu", lambda: L(_loss_args(device="cpu")))
    add("loss: tgt_img not a tensor", lambda: L(_with(_loss_args(), 0, None)))
    add("loss: tgt_img bfloat16", lambda: L(_with(_loss_args(), 0, T(2, 3, 16, 24, dtype=torch.bfloat16))))
    add("loss: tgt_img ndim", lambda: L(_with(_loss_args(), 0, T(3, 16, 24))))
    add("loss: src_imgs stacked", lambda: L(_with(_loss_args(), 1, T(2, 6, 16, 24))))
    add("loss: src_imgs float64", lambda: L(_with(_loss_args(), 1, T(2, 2, 3, 16, 24, **F64))))
    add("loss: tgt_img of 2 channels", lambda: L(_with(_loss_args(), 0, T(2, 2, 16, 24))))
    add("loss: tgt_img of another B", lambda: L(_with(_loss_args(), 0, T(1, 3, 16, 24))))
    add("loss: src_imgs of 4 channels", lambda: L(_with(_loss_args(), 1, T(2, 2, 4, 16, 24))))
    add("loss: no sources", lambda: L(_with(_with(_loss_args(), 1, T(2, 0, 3, 16, 24)), 4, [])))
    add("loss: 9 sources", lambda: L(_loss_args(n=9)))
    add("loss: no scales", lambda: L(_with(_loss_args(), 3, [])))
    add("loss: 9 scales", lambda: L(_loss_args(H=1024, W=1024, S=9)))
    add("loss: intrinsics of one scale", lambda: L(_with(_loss_args(), 2, T(2, 1, 3, 3))))
    add("loss: intrinsics ndim", lambda: L(_with(_loss_args(), 2, T(2, 3, 3))))
    add("loss: intrinsics float16", lambda: L(_with(_loss_args(), 2, T(2, 2, 3, 3, dtype=torch.float16))))
    add("loss: pred_disps[1] of scale 0", lambda: L(_with(_loss_args(), 3, [T(2, 1, 16, 24), T(2, 1, 16, 24)])))
    add("loss: pred_disps[0] of 2 channels", lambda: L(_with(_loss_args(), 3, [T(2, 2, 16, 24), T(2, 1, 8, 12)])))
    add("loss: pred_disps[1] float64", lambda: L(_with(_loss_args(), 3, [T(2, 1, 16, 24), T(2, 1, 8, 12, **F64)])))
    add("loss: pred_disps[0] int32", lambda: L(_with(_loss_args(), 3, [T(2, 1, 16, 24, **I32), T(2, 1, 8, 12)])))
    add("loss: pred_disps[1] ndim", lambda: L(_with(_loss_args(), 3, [T(2, 1, 16, 24), T(2, 8, 12)])))
    add("loss: pred_disps[0] cpu", lambda: L(_with(_loss_args(), 3, [T(2, 1, 16, 24, **CPU), T(2, 1, 8, 12)])))
    add("loss: pred_disps[0] not a tensor", lambda: L(_with(_loss_args(), 3, [1.0, T(2, 1, 8, 12)])))
    add("loss: one pose short", lambda: L(_with(_loss_args(), 4, [T(2, 6)])))
    add("loss: pred_poses[1] (B,5)", lambda: L(_with(_loss_args(), 4, [T(2, 6), T(2, 5)])))
    add("loss: pred_poses[0] ndim", lambda: L(_with(_loss_args(), 4, [T(12), T(2, 6)])))
    add("loss: pred_poses[1] int32", lambda: L(_with(_loss_args(), 4, [T(2, 6), T(2, 6, **I32)])))
    add("loss: packed poses of 3 sources", lambda: L(_with(_loss_args(), 4, T(2, 18))))
    add("loss: packed poses ndim", lambda: L(_with(_loss_args(), 4, T(2, 2, 6))))
    add("loss: packed poses cpu", lambda: L(_with(_loss_args(), 4, T(2, 12, **CPU))))
    add("loss: exp_reg without masks", lambda: L(_loss_args(), exp_reg=0.2))
    add("loss: exp_reg with one mask short", lambda: L(_loss_args() + [[T(2, 2, 16, 24)]], exp_reg=0.2))
    add("loss: pred_maskes[1] of 1 source", lambda: L(_loss_args() + [[T(2, 2, 16, 24), T(2, 1, 8, 12)]], exp_reg=0.2))
    add("loss: pred_maskes[0] float64", lambda: L(_loss_args() + [[T(2, 2, 16, 24, **F64), T(2, 2, 8, 12)]], exp_reg=0.2))
    add("loss: pred_maskes[1] ndim", lambda: L(_loss_args() + [[T(2, 2, 16, 24), T(2, 2, 96)]], exp_reg=0.2))
    add("module: seq_len", lambda: ta.SFMLearnerLoss(dict(smooth_reg=0.1, exp_reg=0.0, seq_len=4))(*_loss_args()[:3], None, *_loss_args()[3:]))
    add("module: smooth_mode", lambda: ta.SFMLearnerLoss(dict(smooth_reg=0.1, exp_reg=0.0, seq_len=3), smooth_mode="x")(
        *_loss_args()[:3], None, *_loss_args()[3:]))

    # torch_api.scale_arrays_into, disp_activation; augment.augment_images
    sc = ta.scale_arrays_into
    add("scale_arrays_into: no arrays", lambda: sc([], [], T(1)))
    add("scale_arrays_into: 33 arrays", lambda: sc([T(4)] * 33, [T(4)] * 33, T(1)))
    add("scale_arrays_into: one output short", lambda: sc([T(4), T(4)], [T(4)], T(1)))
    add("scale_arrays_into: gy cpu", lambda: sc([T(4)], [T(4)], T(1, **CPU)))
    add("scale_arrays_into: gy float64", lambda: sc([T(4)], [T(4)], T(1, **F64)))
    add("scale_arrays_into: gy of 2 elements", lambda: sc([T(4)], [T(4)], T(2)))
    add("scale_arrays_into: gy not a tensor", lambda: sc([T(4)], [T(4)], 2.0))
    add("scale_arrays_into: xs[1] cpu", lambda: sc([T(4), T(4, **CPU)], [T(4), T(4)], T(())))
    add("scale_arrays_into: ys[0] float64", lambda: sc([T(4)], [T(4, **F64)], T(())))
    add("scale_arrays_into: xs[0] not contiguous", lambda: sc([T(4, 4).t()], [T(4, 4)], T(())))
    add("scale_arrays_into: ys[1] not contiguous", lambda: sc([T(4), T(4, 4)], [T(4), T(4, 4).t()], T(())))
    add("scale_arrays_into: sizes differ", lambda: sc([T(4), T(5)], [T(4), T(4)], T(())))
    add("disp_activation: cpu", lambda: ta.disp_activation([T(1, 1, 4, 4, dtype=torch.bfloat16, **CPU)]))
    add("disp_activation: int32", lambda: ta.disp_activation([T(1, 1, 4, 4), T(1, 1, 2, 2, **I32)]))
    add("disp_activation: float64", lambda: ta.disp_activation([T(1, 1, 4, 4, **F64)]))
    add("disp_activation: not a tensor", lambda: ta.disp_activation([3]))
    P = np.zeros((2, 7))
    add("augment_images: cpu", lambda: augment.augment_images(T(2, 3, 3, 8, 8, **CPU), P))
    add("augment_images: ndim 4", lambda: augment.augment_images(T(2, 9, 8, 8), P))
    add("augment_images: float16", lambda: augment.augment_images(T(2, 3, 3, 8, 8, dtype=torch.float16), P))
    add("augment_images: not a tensor", lambda: augment.augment_images(np.zeros((2, 3, 3, 8, 8), np.float32), P))
    return out + _newer_cases()


def _newer_cases():
    """The refusals of the entry points added after the table was first written (rows are only ever appended)"""
    out = []
    add = lambda label, fn: out.append((label, fn))
    F64, I32, F16, CPU, DEV1 = dict(dtype=torch.float64), dict(dtype=torch.int32), dict(dtype=torch.float16), dict(device="cpu"), \
        dict(device="cuda:1")

    # torch_api.warp_pyramid(src_imgs, intrinsics, pred_disps, pred_poses): the inputs of the loss without tgt_img
    def wp(a, **kw):
        return ta.warp_pyramid(*a[1:], **kw)
    A = _loss_args
    add("warp_pyramid: cpu", lambda: wp(A(device="cpu")))
    add("warp_pyramid: src_imgs not a tensor", lambda: wp(_with(A(), 1, None)))
    add("warp_pyramid: src_imgs stacked", lambda: wp(_with(A(), 1, T(2, 6, 16, 24))))
    add("warp_pyramid: src_imgs float64", lambda: wp(_with(A(), 1, T(2, 2, 3, 16, 24, **F64))))
    add("warp_pyramid: src_imgs of 4 channels", lambda: wp(_with(A(), 1, T(2, 2, 4, 16, 24))))
    add("warp_pyramid: src_imgs of 4 channels, 9 scales", lambda: wp(_with(A(H=1024, W=1024, S=9), 1, T(2, 2, 4, 1024, 1024))))
    add("warp_pyramid: no sources", lambda: wp(_with(_with(A(), 1, T(2, 0, 3, 16, 24)), 4, [])))
    add("warp_pyramid: 8 sources, one pose short", lambda: wp(_with(A(n=8), 4, [T(2, 6)] * 7)))
    add("warp_pyramid: 9 sources", lambda: wp(A(n=9)))
    add("warp_pyramid: 9 sources, no scales", lambda: wp(_with(A(n=9), 3, [])))
    add("warp_pyramid: no scales", lambda: wp(_with(A(), 3, [])))
    add("warp_pyramid: 9 scales", lambda: wp(A(H=1024, W=1024, S=9)))
    add("warp_pyramid: 9 scales, intrinsics cpu", lambda: wp(_with(A(H=1024, W=1024, S=9), 2, T(2, 9, 3, 3, **CPU))))
    add("warp_pyramid: intrinsics cpu", lambda: wp(_with(A(), 2, T(2, 2, 3, 3, **CPU))))
    add("warp_pyramid: intrinsics of one scale", lambda: wp(_with(A(), 2, T(2, 1, 3, 3))))
    add("warp_pyramid: intrinsics of another B", lambda: wp(_with(A(), 2, T(1, 2, 3, 3))))
    add("warp_pyramid: intrinsics ndim", lambda: wp(_with(A(), 2, T(2, 3, 3))))
    add("warp_pyramid: intrinsics float16", lambda: wp(_with(A(), 2, T(2, 2, 3, 3, **F16))))
    add("warp_pyramid: intrinsics require grad", lambda: wp(_with(A(), 2, T(2, 2, 3, 3).requires_grad_())))
    add("warp_pyramid: intrinsics of one scale require grad", lambda: wp(_with(A(), 2, T(2, 1, 3, 3).requires_grad_())))
    add("warp_pyramid: intrinsics require grad, pred_disps[0] cpu",
        lambda: wp(_with(_with(A(), 2, T(2, 2, 3, 3).requires_grad_()), 3, [T(2, 1, 16, 24, **CPU), T(2, 1, 8, 12)])))
    add("warp_pyramid: pred_disps[1] of scale 0", lambda: wp(_with(A(), 3, [T(2, 1, 16, 24), T(2, 1, 16, 24)])))
    add("warp_pyramid: pred_disps[0] of 2 channels", lambda: wp(_with(A(), 3, [T(2, 2, 16, 24), T(2, 1, 8, 12)])))
    add("warp_pyramid: pred_disps[1] float64", lambda: wp(_with(A(), 3, [T(2, 1, 16, 24), T(2, 1, 8, 12, **F64)])))
    add("warp_pyramid: pred_disps[1] ndim", lambda: wp(_with(A(), 3, [T(2, 1, 16, 24), T(2, 8, 12)])))
    add("warp_pyramid: pred_disps[0] cpu", lambda: wp(_with(A(), 3, [T(2, 1, 16, 24, **CPU), T(2, 1, 8, 12)])))
    add("warp_pyramid: pred_disps[0] not a tensor", lambda: wp(_with(A(), 3, [1.0, T(2, 1, 8, 12)])))
    add("warp_pyramid: pred_disps[1] of scale 0, one pose short", lambda: wp(_with(_with(A(), 3, [T(2, 1, 16, 24)] * 2), 4, [T(2, 6)])))
    add("warp_pyramid: one pose short", lambda: wp(_with(A(), 4, [T(2, 6)])))
    add("warp_pyramid: pred_poses[1] (B,5)", lambda: wp(_with(A(), 4, [T(2, 6), T(2, 5)])))
    add("warp_pyramid: pred_poses[0] ndim", lambda: wp(_with(A(), 4, [T(12), T(2, 6)])))
    add("warp_pyramid: pred_poses[1] int32", lambda: wp(_with(A(), 4, [T(2, 6), T(2, 6, **I32)])))
    add("warp_pyramid: packed poses of 3 sources", lambda: wp(_with(A(), 4, T(2, 18))))
    add("warp_pyramid: packed poses ndim", lambda: wp(_with(A(), 4, T(2, 2, 6))))
    add("warp_pyramid: packed poses cpu", lambda: wp(_with(A(), 4, T(2, 12, **CPU))))
    add("warp_pyramid: intrinsics on another device", lambda: wp(_with(A(), 2, T(2, 2, 3, 3, **DEV1))))
    add("warp_pyramid: pred_disps[1] on another device", lambda: wp(_with(A(), 3, [T(2, 1, 16, 24), T(2, 1, 8, 12, **DEV1)])))
    add("warp_pyramid: pred_poses[0] on another device", lambda: wp(_with(A(), 4, [T(2, 6, **DEV1), T(2, 6)])))
    add("warp_pyramid: pred_poses[1] (B,5), intrinsics on another device",
        lambda: wp(_with(_with(A(), 2, T(2, 2, 3, 3, **DEV1)), 4, [T(2, 6), T(2, 5)])))
    # ... and the order of the same checks inside the loss, where the masks come before the device
    L = lambda a, **kw: ta.sfm_learner_loss(*a, **dict(dict(smooth_reg=0.1), **kw))
    add("loss: intrinsics on another device", lambda: L(_with(A(), 2, T(2, 2, 3, 3, **DEV1))))
    add("loss: pred_disps[0] on another device", lambda: L(_with(A(), 3, [T(2, 1, 16, 24, **DEV1), T(2, 1, 8, 12)])))
    add("loss: pred_poses[1] on another device", lambda: L(_with(A(), 4, [T(2, 6), T(2, 6, **DEV1)])))
    add("loss: pred_maskes[1] on another device", lambda: L(A() + [[T(2, 2, 16, 24), T(2, 2, 8, 12, **DEV1)]], exp_reg=0.2))
    add("loss: intrinsics on another device, pred_maskes[1] of 1 source",
        lambda: L(_with(A(), 2, T(2, 2, 3, 3, **DEV1)) + [[T(2, 2, 16, 24), T(2, 1, 8, 12)]], exp_reg=0.2))
    add("loss: intrinsics on another device, exp_reg without masks", lambda: L(_with(A(), 2, T(2, 2, 3, 3, **DEV1)), exp_reg=0.2))
    add("loss: src_imgs of 4 channels, 9 scales", lambda: L(_with(A(H=1024, W=1024, S=9), 1, T(2, 2, 4, 1024, 1024))))
    add("loss: 9 sources, no scales", lambda: L(_with(A(n=9), 3, [])))
    add("loss: 9 scales, intrinsics cpu", lambda: L(_with(A(H=1024, W=1024, S=9), 2, T(2, 9, 3, 3, **CPU))))
    add("loss: intrinsics of one scale, pred_disps[0] cpu", lambda: L(_with(_with(A(), 2, T(2, 1, 3, 3)), 3, [T(2, 1, 16, 24, **CPU), T(2, 1, 8, 12)])))
    add("loss: pred_disps[1] of scale 0, one pose short", lambda: L(_with(_with(A(), 3, [T(2, 1, 16, 24)] * 2), 4, [T(2, 6)])))
    add("loss: one pose short, exp_reg without masks", lambda: L(_with(A(), 4, [T(2, 6)]), exp_reg=0.2))

    # torch_api.photometric_error(imgs, tgt, ssim_rate=): a single tgt is turned into its pyramid by a launch, so only what is
    # checked before that is reachable; a list of targets reaches every check
    pe = lambda imgs, tgt: ta.photometric_error(imgs, tgt, ssim_rate=0.15)
    X = lambda B=2, n=2, H=16, W=24, S=2, **kw: [T(B, n, 3, H >> s, W >> s, **kw) for s in range(S)]
    Y = lambda B=2, H=16, W=24, S=2, **kw: [T(B, 3, H >> s, W >> s, **kw) for s in range(S)]
    add("photometric_error: imgs a tensor", lambda: pe(T(2, 2, 3, 16, 24), Y()))
    add("photometric_error: no scales", lambda: pe([], []))
    add("photometric_error: 9 scales", lambda: pe(X(H=1024, W=1024, S=9), Y(H=1024, W=1024, S=9)))
    add("photometric_error: imgs[0] cpu", lambda: pe(X(**CPU), Y()))
    add("photometric_error: imgs[1] float64", lambda: pe([X()[0], T(2, 2, 3, 8, 12, **F64)], Y()))
    add("photometric_error: imgs[1] int32", lambda: pe([X()[0], T(2, 2, 3, 8, 12, **I32)], Y()))
    add("photometric_error: imgs[0] ndim", lambda: pe([T(2, 6, 16, 24), X()[1]], Y()))
    add("photometric_error: imgs[0] not a tensor", lambda: pe([None, X()[1]], Y()))
    add("photometric_error: imgs[0] of 4 channels", lambda: pe([T(2, 2, 4, 16, 24), X()[1]], Y()))
    add("photometric_error: imgs[1] of another B", lambda: pe([X()[0], T(1, 2, 3, 8, 12)], Y()))
    add("photometric_error: imgs[1] of another n", lambda: pe([X()[0], T(2, 3, 3, 8, 12)], Y()))
    add("photometric_error: no images", lambda: pe(X(n=0), Y()))
    add("photometric_error: 9 images", lambda: pe(X(n=9), Y()))
    add("photometric_error: 9 images, one tgt short", lambda: pe(X(n=9), Y()[:1]))
    add("photometric_error: one tgt short", lambda: pe(X(), Y()[:1]))
    add("photometric_error: tgt[1] cpu", lambda: pe(X(), [Y()[0], T(2, 3, 8, 12, **CPU)]))
    add("photometric_error: tgt[0] float64", lambda: pe(X(), [T(2, 3, 16, 24, **F64), Y()[1]]))
    add("photometric_error: tgt[1] ndim", lambda: pe(X(), [Y()[0], T(2, 1, 3, 8, 12)]))
    add("photometric_error: tgt[1] of scale 0", lambda: pe(X(), [Y()[0], Y()[0]]))
    add("photometric_error: tgt[0] of another B", lambda: pe(X(), [T(1, 3, 16, 24), Y()[1]]))
    add("photometric_error: tgt[0] of 1 channel", lambda: pe(X(), [T(2, 1, 16, 24), Y()[1]]))
    add("photometric_error: imgs[1] on another device", lambda: pe([X()[0], T(2, 2, 3, 8, 12, **DEV1)], Y()))
    add("photometric_error: tgt[0] on another device", lambda: pe(X(), [T(2, 3, 16, 24, **DEV1), Y()[1]]))
    add("photometric_error: tgt[0] of 1 channel, tgt[1] on another device", lambda: pe(X(), [T(2, 1, 16, 24), T(2, 3, 8, 12, **DEV1)]))
    add("photometric_error: single tgt cpu", lambda: pe(X(), T(2, 3, 16, 24, **CPU)))
    add("photometric_error: single tgt ndim", lambda: pe(X(), T(3, 16, 24)))
    add("photometric_error: single tgt float16", lambda: pe(X(), T(2, 3, 16, 24, **F16)))
    add("photometric_error: single tgt of another frame", lambda: pe(X(), T(2, 3, 16, 22)))
    add("photometric_error: single tgt, imgs[1] of scale 0", lambda: pe([X()[0], X()[0]], T(2, 3, 16, 24)))
    add("photometric_error: single tgt of another B", lambda: pe(X(), T(1, 3, 16, 24)))
    add("photometric_error: single tgt of 1 channel", lambda: pe(X(), T(2, 1, 16, 24)))
    add("photometric_error: single tgt of another frame and B", lambda: pe(X(), T(1, 3, 16, 22)))

    # ops.warp_pyramid_fwd / _bwd(src_pyr, disps, poses, K, layout[, g_warped]): the descriptor builder they share (g_warped is
    # looked at after the first data_ptr())
    def P(B=2, H=16, W=24, S=2, n=2, hwc=False):
        a = _bind_args(B, H, W, S, n, hwc)
        return [a[1], a[3], a[4], a[2], "hwc" if hwc else "planar"]
    for name, fn in (("warp_pyramid_fwd", ops.warp_pyramid_fwd), ("warp_pyramid_bwd", lambda *a: ops.warp_pyramid_bwd(*a, [None, None]))):
        c = lambda label, thunk, name=name: add("%s: %s" % (name, label), thunk)
        c("layout", lambda fn=fn: fn(*_with(P(), 4, "nhwc")))
        c("layout None, no scales", lambda fn=fn: fn([], [], P()[2], P()[3], None))
        c("one src scale short", lambda fn=fn: fn(*_with(P(), 0, P()[0][:1])))
        c("no scales", lambda fn=fn: fn([], [], P()[2], P()[3], "planar"))
        c("9 scales", lambda fn=fn: fn(*P(H=1024, W=1024, S=9)))
        c("no sources", lambda fn=fn: fn(*_with(P(), 2, [])))
        c("9 sources", lambda fn=fn: fn(*P(n=9)))
        c("8 sources, 8 scales, src_pyr[7] cpu", lambda fn=fn: fn(*_with(P(H=512, W=512, S=8, n=8), 0, P(H=512, W=512, S=8, n=8)[0][:7] + [T(2, 24, 4, 4, **CPU)])))
        c("src_pyr[1] cpu", lambda fn=fn: fn(*_with(P(), 0, [T(2, 6, 16, 24), T(2, 6, 8, 12, **CPU)])))
        c("src_pyr[0] float64", lambda fn=fn: fn(*_with(P(), 0, [T(2, 6, 16, 24, **F64), T(2, 6, 8, 12)])))
        c("src_pyr planar under hwc", lambda fn=fn: fn(*_with(P(), 4, "hwc")))
        c("src_pyr hwc under planar", lambda fn=fn: fn(*_with(P(hwc=True), 4, "planar")))
        c("disps[1] ndim", lambda fn=fn: fn(*_with(P(), 1, [T(2, 1, 16, 24), T(2, 8, 12)])))
        c("disps[0] not a tensor", lambda fn=fn: fn(*_with(P(), 1, [None, T(2, 1, 8, 12)])))
        c("poses[1] ndim", lambda fn=fn: fn(*_with(P(), 2, [T(2, 6), T(12)])))
        c("poses[0] cpu", lambda fn=fn: fn(*_with(P(), 2, [T(2, 6, **CPU), T(2, 6)])))
        c("poses[0] cpu, intrinsics ndim", lambda fn=fn: fn(*_with(_with(P(), 2, [T(2, 6, **CPU), T(2, 6)]), 3, T(2, 3, 3))))
        c("intrinsics ndim", lambda fn=fn: fn(*_with(P(), 3, T(2, 3, 3))))
        c("intrinsics cpu", lambda fn=fn: fn(*_with(P(), 3, T(2, 2, 3, 3, **CPU))))
        c("intrinsics float64", lambda fn=fn: fn(*_with(P(), 3, T(2, 2, 3, 3, **F64))))
        c("intrinsics of one scale", lambda fn=fn: fn(*_with(P(), 3, T(2, 1, 3, 3))))
        c("intrinsics of another B", lambda fn=fn: fn(*_with(P(), 3, T(1, 2, 3, 3))))
        c("intrinsics of another B, src_pyr[0] of 3 sources", lambda fn=fn: fn(*_with(_with(P(), 3, T(1, 2, 3, 3)), 0, [T(2, 9, 16, 24), T(2, 6, 8, 12)])))
        c("src_pyr[0] of 3 sources", lambda fn=fn: fn(*_with(P(), 0, [T(2, 9, 16, 24), T(2, 6, 8, 12)])))
        c("src_pyr[1] of another frame", lambda fn=fn: fn(*_with(P(), 0, [T(2, 6, 16, 24), T(2, 6, 8, 11)])))
        c("src_pyr[1] of another frame, hwc", lambda fn=fn: fn(*_with(P(hwc=True), 0, [T(2, 2, 16, 24, 3), T(2, 2, 8, 11, 3)])))
        c("disps[0] of 2 channels", lambda fn=fn: fn(*_with(P(), 1, [T(2, 2, 16, 24), T(2, 1, 8, 12)])))
        c("disps[1] of another B", lambda fn=fn: fn(*_with(P(), 1, [T(2, 1, 16, 24), T(1, 1, 8, 12)])))
        c("disps[1] of another B, poses[0] (B,5)", lambda fn=fn: fn(*_with(_with(P(), 1, [T(2, 1, 16, 24), T(1, 1, 8, 12)]), 2, [T(2, 5), T(2, 6)])))
        c("poses[1] (B,5)", lambda fn=fn: fn(*_with(P(), 2, [T(2, 6), T(2, 5)])))
        c("poses[0] of another B", lambda fn=fn: fn(*_with(P(), 2, [T(1, 6), T(2, 6)])))
        c("poses[1] (B,5), src_pyr[1] on another device", lambda fn=fn: fn(*_with(_with(P(), 2, [T(2, 6), T(2, 5)]), 0, [T(2, 6, 16, 24), T(2, 6, 8, 12, **DEV1)])))
        c("src_pyr[1] on another device", lambda fn=fn: fn(*_with(P(), 0, [T(2, 6, 16, 24), T(2, 6, 8, 12, **DEV1)])))
        c("disps[0] on another device", lambda fn=fn: fn(*_with(P(), 1, [T(2, 1, 16, 24, **DEV1), T(2, 1, 8, 12)])))
        c("poses[1] on another device", lambda fn=fn: fn(*_with(P(), 2, [T(2, 6), T(2, 6, **DEV1)])))
        c("intrinsics on another device", lambda fn=fn: fn(*_with(P(), 3, T(2, 2, 3, 3, **DEV1))))

    # ops.photo_error_fwd / _bwd(imgs, tgts, ssim_rate[, g_err]): likewise
    for name, fn in (("photo_error_fwd", lambda i, t: ops.photo_error_fwd(i, t, 0.15)), ("photo_error_bwd", lambda i, t: ops.photo_error_bwd(i, t, 0.15, [None, None]))):
        c = lambda label, thunk, name=name: add("%s: %s" % (name, label), thunk)
        c("imgs a tensor", lambda fn=fn: fn(T(2, 2, 3, 16, 24), Y()))
        c("tgts a tensor", lambda fn=fn: fn(X(), T(2, 3, 16, 24)))
        c("tgts a tensor, no scales", lambda fn=fn: fn([], T(2, 3, 16, 24)))
        c("one tgt short", lambda fn=fn: fn(X(), Y()[:1]))
        c("no scales", lambda fn=fn: fn([], []))
        c("9 scales", lambda fn=fn: fn(X(H=1024, W=1024, S=9), Y(H=1024, W=1024, S=9)))
        c("9 scales, 8 tgts", lambda fn=fn: fn(X(H=1024, W=1024, S=9), Y(H=1024, W=1024, S=8)))
        c("8 scales, 8 images, tgts[7] cpu", lambda fn=fn: fn(X(H=512, W=512, S=8, n=8), Y(H=512, W=512, S=7) + [T(2, 3, 4, 4, **CPU)]))
        c("imgs[1] cpu", lambda fn=fn: fn([X()[0], T(2, 2, 3, 8, 12, **CPU)], Y()))
        c("imgs[0] float16", lambda fn=fn: fn([T(2, 2, 3, 16, 24, **F16), X()[1]], Y()))
        c("imgs[0] ndim", lambda fn=fn: fn([T(2, 6, 16, 24), X()[1]], Y()))
        c("imgs[1] not a tensor", lambda fn=fn: fn([X()[0], None], Y()))
        c("tgts[0] float64", lambda fn=fn: fn(X(), [T(2, 3, 16, 24, **F64), Y()[1]]))
        c("tgts[1] ndim", lambda fn=fn: fn(X(), [Y()[0], T(2, 1, 3, 8, 12)]))
        c("imgs[1] cpu, tgts[0] ndim", lambda fn=fn: fn([X()[0], T(2, 2, 3, 8, 12, **CPU)], [T(6, 16, 24), Y()[1]]))
        c("no images", lambda fn=fn: fn(X(n=0), Y()))
        c("9 images", lambda fn=fn: fn(X(n=9), Y()))
        c("9 images, tgts[0] of another B", lambda fn=fn: fn(X(n=9), [T(1, 3, 16, 24), Y()[1]]))
        c("imgs[0] of 4 channels", lambda fn=fn: fn([T(2, 2, 4, 16, 24), X()[1]], Y()))
        c("imgs[1] of another B", lambda fn=fn: fn([X()[0], T(1, 2, 3, 8, 12)], Y()))
        c("imgs[1] of another n", lambda fn=fn: fn([X()[0], T(2, 3, 3, 8, 12)], Y()))
        c("tgts[1] of scale 0", lambda fn=fn: fn(X(), [Y()[0], Y()[0]]))
        c("tgts[0] of another B", lambda fn=fn: fn(X(), [T(1, 3, 16, 24), Y()[1]]))
        c("tgts[0] of 1 channel", lambda fn=fn: fn(X(), [T(2, 1, 16, 24), Y()[1]]))
        c("tgts[0] of 1 channel, imgs[1] on another device", lambda fn=fn: fn([X()[0], T(2, 2, 3, 8, 12, **DEV1)], [T(2, 1, 16, 24), Y()[1]]))
        c("imgs[1] on another device", lambda fn=fn: fn([X()[0], T(2, 2, 3, 8, 12, **DEV1)], Y()))
        c("tgts[0] on another device", lambda fn=fn: fn(X(), [T(2, 3, 16, 24, **DEV1), Y()[1]]))

    # ops.resize_bwd(gys, in_hw)
    rb = lambda gys: ops.resize_bwd(gys, (16, 24))
    add("resize_bwd: no arrays", lambda: rb([]))
    add("resize_bwd: 9 arrays", lambda: rb([T(1, 3, 8, 8)] * 9))
    add("resize_bwd: 9 arrays on the cpu", lambda: rb([T(1, 3, 8, 8, **CPU)] * 9))
    add("resize_bwd: 8 arrays, the last on the cpu", lambda: rb([T(1, 3, 8, 8)] * 7 + [T(1, 3, 8, 8, **CPU)]))
    add("resize_bwd: one array, cpu", lambda: rb(T(1, 3, 8, 8, **CPU)))
    add("resize_bwd: one array, ndim", lambda: rb(T(3, 8, 8)))
    add("resize_bwd: not a tensor", lambda: rb([None]))
    add("resize_bwd: gys[1] float64", lambda: rb([T(1, 3, 8, 8), T(1, 3, 4, 4, **F64)]))
    add("resize_bwd: gys[1] bfloat16", lambda: rb([T(1, 3, 8, 8), T(1, 3, 4, 4, dtype=torch.bfloat16)]))
    add("resize_bwd: gys[0] ndim", lambda: rb([T(3, 8, 8), T(1, 3, 4, 4)]))
    add("resize_bwd: gys[1] of another N", lambda: rb([T(1, 3, 8, 8), T(2, 3, 4, 4)]))
    add("resize_bwd: gys[2] of another C", lambda: rb([T(1, 3, 8, 8), T(1, 3, 4, 4), T(1, 1, 2, 2)]))
    add("resize_bwd: gys[1] on another device", lambda: rb([T(1, 3, 8, 8), T(1, 3, 4, 4, **DEV1)]))
    add("resize_bwd: gys[1] of another N, gys[2] on another device", lambda: rb([T(1, 3, 8, 8), T(2, 3, 4, 4), T(1, 3, 4, 4, **DEV1)]))

    # ops.warp_bwd_intrinsics(imgs, depth, pose6, K, g_warped): warp_bwd's arguments and checks
    w = lambda imgs=None, depth=None, pose=None, K=None: [T(2, 3, 8, 8) if imgs is None else imgs, T(2, 64) if depth is None else depth,
                                                          T(2, 6) if pose is None else pose, T(2, 3, 3) if K is None else K]
    wk = lambda a, g=None: ops.warp_bwd_intrinsics(*a, T(2, 3, 8, 8) if g is None else g)
    add("warp_bwd_intrinsics: imgs cpu", lambda: wk(w(imgs=T(2, 3, 8, 8, **CPU))))
    add("warp_bwd_intrinsics: imgs ndim 3", lambda: wk(w(imgs=T(3, 8, 8))))
    add("warp_bwd_intrinsics: imgs float64", lambda: wk(w(imgs=T(2, 3, 8, 8, **F64))))
    add("warp_bwd_intrinsics: depth float64", lambda: wk(w(depth=T(2, 64, **F64))))
    add("warp_bwd_intrinsics: depth cpu", lambda: wk(w(depth=T(2, 64, **CPU))))
    add("warp_bwd_intrinsics: depth of 2 rows", lambda: wk(w(depth=T(2, 2, 64))))
    add("warp_bwd_intrinsics: depth of another frame", lambda: wk(w(depth=T(2, 63))))
    add("warp_bwd_intrinsics: depth of another frame, poses ndim", lambda: wk(w(depth=T(2, 63), pose=T(12))))
    add("warp_bwd_intrinsics: poses ndim", lambda: wk(w(pose=T(12))))
    add("warp_bwd_intrinsics: poses (N,5)", lambda: wk(w(pose=T(2, 5))))
    add("warp_bwd_intrinsics: poses (N,5), K cpu", lambda: wk(w(pose=T(2, 5), K=T(2, 3, 3, **CPU))))
    add("warp_bwd_intrinsics: K of another N", lambda: wk(w(K=T(1, 3, 3))))
    add("warp_bwd_intrinsics: K ndim", lambda: wk(w(K=T(2, 9))))
    add("warp_bwd_intrinsics: K of another N, g_warped cpu", lambda: wk(w(K=T(1, 3, 3)), T(2, 3, 8, 8, **CPU)))
    add("warp_bwd_intrinsics: g_warped of another shape", lambda: wk(w(), T(2, 3, 8, 7)))
    add("warp_bwd_intrinsics: g_warped ndim", lambda: wk(w(), T(2, 3, 64)))
    add("warp_bwd_intrinsics: g_warped cpu", lambda: wk(w(), T(2, 3, 8, 8, **CPU)))
    add("warp_bwd_intrinsics: g_warped float64", lambda: wk(w(depth=T(2, 3, 64)), T(2, 3, 8, 8, **F64)))

    # ops.pose_proj_bwd_intrinsics(pose6, K, g_proj)
    pk = ops.pose_proj_bwd_intrinsics
    add("pose_proj_bwd_intrinsics: pose6 ndim", lambda: pk(T(12), T(2, 3, 3), T(2, 4, 4)))
    add("pose_proj_bwd_intrinsics: pose6 cpu", lambda: pk(T(2, 6, **CPU), T(2, 3, 3), T(2, 4, 4)))
    add("pose_proj_bwd_intrinsics: K cpu", lambda: pk(T(2, 6), T(2, 3, 3, **CPU), T(2, 4, 4)))
    add("pose_proj_bwd_intrinsics: K ndim", lambda: pk(T(2, 6), T(2, 9), T(2, 4, 4)))
    add("pose_proj_bwd_intrinsics: K float64, g_proj cpu", lambda: pk(T(2, 6), T(2, 3, 3, **F64), T(2, 4, 4, **CPU)))
    add("pose_proj_bwd_intrinsics: g_proj ndim", lambda: pk(T(2, 6), T(2, 3, 3), T(2, 16)))
    add("pose_proj_bwd_intrinsics: g_proj int32", lambda: pk(T(2, 6), T(2, 3, 3), T(2, 4, 4, **I32)))
    add("pose_proj_bwd_intrinsics: pose6 (N,5)", lambda: pk(T(2, 5), T(2, 3, 3), T(2, 4, 4)))
    add("pose_proj_bwd_intrinsics: K of another N", lambda: pk(T(2, 6), T(3, 3, 3), T(2, 4, 4)))
    add("pose_proj_bwd_intrinsics: K (N,3,4)", lambda: pk(T(2, 6), T(2, 3, 4), T(2, 4, 4)))
    add("pose_proj_bwd_intrinsics: g_proj (N,3,4)", lambda: pk(T(2, 6), T(2, 3, 3), T(2, 3, 4)))
    add("pose_proj_bwd_intrinsics: g_proj of another N", lambda: pk(T(2, 6), T(2, 3, 3), T(1, 4, 4)))
    return out


def refusal(fn):
    """[exception class, message] of a case; a case that raises nothing, or trips over a fake tensor instead of a check, is a
    mistake in the table"""
    with FakeTensorMode():
        try:
            fn()
        except (TypeError, ValueError) as e:
            return [type(e).__name__, str(e)]
    raise AssertionError("not refused")


def rejects():
    labels = [label for label, _ in cases()]
    assert len(set(labels)) == len(labels), "labels repeat"
    return [[label] + refusal(fn) for label, fn in cases()]


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    t = plan_tables()
    path = os.path.join(out_dir, "host_plans.npz")
    np.savez_compressed(path, **t)
    print("%d configurations (%d refused by the library, %d pixel-interleaved), %d bytes" % (
        len(t["params"]), int((t["error"] != "").sum()), int(t["hwc"].sum()), os.path.getsize(path)))
    r = rejects()
    path = os.path.join(out_dir, "host_rejects.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in r) + "\n]\n")
    print("%d refusals, %d bytes" % (len(r), os.path.getsize(path)))
