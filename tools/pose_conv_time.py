#!/usr/bin/env python3
"""Timing of the pose and depth conventions of include/sfmwarp_pose.h with HIP events, at the cells of profiles/conventions_time.txt:
128 x 416, 4 scales, 2 sources, B = 4 and B = 32.

  1. default   ops.warp_pyramid_fwd / _bwd, ops.warp_full_res_fwd / _bwd and torch_api.min_reprojection_loss(full_res=True,
               smooth_weight=1e-3) WITHOUT the new arguments against the same calls in the parent commit's library: that path is to be
               the same kernels.  `--parent PATH` names that build's libsfmwarp.so (loaded with the tables of the symbols it has and
               swapped in under ops for its turns, as tools/conventions_time.py does).  The rule of profiles/conventions_time.txt: this
               build's median <= the parent's median + the parent's spread (p90 - p10); a miss is printed as MISS.  Without --parent
               this part is skipped and says so.
  2. modes     Monodepth2's objective as ONE node -- min_reprojection_loss(full_res=True, ssim_padding="reflect",
               upsample="half_pixel", pose_format="axis_angle", invert=[True, False], depth_range=(0.1, 100)) -- against the same
               objective with the two conventions written in aten in front of the call: the Rodrigues formula and the inversion as
               torch operations feeding pose_format="matrix", a * disp + b as a torch operation feeding the disparities, and, because
               the one list of disparities then no longer is the raw one, the smoothness term as a second node
               (disparity_smoothness on the raw disparities); and against the same call WITHOUT the three arguments (Euler, 1 / disp) on
               the same tensors, which is what the arguments themselves cost.  No bar: all are recorded.

Each forward alone and forward + backward.  The two routes of a cell alternate launch by launch in one process.  Per cell: --warmup
steps of each (default 20), then --launches timed ones (default 200), each between its own pair of events; median, p10 and p90 in
microseconds; `train` is the same number of steps between ONE pair of events, per step.

usage: python tools/pose_conv_time.py [--parent PATH] [--warmup 20] [--launches 200] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resize_bwd_time import time_alternating  # noqa: E402

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

H, W, S, N_SRC = 128, 416, 4, 2
ALPHA, SMOOTH = 0.85, 1e-3
DEPTH_RANGE = (0.1, 100.0)
INVERT = [True, False]
MONODEPTH2 = dict(full_res=True, ssim_padding="reflect", upsample="half_pixel")


def load_parent(path):
    """the parent build bound with the binding's tables, without the symbols it does not have"""
    lib = C.CDLL(path)
    for table in (_lib.SYMBOLS, _lib.EXT_SYMBOLS, _lib.SMOOTH_SYMBOLS, _lib.FULL_RES_SYMBOLS, _lib.CONV_SYMBOLS):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.sfm_abi_version() == _lib.SFM_ABI_VERSION
    return lib


def with_library(lib, fn):
    """fn with `lib` under ops for the duration of the call"""
    def run(*args):
        keep, ops.lib = ops.lib, lib
        try:
            return fn(*args)
        finally:
            ops.lib = keep
    return run


def rodrigues(a):
    """Monodepth2's rot_from_axisangle in aten: (B,3) -> (B,3,3)"""
    angle = torch.norm(a, 2, 1, True)
    axis = a / (angle + 1e-7)
    ca, sa = torch.cos(angle)[:, 0], torch.sin(angle)[:, 0]
    Cc = 1 - ca
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    xs, ys, zs, xC, yC, zC = x * sa, y * sa, z * sa, x * Cc, y * Cc, z * Cc
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    return torch.stack([x * xC + ca, xyC - zs, zxC + ys, xyC + zs, y * yC + ca, yzC - xs, zxC - ys, yzC + xs, z * zC + ca], 1).view(-1, 3, 3)


def transformation_from_parameters(pose6, invert):
    """Monodepth2's function of that name, rows 0..2: (B,6) -> (B,3,4)"""
    R, t = rodrigues(pose6[:, :3]), pose6[:, 3:, None]
    if invert:
        R = R.transpose(1, 2)
        t = -(R @ t)
    return torch.cat([R, t], 2)


def workloads(B, dev):
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_SRC, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    tgt, src, K, K0 = t(d["tgt"]), t(d["src"]), t(d["intrinsics"]), t(d["intrinsics"][:, 0])
    disps, poses = [t(a).requires_grad_() for a in d["disps"]], [(t(a) * 0.1).requires_grad_() for a in d["poses"]]
    # a sigmoid's output for the depth range: the synthetic disparities squashed into (0, 1)
    units = [(x.detach() / (1 + x.detach())).requires_grad_() for x in disps]
    leaves = disps + poses + units
    raw_d, raw_p = [x.detach() for x in disps], [x.detach() for x in poses]
    gen = torch.Generator().manual_seed(3)
    g = [torch.randn((B, N_SRC, 3, H >> s, W >> s), generator=gen).to(dev) for s in range(S)]
    g_full = [torch.randn((B, N_SRC, 3, H, W), generator=gen).to(dev) for _ in range(S)]
    stacked = src.view(B, 3 * N_SRC, H, W)
    pyr, hwc = ops.pyramid_hwc(stacked, S), ops.pyramid_hwc(stacked, 1)[0]
    a_, b_ = 1.0 / DEPTH_RANGE[0] - 1.0 / DEPTH_RANGE[1], 1.0 / DEPTH_RANGE[1]

    def clear():
        for x in leaves:
            x.grad = None

    def warp_pyramid(grad):
        ops.warp_pyramid_fwd(pyr, raw_d, raw_p, K, "hwc")
        if grad:
            ops.warp_pyramid_bwd(pyr, raw_d, raw_p, K, "hwc", g)

    def warp_full_res(grad):
        ops.warp_full_res_fwd(hwc, raw_d, raw_p, K0, "hwc")
        if grad:
            ops.warp_full_res_bwd(hwc, raw_d, raw_p, K0, "hwc", g_full)

    def composite(grad):
        clear()
        with torch.set_grad_enabled(grad):
            total = ta.min_reprojection_loss(tgt, src, K0, disps, poses, ssim_rate=ALPHA, smooth_weight=SMOOTH, full_res=True)
        if grad:
            total.backward()

    def one_node(grad):
        clear()
        with torch.set_grad_enabled(grad):
            total = ta.min_reprojection_loss(tgt, src, K0, units, poses, ssim_rate=ALPHA, smooth_weight=SMOOTH, pose_format="axis_angle",
                                             invert=INVERT, depth_range=DEPTH_RANGE, **MONODEPTH2)
        if grad:
            total.backward()

    def aten_in_front(grad):
        clear()
        with torch.set_grad_enabled(grad):
            Ts = [transformation_from_parameters(p, inv) for p, inv in zip(poses, INVERT)]
            scaled = [a_ * x + b_ for x in units]
            total = ta.min_reprojection_loss(tgt, src, K0, scaled, Ts, ssim_rate=ALPHA, pose_format="matrix", **MONODEPTH2)
            total = total + SMOOTH * ta.disparity_smoothness(units, tgt)[0]
        if grad:
            total.backward()

    def without(grad):
        clear()
        with torch.set_grad_enabled(grad):
            total = ta.min_reprojection_loss(tgt, src, K0, units, poses, ssim_rate=ALPHA, smooth_weight=SMOOTH, **MONODEPTH2)
        if grad:
            total.backward()

    return {"warp_pyramid": warp_pyramid, "warp_full_res": warp_full_res, "composite": composite}, (one_node, aten_in_front, without)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per cell")
    if not torch.cuda.is_available():
        sys.exit("pose_conv_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    parent = load_parent(a.parent) if a.parent else None
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("the conventions of include/sfmwarp_pose.h: axis-angle poses, inverted sources, the depth range, %s" % torch.cuda.get_device_name(0))
    say("%d x %d, %d scales, %d sources; %d warm-up + %d timed steps per route and cell, alternating; microseconds" % (H, W, S, N_SRC, a.warmup, a.launches))
    head = "%-4s %-14s %-20s %-14s %8s %8s %8s %8s   %s" % ("B", "what", "step", "route", "median", "p10", "p90", "train", "verdict")
    misses = []

    def cell(B, what, step, names, cand, yard, rule):
        r_c, r_y = time_alternating([cand, yard], a.warmup, a.launches)
        spread = r_y[2] - r_y[1]
        verdict = "%.3fx" % (r_c[0] / r_y[0])
        if rule:
            ok = r_c[0] <= r_y[0] + spread
            if not ok:
                misses.append("B=%d %s %s: %s %.1f, %s %.1f, spread %.1f" % (B, what, step, names[0], r_c[0], names[1], r_y[0], spread))
            verdict += "; rule (<= %.1f + %.1f): %s" % (r_y[0], spread, "ok" if ok else "MISS")
        say("%-4d %-14s %-20s %-14s %8.1f %8.1f %8.1f %8.1f   %s" % (B, what, step, names[0], *r_c, verdict))
        say("%-4d %-14s %-20s %-14s %8.1f %8.1f %8.1f %8.1f" % (B, what, step, names[1], *r_y))

    say()
    say("1. the defaults: this build against the parent commit's library")
    say("rule: this build's median <= the parent's median + the parent's spread (p90 - p10)")
    if parent is None:
        say("   skipped: no --parent library given")
    else:
        say(head)
        for B in (4, 32):
            table, _ = workloads(B, dev)
            for what, fn in table.items():
                for step, grad in (("forward", False), ("forward + backward", True)):
                    cell(B, what, step, ("this", "parent"), lambda: fn(grad), with_library(parent, lambda: fn(grad)), True)
        say("rule: %s" % ("held in every cell" if not misses else "MISS in %d cell(s)" % len(misses)))
        for m in misses:
            say("  MISS " + m)
    say()
    say("2. Monodepth2's objective: the three arguments in ONE node against the same conventions in aten in front of the call, and")
    say("   against the call without the three arguments (no bar)")
    say(head)
    for B in (4, 32):
        _, (one_node, aten, without) = workloads(B, dev)
        for step, grad in (("forward", False), ("forward + backward", True)):
            cell(B, "monodepth2", step, ("one node", "aten in front"), lambda: one_node(grad), lambda: aten(grad), False)
            cell(B, "monodepth2", step, ("one node", "without them"), lambda: one_node(grad), lambda: without(grad), False)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
