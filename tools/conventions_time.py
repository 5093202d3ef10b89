#!/usr/bin/env python3
"""Timing of the two conventions of include/sfmwarp_conventions.h with HIP events, at the cells of profiles/warp_full_res_time.txt:
128 x 416, 4 scales, 2 sources, B = 4 and B = 32.

Two questions, one rule.  A candidate is not slower at the median than its yardstick by more than the yardstick's own spread
(p90 - p10); every cell is printed, a miss as MISS.

  1. default   the calls WITHOUT the new arguments against the same calls in the parent commit's library: nothing on that path
               should have changed.  `--parent PATH` names that build's libsfmwarp.so.  (SFMWARP_LIB selects another build of the
               SAME binding; a library without the new symbols cannot be bound by it, so the parent's is loaded here with the tables
               of the symbols it has and swapped in under ops for its turns.)  Without --parent this part is skipped and says so.
  2. modes     padding="reflect" against padding="zero", upsample="half_pixel" against upsample="align_corners", and the composite in
               both new conventions against the composite in neither, in THIS build.

Per question three rows: the photometric error of the S full-resolution warped sets (ops.photo_error_fwd / _bwd), the
full-resolution warp (ops.warp_full_res_fwd / _bwd), and torch_api.min_reprojection_loss(full_res=True, smooth_weight=1e-3); each
forward alone and forward + backward.  The two routes of a cell alternate launch by launch in one process.  Per cell: --warmup steps
of each (default 20), then --launches timed ones (default 200), each between its own pair of events; median, p10 and p90 in
microseconds; `train` is the same number of steps between ONE pair of events, per step.

--kernels N runs only N forward + backward steps of the two operators in both modes at B = 32 and prints nothing: the workload for one
`rocprofv3 --kernel-trace --stats` run, which tells the kernels of a step apart.

usage: python tools/conventions_time.py [--parent PATH] [--warmup 20] [--launches 200] [--out FILE] [--kernels N]"""
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


def load_parent(path):
    """the parent build bound with the binding's tables, without the symbols it does not have"""
    lib = C.CDLL(path)
    for table in (_lib.SYMBOLS, _lib.EXT_SYMBOLS, _lib.SMOOTH_SYMBOLS, _lib.FULL_RES_SYMBOLS):
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


def workloads(B, dev):
    """{row: fn(grad, padding, upsample)} on the same tensors"""
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_SRC, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    tgt, src, K0 = t(d["tgt"]), t(d["src"]), t(d["intrinsics"][:, 0])
    disps, poses = [t(a).requires_grad_() for a in d["disps"]], [t(a).requires_grad_() for a in d["poses"]]
    leaves = disps + poses
    raw_d, raw_p = [x.detach() for x in disps], [x.detach() for x in poses]
    gen = torch.Generator().manual_seed(3)
    g = [torch.randn((B, N_SRC, 3, H, W), generator=gen).to(dev) for _ in range(S)]
    g_err = [torch.randn((B, N_SRC, H, W), generator=gen).to(dev) for _ in range(S)]
    hwc = ops.pyramid_hwc(src.view(B, 3 * N_SRC, H, W), 1)[0]
    warped = ops.warp_full_res_fwd(hwc, raw_d, raw_p, K0, "hwc")
    tgts = [tgt] * S

    def photo(grad, padding, upsample):
        ops.photo_error_fwd(warped, tgts, ALPHA, padding)
        if grad:
            ops.photo_error_bwd(warped, tgts, ALPHA, g_err, padding)

    def warp(grad, padding, upsample):
        ops.warp_full_res_fwd(hwc, raw_d, raw_p, K0, "hwc", upsample=upsample)
        if grad:
            ops.warp_full_res_bwd(hwc, raw_d, raw_p, K0, "hwc", g, upsample=upsample)

    def composite(grad, padding, upsample):
        for x in leaves:
            x.grad = None
        with torch.set_grad_enabled(grad):
            total = ta.min_reprojection_loss(tgt, src, K0, disps, poses, ssim_rate=ALPHA, smooth_weight=SMOOTH, full_res=True,
                                             ssim_padding=padding, upsample=upsample)
        if grad:
            total.backward()

    return {"photo_error": photo, "warp_full_res": warp, "composite": composite}


# what a row's candidate turns on: (padding, upsample)
MODES = {"photo_error": ("reflect", "align_corners"), "warp_full_res": ("zero", "half_pixel"), "composite": ("reflect", "half_pixel")}
DEFAULT = ("zero", "align_corners")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per cell")
    if not torch.cuda.is_available():
        sys.exit("conventions_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    if a.kernels:
        table = workloads(32, dev)
        for _ in range(a.kernels):
            for what in ("photo_error", "warp_full_res"):
                table[what](True, *DEFAULT)
                table[what](True, *MODES[what])
        torch.cuda.synchronize()
        return
    parent = load_parent(a.parent) if a.parent else None
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("the conventions of include/sfmwarp_conventions.h: reflection-padded SSIM, half-pixel upsampling, %s" % torch.cuda.get_device_name(0))
    say("%d x %d, %d scales, %d sources; %d warm-up + %d timed steps per route and cell, alternating; microseconds" % (H, W, S, N_SRC, a.warmup, a.launches))
    say("rule: candidate median <= yardstick median + the yardstick's spread (p90 - p10)")
    head = "%-4s %-14s %-20s %-10s %8s %8s %8s %8s   %s" % ("B", "what", "step", "route", "median", "p10", "p90", "train", "verdict")
    misses = []

    def cell(question, B, what, step, names, cand, yard):
        r_c, r_y = time_alternating([cand, yard], a.warmup, a.launches)
        spread = r_y[2] - r_y[1]
        ok = r_c[0] <= r_y[0] + spread
        if not ok:
            misses.append("%s B=%d %s %s: %s %.1f, %s %.1f, spread %.1f" % (question, B, what, step, names[0], r_c[0], names[1], r_y[0], spread))
        say("%-4d %-14s %-20s %-10s %8.1f %8.1f %8.1f %8.1f   %.3fx; rule (<= %.1f + %.1f): %s"
            % (B, what, step, names[0], *r_c, r_c[0] / r_y[0], r_y[0], spread, "ok" if ok else "MISS"))
        say("%-4d %-14s %-20s %-10s %8.1f %8.1f %8.1f %8.1f" % (B, what, step, names[1], *r_y))

    say()
    say("1. the default conventions: this build against the parent commit's library")
    if parent is None:
        say("   skipped: no --parent library given")
    else:
        say(head)
        for B in (4, 32):
            for what, fn in workloads(B, dev).items():
                for step, grad in (("forward", False), ("forward + backward", True)):
                    cell("default", B, what, step, ("this", "parent"), lambda: fn(grad, *DEFAULT), with_library(parent, lambda: fn(grad, *DEFAULT)))
    say()
    say("2. the new modes against their default counterparts, this build")
    say(head)
    for B in (4, 32):
        for what, fn in workloads(B, dev).items():
            for step, grad in (("forward", False), ("forward + backward", True)):
                mode = MODES[what]
                cell("modes", B, what, step, ("+".join(m for m, d0 in zip(mode, DEFAULT) if m != d0), "default"),
                     lambda: fn(grad, *mode), lambda: fn(grad, *DEFAULT))
    say()
    say("rule: %s" % ("held in every cell" if not misses else "MISS in %d cell(s)" % len(misses)))
    for m in misses:
        say("  MISS " + m)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
