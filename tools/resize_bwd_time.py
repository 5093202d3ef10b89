#!/usr/bin/env python3
"""Timing of sfm_resize_bwd (ops.resize_bwd) with HIP events.

  1. DispNet's three disp_up backwards (models/disp_net.py:105,111,117): (B,1,16,52)->(32,104), (32,104)->(64,208),
     (64,208)->(128,416) at B = 4 and B = 32, against aten's upsample_bilinear2d_backward(align_corners=True) on the same
     tensors -- what torch.nn.functional.interpolate's autograd runs, called directly so that neither side pays for the autograd
     engine.  The two alternate launch by launch in one process.
  2. The pyramid adjoint at cfg3's shape (N=32, C=6, 128x416, 4 terms) against its byte line: every gy[k] read once, gx written once.

Per shape: --warmup launches of each candidate (default 20), then --launches timed ones (default 200), each between its own pair
of events (the time from the stream reaching the first event to the kernel's end: launch latency is in it when the stream is
idle, for both candidates alike); median, p10 and p90 in microseconds.  `train` is the same number of launches between ONE pair of
events, per launch: what a queue that never runs dry sees.  Output allocation by torch is included on both sides.

usage: python tools/resize_bwd_time.py [--warmup 20] [--launches 200] [--out FILE]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("sfm-learner-chainer_amd.ops")

HBM_BYTES_PER_S = 8e12          # MI355X peak


def percentiles(us):
    return tuple(float(np.percentile(us, q)) for q in (50, 10, 90))


def time_alternating(fns, warmup, launches):
    """[(median, p10, p90, train) in us per fn]: the candidates alternate launch by launch"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)] for _ in fns]
    for i in range(launches):
        for k, fn in enumerate(fns):
            e0, e1 = pairs[k][i]
            e0.record()
            fn()
            e1.record()
    torch.cuda.synchronize()
    out = []
    for k, fn in enumerate(fns):
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs[k]]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(percentiles(us) + (e0.elapsed_time(e1) * 1e3 / launches,))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per shape")
    if not torch.cuda.is_available():
        sys.exit("resize_bwd_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("sfm_resize_bwd vs aten upsample_bilinear2d_backward (align_corners=True), %s" % torch.cuda.get_device_name(0))
    say("%d warm-up + %d timed launches per candidate and shape, alternating; microseconds" % (a.warmup, a.launches))
    say("%-34s %-6s %8s %8s %8s %8s   %s" % ("disp_up backward", "", "median", "p10", "p90", "train", "max |ours - aten|"))
    torch.manual_seed(0)
    for B in (4, 32):
        for h, w in ((16, 52), (32, 104), (64, 208)):
            g = torch.rand((B, 1, 2 * h, 2 * w), device=dev) * 2 - 1
            ours = lambda: ops.resize_bwd(g, (h, w))
            aten = lambda: torch.ops.aten.upsample_bilinear2d_backward(g, [2 * h, 2 * w], [B, 1, h, w], True)
            diff = float((ours() - aten()).abs().max())
            name = "(%d,1,%d,%d)->(%d,%d)" % (B, h, w, 2 * h, 2 * w)
            for who, r in zip(("ours", "aten"), time_alternating([ours, aten], a.warmup, a.launches)):
                say("%-34s %-6s %8.1f %8.1f %8.1f %8.1f   %s" % (name, who, *r, "%.3g" % diff if who == "ours" else ""))
    N, Cc, H, W, S = 32, 6, 128, 416, 4
    gys = [torch.rand((N, Cc, H >> s, W >> s), device=dev) * 2 - 1 for s in range(S)]
    nbytes = 4 * (sum(g.numel() for g in gys) + N * Cc * H * W)
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    (r,) = time_alternating([lambda: ops.resize_bwd(gys, (H, W))], a.warmup, a.launches)
    say()
    say("pyramid adjoint N=%d C=%d %dx%d, %d terms: %.1f MB read + %.1f MB written; at %.0f TB/s that is %.1f us"
        % (N, Cc, H, W, S, 4 * sum(g.numel() for g in gys) / 1e6, 4 * N * Cc * H * W / 1e6, HBM_BYTES_PER_S / 1e12, floor_us))
    say("%-34s %-6s %8.1f %8.1f %8.1f %8.1f   %.0f GB/s algorithmic at the median, %.2f of the byte line"
        % ("", "ours", *r, nbytes / r[0] / 1e3, floor_us / r[0]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
