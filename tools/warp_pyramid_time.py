#!/usr/bin/env python3
"""Timing of torch_api.warp_pyramid with HIP events: the warped source images of every (scale, source) of a step, and the gradient
back through them, against the route a user had before it.

  new     torch_api.warp_pyramid from the full-resolution sources: ops.pyramid_hwc (one launch) + sfm_warp_pyramid_fwd (one launch);
          backward sfm_warp_pyramid_bwd (one launch over the pixels + the fold).
  parent  a planar pyramid from ops.pyramid, then torch_api.projective_inverse_warp once per (scale, source), as
          models/base_model.py:88-94 calls it: 1 / disp, the slices of the pyramid and of the intrinsics, and (backward) the sums of
          d_depth over the sources and its way back to the disparity in torch.

Shape: 128 x 416, 4 scales, 2 sources, at B = 32 and B = 4 (the reference's own batch).  Candidates: forward alone (no_grad) and
forward + backward (torch.autograd.backward on the warped images with fixed upstream gradients: no loss kernel on either side; the
.grad fields are cleared before every step, as optimizer.zero_grad does).  The two routes alternate launch by launch in one process.

Per cell: --warmup steps of each candidate (default 20), then --launches timed ones (default 200), each between its own pair of
events (launch latency is in it when the stream is idle, for both alike); median, p10 and p90 in microseconds.  `train` is the same
number of steps between ONE pair of events, per step: what a queue that never runs dry sees.

usage: python tools/warp_pyramid_time.py [--warmup 20] [--launches 200] [--out FILE]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resize_bwd_time import time_alternating  # noqa: E402

ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

H, W, S, N_SRC = 128, 416, 4, 2


def routes(B, dev):
    """(new, parent): functions (grad) -> (the warped images [s][i], the leaves); same inputs"""
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_SRC, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    src, K = t(d["src"]), t(d["intrinsics"])
    stacked = src.view(B, 3 * N_SRC, H, W)
    disps, poses = [t(a).requires_grad_() for a in d["disps"]], [t(a).requires_grad_() for a in d["poses"]]
    leaves = disps + poses
    gen = torch.Generator().manual_seed(0)
    gs = [torch.randn((B, N_SRC, 3, H >> s, W >> s), generator=gen).to(dev) for s in range(S)]

    def new(grad):
        for x in leaves:
            x.grad = None
        with torch.set_grad_enabled(grad):
            warped = ta.warp_pyramid(src, K, disps, poses)
        if grad:
            torch.autograd.backward(warped, gs)
        return [[w[:, i] for i in range(N_SRC)] for w in warped]

    g_parent = [[g[:, i].contiguous() for i in range(N_SRC)] for g in gs]

    def parent(grad):
        for x in leaves:
            x.grad = None
        with torch.set_grad_enabled(grad):
            pyr = ops.pyramid(stacked, S)
            warped = []
            for s in range(S):
                depth = (1.0 / disps[s]).view(B, -1)
                warped.append([ta.projective_inverse_warp(pyr[s][:, 3 * i:3 * i + 3], depth, poses[i], K[:, s]) for i in range(N_SRC)])
        if grad:
            torch.autograd.backward([w for ws in warped for w in ws], [g for g_s in g_parent for g in g_s])
        return warped

    return new, parent, leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per cell")
    if not torch.cuda.is_available():
        sys.exit("warp_pyramid_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("torch_api.warp_pyramid vs projective_inverse_warp per (scale, source), %s" % torch.cuda.get_device_name(0))
    say("%d x %d, %d scales, %d sources; %d warm-up + %d timed steps per candidate and cell, alternating; microseconds" % (H, W, S, N_SRC, a.warmup, a.launches))
    say("%-6s %-20s %-7s %8s %8s %8s %8s   %s" % ("B", "candidate", "route", "median", "p10", "p90", "train", "new faster at the median"))
    verdicts = []
    for B in (32, 4):
        new, parent, leaves = routes(B, dev)
        # the two routes compute the same thing: the forward bit for bit, the gradients to fp32 summation order
        wn = new(True)
        gn = [x.grad.clone() for x in leaves]
        wp = parent(True)
        same = all(torch.equal(a, b) for ws_n, ws_p in zip(wn, wp) for a, b in zip(ws_n, ws_p))
        worst = max(float((x.grad - g).abs().max() / x.grad.abs().max()) for x, g in zip(leaves, gn))
        say("B = %d: warped images bit-identical: %s; gradients differ by at most %.2g of their maximum" % (B, same, worst))
        for name, grad in (("forward", False), ("forward + backward", True)):
            r_new, r_parent = time_alternating([lambda: new(grad), lambda: parent(grad)], a.warmup, a.launches)
            faster = r_new[0] < r_parent[0]
            verdicts.append(faster)
            say("%-6d %-20s %-7s %8.1f %8.1f %8.1f %8.1f   %s (%.2fx)" % (B, name, "new", *r_new, "yes" if faster else "NO", r_parent[0] / r_new[0]))
            say("%-6d %-20s %-7s %8.1f %8.1f %8.1f %8.1f" % (B, name, "parent", *r_parent))
    say()
    say("new route faster than the parent's in %d of 4 cells" % sum(verdicts))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
