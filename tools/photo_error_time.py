#!/usr/bin/env python3
"""Timing of torch_api.photometric_error with HIP events: the per-pixel L1 + SSIM error map of every (scale, image) of a step, and
the gradient back to the images, against the same formula in aten -- the route a user had before it.

  new   torch_api.photometric_error on the list of images and the list of targets: sfm_photo_error_fwd (one launch); backward
        sfm_photo_error_bwd (one launch).
  aten  per scale, the images of all samples batched: F.avg_pool2d(x, 3, 1, 1, count_include_pad=True) five times, the SSIM index of
        models/base_model.py:126-142 and the absolute difference in elementwise torch, backward by autograd.  The aten route is the
        yardstick: the new route is never timed against itself.

Shape: 128 x 416, 4 scales, 2 images per sample, at B = 32 and B = 4 (the reference's own batch), with ssim_rate 0.85 and 0 (L1 only:
aten then runs no pooling either).  Candidates: forward alone (no_grad) and forward + backward (torch.autograd.backward on the maps
with fixed upstream gradients; the .grad fields are cleared before every step, as optimizer.zero_grad does).  The two routes
alternate launch by launch in one process.

Per cell: --warmup steps of each candidate (default 20), then --launches timed ones (default 200), each between its own pair of
events (launch latency is in it when the stream is idle, for both alike); median, p10 and p90 in microseconds.  `train` is the same
number of steps between ONE pair of events, per step: what a queue that never runs dry sees.

usage: python tools/photo_error_time.py [--warmup 20] [--launches 200] [--out FILE]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resize_bwd_time import time_alternating  # noqa: E402

synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

H, W, S, N_IMG = 128, 416, 4, 2


def aten_photo_error(x, y, alpha):
    """x (B,n,3,h,w), y (B,3,h,w) -> (B,n,h,w): the formula of include/sfmwarp.h in aten"""
    B, n, c, h, w = x.shape
    X, Y = x.reshape(B * n, 3, h, w), y[:, None].expand(B, n, 3, h, w).reshape(B * n, 3, h, w)
    l1 = (X - Y).abs().mean(1)
    if alpha == 0:
        return l1.view(B, n, h, w)
    pool = lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=True)
    mx, my = pool(X), pool(Y)
    sx, sy, sxy = pool(X * X) - mx * mx, pool(Y * Y) - my * my, pool(X * Y) - mx * my
    ssim = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
    e = ((1 - ssim) / 2).clamp(0, 1).mean(1)
    return ((1 - alpha) * l1 + alpha * e).view(B, n, h, w)


def routes(B, alpha, dev):
    """(new, aten, leaves): functions (grad) -> the error maps [s]; same tensors"""
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_IMG, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    imgs = [t(a).view(B, N_IMG, 3, H >> s, W >> s).requires_grad_() for s, a in enumerate(d["src_pyr"])]
    tgts = [t(a) for a in d["tgt_pyr"]]
    gen = torch.Generator().manual_seed(0)
    gs = [torch.randn((B, N_IMG, H >> s, W >> s), generator=gen).to(dev) for s in range(S)]

    def run(fn, grad):
        for x in imgs:
            x.grad = None
        with torch.set_grad_enabled(grad):
            errs = fn()
        if grad:
            torch.autograd.backward(errs, gs)
        return errs

    new = lambda grad: run(lambda: ta.photometric_error(imgs, tgts, ssim_rate=alpha), grad)
    aten = lambda grad: run(lambda: [aten_photo_error(x, y, alpha) for x, y in zip(imgs, tgts)], grad)
    return new, aten, imgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per cell")
    if not torch.cuda.is_available():
        sys.exit("photo_error_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("torch_api.photometric_error vs the same formula in aten (avg_pool2d + autograd), %s" % torch.cuda.get_device_name(0))
    say("%d x %d, %d scales, %d images per sample; %d warm-up + %d timed steps per candidate and cell, alternating; microseconds"
        % (H, W, S, N_IMG, a.warmup, a.launches))
    say("%-4s %-6s %-20s %-6s %8s %8s %8s %8s   %s" % ("B", "alpha", "candidate", "route", "median", "p10", "p90", "train", "new faster at the median"))
    verdicts = []
    for B in (32, 4):
        for alpha in (0.85, 0.0):
            new, aten, leaves = routes(B, alpha, dev)
            # the two routes compute the same thing, to fp32 rounding
            en = [e.detach().clone() for e in new(True)]
            gn = [x.grad.clone() for x in leaves]
            ea = aten(True)
            worst_e = max(float((p - q).abs().max()) for p, q in zip(en, ea))
            worst_g = max(float((x.grad - g).abs().max() / x.grad.abs().max()) for x, g in zip(leaves, gn))
            say("B = %d, alpha = %g: maps differ by at most %.2g, gradients by at most %.2g of their maximum" % (B, alpha, worst_e, worst_g))
            for name, grad in (("forward", False), ("forward + backward", True)):
                r_new, r_aten = time_alternating([lambda: new(grad), lambda: aten(grad)], a.warmup, a.launches)
                faster = r_new[0] < r_aten[0]
                verdicts.append(faster)
                say("%-4d %-6g %-20s %-6s %8.1f %8.1f %8.1f %8.1f   %s (%.2fx)" % (B, alpha, name, "new", *r_new, "yes" if faster else "NO", r_aten[0] / r_new[0]))
                say("%-4d %-6g %-20s %-6s %8.1f %8.1f %8.1f %8.1f" % (B, alpha, name, "aten", *r_aten))
    say()
    say("new route faster than aten in %d of %d cells" % (sum(verdicts), len(verdicts)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
