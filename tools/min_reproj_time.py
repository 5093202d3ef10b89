#!/usr/bin/env python3
"""Timing of torch_api.min_reprojection_loss with HIP events against the route a user had before it: the example of INTEGRATION.md
("The photometric error of that loss") as it stood -- the library's warp_pyramid and photometric_error, then the per-scale tail in
aten.

  new   torch_api.min_reprojection_loss: ONE autograd node; the source pyramid, the warp, the target pyramid, the error maps of the
        warped and of the unwarped pyramid, sfm_min_reproj_fwd (two launches); backward sfm_min_reproj_bwd, sfm_photo_error_bwd,
        sfm_warp_pyramid_bwd.
  aten  warp_pyramid(return_valid=True) and photometric_error twice (the library, two autograd nodes), then per scale where, min, <,
        where, sum, sum, clamp, divide, add in aten with autograd's nodes behind them.  The aten route is the yardstick: the new
        route is never timed against itself.

Shape: 128 x 416, 4 scales, 2 sources, auto-mask on, at B = 4 and B = 32, with ssim_rate 0 and 0.85.  Candidates: forward alone
(no_grad) and forward + backward (total.backward(); the .grad fields are cleared before every step, as optimizer.zero_grad does).
The two routes alternate launch by launch in one process.

Per cell: --warmup steps of each candidate (default 20), then --launches timed ones (default 200), each between its own pair of
events (launch latency is in it when the stream is idle, for both alike); median, p10 and p90 in microseconds.  `train` is the same
number of steps between ONE pair of events, per step: what a queue that never runs dry sees.  `host` is the wall-clock time the host
needs to ISSUE one of those steps (no synchronisation inside the loop): where host is about train, the GPU waits for the host and
the step is host-bound.

usage: python tools/min_reproj_time.py [--warmup 20] [--launches 200] [--out FILE]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resize_bwd_time import time_alternating  # noqa: E402

ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

H, W, S, N_SRC = 128, 416, 4, 2


def example(tgt_img, src_imgs, intrinsics, pred_disps, pred_poses, ssim_rate):
    """min_reprojection_loss_ssim of INTEGRATION.md, as written"""
    B, n_src, _, H, W = src_imgs.shape
    S = len(pred_disps)
    warped, valid = ta.warp_pyramid(src_imgs, intrinsics, pred_disps, pred_poses, return_valid=True)
    unwarped = [p.view(B, n_src, 3, H >> s, W >> s) for s, p in enumerate(ops.pyramid(src_imgs.view(B, 3 * n_src, H, W), S))]
    reproj = ta.photometric_error(warped, tgt_img, ssim_rate=ssim_rate)
    with torch.no_grad():
        ident = ta.photometric_error(unwarped, tgt_img, ssim_rate=ssim_rate)
    total = 0.0
    for s, (e, v, e0) in enumerate(zip(reproj, valid, ident)):
        e = torch.where(v > 0, e, torch.full_like(e, float("inf")))
        best = e.min(1).values
        keep = best < e0.min(1).values
        total = total + torch.where(keep, best, torch.zeros_like(best)).sum() / keep.sum().clamp(min=1) / 2 ** s
    return total


def routes(B, alpha, dev):
    """(new, aten, leaves): functions (grad) -> total; same tensors"""
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_SRC, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    tgt, src, K = t(d["tgt"]), t(d["src"]), t(d["intrinsics"])
    disps, poses = [t(a).requires_grad_() for a in d["disps"]], [t(a).requires_grad_() for a in d["poses"]]
    leaves = disps + poses

    def run(fn, grad):
        for x in leaves:
            x.grad = None
        with torch.set_grad_enabled(grad):
            total = fn()
        if grad:
            total.backward()
        return total

    new = lambda grad: run(lambda: ta.min_reprojection_loss(tgt, src, K, disps, poses, ssim_rate=alpha), grad)
    aten = lambda grad: run(lambda: example(tgt, src, K, disps, poses, alpha), grad)
    return new, aten, leaves


def host_time(fn, steps):
    """microseconds of wall clock the host needs to issue one step (the queue drained before and after, never inside)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e6 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per cell")
    if not torch.cuda.is_available():
        sys.exit("min_reproj_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("torch_api.min_reprojection_loss vs the example of INTEGRATION.md (library stages 1-2 + the aten tail), %s" % torch.cuda.get_device_name(0))
    say("%d x %d, %d scales, %d sources, auto-mask on; %d warm-up + %d timed steps per candidate and cell, alternating; microseconds"
        % (H, W, S, N_SRC, a.warmup, a.launches))
    say("%-4s %-6s %-20s %-6s %8s %8s %8s %8s %8s   %s" % ("B", "alpha", "candidate", "route", "median", "p10", "p90", "train", "host", "new faster at the median"))
    verdicts, bound = [], []
    for B in (4, 32):
        for alpha in (0.0, 0.85):
            new, aten, leaves = routes(B, alpha, dev)
            # the two routes compute the same thing
            tn = float(new(True).detach())
            gn = [x.grad.clone() for x in leaves]
            ta_ = float(aten(True).detach())
            worst_g = max(float((x.grad - g).abs().max() / x.grad.abs().max()) for x, g in zip(leaves, gn))
            say("B = %d, alpha = %g: total %.9g (new) %.9g (aten), gradients differ by at most %.2g of their maximum" % (B, alpha, tn, ta_, worst_g))
            for name, grad in (("forward", False), ("forward + backward", True)):
                r_new, r_aten = time_alternating([lambda: new(grad), lambda: aten(grad)], a.warmup, a.launches)
                h_new, h_aten = host_time(lambda: new(grad), a.launches), host_time(lambda: aten(grad), a.launches)
                faster = r_new[0] < r_aten[0]
                verdicts.append(faster)
                bound.append((B, alpha, name, h_new >= 0.9 * r_new[3], h_aten >= 0.9 * r_aten[3]))
                say("%-4d %-6g %-20s %-6s %8.1f %8.1f %8.1f %8.1f %8.1f   %s (%.2fx)" % (B, alpha, name, "new", *r_new, h_new, "yes" if faster else "NO", r_aten[0] / r_new[0]))
                say("%-4d %-6g %-20s %-6s %8.1f %8.1f %8.1f %8.1f %8.1f" % (B, alpha, name, "aten", *r_aten, h_aten))
    say()
    say("new route faster than the example in %d of %d cells" % (sum(verdicts), len(verdicts)))
    say("host-bound (host >= 0.9 train): " + "; ".join("B=%d alpha=%g %s: new %s, aten %s" % (B, al, nm, "yes" if hn else "no", "yes" if ha else "no")
                                                       for B, al, nm, hn, ha in bound))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
