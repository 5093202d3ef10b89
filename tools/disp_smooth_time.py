#!/usr/bin/env python3
"""Timing of torch_api.disparity_smoothness and of min_reprojection_loss(smooth_weight=...) with HIP events against the routes a user
had before them: Monodepth2's smoothness term written in aten (the example of INTEGRATION.md, "The second term of that loss"), on
the same prebuilt target pyramid.

  term       new   torch_api.disparity_smoothness: ONE autograd node; sfm_disp_smooth_fwd (two launches), backward sfm_disp_smooth_bwd.
             aten  per scale two means, a divide, four slices and differences, abs, a channel mean, exp, a multiply and two means, with
                   autograd's nodes behind them.
  objective  new   torch_api.min_reprojection_loss(smooth_weight=1e-3): ONE node for both terms.
             aten  torch_api.min_reprojection_loss() + 1e-3 * the aten term.
The aten route is the yardstick: the new route is never timed against itself.

Shape: 128 x 416, 4 scales (2 sources for the objective), at B = 4 and B = 32.  Candidates: forward alone (no_grad) and forward +
backward (total.backward(); the .grad fields are cleared before every step, as optimizer.zero_grad does).  The two routes alternate
launch by launch in one process.  Per cell: --warmup steps of each candidate (default 20), then --launches timed ones (default 200),
each between its own pair of events; median, p10 and p90 in microseconds.  `train` is the same number of steps between ONE pair of
events, per step; `host` is the wall-clock time the host needs to ISSUE one step: where host >= 0.9 train the step is host-bound.

Behind the cells of each B, the three launches on their own: sfm_disp_smooth_fwd (pixels + fold) and sfm_disp_smooth_bwd, overwrite and
accumulate, through ops.* back to back between one pair of events -- an upper bound of the kernel time, the host's issue rate
included -- against the algorithmic traffic (16 B/px forward, 20 B/px backward, 24 with accumulate).  --kernels N runs only N such
steps at B = 32 and prints nothing: the workload for one `rocprofv3 --kernel-trace --stats` run, which separates the pixel pass from the fold.

usage: python tools/disp_smooth_time.py [--warmup 20] [--launches 200] [--out FILE] [--kernels N]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from min_reproj_time import host_time  # noqa: E402
from resize_bwd_time import time_alternating  # noqa: E402

ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

H, W, S, N_SRC = 128, 416, 4, 2
SMOOTH_WEIGHT = 1e-3


def example(pred_disps, tgts):
    """disparity_smoothness_aten of INTEGRATION.md, as written, on a prebuilt pyramid"""
    total = 0.0
    for s, (disp, img) in enumerate(zip(pred_disps, tgts)):
        d = disp / (disp.mean(2, True).mean(3, True) + 1e-7)
        gx = (d[:, :, :, :-1] - d[:, :, :, 1:]).abs() * (-(img[:, :, :, :-1] - img[:, :, :, 1:]).abs().mean(1, keepdim=True)).exp()
        gy = (d[:, :, :-1, :] - d[:, :, 1:, :]).abs() * (-(img[:, :, :-1, :] - img[:, :, 1:, :]).abs().mean(1, keepdim=True)).exp()
        total = total + (gx.mean() + gy.mean()) / 2 ** s
    return total


def routes(B, dev):
    """{comparison: (new, aten)}, leaves: functions (grad) -> total; same tensors"""
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_SRC, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    tgt, src, K = t(d["tgt"]), t(d["src"]), t(d["intrinsics"])
    disps, poses = [t(a).requires_grad_() for a in d["disps"]], [t(a).requires_grad_() for a in d["poses"]]
    tgts = ops.pyramid(tgt, S)
    leaves = disps + poses

    def run(fn, grad):
        for x in leaves:
            x.grad = None
        with torch.set_grad_enabled(grad):
            total = fn()
        if grad:
            total.backward()
        return total

    both = dict(ssim_rate=0.85)
    return {
        "term": (lambda grad: run(lambda: ta.disparity_smoothness(disps, tgts)[0], grad),
                 lambda grad: run(lambda: example(disps, tgts), grad)),
        "objective": (lambda grad: run(lambda: ta.min_reprojection_loss(tgt, src, K, disps, poses, smooth_weight=SMOOTH_WEIGHT, **both), grad),
                      lambda grad: run(lambda: ta.min_reprojection_loss(tgt, src, K, disps, poses, **both) + SMOOTH_WEIGHT * example(disps, tgts), grad)),
    }, leaves, (disps, tgts)


def launches_alone(disps, tgts, steps, say=None):
    """the forward and the two backwards through ops.*, `steps` of each back to back between one pair of events"""
    w = [2.0 ** -s for s in range(S)]
    disps = [x.detach() for x in disps]
    g_loss = torch.ones(S + 1, device=disps[0].device)
    loss, stats = ops.disp_smooth_fwd(disps, tgts, w, True, "mean_abs")
    out = ops.disp_smooth_bwd(disps, tgts, stats, g_loss, w, True, "mean_abs")
    px = sum(x.numel() for x in disps)
    cands = [("sfm_disp_smooth_fwd (pixels + fold)", 16, lambda: ops.disp_smooth_fwd(disps, tgts, w, True, "mean_abs")),
             ("sfm_disp_smooth_bwd", 20, lambda: ops.disp_smooth_bwd(disps, tgts, stats, g_loss, w, True, "mean_abs")),
             ("sfm_disp_smooth_bwd, accumulate", 24, lambda: ops.disp_smooth_bwd(disps, tgts, stats, g_loss, w, True, "mean_abs", out=out))]
    for name, bytes_px, fn in cands:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / steps
        host = host_time(fn, steps)
        if say:
            say("%-38s %8.1f us per call between one pair of events, host %6.1f us; %d px x %d B = %.1f MB -> %.2f TB/s at that time"
                % (name, us, host, px, bytes_px, px * bytes_px / 1e6, px * bytes_px / us / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per cell")
    if not torch.cuda.is_available():
        sys.exit("disp_smooth_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    if a.kernels:
        _, _, (disps, tgts) = routes(32, dev)
        launches_alone(disps, tgts, a.kernels)
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("torch_api.disparity_smoothness and min_reprojection_loss(smooth_weight=%g) vs the smoothness term of INTEGRATION.md in aten, %s"
        % (SMOOTH_WEIGHT, torch.cuda.get_device_name(0)))
    say("%d x %d, %d scales, %d sources; %d warm-up + %d timed steps per candidate and cell, alternating; microseconds" % (H, W, S, N_SRC, a.warmup, a.launches))
    say("%-4s %-10s %-20s %-6s %8s %8s %8s %8s %8s   %s" % ("B", "what", "candidate", "route", "median", "p10", "p90", "train", "host", "new faster at the median"))
    verdicts, bound = [], []
    for B in (4, 32):
        table, leaves, (disps, tgts) = routes(B, dev)
        for what, (new, aten) in table.items():
            tn = float(new(True).detach())
            gn = [None if x.grad is None else x.grad.clone() for x in leaves]
            ta_ = float(aten(True).detach())
            worst_g = max(float((x.grad - g).abs().max() / x.grad.abs().max()) for x, g in zip(leaves, gn) if g is not None)
            say("B = %d, %s: total %.9g (new) %.9g (aten), gradients differ by at most %.2g of their maximum" % (B, what, tn, ta_, worst_g))
            for name, grad in (("forward", False), ("forward + backward", True)):
                r_new, r_aten = time_alternating([lambda: new(grad), lambda: aten(grad)], a.warmup, a.launches)
                h_new, h_aten = host_time(lambda: new(grad), a.launches), host_time(lambda: aten(grad), a.launches)
                faster = r_new[0] < r_aten[0]
                verdicts.append((B, what, name, faster))
                bound.append((B, what, name, h_new >= 0.9 * r_new[3], h_aten >= 0.9 * r_aten[3]))
                say("%-4d %-10s %-20s %-6s %8.1f %8.1f %8.1f %8.1f %8.1f   %s (%.2fx)" % (B, what, name, "new", *r_new, h_new, "yes" if faster else "NO", r_aten[0] / r_new[0]))
                say("%-4d %-10s %-20s %-6s %8.1f %8.1f %8.1f %8.1f %8.1f" % (B, what, name, "aten", *r_aten, h_aten))
        say("the launches on their own, B = %d (normalize, mean_abs):" % B)
        launches_alone(disps, tgts, a.launches, say)
    say()
    say("new route faster than the aten one in %d of %d cells%s" % (sum(v[3] for v in verdicts), len(verdicts),
                                                                   "".join("; MISS: B=%d %s %s" % v[:3] for v in verdicts if not v[3])))
    say("host-bound (host >= 0.9 train): " + "; ".join("B=%d %s %s: new %s, aten %s" % (B, wh, nm, "yes" if hn else "no", "yes" if ha else "no")
                                                       for B, wh, nm, hn, ha in bound))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
