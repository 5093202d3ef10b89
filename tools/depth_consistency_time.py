#!/usr/bin/env python3
"""Timing of torch_api.depth_consistency with HIP events: the geometry-consistency maps of every (scale, source) of a step, and the
gradient back through them, against the same term written in aten.

  new   torch_api.depth_consistency: sfm_depth_consistency_fwd (one launch); backward sfm_depth_consistency_bwd (a memset per bound
        d_src_disp, one launch over the pixels + the fold).
  aten  float32 on the device, per (scale, source): the pose matrix (torch_api.pose_matrix), P = K . T, K^-1 by torch.linalg.inv, the
        projection and the doubling outside the view as the library forms them, grid_sample(align_corners=True,
        padding_mode="zeros") of 1 / src_disp, the clamp and the quotient; backward by autograd.

Shape: 128 x 416, 4 scales, 2 sources, at B = 4 and B = 32.  Candidates: forward alone (no_grad), forward + backward with the
gradient of the sources' disparities (d_src_disp: the scatter) and forward + backward without it (src_disps detached on both routes).
The upstream gradients are fixed; the .grad fields are cleared before every step, as optimizer.zero_grad does.  The two routes
alternate launch by launch in one process.

Per cell: --warmup steps of each candidate (default 20), then --launches timed ones (default 200), each between its own pair of
events; median, p10 and p90 in microseconds.  `train` is the same number of steps between ONE pair of events, per step.
The one rule: the new route's median <= the aten route's median + the aten route's spread (p90 - p10).

--kernels N runs only N forward + backward steps of the new route at B = 32, half with and half without d_src_disp, and prints
nothing: the workload for one `rocprofv3 --kernel-trace --stats` run, which tells the kernels of a step apart.

usage: python tools/depth_consistency_time.py [--warmup 20] [--launches 200] [--out FILE] [--kernels N]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resize_bwd_time import time_alternating  # noqa: E402

synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

H, W, S, N_SRC = 128, 416, 4, 2


def aten_term(disps, src_disps, K, poses):
    """[diff_s (B,n_src,h,w)] in aten float32"""
    out = []
    for s, (disp, src) in enumerate(zip(disps, src_disps)):
        B, _, h, w = disp.shape
        Ks = K[:, s]
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=disp.device),
                                torch.arange(w, dtype=torch.float32, device=disp.device), indexing="ij")
        pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, dtype=torch.float32, device=disp.device)], 0)
        cam = (1.0 / disp).reshape(B, 1, h * w) * (torch.linalg.inv(Ks) @ pix)
        per = []
        for i, pose in enumerate(poses):
            Pm = Ks @ ta.pose_matrix(pose, pose_format="euler")
            q = Pm[:, :, :3] @ cam + Pm[:, :, 3:]
            z = q[:, 2] + 1e-10
            xn = (q[:, 0] / z) / ((w - 1) / 2.0) - 1.0
            yn = (q[:, 1] / z) / ((h - 1) / 2.0) - 1.0
            in_x, in_y = (xn > -1) & (xn < 1), (yn > -1) & (yn < 1)
            grid = torch.stack([torch.where(in_x, xn, 2 * xn), torch.where(in_y, yn, 2 * yn)], -1).reshape(B, h, w, 2)
            projected = torch.nn.functional.grid_sample(1.0 / src[:, i:i + 1], grid, mode="bilinear", padding_mode="zeros",
                                                        align_corners=True)[:, 0]
            computed = q[:, 2].clamp(min=1e-3).reshape(B, h, w)
            ok = (in_x & in_y).reshape(B, h, w)
            safe = torch.where(ok, computed + projected, torch.ones_like(projected))
            per.append(torch.where(ok, (computed - projected).abs() / safe, torch.zeros_like(projected)))
        out.append(torch.stack(per, 1))
    return out


def routes(B, dev):
    """(new, aten, leaves): functions (grad, with_src) -> [diff_s]; same inputs"""
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_SRC, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    rng = np.random.RandomState(2)
    K = t(d["intrinsics"])
    disps, poses = [t(a).requires_grad_() for a in d["disps"]], [t(a).requires_grad_() for a in d["poses"]]
    srcs = [t(10.0 / (1.0 + np.exp(-1.5 * rng.uniform(-1, 1, (B, N_SRC) + a.shape[2:]))) + 0.01).requires_grad_() for a in d["disps"]]
    detached = [x.detach() for x in srcs]
    leaves = disps + poses + srcs
    gen = torch.Generator().manual_seed(0)
    gs = [torch.randn((B, N_SRC, H >> s, W >> s), generator=gen).to(dev) for s in range(S)]

    def run(term, grad, with_src):
        for x in leaves:
            x.grad = None
        with torch.set_grad_enabled(grad):
            diff = term(disps, srcs if with_src else detached, K, poses)
        if grad:
            torch.autograd.backward(diff, gs)
        return diff

    new = lambda grad, with_src=True: run(lambda a, b, k, p: ta.depth_consistency(a, b, k, p), grad, with_src)
    aten = lambda grad, with_src=True: run(aten_term, grad, with_src)
    return new, aten, leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_consistency_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    if a.kernels:
        new, _, _ = routes(32, dev)
        for k in range(a.kernels):
            new(True, k % 2 == 0)
        torch.cuda.synchronize()
        return
    if a.warmup < 20 or a.launches < 200:
        ap.error("at least 20 warm-up and 200 timed launches per cell")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("torch_api.depth_consistency vs the same term in aten float32, %s" % torch.cuda.get_device_name(0))
    say("%d x %d, %d scales, %d sources; %d warm-up + %d timed steps per route and cell, alternating; microseconds" % (H, W, S, N_SRC, a.warmup, a.launches))
    say("rule: the new route's median <= the aten route's median + the aten route's spread (p90 - p10)")
    say("%-4s %-34s %-6s %8s %8s %8s %8s   %s" % ("B", "step", "route", "median", "p10", "p90", "train", "verdict"))
    held = []
    for B in (4, 32):
        new, aten, leaves = routes(B, dev)
        # the two routes compute the same function, each in its own float32 order: they part where a pixel sits on a discontinuity (the
        # in-view test, a cell boundary of the sampler, the kink of |computed - projected|; tests/depth_consistency_ref.py: knife),
        # there by the whole jump -- so the typical distance is reported, and how many elements lie beyond it
        dn = torch.cat([x.detach().flatten() for x in new(True)])
        gn = [x.grad.clone() for x in leaves]
        da = torch.cat([x.detach().flatten() for x in aten(True)])
        apart = float(((dn - da).abs() > 1e-4).float().mean())
        typical = float((dn - da).abs().median())
        rel = max(float((x.grad - g).norm() / g.norm()) for x, g in zip(leaves, gn))
        say("B = %d: diff: median distance %.2g, %.4f %% of the elements further apart than 1e-4; gradients: relative L2 distance at most %.2g"
            % (B, typical, 100 * apart, rel))
        for name, grad, with_src in (("forward", False, True), ("forward + backward, d_src_disp", True, True),
                                     ("forward + backward, no d_src_disp", True, False)):
            r_new, r_aten = time_alternating([lambda: new(grad, with_src), lambda: aten(grad, with_src)], a.warmup, a.launches)
            bar = r_aten[0] + (r_aten[2] - r_aten[1])
            ok = r_new[0] <= bar
            held.append(ok)
            say("%-4d %-34s %-6s %8.1f %8.1f %8.1f %8.1f   %.3fx; rule (<= %.1f + %.1f): %s"
                % (B, name, "new", *r_new, r_new[0] / r_aten[0], r_aten[0], r_aten[2] - r_aten[1], "ok" if ok else "MISSED"))
            say("%-4d %-34s %-6s %8.1f %8.1f %8.1f %8.1f" % (B, name, "aten", *r_aten))
    say("rule: held in %s" % ("every cell" if all(held) else "%d of %d cells" % (sum(held), len(held))))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
