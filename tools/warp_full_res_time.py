#!/usr/bin/env python3
"""Timing of torch_api.warp_full_res and min_reprojection_loss(full_res=True) with HIP events against the routes a user had before
them, at the cells of profiles/warp_pyramid_time.txt: 128 x 416, 4 scales, 2 sources, B = 4 and B = 32.

  warp       new     torch_api.warp_full_res: ONE autograd node; sfm_warp_full_res_fwd (one launch), backward sfm_warp_full_res_bwd
                     (pixels, the gather of every low-resolution gradient, the fold).
             parent  torch_api.resize_images per scale + torch_api.projective_inverse_warp per (scale, source): S - 1 + S * n_src nodes.
  c-level    new     ops.warp_full_res_fwd / _bwd on the pixel-interleaved sources: the fused entry points alone.
             unfused ops.resize per resampled scale + ops.warp_pyramid_fwd at equal sizes; backward ops.warp_pyramid_bwd + ops.resize_bwd
                     per resampled scale: the same values bit for bit, with every full-resolution disparity and gradient materialised.
  objective  new     torch_api.min_reprojection_loss(full_res=True): ONE node.
             parent  the same objective with the parent's calls: the loop of INTEGRATION.md, "Full-resolution multi-scale".
The other route is the yardstick: the new route is never timed against itself.

Candidates: forward alone (no_grad) and forward + backward (the .grad fields are cleared before every step, as optimizer.zero_grad
does).  The two routes of a comparison alternate launch by launch in one process.  Per cell: --warmup steps of each candidate
(default 20), then --launches timed ones (default 200), each between its own pair of events; median, p10 and p90 in microseconds: the
spread of a route is its p90 - p10.  `train` is the same number of steps between ONE pair of events, per step; `host` the wall-clock
time the host needs to ISSUE one step.  The rule of the c-level comparison: the fused entry points are not slower at the median than
the unfused route by more than that route's own spread; every cell is printed, a miss as MISS.

--kernels N runs only N forward + backward steps of both c-level routes at B = 32 and prints nothing: the workload for one
`rocprofv3 --kernel-trace --stats` run.

usage: python tools/warp_full_res_time.py [--warmup 20] [--launches 200] [--out FILE] [--kernels N]"""
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
ALPHA = 0.85


def parent_warp(src, K0, disps, poses, tgt_hw):
    """[warped_s (B,n_src,3,H,W)] with the calls the library had before: one resize node per scale, one warp node per (scale, source)"""
    B, n_src = src.shape[:2]
    out = []
    for disp in disps:
        up = disp if tuple(disp.shape[2:]) == tuple(tgt_hw) else ta.resize_images(disp, tgt_hw)
        depth = (1 / up).view(B, -1)
        out.append(torch.stack([ta.projective_inverse_warp(src[:, i], depth, poses[i], K0) for i in range(n_src)], dim=1))
    return out


def parent_objective(tgt, src, K0, disps, poses):
    """INTEGRATION.md, 'Full-resolution multi-scale': the loop min_reprojection_loss(full_res=True) replaces"""
    with torch.no_grad():
        ident = ta.photometric_error([src], [tgt], ssim_rate=ALPHA)[0].min(1).values
    total = 0.0
    for s, warped in enumerate(parent_warp(src, K0, disps, poses, tgt.shape[2:])):
        valid = (warped.detach() != 0).any(2)
        e = ta.photometric_error([warped], [tgt], ssim_rate=ALPHA)[0]
        best = torch.where(valid, e, torch.full_like(e, float("inf"))).min(1).values
        keep = best < ident
        total = total + torch.where(keep, best, torch.zeros_like(best)).sum() / keep.sum().clamp(min=1) / 2 ** s
    return total


def routes(B, dev):
    """{comparison: (new, other)}: functions (grad) -> None on the same tensors"""
    d = synth.make_inputs(B=B, H=H, W=W, n_src=N_SRC, n_scales=S, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    tgt, src, K0 = t(d["tgt"]), t(d["src"]), t(d["intrinsics"][:, 0])
    disps, poses = [t(a).requires_grad_() for a in d["disps"]], [t(a).requires_grad_() for a in d["poses"]]
    leaves = disps + poses
    gen = torch.Generator().manual_seed(3)
    g = [torch.randn((B, N_SRC, 3, H, W), generator=gen).to(dev) for _ in range(S)]
    hwc = ops.pyramid_hwc(src.view(B, 3 * N_SRC, H, W), 1)[0]
    K4 = K0[:, None].expand(B, S, 3, 3).contiguous()
    raw_d, raw_p = [x.detach() for x in disps], [x.detach() for x in poses]

    def run(fn, grad):
        for x in leaves:
            x.grad = None
        with torch.set_grad_enabled(grad):
            total = fn()
        if grad:
            total.backward()

    def dot(warped):
        return sum((a * b).sum() for a, b in zip(warped, g))

    def fused(grad):
        ops.warp_full_res_fwd(hwc, raw_d, raw_p, K0, "hwc")
        if grad:
            ops.warp_full_res_bwd(hwc, raw_d, raw_p, K0, "hwc", g)

    def unfused(grad):
        ups = [raw_d[0]] + [ops.resize(x, (H, W)) for x in raw_d[1:]]
        ops.warp_pyramid_fwd([hwc] * S, ups, raw_p, K4, "hwc")
        if grad:
            d_up, _ = ops.warp_pyramid_bwd([hwc] * S, ups, raw_p, K4, "hwc", g)
            for x, gu in zip(raw_d[1:], d_up[1:]):
                ops.resize_bwd(gu, x.shape[2:])

    kw = dict(ssim_rate=ALPHA)
    return {
        "warp": (lambda grad: run(lambda: dot(ta.warp_full_res(src, K0, disps, poses)), grad),
                 lambda grad: run(lambda: dot(parent_warp(src, K0, disps, poses, (H, W))), grad)),
        "c-level": (fused, unfused),
        "objective": (lambda grad: run(lambda: ta.min_reprojection_loss(tgt, src, K0, disps, poses, full_res=True, **kw), grad),
                      lambda grad: run(lambda: parent_objective(tgt, src, K0, disps, poses), grad)),
    }, leaves


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
        sys.exit("warp_full_res_time: needs a GPU (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    if a.kernels:
        fused, unfused = routes(32, dev)[0]["c-level"]
        for _ in range(a.kernels):
            fused(True)
            unfused(True)
        torch.cuda.synchronize()
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("torch_api.warp_full_res and min_reprojection_loss(full_res=True) vs the routes before them, %s" % torch.cuda.get_device_name(0))
    say("%d x %d, %d scales, %d sources; %d warm-up + %d timed steps per candidate and cell, alternating; microseconds" % (H, W, S, N_SRC, a.warmup, a.launches))
    other_name = {"warp": "parent", "c-level": "unfused", "objective": "parent"}
    say("%-4s %-10s %-20s %-8s %8s %8s %8s %8s %8s   %s" % ("B", "what", "candidate", "route", "median", "p10", "p90", "train", "host", "verdict"))
    misses = []
    for B in (4, 32):
        table, leaves = routes(B, dev)
        for what, (new, other) in table.items():
            if what != "c-level":       # the two routes compute the same thing
                new(True)
                gn = [x.grad.clone() for x in leaves]
                other(True)
                worst = max(float((x.grad - gq).abs().max() / x.grad.abs().max().clamp(min=1e-30)) for x, gq in zip(leaves, gn))
                say("B = %d, %s: gradients of the two routes differ by at most %.2g of their maximum" % (B, what, worst))
            for name, grad in (("forward", False), ("forward + backward", True)):
                r_new, r_other = time_alternating([lambda: new(grad), lambda: other(grad)], a.warmup, a.launches)
                h_new, h_other = host_time(lambda: new(grad), a.launches), host_time(lambda: other(grad), a.launches)
                spread = r_other[2] - r_other[1]
                ok = r_new[0] <= r_other[0] + spread
                if what == "c-level" and not ok:
                    misses.append((B, name, r_new[0], r_other[0], spread))
                verdict = "%.2fx the other route's time" % (r_new[0] / r_other[0])
                if what == "c-level":
                    verdict += "; rule (new <= unfused + its spread %.1f): %s" % (spread, "ok" if ok else "MISS")
                say("%-4d %-10s %-20s %-8s %8.1f %8.1f %8.1f %8.1f %8.1f   %s" % (B, what, name, "new", *r_new, h_new, verdict))
                say("%-4d %-10s %-20s %-8s %8.1f %8.1f %8.1f %8.1f %8.1f" % (B, what, name, other_name[what], *r_other, h_other))
    say()
    say("c-level rule: %s" % ("held in every cell" if not misses else "; ".join(
        "MISS at B=%d %s: new %.1f, unfused %.1f, spread %.1f" % m for m in misses)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
