#!/usr/bin/env python3
"""Time per forward + backward step of the loss, three routes on the same synth inputs (128x416, 2 sources, 4 scales, L1 + SSIM 0.15 +
second-order smoothness 0.1), at the reference's B = 4 and at BASELINE cfg3 (B = 32):

  torch   torch_api.SFMLearnerLoss(...) -> total.backward()          (fused launch + sfm_scale_arrays + per-call allocations)
  link    links.SFMLearnerLoss(...) (Chainer surface) -> loss.backward()
  manual  the link, then torch.autograd.backward(predictions, their .grad): how a torch.nn network reaches those gradients
          through the link.  A training loop pays the autograd engine for the network's backward on either route; this row
          pays it for the six prediction leaves as the torch route does, so `torch - manual` is the route's own extra cost.

Per route: HIP-event time per step over a loop of steps (what a training loop pays on the GPU's timeline; host-bound steps show
their host time here too) and host time per call (enqueue only, no sync).  Also counted: the distinct loss descriptors the torch
route hands to the library over the loop (the library's plan cache keeps the last four per thread, keyed on the descriptor bytes,
pointers included).  --rocprof: re-runs the torch route at cfg3 in a child process under `rocprofv3 --kernel-trace --stats` and
prints the kernel statistics (the scale kernel's time among them).

    python tools/torch_step_time.py [--steps 200] [--rocprof] [--out FILE]
"""
import argparse
import csv
import glob
import importlib
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sfm-learner-chainer_amd"
ta = importlib.import_module(PKG + ".torch_api")
links = importlib.import_module(PKG + ".links")
cs = importlib.import_module(PKG + ".chainer_surface")
synth = importlib.import_module(PKG + ".synth")

CONFIG = dict(seq_len=3, smooth_reg=0.1, exp_reg=0.0, ssim_rate=0.15)


def inputs(B, dev):
    d = synth.make_inputs(B=B, H=128, W=416, n_src=2, n_scales=4, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(d["tgt"]), t(d["src"]), t(d["intrinsics"]), [t(a) for a in d["disps"]], [t(a) for a in d["poses"]]


def torch_step(B, dev):
    tgt, src, K, disps, poses = inputs(B, dev)
    leaves = [a.requires_grad_() for a in disps + poses]
    model = ta.SFMLearnerLoss(CONFIG)

    def step():
        for a in leaves:
            a.grad = None
        total = model(tgt, src, K, None, disps, poses)
        total.backward()
    return step


def link_step(B, dev):
    tgt, src, K, disps, poses = inputs(B, dev)
    vd, vp = [cs.Variable(a) for a in disps], [cs.Variable(a) for a in poses]
    model = links.SFMLearnerLoss(CONFIG)

    def step():
        for v in vd + vp:
            v.cleargrad()
        loss = model(tgt, src, K, None, vd, vp)
        loss.backward()
    return step


def manual_step(B, dev):
    tgt, src, K, disps, poses = inputs(B, dev)
    leaves = [a.requires_grad_() for a in disps + poses]
    vs = [cs.Variable(a.detach()) for a in leaves]
    model = links.SFMLearnerLoss(CONFIG)

    def step():
        for a, v in zip(leaves, vs):
            a.grad = None
            v.cleargrad()
        loss = model(tgt, src, K, None, vs[:4], vs[4:])
        loss.backward()
        torch.autograd.backward(leaves, [v.grad for v in vs])
    return step


def measure(step, steps, reps=5):
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    ev, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e3 / steps)
        host.append((t1 - t0) * 1e6 / steps)
    return float(np.median(ev)), float(np.median(host)), float(np.min(ev)), float(np.max(ev))


def rocprof_stats(steps, out_dir):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return ["rocprofv3 not found: no kernel statistics"]
    shutil.rmtree(out_dir, ignore_errors=True)
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "torch_route", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--steps", str(steps)]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return ["rocprofv3 wrote no kernel_stats.csv under %s" % out_dir]
    lines = ["rocprofv3 --kernel-trace --stats, torch route at cfg3 (B=32), %d steps after 20 warm-up steps:" % steps,
             "  %-48s %7s %10s %10s %10s" % ("kernel", "calls", "avg us", "min us", "max us")]
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name = row["Name"].split("(")[0][:48]
            lines.append("  %-48s %7s %10.2f %10.2f %10.2f" % (name, row["Calls"], float(row["AverageNs"]) / 1e3,
                                                            float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.child:                                   # the profiled process: the torch route at cfg3 only
        step = torch_step(32, dev)
        for _ in range(20 + a.steps):
            step()
        torch.cuda.synchronize()
        return
    lines = ["torch_step_time: forward + backward per step, synth 128x416, 2 sources, 4 scales, L1 + SSIM 0.15 + 2nd-order smoothness 0.1",
             "%s, torch %s; %d steps per repetition, median of 5 (HIP events min..max)" % (
                 torch.cuda.get_device_name(dev), torch.__version__, a.steps)]
    for B, name in ((4, "B=4 (the reference's batch)"), (32, "cfg3 (B=32)")):
        res = {}
        for route, make in (("torch", torch_step), ("link", link_step), ("manual", manual_step)):
            res[route] = measure(make(B, dev), a.steps)
        seen = []
        ta._desc_hook = seen.append
        step = torch_step(B, dev)
        for _ in range(a.steps):
            step()
        ta._desc_hook = None
        torch.cuda.synchronize()
        lines.append("%s:" % name)
        for route in ("torch", "link", "manual"):
            ev, host, lo, hi = res[route]
            lines.append("  %-6s HIP-event %8.2f us/step (%.2f..%.2f)   host %8.2f us/call" % (route, ev, lo, hi, host))
        for other in ("link", "manual"):
            lines.append("  torch - %s: %+.2f us/step (HIP events), %+.2f us/call (host)" % (
                other, res["torch"][0] - res[other][0], res["torch"][1] - res[other][1]))
        lines.append("  torch route: %d distinct descriptors over %d steps (the plan cache keeps 4)" % (len(set(seen)), len(seen)))
    if a.rocprof:
        lines += rocprof_stats(a.steps, tempfile.mkdtemp(prefix="torch_step_rocprof_"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
