#!/usr/bin/env python3
"""The measurement behind FACTORS of tests/intrinsics_exact_ref.py: knife_free.floor_ratio -- max|gpu - o64| / (max|o32 - o64| +
2.5e-7 max|o64|) -- of every array tests/test_intrinsics_exact_gpu.py compares: d_proj and d_intrinsics of sfm_loss_proj_bwd per
scale, whole and per block, over all cases, configurations, layouts and entry points of both projections; K.grad of the torch
route; d_K of sfm_warp_intrinsics_bwd.  Everything here is bitwise reproducible.  The measurement is against the float64
reference, the yardstick is the float32 reference, never the kernel.

usage: python tools/intrinsics_accuracy.py [--out FILE] [--all]      (--all: one line per array, not only the summary)"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import intrinsics_exact_ref as X  # noqa: E402
import test_intrinsics_exact_gpu as T  # noqa: E402
from knife_free import floor_ratio  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("intrinsics_accuracy: needs a GPU")
    ops = importlib.import_module("sfm-learner-chainer_amd.ops")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("the intrinsics gradient against the float64 reference, %s" % torch.cuda.get_device_name(0))
    say("floor_ratio = max|gpu - o64| / (max|o32 - o64| + 2.5e-7 max|o64|) per array and scale")
    worst, count = {}, {}
    for regime, what, kind, name, got, a64, a32 in T.every_row(ops, dev):
        r = floor_ratio(got, a64, a32)
        count[regime] = count.get(regime, 0) + 1
        if a.all:
            say("%-14s %-86s %-26s %.3f" % (regime, what, name, r))
        if r > worst.get((regime, kind), (-1.0, ""))[0]:
            worst[(regime, kind)] = (r, "%s %s" % (what, name))
    for regime in X.REGIMES:
        say()
        say("%s: %d arrays; the largest ratio per kind, and 4 x it rounded up to a power of two (at least 4)" % (regime, count.get(regime, 0)))
        for kind in X.KINDS:
            if (regime, kind) in worst:
                r, what = worst[(regime, kind)]
                fixed = regime == "reference_order" and kind in ("d_proj", "d_K")
                say("  %-11s %7.3f  -> %3s   (%s)" % (kind, r, "K_REF = 4, not derived" if fixed else X.derived_factor(r), what))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
