#!/usr/bin/env python3
"""The measurement behind K_BLOCK and K_D_SRC of tests/test_warp_exact_gpu.py: knife_free.floor_ratio -- max|gpu - o64| /
(max|numpy32 - o64| + 2.5e-7 max|o64|) -- of every array that module compares, over all its cases and settings: ops.warp_fwd /
ops.warp_bwd, ops.warp_pyramid_fwd / _bwd under every convention, d_T of the pyramid warp and of ops.depth_consistency_bwd.  d_src
is scattered with float atomics (its bits vary from call to call) and is measured over --calls calls; everything else is bitwise
reproducible.  The yardstick is the float32 NumPy reference, never the kernel.

usage: python tools/warp_accuracy.py [--calls 5] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_warp_exact_gpu as T  # noqa: E402
from knife_free import floor_ratio  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("warp_accuracy: needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("the image warps against the float64 reference, %s" % torch.cuda.get_device_name(0))
    say("floor_ratio = max|gpu - o64| / (max|numpy32 - o64| + 2.5e-7 max|o64|) per array; d_src over %d calls per case" % a.calls)
    worst = {}
    for what, kind, name, got, a64, a32 in T.every_row(a.calls):
        r = floor_ratio(got, a64, a32)
        if r > worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (r, what)
        say("%-64s %-22s %-13s %.3f" % (what, name, kind, r))
    say()
    say("largest per kind:")
    for kind, (r, what) in sorted(worst.items()):
        say("  %-13s %.3f   (%s)" % (kind, r, what))
    say()
    for kind in sorted(T.FACTORS):
        k = max(4 * worst[kind][0], 4.0)
        say("%s: max(4 x %.3f, 4) = %.3f -> the next power of two: %d" % (kind, worst[kind][0], k, 2 ** int(np.ceil(np.log2(k)))))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
