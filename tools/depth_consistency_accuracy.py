#!/usr/bin/env python3
"""The measurement behind K_D_SRC_DISP of tests/test_depth_consistency_gpu.py: knife_free.floor_ratio -- max|gpu - o64| /
(max|numpy32 - o64| + 2.5e-7 max|o64|) -- of every gradient array of ops.depth_consistency_bwd over all knife-free cases of
tests/depth_consistency_ref.py and --calls repeated calls (d_src_disp is scattered with float atomics: its bits vary from call to
call; d_disp and d_pose do not, and are listed for comparison).  The yardstick is the float32 NumPy reference, never the kernel.

usage: python tools/depth_consistency_accuracy.py [--calls 5] [--out FILE]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import depth_consistency_ref as R  # noqa: E402
from knife_free import floor_ratio  # noqa: E402

ops = importlib.import_module("sfm-learner-chainer_amd.ops")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_consistency_accuracy: needs a GPU")
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("ops.depth_consistency_bwd against the float64 reference, %s" % torch.cuda.get_device_name(0))
    say("floor_ratio = max|gpu - o64| / (max|numpy32 - o64| + 2.5e-7 max|o64|) per array; %d calls per case" % a.calls)
    worst = {}
    for case in R.CASE_LIST:
        d = R.inputs(*case)
        o64, o32 = R.references(*case)
        args = ([t(x) for x in d["disps"]], [t(x) for x in d["src_disps"]], [t(x) for x in d["poses"]], t(d["intrinsics"]), [t(x) for x in d["g_diff"]])
        for call in range(a.calls):
            parts = []
            d_disps, d_poses, d_srcs = ops.depth_consistency_bwd(*args)
            for key, arrays in (("d_disps", d_disps), ("d_poses", d_poses), ("d_src_disps", d_srcs)):
                r = max(floor_ratio(x.cpu().numpy(), a64, a32) for x, a64, a32 in zip(arrays, o64[key], o32[key]))
                worst[key] = max(worst.get(key, 0.0), r)
                parts.append("%s %.3f" % (key, r))
            say("%-34s call %d: %s" % (R.case_id(case), call, ", ".join(parts)))
    say("largest: " + ", ".join("%s %.3f" % kv for kv in worst.items()))
    k = 4 * worst["d_src_disps"]
    say("d_src_disps: 4 x %.3f = %.3f -> the next power of two: %d" % (worst["d_src_disps"], k, 2 ** int(np.ceil(np.log2(k)))))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
