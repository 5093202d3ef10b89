#!/usr/bin/env python3
"""A handful of fused steps that also leave d_intrinsics (for rocprofv3 --kernel-trace --stats over proj_bwd_kernel, the launch of
sfm_loss_proj_bwd): tools/intrinsics_once.py [workload] [steps] [batch]"""
import importlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bench = importlib.import_module("bench")
PKG = "sfm-learner-chainer_amd"
ops = importlib.import_module(PKG + ".ops"); synth = importlib.import_module(PKG + ".synth")
dev = torch.device("cuda", 0)
wl = sys.argv[1] if len(sys.argv) > 1 else "cfg3_edge"
R = bench.Runner(torch, np, ops, synth, dev, wl, "hwc", "fused", batch=int(sys.argv[3]) if len(sys.argv) > 3 else 0)
tgt, src, K, disps, poses, masks = R.fl._keep
R.fl = ops.FusedLoss(**R.cfg).bind(tgt, src, K, disps, poses, masks, norm_B=R.B, layout="hwc", want_d_intrinsics=True)
for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 50):
    R.step()
torch.cuda.synchronize()
assert bool(torch.isfinite(R.fl.d_intrinsics).all())
