#!/usr/bin/env python3
"""Writes plan_table.npz: what the host side of the fused loss decides for a fixed grid of descriptors -- workspace size and, for
each of the three entry points, return code, items, per-scale strips / chunks / rows / tiles, kernel family and resident waves per
SIMD (sfm_loss_plan_info) -- plus a short list of descriptors the library rejects, with the code each returns.

Nothing is launched: the descriptors bind fake non-NULL pointers (as tools/show_plan.py does).  Run it without a GPU and with no
SFM_* variable set (the library then plans for 256 CUs, the MI355X's count).  The committed file pins the selection logic of the
commit that introduced it; tests/test_plan_cpu.py compares the library with it integer for integer.  Regenerate it only in a
change that alters the plan on purpose, and say why.

usage: python tests/golden/make_plan_table.py [out.npz]"""
import ctypes as C
import importlib
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
_lib = importlib.import_module("sfm-learner-chainer_amd._lib")

FAKE = 0x1000                                      # never dereferenced
ENTRIES = ((0, 1), (1, 0), (1, 1))                 # (grad, loss): sfm_loss_fwd, sfm_loss_bwd, sfm_loss_fwd_bwd
MAX_S = 4                                          # scales of the largest frame of the grid
ENTRY_COLS = 2 + 4 * MAX_S + 2                     # rc, items, 4 ints per scale (0 beyond n_scales), family, waves per SIMD
FAMILIES = ("base", "wide", "pair", "reference order", "d_src")

FRAMES = ((128, 416, 4), (256, 832, 4), (64, 208, 3), (37, 53, 2))       # H, W, scales
BATCHES = (1, 4, 7, 8, 11, 16, 24, 32, 48)
N_SRC = (1, 2, 4)
MODES = ("l1", "ssim", "explain")
SMOOTH = (0, 1, 2)
LAYOUTS = (0, 1)                                   # planar, pixel-interleaved
PROJECTIONS = (0, 1)                               # fast, reference order
D_SRC = (0, 1)
WARPED = (0, 1)
PARAMS = ("frame", "B", "n_src", "mode", "smooth_mode", "layout", "projection", "d_src", "warped")


def grid():
    return itertools.product(range(len(FRAMES)), BATCHES, N_SRC, range(len(MODES)), SMOOTH, LAYOUTS, PROJECTIONS, D_SRC, WARPED)


def desc(frame=0, B=4, n_src=2, mode=1, smooth_mode=1, layout=1, projection=0, d_src=0, warped=0):
    H, W, S = FRAMES[frame]
    d = _lib.SfmLossDesc()
    d.B, d.norm_B, d.n_src, d.n_scales = B, max(B, 1), n_src, S
    d.ssim_rate = 0.15 if MODES[mode] == "ssim" else 0.0
    d.exp_reg = 0.2 if MODES[mode] == "explain" else 0.0
    d.smooth_reg, d.smooth_mode = 0.1, smooth_mode
    d.image_layout, d.projection = layout, projection
    d.intrinsics = FAKE
    for s in range(S):
        d.H[s], d.W[s] = H >> s, W >> s
        d.tgt[s] = d.src[s] = d.disp[s] = d.d_disp[s] = FAKE
        if MODES[mode] == "explain":
            d.mask_logits[s] = d.d_mask[s] = FAKE
        if d_src:
            d.d_src[s] = FAKE
        if warped:
            d.warped[s] = FAKE
    for i in range(n_src):
        d.pose[i] = d.d_pose[i] = FAKE
    return d


def describe(p):
    H, W, S = FRAMES[p[0]]
    return "%dx%dx%d scales, B=%d, n_src=%d, %s, smooth_mode=%d, layout=%d, projection=%d, d_src=%d, warped=%d" % (
        H, W, S, p[1], p[2], MODES[p[3]], p[4], p[5], p[6], p[7], p[8])


def row(d):
    """workspace bytes, and ENTRY_COLS ints per entry point"""
    n = d.n_scales
    out = (C.c_int * (1 + 4 * n + 2))()
    r = np.zeros(len(ENTRIES) * ENTRY_COLS, np.int32)
    for e, (grad, loss) in enumerate(ENTRIES):
        o = r[e * ENTRY_COLS:(e + 1) * ENTRY_COLS]
        o[0] = _lib.lib.sfm_loss_plan_info(C.byref(d), grad, loss, out, len(out))
        if o[0] == 0:
            o[1] = out[0]
            o[2:2 + 4 * n] = out[1:1 + 4 * n]
            o[2 + 4 * MAX_S:] = out[1 + 4 * n:]
    return int(_lib.lib.sfm_loss_workspace_bytes(C.byref(d))), r


def _some(d, field, scales):
    for s in scales:
        getattr(d, field)[s] = FAKE


def rejected():
    """(what, descriptor): each has ONE fault; the code is what sfm_loss_fwd returns (it validates before it touches the GPU)"""
    def mk(what, **kw):
        d = desc(frame=3, mode=0)
        for k, v in kw.items():
            setattr(d, k, v)
        return what, d
    cases = [mk("n_src = 0", n_src=0), mk("n_scales = 9", n_scales=9), mk("norm_B < B", norm_B=3), mk("image_layout = 5", image_layout=5),
             mk("projection = 2", projection=2), mk("smooth_mode = 7", smooth_mode=7), mk("exp_reg > 0 without logits", exp_reg=0.2)]
    what, d = mk("H < 3")
    d.H[1] = 2
    cases.append((what, d))
    what, d = mk("HWC scale of 2^24 / 12 pixels or more", n_scales=1, image_layout=1)
    d.H[0], d.W[0] = 1200, 1200
    cases.append((what, d))
    what, d = mk("warped bound for some scales only")
    _some(d, "warped", [0])
    cases.append((what, d))
    return cases


def tables():
    params = np.array(list(grid()), np.int16)
    ws = np.zeros(len(params), np.int64)
    rows = np.zeros((len(params), len(ENTRIES) * ENTRY_COLS), np.int32)
    for k, p in enumerate(params):
        ws[k], rows[k] = row(desc(*(int(v) for v in p)))
    rej = rejected()
    codes = np.array([_lib.lib.sfm_loss_fwd(C.byref(d), None, None, 0, None) for _, d in rej], np.int32)
    return dict(params=params, workspace_bytes=ws, rows=rows, rejected=np.array([w for w, _ in rej]), rejected_codes=codes)


if __name__ == "__main__":
    assert not [k for k in os.environ if k.startswith("SFM_")], "generate the table with no SFM_* variable set"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "plan_table.npz")
    t = tables()
    np.savez_compressed(path, **t)
    fam = t["rows"].reshape(len(t["rows"]), len(ENTRIES), ENTRY_COLS)[:, :, -2]
    print("%d descriptors, %d rejected, %d bytes; families %s" % (len(t["rows"]), len(t["rejected"]), os.path.getsize(path),
                                                                    dict(zip(FAMILIES, np.bincount(fam.ravel(), minlength=5)))))
