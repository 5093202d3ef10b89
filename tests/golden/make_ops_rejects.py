#!/usr/bin/env python3
"""Writes ops_rejects.json: what the operator entry points of include/sfmwarp.h (everything outside sfm_loss_* / sfm_step_*)
answer to arguments they reject, and to the accepted calls that return before any launch -- each row a list
[entry point, arguments, return code, sfm_last_error() text].  ENTRIES are the entry points the table holds; the few whose
rejections are pinned in a CPU test file of their own are listed in PINNED_ELSEWHERE.

Arguments are written as JSON: an int for an int / size_t, null or FAKE for a pointer, null or a list for an array of pointers
(0 = a NULL element) or of lengths, null or a dict of field values for a descriptor (a pointer field: 0 = NULL; an array field: a
list, the rest of the array zero).  Nothing is launched and no pointer is dereferenced: would_launch() restates the validation of
each entry point, and a row whose arguments would pass it with work to do is refused before the library sees it.  Before every
call the last error is set to SENTINEL (a rejected sfm_pyramid_variant), so the text of an accepted call is SENTINEL: accepted
calls leave the message alone.

Run it without a GPU.  The committed file pins return codes, message texts and the ORDER of the checks of the commit that
introduced it; tests/test_ops_rejects_cpu.py replays it against the library as built.  Regenerate it only in a change that alters
a message or a bound on purpose, and say why.

usage: python tests/golden/make_ops_rejects.py [out.json]"""
import ctypes as C
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
_lib = importlib.import_module("sfm-learner-chainer_amd._lib")

FAKE = 64                                          # never dereferenced
P8 = [FAKE] * 8                                    # an array of eight bound pointers
SENTINEL_VARIANT = 7                               # sfm_pyramid_variant(7) is rejected: its message is the sentinel
ALIGNED = 256                                      # a workspace address the library takes; never dereferenced either
# operator entry points whose rejections are pinned by the CPU tests of their own feature instead of this table
PINNED_ELSEWHERE = {
    "sfm_resize_bwd": "tests/test_resize_bwd_cpu.py",
    "sfm_warp_intrinsics_bwd": "tests/test_intrinsics_grad_cpu.py",
    "sfm_warp_intrinsics_bwd_workspace_bytes": "tests/test_intrinsics_grad_cpu.py",
    "sfm_pose_proj_bwd_k": "tests/test_intrinsics_grad_cpu.py",
}
SIZES = ("sfm_warp_bwd_workspace_bytes", "sfm_warp_pyramid_bwd_workspace_bytes")      # answer a size_t, not a code


def _pyramid(ys, N, images, H, W, S, first):
    """ys: the arrays of output pointers; images: planes or images per launch; first: the first scale that is written"""
    if not (all(y is not None for y in ys) and 1 <= S <= 8 and N >= 1 and H >= 1 and W >= 1 and images <= 65535 and S > first):
        return False
    return all(y[s] for y in ys for s in range(first, S)) and \
        all((H >> s) >= 1 and (W >> s) >= 1 and (H >> s) * (W >> s) < 2 ** 31 for s in range(first, S))


def _sampler(a, n_ptr, N, C_, H, W, oH, oW):
    return all(a[:n_ptr]) and 1 <= N <= 65535 and C_ >= 1 and H >= 1 and W >= 1 and oH >= 0 and oW >= 0 and \
        C_ * H * W < 2 ** 31 and C_ * oH * oW < 2 ** 31


def _warp(a, ptrs, N, C_, H, W, depth_rows):
    return all(ptrs) and 1 <= N <= 65535 and C_ >= 1 and H >= 3 and W >= 3 and C_ * H * W < 2 ** 31 and depth_rows in (1, 3)


def _arrays(a, arrays, numel, n, n_max):
    if not (all(a[k] is not None for k in arrays) and a[numel] is not None and 1 <= n <= n_max):
        return False
    ln = a[numel][:n]
    return all(v >= 0 for v in ln) and all(a[k][i] for k in arrays for i, v in enumerate(ln) if v > 0) and 0 < sum(ln) < 2 ** 40


def _pyramid_desc(d, count, tiles, setting, inputs, outputs, per_image=()):
    """The checks the two descriptor entry points share (check_pyramid_shape of csrc/sfm_common.h, then the setting and the
    pointers): True if a launch follows.  count: the per-sample count's field; tiles(H, W): the launch units of one image set of a
    scale; inputs / outputs: the per-scale pointer fields that must be bound; per_image: the per-image ones."""
    if d is None or not (1 <= d[count] <= 8 and 1 <= d["n_scales"] <= 8 and d["B"] >= 0):
        return False
    S, total = d["n_scales"], 0
    H, W = (d["H"] + [0] * 8)[:S], (d["W"] + [0] * 8)[:S]
    for h, w in zip(H, W):
        if h < 3 or w < 3 or 3 * h * w >= 2 ** 31:
            return False
        total += d["B"] * tiles(h, w)
        if total >= 2 ** 31:
            return False
    if not setting(d) or d["B"] == 0:
        return False
    bound = lambda f, n: all((d[f] + [0] * 8)[:n])
    return all(bound(f, S) for f in inputs + outputs) and all(bound(f, d[count]) for f in per_image)


def warp_pyramid_blocks(H, W):
    return (H * W + 255) // 256


def photo_error_tiles(H, W, n_img, bwd):
    strip = 60 if bwd else 62
    return n_img * ((W + strip - 1) // strip) * ((H + 15) // 16)


def _warp_pyramid(d, bwd):
    return _pyramid_desc(d, "n_src", warp_pyramid_blocks, lambda d: d["image_layout"] in (0, 1) and bool(d["intrinsics"]), ["src", "disp"],
                         ["g_warped", "d_disp"] if bwd else ["warped"], ["pose"] + (["d_pose"] if bwd else []))


def warp_pyramid_ws_bytes(d):
    need = sum(d["B"] * warp_pyramid_blocks(h, w) for h, w in zip(d["H"][:d["n_scales"]], d["W"])) * d["n_src"] * 48
    return (need + 255) // 256 * 256 if need else 256


def _photo_error(d, bwd):
    return _pyramid_desc(d, "n_img", lambda h, w: photo_error_tiles(h, w, d["n_img"], bwd), lambda d: 0.0 <= d["ssim_rate"] <= 1.0,
                         ["img", "tgt"], ["g_err", "d_img"] if bwd else ["err"])


def would_launch(name, a):
    """True if the library would pass these arguments on to HIP (a kernel launch or a memset): the validation of csrc/sfm_ops.hip,
    csrc/sfm_warp_pyramid.hip and csrc/sfm_photo_error.hip, restated.  Such a row has no place in the table: its fake pointers
    would be used."""
    if name in ("sfm_pyramid_variant",) + SIZES:
        return False
    if name == "sfm_warp_pyramid_fwd":
        return _warp_pyramid(a[0], False)
    if name == "sfm_warp_pyramid_bwd":
        return _warp_pyramid(a[0], True) and bool(a[1]) and a[1] % 256 == 0 and a[2] >= warp_pyramid_ws_bytes(a[0])
    if name in ("sfm_photo_error_fwd", "sfm_photo_error_bwd"):
        return _photo_error(a[0], name.endswith("bwd"))
    if name in ("sfm_pose_proj_fwd", "sfm_pose_proj_bwd"):
        return all(a[:-2]) and a[-2] > 0
    if name == "sfm_warp_fwd":
        return _warp(a, a[:2] + a[3:6], *a[6:10], a[2])
    if name == "sfm_warp_bwd":
        N, C_, H, W = a[11:15]
        return _warp(a, a[:2] + a[3:8], N, C_, H, W, a[2]) and bool(a[9]) and a[10] >= N * ((H * W + 255) // 256) * 48
    if name in ("sfm_sampler_fwd", "sfm_sampler_interp_fwd"):
        return _sampler(a, 3, *a[3:9]) and a[7] * a[8] > 0
    if name == "sfm_sampler_bwd":
        return _sampler(a, 4, *a[5:11]) and a[9] * a[10] > 0 and (a[9] + 31) // 32 <= 65535
    if name == "sfm_sampler_interp_bwd":                       # (zero-fills gx before it looks at the output size)
        return _sampler(a, 4, *a[5:11]) and (bool(a[4]) or a[9] * a[10] > 0)
    if name == "sfm_resize_fwd":
        return all(a[:2]) and a[2] >= 1 and all(v >= 1 for v in a[3:8]) and a[2] * a[3] <= 65535
    if name == "sfm_pyramid_fwd":
        return bool(a[0]) and a[3] >= 1 and _pyramid([a[1]], a[2], a[2] * a[3], a[4], a[5], a[6], 1)
    if name == "sfm_pyramid_hwc_fwd":
        return bool(a[0]) and a[3] >= 1 and _pyramid([a[1]], a[2], a[2] * a[3], a[4], a[5], a[6], 0)
    if name == "sfm_pyramid_pair_hwc_fwd":
        return all(a[:2]) and 1 <= a[5] <= 8 and _pyramid(a[2:4], a[4], a[4] * (1 + a[5]), a[6], a[7], a[8], 0)
    if name == "sfm_augment_fwd":
        return all(a[:3]) and all(v >= 1 for v in a[3:8]) and a[3] * a[4] * a[5] <= 65535
    if name == "sfm_disp_act_fwd":
        return _arrays(a, [0, 1], 2, a[3], 8)
    if name == "sfm_disp_act_bwd":
        return _arrays(a, [0, 1, 2], 3, a[4], 8)
    if name == "sfm_scale_arrays":
        return bool(a[4]) and _arrays(a, [0, 1], 2, a[3], 32)
    raise KeyError(name)


def call(name, args):
    """-> (return code, sfm_last_error() text) of entry point `name` on the JSON arguments `args`"""
    assert not would_launch(name, args), "%s%r would reach a launch" % (name, tuple(args))
    res, types = _lib.SYMBOLS[name]
    assert len(args) == len(types), (name, args)
    conv, keep = [], []
    for v, t in zip(args, types):
        if t is C.c_void_p:
            conv.append(C.c_void_p(v) if v else None)
        elif t in (C.c_int, C.c_size_t):
            conv.append(v)
        elif v is None:
            conv.append(None)
        elif isinstance(v, dict):
            desc = t._type_()
            for field, value in v.items():
                if isinstance(value, list):
                    for k, e in enumerate(value):
                        getattr(desc, field)[k] = e or None if getattr(desc, field)._type_ is C.c_void_p else e
                else:
                    setattr(desc, field, value)
            keep.append(desc)
            conv.append(C.byref(desc))
        else:
            arr = (t._type_ * len(v))(*[e or None for e in v] if t._type_ is C.c_void_p else v)
            keep.append(arr)
            conv.append(arr)
    assert _lib.lib.sfm_pyramid_variant(SENTINEL_VARIANT) == _lib.ERR_CONFIG
    rc = getattr(_lib.lib, name)(*conv)
    assert rc <= 0 or name in SIZES, "%s%r launched: %d %s" % (name, tuple(args), rc, _lib.last_error())
    return int(rc), _lib.last_error()


def _each_null(name, good, pointers):
    """`good` with each of the pointer arguments NULL in turn"""
    return [(name, good[:k] + [None] + good[k + 1:]) for k in pointers]


def cases():
    F, out = FAKE, []
    add = lambda name, *rows: out.extend((name, list(r)) for r in rows)

    add("sfm_pyramid_variant", [-1], [2], [1], [0])
    add("sfm_warp_bwd_workspace_bytes", [0, 16, 24], [-1, 16, 24], [2, 0, 24], [2, 16, -1], [2, 16, 24], [1, 1, 1])

    for name, n in (("sfm_pose_proj_fwd", 3), ("sfm_pose_proj_bwd", 4)):
        out += _each_null(name, [F] * n + [1, None], range(n))
        add(name, [None] * n + [0, None], [F] * n + [-1, None], [None] * n + [-1, None])       # empty; N < 0; NULL fires before N < 0

    # sfm_warp_fwd: src, depth, depth_rows, pose6, K, warped, N, C, H, W, stream.  depth_rows is the LAST check: depth_rows = 2
    # behind a bound at its edge shows that the bound let it through
    w = lambda depth_rows=1, N=1, C_=3, H=8, W=8, p=F: [p, p, depth_rows, p, p, p, N, C_, H, W, None]
    out += _each_null("sfm_warp_fwd", w(), (0, 1, 3, 4, 5))
    add("sfm_warp_fwd", w(N=0, p=None), w(N=-1), w(N=-1, p=None), w(N=65536), w(N=65535, depth_rows=2), w(N=65536, C_=0),
        w(C_=0), w(C_=0, H=2), w(H=2), w(W=2), w(H=3, W=3, depth_rows=2), w(H=2, depth_rows=2), w(C_=2, H=32768, W=32768),
        w(C_=1, H=32768, W=65535, depth_rows=2), w(C_=2, H=32768, W=32768, depth_rows=2), w(depth_rows=2), w(depth_rows=0))

    # sfm_warp_bwd: src, depth, depth_rows, pose6, K, g_warped, d_depth, d_pose6, d_src, ws, ws_bytes, N, C, H, W, stream.
    # the workspace is the last check
    def wb(depth_rows=1, N=1, C_=3, H=8, W=8, p=F, d_src=None, ws=F, short=1):
        need = max(N, 0) * ((H * W + 255) // 256) * 48
        return [p, p, depth_rows, p, p, p, p, p, d_src, ws, max(need - short, 0), N, C_, H, W, None]
    out += _each_null("sfm_warp_bwd", wb(), (0, 1, 3, 4, 5, 6, 7))
    add("sfm_warp_bwd", wb(N=0, p=None, ws=None), wb(N=-1), wb(N=-1, p=None), wb(N=65536), wb(N=65535), wb(C_=0), wb(H=2), wb(W=2),
        wb(H=3, W=3), wb(H=2, depth_rows=2), wb(C_=2, H=32768, W=32768), wb(C_=1, H=32768, W=65535), wb(depth_rows=2),
        wb(depth_rows=2, ws=None), wb(ws=None, short=0), wb(d_src=F), wb(H=16, W=24, N=2))

    # the four samplers: x, grid, [gy, ggrid, gx,] N, C, H, W, oH, oW, stream.  An empty output (oH = 0) is accepted without a launch
    for name, n in (("sfm_sampler_fwd", 3), ("sfm_sampler_interp_fwd", 3), ("sfm_sampler_bwd", 4), ("sfm_sampler_interp_bwd", 4)):
        def s(N=1, C_=3, H=8, W=8, oH=0, oW=8, p=F, n=n):
            return [p] * n + ([None] if n == 4 else []) + [N, C_, H, W, oH, oW, None]
        out += _each_null(name, s(), range(n))
        add(name, s(N=0, p=None), s(N=-1), s(N=-1, p=None), s(N=65535), s(N=65536), s(N=65536, C_=0), s(C_=0), s(H=0), s(W=0),
            s(oH=-1), s(oW=-1), s(oH=0, oW=0), s(oH=4, oW=0), s(C_=2, H=1 << 30, W=1), s(C_=2 ** 31 - 1, H=1, W=1),
            s(C_=2, H=1, W=1, oH=1 << 30, oW=1), s(C_=0, H=1 << 30, W=4))
    add("sfm_sampler_bwd", [F] * 5 + [1, 1, 8, 8, 2097121, 1, None], [F] * 5 + [65536, 1, 8, 8, 2097121, 1, None],
        [F] * 5 + [1, 3, 8, 8, 0, 8, None])

    # sfm_resize_fwd: x, y, N, C, H, W, oH, oW, stream
    r = lambda N=1, C_=3, H=8, W=8, oH=4, oW=4, p=F: [p, p, N, C_, H, W, oH, oW, None]
    out += _each_null("sfm_resize_fwd", r(), (0, 1))
    add("sfm_resize_fwd", r(N=0, p=None), r(N=-1), r(N=-1, p=None), r(C_=0), r(H=0), r(W=0), r(oH=0), r(oW=0), r(N=65536, C_=1),
        r(N=21846, C_=3), r(N=65536, C_=1, oH=0), r(N=65536, C_=0))

    # sfm_pyramid_fwd: x, y, N, C, H, W, n_scales, stream (y[0] is ignored; n_scales = 1 has nothing to do)
    y0 = [0] + [F] * 7
    p = lambda y=P8, N=1, C_=3, H=16, W=16, S=4, x=F: [x, y, N, C_, H, W, S, None]
    add("sfm_pyramid_fwd", p(x=None), p(y=None), p(x=None, y=None, N=0), p(N=-1), p(S=0), p(S=9), p(S=9, N=65536), p(S=1), p(S=1, y=[0] * 8),
        p(S=1, N=21845), p(S=1, N=21846), p(S=1, N=65535, C_=1), p(S=1, N=65536, C_=1), p(S=1, C_=0), p(S=1, H=0), p(S=1, W=0),
        p(S=8, y=[F, 0] + [F] * 6), p(S=8, y=[F, 0] + [F] * 6, N=21845), p(S=8, H=255, W=255, y=[F] * 7 + [0]), p(y=y0, H=4), p(y=y0, H=16, W=4),
        p(H=4, y=[F, F, F, 0]), p(H=4, y=[F, F, 0, F]), p(S=8, H=64, W=128, y=y0), p(S=2, H=1, W=1, y=y0))

    # sfm_pyramid_hwc_fwd: x, y, N, G, H, W, n_scales, stream (scale 0 is written too)
    add("sfm_pyramid_hwc_fwd", p(x=None), p(y=None), p(x=None, y=None, N=0), p(N=-1), p(S=0), p(S=9), p(S=9, N=65536), p(C_=0), p(H=0), p(W=0),
        p(N=65536, C_=1), p(N=21846), p(N=21845, y=y0), p(N=65535, C_=1, y=y0), p(S=1, y=y0), p(S=8, y=[F, 0] + [F] * 6),
        p(S=8, H=255, W=255, y=[F] * 7 + [0]), p(H=4), p(H=16, W=4), p(H=4, y=[F, F, F, 0]), p(S=8, H=64, W=128), p(S=2, H=1, W=1),
        p(S=1, H=65536, W=65536), p(S=1, H=32768, W=65536), p(S=2, H=32768, W=65535, y=[F, 0] + [F] * 6), p(S=1, H=65536, W=65536, y=y0))

    # sfm_pyramid_pair_hwc_fwd: tgt, src, y_tgt, y_src, N, n_src, H, W, n_scales, stream
    def pp(N=1, n_src=2, H=16, W=16, S=4, tgt=F, src=F, y_tgt=P8, y_src=P8):
        return [tgt, src, y_tgt, y_src, N, n_src, H, W, S, None]
    add("sfm_pyramid_pair_hwc_fwd", pp(tgt=None), pp(src=None), pp(y_tgt=None), pp(y_src=None), pp(N=0, tgt=None, src=None, y_tgt=None, y_src=None),
        pp(N=-1), pp(S=0), pp(S=9), pp(S=9, n_src=0), pp(n_src=0), pp(n_src=9), pp(n_src=8, y_tgt=y0), pp(H=0), pp(W=0), pp(N=21846),
        pp(N=21845, y_tgt=y0), pp(N=21845, y_src=y0), pp(N=7282, n_src=8), pp(N=7281, n_src=8, y_src=y0), pp(N=65535, n_src=1),
        pp(S=1, y_tgt=y0, y_src=y0), pp(S=8, y_src=[F, 0] + [F] * 6), pp(H=4), pp(H=16, W=4), pp(H=4, y_tgt=[F, F, F, 0]), pp(S=2, H=1, W=1),
        pp(S=1, H=65536, W=65536), pp(S=1, H=32768, W=65536), pp(S=2, H=32768, W=65535, y_tgt=[F, 0] + [F] * 6))

    # sfm_augment_fwd: imgs, params, out, B, F, C, H, W, stream
    a = lambda B=1, F_=3, C_=3, H=8, W=8, q=F: [q, q, q, B, F_, C_, H, W, None]
    out += _each_null("sfm_augment_fwd", a(), range(3))
    add("sfm_augment_fwd", a(B=0, q=None), a(B=-1), a(B=-1, q=None), a(F_=0), a(C_=0), a(H=0), a(W=0), a(B=65536, F_=1, C_=1),
        a(B=7282), a(B=16, F_=64, C_=64))

    # sfm_disp_act_fwd: x, disp, numel, n_scales, stream ; sfm_disp_act_bwd: disp, g_disp, g_x, numel, n_scales, stream
    Z8, N8 = [0] * 8, [0] * 8
    for name, n in (("sfm_disp_act_fwd", 2), ("sfm_disp_act_bwd", 3)):
        d = lambda numel=Z8, S=4, arr=P8, n=n: [arr] * n + [numel, S, None]
        out += _each_null(name, d(), range(n + 1))
        add(name, d(arr=N8), d(S=1), d(S=8), d(S=0), d(S=9), d(S=-1), d(numel=None, S=9), d(numel=[0, -1, 0, 0]), d(numel=[0, 0, 0, -1], arr=N8),
            d(numel=[5, 0, 0, 0], arr=N8), d(numel=[-1, 0, 0, 0], arr=N8), d(numel=[0, 5, -1, 0], arr=[F, 0, F, F]), d(numel=[0, 0, 5, 0], arr=[F, F, 0, F]),
            d(numel=[1 << 40, 0, 0, 0]), d(numel=[1 << 39, 1 << 39, 0, 0]), d(numel=[1 << 40, -1, 0, 0]), d(numel=[1 << 40, 5, 0, 0], arr=[F, 0, F, F]))
    add("sfm_disp_act_bwd", [P8, N8, P8, [0, 5, 0, 0], 4, None])

    # sfm_scale_arrays: x, y, numel, n, gy, stream
    P4, Z4, P33, Z33 = [F] * 4, [0] * 4, [F] * 33, [0] * 33
    sc = lambda x=P4, y=P4, numel=Z4, n=4, gy=F: [x, y, numel, n, gy, None]
    add("sfm_scale_arrays", sc(x=None), sc(y=None), sc(numel=None), sc(gy=None), sc(n=0), sc(n=33), sc(n=-1), sc(n=1), sc(n=32, x=P33, y=P33, numel=Z33),
        sc(n=32, x=Z33, y=Z33, numel=Z33), sc(n=33, gy=None), sc(n=33, x=None), sc(n=0, gy=None), sc(gy=None, numel=[-1] * 4), sc(numel=[0, 0, 0, -1]),
        sc(numel=[0, 0, 0, -1], x=Z4), sc(numel=[0, 0, 3, 0], x=Z4), sc(numel=[0, 0, 3, 0], y=Z4), sc(numel=[0, 3, -1, 0], y=[F, 0, F, F]),
        sc(numel=[-1, 3, 0, 0], y=[F, 0, F, F]), sc(x=P33, y=P33, numel=[0] * 31 + [-1], n=32), sc(x=P33, y=P33, numel=[0] * 31 + [-1], n=31))
    return out + _descriptor_cases()


def _without(d, field, k=None):
    """the descriptor `d` with pointer `field` (its element k) NULL"""
    return dict(d, **{field: 0 if k is None else d[field][:k] + [0] + d[field][k + 1:]})


def _descriptor_cases():
    """sfm_warp_pyramid_* and sfm_photo_error_*: (descriptor, [ws, ws_bytes,] stream).  Both check the counts, B, then per scale
    the shape and the running launch-unit count, then their setting (image_layout / ssim_rate), return for an empty batch, and only
    then look at the pointers.  A bound at its edge is shown to pass by the NEXT fault of the same call: a bad setting behind a
    shape, a NULL pointer behind the setting."""
    F, out = FAKE, []
    add = lambda name, *rows: out.extend((name, list(r)) for r in rows)
    n8 = lambda n: min(max(n, 0), 8)
    BIG = (32768, 21845)                           # 3*H*W = 2^31 - 32768: the largest frame of this aspect

    def wp(B=1, n_src=2, S=2, H=(8, 4), W=(8, 3), layout=0, p=F, **over):
        d = dict(B=B, n_src=n_src, n_scales=S, H=list(H), W=list(W), image_layout=layout, src=[p] * n8(S), disp=[p] * n8(S), intrinsics=p,
                 pose=[p] * n8(n_src), warped=[p] * n8(S), valid=[0] * n8(S), g_warped=[p] * n8(S), d_disp=[p] * n8(S), d_pose=[p] * n8(n_src))
        return dict(d, **over)

    def shapes(mk, bad):
        """the rows both descriptors share; `bad`: a setting past its bound (the check behind the shapes)"""
        one = 2 ** 31 // 3
        return [None, mk(**{mk.count: 0}), mk(**{mk.count: 9}), mk(**{mk.count: -1}), mk(**{mk.count: 1, **bad}), mk(**{mk.count: 8, **bad}),
                mk(S=0), mk(S=9), mk(S=-1), mk(S=1, **bad), mk(S=8, H=[8] * 8, W=[8] * 8, **bad), mk(**{mk.count: 0, "S": 0}),
                mk(**{mk.count: 9, "B": -1}), mk(S=9, B=-1), mk(B=-1), mk(B=-1, H=(2, 4)), mk(B=-1, p=0),
                mk(H=(2, 4)), mk(W=(2, 4)), mk(H=(8, 2)), mk(W=(8, 2)), mk(H=(3, 3), W=(3, 3), **bad), mk(H=(2, 2)), mk(H=(8, 2), **bad),
                mk(H=(0, 4)), mk(W=(8, -1)), mk(S=1, H=(8, 2), **bad),
                mk(S=1, H=BIG[:1], W=(BIG[1] + 1,)), mk(S=1, H=BIG[:1], W=BIG[1:], **bad), mk(H=(8, BIG[0]), W=(8, BIG[1] + 1)),
                mk(H=(2, BIG[0]), W=(8, BIG[1] + 1)), mk(S=1, H=(one + 1,), W=(1,)), mk(S=1, H=(3,), W=(one + 1,)), mk(S=1, H=(3,), W=(one // 3 + 1,)),
                mk(S=1, H=(65536,), W=(65536,)), mk(B=0, S=1, H=BIG[:1], W=(BIG[1] + 1,)), mk(B=0, p=0), mk(B=0), mk(B=0, **bad), mk(B=0, p=0, **bad),
                mk(B=0, S=8, H=[3] * 8, W=[3] * 8, p=0, **{mk.count: 8})]
    wp.count = "n_src"

    def overflow(mk, per, **kw):
        """the running count of launch units at 2^31 - 1 and one past it: in one scale, and summed over two; `per`: one image set"""
        edge = (2 ** 31 - 1) // per
        half = (2 ** 31 - 1) // (2 * per)
        big2 = dict(S=2, H=BIG[:1] * 2, W=BIG[1:] * 2)
        return [mk(B=edge, S=1, H=BIG[:1], W=BIG[1:], p=0, **kw), mk(B=edge + 1, S=1, H=BIG[:1], W=BIG[1:], **kw), mk(B=half, p=0, **big2, **kw),
                mk(B=half + 1, **big2, **kw), mk(B=edge + 1, S=2, H=(BIG[0], 2), W=(BIG[1], 8), **kw), mk(B=2 ** 31 - 1, **kw)]

    # sfm_warp_pyramid_fwd: desc, stream
    nulls = lambda d, fields: [_without(d, "intrinsics")] + [_without(d, f, k) for f in fields for k in range(2)]
    rows = shapes(wp, dict(layout=2)) + overflow(wp, warp_pyramid_blocks(*BIG)) + nulls(wp(), ("src", "disp", "warped", "pose")) + [
        wp(layout=-1), wp(layout=2, p=0), wp(layout=1, intrinsics=0), wp(layout=1, p=0), wp(intrinsics=0, src=[0, 0]), wp(src=[F, 0], disp=[0, F]),
        wp(src=[0, F], disp=[0, F]), wp(disp=[0, F], warped=[0, F]), wp(warped=[F, 0], pose=[0, F]), wp(pose=[0, 0]), wp(S=1, n_src=1, warped=[0], g_warped=[0]),
        wp(S=8, H=[8] * 8, W=[8] * 8, warped=[F] * 7 + [0]), wp(n_src=8, pose=[F] * 7 + [0])]
    add("sfm_warp_pyramid_fwd", *[[d, None] for d in rows])

    # sfm_warp_pyramid_bwd_workspace_bytes: desc -> bytes, 0 for a descriptor sfm_warp_pyramid_bwd refuses (the backward's pointers)
    both = shapes(wp, dict(layout=2)) + overflow(wp, warp_pyramid_blocks(*BIG))
    bwd_nulls = nulls(wp(), ("src", "disp", "g_warped", "d_disp", "pose", "d_pose")) + [
        wp(layout=2, p=0), wp(g_warped=[F, 0], d_disp=[0, F]), wp(g_warped=[0, F], d_disp=[0, F]), wp(d_disp=[F, 0], pose=[0, F]),
        wp(pose=[0, F], d_pose=[0, F]), wp(pose=[F, 0], d_pose=[0, F]), wp(n_src=8, d_pose=[F] * 7 + [0])]
    sizes = [wp(), wp(warped=[0, 0]), wp(B=2), wp(B=3, n_src=3, S=3, H=(16, 8, 4), W=(24, 12, 6)), wp(S=1, H=(3,), W=(3,), n_src=1), wp(S=1, H=(16,), W=(16,)),
             wp(S=1, H=(16,), W=(17,), n_src=8), wp(B=4, S=1, H=(128,), W=(416,), layout=1)]
    add("sfm_warp_pyramid_bwd_workspace_bytes", *[[d] for d in both + bwd_nulls + sizes])

    # sfm_warp_pyramid_bwd: desc, ws, ws_bytes, stream.  The workspace is the last check: its size, then its alignment
    good = wp()
    need = warp_pyramid_ws_bytes(good)
    add("sfm_warp_pyramid_bwd", *[[d, ALIGNED, 1 << 40, None] for d in both + bwd_nulls],
        [good, None, need, None], [good, None, 0, None], [good, ALIGNED, need - 1, None], [good, ALIGNED, 0, None], [good, F, need, None],
        [good, F, need - 1, None], [good, ALIGNED + 4, 1 << 40, None], [wp(warped=[0, 0]), None, need, None], [wp(d_pose=[0, F]), None, 0, None],
        [wp(layout=2), None, 0, None], [wp(B=0, p=0), None, 0, None], [wp(B=0), F, 0, None], [None, None, 0, None])

    # sfm_photo_error_fwd / _bwd: desc, stream
    def pe(B=1, n_img=2, S=2, H=(8, 4), W=(8, 3), ssim_rate=0.15, p=F, **over):
        d = dict(B=B, n_img=n_img, n_scales=S, H=list(H), W=list(W), ssim_rate=ssim_rate, img=[p] * n8(S), tgt=[p] * n8(S), err=[p] * n8(S),
                 g_err=[p] * n8(S), d_img=[p] * n8(S))
        return dict(d, **over)
    pe.count = "n_img"
    for name, bwd, outs in (("sfm_photo_error_fwd", False, ("err",)), ("sfm_photo_error_bwd", True, ("g_err", "d_img"))):
        rows = shapes(pe, dict(ssim_rate=1.5)) + overflow(pe, photo_error_tiles(*BIG, 1, bwd), n_img=1) + overflow(pe, photo_error_tiles(*BIG, 8, bwd), n_img=8) \
            + nulls(pe(), ("img", "tgt") + outs)[1:] + [
            pe(ssim_rate=-0.5), pe(ssim_rate=-1e-6), pe(ssim_rate=1.0 + 2.0 ** -23), pe(ssim_rate=0.0, p=0), pe(ssim_rate=-0.0, p=0), pe(ssim_rate=1.0, p=0),
            pe(ssim_rate=1.0, img=[F, 0]), pe(ssim_rate=2.0, p=0), pe(img=[F, 0], tgt=[0, F]), pe(img=[0, F], tgt=[0, F]), pe(tgt=[0, F], **{outs[0]: [0, F]}),
            pe(**{outs[0]: [F, 0], outs[-1]: [0, F]}), pe(S=8, H=[8] * 8, W=[8] * 8, **{outs[-1]: [F] * 7 + [0]}),
            pe(S=1, H=(3,), W=(3,), n_img=1, **{outs[0]: [0], ("err" if bwd else "g_err"): [0]})]
        add(name, *[[d, None] for d in rows])
    return out


ENTRIES = sorted({name for name, _ in cases()})


def table():
    return [[name, args, *call(name, args)] for name, args in cases()]


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ops_rejects.json")
    t = table()
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in t) + "\n]\n")
    codes = {}
    for r in t:
        codes[r[2]] = codes.get(r[2], 0) + 1
    print("%d rows over %d entry points, %d bytes; return codes %s" % (len(t), len({r[0] for r in t}), os.path.getsize(path), codes))
