"""sfm_photo_error_fwd / _bwd and torch_api.photometric_error on the GPU: the L1 + SSIM error map of every (scale, image) of a step in
one launch, its gradient with respect to the images in one more.

The reference is oracle.compute_ssim / compute_ssim_backward plus the L1 terms in fp64 (tests/test_photo_error_cpu.py: `oracle`).
The oracle evaluated in fp32 is one valid fp32 evaluation of the formula; its own distance from fp64 sets the tolerance,
    max |gpu - o64| <= 4 max |o32 - o64| + 1e-6 max |o64|     per array,
the 4 for another, equally valid summation order and contraction (the kernel sums separably and keeps 3x3 sums, the oracle adds nine
terms and divides); a wrong tap, weight or halo is off by 1e-2 and more.  Knife-edge entries leave the BACKWARD comparison only:
those with |e_c| < 1e-5 or |e_c - 1| < 1e-5 (fp64) anywhere in their 3x3 window -- the clip's corners -- and those with
|X_c - Y_c| < 1e-6 themselves -- the corner of |.|; at most 1 % of an array may leave.

Shapes: the smallest at which the kernels can still go wrong.  The tile geometry is read from csrc/sfm_photo_error.hip: rows per
chunk, useful columns of a forward and of a backward strip; the widths are one below, at and one above the first two multiples of
each strip width, the heights lie around the chunk length.

The adjoint identity (forward at X +- eps V contracted with g against <d_img, V> 2 eps, contracted in fp64 on the host from the
GPU's outputs) is held to the same rule: the compared array has one entry per (draw of (V, g), sample, image) and scale -- the
residual of the identity -- and the fp32 oracle's distance from the fp64 oracle over that array is the deviation."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

from test_photo_error_cpu import oracle
from util import Arena, parity_note

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F64 = np.float64
ALPHAS = [0.0, 0.85, 1.0]


def _geometry():
    text = open(os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", "sfm_photo_error.hip")).read()
    return [int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("PE_ROWS", "PE_FWD_STRIP", "PE_BWD_STRIP")]


ROWS, FWD_STRIP, BWD_STRIP = _geometry()


def _around(strip):
    """six scales: widths one below, at and one above the first two multiples of `strip`, heights around the chunk length"""
    return [(ROWS + dh, k * strip + dw) for k in (1, 2) for dh, dw in ((-1, -1), (0, 0), (1, 1))]


# (B, n_img, [(h, w)])
CASES = {
    "3x3": (1, 1, [(3, 3)]),
    "nondyadic": (2, 3, [(17, 61), (9, 31), (5, 16), (3, 8)]),
    "40x130": (2, 2, [(40, 130)]),
    "fwd_strips": (1, 1, _around(FWD_STRIP)),
    "bwd_strips": (1, 1, _around(BWD_STRIP)),
    "two_chunks": (1, 2, [(2 * ROWS - 1, 5), (2 * ROWS, 4), (2 * ROWS + 1, 3)]),
    "max_img": (1, _lib.SFM_MAX_SRC, [(7, 9), (3, 5)]),
}


@pytest.fixture(autouse=True)
def _needs_a_gpu(dev):
    """(the `dev` fixture skips where no GPU is visible)"""


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 host arrays of one case (never modify them): Y a texture as synth makes them -- low-resolution noise upsampled,
    clipped to [-1,1] --, X = Y rolled by two columns plus 0.05 noise, g standard normal"""
    B, n, hw = CASES[name]
    rng = np.random.RandomState(7 + sorted(CASES).index(name))
    X, Y, G = [], [], []
    for h, w in hw:
        tex = 1.4 * synth._smooth_field(rng, B, 3, h, w, 8) + 0.2 * synth._smooth_field(rng, B, 3, h, w, 2)
        y = np.clip(tex, -1, 1).astype(np.float32)
        x = np.stack([np.roll(y, 2, axis=3) + 0.05 * rng.standard_normal(y.shape) for _ in range(n)], axis=1).astype(np.float32)
        X.append(x), Y.append(y), G.append(rng.standard_normal((B, n, h, w)).astype(np.float32))
    return X, Y, G


@functools.lru_cache(maxsize=None)
def reference(name, alpha):
    """per scale: (err64, d64, err32, d32) of the oracle on the float32 inputs"""
    X, Y, G = inputs(name)
    return [oracle(x, y, alpha, g, np.float64) + oracle(x, y, alpha, g, np.float32) for x, y, g in zip(X, Y, G)]


@functools.lru_cache(maxsize=None)
def gpu(name, alpha):
    X, Y, G = inputs(name)
    X, Y, G = [_t(a) for a in X], [_t(a) for a in Y], [_t(a) for a in G]
    return _np(ops.photo_error_fwd(X, Y, alpha)), _np(ops.photo_error_bwd(X, Y, alpha, G))


def _knife(x, y, alpha):
    """the entries (B,n,3,h,w) that leave the backward comparison"""
    x, y = x.astype(F64), y.astype(F64)[:, None]
    out = np.abs(x - y) < 1e-6
    if alpha > 0:
        from test_photo_error_cpu import _pool
        mx, my = _pool(x), _pool(y)
        n1, n2 = 2 * mx * my + 1e-4, 2 * (_pool(x * y) - mx * my) + 9e-4
        d1, d2 = mx * mx + my * my + 1e-4, (_pool(x * x) - mx * mx) + (_pool(y * y) - my * my) + 9e-4
        e = (1 - n1 * n2 / (d1 * d2)) / 2
        near = ((np.abs(e) < 1e-5) | (np.abs(e - 1) < 1e-5)).astype(F64)
        out = out | (_pool(near) > 0)
    return out


def _within(got, o64, o32, what, keep=None):
    """the rule of the module docstring for one array; returns the observed ratio max|gpu - o64| / max|o32 - o64|"""
    keep = np.ones(o64.shape, bool) if keep is None else keep
    assert np.isfinite(got).all(), what
    err = float((np.abs(got.astype(F64) - o64) * keep).max())
    dev = float((np.abs(o32.astype(F64) - o64) * keep).max())
    ratio = err / dev if dev > 0 else (0.0 if err == 0 else float("inf"))
    line = "photo_error %s: max|gpu-o64| %.3g, max|o32-o64| %.3g, ratio %.3g, max|o64| %.3g" % (what, err, dev, ratio, np.abs(o64).max())
    print(line)
    parity_note(line)
    assert err <= 4 * dev + 1e-6 * float(np.abs(o64).max()), line
    return ratio


# ------------------------------------------------------------------------------------------------------------------------
# 1. forward and backward against the oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_and_backward_against_the_oracle(name, alpha):
    X, Y, G = inputs(name)
    err, d_img = gpu(name, alpha)
    for s, (e64, d64, e32, d32) in enumerate(reference(name, alpha)):
        what = "%s alpha=%g scale %d (%dx%d)" % ((name, alpha, s) + X[s].shape[3:])
        assert err[s].shape == e64.shape and d_img[s].shape == d64.shape
        _within(err[s], e64, e32, what + " fwd")
        knife = _knife(X[s], Y[s], alpha)
        assert knife.mean() <= 0.01, "%s: %.3g of the entries are knife-edge: the comparison would mean nothing" % (what, knife.mean())
        _within(d_img[s], d64, d32, what + " bwd", ~knife)


# ------------------------------------------------------------------------------------------------------------------------
# 2. known answers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
def test_identical_images_have_no_error_and_the_range_is_bounded(alpha):
    """X == Y gives no error at any alpha (the oracle: exactly 0).  For inputs in [-1,1] each SSIM term lies in [0,1] and each
    absolute difference in [0,2], so err lies in [0, 2 - alpha]: in [0,1] at alpha = 1, and the SSIM share of it -- err minus the L1
    share -- in [0, alpha] at every alpha.  (No smaller bound holds below alpha = 1: on these inputs, whose roll carries a seam, the
    fp64 oracle itself reaches 1.59 at alpha = 0.)"""
    X, Y, _ = inputs("nondyadic")
    n = X[0].shape[1]
    same = [_t(np.repeat(y[:, None], n, axis=1)) for y in Y]
    for e in ops.photo_error_fwd(same, [_t(y) for y in Y], alpha):
        assert float(e.abs().max()) <= 1e-6
    for name in ("nondyadic", "40x130"):
        X, Y, _ = inputs(name)
        X = [np.clip(x, -1, 1) for x in X]
        for e, x, y in zip(ops.photo_error_fwd([_t(x) for x in X], [_t(y) for y in Y], alpha), X, Y):
            e = e.cpu().numpy().astype(F64)
            assert e.min() >= 0 and e.max() <= 2 - alpha
            share = e - (1 - alpha) * np.abs(x.astype(F64) - y.astype(F64)[:, None]).mean(2)
            assert share.min() >= -1e-6 and share.max() <= alpha + 1e-6


def test_without_ssim_it_is_the_mean_absolute_difference_to_two_ulp():
    for name in ("nondyadic", "40x130", "3x3"):
        X, Y, G = inputs(name)
        err, d_img = gpu(name, 0.0)
        for x, y, g, e, d in zip(X, Y, G, err, d_img):
            diff = x - y[:, None]
            want = (np.abs(diff).astype(F64).sum(2) / 3).astype(np.float32)
            assert (np.abs(e - want) <= 2 * np.spacing(want)).all()
            want = (g[:, :, None].astype(F64) * np.sign(diff) / 3).astype(np.float32)
            assert (np.abs(d - want) <= 2 * np.spacing(np.abs(want))).all()


ADJ_DRAWS, ADJ_EPS = 4, 1e-2


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", ["nondyadic", "40x130"])
def test_adjoint_identity(name, alpha):
    X, Y, _ = inputs(name)
    rng = np.random.RandomState(3)
    res = {"gpu": [], "o64": [], "o32": []}      # per route: [draw][scale] -> residual (B, n)
    fd64 = []
    for _ in range(ADJ_DRAWS):
        V = [rng.standard_normal(x.shape).astype(np.float32) for x in X]
        G = [rng.standard_normal(x.shape[:2] + x.shape[3:]).astype(np.float32) for x in X]
        Xp = [(x + np.float32(ADJ_EPS) * v).astype(np.float32) for x, v in zip(X, V)]
        Xm = [(x - np.float32(ADJ_EPS) * v).astype(np.float32) for x, v in zip(X, V)]
        step = [(xp.astype(F64) - xm.astype(F64)) for xp, xm in zip(Xp, Xm)]      # 2 eps V as the float32 inputs carry it
        Yt, Gt = [_t(y) for y in Y], [_t(g) for g in G]
        routes = {"gpu": (_np(ops.photo_error_fwd([_t(a) for a in Xp], Yt, alpha)), _np(ops.photo_error_fwd([_t(a) for a in Xm], Yt, alpha)),
                          _np(ops.photo_error_bwd([_t(x) for x in X], Yt, alpha, Gt)))}
        for key, dt in (("o64", np.float64), ("o32", np.float32)):
            routes[key] = ([oracle(a, y, alpha, None, dt) for a, y in zip(Xp, Y)], [oracle(a, y, alpha, None, dt) for a, y in zip(Xm, Y)],
                           [oracle(x, y, alpha, g, dt)[1] for x, y, g in zip(X, Y, G)])
        for key, (ep, em, d) in routes.items():
            fd = [((a.astype(F64) - b.astype(F64)) * g).sum(axis=(2, 3)) for a, b, g in zip(ep, em, G)]
            res[key].append([f - (dd.astype(F64) * st).sum(axis=(2, 3, 4)) for f, dd, st in zip(fd, d, step)])
            if key == "o64":
                fd64.append(fd)
    for s in range(len(X)):
        got, o64, o32 = (np.stack([r[s] for r in res[key]]) for key in ("gpu", "o64", "o32"))
        scale = np.stack([f[s] for f in fd64])
        err, dev = np.abs(got - o64).max(), np.abs(o32 - o64).max()
        line = "photo_error adjoint %s alpha=%g scale %d: max|gpu-o64| %.3g, max|o32-o64| %.3g, ratio %.3g, max|fd64| %.3g, max|residual64| %.3g" \
            % (name, alpha, s, err, dev, err / dev if dev else 0.0, np.abs(scale).max(), np.abs(o64).max())
        print(line)
        parity_note(line)
        assert err <= 4 * dev + 1e-6 * np.abs(scale).max(), line


# ------------------------------------------------------------------------------------------------------------------------
# 3. contract
# ------------------------------------------------------------------------------------------------------------------------
def _arena_run(name, alpha, order=None, images=None):
    """Both calls on guarded buffers through the C ABI; scales in `order`, the first `images` images of every sample.
    -> ([err bits per scale], [d_img bits per scale]) in the case's own scale order"""
    X, Y, G = inputs(name)
    B, n, hw = CASES[name]
    order = list(range(len(hw))) if order is None else order
    if images is not None:
        X, G, n = [np.ascontiguousarray(x[:, :images]) for x in X], [np.ascontiguousarray(g[:, :images]) for g in G], images
    specs = []
    for s, (h, w) in enumerate(hw):
        specs += [("img%d" % s, (B, n, 3, h, w), 4 * (s % 4)), ("tgt%d" % s, (B, 3, h, w), 8), ("g%d" % s, (B, n, h, w), 12),
                  ("err%d" % s, (B, n, h, w), 4), ("d%d" % s, (B, n, 3, h, w), 4 * ((s + 1) % 4))]
    ar = Arena(DEV, specs, row_floats=max(w for _, w in hw))
    for s in range(len(hw)):
        ar.set("img%d" % s, X[s]), ar.set("tgt%d" % s, Y[s]), ar.set("g%d" % s, G[s])
        for key in ("img%d", "tgt%d", "g%d"):
            ar.snapshot(key % s)
    d = _lib.SfmPhotoErrorDesc()
    d.B, d.n_img, d.n_scales, d.ssim_rate = B, n, len(hw), alpha
    for k, s in enumerate(order):
        d.H[k], d.W[k] = hw[s]
        d.img[k], d.tgt[k], d.g_err[k], d.err[k], d.d_img[k] = (ar.ptr(key % s) for key in ("img%d", "tgt%d", "g%d", "err%d", "d%d"))
    for fn in (_lib.lib.sfm_photo_error_fwd, _lib.lib.sfm_photo_error_bwd):
        _lib.check(fn(C.byref(d), ops._stream()))
    torch.cuda.synchronize()
    ar.check("%s alpha=%g" % (name, alpha))
    for s in range(len(hw)):
        assert ar.sentinels_left("err%d" % s) == 0 and ar.sentinels_left("d%d" % s) == 0, "scale %d: an output element was not written" % s
        assert not np.isnan(ar.view("err%d" % s).cpu().numpy()).any() and not np.isnan(ar.view("d%d" % s).cpu().numpy()).any()
        for key in ("img%d", "tgt%d", "g%d"):
            ar.unchanged(key % s)
    return [ar.bits("err%d" % s) for s in range(len(hw))], [ar.bits("d%d" % s) for s in range(len(hw))]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", ["nondyadic", "fwd_strips", "bwd_strips", "two_chunks", "max_img", "3x3"])
def test_buffer_contract(name, alpha):
    """NaN-filled outputs are overwritten completely, the 4 KiB guard bands around every array stay untouched, the inputs keep
    their bits, a second run and a run with the scales in reverse order give the same bits, which are those ops returns"""
    first = _arena_run(name, alpha)
    again = _arena_run(name, alpha)
    swapped = _arena_run(name, alpha, order=list(range(len(CASES[name][2])))[::-1])
    err, d_img = gpu(name, alpha)
    for s in range(len(first[0])):
        for k in (0, 1):
            assert np.array_equal(first[k][s], again[k][s]), "scale %d: two runs differ" % s
            assert np.array_equal(first[k][s], swapped[k][s]), "scale %d: the order of the scales shows" % s
        assert np.array_equal(first[0][s], err[s].view(np.int32)) and np.array_equal(first[1][s], d_img[s].view(np.int32))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_an_image_does_not_depend_on_its_neighbours(alpha):
    three = _arena_run("nondyadic", alpha)
    one = _arena_run("nondyadic", alpha, images=1)
    for s in range(len(three[0])):
        assert np.array_equal(three[0][s][:, :1], one[0][s]) and np.array_equal(three[1][s][:, :1], one[1][s])


# ------------------------------------------------------------------------------------------------------------------------
# 4. composition through torch
# ------------------------------------------------------------------------------------------------------------------------
def aten_photo_error(x, y, alpha):
    """the same formula in aten: x (B,n,3,h,w), y (B,3,h,w) -> (B,n,h,w)"""
    F = torch.nn.functional
    B, n, c, h, w = x.shape
    X, Y = x.reshape(B * n, 3, h, w), y[:, None].expand(B, n, 3, h, w).reshape(B * n, 3, h, w)
    pool = lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=True)
    l1 = (X - Y).abs().mean(1)
    if alpha == 0:
        return l1.view(B, n, h, w)
    mx, my = pool(X), pool(Y)
    sx, sy, sxy = pool(X * X) - mx * mx, pool(Y * Y) - my * my, pool(X * Y) - mx * my
    S = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
    e = ((1 - S) / 2).clamp(0, 1).mean(1)
    return ((1 - alpha) * l1 + alpha * e).view(B, n, h, w)


def _step_inputs():
    d = synth.make_inputs(B=2, H=16, W=24, n_src=2, n_scales=2, seed=21)
    return dict(src=_t(d["src"]), tgt=_t(d["tgt"]), K=_t(d["intrinsics"]), disps=[_t(a) for a in d["disps"]], poses=[_t(a) for a in d["poses"]])


def _loss(errs):
    return sum(e.min(dim=1).values.mean() for e in errs)


@pytest.mark.parametrize("alpha", [0.85])
def test_composition_with_warp_pyramid(alpha):
    x = _step_inputs()
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    warped = ta.warp_pyramid(x["src"], x["K"], x["disps"], x["poses"])
    tgts = ops.pyramid(x["tgt"], 2)
    errs = ta.photometric_error(warped, x["tgt"], ssim_rate=alpha)
    assert all(e.requires_grad and e.shape == w.shape[:2] + w.shape[3:] for e, w in zip(errs, warped))
    got = torch.autograd.grad(_loss(errs), leaves, retain_graph=True)

    def through_the_warp(dtype, where):
        w = [t.detach().to(where, dtype).requires_grad_() for t in warped]
        loss = _loss([aten_photo_error(a, y.to(where, dtype), alpha) for a, y in zip(w, tgts)])
        g = torch.autograd.grad(loss, w)
        return torch.autograd.grad(warped, leaves, [t.to(DEV, torch.float32) for t in g], retain_graph=True)

    a32, a64 = through_the_warp(torch.float32, DEV), through_the_warp(torch.float64, "cpu")
    for k, (g, b, r) in enumerate(zip(got, a32, a64)):
        _within(g.cpu().numpy(), r.cpu().numpy().astype(F64), b.cpu().numpy(), "composition alpha=%g %s" % (alpha, "d_disp d_disp d_pose d_pose".split()[k]))


def test_the_example_of_integration_md_trains():
    """INTEGRATION.md, 'The photometric error of that loss', as written: finite loss, finite non-zero gradients, no host sync"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = [b for b in re.findall(r"```python3\n(.*?)```", text, flags=re.S) if "min_reprojection_loss_ssim" in b]
    assert len(block) == 1
    x = _step_inputs()
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    importlib.import_module("sfmwarp")
    env = dict(torch=torch, ta=ta, tgt_img=x["tgt"], src_imgs=x["src"], intrinsics=x["K"], pred_disps=x["disps"], pred_poses=x["poses"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        exec(compile(block[0], "INTEGRATION.md#photometric-error", "exec"), env)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    total = env["min_reprojection_loss_ssim"](x["tgt"], x["src"], x["K"], x["disps"], x["poses"])
    assert bool(torch.isfinite(total)) and float(total) > 0
    for t in leaves:
        assert bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any())


def test_dtype_no_grad_sync_and_graph_capture():
    x = _step_inputs()
    warped = [w.detach() for w in ta.warp_pyramid(x["src"], x["K"], x["disps"], x["poses"])]
    # the gradient dtype follows a bfloat16 input; the target gets none
    wb = [w.to(torch.bfloat16).requires_grad_() for w in warped]
    tgt = x["tgt"].clone().requires_grad_()
    errs = ta.photometric_error(wb, tgt, ssim_rate=0.85)
    assert all(e.dtype == torch.float32 for e in errs)
    _loss(errs).backward()
    assert all(w.grad is not None and w.grad.dtype == torch.bfloat16 and w.grad.shape == w.shape for w in wb) and tgt.grad is None
    # nothing is recorded when no image requires a gradient
    assert all(not e.requires_grad and e.grad_fn is None for e in ta.photometric_error(warped, tgt, ssim_rate=0.85))
    # a list of targets is the single target's pyramid
    for a, b in zip(ta.photometric_error(warped, ops.pyramid(x["tgt"], 2), ssim_rate=0.85), ta.photometric_error(warped, x["tgt"], ssim_rate=0.85)):
        assert _bits(a, b)
    # a library rejection is a ValueError with the library's message
    with pytest.raises(ValueError, match="ssim_rate"):
        ta.photometric_error(warped, x["tgt"], ssim_rate=1.5)

    def step():
        for t in x["disps"] + x["poses"]:
            t.grad = None
        w = ta.warp_pyramid(x["src"], x["K"], x["disps"], x["poses"])
        ident = [p.view(p.shape[0], 2, 3, p.shape[2], p.shape[3]) for p in ops.pyramid(x["src"].view(2, 6, 16, 24), 2)]
        errs = ta.photometric_error(w, x["tgt"], ssim_rate=0.85)
        base = ta.photometric_error(ident, x["tgt"], ssim_rate=0.85)
        loss = sum(torch.minimum(e.min(dim=1).values, b.min(dim=1).values).mean() for e, b in zip(errs, base))
        loss.backward()
        return [loss.detach()] + [t.grad for t in x["disps"] + x["poses"]]

    for t in x["disps"] + x["poses"]:
        t.requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = [t.clone() for t in step()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bits(a, b) for a, b in zip(eager, captured))
    assert float(eager[0]) > 0 and all(float(t.abs().max()) > 0 for t in eager[1:])
