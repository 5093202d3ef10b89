"""References for the two conventions of include/sfmwarp_conventions.h (tests/test_conventions_cpu.py, tests/test_conventions_gpu.py):

  half-pixel upsampling   `axis_taps_hp`, `upsample_hp`, `adjoint_hp`: the NumPy restatement, in the style of tests/warp_full_res_ref.py
                          -- float32 is the statement of the kernels, float64 the same map with exact-enough weights;
  reflection-padded SSIM  `photo_error`: a torch-CPU statement of the definition -- F.pad(mode="reflect") + avg_pool2d -- with autograd,
                          in float64 and float32, written term by term as oracle.compute_ssim is; `fold` and `emulate_reflect`: the
                          ring fold of the backward as the kernel performs it, in NumPy float64.
"""
import functools
import importlib
import os
import re

import numpy as np
import torch

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------------------
# half-pixel upsampling
# ------------------------------------------------------------------------------------------------------------------------
# (H, W) of the full resolution and the (h, w) of each disparity
HP_SHAPES = {
    "24x40": ((24, 40), [(24, 40), (12, 20), (6, 10), (3, 5)]),                  # halvings
    "13x21": ((13, 21), [(13, 21), (7, 10), (1, 1), (1, 4), (20, 30)]),          # non-integer ratios, one row, one element, DOWNsampled
    "130x127": ((130, 127), [(130, 127), (65, 63), (17, 9)]),                    # 65 blocks of 256 pixels per image
}
# one more, not among the nine pairs: ratios above 2, where some elements of the disparity are reached by no output at all
HP_EXTRA = {"9x7": ((9, 7), [(9, 7), (20, 30)])}
HP_PAIRS = [(HW, hw) for HW, sizes in HP_SHAPES.values() for hw in sizes[1:]]      # the nine resampled (full size, disparity size) pairs


def coords_hp(n, on, dtype=F32):
    """max(scale * (o + 0.5) - 0.5, 0) for the `on` outputs along an axis of n inputs, scale = n / on: every operation in `dtype`"""
    scale = dtype(n) / dtype(on)
    u = np.maximum(scale * (np.arange(on).astype(dtype) + dtype(0.5)) - dtype(0.5), dtype(0))
    assert u.dtype == dtype
    return u


def axis_taps_hp(n, on, dtype=F32):
    """(tap0, tap1, w0, w1) of the `on` outputs along an axis of n inputs as resize_hp_coord / resize_hp_taps form them"""
    u = coords_hp(n, on, dtype)
    t0 = np.minimum(np.floor(u).astype(np.int64), n - 1)
    t1 = np.minimum(t0 + 1, n - 1)
    w1 = u - t0.astype(dtype)
    w0 = dtype(1) - w1
    assert w0.dtype == dtype and w1.dtype == dtype
    return t0, t1, w0, w1


def upsample_hp(x, out_hw, dtype=F32):
    """x (N,C,h,w) -> (N,C,H,W): resize_blend's three statements on the half-pixel taps; a map of equal sizes is used as it is"""
    x = np.asarray(x, dtype=dtype)
    H, W = out_hw
    if tuple(x.shape[2:]) == (H, W):
        return x
    v0, v1, wv0, wv1 = axis_taps_hp(x.shape[2], H, dtype)
    u0, u1, wu0, wu1 = axis_taps_hp(x.shape[3], W, dtype)
    top = x[:, :, v0][:, :, :, u0] * wu0 + x[:, :, v0][:, :, :, u1] * wu1
    bot = x[:, :, v1][:, :, :, u0] * wu0 + x[:, :, v1][:, :, :, u1] * wu1
    y = top * wv0[:, None] + bot * wv1[:, None]
    assert y.dtype == dtype
    return y


def adjoint_hp(gy, in_hw, dtype=F32):
    """gy (N,C,H,W) -> (N,C,h,w), the adjoint of `upsample_hp` as warp_full_gather_kernel<HP> adds it up: per low-resolution element
    the contributions gy * (wv * wu) in ascending (oy, ox); of an axis' two taps the one that lands on the element, their sum
    where both do (the far edge, one input row or column); an element no output touches stays exactly 0"""
    gy = np.asarray(gy, dtype=dtype)
    h, w = in_hw
    if tuple(gy.shape[2:]) == (h, w):
        return gy
    v0, v1, wv0, wv1 = axis_taps_hp(h, gy.shape[2], dtype)
    u0, u1, wu0, wu1 = axis_taps_hp(w, gy.shape[3], dtype)
    gx = np.zeros(gy.shape[:2] + (h, w), dtype=dtype)
    for oy in range(gy.shape[2]):
        rows = [(v0[oy], wv0[oy] + wv1[oy])] if v0[oy] == v1[oy] else [(v0[oy], wv0[oy]), (v1[oy], wv1[oy])]
        for ox in range(gy.shape[3]):
            cols = [(u0[ox], wu0[ox] + wu1[ox])] if u0[ox] == u1[ox] else [(u0[ox], wu0[ox]), (u1[ox], wu1[ox])]
            g = gy[:, :, oy, ox]
            for r, wv in rows:
                for c, wu in cols:
                    gx[:, :, r, c] += g * dtype(wv * wu)
    assert gx.dtype == dtype
    return gx


def interpolate_aten(x, out_hw, dtype=torch.float64):
    """the independent opinion: torch.nn.functional.interpolate(mode="bilinear", align_corners=False) on the CPU"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return torch.nn.functional.interpolate(t, size=tuple(out_hw), mode="bilinear", align_corners=False).numpy()


def adjoint64_aten_hp(gy, in_hw):
    """... and its float64 autograd"""
    g = torch.from_numpy(np.asarray(gy, dtype=F64))
    x = torch.zeros(tuple(g.shape[:2]) + tuple(int(v) for v in in_hw), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.interpolate(x, size=tuple(g.shape[2:]), mode="bilinear", align_corners=False).backward(g)
    return x.grad.numpy()


# ------------------------------------------------------------------------------------------------------------------------
# reflection-padded SSIM
# ------------------------------------------------------------------------------------------------------------------------
def geometry():
    """PE_ROWS, PE_FWD_STRIP, PE_BWD_STRIP of csrc/sfm_photo_error.hip"""
    text = open(os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", "sfm_photo_error.hip")).read()
    return [int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("PE_ROWS", "PE_FWD_STRIP", "PE_BWD_STRIP")]


ROWS, FWD_STRIP, BWD_STRIP = geometry()
MAX_SRC = 8      # SFM_MAX_SRC


def _around(strip):
    """eight scales: widths one below, at, one and two above the first two multiples of `strip`, heights likewise around the chunk
    length.  The +2 puts column W-2 on the first useful lane of a strip and row H-2 on the last row of a chunk."""
    return [(ROWS + d, k * strip + d) for k in (1, 2) for d in (-1, 0, 1, 2)]


# (B, n_img, [(h, w)], seed)
REFLECT_CASES = {
    "tiny": (1, 1, [(2, 2), (2, 3), (3, 2), (3, 3)], 11),
    "nondyadic": (2, 3, [(17, 61), (9, 31), (5, 16), (3, 8)], 12),
    "fwd_strips": (1, 1, _around(FWD_STRIP), 13),
    "bwd_strips": (1, 1, _around(BWD_STRIP), 14),
    "two_chunks": (1, 2, [(2 * ROWS - 1, 5), (2 * ROWS, 4), (2 * ROWS + 1, 3), (2 * ROWS + 2, 2)], 15),
    "max_img": (1, MAX_SRC, [(7, 9), (2, 5)], 16),
}
ALPHAS = [0.0, 0.85, 1.0]


@functools.lru_cache(maxsize=None)
def reflect_inputs(name):
    """float32 host arrays of one case (never modify them), as tests/test_photo_error_gpu.py makes them: Y a texture -- low-resolution
    noise upsampled, clipped to [-1,1] --, X = Y rolled by two columns plus 0.05 noise, g standard normal"""
    synth = importlib.import_module("sfm-learner-chainer_amd.synth")
    B, n, hw, seed = REFLECT_CASES[name]
    rng = np.random.RandomState(seed)
    X, Y, G = [], [], []
    for h, w in hw:
        tex = 1.4 * synth._smooth_field(rng, B, 3, h, w, 8) + 0.2 * synth._smooth_field(rng, B, 3, h, w, 2)
        y = np.clip(tex, -1, 1).astype(F32)
        x = np.stack([np.roll(y, 2, axis=3) + 0.05 * rng.standard_normal(y.shape) for _ in range(n)], axis=1).astype(F32)
        X.append(x), Y.append(y), G.append(rng.standard_normal((B, n, h, w)).astype(F32))
    return X, Y, G


def _pool_t(t, padding):
    """the 3x3 average of the last two axes of a (N,C,h,w) tensor: over the reflection-padded image, or zero-padded and divided by 9"""
    Fn = torch.nn.functional
    if padding == "reflect":
        return Fn.avg_pool2d(Fn.pad(t, (1, 1, 1, 1), mode="reflect"), 3, 1)
    assert padding == "zero"
    return Fn.avg_pool2d(t, 3, 1, 1, count_include_pad=True)


def ssim_terms(x, y, padding):
    """(1 - SSIM) / 2 before the clip, term by term as oracle.compute_ssim writes models/base_model.py:126-142; x, y (N,3,h,w) tensors"""
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mu_x, mu_y = _pool_t(x, padding), _pool_t(y, padding)
    sigma_x = _pool_t(x ** 2, padding) - mu_x ** 2
    sigma_y = _pool_t(y ** 2, padding) - mu_y ** 2
    sigma_xy = _pool_t(x * y, padding) - mu_x * mu_y
    n1, n2 = 2 * mu_x * mu_y + c1, 2 * sigma_xy + c2
    d1, d2 = mu_x ** 2 + mu_y ** 2 + c1, sigma_x + sigma_y + c2
    return (1 - (n1 * n2) / (d1 * d2)) / 2


def photo_error(X, Y, alpha, g=None, dtype=np.float64, padding="reflect"):
    """err (B,n,h,w) and, with g, d_img (B,n,3,h,w) by autograd, as host arrays of `dtype`: X (B,n,3,h,w), Y (B,3,h,w).  The
    definition of include/sfmwarp_conventions.h: (1 - alpha) mean_c |X - Y| + alpha mean_c clip((1 - SSIM) / 2, 0, 1), the 3x3 averages
    of SSIM over ReflectionPad2d(1) of the images; Y is a constant"""
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    x = torch.from_numpy(np.ascontiguousarray(X)).to(td).requires_grad_(g is not None)
    y = torch.from_numpy(np.ascontiguousarray(Y)).to(td)
    B, n, _, h, w = x.shape
    xf, yf = x.reshape(B * n, 3, h, w), y[:, None].expand(B, n, 3, h, w).reshape(B * n, 3, h, w)
    third = torch.tensor(1.0, dtype=td) / 3
    err = (1 - alpha) * ((xf - yf).abs().sum(1) * third)
    if alpha > 0:
        err = err + alpha * (ssim_terms(xf, yf, padding).clamp(0, 1).sum(1) * third)
    err = err.view(B, n, h, w)
    if g is None:
        return err.detach().numpy()
    err.backward(torch.from_numpy(np.ascontiguousarray(g)).to(td))
    return err.detach().numpy(), x.grad.numpy()


@functools.lru_cache(maxsize=None)
def reflect_reference(name, alpha, padding="reflect"):
    """per scale: (err64, d64, err32, d32) of `photo_error` on the float32 inputs (never modify them)"""
    X, Y, G = reflect_inputs(name)
    return [photo_error(x, y, alpha, g, np.float64, padding) + photo_error(x, y, alpha, g, np.float32, padding) for x, y, g in zip(X, Y, G)]


def _pool_np(a, padding):
    """3x3 sum / 9 of the last two axes of a NumPy array, padded as named"""
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)], mode="reflect" if padding == "reflect" else "constant")
    h, w = a.shape[-2:]
    return sum(p[..., i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0


def knife(x, y, alpha, padding="reflect"):
    """the entries (B,n,3,h,w) that leave the backward comparison: the rule of tests/test_photo_error_gpu.py with the windows of
    `padding` -- |e_c| or |e_c - 1| below 1e-5 (fp64) anywhere in the 3x3 window an entry takes part in, |X_c - Y_c| below 1e-6 itself"""
    x, y = x.astype(F64), y.astype(F64)[:, None]
    out = np.abs(x - y) < 1e-6
    if alpha > 0:
        P = lambda a: _pool_np(a, padding)
        mx, my = P(x), P(y)
        n1, n2 = 2 * mx * my + 1e-4, 2 * (P(x * y) - mx * my) + 9e-4
        d1, d2 = mx * mx + my * my + 1e-4, (P(x * x) - mx * mx) + (P(y * y) - my * my) + 9e-4
        e = (1 - n1 * n2 / (d1 * d2)) / 2
        near = ((np.abs(e) < 1e-5) | (np.abs(e - 1) < 1e-5)).astype(F64)
        # (the reflected window of an entry holds exactly the pixels whose windows read the entry: `fold(near) > 0` is the same set)
        out = out | (P(near) > 0)
    return out


def fold(m):
    """The adjoint of "ReflectionPad2d(1), then the 3x3 SUM" applied to a map m (..., h, w) that exists at image pixels only, as
    photo_err_bwd_kernel<true, true> forms it: along the row the 3-sum plus, at columns 1 and W-2, the neighbour at column 0 and W-1
    once more; then the same down the columns with the rows' sums"""
    def along(a, axis):
        a = np.moveaxis(a, axis, -1)
        n = a.shape[-1]
        z = np.zeros(a.shape[:-1] + (1,), a.dtype)
        left, right = np.concatenate([z, a[..., :-1]], -1), np.concatenate([a[..., 1:], z], -1)
        s = (a + left) + right
        s[..., 1] += left[..., 1]
        s[..., n - 2] += right[..., n - 2]
        return np.moveaxis(s, -1, axis)
    return along(along(np.asarray(m), -1), -2)


def emulate_reflect(X, Y, alpha, g):
    """d_img (B,n,3,h,w) in NumPy float64: tests/test_photo_error_cpu.py's `emulate` with the reflected statistics and `fold` / 9 in
    place of the second pooling, 2 x fold(..) and y fold(..) formed once per output"""
    X, Y = np.asarray(X, F64), np.asarray(Y, F64)[:, None]
    c1, c2 = 1e-4, 9e-4
    P = lambda a: _pool_np(a, "reflect")
    mx, my = P(X), P(Y)
    exx, eyy, exy = P(X * X), P(Y * Y), P(X * Y)
    n1, n2 = 2 * mx * my + c1, 2 * (exy - mx * my) + c2
    d1, d2 = mx * mx + my * my + c1, (exx - mx * mx) + (eyy - my * my) + c2
    S = n1 * n2 / (d1 * d2)
    e = (1 - S) / 2
    g = np.asarray(g, F64)[:, :, None]
    kappa = alpha / 3 * g * -0.5 * ((e > 0) & (e < 1))
    dS_dmx = (2 * my * (n2 - n1) - S * 2 * mx * (d2 - d1)) / (d1 * d2)
    dS_dexx, dS_dexy = -S / d2, 2 * n1 / (d1 * d2)
    return (1 - alpha) / 3 * g * np.sign(X - Y) + fold(kappa * dS_dmx) / 9 + 2 * X * (fold(kappa * dS_dexx) / 9) + Y * (fold(kappa * dS_dexy) / 9)
