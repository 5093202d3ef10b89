"""The operator kernels of csrc/sfm_ops.hip at the shapes, grids and values where kernels go wrong, against a plain
high-precision reference of the same operation (the NumPy oracle evaluated in float64, and torch float64 autograd as a
second opinion), and the accumulate / NULL-output contracts of include/sfmwarp.h called through the C ABI directly.

tests/test_ops_gpu.py holds the operators at friendly shapes; this module is the edges: widths and heights at the
64-lane, 8-row and 32-row boundaries of the sampler's backward, fields whose neighbouring output pixels share a source
cell (zoom-in) or sit exactly on the lattice, one-pixel images and scales, ragged and empty activation scales,
saturated logits and clipped angles.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import sfm_oracle as O
from util import parity_note, to_dev, to_np

pytestmark = pytest.mark.gpu

F64 = np.float64
KNIFE_PX = 1e-5      # padded positions this close to a lattice line may take either cell in fp32 versus fp64
KNIFE_CAP = 0.01     # ... and may exclude at most this share of a field's ggrid components from the fp64 comparison


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(ops):
    return ops._stream()


# ------------------------------------------------------------------------------------------------------------------------
# F.spatial_transformer_sampler (models/transform.py:189): sfm_sampler_fwd / sfm_sampler_bwd
# ------------------------------------------------------------------------------------------------------------------------
def _to_grid(u, v, H, W):
    """unpadded pixel positions (fp64) -> the normalised float32 grid (N,2,oH,oW) the sampler takes"""
    return np.stack([u / ((W - 1) / 2.0) - 1.0, v / ((H - 1) / 2.0) - 1.0], axis=1).astype(np.float32)


def make_field(family, N, H, W, oH, oW, rng):
    """Grids of one family (see test_sampler_edges).  Positions are generated in fp64 pixel units, then normalised."""
    oy, ox = np.meshgrid(np.arange(oH, dtype=F64), np.arange(oW, dtype=F64), indexing="ij")
    oy, ox = np.broadcast_to(oy, (N, oH, oW)), np.broadcast_to(ox, (N, oH, oW))
    n = np.arange(N, dtype=F64)[:, None, None]
    if family == "identity":        # exact integers on the padded lattice, the zero ring included: wx1 == wy1 == 0
        assert ((W - 1) & (W - 2)) == 0 and ((H - 1) & (H - 2)) == 0, "the identity lattice needs W-1, H-1 powers of two"
        u = np.mod(ox + 3 * n, W + 2) - 1
        v = np.mod(oy + n, H + 2) - 1
    elif family == "shift":         # a constant sub-pixel shift: every lane's right-hand taps are its neighbour's left-hand taps
        u = ox + 0.37 + 0.11 * n
        v = oy + 0.61 - 0.2 * n
    elif family in ("zoom2", "zoom3.5", "zoomout"):   # about an off-centre point: neighbours share a cell (zoom-in) or skip one
        z = {"zoom2": 2.0, "zoom3.5": 3.5, "zoomout": 0.5}[family]
        cu, cv = 0.31 * W + 0.17 + n, 0.43 * H + 0.29
        u = cu + (ox - 0.31 * oW) / z
        v = cv + (oy - 0.43 * oH) / z
    elif family == "smooth":        # a smooth field that crosses the zero-pad ring and leaves the padded image on both sides
        u = ox * ((W + 5.0) / max(oW - 1, 1)) - 2.5 + 1.5 * np.sin(oy / 5.0 + n)
        v = oy * ((H + 5.0) / max(oH - 1, 1)) - 2.5 + 1.5 * np.cos(ox / 7.0 - n + 0.3)
    elif family == "edges":         # grid values exactly at +-1 and at the padded edges +-(1 + 2/(W-1)), mixed with random ones
        assert ((W - 1) & (W - 2)) == 0 and ((H - 1) & (H - 2)) == 0, "the padded edges are exact only for W-1, H-1 powers of two"
        g = rng.uniform(-1.3, 1.3, size=(N, 2, oH, oW))
        for k, L in ((0, W), (1, H)):
            choice = np.array([-1.0, 1.0, -(1 + 2.0 / (L - 1)), 1 + 2.0 / (L - 1)])
            pick = rng.uniform(size=(N, oH, oW)) < 0.5
            g[:, k][pick] = choice[rng.randint(0, 4, size=int(pick.sum()))]
        return g.astype(np.float32)
    else:
        raise ValueError(family)
    return _to_grid(u, v, H, W)


def _padded_pos(grid, H, W, dtype):
    """the sampler's padded positions (u, v) as the fp32 kernel / the fp64 oracle form them, and whether they are inside"""
    g = grid.astype(dtype)
    u = (g[:, 0] + dtype(1)) * dtype(W - 1) / dtype(2) + dtype(1)
    v = (g[:, 1] + dtype(1)) * dtype(H - 1) / dtype(2) + dtype(1)
    return u, v


def sampler_knife(grid, H, W):
    """(N,2,oH,oW) bool: ggrid components whose cell may legitimately differ between fp32 and fp64 -- the fp64 position within
    KNIFE_PX of a lattice line (padded edges included) unless fp32 forms the very same position, or the two clipped cells or
    inside-tests differing outright; never where both lie outside the padded image (the component is 0).  Only du/dv of the sample jumps there (gu at a column line, gv at a row line); the value,
    gx and the other component are continuous."""
    u32, v32 = _padded_pos(grid, H, W, np.float32)
    u64, v64 = _padded_pos(grid, H, W, F64)
    out = []
    for p32, p64, L in ((u32, u64, W), (v32, v64, H)):
        near = np.abs(p64 - np.rint(p64)) < KNIFE_PX
        c32 = np.floor(np.clip(p32, 0, L + 1)).clip(0, L)
        c64 = np.floor(np.clip(p64, 0, L + 1)).clip(0, L)
        ok32, ok64 = (p32 >= 0) & (p32 <= L + 1), (p64 >= 0) & (p64 <= L + 1)
        out.append(((near & (p32.astype(F64) != p64)) | (c32 != c64) | (ok32 != ok64)) & (ok32 | ok64))
    return np.stack(out, axis=1)


def _grid_sample_torch(x, grid, gy):
    """torch float64 autograd of grid_sample(align_corners=True, padding_mode="zeros"): (y, gx, ggrid)"""
    import torch.nn.functional as TF
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(grid, dtype=torch.float64, requires_grad=True)
    y = TF.grid_sample(xt, gt.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=True)
    (y * torch.tensor(gy, dtype=torch.float64)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), gt.grad.numpy()


# (family, C, H, W, oH, oW, torch second opinion): oW in {1, 63, 64, 65, 130}, oH in {1, 7, 8, 9, 31, 32, 33}, C on both sides of
# SAMPLER_BWD_MAXC = 4 (the carrying and the non-carrying instantiation of sampler_bwd_kernel)
SAMPLER_CASES = [
    ("identity", 1, 33, 65, 33, 130, True), ("identity", 4, 9, 65, 8, 64, False), ("identity", 8, 17, 33, 9, 65, False),
    ("identity", 2, 5, 9, 1, 63, False),
    ("shift", 2, 40, 70, 32, 64, True), ("shift", 5, 9, 70, 7, 63, False), ("shift", 3, 4, 66, 1, 65, False),
    ("shift", 1, 34, 140, 33, 130, False),
    ("zoom2", 1, 20, 80, 31, 130, True), ("zoom2", 4, 20, 40, 33, 65, False), ("zoom2", 8, 10, 40, 9, 64, False),
    ("zoom2", 3, 12, 30, 8, 1, False),
    ("zoom3.5", 2, 12, 30, 32, 63, True), ("zoom3.5", 3, 10, 50, 8, 130, False), ("zoom3.5", 5, 12, 12, 33, 1, False),
    ("zoom3.5", 4, 6, 40, 31, 64, False),
    ("zoomout", 3, 30, 140, 9, 64, True), ("zoomout", 1, 5, 270, 1, 130, False), ("zoomout", 2, 70, 70, 32, 33, False),
    ("smooth", 4, 31, 130, 31, 130, True), ("smooth", 2, 7, 65, 7, 65, False), ("smooth", 8, 33, 64, 33, 64, False),
    ("smooth", 1, 9, 63, 9, 63, False),
    ("edges", 3, 9, 65, 8, 64, True), ("edges", 4, 33, 17, 33, 65, False), ("edges", 5, 5, 9, 7, 63, False),
]


@pytest.mark.parametrize("case", SAMPLER_CASES, ids=lambda c: "%s-C%d-%dx%d-to-%dx%d" % c[:6])
def test_sampler_edges(ops, dev, case):
    """sfm_sampler_fwd / sfm_sampler_bwd on the fields where the backward's share passing goes wrong if it goes wrong anywhere:
    the identity lattice (exact integers, wx1 == 0), a constant sub-pixel shift (every lane merges with its neighbour), zoom-in
    x2 and x3.5 (several output pixels share one source cell: the pending shares must be flushed, not merged), zoom-out x0.5,
    a smooth field across the zero-pad ring and out of the padded image, and grid values exactly at +-1 and the padded edges.
    Tolerances:
      * against the fp32 oracle (same cell choice as the kernel): y at rtol 1e-5 / atol 1e-6, ggrid at rtol 1e-4 / atol 1e-5 of
        its maximum, gx at rtol 1e-4 / atol 2e-5 -- those of tests/test_ops_gpu.py;
      * against the fp64 oracle: y, gx and ggrid element-wise within 1e-4 of the array's maximum magnitude; ggrid components
        whose position may take the other cell in fp32 (sampler_knife) are excluded, their share printed and capped at 1 %;
      * torch float64 grid_sample + autograd for one shape per family, by the fp64 criteria; ggrid additionally excludes the
        far padded edge u == W+1 (v == H+1), where the reference's clip keeps the cell [W, W+1] and torch has no in-image tap."""
    family, Cc, H, W, oH, oW, with_torch = case
    N = 2
    rng = np.random.RandomState(zlib.crc32(repr(case[:6]).encode()))
    x = rng.uniform(-1, 1, size=(N, Cc, H, W)).astype(np.float32)
    grid = make_field(family, N, H, W, oH, oW, rng)
    gy = rng.normal(size=(N, Cc, oH, oW)).astype(np.float32)
    xd, gd, gyd = to_dev(x, dev), to_dev(grid, dev), to_dev(gy, dev)
    y = to_np(ops.sampler_fwd(xd, gd))
    gx, gg = (to_np(t) for t in ops.sampler_bwd(xd, gd, gyd))
    # fp32 oracle
    np.testing.assert_allclose(y, O.spatial_transformer_sampler(x, grid), rtol=1e-5, atol=1e-6)
    w_gx, w_gg = O.spatial_transformer_sampler_backward(x, grid, gy)
    np.testing.assert_allclose(gg, w_gg, rtol=1e-4, atol=1e-5 * max(np.abs(w_gg).max(), 1e-30))
    np.testing.assert_allclose(gx, w_gx, rtol=1e-4, atol=2e-5)
    # fp64 oracle
    knife = sampler_knife(grid, H, W)
    share = float(knife.mean())
    parity_note("sampler %s C=%d %dx%d -> %dx%d: fp64 comparison excludes %.3f%% of the ggrid components (cap %.0f%%)" % (
        family, Cc, H, W, oH, oW, 100 * share, 100 * KNIFE_CAP))
    assert share <= KNIFE_CAP, "too many knife-edge positions (%.3f%%): the exclusion would hide real errors" % (100 * share)
    y64 = O.spatial_transformer_sampler(x, grid, dtype=F64)
    gx64, gg64 = O.spatial_transformer_sampler_backward(x, grid, gy, dtype=F64)

    def judge(got, want, excl, what):
        scale = max(float(np.abs(want).max()), 1e-30)
        err = np.abs(got.astype(F64) - want)
        if excl is not None:
            err = np.where(excl, 0.0, err)
        assert err.max() <= 1e-4 * scale, "%s: max error %.3g of the maximum %.3g (tol 1e-4)" % (what, err.max() / scale, scale)
        return err.max() / scale

    e = [judge(y, y64, None, "y vs fp64"), judge(gx, gx64, None, "gx vs fp64"), judge(gg, gg64, knife, "ggrid vs fp64")]
    parity_note("sampler %s C=%d %dx%d -> %dx%d: vs fp64 y %.1e, gx %.1e, ggrid %.1e of the maximum" % (family, Cc, H, W, oH, oW, *e))
    if with_torch:
        ty, tgx, tgg = _grid_sample_torch(x, grid, gy)
        u64, v64 = _padded_pos(grid, H, W, F64)
        far = np.stack([np.abs(u64 - (W + 1)) < KNIFE_PX, np.abs(v64 - (H + 1)) < KNIFE_PX], axis=1)
        judge(y, ty, None, "y vs torch")
        judge(gx, tgx, None, "gx vs torch")
        judge(gg, tgg, knife | far, "ggrid vs torch")


def _sampler_bwd_raw(ops, x, grid, gy, ggrid, gx):
    N, Cc, H, W = x.shape
    oH, oW = grid.shape[2:]
    ops.check(ops.lib.sfm_sampler_bwd(_p(x), _p(grid), _p(gy), _p(ggrid), _p(gx), N, Cc, H, W, oH, oW, _stream(ops)))


@pytest.mark.parametrize("family,Cc", [("zoom2", 3), ("zoom3.5", 5), ("smooth", 2)])
def test_sampler_bwd_accumulates_into_gx_and_takes_a_null_gx(ops, dev, family, Cc):
    """include/sfmwarp.h: gx of sfm_sampler_bwd is ACCUMULATED.  Called through the C ABI (ops.sampler_bwd always hands it zeros):
    gx pre-filled with random R must come back as R + (the result into zeros), within 1e-6 of its maximum (float atomics add in
    any order); with gx = NULL nothing is scattered and ggrid is bit for bit the ggrid of the call with gx bound."""
    N, H, W, oH, oW = 2, 20, 70, 33, 65
    rng = np.random.RandomState(31)
    x = to_dev(rng.uniform(-1, 1, size=(N, Cc, H, W)).astype(np.float32), dev)
    grid = to_dev(make_field(family, N, H, W, oH, oW, rng), dev)
    gy = to_dev(rng.normal(size=(N, Cc, oH, oW)).astype(np.float32), dev)
    R = rng.normal(size=(N, Cc, H, W)).astype(np.float32)
    gx0, gg0 = torch.zeros_like(x), torch.empty_like(grid)
    _sampler_bwd_raw(ops, x, grid, gy, gg0, gx0)
    gxr, ggr = to_dev(R, dev), torch.empty_like(grid)
    _sampler_bwd_raw(ops, x, grid, gy, ggr, gxr)
    ggn = torch.full_like(grid, np.nan)
    _sampler_bwd_raw(ops, x, grid, gy, ggn, None)
    want = R.astype(F64) + to_np(gx0)
    assert np.abs(to_np(gxr) - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(to_np(gx0)).max() > 0
    np.testing.assert_array_equal(to_np(ggr), to_np(gg0))
    np.testing.assert_array_equal(to_np(ggn), to_np(gg0))


def test_interp_bwd_zeroes_gx(ops, dev):
    """sfm_sampler_interp_bwd: gx, if bound, is zero-FILLED (spational_transformer_sampler_interp.py:148), whatever it held."""
    N, Cc, H, W = 2, 3, 12, 20
    rng = np.random.RandomState(32)
    x = to_dev(rng.uniform(-1, 1, size=(N, Cc, H, W)).astype(np.float32), dev)
    grid = to_dev(np.stack([rng.uniform(-1, W, size=(N, H, W)), rng.uniform(-1, H, size=(N, H, W))], 1).astype(np.float32), dev)
    gy = to_dev(rng.normal(size=(N, Cc, H, W)).astype(np.float32), dev)
    gx = to_dev(rng.normal(size=(N, Cc, H, W)).astype(np.float32) + 5, dev)
    gg = torch.empty_like(grid)
    ops.check(ops.lib.sfm_sampler_interp_bwd(_p(x), _p(grid), _p(gy), _p(gg), _p(gx), N, Cc, H, W, H, W, _stream(ops)))
    assert not to_np(gx).any()
    _, want = ops.interp_bwd(x, grid, gy, want_gx=False)
    np.testing.assert_array_equal(to_np(gg), to_np(want))


def test_warp_bwd_accumulates_into_d_src(ops, synth, dev):
    """include/sfmwarp.h: d_src of sfm_warp_bwd is ACCUMULATED (ops.warp_bwd zeroes it): into random R it must give R + (the
    result into zeros) within 1e-6 of its maximum, and leave d_depth / d_pose as the call without d_src computes them."""
    N, Cc, H, W = 2, 3, 16, 52
    d = synth.make_inputs(B=N, H=H, W=W, n_src=1, n_scales=1, seed=33)
    rng = np.random.RandomState(33)
    imgs = to_dev(d["src"].reshape(N, -1, H, W)[:, :Cc], dev)
    depth = to_dev((1.0 / d["disps"][0]).reshape(N, H * W), dev)
    pose, K = to_dev(d["poses"][0], dev), to_dev(d["intrinsics"][:, 0], dev)
    g = to_dev(rng.normal(size=(N, Cc, H, W)).astype(np.float32), dev)
    dd0, dp0, ds0 = ops.warp_bwd(imgs, depth, pose, K, g, want_d_src=True)
    R = rng.normal(size=(N, Cc, H, W)).astype(np.float32)
    ds, dd, dp = to_dev(R, dev), torch.empty_like(dd0), torch.empty_like(dp0)
    nbytes = ops.lib.sfm_warp_bwd_workspace_bytes(N, H, W)
    ws = torch.empty((nbytes // 4 + 1,), dtype=torch.float32, device=dev)
    ops.check(ops.lib.sfm_warp_bwd(_p(imgs), _p(depth), 1, _p(pose), _p(K), _p(g), _p(dd), _p(dp), _p(ds), _p(ws), nbytes,
                                   N, Cc, H, W, _stream(ops)))
    want = R.astype(F64) + to_np(ds0)
    assert np.abs(to_np(ds0)).max() > 0
    assert np.abs(to_np(ds) - want).max() <= 1e-6 * np.abs(want).max()
    np.testing.assert_array_equal(to_np(dd), to_np(dd0))
    np.testing.assert_array_equal(to_np(dp), to_np(dp0))


# ------------------------------------------------------------------------------------------------------------------------
# F.resize_images (models/base_model.py:70-72), the pyramids, data_augmentation
# ------------------------------------------------------------------------------------------------------------------------
def resize_tol64(H, W, oH, oW):
    """fp64 comparison of an align-corners resize of [-1, 1] images: the kernel samples at float32(linspace), within half an ulp
    of the exact position; the value moves by at most 2 per pixel of position in each direction -> 2e-6 (the fp32 tests'
    atol) + 2 ulp(max(H, W))"""
    return 2e-6 + 2 * float(np.spacing(np.float32(max(H, W))))


@pytest.mark.parametrize("shape,out", [
    ((2, 3, 16, 24), (32, 48)), ((1, 2, 10, 13), (31, 40)),                   # upsampling: 2x, 3x + 1
    ((2, 1, 17, 19), (1, 7)), ((1, 3, 9, 23), (5, 1)), ((2, 2, 11, 9), (1, 1)),  # a 1-row / 1-column / 1-pixel output
    ((1, 1, 1, 1), (3, 4)), ((2, 2, 1, 9), (4, 5)), ((1, 3, 7, 1), (3, 6)),    # 1-pixel, 1-row, 1-column inputs
    ((1, 3, 2, 7), (5, 3)), ((2, 3, 2, 2), (7, 7)), ((1, 2, 9, 2), (4, 1)),    # 2-pixel inputs
    ((3, 21845, 2, 3), (3, 2)),                                               # N*C = 65535, the grid's limit
])
def test_resize_edges(ops, dev, shape, out):
    """sfm_resize_fwd against the fp32 oracle (rtol 1e-5 / atol 2e-6, as tests/test_ops_gpu.py) and the fp64 oracle
    (atol resize_tol64), non-square ratios throughout so that a row step taken from the column count shows."""
    rng = np.random.RandomState(41)
    x = rng.uniform(-1, 1, size=shape).astype(np.float32)
    got = to_np(ops.resize(to_dev(x, dev), out))
    np.testing.assert_allclose(got, O.resize_images(x, out), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(got, O.resize_images(x, out, dtype=F64), rtol=0, atol=resize_tol64(*shape[2:], *out))


@pytest.mark.parametrize("shape", [(2, 3, 37, 70), (1, 1, 1, 1), (1, 2, 1, 64), (2, 3, 128, 256)])
def test_resize_to_the_same_size_is_the_identity(ops, dev, shape):
    """oH, oW = H, W: linspace(0, L-1, L) is 0, 1, ..., and every weight is 0 or 1: the input, bit for bit"""
    x = np.random.RandomState(42).uniform(-1, 1, size=shape).astype(np.float32)
    np.testing.assert_array_equal(to_np(ops.resize(to_dev(x, dev), shape[2:])), x)


@pytest.mark.parametrize("shape,n_scales", [((2, 3, 128, 256), 8), ((1, 6, 37, 70), 6), ((2, 3, 9, 5), 3)])
def test_pyramids_down_to_one_pixel(ops, dev, shape, n_scales):
    """sfm_pyramid_fwd / _hwc_fwd / _pair_hwc_fwd with scales down to 1 px (128x256 at 8 scales ends at 1x2; 37x70 at 6 ends at
    1x2 with W % 4 != 0).  Each scale against the fp64 resize (resize_tol64) and bit for bit the single resize; HWC the planar
    values interleaved, bit for bit; the pair launch the two single pyramids, and the band kernel the per-pixel kernel, bit
    for bit."""
    N, Cc, H, W = shape
    rng = np.random.RandomState(43)
    x = rng.uniform(-1, 1, size=shape).astype(np.float32)
    xd = to_dev(x, dev)
    planar = ops.pyramid(xd, n_scales)
    assert (H >> (n_scales - 1)) >= 1 and (W >> (n_scales - 1)) >= 1
    for s in range(1, n_scales):
        oh, ow = H >> s, W >> s
        got = to_np(planar[s])
        np.testing.assert_allclose(got, O.resize_images(x, (oh, ow), dtype=F64), rtol=0, atol=resize_tol64(H, W, oh, ow))
        np.testing.assert_array_equal(got, to_np(ops.resize(xd, (oh, ow))))
    hwc = ops.pyramid_hwc(xd, n_scales)
    for s in range(n_scales):
        np.testing.assert_array_equal(to_np(hwc[s]), to_np(ops.to_hwc(planar[s])))
    if Cc == 3:
        src = to_dev(rng.uniform(-1, 1, size=(N, 6, H, W)).astype(np.float32), dev)
        band = [to_np(a).copy() for pyr in ops.pyramid_pair_hwc(xd, src, n_scales) for a in pyr]
        per_pixel = [to_np(a).copy() for pyr in ops.pyramid_pair_hwc(xd, src, n_scales, per_pixel=True) for a in pyr]
        singles = [to_np(a) for a in hwc] + [to_np(a) for a in ops.pyramid_hwc(src, n_scales)]
        for a, b, c in zip(band, per_pixel, singles):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)


def _augment(ops, dev, imgs, params):
    B, Fr, Cc, H, W = imgs.shape
    x, p = to_dev(imgs, dev), to_dev(np.asarray(params, np.float32), dev)
    out = torch.empty_like(x)
    ops.check(ops.lib.sfm_augment_fwd(_p(x), _p(p), _p(out), B, Fr, Cc, H, W, _stream(ops)))
    return to_np(out)


@pytest.mark.parametrize("Cc,Fr,H,W", [(1, 1, 17, 23), (3, 5, 17, 23), (4, 1, 32, 104), (3, 1, 9, 7), (4, 5, 13, 31)])
def test_augment_edges(ops, dev, Cc, Fr, H, W):
    """sfm_augment_fwd against the oracle's data_augmentation (kitti_raw_transformed.py:23-74) with 9 samples of mixed parameters:
    scale 1.0 at offset 0 (the identity: bit for bit), the largest scale at the largest offsets with and without the flip, and
    random draws.  fp32 oracle at rtol 1e-5 / atol 2e-6 (tests/test_api_gpu.py), fp64 oracle at resize_tol64."""
    B = 9
    rng = np.random.RandomState(44 + Cc + Fr)
    imgs = rng.uniform(-1, 1, size=(B, Fr, Cc, H, W)).astype(np.float32)
    draws = []
    for b in range(B):
        xs, ys = (1.0, 1.0) if b < 2 else ((1.15, 1.15) if b < 5 else tuple(rng.uniform(1, 1.15, 2)))
        sh, sw = int(H * ys), int(W * xs)
        if b < 2:
            oy = ox = 0
        elif b < 5:
            oy, ox = sh - H, sw - W
        else:
            oy, ox = rng.randint(0, sh - H + 1), rng.randint(0, sw - W + 1)
        flip = b in (1, 3, 4, 6)
        draws.append((xs, ys, sh, sw, oy, ox, flip))
    params = [(sh, sw, oy, ox, float(flip)) for (_, _, sh, sw, oy, ox, flip) in draws]
    got = _augment(ops, dev, imgs, params)
    np.testing.assert_array_equal(got[0], imgs[0])
    np.testing.assert_array_equal(got[1], imgs[1][..., ::-1])
    K = np.eye(3, dtype=np.float32)
    for b, (xs, ys, sh, sw, oy, ox, flip) in enumerate(draws):
        for dtype, kw in ((np.float32, dict(rtol=1e-5, atol=2e-6)), (F64, dict(rtol=0, atol=resize_tol64(H, W, sh, sw)))):
            t, s_, _ = O.data_augmentation(imgs[b, 0], imgs[b, 1:], K, xs, ys, oy, ox, flip, dtype=dtype)
            np.testing.assert_allclose(got[b], np.concatenate([t[None], s_]), err_msg="sample %d %s" % (b, dtype.__name__), **kw)


# ------------------------------------------------------------------------------------------------------------------------
# DispNet's activation (models/disp_net.py:7-8,104-122): sfm_disp_act_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", [[1, 255, 256, 0, 257, 65537, 3, 1000], [0, 7, 0, 0, 512, 1, 0, 4097], [300]])
def test_disp_act_ragged_empty_and_saturated(ops, dev, numel):
    """Up to 8 scales of ragged sizes (not multiples of the 256-thread block) with empty scales between non-empty ones, logits
    in {0, +-5, +-15, +-30, +-90} and N(0, 3).
      * forward against fp64 10 sigma(x) + 0.01: 2e-6 relative, element-wise;
      * backward against fp64 g 10 sigma (1 - sigma).  The kernel recovers s = (disp - 0.01) / 10 from the float32 disp it is
        handed (the ABI passes disp, not x), where Chainer's sigmoid backward uses its own float32 output y (1 - y).  Near
        saturation 1 - s is then only known to the resolution of disp: the error is |g| times the forward's own error of disp
        plus the rounding of the recovery, at most 2 ulp(disp).  Bound, element-wise everywhere:
            |g_x - want| <= |g| (|disp - disp64| + 2 ulp(disp)) + 2e-4 |want|,
        and 2e-4 relative alone where |x| <= 6.  (Between 6 and 8 the one-ulp term alone reaches 3.8e-4 of the value at
        x = 7.9; at |x| >= 15 it is all there is: 1 - s is below the resolution of disp and the gradient is a few ulp of
        disp times |g| -- never larger.)"""
    rng = np.random.RandomState(51)
    special = np.array([0, 5, -5, 15, -15, 30, -30, 90, -90], np.float32)
    xs = []
    for n in numel:
        a = rng.normal(0, 3, size=n).astype(np.float32)
        a[: min(n, 2 * len(special))] = np.tile(special, 2)[: min(n, 2 * len(special))]
        xs.append(to_dev(a.reshape(n), dev))
    disps = ops.disp_act_fwd(xs)
    gs = [to_dev(rng.normal(size=n).astype(np.float32), dev) for n in numel]
    g_x = ops.disp_act_bwd(disps, gs)
    worst = [0.0, 0.0]
    for x, dd, g, gxk in zip(xs, disps, gs, g_x):
        x64, dd, g, gxk = to_np(x).astype(F64), to_np(dd), to_np(g).astype(F64), to_np(gxk)
        if x64.size == 0:
            assert dd.size == 0 and gxk.size == 0
            continue
        s = 1.0 / (1.0 + np.exp(-x64))
        d64 = 10.0 * s + 0.01
        rel = np.abs(dd - d64) / d64
        assert rel.max() <= 2e-6, rel.max()
        want = g * 10.0 * s * (1.0 - s)
        err = np.abs(gxk - want)
        bound = np.abs(g) * (np.abs(dd - d64) + 2 * np.spacing(dd).astype(F64)) + 2e-4 * np.abs(want)
        assert (err <= bound).all(), "g_x beyond the ulp bound at x = %s" % x64[err > bound][:5]
        mid = np.abs(x64) <= 6
        assert (err[mid] <= 2e-4 * np.abs(want[mid])).all(), "g_x beyond 2e-4 relative at x = %s" % x64[mid][err[mid] > 2e-4 * np.abs(want[mid])][:5]
        worst[0] = max(worst[0], float(rel.max()))
        worst[1] = max(worst[1], float((err / np.maximum(bound, 1e-300)).max()))
    parity_note("disp_act %s: forward max rel %.2e (tol 2e-6), backward at most %.2f of the ulp bound" % (numel, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------------------------------
# proj_tgt_to_src (models/transform.py:64-91): sfm_pose_proj_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
PI32 = np.float32(np.pi)                                  # 3.14159274 > pi: clipped
PI32_IN = np.nextafter(PI32, np.float32(0))               # 3.14159250 < pi: not clipped


def proj_tgt_to_src64(pose, K):
    """proj_tgt_to_src (transform.py:11-91) in float64 on the angles F.clip leaves in the reference's float32 arrays: clip(x, -pi, pi)
    of a float32 array is float32(+-pi) = +-3.14159274 at the bounds (the fp64 oracle would clip once more, to the double pi)"""
    th = np.clip(pose[:, :3], -PI32, PI32).astype(F64)
    c, s = np.cos(th), np.sin(th)
    N = pose.shape[0]
    z, o = np.zeros(N), np.ones(N)
    X = np.stack([o, z, z, z, c[:, 0], -s[:, 0], z, s[:, 0], c[:, 0]], 1).reshape(N, 3, 3)
    Y = np.stack([c[:, 1], z, s[:, 1], z, o, z, -s[:, 1], z, c[:, 1]], 1).reshape(N, 3, 3)
    Z = np.stack([c[:, 2], -s[:, 2], z, s[:, 2], c[:, 2], z, z, z, o], 1).reshape(N, 3, 3)
    T = np.zeros((N, 4, 4))
    T[:, :3, :3] = np.matmul(np.matmul(X, Y), Z)
    T[:, :3, 3] = pose[:, 3:]
    T[:, 3, 3] = 1
    Tabs = np.abs(T)                                       # ... and the magnitudes its rounding errors scale with
    Tabs[:, :3, :3] = np.matmul(np.matmul(np.abs(X), np.abs(Y)), np.abs(Z))
    return np.matmul(O._K4(K, F64), T), np.matmul(np.abs(O._K4(K, F64)), Tabs)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_pose_proj_block_edges_and_clipped_angles(ops, dev, N):
    """sfm_pose_proj_fwd / _bwd for N across the 64-thread block, a skewed K, and angles at float32(+-pi), one float inward of
    it, and +-4 (clipped by F.clip, transform.py:23).
      * forward against fp64: |err| <= 1e-6 |K4| . (|X| . |Y| . |Z|, |t|) element-wise, the error bound of the products
        of the chain for factors accurate to a few ulp.  The fp64 evaluation takes the clipped angle as the reference's float32 F.clip leaves it
        (float32(pi), whose sine is -8.7e-8, not 1e-16); where nothing is clipped it is the fp64 oracle's;
      * backward against torch float64 AUTOGRAD of the reference's chain (tests/test_oracle_vs_torch_cpu.py), not the
        hand-derived backward: rtol 2e-4 / atol 2e-4 of the maximum (tests/test_ops_gpu.py);
      * d(angle) exactly 0 wherever the angle is clipped, and the same zeros in autograd."""
    from test_oracle_vs_torch_cpu import proj_tgt_to_src as torch_proj
    rng = np.random.RandomState(60 + N)
    pose = np.concatenate([rng.normal(0, 0.5, size=(N, 3)), rng.normal(0, 0.3, size=(N, 3))], axis=1).astype(np.float32)
    special = np.array([PI32, -PI32, PI32_IN, -PI32_IN, 4.0, -4.0], np.float32)
    pick = rng.uniform(size=(N, 3)) < 0.4
    pose[:, :3][pick] = special[rng.randint(0, len(special), size=int(pick.sum()))]
    if N >= 6:
        pose[:6, 0] = special
    K = np.tile(np.array([[241.7, 0, 204.2], [0, 246.3, 59.0], [0, 0, 1]], np.float32), (N, 1, 1))
    K[:, 0, 1] = rng.normal(0, 3.0, N)                    # skew
    K[:, 0, 0] *= rng.uniform(0.5, 2, N).astype(np.float32)
    pd, Kd = to_dev(pose, dev), to_dev(K, dev)
    proj = to_np(ops.pose_proj_fwd(pd, Kd))
    want, mag = proj_tgt_to_src64(pose, K)
    bound = 1e-6 * mag
    assert (np.abs(proj - want) <= bound).all(), np.abs(proj - want).max()
    unclipped = ((pose[:, :3] > -np.pi) & (pose[:, :3] < np.pi)).all(1)       # there the fp64 oracle is the same function
    np.testing.assert_allclose(want[unclipped], O.proj_tgt_to_src(pose[unclipped], K[unclipped], dtype=F64), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(proj[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (N, 1)))
    g = rng.normal(size=(N, 4, 4)).astype(np.float32)
    got = to_np(ops.pose_proj_bwd(pd, Kd, to_dev(g, dev)))
    vt = torch.tensor(pose, dtype=torch.float64, requires_grad=True)
    (torch_proj(vt, torch.tensor(K, dtype=torch.float64)) * torch.tensor(g, dtype=torch.float64)).sum().backward()
    w = vt.grad.numpy()
    np.testing.assert_allclose(got, w, rtol=2e-4, atol=2e-4 * np.abs(w).max())
    clipped = ~((pose[:, :3] > -np.pi) & (pose[:, :3] < np.pi))
    assert clipped.any() or N < 6
    assert not got[:, :3][clipped].any() and not w[:, :3][clipped].any()
    if N >= 6:
        assert (got[2:4, 0] != 0).all(), "float32(pi) one step inward is not clipped"
