"""NumPy restatement of what sfm_warp_full_res_* adds to the warp (tests/test_warp_full_res_cpu.py, tests/test_warp_full_res_gpu.py):
the align-corners upsampling of a disparity to the full resolution and its adjoint, in the kernels' arithmetic and order, in any
floating-point type -- float32 is the statement of the kernels, float64 the same map with exact-enough weights."""
import numpy as np

F32, F64 = np.float32, np.float64

# (H, W) of the full resolution and the (h, w) of each disparity: the shapes of tests/test_warp_full_res_gpu.py
SHAPES = {
    "24x40": ((24, 40), [(24, 40), (12, 20), (6, 10), (3, 5)]),             # halvings
    "13x21": ((13, 21), [(13, 21), (7, 10), (1, 1)]),                       # non-integer ratios; one row and column: a step of 0
    "130x127": ((130, 127), [(130, 127), (65, 63), (17, 9)]),               # 65 blocks of 256 pixels per image
}


def axis_taps(n, on, dtype=F32):
    """(tap0, tap1, w0, w1) of the `on` outputs along an axis of n inputs as resize_coord / resize_taps form them: the position
    o * step with step = (n - 1) / (on - 1) in double -- rounded to float32 in the kernels, kept in float64 for dtype float64"""
    step = F64(n - 1) / F64(on - 1) if on > 1 else F64(0)
    u = (np.arange(on, dtype=F64) * step).astype(dtype)
    t0 = np.clip(np.floor(u).astype(np.int64), 0, max(n - 2, 0))
    t1 = np.minimum(t0 + 1, n - 1)
    w1 = u - t0.astype(dtype)
    w0 = dtype(1) - w1
    assert w0.dtype == dtype and w1.dtype == dtype
    return t0, t1, w0, w1


def upsample(x, out_hw, dtype=F32):
    """x (N,C,h,w) -> (N,C,H,W): resize_blend's three statements -- top = a0 wu0 + a1 wu1, bot likewise, top wv0 + bot wv1"""
    x = np.asarray(x, dtype=dtype)
    H, W = out_hw
    v0, v1, wv0, wv1 = axis_taps(x.shape[2], H, dtype)
    u0, u1, wu0, wu1 = axis_taps(x.shape[3], W, dtype)
    top = x[:, :, v0][:, :, :, u0] * wu0 + x[:, :, v0][:, :, :, u1] * wu1
    bot = x[:, :, v1][:, :, :, u0] * wu0 + x[:, :, v1][:, :, :, u1] * wu1
    y = top * wv0[:, None] + bot * wv1[:, None]
    assert y.dtype == dtype
    return y


def adjoint(gy, in_hw, dtype=F32):
    """gy (N,C,H,W) -> (N,C,h,w), the adjoint of `upsample` as warp_full_gather_kernel (resize_bwd_kernel with one term) adds it up:
    per low-resolution element the contributions gy * (wv * wu) in ascending (oy, ox); of an axis' two taps the one that lands on the
    element, their sum where both do (one input row or column)"""
    gy = np.asarray(gy, dtype=dtype)
    h, w = in_hw
    v0, v1, wv0, wv1 = axis_taps(h, gy.shape[2], dtype)
    u0, u1, wu0, wu1 = axis_taps(w, gy.shape[3], dtype)
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


def adjoint64_aten(gy, in_hw):
    """the independent opinion: float64 autograd of torch.nn.functional.interpolate(mode="bilinear", align_corners=True) on the CPU"""
    import torch
    g = torch.from_numpy(np.asarray(gy, dtype=F64))
    x = torch.zeros(tuple(g.shape[:2]) + tuple(int(v) for v in in_hw), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.interpolate(x, size=tuple(g.shape[2:]), mode="bilinear", align_corners=True).backward(g)
    return x.grad.numpy()


def workspace_bytes(B, n_src, H, W, hw):
    """sfm_warp_full_res_bwd_workspace_bytes as include/sfmwarp_full_res.h states it"""
    need = 48 * n_src * len(hw) * B * -(-(H * W) // 256) + 4 * B * H * W * sum(1 for s in hw if tuple(s) != (H, W))
    return -(-need // 256) * 256 if need else 256
