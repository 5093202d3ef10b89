"""References for the backward of F.resize_images (tests/test_resize_bwd_cpu.py, tests/test_resize_bwd_gpu.py): the fp64 autograd
of torch's align-corners bilinear interpolation on the CPU, a NumPy emulation of the kernel's fp32 arithmetic and summation order,
and the tolerance that separates the two -- derived, not measured."""
import numpy as np

F32 = np.float32

# (input shape, output size): tests/test_ops_edges_gpu.py::test_resize_edges with input and output swapped in role, the odd
# pyramid ratios and a 16x upsample
EDGE_CASES = [
    ((2, 3, 16, 24), (32, 48)), ((1, 2, 10, 13), (31, 40)),                      # upsampling
    ((2, 1, 17, 19), (1, 7)), ((1, 3, 9, 23), (5, 1)), ((2, 2, 11, 9), (1, 1)),  # one-row, one-column, one-pixel outputs
    ((1, 1, 1, 1), (3, 4)), ((2, 2, 1, 9), (4, 5)), ((1, 3, 7, 1), (3, 6)),      # one-pixel, one-row, one-column inputs
    ((1, 3, 2, 7), (5, 3)), ((2, 3, 2, 2), (7, 7)), ((1, 2, 9, 2), (4, 1)),      # two-pixel inputs
    ((3, 21845, 2, 3), (3, 2)),                                                 # N*C = 65535, the forward's grid limit
    ((1, 1, 37, 70), (18, 35)), ((1, 1, 37, 70), (9, 17)), ((1, 1, 37, 70), (4, 8)),   # odd pyramid ratios
    ((1, 1, 8, 26), (128, 416)),                                                # 16x upsample
]
# steps of exactly 0.5, 0.25, 2 and 1: every weight is dyadic, so integer gradients give exact sums in any order and precision
EXACT_CASES = [
    ((2, 3, 5, 7), (9, 13)), ((2, 3, 3, 4), (9, 13)), ((2, 3, 9, 13), (5, 7)), ((2, 3, 37, 70), (37, 70)), ((1, 2, 1, 64), (1, 64)),
]
PYRAMID_CASES = [((2, 3, 128, 256), 8), ((1, 6, 37, 70), 6), ((2, 3, 9, 5), 3)]


def edge_gy(shape, out, seed=61):
    """uniform in [-1, 1]"""
    return np.random.RandomState(seed).uniform(-1, 1, size=shape[:2] + tuple(out)).astype(F32)


def exact_gy(shape, out, seed=62):
    """integers in [-8, 8]"""
    return np.random.RandomState(seed).randint(-8, 9, size=shape[:2] + tuple(out)).astype(F32)


def axis_taps(n, on):
    """(tap0, tap1, w0, w1) of the `on` outputs along an axis of n inputs, as resize_coord / resize_taps form them: the position
    o * step with step = (n - 1) / (on - 1) in double, rounded to float32; one output samples at 0"""
    step = np.float64(n - 1) / np.float64(on - 1) if on > 1 else np.float64(0)
    u = (np.arange(on, dtype=np.float64) * step).astype(F32)
    t0 = np.clip(np.floor(u).astype(np.int64), 0, max(n - 2, 0))
    t1 = np.minimum(t0 + 1, n - 1)
    w1 = u - t0.astype(F32)
    w0 = F32(1) - w1
    assert w0.dtype == F32 and w1.dtype == F32
    return t0, t1, w0, w1


def touch_count(n, on):
    """the largest number of outputs whose taps touch one input index (c_y, c_x of the tolerance)"""
    t0, t1, _, _ = axis_taps(n, on)
    hits = np.zeros((n,), dtype=np.int64)
    for o in range(on):
        for i in {int(t0[o]), int(t1[o])}:
            hits[i] += 1
    return int(hits.max())


def ref64(gy, in_hw):
    """R^T gy in fp64: autograd of torch.nn.functional.interpolate(mode="bilinear", align_corners=True) on the CPU
    (tests/test_oracle_vs_torch_cpu.py holds the oracle's forward equal to it to 1e-12)"""
    import torch
    g = torch.from_numpy(np.asarray(gy, dtype=np.float64))
    x = torch.zeros(tuple(g.shape[:2]) + tuple(int(v) for v in in_hw), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.interpolate(x, size=tuple(g.shape[2:]), mode="bilinear", align_corners=True)
    y.backward(g)
    return x.grad.numpy()


def tol(gy, in_hw):
    """atol of one term: c_y * c_x * max|gy| * (2 * spacing(float32(max(H, W))) + 2^-22).  At most c_y * c_x outputs contribute to
    one input element; each contribution's weight is off by at most the forward's half-ulp position error per axis (the argument
    of test_ops_edges_gpu.resize_tol64: two spacings of the largest coordinate cover both axes), and forming the two weights, their
    product, the product with gy and the running sum is four fp32 roundings of values of at most max|gy| (4 * 2^-24)."""
    H, W = int(in_hw[0]), int(in_hw[1])
    c = touch_count(H, gy.shape[2]) * touch_count(W, gy.shape[3])
    return c * float(np.abs(gy).max()) * (2 * float(np.spacing(F32(max(H, W)))) + 2.0 ** -22)


def emulate(gys, in_hw):
    """sum_k R_k^T gys[k] in the kernel's fp32 arithmetic and order: per input element the contributions gy * (wv * wu), added
    term after term in ascending (oy, ox); of an axis' two taps the one that lands on the element, their sum where both do."""
    H, W = int(in_hw[0]), int(in_hw[1])
    gx = np.zeros(gys[0].shape[:2] + (H, W), dtype=F32)
    for gy in gys:
        gy = np.asarray(gy, dtype=F32)
        v0, v1, wv0, wv1 = axis_taps(H, gy.shape[2])
        u0, u1, wu0, wu1 = axis_taps(W, gy.shape[3])
        for oy in range(gy.shape[2]):
            rows = [(v0[oy], wv0[oy] + wv1[oy])] if v0[oy] == v1[oy] else [(v0[oy], wv0[oy]), (v1[oy], wv1[oy])]
            for ox in range(gy.shape[3]):
                cols = [(u0[ox], wu0[ox] + wu1[ox])] if u0[ox] == u1[ox] else [(u0[ox], wu0[ox]), (u1[ox], wu1[ox])]
                g = gy[:, :, oy, ox]
                for r, wv in rows:
                    for c, wu in cols:
                        gx[:, :, r, c] += g * F32(wv * wu)
    assert gx.dtype == F32
    return gx
