"""The pseudo-code of include/sfmwarp_disp_smooth.h restated in NumPy: the reference of tests/test_disp_smooth_cpu.py and
tests/test_disp_smooth_gpu.py.  The per-pixel terms are float32 (differences, |.|, exp(-a / 3), the product), their sums are
math.fsum of the float64 values (the exact sum, rounded once); the values come back BEFORE the final rounding to float32.  With it,
`aten_statement`: the term as a user writes it with torch tensors, whose float64 evaluation is the reference of the tolerance
tests and whose float32 evaluation sets their tolerance.  A plain module: no fixtures, no device."""
import math

import numpy as np

EDGE_MEAN_ABS, EDGE_ABS_MEAN = 0, 1
F = np.float32


def aten_statement(disps, imgs, weights, normalize, edge):
    """The term as a user writes it in aten (Monodepth2's get_smooth_loss on disp / (mean + 1e-7) for normalize, "mean_abs"), in the
    dtype and on the device of `disps` (torch tensors, autograd on) -> (total, [per scale])"""
    per_scale = []
    for d, img in zip(disps, imgs):
        if normalize:
            d = d / (d.mean(2, True).mean(3, True) + 1e-7)
        gx, gy = img[:, :, :, :-1] - img[:, :, :, 1:], img[:, :, :-1, :] - img[:, :, 1:, :]
        if edge == "mean_abs":
            ax, ay = gx.abs().mean(1, keepdim=True), gy.abs().mean(1, keepdim=True)
        else:
            ax, ay = gx.mean(1, keepdim=True).abs(), gy.mean(1, keepdim=True).abs()
        sx = (d[:, :, :, :-1] - d[:, :, :, 1:]).abs() * (-ax).exp()
        sy = (d[:, :, :-1, :] - d[:, :, 1:, :]).abs() * (-ay).exp()
        per_scale.append(sx.mean() + sy.mean())
    return sum(w * t for w, t in zip(weights, per_scale)), per_scale


def edge_weights(img, edge):
    """img (B,3,h,w) float32 -> (w_x (B,h,w-1), w_y (B,h-1,w)) float32: exp(-a / 3), a as the header brackets it"""
    img = np.asarray(img, F)

    def weight(e):                        # e (B,3,...): the channel differences
        a = (np.abs(e[:, 0]) + np.abs(e[:, 1])) + np.abs(e[:, 2]) if edge == EDGE_MEAN_ABS else np.abs((e[:, 0] + e[:, 1]) + e[:, 2])
        return np.exp(-(a.astype(F) / F(3))).astype(F)

    return weight(img[:, :, :, 1:] - img[:, :, :, :-1]), weight(img[:, :, 1:] - img[:, :, :-1])


def sample_stats(disp, img, normalize, edge):
    """One scale: disp (B,1,h,w), img (B,3,h,w) -> (B,3) float64: M_b, X_b, Y_b"""
    d = np.asarray(disp, F)[:, 0]
    B, h, w = d.shape
    wx, wy = edge_weights(img, edge)
    tx = (np.abs(d[:, :, 1:] - d[:, :, :-1]) * wx).astype(F)
    ty = (np.abs(d[:, 1:] - d[:, :-1]) * wy).astype(F)
    out = np.zeros((B, 3), np.float64)
    for b in range(B):
        out[b, 0] = math.fsum(d[b].astype(np.float64).ravel().tolist()) / (h * w) + 1e-7 if normalize else 1.0
        out[b, 1] = math.fsum(tx[b].astype(np.float64).ravel().tolist())
        out[b, 2] = math.fsum(ty[b].astype(np.float64).ravel().tolist())
    return out


def coefficients(B, h, w):
    return 1.0 / (B * h * (w - 1)), 1.0 / (B * (h - 1) * w)


def forward(disps, imgs, weights, normalize, edge):
    """Every scale -> (loss (S+1,) float64: the values BEFORE the final rounding to float32, stats (S,B,3) float64)"""
    S = len(disps)
    B = disps[0].shape[0]
    loss, stats = np.zeros(S + 1, np.float64), np.zeros((S, B, 3), np.float64)
    for s in range(S):
        _, _, h, w = disps[s].shape
        cx, cy = coefficients(B, h, w)
        stats[s] = sample_stats(disps[s], imgs[s], normalize, edge)
        loss[s] = math.fsum(((cx * X + cy * Y) / abs(M) for M, X, Y in stats[s]))
    loss[S] = math.fsum(float(F(weights[s])) * loss[s] for s in range(S))
    return loss, stats


def backward(disps, imgs, stats, g_loss, weights, normalize, edge, out=None):
    """-> [g_disp_s (B,1,h,w) float32]; the three per-sample factors in float64, rounded to float32, the rest in float32 in the
    header's order; with `out` (a list of float32 arrays) ONE float32 addition onto it"""
    g_loss = np.asarray(g_loss, F)
    S = len(disps)
    res = []
    for s in range(S):
        d = np.asarray(disps[s], F)[:, 0]
        B, h, w = d.shape
        cx, cy = coefficients(B, h, w)
        wx, wy = edge_weights(imgs[s], edge)
        tx = np.zeros((B, h, w + 1), F)                       # t_x(y,x) at [:, :, x + 1]; zero past both borders
        ty = np.zeros((B, h + 1, w), F)
        tx[:, :, 1:w] = np.sign(d[:, :, 1:] - d[:, :, :-1]) * wx
        ty[:, 1:h] = np.sign(d[:, 1:] - d[:, :-1]) * wy
        ks = np.float64(g_loss[s]) + np.float64(F(weights[s])) * np.float64(g_loss[S])
        g = np.zeros((B, 1, h, w), F)
        for b in range(B):
            M, X, Y = stats[s][b]
            fx, fy = F(ks * cx / abs(M)), F(ks * cy / abs(M))
            fm = F(ks * (cx * X + cy * Y) / (M * abs(M) * (h * w))) if normalize else F(0)
            g[b, 0] = ((fx * (tx[b, :, :-1] - tx[b, :, 1:])).astype(F) + (fy * (ty[b, :-1] - ty[b, 1:])).astype(F)).astype(F) - fm
        res.append(g if out is None else (np.asarray(out[s], F) + g).astype(F))
    return res
