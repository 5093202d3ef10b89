"""include/sfmwarp_pairwise.h restated in NumPy: float32 products, fp64 sums, the same selections -- and the same header's
formulas once more as compute_pairwise_loss / mean_on_mask would be written in torch (float64, on the CPU, differentiated by
autograd), which is what the restatement is held against.  A plain module: no fixtures, no device."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
ONE = F32(1.0)


def keep_mask(e, valid, ident, c):
    """the header's keep for one (scale, source): arrays (B,h,w)"""
    k = np.ones(e.shape, dtype=bool)
    if valid is not None:
        k &= valid > 0
    if ident is not None:
        with np.errstate(invalid="ignore"):
            k &= (e if c is None else c) < ident
    return k


def forward(errs, diffs, valids, idents, cmps, weights, min_counts):
    """-> (loss float32 (2*S*n+2,), count int32 (S*n,), [keep_s int8 (B,n,h,w)]); valids: None or a list with None entries"""
    S, n = len(errs), errs[0].shape[1]
    N = S * n
    loss, count, keeps = np.zeros(2 * N + 2, F32), np.zeros(N, np.int32), []
    qp, qg = np.zeros(N, F64), np.zeros(N, F64)
    for s in range(S):
        keep = np.zeros(errs[s].shape, np.int8)
        for i in range(n):
            e, d = errs[s][:, i], diffs[s][:, i]
            k = keep_mask(e, None if valids is None or valids[s] is None else valids[s][:, i],
                          None if idents is None else idents[s][:, i], None if cmps is None else cmps[s][:, i])
            with np.errstate(invalid="ignore", over="ignore"):
                t = (e * (ONE - d)).astype(F32)             # one float32 subtraction, one float32 product
            cnt = int(k.sum())
            sp, sg = t[k].astype(F64).sum(), d[k].astype(F64).sum()      # selection: a dropped NaN stays out
            j = s * n + i
            keep[:, i], count[j] = k, cnt
            qp[j] = sp / max(cnt, 1) if cnt > min_counts[0] else 0.0
            qg[j] = sg / max(cnt, 1) if cnt > min_counts[1] else 0.0
        keeps.append(keep)
    loss[:N], loss[N:2 * N] = qp.astype(F32), qg.astype(F32)
    for q, at in ((qp, 2 * N), (qg, 2 * N + 1)):
        total = None
        for s in range(S):
            inner = q[s * n]
            for i in range(1, n):
                inner = inner + q[s * n + i]
            term = F64(F32(weights[s])) * inner
            total = term if total is None else total + term
        loss[at] = F32(total)
    return loss, count, keeps


def backward(errs, diffs, keeps, count, g_loss, weights, min_counts, detach_weight):
    """-> ([g_err_s], [g_diff_s]) float32, to be compared bit for bit"""
    S, n = len(errs), errs[0].shape[1]
    N = S * n
    g_errs, g_diffs = [], []
    for s in range(S):
        ge, gd = np.zeros(errs[s].shape, F32), np.zeros(errs[s].shape, F32)
        for i in range(n):
            j = s * n + i
            cnt, w = int(count[j]), F64(F32(weights[s]))
            cp = F32((F64(g_loss[j]) + w * F64(g_loss[2 * N])) / F64(max(cnt, 1))) if cnt > min_counts[0] else F32(0)
            cg = F32((F64(g_loss[N + j]) + w * F64(g_loss[2 * N + 1])) / F64(max(cnt, 1))) if cnt > min_counts[1] else F32(0)
            e, d, k = errs[s][:, i], diffs[s][:, i], keeps[s][:, i] != 0
            with np.errstate(invalid="ignore", over="ignore"):
                a = ((ONE - d) * cp).astype(F32)
                b = np.full(e.shape, cg, F32) if detach_weight else (cg - (e * cp).astype(F32)).astype(F32)
            ge[:, i], gd[:, i] = np.where(k, a, F32(0)), np.where(k, b, F32(0))
        g_errs.append(ge)
        g_diffs.append(gd)
    return g_errs, g_diffs


def mean_on_mask(diff, mask, min_count):
    """SC-SfMLearner's mean_on_mask with its threshold as a parameter (its own: mask.sum() > 10000 on the expanded mask)"""
    if mask.sum() > min_count:
        return (diff * mask).sum() / mask.sum().clamp(min=1)
    return (diff * 0).sum()


def torch_statement(errs, diffs, valids, idents, cmps, weights, min_counts, detach_weight, g_loss):
    """compute_pairwise_loss's tail in float64 torch on the CPU for every (scale, source), and its autograd gradients for the upstream
    gradients g_loss in the layout of the header -> (loss float64 (2*S*n+2,), [g_err_s], [g_diff_s] float64)"""
    S, n = len(errs), errs[0].shape[1]
    E = [torch.from_numpy(a.astype(F64)).requires_grad_() for a in errs]
    D = [torch.from_numpy(a.astype(F64)).requires_grad_() for a in diffs]
    photo, geom = [], []
    tp = tg = 0.0
    for s in range(S):
        for i in range(n):
            e, d = E[s][:, i], D[s][:, i]
            mask = torch.ones_like(e)
            if valids is not None and valids[s] is not None:
                mask = mask * torch.from_numpy(valids[s][:, i] > 0).to(torch.float64)                   # valid_mask
            if idents is not None:
                c = torch.from_numpy((errs if cmps is None else cmps)[s][:, i].astype(F64))
                mask = mask * (c < torch.from_numpy(idents[s][:, i].astype(F64))).to(torch.float64)     # auto_mask
            weight_mask = 1 - d
            if detach_weight:
                weight_mask = weight_mask.detach()
            photo.append(mean_on_mask(e * weight_mask, mask, min_counts[0]))
            geom.append(mean_on_mask(d, mask, min_counts[1]))
            tp = tp + float(F32(weights[s])) * photo[-1]
            tg = tg + float(F32(weights[s])) * geom[-1]
    loss = torch.stack(photo + geom + [tp, tg])
    (loss * torch.from_numpy(np.asarray(g_loss, F64))).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return loss.detach().numpy(), [zero(t).numpy() for t in E], [zero(t).numpy() for t in D]


def inputs(B, n, hw, seed, valid_none=(), share=0.7):
    """errs in (0.01, 1), diffs in [0, 0.9), valids 0 | 1 (None at the scales of `valid_none`), idents and cmps around errs"""
    rng = np.random.RandomState(seed)
    out = dict(errs=[], diffs=[], valids=[], idents=[], cmps=[])
    for s, (h, w) in enumerate(hw):
        shape = (B, n, h, w)
        e = rng.uniform(0.01, 1.0, shape).astype(F32)
        out["errs"].append(e)
        out["diffs"].append(rng.uniform(0.0, 0.9, shape).astype(F32))
        out["valids"].append(None if s in valid_none else (rng.uniform(size=shape) < share).astype(F32))
        out["idents"].append((e + rng.uniform(-0.2, 0.3, shape)).astype(F32))
        out["cmps"].append(rng.uniform(0.01, 1.0, shape).astype(F32))
    return out


def ulp_distance(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude (0 for equal values, NaN pairs included)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        top = np.maximum(np.abs(a), np.abs(b)).astype(F32)
        dist = np.abs(a - b) / np.spacing(np.maximum(top, np.finfo(F32).tiny)).astype(F64)
    return np.where(both_nan | (a == b), 0.0, dist)
