"""The pseudo-code of include/sfmwarp_min_reproj.h restated in NumPy: the reference of tests/test_min_reproj_cpu.py and
tests/test_min_reproj_gpu.py.  Comparisons run on the float32 values themselves, so winner, count and g_err are exact; the sums
are math.fsum of the float64 values of the kept `best` (the exact sum, rounded once).  A plain module: no fixtures, no device."""
import math

import numpy as np

NORM_KEPT, NORM_ALL = 0, 1


def select(err, valid=None, ident=None):
    """One scale: err (B,n_err,h,w) float32, valid the same shape or None, ident (B,n_ident,h,w) or None
    -> (winner (B,h,w) int8, best (B,h,w) float32: +inf where no source competes)"""
    err = np.asarray(err, np.float32)
    B, n, h, w = err.shape
    best = np.full((B, h, w), np.inf, np.float32)
    win = np.full((B, h, w), -1, np.int8)
    with np.errstate(invalid="ignore"):
        for i in range(n):                                            # ascending: the first index wins a tie
            ok = err[:, i] < best                                     # NaN and +inf never win
            if valid is not None:
                ok &= np.asarray(valid, np.float32)[:, i] > 0
            best = np.where(ok, err[:, i], best)
            win = np.where(ok, np.int8(i), win)
        keep = win >= 0
        if ident is not None:
            ident = np.asarray(ident, np.float32)
            floor = np.full((B, h, w), np.inf, np.float32)
            for j in range(ident.shape[1]):
                floor = np.where(ident[:, j] < floor, ident[:, j], floor)
            keep &= best < floor                                      # strict
    return np.where(keep, win, np.int8(-1)).astype(np.int8), best


def denominator(count, B, h, w, norm):
    return float(max(count, 1)) if norm == NORM_KEPT else float(B * h * w)


def forward(errs, valids, idents, weights, norm):
    """Every scale: errs[s], valids (None or a list with None entries), idents (None or a list), weights[s] (float32 values)
    -> (loss (S+1,) float64: the values BEFORE the final rounding to float32, count (S,) int32, [winner_s])"""
    S = len(errs)
    loss, count, winners = np.zeros(S + 1, np.float64), np.zeros(S, np.int32), []
    terms = []
    for s in range(S):
        B, _, h, w = errs[s].shape
        win, best = select(errs[s], None if valids is None else valids[s], None if idents is None else idents[s])
        keep = win >= 0
        count[s] = int(keep.sum())
        total = math.fsum(best[keep].astype(np.float64).tolist())
        denom = denominator(count[s], B, h, w, norm)
        loss[s] = total / denom
        terms.append(float(np.float32(weights[s])) * total / denom)
        winners.append(win)
    loss[S] = math.fsum(terms)
    return loss, count, winners


def backward(winners, count, g_loss, n_err, weights, norm):
    """-> [g_err_s (B,n_err,h,w) float32]: c_s, one quotient of doubles rounded to float32, at the winner of a kept pixel, else 0"""
    S = len(winners)
    g_loss = np.asarray(g_loss, np.float32)
    out = []
    for s, win in enumerate(winners):
        B, h, w = win.shape
        num = np.float64(g_loss[s]) + np.float64(np.float32(weights[s])) * np.float64(g_loss[S])
        c = np.float32(num / np.float64(denominator(int(count[s]), B, h, w, norm)))
        out.append(np.where(win[:, None] == np.arange(n_err, dtype=np.int8)[None, :, None, None], c, np.float32(0)).astype(np.float32))
    return out


def within_one_ulp(got, want64):
    """|got - want64| <= 1 float32 ulp at want64, `got` a float32: the kernel's fp64 sum is far below half an ulp off the exact one, the
    1 ulp covers the final rounding"""
    want32 = np.float32(want64)
    return abs(float(got) - float(want64)) <= float(np.spacing(np.abs(want32))) if np.isfinite(want32) else got == want32
