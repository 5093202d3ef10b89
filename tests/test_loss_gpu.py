"""GPU parity of the fused multi-scale loss (sfm_loss_fwd / _bwd / _fwd_bwd through the C ABI)
against the CPU oracle, on identical seeded inputs.

Tolerances (fp32, north_star: 1e-4 relative on the loss):
  * the five reported scalars ............. 1e-4 relative
  * d_disp / d_pose / d_mask / d_src ...... 2e-3 of the array's largest magnitude, element-wise,
    outside knife-edge pixels (see tests/util.py); they are sums of many fp32 terms whose
    order differs between the oracle (NumPy) and the wave-level reductions.
(tests/test_loss_exact_gpu.py compares every element of the same gradients with the fp64 oracle, without a mask, on inputs that have no knife-edge pixel.)
"""
import os

import numpy as np
import pytest

from oracle import sfm_oracle as O
from oracle.parity import knife_mask, position_uncertainty, rel_l2, tap_contrast
from util import assert_close_masked, dilate, parity_note, parity_row, to_dev, to_np

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4
GRAD_TOL = 2e-3
KEYS = ["total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss"]


def _oracle(d, cfg, norm_B=None, want_d_src=False):
    return O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"],
                      backward=True, want_d_src=want_d_src, keep_warped=True, norm_batch=norm_B, **cfg)


def _bind(ops, dev, d, cfg, norm_B=None, want_d_src=False, layout="planar", want_warped=False, projection="fast"):
    fl = ops.FusedLoss(projection=projection, **cfg)
    tgt, src = [to_dev(a, dev) for a in d["tgt_pyr"]], [to_dev(a, dev) for a in d["src_pyr"]]
    if layout == "hwc":      # the same values, pixel-interleaved (SFM_LAYOUT_HWC)
        tgt, src = [ops.to_hwc(a) for a in tgt], [ops.to_hwc(a) for a in src]
    fl.bind(tgt, src, to_dev(d["intrinsics"], dev), [to_dev(a, dev) for a in d["disps"]],
            [to_dev(a, dev) for a in d["poses"]],
            [to_dev(a, dev) for a in d["masks"]] if d["masks"] is not None else None,
            norm_B=norm_B, want_d_src=want_d_src, layout=layout, want_warped=want_warped)
    return fl


WARP_TOL = 1e-4      # north_star: warped pixels within 1e-4 (of the image range, [-1, 1]) of the reference
FLIP_THR = 8e-6      # |x_n| within this of 1: the strict `-1 < x < 1` test (transform.py:129) is decided by the last bits


def position_tolerance(d, s):
    """(dU, dV), each (B,n,h,w): how far apart two correct fp32 evaluations of the sampling positions of scale s may lie
    (oracle/parity.py: first-order error bound from the inputs alone)."""
    per = [position_uncertainty(d["intrinsics"][:, s], pose, d["disps"][s]) for pose in d["poses"]]
    return np.stack([p[0] for p in per], axis=1), np.stack([p[1] for p in per], axis=1)


def value_tolerance(d, ref, s):
    """(B,n,h,w): what the fp32 uncertainty of the sampling position moves the bilinear sample by at each pixel of scale s:
    (contrast between the cell's horizontally adjacent taps) x dU + (vertically adjacent) x dV."""
    dU, dV = position_tolerance(d, s)
    n = ref["uv"][s].shape[1]
    G = [tap_contrast(d["src_pyr"][s][:, 3 * i:3 * i + 3], ref["uv"][s][:, i, 0], ref["uv"][s][:, i, 1]) for i in range(n)]
    Gu, Gv = np.stack([a for a, _ in G], axis=1), np.stack([b for _, b in G], axis=1)
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(Gu * dU + Gv * dV, nan=0.0, posinf=np.inf)


def cell_width_from_position_bound(d, floor=1e-4):
    """scale -> (B,n,h,w): the width of the cell-boundary knife class taken from the fp32 uncertainty of each sample's position
    (never below the flat `floor` px the small tests use): a sample closer to a lattice line than two correct fp32 evaluations may
    lie apart can land in either cell.  Replaces the hand-set widths of round 3 (2.5e-4 px at the full batch, where one sample in
    1.7 M sat 1.2e-4 px from a line; 5e-4 px for a 1408-wide frame, where an ulp of U is 1.2e-4 px)."""
    def width(s):
        dU, dV = position_tolerance(d, s)
        return np.maximum(floor, np.maximum(dU, dV))
    return width


def knife_widths(d, ref, cell_floor=1e-4, abs_floor=3e-5):
    """The widths of the two knife classes that follow from WHERE a sample lands, as keyword arguments of _check_grads, both
    taken from the fp32 uncertainty of each sample's position (oracle/parity.py) and never below the flat widths of the small
    tests: the cell-boundary class (see cell_width_from_position_bound) and the kink of |I^ - I| (models/base_model.py:95) --
    sign(I^ - I) is undecided where |I^ - I| is smaller than what that uncertainty moves I^ by."""
    return dict(cell_thr=cell_width_from_position_bound(d, cell_floor),
                abs_thr=lambda s: np.maximum(abs_floor, value_tolerance(d, ref, s)))


VACUOUS_ALLOWANCE = 1e-3      # a pixel whose position allowance exceeds this (of the range) is in effect not compared ...
VACUOUS_SHARE_CAP = 1e-4      # ... at most 0.01 % of a scale's pixels may be (round-4 verdict: the allowance had no cap below the image range)


def _check_warped(fl, ref, what, d, flat=False, flat_tol=WARP_TOL, max_over_flat=None):
    """The warped images the FUSED kernel computed its loss on (SfmLossDesc.warped, written by the kernel that is benchmarked)
    against the oracle's curr_proj_img (models/base_model.py:90-94), pixel for pixel:
      * the sets of exactly-zero (not in view, :96) pixels agree except at pixels the ORACLE places within FLIP_THR of the strict
        in-view test -- those that differ are counted and printed;
      * flat=True (seam-free inputs, synth.make_inputs(seam="shift"); the reference-order variants on any input): everywhere else
        |I^ - I^_oracle| <= flat_tol of the image range, no other term -- north_star's criterion as it is written;
      * flat=False (the rolled inputs of rounds 1-4: a wrap-around seam of contrast 2.0 in the sources): WARP_TOL of the range + what
        the fp32 uncertainty of the sampling POSITION moves the bilinear sample by at that pixel: (contrast between the cell's
        horizontally adjacent taps) x dU + (vertical) x dV, with (dU, dV) the first-order rounding bound of oracle/parity.py
        (1 .. 2e-4 px at U = 400; unbounded where z -> 0).  On a step edge of contrast 2 NO fp32 evaluation meets a flat 1e-4: the
        fp32 oracle itself is 2.4e-4 from the fp64 one there.  Pixels whose allowance exceeds VACUOUS_ALLOWANCE are in effect not
        compared: they are counted, printed and capped at VACUOUS_SHARE_CAP of a scale.
    `max_over_flat`: cap on the number of pixels above the flat WARP_TOL (None: only printed).
    Returns the number of pixels zeroed differently."""
    assert fl.warped is not None
    n_flip = n_over = n_vac = n_px = 0
    worst = worst_flat = 0.0
    for s, (g, w) in enumerate(zip(fl.warped, ref["warped"])):
        g = to_np(g)
        assert g.shape == w.shape, (g.shape, w.shape)
        assert np.isfinite(g).all(), "%s: non-finite warped pixels at scale %d" % (what, s)
        kz, oz = (g == 0).all(axis=2), (w == 0).all(axis=2)                   # (B,n,h,w)
        mism = kz != oz
        near = ref["margin"][s] < FLIP_THR
        assert not (mism & ~near).any(), "%s scale %d: %d pixels zeroed differently from the oracle AWAY from the strict in-view test" % (
            what, s, int((mism & ~near).sum()))
        n_flip += int(mism.sum())
        scale = max(float(np.abs(w).max()), 1.0)
        err = np.abs(g.astype(np.float64) - w).max(axis=2)
        err[mism] = 0.0
        n_px += err.size
        if flat:
            tol = np.full(err.shape, flat_tol * scale)
        else:
            allow = np.minimum(value_tolerance(d, ref, s), 2.0 * scale)
            vac = allow > VACUOUS_ALLOWANCE * scale
            n_vac += int(vac.sum())
            assert vac.mean() <= VACUOUS_SHARE_CAP, "%s scale %d: %d of %d pixels (%.4f %%) carry a position allowance above %g of the range: the comparison would be vacuous there" % (
                what, s, int(vac.sum()), vac.size, 100 * vac.mean(), VACUOUS_ALLOWANCE)
            tol = WARP_TOL * scale + allow
        bad = err > tol
        assert not bad.any(), "%s scale %d: %d warped pixels off by more than %s; worst %.3g at tolerance %.3g" % (
            what, s, int(bad.sum()), "the flat %g of the range" % flat_tol if flat else "%g + (tap contrast x position uncertainty)" % WARP_TOL,
            float(err[bad].max()), float(tol[bad][np.argmax(err[bad])]))
        n_over += int((err > WARP_TOL * scale).sum())
        worst_flat = max(worst_flat, float(err.max()) / scale)
        worst = max(worst, float((err / tol).max()))
    if max_over_flat is not None:
        assert n_over <= max_over_flat, "%s: %d warped pixels above the flat %g of the range (cap %d)" % (what, n_over, WARP_TOL, max_over_flat)
    crit = ("FLAT %.0e" % flat_tol) if flat else "1e-4 + tap contrast x position uncertainty"
    parity_note("warped pixels %s [%s]: max |I^ - I^_oracle| %.2e of the range; %d of %d pixels above the flat %.0e (worst pixel at %.2f of its tolerance); "
                "%d pixels with an allowance above %.0e (in effect unchecked; cap %.2f %% of a scale); %d pixels zeroed differently (all within %.0e of the strict test)" % (
                    what, crit, worst_flat, n_over, n_px, WARP_TOL, worst, n_vac, VACUOUS_ALLOWANCE, 100 * VACUOUS_SHARE_CAP, n_flip, FLIP_THR))
    parity_row(kind="warped", case=what, criterion=crit, worst_of_range=worst_flat, over_flat=n_over, pixels=n_px, vacuous=n_vac, zeroed_differently=n_flip)
    return n_flip


def _check_losses(loss5, ref, slack=0.0):
    """`slack`: absolute allowance for pixels that sit on the strict `-1 < x < 1` test (only the random sweep passes one:
    counted, bounded and reported there); 0 everywhere else."""
    got = to_np(loss5)
    for k, name in enumerate(KEYS):
        want = ref[name]
        assert abs(got[k] - want) <= LOSS_RTOL * max(abs(want), 1e-6) + slack, (name, got[k], want, slack)


KNIFE_CAP_LARGE, KNIFE_CAP_SMALL, KNIFE_SMALL_PX = 0.01, 0.05, 20000
L2_TOL = 1e-4      # relative L2 error of a gradient array outside knife pixels (next to the element-wise max criterion)


def knife_cap(n_px):
    """Largest share of a scale's pixels that may be excluded from ELEMENT-WISE gradient comparisons: 1 % at image sizes of
    the BASELINE configs; 5 % for the small images of the shape tests, where a handful of dilated pixels is already percents."""
    return KNIFE_CAP_LARGE if n_px >= KNIFE_SMALL_PX else KNIFE_CAP_SMALL


def _knife(ref, s, n_src, thr=8e-6, cell_thr=1e-4, abs_thr=3e-5, clip_thr=5e-5, what=""):
    """Pixels of scale s where the reference's function itself is discontinuous in (disp, pose), so that two
    fp32 evaluations of it may legitimately land on different sides; excluded from ELEMENT-WISE gradient
    comparisons (never from the loss comparison), each class with the footprint it can influence:
      * the strict `-1 < x < 1` test (models/transform.py:129) within `thr` of its boundary: the pixel flips
        between sampled and exactly 0 -> changes the SSIM windows around it -> 5x5 footprint;
      * (1-SSIM)/2 within `clip_thr` of the kinks of F.clip at 0 / 1 (models/base_model.py:142): the SSIM
        partials of that window switch on/off -> 3x3 footprint;
      * the sample within `cell_thr` px of a cell boundary of the bilinear lattice (dI^/du jumps) and
        0 < |I^ - I| < `abs_thr` (kink of F.absolute, models/base_model.py:95): the pixel itself.
    The excluded share is reported (parity_note) and asserted to stay below knife_cap, so the exclusion cannot hide a
    real error."""
    m, flip, clip, own = knife_mask(ref, s, thr, cell_thr, abs_thr, clip_thr)
    share, cap = float(m.mean()), knife_cap(m.shape[-2] * m.shape[-1])     # the cap goes by the size of ONE image
    parity_note("knife %s scale %d (%d px, %d src): excluded %.3f%% (cap %.0f%%): %d flip, %d clip, %d cell/abs pixels" % (
        what, s, m.size, n_src, 100 * share, 100 * cap, int(flip.sum()), int(clip.sum()), int(own.sum())))
    assert share <= cap, "too many knife-edge pixels (%.3f%% > %.0f%%): the exclusion would hide real errors" % (100 * share, 100 * cap)
    return m[:, None]                                 # (B,1,h,w)


def _judged64(got, w32, w64, knife, what, extra=0.0, arraywise=False):
    """Second opinion from the fp64 oracle for an array that misses the flat fp32 criterion: where the gradient is
    ill-conditioned in fp32 (far points: d_disp = -gD / disp^2 amplifies the rounding of the sampling coordinates; d_pose sums
    1e4..1e5 signed terms) BOTH fp32 evaluations sit away from the fp64 value, and the kernel may be off by the flat tolerance
    or three times the fp32 oracle's own error, whichever is larger.  Same knife mask, no other allowance.
    `arraywise` (d_pose, (B,6)): every element of the array is a sum of signed terms over pixel populations of the same
    statistics, and WHICH sample the fp32 oracle's summation order / branch decisions hit hardest is chance: the yardstick is the
    fp32 oracle's WORST element error over the array, not the error at the same element.  (Where that yardstick is large -- 3e-3
    at 256x832, more behind the camera where single near-singular samples carry percents of a sum -- d_pose of the reference's
    function is simply not defined more precisely in fp32; tests/test_parity_tools_cpu.py checks that at ordinary sizes a 1 %
    error still fails through this rung.)"""
    got = np.asarray(got, np.float64)
    own = np.abs(np.asarray(w32, np.float64) - w64)
    if arraywise:
        own = np.full(own.shape, own.max())
    tol = np.maximum((GRAD_TOL + extra) * np.abs(w64).max(), 3.0 * own)
    bad = np.abs(got - w64) > tol
    if knife is not None:
        bad &= ~np.broadcast_to(knife, got.shape)
    assert not bad.any(), "%s: %d elements off by more than max(%g of the array's maximum, 3x the fp32 oracle's own error) vs the fp64 oracle" % (
        what, int(bad.sum()), GRAD_TOL)
    keep = np.ones(got.shape, bool) if knife is None else ~np.broadcast_to(knife, got.shape)
    m64 = max(float(np.abs(w64).max()), 1e-30)
    parity_note("second opinion (fp64 oracle) used for %s: passed -- kernel max |err| %.2e of the maximum vs the fp64 oracle; the fp32 oracle's own worst %.2e" % (
        what, float((np.abs(got - w64) * keep).max()) / m64, float((np.abs(np.asarray(w32, np.float64) - w64) * keep).max()) / m64))


POSE_PER_FLIP = GRAD_TOL     # what one pixel on the strict in-view test may move d_pose by (of its maximum), at 10^4 pixels per image
POSE_FLIP_CAP = 1e-3         # ... in total, per comparison: the effective element-wise tolerance of d_pose never exceeds 3e-3
POSE_L2_TOL = 1e-3           # relative L2 error of a d_pose array (its six components per sample, all samples) at the 128x416
                             # BASELINE size; 2e-3 for images of more than 10^5 pixels (cfg5, 256x832: four times the signed
                             # terms per sum and the in-view flips that go with them; measured 1.1e-3 .. 1.7e-3 there, and the
                             # fp32 ORACLE itself is 0.4e-3 .. 2.5e-3 away from the fp64 one)


def src_footprints(ref, s, knife):
    """The 2x2 scatter footprints in the source images of the knife-edge target pixels of scale s: (B, 3 n_src, h, w) bool.
    For d_src the pixels ON the kink of |I^ - I| count as well (the oracle's `abs_zero`: in view and I^ == I exactly in some channel --
    saturated or flat regions): sign(0) = 0 there, and an evaluation whose bilinear sample of four equal taps lands one ulp beside
    them scatters +-k instead.  d_disp and d_pose do not see that (equal taps: no gradient with respect to the position), d_src does."""
    uv = ref["uv"][s]                                  # (B,n,2,h,w)
    B, n, _, h, w = uv.shape
    out = np.zeros((B, n, h, w), bool)
    kb = np.broadcast_to(knife.reshape(B, 1, h, w), (B, n, h, w))
    if "abs_zero" in ref:
        kb = kb | np.asarray(ref["abs_zero"][s], bool)
    with np.errstate(invalid="ignore"):
        u0, v0 = np.floor(uv[:, :, 0]), np.floor(uv[:, :, 1])
    ok = kb & np.isfinite(u0) & np.isfinite(v0) & (u0 >= -1) & (u0 <= w - 1) & (v0 >= -1) & (v0 <= h - 1)
    bi, ni, _, _ = np.nonzero(ok)
    uu, vv = u0[ok].astype(np.int64), v0[ok].astype(np.int64)
    for dv in (0, 1):
        for du in (0, 1):
            y, x = vv + dv, uu + du
            m = (y >= 0) & (y < h) & (x >= 0) & (x < w)
            out[bi[m], ni[m], y[m], x[m]] = True
    return np.repeat(out, 3, axis=1)


def pose_explained_by_discontinuities(d, cfg, ref, i, got, norm_B=None, cell_thr=1e-4, max_px=48, max_jumps=2, hint=None):
    """Third opinion for d_pose[i] (B,6): is the kernel's value the ORACLE's with a few named pixels on the other side of a
    discontinuity they sit on?  For every sample whose d_pose row is off by more than a quarter of the gradient tolerance, the
    fp32 oracle is re-run on that sample and source alone (same normalisation: norm_batch) with ONE knife-edge pixel's disparity
    nudged by +-1e-3 / +-1e-2 of its value (or its target texel by +-1e-4: the kink of |I^ - I|); a nudge that makes d_pose JUMP
    (by more than 1e-4 of its maximum; the smooth response to such a nudge is <= 1e-2 of one pixel's share, 1e-5) is that pixel
    taking its other branch.  The knife-edge pixels of the sample are probed one at a time, the most decisive first (see below),
    at most `max_px` of them; a pixel's jump is taken only when it removes at least 30 % of what is left of the difference, AT
    MOST `max_jumps` per sample (with dozens of free 6-vectors a genuine error could be fitted away: round-3 advisor finding),
    and the search stops as soon as the rest is below the trigger.  Returns the oracle's array with the taken jumps added and the
    list of pixels; the caller judges the kernel against it with the flat criteria.
    `hint`: optionally the kernel's d_disp arrays -- a pixel that took the other branch shows in d_disp as well (it is excluded from
    THAT comparison by the knife mask), so the candidates are probed in the order of |d_disp - d_disp_oracle| at them.  It only
    orders the probes: what is taken is still a jump of the ORACLE at a pixel the oracle itself has on a discontinuity."""
    want = np.asarray(ref["d_poses"][i], np.float64)
    got = np.asarray(got, np.float64)
    scale = float(np.abs(want).max())
    S = len(d["disps"])
    B = want.shape[0]
    Bn = B if norm_B is None else norm_B
    kw = dict(cfg, smooth_reg=0.0)
    out, named = want.copy(), []
    for b in np.nonzero(np.abs(got - want).max(axis=1) > 0.25 * GRAD_TOL * scale)[0]:
        sl = slice(int(b), int(b) + 1)
        base_in = dict(tgt_pyr=[a[sl] for a in d["tgt_pyr"]], src_pyr=[a[sl, 3 * i:3 * i + 3] for a in d["src_pyr"]], intrinsics=d["intrinsics"][sl],
                       poses=[d["poses"][i][sl]], masks=[a[sl, i:i + 1] for a in d["masks"]] if (d["masks"] is not None and cfg.get("exp_reg")) else None)

        def pose_grad(disps, tgt=None):
            r = O.sfm_loss(base_in["tgt_pyr"] if tgt is None else tgt, base_in["src_pyr"], base_in["intrinsics"], disps, base_in["poses"],
                           base_in["masks"], backward=True, norm_batch=Bn, **kw)
            return np.asarray(r["d_poses"][0][0], np.float64)

        disps0 = [a[sl].copy() for a in d["disps"]]
        base = pose_grad(disps0)
        assert np.abs(base - want[b]).max() <= 1e-5 * scale, "the one-sample oracle run does not reproduce the batch's d_pose"
        cands = []
        for s in range(S):
            m = ((ref["margin"][s][b, i] < 8e-6) | (ref["cell_margin"][s][b, i] < cell_thr) | (ref["abs_margin"][s][b, i] < 3e-5)
                 | (ref["clip_margin"][s][b, i] < 5e-5))
            cands += [(s, int(y), int(x)) for y, x in np.argwhere(m)]
        # Probed ONE BY ONE, the most decisive first: pixels on the strict in-view test (the whole term appears / disappears), then
        # by how uncertain the sampling position is (near-singular samples, |z| small, carry the largest terms of the sums and the
        # least decided branch); at most `max_px` probes, and the search stops as soon as the residual is explained.
        unc = {}
        for s in range(S):
            dU, dV = position_tolerance(d, s)
            unc[s] = np.maximum(dU[b, i], dV[b, i])
        cands.sort(key=lambda c: (not ref["margin"][c[0]][b, i, c[1], c[2]] < 8e-6, -float(unc[c[0]][c[1], c[2]])))
        if hint is not None:
            cands.sort(key=lambda c: -abs(float(hint[c[0]][b, 0, c[1], c[2]]) - float(ref["d_disps"][c[0]][b, 0, c[1], c[2]])))
        n_cands, cands = len(cands), cands[:max_px]

        def probe(s, y, x):
            jumps = []

            def note(dlt):
                if np.abs(dlt).max() > 1e-4 * scale and not any(np.abs(dlt - q).max() < 1e-5 * scale for q in jumps):
                    jumps.append(dlt)

            for rel in (1e-3, -1e-3, 1e-2, -1e-2):
                disps = [a.copy() for a in disps0]
                disps[s][0, 0, y, x] *= np.float32(1 + rel)
                note(pose_grad(disps) - base)
            # the kink of |I^ - I| is crossed most directly from the target's side: the pixel's three channels moved by +-1e-4
            # (more than the 3e-5 within which the knife mask puts a pixel on the kink, 1e-4 of the image range)
            for dt in (1e-4, -1e-4):
                tgt = [a.copy() for a in base_in["tgt_pyr"]]
                tgt[s][0, :, y, x] += np.float32(dt)
                dlt = pose_grad(disps0, tgt) - base
                note(dlt)
                # ... and the kink has a value of its own: F.absolute's backward is sign(0) = 0 where one evaluation finds
                # I^ - I == 0 exactly -- half way between the two signs
                if ref["abs_margin"][s][b, i, y, x] < 3e-5:
                    note(0.5 * dlt)
            return jumps

        res, used = got[b] - want[b], 0
        for (s, y, x) in cands:
            if used >= max_jumps or np.abs(res).max() <= 0.25 * GRAD_TOL * scale:
                break
            jumps = probe(s, y, x)
            if os.environ.get("SFM_EXPLAIN_DEBUG"):
                print("explain sample %d: residual/scale %s; probe %s: %d jumps" % (b, res / scale, (s, y, x), len(jumps)))
            if not jumps:
                continue
            best = min(jumps, key=lambda dlt: np.linalg.norm(res - dlt))
            if np.linalg.norm(res - best) > 0.7 * np.linalg.norm(res):      # a named pixel must carry a real share of the difference
                continue
            used += 1
            res = res - best
            out[b] += best
            named.append("sample %d scale %d pixel (%d,%d)" % (b, s, y, x))
        if os.environ.get("SFM_EXPLAIN_DEBUG"):
            print("explain sample %d: %d candidates, %d probed at most, named %s" % (b, n_cands, len(cands), named))
    return out, named


def _check_grads(fl, ref, n_src, check_src=False, check_mask=False, check_pose=True, what="", ref64=None, cell_thr=1e-4, explain=None,
                 abs_thr=3e-5):
    """`ref64`: optional callable returning the fp64 oracle's result; consulted only for an array that misses the fp32
    criterion (see _judged64), and every such use is reported.  `cell_thr`, `abs_thr`: see _knife (`cell_thr` may be a callable
    scale -> width, e.g. cell_width_from_position_bound).  `explain`: optional callable
    (i, got) -> pose_explained_by_discontinuities(...), consulted for a d_pose array that misses everything else."""
    worst = 0.0
    r64 = []

    def second(key, idx):
        if not r64:
            r64.append(ref64())
        return r64[0][key][idx]

    def measured(got, w, knife):
        """(largest element-wise error outside the knife mask, of the array's largest magnitude; relative L2 outside the mask)"""
        g64, w64_ = np.asarray(got, np.float64), np.asarray(w, np.float64)
        keep = np.ones(g64.shape, bool) if knife is None else ~np.broadcast_to(knife, g64.shape)
        return float((np.abs(g64 - w64_) * keep).max() / max(np.abs(w64_).max(), 1e-30)), rel_l2(got, w, knife)

    def close(got, w, knife, name, key, idx, extra=0.0):
        """-> the rung that decided the element-wise comparison"""
        try:
            try:
                assert_close_masked(got, w, GRAD_TOL, knife, what=name)
                return "flat"
            except AssertionError:
                if not extra:
                    raise
                assert_close_masked(got, w, GRAD_TOL + extra, knife, what=name)
                parity_note("in-view allowance USED for %s %s: misses the flat %.0e, passes at %.2e" % (what, name, GRAD_TOL, GRAD_TOL + extra))
                return "in-view allowance"
        except AssertionError:
            if ref64 is None:
                raise
            _judged64(got, w, second(key, idx), knife, "%s %s" % (what, name), extra=extra, arraywise=(key == "d_poses"))
            return "fp64 second opinion"

    def l2_ok(got, w, knife, name, key, idx, tol=L2_TOL):
        """-> (relative L2 that was judged, the rung that decided)"""
        l2 = rel_l2(got, w, knife)
        if l2 > tol:
            # one ill-conditioned element can carry the whole norm: the fp64 oracle decides, with the fp32 oracle's own error as the yardstick
            assert ref64 is not None, "%s: relative L2 error %.2e outside knife pixels" % (name, l2)
            w64 = second(key, idx)
            mine, theirs = rel_l2(got, w64, knife), rel_l2(w, w64, knife)
            assert mine <= max(tol, 3.0 * theirs), "%s: relative L2 error %.2e vs the fp64 oracle (the fp32 oracle's own: %.2e)" % (name, mine, theirs)
            parity_note("second opinion (fp64 oracle) used for the L2 norm of %s %s: %.2e vs the fp32 oracle's own %.2e" % (what, name, mine, theirs))
            return min(l2, mine), "fp64 second opinion"
        return l2, "flat"

    def record(name, got, w, knife, rung_e, rung_l2, tol_e, tol_l2, knife_share=None, key=None, idx=None):
        e, l2 = measured(got, w, knife)
        row = dict(case=what, array=name, elementwise_rung=rung_e, elementwise_err=e, elementwise_tol=tol_e, l2_rung=rung_l2, l2_err=l2, l2_tol=tol_l2,
                   knife_share=knife_share)
        if "fp64" in rung_e or "fp64" in rung_l2:      # what the fp64 oracle says: the kernel's distance to it and the fp32 oracle's own
            w64 = second(key, idx)
            e64, l64 = measured(got, w64, knife)
            own_e, own_l = measured(w, w64, knife)
            row.update(err_vs_fp64=e64, l2_vs_fp64=l64, oracle32_own_err=own_e, oracle32_own_l2=own_l)
        parity_row(**row)

    cell_of = cell_thr if callable(cell_thr) else (lambda s_: cell_thr)     # per scale: a width in px, or an array (B,n,h,w) of widths
    abs_of = abs_thr if callable(abs_thr) else (lambda s_: abs_thr)
    observed = None      # per sample: knife-edge pixels where the kernel demonstrably took the other branch (a count; REPORTED only)
    on_test = None       # per sample: pixels the ORACLE places within `thr` of the strict in-view test (what the allowance goes by)
    knives = []
    for s, (g, w) in enumerate(zip(fl.d_disps, ref["d_disps"])):
        knife = _knife(ref, s, n_src, what=what, cell_thr=cell_of(s), abs_thr=abs_of(s))
        knives.append(knife)
        gnp = to_np(g)
        # (a quarter of the gradient tolerance already counts as "took the other branch": rounding noise is 1000x smaller)
        off = (np.abs(gnp.astype(np.float64) - w) > 0.25 * GRAD_TOL * np.abs(w).max()) & np.broadcast_to(knife, w.shape)
        cnt = off.reshape(off.shape[0], -1).sum(axis=1)
        observed = cnt if observed is None else observed + cnt
        flip = knife_mask(ref, s, cell_thr=cell_of(s), abs_thr=abs_of(s))[1]   # (B,h,w): from the oracle's own margins only
        fc = flip.reshape(flip.shape[0], -1).sum(axis=1)
        on_test = fc if on_test is None else on_test + fc
        rung_e = close(gnp, w, knife, "d_disp[%d]" % s, "d_disps", s)
        l2, rung_l2 = l2_ok(gnp, w, knife, "d_disp[%d]" % s, "d_disps", s)
        worst = max(worst, l2)
        record("d_disp[%d]" % s, gnp, w, knife, rung_e, rung_l2, GRAD_TOL, L2_TOL, float(knife.mean()), key="d_disps", idx=s)
        if check_mask:
            # d_mask (B,n,h,w) is a per-pixel, per-source quantity (the explainability branch has no SSIM window, base_model.py:103-109):
            # its gradient k_pix e1 s (1-s) carries e1 = sum_c |I^ - I| of THAT pixel, which is the whole term or 0 according to the strict
            # in-view test -- so a pixel the ORACLE has within FLIP_THR of that test is excluded, that pixel of that source only (no
            # footprint), counted.  (Rounds 1-3 compared d_mask without any exclusion; 1000 sweep cases never put a flip on an
            # explainability case, the 400-case soak of round 4 did: 1 element of 575 280, oracle margin 2.4e-7, the oracle's warped
            # pixel exactly 0 and the kernel's sampled -- tools/diag_sweep_mask.py.)
            mflip = ref["margin"][s] < FLIP_THR                                   # (B,n,h,w)
            if mflip.any():
                parity_note("knife %s d_mask[%d]: %d of %d elements on the strict in-view test excluded" % (what, s, int(mflip.sum()), mflip.size))
            assert mflip.mean() <= knife_cap(mflip.shape[-2] * mflip.shape[-1])
            rung_e = close(to_np(fl.d_masks[s]), ref["d_masks"][s], mflip, "d_mask[%d]" % s, "d_masks", s)
            _, rung_l2 = l2_ok(to_np(fl.d_masks[s]), ref["d_masks"][s], mflip, "d_mask[%d]" % s, "d_masks", s)
            record("d_mask[%d]" % s, to_np(fl.d_masks[s]), ref["d_masks"][s], mflip, rung_e, rung_l2, GRAD_TOL, L2_TOL, key="d_masks", idx=s)
    # d_pose of a sample sums SIGNED terms of all its pixels and scales: a pixel on the strict in-view test that the two fp32
    # evaluations place on different sides changes one term by its full size, which can be many times the net sum's share of a
    # pixel (measured: one such pixel of a 92x108 image moved d_pose by 0.26 % of its maximum).  The allowance goes by how many
    # pixels the ORACLE puts within `thr` of that test (nothing the kernel computes enters it): one gradient tolerance per such
    # pixel at 10^4 pixels per image and proportionally less above, POSE_FLIP_CAP in total.  The observed count is printed.
    # An array that still misses a criterion can be EXPLAINED where the oracle is cheap to re-run (`explain`, see
    # pose_explained_by_discontinuities): the oracle is re-evaluated with single named pixels pushed across the discontinuity
    # they sit on, and the kernel must then meet the flat criteria, without any allowance, against that evaluation.
    n_on_test = 0 if on_test is None else int(on_test.max())
    n_observed = 0 if observed is None else int(observed.max())
    px0 = float(fl.d_disps[0].shape[-2] * fl.d_disps[0].shape[-1])      # a pixel's weight in the sums falls with the image size
    extra = min(POSE_FLIP_CAP, POSE_PER_FLIP * min(1.0, 1.0e4 / px0) * n_on_test)
    worst_pose = 0.0
    pose_l2_tol = POSE_L2_TOL if px0 <= 1.0e5 else 2.0 * POSE_L2_TOL
    for i, (g, w) in enumerate(zip(fl.d_poses, ref["d_poses"]) if check_pose else ()):
        try:
            rung_e = close(to_np(g), w, None, "d_pose[%d]" % i, "d_poses", i, extra=extra)
            l2, rung_l2 = l2_ok(to_np(g), w, None, "d_pose[%d]" % i, "d_poses", i, tol=pose_l2_tol)
            worst_pose = max(worst_pose, l2)
            record("d_pose[%d]" % i, to_np(g), w, None, rung_e, rung_l2, GRAD_TOL + (extra if rung_e != "flat" else 0.0), pose_l2_tol, key="d_poses", idx=i)
        except AssertionError as first:
            if explain is None:
                raise
            w2, named = explain(i, to_np(g))
            if w2 is None or not named:
                raise AssertionError("%s\n(not explained by knife-edge pixels: %s)" % (first, named))
            # against the oracle with the named pixels on their other branch: the flat criteria, no allowance
            assert_close_masked(to_np(g), w2, GRAD_TOL, None, what="d_pose[%d] vs the oracle with %s on the other branch" % (i, named))
            l2 = rel_l2(to_np(g), w2)
            assert l2 <= pose_l2_tol, "d_pose[%d]: relative L2 %.2e vs the oracle with %s on the other branch" % (i, l2, named)
            worst_pose = max(worst_pose, l2)
            record("d_pose[%d]" % i, to_np(g), w, None, "explained by named pixels", "explained by named pixels", GRAD_TOL, pose_l2_tol)
            parity_note("d_pose EXPLAINED for %s d_pose[%d]: misses the criteria against the oracle as is (%s); equals the oracle with %s "
                        "pushed across the discontinuity it sits on (relative L2 %.2e, flat %.0e met)" % (
                            what, i, str(first).split("\n")[0][:120], ", ".join(named), l2, GRAD_TOL))
    parity_note("grads %s: worst relative L2 of d_disp outside knife pixels %.2e (tol %.0e), of d_pose %.2e (tol %.0e); d_pose "
                "element-wise allowance %.2e for %d pixels the oracle has on the in-view test (%d observed as taken differently)" % (
                    what, worst, L2_TOL, worst_pose, pose_l2_tol, extra, n_on_test, n_observed))
    if check_src:
        for s, (g, w) in enumerate(zip(fl.d_srcs, ref["d_srcs"])):
            # element-wise everywhere except on the 2x2 scatter footprints of the knife-edge target pixels; a second opinion from the
            # fp64 oracle, where one is offered, for an array that misses that (the sign of I^ - I and the cell of a sample are
            # decided by the last bits of a position in BOTH fp32 evaluations: tools/diag_sweep_dsrc.py)
            fp = src_footprints(ref, s, knives[s])
            try:
                assert_close_masked(to_np(g), w, GRAD_TOL, fp, what="d_src[%d]" % s)
            except AssertionError:
                if ref64 is None:
                    raise
                _judged64(to_np(g), w, second("d_srcs", s), fp, "%s d_src[%d]" % (what, s))


CONFIGS = {
    "l1": dict(),
    "l1_smooth": dict(smooth_reg=0.1),
    "ssim_smooth": dict(smooth_reg=0.1, ssim_rate=0.15),
    "ssim_only": dict(ssim_rate=0.15),
    "edge_aware": dict(smooth_reg=0.1, ssim_rate=0.15, smooth_mode="edge_aware"),
    "edge_aware_l1": dict(smooth_reg=0.3, smooth_mode="edge_aware"),
    "explain": dict(smooth_reg=0.1, exp_reg=0.2),
    "explain_alpha": dict(smooth_reg=0.1, exp_reg=0.2, ssim_rate=0.15),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("shape", [(2, 32, 48, 2, 3), (1, 37, 70, 2, 1), (2, 20, 130, 4, 2)])
def test_fused_loss_matches_oracle(ops, synth, dev, name, shape):
    B, H, W, n_src, n_scales = shape
    cfg = CONFIGS[name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=11, with_masks=True)
    ref = _oracle(d, cfg, want_d_src=True)
    fl = _bind(ops, dev, d, cfg, want_d_src=True)
    _check_losses(fl.forward(), ref)
    fl.backward(1.0)
    _check_grads(fl, ref, n_src, check_src=True, check_mask=bool(cfg.get("exp_reg")))
    # the fused launch returns the same loss and the same gradients
    g_sep = [to_np(t).copy() for t in fl.d_disps] + [to_np(t).copy() for t in fl.d_poses]
    _check_losses(fl.forward_backward(), ref)
    g_fused = [to_np(t) for t in fl.d_disps] + [to_np(t) for t in fl.d_poses]
    for a, b in zip(g_sep, g_fused):   # two instantiations of one template: same math, ulp-level differences
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * np.abs(a).max())


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("shape", [(2, 32, 48, 2, 3), (1, 37, 70, 2, 1), (3, 20, 130, 4, 2)])
def test_hwc_layout_gives_the_planar_results(ops, synth, dev, name, shape):
    """SFM_LAYOUT_HWC only changes how the images are fetched: every entry point returns what it returns for the
    reference's planar layout -- the loss bit for bit, the gradients to the last ulps (another instantiation of the
    same template) -- and the oracle parity of the planar path carries over."""
    B, H, W, n_src, n_scales = shape
    cfg = CONFIGS[name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=13, with_masks=True)
    ref = _oracle(d, cfg, want_d_src=True)
    a = _bind(ops, dev, d, cfg, want_d_src=True)
    b = _bind(ops, dev, d, cfg, want_d_src=True, layout="hwc")
    for run in ("separate", "fused"):
        if run == "separate":
            la, lb = to_np(a.forward()).copy(), to_np(b.forward()).copy()
            a.backward(1.0); b.backward(1.0)
        else:
            la, lb = to_np(a.forward_backward()).copy(), to_np(b.forward_backward()).copy()
        np.testing.assert_allclose(lb, la, rtol=2e-7, atol=0)
        groups = [(a.d_disps, b.d_disps), (a.d_poses, b.d_poses), (a.d_srcs, b.d_srcs)]
        if cfg.get("exp_reg"):
            groups.append((a.d_masks, b.d_masks))
        for ga, gb in groups:
            for x, y in zip(ga, gb):
                x, y = to_np(x), to_np(y)
                assert x.shape == y.shape
                np.testing.assert_allclose(y, x, rtol=0, atol=2e-5 * max(np.abs(x).max(), 1e-30))
    _check_losses(b.loss5, ref)
    _check_grads(b, ref, n_src, check_src=True, check_mask=bool(cfg.get("exp_reg")))


def test_upstream_gradient_scales_linearly(ops, synth, dev):
    cfg = CONFIGS["ssim_smooth"]
    d = synth.make_inputs(B=2, H=32, W=48, n_src=2, n_scales=2, seed=5)
    fl = _bind(ops, dev, d, cfg)
    fl.backward(1.0)
    g1 = [to_np(t).copy() for t in fl.d_disps + fl.d_poses]
    fl.backward(-2.5)
    g2 = [to_np(t) for t in fl.d_disps + fl.d_poses]
    for a, b in zip(g1, g2):
        np.testing.assert_allclose(b, -2.5 * a, rtol=0, atol=2e-5 * np.abs(a).max())


def test_batch_shard_is_additive(ops, synth, dev):
    """norm_B = global batch: the shard losses add up to the full-batch loss and the
    per-sample gradients are those of the full batch."""
    cfg = CONFIGS["ssim_smooth"]
    d = synth.make_inputs(B=4, H=32, W=48, n_src=2, n_scales=2, seed=9)
    full = _bind(ops, dev, d, cfg)
    lf = to_np(full.forward_backward()).astype(np.float64)
    tot = np.zeros(5)
    for lo in (0, 2):
        sl = slice(lo, lo + 2)
        part = dict(d, tgt_pyr=[a[sl] for a in d["tgt_pyr"]], src_pyr=[a[sl] for a in d["src_pyr"]],
                    intrinsics=d["intrinsics"][sl], disps=[a[sl] for a in d["disps"]],
                    poses=[a[sl] for a in d["poses"]])
        sh = _bind(ops, dev, part, cfg, norm_B=4)
        tot += to_np(sh.forward_backward()).astype(np.float64)
        for s in range(2):
            np.testing.assert_allclose(to_np(sh.d_disps[s]), to_np(full.d_disps[s])[sl], rtol=1e-5, atol=1e-10)
        for i in range(2):
            np.testing.assert_allclose(to_np(sh.d_poses[i]), to_np(full.d_poses[i])[sl], rtol=1e-5, atol=1e-10)
    np.testing.assert_allclose(tot, lf, rtol=1e-5)


def count_in_view_mismatches(ops, dev, d, ref, layout, what):
    """How many pixels the fused kernel zeroes differently from the oracle -- counted, not inferred.  With the L1 term alone and
    ONE source, d_disp of a pixel is exactly 0 iff its sample is not in view (or its photometric gradient vanishes by itself), so
    the zero set of a single-source L1-only launch IS the kernel's out-of-view set of that source; the oracle's is the mask of
    models/base_model.py:96 on its warped image.  Returns / prints per source and scale (kernel out & oracle in, kernel in & oracle out)."""
    n_src = len(d["poses"])
    total = [0, 0]
    per_scale = [0] * len(d["disps"])
    for i in range(n_src):
        one = dict(d, src_pyr=[a[:, 3 * i:3 * i + 3] for a in d["src_pyr"]], poses=[d["poses"][i]], masks=None)
        fl = _bind(ops, dev, one, dict(), layout=layout)
        fl.forward_backward()
        # the oracle on the same single-source L1-only problem: its zero set holds the same flat-region zeros (clipped
        # texture: dI^/du = dI^/dv = 0 in view), so the DIFFERENCE of the two sets is the pixels zeroed differently
        o1 = O.sfm_loss(one["tgt_pyr"], one["src_pyr"], one["intrinsics"], one["disps"], one["poses"], None, backward=True)
        for s, g in enumerate(fl.d_disps):
            k_out = to_np(g)[:, 0] == 0
            o_out = o1["d_disps"][s][:, 0] == 0
            a, b = int((k_out & ~o_out).sum()), int((~k_out & o_out).sum())
            near = int((k_out != o_out)[ref["margin"][s][:, i] < 8e-6].sum())
            total[0] += a
            total[1] += b
            per_scale[s] += a + b
            if a or b:
                parity_note("in-view sets %s src %d scale %d: kernel out / oracle in %d, kernel in / oracle out %d of %d px (%d of them within 8e-6 of the strict test)" % (
                    what, i, s, a, b, k_out.size, near))
    parity_note("in-view sets %s: %d + %d pixels zeroed differently from the oracle over %d sources x %d scales" % (
        what, total[0], total[1], n_src, len(d["disps"])))
    count_in_view_mismatches.per_scale = per_scale
    return total


@pytest.mark.parametrize("cfg_name,B,H,W,n_src,n_scales", [
    ("l1", 1, 128, 416, 2, 1),             # BASELINE cfg1: the CPU reference's own case (1 snippet, 1 scale, L1 only), on the HIP path
    ("l1_smooth", 8, 128, 416, 2, 4),      # BASELINE cfg2 at full size
    ("ssim_smooth", 4, 128, 416, 2, 4),    # cfg3's live loss mode (2nd-order smoothness), full resolution, oracle-sized batch
    ("edge_aware", 4, 128, 416, 2, 4),     # BASELINE cfg3 AS WRITTEN: L1 + SSIM + EDGE-AWARE smoothness (base_model.py:144-155)
])
@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_baseline_configs_vs_oracle(ops, synth, dev, cfg_name, B, H, W, n_src, n_scales, layout):
    """BASELINE.json configs at full 128x416 resolution against the oracle, at batches the oracle finishes in seconds."""
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=1)
    ref = _oracle(d, cfg)
    fl = _bind(ops, dev, d, cfg, layout=layout, want_warped=True)
    what = "%s B=%d %dx%d %s" % (cfg_name, B, H, W, layout)
    _check_losses(fl.forward(), ref)
    _check_warped(fl, ref, what + " [sfm_loss_fwd]", d)
    w_fwd = [to_np(t).copy() for t in fl.warped]
    for t in fl.warped:
        t.fill_(7.0)
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, what + " [sfm_loss_fwd_bwd]", d)
    for a, t in zip(w_fwd, fl.warped):      # the two entry points warp with the same statements
        np.testing.assert_array_equal(a, to_np(t))
    _check_grads(fl, ref, n_src, what=what)
    a, b = count_in_view_mismatches(ops, dev, d, ref, layout, what)
    # every pixel the two evaluations treat differently sits on the strict test (the knife mask covers it): a handful per image
    assert a + b <= 4 * B * n_src * n_scales, (a, b)


@pytest.mark.parametrize("cfg_name,B,H,W,n_src", [
    ("ssim_smooth", 32, 128, 416, 2),     # BASELINE cfg3 / cfg4's per-GPU share at the FULL batch, live smoothness form
    ("edge_aware", 32, 128, 416, 2),      # BASELINE cfg3 as written (edge-aware smoothness), full batch
    ("ssim_smooth", 8, 256, 832, 4),      # BASELINE cfg5 at its full batch, 5-frame snippet = 4 sources
])
def test_full_batch_vs_oracle(ops, synth, dev, cfg_name, B, H, W, n_src):
    """BASELINE cfg3 (both smoothness forms) and cfg5 at their FULL batch against the fp32 oracle (a minute of NumPy each), in the
    pixel-interleaved layout bench.py measures: the five scalars to 1e-4, every gradient by the criteria of _check_grads."""
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=4, seed=1)
    ref = _oracle(d, cfg)
    fl = _bind(ops, dev, d, cfg, layout="hwc", want_warped=True)
    _check_losses(fl.forward_backward(), ref)
    what = "FULL BATCH %s B=%d %dx%d %d src hwc" % (cfg_name, B, H, W, n_src)
    _check_warped(fl, ref, what + " [sfm_loss_fwd_bwd]", d)
    # the launch without the warped output (another instantiation of the same template: what bench.py times) gives the same loss and gradients
    plain = _bind(ops, dev, d, cfg, layout="hwc")
    np.testing.assert_array_equal(to_np(plain.forward_backward()), to_np(fl.loss5))
    for a, b in zip(plain.d_disps + plain.d_poses, fl.d_disps + fl.d_poses):
        np.testing.assert_array_equal(to_np(a), to_np(b))
    # (the fp64 oracle is only evaluated if an array misses the fp32 criterion -- an ill-conditioned far point among 1.7 million
    # pixels -- and every such use is printed)
    ref64 = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True,
                               dtype=np.float64, **cfg)
    # cell_thr: among 1.7 million samples one lands 1.2e-4 px from a lattice line (sample 0, scale 0, (11, 397), U = 361.9999) and
    # is placed in the neighbouring cell by the kernel (dI^/du jumps there); the cell-boundary class is as wide as the fp32
    # uncertainty of each sample's position (oracle/parity.py: 1 .. 2e-4 px here), not a hand-set constant
    _check_grads(fl, ref, n_src, what=what, ref64=ref64, **knife_widths(d, ref))
    count_in_view_mismatches(ops, dev, d, ref, "hwc", what)


@pytest.mark.parametrize("cfg_name,B,H,W,n_src,n_scales", [
    ("l1", 1, 128, 416, 2, 1),             # BASELINE cfg1
    ("l1_smooth", 8, 128, 416, 2, 4),      # BASELINE cfg2
    ("ssim_smooth", 4, 128, 416, 2, 4),    # cfg3, live smoothness, oracle-sized batch
    ("edge_aware", 4, 128, 416, 2, 4),     # cfg3 as written
    ("edge_aware", 32, 128, 416, 2, 4),    # cfg3 as written at its FULL batch: the launch bench.py's headline times
])
def test_warped_pixels_meet_the_flat_tolerance_on_seam_free_inputs(ops, synth, dev, cfg_name, B, H, W, n_src, n_scales):
    """north_star: "within 1e-4 rel fp32 on loss AND WARPED PIXELS" -- as a statement without an allowance.  Inputs: SURVEY 8(d)'s
    "src = tgt pattern SHIFTED by a few px" with the border replicated (synth.make_inputs(seam="shift")) instead of rolled around:
    no artificial step edge.  Every warped pixel of the benchmarked kernel (sfm_loss_fwd_bwd, pixel-interleaved) within the FLAT
    1e-4 of the image range of the oracle's curr_proj_img (models/base_model.py:90-94), except pixels zeroed differently, all of
    which the oracle places within 8e-6 of the strict in-view test (transform.py:129)."""
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=1, seam="shift")
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=False, keep_warped=True, **cfg)
    fl = _bind(ops, dev, d, cfg, layout="hwc", want_warped=True)
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, "SEAM-FREE %s B=%d %dx%d hwc" % (cfg_name, B, H, W), d, flat=True)


@pytest.mark.parametrize("cfg_name,B,H,W", [
    ("edge_aware", 4, 128, 416),     # BASELINE cfg3 as written, oracle-sized batch
    ("ssim_smooth", 2, 256, 832),    # the 256x832 frame of cfg5 (2 sources)
])
def test_smooth_disparity_field_vs_oracle(ops, synth, dev, cfg_name, B, H, W):
    """The inputs of bench.py's `*_smooth_disp` keys (synth.make_inputs(disp_div=32, disp_noise=0): a disparity field as smooth as a
    network's away from object boundaries; neighbouring samples' taps stay in neighbouring texels, which is where the gather runs
    8-15 % faster, profiles/r05_process_modes.txt 3.) against the oracle: the five scalars, the warped pixels and every gradient by the
    criteria of the default (rough) field -- a coherent warp is a different regime of the same kernel (in-view sets with long straight
    borders, cell boundaries crossed by whole runs of lanes at once), not an easier one."""
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=2, n_scales=4, seed=1, disp_div=32, disp_noise=0.0)
    ref = _oracle(d, cfg)
    fl = _bind(ops, dev, d, cfg, layout="hwc", want_warped=True)
    what = "SMOOTH DISPARITY %s B=%d %dx%d hwc" % (cfg_name, B, H, W)
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, what + " [sfm_loss_fwd_bwd]", d)
    ref64 = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True,
                               dtype=np.float64, **cfg)
    _check_grads(fl, ref, 2, what=what, ref64=ref64, **knife_widths(d, ref))
    count_in_view_mismatches(ops, dev, d, ref, "hwc", what)


@pytest.mark.parametrize("cfg_name", ["l1", "l1_smooth", "ssim_smooth", "edge_aware", "explain"])
def test_header_read_from_the_struct_gives_the_same_bits(ops, synth, dev, cfg_name):
    """The kernels take the header of their argument block (batch, counts, tile counts packed into 16-bit halves) as preloaded scalar
    arguments; a batch or a tile count beyond 16 bits makes them read it from the struct instead.  No shape a test can afford reaches
    that path, so sfm_loss_variant(3) forces it: all three entry points, every output bit for bit the default launch's."""
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=3, H=48, W=136, n_src=2, n_scales=3, seed=17, with_masks=True)
    outs = []
    for forced in (False, True):
        fl = _bind(ops, dev, d, cfg, layout="hwc")
        hook = (lambda: ops.check(ops.lib.sfm_loss_variant(3))) if forced else (lambda: None)
        hook()
        l_fwd = to_np(fl.forward()).copy()
        hook()
        l_both = to_np(fl.forward_backward()).copy()
        g_both = [to_np(t).copy() for t in fl.d_disps + fl.d_poses + (fl.d_masks or [])]
        hook()
        fl.backward(1.0)
        g_bwd = [to_np(t).copy() for t in fl.d_disps + fl.d_poses + (fl.d_masks or [])]
        outs.append((l_fwd, l_both, g_both, g_bwd))
    (a_fwd, a_both, a_g, a_b), (b_fwd, b_both, b_g, b_b) = outs
    np.testing.assert_array_equal(a_fwd, b_fwd)
    np.testing.assert_array_equal(a_both, b_both)
    for x, y in zip(a_g + a_b, b_g + b_b):
        np.testing.assert_array_equal(x, y)


def test_warped_pixels_at_256x832_on_seam_free_inputs(ops, synth, dev):
    """BASELINE cfg5 (B=8, 256x832, 4 sources) on seam-free inputs.  At U ~ 800 one ulp of a sampling position is 6e-5 px and two
    correct fp32 evaluations of it lie up to 3e-4 px apart: the product kernel is held to a flat 2e-4 of the range with at most
    0.01 % of the pixels above 1e-4, next to the yardstick -- how far the fp32 ORACLE is from the fp64 one on the same inputs -- and
    the same launch with projection="reference_order" (SFM_PROJECTION_REFERENCE_ORDER: the oracle's own rounding sequence per pixel,
    a mode a caller selects in the descriptor since ABI v5) to the FLAT 1e-4 with NO pixel above it, and its gradients by the usual
    criteria.  (The mode follows the oracle's roundings up to sin / cos of the pose angles -- NumPy's float32 sin / cos differ
    between CPUs -- so one source in a few has a projection that differs in the last bits; tools/diag_ref_pose.py: at this size that is
    source 2, where the fp32 ORACLE is 3.4e-3 of the maximum from the fp64 one on d_pose of one sample and this mode 2e-4.  The fp64
    second opinion is therefore offered here too; which rung decided is recorded.)"""
    cfg = CONFIGS["ssim_smooth"]
    B, H, W, n_src = 8, 256, 832, 4
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=4, seed=1, seam="shift")
    kw = dict(backward=False, keep_warped=True, **cfg)
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, **kw)
    ref64 = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, dtype=np.float64, **kw)
    own = sum(int(((np.abs(a - b).max(axis=2) > WARP_TOL) & ((a == 0).all(axis=2) == (b == 0).all(axis=2))).sum()) for a, b in zip(ref["warped"], ref64["warped"]))
    n_px = sum(a.shape[0] * a.shape[1] * a.shape[3] * a.shape[4] for a in ref["warped"])
    parity_note("yardstick SEAM-FREE cfg5: the fp32 oracle itself is more than 1e-4 of the range from the fp64 oracle at %d of %d warped pixels" % (own, n_px))
    fl = _bind(ops, dev, d, cfg, layout="hwc", want_warped=True)
    what = "SEAM-FREE ssim_smooth B=%d %dx%d %d src hwc" % (B, H, W, n_src)
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, what, d, flat=True, flat_tol=2e-4, max_over_flat=int(1e-4 * n_px))
    # ... and the kernel against the fp64 oracle (the function itself, no fp32 evaluation's roundings): is the kernel a worse fp32
    # evaluation than the reference's, or do two equally good ones simply lie further apart than either does from the truth?
    k64 = sum(int(((np.abs(to_np(g).astype(np.float64) - b).max(axis=2) > WARP_TOL) & ((to_np(g) == 0).all(axis=2) == (b == 0).all(axis=2))).sum())
              for g, b in zip(fl.warped, ref64["warped"]))
    w64 = max(float(np.abs(to_np(g).astype(np.float64) - b).max(axis=2)[(to_np(g) == 0).all(axis=2) == (b == 0).all(axis=2)].max()) for g, b in zip(fl.warped, ref64["warped"]))
    o64 = max(float(np.abs(a - b).max(axis=2)[(a == 0).all(axis=2) == (b == 0).all(axis=2)].max()) for a, b in zip(ref["warped"], ref64["warped"]))
    parity_note("yardstick SEAM-FREE cfg5: the KERNEL is more than 1e-4 of the range from the fp64 oracle at %d of %d warped pixels (worst %.2e; the fp32 oracle's worst %.2e)" % (
        k64, n_px, w64, o64))
    fr = _bind(ops, dev, d, cfg, layout="hwc", want_warped=True, projection="reference_order")
    _check_losses(fr.forward_backward(), ref)
    _check_warped(fr, ref, what + " [projection = reference_order]", d, flat=True, max_over_flat=0)
    refb = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True, keep_warped=True, **cfg)
    ref64b = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True, dtype=np.float64, **cfg)
    _check_grads(fr, refb, n_src, what=what + " [projection = reference_order]", ref64=ref64b, **knife_widths(d, refb))


@pytest.mark.parametrize("motion", [None, "behind", "large"])
def test_reference_order_projection_meets_the_flat_tolerance_on_rolled_inputs(ops, synth, dev, motion):
    """projection="reference_order" (SfmLossDesc.projection = SFM_PROJECTION_REFERENCE_ORDER) -- the fused kernel with the projection
    in the reference's own evaluation order (transform.py:105-108,122-131,189; nothing fused, quotients as v_rcp + residual
    correction) -- against the oracle on the ROLLED inputs, seam included: every warped pixel within the FLAT 1e-4, no pixel zeroed
    differently away from the strict test, the loss and every gradient by the flat criteria (no fp64 second opinion is offered).
    What separates the FAST projection from the flat criterion on a contrast-2.0 seam is therefore the rounding sequence of the
    sampling position, nothing else (profiles/r06_reference_order.txt has the kernel times)."""
    cfg = CONFIGS["edge_aware"]
    kw = dict(B=4, H=128, W=416, n_src=2, n_scales=4)
    d = synth.make_inputs(seed=1, **kw) if motion is None else make_motion_inputs(synth, motion, seed=21, **kw)
    ref = _oracle(d, cfg)
    what = "REFERENCE-ORDER PROJECTION %s edge_aware B=4 128x416 hwc" % (motion or "default motion")
    fl = _bind(ops, dev, d, cfg, layout="hwc", want_warped=True, projection="reference_order")
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, what, d, flat=True, max_over_flat=0)
    _check_grads(fl, ref, 2, what=what, **knife_widths(d, ref))


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("shape", [(2, 32, 48, 2, 3), (3, 20, 130, 4, 2)])
def test_reference_order_projection_every_mode_entry_point_and_layout(ops, synth, dev, name, shape):
    """SFM_PROJECTION_REFERENCE_ORDER exists for every launch the FAST projection has (all loss modes, the three entry points, both
    image layouts, with and without the warped output) except the ones that also produce d_src: each against the oracle by the
    usual criteria, the warped pixels by the FLAT one, planar = hwc, fused = separate."""
    B, H, W, n_src, n_scales = shape
    cfg = CONFIGS[name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=19, with_masks=True)
    ref = _oracle(d, cfg)
    outs = {}
    for layout in ("planar", "hwc"):
        fl = _bind(ops, dev, d, cfg, layout=layout, want_warped=True, projection="reference_order")
        _check_losses(fl.forward(), ref)
        _check_warped(fl, ref, "REFERENCE-ORDER PROJECTION %s %s [sfm_loss_fwd]" % (name, layout), d, flat=True, max_over_flat=0)
        fl.backward(1.0)
        _check_grads(fl, ref, n_src, check_mask=bool(cfg.get("exp_reg")), what="REFERENCE-ORDER PROJECTION %s %s" % (name, layout))
        g_sep = [to_np(t).copy() for t in fl.d_disps + fl.d_poses + (fl.d_masks or [])]
        l_fused = to_np(fl.forward_backward()).copy()
        _check_losses(l_fused, ref)
        _check_warped(fl, ref, "REFERENCE-ORDER PROJECTION %s %s [sfm_loss_fwd_bwd]" % (name, layout), d, flat=True, max_over_flat=0)
        g_fused = [to_np(t).copy() for t in fl.d_disps + fl.d_poses + (fl.d_masks or [])]
        for a, b in zip(g_sep, g_fused):
            np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * max(np.abs(a).max(), 1e-30))
        plain = _bind(ops, dev, d, cfg, layout=layout, projection="reference_order")      # the launch WITHOUT the warped output: same bits
        np.testing.assert_array_equal(to_np(plain.forward_backward()), l_fused)
        for a, b in zip([to_np(t) for t in plain.d_disps + plain.d_poses], g_fused):
            np.testing.assert_array_equal(a, b)
        outs[layout] = (l_fused, g_fused)
    np.testing.assert_allclose(outs["hwc"][0], outs["planar"][0], rtol=2e-7, atol=0)
    for a, b in zip(outs["planar"][1], outs["hwc"][1]):
        np.testing.assert_allclose(b, a, rtol=0, atol=2e-5 * max(np.abs(a).max(), 1e-30))


def traced_items(ops, fl, launch):
    """Work items the main kernel of ONE launch really ran: sfm_loss_debug_trace makes every wavefront of the next sfm_loss_* call
    write a 32-byte record {start, end, HW_ID, XCC_ID} (start > 0) at its item's index.  The buffer is sized by the header's own
    bound (items <= sfm_loss_workspace_bytes / 64), never by sfm_loss_plan_info -- that is the number under test."""
    import ctypes as C
    import torch
    n_rec = ops.lib.sfm_loss_workspace_bytes(C.byref(fl.desc)) // 64
    assert n_rec > 0
    buf = torch.zeros((n_rec, 4), dtype=torch.int64, device=fl.device)
    torch.cuda.synchronize()
    ops.check(ops.lib.sfm_loss_debug_trace(C.c_void_p(buf.data_ptr())))
    launch()
    torch.cuda.synchronize()
    return int((buf != 0).any(dim=1).sum().item())


def planned_items(ops, fl, grad, loss):
    import ctypes as C
    out = (C.c_int * (1 + 4 * fl.desc.n_scales))()
    ops.check(ops.lib.sfm_loss_plan_info(C.byref(fl.desc), grad, loss, out, len(out)))
    return out[0]


# (B = 8 at 128x416: the smallest reference-sized batch whose one-source chunks are taller than the 4-row minimum, so that the two
#  forms plan different item counts -- below it both cut every scale into 4-row chunks and run as many items)
PAIR_SHAPES = [(2, 32, 48, 2, 3), (3, 20, 130, 4, 2), (4, 128, 416, 2, 4), (1, 37, 70, 6, 1), (8, 128, 416, 2, 4)]


@pytest.mark.parametrize("cfg_name", ["ssim_smooth", "ssim_only", "edge_aware"])
@pytest.mark.parametrize("shape", PAIR_SHAPES)
def test_two_sources_per_pass_gives_the_one_source_results(ops, synth, dev, cfg_name, shape):
    """loss_kernel_pair (sfm_ssim_pair.h, round 6): SSIM gradient launches of an even number of sources can walk TWO sources per pass
    at two waves per SIMD (the library picks that form where it is faster: small batches; profiles/r06_pair_kernel.txt).  Per pixel
    it is the one-source kernels' arithmetic; what differs is the chunking (fewer, taller chunks: another summation order of the
    per-wave partials) and the order in which the sources' shares of d_disp are added.  sfm_loss_variant(5) / (4) select either form
    for one call: same loss to 2e-7, same gradients to 2e-5 of their maximum -- and the pair form against the oracle by the usual
    criteria."""
    B, H, W, n_src, n_scales = shape
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=23)
    ref = _oracle(d, cfg)
    fl = _bind(ops, dev, d, cfg, layout="hwc")
    outs = {}
    for variant in (4, 5):
        loss = to_np(fl.forward_backward(variant=variant)).copy()
        outs[variant] = (loss, [to_np(t).copy() for t in fl.d_disps + fl.d_poses])
        ops.check(ops.lib.sfm_loss_variant(variant))
        fl.backward(1.0)                                        # sfm_loss_bwd has the pair form too
        for a, b in zip(outs[variant][1], [to_np(t) for t in fl.d_disps + fl.d_poses]):
            np.testing.assert_allclose(b, a, rtol=0, atol=2e-5 * max(np.abs(a).max(), 1e-30))
    np.testing.assert_allclose(outs[5][0], outs[4][0], rtol=2e-7, atol=0)
    for a, b in zip(outs[4][1], outs[5][1]):
        np.testing.assert_allclose(b, a, rtol=0, atol=2e-5 * max(np.abs(a).max(), 1e-30))
    what = "TWO SOURCES PER PASS %s B=%d %dx%d %d src" % (cfg_name, B, H, W, n_src)
    _check_losses(fl.forward_backward(variant=5), ref)
    _check_grads(fl, ref, n_src, what=what, **knife_widths(d, ref))
    # the variants are two kernels with two plans: the pair form's chunks are taller, so it runs no more work items than the
    # one-source form (counted on the device) -- strictly fewer unless both are at the 4-row minimum chunk, which is where the count
    # cannot tell them apart (test_two_sources_per_pass_is_the_default_of_some_small_launch needs a shape where it can).  The
    # default launch runs exactly what sfm_loss_plan_info reports, and that is one of the two (which one is choose_variant's choice).
    items = {v: traced_items(ops, fl, lambda: fl.forward_backward(variant=v)) for v in (4, 5)}
    default = traced_items(ops, fl, fl.forward_backward)
    planned = planned_items(ops, fl, 1, 1)
    parity_note("two sources per pass %s B=%d %dx%d %d src: items one-source %d, pair %d, default %d (planned %d)" % (
        cfg_name, B, H, W, n_src, items[4], items[5], default, planned))
    assert 0 < items[5] <= items[4], items
    assert default == planned and default in (items[4], items[5]), (default, planned, items)


@pytest.mark.parametrize("cfg_name", ["ssim_smooth", "ssim_only", "edge_aware"])
def test_two_sources_per_pass_is_the_default_of_some_small_launch(ops, synth, dev, cfg_name):
    """What the pair-form test above cannot see from one shape: over its shapes, at least one default launch (a small batch) IS the
    two-sources-per-pass launch -- the traced item count of the default equals that of sfm_loss_variant(5) and is below that of
    (4), so the hook really switched the kernel.  Which shapes do is left to choose_variant (sfm_loss.hip)."""
    taken = []
    for shape in PAIR_SHAPES:
        B, H, W, n_src, n_scales = shape
        d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=23)
        fl = _bind(ops, dev, d, CONFIGS[cfg_name], layout="hwc")
        items = {v: traced_items(ops, fl, lambda: fl.forward_backward(variant=v)) for v in (4, 5)}
        default = traced_items(ops, fl, fl.forward_backward)
        assert default in (items[4], items[5]), (shape, default, items)
        if default == items[5] < items[4]:
            taken.append(shape)
    parity_note("pair form by default (%s): %s" % (cfg_name, taken))
    assert taken, "no shape of %s takes the two-sources-per-pass form by default" % PAIR_SHAPES


@pytest.mark.parametrize("case", [
    # (config, B, H, W, n_src, n_scales, layout): SSIM + HWC + even sources (two sources per pass without the outputs) at a small
    # and at the reference's batch, and an L1-only small launch (the wide form without the outputs)
    ("ssim_smooth", 2, 32, 48, 2, 3, "hwc"), ("ssim_smooth", 8, 128, 416, 2, 4, "hwc"), ("l1", 2, 32, 48, 2, 3, "planar"),
    ("l1_smooth", 1, 37, 70, 4, 2, "hwc"),
])
@pytest.mark.parametrize("output", ["d_src", "warped"])
def test_plan_info_counts_the_items_of_launches_with_outputs(ops, synth, dev, case, output):
    """sfm_loss_plan_info(desc, grad, loss)[0] is the number of work items the main kernel of that entry point runs for `desc`
    -- also for a descriptor that binds d_src (no pair or wide form: the d_src kernels) or warped (no pair form), which decide
    the kernel as much as the loss configuration does.  Each entry point that uses the output: its traced item count."""
    cfg_name, B, H, W, n_src, n_scales, layout = case
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=29)
    fl = _bind(ops, dev, d, CONFIGS[cfg_name], layout=layout, want_d_src=output == "d_src", want_warped=output == "warped")
    entries = {(1, 1): fl.forward_backward, (1, 0): lambda: fl.backward(1.0)} if output == "d_src" else \
        {(1, 1): fl.forward_backward, (0, 1): fl.forward}
    for (grad, loss), launch in entries.items():
        traced, planned = traced_items(ops, fl, launch), planned_items(ops, fl, grad, loss)
        parity_note("plan_info %s B=%d %dx%d %d src %s with %s, entry (%d,%d): planned %d, traced %d" % (
            cfg_name, B, H, W, n_src, layout, output, grad, loss, planned, traced))
        assert traced > 0 and planned == traced, (grad, loss, planned, traced)


@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_reference_order_projection_with_d_src(ops, synth, dev, layout):
    """SFM_PROJECTION_REFERENCE_ORDER together with d_src (refused until the d_src of two launches: dsrc_scatter_kernel re-projects in
    either order): the reference-order kernels record dL/dI^ themselves, the second launch samples by the reference's chain -- loss,
    every gradient and d_src against the oracle."""
    cfg = CONFIGS["edge_aware"]
    d = synth.make_inputs(B=2, H=64, W=208, n_src=2, n_scales=3, seed=43)
    ref = _oracle(d, cfg, want_d_src=True)
    fl = _bind(ops, dev, d, cfg, want_d_src=True, layout=layout, projection="reference_order")
    _check_losses(fl.forward_backward(), ref)
    _check_grads(fl, ref, 2, check_src=True, what="REFERENCE-ORDER PROJECTION with d_src, edge_aware B=2 64x208 %s" % layout, **knife_widths(d, ref))
    with pytest.raises(ValueError, match="projection"):
        ops.FusedLoss(projection="exact")


MOTIONS = {
    # name: (rot_sigma, trans_sigma, forced tz range or None).  synth's default (0.01, 0.02) is the scale of an untrained PoseNet
    # (pose_net.py:52); these are what a trained one, or a diverging one, can put out.
    "medium": (0.05, 0.10, None),          # gather footprints several times wider, a quarter of the frame out of view
    "large": (0.15, 0.25, None),           # rotations of tenths of a radian: most of the frame out of view
    "behind": (0.01, 0.02, (-0.6, -0.3)),  # the camera moved BEHIND part of the scene: z = q2 + 1e-10 < 0 there (transform.py:122-125);
                                           # the reference still divides, and samples every mirrored point that lands in view
}


def make_motion_inputs(synth, motion, **kw):
    rot, trans, tz = MOTIONS[motion]
    d = synth.make_inputs(rot_sigma=rot, trans_sigma=trans, **kw)
    if tz is not None:
        rng = np.random.RandomState(1000 + kw.get("seed", 0))
        for p in d["poses"]:
            p[:, 5] = rng.uniform(tz[0], tz[1], size=p.shape[0]).astype(np.float32)
    return d


def motion_stats(d, ref, what):
    """Prints (parity_note) what the inputs exercise: the share of warped pixels not in view and of samples with z < 0."""
    oov = np.mean([float((w == 0).all(axis=2).mean()) for w in ref["warped"]])
    neg = []
    for s, disp in enumerate(d["disps"]):
        K = d["intrinsics"][:, s]
        B, _, h, w = disp.shape
        for pose in d["poses"]:
            Pm = O.proj_tgt_to_src(pose, K)
            cam, _ = O.pixel2cam(np.broadcast_to((1.0 / disp).reshape(B, 1, h * w), (B, 3, h * w)), O.generate_2dmeshgrid(h, w, B), K)
            neg.append(float(((Pm @ cam)[:, 2] < 0).mean()))
    parity_note("motion %s: %.1f%% of the warped pixels not in view, %.1f%% of the samples behind the source camera (z < 0)" % (
        what, 100 * oov, 100 * float(np.mean(neg))))
    return oov, float(np.mean(neg))


@pytest.mark.parametrize("motion", sorted(MOTIONS))
@pytest.mark.parametrize("cfg_name,B,H,W,n_src,n_scales,layout", [
    ("ssim_smooth", 1, 37, 70, 2, 1, "planar"),
    ("explain", 2, 37, 70, 2, 2, "hwc"),
    ("edge_aware", 4, 128, 416, 2, 4, "hwc"),       # BASELINE cfg3 as written, oracle-sized batch
    ("l1_smooth", 4, 128, 416, 2, 4, "planar"),     # cfg2's loss
])
def test_large_motion_vs_oracle(ops, synth, dev, motion, cfg_name, B, H, W, n_src, n_scales, layout):
    """Inputs away from synth's small-motion default: wide gather footprints, most of a frame out of view, and samples BEHIND the
    source camera (z < 0: the reference divides anyway, transform.py:122-125, and samples the mirrored points that land in view).
    Loss, warped pixels and every gradient against the oracle by the criteria of the small-motion tests; where the projection is
    ill-conditioned (|z| small) both fp32 evaluations sit away from the fp64 one, which then decides (printed)."""
    cfg = CONFIGS[cfg_name]
    d = make_motion_inputs(synth, motion, B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=21, with_masks=True)
    ref = _oracle(d, cfg)
    what = "MOTION %s %s B=%d %dx%d %s" % (motion, cfg_name, B, H, W, layout)
    oov, neg = motion_stats(d, ref, what)
    if motion == "behind":
        assert neg > 0.05, "the case is meant to put a counted share of the samples behind the camera"
    else:
        assert oov > (0.15 if motion == "medium" else 0.5)
    ref64 = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True,
                               keep_warped=True, dtype=np.float64, **cfg)
    # (behind the camera the samples near z = 0 carry percents of a sample's d_pose each, and which cell / side of the in-view test
    #  such a sample lands in is decided by the last bit of its position: up to THREE named pixels per sample there, two elsewhere.
    #  Round 6: with the in-wave geometry on the reference's roundings the FAST projection takes another branch than the fp32 oracle
    #  at two pixels of sample 1 -- tools/diag_motion_pose.py: the REFERENCE_ORDER projection follows the oracle to 1e-6 on the same
    #  input, which is what the second half of this test holds it to.)
    fl = _bind(ops, dev, d, cfg, layout=layout, want_warped=True)
    explain = lambda i, got: pose_explained_by_discontinuities(d, cfg, ref, i, got, max_jumps=3 if motion == "behind" else 2,
                                                               hint=[to_np(t) for t in fl.d_disps])
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, what, d)
    _check_grads(fl, ref, n_src, what=what, ref64=ref64, explain=explain, check_mask=bool(cfg.get("exp_reg")), **knife_widths(d, ref))
    count_in_view_mismatches(ops, dev, d, ref, layout, what)
    # ... and SFM_PROJECTION_REFERENCE_ORDER on the same inputs: the flat criteria, no second opinion, no named pixels
    fr = _bind(ops, dev, d, cfg, layout=layout, want_warped=True, projection="reference_order")
    _check_losses(fr.forward_backward(), ref)
    # (rolled inputs: a seam of contrast 2.0 in the sources, and the mode follows the oracle's roundings up to sin / cos of the pose
    #  angles -- at most two pixels of the four scales may exceed the flat 1e-4, by the position-uncertainty criterion of the seam)
    _check_warped(fr, ref, what + " [projection = reference_order]", d, max_over_flat=2)
    _check_grads(fr, ref, n_src, what=what + " [projection = reference_order]", check_mask=bool(cfg.get("exp_reg")), **knife_widths(d, ref))


@pytest.mark.parametrize("cfg_name", ["edge_aware", "l1_smooth", "explain"])
@pytest.mark.parametrize("motion", [None, "medium", "large", "behind"])
def test_d_src_through_the_lds_window(ops, synth, dev, motion, cfg_name):
    """The optional dL/d(src) output (north_star: the backward "scatters dL/d(depth, pose, src_img)") at the BASELINE frame size:
    the gradient kernels record dL/dI^ of every warped pixel and a second launch (csrc/sfm_loss_dsrc.hip, dsrc_scatter_kernel)
    re-projects the pixels and sums their taps in an LDS window of doubles per (sample, source, band of columns) that follows the
    mean tap row and column of the band; a row that leaves the window reaches memory once, taps outside it go to memory directly.
    Default motion keeps most taps inside the window; `medium` / `large` / `behind` (wide and mirrored footprints, most of the frame
    out of view) exercise the direct path and windows that move in both directions.  d_src element-wise against the oracle outside
    the scatter footprints of knife-edge pixels, loss and the other gradients by the usual criteria (the main launch runs another
    instantiation of the kernel)."""
    cfg = CONFIGS[cfg_name]
    kw = dict(B=4, H=128, W=416, n_src=2, n_scales=4, with_masks=True)      # (the inputs of test_large_motion_vs_oracle)
    d = synth.make_inputs(seed=21, **kw) if motion is None else make_motion_inputs(synth, motion, seed=21, **kw)
    ref = _oracle(d, cfg, want_d_src=True)
    ref64 = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True, want_d_src=True,
                               keep_warped=True, dtype=np.float64, **cfg)
    what = "D_SRC %s %s B=4 128x416 hwc" % (motion or "default motion", cfg_name)
    fl = _bind(ops, dev, d, cfg, want_d_src=True, layout="hwc")
    explain = lambda i, got: pose_explained_by_discontinuities(d, cfg, ref, i, got, max_jumps=3 if motion == "behind" else 2,
                                                               hint=[to_np(t) for t in fl.d_disps])      # (see test_large_motion_vs_oracle)
    _check_losses(fl.forward_backward(), ref)
    _check_grads(fl, ref, 2, check_src=True, check_mask=bool(cfg.get("exp_reg")), what=what, ref64=ref64, explain=explain, **knife_widths(d, ref))
    # the same through the separate backward entry point, accumulated twice: d_src is ADDED to what the buffers hold (sfmwarp.h)
    first = [to_np(t).copy() for t in fl.d_srcs]
    fl.d_srcs, keep = fl.d_srcs, fl._zero_d_src
    fl._zero_d_src = lambda: None
    fl.backward(1.0)
    fl._zero_d_src = keep
    for a, t, w in zip(first, fl.d_srcs, ref["d_srcs"]):
        np.testing.assert_allclose(to_np(t), 2.0 * a, rtol=0, atol=2e-5 * max(float(np.abs(w).max()), 1e-30))


@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_d_src_of_some_scales_only(ops, synth, dev, layout):
    """SfmLossDesc.d_src[s] may be NULL for any scale: the scales that bind it get what they get when every scale binds it (the second
    launch has workgroups for them only; the record of dL/dI^ in the workspace has room for them only), the loss and the other
    gradients do not change."""
    cfg = CONFIGS["ssim_smooth"]
    d = synth.make_inputs(B=3, H=64, W=200, n_src=3, n_scales=4, seed=41)
    full = _bind(ops, dev, d, cfg, want_d_src=True, layout=layout)
    part = _bind(ops, dev, d, cfg, want_d_src=[False, True, False, True], layout=layout)
    lf, lp = to_np(full.forward_backward()).copy(), to_np(part.forward_backward()).copy()
    np.testing.assert_array_equal(lp, lf)
    assert part.d_srcs[0] is None and part.d_srcs[2] is None
    for s in (1, 3):      # the same sums, added in another order (float atomics)
        a, b = to_np(full.d_srcs[s]), to_np(part.d_srcs[s])
        assert np.abs(a).max() > 0
        np.testing.assert_allclose(b, a, rtol=0, atol=2e-6 * np.abs(a).max())
    for a, b in zip(full.d_disps + full.d_poses, part.d_disps + part.d_poses):
        np.testing.assert_array_equal(to_np(b), to_np(a))


@pytest.mark.parametrize("cfg_name", ["edge_aware", "l1_smooth"])
def test_d_src_under_heavy_minification(ops, synth, dev, cfg_name):
    """Several lanes of ONE instruction landing on one texel of the d_src window (round-5 advisor finding; since round 6 the adds are
    LDS atomics on doubles, ds_add_f64, and the hardware serialises them).  Here the source is sampled with a minification of 3 - 10
    (the camera pulled back by 3 along z, depths 0.1 - 2: U = cx + (x - cx) D / (D + tz)): runs of 3 - 10 neighbouring lanes share a
    texel in every tap instruction, and d_src must still be the oracle's sum."""
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=2, H=64, W=208, n_src=2, n_scales=3, seed=31, rot_sigma=0.002, trans_sigma=0.005)
    for p in d["poses"]:
        p[:, 5] = np.float32(3.0)
    ref = _oracle(d, cfg, want_d_src=True)
    with np.errstate(invalid="ignore"):
        du = np.abs(np.diff(ref["uv"][0][:, :, 0], axis=-1))
    shared = float((du[np.isfinite(du)] < 0.34).mean())
    assert shared > 0.5, "the case is meant to put three or more neighbouring lanes on one source column (share with |dU/dx| < 1/3: %.2f)" % shared
    fl = _bind(ops, dev, d, cfg, want_d_src=True, layout="hwc")
    _check_losses(fl.forward_backward(), ref)
    what = "D_SRC MINIFICATION %s B=2 64x208 hwc" % cfg_name
    ref64 = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True, want_d_src=True,
                               dtype=np.float64, **cfg)
    _check_grads(fl, ref, 2, check_src=True, what=what, ref64=ref64, **knife_widths(d, ref))
    parity_note("d_src %s: %.0f %% of neighbouring output pixels less than a third of a source column apart" % (what, 100 * shared))


@pytest.mark.parametrize("motion", ["medium", "behind"])
def test_large_motion_full_batch_vs_oracle(ops, synth, dev, motion):
    """The same at BASELINE cfg3's FULL batch (B=32, as written: edge-aware smoothness), pixel-interleaved: the launch bench.py's
    `cfg3_large_motion` key times."""
    cfg = CONFIGS["edge_aware"]
    d = make_motion_inputs(synth, motion, B=32, H=128, W=416, n_src=2, n_scales=4, seed=1)
    ref = _oracle(d, cfg)
    what = "MOTION %s FULL BATCH edge_aware B=32 128x416 hwc" % motion
    motion_stats(d, ref, what)
    ref64 = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True,
                               keep_warped=True, dtype=np.float64, **cfg)
    fl = _bind(ops, dev, d, cfg, layout="hwc", want_warped=True)
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, what, d)
    _check_grads(fl, ref, 2, what=what, ref64=ref64, **knife_widths(d, ref))


@pytest.mark.parametrize("smooth_field", [False, True])
def test_d_src_full_batch_vs_oracle(ops, synth, dev, smooth_field):
    """d_src at BASELINE cfg3's FULL batch (B=32, as written, pixel-interleaved): the launches bench.py's `cfg3_d_src` and
    `cfg3_d_src_smooth_disp` keys time -- 512 workgroups of the second launch in two rounds over the chip, windows that move every
    step, the samples outside them on the direct path -- against the oracle, d_src element-wise."""
    cfg = CONFIGS["edge_aware"]
    kw = dict(disp_div=32, disp_noise=0.0) if smooth_field else {}
    d = synth.make_inputs(B=32, H=128, W=416, n_src=2, n_scales=4, seed=1, **kw)
    ref = _oracle(d, cfg, want_d_src=True)
    ref64 = lambda: O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True, want_d_src=True,
                               keep_warped=True, dtype=np.float64, **cfg)
    what = "D_SRC FULL BATCH edge_aware B=32 128x416 hwc%s" % (" smooth disparity field" if smooth_field else "")
    fl = _bind(ops, dev, d, cfg, want_d_src=True, layout="hwc")
    _check_losses(fl.forward_backward(), ref)
    _check_grads(fl, ref, 2, check_src=True, what=what, ref64=ref64, **knife_widths(d, ref))
    # ... and a second call accumulates the same sums again (float atomics: to rounding)
    first = [to_np(t).copy() for t in fl.d_srcs]
    keep = fl._zero_d_src
    fl._zero_d_src = lambda: None
    fl.backward(1.0)
    fl._zero_d_src = keep
    for a, t in zip(first, fl.d_srcs):
        np.testing.assert_allclose(to_np(t), 2.0 * a, rtol=0, atol=2e-5 * max(float(np.abs(a).max()), 1e-30))


@pytest.mark.parametrize("cfg_name,B,H,W,n_src", [
    ("ssim_smooth", 32, 128, 416, 2),     # BASELINE cfg3 / cfg4's per-GPU share, live smoothness form
    ("edge_aware", 32, 128, 416, 2),      # BASELINE cfg3 as written (edge-aware smoothness)
    ("ssim_smooth", 8, 256, 832, 4),      # BASELINE cfg5, 5-frame snippet = 4 sources
    ("ssim_smooth", 8, 256, 832, 2),      # BASELINE cfg5 as parenthesised (2 source views)
])
def test_full_size_properties(ops, synth, dev, cfg_name, B, H, W, n_src):
    """BASELINE configs at their FULL batch: size-independent properties instead of an oracle run --
      * determinism: two runs agree bit for bit (loss and every gradient);
      * fused launch == separate forward / backward launches;
      * batch additivity: the loss is the sum of the two half-batch losses with norm_B = B, and every sample's
        gradients are those the half-batch run gives it -- which ties the full batch to the oracle-checked small batches;
      * hwc layout == planar layout; everything finite."""
    import torch
    cfg = CONFIGS[cfg_name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=4, seed=1)
    fl = _bind(ops, dev, d, cfg, layout="hwc")
    l1 = to_np(fl.forward_backward()).copy()
    g1 = [to_np(t).copy() for t in fl.d_disps + fl.d_poses]
    l2 = to_np(fl.forward_backward()).copy()
    g2 = [to_np(t) for t in fl.d_disps + fl.d_poses]
    np.testing.assert_array_equal(l1, l2)
    for a, b in zip(g1, g2):
        np.testing.assert_array_equal(a, b)
        assert np.isfinite(a).all()
    lf = to_np(fl.forward())
    np.testing.assert_allclose(lf, l1, rtol=2e-5)
    fl.backward(1.0)
    for a, t in zip(g1, fl.d_disps + fl.d_poses):
        np.testing.assert_allclose(to_np(t), a, rtol=0, atol=2e-5 * np.abs(a).max())
    # the two halves of the batch, normalised by the full batch
    tot = np.zeros(5)
    for lo in (0, B // 2):
        sl = slice(lo, lo + B // 2)
        part = dict(d, tgt_pyr=[a[sl] for a in d["tgt_pyr"]], src_pyr=[a[sl] for a in d["src_pyr"]], intrinsics=d["intrinsics"][sl],
                    disps=[a[sl] for a in d["disps"]], poses=[a[sl] for a in d["poses"]])
        sh = _bind(ops, dev, part, cfg, norm_B=B, layout="planar")
        tot += to_np(sh.forward_backward()).astype(np.float64)
        for s in range(4):
            np.testing.assert_allclose(to_np(sh.d_disps[s]), g1[s][sl], rtol=0, atol=2e-5 * np.abs(g1[s]).max())
        for i in range(n_src):
            np.testing.assert_allclose(to_np(sh.d_poses[i]), g1[4 + i][sl], rtol=0, atol=2e-5 * np.abs(g1[4 + i]).max())
    np.testing.assert_allclose(tot, l1.astype(np.float64), rtol=2e-5)
    torch.cuda.synchronize()


def test_identity_pose_identical_images_give_zero_photometric_loss(ops, synth, dev):
    """pose = 0 => I^ = src inside a 1-px zero frame; with
    src == tgt the L1 and SSIM terms vanish on the interior and the frame is masked out."""
    d = synth.make_inputs(B=2, H=32, W=64, n_src=2, n_scales=2, seed=3)
    # power-of-two intrinsics make K . K^-1 exact
    K = np.zeros((2, 3, 3), np.float32)
    K[:, 0, 0] = 64.0
    K[:, 1, 1] = 32.0
    K[:, 0, 2] = 32.0
    K[:, 1, 2] = 16.0
    K[:, 2, 2] = 1.0
    d["intrinsics"] = synth.multi_scale_intrinsics(K, 2)
    d["poses"] = [np.zeros((2, 6), np.float32) for _ in range(2)]
    # a power-of-two depth keeps every product of the projection exact, in the reference's
    # evaluation order too, so the 1-px frame is decided exactly (not by rounding)
    d["disps"] = [np.full_like(a, 4.0) for a in d["disps"]]
    d["src_pyr"] = [np.concatenate([t, t], axis=1) for t in d["tgt_pyr"]]
    fl = _bind(ops, dev, d, dict(ssim_rate=0.15))
    loss = to_np(fl.forward())
    assert abs(loss[1]) < 2e-6          # pixel: exact 0 up to the fp32 rounding of U = q0/z
    # SSIM is NOT zero next to the zero frame (unmasked zeros enter the 3x3 windows), but must match the oracle
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], ssim_rate=0.15)
    assert abs(loss[4] - ref["ssim_loss"]) <= 1e-4 * max(ref["ssim_loss"], 1e-6)


@pytest.mark.parametrize("layout", ["planar", "hwc"])
def test_images_outside_the_unit_range(ops, synth, dev, layout):
    """The input contract is the reference's: images uint8 / 127.5 - 1 in [-1, 1] (datasets/kitti/kitti_raw_dataset.py:12-14).
    What happens outside it, pinned (round-3 advisor finding):
      * the zero mask of models/base_model.py:96 and the L1 path hold for images of ANY finite range -- checked here on 0..255
        images: loss and every gradient against the oracle (rounds 1-3 OR-ed the channels' bit patterns for the mask, which
        silently mis-masked pixels once values of 128+ met values in [1, 2): pixel_loss was 3.6 % low);
      * with SSIM the five scalars still match the oracle at 0..255; the gradients do not have to be finite there: the variance
        terms E[x^2] - mu^2 cancel in fp32 at that range (in the reference too), the denominator of SSIM can reach 0, and the
        packed clip mask then multiplies an infinite reciprocal by 0 where the reference's F.clip backward gives 0
        (include/sfmwarp.h states the range the SSIM gradient is defined for);
      * a NaN pixel makes the loss NaN, as in the reference."""
    d = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=2, seed=3)
    big = dict(d, tgt_pyr=[(a * 127.5 + 127.5).astype(np.float32) for a in d["tgt_pyr"]],
               src_pyr=[(a * 127.5 + 127.5).astype(np.float32) for a in d["src_pyr"]])
    cfg = CONFIGS["l1_smooth"]
    ref = _oracle(big, cfg)
    fl = _bind(ops, dev, big, cfg, layout=layout, want_warped=True)
    _check_losses(fl.forward_backward(), ref)
    _check_warped(fl, ref, "0..255 images l1_smooth %s" % layout, big)
    kw = knife_widths(big, ref, abs_floor=3e-5 * 127.5)           # the kink of |I^ - I| in units of the image range
    _check_grads(fl, ref, 2, what="0..255 images l1_smooth %s" % layout, **kw)
    cfg = CONFIGS["ssim_smooth"]
    _check_losses(_bind(ops, dev, big, cfg, layout=layout).forward(), _oracle(big, cfg))
    # in contract every output is finite, SSIM included
    fl = _bind(ops, dev, d, cfg, layout=layout)
    assert np.isfinite(to_np(fl.forward_backward())).all()
    assert all(np.isfinite(to_np(t)).all() for t in fl.d_disps + fl.d_poses)
    # a NaN pixel: the reference's loss is NaN (F.absolute / F.mean propagate it) and so is this one
    bad = dict(d, src_pyr=[a.copy() for a in d["src_pyr"]])
    bad["src_pyr"][0][0, 1, 10, 40] = np.nan
    loss5 = to_np(_bind(ops, dev, bad, cfg, layout=layout).forward())
    assert np.isnan(loss5[0]) and np.isnan(loss5[1]) and np.isfinite(loss5[2])      # total, pixel; the smoothness term does not see the images


def test_argument_errors(ops, synth, dev):
    d = synth.make_inputs(B=1, H=16, W=24, n_src=2, n_scales=1, seed=3)
    with pytest.raises(ValueError):
        ops.FusedLoss(smooth_mode="bogus")
    with pytest.raises(ValueError):          # exp_reg without masks
        _bind(ops, dev, d, dict(exp_reg=0.2))
    with pytest.raises(TypeError):           # CPU tensors are rejected, no fallback
        import torch
        ops.FusedLoss().bind([torch.from_numpy(a) for a in d["tgt_pyr"]], [torch.from_numpy(a) for a in d["src_pyr"]],
                             torch.from_numpy(d["intrinsics"]), [torch.from_numpy(a) for a in d["disps"]],
                             [torch.from_numpy(a) for a in d["poses"]])
    with pytest.raises(ValueError):          # unknown layout name
        _bind(ops, dev, d, dict(), layout="chw")
    with pytest.raises(TypeError):           # planar arrays announced as pixel-interleaved
        ops.FusedLoss().bind([to_dev(a, dev) for a in d["tgt_pyr"]], [to_dev(a, dev) for a in d["src_pyr"]],
                             to_dev(d["intrinsics"], dev), [to_dev(a, dev) for a in d["disps"]],
                             [to_dev(a, dev) for a in d["poses"]], layout="hwc")
    fl = _bind(ops, dev, d, dict())
    fl.desc.image_layout = 7                 # the C ABI rejects a layout code it does not know
    with pytest.raises(ValueError):
        fl.forward()
    tiny = synth.make_inputs(B=1, H=16, W=24, n_src=1, n_scales=4, seed=3)   # smallest scale 2x3 < 3
    with pytest.raises((TypeError, ValueError)):
        _bind(ops, dev, tiny, dict())


def test_entry_points_are_graph_capturable_and_stream_safe(ops, synth, dev):
    """The launch functions allocate nothing and never synchronise: a step can be captured into a
    HIP graph and replayed, and two bound instances can run concurrently on two streams."""
    import torch
    cfg = CONFIGS["ssim_smooth"]
    d = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=2, seed=13)
    fl = _bind(ops, dev, d, cfg)
    want = to_np(fl.forward_backward()).copy()
    g_want = to_np(fl.d_disps[0]).copy()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fl.forward_backward()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        fl.forward_backward()
    torch.cuda.synchronize()
    fl.loss5.zero_()
    fl.d_disps[0].zero_()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(to_np(fl.loss5), want)
    np.testing.assert_array_equal(to_np(fl.d_disps[0]), g_want)
    # two independent instances on two streams
    d2 = synth.make_inputs(B=3, H=32, W=104, n_src=2, n_scales=2, seed=14)
    fl2 = _bind(ops, dev, d2, cfg)
    want2 = to_np(fl2.forward_backward()).copy()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(5):
        with torch.cuda.stream(s1):
            fl.forward_backward()
        with torch.cuda.stream(s2):
            fl2.forward_backward()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(to_np(fl.loss5), want)
    np.testing.assert_array_equal(to_np(fl2.loss5), want2)
