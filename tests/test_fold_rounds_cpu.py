"""The preconditions of the GPU tests that follow a fold kernel past its first 64 partial sums, checked without a GPU.

Three gradient paths end in a kernel in which ONE wave adds a sample's partial sums, lane l taking partials l, l + 64, l + 128, ...:
    warp_pyr_fold_kernel   csrc/sfm_warp_pyramid.hip   256-pixel blocks per (sample, source, scale)   d_pose of sfm_warp_pyramid_bwd
    intr_bwd_fold_kernel   csrc/sfm_ops.hip            256-pixel blocks per sample                    d_K of sfm_warp_intrinsics_bwd
    proj_bwd_kernel        csrc/sfm_loss.hip           tiles per (sample, scale, source)              d_proj, d_intrinsics of sfm_loss_proj_bwd
A case of at most 64 partials never takes the second trip of that loop, and would pass whatever a later trip did.  The cases that
go further are  tests/test_warp_pyramid_gpu.py::FOLD_CASES (65 blocks),  tests/test_intrinsics_grad_gpu.py::WARP_LARGE (65 and 208
blocks),  tests/intrinsics_grad.py::LARGE_SHAPES / LARGE_FAMILY_CASES (66, 128 and 224 tiles)  and, on textured inputs,
tests/intrinsics_exact_ref.py::FOLD_SHAPE (65 tiles).  A block size or a plan heuristic
that changes could take them back inside the first trip without any of those tests failing; this module fails instead.

  1. the block sizes, read from the sources, give more than 64 blocks at scale 0 of every such warp case;
  2. sfm_loss_plan_info (host only, nothing is launched) gives the expected kernel family and more than 64 tiles for every such
     fused case;
  3. discrimination for the two warp operators: the fp64 autograd reference is evaluated again with the upstream gradient zeroed on
     every pixel j >= 64 * 256 of each image -- what a fold that stops after its first trip would return -- and must move, in every
     sample, by at least 5 x the tolerance the GPU test compares with.  This is a condition on the inputs, not on the kernel.
For the fused loss the map from tiles to pixels is internal to the kernels, so there is no such reference here.  There the guarantee
is the share of tiles beyond the first trip (2 of 66, 64 of 128, 160 of 224: asserted below) together with the comparison of d_proj
per scale in test_d_intrinsics_against_fp64_autograd_on_ramp_inputs, which sees one scale's fold alone."""
import os
import re

import numpy as np
import pytest

import intrinsics_exact_ref as XR
import intrinsics_grad as IG
import test_intrinsics_grad_gpu as KG      # (importing a GPU module's cases launches nothing)
import test_warp_pyramid_gpu as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64
TUNING = [k for k in os.environ if k.startswith("SFM_")]      # (read once per process by the library: cannot be unset here)


def _constant(source, name):
    text = open(os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", source)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


WP_BLOCK, WARP_BLOCK = _constant("sfm_warp_pyramid.hip", "WP_BLOCK"), _constant("sfm_ops.hip", "WARP_BLOCK")


def _blocks(h, w, block):
    return -(-h * w // block)


# ------------------------------------------------------------------------------------------------------------------------
# 1. blocks
# ------------------------------------------------------------------------------------------------------------------------
def test_the_new_warp_cases_have_more_than_64_blocks():
    assert WP.FOLD_CASES and all(c in WP.CASES for c in WP.FOLD_CASES)
    assert {kind for _, _, kind in WP.FOLD_CASES} == {None, "general"}
    for shape, _, _ in WP.FOLD_CASES:
        B, H, W, n, S = shape
        assert _blocks(H, W, WP_BLOCK) > WAVE and B > 1 and n > 1, shape      # ... with a later sample and a later source
    # the counts the docstring of tests/test_warp_pyramid_gpu.py states, every scale of every shape
    per_scale = {shape: [_blocks(shape[1] >> s, shape[2] >> s, WP_BLOCK) for s in range(shape[4])] for shape in WP.SHAPES}
    assert per_scale == {(2, 24, 40, 1, 3): [4, 1, 1], (2, 20, 52, 3, 2): [5, 2], (3, 16, 52, 4, 1): [4], (2, 130, 127, 2, 2): [65, 16]}
    assert (130 * 127) % WP_BLOCK == 126                                      # a partial last block
    large = sorted({shape for _, _, shape in KG.WARP_K_CASES if shape != KG.WARP_SMALL})
    assert large == sorted(KG.WARP_LARGE) and len(large) == 2
    assert [_blocks(s[1], s[2], WARP_BLOCK) for s in KG.WARP_LARGE] == [65, 208] and all(s[0] > 1 for s in KG.WARP_LARGE)
    for shape in KG.WARP_LARGE:      # C = 3 with one depth row and at least one case of three depth rows at each shape
        have = {(c, r) for c, r, s in KG.WARP_K_CASES if s == shape}
        assert (3, 1) in have and any(r == 3 for _, r in have), shape


# ------------------------------------------------------------------------------------------------------------------------
# 2. tiles and families
# ------------------------------------------------------------------------------------------------------------------------
def test_the_new_fused_cases_have_more_than_64_tiles_in_the_expected_family():
    assert not TUNING, "the plan holds for a library without tuning overrides; unset %s" % TUNING
    assert all(c in KG.FAMILY_CASES for c in IG.LARGE_FAMILY_CASES)
    at_66 = [c for c in IG.LARGE_FAMILY_CASES if c[1] == IG.LARGE_SHAPES[0]]
    assert sorted(c[6] for c in at_66) == sorted(IG.FAMILIES.values())        # every family once at 66 tiles
    assert sorted(c[6] for c in IG.LARGE_FAMILY_CASES if c[1] == IG.LARGE_SHAPES[2]) == ["base", "pair"]
    for name, shape, mode, layout, projection, want_d_src, fam in IG.LARGE_FAMILY_CASES:
        for loss in (1, 0):          # sfm_loss_fwd_bwd, and the sfm_loss_bwd the test runs after it
            tiles, got = IG.host_plan(shape, mode, layout, projection, want_d_src, grad=1, loss=loss)
            assert got == fam and tiles == IG.LARGE_TILES[shape] and max(tiles) > WAVE, (name, loss, got, tiles)
    # sfm_loss_bwd alone, on the descriptor the workload binds
    assert IG.host_plan(IG.LARGE_SHAPES[0], "ssim_smooth", "hwc", grad=1, loss=0)[1] == "pair"
    # the end-to-end cases: every configuration, projection and layout of every large shape
    for shape, kind in KG.END_TO_END:
        if shape in IG.LARGE_SHAPES:
            assert kind == "general"
            for mode in IG.CONFIGS:
                for projection in ("reference_order", "fast"):
                    for layout in ("planar", "hwc"):
                        tiles = IG.host_plan(shape, mode, layout, projection)[0]
                        assert tiles == IG.LARGE_TILES[shape] and max(tiles) > WAVE, (shape, mode, projection, layout, tiles)
    assert [s for s, _ in KG.END_TO_END if s in IG.LARGE_SHAPES] == IG.LARGE_SHAPES
    # the share of a sample's scale-0 tiles that only a later trip reaches, and a scale that is the boundary itself
    assert [IG.LARGE_TILES[s][0] - WAVE for s in IG.LARGE_SHAPES] == [2, 64, 160] and IG.LARGE_TILES[IG.LARGE_SHAPES[2]][1] == WAVE
    # the small shapes stay what their docstrings say: at most 6 tiles per scale
    assert max(max(IG.host_plan(s, "ssim_smooth")[0]) for s in IG.SHAPES) <= 6
    # the textured, knife-free frame of tests/intrinsics_exact_ref.py: 260 rows in 4-row chunks, one strip -- 65 tiles, one lane goes
    # round a second time -- in every launch tests/test_intrinsics_exact_gpu.py makes of it
    assert XR.FOLD_SHAPE == (1, 260, 20, 2, 1) and XR.FOLD_TILES == [65] and XR.FOLD_SHAPE in XR.CASES
    for mode in XR.CONFIGS:
        for projection in ("reference_order", "fast"):
            for layout in ("planar", "hwc"):
                for want_d_src in (False, True):
                    for loss in (1, 0):
                        tiles = IG.host_plan(XR.FOLD_SHAPE, mode, layout, projection, want_d_src, grad=1, loss=loss)[0]
                        assert tiles == XR.FOLD_TILES and max(tiles) > WAVE, (mode, projection, layout, want_d_src, loss, tiles)


def test_the_pose_tolerance_follows_the_documented_rule():
    """1e-5 for 100 tiles is a margin of 1.7 over 100 x 2^-24; the same margin for T tiles, never below 1e-5"""
    assert KG.POSE_TOL == 1e-5 and 1.6 < KG.POSE_TOL / (100 * 2.0 ** -24) < 1.7
    assert KG.pose_tol([6, 2, 1]) == KG.pose_tol([98]) == 1e-5
    assert KG.pose_tol([224, 64, 16, 4]) == 1.7 * 308 * 2.0 ** -24 and 3.1e-5 < KG.pose_tol([224, 64, 16, 4]) < 3.2e-5


# ------------------------------------------------------------------------------------------------------------------------
# 3. discrimination
# ------------------------------------------------------------------------------------------------------------------------
LARGE_K = [(c, r, s) for c, r, s in KG.WARP_K_CASES if s != KG.WARP_SMALL]


@pytest.mark.parametrize("C_,depth_rows,shape", LARGE_K, ids=["%d-%d-%dx%d" % (c, r, s[1], s[2]) for c, r, s in LARGE_K])
def test_d_K_of_the_warp_moves_when_the_later_trips_are_dropped(C_, depth_rows, shape):
    """every entry of d_K, measured as the GPU test measures it (intrinsics_grad.entry_errors: the worst sample over the entry's
    size), by at least 5 x REF_TOL; and each sample on its own in at least one entry, so that a trip dropped for one sample alone
    shows too.  Measured: 1.0e-2 at least at 130 x 127 (3-1), 0.17 at least at 128 x 416 (1-1)."""
    imgs, depth, pose, K, g = KG.warp_case(C_, depth_rows, shape)
    N, _, H, W = imgs.shape
    depth3 = depth if depth_rows == 3 else np.repeat(depth[:, None], 3, axis=1)
    ref = IG.autograd_warp(imgs, depth3, pose, K, g)
    cut = g.copy().reshape(N, C_, H * W)
    cut[:, :, WAVE * WARP_BLOCK:] = 0
    first_trip = IG.autograd_warp(imgs, depth3, pose, K, cut.reshape(g.shape))
    moved = IG.entry_errors(first_trip, ref)
    assert moved.shape == (1, 3, 3) and moved.min() >= 5 * KG.REF_TOL, moved
    per_sample = (np.abs(first_trip - ref) / np.abs(ref).max(axis=0)).reshape(N, 9).max(axis=1)
    assert per_sample.min() >= 5 * KG.REF_TOL, per_sample


@pytest.mark.parametrize("case", WP.FOLD_CASES, ids=[WP.IDS[WP.CASES.index(c)] for c in WP.FOLD_CASES])
def test_d_pose_of_the_warp_pyramid_moves_when_the_later_trips_are_dropped(case):
    """max |change| / max |d_pose| of every source against 5 x 1e-5, the bound on |new - A| / max |A| (the other criterion, E_new <=
    1.5 E_old + 2e-6, allows 2.3e-5 at the E_old of 1.4e-5 observed on the MI355X).  Measured: 0.03 at least, a thousand times either.
    Per (sample, source) the 126 pixels of block 64 -- the frame's bottom row -- carry 0.03 to 0.14 of max |d_pose|, except for
    the second source of the second sample, where that row is out of view and carries exactly nothing: every sample and every
    source has a pair that discriminates, that one pair has not."""
    h = WP.host_case(*case)
    B, H, W, n, S = h["shape"]
    ref, first_trip = WP._autograd_d_pose(h), WP._autograd_d_pose(h, first_pixels=WAVE * WP_BLOCK)
    assert len(ref) == n
    moved = np.stack([np.abs(first_trip[i] - ref[i]).max(axis=1) / np.abs(ref[i]).max() for i in range(n)])      # (source, sample)
    assert moved.shape == (n, B)
    assert (moved.max(axis=1) >= 5 * 1e-5).all() and (moved.max(axis=0) >= 5 * 1e-5).all(), moved
    assert (moved >= 5 * 1e-5).sum() >= n * B - 1, moved
