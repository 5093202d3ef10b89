"""The gradient with respect to the camera intrinsics on the GPU: sfm_loss_proj_bwd behind every kind of gradient launch of the fused
loss, sfm_warp_intrinsics_bwd and sfm_pose_proj_bwd_k (include/sfmwarp.h).

  1. self-consistency: d_intrinsics against the closed form (tests/intrinsics_grad.py, NumPy fp64) evaluated on the library's own
     d_proj, 1e-5 per entry -- the kernel works in fp64 and the test's input is rounded once (CPU floor 9.2e-7,
     tests/test_intrinsics_grad_cpu.py).  Knife pixels cannot affect it, so it runs on ramp AND on ordinary inputs, for every kernel
     family sfm_loss_plan_info can report and every entry point.
  2. d_proj against the d_pose the library has returned all along: both fold the same fp32 tile sums, finalize_kernel in fp32
     (<= 100 tiles x 2^-24 = 6e-6), hence 1e-5 of max |d_pose|; with T tiles per sample (sfm_loss_plan_info) the same rule gives
     max(1e-5, 1.7 T 2^-24) -- 1.7 is the margin 1e-5 has over 100 tiles.  Every case of up to 98 tiles keeps 1e-5.
  3. end to end against fp64 autograd on the ramp inputs (no knife pixels, nothing excluded): 1e-3 per entry for the reference-order
     projection and the warp operator (10 x the fp32 floor measured on the CPU), the project's GRAD_TOL for the fast projection.
  4. the operators.
Every tolerance is PER ENTRY of K and per scale (intrinsics_grad.entry_errors), never against the array maximum.

How far the folds are followed.  Both fold kernels here add a sample's partial sums with one wave, lane l taking partials l, l + 64,
l + 128, ...; a shape of at most 64 partials never leaves the first trip of that loop.
  proj_bwd_kernel (sfm_loss_proj_bwd), tiles per (sample, scale):
    intrinsics_grad.SHAPES and the small FAMILY_CASES      at most 6: the first trip only
    (2, 264, 60, 2, 2)   66, 33            two lanes go round a second time; a second sample
    (2, 128, 208, 3, 1)  128               exactly two full trips; three sources
    (1, 128, 416, 2, 4)  224, 64, 16, 4    three trips and a half at scale 0, exactly one at scale 1
  intr_bwd_fold_kernel (sfm_warp_intrinsics_bwd), 256-pixel blocks per sample:
    (2, 17, 29)    2                       the first trip only
    (2, 130, 127)  65                      one lane goes round a second time, with 126 pixels in its block; a second sample
    (2, 128, 416)  208                     three full trips and a part of a fourth
tests/test_fold_rounds_cpu.py pins these counts, and shows for the warp operator that the reference moves by far more than the
tolerance when the pixels beyond the first 64 blocks are left out.  For the fused loss the map from tiles to pixels is internal;
there the guarantee is the share of tiles beyond the first trip (2 of 66, 64 of 128, 160 of 224) together with the comparison of
d_proj per scale, which sees one scale's fold alone where the sum in d_K blurs it."""
import ctypes as C

import numpy as np
import pytest
import torch

import intrinsics_grad as IG
from oracle import sfm_oracle as O
from test_loss_gpu import GRAD_TOL, _bind
from util import parity_note, to_dev, to_np

pytestmark = pytest.mark.gpu

SELF_TOL = 1e-5
POSE_TOL = 1e-5
REF_TOL = 1e-3
FAMILIES = IG.FAMILIES


note = parity_note      # every observed worst value goes into the parity statistics the suite prints and keeps (tests/conftest.py)


def plan(ops, fl, grad, loss):
    """([tiles per sample of scale s], family name) of the entry point (grad, loss) on the bound descriptor"""
    return IG.plan_of(ops.lib, fl.desc, grad, loss)


def pose_tol(tiles):
    """the module docstring's rule for T tiles per sample"""
    return max(POSE_TOL, 1.7 * sum(tiles) * 2.0 ** -24)


def bind(ops, dev, d, mode, layout="planar", projection="fast", want_d_src=False, norm_B=None, frames=False):
    """a FusedLoss on the inputs d that leaves d_intrinsics and d_proj.  frames: the pixel-interleaved pyramid buffers
    step_from_frames writes (the bound pyramids then come from the full-resolution frames)"""
    cfg = IG.CONFIGS[mode]
    fl = ops.FusedLoss(projection=projection, **cfg)
    S = len(d["disps"])
    if frames:
        tgt, src = ops.pyramid_pair_hwc(to_dev(d["tgt_pyr"][0], dev), to_dev(d["src_pyr"][0], dev), S)
        layout = "hwc"
    else:
        tgt, src = [to_dev(a, dev) for a in d["tgt_pyr"]], [to_dev(a, dev) for a in d["src_pyr"]]
        if layout == "hwc":
            tgt, src = [ops.to_hwc(a) for a in tgt], [ops.to_hwc(a) for a in src]
    fl.bind(tgt, src, to_dev(d["intrinsics"], dev), [to_dev(a, dev) for a in d["disps"]], [to_dev(a, dev) for a in d["poses"]],
            [to_dev(a, dev) for a in d["masks"]], norm_B=norm_B, want_d_src=want_d_src, layout=layout, want_d_intrinsics=True,
            want_d_proj=True)
    return fl


def check_self(fl, d, what):
    """d_intrinsics against the closed form on the library's own d_proj; returns (d_intrinsics, d_proj) as NumPy arrays"""
    dK, dP = to_np(fl.d_intrinsics).copy(), to_np(fl.d_proj).copy()
    assert np.isfinite(dK).all() and np.isfinite(dP).all(), what
    err = IG.worst(dK, IG.d_k_from_d_proj(d["intrinsics"], d["poses"], dP))
    note("INTRINSICS self-consistency %s: worst entry %.3g (tol %.0e)" % (what, err, SELF_TOL))
    assert err <= SELF_TOL, (what, err)
    return dK, dP


def check_pose(ops, fl, d, dP, what, loss=1):
    """d_proj through the oracle's backward of proj_tgt_to_src (fp64), summed over the scales, against the library's d_pose;
    loss: 0 after sfm_loss_bwd, 1 after the calls that also compute the loss (the plan whose tiles were folded)"""
    B, S, n = dP.shape[:3]
    tol = pose_tol(plan(ops, fl, 1, loss)[0])
    for i in range(n):
        got = np.zeros((B, 6))
        for s in range(S):
            g = np.zeros((B, 4, 4))
            g[:, :3] = dP[:, s, i]
            got += O.proj_tgt_to_src_backward(d["poses"][i], d["intrinsics"][:, s], g, np.float64)
        ref = to_np(fl.d_poses[i]).astype(np.float64)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        note("INTRINSICS d_proj -> d_pose[%d] %s: %.3g of max |d_pose| (tol %.3g)" % (i, what, err, tol))
        assert err <= tol, (what, i, err, tol)


# (name, shape, mode, layout, projection, want_d_src, the family the gradient launch must be)
FAMILY_CASES = [
    ("base planar", (2, 17, 29, 3, 2), "ssim_smooth", "planar", "fast", False, "base"),
    ("base hwc three sources", (2, 17, 29, 3, 2), "ssim_smooth", "hwc", "fast", False, "base"),
    ("wide", (3, 24, 40, 2, 3), "l1", "planar", "fast", False, "wide"),
    ("pair", (2, 12, 20, 2, 2), "ssim_smooth", "hwc", "fast", False, "pair"),
    ("pair four sources", (2, 16, 52, 4, 1), "edge_aware", "hwc", "fast", False, "pair"),
    ("ref planar", (3, 24, 40, 2, 3), "ssim_smooth", "planar", "reference_order", False, "ref"),
    ("ref hwc", (2, 17, 29, 3, 2), "edge_aware", "hwc", "reference_order", False, "ref"),
    ("ref with d_src", (2, 12, 20, 2, 2), "ssim_smooth", "planar", "reference_order", True, "ref"),
    ("dsrc", (2, 17, 29, 3, 2), "ssim_smooth", "hwc", "fast", True, "dsrc"),
    ("dsrc l1", (2, 16, 52, 4, 1), "l1", "planar", "fast", True, "dsrc"),
    ("explain", (3, 24, 40, 2, 3), "explain", "planar", "fast", False, "base"),
    ("explain hwc", (2, 12, 20, 2, 2), "explain", "hwc", "fast", False, "base"),
] + IG.LARGE_FAMILY_CASES      # ... and every family past 64 tiles per sample and scale


@pytest.mark.parametrize("inputs", ["ramp", "synth"])
@pytest.mark.parametrize("case", FAMILY_CASES, ids=[c[0].replace(" ", "_") for c in FAMILY_CASES])
def test_d_intrinsics_is_the_closed_form_of_d_proj_in_every_kernel_family(ops, dev, case, inputs):
    name, shape, mode, layout, projection, want_d_src, fam = case
    d = (IG.ramp_inputs if inputs == "ramp" else IG.synth_inputs)(shape, "general")
    fl = bind(ops, dev, d, mode, layout, projection, want_d_src)
    what = "%s [%s, %s inputs]" % (name, mode, inputs)
    tiles, got_fam = plan(ops, fl, 1, 1)
    assert got_fam == fam, (what, got_fam)
    if case in IG.LARGE_FAMILY_CASES:      # what the case is for: a fold that goes round again
        assert max(tiles) > 64 and tiles == IG.LARGE_TILES[shape], (what, tiles)
    fl.forward_backward()
    dK, dP = check_self(fl, d, what + " sfm_loss_fwd_bwd")
    check_pose(ops, fl, d, dP, what + " sfm_loss_fwd_bwd")
    # the same launch with its header read from the struct (hook 3 leaves the tile layout alone): the same bits
    fl.d_intrinsics.fill_(7.0), fl.d_proj.fill_(7.0)
    fl.forward_backward(variant=3)
    assert np.array_equal(to_np(fl.d_intrinsics), dK) and np.array_equal(to_np(fl.d_proj), dP), what + " hook 3"
    # sfm_loss_bwd lays its work out on its own (its family may differ): gy = 2.5 is in the sums
    fam_b = plan(ops, fl, 1, 0)[1]
    fl.backward(2.5)
    dKb, dPb = check_self(fl, d, what + " sfm_loss_bwd gy=2.5 (%s)" % fam_b)
    check_pose(ops, fl, d, dPb, what + " sfm_loss_bwd gy=2.5", loss=0)
    if fam_b == fam:       # the same per-pixel arithmetic: 2.5 x up to the rounding of gy into the per-pixel factors
        err = IG.worst(dKb, 2.5 * dK.astype(np.float64))
        note("INTRINSICS %s: sfm_loss_bwd(2.5) against 2.5 x sfm_loss_fwd_bwd, worst entry %.3g" % (what, err))
        assert err <= SELF_TOL, (what, err)


@pytest.mark.parametrize("inputs", ["ramp", "synth"])
def test_step_from_frames_and_a_batch_shard(ops, dev, inputs):
    shape = (3, 24, 40, 2, 3)
    d = (IG.ramp_inputs if inputs == "ramp" else IG.synth_inputs)(shape, "skew")
    fl = bind(ops, dev, d, "ssim_smooth", frames=True)
    fl.step_from_frames(to_dev(d["tgt_pyr"][0], dev), to_dev(d["src_pyr"][0], dev), grad=True)
    dK, dP = check_self(fl, d, "sfm_step_fwd_bwd [%s inputs]" % inputs)
    check_pose(ops, fl, d, dP, "sfm_step_fwd_bwd [%s inputs]" % inputs)
    # norm_B > B: every mean divides by the global batch, and so do the sums
    fs = bind(ops, dev, d, "ssim_smooth", layout="hwc", norm_B=2 * shape[0])
    fs.forward_backward()
    dKs, dPs = check_self(fs, d, "norm_B = 2 B [%s inputs]" % inputs)
    check_pose(ops, fs, d, dPs, "norm_B = 2 B [%s inputs]" % inputs)
    if inputs == "ramp":      # (the pyramid of a ramp is the ramp up to rounding: the same loss, half of it)
        assert IG.worst(2.0 * dKs.astype(np.float64), dK) <= 1e-3


def test_two_calls_agree_bit_for_bit_and_the_defaults_launch_nothing(ops, dev):
    d = IG.ramp_inputs((2, 17, 29, 3, 2), "general")
    fl = bind(ops, dev, d, "ssim_smooth")
    fl.forward_backward()
    dK, dP = to_np(fl.d_intrinsics).copy(), to_np(fl.d_proj).copy()
    for _ in range(2):      # the call reads the workspace and never writes it: it may be repeated
        fl.d_intrinsics.fill_(3.0), fl.d_proj.fill_(3.0)
        fl._proj_bwd(1)
        assert np.array_equal(to_np(fl.d_intrinsics), dK) and np.array_equal(to_np(fl.d_proj), dP)
    # either output alone
    only_k = torch.full_like(fl.d_intrinsics, 5.0)
    ops._launch(dev, ops.lib.sfm_loss_proj_bwd, C.byref(fl.desc), 1, C.c_void_p(fl._ws_ptr), fl._ws_bytes, None, C.c_void_p(only_k.data_ptr()))
    only_p = torch.full_like(fl.d_proj, 5.0)
    ops._launch(dev, ops.lib.sfm_loss_proj_bwd, C.byref(fl.desc), 1, C.c_void_p(fl._ws_ptr), fl._ws_bytes, C.c_void_p(only_p.data_ptr()), None)
    assert np.array_equal(to_np(only_k), dK) and np.array_equal(to_np(only_p), dP)
    # the other gradients do not depend on the extra call, and without the flags there is none
    plain = _bind(ops, dev, d, IG.CONFIGS["ssim_smooth"])
    assert plain.d_intrinsics is None and plain.d_proj is None and plain._proj_args is None
    plain.forward_backward()
    for a, b in zip(plain.d_disps + plain.d_poses, fl.d_disps + fl.d_poses):
        assert torch.equal(a, b)


END_TO_END = [(shape, kind) for shape in IG.SHAPES for kind in IG.KINDS] + [(shape, "general") for shape in IG.LARGE_SHAPES]


@pytest.mark.parametrize("shape,kind", END_TO_END, ids=["%s-%s" % ("x".join(map(str, s)), k) for s, k in END_TO_END])
def test_d_intrinsics_against_fp64_autograd_on_ramp_inputs(ops, dev, shape, kind):
    """REFERENCE_ORDER: 1e-3 per entry, 10 x the fp32 floor of tests/test_intrinsics_grad_cpu.py.  FAST: the project's GRAD_TOL.

    At intrinsics_grad.LARGE_SHAPES (general cameras; tiles per scale in the module docstring) d_proj too is compared with
    autograd's dL/dPm, per scale, source and entry, by the same rule and with the same two tolerances.  The fp32 floors there --
    fp32 autograd against fp64 autograd on the CPU, worst entry over the four loss configurations:
        shape                 d_K       d_proj
        (2, 264, 60, 2, 2)    1.6e-5    1.2e-5
        (2, 128, 208, 3, 1)   5.9e-6    6.3e-5
        (1, 128, 416, 2, 4)   5.7e-6    1.2e-4   (ssim_smooth and edge_aware; 4e-6 without the SSIM term)
    so REF_TOL keeps a margin of 8 x or more."""
    d = IG.ramp_inputs(shape, kind)
    large = tuple(shape) in IG.LARGE_SHAPES
    worst = {"reference_order": 0.0, "fast": 0.0}
    for mode in IG.CONFIGS:
        ref = IG.reference(tuple(shape), kind, mode)
        for projection in ("reference_order", "fast"):
            for layout in ("planar", "hwc"):
                fl = bind(ops, dev, d, mode, layout, projection)
                fl.forward_backward()
                err = IG.worst(to_np(fl.d_intrinsics), ref["d_K"])
                worst[projection] = max(worst[projection], err)
                tol = REF_TOL if projection == "reference_order" else GRAD_TOL
                what = "%s cameras %s B=%d %dx%d %d src %s %s" % (kind or "canonical", mode, shape[0], shape[1], shape[2], shape[3], layout,
                                                                projection)
                note("INTRINSICS end to end %s: worst entry %.3g (tol %.0e)" % (what, err, tol))
                assert err <= tol, (mode, projection, layout, err)
                if large:
                    assert max(plan(ops, fl, 1, 1)[0]) > 64
                    per_scale = IG.proj_entry_errors(to_np(fl.d_proj), ref["d_proj"]).max(axis=(1, 2, 3))
                    note("INTRINSICS end to end d_proj %s: worst entry of scale 0.. %s (tol %.0e)"
                         % (what, " ".join("%.3g" % e for e in per_scale), tol))
                    assert (per_scale <= tol).all(), (mode, projection, layout, per_scale)


# ---------------------------------------------------------------------------------------------------------------------------
# the operators
# ---------------------------------------------------------------------------------------------------------------------------
def warp_case(C_, depth_rows, shape=(2, 17, 29, 3, 2)):
    """ramp sources (the first C_ channel planes of the ramp pyramid), general cameras, a smooth random upstream gradient and, for
    depth_rows = 3, three different depth rows (models/transform.py:107)"""
    import importlib
    synth = importlib.import_module("sfm-learner-chainer_amd.synth")
    d = IG.ramp_inputs(shape, "general")
    N, H, W = shape[:3]
    rng = np.random.RandomState(40 + C_)
    imgs = np.ascontiguousarray(d["src_pyr"][0][:, :C_])
    depth = (1.0 / d["disps"][0]).reshape(N, 1, H * W)
    if depth_rows == 3:
        rows = 1.0 + 0.1 * synth._smooth_field(rng, N, 3, H, W, 4).reshape(N, 3, H * W)
        depth = np.ascontiguousarray(depth * rows, dtype=np.float32)
    else:
        depth = np.ascontiguousarray(depth[:, 0], dtype=np.float32)
    g = synth._smooth_field(rng, N, C_, H, W, 4)
    return imgs, depth, d["poses"][0], np.ascontiguousarray(d["intrinsics"][:, 0]), g


WARP_SMALL = (2, 17, 29, 3, 2)
WARP_LARGE = [(2, 130, 127, 2, 1), (2, 128, 416, 2, 1)]      # 65 and 208 blocks of 256 pixels per sample
# (C_, depth_rows, shape); the small shape keeps the ids it has always had
WARP_K_CASES = [(c, r, shape) for shape in [WARP_SMALL] + WARP_LARGE for c in (1, 3, 5) for r in (1, 3)]
WARP_K_IDS = ["%d-%d" % (c, r) + ("" if shape == WARP_SMALL else "-%dx%d" % shape[1:3]) for c, r, shape in WARP_K_CASES]


@pytest.mark.parametrize("C_,depth_rows,shape", WARP_K_CASES, ids=WARP_K_IDS)
def test_warp_intrinsics_bwd_against_autograd(ops, dev, C_, depth_rows, shape):
    """REF_TOL = 1e-3 per entry against fp64 autograd, ten times the fp32 floor.  The floor of every case beyond 64 blocks -- fp32
    autograd against fp64 autograd on the CPU, worst entry, on warp_case's inputs; a case is kept only where it is at most 1e-4:
        C_, depth_rows    130 x 127 (65 blocks)    128 x 416 (208 blocks)
        1, 1              5.4e-6                   5.4e-5
        1, 3              1.0e-5                   3.4e-5
        3, 1              2.8e-6                   1.3e-5
        3, 3              2.9e-6                   2.9e-5
        5, 1              1.5e-5                   2.6e-5
        5, 3              1.0e-5                   2.9e-5"""
    imgs, depth, pose, K, g = warp_case(C_, depth_rows, shape)
    N, _, H, W = imgs.shape
    depth3 = depth if depth_rows == 3 else np.repeat(depth[:, None], 3, axis=1)
    ref = IG.autograd_warp(imgs, depth3, pose, K, g)
    args = [to_dev(a, dev) for a in (imgs, depth, pose, K, g)]
    before = ops.warp_bwd(*args, want_d_src=False)
    got = ops.warp_bwd_intrinsics(*args)
    after = ops.warp_bwd(*args, want_d_src=False)
    err = IG.worst(to_np(got), ref)
    note("INTRINSICS sfm_warp_intrinsics_bwd C=%d depth_rows=%d %dx%d: worst entry %.3g (tol %.0e)" % (C_, depth_rows, H, W, err, REF_TOL))
    assert err <= REF_TOL, err
    assert torch.equal(ops.warp_bwd_intrinsics(*args), got)                      # no atomics: bitwise repeatable
    for a, b in zip(before[:2], after[:2]):                                       # sfm_warp_bwd does not notice the call
        assert torch.equal(a, b)
    # ... and d_depth / d_pose still are what autograd says (the shared per-pixel code)
    if depth_rows == 3:
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        import test_oracle_vs_torch_cpu as T
        dp, po = t(depth3).requires_grad_(True), t(pose).requires_grad_(True)
        (T.projective_inverse_warp(t(imgs), dp, po, t(K)) * t(g)).sum().backward()
        assert np.abs(to_np(after[1]) - po.grad.numpy()).max() <= REF_TOL * np.abs(po.grad.numpy()).max()
        assert np.abs(to_np(after[0]) - dp.grad.numpy()).max() <= REF_TOL * np.abs(dp.grad.numpy()).max()


def test_pose_proj_bwd_intrinsics_is_the_closed_form(ops, dev):
    rng = np.random.RandomState(9)
    N = 70                                                                        # more than one block of 64
    pose = np.concatenate([rng.uniform(-3.5, 3.5, (N, 3)), rng.normal(0, 0.5, (N, 3))], axis=1).astype(np.float32)   # some angles clipped
    K = (np.eye(3) + 0.1 * rng.normal(size=(N, 3, 3))).astype(np.float32)
    g = rng.normal(size=(N, 4, 4)).astype(np.float32)
    got = ops.pose_proj_bwd_intrinsics(to_dev(pose, dev), to_dev(K, dev), to_dev(g, dev))
    err = IG.worst(to_np(got), IG.d_k_of_proj(pose, g))
    note("INTRINSICS sfm_pose_proj_bwd_k N=%d: worst entry %.3g (tol %.0e)" % (N, err, SELF_TOL))
    assert err <= SELF_TOL, err
    assert torch.equal(ops.pose_proj_bwd_intrinsics(to_dev(pose, dev), to_dev(K, dev), to_dev(g, dev)), got)
