"""The fused loss and the warp operator on GENERAL cameras and on images with exact zeros, against the CPU oracle.

Every other GPU test takes its intrinsics from synth.make_inputs: [[fx,0,cx],[0,fy,cy],[0,0,1]], scale s = scale 0 over 2**s, and
images without a single exact 0.  The C ABI accepts any invertible 3x3 per (sample, scale) and the kernels are written for one; K
enters at five code sites -- the main kernels (the FAST fold M = P K^-1), the reference-order chain, the second launch of d_src (which
re-projects), finalize_kernel (its own inverse, K^T gPm) and the warp operator.  tests/cameras.py makes the cameras (skew, a general
bottom row, unrelated scales, a scaled matrix, all together) and the zero regions; tests/test_oracle_vs_torch_cpu.py holds the oracle
against torch autograd on exactly these inputs and shows that a result with any one entry of K ignored would miss the criteria used
here by a factor of ten.  The criteria are those of tests/test_loss_gpu.py, unchanged."""
import ctypes as C

import numpy as np
import pytest

import cameras
from oracle import sfm_oracle as O
from test_loss_gpu import CONFIGS, _bind, _check_grads, _check_losses, _check_warped, _oracle, knife_widths
from test_oracle_vs_torch_cpu import zero_pixel_shares
from test_ops_gpu import check_warp_fwd_bwd, warp_inputs
from util import parity_note, parity_row, to_np

pytestmark = pytest.mark.gpu

SHAPES = list(cameras.CASES)
FAMILIES = {0: "base", 1: "wide", 2: "pair", 3: "ref", 4: "dsrc"}
_cache = {}


def case(synth, shape, kind, mode, zeros=False):
    """(inputs, fp32 oracle with d_src, callable -> fp64 oracle) of one case, computed once and shared (never modified)"""
    key = (tuple(shape), kind, mode, zeros)
    if key not in _cache:
        d = cameras.camera_inputs(synth, shape, kind, zeros=zeros)
        cfg = CONFIGS[mode]
        ref = _oracle(d, cfg, want_d_src=True)
        r64 = []

        def ref64():
            if not r64:
                r64.append(O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True,
                                      want_d_src=True, keep_warped=True, dtype=np.float64, **cfg))
            return r64[0]
        _cache[key] = (d, ref, ref64)
    return _cache[key]


def family(ops, fl, grad, loss):
    """the kernel family sfm_loss_plan_info reports for the bound descriptor and the entry point (include/sfmwarp.h)"""
    n = fl.desc.n_scales
    out = (C.c_int * (1 + 4 * n + 2))()
    ops.check(ops.lib.sfm_loss_plan_info(C.byref(fl.desc), grad, loss, out, len(out)))
    return out[1 + 4 * n]


def tag(shape, kind, mode, layout, projection, zeros=False):
    return "CAMERAS %s%s %s B=%d %dx%d %d src %s %s" % (kind or "canonical", " + exact zeros" if zeros else "", mode, shape[0], shape[1],
                                                        shape[2], shape[3], layout, projection)


def check_entry_points(ops, dev, synth, shape, kind, mode, layout, projection, entries, zeros=False):
    """The launches `entries` (of "forward", "backward", "forward_backward") of one case against the oracle: the five scalars at
    LOSS_RTOL, the warped pixels (FAST projection: 1e-4 + tap contrast x position uncertainty; reference order: the flat 1e-4), every
    gradient by _check_grads with the position-derived knife widths and the fp64 oracle on offer -- first with the warped output
    bound, then with d_src bound (another main kernel and the second launch, which re-projects).  Returns what it computed."""
    d, ref, ref64 = case(synth, shape, kind, mode, zeros)
    cfg, n_src = CONFIGS[mode], shape[3]
    what = tag(shape, kind, mode, layout, projection, zeros)
    flat = projection == "reference_order"
    masks = bool(cfg.get("exp_reg"))
    kw = dict(ref64=ref64, check_mask=masks, **knife_widths(d, ref))
    out = {}

    def grads(fl):
        return [to_np(t).copy() for t in fl.d_disps + fl.d_poses + (fl.d_masks or [])]

    fl = _bind(ops, dev, d, cfg, layout=layout, want_warped=True, projection=projection)
    fams = set()
    if "forward" in entries:
        _check_losses(fl.forward(), ref)
        _check_warped(fl, ref, what + " [sfm_loss_fwd]", d, flat=flat)
        fams.add(family(ops, fl, 0, 1))
    if "backward" in entries:
        fl.backward(1.0)
        _check_grads(fl, ref, n_src, what=what + " [sfm_loss_bwd]", **kw)
        fams.add(family(ops, fl, 1, 0))
    if "forward_backward" in entries:
        for t in fl.warped:
            t.fill_(7.0)
        _check_losses(fl.forward_backward(), ref)
        _check_warped(fl, ref, what + " [sfm_loss_fwd_bwd]", d, flat=flat)
        _check_grads(fl, ref, n_src, what=what + " [sfm_loss_fwd_bwd]", **kw)
        out["loss"], out["grads"] = to_np(fl.loss5).copy(), grads(fl)
        fams.add(family(ops, fl, 1, 1))
        # ... and without the optional outputs: the launch a training step makes (at these sizes the pair form for SSIM modes in the
        # pixel-interleaved layout, the wide form for L1 ones)
        fp = _bind(ops, dev, d, cfg, layout=layout, projection=projection)
        _check_losses(fp.forward_backward(), ref)
        _check_grads(fp, ref, n_src, what=what + " no optional output [sfm_loss_fwd_bwd]", **kw)
        fams.add(family(ops, fp, 1, 1))
    fs = _bind(ops, dev, d, cfg, layout=layout, want_d_src=True, projection=projection)
    if "backward" in entries:
        fs.backward(1.0)
        _check_grads(fs, ref, n_src, check_src=True, what=what + " with d_src [sfm_loss_bwd]", **kw)
        fams.add(family(ops, fs, 1, 0))
    if "forward_backward" in entries:
        _check_losses(fs.forward_backward(), ref)
        _check_grads(fs, ref, n_src, check_src=True, what=what + " with d_src [sfm_loss_fwd_bwd]", **kw)
        out["d_srcs"] = [to_np(t).copy() for t in fs.d_srcs]
        fams.add(family(ops, fs, 1, 1))
    parity_row(kind="cameras", case=what, camera=kind or "canonical", zeros=zeros, families=sorted(FAMILIES[f] for f in fams))
    return out


def same_to_ulps(a, b):
    """two instantiations of one template (tests/test_loss_gpu.py: test_hwc_layout_gives_the_planar_results)"""
    np.testing.assert_allclose(b["loss"], a["loss"], rtol=2e-7, atol=0)
    for x, y in zip(a["grads"] + a["d_srcs"], b["grads"] + b["d_srcs"]):
        assert x.shape == y.shape
        np.testing.assert_allclose(y, x, rtol=0, atol=2e-5 * max(np.abs(x).max(), 1e-30))


@pytest.mark.parametrize("projection", ["fast", "reference_order"])
@pytest.mark.parametrize("mode", cameras.MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_general_cameras_every_entry_point_layout_and_projection(ops, synth, dev, shape, mode, projection):
    """Skew, a general bottom row and unrelated scales TOGETHER: the three entry points in both layouts and both projections, with
    the warped output, the explainability masks and d_src -- and the pixel-interleaved layout returns what the planar one does."""
    outs = {layout: check_entry_points(ops, dev, synth, shape, "general", mode, layout, projection,
                                       ("forward", "backward", "forward_backward")) for layout in ("planar", "hwc")}
    same_to_ulps(outs["planar"], outs["hwc"])


@pytest.mark.parametrize("projection", ["fast", "reference_order"])
@pytest.mark.parametrize("kind", ["skew", "bottom", "per_scale", "scaled"])
@pytest.mark.parametrize("shape", SHAPES)
def test_single_camera_kinds(ops, synth, dev, shape, kind, projection):
    """One departure from the canonical K at a time (so that a failure names the entries), each in the loss mode cameras.MODE_OF
    gives it: sfm_loss_fwd_bwd in both layouts and both projections, warped output and d_src included."""
    outs = {layout: check_entry_points(ops, dev, synth, shape, kind, cameras.MODE_OF[kind], layout, projection, ("forward_backward",))
            for layout in ("planar", "hwc")}
    same_to_ulps(outs["planar"], outs["hwc"])


def test_every_kernel_family_runs_on_a_general_camera(ops, synth, dev):
    """The fused loss has five families of main kernels (sfm_loss_plan_info: 0 base, 1 wide, 2 pair, 3 reference order, 4 d_src),
    each with its own copy of the geometry set-up.  One launch of each on the general cameras, the family read from the plan, the
    result against the oracle; the pair form also through the one-call hook against the one-source form (same loss to 2e-7, same
    gradients to 2e-5 of their maximum)."""
    shape = SHAPES[0]
    n_src = shape[3]
    launches = [      # (mode, layout, bind arguments, the family the planner is expected to choose at this size)
        ("explain", "hwc", dict(), 0),
        ("l1", "planar", dict(), 1),
        ("ssim_smooth", "hwc", dict(), 2),
        ("ssim_smooth", "hwc", dict(projection="reference_order"), 3),
        ("edge_aware", "hwc", dict(want_d_src=True), 4),
    ]
    seen = set()
    for mode, layout, kw, expected in launches:
        d, ref, ref64 = case(synth, shape, "general", mode)
        cfg = CONFIGS[mode]
        fl = _bind(ops, dev, d, cfg, layout=layout, **kw)
        fam = family(ops, fl, 1, 1)
        what = "CAMERAS general, family %s: %s %s" % (FAMILIES[fam], mode, layout)
        ck = dict(what=what, ref64=ref64, check_mask=bool(cfg.get("exp_reg")), check_src=bool(kw.get("want_d_src")), **knife_widths(d, ref))
        if expected == 2:
            outs = {}
            for variant in (4, 5):
                loss = to_np(fl.forward_backward(variant=variant)).copy()
                outs[variant] = (loss, [to_np(t).copy() for t in fl.d_disps + fl.d_poses])
            np.testing.assert_allclose(outs[5][0], outs[4][0], rtol=2e-7, atol=0)
            for a, b in zip(outs[4][1], outs[5][1]):
                np.testing.assert_allclose(b, a, rtol=0, atol=2e-5 * max(np.abs(a).max(), 1e-30))
            _check_losses(fl.forward_backward(variant=5), ref)
            _check_grads(fl, ref, n_src, **dict(ck, what=what + " [sfm_loss_variant(5)]"))
        _check_losses(fl.forward_backward(), ref)
        _check_grads(fl, ref, n_src, **ck)
        assert fam == expected, "%s %s: the planner chose family %s, not %s" % (mode, layout, FAMILIES[fam], FAMILIES[expected])
        seen.add(fam)
    parity_note("CAMERAS general: kernel families that ran: %s" % sorted(FAMILIES[f] for f in seen))
    assert seen == set(FAMILIES), sorted(seen)


@pytest.mark.parametrize("mode", ["l1", "ssim_smooth", "edge_aware", "explain"])
@pytest.mark.parametrize("kind", cameras.KINDS)
def test_header_read_from_the_struct_gives_the_same_bits_on_general_cameras(ops, synth, dev, kind, mode):
    """test_loss_gpu.test_header_read_from_the_struct_gives_the_same_bits, whatever K is: sfm_loss_variant(3) changes where the
    kernels read their header from, nothing else -- every output bit for bit."""
    d, _, _ = case(synth, SHAPES[1], kind, mode)
    outs = []
    for forced in (False, True):
        fl = _bind(ops, dev, d, CONFIGS[mode], layout="hwc")
        hook = (lambda: ops.check(ops.lib.sfm_loss_variant(3))) if forced else (lambda: None)
        hook()
        l_fwd = to_np(fl.forward()).copy()
        hook()
        l_both = to_np(fl.forward_backward()).copy()
        g_both = [to_np(t).copy() for t in fl.d_disps + fl.d_poses + (fl.d_masks or [])]
        hook()
        fl.backward(1.0)
        outs.append([l_fwd, l_both] + g_both + [to_np(t).copy() for t in fl.d_disps + fl.d_poses + (fl.d_masks or [])])
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("kind", cameras.KINDS)
def test_batch_shard_is_additive_on_general_cameras(ops, synth, dev, kind):
    """test_loss_gpu.test_batch_shard_is_additive with a camera of its own per sample and scale: a shard (norm_B = the global
    batch) sees ITS samples' cameras -- the shard losses add up to the full batch's, the per-sample gradients are the full batch's."""
    shape = SHAPES[2]                      # B = 9: shards of 4 and 5
    cfg = CONFIGS["ssim_smooth"]
    d, _, _ = case(synth, shape, kind, "ssim_smooth")
    B, S, n_src = shape[0], shape[4], shape[3]
    full = _bind(ops, dev, d, cfg)
    lf = to_np(full.forward_backward()).astype(np.float64)
    tot = np.zeros(5)
    for sl in (slice(0, 4), slice(4, 9)):
        part = dict(d, tgt_pyr=[a[sl] for a in d["tgt_pyr"]], src_pyr=[a[sl] for a in d["src_pyr"]], intrinsics=d["intrinsics"][sl],
                    disps=[a[sl] for a in d["disps"]], poses=[a[sl] for a in d["poses"]], masks=None)
        sh = _bind(ops, dev, part, cfg, norm_B=B)
        tot += to_np(sh.forward_backward()).astype(np.float64)
        for s in range(S):
            np.testing.assert_allclose(to_np(sh.d_disps[s]), to_np(full.d_disps[s])[sl], rtol=1e-5, atol=1e-10)
        for i in range(n_src):
            np.testing.assert_allclose(to_np(sh.d_poses[i]), to_np(full.d_poses[i])[sl], rtol=1e-5, atol=1e-10)
    np.testing.assert_allclose(tot, lf, rtol=1e-5)


@pytest.mark.parametrize("depth_rows", [1, 3])
@pytest.mark.parametrize("texture", ["smooth", "noise"])
@pytest.mark.parametrize("kind", ["skew", "bottom", "scaled", "general"])
@pytest.mark.parametrize("shape", [(2, 3, 16, 52), (1, 3, 37, 70)])
def test_projective_inverse_warp_on_general_cameras(ops, synth, dev, shape, kind, texture, depth_rows):
    """sfm_warp_fwd / _bwd (test_ops_gpu.test_projective_inverse_warp_fwd_bwd: the same inputs, the same assertions) with the
    intrinsics of cameras.cameras: 1e-4 at every warped pixel with no exclusion, the oracle's zero set, the backward's criteria."""
    check_warp_fwd_bwd(ops, dev, warp_inputs(synth, shape, texture, depth_rows, kind), shape, "%s K=%s" % (texture, kind), depth_rows)


@pytest.mark.parametrize("projection", ["fast", "reference_order"])
@pytest.mark.parametrize("layout", ["planar", "hwc"])
@pytest.mark.parametrize("mode", ["l1", "ssim_smooth", "edge_aware", "explain"])
@pytest.mark.parametrize("kind", [None, "general"])
def test_exact_zero_pixels(ops, synth, dev, kind, mode, layout, projection):
    """The zero mask of models/base_model.py:96 -- a warped pixel whose three channels are exactly 0 takes no part in the loss -- on
    samples that are IN VIEW (synth keeps every value away from 0, so every other test only meets it out of view): a rectangle of
    zeros in all channels of the target and the sources, next to regions with ONE zero channel in the sources (channel 1) and in the
    target (channel 2), which must not be masked.  From the oracle: at least 3 % of the pixels of every scale are in view and masked,
    none of them where only one channel is zero.  Then loss, warped pixels (zero sets included) and every gradient, d_src and d_mask
    among them, with synth's cameras and with the general ones."""
    shape = SHAPES[0]
    d, ref, _ = case(synth, shape, kind, mode, zeros=True)
    _, rect, one_src, one_tgt = cameras.zero_regions(d)
    shares = zero_pixel_shares(d, ref, one_src, one_tgt)
    parity_note("exact zeros %s %s: in view and masked %s %% of the pixels per scale" % (kind or "canonical", mode, ["%.1f" % (100 * x) for x in shares]))
    assert min(shares) >= 0.03, shares
    check_entry_points(ops, dev, synth, shape, kind, mode, layout, projection, ("forward_backward",), zeros=True)
