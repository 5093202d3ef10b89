"""sfm_warp_pyramid_fwd / _bwd and torch_api.warp_pyramid on the GPU: all scales and sources of a step warped in one launch and
differentiated in one launch plus a fold.  The parent's operators -- ops.warp_fwd / ops.warp_bwd, one (scale, source) per call --
are the reference: the forward bit for bit, d_disp to a bound counted in roundings, d_pose against fp64 autograd no worse than
the per-call route.  No pixel is excluded anywhere.

Shapes (B, H, W, n_src, S), with the 256-pixel blocks per image of every scale.  warp_pyr_fold_kernel adds the block sums of
one (sample, source, scale) with one wave, lane l taking blocks l, l + 64, ...: only the last shape leaves the first trip of that loop.
  (2, 24, 40, 1, 3)    4, 1, 1 blocks   a last scale of 6 x 10 = 60 pixels: less than one wave, one source
  (2, 20, 52, 3, 2)    5, 2 blocks      1040 pixels = four full blocks + 16, an odd source count
  (3, 16, 52, 4, 1)    4 blocks         four sources, one scale, B = 3
  (2, 130, 127, 2, 2)  65, 16 blocks    16510 pixels: lane 0 goes round a second time, for a last block of 126 pixels; scale 1 is
                                        65 x 63 = 4095 pixels, one short of 16 full blocks; a second sample and a second source,
                                        so that the offsets of both are taken with more than 64 blocks
The first three with synth's default motion and with rot_sigma = 0.3, trans_sigma = 0.5 (samples out of view and behind the camera),
the last with the default motion; the second and the last also with general cameras (tests/cameras.py), so that scale s reads its
own K.  tests/test_fold_rounds_cpu.py pins the block counts and shows that the fp64 reference of d_pose moves by far more than the
tolerances here when the pixels beyond the first 64 blocks are left out."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import cameras
from util import GUARD_MIN_BYTES, SENTINEL, Arena, parity_note

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

SHAPES = [(2, 24, 40, 1, 3), (2, 20, 52, 3, 2), (3, 16, 52, 4, 1), (2, 130, 127, 2, 2)]
FOLD_SHAPE = SHAPES[3]                             # more than 64 blocks at scale 0
LARGE = dict(rot_sigma=0.3, trans_sigma=0.5)
CASES = [(shape, motion, None) for shape in SHAPES[:3] for motion in ("default", "large")] + [(SHAPES[1], "default", "general")]
FOLD_CASES = [(FOLD_SHAPE, "default", None), (FOLD_SHAPE, "default", "general")]
CASES += FOLD_CASES                                # (appended: the tests below name earlier cases by index)
IDS = ["%s-%s%s" % ("x".join(map(str, s)), m, "-" + k if k else "") for s, m, k in CASES]
F64 = np.float64
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _needs_a_gpu(dev):
    """(the `dev` fixture skips where no GPU is visible)"""


def _bits(a, b):
    """bitwise equality of two float tensors (NaN payloads and the sign of zero included)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    return torch.equal(a.detach().contiguous().view(it), b.detach().contiguous().view(it))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def host_case(shape, motion, kind):
    """the inputs of one case on the host (never modify them): synth's arrays `d` and the upstream gradients `g`"""
    B, H, W, n, S = shape
    seed = 11 + SHAPES.index(shape)
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n, n_scales=S, seed=seed, **(LARGE if motion == "large" else {}))
    d = cameras.with_cameras(d, kind, 1000 + seed)
    gen = torch.Generator().manual_seed(100 + seed)
    return dict(d=d, shape=shape, g=[torch.randn((B, n, 3, H >> s, W >> s), generator=gen) for s in range(S)])


@functools.lru_cache(maxsize=None)
def case(shape, motion, kind):
    """Everything the tests of one case share, computed once (never modify it): the inputs, the new route's outputs in both
    layouts, and the parent's per-(scale, source) operators on the same inputs."""
    B, H, W, n, S = shape
    h = host_case(shape, motion, kind)
    d = h["d"]
    x = dict(d=d, shape=shape, planar=[_t(a) for a in d["src_pyr"]], disps=[_t(a) for a in d["disps"]], poses=[_t(a) for a in d["poses"]],
             K=_t(d["intrinsics"]))
    x["hwc"] = [ops.to_hwc(a) for a in x["planar"]]
    x["g"] = [g.to(DEV) for g in h["g"]]
    for layout in ("planar", "hwc"):
        x["warped_" + layout], x["valid_" + layout] = ops.warp_pyramid_fwd(x[layout], x["disps"], x["poses"], x["K"], layout, want_valid=True)
        x["bwd_" + layout] = ops.warp_pyramid_bwd(x[layout], x["disps"], x["poses"], x["K"], layout, x["g"])
    # the parent's route: one call per (scale, source), depth = 1 / disp in torch
    x["ref_warped"], x["ref_d_depth"], x["ref_d_pose"] = {}, {}, {}
    for s in range(S):
        depth = (1 / x["disps"][s]).view(B, -1)
        for i in range(n):
            src = x["planar"][s][:, 3 * i:3 * i + 3]
            x["ref_warped"][s, i] = ops.warp_fwd(src, depth, x["poses"][i], x["K"][:, s])
            dd, dp, _ = ops.warp_bwd(src, depth, x["poses"][i], x["K"][:, s], x["g"][s][:, i].contiguous())
            x["ref_d_depth"][s, i], x["ref_d_pose"][s, i] = dd.view(B, 1, H >> s, W >> s), dp
    torch.cuda.synchronize()
    return x


# ------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,motion,kind", CASES, ids=IDS)
def test_forward_is_the_operator_bit_for_bit_in_both_layouts(shape, motion, kind):
    x = case(shape, motion, kind)
    B, H, W, n, S = shape
    seen = torch.zeros(2)
    for s in range(S):
        wp, wh, vp, vh = x["warped_planar"][s], x["warped_hwc"][s], x["valid_planar"][s], x["valid_hwc"][s]
        assert tuple(wp.shape) == (B, n, 3, H >> s, W >> s) and tuple(vp.shape) == (B, n, H >> s, W >> s)
        assert _bits(wp, wh) and _bits(vp, vh), s
        for i in range(n):
            assert _bits(wp[:, i], x["ref_warped"][s, i]), (s, i)
        # no operator hands out the grid test itself: the mask holds only 0 and 1, and 0 means that all three channels are exactly 0
        assert bool(((vp == 0) | (vp == 1)).all())
        assert bool((wp[(vp == 0)[:, :, None].expand_as(wp)] == 0).all()), s
        seen += torch.tensor([float((vp == 0).sum()), float((vp == 1).sum())])
    # a few pixels of synth's default motion leave the frame, most stay; the large motion throws whole regions out -- both values occur
    assert seen[1] > 0 and (seen[0] > 0 if motion == "large" else seen[1] > seen[0]), seen


def test_forward_without_the_mask_and_the_backward_fields(dev):
    """want_valid=False binds no valid[] and, like every forward, none of the backward's fields: the same warped bits"""
    x = case(*CASES[2])
    for layout in ("planar", "hwc"):
        out = ops.warp_pyramid_fwd(x[layout], x["disps"], x["poses"], x["K"], layout)
        assert all(_bits(a, b) for a, b in zip(out, x["warped_planar"]))


# ------------------------------------------------------------------------------------------------------------------------
# 2. d_disp
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,motion,kind", CASES, ids=IDS)
def test_d_disp_within_its_counted_roundings(shape, motion, kind):
    """ref = -(sum_i d_depth_i) / disp^2 in fp64 from the parent's per-source d_depth; |got - ref| <= 8 * 2^-24 * (sum_i |d_depth_i|) / disp^2:
    n_src - 1 <= 3 adds, one multiply and one divide at half an ulp each, rounded up"""
    x = case(shape, motion, kind)
    B, H, W, n, S = shape
    assert all(_bits(a, b) for a, b in zip(x["bwd_planar"][0], x["bwd_hwc"][0]))
    for s in range(S):
        got = x["bwd_planar"][0][s].cpu().numpy().astype(F64)
        disp = x["disps"][s].cpu().numpy().astype(F64)
        dd = np.stack([x["ref_d_depth"][s, i].cpu().numpy().astype(F64) for i in range(n)])
        ref = -dd.sum(axis=0) / disp ** 2
        bound = 8 * 2.0 ** -24 * np.abs(dd).sum(axis=0) / disp ** 2
        err = np.abs(got - ref)
        assert got.shape == (B, 1, H >> s, W >> s) and np.isfinite(got).all()
        parity_note("warp_pyramid d_disp %s scale %d: worst |got - ref| / bound = %.3g" % (IDS[CASES.index((shape, motion, kind))], s,
                                                                                        float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), (s, float((err - bound).max()))
        dead = (x["valid_planar"][s] == 0).all(dim=1, keepdim=True).cpu().numpy()
        assert (got[dead] == 0).all(), s


# ------------------------------------------------------------------------------------------------------------------------
# 3. d_pose
# ------------------------------------------------------------------------------------------------------------------------
def _autograd_d_pose(x, first_pixels=None):
    """fp64 autograd of the torch restatement of projective_inverse_warp (tests/test_oracle_vs_torch_cpu.py, switched to fp64 the way
    tests/intrinsics_grad.py::autograd_warp does), summed over the scales: d_pose per source.  x: a case or a host_case.
    first_pixels: the upstream gradient counts only on pixels j < first_pixels of every image (tests/test_fold_rounds_cpu.py)"""
    import test_oracle_vs_torch_cpu as T
    d = x["d"]
    B, H, W, n, S = x["shape"]
    saved = T.DT
    T.DT = torch.float64
    try:
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))
        poses = [t(a).requires_grad_(True) for a in d["poses"]]
        total = 0
        for s in range(S):
            depth = (1.0 / t(d["disps"][s])).reshape(B, 1, -1).expand(B, 3, -1)
            for i in range(n):
                out = T.projective_inverse_warp(t(d["src_pyr"][s][:, 3 * i:3 * i + 3]), depth, poses[i], t(d["intrinsics"][:, s]))
                g = x["g"][s][:, i].cpu().numpy().astype(F64)
                if first_pixels is not None:
                    g.reshape(B, 3, -1)[:, :, first_pixels:] = 0
                total = total + (out * t(g)).sum()
        total.backward()
    finally:
        T.DT = saved
    return [p.grad.numpy().astype(F64) for p in poses]


@pytest.mark.parametrize("shape,motion,kind", CASES, ids=IDS)
def test_d_pose_no_worse_than_the_per_call_route(shape, motion, kind):
    """A = the parent's route (sum over the scales, in fp64 on the host, of ops.warp_bwd's d_pose), B = fp64 autograd.  Both routes
    add bit-identical per-pixel terms, only the order of the fp32 partial sums differs: E_new <= 1.5 E_old + 2e-6 (2e-6: about 32
    fp32 ulps, for an E_old that happens to be tiny); in-view decisions that fp64 takes differently are common to both sides.
    And max |new - A| <= 1e-5 max |A|, the bound include/sfmwarp.h states for reference-order arithmetic."""
    x = case(shape, motion, kind)
    B, H, W, n, S = shape
    ref_b = _autograd_d_pose(x)
    assert all(_bits(a, b) for a, b in zip(x["bwd_planar"][1], x["bwd_hwc"][1]))
    for i in range(n):
        new = x["bwd_planar"][1][i].cpu().numpy().astype(F64)
        a = sum(x["ref_d_pose"][s, i].cpu().numpy().astype(F64) for s in range(S))
        assert new.shape == (B, 6) and np.isfinite(new).all()
        scale = np.abs(ref_b[i]).max()
        if scale == 0:      # a source that is nowhere in view, in fp64 as in fp32 (the large motion has two): exactly zero on every route
            assert motion == "large" and not new.any() and not a.any(), i
            parity_note("warp_pyramid d_pose %s source %d: nowhere in view, d_pose exactly 0" % (IDS[CASES.index((shape, motion, kind))], i))
            continue
        e_new, e_old = np.abs(new - ref_b[i]).max() / scale, np.abs(a - ref_b[i]).max() / scale
        self_err = np.abs(new - a).max() / np.abs(a).max()
        parity_note("warp_pyramid d_pose %s source %d: E_new %.3g E_old %.3g |new - A| / max|A| %.3g"
                    % (IDS[CASES.index((shape, motion, kind))], i, e_new, e_old, self_err))
        assert e_new <= 1.5 * e_old + 2e-6, (i, e_new, e_old)
        assert self_err <= 1e-5, (i, self_err)


# ------------------------------------------------------------------------------------------------------------------------
# 4. determinism and buffers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,which", [("planar", 3), ("hwc", 3), ("planar", CASES.index(FOLD_CASES[1])), ("hwc", CASES.index(FOLD_CASES[1]))],
                         ids=["planar", "hwc", "planar-65_blocks", "hwc-65_blocks"])
def test_two_backward_calls_agree_bit_for_bit(layout, which):
    x = case(*CASES[which])
    d_disps, d_poses = ops.warp_pyramid_bwd(x[layout], x["disps"], x["poses"], x["K"], layout, x["g"])
    for a, b in zip(d_disps + d_poses, x["bwd_" + layout][0] + x["bwd_" + layout][1]):
        assert _bits(a, b)


@pytest.mark.parametrize("layout,res,which", [("planar", 0, 2), ("hwc", 4, 2), ("hwc", 12, 2), ("hwc", 4, CASES.index(FOLD_CASES[0]))],
                         ids=["planar-0", "hwc-4", "hwc-12", "hwc-4-65_blocks"])
def test_buffer_contract(dev, layout, res, which):
    """every output pre-filled with the sentinel is overwritten completely, inputs are only read, and the guard bands around warped,
    valid, d_disp, d_pose and the workspace stay as they were; placed at `res` bytes off a 16-byte boundary.  The workspace starts
    out as NaN sentinels: a fold that reads a block sum nobody wrote (the 65-block case takes its second trip) gives a NaN d_pose"""
    x = case(*CASES[which])
    B, H, W, n, S = x["shape"]
    hw = [(H >> s, W >> s) for s in range(S)]
    d = _lib.SfmWarpPyramidDesc()
    d.B, d.n_src, d.n_scales, d.image_layout = B, n, S, ops._LAYOUTS[layout]
    specs = [("K", (B, S, 3, 3), res)] + [("pose%d" % i, (B, 6), res) for i in range(n)] + [("d_pose%d" % i, (B, 6), res) for i in range(n)]
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
        specs += [("src%d" % s, tuple(x[layout][s].shape), res), ("disp%d" % s, (B, 1, h, w), res), ("g%d" % s, (B, n, 3, h, w), res),
                  ("warped%d" % s, (B, n, 3, h, w), res), ("valid%d" % s, (B, n, h, w), res), ("d_disp%d" % s, (B, 1, h, w), res)]
    for s in range(S):
        d.src[s] = d.disp[s] = d.g_warped[s] = d.d_disp[s] = 0x1000       # placeholders for the query: never dereferenced
    for i in range(n):
        d.pose[i] = d.d_pose[i] = 0x1000
    d.intrinsics = 0x1000
    nbytes = _lib.lib.sfm_warp_pyramid_bwd_workspace_bytes(C.byref(d))
    assert nbytes > 0 and nbytes % 256 == 0
    arena = Arena(dev, specs + [("ws", nbytes, "ws")], row_floats=3 * W)
    assert arena.guard >= GUARD_MIN_BYTES
    inputs = [("K", x["K"])] + [("pose%d" % i, x["poses"][i]) for i in range(n)]
    for s in range(S):
        inputs += [("src%d" % s, x[layout][s]), ("disp%d" % s, x["disps"][s]), ("g%d" % s, x["g"][s])]
    for name, a in inputs:
        arena.set(name, a)
        arena.snapshot(name)
    d.intrinsics = arena.ptr("K")
    for i in range(n):
        d.pose[i], d.d_pose[i] = arena.ptr("pose%d" % i), arena.ptr("d_pose%d" % i)
    for s in range(S):
        d.src[s], d.disp[s], d.g_warped[s] = arena.ptr("src%d" % s), arena.ptr("disp%d" % s), arena.ptr("g%d" % s)
        d.warped[s], d.valid[s], d.d_disp[s] = arena.ptr("warped%d" % s), arena.ptr("valid%d" % s), arena.ptr("d_disp%d" % s)
    outs = ["d_pose%d" % i for i in range(n)] + ["%s%d" % (k, s) for s in range(S) for k in ("warped", "valid", "d_disp")]
    assert all(arena.sentinels_left(o) == arena.nbytes(o) // 4 for o in outs) and arena.sentinels_left("ws") == nbytes // 4
    ops._launch(dev, _lib.lib.sfm_warp_pyramid_fwd, C.byref(d))
    ops._launch(dev, _lib.lib.sfm_warp_pyramid_bwd, C.byref(d), C.c_void_p(arena.ptr("ws")), nbytes)
    for o in outs:
        assert arena.sentinels_left(o) == 0, o
    arena.check("sfm_warp_pyramid_fwd / _bwd (%s)" % layout)
    for name, _ in inputs:
        arena.unchanged(name)
    as_bits = lambda t: t.contiguous().view(torch.int32).cpu().numpy()
    for s in range(S):
        np.testing.assert_array_equal(arena.bits("warped%d" % s), as_bits(x["warped_" + layout][s]))
        np.testing.assert_array_equal(arena.bits("valid%d" % s), as_bits(x["valid_" + layout][s]))
        np.testing.assert_array_equal(arena.bits("d_disp%d" % s), as_bits(x["bwd_" + layout][0][s]))
    for i in range(n):
        np.testing.assert_array_equal(arena.bits("d_pose%d" % i), as_bits(x["bwd_" + layout][1][i]))
    assert SENTINEL == 0x7FA5A5A5


# ------------------------------------------------------------------------------------------------------------------------
# 5. autograd
# ------------------------------------------------------------------------------------------------------------------------
def _torch_inputs(shape, seed=5):
    B, H, W, n, S = shape
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n, n_scales=S, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    return dict(src=_t(d["src"]), K=_t(d["intrinsics"]), disps=[_t(a).requires_grad_() for a in d["disps"]],
                packed=_t(np.concatenate(d["poses"], axis=1)).requires_grad_(),
                w=[torch.randn((B, n, 3, H >> s, W >> s), generator=gen).to(DEV) for s in range(S)])


def _loss(x, disps=None, packed=None, **kw):
    out = ta.warp_pyramid(x["src"], x["K"], x["disps"] if disps is None else disps, x["packed"] if packed is None else packed, **kw)
    warped = out[0] if kw.get("return_valid") else out
    return sum((w * a).sum() for w, a in zip(x["w"], warped)), out


def _expected(x):
    B, n, _, H, W = x["src"].shape
    S = len(x["disps"])
    pyr = ops.pyramid_hwc(x["src"].view(B, 3 * n, H, W), S)
    poses = [x["packed"].detach()[:, 6 * i:6 * i + 6].contiguous() for i in range(n)]
    disps = [t.detach() for t in x["disps"]]
    warped, valid = ops.warp_pyramid_fwd(pyr, disps, poses, x["K"], "hwc", want_valid=True)
    d_disps, d_poses = ops.warp_pyramid_bwd(pyr, disps, poses, x["K"], "hwc", x["w"])
    return warped, valid, d_disps, torch.cat(d_poses, dim=1)


def test_autograd_gives_the_operators_bits():
    x = _torch_inputs(SHAPES[1])
    warped, valid, d_disps, d_packed = _expected(x)
    total, (got, got_valid) = _loss(x, return_valid=True)
    assert len(got) == len(got_valid) == len(warped)
    for a, b, va, vb in zip(got, warped, got_valid, valid):
        assert a.requires_grad and not va.requires_grad and _bits(a, b) and _bits(va, vb)
    total.backward()
    for t, w in zip(x["disps"], d_disps):
        assert _bits(t.grad, w)
    assert _bits(x["packed"].grad, d_packed)
    # a list of poses instead of the packed tensor, and a scale the loss does not use: its upstream gradient is None -> zeros
    poses = [x["packed"].detach()[:, 6 * i:6 * i + 6].clone().requires_grad_() for i in range(3)]
    disps = [t.detach().clone().requires_grad_() for t in x["disps"]]
    out = ta.warp_pyramid(x["src"], x["K"], disps, poses)
    (x["w"][1] * out[1]).sum().backward()
    pyr = ops.pyramid_hwc(x["src"].view(2, 9, 20, 52), 2)
    e_disps, e_poses = ops.warp_pyramid_bwd(pyr, [t.detach() for t in disps], [t.detach() for t in poses], x["K"], "hwc",
                                            [torch.zeros_like(x["w"][0]), x["w"][1]])
    assert all(_bits(t.grad, w) for t, w in zip(disps + poses, e_disps + e_poses))
    assert bool((disps[0].grad == 0).all())
    # without a gradient required nothing is recorded
    with torch.no_grad():
        assert not ta.warp_pyramid(x["src"], x["K"], x["disps"], x["packed"])[0].requires_grad


def test_bf16_predictions_get_bf16_gradients():
    x = _torch_inputs(SHAPES[0])
    d16 = [t.detach().to(torch.bfloat16).requires_grad_() for t in x["disps"]]
    p16 = x["packed"].detach().to(torch.bfloat16).requires_grad_()
    _loss(x, d16, p16)[0].backward()
    d32 = [t.detach().float().requires_grad_() for t in d16]
    p32 = p16.detach().float().requires_grad_()
    _loss(x, d32, p32)[0].backward()
    for a, b in zip(d16 + [p16], d32 + [p32]):
        assert a.grad.dtype == torch.bfloat16 and _bits(a.grad, b.grad.to(torch.bfloat16))


def test_the_example_of_integration_md_trains():
    """INTEGRATION.md, 'Your own loss on the library's warp': a per-pixel minimum over the sources on warp_pyramid's output gives
    a finite loss and finite, non-zero gradients, without a host sync"""
    x = _torch_inputs(SHAPES[1])
    tgt_img = _t(synth.make_inputs(B=2, H=20, W=52, n_src=3, n_scales=2, seed=5)["tgt"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        warped, valid = ta.warp_pyramid(x["src"], x["K"], x["disps"], x["packed"], return_valid=True)
        total = 0.0
        for s, (w, v) in enumerate(zip(warped, valid)):
            tgt = ta.resize_images(tgt_img, w.shape[3:])
            err = (w - tgt[:, None]).abs().mean(2)
            err = torch.where(v > 0, err, torch.full_like(err, float("inf")))
            best = err.min(1).values
            seen = torch.isfinite(best)
            total = total + torch.where(seen, best, torch.zeros_like(best)).sum() / seen.sum().clamp(min=1) / 2 ** s
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(total)) and float(total) > 0
    for t in x["disps"] + [x["packed"]]:
        assert bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any())


def test_intrinsics_that_require_grad_are_refused():
    x = _torch_inputs(SHAPES[0])
    with pytest.raises(TypeError, match="projective_inverse_warp"):
        ta.warp_pyramid(x["src"], x["K"].clone().requires_grad_(), x["disps"], x["packed"])


def test_graph_capture_replays_bitwise():
    x = _torch_inputs(SHAPES[1], seed=6)
    y = _torch_inputs(SHAPES[1], seed=7)
    y["w"] = x["w"]                            # (constants of the captured loss)
    leaves = lambda z: z["disps"] + [z["packed"]]
    static = [x["src"], x["K"]] + [t.detach() for t in leaves(x)]

    def run(z):
        total, out = _loss(z)
        total.backward()
        return out

    def clear(z):
        for t in leaves(z):
            t.grad = None

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x)
        clear(x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(x)
    grads = [t.grad for t in leaves(x)]
    with torch.no_grad():
        for dst, src in zip(static, [y["src"], y["K"]] + leaves(y)):
            dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    want = run(y)
    assert all(_bits(a, b) for a, b in zip(out, want))
    assert all(_bits(a, t.grad) for a, t in zip(grads, leaves(y)))
    del g
