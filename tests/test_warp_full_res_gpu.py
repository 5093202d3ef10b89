"""sfm_warp_full_res_fwd / _bwd, torch_api.warp_full_res and min_reprojection_loss(full_res=True) on the GPU: the disparity of every
scale upsampled to the full resolution inside the warp of the full-resolution sources.  The definition of
include/sfmwarp_full_res.h is the reference, bit for bit: ops.resize of each disparity (skipped at equal sizes) ->
ops.warp_pyramid_fwd / _bwd at equal sizes with one camera -> ops.resize_bwd of each d_disp.

Shapes (tests/warp_full_res_ref.py), the smallest at which each loop can go wrong, each with 1 and 3 sources:
  24x40    disparities 24x40, 12x20, 6x10, 3x5      halvings; 4 blocks of 256 pixels per image, the last of 192
  13x21    13x21, 7x10, 1x1                         non-integer ratios; one row and column: a step of 0; 2 blocks, the last of 17
  130x127  130x127, 65x63, 17x9, B = 2              65 blocks per image: the fold's lane 0 goes round a second time
and 24x40 with three sources once more on a general 3x3 camera (tests/cameras.py)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import cameras
import warp_full_res_ref as R
from test_disp_smooth_cpu import rule
from util import GUARD_MIN_BYTES, SENTINEL, Arena, parity_note

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
BATCH = {"24x40": 2, "13x21": 2, "130x127": 2}
CASES = [(name, n, None) for name in R.SHAPES for n in (1, 3)] + [("24x40", 3, "general")]
IDS = ["%s-%dsrc%s" % (name, n, "-" + k if k else "") for name, n, k in CASES]
LAYOUTS = ("planar", "hwc")


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
def host_case(name, n_src, kind):
    """the inputs of one case on the host (never modify them): synth's full-resolution frames, camera and poses, a disparity of
    every size in DispNet's range, and the upstream gradients"""
    (H, W), hw = R.SHAPES[name]
    B, seed = BATCH[name], 31 + 7 * list(R.SHAPES).index(name) + n_src
    d = cameras.with_cameras(synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=1, seed=seed), kind, 1000 + seed)
    rng = np.random.RandomState(seed)
    disps = [(10.0 / (1.0 + np.exp(-1.5 * rng.uniform(-1, 1, (B, 1, h, w)))) + 0.01).astype(F32) for h, w in hw]
    gen = torch.Generator().manual_seed(100 + seed)
    return dict(src=d["src_pyr"][0], K=d["intrinsics"][:, 0], poses=d["poses"], disps=disps, B=B, H=H, W=W, hw=hw, n_src=n_src,
                g=[torch.randn((B, n_src, 3, H, W), generator=gen) for _ in hw])


@functools.lru_cache(maxsize=None)
def case(name, n_src, kind):
    """Everything the tests of one case share, computed once (never modify it): the inputs, the new calls' outputs in both layouts,
    and the definition run through the existing operators"""
    h = host_case(name, n_src, kind)
    B, H, W, hw = h["B"], h["H"], h["W"], h["hw"]
    S = len(hw)
    x = dict(h, planar=_t(h["src"]), K=_t(h["K"]), poses=[_t(a) for a in h["poses"]], disps=[_t(a) for a in h["disps"]], g=[g.to(DEV) for g in h["g"]])
    x["hwc"] = ops.to_hwc(x["planar"])
    for layout in LAYOUTS:
        x["fwd_" + layout] = ops.warp_full_res_fwd(x[layout], x["disps"], x["poses"], x["K"], layout, want_valid=True)
        x["bwd_" + layout] = ops.warp_full_res_bwd(x[layout], x["disps"], x["poses"], x["K"], layout, x["g"])
    # the definition: resize (skipped at equal sizes), the pyramid calls at equal sizes with the one camera at every scale, resize_bwd
    ups = [t if tuple(t.shape[2:]) == (H, W) else ops.resize(t, (H, W)) for t in x["disps"]]
    K4 = x["K"][:, None].expand(B, S, 3, 3).contiguous()
    x["ref_fwd"] = ops.warp_pyramid_fwd([x["hwc"]] * S, ups, x["poses"], K4, "hwc", want_valid=True)
    d_up, x["ref_d_pose"] = ops.warp_pyramid_bwd([x["hwc"]] * S, ups, x["poses"], K4, "hwc", x["g"])
    x["ref_d_up"] = d_up
    x["ref_d_disp"] = [g if tuple(t.shape[2:]) == (H, W) else ops.resize_bwd(g, t.shape[2:]) for g, t in zip(d_up, x["disps"])]
    torch.cuda.synchronize()
    return x


# ------------------------------------------------------------------------------------------------------------------------
# 1. forward and backward are the definition, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_src,kind", CASES, ids=IDS)
def test_forward_is_resize_then_the_pyramid_warp_bit_for_bit(name, n_src, kind):
    x = case(name, n_src, kind)
    B, H, W = x["B"], x["H"], x["W"]
    ref_warped, ref_valid = x["ref_fwd"]
    seen = 0
    for layout in LAYOUTS:
        warped, valid = x["fwd_" + layout]
        assert len(warped) == len(valid) == len(x["hw"])
        for s in range(len(x["hw"])):
            assert tuple(warped[s].shape) == (B, n_src, 3, H, W) and tuple(valid[s].shape) == (B, n_src, H, W)
            assert _bits(warped[s], ref_warped[s]), (layout, s)
            assert _bits(valid[s], ref_valid[s]), (layout, s)
            seen += int((valid[s] == 1).sum())
    assert seen > 0
    # without the mask: the same warped bits
    for layout in LAYOUTS:
        out = ops.warp_full_res_fwd(x[layout], x["disps"], x["poses"], x["K"], layout)
        assert all(_bits(a, b) for a, b in zip(out, ref_warped))


@pytest.mark.parametrize("name,n_src,kind", CASES, ids=IDS)
def test_backward_is_the_pyramid_backward_then_resize_bwd_bit_for_bit(name, n_src, kind):
    x = case(name, n_src, kind)
    for layout in LAYOUTS:
        d_disps, d_poses = x["bwd_" + layout]
        for i in range(n_src):
            assert _bits(d_poses[i], x["ref_d_pose"][i]), (layout, i)
        for s, hw in enumerate(x["hw"]):
            assert tuple(d_disps[s].shape) == (x["B"], 1) + hw
            assert _bits(d_disps[s], x["ref_d_disp"][s]), (layout, s)
            assert bool(torch.isfinite(d_disps[s]).all()) and float(d_disps[s].abs().max()) > 0, s


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name,n_src,kind", [CASES[1], CASES[3], CASES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_two_calls_with_differently_filled_workspaces_agree_bit_for_bit(name, n_src, kind, layout):
    x = case(name, n_src, kind)
    nbytes = R.workspace_bytes(x["B"], n_src, x["H"], x["W"], x["hw"])
    for word in (SENTINEL, 0x3F800000, 0xFFFFFFFF):      # NaN, 1.0f and another NaN where partials and d_up will be read from
        ws = torch.full((nbytes // 4,), word - (1 << 32) if word >= (1 << 31) else word, dtype=torch.int32, device=DEV)
        d_disps, d_poses = ops.warp_full_res_bwd(x[layout], x["disps"], x["poses"], x["K"], layout, x["g"], ws=ws)
        for a, b in zip(d_disps + d_poses, x["bwd_" + layout][0] + x["bwd_" + layout][1]):
            assert _bits(a, b), hex(word)
    with pytest.raises(ValueError, match="bytes"):
        ops.warp_full_res_bwd(x[layout], x["disps"], x["poses"], x["K"], layout, x["g"], ws=ws[:nbytes // 4 - 64])


# ------------------------------------------------------------------------------------------------------------------------
# 2. guarded buffers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,res,which", [("planar", 0, 1), ("hwc", 4, 3), ("hwc", 12, 5), ("planar", 8, 6)],
                         ids=["planar-0-24x40", "hwc-4-13x21", "hwc-12-130x127", "planar-8-general"])
def test_buffer_contract(dev, layout, res, which):
    """every output pre-filled with the sentinel is overwritten completely, inputs are only read, and the guard bands around warped,
    valid, d_disp, d_pose and a workspace of exactly the stated size stay as they were; placed at `res` bytes off a 16-byte boundary.
    valid of the odd scales is left NULL: its array keeps every sentinel.  The workspace starts out as NaN sentinels: a fold or a
    gather that reads a word nobody wrote gives a NaN."""
    name, n, kind = CASES[which]
    x = case(name, n, kind)
    B, H, W, hw = x["B"], x["H"], x["W"], x["hw"]
    S = len(hw)
    d = _lib.SfmWarpFullResDesc()
    d.B, d.n_src, d.n_scales, d.H, d.W, d.image_layout = B, n, S, H, W, ops._LAYOUTS[layout]
    specs = [("K", (B, 3, 3), res), ("src", tuple(x[layout].shape), res)]
    specs += [("pose%d" % i, (B, 6), res) for i in range(n)] + [("d_pose%d" % i, (B, 6), res) for i in range(n)]
    for s, (h, w) in enumerate(hw):
        d.h[s], d.w[s] = h, w
        specs += [("disp%d" % s, (B, 1, h, w), res), ("g%d" % s, (B, n, 3, H, W), res), ("warped%d" % s, (B, n, 3, H, W), res),
                  ("valid%d" % s, (B, n, H, W), res), ("d_disp%d" % s, (B, 1, h, w), res)]
    nbytes = _lib.lib.sfm_warp_full_res_bwd_workspace_bytes(C.byref(d))      # (no pointer is bound yet)
    assert nbytes == R.workspace_bytes(B, n, H, W, hw)
    arena = Arena(dev, specs + [("ws", nbytes, "ws")], row_floats=3 * W)
    assert arena.guard >= GUARD_MIN_BYTES
    inputs = [("K", x["K"]), ("src", x[layout])] + [("pose%d" % i, x["poses"][i]) for i in range(n)]
    for s in range(S):
        inputs += [("disp%d" % s, x["disps"][s]), ("g%d" % s, x["g"][s])]
    for key, a in inputs:
        arena.set(key, a)
        arena.snapshot(key)
    d.intrinsics, d.src = arena.ptr("K"), arena.ptr("src")
    for i in range(n):
        d.pose[i], d.d_pose[i] = arena.ptr("pose%d" % i), arena.ptr("d_pose%d" % i)
    bound = [s for s in range(S) if s % 2 == 0]
    for s in range(S):
        d.disp[s], d.g_warped[s] = arena.ptr("disp%d" % s), arena.ptr("g%d" % s)
        d.warped[s], d.d_disp[s] = arena.ptr("warped%d" % s), arena.ptr("d_disp%d" % s)
        if s in bound:
            d.valid[s] = arena.ptr("valid%d" % s)
    outs = ["d_pose%d" % i for i in range(n)] + ["%s%d" % (k, s) for s in range(S) for k in ("warped", "d_disp")] + ["valid%d" % s for s in bound]
    assert all(arena.sentinels_left(o) == arena.nbytes(o) // 4 for o in outs) and arena.sentinels_left("ws") == nbytes // 4
    ops._launch(dev, _lib.lib.sfm_warp_full_res_fwd, C.byref(d))
    ops._launch(dev, _lib.lib.sfm_warp_full_res_bwd, C.byref(d), C.c_void_p(arena.ptr("ws")), nbytes)
    torch.cuda.synchronize()
    for o in outs:
        assert arena.sentinels_left(o) == 0, o
    for s in range(S):
        if s not in bound:
            assert arena.sentinels_left("valid%d" % s) == arena.nbytes("valid%d" % s) // 4, "valid[%d] is NULL: nothing is written" % s
    arena.check("sfm_warp_full_res_fwd / _bwd (%s)" % layout)
    for key, _ in inputs:
        arena.unchanged(key)
    as_bits = lambda t: t.contiguous().view(torch.int32).cpu().numpy()
    for s in range(S):
        np.testing.assert_array_equal(arena.bits("warped%d" % s), as_bits(x["ref_fwd"][0][s]))
        np.testing.assert_array_equal(arena.bits("d_disp%d" % s), as_bits(x["ref_d_disp"][s]))
        if s in bound:
            np.testing.assert_array_equal(arena.bits("valid%d" % s), as_bits(x["ref_fwd"][1][s]))
    for i in range(n):
        np.testing.assert_array_equal(arena.bits("d_pose%d" % i), as_bits(x["ref_d_pose"][i]))


# ------------------------------------------------------------------------------------------------------------------------
# 3. an independent opinion on the gather
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_src,kind", [CASES[1], CASES[2], CASES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_d_disp_against_float64_aten(name, n_src, kind):
    """d_disp of every resampled scale against float64 autograd of F.interpolate(bilinear, align_corners=True) on the CPU, applied to
    the full-resolution gradient the kernel gathers from (the pyramid backward's d_disp at equal sizes).  Allowed: 4 x the distance
    of the float32 NumPy restatement (tests/warp_full_res_ref.py) from the same float64 value -- the float32 statement's own rounding,
    measured, not guessed (+ 1e-6 of the largest value, the floor of the rule of tests/test_disp_smooth_gpu.py)."""
    x = case(name, n_src, kind)
    d_disps = x["bwd_hwc"][0]
    checked = 0
    for s, hw in enumerate(x["hw"]):
        if hw == (x["H"], x["W"]):
            continue
        d_up = x["ref_d_up"][s].cpu().numpy()
        o64 = R.adjoint64_aten(d_up, hw)
        o32 = R.adjoint(d_up, hw, F32)
        ratio = rule(d_disps[s].cpu().numpy(), o64, o32, "warp_full_res %s scale %d (%dx%d) d_disp against float64 aten" % ((IDS[CASES.index((name, n_src, kind))], s) + hw))
        parity_note("warp_full_res %s scale %d d_disp: max|gpu - o64| / max|numpy32 - o64| = %.3g" % (name, s, ratio))
        checked += 1
    assert checked == len(x["hw"]) - 1


# ------------------------------------------------------------------------------------------------------------------------
# 4. torch_api.warp_full_res
# ------------------------------------------------------------------------------------------------------------------------
def _torch_inputs(name="13x21", n_src=3, seed=5, four_d_K=False):
    (H, W), hw = R.SHAPES[name]
    B = 2
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=1, seed=seed)
    rng = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    K = _t(d["intrinsics"][:, 0])
    return dict(src=_t(d["src"]), K=K, hw=hw, H=H, W=W,
                disps=[_t(10.0 / (1.0 + np.exp(-1.5 * rng.uniform(-1, 1, (B, 1, h, w)))) + 0.01).requires_grad_() for h, w in hw],
                packed=_t(np.concatenate(d["poses"], axis=1)).requires_grad_(),
                w=[torch.randn((B, n_src, 3, H, W), generator=gen).to(DEV) for _ in hw])


def _loss(x, disps=None, packed=None, **kw):
    out = ta.warp_full_res(x["src"], x["K"], x["disps"] if disps is None else disps, x["packed"] if packed is None else packed, **kw)
    warped = out[0] if kw.get("return_valid") else out
    return sum((w * a).sum() for w, a in zip(x["w"], warped)), out


def _expected(x):
    B, n, _, H, W = x["src"].shape
    hwc = ops.pyramid_hwc(x["src"].view(B, 3 * n, H, W), 1)[0]
    poses = [x["packed"].detach()[:, 6 * i:6 * i + 6].contiguous() for i in range(n)]
    disps = [t.detach() for t in x["disps"]]
    warped, valid = ops.warp_full_res_fwd(hwc, disps, poses, x["K"], "hwc", want_valid=True)
    d_disps, d_poses = ops.warp_full_res_bwd(hwc, disps, poses, x["K"], "hwc", x["w"])
    return warped, valid, d_disps, torch.cat(d_poses, dim=1)


def test_autograd_gives_the_operators_bits():
    x = _torch_inputs()
    warped, valid, d_disps, d_packed = _expected(x)
    total, (got, got_valid) = _loss(x, return_valid=True)
    assert len(got) == len(got_valid) == len(warped)
    for a, b, va, vb in zip(got, warped, got_valid, valid):
        assert a.requires_grad and not va.requires_grad and _bits(a, b) and _bits(va, vb)
    total.backward()
    for t, w in zip(x["disps"], d_disps):
        assert t.grad.shape == t.shape and _bits(t.grad, w)
    assert _bits(x["packed"].grad, d_packed)
    # the (B,S,3,3) intrinsics of sfm_learner_loss: [:, 0] is used
    S = len(x["disps"])
    K4 = torch.stack([x["K"] / 2 ** s for s in range(S)], dim=1)
    assert all(_bits(a, b) for a, b in zip(ta.warp_full_res(x["src"], K4, x["disps"], x["packed"]), warped))
    # a scale the loss does not use: its upstream gradient is None -> zeros
    disps = [t.detach().clone().requires_grad_() for t in x["disps"]]
    packed = x["packed"].detach().clone().requires_grad_()
    out = ta.warp_full_res(x["src"], x["K"], disps, packed)
    (x["w"][1] * out[1]).sum().backward()
    assert bool((disps[0].grad == 0).all()) and bool((disps[2].grad == 0).all()) and float(disps[1].grad.abs().max()) > 0
    with torch.no_grad():
        assert not ta.warp_full_res(x["src"], x["K"], x["disps"], x["packed"])[0].requires_grad


def test_bf16_predictions_get_bf16_gradients():
    x = _torch_inputs("24x40", 1)
    d16 = [t.detach().to(torch.bfloat16).requires_grad_() for t in x["disps"]]
    p16 = x["packed"].detach().to(torch.bfloat16).requires_grad_()
    _loss(x, d16, p16)[0].backward()
    d32 = [t.detach().float().requires_grad_() for t in d16]
    p32 = p16.detach().float().requires_grad_()
    _loss(x, d32, p32)[0].backward()
    for a, b in zip(d16 + [p16], d32 + [p32]):
        assert a.grad.dtype == torch.bfloat16 and a.grad.shape == a.shape and _bits(a.grad, b.grad.to(torch.bfloat16))


def test_intrinsics_that_require_grad_are_refused():
    x = _torch_inputs("24x40", 1)
    with pytest.raises(TypeError, match="projective_inverse_warp"):
        ta.warp_full_res(x["src"], x["K"].clone().requires_grad_(), x["disps"], x["packed"])
    with pytest.raises(TypeError, match="intrinsics"):
        ta.warp_full_res(x["src"], x["K"][:, :2], x["disps"], x["packed"])


def _captured(step):
    """(eager, captured and replayed once) results of step()"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = [t.clone() for t in step()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    return eager, captured


def test_no_sync_and_graph_capture():
    x = _torch_inputs()
    leaves = x["disps"] + [x["packed"]]

    def step():
        for t in leaves:
            t.grad = None
        total, out = _loss(x)
        total.backward()
        # (detached: a result that keeps its grad_fn keeps the eager run's autograd graph alive, and with it the leaves' gradient
        #  accumulators, which belong to the stream of that run -- the capture would then fork onto that stream)
        return [t.detach() for t in out] + [t.grad for t in leaves]

    eager, captured = _captured(step)
    assert all(_bits(a, b) for a, b in zip(eager, captured))
    assert all(float(t.abs().max()) > 0 for t in eager)


# ------------------------------------------------------------------------------------------------------------------------
# 5. min_reprojection_loss(full_res=True)
# ------------------------------------------------------------------------------------------------------------------------
STEPS = {"40x130": dict(B=2, H=40, W=130, n_src=2, n_scales=2), "24x56": dict(B=1, H=24, W=56, n_src=3, n_scales=3)}


def _step_inputs(step):
    d = synth.make_inputs(seed=21, **STEPS[step])
    return dict(src=_t(d["src"]), tgt=_t(d["tgt"]), K=_t(d["intrinsics"]), disps=[_t(a) for a in d["disps"]], poses=[_t(a) for a in d["poses"]])


@pytest.mark.parametrize("smooth_weight", [0.0, 1e-3])
@pytest.mark.parametrize("auto_mask", [True, False])
@pytest.mark.parametrize("step", sorted(STEPS))
def test_full_res_composite_is_its_stages(step, auto_mask, smooth_weight):
    """total, d_disp and d_pose are, bit for bit, the chain run by hand through ops.*: every scale at full resolution against the one
    full-resolution target, the identity error computed once, the smoothness on the target pyramid at each disparity's own size"""
    alpha = 0.85
    x = _step_inputs(step)
    src, tgt, K, disps, poses = x["src"], x["tgt"], x["K"], x["disps"], x["poses"]
    B, n_src, _, H, W = src.shape
    S = len(disps)
    leaves = [t.requires_grad_() for t in disps + poses]
    total = ta.min_reprojection_loss(tgt, src, K, disps, poses, ssim_rate=alpha, auto_mask=auto_mask, smooth_weight=smooth_weight, full_res=True)
    assert total.dim() == 0 and total.dtype == torch.float32 and total.grad_fn is not None
    got = torch.autograd.grad(total, leaves)
    with torch.no_grad():
        w = [2.0 ** -s for s in range(S)]
        stacked = src.view(B, 3 * n_src, H, W)
        hwc = ops.pyramid_hwc(stacked, 1)[0]
        K0 = K[:, 0].contiguous()
        warped, valid = ops.warp_full_res_fwd(hwc, disps, poses, K0, "hwc", True)
        errs = ops.photo_error_fwd(warped, [tgt] * S, alpha)
        idents = ops.photo_error_fwd([stacked.view(B, n_src, 3, H, W)], [tgt], alpha) * S if auto_mask else None
        loss, count, winners = ops.min_reproj_fwd(errs, valid, idents, w, "kept")
        g_loss = torch.zeros(S + 1, device=DEV)
        g_loss[S] = 1
        g_errs = ops.min_reproj_bwd(winners, count, g_loss, n_src, w, "kept", [(H, W)] * S)
        d_disps, d_poses = ops.warp_full_res_bwd(hwc, disps, poses, K0, "hwc", ops.photo_error_bwd(warped, [tgt] * S, alpha, g_errs))
        want = loss[S]
        if smooth_weight:
            sw = [smooth_weight * v for v in w]
            tgts = ops.pyramid(tgt, S)
            sm_loss, stats = ops.disp_smooth_fwd(disps, tgts, sw, True, "mean_abs")
            want = loss[S] + sm_loss[S]
            ops.disp_smooth_bwd(disps, tgts, stats, g_loss, sw, True, "mean_abs", out=d_disps)
    assert _bits(total.detach(), want)
    for k, (a, b) in enumerate(zip(got, d_disps + d_poses)):
        assert _bits(a, b), k
    # (a sanity check of the inputs, not of the library: with the auto-mask a coarse scale of a small frame may keep few pixels)
    assert float(total.detach()) > 0 and all(bool(torch.isfinite(t).all()) for t in got) and 0 < int(count[0])
    assert float(got[0].abs().max()) > 0 and any(float(t.abs().max()) > 0 for t in got[S:])
    # it is another objective than the pyramid form
    assert not _bits(total.detach(), ta.min_reprojection_loss(tgt, src, K, disps, poses, ssim_rate=alpha, auto_mask=auto_mask,
                                                              smooth_weight=smooth_weight).detach())


def _example(x, alpha, smooth_weight, tail):
    """INTEGRATION.md, 'Full-resolution multi-scale': the loop min_reprojection_loss(full_res=True) replaces, written with the
    calls the library had before -- resize_images per scale, projective_inverse_warp per (scale, source) -- and aten; tail: the
    dtype its last where / sum / divide and the smoothness run in"""
    src, tgt, K0 = x["src"], x["tgt"], x["K"][:, 0].contiguous()
    B, n_src, _, H, W = src.shape
    with torch.no_grad():
        ident = ta.photometric_error([src], [tgt], ssim_rate=alpha)[0]
    total = 0.0
    for s, disp in enumerate(x["disps"]):
        depth = (1 / ta.resize_like(disp, tgt)).view(B, H * W)
        warped = torch.stack([ta.projective_inverse_warp(src[:, i], depth, x["poses"][i], K0) for i in range(n_src)], dim=1)
        valid = (warped.detach() != 0).any(2)      # the reference's own mask: a pixel out of view is exactly 0 in all three channels
        e = ta.photometric_error([warped], [tgt], ssim_rate=alpha)[0]
        e = torch.where(valid, e, torch.full_like(e, float("inf")))
        best = e.min(1).values
        keep = best < ident.min(1).values
        total = total + torch.where(keep, best, torch.zeros_like(best)).to(tail).sum() / keep.sum().clamp(min=1) / 2 ** s
    if smooth_weight:
        from test_disp_smooth_gpu import disparity_smoothness_aten
        total = total + smooth_weight * disparity_smoothness_aten(x["disps"], tgt, tail)
    return total


@pytest.mark.parametrize("smooth_weight", [0.0, 1e-3])
@pytest.mark.parametrize("step", sorted(STEPS))
def test_full_res_composite_against_the_example_in_aten(step, smooth_weight):
    """with the auto-mask, and with and without the smoothness term: the total within 2 float32 ulps of the example with a float64
    tail (the smoothness term added: by the rule below), every gradient within 4 x the distance of the example with a float32 tail
    from it -- the assertions of tests/test_min_reproj_gpu.py and tests/test_disp_smooth_gpu.py for the pyramid form"""
    alpha = 0.85
    x = _step_inputs(step)
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    S = len(x["disps"])
    total = ta.min_reprojection_loss(x["tgt"], x["src"], x["K"], x["disps"], x["poses"], ssim_rate=alpha, smooth_weight=smooth_weight, full_res=True)
    got = torch.autograd.grad(total, leaves)
    t64 = _example(x, alpha, smooth_weight, torch.float64)
    g64 = torch.autograd.grad(t64, leaves)
    t32 = _example(x, alpha, smooth_weight, torch.float32)
    g32 = torch.autograd.grad(t32, leaves)
    want = float(t64.detach())
    ulps = abs(float(total.detach()) - want) / float(np.spacing(F32(want)))
    line = "min_reprojection_loss(full_res) %s smooth=%g: total %.9g, float64 tail %.17g (%.3g ulp), float32 tail %.9g" % (
        step, smooth_weight, float(total.detach()), want, ulps, float(t32.detach()))
    print(line)
    parity_note(line)
    if smooth_weight:
        rule(float(total.detach()), want, float(t32.detach()), "full_res %s composite total against the example" % step)
    else:
        assert ulps <= 2, line
    for k, (g, r, b) in enumerate(zip(got, g64, g32)):
        what = "d_disp[%d]" % k if k < S else "d_pose[%d]" % (k - S)
        rule(g.cpu().numpy(), r.cpu().numpy(), b.cpu().numpy(), "full_res %s smooth=%g %s against the example" % (step, smooth_weight, what))


@pytest.mark.parametrize("step", sorted(STEPS))
def test_full_res_false_is_the_existing_call(step):
    x = _step_inputs(step)
    args = (x["tgt"], x["src"], x["K"], x["disps"], x["poses"])
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    for kw in (dict(), dict(smooth_weight=1e-3), dict(auto_mask=False)):
        a = ta.min_reprojection_loss(*args, ssim_rate=0.85, **kw)
        b = ta.min_reprojection_loss(*args, ssim_rate=0.85, full_res=False, **kw)
        assert _bits(a.detach(), b.detach())
        assert all(_bits(p, q) for p, q in zip(torch.autograd.grad(a, leaves), torch.autograd.grad(b, leaves)))


def test_full_res_dtypes_errors_and_graph_capture():
    x = _step_inputs("40x130")
    disps = [t.to(torch.bfloat16).requires_grad_() for t in x["disps"]]
    packed = torch.cat(x["poses"], dim=1).requires_grad_()
    # the full-resolution camera alone is enough
    total = ta.min_reprojection_loss(x["tgt"], x["src"], x["K"][:, 0], disps, packed, ssim_rate=0.85, full_res=True)
    total.backward()
    assert all(t.grad is not None and t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape for t in disps)
    assert packed.grad is not None and packed.grad.shape == packed.shape
    with pytest.raises(TypeError, match="intrinsics"):
        ta.min_reprojection_loss(x["tgt"], x["src"], x["K"].clone().requires_grad_(), x["disps"], x["poses"], ssim_rate=0.85, full_res=True)
    # any disparity sizes without the smoothness term; with it, the target pyramid's
    odd = [x["disps"][0], x["disps"][1][:, :, :7, :11].contiguous()]
    assert float(ta.min_reprojection_loss(x["tgt"], x["src"], x["K"], odd, x["poses"], ssim_rate=0.85, full_res=True)) > 0
    with pytest.raises(TypeError, match="smooth_weight"):
        ta.min_reprojection_loss(x["tgt"], x["src"], x["K"], odd, x["poses"], ssim_rate=0.85, smooth_weight=1e-3, full_res=True)

    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]

    def step():
        for t in leaves:
            t.grad = None
        loss = ta.min_reprojection_loss(x["tgt"], x["src"], x["K"], x["disps"], x["poses"], ssim_rate=0.85, smooth_weight=1e-3, full_res=True)
        loss.backward()
        return [loss.detach()] + [t.grad for t in leaves]

    eager, captured = _captured(step)
    assert all(_bits(a, b) for a, b in zip(eager, captured))
    assert float(eager[0]) > 0 and float(eager[1].abs().max()) > 0 and any(float(t.abs().max()) > 0 for t in eager[3:])
