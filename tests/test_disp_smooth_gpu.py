"""sfm_disp_smooth_fwd / _bwd, torch_api.disparity_smoothness and min_reprojection_loss(smooth_weight=...) on the GPU.

The reference is the term as a user writes it in aten (tests/disp_smooth_ref.py: aten_statement), evaluated in float64 on the float32
inputs; the same statement in float32 is one valid float32 evaluation of the formula, and its own distance from float64 sets the
tolerance -- the rule of tests/test_photo_error_gpu.py, per array and per loss value:
    max|gpu - o64| <= 4 max|o32 - o64| + 1e-6 max|o64|.
Nothing is masked and no pixel is left out: the float32 difference of two float32 values has the sign of the exact difference, so no
pixel sits on the corner of |.| except the exact zeros, where both sides give 0.

Shapes: the smallest at which the kernels can still go wrong -- the run length DS_BLOCK_PIXELS is read from csrc/sfm_disp_smooth.hip;
3x3; maps one pixel below, at and just above one and two runs; widths 63, 64, 65 and 129 (a row end inside a wave, on a wave end and
-- four rows of 64 -- on a block end); one map whose single sample has more partials than two rounds of the fold's 64 lanes; a
four-scale pyramid of odd, unrelated sizes; more (scale, sample) pairs than twice the waves of the fold's block (DS_FOLD_WAVES, read
from the same file), so that a wave finishes a third sample; a batch of more than 128, the third round of the ordered sum over the
samples.  Inputs (tests/test_disp_smooth_cpu.py: make_inputs): disparities in (0.01, 10) with flat patches and both signs of difference, the means of neighbouring samples a factor of about 4 or 16 apart, images in [-1,1]."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

from oracle import sfm_oracle as oracle
from test_disp_smooth_cpu import COMBOS, EDGES, g_loss_of, make_inputs, rule, statement, weights_of
from test_min_reproj_gpu import _example_with_a_float64_tail, _frame, _step_inputs
from util import Arena, SENTINEL, parity_note

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
_HIP = open(os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", "sfm_disp_smooth.hip")).read()
BP = int(re.search(r"constexpr int DS_BLOCK_PIXELS = (\d+);", _HIP).group(1))
FOLD_WAVES = int(re.search(r"constexpr int DS_FOLD_WAVES = (\d+);", _HIP).group(1))      # a wave of the fold finishes the samples wave, wave + FOLD_WAVES, ...
RUNS = [_frame(BP - 1, -1), _frame(BP, 0), _frame(BP + 1, 1), _frame(2 * BP - 1, -1), _frame(2 * BP, 0), _frame(2 * BP + 1, 1)]
FOLD = (BP // 2 + 2, BP - 1)        # 130 x 255 for runs of 256: 130 partials per sample

# (B, [(h, w)], seed)
CASES = {
    "3x3": (2, ((3, 3),), 31),
    "runs": (2, tuple(RUNS), 32),
    "widths": (2, ((5, 63), (5, 64), (5, 65), (3, 129)), 33),
    "fold": (2, (FOLD,), 34),
    "pyramid": (3, ((17, 61), (9, 31), (5, 16), (3, 8)), 35),
    "waves": (2 * FOLD_WAVES // 4 + 1, ((3, 3), (3, 4), (4, 3), (3, 5)), 36),      # every wave of the fold finishes a third sample
    "batch": (2 * 64 + 3, ((3, 3),), 37),                                          # the sum over the samples goes into its third round of 64
}


def _nrun(h, w):
    return -(-(h * w) // BP)


def test_the_shapes_are_the_ones_the_kernels_can_go_wrong_at():
    px = [h * w for h, w in RUNS]
    assert BP - 4 <= px[0] < BP == px[1] < px[2] <= BP + 4 and 2 * BP - 4 <= px[3] < 2 * BP == px[4] < px[5] <= 2 * BP + 4, px
    assert [_nrun(h, w) for h, w in RUNS] == [1, 1, 2, 2, 2, 3]
    assert BP != 256 or (FOLD == (130, 255) and _nrun(*FOLD) == 130)
    assert _nrun(*FOLD) > 128, "a single sample has more partials than two rounds of the fold's 64 lanes"
    assert [w for _, w in CASES["widths"][1]] == [63, 64, 65, 129] and all(h * w > 64 for h, w in CASES["widths"][1])
    assert BP % 64 == 0 and BP // 64 <= 5, "rows of 64 end on wave ends, and one of the five on a block end"
    B, hw, _ = CASES["waves"]
    assert len(hw) * B > 2 * FOLD_WAVES and len(hw) == 4, "some wave of the fold's block finishes a first, a second and a third (scale, sample)"
    assert CASES["batch"][0] > 2 * 64 and CASES["batch"][0] % 64, "the ordered sum over the samples runs three rounds of 64, the last one partly filled"
    assert "j += 64)" in _HIP, "a lane of the fold adds every 64th partial: 130 of them are three rounds"
    assert CASES["3x3"][1] == ((3, 3),) and len(CASES["pyramid"][1]) == 4 and all(h % 2 and w >= 3 for h, w in CASES["pyramid"][1])
    for name, (B, hw, seed) in CASES.items():
        disps, imgs = make_inputs(B, list(hw), seed)
        for d, img in zip(disps, imgs):
            means = d.reshape(B, -1).mean(1)
            assert 0.01 < d.min() and d.max() < 10 and (np.maximum(means[1:] / means[:-1], means[:-1] / means[1:]) >= 2).all() and np.abs(img).max() <= 1, name
            dx, dy = np.diff(d, axis=3), np.diff(d, axis=2)
            assert (dx == 0).any() and (dy == 0).any() and (dx > 0).any() and (dx < 0).any() and (dy > 0).any() and (dy < 0).any(), name


@pytest.fixture(autouse=True)
def _needs_a_gpu(dev):
    """(the `dev` fixture skips where no GPU is visible)"""


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _w(S):
    return [float(w) for w in weights_of(S)]


@functools.lru_cache(maxsize=None)
def gpu(name, normalize, edge):
    """-> (loss (S+1,), stats (S,B,3), [g_disp_s]) as host arrays, through ops.*"""
    B, hw, seed = CASES[name]
    disps, imgs = make_inputs(B, list(hw), seed)
    S = len(hw)
    D, I = [_t(a) for a in disps], [_t(a) for a in imgs]
    loss, stats = ops.disp_smooth_fwd(D, I, _w(S), normalize, edge)
    g = ops.disp_smooth_bwd(D, I, stats, _t(g_loss_of(S)), _w(S), normalize, edge)
    return loss.cpu().numpy(), stats.cpu().numpy(), [t.cpu().numpy() for t in g]


# ------------------------------------------------------------------------------------------------------------------------
# 1. values and gradients against the float64 statement
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize,edge", COMBOS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_and_backward_against_the_statement(name, normalize, edge):
    B, hw, seed = CASES[name]
    S = len(hw)
    loss, stats, g = gpu(name, normalize, edge)
    l64, g64 = statement(CASES[name], normalize, edge, torch.float64)
    l32, g32 = statement(CASES[name], normalize, edge, torch.float32)
    assert loss.dtype == F32 and loss.shape == (S + 1,) and stats.dtype == F64 and stats.shape == (S, B, 3)
    what = "%s normalize=%d %s" % (name, normalize, edge)
    for s in range(S + 1):
        parity_note("disp_smooth %s loss[%d]: ratio %.3g" % (what, s, rule(loss[s], l64[s], l32[s], "%s loss[%d]" % (what, s))))
    for s in range(S):
        assert g[s].dtype == F32 and g[s].shape == (B, 1) + hw[s]
        parity_note("disp_smooth %s g_disp[%d]: ratio %.3g" % (what, s, rule(g[s], g64[s], g32[s], "%s g_disp[%d]" % (what, s))))
    # stats are what the header says: the per-sample mean + 1e-7 (or 1), and non-negative sums
    disps, _ = make_inputs(B, list(hw), seed)
    for s in range(S):
        want = disps[s].astype(F64).reshape(B, -1).mean(1) + 1e-7 if normalize else np.ones(B)
        assert np.allclose(stats[s, :, 0], want, rtol=1e-13, atol=0) and (stats[s, :, 1:] > 0).all(), (s, stats[s])


# ------------------------------------------------------------------------------------------------------------------------
# 2. cross-checks at normalize = False, edge = "abs_mean": the oracle and the fused loss
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pyramid", "widths", "fold"])
def test_gradient_against_the_oracle(name):
    B, hw, seed = CASES[name]
    disps, imgs = make_inputs(B, list(hw), seed)
    S = len(hw)
    D, I = [_t(a) for a in disps], [_t(a) for a in imgs]
    one = [1.0] * S
    loss, stats = ops.disp_smooth_fwd(D, I, one, False, "abs_mean")
    g = ops.disp_smooth_bwd(D, I, stats, _t(np.array([1.0] * S + [0.0], F32)), one, False, "abs_mean")
    for s in range(S):
        o = {dt: (oracle.compute_disp_smooth(imgs[s], disps[s], dt), oracle.compute_disp_smooth_backward(imgs[s], disps[s], dt)) for dt in (F64, F32)}
        rule(float(loss[s]), o[F64][0], o[F32][0], "%s scale %d loss against the oracle" % (name, s))
        rule(g[s].cpu().numpy(), o[F64][1], o[F32][1], "%s scale %d g_disp against the oracle" % (name, s))


@pytest.mark.parametrize("step", ["40x130", "24x56"])
def test_total_against_the_fused_loss(step):
    """weights smooth_reg / 2**s: the smooth term of sfm_learner_loss(smooth_mode="edge_aware"), to the loss tolerance of the fused
    kernel (1e-4 relative)"""
    x = _step_inputs(step)
    smooth_reg = 0.3
    S = len(x["disps"])
    with torch.no_grad():
        _, terms = ta.sfm_learner_loss(x["tgt"], x["src"], x["K"], x["disps"], x["poses"], smooth_reg=smooth_reg, smooth_mode="edge_aware")
        total, _ = ta.disparity_smoothness(x["disps"], x["tgt"], normalize=False, edge="abs_mean", weights=[smooth_reg / 2 ** s for s in range(S)])
    want, got = float(terms[1]), float(total)
    print("disp_smooth %s: total %.9g, fused smooth term %.9g, relative %.3g" % (step, got, want, abs(got - want) / abs(want)))
    assert want > 0 and abs(got - want) <= 1e-4 * abs(want), (got, want)


# ------------------------------------------------------------------------------------------------------------------------
# 3. accumulate, determinism and the buffer contract
# ------------------------------------------------------------------------------------------------------------------------
def _arena_run(name, normalize, edge, ws_word, pre=None):
    """Both calls on guarded buffers at sub-tensor offsets through the C ABI; the workspace filled with `ws_word`, loss, stats and
    g_disp with the sentinel (a NaN) -- or g_disp with pre[s] and accumulate = 1 -> (loss bits, stats, [g_disp bits])"""
    B, hw, seed = CASES[name]
    disps, imgs = make_inputs(B, list(hw), seed)
    S = len(hw)
    d = _lib.SfmDispSmoothDesc()
    d.B, d.n_scales, d.normalize, d.edge, d.accumulate = B, S, int(normalize), EDGES[edge], int(pre is not None)
    for s, ((h, w), wt) in enumerate(zip(hw, _w(S))):
        d.H[s], d.W[s], d.weight[s] = h, w, wt
    nbytes = _lib.lib.sfm_disp_smooth_workspace_bytes(C.byref(d))
    assert nbytes % 256 == 0 and nbytes >= 24 * sum(B * _nrun(h, w) for h, w in hw)
    specs = [("loss", (S + 1,), 4), ("stats", (S * B * 3 * 2,), 8), ("g_loss", (S + 1,), 12), ("ws", nbytes, "ws")]     # stats: doubles
    for s, (h, w) in enumerate(hw):
        specs += [("disp%d" % s, (B, 1, h, w), 4 * (s % 4)), ("img%d" % s, (B, 3, h, w), 4 * ((s + 1) % 4)), ("g%d" % s, (B, 1, h, w), 4 * ((s + 2) % 4))]
    ar = Arena(DEV, specs, row_floats=max(w for _, w in hw))
    ar.set("g_loss", g_loss_of(S))
    ar.fill_bits("ws", ws_word)
    inputs_ = ["g_loss"]
    for s in range(S):
        ar.set("disp%d" % s, disps[s]), ar.set("img%d" % s, imgs[s])
        inputs_ += ["disp%d" % s, "img%d" % s]
        if pre is not None:
            ar.set("g%d" % s, pre[s])
        d.disp[s], d.img[s], d.g_disp[s] = ar.ptr("disp%d" % s), ar.ptr("img%d" % s), ar.ptr("g%d" % s)
    d.loss, d.stats, d.g_loss = ar.ptr("loss"), ar.ptr("stats"), ar.ptr("g_loss")
    for key in inputs_:
        ar.snapshot(key)
    _lib.check(_lib.lib.sfm_disp_smooth_fwd(C.byref(d), C.c_void_p(ar.ptr("ws")), nbytes, ops._stream()))
    ar.snapshot("stats")
    _lib.check(_lib.lib.sfm_disp_smooth_bwd(C.byref(d), ops._stream()))
    torch.cuda.synchronize()
    what = "%s normalize=%d %s" % (name, normalize, edge)
    ar.check(what)                                    # nothing before or behind any array
    assert ar.sentinels_left("loss") == 0 and ar.sentinels_left("stats") == 0, what
    for key in inputs_ + ["stats"]:
        ar.unchanged(key)                             # (the backward reads stats, it does not write them)
    for s in range(S):
        assert ar.sentinels_left("g%d" % s) == 0, "%s scale %d: an element of g_disp was not written" % (what, s)
    return ar.bits("loss"), ar.bits("stats").view(F64).reshape(S, B, 3), [ar.bits("g%d" % s) for s in range(S)]


@pytest.mark.parametrize("normalize,edge", [(True, "mean_abs"), (False, "abs_mean")])
@pytest.mark.parametrize("name", sorted(CASES))
def test_buffer_contract_determinism_and_accumulate(name, normalize, edge):
    """NaN-filled loss, stats and g_disp are overwritten completely, the guard bands around every array and the workspace stay
    untouched, the inputs keep their bits; two calls whose workspaces held different garbage agree bit for bit, and with what ops
    returns from its own allocations; with accumulate the result is pre + g0, ONE float32 addition, bit for bit"""
    first = _arena_run(name, normalize, edge, SENTINEL)
    again = _arena_run(name, normalize, edge, 0xFFFFFFFF)             # as fp64 partials: NaN
    loss, stats, g = gpu(name, normalize, edge)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[0], loss.view(np.int32))
    assert np.array_equal(first[1].view(np.int64), again[1].view(np.int64)) and np.array_equal(first[1].view(np.int64), stats.view(np.int64))
    rng = np.random.RandomState(9)
    pre = [rng.standard_normal(x.shape).astype(F32) * F32(np.abs(x).max()) for x in g]
    added = _arena_run(name, normalize, edge, SENTINEL, pre)
    for s in range(len(g)):
        assert np.array_equal(first[2][s], again[2][s]) and np.array_equal(first[2][s], g[s].view(np.int32)), s
        want = (_t(pre[s]) + _t(g[s])).cpu().numpy()
        assert np.array_equal(added[2][s], want.view(np.int32)), "scale %d: %d words differ from pre + g0" % (s, (added[2][s] != want.view(np.int32)).sum())
    # ops: a given `out` list is added to in place and returned
    B, hw, seed = CASES[name]
    disps, imgs = make_inputs(B, list(hw), seed)
    S = len(hw)
    out = [_t(p) for p in pre]
    got = ops.disp_smooth_bwd([_t(a) for a in disps], [_t(a) for a in imgs], _t(stats), _t(g_loss_of(S)), _w(S), normalize, edge, out=out)
    assert all(a is b for a, b in zip(got, out)) and all(np.array_equal(t.cpu().numpy().view(np.int32), a) for t, a in zip(out, added[2]))


# ------------------------------------------------------------------------------------------------------------------------
# 4. autograd
# ------------------------------------------------------------------------------------------------------------------------
def test_disparity_smoothness_autograd():
    """both outputs carry a gradient to the disparities and to nothing else; bf16 and fp16 maps get their own dtype back; a full
    target and the list of its pyramid agree; nothing is recorded without a leaf"""
    name, normalize, edge = "pyramid", True, "mean_abs"
    B, hw, seed = CASES[name]
    disps, imgs = make_inputs(B, list(hw), seed)
    S = len(hw)
    loss, stats, want_g = gpu(name, normalize, edge)
    g_loss = g_loss_of(S)
    xs = [_t(a).requires_grad_() for a in disps]
    ys = [_t(a).requires_grad_() for a in imgs]
    total, per_scale = ta.disparity_smoothness(xs, ys, weights=_w(S))
    assert total.dim() == 0 and _bits(total, _t(loss)[S]) and _bits(per_scale, _t(loss)[:S])
    (total * float(g_loss[S]) + (per_scale * _t(g_loss[:S])).sum()).backward()
    for s in range(S):
        assert np.array_equal(xs[s].grad.cpu().numpy().view(np.int32), want_g[s].view(np.int32)), s
        assert ys[s].grad is None
    for dtype in (torch.bfloat16, torch.float16):
        half = [_t(a).to(dtype).requires_grad_() for a in disps]
        t, _ = ta.disparity_smoothness(half, [_t(a) for a in imgs], normalize=False, edge="abs_mean")
        assert t.dtype == torch.float32
        t.backward()
        assert all(h.grad is not None and h.grad.dtype == dtype and h.grad.shape == h.shape and float(h.grad.abs().max()) > 0 for h in half)
        # ... and it is the float32 gradient at the upcast input, rounded once to the input's dtype
        up = [h.detach().to(torch.float32).requires_grad_() for h in half]
        t32, _ = ta.disparity_smoothness(up, [_t(a) for a in imgs], normalize=False, edge="abs_mean")
        assert _bits(t32.detach(), t.detach())
        t32.backward()
        for s, (h, u) in enumerate(zip(half, up)):
            assert torch.equal(h.grad.view(torch.int16), u.grad.to(dtype).view(torch.int16)), (dtype, s)
    assert not ta.disparity_smoothness([x.detach() for x in xs], ys)[0].requires_grad
    # a full-resolution target is turned into the pyramid of sfm_learner_loss
    x = _step_inputs("40x130")
    a = ta.disparity_smoothness(x["disps"], x["tgt"])
    b = ta.disparity_smoothness(x["disps"], ops.pyramid(x["tgt"], len(x["disps"])), weights=[1.0, 0.5])
    assert _bits(a[0], b[0]) and _bits(a[1], b[1]) and float(a[0]) > 0
    with pytest.raises(TypeError, match="pred_disps"):
        ta.disparity_smoothness(x["disps"][::-1], x["tgt"])
    with pytest.raises(ValueError, match="weight"):
        ta.disparity_smoothness(x["disps"], x["tgt"], weights=[1.0, -1.0])


def _captured(step):
    """eager under the synchronisation-forbidding guard, then captured in a graph and replayed -> (eager, captured)"""
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
    x = _step_inputs("40x130")
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    S = len(x["disps"])

    def alone():
        for t in leaves:
            t.grad = None
        total, per_scale = ta.disparity_smoothness(x["disps"], x["tgt"])
        (total + per_scale.sum()).backward()
        return [total.detach(), per_scale.detach()] + [t.grad for t in leaves[:S]]

    def composite():
        for t in leaves:
            t.grad = None
        loss = ta.min_reprojection_loss(x["tgt"], x["src"], x["K"], x["disps"], x["poses"], ssim_rate=0.85, smooth_weight=1e-3)
        loss.backward()
        return [loss.detach()] + [t.grad for t in leaves]

    for step in (alone, composite):
        eager, captured = _captured(step)
        assert all(_bits(a, b) for a, b in zip(eager, captured)), step.__name__
        assert float(eager[0]) > 0 and float(eager[1].abs().max()) > 0 and float(eager[-1].abs().max()) > 0, step.__name__


# ------------------------------------------------------------------------------------------------------------------------
# 5. the composite
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth_weight", [1e-3, 0.25])
@pytest.mark.parametrize("step", ["40x130", "24x56"])
def test_composite_is_the_sum_of_its_two_calls(step, smooth_weight):
    x = _step_inputs(step)
    args = (x["tgt"], x["src"], x["K"], x["disps"], x["poses"])
    S = len(x["disps"])
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    both = ta.min_reprojection_loss(*args, ssim_rate=0.85, smooth_weight=smooth_weight)
    assert both.dim() == 0 and both.dtype == torch.float32
    got = torch.autograd.grad(both, leaves)
    photo = ta.min_reprojection_loss(*args, ssim_rate=0.85)
    d_photo = torch.autograd.grad(photo, leaves)
    smooth, _ = ta.disparity_smoothness(x["disps"], x["tgt"], weights=[float(F32(smooth_weight * 2.0 ** -s)) for s in range(S)])
    d_smooth = torch.autograd.grad(smooth, leaves[:S])
    assert _bits(both.detach(), photo.detach() + smooth.detach())
    for s in range(S):
        assert _bits(got[s], d_photo[s] + d_smooth[s]), "d_disp[%d]" % s
        assert float(d_smooth[s].abs().max()) > 0 and not _bits(got[s], d_photo[s])
    for k in range(S, len(leaves)):
        assert _bits(got[k], d_photo[k]), "d_pose[%d]" % (k - S)
    # the other settings reach the kernel too
    other = ta.min_reprojection_loss(*args, ssim_rate=0.85, smooth_weight=smooth_weight, smooth_normalize=False, smooth_edge="abs_mean")
    plain, _ = ta.disparity_smoothness(x["disps"], x["tgt"], normalize=False, edge="abs_mean",
                                       weights=[float(F32(smooth_weight * 2.0 ** -s)) for s in range(S)])
    assert _bits(other.detach(), photo.detach() + plain.detach()) and not _bits(other.detach(), both.detach())


@pytest.mark.parametrize("step", ["40x130", "24x56"])
def test_smooth_weight_zero_is_the_existing_call(step):
    x = _step_inputs(step)
    args = (x["tgt"], x["src"], x["K"], x["disps"], x["poses"])
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    a = ta.min_reprojection_loss(*args, ssim_rate=0.85)
    b = ta.min_reprojection_loss(*args, ssim_rate=0.85, smooth_weight=0.0, smooth_normalize=False, smooth_edge="abs_mean")
    assert _bits(a.detach(), b.detach())
    assert all(_bits(p, q) for p, q in zip(torch.autograd.grad(a, leaves), torch.autograd.grad(b, leaves)))


def disparity_smoothness_aten(pred_disps, tgt_img, dtype=torch.float32):
    """INTEGRATION.md's example; dtype: what its arithmetic runs in (the pyramid is the library's float32 one either way)"""
    total = 0.0
    for s, (disp, img) in enumerate(zip(pred_disps, ops.pyramid(tgt_img, len(pred_disps)))):
        disp, img = disp.to(dtype), img.to(dtype)
        d = disp / (disp.mean(2, True).mean(3, True) + 1e-7)
        gx = (d[:, :, :, :-1] - d[:, :, :, 1:]).abs() * (-(img[:, :, :, :-1] - img[:, :, :, 1:]).abs().mean(1, keepdim=True)).exp()
        gy = (d[:, :, :-1, :] - d[:, :, 1:, :]).abs() * (-(img[:, :, :-1, :] - img[:, :, 1:, :]).abs().mean(1, keepdim=True)).exp()
        total = total + (gx.mean() + gy.mean()) / 2 ** s
    return total


@pytest.mark.parametrize("step", ["40x130", "24x56"])
def test_composite_against_the_example_in_aten(step):
    """min_reprojection_loss_ssim(...) + 1e-3 * disparity_smoothness_aten(...) of INTEGRATION.md, its tail and the smoothness in
    float64 (the reference) and in float32 (the deviation)"""
    x = _step_inputs(step)
    w = 1e-3
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    S = len(x["disps"])
    total = ta.min_reprojection_loss(x["tgt"], x["src"], x["K"], x["disps"], x["poses"], ssim_rate=0.85, smooth_weight=w)
    got = torch.autograd.grad(total, leaves)
    t64 = _example_with_a_float64_tail(x, 0.85, torch.float64)[0] + w * disparity_smoothness_aten(x["disps"], x["tgt"], torch.float64)
    g64 = torch.autograd.grad(t64, leaves)
    t32 = _example_with_a_float64_tail(x, 0.85, torch.float32)[0] + w * disparity_smoothness_aten(x["disps"], x["tgt"], torch.float32)
    g32 = torch.autograd.grad(t32, leaves)
    # the smoothness alone, as a value
    mine, _ = ta.disparity_smoothness([t.detach() for t in x["disps"]], x["tgt"])
    with torch.no_grad():
        s64, s32 = disparity_smoothness_aten(x["disps"], x["tgt"], torch.float64), disparity_smoothness_aten(x["disps"], x["tgt"], torch.float32)
    rule(float(mine), float(s64), float(s32), "%s disparity_smoothness against the example" % step)
    rule(float(total.detach()), float(t64.detach()), float(t32.detach()), "%s composite total against the example" % step)
    for k, (g, r, b) in enumerate(zip(got, g64, g32)):
        name = "d_disp[%d]" % k if k < S else "d_pose[%d]" % (k - S)
        rule(g.cpu().numpy(), r.cpu().numpy(), b.cpu().numpy(), "%s composite %s against the example" % (step, name))
