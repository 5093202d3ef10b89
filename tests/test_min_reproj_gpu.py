"""sfm_min_reproj_fwd / _bwd, torch_api.min_reprojection and torch_api.min_reprojection_loss on the GPU.

The reference is tests/min_reproj_ref.py, the pseudo-code of include/sfmwarp_min_reproj.h in NumPy.  Every comparison of a
selection runs on the float32 values themselves, so winner, count and g_err are compared EXACTLY and nothing is excluded.  The
sums: the kernel adds in fp64 (53 bits for at most 2^31 float32 terms of one sign: its error is far below half a float32 ulp), the
reference is math.fsum, so loss[s] and loss[n_scales] may differ by the final rounding alone: 1 float32 ulp.

Shapes: the smallest at which the kernels can still go wrong -- the run length MR_BLOCK_PIXELS is read from
csrc/sfm_min_reproj.hip; maps of one pixel below, at and just above one and two runs (257 is prime: 258 = 3 x 86 is the first map
above one run with both sides >= 3), one map of more than 128 runs in all (the fold's third round), the largest source counts on
a non-dyadic pyramid, and 3 x 3.  Planted in every case: ties, NaN, +inf, pixels with no finite source, pixels with every source
invalid, ident equal to best, NaN and +inf in ident, and (where there is more than one scale) one scale with nothing kept."""
import ctypes as C
import functools
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import min_reproj_ref as R
from test_photo_error_gpu import _within
from util import Arena, SENTINEL, parity_note

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
BP = int(re.search(r"constexpr int MR_BLOCK_PIXELS = (\d+);",
                   open(os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", "sfm_min_reproj.hip")).read()).group(1))
NORMS = {"kept": R.NORM_KEPT, "all": R.NORM_ALL}


def _frame(pixels, step):
    """(h, w), both >= 3, of the first map of `pixels`, pixels + step, ... pixels that has one"""
    while True:
        for h in range(3, math.isqrt(pixels) + 1):
            if pixels % h == 0:
                return h, pixels // h
        assert step, "%d pixels make no map with both sides >= 3" % pixels
        pixels += step


RUNS = [_frame(BP - 1, -1), _frame(BP, 0), _frame(BP + 1, 1), _frame(2 * BP - 1, -1), _frame(2 * BP, 0), _frame(2 * BP + 1, 1)]

# (B, n_err, n_ident, [(h, w)])
CASES = {
    "3x3": (1, 1, 0, [(3, 3)]),
    "runs": (2, 2, 1, RUNS),
    "fold": (2, 2, 3, [(130, 127)]),
    "max": (2, _lib.SFM_MAX_SRC, _lib.SFM_MAX_SRC, [(17, 61), (9, 31), (5, 16), (3, 8)]),
}
NOTHING_KEPT = {"runs": 2, "max": 1}          # the scale of a case at which no pixel is kept
VALID = {"all": lambda s: True, "none": lambda s: False, "subset": lambda s: s % 2 == 0}


def _blocks(B, hw):
    return [B * -(-(h * w) // BP) for h, w in hw]


def test_the_shapes_are_the_ones_the_kernels_can_go_wrong_at():
    px = [h * w for h, w in RUNS]
    assert BP - 4 <= px[0] < BP == px[1] < px[2] <= BP + 4 and 2 * BP - 4 <= px[3] < 2 * BP == px[4] < px[5] <= 2 * BP + 4, px
    assert [-(-(h * w) // BP) for h, w in RUNS] == [1, 1, 2, 2, 2, 3]
    B, _, _, hw = CASES["fold"]
    assert BP != 256 or _blocks(B, hw) == [130]
    assert _blocks(B, hw)[0] > 128, "the fold goes past its first and its second round of 64 partials"


@pytest.fixture(autouse=True)
def _needs_a_gpu(dev):
    """(the `dev` fixture skips where no GPU is visible)"""


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _weights(S):
    return [float(F32(0.9 ** s)) for s in range(S)]          # not powers of two: the weighted sum and c_s round


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 host arrays of one case (never modify them): ([err_s], [valid_s], [ident_s] or None, g_loss)"""
    B, n, m, hw = CASES[name]
    rng = np.random.RandomState(11 + sorted(CASES).index(name))
    E, V, I = [], [], []
    for s, (h, w) in enumerate(hw):
        P = h * w
        e = rng.uniform(0.05, 1.0, (B, n, P)).astype(F32)
        v = (rng.uniform(size=(B, n, P)) < 0.8).astype(F32)
        i = rng.uniform(0.05, 1.2, (B, max(m, 1), P)).astype(F32)
        pick = lambda: rng.choice(P, size=max(1, min(6, P // 8)), replace=False)
        q = pick()                                   # ties at the minimum, all sources valid: the first index wins
        e[:, :, q], v[:, :, q] = 0.01, 1
        e[:, rng.randint(n), pick()] = np.nan        # a NaN and a +inf entry never win
        e[:, rng.randint(n), pick()] = np.inf
        q = pick()                                   # no finite source at all
        e[:, :, q] = np.nan
        e[:, n - 1, q] = np.inf
        v[:, :, pick()] = 0                          # every source invalid
        i[:, m - 1 if m else 0, pick()] = np.nan     # NaN and +inf in ident are no floor
        i[:, 0, pick()] = np.inf
        q = pick()                                   # best == floor: not kept
        e[:, :, q], v[:, :, q], i[:, :, q] = 0.3, 1, 0.5
        i[:, 0, q] = 0.3
        if NOTHING_KEPT.get(name) == s:
            e[:] = np.inf
        E.append(e.reshape(B, n, h, w)), V.append(v.reshape(B, n, h, w)), I.append(i.reshape(B, max(m, 1), h, w))
    return E, V, (I if m else None), rng.standard_normal(len(hw) + 1).astype(F32)


def _variant(name, valid, ident):
    E, V, I, g_loss = inputs(name)
    return E, [v if VALID[valid](s) else None for s, v in enumerate(V)], (I if ident else None), g_loss


@functools.lru_cache(maxsize=None)
def reference(name, valid, ident, norm):
    E, V, I, g_loss = _variant(name, valid, ident)
    w = _weights(len(E))
    loss, count, winners = R.forward(E, V, I, w, NORMS[norm])
    return loss, count, winners, R.backward(winners, count, g_loss, E[0].shape[1], w, NORMS[norm])


@functools.lru_cache(maxsize=None)
def gpu(name, valid, ident, norm):
    E, V, I, g_loss = _variant(name, valid, ident)
    w = _weights(len(E))
    loss, count, winners = ops.min_reproj_fwd([_t(e) for e in E], [None if v is None else _t(v) for v in V],
                                              None if I is None else [_t(i) for i in I], w, norm)
    g = ops.min_reproj_bwd(winners, count, _t(g_loss), E[0].shape[1], w, norm, [e.shape[2:] for e in E])
    return loss.cpu().numpy(), count.cpu().numpy(), [t.cpu().numpy() for t in winners], [t.cpu().numpy() for t in g]


VARIANTS = [(name, valid, ident, norm) for name in sorted(CASES) for valid in sorted(VALID) for ident in ((False, True) if CASES[name][2] else (False,))
            for norm in sorted(NORMS)]


# ------------------------------------------------------------------------------------------------------------------------
# 1. + 2. forward and backward against the reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,valid,ident,norm", VARIANTS)
def test_forward_and_backward_against_the_reference(name, valid, ident, norm):
    loss, count, winners, g = gpu(name, valid, ident, norm)
    want_loss, want_count, want_winners, want_g = reference(name, valid, ident, norm)
    S = len(winners)
    assert count.dtype == np.int32 and np.array_equal(count, want_count), (count, want_count)
    for s in range(S):
        assert winners[s].dtype == np.int8 and np.array_equal(winners[s], want_winners[s]), "scale %d: %d winners differ" % (
            s, (winners[s] != want_winners[s]).sum())
    assert loss.dtype == F32 and loss.shape == (S + 1,)
    for s in range(S + 1):
        print("min_reproj %s valid=%s ident=%s norm=%s loss[%d]: gpu %.9g, reference %.17g" % (name, valid, ident, norm, s, loss[s], want_loss[s]))
        assert R.within_one_ulp(loss[s], want_loss[s]), (s, loss[s], want_loss[s])
    for s in range(S):
        assert g[s].dtype == F32 and g[s].shape == want_g[s].shape
        assert np.array_equal(g[s].view(np.int32), want_g[s].view(np.int32)), "scale %d: %d of %d gradient words differ" % (
            s, (g[s].view(np.int32) != want_g[s].view(np.int32)).sum(), g[s].size)
    # the case is what it says: something is kept and something dropped, the planted scale keeps nothing and stays finite
    if name != "3x3":
        assert 0 < count.sum() and any(0 < c < w.size for c, w in zip(count, winners))
    if name in NOTHING_KEPT:
        s = NOTHING_KEPT[name]
        assert count[s] == 0 and loss[s] == 0 and (g[s] == 0).all() and np.isfinite(loss).all()


# ------------------------------------------------------------------------------------------------------------------------
# 3. determinism and contract
# ------------------------------------------------------------------------------------------------------------------------
def _arena_run(name, valid, ident, norm, ws_word):
    """Both calls on guarded buffers through the C ABI, the workspace filled with `ws_word`
    -> (loss bits, count, [winner bytes], [g_err bits])"""
    E, V, I, g_loss = _variant(name, valid, ident)
    B, n, m, hw = CASES[name]
    m = m if I is not None else 0
    S = len(hw)
    d = _lib.SfmMinReprojDesc()
    d.B, d.n_err, d.n_ident, d.n_scales, d.norm = B, n, m, S, NORMS[norm]
    for s, ((h, w), wt) in enumerate(zip(hw, _weights(S))):
        d.H[s], d.W[s], d.weight[s] = h, w, wt
    nbytes = _lib.lib.sfm_min_reproj_workspace_bytes(C.byref(d))
    assert nbytes % 256 == 0 and nbytes >= 12 * sum(_blocks(B, hw))
    specs = [("loss", (S + 1,), 4), ("count", (S,), 8), ("g_loss", (S + 1,), 12), ("ws", nbytes, "ws")]
    for s, (h, w) in enumerate(hw):
        specs += [("err%d" % s, (B, n, h, w), 4 * (s % 4)), ("g%d" % s, (B, n, h, w), 4 * ((s + 1) % 4)),
                  ("win%d" % s, (-(-(B * h * w) // 4),), 4 * ((s + 2) % 4))]      # int8 (B,h,w) in whole words: the tail stays sentinel
        if V[s] is not None:
            specs.append(("valid%d" % s, (B, n, h, w), 8))
        if m:
            specs.append(("ident%d" % s, (B, m, h, w), 12))
    ar = Arena(DEV, specs, row_floats=max(w for _, w in hw))
    inputs_ = ["g_loss"]
    ar.set("g_loss", g_loss)
    ar.fill_bits("ws", ws_word)
    for s in range(S):
        ar.set("err%d" % s, E[s])
        inputs_.append("err%d" % s)
        d.err[s], d.g_err[s], d.winner[s] = ar.ptr("err%d" % s), ar.ptr("g%d" % s), ar.ptr("win%d" % s)
        if V[s] is not None:
            ar.set("valid%d" % s, V[s])
            inputs_.append("valid%d" % s)
            d.valid[s] = ar.ptr("valid%d" % s)
        if m:
            ar.set("ident%d" % s, I[s])
            inputs_.append("ident%d" % s)
            d.ident[s] = ar.ptr("ident%d" % s)
    d.loss, d.count, d.g_loss = ar.ptr("loss"), ar.ptr("count"), ar.ptr("g_loss")
    for key in inputs_:
        ar.snapshot(key)
    _lib.check(_lib.lib.sfm_min_reproj_fwd(C.byref(d), C.c_void_p(ar.ptr("ws")), nbytes, ops._stream()))
    _lib.check(_lib.lib.sfm_min_reproj_bwd(C.byref(d), ops._stream()))
    torch.cuda.synchronize()
    what = "%s valid=%s ident=%s norm=%s" % (name, valid, ident, norm)
    ar.check(what)                                    # nothing before or behind any array: loss ends after n_scales + 1 floats
    assert ar.sentinels_left("loss") == 0 and ar.sentinels_left("count") == 0, what
    for key in inputs_:
        ar.unchanged(key)
    winners, g = [], []
    word = np.frombuffer(np.array([SENTINEL], np.int32).tobytes(), np.int8)      # the bytes of one sentinel word
    for s, (h, w) in enumerate(hw):
        assert ar.sentinels_left("g%d" % s) == 0, "%s scale %d: an element of g_err was not written" % (what, s)
        raw = ar.bits("win%d" % s).view(np.int8)
        used = B * h * w
        assert np.array_equal(raw[used:], word[used % 4:] if used % 4 else word[:0]), "%s scale %d: bytes behind winner were written" % (what, s)
        assert ((raw[:used] >= -1) & (raw[:used] < n)).all(), "%s scale %d: a winner was not written" % (what, s)
        winners.append(raw[:used].reshape(B, h, w).copy())
        g.append(ar.bits("g%d" % s))
    return ar.bits("loss"), ar.bits("count"), winners, g


@pytest.mark.parametrize("name,valid,ident,norm", [v for v in VARIANTS if v[1] == "subset" and v[2] == bool(CASES[v[0]][2])])
def test_buffer_contract(name, valid, ident, norm):
    """Sentinel-filled outputs are overwritten completely -- every element of g_err, winner, loss and count --, the guard bands around
    every array and the workspace stay untouched (so does the rest of the last word behind an int8 map), the inputs keep their bits;
    two calls whose workspaces held different garbage agree bit for bit, and with what ops returns"""
    first = _arena_run(name, valid, ident, norm, SENTINEL)
    again = _arena_run(name, valid, ident, norm, 0xFFFFFFFF)          # as fp64 sums: NaN; as counts: -1
    loss, count, winners, g = gpu(name, valid, ident, norm)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[0], loss.view(np.int32))
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[1], count)
    for s in range(len(winners)):
        assert np.array_equal(first[2][s], again[2][s]) and np.array_equal(first[2][s], winners[s]), s
        assert np.array_equal(first[3][s], again[3][s]) and np.array_equal(first[3][s], g[s].view(np.int32)), s


def test_min_reprojection_autograd():
    """torch_api.min_reprojection: both outputs carry a gradient to errs and to nothing else; bf16 maps get bf16 gradients"""
    name, valid, ident, norm = "max", "subset", True, "kept"
    E, V, I, g_loss = _variant(name, valid, ident)
    S, w = len(E), _weights(len(E))
    errs = [_t(e).requires_grad_() for e in E]
    valids = [None if v is None else _t(v).requires_grad_() for v in V]
    total, per_scale, winners = ta.min_reprojection(errs, valid=valids, ident=[_t(i) for i in I], weights=w, norm=norm)
    loss, count, want_winners, want_g = gpu(name, valid, ident, norm)
    assert total.dim() == 0 and _bits(total, _t(loss)[S]) and _bits(per_scale, _t(loss)[:S])
    assert all(t.dtype == torch.int8 and not t.requires_grad and np.array_equal(t.cpu().numpy(), x) for t, x in zip(winners, want_winners))
    (total * float(g_loss[S]) + (per_scale * _t(g_loss[:S])).sum()).backward()
    for s in range(S):
        assert np.array_equal(errs[s].grad.cpu().numpy().view(np.int32), want_g[s].view(np.int32)), s
        assert valids[s] is None or valids[s].grad is None
    half = [_t(e).to(torch.bfloat16).requires_grad_() for e in E]
    ta.min_reprojection(half, weights=w)[0].backward()
    assert all(t.grad is not None and t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape for t in half)
    assert not ta.min_reprojection([e.detach() for e in errs])[0].requires_grad


# ------------------------------------------------------------------------------------------------------------------------
# 4. + 5. the composite
# ------------------------------------------------------------------------------------------------------------------------
STEPS = {"40x130": dict(B=2, H=40, W=130, n_src=2, n_scales=2), "24x56": dict(B=1, H=24, W=56, n_src=3, n_scales=3)}


def _step_inputs(step):
    d = synth.make_inputs(seed=21, **STEPS[step])
    t = lambda a: _t(np.ascontiguousarray(a, dtype=F32))
    return dict(src=t(d["src"]), tgt=t(d["tgt"]), K=t(d["intrinsics"]), disps=[t(a) for a in d["disps"]], poses=[t(a) for a in d["poses"]])


@pytest.mark.parametrize("auto_mask", [True, False])
@pytest.mark.parametrize("alpha", [0.0, 0.85])
@pytest.mark.parametrize("step", sorted(STEPS))
def test_composite_is_its_stages(step, alpha, auto_mask):
    """min_reprojection_loss is, bit for bit in total, d_disp and d_pose, the chain run by hand through ops.*"""
    x = _step_inputs(step)
    src, tgt, K, disps, poses = x["src"], x["tgt"], x["K"], x["disps"], x["poses"]
    B, n_src, _, H, W = src.shape
    S = len(disps)
    leaves = [t.requires_grad_() for t in disps + poses]
    total = ta.min_reprojection_loss(tgt, src, K, disps, poses, ssim_rate=alpha, auto_mask=auto_mask)
    assert total.dim() == 0 and total.dtype == torch.float32 and total.grad_fn is not None
    got = torch.autograd.grad(total, leaves)

    with torch.no_grad():
        w = [2.0 ** -s for s in range(S)]
        stacked = src.view(B, 3 * n_src, H, W)
        pyr = ops.pyramid_hwc(stacked, S)
        warped, valid = ops.warp_pyramid_fwd(pyr, disps, poses, K, "hwc", True)
        tgts = ops.pyramid(tgt, S)
        errs = ops.photo_error_fwd(warped, tgts, alpha)
        idents = ops.photo_error_fwd([p.view(B, n_src, 3, H >> s, W >> s) for s, p in enumerate(ops.pyramid(stacked, S))], tgts, alpha) if auto_mask else None
        loss, count, winners = ops.min_reproj_fwd(errs, valid, idents, w, "kept")
        g_loss = torch.zeros(S + 1, device=DEV)
        g_loss[S] = 1
        g_errs = ops.min_reproj_bwd(winners, count, g_loss, n_src, w, "kept", [(H >> s, W >> s) for s in range(S)])
        d_disps, d_poses = ops.warp_pyramid_bwd(pyr, disps, poses, K, "hwc", ops.photo_error_bwd(warped, tgts, alpha, g_errs))
    assert _bits(total.detach(), loss[S])
    for k, (a, b) in enumerate(zip(got, d_disps + d_poses)):
        assert _bits(a, b), k
    # (a sanity check of the inputs, not of the library: with the auto-mask a coarse scale of a small frame may keep pixels of one
    #  source only, or -- 24x56 at alpha = 0.85, scale 2 -- none at all, which the mean has to survive)
    assert float(total.detach()) > 0 and all(bool(torch.isfinite(t).all()) for t in got) and 0 < int(count[0])
    assert float(got[0].abs().max()) > 0 and any(float(t.abs().max()) > 0 for t in got[S:])
    assert any(int((wn < 0).sum()) > 0 for wn in winners), "something is dropped"


def _example_with_a_float64_tail(x, alpha, tail):
    """INTEGRATION.md's min_reprojection_loss_ssim; tail: the dtype its last where / sum / divide runs in
    -> (total, [best], [keep], [index of the minimum], [is the minimum unique], [reproj], [valid], [ident])"""
    src, tgt = x["src"], x["tgt"]
    B, n_src, _, H, W = src.shape
    S = len(x["disps"])
    warped, valid = ta.warp_pyramid(src, x["K"], x["disps"], x["poses"], return_valid=True)
    unwarped = [p.view(B, n_src, 3, H >> s, W >> s) for s, p in enumerate(ops.pyramid(src.view(B, 3 * n_src, H, W), S))]
    reproj = ta.photometric_error(warped, tgt, ssim_rate=alpha)
    with torch.no_grad():
        ident = ta.photometric_error(unwarped, tgt, ssim_rate=alpha)
    total, bests, keeps, idx, unique = 0.0, [], [], [], []
    for s, (e, v, e0) in enumerate(zip(reproj, valid, ident)):
        e = torch.where(v > 0, e, torch.full_like(e, float("inf")))
        best, i = e.min(1)
        keep = best < e0.min(1).values
        total = total + torch.where(keep, best, torch.zeros_like(best)).to(tail).sum() / keep.sum().clamp(min=1) / 2 ** s
        bests.append(best.detach()), keeps.append(keep), idx.append(i), unique.append((e == best[:, None]).sum(1) == 1)
    return total, bests, keeps, idx, unique, reproj, valid, ident


@pytest.mark.parametrize("alpha", [0.0, 0.85])
@pytest.mark.parametrize("step", sorted(STEPS))
def test_composite_against_the_example_in_aten(step, alpha):
    x = _step_inputs(step)
    leaves = [t.requires_grad_() for t in x["disps"] + x["poses"]]
    S = len(x["disps"])
    total = ta.min_reprojection_loss(x["tgt"], x["src"], x["K"], x["disps"], x["poses"], ssim_rate=alpha)
    got = torch.autograd.grad(total, leaves)
    t64, bests, keeps, idx, unique, reproj, valid, ident = _example_with_a_float64_tail(x, alpha, torch.float64)
    g64 = torch.autograd.grad(t64, leaves)
    t32 = _example_with_a_float64_tail(x, alpha, torch.float32)[0]
    g32 = torch.autograd.grad(t32, leaves)
    # the selection: the same keep mask, the same best values, the same source wherever the minimum is unique
    mine, per_scale, winners = ta.min_reprojection([e.detach() for e in reproj], valid=valid, ident=ident)
    assert _bits(mine, total.detach())
    for s in range(S):
        kept = winners[s] >= 0
        assert torch.equal(kept, keeps[s]) and int(kept.sum()) < kept.numel(), s
        taken = reproj[s].detach().gather(1, winners[s].clamp(min=0).long()[:, None])[:, 0]
        assert torch.equal(taken[kept].view(torch.int32), bests[s][kept].view(torch.int32)), s
        same = kept & unique[s]
        assert torch.equal(winners[s][same].long(), idx[s][same]) and (s > 0 or int(same.sum()) > 0), s
    want = float(t64.detach())
    ulps = abs(float(total.detach()) - want) / float(np.spacing(F32(want)))
    line = "min_reprojection_loss %s alpha=%g: total %.9g, float64 tail %.17g (%.3g ulp), float32 tail %.9g" % (step, alpha, float(total.detach()), want, ulps, float(t32.detach()))
    print(line)
    parity_note(line)
    assert ulps <= 2, line
    for k, (g, r, b) in enumerate(zip(got, g64, g32)):
        name = "d_disp[%d]" % k if k < S else "d_pose[%d]" % (k - S)
        _within(g.cpu().numpy(), r.cpu().numpy().astype(F64), b.cpu().numpy(), "min_reprojection_loss %s alpha=%g %s" % (step, alpha, name))


# ------------------------------------------------------------------------------------------------------------------------
# 6. dtypes and capture
# ------------------------------------------------------------------------------------------------------------------------
def test_dtypes_no_sync_and_graph_capture():
    x = _step_inputs("40x130")
    args = lambda disps, poses: (x["tgt"], x["src"], x["K"], disps, poses)
    # bfloat16 disparities get bfloat16 gradients, a packed pose tensor its own shape; the frames and the intrinsics get none
    disps = [t.to(torch.bfloat16).requires_grad_() for t in x["disps"]]
    packed = torch.cat(x["poses"], dim=1).requires_grad_()
    tgt = x["tgt"].clone().requires_grad_()
    total = ta.min_reprojection_loss(tgt, x["src"], x["K"], disps, packed, ssim_rate=0.85)
    assert total.dtype == torch.float32
    total.backward()
    assert all(t.grad is not None and t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape for t in disps)
    assert packed.grad is not None and packed.grad.shape == packed.shape and tgt.grad is None
    with pytest.raises(TypeError, match="intrinsics"):
        ta.min_reprojection_loss(*args(x["disps"], x["poses"])[:2], x["K"].clone().requires_grad_(), x["disps"], x["poses"], ssim_rate=0.85)
    with pytest.raises(ValueError, match="norm"):
        ta.min_reprojection_loss(*args(x["disps"], x["poses"]), ssim_rate=0.85, norm="mean")
    with pytest.raises(ValueError, match="weight"):
        ta.min_reprojection_loss(*args(x["disps"], x["poses"]), ssim_rate=0.85, weights=[1.0, -1.0])
    # "all": the same selection over all pixels -- never more than "kept", which divides by fewer
    with torch.no_grad():
        kept = ta.min_reprojection_loss(*args(x["disps"], x["poses"]), ssim_rate=0.85)
        every = ta.min_reprojection_loss(*args(x["disps"], x["poses"]), ssim_rate=0.85, norm="all")
    assert not kept.requires_grad and 0 < float(every) < float(kept)

    leaves = x["disps"] + x["poses"]

    def step():
        for t in leaves:
            t.grad = None
        loss = ta.min_reprojection_loss(*args(x["disps"], x["poses"]), ssim_rate=0.85)
        loss.backward()
        return [loss.detach()] + [t.grad for t in leaves]

    for t in leaves:
        t.requires_grad_()
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
    assert all(_bits(a, b) for a, b in zip(eager, captured))
    assert float(eager[0]) > 0 and float(eager[1].abs().max()) > 0 and any(float(t.abs().max()) > 0 for t in eager[3:])
