"""sfm_pairwise_fwd / _bwd, torch_api.pairwise_mean and torch_api.sc_sfm_loss on the GPU.

The reference is tests/sc_pairwise_ref.py, the formulas of include/sfmwarp_pairwise.h in NumPy.  Every selection and every gradient
element is float32 arithmetic on float32 values in a stated order, so keep, count, g_err and g_diff are compared EXACTLY.  The sums:
the kernel adds positive float32 terms in fp64 in its own order, the reference in NumPy's, so each fp64 sum differs far below half a
float32 ulp and a scalar by its final rounding alone: 1 float32 ulp.

Shapes: maps of 3x3 (9 px, below one wavefront), 16x17 (one run of 256 plus 16), 5x103 (two runs plus 3) and 48x120 with B = 3 (23
runs per sample, 69 per (scale, source): the fold's second round of 64), with 1 and 4 sources, and 1 and 4 scales of unrelated sizes
in one call."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

import sc_pairwise_ref as R
from util import Arena, SENTINEL, parity_note

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
synth = importlib.import_module("sfm-learner-chainer_amd.synth")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
BP = int(re.search(r"constexpr int PW_BLOCK_PIXELS = (\d+);",
                   open(os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", "sfm_pairwise.hip")).read()).group(1))

# (B, n_src, [(h, w)])
CASES = {
    "3x3": (1, 1, [(3, 3)]),
    "fold": (3, 1, [(48, 120)]),
    "all": (3, 4, [(16, 17), (48, 120), (3, 3), (5, 103)]),
}
# (valid: which scales have one, ident, cmp)
VARIANTS = {"plain": (lambda s: True, False, False), "valid_some": (lambda s: s % 2 == 1, False, False),
            "ident": (lambda s: True, True, False), "ident_cmp": (lambda s: s != 2, True, True)}


def test_the_shapes_are_the_ones_the_kernels_can_go_wrong_at():
    assert BP == 256
    runs = lambda h, w: -(-(h * w) // BP)
    assert [(h * w, runs(h, w)) for h, w in CASES["all"][2]] == [(BP + 16, 2), (22 * BP + 128, 23), (9, 1), (2 * BP + 3, 3)]
    assert CASES["all"][0] * runs(48, 120) == 69 > 64, "the fold's lanes 0..4 go round a second time"


@pytest.fixture(autouse=True)
def _needs_a_gpu(dev):
    """(the `dev` fixture skips where no GPU is visible)"""


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ts(arrays):
    return None if arrays is None else [None if a is None else _t(a) for a in arrays]


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(a, b):
    """two host arrays hold the same bits"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _weights(S):
    return [float(F32(0.9 ** s)) for s in range(S)]          # not powers of two: the weighted sums and cp, cg round


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 host arrays of one case (never modify them), ties c == ident planted for both forms of the auto-mask"""
    B, n, hw = CASES[name]
    x = R.inputs(B, n, hw, seed=31 + sorted(CASES).index(name))
    rng = np.random.RandomState(5)
    for s, (h, w) in enumerate(hw):
        P = h * w
        q = rng.choice(P, size=max(1, P // 16), replace=False)
        for key in ("errs", "cmps", "idents"):
            flat = x[key][s].reshape(B, n, P)
            flat[:, :, q] = F32(0.25)                        # err == cmp == ident: dropped under either form
        if x["valids"][s] is not None:
            x["valids"][s].reshape(B, n, P)[:, :, q] = 1
    N = len(hw) * n
    x["g_loss"] = np.random.RandomState(9).uniform(0.2, 1.5, 2 * N + 2).astype(F32)
    return x


def _variant(name, variant):
    x = inputs(name)
    on, ident, cmp = VARIANTS[variant]
    return (x["errs"], x["diffs"], [v if on(s) else None for s, v in enumerate(x["valids"])], x["idents"] if ident else None,
            x["cmps"] if cmp else None, x["g_loss"])


def run(E, D, V, I, Cm, g_loss, weights, min_counts=(0, 0), detach=False, want_g_diff=True):
    """ops.pairwise_fwd + ops.pairwise_bwd -> host arrays (loss, count, [keep], [g_err], [g_diff] or None)"""
    errs, diffs = _ts(E), _ts(D)
    loss, count, keeps = ops.pairwise_fwd(errs, diffs, _ts(V), _ts(I), _ts(Cm), weights, min_counts, detach)
    g_errs, g_diffs = ops.pairwise_bwd(errs, diffs, keeps, count, _t(g_loss), weights, min_counts, detach, want_g_diff=want_g_diff)
    host = lambda ts: None if ts is None else [t.cpu().numpy() for t in ts]
    return loss.cpu().numpy(), count.cpu().numpy(), host(keeps), host(g_errs), host(g_diffs)


def check(got, E, D, V, I, Cm, g_loss, weights, min_counts=(0, 0), detach=False, what=""):
    """keep, count, g_err, g_diff bit for bit against the restatement, the scalars within 1 ulp"""
    loss, count, keeps, g_errs, g_diffs = got
    w_loss, w_count, w_keeps = R.forward(E, D, V, I, Cm, weights, min_counts)
    w_errs, w_diffs = R.backward(E, D, w_keeps, w_count, g_loss, weights, min_counts, detach)
    assert _same(count, w_count), what
    for s in range(len(E)):
        assert _same(keeps[s], w_keeps[s]), (what, s)
        assert _same(g_errs[s], w_errs[s]), (what, s)
        assert g_diffs is None or _same(g_diffs[s], w_diffs[s]), (what, s)
    worst = float(R.ulp_distance(loss, w_loss).max())
    print("pairwise %s: scalars within %.3g ulp of the restatement" % (what, worst))
    assert worst <= 1, what
    return w_loss, w_count, w_keeps


# ------------------------------------------------------------------------------------------------------------------------
# 1. values at the run-boundary sizes, every form of the selection
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("detach", [False, True], ids=["weight_grad", "detach_weight"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(name, variant, detach):
    E, D, V, I, Cm, g_loss = _variant(name, variant)
    w = _weights(len(E))
    got = run(E, D, V, I, Cm, g_loss, w, detach=detach)
    _, count, keeps = check(got, E, D, V, I, Cm, g_loss, w, detach=detach, what="%s %s detach=%d" % (name, variant, detach))
    if name != "3x3":
        assert count.min() > 0 and all(0 < k.mean() < 1 for k, v in zip(keeps, V) if v is not None or I is not None)
    if I is not None:      # the planted ties are dropped although they are in view
        x = inputs(name)
        for s, k in enumerate(keeps):
            tie = (x["cmps"] if Cm is not None else x["errs"])[s] == x["idents"][s]
            assert tie.any() and not k[tie].any(), s
    # without g_diff: the same g_err
    assert all(_same(a, b) for a, b in zip(run(E, D, V, I, Cm, g_loss, w, detach=detach, want_g_diff=False)[3], got[3]))


# ------------------------------------------------------------------------------------------------------------------------
# 2. selection, not multiplication: non-finite values at dropped and at kept pixels
# ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_values_at_dropped_pixels_change_nothing():
    E, D, V, I, Cm, g_loss = _variant("all", "ident_cmp")
    w = _weights(len(E))
    clean = run(E, D, V, I, Cm, g_loss, w)
    keeps = clean[2]
    E2, D2 = [e.copy() for e in E], [d.copy() for d in D]
    for s, k in enumerate(keeps):
        dropped = np.argwhere(k == 0)
        assert len(dropped) >= 4, s
        for j, bad in enumerate((np.nan, np.inf, -np.inf, np.nan)):
            (E2 if j % 2 == 0 else D2)[s][tuple(dropped[j * (len(dropped) // 4)])] = bad
        b, i, y, x_ = dropped[-1]
        E2[s][b, i, y, x_] = D2[s][b, i, y, x_] = np.nan
    dirty = run(E2, D2, V, I, Cm, g_loss, w)
    assert _same(clean[0], dirty[0]) and _same(clean[1], dirty[1])
    for k in (2, 3, 4):
        assert all(_same(a, b) for a, b in zip(clean[k], dirty[k])), k


@pytest.mark.parametrize("where", ["err", "diff"])
def test_a_nan_at_a_kept_pixel_reaches_its_pair_and_the_totals_only(where):
    E, D, V, I, Cm, g_loss = _variant("all", "plain")
    B, n, hw = CASES["all"]
    S, N = len(hw), len(hw) * n
    w = _weights(S)
    clean = run(E, D, V, I, Cm, g_loss, w)
    s, i = 1, 2
    b, y, x_ = np.argwhere(clean[2][s][:, i] != 0)[7]
    E2, D2 = [e.copy() for e in E], [d.copy() for d in D]
    (E2 if where == "err" else D2)[s][b, i, y, x_] = np.nan
    dirty = run(E2, D2, V, I, Cm, g_loss, w)
    j = s * n + i
    hit = {j, 2 * N} | ({N + j, 2 * N + 1} if where == "diff" else set())      # err reaches the photometric mean alone, diff both
    for k in range(2 * N + 2):
        if k in hit:
            assert np.isnan(dirty[0][k]), k
        else:
            assert dirty[0][k:k + 1].tobytes() == clean[0][k:k + 1].tobytes(), k
    assert _same(clean[1], dirty[1]) and all(_same(a, b) for a, b in zip(clean[2], dirty[2]))
    for k in (3, 4):      # the gradients: that pixel's alone -- g_err = (1 - diff) * cp reads diff, g_diff = cg - err * cp reads err
        for t in range(S):
            same = dirty[k][t].view(np.int32) == clean[k][t].view(np.int32)
            if t == s and (k == 3) == (where == "diff"):
                assert np.isnan(dirty[k][t][b, i, y, x_])
                same[b, i, y, x_] = True
            assert same.all(), (k, t)


# ------------------------------------------------------------------------------------------------------------------------
# 3. the thresholds of mean_on_mask
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["photo", "geom"])
def test_a_mean_needs_more_than_min_count_pixels(which):
    E, D, V, I, Cm, g_loss = _variant("all", "ident")
    B, n, hw = CASES["all"]
    S, N = len(hw), len(hw) * n
    w = _weights(S)
    base = run(E, D, V, I, Cm, g_loss, w)
    count = base[1]
    s, i = 3, 1
    j = s * n + i
    c = int(count[j])
    assert 1 < c < count.max(), "other pairs keep more pixels than this one"
    own, other = (slice(0, N), slice(N, 2 * N)) if which == "photo" else (slice(N, 2 * N), slice(0, N))
    for m, on in ((c, False), (c - 1, True)):
        mc = (m, 0) if which == "photo" else (0, m)
        got = run(E, D, V, I, Cm, g_loss, w, min_counts=mc)
        check(got, E, D, V, I, Cm, g_loss, w, min_counts=mc, what="min_count_%s=%d (count %d)" % (which, m, c))
        loss = got[0]
        assert _same(loss[other], base[0][other]), "the other threshold is independent"
        assert _same(got[1], count) and all(_same(a, b) for a, b in zip(got[2], base[2]))
        if on:      # count == min_count + 1: the mean
            assert loss[own][j] == base[0][own][j] != 0
            assert _same(got[3][s][:, i], base[3][s][:, i]) and _same(got[4][s][:, i], base[4][s][:, i])
        else:       # count == min_count: exactly 0, and so are its gradients (g_diff keeps the other term's)
            assert loss[own][j] == 0
            if which == "photo":
                assert not got[3][s][:, i].any(), "g_err of the pair is exactly 0"
                cg = got[4][s][:, i][base[2][s][:, i] != 0]
                assert (cg == cg[0]).all() and cg[0] != 0, "g_diff is cg alone"
            else:
                assert _same(got[3][s][:, i], base[3][s][:, i])
        for t in range(S):      # pairs above the threshold are what they were
            for u in range(n):
                if count[t * n + u] > m:
                    assert _same(got[3][t][:, u], base[3][t][:, u]) and _same(got[4][t][:, u], base[4][t][:, u]), (t, u)
    both = run(E, D, V, I, Cm, g_loss, w, min_counts=(c, c))
    assert both[0][j] == 0 and both[0][N + j] == 0 and not both[3][s][:, i].any() and not both[4][s][:, i].any()


def test_nothing_kept():
    E, D, V, I, Cm, g_loss = _variant("all", "plain")
    B, n, hw = CASES["all"]
    N = len(hw) * n
    w = _weights(len(hw))
    V = [v.copy() for v in V]
    V[0][:, 1] = 0
    V[2][:] = -1.0
    got = run(E, D, V, I, Cm, g_loss, w)
    check(got, E, D, V, I, Cm, g_loss, w, what="nothing kept")
    for j in [0 * n + 1] + [2 * n + u for u in range(n)]:
        assert got[1][j] == 0 and got[0][j] == 0 and got[0][N + j] == 0
    assert not got[3][0][:, 1].any() and not got[4][0][:, 1].any() and not got[3][2].any() and not got[4][2].any() and not got[2][2].any()
    assert np.isfinite(got[0]).all()


# ------------------------------------------------------------------------------------------------------------------------
# 4. the buffer contract
# ------------------------------------------------------------------------------------------------------------------------
def _arena_run(name, variant, ws_word):
    E, D, V, I, Cm, g_loss = _variant(name, variant)
    B, n, hw = CASES[name]
    S, N = len(hw), len(hw) * n
    d = _lib.SfmPairwiseDesc()
    d.B, d.n_src, d.n_scales = B, n, S
    for s, ((h, w), wt) in enumerate(zip(hw, _weights(S))):
        d.H[s], d.W[s], d.weight[s] = h, w, wt
    nbytes = _lib.lib.sfm_pairwise_workspace_bytes(C.byref(d))
    assert nbytes % 256 == 0 and nbytes >= 20 * n * sum(B * -(-(h * w) // BP) for h, w in hw)
    specs = [("loss", (2 * N + 2,), 4), ("count", (N,), 8), ("g_loss", (2 * N + 2,), 12), ("ws", nbytes, "ws")]
    maps = {"err": E, "diff": D, "valid": V, "ident": I, "cmp": Cm}
    for s, (h, w) in enumerate(hw):
        for k, key in enumerate(maps):
            if maps[key] is not None and maps[key][s] is not None:
                specs.append(("%s%d" % (key, s), (B, n, h, w), 4 * ((s + k) % 4)))
        specs += [("g_err%d" % s, (B, n, h, w), 4 * ((s + 1) % 4)), ("g_diff%d" % s, (B, n, h, w), 4 * ((s + 3) % 4)),
                  ("keep%d" % s, (-(-(B * n * h * w) // 4),), 4 * ((s + 2) % 4))]      # int8 in whole words: the tail stays sentinel
    ar = Arena(DEV, specs, row_floats=max(w for _, w in hw))
    held = ["g_loss"]
    ar.set("g_loss", g_loss)
    ar.fill_bits("ws", ws_word)
    for s in range(S):
        for key, arrays in maps.items():
            if arrays is not None and arrays[s] is not None:
                ar.set("%s%d" % (key, s), arrays[s])
                held.append("%s%d" % (key, s))
                getattr(d, key)[s] = ar.ptr("%s%d" % (key, s))
        d.keep[s], d.g_err[s], d.g_diff[s] = ar.ptr("keep%d" % s), ar.ptr("g_err%d" % s), ar.ptr("g_diff%d" % s)
    d.loss, d.count, d.g_loss = ar.ptr("loss"), ar.ptr("count"), ar.ptr("g_loss")
    for key in held:
        ar.snapshot(key)
    _lib.check(_lib.lib.sfm_pairwise_fwd(C.byref(d), C.c_void_p(ar.ptr("ws")), nbytes, ops._stream()))
    _lib.check(_lib.lib.sfm_pairwise_bwd(C.byref(d), ops._stream()))
    torch.cuda.synchronize()
    what = "%s %s" % (name, variant)
    ar.check(what)                                    # nothing before or behind any array: loss ends after 2N + 2 floats
    assert ar.sentinels_left("loss") == 0 and ar.sentinels_left("count") == 0, what
    for key in held:
        ar.unchanged(key)
    keeps, g_errs, g_diffs = [], [], []
    word = np.frombuffer(np.array([SENTINEL], np.int32).tobytes(), np.int8)      # the bytes of one sentinel word
    for s, (h, w) in enumerate(hw):
        assert ar.sentinels_left("g_err%d" % s) == 0 and ar.sentinels_left("g_diff%d" % s) == 0, "%s scale %d: an element was not written" % (what, s)
        raw = ar.bits("keep%d" % s).view(np.int8)
        used = B * n * h * w
        assert np.array_equal(raw[used:], word[used % 4:] if used % 4 else word[:0]), "%s scale %d: bytes behind keep were written" % (what, s)
        assert ((raw[:used] == 0) | (raw[:used] == 1)).all(), "%s scale %d: a keep was not written" % (what, s)
        keeps.append(raw[:used].reshape(B, n, h, w).copy())
        g_errs.append(ar.bits("g_err%d" % s)), g_diffs.append(ar.bits("g_diff%d" % s))
    return ar.bits("loss"), ar.bits("count"), keeps, g_errs, g_diffs


@pytest.mark.parametrize("name,variant", [("3x3", "plain"), ("all", "ident_cmp"), ("all", "valid_some")])
def test_buffer_contract(name, variant):
    """Sentinel-filled outputs are overwritten completely, the guard words around every array and the workspace stay untouched (so
    does the rest of the last word behind an int8 map), the inputs keep their bits; two calls whose workspaces held different
    garbage (NaN bytes among them) agree bit for bit, and with what ops returns"""
    first = _arena_run(name, variant, SENTINEL)
    again = _arena_run(name, variant, 0xFFFFFFFF)          # as fp64 sums: NaN; as counts: -1
    E, D, V, I, Cm, g_loss = _variant(name, variant)
    loss, count, keeps, g_errs, g_diffs = run(E, D, V, I, Cm, g_loss, _weights(len(E)))
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[0], loss.view(np.int32))
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[1], count)
    for s in range(len(keeps)):
        assert np.array_equal(first[2][s], again[2][s]) and np.array_equal(first[2][s], keeps[s]), s
        assert np.array_equal(first[3][s], again[3][s]) and np.array_equal(first[3][s], g_errs[s].view(np.int32)), s
        assert np.array_equal(first[4][s], again[4][s]) and np.array_equal(first[4][s], g_diffs[s].view(np.int32)), s


def test_the_empty_batch():
    d = _lib.SfmPairwiseDesc()
    d.B, d.n_src, d.n_scales, d.H[0], d.W[0] = 0, 2, 1, 8, 8
    assert _lib.lib.sfm_pairwise_fwd(C.byref(d), None, 0, ops._stream()) == 0 and _lib.lib.sfm_pairwise_bwd(C.byref(d), ops._stream()) == 0
    e = torch.zeros((0, 2, 8, 8), device=DEV)
    loss, count, keeps = ops.pairwise_fwd([e], [e], None, None, None, [1.0], (0, 0), False)
    assert not loss.cpu().numpy().any() and not count.cpu().numpy().any() and tuple(keeps[0].shape) == (0, 2, 8, 8)


# ------------------------------------------------------------------------------------------------------------------------
# 5. torch_api.pairwise_mean
# ------------------------------------------------------------------------------------------------------------------------
def test_pairwise_mean_autograd():
    """all four scalars carry a gradient to errs and diffs and to nothing else, bit for bit ops.pairwise_bwd; bf16 maps get bf16
    gradients; upstream gradients that are None are zeros"""
    E, D, V, I, Cm, g_loss = _variant("all", "ident_cmp")
    B, n, hw = CASES["all"]
    S, N = len(hw), len(hw) * n
    w = _weights(S)
    for detach in (False, True):
        errs, diffs = [_t(e).requires_grad_() for e in E], [_t(d).requires_grad_() for d in D]
        valids = [None if v is None else _t(v).requires_grad_() for v in V]
        idents = [_t(a).requires_grad_() for a in I]
        pt, gt, p, g, keeps = ta.pairwise_mean(errs, diffs, valid=valids, ident=idents, cmp=_ts(Cm), weights=w, detach_weight=detach)
        loss, count, w_keeps, w_errs, w_diffs = run(E, D, V, I, Cm, g_loss, w, detach=detach)
        assert pt.dim() == 0 and gt.dim() == 0 and tuple(p.shape) == (S, n) == tuple(g.shape)
        assert _bits(torch.cat([p.reshape(-1), g.reshape(-1), pt.reshape(1), gt.reshape(1)]).detach(), _t(loss))
        assert all(t.dtype == torch.int8 and not t.requires_grad and _same(t.cpu().numpy(), k) for t, k in zip(keeps, w_keeps))
        gl = _t(g_loss)
        ((p.reshape(-1) * gl[:N]).sum() + (g.reshape(-1) * gl[N:2 * N]).sum() + pt * gl[2 * N] + gt * gl[2 * N + 1]).backward()
        for s in range(S):
            assert _same(errs[s].grad.cpu().numpy(), w_errs[s]) and _same(diffs[s].grad.cpu().numpy(), w_diffs[s]), (detach, s)
            assert (valids[s] is None or valids[s].grad is None) and idents[s].grad is None
    # None upstream: the photometric total alone, and diffs that want no gradient
    errs, diffs = [_t(e).requires_grad_() for e in E], _ts(D)
    ta.pairwise_mean(errs, diffs, valid=_ts(V), weights=w)[0].backward()
    only = g_loss * 0
    only[2 * N] = 1
    want = run(E, D, V, None, None, only, w)[3]
    assert all(_same(t.grad.cpu().numpy(), a) for t, a in zip(errs, want))
    half_e, half_d = [_t(e).to(torch.bfloat16).requires_grad_() for e in E], [_t(d).to(torch.bfloat16).requires_grad_() for d in D]
    out = ta.pairwise_mean(half_e, half_d)
    assert out[0].dtype == torch.float32
    (out[0] + out[1]).backward()
    assert all(t.grad is not None and t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape for t in half_e + half_d)
    assert not ta.pairwise_mean(_ts(E), _ts(D))[0].requires_grad
    unweighted = ta.pairwise_mean(_ts(E), _ts(D), valid=_ts(V))
    assert _bits(unweighted[0], _t(run(E, D, V, None, None, g_loss, [1.0] * S)[0])[2 * N]), "weights=None is 1.0 per scale"
    with pytest.raises(ValueError, match="weight"):
        ta.pairwise_mean(_ts(E), _ts(D), weights=[1.0, -1.0, 1.0, 1.0])


def test_pairwise_mean_reads_nothing_on_the_host_and_is_captured():
    E, D, V, I, Cm, g_loss = _variant("all", "ident")
    errs, diffs = [_t(e).requires_grad_() for e in E], [_t(d).requires_grad_() for d in D]
    valids, idents = _ts(V), _ts(I)
    leaves = errs + diffs

    def step():
        for t in leaves:
            t.grad = None
        pt, gt, p, g, keeps = ta.pairwise_mean(errs, diffs, valid=valids, ident=idents, min_count=(5, 7))
        (pt + 0.5 * gt).backward()
        return [pt.detach(), gt.detach(), p.detach(), g.detach()] + [t.grad for t in leaves]

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
    with torch.cuda.graph(graph):      # one stream: the capture has no parallel branches
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bits(a, b) for a, b in zip(eager, captured))
    assert float(eager[0]) > 0 and float(eager[4].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------
# 6. torch_api.sc_sfm_loss: 24x40, 2 scales, 2 sources, B = 2
# ------------------------------------------------------------------------------------------------------------------------
STEP = dict(B=2, H=24, W=40, n_src=2, n_scales=2)
SCATTER_TOL = 64 * float(np.finfo(F32).eps)      # an element of d_src_disp: a few tens of float atomics in any order, of max|d_src_disp|


def _step_inputs():
    """fresh device tensors of the one step: the disparities and the poses are leaves"""
    d = synth.make_inputs(seed=21, **STEP)
    others = [synth.make_inputs(seed=22 + i, **STEP)["disps"] for i in range(STEP["n_src"])]
    t = lambda a: _t(np.ascontiguousarray(a, dtype=F32))
    x = dict(src=t(d["src"]), tgt=t(d["tgt"]), K=t(d["intrinsics"]), disps=[t(a).requires_grad_() for a in d["disps"]],
             poses=[t(a).requires_grad_() for a in d["poses"]],
             src_disps=[t(np.concatenate([o[s] for o in others], axis=1)).requires_grad_() for s in range(STEP["n_scales"])])
    assert all(float(a.detach().min()) > 0 for a in x["disps"] + x["src_disps"])
    return x


def _leaves(x):
    return x["disps"] + x["src_disps"] + x["poses"]


def _stages(x, tgt=None, src=None, K=None, disps=None, src_disps=None, poses=None, *, ssim_rate=0.85, geometry_weight=0.5, smooth_weight=0.0,
            auto_mask=False, with_mask=True, detach_weight=False, min_count=(0, 0), weights=None, conv={}):
    """one direction as its public stages, one after the other -> (total, photo, geometry, smooth total or None)"""
    tgt, src, K = (x["tgt"] if tgt is None else tgt), (x["src"] if src is None else src), (x["K"] if K is None else K)
    disps, src_disps, poses = disps or x["disps"], src_disps or x["src_disps"], poses or x["poses"]
    B, n, _, H, W = src.shape
    S = len(disps)
    warped, valid = ta.warp_pyramid(src, K, disps, poses, return_valid=True, **conv)
    errs = ta.photometric_error(warped, tgt, ssim_rate=ssim_rate)
    ident = cmp = None
    if auto_mask:
        plain = [p.view(B, n, 3, H >> s, W >> s) for s, p in enumerate(ops.pyramid(src.view(B, 3 * n, H, W), S))]
        with torch.no_grad():
            if auto_mask == "l1":
                cmp = ta.photometric_error(warped, tgt, ssim_rate=0.0)
                ident = ta.photometric_error(plain, tgt, ssim_rate=0.0)
            else:
                ident = ta.photometric_error(plain, tgt, ssim_rate=ssim_rate)
    diffs = ta.depth_consistency(disps, src_disps, K, poses, **conv)
    kw = dict(valid=valid, ident=ident, cmp=cmp, weights=weights, min_count=min_count)
    if with_mask:
        photo, geom = ta.pairwise_mean(errs, diffs, detach_weight=detach_weight, **kw)[:2]
    else:
        photo = ta.pairwise_mean(errs, [torch.zeros_like(d) for d in diffs], detach_weight=True, **kw)[0]
        geom = ta.pairwise_mean([e.detach() for e in errs], diffs, detach_weight=True, **kw)[1]
    total = photo + geometry_weight * geom
    smooth = None
    if smooth_weight:
        ws = [1.0] * S if weights is None else weights
        smooth = ta.disparity_smoothness(disps, tgt, weights=[smooth_weight * w for w in ws])[0]
    return total, photo, geom, smooth


def _grads(total, smooth, leaves, n_disps):
    """the gradients in the node's order: (warp + depth_consistency) -- two terms, commutative --, then + smoothness"""
    g = list(torch.autograd.grad(total, leaves, retain_graph=smooth is not None))
    if smooth is not None:
        for k, gs in enumerate(torch.autograd.grad(smooth, leaves[:n_disps])):
            g[k] = g[k] + gs
    return g


def _scatter_close(a, b, what):
    top = float(b.abs().max())
    err = float((a - b).abs().max())
    print("%s: max|difference| %.3g of max %.3g (bound %.3g)" % (what, err, top, SCATTER_TOL * top))
    assert top > 0 and err <= SCATTER_TOL * top, what


SC_CASES = {
    "default": dict(),
    "auto_l1": dict(auto_mask="l1"),
    "auto_error": dict(auto_mask="error", ssim_rate=0.5),
    "no_mask": dict(with_mask=False, auto_mask="l1"),
    "detach": dict(detach_weight=True, geometry_weight=0.3),
    "smooth": dict(smooth_weight=0.1, weights=[1.0, 0.7]),
    "smooth_no_mask": dict(smooth_weight=0.05, with_mask=False),
    "depth_range": dict(conv=dict(depth_range=(0.1, 100.0), pose_format="axis_angle", invert=[True, True]), smooth_weight=0.1),
    "min_count": dict(min_count=(100, 420)),      # (scale 1 has 2 * 240 pixels per source: its geometry mean falls under the threshold)
}


@pytest.mark.parametrize("case", sorted(SC_CASES))
def test_one_direction_is_its_stages(case):
    """bit for bit: the three scalars and every gradient (d_src_disp, an atomic scatter, within its tolerance)"""
    kw = dict(SC_CASES[case])
    conv = kw.pop("conv", {})
    x = _step_inputs()
    S = len(x["disps"])
    leaves = _leaves(x)
    out = ta.sc_sfm_loss(x["tgt"], x["src"], x["K"], x["disps"], x["src_disps"], x["poses"], bidirectional=False, **kw, **conv)
    assert all(t.dim() == 0 and t.dtype == torch.float32 and t.grad_fn is not None for t in out)
    got = torch.autograd.grad(out[0], leaves)
    total, photo, geom, smooth = _stages(x, conv=conv, **kw)
    want = _grads(total, smooth, leaves, S)
    if smooth is not None:
        total = total + smooth
    assert _bits(out[0].detach(), total.detach()) and _bits(out[1].detach(), photo.detach()) and _bits(out[2].detach(), geom.detach()), case
    for k, (a, b) in enumerate(zip(got, want)):
        if S <= k < 2 * S:
            _scatter_close(a, b, "%s d_src_disp[%d]" % (case, k - S))
        else:
            assert _bits(a, b), (case, k)
    assert float(out[1]) > 0 and float(out[2]) > 0 and all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in got)
    # the other two scalars carry their own gradients: the geometry alone reaches the disparities through depth_consistency only
    g_geom = torch.autograd.grad(ta.sc_sfm_loss(x["tgt"], x["src"], x["K"], x["disps"], x["src_disps"], x["poses"], bidirectional=False,
                                                **kw, **conv)[2], x["disps"])
    w_geom = torch.autograd.grad(_stages(x, conv=conv, **kw)[2], x["disps"])
    assert all(torch.equal(a, b) for a, b in zip(g_geom, w_geom))      # (equal as numbers: the node adds the warp's zeros to them)


def _reshaped(x):
    """the second direction's inputs in plain aten: every source is the target of a batch of B * n_src, the original target its one
    reference frame"""
    B, n, _, H, W = x["src"].shape
    M = B * n
    return dict(tgt=x["src"].reshape(M, 3, H, W), src=x["tgt"][:, None].expand(B, n, 3, H, W).reshape(M, 1, 3, H, W),
                K=x["K"].repeat_interleave(n, dim=0), disps=[t.reshape(M, 1, *t.shape[2:]) for t in x["src_disps"]],
                src_disps=[t.expand(B, n, *t.shape[2:]).reshape(M, 1, *t.shape[2:]) for t in x["disps"]],
                poses=[torch.stack(x["poses"], 1).reshape(M, 6)])


@pytest.mark.parametrize("case", ["default", "auto_l1", "smooth"])
def test_bidirectional_is_the_two_one_direction_calls(case):
    kw = dict(SC_CASES[case])
    x = _step_inputs()
    S = len(x["disps"])
    leaves = _leaves(x)
    out = ta.sc_sfm_loss(x["tgt"], x["src"], x["K"], x["disps"], x["src_disps"], x["poses"], **kw)
    got = torch.autograd.grad(out[0], leaves)
    one = ta.sc_sfm_loss(x["tgt"], x["src"], x["K"], x["disps"], x["src_disps"], x["poses"], bidirectional=False, **kw)
    r = _reshaped(x)
    kw.pop("smooth_weight", None)      # the smoothness term is the target frame's, in the first direction
    two = ta.sc_sfm_loss(r["tgt"], r["src"], r["K"], r["disps"], r["src_disps"], r["poses"], bidirectional=False, invert=[True], **kw)
    for a, b, c in zip(out, one, two):
        assert _bits(a.detach(), (b + c).detach())
    want = torch.autograd.grad(one[0] + two[0], leaves)
    for k, (a, b) in enumerate(zip(got, want)):
        if k < 2 * S:      # every disparity gradient holds one direction's scatter
            _scatter_close(a, b, "%s bidirectional d_disp[%d]" % (case, k))
        else:
            assert _bits(a, b), (case, k)
    assert float(two[1]) > 0 and float(two[2]) > 0


def _example_tail(maps, dtype, device):
    """the tail of INTEGRATION.md's pairwise_loss for ONE reference frame per call: (photo, geometry)"""
    photo = geometry = 0.0
    for e, d, v in maps:
        e, d, v = (t.detach().to(device=device, dtype=dtype) for t in (e, d, v))
        photo = photo + (e * (1 - d) * v).sum() / v.sum().clamp(min=1)
        geometry = geometry + (d * v).sum() / v.sum().clamp(min=1)
    return photo, geometry


def test_against_the_example_of_the_integration_guide():
    """INTEGRATION.md's pairwise_loss, its tail evaluated in float64 on the CPU from the GPU's own maps: the first direction per
    reference frame, as compute_photo_and_geometry_loss loops; the second on the reshaped inputs.  Bound: four times the distance
    of the float32 aten tail from that float64 value, at least 1 ulp."""
    x = _step_inputs()
    out = ta.sc_sfm_loss(x["tgt"], x["src"], x["K"], x["disps"], x["src_disps"], x["poses"])
    sums = {torch.float64: [0.0, 0.0], torch.float32: [0.0, 0.0]}
    with torch.no_grad():
        r = _reshaped(x)
        calls = [(x["tgt"], x["src"][:, i:i + 1], x["K"], x["disps"], [t[:, i:i + 1] for t in x["src_disps"]], [x["poses"][i]], None)
                 for i in range(STEP["n_src"])]
        calls.append((r["tgt"], r["src"], r["K"], r["disps"], r["src_disps"], r["poses"], [True]))
        for tgt, ref, K, disps, ref_disps, poses, invert in calls:
            warped, valid = ta.warp_pyramid(ref, K, disps, poses, return_valid=True, invert=invert)
            errs = ta.photometric_error(warped, tgt, ssim_rate=0.85)
            diffs = ta.depth_consistency(disps, ref_disps, K, poses, invert=invert)
            for dtype, device in ((torch.float64, "cpu"), (torch.float32, DEV)):
                p, g = _example_tail(list(zip(errs, diffs, valid)), dtype, device)
                sums[dtype][0] = sums[dtype][0] + p
                sums[dtype][1] = sums[dtype][1] + g
    for name, got, pick in (("photo", out[1], lambda p, g: p), ("geometry", out[2], lambda p, g: g), ("total", out[0], lambda p, g: p + 0.5 * g)):
        t64, t32, mine = float(pick(*sums[torch.float64])), float(pick(*sums[torch.float32])), float(got.detach())
        ulp = float(np.spacing(F32(abs(t64))))
        bound = max(4 * abs(t32 - t64), ulp)
        line = "sc_sfm_loss %s: %.9g, float64 tail %.17g (%.3g ulp), float32 aten tail %.9g (%.3g ulp)" % (
            name, mine, t64, abs(mine - t64) / ulp, t32, abs(t32 - t64) / ulp)
        print(line)
        parity_note(line)
        assert abs(mine - t64) <= bound, line


def test_sc_sfm_loss_dtypes_constants_and_capture():
    x = _step_inputs()
    args = (x["tgt"], x["src"], x["K"])
    disps = [t.detach().to(torch.bfloat16).requires_grad_() for t in x["disps"]]
    src_disps = [t.detach() for t in x["src_disps"]]      # constants: the kernel without the scatter
    packed = torch.cat([p.detach() for p in x["poses"]], dim=1).requires_grad_()
    tgt = x["tgt"].clone().requires_grad_()
    total = ta.sc_sfm_loss(tgt, x["src"], x["K"], disps, src_disps, packed, auto_mask="l1")[0]
    assert total.dtype == torch.float32
    total.backward()
    assert all(t.grad is not None and t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape for t in disps)
    assert packed.grad is not None and packed.grad.shape == packed.shape and tgt.grad is None
    with pytest.raises(TypeError, match="intrinsics"):
        ta.sc_sfm_loss(x["tgt"], x["src"], x["K"].clone().requires_grad_(), x["disps"], x["src_disps"], x["poses"])
    with pytest.raises(ValueError, match="weight"):
        ta.sc_sfm_loss(*args, x["disps"], x["src_disps"], x["poses"], weights=[1.0, -1.0])
    with pytest.raises(TypeError, match="src_disps"):
        ta.sc_sfm_loss(*args, x["disps"], x["disps"], x["poses"])
    with torch.no_grad():
        assert not ta.sc_sfm_loss(*args, x["disps"], x["src_disps"], x["poses"])[0].requires_grad

    leaves = x["disps"] + x["poses"]      # (no d_src_disp in this step: its scatter is not bitwise reproducible)
    held = [t.detach() for t in x["src_disps"]]

    def step():
        for t in leaves:
            t.grad = None
        out = ta.sc_sfm_loss(*args, x["disps"], held, x["poses"], auto_mask="l1", smooth_weight=0.1, bidirectional=False)
        out[0].backward()
        return [t.detach() for t in out] + [t.grad for t in leaves]

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
