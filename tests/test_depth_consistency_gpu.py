"""sfm_depth_consistency_fwd / _bwd and torch_api.depth_consistency on the GPU (include/sfmwarp_depth_consistency.h).

  1. identities, bit for bit: valid is the pyramid warp's, projected is sfm_warp_fwd on the one-channel image 1 / src_disp, diff is
     the quotient of the returned depths; the conventions reach the new kernels as they reach the pyramid warp's;
  2. the knife-free cases of tests/depth_consistency_ref.py against float64, nothing excluded, the float32 NumPy reference as the
     yardstick (knife_free.rule);
  3. the large case (65 blocks per image) with the upstream gradient zeroed on the pairs `knife` marks;
  4. reproducibility and buffers; 5. the autograd node."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import cameras
import depth_consistency_ref as R
from knife_free import floor_ratio, rule
from util import GUARD_MIN_BYTES, SENTINEL, Arena, parity_note

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
SMALL = [(shape, seeds[0], None) for shape, seeds in R.CASES.items()]
GENERAL = ((1, 24, 40, 3, 3), R.CASES[(1, 24, 40, 3, 3)][0], "general")
BIG = (R.LARGE, R.LARGE_SEED, None)
IDENTITY_CASES = SMALL + [BIG, GENERAL]
KNIFE_FREE = [(shape, seed, None) for shape, seed in R.CASE_LIST]

# The factor of `rule` for d_src_disp, derived as knife_free.K_FAST is: the largest floor_ratio over all knife-free cases and 5
# repeated calls on an MI355X (profiles/depth_consistency_accuracy.txt, written by tools/depth_consistency_accuracy.py: 0.986), times
# 4 (the scatter's order of additions varies from call to call, and another compiler schedules differently), rounded up to a power
# of two: 3.94 -> 4.  The yardstick is the float32 NumPy reference, never the kernel.
K_D_SRC_DISP = 4


def ident(case):
    (B, H, W, n_src, S), seed, kind = case
    return "B%d-%dx%d-%dsrc-%dsc-seed%d%s" % (B, H, W, n_src, S, seed, "-" + kind if kind else "")


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
def host_case(shape, seed, kind):
    """the inputs of one case on the host (never modify them).  The large case: g_diff is 0 on the pairs `knife` marks -- a choice
    of input: those pairs then contribute exact zeros."""
    d = R.inputs(shape, seed)
    if kind is not None:
        d = cameras.with_cameras(d, kind, 1000 + seed)
    marks = None
    if shape == R.LARGE:
        marks = R.knife(d)
        d = dict(d, g_diff=[np.where(m, F32(0), g) for m, g in zip(marks, d["g_diff"])])
    return d, marks


@functools.lru_cache(maxsize=None)
def references(shape, seed, kind):
    """(o64, o32) on the inputs of host_case, computed once and shared: never modified"""
    d, _ = host_case(shape, seed, kind)
    return R.reference(d, F64), R.reference(d, F32)


@functools.lru_cache(maxsize=None)
def case(shape, seed, kind=None):
    """everything the tests of one case share, computed once (never modify it): the inputs on the device and the new calls' outputs"""
    d, marks = host_case(shape, seed, kind)
    x = dict(B=d["B"], n_src=d["n_src"], S=d["n_scales"], marks=marks, K=_t(d["intrinsics"]), disps=[_t(a) for a in d["disps"]],
             src_disps=[_t(a) for a in d["src_disps"]], poses=[_t(a) for a in d["poses"]], g=[_t(a) for a in d["g_diff"]])
    x["hw"] = [tuple(t.shape[2:]) for t in x["disps"]]
    x["args"] = (x["disps"], x["src_disps"], x["poses"], x["K"])
    x["diff"], x["valid"], x["computed"], x["projected"] = ops.depth_consistency_fwd(*x["args"], want_valid=True, want_depths=True)
    x["d_disps"], x["d_poses"], x["d_src_disps"] = ops.depth_consistency_bwd(*x["args"], x["g"])
    torch.cuda.synchronize()
    return x


# ------------------------------------------------------------------------------------------------------------------------
# 1. identities, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
def _images(x):
    gen = torch.Generator().manual_seed(7)
    return [torch.rand((x["B"], 3 * x["n_src"], h, w), generator=gen).to(DEV) for h, w in x["hw"]]


def _quotient(c, p):
    """|c - p| / (c + p) in float32, formed on the host (IEEE operations)"""
    c, p = c.cpu().numpy(), p.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        return _t(np.abs(c - p) / (c + p))


@pytest.mark.parametrize("c", IDENTITY_CASES, ids=ident)
def test_the_forward_is_the_existing_warps_bit_for_bit(c):
    x = case(*c)
    B, n = x["B"], x["n_src"]
    _, valid = ops.warp_pyramid_fwd(_images(x), x["disps"], x["poses"], x["K"], "planar", want_valid=True)
    seen = 0
    for s, (h, w) in enumerate(x["hw"]):
        for t in (x["diff"][s], x["valid"][s], x["computed"][s], x["projected"][s]):
            assert tuple(t.shape) == (B, n, h, w) and bool(torch.isfinite(t).all())
        assert _bits(x["valid"][s], valid[s]), s
        depth = _t(F32(1) / x["disps"][s].cpu().numpy()).view(B, h * w)                  # (IEEE quotients, formed on the host)
        src_depth = _t(F32(1) / x["src_disps"][s].cpu().numpy())
        for i in range(n):
            want = ops.warp_fwd(src_depth[:, i:i + 1].contiguous(), depth, x["poses"][i], x["K"][:, s].contiguous())
            assert _bits(x["projected"][s][:, i], want[:, 0]), (s, i)
        ok = x["valid"][s] == 1
        cc, pp = x["computed"][s], x["projected"][s]
        assert bool((x["diff"][s][~ok] == 0).all()) and bool((x["computed"][s] >= 1e-3).all())
        assert _bits(x["diff"][s][ok], _quotient(cc, pp)[ok]), s
        assert float(x["diff"][s].max()) < 1 and float(x["diff"][s].min()) >= 0
        seen += int(ok.sum())
        assert int(ok.sum()) > 0, s
    assert 0 < seen < sum(v.numel() for v in x["valid"]), "pixels in view and pixels out of view"
    # without the optional outputs: the same bits
    assert all(_bits(a, b) for a, b in zip(ops.depth_consistency_fwd(*x["args"]), x["diff"]))
    diff, valid2 = ops.depth_consistency_fwd(*x["args"], want_valid=True)
    assert all(_bits(a, b) for a, b in zip(diff + valid2, x["diff"] + x["valid"]))
    diff, cc2, pp2 = ops.depth_consistency_fwd(*x["args"], want_depths=True)
    assert all(_bits(a, b) for a, b in zip(diff + cc2 + pp2, x["diff"] + x["computed"] + x["projected"]))


@pytest.mark.parametrize("c", IDENTITY_CASES, ids=ident)
def test_the_conventions_reach_the_kernels_as_they_reach_the_pyramid_warp(c):
    x = case(*c)
    n = x["n_src"]
    lo, hi = 0.1, 100.0
    kw = dict(pose_format="axis_angle", invert=[i % 2 == 0 for i in range(n)], depth_affine=(1.0 / lo - 1.0 / hi, 1.0 / hi))
    disps = [t / 10.02 for t in x["disps"]]              # Monodepth2's disparities lie in (0, 1)
    srcs = [t / 10.02 for t in x["src_disps"]]
    diff, valid, computed, projected = ops.depth_consistency_fwd(disps, srcs, x["poses"], x["K"], want_valid=True, want_depths=True, **kw)
    _, want = ops.warp_pyramid_fwd(_images(x), disps, x["poses"], x["K"], "planar", want_valid=True, **kw)
    for s in range(x["S"]):
        assert _bits(valid[s], want[s]), s
        ok = valid[s] == 1
        assert _bits(diff[s][ok], _quotient(computed[s], projected[s])[ok]) and bool((diff[s][~ok] == 0).all())
        assert float(projected[s].max()) <= hi * (1 + 1e-5), "the affine map acts on the sources' disparities too"
    # pose_format="matrix" on pose_mat_fwd's matrices is the Euler call, every output
    mats = [ops.pose_mat_fwd(p, "euler", False) for p in x["poses"]]
    got = ops.depth_consistency_fwd(x["disps"], x["src_disps"], mats, x["K"], want_valid=True, want_depths=True, pose_format="matrix")
    for name, group in zip(("diff", "valid", "computed", "projected"), got):
        assert all(_bits(a, b) for a, b in zip(group, x[name])), name
    # ... and backward: the gradient of the matrix taken through pose_mat_bwd is the Euler call's d_pose
    d_disps, d_mats, _ = ops.depth_consistency_bwd(x["disps"], x["src_disps"], mats, x["K"], x["g"], want_d_src_disp=False, pose_format="matrix")
    assert all(_bits(a, b) for a, b in zip(d_disps, x["d_disps"]))
    for i in range(n):
        assert tuple(d_mats[i].shape) == (x["B"], 3, 4)
        assert _bits(ops.pose_mat_bwd(x["poses"][i], "euler", False, d_mats[i]), x["d_poses"][i]), i


@pytest.mark.parametrize("c", SMALL[:2], ids=ident)
def test_the_conventions_backward_is_the_default_backward_behind_them(c):
    """the affine depth map: the default call on (disp * a) + b formed by two float32 operations, d_disp and d_src_disp that call's
    times a; axis-angle and inverted poses: the "matrix" call on pose_mat_fwd's output, d_pose pose_mat_bwd of that call's d_T"""
    x = case(*c)
    n = x["n_src"]
    a, b = 1.0 / 0.1 - 1.0 / 100.0, 1.0 / 100.0
    disps, srcs = [t / 10.02 for t in x["disps"]], [t / 10.02 for t in x["src_disps"]]
    sd, sd_src = [(t * a) + b for t in disps], [(t * a) + b for t in srcs]
    got = ops.depth_consistency_fwd(disps, srcs, x["poses"], x["K"], want_valid=True, want_depths=True, depth_affine=(a, b))
    want = ops.depth_consistency_fwd(sd, sd_src, x["poses"], x["K"], want_valid=True, want_depths=True)
    assert all(_bits(p, q) for g, w in zip(got, want) for p, q in zip(g, w))
    d_disps, d_poses, d_srcs = ops.depth_consistency_bwd(disps, srcs, x["poses"], x["K"], x["g"], depth_affine=(a, b))
    w_disps, w_poses, w_srcs = ops.depth_consistency_bwd(sd, sd_src, x["poses"], x["K"], x["g"])
    scale = torch.tensor(a, dtype=torch.float32, device=DEV)
    assert all(_bits(p, q * scale) for p, q in zip(d_disps, w_disps)) and all(_bits(p, q) for p, q in zip(d_poses, w_poses))
    for p, q in zip(d_srcs, w_srcs):      # (scattered: equal up to the order of the additions)
        assert float((p - q * scale).abs().max()) <= 1e-5 * float(p.abs().max()) and float(p.abs().max()) > 0
    for fmt in ("axis_angle", "euler"):
        inv = [i % 2 == 0 for i in range(n)]
        mats = [ops.pose_mat_fwd(p, fmt, inv[i]) for i, p in enumerate(x["poses"])]
        d_disps, d_poses, _ = ops.depth_consistency_bwd(*x["args"][:2], x["poses"], x["K"], x["g"], want_d_src_disp=False, pose_format=fmt, invert=inv)
        m_disps, d_mats, _ = ops.depth_consistency_bwd(*x["args"][:2], mats, x["K"], x["g"], want_d_src_disp=False, pose_format="matrix")
        assert all(_bits(p, q) for p, q in zip(d_disps, m_disps)), fmt
        for i in range(n):
            assert _bits(d_poses[i], ops.pose_mat_bwd(x["poses"][i], fmt, inv[i], d_mats[i])), (fmt, i)
            assert float(d_poses[i].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------
# 2. and 3. against float64
# ------------------------------------------------------------------------------------------------------------------------
def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _rules(c, what, keys):
    x = case(*c)
    o64, o32 = references(*c)
    for key, name, k in keys:
        for j, (got, a64, a32) in enumerate(zip(_np(x[key]), o64[name], o32[name])):
            if name == "d_src_disps":
                print("floor_ratio %s %s[%d]: %.3g" % (ident(c), name, j, floor_ratio(got, a64, a32)))
            ratio = rule(got, a64, a32, "%s %s %s[%d]" % (what, ident(c), name, j), k=k)
            parity_note("depth_consistency %s %s[%d]: max|gpu - o64| / max|numpy32 - o64| = %.3g (k = %g)" % (ident(c), name, j, ratio, k))


GRAD_KEYS = [("d_disps", "d_disps", 4), ("d_poses", "d_poses", 4), ("d_src_disps", "d_src_disps", K_D_SRC_DISP)]


@pytest.mark.parametrize("c", KNIFE_FREE, ids=ident)
def test_knife_free_cases_against_float64(c):
    """every element of diff, computed, d_disp, d_pose and d_src_disp, nothing excluded; upstream g_diff is randn"""
    x = case(*c)
    o64, o32 = references(*c)
    assert not any(m.any() for m in R.knife_of(o64) + R.knife_of(o32)), "the case is knife-free (tests/test_depth_consistency_cpu.py)"
    for s in range(x["S"]):
        assert np.array_equal(x["valid"][s].cpu().numpy(), o64["valid"][s]), s
    _rules(c, "knife-free", [("diff", "diff", 4), ("computed", "computed", 4), ("projected", "projected", 4)] + GRAD_KEYS)


def test_the_large_case_against_float64():
    """65 blocks per image: the fold's lane 0 goes round a second time.  g_diff is 0 on the pairs `knife` marks; the gradients hold
    the rules over the whole arrays, diff on the pairs knife does not mark"""
    x = case(*BIG)
    o64, o32 = references(*BIG)
    marks = x["marks"][0]
    share = marks.mean()
    print("large case: knife marks %.3f %% of the pairs" % (100 * share))
    assert 0 < share <= R.LARGE_KNIFE_CAP
    _rules(BIG, "large", GRAD_KEYS)
    got = x["diff"][0].cpu().numpy()
    rule(got[~marks], o64["diff"][0][~marks], o32["diff"][0][~marks], "large diff off the knife", k=4)
    assert np.array_equal(x["valid"][0].cpu().numpy()[~marks], o64["valid"][0][~marks])


# ------------------------------------------------------------------------------------------------------------------------
# 4. reproducibility and buffers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [SMALL[1], BIG], ids=ident)
def test_two_calls_with_differently_filled_workspaces_agree_bit_for_bit(c):
    x = case(*c)
    nbytes = sum(x["B"] * ((h * w + 255) // 256) for h, w in x["hw"]) * x["n_src"] * 12 * 4
    nbytes = -(-nbytes // 256) * 256
    for word in (SENTINEL, 0x3F800000, 0xFFFFFFFF):      # NaN, 1.0f and another NaN where the partials will be read from
        ws = torch.full((nbytes // 4,), word - (1 << 32) if word >= (1 << 31) else word, dtype=torch.int32, device=DEV)
        for want in (True, False):                       # with d_src_disp unbound: the other kernel, the same bits
            d_disps, d_poses, d_src = ops.depth_consistency_bwd(*x["args"], x["g"], want_d_src_disp=want, ws=ws)
            assert (d_src is not None) == want
            for a, b in zip(d_disps + d_poses, x["d_disps"] + x["d_poses"]):
                assert _bits(a, b), (hex(word), want)
    with pytest.raises(ValueError, match="bytes"):
        ops.depth_consistency_bwd(*x["args"], x["g"], ws=ws[:nbytes // 4 - 64])


@pytest.mark.parametrize("c,res", [(KNIFE_FREE[0], 12), (KNIFE_FREE[2], 4), (BIG, 0), (GENERAL, 8)], ids=["13x21-12", "24x40-4", "130x127-0", "general-8"])
def test_buffer_contract(dev, c, res):
    """every bound output pre-filled with the sentinel is overwritten completely -- d_src_disp too: it is cleared by the call, not
    accumulated into --, inputs are only read, and the guard bands around every output and a workspace of exactly the stated size stay
    as they were; placed at `res` bytes off a 16-byte boundary.  Each optional output is left NULL on its own, and scale by scale:
    its array keeps every sentinel and the others keep their bits.  The workspace starts out as NaN sentinels."""
    x = case(*c)
    B, n, S, hw = x["B"], x["n_src"], x["S"], x["hw"]
    d = _lib.SfmDepthConsDesc()
    d.B, d.n_src, d.n_scales = B, n, S
    specs = [("K", (B, S, 3, 3), res)] + [("pose%d" % i, (B, 6), res) for i in range(n)] + [("d_pose%d" % i, (B, 6), res) for i in range(n)]
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
        specs += [("disp%d" % s, (B, 1, h, w), res), ("d_disp%d" % s, (B, 1, h, w), res)]
        specs += [("%s%d" % (k, s), (B, n, h, w), res) for k in ("src_disp", "g", "diff", "valid", "computed", "projected", "d_src_disp")]
    nbytes = _lib.lib.sfm_depth_consistency_bwd_workspace_bytes(C.byref(d), None)      # (no pointer is bound yet)
    assert nbytes > 0 and nbytes % 256 == 0
    arena = Arena(dev, specs + [("ws", nbytes, "ws")], row_floats=hw[0][1])
    assert arena.guard >= GUARD_MIN_BYTES
    inputs = [("K", x["K"])] + [("pose%d" % i, x["poses"][i]) for i in range(n)]
    for s in range(S):
        inputs += [("disp%d" % s, x["disps"][s]), ("src_disp%d" % s, x["src_disps"][s]), ("g%d" % s, x["g"][s])]
    for key, a in inputs:
        arena.set(key, a)
        arena.snapshot(key)
    d.intrinsics = arena.ptr("K")
    for i in range(n):
        d.pose[i], d.d_pose[i] = arena.ptr("pose%d" % i), arena.ptr("d_pose%d" % i)
    for s in range(S):
        d.disp[s], d.src_disp[s], d.g_diff[s] = arena.ptr("disp%d" % s), arena.ptr("src_disp%d" % s), arena.ptr("g%d" % s)
        d.diff[s], d.d_disp[s] = arena.ptr("diff%d" % s), arena.ptr("d_disp%d" % s)
    optional = ("valid", "computed", "projected", "d_src_disp")
    always = ["d_pose%d" % i for i in range(n)] + ["%s%d" % (k, s) for s in range(S) for k in ("diff", "d_disp")]
    as_bits = lambda t: t.contiguous().view(torch.int32).cpu().numpy()
    o64, o32 = references(*c)
    # which optional outputs are bound: all of them; all but one, for each; the even scales only
    for unbound in [()] + [(k,) for k in optional] + ([tuple("%s%d" % (k, s) for k in optional for s in range(1, S, 2))] if S > 1 else []):
        bound = [(k, s) for k in optional for s in range(S) if k not in unbound and "%s%d" % (k, s) not in unbound]
        for o in always + ["%s%d" % (k, s) for k in optional for s in range(S)] + ["ws"]:
            arena.fill_bits(o)
        for k in optional:
            for s in range(S):
                getattr(d, k)[s] = arena.ptr("%s%d" % (k, s)) if (k, s) in bound else None
        ops._launch(dev, _lib.lib.sfm_depth_consistency_fwd, C.byref(d), None)
        ops._launch(dev, _lib.lib.sfm_depth_consistency_bwd, C.byref(d), None, C.c_void_p(arena.ptr("ws")), nbytes)
        torch.cuda.synchronize()
        for o in always:
            assert arena.sentinels_left(o) == 0, (unbound, o)
        for k in optional:
            for s in range(S):
                left, words = arena.sentinels_left("%s%d" % (k, s)), arena.nbytes("%s%d" % (k, s)) // 4
                assert left == (0 if (k, s) in bound else words), (unbound, k, s, "written completely if bound, not at all if NULL")
        arena.check("sfm_depth_consistency_fwd / _bwd, NULL: %s" % (unbound,))
        for key, _ in inputs:
            arena.unchanged(key)
        for s in range(S):
            np.testing.assert_array_equal(arena.bits("diff%d" % s), as_bits(x["diff"][s]))
            np.testing.assert_array_equal(arena.bits("d_disp%d" % s), as_bits(x["d_disps"][s]))
            for k, key in (("valid", "valid"), ("computed", "computed"), ("projected", "projected")):
                if (k, s) in bound:
                    np.testing.assert_array_equal(arena.bits("%s%d" % (k, s)), as_bits(x[key][s]))
            if ("d_src_disp", s) in bound and c[2] is None:      # overwritten, not accumulated: the sentinel leaves nothing beyond the rule
                rule(arena.view("d_src_disp%d" % s).cpu().numpy(), o64["d_src_disps"][s], o32["d_src_disps"][s],
                     "d_src_disp[%d] over a sentinel" % s, k=K_D_SRC_DISP)
        for i in range(n):
            np.testing.assert_array_equal(arena.bits("d_pose%d" % i), as_bits(x["d_poses"][i]))


# ------------------------------------------------------------------------------------------------------------------------
# 5. torch_api.depth_consistency
# ------------------------------------------------------------------------------------------------------------------------
def _torch_inputs(c=SMALL[1]):
    x = case(*c)
    return dict(K=x["K"], w=x["g"], disps=[t.clone().requires_grad_() for t in x["disps"]], srcs=[t.clone().requires_grad_() for t in x["src_disps"]],
                packed=torch.cat(x["poses"], dim=1).requires_grad_()), x


def _loss(t, disps=None, srcs=None, packed=None, **kw):
    out = ta.depth_consistency(t["disps"] if disps is None else disps, t["srcs"] if srcs is None else srcs, t["K"],
                               t["packed"] if packed is None else packed, **kw)
    diff = out[0] if isinstance(out, tuple) else out
    return sum((w * a).sum() for w, a in zip(t["w"], diff)), out


def test_autograd_gives_the_operators_bits():
    t, x = _torch_inputs()
    total, (diff, valid, computed, projected) = _loss(t, return_valid=True, return_depths=True)
    for name, group in zip(("diff", "valid", "computed", "projected"), (diff, valid, computed, projected)):
        assert len(group) == x["S"] and all(_bits(a, b) for a, b in zip(group, x[name])), name
        assert all(a.requires_grad == (name == "diff") for a in group), name
    assert all(a.grad_fn is diff[0].grad_fn for a in diff) and type(diff[0].grad_fn).__name__.startswith("_DepthConsistency"), "ONE node"
    total.backward()
    o64, o32 = references(*SMALL[1])
    for s in range(x["S"]):
        assert t["disps"][s].grad.shape == t["disps"][s].shape and _bits(t["disps"][s].grad, x["d_disps"][s])
        rule(t["srcs"][s].grad.cpu().numpy(), o64["d_src_disps"][s], o32["d_src_disps"][s], "autograd d_src_disp[%d]" % s, k=K_D_SRC_DISP)
    assert _bits(t["packed"].grad, torch.cat(x["d_poses"], dim=1))
    assert isinstance(_loss(t)[1], list) and len(_loss(t, return_valid=True)[1]) == 2 and len(_loss(t, return_depths=True)[1]) == 3
    # a scale the loss does not use: its upstream gradient is None -> zeros
    disps = [a.detach().clone().requires_grad_() for a in t["disps"]]
    out = ta.depth_consistency(disps, [a.detach() for a in t["srcs"]], t["K"], t["packed"].detach())
    (t["w"][1] * out[1]).sum().backward()
    assert bool((disps[0].grad == 0).all()) and bool((disps[2].grad == 0).all()) and float(disps[1].grad.abs().max()) > 0
    with torch.no_grad():
        assert not ta.depth_consistency(t["disps"], t["srcs"], t["K"], t["packed"])[0].requires_grad
        # the three convention arguments reach the operator: depth_range is Monodepth2's disp_to_depth as an affine map
        inv = [i % 2 == 0 for i in range(x["n_src"])]
        got = ta.depth_consistency(t["disps"], t["srcs"], t["K"], t["packed"], pose_format="axis_angle", invert=inv, depth_range=(0.1, 100.0))
        want = ops.depth_consistency_fwd(*x["args"], pose_format="axis_angle", invert=inv, depth_affine=(1.0 / 0.1 - 1.0 / 100.0, 1.0 / 100.0))
        assert all(_bits(a, b) for a, b in zip(got, want)) and not _bits(got[0], x["diff"][0])


def test_bf16_predictions_get_bf16_gradients():
    t, _ = _torch_inputs(SMALL[0])
    d16 = [a.detach().to(torch.bfloat16).requires_grad_() for a in t["disps"]]
    s16 = [a.detach().to(torch.bfloat16).requires_grad_() for a in t["srcs"]]
    p16 = t["packed"].detach().to(torch.bfloat16).requires_grad_()
    _loss(t, d16, s16, p16)[0].backward()
    d32 = [a.detach().float().requires_grad_() for a in d16]
    s32 = [a.detach().float().requires_grad_() for a in s16]
    p32 = p16.detach().float().requires_grad_()
    _loss(t, d32, s32, p32)[0].backward()
    for a, b in zip(d16 + [p16], d32 + [p32]):
        assert a.grad.dtype == torch.bfloat16 and a.grad.shape == a.shape and _bits(a.grad, b.grad.to(torch.bfloat16))
    for a, b in zip(s16, s32):      # (scattered: equal up to the order of the additions, far below a bfloat16's spacing almost everywhere)
        assert a.grad.dtype == torch.bfloat16 and a.grad.shape == a.shape
        assert float((a.grad.float() - b.grad).abs().max()) <= 2.0 ** -7 * float(b.grad.abs().max())


def test_intrinsics_that_require_grad_are_refused():
    t, _ = _torch_inputs(SMALL[0])
    with pytest.raises(TypeError, match="intrinsics"):
        ta.depth_consistency(t["disps"], t["srcs"], t["K"].clone().requires_grad_(), t["packed"])
    with pytest.raises(TypeError, match="intrinsics"):
        ta.depth_consistency(t["disps"], t["srcs"], t["K"][:, :, :2], t["packed"])


def test_src_disps_without_grad_launch_no_scatter(monkeypatch):
    t, x = _torch_inputs()
    calls = []
    real = ops.depth_consistency_bwd

    def spy(*args, **kw):
        out = real(*args, **kw)
        calls.append((kw.get("want_d_src_disp"), out[2]))
        return out

    monkeypatch.setattr(ops, "depth_consistency_bwd", spy)
    _loss(t, srcs=[a.detach() for a in t["srcs"]])[0].backward()
    assert calls == [(False, None)], "d_src_disp is not allocated and the kernel without the scatter runs"
    assert all(a.grad is None for a in t["srcs"])
    for s in range(x["S"]):
        assert _bits(t["disps"][s].grad, x["d_disps"][s])
    assert _bits(t["packed"].grad, torch.cat(x["d_poses"], dim=1))
    _loss(t)[0].backward()
    assert calls[1][0] is True and calls[1][1] is not None


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
    t, x = _torch_inputs()
    leaves = t["disps"] + [t["packed"]] + t["srcs"]
    exact = x["S"] + len(t["disps"]) + 1

    def step():
        for a in leaves:
            a.grad = None
        total, out = _loss(t)
        total.backward()
        # (detached: a result that keeps its grad_fn keeps the eager run's autograd graph alive, and with it the leaves' gradient
        #  accumulators, which belong to the stream of that run -- the capture would then fork onto that stream)
        return [a.detach() for a in out] + [a.grad for a in leaves]

    eager, captured = _captured(step)
    assert all(_bits(a, b) for a, b in zip(eager[:exact], captured[:exact])), "diff, d_disp and d_pose replay to the eager bits"
    assert all(float(a.abs().max()) > 0 for a in eager)
    o64, o32 = references(*SMALL[1])
    for s, a in enumerate(captured[exact:]):      # the memset is part of the graph: a replay does not accumulate
        rule(a.cpu().numpy(), o64["d_src_disps"][s], o32["d_src_disps"][s], "replayed d_src_disp[%d]" % s, k=K_D_SRC_DISP)
