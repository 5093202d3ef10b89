"""The image warps on the GPU against float64, every element, nothing excluded: sfm_warp_fwd / sfm_warp_bwd (one and three depth
rows, three and five channels), sfm_warp_pyramid_* in both layouts, its _conv_ forms under every convention of
include/sfmwarp_pose.h, and d_T -- all 12 entries of the gradient of a "matrix" pose -- from the pyramid warp and from
sfm_depth_consistency_bwd.

The inputs are the knife-free cases of tests/warp_exact_ref.py (tests/test_warp_exact_cpu.py proves them knife-free and shows that
the rule rejects what the 2e-3 criteria let pass).  Before any rule `valid` and the set of exactly-zero pixels are the float64
reference's, pixel for pixel.  Then knife_free.rule per array: max|got - o64| <= k max|o32 - o64| + 1e-6 max|o64|, o64 / o32 the
reference in float64 / float32 on the same float32 inputs: the yardstick is the two references, never the kernel.

k = 4 on every whole array: the project's standing factor for a float32 kernel in the reference's own evaluation order
(knife_free.K_REF).  The translation column of d_T and d_pose can be orders of magnitude larger than the rotation block, so a
max-norm rule on the whole array can hide the rotation block: the rule is applied to the blocks as well, with the factors K_BLOCK,
and to d_src (float atomics) with K_D_SRC -- measured, see there."""
import functools
import importlib

import numpy as np
import pytest
import torch

import depth_consistency_ref as DR
import warp_exact_ref as R
from knife_free import K_REF, floor_ratio, rule
from util import parity_note

pytestmark = pytest.mark.gpu

ops = importlib.import_module("sfm-learner-chainer_amd.ops")

DEV = "cuda:0"
K = K_REF

# The factors of `rule` for the rotation and translation blocks of d_T (B,3,4) and d_pose (B,6) and for d_src, derived as
# knife_free.K_FAST and K_D_SRC_DISP are: the largest knife_free.floor_ratio -- max|gpu - o64| / (max|numpy32 - o64| + 2.5e-7 max|o64|),
# per block -- over every case, setting and call of this module on an MI355X (profiles/warp_accuracy.txt, written by
# tools/warp_accuracy.py), times 4 (another compiler schedules differently; d_src's order of additions varies from call to call: 5
# calls per case), rounded up to a power of two, and at least 4.
# measured: d_T_rot 1.970, d_T_trans 1.775, d_pose_rot 1.848, d_pose_trans 1.804 (each 4 x -> 7.1 .. 7.9 -> 8), d_src 0.985 (3.94 -> 4).
# The whole arrays, held to k = 4, measured 1.19 (warped), 1.06 (d_disp), 0.97 (d_depth), 1.80 (d_pose) and 1.78 (d_T) at the most.
K_BLOCK = {"d_T_rot": 8, "d_T_trans": 8, "d_pose_rot": 8, "d_pose_trans": 8}
K_D_SRC = 4
FACTORS = dict(K_BLOCK, d_src=K_D_SRC)


@pytest.fixture(autouse=True)
def _needs_a_gpu(dev):
    """(the `dev` fixture skips where no GPU is visible)"""


def _bits(a, b):
    """bitwise equality of two float tensors (NaN payloads and the sign of zero included)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def blocks(kind, name, got, a64, a32):
    """[(kind, name, got, o64, o32)] of a d_T (B,3,4) or a d_pose (B,6): the whole array, its rotation block, its translation block"""
    cut = (lambda a: a[:, :, :3], lambda a: a[:, :, 3]) if a64.ndim == 3 else (lambda a: a[:, :3], lambda a: a[:, 3:])
    return [(kind, name, got, a64, a32)] + [("%s_%s" % (kind, part), "%s %s" % (name, part), f(got), f(a64), f(a32))
                                           for part, f in zip(("rot", "trans"), cut)]


def check(rows, what):
    """knife_free.rule on every row (kind, name, got, o64, o32), k = 4 or the kind's measured factor; one parity note per array"""
    for kind, name, got, a64, a32 in rows:
        k = FACTORS.get(kind, K)
        ratio = rule(got, a64, a32, "%s %s" % (what, name), k=k)
        parity_note("warp_exact %s %s: max|gpu - o64| / max|numpy32 - o64| = %.3g, floor_ratio %.3g (k = %g)"
                    % (what, name, ratio, floor_ratio(got, a64, a32), k))


# ------------------------------------------------------------------------------------------------------------------------
# 1. sfm_warp_fwd / sfm_warp_bwd
# ------------------------------------------------------------------------------------------------------------------------
OPERATOR_CASES = [(c, rows, C, i) for c in R.CASE_LIST for rows, C in R.OPERATOR_FORMS for i in range(c[0][3])]
OPERATOR_CASES += [(R.OPERATOR_C5_CASE, rows, 5, 0) for rows in (1, 3)]


def op_ident(v):
    c, rows, C, i = v
    return "%s-rows%d-C%d-src%d" % (R.ident(c), rows, C, i)


def operator_rows(v):
    """one call of ops.warp_fwd and ops.warp_bwd(want_d_src=True) -> (its outputs, o64, o32, the rows for `check`)"""
    (shape, seed, _), rows, C, i = v
    d = R.inputs(shape, seed, "default")
    imgs, _, dev_depth, pose, Kc, g = R.operator_inputs(d, rows, C, i)
    args = [_t(a) for a in (imgs, dev_depth, pose, Kc)]
    warped = ops.warp_fwd(*args).cpu().numpy()
    d_depth, d_pose, d_src = ops.warp_bwd(*args, _t(g), want_d_src=True)
    B, _, H, W = imgs.shape
    got = dict(warped=warped, d_depth=d_depth.cpu().numpy().reshape(B, rows, H, W), d_pose=d_pose.cpu().numpy(), d_src=d_src.cpu().numpy())
    o64, o32 = R.operator_references(shape, seed, rows, C, i)
    out = [(key, key, got[key], o64[key], o32[key]) for key in ("warped", "d_depth", "d_src")]
    return got, o64, o32, out + blocks("d_pose", "d_pose", got["d_pose"], o64["d_pose"], o32["d_pose"])


@pytest.mark.parametrize("v", OPERATOR_CASES, ids=op_ident)
def test_the_operator_against_float64(v):
    """warped, d_depth and d_pose at k = 4, d_src (scattered with float atomics) at K_D_SRC; every source of every default case at
    scale 0, one and three depth rows, and five channels on one case"""
    got, o64, o32, rows = operator_rows(v)
    assert not (R.operator_knife_of(o64) | R.operator_knife_of(o32)).any(), "the case is knife-free (tests/test_warp_exact_cpu.py)"
    assert np.array_equal((got["warped"] == 0).all(axis=1), o64["valid"] == 0), "the exactly-zero pixels are the float64 reference's"
    dead = np.broadcast_to((o64["valid"] == 0)[:, None], got["d_depth"].shape)
    assert (got["d_depth"][dead] == 0).all()
    check(rows, "operator %s" % op_ident(v))


# ------------------------------------------------------------------------------------------------------------------------
# 2. sfm_warp_pyramid_* and its _conv_ forms
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pyramid(case, layout="planar", rigid_matrix=False):
    """ops.warp_pyramid_fwd / _bwd on one case under its setting's conventions, computed once (never modify it) -> dict of NumPy
    lists warped, valid, d_disps, d_poses.  rigid_matrix: the poses handed over as pose_mat_fwd's 3x4, pose_format="matrix"."""
    d = R.inputs(*case)
    src = [_t(a) for a in d["src_pyr"]]
    if layout == "hwc":
        src = [ops.to_hwc(a) for a in src]
    poses = [_t(p) for p in d["poses"]]
    kw = dict(pose_format=d["fmt"], invert=d["invert"] if any(d["invert"]) else None,
              depth_affine=tuple(float(v) for v in d["affine"]) if d["affine"] is not None else None)
    if rigid_matrix:
        poses = [ops.pose_mat_fwd(p, d["fmt"], d["invert"][i]) for i, p in enumerate(poses)]
        kw.update(pose_format="matrix", invert=None)
    args = (src, [_t(a) for a in d["disps"]], poses, _t(d["intrinsics"]), layout)
    warped, valid = ops.warp_pyramid_fwd(*args, want_valid=True, **kw)
    d_disps, d_poses = ops.warp_pyramid_bwd(*args, [_t(a) for a in d["g"]], **kw)
    torch.cuda.synchronize()
    return dict(warped=_np(warped), valid=_np(valid), d_disps=_np(d_disps), d_poses=_np(d_poses))


def pyramid_rows(case, got, pose_key="d_poses"):
    """the facts that come before any rule, then the rows for `check`; pose_key: the reference array d_poses is compared with"""
    o64, o32 = R.references(*case)
    assert not any(m.any() for m in R.knife_of(o64) + R.knife_of(o32)), "the case is knife-free (tests/test_warp_exact_cpu.py)"
    rows = []
    for s in range(case[0][4]):
        assert np.array_equal(got["valid"][s], o64["valid"][s]), s
        assert np.array_equal((got["warped"][s] == 0).all(axis=2), o64["valid"][s] == 0), "the exactly-zero pixels are the float64 reference's"
        assert (got["d_disps"][s][(o64["valid"][s] == 0).all(axis=1, keepdims=True)] == 0).all(), s
        rows += [("warped", "warped[%d]" % s, got["warped"][s], o64["warped"][s], o32["warped"][s]),
                 ("d_disp", "d_disp[%d]" % s, got["d_disps"][s], o64["d_disps"][s], o32["d_disps"][s])]
    kind = "d_T" if pose_key == "d_T" else "d_pose"
    for i, a in enumerate(got["d_poses"]):
        assert a.shape == o64[pose_key][i].shape, (i, a.shape)
        rows += blocks(kind, "%s[%d]" % (kind, i), a, o64[pose_key][i], o32[pose_key][i])
    return rows


@pytest.mark.parametrize("case", R.CASE_LIST, ids=R.ident)
def test_the_pyramid_warp_against_float64(case):
    check(pyramid_rows(case, pyramid(case)), "pyramid %s" % R.ident(case))


@pytest.mark.parametrize("case", R.CASE_LIST + R.CONV_CASE_LIST[:2] + R.MATRIX_CASE_LIST[:1], ids=R.ident)
def test_hwc_is_the_planar_result_bit_for_bit(case):
    a, b = pyramid(case), pyramid(case, "hwc")
    for key in ("warped", "valid", "d_disps", "d_poses"):
        assert all(_bits(torch.from_numpy(p), torch.from_numpy(q)) for p, q in zip(a[key], b[key])), key


@pytest.mark.parametrize("case", R.CONV_CASE_LIST + R.ALONE_CASE_LIST, ids=R.ident)
def test_the_conventions_against_float64(case):
    """axis-angle poses, inverted even sources and the affine depth map together (d_disp includes disp_scale), and each alone"""
    d = R.inputs(*case)
    assert d["fmt"] != "euler" or any(d["invert"]) or d["affine"] is not None
    check(pyramid_rows(case, pyramid(case)), "conventions %s" % R.ident(case))


@pytest.mark.parametrize("case", R.CONV_CASE_LIST, ids=R.ident)
def test_d_T_of_rigid_matrices_against_float64(case):
    """pose_format="matrix" on pose_mat_fwd's matrices of the axis-angle, partly inverted poses: d_T, all 12 entries, against the
    reference's gradient of T = [R|t]"""
    got = pyramid(case, rigid_matrix=True)
    assert all(a.shape == (case[0][0], 3, 4) for a in got["d_poses"])
    check(pyramid_rows(case, got, "d_T"), "rigid matrix %s" % R.ident(case))


@pytest.mark.parametrize("case", R.MATRIX_CASE_LIST, ids=R.ident)
def test_d_T_of_matrices_that_are_not_rigid_against_float64(case):
    """every entry of T off its rigid value by up to 2 %: what a learned or composed 3x4 is"""
    got = pyramid(case)
    assert all(a.shape == (case[0][0], 3, 4) for a in got["d_poses"])
    check(pyramid_rows(case, got, "d_T"), "matrix %s" % R.ident(case))


# ------------------------------------------------------------------------------------------------------------------------
# 3. d_T of sfm_depth_consistency_bwd
# ------------------------------------------------------------------------------------------------------------------------
def depth_consistency_rows(case):
    d = DR.inputs(*case)
    o64, o32 = DR.references(*case)
    poses = [_t(p) for p in d["poses"]]
    mats = [ops.pose_mat_fwd(p, "euler", False) for p in poses]
    _, d_T, _ = ops.depth_consistency_bwd([_t(a) for a in d["disps"]], [_t(a) for a in d["src_disps"]], mats, _t(d["intrinsics"]),
                                          [_t(a) for a in d["g_diff"]], want_d_src_disp=False, pose_format="matrix")
    rows = []
    for i, a in enumerate(_np(d_T)):
        assert a.shape == (d["B"], 3, 4)
        rows += blocks("d_T", "d_T[%d]" % i, a, o64["d_T"][i], o32["d_T"][i])
    return rows


@pytest.mark.parametrize("case", DR.CASE_LIST, ids=DR.case_id)
def test_d_T_of_the_depth_consistency_term_against_float64(case):
    check(depth_consistency_rows(case), "depth_consistency %s" % DR.case_id(case))


def every_row(calls=1):
    """(what, kind, name, got, o64, o32) of every comparison of this module, the scattered d_src `calls` times: what
    tools/warp_accuracy.py measures the factors on"""
    for v in OPERATOR_CASES:
        for call in range(calls):
            for row in operator_rows(v)[3]:
                if call == 0 or row[0] == "d_src":
                    yield ("operator %s call %d" % (op_ident(v), call),) + row
    for case in R.CASE_LIST + R.CONV_CASE_LIST + R.ALONE_CASE_LIST:
        for row in pyramid_rows(case, pyramid(case)):
            yield ("pyramid %s" % R.ident(case),) + row
    for case in R.CONV_CASE_LIST:
        for row in pyramid_rows(case, pyramid(case, rigid_matrix=True), "d_T"):
            yield ("rigid matrix %s" % R.ident(case),) + row
    for case in R.MATRIX_CASE_LIST:
        for row in pyramid_rows(case, pyramid(case), "d_T"):
            yield ("matrix %s" % R.ident(case),) + row
    for case in DR.CASE_LIST:
        for row in depth_consistency_rows(case):
            yield ("depth_consistency %s" % DR.case_id(case),) + row
