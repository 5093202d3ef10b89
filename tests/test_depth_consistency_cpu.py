"""include/sfmwarp_depth_consistency.h without a GPU: the two float64 statements of the term (tests/depth_consistency_ref.py) agree;
the knife-free cases are knife-free and the large case stays under its cap; the side header, the binding and the library declare the
same struct and the same three entry points; every documented rejection answers with its code, in the documented order and before
any HIP call (the pointers are fakes that are never dereferenced); and the Python argument errors that are raised before a device
is touched."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_header as AH
import depth_consistency_ref as R

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmwarp_depth_consistency.h")
CSRC = os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc")
FAKE = 0x10000                 # never dereferenced
WS = C.c_void_p(0x100000)      # on a 256-byte boundary, never dereferenced
ENTRY_POINTS = sorted(["sfm_depth_consistency_fwd", "sfm_depth_consistency_bwd_workspace_bytes", "sfm_depth_consistency_bwd"])
EULER, AXIS, MATRIX = 0, 1, 2
F32, F64 = np.float32, np.float64

with open(HEADER) as _f:
    RAW = _f.read()
TEXT = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)      # the header without its comments


# ------------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASE_LIST, ids=R.case_id)
def test_the_two_float64_statements_agree(case):
    """NumPy on the oracle's warp with a hand-derived backward against torch autograd through grid_sample, inv and matmul"""
    o64, _ = R.references(*case)
    t = R.torch_opinion(R.inputs(*case))
    for key in ("diff",) + R.GRADS + ("d_T",):      # d_T: all 12 entries of the gradient of T = [R|t], what pose_format="matrix" returns
        assert len(o64[key]) == len(t[key])
        for k, (a, b) in enumerate(zip(o64[key], t[key])):
            top = np.abs(a).max()
            err = np.abs(a - b).max()
            print("%s[%d]: max|numpy64 - torch64| = %.3g of max %.3g" % (key, k, err, top))
            assert top > 0 and err <= 1e-9 * top, (key, k)


@pytest.mark.parametrize("case", R.CASE_LIST, ids=R.case_id)
def test_the_knife_free_cases_are_knife_free(case):
    shape, seed = case
    assert sum(a.size for a in R.inputs(*case)["src_disps"]) <= 4000, "a knife-free case has about 3,000 pixel-source pairs at the most"
    assert R.failed_conditions(shape, seed) == []
    o64, o32 = R.references(*case)
    for o in (o64, o32):
        assert not any(m.any() for m in R.knife_of(o))
    for s, v in enumerate(o64["valid"]):
        assert np.array_equal(v, o32["valid"][s])
        for i in range(v.shape[1]):
            assert R.VALID_SHARE[0] <= v[:, i].mean() <= R.VALID_SHARE[1], (s, i)
    for name, y in R.yardsticks(o64, o32):
        print("%s: max|o32 - o64| / max|o64| = %.3g" % (name, y))
        assert 0 < y <= R.YARDSTICK_MAX, name
    # in view, away from the clamp, both signs of computed - projected: the term is not trivially smooth
    signs = np.concatenate([np.sign(c - p)[v == 1] for c, p, v in zip(o64["computed"], o64["projected"], o64["valid"])])
    assert (signs > 0).any() and (signs < 0).any()
    assert all(float(d.max()) < 1 and float(d.min()) >= 0 for d in o64["diff"])


def test_search_finds_the_seeds():
    shape = (2, 13, 21, 2, 1)
    assert tuple(R.search(shape, 0, 2)) == R.CASES[shape]
    assert R.failed_conditions((2, 13, 21, 2, 1), 2) != [], "seed 2 is not knife-free: the conditions do reject"


def test_the_large_case_stays_under_its_cap():
    B, H, W, n_src, S = R.LARGE
    assert (H * W + 255) // 256 == 65, "65 blocks per image: the fold's lane 0 goes round a second time"
    marks = R.knife(R.inputs(R.LARGE, R.LARGE_SEED))
    share = sum(int(m.sum()) for m in marks) / sum(m.size for m in marks)
    print("large case: knife marks %.3f %% of the (pixel, source) pairs" % (100 * share))
    assert 0 < share <= R.LARGE_KNIFE_CAP


# ------------------------------------------------------------------------------------------------------------------------
# 2. header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def _prototypes():
    code = re.sub(r"^\s*#.*$", "", TEXT, flags=re.M)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(sfm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}


def test_the_side_header_stands_beside_the_main_one():
    assert '#include "sfmwarp.h"' in RAW and '#include "sfmwarp_pose.h"' in RAW
    first = re.search(r"/\*.*?\*/", RAW, flags=re.S).group(0)
    assert "sfmwarp.h" in first and "FOLLOW-UP" in first, "the first comment says that this header is to be folded into sfmwarp.h"
    assert "inverse_warp2" in first and "compute_pairwise_loss" in first, "the SC-SfMLearner statements it restates, by function name"
    assert "SFM_ABI_VERSION" not in TEXT and _lib.SFM_ABI_VERSION == 6 and L.sfm_abi_version() == 6
    assert "#define" not in re.sub(r"#define SFMWARP_DEPTH_CONSISTENCY_H_", "", TEXT), "it uses the constants of sfmwarp.h, it adds no macro"
    assert TEXT.count("typedef") == 1, "one struct of its own: SfmDepthConsDesc"
    assert "bitwise reproducible" in RAW and "NOT" in RAW, "it says which outputs are reproducible and that d_src_disp is not"


def test_the_struct_is_the_headers(monkeypatch):
    monkeypatch.setattr(AH, "TEXT", TEXT)
    assert [f[0] for f in AH.struct_fields("SfmDepthConsDesc")] == [
        "B", "n_src", "n_scales", "H", "W", "disp", "src_disp", "intrinsics", "pose", "diff", "valid", "computed", "projected", "g_diff",
        "d_disp", "d_src_disp", "d_pose"]
    AH.assert_layout(_lib.SfmDepthConsDesc, "SfmDepthConsDesc")
    ptr, S, N = C.sizeof(C.c_void_p), _lib.SFM_MAX_SCALES, _lib.SFM_MAX_SRC
    assert _lib.SfmDepthConsDesc.disp.offset == -(-(12 + 8 * S) // ptr) * ptr
    assert C.sizeof(_lib.SfmDepthConsDesc) == _lib.SfmDepthConsDesc.disp.offset + ptr * (9 * S + 2 * N + 1)


def test_the_symbol_table_is_the_headers_and_disjoint_from_the_other_six():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.DEPTH_CONS_SYMBOLS) == ENTRY_POINTS
    for other in (_lib.SYMBOLS, _lib.EXT_SYMBOLS, _lib.SMOOTH_SYMBOLS, _lib.FULL_RES_SYMBOLS, _lib.CONV_SYMBOLS, _lib.POSE_SYMBOLS):
        assert not set(_lib.DEPTH_CONS_SYMBOLS) & set(other)
    kinds = {"const SfmDepthConsDesc *": C.POINTER(_lib.SfmDepthConsDesc), "const SfmPoseConv *": C.POINTER(_lib.SfmPoseConv),
             "void *": C.c_void_p, "size_t ": C.c_size_t}
    for name, params in protos.items():
        res, args = _lib.DEPTH_CONS_SYMBOLS[name]
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        assert len(args) == len(params), name
        assert res is (C.c_size_t if name.endswith("_bytes") else C.c_int)
        assert re.search(r"\b(size_t|int)\s+%s\(" % name, TEXT).group(1) == ("size_t" if name.endswith("_bytes") else "int")
        for param, arg in zip(params, args):
            kind = re.match(r"(const \w+ \*|\w+ \*|\w+ )", param).group(1)
            assert kinds[kind] == arg, (name, param)


def test_the_library_exports_the_three_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported


def test_the_unit_is_built_from_the_one_copy_of_the_pixel_code():
    unit = open(os.path.join(CSRC, "sfm_depth_consistency.hip")).read()
    for header in ("sfm_common.h", "sfm_pose.h", "sfm_warp_pixel.h"):
        assert '#include "%s"' % header in unit
    for fn in ("ref_project(", "pad_taps(", "pad_blend(", "warp_pixel_gq(", "warp_pixel_gdepth(", "warp_pixel_gpm(", "make_geom_conv(A.conv",
               "conv_sd(", "conv_d_disp(", "pose_fold_conv(A.conv", "check_pose_conv(", "check_pyramid_shape(", "hipMemsetAsync("):
        assert fn in unit, fn
        assert not re.search(r"__forceinline__ \w+ %s" % re.escape(fn.split("(")[0]) + r"\(", unit), "%s is used, not redefined" % fn
    assert "fp contract(off)" in unit
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "sfm_depth_consistency.hip" in make and make.count("sfmwarp_depth_consistency.h") == 2


def test_the_python_signatures():
    p = inspect.signature(ops.depth_consistency_fwd).parameters
    assert list(p)[:4] == ["disps", "src_disps", "poses", "K"]
    assert (p["want_valid"].default, p["want_depths"].default) == (False, False)
    assert (p["pose_format"].default, p["invert"].default, p["depth_affine"].default) == ("euler", None, None)
    p = inspect.signature(ops.depth_consistency_bwd).parameters
    assert list(p)[:5] == ["disps", "src_disps", "poses", "K", "g_diff"] and p["want_d_src_disp"].default is True
    p = inspect.signature(ta.depth_consistency).parameters
    assert list(p)[:4] == ["pred_disps", "src_disps", "intrinsics", "pred_poses"]
    assert (p["return_valid"].default, p["return_depths"].default) == (False, False)
    assert (p["pose_format"].default, p["invert"].default, p["depth_range"].default) == ("euler", None, None)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("return_valid", "return_depths", "pose_format", "invert", "depth_range"))
    assert "depth_consistency" in ta.__all__ and "depth_consistency_fwd" in ops.__all__ and "depth_consistency_bwd" in ops.__all__


# ------------------------------------------------------------------------------------------------------------------------
# 3. what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _conv(fmt=AXIS, invert=(1, 0), scale=9.99, shift=0.01):
    c = _lib.SfmPoseConv()
    c.pose_format, c.disp_scale, c.disp_shift = fmt, scale, shift
    for i, v in enumerate(invert):
        c.invert[i] = v
    return c


POINTERS = ("disp", "src_disp", "diff", "valid", "computed", "projected", "g_diff", "d_disp", "d_src_disp")


def _desc(B=2, n_src=2, n_scales=2, hw=((16, 24), (8, 12)), **kw):
    d = _lib.SfmDepthConsDesc()
    d.B, d.n_src, d.n_scales = B, n_src, n_scales
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
    for s in range(_lib.SFM_MAX_SCALES):
        for name in POINTERS:
            getattr(d, name)[s] = FAKE
    for i in range(_lib.SFM_MAX_SRC):
        d.pose[i] = d.d_pose[i] = FAKE
    d.intrinsics = FAKE
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def _ref(x):
    return C.byref(x) if x is not None else None


def fwd(d, c=None):
    return L.sfm_depth_consistency_fwd(_ref(d), _ref(c), None), _lib.last_error()


def bwd(d, c=None, ws=WS, nbytes=1 << 40):
    return L.sfm_depth_consistency_bwd(_ref(d), _ref(c), ws, nbytes, None), _lib.last_error()


def query(d, c=None):
    return L.sfm_depth_consistency_bwd_workspace_bytes(_ref(d), _ref(c))


CALLS = ((fwd, "sfm_depth_consistency_fwd"), (bwd, "sfm_depth_consistency_bwd"))
BAD_CONVS = [(dict(fmt=3), "pose_format=3"), (dict(fmt=-1), "pose_format=-1"), (dict(invert=(2, 0)), "invert[0]=2"),
             (dict(invert=(0, -1)), "invert[1]=-1"), (dict(fmt=MATRIX, invert=(0, 1)), "SFM_POSE_MATRIX"),
             (dict(scale=float("nan")), "disp_scale"), (dict(shift=float("inf")), "disp_shift"), (dict(scale=float("-inf")), "disp_scale")]


def test_the_descriptor_then_the_shape():
    bad_conv = _conv(fmt=7)
    for call, who in CALLS:
        rc, msg = call(None, bad_conv)
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
        for bad, word in ((dict(n_src=0), "n_src"), (dict(n_src=9), "n_src"), (dict(n_scales=0), "n_scales"), (dict(n_scales=9), "n_scales"),
                          (dict(B=-1), "B=-1"), (dict(H=(1, 2)), "H=2"), (dict(W=(0, 2)), "W=2"), (dict(H=(0, 40000), W=(0, 40000)), "too large"),
                          (dict(B=1 << 30, H=(0, 17), W=(0, 17)), "too many")):
            rc, msg = call(_desc(**bad), bad_conv)            # ... before the conventions are looked at: they are bad here
            assert rc == _lib.ERR_SHAPE and word in msg and msg.startswith(who), (bad, rc, msg)
            with pytest.raises(TypeError):
                _lib.check(rc)
            assert query(_desc(**bad)) == 0
        # the order inside the group: n_src, n_scales, B, the frames
        assert "n_src" in call(_desc(n_src=0, n_scales=0, B=-1))[1] and "n_scales" in call(_desc(n_scales=0, B=-1))[1]
        assert "B=-1" in call(_desc(B=-1, H=(0, 1)))[1]
    assert query(None) == 0


def test_then_the_conventions_when_there_are_some():
    for call, who in CALLS:
        for bad, word in BAD_CONVS:
            for d in (_desc(intrinsics=None), _desc(B=0)):                                     # before the pointers, before the empty batch
                rc, msg = call(d, _conv(**bad))
                assert rc == _lib.ERR_CONFIG and word in msg and msg.startswith(who), (bad, rc, msg)
                with pytest.raises(ValueError):
                    _lib.check(rc)
        assert call(_desc(B=0), _conv(invert=(1, 0, 7)))[0] == 0, "an invert flag beyond n_src is not looked at"
        assert call(_desc(B=0, n_src=3), _conv(invert=(1, 0, 7)))[0] == _lib.ERR_CONFIG
        assert "pose_format" in call(_desc(), _conv(fmt=5, invert=(2, 0), scale=float("nan")))[1]
        assert "invert[0]=2" in call(_desc(), _conv(fmt=MATRIX, invert=(2, 0), scale=float("nan")))[1]
    for bad, _ in BAD_CONVS:
        assert query(_desc(), _conv(**bad)) == 0
    assert query(_desc(), None) > 0, "no conventions: the defaults"


@pytest.mark.parametrize("conv", [None, dict(fmt=EULER, invert=(), scale=1.0, shift=0.0), dict(), dict(fmt=MATRIX, invert=())],
                         ids=["none", "default", "axis_angle", "matrix"])
def test_then_the_empty_batch_the_pointers_and_the_workspace(conv):
    c = _conv(**conv) if conv is not None else None
    empty = _desc(B=0, intrinsics=None)
    assert fwd(empty, c)[0] == 0 and bwd(empty, c, None, 0)[0] == 0
    order = [("intrinsics", (fwd, bwd)), (("disp", 0), (fwd, bwd)), (("src_disp", 0), (fwd, bwd)), (("diff", 0), (fwd,)), (("g_diff", 0), (bwd,)),
             (("d_disp", 0), (bwd,)), (("disp", 1), (fwd, bwd)), (("src_disp", 1), (fwd, bwd)), (("diff", 1), (fwd,)), (("g_diff", 1), (bwd,)),
             (("d_disp", 1), (bwd,)), (("pose", 0), (fwd, bwd)), (("d_pose", 0), (bwd,)), (("pose", 1), (fwd, bwd)), (("d_pose", 1), (bwd,))]
    for k, (field, calls) in enumerate(order):
        for call in calls:
            # this pointer and every later one of the call NULL: the first in the documented order is the one that is named
            null = {}
            for later, later_calls in order[k:]:
                if call in later_calls:
                    if isinstance(later, tuple):
                        null.setdefault(later[0], []).append(later[1])
                    else:
                        null[later] = None
            d = _desc()
            for name, where in null.items():
                if where is None:
                    setattr(d, name, None)
                else:
                    for at in where:
                        getattr(d, name)[at] = None
            rc, msg = call(d, c)
            assert rc == _lib.ERR_NULL and ("%s[%d]" % field if isinstance(field, tuple) else field) in msg, (field, rc, msg)
    # the optional ones, each on its own and all together; entries beyond n_scales and n_src are not looked at
    for names in (("valid",), ("computed",), ("projected",), ("d_src_disp",), ("valid", "computed", "projected", "d_src_disp")):
        d = _desc(B=0)
        for name in names:
            for s in range(_lib.SFM_MAX_SCALES):
                getattr(d, name)[s] = None
        assert fwd(d, c)[0] == 0 and bwd(d, c)[0] == 0
    assert bwd(_desc(intrinsics=None), c, None, 0)[0] == _lib.ERR_NULL                          # the pointers before the workspace
    d = _desc()
    need = query(d, c)
    assert need == -(-(2 * (2 + 1) * 2 * 12 * 4) // 256) * 256, "(blocks of all scales and samples) * n_src * 12 floats"
    for ws, nbytes, word in ((None, need, "needed"), (WS, need - 1, "needed"), (C.c_void_p(WS.value + 128), need, "aligned")):
        rc, msg = bwd(d, c, ws, nbytes)
        assert rc == _lib.ERR_WORKSPACE and word in msg and msg.startswith("sfm_depth_consistency_bwd"), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    bare = _desc(intrinsics=None)
    for s in range(_lib.SFM_MAX_SCALES):
        for name in POINTERS:
            getattr(bare, name)[s] = None
    assert query(bare, c) == need, "the query looks at no pointer, and the workspace does not depend on the conventions"


def test_the_workspace_is_the_pyramid_warps():
    for B, n_src, hw in ((3, 3, ((130, 127), (16, 52))), (1, 1, ((3, 3),)), (2, 8, ((20, 130), (10, 65), (5, 32)))):
        d = _desc(B=B, n_src=n_src, n_scales=len(hw), hw=hw)
        wp = _lib.SfmWarpPyramidDesc()
        wp.B, wp.n_src, wp.n_scales = B, n_src, len(hw)
        for s, (h, w) in enumerate(hw):
            wp.H[s], wp.W[s] = h, w
        c = _conv()      # (the pyramid warp's query that looks at no pointer is the one with conventions)
        assert query(d) == query(d, c) == L.sfm_warp_pyramid_conv_bwd_workspace_bytes(C.byref(wp), C.byref(c)) > 0


# ------------------------------------------------------------------------------------------------------------------------
# 4. the Python argument errors that need no device
# ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_anything_else():
    x = torch.zeros(1)                       # never looked at
    for bad, word in ((dict(pose_format="quaternion"), "pose_format"), (dict(depth_range=(0.0, 100.0)), "depth_range"),
                      (dict(depth_range=(2.0, 1.0)), "depth_range"), (dict(depth_range=0.1), "depth_range"), (dict(invert=True), "invert"),
                      (dict(invert=[2, 0]), "invert"), (dict(invert="ab"), "invert"), (dict(pose_format="matrix", invert=[True, False]), "matrix")):
        with pytest.raises(ValueError, match=word):
            ta.depth_consistency([x], [x], x, [x], **bad)
    with pytest.raises(TypeError):           # valid conventions: the first complaint is about the arrays (CPU tensors)
        ta.depth_consistency([x], [x], x, [x], pose_format="axis_angle", invert=[True, False], depth_range=(0.1, 100.0))
    with pytest.raises(TypeError, match="per scale"):
        ta.depth_consistency(x, [x], x, [x])
    with pytest.raises(TypeError, match="scales"):
        ta.depth_consistency([x], [x, x], x, [x])
    with pytest.raises(TypeError, match="scales"):
        ta.depth_consistency([], [], x, [x])
    for fn, args in ((ops.depth_consistency_fwd, ([x], [x], [x, x], x)), (ops.depth_consistency_bwd, ([x], [x], [x, x], x, [x]))):
        with pytest.raises(ValueError, match="pose_format"):
            fn(*args, pose_format="rodrigues")
        with pytest.raises(ValueError, match="invert"):
            fn(*args, invert=[True])
        with pytest.raises(ValueError, match="matrix"):
            fn(*args, pose_format="matrix", invert=[False, True])
        with pytest.raises(ValueError, match="depth_affine"):
            fn(*args, depth_affine=(float("nan"), 0.0))
        with pytest.raises(TypeError, match="one entry per scale"):
            fn(*((args[0], [x, x]) + args[2:]))
        with pytest.raises(TypeError, match="CPU"):
            fn(*args)
