"""include/sfmwarp_pose.h without a GPU: the side header, the binding and the library declare the same struct and the same eight entry
points; every documented rejection answers with its code, in the documented order and before any HIP call (the pointers are fakes
that are never dereferenced); the workspace queries; the restatement of the pose conventions (tests/pose_conv_ref.py) against
torch.linalg.matrix_exp, its own inverse and the oracle; and the Python argument errors that are raised before a device is touched."""
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
import pose_conv_ref as R
from oracle import sfm_oracle as O

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmwarp_pose.h")
CSRC = os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc")
FAKE = 0x10000                 # never dereferenced
WS = C.c_void_p(0x100000)      # on a 256-byte boundary, never dereferenced
ENTRY_POINTS = sorted(["sfm_pose_mat_fwd", "sfm_pose_mat_bwd", "sfm_warp_pyramid_conv_fwd", "sfm_warp_pyramid_conv_bwd_workspace_bytes",
                       "sfm_warp_pyramid_conv_bwd", "sfm_warp_full_res_conv_fwd", "sfm_warp_full_res_conv_bwd_workspace_bytes",
                       "sfm_warp_full_res_conv_bwd"])
EULER, AXIS, MATRIX = 0, 1, 2
F32, F64 = np.float32, np.float64

with open(HEADER) as _f:
    RAW = _f.read()
TEXT = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)      # the header without its comments


# ------------------------------------------------------------------------------------------------------------------------
# 1. header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def _prototypes():
    code = re.sub(r"^\s*#.*$", "", TEXT, flags=re.M)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(sfm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}


def test_the_side_header_stands_beside_the_main_one():
    assert '#include "sfmwarp.h"' in RAW and '#include "sfmwarp_full_res.h"' in RAW
    first = re.search(r"/\*.*?\*/", RAW, flags=re.S).group(0)
    assert "sfmwarp.h" in first and "FOLLOW-UP" in first, "the first comment says that this header is to be folded into sfmwarp.h"
    assert "SFM_ABI_VERSION" not in TEXT and _lib.SFM_ABI_VERSION == 6 and L.sfm_abi_version() == 6
    assert "#define" not in re.sub(r"#define SFMWARP_POSE_H_", "", TEXT), "it uses the constants of sfmwarp.h, it adds no macro"
    assert TEXT.count("typedef") == 1, "one struct of its own: SfmPoseConv"


def test_the_struct_is_the_headers(monkeypatch):
    monkeypatch.setattr(AH, "TEXT", TEXT)
    assert [f[0] for f in AH.struct_fields("SfmPoseConv")] == ["pose_format", "invert", "disp_scale", "disp_shift"]
    AH.assert_layout(_lib.SfmPoseConv, "SfmPoseConv")
    assert C.sizeof(_lib.SfmPoseConv) == 4 + 4 * _lib.SFM_MAX_SRC + 8
    assert _lib.SfmPoseConv.invert.offset == 4 and _lib.SfmPoseConv.disp_scale.offset == 4 + 4 * _lib.SFM_MAX_SRC


def test_the_enum_is_the_name_table():
    enums = dict((name, int(value)) for name, value in re.findall(r"(SFM_[A-Z_]+) = (\d+)", TEXT))
    assert enums == {"SFM_POSE_EULER": 0, "SFM_POSE_AXIS_ANGLE": 1, "SFM_POSE_MATRIX": 2}
    assert _lib.POSE_FORMATS == {"euler": 0, "axis_angle": 1, "matrix": 2}
    assert [_lib.pose_format_id(n) for n in ("euler", "axis_angle", "matrix")] == [0, 1, 2]
    for bad in ("quaternion", None, 1, ""):
        with pytest.raises(ValueError, match="must be one of"):
            _lib.pose_format_id(bad)


def test_the_symbol_table_is_the_headers_and_disjoint_from_the_other_five():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.POSE_SYMBOLS) == ENTRY_POINTS
    for other in (_lib.SYMBOLS, _lib.EXT_SYMBOLS, _lib.SMOOTH_SYMBOLS, _lib.FULL_RES_SYMBOLS, _lib.CONV_SYMBOLS):
        assert not set(_lib.POSE_SYMBOLS) & set(other)
    kinds = {"const SfmWarpPyramidDesc *": C.POINTER(_lib.SfmWarpPyramidDesc), "const SfmWarpFullResDesc *": C.POINTER(_lib.SfmWarpFullResDesc),
             "const SfmPoseConv *": C.POINTER(_lib.SfmPoseConv), "const float *": C.c_void_p, "float *": C.c_void_p, "void *": C.c_void_p,
             "int32_t ": C.c_int32, "int ": C.c_int, "size_t ": C.c_size_t}
    for name, params in protos.items():
        res, args = _lib.POSE_SYMBOLS[name]
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        assert len(args) == len(params), name
        assert res is (C.c_size_t if name.endswith("_bytes") else C.c_int)
        assert re.search(r"\b(size_t|int) %s\(" % name, TEXT).group(1) == ("size_t" if name.endswith("_bytes") else "int")
        for param, arg in zip(params, args):
            kind = re.match(r"(const \w+ \*|\w+ \*|\w+ )", param).group(1)
            assert kinds[kind] == arg, (name, param)


def test_the_library_exports_the_eight_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported


def test_the_pose_code_has_one_copy():
    """one T builder, one backward, one P = K . T step: defined once, used by the operator unit and by both warps"""
    units = {name: open(os.path.join(CSRC, name)).read() for name in os.listdir(CSRC) if name.endswith((".hip", ".h"))}
    where = {"pose_mat": "sfm_pose.h", "pose_mat_backward": "sfm_pose.h", "axis_angle_rot": "sfm_pose.h", "make_geom": "sfm_pose.h",
             "geom_from_T": "sfm_common.h", "euler2mat": "sfm_common.h"}
    for fn, home in where.items():
        defined = [name for name, text in units.items() if re.search(r"__forceinline__ \w+ %s\(" % fn, text)]
        assert defined == [home], (fn, defined)
    for name in ("sfm_ops.hip", "sfm_warp_pyramid.hip", "sfm_warp_full_res.hip"):
        assert '#include "sfm_pose.h"' in units[name]
        assert "atomic" not in units[name].replace("No atomics", "").replace("no atomics", "") or name == "sfm_ops.hip"
    for name in ("sfm_warp_pyramid.hip", "sfm_warp_full_res.hip"):      # the format is a kernel argument looked at by the geometry lanes
        assert "make_geom_conv(A.conv" in units[name] and "pose_fold_conv(A.conv" in units[name]
    assert "fp contract(off)" in units["sfm_pose.h"]


def test_the_python_defaults_are_the_existing_calls():
    for fn in (ops.warp_pyramid_fwd, ops.warp_pyramid_bwd, ops.warp_full_res_fwd, ops.warp_full_res_bwd):
        p = inspect.signature(fn).parameters
        assert (p["pose_format"].default, p["invert"].default, p["depth_affine"].default) == ("euler", None, None), fn.__name__
    for fn in (ta.warp_pyramid, ta.warp_full_res, ta.min_reprojection_loss):
        p = inspect.signature(fn).parameters
        assert (p["pose_format"].default, p["invert"].default, p["depth_range"].default) == ("euler", None, None), fn.__name__
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("pose_format", "invert", "depth_range"))
    p = inspect.signature(ta.pose_matrix).parameters
    assert (p["pose_format"].default, p["invert"].default) == ("axis_angle", False)
    assert ops.pose_conv() is None and ops.pose_conv("euler", [False, False], (1.0, 0.0), 2) is None
    assert ops._warp_pyramid_calls(None) == (L.sfm_warp_pyramid_fwd, L.sfm_warp_pyramid_bwd_workspace_bytes, L.sfm_warp_pyramid_bwd)
    assert ops._warp_full_res_conv_calls("align_corners", None) == (L.sfm_warp_full_res_fwd, L.sfm_warp_full_res_bwd_workspace_bytes, L.sfm_warp_full_res_bwd)
    c = ops.pose_conv("axis_angle", [True, False], (9.99, 0.01), 2)
    assert (c.pose_format, list(c.invert)[:3], c.disp_scale, c.disp_shift) == (1, [1, 0, 0], F32(9.99), F32(0.01))
    assert ops.pose_conv("matrix").pose_format == 2 and ops.pose_conv(invert=[False, True]).invert[1] == 1


# ------------------------------------------------------------------------------------------------------------------------
# 2. what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _conv(fmt=AXIS, invert=(1, 0), scale=9.99, shift=0.01):
    c = _lib.SfmPoseConv()
    c.pose_format, c.disp_scale, c.disp_shift = fmt, scale, shift
    for i, v in enumerate(invert):
        c.invert[i] = v
    return c


DEFAULT = dict(fmt=EULER, invert=(), scale=1.0, shift=0.0)


def _set(d, kw):
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def _wp(B=2, n_src=2, n_scales=2, hw=((16, 24), (8, 12)), image_layout=0, **kw):
    d = _lib.SfmWarpPyramidDesc()
    d.B, d.n_src, d.n_scales, d.image_layout = B, n_src, n_scales, image_layout
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
    for s in range(_lib.SFM_MAX_SCALES):
        d.src[s] = d.disp[s] = d.warped[s] = d.valid[s] = d.g_warped[s] = d.d_disp[s] = FAKE
    for i in range(_lib.SFM_MAX_SRC):
        d.pose[i] = d.d_pose[i] = FAKE
    d.intrinsics = FAKE
    return _set(d, kw)


def _wf(B=2, n_src=2, n_scales=2, H=16, W=24, hw=((16, 24), (5, 7)), image_layout=0, **kw):
    d = _lib.SfmWarpFullResDesc()
    d.B, d.n_src, d.n_scales, d.H, d.W, d.image_layout = B, n_src, n_scales, H, W, image_layout
    for s, (h, w) in enumerate(hw):
        d.h[s], d.w[s] = h, w
    for s in range(_lib.SFM_MAX_SCALES):
        d.disp[s] = d.warped[s] = d.valid[s] = d.g_warped[s] = d.d_disp[s] = FAKE
    for i in range(_lib.SFM_MAX_SRC):
        d.pose[i] = d.d_pose[i] = FAKE
    d.src = d.intrinsics = FAKE
    return _set(d, kw)


def _ref(x):
    return C.byref(x) if x is not None else None


class Pyr:
    """the three pyramid entry points as (descriptor, conventions) -> answer"""
    name, make, null = "sfm_warp_pyramid_conv", staticmethod(_wp), dict(intrinsics=None)

    @staticmethod
    def fwd(d, c, up=0):
        return L.sfm_warp_pyramid_conv_fwd(_ref(d), _ref(c), None), _lib.last_error()

    @staticmethod
    def bwd(d, c, up=0, ws=WS, nbytes=1 << 40):
        return L.sfm_warp_pyramid_conv_bwd(_ref(d), _ref(c), ws, nbytes, None), _lib.last_error()

    @staticmethod
    def query(d, c, up=0):
        return L.sfm_warp_pyramid_conv_bwd_workspace_bytes(_ref(d), _ref(c))


class Full:
    name, make, null = "sfm_warp_full_res_conv", staticmethod(_wf), dict(intrinsics=None)

    @staticmethod
    def fwd(d, c, up=0):
        return L.sfm_warp_full_res_conv_fwd(_ref(d), up, _ref(c), None), _lib.last_error()

    @staticmethod
    def bwd(d, c, up=0, ws=WS, nbytes=1 << 40):
        return L.sfm_warp_full_res_conv_bwd(_ref(d), up, _ref(c), ws, nbytes, None), _lib.last_error()

    @staticmethod
    def query(d, c, up=0):
        return L.sfm_warp_full_res_conv_bwd_workspace_bytes(_ref(d), up, _ref(c))


WARPS = [Pyr, Full]
BAD_CONVS = [(dict(fmt=3), "pose_format=3"), (dict(fmt=-1), "pose_format=-1"), (dict(invert=(2, 0)), "invert[0]=2"),
             (dict(invert=(0, -1)), "invert[1]=-1"), (dict(fmt=MATRIX, invert=(0, 1)), "SFM_POSE_MATRIX"),
             (dict(scale=float("nan")), "disp_scale"), (dict(shift=float("inf")), "disp_shift"), (dict(scale=float("-inf")), "disp_scale")]


@pytest.mark.parametrize("E", WARPS, ids=lambda E: E.name)
def test_the_existing_rejections_come_first_with_their_codes(E):
    for call, who in ((E.fwd, E.name + "_fwd"), (E.bwd, E.name + "_bwd")):
        rc, msg = call(None, _conv())
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
        for bad in (dict(n_src=0), dict(n_src=9), dict(n_scales=0), dict(n_scales=9), dict(B=-1)):
            rc, msg = call(E.make(**bad), None)            # ... before the conventions are looked at: they are NULL here
            assert rc == _lib.ERR_SHAPE and msg.startswith(who), (bad, rc, msg)
            with pytest.raises(TypeError):
                _lib.check(rc)
        for layout in (-1, 2):
            rc, msg = call(E.make(image_layout=layout), None)      # c NULL after a bad image_layout: still the layout's code
            assert rc == _lib.ERR_CONFIG and "image_layout" in msg and msg.startswith(who), (rc, msg)
    assert E.query(None, _conv()) == 0 and E.query(E.make(n_src=0), _conv()) == 0 and E.query(E.make(image_layout=2), _conv()) == 0
    rc, msg = Full.fwd(_wf(), None, 9)                                                      # upsample before the conventions
    assert rc == _lib.ERR_CONFIG and "upsample=9" in msg
    assert Full.bwd(_wf(), None, 9)[0] == _lib.ERR_CONFIG and Full.query(_wf(), _conv(), 9) == 0


@pytest.mark.parametrize("E", WARPS, ids=lambda E: E.name)
def test_null_conventions_then_bad_conventions(E):
    for call, who in ((E.fwd, E.name + "_fwd"), (E.bwd, E.name + "_bwd")):
        rc, msg = call(E.make(**E.null), None)
        assert rc == _lib.ERR_NULL and "conventions" in msg and msg.startswith(who), (rc, msg)
        assert call(E.make(B=0), None)[0] == _lib.ERR_NULL                                 # ... before the empty batch
        for bad, word in BAD_CONVS:
            for d in (E.make(**E.null), E.make(B=0)):                                         # before the pointers, before the empty batch
                rc, msg = call(d, _conv(**bad))
                assert rc == _lib.ERR_CONFIG and word in msg and msg.startswith(who), (bad, rc, msg)
                with pytest.raises(ValueError):
                    _lib.check(rc)
        # an invert flag beyond n_src is not looked at
        assert call(E.make(B=0), _conv(invert=(1, 0, 7)))[0] == 0
        assert call(E.make(B=0, n_src=3, n_scales=1), _conv(invert=(1, 0, 7)))[0] == _lib.ERR_CONFIG
        # the order inside the group: format, the flags, MATRIX with a flag, the affine map
        assert "pose_format" in call(E.make(), _conv(fmt=5, invert=(2, 0), scale=float("nan")))[1]
        assert "invert[0]=2" in call(E.make(), _conv(fmt=MATRIX, invert=(2, 0), scale=float("nan")))[1]
        assert "SFM_POSE_MATRIX" in call(E.make(), _conv(fmt=MATRIX, invert=(1, 0), scale=float("nan")))[1]
    assert E.query(E.make(), None) == 0
    for bad, _ in BAD_CONVS:
        assert E.query(E.make(), _conv(**bad)) == 0


@pytest.mark.parametrize("E", WARPS, ids=lambda E: E.name)
@pytest.mark.parametrize("conv", [DEFAULT, dict(), dict(fmt=MATRIX, invert=())], ids=["default", "axis_angle", "matrix"])
def test_then_the_empty_batch_the_pointers_and_the_workspace(E, conv):
    c = _conv(**conv)
    assert E.fwd(E.make(B=0, **E.null), c)[0] == 0 and E.bwd(E.make(B=0, **E.null), c, 0, None, 0)[0] == 0
    for field, calls in (("intrinsics", (E.fwd, E.bwd)), (("disp", 1), (E.fwd, E.bwd)), (("warped", 0), (E.fwd,)), (("g_warped", 1), (E.bwd,)),
                         (("d_disp", 0), (E.bwd,)), (("pose", 1), (E.fwd, E.bwd)), (("d_pose", 0), (E.bwd,))):
        null = {field[0]: (field[1], None)} if isinstance(field, tuple) else {field: None}
        for call in calls:
            rc, msg = call(E.make(**null), c)
            assert rc == _lib.ERR_NULL and ("%s[%d]" % field if isinstance(field, tuple) else field) in msg, (field, rc, msg)
    assert E.bwd(E.make(**E.null), c, 0, None, 0)[0] == _lib.ERR_NULL                         # the pointers before the workspace
    d = E.make()
    need = E.query(d, c)
    assert need > 0 and need % 256 == 0
    for ws, nbytes, word in ((None, need, "needed"), (WS, need - 1, "needed"), (C.c_void_p(WS.value + 128), need, "aligned")):
        rc, msg = E.bwd(d, c, 0, ws, nbytes)
        assert rc == _lib.ERR_WORKSPACE and word in msg and msg.startswith(E.name + "_bwd"), (rc, msg)
    # the query looks at no pointer, and the workspace does not depend on the conventions
    bare = E.make()
    for s in range(_lib.SFM_MAX_SCALES):
        bare.disp[s] = bare.warped[s] = bare.g_warped[s] = bare.d_disp[s] = None
    bare.intrinsics = None
    assert E.query(bare, c) == need == E.query(d, _conv(**DEFAULT))


def test_the_workspace_is_the_existing_calls():
    wp, wf = _wp(B=3, n_src=3, hw=((130, 127), (16, 52))), _wf(B=3, n_src=3, H=20, W=30, hw=((20, 30), (13, 21)))
    for c in (_conv(**DEFAULT), _conv(), _conv(fmt=MATRIX, invert=())):
        assert Pyr.query(wp, c) == L.sfm_warp_pyramid_bwd_workspace_bytes(C.byref(wp)) > 0
        for up in (0, 1):
            assert Full.query(wf, c, up) == L.sfm_warp_full_res_up_bwd_workspace_bytes(C.byref(wf), up) > 0


def test_the_pose_operator_rejects():
    p = C.c_void_p(FAKE)
    fwd = lambda fmt, inv, N=4, a=p, b=p: (L.sfm_pose_mat_fwd(a, fmt, inv, b, N, None), _lib.last_error())
    bwd = lambda fmt, inv, N=4, a=p, b=p, c=p: (L.sfm_pose_mat_bwd(a, fmt, inv, b, c, N, None), _lib.last_error())
    for call, who in ((fwd, "sfm_pose_mat_fwd"), (bwd, "sfm_pose_mat_bwd")):
        for fmt in (MATRIX, 3, -1):
            rc, msg = call(fmt, 0)
            assert rc == _lib.ERR_CONFIG and "format=%d" % fmt in msg and msg.startswith(who), (rc, msg)
        for inv in (2, -1):
            rc, msg = call(AXIS, inv)
            assert rc == _lib.ERR_CONFIG and "invert=%d" % inv in msg and msg.startswith(who)
        assert call(AXIS, 1, -1)[0] == _lib.ERR_SHAPE and call(7, 0, -1)[0] == _lib.ERR_CONFIG
        assert call(EULER, 0, 0, None, None)[0] == 0                                        # an empty batch: nothing launched
        assert call(AXIS, 1, 4, None)[0] == _lib.ERR_NULL and call(AXIS, 1, 4, p, None)[0] == _lib.ERR_NULL
    assert bwd(EULER, 0, 4, p, p, None)[0] == _lib.ERR_NULL


# ------------------------------------------------------------------------------------------------------------------------
# 3. the restatement, in float64
# ------------------------------------------------------------------------------------------------------------------------
NORMS = (1e-3, 1e-2, 0.3, 2.5, 4.0)


def _skew(a):
    K = torch.zeros(a.shape[0], 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    return K


def test_axis_angle_is_the_matrix_exponential():
    """the formula's own 1e-7 shortens the axis by 1e-7 / |a|: at most 1.5e-7 in an entry of R here, so 1e-6 holds with room"""
    p = R.sample_poses(NORMS, seed=21).astype(F64)
    T = R.pose_matrix(p, "axis_angle", False, F64)
    want = torch.linalg.matrix_exp(_skew(torch.from_numpy(p[:, :3]))).numpy()
    err = np.abs(T[:, :, :3] - want).reshape(len(NORMS), -1).max(axis=1)
    print("axis_angle vs matrix_exp, per |a| %s: %s" % (NORMS, ["%.2g" % e for e in err]))
    assert err.max() <= 1e-6 and np.array_equal(T[:, :, 3], p[:, 3:])
    assert np.abs(R.pose_matrix_t(torch.from_numpy(p), "axis_angle").numpy() - T).max() <= 1e-15       # the torch statement is the same
    assert np.abs(np.linalg.norm(p[:, :3], axis=1) - NORMS).max() <= 1e-7


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_invert_composed_with_the_forward_is_the_identity(fmt):
    p = R.sample_poses(NORMS + (0.0,), seed=22).astype(F64)
    bottom = np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (len(p), 1, 1))
    A = np.concatenate([R.pose_matrix(p, fmt, False, F64), bottom], 1)
    Ainv = np.concatenate([R.pose_matrix(p, fmt, True, F64), bottom], 1)
    assert np.abs(A @ Ainv - np.eye(4)).max() <= 1e-6 and np.abs(Ainv @ A - np.eye(4)).max() <= 1e-6
    assert np.abs(R.pose_matrix_t(torch.from_numpy(p), fmt, True).numpy() - Ainv[:, :3]).max() <= 1e-15


def test_the_zero_vector_gives_the_identity_and_a_zero_gradient():
    p = np.zeros((2, 6), F64)
    p[1, 3:] = (0.1, -0.2, 0.3)
    g = np.random.RandomState(23).standard_normal((2, 3, 4))
    for dtype, tdtype in ((F64, torch.float64), (F32, torch.float32)):
        for invert in (False, True):
            T = R.pose_matrix(p, "axis_angle", invert, dtype)
            assert T.dtype == dtype and np.array_equal(T[:, :, :3], np.tile(np.eye(3, dtype=dtype), (2, 1, 1)))
            d = R.pose_matrix_grad(p, "axis_angle", invert, g, tdtype)
            assert np.array_equal(d[:, :3], np.zeros((2, 3))), "autograd gives exactly 0 at a = 0"
            assert np.abs(np.abs(d[:, 3:]) - np.abs(g[:, :, 3])).max() <= 1e-6       # R = I: the translation's gradient is +-g_t


def test_euler_is_the_oracle():
    p = R.sample_poses((0.01, 0.3, 2.5, 3.5), seed=24)
    p[3, :3] = (3.5, -0.2, 0.1)                      # one angle outside (-pi, pi): clipped
    for dtype in (F32, F64):
        T = R.pose_matrix(p, "euler", False, dtype)
        want = O.pose_vec2mat(p, dtype)
        assert T.dtype == dtype and np.array_equal(T, want[:, :3]) and np.array_equal(T[:, :, :3], O.euler2mat(p[:, :3], dtype))
    assert np.abs(R.pose_matrix_t(torch.from_numpy(p), "euler").numpy() - R.pose_matrix(p, "euler", False, F64)).max() <= 1e-15
    d = R.pose_matrix_grad(p, "euler", False, np.ones((4, 3, 4)))
    assert d[3, 0] == 0 and (d[:3, :3] != 0).all(), "the clip's gradient is 0 outside (-pi, pi)"


def test_the_float32_restatement_is_float32_close():
    """what the GPU test takes its bound from: the float32 statements are within float32 rounding of the float64 ones"""
    p = R.sample_poses((0.0,) + NORMS, seed=25)
    g = np.random.RandomState(26).standard_normal((len(p), 3, 4)).astype(F32)
    for fmt in R.FORMATS:
        for invert in (False, True):
            e = R.rel_err(R.pose_matrix(p, fmt, invert, F32), R.pose_matrix(p, fmt, invert, F64))
            assert e.max() <= 1e-6, (fmt, invert, e)
            e = R.rel_err(R.pose_matrix_grad(p, fmt, invert, g, torch.float32), R.pose_matrix_grad(p, fmt, invert, g))
            print("float32 autograd vs float64, %s invert=%d: %s" % (fmt, invert, ["%.2g" % v for v in e]))
            assert e.max() <= 1e-3, (fmt, invert, e)


def test_disp_affine_is_disp_to_depth():
    a, b = R.disp_affine((0.1, 100.0))
    assert (a, b) == (1 / 0.1 - 1 / 100.0, 1 / 100.0)
    disp = np.linspace(0, 1, 7)
    assert np.allclose(1 / (a * disp + b), 1 / (0.01 + (10 - 0.01) * disp), rtol=1e-15)
    assert ta._pose_conv_args(None, "euler", None, (0.1, 100.0)) == ("euler", None, (a, b))


# ------------------------------------------------------------------------------------------------------------------------
# 4. the Python argument errors that need no device
# ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_value_errors_before_anything_else():
    x = torch.zeros(1)                       # never looked at
    src = torch.zeros(1, 2, 3, 8, 8)         # a CPU tensor: only its shape is read, for the number of sources
    for fn, args in ((ta.warp_pyramid, (src, x, [x], [x])), (ta.warp_full_res, (src, x, [x], [x])),
                     (lambda *a, **k: ta.min_reprojection_loss(*a, ssim_rate=0.85, **k), (x, src, x, [x], [x]))):
        with pytest.raises(ValueError, match="pose_format"):
            fn(*args, pose_format="quaternion")
        for bad in ((0.0, 100.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (0.1, float("inf")), (0.1, float("nan")), (0.1,), 0.1, "ab", (0.1, 1.0, 2.0)):
            with pytest.raises(ValueError, match="depth_range"):
                fn(*args, depth_range=bad)
        for bad in ([True], [True, False, True], True, [2, 0], "ab"):
            with pytest.raises(ValueError, match="invert"):
                fn(*args, invert=bad)
        with pytest.raises(ValueError, match="matrix"):
            fn(*args, pose_format="matrix", invert=[True, False])
        with pytest.raises(TypeError):       # valid conventions: the first complaint is about the arrays
            fn(*args, pose_format="axis_angle", invert=[True, False], depth_range=(0.1, 100.0))
        with pytest.raises(TypeError):
            fn(*args, pose_format="matrix", invert=[False, False])
    with pytest.raises(ValueError, match="pose_format"):
        ta.pose_matrix(x, pose_format="matrix")
    with pytest.raises(ValueError, match="invert"):
        ta.pose_matrix(x, invert=[True])
    with pytest.raises(TypeError):
        ta.pose_matrix(x)                    # a CPU tensor
    with pytest.raises(ValueError, match="invert"):
        ops.pose_conv("axis_angle", [True], None, 2)
    with pytest.raises(ValueError, match="matrix"):
        ops.pose_conv("matrix", [False, True], None, 2)
    with pytest.raises(ValueError, match="depth_affine"):
        ops.pose_conv("euler", None, (float("nan"), 0.0))
    with pytest.raises(ValueError, match="pose_format"):
        ops.pose_mat_fwd(x, "matrix", 0)
    with pytest.raises(ValueError, match="pose_format"):
        ops.pose_mat_bwd(x, "rodrigues", 0, x)
