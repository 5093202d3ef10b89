"""sfm_warp_full_res_* (include/sfmwarp_full_res.h) without a GPU: the side header, the binding and the library declare the same
three entry points and the same descriptor; every documented rejection answers with its code and a message, in the documented order
and before any HIP call (the pointers are fakes that are never dereferenced); the workspace query; and the NumPy restatement of the
upsampling and its adjoint (tests/warp_full_res_ref.py) against the oracle's resize and, in float64, against itself as an adjoint."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import warp_full_res_ref as R
from oracle import sfm_oracle as O

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmwarp_full_res.h")
CSRC = os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc")
FAKE = 0x10000                 # never dereferenced
ENTRY_POINTS = ["sfm_warp_full_res_bwd", "sfm_warp_full_res_bwd_workspace_bytes", "sfm_warp_full_res_fwd"]
CONSTANTS = {"SFM_MAX_SCALES": _lib.SFM_MAX_SCALES, "SFM_MAX_SRC": _lib.SFM_MAX_SRC}
F32, F64 = np.float32, np.float64

with open(HEADER) as _f:
    RAW = _f.read()
TEXT = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)      # the header without its comments


# ------------------------------------------------------------------------------------------------------------------------
# 1. + 2. header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def _prototypes():
    code = re.sub(r"^\s*#.*$", "", TEXT, flags=re.M)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(sfm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}


def _struct_fields():
    """[(field, ctypes element type, count)] of SfmWarpFullResDesc in declaration order"""
    body = re.search(r"typedef struct SfmWarpFullResDesc \{(.*?)\} SfmWarpFullResDesc;", TEXT, flags=re.S).group(1)
    kinds = {"const float *": C.c_void_p, "float *": C.c_void_p, "int32_t ": C.c_int32}
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const float \*|float \*|int32_t )(.*)$", decl)
        assert m, decl
        for item in m.group(2).split(","):
            a = re.match(r"(\w+)(?:\[(\w+)\])?$", item.strip().lstrip("*"))
            assert a, item
            fields.append((a.group(1), kinds[m.group(1)], CONSTANTS[a.group(2)] if a.group(2) else 1))
    return fields


def test_the_side_header_stands_beside_the_main_one():
    assert '#include "sfmwarp.h"' in RAW
    first = re.search(r"/\*.*?\*/", RAW, flags=re.S).group(0)
    assert "sfmwarp.h" in first and "FOLLOW-UP" in first, "the first comment says that this header is to be folded into sfmwarp.h"
    assert "SFM_ABI_VERSION" not in TEXT and _lib.SFM_ABI_VERSION == 6
    assert "#define" not in re.sub(r"#define SFMWARP_FULL_RES_H_", "", TEXT), "it uses the constants of sfmwarp.h, it adds none"


def test_the_symbol_table_is_the_headers_and_disjoint_from_the_other_three():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.FULL_RES_SYMBOLS) == ENTRY_POINTS
    for other in (_lib.SYMBOLS, _lib.EXT_SYMBOLS, _lib.SMOOTH_SYMBOLS):
        assert not set(_lib.FULL_RES_SYMBOLS) & set(other)
    for name, params in protos.items():
        res, args = _lib.FULL_RES_SYMBOLS[name]
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        assert len(args) == len(params), name
        assert res is (C.c_size_t if name.endswith("_bytes") else C.c_int)
        for param, arg in zip(params, args):                       # pointers at the header's positions, integers elsewhere
            if param.startswith("const SfmWarpFullResDesc *"):
                assert arg == C.POINTER(_lib.SfmWarpFullResDesc), (name, param)
            elif "*" in param:
                assert arg is C.c_void_p, (name, param)
            else:
                assert param.startswith("size_t ") and arg is C.c_size_t, (name, param)


def test_descriptor_matches_the_header():
    fields = _struct_fields()
    struct = _lib.SfmWarpFullResDesc
    assert [f[0] for f in fields] == [f[0] for f in struct._fields_] == [
        "B", "n_src", "n_scales", "H", "W", "h", "w", "image_layout", "src", "disp", "intrinsics", "pose", "warped", "valid", "g_warped",
        "d_disp", "d_pose"]
    off, align = 0, 1
    for (field, ctype, count), (_, bound) in zip(fields, struct._fields_):
        size = C.sizeof(ctype)
        off = -(-off // size) * size                                # the C layout rule: a multiple of the element size
        assert getattr(struct, field).offset == off, field
        assert getattr(struct, field).size == size * count, field
        elem = bound._type_ if count > 1 else bound
        assert C.sizeof(elem) == size, field
        off += size * count
        align = max(align, size)
    assert C.sizeof(struct) == -(-off // align) * align


def test_the_library_exports_the_three_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported
    assert L.sfm_abi_version() == 6


def test_the_resampling_helpers_have_one_copy():
    """resize_coord, resize_taps, resize_blend and resize_first_at are defined in csrc/sfm_resize.h and nowhere else; both units
    that resample include it; the block of the new unit is the pyramid's"""
    units = {name: open(os.path.join(CSRC, name)).read() for name in os.listdir(CSRC) if name.endswith((".hip", ".h"))}
    for fn in ("resize_coord", "resize_tap0", "resize_taps", "resize_blend", "resize_read", "resize_first_at"):
        defined = [name for name, text in units.items() if re.search(r"__forceinline__ \w+ %s\(" % fn, text)]
        assert defined == ["sfm_resize.h"], (fn, defined)
    for name in ("sfm_ops.hip", "sfm_warp_full_res.hip"):
        assert '#include "sfm_resize.h"' in units[name]
    block = lambda name, const: int(re.search(r"constexpr int %s = (\d+);" % const, units[name]).group(1))
    assert block("sfm_warp_full_res.hip", "WF_BLOCK") == block("sfm_warp_pyramid.hip", "WP_BLOCK") == 256


# ------------------------------------------------------------------------------------------------------------------------
# 3. reject paths: what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _desc(B=2, n_src=2, n_scales=2, H=16, W=24, hw=((16, 24), (5, 7)), image_layout=0, **kw):
    d = _lib.SfmWarpFullResDesc()
    d.B, d.n_src, d.n_scales, d.H, d.W, d.image_layout = B, n_src, n_scales, H, W, image_layout
    for s, (h, w) in enumerate(hw):
        d.h[s], d.w[s] = h, w
    for s in range(_lib.SFM_MAX_SCALES):
        d.disp[s] = d.warped[s] = d.valid[s] = d.g_warped[s] = d.d_disp[s] = FAKE
    for i in range(_lib.SFM_MAX_SRC):
        d.pose[i] = d.d_pose[i] = FAKE
    d.src = d.intrinsics = FAKE
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


WS = C.c_void_p(0x100000)      # on a 256-byte boundary, never dereferenced


def _fwd(d):
    return L.sfm_warp_full_res_fwd(C.byref(d) if d is not None else None, None), _lib.last_error()


def _bwd(d, ws=WS, nbytes=1 << 40):
    return L.sfm_warp_full_res_bwd(C.byref(d) if d is not None else None, ws, nbytes, None), _lib.last_error()


def _query(d):
    return L.sfm_warp_full_res_bwd_workspace_bytes(C.byref(d) if d is not None else None)


def _both(d):
    return (("sfm_warp_full_res_fwd",) + _fwd(d), ("sfm_warp_full_res_bwd",) + _bwd(d))


def test_null_descriptor():
    for who, rc, msg in _both(None):
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
    assert _query(None) == 0


BAD_SHAPES = [(dict(n_src=0), "n_src"), (dict(n_src=9), "n_src"), (dict(n_scales=0), "n_scales"), (dict(n_scales=9), "n_scales"),
              (dict(B=-1), "B="), (dict(H=2), "H="), (dict(W=2), "W="), (dict(h=(1, 0)), "scale 1"), (dict(w=(0, -3)), "scale 0"),
              (dict(H=1 << 15, W=1 << 15), "3*H*W"), (dict(h=(1, 1 << 15), w=(1, 1 << 15)), "3*h*w"),
              (dict(B=(1 << 31) - 1, H=3, W=3), "256-pixel blocks"),
              (dict(B=1 << 20, n_scales=1, H=3, W=3, h=(0, 1 << 14), w=(0, 1 << 14)), "256-element blocks")]


@pytest.mark.parametrize("bad,word", BAD_SHAPES, ids=[w for _, w in BAD_SHAPES])
def test_bad_shapes(bad, word):
    for who, rc, msg in _both(_desc(**bad)):
        assert rc == _lib.ERR_SHAPE and msg.startswith(who) and word in msg, (rc, msg)
        with pytest.raises(TypeError):
            _lib.check(rc)
    assert _query(_desc(**bad)) == 0


def test_sizes_beyond_n_scales_are_not_looked_at():
    assert _fwd(_desc(B=0, n_scales=1, hw=((16, 24), (0, -1))))[0] == 0


@pytest.mark.parametrize("layout", [-1, 2])
def test_bad_layout(layout):
    for who, rc, msg in _both(_desc(image_layout=layout)):
        assert rc == _lib.ERR_CONFIG and msg.startswith(who) and "image_layout" in msg, (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert _query(_desc(image_layout=layout)) == 0


FWD_PTRS = ["intrinsics", "src", ("disp", 0), ("warped", 1), ("pose", 1)]
BWD_PTRS = ["intrinsics", "src", ("disp", 1), ("g_warped", 0), ("d_disp", 1), ("pose", 0), ("d_pose", 1)]


def _null(field):
    return {field[0]: (field[1], None)} if isinstance(field, tuple) else {field: None}


def _named(field):
    return "%s[%d]" % field if isinstance(field, tuple) else field


@pytest.mark.parametrize("field", FWD_PTRS, ids=str)
def test_forward_null_pointers(field):
    rc, msg = _fwd(_desc(**_null(field)))
    assert rc == _lib.ERR_NULL and _named(field) in msg and msg.startswith("sfm_warp_full_res_fwd"), (rc, msg)
    with pytest.raises(TypeError):
        _lib.check(rc)


@pytest.mark.parametrize("field", BWD_PTRS, ids=str)
def test_backward_null_pointers(field):
    rc, msg = _bwd(_desc(**_null(field)))
    assert rc == _lib.ERR_NULL and _named(field) in msg and msg.startswith("sfm_warp_full_res_bwd"), (rc, msg)


def test_each_call_ignores_the_others_arrays():
    """valid may be NULL scale by scale; the backward does not look at warped and valid: with those NULL it gets as far as its
    workspace check.  The forward does not look at g_warped, d_disp and d_pose: with those NULL it has no check left and would
    launch, so its descriptor keeps one NULL pointer of its own, the last it checks."""
    d = _desc()
    for s in range(_lib.SFM_MAX_SCALES):
        d.warped[s] = d.valid[s] = None
    rc, msg = _bwd(d, None, 0)
    assert rc == _lib.ERR_WORKSPACE, (rc, msg)
    d = _desc(pose=(1, None))
    for s in range(_lib.SFM_MAX_SCALES):
        d.valid[s] = d.g_warped[s] = d.d_disp[s] = None
    for i in range(_lib.SFM_MAX_SRC):
        d.d_pose[i] = None
    rc, msg = _fwd(d)
    assert rc == _lib.ERR_NULL and "pose[1]" in msg, (rc, msg)


def test_workspace_rejections():
    d = _desc()
    need = _query(d)
    assert need > 0
    for ws, nbytes, word in ((None, need, "needed"), (WS, need - 1, "needed"), (WS, 0, "needed"), (C.c_void_p(WS.value + 128), need, "aligned"),
                             (C.c_void_p(WS.value + 4), 1 << 30, "aligned")):
        rc, msg = _bwd(d, ws, nbytes)
        assert rc == _lib.ERR_WORKSPACE and word in msg and msg.startswith("sfm_warp_full_res_bwd"), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)


def test_rejections_come_in_the_documented_order():
    """descriptor, shape, layout, the empty batch, the pointers, the workspace"""
    null = dict(src=None, disp=(0, None))
    for call in (_fwd, _bwd):
        assert call(_desc(n_src=0, image_layout=7, **null))[0] == _lib.ERR_SHAPE
        assert call(_desc(H=2, image_layout=7, B=0))[0] == _lib.ERR_SHAPE
        assert call(_desc(h=(1, 0), image_layout=7, B=0))[0] == _lib.ERR_SHAPE
        assert call(_desc(image_layout=7, **null))[0] == _lib.ERR_CONFIG
        assert call(_desc(B=0, image_layout=7))[0] == _lib.ERR_CONFIG              # an empty batch still has its layout checked
        assert call(_desc(B=0, **null))[0] == 0                                    # ... but not its pointers
        assert call(_desc(**null))[0] == _lib.ERR_NULL
    # inside the shape group, in the header's order: n_src, n_scales, B, H and W, h and w, 3*H*W, 3*h*w
    for bad, word in ((dict(n_src=0, n_scales=0), "n_src"), (dict(n_scales=0, B=-1), "n_scales"), (dict(B=-1, H=2), "B="),
                      (dict(H=2, h=(0, 0)), "H="), (dict(h=(0, 0), H=1 << 15, W=1 << 15), "h=0"),
                      (dict(H=1 << 15, W=1 << 15, h=(1, 1 << 15), w=(1, 1 << 15)), "3*H*W")):
        assert word in _fwd(_desc(**bad))[1], bad
    # inside the pointers: intrinsics, src, then scale by scale, then source by source
    assert "intrinsics" in _bwd(_desc(intrinsics=None, src=None))[1]
    assert "src" in _bwd(_desc(src=None, disp=(0, None)))[1]
    assert "disp[0]" in _bwd(_desc(disp=(0, None), g_warped=(0, None)))[1]
    assert "g_warped[0]" in _bwd(_desc(g_warped=(0, None), d_disp=(0, None)))[1]
    assert "d_disp[0]" in _bwd(_desc(d_disp=(0, None), disp=(1, None)))[1]
    assert "disp[1]" in _bwd(_desc(disp=(1, None), pose=(0, None)))[1]
    assert "pose[0]" in _bwd(_desc(pose=(0, None), d_pose=(0, None)))[1]
    assert _bwd(_desc(**null), None, 0)[0] == _lib.ERR_NULL                        # the pointers before the workspace
    assert _bwd(_desc(B=0), None, 0)[0] == 0                                       # an empty batch needs no workspace


def test_empty_batch_launches_nothing_and_checks_no_pointer():
    e = _lib.SfmWarpFullResDesc()          # an empty shard: every pointer NULL, the shape and the layout still checked
    e.n_src, e.n_scales, e.H, e.W, e.h[0], e.w[0] = 2, 1, 16, 24, 4, 6
    assert _fwd(e)[0] == 0 and _bwd(e, None, 0)[0] == 0
    assert _query(e) == 256
    e.H = 2
    assert _fwd(e)[0] == _lib.ERR_SHAPE and _bwd(e, None, 0)[0] == _lib.ERR_SHAPE and _query(e) == 0


# ------------------------------------------------------------------------------------------------------------------------
# 4. the workspace query
# ------------------------------------------------------------------------------------------------------------------------
QUERIES = [(1, 1, (3, 3), [(3, 3)]), (1, 1, (3, 3), [(1, 1)]), (2, 3, (24, 40), [(24, 40), (12, 20), (6, 10), (3, 5)]),
           (2, 1, (13, 21), [(13, 21), (7, 10), (1, 1)]), (2, 3, (130, 127), [(130, 127), (65, 63), (17, 9)]),
           (32, 2, (128, 416), [(128, 416), (64, 208), (32, 104), (16, 52)]), (3, 2, (16, 16), [(32, 32), (16, 16)])]


@pytest.mark.parametrize("B,n_src,HW,hw", QUERIES)
def test_workspace_query(B, n_src, HW, hw):
    """a multiple of 256 that holds 48 bytes per 256-pixel block and source plus B*H*W floats per resampled scale, and no more than
    the next multiple; it looks at no pointer"""
    d = _lib.SfmWarpFullResDesc()          # every pointer NULL
    d.B, d.n_src, d.n_scales, d.H, d.W = B, n_src, len(hw), HW[0], HW[1]
    for s, (h, w) in enumerate(hw):
        d.h[s], d.w[s] = h, w
    got = _query(d)
    blocks = len(hw) * B * -(-(HW[0] * HW[1]) // 256)
    resampled = sum(1 for s in hw if s != HW)
    assert got % 256 == 0 and got == -(-(48 * n_src * blocks + 4 * B * HW[0] * HW[1] * resampled) // 256) * 256
    assert got == R.workspace_bytes(B, n_src, HW[0], HW[1], hw)
    assert _query(_desc(B=B, n_src=n_src, n_scales=len(hw), H=HW[0], W=HW[1], hw=hw)) == got      # the same with every pointer bound
    d.image_layout = 1
    assert _query(d) == got
    d.B = B + 40
    assert _query(d) > got                                                   # it grows with the batch


# ------------------------------------------------------------------------------------------------------------------------
# 5. the NumPy restatement of the upsampling and its adjoint
# ------------------------------------------------------------------------------------------------------------------------
PAIRS = [(HW, hw) for HW, sizes in R.SHAPES.values() for hw in sizes[1:]] + [((24, 40), (24, 40)), ((9, 7), (20, 3))]


@pytest.mark.parametrize("HW,hw", PAIRS, ids=["%dx%d-from-%dx%d" % (HW + hw) for HW, hw in PAIRS])
def test_the_restatement_is_the_oracles_resize(HW, hw):
    """float64: the oracle's F.resize_images, which samples at numpy.linspace where the kernels sample at o * step, to 1e-12; float32:
    to a coordinate's rounding -- a position within one float32 spacing of the oracle's, the value moving by at most max - min per
    pixel of position on each axis -- plus the blend's three roundings"""
    x = np.random.RandomState(3).uniform(0.01, 10.0, (2, 1) + hw)
    assert np.abs(R.upsample(x, HW, F64) - O.resize_images(x, HW, F64)).max() <= 1e-12 * 10
    got, want = R.upsample(x, HW, F32), O.resize_images(x.astype(F32), HW, F32)
    assert got.dtype == F32 and got.shape == (2, 1) + HW
    bound = 2 * 10.0 * float(np.spacing(F32(max(hw)))) + 3 * 2.0 ** -24 * 10.0
    assert np.abs(got.astype(F64) - want.astype(F64)).max() <= bound
    if hw == HW:        # equal sizes: a step of exactly 1, weights 1 and 0 -- the map is the identity
        assert np.array_equal(got, x.astype(F32))
    if hw == (1, 1):    # one element: a step of 0, every output is that element
        assert np.array_equal(got, np.broadcast_to(x.astype(F32), got.shape))


@pytest.mark.parametrize("HW,hw", PAIRS, ids=["%dx%d-from-%dx%d" % (HW + hw) for HW, hw in PAIRS])
def test_the_restated_adjoint_is_the_adjoint(HW, hw):
    """<R x, y> = <x, R^T y> in float64 to its rounding, R^T against aten's float64 autograd, and the float32 statement within the
    roundings of its own sums of the float64 one"""
    rng = np.random.RandomState(4)
    x, y = rng.standard_normal((2, 1) + hw), rng.standard_normal((2, 1) + HW)
    rx, rty = R.upsample(x, HW, F64), R.adjoint(y, hw, F64)
    lhs, rhs = float((rx * y).sum()), float((x * rty).sum())
    scale = float(np.abs(rx * y).sum())
    assert abs(lhs - rhs) <= 1e-13 * scale, (lhs, rhs)
    assert rty.shape == x.shape and np.abs(rty - R.adjoint64_aten(y, hw)).max() <= 1e-12 * max(1.0, float(np.abs(rty).max()))
    assert float(rty.sum()) == pytest.approx(float(y.sum()), rel=1e-12, abs=1e-9)      # the weights of one output add up to 1
    r32 = R.adjoint(y, hw, F32)
    terms = R.adjoint(np.abs(y), hw, F64)                                            # the sum of |contributions| per element
    # per contribution: the weights' position error (a float32 spacing of the coordinate per axis), the product and the running sum
    n_terms = -(-HW[0] // hw[0]) * -(-HW[1] // hw[1]) * 4 + 4
    bound = terms * (2 * float(np.spacing(F32(max(hw)))) + (n_terms + 3) * 2.0 ** -24) + 1e-30
    assert r32.dtype == F32 and (np.abs(r32.astype(F64) - rty) <= bound).all()


# ------------------------------------------------------------------------------------------------------------------------
# ops.warp_full_res_* and torch_api.warp_full_res: what they refuse before anything reaches the library
# ------------------------------------------------------------------------------------------------------------------------
def test_type_and_value_errors():
    assert "warp_full_res" in ta.__all__ and {"warp_full_res_fwd", "warp_full_res_bwd"} <= set(ops.__all__)
    src, K = torch.zeros(2, 2, 3, 16, 24), torch.eye(3).repeat(2, 1, 1)
    disps, poses = [torch.ones(2, 1, 16, 24), torch.ones(2, 1, 4, 6)], [torch.zeros(2, 6)] * 2
    with pytest.raises(TypeError):                                   # CPU tensors: there is no CPU path
        ta.warp_full_res(src, K, disps, poses)
    with pytest.raises(TypeError):
        ops.warp_full_res_fwd(src.view(2, 6, 16, 24), disps, poses, K, "planar")
    with pytest.raises(ValueError, match="layout"):
        ops.warp_full_res_fwd(src.view(2, 6, 16, 24), disps, poses, K, "chw")
    with pytest.raises(TypeError, match="per scale"):
        ops.warp_full_res_fwd(src.view(2, 6, 16, 24), [], poses, K, "planar")
    import inspect
    assert inspect.signature(ta.min_reprojection_loss).parameters["full_res"].default is False
