"""include/sfmwarp_conventions.h without a GPU: the side header, the binding and the library declare the same five entry points;
every documented rejection answers with its code and a message, in the documented order and before any HIP call (the pointers are
fakes that are never dereferenced); the workspace query; the NumPy restatement of the half-pixel upsampling and its adjoint
(tests/conventions_ref.py) against aten; the torch statement of the reflection-padded error, the ring fold of its backward, and, from
the references alone, that the cases of tests/test_conventions_gpu.py can tell the two paddings apart."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conventions_ref as R
import warp_full_res_ref as AC

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmwarp_conventions.h")
CSRC = os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc")
FAKE = 0x10000                 # never dereferenced
ENTRY_POINTS = ["sfm_photo_error_pad_bwd", "sfm_photo_error_pad_fwd", "sfm_warp_full_res_up_bwd", "sfm_warp_full_res_up_bwd_workspace_bytes",
                "sfm_warp_full_res_up_fwd"]
ZERO, REFLECT, ALIGN, HALF = 0, 1, 0, 1
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
    assert "#define" not in re.sub(r"#define SFMWARP_CONVENTIONS_H_", "", TEXT), "it uses the constants of sfmwarp.h, it adds no macro"
    assert "typedef" not in TEXT, "it uses the descriptors of sfmwarp.h and sfmwarp_full_res.h, it adds none"


def test_the_enums_are_the_name_tables():
    enums = dict((name, int(value)) for name, value in re.findall(r"(SFM_[A-Z_]+) = (\d+)", TEXT))
    assert enums == {"SFM_SSIM_PAD_ZERO": 0, "SFM_SSIM_PAD_REFLECT": 1, "SFM_UPSAMPLE_ALIGN_CORNERS": 0, "SFM_UPSAMPLE_HALF_PIXEL": 1}
    assert _lib.SSIM_PADDINGS == {"zero": 0, "reflect": 1} and _lib.UPSAMPLES == {"align_corners": 0, "half_pixel": 1}
    assert _lib.ssim_padding_id("reflect") == 1 and _lib.upsample_id("half_pixel") == 1
    for lookup in (_lib.ssim_padding_id, _lib.upsample_id):
        for bad in ("border", None, 1, ""):
            with pytest.raises(ValueError, match="must be one of"):
                lookup(bad)


def test_the_symbol_table_is_the_headers_and_disjoint_from_the_other_four():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.CONV_SYMBOLS) == ENTRY_POINTS
    for other in (_lib.SYMBOLS, _lib.EXT_SYMBOLS, _lib.SMOOTH_SYMBOLS, _lib.FULL_RES_SYMBOLS):
        assert not set(_lib.CONV_SYMBOLS) & set(other)
    descs = {"const SfmPhotoErrorDesc *": _lib.SfmPhotoErrorDesc, "const SfmWarpFullResDesc *": _lib.SfmWarpFullResDesc}
    for name, params in protos.items():
        res, args = _lib.CONV_SYMBOLS[name]
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        assert len(args) == len(params), name
        assert res is (C.c_size_t if name.endswith("_bytes") else C.c_int)
        assert re.search(r"\b(size_t|int) %s\(" % name, TEXT).group(1) == ("size_t" if name.endswith("_bytes") else "int")
        for k, (param, arg) in enumerate(zip(params, args)):
            if k == 0:
                assert arg == C.POINTER(descs[re.match(r"const \w+ \*", param).group(0)]), (name, param)
            elif param.startswith("int32_t "):
                assert k == 1 and arg is C.c_int32 and param.split()[1] == ("padding" if "photo" in name else "upsample"), (name, param)
            elif "*" in param:
                assert arg is C.c_void_p, (name, param)
            else:
                assert param.startswith("size_t ") and arg is C.c_size_t, (name, param)


def test_the_library_exports_the_five_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported


def test_the_helpers_have_one_copy_and_the_pinned_lines_stay():
    units = {name: open(os.path.join(CSRC, name)).read() for name in os.listdir(CSRC) if name.endswith((".hip", ".h"))}
    for fn in ("resize_hp_coord", "resize_hp_tap0", "resize_hp_taps", "resize_hp_first_at"):
        defined = [name for name, text in units.items() if re.search(r"__forceinline__ \w+ %s\(" % fn, text)]
        assert defined == ["sfm_resize.h"], (fn, defined)
    assert R.geometry() == [16, 62, 60]
    for name in ("sfm_photo_error.hip", "sfm_warp_full_res.hip"):
        assert "sfmwarp_conventions.h" in units[name]
    pe = units["sfm_photo_error.hip"]
    assert "__shared__" not in pe and "atomic" not in pe.replace("no atomics", ""), "no LDS, no atomics in the photo-error unit"
    assert "template <bool SSIM, bool REFLECT = false>" in pe and "template <bool HWC, bool HP = false>" in units["sfm_warp_full_res.hip"]


def test_the_python_defaults_are_the_existing_calls():
    for fn, arg, default in ((ops.photo_error_fwd, "padding", "zero"), (ops.photo_error_bwd, "padding", "zero"),
                             (ops.warp_full_res_fwd, "upsample", "align_corners"), (ops.warp_full_res_bwd, "upsample", "align_corners"),
                             (ta.photometric_error, "padding", "zero"), (ta.warp_full_res, "upsample", "align_corners"),
                             (ta.min_reprojection_loss, "ssim_padding", "zero"), (ta.min_reprojection_loss, "upsample", "align_corners")):
        assert inspect.signature(fn).parameters[arg].default == default, (fn.__name__, arg)
    assert ops._photo_error_calls("zero") == (L.sfm_photo_error_fwd, L.sfm_photo_error_bwd)
    assert ops._warp_full_res_calls("align_corners") == (L.sfm_warp_full_res_fwd, L.sfm_warp_full_res_bwd_workspace_bytes, L.sfm_warp_full_res_bwd)


def test_bad_names_are_value_errors_before_anything_else():
    x = torch.zeros(1)       # never looked at
    with pytest.raises(ValueError, match="padding"):
        ta.photometric_error([x], x, ssim_rate=0.85, padding="border")
    with pytest.raises(ValueError, match="upsample"):
        ta.warp_full_res(x, x, [x], [x], upsample="nearest")
    with pytest.raises(ValueError, match="ssim_padding"):
        ta.min_reprojection_loss(x, x, x, [x], [x], ssim_rate=0.85, ssim_padding="replicate")
    with pytest.raises(ValueError, match="upsample"):
        ta.min_reprojection_loss(x, x, x, [x], [x], ssim_rate=0.85, full_res=True, upsample="bicubic")
    with pytest.raises(ValueError, match="full_res=True"):
        ta.min_reprojection_loss(x, x, x, [x], [x], ssim_rate=0.85, upsample="half_pixel")
    with pytest.raises(ValueError, match="padding"):
        ops._photo_error_calls("border")
    with pytest.raises(ValueError, match="upsample"):
        ops._warp_full_res_calls("nearest")


# ------------------------------------------------------------------------------------------------------------------------
# 2. sfm_photo_error_pad_*: what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _pe(B=2, n_img=2, n_scales=2, hw=((16, 24), (9, 31)), ssim_rate=0.85, **kw):
    d = _lib.SfmPhotoErrorDesc()
    d.B, d.n_img, d.n_scales, d.ssim_rate = B, n_img, n_scales, ssim_rate
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
    for s in range(max(0, min(n_scales, _lib.SFM_MAX_SCALES))):
        d.img[s] = d.tgt[s] = d.err[s] = d.g_err[s] = d.d_img[s] = FAKE
    for k, v in kw.items():
        getattr(d, k)[v[0]] = v[1]
    return d


def _pe_both(d, padding):
    ref = C.byref(d) if d is not None else None
    out = []
    for name in ("sfm_photo_error_pad_fwd", "sfm_photo_error_pad_bwd"):
        out.append((name, getattr(L, name)(ref, padding, None), _lib.last_error()))
    return out


NULL_IMG = dict(img=(0, None))      # a descriptor that passes every check keeps one NULL pointer: nothing is ever launched here


@pytest.mark.parametrize("padding", [ZERO, REFLECT])
def test_photo_error_pad_repeats_the_existing_rejections(padding):
    for who, rc, msg in _pe_both(None, padding):
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
    for bad, word in ((dict(n_img=0), "n_img"), (dict(n_img=9), "n_img"), (dict(n_scales=0), "n_scales"), (dict(n_scales=9), "n_scales"),
                      (dict(B=-1), "B="), (dict(H=(1, 0)), "scale 1"), (dict(W=(0, -2)), "scale 0"),
                      (dict(H=(0, 1 << 15), W=(0, 1 << 15)), "3*H*W"), (dict(B=1 << 30, n_img=8, n_scales=1, hw=((16, 24),)), "tiles")):
        for who, rc, msg in _pe_both(_pe(**bad), padding):
            assert rc == _lib.ERR_SHAPE and msg.startswith(who) and word in msg, (bad, rc, msg)
            with pytest.raises(TypeError):
                _lib.check(rc)
    for rate in (-0.01, 1.01, float("nan"), float("inf")):
        for who, rc, msg in _pe_both(_pe(ssim_rate=rate), padding):
            assert rc == _lib.ERR_CONFIG and "ssim_rate" in msg and msg.startswith(who), (rc, msg)
    for rate in (0.0, 0.85, 1.0):
        assert all(rc == 0 for _, rc, _ in _pe_both(_pe(B=0, ssim_rate=rate), padding))
    for field, calls in ((("img", 1), (0, 1)), (("tgt", 0), (0, 1)), (("err", 1), (0,)), (("g_err", 0), (1,)), (("d_img", 1), (1,))):
        got = _pe_both(_pe(**{field[0]: (field[1], None)}), padding)
        for k in calls:
            who, rc, msg = got[k]
            assert rc == _lib.ERR_NULL and "%s[%d]" % field in msg and msg.startswith(who), (rc, msg)
            with pytest.raises(TypeError):
                _lib.check(rc)


@pytest.mark.parametrize("padding", [-1, 2, 7, 1 << 20])
def test_a_padding_outside_the_enum_is_a_config_error(padding):
    for who, rc, msg in _pe_both(_pe(**NULL_IMG), padding):
        assert rc == _lib.ERR_CONFIG and "padding=%d" % padding in msg and msg.startswith(who), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)


def test_reflection_needs_two_rows_and_columns_and_no_more():
    for hw in (((16, 24), (1, 31)), ((16, 1), (9, 31)), ((1, 1), (9, 31))):
        for who, rc, msg in _pe_both(_pe(hw=hw, **NULL_IMG), REFLECT):
            assert rc == _lib.ERR_SHAPE and "reflection" in msg and msg.startswith(who), (rc, msg)
            assert "scale %d" % (1 if hw[1][0] == 1 else 0) in msg
    for hw in (((2, 2), (2, 3)), ((3, 2), (3, 3))):            # taken: the first complaint is the NULL pointer
        for who, rc, msg in _pe_both(_pe(hw=hw, **NULL_IMG), REFLECT):
            assert rc == _lib.ERR_NULL and "img[0]" in msg, (rc, msg)
        assert all(rc == 0 for _, rc, _ in _pe_both(_pe(hw=hw, B=0), REFLECT))
        # the zero-padded calls keep the floor they had: 3 x 3, through either entry point
        for who, rc, msg in _pe_both(_pe(hw=hw, **NULL_IMG), ZERO):
            assert rc == _lib.ERR_SHAPE and "need H,W >= 3" in msg, (rc, msg)
        d = _pe(hw=hw, **NULL_IMG)
        assert L.sfm_photo_error_fwd(C.byref(d), None) == _lib.ERR_SHAPE and L.sfm_photo_error_bwd(C.byref(d), None) == _lib.ERR_SHAPE


def test_photo_error_pad_rejections_come_in_the_documented_order():
    """descriptor, shape, ssim_rate, padding, the reflection's floor, the empty batch, the pointers"""
    one_row = ((16, 24), (1, 31))
    for k in (0, 1):
        call = lambda d, padding: _pe_both(d, padding)[k][1]
        assert call(_pe(n_img=0, ssim_rate=2.0, **NULL_IMG), 7) == _lib.ERR_SHAPE
        assert call(_pe(H=(1, 0), ssim_rate=2.0, B=0), REFLECT) == _lib.ERR_SHAPE             # a frame that does not exist: the shape group
        assert call(_pe(ssim_rate=2.0, **NULL_IMG), 7) == _lib.ERR_CONFIG
        assert "ssim_rate" in _pe_both(_pe(ssim_rate=2.0), 7)[k][2]                           # ssim_rate before padding
        assert "ssim_rate" in _pe_both(_pe(hw=one_row, ssim_rate=2.0), REFLECT)[k][2]         # ... and before the reflection's floor
        assert "need H,W >= 3" in _pe_both(_pe(hw=one_row, **NULL_IMG), 7)[k][2]              # any other padding: the shape group's 3 x 3
        assert call(_pe(hw=one_row, B=0), REFLECT) == _lib.ERR_SHAPE                          # the floor before the empty batch
        assert call(_pe(B=0), 7) == _lib.ERR_CONFIG                                           # an empty batch still has its settings checked
        assert call(_pe(B=0, **NULL_IMG), REFLECT) == 0                                       # ... but not its pointers
        assert call(_pe(**NULL_IMG), REFLECT) == _lib.ERR_NULL
    e = _lib.SfmPhotoErrorDesc()            # an empty shard: no pointer at all
    e.n_img, e.n_scales, e.H[0], e.W[0] = 2, 1, 2, 2
    assert [rc for _, rc, _ in _pe_both(e, REFLECT)] == [0, 0]
    assert [rc for _, rc, _ in _pe_both(e, ZERO)] == [_lib.ERR_SHAPE] * 2
    # each call ignores the other's arrays: the first complaint names an array of the call's own
    e.B, e.ssim_rate = 1, 0.5
    e.img[0] = e.tgt[0] = FAKE
    fwd, bwd = _pe_both(e, REFLECT)
    assert fwd[1] == _lib.ERR_NULL and "err[0]" in fwd[2] and bwd[1] == _lib.ERR_NULL and "g_err[0]" in bwd[2]


# ------------------------------------------------------------------------------------------------------------------------
# 3. sfm_warp_full_res_up_*
# ------------------------------------------------------------------------------------------------------------------------
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
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


WS = C.c_void_p(0x100000)      # on a 256-byte boundary, never dereferenced


def _wf_fwd(d, up):
    return L.sfm_warp_full_res_up_fwd(C.byref(d) if d is not None else None, up, None), _lib.last_error()


def _wf_bwd(d, up, ws=WS, nbytes=1 << 40):
    return L.sfm_warp_full_res_up_bwd(C.byref(d) if d is not None else None, up, ws, nbytes, None), _lib.last_error()


def _wf_query(d, up):
    return L.sfm_warp_full_res_up_bwd_workspace_bytes(C.byref(d) if d is not None else None, up)


def _wf_both(d, up):
    return (("sfm_warp_full_res_up_fwd",) + _wf_fwd(d, up), ("sfm_warp_full_res_up_bwd",) + _wf_bwd(d, up))


NULL_SRC = dict(src=None)


@pytest.mark.parametrize("up", [ALIGN, HALF])
def test_warp_full_res_up_repeats_the_existing_rejections(up):
    for who, rc, msg in _wf_both(None, up):
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
    assert _wf_query(None, up) == 0
    for bad, word in ((dict(n_src=0), "n_src"), (dict(n_src=9), "n_src"), (dict(n_scales=0), "n_scales"), (dict(n_scales=9), "n_scales"),
                      (dict(B=-1), "B="), (dict(H=2), "H="), (dict(W=2), "W="), (dict(h=(1, 0)), "scale 1"), (dict(w=(0, -3)), "scale 0"),
                      (dict(H=1 << 15, W=1 << 15), "3*H*W"), (dict(h=(1, 1 << 15), w=(1, 1 << 15)), "3*h*w"),
                      (dict(B=(1 << 31) - 1, H=3, W=3), "256-pixel blocks"),
                      (dict(B=1 << 20, n_scales=1, H=3, W=3, h=(0, 1 << 14), w=(0, 1 << 14)), "256-element blocks")):
        for who, rc, msg in _wf_both(_wf(**bad), up):
            assert rc == _lib.ERR_SHAPE and msg.startswith(who) and word in msg, (bad, rc, msg)
            with pytest.raises(TypeError):
                _lib.check(rc)
        assert _wf_query(_wf(**bad), up) == 0
    for layout in (-1, 2):
        for who, rc, msg in _wf_both(_wf(image_layout=layout), up):
            assert rc == _lib.ERR_CONFIG and msg.startswith(who) and "image_layout" in msg, (rc, msg)
        assert _wf_query(_wf(image_layout=layout), up) == 0
    for field in ("intrinsics", "src", ("disp", 0), ("warped", 1), ("pose", 1)):
        null = {field[0]: (field[1], None)} if isinstance(field, tuple) else {field: None}
        rc, msg = _wf_fwd(_wf(**null), up)
        assert rc == _lib.ERR_NULL and ("%s[%d]" % field if isinstance(field, tuple) else field) in msg and msg.startswith("sfm_warp_full_res_up_fwd")
    for field in ("intrinsics", "src", ("disp", 1), ("g_warped", 0), ("d_disp", 1), ("pose", 0), ("d_pose", 1)):
        null = {field[0]: (field[1], None)} if isinstance(field, tuple) else {field: None}
        rc, msg = _wf_bwd(_wf(**null), up)
        assert rc == _lib.ERR_NULL and ("%s[%d]" % field if isinstance(field, tuple) else field) in msg and msg.startswith("sfm_warp_full_res_up_bwd")
    d = _wf()
    need = _wf_query(d, up)
    assert need > 0
    for ws, nbytes, word in ((None, need, "needed"), (WS, need - 1, "needed"), (WS, 0, "needed"), (C.c_void_p(WS.value + 128), need, "aligned")):
        rc, msg = _wf_bwd(d, up, ws, nbytes)
        assert rc == _lib.ERR_WORKSPACE and word in msg and msg.startswith("sfm_warp_full_res_up_bwd"), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)


@pytest.mark.parametrize("up", [-1, 2, 9])
def test_an_upsample_outside_the_enum_is_a_config_error(up):
    for who, rc, msg in _wf_both(_wf(**NULL_SRC), up):
        assert rc == _lib.ERR_CONFIG and "upsample=%d" % up in msg and msg.startswith(who), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert _wf_query(_wf(), up) == 0


def test_warp_full_res_up_rejections_come_in_the_documented_order():
    """descriptor, shape, layout, upsample, the empty batch, the pointers, the workspace"""
    null = dict(src=None, disp=(0, None))
    for call in (_wf_fwd, _wf_bwd):
        assert call(_wf(n_src=0, image_layout=7, **null), 9)[0] == _lib.ERR_SHAPE
        assert call(_wf(H=2, image_layout=7, B=0), 9)[0] == _lib.ERR_SHAPE
        assert "image_layout" in call(_wf(image_layout=7, **null), 9)[1]                    # the layout before upsample
        assert call(_wf(**null), 9)[0] == _lib.ERR_CONFIG
        assert call(_wf(B=0), 9)[0] == _lib.ERR_CONFIG                                      # an empty batch still has its settings checked
        assert call(_wf(B=0, **null), HALF)[0] == 0                                         # ... but not its pointers
        assert call(_wf(**null), HALF)[0] == _lib.ERR_NULL
    assert _wf_bwd(_wf(**null), HALF, None, 0)[0] == _lib.ERR_NULL                          # the pointers before the workspace
    assert _wf_bwd(_wf(B=0), HALF, None, 0)[0] == 0                                         # an empty batch needs no workspace
    assert _wf_bwd(_wf(), 9, None, 0)[0] == _lib.ERR_CONFIG


QUERIES = [(1, 1, (3, 3), [(3, 3)]), (1, 1, (3, 3), [(1, 1)]), (32, 2, (128, 416), [(128, 416), (64, 208), (32, 104), (16, 52)]),
           (3, 2, (16, 16), [(32, 32), (16, 16)])] + [(2, n, HW, hw) for HW, hw in R.HP_SHAPES.values() for n in (1, 3)]


@pytest.mark.parametrize("B,n_src,HW,hw", QUERIES)
def test_the_workspace_is_the_existing_calls_for_both_values(B, n_src, HW, hw):
    d = _lib.SfmWarpFullResDesc()          # every pointer NULL: the query looks at none
    d.B, d.n_src, d.n_scales, d.H, d.W = B, n_src, len(hw), HW[0], HW[1]
    for s, (h, w) in enumerate(hw):
        d.h[s], d.w[s] = h, w
    want = L.sfm_warp_full_res_bwd_workspace_bytes(C.byref(d))
    assert want == AC.workspace_bytes(B, n_src, HW[0], HW[1], hw) > 0
    assert _wf_query(d, ALIGN) == want and _wf_query(d, HALF) == want


# ------------------------------------------------------------------------------------------------------------------------
# 4. the half-pixel restatement
# ------------------------------------------------------------------------------------------------------------------------
IDS = ["%dx%d-from-%dx%d" % (HW + hw) for HW, hw in R.HP_PAIRS]


def test_the_nine_pairs():
    assert len(R.HP_PAIRS) == 9 and ((13, 21), (20, 30)) in R.HP_PAIRS and ((13, 21), (1, 1)) in R.HP_PAIRS


@pytest.mark.parametrize("HW,hw", R.HP_PAIRS, ids=IDS)
def test_the_restatement_is_atens_interpolate(HW, hw):
    """float64: F.interpolate(bilinear, align_corners=False) to 1e-12 (measured: 1.8e-14; the margin is for other shapes); float32: as
    close to float64 as aten's own float32 -- within 4 x its distance plus 1e-6 of the largest value, the project's rule"""
    x = np.random.RandomState(3).uniform(0.01, 10.0, (2, 1) + hw)
    o64 = R.interpolate_aten(x, HW)
    got64 = R.upsample_hp(x, HW, F64)
    assert got64.dtype == F64 and got64.shape == (2, 1) + HW
    print("upsample_hp %s: max|numpy64 - aten64| %.3g" % (IDS[R.HP_PAIRS.index((HW, hw))], np.abs(got64 - o64).max()))
    assert np.abs(got64 - o64).max() <= 1e-12
    got32, a32 = R.upsample_hp(x, HW, F32), R.interpolate_aten(x.astype(F32), HW, torch.float32)
    assert got32.dtype == F32
    err, dev = np.abs(got32.astype(F64) - o64).max(), np.abs(a32.astype(F64) - o64).max()
    print("upsample_hp %s: max|numpy32 - aten64| %.3g, max|aten32 - aten64| %.3g" % (IDS[R.HP_PAIRS.index((HW, hw))], err, dev))
    assert err <= 4 * dev + 1e-6 * np.abs(o64).max()


def test_a_scale_of_the_full_size_is_used_as_it_is():
    x = np.random.RandomState(5).uniform(0.01, 10.0, (2, 1, 13, 21)).astype(F32)
    assert R.upsample_hp(x, (13, 21), F32) is not None and np.array_equal(R.upsample_hp(x, (13, 21), F32), x)
    assert np.array_equal(R.adjoint_hp(x, (13, 21), F32), x)


@pytest.mark.parametrize("HW,hw", R.HP_PAIRS, ids=IDS)
def test_the_restated_adjoint_is_the_adjoint(HW, hw):
    """<R x, y> = <x, R^T y> in float64 to its rounding, R^T against aten's float64 autograd to 1e-12, and the float32 statement
    within the roundings of its own sums of the float64 one"""
    rng = np.random.RandomState(4)
    x, y = rng.standard_normal((2, 1) + hw), rng.standard_normal((2, 1) + HW)
    rx, rty = R.upsample_hp(x, HW, F64), R.adjoint_hp(y, hw, F64)
    lhs, rhs = float((rx * y).sum()), float((x * rty).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(np.abs(rx * y).sum()), (lhs, rhs)
    assert rty.shape == x.shape and np.abs(rty - R.adjoint64_aten_hp(y, hw)).max() <= 1e-12 * max(1.0, float(np.abs(rty).max()))
    assert float(rty.sum()) == pytest.approx(float(y.sum()), rel=1e-12, abs=1e-9)      # the weights of one output add up to 1
    r32 = R.adjoint_hp(y, hw, F32)
    terms = R.adjoint_hp(np.abs(y), hw, F64)                                          # the sum of |contributions| per element
    # per contribution: the weights' position error (the float32 coordinate: three roundings at the size of the axis), the product
    # and the running sum
    n_terms = (-(-HW[0] // hw[0]) + 1) * (-(-HW[1] // hw[1]) + 1) * 4 + 4
    bound = terms * (2 * 3 * float(np.spacing(F32(max(hw)))) + (n_terms + 3) * 2.0 ** -24) + 1e-30
    assert r32.dtype == F32 and (np.abs(r32.astype(F64) - rty) <= bound).all()


def test_the_float32_coordinate_never_decreases():
    """what the first-index search of resize_hp_first_at rests on, for every axis of every shape used on the GPU; and the taps stay
    inside the input"""
    axes = {(n, on) for HW, hw in R.HP_PAIRS for n, on in zip(hw, HW)} | {(16, 128), (52, 416), (32, 128), (104, 416), (64, 128), (208, 416)}
    for n, on in sorted(axes):
        u = R.coords_hp(n, on, F32)
        assert u.dtype == F32 and (np.diff(u) >= 0).all() and u[0] >= 0, (n, on)
        t0, t1, w0, w1 = R.axis_taps_hp(n, on, F32)
        assert (np.diff(t0) >= 0).all() and t0.min() >= 0 and t1.max() <= n - 1 and (t1 - t0 <= 1).all(), (n, on)
        assert w1.min() >= 0 and w1.max() <= 1, (n, on)


def test_a_downsampled_scale_leaves_elements_at_exactly_zero():
    """an element that no output's taps reach receives exactly 0.  That takes a ratio above 2 -- two taps per output, one input apart:
    at 20x30 -> 13x21, the downsampled scale of the GPU cases, every element is still reached; at 20x30 -> 9x7, the extra GPU case, not"""
    assert (R.adjoint_hp(np.ones((1, 1, 13, 21), F32), (20, 30), F32) > 0).all()
    (HW, sizes), = [R.HP_EXTRA["9x7"]]
    hw = sizes[1]
    assert hw == (20, 30)
    g = np.random.RandomState(6).uniform(0.5, 1.5, (2, 1) + HW).astype(F32)       # positive: an element that is touched cannot cancel
    d = R.adjoint_hp(g, hw, F32)
    assert d.shape == (2, 1) + hw
    untouched = d[0, 0] == 0
    assert 0 < untouched.sum() < untouched.size and np.array_equal(untouched, d[1, 0] == 0)
    v0, v1, _, _ = R.axis_taps_hp(hw[0], HW[0], F32)
    u0, u1, _, _ = R.axis_taps_hp(hw[1], HW[1], F32)
    rows, cols = np.zeros(hw[0], bool), np.zeros(hw[1], bool)
    rows[v0] = rows[v1] = cols[u0] = cols[u1] = True
    # (a tap whose weight is exactly 0 touches its element with a contribution of +0)
    assert not (untouched & np.outer(rows, cols) & (R.adjoint_hp(np.ones_like(g), hw, F64)[0, 0] != 0)).any()
    assert untouched[~np.outer(rows, cols)].all()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the reflection reference
# ------------------------------------------------------------------------------------------------------------------------
def test_the_reflected_window_is_reflection_pad_then_avg_pool():
    """the definition, literally: torch.nn.ReflectionPad2d(1) + AvgPool2d(3, 1); row -1 is row 1, row H is row H-2"""
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float64).reshape(2, 3, 4, 5) ** 1.5
    want = torch.nn.AvgPool2d(3, 1)(torch.nn.ReflectionPad2d(1)(x))
    assert torch.equal(R._pool_t(x, "reflect"), want)
    assert np.abs(R._pool_np(x.numpy(), "reflect") - want.numpy()).max() <= 1e-12 * float(want.max())
    p = torch.nn.ReflectionPad2d(1)(x)
    assert torch.equal(p[:, :, 0, 1:-1], x[:, :, 1]) and torch.equal(p[:, :, -1, 1:-1], x[:, :, -2]) and torch.equal(p[:, :, 1:-1, 0], x[:, :, :, 1])
    assert p[0, 0, 0, 0] == x[0, 0, 1, 1] and p[0, 0, -1, -1] == x[0, 0, -2, -2]


@pytest.mark.parametrize("hw", [(2, 2), (2, 3), (3, 2), (3, 3), (5, 7)], ids=lambda hw: "%dx%d" % hw)
def test_the_ring_fold_is_the_adjoint_of_pad_then_pool(hw):
    """float64: `fold` -- the neighbour counted once more at columns 1 and W-2, the neighbouring row's sums once more at rows 1 and
    H-2 -- equals autograd of sum(k * pool(pad(m))) with respect to m, and the whole backward built on it equals autograd of the padded
    formula"""
    rng = np.random.RandomState(8)
    k = rng.standard_normal((2, 3) + hw)
    m = torch.zeros((2, 3) + hw, dtype=torch.float64, requires_grad=True)
    (R._pool_t(m, "reflect") * torch.from_numpy(k)).sum().backward()
    assert np.abs(R.fold(k) / 9 - m.grad.numpy()).max() <= 4e-16 * np.abs(k).max() * 9
    assert R.fold(np.ones(hw)).sum() == 9 * hw[0] * hw[1]                             # every window holds nine real values
    Y = rng.uniform(-1, 1, (2, 3) + hw)
    X = np.roll(Y, 1, axis=3)[:, None] + 0.3 * rng.standard_normal((2, 2, 3) + hw)
    g = rng.standard_normal((2, 2) + hw)
    for alpha in (0.85, 1.0):
        _, want = R.photo_error(X, Y, alpha, g, np.float64)
        got = R.emulate_reflect(X, Y, alpha, g)
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (alpha, np.abs(got - want).max())


def test_the_knife_windows_are_the_windows_that_read_an_entry():
    near = (np.random.RandomState(9).uniform(size=(2, 3, 7, 9)) < 0.05).astype(F64)
    assert np.array_equal(R._pool_np(near, "reflect") > 0, R.fold(near) > 0)


@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("name", sorted(R.REFLECT_CASES))
def test_the_cases_are_fit_to_judge(name, alpha):
    """from the references alone: the entries that leave the backward comparison are at most 1 % of an array, none in the tiny shapes;
    and the zero-padded float64 reference FAILS the rule of tests/test_conventions_gpu.py against the reflected one, forward and
    backward, wherever the SSIM term takes part -- the test can tell the two apart.  Without it (alpha = 0) the two agree exactly."""
    X, Y, G = R.reflect_inputs(name)
    assert len(X) <= _lib.SFM_MAX_SCALES and X[0].shape[1] <= _lib.SFM_MAX_SRC == R.MAX_SRC
    ref, zero = R.reflect_reference(name, alpha), R.reflect_reference(name, alpha, "zero")
    for s, ((e64, d64, e32, d32), (z64, zd64, _, _)) in enumerate(zip(ref, zero)):
        knife = R.knife(X[s], Y[s], alpha)
        assert knife.shape == d64.shape
        assert knife.mean() <= 0.01, "%s scale %d: %.3g of the entries are knife-edge" % (name, s, knife.mean())
        if name == "tiny":
            assert not knife.any()
        for what, o64, o32, z, keep in (("fwd", e64, e32, z64, np.ones(e64.shape, bool)), ("bwd", d64, d32, zd64, ~knife)):
            allowed = 4 * float((np.abs(o32.astype(F64) - o64) * keep).max()) + 1e-6 * float(np.abs(o64).max())
            off = float((np.abs(z - o64) * keep).max())
            if alpha == 0:
                assert off == 0
            else:
                assert off > allowed, "%s scale %d %s: zero padding is off by %.3g, the rule allows %.3g" % (name, s, what, off, allowed)
        if alpha > 0:      # the two differ on the border ring and nowhere else (forward)
            inner = np.abs(z64 - e64)[..., 1:-1, 1:-1]
            assert inner.size == 0 or inner.max() <= 1e-12
