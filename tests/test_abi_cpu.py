"""The C-ABI library loads on a host without a GPU and exports every symbol include/sfmwarp.h
declares; argument validation (which happens before any HIP call) follows the error convention."""
import ctypes as C
import importlib
import re

import pytest

import abi_header

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
DESCRIPTORS = {"SfmLossDesc": _lib.SfmLossDesc, "SfmWarpPyramidDesc": _lib.SfmWarpPyramidDesc, "SfmPhotoErrorDesc": _lib.SfmPhotoErrorDesc}


def test_header_and_binding_declare_the_same_symbols():
    assert abi_header.declared() == sorted(_lib.SYMBOLS) == sorted(abi_header.prototypes())


def test_library_exports_every_declared_symbol():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in abi_header.declared():
        assert hasattr(raw, name), name
    assert raw.sfm_abi_version() == _lib.SFM_ABI_VERSION


def test_the_abi_version_and_every_descriptor_layout_match_the_header():
    """One header, one version: an entry point added to it leaves the older declarations as they were exactly when the version and
    the three descriptors still are what the binding says (the descriptor BYTES are pinned by tests/golden/host_plans.npz)."""
    assert re.findall(r"#define SFM_ABI_VERSION (\d+)", abi_header.TEXT) == ["6"] and _lib.SFM_ABI_VERSION == 6
    assert sorted(re.findall(r"typedef struct (\w+)", abi_header.TEXT)) == sorted(DESCRIPTORS)
    for name, struct in DESCRIPTORS.items():
        abi_header.assert_layout(struct, name)


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)


def test_every_binding_has_the_parameters_of_its_prototype():
    """per symbol: as many argtypes as the prototype has parameters, and a pointer type wherever the header has a pointer"""
    for name, (res, args) in _lib.SYMBOLS.items():
        params = abi_header.parameters(name)
        assert len(args) == len(params), (name, params)
        for k, (t, param) in enumerate(zip(args, params)):
            assert _is_pointer(t) == ("*" in param), (name, k, param, t)
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == args and fn.restype == res, name


def test_descriptor_layout_matches_the_header():
    # 4 + 8 + 8 int32, 3 float, 1 int32, then 4*8 + 1 + 8 + 8 + 8 + 8 + 8 pointers, then image_layout (int32, padded to 8),
    # then the 8 pointers of `warped` (ABI v4), then projection (int32, padded to 8; ABI v5)
    assert C.sizeof(_lib.SfmLossDesc) == 4 * (4 + 8 + 8 + 3 + 1) + 8 * (8 * 4 + 1 + 8 + 8 * 3 + 8) + 8 + 8 * 8 + 8
    assert _lib.SfmLossDesc.tgt.offset % 8 == 0
    assert _lib.SfmLossDesc.image_layout.offset == C.sizeof(_lib.SfmLossDesc) - 8 - 8 * 8 - 8
    assert _lib.SfmLossDesc.warped.offset == C.sizeof(_lib.SfmLossDesc) - 8 * 8 - 8
    assert _lib.SfmLossDesc.projection.offset == C.sizeof(_lib.SfmLossDesc) - 8


def test_projection_field_is_validated_without_a_gpu():
    """SfmLossDesc.projection (ABI v5): FAST and REFERENCE_ORDER size the same workspace, with and without d_src (since the d_src of
    round 6's two launches both projections produce it); any other value is SFM_ERR_CONFIG from every entry point."""
    d = _desc(ssim_rate=0.15, smooth_reg=0.1, smooth_mode=_lib.SMOOTH_SECOND_ORDER)
    n = _lib.lib.sfm_loss_workspace_bytes(C.byref(d))
    d.projection = _lib.SFM_PROJECTION_REFERENCE_ORDER
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) == n > 0
    d.d_src[0] = d.d_src[1] = 0x1000
    with_d_src = _lib.lib.sfm_loss_workspace_bytes(C.byref(d))
    d.projection = _lib.SFM_PROJECTION_FAST
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) == with_d_src > n
    d = _desc(projection=2)
    assert _lib.lib.sfm_loss_fwd(C.byref(d), None, None, 0, None) == _lib.ERR_CONFIG and "projection" in _lib.last_error()


def _desc(**kw):
    d = _lib.SfmLossDesc()
    d.B, d.norm_B, d.n_src, d.n_scales = 2, 2, 2, 2
    d.H[0], d.W[0], d.H[1], d.W[1] = 16, 24, 8, 12
    fake = 0x1000   # never dereferenced: validation fails / sizing only
    for s in range(2):
        d.tgt[s] = d.src[s] = d.disp[s] = fake
    d.pose[0] = d.pose[1] = fake
    d.intrinsics = fake
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_workspace_query_needs_no_gpu():
    d = _desc(ssim_rate=0.15, smooth_reg=0.1, smooth_mode=_lib.SMOOTH_SECOND_ORDER)
    n = _lib.lib.sfm_loss_workspace_bytes(C.byref(d))
    assert n > 0 and n % 256 == 0
    assert _lib.lib.sfm_warp_bwd_workspace_bytes(2, 16, 24) == 2 * ((16 * 24 + 255) // 256) * 12 * 4
    assert _lib.lib.sfm_warp_bwd_workspace_bytes(0, 16, 24) == 0


def test_workspace_with_d_src_holds_the_record_of_the_image_gradient():
    """With SfmLossDesc.d_src bound the main launch records dL/dI^ of every warped pixel in the workspace (B x 3 n_src x h x w floats
    per scale that binds it) for the second launch, dsrc_scatter_kernel: the query grows by exactly that, per bound scale."""
    d = _desc(ssim_rate=0.15, smooth_reg=0.1, smooth_mode=_lib.SMOOTH_SECOND_ORDER)
    base = _lib.lib.sfm_loss_workspace_bytes(C.byref(d))
    rec = lambda s: -(-d.B * 3 * d.n_src * d.H[s] * d.W[s] * 4 // 256) * 256      # rounded up to the 256-byte alignment of a workspace array
    d.d_src[0] = 0x1000
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) == base + rec(0)
    d.d_src[1] = 0x1000
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) == base + rec(0) + rec(1)
    d.d_src[0] = None
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) == base + rec(1)


@pytest.mark.parametrize("bad,code", [
    (dict(n_src=0), _lib.ERR_SHAPE), (dict(n_src=9), _lib.ERR_SHAPE), (dict(n_scales=0), _lib.ERR_SHAPE),
    (dict(norm_B=1), _lib.ERR_CONFIG), (dict(ssim_rate=1.5), _lib.ERR_CONFIG), (dict(smooth_mode=7), _lib.ERR_CONFIG), (dict(image_layout=5), _lib.ERR_CONFIG),
    (dict(intrinsics=None), _lib.ERR_NULL), (dict(exp_reg=0.2), _lib.ERR_NULL),   # exp_reg without mask logits
])
def test_bad_descriptors_are_rejected_with_a_message(bad, code):
    d = _desc(**bad)
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) == 0
    rc = _lib.lib.sfm_loss_fwd(C.byref(d), None, None, 0, None)
    assert rc == code
    assert _lib.last_error()
    with pytest.raises((TypeError, ValueError)):
        _lib.check(rc)


def test_tiny_scale_is_rejected():
    d = _desc()
    d.H[1], d.W[1] = 2, 12
    assert _lib.lib.sfm_loss_fwd(C.byref(d), None, None, 0, None) == _lib.ERR_SHAPE


def test_hwc_layout_rejects_images_whose_byte_offsets_leave_fp32():
    """SFM_LAYOUT_HWC forms the byte offset of a gather inside one image exactly in fp32: an image of a scale must have fewer than
    2^24 / 12 pixels; the planar layout takes the same shape."""
    d = _desc(n_scales=1, image_layout=_lib.SFM_LAYOUT_HWC)
    d.B = d.norm_B = 1
    d.H[0], d.W[0] = 1200, 1200            # 1.44 M pixels > 1,398,101
    assert _lib.lib.sfm_loss_fwd(C.byref(d), None, None, 0, None) == _lib.ERR_SHAPE and "2^24" in _lib.last_error()
    d.image_layout = _lib.SFM_LAYOUT_PLANAR
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) > 0
    d.image_layout = _lib.SFM_LAYOUT_HWC
    d.H[0], d.W[0] = 1000, 1398            # just below the limit
    assert _lib.lib.sfm_loss_workspace_bytes(C.byref(d)) > 0


def test_missing_workspace_is_reported_before_any_launch():
    d = _desc()
    buf = (C.c_float * 5)()
    rc = _lib.lib.sfm_loss_fwd(C.byref(d), C.cast(buf, C.c_void_p), None, 0, None)
    assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()


def _call(entry, d, loss5, ws, ws_bytes):
    L = _lib.lib
    fake = C.c_void_p(0x1000)
    if entry == "sfm_loss_bwd":
        return L.sfm_loss_bwd(C.byref(d), 1.0, ws, ws_bytes, None)
    if entry.startswith("sfm_step"):
        return getattr(L, entry)(fake, fake, C.byref(d), loss5, ws, ws_bytes, None)
    return getattr(L, entry)(C.byref(d), loss5, ws, ws_bytes, None)


@pytest.mark.parametrize("entry", ["sfm_loss_fwd", "sfm_loss_bwd", "sfm_loss_fwd_bwd", "sfm_step_fwd", "sfm_step_fwd_bwd"])
def test_short_or_misaligned_workspace_is_rejected_before_any_launch(entry):
    """include/sfmwarp.h: `ws` holds at least sfm_loss_workspace_bytes(desc) bytes and starts on a 256-byte boundary.  One byte
    short, or 4 / 128 bytes off the boundary: SFM_ERR_WORKSPACE with a message, from every entry point, before anything is launched
    (no device here: a launch would fail with a positive code instead).  sfm_step_* reject before they write the pyramids, too."""
    d = _desc(ssim_rate=0.15, smooth_reg=0.1, smooth_mode=_lib.SMOOTH_SECOND_ORDER, image_layout=_lib.SFM_LAYOUT_HWC)
    for s in range(2):
        d.d_disp[s] = 0x1000
    d.d_pose[0] = d.d_pose[1] = 0x1000
    n = _lib.lib.sfm_loss_workspace_bytes(C.byref(d))
    assert n > 0 and n % 256 == 0
    buf = (C.c_float * 5)()
    loss5 = C.cast(buf, C.c_void_p)
    for ws, ws_bytes, word in ((0x10000, n - 1, "needed"), (0x10004, n, "aligned"), (0x10080, n, "aligned"), (0x10004, n + 4096, "aligned"),
                               (None, n, "needed")):
        rc = _call(entry, d, loss5, C.c_void_p(ws) if ws else None, ws_bytes)
        assert rc == _lib.ERR_WORKSPACE, (entry, ws, ws_bytes, rc, _lib.last_error())
        assert "workspace" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
        with pytest.raises(ValueError):
            _lib.check(rc)


def test_warp_bwd_workspace_one_byte_short_is_rejected():
    fake = C.c_void_p(0x1000)
    n = _lib.lib.sfm_warp_bwd_workspace_bytes(2, 16, 24)
    rc = _lib.lib.sfm_warp_bwd(fake, fake, 1, fake, fake, fake, fake, fake, None, fake, n - 1, 2, 3, 16, 24, None)
    assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    assert _lib.lib.sfm_warp_bwd(fake, fake, 1, fake, fake, fake, fake, fake, None, None, n, 2, 3, 16, 24, None) == _lib.ERR_WORKSPACE


def test_operator_argument_errors_need_no_gpu():
    L = _lib.lib
    assert L.sfm_warp_fwd(None, None, 1, None, None, None, 1, 3, 8, 8, None) == _lib.ERR_NULL
    fake = C.c_void_p(0x1000)
    assert L.sfm_warp_fwd(fake, fake, 1, fake, fake, fake, 1, 3, 2, 8, None) == _lib.ERR_SHAPE     # H < 3
    assert L.sfm_warp_fwd(fake, fake, 2, fake, fake, fake, 1, 3, 8, 8, None) == _lib.ERR_SHAPE     # depth_rows
    assert L.sfm_warp_fwd(None, None, 1, None, None, None, 0, 3, 8, 8, None) == 0                  # empty batch
    assert L.sfm_sampler_interp_fwd(fake, fake, fake, 1, 0, 8, 8, 8, 8, None) == _lib.ERR_SHAPE    # C = 0
