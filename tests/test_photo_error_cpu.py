"""The photometric error maps (include/sfmwarp.h) without a GPU: header, binding and library declare the same two entry
points and the same descriptor, every documented rejection answers with its code and a message, in the documented order and before
any HIP call (the pointers are fakes that are never dereferenced), the type errors of torch_api.photometric_error and
ops.photo_error_*, and the formulas of the header restated in NumPy and checked against the oracle."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import abi_header
from oracle import sfm_oracle as O

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
FAKE = 0x10000                 # never dereferenced
ENTRY_POINTS = ["sfm_photo_error_bwd", "sfm_photo_error_fwd"]


# ------------------------------------------------------------------------------------------------------------------------
# header and binding
# ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_declare_the_same_symbols():
    pick = lambda names: sorted(n for n in names if n.startswith("sfm_photo_error"))
    assert pick(abi_header.declared()) == pick(_lib.SYMBOLS) == ENTRY_POINTS
    for name in ENTRY_POINTS:
        res, args = _lib.SYMBOLS[name]
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        assert args == [C.POINTER(_lib.SfmPhotoErrorDesc), C.c_void_p] and res is C.c_int


def test_descriptor_matches_the_header():
    abi_header.assert_layout(_lib.SfmPhotoErrorDesc, "SfmPhotoErrorDesc")
    assert [f[0] for f in abi_header.struct_fields("SfmPhotoErrorDesc")] == ["B", "n_img", "n_scales", "H", "W", "ssim_rate", "img", "tgt", "err",
                                                                            "g_err", "d_img"]
    assert dict(_lib.SfmPhotoErrorDesc._fields_)["ssim_rate"] is C.c_float


# ------------------------------------------------------------------------------------------------------------------------
# reject paths: what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _desc(B=2, n_img=2, n_scales=2, hw=((16, 24), (9, 31)), ssim_rate=0.85, **kw):
    d = _lib.SfmPhotoErrorDesc()
    d.B, d.n_img, d.n_scales, d.ssim_rate = B, n_img, n_scales, ssim_rate
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
    for s in range(max(0, min(n_scales, _lib.SFM_MAX_SCALES))):
        d.img[s] = d.tgt[s] = d.err[s] = d.g_err[s] = d.d_img[s] = FAKE
    for k, v in kw.items():
        getattr(d, k)[v[0]] = v[1]
    return d


def _fwd(d):
    return L.sfm_photo_error_fwd(C.byref(d) if d is not None else None, None), _lib.last_error()


def _bwd(d):
    return L.sfm_photo_error_bwd(C.byref(d) if d is not None else None, None), _lib.last_error()


def _both(d):
    return (("sfm_photo_error_fwd",) + _fwd(d), ("sfm_photo_error_bwd",) + _bwd(d))


def test_null_descriptor():
    for who, rc, msg in _both(None):
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)


BAD_SHAPES = [dict(n_img=0), dict(n_img=9), dict(n_scales=0), dict(n_scales=9), dict(B=-1), dict(H=(1, 2)), dict(W=(0, 2)),
              dict(H=(0, 0)), dict(H=(0, 1 << 15), W=(0, 1 << 15))]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=[str(sorted(b.items())) for b in BAD_SHAPES])
def test_bad_shapes(bad):
    for who, rc, msg in _both(_desc(**bad)):
        assert rc == _lib.ERR_SHAPE and msg.startswith(who), (rc, msg)
        with pytest.raises(TypeError):
            _lib.check(rc)


def test_too_many_tiles():
    d = _desc(B=1 << 30, n_img=8, n_scales=1, hw=((16, 24),))
    for who, rc, msg in _both(d):
        assert rc == _lib.ERR_SHAPE and "tiles" in msg and msg.startswith(who), (rc, msg)


@pytest.mark.parametrize("rate", [-0.01, 1.01, float("nan"), float("inf"), -float("inf")])
def test_bad_ssim_rate(rate):
    for who, rc, msg in _both(_desc(ssim_rate=rate)):
        assert rc == _lib.ERR_CONFIG and "ssim_rate" in msg and msg.startswith(who), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)


@pytest.mark.parametrize("rate", [0.0, 0.85, 1.0])
def test_the_ends_of_the_ssim_rate_range_are_taken(rate):
    d = _desc(B=0, ssim_rate=rate)
    assert _fwd(d)[0] == 0 and _bwd(d)[0] == 0


BOTH = [("img", 1), ("tgt", 0)]
FWD_ONLY = [("err", 1)]
BWD_ONLY = [("g_err", 0), ("d_img", 1)]


@pytest.mark.parametrize("field", BOTH + FWD_ONLY, ids=str)
def test_forward_null_pointers(field):
    rc, msg = _fwd(_desc(**{field[0]: (field[1], None)}))
    assert rc == _lib.ERR_NULL and "%s[%d]" % field in msg and msg.startswith("sfm_photo_error_fwd"), (rc, msg)


@pytest.mark.parametrize("field", BOTH + BWD_ONLY, ids=str)
def test_backward_null_pointers(field):
    rc, msg = _bwd(_desc(**{field[0]: (field[1], None)}))
    assert rc == _lib.ERR_NULL and "%s[%d]" % field in msg and msg.startswith("sfm_photo_error_bwd"), (rc, msg)


def test_rejections_come_in_the_documented_order():
    """shape before ssim_rate before the empty batch before the pointers"""
    null_img = dict(img=(0, None))
    for call in (_fwd, _bwd):
        assert call(_desc(n_img=0, ssim_rate=2.0, **null_img))[0] == _lib.ERR_SHAPE
        assert call(_desc(H=(1, 2), ssim_rate=2.0, B=0))[0] == _lib.ERR_SHAPE
        assert call(_desc(ssim_rate=2.0, **null_img))[0] == _lib.ERR_CONFIG
        assert call(_desc(B=0, ssim_rate=2.0))[0] == _lib.ERR_CONFIG          # an empty batch still has its settings checked
        assert call(_desc(B=0, **null_img))[0] == 0                         # ... but not its pointers
        assert call(_desc(**null_img))[0] == _lib.ERR_NULL
    # each call ignores the other's arrays: with them NULL it gets as far as ... a launch, which is not made here; so the check is
    # that the FIRST complaint of a descriptor with everything NULL names an array of the call's own
    d = _desc(B=0)
    e = _lib.SfmPhotoErrorDesc()
    e.B, e.n_img, e.n_scales, e.H[0], e.W[0], e.ssim_rate = 1, 1, 1, 5, 7, 0.5
    e.img[0] = e.tgt[0] = FAKE
    assert _fwd(e)[0] == _lib.ERR_NULL and "err[0]" in _lib.last_error()
    assert _bwd(e)[0] == _lib.ERR_NULL and "g_err[0]" in _lib.last_error()
    e.g_err[0] = FAKE
    assert _bwd(e)[0] == _lib.ERR_NULL and "d_img[0]" in _lib.last_error()
    assert _fwd(d)[0] == 0


def test_empty_batch_launches_nothing():
    e = _lib.SfmPhotoErrorDesc()            # an empty shard: no pointer at all, the shape still checked
    e.n_img, e.n_scales, e.H[0], e.W[0] = 2, 1, 16, 24
    assert _fwd(e)[0] == 0 and _bwd(e)[0] == 0
    e.H[0] = 2
    assert _fwd(e)[0] == _lib.ERR_SHAPE and _bwd(e)[0] == _lib.ERR_SHAPE


# ------------------------------------------------------------------------------------------------------------------------
# torch_api.photometric_error and ops.photo_error_*: what they refuse before anything reaches the library
# ------------------------------------------------------------------------------------------------------------------------
def test_type_errors():
    assert "photometric_error" in ta.__all__ and {"photo_error_fwd", "photo_error_bwd"} <= set(ops.__all__)
    B, n, H, W = 2, 2, 16, 24
    imgs = [torch.zeros(B, n, 3, H, W), torch.zeros(B, n, 3, H // 2, W // 2)]
    tgt = torch.zeros(B, 3, H, W)
    tgts = [tgt, torch.zeros(B, 3, H // 2, W // 2)]
    for args in ((imgs, tgt),                                          # CPU tensors: there is no CPU path
                 (imgs, tgts),
                 ([imgs[0][:, 0], imgs[1]], tgts),                     # wrong rank
                 ([imgs[0][:, :, :2], imgs[1][:, :, :2]], tgts),       # two channels
                 (imgs, tgts[:1]),                                     # one target scale for two image scales
                 (imgs[::-1], tgt),                                    # h_s != H >> s
                 ([imgs[0], imgs[0]], tgt),
                 (imgs[0], tgt),                                       # not a list
                 ([], []),
                 ([t.numpy() for t in imgs], tgts)):
        with pytest.raises(TypeError):
            ta.photometric_error(*args, ssim_rate=0.85)
    g = [torch.zeros(B, n, H, W), torch.zeros(B, n, H // 2, W // 2)]
    for args in ((imgs, tgts), ([imgs[0][:, 0], imgs[1]], tgts), ([imgs[0][:, :, :2], imgs[1]], tgts), (imgs, tgts[:1]),
                 (imgs, [tgts[0], tgts[0]]), (imgs[0], tgts[0])):
        with pytest.raises(TypeError):
            ops.photo_error_fwd(*args, 0.85)
        with pytest.raises(TypeError):
            ops.photo_error_bwd(*args, 0.85, g)


@pytest.mark.parametrize("case", ["rank", "channels", "scales", "halving", "list"])
def test_shape_errors_are_found_by_the_shape_checks(case, monkeypatch):
    """The same refusals with the device test out of the way (CPU tensors stand in for device tensors; nothing is launched: every
    case fails before the library is reached), so that it is the shape check that speaks."""
    def dev(t, name, ndim=None, dtypes=ops.FLOAT32):
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or (ndim is not None and t.dim() != ndim):
            raise TypeError("%s: rank or dtype" % name)
        return t.contiguous()

    monkeypatch.setattr(ops, "_dev", dev)
    monkeypatch.setattr(ops, "_launch", lambda *a: pytest.fail("reached the library"))
    B, n, H, W = 2, 2, 16, 24
    imgs = [torch.zeros(B, n, 3, H, W), torch.zeros(B, n, 3, H // 2, W // 2)]
    tgt = torch.zeros(B, 3, H, W)
    tgts = [tgt, torch.zeros(B, 3, H // 2, W // 2)]
    args, word = {"rank": (([imgs[0][:, 0], imgs[1]], tgts), "rank"),
                  "channels": (([t[:, :, :2] for t in imgs], tgts), r"\(B,n,3,h,w\)"),
                  "scales": ((imgs, tgts[:1]), "2 scales but tgt has 1"),
                  "halving": ((imgs[::-1], tgt), "H>>0"),
                  "list": ((imgs[0], tgt), "list")}[case]
    with pytest.raises(TypeError, match=word):
        ta.photometric_error(*args, ssim_rate=0.85)
    with pytest.raises(TypeError):                                       # ... and a float64 image is a dtype error
        ta.photometric_error([t.double() for t in imgs], tgts, ssim_rate=0.85)


# ------------------------------------------------------------------------------------------------------------------------
# the formulas of the header, restated: pooled partials and the L1 sign term
# ------------------------------------------------------------------------------------------------------------------------
def _pool(a):
    """zero-padded 3x3 sum / 9 of the last two axes"""
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)])
    h, w = a.shape[-2:]
    return sum(p[..., i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0


def emulate(X, Y, alpha, g=None):
    """err (B,n,h,w) and, with g, d_img (B,n,3,h,w) of include/sfmwarp.h in fp64: X (B,n,3,h,w), Y (B,3,h,w)"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)[:, None]
    c1, c2 = 1e-4, 9e-4
    mx, my = _pool(X), _pool(Y)
    exx, eyy, exy = _pool(X * X), _pool(Y * Y), _pool(X * Y)
    n1, n2 = 2 * mx * my + c1, 2 * (exy - mx * my) + c2
    d1, d2 = mx * mx + my * my + c1, (exx - mx * mx) + (eyy - my * my) + c2
    S = n1 * n2 / (d1 * d2)
    e = (1 - S) / 2
    err = (1 - alpha) * np.abs(X - Y).sum(2) / 3 + alpha * np.clip(e, 0, 1).sum(2) / 3
    if g is None:
        return err
    g = np.asarray(g, np.float64)[:, :, None]
    kappa = alpha / 3 * g * -0.5 * ((e > 0) & (e < 1))
    # S(mu_x, E[xx], E[xy]) with sigma_x = E[xx] - mu_x^2 and sigma_xy = E[xy] - mu_x mu_y: the chain rule term by term
    dS_dn1, dS_dn2, dS_dd1, dS_dd2 = n2 / (d1 * d2), n1 / (d1 * d2), -S / d1, -S / d2
    dS_dmx = dS_dn1 * 2 * my + dS_dn2 * (-2 * my) + dS_dd1 * 2 * mx + dS_dd2 * (-2 * mx)
    dS_dexx, dS_dexy = dS_dd2, dS_dn2 * 2
    d = (1 - alpha) / 3 * g * np.sign(X - Y) + _pool(kappa * dS_dmx) + 2 * X * _pool(kappa * dS_dexx) + Y * _pool(kappa * dS_dexy)
    return err, d


def oracle(X, Y, alpha, g=None, dtype=np.float64):
    """The same from oracle.compute_ssim / compute_ssim_backward (per image: the oracle takes (N,C,h,w)) plus the L1 terms"""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    B, n = X.shape[:2]
    alpha, third = dtype(alpha), dtype(1) / dtype(3)
    err, d = np.zeros(X.shape[:2] + X.shape[3:], dtype), np.zeros(X.shape, dtype)
    for i in range(n):
        diff = X[:, i] - Y
        err[:, i] = (1 - alpha) * (np.abs(diff).sum(1) * third)
        if alpha > 0:
            err[:, i] += alpha * (O.compute_ssim(X[:, i], Y, dtype).sum(1) * third)
        if g is not None:
            gi = np.asarray(g, dtype)[:, i, None]
            d[:, i] = (1 - alpha) * third * gi * np.sign(diff)
            if alpha > 0:
                d[:, i] += O.compute_ssim_backward(X[:, i], Y, np.broadcast_to(alpha * third * gi, diff.shape), dtype)
    return (err, d) if g is not None else err


@pytest.mark.parametrize("alpha", [0.0, 0.85, 1.0])
def test_the_formulas_of_the_header_are_the_oracles(alpha):
    rng = np.random.default_rng(5)
    B, n, h, w = 2, 2, 5, 7
    Y = rng.uniform(-1, 1, (B, 3, h, w))
    X = np.roll(Y, 2, axis=3)[:, None] + 0.3 * rng.standard_normal((B, n, 3, h, w))
    X[0, 0, :, 1, 2] = Y[0, :, 1, 2]                      # sign(0) = 0
    g = rng.standard_normal((B, n, h, w))
    err, d = emulate(X, Y, alpha, g)
    want_err, want_d = oracle(X, Y, alpha, g)
    np.testing.assert_allclose(err, want_err, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(d, want_d, rtol=1e-10, atol=1e-12)
    assert err.min() >= 0 and err.max() > 0.1
    if alpha == 0:
        assert (d[0, 0, :, 1, 2] == 0).all()
        np.testing.assert_allclose(d, g[:, :, None] * np.sign(X - Y[:, None]) / 3, rtol=1e-15, atol=0)
    # and the gradient is the gradient: central differences of the emulation itself
    V = rng.standard_normal(X.shape)
    eps = 1e-6
    fd = ((emulate(X + eps * V, Y, alpha) - emulate(X - eps * V, Y, alpha)) * g).sum() / (2 * eps)
    assert abs(fd - (d * V).sum()) <= 1e-5 * max(1.0, abs(fd))
