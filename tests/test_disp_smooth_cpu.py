"""sfm_disp_smooth_* (include/sfmwarp_disp_smooth.h) without a GPU: the side header, the binding and the library declare the same
three entry points and the same descriptor; every documented rejection answers with its code and a message, in the documented order
and before any HIP call (the pointers are fakes that are never dereferenced); the workspace query; the NumPy restatement
(tests/disp_smooth_ref.py) on hand-made cases whose answers are written out here, and against the float64 statements -- the term
as written in aten, and oracle.compute_disp_smooth / _backward -- by the rule of tests/test_photo_error_gpu.py with the restatement
in the place of the GPU:  max|ref - o64| <= 4 max|o32 - o64| + 1e-6 max|o64|,  o32 the same statement in float32.  (A float32
emulation of the factored arithmetic on a CPU gave a loss within 2.6e-8 relative and a gradient within 9e-8 of its maximum at every
shape up to 128x416.)"""
import ctypes as C
import functools
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import disp_smooth_ref as R
from oracle import sfm_oracle as oracle

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmwarp_disp_smooth.h")
KERNELS = os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", "sfm_disp_smooth.hip")
FAKE = 0x10000                 # never dereferenced
ENTRY_POINTS = ["sfm_disp_smooth_bwd", "sfm_disp_smooth_fwd", "sfm_disp_smooth_workspace_bytes"]
CONSTANTS = {"SFM_MAX_SCALES": _lib.SFM_MAX_SCALES}
F32, F64 = np.float32, np.float64
EDGES = {"mean_abs": R.EDGE_MEAN_ABS, "abs_mean": R.EDGE_ABS_MEAN}
COMBOS = [(normalize, edge) for normalize in (True, False) for edge in sorted(EDGES)]

with open(HEADER) as _f:
    RAW = _f.read()
TEXT = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)      # the header without its comments
DS_BLOCK_PIXELS = int(re.search(r"constexpr int DS_BLOCK_PIXELS = (\d+);", open(KERNELS).read()).group(1))


# ------------------------------------------------------------------------------------------------------------------------
# 1. header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def _prototypes():
    code = re.sub(r"^\s*#.*$", "", TEXT, flags=re.M)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(sfm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}


def _struct_fields():
    """[(field, ctypes element type, count)] of SfmDispSmoothDesc in declaration order"""
    body = re.search(r"typedef struct SfmDispSmoothDesc \{(.*?)\} SfmDispSmoothDesc;", TEXT, flags=re.S).group(1)
    kinds = {"const float *": C.c_void_p, "float *": C.c_void_p, "double *": C.c_void_p, "int32_t ": C.c_int32, "float ": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const float \*|float \*|double \*|int32_t |float )(.*)$", decl)
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
    assert re.search(r"#define SFM_DISP_SMOOTH_EDGE_MEAN_ABS (\d+)", TEXT).group(1) == str(_lib.DISP_SMOOTH_EDGES["mean_abs"]) == str(R.EDGE_MEAN_ABS) == "0"
    assert re.search(r"#define SFM_DISP_SMOOTH_EDGE_ABS_MEAN (\d+)", TEXT).group(1) == str(_lib.DISP_SMOOTH_EDGES["abs_mean"]) == str(R.EDGE_ABS_MEAN) == "1"
    assert _lib.DISP_SMOOTH_EDGES == {"mean_abs": 0, "abs_mean": 1} and _lib.disp_smooth_edge_id("abs_mean") == 1
    assert not set(_lib.SMOOTH_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.EXT_SYMBOLS))


def test_header_binding_and_library_declare_the_same_symbols():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.SMOOTH_SYMBOLS) == ENTRY_POINTS
    for name, params in protos.items():
        res, args = _lib.SMOOTH_SYMBOLS[name]
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        assert len(args) == len(params), name
        assert res is (C.c_size_t if name.endswith("_bytes") else C.c_int)
        for param, arg in zip(params, args):                       # pointers at the header's positions, integers elsewhere
            if param.startswith("const SfmDispSmoothDesc *"):
                assert arg == C.POINTER(_lib.SfmDispSmoothDesc), (name, param)
            elif "*" in param:
                assert arg is C.c_void_p, (name, param)
            else:
                assert param.startswith("size_t ") and arg is C.c_size_t, (name, param)


def test_descriptor_matches_the_header():
    fields = _struct_fields()
    struct = _lib.SfmDispSmoothDesc
    assert [f[0] for f in fields] == [f[0] for f in struct._fields_] == [
        "B", "n_scales", "H", "W", "normalize", "edge", "accumulate", "weight", "disp", "img", "loss", "stats", "g_loss", "g_disp"]
    off, align = 0, 1
    for (field, ctype, count), (_, bound) in zip(fields, struct._fields_):
        size = C.sizeof(ctype)
        off = -(-off // size) * size                                # the C layout rule: a multiple of the element size
        assert getattr(struct, field).offset == off, field
        assert getattr(struct, field).size == size * count, field
        elem = bound._type_ if count > 1 else bound
        assert C.sizeof(elem) == size and (elem is C.c_float) == (ctype is C.c_float), field
        off += size * count
        align = max(align, size)
    assert C.sizeof(struct) == -(-off // align) * align


def test_the_library_exports_the_three_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported
    assert L.sfm_abi_version() == 6


# ------------------------------------------------------------------------------------------------------------------------
# 2. reject paths: what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _desc(B=2, n_scales=2, hw=((16, 24), (9, 31)), normalize=1, edge=0, accumulate=0, weight=(1.0, 0.5), **kw):
    d = _lib.SfmDispSmoothDesc()
    d.B, d.n_scales, d.normalize, d.edge, d.accumulate = B, n_scales, normalize, edge, accumulate
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
    for s, w in enumerate(weight):
        d.weight[s] = w
    for s in range(max(0, min(n_scales, _lib.SFM_MAX_SCALES))):
        d.disp[s] = d.img[s] = d.g_disp[s] = FAKE
    d.loss = d.stats = d.g_loss = FAKE
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


WS = C.c_void_p(0x100000)      # on a 256-byte boundary, never dereferenced


def _fwd(d, ws=WS, nbytes=1 << 30):
    return L.sfm_disp_smooth_fwd(C.byref(d) if d is not None else None, ws, nbytes, None), _lib.last_error()


def _bwd(d):
    return L.sfm_disp_smooth_bwd(C.byref(d) if d is not None else None, None), _lib.last_error()


def _query(d):
    return L.sfm_disp_smooth_workspace_bytes(C.byref(d) if d is not None else None)


def _both(d):
    return (("sfm_disp_smooth_fwd",) + _fwd(d), ("sfm_disp_smooth_bwd",) + _bwd(d))


def test_null_descriptor():
    for who, rc, msg in _both(None):
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
    assert _query(None) == 0


BAD_SHAPES = [dict(n_scales=0), dict(n_scales=9), dict(B=-1), dict(H=(1, 2)), dict(W=(0, 2)), dict(H=(0, 0)),
              dict(H=(0, 1 << 15), W=(0, 1 << 15))]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=[str(sorted(b.items())) for b in BAD_SHAPES])
def test_bad_shapes(bad):
    for who, rc, msg in _both(_desc(**bad)):
        assert rc == _lib.ERR_SHAPE and msg.startswith(who), (rc, msg)
        assert any(word in msg for word in bad), (bad, msg)
        with pytest.raises(TypeError):
            _lib.check(rc)
    assert _query(_desc(**bad)) == 0


def test_too_many_runs():
    d = _desc(B=(1 << 31) - 1, hw=((3, 3), (3, 3)))
    for who, rc, msg in _both(d):
        assert rc == _lib.ERR_SHAPE and "runs" in msg and msg.startswith(who), (rc, msg)


BAD_CONFIG = [dict(normalize=2), dict(normalize=-1), dict(edge=2), dict(edge=-1), dict(accumulate=2), dict(accumulate=-1),
              dict(weight=(0, -1.0)), dict(weight=(1, float("nan"))), dict(weight=(1, -float("inf")))]


@pytest.mark.parametrize("bad", BAD_CONFIG, ids=[str(sorted(b.items())) for b in BAD_CONFIG])
def test_bad_configuration(bad):
    for who, rc, msg in _both(_desc(**bad)):
        assert rc == _lib.ERR_CONFIG and msg.startswith(who) and next(iter(bad)) in msg, (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert _query(_desc(**bad)) == 0


def test_the_settings_are_checked_in_the_documented_order():
    """normalize, edge, accumulate, the weights"""
    for call in (_fwd, _bwd):
        assert "normalize" in call(_desc(normalize=2, edge=5, accumulate=3, weight=(-1.0, 1.0)))[1]
        assert "edge" in call(_desc(edge=5, accumulate=3, weight=(-1.0, 1.0)))[1]
        assert "accumulate" in call(_desc(accumulate=3, weight=(-1.0, 1.0)))[1]
        assert "weight[0]" in call(_desc(weight=(-1.0, -1.0)))[1]


def test_weights_beyond_n_scales_are_not_looked_at():
    assert _fwd(_desc(B=0, weight=(1.0, 0.0, -1.0, float("nan"))))[0] == 0


FWD_PTRS = [("disp", 1), ("img", 0), "loss", "stats"]
BWD_PTRS = [("disp", 0), ("img", 1), ("g_disp", 1), "stats", "g_loss"]


def _null(field):
    return {field[0]: (field[1], None)} if isinstance(field, tuple) else {field: None}


def _named(field):
    return "%s[%d]" % field if isinstance(field, tuple) else field


@pytest.mark.parametrize("field", FWD_PTRS, ids=str)
def test_forward_null_pointers(field):
    rc, msg = _fwd(_desc(**_null(field)))
    assert rc == _lib.ERR_NULL and _named(field) in msg and msg.startswith("sfm_disp_smooth_fwd"), (rc, msg)
    with pytest.raises(TypeError):
        _lib.check(rc)


@pytest.mark.parametrize("field", BWD_PTRS, ids=str)
def test_backward_null_pointers(field):
    rc, msg = _bwd(_desc(**_null(field)))
    assert rc == _lib.ERR_NULL and _named(field) in msg and msg.startswith("sfm_disp_smooth_bwd"), (rc, msg)


def test_the_pointers_are_checked_in_the_documented_order():
    """scale by scale disp, img and (backward) g_disp; then loss (forward), stats, g_loss (backward)"""
    for call in (_fwd, _bwd):
        assert "img[0]" in call(_desc(img=(0, None), disp=(1, None), stats=None))[1]
        assert "disp[0]" in call(_desc(img=(0, None), disp=(0, None)))[1]
        assert "disp[1]" in call(_desc(disp=(1, None), loss=None, stats=None, g_loss=None))[1]
    assert "loss" in _fwd(_desc(loss=None, stats=None))[1]
    assert "g_disp[0]" in _bwd(_desc(g_disp=(0, None), img=(1, None)))[1]
    assert "stats" in _bwd(_desc(stats=None, g_loss=None))[1]


def test_each_call_ignores_the_others_arrays():
    """the forward does not look at g_loss and g_disp, the backward not at loss: with those NULL a call gets as far as its next
    check -- the workspace for the forward.  (The backward has no check left: it would launch, so its descriptor keeps one NULL
    pointer of its own.)"""
    d = _desc(g_loss=None)
    for s in range(2):
        d.g_disp[s] = None
    rc, msg = _fwd(d, None, 0)
    assert rc == _lib.ERR_WORKSPACE, (rc, msg)
    rc, msg = _bwd(_desc(loss=None, g_loss=None))
    assert rc == _lib.ERR_NULL and "g_loss" in msg, (rc, msg)


def test_workspace_rejections():
    d = _desc()
    need = _query(d)
    assert need > 0
    for ws, nbytes, word in ((None, need, "needed"), (WS, need - 1, "needed"), (WS, 0, "needed"), (C.c_void_p(WS.value + 128), need, "aligned"),
                             (C.c_void_p(WS.value + 4), 1 << 30, "aligned")):
        rc, msg = _fwd(d, ws, nbytes)
        assert rc == _lib.ERR_WORKSPACE and word in msg and msg.startswith("sfm_disp_smooth_fwd"), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)


def test_rejections_come_in_the_documented_order():
    """descriptor, shape, configuration, the empty batch, the pointers, the workspace"""
    null_in = dict(disp=(0, None), stats=None)
    for call in (_fwd, _bwd):
        assert call(_desc(n_scales=0, edge=7, **null_in))[0] == _lib.ERR_SHAPE
        assert call(_desc(H=(1, 2), weight=(-1.0, 1.0), B=0))[0] == _lib.ERR_SHAPE
        assert call(_desc(edge=7, **null_in))[0] == _lib.ERR_CONFIG
        assert call(_desc(B=0, normalize=7))[0] == _lib.ERR_CONFIG                # an empty batch still has its settings checked
        assert call(_desc(B=0, weight=(1.0, -2.0)))[0] == _lib.ERR_CONFIG
        assert call(_desc(B=0, **null_in))[0] == 0                                # ... but not its pointers
        assert call(_desc(**null_in))[0] == _lib.ERR_NULL
    assert _fwd(_desc(**null_in), None, 0)[0] == _lib.ERR_NULL                    # the pointers before the workspace
    assert _fwd(_desc(B=0), None, 0)[0] == 0                                      # an empty batch needs no workspace


def test_empty_batch_launches_nothing_and_checks_no_pointer():
    e = _lib.SfmDispSmoothDesc()            # an empty shard: every pointer NULL, the shape and the settings still checked
    e.n_scales, e.H[0], e.W[0], e.weight[0] = 1, 16, 24, 1.0
    assert _fwd(e, None, 0)[0] == 0 and _bwd(e)[0] == 0
    assert _query(e) == 256
    e.H[0] = 2
    assert _fwd(e, None, 0)[0] == _lib.ERR_SHAPE and _bwd(e)[0] == _lib.ERR_SHAPE and _query(e) == 0


def _blocks(B, hw):
    return sum(B * -(-(h * w) // DS_BLOCK_PIXELS) for h, w in hw)


@pytest.mark.parametrize("B,hw", [(1, [(3, 3)]), (2, [(16, 24), (9, 31)]), (3, [(130, 127)]), (32, [(128, 416), (64, 208), (32, 104), (16, 52)]),
                                  (1, [(3, DS_BLOCK_PIXELS)]), (5, [(3, DS_BLOCK_PIXELS // 3 + 1)])])
def test_workspace_query(B, hw):
    """a multiple of 256 that holds 24 bytes -- three fp64 sums -- per run of DS_BLOCK_PIXELS pixels, and no more than the next
    multiple; it looks at no pointer"""
    d = _lib.SfmDispSmoothDesc()
    d.B, d.n_scales = B, len(hw)
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s], d.weight[s] = h, w, 1.0
    got = _query(d)
    assert got % 256 == 0 and got == -(-24 * _blocks(B, hw) // 256) * 256, (got, _blocks(B, hw))
    d.B = B + 40
    assert _query(d) > got                                                   # it grows with the number of blocks
    d.normalize, d.edge, d.accumulate = 1, 1, 1
    assert _query(d) == -(-24 * _blocks(B + 40, hw) // 256) * 256           # ... and with nothing else


# ------------------------------------------------------------------------------------------------------------------------
# 3. the NumPy restatement on hand-made cases
# ------------------------------------------------------------------------------------------------------------------------
def _one(d, img=None):
    d = np.asarray(d, F32)[None, None]
    return d, (np.zeros((1, 3) + d.shape[2:], F32) if img is None else np.asarray(img, F32)[None])


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_reference_ramp_under_a_constant_image(edge):
    """d = 1 + x + 3 y on 3x3, every weight 1: six |Dx| = 1 and six |Dy| = 3, c_x = c_y = 1/6 -> 1 + 3; the mean is 5"""
    d, img = _one([[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    loss, stats = R.forward([d], [img], [0.5], False, EDGES[edge])
    assert stats[0, 0].tolist() == [1.0, 6.0, 18.0] and loss.tolist() == [4.0, 2.0]
    (g,) = R.backward([d], [img], stats, [1.0, 0.0], [0.5], False, EDGES[edge])
    sixth = float(F32(1 / 6))
    assert g.dtype == F32 and g[0, 0].tolist() == [[-2 * sixth, -sixth, 0.0], [-sixth, 0.0, sixth], [0.0, sixth, 2 * sixth]]
    loss_n, stats_n = R.forward([d], [img], [0.5], True, EDGES[edge])
    assert stats_n[0, 0].tolist() == [5.0 + 1e-7, 6.0, 18.0] and loss_n[0] == 4.0 / (5.0 + 1e-7) and loss_n[1] == 0.5 * loss_n[0]
    # through the mean every pixel gets the same -loss / (M P) on top: a ramp scaled by any factor has the same normalised value
    (gn,) = R.backward([d], [img], stats_n, [1.0, 0.0], [0.5], True, EDGES[edge])
    M = 5.0 + 1e-7
    want = (F32(1 / 6 / M) * (g[0, 0] / F32(1 / 6))).astype(F32) - F32(4.0 / (M * M * 9))
    assert np.array_equal(gn[0, 0], want) and abs(float((gn[0, 0].astype(F64) * d[0, 0]).sum())) < 1e-6
    # the total's upstream gradient arrives through the weight, and `out` is added to once
    (g2,) = R.backward([d], [img], stats, [0.0, 3.0], [0.5], False, EDGES[edge], out=[np.ones_like(d)])
    assert np.array_equal(g2, (1 + (F32(1.5 / 6) * (g / F32(1 / 6))).astype(F32)).astype(F32))


def test_reference_flat_patch():
    """sign(0) = 0: a flat map has no loss and no gradient, a map with a flat part none there"""
    d, img = _one(np.full((3, 4), 2.0))
    for normalize in (False, True):
        loss, stats = R.forward([d], [img], [1.0], normalize, R.EDGE_MEAN_ABS)
        assert loss.tolist() == [0.0, 0.0] and stats[0, 0, 1:].tolist() == [0.0, 0.0]
        (g,) = R.backward([d], [img], stats, [1.0, 1.0], [1.0], normalize, R.EDGE_MEAN_ABS)
        assert not g.any()
    d, img = _one([[1, 1, 2], [1, 1, 2], [1, 1, 2]])
    loss, stats = R.forward([d], [img], [1.0], False, R.EDGE_MEAN_ABS)
    assert stats[0, 0].tolist() == [1.0, 3.0, 0.0] and loss[0] == 0.5
    (g,) = R.backward([d], [img], stats, [1.0, 0.0], [1.0], False, R.EDGE_MEAN_ABS)
    sixth = float(F32(1 / 6))
    assert g[0, 0].tolist() == [[0.0, -sixth, sixth]] * 3


def test_reference_a_single_image_edge():
    """between the columns 1 and 2 channel 0 rises by 3 ln 2 and channel 1 falls by it: mean_c |DI| = 2 ln 2 -> w = 1/4,
    |mean_c DI| = 0 -> w = 1; d = x, so X = 3 (1 + w), Y = 0, loss = (1 + w) / 2"""
    step = 3 * math.log(2.0)
    img = np.zeros((3, 3, 3), F32)
    img[0, :, 2], img[1, :, 2] = step, -step
    d, img = _one([[0, 1, 2]] * 3, img)
    for edge, w in ((R.EDGE_MEAN_ABS, 0.25), (R.EDGE_ABS_MEAN, 1.0)):
        loss, stats = R.forward([d], [img], [1.0], False, edge)
        assert stats[0, 0, 1] == pytest.approx(3 * (1 + w), rel=1e-6) and stats[0, 0, 2] == 0 and loss[0] == pytest.approx((1 + w) / 2, rel=1e-6)
        (g,) = R.backward([d], [img], stats, [1.0, 0.0], [1.0], False, edge)
        assert g[0, 0, 1].tolist() == pytest.approx([-1 / 6, (1 - w) / 6, w / 6], rel=1e-6, abs=1e-9)


# ------------------------------------------------------------------------------------------------------------------------
# 4. the restatement against the float64 statements
# ------------------------------------------------------------------------------------------------------------------------
def make_inputs(B, hw, seed):
    """float32 host arrays ([disp_s (B,1,h,w)], [img_s (B,3,h,w)]): disparities in (0.01, 10) with both signs of difference, flat
    patches (exact zero differences) and the means of neighbouring samples a factor of about 4 or 16 apart; images in [-1,1]"""
    rng = np.random.RandomState(seed)
    disps, imgs = [], []
    for h, w in hw:
        d = rng.uniform(0.1, 0.9, (B, 1, h, w))
        d[:, :, : max(2, h // 3), : max(2, w // 4)] = 0.4                       # a flat corner
        if h >= 5:
            d[:, :, h // 2:h // 2 + 2, :] = d[:, :, h // 2:h // 2 + 1, :]      # two equal rows: zero vertical differences
        d *= (4.0 ** (np.arange(B) % 3))[:, None, None, None] * 0.3    # neighbours in the batch 4x or 16x apart, all below 10
        disps.append(d.astype(F32))
        imgs.append(np.clip(rng.uniform(-1.3, 1.3, (B, 3, h, w)), -1, 1).astype(F32))
    return disps, imgs


def rule(got, o64, o32, what):
    """max|got - o64| <= 4 max|o32 - o64| + 1e-6 max|o64|; prints and returns the observed ratio"""
    got, o64, o32 = np.asarray(got, F64), np.asarray(o64, F64), np.asarray(o32, F64)
    assert np.isfinite(got).all(), what
    err, dev, top = float(np.abs(got - o64).max()), float(np.abs(o32 - o64).max()), float(np.abs(o64).max())
    ratio = err / dev if dev > 0 else (0.0 if err == 0 else float("inf"))
    line = "disp_smooth %s: max|got-o64| %.3g, max|o32-o64| %.3g, ratio %.3g, max|o64| %.3g" % (what, err, dev, ratio, top)
    print(line)
    assert err <= 4 * dev + 1e-6 * top, line
    return ratio


@functools.lru_cache(maxsize=None)
def statement(key, normalize, edge, dtype, device="cpu"):
    """the aten statement on the inputs `key` = (B, hw, seed) in `dtype`, upstream gradients G_LOSS(S)
    -> (loss (S+1,) , [g_disp_s]) as float64 host arrays"""
    B, hw, seed = key
    disps, imgs = make_inputs(B, list(hw), seed)
    S = len(hw)
    xs = [torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_() for a in disps]
    ys = [torch.from_numpy(a).to(device=device, dtype=dtype) for a in imgs]
    total, per_scale = R.aten_statement(xs, ys, [float(w) for w in weights_of(S)], normalize, edge)
    g_loss = g_loss_of(S)
    (total * float(g_loss[S]) + sum(t * float(g) for t, g in zip(per_scale, g_loss[:S]))).backward()
    loss = np.array([float(t.detach()) for t in per_scale] + [float(total.detach())], F64)
    return loss, [x.grad.cpu().numpy().astype(F64) for x in xs]


def weights_of(S):
    return [F32(0.9 ** s) for s in range(S)]          # not powers of two: the weighted sum and k_s round


def g_loss_of(S):
    return (np.random.RandomState(5).uniform(0.5, 1.5, S + 1) * np.where(np.arange(S + 1) % 2, -1, 1)).astype(F32)


SHAPES = [(3, 3), (5, 67), (130, 127)]


@pytest.mark.parametrize("normalize,edge", COMBOS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_reference_against_the_statement_in_float64(hw, normalize, edge):
    key = (2, (hw,), 3)
    disps, imgs = make_inputs(*[key[0], list(key[1]), key[2]])
    assert float(disps[0][1].mean()) > 2 * float(disps[0][0].mean()) and 0.01 < disps[0].min() and disps[0].max() < 10
    loss, stats = R.forward(disps, imgs, weights_of(1), normalize, EDGES[edge])
    g = R.backward(disps, imgs, stats, g_loss_of(1), weights_of(1), normalize, EDGES[edge])
    l64, g64 = statement(key, normalize, edge, torch.float64)
    l32, g32 = statement(key, normalize, edge, torch.float32)
    what = "reference %dx%d normalize=%d %s" % (hw + (normalize, edge))
    for s in range(2):
        rule(loss[s], l64[s], l32[s], "%s loss[%d]" % (what, s))
    rule(g[0], g64[0], g32[0], what + " g_disp")


@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_reference_against_the_oracle(hw):
    """normalize = 0 with edge = abs_mean is compute_disp_smooth of the oracle, value and gradient"""
    disps, imgs = make_inputs(2, [hw], 3)
    one = [F32(1)]
    loss, stats = R.forward(disps, imgs, one, False, R.EDGE_ABS_MEAN)
    (g,) = R.backward(disps, imgs, stats, np.array([1, 0], F32), one, False, R.EDGE_ABS_MEAN)
    o = {dt: (oracle.compute_disp_smooth(imgs[0], disps[0], dt), oracle.compute_disp_smooth_backward(imgs[0], disps[0], dt)) for dt in (F64, F32)}
    what = "reference %dx%d against the oracle" % hw
    rule(loss[0], o[F64][0], o[F32][0], what + " loss")
    rule(g, o[F64][1], o[F32][1], what + " g_disp")


# ------------------------------------------------------------------------------------------------------------------------
# 5. ops.disp_smooth_* and torch_api: what they refuse before anything reaches the library
# ------------------------------------------------------------------------------------------------------------------------
def test_type_and_value_errors():
    assert "disparity_smoothness" in ta.__all__ and {"disp_smooth_fwd", "disp_smooth_bwd"} <= set(ops.__all__)
    disps, tgts = [torch.zeros(2, 1, 16, 24), torch.zeros(2, 1, 8, 12)], [torch.zeros(2, 3, 16, 24), torch.zeros(2, 3, 8, 12)]
    for args in ((disps, tgts), (disps[0], tgts), ([], []), ([d.numpy() for d in disps], tgts)):      # CPU tensors: there is no CPU path
        with pytest.raises(TypeError):
            ta.disparity_smoothness(*args)
        with pytest.raises(TypeError):
            ops.disp_smooth_fwd(*args, [1.0, 0.5], True, "mean_abs")
        with pytest.raises(TypeError):
            ops.disp_smooth_bwd(*args, torch.zeros(2, 2, 3, dtype=torch.float64), torch.zeros(3), [1.0, 0.5], True, "mean_abs")
    with pytest.raises(TypeError):
        ops.disp_smooth_fwd(disps, tgts[:1], [1.0, 0.5], True, "mean_abs")
    with pytest.raises(TypeError, match="weight"):
        ops.disp_smooth_fwd(disps, tgts, [1.0], True, "mean_abs")
    with pytest.raises(ValueError, match="edge"):
        _lib.disp_smooth_edge_id("mean")
    with pytest.raises(ValueError, match="edge"):
        ta.disparity_smoothness(disps, tgts, edge="sobel")
    # the new arguments of min_reprojection_loss are looked at before any array
    for bad in (dict(smooth_weight=-1.0), dict(smooth_weight=float("nan")), dict(smooth_weight=1e-3, smooth_edge="sobel")):
        with pytest.raises(ValueError, match="smooth_weight|edge"):
            ta.min_reprojection_loss(None, None, None, None, None, ssim_rate=0.85, **bad)
    with pytest.raises(TypeError):
        ta.min_reprojection_loss(None, None, None, None, None, ssim_rate=0.85, smooth_weight=1e-3)
