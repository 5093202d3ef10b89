"""sfm_min_reproj_* (include/sfmwarp_min_reproj.h) without a GPU: the side header, the binding and the library declare the same
three entry points and the same descriptor; every documented rejection answers with its code and a message, in the documented order
and before any HIP call (the pointers are fakes that are never dereferenced); the workspace query; and the NumPy reference
(tests/min_reproj_ref.py) on hand-made cases whose answers are written out here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import min_reproj_ref as R

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmwarp_min_reproj.h")
KERNELS = os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc", "sfm_min_reproj.hip")
FAKE = 0x10000                 # never dereferenced
ENTRY_POINTS = ["sfm_min_reproj_bwd", "sfm_min_reproj_fwd", "sfm_min_reproj_workspace_bytes"]
CONSTANTS = {"SFM_MAX_SCALES": _lib.SFM_MAX_SCALES, "SFM_MAX_SRC": _lib.SFM_MAX_SRC}

with open(HEADER) as _f:
    RAW = _f.read()
TEXT = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)      # the header without its comments
MR_BLOCK_PIXELS = int(re.search(r"constexpr int MR_BLOCK_PIXELS = (\d+);", open(KERNELS).read()).group(1))


# ------------------------------------------------------------------------------------------------------------------------
# 1. + 2. header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def _prototypes():
    code = re.sub(r"^\s*#.*$", "", TEXT, flags=re.M)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(sfm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}


def _struct_fields():
    """[(field, ctypes element type, count)] of SfmMinReprojDesc in declaration order"""
    body = re.search(r"typedef struct SfmMinReprojDesc \{(.*?)\} SfmMinReprojDesc;", TEXT, flags=re.S).group(1)
    kinds = {"const float *": C.c_void_p, "float *": C.c_void_p, "int8_t *": C.c_void_p, "int32_t *": C.c_void_p,
             "int32_t ": C.c_int32, "float ": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const float \*|float \*|int8_t \*|int32_t \*|int32_t |float )(.*)$", decl)
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
    assert re.search(r"#define SFM_MIN_REPROJ_NORM_KEPT (\d+)", TEXT).group(1) == str(_lib.MIN_REPROJ_NORM_KEPT) == str(R.NORM_KEPT)
    assert re.search(r"#define SFM_MIN_REPROJ_NORM_ALL (\d+)", TEXT).group(1) == str(_lib.MIN_REPROJ_NORM_ALL) == str(R.NORM_ALL)
    assert not set(_lib.EXT_SYMBOLS) & set(_lib.SYMBOLS)


def test_header_binding_and_library_declare_the_same_symbols():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.EXT_SYMBOLS) == ENTRY_POINTS
    for name, params in protos.items():
        res, args = _lib.EXT_SYMBOLS[name]
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype == res, name
        assert len(args) == len(params), name
        assert res is (C.c_size_t if name.endswith("_bytes") else C.c_int)
        for param, arg in zip(params, args):                       # pointers at the header's positions, integers elsewhere
            if param.startswith("const SfmMinReprojDesc *"):
                assert arg == C.POINTER(_lib.SfmMinReprojDesc), (name, param)
            elif "*" in param:
                assert arg is C.c_void_p, (name, param)
            else:
                assert param.startswith("size_t ") and arg is C.c_size_t, (name, param)


def test_descriptor_matches_the_header():
    fields = _struct_fields()
    struct = _lib.SfmMinReprojDesc
    assert [f[0] for f in fields] == [f[0] for f in struct._fields_] == [
        "B", "n_err", "n_ident", "n_scales", "H", "W", "norm", "weight", "err", "valid", "ident", "winner", "loss", "count", "g_loss", "g_err"]
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
# 3. reject paths: what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _desc(B=2, n_err=2, n_ident=1, n_scales=2, hw=((16, 24), (9, 31)), norm=0, weight=(1.0, 0.5), **kw):
    d = _lib.SfmMinReprojDesc()
    d.B, d.n_err, d.n_ident, d.n_scales, d.norm = B, n_err, n_ident, n_scales, norm
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
    for s, w in enumerate(weight):
        d.weight[s] = w
    for s in range(max(0, min(n_scales, _lib.SFM_MAX_SCALES))):
        d.err[s] = d.valid[s] = d.ident[s] = d.winner[s] = d.g_err[s] = FAKE
    d.loss = d.count = d.g_loss = FAKE
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


WS = C.c_void_p(0x100000)      # on a 256-byte boundary, never dereferenced


def _fwd(d, ws=WS, nbytes=1 << 30):
    return L.sfm_min_reproj_fwd(C.byref(d) if d is not None else None, ws, nbytes, None), _lib.last_error()


def _bwd(d):
    return L.sfm_min_reproj_bwd(C.byref(d) if d is not None else None, None), _lib.last_error()


def _query(d):
    return L.sfm_min_reproj_workspace_bytes(C.byref(d) if d is not None else None)


def _both(d):
    return (("sfm_min_reproj_fwd",) + _fwd(d), ("sfm_min_reproj_bwd",) + _bwd(d))


def test_null_descriptor():
    for who, rc, msg in _both(None):
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
    assert _query(None) == 0


BAD_SHAPES = [dict(n_err=0), dict(n_err=9), dict(n_ident=-1), dict(n_ident=9), dict(n_scales=0), dict(n_scales=9), dict(B=-1),
              dict(H=(1, 2)), dict(W=(0, 2)), dict(H=(0, 0)), dict(H=(0, 1 << 15), W=(0, 1 << 15)),
              dict(B=1 << 22, H=(0, 32), W=(0, 32))]      # B * H * W = 2^32: count[s] would not fit an int32


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


BAD_CONFIG = [dict(norm=2), dict(norm=-1), dict(weight=(0, -1.0)), dict(weight=(1, float("nan"))), dict(weight=(1, -float("inf")))]


@pytest.mark.parametrize("bad", BAD_CONFIG, ids=[str(sorted(b.items())) for b in BAD_CONFIG])
def test_bad_configuration(bad):
    for who, rc, msg in _both(_desc(**bad)):
        assert rc == _lib.ERR_CONFIG and msg.startswith(who) and next(iter(bad)) in msg, (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert _query(_desc(**bad)) == 0


def test_weights_beyond_n_scales_are_not_looked_at():
    assert _fwd(_desc(B=0, weight=(1.0, 0.0, -1.0, float("nan"))))[0] == 0


FWD_PTRS = [("err", 1), ("ident", 0), ("winner", 1), "loss", "count"]
BWD_PTRS = [("winner", 0), ("g_err", 1), "count", "g_loss"]


def _null(field):
    return {field[0]: (field[1], None)} if isinstance(field, tuple) else {field: None}


def _named(field):
    return "%s[%d]" % field if isinstance(field, tuple) else field


@pytest.mark.parametrize("field", FWD_PTRS, ids=str)
def test_forward_null_pointers(field):
    rc, msg = _fwd(_desc(**_null(field)))
    assert rc == _lib.ERR_NULL and _named(field) in msg and msg.startswith("sfm_min_reproj_fwd"), (rc, msg)
    with pytest.raises(TypeError):
        _lib.check(rc)


@pytest.mark.parametrize("field", BWD_PTRS, ids=str)
def test_backward_null_pointers(field):
    rc, msg = _bwd(_desc(**_null(field)))
    assert rc == _lib.ERR_NULL and _named(field) in msg and msg.startswith("sfm_min_reproj_bwd"), (rc, msg)


def test_each_call_ignores_the_others_arrays():
    """valid may be NULL scale by scale, ident with n_ident = 0; the forward does not look at g_loss and g_err, the backward not at
    err, valid, ident and loss: with those NULL a call gets as far as its next check -- the workspace for the forward.  (The
    backward has no check left: it would launch, so its descriptor keeps one NULL pointer of its own.)"""
    d = _desc(n_ident=0, g_loss=None)
    for s in range(2):
        d.valid[s] = d.ident[s] = d.g_err[s] = None
    rc, msg = _fwd(d, None, 0)
    assert rc == _lib.ERR_WORKSPACE, (rc, msg)
    d = _desc(loss=None, count=None)
    for s in range(2):
        d.err[s] = d.valid[s] = d.ident[s] = None
    rc, msg = _bwd(d)
    assert rc == _lib.ERR_NULL and "count" in msg, (rc, msg)


def test_workspace_rejections():
    d = _desc()
    need = _query(d)
    assert need > 0
    for ws, nbytes, word in ((None, need, "needed"), (WS, need - 1, "needed"), (WS, 0, "needed"), (C.c_void_p(WS.value + 128), need, "aligned"),
                             (C.c_void_p(WS.value + 4), 1 << 30, "aligned")):
        rc, msg = _fwd(d, ws, nbytes)
        assert rc == _lib.ERR_WORKSPACE and word in msg and msg.startswith("sfm_min_reproj_fwd"), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)


def test_rejections_come_in_the_documented_order():
    """descriptor, shape, configuration, the empty batch, the pointers, the workspace"""
    null_err = dict(err=(0, None), winner=(0, None))
    for call in (_fwd, _bwd):
        assert call(_desc(n_err=0, norm=7, **null_err))[0] == _lib.ERR_SHAPE
        assert call(_desc(n_ident=9, norm=7, B=0))[0] == _lib.ERR_SHAPE
        assert call(_desc(H=(1, 2), weight=(-1.0, 1.0), B=0))[0] == _lib.ERR_SHAPE
        assert call(_desc(norm=7, **null_err))[0] == _lib.ERR_CONFIG
        assert call(_desc(B=0, norm=7))[0] == _lib.ERR_CONFIG                # an empty batch still has its settings checked
        assert call(_desc(B=0, weight=(1.0, -2.0)))[0] == _lib.ERR_CONFIG
        assert call(_desc(B=0, **null_err))[0] == 0                          # ... but not its pointers
        assert call(_desc(**null_err))[0] == _lib.ERR_NULL
    assert _fwd(_desc(**null_err), None, 0)[0] == _lib.ERR_NULL              # the pointers before the workspace
    assert _fwd(_desc(B=0), None, 0)[0] == 0                                 # an empty batch needs no workspace


def test_empty_batch_launches_nothing_and_checks_no_pointer():
    e = _lib.SfmMinReprojDesc()            # an empty shard: every pointer NULL, the shape and the settings still checked
    e.n_err, e.n_ident, e.n_scales, e.H[0], e.W[0], e.weight[0] = 2, 2, 1, 16, 24, 1.0
    assert _fwd(e, None, 0)[0] == 0 and _bwd(e)[0] == 0
    assert _query(e) == 256
    e.H[0] = 2
    assert _fwd(e, None, 0)[0] == _lib.ERR_SHAPE and _bwd(e)[0] == _lib.ERR_SHAPE and _query(e) == 0


# ------------------------------------------------------------------------------------------------------------------------
# 4. the workspace query
# ------------------------------------------------------------------------------------------------------------------------
def _blocks(B, hw):
    return sum(B * -(-(h * w) // MR_BLOCK_PIXELS) for h, w in hw)


@pytest.mark.parametrize("B,hw", [(1, [(3, 3)]), (2, [(16, 24), (9, 31)]), (3, [(130, 127)]), (32, [(128, 416), (64, 208), (32, 104), (16, 52)]),
                                  (1, [(3, MR_BLOCK_PIXELS)]), (5, [(3, MR_BLOCK_PIXELS // 3 + 1)])])
def test_workspace_query(B, hw):
    """a multiple of 256 that holds 12 bytes -- an fp64 sum and an int32 count -- per run of MR_BLOCK_PIXELS pixels, and no more than
    the next multiple; it looks at no pointer"""
    d = _lib.SfmMinReprojDesc()
    d.B, d.n_err, d.n_ident, d.n_scales = B, 2, 0, len(hw)
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s], d.weight[s] = h, w, 1.0
    got = _query(d)
    assert got % 256 == 0 and got == -(-12 * _blocks(B, hw) // 256) * 256, (got, _blocks(B, hw))
    d.B = B + 40
    assert _query(d) > got                                                   # it grows with the number of blocks
    d.n_err, d.n_ident = 8, 8
    assert _query(d) == -(-12 * _blocks(B + 40, hw) // 256) * 256           # ... and with nothing else


# ------------------------------------------------------------------------------------------------------------------------
# 5. the NumPy reference on hand-made cases
# ------------------------------------------------------------------------------------------------------------------------
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _maps(*rows):
    """(1, n, 1, w) from n rows of w values"""
    return np.array(rows, np.float32)[None, :, None, :]


def test_reference_tie_invalid_nan_inf_and_the_strict_floor():
    #            tie    all invalid   best == floor   NaN first   +inf first   both non-finite   plain
    err = _maps([0.5,   0.1,          0.3,            NAN,        INF,         NAN,              0.7],
                [0.5,   0.2,          0.4,            0.6,        0.9,         INF,              0.2])
    valid = _maps([1,   0,            1,              1,          1,           1,                1],
                  [1,   0,            1,              1,          1,           1,                0])
    ident = _maps([1.0, 1.0,          0.3,            1.0,        1.0,         1.0,              0.7],
                  [2.0, 2.0,          0.5,            NAN,        INF,         2.0,              0.8])
    win, best = R.select(err, valid, ident)
    assert win.dtype == np.int8 and win.shape == (1, 1, 7)
    assert win.ravel().tolist() == [0, -1, -1, 1, 1, -1, -1]           # (the last: its best 0.7 is not below the floor 0.7)
    assert best.ravel()[[0, 3, 4]].tolist() == [0.5, np.float32(0.6), np.float32(0.9)] and np.isinf(best.ravel()[[1, 5]]).all()
    # without the auto-mask the pixels the floor dropped come back; without valid the invalid ones
    assert R.select(err, valid, None)[0].ravel().tolist() == [0, -1, 0, 1, 1, -1, 0]
    assert R.select(err, None, None)[0].ravel().tolist() == [0, 0, 0, 1, 1, -1, 1]
    # an ident that is +inf or NaN everywhere is no floor at all
    assert R.select(err, valid, np.full_like(ident, NAN))[0].ravel().tolist() == [0, -1, 0, 1, 1, -1, 0]

    w = [np.float32(0.25)]
    loss, count, winners = R.forward([err], [valid], [ident], w, R.NORM_KEPT)
    total = float(np.float32(0.5)) + float(np.float32(0.6)) + float(np.float32(0.9))
    assert count.tolist() == [3] and loss[0] == total / 3 and loss[1] == 0.25 * total / 3
    loss_all, count_all, _ = R.forward([err], [valid], [ident], w, R.NORM_ALL)
    assert count_all.tolist() == [3] and loss_all[0] == total / 7 and loss_all[1] == 0.25 * total / 7

    g_loss = np.array([2.0, 8.0], np.float32)
    (g,) = R.backward(winners, count, g_loss, 2, w, R.NORM_KEPT)
    c = np.float32((2.0 + 0.25 * 8.0) / 3)
    assert g.dtype == np.float32 and g.shape == err.shape
    assert g[0, 0, 0].tolist() == [c, 0, 0, 0, 0, 0, 0] and g[0, 1, 0].tolist() == [0, 0, 0, c, c, 0, 0]
    (g,) = R.backward(winners, count, g_loss, 2, w, R.NORM_ALL)
    assert g[0, 0, 0, 0] == np.float32(4.0 / 7) and (g != 0).sum() == 3


@pytest.mark.parametrize("norm", [R.NORM_KEPT, R.NORM_ALL])
def test_reference_a_scale_with_nothing_kept(norm):
    """loss 0, count 0, no NaN; the other scale is unaffected and the total is its weighted share alone"""
    rng = np.random.default_rng(0)
    e0, e1 = rng.uniform(0.1, 1, (2, 2, 3, 5)).astype(np.float32), rng.uniform(0.1, 1, (2, 2, 4, 3)).astype(np.float32)
    nothing = np.zeros_like(e0)                                              # every source invalid everywhere
    loss, count, winners = R.forward([e0, e1], [nothing, None], None, [np.float32(1), np.float32(0.5)], norm)
    assert count.tolist() == [0, 24] and loss[0] == 0 and np.isfinite(loss).all() and (winners[0] == -1).all()
    assert loss[1] == pytest.approx(float(e1.min(1).astype(np.float64).sum()) / 24, rel=1e-15) and loss[2] == pytest.approx(0.5 * loss[1], rel=1e-15)
    g = R.backward(winners, count, np.array([1, 1, 1], np.float32), 2, [1.0, 0.5], norm)
    assert (g[0] == 0).all() and np.isfinite(g[1]).all() and (g[1] != 0).sum() == 24
    # the same through an ident that is below everything
    loss, count, _ = R.forward([e0, e1], None, [np.zeros_like(e0), np.full_like(e1, 2)], [1.0, 0.5], norm)
    assert count.tolist() == [0, 24] and loss[0] == 0


def test_reference_ulp_rule():
    x = np.float32(0.3)
    assert R.within_one_ulp(x, float(x)) and R.within_one_ulp(np.nextafter(x, np.float32(1)), float(x))
    assert not R.within_one_ulp(np.nextafter(np.nextafter(x, np.float32(1)), np.float32(1)), float(x))
    assert R.within_one_ulp(np.float32(0), 0.0) and not R.within_one_ulp(np.float32(1e-30), 0.0)


# ------------------------------------------------------------------------------------------------------------------------
# ops.min_reproj_* and torch_api.min_reprojection*: what they refuse before anything reaches the library
# ------------------------------------------------------------------------------------------------------------------------
def test_type_and_value_errors():
    assert {"min_reprojection", "min_reprojection_loss"} <= set(ta.__all__) and {"min_reproj_fwd", "min_reproj_bwd"} <= set(ops.__all__)
    errs = [torch.zeros(2, 2, 16, 24), torch.zeros(2, 2, 8, 12)]
    for args in ((errs,), (errs[0],), ([],), ([e.numpy() for e in errs],)):      # CPU tensors: there is no CPU path
        with pytest.raises(TypeError):
            ta.min_reprojection(*args)
        with pytest.raises(TypeError):
            ops.min_reproj_fwd(*args, None, None, [1.0, 0.5], "kept")
    with pytest.raises(TypeError):
        ops.min_reproj_bwd([torch.zeros(2, 16, 24)], torch.zeros(1, dtype=torch.int32), torch.zeros(2), 2, [1.0], "kept", [(16, 24)])
    with pytest.raises(ValueError, match="norm"):
        _lib.min_reproj_norm_id("mean")
    with pytest.raises(TypeError, match="weights"):
        ta._scale_weights([1.0], 2)
    assert ta._scale_weights(None, 3) == (1.0, 0.5, 0.25)
