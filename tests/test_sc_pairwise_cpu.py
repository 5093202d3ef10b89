"""include/sfmwarp_pairwise.h without a GPU: the side header, the binding and the library declare the same struct and the same three
entry points; every documented rejection answers with its code, in the documented order and before any HIP call (the pointers are
fakes that are never dereferenced: no call here passes every check); the Python argument errors that are raised before a device is
touched; and the NumPy restatement of the header (tests/sc_pairwise_ref.py) against a float64 torch statement of mean_on_mask /
compute_pairwise_loss, values and autograd gradients."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sc_pairwise_ref as R

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmwarp_pairwise.h")
CSRC = os.path.join(ROOT, "sfm-learner-chainer_amd", "csrc")
FAKE = 0x10000                 # never dereferenced
WS = C.c_void_p(0x100000)      # on a 256-byte boundary, never dereferenced
ENTRY_POINTS = sorted(["sfm_pairwise_workspace_bytes", "sfm_pairwise_fwd", "sfm_pairwise_bwd"])
OTHER_TABLES = ("SYMBOLS", "EXT_SYMBOLS", "SMOOTH_SYMBOLS", "FULL_RES_SYMBOLS", "CONV_SYMBOLS", "POSE_SYMBOLS", "DEPTH_CONS_SYMBOLS")
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


def _struct_fields():
    """[(field, element size, count)] of SfmPairwiseDesc in declaration order"""
    body = re.search(r"typedef struct SfmPairwiseDesc \{(.*?)\} SfmPairwiseDesc;", TEXT, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const float \*|float \*|int8_t \*|int32_t \*|int32_t |float )(.*)$", decl)
        assert m, decl
        size = C.sizeof(C.c_void_p) if m.group(1).endswith("*") else 4
        for item in m.group(2).split(","):
            a = re.match(r"(\w+)(?:\[(\w+)\])?$", item.strip().lstrip("*"))
            assert a, item
            fields.append((a.group(1), size, {"SFM_MAX_SCALES": _lib.SFM_MAX_SCALES, "SFM_MAX_SRC": _lib.SFM_MAX_SRC}[a.group(2)] if a.group(2) else 1))
    return fields


def test_the_side_header_stands_beside_the_main_one():
    assert '#include "sfmwarp.h"' in RAW
    first = re.search(r"/\*.*?\*/", RAW, flags=re.S).group(0)
    assert "sfmwarp.h" in first and "FOLLOW-UP" in first, "the first comment says that this header is to be folded into sfmwarp.h"
    assert "compute_pairwise_loss" in first and "mean_on_mask" in first, "the SC-SfMLearner statements it restates, by function name"
    assert "no address from data" in first, "the paragraph on non-finite inputs says so"
    assert "SFM_ABI_VERSION" not in TEXT and _lib.SFM_ABI_VERSION == 6 and L.sfm_abi_version() == 6
    assert "#define" not in re.sub(r"#define SFMWARP_PAIRWISE_H_", "", TEXT), "it uses the constants of sfmwarp.h, it adds no macro"
    assert TEXT.count("typedef") == 1, "one struct of its own: SfmPairwiseDesc"
    main = open(os.path.join(ROOT, "include", "sfmwarp.h")).read()
    assert "pairwise" not in main, "sfmwarp.h is not edited"


def test_the_struct_is_the_headers():
    fields = _struct_fields()
    assert [f[0] for f in fields] == ["B", "n_src", "n_scales", "H", "W", "detach_weight", "min_count_photo", "min_count_geom", "weight", "err",
                                      "diff", "valid", "ident", "cmp", "keep", "loss", "count", "g_loss", "g_err", "g_diff"]
    struct = _lib.SfmPairwiseDesc
    assert [f[0] for f in fields] == [f[0] for f in struct._fields_]
    off, align = 0, 1
    for field, size, count in fields:
        off = -(-off // size) * size
        assert getattr(struct, field).offset == off, field
        assert getattr(struct, field).size == size * count, field
        off += size * count
        align = max(align, size)
    assert C.sizeof(struct) == -(-off // align) * align
    ptr, S = C.sizeof(C.c_void_p), _lib.SFM_MAX_SCALES
    assert struct.err.offset == -(-(4 * (6 + 3 * S)) // ptr) * ptr
    assert C.sizeof(struct) == struct.err.offset + ptr * (8 * S + 3)


def test_the_symbol_table_is_the_headers_and_disjoint_from_the_other_seven():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.PAIRWISE_SYMBOLS) == ENTRY_POINTS
    for other in OTHER_TABLES:
        assert not set(_lib.PAIRWISE_SYMBOLS) & set(getattr(_lib, other)), other
    kinds = {"const SfmPairwiseDesc *": C.POINTER(_lib.SfmPairwiseDesc), "void *": C.c_void_p, "size_t ": C.c_size_t}
    for name, params in protos.items():
        res, args = _lib.PAIRWISE_SYMBOLS[name]
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


def test_the_unit_reuses_the_shared_pieces_and_is_built():
    unit = open(os.path.join(CSRC, "sfm_pairwise.hip")).read()
    for header in ("sfm_common.h", "sfm_warp_pixel.h"):
        assert '#include "%s"' % header in unit
    for fn in ("scale_of<0>(", "check_pyramid_shape(", "wave_sum_d(", "ldf(", "stf("):
        assert fn in unit, fn
        assert not re.search(r"__forceinline__ \w+ %s\(" % re.escape(fn.split("(")[0].split("<")[0]), unit), "%s is used, not redefined" % fn
    assert "fp contract(off)" in unit and "atomic" not in unit.lower().replace("no atomics", "")
    assert re.search(r"constexpr int PW_BLOCK_PIXELS = (\d+);", unit).group(1) == "256"
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "sfm_pairwise.hip" in make and make.count("sfmwarp_pairwise.h") == 2, "the unit, and the header in both rules"
    for name in ("sfmwarp_pairwise.h", "sfm_pairwise.hip"):      # no existing header or unit is a substring of the new names
        for old in os.listdir(os.path.join(ROOT, "include")) + os.listdir(CSRC):
            assert old == name or old not in name, (old, name)


def test_the_python_signatures():
    p = inspect.signature(ops.pairwise_fwd).parameters
    assert list(p) == ["errs", "diffs", "valids", "idents", "cmps", "weights", "min_counts", "detach_weight"]
    p = inspect.signature(ops.pairwise_bwd).parameters
    assert list(p)[:8] == ["errs", "diffs", "keeps", "count", "g_loss", "weights", "min_counts", "detach_weight"]
    p = inspect.signature(ta.pairwise_mean).parameters
    assert list(p)[:2] == ["errs", "diffs"]
    assert [p[k].default for k in ("valid", "ident", "cmp", "weights", "min_count", "detach_weight")] == [None, None, None, None, (0, 0), False]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("valid", "ident", "cmp", "weights", "min_count", "detach_weight"))
    p = inspect.signature(ta.sc_sfm_loss).parameters
    assert list(p)[:6] == ["tgt_img", "src_imgs", "intrinsics", "tgt_disps", "src_disps", "pred_poses"]
    defaults = dict(ssim_rate=0.85, geometry_weight=0.5, smooth_weight=0.0, auto_mask=False, with_mask=True, detach_weight=False,
                    min_count=(0, 0), weights=None, bidirectional=True, ssim_padding="zero", pose_format="euler", invert=None,
                    depth_range=None, smooth_normalize=True, smooth_edge="mean_abs")
    assert {k: p[k].default for k in defaults} == defaults
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in defaults)
    assert "pairwise_mean" in ta.__all__ and "sc_sfm_loss" in ta.__all__ and "pairwise_fwd" in ops.__all__ and "pairwise_bwd" in ops.__all__
    assert "2**-s" in ta.pairwise_mean.__doc__, "the default weights differ from min_reprojection's, and the docstring says so"
    assert "clamp(0, 1)" in ta.sc_sfm_loss.__doc__, "what is out of scope is said"


# ------------------------------------------------------------------------------------------------------------------------
# 2. what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
PER_SCALE = ("err", "diff", "valid", "ident", "cmp", "keep", "g_err", "g_diff")


def _desc(B=2, n_src=2, n_scales=2, hw=((16, 24), (8, 12)), **kw):
    d = _lib.SfmPairwiseDesc()
    d.B, d.n_src, d.n_scales = B, n_src, n_scales
    for s, (h, w) in enumerate(hw):
        d.H[s], d.W[s] = h, w
    for s in range(_lib.SFM_MAX_SCALES):
        d.weight[s] = 1.0
        for name in PER_SCALE:
            getattr(d, name)[s] = FAKE
    d.loss = d.count = d.g_loss = FAKE
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def _ref(x):
    return C.byref(x) if x is not None else None


def fwd(d, ws=None, nbytes=0):      # (the default workspace is the one the forward rejects LAST: nothing is ever launched)
    return L.sfm_pairwise_fwd(_ref(d), ws, nbytes, None), _lib.last_error()


def bwd(d):
    return L.sfm_pairwise_bwd(_ref(d), None), _lib.last_error()


def query(d):
    return L.sfm_pairwise_workspace_bytes(_ref(d))


CALLS = ((fwd, "sfm_pairwise_fwd"), (bwd, "sfm_pairwise_bwd"))
# the rejects of the header's list in its order: each row fails its own check and, where it can, every LATER one too
SHAPE_REJECTS = [(dict(n_src=0), "n_src"), (dict(n_src=9), "n_src"), (dict(n_scales=0), "n_scales"), (dict(n_scales=9), "n_scales"),
                 (dict(B=-1), "B=-1"), (dict(H=(1, 2)), "H=2"), (dict(W=(0, 2)), "W=2"), (dict(H=(0, 40000), W=(0, 40000)), "too large"),
                 (dict(B=1 << 30, H=(0, 17), W=(0, 17)), "too many"), (dict(B=1 << 17, H=(0, 128), W=(0, 128)), "int32 count")]
CONFIG_REJECTS = [(dict(detach_weight=2), "detach_weight=2"), (dict(detach_weight=-1), "detach_weight=-1"),
                  (dict(min_count_photo=-1), "min_count_photo"), (dict(min_count_geom=-5), "min_count_geom"),
                  (dict(weight=(1, -0.5)), "weight[1]"), (dict(weight=(0, float("nan"))), "weight[0]")]


def test_the_descriptor_then_the_shape():
    for call, who in CALLS:
        rc, msg = call(None)
        assert rc == _lib.ERR_NULL and "descriptor" in msg and msg.startswith(who)
        for bad, word in SHAPE_REJECTS:
            rc, msg = call(_desc(detach_weight=7, err=(0, None), **bad))      # ... before the settings and the pointers: both are bad here
            assert rc == _lib.ERR_SHAPE and word in msg and msg.startswith(who), (bad, rc, msg)
            with pytest.raises(TypeError):
                _lib.check(rc)
            assert query(_desc(**bad)) == 0
        # the order inside the group: n_src, n_scales, B, the frames, the count
        assert "n_src" in call(_desc(n_src=0, n_scales=0, B=-1))[1] and "n_scales" in call(_desc(n_scales=0, B=-1))[1]
        assert "B=-1" in call(_desc(B=-1, H=(0, 1)))[1]
    assert query(None) == 0


def test_then_the_settings():
    for call, who in CALLS:
        for bad, word in CONFIG_REJECTS:
            for d in (_desc(err=(0, None), **bad), _desc(B=0, **bad)):          # before the pointers, before the empty batch
                rc, msg = call(d)
                assert rc == _lib.ERR_CONFIG and word in msg and msg.startswith(who), (bad, rc, msg)
                with pytest.raises(ValueError):
                    _lib.check(rc)
            assert query(_desc(**bad)) == 0
        # the order inside the group: detach_weight, min_count_photo, min_count_geom, the weights
        assert "detach_weight" in call(_desc(detach_weight=3, min_count_photo=-1, min_count_geom=-1, weight=(0, -1.0)))[1]
        assert "min_count_photo" in call(_desc(min_count_photo=-1, min_count_geom=-1, weight=(0, -1.0)))[1]
        assert "min_count_geom" in call(_desc(min_count_geom=-1, weight=(0, -1.0)))[1]
        assert call(_desc(B=0, weight=(5, -1.0)))[0] == 0, "a weight beyond n_scales is not looked at"


def test_then_the_empty_batch_the_pointers_and_the_workspace():
    empty = _desc(B=0)
    for name in PER_SCALE:
        for s in range(_lib.SFM_MAX_SCALES):
            getattr(empty, name)[s] = None
    empty.loss = empty.count = empty.g_loss = None
    assert fwd(empty)[0] == 0 and bwd(empty)[0] == 0, "B == 0 returns 0 with NULL pointers"
    order = [(("err", 0), (fwd, bwd)), (("diff", 0), (fwd, bwd)), (("keep", 0), (fwd, bwd)), (("g_err", 0), (bwd,)),
             (("err", 1), (fwd, bwd)), (("diff", 1), (fwd, bwd)), (("keep", 1), (fwd, bwd)), (("g_err", 1), (bwd,)),
             ("loss", (fwd,)), ("count", (fwd, bwd)), ("g_loss", (bwd,))]
    for k, (field, calls) in enumerate(order):
        for call in calls:
            # this pointer and every later one of the call NULL: the first in the documented order is the one that is named
            d = _desc()
            for later, later_calls in order[k:]:
                if call in later_calls:
                    if isinstance(later, tuple):
                        getattr(d, later[0])[later[1]] = None
                    else:
                        setattr(d, later, None)
            rc, msg = call(d)
            assert rc == _lib.ERR_NULL and ("%s[%d]" % field if isinstance(field, tuple) else field) in msg, (field, rc, msg)
            with pytest.raises(TypeError):
                _lib.check(rc)
    # bound for some scales but not all: after the pointers above, before the workspace
    for name, call in (("ident", fwd), ("cmp", fwd), ("g_diff", bwd)):
        for at in (0, 1):
            rc, msg = call(_desc(**{name: (at, None)}))
            assert rc == _lib.ERR_NULL and name in msg and "all or none" in msg, (name, rc, msg)
    assert "ident" in fwd(_desc(ident=(0, None), cmp=(1, None)))[1]
    assert "loss" in fwd(_desc(loss=None, ident=(0, None)))[1]
    # valid is optional scale by scale; ident, cmp and g_diff may be NULL for every scale; entries beyond n_scales are not looked at:
    # each of these reaches the workspace check, which is the last one (and nothing is launched)
    need = query(_desc())
    assert need == -(-(2 * (2 + 1) * 2 * 20) // 256) * 256, "(runs of all scales and samples) * n_src * 20 bytes"
    for kw in (dict(valid=(0, None)), dict(valid=(1, None)), dict(ident=(5, None)), dict(err=(2, None))):
        rc, msg = fwd(_desc(**kw))
        assert rc == _lib.ERR_WORKSPACE and "needed" in msg, (kw, rc, msg)
    d = _desc()
    for s in range(2):
        d.ident[s] = d.cmp[s] = None
    assert fwd(d)[0] == _lib.ERR_WORKSPACE
    for ws, nbytes, word in ((None, need, "needed"), (WS, need - 1, "needed"), (C.c_void_p(WS.value + 128), need, "aligned")):
        rc, msg = fwd(_desc(), ws, nbytes)
        assert rc == _lib.ERR_WORKSPACE and word in msg and msg.startswith("sfm_pairwise_fwd"), (rc, msg)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert fwd(_desc(err=(0, None)), None, 0)[0] == _lib.ERR_NULL, "the pointers before the workspace"
    bare = _desc()
    for name in PER_SCALE:
        for s in range(_lib.SFM_MAX_SCALES):
            getattr(bare, name)[s] = None
    bare.loss = bare.count = bare.g_loss = None
    assert query(bare) == need, "the query looks at no pointer"
    for B, n_src, hw in ((3, 4, ((48, 120),)), (1, 1, ((3, 3),)), (2, 8, ((20, 130), (10, 65), (5, 32)))):
        runs = sum(B * -(-h * w // 256) for h, w in hw)
        assert query(_desc(B=B, n_src=n_src, n_scales=len(hw), hw=hw)) == -(-(runs * n_src * 20) // 256) * 256


# ------------------------------------------------------------------------------------------------------------------------
# 3. the Python argument errors that need no device
# ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_anything_else():
    x = torch.zeros(1)                       # never looked at
    for bad in (dict(min_count=(0, -1)), dict(min_count=3), dict(min_count=(1, 2, 3))):
        with pytest.raises(ValueError, match="min_count"):
            ta.pairwise_mean([x], [x], **bad)
    with pytest.raises(TypeError, match="per scale"):
        ta.pairwise_mean(x, [x])
    with pytest.raises(TypeError, match="scales"):
        ta.pairwise_mean([x], [x, x])
    with pytest.raises(TypeError, match="weights"):
        ta.pairwise_mean([x], [x], weights=[1.0, 1.0])
    with pytest.raises(TypeError, match="CPU"):
        ta.pairwise_mean([x], [x])
    for fn, args in ((ops.pairwise_fwd, ([x], [x], None, None, None, [1.0], (0, 0), False)),
                     (ops.pairwise_bwd, ([x], [x], [x], x, x, [1.0], (0, 0), False))):
        with pytest.raises(TypeError, match="CPU"):
            fn(*args)
        with pytest.raises(TypeError, match="one entry per scale"):
            fn(*(([x, x],) + args[1:]))
    for bad, word in ((dict(auto_mask="ssim"), "auto_mask"), (dict(auto_mask=True), "auto_mask"), (dict(ssim_padding="edge"), "ssim_padding"),
                      (dict(pose_format="matrix"), "matrix"), (dict(pose_format="quaternion"), "pose_format"), (dict(invert=[True, False]), "one inversion flag"),
                      (dict(min_count=(-1, 0)), "min_count"), (dict(smooth_weight=-1.0), "smooth_weight"), (dict(depth_range=(2.0, 1.0)), "depth_range")):
        with pytest.raises(ValueError, match=word):
            ta.sc_sfm_loss(x, x, x, [x], [x], [x], **bad)
    with pytest.raises(TypeError):           # valid settings: the first complaint is about the arrays (CPU tensors)
        ta.sc_sfm_loss(x, x, x, [x], [x], [x], auto_mask="l1", pose_format="matrix", bidirectional=False)


# ------------------------------------------------------------------------------------------------------------------------
# 4. the restatement against compute_pairwise_loss / mean_on_mask in float64 torch
# ------------------------------------------------------------------------------------------------------------------------
# What separates the two: the restatement rounds 1 - diff and err * (1 - diff) to float32 (two roundings of at most 2^-24 each, relative,
# on a sum of positive terms) and each scalar once more (half an ulp): at most 0.5 + 2 ulp for a scalar.  A gradient element is
# cp or cg rounded once (2^-24) and combined by one or two more float32 operations; g_diff = cg - err * cp can cancel, so it is held
# in units of the spacing at |cg| + |err * cp|.  A relative 2^-24 is at most one ulp of the result, so the worst cases are 2.5 ulp for
# a scalar and 3 for a gradient element.  MEASURED here (the eight cases below): scalars at most 0.51 ulp, g_err at most
# 1.67 ulp, g_diff at most 1.12 of that spacing.  The bounds are the worst cases of the argument, not the measurement.
SCALAR_ULP, G_ERR_ULP, G_DIFF_ULP = 2.5, 3.0, 3.0
# min_counts: which of the two thresholds is set -- to the median of the counts, so that half of the pairs fall under it
STATEMENT_CASES = [dict(), dict(detach=True), dict(ident=True), dict(ident=True, cmp=True), dict(min_counts=(True, False)),
                   dict(min_counts=(False, True)), dict(ident=True, cmp=True, detach=True, min_counts=(True, True), valid_none=(1,)),
                   dict(valid=False)]


@pytest.mark.parametrize("case", STATEMENT_CASES, ids=lambda c: "-".join(sorted(c)) or "plain")
def test_the_restatement_is_compute_pairwise_loss(case):
    hw, B, n = ((9, 14), (5, 7), (12, 6)), 3, 2
    x = R.inputs(B, n, hw, seed=7, valid_none=case.get("valid_none", ()))
    valids = x["valids"] if case.get("valid", True) else None
    idents = x["idents"] if case.get("ident") else None
    cmps = x["cmps"] if case.get("cmp") else None
    weights, detach = (1.0, 0.5, 0.3), case.get("detach", False)
    N = len(hw) * n
    median = int(np.median(R.forward(x["errs"], x["diffs"], valids, idents, cmps, weights, (0, 0))[1]))
    min_counts = tuple(median if on else 0 for on in case.get("min_counts", (False, False)))
    g_loss = np.random.RandomState(3).uniform(0.2, 1.5, 2 * N + 2).astype(F32)
    loss, count, keeps = R.forward(x["errs"], x["diffs"], valids, idents, cmps, weights, min_counts)
    g_errs, g_diffs = R.backward(x["errs"], x["diffs"], keeps, count, g_loss, weights, min_counts, detach)
    want, w_errs, w_diffs = R.torch_statement(x["errs"], x["diffs"], valids, idents, cmps, weights, min_counts, detach, g_loss)
    if any(min_counts):      # the case does what it is for: some pairs fall under the threshold and some do not
        for k, m in enumerate(min_counts):
            if m:
                assert (count <= m).any() and (count > m).any(), count
                assert (loss[k * N:(k + 1) * N][count <= m] == 0).all()
    assert count.min() > 0 and (valids is None or all(0 < k.mean() < 1 for k in keeps))
    worst = R.ulp_distance(loss, want).max()
    print("scalars: %.3g ulp" % worst)
    assert worst <= SCALAR_ULP
    for s in range(len(hw)):
        e = R.ulp_distance(g_errs[s], w_errs[s]).max()
        # the spacing at |cg| + |err * cp| >= |g_diff|: cg = g_diff + err * cp in exact arithmetic, err * cp = err * g_err / (1 - diff)
        ecp = np.abs(x["errs"][s].astype(F64) * w_errs[s] / (1.0 - x["diffs"][s].astype(F64)))
        top = np.abs(w_diffs[s]) + (0 if detach else 2 * ecp)
        d = (np.abs(g_diffs[s] - w_diffs[s]) / np.spacing(np.maximum(top, np.finfo(F32).tiny).astype(F32)).astype(F64)).max()
        print("scale %d: g_err %.3g ulp, g_diff %.3g spacings" % (s, e, d))
        assert e <= G_ERR_ULP and d <= G_DIFF_ULP
        assert any(min_counts) or ((g_errs[s] != 0) == (keeps[s] != 0)).all()
