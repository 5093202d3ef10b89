"""What can be proven about non-finite and absurd geometry inputs WITHOUT a device, before any of them goes to one
(tests/hostile_inputs.py is the catalogue, tests/test_hostile_inputs_gpu.py runs it):

  1. the helpers -- classes, same_numbers, corrupt -- do what the GPU module relies on;
  2. THE INDEX RESTATEMENT: the integer part of pad_taps (csrc/sfm_warp_pixel.h), interp_taps (csrc/sfm_ops.hip), project_q
     (csrc/sfm_common.h) and ref_proj_cell (csrc/sfm_ssim_pass.h), restated in float32 NumPy, forms on EVERY catalogue input only
     indices inside the image or on its one-pixel zero frame, and applies the C conversion (int) only to operands for which it is
     defined.  The restatement follows the C semantics, not NumPy's: fmaxf(NaN, 0) = 0 and fminf(fmaxf(x, lo), hi) turns a NaN into
     lo, where np.clip keeps the NaN -- test_the_c_clamp_is_not_np_clip states the difference, and test_the_restatement_is_the_oracle
     _on_clean_inputs ties the restatement to the statement the rest of the suite trusts;
  3. the extreme but finite values: the float32 oracle raises no floating-point exception on them, and agrees with the float64
     oracle on the in-view set with a margin of 1e-3;
  4. the table of deliberate deviations is consistent: the float32 statements and the same statements with the kernels' clamps
     differ on a catalogue case exactly when an entry of hostile_inputs.DEVIATIONS applies to it, every entry is hit, and every
     entry's line stands in the header it names."""
import os

import numpy as np
import pytest

import hostile_inputs as HI
import warp_exact_ref as R
from hostile_inputs import F32, F64, INF, NAN
from oracle import sfm_oracle as O
import knife_free as KF
from test_loss_gpu import CONFIGS, _knife

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the helpers
# ---------------------------------------------------------------------------------------------------------------------------
def test_classes_same_numbers_and_corrupt():
    a = np.array([1.0, -0.0, INF, -INF, NAN, 1e-40, 3e38], F32)
    assert HI.classes(a).tolist() == [HI.FINITE, HI.FINITE, HI.POS_INF, HI.NEG_INF, HI.IS_NAN, HI.FINITE, HI.FINITE]
    b = a.copy()
    b[1] = 0.0                                                   # -0 == +0
    b.view(np.uint32)[4] = 0x7FA5A5A5                            # another NaN payload
    assert HI.same_numbers(a, b) and not HI.same_bits(a, b)
    b[0] = np.nextafter(F32(1), F32(2))
    assert not HI.same_numbers(a, b)
    assert not HI.same_numbers(a, a[:-1])
    base = dict(disps=[np.ones((2, 1, 3, 4), F32)], poses=[np.zeros((2, 6), F32)], B=2)
    d = HI.corrupt(base, ("disps", 0), (0, 0, 1, 2), NAN)
    assert np.isnan(d["disps"][0][0, 0, 1, 2]) and np.isnan(d["disps"][0]).sum() == 1
    assert (base["disps"][0] == 1).all(), "the clean input is never modified"
    assert HI.same_bits(d["disps"][0][1], base["disps"][0][1]) and HI.same_bits(d["poses"][0], base["poses"][0])
    with pytest.raises(AssertionError):
        HI.corrupt(base, ("disps", 0), (1, 0, 1, 2), NAN)        # sample 1 is never touched
    s = HI.stack2(dict(a=np.arange(6, dtype=F32).reshape(1, 6), l=[np.ones((1, 2), F32)], B=1, fmt="euler"))
    assert s["B"] == 2 and s["a"].shape == (2, 6) and (s["a"][0] == s["a"][1]).all() and s["l"][0].shape == (2, 2) and s["fmt"] == "euler"


def test_every_case_touches_sample_0_only():
    for h in HI.CATALOGUE + HI.EXTREME_FINITE:
        clean, d = HI.BASES[h.group](h.base), HI.inputs_of(h)
        changed = 0
        for key, v in clean.items():
            for a, b in zip(v if isinstance(v, list) else [v], d[key] if isinstance(v, list) else [d[key]]):
                if isinstance(a, np.ndarray):
                    assert a.shape[0] == 2, (HI.hid(h), key, "B >= 2: one sample stays clean")
                    assert HI.same_bits(a[1], b[1]), (HI.hid(h), key)
                    changed += int((a[0].view(np.int32) != b[0].view(np.int32)).sum())
        want = 1 if isinstance(h.where, tuple) else len(h.where)
        assert changed == want, (HI.hid(h), changed, want)


def test_the_catalogue_has_what_the_issue_lists():
    tags = {(h.group, h.tag) for h in HI.CATALOGUE}
    for group in ("warp", "loss"):
        got = {h.tag.split("_")[1] for h in HI.catalogue(group) if h.tag.startswith("disp_")}
        assert got == set(HI.DISP_VALUES), (group, got)
        for t in ("rot_nan", "rot_+inf", "rot_1e30", "trans_nan", "trans_+inf", "trans_1e30", "K_nan", "K_zero_row", "K_focal_0", "K_focal_1e30"):
            assert (group, t) in tags, (group, t)
    for base, (shape, _) in HI.WARP_BASES.items():
        P = shape[1] * shape[2]
        px = {h.per_pixel[1] for h in HI.catalogue("warp", base=base) if h.tag.startswith("disp_nan")}
        assert px == {0, 255, 256, P - 1} and P - 1 > 256 and (P - 1) % 256 != 255, "a seam between two blocks and a partial last block"
    for base, (shape, _) in HI.LOSS_BASES.items():
        W, S = shape[2], shape[4]
        px = {(h.per_pixel[0],) + divmod(h.per_pixel[1], W >> h.per_pixel[0]) for h in HI.catalogue("loss", base=base) if h.tag.startswith("disp_nan")}
        assert {(0, 3, 0), (0, 4, W - 1)} <= px and (S == 1 or any(s == S - 1 for s, _, _ in px)), px
    for group in ("sampler", "interp"):
        for base in HI.SAMPLER_BASES:
            mix = HI.catalogue(group, base=base, tag="grid_mix")[0]
            assert set(map(HI._name, mix.value.tolist())) == set(map(HI._name, HI.GRID_VALUES))
            oH, oW = HI.SAMPLER_BASES[base][4:]
            assert abs(len(mix.where) - 2 * oH * oW / 50.0) <= 1, "one entry in fifty"
    assert {"gy_nan", "gy_+inf"} <= {t for g, t in tags if g == "sampler"} and {"g_nan", "g_+inf", "g_op_nan", "g_op_+inf"} <= {t for g, t in tags if g == "warp"}
    assert max(HI.SAMPLER_BASES["C3"][1], 4) == 4 < HI.SAMPLER_BASES["C5"][1], "both sides of SAMPLER_BWD_MAXC"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the index restatement
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_c_clamp_is_not_np_clip():
    """THE difference this module turns on: np.clip keeps a NaN, the kernels' fminf(fmaxf(x, lo), hi) returns lo for it.  A
    restatement with np.clip would call NaN indices "never formed"; the kernels form index 0 from them."""
    x = np.array([NAN, -INF, INF, -3e9, 3e9, 2.5], F32)
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.clip(x, 0, 7)[0])
    assert HI.c_clamp(x, 0, 7).tolist() == [0.0, 0.0, 7.0, 0.0, 7.0, 2.5]
    assert HI.c_clamp(np.array([NAN], F32), -np.pi, np.pi)[0] == F32(-np.pi), "a NaN Euler angle is -pi"
    v, ok = HI.c_int(x)
    assert ok.tolist() == [False, False, False, False, False, True] and v[5] == 2, "(int) of NaN, infinities and |x| >= 2^31 is undefined"
    # the proxy that gives the ORACLE the kernels' clamp changes np.clip and nothing else
    with HI.c_clamps():
        assert O.np.clip(F32(NAN), 0, 7) == 0 and O.np.floor is np.floor
    with np.errstate(invalid="ignore"):
        assert O.np is np and np.isnan(O.np.clip(F32(NAN), 0, 7))


@pytest.mark.parametrize("base", sorted(HI.SAMPLER_BASES))
def test_the_restatement_is_the_oracle_on_clean_inputs(base):
    """on finite inputs pad_taps_c and interp_taps_c form the cells of oracle._sampler_coords / _interp_parts, and the warp's grid
    of ref_project_grid_c is oracle.cam2pixel's, bit for bit"""
    d = HI.sampler_base(base)
    _, C, H, W, oH, oW = HI.SAMPLER_BASES[base]
    u0, v0, ok = HI.pad_taps_c(d["grid"][:, 0].reshape(2, -1), d["grid"][:, 1].reshape(2, -1), H, W)
    _, _, w_u0, w_v0, _, _, _, _, _, _ = O._sampler_coords(d["grid"], H, W, F32)
    assert ok.all() and np.array_equal(u0, w_u0) and np.array_equal(v0, w_v0)
    got = HI.interp_taps_c(d["grid_px"][:, 0].reshape(-1), d["grid_px"][:, 1].reshape(-1), H, W)
    want = O._interp_parts(d["grid_px"], H, W, F32)[:4]
    assert got[4].all() and all(np.array_equal(a, b) for a, b in zip(got[:4], want))
    for name in HI.WARP_BASES:
        w = HI.warp_base(name)
        for h in HI.catalogue("warp", base=name)[:1]:
            grids = HI.sampler_grid_of(h, w)
        k = 0
        for s, disp in enumerate(w["disps"]):
            hh, ww = disp.shape[2:]
            for p in w["poses"]:
                gx, gy = HI.ref_project_grid_c(p, w["intrinsics"][:, s], (F32(1) / disp).reshape(2, -1), hh, ww)
                assert HI.same_bits(gx.reshape(-1), grids[k][0]) and HI.same_bits(gy.reshape(-1), grids[k][1]), (name, s)
                k += 1


def _assert_padded(u0, v0, ok, H, W, what):
    assert ok.all(), "%s: (int) applied to %d operands it is undefined for" % (what, int((~ok).sum()))
    assert u0.min() >= 0 and u0.max() <= W and v0.min() >= 0 and v0.max() <= H, \
        "%s: a top-left tap outside [0, W] x [0, H] of the padded image: u0 in [%d, %d], v0 in [%d, %d]" % (what, u0.min(), u0.max(), v0.min(), v0.max())


def _assert_inside(u0, v0, inview, ok, H, W, what):
    assert ok.all(), "%s: (int) applied to %d in-view operands it is undefined for" % (what, int((~ok).sum()))
    assert (u0 >= 0).all() and (u0 <= W - 2).all() and (v0 >= 0).all() and (v0 <= H - 2).all(), "%s: a tap outside the image" % what
    assert (u0[~inview] == 0).all() and (v0[~inview] == 0).all(), "%s: a lane that is not in view addresses pixel 0" % what


@pytest.mark.parametrize("h", HI.CATALOGUE + HI.EXTREME_FINITE, ids=HI.hid)
def test_no_index_leaves_the_image_or_its_zero_frame(h):
    """every index pad_taps, interp_taps, project_q and ref_proj_cell would form on this input, in float32 with C semantics"""
    d = HI.inputs_of(h)
    what = HI.hid(h)
    if h.group == "sampler":
        _, C, H, W, oH, oW = HI.SAMPLER_BASES[h.base]
        _assert_padded(*HI.pad_taps_c(d["grid"][:, 0], d["grid"][:, 1], H, W), H, W, what)
    elif h.group == "interp":
        _, C, H, W, oH, oW = HI.SAMPLER_BASES[h.base]
        u0, v0, u1, v1, ok = HI.interp_taps_c(d["grid_px"][:, 0], d["grid_px"][:, 1], H, W)
        assert ok.all(), what
        for a, n in ((u0, W), (u1, W), (v0, H), (v1, H)):
            assert a.min() >= 0 and a.max() <= n - 1, what
    else:
        B = d["disps"][0].shape[0]
        for s, disp in enumerate(d["disps"]):
            H, W = disp.shape[2:]
            K = d["intrinsics"][:, s]
            with np.errstate(all="ignore"):
                depth = (F32(1) / disp).reshape(B, -1)
            for i, p in enumerate(d["poses"]):
                tag = "%s scale %d source %d" % (what, s, i)
                gx, gy = HI.ref_project_grid_c(p, K, depth, H, W)
                # the reference-order paths: sfm_warp_*, sfm_warp_pyramid_*, sfm_warp_full_res_*, sfm_depth_consistency_*
                _assert_padded(*HI.pad_taps_c(gx, gy, H, W), H, W, tag + " pad_taps")
                if h.group == "loss":
                    _assert_inside(*HI.ref_cell_c(gx, gy, H, W), H, W, tag + " ref_proj_cell")
                    q = HI.fast_project_q_c(p, K, disp.reshape(B, -1), H, W)
                    _assert_inside(*HI.project_q_c(*q, H, W), H, W, tag + " project_q")
                elif s == 0:
                    # sfm_warp_fwd takes the DEPTH itself: the catalogue's disparity values written into the depth map
                    raw = HI.ref_project_grid_c(p, K, disp.reshape(B, -1), H, W)
                    _assert_padded(*HI.pad_taps_c(*raw, H, W), H, W, tag + " pad_taps on the value as a depth")


def test_the_restatement_would_catch_a_missing_clamp():
    """the assertions above are not vacuous: without pad_taps' clamp of the padded position the same inputs form indices far outside"""
    h = HI.catalogue("sampler", base="C3", tag="grid_mix")[0]
    d = HI.inputs_of(h)
    _, C, H, W, oH, oW = HI.SAMPLER_BASES["C3"]
    with np.errstate(all="ignore"):
        up = (d["grid"][:, 0] + F32(1)) * F32(W - 1) * F32(0.5) + F32(1)
    v, ok = HI.c_int(np.floor(up))
    assert not ok.all() and (np.abs(v) > W + 1).any()
    with pytest.raises(AssertionError):
        _assert_padded(v, v, ok, H, W, "no clamp")
    # ... and project_q's sign test rejects what a plain 0 < U comparison chain on a NaN would not have to
    q0 = np.array([NAN, INF, -INF, 3e9, 5.0], F32)
    u0, v0, inview, ok = HI.project_q_c(q0, np.full(5, 2.0, F32), np.ones(5, F32), 8, 12)
    assert inview.tolist() == [False, False, False, False, True] and ok.all() and u0.tolist() == [0, 0, 0, 0, 5]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the extreme but finite values
# ---------------------------------------------------------------------------------------------------------------------------
EXTREME_CONFIGS = ("ssim_smooth", "edge_aware", "explain_alpha")


def _loss(d, cfg, dtype, strict):
    mode = "raise" if strict else "ignore"
    with np.errstate(over=mode, invalid=mode, divide=mode):
        return O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True,
                          want_d_src=True, keep_warped=True, dtype=dtype, **cfg)


@pytest.mark.parametrize("h", HI.EXTREME_FINITE, ids=HI.hid)
def test_extreme_finite_values_stay_finite_and_clear_of_the_view_border(h):
    """(a) the float32 oracle raises no overflow, invalid-operation or division exception on the value, forward or backward, so it
    forms no non-finite intermediate; (b) float32 and float64 put the same pixels in view, and every pixel whose projection the
    value moved lies at least EXTREME_MARGIN from the strict in-view test in both.  Prints the margins."""
    d, clean = HI.inputs_of(h), HI.BASES[h.group](h.base)
    if h.group == "loss":
        for name in EXTREME_CONFIGS:
            r32 = _loss(d, CONFIGS[name], F32, strict=True)
            for key in ("d_disps", "d_poses", "d_srcs"):
                assert all(np.isfinite(a).all() for a in r32[key]), (name, key)
            assert all(np.isfinite(r32[k]) for k in ("total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss"))
        r64, c32 = _loss(d, CONFIGS["ssim_smooth"], F64, strict=False), _loss(clean, CONFIGS["ssim_smooth"], F32, strict=True)
        moved_any = False
        for s in range(len(d["disps"])):
            assert np.array_equal((r32["warped"][s] == 0).all(axis=2), (r64["warped"][s] == 0).all(axis=2)), "the in-view sets agree"
            moved = (r32["uv"][s] != c32["uv"][s]).any(axis=2)
            assert not moved[1].any(), "sample 1 is clean"
            if moved.any():
                moved_any = True
                m = min(float(r32["margin"][s][moved].min()), float(r64["margin"][s][moved].min()))
                print("%s scale %d: %d projections moved, smallest margin %.3g" % (HI.hid(h), s, int(moved.sum()), m))
                assert m >= HI.EXTREME_MARGIN, (s, m)
        assert moved_any, "the value changes some projection"
        # ... and the criteria of tests/test_loss_gpu.py can be applied at all: the float32 oracle is a yardstick (within
        # knife_free.YARDSTICK_MAX of the float64 one in every gradient array) and the knife classes stay below their cap
        cfg = CONFIGS["ssim_smooth"]
        for name, y in KF.yardsticks(r64, _loss(d, cfg, F32, strict=True), dict(cfg)):
            assert y <= KF.YARDSTICK_MAX, (name, y)
        for s in range(len(d["disps"])):
            _knife(r32, s, len(d["poses"]))
    else:
        source = h.what[1]
        for rows, C in R.OPERATOR_FORMS:
            with np.errstate(over="raise", invalid="raise", divide="raise"):
                r32 = R.operator_reference(d, F32, rows, C, source)
            r64, c32 = R.operator_reference(d, F64, rows, C, source), R.operator_reference(clean, F32, rows, C, source)
            assert all(np.isfinite(r32[k]).all() for k in R.OPERATOR_ARRAYS)
            assert np.array_equal(r32["valid"], r64["valid"])
            m = min(float(r32["margin"][0].min()), float(r64["margin"][0].min()))
            print("%s rows %d: smallest margin of sample 0 %.3g" % (HI.hid(h), rows, m))
            assert m >= HI.EXTREME_MARGIN and not np.array_equal(r32["warped"][0], c32["warped"][0])
            assert HI.same_bits(r32["warped"][1], c32["warped"][1])


REPLACED = [      # (base, what, where, value, which condition it fails): why EXTREME_FINITE does not hold the issue's own value
    ("32x48", ("disps", 0), (0, 0, 4, 24), 1e30, "exception"), ("32x48", ("disps", 0), (0, 0, 3, 0), 1e-30, "exception"),
    ("37x70", "intrinsics", (0, 0, 0, 0), 1e30, "margin"), ("32x48", ("poses", 0), (0, 1), 1e30, "margin"), ("37x70", ("poses", 0), (0, 1), 1e30, "margin"),
    ("37x70", ("disps", 0), (0, 0, 3, 0), 1e-15, "yardstick"), ("32x48", ("disps", 0), (0, 0, 4, 24), 1e-15, "yardstick"),
    ("37x70", ("poses", 1), (0, 5), 1e30, "knife"),
]


@pytest.mark.parametrize("base,what,where,value,fails", REPLACED, ids=lambda v: str(v).replace(" ", ""))
def test_the_replaced_values_do_fail_their_condition(base, what, where, value, fails):
    """a value is replaced because it FAILS a condition, not because it is inconvenient: each replaced value, on the same inputs"""
    d, clean = HI.corrupt(HI.loss_base(base), what, where, value), HI.loss_base(base)
    cfg = CONFIGS["ssim_smooth"]
    if fails == "exception":
        with pytest.raises(FloatingPointError):
            _loss(d, cfg, F32, strict=True)
    elif fails == "yardstick":
        r32, r64 = _loss(d, cfg, F32, strict=False), _loss(d, cfg, F64, strict=False)
        assert max(y for _, y in KF.yardsticks(r64, r32, dict(cfg))) > 100 * KF.YARDSTICK_MAX
    elif fails == "knife":
        with pytest.raises(AssertionError, match="too many knife-edge pixels"):
            _knife(_loss(d, cfg, F32, strict=True), 0, 2)
    else:
        r32, c32 = _loss(d, cfg, F32, strict=True), _loss(clean, cfg, F32, strict=True)
        m = min(float(r32["margin"][s][(r32["uv"][s] != c32["uv"][s]).any(axis=2)].min()) for s in range(len(d["disps"]))
                if (r32["uv"][s] != c32["uv"][s]).any())
        assert m < HI.EXTREME_MARGIN, m


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the deviation table
# ---------------------------------------------------------------------------------------------------------------------------
def _statement_classes(h, d, c):
    """{output name: classes} of the case's float32 statement, forward outputs (and the samplers' backward); None where the
    reference cannot be evaluated at all (the interp sampler on a NaN position)"""
    if h.group == "sampler":
        return {k: HI.classes(v) for k, v in HI.sampler_statement(d, c).items()}
    if h.group == "interp":
        try:
            return {k: HI.classes(v) for k, v in HI.interp_statement(d, c).items()}
        except ValueError:
            return None
    if h.group == "warp":
        out = HI.warp_pyramid_statement(d, c, backward=False)
        return {"%s[%d]" % (k, s): HI.classes(a) for k, v in out.items() for s, a in enumerate(v)}
    res = HI.loss_statement(d, CONFIGS["ssim_smooth"], c, backward=False)
    out = {"warped[%d]" % s: HI.classes(a) for s, a in enumerate(res["warped"])}
    out.update({k: HI.classes(np.float64(res[k])) for k in ("total_loss", "pixel_loss", "smooth_loss", "ssim_loss")})
    return out


_hit = {}


@pytest.mark.parametrize("h", HI.CATALOGUE, ids=HI.hid)
def test_the_statements_deviate_from_the_kernels_clamps_only_where_the_table_says(h):
    """the float32 statement with np.clip and the same statement with fminf(fmaxf(.)) give the same classes on this case unless an
    entry of DEVIATIONS applies to it -- and where one applies, they do differ (the entry is not a blanket excuse)"""
    d = HI.inputs_of(h)
    names = HI.deviations_of(h, d)
    plain, clamped = _statement_classes(h, d, False), _statement_classes(h, d, True)
    assert clamped is not None
    differ = plain is None or any(not np.array_equal(plain[k], clamped[k]) for k in clamped)
    assert differ == bool(names), "%s: statements %s, table says %s" % (HI.hid(h), "differ" if differ else "agree", names or "no deviation")
    for n in names:
        _hit.setdefault(n, []).append(HI.hid(h))
    if h.group == "warp" and h.what != ("g", 0):      # ... and sfm_warp_*'s own statement (one source, the value written as a DEPTH)
        for rows in (1, 3):
            a = HI.operator_arrays(h, rows, 3)
            plain, clamped = HI.warp_operator_statement(a), HI.warp_operator_statement(a, c=True)
            differ = any(not np.array_equal(HI.classes(plain[k]), HI.classes(clamped[k])) for k in plain if k != "grid")
            assert differ == bool(HI.operator_deviations_of(h, a)), (HI.hid(h), rows)


def test_every_deviation_is_hit_and_documented():
    """(runs after the parametrised test above in file order) every entry of DEVIATIONS applies to some catalogue case, and its line
    stands in the header it names"""
    if not _hit:      # run on its own: fill the record
        for h in HI.CATALOGUE:
            for n in HI.deviations_of(h):
                _hit.setdefault(n, []).append(HI.hid(h))
    for name, e in HI.DEVIATIONS.items():
        text = " ".join(open(os.path.join(ROOT, e["header"])).read().replace(" * ", " ").split())
        assert e["line"] in text, "%s does not say: %s" % (e["header"], e["line"])
        if e.get("scope") == "gpu":      # pinned by tests/test_hostile_inputs_gpu.py, which must name it
            assert 'HI.DEVIATIONS["%s"]' % name in open(os.path.join(ROOT, "tests", "test_hostile_inputs_gpu.py")).read(), \
                "%s is not looked up by the GPU module" % name
            continue
        assert _hit.get(name), "no catalogue case deviates as %r" % name
        groups = {c.split("-")[0] for c in _hit[name]}
        print("%s: %d cases (%s)" % (name, len(_hit[name]), ", ".join(sorted(groups))))
