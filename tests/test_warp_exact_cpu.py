"""tests/warp_exact_ref.py without a GPU: the proof that tests/test_warp_exact_gpu.py may compare every element of every output of
the image warps with float64, and that doing so is not vacuous.

  a. every listed case is knife-free in both precisions: no pair within reach of the strict in-view test or of a cell boundary of
     the bilinear lattice, the same `valid` in float32 and float64, a valid share inside VALID_SHARE for every (scale, source),
     every yardstick max|o32 - o64| / max|o64| positive and at most YARDSTICK_MAX (the numbers are depth_consistency_ref's own);
  b. the two float64 statements -- NumPy on the oracle's pieces with a hand-derived backward, torch autograd through grid_sample --
     agree within 1e-9 of each array's maximum, d_T (all 12 entries) included;
  c. the rule has teeth: four planted errors in the float32 reference, each accepted by the criteria the suite had for the warps
     (2e-3 of the array's maximum; d_pose 2e-3 element-wise and 1e-3 in L2; d_T seen only through pose_mat_bwd) and rejected by
     knife_free.rule with k = 4;
  d. nothing is hidden: the masks are all-False."""
import numpy as np
import pytest

import pose_conv_ref as PR
import warp_exact_ref as R
from knife_free import allowance, rule
from util import assert_close_masked

F32, F64 = np.float32, np.float64
TEETH = ((1, 24, 40, 3, 3), 6, "default")       # Euler, not inverted, three sources, three scales
OPERATOR_CASES = [(c, rows, C, i) for c in R.CASE_LIST for rows, C in R.OPERATOR_FORMS for i in range(c[0][3])]
OPERATOR_CASES += [(R.OPERATOR_C5_CASE, rows, 5, 0) for rows in (1, 3)]


def op_ident(v):
    c, rows, C, i = v
    return "%s-rows%d-C%d-src%d" % (R.ident(c), rows, C, i)


# ------------------------------------------------------------------------------------------------------------------------
# a. knife-free
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.ident)
def test_the_cases_are_knife_free(case):
    shape, seed, setting = case
    assert sum(a.size for a in R.inputs(*case)["disps"]) * shape[3] <= 4000, "a knife-free case has about 3,000 pixel-source pairs at the most"
    assert R.failed_conditions(*case) == []
    o64, o32 = R.references(*case)
    for o in (o64, o32):
        assert not any(m.any() for m in R.knife_of(o))
    for s, v in enumerate(o64["valid"]):
        assert np.array_equal(v, o32["valid"][s])
        for i in range(v.shape[1]):
            assert R.VALID_SHARE[0] <= v[:, i].mean() <= R.VALID_SHARE[1], (s, i)
        # the zero set of the warped image is the complement of valid, in both precisions
        for o in (o64, o32):
            assert np.array_equal((o["warped"][s] == 0).all(axis=2), o["valid"][s] == 0), s
    for name, y in R.yardsticks(o64, o32):
        print("%s: max|o32 - o64| / max|o64| = %.3g" % (name, y))
        assert 0 < y <= R.YARDSTICK_MAX, name


@pytest.mark.parametrize("v", OPERATOR_CASES, ids=op_ident)
def test_the_operator_forms_are_knife_free(v):
    """one and three depth rows (the three rows scaled by factors in (0.98, 1.02), which moves the samples), three and five channels"""
    (shape, seed, _), rows, C, i = v
    o64, o32 = R.operator_references(shape, seed, rows, C, i)
    assert not (R.operator_knife_of(o64) | R.operator_knife_of(o32)).any()
    assert np.array_equal(o64["valid"], o32["valid"]) and R.VALID_SHARE[0] <= o64["valid"].mean() <= R.VALID_SHARE[1]
    for o in (o64, o32):
        assert np.array_equal((o["warped"] == 0).all(axis=1), o["valid"] == 0)
    assert o64["d_depth"].shape == (shape[0], rows, shape[1], shape[2]) and o64["d_src"].shape == (shape[0], C, shape[1], shape[2])
    for name, y in R.yardsticks(o64, o32, keys=R.OPERATOR_ARRAYS):
        print("%s: max|o32 - o64| / max|o64| = %.3g" % (name, y))
        assert 0 < y <= R.YARDSTICK_MAX, name
    if rows == 1 and C == 3:      # in float32, where 1 / disp is the same number on both sides, the operator's one-row form IS one
        m32 = R.references(shape, seed, "default")[1]      # (scale, source) of the multi-scale reference at scale 0
        assert np.array_equal(o32["warped"], m32["warped"][0][:, i]) and np.array_equal(o32["valid"], m32["valid"][0][:, i])


def test_search_finds_the_seeds():
    shape = (2, 13, 21, 2, 1)
    assert tuple(R.search(shape, "conv", 0, 3)) == R.CONV_CASES[shape]
    assert R.failed_conditions(shape, 0, "conv") != [], "seed 0 is not knife-free under the conventions: the conditions do reject"
    assert R.search_rows(shape, 1, 5) == [R.ROWS_DRAWS[(shape, 1)]], "the depth-row draw is the first that search_rows finds"
    assert R.CASES is R.DR.CASES, "the default cases ARE the geometry-consistency term's: one proof, two consumers"
    for case in R.MATRIX_CASE_LIST:      # the matrices are not rigid: R R^T is not the identity by far more than float32 rounding
        for T in R.inputs(*case)["poses"]:
            RRt = np.einsum("nij,nkj->nik", T[:, :, :3].astype(F64), T[:, :, :3].astype(F64))
            assert np.abs(RRt - np.eye(3)).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------------------
# b. two opinions
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.ident)
def test_the_two_float64_statements_agree(case):
    o64, _ = R.references(*case)
    t = R.torch_opinion(R.inputs(*case))
    for key in R.ARRAYS:
        assert len(o64[key]) == len(t[key])
        for k, (a, b) in enumerate(zip(o64[key], t[key])):
            top, err = np.abs(a).max(), np.abs(a - b).max()
            print("%s[%d]: max|numpy64 - torch64| = %.3g of max %.3g" % (key, k, err, top))
            assert a.shape == b.shape and top > 0 and err <= 1e-9 * top, (key, k)
    if case[2] == "matrix":
        assert all(a.shape == (case[0][0], 3, 4) and a is b for a, b in zip(o64["d_T"], o64["d_poses"])), "under 'matrix' d_pose IS d_T"


def test_the_euler_reference_is_the_oracles_backward():
    """on the default conventions the few lines of `reference` that the oracle does not have change nothing: d_pose through
    pose_matrix_grad is oracle.proj_tgt_to_src_backward's within float64 rounding, warped and d_disp are the oracle's bit for bit"""
    d = R.inputs(*TEETH)
    o64, _ = R.references(*TEETH)
    B = d["B"]
    for i in range(d["n_src"]):
        g_pose = 0
        for s in range(d["n_scales"]):
            h, w = d["disps"][s].shape[2:]
            depthes = np.broadcast_to((1 / d["disps"][s].astype(F64)).reshape(B, 1, h * w), (B, 3, h * w))
            args = (d["src_pyr"][s][:, 3 * i:3 * i + 3], depthes, d["poses"][i], d["intrinsics"][:, s])
            assert np.array_equal(R.O.projective_inverse_warp(*args, F64), o64["warped"][s][:, i])
            g_pose = g_pose + R.O.projective_inverse_warp_backward(*args, d["g"][s][:, i], F64)[1]
        assert np.abs(g_pose - o64["d_poses"][i]).max() <= 1e-12 * np.abs(g_pose).max()


# ------------------------------------------------------------------------------------------------------------------------
# c. the rule has teeth
# ------------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, F64) - b) / np.linalg.norm(b))


def _old_accepts(o32, got):
    """the criteria the suite had: d_disp element-wise at 2e-3 of the array's maximum, d_pose at 2e-3 element-wise and 1e-3 in L2,
    both against the float32 statement; d_T only through the pose operator's backward"""
    for s, a in enumerate(got["d_disps"]):
        assert_close_masked(a, o32["d_disps"][s], 2e-3, None, what="d_disp[%d]" % s)
    for i, a in enumerate(got["d_poses"]):
        assert np.abs(a - o32["d_poses"][i]).max() <= 2e-3 * np.abs(o32["d_poses"][i]).max() and _rel_l2(a, o32["d_poses"][i]) <= 1e-3
    return True


def _new_rejects(o64, o32, got, key, k):
    with pytest.raises(AssertionError, match="knife-free"):
        rule(got[key][k], o64[key][k], o32[key][k], "planted %s[%d]" % (key, k), k=4)
    return True


def _planted(o32, **changed):
    return dict(o32, **changed)


def test_a_scaled_d_disp_is_rejected():
    o64, o32 = R.references(*TEETH)
    got = _planted(o32, d_disps=[(a * F32(1 + 1e-3)).astype(F32) for a in o32["d_disps"]])
    assert _old_accepts(o32, got)
    assert all(_new_rejects(o64, o32, got, "d_disps", s) for s in range(len(got["d_disps"])))


def test_a_dropped_source_is_rejected():
    """One source's share of d_disp left out at ten pixels.  At the ten pixels where d_disp is largest the share is 0.3 .. 0.8 of
    the array's maximum and the 2e-3 criterion sees it; the plant takes the ten largest shares that criterion cannot see: those
    below 1.9e-3 of the maximum."""
    o64, o32 = R.references(*TEETH)
    dd, parts = o32["d_disps"][0], o32["d_disp_parts"][0]
    top = np.abs(dd).max()
    worst = np.argsort(-np.abs(dd).ravel())[:10]
    assert all(np.abs(parts[:, i].ravel()[worst]).max() > 0.1 * top for i in range(parts.shape[1])), "at the largest pixels: visible at 2e-3"
    share = np.abs(parts[:, 1]).ravel()
    share = np.where(share <= 1.9e-3 * top, share, 0)
    ten = np.argsort(-share)[:10]
    assert share[ten].min() > 0, "ten pixels with a share of source 1 that is not zero"
    bad = dd.copy()
    bad.reshape(-1)[ten] -= parts[:, 1].ravel()[ten]
    got = _planted(o32, d_disps=[bad] + o32["d_disps"][1:])
    print("dropped shares: %.3g .. %.3g of max|d_disp|, the rule grants %.3g" % (share[ten].min() / top, share[ten].max() / top,
                                                                               allowance(o64["d_disps"][0], dd, 4) / top))
    assert _old_accepts(o32, got) and _new_rejects(o64, o32, got, "d_disps", 0)


SWAP = ("swap_wy", 0, 1, 0, 237)      # scale 0, source 1, sample 0, pixel (5, 37): in view, and its d_disp moves by 1.7e-3 of the maximum


def test_swapped_row_weights_at_one_pixel_are_rejected():
    """gu of one in-view pixel with wy0 and wy1 swapped: d_disp of that pixel moves by some 1e-3 of the array's maximum, d_T by that
    one pixel's share of a sum over all of them"""
    o64, o32 = R.references(*TEETH)
    _, s, i, b, p = SWAP
    assert o64["valid"][s].reshape(1, 3, -1)[b, i, p] == 1
    got = R.reference(R.inputs(*TEETH), F32, plant=SWAP)
    moved = np.abs(got["d_disps"][s] - o32["d_disps"][s]).ravel()
    assert (moved > 0).sum() == 1 and moved[p] > 0, "one pixel of d_disp, and the sums of d_T"
    print("swapped weights: d_disp of the pixel moves by %.3g of max|d_disp|" % (moved[p] / np.abs(o32["d_disps"][s]).max()))
    assert not np.array_equal(got["d_T"][i], o32["d_T"][i]) and np.array_equal(got["d_T"][0], o32["d_T"][0])
    assert _old_accepts(o32, got) and _new_rejects(o64, o32, got, "d_disps", s)


def test_a_d_T_error_off_the_rigid_tangent_space_is_rejected():
    """d_T + eps max|d_T| (S . R) in the rotation block, S symmetric: for T = [R|t] every rigid tangent is [w]x R, and
    <S R, [w]x R> = tr(S [w]x) = 0.  pose_matrix_grad, which is all the suite saw of d_T, does not move; the rule on d_T does."""
    o64, o32 = R.references(*TEETH)
    d = R.inputs(*TEETH)
    assert d["fmt"] == "euler" and not any(d["invert"])
    rng = np.random.RandomState(11)
    for i, a in enumerate(o32["d_T"]):
        S = rng.standard_normal((3, 3))
        S = S + S.T
        Rm = PR.pose_matrix(d["poses"][i], "euler", False, F64)[:, :, :3]
        bad = a.astype(F64).copy()
        bad[:, :, :3] += 1e-3 * np.abs(a).max() * np.einsum("ij,njk->nik", S, Rm)
        before = PR.pose_matrix_grad(d["poses"][i], "euler", False, a.astype(F64))
        after = PR.pose_matrix_grad(d["poses"][i], "euler", False, bad)
        print("d_T[%d]: d_pose moves by %.3g of its maximum" % (i, np.abs(after - before).max() / np.abs(before).max()))
        assert np.abs(after - before).max() <= 1e-9 * np.abs(before).max(), "invisible through the pose operator's backward"
        got = _planted(o32, d_T=[bad.astype(F32) if k == i else t for k, t in enumerate(o32["d_T"])])
        assert _old_accepts(o32, got) and _new_rejects(o64, o32, got, "d_T", i)
        with pytest.raises(AssertionError, match="knife-free"):      # ... and on the rotation block alone
            rule(bad[:, :, :3], o64["d_T"][i][:, :, :3], a[:, :, :3], "planted rotation block of d_T[%d]" % i, k=4)


def test_the_unplanted_reference_passes_both():
    o64, o32 = R.references(*TEETH)
    assert _old_accepts(o32, o32)
    for key in R.ARRAYS:
        for k in range(len(o32[key])):
            assert rule(o32[key][k], o64[key][k], o32[key][k], "%s[%d]" % (key, k), k=4) == 1.0


# ------------------------------------------------------------------------------------------------------------------------
# d. nothing is hidden
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.ident)
def test_no_case_excludes_an_element(case):
    marks = R.knife(R.inputs(*case), R.references(*case))
    assert len(marks) == case[0][4] and all(m.dtype == bool and m.shape == v.shape and not m.any()
                                            for m, v in zip(marks, R.references(*case)[0]["valid"]))
    if case in R.CASE_LIST:
        shape, seed, _ = case
        for rows, C in R.OPERATOR_FORMS:
            for i in range(shape[3]):
                o64, o32 = R.operator_references(shape, seed, rows, C, i)
                assert not (R.operator_knife_of(o64) | R.operator_knife_of(o32)).any()
