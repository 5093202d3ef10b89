"""What tests/test_intrinsics_exact_gpu.py relies on, proved WITHOUT a GPU from the references of tests/intrinsics_exact_ref.py:

  1. the cases are knife-free by conditions 1-4 of tests/test_knife_free_cpu.py, in float64 and in float32, under each of the four
     configurations -- the yardstick condition max|o32 - o64| <= 1e-4 max|o64| for every block of d_proj and d_K;
  2. the inputs are knife_free's inputs with the cameras replaced by general ones and nothing else changed;
  3. the two float64 statements -- the NumPy oracle with the closed form, torch autograd with K a leaf -- agree to 1e-9 of every
     block's maximum;
  4. the sampler's gradient with its weights swapped is INVISIBLE to the ramp criterion of tests/test_intrinsics_grad_gpu.py (1e-3
     per entry in mode l1) and fails the new rule on every textured case, under K_REF = 4 and under every committed factor; so do a
     loss weight off by a per mille and a d_K that lacks its K^-1 route for one source at the last scale;
  5. the committed factors follow from the committed measurements by the stated rule;
  6. the operator's cases: the closed form on the oracle's gPm agrees with autograd to 1e-9, the general-camera cases are
     knife-free by warp_exact_ref's own conditions and are what its search finds.
"""
import numpy as np
import pytest

import cameras
import intrinsics_exact_ref as X
import intrinsics_grad as IG
import knife_free as KF
import warp_exact_ref as R
from oracle import sfm_oracle as O

F32, F64 = np.float32, np.float64
AGREE = 1e-9
RAMP_TOL = 1e-3      # tests/test_intrinsics_grad_gpu.py::REF_TOL

cases = pytest.mark.parametrize("case", X.CASE_LIST, ids=X.case_id)
configs = pytest.mark.parametrize("cfg_name", sorted(X.CONFIGS))


def test_the_cases_are_the_shapes_the_kernels_can_go_wrong_at():
    """two seeds per shape; more than one strip, a ragged last strip, an odd height, three scales, two samples, an odd source count
    and a plan above 64 tiles all occur; every frame has at most 5200 pixels"""
    assert all(len(seeds) == 2 and len(set(seeds)) == 2 for seeds in X.CASES.values())
    shapes = list(X.CASES)
    assert any(W > 128 for _, _, W, _, _ in shapes) and any(64 < W < 128 and W % 64 for _, _, W, _, _ in shapes) and any(W <= 64 for _, _, W, _, _ in shapes)
    assert any(H % 2 and H % 4 for _, H, _, _, _ in shapes)
    assert any(S >= 3 for *_, S in shapes) and any(B > 1 for B, *_ in shapes) and any(n % 2 for _, _, _, n, _ in shapes)
    assert all(H * W <= 5200 for _, H, W, _, _ in shapes)
    assert set(KF.CASES) < set(shapes) and X.FOLD_SHAPE in shapes
    tiles = {shape: IG.host_plan(shape, "ssim_smooth")[0] for shape in shapes}
    assert tiles[X.FOLD_SHAPE] == X.FOLD_TILES and max(X.FOLD_TILES) > 64 and all(max(t) <= 64 for s, t in tiles.items() if s != X.FOLD_SHAPE), tiles
    assert X.CONFIGS is IG.CONFIGS and len(X.CONFIGS) == 4


@cases
def test_the_inputs_are_the_knife_free_inputs_under_general_cameras(case):
    shape, seed = case
    d, base = X.inputs(shape, seed), KF.make_inputs(shape, seed)
    assert set(d) == set(base)
    for key in base:
        if key == "intrinsics":
            continue
        a, b = d[key], base[key]
        assert all(np.array_equal(p, q) for p, q in zip(a, b)) if isinstance(b, list) else np.array_equal(a, b), key
    K, K0 = d["intrinsics"], base["intrinsics"]
    assert K.dtype == F32 and np.array_equal(K, cameras.cameras(base, "general", 1000 + seed))
    assert (K[:, :, 0, 1] != 0).all() and (K[:, :, 1, 0] != 0).all() and (K[:, :, 2, :2] != 0).all() and (K[:, :, 2, 2] != 1).all()
    assert (K0[:, :, 0, 1] == 0).all() and (K0[:, :, 2, :2] == 0).all()
    for name in cameras.ABLATIONS:        # every shortcut through K changes this K (with one scale there is none to rebuild)
        assert not np.array_equal(cameras.ABLATIONS[name](K), K) or (shape[4] == 1 and name == "scales rebuilt from scale 0"), name


def test_want_d_proj_adds_d_proj_and_changes_nothing_else():
    case = X.CASE_LIST[2]
    d, cfg = X.inputs(*case), X.CONFIGS["ssim_smooth"]
    args = (d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"])
    for dtype in (F64, F32):
        plain = O.sfm_loss(*args, backward=True, dtype=dtype, **cfg)
        full = O.sfm_loss(*args, backward=True, dtype=dtype, want_d_proj=True, **cfg)
        assert set(full) == set(plain) | {"d_proj"} and "d_proj" not in O.sfm_loss(*args, dtype=dtype, want_d_proj=True, **cfg)
        for key in plain:
            a, b = plain[key], full[key]
            if isinstance(a, list):
                assert all(np.array_equal(p, q) for p, q in zip(a, b)), key
            else:
                assert a is b is None or a == b, key
        B, S, n = case[0][0], case[0][4], case[0][3]
        assert full["d_proj"].shape == (B, S, n, 3, 4) and full["d_proj"].dtype == dtype
        for i in range(n):      # folded through the oracle's own backward of proj_tgt_to_src it is the d_pose the oracle returns
            g = np.zeros((B, S, 4, 4), dtype)
            g[:, :, :3] = full["d_proj"][:, :, i]
            folded = sum(O.proj_tgt_to_src_backward(d["poses"][i], d["intrinsics"][:, s], g[:, s], dtype) for s in range(S))
            assert np.abs(folded - full["d_poses"][i]).max() <= (1e-12 if dtype is F64 else 1e-4) * np.abs(full["d_poses"][i]).max()


@configs
@cases
def test_no_knife_pixel_and_the_masked_branch_is_present(case, cfg_name):
    d = X.inputs(*case)
    for r, which in zip(X.references(*case, cfg_name), ("fp64", "fp32")):
        found = KF.knife_pixels(d, r["res"])
        assert not any(found.values()), "%s oracle: %s" % (which, found)
        for s, share in enumerate(KF.masked_shares(r["res"])):
            assert KF.MASKED_SHARE[0] <= share <= KF.MASKED_SHARE[1], (which, s, share)


@cases
def test_no_smoothness_stencil_near_its_kink(case):
    d = X.inputs(*case)
    for mode in ("second_order", "edge_aware"):
        for dtype in (F64, F32):
            assert KF.smooth_kink_margin(d, mode, dtype) >= KF.SMOOTH_KINK_MIN, (mode, dtype.__name__)


@configs
@cases
def test_the_yardstick_of_every_block_is_not_vacuous(case, cfg_name):
    ys = X.yardsticks(*X.references(*case, cfg_name))
    print("yardsticks %s %s: %s" % (X.case_id(case), cfg_name, ", ".join("%s %.2e" % y for y in ys)))
    assert len(ys) == case[0][4] * len(X.KINDS) and all(0 < y <= X.YARDSTICK_MAX for _, y in ys), [y for y in ys if not 0 < y[1] <= X.YARDSTICK_MAX]


@configs
@cases
def test_the_two_float64_statements_agree(case, cfg_name):
    r64, _ = X.references(*case, cfg_name)
    second = X.second_opinion(*case, cfg_name)
    worst = 0.0
    for _, name, got, a64, _ in X.rows(second["d_proj"], second["d_K"], r64, r64):
        err, _, top = KF.distances(got, a64, a64)
        worst = max(worst, err / top)
        assert err <= AGREE * top, (name, err / top)
    print("the two float64 statements %s %s: %.3g of a block's maximum at the most" % (X.case_id(case), cfg_name, worst))


@pytest.mark.parametrize("shape", list(X.CASES), ids=lambda s: "x".join(map(str, s)))
def test_swapped_sampler_weights_pass_the_ramp_criterion(shape):
    """on intrinsics_grad.ramp_inputs of the same shape, mode l1, the plant stays inside 1e-3 per entry (intrinsics_grad.worst /
    proj_entry_errors): the existing end-to-end tests cannot see the bilinear sampler's gradient"""
    d, cfg = IG.ramp_inputs(shape, X.KIND), X.CONFIGS["l1"]
    ref, bad = X.statement(d, cfg, F64), X.plant_swapped_weights(d, cfg)
    e_k, e_p = IG.worst(bad["d_K"], ref["d_K"]), float(IG.proj_entry_errors(bad["d_proj"], ref["d_proj"]).max())
    print("swapped sampler weights on ramps %s: worst entry of d_K moves by %.3g, of d_proj by %.3g" % (shape, e_k, e_p))
    assert 0 < e_k <= RAMP_TOL and 0 < e_p <= RAMP_TOL, (e_k, e_p)


def caught(plant, r64, r32, what):
    """the plant misses the rule in at least one block under every set of factors"""
    rows = X.rows(plant["d_proj"], plant["d_K"], r64, r32)
    for name, k_of in X.factor_sets().items():
        assert set(k_of) <= set(X.KINDS) and k_of, name
        out = X.outside(rows, k_of)
        assert out, "%s passes the rule under %s" % (what, name)
        print("%s under %s: outside in %d rows, the furthest %s at %.3g allowances" % ((what, name, len(out)) + max(out, key=lambda o: o[1])))


@configs
@cases
def test_swapped_sampler_weights_fail_the_rule(case, cfg_name):
    r64, r32 = X.references(*case, cfg_name)
    caught(X.plant_swapped_weights(X.inputs(*case), X.CONFIGS[cfg_name]), r64, r32, "swapped sampler weights %s %s" % (X.case_id(case), cfg_name))
    assert O.spatial_transformer_sampler_backward.__module__ == O.__name__      # the oracle is itself again


@pytest.mark.parametrize("cfg_name", sorted(name for name, cfg in X.CONFIGS.items() if cfg.get(X.PLANT_WEIGHT)))
@cases
def test_a_weight_off_by_a_per_mille_fails_the_rule(case, cfg_name):
    """ssim_rate is the one loss weight that reaches d_proj: smooth_reg and exp_reg move d_disp and d_mask only (asserted)"""
    d, cfg = X.inputs(*case), X.CONFIGS[cfg_name]
    r64, r32 = X.references(*case, cfg_name)
    caught(X.plant_weight(d, cfg), r64, r32, "%s x 1.001 %s %s" % (X.PLANT_WEIGHT, X.case_id(case), cfg_name))
    other = X.statement(d, cfg, F64, smooth_reg=cfg["smooth_reg"] * 1.001)
    assert np.array_equal(other["d_proj"], r64["d_proj"])


def test_the_other_weights_do_not_reach_d_proj():
    case = X.CASE_LIST[0]
    d, cfg = X.inputs(*case), X.CONFIGS["explain"]
    assert X.plant_weight(d, cfg) is None and X.plant_weight(d, X.CONFIGS["l1"]) is None
    r64, _ = X.references(*case, "explain")
    for weight in ("smooth_reg", "exp_reg"):
        assert np.array_equal(X.statement(d, cfg, F64, **{weight: cfg[weight] * 1.001})["d_proj"], r64["d_proj"]), weight


@configs
@cases
def test_d_K_without_its_inverse_route_fails_the_rule(case, cfg_name):
    d = X.inputs(*case)
    r64, r32 = X.references(*case, cfg_name)
    for source in (0, case[0][3] - 1):
        bad = X.plant_no_inverse_route(d, r64, source)
        assert np.array_equal(bad["d_K"][:, :-1], r64["d_K"][:, :-1]) and bad["d_proj"] is r64["d_proj"]
        caught(bad, r64, r32, "d_K without the K^-1 route of source %d at the last scale, %s %s" % (source, X.case_id(case), cfg_name))


def test_the_closed_form_without_a_route_is_what_the_plant_says():
    """the plant is the closed form with one term left out: with every source's term left out at every scale it is the
    proj_tgt_to_src route alone (intrinsics_grad.d_k_of_proj)"""
    case = X.CASE_LIST[2]
    d = X.inputs(*case)
    r64, _ = X.references(*case, "l1")
    S, n = case[0][4], case[0][3]
    g = np.zeros((case[0][0], 4, 4))
    g[:, :3] = r64["d_proj"][:, S - 1, 0]
    only = IG.d_k_of_proj(d["poses"][0], g)
    full = IG.d_k_from_d_proj(d["intrinsics"][:, S - 1:], d["poses"][:1], r64["d_proj"][:, S - 1:, :1])[:, 0]
    one = dict(d_proj=r64["d_proj"][:, :, :1], d_K=IG.d_k_from_d_proj(d["intrinsics"], d["poses"][:1], r64["d_proj"][:, :, :1]))
    bad = X.plant_no_inverse_route(dict(d, poses=d["poses"][:1]), one, 0)
    assert n > 1 and np.abs(bad["d_K"][:, -1] - only).max() <= 1e-12 * np.abs(only).max() and np.abs(full - only).max() > 0.01 * np.abs(only).max()


def test_the_factors_follow_from_the_measurements():
    assert set(X.FACTORS) == set(X.MEASURED) == set(X.REGIMES) == {"reference_order", "fast", "operator"}
    for regime in X.REGIMES:
        kinds = X.K_KINDS if regime == "operator" else X.KINDS
        assert set(X.FACTORS[regime]) == set(X.MEASURED[regime]) == set(kinds), regime
        for kind in kinds:
            k, r = X.FACTORS[regime][kind], X.MEASURED[regime][kind]
            if regime == "reference_order" and kind in ("d_proj", "d_K"):
                assert k == X.K_REF == 4 and r <= 4, (kind, r)          # the standing factor: held, not derived
            else:
                assert k == X.derived_factor(r) and k >= 4 and k & (k - 1) == 0 and r > 0, (regime, kind, k, r)
    assert [X.derived_factor(r) for r in (0.2, 1.0, 1.01, 2.0, 3.54, 4.01)] == [4, 4, 8, 8, 16, 32]


def test_search_finds_the_committed_seeds_and_rejects_others():
    shape = X.FOLD_SHAPE
    assert X.search(shape, 376, 8, want=1) == [X.CASES[shape][0]]
    assert any("yardstick" in line for line in X.failed_conditions(shape, 353))      # knife-free, but one block's yardstick is 1.6e-4
    assert X.failed_conditions(shape, 354)


# ---------------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_operator_cases():
    have = {(c[2], rows_, C) for c, rows_, C, _ in X.OPERATOR_CASES}
    assert have == {("default", 1, 3), ("default", 3, 3), ("default", 1, 5), ("default", 3, 5), (X.GENERAL_SETTING, 1, 3), (X.GENERAL_SETTING, 3, 3)}
    for c in X.GENERAL_OPERATOR_CASES:
        assert {i for cc, _, _, i in X.OPERATOR_CASES if cc == c} == set(range(c[0][3]))
    assert len(set(X.OPERATOR_CASES)) == len(X.OPERATOR_CASES)


@pytest.mark.parametrize("case", X.GENERAL_OPERATOR_CASES, ids=R.ident)
def test_the_general_camera_cases_are_knife_free(case):
    """warp_exact_ref's own conditions (every source, the three-row form included, both precisions, the yardsticks), and the cameras
    are tests/cameras.py's general ones on the same draw of everything else"""
    shape, seed, setting = case
    assert R.failed_conditions(shape, seed, setting) == []
    d, base = R.inputs(shape, seed, setting), R.make_inputs(shape, seed, "default", rows_draw=0)
    assert np.array_equal(d["intrinsics"], cameras.cameras(base, "general", 1000 + seed)) and np.array_equal(d["rows"], base["rows"])
    for key in ("src_pyr", "tgt_pyr", "disps", "poses", "g"):
        assert all(np.array_equal(p, q) for p, q in zip(d[key], base[key])), key
    for i in range(shape[3]):
        for rows_ in (1, 3):
            o64, o32 = R.operator_reference(d, F64, rows_, 3, i), R.operator_reference(d, F32, rows_, 3, i)
            assert not (R.operator_knife_of(o64) | R.operator_knife_of(o32)).any() and np.array_equal(o64["valid"], o32["valid"])


def test_search_finds_the_general_camera_seeds():
    (shape, seeds), = R.GENERAL_CASES.items()
    assert tuple(R.search(shape, X.GENERAL_SETTING, 0, max(seeds) + 1)) == seeds


@pytest.mark.parametrize("v", X.OPERATOR_CASES, ids=X.op_ident)
def test_the_operator_references(v):
    """the yardstick of every block is at most 1e-4 of its maximum; for one depth row the closed form on the oracle's gPm agrees
    with autograd to 1e-9 of every block's maximum"""
    a64, a32 = X.operator_references(v)
    for _, name, _, x, y in X.k_rows(a64, a64, a32):
        _, dev, top = KF.distances(x, x, y)
        assert 0 < dev <= X.YARDSTICK_MAX * top, (name, dev / top)
    if v[1] == 1:
        for _, name, got, x, _ in X.k_rows(X.operator_closed_form(v), a64, a64):
            err, _, top = KF.distances(got, x, x)
            assert err <= AGREE * top, (name, err / top)
