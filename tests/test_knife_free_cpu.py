"""The conditions under which tests/test_loss_exact_gpu.py may compare every element of every gradient of the fused loss with the
fp64 oracle, proved WITHOUT a GPU, from the oracle alone, for every case and seed of tests/knife_free.py under every configuration
of test_loss_gpu.CONFIGS:

  1. no knife pixel: oracle/parity.knife_mask is empty at every scale (the cell-boundary class max(1e-4 px, position bound) wide),
     by the fp64 oracle's margins and by the fp32 oracle's, and no pixel sits ON the kink of |I^ - I| (abs_zero);
  2. a class that mask does not have: every disparity stencil whose absolute value a smoothness term takes (second_order: the
     four second differences; edge_aware: dx and dy) is at least 1e-5 in magnitude;
  3. the masked branch is present: at every scale 2 % .. 75 % of the (pixel, source) pairs have an all-zero warped value;
  4. the yardstick cannot become vacuous: max|o32 - o64| <= 1e-4 max|o64| for every gradient array;
  5. the tolerance has teeth: the fp64 oracle with ONE non-zero weight of the configuration times 1.001 differs from the fp64 oracle,
     in at least one gradient array, by more than twice what knife_free.rule grants that array -- with K_REF and with K_FAST.
"""
import numpy as np
import pytest

import knife_free as KF
from test_loss_gpu import CONFIGS

WEIGHTS = ("ssim_rate", "smooth_reg", "exp_reg")
# (array kind, weight): the pairs for which the FAST regime's measured factor (knife_free.K_FAST) sees an error of 1 % in the
# weight, not of 0.1 %: with K_FAST[kind] the allowance of an array of that kind is too wide for 0.1 %.  None is needed: with the
# committed K_FAST every weight is seen at 0.1 % by some array.
RELAXED_FAST = set()

cases = pytest.mark.parametrize("case", KF.CASE_LIST, ids=KF.case_id)
configs = pytest.mark.parametrize("cfg_name", sorted(CONFIGS))


def test_the_cases_are_the_shapes_the_kernels_can_go_wrong_at():
    """two seeds per shape; more than one strip (W > 64), a ragged last strip, an odd height, more than one chunk of four rows,
    several scales, two samples and an odd source count all occur"""
    assert all(len(seeds) == 2 and len(set(seeds)) == 2 for seeds in KF.CASES.values())
    shapes = list(KF.CASES)
    assert any(W > 128 for _, _, W, _, _ in shapes) and any(64 < W < 128 and W % 64 for _, _, W, _, _ in shapes) and any(W <= 64 for _, _, W, _, _ in shapes)
    assert any(H % 2 and H % 4 for _, H, _, _, _ in shapes) and all(H > 4 for _, H, _, _, _ in shapes)
    assert any(S >= 3 for *_, S in shapes) and any(B > 1 for B, *_ in shapes) and any(n % 2 for _, _, _, n, _ in shapes)
    assert all(B * H * W * n <= 2 * 5200 for B, H, W, n, _ in shapes)


@cases
def test_the_inputs_are_the_rescaled_synth_inputs(case):
    shape, seed = case
    B, H, W, n_src, S = shape
    d = KF.inputs(shape, seed)
    base = KF.synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=S, seed=seed, with_masks=True, seam="shift")
    for key in ("disps", "poses", "masks"):
        assert all(np.array_equal(a, b) for a, b in zip(d[key], base[key])), key
    assert np.array_equal(d["intrinsics"], base["intrinsics"])
    assert np.array_equal(d["tgt"], np.float32(0.3) * base["tgt"])
    off = d["src"] - np.float32(0.3) * base["src"]                       # +-0.45 per (sample, source, channel), both signs present
    assert off.dtype == np.float32 and np.allclose(np.abs(off), 0.45, rtol=0, atol=1e-6)
    assert (off.min(axis=(3, 4)) > 0).sum() + (off.max(axis=(3, 4)) < 0).sum() == B * n_src * 3
    assert (off > 0).any() and (off < 0).any()
    assert all(a.dtype == np.float32 for key in ("tgt_pyr", "src_pyr") for a in d[key])
    assert np.array_equal(d["tgt_pyr"][0], d["tgt"]) and np.array_equal(d["src_pyr"][0], d["src"].reshape(B, 3 * n_src, H, W))
    assert [a.shape[2:] for a in d["src_pyr"]] == [a.shape[2:] for a in d["disps"]]


@configs
@cases
def test_no_knife_pixel(case, cfg_name):
    d = KF.inputs(*case)
    for ref, which in zip(KF.references(*case, cfg_name), ("fp64", "fp32")):
        found = KF.knife_pixels(d, ref)
        assert not any(found.values()), "%s oracle: %s" % (which, found)


@cases
def test_no_smoothness_stencil_near_its_kink(case):
    d = KF.inputs(*case)
    for mode in ("second_order", "edge_aware"):
        for dtype in (np.float64, np.float32):
            assert KF.smooth_kink_margin(d, mode, dtype) >= KF.SMOOTH_KINK_MIN, (mode, dtype.__name__, KF.smooth_kink_margin(d, mode, dtype))


def test_the_smoothness_class_sees_a_stencil_on_its_kink():
    """(a linear ramp has second differences of zero and first differences that are not)"""
    ramp = np.arange(20, dtype=np.float32).reshape(1, 1, 4, 5)
    assert KF.smooth_kink_margin(dict(disps=[ramp]), "second_order") == 0.0
    assert KF.smooth_kink_margin(dict(disps=[ramp]), "edge_aware") == 1.0
    assert [t.shape[2:] for t in KF.smooth_stencils(ramp, "second_order")] == [(4, 3), (3, 4), (3, 4), (2, 5)]


@configs
@cases
def test_the_masked_branch_is_present(case, cfg_name):
    o64, o32 = KF.references(*case, cfg_name)
    for ref in (o64, o32):
        for s, share in enumerate(KF.masked_shares(ref)):
            assert KF.MASKED_SHARE[0] <= share <= KF.MASKED_SHARE[1], (s, share)


@configs
@cases
def test_the_yardstick_is_not_vacuous(case, cfg_name):
    o64, o32 = KF.references(*case, cfg_name)
    ys = KF.yardsticks(o64, o32, CONFIGS[cfg_name])
    print("yardsticks %s %s: %s" % (KF.case_id(case), cfg_name, ", ".join("%s %.2e" % y for y in ys)))
    assert len(ys) >= 2 and all(0 < y <= KF.YARDSTICK_MAX for _, y in ys), ys


def seen_by(o64, o32, p64, cfg, k_of, kinds):
    """the gradient arrays of `kinds` in which the perturbed fp64 oracle p64 differs from o64 by more than twice the rule's allowance"""
    out = []
    for (kind, name, a64), (_, _, a32), (_, _, ap) in zip(KF.arrays_of(o64, cfg), KF.arrays_of(o32, cfg), KF.arrays_of(p64, cfg)):
        if kind != "loss" and kind in kinds:
            moved = float(np.abs(np.asarray(ap, np.float64) - a64).max())
            if moved > 2 * KF.allowance(a64, a32, k_of[kind]):
                out.append((name, moved / KF.allowance(a64, a32, k_of[kind])))
    return out


@configs
@cases
def test_the_tolerance_has_teeth(case, cfg_name):
    d, cfg = KF.inputs(*case), CONFIGS[cfg_name]
    o64, o32 = KF.references(*case, cfg_name)
    grad_kinds = [k for k in KF.KINDS if k != "loss"]
    for weight in WEIGHTS:
        if not cfg.get(weight):
            continue
        p64 = {f: KF.oracle(d, cfg, np.float64, **{weight: cfg[weight] * f}) for f in (1.001,)}
        ref = seen_by(o64, o32, p64[1.001], cfg, {k: KF.K_REF for k in KF.KINDS}, grad_kinds)
        assert ref, "reference-order regime (k = %d): no gradient array sees %s x 1.001" % (KF.K_REF, weight)
        relaxed = [k for k in grad_kinds if (k, weight) in RELAXED_FAST]
        fast = seen_by(o64, o32, p64[1.001], cfg, KF.K_FAST, [k for k in grad_kinds if k not in relaxed])
        if not fast and relaxed:
            p64[1.01] = KF.oracle(d, cfg, np.float64, **{weight: cfg[weight] * 1.01})
            fast = seen_by(o64, o32, p64[1.01], cfg, KF.K_FAST, relaxed)
        assert fast, "fast regime (K_FAST = %s): no gradient array sees %s x 1.001 (x 1.01 for %s)" % (KF.K_FAST, weight, sorted(RELAXED_FAST))
        print("teeth %s %s %s: times twice the allowance -- reference order %s; fast %s" % (
            KF.case_id(case), cfg_name, weight, ", ".join("%s %.1f" % (n, r / 2) for n, r in ref), ", ".join("%s %.1f" % (n, r / 2) for n, r in fast)))


def test_the_rule_is_the_standing_rule_with_a_factor():
    """tests/test_disp_smooth_cpu.py::rule at k = 4; one element out of thousands off by more than the allowance fails it"""
    rng = np.random.RandomState(0)
    o64 = rng.standard_normal((2, 1, 9, 11))
    o32 = o64 + 1e-6 * rng.uniform(-1, 1, o64.shape)
    dev, top = np.abs(o32 - o64).max(), np.abs(o64).max()
    assert KF.allowance(o64, o32, 4) == 4 * dev + 1e-6 * top
    got = o64.copy()
    got[1, 0, 8, 10] += 0.999 * KF.allowance(o64, o32, 4)
    assert KF.rule(got, o64, o32, "inside") == pytest.approx(0.999 * KF.allowance(o64, o32, 4) / dev)
    got[1, 0, 8, 10] = o64[1, 0, 8, 10] + 1.001 * KF.allowance(o64, o32, 4)
    with pytest.raises(AssertionError):
        KF.rule(got, o64, o32, "outside")
    KF.rule(got, o64, o32, "a larger factor", k=8)
    with pytest.raises(AssertionError):
        KF.rule(np.where(np.arange(11) == 3, np.nan, o64), o64, o32, "not finite")
    assert KF.rule(0.0, 0.0, 0.0, "a term the configuration does not have") == 0.0
    assert KF.floor_ratio(got, o64, o32) == pytest.approx(1.001 * KF.allowance(o64, o32, 4) / (dev + KF.FLOOR * top))
    assert set(KF.K_FAST) == set(KF.KINDS) and all(k >= 1 and k & (k - 1) == 0 for k in KF.K_FAST.values())      # powers of two


def test_search_finds_the_committed_seeds_and_rejects_others():
    shape = (1, 37, 70, 2, 1)
    first = min(KF.CASES[shape])
    found = KF.search(shape, first - 3, 4)
    assert first in found and len(found) < 4, found
    assert any("smoothness" in line for line in KF.failed_conditions(shape, 2))      # knife-free but for the smoothness class
