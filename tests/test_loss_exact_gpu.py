"""The fused loss (sfm_loss_fwd / _bwd / _fwd_bwd) against the fp64 ORACLE on knife-free inputs (tests/knife_free.py): the five
scalars and EVERY element of d_disp, d_pose, d_mask and d_src by

    max|gpu - o64| <= k max|o32 - o64| + 1e-6 max|o64|          (knife_free.rule; o32 the same oracle in float32)

-- no knife mask, no in-view allowance, no second opinion, no named pixels: tests/test_knife_free_cpu.py proves from the oracle alone
that these inputs have no pixel near a discontinuity of the reference's function, that max|o32 - o64| stays below 1e-4 of the
array's maximum, and that a 0.1 % error in any loss weight exceeds twice what the rule grants.  (tests/test_loss_gpu.py compares
the same kernels on inputs that do have such pixels, at 2e-3 behind its ladder of allowances.)

Every launch that is a kernel of its own (Family in csrc/sfm_loss_kernels.h), the family read from sfm_loss_plan_info:
  * ref  -- projection="reference_order": k = K_REF = 4, all eight configurations, both layouts, forward() + backward(1.0) and
    forward_backward(), and once more with d_src;
  * base, wide, pair, dsrc -- the default projection: k = K_FAST per array kind, measured on an MI355X
    (profiles/loss_grad_accuracy.txt); the SSIM configurations in the pixel-interleaved layout with an even source count in both the
    one-source and the two-sources-per-pass form (sfm_loss_variant), on the same inputs.
Each measured ratio is reported (util.parity_note / parity_row, kind "knife_free")."""
import ctypes as C

import numpy as np
import pytest

import knife_free as KF
from test_loss_gpu import CONFIGS, KEYS, _bind
from util import parity_note, parity_row, to_np

pytestmark = pytest.mark.gpu

FAMILIES = {0: "base", 1: "wide", 2: "pair", 3: "ref", 4: "dsrc"}      # what sfm_loss_plan_info reports (include/sfmwarp.h)
HOOK_ONE_SOURCE, HOOK_TWO_SOURCES = 4, 5                                  # sfm_loss_variant (csrc/sfm_loss.hip)
ENTRY = {"forward": (0, 1), "backward": (1, 0), "forward_backward": (1, 1)}
STALE = 7.0


def family(ops, fl, entry):
    """the kernel family sfm_loss_plan_info reports for the bound descriptor and the entry point"""
    n = fl.desc.n_scales
    out = (C.c_int * (1 + 4 * n + 2))()
    ops.check(ops.lib.sfm_loss_plan_info(C.byref(fl.desc), ENTRY[entry][0], ENTRY[entry][1], out, len(out)))
    return FAMILIES[out[1 + 4 * n]]


def expected_family(cfg, layout, n_src, entry, projection="fast", d_src=False):
    """the family a launch of these small cases must be (choose_variant, csrc/sfm_loss.hip); a tuple where the planner may choose"""
    grad = ENTRY[entry][0]
    ssim = bool(cfg.get("ssim_rate")) and not cfg.get("exp_reg")
    if projection == "reference_order":
        return ("ref",)
    if grad and d_src:
        return ("dsrc",)
    if grad and ssim and layout == "hwc" and n_src % 2 == 0:
        return ("base", "pair")
    if grad and not ssim and not cfg.get("exp_reg"):
        return ("wide",)
    return ("base",)


def stale(fl):
    """every gradient array the next launch has to overwrite holds a value no gradient has (d_src is cleared by the binding)"""
    for t in fl.d_disps + fl.d_poses + (fl.d_masks or []):
        t.fill_(STALE)


def outputs(fl, cfg, loss5=None, grad=False):
    """name -> host copy of what the launch wrote, under the names of knife_free.arrays_of"""
    got = {}
    if loss5 is not None:
        got.update((name, float(v)) for name, v in zip(KEYS, to_np(loss5)))
    if grad:
        got.update(("d_disp[%d]" % s, to_np(t).copy()) for s, t in enumerate(fl.d_disps))
        got.update(("d_pose[%d]" % i, to_np(t).copy()) for i, t in enumerate(fl.d_poses))
        if cfg.get("exp_reg"):
            got.update(("d_mask[%d]" % s, to_np(t).copy()) for s, t in enumerate(fl.d_masks))
        if fl.d_srcs is not None:
            got.update(("d_src[%d]" % s, to_np(t).copy()) for s, t in enumerate(fl.d_srcs))
    return got


def compare(got, case, cfg_name, k_of, fam, what, kinds):
    """every array of `kinds` the configuration has, by the rule with k = k_of[kind]; one parity row per array"""
    (shape, seed), cfg = case, CONFIGS[cfg_name]
    o64, o32 = KF.references(shape, seed, cfg_name)
    seen, worst = set(), {}
    for (kind, name, a64), (_, _, a32) in zip(KF.arrays_of(o64, cfg), KF.arrays_of(o32, cfg)):
        if kind not in kinds:
            continue
        g = got[name]                                                   # (a missing array is an error, never a skipped comparison)
        err, dev, top = KF.distances(g, a64, a32)
        fr = KF.floor_ratio(g, a64, a32)
        parity_row(kind="knife_free", case=KF.case_id(case), config=cfg_name, family=fam, launch=what, array_kind=kind, array=name,
                   err=err, oracle32_own_err=dev, top=top, floor_ratio=fr, k=k_of[kind])
        worst[kind] = max(worst.get(kind, 0.0), fr)
        KF.rule(g, a64, a32, "%s %s %s [%s] %s" % (KF.case_id(case), cfg_name, what, fam, name), k=k_of[kind])
        seen.add(kind)
    assert seen == set(kinds), (seen, kinds)
    parity_note("knife-free %s %s %s [%s]: max|gpu-o64| / (max|o32-o64| + 2.5e-7 max|o64|) %s" % (
        KF.case_id(case), cfg_name, what, fam, ", ".join("%s %.2f (k %g)" % (k, worst[k], k_of[k]) for k in KF.KINDS if k in worst)))


def grad_kinds(cfg, d_src):
    return ["d_disp", "d_pose"] + (["d_mask"] if cfg.get("exp_reg") else []) + (["d_src"] if d_src else [])


def check_entry_points(ops, fl, case, cfg_name, layout, k_of, projection, d_src, tag):
    """forward() + backward(1.0), then forward_backward(), each launch against the fp64 oracle and in the family it has to be"""
    cfg, n_src = CONFIGS[cfg_name], case[0][3]
    fams = {e: family(ops, fl, e) for e in ENTRY}
    for e, fam in fams.items():
        assert fam in expected_family(cfg, layout, n_src, e, projection, d_src), (e, fam)
    gk = grad_kinds(cfg, d_src)
    compare(outputs(fl, cfg, loss5=fl.forward()), case, cfg_name, k_of, fams["forward"], "%s %s forward" % (tag, layout), ["loss"])
    stale(fl)
    fl.backward(1.0)
    compare(outputs(fl, cfg, grad=True), case, cfg_name, k_of, fams["backward"], "%s %s backward" % (tag, layout), gk)
    stale(fl)
    fl.loss5.fill_(STALE)
    loss5 = fl.forward_backward()
    both = outputs(fl, cfg, loss5=loss5, grad=True)
    compare(both, case, cfg_name, k_of, fams["forward_backward"], "%s %s forward_backward" % (tag, layout), ["loss"] + gk)
    return fams, both


K_OF_REF = {kind: KF.K_REF for kind in KF.KINDS}


@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
@pytest.mark.parametrize("case", KF.CASE_LIST, ids=KF.case_id)
def test_reference_order_projection_to_the_oracles_own_accuracy(ops, dev, case, cfg_name):
    """family ref: every entry point in both layouts, without and with d_src, within K_REF = 4 times the fp32 oracle's own distance
    from the fp64 oracle"""
    d, cfg = KF.inputs(*case), CONFIGS[cfg_name]
    for layout in ("planar", "hwc"):
        for d_src in (False, True):
            fl = _bind(ops, dev, d, cfg, layout=layout, want_d_src=d_src, projection="reference_order")
            fams, _ = check_entry_points(ops, fl, case, cfg_name, layout, K_OF_REF, "reference_order", d_src,
                                         "reference order" + (" with d_src" if d_src else ""))
            assert set(fams.values()) == {"ref"}, fams


@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
@pytest.mark.parametrize("case", KF.CASE_LIST, ids=KF.case_id)
def test_fast_projection_to_its_measured_accuracy(ops, dev, case, cfg_name):
    """families base, wide, pair and dsrc: every entry point in both layouts, without and with d_src, within K_FAST (per array kind)
    times the fp32 oracle's own distance from the fp64 oracle; where the two-sources-per-pass form exists, both forms"""
    d, cfg, n_src = KF.inputs(*case), CONFIGS[cfg_name], case[0][3]
    for layout in ("planar", "hwc"):
        fl = _bind(ops, dev, d, cfg, layout=layout)
        fams, default = check_entry_points(ops, fl, case, cfg_name, layout, KF.K_FAST, "fast", False, "fast")
        if expected_family(cfg, layout, n_src, "forward_backward") == ("base", "pair"):
            # the one-call hook decides between loss_kernel (one source per pass) and loss_kernel_pair: both against the ORACLE, and
            # the default launch is bit for bit the form the plan reports
            gk = grad_kinds(cfg, False)
            for hook, fam in ((HOOK_ONE_SOURCE, "base"), (HOOK_TWO_SOURCES, "pair")):
                stale(fl)
                fl.loss5.fill_(STALE)
                loss5 = fl.forward_backward(variant=hook)
                got = outputs(fl, cfg, loss5=loss5, grad=True)
                compare(got, case, cfg_name, KF.K_FAST, fam, "fast hwc forward_backward, sfm_loss_variant(%d)" % hook, ["loss"] + gk)
                if fam == fams["forward_backward"]:
                    for name, a in default.items():
                        np.testing.assert_array_equal(got[name], a, err_msg=name)
                stale(fl)
                ops.check(ops.lib.sfm_loss_variant(hook))
                fl.backward(1.0)
                compare(outputs(fl, cfg, grad=True), case, cfg_name, KF.K_FAST, fam, "fast hwc backward, sfm_loss_variant(%d)" % hook, gk)
        fs = _bind(ops, dev, d, cfg, layout=layout, want_d_src=True)
        fams_s, _ = check_entry_points(ops, fs, case, cfg_name, layout, KF.K_FAST, "fast", True, "fast with d_src")
        assert fams_s["backward"] == fams_s["forward_backward"] == "dsrc", fams_s


@pytest.mark.parametrize("projection", ["fast", "reference_order"])
@pytest.mark.parametrize("cfg_name", sorted(name for name, cfg in CONFIGS.items() if cfg))
def test_a_kernel_with_a_weight_off_by_a_per_mille_misses_the_rule(ops, dev, cfg_name, projection):
    """What tests/test_knife_free_cpu.py proves of the oracle, seen on the device: the same launch with ONE loss weight times 1.001
    lands outside the rule's allowance in at least one gradient array -- the comparison would notice a mis-weighted term."""
    case = KF.CASE_LIST[2]
    d, cfg = KF.inputs(*case), CONFIGS[cfg_name]
    o64, o32 = KF.references(*case, cfg_name)
    k_of = K_OF_REF if projection == "reference_order" else KF.K_FAST
    for weight in ("ssim_rate", "smooth_reg", "exp_reg"):
        if not cfg.get(weight):
            continue
        fl = _bind(ops, dev, d, dict(cfg, **{weight: cfg[weight] * 1.001}), layout="hwc", want_d_src=True, projection=projection)
        stale(fl)
        got = outputs(fl, cfg, loss5=fl.forward_backward(), grad=True)
        missed = []
        for (kind, name, a64), (_, _, a32) in zip(KF.arrays_of(o64, cfg), KF.arrays_of(o32, cfg)):
            if kind != "loss" and KF.distances(got[name], a64, a32)[0] > KF.allowance(a64, a32, k_of[kind]):
                missed.append(name)
        parity_note("knife-free %s %s, %s x 1.001 [%s]: outside the allowance in %s" % (KF.case_id(case), cfg_name, weight, projection, missed))
        assert missed, (weight, projection)


def test_each_of_the_five_families_runs():
    """What the two tests above reach, from the plan alone (sfm_loss_plan_info launches nothing): over the cases and configurations
    they run, every family is the planned kernel of some launch -- pair by the planner's own choice, not only through the hook."""
    import intrinsics_grad as IG
    planned = set()
    for shape in KF.CASES:
        n_src = shape[3]
        for mode in IG.CONFIGS:                  # (the configurations of tests/intrinsics_grad.py are four of CONFIGS, same values)
            assert IG.CONFIGS[mode] == CONFIGS[mode]
            for layout in ("planar", "hwc"):
                for projection in ("fast", "reference_order"):
                    for d_src in (False, True):
                        for e, (grad, loss) in ENTRY.items():
                            fam = IG.host_plan(shape, mode, layout, projection, d_src, grad, loss)[1]
                            assert fam in expected_family(CONFIGS[mode], layout, n_src, e, projection, d_src), (shape, mode, layout, e, fam)
                            planned.add(fam)
    assert planned == set(FAMILIES.values()), planned


def test_one_launch_of_each_family(ops, dev):
    """One case, five launches, each asserted through sfm_loss_plan_info to be the family it is meant to be, each against the fp64
    oracle by the rule."""
    case = KF.CASE_LIST[0]
    d = KF.inputs(*case)
    launches = [      # (configuration, layout, bind arguments, family)
        ("explain_alpha", "hwc", dict(), "base"),
        ("l1", "planar", dict(), "wide"),
        ("ssim_smooth", "hwc", dict(), "pair"),
        ("edge_aware", "hwc", dict(projection="reference_order"), "ref"),
        ("ssim_only", "planar", dict(want_d_src=True), "dsrc"),
    ]
    ran = set()
    for cfg_name, layout, kw, want in launches:
        cfg = CONFIGS[cfg_name]
        fl = _bind(ops, dev, d, cfg, layout=layout, **kw)
        fam = family(ops, fl, "forward_backward")
        assert fam == want, "%s %s: the planner chose family %s, not %s" % (cfg_name, layout, fam, want)
        stale(fl)
        got = outputs(fl, cfg, loss5=fl.forward_backward(), grad=True)
        compare(got, case, cfg_name, K_OF_REF if want == "ref" else KF.K_FAST, fam, "one launch of each family, %s" % layout,
                ["loss"] + grad_kinds(cfg, bool(kw.get("want_d_src"))))
        ran.add(fam)
    assert ran == set(FAMILIES.values()), ran
