"""The gradient with respect to the camera intrinsics on the GPU against float64, on textured knife-free inputs under general
cameras (tests/intrinsics_exact_ref.py; tests/test_intrinsics_exact_cpu.py proves the cases knife-free, the two float64 statements
equal and every planted error caught): d_proj = dL/dPm and d_intrinsics of sfm_loss_proj_bwd behind every kernel family of the
fused loss, d_K of sfm_warp_intrinsics_bwd, and K.grad of the torch route.

Every comparison is knife_free.rule -- max|gpu - o64| <= k max|o32 - o64| + 1e-6 max|o64| -- per scale, on the whole array and on
every block of like unit (intrinsics_exact_ref.PROJ_BLOCKS / K_BLOCKS), nothing excluded.  k = K_REF = 4 on the whole arrays with
projection="reference_order"; every other factor is measured (intrinsics_exact_ref.FACTORS, profiles/intrinsics_accuracy.txt).  The
yardstick is the float32 reference, never the kernel.

tests/test_intrinsics_grad_gpu.py keeps the ramp inputs: the only end-to-end check at 128 .. 224 tiles; a ramp cannot see the
bilinear sampler's gradient (the four tap differences of a cell are equal), these inputs can."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import intrinsics_exact_ref as X
import intrinsics_grad as IG
import knife_free as KF
import warp_exact_ref as R
from test_loss_exact_gpu import expected_family
from util import parity_note, to_dev, to_np

pytestmark = pytest.mark.gpu

STALE = 7.0
ENTRIES = (("sfm_loss_bwd", 0), ("sfm_loss_fwd_bwd", 1))      # (entry point, the `loss` argument of sfm_loss_proj_bwd behind it)
ENTRY_NAME = {0: "backward", 1: "forward_backward"}             # test_loss_exact_gpu.ENTRY's names
PROJECTIONS = ("reference_order", "fast")
LAUNCHES = [(layout, d_src) for layout in ("planar", "hwc") for d_src in (False, True)]
TORCH_CASE, TORCH_CONFIG = X.CASE_LIST[0], "ssim_smooth"       # one scale: the route's own pyramid is the frame itself


def bind(ops, dev, d, cfg, layout, projection, d_src, buffers=None):
    """a FusedLoss on the inputs d that leaves d_intrinsics and d_proj (tests/test_intrinsics_grad_gpu.py::bind, with `buffers`)"""
    fl = ops.FusedLoss(projection=projection, **cfg)
    tgt, src = [to_dev(a, dev) for a in d["tgt_pyr"]], [to_dev(a, dev) for a in d["src_pyr"]]
    if layout == "hwc":
        tgt, src = [ops.to_hwc(a) for a in tgt], [ops.to_hwc(a) for a in src]
    fl.bind(tgt, src, to_dev(d["intrinsics"], dev), [to_dev(a, dev) for a in d["disps"]], [to_dev(a, dev) for a in d["poses"]],
            [to_dev(a, dev) for a in d["masks"]], want_d_src=d_src, layout=layout, want_d_intrinsics=True, want_d_proj=True, buffers=buffers)
    return fl


def run(fl, loss):
    """one gradient entry point with sfm_loss_proj_bwd behind it, the outputs holding a value no gradient has before -> (d_proj,
    d_intrinsics) as host copies"""
    fl.d_proj.fill_(STALE), fl.d_intrinsics.fill_(STALE)
    if loss:
        fl.forward_backward()
    else:
        fl.forward()
        fl.backward(1.0)
    return to_np(fl.d_proj).copy(), to_np(fl.d_intrinsics).copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fused_launches(ops, dev, case, cfg_name, projection, cfg=None):
    """every launch of one case under one configuration and projection: both layouts, without and with d_src, after sfm_loss_bwd and
    after sfm_loss_fwd_bwd; each asserted to be the family it has to be, finite, and repeated bit for bit
    -> (what, family, d_proj, d_intrinsics, the bound FusedLoss)"""
    d, n_src = X.inputs(*case), case[0][3]
    base = X.CONFIGS[cfg_name]
    for layout, d_src in LAUNCHES:
        fl = bind(ops, dev, d, base if cfg is None else cfg, layout, projection, d_src)
        for entry, loss in ENTRIES:
            fam = IG.plan_of(ops.lib, fl.desc, 1, loss)[1]
            what = "%s %s %s %s%s %s" % (X.case_id(case), cfg_name, projection, layout, " with d_src" if d_src else "", entry)
            assert fam in expected_family(base, layout, n_src, ENTRY_NAME[loss], projection, d_src), (what, fam)
            dP, dK = run(fl, loss)
            assert np.isfinite(dP).all() and np.isfinite(dK).all(), what
            again = run(fl, loss)
            assert np.array_equal(bits(again[0]), bits(dP)) and np.array_equal(bits(again[1]), bits(dK)), "%s: two calls differ" % what
            yield what, fam, dP, dK, fl


def check(rows, k_of, what):
    """knife_free.rule on every row with its kind's factor; one parity note per launch: the largest floor_ratio per kind"""
    worst = {}
    for kind, name, got, a64, a32 in rows:
        worst[kind] = max(worst.get(kind, 0.0), KF.floor_ratio(got, a64, a32))
    parity_note("intrinsics_exact %s: max|gpu-o64| / (max|o32-o64| + 2.5e-7 max|o64|) %s" % (
        what, ", ".join("%s %.2f (k %g)" % (kind, r, k_of[kind]) for kind, r in worst.items())))
    for kind, name, got, a64, a32 in rows:
        KF.rule(got, a64, a32, "%s %s" % (what, name), k=k_of[kind])


def nan_adjacent(ops, dev, case, cfg_name, projection, want):
    """once more with the workspace and, directly behind it in the same allocation, both outputs pre-filled with NaN: both are
    documented as overwritten, and hold the bits of the ordinary launch"""
    d = X.inputs(*case)
    probe = bind(ops, dev, d, X.CONFIGS[cfg_name], "hwc", projection, False)
    ws_bytes = -(-probe._ws_bytes // 256) * 256
    B, S, n = want[0].shape[:3]
    n_p, n_k = B * S * n * 12, B * S * 9
    block = torch.full((ws_bytes // 4 + n_p + n_k,), float("nan"), dtype=torch.float32, device=dev)
    assert block.data_ptr() % 256 == 0
    fl = bind(ops, dev, d, X.CONFIGS[cfg_name], "hwc", projection, False, buffers=dict(ws=block[:ws_bytes // 4]))
    fl.forward_backward()
    p_proj = block.data_ptr() + ws_bytes
    ops._launch(dev, ops.lib.sfm_loss_proj_bwd, fl._desc_ref, 1, fl._ws_arg, fl._ws_bytes, C.c_void_p(p_proj), C.c_void_p(p_proj + 4 * n_p))
    out = to_np(block[ws_bytes // 4:])
    assert np.isfinite(out).all(), "an element of an output was never written"
    assert np.array_equal(bits(out[:n_p]), bits(want[0]).ravel()) and np.array_equal(bits(out[n_p:]), bits(want[1]).ravel())


def fused_case(ops, dev, case, cfg_name, projection):
    r64, r32 = X.references(*case, cfg_name)
    fams, hwc = set(), None
    for what, fam, dP, dK, fl in fused_launches(ops, dev, case, cfg_name, projection):
        check(X.rows(dP, dK, r64, r32), X.FACTORS[projection], "%s [%s]" % (what, fam))
        fams.add(fam)
        if " hwc sfm_loss_fwd_bwd" in what:
            hwc = (dP, dK)
    nan_adjacent(ops, dev, case, cfg_name, projection, hwc)
    return fams


@pytest.mark.parametrize("cfg_name", sorted(X.CONFIGS))
@pytest.mark.parametrize("case", X.CASE_LIST, ids=X.case_id)
def test_reference_order_projection_against_float64(ops, dev, case, cfg_name):
    """family ref: the whole d_proj[:, s] and d_K[:, s] within K_REF = 4 times the float32 oracle's own distance from float64, the
    blocks within their measured factors"""
    assert X.FACTORS["reference_order"]["d_proj"] == X.FACTORS["reference_order"]["d_K"] == X.K_REF == 4
    assert fused_case(ops, dev, case, cfg_name, "reference_order") == {"ref"}


@pytest.mark.parametrize("cfg_name", sorted(X.CONFIGS))
@pytest.mark.parametrize("case", X.CASE_LIST, ids=X.case_id)
def test_fast_projection_against_float64(ops, dev, case, cfg_name):
    """families base, wide, pair and dsrc (the planner's own choice, never sfm_loss_variant(4) / (5): the header leaves
    sfm_loss_proj_bwd unspecified after them), every kind within its measured factor"""
    fams = fused_case(ops, dev, case, cfg_name, "fast")
    assert "dsrc" in fams and "ref" not in fams, fams
    assert ("wide" in fams) == (cfg_name == "l1"), fams


def test_each_of_the_five_families_is_reached():
    """what the two tests above launch, from the plan alone (sfm_loss_plan_info launches nothing): over their cases, configurations,
    layouts and entry points every family is the planned kernel of some launch"""
    planned = set()
    for shape in X.CASES:
        for mode in X.CONFIGS:
            for projection in PROJECTIONS:
                for layout, d_src in LAUNCHES:
                    for _, loss in ENTRIES:
                        fam = IG.host_plan(shape, mode, layout, projection, d_src, 1, loss)[1]
                        assert fam in expected_family(X.CONFIGS[mode], layout, shape[3], ENTRY_NAME[loss], projection, d_src), (shape, mode, fam)
                        planned.add(fam)
    assert planned == set(IG.FAMILIES.values()), planned


def test_one_launch_of_each_family(ops, dev):
    """one case, five launches, each asserted through sfm_loss_plan_info to be the family it is meant to be, each by the rule"""
    case = X.CASE_LIST[0]
    d = X.inputs(*case)
    launches = [      # (configuration, layout, projection, d_src, family)
        ("explain", "hwc", "fast", False, "base"),
        ("l1", "planar", "fast", False, "wide"),
        ("ssim_smooth", "hwc", "fast", False, "pair"),
        ("edge_aware", "hwc", "reference_order", False, "ref"),
        ("ssim_smooth", "planar", "fast", True, "dsrc"),
    ]
    ran = set()
    for cfg_name, layout, projection, d_src, want in launches:
        fl = bind(ops, dev, d, X.CONFIGS[cfg_name], layout, projection, d_src)
        fam = IG.plan_of(ops.lib, fl.desc, 1, 1)[1]
        assert fam == want, "%s %s: the planner chose family %s, not %s" % (cfg_name, layout, fam, want)
        dP, dK = run(fl, 1)
        check(X.rows(dP, dK, *X.references(*case, cfg_name)), X.FACTORS[projection], "one launch of each family, %s %s [%s]" % (cfg_name, layout, fam))
        ran.add(fam)
    assert ran == set(IG.FAMILIES.values()), ran


def test_the_fold_goes_past_its_first_trip_on_textured_inputs(ops, dev):
    """the 260 x 20 frame is 65 tiles in every launch of the tests above (tests/test_fold_rounds_cpu.py pins the host plan)"""
    d = X.inputs(X.FOLD_SHAPE, X.CASES[X.FOLD_SHAPE][0])
    for projection in PROJECTIONS:
        for layout, d_src in LAUNCHES:
            fl = bind(ops, dev, d, X.CONFIGS["ssim_smooth"], layout, projection, d_src)
            for _, loss in ENTRIES:
                assert IG.plan_of(ops.lib, fl.desc, 1, loss)[0] == X.FOLD_TILES


# ------------------------------------------------------------------------------------------------------------------------
# sfm_warp_intrinsics_bwd
# ------------------------------------------------------------------------------------------------------------------------
def operator_rows(ops, dev, v):
    (shape, seed, setting), rows_, C_, i = v
    imgs, _, dev_depth, pose, K, g = R.operator_inputs(R.inputs(shape, seed, setting), rows_, C_, i)
    args = [to_dev(a, dev) for a in (imgs, dev_depth, pose, K, g)]
    got = ops.warp_bwd_intrinsics(*args)
    assert torch.isfinite(got).all() and torch.equal(ops.warp_bwd_intrinsics(*args).view(torch.int32), got.view(torch.int32))
    a64, a32 = X.operator_references(v)
    return X.k_rows(to_np(got).astype(np.float64), a64, a32)


@pytest.mark.parametrize("v", X.OPERATOR_CASES, ids=X.op_ident)
def test_warp_intrinsics_bwd_against_float64(ops, dev, v):
    """every source of warp_exact_ref's operator cases and of the general-camera cases, one and three depth rows, five channels on
    one case: fp64 autograd the reference, fp32 autograd the yardstick, the whole d_K and its four blocks"""
    check(operator_rows(ops, dev, v), X.FACTORS["operator"], "operator %s" % X.op_ident(v))


# ------------------------------------------------------------------------------------------------------------------------
# torch
# ------------------------------------------------------------------------------------------------------------------------
def torch_rows(dev):
    """K.grad of torch_api.sfm_learner_loss on one case (tests/test_intrinsics_torch_gpu.py ties it bit for bit to the fused value)"""
    ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
    d = X.inputs(*TORCH_CASE)
    assert TORCH_CASE[0][4] == 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    K = t(d["intrinsics"]).requires_grad_()
    total, _ = ta.sfm_learner_loss(t(d["tgt"]), t(d["src"]), K, [t(a).requires_grad_() for a in d["disps"]],
                                   [t(a).requires_grad_() for a in d["poses"]], None, **X.CONFIGS[TORCH_CONFIG])
    total.backward()
    r64, r32 = X.references(*TORCH_CASE, TORCH_CONFIG)
    return X.k_rows(to_np(K.grad).astype(np.float64), r64["d_K"], r32["d_K"])


def test_the_torch_route_against_float64(dev):
    check(torch_rows(dev), X.FACTORS["fast"], "torch_api.sfm_learner_loss %s %s" % (X.case_id(TORCH_CASE), TORCH_CONFIG))


# ------------------------------------------------------------------------------------------------------------------------
# teeth
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("projection", PROJECTIONS)
@pytest.mark.parametrize("cfg_name", sorted(name for name, cfg in X.CONFIGS.items() if cfg.get(X.PLANT_WEIGHT)))
def test_a_kernel_with_a_weight_off_by_a_per_mille_misses_the_rule(ops, dev, cfg_name, projection):
    """what tests/test_intrinsics_exact_cpu.py proves of the oracle, seen on the device: the same launch with ssim_rate (the one
    loss weight that reaches d_proj) times 1.001 lands outside the rule's allowance in at least one block"""
    case = X.CASE_LIST[2]
    cfg = X.CONFIGS[cfg_name]
    r64, r32 = X.references(*case, cfg_name)
    fl = bind(ops, dev, X.inputs(*case), dict(cfg, **{X.PLANT_WEIGHT: cfg[X.PLANT_WEIGHT] * 1.001}), "hwc", projection, False)
    dP, dK = run(fl, 1)
    missed = X.outside(X.rows(dP, dK, r64, r32), X.FACTORS[projection])
    assert missed, (cfg_name, projection)
    parity_note("intrinsics_exact %s %s, %s x 1.001 [%s]: outside the allowance in %d arrays, the furthest %s at %.1f allowances" % (
        (X.case_id(case), cfg_name, X.PLANT_WEIGHT, projection, len(missed)) + max(missed, key=lambda m: m[1])))


# ------------------------------------------------------------------------------------------------------------------------
# what tools/intrinsics_accuracy.py measures the factors on
# ------------------------------------------------------------------------------------------------------------------------
def every_row(ops, dev):
    """(regime, what, kind, name, got, o64, o32) of every comparison of this module"""
    for case in X.CASE_LIST:
        for cfg_name in sorted(X.CONFIGS):
            r64, r32 = X.references(*case, cfg_name)
            for projection in PROJECTIONS:
                for what, fam, dP, dK, _ in fused_launches(ops, dev, case, cfg_name, projection):
                    for row in X.rows(dP, dK, r64, r32):
                        yield (projection, "%s [%s]" % (what, fam)) + row
    for row in torch_rows(dev):
        yield ("fast", "torch_api.sfm_learner_loss %s %s" % (X.case_id(TORCH_CASE), TORCH_CONFIG)) + row
    for v in X.OPERATOR_CASES:
        for row in operator_rows(ops, dev, v):
            yield ("operator", "operator %s" % X.op_ident(v)) + row
