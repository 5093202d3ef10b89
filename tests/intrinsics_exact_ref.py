"""The gradient with respect to the camera intrinsics in float64, on textured inputs that have no pixel within reach of a
discontinuity -- a reference, not a test; host only: NumPy and torch on the CPU, no device, no library call.
tests/test_intrinsics_exact_cpu.py proves what is claimed here, tests/test_intrinsics_exact_gpu.py compares the kernels
(sfm_loss_proj_bwd behind every kernel family of the fused loss, sfm_warp_intrinsics_bwd, the torch route).

  * Inputs: knife_free.make_inputs(shape, seed, "general") -- the rescaled synth textures of tests/knife_free.py with the general
    cameras of tests/cameras.py (skew, a bottom row, per-scale rows; drawn with the seed 1000 + seed) and nothing else changed.  New
    cameras move every sample, so CASES has seeds of its own, found by `search`.
  * d_proj (B,S,n,3,4) = dL/dPm: oracle.sfm_loss(want_d_proj=True), rows 0..2 of the gPm that
    oracle.projective_inverse_warp_backward forms for every (scale, source).
  * d_K (B,S,3,3): the closed form intrinsics_grad.d_k_from_d_proj IN FLOAT64 applied to that d_proj.  include/sfmwarp.h: the
    kernel folds fp32 tile sums and forms K^-1 and the products in fp64 -- so the float32 statement of d_K, the yardstick, is the
    float64 closed form on the float32 oracle's d_proj, not a closed form evaluated in float32.
  * The second float64 opinion: intrinsics_grad.autograd_loss(d, cfg, want_gq=True), torch autograd with K a leaf; the two agree to
    1e-9 of every block's maximum (measured: 1.5e-15 .. 6.4e-15 of the array maximum).
  * Blocks.  The entries of d_K differ by a factor of 100 between the bottom row and the focal entries, and so do the columns of
    d_proj: a whole-array maximum sees K20 and K21 only.  Every comparison is per scale, on the whole array AND on blocks of like
    unit, each by knife_free.rule on the block's own array: max|got - o64| <= k max|o32 - o64| + 1e-6 max|o64|.  Nothing excluded.
  * Plants: the float64 reference with one error each; the rule has to reject every one of them under every committed factor.
  * The operator: sfm_warp_intrinsics_bwd on the operator cases of tests/warp_exact_ref.py and on cases with general cameras;
    reference intrinsics_grad.autograd_warp in float64, yardstick the same in float32; for one depth row also the closed form on
    the oracle's gPm.
"""
import contextlib
import functools

import numpy as np

import intrinsics_grad as IG
import knife_free as KF
import warp_exact_ref as R
from oracle import sfm_oracle as O

F32, F64 = np.float32, np.float64
KIND = "general"
CONFIGS = IG.CONFIGS                   # l1, ssim_smooth, edge_aware, explain: four of test_loss_gpu.CONFIGS, same values

# (B, H, W, n_src, n_scales) -> seeds: knife_free.CASES' shapes (what each is for: there) under the general cameras, and one frame
# of 65 tiles -- 260 rows in 4-row chunks, one strip -- that takes proj_bwd_kernel past its first trip on textured inputs
# (tests/test_fold_rounds_cpu.py pins the count).  Each seed passes `failed_conditions` under all four configurations.
CASES = {
    (1, 37, 70, 2, 1): (9, 12),
    (2, 32, 48, 2, 3): (1, 38),
    (1, 20, 130, 2, 2): (14, 30),
    (1, 37, 70, 3, 1): (29, 60),
    (1, 260, 20, 2, 1): (379, 465),     # (353 misses the yardstick condition: K[2,2], one number at B = 1, 1.6e-4 under the SSIM term)
}
CASE_LIST = [(shape, seed) for shape, seeds in CASES.items() for seed in seeds]
FOLD_SHAPE, FOLD_TILES = (1, 260, 20, 2, 1), [65]
case_id = KF.case_id

# name -> (rows, columns) of d_proj[:, s] (B,n,3,4) and of d_K[:, s] (B,3,3); the whole arrays are the kinds "d_proj" and "d_K"
PROJ_BLOCKS = {
    "P[0:2,0:2]": (slice(0, 2), slice(0, 2)), "P[0:2,2]": (slice(0, 2), slice(2, 3)), "P[0:2,3]": (slice(0, 2), slice(3, 4)),
    "P[2,0:2]": (slice(2, 3), slice(0, 2)), "P[2,2]": (slice(2, 3), slice(2, 3)), "P[2,3]": (slice(2, 3), slice(3, 4)),
}
K_BLOCKS = {
    "K[0:2,0:2]": (slice(0, 2), slice(0, 2)), "K[0:2,2]": (slice(0, 2), slice(2, 3)),
    "K[2,0:2]": (slice(2, 3), slice(0, 2)), "K[2,2]": (slice(2, 3), slice(2, 3)),
}
PROJ_KINDS = ("d_proj",) + tuple(PROJ_BLOCKS)
K_KINDS = ("d_K",) + tuple(K_BLOCKS)
KINDS = PROJ_KINDS + K_KINDS

# The factor k of knife_free.rule per regime and kind.
#   reference_order, whole arrays: knife_free.K_REF = 4, the project's standing factor -- not measured, not to be widened.
#   every block, and the whole arrays of the default projection ("fast": families base, wide, pair, dsrc) and of the operator:
#   MEASURED on an MI355X as knife_free.K_FAST was -- the largest knife_free.floor_ratio, max|gpu - o64| / (max|o32 - o64| +
#   2.5e-7 max|o64|), over all cases, configurations, layouts and entry points (profiles/intrinsics_accuracy.txt, written by
#   tools/intrinsics_accuracy.py), times 4 (the kernels are bitwise reproducible: the factor is for another compiler schedule),
#   rounded up to a power of two, at least 4.  The measured ratios stand beside the factors.
#   The largest ratios of the default projection -- 9.6 in P[0:2,2], 12.4 in K[0:2,2] -- come from family base behind sfm_loss_bwd
#   in the planar layout; every planted error of tests/test_intrinsics_exact_cpu.py still fails the rule under these factors (the
#   nearest: ssim_rate x 1.001 at 2.3 allowances).
MEASURED = {
    "reference_order": {"d_proj": 1.710, "P[0:2,0:2]": 1.012, "P[0:2,2]": 1.233, "P[0:2,3]": 1.335, "P[2,0:2]": 1.554, "P[2,2]": 2.382,
                        "P[2,3]": 3.376, "d_K": 1.488, "K[0:2,0:2]": 1.869, "K[0:2,2]": 2.388, "K[2,0:2]": 3.326, "K[2,2]": 1.641},
    "fast": {"d_proj": 2.586, "P[0:2,0:2]": 1.715, "P[0:2,2]": 9.591, "P[0:2,3]": 2.861, "P[2,0:2]": 4.079, "P[2,2]": 5.114,
             "P[2,3]": 3.619, "d_K": 4.049, "K[0:2,0:2]": 6.166, "K[0:2,2]": 12.385, "K[2,0:2]": 5.459, "K[2,2]": 5.515},
    "operator": {"d_K": 2.520, "K[0:2,0:2]": 1.932, "K[0:2,2]": 2.436, "K[2,0:2]": 4.165, "K[2,2]": 5.554},
}
FACTORS = {
    "reference_order": {"d_proj": 4, "P[0:2,0:2]": 8, "P[0:2,2]": 8, "P[0:2,3]": 8, "P[2,0:2]": 8, "P[2,2]": 16,
                        "P[2,3]": 16, "d_K": 4, "K[0:2,0:2]": 8, "K[0:2,2]": 16, "K[2,0:2]": 16, "K[2,2]": 8},
    "fast": {"d_proj": 16, "P[0:2,0:2]": 8, "P[0:2,2]": 64, "P[0:2,3]": 16, "P[2,0:2]": 32, "P[2,2]": 32,
             "P[2,3]": 16, "d_K": 32, "K[0:2,0:2]": 32, "K[0:2,2]": 64, "K[2,0:2]": 32, "K[2,2]": 32},
    "operator": {"d_K": 16, "K[0:2,0:2]": 8, "K[0:2,2]": 16, "K[2,0:2]": 32, "K[2,2]": 32},
}
K_REF = KF.K_REF
REGIMES = tuple(FACTORS)
YARDSTICK_MAX = KF.YARDSTICK_MAX       # max|o32 - o64| / max|o64| of every block


def derived_factor(ratio):
    """the stated rule: 4 x the largest measured ratio, rounded up to a power of two, at least 4"""
    return int(2 ** np.ceil(np.log2(max(4.0 * ratio, 4.0))))


# ---------------------------------------------------------------------------------------------------------------------------
# the fused loss
# ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(shape, seed):
    return KF.make_inputs(shape, seed, KIND)


@functools.lru_cache(maxsize=None)
def inputs(shape, seed):
    """computed once and shared: never modified"""
    return make_inputs(shape, seed)


def oracle(d, cfg, dtype, **weights):
    """oracle.sfm_loss on the float32 inputs d in `dtype` with d_proj and the intermediates the knife conditions read; `weights`
    override entries of cfg"""
    return O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True, keep_warped=True,
                      want_d_proj=True, dtype=dtype, **dict(cfg, **weights))


def d_k(d, d_proj):
    """the closed form in float64 on a d_proj of either precision (see the module docstring)"""
    return IG.d_k_from_d_proj(d["intrinsics"], d["poses"], d_proj)


def statement(d, cfg, dtype, **weights):
    """-> dict d_proj (B,S,n,3,4) as float64 values of the `dtype` evaluation, d_K (B,S,3,3), res: the oracle's whole result"""
    res = oracle(d, cfg, dtype, **weights)
    assert res["d_proj"].dtype == dtype
    d_proj = np.asarray(res["d_proj"], F64)
    return dict(d_proj=d_proj, d_K=d_k(d, d_proj), res=res)


@functools.lru_cache(maxsize=None)
def references(shape, seed, cfg_name):
    """(r64, r32) of one case under one configuration, computed once and shared: never modified"""
    d = inputs(shape, seed)
    return statement(d, CONFIGS[cfg_name], F64), statement(d, CONFIGS[cfg_name], F32)


@functools.lru_cache(maxsize=None)
def second_opinion(shape, seed, cfg_name):
    """torch autograd in float64 with K a leaf: d_K and d_proj"""
    return IG.autograd_loss(inputs(shape, seed), CONFIGS[cfg_name], want_gq=True)


def _cut(a, rows, cols):
    return a[..., rows, cols]


def proj_rows(got, a64, a32):
    """[(kind, name, got, o64, o32)] of a d_proj (B,S,n,3,4): per scale the whole array and its six blocks, all sources together"""
    out = []
    for s in range(a64.shape[1]):
        g, x, y = got[:, s], a64[:, s], a32[:, s]
        out.append(("d_proj", "d_proj[:, %d]" % s, g, x, y))
        out += [(kind, "d_proj[:, %d] %s" % (s, kind), _cut(g, *rc), _cut(x, *rc), _cut(y, *rc)) for kind, rc in PROJ_BLOCKS.items()]
    return out


def k_rows(got, a64, a32):
    """the same for a d_K (B,S,3,3), or (N,3,3) of the operator: per scale the whole array and its four blocks"""
    if a64.ndim == 3:
        got, a64, a32 = got[:, None], a64[:, None], a32[:, None]
    out = []
    for s in range(a64.shape[1]):
        g, x, y = got[:, s], a64[:, s], a32[:, s]
        out.append(("d_K", "d_K[:, %d]" % s, g, x, y))
        out += [(kind, "d_K[:, %d] %s" % (s, kind), _cut(g, *rc), _cut(x, *rc), _cut(y, *rc)) for kind, rc in K_BLOCKS.items()]
    return out


def rows(got_proj, got_k, r64, r32):
    """every compared array of one launch of the fused loss"""
    return proj_rows(np.asarray(got_proj, F64), r64["d_proj"], r32["d_proj"]) + k_rows(np.asarray(got_k, F64), r64["d_K"], r32["d_K"])


def outside(rows_, k_of):
    """[(name, distance / allowance)] of the rows that miss knife_free.rule with the factor k_of[kind] (kinds k_of lacks: not looked at)"""
    out = []
    for kind, name, got, a64, a32 in rows_:
        if kind in k_of:
            err, allow = KF.distances(got, a64, a32)[0], KF.allowance(a64, a32, k_of[kind])
            if err > allow:
                out.append((name, err / allow))
    return out


def factor_sets():
    """{name: k_of} of every set of factors a plant has to fail under: K_REF on every kind, and each regime's committed factors"""
    sets = {"K_REF on every kind": {kind: K_REF for kind in KINDS}}
    sets.update(FACTORS)
    return sets


def yardsticks(r64, r32):
    """[(name, max|o32 - o64| / max|o64|)] of every row"""
    out = []
    for _, name, _, a64, a32 in rows(r64["d_proj"], r64["d_K"], r64, r32):
        _, dev, top = KF.distances(a64, a64, a32)
        out.append((name, dev / top if top > 0 else float("inf")))
    return out


def failed_conditions(shape, seed, cfg_names=tuple(CONFIGS)):
    """the conditions of tests/test_intrinsics_exact_cpu.py that (shape, seed) misses, as strings (empty: the case may be used):
    knife_free's conditions 1-3 under knife_free.SEARCH_CONFIG first (cheap), then under every configuration of `cfg_names` in both
    precisions, with the yardstick of every block"""
    bad = KF.failed_conditions(shape, seed, with_yardstick=False, kind=KIND)
    if bad:
        return bad
    d = make_inputs(shape, seed)
    for name in cfg_names:
        pair = statement(d, CONFIGS[name], F64), statement(d, CONFIGS[name], F32)
        for r, prec in zip(pair, ("float64", "float32")):
            bad += ["%s: %d %s pixels (%s oracle)" % (name, n, k, prec) for k, n in KF.knife_pixels(d, r["res"]).items() if n]
            bad += ["%s: masked share %.3f at scale %d (%s)" % (name, share, s, prec) for s, share in enumerate(KF.masked_shares(r["res"]))
                    if not KF.MASKED_SHARE[0] <= share <= KF.MASKED_SHARE[1]]
        bad += ["%s: yardstick of %s is %.3g of its maximum" % (name, what, y) for what, y in yardsticks(*pair) if not 0 < y <= YARDSTICK_MAX]
    return bad


def search(shape, first_seed, n, want=2):
    """the first `want` seeds in [first_seed, first_seed + n) that pass failed_conditions: how the seeds of CASES were found"""
    found = []
    for seed in range(first_seed, first_seed + n):
        if not failed_conditions(shape, seed):
            found.append(seed)
            if len(found) == want:
                break
    return found


# ---------------------------------------------------------------------------------------------------------------------------
# planted errors, float64: each returns dict(d_proj, d_K) as `statement` does, with one error
# ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def swapped_sampler_weights():
    """oracle.spatial_transformer_sampler_backward with wx0 <-> wx1 and wy0 <-> wy1 at every pixel (the forward pass keeps its own)"""
    real_bwd, real_coords = O.spatial_transformer_sampler_backward, O._sampler_coords

    def coords(*a):
        u, v, u0, v0, u1, v1, wx0, wx1, wy0, wy1 = real_coords(*a)
        return u, v, u0, v0, u1, v1, wx1, wx0, wy1, wy0

    def bwd(*a, **kw):
        O._sampler_coords = coords
        try:
            return real_bwd(*a, **kw)
        finally:
            O._sampler_coords = real_coords
    O.spatial_transformer_sampler_backward = bwd
    try:
        yield
    finally:
        O.spatial_transformer_sampler_backward = real_bwd


def plant_swapped_weights(d, cfg):
    """(a) the sampler's gu and gv with the two weights of each swapped: on an affine image the four tap differences of a cell are
    equal and the weights do not matter; on a texture this is an error of order one"""
    with swapped_sampler_weights():
        return statement(d, cfg, F64)


PLANT_WEIGHT = "ssim_rate"       # the one loss weight that reaches d_proj (smooth_reg and exp_reg reach d_disp and d_mask only)


def plant_weight(d, cfg):
    """(b) ssim_rate times 1.001 (tests/test_knife_free_cpu.py, condition 5); None for a configuration without the SSIM term"""
    if not cfg.get(PLANT_WEIGHT):
        return None
    return statement(d, cfg, F64, **{PLANT_WEIGHT: cfg[PLANT_WEIGHT] * 1.001})


def plant_no_inverse_route(d, r64, source=0):
    """(c) d_K without its second route -- the one through K^-1 in pixel2cam -- for one source at the last scale only"""
    K, g = np.asarray(d["intrinsics"], F64)[:, -1:], r64["d_proj"][:, -1:]
    R_, _ = IG.rt(d["poses"][source])
    Rt = np.transpose(R_, (0, 2, 1))[:, None]
    route = np.transpose(np.linalg.inv(K), (0, 1, 3, 2)) @ Rt @ np.transpose(K, (0, 1, 3, 2)) @ g[:, :, source, :, :3]
    d_K = r64["d_K"].copy()
    d_K[:, -1:] += route
    return dict(d_proj=r64["d_proj"], d_K=d_K)


# ---------------------------------------------------------------------------------------------------------------------------
# the operator: sfm_warp_intrinsics_bwd
# ---------------------------------------------------------------------------------------------------------------------------
# warp_exact_ref's operator cases (synth's own cameras), and under the general cameras the first two seeds that
# warp_exact_ref.search(shape, "general_cameras", 0, 40) finds (every source, one and three depth rows; the three-row draw is
# warp_exact_ref.ROWS_DRAWS' for the case, 0 where not listed)
GENERAL_SETTING = "general_cameras"
GENERAL_OPERATOR_CASES = R.case_list(R.GENERAL_CASES, GENERAL_SETTING)
OPERATOR_CASES = [(c, rows_, C, i) for c in R.CASE_LIST + GENERAL_OPERATOR_CASES for rows_, C in R.OPERATOR_FORMS for i in range(c[0][3])]
OPERATOR_CASES += [(R.OPERATOR_C5_CASE, rows_, 5, 0) for rows_ in (1, 3)]


def op_ident(v):
    c, rows_, C, i = v
    return "%s-rows%d-C%d-src%d" % (R.ident(c), rows_, C, i)


@functools.lru_cache(maxsize=None)
def operator_references(v):
    """(d_K in float64, d_K in float32) (N,3,3) of intrinsics_grad.autograd_warp on one operator case, computed once and shared"""
    (shape, seed, setting), rows_, C, i = v
    imgs, depthes, _, pose, K, g = R.operator_inputs(R.inputs(shape, seed, setting), rows_, C, i)
    return tuple(IG.autograd_warp(imgs, depthes, pose, K, g, dtype) for dtype in ("float64", "float32"))


def operator_closed_form(v, dtype=F64):
    """one depth row: the closed form (float64) on the gPm of oracle.projective_inverse_warp_backward evaluated in `dtype`"""
    (shape, seed, setting), rows_, C, i = v
    assert rows_ == 1
    imgs, depthes, _, pose, K, g = R.operator_inputs(R.inputs(shape, seed, setting), rows_, C, i)
    gPm = O.projective_inverse_warp_backward(imgs, depthes, pose, K, g, dtype, want_gPm=True)[3]
    return IG.d_k_from_d_proj(K[:, None], [pose], np.asarray(gPm, F64)[:, None, None, :3])[:, 0]
