"""Non-finite and absurd GEOMETRY inputs -- a disparity, a depth, a pose entry, an intrinsics entry, a sampler grid entry, an
upstream gradient -- for every kernel that turns such a number into a memory address: the catalogue, the helpers that compare
results element by element, the integer part of the three address-forming functions restated with C semantics, and the table of
the places where the kernels deliberately differ from the project's float32 NumPy statements.

Host only: no device, no library call.  tests/test_hostile_inputs_cpu.py proves from these statements alone that no catalogue input
forms an index outside the image or its zero frame, and that the float32 statements deviate from the kernels' clamps only where
DEVIATIONS says so; tests/test_hostile_inputs_gpu.py runs the kernels on the same catalogue.

Every case starts from a clean input the suite already holds to float64 (tests/warp_exact_ref.py, tests/knife_free.py,
tests/test_ops_edges_gpu.py), with B = 2.  ONE entry of sample 0 is overwritten (the sampler grids: one entry in fifty of sample
0); sample 1 is never touched, so that every per-sample output of sample 1 must keep the bits of the clean run.

C SEMANTICS.  fmaxf(NaN, 0) = 0 and fminf(NaN, 0) = 0 -- the non-NaN operand -- where np.clip keeps the NaN.  The kernels clamp
with fminf(fmaxf(x, lo), hi): a NaN becomes `lo`.  Everything below that restates kernel code uses np.fmax / np.fmin (which have
the C semantics), never np.clip, and `c_int` stands for the C conversion `(int)x`, which is undefined for a NaN, an infinity or
|x| >= 2^31: it REPORTS such operands instead of converting them."""
import collections
import contextlib
import functools
import zlib

import numpy as np

import knife_free as KF
import warp_exact_ref as R
from oracle import sfm_oracle as O

F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")

# ---------------------------------------------------------------------------------------------------------------------------
# helpers of the comparisons
# ---------------------------------------------------------------------------------------------------------------------------
FINITE, POS_INF, NEG_INF, IS_NAN = 0, 1, 2, 3


def classes(a):
    """each element -> FINITE, POS_INF, NEG_INF or IS_NAN (int8, the shape of a)"""
    a = np.asarray(a)
    out = np.zeros(a.shape, np.int8)
    out[np.isposinf(a)] = POS_INF
    out[np.isneginf(a)] = NEG_INF
    out[np.isnan(a)] = IS_NAN
    return out


def same_numbers(a, b):
    """equality of VALUES: NaN == NaN (whatever the payload) and -0 == +0"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def same_bits(a, b):
    """bitwise equality of two float32 arrays (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32), b.view(np.int32)))


def _copy(v):
    if isinstance(v, np.ndarray):
        return v.copy()
    if isinstance(v, (list, tuple)):
        return type(v)(_copy(x) for x in v)
    return v


def corrupt(case, what, where, value):
    """A deep copy of the input dict `case` with ONE entry overwritten: what = "key" or ("key", k) for the k-th array of a list,
    where = the index of the entry in that array (its first component is the sample: always 0), value = the float written.
    where = a boolean / integer index array selects several entries of sample 0 and `value` is then an array of that many values
    (the sampler grids)."""
    out = {k: _copy(v) for k, v in case.items()}
    key, k = what if isinstance(what, tuple) else (what, None)
    a = out[key] if k is None else out[key][k]
    assert isinstance(a, np.ndarray) and a.dtype == F32, (what, type(a))
    if isinstance(where, tuple):
        assert where[0] == 0, "only sample 0 is ever corrupted"
        a[where] = F32(value)
    else:
        a[0].reshape(-1)[np.asarray(where)] = np.asarray(value, F32)
    return out


def stack2(d):
    """a B = 1 input dict with its sample repeated: B = 2, sample 1 the clean copy"""
    def rep(v):
        if isinstance(v, np.ndarray):
            assert v.shape[0] == 1, v.shape
            return np.ascontiguousarray(np.concatenate([v, v], axis=0))
        if isinstance(v, list):
            return [rep(x) for x in v]
        return v
    out = {k: rep(v) for k, v in d.items()}
    if "B" in out:
        out["B"] = 2
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the values
# ---------------------------------------------------------------------------------------------------------------------------
# a disparity (sfm_warp_*: a depth)
DISP_VALUES = collections.OrderedDict([
    ("nan", NAN), ("+inf", INF), ("-inf", -INF), ("+0", 0.0), ("-0", -0.0), ("negative", -0.5), ("denormal", 1e-40), ("1e-30", 1e-30),
    ("1e30", 1e30)])
POSE_VALUES = collections.OrderedDict([("nan", NAN), ("+inf", INF), ("1e30", 1e30)])
GRID_VALUES = (NAN, INF, -INF, 1e30, -1e30, 3e9, -3e9)      # 3e9: beyond the `int` range after scaling, and before it
UPSTREAM_VALUES = collections.OrderedDict([("nan", NAN), ("+inf", INF)])
# (the extreme but FINITE values: EXTREME_FINITE, below the catalogue)

Hostile = collections.namedtuple("Hostile", "group base what where value tag per_pixel")
#   group     which statement / entry points the case belongs to ("sampler", "interp", "warp", "loss")
#   base      the key of the clean input (BASES[group])
#   per_pixel for a corrupted disparity / depth / upstream pixel: (scale, flat pixel index) -- what locality (2c) exempts; else None


def hid(h):
    return "%s-%s-%s" % (h.group, h.base, h.tag)


# ---------------------------------------------------------------------------------------------------------------------------
# clean inputs
# ---------------------------------------------------------------------------------------------------------------------------
WARP_BASES = {"13x21": ((2, 13, 21, 2, 1), R.CASES[(2, 13, 21, 2, 1)][0]), "24x40": ((1, 24, 40, 3, 3), R.CASES[(1, 24, 40, 3, 3)][0])}
LOSS_BASES = {"32x48": ((2, 32, 48, 2, 3), 12), "37x70": ((1, 37, 70, 2, 1), 16)}
# (family of tests/test_ops_edges_gpu.py::make_field, C, H, W, oH, oW), N = 2: C on both sides of SAMPLER_BWD_MAXC = 4
SAMPLER_BASES = {"C3": ("edges", 3, 9, 65, 8, 64), "C5": ("edges", 5, 5, 9, 7, 63)}
MIN_CHUNK_ROWS = 4      # csrc/sfm_loss_kernels.h: small launches are cut into chunks of four rows
WARP_BLOCK = 256        # csrc/sfm_ops.hip, sfm_warp_pyramid.hip: pixels per block


@functools.lru_cache(maxsize=None)
def warp_base(name):
    """tests/warp_exact_ref.py's inputs (default conventions) at B = 2: never modified"""
    shape, seed = WARP_BASES[name]
    d = R.inputs(shape, seed, "default")
    return d if shape[0] == 2 else stack2(d)


@functools.lru_cache(maxsize=None)
def loss_base(name):
    """tests/knife_free.py's inputs at B = 2: never modified"""
    shape, seed = LOSS_BASES[name]
    d = KF.inputs(shape, seed)
    return d if shape[0] == 2 else stack2(d)


@functools.lru_cache(maxsize=None)
def sampler_base(name):
    """x (2,C,H,W), grid (2,2,oH,oW) of the "edges" family (values at +-1 and at the padded edges among random ones within +-1.3),
    grid_px: the same positions in pixel units (sfm_sampler_interp_*), gy (2,C,oH,oW): never modified"""
    import test_ops_edges_gpu as E
    case = SAMPLER_BASES[name]
    family, C, H, W, oH, oW = case
    rng = np.random.RandomState(zlib.crc32(repr(case).encode()))
    x = rng.uniform(-1, 1, size=(2, C, H, W)).astype(F32)
    grid = E.make_field(family, 2, H, W, oH, oW, rng)
    gy = rng.normal(size=(2, C, oH, oW)).astype(F32)
    px = np.stack([(grid[:, 0] + 1) * F32((W - 1) / 2.0), (grid[:, 1] + 1) * F32((H - 1) / 2.0)], axis=1).astype(F32)
    return dict(x=x, grid=grid, grid_px=np.ascontiguousarray(px), gy=gy)


BASES = {"warp": warp_base, "loss": loss_base, "sampler": sampler_base, "interp": sampler_base}


def inputs_of(h):
    """the corrupted input dict of a catalogue case"""
    return corrupt(BASES[h.group](h.base), h.what, h.where, h.value)


# ---------------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------------
def _grid_mix(n_entries):
    """(flat indices into sample 0's (2, oH, oW) grid, values): one entry in fifty, GRID_VALUES in turn; 50 is even and the first
    index odd in neither component's favour: offsets 7, 57, ... land in the x half and in the y half of the flattened array"""
    idx = np.arange(7, n_entries, 50)
    return idx, np.array([GRID_VALUES[k % len(GRID_VALUES)] for k in range(idx.size)], F32)


def _sampler_catalogue():
    out = []
    for group, key in (("sampler", "grid"), ("interp", "grid_px")):
        for base, (_, C, H, W, oH, oW) in SAMPLER_BASES.items():
            idx, vals = _grid_mix(2 * oH * oW)
            assert (idx < oH * oW).any() and (idx >= oH * oW).any(), "both components"
            out.append(Hostile(group, base, key, idx, vals, "grid_mix", None))
            for k, v in enumerate(GRID_VALUES):      # ... and each value alone, once per component
                comp = k % 2
                out.append(Hostile(group, base, key, (0, comp, oH // 2, oW // 3), v, "grid_%s_%s" % ("xy"[comp], _name(v)), None))
            for name, v in UPSTREAM_VALUES.items():
                out.append(Hostile(group, base, "gy", (0, C - 1, oH - 1, 1), v, "gy_%s" % name, None))
    return out


def _name(v):
    return "nan" if v != v else ("%+g" % v).replace("+inf", "+inf")


def warp_pixels(P):
    """0, both sides of the seam between the first two blocks, the last lane of the last (partial) block"""
    return (0, WARP_BLOCK - 1, WARP_BLOCK, P - 1)


def _warp_catalogue():
    out = []
    for base, (shape, _) in WARP_BASES.items():
        _, H, W, n_src, S = shape
        P = H * W
        for name, v in DISP_VALUES.items():
            for p in warp_pixels(P):
                out.append(Hostile("warp", base, ("disps", 0), (0, 0, p // W, p % W), v, "disp_%s_px%d" % (name, p), (0, p)))
        for name, v in POSE_VALUES.items():
            out.append(Hostile("warp", base, ("poses", 0), (0, 1), v, "rot_%s" % name, None))
            out.append(Hostile("warp", base, ("poses", n_src - 1), (0, 5), v, "trans_%s" % name, None))
        out += _intrinsics_cases("warp", base)
        for name, v in UPSTREAM_VALUES.items():
            out.append(Hostile("warp", base, ("g", 0), (0, 0, 1, H // 2, W // 2), v, "g_%s" % name, (0, (H // 2) * W + W // 2)))
            out.append(Hostile("warp", base, "g_op", (0, 0, 1, H // 2, W // 2), v, "g_op_%s" % name, (0, (H // 2) * W + W // 2)))
    return out


def _intrinsics_cases(group, base):
    """an entry NaN; a zero row (singular); focal length 0; focal length 1e30 -- at scale 0 of sample 0"""
    return [Hostile(group, base, "intrinsics", (0, 0, 0, 2), NAN, "K_nan", None),
            Hostile(group, base, "intrinsics", (0, 0, 2), 0.0, "K_zero_row", None),
            Hostile(group, base, "intrinsics", (0, 0, 0, 0), 0.0, "K_focal_0", None),
            Hostile(group, base, "intrinsics", (0, 0, 0, 0), 1e30, "K_focal_1e30", None)]


def loss_pixels(shape):
    """(scale, row, column): both sides of the seam between the first two chunks of four rows, in the columns 0 and W - 1, and one
    pixel of the coarsest scale"""
    _, H, W, _, S = shape
    px = [(0, MIN_CHUNK_ROWS - 1, 0), (0, MIN_CHUNK_ROWS, W - 1), (0, MIN_CHUNK_ROWS - 1, W // 2), (0, MIN_CHUNK_ROWS, W // 2)]
    if S > 1:
        hs, ws = H >> (S - 1), W >> (S - 1)
        px.append((S - 1, hs // 2, ws // 2))
    return px


def _loss_catalogue():
    out = []
    for base, (shape, _) in LOSS_BASES.items():
        _, H, W, n_src, S = shape
        for name, v in DISP_VALUES.items():
            for s, y, x in loss_pixels(shape):
                ws = W >> s
                out.append(Hostile("loss", base, ("disps", s), (0, 0, y, x), v, "disp_%s_s%d_y%d_x%d" % (name, s, y, x), (s, y * ws + x)))
        for name, v in POSE_VALUES.items():
            out.append(Hostile("loss", base, ("poses", 0), (0, 1), v, "rot_%s" % name, None))
            out.append(Hostile("loss", base, ("poses", n_src - 1), (0, 5), v, "trans_%s" % name, None))
        out += _intrinsics_cases("loss", base)
    return out


# The extreme but FINITE values.  tests/test_hostile_inputs_cpu.py proves two conditions of each from the oracle alone: the float32
# oracle forms no non-finite intermediate on it (no floating-point exception anywhere, forward and backward), and the float32 and the
# float64 oracle agree on the in-view set, every pixel whose projection the value moves lying at least EXTREME_MARGIN (normalised
# units) from the strict in-view test.  A value that fails is REPLACED by one that passes:
#   * a disparity of 1e30: the smoothness terms overflow float32 (differences of 1e30 times their weights)  -> 1e15
#   * a disparity of 1e-30 is a depth of 1e30: 0 x inf in the backward's -gD / disp^2                        -> 1e-15, and only
#     where the pixel leaves the view in every source (32x48, row 3, column 0): in view, d_disp = -gD / disp^2 of such a pixel is
#     the difference of numbers 1e30 apart, and the float32 oracle is 4 % .. 1e8 away from the float64 one -- no yardstick (37x70: no
#     catalogue pixel leaves both views)
#   * a translation of 1e30: tz passes at 32x48 (every pixel of the source lands on the epipole); at 37x70 the epipole lies on a
#     cell boundary of the bilinear lattice and ALL pixels of the source are knife pixels of tests/test_loss_gpu.py  -> tx there (every
#     pixel of the source leaves the view)
#   * a focal length of 1e30: passes at the coarsest scale of the three-scale case (every pixel leaves the view by 4e-3 and more);
#     at scale 0 of either case a pixel lands within 1.5e-4 .. 3.3e-4 of the border                           -> the coarsest scale only
#   * an Euler angle of 1e30 (pi after the clip): a rotation by pi re-lands every pixel, and in the loss cases (2000 pixels and
#     more per sample) some pixel always lands within 1e-3 of the border -- the best of the twelve (source, axis, sign) choices
#     reaches 5.3e-4 --; on the warp operator's 13x21 case (273 pixels) source 0, axis y reaches 3.3e-3        -> the operator, 13x21
EXTREME_MARGIN = 1e-3


def _extreme_finite():
    out = []
    for base, (shape, _) in LOSS_BASES.items():
        _, H, W, n_src, S = shape
        out.append(Hostile("loss", base, ("disps", 0), (0, 0, MIN_CHUNK_ROWS, W // 2), 1e15, "extreme_disp_1e15", (0, MIN_CHUNK_ROWS * W + W // 2)))
        if base == "32x48":
            out.append(Hostile("loss", base, ("disps", 0), (0, 0, MIN_CHUNK_ROWS - 1, 0), 1e-15, "extreme_disp_1e-15", (0, (MIN_CHUNK_ROWS - 1) * W)))
        out.append(Hostile("loss", base, ("poses", n_src - 1), (0, 5 if base == "32x48" else 3), 1e30, "extreme_trans_1e30", None))
        if S > 1:
            out.append(Hostile("loss", base, "intrinsics", (0, S - 1, 0, 0), 1e30, "extreme_focal_1e30", None))
    out.append(Hostile("warp", "13x21", ("poses", 0), (0, 1), 1e30, "extreme_angle_1e30", None))
    return out


EXTREME_FINITE = _extreme_finite()

CATALOGUE = _sampler_catalogue() + _warp_catalogue() + _loss_catalogue()
assert len(set(map(hid, CATALOGUE + EXTREME_FINITE))) == len(CATALOGUE) + len(EXTREME_FINITE)


def catalogue(group, **match):
    return [h for h in CATALOGUE if h.group == group and all(getattr(h, k) == v for k, v in match.items())]


# ---------------------------------------------------------------------------------------------------------------------------
# the integer part of the address-forming functions, with C semantics
# ---------------------------------------------------------------------------------------------------------------------------
INT_MAX = 2 ** 31


def c_int(x):
    """(int)x for float32 x -> (values as int64, convertible): `convertible` is False where the C conversion is undefined (NaN,
    infinities, |x| >= 2^31); the value there is 0 and must not be used"""
    x = np.asarray(x, F32)
    ok = np.isfinite(x) & (np.abs(x) < INT_MAX)
    return np.where(ok, np.trunc(np.where(ok, x, 0)), 0).astype(np.int64), ok


def c_clamp(x, lo, hi):
    """fminf(fmaxf(x, lo), hi): a NaN becomes lo"""
    return np.fmin(np.fmax(np.asarray(x, F32), F32(lo)), F32(hi)).astype(F32)


def pad_taps_c(gx, gy, H, W):
    """csrc/sfm_warp_pixel.h pad_taps, its integer part: -> (u0, v0 in PADDED coordinates, convertible).  The four taps are
    (v0 + a, u0 + b), a, b in {0, 1}: pad_read / HwcImage3::texel / the d_src scatter load or store only where pad_inside holds,
    so every tap must lie in [0, H+1] x [0, W+1] -- inside the image or on its one-pixel zero frame."""
    with np.errstate(all="ignore"):
        gx, gy = np.asarray(gx, F32), np.asarray(gy, F32)
        up = (gx + F32(1)) * F32(W - 1) * F32(0.5) + F32(1)
        vp = (gy + F32(1)) * F32(H - 1) * F32(0.5) + F32(1)
        uc, vc = c_clamp(up, 0, W + 1), c_clamp(vp, 0, H + 1)
        fu, ok_u = c_int(np.floor(uc))
        fv, ok_v = c_int(np.floor(vc))
    u0 = np.minimum(np.maximum(fu, 0), W)
    v0 = np.minimum(np.maximum(fv, 0), H)
    return u0, v0, ok_u & ok_v


def interp_taps_c(u, v, H, W):
    """csrc/sfm_ops.hip interp_taps, its integer part: -> (u0, v0, u1, v1, convertible); all four index the image directly, so each
    must lie in [0, W-1] / [0, H-1]"""
    with np.errstate(all="ignore"):
        u, v = np.asarray(u, F32), np.asarray(v, F32)
        u0, v0 = np.floor(u), np.floor(v)
        u1, v1 = u0 + F32(1), v0 + F32(1)
        parts = [c_int(c_clamp(a, 0, n - 1)) for a, n in ((u0, W), (v0, H), (u1, W), (v1, H))]
    return tuple(p[0] for p in parts) + (np.logical_and.reduce([p[1] for p in parts]),)


def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 operands: the product is exact in float64"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def project_q_c(q0, q1, q2, H, W):
    """csrc/sfm_common.h project_q, its integer part: -> (u0, v0, inview, convertible).  The conversion (int)U is applied to every
    lane and SELECTED by inview (v_cvt_i32_f32 saturates and maps NaN to 0: the select discards it); `convertible` therefore
    covers the in-view lanes only.  In view the taps (v0 + a, u0 + b) must lie inside the image: u0 in [0, W-2], v0 in [0, H-2]."""
    with np.errstate(all="ignore"):
        q0, q1, q2 = (np.asarray(a, F32) for a in (q0, q1, q2))
        z = q2 + F32(1e-10)
        rz = (F32(1) / z).astype(F32)
        div_r = lambda a: _fma32(_fma32(-(a * rz), z, a), rz, a * rz)
        U, V = div_r(q0), div_r(q1)
        su, sv = U * (F32(W - 1) - U), V * (F32(H - 1) - V)
        inview = (su > 0) & (sv > 0)
        iu, ok_u = c_int(U)
        iv, ok_v = c_int(V)
    u0, v0 = np.where(inview, iu, 0), np.where(inview, iv, 0)
    return u0, v0, inview, (ok_u & ok_v) | ~inview


def euler_matrix_c(r):
    """csrc/sfm_common.h euler2mat on (N,3) float32 angles: the clip is fminf(fmaxf(r, -pi), pi) -- a NaN angle becomes -pi"""
    pi = F32(np.pi)
    rc = c_clamp(r, -pi, pi)
    c, s = np.cos(rc).astype(F32), np.sin(rc).astype(F32)
    N = rc.shape[0]
    z, o = np.zeros(N, F32), np.ones(N, F32)
    Z = np.stack([c[:, 2], -s[:, 2], z, s[:, 2], c[:, 2], z, z, z, o], 1).reshape(N, 3, 3)
    Y = np.stack([c[:, 1], z, s[:, 1], z, o, z, -s[:, 1], z, c[:, 1]], 1).reshape(N, 3, 3)
    X = np.stack([o, z, z, z, c[:, 0], -s[:, 0], z, s[:, 0], c[:, 0]], 1).reshape(N, 3, 3)
    return O._bmm(O._bmm(X, Y), Z)


def geom_c(pose6, K):
    """make_geom / geom_from_T (csrc/sfm_common.h) in float32: -> (P (N,3,4) = K . [R|t], Kinv (N,3,3), M = P[:, :, :3] . Kinv)"""
    with np.errstate(all="ignore"):
        pose6, K = np.asarray(pose6, F32), np.asarray(K, F32)
        T = np.concatenate([euler_matrix_c(pose6[:, :3]), pose6[:, 3:, None]], axis=2)
        P = O._bmm(K, T)
        Kinv = O.batch_inv3(K)
        return P, Kinv, O._bmm(P[:, :, :3], Kinv)


def _pix(H, W):
    ys, xs = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    return xs.reshape(-1), ys.reshape(-1)


def ref_project_grid_c(pose6, K, depth, H, W):
    """ref_project (csrc/sfm_warp_pixel.h) in float32 for depth (N, H*W): the grid coordinates (gx, gy), each (N, H*W), that the
    reference-order paths hand to pad_taps"""
    with np.errstate(all="ignore"):
        P, Kinv, _ = geom_c(pose6, K)
        x, y = _pix(H, W)
        ray = [(Kinv[:, j, 0:1] * x + Kinv[:, j, 1:2] * y) + Kinv[:, j, 2:3] for j in range(3)]
        c = [np.asarray(depth, F32) * r for r in ray]
        q = [((P[:, k, 0:1] * c[0] + P[:, k, 1:2] * c[1]) + P[:, k, 2:3] * c[2]) + P[:, k, 3:4] for k in range(3)]
        z = q[2] + F32(1e-10)
        xn = (q[0] / z) / F32((W - 1) / 2.0) - F32(1)
        yn = (q[1] / z) / F32((H - 1) / 2.0) - F32(1)
        mx = np.where((xn > -1) & (xn < 1), F32(1), F32(2))
        my = np.where((yn > -1) & (yn < 1), F32(1), F32(2))
        return (xn * mx).astype(F32), (yn * my).astype(F32)


def ref_cell_c(gx, gy, H, W):
    """the reference-order projection of the fused loss (csrc/sfm_ssim_pass.h ref_position / ref_proj_cell), its integer part, from
    ref_project's grid coordinates: in view iff both lie strictly inside (-1, 1) (a doubled or NaN coordinate does not); the cell
    is floor(up) - 1 of the sampler's padded position, folded onto [.., W-2] -> (u0, v0, inview, convertible); in view the taps
    (v0 + a, u0 + b) must lie inside the image"""
    with np.errstate(all="ignore"):
        gx, gy = np.asarray(gx, F32), np.asarray(gy, F32)
        inview = (F32(1) - gx * gx > 0) & (F32(1) - gy * gy > 0)
        up = ((gx + F32(1)) * F32(W - 1)) * F32(0.5) + F32(1)
        vp = ((gy + F32(1)) * F32(H - 1)) * F32(0.5) + F32(1)
        iu, ok_u = c_int(np.floor(up) - F32(1))
        iv, ok_v = c_int(np.floor(vp) - F32(1))
    u0 = np.where(inview, np.minimum(iu, W - 2), 0)
    v0 = np.where(inview, np.minimum(iv, H - 2), 0)
    return u0, v0, inview, (ok_u & ok_v) | ~inview


def fast_project_q_c(pose6, K, disp, H, W):
    """the default projection of the fused loss (csrc/sfm_common.h project): q = D (M . pix) + P[:, 3], D = 1 / disp, for
    disp (N, H*W) -> (q0, q1, q2), each (N, H*W)"""
    with np.errstate(all="ignore"):
        P, _, M = geom_c(pose6, K)
        x, y = _pix(H, W)
        D = (F32(1) / np.asarray(disp, F32)).astype(F32)
        a = [_fma32(M[:, k, 1:2], y, _fma32(M[:, k, 0:1], x, M[:, k, 2:3])) for k in range(3)]
        return tuple(_fma32(D, a[k], P[:, k, 3:4]) for k in range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# the float32 statements, and the same statements with the kernels' clamps
# ---------------------------------------------------------------------------------------------------------------------------
class _CClampNumpy:
    """numpy with ONE function replaced: clip(x, lo, hi) = fmin(fmax(x, lo), hi), the C clamp (a NaN becomes lo) -- for the clips the
    deviations in `on` name only: the Euler angle clip has a negative lower bound (-pi), the sampler's clips start at 0"""

    def __init__(self, on):
        self._euler, self._sampler = "nan_euler_angle_is_minus_pi" in on, "nan_position_reads_the_zero_frame" in on

    def __getattr__(self, name):
        return getattr(np, name)

    def clip(self, x, lo, hi, **kw):
        if (self._euler if np.all(np.asarray(lo) < 0) else self._sampler):
            return np.fmin(np.fmax(x, lo), hi)
        return np.clip(x, lo, hi)


@contextlib.contextmanager
def c_clamps(on=True):
    """on: True, or the names of the DEVIATIONS entries that apply.  Inside, the np.clip of oracle/sfm_oracle.py that an entry names
    -- the Euler angle clip (transform.py:23), the sampler's clip of the padded position -- has the C semantics of the kernels'
    fminf(fmaxf(.)); a clip no entry names stays NumPy's.  Nothing else of the oracle changes: the statement stays the
    project's own, with exactly the primitive swapped that DEVIATIONS names."""
    if not on:
        yield
        return
    saved = O.np
    O.np = _CClampNumpy(tuple(DEVIATIONS) if on is True else tuple(on))
    try:
        yield
    finally:
        O.np = saved


def _interp_parts_c(grid, H, W, dtype):
    """oracle._interp_parts with the C clamp (ndarray.clip is a method: c_clamps cannot reach it)"""
    u, v = grid[:, 0].reshape(-1), grid[:, 1].reshape(-1)
    u0, v0 = np.floor(u), np.floor(v)
    u1, v1 = u0 + 1, v0 + 1
    u0, v0, u1, v1 = (np.fmin(np.fmax(a, 0), n - 1) for a, n in ((u0, W), (v0, H), (u1, W), (v1, H)))
    return (u0.astype(np.int32), v0.astype(np.int32), u1.astype(np.int32), v1.astype(np.int32),
            (u1 - u).astype(dtype), (u - u0).astype(dtype), (v1 - v).astype(dtype), (v - v0).astype(dtype))


@contextlib.contextmanager
def _interp_c(on):
    saved = O._interp_parts
    if on:
        O._interp_parts = _interp_parts_c
    try:
        yield
    finally:
        O._interp_parts = saved


def sampler_statement(d, c=False):
    """oracle.spatial_transformer_sampler and its backward in float32 -> dict y, ggrid, gx"""
    with np.errstate(all="ignore"), c_clamps(c):
        y = O.spatial_transformer_sampler(d["x"], d["grid"])
        gx, ggrid = O.spatial_transformer_sampler_backward(d["x"], d["grid"], d["gy"])
    return dict(y=y, ggrid=ggrid, gx=gx)


def interp_statement(d, c=False):
    """oracle.interp_sampler_forward / _backward in float32 on the pixel-unit grid -> dict y, ggrid, gx (all zeros).  The NumPy
    statement cannot index with a NaN position (astype(int32) of a NaN is whatever the platform gives): with c=False a NaN position
    is a ValueError -- the reference has no value there; infinities and |x| >= 2^31 it clips like the kernel."""
    g = np.asarray(d["grid_px"], F32)
    if not c and np.isnan(g).any():
        raise ValueError("the reference's interp sampler cannot index with a NaN position")
    with np.errstate(all="ignore"), _interp_c(c):
        y = O.interp_sampler_forward(d["x"], g)
        gx, ggrid = O.interp_sampler_backward(d["x"], g, d["gy"])
    return dict(y=np.asarray(y, F32), ggrid=np.asarray(ggrid, F32), gx=np.asarray(gx, F32))


def operator_source(h):
    """the source sfm_warp_* is run on for a case of the group "warp": the one whose pose is corrupted, else source 0"""
    return h.what[1] if isinstance(h.what, tuple) and h.what[0] == "poses" else 0


def operator_arrays(h, depth_rows, C):
    """The arrays of one sfm_warp_fwd / _bwd / _intrinsics_bwd call on a case of the group "warp" (None: the clean input of base h):
    tests/warp_exact_ref.py's operator_inputs at scale 0.  sfm_warp_* takes a DEPTH: a case that corrupts the disparity of scale 0
    writes its value into the depth map instead (all three rows of the pixel).  -> dict imgs (B,C,H,W), depthes (B,3,P) as the
    oracle reads them, depth as the operator reads it ((B,P) or (B,3,P)), pose (B,6), K (B,3,3), g (B,C,H,W)"""
    as_depth = h.what == ("disps", 0)
    d = warp_base(h.base) if as_depth else inputs_of(h)
    imgs, depthes, dev_depth, pose, K, g = (np.array(a, F32) for a in R.operator_inputs(d, depth_rows, C, operator_source(h)))
    if as_depth:
        p = h.per_pixel[1]
        depthes[0, :, p] = F32(h.value)
        dev_depth[(0, slice(None), p) if depth_rows == 3 else (0, p)] = F32(h.value)
    return dict(imgs=imgs, depthes=depthes, depth=dev_depth, pose=pose, K=K, g=g)


def clean_operator_arrays(base, depth_rows, C, source):
    imgs, depthes, dev_depth, pose, K, g = (np.array(a, F32) for a in R.operator_inputs(warp_base(base), depth_rows, C, source))
    return dict(imgs=imgs, depthes=depthes, depth=dev_depth, pose=pose, K=K, g=g)


def warp_operator_statement(a, c=False):
    """oracle.projective_inverse_warp and its backward in float32 on the arrays of operator_arrays (what tests/warp_exact_ref.py's
    operator_reference evaluates) -> dict warped, valid (B,H,W), d_depth (B,rows,H,W), d_pose, d_src, and grid: what went to the sampler"""
    B, _, H, W = a["imgs"].shape
    rows = 3 if a["depth"].ndim == 3 else 1
    with np.errstate(all="ignore"), c_clamps(c):
        warped, aux = O.projective_inverse_warp(a["imgs"], a["depthes"], a["pose"], a["K"], F32, return_aux=True)
        g_dep, g_pose, g_img = O.projective_inverse_warp_backward(a["imgs"], a["depthes"], a["pose"], a["K"], a["g"], F32, want_gimgs=True)
    d_depth = (g_dep.sum(axis=1, keepdims=True) if rows == 1 else g_dep).reshape(B, rows, H, W)
    return dict(warped=warped, valid=(aux["mask"] == 1).all(axis=1).astype(F32).reshape(B, H, W), d_depth=d_depth.astype(F32),
                d_pose=g_pose, d_src=g_img, grid=aux["grid"])


def warp_pyramid_statement(d, c=False, backward=True):
    """tests/warp_exact_ref.py's reference in float32: every (scale, source) -> dict of per-scale lists warped, valid, d_disps and
    the per-source list d_poses"""
    with np.errstate(all="ignore"), c_clamps(c):
        ref = R.reference(d, F32, backward=backward)
        if backward:
            # d_pose from d_T = K^T . gPm through the ORACLE's Euler tail (proj_tgt_to_src_backward with K = 1): the same function as
            # warp_exact_ref's torch autograd on finite poses, and one whose clip c_clamps reaches
            assert d["fmt"] == "euler" and not any(d["invert"])
            eye = np.tile(np.eye(3, dtype=F32), (d["B"], 1, 1))
            pad = lambda t: np.concatenate([t, np.zeros((t.shape[0], 1, 4), F32)], axis=1).astype(F32)
            ref["d_poses"] = [O.proj_tgt_to_src_backward(p, eye, pad(t), F32) for p, t in zip(d["poses"], ref["d_T"])]
    return {k: ref[k] for k in (("warped", "valid", "d_disps", "d_poses") if backward else ("warped", "valid"))}


def loss_statement(d, cfg, c=False, backward=True, want_d_src=False):
    """oracle.sfm_loss in float32 -> its result dict"""
    with np.errstate(all="ignore"), c_clamps(c):
        return O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=backward,
                          want_d_src=want_d_src, keep_warped=True, dtype=F32, **cfg)


# ---------------------------------------------------------------------------------------------------------------------------
# the deliberate deviations of the kernels from the float32 statements
# ---------------------------------------------------------------------------------------------------------------------------
def has_nan_angle(h, d, grids=None):
    if h.group == "conv":
        return d["fmt"] == "euler" and any(np.isnan(np.asarray(p)[:, :3]).any() for p in d["poses"])
    return h.group in ("warp", "loss") and any(np.isnan(np.asarray(p)[:, :3]).any() for p in d["poses"])


def sampler_grid_of(h, d):
    """the grids the statement hands to its sampler on input d: [(grid_x, grid_y)] as flat float32 arrays"""
    if h.group in ("sampler", "interp"):
        g = d["grid" if h.group == "sampler" else "grid_px"]
        return [(g[:, 0].reshape(-1), g[:, 1].reshape(-1))]
    out = []
    with np.errstate(all="ignore"):
        for s, disp in enumerate(d["disps"]):
            hh, ww = disp.shape[2:]
            depth = (F32(1) / disp).reshape(disp.shape[0], -1)
            for p in d["poses"]:
                P = O.proj_tgt_to_src(p, d["intrinsics"][:, s], F32)      # (the reference's own clip: a NaN angle stays NaN)
                cam, _ = O.pixel2cam(np.broadcast_to(depth[:, None], (depth.shape[0], 3, hh * ww)),
                                     O.generate_2dmeshgrid(hh, ww, depth.shape[0], F32), d["intrinsics"][:, s], F32)
                grid, _ = O.cam2pixel(cam, P, hh, ww, F32)
                out.append((grid[:, 0].reshape(-1), grid[:, 1].reshape(-1)))
    return out


def has_nan_position(h, d, grids=None):
    if h.group == "conv" and grids is None:      # (under other conventions: the plain statement's warped is NaN exactly where its position is)
        with np.errstate(all="ignore"):
            return any(np.isnan(w).any() for w in R.reference(d, F32, backward=False)["warped"])
    grids = sampler_grid_of(h, d) if grids is None else grids
    return any(np.isnan(gx).any() or np.isnan(gy).any() for gx, gy in grids)


def _rcp_refined_c(b):
    """csrc/sfm_common.h rcp_refined: r = 1 / b with one residual correction -- NaN for an infinite b (0 x inf in the residual)"""
    with np.errstate(all="ignore"):
        b = np.asarray(b, F32)
        r = (F32(1) / b).astype(F32)
        return _fma32(_fma32(-b, r, F32(1)), r, r)


def loss_nan_positions(d, projection):
    """per scale the (B, n_src, h, w) bool array of the samples whose position the fused loss forms as NaN, from the float32
    restatements: the default projection's U = q0 / z, V = q1 / z (project_q), or the reference-order grid coordinates with the depth
    rcp_refined(disp) (ref_position)"""
    out = []
    with np.errstate(all="ignore"):
        for s, disp in enumerate(d["disps"]):
            B, _, h, w = disp.shape
            per = []
            for p in d["poses"]:
                if projection == "fast":
                    q0, q1, q2 = fast_project_q_c(p, d["intrinsics"][:, s], disp.reshape(B, -1), h, w)
                    z = q2 + F32(1e-10)
                    rz = (F32(1) / z).astype(F32)
                    div_r = lambda a: _fma32(_fma32(-(a * rz), z, a), rz, a * rz)
                    bad = np.isnan(div_r(q0)) | np.isnan(div_r(q1))
                else:
                    gx, gy = ref_project_grid_c(p, d["intrinsics"][:, s], _rcp_refined_c(disp.reshape(B, -1)), h, w)
                    bad = np.isnan(gx) | np.isnan(gy)
                per.append(bad.reshape(B, h, w))
            out.append(np.stack(per, axis=1))
    return out


# name -> (the header line that documents it, applies(h, corrupted inputs) from the STATEMENT alone, what the kernels do)
DEVIATIONS = collections.OrderedDict([
    ("nan_position_reads_the_zero_frame", dict(
        header="include/sfmwarp.h",
        line="a NaN grid coordinate is clamped to the first column / row of the zero frame",
        applies=has_nan_position,
        what="pad_taps / interp_taps clamp with fminf(fmaxf(.)): a NaN coordinate becomes 0 where np.clip keeps it, so the sample "
             "and its gradient share are exactly 0 where the reference's formula gives NaN")),
    ("nan_euler_angle_is_minus_pi", dict(
        header="include/sfmwarp.h",
        line="a NaN Euler angle is read as -pi",
        applies=has_nan_angle,
        what="euler2mat clips with fminf(fmaxf(r, -pi), pi): a NaN angle becomes -pi (and its own gradient 0, the clip's backward) "
             "where np.clip keeps it")),
    # the entries below are pinned on the device only (tests/test_hostile_inputs_gpu.py): they are not a clamp of the statements
    ("loss_nan_position_by_layout", dict(
        header="include/sfmwarp.h", scope="gpu",
        line="in the planar layout its warped value is exactly 0; in the pixel-interleaved layout it is NaN",
        what="fused loss: a sample whose position is NaN is not in view; the planar kernels select 0 for it, the pixel-interleaved "
             "ones blend zero taps with NaN fractions")),
    ("loss_non_finite_pose_is_swallowed", dict(
        header="include/sfmwarp.h", scope="gpu",
        line="A non-finite POSE entry is NOT reported by the fused loss",
        what="fused loss: a NaN angle is -pi to every kernel (all outputs finite, its own gradient 0); a NaN or infinite translation "
             "puts every pixel of that source at a NaN position, with the consequences of loss_nan_position_by_layout -- the "
             "reference's loss and d_pose are NaN in both cases")),
    ("reference_order_infinite_disparity", dict(
        header="include/sfmwarp.h", scope="gpu",
        line="an infinite disparity is depth 0 in the default projection and a NaN depth under SFM_PROJECTION_REFERENCE_ORDER",
        what="rcp_refined(inf) = NaN (0 x inf in its residual), v_rcp_f32(inf) = 0")),
    ("smoothness_of_infinite_disparity_is_nan", dict(
        header="include/sfmwarp.h", scope="gpu",
        line="the smoothness terms of a stencil that holds an infinite disparity are NaN",
        what="inf - inf in the kernels' stencils, where the statement's order of differences gives +inf")),
    ("loss_gradients_of_a_hostile_disparity", dict(
        header="include/sfmwarp.h", scope="gpu",
        line="the class of the gradients around a hostile disparity is a property of each formula",
        what="fused loss: the kernels' sign(NaN) is +-1 where np.sign gives NaN (smoothness and L1 backward), -gD / disp^2 is formed "
             "from 1 / disp (0 x inf where the statement divides), and the SSIM window spreads a NaN warped value: d_disp, d_src and "
             "d_mask near such a pixel are held to each other across launches, not to the statement")),
    ("projection_bottom_row_is_exact", dict(
        header="include/sfmwarp.h", scope="gpu",
        line="row 3 of the output is written as (0, 0, 0, 1) whatever the pose",
        what="sfm_pose_proj_fwd: the statement multiplies K4's bottom row with a non-finite translation (0 x NaN = NaN)")),
])


# ---------------------------------------------------------------------------------------------------------------------------
# the pose conventions of include/sfmwarp_pose.h (the _conv_ entry points): axis-angle and inverted poses, the affine depth map,
# "matrix" poses -- tests/warp_exact_ref.py's knife-free cases of those settings at B = 2, one pose entry of sample 0 overwritten
# ---------------------------------------------------------------------------------------------------------------------------
CONV_BASES = {"conv": ((2, 13, 21, 2, 1), R.CONV_CASES[(2, 13, 21, 2, 1)][0], "conv"),
              "axis_angle": R.ALONE_CASES["axis_angle"] + ("axis_angle",), "invert": R.ALONE_CASES["invert"] + ("invert",),
              "matrix": ((1, 24, 40, 3, 3), R.MATRIX_CASES[(1, 24, 40, 3, 3)][0], "matrix")}


@functools.lru_cache(maxsize=None)
def conv_base(name):
    shape, seed, setting = CONV_BASES[name]
    d = R.inputs(shape, seed, setting)
    return d if shape[0] == 2 else stack2(d)


BASES["conv"] = conv_base


def _conv_catalogue():
    out = []
    for base, (shape, _, setting) in CONV_BASES.items():
        n_src = shape[3]
        if setting == "matrix":      # an entry of T: of the rotation block, of the translation column
            for name, v in (("nan", NAN), ("+inf", INF)):
                out.append(Hostile("conv", base, ("poses", 0), (0, 1, 1), v, "T_rot_%s" % name, None))
                out.append(Hostile("conv", base, ("poses", n_src - 1), (0, 2, 3), v, "T_trans_%s" % name, None))
        else:
            values = (("nan", NAN), ("1e30", 1e30)) if setting != "invert" else (("nan", NAN), ("+inf", INF))
            for name, v in values:
                out.append(Hostile("conv", base, ("poses", 0), (0, 1), v, "angle_%s" % name, None))      # source 0: inverted under conv / invert
            out.append(Hostile("conv", base, ("poses", n_src - 1), (0, 5), NAN, "trans_nan", None))
    return out


CONV_CATALOGUE = _conv_catalogue()


def warp_conv_statement(d, c=False):
    """tests/warp_exact_ref.py's reference in float32 under the case's own conventions (pose_conv_ref's matrices and their torch
    gradients) -> dict of lists warped, valid, d_disps, d_poses.  c: the SAMPLER's clip is the kernels' (a NaN position); under
    axis-angle and matrix poses there is no Euler clip, under "invert" (Euler) c also makes a NaN angle -pi in the forward."""
    with np.errstate(all="ignore"), c_clamps(c):
        ref = R.reference(d, F32)
        if c and "nan_euler_angle_is_minus_pi" in (tuple(DEVIATIONS) if c is True else c) and d["fmt"] == "euler":
            # pose_conv_ref's gradient is torch autograd, whose clamp c_clamps cannot reach: the deviation stated on its input -- the
            # NaN angle is -pi, and receives the gradient 0 (the clip's backward)
            import torch
            out = []
            for i, (p, t) in enumerate(zip(d["poses"], ref["d_T"])):
                bad = np.isnan(p)
                bad[:, 3:] = False
                g = np.array(R.PR.pose_matrix_grad(np.where(bad, F32(-np.pi), p).astype(F32), "euler", d["invert"][i], t, torch.float32), F32)
                g[bad] = 0
                out.append(g)
            ref["d_poses"] = out
    return {k: ref[k] for k in ("warped", "valid", "d_disps", "d_poses")}


def deviations_of(h, d=None, grids=None):
    """the names of the DEVIATIONS entries that apply to a catalogue case; grids: the [(grid_x, grid_y)] the statement in question
    hands to its sampler, where that is not the multi-scale statement of the case's group (sfm_warp_*: one source, the depth itself)"""
    d = inputs_of(h) if d is None else d
    return [name for name, e in DEVIATIONS.items() if "applies" in e and e["applies"](h, d, grids)]


def operator_deviations_of(h, a):
    """deviations_of for one sfm_warp_* call on the arrays of operator_arrays: the positions are those of that call"""
    with np.errstate(all="ignore"):
        grid = warp_operator_statement(a)["grid"]
    fake = dict(poses=[a["pose"]])
    return deviations_of(h, fake, [(grid[:, 0].reshape(-1), grid[:, 1].reshape(-1))])
