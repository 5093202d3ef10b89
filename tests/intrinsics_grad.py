"""Shared by the tests of the gradient with respect to the camera intrinsics: the ramp inputs, the closed form in NumPy fp64, the
per-entry criterion and the fp64 autograd reference.  Test infrastructure only; NumPy / torch on the host.

Ramp inputs.  On synth.make_inputs textures every small shape has pixels on a knife edge -- a cell boundary of the bilinear
lattice, the kink of |I^ - I|, a kink of the SSIM clip -- and twelve numbers summed over a few hundred pixels move by more than any
honest tolerance when one such pixel changes side.  Affine images have none: bilinear sampling of an affine image has no kink at
lattice lines, I^ - I keeps one sign with a margin of >= 0.3 (sources inside [0.15, 0.95], the target inside [-0.95, -0.15]), and
the align-corners pyramid of a ramp is the same ramp."""
import functools

import numpy as np

import cameras
from oracle import sfm_oracle as O

# (B, H, W, n_src, n_scales): small; odd sizes, three sources (no pair form); three scales; the reference's smallest scale, four sources
SHAPES = [(2, 12, 20, 2, 2), (2, 17, 29, 3, 2), (3, 24, 40, 2, 3), (2, 16, 52, 4, 1)]
# Frames whose tile count per (sample, scale) passes 64, the width of the wave that folds the tiles in proj_bwd_kernel (lane l takes
# tiles l, l + 64, ...).  Tiles per scale from sfm_loss_plan_info (4-row chunks at these batch sizes; tests/test_fold_rounds_cpu.py
# pins them):
#   (2, 264, 60, 2, 2)   66, 33          one strip wide: two lanes go round a second time, and there is a second sample
#   (2, 128, 208, 3, 1)  128             exactly two full trips; three sources (no pair form)
#   (1, 128, 416, 2, 4)  224, 64, 16, 4  the workload's own pyramid; scale 1 is the boundary itself
LARGE_SHAPES = [(2, 264, 60, 2, 2), (2, 128, 208, 3, 1), (1, 128, 416, 2, 4)]
LARGE_TILES = {LARGE_SHAPES[0]: [66, 33], LARGE_SHAPES[1]: [128], LARGE_SHAPES[2]: [224, 64, 16, 4]}
KINDS = (None, "skew", "general")
FAMILIES = {0: "base", 1: "wide", 2: "pair", 3: "ref", 4: "dsrc"}
CONFIGS = {
    "l1": dict(),
    "ssim_smooth": dict(smooth_reg=0.1, ssim_rate=0.15),
    "edge_aware": dict(smooth_reg=0.1, ssim_rate=0.15, smooth_mode="edge_aware"),
    "explain": dict(smooth_reg=0.1, exp_reg=0.2),
}
SEED = 3
# (name, shape, mode, layout, projection, want_d_src, the family the gradient launch must be): every kernel family with 66 tiles at
# scale 0, and the pair and base families on the workload's pyramid (224 tiles at scale 0)
LARGE_FAMILY_CASES = [
    ("pair 66 tiles", LARGE_SHAPES[0], "ssim_smooth", "hwc", "fast", False, "pair"),
    ("base 66 tiles", LARGE_SHAPES[0], "ssim_smooth", "planar", "fast", False, "base"),
    ("wide 66 tiles", LARGE_SHAPES[0], "l1", "planar", "fast", False, "wide"),
    ("ref 66 tiles", LARGE_SHAPES[0], "ssim_smooth", "planar", "reference_order", False, "ref"),
    ("dsrc 66 tiles", LARGE_SHAPES[0], "ssim_smooth", "hwc", "fast", True, "dsrc"),
    ("pair 224 tiles", LARGE_SHAPES[2], "ssim_smooth", "hwc", "fast", False, "pair"),
    ("base 224 tiles", LARGE_SHAPES[2], "ssim_smooth", "planar", "fast", False, "base"),
]


def plan_of(lib, desc, grad, loss):
    """sfm_loss_plan_info of a descriptor whose pointers are bound (any non-NULL value; nothing is launched) for the entry point
    (grad, loss) -> ([tiles of scale s], family name)"""
    import ctypes as C
    n = desc.n_scales
    out = (C.c_int * (1 + 4 * n + 2))()
    rc = lib.sfm_loss_plan_info(C.byref(desc), grad, loss, out, len(out))
    assert rc == 0, rc
    return [out[4 + 4 * s] for s in range(n)], FAMILIES[out[1 + 4 * n]]


def host_plan(shape, mode, layout="planar", projection="fast", want_d_src=False, grad=1, loss=1):
    """plan_of for the descriptor bind() of tests/test_intrinsics_grad_gpu.py builds for the case, on the host alone: fake pointers
    that are never dereferenced (as tools/show_plan.py and tests/golden/make_plan_table.py do)"""
    import importlib
    _lib = importlib.import_module("sfm-learner-chainer_amd._lib")
    ops = importlib.import_module("sfm-learner-chainer_amd.ops")
    B, H, W, n_src, S = shape
    cfg = dict(smooth_reg=0.0, exp_reg=0.0, ssim_rate=0.0, smooth_mode="second_order")
    cfg.update(CONFIGS[mode])
    d = ops.loss_desc(B, B, n_src, [(H >> s, W >> s) for s in range(S)],
                      (cfg["smooth_reg"], cfg["exp_reg"], cfg["ssim_rate"], _lib.smooth_mode_id(cfg["smooth_mode"]), _lib.projection_id(projection)),
                      layout)
    fake = 0x1000
    d.intrinsics = fake
    for s in range(S):
        d.tgt[s] = d.src[s] = d.disp[s] = d.d_disp[s] = fake
        if cfg["exp_reg"] > 0:
            d.mask_logits[s] = d.d_mask[s] = fake
        if want_d_src:
            d.d_src[s] = fake
    for i in range(n_src):
        d.pose[i] = d.d_pose[i] = fake
    return plan_of(_lib.lib, d, grad, loss)


def _ramp(rng, B, G, h_w, lo, hi):
    """per sample, image and channel a, b ~ U(-0.3, 0.3) and c such that c + a u + b v, u, v in [0, 1], lies inside [lo, hi];
    -> a function (h, w) -> (B, 3 G, h, w) float32 with the same a, b, c at every size"""
    a, b = rng.uniform(-0.3, 0.3, (B, 3 * G)), rng.uniform(-0.3, 0.3, (B, 3 * G))
    low, high = np.minimum(a, 0) + np.minimum(b, 0), np.maximum(a, 0) + np.maximum(b, 0)
    c = rng.uniform(lo - low, hi - high)

    def at(h, w):
        u, v = np.arange(w) / (w - 1.0), np.arange(h) / (h - 1.0)
        img = c[:, :, None, None] + a[:, :, None, None] * u[None, None, None, :] + b[:, :, None, None] * v[None, None, :, None]
        return np.ascontiguousarray(img, dtype=np.float32)
    return at


@functools.lru_cache(maxsize=None)
def _ramp_inputs(shape, kind, seed):
    import importlib
    synth = importlib.import_module("sfm-learner-chainer_amd.synth")
    B, H, W, n_src, n_scales = shape
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=seed, with_masks=True, seam="shift")
    d = dict(cameras.with_cameras(d, kind, 1000 + seed))
    rng = np.random.RandomState(7000 + seed)
    src_at, tgt_at = _ramp(rng, B, n_src, (H, W), 0.15, 0.95), _ramp(rng, B, 1, (H, W), -0.95, -0.15)
    d["tgt_pyr"] = [tgt_at(H >> s, W >> s) for s in range(n_scales)]
    d["src_pyr"] = [src_at(H >> s, W >> s) for s in range(n_scales)]
    d["tgt"], d["src"] = d["tgt_pyr"][0], d["src_pyr"][0].reshape(B, n_src, 3, H, W)
    for s in range(n_scales):
        assert d["src_pyr"][s].min() >= 0.15 - 1e-6 and d["src_pyr"][s].max() <= 0.95 + 1e-6
        assert d["tgt_pyr"][s].min() >= -0.95 - 1e-6 and d["tgt_pyr"][s].max() <= -0.15 + 1e-6
    return d


def ramp_inputs(shape, kind=None, seed=SEED):
    """synth.make_inputs(seam="shift", with_masks=True) for the shape, the cameras of `kind` (tests/cameras.py; None: synth's own),
    and ramps for both pyramids.  Computed once per case and shared: never modify the arrays."""
    return _ramp_inputs(tuple(shape), kind, seed)


def synth_inputs(shape, kind=None, seed=SEED):
    """the same case on synth's own textures (for the tests knife pixels cannot affect)"""
    import importlib
    synth = importlib.import_module("sfm-learner-chainer_amd.synth")
    B, H, W, n_src, n_scales = shape
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=seed, with_masks=True, seam="shift")
    return cameras.with_cameras(d, kind, 1000 + seed)


# ---------------------------------------------------------------------------------------------------------------------------
# the closed form, NumPy fp64
# ---------------------------------------------------------------------------------------------------------------------------
def rt(pose):
    """pose (N,6) -> R (N,3,3), t (N,3) in fp64 (models/transform.py:11-59)"""
    pose = np.asarray(pose, np.float64)
    return O.euler2mat(pose[:, :3], np.float64), pose[:, 3:]


def d_k_from_d_proj(K, poses, d_proj):
    """K (B,S,3,3), poses: n arrays (B,6), d_proj (B,S,n,3,4) = dL/dPm ->
    d_K (B,S,3,3) = sum_i gPm_i[:, :3] R_i^T + gPm_i[:, 3] t_i^T - K^-T R_i^T K^T gPm_i[:, :3]      (one depth per pixel)"""
    K, g = np.asarray(K, np.float64), np.asarray(d_proj, np.float64)
    Kit = np.transpose(np.linalg.inv(K), (0, 1, 3, 2))
    out = np.zeros_like(K)
    for i, pose in enumerate(poses):
        R, t = rt(pose)
        Rt = np.transpose(R, (0, 2, 1))[:, None]
        g3 = g[:, :, i, :, :3]
        out += g3 @ Rt + g[:, :, i, :, 3:4] * t[:, None, None, :]
        out -= Kit @ Rt @ np.transpose(K, (0, 1, 3, 2)) @ g3
    return out


def d_k_of_proj(pose, g_proj):
    """the proj_tgt_to_src route alone: pose (N,6), g_proj (N,4,4) -> g_proj[:, :3, :] . [R|t]^T  (N,3,3)"""
    R, t = rt(pose)
    g = np.asarray(g_proj, np.float64)
    return g[:, :3, :3] @ np.transpose(R, (0, 2, 1)) + g[:, :3, 3:4] * t[:, None, :]


def entry_errors(got, ref):
    """got, ref (B,S,3,3) or (N,3,3): per scale s and entry (i, j)  max_b |got - ref| / max_b |ref[b, s, i, j]|  -> (S,3,3).
    Never the array maximum: the bottom row of d_K is 100 x the focal entries and an array-maximum criterion would not see fx."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), (got.shape, ref.shape)
    if got.ndim == 3:
        got, ref = got[:, None], ref[:, None]
    scale = np.abs(ref).max(axis=0)
    assert (scale > 0).all(), "an entry of the reference gradient is zero in every sample"
    return np.abs(got - ref).max(axis=0) / scale


def worst(got, ref):
    return float(entry_errors(got, ref).max())


def proj_entry_errors(got, ref):
    """the same rule for d_proj (B,S,n,3,4): per scale, source and entry  max_b |got - ref| / max_b |ref|  -> (S,n,3,4)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.ndim == 5 and np.isfinite(got).all(), (got.shape, ref.shape)
    scale = np.abs(ref).max(axis=0)
    assert (scale > 0).all(), "an entry of the reference gradient is zero in every sample"
    return np.abs(got - ref).max(axis=0) / scale


# ---------------------------------------------------------------------------------------------------------------------------
# torch autograd references (tests/test_oracle_vs_torch_cpu.py's restatement of the reference, intrinsics as a leaf)
# ---------------------------------------------------------------------------------------------------------------------------
def autograd_loss(d, cfg, dtype="float64", want_gq=False):
    """d_K (B,S,3,3) of torch_loss with `intrinsics` a leaf, evaluated in `dtype`; also d_pose per source.  `want_gq`: also
    dL/dPm (B,S,n,3,4), taken by autograd at the projection matrices (the same loss with proj_tgt_to_src recorded)."""
    import torch
    import test_oracle_vs_torch_cpu as T
    dt = getattr(torch, dtype)
    saved = T.DT
    T.DT = dt
    try:
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dt)
        K = t(d["intrinsics"]).requires_grad_(True)
        poses = [t(a).requires_grad_(True) for a in d["poses"]]
        projs = []
        if want_gq:
            real = T.proj_tgt_to_src

            def recording(vec, Kx):
                p = real(vec, Kx)
                p.retain_grad()
                projs.append(p)
                return p
            T.proj_tgt_to_src = recording
        try:
            out = T.torch_loss([t(a) for a in d["tgt_pyr"]], [t(a) for a in d["src_pyr"]], K, [t(a) for a in d["disps"]], poses,
                               [t(a) for a in d["masks"]], **cfg)
            out[0].backward()
        finally:
            if want_gq:
                T.proj_tgt_to_src = real
    finally:
        T.DT = saved
    res = dict(d_K=K.grad.numpy().astype(np.float64), d_poses=[p.grad.numpy().astype(np.float64) for p in poses])
    if want_gq:
        S, n = len(d["disps"]), len(d["poses"])
        g = np.stack([p.grad.numpy()[:, :3, :] for p in projs], axis=1).astype(np.float64)      # (B, S n, 3, 4), scale-major
        res["d_proj"] = g.reshape(g.shape[0], S, n, 3, 4)
    return res


@functools.lru_cache(maxsize=None)
def reference(shape, kind, mode, seed=SEED):
    """fp64 autograd on the ramp inputs of the case, computed once and shared: d_K, d_poses and d_proj"""
    return autograd_loss(ramp_inputs(shape, kind, seed), CONFIGS[mode], want_gq=True)


def autograd_warp(imgs, depthes, pose, K, g_warped, dtype="float64"):
    """d_K (N,3,3) of projective_inverse_warp for the upstream gradient g_warped; depthes (N,3,H*W)"""
    import torch
    import test_oracle_vs_torch_cpu as T
    dt = getattr(torch, dtype)
    saved = T.DT
    T.DT = dt
    try:
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dt)
        Kt = t(K).requires_grad_(True)
        out = T.projective_inverse_warp(t(imgs), t(depthes), t(pose), Kt)
        (out * t(g_warped)).sum().backward()
    finally:
        T.DT = saved
    return Kt.grad.numpy().astype(np.float64)
