"""The pose conventions of include/sfmwarp_pose.h restated in NumPy and torch on the CPU -- a reference, not a test.

  pose_matrix(pose6, fmt, invert, dtype)        (N,6) -> T (N,3,4) in NumPy, float32 or float64.  "euler" delegates to the oracle's
                                                euler2mat / pose_vec2mat; "axis_angle" is Monodepth2's rot_from_axisangle, literally
                                                (C = 1 - cos, the 1e-7 in the normalisation); invert: [R^T | -R^T t].
  pose_matrix_t(pose6, fmt, invert, dtype)      the same as differentiable torch, for the gradients through autograd: float64 is the
                                                reference, float32 the statement a float32 kernel is given its margin over.
  pose_matrix_grad(pose6, fmt, invert, g, dtype)  d_pose6 (N,6) for an upstream g (N,3,4), by autograd of pose_matrix_t.
  rel_err(got, ref)                             per sample: max |got - ref| / max |ref|.
  disp_affine(depth_range)                      (disp_scale, disp_shift) of a (min_depth, max_depth), in Python floats."""
import numpy as np
import torch

from oracle import sfm_oracle as O

F32, F64 = np.float32, np.float64
FORMATS = ("euler", "axis_angle")
EPS = 1e-7      # Monodepth2: axis = vec / (angle + 1e-7)


def axis_angle_rot(a, dtype=F64):
    """rot_from_axisangle (Monodepth2, layers.py): a (N,3) -> R (N,3,3), every operation in `dtype`"""
    a = np.asarray(a, dtype=dtype)
    angle = np.sqrt((a * a).sum(axis=1, dtype=dtype)).astype(dtype)
    axis = a / (angle + dtype(EPS))[:, None]
    ca, sa = np.cos(angle), np.sin(angle)
    C = dtype(1) - ca
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    xs, ys, zs = x * sa, y * sa, z * sa
    xC, yC, zC = x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    R = np.stack([x * xC + ca, xyC - zs, zxC + ys,
                  xyC + zs, y * yC + ca, yzC - xs,
                  zxC - ys, yzC + xs, z * zC + ca], axis=1).reshape(-1, 3, 3)
    assert R.dtype == dtype
    return R


def pose_matrix(pose6, fmt, invert=False, dtype=F64):
    pose6 = np.asarray(pose6, dtype=dtype)
    if fmt == "euler":
        T = O.pose_vec2mat(pose6, dtype)[:, :3]
        R, t = T[:, :, :3], T[:, :, 3]
    else:
        assert fmt == "axis_angle", fmt
        R, t = axis_angle_rot(pose6[:, :3], dtype), pose6[:, 3:]
    if invert:
        Rt = R.transpose(0, 2, 1)
        R, t = Rt, -np.einsum("nij,nj->ni", Rt, t).astype(dtype)
    out = np.concatenate([R, t[:, :, None]], axis=2).astype(dtype)
    assert out.shape == (pose6.shape[0], 3, 4)
    return out


def _euler_t(r):
    """euler2mat (transform.py:11-40) in torch: the angles clipped to [-pi, pi] of the dtype (F.clip: no gradient outside)"""
    pi = float(np.float32(np.pi)) if r.dtype == torch.float32 else float(np.pi)
    rc = torch.clamp(r, -pi, pi)
    c, s = torch.cos(rc), torch.sin(rc)
    zero, one = torch.zeros_like(c[:, 0]), torch.ones_like(c[:, 0])
    Z = torch.stack([c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one], 1).reshape(-1, 3, 3)
    Y = torch.stack([c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]], 1).reshape(-1, 3, 3)
    X = torch.stack([one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]], 1).reshape(-1, 3, 3)
    return (X @ Y) @ Z


def _axis_angle_t(a):
    """rot_from_axisangle as Monodepth2 writes it: torch.norm, axis = vec / (angle + 1e-7)"""
    angle = torch.norm(a, 2, 1, True)
    axis = a / (angle + EPS)
    ca, sa = torch.cos(angle)[:, 0], torch.sin(angle)[:, 0]
    C = 1 - ca
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    xs, ys, zs = x * sa, y * sa, z * sa
    xC, yC, zC = x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    return torch.stack([x * xC + ca, xyC - zs, zxC + ys, xyC + zs, y * yC + ca, yzC - xs, zxC - ys, yzC + xs, z * zC + ca], 1).reshape(-1, 3, 3)


def pose_matrix_t(pose6, fmt, invert=False, dtype=torch.float64):
    """pose6: a torch tensor (N,6) (a leaf, where a gradient is wanted) -> T (N,3,4) in `dtype`"""
    p = pose6.to(dtype)
    R = _euler_t(p[:, :3]) if fmt == "euler" else _axis_angle_t(p[:, :3])
    t = p[:, 3:]
    if invert:
        R = R.transpose(1, 2)
        t = -(R @ t[:, :, None])[:, :, 0]
    return torch.cat([R, t[:, :, None]], 2)


def pose_matrix_grad(pose6, fmt, invert, g_T, dtype=torch.float64):
    """d_pose6 (N,6) as NumPy for the upstream g_T (N,3,4), by autograd of pose_matrix_t in `dtype`"""
    p = torch.from_numpy(np.asarray(pose6)).to(dtype).requires_grad_()
    T = pose_matrix_t(p, fmt, invert, dtype)
    T.backward(torch.from_numpy(np.asarray(g_T)).to(dtype))
    return p.grad.numpy()


def rel_err(got, ref):
    """per sample: the largest absolute distance from `ref`, divided by that sample's largest reference magnitude (1 for a sample
    whose reference is all zeros: the distance itself)"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    n = ref.shape[0]
    scale = np.abs(ref).reshape(n, -1).max(axis=1)
    return np.abs(got - ref).reshape(n, -1).max(axis=1) / np.where(scale > 0, scale, 1.0)


def disp_affine(depth_range):
    """Monodepth2's disp_to_depth: depth = 1 / (min_disp + (max_disp - min_disp) * disp) -> (disp_scale, disp_shift)"""
    lo, hi = float(depth_range[0]), float(depth_range[1])
    return 1.0 / lo - 1.0 / hi, 1.0 / hi


def sample_poses(norms, seed, t_scale=0.1):
    """(len(norms), 6) float32: rotation vectors of the given lengths in random directions (0: exactly zero), translations of order
    t_scale"""
    rng = np.random.RandomState(seed)
    out = np.zeros((len(norms), 6), F64)
    for k, n in enumerate(norms):
        d = rng.standard_normal(3)
        out[k, :3] = d / np.linalg.norm(d) * n
        out[k, 3:] = rng.uniform(-1, 1, 3) * t_scale
    return out.astype(F32)
