// The pose conventions of include/sfmwarp_pose.h as device code: the ONE builder of T = [R|t] (pose_mat) and its backward
// (pose_mat_backward), shared by the pose operator (sfm_ops.hip), the geometry lanes and the folds of sfm_warp_pyramid.hip and
// sfm_warp_full_res.hip, and -- through make_geom / pose_backward, which are the Euler case without inversion -- by every operator
// kernel of sfm_ops.hip.  P = K . T is geom_from_T (sfm_common.h).  One lane per matrix everywhere: nothing here is per pixel.
#pragma once
#include "sfm_common.h"
#include "../../include/sfmwarp_pose.h"

namespace sfm {

// sin and cos of ANY finite angle: sincos_pi where it is valid, the library's full-range routine elsewhere
__device__ __forceinline__ void sincos_any(const float a, float* sn, float* cs) {
  const float pi = 3.14159265358979323846f;
  if (fabsf(a) <= pi) {
    sincos_pi(a, sn, cs);
  } else {      // (two calls by value: the combined routine returns the cosine through a pointer to private memory)
    *sn = sinf(a);
    *cs = cosf(a);
  }
}

struct AxisRot {  // rot_from_axisangle intermediates, kept for the backward
  float n, d;     // |a|, |a| + 1e-7
  float u[3];     // a / d
  float sa, ca, C;
};

// Monodepth2's rot_from_axisangle (layers.py): R = C u u^T + ca I + sa [u]x with u = a / (|a| + 1e-7), C = 1 - ca.  C is formed
// as sa^2 / (1 + ca) where ca > 0: the same number without the cancellation (at |a| = 1e-2, 1 - ca keeps 11 of its 24 bits).
__device__ __forceinline__ void axis_angle_rot(const float* a, AxisRot& o, float* R) {
#pragma clang fp contract(off)
  o.n = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  o.d = o.n + 1e-7f;
#pragma unroll
  for (int k = 0; k < 3; ++k) o.u[k] = a[k] / o.d;
  sincos_any(o.n, &o.sa, &o.ca);
  o.C = o.ca > 0.f ? (o.sa * o.sa) / (1.0f + o.ca) : 1.0f - o.ca;
  const float x = o.u[0], y = o.u[1], z = o.u[2];
  const float xs = x * o.sa, ys = y * o.sa, zs = z * o.sa;
  const float xC = x * o.C, yC = y * o.C, zC = z * o.C;
  R[0] = x * xC + o.ca, R[1] = y * xC - zs, R[2] = z * xC + ys;
  R[3] = x * yC + zs, R[4] = y * yC + o.ca, R[5] = z * yC - xs;
  R[6] = x * zC - ys, R[7] = y * zC + xs, R[8] = z * zC + o.ca;
}

// the derivative of exactly that formula (the 1e-7 included) for gR = dL/dR (3x3): d|a|/da = a / |a|, and 0 at a = 0 as autograd
// gives it -- there u = 0, C = 0 and sa = 0, so every term is exactly 0
__device__ __forceinline__ void axis_angle_backward(const float* a, const AxisRot& o, const float* gR, float* d_a) {
#pragma clang fp contract(off)
  const float* u = o.u;
  // w: dL/d(sa [u]x) per component of u;  S = gR + gR^T
  const float w[3] = {gR[7] - gR[5], gR[2] - gR[6], gR[3] - gR[1]};
  float Su[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Su[i] = ((gR[i * 3 + 0] + gR[0 * 3 + i]) * u[0] + (gR[i * 3 + 1] + gR[1 * 3 + i]) * u[1]) + (gR[i * 3 + 2] + gR[2 * 3 + i]) * u[2];
  const float g_C = 0.5f * ((Su[0] * u[0] + Su[1] * u[1]) + Su[2] * u[2]);      // u^T gR u
  const float g_ca = (gR[0] + gR[4]) + gR[8];
  const float g_sa = (w[0] * u[0] + w[1] * u[1]) + w[2] * u[2];
  float g_u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) g_u[k] = o.C * Su[k] + o.sa * w[k];
  // dL/d|a|: through the angle (dC = sa, dca = -sa, dsa = ca) and through d = |a| + 1e-7 (du = -u / d)
  const float g_angle = o.sa * (g_C - g_ca) + o.ca * g_sa;
  const float g_d = -(((g_u[0] * u[0] + g_u[1] * u[1]) + g_u[2] * u[2]) / o.d);
  const float g_n = g_angle + g_d;
#pragma unroll
  for (int k = 0; k < 3; ++k) d_a[k] = g_u[k] / o.d + (o.n > 0.f ? g_n * (a[k] / o.n) : 0.f);
}

// T (3x4, row-major) = [R|t] of pose6 in `format` (SFM_POSE_EULER: euler2mat / pose_vec2mat; SFM_POSE_AXIS_ANGLE: above);
// invert: [R^T | -R^T t], Monodepth2's R^T . T(-t)
__device__ __forceinline__ void pose_mat(const int format, const int invert, const float* pose6, float* T) {
#pragma clang fp contract(off)
  float R[9];
  if (format == SFM_POSE_AXIS_ANGLE) {
    AxisRot ar;
    axis_angle_rot(pose6, ar, R);
  } else {
    Rot rot;
    euler2mat(pose6, rot);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rot.R[k];
  }
  const float t[3] = {pose6[3], pose6[4], pose6[5]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (invert) {
#pragma unroll
      for (int j = 0; j < 3; ++j) T[i * 4 + j] = R[j * 3 + i];
      T[i * 4 + 3] = -((R[0 * 3 + i] * t[0] + R[1 * 3 + i] * t[1]) + R[2 * 3 + i] * t[2]);
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) T[i * 4 + j] = R[i * 3 + j];
      T[i * 4 + 3] = t[i];
    }
  }
}

// the backward of pose_mat for gT = dL/dT (3x4, row-major)
__device__ __forceinline__ void pose_mat_backward(const int format, const int invert, const float* pose6, const float* gT, float* d_pose6) {
  Rot rot;
  AxisRot ar;
  float R[9];
  if (format == SFM_POSE_AXIS_ANGLE) {
    axis_angle_rot(pose6, ar, R);
  } else {
    euler2mat(pose6, rot);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rot.R[k];
  }
  float g[12];      // dL/d[R|t] of the transform that is not inverted
  if (invert) {
#pragma clang fp contract(off)
    // T = [R^T | -R^T t]:  gR[j][i] = gT[i][j] - t[j] gT[i][3],  gt[j] = -sum_i R[j][i] gT[i][3]
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int i = 0; i < 3; ++i) g[j * 4 + i] = gT[i * 4 + j] - pose6[3 + j] * gT[i * 4 + 3];
      g[j * 4 + 3] = -((R[j * 3 + 0] * gT[0 * 4 + 3] + R[j * 3 + 1] * gT[1 * 4 + 3]) + R[j * 3 + 2] * gT[2 * 4 + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) g[k] = gT[k];
  }
  if (format == SFM_POSE_AXIS_ANGLE) {
    const float gR[9] = {g[0], g[1], g[2], g[4], g[5], g[6], g[8], g[9], g[10]};
    axis_angle_backward(pose6, ar, gR, d_pose6);
#pragma unroll
    for (int k = 0; k < 3; ++k) d_pose6[3 + k] = g[k * 4 + 3];
  } else {
    pose_backward(pose6, rot, g, d_pose6);
  }
}

// pose_mat_backward for a format and a flag known only at run time (uniform over a launch): one branch per pair, each the code of
// its compile-time pair -- so that the Euler pair is, instruction for instruction, what pose_backward inlines everywhere else
// (each pair stores its own six results: one array shared by the four branches ends up in scratch memory)
template <int FORMAT, int INVERT>
__device__ __forceinline__ void pose_mat_backward_store(const float* pose6, const float* gT, float* out) {
  float d[6];
  pose_mat_backward(FORMAT, INVERT, pose6, gT, d);
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = d[k];
}

__device__ __forceinline__ void pose_mat_backward_rt(const int format, const int invert, const float* pose6, const float* gT, float* out) {
  if (format == SFM_POSE_AXIS_ANGLE) {
    if (invert) pose_mat_backward_store<SFM_POSE_AXIS_ANGLE, 1>(pose6, gT, out);
    else pose_mat_backward_store<SFM_POSE_AXIS_ANGLE, 0>(pose6, gT, out);
  } else {
    if (invert) pose_mat_backward_store<SFM_POSE_EULER, 1>(pose6, gT, out);
    else pose_mat_backward_store<SFM_POSE_EULER, 0>(pose6, gT, out);
  }
}

// proj_tgt_to_src (models/transform.py:64-91) for one sample: the Euler pose, not inverted
__device__ __forceinline__ void make_geom(const float* pose6, const float* K, Geom& g) {
  float T[12];
  pose_mat(SFM_POSE_EULER, 0, pose6, T);
  geom_from_T(T, K, g);
}

__device__ __forceinline__ void pose_backward(const float* pose6, const float* gT3, float* d_pose6) {
  pose_mat_backward(SFM_POSE_EULER, 0, pose6, gT3, d_pose6);
}

// What the warps of include/sfmwarp_pose.h carry beside their arguments: uniform over a launch
struct PoseConvArgs {
  int format;                 // SFM_POSE_*
  int invert[SFM_MAX_SRC];
  int affine;                 // 0: depth = 1 / disp, the existing statement
  float disp_scale, disp_shift;
};

// the geometry of one source under a convention: T as pose_mat builds it, or the caller's 3x4 (SFM_POSE_MATRIX), then P = K . T
__device__ __forceinline__ void make_geom_conv(const PoseConvArgs& c, const int i, const float* pose, const size_t b, const float* K, Geom& g) {
  float T[12];
  if (c.format == SFM_POSE_MATRIX) {
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = pose[b * 12 + k];
  } else {
    pose_mat(c.format, c.invert[i], pose + b * 6, T);
  }
  geom_from_T(T, K, g);
}

// the end of a fold under a convention: gT3 as it is (SFM_POSE_MATRIX) or through pose_mat_backward
__device__ __forceinline__ void pose_fold_conv(const PoseConvArgs& c, const int i, const float* pose, const size_t b, const float* gT3, float* d_pose) {
  if (c.format == SFM_POSE_MATRIX) {
#pragma unroll
    for (int k = 0; k < 12; ++k) d_pose[b * 12 + k] = gT3[k];
  } else {
    pose_mat_backward_rt(c.format, c.invert[i], pose + b * 6, gT3, d_pose + b * 6);
  }
}

// depth and d_disp under the affine map sd = disp_scale * disp + disp_shift (two roundings: callers run with fp contract(off))
__device__ __forceinline__ float conv_sd(const PoseConvArgs& c, const float disp) {
#pragma clang fp contract(off)
  return c.affine ? c.disp_scale * disp + c.disp_shift : disp;
}
__device__ __forceinline__ float conv_d_disp(const PoseConvArgs& c, const float g_depth, const float sd) {
#pragma clang fp contract(off)
  const float d = -g_depth / (sd * sd);
  return c.affine ? d * c.disp_scale : d;
}

// The conventions of a call, checked in the order include/sfmwarp_pose.h states (after image_layout / upsample, before B == 0)
inline int check_pose_conv(const char* who, const SfmPoseConv* c, const int n_src, PoseConvArgs& o) {
  SFM_REQUIRE(c, SFM_ERR_NULL, "%s: NULL conventions", who);
  SFM_REQUIRE(c->pose_format == SFM_POSE_EULER || c->pose_format == SFM_POSE_AXIS_ANGLE || c->pose_format == SFM_POSE_MATRIX, SFM_ERR_CONFIG,
              "%s: pose_format=%d", who, (int)c->pose_format);
  for (int i = 0; i < n_src; ++i)
    SFM_REQUIRE(c->invert[i] == 0 || c->invert[i] == 1, SFM_ERR_CONFIG, "%s: invert[%d]=%d, need 0 or 1", who, i, (int)c->invert[i]);
  for (int i = 0; i < n_src; ++i)
    SFM_REQUIRE(!(c->pose_format == SFM_POSE_MATRIX && c->invert[i]), SFM_ERR_CONFIG,
                "%s: invert[%d] with SFM_POSE_MATRIX: a general 3x4 has no R^T inverse, the caller inverts", who, i);
  SFM_REQUIRE(__builtin_isfinite(c->disp_scale) && __builtin_isfinite(c->disp_shift), SFM_ERR_CONFIG, "%s: disp_scale=%g disp_shift=%g, need finite values",
              who, (double)c->disp_scale, (double)c->disp_shift);
  o.format = c->pose_format;
  for (int i = 0; i < SFM_MAX_SRC; ++i) o.invert[i] = i < n_src ? c->invert[i] : 0;
  o.affine = !(c->disp_scale == 1.0f && c->disp_shift == 0.0f);
  o.disp_scale = c->disp_scale, o.disp_shift = c->disp_shift;
  return SFM_OK;
}

// true where a call with these conventions IS the existing call
inline bool pose_conv_is_default(const PoseConvArgs& c) {
  bool inv = false;
  for (int i = 0; i < SFM_MAX_SRC; ++i) inv = inv || c.invert[i];
  return c.format == SFM_POSE_EULER && !inv && !c.affine;
}

}  // namespace sfm
