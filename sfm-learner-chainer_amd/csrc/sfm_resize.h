// F.resize_images, align-corners bilinear (models/base_model.py:70-72), per output element: ONE copy for every translation unit
// that resamples -- sfm_ops.hip (resize forward and backward, the three pyramid kernels, augment) and sfm_warp_full_res.hip (the
// disparity upsampled inside the warp, and its adjoint).  Below them, under names of their own, the half-pixel taps that
// sfm_warp_full_res.hip offers beside them (include/sfmwarp_conventions.h).  gfx950 only.
#pragma once
#include "sfm_common.h"

namespace sfm {

// ------------------------------------------------------------------------------------------
// F.resize_images, align-corners bilinear (models/base_model.py:70-72).  Source coordinate, taps and weights, and the blend are
// these functions for every kernel that resamples (resize, the three pyramid kernels, augment): that their values agree bit for
// bit is a property of the code (one exception: pyramid_hwc_fwd_kernel writes the blend out, see there).  Each carries its own
// contract(off): the pragma is lexical and does not follow the caller.
// ------------------------------------------------------------------------------------------
struct ResizeTap {
  int u0, u1, v0, v1;
  float wu0, wu1, wv0, wv1;
};

// numpy.linspace(0, W-1, oW)[o] = o * step with step = (W-1)/(oW-1), evaluated in double (o: an output index, converted by the call)
__device__ __forceinline__ float resize_coord(const double o, const double step) {
#pragma clang fp contract(off)
  return (float)(o * step);
}

__device__ __forceinline__ int resize_tap0(const float x, const int n) { return min(max((int)floorf(x), 0), max(n - 2, 0)); }

__device__ __forceinline__ ResizeTap resize_taps(const float u, const float v, const int H, const int W) {
#pragma clang fp contract(off)
  ResizeTap t;
  t.u0 = resize_tap0(u, W), t.v0 = resize_tap0(v, H);
  t.u1 = min(t.u0 + 1, W - 1), t.v1 = min(t.v0 + 1, H - 1);
  t.wu1 = u - (float)t.u0, t.wv1 = v - (float)t.v0;
  t.wu0 = 1.0f - t.wu1, t.wv0 = 1.0f - t.wv1;
  return t;
}

// a0 a1 / b0 b1: the values at (v0, u0) (v0, u1) / (v1, u0) (v1, u1), however the caller fetched them
__device__ __forceinline__ float resize_blend(const ResizeTap& t, const float a0, const float a1, const float b0, const float b1) {
#pragma clang fp contract(off)
  const float top = a0 * t.wu0 + a1 * t.wu1;
  const float bot = b0 * t.wu0 + b1 * t.wu1;
  return top * t.wv0 + bot * t.wv1;
}

__device__ __forceinline__ float resize_read(const ResizeTap& t, const float* img, const int W) {
  return resize_blend(t, img[t.v0 * W + t.u0], img[t.v0 * W + t.u1], img[t.v1 * W + t.u0], img[t.v1 * W + t.u1]);
}

// the first o in [0, on] with resize_tap0(resize_coord(o, step), n) >= k (on: there is none)
__device__ __forceinline__ int resize_first_at(const int k, const int n, const int on, const double step, const double inv_step) {
  if (k <= 0) return 0;
  if (k > max(n - 2, 0)) return on;              // tap0 never exceeds n - 2
  int o = (int)fmin(ceil((double)k * inv_step), (double)on);
  while (o > 0 && resize_tap0(resize_coord(o - 1, step), n) >= k) --o;
  while (o < on && resize_tap0(resize_coord(o, step), n) < k) ++o;
  return o;
}

// ------------------------------------------------------------------------------------------
// Half-pixel bilinear, F.interpolate(mode="bilinear", align_corners=False) (include/sfmwarp_conventions.h): the coordinate and the
// taps under names of their own; the blend and the read are resize_blend and resize_read above.  All float32, contraction off.
// ------------------------------------------------------------------------------------------
// max(scale * (o + 0.5) - 0.5, 0) with scale = (float)n / (float)on formed on the host: non-decreasing in o, every step rounds monotonically
__device__ __forceinline__ float resize_hp_coord(const int o, const float scale) {
#pragma clang fp contract(off)
  const float c = scale * ((float)o + 0.5f);
  return fmaxf(c - 0.5f, 0.0f);
}

// (x >= 0 and below n + 1 for every output; the clamp keeps an index in bounds whatever a caller passes)
__device__ __forceinline__ int resize_hp_tap0(const float x, const int n) { return min(max((int)floorf(x), 0), n - 1); }

__device__ __forceinline__ ResizeTap resize_hp_taps(const float u, const float v, const int H, const int W) {
#pragma clang fp contract(off)
  ResizeTap t;
  t.u0 = resize_hp_tap0(u, W), t.v0 = resize_hp_tap0(v, H);
  t.u1 = min(t.u0 + 1, W - 1), t.v1 = min(t.v0 + 1, H - 1);
  t.wu1 = u - (float)t.u0, t.wv1 = v - (float)t.v0;
  t.wu0 = 1.0f - t.wu1, t.wv0 = 1.0f - t.wv1;
  return t;
}

// the first o in [0, on] with resize_hp_tap0(resize_hp_coord(o, scale), n) >= k (on: there is none); inv_scale = (float)on / (float)n
// only places the first guess, (k + 0.5) / scale - 0.5: the two walks settle it on the coordinate the kernels use
__device__ __forceinline__ int resize_hp_first_at(const int k, const int n, const int on, const float scale, const float inv_scale) {
  if (k <= 0) return 0;
  if (k > n - 1) return on;                      // tap0 never exceeds n - 1
  int o = (int)fminf(fmaxf(ceilf(((float)k + 0.5f) * inv_scale - 0.5f), 0.0f), (float)on);
  while (o > 0 && resize_hp_tap0(resize_hp_coord(o - 1, scale), n) >= k) --o;
  while (o < on && resize_hp_tap0(resize_hp_coord(o, scale), n) < k) ++o;
  return o;
}

}  // namespace sfm
