// The per-pixel code of projective_inverse_warp (models/transform.py:94-133,156-193) in the reference's own evaluation order: the
// projection, the sampler's taps on the zero-padded image, the blend and the backward chain down to dL/dq.  ONE copy for every
// translation unit that warps pixel by pixel: sfm_ops.hip (sfm_warp_fwd / sfm_warp_bwd / sfm_warp_intrinsics_bwd and the sampler
// kernels) and sfm_warp_pyramid.hip (all scales and sources of a step in one launch).  gfx950 only.
//
// Where an image is read, the functions take an ACCESSOR instead of a pointer, so that the same code reads a tap from either layout:
//   PlanarImage  C planes of H*W floats (the reference's NCHW): one 4-byte load per tap and channel
//   HwcImage3    pixel-interleaved, three channels (SFM_LAYOUT_HWC): one 12-byte load per tap
// accessor.fetch(t, H, W) addresses the four taps of `t` (HwcImage3: loads them); fetched.get(c, x) hands out channel c's four values,
// exactly 0 for a tap on the one-pixel zero frame.  Same values from both, hence the same results bit for bit.
#pragma once
#include "sfm_common.h"

namespace sfm {

// gT3 (3x4) = K^T . gPm[0:3, :]   (K4^T . gPm restricted to the rows that reach R and t)
__device__ __forceinline__ void kt_times_gpm(const float* K, const float* gPm3x4, float* gT3, bool accumulate) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = K[0 * 3 + i] * gPm3x4[0 * 4 + j] + K[1 * 3 + i] * gPm3x4[1 * 4 + j] + K[2 * 3 + i] * gPm3x4[2 * 4 + j];
      gT3[i * 4 + j] = accumulate ? gT3[i * 4 + j] + v : v;
    }
}

// the scale a flat index over several scales belongs to: the last s >= FIRST with j >= begin[s]
template <int FIRST, typename Index>
__device__ __forceinline__ int scale_of(const Index j, const Index* begin, const int n_scales) {
  int s = FIRST;
#pragma unroll
  for (int k = FIRST + 1; k < SFM_MAX_SCALES; ++k)
    if (k < n_scales && j >= begin[k]) s = k;
  return s;
}

// ------------------------------------------------------------------------------------------
// F.spatial_transformer_sampler (call site models/transform.py:189): general semantics on the
// zero-padded image, for arbitrary grids
// ------------------------------------------------------------------------------------------
struct PadTap {
  int u0, v0;             // top-left tap in PADDED coordinates, u0 in [0,W], v0 in [0,H]
  float wx0, wx1, wy0, wy1;
  bool ok_u, ok_v;        // coordinate inside the padded image (gradient mask)
};

__device__ __forceinline__ PadTap pad_taps(float gx, float gy, int H, int W) {
#pragma clang fp contract(off)
  PadTap t;
  const float up = (gx + 1.0f) * (float)(W - 1) * 0.5f + 1.0f;
  const float vp = (gy + 1.0f) * (float)(H - 1) * 0.5f + 1.0f;
  const float uc = fminf(fmaxf(up, 0.0f), (float)(W + 1));
  const float vc = fminf(fmaxf(vp, 0.0f), (float)(H + 1));
  t.u0 = min(max((int)floorf(uc), 0), W);
  t.v0 = min(max((int)floorf(vc), 0), H);
  t.wx0 = (float)(t.u0 + 1) - uc;
  t.wx1 = uc - (float)t.u0;
  t.wy0 = (float)(t.v0 + 1) - vc;
  t.wy1 = vc - (float)t.v0;
  t.ok_u = (up >= 0.0f) && (up <= (float)(W + 1));
  t.ok_v = (vp >= 0.0f) && (vp <= (float)(H + 1));
  return t;
}

__device__ __forceinline__ bool pad_inside(int v, int u, int H, int W) { return u >= 1 && u <= W && v >= 1 && v <= H; }   // padded coords

// one channel plane
__device__ __forceinline__ float pad_read(const float* img, int v, int u, int H, int W) {  // padded coords
  return (u >= 1 && u <= W && v >= 1 && v <= H) ? img[(v - 1) * W + (u - 1)] : 0.0f;
}

struct PlanarImage {
  const float* img;   // channel 0 of the image
  size_t P;           // floats between two channel planes
  struct Fetched {
    const float* img;
    size_t P;
    int v0, u0, H, W;
    __device__ __forceinline__ void get(const int c, float (&x)[4]) const {
      const float* pl = img + c * P;
      x[0] = pad_read(pl, v0, u0, H, W), x[1] = pad_read(pl, v0, u0 + 1, H, W);
      x[2] = pad_read(pl, v0 + 1, u0, H, W), x[3] = pad_read(pl, v0 + 1, u0 + 1, H, W);
    }
  };
  __device__ __forceinline__ Fetched fetch(const PadTap& t, const int H, const int W) const { return Fetched{img, P, t.v0, t.u0, H, W}; }
};

struct __attribute__((packed, aligned(4))) Texel3 {   // one pixel-interleaved texel; only 4-byte alignment is guaranteed
  float c[3];
};

struct HwcImage3 {
  const float* img;   // (h, w, 3) of one image: fewer than 2^32 / 12 pixels (byte offsets are 32-bit, ld_off)
  struct Fetched {
    Texel3 t[4];
    __device__ __forceinline__ void get(const int c, float (&x)[4]) const {
      x[0] = t[0].c[c], x[1] = t[1].c[c], x[2] = t[2].c[c], x[3] = t[3].c[c];
    }
  };
  __device__ __forceinline__ Texel3 texel(const int v, const int u, const int H, const int W) const {
    if (pad_inside(v, u, H, W)) return ld_off<Texel3>(img, (unsigned)((v - 1) * W + (u - 1)) * 12u);
    return Texel3{{0.0f, 0.0f, 0.0f}};
  }
  __device__ __forceinline__ Fetched fetch(const PadTap& t, const int H, const int W) const {
    return Fetched{{texel(t.v0, t.u0, H, W), texel(t.v0, t.u0 + 1, H, W), texel(t.v0 + 1, t.u0, H, W), texel(t.v0 + 1, t.u0 + 1, H, W)}};
  }
};

// the sampler's blend of four tap values x = (v0,u0) (v0,u0+1) (v0+1,u0) (v0+1,u0+1): weights' products first, then left to right
__device__ __forceinline__ float pad_blend(const PadTap& t, const float (&x)[4]) {
#pragma clang fp contract(off)
  const float w1 = t.wx0 * t.wy0, w2 = t.wx1 * t.wy0, w3 = t.wx0 * t.wy1, w4 = t.wx1 * t.wy1;
  float v = w1 * x[0];
  v += w2 * x[1];
  v += w3 * x[2];
  v += w4 * x[3];
  return v;
}

// ------------------------------------------------------------------------------------------
// projective_inverse_warp  (models/transform.py:156-193) -- the API-parity operator.
//
// Unlike the fused loss kernels (which pre-multiply the geometry), this operator keeps the REFERENCE'S
// evaluation order, step by step and without fused multiply-adds:
//   ray = K^-1 . (x, y, 1)                         transform.py:105-106   (batch_matmul: left to right over k)
//   c   = D (.) ray ; c4 = (c, 1)                  :107-108
//   q   = Pm . c4 ; z = q2 + 1e-10                 :122-123
//   xn  = (q0 / z) / ((W-1)/2.) - 1 ; yn likewise  :124-125
//   each component not strictly inside (-1, 1) is doubled   :128-131
//   F.spatial_transformer_sampler on the zero-padded image  :189  (pad_taps / pad_read above)
// so that the set of exactly-zero output pixels and the sampling positions are the reference's own.
// ------------------------------------------------------------------------------------------
struct RefProj {
  float ray[3], c[3];   // K^-1 . pix ; D (.) ray
  float z, U, V;        // q2 + 1e-10 ; q0 / z ; q1 / z
  float mx, my;         // 1 inside (-1, 1), else 2     (transform.py:128-130)
  float gx, gy;         // the grid coordinates handed to the sampler (xn * mx, yn * my)
};

__device__ __forceinline__ RefProj ref_project(const Geom& g, const float xf, const float yf, const float* D, const int H, const int W) {
#pragma clang fp contract(off)
  RefProj r;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r.ray[j] = (g.Kinv[j * 3 + 0] * xf + g.Kinv[j * 3 + 1] * yf) + g.Kinv[j * 3 + 2];   // the third coordinate of pix is 1
    r.c[j] = D[j] * r.ray[j];
  }
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = ((g.P[k * 4 + 0] * r.c[0] + g.P[k * 4 + 1] * r.c[1]) + g.P[k * 4 + 2] * r.c[2]) + g.P[k * 4 + 3];
  r.z = q[2] + 1e-10f;
  r.U = q[0] / r.z;
  r.V = q[1] / r.z;
  const float half_w = (float)((double)(W - 1) / 2.0), half_h = (float)((double)(H - 1) / 2.0);
  const float xn = r.U / half_w - 1.0f, yn = r.V / half_h - 1.0f;
  r.mx = (xn > -1.0f && xn < 1.0f) ? 1.0f : 2.0f;     // NaN compares false: doubled, stays NaN
  r.my = (yn > -1.0f && yn < 1.0f) ? 1.0f : 2.0f;
  r.gx = xn * r.mx;
  r.gy = yn * r.my;
  return r;
}

__device__ __forceinline__ void load_depth3(const float* depth, const int n, const int drows, const int P, const int j, float* D) {
  if (drows == 1) {   // one row of the reference's (N,3,H*W) broadcast (base_model.py:82-84)
    D[0] = D[1] = D[2] = depth[(size_t)n * P + j];
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r) D[r] = depth[((size_t)n * 3 + r) * P + j];
  }
}

// per pixel: the reference's backward chain sampler -> x mask -> normalisation -> perspective division, i.e. dL/dq of q = Pm . c4
// (transform.py:122-131,189 backward), and the sampler's scatter into d_src when that is bound.  ONE function for sfm_warp_bwd,
// sfm_warp_intrinsics_bwd and sfm_warp_pyramid_bwd: they differentiate the same dL/dq.
//   img: the C channels of the image this pixel samples ; D: its three depths ; g_warped, d_src: THAT image's C planes of H*W
//   floats (planar in both image layouts; d_src may be NULL) ; j: the pixel
struct WarpGq {
  RefProj r;
  float gq[3];
};

template <typename Image>
__device__ __forceinline__ WarpGq warp_pixel_gq(const Geom& g, const Image& img, const float* D, const float* __restrict__ g_warped,
                                                float* __restrict__ d_src, const int C, const int H, const int W, const int j) {
#pragma clang fp contract(off)
  WarpGq o;
  const int P = H * W;
  const int y = j / W, x = j - y * W;
  o.r = ref_project(g, (float)x, (float)y, D, H, W);
  const RefProj& r = o.r;
  const PadTap t = pad_taps(r.gx, r.gy, H, W);
  const auto taps = img.fetch(t, H, W);
  float gu = 0.f, gv = 0.f;
  for (int c = 0; c < C; ++c) {
    const float gc = g_warped[(size_t)c * P + j];
    float xs[4];
    taps.get(c, xs);
    const float x1 = xs[0], x2 = xs[1], x3 = xs[2], x4 = xs[3];
    gu += gc * (-t.wy0 * x1 + t.wy0 * x2 - t.wy1 * x3 + t.wy1 * x4);
    gv += gc * (-t.wx0 * x1 - t.wx1 * x2 + t.wx0 * x3 + t.wx1 * x4);
    if (d_src) {
      float* dst = d_src + (size_t)c * P;
      const int u = t.u0, v = t.v0;   // padded coordinates: taps on the zero frame receive nothing
      if (u >= 1 && u <= W && v >= 1 && v <= H) atomicAdd(dst + (v - 1) * W + (u - 1), gc * t.wx0 * t.wy0);
      if (u + 1 >= 1 && u + 1 <= W && v >= 1 && v <= H) atomicAdd(dst + (v - 1) * W + u, gc * t.wx1 * t.wy0);
      if (u >= 1 && u <= W && v + 1 >= 1 && v + 1 <= H) atomicAdd(dst + v * W + (u - 1), gc * t.wx0 * t.wy1);
      if (u + 1 >= 1 && u + 1 <= W && v + 1 >= 1 && v + 1 <= H) atomicAdd(dst + v * W + u, gc * t.wx1 * t.wy1);
    }
  }
  // sampler backward to the grid, then p_s_xy *= mask (transform.py:131)
  const float ggx = t.ok_u ? gu * ((float)(W - 1) * 0.5f) : 0.f;
  const float ggy = t.ok_v ? gv * ((float)(H - 1) * 0.5f) : 0.f;
  const float half_w = (float)((double)(W - 1) / 2.0), half_h = (float)((double)(H - 1) / 2.0);
  const float gU = (ggx * r.mx) / half_w, gV = (ggy * r.my) / half_h;
  o.gq[0] = gU / r.z;
  o.gq[1] = gV / r.z;
  o.gq[2] = -(gU * r.U + gV * r.V) / r.z;
  return o;
}

// d_depth of one pixel: g_c = Pm^T . gq ; g_depthes[k] = g_c[k] * ray[k]   (transform.py:107,122 backward)
__device__ __forceinline__ void warp_pixel_gdepth(const Geom& g, const WarpGq& w, float (&gd)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) gd[k] = ((g.P[k] * w.gq[0] + g.P[4 + k] * w.gq[1]) + g.P[8 + k] * w.gq[2]) * w.r.ray[k];
}

// the 12 sums of gPm = gq (x) (c, 1) one pixel contributes (transform.py:122 backward)
__device__ __forceinline__ void warp_pixel_gpm(const WarpGq& w, float* acc) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    acc[k * 4 + 0] = w.gq[k] * w.r.c[0]; acc[k * 4 + 1] = w.gq[k] * w.r.c[1]; acc[k * 4 + 2] = w.gq[k] * w.r.c[2]; acc[k * 4 + 3] = w.gq[k];
  }
}

}  // namespace sfm
