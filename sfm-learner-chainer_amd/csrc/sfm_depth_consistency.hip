// The geometry-consistency term of SC-SfMLearner on this library's warp (include/sfmwarp_depth_consistency.h): per (scale, source,
// target pixel) the depth of the pixel's 3-D point in the source camera against the source's own depth map sampled where the point
// lands.  Forward ONE launch, backward ONE launch plus a fold of one wavefront per (sample, source).  Per pixel it is the code of
// sfm_warp_pyramid_conv_* (sfm_warp_pixel.h, sfm_pose.h): the projection, the taps, the blend, the sampler backward, g_depth and the
// gPm terms are those functions, not copies.  What is new here is the image that is sampled (1 / sd of the source's disparity,
// formed tap by tap), the third component of Pm . c4 kept instead of thrown away, and the quotient's derivative.  gfx950 only.
//
// The grid is sfm_warp_pyramid.hip's: block index -> (scale, sample, 256-pixel block) through per-scale prefix counts; a block
// builds the geometry of each of its sources once; a thread reads its disparity once and loops over the sources.
#include "sfm_common.h"
#include "sfm_pose.h"
#include "sfm_warp_pixel.h"
#include "../../include/sfmwarp_depth_consistency.h"

namespace sfm {

constexpr int DC_BLOCK = 256;
constexpr int DC_WAVES = DC_BLOCK / 64;

struct DepthConsArgs {
  const float* disp[SFM_MAX_SCALES];
  const float* src_disp[SFM_MAX_SCALES];
  float* diff[SFM_MAX_SCALES];              // fwd
  float* valid[SFM_MAX_SCALES];             // fwd, entries may be NULL
  float* computed[SFM_MAX_SCALES];          // fwd, entries may be NULL
  float* projected[SFM_MAX_SCALES];         // fwd, entries may be NULL
  const float* g_diff[SFM_MAX_SCALES];      // bwd
  float* d_disp[SFM_MAX_SCALES];            // bwd
  float* d_src_disp[SFM_MAX_SCALES];        // bwd, entries may be NULL
  const float* pose[SFM_MAX_SRC];
  float* d_pose[SFM_MAX_SRC];               // bwd (fold)
  const float* K;                           // (B, n_scales, 3, 3)
  float* part;                              // bwd: [block][source][12] block sums of gPm
  int H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];
  int nblk[SFM_MAX_SCALES];                 // 256-pixel blocks of one image of scale s
  int begin[SFM_MAX_SCALES + 1];            // prefix sums of B * nblk[s]: the first block of scale s
  int B, n_src, n_scales;
  PoseConvArgs conv;                        // the defaults where the caller passed no conventions
};

struct DepthConsBlock {
  int s, b, blk;
};

__device__ __forceinline__ DepthConsBlock depth_cons_block(const DepthConsArgs& A) {
  DepthConsBlock w;
  const int bid = blockIdx.x;
  w.s = scale_of<0>(bid, A.begin, A.n_scales);
  const int r = bid - A.begin[w.s];
  w.b = r / A.nblk[w.s];
  w.blk = r - w.b * A.nblk[w.s];
  return w;
}

__device__ __forceinline__ void depth_cons_geoms(const DepthConsArgs& A, const DepthConsBlock& w, Geom* g) {
  if ((int)threadIdx.x < A.n_src) {
    const float* K = A.K + ((size_t)w.b * A.n_scales + w.s) * 9;
    make_geom_conv(A.conv, threadIdx.x, A.pose[threadIdx.x], (size_t)w.b, K, g[threadIdx.x]);
  }
  __syncthreads();
}

// One source's disparity plane as the image accessor of sfm_warp_pixel.h: fetch loads the sd of the four taps (a tap on the zero
// frame loads nothing), get hands out the DEPTH 1 / sd of each, exactly 0 on the frame.  One channel: c is not looked at.
struct DepthImage {
  const float* disp;          // (h, w) of one source
  const PoseConvArgs& conv;
  struct Fetched {
    float sd[4];
    bool in[4];
    __device__ __forceinline__ void get(const int, float (&x)[4]) const {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = in[k] ? 1.0f / sd[k] : 0.0f;
    }
  };
  __device__ __forceinline__ Fetched fetch(const PadTap& t, const int H, const int W) const {
    Fetched f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = t.v0 + (k >> 1), u = t.u0 + (k & 1);      // padded coordinates, in pad_blend's order
      f.in[k] = pad_inside(v, u, H, W);
      f.sd[k] = f.in[k] ? conv_sd(conv, disp[(v - 1) * W + (u - 1)]) : 0.0f;
    }
    return f;
  }
};

// the third component of Pm . c4 as ref_project forms it, before its + 1e-10
__device__ __forceinline__ float depth_cons_q2(const Geom& g, const RefProj& r) {
#pragma clang fp contract(off)
  return ((g.P[2 * 4 + 0] * r.c[0] + g.P[2 * 4 + 1] * r.c[1]) + g.P[2 * 4 + 2] * r.c[2]) + g.P[2 * 4 + 3];
}

__global__ void __launch_bounds__(DC_BLOCK) depth_cons_fwd_kernel(const DepthConsArgs A) {
#pragma clang fp contract(off)
  __shared__ Geom g[SFM_MAX_SRC];
  const DepthConsBlock w = depth_cons_block(A);
  depth_cons_geoms(A, w, g);
  const int H = A.H[w.s], W = A.W[w.s], P = H * W;
  const int j = w.blk * DC_BLOCK + threadIdx.x;
  if (j >= P) return;
  const int y = j / W, x = j - y * W;
  const float sd = conv_sd(A.conv, A.disp[w.s][(size_t)w.b * P + j]);
  const float depth = 1.0f / sd;
  const float D[3] = {depth, depth, depth};
  float *valid = A.valid[w.s], *computed = A.computed[w.s], *projected = A.projected[w.s];
  for (int i = 0; i < A.n_src; ++i) {
    const size_t at = ((size_t)w.b * A.n_src + i) * (size_t)P;
    const RefProj r = ref_project(g[i], (float)x, (float)y, D, H, W);
    const PadTap t = pad_taps(r.gx, r.gy, H, W);
    const auto taps = DepthImage{A.src_disp[w.s] + at, A.conv}.fetch(t, H, W);
    float x4[4];
    taps.get(0, x4);
    const float c = fmaxf(depth_cons_q2(g[i], r), 1e-3f);
    const float p = pad_blend(t, x4);
    const bool ok = r.mx == 1.0f && r.my == 1.0f;
    A.diff[w.s][at + j] = ok ? fabsf(c - p) / (c + p) : 0.0f;
    if (valid) valid[at + j] = ok ? 1.0f : 0.0f;
    if (computed) computed[at + j] = c;
    if (projected) projected[at + j] = p;
  }
}

// SCATTER: d_src_disp of at least one scale is bound
template <bool SCATTER>
__global__ void __launch_bounds__(DC_BLOCK) depth_cons_bwd_kernel(const DepthConsArgs A) {
#pragma clang fp contract(off)
  __shared__ Geom g[SFM_MAX_SRC];
  __shared__ float red[DC_WAVES][SFM_MAX_SRC][12];
  const DepthConsBlock w = depth_cons_block(A);
  depth_cons_geoms(A, w, g);
  const int H = A.H[w.s], W = A.W[w.s], P = H * W;
  const int j = w.blk * DC_BLOCK + threadIdx.x;
  const bool have = j < P;                       // no early exit: the lanes of a wave add up their sums below
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float sd = have ? conv_sd(A.conv, A.disp[w.s][(size_t)w.b * P + j]) : 1.0f;
  const float depth = 1.0f / sd;
  const float D[3] = {depth, depth, depth};
  float g_depth = 0.f;
  for (int i = 0; i < A.n_src; ++i) {
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    if (have) {
      const size_t at = ((size_t)w.b * A.n_src + i) * (size_t)P;
      const DepthImage img{A.src_disp[w.s] + at, A.conv};
      // the sampler chain for the upstream value g itself (it is linear in it); the quotient's factor f_p follows below
      WarpGq q = warp_pixel_gq(g[i], img, D, A.g_diff[w.s] + at, nullptr, 1, H, W, j);
      const RefProj& r = q.r;
      const PadTap t = pad_taps(r.gx, r.gy, H, W);
      const auto taps = img.fetch(t, H, W);
      float x4[4];
      taps.get(0, x4);
      const float q2 = depth_cons_q2(g[i], r);
      const float c = fmaxf(q2, 1e-3f);
      const float p = pad_blend(t, x4);
      const bool ok = r.mx == 1.0f && r.my == 1.0f;
      const float gd_up = A.g_diff[w.s][at + j];
      const float den = c + p, dd = den * den, sgn = signf(c - p);
      const float f_c = sgn * ((2.0f * p) / dd), f_p = -(sgn * ((2.0f * c) / dd));
      const float g_c = gd_up * f_c, g_p = gd_up * f_p;
#pragma unroll
      for (int k = 0; k < 3; ++k) q.gq[k] = ok ? f_p * q.gq[k] : 0.0f;      // an invalid pixel contributes exact zeros
      if (ok && q2 > 1e-3f) q.gq[2] = q.gq[2] + g_c;                         // the clamp's derivative
      float gd[3];
      warp_pixel_gdepth(g[i], q, gd);
      g_depth = g_depth + ((gd[0] + gd[1]) + gd[2]);      // the sources in ascending order
      warp_pixel_gpm(q, acc);
      if constexpr (SCATTER) {
        float* dst = A.d_src_disp[w.s];
        if (dst && ok) {
          dst += at;
          const float wk[4] = {t.wx0 * t.wy0, t.wx1 * t.wy0, t.wx0 * t.wy1, t.wx1 * t.wy1};      // pad_blend's products
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int v = t.v0 + (k >> 1), u = t.u0 + (k & 1);
            if (taps.in[k]) atomicAdd(dst + (v - 1) * W + (u - 1), conv_d_disp(A.conv, g_p * wk[k], taps.sd[k]));
          }
        }
      }
    }
    wave_sums_lockstep(acc);                     // (lanes without a pixel contribute zeros)
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < 12; ++k) red[wave][i][k] = acc[k];
    }
  }
  if (have) A.d_disp[w.s][(size_t)w.b * P + j] = conv_d_disp(A.conv, g_depth, sd);
  __syncthreads();
  if ((int)threadIdx.x < A.n_src * 12) {
    const int i = threadIdx.x / 12, k = threadIdx.x - i * 12;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < DC_WAVES; ++v) s += red[v][i][k];
    A.part[((size_t)blockIdx.x * A.n_src + i) * 12 + k] = s;
  }
}

// one wave per (sample, source): warp_pyr_conv_fold_kernel on this unit's arguments
__global__ void __launch_bounds__(64) depth_cons_fold_kernel(const DepthConsArgs A) {
  const int b = blockIdx.x / A.n_src, i = blockIdx.x - b * A.n_src, lane = threadIdx.x;
  float gT3[12];
  for (int s = 0; s < A.n_scales; ++s) {
    const int nblk = A.nblk[s];
    const float* part = A.part + (((size_t)A.begin[s] + (size_t)b * nblk) * A.n_src + i) * 12;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (int blk = lane; blk < nblk; blk += 64)
#pragma unroll
      for (int k = 0; k < 12; ++k) acc[k] += (double)part[(size_t)blk * A.n_src * 12 + k];
    float gPm[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) gPm[k] = (float)wave_sum_d(acc[k]);
    kt_times_gpm(A.K + ((size_t)b * A.n_scales + s) * 9, gPm, gT3, s > 0);
  }
  if (lane == 0) pose_fold_conv(A.conv, i, A.pose[i], (size_t)b, gT3, A.d_pose[i]);
}

// What the three calls check and fill in, in the order the header states.  bwd: the pointers of the backward, else those of the
// forward; sizes_only: the workspace query, which looks at no pointer.
static int depth_cons_setup(DepthConsArgs& A, const char* who, const SfmDepthConsDesc* d, const SfmPoseConv* c, const bool bwd,
                            const bool sizes_only = false) {
  SFM_REQUIRE(d, SFM_ERR_NULL, "%s: NULL descriptor", who);
  const auto blocks = [&A](const int s, const int H, const int W) { return (long long)(A.nblk[s] = (H * W + DC_BLOCK - 1) / DC_BLOCK); };
  if (int e = check_pyramid_shape(who, d->B, d->n_src, "n_src", d->n_scales, d->H, d->W, "256-pixel blocks", "", blocks, A.H, A.W, A.begin))
    return e;
  A.B = d->B, A.n_src = d->n_src, A.n_scales = d->n_scales;
  const SfmPoseConv defaults = {SFM_POSE_EULER, {0}, 1.0f, 0.0f};
  if (int e = check_pose_conv(who, c ? c : &defaults, d->n_src, A.conv)) return e;
  if (sizes_only) return SFM_OK;
  if (d->B == 0) return SFM_OK;   // empty batch: nothing to do, pointers may be NULL
  SFM_REQUIRE(d->intrinsics, SFM_ERR_NULL, "%s: intrinsics is NULL", who);
  A.K = d->intrinsics;
  A.part = nullptr;
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->disp[s], SFM_ERR_NULL, "%s: disp[%d] is NULL", who, s);
    SFM_REQUIRE(d->src_disp[s], SFM_ERR_NULL, "%s: src_disp[%d] is NULL", who, s);
    if (bwd) {
      SFM_REQUIRE(d->g_diff[s], SFM_ERR_NULL, "%s: g_diff[%d] is NULL", who, s);
      SFM_REQUIRE(d->d_disp[s], SFM_ERR_NULL, "%s: d_disp[%d] is NULL", who, s);
    } else {
      SFM_REQUIRE(d->diff[s], SFM_ERR_NULL, "%s: diff[%d] is NULL", who, s);
    }
    A.disp[s] = d->disp[s], A.src_disp[s] = d->src_disp[s];
    A.diff[s] = d->diff[s], A.valid[s] = d->valid[s], A.computed[s] = d->computed[s], A.projected[s] = d->projected[s];
    A.g_diff[s] = d->g_diff[s], A.d_disp[s] = d->d_disp[s], A.d_src_disp[s] = d->d_src_disp[s];
  }
  for (int i = 0; i < d->n_src; ++i) {
    SFM_REQUIRE(d->pose[i], SFM_ERR_NULL, "%s: pose[%d] is NULL", who, i);
    if (bwd) SFM_REQUIRE(d->d_pose[i], SFM_ERR_NULL, "%s: d_pose[%d] is NULL", who, i);
    A.pose[i] = d->pose[i], A.d_pose[i] = d->d_pose[i];
  }
  return SFM_OK;
}

static size_t depth_cons_ws_bytes(const DepthConsArgs& A) {
  const size_t need = (size_t)A.begin[A.n_scales] * A.n_src * 12 * sizeof(float);
  return need ? (need + 255) / 256 * 256 : 256;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_depth_consistency_fwd(const SfmDepthConsDesc* d, const SfmPoseConv* c, void* stream) {
  const char* who = "sfm_depth_consistency_fwd";
  DepthConsArgs A;
  if (int e = depth_cons_setup(A, who, d, c, false)) return e;
  if (d->B == 0) return SFM_OK;
  hipLaunchKernelGGL(depth_cons_fwd_kernel, dim3(A.begin[A.n_scales]), dim3(DC_BLOCK), 0, (hipStream_t)stream, A);
  return check_launch(who);
}

size_t sfm_depth_consistency_bwd_workspace_bytes(const SfmDepthConsDesc* d, const SfmPoseConv* c) {
  DepthConsArgs A;
  if (depth_cons_setup(A, "sfm_depth_consistency_bwd_workspace_bytes", d, c, true, true)) return 0;
  return depth_cons_ws_bytes(A);
}

int sfm_depth_consistency_bwd(const SfmDepthConsDesc* d, const SfmPoseConv* c, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "sfm_depth_consistency_bwd";
  DepthConsArgs A;
  if (int e = depth_cons_setup(A, who, d, c, true)) return e;
  if (d->B == 0) return SFM_OK;
  const size_t need = depth_cons_ws_bytes(A);
  SFM_REQUIRE(ws && ws_bytes >= need, SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, need, ws ? ws_bytes : (size_t)0);
  SFM_REQUIRE(((uintptr_t)ws & 255) == 0, SFM_ERR_WORKSPACE, "%s: workspace must be aligned to 256 bytes", who);
  A.part = (float*)ws;
  const hipStream_t st = (hipStream_t)stream;
  bool scatter = false;
  for (int s = 0; s < A.n_scales; ++s) {
    if (!A.d_src_disp[s]) continue;
    scatter = true;      // the kernel accumulates into it: cleared on the stream first, so that the call stays capturable
    const hipError_t e = hipMemsetAsync(A.d_src_disp[s], 0, (size_t)A.B * A.n_src * A.H[s] * A.W[s] * sizeof(float), st);
    if (e != hipSuccess) return fail((int)e, "%s: memset: %s", who, hipGetErrorString(e));
  }
  const dim3 grid(A.begin[A.n_scales]), fold(A.B * A.n_src);
  if (scatter) hipLaunchKernelGGL(depth_cons_bwd_kernel<true>, grid, dim3(DC_BLOCK), 0, st, A);
  else hipLaunchKernelGGL(depth_cons_bwd_kernel<false>, grid, dim3(DC_BLOCK), 0, st, A);
  hipLaunchKernelGGL(depth_cons_fold_kernel, fold, dim3(64), 0, st, A);
  return check_launch(who);
}

}  // extern "C"
