// The differentiable warp of the whole source pyramid of one step (include/sfmwarp.h): every scale and every source
// warped in ONE launch, differentiated in ONE launch plus a fold of one wavefront per (sample, source).  Per pixel it is the code of
// sfm_warp_fwd / sfm_warp_bwd (sfm_warp_pixel.h: the reference's own evaluation order), so the values are those operators' bit for
// bit.  gfx950 only.
//
// One grid covers every (scale, sample, 256-pixel block): block index -> (s, b, block) through per-scale prefix counts.  A block
// builds the geometry of each of its sources once (one LDS slot per source, built by n_src lanes side by side); a thread reads
// its disparity once and loops over the sources.
#include "sfm_common.h"
#include "sfm_pose.h"
#include "sfm_warp_pixel.h"

namespace sfm {

constexpr int WP_BLOCK = 256;
constexpr int WP_WAVES = WP_BLOCK / 64;

struct WarpPyrArgs {
  const float* src[SFM_MAX_SCALES];
  const float* disp[SFM_MAX_SCALES];
  float* warped[SFM_MAX_SCALES];          // fwd
  float* valid[SFM_MAX_SCALES];           // fwd, entries may be NULL
  const float* g_warped[SFM_MAX_SCALES];  // bwd
  float* d_disp[SFM_MAX_SCALES];          // bwd
  const float* pose[SFM_MAX_SRC];
  float* d_pose[SFM_MAX_SRC];             // bwd (fold)
  const float* K;                         // (B, n_scales, 3, 3)
  float* part;                            // bwd: [block][source][12] block sums of gPm
  int H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];
  int nblk[SFM_MAX_SCALES];               // 256-pixel blocks of one image of scale s
  int begin[SFM_MAX_SCALES + 1];          // prefix sums of B * nblk[s]: the first block of scale s
  int B, n_src, n_scales;
  PoseConvArgs conv;                      // include/sfmwarp_pose.h: read by the _conv_ kernels only
};

// where a block works: scale, sample, block of the image -- uniform over the block
struct WarpPyrBlock {
  int s, b, blk;
};

__device__ __forceinline__ WarpPyrBlock warp_pyr_block(const WarpPyrArgs& A) {
  WarpPyrBlock w;
  const int bid = blockIdx.x;
  w.s = scale_of<0>(bid, A.begin, A.n_scales);
  const int r = bid - A.begin[w.s];
  w.b = r / A.nblk[w.s];
  w.blk = r - w.b * A.nblk[w.s];
  return w;
}

// source i of sample b at a scale of P pixels, in either layout (both hold 3 P floats per image, images in (b, i) order)
template <bool HWC>
__device__ __forceinline__ auto warp_pyr_image(const float* src, const size_t image, const int P) {
  if constexpr (HWC) return HwcImage3{src + image * 3 * (size_t)P};
  else return PlanarImage{src + image * 3 * (size_t)P, (size_t)P};
}

// the geometry of every source of this block's (sample, scale): lane i builds source i.  CONV: under the conventions of
// include/sfmwarp_pose.h -- the format is tested here, once per block, by the lanes that build
template <bool CONV>
__device__ __forceinline__ void warp_pyr_geoms(const WarpPyrArgs& A, const WarpPyrBlock& w, Geom* g) {
  if ((int)threadIdx.x < A.n_src) {
    const float* K = A.K + ((size_t)w.b * A.n_scales + w.s) * 9;
    if constexpr (CONV) make_geom_conv(A.conv, threadIdx.x, A.pose[threadIdx.x], (size_t)w.b, K, g[threadIdx.x]);
    else make_geom(A.pose[threadIdx.x] + (size_t)w.b * 6, K, g[threadIdx.x]);
  }
  __syncthreads();
}

// CONV = false is the kernel as it stood; CONV = true differs in the geometry lanes and in how the disparity becomes a depth
template <bool HWC, bool CONV>
__device__ __forceinline__ void warp_pyr_fwd_body(const WarpPyrArgs& A) {
#pragma clang fp contract(off)
  __shared__ Geom g[SFM_MAX_SRC];
  const WarpPyrBlock w = warp_pyr_block(A);
  warp_pyr_geoms<CONV>(A, w, g);
  const int H = A.H[w.s], W = A.W[w.s], P = H * W;
  const int j = w.blk * WP_BLOCK + threadIdx.x;
  if (j >= P) return;
  const int y = j / W, x = j - y * W;
  float disp = A.disp[w.s][(size_t)w.b * P + j];
  if constexpr (CONV) disp = conv_sd(A.conv, disp);
  const float depth = 1.0f / disp;                                    // models/base_model.py:60
  const float D[3] = {depth, depth, depth};
  float* valid = A.valid[w.s];
  for (int i = 0; i < A.n_src; ++i) {
    const size_t image = (size_t)w.b * A.n_src + i;
    const RefProj r = ref_project(g[i], (float)x, (float)y, D, H, W);
    const PadTap t = pad_taps(r.gx, r.gy, H, W);
    const auto taps = warp_pyr_image<HWC>(A.src[w.s], image, P).fetch(t, H, W);
    float* out = A.warped[w.s] + image * 3 * (size_t)P + j;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float x4[4];
      taps.get(c, x4);
      out[(size_t)c * P] = pad_blend(t, x4);
    }
    if (valid) valid[image * (size_t)P + j] = (r.mx == 1.0f && r.my == 1.0f) ? 1.0f : 0.0f;      // transform.py:129
  }
}

template <bool HWC>
__global__ void __launch_bounds__(WP_BLOCK) warp_pyr_fwd_kernel(const WarpPyrArgs A) {
  warp_pyr_fwd_body<HWC, false>(A);
}
template <bool HWC>
__global__ void __launch_bounds__(WP_BLOCK) warp_pyr_conv_fwd_kernel(const WarpPyrArgs A) {
  warp_pyr_fwd_body<HWC, true>(A);
}

template <bool HWC, bool CONV>
__device__ __forceinline__ void warp_pyr_bwd_body(const WarpPyrArgs& A) {
#pragma clang fp contract(off)
  __shared__ Geom g[SFM_MAX_SRC];
  __shared__ float red[WP_WAVES][SFM_MAX_SRC][12];
  const WarpPyrBlock w = warp_pyr_block(A);
  warp_pyr_geoms<CONV>(A, w, g);
  const int H = A.H[w.s], W = A.W[w.s], P = H * W;
  const int j = w.blk * WP_BLOCK + threadIdx.x;
  const bool have = j < P;                       // no early exit: the lanes of a wave add up their sums below
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float disp = have ? A.disp[w.s][(size_t)w.b * P + j] : 1.0f;
  if constexpr (CONV) disp = have ? conv_sd(A.conv, disp) : 1.0f;      // (sd from here on)
  const float depth = 1.0f / disp;               // models/base_model.py:60
  const float D[3] = {depth, depth, depth};
  float g_depth = 0.f;
  for (int i = 0; i < A.n_src; ++i) {
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    if (have) {
      const size_t image = (size_t)w.b * A.n_src + i;
      const WarpGq q = warp_pixel_gq(g[i], warp_pyr_image<HWC>(A.src[w.s], image, P), D, A.g_warped[w.s] + image * 3 * (size_t)P, nullptr,
                                     3, H, W, j);
      float gd[3];
      warp_pixel_gdepth(g[i], q, gd);
      g_depth = g_depth + ((gd[0] + gd[1]) + gd[2]);      // sfm_warp_bwd's d_depth (depth_rows = 1), the sources in ascending order
      warp_pixel_gpm(q, acc);
    }
    wave_sums_lockstep(acc);                     // (lanes without a pixel contribute zeros)
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < 12; ++k) red[wave][i][k] = acc[k];
    }
  }
  if constexpr (CONV) {
    if (have) A.d_disp[w.s][(size_t)w.b * P + j] = conv_d_disp(A.conv, g_depth, disp);
  } else {
    if (have) A.d_disp[w.s][(size_t)w.b * P + j] = -g_depth / (disp * disp);      // depth = 1 / disp
  }
  __syncthreads();
  if ((int)threadIdx.x < A.n_src * 12) {
    const int i = threadIdx.x / 12, k = threadIdx.x - i * 12;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < WP_WAVES; ++v) s += red[v][i][k];
    A.part[((size_t)blockIdx.x * A.n_src + i) * 12 + k] = s;
  }
}

template <bool HWC>
__global__ void __launch_bounds__(WP_BLOCK) warp_pyr_bwd_kernel(const WarpPyrArgs A) {
  warp_pyr_bwd_body<HWC, false>(A);
}
template <bool HWC>
__global__ void __launch_bounds__(WP_BLOCK) warp_pyr_conv_bwd_kernel(const WarpPyrArgs A) {
  warp_pyr_bwd_body<HWC, true>(A);
}

// one wave per (sample, source): per scale the fixed-order sum of that scale's block partials in fp64, rounded to fp32 and taken
// through that scale's K^T; the scales added in ascending order; then the pose backward (CONV: of the chosen convention)
template <bool CONV>
__device__ __forceinline__ void warp_pyr_fold_body(const WarpPyrArgs& A) {
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
  if (lane == 0) {
    if constexpr (CONV) {
      pose_fold_conv(A.conv, i, A.pose[i], (size_t)b, gT3, A.d_pose[i]);
    } else {
      float d[6];
      pose_backward(A.pose[i] + (size_t)b * 6, gT3, d);
#pragma unroll
      for (int k = 0; k < 6; ++k) A.d_pose[i][(size_t)b * 6 + k] = d[k];
    }
  }
}

__global__ void __launch_bounds__(64) warp_pyr_fold_kernel(const WarpPyrArgs A) { warp_pyr_fold_body<false>(A); }
__global__ void __launch_bounds__(64) warp_pyr_conv_fold_kernel(const WarpPyrArgs A) { warp_pyr_fold_body<true>(A); }

// What both calls check and fill in, in the order the header states.  bwd: the pointers of the backward, else those of the forward.
// conv: the call is one of include/sfmwarp_pose.h and `c` its conventions, checked between the layout and the empty batch;
// sizes_only: its workspace query, which looks at no pointer.
static int warp_pyr_setup(WarpPyrArgs& A, const char* who, const SfmWarpPyramidDesc* d, const bool bwd, const bool conv = false,
                          const SfmPoseConv* c = nullptr, const bool sizes_only = false) {
  SFM_REQUIRE(d, SFM_ERR_NULL, "%s: NULL descriptor", who);
  const auto blocks = [&A](const int s, const int H, const int W) { return (long long)(A.nblk[s] = (H * W + WP_BLOCK - 1) / WP_BLOCK); };
  if (int e = check_pyramid_shape(who, d->B, d->n_src, "n_src", d->n_scales, d->H, d->W, "256-pixel blocks", "", blocks, A.H, A.W, A.begin))
    return e;
  A.B = d->B, A.n_src = d->n_src, A.n_scales = d->n_scales;
  SFM_REQUIRE(d->image_layout == SFM_LAYOUT_PLANAR || d->image_layout == SFM_LAYOUT_HWC, SFM_ERR_CONFIG, "%s: image_layout=%d", who,
              d->image_layout);
  if (conv) {
    if (int e = check_pose_conv(who, c, d->n_src, A.conv)) return e;
  }
  if (sizes_only) return SFM_OK;
  if (d->B == 0) return SFM_OK;   // empty batch: nothing to do, pointers may be NULL
  SFM_REQUIRE(d->intrinsics, SFM_ERR_NULL, "%s: intrinsics is NULL", who);
  A.K = d->intrinsics;
  A.part = nullptr;
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->src[s], SFM_ERR_NULL, "%s: src[%d] is NULL", who, s);
    SFM_REQUIRE(d->disp[s], SFM_ERR_NULL, "%s: disp[%d] is NULL", who, s);
    A.src[s] = d->src[s], A.disp[s] = d->disp[s];
    if (bwd) {
      SFM_REQUIRE(d->g_warped[s], SFM_ERR_NULL, "%s: g_warped[%d] is NULL", who, s);
      SFM_REQUIRE(d->d_disp[s], SFM_ERR_NULL, "%s: d_disp[%d] is NULL", who, s);
    } else {
      SFM_REQUIRE(d->warped[s], SFM_ERR_NULL, "%s: warped[%d] is NULL", who, s);
    }
    A.warped[s] = d->warped[s], A.valid[s] = d->valid[s], A.g_warped[s] = d->g_warped[s], A.d_disp[s] = d->d_disp[s];
  }
  for (int i = 0; i < d->n_src; ++i) {
    SFM_REQUIRE(d->pose[i], SFM_ERR_NULL, "%s: pose[%d] is NULL", who, i);
    if (bwd) SFM_REQUIRE(d->d_pose[i], SFM_ERR_NULL, "%s: d_pose[%d] is NULL", who, i);
    A.pose[i] = d->pose[i], A.d_pose[i] = d->d_pose[i];
  }
  return SFM_OK;
}

static size_t warp_pyr_ws_bytes(const WarpPyrArgs& A) {
  const size_t need = (size_t)A.begin[A.n_scales] * A.n_src * 12 * sizeof(float);
  return need ? (need + 255) / 256 * 256 : 256;
}

// the launches of a checked call; conv: the kernels that read A.conv, else the existing ones
static int warp_pyr_launch_fwd(const char* who, const WarpPyrArgs& A, const bool hwc, const bool conv, void* stream) {
  const dim3 grid(A.begin[A.n_scales]);
  const hipStream_t st = (hipStream_t)stream;
  if (conv) {
    if (hwc) hipLaunchKernelGGL(warp_pyr_conv_fwd_kernel<true>, grid, dim3(WP_BLOCK), 0, st, A);
    else hipLaunchKernelGGL(warp_pyr_conv_fwd_kernel<false>, grid, dim3(WP_BLOCK), 0, st, A);
  } else {
    if (hwc) hipLaunchKernelGGL(warp_pyr_fwd_kernel<true>, grid, dim3(WP_BLOCK), 0, st, A);
    else hipLaunchKernelGGL(warp_pyr_fwd_kernel<false>, grid, dim3(WP_BLOCK), 0, st, A);
  }
  return check_launch(who);
}

static int warp_pyr_launch_bwd(const char* who, WarpPyrArgs& A, const bool hwc, const bool conv, void* ws, size_t ws_bytes, void* stream) {
  const size_t need = warp_pyr_ws_bytes(A);
  SFM_REQUIRE(ws && ws_bytes >= need, SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, need, ws ? ws_bytes : (size_t)0);
  SFM_REQUIRE(((uintptr_t)ws & 255) == 0, SFM_ERR_WORKSPACE, "%s: workspace must be aligned to 256 bytes", who);
  A.part = (float*)ws;
  const dim3 grid(A.begin[A.n_scales]), fold(A.B * A.n_src);
  const hipStream_t st = (hipStream_t)stream;
  if (conv) {
    if (hwc) hipLaunchKernelGGL(warp_pyr_conv_bwd_kernel<true>, grid, dim3(WP_BLOCK), 0, st, A);
    else hipLaunchKernelGGL(warp_pyr_conv_bwd_kernel<false>, grid, dim3(WP_BLOCK), 0, st, A);
    hipLaunchKernelGGL(warp_pyr_conv_fold_kernel, fold, dim3(64), 0, st, A);
  } else {
    if (hwc) hipLaunchKernelGGL(warp_pyr_bwd_kernel<true>, grid, dim3(WP_BLOCK), 0, st, A);
    else hipLaunchKernelGGL(warp_pyr_bwd_kernel<false>, grid, dim3(WP_BLOCK), 0, st, A);
    hipLaunchKernelGGL(warp_pyr_fold_kernel, fold, dim3(64), 0, st, A);
  }
  return check_launch(who);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_warp_pyramid_fwd(const SfmWarpPyramidDesc* d, void* stream) {
  const char* who = "sfm_warp_pyramid_fwd";
  WarpPyrArgs A;
  if (int e = warp_pyr_setup(A, who, d, false)) return e;
  if (d->B == 0) return SFM_OK;
  return warp_pyr_launch_fwd(who, A, d->image_layout == SFM_LAYOUT_HWC, false, stream);
}

size_t sfm_warp_pyramid_bwd_workspace_bytes(const SfmWarpPyramidDesc* d) {
  WarpPyrArgs A;
  if (warp_pyr_setup(A, "sfm_warp_pyramid_bwd_workspace_bytes", d, true)) return 0;
  return warp_pyr_ws_bytes(A);
}

int sfm_warp_pyramid_bwd(const SfmWarpPyramidDesc* d, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "sfm_warp_pyramid_bwd";
  WarpPyrArgs A;
  if (int e = warp_pyr_setup(A, who, d, true)) return e;
  if (d->B == 0) return SFM_OK;
  return warp_pyr_launch_bwd(who, A, d->image_layout == SFM_LAYOUT_HWC, false, ws, ws_bytes, stream);
}

// include/sfmwarp_pose.h.  Conventions that are the defaults launch the existing kernels.
int sfm_warp_pyramid_conv_fwd(const SfmWarpPyramidDesc* d, const SfmPoseConv* c, void* stream) {
  const char* who = "sfm_warp_pyramid_conv_fwd";
  WarpPyrArgs A;
  if (int e = warp_pyr_setup(A, who, d, false, true, c)) return e;
  if (d->B == 0) return SFM_OK;
  return warp_pyr_launch_fwd(who, A, d->image_layout == SFM_LAYOUT_HWC, !pose_conv_is_default(A.conv), stream);
}

size_t sfm_warp_pyramid_conv_bwd_workspace_bytes(const SfmWarpPyramidDesc* d, const SfmPoseConv* c) {
  WarpPyrArgs A;
  if (warp_pyr_setup(A, "sfm_warp_pyramid_conv_bwd_workspace_bytes", d, true, true, c, true)) return 0;
  return warp_pyr_ws_bytes(A);
}

int sfm_warp_pyramid_conv_bwd(const SfmWarpPyramidDesc* d, const SfmPoseConv* c, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "sfm_warp_pyramid_conv_bwd";
  WarpPyrArgs A;
  if (int e = warp_pyr_setup(A, who, d, true, true, c)) return e;
  if (d->B == 0) return SFM_OK;
  return warp_pyr_launch_bwd(who, A, d->image_layout == SFM_LAYOUT_HWC, !pose_conv_is_default(A.conv), ws, ws_bytes, stream);
}

}  // extern "C"
