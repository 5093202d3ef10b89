// The full-resolution multi-scale warp (include/sfmwarp_full_res.h): ONE full-resolution source set warped with the disparity of
// every scale, each upsampled to the full resolution inside the kernel -- no full-resolution disparity is written by the forward.
// Per pixel it is sfm_warp_pyramid.hip's code (sfm_warp_pixel.h) on a disparity formed by sfm_resize_fwd's code (sfm_resize.h),
// in the same 256-pixel blocks and with the same fold, so the values are those of sfm_resize_fwd -> sfm_warp_pyramid_* at equal
// sizes -> sfm_resize_bwd bit for bit.  gfx950 only.
//
// One grid covers every (scale, sample, 256-pixel block): all scales have the full resolution, so block index = (s * B + b) * nblk
// + block.  A block builds the geometry of each of its sources once -- the same for every scale: one camera --, a thread forms
// its disparity once from the four low-resolution taps and loops over the sources.
//
// HP (include/sfmwarp_conventions.h) is a template parameter of the two pixel kernels and of the gather: the four taps and their
// weights are the half-pixel ones of F.interpolate(align_corners=False) (sfm_resize.h), everything else is the same code; the
// align-corners instantiations keep theirs.
#include "sfm_common.h"
#include "sfm_pose.h"
#include "sfm_resize.h"
#include "sfm_warp_pixel.h"
#include "../../include/sfmwarp_full_res.h"
#include "../../include/sfmwarp_conventions.h"

namespace sfm {

constexpr int WF_BLOCK = 256;     // sfm_warp_pyramid.hip's WP_BLOCK: the block partials of gPm are sums over the same pixels
constexpr int WF_WAVES = WF_BLOCK / 64;

struct WarpFullArgs {
  const float* src;
  const float* disp[SFM_MAX_SCALES];
  float* warped[SFM_MAX_SCALES];          // fwd
  float* valid[SFM_MAX_SCALES];           // fwd, entries may be NULL
  const float* g_warped[SFM_MAX_SCALES];  // bwd
  float* d_disp[SFM_MAX_SCALES];          // bwd
  float* d_up[SFM_MAX_SCALES];            // bwd: (B,1,H,W) in the workspace for a resampled scale, d_disp[s] for a scale of size (H, W)
  const float* pose[SFM_MAX_SRC];
  float* d_pose[SFM_MAX_SRC];             // bwd (fold)
  const float* K;                         // (B, 3, 3)
  float* part;                            // bwd: [block][source][12] block sums of gPm
  // the upsampling's steps as resize_fwd_kernel forms them, (h-1)/(H-1), and their reciprocals (0 for a step of 0) as sfm_resize_bwd
  // forms them: all in double on the host
  double step_u[SFM_MAX_SCALES], step_v[SFM_MAX_SCALES], inv_u[SFM_MAX_SCALES], inv_v[SFM_MAX_SCALES];
  // the half-pixel upsampling's scales, (float)w / (float)W, and the reciprocal ratios (a first guess of the gather only): float32, host
  float hp_u[SFM_MAX_SCALES], hp_v[SFM_MAX_SCALES], hp_inv_u[SFM_MAX_SCALES], hp_inv_v[SFM_MAX_SCALES];
  long long gather[SFM_MAX_SCALES + 1];   // prefix sums of B * h * w over the RESAMPLED scales (the others count 0)
  int h[SFM_MAX_SCALES], w[SFM_MAX_SCALES];
  bool resampled[SFM_MAX_SCALES];
  int H, W, nblk;                         // nblk: 256-pixel blocks of one image
  int B, n_src, n_scales;
  PoseConvArgs conv;                      // include/sfmwarp_pose.h: read by the _conv_ kernels only
};

// where a block works: scale, sample, block of the image -- uniform over the block
struct WarpFullBlock {
  int s, b, blk;
};

__device__ __forceinline__ WarpFullBlock warp_full_block(const WarpFullArgs& A) {
  WarpFullBlock w;
  const int per_scale = A.B * A.nblk;
  w.s = blockIdx.x / per_scale;
  const int r = blockIdx.x - w.s * per_scale;
  w.b = r / A.nblk;
  w.blk = r - w.b * A.nblk;
  return w;
}

template <bool HWC>
__device__ __forceinline__ auto warp_full_image(const float* src, const size_t image, const int P) {
  if constexpr (HWC) return HwcImage3{src + image * 3 * (size_t)P};
  else return PlanarImage{src + image * 3 * (size_t)P, (size_t)P};
}

// the geometry of every source of this block's sample: lane i builds source i.  CONV: under the conventions of
// include/sfmwarp_pose.h -- the format is tested here, once per block, by the lanes that build
template <bool CONV>
__device__ __forceinline__ void warp_full_geoms(const WarpFullArgs& A, const WarpFullBlock& w, Geom* g) {
  if ((int)threadIdx.x < A.n_src) {
    if constexpr (CONV) make_geom_conv(A.conv, threadIdx.x, A.pose[threadIdx.x], (size_t)w.b, A.K + (size_t)w.b * 9, g[threadIdx.x]);
    else make_geom(A.pose[threadIdx.x] + (size_t)w.b * 6, A.K + (size_t)w.b * 9, g[threadIdx.x]);
  }
  __syncthreads();
}

// up[s][b, y, x]: the element itself at equal sizes, else resize_fwd_kernel's value (W, H >= 3: more than one output per axis) or,
// HP, the half-pixel value of include/sfmwarp_conventions.h
template <bool HP>
__device__ __forceinline__ float warp_full_disp(const WarpFullArgs& A, const WarpFullBlock& w, const int y, const int x, const int j) {
#pragma clang fp contract(off)
  const int h = A.h[w.s], ww = A.w[w.s];
  const float* disp = A.disp[w.s] + (size_t)w.b * h * ww;
  if (!A.resampled[w.s]) return disp[j];
  if constexpr (HP) {
    const float u = resize_hp_coord(x, A.hp_u[w.s]);
    const float v = resize_hp_coord(y, A.hp_v[w.s]);
    return resize_read(resize_hp_taps(u, v, h, ww), disp, ww);
  }
  const float u = resize_coord(x, A.step_u[w.s]);
  const float v = resize_coord(y, A.step_v[w.s]);
  return resize_read(resize_taps(u, v, h, ww), disp, ww);
}

// CONV = false is the kernel as it stood; CONV = true differs in the geometry lanes and in how up[s] becomes a depth
template <bool HWC, bool HP, bool CONV>
__device__ __forceinline__ void warp_full_fwd_body(const WarpFullArgs& A) {
#pragma clang fp contract(off)
  __shared__ Geom g[SFM_MAX_SRC];
  const WarpFullBlock w = warp_full_block(A);
  warp_full_geoms<CONV>(A, w, g);
  const int H = A.H, W = A.W, P = H * W;
  const int j = w.blk * WF_BLOCK + threadIdx.x;
  if (j >= P) return;
  const int y = j / W, x = j - y * W;
  float disp = warp_full_disp<HP>(A, w, y, x, j);
  if constexpr (CONV) disp = conv_sd(A.conv, disp);
  const float depth = 1.0f / disp;                                     // models/base_model.py:60
  const float D[3] = {depth, depth, depth};
  float* valid = A.valid[w.s];
  for (int i = 0; i < A.n_src; ++i) {
    const size_t image = (size_t)w.b * A.n_src + i;
    const RefProj r = ref_project(g[i], (float)x, (float)y, D, H, W);
    const PadTap t = pad_taps(r.gx, r.gy, H, W);
    const auto taps = warp_full_image<HWC>(A.src, image, P).fetch(t, H, W);
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

template <bool HWC, bool HP = false>
__global__ void __launch_bounds__(WF_BLOCK) warp_full_fwd_kernel(const WarpFullArgs A) {
  warp_full_fwd_body<HWC, HP, false>(A);
}
template <bool HWC, bool HP = false>
__global__ void __launch_bounds__(WF_BLOCK) warp_full_conv_fwd_kernel(const WarpFullArgs A) {
  warp_full_fwd_body<HWC, HP, true>(A);
}

template <bool HWC, bool HP, bool CONV>
__device__ __forceinline__ void warp_full_bwd_body(const WarpFullArgs& A) {
#pragma clang fp contract(off)
  __shared__ Geom g[SFM_MAX_SRC];
  __shared__ float red[WF_WAVES][SFM_MAX_SRC][12];
  const WarpFullBlock w = warp_full_block(A);
  warp_full_geoms<CONV>(A, w, g);
  const int H = A.H, W = A.W, P = H * W;
  const int j = w.blk * WF_BLOCK + threadIdx.x;
  const bool have = j < P;                       // no early exit: the lanes of a wave add up their sums below
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = j / W, x = j - y * W;
  float disp = have ? warp_full_disp<HP>(A, w, y, x, j) : 1.0f;
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
      const WarpGq q = warp_pixel_gq(g[i], warp_full_image<HWC>(A.src, image, P), D, A.g_warped[w.s] + image * 3 * (size_t)P, nullptr,
                                     3, H, W, j);
      float gd[3];
      warp_pixel_gdepth(g[i], q, gd);
      g_depth = g_depth + ((gd[0] + gd[1]) + gd[2]);      // sfm_warp_pyramid_bwd's sum: the sources in ascending order
      warp_pixel_gpm(q, acc);
    }
    wave_sums_lockstep(acc);                     // (lanes without a pixel contribute zeros)
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < 12; ++k) red[wave][i][k] = acc[k];
    }
  }
  if constexpr (CONV) {
    if (have) A.d_up[w.s][(size_t)w.b * P + j] = conv_d_disp(A.conv, g_depth, disp);      // the factor disp_scale before the gather
  } else {
    if (have) A.d_up[w.s][(size_t)w.b * P + j] = -g_depth / (disp * disp);      // depth = 1 / up
  }
  __syncthreads();
  if ((int)threadIdx.x < A.n_src * 12) {
    const int i = threadIdx.x / 12, k = threadIdx.x - i * 12;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < WF_WAVES; ++v) s += red[v][i][k];
    A.part[((size_t)blockIdx.x * A.n_src + i) * 12 + k] = s;
  }
}

template <bool HWC, bool HP = false>
__global__ void __launch_bounds__(WF_BLOCK) warp_full_bwd_kernel(const WarpFullArgs A) {
  warp_full_bwd_body<HWC, HP, false>(A);
}
template <bool HWC, bool HP = false>
__global__ void __launch_bounds__(WF_BLOCK) warp_full_conv_bwd_kernel(const WarpFullArgs A) {
  warp_full_bwd_body<HWC, HP, true>(A);
}

// d_disp[s] = R_s^T d_up[s] for every resampled scale in one launch: resize_bwd_kernel with one term, one thread per element of
// d_disp[s], which adds the full-resolution values whose taps touch it in ascending (oy, ox).  HP: the same sum over the half-pixel
// taps -- the first outputs that reach a tap found on the float32 coordinate the forward uses, which is non-decreasing in the index
template <bool HP = false>
__global__ void __launch_bounds__(256) warp_full_gather_kernel(const WarpFullArgs A) {
#pragma clang fp contract(off)
  const long long jj = (long long)blockIdx.x * 256 + threadIdx.x;
  if (jj >= A.gather[A.n_scales]) return;
  const int s = scale_of<0>(jj, A.gather, A.n_scales);
  const long long j = jj - A.gather[s];
  const int H = A.h[s], W = A.w[s], oH = A.H, oW = A.W;      // (named as in resize_bwd_kernel: H x W inputs, oH x oW outputs)
  const int HW = H * W;
  const int nc = (int)(j / HW), r = (int)(j - (long long)nc * HW);
  const int iy = r / W, ix = r - iy * W;
  if constexpr (HP) {
    const float* g = A.d_up[s] + (size_t)nc * oH * oW;
    float acc = 0.f;
    const float su = A.hp_u[s], sv = A.hp_v[s];
    const int x0 = resize_hp_first_at(ix - 1, W, oW, su, A.hp_inv_u[s]), x1 = resize_hp_first_at(ix + 1, W, oW, su, A.hp_inv_u[s]);
    const int y0 = resize_hp_first_at(iy - 1, H, oH, sv, A.hp_inv_v[s]), y1 = resize_hp_first_at(iy + 1, H, oH, sv, A.hp_inv_v[s]);
    for (int oy = y0; oy < y1; ++oy) {
      const float v = resize_hp_coord(oy, sv);
      for (int ox = x0; ox < x1; ++ox) {
        const ResizeTap t = resize_hp_taps(resize_hp_coord(ox, su), v, H, W);
        const float wu = (t.u0 == ix ? t.wu0 : 0.f) + (t.u1 == ix ? t.wu1 : 0.f);
        const float wv = (t.v0 == iy ? t.wv0 : 0.f) + (t.v1 == iy ? t.wv1 : 0.f);
        acc = acc + g[oy * oW + ox] * (wv * wu);
      }
    }
    A.d_disp[s][j] = acc;
    return;
  }
  const double su = A.step_u[s], sv = A.step_v[s];
  const int x0 = resize_first_at(ix - 1, W, oW, su, A.inv_u[s]), x1 = resize_first_at(ix + 1, W, oW, su, A.inv_u[s]);
  const int y0 = resize_first_at(iy - 1, H, oH, sv, A.inv_v[s]), y1 = resize_first_at(iy + 1, H, oH, sv, A.inv_v[s]);
  const float* g = A.d_up[s] + (size_t)nc * oH * oW;
  float acc = 0.f;
  for (int oy = y0; oy < y1; ++oy) {
    const float v = resize_coord(oy, sv);
    for (int ox = x0; ox < x1; ++ox) {
      const ResizeTap t = resize_taps(resize_coord(ox, su), v, H, W);
      const float wu = (t.u0 == ix ? t.wu0 : 0.f) + (t.u1 == ix ? t.wu1 : 0.f);
      const float wv = (t.v0 == iy ? t.wv0 : 0.f) + (t.v1 == iy ? t.wv1 : 0.f);
      acc = acc + g[oy * oW + ox] * (wv * wu);      // gy * (wv * wu): the weights' product first
    }
  }
  A.d_disp[s][j] = acc;
}

// one wave per (sample, source): warp_pyr_fold_kernel with one camera for every scale
template <bool CONV>
__device__ __forceinline__ void warp_full_fold_body(const WarpFullArgs& A) {
  const int b = blockIdx.x / A.n_src, i = blockIdx.x - b * A.n_src, lane = threadIdx.x;
  const int nblk = A.nblk;
  float gT3[12];
  for (int s = 0; s < A.n_scales; ++s) {
    const float* part = A.part + ((((size_t)s * A.B + b) * nblk) * A.n_src + i) * 12;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (int blk = lane; blk < nblk; blk += 64)
#pragma unroll
      for (int k = 0; k < 12; ++k) acc[k] += (double)part[(size_t)blk * A.n_src * 12 + k];
    float gPm[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) gPm[k] = (float)wave_sum_d(acc[k]);
    kt_times_gpm(A.K + (size_t)b * 9, gPm, gT3, s > 0);
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

__global__ void __launch_bounds__(64) warp_full_fold_kernel(const WarpFullArgs A) { warp_full_fold_body<false>(A); }
__global__ void __launch_bounds__(64) warp_full_conv_fold_kernel(const WarpFullArgs A) { warp_full_fold_body<true>(A); }

// The sizes and the layout, in the order the header states them: everything the workspace query needs, no pointer looked at.
// conv: the call is one of include/sfmwarp_pose.h and `c` its conventions, checked last.
static int warp_full_shape(WarpFullArgs& A, const char* who, const SfmWarpFullResDesc* d, const int32_t upsample = SFM_UPSAMPLE_ALIGN_CORNERS,
                           const bool conv = false, const SfmPoseConv* c = nullptr) {
  SFM_REQUIRE(d, SFM_ERR_NULL, "%s: NULL descriptor", who);
  SFM_REQUIRE(d->n_src >= 1 && d->n_src <= SFM_MAX_SRC, SFM_ERR_SHAPE, "%s: n_src=%d, need 1..%d", who, d->n_src, SFM_MAX_SRC);
  SFM_REQUIRE(d->n_scales >= 1 && d->n_scales <= SFM_MAX_SCALES, SFM_ERR_SHAPE, "%s: n_scales=%d, need 1..%d", who, d->n_scales,
              SFM_MAX_SCALES);
  SFM_REQUIRE(d->B >= 0, SFM_ERR_SHAPE, "%s: B=%d", who, d->B);
  SFM_REQUIRE(d->H >= 3 && d->W >= 3, SFM_ERR_SHAPE, "%s: H=%d W=%d, need H,W >= 3", who, d->H, d->W);
  for (int s = 0; s < d->n_scales; ++s)
    SFM_REQUIRE(d->h[s] >= 1 && d->w[s] >= 1, SFM_ERR_SHAPE, "%s: scale %d: h=%d w=%d, need h,w >= 1", who, s, d->h[s], d->w[s]);
  SFM_REQUIRE(3ll * d->H * d->W < (1ll << 31), SFM_ERR_SHAPE, "%s: 3*H*W too large", who);
  A.B = d->B, A.n_src = d->n_src, A.n_scales = d->n_scales, A.H = d->H, A.W = d->W;
  A.nblk = (d->H * d->W + WF_BLOCK - 1) / WF_BLOCK;
  A.gather[0] = 0;
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(3ll * d->h[s] * d->w[s] < (1ll << 31), SFM_ERR_SHAPE, "%s: scale %d: 3*h*w too large", who, s);
    const int h = A.h[s] = d->h[s], w = A.w[s] = d->w[s];
    A.resampled[s] = h != d->H || w != d->W;
    A.gather[s + 1] = A.gather[s] + (A.resampled[s] ? (long long)d->B * h * w : 0);
    // numpy.linspace's step, as resize_fwd_kernel forms it, and sfm_resize_bwd's reciprocal
    A.step_u[s] = (double)(w - 1) / (double)(d->W - 1);
    A.step_v[s] = (double)(h - 1) / (double)(d->H - 1);
    A.inv_u[s] = A.step_u[s] > 0.0 ? 1.0 / A.step_u[s] : 0.0;
    A.inv_v[s] = A.step_v[s] > 0.0 ? 1.0 / A.step_v[s] : 0.0;
    A.hp_u[s] = (float)w / (float)d->W, A.hp_v[s] = (float)h / (float)d->H;
    A.hp_inv_u[s] = (float)d->W / (float)w, A.hp_inv_v[s] = (float)d->H / (float)h;
  }
  const long long blocks = (long long)d->n_scales * d->B * A.nblk, gather_blocks = (A.gather[d->n_scales] + 255) / 256;
  SFM_REQUIRE(blocks < (1ll << 31), SFM_ERR_SHAPE, "%s: too many 256-pixel blocks (%lld)", who, blocks);
  SFM_REQUIRE(gather_blocks < (1ll << 31), SFM_ERR_SHAPE, "%s: too many 256-element blocks of d_disp (%lld)", who, gather_blocks);
  SFM_REQUIRE(d->image_layout == SFM_LAYOUT_PLANAR || d->image_layout == SFM_LAYOUT_HWC, SFM_ERR_CONFIG, "%s: image_layout=%d", who,
              d->image_layout);
  SFM_REQUIRE(upsample == SFM_UPSAMPLE_ALIGN_CORNERS || upsample == SFM_UPSAMPLE_HALF_PIXEL, SFM_ERR_CONFIG, "%s: upsample=%d", who,
              (int)upsample);
  if (conv) return check_pose_conv(who, c, d->n_src, A.conv);
  return SFM_OK;
}

// The pointers of a non-empty batch.  bwd: those of the backward, else those of the forward.
static int warp_full_pointers(WarpFullArgs& A, const char* who, const SfmWarpFullResDesc* d, const bool bwd) {
  SFM_REQUIRE(d->intrinsics, SFM_ERR_NULL, "%s: intrinsics is NULL", who);
  SFM_REQUIRE(d->src, SFM_ERR_NULL, "%s: src is NULL", who);
  A.K = d->intrinsics, A.src = d->src, A.part = nullptr;
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->disp[s], SFM_ERR_NULL, "%s: disp[%d] is NULL", who, s);
    if (bwd) {
      SFM_REQUIRE(d->g_warped[s], SFM_ERR_NULL, "%s: g_warped[%d] is NULL", who, s);
      SFM_REQUIRE(d->d_disp[s], SFM_ERR_NULL, "%s: d_disp[%d] is NULL", who, s);
    } else {
      SFM_REQUIRE(d->warped[s], SFM_ERR_NULL, "%s: warped[%d] is NULL", who, s);
    }
    A.disp[s] = d->disp[s], A.warped[s] = d->warped[s], A.valid[s] = d->valid[s], A.g_warped[s] = d->g_warped[s];
    A.d_disp[s] = A.d_up[s] = d->d_disp[s];
  }
  for (int i = 0; i < d->n_src; ++i) {
    SFM_REQUIRE(d->pose[i], SFM_ERR_NULL, "%s: pose[%d] is NULL", who, i);
    if (bwd) SFM_REQUIRE(d->d_pose[i], SFM_ERR_NULL, "%s: d_pose[%d] is NULL", who, i);
    A.pose[i] = d->pose[i], A.d_pose[i] = d->d_pose[i];
  }
  return SFM_OK;
}

static size_t warp_full_part_bytes(const WarpFullArgs& A) { return (size_t)A.n_scales * A.B * A.nblk * A.n_src * 12 * sizeof(float); }

static size_t warp_full_ws_bytes(const WarpFullArgs& A) {
  size_t need = warp_full_part_bytes(A);
  for (int s = 0; s < A.n_scales; ++s)
    if (A.resampled[s]) need += (size_t)A.B * A.H * A.W * sizeof(float);
  return need ? (need + 255) / 256 * 256 : 256;
}

// the three calls, for either upsampling: the existing entry points pass SFM_UPSAMPLE_ALIGN_CORNERS.  conv: a call of
// include/sfmwarp_pose.h; conventions that are the defaults launch the existing kernels
static int warp_full_fwd(const char* who, const SfmWarpFullResDesc* d, const int32_t upsample, void* stream, const bool conv = false,
                         const SfmPoseConv* c = nullptr) {
  WarpFullArgs A;
  if (int e = warp_full_shape(A, who, d, upsample, conv, c)) return e;
  if (d->B == 0) return SFM_OK;   // empty batch: nothing to do, pointers may be NULL
  if (int e = warp_full_pointers(A, who, d, false)) return e;
  const dim3 grid(A.n_scales * A.B * A.nblk);
  const hipStream_t st = (hipStream_t)stream;
  const bool hwc = d->image_layout == SFM_LAYOUT_HWC;
  if (conv && !pose_conv_is_default(A.conv)) {
    if (upsample == SFM_UPSAMPLE_HALF_PIXEL) {
      if (hwc) hipLaunchKernelGGL((warp_full_conv_fwd_kernel<true, true>), grid, dim3(WF_BLOCK), 0, st, A);
      else hipLaunchKernelGGL((warp_full_conv_fwd_kernel<false, true>), grid, dim3(WF_BLOCK), 0, st, A);
    } else {
      if (hwc) hipLaunchKernelGGL((warp_full_conv_fwd_kernel<true, false>), grid, dim3(WF_BLOCK), 0, st, A);
      else hipLaunchKernelGGL((warp_full_conv_fwd_kernel<false, false>), grid, dim3(WF_BLOCK), 0, st, A);
    }
  } else if (upsample == SFM_UPSAMPLE_HALF_PIXEL) {
    if (hwc) hipLaunchKernelGGL((warp_full_fwd_kernel<true, true>), grid, dim3(WF_BLOCK), 0, st, A);
    else hipLaunchKernelGGL((warp_full_fwd_kernel<false, true>), grid, dim3(WF_BLOCK), 0, st, A);
  } else {
    if (hwc) hipLaunchKernelGGL((warp_full_fwd_kernel<true, false>), grid, dim3(WF_BLOCK), 0, st, A);
    else hipLaunchKernelGGL((warp_full_fwd_kernel<false, false>), grid, dim3(WF_BLOCK), 0, st, A);
  }
  return check_launch(who);
}

static int warp_full_bwd(const char* who, const SfmWarpFullResDesc* d, const int32_t upsample, void* ws, size_t ws_bytes, void* stream,
                         const bool conv = false, const SfmPoseConv* c = nullptr) {
  WarpFullArgs A;
  if (int e = warp_full_shape(A, who, d, upsample, conv, c)) return e;
  if (d->B == 0) return SFM_OK;
  if (int e = warp_full_pointers(A, who, d, true)) return e;
  const size_t need = warp_full_ws_bytes(A);
  SFM_REQUIRE(ws && ws_bytes >= need, SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, need, ws ? ws_bytes : (size_t)0);
  SFM_REQUIRE(((uintptr_t)ws & 255) == 0, SFM_ERR_WORKSPACE, "%s: workspace must be aligned to 256 bytes", who);
  A.part = (float*)ws;
  float* up = (float*)((char*)ws + warp_full_part_bytes(A));      // (a multiple of 48 bytes: floats stay aligned)
  for (int s = 0; s < A.n_scales; ++s)
    if (A.resampled[s]) A.d_up[s] = up, up += (size_t)A.B * A.H * A.W;
  const dim3 grid(A.n_scales * A.B * A.nblk);
  const hipStream_t st = (hipStream_t)stream;
  const bool hwc = d->image_layout == SFM_LAYOUT_HWC, hp = upsample == SFM_UPSAMPLE_HALF_PIXEL;
  const bool other = conv && !pose_conv_is_default(A.conv);
  if (other) {
    if (hp) {
      if (hwc) hipLaunchKernelGGL((warp_full_conv_bwd_kernel<true, true>), grid, dim3(WF_BLOCK), 0, st, A);
      else hipLaunchKernelGGL((warp_full_conv_bwd_kernel<false, true>), grid, dim3(WF_BLOCK), 0, st, A);
    } else {
      if (hwc) hipLaunchKernelGGL((warp_full_conv_bwd_kernel<true, false>), grid, dim3(WF_BLOCK), 0, st, A);
      else hipLaunchKernelGGL((warp_full_conv_bwd_kernel<false, false>), grid, dim3(WF_BLOCK), 0, st, A);
    }
  } else if (hp) {
    if (hwc) hipLaunchKernelGGL((warp_full_bwd_kernel<true, true>), grid, dim3(WF_BLOCK), 0, st, A);
    else hipLaunchKernelGGL((warp_full_bwd_kernel<false, true>), grid, dim3(WF_BLOCK), 0, st, A);
  } else {
    if (hwc) hipLaunchKernelGGL((warp_full_bwd_kernel<true, false>), grid, dim3(WF_BLOCK), 0, st, A);
    else hipLaunchKernelGGL((warp_full_bwd_kernel<false, false>), grid, dim3(WF_BLOCK), 0, st, A);
  }
  const long long n_gather = A.gather[A.n_scales];
  if (n_gather > 0) {
    const dim3 gg((unsigned)((n_gather + 255) / 256));
    if (hp) hipLaunchKernelGGL(warp_full_gather_kernel<true>, gg, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(warp_full_gather_kernel<false>, gg, dim3(256), 0, st, A);
  }
  if (other) hipLaunchKernelGGL(warp_full_conv_fold_kernel, dim3(d->B * d->n_src), dim3(64), 0, st, A);
  else hipLaunchKernelGGL(warp_full_fold_kernel, dim3(d->B * d->n_src), dim3(64), 0, st, A);
  return check_launch(who);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_warp_full_res_fwd(const SfmWarpFullResDesc* d, void* stream) {
  return warp_full_fwd("sfm_warp_full_res_fwd", d, SFM_UPSAMPLE_ALIGN_CORNERS, stream);
}

size_t sfm_warp_full_res_bwd_workspace_bytes(const SfmWarpFullResDesc* d) {
  WarpFullArgs A;
  if (warp_full_shape(A, "sfm_warp_full_res_bwd_workspace_bytes", d)) return 0;
  return warp_full_ws_bytes(A);
}

int sfm_warp_full_res_bwd(const SfmWarpFullResDesc* d, void* ws, size_t ws_bytes, void* stream) {
  return warp_full_bwd("sfm_warp_full_res_bwd", d, SFM_UPSAMPLE_ALIGN_CORNERS, ws, ws_bytes, stream);
}

// include/sfmwarp_conventions.h
int sfm_warp_full_res_up_fwd(const SfmWarpFullResDesc* d, int32_t upsample, void* stream) {
  return warp_full_fwd("sfm_warp_full_res_up_fwd", d, upsample, stream);
}

size_t sfm_warp_full_res_up_bwd_workspace_bytes(const SfmWarpFullResDesc* d, int32_t upsample) {
  WarpFullArgs A;
  if (warp_full_shape(A, "sfm_warp_full_res_up_bwd_workspace_bytes", d, upsample)) return 0;
  return warp_full_ws_bytes(A);
}

int sfm_warp_full_res_up_bwd(const SfmWarpFullResDesc* d, int32_t upsample, void* ws, size_t ws_bytes, void* stream) {
  return warp_full_bwd("sfm_warp_full_res_up_bwd", d, upsample, ws, ws_bytes, stream);
}

// include/sfmwarp_pose.h
int sfm_warp_full_res_conv_fwd(const SfmWarpFullResDesc* d, int32_t upsample, const SfmPoseConv* c, void* stream) {
  return warp_full_fwd("sfm_warp_full_res_conv_fwd", d, upsample, stream, true, c);
}

size_t sfm_warp_full_res_conv_bwd_workspace_bytes(const SfmWarpFullResDesc* d, int32_t upsample, const SfmPoseConv* c) {
  WarpFullArgs A;
  if (warp_full_shape(A, "sfm_warp_full_res_conv_bwd_workspace_bytes", d, upsample, true, c)) return 0;
  return warp_full_ws_bytes(A);
}

int sfm_warp_full_res_conv_bwd(const SfmWarpFullResDesc* d, int32_t upsample, const SfmPoseConv* c, void* ws, size_t ws_bytes, void* stream) {
  return warp_full_bwd("sfm_warp_full_res_conv_bwd", d, upsample, ws, ws_bytes, stream, true, c);
}

}  // extern "C"
