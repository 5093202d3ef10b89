// Fused multi-scale view-synthesis loss (forward, backward, forward+backward) for gfx950.
//
// Restates the loop of SFMLearner.__call__, models/base_model.py:69-124 (citations into
// pfnet/sfm-learner-chainer), per (sample b, scale s, source i, pixel):
//   depth = 1/disp (:60) -> projective_inverse_warp (:90-94, models/transform.py:156-193)
//   -> |I^ - I| with the all-channels-zero mask (:95-100,:111) -> SSIM (:112-115,:126-142)
//   -> smoothness of the disparity (:75-77,:169-185 or :144-155) -> explainability (:103-109)
// and the hand-derived backward to disp, pose, mask logits and (optionally) the source image.
//
// Execution model ("wave strip"): one 64-lane wavefront owns a strip of one image at one scale:
// 64 consecutive columns (the outer HL/HR lanes are halo) and `chunk_rows` rows (+ halo rows).
// It walks down its rows keeping the last rows in registers, so that
//   * horizontal neighbours come from DPP wave shifts (no LDS, no barrier),
//   * vertical neighbours come from a register ring,
//   * the 3x3 SSIM pools and their transposes are separable sums over those two,
//   * depth gradients of all sources are summed in a wave-private LDS tile and d_disp is
//     written exactly once, coalesced; the 12 sums of dL/dPm are reduced in-wavefront.
// All scales, sources and samples of a step are covered by ONE launch of loss_kernel (every wave builds the geometry of its
// passes itself: sfm_ssim_pass.h, build_pass_geom), followed by a tiny one: finalize_kernel reduces the per-wave partials in a
// fixed order (bitwise reproducible) and finishes d_pose.
#include <stdlib.h>
#include <string.h>

#include <hip/hip_ext.h>

#include "sfm_loss_kernels.h"

namespace sfm {

// ------------------------------------------------------------------------------------------
// finalize: fixed-order reduction of the per-wave partials
//   blocks [0, B*n_src): d_pose of (b, i)         (only when do_pose)
//   last block        : the five reported scalars (only when loss5 != nullptr)
// ------------------------------------------------------------------------------------------
#ifdef SFM_FIN_STAMPS   // diagnostic build only: 100 MHz time stamps of finalize_kernel's stages into the debug trace buffer (tools/trace_finalize.py)
#define SFM_FSTAMP(slot) do { if (A.trace && threadIdx.x == 0) A.trace[200000 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define SFM_FSTAMP_F(slot) do { if (A.trace && threadIdx.x == 64) A.trace[200000 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)   // first FOLDING wave
#else
#define SFM_FSTAMP(slot) do { } while (0)
#define SFM_FSTAMP_F(slot) do { } while (0)
#endif

constexpr int FINALIZE_WAVES = 16;   // waves of the block that sums the loss partials (the pose blocks use one)

// The first fourteen dwords of the argument block are PRELOADED into scalar registers by the dispatcher (-mllvm
// -amdgpu-kernarg-preload-count=14 in the Makefile; every other kernel of this file takes one by-value struct, which is never preloaded):
// what a pose block needs to form the addresses of its first loads is there when the wave starts, instead of one scalar round trip
// later (tools/anyorder_probe.hip: 0.15 us per kernel on this stack; stamps of this kernel: 0.5 us from its start to "tiles known").
//   q_bsc: B | n_src << 16 | n_scales << 20 | COMPACT << 24 | POSE << 25 | LOSS << 26;  q_t01 .. q_t67: tiles_of[] as 16-bit halves;
//   q_loss_back: bytes from part_loss up to part_gpm (both lie in the caller's workspace: the loss block's pointer without a round trip).
// COMPACT = 0 (a tile count or B beyond 16 bits: planar frames of tens of megapixels): the fields are read from the struct, as before.
// (FIN_* and the HDR_* field positions: sfm_loss_kernels.h, next to make_hdr)
__global__ void __launch_bounds__(64 * FINALIZE_WAVES) finalize_kernel(const float* __restrict__ q_gpm, const float* __restrict__ q_intr,
                                                                       const float* __restrict__ q_pose0, const float* __restrict__ q_pose1,
                                                                       const unsigned q_bsc, const unsigned q_t01, const unsigned q_t23,
                                                                       const unsigned q_t45, const unsigned q_t67, const unsigned q_loss_back,
                                                                       const LossArgs A, float* __restrict__ loss5) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  static_assert(SFM_MAX_SCALES == 8, "four packed words of tile counts");
  const bool compact = (q_bsc & FIN_COMPACT) != 0;
  int hB, h_src, h_scales, h_items, tlh[SFM_MAX_SCALES], ibh[SFM_MAX_SCALES];
  const float *h_gpm, *h_intr, *h_loss;
  if (compact) {          // (uniform)
    hB = (int)(q_bsc & HDR_B_MASK); h_src = (int)((q_bsc >> HDR_SRC_SHIFT) & HDR_NIBBLE); h_scales = (int)((q_bsc >> HDR_SCALES_SHIFT) & HDR_NIBBLE);
    const unsigned tw[4] = {q_t01, q_t23, q_t45, q_t67};
    int run = 0;
#pragma unroll
    for (int k = 0; k < SFM_MAX_SCALES; ++k) {
      tlh[k] = (int)((tw[hdr_tile_word(k)] >> hdr_tile_shift(k)) & HDR_TILE_MASK);
      ibh[k] = run;                              // plan_items: item_begin of a scale = B x the tiles of the scales before it
      run += hB * tlh[k];
    }
    h_items = run;
    h_gpm = q_gpm; h_intr = q_intr;
    h_loss = reinterpret_cast<const float*>(reinterpret_cast<const char*>(q_gpm) - q_loss_back);
  } else {
    hB = A.B; h_src = A.n_src; h_scales = A.n_scales;
#pragma unroll
    for (int k = 0; k < SFM_MAX_SCALES; ++k) { tlh[k] = A.tiles_of[k]; ibh[k] = A.item_begin_of[k]; }
    h_gpm = A.part_gpm; h_intr = A.intrinsics; h_loss = A.part_loss; h_items = A.items;
  }
  const int n_pose_blocks = (q_bsc & FIN_POSE) ? hB * h_src : 0;
  if ((int)blockIdx.x < n_pose_blocks) {
    // d_pose of (b, i): every lane folds its tiles of every scale into K_s^T . gPm (linear), one in-register wave reduction (DPP).
    // A sample with many tiles (308 at cfg2, 376 at cfg5) is spread over the sixteen waves of the block, so that its partials are
    // fetched in ONE round of independent loads instead of up to six dependent rounds (-1 us on those steps); the waves' sums meet
    // in LDS and are added in wave order: a fixed order, the result does not depend on timing.
    const int b = blockIdx.x / h_src, i = blockIdx.x - b * h_src;
    const bool stamp = blockIdx.x == 0;
    if (stamp) SFM_FSTAMP(0);
    __shared__ float pose_red[FINALIZE_WAVES][6];
    // This block is a chain of round trips to memory with little arithmetic between them, so it is written to need ONE: what the
    // addresses of the first loads are formed from arrives preloaded (above), and the pose (helper wave) and the partials (folding
    // waves) go out together; the pose pointer of source i is selected, never loaded through an index.
    int tl[SFM_MAX_SCALES], ib[SFM_MAX_SCALES];
#pragma unroll
    for (int k = 0; k < SFM_MAX_SCALES; ++k) { tl[k] = tlh[k]; ib[k] = ibh[k]; }
    const float* pp = nullptr;
    float* dp = nullptr;
#pragma unroll
    for (int k = 0; k < SFM_MAX_SRC; ++k) {
      float* dk = A.d_pose[k];                 // (needed at the very end: its round trip hides behind everything else)
      asm volatile("" : "+s"(dk));             // (keeps the selection from being folded back into an indexed load)
      dp = (i == k) ? dk : dp;
    }
    if (compact && i < 2) {                    // (uniform) the pose pointers of the first two sources are preloaded
      pp = (i == 0) ? q_pose0 : q_pose1;
    } else {
#pragma unroll
      for (int k = 0; k < SFM_MAX_SRC; ++k) {
        const float* pk = A.pose[k];
        asm volatile("" : "+s"(pk));
        pp = (i == k) ? pk : pp;
      }
    }
    int total = 0;
#pragma unroll
    for (int k = 0; k < SFM_MAX_SCALES; ++k) total += tl[k];
    // The block's waves: the FIRST one is the HELPER -- it builds the Jacobian of the Euler chain, dR/d(theta_k) with the clip mask of
    // transform.py:23 folded in, while the others wait for their partials; the next nfold waves FOLD, one tile per lane (cfg3: 96 tiles,
    // two waves; cfg2 / cfg5: 308 / 376, five / six waves; a sample of more than 960 tiles goes round again), the rest leave at once.
    // Every lane contracts its folded sums with the Jacobian -- d_pose[k] = <dL/dR, dR/d(theta_k)>, d_pose[3 + k] = dL/dt_k are linear
    // in them -- so SIX values go through the wave reduction (not twelve) and nothing is left to do behind it; the folding waves' six sums
    // meet in LDS and are added in wave order: a fixed order, the result does not depend on timing.
    // (Rounds 3-5 had two forms: one wave + helper for samples of up to 128 tiles, sixteen waves, twelve sums each and a 150-instruction
    //  pose_backward by one lane at the very end for the others.)
    const int nfold = min((total + 63) / 64, FINALIZE_WAVES - 1);    // block-uniform, >= 1
    const bool helper = wave == 0;         // (the wave that is launched FIRST: its chain -- pose, sincos, Jacobian -- is the longest)
    const int fw = wave - 1;               // folding wave 0 .. nfold-1
    __shared__ float jac[27];
    if (helper) {
      const float pi = 3.14159265358979323846f;
      float ang[3], sn[3], cs[3], msk[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) ang[k] = pp[b * 6 + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        sincos_pi(fminf(fmaxf(ang[k], -pi), pi), &sn[k], &cs[k]);
        msk[k] = (ang[k] > -pi && ang[k] < pi) ? 1.f : 0.f;        // F.clip backward
      }
      // R = (X Y) Z (transform.py:27-39); its derivatives in CLOSED FORM -- the products with the zeros and ones of X, Y, Z and of their
      // derivatives written out (30 instructions instead of the 160 of six general 3x3 products: the helper is what the folding waves
      // wait for at the barrier):
      //   X Y  = [[cy, 0, sy], [sx sy, cx, -sx cy], [-cx sy, sx, cx cy]]
      //   X'Y  = [[0, 0, 0], [cx sy, -sx, -cx cy], [sx sy, cx, -sx cy]]          X Y' = [[-sy, 0, cy], [sx cy, 0, sx sy], [-cx cy, 0, -cx sy]]
      //   M Z  = [M0 cz + M1 sz, -M0 sz + M1 cz, M2] (columns)                   M Z' = [-M0 sz + M1 cz, -M0 cz - M1 sz, 0]
      const float sx = sn[0], cx = cs[0], sy = sn[1], cy = cs[1], sz = sn[2], cz = cs[2];
      const float sxsy = sx * sy, sxcy = sx * cy, cxsy = cx * sy, cxcy = cx * cy;
      float J[27];
      // dR/d(theta_x) = (X'Y) Z
      J[0] = 0.f; J[1] = 0.f; J[2] = 0.f;
      J[3] = fmaf(cxsy, cz, -(sx * sz)); J[4] = -fmaf(cxsy, sz, sx * cz); J[5] = -cxcy;
      J[6] = fmaf(sxsy, cz, cx * sz);    J[7] = fmaf(-sxsy, sz, cx * cz); J[8] = -sxcy;
      // dR/d(theta_y) = (X Y') Z      (the middle column of X Y' is zero)
      J[9] = -(sy * cz);   J[10] = sy * sz;      J[11] = cy;
      J[12] = sxcy * cz;   J[13] = -(sxcy * sz); J[14] = sxsy;
      J[15] = -(cxcy * cz); J[16] = cxcy * sz;   J[17] = -cxsy;
      // dR/d(theta_z) = (X Y) Z'
      J[18] = -(cy * sz);                  J[19] = -(cy * cz);                    J[20] = 0.f;
      J[21] = fmaf(-sxsy, sz, cx * cz);    J[22] = -fmaf(sxsy, cz, cx * sz);      J[23] = 0.f;
      J[24] = fmaf(cxsy, sz, sx * cz);     J[25] = fmaf(cxsy, cz, -(sx * sz));    J[26] = 0.f;
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 27; ++k) jac[k] = J[k] * msk[k / 9];
      }
      __syncthreads();
      return;
    }
    if (fw >= nfold) return;
    if (stamp) SFM_FSTAMP_F(1);
    float gT3[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) gT3[k] = 0.f;
    // (macros, not lambdas: arrays captured by reference are not split into registers, the compiler parks them in LDS and fetches
    //  the workgroup size for that from the dispatch packet -- in host memory, 10 us away)
#define SFM_FIN_FETCH(idx_, v0_, v1_, v2_, K_)                                                                                    \
  {                                                                                                                               \
    int s_ = 0, off_ = 0;                                                                                                         \
    _Pragma("unroll") for (int k = 0; k < SFM_MAX_SCALES - 1; ++k)                                                                \
        if ((idx_) >= off_ + tl[k] && s_ == k) { off_ += tl[k]; s_ = k + 1; }                                                     \
    int ibs_ = ib[0], tls_ = tl[0];                                                                                               \
    _Pragma("unroll") for (int k = 1; k < SFM_MAX_SCALES; ++k) { ibs_ = (s_ == k) ? ib[k] : ibs_; tls_ = (s_ == k) ? tl[k] : tls_; } \
    const float4* p_ = reinterpret_cast<const float4*>(h_gpm + ((size_t)(ibs_ + b * tls_ + ((idx_) - off_)) * h_src + i) * 12);  \
    v0_ = p_[0]; v1_ = p_[1]; v2_ = p_[2];                                                                                        \
    const float* Kp_ = h_intr + ((size_t)b * h_scales + s_) * 9;                                                                  \
    _Pragma("unroll") for (int k = 0; k < 9; ++k) K_[k] = Kp_[k];                                                                 \
  }
    // the tile's raw pose sums S_k = (sum x A_k, B_k, A_k, C_k) (pose_sums_raw) -> dL/dPm[k][j] = Kinv[j] . S_k[0:3], [k][3] = S_k[3];
    // then gT3 += K^T . gPm   (K4^T . gPm of the rows that reach R and t)
#define SFM_FIN_FOLD(v0_, v1_, v2_, K_)                                                                                           \
  {                                                                                                                               \
    const float s_[12] = {v0_.x, v0_.y, v0_.z, v0_.w, v1_.x, v1_.y, v1_.z, v1_.w, v2_.x, v2_.y, v2_.z, v2_.w};                    \
    float Ki_[9], g_[12];                                                                                                         \
    inv3_fast(K_, Ki_);                                                                                                           \
    _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                                               \
      _Pragma("unroll") for (int j = 0; j < 3; ++j)                                                                               \
          g_[k * 4 + j] = fmaf(Ki_[j * 3 + 2], s_[k * 4 + 2], fmaf(Ki_[j * 3 + 1], s_[k * 4 + 1], Ki_[j * 3 + 0] * s_[k * 4 + 0])); \
      g_[k * 4 + 3] = s_[k * 4 + 3];                                                                                              \
    }                                                                                                                             \
    _Pragma("unroll") for (int r = 0; r < 3; ++r)                                                                                 \
        _Pragma("unroll") for (int c = 0; c < 4; ++c)                                                                             \
            gT3[r * 4 + c] += K_[0 * 3 + r] * g_[0 * 4 + c] + K_[1 * 3 + r] * g_[1 * 4 + c] + K_[2 * 3 + r] * g_[2 * 4 + c];      \
  }
    const int stride = 64 * nfold;
    const int idx0 = fw * 64 + lane;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0;
    float Ka[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (idx0 < total) SFM_FIN_FETCH(idx0, a0, a1, a2, Ka)
    if (stamp) SFM_FSTAMP_F(2);
    if (idx0 < total) SFM_FIN_FOLD(a0, a1, a2, Ka)
    for (int idx = idx0 + stride; idx < total; idx += stride) {   // (samples of more than 960 tiles)
      SFM_FIN_FETCH(idx, a0, a1, a2, Ka)
      SFM_FIN_FOLD(a0, a1, a2, Ka)
    }
#undef SFM_FIN_FETCH
#undef SFM_FIN_FOLD
    __syncthreads();                       // the helper's Jacobian (the helper and the folding waves)
    float d[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) a = fmaf(gT3[r * 4 + c], jac[k * 9 + r * 3 + c], a);
      d[k] = a;
      d[3 + k] = gT3[k * 4 + 3];
    }
#ifdef SFM_FIN_STAMPS
    if (stamp && d[0] != 77.f) SFM_FSTAMP_F(3);
#endif
    wave_sums_lockstep(d);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = lane63(d[k]);
#ifdef SFM_FIN_STAMPS
    if (stamp && d[0] != 77.f) SFM_FSTAMP_F(4);
#endif
    if (nfold > 1) {                       // (block-uniform)
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) pose_red[fw][k] = d[k];
      }
      __syncthreads();
      if (fw != 0) return;
      if (lane < 6) {                      // lane k adds the folding waves' sums of component k in wave order and stores it
        float a = pose_red[0][lane];
        for (int wv = 1; wv < nfold; ++wv) a += pose_red[wv][lane];
        dp[b * 6 + lane] = a;
      }
    } else if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) dp[b * 6 + k] = d[k];
    }
#ifdef SFM_FIN_STAMPS
    if (stamp && d[0] != 77.f) SFM_FSTAMP_F(5);
#endif
    return;
  }
  if (!(q_bsc & FIN_LOSS)) return;
  // the five reported scalars.  Every lane sums its items in fp64 (sixteen waves: one round of independent loads at cfg3); the 1024
  // lane sums of each scalar meet in LDS, and FOUR waves -- one per scalar, so one per SIMD -- add their scalar's sixteen wave
  // columns lane by lane in wave order and reduce the 64 lane sums in registers ((hi, lo) float pair, DPP): a fixed order, the
  // result does not depend on timing.  (Until round 5 each of the sixteen waves ran a DPP reduction of all four scalars: 150
  // instructions x four waves per SIMD = 0.9 us between the arrival of the partials and the barrier; now 0.4.)
  SFM_FSTAMP(8);
  __shared__ double lane_acc[4][FINALIZE_WAVES][64];
  __shared__ double scalar_red[4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const float4* pl = reinterpret_cast<const float4*>(h_loss);
#pragma unroll 4
  for (int t = threadIdx.x; t < h_items; t += 64 * FINALIZE_WAVES) {
    const float4 v = pl[t];
    acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
  }
#ifdef SFM_FIN_STAMPS
  if (acc[0] != 77.0) SFM_FSTAMP(9);
#endif
#pragma unroll
  for (int k = 0; k < 4; ++k) lane_acc[k][wave][lane] = acc[k];
  __syncthreads();
  SFM_FSTAMP(10);
  if (wave >= 4) return;
  {
    static_assert(FINALIZE_WAVES % 4 == 0, "four chains of wave columns");
    double m4[4] = {0.0, 0.0, 0.0, 0.0};   // (four chains side by side instead of sixteen additions in a row; combined in a fixed order)
#pragma unroll
    for (int wv = 0; wv < FINALIZE_WAVES; ++wv) m4[wv & 3] += lane_acc[wave][wv][lane];
    const double m = (m4[0] + m4[1]) + (m4[2] + m4[3]);
    float hl[2];
    hl[0] = (float)m;
    hl[1] = (float)(m - (double)hl[0]);
    wave_sums_lockstep(hl);
    const double r = (double)lane63(hl[0]) + (double)lane63(hl[1]);
    if (lane == 0) scalar_red[wave] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double pixel = scalar_red[0], ssim = scalar_red[1], smooth = scalar_red[2], expl = scalar_red[3];
    const double a = (double)A.alpha;
    loss5[0] = (float)((1.0 - a) * pixel + a * ssim + smooth + expl);   // base_model.py:117-118
    loss5[1] = (float)pixel;
    loss5[2] = (float)smooth;
    loss5[3] = (float)expl;
    loss5[4] = (float)ssim;
    SFM_FSTAMP(11);
  }
}

// ------------------------------------------------------------------------------------------
// sfm_loss_proj_bwd: dL/dPm and dL/d(intrinsics) from the raw pose sums a gradient launch has left in part_gpm
//   block = (sample b, scale s), wave i = source i: every lane adds its tiles t = lane, lane + 64, ... in ascending order in fp64,
//   the 64 lane sums meet in an xor butterfly (a fixed order), lane 0 forms K^-1 and the products in fp64:
//     gPm[:, 0:3] = S . K^-T , gPm[:, 3] = s3           (pose_sums_raw; what finalize_kernel forms per tile in fp32)
//     dK_i = gPm[:, 0:3] . R^T + gPm[:, 3] . t^T - K^-T . R^T . K^T . gPm[:, 0:3]      (transform.py:86-88 and, via F.batch_inv, :105)
//   and the sources' dK_i are added in source order.  Reads the workspace, writes only its two outputs.
// ------------------------------------------------------------------------------------------
struct ProjBwdArgs {
  const float* part_gpm;
  const float* intrinsics;
  const float* pose[SFM_MAX_SRC];
  float* d_proj;   // (B, n_scales, n_src, 3, 4) or nullptr
  float* d_intr;   // (B, n_scales, 3, 3) or nullptr
  int B, n_src, n_scales;
  int tiles_of[SFM_MAX_SCALES], item_begin_of[SFM_MAX_SCALES];
};

__global__ void __launch_bounds__(64 * SFM_MAX_SRC) proj_bwd_kernel(const ProjBwdArgs A) {
  __shared__ double dk_of[SFM_MAX_SRC][9];
  const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;      // blockDim.x = 64 * n_src
  const int b = blockIdx.x / A.n_scales, s = blockIdx.x - b * A.n_scales;
  const int tiles = A.tiles_of[s];
  const size_t first = (size_t)A.item_begin_of[s] + (size_t)b * tiles;
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  for (int t = lane; t < tiles; t += 64) {
    const float4* p = reinterpret_cast<const float4*>(A.part_gpm + ((first + t) * A.n_src + i) * 12);
    const float4 v0 = p[0], v1 = p[1], v2 = p[2];
    acc[0] += (double)v0.x; acc[1] += (double)v0.y; acc[2] += (double)v0.z; acc[3] += (double)v0.w;
    acc[4] += (double)v1.x; acc[5] += (double)v1.y; acc[6] += (double)v1.z; acc[7] += (double)v1.w;
    acc[8] += (double)v2.x; acc[9] += (double)v2.y; acc[10] += (double)v2.z; acc[11] += (double)v2.w;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = wave_sum_d(acc[k]);
  if (lane == 0) {
    const float* Kp = A.intrinsics + ((size_t)b * A.n_scales + s) * 9;
    double K[9], Ki[9], R[9], t[3], gPm[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) K[k] = (double)Kp[k];
    inv3_d(K, Ki);
    const float* pp = A.pose[0];      // (selected, not indexed: the argument block stays in scalar registers)
#pragma unroll
    for (int k = 1; k < SFM_MAX_SRC; ++k) pp = (i == k) ? A.pose[k] : pp;
    pose_rt_d(pp + (size_t)b * 6, R, t);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int j = 0; j < 3; ++j) gPm[k * 4 + j] = Ki[j * 3 + 0] * acc[k * 4 + 0] + Ki[j * 3 + 1] * acc[k * 4 + 1] + Ki[j * 3 + 2] * acc[k * 4 + 2];
      gPm[k * 4 + 3] = acc[k * 4 + 3];
    }
    if (A.d_proj) {
      float* o = A.d_proj + (((size_t)b * A.n_scales + s) * A.n_src + i) * 12;
#pragma unroll
      for (int k = 0; k < 12; ++k) o[k] = (float)gPm[k];
    }
    double g3[9], m1[9], m2[9], m3[9], dK[9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) { g3[k * 3 + j] = gPm[k * 4 + j]; dK[k * 3 + j] = 0.0; }
    dk_from_gpm_d(gPm, R, t, dK);
    mat3_mul_tn_d(K, g3, m1);      // K^T . gPm3
    mat3_mul_tn_d(R, m1, m2);      // R^T . K^T . gPm3
    mat3_mul_tn_d(Ki, m2, m3);     // K^-T . R^T . K^T . gPm3
#pragma unroll
    for (int k = 0; k < 9; ++k) dk_of[i][k] = dK[k] - m3[k];
  }
  __syncthreads();
  if (A.d_intr && threadIdx.x < 9) {
    double a = dk_of[0][threadIdx.x];
    for (int k = 1; k < A.n_src; ++k) a += dk_of[k][threadIdx.x];
    A.d_intr[((size_t)b * A.n_scales + s) * 9 + threadIdx.x] = (float)a;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// The preloaded launch header of both launches (make_hdr, finalize_kernel), packed once, when the plan is made.
struct PackedHdr {
  bool compact;        // false (a tile count or B beyond 16 bits): the kernels read the fields from the struct
  unsigned bsc;        // B | n_src << 16 | n_scales << 20
  unsigned tiles[4];   // tiles_of[] as 16-bit halves
};

struct Plan {
  LossArgs args;
  size_t off_loss, off_gpm, total;
  size_t off_rec[SFM_MAX_SCALES];   // with d_src bound: the record of dL/dI^ of the scale (B, 3 n_src, h, w) that the second launch reads
  DsrcArgs dsrc_args;               // ... and that launch (dsrc_scatter_kernel, sfm_loss_dsrc.hip)
  Variant v;                        // the main kernel (choose_variant)
  const void* kernel;               // ... its __global__, resolved here so that a cached plan launches without another look-up
  bool dsrc;                        // the CALL also produces dL/d(src): the main launch records dL/dI^ and a second launch follows
  PackedHdr hdr;
};

struct Entry { bool grad, loss; };          // the entry point: sfm_loss_fwd {0, 1}, sfm_loss_bwd {1, 0}, sfm_loss_fwd_bwd {1, 1}
enum class Outputs { Unchecked, Checked };  // Checked: a call that writes them (the queries plan from the descriptor's shape alone)

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The one-call hooks of the calling thread: they hold for the NEXT sfm_loss_* call only, whatever becomes of it.
constexpr int HOOK_STRUCT_HEADER = 3;   // sfm_loss_variant: the header read from the struct (the path of counts beyond 16 bits)
constexpr int HOOK_ONE_SOURCE = 4, HOOK_TWO_SOURCES = 5;   // ... one source per pass / two where possible, whatever the default
struct Hooks {
  int variant;                      // sfm_loss_variant
  unsigned long long* trace;        // sfm_loss_debug_trace
  hipEvent_t ev_start, ev_stop;     // sfm_loss_profile_events: recorded right before / after the main kernel
};
static thread_local Hooks g_hooks = {};
static int pair_hook_of(const int variant) { return variant == HOOK_ONE_SOURCE ? 0 : (variant == HOOK_TWO_SOURCES ? 1 : -1); }

// ---- work decomposition -----------------------------------------------------------------
// One wavefront per (scale, sample, strip, chunk of rows).  A wave lives for the whole launch, so the chunk
// height is chosen such that all items fit in as few full "rounds" of resident waves as possible while the
// halo rows (recomputed per chunk) stay a small fraction.  The number of resident waves follows from the
// __launch_bounds__ of the kernel variant (waves_per_simd; LDS and the 32-waves-per-CU cap allow more) and
// from the CU count of the device -- no occupancy query, nothing that differs between a CPU-only host and
// the GPU box.
constexpr int MI355X_CUS = 256;   // 8 XCDs x 32 CUs (MI355X_MICROARCH.md); used when no device is visible

static int device_cus() {
  static int cus_of[64];   // 0 = not asked yet; a benign race writes the same value twice
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return MI355X_CUS; }
  if (cus_of[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = MI355X_CUS; }
    cus_of[dev] = cus;
  }
  return cus_of[dev];
}

// tuning overrides (development only), read from the environment ONCE per process
struct Tuning {
  int chunk_rows = 0;                       // SFM_CHUNK_ROWS: fixed target height
  int rows_list[SFM_MAX_SCALES] = {0};      // SFM_CHUNK_ROWS_LIST: chunk height per scale, "13,13,16,8"
  bool has_prio = false;
  unsigned prio_tab = 0;                    // SFM_PRIO_TABLE: "0123,3210" = levels of ranks 0.. in phase 1, phase 2
  bool no_wide = false;                     // SFM_NO_WIDE: small L1 launches on the four-wave build too
  int pair = -1;                            // SFM_PAIR=0 / 1: never / whenever possible two sources per pass (default: choose_variant decides)
  bool no_fill = false;                     // SFM_NO_FILL: no slot-filling refinement of the chunk heights (plan_chunks)
  int deal_below = 8;                       // SFM_DEAL_ITEMS_BELOW: batches smaller than this have their ITEMS dealt out over the XCDs (8 contiguous
                                            // ranges of the item list) instead of whole samples (b mod 8).  Measured at B = 8 (9): cfg5_2src +9.9 %,
                                            // cfg5 +3 %, cfg2 +1.6 %; items round-robin +22 .. +48 % (profiles/r05_wave_stage_stamps_cfg5_2src.txt)
  Tuning() {
    if (const char* e = getenv("SFM_DEAL_ITEMS_BELOW")) deal_below = atoi(e);
    no_wide = getenv("SFM_NO_WIDE") != nullptr;
    no_fill = getenv("SFM_NO_FILL") != nullptr;
    if (const char* e = getenv("SFM_PAIR")) pair = atoi(e) != 0;
    if (const char* e = getenv("SFM_CHUNK_ROWS")) chunk_rows = atoi(e);
    if (const char* rl = getenv("SFM_CHUNK_ROWS_LIST")) {
      for (int k = 0; *rl && k < SFM_MAX_SCALES; ++k) {
        rows_list[k] = atoi(rl);
        while (*rl && *rl != ',') ++rl;
        if (*rl == ',') ++rl;
      }
    }
    if (const char* pt = getenv("SFM_PRIO_TABLE")) {
      int phase = 0, r = 0;
      for (; *pt; ++pt) {
        if (*pt == ',') { phase = 1; r = 0; }
        else if (*pt >= '0' && *pt <= '3' && r < 4) { prio_tab |= (unsigned)(*pt - '0') << (8 * phase + 2 * r); ++r; }
      }
      has_prio = true;
    }
  }
};
static const Tuning& tuning() { static const Tuning t; return t; }

// chunk height per scale for a target height T: equal chunks, never more than T rows
static void chunk_layout(const SfmLossDesc* d, int sw, int halo2, int T, int* rows, long long* items, long long* work, int* maxcost) {
  // (T: at most this many rows per chunk)
  *items = 0; *work = 0; *maxcost = 0;
  for (int s = 0; s < d->n_scales; ++s) {
    const int h = d->H[s], strips = (d->W[s] + sw - 1) / sw;
    const int n = (h + T - 1) / T;
    rows[s] = (h + n - 1) / n;
    const int cost = rows[s] + halo2;
    const long long cnt = (long long)d->B * strips * ((h + rows[s] - 1) / rows[s]);
    *items += cnt;
    *work += cnt * cost;
    if (cost > *maxcost) *maxcost = cost;
  }
}

static void plan_chunks(const SfmLossDesc* d, int sw, int halo2, int slots, int passes /* walks of a wave down its chunk */, int* rows,
                        const int max_rows = MAX_CHUNK_ROWS) {
  const int forced = tuning().chunk_rows;
  int bestT = max_rows;
  double best = 1e300;
  for (int T = MIN_CHUNK_ROWS; T <= max_rows; ++T) {
    if (forced >= MIN_CHUNK_ROWS && forced <= MAX_CHUNK_ROWS && T != forced) continue;
    long long items, work;
    int maxcost, r[SFM_MAX_SCALES];
    chunk_layout(d, sw, halo2, T, r, &items, &work, &maxcost);
    const double rounds = (double)((items + slots - 1) / slots);
    // resident waves run concurrently: a launch lasts about `rounds` times the longest item, and never
    // less than the total work spread over all slots
    double est = rounds * maxcost;
    const double flat = (double)work / slots;
    if (flat > est) est = flat;
    est += 1e-3 * (double)work / slots;   // tie-break: less recomputed halo
    if (est < best) { best = est; bestT = T; }
  }
  long long items, work;
  int maxcost;
  chunk_layout(d, sw, halo2, bestT, rows, &items, &work, &maxcost);
  // Refinement for launches that fit ONE resident round: the equal-height search above leaves slots empty (cfg3: 2912 items on
  // 3072 slots, i.e. 160 SIMDs with two waves instead of three, which finish at 31-48 us of a 55 us launch).  The empty slots are
  // filled by splitting the chunks of the scale with the tallest chunks that still fits, one more chunk at a time: every extra
  // chunk costs its halo rows again (+1 % of the row steps at cfg3).  Measured (profiles/r04_ab_chunk_fill.txt): the main kernel gets
  // 1.5 - 2.2 % shorter where a wave is SHORT -- B = 16 / 24 / 32 at 128x416 with two sources, cfg5 with two sources -- and 3 - 5 %
  // LONGER where it is long (cfg5 with four sources: 17 steps x 4; B = 48: 26 steps x 2), so the refinement is applied while a
  // wave's row steps, tallest chunk x sources, stay within 40.
  if (!tuning().no_fill && items <= slots && !(forced >= MIN_CHUNK_ROWS && forced <= MAX_CHUNK_ROWS) && (long long)maxcost * passes <= 40) {
    for (;;) {
      int pick = -1, pick_rows = 0;
      long long pick_add = 0;
      for (int s = 0; s < d->n_scales; ++s) {
        const int h = d->H[s], strips = (d->W[s] + sw - 1) / sw;
        const int chunks = (h + rows[s] - 1) / rows[s];
        if (rows[s] <= MIN_CHUNK_ROWS) continue;
        const int nr = (h + chunks) / (chunks + 1);                 // ceil(h / (chunks + 1))
        if (nr < MIN_CHUNK_ROWS || nr >= rows[s]) continue;
        const long long add = (long long)d->B * strips * ((h + nr - 1) / nr - chunks);
        if (add <= 0 || items + add > slots) continue;
        if (rows[s] > pick_rows) { pick = s; pick_rows = rows[s]; pick_add = add; }
      }
      if (pick < 0) break;
      const int h = d->H[pick], chunks = (h + rows[pick] - 1) / rows[pick];
      rows[pick] = (h + chunks) / (chunks + 1);
      items += pick_add;
    }
  }
  for (int k = 0; k < d->n_scales; ++k) {
    const int v = tuning().rows_list[k];
    if (v >= MIN_CHUNK_ROWS && v <= max_rows) rows[k] = v;
  }
}

// upper bound of the item count over every chunking plan_chunks can choose (chunks are never shorter than
// MIN_CHUNK_ROWS unless the image is): what sfm_loss_workspace_bytes sizes for, on any host
static long long max_items(const SfmLossDesc* d, int sw) {
  long long items = 0;
  for (int s = 0; s < d->n_scales; ++s) {
    const int h = d->H[s], strips = (d->W[s] + sw - 1) / sw;
    items += (long long)d->B * strips * ((h + MIN_CHUNK_ROWS - 1) / MIN_CHUNK_ROWS);
  }
  return items;
}

constexpr int PAIR_BELOW_ROWS = 12;   // see choose_variant

// ---- the plan, in stages ----------------------------------------------------------------
// what a descriptor must satisfy whatever the entry point; the output arrays are left to validate_outputs
static int validate(const SfmLossDesc* d) {
  if (!d) return fail(SFM_ERR_NULL, "sfm_loss: NULL descriptor");
  if (d->B < 0 || d->B > (1 << 20)) return fail(SFM_ERR_SHAPE, "sfm_loss: B=%d", d->B);
  if (d->norm_B < d->B || d->norm_B < 1) return fail(SFM_ERR_CONFIG, "sfm_loss: norm_B=%d must be >= max(B,1) (B=%d)", d->norm_B, d->B);
  if (d->n_src < 1 || d->n_src > SFM_MAX_SRC) return fail(SFM_ERR_SHAPE, "sfm_loss: n_src=%d not in [1,%d]", d->n_src, SFM_MAX_SRC);
  if (d->n_scales < 1 || d->n_scales > SFM_MAX_SCALES)
    return fail(SFM_ERR_SHAPE, "sfm_loss: n_scales=%d not in [1,%d]", d->n_scales, SFM_MAX_SCALES);
  if (!(d->ssim_rate >= 0.f && d->ssim_rate <= 1.f)) return fail(SFM_ERR_CONFIG, "sfm_loss: ssim_rate=%g not in [0,1]", d->ssim_rate);
  if (!(d->smooth_reg >= 0.f) || !(d->exp_reg >= 0.f)) return fail(SFM_ERR_CONFIG, "sfm_loss: negative regulariser weight");
  if (d->smooth_mode < SFM_SMOOTH_NONE || d->smooth_mode > SFM_SMOOTH_EDGE_AWARE)
    return fail(SFM_ERR_CONFIG, "sfm_loss: smooth_mode=%d", d->smooth_mode);
  if (!d->intrinsics) return fail(SFM_ERR_NULL, "sfm_loss: intrinsics is NULL");
  if (d->image_layout != SFM_LAYOUT_PLANAR && d->image_layout != SFM_LAYOUT_HWC)
    return fail(SFM_ERR_CONFIG, "sfm_loss: image_layout=%d", d->image_layout);
  if (d->projection != SFM_PROJECTION_FAST && d->projection != SFM_PROJECTION_REFERENCE_ORDER)
    return fail(SFM_ERR_CONFIG, "sfm_loss: projection=%d", d->projection);
  for (int i = 0; i < d->n_src; ++i)
    if (!d->pose[i]) return fail(SFM_ERR_NULL, "sfm_loss: pose[%d] is NULL", i);
  for (int s = 0; s < d->n_scales; ++s) {
    const int h = d->H[s], w = d->W[s];
    if (h < 3 || w < 3) return fail(SFM_ERR_SHAPE, "sfm_loss: scale %d is %dx%d, need H,W >= 3", s, h, w);
    if ((long long)d->B * 3 * d->n_src * h * w >= (1ll << 31)) return fail(SFM_ERR_SHAPE, "sfm_loss: scale %d too large", s);
    // (byte offsets inside one pixel-interleaved image are formed exactly in fp32 by the gather of the HWC kernels)
    if (d->image_layout == SFM_LAYOUT_HWC && (long long)h * w * 12 >= (1ll << 24))
      return fail(SFM_ERR_SHAPE, "sfm_loss: scale %d is %dx%d, SFM_LAYOUT_HWC takes images of fewer than 2^24 / 12 pixels", s, h, w);
    if (!d->tgt[s] || !d->src[s] || !d->disp[s]) return fail(SFM_ERR_NULL, "sfm_loss: tgt/src/disp[%d] is NULL", s);
    // (the second launch of a call with d_src addresses the record of one (sample, source) with 32-bit byte offsets)
    if (d->d_src[s] && (long long)h * w * 12 >= (1ll << 32)) return fail(SFM_ERR_SHAPE, "sfm_loss: scale %d is %dx%d, d_src takes images of fewer than 2^32 / 12 pixels", s, h, w);
    if (d->exp_reg > 0.f && !d->mask_logits[s]) return fail(SFM_ERR_NULL, "sfm_loss: exp_reg > 0 but mask_logits[%d] is NULL", s);
  }
  return SFM_OK;
}

// the arrays the entry point writes (a valid descriptor)
static int validate_outputs(const SfmLossDesc* d, const Entry e) {
  if (e.loss) {      // the optional warped-image output: an array for every scale or for none
    int n_w = 0;
    for (int s = 0; s < d->n_scales; ++s) n_w += d->warped[s] != nullptr;
    if (n_w != 0 && n_w != d->n_scales) return fail(SFM_ERR_NULL, "sfm_loss: warped[] is set for %d of %d scales (all or none)", n_w, d->n_scales);
  }
  if (!e.grad) return SFM_OK;
  for (int i = 0; i < d->n_src; ++i)
    if (!d->d_pose[i]) return fail(SFM_ERR_NULL, "sfm_loss: d_pose[%d] is NULL", i);
  for (int s = 0; s < d->n_scales; ++s) {
    if (!d->d_disp[s]) return fail(SFM_ERR_NULL, "sfm_loss: d_disp[%d] is NULL", s);
    if (d->exp_reg > 0.f && !d->d_mask[s]) return fail(SFM_ERR_NULL, "sfm_loss: exp_reg > 0 but d_mask[%d] is NULL", s);
  }
  return SFM_OK;
}

static bool any_bound(float* const* arr, const int n) {
  for (int s = 0; s < n; ++s)
    if (arr[s]) return true;
  return false;
}

// Which kernel serves the launch.  It follows from the descriptor's pointers whether or not the call checks its outputs, so that
// sfm_loss_plan_info reports the launch the call will make.  `pair_hook`: 0 / 1 = the one-call hook's choice, -1 = none.
static Variant choose_variant(const SfmLossDesc* d, const Entry e, const int cus, const int pair_hook) {
  Variant v = {};
  v.grad = e.grad;
  v.loss = e.loss;
  v.expl = d->exp_reg > 0.f;                       // base_model.py:86,103
  v.ssim = !v.expl && d->ssim_rate > 0.f;          // base_model.py:110-112
  v.smode = d->smooth_reg > 0.f ? d->smooth_mode : SFM_SMOOTH_NONE;   // base_model.py:75
  v.hwc = d->image_layout == SFM_LAYOUT_HWC;
  v.warped = e.loss && any_bound(d->warped, d->n_scales);
  v.family = Family::Base;
  const HaloCols hc = halo_of(v);
  if (d->projection == SFM_PROJECTION_REFERENCE_ORDER) {
    v.family = Family::Ref;                        // (these kernels record dL/dI^ themselves when d_src is bound)
  } else if (e.grad && any_bound(d->d_src, d->n_scales)) {
    v.family = Family::Dsrc;
  } else if (e.grad && v.ssim && v.hwc && !v.warped && d->n_src % 2 == 0) {
    // Two sources per pass (loss_kernel_pair): the SSIM gradient launches of the pixel-interleaved layout with an even number of
    // sources, without the warped output.  By default where it measured faster (profiles/r06_pair_kernel.txt): launches whose
    // one-source plan has to cut the largest scale into chunks of at most PAIR_BELOW_ROWS rows to fill the chip (B <= 24 at 128x416:
    // -2 ... -12 % kernel time; the halo rows of short chunks are what the taller chunks of two thirds as many waves save).  At
    // BASELINE cfg3 / cfg5 (15 / 13 rows) it is 1 - 5 % SLOWER -- 11 % fewer vector instructions, issued 12 % less densely by two
    // waves per SIMD than by three -- and is not used.
    int rows1[SFM_MAX_SCALES];
    plan_chunks(d, hc.sw, 2 * hc.hr, cus * 4 * waves_per_simd(v), d->n_src, rows1);
    bool pair = rows1[0] <= PAIR_BELOW_ROWS;
    if (tuning().pair >= 0) pair = tuning().pair != 0;
    if (pair_hook >= 0) pair = pair_hook != 0;
    if (pair) v.family = Family::Pair;
  } else if (e.grad && !v.ssim && !v.expl && !tuning().no_wide &&
             max_items(d, hc.sw) <= (long long)cus * 4 * waves_per_simd(Family::Wide, false, true)) {
    v.family = Family::Wide;   // (a launch is "small" when even at the smallest chunk height its waves fit the SIMDs three deep)
  }
  return v;
}

static const void* kernel_of(const Variant& v) {
  switch (v.family) {
    case Family::Wide: return lift_variant<Family::Wide>(v);
    case Family::Pair: return kernel_of_pair(v);
    case Family::Ref: return kernel_of_ref(v);
    case Family::Dsrc: return kernel_of_dsrc(v);
    default: return lift_variant<Family::Base>(v);
  }
}

// the inputs, the outputs of the entry point (validate_outputs has seen them where the plan is one a call launches) and the
// per-scale constants
static void fill_args(const SfmLossDesc* d, const Variant& v, LossArgs& A) {
  memset(&A, 0, sizeof(A));
  A.B = d->B;
  A.n_src = d->n_src;
  A.n_scales = d->n_scales;
  A.alpha = d->ssim_rate;
  A.intrinsics = d->intrinsics;
  for (int i = 0; i < d->n_src; ++i) {
    A.pose[i] = d->pose[i];
    if (v.grad) A.d_pose[i] = d->d_pose[i];
  }
  for (int s = 0; s < d->n_scales; ++s) {
    ScaleArgs& S = A.sc[s];
    const int h = d->H[s], w = d->W[s];
    S.tgt = d->tgt[s];
    S.src = d->src[s];
    S.disp = d->disp[s];
    S.mlog = v.expl ? d->mask_logits[s] : nullptr;
    S.warped = v.loss ? d->warped[s] : nullptr;
    if (v.grad) {
      S.d_disp = d->d_disp[s];
      S.d_mask = v.expl ? d->d_mask[s] : nullptr;
      S.d_src = d->d_src[s];
    }
    S.h = h;
    S.w = w;
    const double nb = (double)d->norm_B;
    S.inv_cnt = (float)(1.0 / (nb * 3.0 * h * w));
    const double wgt = (double)d->smooth_reg / (double)(1 << s);               // base_model.py:76
    S.c_dx2 = (float)(wgt / (nb * h * (w - 2)));
    S.c_dy2 = (float)(wgt / (nb * (h - 2) * w));
    S.c_dxy = (float)(wgt / (nb * (h - 1) * (w - 1)));
    S.c_ex = (float)(wgt / (nb * h * (w - 1)));
    S.c_ey = (float)(wgt / (nb * (h - 1) * w));
    S.c_exp = (float)((double)d->exp_reg / (nb * h * w));
  }
}

// the items of the launch: chunk heights, tiles per scale, and how the waves of a SIMD share it (issue priorities, dealing)
static void plan_items(const SfmLossDesc* d, const Variant& v, const int cus, LossArgs& A) {
  const HaloCols hc = halo_of(v);
  const int waves = waves_per_simd(v);
  A.simds_per_xcd = (cus % 8 == 0) ? cus / 8 * 4 : 128;   // gfx950: 8 XCDs, 4 SIMDs per CU
  A.prio_top = waves - 1 < 3 ? waves - 1 : 3;
  A.prio_tab = 0;
  for (int r = 0; r <= A.prio_top; ++r)   // youngest preferred in the first half of the sources, oldest in the second
    A.prio_tab |= (unsigned)r << (2 * r) | (unsigned)(A.prio_top - r) << (8 + 2 * r);
  if (tuning().has_prio) A.prio_tab = tuning().prio_tab & 0xffffu;
  if (d->B < (tuning().deal_below > 8 ? tuning().deal_below : 8)) A.prio_tab |= 0x80000000u;   // fewer samples than XCDs (or asked for): deal items
  int rows[SFM_MAX_SCALES];
  plan_chunks(d, hc.sw, 2 * hc.hr, cus * 4 * waves, d->n_src / sources_per_pass(v.family), rows);
  int items = 0;
  for (int s = 0; s < d->n_scales; ++s) {
    ScaleArgs& S = A.sc[s];
    S.strips = (S.w + hc.sw - 1) / hc.sw;
    S.chunk_rows = rows[s];
    S.chunks = (S.h + rows[s] - 1) / rows[s];
    S.tiles = S.strips * S.chunks;
    S.item_begin = items;
    A.tiles_of[s] = S.tiles;
    A.item_begin_of[s] = items;
    items += d->B * S.tiles;
  }
  A.items = items;
}

// The preloaded header: B, n_src, n_scales and the tile counts packed, where they fit their fields.
static PackedHdr pack_header(const LossArgs& A) {
  PackedHdr h = {};
  h.compact = A.B <= (int)HDR_B_MASK && A.n_src <= (int)HDR_NIBBLE && A.n_scales <= (int)HDR_NIBBLE;
  for (int k = 0; k < SFM_MAX_SCALES; ++k) h.compact = h.compact && A.tiles_of[k] >= 0 && A.tiles_of[k] <= (int)HDR_TILE_MASK;
  if (!h.compact) return h;
  h.bsc = (unsigned)A.B | (unsigned)A.n_src << HDR_SRC_SHIFT | (unsigned)A.n_scales << HDR_SCALES_SHIFT;
  for (int k = 0; k < SFM_MAX_SCALES; ++k) h.tiles[hdr_tile_word(k)] |= (unsigned)A.tiles_of[k] << hdr_tile_shift(k);
  return h;
}

static void set_gy(Plan& p, const float gy);
static void plan_dsrc(const SfmLossDesc* d, const int cus, Plan& p);

// The workspace layout does not depend on the chunking (nor on the device): the two partial-sum arrays are placed
// and sized for the largest item count any chunking can produce.
static int plan_workspace(const SfmLossDesc* d, const int cus, Plan& p) {
  const size_t cap = (size_t)max_items(d, halo_of(p.v).sw);
  if ((size_t)p.args.items > cap) return fail(SFM_ERR_CONFIG, "sfm_loss: internal error: %d items exceed the bound %zu", p.args.items, cap);
  p.off_loss = 0;
  p.off_gpm = align_up(p.off_loss + cap * 4 * sizeof(float), 256);
  p.total = align_up(p.off_gpm + cap * d->n_src * 12 * sizeof(float), 256);
  // dL/d(src): the record of dL/dI^ per scale that binds d_src (whatever the entry point: the workspace is sized from the descriptor)
  plan_dsrc(d, cus, p);
  return SFM_OK;
}

// validates the descriptor and lays out items + workspace for the given entry point
static int make_plan(const SfmLossDesc* d, const Entry e, const Outputs out, const float gy, Plan& p, const int pair_hook = -1) {
  if (int err = validate(d)) return err;
  if (out == Outputs::Checked)
    if (int err = validate_outputs(d, e)) return err;
  const int cus = device_cus();
  p.v = choose_variant(d, e, cus, pair_hook);
  p.dsrc = e.grad && any_bound(d->d_src, d->n_scales);
  p.kernel = kernel_of(p.v);
  if (!p.kernel) return fail(SFM_ERR_CONFIG, "sfm_loss: internal error: no kernel of family %d for this launch", (int)p.v.family);
  fill_args(d, p.v, p.args);
  plan_items(d, p.v, cus, p.args);
  set_gy(p, gy);
  p.hdr = pack_header(p.args);
  return plan_workspace(d, cus, p);
}

// The second launch of a call with d_src bound: bands, window and workgroups (DsrcArgs), and the place of the records in the workspace.
static void plan_dsrc(const SfmLossDesc* d, const int cus, Plan& p) {
  DsrcArgs& D = p.dsrc_args;
  memset(&D, 0, sizeof(D));
  D.B = d->B; D.n_src = d->n_src; D.n_scales = d->n_scales;
  D.intrinsics = d->intrinsics;
  D.ref = d->projection == SFM_PROJECTION_REFERENCE_ORDER;
  for (int i = 0; i < d->n_src; ++i) D.pose[i] = d->pose[i];
  // bands of at most max_segs 64-lane segments: as wide as possible (fewer overlapping windows) while the largest scale still gives
  // half the CUs a workgroup
  int max_segs = DSRC_MAX_SEGS;
  int lds_bytes = DSRC_LDS_BYTES;
  D.margin = DSRC_MARGIN;
  if (const char* e = getenv("SFM_DSRC_SEGS")) max_segs = atoi(e) >= 2 ? 2 : 1;        // (development)
  if (const char* e = getenv("SFM_DSRC_LDS_KB")) lds_bytes = atoi(e) * 1024 < lds_bytes ? atoi(e) * 1024 : lds_bytes;
  if (const char* e = getenv("SFM_DSRC_MARGIN")) D.margin = atoi(e);
  int s0 = -1;
  for (int s = 0; s < d->n_scales; ++s)
    if (d->d_src[s] && s0 < 0) s0 = s;
  if (s0 >= 0)
    while (max_segs > 1 && (long long)d->B * d->n_src * ((d->W[s0] + 64 * max_segs - 1) / (64 * max_segs)) < cus / 2) max_segs >>= 1;
  int wgs = 0, widest = 0;
  for (int s = 0; s < d->n_scales; ++s) {
    p.off_rec[s] = 0;
    DsrcScale& S = D.sc[s];
    S.wg_begin = wgs;
    if (!d->d_src[s]) continue;
    const int h = d->H[s], w = d->W[s];
    p.off_rec[s] = p.total;
    p.total = align_up(p.total + (size_t)d->B * d->n_src * 3 * h * w * sizeof(float), 256);
    S.disp = d->disp[s];
    S.d_src = d->d_src[s];
    S.h = h; S.w = w;
    S.bands = (w + 64 * max_segs - 1) / (64 * max_segs);
    S.band_w = (w + S.bands - 1) / S.bands;
    const int segs = (S.band_w + 63) / 64;
    S.seg_shift = segs > 1 ? 1 : 0;
    wgs += d->B * d->n_src * S.bands;
    if (S.band_w > widest) widest = S.band_w;
  }
  D.wgs = wgs;
  D.win_cols = widest + 2 * D.margin;
  if (D.win_cols < 16) D.win_cols = 16;
  // as many rows as the LDS holds, at most 64
  int rows = 64;
  while (rows > 8 && dsrc_lds_bytes(rows, D.win_cols) > (size_t)lds_bytes) --rows;
  D.win_rows = rows;
  D.nq = (D.win_cols + 63) / 64;
  D.nq_inv16 = (65536 + D.nq - 1) / D.nq;
}

static void set_gy(Plan& p, const float gy) {
  LossArgs& A = p.args;
  A.gy = gy;
  for (int s = 0; s < A.n_scales; ++s) {
    ScaleArgs& S = A.sc[s];
    S.k_pix = gy * (1.0f - A.alpha) * S.inv_cnt;
    S.kq = -gy * A.alpha * S.inv_cnt;
    S.k_exp = gy * S.c_exp;
  }
}

static void bind_workspace(Plan& p, void* ws) {
  char* base = (char*)ws;
  p.args.part_loss = (float*)(base + p.off_loss);
  p.args.part_gpm = (float*)(base + p.off_gpm);
  if (p.dsrc)
    for (int s = 0; s < p.args.n_scales; ++s)
      if (p.dsrc_args.sc[s].d_src) {
        p.args.sc[s].d_src = (float*)(base + p.off_rec[s]);       // the main launch writes the record ...
        p.dsrc_args.sc[s].rec = (const float*)(base + p.off_rec[s]);   // ... the second launch reads it
      }
}

static hipError_t launch_main(const Plan& p, const Hooks& hooks, hipStream_t st) {
  LossArgs args = p.args;
  // the preloaded header (make_hdr); HOOK_STRUCT_HEADER (tests): the header read from the struct
  const PackedHdr hdr = hooks.variant == HOOK_STRUCT_HEADER ? PackedHdr{} : p.hdr;
  unsigned h_bn = hdr.compact ? hdr.bsc | (unsigned)args.prio_top << HDR_PRIO_SHIFT | 1u << HDR_COMPACT_BIT : 0u;
  unsigned h_t[4] = {hdr.tiles[0], hdr.tiles[1], hdr.tiles[2], hdr.tiles[3]};
  void* kargs[] = {&h_bn, &args.items, &args.simds_per_xcd, &args.prio_tab, &h_t[0], &h_t[1], &h_t[2], &h_t[3], &args.trace, &args};
  // 8 x (items of the busiest XCD): see the item mapping at the top of loss_kernel
  int tiles_per_sample = 0;
  for (int s = 0; s < p.args.n_scales; ++s) tiles_per_sample += p.args.sc[s].tiles;
  const int per_xcd = (int)p.args.prio_tab >= 0 ? (p.args.B / 8) * tiles_per_sample + ((p.args.B % 8) * tiles_per_sample + 7) / 8 : (p.args.items + 7) / 8;
  // With profiling events the kernel is launched through hipExtLaunchKernel: the events then carry the begin / end
  // timestamps of THIS dispatch (what rocprofv3's kernel trace reports), and no marker packets are put between the
  // launches of a step (hipEventRecord on either side of the kernel costs the step several microseconds).
  const size_t smem = 0;
  if (hooks.ev_start && hooks.ev_stop)
    return hipExtLaunchKernel(p.kernel, dim3(8 * per_xcd), dim3(64 * WAVES_PER_BLOCK), kargs, smem, st, hooks.ev_start, hooks.ev_stop, 0);
  return hipLaunchKernel(p.kernel, dim3(8 * per_xcd), dim3(64 * WAVES_PER_BLOCK), kargs, smem, st);
}

static void launch_finalize(const Plan& p, const Hooks& hooks, float* loss5, hipStream_t st) {
  const LossArgs& a = p.args;
  const PackedHdr hdr = hooks.variant == HOOK_STRUCT_HEADER ? PackedHdr{} : p.hdr;
  const unsigned bsc = (hdr.compact ? hdr.bsc | FIN_COMPACT : 0u) | (p.v.grad ? FIN_POSE : 0u) | (p.v.loss ? FIN_LOSS : 0u);
  const int n_pose_blocks = p.v.grad ? a.B * a.n_src : 0;
  hipLaunchKernelGGL(finalize_kernel, dim3(n_pose_blocks + 1), dim3(64 * FINALIZE_WAVES), 0, st, (const float*)a.part_gpm, a.intrinsics, a.pose[0],
                     a.pose[1], bsc, hdr.tiles[0], hdr.tiles[1], hdr.tiles[2], hdr.tiles[3], (unsigned)(p.off_gpm - p.off_loss), a,
                     p.v.loss ? loss5 : (float*)nullptr);
}

// The plan of a descriptor depends only on the descriptor's bytes and the entry point: the last few are kept per
// thread, so that a training loop that calls with the same buffers every step does the validation and the chunk
// search once.  (Thread-local, like the error string: no state is shared between threads.)
struct CachedPlan {
  SfmLossDesc desc;
  int device, pair_hook;
  Entry entry;
  bool valid;
  Plan plan;
};
constexpr int PLAN_CACHE = 4;
static thread_local CachedPlan g_plans[PLAN_CACHE];
static thread_local unsigned g_plan_clock = 0;

static int cached_plan(const SfmLossDesc* d, const Entry e, float gy, Plan& out, const int pair_hook) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; }
  for (int k = 0; k < PLAN_CACHE; ++k) {
    CachedPlan& c = g_plans[k];
    if (c.valid && c.entry.grad == e.grad && c.entry.loss == e.loss && c.device == dev && c.pair_hook == pair_hook &&
        memcmp(&c.desc, d, sizeof(SfmLossDesc)) == 0) {
      out = c.plan;
      set_gy(out, gy);
      return SFM_OK;
    }
  }
  if (int err = make_plan(d, e, Outputs::Checked, gy, out, pair_hook)) return err;
  CachedPlan& c = g_plans[g_plan_clock++ % PLAN_CACHE];
  c.desc = *d; c.device = dev; c.pair_hook = pair_hook; c.entry = e; c.plan = out; c.valid = true;
  return SFM_OK;
}

// `frames` (sfm_step_*): the full-resolution frames whose pyramids are written into d->tgt[] / d->src[] first -- after every
// argument of the call has been checked, so that a rejected call has launched nothing and written nothing.  nullptr: sfm_loss_*.
struct Frames { const float *tgt, *src; };

static int run(const SfmLossDesc* d, const Entry e, float gy, float* loss5, void* ws, size_t ws_bytes, void* stream, const char* who,
               const Frames* frames) {
  hipStream_t st = (hipStream_t)stream;
  // the one-call hooks are taken -- and forgotten -- here, whatever becomes of the call
  const Hooks hooks = g_hooks;
  g_hooks = Hooks{};
  if (d && d->B == 0) {   // empty shard: nothing to launch (input pointers of empty arrays may be NULL)
    if (e.loss) {
      if (!loss5) return fail(SFM_ERR_NULL, "%s: loss5 is NULL", who);
      hipError_t err = hipMemsetAsync(loss5, 0, 5 * sizeof(float), st);
      if (err != hipSuccess) return fail((int)err, "%s: memset: %s", who, hipGetErrorString(err));
    }
    return SFM_OK;
  }
  if (!d) return fail(SFM_ERR_NULL, "%s: NULL descriptor", who);
  Plan p;
  if (int err = cached_plan(d, e, gy, p, pair_hook_of(hooks.variant))) return err;
  if (e.loss && !loss5) return fail(SFM_ERR_NULL, "%s: loss5 is NULL", who);
  if (!ws || ws_bytes < p.total) return fail(SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, p.total, ws_bytes);
  if (((uintptr_t)ws & 255) != 0) return fail(SFM_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
  if (frames)
    if (int err = sfm_pyramid_pair_hwc_fwd(frames->tgt, frames->src, (float* const*)d->tgt, (float* const*)d->src, d->B, d->n_src, d->H[0],
                                           d->W[0], d->n_scales, stream))
      return err;
  bind_workspace(p, ws);
  p.args.trace = hooks.trace;
  hipError_t le = launch_main(p, hooks, st);
  if (le != hipSuccess) return fail((int)le, "%s: launch of the main kernel: %s", who, hipGetErrorString(le));
  if (p.dsrc) {      // dL/d(src) from the record the main launch has just written
    le = launch_dsrc_scatter(p.dsrc_args, st);
    if (le != hipSuccess) return fail((int)le, "%s: launch of the d_src kernel: %s", who, hipGetErrorString(le));
  }
  launch_finalize(p, hooks, loss5, st);
  return check_launch(who);
}

constexpr Entry ENTRY_FWD = {false, true}, ENTRY_BWD = {true, false}, ENTRY_FWD_BWD = {true, true};

}  // namespace sfm

extern "C" {

size_t sfm_loss_workspace_bytes(const SfmLossDesc* desc) {
  // the three entry points lay their work out differently: size for the largest
  size_t total = 0;
  for (const sfm::Entry e : {sfm::ENTRY_FWD, sfm::ENTRY_BWD, sfm::ENTRY_FWD_BWD}) {
    sfm::Plan p;
    if (sfm::make_plan(desc, e, sfm::Outputs::Unchecked, 1.f, p) != SFM_OK) return 0;
    if (p.total > total) total = p.total;
  }
  return total;
}

int sfm_loss_plan_info(const SfmLossDesc* desc, int grad, int loss, int* out, int n_out) {
  sfm::Plan p;
  if (int e = sfm::make_plan(desc, sfm::Entry{grad != 0, loss != 0}, sfm::Outputs::Unchecked, 1.f, p)) return e;
  if (!out || n_out < 1 + 4 * desc->n_scales) return sfm::fail(SFM_ERR_NULL, "sfm_loss_plan_info: out needs 1 + 4 * n_scales ints");
  out[0] = p.args.items;
  for (int s = 0; s < desc->n_scales; ++s) {
    const sfm::ScaleArgs& S = p.args.sc[s];
    int* o = out + 1 + 4 * s;
    o[0] = S.strips; o[1] = S.chunks; o[2] = S.chunk_rows; o[3] = S.tiles;
  }
  if (n_out >= 1 + 4 * desc->n_scales + 2) {      // the kernel family of the main launch and its resident waves per SIMD
    out[1 + 4 * desc->n_scales] = (int)p.v.family;
    out[2 + 4 * desc->n_scales] = sfm::waves_per_simd(p.v);
  }
  return SFM_OK;
}

int sfm_loss_variant(int variant) {
  if (variant != 0 && (variant < sfm::HOOK_STRUCT_HEADER || variant > sfm::HOOK_TWO_SOURCES))
    return sfm::fail(SFM_ERR_CONFIG, "sfm_loss_variant: %d is not 0, 3, 4 or 5", variant);
  sfm::g_hooks.variant = variant;
  return SFM_OK;
}

int sfm_loss_debug_trace(void* buf) {
  sfm::g_hooks.trace = (unsigned long long*)buf;
  return SFM_OK;
}

int sfm_loss_profile_events(void* ev_start, void* ev_stop) {
  sfm::g_hooks.ev_start = (hipEvent_t)ev_start;
  sfm::g_hooks.ev_stop = (hipEvent_t)ev_stop;
  return SFM_OK;
}

int sfm_loss_fwd(const SfmLossDesc* desc, float* loss5, void* ws, size_t ws_bytes, void* stream) {
  return sfm::run(desc, sfm::ENTRY_FWD, 1.f, loss5, ws, ws_bytes, stream, "sfm_loss_fwd", nullptr);
}

int sfm_loss_bwd(const SfmLossDesc* desc, float gy, void* ws, size_t ws_bytes, void* stream) {
  return sfm::run(desc, sfm::ENTRY_BWD, gy, nullptr, ws, ws_bytes, stream, "sfm_loss_bwd", nullptr);
}

int sfm_loss_fwd_bwd(const SfmLossDesc* desc, float* loss5, void* ws, size_t ws_bytes, void* stream) {
  return sfm::run(desc, sfm::ENTRY_FWD_BWD, 1.f, loss5, ws, ws_bytes, stream, "sfm_loss_fwd_bwd", nullptr);
}

int sfm_loss_proj_bwd(const SfmLossDesc* desc, int loss, const void* ws, size_t ws_bytes, float* d_proj, float* d_intrinsics,
                      void* stream) {
  const char* who = "sfm_loss_proj_bwd";
  if (!desc) return sfm::fail(SFM_ERR_NULL, "%s: NULL descriptor", who);
  if (desc->B == 0) {      // empty shard: nothing to launch (input pointers of empty arrays may be NULL, as for sfm_loss_bwd)
    if (!d_proj && !d_intrinsics) return sfm::fail(SFM_ERR_NULL, "%s: d_proj and d_intrinsics are both NULL", who);
    return SFM_OK;
  }
  // the plan of the gradient call whose sums lie in `ws` (found in the thread's plan cache when that call has just been made):
  // the library's own choice of kernel, no one-call hook
  sfm::Plan p;
  if (int err = sfm::cached_plan(desc, loss ? sfm::ENTRY_FWD_BWD : sfm::ENTRY_BWD, 1.f, p, -1)) return err;
  if (!d_proj && !d_intrinsics) return sfm::fail(SFM_ERR_NULL, "%s: d_proj and d_intrinsics are both NULL", who);
  if (!ws || ws_bytes < p.total) return sfm::fail(SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, p.total, ws_bytes);
  if (((uintptr_t)ws & 255) != 0) return sfm::fail(SFM_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
  sfm::ProjBwdArgs A = {};
  A.part_gpm = (const float*)((const char*)ws + p.off_gpm);
  A.intrinsics = desc->intrinsics;
  for (int i = 0; i < desc->n_src; ++i) A.pose[i] = desc->pose[i];
  A.d_proj = d_proj;
  A.d_intr = d_intrinsics;
  A.B = desc->B; A.n_src = desc->n_src; A.n_scales = desc->n_scales;
  for (int s = 0; s < SFM_MAX_SCALES; ++s) { A.tiles_of[s] = p.args.tiles_of[s]; A.item_begin_of[s] = p.args.item_begin_of[s]; }
  hipLaunchKernelGGL(sfm::proj_bwd_kernel, dim3(desc->B * desc->n_scales), dim3(64 * desc->n_src), 0, (hipStream_t)stream, A);
  return sfm::check_launch(who);
}

// One step of SFMLearner.__call__ from the full-resolution frames (models/base_model.py:48-124) in ONE call: the loop head :69-72 --
// both pyramids, pixel-interleaved, into the buffers the descriptor binds as tgt[] / src[] -- then the fused loss.
static int step_from_frames(const float* tgt_full, const float* src_full, const SfmLossDesc* d, bool grad, float* loss5, void* ws,
                            size_t ws_bytes, void* stream, const char* who) {
  if (!d) return sfm::fail(SFM_ERR_NULL, "%s: NULL descriptor", who);
  if (d->image_layout != SFM_LAYOUT_HWC)
    return sfm::fail(SFM_ERR_CONFIG, "%s: the descriptor must bind pixel-interleaved pyramid buffers (SFM_LAYOUT_HWC): they are what this call writes", who);
  if (d->n_scales < 1 || d->n_scales > SFM_MAX_SCALES) return sfm::fail(SFM_ERR_SHAPE, "%s: n_scales=%d", who, d->n_scales);
  for (int s = 1; s < d->n_scales; ++s)
    if (d->H[s] != d->H[0] >> s || d->W[s] != d->W[0] >> s)
      return sfm::fail(SFM_ERR_SHAPE, "%s: scale %d is %dx%d, the pyramid of a %dx%d frame has %dx%d there (base_model.py:70)", who, s, d->H[s],
                       d->W[s], d->H[0], d->W[0], d->H[0] >> s, d->W[0] >> s);
  // (the descriptor's pyramid pointers are inputs of the loss and outputs of this call: the caller owns the buffers either way.
  //  sfm::run writes the pyramids -- sfm_pyramid_pair_hwc_fwd -- once it has accepted the descriptor, loss5 and the workspace)
  const sfm::Frames frames = {tgt_full, src_full};
  const int rc = sfm::run(d, grad ? sfm::ENTRY_FWD_BWD : sfm::ENTRY_FWD, 1.f, loss5, ws, ws_bytes, stream, who, &frames);
  if (rc < 0) sfm_pyramid_variant(0);      // a rejected step has consumed the one-call pyramid hook too, like a rejected pyramid call
  return rc;
}

int sfm_step_fwd(const float* tgt_full, const float* src_full, const SfmLossDesc* desc, float* loss5, void* ws, size_t ws_bytes, void* stream) {
  return step_from_frames(tgt_full, src_full, desc, false, loss5, ws, ws_bytes, stream, "sfm_step_fwd");
}

int sfm_step_fwd_bwd(const float* tgt_full, const float* src_full, const SfmLossDesc* desc, float* loss5, void* ws, size_t ws_bytes,
                     void* stream) {
  return step_from_frames(tgt_full, src_full, desc, true, loss5, ws, ws_bytes, stream, "sfm_step_fwd_bwd");
}

}  // extern "C"
