// The masked means of SC-SfMLearner's compute_pairwise_loss (include/sfmwarp_pairwise.h): per (scale, source) the mean of
// err * (1 - diff) and of diff over the pixels that are in view and pass the auto-mask -- every scale and source of a step in TWO
// launches forward (the pixels, then a fold of one wavefront per (scale, source)) and ONE backward.  No atomics: every partial sum is
// written once by one lane and added in a fixed order in fp64, so two calls agree bit for bit.  gfx950 only.
//
// The grid is that of sfm_min_reproj.hip: one block per (scale, sample, run of PW_BLOCK_PIXELS consecutive pixels of that sample's
// flattened map), block index -> (s, b, run) through per-scale prefix counts; one pixel per lane, which loops over the sources.
// No address is formed from data: every index comes from the block, the lane and the descriptor's sizes.
#include "sfm_common.h"
#include "sfm_warp_pixel.h"
#include "../../include/sfmwarp_pairwise.h"

namespace sfm {

// the run length (tests/test_sc_pairwise_cpu.py and tests/test_sc_pairwise_gpu.py read this line)
constexpr int PW_BLOCK_PIXELS = 256;
constexpr int PW_BLOCK = PW_BLOCK_PIXELS;      // one pixel per lane
constexpr int PW_WAVES = PW_BLOCK / 64;
constexpr int PW_FOLD_WAVES = 16;              // the fold: one block, each wave takes the (scale, source) pairs w, w + 16, ...
constexpr int PW_MAX_PAIRS = SFM_MAX_SCALES * SFM_MAX_SRC;

struct PairwiseArgs {
  const float* err[SFM_MAX_SCALES];
  const float* diff[SFM_MAX_SCALES];
  const float* valid[SFM_MAX_SCALES];     // entries may be NULL
  const float* ident[SFM_MAX_SCALES];     // all NULL or all bound
  const float* cmp[SFM_MAX_SCALES];       // all NULL or all bound
  int8_t* keep[SFM_MAX_SCALES];
  float* g_err[SFM_MAX_SCALES];           // bwd
  float* g_diff[SFM_MAX_SCALES];          // bwd: all NULL or all bound
  float* loss;                            // fwd (fold)
  int* count;                             // fwd (fold) writes, bwd reads
  const float* g_loss;                    // bwd
  double* part_sp;                        // fwd: [block * n_src + i] the block's sum of err * (1 - diff) over its kept pixels of source i
  double* part_sg;                        // fwd: [block * n_src + i] ... of diff
  int* part_cnt;                          // fwd: [block * n_src + i] the block's kept pixels of source i
  float weight[SFM_MAX_SCALES];
  int H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];
  int nrun[SFM_MAX_SCALES];               // runs of one sample's map at scale s
  int begin[SFM_MAX_SCALES + 1];          // prefix sums of B * nrun[s]: the first block of scale s
  int B, n_src, n_scales, detach_weight, min_count_photo, min_count_geom;
};

struct PairwiseBlock {   // where a block works: scale, sample, run -- uniform over the block
  int s, b, run;
};

__device__ __forceinline__ PairwiseBlock pairwise_block(const PairwiseArgs& A) {
  PairwiseBlock w;
  const int bid = blockIdx.x;
  w.s = scale_of<0>(bid, A.begin, A.n_scales);
  const int r = bid - A.begin[w.s];
  w.b = r / A.nrun[w.s];
  w.run = r - w.b * A.nrun[w.s];
  return w;
}

__device__ __forceinline__ int wave_sum_int(int v) {   // the butterfly of wave_sum_d: the same value in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(PW_BLOCK) pairwise_fwd_kernel(const PairwiseArgs A) {
#pragma clang fp contract(off)
  __shared__ double red_sp[SFM_MAX_SRC][PW_WAVES], red_sg[SFM_MAX_SRC][PW_WAVES];
  __shared__ int red_cnt[SFM_MAX_SRC][PW_WAVES];
  const PairwiseBlock w = pairwise_block(A);
  const int P = A.H[w.s] * A.W[w.s];
  const int p = w.run * PW_BLOCK_PIXELS + (int)threadIdx.x;
  const bool have = p < P;                       // no early exit: the lanes of a wave add up their sums below
  const unsigned pc = (unsigned)(have ? p : 0);  // a lane past the end loads pixel 0 and drops it
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t base = (size_t)w.b * A.n_src * P;
  const float* err = A.err[w.s] + base;
  const float* diff = A.diff[w.s] + base;
  const float* valid = A.valid[w.s] ? A.valid[w.s] + base : nullptr;
  const float* ident = A.ident[w.s] ? A.ident[w.s] + base : nullptr;
  const float* cmp = A.cmp[w.s] ? A.cmp[w.s] + base : nullptr;
  int8_t* keep = A.keep[w.s] + base;
  for (int i = 0; i < A.n_src; ++i) {
    const size_t plane = (size_t)i * P;
    const float e = ldf(err + plane, pc), d = ldf(diff + plane, pc);
    bool k = have;
    if (valid) k = k && ldf(valid + plane, pc) > 0.f;
    if (ident) {
      const float c = cmp ? ldf(cmp + plane, pc) : e;
      k = k && c < ldf(ident + plane, pc);       // strict: a tie and a NaN on either side drop the pixel
    }
    if (have) keep[plane + p] = (int8_t)(k ? 1 : 0);
    const float t = e * (1.0f - d);
    const double sp = wave_sum_d(k ? (double)t : 0.0);      // selection, not a product with 0: a dropped NaN stays out
    const double sg = wave_sum_d(k ? (double)d : 0.0);
    const int cnt = wave_sum_int(k ? 1 : 0);
    if (lane == 0) red_sp[i][wave] = sp, red_sg[i][wave] = sg, red_cnt[i][wave] = cnt;
  }
  __syncthreads();
  if ((int)threadIdx.x < A.n_src) {              // one thread per source: the waves in ascending order
    const int i = threadIdx.x;
    double tp = red_sp[i][0], tg = red_sg[i][0];
    int tc = red_cnt[i][0];
#pragma unroll
    for (int v = 1; v < PW_WAVES; ++v) tp += red_sp[i][v], tg += red_sg[i][v], tc += red_cnt[i][v];
    const size_t at = (size_t)blockIdx.x * A.n_src + i;
    A.part_sp[at] = tp;
    A.part_sg[at] = tg;
    A.part_cnt[at] = tc;
  }
}

// one wave per (scale, source), PW_FOLD_WAVES at a time: lane l adds the partials l, l + 64, ... of its pair in ascending order in
// fp64, the 64 lanes are combined by the butterfly; then thread 0 adds the sources and the weighted scales in ascending order
__global__ void __launch_bounds__(64 * PW_FOLD_WAVES) pairwise_fold_kernel(const PairwiseArgs A) {
#pragma clang fp contract(off)
  __shared__ double qp[PW_MAX_PAIRS], qg[PW_MAX_PAIRS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_pairs = A.n_scales * A.n_src;
  for (int j = wave; j < n_pairs; j += PW_FOLD_WAVES) {      // (uniform over the wave)
    const int s = j / A.n_src, i = j - s * A.n_src;
    const int first = A.begin[s], n = A.begin[s + 1] - first;
    double sp = 0.0, sg = 0.0;
    int cnt = 0;
    for (int k = lane; k < n; k += 64) {
      const size_t at = (size_t)(first + k) * A.n_src + i;
      sp += A.part_sp[at], sg += A.part_sg[at], cnt += A.part_cnt[at];
    }
    sp = wave_sum_d(sp);
    sg = wave_sum_d(sg);
    cnt = wave_sum_int(cnt);
    if (lane == 0) {
      const double denom = (double)max(cnt, 1);
      const double mp = cnt > A.min_count_photo ? sp / denom : 0.0;
      const double mg = cnt > A.min_count_geom ? sg / denom : 0.0;
      A.loss[j] = (float)mp;
      A.loss[n_pairs + j] = (float)mg;
      A.count[j] = cnt;
      qp[j] = mp, qg[j] = mg;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tp = 0.0, tg = 0.0;
    for (int s = 0; s < A.n_scales; ++s) {
      double ip = qp[s * A.n_src], ig = qg[s * A.n_src];
      for (int i = 1; i < A.n_src; ++i) ip += qp[s * A.n_src + i], ig += qg[s * A.n_src + i];
      const double wp = (double)A.weight[s] * ip, wg = (double)A.weight[s] * ig;
      tp = s ? tp + wp : wp;
      tg = s ? tg + wg : wg;
    }
    A.loss[2 * n_pairs] = (float)tp;
    A.loss[2 * n_pairs + 1] = (float)tg;
  }
}

__global__ void __launch_bounds__(PW_BLOCK) pairwise_bwd_kernel(const PairwiseArgs A) {
#pragma clang fp contract(off)
  __shared__ float cps[SFM_MAX_SRC], cgs[SFM_MAX_SRC];
  const PairwiseBlock w = pairwise_block(A);
  const int n_pairs = A.n_scales * A.n_src;
  if ((int)threadIdx.x < A.n_src) {              // once per block and source: correctly rounded quotients of doubles, rounded to fp32
    const int j = w.s * A.n_src + (int)threadIdx.x;
    const int cnt = A.count[j];
    const double denom = (double)max(cnt, 1), wt = (double)A.weight[w.s];
    cps[threadIdx.x] = cnt > A.min_count_photo ? (float)(((double)A.g_loss[j] + wt * (double)A.g_loss[2 * n_pairs]) / denom) : 0.f;
    cgs[threadIdx.x] = cnt > A.min_count_geom ? (float)(((double)A.g_loss[n_pairs + j] + wt * (double)A.g_loss[2 * n_pairs + 1]) / denom) : 0.f;
  }
  __syncthreads();
  const int P = A.H[w.s] * A.W[w.s];
  const int p = w.run * PW_BLOCK_PIXELS + (int)threadIdx.x;
  if (p >= P) return;
  const size_t base = (size_t)w.b * A.n_src * P;
  const float* err = A.err[w.s] + base;
  const float* diff = A.diff[w.s] + base;
  const int8_t* keep = A.keep[w.s] + base;
  float* g_err = A.g_err[w.s] + base;
  float* g_diff = A.g_diff[w.s] ? A.g_diff[w.s] + base : nullptr;
  for (int i = 0; i < A.n_src; ++i) {
    const size_t plane = (size_t)i * P;
    const bool k = keep[plane + p] != 0;
    const float e = ldf(err + plane, (unsigned)p), d = ldf(diff + plane, (unsigned)p);
    const float cp = cps[i], cg = cgs[i];
    const float ge = (1.0f - d) * cp;
    stf(g_err + plane, (unsigned)p, k ? ge : 0.f);
    if (g_diff) {
      const float gd = A.detach_weight ? cg : cg - e * cp;
      stf(g_diff + plane, (unsigned)p, k ? gd : 0.f);
    }
  }
}

// What every call checks and fills in, in the order the header states.  stage: 0 = the workspace query (no pointer is looked at),
// 1 = the pointers of the forward, 2 = those of the backward.
static int pairwise_setup(PairwiseArgs& A, const char* who, const SfmPairwiseDesc* d, const int stage) {
  SFM_REQUIRE(d, SFM_ERR_NULL, "%s: NULL descriptor", who);
  const auto runs = [&A](const int s, const int H, const int W) { return (long long)(A.nrun[s] = (H * W + PW_BLOCK_PIXELS - 1) / PW_BLOCK_PIXELS); };
  if (int e = check_pyramid_shape(who, d->B, d->n_src, "n_src", d->n_scales, d->H, d->W, "runs of pixels", "", runs, A.H, A.W, A.begin))
    return e;
  for (int s = 0; s < d->n_scales; ++s)
    SFM_REQUIRE((long long)d->B * d->H[s] * d->W[s] < (1ll << 31), SFM_ERR_SHAPE, "%s: scale %d: B*H*W too large for an int32 count", who, s);
  A.B = d->B, A.n_src = d->n_src, A.n_scales = d->n_scales;
  SFM_REQUIRE(d->detach_weight == 0 || d->detach_weight == 1, SFM_ERR_CONFIG, "%s: detach_weight=%d, need 0 or 1", who, d->detach_weight);
  SFM_REQUIRE(d->min_count_photo >= 0, SFM_ERR_CONFIG, "%s: min_count_photo=%d, need >= 0", who, d->min_count_photo);
  SFM_REQUIRE(d->min_count_geom >= 0, SFM_ERR_CONFIG, "%s: min_count_geom=%d, need >= 0", who, d->min_count_geom);
  A.detach_weight = d->detach_weight, A.min_count_photo = d->min_count_photo, A.min_count_geom = d->min_count_geom;
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->weight[s] >= 0.f, SFM_ERR_CONFIG, "%s: weight[%d]=%g, need weight >= 0", who, s, (double)d->weight[s]);
    A.weight[s] = d->weight[s];
  }
  if (d->B == 0 || stage == 0) return SFM_OK;   // empty batch: nothing to do, pointers may be NULL
  int n_ident = 0, n_cmp = 0, n_g_diff = 0;
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->err[s], SFM_ERR_NULL, "%s: err[%d] is NULL", who, s);
    SFM_REQUIRE(d->diff[s], SFM_ERR_NULL, "%s: diff[%d] is NULL", who, s);
    SFM_REQUIRE(d->keep[s], SFM_ERR_NULL, "%s: keep[%d] is NULL", who, s);
    if (stage == 2) SFM_REQUIRE(d->g_err[s], SFM_ERR_NULL, "%s: g_err[%d] is NULL", who, s);
    A.err[s] = d->err[s], A.diff[s] = d->diff[s], A.keep[s] = d->keep[s];
    if (stage == 1) {
      A.valid[s] = d->valid[s], A.ident[s] = d->ident[s], A.cmp[s] = d->cmp[s];
      n_ident += d->ident[s] != nullptr, n_cmp += d->cmp[s] != nullptr;
    } else {
      A.g_err[s] = d->g_err[s], A.g_diff[s] = d->g_diff[s];
      n_g_diff += d->g_diff[s] != nullptr;
    }
  }
  if (stage == 1) SFM_REQUIRE(d->loss, SFM_ERR_NULL, "%s: loss is NULL", who);
  SFM_REQUIRE(d->count, SFM_ERR_NULL, "%s: count is NULL", who);
  if (stage == 2) SFM_REQUIRE(d->g_loss, SFM_ERR_NULL, "%s: g_loss is NULL", who);
  A.loss = d->loss, A.count = d->count, A.g_loss = d->g_loss;
  SFM_REQUIRE(n_ident == 0 || n_ident == d->n_scales, SFM_ERR_NULL, "%s: ident is bound for %d of %d scales, need all or none", who, n_ident, d->n_scales);
  SFM_REQUIRE(n_cmp == 0 || n_cmp == d->n_scales, SFM_ERR_NULL, "%s: cmp is bound for %d of %d scales, need all or none", who, n_cmp, d->n_scales);
  SFM_REQUIRE(n_g_diff == 0 || n_g_diff == d->n_scales, SFM_ERR_NULL, "%s: g_diff is bound for %d of %d scales, need all or none", who, n_g_diff,
              d->n_scales);
  return SFM_OK;
}

// per (run, source) 8 bytes of Sp, 8 of Sg and 4 of count: the doubles first, so that all three arrays are aligned
static size_t pairwise_ws_bytes(const PairwiseArgs& A) {
  const size_t need = (size_t)A.begin[A.n_scales] * A.n_src * (2 * sizeof(double) + sizeof(int));
  return need ? (need + 255) / 256 * 256 : 256;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_pairwise_workspace_bytes(const SfmPairwiseDesc* d) {
  PairwiseArgs A = {};
  if (pairwise_setup(A, "sfm_pairwise_workspace_bytes", d, 0)) return 0;
  return pairwise_ws_bytes(A);
}

int sfm_pairwise_fwd(const SfmPairwiseDesc* d, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "sfm_pairwise_fwd";
  PairwiseArgs A = {};
  if (int e = pairwise_setup(A, who, d, 1)) return e;
  if (d->B == 0) return SFM_OK;
  const size_t need = pairwise_ws_bytes(A);
  SFM_REQUIRE(ws && ws_bytes >= need, SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, need, ws ? ws_bytes : (size_t)0);
  SFM_REQUIRE(((uintptr_t)ws & 255) == 0, SFM_ERR_WORKSPACE, "%s: workspace must be aligned to 256 bytes", who);
  const size_t n_part = (size_t)A.begin[A.n_scales] * A.n_src;
  A.part_sp = (double*)ws;
  A.part_sg = A.part_sp + n_part;
  A.part_cnt = (int*)(A.part_sg + n_part);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pairwise_fwd_kernel, dim3(A.begin[A.n_scales]), dim3(PW_BLOCK), 0, st, A);
  hipLaunchKernelGGL(pairwise_fold_kernel, dim3(1), dim3(64 * PW_FOLD_WAVES), 0, st, A);
  return check_launch(who);
}

int sfm_pairwise_bwd(const SfmPairwiseDesc* d, void* stream) {
  const char* who = "sfm_pairwise_bwd";
  PairwiseArgs A = {};
  if (int e = pairwise_setup(A, who, d, 2)) return e;
  if (d->B == 0) return SFM_OK;
  hipLaunchKernelGGL(pairwise_bwd_kernel, dim3(A.begin[A.n_scales]), dim3(PW_BLOCK), 0, (hipStream_t)stream, A);
  return check_launch(who);
}

}  // extern "C"
