// The last stage of a Monodepth2-style loss on the library's warp (include/sfmwarp_min_reproj.h): per pixel the minimum of the error
// maps over the sources, the auto-mask against the unwarped sources, and the mean -- every scale of a step in TWO launches forward
// (the pixels, then a fold of one wavefront per scale) and ONE backward.  No atomics: every partial sum is written once by one
// lane and added in a fixed order in fp64, so two calls agree bit for bit.  gfx950 only.
//
// One grid covers every (scale, sample, run of MR_BLOCK_PIXELS consecutive pixels of that sample's flattened map): block index ->
// (s, b, run) through per-scale prefix counts, as in sfm_warp_pyramid.hip.  One pixel per lane, coalesced dword loads: the maps
// are single-channel and each is read once, there is nothing to keep in registers or LDS but the block's four wave sums.
#include "sfm_common.h"
#include "sfm_warp_pixel.h"
#include "../../include/sfmwarp_min_reproj.h"

namespace sfm {

// the run length (tests/test_min_reproj_cpu.py and tests/test_min_reproj_gpu.py read this line)
constexpr int MR_BLOCK_PIXELS = 256;
constexpr int MR_BLOCK = MR_BLOCK_PIXELS;      // one pixel per lane
constexpr int MR_WAVES = MR_BLOCK / 64;

struct MinReprojArgs {
  const float* err[SFM_MAX_SCALES];
  const float* valid[SFM_MAX_SCALES];     // entries may be NULL
  const float* ident[SFM_MAX_SCALES];     // read iff n_ident > 0
  int8_t* winner[SFM_MAX_SCALES];
  float* g_err[SFM_MAX_SCALES];           // bwd
  float* loss;                            // fwd (fold)
  int* count;                             // fwd (fold) writes, bwd reads
  const float* g_loss;                    // bwd
  double* part_sum;                       // fwd: [block] the block's sum of `best` over its kept pixels
  int* part_cnt;                          // fwd: [block] the block's kept pixels
  float weight[SFM_MAX_SCALES];
  int H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];
  int nrun[SFM_MAX_SCALES];               // runs of one sample's map at scale s
  int begin[SFM_MAX_SCALES + 1];          // prefix sums of B * nrun[s]: the first block of scale s
  int B, n_err, n_ident, n_scales, norm;
};

// where a block works: scale, sample, run -- uniform over the block
struct MinReprojBlock {
  int s, b, run;
};

__device__ __forceinline__ MinReprojBlock min_reproj_block(const MinReprojArgs& A) {
  MinReprojBlock w;
  const int bid = blockIdx.x;
  w.s = scale_of<0>(bid, A.begin, A.n_scales);
  const int r = bid - A.begin[w.s];
  w.b = r / A.nrun[w.s];
  w.run = r - w.b * A.nrun[w.s];
  return w;
}

__device__ __forceinline__ int wave_sum_i(int v) {   // the butterfly of wave_sum_d: the same value in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// denom[s] of the header, from the count the fold wrote
__device__ __forceinline__ double min_reproj_denom(const MinReprojArgs& A, const int s, const int count) {
  return A.norm == SFM_MIN_REPROJ_NORM_KEPT ? (double)max(count, 1) : (double)A.B * (double)(A.H[s] * A.W[s]);
}

__global__ void __launch_bounds__(MR_BLOCK) min_reproj_fwd_kernel(const MinReprojArgs A) {
  __shared__ double red_sum[MR_WAVES];
  __shared__ int red_cnt[MR_WAVES];
  const MinReprojBlock w = min_reproj_block(A);
  const int P = A.H[w.s] * A.W[w.s];
  const int p = w.run * MR_BLOCK_PIXELS + (int)threadIdx.x;
  const bool have = p < P;                       // no early exit: the lanes of a wave add up their sums below
  const unsigned pc = (unsigned)(have ? p : 0);  // a lane past the end loads pixel 0 and drops it
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float inf = __builtin_inff();
  float best = inf;
  int win = -1;
  const float* err = A.err[w.s] + (size_t)w.b * A.n_err * P;
  const float* valid = A.valid[w.s] ? A.valid[w.s] + (size_t)w.b * A.n_err * P : nullptr;
  for (int i = 0; i < A.n_err; ++i) {
    const float e = ldf(err + (size_t)i * P, pc);
    const bool ok = valid ? ldf(valid + (size_t)i * P, pc) > 0.f : true;
    if (ok && e < best) best = e, win = i;       // strict: the first index wins a tie, NaN and +inf never win
  }
  bool keep = have && win >= 0;
  if (A.n_ident > 0) {
    const float* ident = A.ident[w.s] + (size_t)w.b * A.n_ident * P;
    float floor = inf;
    for (int j = 0; j < A.n_ident; ++j) {
      const float e = ldf(ident + (size_t)j * P, pc);
      if (e < floor) floor = e;
    }
    keep = keep && best < floor;                 // strict: a pixel the unwarped source explains as well is dropped
  }
  if (have) A.winner[w.s][(size_t)w.b * P + p] = (int8_t)(keep ? win : -1);
  const double sum = wave_sum_d(keep ? (double)best : 0.0);
  const int cnt = wave_sum_i(keep ? 1 : 0);
  if (lane == 0) red_sum[wave] = sum, red_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {                        // the waves in ascending order
    double ts = red_sum[0];
    int tc = red_cnt[0];
#pragma unroll
    for (int v = 1; v < MR_WAVES; ++v) ts += red_sum[v], tc += red_cnt[v];
    A.part_sum[blockIdx.x] = ts;
    A.part_cnt[blockIdx.x] = tc;
  }
}

// one wave per scale: lane l adds the block partials l, l + 64, ... of its scale in ascending order in fp64, the 64 lanes are
// combined by the butterfly; then thread 0 adds the weighted scales in ascending order
__global__ void __launch_bounds__(64 * SFM_MAX_SCALES) min_reproj_fold_kernel(const MinReprojArgs A) {
#pragma clang fp contract(off)
  __shared__ double term[SFM_MAX_SCALES];
  const int s = threadIdx.x >> 6, lane = threadIdx.x & 63;      // (the launch has 64 * n_scales threads)
  const int first = A.begin[s], n = A.begin[s + 1] - first;
  double acc = 0.0;
  int cnt = 0;
  for (int k = lane; k < n; k += 64) acc += A.part_sum[first + k], cnt += A.part_cnt[first + k];
  acc = wave_sum_d(acc);
  cnt = wave_sum_i(cnt);
  if (lane == 0) {
    const double denom = min_reproj_denom(A, s, cnt);
    A.loss[s] = (float)(acc / denom);
    A.count[s] = cnt;
    term[s] = (double)A.weight[s] * acc / denom;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = term[0];
    for (int k = 1; k < A.n_scales; ++k) total += term[k];
    A.loss[A.n_scales] = (float)total;
  }
}

__global__ void __launch_bounds__(MR_BLOCK) min_reproj_bwd_kernel(const MinReprojArgs A) {
#pragma clang fp contract(off)
  __shared__ float cs;
  const MinReprojBlock w = min_reproj_block(A);
  if (threadIdx.x == 0)                          // once per block: one correctly rounded quotient of doubles, rounded to fp32
    cs = (float)(((double)A.g_loss[w.s] + (double)A.weight[w.s] * (double)A.g_loss[A.n_scales]) / min_reproj_denom(A, w.s, A.count[w.s]));
  __syncthreads();
  const int P = A.H[w.s] * A.W[w.s];
  const int p = w.run * MR_BLOCK_PIXELS + (int)threadIdx.x;
  if (p >= P) return;
  const float c = cs;
  const int win = A.winner[w.s][(size_t)w.b * P + p];
  float* g = A.g_err[w.s] + (size_t)w.b * A.n_err * P;
  for (int i = 0; i < A.n_err; ++i) stf(g + (size_t)i * P, (unsigned)p, win == i ? c : 0.f);
}

// What every call checks and fills in, in the order the header states.  stage: 0 = the workspace query (no pointer is looked at),
// 1 = the pointers of the forward, 2 = those of the backward.
static int min_reproj_setup(MinReprojArgs& A, const char* who, const SfmMinReprojDesc* d, const int stage) {
  SFM_REQUIRE(d, SFM_ERR_NULL, "%s: NULL descriptor", who);
  const auto runs = [&A](const int s, const int H, const int W) { return (long long)(A.nrun[s] = (H * W + MR_BLOCK_PIXELS - 1) / MR_BLOCK_PIXELS); };
  if (int e = check_pyramid_shape(who, d->B, d->n_err, "n_err", d->n_scales, d->H, d->W, "runs of pixels", "", runs, A.H, A.W, A.begin))
    return e;
  SFM_REQUIRE(d->n_ident >= 0 && d->n_ident <= SFM_MAX_SRC, SFM_ERR_SHAPE, "%s: n_ident=%d, need 0..%d", who, d->n_ident, SFM_MAX_SRC);
  for (int s = 0; s < d->n_scales; ++s)
    SFM_REQUIRE((long long)d->B * d->H[s] * d->W[s] < (1ll << 31), SFM_ERR_SHAPE, "%s: scale %d: B*H*W too large for an int32 count", who, s);
  A.B = d->B, A.n_err = d->n_err, A.n_ident = d->n_ident, A.n_scales = d->n_scales, A.norm = d->norm;
  SFM_REQUIRE(d->norm == SFM_MIN_REPROJ_NORM_KEPT || d->norm == SFM_MIN_REPROJ_NORM_ALL, SFM_ERR_CONFIG, "%s: norm=%d", who, d->norm);
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->weight[s] >= 0.f, SFM_ERR_CONFIG, "%s: weight[%d]=%g, need weight >= 0", who, s, (double)d->weight[s]);
    A.weight[s] = d->weight[s];
  }
  if (d->B == 0 || stage == 0) return SFM_OK;   // empty batch: nothing to do, pointers may be NULL
  for (int s = 0; s < d->n_scales; ++s) {
    if (stage == 1) {
      SFM_REQUIRE(d->err[s], SFM_ERR_NULL, "%s: err[%d] is NULL", who, s);
      if (d->n_ident > 0) SFM_REQUIRE(d->ident[s], SFM_ERR_NULL, "%s: ident[%d] is NULL", who, s);
    }
    SFM_REQUIRE(d->winner[s], SFM_ERR_NULL, "%s: winner[%d] is NULL", who, s);
    if (stage == 2) SFM_REQUIRE(d->g_err[s], SFM_ERR_NULL, "%s: g_err[%d] is NULL", who, s);
    A.err[s] = d->err[s], A.valid[s] = d->valid[s], A.ident[s] = d->ident[s], A.winner[s] = d->winner[s], A.g_err[s] = d->g_err[s];
  }
  if (stage == 1) SFM_REQUIRE(d->loss, SFM_ERR_NULL, "%s: loss is NULL", who);
  SFM_REQUIRE(d->count, SFM_ERR_NULL, "%s: count is NULL", who);
  if (stage == 2) SFM_REQUIRE(d->g_loss, SFM_ERR_NULL, "%s: g_loss is NULL", who);
  A.loss = d->loss, A.count = d->count, A.g_loss = d->g_loss;
  return SFM_OK;
}

// 8 bytes of sum and 4 of count per block: all the sums first, so that both arrays are aligned
static size_t min_reproj_ws_bytes(const MinReprojArgs& A) {
  const size_t need = (size_t)A.begin[A.n_scales] * (sizeof(double) + sizeof(int));
  return need ? (need + 255) / 256 * 256 : 256;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_min_reproj_workspace_bytes(const SfmMinReprojDesc* d) {
  MinReprojArgs A = {};
  if (min_reproj_setup(A, "sfm_min_reproj_workspace_bytes", d, 0)) return 0;
  return min_reproj_ws_bytes(A);
}

int sfm_min_reproj_fwd(const SfmMinReprojDesc* d, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "sfm_min_reproj_fwd";
  MinReprojArgs A = {};
  if (int e = min_reproj_setup(A, who, d, 1)) return e;
  if (d->B == 0) return SFM_OK;
  const size_t need = min_reproj_ws_bytes(A);
  SFM_REQUIRE(ws && ws_bytes >= need, SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, need, ws ? ws_bytes : (size_t)0);
  SFM_REQUIRE(((uintptr_t)ws & 255) == 0, SFM_ERR_WORKSPACE, "%s: workspace must be aligned to 256 bytes", who);
  A.part_sum = (double*)ws;
  A.part_cnt = (int*)(A.part_sum + A.begin[A.n_scales]);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(min_reproj_fwd_kernel, dim3(A.begin[A.n_scales]), dim3(MR_BLOCK), 0, st, A);
  hipLaunchKernelGGL(min_reproj_fold_kernel, dim3(1), dim3(64 * d->n_scales), 0, st, A);
  return check_launch(who);
}

int sfm_min_reproj_bwd(const SfmMinReprojDesc* d, void* stream) {
  const char* who = "sfm_min_reproj_bwd";
  MinReprojArgs A = {};
  if (int e = min_reproj_setup(A, who, d, 2)) return e;
  if (d->B == 0) return SFM_OK;
  hipLaunchKernelGGL(min_reproj_bwd_kernel, dim3(A.begin[A.n_scales]), dim3(MR_BLOCK), 0, (hipStream_t)stream, A);
  return check_launch(who);
}

}  // extern "C"
