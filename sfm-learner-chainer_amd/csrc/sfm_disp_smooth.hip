// The edge-aware smoothness of the (mean-normalised) disparity (include/sfmwarp_disp_smooth.h): every scale of a step in TWO
// launches forward (the pixels, then a fold of one block) and ONE backward.  |D(d/M)| = |Dd| / |M|, so ONE pass over d and I
// collects the three per-sample sums (sum d, X, Y) and the fold finishes the value: no normalised copy, no second pass.  No atomics:
// every partial is written once by one lane and added in a fixed order in fp64, so two calls agree bit for bit.  gfx950 only.
//
// One grid covers every (scale, sample, run of DS_BLOCK_PIXELS consecutive pixels of that sample's flattened map), as in
// sfm_min_reproj.hip.  One pixel per lane; the right and the lower neighbour come from loads of their own (cache hits: the same
// lines the neighbouring lanes and the next rows' blocks read).  A neighbour past the border is the pixel itself: then Dd = 0, the
// forward's term is |0| * w = 0 and the backward's sign(0) * w = 0, which is what "terms past the border equal 0" asks for.
#include "sfm_common.h"
#include "sfm_warp_pixel.h"
#include "../../include/sfmwarp_disp_smooth.h"

namespace sfm {

// the run length (tests/test_disp_smooth_cpu.py and tests/test_disp_smooth_gpu.py read this line)
constexpr int DS_BLOCK_PIXELS = 256;
constexpr int DS_BLOCK = DS_BLOCK_PIXELS;      // one pixel per lane
constexpr int DS_WAVES = DS_BLOCK / 64;
constexpr int DS_FOLD_WAVES = 16;              // the fold: one block, each wave finishes the samples wave, wave + 16, ... of every scale

struct DispSmoothArgs {
  const float* disp[SFM_MAX_SCALES];
  const float* img[SFM_MAX_SCALES];
  float* g_disp[SFM_MAX_SCALES];          // bwd
  float* loss;                            // fwd (fold)
  double* stats;                          // [s][b][M,X,Y]: fwd (fold) writes, bwd reads
  const float* g_loss;                    // bwd
  double* part;                           // fwd: [block][sum d, X, Y]
  float weight[SFM_MAX_SCALES];
  int H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];
  int nrun[SFM_MAX_SCALES];               // runs of one sample's map at scale s
  int begin[SFM_MAX_SCALES + 1];          // prefix sums of B * nrun[s]: the first block of scale s
  int B, n_scales, normalize, edge, accumulate;
};

// where a block works: scale, sample, run -- uniform over the block
struct DispSmoothBlock {
  int s, b, run;
};

__device__ __forceinline__ DispSmoothBlock disp_smooth_block(const DispSmoothArgs& A) {
  DispSmoothBlock w;
  const int bid = blockIdx.x;
  w.s = scale_of<0>(bid, A.begin, A.n_scales);
  const int r = bid - A.begin[w.s];
  w.b = r / A.nrun[w.s];
  w.run = r - w.b * A.nrun[w.s];
  return w;
}

// one pixel of one sample: the disparity and the three channels
struct DispSmoothPix {
  float d, i[3];
};

__device__ __forceinline__ DispSmoothPix disp_smooth_load(const float* d, const float* img, const int P, const unsigned p) {
  DispSmoothPix o;
  o.d = ldf(d, p);
#pragma unroll
  for (int c = 0; c < 3; ++c) o.i[c] = ldf(img + (size_t)c * P, p);
  return o;
}

// w of the header between two pixels: exp(-a / 3) = exp2(a KE), the mean over the channels folded into the constant
__device__ __forceinline__ float disp_smooth_weight(const DispSmoothPix& near, const DispSmoothPix& far, const int edge) {
#pragma clang fp contract(off)
  const float KE = -1.44269504088896341f / 3.0f;
  const float e0 = far.i[0] - near.i[0], e1 = far.i[1] - near.i[1], e2 = far.i[2] - near.i[2];
  const float a = edge == SFM_DISP_SMOOTH_EDGE_MEAN_ABS ? (fabsf(e0) + fabsf(e1)) + fabsf(e2) : fabsf((e0 + e1) + e2);
  return __builtin_amdgcn_exp2f(a * KE);
}

// sign(t) w with sign(0) = 0
__device__ __forceinline__ float disp_smooth_signed(const float w, const float t) { return (t != 0.f) ? __builtin_copysignf(w, t) : 0.f; }

__global__ void __launch_bounds__(DS_BLOCK) disp_smooth_fwd_kernel(const DispSmoothArgs A) {
#pragma clang fp contract(off)
  __shared__ double red[DS_WAVES][3];
  const DispSmoothBlock k = disp_smooth_block(A);
  const int w = A.W[k.s], P = A.H[k.s] * w;
  const int p = k.run * DS_BLOCK_PIXELS + (int)threadIdx.x;
  const bool have = p < P;                       // no early exit: the lanes of a wave add up their sums below
  const int pc = have ? p : 0;                   // a lane past the end works on pixel 0 and drops it
  const int y = pc / w, x = pc - y * w;
  const int pr = (have && x + 1 < w) ? pc + 1 : pc;    // past the border: the pixel itself (a zero term)
  const int pd = (have && pc + w < P) ? pc + w : pc;
  const float* d = A.disp[k.s] + (size_t)k.b * P;
  const float* img = A.img[k.s] + (size_t)k.b * 3 * P;
  const DispSmoothPix c = disp_smooth_load(d, img, P, (unsigned)pc);
  const DispSmoothPix r = disp_smooth_load(d, img, P, (unsigned)pr);
  const DispSmoothPix l = disp_smooth_load(d, img, P, (unsigned)pd);
  const float tx = fabsf(r.d - c.d) * disp_smooth_weight(c, r, A.edge);
  const float ty = fabsf(l.d - c.d) * disp_smooth_weight(c, l, A.edge);
  const double sd = wave_sum_d(have ? (double)c.d : 0.0);
  const double sx = wave_sum_d((double)tx);
  const double sy = wave_sum_d((double)ty);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) red[wave][0] = sd, red[wave][1] = sx, red[wave][2] = sy;
  __syncthreads();
  if (threadIdx.x < 3) {                         // the waves in ascending order
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int v = 1; v < DS_WAVES; ++v) t += red[v][threadIdx.x];
    A.part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
  }
}

// (c_x X + c_y Y) / |M| of one sample, from its stats
__device__ __forceinline__ double disp_smooth_term(const DispSmoothArgs& A, const int s, const double M, const double X, const double Y) {
  const double cx = 1.0 / ((double)A.B * A.H[s] * (A.W[s] - 1)), cy = 1.0 / ((double)A.B * (A.H[s] - 1) * A.W[s]);
  return (cx * X + cy * Y) / fabs(M);
}

// One block.  First every (scale, sample) is finished by one wave: lane l adds the partials l, l + 64, ... of the sample in
// ascending order in fp64, the 64 lanes are combined by the butterfly, lane 0 writes M, X, Y into stats.  Then wave s adds the
// samples of scale s in ascending order, and thread 0 the weighted scales.
__global__ void __launch_bounds__(64 * DS_FOLD_WAVES) disp_smooth_fold_kernel(const DispSmoothArgs A) {
#pragma clang fp contract(off)
  __shared__ double term[SFM_MAX_SCALES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int q = wave; q < A.n_scales * A.B; q += DS_FOLD_WAVES) {
    const int s = q / A.B, b = q - s * A.B;
    const int n = A.nrun[s];
    const double* part = A.part + ((size_t)A.begin[s] + (size_t)b * n) * 3;
    double sd = 0.0, sx = 0.0, sy = 0.0;
    for (int j = lane; j < n; j += 64) sd += part[3 * j], sx += part[3 * j + 1], sy += part[3 * j + 2];
    sd = wave_sum_d(sd), sx = wave_sum_d(sx), sy = wave_sum_d(sy);
    if (lane == 0) {
      double* st = A.stats + (size_t)q * 3;
      st[0] = A.normalize ? sd / (double)(A.H[s] * A.W[s]) + 1e-7 : 1.0;
      st[1] = sx;
      st[2] = sy;
    }
  }
  __syncthreads();                               // (the block's own writes to stats are visible to it behind the barrier)
  if (wave < A.n_scales) {
    const int s = wave;
    double acc = 0.0;
    for (int b0 = 0; b0 < A.B; b0 += 64) {       // 64 samples at a time: a term per lane, added by lane order
      const int b = b0 + lane;
      double t = 0.0;                            // (a lane past the batch adds +0, which changes nothing)
      if (b < A.B) {
        const double* st = A.stats + ((size_t)s * A.B + b) * 3;
        t = disp_smooth_term(A, s, st[0], st[1], st[2]);
      }
      for (int j = 0; j < 64; ++j) acc += __shfl(t, j, 64);
    }
    if (lane == 0) {
      A.loss[s] = (float)acc;
      term[s] = (double)A.weight[s] * acc;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = term[0];
    for (int j = 1; j < A.n_scales; ++j) total += term[j];
    A.loss[A.n_scales] = (float)total;
  }
}

__global__ void __launch_bounds__(DS_BLOCK) disp_smooth_bwd_kernel(const DispSmoothArgs A) {
#pragma clang fp contract(off)
  __shared__ float fac[3];
  const DispSmoothBlock k = disp_smooth_block(A);
  const int h = A.H[k.s], w = A.W[k.s], P = h * w;
  if (threadIdx.x == 0) {                        // once per block, in fp64, rounded to fp32
    const double* st = A.stats + ((size_t)k.s * A.B + k.b) * 3;
    const double M = st[0], X = st[1], Y = st[2];
    const double ks = (double)A.g_loss[k.s] + (double)A.weight[k.s] * (double)A.g_loss[A.n_scales];
    const double cx = 1.0 / ((double)A.B * h * (w - 1)), cy = 1.0 / ((double)A.B * (h - 1) * w);
    fac[0] = (float)(ks * cx / fabs(M));
    fac[1] = (float)(ks * cy / fabs(M));
    fac[2] = A.normalize ? (float)(ks * (cx * X + cy * Y) / (M * fabs(M) * (double)P)) : 0.f;
  }
  __syncthreads();
  const int p = k.run * DS_BLOCK_PIXELS + (int)threadIdx.x;
  if (p >= P) return;
  const int y = p / w, x = p - y * w;
  const float* d = A.disp[k.s] + (size_t)k.b * P;
  const float* img = A.img[k.s] + (size_t)k.b * 3 * P;
  // past the border: the pixel itself, a zero difference and so a zero term
  const DispSmoothPix c = disp_smooth_load(d, img, P, (unsigned)p);
  const DispSmoothPix r = disp_smooth_load(d, img, P, (unsigned)(x + 1 < w ? p + 1 : p));
  const DispSmoothPix l = disp_smooth_load(d, img, P, (unsigned)(x > 0 ? p - 1 : p));
  const DispSmoothPix dn = disp_smooth_load(d, img, P, (unsigned)(y + 1 < h ? p + w : p));
  const DispSmoothPix up = disp_smooth_load(d, img, P, (unsigned)(y > 0 ? p - w : p));
  const float tx = disp_smooth_signed(disp_smooth_weight(c, r, A.edge), r.d - c.d);      // t_x(y,x)
  const float txl = disp_smooth_signed(disp_smooth_weight(l, c, A.edge), c.d - l.d);     // t_x(y,x-1)
  const float ty = disp_smooth_signed(disp_smooth_weight(c, dn, A.edge), dn.d - c.d);    // t_y(y,x)
  const float tyu = disp_smooth_signed(disp_smooth_weight(up, c, A.edge), c.d - up.d);   // t_y(y-1,x)
  const float g = (fac[0] * (txl - tx) + fac[1] * (tyu - ty)) - fac[2];
  float* out = A.g_disp[k.s] + (size_t)k.b * P;
  stf(out, (unsigned)p, A.accumulate ? ldf(out, (unsigned)p) + g : g);
}

// What every call checks and fills in, in the order the header states.  stage: 0 = the workspace query (no pointer is looked at),
// 1 = the pointers of the forward, 2 = those of the backward.
static int disp_smooth_setup(DispSmoothArgs& A, const char* who, const SfmDispSmoothDesc* d, const int stage) {
  SFM_REQUIRE(d, SFM_ERR_NULL, "%s: NULL descriptor", who);
  const auto runs = [&A](const int s, const int H, const int W) { return (long long)(A.nrun[s] = (H * W + DS_BLOCK_PIXELS - 1) / DS_BLOCK_PIXELS); };
  if (int e = check_pyramid_shape(who, d->B, 1, "n_img", d->n_scales, d->H, d->W, "runs of pixels", "", runs, A.H, A.W, A.begin)) return e;
  A.B = d->B, A.n_scales = d->n_scales, A.normalize = d->normalize, A.edge = d->edge, A.accumulate = d->accumulate;
  SFM_REQUIRE(d->normalize == 0 || d->normalize == 1, SFM_ERR_CONFIG, "%s: normalize=%d, need 0 or 1", who, d->normalize);
  SFM_REQUIRE(d->edge == SFM_DISP_SMOOTH_EDGE_MEAN_ABS || d->edge == SFM_DISP_SMOOTH_EDGE_ABS_MEAN, SFM_ERR_CONFIG, "%s: edge=%d", who, d->edge);
  SFM_REQUIRE(d->accumulate == 0 || d->accumulate == 1, SFM_ERR_CONFIG, "%s: accumulate=%d, need 0 or 1", who, d->accumulate);
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->weight[s] >= 0.f, SFM_ERR_CONFIG, "%s: weight[%d]=%g, need weight >= 0", who, s, (double)d->weight[s]);
    A.weight[s] = d->weight[s];
  }
  if (d->B == 0 || stage == 0) return SFM_OK;   // empty batch: nothing to do, pointers may be NULL
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->disp[s], SFM_ERR_NULL, "%s: disp[%d] is NULL", who, s);
    SFM_REQUIRE(d->img[s], SFM_ERR_NULL, "%s: img[%d] is NULL", who, s);
    if (stage == 2) SFM_REQUIRE(d->g_disp[s], SFM_ERR_NULL, "%s: g_disp[%d] is NULL", who, s);
    A.disp[s] = d->disp[s], A.img[s] = d->img[s], A.g_disp[s] = d->g_disp[s];
  }
  if (stage == 1) SFM_REQUIRE(d->loss, SFM_ERR_NULL, "%s: loss is NULL", who);
  SFM_REQUIRE(d->stats, SFM_ERR_NULL, "%s: stats is NULL", who);
  if (stage == 2) SFM_REQUIRE(d->g_loss, SFM_ERR_NULL, "%s: g_loss is NULL", who);
  A.loss = d->loss, A.stats = d->stats, A.g_loss = d->g_loss;
  return SFM_OK;
}

// three doubles per block
static size_t disp_smooth_ws_bytes(const DispSmoothArgs& A) {
  const size_t need = (size_t)A.begin[A.n_scales] * 3 * sizeof(double);
  return need ? (need + 255) / 256 * 256 : 256;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

size_t sfm_disp_smooth_workspace_bytes(const SfmDispSmoothDesc* d) {
  DispSmoothArgs A = {};
  if (disp_smooth_setup(A, "sfm_disp_smooth_workspace_bytes", d, 0)) return 0;
  return disp_smooth_ws_bytes(A);
}

int sfm_disp_smooth_fwd(const SfmDispSmoothDesc* d, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "sfm_disp_smooth_fwd";
  DispSmoothArgs A = {};
  if (int e = disp_smooth_setup(A, who, d, 1)) return e;
  if (d->B == 0) return SFM_OK;
  const size_t need = disp_smooth_ws_bytes(A);
  SFM_REQUIRE(ws && ws_bytes >= need, SFM_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, got %zu", who, need, ws ? ws_bytes : (size_t)0);
  SFM_REQUIRE(((uintptr_t)ws & 255) == 0, SFM_ERR_WORKSPACE, "%s: workspace must be aligned to 256 bytes", who);
  A.part = (double*)ws;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(disp_smooth_fwd_kernel, dim3(A.begin[A.n_scales]), dim3(DS_BLOCK), 0, st, A);
  hipLaunchKernelGGL(disp_smooth_fold_kernel, dim3(1), dim3(64 * DS_FOLD_WAVES), 0, st, A);
  return check_launch(who);
}

int sfm_disp_smooth_bwd(const SfmDispSmoothDesc* d, void* stream) {
  const char* who = "sfm_disp_smooth_bwd";
  DispSmoothArgs A = {};
  if (int e = disp_smooth_setup(A, who, d, 2)) return e;
  if (d->B == 0) return SFM_OK;
  hipLaunchKernelGGL(disp_smooth_bwd_kernel, dim3(A.begin[A.n_scales]), dim3(DS_BLOCK), 0, (hipStream_t)stream, A);
  return check_launch(who);
}

}  // extern "C"
