// The per-pixel photometric error maps of a whole warped pyramid (include/sfmwarp.h): alpha * SSIM + (1 - alpha) * L1 of
// every (scale, sample, image) in ONE launch, its gradient with respect to the images in ONE launch.  No workspace, no atomics, no
// LDS: every output element is written once by one lane, in a fixed evaluation order.  gfx950 only.
//
// One grid covers every tile of every scale: wave index -> (scale, sample, row chunk, column strip, image) through per-scale prefix
// counts, the image fastest, so that the waves of a workgroup read the same target rows.  A wave owns a strip of 64 columns, one
// lane per column, and marches down PE_ROWS rows with the rows it still needs in registers:
//   horizontal 3-sums  hsum3 (DPP wave shifts: lanes 0 and 63 have no neighbour, so each pooling costs one column on each side),
//   vertical 3-sums    the sums of the two rows before, kept in registers (each pooling costs one row at each chunk end).
// The forward pools once: 62 useful columns per strip, rows y0-1 .. y1.  The backward pools twice -- the statistics at p, then the
// three partial maps at q -- hence 60 useful columns and rows y0-2 .. y1+1; the statistics are recomputed, never stored.
// Outside the image every load is clamped to an address inside it and its value replaced by zero: the zero padding of
// F.average_pooling_2d costs no divergent load.  REFLECT (include/sfmwarp_conventions.h) is a template parameter of both kernels: the
// same march over the image extended by ReflectionPad2d(1) -- the ring's loads are clamps of the same kind, its share of the backward
// is folded back in registers --, the zero-padded instantiations keep their code.
//
// The pooled quantities stay 3x3 SUMS (sx = 9 mu_x, ...): the SSIM index is a ratio in which every 1/9 cancels,
//   S = (2 sx sy + 81 c1)(2 (9 sxy - sx sy) + 81 c2) / ((sx^2 + sy^2 + 81 c1)(9 sxx - sx^2 + 9 syy - sy^2 + 81 c2)),
// one rounding per term less than dividing each sum first.
#include "sfm_common.h"
#include "sfm_warp_pixel.h"
#include "../../include/sfmwarp_conventions.h"

namespace sfm {

// the tile geometry (tests/test_photo_error_gpu.py reads these three lines)
constexpr int PE_ROWS = 16;        // rows of one chunk
constexpr int PE_FWD_STRIP = 62;   // useful columns of one forward strip:  64 lanes - 2 * 1 halo column
constexpr int PE_BWD_STRIP = 60;   // useful columns of one backward strip: 64 lanes - 2 * 2 halo columns
constexpr int PE_BLOCK = 256;
constexpr int PE_WAVES = PE_BLOCK / 64;

struct PhotoErrArgs {
  const float* img[SFM_MAX_SCALES];
  const float* tgt[SFM_MAX_SCALES];
  float* err[SFM_MAX_SCALES];            // fwd
  const float* g_err[SFM_MAX_SCALES];    // bwd
  float* d_img[SFM_MAX_SCALES];          // bwd
  int H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];
  int nstrip[SFM_MAX_SCALES];            // column strips of one image of scale s
  int nchunk[SFM_MAX_SCALES];            // row chunks of one image of scale s
  int begin[SFM_MAX_SCALES + 1];         // prefix sums of B * n_img * nstrip[s] * nchunk[s]: the first tile of scale s
  int B, n_img, n_scales;
  float w_l1;                            // (1 - alpha) / 3
  float w_ssim;                          // alpha / 3
};

// where a wave works -- uniform over the wave
struct PhotoErrTile {
  int s, H, W;
  int x0;             // first useful column of the strip
  int y0, y1;         // rows [y0, y1) of the chunk
  size_t image;       // b * n_img + i
  size_t sample;      // b
  bool any;
};

template <int STRIP>
__device__ __forceinline__ PhotoErrTile photo_err_tile(const PhotoErrArgs& A) {
  PhotoErrTile t;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long tile = (long long)blockIdx.x * PE_WAVES + wave;
  t.any = tile < (long long)A.begin[A.n_scales];
  const int id = t.any ? (int)tile : 0;
  t.s = scale_of<0>(id, A.begin, A.n_scales);
  t.H = A.H[t.s], t.W = A.W[t.s];
  int r = id - A.begin[t.s];
  const int i = r % A.n_img;
  r /= A.n_img;
  const int strip = r % A.nstrip[t.s];
  r /= A.nstrip[t.s];
  const int chunk = r % A.nchunk[t.s];
  const int b = r / A.nchunk[t.s];
  t.x0 = strip * STRIP;
  t.y0 = chunk * PE_ROWS;
  t.y1 = min(t.y0 + PE_ROWS, t.H);
  t.sample = (size_t)b;
  t.image = (size_t)b * A.n_img + i;
  return t;
}

constexpr float PE_C1 = 81.f * 1e-4f;   // 81 * 0.01^2: the constants of base_model.py:128-129 on the scale of the 3x3 sums
constexpr float PE_C2 = 81.f * 9e-4f;   // 81 * 0.03^2

// the five horizontal 3-sums of one channel of one row: X, Y, X^2, Y^2, XY
__device__ __forceinline__ void pe_hsums(const float x, const float y, float (&h)[5]) {
  h[0] = hsum3(x);
  h[1] = hsum3(y);
  h[2] = hsum3(x * x);
  h[3] = hsum3(y * y);
  h[4] = hsum3(x * y);
}

// what both passes need of the SSIM index at one pixel, from the 3x3 sums
struct PeStat {
  float sx, sy;
  float n1, n2, d1, d2;   // 81 x the n1, n2, d1, d2 of base_model.py:137-140
  float r;                // 1 / (d1 d2)
  float S;
};

__device__ __forceinline__ PeStat pe_stat(const float (&a)[5], const float (&b)[5], const float (&h)[5]) {
  PeStat o;
  o.sx = (a[0] + b[0]) + h[0];
  o.sy = (a[1] + b[1]) + h[1];
  const float sxx = (a[2] + b[2]) + h[2], syy = (a[3] + b[3]) + h[3], sxy = (a[4] + b[4]) + h[4];
  o.n1 = 2.f * o.sx * o.sy + PE_C1;
  o.n2 = 2.f * (9.f * sxy - o.sx * o.sy) + PE_C2;
  o.d1 = o.sx * o.sx + o.sy * o.sy + PE_C1;
  o.d2 = (9.f * sxx - o.sx * o.sx) + (9.f * syy - o.sy * o.sy) + PE_C2;
  const float den = o.d1 * o.d2;
  o.r = rcp_refined(den);
  o.S = div_r(o.n1 * o.n2, den, o.r);
  return o;
}

// one row of X and of Y, three channels: a lane outside the image (its column, or the whole row) holds zeros
struct PeRow {
  float x[3], y[3];
};

// REFLECT (include/sfmwarp_conventions.h): the image extended by ReflectionPad2d(1).  Index -1 reads index 1 and index n reads index
// n-2 (n >= 2); whatever lies further out is clamped into the image and dropped, as without reflection.
__device__ __forceinline__ int pe_reflect(const int i, const int n) {
  const int m = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
  return min(max(m, 0), n - 1);
}

template <bool REFLECT = false>
__device__ __forceinline__ PeRow pe_load_row(const float* X, const float* Y, const int row, const int H, const int W, const unsigned xc,
                                             const bool colin) {
  PeRow o;
  // (REFLECT: rows -1 and H count too, read from rows 1 and H-2 -- the row index stays uniform over the wave)
  const bool in = REFLECT ? colin & (row >= -1) & (row <= H) : colin & (row >= 0) & (row < H);
  const size_t P = (size_t)H * W;
  const size_t at = (size_t)(REFLECT ? pe_reflect(row, H) : min(max(row, 0), H - 1)) * W;      // in bounds; a value outside is dropped
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float xv = ldf(X + c * P + at, xc), yv = ldf(Y + c * P + at, xc);
    o.x[c] = in ? xv : 0.f;
    o.y[c] = in ? yv : 0.f;
  }
  return o;
}

template <bool SSIM, bool REFLECT = false>
__global__ void __launch_bounds__(PE_BLOCK) photo_err_fwd_kernel(const PhotoErrArgs A) {
  const PhotoErrTile t = photo_err_tile<PE_FWD_STRIP>(A);
  if (!t.any) return;
  const int H = t.H, W = t.W, lane = threadIdx.x & 63;
  const size_t P = (size_t)H * W;
  const int x = t.x0 + lane - 1;
  // the lane's value counts: the image's columns, with REFLECT the ring columns -1 and W too, loaded from 1 and W-2 -- a per-lane
  // clamp of the same kind, no divergent load (a lane that writes has xc == x either way)
  const bool colin = REFLECT ? (x >= -1) & (x <= W) : (x >= 0) & (x < W);
  const unsigned xc = (unsigned)(REFLECT ? pe_reflect(x, W) : min(max(x, 0), W - 1));
  const bool mine = (lane >= 1) & (lane <= PE_FWD_STRIP) & (x < W);      // the columns this lane writes
  const float* X = A.img[t.s] + t.image * 3 * P;
  const float* Y = A.tgt[t.s] + t.sample * 3 * P;
  float* out = A.err[t.s] + t.image * P;
  if constexpr (!SSIM) {
    for (int r = t.y0; r < t.y1; ++r) {
      const PeRow v = pe_load_row(X, Y, r, H, W, xc, colin);
      const float l1 = (fabsf(v.x[0] - v.y[0]) + fabsf(v.x[1] - v.y[1])) + fabsf(v.x[2] - v.y[2]);
      if (mine) stf(out + (size_t)r * W, xc, A.w_l1 * l1);
    }
  } else {
    float a[3][5], b[3][5];      // the horizontal sums of rows r-2 and r-1
    PeRow prev;                  // row r-1
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < 5; ++k) a[c][k] = b[c][k] = 0.f;
      prev.x[c] = prev.y[c] = 0.f;
    }
    for (int r = t.y0 - 1; r <= t.y1; ++r) {
      const PeRow v = pe_load_row<REFLECT>(X, Y, r, H, W, xc, colin);
      float h[3][5];
#pragma unroll
      for (int c = 0; c < 3; ++c) pe_hsums(v.x[c], v.y[c], h[c]);
      if (r > t.y0) {            // rows r-2, r-1, r are in hand: row r-1 goes out
        float l1 = 0.f, e = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const PeStat st = pe_stat(a[c], b[c], h[c]);
          const float ec = fminf(fmaxf(0.5f * (1.f - st.S), 0.f), 1.f);
          e = c ? e + ec : ec;
          const float ac = fabsf(prev.x[c] - prev.y[c]);
          l1 = c ? l1 + ac : ac;
        }
        if (mine) stf(out + (size_t)(r - 1) * W, xc, A.w_l1 * l1 + A.w_ssim * e);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int k = 0; k < 5; ++k) a[c][k] = b[c][k], b[c][k] = h[c][k];
      }
      prev = v;
    }
  }
}

// hsum3 of a partial map under REFLECT: the adjoint of "pad, then pool" along the row.  What the pooling sends to padded column -1
// comes from column 0 alone and belongs to column 1, what it sends to column W from column W-1 alone and belongs to column W-2: the
// neighbour's value hsum3 already holds, counted once more there (both at W == 3; columns 1 and 0 at W == 2).
__device__ __forceinline__ float pe_hsum3_fold(float m, const bool again_left, const bool again_right) {
  asm("" : "+v"(m));
  const float l = from_left(m), r = from_right(m);
  return ((m + l) + r) + ((again_left ? l : 0.f) + (again_right ? r : 0.f));
}

template <bool SSIM, bool REFLECT = false>
__global__ void __launch_bounds__(PE_BLOCK) photo_err_bwd_kernel(const PhotoErrArgs A) {
  const PhotoErrTile t = photo_err_tile<PE_BWD_STRIP>(A);
  if (!t.any) return;
  const int H = t.H, W = t.W, lane = threadIdx.x & 63;
  const size_t P = (size_t)H * W;
  const int x = t.x0 + lane - 2;
  const bool colin = (x >= 0) & (x < W);
  // the lane's X and Y count: colin, with REFLECT the ring columns -1 and W too, loaded from 1 and W-2 (g_err and the maps stay on colin)
  const bool colld = REFLECT ? (x >= -1) & (x <= W) : colin;
  const unsigned xc = (unsigned)(REFLECT ? pe_reflect(x, W) : min(max(x, 0), W - 1));
  const bool again_left = x == 1, again_right = x == W - 2;      // REFLECT: the columns that receive the ring's share
  const bool mine = (lane >= 2) & (lane < 2 + PE_BWD_STRIP) & (x < W);
  const float* X = A.img[t.s] + t.image * 3 * P;
  const float* Y = A.tgt[t.s] + t.sample * 3 * P;
  const float* G = A.g_err[t.s] + t.image * P;
  float* out = A.d_img[t.s] + t.image * 3 * P;
  if constexpr (!SSIM) {
    for (int r = t.y0; r < t.y1; ++r) {
      const PeRow v = pe_load_row(X, Y, r, H, W, xc, colin);
      const float g = A.w_l1 * ldf(G + (size_t)r * W, xc);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (mine) stf(out + c * P + (size_t)r * W, xc, g * signf(v.x[c] - v.y[c]));
    }
  } else {
    float a[3][5], b[3][5];      // the horizontal sums of X, Y, X^2, Y^2, XY of rows r-2 and r-1
    float ma[3][3], mb[3][3];    // the horizontal sums of the three partial maps of rows r-3 and r-2
    PeRow p1, p2;                // rows r-1 and r-2
    float g2 = 0.f;              // g_err of row r-2
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < 5; ++k) a[c][k] = b[c][k] = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) ma[c][k] = mb[c][k] = 0.f;
      p1.x[c] = p1.y[c] = p2.x[c] = p2.y[c] = 0.f;
    }
    const float kw = -0.5f * A.w_ssim;
    for (int r = t.y0 - 2; r <= t.y1 + 1; ++r) {
      const PeRow v = pe_load_row<REFLECT>(X, Y, r, H, W, xc, colld);
      float h[3][5], hm[3][3];
#pragma unroll
      for (int c = 0; c < 3; ++c) pe_hsums(v.x[c], v.y[c], h[c]);
      // the upstream gradient of row p = r-1, zero outside the image: so are the partial maps there (the second pooling is
      // zero-padded like the first; with REFLECT the maps exist at image pixels only and the ring's share is folded back below)
      const int p = r - 1;
      const bool pin = colin & (p >= 0) & (p < H);
      const float gl = ldf(G + (size_t)min(max(p, 0), H - 1) * W, xc);
      const float g1 = pin ? gl : 0.f;
      if (r >= t.y0) {           // rows r-2, r-1, r are in hand: the statistics and the partial maps of row p
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const PeStat st = pe_stat(a[c], b[c], h[c]);
          const float e = 0.5f * (1.f - st.S);
          const float kappa = (pin & (e > 0.f) & (e < 1.f)) ? kw * g1 : 0.f;                          // F.clip backward
          const float kr = kappa * st.r;
          // kappa times, on the scale of the sums, (1/9) dS/dmu_x, (1/81) dS/dE[xx], (1/162) dS/dE[xy]  (SURVEY.md App. A.3):
          // Pool's own 1/9 and these factors leave 1, 9 and 18 for the three sums below
          const float m0 = kr * (2.f * (st.sy * (st.n2 - st.n1) - st.S * st.sx * (st.d2 - st.d1)));
          const float m1 = kappa * (-st.S) * rcp_refined(st.d2);
          const float m2 = kr * st.n1;
          if constexpr (REFLECT) {
            hm[c][0] = pe_hsum3_fold(kappa != 0.f ? m0 : 0.f, again_left, again_right);
            hm[c][1] = pe_hsum3_fold(kappa != 0.f ? m1 : 0.f, again_left, again_right);
            hm[c][2] = pe_hsum3_fold(kappa != 0.f ? m2 : 0.f, again_left, again_right);
          } else {
            hm[c][0] = hsum3(kappa != 0.f ? m0 : 0.f);
            hm[c][1] = hsum3(kappa != 0.f ? m1 : 0.f);
            hm[c][2] = hsum3(kappa != 0.f ? m2 : 0.f);
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) hm[c][0] = hm[c][1] = hm[c][2] = 0.f;
      }
      if (r >= t.y0 + 2) {       // the maps of rows r-3, r-2, r-1 are in hand: row q = r-2 goes out
        const size_t at = (size_t)(r - 2) * W;
        const float gq = A.w_l1 * g2;
        // REFLECT, the same fold down the columns: padded row -1 holds the sums of row 0 alone and belongs to row 1, padded row H
        // those of row H-1 alone and belongs to row H-2 -- the previous or the next row's sums once more (uniform over the wave)
        const float up_again = (REFLECT && r - 2 == 1) ? 1.f : 0.f, down_again = (REFLECT && r - 2 == H - 2) ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float sa = (ma[c][0] + mb[c][0]) + hm[c][0];
          float sb = (ma[c][1] + mb[c][1]) + hm[c][1];
          float se = (ma[c][2] + mb[c][2]) + hm[c][2];
          if constexpr (REFLECT) {      // the three summed maps are completed first
            sa = sa + (up_again * ma[c][0] + down_again * hm[c][0]);
            sb = sb + (up_again * ma[c][1] + down_again * hm[c][1]);
            se = se + (up_again * ma[c][2] + down_again * hm[c][2]);
          }
          const float d = gq * signf(p2.x[c] - p2.y[c]) + (sa + 18.f * (p2.x[c] * sb + p2.y[c] * se));
          if (mine) stf(out + c * P + at, xc, d);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int k = 0; k < 5; ++k) a[c][k] = b[c][k], b[c][k] = h[c][k];
#pragma unroll
        for (int k = 0; k < 3; ++k) ma[c][k] = mb[c][k], mb[c][k] = hm[c][k];
      }
      p2 = p1, p1 = v, g2 = g1;
    }
  }
}

// What both calls check and fill in, in the order the header states.  bwd: the pointers of the backward, else those of the forward.
static int photo_err_setup(PhotoErrArgs& A, const char* who, const SfmPhotoErrorDesc* d, const bool bwd,
                           const int32_t padding = SFM_SSIM_PAD_ZERO) {
  SFM_REQUIRE(d, SFM_ERR_NULL, "%s: NULL descriptor", who);
  const int strip = bwd ? PE_BWD_STRIP : PE_FWD_STRIP;
  const auto tiles = [&A, d, strip](const int s, const int H, const int W) {
    A.nstrip[s] = (W + strip - 1) / strip;
    A.nchunk[s] = (H + PE_ROWS - 1) / PE_ROWS;
    return (long long)d->n_img * A.nstrip[s] * A.nchunk[s];
  };
  if (padding != SFM_SSIM_PAD_REFLECT) {
    if (int e = check_pyramid_shape(who, d->B, d->n_img, "n_img", d->n_scales, d->H, d->W, "wavefront tiles", ": the grid would overflow",
                                    tiles, A.H, A.W, A.begin))
      return e;
  } else {
    // The same checks in the same order with one difference: check_pyramid_shape refuses a frame below 3 x 3, which the zero-padded
    // calls keep refusing; the reflected window needs two rows and columns and no more, so here the shape group asks only for a
    // frame that exists and the reflection's own floor follows the settings, where include/sfmwarp_conventions.h states it.
    SFM_REQUIRE(d->n_img >= 1 && d->n_img <= SFM_MAX_SRC, SFM_ERR_SHAPE, "%s: n_img=%d, need 1..%d", who, d->n_img, SFM_MAX_SRC);
    SFM_REQUIRE(d->n_scales >= 1 && d->n_scales <= SFM_MAX_SCALES, SFM_ERR_SHAPE, "%s: n_scales=%d, need 1..%d", who, d->n_scales,
                SFM_MAX_SCALES);
    SFM_REQUIRE(d->B >= 0, SFM_ERR_SHAPE, "%s: B=%d", who, d->B);
    long long total = 0;
    A.begin[0] = 0;
    for (int s = 0; s < d->n_scales; ++s) {
      SFM_REQUIRE(d->H[s] >= 1 && d->W[s] >= 1, SFM_ERR_SHAPE, "%s: scale %d: H=%d W=%d, need H,W >= 1", who, s, d->H[s], d->W[s]);
      SFM_REQUIRE(3ll * d->H[s] * d->W[s] < (1ll << 31), SFM_ERR_SHAPE, "%s: scale %d: 3*H*W too large", who, s);
      A.H[s] = d->H[s], A.W[s] = d->W[s];
      total += (long long)d->B * tiles(s, A.H[s], A.W[s]);
      SFM_REQUIRE(total < (1ll << 31), SFM_ERR_SHAPE, "%s: too many wavefront tiles (%lld): the grid would overflow", who, total);
      A.begin[s + 1] = (int)total;
    }
  }
  A.B = d->B, A.n_img = d->n_img, A.n_scales = d->n_scales;
  SFM_REQUIRE(d->ssim_rate >= 0.f && d->ssim_rate <= 1.f, SFM_ERR_CONFIG, "%s: ssim_rate=%g, need 0 <= ssim_rate <= 1", who,
              (double)d->ssim_rate);
  A.w_l1 = (1.f - d->ssim_rate) / 3.f;
  A.w_ssim = d->ssim_rate / 3.f;
  SFM_REQUIRE(padding == SFM_SSIM_PAD_ZERO || padding == SFM_SSIM_PAD_REFLECT, SFM_ERR_CONFIG, "%s: padding=%d", who, (int)padding);
  if (padding == SFM_SSIM_PAD_REFLECT)
    for (int s = 0; s < d->n_scales; ++s)
      SFM_REQUIRE(d->H[s] >= 2 && d->W[s] >= 2, SFM_ERR_SHAPE, "%s: scale %d: H=%d W=%d, reflection padding needs H,W >= 2", who, s, d->H[s],
                  d->W[s]);
  if (d->B == 0) return SFM_OK;   // empty batch: nothing to do, pointers may be NULL
  for (int s = 0; s < d->n_scales; ++s) {
    SFM_REQUIRE(d->img[s], SFM_ERR_NULL, "%s: img[%d] is NULL", who, s);
    SFM_REQUIRE(d->tgt[s], SFM_ERR_NULL, "%s: tgt[%d] is NULL", who, s);
    if (bwd) {
      SFM_REQUIRE(d->g_err[s], SFM_ERR_NULL, "%s: g_err[%d] is NULL", who, s);
      SFM_REQUIRE(d->d_img[s], SFM_ERR_NULL, "%s: d_img[%d] is NULL", who, s);
    } else {
      SFM_REQUIRE(d->err[s], SFM_ERR_NULL, "%s: err[%d] is NULL", who, s);
    }
    A.img[s] = d->img[s], A.tgt[s] = d->tgt[s], A.err[s] = d->err[s], A.g_err[s] = d->g_err[s], A.d_img[s] = d->d_img[s];
  }
  return SFM_OK;
}

static dim3 photo_err_grid(const PhotoErrArgs& A) { return dim3((unsigned)((A.begin[A.n_scales] + PE_WAVES - 1) / PE_WAVES)); }

// the two calls, for either padding: the existing entry points pass SFM_SSIM_PAD_ZERO.  Without the SSIM term no window is formed
// and the padding selects nothing.
static int photo_err_fwd(const char* who, const SfmPhotoErrorDesc* d, const int32_t padding, void* stream) {
  PhotoErrArgs A = {};
  if (int e = photo_err_setup(A, who, d, false, padding)) return e;
  if (d->B == 0) return SFM_OK;
  const dim3 grid = photo_err_grid(A), block(PE_BLOCK);
  const hipStream_t st = (hipStream_t)stream;
  if (!(d->ssim_rate > 0.f)) hipLaunchKernelGGL((photo_err_fwd_kernel<false, false>), grid, block, 0, st, A);
  else if (padding == SFM_SSIM_PAD_REFLECT) hipLaunchKernelGGL((photo_err_fwd_kernel<true, true>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((photo_err_fwd_kernel<true, false>), grid, block, 0, st, A);
  return check_launch(who);
}

static int photo_err_bwd(const char* who, const SfmPhotoErrorDesc* d, const int32_t padding, void* stream) {
  PhotoErrArgs A = {};
  if (int e = photo_err_setup(A, who, d, true, padding)) return e;
  if (d->B == 0) return SFM_OK;
  const dim3 grid = photo_err_grid(A), block(PE_BLOCK);
  const hipStream_t st = (hipStream_t)stream;
  if (!(d->ssim_rate > 0.f)) hipLaunchKernelGGL((photo_err_bwd_kernel<false, false>), grid, block, 0, st, A);
  else if (padding == SFM_SSIM_PAD_REFLECT) hipLaunchKernelGGL((photo_err_bwd_kernel<true, true>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((photo_err_bwd_kernel<true, false>), grid, block, 0, st, A);
  return check_launch(who);
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_photo_error_fwd(const SfmPhotoErrorDesc* d, void* stream) { return photo_err_fwd("sfm_photo_error_fwd", d, SFM_SSIM_PAD_ZERO, stream); }

int sfm_photo_error_bwd(const SfmPhotoErrorDesc* d, void* stream) { return photo_err_bwd("sfm_photo_error_bwd", d, SFM_SSIM_PAD_ZERO, stream); }

// include/sfmwarp_conventions.h
int sfm_photo_error_pad_fwd(const SfmPhotoErrorDesc* d, int32_t padding, void* stream) {
  return photo_err_fwd("sfm_photo_error_pad_fwd", d, padding, stream);
}

int sfm_photo_error_pad_bwd(const SfmPhotoErrorDesc* d, int32_t padding, void* stream) {
  return photo_err_bwd("sfm_photo_error_pad_bwd", d, padding, stream);
}

}  // extern "C"
