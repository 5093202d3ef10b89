/*
 * sfmwarp_disp_smooth.h -- a SIDE header of libsfmwarp.so: sfm_disp_smooth_*, the second term of a Monodepth2-style loss, the
 * edge-aware smoothness of the (mean-normalised) disparity.  It stands beside include/sfmwarp.h (whose conventions, constants and
 * error codes it uses) and include/sfmwarp_min_reproj.h for the same reason as the latter: the tables that pin sfmwarp.h's
 * descriptors and pointer prototypes live in test files a feature does not edit.  FOLLOW-UP: fold this section into sfmwarp.h (and
 * _lib.SMOOTH_SYMBOLS into _lib.SYMBOLS) together with those tables.  SFM_ABI_VERSION is unchanged: nothing that existed moved.
 */
#ifndef SFMWARP_DISP_SMOOTH_H_
#define SFMWARP_DISP_SMOOTH_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The edge-aware first-order smoothness of the disparity of every scale of a step.
 *
 * For sample b, scale s with map h x w, P = h * w, disparity d (B,1,h,w) and image I (B,3,h,w), planar:
 *   M_b   = normalize ? (sum_p d[b,p]) / P + 1e-7 : 1                                                       (fp64)
 *   a_x(y,x) = edge == MEAN_ABS ? (|DxI_0| + |DxI_1|) + |DxI_2|  :  |(DxI_0 + DxI_1) + DxI_2|,   DxI_c = I_c(y,x+1) - I_c(y,x)
 *   w_x(y,x) = exp(-a_x / 3),   and a_y, w_y likewise with Dy = (y+1,x) - (y,x)                            (fp32 per pixel)
 *   X_b   = sum over y < h, x < w-1 of |d(y,x+1) - d(y,x)| * w_x(y,x)       (terms in fp32, summed in fp64 in a fixed order)
 *   Y_b   = sum over y < h-1, x < w of |d(y+1,x) - d(y,x)| * w_y(y,x)
 *   c_x   = 1 / (B*h*(w-1)),  c_y = 1 / (B*(h-1)*w)
 *   loss[s]        = (float) sum_b (c_x X_b + c_y Y_b) / |M_b|              (b ascending)
 *   loss[n_scales] = (float) sum_s (double)weight[s] * (the fp64 value of loss[s])
 *   stats[(s*B + b)*3 + 0..2] = M_b, X_b, Y_b
 * |D(d/M)| = |Dd| / |M|: the value is the smoothness of d / M_b without a normalised copy.
 * edge = MEAN_ABS with normalize = 1 is Monodepth2's get_smooth_loss on disp / (mean + 1e-7); edge = ABS_MEAN with normalize = 0 is
 * compute_disp_smooth of models/base_model.py:144-155.
 * Non-finite and degenerate inputs: a NaN disparity makes X_b, Y_b (and, with normalize, M_b) of that sample NaN, hence loss[s] and
 * loss[n_scales]; with normalize every gradient of that sample is NaN, without it the gradient stays FINITE (it is sign(Dd) w c, and
 * the sign of a NaN difference is taken as +-1): the loss, not the gradient, reports it.  A zero disparity among positive ones is
 * an ordinary value.  Other samples' statistics and gradients keep their bits (tests/test_hostile_inputs_gpu.py).
 * M_b = 0 is not checked (a network's disparities are positive): the divisions then give +inf, or NaN where X_b = Y_b = 0, in
 * loss[s], loss[n_scales] and every gradient of that sample.
 * ---------------------------------------------------------------------------------------- */
#define SFM_DISP_SMOOTH_EDGE_MEAN_ABS 0 /* exp(-mean_c |DI_c|)                                         */
#define SFM_DISP_SMOOTH_EDGE_ABS_MEAN 1 /* exp(-|mean_c DI_c|)                                         */

typedef struct SfmDispSmoothDesc {
  int32_t B, n_scales;
  int32_t H[SFM_MAX_SCALES], W[SFM_MAX_SCALES]; /* independent per scale (not required to be halvings), each >= 3         */
  int32_t normalize;                            /* 0 or 1                                                                  */
  int32_t edge;                                 /* SFM_DISP_SMOOTH_EDGE_*                                                  */
  int32_t accumulate;                           /* 0 or 1; read by the backward only                                       */
  float weight[SFM_MAX_SCALES];                 /* of scale s in loss[n_scales]; >= 0, not NaN                            */
  const float *disp[SFM_MAX_SCALES];            /* (B,1,h,w)                                                               */
  const float *img[SFM_MAX_SCALES];             /* (B,3,h,w) planar                                                        */
  float *loss;                                  /* fwd: n_scales + 1 floats, overwritten                                   */
  double *stats;                                /* n_scales * B * 3 doubles [s][b][M,X,Y]: fwd overwrites, bwd reads       */
  const float *g_loss;                          /* bwd: n_scales + 1 floats, the upstream gradients of loss                */
  float *g_disp[SFM_MAX_SCALES];                /* bwd: (B,1,h,w), overwritten, or added to with accumulate                */
} SfmDispSmoothDesc;

/* Forward, two launches: one over runs of consecutive pixels of every (scale, sample) -- one pass over d and I that writes one
 * partial of three doubles (sum d, X, Y) per run into ws -- and a fold of one block, which adds the partials of each sample in a
 * fixed order in fp64, writes stats, and adds the samples and then the scales in ascending order.  No atomics: two calls on the same
 * inputs agree bit for bit.
 * Reads disp, img, weight; writes loss, stats; ignores g_loss, g_disp and accumulate's meaning (its range is still checked).
 * ws: sfm_disp_smooth_workspace_bytes(d) bytes of scratch on a 256-byte boundary (a multiple of 256; 24 bytes per run of pixels;
 * 0 on a descriptor whose sizes or settings the forward rejects -- the query looks at no pointer).  Content undefined before and
 * after the call. */
size_t sfm_disp_smooth_workspace_bytes(const SfmDispSmoothDesc *d);
int sfm_disp_smooth_fwd(const SfmDispSmoothDesc *d, void *ws, size_t ws_bytes, void *stream);

/* Backward for the upstream gradients g_loss, one launch.  With k_s = g_loss[s] + weight[s] * g_loss[n_scales],
 * t_x = sign(Dxd) * w_x, t_y = sign(Dyd) * w_y, sign(0) = 0, and terms past the border equal to 0:
 *   g(b,y,x) = (k_s c_x / |M_b|) (t_x(y,x-1) - t_x(y,x)) + (k_s c_y / |M_b|) (t_y(y-1,x) - t_y(y,x))
 *              - normalize * k_s (c_x X_b + c_y Y_b) / (M_b |M_b| P)        (the path through the mean: the same for every pixel of b)
 *   g_disp[s][b,y,x] = accumulate ? g_disp[s][b,y,x] + g : g                (g formed first, then ONE fp32 addition; every element written)
 * The three per-sample factors are formed once per block in fp64 and rounded to fp32.  stats and g_loss are read on the device: the
 * host reads nothing, so the call can be captured in a graph.  The image gets no gradient (a constant).
 * Reads disp, img, stats, g_loss, weight; writes g_disp; ignores loss. */
int sfm_disp_smooth_bwd(const SfmDispSmoothDesc *d, void *stream);

/* Errors of the calls, checked in this order before any HIP call:
 *   d NULL -> SFM_ERR_NULL;
 *   n_scales outside 1..SFM_MAX_SCALES, B < 0, any H[s] or W[s] < 3, 3 * H[s] * W[s] >= 2^31, or 2^31 or more runs of pixels in all
 *     -> SFM_ERR_SHAPE;
 *   normalize not 0 or 1, edge not SFM_DISP_SMOOTH_EDGE_MEAN_ABS or SFM_DISP_SMOOTH_EDGE_ABS_MEAN, accumulate not 0 or 1, or a
 *     weight[s], s < n_scales, negative or NaN -> SFM_ERR_CONFIG (in this order);
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned (an empty shard's pointers may be NULL);
 *   a pointer the call reads or writes is NULL -> SFM_ERR_NULL:
 *     sfm_disp_smooth_fwd: disp[s], img[s] scale by scale, then loss, stats;
 *     sfm_disp_smooth_bwd: disp[s], img[s], g_disp[s] scale by scale, then stats, g_loss;
 *   sfm_disp_smooth_fwd: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE. */

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_DISP_SMOOTH_H_ */
