/*
 * sfmwarp_min_reproj.h -- a SIDE header of libsfmwarp.so: sfm_min_reproj_*, the last stage of a Monodepth2-style loss on the
 * library's warp.  It stands beside include/sfmwarp.h (whose conventions, constants and error codes it uses) because the tables that
 * pin that header's descriptors and pointer prototypes live in test files a feature does not edit; sfm_photo_error_* started the
 * same way.  FOLLOW-UP: fold this section into sfmwarp.h (and _lib.EXT_SYMBOLS into _lib.SYMBOLS) together with those tables.
 * SFM_ABI_VERSION is unchanged: nothing that existed moved.
 */
#ifndef SFMWARP_MIN_REPROJ_H_
#define SFMWARP_MIN_REPROJ_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The per-pixel minimum over the sources, the auto-mask and the mean of every scale of a step.
 *
 * What it is for: the third stage behind sfm_warp_pyramid_* and sfm_photo_error_*.  `err` holds the error maps of the WARPED
 * sources (sfm_photo_error_fwd on the warped pyramid), `valid` the in-view masks of the warp, `ident` the error maps of the UNWARPED
 * sources, which the auto-mask compares against (static scenes, objects that move with the camera).  Per sample b, scale s and
 * pixel p:
 *   best = +inf, win = -1
 *   for i = 0 .. n_err-1 ascending:   if (valid[s] NULL or valid[s][b,i,p] > 0) and err[s][b,i,p] < best:  best = err, win = i
 *                                     (the first index wins a tie; a NaN or +inf entry never wins)
 *   floor = +inf;  for j = 0 .. n_ident-1 ascending:  if ident[s][b,j,p] < floor:  floor = ident
 *   keep   = win >= 0 and (n_ident == 0 or best < floor)            (strict)
 *   winner[s][b,p] = keep ? win : -1
 * and per scale, over the batch:
 *   count[s] = the number of kept pixels,   sum[s] = the sum of `best` over them (fp64, a fixed order),
 *   denom[s] = max(count[s], 1) for SFM_MIN_REPROJ_NORM_KEPT  |  B * h * w for SFM_MIN_REPROJ_NORM_ALL,
 *   loss[s]  = (float)(sum[s] / denom[s]),
 *   loss[n_scales] = (float)(sum over s, ascending, of (double)weight[s] * sum[s] / denom[s]).
 * A scale with nothing kept has loss 0 and count 0 under either norm.
 * ---------------------------------------------------------------------------------------- */
#define SFM_MIN_REPROJ_NORM_KEPT 0 /* the mean over the kept pixels                                   */
#define SFM_MIN_REPROJ_NORM_ALL 1  /* the mean over all pixels, the dropped ones counted as zeros     */

typedef struct SfmMinReprojDesc {
  int32_t B, n_err, n_ident, n_scales;          /* n_ident = 0: no auto-mask, ident[] is not read                          */
  int32_t H[SFM_MAX_SCALES], W[SFM_MAX_SCALES]; /* independent per scale (not required to be halvings)                     */
  int32_t norm;                                 /* SFM_MIN_REPROJ_NORM_*                                                   */
  float weight[SFM_MAX_SCALES];                 /* of scale s in loss[n_scales]; >= 0, not NaN                            */
  const float *err[SFM_MAX_SCALES];             /* fwd: (B,n_err,h,w)                                                      */
  const float *valid[SFM_MAX_SCALES];           /* fwd: (B,n_err,h,w) or NULL, scale by scale                              */
  const float *ident[SFM_MAX_SCALES];           /* fwd: (B,n_ident,h,w), read iff n_ident > 0                              */
  int8_t *winner[SFM_MAX_SCALES];               /* (B,h,w): overwritten by the forward, read by the backward               */
  float *loss;                                  /* fwd: n_scales + 1 floats, overwritten                                   */
  int32_t *count;                               /* n_scales: overwritten by the forward, read by the backward              */
  const float *g_loss;                          /* bwd: n_scales + 1 floats, the upstream gradients of loss                */
  float *g_err[SFM_MAX_SCALES];                 /* bwd: (B,n_err,h,w) overwritten                                          */
} SfmMinReprojDesc;

/* Forward, two launches: one over runs of consecutive pixels of every (scale, sample) -- it writes winner and one (fp64 sum, int32
 * count) partial per run into ws -- and a fold of one wavefront per scale, which adds the partials in a fixed order in fp64 and
 * writes loss and count.  No atomics: two calls on the same inputs agree bit for bit.
 * Reads err, valid, ident, weight; ignores g_loss and g_err.
 * ws: sfm_min_reproj_workspace_bytes(d) bytes of scratch on a 256-byte boundary (a multiple of 256; 12 bytes per run of pixels;
 * 0 on a descriptor whose sizes or settings the forward rejects -- the query looks at no pointer).  Content undefined before and
 * after the call. */
size_t sfm_min_reproj_workspace_bytes(const SfmMinReprojDesc *d);
int sfm_min_reproj_fwd(const SfmMinReprojDesc *d, void *ws, size_t ws_bytes, void *stream);

/* Backward for the upstream gradients g_loss, one launch:
 *   c_s = (float)(((double)g_loss[s] + (double)weight[s] * (double)g_loss[n_scales]) / denom[s])
 *   g_err[s][b,i,p] = winner[s][b,p] == i ? c_s : 0             every element written
 * winner, count (for denom under SFM_MIN_REPROJ_NORM_KEPT) and g_loss are read on the device: the host reads nothing, so the call
 * can be captured in a graph.  `valid` and `ident` get no gradient (constants); neither does a source that lost the minimum.
 * Reads winner, count, g_loss, weight; ignores err, valid, ident and loss. */
int sfm_min_reproj_bwd(const SfmMinReprojDesc *d, void *stream);

/* Errors of the calls, checked in this order before any HIP call:
 *   d NULL -> SFM_ERR_NULL;
 *   n_err outside 1..SFM_MAX_SRC, n_scales outside 1..SFM_MAX_SCALES, B < 0, any H[s] or W[s] < 3, 3 * H[s] * W[s] >= 2^31, 2^31 or
 *     more runs of pixels in all, n_ident outside 0..SFM_MAX_SRC, or B * H[s] * W[s] >= 2^31 (count[s] is an int32)
 *     -> SFM_ERR_SHAPE;
 *   norm not SFM_MIN_REPROJ_NORM_KEPT or SFM_MIN_REPROJ_NORM_ALL, or a weight[s], s < n_scales, negative or NaN -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned (an empty shard's pointers may be NULL);
 *   a pointer the call reads or writes is NULL (valid[s] excepted; ident[s] only with n_ident > 0) -> SFM_ERR_NULL;
 *   sfm_min_reproj_fwd: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE. */

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_MIN_REPROJ_H_ */
