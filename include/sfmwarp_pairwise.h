/*
 * sfmwarp_pairwise.h -- a SIDE header of libsfmwarp.so: sfm_pairwise_*, the masked means of SC-SfMLearner's compute_pairwise_loss
 * (Bian et al., NeurIPS 2019) -- the last stage behind sfm_warp_pyramid_*, sfm_photo_error_* and sfm_depth_consistency_*.  It stands
 * beside include/sfmwarp.h (whose constants and error codes it uses) for the same reason as the other six side headers: the tables
 * that pin sfmwarp.h's prototypes live in test files a feature does not edit.  FOLLOW-UP: fold this header (and
 * _lib.PAIRWISE_SYMBOLS into _lib.SYMBOLS) into sfmwarp.h at the next change of SFM_ABI_VERSION.  The version is unchanged here:
 * nothing that existed moved.
 *
 * What it restates of SC-SfMLearner, by function name (formulas quoted, no code taken):
 *   compute_pairwise_loss:  weight_mask = 1 - diff_depth;  diff_img = diff_img * weight_mask (with_mask);
 *                           auto_mask = (diff_img.mean(1) < (tgt_img - ref_img).abs().mean(1)) * valid_mask (with_auto_mask);
 *                           reconstruction_loss = mean_on_mask(diff_img, valid_mask);
 *                           geometry_consistency_loss = mean_on_mask(diff_depth, valid_mask).
 *   mean_on_mask:           mask.sum() > 10000 ? (diff * mask).sum() / mask.sum() : 0, the mask expanded to the channels of diff.
 *                           On this library's channel-mean error map that is min_count_photo = 3333 and min_count_geom = 10000;
 *                           0 for both is the clamp(min=1) of INTEGRATION.md 5.
 *
 * Non-finite inputs (sfmwarp.h, "NON-FINITE AND DEGENERATE INPUTS"): the kernels form no address from data -- every index comes from
 * the block and lane numbers and the descriptor's sizes.  A dropped pixel is excluded by SELECTION, not by a product with 0: a NaN or
 * an infinity in err or diff there changes no output.  At a kept pixel it reaches photo and geom of that (scale, source), the two
 * totals, and in the backward that pixel's g_err / g_diff, nothing else.  A NaN in valid, ident or cmp drops the pixel (the
 * comparisons are strict and false on NaN).
 */
#ifndef SFMWARP_PAIRWISE_H_
#define SFMWARP_PAIRWISE_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SfmPairwiseDesc {
  int32_t B, n_src, n_scales;
  int32_t H[SFM_MAX_SCALES], W[SFM_MAX_SCALES]; /* independent per scale                                                       */
  int32_t detach_weight;                        /* 0 | 1: 1 = the weight 1 - diff carries no gradient to diff                  */
  int32_t min_count_photo, min_count_geom;      /* >= 0: a mean over count <= min_count pixels is 0 (mean_on_mask)             */
  float weight[SFM_MAX_SCALES];                 /* of scale s in the two totals; >= 0, not NaN                                 */
  const float *err[SFM_MAX_SCALES];             /* (B,n_src,h,w) the photometric error of the warped sources                   */
  const float *diff[SFM_MAX_SCALES];            /* (B,n_src,h,w) diff_depth of sfm_depth_consistency_fwd                       */
  const float *valid[SFM_MAX_SCALES];           /* fwd: (B,n_src,h,w) or NULL, scale by scale                                  */
  const float *ident[SFM_MAX_SCALES];           /* fwd: (B,n_src,h,w), or NULL for EVERY scale: no auto-mask                   */
  const float *cmp[SFM_MAX_SCALES];             /* fwd: (B,n_src,h,w), or NULL for EVERY scale: err is compared with ident     */
  int8_t *keep[SFM_MAX_SCALES];                 /* (B,n_src,h,w) 0 | 1: overwritten by the forward, read by the backward       */
  float *loss;                                  /* fwd: 2*n_scales*n_src + 2 floats, overwritten (layout below)                */
  int32_t *count;                               /* n_scales*n_src: overwritten by the forward, read by the backward            */
  const float *g_loss;                          /* bwd: the upstream gradients, in the layout of loss                          */
  float *g_err[SFM_MAX_SCALES];                 /* bwd: (B,n_src,h,w) overwritten                                              */
  float *g_diff[SFM_MAX_SCALES];                /* bwd: (B,n_src,h,w) overwritten, or NULL for EVERY scale: not computed       */
} SfmPairwiseDesc;

/* ------------------------------------------------------------------------------------------
 * loss = photo[s*n_src+i] (n_scales*n_src floats), then geom[s*n_src+i], then photo_total, geom_total.
 *
 * Per (scale s, source i), over the whole batch; float32 without fused multiply-adds unless stated:
 *   c          = cmp ? cmp[s][b,i,p] : err[s][b,i,p]
 *   keep(b,p)  = (valid[s] NULL or valid[s][b,i,p] > 0) and (ident NULL or c < ident[s][b,i,p])       strict: a NaN drops the pixel
 *   t(b,p)     = err * (1.0f - diff)                                    one float32 subtraction, one float32 product
 *   count[s,i] = the number of kept pixels
 *   Sp, Sg     = the fp64 sums of (double)t and (double)diff over the kept pixels, in a fixed order
 *   photo[s,i] = count > min_count_photo ? (float)(Sp / max(count,1)) : 0
 *   geom[s,i]  = count > min_count_geom  ? (float)(Sg / max(count,1)) : 0
 *   photo_total = (float)(sum over s ascending of (double)weight[s] * (sum over i ascending of the fp64 quotients, 0 where the
 *                 threshold fails));   geom_total likewise.
 *
 * FORWARD, two launches: one over runs of 256 consecutive pixels of every (scale, sample) -- it writes keep and one (fp64 Sp, fp64
 * Sg, int32 count) partial per (run, source) into ws -- and a fold of one wavefront per (scale, source): lane l adds the partials
 * l, l + 64, ... of its (scale, source) in ascending order (sample-major, then run), the lanes are combined by the xor butterfly,
 * then one thread adds the totals in ascending order.  No atomics: two calls on the same inputs agree bit for bit, whatever ws held.
 * Reads err, diff, valid, ident, cmp, weight, min_count_*; ignores g_loss, g_err, g_diff, detach_weight's value (it is checked).
 * ws: sfm_pairwise_workspace_bytes(d) bytes on a 256-byte boundary (a multiple of 256: 20 bytes per (run, source); 0 on a
 * descriptor whose sizes or settings the forward rejects -- the query looks at no pointer).  Content undefined before and after.
 *
 * BACKWARD for g_loss, one launch:
 *   cp = count > min_count_photo ? (float)(((double)g_loss[photo s,i] + (double)weight[s] * (double)g_loss[photo_total]) / max(count,1)) : 0
 *   cg = likewise from the geom entries and min_count_geom
 *   g_err [s][b,i,p] = keep ? (1.0f - diff) * cp : 0
 *   g_diff[s][b,i,p] = keep ? (detach_weight ? cg : cg - err * cp) : 0                  every element written
 * keep, count, g_loss, err and diff are read on the device: the host reads nothing, so the call can be captured in a graph.
 * valid, ident and cmp get no gradient (constants).  Reads keep, count, g_loss, err, diff, weight, min_count_*, detach_weight.
 *
 * Errors, checked in this order before any HIP call:
 *   d NULL -> SFM_ERR_NULL;
 *   n_src outside 1..SFM_MAX_SRC, n_scales outside 1..SFM_MAX_SCALES, B < 0, any H[s] or W[s] < 3, 3 * H[s] * W[s] >= 2^31, 2^31 or
 *     more runs of pixels in all, or B * H[s] * W[s] >= 2^31 (count is an int32) -> SFM_ERR_SHAPE;
 *   detach_weight not 0 or 1, min_count_photo < 0, min_count_geom < 0, or a weight[s], s < n_scales, negative or NaN
 *     -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned (an empty shard's pointers may be NULL);
 *   a pointer the call reads or writes is NULL -> SFM_ERR_NULL: per scale err, diff, keep and (bwd) g_err; then (fwd) loss, count,
 *     (bwd) g_loss;  valid[s] is optional scale by scale, g_diff when NULL for every scale;
 *   ident, cmp (fwd) or g_diff (bwd) bound for some scales but not all -> SFM_ERR_NULL;
 *   sfm_pairwise_fwd: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
size_t sfm_pairwise_workspace_bytes(const SfmPairwiseDesc *d);
int    sfm_pairwise_fwd(const SfmPairwiseDesc *d, void *ws, size_t ws_bytes, void *stream);
int    sfm_pairwise_bwd(const SfmPairwiseDesc *d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_PAIRWISE_H_ */
