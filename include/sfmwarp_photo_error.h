/*
 * sfmwarp_photo_error.h -- the per-pixel photometric error maps of a whole warped pyramid: entry points of libsfmwarp.so next to
 * the sets that sfmwarp.h, sfmwarp_ext.h, sfmwarp_intrinsics.h and sfmwarp_warp_pyramid.h declare.  Same library, same conventions
 * (float32, C-contiguous device tensors owned by the caller; 4-byte alignment; "overwritten" outputs are written completely and
 * never read; return 0, SFM_ERR_* before anything is launched, or a hipError_t; sfm_last_error() has the message) and the same
 * SFM_ABI_VERSION: nothing declared in the other headers changes.
 *
 * What it is for: the companion of sfm_warp_pyramid_*.  A loss of the caller's own on the warped images -- a per-pixel minimum over
 * the sources, auto-masking against the unwarped source, a robust penalty -- is "alpha * SSIM + (1 - alpha) * L1 per pixel, then a
 * minimum or a mask, then a mean".  The fused loss (sfm_loss_*) reduces its SSIM to a scalar at once and takes no upstream
 * gradient; these calls hand out the per-pixel map of every (scale, image) of a step in ONE launch and differentiate it with
 * respect to the images in ONE more, so that what remains for the caller works on small single-channel maps.
 *
 * Per sample b, image i, scale s, pixel p and channel c = 0..2, with X = img, Y = tgt and Pool the zero-padded 3x3 sum divided by 9
 * always (F.average_pooling_2d(., 3, 1, 1)):
 *   S_c    = the SSIM index of models/base_model.py:126-142 (c1 = 0.01^2, c2 = 0.03^2),   e_c = clip((1 - S_c) / 2, 0, 1)
 *   err(p) = (1 - alpha) * (1/3) * sum_c |X_c - Y_c|(p)  +  alpha * (1/3) * sum_c e_c(p)
 * This is the reference's own zero-padded window (not the reflection padding of Monodepth2).  Nothing is masked inside: the zeros of
 * out-of-view pixels take part in their neighbours' windows as in the reference, and the caller has `valid` from the warp.
 */
#ifndef SFMWARP_PHOTO_ERROR_H_
#define SFMWARP_PHOTO_ERROR_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SfmPhotoErrorDesc {
  int32_t B, n_img, n_scales;                     /* n_img images per sample, all compared with that sample's one target */
  int32_t H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];   /* independent per scale (not required to be halvings)                 */
  float ssim_rate;                                /* alpha in [0,1]; 0 = L1 only (no SSIM code runs), 1 = SSIM only      */
  const float *img[SFM_MAX_SCALES];               /* (B,n_img,3,h,w) planar: the layout of SfmWarpPyramidDesc.warped,    */
                                                  /* byte for byte the planar source pyramid (B,3*n_img,h,w)             */
  const float *tgt[SFM_MAX_SCALES];               /* (B,3,h,w) planar                                                    */
  float *err[SFM_MAX_SCALES];                     /* fwd: (B,n_img,h,w) overwritten                                      */
  const float *g_err[SFM_MAX_SCALES];             /* bwd: (B,n_img,h,w)                                                  */
  float *d_img[SFM_MAX_SCALES];                   /* bwd: (B,n_img,3,h,w) overwritten                                    */
} SfmPhotoErrorDesc;

/* Forward, one launch: err[s][b, i] as defined above for every scale s < n_scales, image i < n_img and sample b < B.
 * Reads img and tgt; ignores g_err and d_img. */
int sfm_photo_error_fwd(const SfmPhotoErrorDesc *d, void *stream);

/* Backward for the upstream gradients g_err[s], one launch:
 *   kappa_c(p) = (alpha / 3) * g_err(p) * (-1/2) * [0 < (1 - S_c) / 2 < 1]                               (F.clip backward)
 *   d_img_c(q) = ((1 - alpha) / 3) * g_err(q) * sign(X_c - Y_c)(q)                                       (sign(0) = 0)
 *              + Pool(kappa * dS/dmu_x)(q) + 2 X_c(q) * Pool(kappa * dS/dE[xx])(q) + Y_c(q) * Pool(kappa * dS/dE[xy])(q)
 * with the statistics recomputed, not stored.  The target is a constant, as everywhere in this library: it gets no gradient.
 * No atomics, no workspace: two calls on the same inputs agree bit for bit.
 * Reads img, tgt and g_err; ignores err. */
int sfm_photo_error_bwd(const SfmPhotoErrorDesc *d, void *stream);

/* Errors of both calls, checked in this order before any HIP call:
 *   d NULL -> SFM_ERR_NULL;
 *   n_img outside 1..SFM_MAX_SRC, n_scales outside 1..SFM_MAX_SCALES, B < 0, any H[s] or W[s] < 3, 3 * H[s] * W[s] >= 2^31, or
 *     2^31 or more wavefront tiles in all (a grid that would overflow) -> SFM_ERR_SHAPE;
 *   ssim_rate outside [0,1], or NaN -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned (an empty shard's pointers may be NULL);
 *   a pointer the call reads or writes is NULL -> SFM_ERR_NULL. */

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_PHOTO_ERROR_H_ */
