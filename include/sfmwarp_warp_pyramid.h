/*
 * sfmwarp_warp_pyramid.h -- the differentiable warp of the whole source pyramid of one step: entry points of libsfmwarp.so next to
 * the sets that sfmwarp.h, sfmwarp_ext.h and sfmwarp_intrinsics.h declare.  Same library, same conventions (float32, C-contiguous
 * device tensors owned by the caller; 4-byte alignment; "overwritten" outputs are written completely and never read; return 0,
 * SFM_ERR_* before anything is launched, or a hipError_t; sfm_last_error() has the message) and the same SFM_ABI_VERSION: nothing
 * declared in the other headers changes.
 *
 * What it is for: a loss of the caller's own on the warped images -- a per-pixel minimum over the sources, auto-masking, a robust
 * penalty, a feature loss -- with the gradient back through the warp.  The fused loss (sfm_loss_*) hands the warped images out
 * (SfmLossDesc.warped) but takes no upstream gradient for them; sfm_warp_fwd / sfm_warp_bwd take one, for ONE (scale, source) per
 * call.  These calls warp every scale and every source of a step in ONE launch (models/base_model.py:81-94 for all s and i) and
 * differentiate them in ONE launch plus a small fold, from the inputs sfm_loss_* takes.
 *
 * Per pixel it is sfm_warp_fwd / sfm_warp_bwd with depth_rows = 1 and depth = 1 / disp (models/base_model.py:60; the correctly
 * rounded quotient): the same device code in the reference's own evaluation order (models/transform.py:94-133,189), hence
 *   warped[s][:, i] == sfm_warp_fwd(src[s][:, 3i:3i+3], 1 / disp[s], pose[i], intrinsics[:, s])   bit for bit, in both image layouts.
 */
#ifndef SFMWARP_WARP_PYRAMID_H_
#define SFMWARP_WARP_PYRAMID_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SfmWarpPyramidDesc {
  int32_t B, n_src, n_scales;
  int32_t H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];
  int32_t image_layout;                       /* SFM_LAYOUT_* of src[]                        */
  const float *src[SFM_MAX_SCALES];           /* (B,3*n_src,h,w) planar | (B,n_src,h,w,3) hwc */
  const float *disp[SFM_MAX_SCALES];          /* (B,1,h,w)                                    */
  const float *intrinsics;                    /* (B,n_scales,3,3), any invertible 3x3         */
  const float *pose[SFM_MAX_SRC];             /* (B,6)                                        */
  float *warped[SFM_MAX_SCALES];              /* fwd: (B,n_src,3,h,w) overwritten             */
  float *valid[SFM_MAX_SCALES];               /* fwd: (B,n_src,h,w) or NULL                   */
  const float *g_warped[SFM_MAX_SCALES];      /* bwd: (B,n_src,3,h,w)                         */
  float *d_disp[SFM_MAX_SCALES];              /* bwd: (B,1,h,w) overwritten                   */
  float *d_pose[SFM_MAX_SRC];                 /* bwd: (B,6) overwritten                       */
} SfmWarpPyramidDesc;

/* Forward, one launch: warped[s][b, i] = projective_inverse_warp(source i of src[s][b], 1 / disp[s][b], pose[i][b],
 * intrinsics[b, s]) for every scale s < n_scales, source i < n_src and sample b < B; planar in both image layouts (the layout of
 * SfmLossDesc.warped), exactly 0 where the sample is not in view.
 * valid[s], where bound (any subset of the scales), overwritten: 1.0f where both strict tests of models/transform.py:129 hold
 * (-1 < xn < 1 and -1 < yn < 1), else 0.0f -- 0 implies that the three warped channels are exactly 0.
 * Reads src, disp, intrinsics, pose; ignores g_warped, d_disp, d_pose. */
int sfm_warp_pyramid_fwd(const SfmWarpPyramidDesc *d, void *stream);

/* Backward for the upstream gradients g_warped[s], one launch over the pixels plus a fold of one wavefront per (sample, source):
 *   d_disp[s] = -(sum over i, ascending, of source i's d_depth as sfm_warp_bwd forms it with depth_rows = 1) / (disp * disp),
 *               written once per pixel;
 *   d_pose[i] = the pose backward of  sum over s, ascending, of  K_s^T . gPm[s, i]  (models/transform.py:43-91 backward), gPm[s, i]
 *               the sum of that scale's block partials in a fixed order in fp64, rounded to fp32.
 * No atomics: two calls on the same inputs agree bit for bit.  No gradient for the source images or the intrinsics
 * (sfm_warp_bwd's d_src and sfm_warp_intrinsics_bwd provide those per scale and source).
 * Reads src, disp, intrinsics, pose, g_warped; ignores warped and valid.
 * ws: sfm_warp_pyramid_bwd_workspace_bytes(d) bytes of scratch on a 256-byte boundary (0 on a descriptor the backward rejects; a
 * multiple of 256; 48 bytes per 256-pixel block and source).  Content undefined before and after the call. */
size_t sfm_warp_pyramid_bwd_workspace_bytes(const SfmWarpPyramidDesc *d);
int sfm_warp_pyramid_bwd(const SfmWarpPyramidDesc *d, void *ws, size_t ws_bytes, void *stream);

/* Errors of both calls, checked in this order before any HIP call:
 *   d NULL -> SFM_ERR_NULL;
 *   n_src outside 1..SFM_MAX_SRC, n_scales outside 1..SFM_MAX_SCALES, B < 0, any H[s] or W[s] < 3, 3 * H[s] * W[s] >= 2^31, or
 *     2^31 or more 256-pixel blocks in all -> SFM_ERR_SHAPE;
 *   image_layout not SFM_LAYOUT_PLANAR or SFM_LAYOUT_HWC -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned (an empty shard's pointers may be NULL);
 *   a pointer the call reads or writes is NULL (valid[s] excepted) -> SFM_ERR_NULL;
 *   sfm_warp_pyramid_bwd: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE.
 * The pixel-interleaved layout needs no frame-size limit of its own here (sfm_loss_* forms a tap's byte offset in fp32 and is limited
 * to 2^24 / 12 pixels per image; these kernels form it in integers). */

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_WARP_PYRAMID_H_ */
