/*
 * sfmwarp_full_res.h -- a SIDE header of libsfmwarp.so: sfm_warp_full_res_*, the "full-resolution multi-scale" warp of a
 * Monodepth2-style loss: the disparity of every scale upsampled to the input resolution INSIDE the warp of the full-resolution
 * sources.  It stands beside include/sfmwarp.h (whose conventions, constants and error codes it uses),
 * include/sfmwarp_min_reproj.h and include/sfmwarp_disp_smooth.h for the same reason as those two: the tables that pin sfmwarp.h's
 * descriptors and pointer prototypes live in test files a feature does not edit.  FOLLOW-UP: fold this section into sfmwarp.h (and
 * _lib.FULL_RES_SYMBOLS into _lib.SYMBOLS) together with those tables.  SFM_ABI_VERSION is unchanged: nothing that existed moved.
 *
 * Non-finite and degenerate inputs (sfmwarp.h, "NON-FINITE AND DEGENERATE INPUTS"; tests/test_hostile_inputs_gpu.py): the taps of
 * the in-kernel upsampling come from the pixel's coordinates, never from data.  A NaN, zero or infinite coarse disparity reaches
 * the full-resolution pixels whose bilinear footprint reads it -- a tap of weight 0 included (0 x NaN) -- and no other pixel; there
 * the operator path's rule holds (value 0 and valid 0 for a NaN position, NaN in d_disp of the footprint and in that sample's d_pose).
 * The _up_ and _conv_ forms behave alike.
 */
#ifndef SFMWARP_FULL_RES_H_
#define SFMWARP_FULL_RES_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The warp of ONE full-resolution source set with the disparity of every scale, each upsampled to that resolution.
 *
 * Definition.  For scale s with a disparity of h_s x w_s and the full resolution H x W:
 *   up[s] = disp[s]                                          where (h_s, w_s) == (H, W);
 *   up[s] = sfm_resize_fwd(disp[s] -> (H, W))                elsewhere, bit for bit (align-corners bilinear, F.resize_images).
 * warped, valid, d_up and d_pose are those of sfm_warp_pyramid_fwd / sfm_warp_pyramid_bwd, bit for bit, called with n_scales
 * scales all of size (H, W), src[s] = src, disp[s] = up[s] and intrinsics[:, s] = intrinsics, and
 *   d_disp[s] = d_up[s]                                      where (h_s, w_s) == (H, W);
 *   d_disp[s] = sfm_resize_bwd(d_up[s], n_terms = 1)         elsewhere, bit for bit.
 * No full-resolution disparity is written by the forward: a lane forms up[s] at its pixel from the four taps of disp[s].
 * ---------------------------------------------------------------------------------------- */
typedef struct SfmWarpFullResDesc {
  int32_t B, n_src, n_scales;
  int32_t H, W;                               /* the full resolution: of src, warped, valid, g_warped; each >= 3          */
  int32_t h[SFM_MAX_SCALES], w[SFM_MAX_SCALES]; /* of disp[s]: each >= 1, independent per scale (halvings not required)     */
  int32_t image_layout;                       /* SFM_LAYOUT_* of src                                                      */
  const float *src;                           /* (B,3*n_src,H,W) planar | (B,n_src,H,W,3) hwc                             */
  const float *disp[SFM_MAX_SCALES];          /* (B,1,h_s,w_s)                                                            */
  const float *intrinsics;                    /* (B,3,3): the full-resolution camera, any invertible 3x3                  */
  const float *pose[SFM_MAX_SRC];             /* (B,6)                                                                    */
  float *warped[SFM_MAX_SCALES];              /* fwd: (B,n_src,3,H,W) overwritten                                         */
  float *valid[SFM_MAX_SCALES];               /* fwd: (B,n_src,H,W) or NULL                                               */
  const float *g_warped[SFM_MAX_SCALES];      /* bwd: (B,n_src,3,H,W)                                                     */
  float *d_disp[SFM_MAX_SCALES];              /* bwd: (B,1,h_s,w_s) overwritten                                           */
  float *d_pose[SFM_MAX_SRC];                 /* bwd: (B,6) overwritten                                                   */
} SfmWarpFullResDesc;

/* Forward, one launch over the 256-pixel blocks of every (scale, sample), no workspace:
 *   warped[s][b, i] = projective_inverse_warp(source i of src[b], 1 / up[s][b], pose[i][b], intrinsics[b]);
 * valid[s], where bound (any subset of the scales), as in sfm_warp_pyramid_fwd.
 * Reads src, disp, intrinsics, pose; ignores g_warped, d_disp, d_pose. */
int sfm_warp_full_res_fwd(const SfmWarpFullResDesc *d, void *stream);

/* Backward for the upstream gradients g_warped[s], three launches:
 *   one over the full-resolution pixels of every scale, which writes the block partials of gPm and d_up[s] -- into the workspace
 *     for a resampled scale, into d_disp[s] for a scale of size (H, W);
 *   ONE for all resampled scales, one thread per element of d_disp[s], which adds the d_up[s] that reach it in ascending (oy, ox) as
 *     sfm_resize_bwd does for one term (only when some scale is resampled);
 *   the fold of one wavefront per (sample, source): per scale the block partials in a fixed order in fp64, rounded to fp32, through
 *     K^T, the scales ascending, then the pose backward -- sfm_warp_pyramid_bwd's.
 * No atomics: two calls on the same inputs agree bit for bit whatever the workspace held.  The host reads nothing from the device.
 * Reads src, disp, intrinsics, pose, g_warped; ignores warped and valid.
 * ws: sfm_warp_full_res_bwd_workspace_bytes(d) bytes of scratch on a 256-byte boundary:
 *   48 * n_src * n_scales * B * ceil(H*W / 256)  +  4 * B*H*W * (the number of scales with (h_s, w_s) != (H, W)),
 * rounded up to a multiple of 256 (256 when that is 0).  The query returns 0 on a descriptor whose sizes or layout the backward
 * rejects; it looks at no pointer.  Content undefined before and after the call. */
size_t sfm_warp_full_res_bwd_workspace_bytes(const SfmWarpFullResDesc *d);
int sfm_warp_full_res_bwd(const SfmWarpFullResDesc *d, void *ws, size_t ws_bytes, void *stream);

/* Errors of both calls, checked in this order before any HIP call:
 *   d NULL -> SFM_ERR_NULL;
 *   n_src outside 1..SFM_MAX_SRC, n_scales outside 1..SFM_MAX_SCALES, B < 0, H or W < 3, any h[s] or w[s] < 1, 3 * H * W >= 2^31,
 *     any 3 * h[s] * w[s] >= 2^31, or 2^31 or more blocks in a launch (256-pixel blocks: n_scales * B * ceil(H*W / 256); 256-element
 *     blocks of the gather: the B * h[s] * w[s] of the resampled scales together) -> SFM_ERR_SHAPE;
 *   image_layout not SFM_LAYOUT_PLANAR or SFM_LAYOUT_HWC -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned (an empty shard's pointers may be NULL);
 *   a pointer the call reads or writes is NULL (valid[s] excepted) -> SFM_ERR_NULL: intrinsics, src, then scale by scale disp[s] and
 *     warped[s] (fwd) or g_warped[s], d_disp[s] (bwd), then source by source pose[i] and, bwd, d_pose[i];
 *   sfm_warp_full_res_bwd: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE. */

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_FULL_RES_H_ */
