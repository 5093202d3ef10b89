/*
 * sfmwarp_depth_consistency.h -- a SIDE header of libsfmwarp.so: the geometry-consistency term of SC-SfMLearner (Bian et al.,
 * NeurIPS 2019) on this library's own warp.  For every scale, source and target pixel it compares the depth of the target pixel's
 * 3-D point seen from the source camera (the COMPUTED depth) with the source frame's own depth prediction sampled where that point
 * lands (the PROJECTED depth), differentiably with respect to both disparity maps and the pose.  It stands beside include/sfmwarp.h
 * (whose constants and error codes it uses) and include/sfmwarp_pose.h (whose conventions it takes) for the same reason as the other
 * five side headers: the tables that pin sfmwarp.h's prototypes live in test files a feature does not edit.  FOLLOW-UP: fold this
 * header (and _lib.DEPTH_CONS_SYMBOLS into _lib.SYMBOLS) into sfmwarp.h at the next change of SFM_ABI_VERSION.  SFM_ABI_VERSION is
 * unchanged here: nothing that existed moved.
 *
 * What it restates of SC-SfMLearner, by function name (formulas quoted, no code taken):
 *   inverse_warp2:          computed_depth = Z.clamp(min=1e-3) of the 3-D point in the source camera;
 *                           projected_depth = grid_sample(ref_depth, pixel coordinates, padding_mode="zeros");
 *                           valid_mask = the sampling position lies inside the view in both coordinates.
 *   compute_pairwise_loss:  diff_depth = ((computed_depth - projected_depth).abs() / (computed_depth + projected_depth)).clamp(0, 1);
 *                           weight_mask = 1 - diff_depth (the self-discovered mask); the geometry loss is the mean of diff_depth
 *                           over valid_mask.  The mean and the weighting are sfm_pairwise_* (include/sfmwarp_pairwise.h).
 *
 * Non-finite and degenerate inputs (sfmwarp.h, "NON-FINITE AND DEGENERATE INPUTS"; tests/test_hostile_inputs_gpu.py): positions are
 * those of sfm_warp_pyramid_*, so a pixel whose projected position is NaN has diff 0 and valid 0, nothing is scattered for it, and
 * d_disp of the pixel and that sample's d_pose / d_T are NaN; `computed` is fmaxf(q2, 1e-3), which turns a NaN q2 into 1e-3.  Other
 * pixels' maps and other samples keep their bits.
 */
#ifndef SFMWARP_DEPTH_CONSISTENCY_H_
#define SFMWARP_DEPTH_CONSISTENCY_H_

#include "sfmwarp.h"
#include "sfmwarp_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SfmDepthConsDesc {
  int32_t B, n_src, n_scales;
  int32_t H[SFM_MAX_SCALES], W[SFM_MAX_SCALES];     /* independent per scale */
  const float *disp[SFM_MAX_SCALES];                /* (B,1,h,w)      target disparity                     */
  const float *src_disp[SFM_MAX_SCALES];            /* (B,n_src,h,w)  the sources' own disparities         */
  const float *intrinsics;                          /* (B,n_scales,3,3) */
  const float *pose[SFM_MAX_SRC];                   /* (B,6) | (B,3,4) with SFM_POSE_MATRIX */
  float *diff[SFM_MAX_SCALES];                      /* fwd: (B,n_src,h,w) overwritten */
  float *valid[SFM_MAX_SCALES];                     /* fwd: (B,n_src,h,w) or NULL */
  float *computed[SFM_MAX_SCALES], *projected[SFM_MAX_SCALES];   /* fwd: (B,n_src,h,w) or NULL, scale by scale */
  const float *g_diff[SFM_MAX_SCALES];              /* bwd: (B,n_src,h,w) */
  float *d_disp[SFM_MAX_SCALES];                    /* bwd: (B,1,h,w) overwritten */
  float *d_src_disp[SFM_MAX_SCALES];                /* bwd: (B,n_src,h,w) overwritten, or NULL: not computed */
  float *d_pose[SFM_MAX_SRC];                       /* bwd: overwritten */
} SfmDepthConsDesc;

/* ------------------------------------------------------------------------------------------
 * c == NULL means the defaults of include/sfmwarp_pose.h: SFM_POSE_EULER, no inversion, depth = 1 / disp.  All arithmetic is float32
 * without fused multiply-adds, in the order written here.
 *
 * FORWARD: one launch, one thread per target pixel, which loops over the sources.  Per (scale s, sample b, source i, pixel (x, y)):
 *   sd = disp_scale * disp + disp_shift (disp itself under (1, 0)),  depth = 1.0f / sd
 *   the projection, the sampling position, the four taps with their weights and `valid` are those of sfm_warp_pyramid_conv_fwd for
 *     the same pose, intrinsics, disparity and conventions, bit for bit (the same device functions)
 *   q2 = ((Pm[2][0] c0 + Pm[2][1] c1) + Pm[2][2] c2) + Pm[2][3], c = depth * (K^-1 . (x, y, 1)): the third component of Pm . c4 as the
 *     projection forms it, before its + 1e-10
 *   computed  = fmaxf(q2, 1e-3f)                                inverse_warp2's Z.clamp(min=1e-3).  This is the depth in the source
 *                                                               camera whenever the third row of K is (0, 0, 1).
 *   projected = ((w1 x1 + w2 x2) + w3 x3) + w4 x4               the sampler's blend with x[k] = 1.0f / (disp_scale * src_disp[tap k] +
 *     disp_shift) for a tap inside the image and exactly 0 on the one-pixel zero frame: the bilinear sample of the source's DEPTH
 *     map, bit for bit sfm_warp_fwd on the one-channel image 1 / sd_src
 *   valid     = both normalised coordinates strictly inside (-1, 1) ? 1 : 0
 *   diff      = valid ? fabsf(computed - projected) / (computed + projected) : 0
 *   A valid pixel has all four taps inside the image, so for positive disparities the denominator is at least 1e-3 and diff lies in
 *   [0, 1): compute_pairwise_loss's clamp(0, 1) never acts and is left out.  Every bound output element is written.
 *
 * BACKWARD for g_diff: one launch over the pixels, then a fold of one wavefront per (sample, source), exactly as
 * sfm_warp_pyramid_conv_bwd: block sums of the 12 entries of gPm, a fixed-order fp64 sum of them per scale, rounded to float32 and
 * taken through K_s^T, the scales added in ascending order, then the pose backward of the chosen convention.  Per valid pixel, with
 * g = g_diff, sgn = sign(computed - projected) (0 at equality) and den = computed + projected, the rounding order is
 *   dd  = den * den
 *   f_c = sgn * ((2 projected) / dd)        f_p = -(sgn * ((2 computed) / dd))
 *   g_c = g * f_c                           g_p = g * f_p
 *   gq  = f_p * (dL/dq of sfm_warp_bwd for the one-channel image 1 / sd_src and the upstream value g)     (that chain is linear in
 *         its upstream value; f_p multiplies its three results)
 *   gq[2] += g_c  where q2 > 1e-3f          the clamp's derivative
 *   then g_depth and the 12 gPm terms as in sfm_warp_bwd;  d_disp = (-(sum over the sources, ascending, of g_depth) / (sd sd))
 *   [* disp_scale].  An invalid pixel contributes exact zeros everywhere.
 *   d_src_disp[tap k] += (-(g_p w_k) / (sd_k sd_k)) [* disp_scale] for the up to four taps inside the image, w_k the blend's weight
 *   products, added with float atomics.  The call first zeroes every bound d_src_disp[s] with a memset on the stream, so the whole
 *   call can be captured in a graph.  d_src_disp[s] == NULL for EVERY s selects kernels without the scatter; a scale whose entry is
 *   NULL while another's is bound is skipped.
 *
 * diff, valid, computed, projected, d_disp and d_pose are bitwise reproducible: no atomics, fixed orders, whatever the workspace
 * held.  d_src_disp is NOT: the order in which the atomic adds arrive varies from call to call.
 *
 * Errors, checked in this order before any HIP call:
 *   d NULL -> SFM_ERR_NULL;
 *   n_src not in 1..SFM_MAX_SRC, n_scales not in 1..SFM_MAX_SCALES, B < 0, an H or W below 3, 3*H*W or the number of 256-pixel
 *     blocks of all scales at or above 2^31 -> SFM_ERR_SHAPE;
 *   c not NULL: pose_format not one of SFM_POSE_*, invert[i] not 0 or 1 for an i < n_src, SFM_POSE_MATRIX with a non-zero invert[i],
 *     disp_scale or disp_shift not finite -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned;
 *   a pointer the call reads or writes is NULL -> SFM_ERR_NULL: intrinsics, then per scale disp, src_disp and (fwd) diff or (bwd)
 *     g_diff, d_disp, then per source pose and (bwd) d_pose.  valid, computed, projected and d_src_disp are optional;
 *   the backward: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE.
 * The workspace is (blocks of all scales and samples) * n_src * 12 floats, rounded up to 256 bytes, the rule of
 * sfm_warp_pyramid_bwd; its content on entry does not matter.  The query looks at no pointer and returns 0 on what the backward
 * rejects.
 * ---------------------------------------------------------------------------------------- */
int    sfm_depth_consistency_fwd(const SfmDepthConsDesc *d, const SfmPoseConv *c, void *stream);
size_t sfm_depth_consistency_bwd_workspace_bytes(const SfmDepthConsDesc *d, const SfmPoseConv *c);
int    sfm_depth_consistency_bwd(const SfmDepthConsDesc *d, const SfmPoseConv *c, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_DEPTH_CONSISTENCY_H_ */
