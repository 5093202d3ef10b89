/*
 * sfmwarp_intrinsics.h -- the gradient with respect to the camera intrinsics: entry points of libsfmwarp.so next to the sets that
 * sfmwarp.h and sfmwarp_ext.h declare.  Same library, same conventions (float32, C-contiguous device tensors owned by the caller;
 * 4-byte alignment; "overwritten" outputs are written completely and never read; return 0, SFM_ERR_* before anything is launched,
 * or a hipError_t; sfm_last_error() has the message) and the same SFM_ABI_VERSION: nothing declared in sfmwarp.h changes, and
 * SfmLossDesc is the one declared there.
 *
 * The intrinsics enter the view synthesis twice (citations into pfnet/sfm-learner-chainer): Pm = K4 . [R|t] in proj_tgt_to_src
 * (models/transform.py:86-88) and ray = K^-1 . pix through F.batch_inv in pixel2cam (:105).  With gPm = dL/dPm (rows 0..2):
 *   dL/dK = gPm[:, 0:3] . R^T + gPm[:, 3] . t^T  -  K^-T . gKinv . K^-T ,   gKinv = dL/d(K^-1) = sum over pixels of g_ray (x) pix .
 * With ONE depth per pixel (models/base_model.py:82-84) gKinv = (K R)^T . gPm[:, 0:3] . K^T, so the second term is
 * K^-T . R^T . K^T . gPm[:, 0:3]: the gradient follows from gPm alone.
 */
#ifndef SFMWARP_INTRINSICS_H_
#define SFMWARP_INTRINSICS_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fused loss: dL/dPm and dL/d(intrinsics) from the pose sums that the gradient call has left in its workspace.
 * Call it AFTER sfm_loss_bwd (loss = 0), or after sfm_loss_fwd_bwd / sfm_step_fwd_bwd (loss = 1), with the same descriptor bytes,
 * the same `ws` and `ws_bytes` on the same stream, before anything else uses `ws`.  It reads `ws`, never writes it, and may be
 * called more than once.
 *   d_proj       (B, n_scales, n_src, 3, 4), overwritten: dL/dPm, rows 0..2, of each proj_tgt_to_src call of the loop
 *                (models/base_model.py:90-94, models/transform.py:86-88); row 3 of Pm has zero gradient.
 *   d_intrinsics (B, n_scales, 3, 3), overwritten: dL/d(intrinsics[b, s]) summed over the sources: both routes above, transform.py:86-88
 *                and, through F.batch_inv, :105.
 * Either may be NULL, not both.  Both carry the gy of the gradient call (it is in the sums); with norm_B > B they are this shard's
 * additive share.
 * One launch.  The tiles of a (sample, scale, source) are folded in a fixed order in fp64, K^-1 and the products formed in fp64
 * and rounded once: two calls agree bit for bit.  The tile layout is found with the plan look-up of the gradient call (the
 * library's own choice of kernel): after a gradient call that consumed sfm_loss_variant(4) or (5) the result is UNSPECIFIED
 * (hook 3 leaves the layout alone).  B == 0 (an empty shard, whose input pointers may be NULL as for sfm_loss_bwd): only the first
 * and the third check below are made, nothing is launched.
 * Errors, checked in this order before any HIP call: desc NULL -> SFM_ERR_NULL; the descriptor rejected as by sfm_loss_bwd (its code);
 * d_proj and d_intrinsics both NULL -> SFM_ERR_NULL; ws NULL, ws_bytes below sfm_loss_workspace_bytes' layout for this call or ws off
 * the 256-byte boundary -> SFM_ERR_WORKSPACE. */
int sfm_loss_proj_bwd(const SfmLossDesc *desc, int loss, const void *ws, size_t ws_bytes, float *d_proj, float *d_intrinsics,
                      void *stream);

/* The missing output of sfm_warp_bwd: d_K (N,3,3), overwritten, the gradient of projective_inverse_warp (models/transform.py:156-193)
 * with respect to K for the upstream gradient g_warped -- through proj_tgt_to_src (:86-88) and through pixel2cam's F.batch_inv
 * (:105-107; with depth_rows = 3 the three rows of `depthes` may differ, :107).  Arguments, shapes and checks as for sfm_warp_bwd:
 * N = 0 returns at once; a NULL tensor -> SFM_ERR_NULL; N, C, H, W as there, depth_rows 1 or 3 -> SFM_ERR_SHAPE; ws NULL or shorter
 * than sfm_warp_intrinsics_bwd_workspace_bytes(N, H, W) (4-byte aligned scratch) -> SFM_ERR_WORKSPACE.
 * The pixels are re-projected in the reference's own order and dL/dq formed exactly as by sfm_warp_bwd (the same device code);
 * block sums in fp32, folded in a fixed order in fp64, the products in fp64, rounded once.  No atomics: two calls agree bit for bit. */
size_t sfm_warp_intrinsics_bwd_workspace_bytes(int N, int H, int W);
int sfm_warp_intrinsics_bwd(const float *src, const float *depth, int depth_rows, const float *pose6, const float *K,
                            const float *g_warped, float *d_K, void *ws, size_t ws_bytes, int N, int C, int H, int W, void *stream);

/* The K half of sfm_pose_proj_bwd (models/transform.py:86-88, Pm = K4 . [R|t]):
 *   pose6 (N,6), K (N,3,3), g_proj (N,4,4)  ->  d_K (N,3,3), overwritten  =  g_proj[0:3, :] . [R|t]^T   (row 3 of g_proj is not read;
 * K is not read either -- the product is linear in it -- and is taken for symmetry with sfm_pose_proj_bwd: it must not be NULL).
 * N = 0 returns at once; a NULL pointer -> SFM_ERR_NULL; N < 0 -> SFM_ERR_SHAPE. */
int sfm_pose_proj_bwd_k(const float *pose6, const float *K, const float *g_proj, float *d_K, int N, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_INTRINSICS_H_ */
