/*
 * sfmwarp_ext.h -- entry points of libsfmwarp.so newer than the set sfmwarp.h declares.  Same library, same conventions
 * (float32, C-contiguous, NCHW device tensors owned by the caller; 4-byte alignment; "overwritten" outputs are written completely
 * and never read; return 0, SFM_ERR_* before anything is launched, or a hipError_t; sfm_last_error() has the message) and the same
 * SFM_ABI_VERSION: nothing declared in sfmwarp.h changes.
 */
#ifndef SFMWARP_EXT_H_
#define SFMWARP_EXT_H_

#include "sfmwarp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_RESIZE_MAX_TERMS 8
/* Backward of F.resize_images (models/disp_net.py:14,105,111,117; the adjoint of the loop head models/base_model.py:70-72):
 *   gx (N,C,H,W), OVERWRITTEN  =  sum over k < n_terms of  R_k^T gy[k],   gy[k] (N,C,oH[k],oW[k]),
 * R_k = sfm_resize_fwd to (oH[k], oW[k]).  n_terms = 1: the plain backward.  n_terms = S with oH[k] = H >> k, oW[k] = W >> k:
 * the adjoint of sfm_pyramid_fwd including scale 0 (d_src[] of the fused loss -> the gradient of the full-resolution frames).
 * gy, oH, oW: HOST arrays of n_terms entries.  No atomics; the sum runs in a fixed order (k, then oy, then ox, ascending):
 * two calls on the same inputs agree bit for bit.
 * Any N*C (no grid limit), any H, W, oH[k], oW[k] >= 1; N = 0 is validated like any call, launches nothing, and its gx and gy[k] may
 * be NULL.  Errors, checked in this order before any HIP call: gy, oH or oW NULL, or gx NULL while N != 0 -> SFM_ERR_NULL; n_terms
 * outside 1..SFM_RESIZE_MAX_TERMS -> SFM_ERR_SHAPE; N < 0, C, H or W < 1 -> SFM_ERR_SHAPE; per term oH[k] or oW[k] < 1 ->
 * SFM_ERR_SHAPE, then gy[k] NULL while N > 0 -> SFM_ERR_NULL; N*C*H*W or the elements of all gy[k] together >= 2^40 -> SFM_ERR_SHAPE. */
int sfm_resize_bwd(const float *const *gy, const int *oH, const int *oW, int n_terms, float *gx,
                   int N, int C, int H, int W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_EXT_H_ */
