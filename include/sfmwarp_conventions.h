/*
 * sfmwarp_conventions.h -- a SIDE header of libsfmwarp.so: the two conventions of Monodepth2's own code that sfm_photo_error_* and
 * sfm_warp_full_res_* did not offer -- the SSIM window over the REFLECTION-padded image, and the disparity upsampled with HALF-PIXEL
 * centres (align_corners=False) -- as selectable arguments of entry points that otherwise are the existing ones.  It stands beside
 * include/sfmwarp.h (whose descriptors, constants and error codes it uses) and include/sfmwarp_full_res.h for the same reason as
 * the other side headers: the tables that pin sfmwarp.h's prototypes live in test files a feature does not edit.  FOLLOW-UP: fold
 * the two arguments into the descriptors of sfmwarp.h (and _lib.CONV_SYMBOLS into _lib.SYMBOLS) together with those tables, at the
 * next change of SFM_ABI_VERSION.  SFM_ABI_VERSION is unchanged here: nothing that existed moved.
 */
#ifndef SFMWARP_CONVENTIONS_H_
#define SFMWARP_CONVENTIONS_H_

#include "sfmwarp.h"
#include "sfmwarp_full_res.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the padding of the 3x3 SSIM window */
enum { SFM_SSIM_PAD_ZERO = 0, SFM_SSIM_PAD_REFLECT = 1 };
/* where the samples of a low-resolution disparity sit */
enum { SFM_UPSAMPLE_ALIGN_CORNERS = 0, SFM_UPSAMPLE_HALF_PIXEL = 1 };

/* ------------------------------------------------------------------------------------------
 * sfm_photo_error_fwd / sfm_photo_error_bwd with the padding of the SSIM window chosen.
 *
 * padding == SFM_SSIM_PAD_ZERO: the existing calls -- the same kernels, the same bits.
 * padding == SFM_SSIM_PAD_REFLECT: the same formula with every 3x3 average taken over the image extended by one pixel of
 *   reflection (torch.nn.ReflectionPad2d(1) followed by AvgPool2d(3, 1)): row -1 is row 1, row H is row H-2, the columns likewise,
 *   so every window holds nine real values.  The backward is the adjoint of "pad, then pool": what the second pooling sends to a
 *   padded row or column is added to the row or column it mirrors.  The L1 term does not look at the padding.
 * One launch each, no workspace, no atomics, no LDS, every output element written once, as the existing calls.
 *
 * Errors, checked in this order before any HIP call:
 *   everything sfm_photo_error_* checks up to and including ssim_rate, with its codes (d NULL -> SFM_ERR_NULL; n_img, n_scales,
 *     B, H, W, the grid -> SFM_ERR_SHAPE; ssim_rate outside [0,1] -> SFM_ERR_CONFIG).  One difference: sfm_photo_error_* refuse a
 *     frame below 3 x 3, and so do these calls for every padding but SFM_SSIM_PAD_REFLECT, for which this group asks H, W >= 1 only;
 *   padding not SFM_SSIM_PAD_ZERO or SFM_SSIM_PAD_REFLECT -> SFM_ERR_CONFIG;
 *   SFM_SSIM_PAD_REFLECT and any H[s] or W[s] below 2 (reflection needs a second row and column, and no more) -> SFM_ERR_SHAPE;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned;
 *   a pointer the call reads or writes is NULL -> SFM_ERR_NULL, scale by scale as in sfm_photo_error_*.
 * ---------------------------------------------------------------------------------------- */
int sfm_photo_error_pad_fwd(const SfmPhotoErrorDesc *d, int32_t padding, void *stream);
int sfm_photo_error_pad_bwd(const SfmPhotoErrorDesc *d, int32_t padding, void *stream);

/* ------------------------------------------------------------------------------------------
 * sfm_warp_full_res_fwd / _bwd with the upsampling of the disparities chosen.
 *
 * upsample == SFM_UPSAMPLE_ALIGN_CORNERS: the existing calls -- the same kernels, the same bits.
 * upsample == SFM_UPSAMPLE_HALF_PIXEL: up[s] of a scale with (h_s, w_s) != (H, W) is
 *   torch.nn.functional.interpolate(disp[s], (H, W), mode="bilinear", align_corners=False), stated in float32 without contraction:
 *     scale_u = (float)w / (float)W                      formed on the host
 *     u   = max(scale_u * (x + 0.5f) - 0.5f, 0)
 *     u0  = min(floor(u), w - 1),  u1 = min(u0 + 1, w - 1),  wu1 = u - u0,  wu0 = 1 - wu1
 *   v likewise, and the blend of sfm_resize_fwd: (a0 wu0 + a1 wu1) wv0 + (b0 wu0 + b1 wu1) wv1.  A scale of size (H, W) is used as
 *   it is.  warped, valid, d_up, the block partials and the fold are those of sfm_warp_full_res_* on these up[s], bit for bit;
 *   d_disp[s] of a resampled scale is the adjoint of that upsampling: per element the contributions d_up * (wv * wu) in ascending
 *   (oy, ox), the weights of an axis' two taps summed first where both land on the element; an element no output touches (a
 *   disparity larger than the full resolution) gets exactly 0.  Still one launch for all resampled scales, no atomics.
 * The workspace of the backward is that of sfm_warp_full_res_bwd for either value.
 *
 * Errors, checked in this order before any HIP call:
 *   everything sfm_warp_full_res_* checks up to and including image_layout, with its codes;
 *   upsample not SFM_UPSAMPLE_ALIGN_CORNERS or SFM_UPSAMPLE_HALF_PIXEL -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned;
 *   a pointer the call reads or writes is NULL -> SFM_ERR_NULL, in the order of sfm_warp_full_res_*;
 *   sfm_warp_full_res_up_bwd: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE.
 * The query returns 0 on a descriptor or an upsample value the backward rejects; it looks at no pointer.
 * ---------------------------------------------------------------------------------------- */
int sfm_warp_full_res_up_fwd(const SfmWarpFullResDesc *d, int32_t upsample, void *stream);
size_t sfm_warp_full_res_up_bwd_workspace_bytes(const SfmWarpFullResDesc *d, int32_t upsample);
int sfm_warp_full_res_up_bwd(const SfmWarpFullResDesc *d, int32_t upsample, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_CONVENTIONS_H_ */
