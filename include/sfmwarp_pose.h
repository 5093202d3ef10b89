/*
 * sfmwarp_pose.h -- a SIDE header of libsfmwarp.so: the two conventions of Monodepth2's code that sit INSIDE the warp kernels -- how
 * a pose becomes the rigid transform [R|t] (Euler angles, an axis-angle vector, or a 3x4 matrix handed over as it is; optionally the
 * inverse transform per source) and how a disparity becomes a depth (1 / (a * disp + b)) -- as selectable arguments of entry
 * points that otherwise are sfm_warp_pyramid_* and sfm_warp_full_res_*, plus the pose operator on its own.  It stands beside
 * include/sfmwarp.h (whose descriptors, constants and error codes it uses) for the same reason as the other four side headers: the
 * tables that pin sfmwarp.h's prototypes live in test files a feature does not edit.  FOLLOW-UP: fold SfmPoseConv into the two
 * descriptors (and _lib.POSE_SYMBOLS into _lib.SYMBOLS) at the next change of SFM_ABI_VERSION.  SFM_ABI_VERSION is unchanged here:
 * nothing that existed moved.
 *
 * Non-finite and degenerate inputs (sfmwarp.h says what every entry point guarantees on them; tests/test_hostile_inputs_gpu.py):
 * a NaN Euler angle is read as -pi (the clip is fminf(fmaxf(r, -pi), pi)) and receives the gradient 0; +-inf and 1e30 are +-pi, as
 * in the reference.  An axis-angle vector with a NaN entry gives a NaN matrix; one of 1e30 a finite one (sinf / cosf of the norm).
 * A NaN or infinite translation, or such an entry of a "matrix" pose, stays in T as it is; in the _conv_ warps every pixel of that
 * (sample, source) then has a NaN position: value 0, valid 0, and NaN in d_disp, d_pose / d_T of that sample.  Other samples keep
 * their bits.
 */
#ifndef SFMWARP_POSE_H_
#define SFMWARP_POSE_H_

#include "sfmwarp.h"
#include "sfmwarp_full_res.h"
#include "sfmwarp_conventions.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what pose[i] holds */
enum { SFM_POSE_EULER = 0, SFM_POSE_AXIS_ANGLE = 1, SFM_POSE_MATRIX = 2 };

typedef struct SfmPoseConv {
  int32_t pose_format;            /* SFM_POSE_*                                                        */
  int32_t invert[SFM_MAX_SRC];    /* 0 | 1 per source: use the inverse rigid transform                 */
  float disp_scale, disp_shift;   /* depth = 1 / (disp_scale * disp + disp_shift); (1, 0): 1 / disp    */
} SfmPoseConv;

/* ------------------------------------------------------------------------------------------
 * The pose operator: T (N,3,4) row-major = [R|t] of pose6 (N,6), one thread per matrix, and its backward for an upstream g_T (N,3,4).
 *
 * format == SFM_POSE_EULER: pose6 = (rx, ry, rz, tx, ty, tz); R = (X . Y) . Z of the angles clipped to [-pi, pi] (euler2mat /
 *   pose_vec2mat), the [R|t] behind sfm_pose_proj_fwd bit for bit.  The backward is sfm_pose_proj_bwd's behind K^T: an angle outside
 *   (-pi, pi) gets 0.
 * format == SFM_POSE_AXIS_ANGLE: pose6 = (ax, ay, az, tx, ty, tz); R is Monodepth2's rot_from_axisangle:
 *     angle = |a|,  (x, y, z) = a / (angle + 1e-7),  ca = cos angle,  sa = sin angle,  C = 1 - ca
 *     R = [[x x C + ca,  x y C - z sa,  z x C + y sa],
 *          [x y C + z sa,  y y C + ca,  y z C - x sa],
 *          [z x C - y sa,  y z C + x sa,  z z C + ca]]
 *   The angle is not clipped: sin and cos are right for any finite angle.  C is formed as sa^2 / (1 + ca) where ca > 0 (the same
 *   number without the cancellation of 1 - ca at the small angles a pose head emits).  The backward is the derivative of exactly
 *   this formula, the 1e-7 included; at a = 0 it is exactly 0.
 * invert == 1, either format: T = [R^T | -R^T t] -- R transposed, not inverted; the backward is that map's.
 * SFM_POSE_MATRIX is not a format of this operator.
 *
 * Errors, checked in this order before any HIP call: format not SFM_POSE_EULER or SFM_POSE_AXIS_ANGLE, then invert not 0 or 1 ->
 * SFM_ERR_CONFIG; N < 0 -> SFM_ERR_SHAPE; N == 0: nothing more is checked, nothing is launched, 0 is returned; a NULL pointer ->
 * SFM_ERR_NULL.  format and invert are uniform over the launch.
 * ---------------------------------------------------------------------------------------- */
int sfm_pose_mat_fwd(const float *pose6, int32_t format, int32_t invert, float *T, int N, void *stream);
int sfm_pose_mat_bwd(const float *pose6, int32_t format, int32_t invert, const float *g_T, float *d_pose6, int N, void *stream);

/* ------------------------------------------------------------------------------------------
 * sfm_warp_pyramid_* and sfm_warp_full_res_up_* with the pose and depth conventions chosen.  The descriptors are the existing ones.
 *
 * pose[i] and d_pose[i] are (B,6) for SFM_POSE_EULER and SFM_POSE_AXIS_ANGLE, and (B,3,4) row-major for SFM_POSE_MATRIX: rows 0..2
 * of T, any 3x4, not required to be rigid.
 *   EULER / AXIS_ANGLE: the lane that builds a source's geometry forms T as sfm_pose_mat_fwd does (the same device function, invert[i]
 *     honoured), then P = K . T in the operation order of the existing calls; the fold ends in sfm_pose_mat_bwd's device function.
 *   MATRIX: P = K . T with T read as given; d_pose[i] is the fold's sum K^T . gPm over the scales (3x4), nothing behind it.
 * disp_scale, disp_shift: sd = disp_scale * disp + disp_shift (a multiply, then an add: two roundings), depth = 1.0f / sd, and
 *   d_disp = (-g_depth / (sd * sd)) * disp_scale, rounded in that order.  In sfm_warp_full_res_* the map acts on the upsampled value
 *   up[s]; d_up carries the factor disp_scale before the gather.  (1, 0) takes the existing code path.
 * With c = {SFM_POSE_EULER, invert all 0, 1, 0} every call IS the existing one: the same kernels, the same bits.  The workspace
 * does not depend on c.  No launch is added: the pose work happens in the lanes that do it in the existing calls.
 *
 * Errors, checked in this order before any HIP call:
 *   everything the existing call checks up to and including image_layout (and, sfm_warp_full_res_*, upsample), with its codes;
 *   c NULL -> SFM_ERR_NULL;
 *   pose_format not one of SFM_POSE_*, invert[i] not 0 or 1 for an i < n_src, SFM_POSE_MATRIX with a non-zero invert[i] (a general
 *     3x4 has no R^T inverse: the caller inverts), disp_scale or disp_shift not finite -> SFM_ERR_CONFIG;
 *   B == 0: nothing more is checked, nothing is launched, 0 is returned;
 *   a pointer the call reads or writes is NULL -> SFM_ERR_NULL, in the order of the existing call;
 *   the backward: ws NULL, ws_bytes below the query's answer, or ws off the 256-byte boundary -> SFM_ERR_WORKSPACE.
 * The queries return 0 on anything the backward rejects; they look at no pointer.
 * ---------------------------------------------------------------------------------------- */
int sfm_warp_pyramid_conv_fwd(const SfmWarpPyramidDesc *d, const SfmPoseConv *c, void *stream);
size_t sfm_warp_pyramid_conv_bwd_workspace_bytes(const SfmWarpPyramidDesc *d, const SfmPoseConv *c);
int sfm_warp_pyramid_conv_bwd(const SfmWarpPyramidDesc *d, const SfmPoseConv *c, void *ws, size_t ws_bytes, void *stream);
int sfm_warp_full_res_conv_fwd(const SfmWarpFullResDesc *d, int32_t upsample, const SfmPoseConv *c, void *stream);
size_t sfm_warp_full_res_conv_bwd_workspace_bytes(const SfmWarpFullResDesc *d, int32_t upsample, const SfmPoseConv *c);
int sfm_warp_full_res_conv_bwd(const SfmWarpFullResDesc *d, int32_t upsample, const SfmPoseConv *c, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_POSE_H_ */
