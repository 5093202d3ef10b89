/*
 * sfmwarp.h -- C ABI of libsfmwarp.so: the MI355X (gfx950) implementation of SfM-Learner's
 * photometric view-synthesis loss path.
 *
 * Every entry point replaces a piece of pfnet/sfm-learner-chainer (citations are
 * file:line into that repository).  Conventions:
 *
 *   - all tensors are float32, C-contiguous, NCHW, resident in device (HBM) memory and owned
 *     by the caller; the library never allocates, frees or keeps a pointer after return;
 *   - alignment: 4 bytes (that of a float) suffices for every tensor, input or output, each scale and each pose on its own -- a
 *     contiguous view into a larger array (a batch shard `a[lo:hi]`) is as good as an allocation of its own, with the same results
 *     bit for bit; where a kernel has a 16-byte path it tests the addresses itself.  The one exception is the scratch `ws` of
 *     sfm_loss_* / sfm_step_*: 256 bytes (see there);
 *   - memory written: an output marked "overwritten" is written completely, whatever it held (it is never read); one marked
 *     ACCUMULATED is added to; inputs are only read; scratch (`ws`) may hold anything before the call and holds nothing of use
 *     after it -- no result depends on its previous content; nothing outside the outputs and `ws_bytes` of `ws` is written.  A call
 *     that returns SFM_ERR_* has launched nothing and written nothing;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call is
 *     asynchronous with respect to the host, re-entrant, and keeps no global mutable state
 *     (the reference's module globals `filler` / `meshgrid`, models/transform.py:62,135, are
 *     deliberately not reproduced).  Per THREAD the library remembers the launch plans of the last
 *     four distinct (descriptor bytes, device, entry point) combinations of sfm_loss_*: host-side
 *     integers only, no device memory, never a pointer that is used without being passed in again;
 *   - image values: the reference's input contract is uint8 / 127.5 - 1, i.e. [-1, 1]
 *     (datasets/kitti/kitti_raw_dataset.py:12-14).  Warp, zero mask (models/base_model.py:96), L1 and smoothness hold for finite
 *     images of any range.  The SSIM terms (models/base_model.py:126-142) form variances as E[x^2] - mu^2 in fp32, as the
 *     reference does: beyond a range of about +-16 those cancel, SSIM's denominator can reach 0, and where the reference's
 *     F.clip backward then yields a zero gradient this library may yield a non-finite one (the loss scalars stay right).
 *     A NaN anywhere in an image makes the loss NaN, as in the reference.  Image values are taken to be zero or NORMAL
 *     floats: the zero mask of models/base_model.py:96 is formed as clamp(max_c |I^_c| * 2^127, 0, 1), which is exactly 0 / 1 for those
 *     and a fraction of 1 for a pixel whose three warped channels are all subnormal (|.| < 1.2e-38; uint8 / 127.5 - 1 has none);
 *   - NON-FINITE AND DEGENERATE INPUTS (a disparity, depth, pose, intrinsics or grid entry that is NaN, +-inf, 0, negative,
 *     denormal or 1e+-30; an upstream gradient that is NaN or inf).  Every entry point of this header and of sfmwarp_pose.h,
 *     sfmwarp_full_res.h, sfmwarp_depth_consistency.h terminates, returns 0 and reads and writes inside its arrays on them
 *     (profiles/hostile_inputs_audit.md lists every place where such a number becomes an address, with its guard); what one sample
 *     holds never changes a bit of another sample's outputs, and a hostile disparity changes the forward outputs of its own pixel
 *     only (sfm_warp_full_res_*: of the pixels whose upsampling reads it); every call gives the same bits twice (the outputs
 *     accumulated with atomics: the same finite / inf / NaN pattern).  tests/test_hostile_inputs_gpu.py pins all of it.  The values:
 *       * sfm_sampler_*, and the sampler inside sfm_warp_*, sfm_warp_pyramid_*, sfm_warp_full_res_*, sfm_depth_consistency_*: the
 *         padded position is clamped with fminf(fmaxf(.)), so a NaN grid coordinate is clamped to the first column / row of the zero
 *         frame -- the sample is exactly 0 and its ggrid component 0 where the reference's formula (np.clip keeps a NaN) gives NaN; a
 *         position that is +-inf or beyond the int range is clipped to the frame like any position outside, as in the reference.
 *         sfm_sampler_interp_*: a NaN coordinate takes the first column / row with NaN weights (y, and the ggrid formed with them, NaN).
 *       * operator path (sfm_warp_*, sfm_warp_pyramid_*, sfm_warp_full_res_*, sfm_depth_consistency_*): a pixel whose projected
 *         position is NaN (a NaN or zero disparity, a NaN depth, a NaN or infinite translation, a NaN or singular K) has the value 0
 *         and valid 0, but its dL/dq = 0 / z is NaN: d_depth / d_disp of that pixel and ALL of that sample's d_pose, d_T and d_K for
 *         that source are NaN.  Zero disparity is depth +inf: out of view (a NaN position wherever the ray has a zero component).
 *       * Euler poses everywhere (sfm_pose_proj_*, sfm_pose_mat_*, the warps, the fused loss): the clip of transform.py:23 is
 *         fminf(fmaxf(r, -pi), pi): a NaN Euler angle is read as -pi, and its own gradient is 0 (the clip's backward); an angle of
 *         +-inf or 1e30 is +-pi, as in the reference.  sfm_pose_proj_fwd: row 3 of the output is written as (0, 0, 0, 1) whatever the
 *         pose (the reference's 0 x NaN there is NaN).  An axis-angle vector with a NaN entry gives a NaN matrix, as the formula does.
 *       * fused loss (sfm_loss_*, sfm_step_*), both projections: a sample whose position is not finite is NOT IN VIEW -- no tap of
 *         it is addressed, it receives and contributes no gradient through the sampler.  If the position is NaN, in the planar layout
 *         its warped value is exactly 0; in the pixel-interleaved layout it is NaN (the zero taps are blended with NaN fractions), and
 *         then pixel_loss and total_loss are NaN (ssim_loss is not: the zero mask counts the pixel as masked) -- the planar layout
 *         swallows it, as the clamped sampler does.  The kernel families and entry points of one layout and projection agree on the
 *         class (finite / inf / NaN) of every output element and on the exactly-zero set of warped; so do the two projections, except
 *         for an infinite disparity (below).  d_disp of the
 *         pixel, and d_pose of every source of that sample, are NaN in both layouts; beyond that the class of the gradients around a
 *         hostile disparity is a property of each formula (the sign of a NaN difference is taken as +-1, the SSIM window spreads a NaN
 *         warped value in the pixel-interleaved layout): the launches of a layout agree on it, the reference's formula need not.
 *         A non-finite POSE entry is NOT reported by the fused loss, where the reference's loss and d_pose are NaN: a NaN angle is
 *         -pi to every kernel -- every output is finite, the angle's own gradient 0 --, and a NaN or infinite translation puts every
 *         pixel of that source at a NaN position (planar: the source contributes exact zeros and the scalars stay finite;
 *         pixel-interleaved: NaN as above; d_disp of that sample is NaN in both).
 *         an infinite disparity is depth 0 in the default projection and a NaN depth under SFM_PROJECTION_REFERENCE_ORDER (its 1 / disp
 *         carries a residual correction: 0 x inf); the smoothness terms of a stencil that holds an infinite disparity are NaN
 *         (inf - inf) where the reference's order of differences gives +inf.
 *       * a singular or NaN K makes K^-1 non-finite: every pixel of that (sample, scale) is as above.
 *     WHAT A CALLER MUST CHECK ITSELF: the poses (a NaN angle leaves no trace in any output); and, in the planar layout, the
 *     disparities -- it can return a finite loss for a NaN or zero disparity (the gradients are then NaN: torch.isfinite on d_disp /
 *     d_pose, or a GradScaler, sees it).  Nothing validates inputs on the device, because that would synchronise;
 *   - return value: 0 on success; SFM_ERR_* (<0) for a rejected argument; a positive value is
 *     a hipError_t from the launch.  sfm_last_error() returns a thread-local message.
 *     No exception or abort crosses the ABI.
 */
#ifndef SFMWARP_H_
#define SFMWARP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_ABI_VERSION 6

#define SFM_OK 0
#define SFM_ERR_NULL (-1)      /* a required pointer is NULL                       */
#define SFM_ERR_SHAPE (-2)     /* a dimension is out of the supported range        */
#define SFM_ERR_CONFIG (-3)    /* inconsistent loss configuration                  */
#define SFM_ERR_WORKSPACE (-4) /* workspace missing, too small or misaligned         */

#define SFM_MAX_SCALES 8
#define SFM_MAX_SRC 8

int sfm_abi_version(void);
const char *sfm_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Pose -> projection.  proj_tgt_to_src(), models/transform.py:64-91 (euler2mat :11-40,
 * pose_vec2mat :43-59), kept on the device (the reference hops to the CPU, :76-80,89-90).
 *   pose6 (N,6) rx,ry,rz,tx,ty,tz ; K (N,3,3)  ->  proj (N,4,4) = [[K,0],[0,1]] . [[R,t],[0,1]]
 * Backward: g_proj (N,4,4) -> d_pose6 (N,6) (overwritten).
 * ---------------------------------------------------------------------------------------- */
int sfm_pose_proj_fwd(const float *pose6, const float *K, float *proj, int N, void *stream);
int sfm_pose_proj_bwd(const float *pose6, const float *K, const float *g_proj, float *d_pose6, int N,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * projective_inverse_warp(imgs, depthes, poses, K), models/transform.py:156-193
 * (pixel2cam :94-109, cam2pixel :111-133 incl. the x2 rule :128-131, and the
 * F.spatial_transformer_sampler call :189).
 *   src (N,C,H,W) ; depth (N,depth_rows,H*W) ; pose6 (N,6) ; K (N,3,3)  ->  warped (N,C,H,W).
 *   depth_rows = 3: the reference's `depthes` (N,3,H*W), one depth per camera coordinate (:107);
 *   depth_rows = 1: ONE row of it, for the case the caller knows the three rows are the
 *   broadcast of models/base_model.py:82-84 (d_depth is then the sum over the three rows).
 * Backward for an upstream gradient g_warped (N,C,H,W):
 *   d_depth (N,depth_rows,H*W) overwritten
 *   d_pose6 (N,6)     overwritten
 *   d_src   (N,C,H,W) or NULL; ACCUMULATED into (zero it first) with float atomics
 *   ws: sfm_warp_bwd_workspace_bytes(N,H,W) bytes of scratch (4-byte aligned; fewer bytes: SFM_ERR_WORKSPACE).
 * H, W >= 3 (below that the reference's x2 rule no longer implies zero fill).
 * ---------------------------------------------------------------------------------------- */
int sfm_warp_fwd(const float *src, const float *depth, int depth_rows, const float *pose6, const float *K,
                 float *warped, int N, int C, int H, int W, void *stream);
size_t sfm_warp_bwd_workspace_bytes(int N, int H, int W);
int sfm_warp_bwd(const float *src, const float *depth, int depth_rows, const float *pose6, const float *K,
                 const float *g_warped, float *d_depth, float *d_pose6, float *d_src, void *ws,
                 size_t ws_bytes, int N, int C, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * F.spatial_transformer_sampler(x, grid) as called at models/transform.py:189 (Chainer
 * built-in): normalized grid (N,2,oH,oW) with [:,0]=x, [:,1]=y in [-1,1]; bilinear; the image
 * is zero-padded by one pixel and coordinates are clipped to the padded image.
 *   fwd: x (N,C,H,W), grid -> y (N,C,oH,oW)
 *   bwd: gy -> ggrid (N,2,oH,oW) overwritten ; gx (N,C,H,W) or NULL, ACCUMULATED (atomics)
 * ---------------------------------------------------------------------------------------- */
int sfm_sampler_fwd(const float *x, const float *grid, float *y, int N, int C, int H, int W, int oH, int oW,
                    void *stream);
int sfm_sampler_bwd(const float *x, const float *grid, const float *gy, float *ggrid, float *gx, int N,
                    int C, int H, int W, int oH, int oW, void *stream);

/* ------------------------------------------------------------------------------------------
 * SpatialTransformerSamplerInterp, models/spational_transformer_sampler_interp.py:9-159:
 * grid in PIXEL coordinates; weights formed after clipping the taps (:46-55), so the result is
 * exactly 0 outside [0,W-1) x [0,H-1); backward returns ggrid (:129-147) and gx == 0 (:148).
 *   fwd: _forward :32-78 ; bwd: _backward :86-149 (gx, if not NULL, is zero-filled).
 * ---------------------------------------------------------------------------------------- */
int sfm_sampler_interp_fwd(const float *x, const float *grid, float *y, int N, int C, int H, int W, int oH,
                           int oW, void *stream);
int sfm_sampler_interp_bwd(const float *x, const float *grid, const float *gy, float *ggrid, float *gx,
                           int N, int C, int H, int W, int oH, int oW, void *stream);

/* ------------------------------------------------------------------------------------------
 * The fused multi-scale loss: the loop of SFMLearner.__call__, models/base_model.py:69-124,
 * from the image pyramid onwards -- depth = 1/disp (:60), projective_inverse_warp (:90-94),
 * L1 + zero mask (:95-100,:111), SSIM (:112-115, compute_ssim :126-142), smoothness
 * (:75-77 compute_smooth_loss :169-185, or the edge-aware compute_disp_smooth :144-155 that
 * the reference leaves commented out at :78-80), explainability (:103-109, :157-167) and the
 * assembly of the five reported scalars (:117-123).
 * ---------------------------------------------------------------------------------------- */
#define SFM_SMOOTH_NONE 0
#define SFM_SMOOTH_SECOND_ORDER 1 /* base_model.py:169-185 (the live one) */
#define SFM_SMOOTH_EDGE_AWARE 2   /* base_model.py:144-155                */

/* Memory layout of the image pyramids handed to sfm_loss_* (tgt[s], src[s]):
 *   SFM_LAYOUT_PLANAR  the reference's: tgt (B,3,h,w), src (B,3*n_src,h,w)   (base_model.py:71-72)
 *   SFM_LAYOUT_HWC     pixel-interleaved: tgt (B,h,w,3), src (B,n_src,h,w,3) -- what sfm_pyramid_hwc_fwd writes.
 * Same values, same results (bit for bit); HWC lets the kernel fetch the three channels of a tap with one
 * 12-byte load (6 instead of 10 vector loads per pixel row) and is the layout the fused loss runs fastest on.
 * Disparities, masks and every gradient output (d_src included) are planar in both cases. */
#define SFM_LAYOUT_PLANAR 0
#define SFM_LAYOUT_HWC 1

/* How the fused kernels evaluate the per-pixel projection of projective_inverse_warp (models/transform.py:94-133,189).  (ABI v5)
 * Both take the pose -> projection products of proj_tgt_to_src and batch_inv in the reference's own roundings
 * (R = (X . Y) . Z, K4 . T and adj(K) / det as separate multiplies, adds and correctly rounded quotients: transform.py:11-91,105).
 *   SFM_PROJECTION_FAST             q = D (M . pix) + P[:,3] with M = P[:, :3] . K^-1 folded once per wavefront; the strict in-view
 *                                   test of transform.py:129 on U = q0 / z directly and the sample taken at (U, V).  16 vector
 *                                   instructions per pixel row.  GUARANTEES: the five loss scalars to 1e-4 relative; the warped pixels
 *                                   within 1e-4 of the image range of the reference's up to 128 x 416 frames; at 256 x 832, where one
 *                                   ulp of a sampling position is 6e-5 px, within 2e-4 with fewer than 0.01 % of the pixels beyond 1e-4.
 *   SFM_PROJECTION_REFERENCE_ORDER  the reference's own chain per pixel: ray = K^-1 . pix, c = D ray, q = Pm . (c, 1), U = q0 / z,
 *                                   xn = U / ((W-1)/2.) - 1, the strict test on xn, the sampler's position (xn + 1) (W-1) / 2 --
 *                                   every multiply, add and quotient rounded where the reference rounds it (quotients as v_rcp +
 *                                   residual correction: the IEEE result except in rare double-rounding cases).  45 vector
 *                                   instructions per pixel row: the launch is about 10 % longer.  GUARANTEES: warped pixels within
 *                                   1e-4 of the image range at ANY frame size, seams, large motion and samples behind the camera
 *                                   included, and gradients that need no second opinion (d_pose within 1e-5 of its maximum).
 * Both produce d_src (a second launch re-projects the pixels by the same chain). */
#define SFM_PROJECTION_FAST 0
#define SFM_PROJECTION_REFERENCE_ORDER 1

typedef struct SfmLossDesc {
  int32_t B;        /* samples held by this call (a batch shard)                              */
  int32_t norm_B;   /* batch size used in every mean: the GLOBAL batch when sharded, else B   */
  int32_t n_src;    /* seq_len - 1 (base_model.py:34)                                         */
  int32_t n_scales; /* len(pred_disps) (:66)                                                  */
  int32_t H[SFM_MAX_SCALES];
  int32_t W[SFM_MAX_SCALES];
  float smooth_reg;    /* config['smooth_reg'] (:37); 0 disables (:75)                        */
  float exp_reg;       /* config['exp_reg'] (:38); 0 disables (:86,:103)                      */
  float ssim_rate;     /* config.get('ssim_rate', 0) (:39)                                    */
  int32_t smooth_mode; /* SFM_SMOOTH_*                                                        */
  /* inputs */
  const float *tgt[SFM_MAX_SCALES];         /* (B,3,h,w)        curr_tgt_img  (:71)  [layout] */
  const float *src[SFM_MAX_SCALES];         /* (B,3*n_src,h,w)  curr_src_imgs (:72)  [layout] */
  const float *disp[SFM_MAX_SCALES];        /* (B,1,h,w)        pred_disps    (:59)           */
  const float *mask_logits[SFM_MAX_SCALES]; /* (B,n_src,h,w)    pred_maskes (:62) or NULL     */
  const float *intrinsics;                  /* (B,n_scales,3,3) (:85): ANY invertible 3x3 per (sample, scale) -- skew, a general
                                             * bottom row, a scaled matrix -- and the scales need not be related (scale s is read, never
                                             * derived from scale 0); all nine entries are used, as by F.batch_inv / F.batch_matmul
                                             * (transform.py:43-91,105).  Held by tests/test_cameras_gpu.py.                            */
  const float *pose[SFM_MAX_SRC];           /* (B,6)            pred_poses[i] (:62)           */
  /* gradient outputs (backward only) */
  float *d_disp[SFM_MAX_SCALES]; /* (B,1,h,w)     overwritten                                 */
  float *d_pose[SFM_MAX_SRC];    /* (B,6)         overwritten                                 */
  float *d_mask[SFM_MAX_SCALES]; /* (B,n_src,h,w) overwritten; required iff exp_reg != 0      */
  /* optional: dL/d(curr_src_imgs) (the reference computes it -- the sampler's gx, models/transform.py:189 -- and drops it,
   * base_model.py:71-72 `.data`).  Any subset of the scales may bind it.  Binding it adds a second kernel launch to
   * sfm_loss_bwd / sfm_loss_fwd_bwd (the pixels re-projected, their taps summed in on-chip memory) and, per bound scale,
   * B*3*n_src*h*w floats to sfm_loss_workspace_bytes (dL/d(warped pixel), recorded by the first launch). */
  float *d_src[SFM_MAX_SCALES];  /* (B,3*n_src,h,w) or NULL; ACCUMULATED (atomics)            */
  int32_t image_layout;          /* SFM_LAYOUT_* of tgt[] and src[]                           */
  /* optional output of sfm_loss_fwd and sfm_loss_fwd_bwd (ignored by sfm_loss_bwd): the warped source images the loss
   * was computed on, curr_proj_img of models/base_model.py:90-94, i.e. what projective_inverse_warp returns for source i
   * at scale s -- exactly 0 where the sample is not in view (:96).  Planar in both image layouts. (ABI v4) */
  float *warped[SFM_MAX_SCALES]; /* (B,n_src,3,h,w) or NULL; overwritten                      */
  int32_t projection;            /* SFM_PROJECTION_* (ABI v5); 0 = SFM_PROJECTION_FAST        */
} SfmLossDesc;

/* scratch needed by the three calls below for this descriptor (0 on a bad descriptor; a multiple of 256).  It depends on the shapes,
 * on n_src and on WHICH d_src[] are bound: query with the descriptor the calls will get.
 * `ws` of sfm_loss_* and sfm_step_*: at least that many bytes (`ws_bytes` says how many), starting on a 256-BYTE boundary -- the
 * per-wavefront partial sums are laid out in it in 256-byte aligned arrays of 16- and 48-byte records that are read back 16 bytes at
 * a time.  ws NULL, ws_bytes too small or ws off the boundary: SFM_ERR_WORKSPACE before anything is launched.  Its content is
 * undefined before and after a call; two calls in flight at the same time (two streams) need a workspace each. */
size_t sfm_loss_workspace_bytes(const SfmLossDesc *desc);

/* loss5 (device, 5 floats): total, pixel, smooth, exp, ssim -- the chainer.report keys
 * (:119-123) in that order.  With norm_B > B the values are this shard's additive share. */
int sfm_loss_fwd(const SfmLossDesc *desc, float *loss5, void *ws, size_t ws_bytes, void *stream);
/* gradients of total_loss scaled by the upstream gradient gy (loss.backward() => gy = 1) */
int sfm_loss_bwd(const SfmLossDesc *desc, float gy, void *ws, size_t ws_bytes, void *stream);
/* forward and backward in one launch: loss5 and the gradients for gy = 1 */
int sfm_loss_fwd_bwd(const SfmLossDesc *desc, float *loss5, void *ws, size_t ws_bytes, void *stream);

/* Measurement hook (the reference times the same loop with CUDA events, models/utils.py:16-30,
 * models/base_model.py:67): the NEXT sfm_loss_* call of the calling thread records the two
 * hipEvent_t handles on its stream immediately before and after its main kernel, then forgets
 * them.  NULL disables. */
int sfm_loss_profile_events(void *ev_start, void *ev_stop);
/* Host-side only (no device needed): the work decomposition the library chooses for `desc` and the entry point given by
 * (grad, loss) = (0,1) sfm_loss_fwd, (1,0) sfm_loss_bwd, (1,1) sfm_loss_fwd_bwd.  out[0] = wavefront items of the launch; then
 * per scale four ints: strips, row chunks per strip, rows of a chunk, items per sample (n_out >= 1 + 4 * n_scales).  With
 * n_out >= 1 + 4 * n_scales + 2 two more ints follow: the kernel family of the main launch (0 base, 1 the three-waves-per-SIMD build
 * of the small L1 gradient launches, 2 two sources per pass, 3 reference-order projection, 4 the kernels that record dL/dI^ for d_src)
 * and its resident waves per SIMD.  For tests and tuning; nothing is launched. */
int sfm_loss_plan_info(const SfmLossDesc *desc, int grad, int loss, int *out, int n_out);

/* Development / test hook, consumed by the NEXT sfm_loss_* call of the calling thread (whatever becomes of that call), then back
 * to 0.  3 = the kernels read the header of their argument block from the struct instead of taking it as preloaded scalar arguments
 * -- the path of a batch or a tile count beyond 16 bits, which no test could reach otherwise (results are bit-identical to 0).
 * 4 / 5 = one source per pass / two sources per pass wherever the latter exists (SSIM gradient launches in SFM_LAYOUT_HWC with an
 * even number of sources, FAST projection, no d_src), whatever the library would choose: the same arithmetic per pixel, the two
 * sources' shares of d_disp added in another order (in-process A/B timing and tests).
 * (Rounds 4-5 selected the projection with values 1 and 2 here: that is SfmLossDesc.projection since ABI v5.) */
int sfm_loss_variant(int variant);
/* Diagnostics: the NEXT sfm_loss_* call of this thread makes every wavefront of its main kernel
 * write {start, end (100 MHz realtime counter), HW_ID, XCC_ID} as 4 x uint64 per work item into
 * buf (device memory, 32 bytes * number of items; items <= workspace_bytes / 64). NULL disables. */
int sfm_loss_debug_trace(void *buf);

/* ------------------------------------------------------------------------------------------
 * F.resize_images(x, (oH,oW)) as used for the pyramid, models/base_model.py:70-72:
 * bilinear, align-corners.  x (N,C,H,W) -> y (N,C,oH,oW).
 * ---------------------------------------------------------------------------------------- */
int sfm_resize_fwd(const float *x, float *y, int N, int C, int H, int W, int oH, int oW, void *stream);

/* The image pyramid of one step in ONE launch: the loop head models/base_model.py:69-72 for one
 * tensor.  x (N,C,H,W) -> y[s] (N,C,H>>s,W>>s) for s = 1..n_scales-1, every scale resampled from
 * the full-resolution input (as the reference does); y[0] is ignored (scale 0 is x itself). */
int sfm_pyramid_fwd(const float *x, float *const *y, int N, int C, int H, int W, int n_scales, void *stream);
/* The same pyramid written pixel-interleaved for SFM_LAYOUT_HWC: x (N,3*G,H,W) planar, G images per sample
 * (1 for the target, n_src for the sources, base_model.py:50-57) -> y[s] (N,G,H>>s,W>>s,3) for s = 0..n_scales-1
 * (scale 0 is the re-laid-out input).  Values are identical to sfm_pyramid_fwd's. */
int sfm_pyramid_hwc_fwd(const float *x, float *const *y, int N, int G, int H, int W, int n_scales, void *stream);
/* Development / test hook: which kernel the NEXT sfm_pyramid_hwc_fwd / sfm_pyramid_pair_hwc_fwd call of the calling thread runs,
 * then back to automatic.  0 = automatic (the band kernel that reads every input pixel once, where the shape allows),
 * 1 = the one-thread-per-output-pixel kernel.  Same values bit for bit.  The hook is consumed by that next call whatever becomes
 * of it (empty batch, rejected argument); sfm_pyramid_fwd (planar) does not take it. */
int sfm_pyramid_variant(int variant);
/* Both pyramids of a step in ONE launch: tgt (N,3,H,W) and src (N,3*n_src,H,W) (base_model.py:50-57) ->
 * y_tgt[s] (N,1,h,w,3), y_src[s] (N,n_src,h,w,3), s = 0..n_scales-1: the whole loop head :69-72. */
int sfm_pyramid_pair_hwc_fwd(const float *tgt, const float *src, float *const *y_tgt, float *const *y_src, int N, int n_src,
                             int H, int W, int n_scales, void *stream);

/* One step of SFMLearner.__call__ from the FULL-RESOLUTION frames in one call (models/base_model.py:48-124; ABI v5): the loop head
 * :69-72 -- sfm_pyramid_pair_hwc_fwd of tgt_full (B,3,H,W) and src_full (B,3*n_src,H,W) into the buffers desc->tgt[s] /
 * desc->src[s], which the descriptor must bind as SFM_LAYOUT_HWC with H[s] = H[0] >> s, W[s] = W[0] >> s -- followed by
 * sfm_loss_fwd (sfm_step_fwd) or sfm_loss_fwd_bwd (sfm_step_fwd_bwd) on the same stream.  Exactly the two calls it replaces, same
 * results bit for bit; it exists for callers whose step is host-bound (the reference trains at B = 4, experiments/sfm_learner_v1.yml:43:
 * 25 us of GPU work per step): one trip through the FFI, one argument conversion, one plan look-up.  Every argument -- descriptor,
 * loss5, workspace -- is checked BEFORE the pyramids are written: a rejected step leaves desc->tgt[] / desc->src[] as they were. */
int sfm_step_fwd(const float *tgt_full, const float *src_full, const SfmLossDesc *desc, float *loss5, void *ws, size_t ws_bytes,
                 void *stream);
int sfm_step_fwd_bwd(const float *tgt_full, const float *src_full, const SfmLossDesc *desc, float *loss5, void *ws, size_t ws_bytes,
                     void *stream);

/* ------------------------------------------------------------------------------------------
 * DispNet's output activation for all scales in one launch, models/disp_net.py:7-8 and
 * :104,:110,:116,:122:  disp = 10 * sigmoid(x) + 0.01.  numel[s] = elements of scale s.
 * Backward: g_x = g_disp * 10 * s * (1 - s), s recovered from disp (overwrites g_x).
 * ---------------------------------------------------------------------------------------- */
int sfm_disp_act_fwd(const float *const *x, float *const *disp, const long long *numel, int n_scales, void *stream);
int sfm_disp_act_bwd(const float *const *disp, const float *const *g_disp, float *const *g_x, const long long *numel,
                     int n_scales, void *stream);

/* ------------------------------------------------------------------------------------------
 * The gradients of a gy = 1 backward (sfm_loss_fwd_bwd, sfm_step_fwd_bwd) scaled by an upstream gradient that lives on the
 * DEVICE (ABI v6): the 0-d grad_output an autograd engine hands over, read by the kernel, never by the host -- so the scaling
 * needs no device sync and can be captured in a graph.
 *   y[k][j] = x[k][j] * gy[0] for k < n, j < numel[k]: ONE IEEE fp32 multiply per element (bitwise x * gy, for gy = +-0, inf and
 *   NaN too).  One launch for all n <= 32 arrays (d_disp x8, d_pose x8, d_mask x8, d_src x8).  y[k] == x[k] (in place) is
 *   allowed, partial overlap is not.  numel[k] == 0 skips array k (its pointers may be NULL); a total of 0 launches nothing.
 * Errors: x, y, numel or gy NULL -> SFM_ERR_NULL; n outside 1..32 or numel[k] < 0 -> SFM_ERR_SHAPE (checked before any HIP call).
 * ---------------------------------------------------------------------------------------- */
int sfm_scale_arrays(const float *const *x, float *const *y, const long long *numel, int n, const float *gy, void *stream);

/* ------------------------------------------------------------------------------------------
 * data_augmentation(), datasets/kitti/kitti_raw_transformed.py:23-74, image side: random scaling
 * (:32-45, F.resize_images to (scaled_h, scaled_w)), random crop back to (H,W) at (offset_y,
 * offset_x) (:48-59) and horizontal flip (:62-67) as ONE gather per output pixel.
 *   imgs (B,F,C,H,W): target + sources of each sample ; out the same shape ;
 *   params (B,5) float: scaled_h, scaled_w, offset_y, offset_x, flip (0/1), drawn on the host in the
 *   reference's order (the intrinsics update :41-44,:54-57,:66 is 4 scalars per sample, host side).
 * ---------------------------------------------------------------------------------------- */
int sfm_augment_fwd(const float *imgs, const float *params, float *out, int B, int F, int C, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------
 * The backward of sfm_resize_fwd.
 * ---------------------------------------------------------------------------------------- */
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

/* ------------------------------------------------------------------------------------------
 * The gradient with respect to the camera intrinsics.
 *
 * The intrinsics enter the view synthesis twice (citations into pfnet/sfm-learner-chainer): Pm = K4 . [R|t] in proj_tgt_to_src
 * (models/transform.py:86-88) and ray = K^-1 . pix through F.batch_inv in pixel2cam (:105).  With gPm = dL/dPm (rows 0..2):
 *   dL/dK = gPm[:, 0:3] . R^T + gPm[:, 3] . t^T  -  K^-T . gKinv . K^-T ,   gKinv = dL/d(K^-1) = sum over pixels of g_ray (x) pix .
 * With ONE depth per pixel (models/base_model.py:82-84) gKinv = (K R)^T . gPm[:, 0:3] . K^T, so the second term is
 * K^-T . R^T . K^T . gPm[:, 0:3]: the gradient follows from gPm alone.
 * ---------------------------------------------------------------------------------------- */
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

/* ------------------------------------------------------------------------------------------
 * The differentiable warp of the whole source pyramid of one step.
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
 * ---------------------------------------------------------------------------------------- */
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

/* ------------------------------------------------------------------------------------------
 * The per-pixel photometric error maps of a whole warped pyramid.
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
 * ---------------------------------------------------------------------------------------- */
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

/* ------------------------------------------------------------------------------------------
 * DEVELOPMENT ONLY -- environment variables the library reads ONCE per process (at the first call that needs them; setting them
 * later has no effect).  They move work between wavefronts or pick another kernel for the same arithmetic; none changes a result
 * beyond the summation order of the per-wave partial sums.  Not part of the interface: names and meaning may change.
 *   fused loss (csrc/sfm_loss.hip, struct Tuning):
 *     SFM_CHUNK_ROWS=n            rows of a wave's chunk at every scale (4..28) instead of the planned heights
 *     SFM_CHUNK_ROWS_LIST=a,b,..  the same per scale
 *     SFM_NO_FILL                 no slot-filling refinement of the chunk heights (plan_chunks)
 *     SFM_NO_WIDE                 small L1 launches on the four-waves-per-SIMD build too
 *     SFM_PAIR=0|1                never / wherever possible two sources per pass (as sfm_loss_variant 4 / 5, for a whole process)
 *     SFM_PRIO_TABLE=abc,def      issue-priority levels of the dispatch rounds in the first / second half of the sources
 *     SFM_DEAL_ITEMS_BELOW=n      batches smaller than n (default 8) have their items, not whole samples, dealt over the XCDs
 *   image pyramid (csrc/sfm_ops.hip, struct PyramidTuning):
 *     SFM_PYRAMID_BAND_ROWS=n     input rows per band of the band kernel
 *     SFM_PYRAMID_THREADS=n       threads per workgroup of the band kernel
 * One-call hooks with the same purpose are entry points above: sfm_loss_variant, sfm_pyramid_variant, sfm_loss_profile_events,
 * sfm_loss_debug_trace.  Diagnostic BUILDS (never the product): -DSFM_STAMPS (`make stamps`), -DSFM_FIN_STAMPS.
 * ---------------------------------------------------------------------------------------- */

#ifdef __cplusplus
}
#endif
#endif /* SFMWARP_H_ */
