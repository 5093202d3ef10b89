"""The oracle against an INDEPENDENT implementation with an independent backward.

`oracle/sfm_oracle.py` restates the reference op for op in NumPy and carries a hand-derived backward.
Here the same loss -- models/transform.py:11-193 and models/base_model.py:57-185 of pfnet/sfm-learner-chainer -- is written a
second time with torch ops on the CPU in float64, and its gradients come from torch's AUTOGRAD, not from any formula of
this repository:

  F.spatial_transformer_sampler  -> torch.nn.functional.grid_sample(align_corners=True, padding_mode="zeros")
  F.average_pooling_2d(x, 3,1,1) -> avg_pool2d(3, 1, 1)  (count_include_pad: divide by 9 always)
  F.resize_images                -> interpolate(mode="bilinear", align_corners=True)
  F.batch_matmul / F.batch_inv   -> torch.matmul / torch.linalg.inv
  F.sigmoid_cross_entropy(x, 1)  -> softplus(-x)

This does not pin the oracle on Chainer 4.0.0b1 (that needs tests/golden/make_chainer_golden.py on a machine that has
it); it removes the risk that the hand-derived backward and the finite-difference spot checks share a blind spot, and it
holds the published semantics of the four Chainer ops the path uses against a second, widely used implementation of them.
Tolerance: 1e-10 relative (both sides are float64; measured agreement ~1e-14).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import cameras
import test_loss_gpu as L      # its constants and knife widths (nothing in it runs here)
import test_ops_gpu as OPS     # the inputs of its warp test
from oracle import sfm_oracle as O
from oracle.parity import knife_mask

TOL = 1e-10
DT = torch.float64


def euler2mat(r):
    """models/transform.py:11-40"""
    r = torch.clamp(r, -math.pi, math.pi)
    c, s = torch.cos(r), torch.sin(r)
    zeros, ones = torch.zeros_like(r[:, 0]), torch.ones_like(r[:, 0])
    zmat = torch.stack([c[:, 2], -s[:, 2], zeros, s[:, 2], c[:, 2], zeros, zeros, zeros, ones], dim=1).reshape(-1, 3, 3)
    ymat = torch.stack([c[:, 1], zeros, s[:, 1], zeros, ones, zeros, -s[:, 1], zeros, c[:, 1]], dim=1).reshape(-1, 3, 3)
    xmat = torch.stack([ones, zeros, zeros, zeros, c[:, 0], -s[:, 0], zeros, s[:, 0], c[:, 0]], dim=1).reshape(-1, 3, 3)
    return torch.matmul(torch.matmul(xmat, ymat), zmat)


def proj_tgt_to_src(vec, K):
    """models/transform.py:43-91"""
    N = vec.shape[0]
    filler = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=DT).reshape(1, 1, 4).repeat(N, 1, 1)
    T = torch.cat([torch.cat([euler2mat(vec[:, :3]), vec[:, 3:].reshape(N, 3, 1)], dim=2), filler], dim=1)
    K_ = torch.cat([torch.cat([K, torch.zeros((N, 3, 1), dtype=DT)], dim=2), filler], dim=1)
    return torch.matmul(K_, T)


def projective_inverse_warp(imgs, depthes, poses, K):
    """models/transform.py:94-193; depthes (N,3,H*W)"""
    N, _, H, W = imgs.shape
    proj = proj_tgt_to_src(poses, K)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=DT), torch.arange(W, dtype=DT), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], dim=0).reshape(1, 3, H * W).expand(N, 3, H * W)
    cam = depthes * torch.matmul(torch.linalg.inv(K), pix)                                          # :105-107
    cam = torch.cat([cam, torch.ones((N, 1, H * W), dtype=DT)], dim=1)                              # :108
    q = torch.matmul(proj, cam)                                                                     # :122
    z = q[:, 2:3] + 1e-10                                                                           # :123
    px = (q[:, 0:1] / z) / ((W - 1) / 2.) - 1                                                       # :124
    py = (q[:, 1:2] / z) / ((H - 1) / 2.) - 1                                                       # :125
    p = torch.cat([px, py], dim=1)
    inside = (p.detach() > -1) & (p.detach() < 1)                                                   # :128-131
    p = p * torch.where(inside, torch.ones_like(p), torch.full_like(p, 2.0))
    grid = p.reshape(N, 2, H, W).permute(0, 2, 3, 1)                                                # (N,H,W,2): x, y
    return TF.grid_sample(imgs, grid, mode="bilinear", padding_mode="zeros", align_corners=True)    # :189


def compute_ssim(x, y):
    """models/base_model.py:126-142 (target-side statistics detached: `.data`)"""
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    pool = lambda t: TF.avg_pool2d(t, 3, 1, 1)
    mu_x, mu_y = pool(x), pool(y).detach()
    sigma_x = pool(x ** 2) - mu_x ** 2
    sigma_y = pool(y ** 2).detach() - mu_y ** 2
    sigma_xy = pool(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + c1) * (2 * sigma_xy + c2)
    d = (mu_x ** 2 + mu_y ** 2 + c1) * (sigma_x + sigma_y + c2)
    return torch.clamp((1 - n / d) / 2, 0., 1.)


def gradient(t):
    return t[:, :, :, 1:] - t[:, :, :, :-1], t[:, :, 1:] - t[:, :, :-1]      # D_dx, D_dy


def compute_smooth_loss(d):
    """models/base_model.py:169-185"""
    dx, dy = gradient(d)
    dx2, dxdy = gradient(dx)
    dydx, dy2 = gradient(dy)
    return dx2.abs().mean() + dxdy.abs().mean() + dydx.abs().mean() + dy2.abs().mean()


def compute_disp_smooth(img, d):
    """models/base_model.py:144-155"""
    i_dx, i_dy = gradient(img)
    i_dx, i_dy = i_dx.mean(dim=1, keepdim=True), i_dy.mean(dim=1, keepdim=True)
    d_dx, d_dy = gradient(d)
    return (d_dx.abs() * torch.exp(-i_dx.abs())).mean() + (d_dy.abs() * torch.exp(-i_dy.abs())).mean()


def torch_loss(tgt_pyr, src_pyr, intrinsics, disps, poses, masks, smooth_reg=0.0, exp_reg=0.0, ssim_rate=0.0,
               smooth_mode="second_order"):
    """SFMLearner.__call__ from the pyramid onwards, models/base_model.py:57-124"""
    B = tgt_pyr[0].shape[0]
    n_src = len(poses)
    smooth_loss = exp_loss = pixel_loss = ssim_loss = torch.zeros((), dtype=DT)
    for ns in range(len(disps)):
        tgt, src = tgt_pyr[ns], src_pyr[ns]
        if smooth_reg:                                                                    # :75-80
            term = compute_smooth_loss(disps[ns]) if smooth_mode == "second_order" else compute_disp_smooth(tgt, disps[ns])
            smooth_loss = smooth_loss + (smooth_reg / (2 ** ns)) * term
        depth = (1. / disps[ns]).reshape(B, 1, -1).expand(B, 3, -1)                       # :60,:81-84
        K = intrinsics[:, ns]
        for i in range(n_src):
            proj = projective_inverse_warp(src[:, i * 3:(i + 1) * 3], depth, poses[i], K)  # :90-94
            err = (proj - tgt).abs()                                                      # :95
            mask = (proj.detach() == 0).all(dim=1, keepdim=True).expand_as(err)           # :96-97
            err = torch.where(mask, torch.zeros_like(err), err)                           # :98-100
            if exp_reg:                                                                   # :103-109
                logit = masks[ns][:, i:i + 1]
                exp_loss = exp_loss + exp_reg * TF.softplus(-logit).mean()               # :157-167
                pixel_loss = pixel_loss + (err * torch.sigmoid(logit).expand_as(err)).mean()
            else:
                pixel_loss = pixel_loss + err.mean()                                      # :111
                if ssim_rate:                                                             # :112-115
                    ssim_loss = ssim_loss + (compute_ssim(proj, tgt) * (1 - mask.to(DT))).mean()
    total = (1 - ssim_rate) * pixel_loss + ssim_rate * ssim_loss + smooth_loss + exp_loss  # :117-118
    return total, pixel_loss, smooth_loss, exp_loss, ssim_loss


CONFIGS = {
    "l1": dict(),
    "l1_smooth": dict(smooth_reg=0.1),
    "ssim_smooth": dict(smooth_reg=0.1, ssim_rate=0.15),
    "ssim_only": dict(ssim_rate=0.15),
    "edge_aware": dict(smooth_reg=0.1, ssim_rate=0.15, smooth_mode="edge_aware"),
    "edge_aware_l1": dict(smooth_reg=0.3, smooth_mode="edge_aware"),
    "explain": dict(smooth_reg=0.1, exp_reg=0.2),
    "explain_alpha": dict(smooth_reg=0.1, exp_reg=0.2, ssim_rate=0.15),
}


def _compare_with_autograd(d, cfg, with_src=False):
    """The fp64 oracle against torch autograd on the inputs d: the five scalars, d_disp, d_pose, d_mask (explainability modes) and,
    `with_src`, d_srcs against the gradient of the source pyramid taken as a leaf -- everything at TOL, nothing excluded.  (d_srcs
    can only be compared without a mask on inputs free of exact ties I^ == I, where sign(0) is a convention: asserted from the
    oracle's `abs_zero`.)  Returns the oracle's result."""
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True,
                     dtype=np.float64, keep_warped=True, want_d_src=with_src, **cfg)
    n_scales, n_src = len(d["disps"]), len(d["poses"])
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    disps = [t(a).requires_grad_(True) for a in d["disps"]]
    poses = [t(a).requires_grad_(True) for a in d["poses"]]
    masks = [t(a).requires_grad_(True) for a in d["masks"]]
    srcs = [t(a).requires_grad_(with_src) for a in d["src_pyr"]]
    out = torch_loss([t(a) for a in d["tgt_pyr"]], srcs, t(d["intrinsics"]), disps, poses, masks, **cfg)
    out[0].backward()
    for got, key in zip(out, ("total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss")):
        assert abs(float(got.detach()) - ref[key]) <= TOL * max(abs(ref[key]), 1e-12), (key, float(got.detach()), ref[key])
    # some pixels really are out of view / masked in this case: the x2 rule and the zero fill are exercised
    out_of_view = [float((w == 0).all(axis=2).mean()) for w in ref["warped"]]
    assert max(out_of_view) > 0.01, out_of_view

    def close(a, b, what):
        a, b = a.numpy() if a is not None else np.zeros_like(b), np.asarray(b, np.float64)
        assert np.abs(a - b).max() <= TOL * max(np.abs(b).max(), 1e-30), (what, np.abs(a - b).max(), np.abs(b).max())

    for s in range(n_scales):
        close(disps[s].grad, ref["d_disps"][s], "d_disp[%d]" % s)
        if cfg.get("exp_reg"):
            close(masks[s].grad, ref["d_masks"][s], "d_mask[%d]" % s)
        if with_src:
            assert not ref["abs_zero"][s].any(), "scale %d: %d in-view pixels with I^ == I exactly" % (s, int(ref["abs_zero"][s].sum()))
            assert np.abs(ref["d_srcs"][s]).max() > 0
            close(srcs[s].grad, ref["d_srcs"][s], "d_src[%d]" % s)
    for i in range(n_src):
        close(poses[i].grad, ref["d_poses"][i], "d_pose[%d]" % i)
    return ref


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("shape", [(2, 24, 40, 2, 2), (1, 17, 29, 3, 3)])
def test_oracle_loss_and_gradients_match_torch_autograd(synth, name, shape):
    B, H, W, n_src, n_scales = shape
    cfg = CONFIGS[name]
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, seed=31, with_masks=True)
    # larger motion than the synthetic default, so that a good share of the pixels leaves the view (zero fill, x2 rule, mask)
    rng = np.random.RandomState(5)
    d["poses"] = [p + rng.normal(0, 0.03, p.shape).astype(np.float32) * np.array([1, 1, 1, 4, 4, 4], np.float32) for p in d["poses"]]
    _compare_with_autograd(d, cfg)


def tie_free(d, seed=77):
    """d with the target pyramid moved off the sources' values (x 0.97 + 0.01 N(0,1)): synth's saturated +-1 regions otherwise put
    I^ == I exactly at in-view pixels, where d_src depends on the convention sign(0) = 0 (tests/test_loss_gpu.py: src_footprints)."""
    rng = np.random.RandomState(seed)
    return dict(d, tgt_pyr=[(a * 0.97 + 0.01 * rng.standard_normal(a.shape)).astype(np.float32) for a in d["tgt_pyr"]])


CAMERA_SHAPE = (2, 32, 48, 2, 3)


@pytest.mark.parametrize("name", cameras.MODES)
@pytest.mark.parametrize("kind", cameras.KINDS)
def test_oracle_matches_torch_autograd_on_general_cameras(synth, kind, name):
    """The oracle is the yardstick of tests/test_cameras_gpu.py: here it is held against autograd for intrinsics that are not
    [[fx,0,cx],[0,fy,cy],[0,0,1]] (skew, a general bottom row, scales that are not scale 0 over 2**s, a scaled matrix), d_srcs
    included."""
    d = tie_free(cameras.camera_inputs(synth, CAMERA_SHAPE, kind))
    _compare_with_autograd(d, CONFIGS[name], with_src=True)


@pytest.mark.parametrize("name", cameras.MODES)
@pytest.mark.parametrize("kind", [None, "general"])
def test_oracle_matches_torch_autograd_on_exact_zero_pixels(synth, kind, name):
    """Images with exact zeros (cameras.zero_regions): samples that are IN VIEW and masked because all three warped channels are 0
    (models/base_model.py:96), next to regions with ONE zero channel, which must not be -- with synth's cameras and general ones."""
    d, rect, one_src, one_tgt = cameras.zero_regions(tie_free(cameras.camera_inputs(synth, CAMERA_SHAPE, kind)))
    ref = _compare_with_autograd(d, CONFIGS[name], with_src=True)
    for s, share in enumerate(zero_pixel_shares(d, ref, one_src, one_tgt)):
        assert share >= 0.03, (s, share)


def in_view(d, ref, s):
    """(B,n,h,w): the sampling position of the oracle passes the strict test of models/transform.py:129"""
    h, w = d["disps"][s].shape[2:]
    with np.errstate(invalid="ignore"):
        xn, yn = ref["uv"][s][:, :, 0] / ((w - 1) / 2.) - 1, ref["uv"][s][:, :, 1] / ((h - 1) / 2.) - 1
        return (xn > -1) & (xn < 1) & (yn > -1) & (yn < 1)


def zero_pixel_shares(d, ref, one_src, one_tgt):
    """Per scale, the share of the (sample, source, pixel) triples that are in view AND masked (all three warped channels exactly
    0); asserts on the way that a zero in ONE channel masks nothing: no in-view pixel of the target's one-channel region, and no
    in-view pixel whose four taps all lie in the sources' one-channel region, is masked."""
    shares = []
    for s, w in enumerate(ref["warped"]):
        inv = in_view(d, ref, s)
        masked = (w == 0).all(axis=2)
        assert not (masked & inv & one_tgt[s]).any(), "scale %d: masked in-view pixels inside the target's one-channel region" % s
        hh, ww = one_src[s].shape
        with np.errstate(invalid="ignore"):
            u0 = np.clip(np.nan_to_num(np.floor(ref["uv"][s][:, :, 0])), 0, ww - 2).astype(np.int64)
            v0 = np.clip(np.nan_to_num(np.floor(ref["uv"][s][:, :, 1])), 0, hh - 2).astype(np.int64)
        a = one_src[s]
        taps_in = a[v0, u0] & a[v0, u0 + 1] & a[v0 + 1, u0] & a[v0 + 1, u0 + 1]
        assert (taps_in & inv).any(), "scale %d: no in-view sample inside the sources' one-channel region" % s
        assert not (masked & inv & taps_in).any(), "scale %d: masked in-view pixels whose taps lie in the sources' one-channel region" % s
        shares.append(float((masked & inv).mean()))
    return shares


def _knife(d, ref, s):
    """the pixels test_loss_gpu._check_grads excludes from the element-wise comparison of d_disp[s], with the widths
    tests/test_cameras_gpu.py passes (knife_widths)"""
    kw = L.knife_widths(d, ref)
    return knife_mask(ref, s, cell_thr=kw["cell_thr"](s), abs_thr=kw["abs_thr"](s))[0][:, None]


def visible_difference(d, ref, other):
    """By how many times its tolerance the result `other` misses the comparison tests/test_loss_gpu.py would make against `ref`
    (both from the fp32 oracle on the inputs d, `other` with another K): the larger of (a) the relative difference of a loss scalar
    over LOSS_RTOL and (b) the largest difference of d_disp over GRAD_TOL of its maximum, at pixels outside the knife mask of BOTH
    evaluations (a kernel that computed `other` is compared outside ref's mask; outside both, neither side sits on a discontinuity)."""
    loss = max(abs(other[k] - ref[k]) / max(abs(ref[k]), 1e-6) for k in L.KEYS) / L.LOSS_RTOL
    grad = 0.0
    for s, (a, b) in enumerate(zip(other["d_disps"], ref["d_disps"])):
        keep = ~(_knife(d, ref, s) | _knife(d, other, s))
        grad = max(grad, float((np.abs(a.astype(np.float64) - b) * keep).max() / np.abs(b).max()) / L.GRAD_TOL)
    return loss, grad


def _oracle32(d, cfg):
    return O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True, keep_warped=True, **cfg)


@pytest.mark.parametrize("shape,zeros,kind", [(shape, False, kind) for shape in cameras.CASES for kind in cameras.KINDS]
                         + [(CAMERA_SHAPE, True, "general")])
def test_a_kernel_that_ignored_an_entry_of_K_would_fail(synth, shape, zeros, kind):
    """What makes tests/test_cameras_gpu.py a test of the general 3x3: on its exact inputs (shapes, seeds, loss modes; `True`: with
    the exact-zero regions), a result computed with one entry of K ignored -- K01, K10, K20, K21 taken as 0, K22 as 1, the scales
    rebuilt from scale 0, or K divided by K22 -- differs from the right one by at least TEN times a tolerance the GPU tests apply:
    LOSS_RTOL on a loss scalar or GRAD_TOL of the maximum on d_disp outside the knife mask.  Both sides are the fp32 oracle.
    The table of which ablation can show on which kind (cameras.ABLATIONS_OF) is checked too: an ablation that is not listed
    leaves that kind's K bit for bit as it is."""
    d = cameras.camera_inputs(synth, shape, kind, zeros=zeros)
    K = d["intrinsics"]
    for name, ablate in cameras.ABLATIONS.items():
        if name not in cameras.ABLATIONS_OF[kind]:
            np.testing.assert_array_equal(ablate(K), K, err_msg="%s changes the %s cameras: list it" % (name, kind))
    for mode in (cameras.MODES if kind == "general" else (cameras.MODE_OF[kind],)):
        cfg = CONFIGS[mode]
        ref = _oracle32(d, cfg)
        for name in cameras.ABLATIONS_OF[kind]:
            Ka = np.ascontiguousarray(cameras.ABLATIONS[name](K), dtype=np.float32)
            assert Ka.shape == K.shape and not np.array_equal(Ka, K)
            loss, grad = visible_difference(d, ref, _oracle32(dict(d, intrinsics=Ka), cfg))
            print("%s %s %s %s: loss off by %.1f x LOSS_RTOL, d_disp by %.1f x GRAD_TOL" % (shape, kind, mode, name, loss, grad))
            assert max(loss, grad) >= 10.0, (shape, kind, mode, name, loss, grad)


@pytest.mark.parametrize("kind", ["skew", "bottom", "scaled", "general"])
@pytest.mark.parametrize("shape", [(2, 3, 16, 52), (1, 3, 37, 70)])
def test_a_warp_operator_that_ignored_an_entry_of_K_would_fail(synth, shape, kind):
    """The same for the inputs of test_cameras_gpu.test_projective_inverse_warp_on_general_cameras: with one entry of K ignored
    the oracle's warped image moves by at least ten times that test's 1e-4 at a pixel both evaluations sample -- on the white-noise
    texture of that test (on the smooth one K20 moves the pixels by 8e-4 only: there the backward's comparisons would notice)."""
    inp = OPS.warp_inputs(synth, shape, "noise", 1, kind)
    imgs, depthes, pose, K = inp["imgs"], inp["depthes"], inp["pose"], inp["K"][:, None]
    want = O.projective_inverse_warp(imgs, depthes, pose, K[:, 0])
    for name in cameras.ABLATIONS_OF[kind]:
        if name == "scales rebuilt from scale 0":      # the operator sees one scale
            continue
        other = O.projective_inverse_warp(imgs, depthes, pose, cameras.ABLATIONS[name](K)[:, 0])
        both = ~(want == 0).all(1, keepdims=True) & ~(other == 0).all(1, keepdims=True)
        assert (np.abs(other - want) * both).max() >= 10 * 1e-4, (shape, kind, name, float((np.abs(other - want) * both).max()))


def test_oracle_sampler_matches_grid_sample():
    """F.spatial_transformer_sampler as restated by the oracle against grid_sample on a random grid that
    reaches beyond the image (the zero-padded ring included), forward and both gradients."""
    rng = np.random.RandomState(3)
    x = rng.uniform(-1, 1, (2, 3, 9, 13))
    grid = rng.uniform(-1.3, 1.3, (2, 2, 7, 11))
    gy = rng.normal(0, 1, (2, 3, 7, 11))
    y = O.spatial_transformer_sampler(x, grid, dtype=np.float64)
    gx, ggrid = O.spatial_transformer_sampler_backward(x, grid, gy, dtype=np.float64)
    xt, gt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(grid).requires_grad_(True)
    yt = TF.grid_sample(xt, gt.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=True)
    yt.backward(torch.from_numpy(gy))
    np.testing.assert_allclose(y, yt.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(gx, xt.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ggrid, gt.grad.numpy(), rtol=0, atol=1e-11)


def test_oracle_resize_and_pooling_match_torch():
    """F.resize_images (align-corners bilinear) and F.average_pooling_2d(3,1,1) (divide by 9, zero padding) as the oracle restates them."""
    rng = np.random.RandomState(4)
    x = rng.uniform(-1, 1, (2, 3, 16, 28))
    for oh, ow in ((8, 14), (4, 7), (16, 28), (5, 9)):
        want = TF.interpolate(torch.from_numpy(x), size=(oh, ow), mode="bilinear", align_corners=True).numpy()
        np.testing.assert_allclose(O.resize_images(x, (oh, ow), dtype=np.float64), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(O.average_pooling_3x3(x), TF.avg_pool2d(torch.from_numpy(x), 3, 1, 1).numpy(), rtol=0, atol=1e-13)
