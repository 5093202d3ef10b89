"""GPU tests of the drop-in surface: the reference's operators and loss link under their own
names (Variable in, Variable out, .backward()), against the oracle."""
import importlib
import os

import numpy as np
import pytest

from oracle import sfm_oracle as O
from util import assert_close_masked, dilate, to_dev, to_np

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

cs = importlib.import_module("sfm-learner-chainer_amd.chainer_surface")
fn = importlib.import_module("sfm-learner-chainer_amd.functions")
links = importlib.import_module("sfm-learner-chainer_amd.links")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")


def test_interp_function_call_and_backward_like_the_reference(dev):
    z = np.load(os.path.join(GOLD, "interp_sampler_small.npz"))
    x = cs.Variable(to_dev(z["x"], dev))
    grid = cs.Variable(to_dev(z["grid"], dev))
    y = fn.spatial_transformer_sampler_interp(x, grid)
    assert isinstance(y, cs.Variable) and y.creator is not None
    np.testing.assert_array_equal(to_np(y.data), z["y"])
    y.grad = to_dev(z["gy"], dev)
    y.backward()
    np.testing.assert_array_equal(to_np(grid.grad), z["ggrid"])
    assert not to_np(x.grad).any()                       # gx == 0 (:148)


def test_projective_inverse_warp_function(synth, dev):
    N, H, W = 2, 32, 52
    d = synth.make_inputs(B=N, H=H, W=W, n_src=2, n_scales=1, seed=6)
    imgs = d["src_pyr"][0][:, :3].copy()
    depth = (1.0 / d["disps"][0]).reshape(N, 1, H * W).astype(np.float32)
    rng = np.random.RandomState(0)
    # general case: three DIFFERENT depth rows (the reference's signature allows it, transform.py:98,107)
    depthes = (np.broadcast_to(depth, (N, 3, H * W)) * (1 + 0.02 * rng.standard_normal((N, 3, 1)))).astype(np.float32)
    pose, K = d["poses"][0], d["intrinsics"][:, 0]
    dv, pv = cs.Variable(to_dev(depthes, dev)), cs.Variable(to_dev(pose, dev))
    out = fn.projective_inverse_warp(to_dev(imgs, dev), dv, pv, to_dev(K, dev))
    want, aux = O.projective_inverse_warp(imgs, depthes, pose, K, return_aux=True)
    knife = (aux["margin"] < 2e-5)[:, None]
    assert_close_masked(to_np(out.data), want, 1e-4, knife, what="warped (3 depth rows)")
    g = (want - d["tgt_pyr"][0]).astype(np.float32)      # an L2-style upstream gradient
    out.grad = to_dev(g, dev)
    out.backward()
    w_dep, w_pose, _ = O.projective_inverse_warp_backward(imgs, depthes, pose, K, g)
    kcell = knife | ((aux["cell_margin"] < 3e-4) & ~(want == 0).all(1))[:, None]
    assert_close_masked(to_np(dv.grad).reshape(N, 3, H, W), w_dep.reshape(N, 3, H, W), 1e-3, kcell, what="g_depthes")
    assert_close_masked(to_np(pv.grad), w_pose, 2e-3, what="g_poses")


def test_proj_tgt_to_src_function(dev):
    rng = np.random.RandomState(1)
    vec = rng.normal(0, 0.05, (4, 6)).astype(np.float32)
    K = np.tile(np.array([[241.7, 0, 204.2], [0, 246.3, 59.0], [0, 0, 1]], np.float32), (4, 1, 1))
    v = cs.Variable(to_dev(vec, dev))
    P = fn.proj_tgt_to_src(v, to_dev(K, dev), 4)
    np.testing.assert_allclose(to_np(P.data), O.proj_tgt_to_src(vec, K), rtol=2e-6, atol=2e-5)
    g = rng.normal(size=(4, 4, 4)).astype(np.float32)
    P.grad = to_dev(g, dev)
    P.backward()
    want = O.proj_tgt_to_src_backward(vec.astype(np.float64), K.astype(np.float64), g.astype(np.float64), np.float64)
    np.testing.assert_allclose(to_np(v.grad), want, rtol=0, atol=2e-4 * np.abs(want).max())


@pytest.mark.parametrize("config", [
    {"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 3},                          # experiments/sfm_learner_v1.yml
    {"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 3, "ssim_rate": 0.15},       # experiments/sfm_learner_v1_ssim.yml
    {"smooth_reg": 0.1, "exp_reg": 0.2, "seq_len": 5},                        # experiments/sfm_learner_v1_odom.yml
])
def test_sfm_learner_loss_link(synth, dev, config):
    """SFMLearner.__call__ (models/base_model.py:48-124) from the network outputs onwards:
    the pyramid is built on the device (F.resize_images, :70-72)."""
    n_src = config["seq_len"] - 1
    B, H, W, S = 2, 32, 104, 3
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=S, seed=8, with_masks=True)
    link = links.SFMLearnerLoss(config)
    disps = [cs.Variable(to_dev(a, dev)) for a in d["disps"]]
    poses = [cs.Variable(to_dev(a, dev)) for a in d["poses"]]
    masks = [cs.Variable(to_dev(a, dev)) for a in d["masks"]]
    K = to_dev(d["intrinsics"], dev)
    loss = link(to_dev(d["tgt"], dev), to_dev(d["src"], dev), K, K, disps, poses, masks)
    cfg = dict(smooth_reg=config["smooth_reg"], exp_reg=config["exp_reg"], ssim_rate=config.get("ssim_rate", 0.0))
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], d["masks"], backward=True,
                     keep_warped=True, **cfg)
    assert isinstance(loss, cs.Variable) and loss.shape == ()
    assert abs(float(loss.data) - ref.total_loss) <= 1e-4 * abs(ref.total_loss)
    rep = cs.get_report(link)      # scoped by the observer that reported (the link), as chainer.report's observer argument
    for k in ("total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss"):     # :119-123
        assert abs(float(rep[k]) - ref[k]) <= 1e-4 * max(abs(ref[k]), 1e-6), k
    loss.backward()
    from test_loss_gpu import _knife
    for s in range(S):
        assert_close_masked(to_np(disps[s].grad), ref.d_disps[s], 2e-3, _knife(ref, s, n_src), what="disp.grad[%d]" % s)
    for i in range(n_src):
        assert_close_masked(to_np(poses[i].grad), ref.d_poses[i], 2e-3, what="pose.grad[%d]" % i)
    if config["exp_reg"]:
        for s in range(S):
            assert_close_masked(to_np(masks[s].grad), ref.d_masks[s], 2e-3, what="mask.grad[%d]" % s)
    else:
        assert all(m.grad is None for m in masks)


def test_loss_link_takes_frames_above_the_pixel_interleaved_limit(synth, dev):
    """SFM_LAYOUT_HWC is limited to images of fewer than 2^24 / 12 = 1,398,101 pixels per scale (the gather forms byte offsets in
    fp32); the link binds the reference's planar layout for larger frames instead of failing (round-3 advisor finding), with the
    same results: against the oracle, twice (the second call re-uses the bound buffers, scale 0 included)."""
    B, H, W, S = 1, 1024, 1408, 2          # 1,441,792 pixels at scale 0
    assert H * W >= links.HWC_MAX_PIXELS
    d = synth.make_inputs(B=B, H=H, W=W, n_src=1, n_scales=S, seed=4)
    config = {"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 2, "ssim_rate": 0.15}
    link = links.SFMLearnerLoss(config)
    K = to_dev(d["intrinsics"], dev)
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], None, backward=True, keep_warped=True,
                     smooth_reg=0.1, ssim_rate=0.15)
    from test_loss_gpu import _knife, knife_widths
    kw = knife_widths(d, ref)
    for call in range(2):
        disps = [cs.Variable(to_dev(a, dev)) for a in d["disps"]]
        poses = [cs.Variable(to_dev(a, dev)) for a in d["poses"]]
        loss = link(to_dev(d["tgt"], dev), to_dev(d["src"], dev), K, K, disps, poses)
        assert abs(float(loss.data) - ref.total_loss) <= 1e-4 * abs(ref.total_loss), call
        loss.backward()
        for s in range(S):
            # (the cell-boundary and |I^ - I|-kink knife classes as wide as the fp32 uncertainty of each sample's position makes them:
            #  an ulp of U = 1400 is 1.2e-4 px, four times that of the 416-wide BASELINE frames)
            knife = _knife(ref, s, 1, what="1.4 Mpx planar link", cell_thr=kw["cell_thr"](s), abs_thr=kw["abs_thr"](s))
            assert_close_masked(to_np(disps[s].grad), ref.d_disps[s], 2e-3, knife, what="disp.grad[%d]" % s)
    st = next(iter(link._cache.values()))
    assert st.layout == "planar"
    # ... while the C ABI still rejects the pixel-interleaved layout at this size, with a message
    ops = importlib.import_module("sfm-learner-chainer_amd.ops")
    with pytest.raises(TypeError, match="2\\^24"):
        ops.FusedLoss(smooth_reg=0.1).bind([ops.to_hwc(to_dev(a, dev)) for a in d["tgt_pyr"]], [ops.to_hwc(to_dev(a, dev)) for a in d["src_pyr"]],
                                           K, [to_dev(a, dev) for a in d["disps"]], [to_dev(a, dev) for a in d["poses"]], layout="hwc")


def test_loss_link_without_backprop_and_with_upstream_gradient(synth, dev):
    d = synth.make_inputs(B=2, H=32, W=52, n_src=2, n_scales=2, seed=2)
    link = links.SFMLearnerLoss({"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 3, "ssim_rate": 0.15})
    K = to_dev(d["intrinsics"], dev)
    args = (to_dev(d["tgt"], dev), to_dev(d["src"], dev), K, K)
    mk = lambda: ([cs.Variable(to_dev(a, dev)) for a in d["disps"]], [cs.Variable(to_dev(a, dev)) for a in d["poses"]])
    with cs.no_backprop_mode():                           # models/base_model.py:190-191
        disps, poses = mk()
        l0 = link(*args, disps, poses)
    assert l0.creator is None
    disps, poses = mk()
    l1 = link(*args, disps, poses)
    np.testing.assert_allclose(float(l1.data), float(l0.data), rtol=2e-5)
    l1.backward()
    g1 = to_np(disps[0].grad).copy()
    disps2, poses2 = mk()
    l2 = link(*args, disps2, poses2)
    import torch
    l2.grad = torch.full((), 3.0, device=dev)            # e.g. a loss scale
    l2.backward()
    np.testing.assert_allclose(to_np(disps2[0].grad), 3.0 * g1, rtol=1e-6, atol=1e-12)


def test_loss_link_reuses_its_buffers_across_calls(synth, dev):
    """The drop-in path of a training loop: consecutive calls of one link with the same shapes reuse the pyramids, the
    workspace and the gradient arrays (no allocation, the library's plan cache is hit) and give identical results; new
    frames / network outputs of the same shapes are picked up; a loss scale set by the caller is applied on every backward;
    two links keep separate reports; the HIP-graph replay gives the eager results bit for bit."""
    import torch
    d = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=3, seed=6)
    d2 = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=3, seed=7)
    cfgd = {"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 3, "ssim_rate": 0.15}
    ref = [O.sfm_loss(x["tgt_pyr"], x["src_pyr"], x["intrinsics"], x["disps"], x["poses"], backward=True, smooth_reg=0.1, ssim_rate=0.15) for x in (d, d2)]

    def run(link, x, scale=None):
        disps = [cs.Variable(to_dev(a, dev)) for a in x["disps"]]
        poses = [cs.Variable(to_dev(a, dev)) for a in x["poses"]]
        K = to_dev(x["intrinsics"], dev)
        loss = link(to_dev(x["tgt"], dev), to_dev(x["src"], dev), K, K, disps, poses)
        if scale is not None:
            loss.grad = torch.full((), scale, device=dev)
        loss.backward()
        return float(loss.data), [to_np(v.grad).copy() for v in disps + poses], [v.grad.data_ptr() for v in disps + poses]

    link = links.SFMLearnerLoss(cfgd)
    l_a, g_a, p_a = run(link, d)
    st_a = next(iter(link._cache.values()))
    l_b, g_b, p_b = run(link, d)                        # the same values again
    assert next(iter(link._cache.values())) is st_a and p_a == p_b       # same FusedLoss, same gradient arrays handed out
    assert l_a == l_b
    for x, y in zip(g_a, g_b):
        np.testing.assert_array_equal(x, y)
    assert abs(l_a - ref[0].total_loss) <= 1e-4 * abs(ref[0].total_loss)
    l_c, g_c, _ = run(link, d2)                         # other frames and network outputs, same shapes: buffers reused, values new
    assert next(iter(link._cache.values())) is st_a
    assert abs(l_c - ref[1].total_loss) <= 1e-4 * abs(ref[1].total_loss)
    np.testing.assert_allclose(g_c[-1], ref[1].d_poses[-1], rtol=0, atol=2e-3 * np.abs(ref[1].d_poses[-1]).max())
    l_d, g_d, _ = run(link, d, scale=3.0)               # a gradient set by the caller is multiplied in ...
    for x, y in zip(g_a, g_d):
        np.testing.assert_allclose(y, 3.0 * x, rtol=1e-6, atol=1e-12)
    l_e, g_e, _ = run(link, d)                          # ... and does not stick to the next call
    for x, y in zip(g_a, g_e):
        np.testing.assert_array_equal(x, y)
    other = links.SFMLearnerLoss(cfgd, cache_buffers=False)
    l_f, g_f, p_f = run(other, d2)
    assert l_f == l_c and not other._cache
    assert cs.get_report(other)["total_loss"] is not cs.get_report(link)["total_loss"]
    assert abs(float(cs.get_report(link)["total_loss"]) - l_e) == 0 and abs(float(cs.get_report(other)["total_loss"]) - l_f) == 0
    # HIP-graph replay: static input arrays, as a caller with pre-allocated batch buffers has them
    glink = links.SFMLearnerLoss(cfgd, use_graph=True)
    disps = [cs.Variable(to_dev(a, dev)) for a in d["disps"]]
    poses = [cs.Variable(to_dev(a, dev)) for a in d["poses"]]
    K, tgt, src = to_dev(d["intrinsics"], dev), to_dev(d["tgt"], dev), to_dev(d["src"], dev)
    for it in range(4):          # 1st call binds, 2nd sees the addresses again and captures, 3rd and 4th replay
        for v in disps + poses:
            v.cleargrad()
        loss = glink(tgt, src, K, K, disps, poses)
        loss.backward()
        assert float(loss.data) == l_a, it
        for x, v in zip(g_a, disps + poses):
            np.testing.assert_array_equal(x, to_np(v.grad))
    assert next(iter(glink._cache.values())).graph is not None
    tgt.copy_(to_dev(d2["tgt"], dev))                   # new pixels in the SAME arrays: the replayed pyramid launch picks them up
    loss = glink(tgt, src, K, K, disps, poses)
    assert float(loss.data) != l_a


def test_loss_link_keeps_per_call_state(synth, dev):
    """forward(A), forward(B), then backward on the loss of A: with cache_buffers=True (the default) the link's cached gradient
    arrays hold B's gradients by then, so the stale backward raises instead of silently returning them (Chainer keeps per-call
    state; with cache_buffers=False so does this link).  The returned loss and the reported scalars of A keep their values."""
    import pytest as _pytest
    dA = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=2, seed=8)
    dB = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=2, seed=9)
    cfgd = {"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 3, "ssim_rate": 0.15}

    def call(link, x):
        disps = [cs.Variable(to_dev(a, dev)) for a in x["disps"]]
        poses = [cs.Variable(to_dev(a, dev)) for a in x["poses"]]
        K = to_dev(x["intrinsics"], dev)
        return link(to_dev(x["tgt"], dev), to_dev(x["src"], dev), K, K, disps, poses), disps, poses

    link = links.SFMLearnerLoss(cfgd)
    la, disps_a, _ = call(link, dA)
    va, rep_a = float(la.data), cs.get_report(link)["total_loss"]
    lb, disps_b, _ = call(link, dB)
    assert float(lb.data) != va
    assert float(la.data) == va and float(rep_a) == va          # A's scalars were not overwritten by call B
    with _pytest.raises(RuntimeError, match="called again since"):
        la.backward()
    lb.backward()                                                # the latest call's backward is fine
    gb = to_np(disps_b[0].grad).copy()
    # per-call state, as in Chainer: both orders work and give each call its own gradients
    free = links.SFMLearnerLoss(cfgd, cache_buffers=False)
    la2, disps_a2, _ = call(free, dA)
    lb2, disps_b2, _ = call(free, dB)
    la2.backward()
    lb2.backward()
    np.testing.assert_array_equal(to_np(disps_b2[0].grad), gb)
    assert float(la2.data) == va and np.abs(to_np(disps_a2[0].grad) - gb).max() > 0


def test_disp_activation_all_scales_in_one_launch(dev):
    """models/disp_net.py:104-122 and its backward; chained in front of the loss link the gradient lands
    on the raw network outputs"""
    rng = np.random.RandomState(0)
    xs_np = [rng.normal(0, 2, (2, 1, 32 >> s, 52 >> s)).astype(np.float32) for s in range(3)]
    xs = [cs.Variable(to_dev(a, dev)) for a in xs_np]
    disps = fn.disp_activation(xs)
    for d, x in zip(disps, xs_np):
        np.testing.assert_allclose(to_np(d.data), 10.0 / (1.0 + np.exp(-x.astype(np.float64))) + 0.01, rtol=2e-6)
        assert d.data.min() > 0.01 and d.data.max() < 10.01
    g_np = [rng.normal(size=a.shape).astype(np.float32) for a in xs_np]
    for d, g in zip(disps, g_np):
        d.grad = to_dev(g, dev)
    disps[0].backward()
    for x, xn, g in zip(xs, xs_np, g_np):
        sg = 1.0 / (1.0 + np.exp(-xn.astype(np.float64)))
        np.testing.assert_allclose(to_np(x.grad), g * 10.0 * sg * (1 - sg), rtol=2e-4, atol=1e-6)


def test_loss_gradient_reaches_the_disparity_logits(synth, dev):
    d = synth.make_inputs(B=2, H=32, W=52, n_src=2, n_scales=2, seed=3)
    logits_np = [np.log((a - 0.01) / (10.01 - a)).astype(np.float32) for a in d["disps"]]     # inverse of the activation
    logits = [cs.Variable(to_dev(a, dev)) for a in logits_np]
    disps = fn.disp_activation(logits)
    poses = [cs.Variable(to_dev(a, dev)) for a in d["poses"]]
    link = links.SFMLearnerLoss({"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 3, "ssim_rate": 0.15})
    K = to_dev(d["intrinsics"], dev)
    loss = link(to_dev(d["tgt"], dev), to_dev(d["src"], dev), K, K, disps, poses)
    loss.backward()
    disp_np = [10.0 / (1.0 + np.exp(-a.astype(np.float64))) + 0.01 for a in logits_np]
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], [a.astype(np.float32) for a in disp_np], d["poses"],
                     backward=True, smooth_reg=0.1, ssim_rate=0.15)
    assert abs(float(loss.data) - ref.total_loss) <= 2e-4 * abs(ref.total_loss)
    for s in range(2):
        sg = (disp_np[s] - 0.01) / 10.0
        want = ref.d_disps[s] * 10.0 * sg * (1 - sg)
        err = np.abs(to_np(logits[s].grad) - want)
        assert (err > 3e-3 * np.abs(want).max()).mean() < 0.02


def test_on_device_augmentation_matches_the_reference_composition(synth, dev):
    """datasets/kitti/kitti_raw_transformed.py:23-74: resize -> crop -> flip + intrinsics, per sample"""
    aug = importlib.import_module("sfm-learner-chainer_amd.augment")
    B, H, W, S = 4, 32, 104, 2
    d = synth.make_inputs(B=B, H=H, W=W, n_src=S, n_scales=1, seed=12)
    K = d["intrinsics"][:, 0]
    rng = np.random.RandomState(5)
    params = aug.sample_params(rng, B, H, W)
    params[0, 6], params[1, 6] = 1.0, 0.0                # make sure both flip states occur
    imgs = np.concatenate([d["tgt"][:, None], d["src"]], axis=1)
    got = to_np(aug.augment_images(to_dev(imgs, dev), params))
    gotK = aug.augment_intrinsics(K, params, W)
    for b in range(B):
        xs, ys, sh, sw, oy, ox, flip = params[b]
        t, s_, Kb = O.data_augmentation(d["tgt"][b], d["src"][b], K[b], xs, ys, int(oy), int(ox), bool(flip))
        np.testing.assert_allclose(got[b, 0], t, rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(got[b, 1:], s_, rtol=1e-5, atol=2e-6)
        np.testing.assert_array_equal(gotK[b], Kb)
    # the batched entry point: same random stream -> same parameters
    import torch
    t2, s2, Kms = aug.data_augmentation(to_dev(d["tgt"], dev), to_dev(d["src"], dev), K, rng=np.random.RandomState(5), n_scales=3)
    p2 = aug.sample_params(np.random.RandomState(5), B, H, W)
    np.testing.assert_array_equal(to_np(t2), to_np(aug.augment_images(to_dev(imgs, dev), p2))[:, 0])
    np.testing.assert_array_equal(Kms, aug.get_multi_scale_intrinsics(aug.augment_intrinsics(K, p2, W), 3))
    assert tuple(s2.shape) == (B, S, 3, H, W) and Kms.shape == (B, 3, 3, 3)


def test_on_device_augmentation_indexing_matches_the_reference_run_golden(dev):
    """PINNED (round 6, K path + indexing): sfm_augment_fwd with the crop offsets / flip decisions the REFERENCE's own
    data_augmentation drew (tests/golden/intrinsics_aug.npz, datasets/kitti/kitti_raw_transformed.py:23-74 executed unmodified) on
    an image that is LINEAR in x and y: an align-corners bilinear resize of a linear ramp is the ramp on the resized lattice, so
    out(y, x) = ramp at resized position (offset_y + y, offset_x + x) -- mirrored in x when flipped -- is known in closed form and
    any error in the kernel's crop / flip indexing shows as a whole-pixel step."""
    aug = importlib.import_module("sfm-learner-chainer_amd.augment")
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intrinsics_aug.npz"))
    for k in range(int(z["n_cases"])):
        g = lambda name: z["c%d_%s" % (k, name)]
        H, W = [int(v) for v in g("hw")]
        S = int(g("n_src"))
        sh, sw = [int(v) for v in g("scaled_hw")]
        oy, ox = [int(v) for v in g("offset_yx")]
        flip = bool(g("flip"))
        params = aug.sample_params(np.random.RandomState(int(g("seed"))), 1, H, W)
        assert (int(params[0, 4]), int(params[0, 5]), bool(params[0, 6])) == (oy, ox, flip)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        a = np.arange(1, S + 2, dtype=np.float64)[:, None, None, None] * 0.01          # one slope per frame ...
        cch = np.arange(3, dtype=np.float64)[None, :, None, None] * 0.1                # ... one offset per channel
        imgs = (a * xs + 0.5 * a * ys + cch)[None]                                     # (1, F, 3, H, W)
        got = to_np(aug.augment_images(to_dev(imgs.astype(np.float32), dev), params))[0]
        # resized lattice -> input coordinates (align corners: F.resize_images, base_model.py:71 / kitti_raw_transformed.py:39)
        yy = (oy + np.arange(H, dtype=np.float64)) * (H - 1) / max(sh - 1, 1)
        xcol = ox + np.arange(W, dtype=np.float64)
        if flip:
            xcol = xcol[::-1]
        xx = xcol * (W - 1) / max(sw - 1, 1)
        want = a * xx[None, None, None, :] + 0.5 * a * yy[None, None, :, None] + cch
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5 * np.abs(want).max(), err_msg="case %d" % k)
        np.testing.assert_array_equal(aug.augment_intrinsics(g("K_in")[None], params, W)[0], g("K_out"))


def test_step_from_frames_is_the_two_calls_it_replaces(synth, dev):
    """sfm_step_fwd_bwd / sfm_step_fwd (ABI v5): pyramids + fused loss from the full-resolution frames in ONE call through the C ABI
    (models/base_model.py:48-124) -- bit for bit what sfm_pyramid_pair_hwc_fwd followed by sfm_loss_fwd_bwd / sfm_loss_fwd give;
    a planar descriptor and a pyramid shape that is not H >> s are refused with a message."""
    import torch
    d = synth.make_inputs(B=3, H=48, W=136, n_src=2, n_scales=3, seed=8)
    tgt, src = to_dev(d["tgt"], dev), to_dev(d["src"], dev).reshape(3, 6, 48, 136)
    args = (to_dev(d["intrinsics"], dev), [to_dev(a, dev) for a in d["disps"]], [to_dev(a, dev) for a in d["poses"]])
    cfg = dict(smooth_reg=0.1, ssim_rate=0.15, smooth_mode="edge_aware")
    pyr = ops.pyramid_pair_hwc(tgt, src, 3)
    two = ops.FusedLoss(**cfg).bind(list(pyr[0]), list(pyr[1]), *args, layout="hwc")
    l_two = to_np(two.forward_backward()).copy()
    g_two = [to_np(t).copy() for t in two.d_disps + two.d_poses]
    f_two = to_np(two.forward()).copy()
    blank = ([torch.zeros_like(a) for a in pyr[0]], [torch.zeros_like(a) for a in pyr[1]])     # the call writes the pyramids itself
    one = ops.FusedLoss(**cfg).bind(blank[0], blank[1], *args, layout="hwc")
    l_one = to_np(one.step_from_frames(tgt, src, grad=True)).copy()
    np.testing.assert_array_equal(l_one, l_two)
    for a, b in zip(g_two, [to_np(t) for t in one.d_disps + one.d_poses]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(list(pyr[0]) + list(pyr[1]), blank[0] + blank[1]):
        np.testing.assert_array_equal(to_np(a), to_np(b))
    np.testing.assert_array_equal(to_np(one.step_from_frames(tgt, src, grad=False)), f_two)
    planar = ops.FusedLoss(**cfg).bind([to_dev(a, dev) for a in d["tgt_pyr"]], [to_dev(a, dev) for a in d["src_pyr"]], *args)
    with pytest.raises(ValueError, match="SFM_LAYOUT_HWC"):
        planar.step_from_frames(tgt, src)
    one.desc.H[1] += 1
    with pytest.raises(TypeError, match="pyramid"):
        one.step_from_frames(tgt, src)


def test_loss_link_fast_path_for_repeated_arrays(synth, dev):
    """Round 6 (round-5 verdict item 7): a call of the link with the previous call's objects -- the same arrays at the same
    addresses: static input buffers -- skips validation and re-binding.  It must still read the CURRENT values of those arrays, give
    per-call losses and reports, respect requires_grad / no_backprop_mode, and fall back to the full path as soon as any argument is
    another object, another array, or an array that moved."""
    import torch
    d = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=3, seed=6)
    d2 = synth.make_inputs(B=2, H=32, W=104, n_src=2, n_scales=3, seed=7)
    cfgd = {"smooth_reg": 0.1, "exp_reg": 0, "seq_len": 3, "ssim_rate": 0.15}
    ref = [O.sfm_loss(x["tgt_pyr"], x["src_pyr"], x["intrinsics"], x["disps"], x["poses"], backward=True, smooth_reg=0.1, ssim_rate=0.15) for x in (d, d2)]
    link = links.SFMLearnerLoss(cfgd)
    disps = [cs.Variable(to_dev(a, dev)) for a in d["disps"]]
    poses = [cs.Variable(to_dev(a, dev)) for a in d["poses"]]
    K, tgt, src = to_dev(d["intrinsics"], dev), to_dev(d["tgt"], dev), to_dev(d["src"], dev)

    def step():
        for v in disps + poses:
            v.cleargrad()
        loss = link(tgt, src, K, K, disps, poses)
        loss.backward()
        return loss, [to_np(v.grad).copy() for v in disps + poses]

    l0, g0 = step()                                     # full path: binds
    assert link._repeat is not None
    l1, g1 = step()                                     # fast path
    assert float(l1.data) == float(l0.data) and l1 is not l0 and l1.data.data_ptr() != l0.data.data_ptr()
    for a, b in zip(g0, g1):
        np.testing.assert_array_equal(a, b)
    assert abs(float(l1.data) - ref[0].total_loss) <= 1e-4 * abs(ref[0].total_loss)
    assert float(cs.get_report(link)["total_loss"]) == float(l1.data) and cs.get_report(link)["ssim_loss"] is not None
    # new VALUES in the same arrays (what a loop with static buffers does every iteration) are read
    tgt.copy_(to_dev(d2["tgt"], dev)); src.copy_(to_dev(d2["src"], dev)); K.copy_(to_dev(d2["intrinsics"], dev))
    for v, a in zip(disps + poses, d2["disps"] + d2["poses"]):
        v.data.copy_(to_dev(a, dev))
    l2, g2 = step()
    assert abs(float(l2.data) - ref[1].total_loss) <= 1e-4 * abs(ref[1].total_loss)
    np.testing.assert_allclose(g2[-1], ref[1].d_poses[-1], rtol=0, atol=2e-3 * np.abs(ref[1].d_poses[-1]).max())
    assert float(l0.data) != float(l2.data)             # ... and the loss of an earlier call kept its value
    # no_backprop_mode and requires_grad are honoured per call
    with cs.no_backprop_mode():
        l3 = link(tgt, src, K, K, disps, poses)
    assert l3.creator is None and float(l3.data) == float(l2.data)
    # another array in one Variable: the full path again (and the right values)
    disps[0].data = to_dev(d["disps"][0], dev)
    l4, _ = step()
    assert float(l4.data) != float(l2.data)
    want = O.sfm_loss(d2["tgt_pyr"], d2["src_pyr"], d2["intrinsics"], [d["disps"][0]] + d2["disps"][1:], d2["poses"], smooth_reg=0.1, ssim_rate=0.15)
    assert abs(float(l4.data) - want.total_loss) <= 1e-4 * abs(want.total_loss)
    # a stale backward is still refused on the fast path
    la = link(tgt, src, K, K, disps, poses)
    lb = link(tgt, src, K, K, disps, poses)
    with pytest.raises(RuntimeError, match="cache_buffers"):
        la.backward()
    lb.backward()


def test_arrays_on_a_device_that_is_not_current(synth):
    """Every wrapper launches on the device its ARRAYS live on, whichever device is current (ops._launch enters a device guard only
    then): with cuda:0 current and the arrays on cuda:1, the fused loss in both layouts, ops.pyramid_pair_hwc, ops.warp_fwd and
    torch_api.sfm_learner_loss + backward() give the bits of the same calls made with cuda:1 current, and cuda:0 is still current
    afterwards.  Bitwise throughout: no d_src is asked for, and d_pose is compared bitwise as in test_buffer_contracts_gpu.py."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: the device-guard branch needs arrays on a second one")
    ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
    other = torch.device("cuda:1")
    B, H, W, S = 1, 16, 24, 2
    d = synth.make_inputs(B=B, H=H, W=W, n_src=1, n_scales=S, seed=3)
    cfg = dict(smooth_reg=0.1, ssim_rate=0.15)

    def run():
        got = []
        tgt, src, K = to_dev(d["tgt"], other), to_dev(d["src"], other), to_dev(d["intrinsics"], other)
        pair = ops.pyramid_pair_hwc(tgt, src.reshape(B, 3, H, W), S)
        got += list(pair[0]) + list(pair[1])
        for layout, pyr in (("hwc", pair), ("planar", [[to_dev(a, other) for a in d[k]] for k in ("tgt_pyr", "src_pyr")])):
            fl = ops.FusedLoss(**cfg).bind(pyr[0], pyr[1], K, [to_dev(a, other) for a in d["disps"]],
                                           [to_dev(a, other) for a in d["poses"]], layout=layout)
            got += [fl.forward_backward().clone()] + fl.d_disps + fl.d_poses
        depth = (1.0 / d["disps"][0]).reshape(B, H * W)
        got.append(ops.warp_fwd(tgt, to_dev(depth, other), to_dev(d["poses"][0], other), K[:, 0].contiguous()))
        leaves = [to_dev(a, other).requires_grad_() for a in d["disps"] + d["poses"]]
        total, terms = ta.sfm_learner_loss(tgt, src, K, leaves[:S], leaves[S:], **cfg)
        total.backward()
        got += [total, terms] + [a.grad for a in leaves]
        assert all(t.device == other for t in got)
        return [to_np(t).copy() for t in got]

    torch.cuda.set_device(0)
    got = run()
    assert torch.cuda.current_device() == 0
    with torch.cuda.device(other):
        want = run()
    assert torch.cuda.current_device() == 0 and len(got) == len(want) == 2 * S + 2 * (1 + S + 1) + 1 + 2 + S + 1
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(b).all() and np.abs(b).max() > 0, k
        np.testing.assert_array_equal(a, b, err_msg="output %d" % k)
