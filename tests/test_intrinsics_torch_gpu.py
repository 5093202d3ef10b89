"""The gradient with respect to the intrinsics through the Python layers on the MI355X: torch_api (sfm_learner_loss, the custom
operator, projective_inverse_warp, multi_scale_intrinsics), functions and links.  The values are ops.FusedLoss's d_intrinsics /
ops.warp_bwd_intrinsics (held against autograd by tests/test_intrinsics_grad_gpu.py); here they must arrive bit for bit, scaled on
the device, without a host sync, under graph capture and torch.compile."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import intrinsics_grad as IG

pytestmark = pytest.mark.gpu

ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
links = importlib.import_module("sfm-learner-chainer_amd.links")
functions = importlib.import_module("sfm-learner-chainer_amd.functions")
cs = importlib.import_module("sfm-learner-chainer_amd.chainer_surface")

CFG = dict(smooth_reg=0.1, ssim_rate=0.15)
SHAPE = (3, 24, 40, 2, 3)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _inputs(dev, d, masks=False):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    leaf = lambda a: t(a).requires_grad_()
    return dict(d=d, tgt=t(d["tgt"]), src=t(d["src"]), K=leaf(d["intrinsics"]), disps=[leaf(a) for a in d["disps"]],
                poses=[leaf(a) for a in d["poses"]], masks=[leaf(a) for a in d["masks"]] if masks else None)


def _loss(x, K=None, **cfg):
    return ta.sfm_learner_loss(x["tgt"], x["src"], x["K"] if K is None else K, x["disps"], x["poses"], x["masks"], **cfg)


def _leaves(x):
    return [x["K"]] + x["disps"] + x["poses"] + (x["masks"] or [])


def _clear(x):
    for t in _leaves(x):
        t.grad = None


def _fused(ops, x, hwc=True, **cfg):
    """ops.FusedLoss on the same arrays, as the torch route runs it: (d_intrinsics, the other gradients) for gy = 1"""
    B, n, _, H, W = x["src"].shape
    S = len(x["disps"])
    stacked = x["src"].reshape(B, 3 * n, H, W)
    det = lambda ts: [t.detach() for t in ts] if ts is not None else None
    fl = ops.FusedLoss(**cfg)
    if hwc:
        yt, ys = ops.pyramid_pair_hwc(x["tgt"], stacked, S)
        pyr = (list(yt), list(ys))
    else:
        pyr = (ops.pyramid(x["tgt"].clone(), S), ops.pyramid(stacked.clone(), S))
    fl.bind(pyr[0], pyr[1], x["K"].detach(), det(x["disps"]), det(x["poses"]), det(x["masks"]), layout="hwc" if hwc else "planar",
            want_d_intrinsics=True)
    fl.forward_backward()
    return fl.d_intrinsics.clone(), [g.clone() for g in fl.d_disps + fl.d_poses + (fl.d_masks or [])]


@pytest.mark.parametrize("case", ["ssim", "masks_reference_order"])
def test_intrinsics_grad_is_the_fused_d_intrinsics_times_the_upstream_gradient(ops, dev, case):
    cfg = dict(CFG) if case == "ssim" else dict(smooth_reg=0.1, exp_reg=0.2, projection="reference_order")
    x = _inputs(dev, IG.ramp_inputs(SHAPE, "general"), masks=case != "ssim")
    want_k, want = _fused(ops, x, **cfg)
    assert float(want_k.abs().min()) > 0
    total, _ = _loss(x, **cfg)
    total.backward()
    assert _bits(x["K"].grad, want_k)
    for g, w in zip([t.grad for t in _leaves(x)[1:]], want):
        assert _bits(g, w)
    _clear(x)
    total, _ = _loss(x, **cfg)
    (2.5 * total).backward()
    assert _bits(x["K"].grad, want_k * torch.tensor(2.5, device=dev))
    for g, w in zip([t.grad for t in _leaves(x)[1:]], want):
        assert _bits(g, w * torch.tensor(2.5, device=dev))
    _clear(x)
    opt = torch.optim.SGD(_leaves(x), lr=0.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    total, _ = _loss(x, **cfg)
    scaler.scale(total).backward()
    scaler.unscale_(opt)
    assert _bits(x["K"].grad, want_k)
    # intrinsics that do not require grad: the launches and the results of before
    _clear(x)
    total, _ = _loss(x, K=x["K"].detach(), **cfg)
    total.backward()
    assert x["K"].grad is None
    for g, w in zip([t.grad for t in _leaves(x)[1:]], want):
        assert _bits(g, w)
    # every prediction detached: no gradient launch runs, and the intrinsics get none (as before)
    total, _ = ta.sfm_learner_loss(x["tgt"], x["src"], x["K"], [t.detach() for t in x["disps"]], [t.detach() for t in x["poses"]],
                                   [t.detach() for t in x["masks"]] if x["masks"] else None, **cfg)
    _clear(x)
    total.backward()
    assert x["K"].grad is None


def test_planar_route_for_large_frames(ops, synth, dev):
    """frames of HWC_MAX_PIXELS or more: the planar pyramid + sfm_loss_fwd_bwd + sfm_loss_proj_bwd"""
    d = synth.make_inputs(B=1, H=1024, W=1376, n_src=1, n_scales=1, seed=1)
    assert 1024 * 1376 >= links.HWC_MAX_PIXELS
    x = _inputs(dev, d)
    want_k, _ = _fused(ops, x, hwc=False, **CFG)
    total, _ = _loss(x, **CFG)
    total.backward()
    assert _bits(x["K"].grad, want_k) and bool((want_k != 0).any())


def test_a_focal_and_centre_parameter_receives_its_gradient(ops, dev):
    d = IG.ramp_inputs(SHAPE, None)           # synth's own cameras ARE multi_scale_intrinsics of scale 0
    x = _inputs(dev, d)
    K0 = torch.from_numpy(d["intrinsics"][:, 0]).to(dev)
    f = torch.stack([K0[:, 0, 0], K0[:, 1, 1], K0[:, 0, 2], K0[:, 1, 2]], dim=1).requires_grad_()
    K = ta.multi_scale_intrinsics(f, SHAPE[4])
    assert _bits(K, x["K"])
    want_k, _ = _fused(ops, x, **CFG)
    total, _ = _loss(x, K=K, **CFG)
    total.backward()
    div = torch.tensor([1.0, 0.5, 0.25], device=dev)[None, :]
    expect = torch.stack([(want_k[:, :, 0, 0] * div).sum(1), (want_k[:, :, 1, 1] * div).sum(1), (want_k[:, :, 0, 2] * div).sum(1),
                          (want_k[:, :, 1, 2] * div).sum(1)], dim=1)
    assert f.grad is not None and f.grad.shape == (SHAPE[0], 4)
    torch.testing.assert_close(f.grad, expect, rtol=1e-5, atol=0)
    assert float(f.grad.abs().min()) > 0


def test_the_step_never_syncs(dev):
    d = IG.ramp_inputs(SHAPE, None)
    x = _inputs(dev, d)
    K0 = torch.from_numpy(d["intrinsics"][:, 0]).to(dev)
    f = torch.stack([K0[:, 0, 0], K0[:, 1, 1], K0[:, 0, 2], K0[:, 1, 2]], dim=1).requires_grad_()
    total, _ = _loss(x, **CFG)                     # warm: plans, allocator blocks
    total.backward()
    _clear(x)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, terms = _loss(x, **CFG)
        total.backward()
        total2, _ = _loss(x, K=ta.multi_scale_intrinsics(f, SHAPE[4]), **CFG)      # a parameter on the way, too
        total2.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(x["K"].grad).all() and torch.isfinite(f.grad).all() and bool((f.grad != 0).all())


def test_graph_capture_with_a_static_K(dev):
    """the captured-step recipe of INTEGRATION.md 5 with the intrinsics among the static tensors that receive a gradient"""
    x = _inputs(dev, IG.ramp_inputs(SHAPE, "general", seed=3))
    news = [_inputs(dev, IG.ramp_inputs(SHAPE, "general", seed=s)) for s in (4, 5)]
    static = [x["tgt"], x["src"]] + [t.detach() for t in _leaves(x)]

    def run():
        total, terms = _loss(x, **CFG)
        total.backward()
        return total, terms

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
            _clear(x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        total, terms = run()
    grads = [t.grad for t in _leaves(x)]
    for y in news:
        with torch.no_grad():
            for dst, src in zip(static, [y["tgt"], y["src"]] + _leaves(y)):
                dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        et, _ = _loss(y, **CFG)
        et.backward()
        assert _bits(total, et)
        for a, b in zip(grads, [t.grad for t in _leaves(y)]):
            assert _bits(a, b)
        assert bool((y["K"].grad != 0).all())
    del g


def test_torch_compile_without_graph_break(dev):
    x = _inputs(dev, IG.ramp_inputs(SHAPE, "general"))
    total, terms = _loss(x, **CFG)
    total.backward()
    want, want_grads = total.detach(), [t.grad.clone() for t in _leaves(x)]
    _clear(x)

    def step(tgt, src, K, disps, poses):
        return ta.sfm_learner_loss(tgt, src, K, disps, poses, smooth_reg=0.1, ssim_rate=0.15)

    torch._dynamo.reset()
    compiled = torch.compile(step, backend="aot_eager", fullgraph=True)
    total, terms = compiled(x["tgt"], x["src"], x["K"], x["disps"], x["poses"])
    (2.5 * total).backward()
    assert _bits(total, want)
    for t, w in zip(_leaves(x), want_grads):
        assert _bits(t.grad, w * torch.tensor(2.5, device=dev))
    # the custom operator and its registered autograd, eagerly: what torch.compile traces
    _clear(x)
    B, n, _, H, W = x["src"].shape
    total, terms, unit = torch.ops.sfmwarp.sfm_learner_loss_k(x["tgt"], x["src"].reshape(B, 3 * n, H, W), x["K"], x["disps"], x["poses"],
                                                              [], 0.1, 0.0, 0.15, 1, 0, B, True)
    total.backward()
    for t, w in zip(_leaves(x), want_grads):
        assert _bits(t.grad, w)


# ---------------------------------------------------------------------------------------------------------------------------
# the operators and the Chainer-style surface
# ---------------------------------------------------------------------------------------------------------------------------
def _warp_arrays(dev):
    from test_intrinsics_grad_gpu import warp_case
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in warp_case(3, 3)]


def test_projective_inverse_warp_returns_d_K(ops, dev):
    imgs, depth, pose, K, g = _warp_arrays(dev)
    want = ops.warp_bwd_intrinsics(imgs, depth, pose, K, g)
    d_depth, d_pose, _ = ops.warp_bwd(imgs, depth, pose, K, g)
    dp, po, Kl = depth.clone().requires_grad_(), pose.clone().requires_grad_(), K.clone().requires_grad_()
    ta.projective_inverse_warp(imgs, dp, po, Kl).backward(g)
    assert _bits(Kl.grad, want) and _bits(dp.grad, d_depth) and _bits(po.grad, d_pose) and bool((want != 0).all())
    # the Chainer-style Function: K as a Variable receives it, K as an array (the reference's call) costs nothing
    V = cs.Variable
    vK = V(K.clone())
    out = functions.projective_inverse_warp(V(imgs, requires_grad=False), V(depth.clone()), V(pose.clone()), vK)
    out.grad = g
    out.backward()
    assert _bits(vK.grad, want)
    vd = V(depth.clone())
    out = functions.projective_inverse_warp(imgs, vd, V(pose.clone()), K)
    out.grad = g
    out.backward()
    assert _bits(vd.grad, d_depth)


def test_proj_tgt_to_src_returns_d_K(ops, dev):
    _, _, pose, K, _ = _warp_arrays(dev)
    g = torch.randn((pose.shape[0], 4, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    want = ops.pose_proj_bwd_intrinsics(pose, K, g)
    vp, vK = cs.Variable(pose.clone()), cs.Variable(K.clone())
    out = functions.proj_tgt_to_src(vp, vK)
    out.grad = g
    out.backward()
    assert _bits(vK.grad, want) and _bits(vp.grad, ops.pose_proj_bwd(pose, K, g))
    err = IG.worst(want.cpu().numpy(), IG.d_k_of_proj(pose.cpu().numpy(), g.cpu().numpy()))
    assert err <= 1e-5, err


@pytest.mark.parametrize("use_graph", [False, True])
def test_the_link_fills_intrinsics_grad(ops, dev, use_graph):
    d = IG.ramp_inputs(SHAPE, "general")
    x = _inputs(dev, d)
    want_k, want = _fused(ops, x, **CFG)
    V = cs.Variable
    link = links.SFMLearnerLoss(dict(seq_len=SHAPE[3] + 1, smooth_reg=0.1, exp_reg=0.0, ssim_rate=0.15), use_graph=use_graph)
    K = V(x["K"].detach().clone())
    disps, poses = [V(t.detach().clone()) for t in x["disps"]], [V(t.detach().clone()) for t in x["poses"]]
    for _ in range(3):                       # the first call binds, a repeated call takes the fast path / replays the graph
        for v in [K] + disps + poses:
            v.cleargrad()
        loss = link(x["tgt"], x["src"], K, None, disps, poses)
        loss.backward()
        assert _bits(K.grad, want_k)
        for v, w in zip(disps + poses, want):
            assert _bits(v.grad, w)
    # a loss scale set by the caller reaches it; an array (the reference's call) gets nothing and costs nothing
    K.cleargrad()
    loss = link(x["tgt"], x["src"], K, None, disps, poses)
    loss.grad = torch.tensor(2.5, device=dev)
    loss.backward()
    assert _bits(K.grad, want_k * torch.tensor(2.5, device=dev))
    loss = link(x["tgt"], x["src"], x["K"].detach(), None, disps, poses)
    loss.backward()
    assert link._cache and all(st.fused.d_intrinsics is None for st in link._cache.values())


def test_integration_example_of_learned_intrinsics_runs(dev):
    """INTEGRATION.md 5, the learned-intrinsics block, as written"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    blocks = re.findall(r"```py\n(.*?)```", text[text.index("## 5. From a PyTorch training loop"):], flags=re.S)
    assert len(blocks) == 1
    d = IG.ramp_inputs(SHAPE, None)
    x = _inputs(dev, d)
    env = dict(torch=torch, ta=ta, tgt_img=x["tgt"], src_imgs=x["src"], pred_disps=x["disps"], pred_poses=x["poses"],
               K0=torch.from_numpy(d["intrinsics"][:, 0]).to(dev))
    exec(compile(blocks[0], "INTEGRATION.md#5-intrinsics", "exec"), env)
    assert env["calib"].grad is not None and bool((env["calib"].grad != 0).all()) and torch.isfinite(env["total"])
