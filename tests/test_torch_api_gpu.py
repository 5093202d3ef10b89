"""sfmwarp.torch_api on the MI355X: the autograd route gives the fused loss's own values and gradients bit for bit, scales them on
the device (loss scaling, GradScaler, graph capture, no host sync), keeps every call's gradients apart, trains a torch.nn network,
compiles without a graph break, takes autocast's bf16 outputs, and its scale kernel is exact at its edges."""
import importlib

import numpy as np
import pytest
import torch

from oracle import parity
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
links = importlib.import_module("sfm-learner-chainer_amd.links")
cs = importlib.import_module("sfm-learner-chainer_amd.chainer_surface")

CFG = dict(smooth_reg=0.1, ssim_rate=0.15)


def _bits(a, b):
    """bitwise equality of two float tensors (NaN payloads and the sign of zero included)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[a.dtype]
    return torch.equal(a.detach().contiguous().view(it), b.detach().contiguous().view(it))


def _inputs(synth, dev, B=2, H=32, W=104, n_src=2, S=2, seed=1, with_masks=False):
    d = synth.make_inputs(B=B, H=H, W=W, n_src=n_src, n_scales=S, seed=seed, with_masks=with_masks)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    leaf = lambda a: t(a).requires_grad_()
    return dict(d=d, tgt=t(d["tgt"]), src=t(d["src"]), K=t(d["intrinsics"]), disps=[leaf(a) for a in d["disps"]],
                poses=[leaf(a) for a in d["poses"]], masks=[leaf(a) for a in d["masks"]] if with_masks else None)


def _loss(x, **cfg):
    return ta.sfm_learner_loss(x["tgt"], x["src"], x["K"], x["disps"], x["poses"], x["masks"], **cfg)


def _leaves(x):
    return x["disps"] + x["poses"] + (x["masks"] or [])


def _grads(x):
    return [t.grad.clone() for t in _leaves(x)]


def _clear(x):
    for t in _leaves(x):
        t.grad = None


def _fused(ops, x, hwc, **cfg):
    """ops.FusedLoss.forward_backward on the same inputs: loss5 and the gradients for gy = 1"""
    tgt, src = x["tgt"], x["src"]
    B, n, _, H, W = src.shape
    S = len(x["disps"])
    stacked = src.reshape(B, 3 * n, H, W)
    fl = ops.FusedLoss(**cfg)
    det = lambda ts: [t.detach() for t in ts] if ts is not None else None
    if hwc:
        yt, ys = ops.pyramid_pair_hwc(tgt, stacked, S)
        fl.bind(list(yt), list(ys), x["K"], det(x["disps"]), det(x["poses"]), det(x["masks"]), layout="hwc")
    else:
        fl.bind(ops.pyramid(tgt.clone(), S), ops.pyramid(stacked.clone(), S), x["K"], det(x["disps"]), det(x["poses"]),
                det(x["masks"]), layout="planar")
    loss5 = fl.forward_backward().clone()
    return loss5, [g.clone() for g in fl.d_disps + fl.d_poses + (fl.d_masks or [])]


@pytest.mark.parametrize("case", ["hwc", "planar", "masks", "ssim_edge", "reference_order"])
def test_matches_fused_loss_bitwise(ops, synth, dev, case):
    shape, cfg = dict(), dict(CFG)
    if case == "planar":                 # 1024 x 1376 = 1.41 M pixels >= links.HWC_MAX_PIXELS: pyramid + sfm_loss_fwd_bwd
        shape = dict(B=1, H=1024, W=1376)
    if case == "masks":                  # odometry: four sources + explainability
        shape = dict(n_src=4, S=3, with_masks=True)
        cfg["exp_reg"] = 0.2
    if case == "ssim_edge":
        cfg.update(ssim_rate=0.85, smooth_mode="edge_aware")
    if case == "reference_order":
        cfg["projection"] = "reference_order"
    x = _inputs(synth, dev, **shape)
    assert (x["tgt"].shape[2] * x["tgt"].shape[3] < links.HWC_MAX_PIXELS) == (case != "planar")
    total, terms = _loss(x, **cfg)
    total.backward()
    loss5, want = _fused(ops, x, case != "planar", **cfg)
    assert total.shape == () and terms.shape == (4,) and not terms.requires_grad
    assert _bits(total, loss5[0]) and _bits(terms, loss5[1:])
    got = _grads(x)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert _bits(g, w), k


def test_loss_scaling_and_grad_scaler(synth, dev):
    x = _inputs(synth, dev)
    total, _ = _loss(x, **CFG)
    total.backward()
    unit = _grads(x)
    _clear(x)
    total, _ = _loss(x, **CFG)
    (2.5 * total).backward()
    for g, u in zip(_grads(x), unit):
        assert _bits(g, u * torch.tensor(2.5, device=dev))
    _clear(x)
    total, _ = _loss(x, **CFG)
    total.backward(torch.zeros((), device=dev))
    assert all(bool((g == 0).all()) for g in _grads(x))
    _clear(x)
    opt = torch.optim.SGD(_leaves(x), lr=0.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    total, _ = _loss(x, **CFG)
    scaler.scale(total).backward()
    scaler.unscale_(opt)
    for g, u in zip(_grads(x), unit):
        assert _bits(g, u)


def test_forward_and_backward_never_sync(synth, dev):
    x = _inputs(synth, dev)
    total, _ = _loss(x, **CFG)          # warm: plans, allocator blocks
    total.backward()
    _clear(x)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, terms = _loss(x, **CFG)
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(terms).all()


def test_two_forwards_keep_their_own_gradients(synth, dev):
    a, b = _inputs(synth, dev, seed=1), _inputs(synth, dev, seed=2)
    singles = []
    for x in (a, b):
        total, _ = _loss(x, **CFG)
        total.backward()
        singles.append(_grads(x))
        _clear(x)
    ta_, _ = _loss(a, **CFG)
    tb_, _ = _loss(b, **CFG)
    (ta_ + tb_).backward()
    for x, single in zip((a, b), singles):
        for g, w in zip(_grads(x), single):
            assert _bits(g, w)


class _Net(torch.nn.Module):
    """stand-in for DispNet + PoseNet: 4-scale disparities through disp_activation, packed (B, 6 n_src) poses"""

    def __init__(self, n_src, S):
        super().__init__()
        self.body = torch.nn.Conv2d(3 * (1 + n_src), 8, 3, padding=1)
        self.heads = torch.nn.ModuleList([torch.nn.Conv2d(8, 1, 3, padding=1) for _ in range(S)])
        self.pose = torch.nn.Conv2d(8, 6 * n_src, 1)

    def forward(self, tgt, stacked):
        h = torch.tanh(self.body(torch.cat([tgt, stacked], 1)))
        logits = [head(torch.nn.functional.avg_pool2d(h, 2 ** s) if s else h) for s, head in enumerate(self.heads)]
        return ta.disp_activation(logits), 0.01 * self.pose(h).mean((2, 3))


def test_trains_a_network_like_the_manual_route(synth, dev):
    x = _inputs(synth, dev, B=2, H=32, W=96, S=4)
    B, n, _, H, W = x["src"].shape
    stacked = x["src"].reshape(B, 3 * n, H, W)
    torch.manual_seed(0)
    net = _Net(n, 4).to(dev)
    config = dict(smooth_reg=0.1, exp_reg=0.0, ssim_rate=0.15, seq_len=n + 1)
    # the torch route
    loss = ta.SFMLearnerLoss(config)
    disps, pose = net(x["tgt"], stacked)
    total = loss(x["tgt"], x["src"], x["K"], None, disps, pose)
    total.backward()
    got = [p.grad.clone() for p in net.parameters()]
    assert set(loss.last_report) == {"total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss"}
    # the manual route: Chainer-surface link, then torch.autograd.backward(outputs, grads)
    net.zero_grad(set_to_none=True)
    disps, pose = net(x["tgt"], stacked)
    poses = list(pose.split(6, 1))
    vd, vp = [cs.Variable(d.detach()) for d in disps], [cs.Variable(p.detach()) for p in poses]
    link = links.SFMLearnerLoss(config, cache_buffers=False)
    lv = link(x["tgt"], x["src"], x["K"], None, vd, vp)
    lv.backward()
    torch.autograd.backward(disps + poses, [v.grad for v in vd + vp])
    assert _bits(total.detach(), lv.data)
    for g, p in zip(got, net.parameters()):
        w = p.grad
        assert float((g - w).abs().max()) <= 1e-6 * float(w.abs().max()) + 1e-30
    # one optimizer step on the torch route's gradients
    for g, p in zip(got, net.parameters()):
        p.grad = g
    before = [p.detach().clone() for p in net.parameters()]
    torch.optim.SGD(net.parameters(), lr=0.1).step()
    assert any(not torch.equal(a, p) for a, p in zip(before, net.parameters()))
    assert all(torch.isfinite(p).all() for p in net.parameters())


def test_torch_compile_without_graph_break(synth, dev):
    x = _inputs(synth, dev)
    total, terms = _loss(x, **CFG)
    total.backward()
    want, want_terms, want_grads = total.detach(), terms, _grads(x)
    _clear(x)

    def step(tgt, src, K, disps, poses):
        return ta.sfm_learner_loss(tgt, src, K, disps, poses, smooth_reg=0.1, ssim_rate=0.15)

    torch._dynamo.reset()
    compiled = torch.compile(step, backend="aot_eager", fullgraph=True)
    total, terms = compiled(x["tgt"], x["src"], x["K"], x["disps"], x["poses"])
    total.backward()
    assert _bits(total, want) and _bits(terms, want_terms)
    for g, w in zip(_grads(x), want_grads):
        assert _bits(g, w)
    # the custom operator and its registered autograd, eagerly: what torch.compile traces
    _clear(x)
    B, n, _, H, W = x["src"].shape
    total, terms, unit = torch.ops.sfmwarp.sfm_learner_loss(x["tgt"], x["src"].reshape(B, 3 * n, H, W), x["K"], x["disps"], x["poses"],
                                                            [], 0.1, 0.0, 0.15, 1, 0, B, True)
    total.backward()
    assert _bits(total, want) and _bits(terms, want_terms) and not unit.requires_grad
    for g, w in zip(_grads(x), want_grads):
        assert _bits(g, w)


def test_graph_capture_replays_bitwise(synth, dev):
    x = _inputs(synth, dev, seed=1)
    news = [_inputs(synth, dev, seed=s) for s in (2, 3, 4)]
    static = [x["tgt"], x["src"], x["K"]] + [t.detach() for t in _leaves(x)]

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
            for dst, src in zip(static, [y["tgt"], y["src"], y["K"]] + _leaves(y)):
                dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        et, eterms = _loss(y, **CFG)
        et.backward()
        assert _bits(total, et) and _bits(terms, eterms)
        for a, b in zip(grads, _grads(y)):
            assert _bits(a, b)
    del g


def test_autocast_bf16_outputs(synth, dev):
    x = _inputs(synth, dev)
    d16 = [t.detach().to(torch.bfloat16).requires_grad_() for t in x["disps"]]
    p16 = [t.detach().to(torch.bfloat16).requires_grad_() for t in x["poses"]]
    with torch.autocast("cuda", torch.bfloat16):
        total, terms = ta.sfm_learner_loss(x["tgt"], x["src"], x["K"], d16, p16, **CFG)
    total.backward()
    d32 = [t.detach().float().requires_grad_() for t in d16]
    p32 = [t.detach().float().requires_grad_() for t in p16]
    t32, terms32 = ta.sfm_learner_loss(x["tgt"], x["src"], x["K"], d32, p32, **CFG)
    t32.backward()
    assert total.dtype == torch.float32 and _bits(total, t32) and _bits(terms, terms32)
    for a, b in zip(d16 + p16, d32 + p32):
        assert a.grad.dtype == torch.bfloat16 and _bits(a.grad, b.grad.to(torch.bfloat16))


def test_matches_the_oracle(synth, dev):
    """the criteria of tests/test_loss_gpu.py (and smoke()): scalars 1e-4 relative; d_pose 2e-3 of its maximum element-wise and 1e-3
    in relative L2; d_disp 2e-3 element-wise and 1e-4 in relative L2 outside the knife-edge pixels the oracle names"""
    x = _inputs(synth, dev)
    d = x["d"]
    total, terms = _loss(x, **CFG)
    total.backward()
    ref = O.sfm_loss(d["tgt_pyr"], d["src_pyr"], d["intrinsics"], d["disps"], d["poses"], backward=True, keep_warped=True, **CFG)
    got = torch.cat([total.detach().reshape(1), terms]).cpu().numpy()
    want = np.array([ref[k] for k in ("total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss")])
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-7)
    for p, w in zip(x["poses"], ref["d_poses"]):
        g = p.grad.cpu().numpy()
        np.testing.assert_allclose(g, w, rtol=0, atol=2e-3 * np.abs(w).max())
        assert parity.rel_l2(g, w) <= 1e-3
    for s, (p, w) in enumerate(zip(x["disps"], ref["d_disps"])):
        g = p.grad.cpu().numpy()
        knife = parity.knife_mask(ref, s)[0][:, None]
        assert knife.mean() <= 0.05
        assert (np.abs(g - w) * ~knife).max() <= 2e-3 * np.abs(w).max()
        assert parity.rel_l2(g, w, knife) <= 1e-4


def test_operator_functions_match_ops_bitwise(ops, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    N, Cc, H, W = 2, 3, 24, 40
    imgs = torch.rand((N, Cc, H, W), device=dev, generator=gen).mul_(2).sub_(1).requires_grad_()
    depth = (1.0 + 4 * torch.rand((N, 3, H * W), device=dev, generator=gen)).requires_grad_()
    pose = (0.02 * torch.randn((N, 6), device=dev, generator=gen)).requires_grad_()
    K = torch.tensor([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]], device=dev).expand(N, 3, 3).contiguous()
    out = ta.projective_inverse_warp(imgs, depth, pose, K)
    assert _bits(out, ops.warp_fwd(imgs.detach(), depth.detach(), pose.detach(), K))
    g = torch.randn(out.shape, device=dev, generator=gen)
    out.backward(g)
    d_depth, d_pose, d_src = ops.warp_bwd(imgs.detach(), depth.detach(), pose.detach(), K, g, want_d_src=True)
    assert _bits(depth.grad, d_depth) and _bits(pose.grad, d_pose)
    # d_src is accumulated with float atomics (include/sfmwarp.h): the order of the adds, hence the last bits, may differ by run
    torch.testing.assert_close(imgs.grad, d_src, rtol=1e-5, atol=1e-6)

    xs = [torch.randn((N, 1, H >> s, W >> s), device=dev, generator=gen).requires_grad_() for s in range(4)]
    ys = ta.disp_activation(xs)
    want = ops.disp_act_fwd([t.detach() for t in xs])
    assert all(_bits(a, b) for a, b in zip(ys, want))
    gs = [torch.randn(y.shape, device=dev, generator=gen) for y in ys]
    torch.autograd.backward(ys, gs)
    assert all(_bits(t.grad, w) for t, w in zip(xs, ops.disp_act_bwd(want, gs)))


@pytest.mark.parametrize("gyv", [0.7, -0.0, float("inf"), float("nan")])
def test_scale_arrays_edges(dev, gyv):
    gen = torch.Generator(device=dev).manual_seed(5)
    gy = torch.tensor(gyv, device=dev)
    base = torch.randn((4096,), device=dev, generator=gen)
    base[7] = 0.0
    sizes = [0, 1, 3, 5, 64, 1000]
    xs, outs = [], []
    off = 0
    for k, n in enumerate(sizes):             # views at odd float offsets; outputs co-aligned with their input or not
        xs.append(base[off + 1:off + 1 + n])
        outs.append(torch.empty((n + 8,), device=dev)[1 + (k % 3):1 + (k % 3) + n])
        off += n + 3
    ta.scale_arrays_into(xs, outs, gy)
    for x, y in zip(xs, outs):
        assert _bits(y, x * gy)
    # in place
    xi = [x.clone() for x in xs]
    ta.scale_arrays_into(xi, xi, gy)
    for x, y in zip(xs, xi):
        assert _bits(y, x * gy)
    # 32 arrays in one call
    sizes = torch.randint(0, 3000, (32,), generator=torch.Generator().manual_seed(7)).tolist()
    many = [torch.randn((n,), device=dev, generator=gen) for n in sizes]
    res = [torch.empty_like(t) for t in many]
    ta.scale_arrays_into(many, res, gy)
    assert all(_bits(y, x * gy) for x, y in zip(many, res))
    # the custom op: spans of one flat buffer
    out = torch.ops.sfmwarp.scale_arrays(base, [0, 5, 64, 1000, 2048, 3], gy)
    for o, n in ((0, 5), (64, 1000), (2048, 3)):
        assert _bits(out[o:o + n], base[o:o + n] * gy)


def test_scale_arrays_64_bit_indexing(dev):
    n = (1 << 31) + 3                         # 8.6 GB of floats: vector indices and byte offsets beyond 32 bits
    x = torch.empty((n,), device=dev).uniform_(-1, 1)
    y = torch.empty_like(x)
    gy = torch.tensor(1.5, device=dev)
    ta.scale_arrays_into([x], [y], gy)
    step = 1 << 28
    for i in range(0, n, step):
        assert _bits(y[i:i + step], x[i:i + step] * gy), i
    del x, y
    torch.cuda.empty_cache()


def test_scale_arrays_shares_the_block_cap_across_arrays(dev):
    """More than 2048 blocks' worth of work over several arrays (cfg3's gradient set needs about 2200): the launch deals the capped
    grid out in proportion to the arrays' lengths, and every array is still scaled in full."""
    gen = torch.Generator(device=dev).manual_seed(11)
    gy = torch.tensor(-1.25, device=dev)
    sizes = [1_200_003, 5, 1_100_001, 3, 700_000, 192]
    base = torch.randn((sum(sizes) + 64,), device=dev, generator=gen)
    xs, off = [], 1                            # odd float offsets: scalar heads and tails in every array
    for n in sizes:
        xs.append(base[off:off + n])
        off += n + 1
    assert sum(-(-n // 1024) for n in sizes) > 2048
    ys = [torch.empty((n,), device=dev) for n in sizes]
    ta.scale_arrays_into(xs, ys, gy)
    assert all(_bits(y, x * gy) for x, y in zip(xs, ys))
    xi = [x.clone() for x in xs]
    ta.scale_arrays_into(xi, xi, gy)
    assert all(_bits(y, x * gy) for x, y in zip(xs, xi))


def test_retain_graph_and_a_second_backward(synth, dev):
    x = _inputs(synth, dev)
    total, _ = _loss(x, **CFG)
    total.backward(retain_graph=True)
    unit = _grads(x)
    total.backward()                           # the saved unit gradients are still there: .grad accumulates them again
    for g, u in zip(_grads(x), unit):
        assert _bits(g, u + u)
    with pytest.raises(RuntimeError):          # ... and freed after a backward without retain_graph
        total.backward()


def test_constant_images_get_no_gradient(synth, dev):
    """Only an image or the intrinsics require grad: the loss has a grad_fn, its backward runs and hands out no gradient."""
    x = _inputs(synth, dev)
    tgt = x["tgt"].clone().requires_grad_()
    K = x["K"].clone().requires_grad_()
    disps, poses = [t.detach() for t in x["disps"]], [t.detach() for t in x["poses"]]
    total, _ = ta.sfm_learner_loss(tgt, x["src"], K, disps, poses, **CFG)
    assert total.requires_grad
    total.backward()
    assert tgt.grad is None and K.grad is None


def test_disp_activation_takes_autocast_logits(ops, dev):
    gen = torch.Generator(device=dev).manual_seed(9)
    xs = [torch.randn((2, 1, 32 >> s, 96 >> s), device=dev, generator=gen).to(torch.bfloat16).requires_grad_() for s in range(4)]
    ys = ta.disp_activation(xs)
    want = ops.disp_act_fwd([t.detach().float() for t in xs])
    assert all(y.dtype == torch.float32 and _bits(y, w) for y, w in zip(ys, want))
    gs = [torch.randn(y.shape, device=dev, generator=gen) for y in ys]
    torch.autograd.backward(ys, gs)
    for t, w in zip(xs, ops.disp_act_bwd(want, gs)):
        assert t.grad.dtype == torch.bfloat16 and _bits(t.grad, w.to(torch.bfloat16))


def _integration_blocks():
    """The python blocks of INTEGRATION.md §5, in order."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    section = text[text.index("## 5. From a PyTorch training loop"):]
    return re.findall(r"```python\n(.*?)```", section, flags=re.S)


def test_integration_examples_run(synth, dev):
    """INTEGRATION.md §5 as written: the training loop (bf16 autocast, GradScaler) and the captured step, on two synthetic batches."""
    blocks = _integration_blocks()
    assert len(blocks) == 2
    batches = []
    for seed in (1, 2):
        x = _inputs(synth, dev, B=2, H=32, W=96, S=4, seed=seed)
        batches.append((x["tgt"], x["src"], x["K"]))
    env = {"loader": batches}
    exec(compile(blocks[0], "INTEGRATION.md#5-loop", "exec"), env)
    assert torch.isfinite(env["total"]).all() and env["total"].dtype == torch.float32
    assert set(env["log"]) == {"total_loss", "pixel_loss", "smooth_loss", "exp_loss", "ssim_loss"}
    before = [p.detach().clone() for p in env["net"].parameters()]
    exec(compile(blocks[1], "INTEGRATION.md#5-captured", "exec"), env)
    torch.cuda.synchronize()
    assert torch.isfinite(env["static_total"]).all()
    assert any(not torch.equal(a, p) for a, p in zip(before, env["net"].parameters()))
