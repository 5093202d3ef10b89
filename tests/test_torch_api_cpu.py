"""sfmwarp.torch_api without a GPU: the custom operators are registered and trace under FakeTensorMode, bad inputs are refused
before anything is launched, and sfm_scale_arrays validates its arguments before any HIP call."""
import ctypes as C
import importlib

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
_lib = importlib.import_module("sfm-learner-chainer_amd._lib")


def test_import_registers_the_operators():
    assert hasattr(torch.ops.sfmwarp, "sfm_learner_loss")
    assert hasattr(torch.ops.sfmwarp, "scale_arrays")


def _round(n):
    return -(-n // 64) * 64


@pytest.mark.parametrize("B,H,W,S,n,with_masks", [(32, 128, 416, 4, 2, False),     # cfg3
                                                  (4, 128, 416, 4, 4, True)])      # odometry: 4 sources + explainability
def test_fake_loss_op_shapes(B, H, W, S, n, with_masks):
    with FakeTensorMode():
        f = dict(device="cuda", dtype=torch.float32)
        tgt, src, K = torch.empty(B, 3, H, W, **f), torch.empty(B, 3 * n, H, W, **f), torch.empty(B, S, 3, 3, **f)
        disps = [torch.empty(B, 1, H >> s, W >> s, **f) for s in range(S)]
        poses = [torch.empty(B, 6, **f) for _ in range(n)]
        masks = [torch.empty(B, n, H >> s, W >> s, **f) for s in range(S)] if with_masks else []
        for grad in (True, False):
            total, terms, unit = torch.ops.sfmwarp.sfm_learner_loss(tgt, src, K, disps, poses, masks, 0.1, 0.2 if with_masks else 0.,
                                                                    0.15, _lib.SMOOTH_SECOND_ORDER, 0, B, grad)
            want = sum(_round(B * (H >> s) * (W >> s)) for s in range(S)) + n * _round(B * 6)
            if with_masks:
                want += sum(_round(B * n * (H >> s) * (W >> s)) for s in range(S))
            assert total.shape == () and terms.shape == (4,)
            assert unit.shape == ((want,) if grad else (0,))
            assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in (total, terms, unit))
            scaled = torch.ops.sfmwarp.scale_arrays(unit, [0, 5] if grad else [], total)
            assert scaled.shape == unit.shape and scaled.dtype == torch.float32


def _args(dev="cpu", B=2, H=16, W=24, S=2, n=2):
    return (torch.zeros(B, 3, H, W, device=dev), torch.zeros(B, n, 3, H, W, device=dev), torch.zeros(B, S, 3, 3, device=dev),
            [torch.zeros(B, 1, H >> s, W >> s, device=dev) for s in range(S)], [torch.zeros(B, 6, device=dev) for _ in range(n)])


def test_cpu_tensors_are_refused():
    with pytest.raises(TypeError, match="CPU"):
        ta.sfm_learner_loss(*_args(), smooth_reg=0.1)
    loss = ta.SFMLearnerLoss(dict(smooth_reg=0.1, exp_reg=0.0, seq_len=3))
    with pytest.raises(TypeError, match="CPU"):
        loss(*_args()[:3], None, *_args()[3:])
    with pytest.raises(TypeError, match="CPU"):
        ta.scale_arrays_into([torch.zeros(4)], [torch.zeros(4)], torch.ones(()))


def test_wrong_shapes_and_settings_are_refused_before_any_launch():
    """Shapes are checked on tensors that never reach the device: with fake CUDA tensors any launch would fail differently."""
    with FakeTensorMode():
        tgt, src, K, disps, poses = _args("cuda")
        with pytest.raises(TypeError, match="pred_disps\\[1\\]"):
            ta.sfm_learner_loss(tgt, src, K, [disps[0], disps[0]], poses, smooth_reg=0.1)
        with pytest.raises(TypeError, match="poses"):
            ta.sfm_learner_loss(tgt, src, K, disps, poses[:1], smooth_reg=0.1)
        with pytest.raises(TypeError, match="pred_poses"):
            ta.sfm_learner_loss(tgt, src, K, disps, torch.zeros(2, 18, device="cuda"), smooth_reg=0.1)
        with pytest.raises(TypeError, match="intrinsics"):
            ta.sfm_learner_loss(tgt, src, K[:, :1], disps, poses, smooth_reg=0.1)
        with pytest.raises(TypeError, match="tgt_img"):
            ta.sfm_learner_loss(tgt[:, :2], src, K, disps, poses, smooth_reg=0.1)
        with pytest.raises(TypeError, match="dtype"):
            ta.sfm_learner_loss(tgt, src, K, [d.to(torch.float64) for d in disps], poses, smooth_reg=0.1)
        with pytest.raises(ValueError, match="explainability"):
            ta.sfm_learner_loss(tgt, src, K, disps, poses, smooth_reg=0.1, exp_reg=0.2)
        with pytest.raises(ValueError, match="smooth_mode"):
            ta.sfm_learner_loss(tgt, src, K, disps, poses, smooth_reg=0.1, smooth_mode="third_order")
        with pytest.raises(TypeError, match="seq_len"):
            ta.SFMLearnerLoss(dict(smooth_reg=0.1, exp_reg=0.0, seq_len=4))(tgt, src, K, None, disps, poses)


def test_scale_arrays_rejects_bad_arguments_through_the_c_abi():
    L = _lib.lib
    fake = C.c_void_p(0x1000)
    ptrs = (C.c_void_p * 33)(*([0x1000] * 33))
    n = (C.c_longlong * 33)(*([4] * 33))
    assert L.sfm_scale_arrays(None, ptrs, n, 1, fake, None) == _lib.ERR_NULL
    assert L.sfm_scale_arrays(ptrs, None, n, 1, fake, None) == _lib.ERR_NULL
    assert L.sfm_scale_arrays(ptrs, ptrs, None, 1, fake, None) == _lib.ERR_NULL
    assert L.sfm_scale_arrays(ptrs, ptrs, n, 0, fake, None) == _lib.ERR_SHAPE and "n=0" in _lib.last_error()
    assert L.sfm_scale_arrays(ptrs, ptrs, n, 33, fake, None) == _lib.ERR_SHAPE and "n=33" in _lib.last_error()
    assert L.sfm_scale_arrays(ptrs, ptrs, n, 1, None, None) == _lib.ERR_NULL and "gy" in _lib.last_error()
    neg = (C.c_longlong * 2)(4, -1)
    assert L.sfm_scale_arrays(ptrs, ptrs, neg, 2, fake, None) == _lib.ERR_SHAPE and "numel[1]" in _lib.last_error()
    nulls = (C.c_void_p * 2)(0x1000, None)
    assert L.sfm_scale_arrays(ptrs, nulls, n, 2, fake, None) == _lib.ERR_NULL and "array 1" in _lib.last_error()
    # an empty array may be NULL, and nothing at all to scale launches nothing (no device needed)
    zero = (C.c_longlong * 2)(0, 0)
    assert L.sfm_scale_arrays(nulls, nulls, zero, 2, fake, None) == 0


@pytest.mark.parametrize("spans", [[0], [0, 4, 8], [0, 1] * 33, [-1, 4], [0, -1], [60, 5], [0, 65]])
def test_scale_arrays_op_refuses_spans_outside_its_buffer(spans):
    """The spans of sfmwarp::scale_arrays are checked on the host before anything else: odd length, more than 32 pairs, a negative
    offset or length, or a span past the end of x (64 elements here) would make the kernel read and write outside the buffers."""
    x, gy = torch.zeros(64), torch.ones(())
    with pytest.raises(TypeError, match="span"):
        torch.ops.sfmwarp.scale_arrays(x, spans, gy)
    with FakeTensorMode():
        with pytest.raises(TypeError, match="span"):
            torch.ops.sfmwarp.scale_arrays(torch.empty(64, device="cuda"), spans, torch.ones((), device="cuda"))


def test_disp_activation_refuses_cpu_and_integer_logits():
    with pytest.raises(TypeError, match="CPU"):
        ta.disp_activation([torch.zeros(1, 1, 4, 4, dtype=torch.bfloat16)])
    with FakeTensorMode():
        with pytest.raises(TypeError, match="dtype"):
            ta.disp_activation([torch.zeros(1, 1, 4, 4, dtype=torch.int32, device="cuda")])


def test_plan_cache_is_bounded():
    """One host-side plan per (shapes, settings); the oldest is dropped beyond 16 (an epoch's last, smaller batch, ...)."""
    with FakeTensorMode():
        for B in range(1, 21):
            tgt, src, K, disps, poses = _args("cuda", B=B)
            ta._plan(B, 16, 24, 2, disps, [], poses, (0.1, 0.0, 0.0, _lib.SMOOTH_SECOND_ORDER, 0, B))
    assert len(ta._PLANS) <= ta._MAX_PLANS
