"""The gradient with respect to the camera intrinsics without a GPU: the derivation, the reference floors that hold the margins of
tests/test_intrinsics_grad_gpu.py, the reject paths of the three entry points (include/sfmwarp.h) and
torch_api.multi_scale_intrinsics.

The derivation.  Per (sample, scale) and source i, with Pm = K [R|t] (models/transform.py:86-88), ray = K^-1 pix (:105), one depth per
pixel (models/base_model.py:82-84) and gPm = dL/dPm:
    d_K = sum_i  gPm_i[:, :3] R_i^T + gPm_i[:, 3] t_i^T - K^-T R_i^T K^T gPm_i[:, :3]
(the last term is the F.batch_inv path: gKinv = (K R)^T gPm[:, :3] K^T, gK = -K^-T gKinv K^-T).  torch.autograd, through the torch
restatement of the reference in tests/test_oracle_vs_torch_cpu.py, is the judge."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest
import torch

import abi_header
import intrinsics_grad as IG

_lib = importlib.import_module("sfm-learner-chainer_amd._lib")
ops = importlib.import_module("sfm-learner-chainer_amd.ops")
ta = importlib.import_module("sfm-learner-chainer_amd.torch_api")
L = _lib.lib
FAKE = 0x10000                 # never dereferenced (256-byte aligned: also a workspace address)
CASES = [(shape, kind) for shape in IG.SHAPES for kind in IG.KINDS]
IDS = ["%s-%s" % ("x".join(map(str, s)), k) for s, k in CASES]


# ------------------------------------------------------------------------------------------------------------------------
# header and binding
# ------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ["sfm_loss_proj_bwd", "sfm_pose_proj_bwd_k", "sfm_warp_intrinsics_bwd", "sfm_warp_intrinsics_bwd_workspace_bytes"]


def test_header_binding_and_library_declare_the_same_symbols():
    pick = lambda names: sorted(n for n in names if re.search(r"intrinsics|proj_bwd_k|loss_proj", n))
    assert pick(abi_header.declared()) == pick(_lib.SYMBOLS) == ENTRY_POINTS
    for name in ENTRY_POINTS:
        res, args = _lib.SYMBOLS[name]
        assert getattr(L, name).argtypes == args and getattr(L, name).restype == res, name


# ------------------------------------------------------------------------------------------------------------------------
# the derivation and the floors
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_closed_form_equals_autograd_and_fp32_floors(shape, kind):
    """On the exact ramp inputs of the GPU tests, for the four loss configurations:
      * the closed form on dL/dPm taken from autograd equals autograd's d_K: <= 1e-12 per entry (measured 1.4e-14);
      * an all-fp32 torch evaluation of d_K is within 1.5e-4 per entry of the fp64 one (measured 1.03e-4 at worst over more seeds,
        1e-5 here): the GPU's 1e-3 is ten times this floor;
      * the closed form on dL/dPm rounded to fp32 is within 2e-6 per entry of the exact one (measured 9.2e-7 at worst, 2.4e-7 here):
        the GPU's self-consistency bound of 1e-5 is ten times this floor;
      * all nine entries are non-zero, the smallest at least 6e-3 of the largest (what makes a per-entry criterion usable)."""
    d = IG.ramp_inputs(shape, kind)
    for mode, cfg in IG.CONFIGS.items():
        r = IG.autograd_loss(d, cfg, want_gq=True)
        exact = IG.d_k_from_d_proj(d["intrinsics"], d["poses"], r["d_proj"])
        assert IG.worst(exact, r["d_K"]) <= 1e-12, (mode, IG.worst(exact, r["d_K"]))
        assert np.array_equal(r["d_K"], IG.reference(tuple(shape), kind, mode)["d_K"])         # what the GPU tests compare with
        r32 = IG.autograd_loss(d, cfg, dtype="float32")
        assert IG.worst(r32["d_K"], r["d_K"]) <= 1.5e-4, (mode, IG.worst(r32["d_K"], r["d_K"]))
        rounded = IG.d_k_from_d_proj(d["intrinsics"], d["poses"], r["d_proj"].astype(np.float32))
        assert IG.worst(rounded, exact) <= 2e-6, (mode, IG.worst(rounded, exact))
        size = np.abs(r["d_K"]).max(axis=0)
        assert (size.min(axis=(1, 2)) >= 6e-3 * size.max(axis=(1, 2))).all(), (mode, size)


def test_ramp_inputs_are_ramps_with_a_margin():
    """I = c + a x/(w-1) + b y/(h-1) with the same a, b, c at every scale; sources in [0.15, 0.95], the target in [-0.95, -0.15]"""
    d = IG.ramp_inputs((3, 24, 40, 2, 3), "general")
    for pyr, lo, hi in ((d["src_pyr"], 0.15, 0.95), (d["tgt_pyr"], -0.95, -0.15)):
        corners = [a[:, :, [0, 0, -1, -1], [0, -1, 0, -1]] for a in pyr]
        for a, c in zip(pyr, corners):
            assert lo - 1e-6 <= a.min() and a.max() <= hi + 1e-6
            np.testing.assert_allclose(c, corners[0], rtol=0, atol=1e-6)                                  # the same ramp at every scale
            h, w = a.shape[2:]
            second = a[:, :, 2:, :] - 2 * a[:, :, 1:-1, :] + a[:, :, :-2, :]
            assert np.abs(second).max() <= 1e-6 and np.abs(a[:, :, :, 2:] - 2 * a[:, :, :, 1:-1] + a[:, :, :, :-2]).max() <= 1e-6
    assert d["src_pyr"][0].min() - d["tgt_pyr"][0].max() >= 0.3 - 1e-6


def test_the_closed_form_needs_one_depth_per_pixel():
    """With three different depth rows (models/transform.py:107) gKinv no longer follows from gPm: the warp operator has a per-pixel
    kernel for it.  Here: autograd's d_K of the warp differs from the closed form by far more than any tolerance used."""
    import test_oracle_vs_torch_cpu as T
    d = IG.ramp_inputs((2, 17, 29, 3, 2), "general")
    N, H, W = 2, 17, 29
    rng = np.random.RandomState(1)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    g = rng.normal(size=(N, 3, H, W))
    depth = (1.0 / d["disps"][0]).reshape(N, 1, H * W)
    for rows, same in ((np.ones((1, 3, 1)), True), (np.array([1.0, 1.1, 0.9]).reshape(1, 3, 1), False)):
        K = t(d["intrinsics"][:, 0]).requires_grad_(True)
        saved = T.proj_tgt_to_src
        projs = []

        def rec(vec, Kx):
            p = saved(vec, Kx)
            p.retain_grad()
            projs.append(p)
            return p
        T.proj_tgt_to_src = rec
        try:
            out = T.projective_inverse_warp(t(d["src_pyr"][0][:, :3]), t(depth * rows), t(d["poses"][0]), K)
            (out * t(g)).sum().backward()
        finally:
            T.proj_tgt_to_src = saved
        closed = IG.d_k_from_d_proj(d["intrinsics"][:, :1], d["poses"][:1], projs[0].grad.numpy()[:, None, None, :3, :])[:, 0]
        err = IG.worst(closed, K.grad.numpy())
        assert (err <= 1e-12) if same else (err > 1e-2), (same, err)


# ------------------------------------------------------------------------------------------------------------------------
# reject paths: what the entry points answer before any HIP call
# ------------------------------------------------------------------------------------------------------------------------
def _desc(**kw):
    d = _lib.SfmLossDesc()
    d.B, d.norm_B, d.n_src, d.n_scales = 2, 2, 2, 2
    d.H[0], d.W[0], d.H[1], d.W[1] = 16, 24, 8, 12
    d.ssim_rate, d.smooth_reg, d.smooth_mode = 0.15, 0.1, _lib.SMOOTH_SECOND_ORDER
    for s in range(2):
        d.tgt[s] = d.src[s] = d.disp[s] = d.d_disp[s] = FAKE
    d.pose[0] = d.pose[1] = d.d_pose[0] = d.d_pose[1] = FAKE
    d.intrinsics = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _proj_bwd(d, loss=1, ws=FAKE, ws_bytes=None, d_proj=FAKE, d_K=FAKE):
    n = L.sfm_loss_workspace_bytes(C.byref(d)) if d is not None else 0
    rc = L.sfm_loss_proj_bwd(C.byref(d) if d is not None else None, loss, C.c_void_p(ws) if ws else None,
                             n if ws_bytes is None else ws_bytes, C.c_void_p(d_proj) if d_proj else None, C.c_void_p(d_K) if d_K else None,
                             None)
    return rc, _lib.last_error()


def test_loss_proj_bwd_rejects_in_the_documented_order():
    # 1. NULL descriptor, whatever else is wrong
    rc, msg = _proj_bwd(None, ws=None, d_proj=None, d_K=None)
    assert rc == _lib.ERR_NULL and "descriptor" in msg
    # 2. the descriptor, as sfm_loss_bwd rejects it -- before the outputs and the workspace are looked at
    for bad, code in ((dict(n_src=9), _lib.ERR_SHAPE), (dict(norm_B=1), _lib.ERR_CONFIG), (dict(intrinsics=None), _lib.ERR_NULL),
                      (dict(projection=2), _lib.ERR_CONFIG)):
        d = _desc(**bad)
        want = L.sfm_loss_bwd(C.byref(d), 1.0, None, 0, None)
        want_msg = _lib.last_error()
        for loss in (0, 1):
            rc, msg = _proj_bwd(d, loss=loss, ws=None, ws_bytes=0, d_proj=None, d_K=None)
            assert rc == want == code and msg == want_msg, (bad, rc, msg)
    d = _desc()
    d.d_pose[1] = None                                                # ... its gradient outputs included
    rc, msg = _proj_bwd(d, ws=None, d_proj=None, d_K=None)
    assert rc == _lib.ERR_NULL and "d_pose[1]" in msg
    # 3. both outputs NULL, before the workspace
    rc, msg = _proj_bwd(_desc(), ws=None, ws_bytes=0, d_proj=None, d_K=None)
    assert rc == _lib.ERR_NULL and "both NULL" in msg
    # 4. the workspace: NULL, one byte short, off the 256-byte boundary -- with either output alone
    d = _desc()
    n = L.sfm_loss_workspace_bytes(C.byref(d))
    for kw in (dict(d_proj=None), dict(d_K=None), dict()):
        for ws, nbytes, word in ((None, n, "needed"), (FAKE, n - 1, "needed"), (FAKE + 4, n, "aligned"), (FAKE + 128, n + 4096, "aligned")):
            rc, msg = _proj_bwd(d, ws=ws, ws_bytes=nbytes, **kw)
            assert rc == _lib.ERR_WORKSPACE and "workspace" in msg and word in msg, (kw, ws, nbytes, rc, msg)
            with pytest.raises(ValueError):
                _lib.check(rc)
    # B == 0 launches nothing: an empty shard's input pointers may be NULL, the outputs are still asked for
    e = _lib.SfmLossDesc()
    e.norm_B = 4
    assert _proj_bwd(e, ws=None, ws_bytes=0)[0] == 0
    assert _proj_bwd(e, ws=None, ws_bytes=0, d_proj=None, d_K=None)[0] == _lib.ERR_NULL


def test_warp_intrinsics_bwd_rejects_as_warp_bwd_does():
    f = C.c_void_p(FAKE)
    n = L.sfm_warp_intrinsics_bwd_workspace_bytes(2, 16, 24)
    assert n == 2 * ((16 * 24 + 255) // 256) * 21 * 4 and L.sfm_warp_intrinsics_bwd_workspace_bytes(0, 16, 24) == 0
    call = lambda *a: (L.sfm_warp_intrinsics_bwd(*a), _lib.last_error())
    assert call(None, None, 1, None, None, None, None, None, 0, 0, 3, 16, 24, None)[0] == 0            # empty batch
    for k in range(6):                                                                                # each tensor
        a = [f, f, 1, f, f, f, f, f, n, 2, 3, 16, 24, None]
        a[[0, 1, 3, 4, 5, 6][k]] = None
        rc, msg = call(*a)
        assert rc == _lib.ERR_NULL and msg.startswith("sfm_warp_intrinsics_bwd"), (k, rc, msg)
    for N, Cc, H, W, rows in ((70000, 3, 16, 24, 1), (2, 0, 16, 24, 1), (2, 3, 2, 24, 1), (2, 3, 16, 24, 2)):
        assert call(f, f, rows, f, f, f, f, f, n, N, Cc, H, W, None)[0] == _lib.ERR_SHAPE
    for ws, nbytes in ((f, n - 1), (None, n)):
        rc, msg = call(f, f, 1, f, f, f, f, ws, nbytes, 2, 3, 16, 24, None)
        assert rc == _lib.ERR_WORKSPACE and "workspace" in msg


def test_pose_proj_bwd_k_rejects():
    f = C.c_void_p(FAKE)
    assert L.sfm_pose_proj_bwd_k(None, None, None, None, 0, None) == 0
    for k in range(4):
        a = [f, f, f, f]
        a[k] = None
        assert L.sfm_pose_proj_bwd_k(*a, 3, None) == _lib.ERR_NULL and "sfm_pose_proj_bwd_k" in _lib.last_error()
    assert L.sfm_pose_proj_bwd_k(f, f, f, f, -1, None) == _lib.ERR_SHAPE


# ------------------------------------------------------------------------------------------------------------------------
# torch_api.multi_scale_intrinsics
# ------------------------------------------------------------------------------------------------------------------------
def test_multi_scale_intrinsics_values_and_gradient():
    synth = importlib.import_module("sfm-learner-chainer_amd.synth")
    rng = np.random.RandomState(2)
    K = np.zeros((3, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = rng.uniform(200, 260, 3), rng.uniform(200, 260, 3), rng.uniform(190, 220, 3), rng.uniform(50, 70, 3), 1
    want = synth.multi_scale_intrinsics(K, 4)
    assert np.array_equal(ta.multi_scale_intrinsics(torch.from_numpy(K), 4).numpy(), want)
    f = torch.from_numpy(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)).requires_grad_()
    out = ta.multi_scale_intrinsics(f, 4)
    assert np.array_equal(out.detach().numpy(), want) and out.shape == (3, 4, 3, 3)
    w = torch.from_numpy(rng.normal(size=(3, 4, 3, 3)).astype(np.float32))
    (out * w).sum().backward()
    # d/d(fx) = sum_s w[b, s, 0, 0] / 2^s, and likewise fy [1,1], cx [0,2], cy [1,2]; no other entry depends on the parameter
    div = (2.0 ** -np.arange(4))[None, :]
    wn = w.numpy().astype(np.float64)
    expect = np.stack([(wn[:, :, 0, 0] * div).sum(1), (wn[:, :, 1, 1] * div).sum(1), (wn[:, :, 0, 2] * div).sum(1), (wn[:, :, 1, 2] * div).sum(1)], axis=1)
    np.testing.assert_allclose(f.grad.numpy(), expect, rtol=1e-6, atol=0)
    assert torch.autograd.gradcheck(lambda x: ta.multi_scale_intrinsics(x, 3), (f.detach().double().requires_grad_(),))
    for bad in (torch.zeros(3, 3), torch.zeros(3, 5), torch.zeros(2, 3, 4)):
        with pytest.raises(TypeError):
            ta.multi_scale_intrinsics(bad, 2)
    with pytest.raises(TypeError):
        ta.multi_scale_intrinsics(torch.zeros(2, 4), 9)
