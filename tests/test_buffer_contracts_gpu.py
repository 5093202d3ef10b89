"""The buffer contract of every entry point of include/sfmwarp.h that takes a device pointer: WHERE the kernels write, what they
read back, and what they assume about the addresses they are given.  The value tests (test_loss_gpu.py, test_ops_edges_gpu.py ...)
say the numbers are right on fresh, 512-byte aligned torch allocations; nothing there notices a store that lands in the allocator's
slack, a partial sum that is read from the workspace without having been written by this call, or a 16-byte access formed from a
pointer that is only 4-byte aligned.

Every case here places ALL buffers of a call in one allocation filled with a NaN bit pattern (util.Arena): named sub-buffers with
guards of at least max(4 KiB, two rows) on both sides, each at a chosen residue mod 16 bytes, the workspace on a 256-byte boundary
with exactly the queried number of bytes.  Nothing can fault: every guard is inside the allocation.  Four checks per entry point:

  1. guards and inputs    no guard word changes, no input changes, every "overwritten" output is written completely;
  2. old output content   the outputs pre-filled with the NaN sentinel and with 1e30 give the same bits (accumulated outputs:
                          pre-filled with c, the result is c + reference);
  3. stale scratch        the workspace pre-filled with zeros, the sentinel, 0xFF bytes and the leftovers of OTHER calls;
  4. alignment            every float array at 4 / 8 / 12 mod 16.

THE REFERENCE of every comparison is the same entry point on conventionally allocated tensors (one fresh allocation each) with a
zero-filled workspace -- the placement all oracle-checked tests use -- and the comparison is BITWISE.  The exceptions are the
outputs the header defines as accumulated with float atomics (the order of the additions is not fixed): d_src of the fused loss by
the criterion of test_loss_gpu.py::test_d_src_through_the_lds_window (rtol 0, atol 2e-5 max|d_src| of the scale), gx / d_src of the
operators by that of test_torch_api_gpu.py::test_operator_functions_match_ops_bitwise (rtol 1e-5, atol 1e-6).  (Measured on the
MI355X, and printed by every run in the parity statistics: two runs of the REFERENCE placement itself give different d_src bits at
2 x 37 x 70 and 4 x 128 x 416 -- a few hundred of 1.3 M elements, by one or two ulp, 7e-8 of the maximum -- and the same bits at the
shapes below that; so this comparison stays with the criterion, it cannot be bitwise.)  Some fused cases also
go through _check_losses / _check_grads / _check_warped of test_loss_gpu.py against the oracle, criteria unchanged.

WHY 4-BYTE ALIGNMENT OF THE CALLER'S TENSORS IS ENOUGH -- every access wider than 4 bytes in csrc/, and the pointer it is formed from:

  sfm_ops.hip
    pyramid_hwc_fwd_kernel   float4 loads of three planes of x, float4 stores to y[0] through LDS (`stage`, a static __shared__ float4
                             array): only in blocks where `block_vec` holds, which tests ((x | y[0]) % 16 == 0 and P % 4 == 0) in the
                             kernel itself -- every other block goes pixel by pixel (Float3: packed, aligned(4), a 12-byte store the
                             compiler may only assume dword alignment for; Pair2 the same for 8-byte loads);
    pyramid_band_hwc_kernel  float4 copies x -> LDS (`band`, the only dynamic LDS of the kernel: starts at LDS offset 0, plane spans
                             are multiples of W, W % 4 == 0) and float4 stores to y[0]: launch_pyramid_band() returns false -- the
                             per-pixel kernel runs -- unless W % 4 == 0 and x, y[0] (and the second tensor's x2, y2[0]) are all
                             0 mod 16; band row starts are multiples of W floats.  y[1..] are written with Float3 stores only;
    scale_arrays_kernel      float4 body between a scalar head and tail: scale_arrays_launch() computes the head so that x + head is
                             0 mod 16 when x and y are co-aligned, and makes the WHOLE array the scalar head when they are not;
    everything else          (pose_proj, warp, sampler, interp, resize, pyramid_fwd, augment, disp_act) scalar float accesses;
    LDS                      `Geom g`, `red` are float structs accessed by member.
  sfm_loss.hip               finalize_kernel reads h_gpm / h_loss as float4: both are arrays of the WORKSPACE (offsets multiples of
                             256 bytes, records of 48 / 16 bytes) -- hence the 256-byte alignment sfm::run demands of `ws`, which the
                             header now states; lane_acc / scalar_red are __shared__ doubles indexed by element.
  sfm_ssim_pass.h            pose_sums_raw stores 3 x float4 to gpm_out: the workspace again (48-byte records).
                             The HWC gather: raw buffer loads b128 + b64 of the source taps at byte offset 12 (v0 w + u0) and b96 of
                             the target texel at 12 x -- MUBUF needs dword alignment of base + offset only, and the offsets already
                             take every residue mod 16 on aligned tensors; the range check is in bytes relative to the resource's
                             base, so it does not depend on the base's residue either.  The planar gather and K9 / Rgb / Rgb2 / Rec go
                             through packed, aligned(4) structs (dwordx2 / x3 global accesses at dword alignment).
  sfm_common.h               Tap2 (packed, aligned(4)): 8-byte loads of two adjacent taps, at any pixel offset already.
  sfm_loss_dsrc.hip          DsrcRec records live in the workspace; dsrc_win is LDS (extern, aligned(16), doubles).
  sfm_loss_kernels.h         gacc_all: __shared__ floats.
So no kernel forms a 16-byte access from a caller's tensor without a host-side or in-kernel test of the address, and the only
alignment requirement the library has is the workspace's, which it rejects before any launch (checked below)."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from util import SENTINEL, Arena, parity_note, to_dev, to_np

pytestmark = pytest.mark.gpu

F32 = np.float32
FINITE_FILL = 1e30

# Entry points of include/sfmwarp.h that take a device pointer -> the test function that places their buffers in an arena: one of
# this module, or "file.py::test_name" of another GPU test module (tests/test_buffer_contracts_cpu.py holds this table against the
# header's prototypes and against the names the modules define).
COVERED = {
    "sfm_loss_fwd": "test_fused_guards_and_inputs", "sfm_loss_bwd": "test_fused_guards_and_inputs",
    "sfm_loss_fwd_bwd": "test_fused_guards_and_inputs", "sfm_step_fwd": "test_fused_guards_and_inputs",
    "sfm_step_fwd_bwd": "test_fused_guards_and_inputs",
    "sfm_pose_proj_fwd": "test_op_guards_and_inputs", "sfm_pose_proj_bwd": "test_op_guards_and_inputs",
    "sfm_warp_fwd": "test_op_guards_and_inputs", "sfm_warp_bwd": "test_op_guards_and_inputs",
    "sfm_sampler_fwd": "test_op_guards_and_inputs", "sfm_sampler_bwd": "test_op_guards_and_inputs",
    "sfm_sampler_interp_fwd": "test_op_guards_and_inputs", "sfm_sampler_interp_bwd": "test_op_guards_and_inputs",
    "sfm_resize_fwd": "test_op_guards_and_inputs", "sfm_pyramid_fwd": "test_op_guards_and_inputs",
    "sfm_pyramid_hwc_fwd": "test_op_guards_and_inputs", "sfm_pyramid_pair_hwc_fwd": "test_op_guards_and_inputs",
    "sfm_disp_act_fwd": "test_op_guards_and_inputs", "sfm_disp_act_bwd": "test_op_guards_and_inputs",
    "sfm_augment_fwd": "test_op_guards_and_inputs", "sfm_scale_arrays": "test_scale_arrays_in_an_arena",
    "sfm_pose_proj_bwd_k": "test_op_guards_and_inputs", "sfm_warp_intrinsics_bwd": "test_op_guards_and_inputs",
    "sfm_loss_proj_bwd": "test_fused_proj_bwd_after_every_gradient_entry",
    "sfm_resize_bwd": "test_resize_bwd_gpu.py::test_buffer_contract",
    "sfm_warp_pyramid_fwd": "test_warp_pyramid_gpu.py::test_buffer_contract", "sfm_warp_pyramid_bwd": "test_warp_pyramid_gpu.py::test_buffer_contract",
    "sfm_photo_error_fwd": "test_photo_error_gpu.py::test_buffer_contract", "sfm_photo_error_bwd": "test_photo_error_gpu.py::test_buffer_contract",
}
# measurement and debug hooks: they take a pointer but no tensor of the contract (events; a trace buffer sized by the caller)
EXEMPT = {"sfm_loss_profile_events", "sfm_loss_debug_trace"}


def _i32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def assert_bits(got, want, what):
    """bitwise equality of two float32 arrays, NaN payloads and the sign of zero included"""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg=what)


def residues_for(names, scheme, outputs=()):
    """name -> residue mod 16 of its first byte.  "rr": 4, 8, 12 round-robin in the order of `names` (which lists the arrays of one
    scale next to each other: what a kernel touches together gets different residues)."""
    if scheme == "aligned":
        return {n: 0 for n in names}
    if scheme == "all4":
        return {n: 4 for n in names}
    if scheme == "out0_in12":
        return {n: (0 if n in outputs else 12) for n in names}
    if scheme in ("rr", "rr8"):
        first = 0 if scheme == "rr" else 1
        return {n: (4, 8, 12)[(k + first) % 3] for k, n in enumerate(names)}
    raise ValueError(scheme)


SCHEMES = ("rr", "all4", "out0_in12")


# =====================================================================================================================================
# 2. the fused loss
# =====================================================================================================================================
MODES = {
    "l1": dict(),
    "ssim_smooth": dict(smooth_reg=0.1, ssim_rate=0.15),
    "edge_aware": dict(smooth_reg=0.1, ssim_rate=0.15, smooth_mode="edge_aware"),
    "explain": dict(smooth_reg=0.1, exp_reg=0.2),
    "ssim_only": dict(ssim_rate=0.15),
}

FCase = collections.namedtuple("FCase", "shape inputs mode layout proj warped dsrc variant step oracle")


def _fc(shape, mode, layout, proj="fast", warped=False, dsrc="no", variant=0, inputs="default", step=False, oracle=False):
    assert mode in MODES and layout in ("planar", "hwc") and proj in ("fast", "reference_order") and dsrc in ("no", "all", "sub")
    assert not step or layout == "hwc"
    return FCase(shape, inputs, mode, layout, proj, warped, dsrc, variant, step, oracle)


def fcase_id(c):
    return "%dx%dx%d-n%d-s%d-%s-%s-%s-%s-%s-dsrc_%s-v%d%s%s" % (
        c.shape + (c.inputs, c.mode, c.layout, "fast" if c.proj == "fast" else "reford", "warped" if c.warped else "nowarped", c.dsrc,
                   c.variant, "-step" if c.step else "", "-oracle" if c.oracle else ""))


A, BS, CS, D8, E, F3, G = (1, 3, 3, 1, 1), (1, 5, 61, 2, 1), (9, 16, 24, 2, 2), (3, 33, 40, 8, 1), (2, 70, 36, 2, 2), (2, 37, 71, 3, 3), \
    (4, 128, 416, 2, 4)
OV, BH = (2, 16, 52, 2, 2), (2, 37, 70, 2, 2)                        # every pixel out of view; a source behind the camera
O1, O3 = (2, 32, 48, 2, 3), (3, 20, 130, 4, 2)                      # shapes of the oracle tests of test_loss_gpu.py

FUSED_CASES = [
    _fc(A, "l1", "planar", warped=True, dsrc="all"),
    _fc(A, "ssim_smooth", "hwc", step=True),
    _fc(A, "explain", "planar", proj="reference_order", warped=True),
    _fc(BS, "l1", "hwc", warped=True, dsrc="all"),
    _fc(BS, "edge_aware", "planar"),
    _fc(BS, "ssim_only", "hwc", proj="reference_order", warped=True),
    _fc(BS, "explain", "hwc", dsrc="all"),
    _fc(CS, "ssim_smooth", "hwc", warped=True, step=True),
    _fc(CS, "ssim_smooth", "hwc", variant=5),
    _fc(CS, "ssim_smooth", "hwc", variant=4),
    _fc(CS, "l1", "planar", proj="reference_order", dsrc="all"),
    _fc(CS, "explain", "planar", warped=True, variant=3),
    _fc(CS, "edge_aware", "hwc", dsrc="all", step=True),
    _fc(D8, "ssim_smooth", "planar"),
    _fc(D8, "edge_aware", "hwc", warped=True, variant=5),
    _fc(D8, "l1", "hwc", dsrc="all"),
    _fc(D8, "explain", "hwc", proj="reference_order"),
    _fc(E, "ssim_smooth", "hwc", warped=True, dsrc="all", step=True),
    _fc(E, "ssim_only", "planar"),
    _fc(E, "edge_aware", "planar", proj="reference_order", warped=True, dsrc="all"),
    _fc(E, "l1", "hwc", variant=3),
    _fc(E, "explain", "planar", dsrc="all"),
    _fc(F3, "ssim_smooth", "hwc", warped=True, dsrc="sub", step=True),
    _fc(F3, "l1", "planar", dsrc="sub"),
    _fc(F3, "edge_aware", "hwc", proj="reference_order"),
    _fc(F3, "explain", "hwc", warped=True),
    _fc(F3, "ssim_only", "hwc", variant=4),
    _fc(F3, "ssim_smooth", "planar", proj="reference_order", warped=True, dsrc="all"),
    _fc(G, "ssim_smooth", "hwc", step=True),
    _fc(G, "edge_aware", "hwc", warped=True, dsrc="all"),
    _fc(G, "l1", "planar"),
    _fc(G, "explain", "planar"),
    _fc(G, "ssim_smooth", "hwc", variant=5),
    _fc(G, "ssim_only", "hwc", proj="reference_order", dsrc="sub"),
    _fc(OV, "ssim_smooth", "hwc", warped=True, dsrc="all", inputs="out_of_view"),
    _fc(OV, "l1", "planar", inputs="out_of_view"),
    _fc(OV, "explain", "hwc", dsrc="all", inputs="out_of_view"),
    _fc(BH, "ssim_smooth", "hwc", warped=True, dsrc="all", inputs="behind"),
    _fc(BH, "edge_aware", "planar", proj="reference_order", inputs="behind"),
    _fc(BH, "l1", "hwc", warped=True, inputs="behind"),
    # ... and tied to the oracle (inputs and criteria of the oracle tests of test_loss_gpu.py that run these shapes): every loss
    # mode, both layouts, both projections
    _fc(G, "ssim_smooth", "hwc", warped=True, inputs="seed1", oracle=True),               # test_baseline_configs_vs_oracle
    _fc(G, "edge_aware", "planar", warped=True, inputs="seed1", oracle=True),
    _fc(O1, "l1", "planar", dsrc="all", inputs="seed11", oracle=True),                    # test_fused_loss_matches_oracle
    _fc(O1, "explain", "planar", dsrc="all", inputs="seed11", oracle=True),
    _fc(O1, "ssim_only", "hwc", dsrc="all", inputs="seed13", oracle=True),                # test_hwc_layout_gives_the_planar_results
    _fc(O1, "ssim_smooth", "planar", proj="reference_order", warped=True, inputs="seed19", oracle=True),      # test_reference_order_projection_...
    _fc(O3, "explain", "hwc", proj="reference_order", warped=True, inputs="seed19", oracle=True),
]
assert len(set(map(fcase_id, FUSED_CASES))) == len(FUSED_CASES)

_inputs_cache = {}


def case_inputs(synth, c):
    """the dict of synth.make_inputs for the case (host arrays; cached per shape and input kind)"""
    key = (c.shape, c.inputs)
    if key not in _inputs_cache:
        B, H, W, n_src, n_scales = c.shape
        kw = dict(B=B, H=H, W=W, n_src=n_src, n_scales=n_scales, with_masks=c.inputs != "seed1")      # (seed1: the draws of the test it mirrors)
        if c.inputs == "behind":
            from test_loss_gpu import make_motion_inputs
            d = make_motion_inputs(synth, "behind", seed=21, **kw)
        elif c.inputs.startswith("seed"):
            d = synth.make_inputs(seed=int(c.inputs[4:]), **kw)
        else:
            d = synth.make_inputs(seed=5, **kw)
            if c.inputs == "out_of_view":      # as test_loss_edges_gpu.py::test_everything_out_of_view_is_masked_not_nan
                for p in d["poses"]:
                    p[:, 3] = 50.0
        _inputs_cache[key] = d
    return _inputs_cache[key]


def _hwc(a):
    """(B,3G,h,w) planar -> (B,G,h,w,3), on the host (what ops.to_hwc does on the device)"""
    B, Cc, h, w = a.shape
    return np.ascontiguousarray(a.reshape(B, Cc // 3, 3, h, w).transpose(0, 1, 3, 4, 2))


def dsrc_flags(c):
    S = c.shape[4]
    return [c.dsrc == "all" or (c.dsrc == "sub" and s % 2 == 0) for s in range(S)]      # "sub": [True, False, True, ...]


def fused_buffers(d, c, step):
    """-> (inputs: name -> host array, outputs: name -> shape), both ordered with the arrays of one scale next to each other.
    `step`: the call is sfm_step_*: the full-resolution frames are the inputs and the pyramids are OUTPUTS of the call."""
    B, H, W, n_src, S = c.shape
    hwc = c.layout == "hwc"
    use_masks = bool(MODES[c.mode].get("exp_reg"))
    ins, outs = collections.OrderedDict(), collections.OrderedDict()
    if step:
        ins["tgt_full"], ins["src_full"] = d["tgt_pyr"][0], d["src_pyr"][0]
    flags = dsrc_flags(c)
    for s in range(S):
        h, w = d["disps"][s].shape[2:]
        tgt, src = (_hwc(d["tgt_pyr"][s]), _hwc(d["src_pyr"][s])) if hwc else (d["tgt_pyr"][s], d["src_pyr"][s])
        if step:
            outs["tgt%d" % s], outs["src%d" % s] = tgt.shape, src.shape
        else:
            ins["tgt%d" % s], ins["src%d" % s] = tgt, src
        ins["disp%d" % s] = d["disps"][s]
        if use_masks:
            ins["mask%d" % s] = d["masks"][s]
        outs["d_disp%d" % s] = (B, 1, h, w)
        if use_masks:
            outs["d_mask%d" % s] = (B, n_src, h, w)
        if flags[s]:
            outs["d_src%d" % s] = (B, 3 * n_src, h, w)
        if c.warped:
            outs["warped%d" % s] = (B, n_src, 3, h, w)
    ins["intrinsics"] = d["intrinsics"]
    for i in range(n_src):
        ins["pose%d" % i] = d["poses"][i]
        outs["d_pose%d" % i] = (B, 6)
    outs["loss5"] = (5,)
    return ins, outs


def written_by(entry, name):
    """does this entry point write output `name`?  (include/sfmwarp.h: gradients "backward only", warped "ignored by sfm_loss_bwd")"""
    if name.startswith(("tgt", "src")):
        return entry.startswith("step")
    if name == "loss5" or name.startswith("warped"):
        return entry != "bwd"
    return entry not in ("fwd", "step_fwd")


def entries_of(c):
    return ("fwd_bwd", "fwd", "bwd") + (("step_fwd_bwd", "step_fwd") if c.step else ())


def _bind_from(ops, c, get, S, n_src, use_masks, buffers=None):
    """a FusedLoss bound to the arrays `get(name)` returns (device tensors)"""
    fl = ops.FusedLoss(projection=c.proj, **MODES[c.mode])
    fl.bind([get("tgt%d" % s) for s in range(S)], [get("src%d" % s) for s in range(S)], get("intrinsics"),
            [get("disp%d" % s) for s in range(S)], [get("pose%d" % i) for i in range(n_src)],
            [get("mask%d" % s) for s in range(S)] if use_masks else None,
            want_d_src=dsrc_flags(c) if c.dsrc != "no" else False, layout=c.layout, want_warped=c.warped, buffers=buffers)
    return fl


def _launch(ops, fl, c, entry, frames=None):
    import torch
    if c.variant:
        ops.check(ops.lib.sfm_loss_variant(c.variant))
    if entry == "fwd":
        fl.forward()
    elif entry == "bwd":
        fl.backward(1.0)
    elif entry == "fwd_bwd":
        fl.forward_backward()
    else:
        fl.step_from_frames(frames[0], frames[1], grad=entry == "step_fwd_bwd")
    torch.cuda.synchronize()


def _collect(fl, c, entry, pyr=None):
    """name -> host array of every output the entry point writes"""
    got = {}
    S, n_src = c.shape[4], c.shape[3]
    if entry.startswith("step"):
        for s in range(S):
            got["tgt%d" % s], got["src%d" % s] = to_np(pyr[0][s]).copy(), to_np(pyr[1][s]).copy()
    if entry != "bwd":
        got["loss5"] = to_np(fl.loss5).copy()
        for s in range(S if c.warped else 0):
            got["warped%d" % s] = to_np(fl.warped[s]).copy()
    if entry not in ("fwd", "step_fwd"):
        for s in range(S):
            got["d_disp%d" % s] = to_np(fl.d_disps[s]).copy()
            if fl.d_masks is not None:
                got["d_mask%d" % s] = to_np(fl.d_masks[s]).copy()
            if fl.d_srcs is not None and fl.d_srcs[s] is not None:
                got["d_src%d" % s] = to_np(fl.d_srcs[s]).copy()
        for i in range(n_src):
            got["d_pose%d" % i] = to_np(fl.d_poses[i]).copy()
    return got


_ref_cache = {}


def reference(ops, synth, dev, c, entry):
    """THE reference of this module: the same entry point on conventionally allocated tensors (a fresh allocation each) and a
    zero-filled workspace.  -> (name -> host array, workspace bytes of the descriptor)"""
    import torch
    key = (fcase_id(c), entry)
    if key in _ref_cache:
        return _ref_cache[key]
    d = case_inputs(synth, c)
    step = entry.startswith("step")
    ins, outs = fused_buffers(d, c, step)
    t = {k: to_dev(v, dev) for k, v in ins.items()}
    if step:
        for k, shape in outs.items():
            if k.startswith(("tgt", "src")):
                t[k] = torch.empty(shape, dtype=torch.float32, device=dev)
    S, n_src = c.shape[4], c.shape[3]
    fl = _bind_from(ops, c, t.__getitem__, S, n_src, "mask0" in ins)
    fl.ws.zero_()
    pyr = ([t["tgt%d" % s] for s in range(S)], [t["src%d" % s] for s in range(S)])
    _launch(ops, fl, c, entry, (t.get("tgt_full"), t.get("src_full")))
    got = _collect(fl, c, entry, pyr)
    if any(k.startswith("d_src") for k in got):
        # measured and reported: is the accumulated output the same bits from run to run in ONE placement?
        fl.ws.zero_()
        _launch(ops, fl, c, entry, (t.get("tgt_full"), t.get("src_full")))
        again = _collect(fl, c, entry, pyr)
        same = all(np.array_equal(_i32(again[k]), _i32(got[k])) for k in got if k.startswith("d_src"))
        parity_note("buffer contracts: d_src of two runs of the reference placement (%s %s) bit-identical: %s" % (fcase_id(c), entry, same))
    _ref_cache[key] = (got, fl._ws_bytes)
    return _ref_cache[key]


class Placed:
    """All buffers of one fused-loss call in one arena, a FusedLoss bound to them (bind(buffers=...))."""

    def __init__(self, ops, synth, dev, c, entry, scheme="aligned", ws_room=0, extra=None):
        """ws_room: bytes the workspace REGION has beyond the queried size (for another descriptor's call on the same memory); the
        call under test is always handed exactly the queried bytes.  extra: name -> shape of further buffers of the arena that the
        entry point itself does not know (the outputs of sfm_loss_proj_bwd)."""
        self.c, self.entry, self.ops = c, entry, ops
        self.want, self.ws_bytes = reference(ops, synth, dev, c, entry)
        d = self.d = case_inputs(synth, c)
        self.step = entry.startswith("step")
        self.ins, self.outs = fused_buffers(d, c, self.step)
        names = []
        by_scale = collections.OrderedDict()
        for n in list(self.ins) + list(self.outs):      # arrays of one scale / one source next to each other
            by_scale.setdefault(n[-1] if n[-1].isdigit() else "x", []).append(n)
        for group in by_scale.values():
            names += group
        extra = extra or {}
        names += list(extra)
        res = residues_for(names, scheme, outputs=set(self.outs) | set(extra))
        specs = [(n, (self.ins[n].shape if n in self.ins else extra[n] if n in extra else self.outs[n]), res[n]) for n in names]
        self.ws_region = max(self.ws_bytes, -(-int(ws_room) // 256) * 256)
        specs.append(("ws", self.ws_region, "ws"))
        self.arena = ar = Arena(dev, specs, row_floats=3 * c.shape[3] * c.shape[2])
        for n, a in self.ins.items():
            ar.set(n, a)
            ar.snapshot(n)
        S, n_src = c.shape[4], c.shape[3]
        import torch
        flags = dsrc_flags(c)
        buffers = dict(d_disps=[ar.view("d_disp%d" % s) for s in range(S)], d_poses=[ar.view("d_pose%d" % i) for i in range(n_src)],
                       loss5=ar.view("loss5"), ws=ar.raw("ws").view(torch.uint8)[:self.ws_bytes])
        if "d_mask0" in self.outs:
            buffers["d_masks"] = [ar.view("d_mask%d" % s) for s in range(S)]
        if c.dsrc != "no":
            buffers["d_srcs"] = [ar.view("d_src%d" % s) if flags[s] else None for s in range(S)]
        if c.warped:
            buffers["warped"] = [ar.view("warped%d" % s) for s in range(S)]
        self.fl = _bind_from(ops, c, ar.view, S, n_src, "mask0" in self.ins, buffers=buffers)
        assert self.fl._ws_ptr == ar.ptr("ws") and self.fl._ws_bytes == self.ws_bytes and self.fl._ws_ptr % 256 == 0
        for n in names:
            assert ar.ptr(n) % 16 == res[n], (n, ar.ptr(n) % 16, res[n])
        self.frames = (ar.view("tgt_full"), ar.view("src_full")) if self.step else None
        self.pyr = ([ar.view("tgt%d" % s) for s in range(S)], [ar.view("src%d" % s) for s in range(S)])
        self.what = "%s %s [%s]" % (fcase_id(c), entry, scheme)

    def prefill_outputs(self, value=None):
        """every output = the sentinel (None) or a finite value; d_src is cleared by the binding before a backward either way"""
        for n in self.outs:
            if value is None:
                self.arena.fill_bits(n)
            else:
                self.arena.fill(n, value)

    def fill_ws(self, kind):
        ar = self.arena
        if kind == "zeros":
            ar.fill_bits("ws", 0)
        elif kind == "sentinel":
            ar.fill_bits("ws")
        elif kind == "ff":
            ar.fill_bits("ws", 0xFFFFFFFF)
        else:
            raise ValueError(kind)
        self.reseal_ws()

    def reseal_ws(self):
        """the part of the workspace REGION beyond the queried bytes is a guard of the call under test"""
        self.arena.raw("ws")[self.ws_bytes // 4:].fill_(SENTINEL)

    def run(self):
        _launch(self.ops, self.fl, self.c, self.entry, self.frames)
        return _collect(self.fl, self.c, self.entry, self.pyr)

    def verify(self, got, note="", sentinel_prefill=True):
        ar, what = self.arena, self.what + note
        ar.check(what)
        tail = ar.raw("ws")[self.ws_bytes // 4:]
        assert bool((tail == SENTINEL).all().item()), "%s: bytes beyond the %d queried workspace bytes were written" % (what, self.ws_bytes)
        for n in self.ins:
            ar.unchanged(n)
        for n in self.outs:
            if written_by(self.entry, n):
                if not n.startswith("d_src"):
                    assert not sentinel_prefill or ar.sentinels_left(n) == 0, \
                        "%s: %d elements of the 'overwritten' output %s were never written" % (what, ar.sentinels_left(n), n)
                    assert_bits(got[n], self.want[n], "%s: %s" % (what, n))
            elif sentinel_prefill and not n.startswith("d_src"):
                assert ar.sentinels_left(n) == ar.nbytes(n) // 4, "%s: %s is not an output of this entry point, yet it was written" % (what, n)
        self.verify_d_src(got, what)

    def verify_d_src(self, got, what, plus=None):
        """the accumulated output: criterion of test_d_src_through_the_lds_window (rtol 0, atol 2e-5 max|d_src| of the scale)"""
        for n in got:
            if n.startswith("d_src"):
                w = self.want[n]
                want = w if plus is None else plus[n].astype(np.float64) + w
                assert np.isfinite(got[n]).all(), "%s: %s is not finite" % (what, n)
                if plus is None and not np.array_equal(_i32(got[n]), _i32(w)):
                    parity_note("buffer contracts: %s %s differs from the reference placement in %d of %d elements, max %.3g of max|d_src|" % (
                        what, n, int((_i32(got[n]) != _i32(w)).sum()), w.size, np.abs(got[n] - w).max() / max(float(np.abs(w).max()), 1e-30)))
                np.testing.assert_allclose(got[n], want, rtol=0, atol=2e-5 * max(float(np.abs(w).max()), 1e-30), err_msg="%s: %s" % (what, n))


def _cases(fn):
    return pytest.mark.parametrize("c", FUSED_CASES, ids=fcase_id)(fn)


@_cases
def test_fused_guards_and_inputs(ops, synth, dev, c):
    """Check 1, every entry point of the case: all buffers at 0 mod 16 in a poisoned arena, the workspace exactly the queried bytes
    and poisoned.  Guards intact, inputs bitwise unchanged, no sentinel left in an overwritten output, outputs the reference's bits;
    buffers the entry point does not write stay untouched.  Cases marked `oracle` are also held against the CPU oracle."""
    for entry in entries_of(c):
        p = Placed(ops, synth, dev, c, entry)
        p.verify(p.run())
        if c.oracle and entry == "fwd_bwd":
            from test_loss_gpu import CONFIGS, _check_grads, _check_losses, _check_warped, _oracle
            cfg = MODES[c.mode]
            assert cfg in CONFIGS.values()
            ref = _oracle(p.d, cfg, want_d_src=c.dsrc == "all")
            _check_losses(p.fl.loss5, ref)
            if c.warped and c.proj == "reference_order":
                _check_warped(p.fl, ref, p.what, p.d, flat=True, max_over_flat=0)
            elif c.warped:
                _check_warped(p.fl, ref, p.what, p.d)
            _check_grads(p.fl, ref, c.shape[3], check_src=c.dsrc == "all", check_mask=bool(cfg.get("exp_reg")), what=p.what)


@_cases
def test_fused_old_output_content_is_not_read(ops, synth, dev, c):
    """Check 2: outputs pre-filled with the NaN sentinel and with 1e30 give the reference's bits; d_src pre-filled with a known
    finite array c gives c + reference (the accumulate contract of the header)."""
    for entry in entries_of(c):
        p = Placed(ops, synth, dev, c, entry)
        p.prefill_outputs(FINITE_FILL)
        p.verify(p.run(), " outputs pre-filled with 1e30", sentinel_prefill=False)
        p.prefill_outputs(None)
        p.verify(p.run(), " outputs pre-filled with the sentinel (second call on the same buffers)")
        if c.dsrc != "no" and written_by(entry, "d_src0"):
            rng = np.random.RandomState(3)
            pre = {}
            for n in p.outs:
                if n.startswith("d_src"):      # (of the size of the gradient itself: the rounding of c + x stays below the criterion)
                    pre[n] = (rng.uniform(-1, 1, size=p.outs[n]) * max(float(np.abs(p.want[n]).max()), 1e-3)).astype(F32)
            p.fl._zero_d_src = lambda: [p.arena.set(n, a) for n, a in pre.items()]
            got = p.run()
            p.arena.check(p.what)
            p.verify_d_src(got, p.what + " d_src pre-filled", plus=pre)
            for n in got:
                if not n.startswith("d_src"):
                    assert_bits(got[n], p.want[n], "%s d_src pre-filled: %s" % (p.what, n))


# sfm_loss_proj_bwd: the library's own choice of kernel (after hooks 4 / 5 the header leaves its result unspecified), small shapes
PROJ_CASES = [c for c in FUSED_CASES if c.variant == 0 and c.shape in (A, BS, F3)]
PROJ_OUTS = ("d_proj", "d_intrinsics")


def proj_entries_of(c):
    """(gradient entry point, the `loss` argument that says which one left the sums)"""
    return (("bwd", 0), ("fwd_bwd", 1)) + ((("step_fwd_bwd", 1),) if c.step else ())


def _proj_bwd(ops, fl, loss, d_proj, d_intrinsics):
    import torch
    ops._launch(fl.device, ops.lib.sfm_loss_proj_bwd, fl._desc_ref, loss, fl._ws_arg, fl._ws_bytes,
                C.c_void_p(d_proj) if d_proj else None, C.c_void_p(d_intrinsics) if d_intrinsics else None)
    torch.cuda.synchronize()


def proj_reference(ops, synth, dev, c, entry, loss):
    """the same sequence -- the gradient entry point, then sfm_loss_proj_bwd -- on conventional allocations.  -> name -> host array"""
    import torch
    key = (fcase_id(c), entry, "proj")
    if key not in _ref_cache:
        d = case_inputs(synth, c)
        step = entry.startswith("step")
        ins, outs = fused_buffers(d, c, step)
        t = {k: to_dev(v, dev) for k, v in ins.items()}
        t.update({k: torch.empty(shape, dtype=torch.float32, device=dev) for k, shape in outs.items() if k.startswith(("tgt", "src"))})
        B, _, _, n_src, S = c.shape
        fl = _bind_from(ops, c, t.__getitem__, S, n_src, "mask0" in ins)
        fl.ws.zero_()
        _launch(ops, fl, c, entry, (t.get("tgt_full"), t.get("src_full")))
        out = dict(d_proj=torch.empty((B, S, n_src, 3, 4), device=dev), d_intrinsics=torch.empty((B, S, 3, 3), device=dev))
        _proj_bwd(ops, fl, loss, out["d_proj"].data_ptr(), out["d_intrinsics"].data_ptr())
        _ref_cache[key] = {k: to_np(v).copy() for k, v in out.items()}
    return _ref_cache[key]


@pytest.mark.parametrize("c", PROJ_CASES, ids=fcase_id)
def test_fused_proj_bwd_after_every_gradient_entry(ops, synth, dev, c):
    """sfm_loss_proj_bwd behind sfm_loss_bwd (loss = 0), sfm_loss_fwd_bwd and sfm_step_fwd_bwd (loss = 1), d_proj and d_intrinsics two
    more buffers of the arena.  The guards stay intact; every input and the WHOLE workspace keep their bits ("reads `ws`, never writes
    it"); both outputs are written completely and hold the bits of the same sequence on conventional allocations, whether they held
    1e30 or the sentinel before and at every residue scheme; with one of them NULL the other has the same bits and the NULL one's
    buffer keeps every sentinel."""
    import torch
    B, _, _, n_src, S = c.shape
    extra = collections.OrderedDict(d_proj=(B, S, n_src, 3, 4), d_intrinsics=(B, S, 3, 3))
    for entry, loss in proj_entries_of(c):
        want = proj_reference(ops, synth, dev, c, entry, loss)
        for scheme in ("aligned",) + SCHEMES:
            p = Placed(ops, synth, dev, c, entry, scheme=scheme, extra=extra)
            ar = p.arena
            p.verify(p.run())                                    # the gradient call itself, as in check 1
            ws_before = ar.raw("ws").clone()
            outs_before = {n: ar.raw(n).clone() for n in p.outs}
            ptr = {n: ar.ptr(n) for n in PROJ_OUTS}

            def call(what, fill, **null):
                """one call with both outputs pre-filled by `fill`; null: the outputs passed as NULL"""
                for n in PROJ_OUTS:
                    fill(n)
                _proj_bwd(ops, p.fl, loss, *[None if n in null else ptr[n] for n in PROJ_OUTS])
                what = "%s: sfm_loss_proj_bwd %s" % (p.what, what)
                ar.check(what)
                for n in p.ins:
                    ar.unchanged(n)
                assert torch.equal(ar.raw("ws"), ws_before), "%s wrote the workspace" % what
                for n in p.outs:
                    assert torch.equal(ar.raw(n), outs_before[n]), "%s wrote %s" % (what, n)
                for n in PROJ_OUTS:
                    if n not in null:
                        assert_bits(to_np(ar.view(n)), want[n], "%s: %s" % (what, n))
                return what

            what = call("outputs pre-filled with the sentinel", ar.fill_bits)
            for n in PROJ_OUTS:
                assert ar.sentinels_left(n) == 0, "%s: %d elements of %s were never written" % (what, ar.sentinels_left(n), n)
            if scheme == "aligned":
                call("outputs pre-filled with 1e30", lambda n: ar.fill(n, FINITE_FILL))
                for n in PROJ_OUTS:
                    what = call("with %s = NULL" % n, ar.fill_bits, **{n: True})
                    assert ar.sentinels_left(n) == ar.nbytes(n) // 4, "%s: yet its buffer was written" % what


def _other_descriptor(ops, synth, dev, c):
    """ANOTHER loss on conventional tensors whose workspace has more items per scale than the case's: another mode, a larger batch and
    frame, one more source.  -> (bound FusedLoss factory taking the workspace tensor, its workspace bytes)"""
    B, H, W, n_src, S = c.shape
    mode = "l1" if c.mode in ("ssim_smooth", "edge_aware") else "ssim_smooth"
    oc = _fc((B + 1, H + 13, W + 70, min(n_src + 1, 8), S), mode, "hwc" if c.layout == "planar" else "planar", dsrc="all" if c.dsrc == "no" else "no",
             inputs="default")
    d = case_inputs(synth, oc)
    ins, _ = fused_buffers(d, oc, False)
    t = {k: to_dev(v, dev) for k, v in ins.items()}
    probe = _bind_from(ops, oc, t.__getitem__, S, oc.shape[3], False)
    return (lambda ws: _bind_from(ops, oc, t.__getitem__, S, oc.shape[3], False, buffers=dict(ws=ws))), probe._ws_bytes, oc


@_cases
def test_fused_stale_scratch(ops, synth, dev, c):
    """Check 3: the workspace -- exactly sfm_loss_workspace_bytes of it -- holding zeros, the NaN sentinel, 0xFF bytes, and what a call
    with ANOTHER descriptor (another mode, more items per scale) left on the same memory: once its sfm_loss_fwd_bwd, once its
    sfm_loss_fwd, whose layout of the partial sums differs.  Every output the reference's bits: no item may leave without storing its
    partial, no pixel without its d_src record."""
    import torch
    make_other, other_bytes, oc = _other_descriptor(ops, synth, dev, c)
    for entry in entries_of(c):
        p = Placed(ops, synth, dev, c, entry, ws_room=other_bytes)
        for kind in ("zeros", "sentinel", "ff"):
            p.prefill_outputs(None)
            p.fill_ws(kind)
            p.verify(p.run(), " workspace pre-filled with %s" % kind)
        other = make_other(p.arena.raw("ws").view(torch.uint8)[:max(other_bytes, 256)])
        for other_entry in ("fwd_bwd", "fwd"):
            p.fill_ws("ff")
            _launch(ops, other, oc, other_entry)
            p.arena.check(p.what + " (the other descriptor's call)")
            left = p.arena.raw("ws")[:p.ws_bytes // 4]
            assert int((left != -1).sum().item()) > 0, "the other call left nothing in the workspace of the case"
            p.reseal_ws()
            p.prefill_outputs(None)
            p.verify(p.run(), " workspace holding the leftovers of sfm_loss_%s of %s" % (other_entry, fcase_id(oc)))


@_cases
def test_fused_alignment(ops, synth, dev, c):
    """Check 4: every bound float array -- inputs and outputs, each scale, each pose, loss5 -- at 4 / 8 / 12 mod 16: round-robin (two
    rotations), all at 4, outputs at 0 with inputs at 12.  The workspace stays on its 256-byte boundary.  The reference's bits."""
    for entry in entries_of(c):
        for scheme in SCHEMES + ("rr8",):
            p = Placed(ops, synth, dev, c, entry, scheme=scheme)
            p.verify(p.run())


@pytest.mark.parametrize("entry", ["fwd", "bwd", "fwd_bwd", "step_fwd", "step_fwd_bwd"])
def test_fused_rejections_launch_nothing(ops, synth, dev, entry):
    """A workspace one byte short, or 4 / 128 bytes off its 256-byte boundary, is SFM_ERR_WORKSPACE -- and nothing was launched: every
    output, the workspace and every guard of the arena still hold the sentinel afterwards (sfm_step_*: the pyramids too)."""
    import torch
    _lib = ops._lib
    c = _fc(CS, "ssim_smooth", "hwc", warped=True, dsrc="all", step=True)
    p = Placed(ops, synth, dev, c, entry)
    p.prefill_outputs(None)
    fl, lib = p.fl, ops.lib
    st = ops._stream()
    ws, n = p.arena.ptr("ws"), p.ws_bytes

    def call(ws_ptr, ws_bytes):
        l5, desc = C.c_void_p(p.arena.ptr("loss5")), C.byref(fl.desc)
        if entry == "fwd":
            return lib.sfm_loss_fwd(desc, l5, C.c_void_p(ws_ptr), ws_bytes, st)
        if entry == "bwd":
            return lib.sfm_loss_bwd(desc, 1.0, C.c_void_p(ws_ptr), ws_bytes, st)
        if entry == "fwd_bwd":
            return lib.sfm_loss_fwd_bwd(desc, l5, C.c_void_p(ws_ptr), ws_bytes, st)
        fn = lib.sfm_step_fwd if entry == "step_fwd" else lib.sfm_step_fwd_bwd
        return fn(p.arena.ptr("tgt_full"), p.arena.ptr("src_full"), desc, l5, C.c_void_p(ws_ptr), ws_bytes, st)

    for ws_ptr, ws_bytes, word in ((ws, n - 1, "needed"), (ws + 4, n, "aligned"), (ws + 128, n, "aligned"), (None, n, "needed")):
        assert call(ws_ptr, ws_bytes) == _lib.ERR_WORKSPACE, (ws_ptr, ws_bytes)
        assert "workspace" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    p.arena.check(p.what)
    for name in list(p.outs) + ["ws"]:
        assert p.arena.sentinels_left(name) == p.arena.nbytes(name) // 4, "%s: a rejected call wrote %s" % (p.what, name)
    for name in p.ins:
        p.arena.unchanged(name)
    fl._zero_d_src()
    assert call(ws, n) == 0      # ... and the same arguments with the workspace as queried are accepted
    torch.cuda.synchronize()
    p.verify(_collect(fl, c, entry, p.pyr))


def test_bind_takes_caller_buffers_or_says_why_not(ops, synth, dev):
    """FusedLoss.bind(buffers=...): what this module places its outputs with.  The default still allocates -- the workspace exactly as
    the header states it, sfm_loss_workspace_bytes on a 256-byte boundary -- and a buffer of the wrong shape, a workspace off its
    boundary or too small is refused by name before anything is bound."""
    import torch
    c = _fc(CS, "ssim_smooth", "hwc", dsrc="all")
    d = case_inputs(synth, c)
    ins, _ = fused_buffers(d, c, False)
    t = {k: to_dev(v, dev) for k, v in ins.items()}
    S, n_src = c.shape[4], c.shape[3]
    fl = _bind_from(ops, c, t.__getitem__, S, n_src, False)
    assert fl._ws_ptr % 256 == 0 and fl._ws_bytes == ops.lib.sfm_loss_workspace_bytes(C.byref(fl.desc)) > 0
    assert fl.ws.numel() * fl.ws.element_size() == fl._ws_bytes and fl._ws_ptr == fl.ws.data_ptr()
    n = fl._ws_bytes
    room = torch.empty((n + 512,), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="256-byte boundary"):
        _bind_from(ops, c, t.__getitem__, S, n_src, False, buffers=dict(ws=room[4:4 + n]))
    with pytest.raises(ValueError, match="need %d bytes" % n):
        _bind_from(ops, c, t.__getitem__, S, n_src, False, buffers=dict(ws=room[:n - 256]))
    with pytest.raises(TypeError, match="d_disps"):
        _bind_from(ops, c, t.__getitem__, S, n_src, False, buffers=dict(d_disps=[torch.empty((1,), device=dev)] * S))
    with pytest.raises(TypeError, match="loss5"):
        _bind_from(ops, c, t.__getitem__, S, n_src, False, buffers=dict(loss5=torch.empty((5,), dtype=torch.float64, device=dev)))
    mine = torch.full((5,), 7.0, device=dev)
    got = _bind_from(ops, c, t.__getitem__, S, n_src, False, buffers=dict(loss5=mine, ws=room[:n]))
    assert got.loss5 is mine and got._ws_ptr == room.data_ptr() and got._ws_bytes == n
    assert_bits(to_np(got.forward_backward()), to_np(fl.forward_backward()), "loss5 in the caller's buffer")


PROBE_CASES = [_fc((2, 84, 70, 2, 2), "ssim_smooth", "hwc", warped=True, dsrc="all", step=True), _fc((2, 84, 70, 2, 2), "edge_aware", "planar"),
               _fc((2, 84, 70, 2, 2), "l1", "hwc", dsrc="sub"), _fc((2, 84, 70, 2, 2), "explain", "planar", proj="reference_order", warped=True)]


def run_all_checks(ops, synth, dev, c):
    """the four checks of one case (the child process of test_forced_chunk_heights_keep_the_buffer_contract)"""
    for fn in (test_fused_guards_and_inputs, test_fused_old_output_content_is_not_read, test_fused_stale_scratch, test_fused_alignment):
        fn(ops, synth, dev, c)


@pytest.mark.parametrize("rows", [4, 28])
def test_forced_chunk_heights_keep_the_buffer_contract(rows):
    """Both extremes of the planner (SFM_CHUNK_ROWS = 4 / 28, read once per process: a child process, as
    test_loss_edges_gpu.py::test_forced_chunk_heights): the four checks on PROBE_CASES -- the shape of the existing probe -- with
    chunks of 4 rows (more halo rows than rows, the most partial sums per scale) and of 28 rows."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SFM_CHUNK_ROWS=str(rows))
    r = subprocess.run([sys.executable, os.path.join(here, "forced_chunks_probe.py"), "buffers"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and ("OK buffers rows=%d" % rows) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# =====================================================================================================================================
# 3. the operators of sfm_ops.hip
# =====================================================================================================================================
class OpCase:
    """One call of one operator entry point.
    ins: name -> host array;  outs: name -> (shape, kind) with kind "over" (overwritten: bitwise), "acc" (accumulated with atomics:
    rtol 1e-5 / atol 1e-6; cleared before the call unless a check pre-fills it) or "keep" (the header says the call ignores it: stays
    untouched);  ws: scratch bytes or 0;  call(ptr, ws_ptr, ws_bytes, stream) -> return code, `ptr` name -> address."""

    def __init__(self, ident, entry, ins, outs, call, ws=0, row=0, fixed=None):
        self.id, self.entry, self.ins, self.outs, self.call, self.ws, self.row = ident, entry, ins, outs, call, ws, row
        self.fixed = fixed or {}      # name -> residue that the case pins whatever the scheme (the band-kernel case)
        assert entry in COVERED, entry


def _lists(ptr, names):
    return (C.c_void_p * len(names))(*[ptr(n) if n is not None else None for n in names])


def _op_cases(ops, synth):
    L = ops.lib
    rng = np.random.RandomState(77)
    rnd = lambda *shape: rng.normal(size=shape).astype(F32)
    cases = []
    from test_ops_edges_gpu import make_field

    # ---- pose -> projection
    for N in (1, 64, 65):
        pose = (0.3 * rnd(N, 6)).astype(F32)
        K = np.tile(np.array([[240, 0, 200], [0, 245, 60], [0, 0, 1]], F32), (N, 1, 1)) * (1 + 0.01 * rnd(N, 1, 1))
        ins = dict(pose=pose, K=K.astype(F32))
        cases.append(OpCase("pose_proj_fwd-N%d" % N, "sfm_pose_proj_fwd", ins, dict(proj=((N, 4, 4), "over")),
                            lambda p, w, nb, st, N=N: L.sfm_pose_proj_fwd(p("pose"), p("K"), p("proj"), N, st)))
        ins = dict(pose=pose, K=K.astype(F32), g_proj=rnd(N, 4, 4))
        cases.append(OpCase("pose_proj_bwd-N%d" % N, "sfm_pose_proj_bwd", ins, dict(d_pose=((N, 6), "over")),
                            lambda p, w, nb, st, N=N: L.sfm_pose_proj_bwd(p("pose"), p("K"), p("g_proj"), p("d_pose"), N, st)))
        cases.append(OpCase("pose_proj_bwd_k-N%d" % N, "sfm_pose_proj_bwd_k", ins, dict(d_K=((N, 3, 3), "over")),
                            lambda p, w, nb, st, N=N: L.sfm_pose_proj_bwd_k(p("pose"), p("K"), p("g_proj"), p("d_K"), N, st)))

    # ---- projective_inverse_warp
    for (N, Cc, H, W, drows, with_src) in ((1, 3, 3, 3, 1, True), (2, 3, 8, 61, 3, False), (2, 2, 33, 65, 1, True), (1, 3, 16, 64, 3, True)):
        d = synth.make_inputs(B=N, H=H, W=W, n_src=1, n_scales=1, seed=33)
        imgs = np.ascontiguousarray(d["src"].reshape(N, -1, H, W)[:, :Cc])
        depth = np.ascontiguousarray(np.repeat((1.0 / d["disps"][0]).reshape(N, 1, H * W), drows, axis=1).astype(F32))
        ins = dict(src=imgs, depth=depth, pose=d["poses"][0], K=np.ascontiguousarray(d["intrinsics"][:, 0]))
        tag = "N%d-C%d-%dx%d-rows%d" % (N, Cc, H, W, drows)
        cases.append(OpCase("warp_fwd-" + tag, "sfm_warp_fwd", ins, dict(warped=((N, Cc, H, W), "over")),
                            lambda p, w, nb, st, a=(N, Cc, H, W), r=drows: L.sfm_warp_fwd(p("src"), p("depth"), r, p("pose"), p("K"), p("warped"), *a, st),
                            row=W))
        ins = dict(ins, g_warped=rnd(N, Cc, H, W))
        outs = collections.OrderedDict(d_depth=((N, drows, H * W), "over"), d_pose=((N, 6), "over"))
        if with_src:
            outs["d_src"] = ((N, Cc, H, W), "acc")
        cases.append(OpCase("warp_bwd-%s-%s" % (tag, "d_src" if with_src else "null_d_src"), "sfm_warp_bwd", ins, outs,
                            lambda p, w, nb, st, a=(N, Cc, H, W), r=drows, ws_=with_src: L.sfm_warp_bwd(
                                p("src"), p("depth"), r, p("pose"), p("K"), p("g_warped"), p("d_depth"), p("d_pose"), p("d_src") if ws_ else None,
                                w, nb, *a, st),
                            ws=int(L.sfm_warp_bwd_workspace_bytes(N, H, W)), row=W))
        cases.append(OpCase("warp_intrinsics_bwd-" + tag, "sfm_warp_intrinsics_bwd", ins, dict(d_K=((N, 3, 3), "over")),
                            lambda p, w, nb, st, a=(N, Cc, H, W), r=drows: L.sfm_warp_intrinsics_bwd(
                                p("src"), p("depth"), r, p("pose"), p("K"), p("g_warped"), p("d_K"), w, nb, *a, st),
                            ws=int(L.sfm_warp_intrinsics_bwd_workspace_bytes(N, H, W)), row=W))

    # ---- the two samplers
    for (family, N, Cc, H, W, oH, oW, with_gx) in (("shift", 1, 1, 4, 66, 1, 65, True), ("smooth", 2, 3, 9, 61, 8, 65, True),
                                                  ("zoom2", 2, 5, 32, 64, 33, 64, False), ("zoomout", 1, 2, 7, 65, 9, 63, True)):
        x, gy = rnd(N, Cc, H, W), rnd(N, Cc, oH, oW)
        grid = make_field(family, N, max(H, 2), max(W, 2), oH, oW, rng)
        pix = np.ascontiguousarray(np.stack([(grid[:, 0] + 1) * (W - 1) / 2.0, (grid[:, 1] + 1) * (H - 1) / 2.0], axis=1).astype(F32))
        tag = "%s-N%d-C%d-%dx%d-to-%dx%d" % (family, N, Cc, H, W, oH, oW)
        a = (N, Cc, H, W, oH, oW)
        for name, fwd, bwd, g, gx_kind in (("sampler", L.sfm_sampler_fwd, L.sfm_sampler_bwd, grid, "acc"),
                                           ("sampler_interp", L.sfm_sampler_interp_fwd, L.sfm_sampler_interp_bwd, pix, "over")):
            cases.append(OpCase("%s_fwd-%s" % (name, tag), "sfm_%s_fwd" % name, dict(x=x, grid=g), dict(y=((N, Cc, oH, oW), "over")),
                                lambda p, w, nb, st, f=fwd, a=a: f(p("x"), p("grid"), p("y"), *a, st), row=max(W, oW)))
            outs = collections.OrderedDict(ggrid=((N, 2, oH, oW), "over"))
            if with_gx:
                outs["gx"] = ((N, Cc, H, W), gx_kind)
            cases.append(OpCase("%s_bwd-%s-%s" % (name, tag, "gx" if with_gx else "null_gx"), "sfm_%s_bwd" % name, dict(x=x, grid=g, gy=gy), outs,
                                lambda p, w, nb, st, f=bwd, a=a, wg=with_gx: f(p("x"), p("grid"), p("gy"), p("ggrid"), p("gx") if wg else None, *a, st),
                                row=max(W, oW)))

    # ---- resize
    for (N, Cc, H, W, oH, oW) in ((2, 3, 37, 70, 18, 35), (1, 1, 1, 1, 1, 1), (1, 2, 8, 64, 32, 65), (1, 1, 9, 61, 1, 64)):
        cases.append(OpCase("resize-N%d-C%d-%dx%d-to-%dx%d" % (N, Cc, H, W, oH, oW), "sfm_resize_fwd", dict(x=rnd(N, Cc, H, W)),
                            dict(y=((N, Cc, oH, oW), "over")),
                            lambda p, w, nb, st, a=(N, Cc, H, W, oH, oW): L.sfm_resize_fwd(p("x"), p("y"), *a, st), row=max(W, oW)))

    # ---- the pyramids
    for (N, Cc, H, W, S) in ((1, 6, 37, 70, 3), (2, 3, 9, 5, 3), (2, 3, 32, 64, 4), (1, 3, 8, 61, 2)):
        outs = collections.OrderedDict(("y%d" % s, ((N, Cc, max(H >> s, 1), max(W >> s, 1)), "keep" if s == 0 else "over")) for s in range(S))
        cases.append(OpCase("pyramid-N%d-C%d-%dx%d-S%d" % (N, Cc, H, W, S), "sfm_pyramid_fwd", dict(x=rnd(N, Cc, H, W)), outs,
                            lambda p, w, nb, st, a=(N, Cc, H, W, S): L.sfm_pyramid_fwd(p("x"), _lists(p, ["y%d" % s for s in range(a[4])]), *a, st), row=W))
    for (N, G, H, W, S) in ((1, 2, 37, 70, 3), (2, 1, 9, 5, 3), (2, 1, 32, 64, 4), (1, 2, 16, 68, 3)):      # W % 4 != 0 twice, == 0 twice
        for variant in (0, 1):
            tag = "N%d-G%d-%dx%d-S%d-%s" % (N, G, H, W, S, "band" if variant == 0 else "per_pixel")
            outs = collections.OrderedDict(("y%d" % s, ((N, G, H >> s, W >> s, 3), "over")) for s in range(S))

            def call_hwc(p, w, nb, st, a=(N, G, H, W, S), v=variant):
                ops.check(L.sfm_pyramid_variant(v))
                return L.sfm_pyramid_hwc_fwd(p("x"), _lists(p, ["y%d" % s for s in range(a[4])]), *a, st)
            cases.append(OpCase("pyramid_hwc-" + tag, "sfm_pyramid_hwc_fwd", dict(x=rnd(N, 3 * G, H, W)), outs, call_hwc, row=3 * W))
            outs = collections.OrderedDict()
            for s in range(S):
                outs["yt%d" % s], outs["ys%d" % s] = ((N, 1, H >> s, W >> s, 3), "over"), ((N, G, H >> s, W >> s, 3), "over")

            def call_pair(p, w, nb, st, a=(N, G, H, W, S), v=variant):
                ops.check(L.sfm_pyramid_variant(v))
                return L.sfm_pyramid_pair_hwc_fwd(p("tgt"), p("src"), _lists(p, ["yt%d" % s for s in range(a[4])]),
                                                  _lists(p, ["ys%d" % s for s in range(a[4])]), *a, st)
            cases.append(OpCase("pyramid_pair_hwc-" + tag, "sfm_pyramid_pair_hwc_fwd", dict(tgt=rnd(N, 3, H, W), src=rnd(N, 3 * G, H, W)), outs,
                                call_pair, row=3 * W))
    # launch_pyramid_band looks at x and y[0] only: those at 0 mod 16, y[1..] at 4 / 8 / 12 -- still the band kernel
    N, G, H, W, S = 2, 2, 32, 64, 4
    outs = collections.OrderedDict(("y%d" % s, ((N, G, H >> s, W >> s, 3), "over")) for s in range(S))
    cases.append(OpCase("pyramid_hwc-band_with_unaligned_small_scales", "sfm_pyramid_hwc_fwd", dict(x=rnd(N, 3 * G, H, W)), outs,
                        lambda p, w, nb, st, a=(N, G, H, W, S): L.sfm_pyramid_hwc_fwd(p("x"), _lists(p, ["y%d" % s for s in range(a[4])]), *a, st),
                        row=3 * W, fixed=dict(x=0, y0=0, y1=4, y2=8, y3=12)))
    outs = collections.OrderedDict()
    for s in range(S):
        outs["yt%d" % s], outs["ys%d" % s] = ((N, 1, H >> s, W >> s, 3), "over"), ((N, G, H >> s, W >> s, 3), "over")
    cases.append(OpCase("pyramid_pair_hwc-band_with_unaligned_small_scales", "sfm_pyramid_pair_hwc_fwd", dict(tgt=rnd(N, 3, H, W), src=rnd(N, 3 * G, H, W)), outs,
                        lambda p, w, nb, st, a=(N, G, H, W, S): L.sfm_pyramid_pair_hwc_fwd(
                            p("tgt"), p("src"), _lists(p, ["yt%d" % s for s in range(a[4])]), _lists(p, ["ys%d" % s for s in range(a[4])]), *a, st),
                        row=3 * W, fixed=dict(tgt=0, src=0, yt0=0, ys0=0, yt1=4, ys1=8, yt2=12, ys2=4, yt3=8, ys3=12)))

    # ---- DispNet's activation: ragged and empty scales (test_disp_act_ragged_empty_and_saturated)
    for numel in ([1, 255, 256, 0, 257, 65537, 3, 1000], [0, 7, 0, 0, 512, 1, 0, 4097], [300]):
        S = len(numel)
        live = [k for k in range(S) if numel[k]]
        nn = (C.c_longlong * S)(*numel)
        xs = {"x%d" % k: (3 * rnd(numel[k])).astype(F32) for k in live}
        nm = lambda pre, k, live=live: (pre + str(k)) if k in live else None
        cases.append(OpCase("disp_act_fwd-%s" % "_".join(map(str, numel)), "sfm_disp_act_fwd", xs,
                            collections.OrderedDict(("d%d" % k, ((numel[k],), "over")) for k in live),
                            lambda p, w, nb, st, S=S, nn=nn, nm=nm: L.sfm_disp_act_fwd(
                                _lists(p, [nm("x", k) for k in range(S)]), _lists(p, [nm("d", k) for k in range(S)]), nn, S, st)))
        ins = {"d%d" % k: (10.0 / (1.0 + np.exp(-xs["x%d" % k].astype(np.float64))) + 0.01).astype(F32) for k in live}
        ins.update({"g%d" % k: rnd(numel[k]) for k in live})
        cases.append(OpCase("disp_act_bwd-%s" % "_".join(map(str, numel)), "sfm_disp_act_bwd", ins,
                            collections.OrderedDict(("gx%d" % k, ((numel[k],), "over")) for k in live),
                            lambda p, w, nb, st, S=S, nn=nn, nm=nm: L.sfm_disp_act_bwd(
                                _lists(p, [nm("d", k) for k in range(S)]), _lists(p, [nm("g", k) for k in range(S)]),
                                _lists(p, [nm("gx", k) for k in range(S)]), nn, S, st)))

    # ---- data augmentation
    for (Cc, Fr, H, W) in ((3, 5, 17, 23), (4, 1, 32, 104), (3, 1, 9, 7)):
        B = 4
        params = []
        for b in range(B):
            sc = (1.0, 1.15, 1.07, 1.15)[b]
            sh, sw = int(H * sc), int(W * sc)
            params.append((sh, sw, (0, sh - H, (sh - H) // 2, sh - H)[b], (0, sw - W, (sw - W) // 2, 0)[b], float(b in (1, 2))))
        cases.append(OpCase("augment-C%d-F%d-%dx%d" % (Cc, Fr, H, W), "sfm_augment_fwd",
                            dict(imgs=rng.uniform(-1, 1, size=(B, Fr, Cc, H, W)).astype(F32), params=np.asarray(params, F32)),
                            dict(out=((B, Fr, Cc, H, W), "over")),
                            lambda p, w, nb, st, a=(B, Fr, Cc, H, W): L.sfm_augment_fwd(p("imgs"), p("params"), p("out"), *a, st), row=W))
    return cases


_op_cache = {}


def op_cases(ops, synth):
    if "cases" not in _op_cache:
        _op_cache["cases"] = collections.OrderedDict((c.id, c) for c in _op_cases(ops, synth))
    return _op_cache["cases"]


# the ids, spelled out so that every case is a named test (the list is checked against what _op_cases builds)
OP_IDS = """pose_proj_fwd-N1 pose_proj_bwd-N1 pose_proj_bwd_k-N1 pose_proj_fwd-N64 pose_proj_bwd-N64 pose_proj_bwd_k-N64
pose_proj_fwd-N65 pose_proj_bwd-N65 pose_proj_bwd_k-N65
warp_fwd-N1-C3-3x3-rows1 warp_bwd-N1-C3-3x3-rows1-d_src warp_intrinsics_bwd-N1-C3-3x3-rows1
warp_fwd-N2-C3-8x61-rows3 warp_bwd-N2-C3-8x61-rows3-null_d_src warp_intrinsics_bwd-N2-C3-8x61-rows3
warp_fwd-N2-C2-33x65-rows1 warp_bwd-N2-C2-33x65-rows1-d_src warp_intrinsics_bwd-N2-C2-33x65-rows1
warp_fwd-N1-C3-16x64-rows3 warp_bwd-N1-C3-16x64-rows3-d_src warp_intrinsics_bwd-N1-C3-16x64-rows3
sampler_fwd-shift-N1-C1-4x66-to-1x65 sampler_bwd-shift-N1-C1-4x66-to-1x65-gx sampler_interp_fwd-shift-N1-C1-4x66-to-1x65
sampler_interp_bwd-shift-N1-C1-4x66-to-1x65-gx sampler_fwd-smooth-N2-C3-9x61-to-8x65 sampler_bwd-smooth-N2-C3-9x61-to-8x65-gx
sampler_interp_fwd-smooth-N2-C3-9x61-to-8x65 sampler_interp_bwd-smooth-N2-C3-9x61-to-8x65-gx sampler_fwd-zoom2-N2-C5-32x64-to-33x64
sampler_bwd-zoom2-N2-C5-32x64-to-33x64-null_gx sampler_interp_fwd-zoom2-N2-C5-32x64-to-33x64
sampler_interp_bwd-zoom2-N2-C5-32x64-to-33x64-null_gx sampler_fwd-zoomout-N1-C2-7x65-to-9x63 sampler_bwd-zoomout-N1-C2-7x65-to-9x63-gx
sampler_interp_fwd-zoomout-N1-C2-7x65-to-9x63 sampler_interp_bwd-zoomout-N1-C2-7x65-to-9x63-gx
resize-N2-C3-37x70-to-18x35 resize-N1-C1-1x1-to-1x1 resize-N1-C2-8x64-to-32x65 resize-N1-C1-9x61-to-1x64
pyramid-N1-C6-37x70-S3 pyramid-N2-C3-9x5-S3 pyramid-N2-C3-32x64-S4 pyramid-N1-C3-8x61-S2
pyramid_hwc-N1-G2-37x70-S3-band pyramid_pair_hwc-N1-G2-37x70-S3-band pyramid_hwc-N1-G2-37x70-S3-per_pixel pyramid_pair_hwc-N1-G2-37x70-S3-per_pixel
pyramid_hwc-N2-G1-9x5-S3-band pyramid_pair_hwc-N2-G1-9x5-S3-band pyramid_hwc-N2-G1-9x5-S3-per_pixel pyramid_pair_hwc-N2-G1-9x5-S3-per_pixel
pyramid_hwc-N2-G1-32x64-S4-band pyramid_pair_hwc-N2-G1-32x64-S4-band pyramid_hwc-N2-G1-32x64-S4-per_pixel pyramid_pair_hwc-N2-G1-32x64-S4-per_pixel
pyramid_hwc-N1-G2-16x68-S3-band pyramid_pair_hwc-N1-G2-16x68-S3-band pyramid_hwc-N1-G2-16x68-S3-per_pixel pyramid_pair_hwc-N1-G2-16x68-S3-per_pixel
pyramid_hwc-band_with_unaligned_small_scales pyramid_pair_hwc-band_with_unaligned_small_scales
disp_act_fwd-1_255_256_0_257_65537_3_1000 disp_act_bwd-1_255_256_0_257_65537_3_1000 disp_act_fwd-0_7_0_0_512_1_0_4097
disp_act_bwd-0_7_0_0_512_1_0_4097 disp_act_fwd-300 disp_act_bwd-300
augment-C3-F5-17x23 augment-C4-F1-32x104 augment-C3-F1-9x7""".split()


def test_op_case_list_is_complete(ops, synth):
    assert list(op_cases(ops, synth)) == OP_IDS
    assert len(OP_IDS) == 72 and len(set(OP_IDS)) == 72
    here = {k for k, test in COVERED.items() if "::" not in test}
    assert {c.entry for c in op_cases(ops, synth).values()} | {"sfm_scale_arrays"} | {k for k in here if k.startswith(("sfm_loss", "sfm_step"))} == here
    assert {k for k, test in COVERED.items() if test == "test_op_guards_and_inputs"} == {c.entry for c in op_cases(ops, synth).values()}


def op_reference(ops, dev, oc):
    """the same call on standalone, conventionally allocated buffers: outputs from torch.empty (accumulated ones zeroed), the
    workspace zero-filled.  -> name -> host array"""
    import torch
    if oc.id in _op_cache:
        return _op_cache[oc.id]
    t = {k: to_dev(v, dev) for k, v in oc.ins.items()}
    for k, (shape, kind) in oc.outs.items():
        t[k] = torch.zeros(shape, dtype=torch.float32, device=dev) if kind == "acc" else torch.empty(shape, dtype=torch.float32, device=dev)
    ws = torch.zeros((max(oc.ws, 4),), dtype=torch.uint8, device=dev)
    ops.check(oc.call(lambda n: C.c_void_p(t[n].data_ptr()), C.c_void_p(ws.data_ptr()), oc.ws, ops._stream()))
    torch.cuda.synchronize()
    _op_cache[oc.id] = {k: to_np(t[k]).copy() for k, (_, kind) in oc.outs.items() if kind != "keep"}
    return _op_cache[oc.id]


class PlacedOp:
    def __init__(self, ops, dev, oc, scheme="aligned"):
        self.ops, self.oc = ops, oc
        self.want = op_reference(ops, dev, oc)
        names = list(oc.ins) + list(oc.outs)
        res = residues_for(names, scheme, outputs=set(oc.outs))
        res.update(oc.fixed)
        specs = [(n, oc.ins[n].shape if n in oc.ins else oc.outs[n][0], res[n]) for n in names]
        if oc.ws:
            specs.append(("ws", oc.ws, "ws"))
        self.arena = ar = Arena(dev, specs, row_floats=oc.row)
        for n, a in oc.ins.items():
            ar.set(n, a)
            ar.snapshot(n)
        for n in names:
            assert ar.ptr(n) % 16 == res[n]
        self.what = "%s [%s]" % (oc.id, scheme)

    def run(self, acc_prefill=None):
        import torch
        ar, oc = self.arena, self.oc
        for n, (_, kind) in oc.outs.items():
            if kind == "acc":
                if acc_prefill is None:
                    ar.fill(n, 0.0)
                else:
                    ar.set(n, acc_prefill[n])
        self.ops.check(oc.call(lambda n: C.c_void_p(ar.ptr(n)), C.c_void_p(ar.ptr("ws")) if oc.ws else None, oc.ws, self.ops._stream()))
        torch.cuda.synchronize()
        return {n: to_np(ar.view(n)).copy() for n in oc.outs}

    def verify(self, got, note="", sentinel_prefill=True, acc_prefill=None):
        ar, oc, what = self.arena, self.oc, self.what + note
        ar.check(what)
        for n in oc.ins:
            ar.unchanged(n)
        for n, (_, kind) in oc.outs.items():
            if kind == "keep":
                assert not sentinel_prefill or ar.sentinels_left(n) == ar.nbytes(n) // 4, "%s: %s is ignored by the call, yet it was written" % (what, n)
            elif kind == "over":
                assert not sentinel_prefill or ar.sentinels_left(n) == 0, \
                    "%s: %d elements of the 'overwritten' output %s were never written" % (what, ar.sentinels_left(n), n)
                assert_bits(got[n], self.want[n], "%s: %s" % (what, n))
            else:      # criterion of test_torch_api_gpu.py::test_operator_functions_match_ops_bitwise for outputs accumulated with atomics
                want = self.want[n] if acc_prefill is None else acc_prefill[n].astype(np.float64) + self.want[n]
                np.testing.assert_allclose(got[n], want, rtol=1e-5, atol=1e-6, err_msg="%s: %s" % (what, n))


def _op_ids(fn):
    return pytest.mark.parametrize("ident", OP_IDS)(fn)


@_op_ids
def test_op_guards_and_inputs(ops, synth, dev, ident):
    """Check 1 for the operators: guards intact, inputs unchanged, overwritten outputs written completely and equal to the standalone
    call's bits (accumulated ones within the atomics criterion), ignored pointers (y[0] of sfm_pyramid_fwd) untouched."""
    p = PlacedOp(ops, dev, op_cases(ops, synth)[ident])
    p.verify(p.run())


@_op_ids
def test_op_old_output_content_is_not_read(ops, synth, dev, ident):
    """Check 2: overwritten outputs pre-filled with 1e30, then with the sentinel: the same bits; an accumulated output pre-filled with
    a known array c: c + reference."""
    oc = op_cases(ops, synth)[ident]
    p = PlacedOp(ops, dev, oc)
    for n, (_, kind) in oc.outs.items():
        if kind == "over":
            p.arena.fill(n, FINITE_FILL)
    p.verify(p.run(), " outputs pre-filled with 1e30", sentinel_prefill=False)
    for n, (_, kind) in oc.outs.items():
        if kind == "over":
            p.arena.fill_bits(n)
    p.verify(p.run(), " outputs pre-filled with the sentinel")
    if any(kind == "acc" for _, kind in oc.outs.values()):
        rng = np.random.RandomState(9)
        pre = {n: rng.normal(size=shape).astype(F32) for n, (shape, kind) in oc.outs.items() if kind == "acc"}
        p.verify(p.run(acc_prefill=pre), " accumulated outputs pre-filled", acc_prefill=pre)


@pytest.mark.parametrize("ident", [i for i in OP_IDS if i.startswith(("warp_bwd-", "warp_intrinsics_bwd-"))])
def test_op_stale_scratch(ops, synth, dev, ident):
    """Check 3 for the two operators with a workspace (sfm_warp_bwd: the per-block pose partials; sfm_warp_intrinsics_bwd: the
    per-block sums of gPm and G): exactly the queried bytes, holding zeros, the NaN sentinel, 0xFF bytes, or the partials of a call
    on other inputs -- the same bits; one byte less is rejected."""
    oc = op_cases(ops, synth)[ident]
    p = PlacedOp(ops, dev, oc)
    for kind, word in (("zeros", 0), ("sentinel", SENTINEL), ("0xFF", 0xFFFFFFFF)):
        p.arena.fill_bits("ws", word)
        p.verify(p.run(), " workspace pre-filled with %s" % kind)
    keep = {n: p.arena.view(n).clone() for n in ("g_warped", "pose")}
    p.arena.view("g_warped").mul_(-3.0)
    p.arena.view("pose").add_(0.05)
    p.run()
    for n, t in keep.items():
        p.arena.view(n).copy_(t)
    p.verify(p.run(), " workspace holding the partials of a call on other inputs")
    for n in oc.outs:
        p.arena.fill_bits(n)
    p.arena.fill_bits("ws")
    rc = oc.call(lambda n: C.c_void_p(p.arena.ptr(n)), C.c_void_p(p.arena.ptr("ws")), oc.ws - 1, ops._stream())
    assert rc == ops._lib.ERR_WORKSPACE and "workspace" in ops._lib.last_error()
    import torch
    torch.cuda.synchronize()
    p.arena.check(p.what)
    for n in list(oc.outs) + ["ws"]:
        assert p.arena.sentinels_left(n) == p.arena.nbytes(n) // 4, "a rejected %s wrote %s" % (oc.entry, n)


@_op_ids
def test_op_alignment(ops, synth, dev, ident):
    """Check 4: every array at 4 / 8 / 12 mod 16 (round-robin in two rotations, all at 4, outputs at 0 with inputs at 12): the bits of
    the aligned standalone call.  For the pixel-interleaved pyramids that means: an unaligned x or y[0] takes the per-pixel kernel and
    gives the band kernel's bits (W % 4 == 0 and != 0); the `band_with_unaligned_small_scales` cases pin x and y[0] at 0 mod 16 and
    y[1..] at 4 / 8 / 12, which stays on the band kernel."""
    oc = op_cases(ops, synth)[ident]
    for scheme in SCHEMES + ("rr8",):
        p = PlacedOp(ops, dev, oc, scheme=scheme)
        p.verify(p.run())


@pytest.mark.parametrize("gyv", [1.0, -2.5, 0.0, float("inf"), float("nan")])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_scale_arrays_in_an_arena(ops, dev, gyv, in_place):
    """sfm_scale_arrays as test_torch_api_gpu.py::test_scale_arrays_edges runs it -- ragged arrays at odd float offsets, outputs
    co-aligned with their input or not, empty arrays between them, in place and out of place -- with guards around every array:
    y = x * gy bit for bit (one IEEE multiply), nothing outside y written, x unchanged (out of place), gy unchanged."""
    import torch
    sizes = [0, 1, 3, 5, 64, 1000, 257, 4099]
    rng = np.random.RandomState(5)
    specs, xs = [("gy", (1,), 4)], {}
    for k, n in enumerate(sizes):
        if n:
            xs[k] = rng.normal(size=n).astype(F32)
            xs[k][n // 2] = 0.0
            specs.append(("x%d" % k, (n,), (4, 8, 12, 0)[k % 4]))
            if not in_place:
                specs.append(("y%d" % k, (n,), (4, 8, 12, 0)[k % 4] if k % 2 else (8, 0, 4, 12)[k % 4]))
    ar = Arena(dev, specs)
    ar.set("gy", np.array([gyv], F32))
    ar.snapshot("gy")
    for k, a in xs.items():
        ar.set("x%d" % k, a)
        ar.snapshot("x%d" % k)
    ptr = lambda pre, k: ar.ptr(pre + str(k)) if sizes[k] else None
    n = len(sizes)
    X = (C.c_void_p * n)(*[ptr("x", k) for k in range(n)])
    Y = X if in_place else (C.c_void_p * n)(*[ptr("y", k) for k in range(n)])
    ops.check(ops.lib.sfm_scale_arrays(X, Y, (C.c_longlong * n)(*sizes), n, C.c_void_p(ar.ptr("gy")), ops._stream()))
    torch.cuda.synchronize()
    ar.check("sfm_scale_arrays gy=%r" % gyv)
    ar.unchanged("gy")
    for k, a in xs.items():      # (the reference of test_scale_arrays_edges: torch's own x * gy on the device)
        if not in_place:
            ar.unchanged("x%d" % k)
        want = to_np(to_dev(a, dev) * torch.tensor(gyv, device=dev))
        assert_bits(to_np(ar.view(("x" if in_place else "y") + str(k))), want, "array %d (%d elements)" % (k, a.size))
