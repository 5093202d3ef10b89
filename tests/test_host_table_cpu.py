"""The Python host layer without a GPU: what torch_api._plan decides for a grid of configurations (descriptor bytes, workspace,
scratch offsets, gradient spans) and what every entry point answers to arguments it refuses before the first data_ptr(), compared
with the tables tests/golden/make_host_table.py wrote at the commit before the host layer was rewritten (64c4253)."""
import importlib.util
import json
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_host_table", os.path.join(GOLD, "make_host_table.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


@pytest.fixture(scope="module")
def plans():
    with np.load(os.path.join(GOLD, "host_plans.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rejects():
    with open(os.path.join(GOLD, "host_rejects.json")) as f:
        return json.load(f)


def test_the_plan_grid_is_the_fixture(plans):
    assert plans["params"].tolist() == [list(p) for p in T.grid()]
    assert len(plans["params"]) == 2 * 3 * 3 * 2 * 2 * 3 * 2 * 2
    planar = plans["params"][:, 1] == 2
    ok = plans["error"] == ""
    assert not plans["hwc"][planar].any() and plans["hwc"][~planar & ok].all()
    # (a 16x24 frame has a 2x3 fourth scale: the library's own refusal, through the zero-bytes answer of sfm_loss_workspace_bytes)
    assert (~ok).sum() == 144 and set(plans["error"][~ok]) == {"TypeError: sfm_loss: scale 3 is 2x3, need H,W >= 3"}
    assert all(p[1] == 0 and p[3] == 4 for p in plans["params"][~ok])


def test_every_plan_is_the_pinned_one_byte_for_byte(plans):
    now = T.plan_tables()
    assert sorted(now) == sorted(plans)
    bad = []
    for k in range(len(plans["params"])):
        for name in plans:
            if not np.array_equal(now[name][k], plans[name][k]):
                bad.append("%s: %s" % (dict(zip(T.PARAMS, plans["params"][k].tolist())), name))
    assert not bad, "%d fields differ:\n%s" % (len(bad), "\n".join(bad[:10]))


def test_the_refusals_are_the_fixture(rejects):
    assert [r[0] for r in rejects] == [label for label, _ in T.cases()]
    heads = {r[0].split(":")[0] for r in rejects}
    assert {"resize", "pose_proj_fwd", "pose_proj_bwd", "warp_fwd", "warp_bwd", "sampler_fwd", "sampler_bwd", "interp_fwd",
            "interp_bwd", "pyramid", "pyramid_hwc", "pyramid_pair_hwc", "disp_act_fwd", "disp_act_bwd", "FusedLoss", "bind", "loss",
            "scale_arrays_into", "disp_activation", "augment_images", "warp_pyramid", "photometric_error", "warp_pyramid_fwd",
            "warp_pyramid_bwd", "photo_error_fwd", "photo_error_bwd", "resize_bwd", "warp_bwd_intrinsics", "pose_proj_bwd_intrinsics"} <= heads


def test_every_refusal_has_the_pinned_class_and_text(rejects):
    bad = []
    for (label, fn), (_, cls, text) in zip(T.cases(), rejects):
        try:
            got = T.refusal(fn)
        except Exception as e:          # (another class of exception, or none: reported with the rest)
            got = [type(e).__name__, str(e)]
        if got != [cls, text]:
            bad.append("%s: pinned %s %r, now %s %r" % (label, cls, text, got[0], got[1]))
    assert not bad, "%d of %d differ:\n%s" % (len(bad), len(rejects), "\n".join(bad[:10]))


def test_the_launcher_enters_the_device_guard_only_for_another_device(monkeypatch):
    """ops._launch, the one place a call through the C ABI is made: the stream of the arrays' device is appended, the return code is
    checked, and the device guard is entered -- and left, whatever the call answers -- only when that device is not the current
    one.  (The GPU suite runs the second branch only on a machine with two devices.)"""
    import torch
    events = []

    class Guard:
        def __init__(self, index):
            events.append(("guard", index))

        def __enter__(self):
            events.append("enter")

        def __exit__(self, *exc):
            events.append("exit")

    def call(*args):
        events.append(args)
        return 0

    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", Guard)
    monkeypatch.setattr(T.ops, "_stream", lambda index: ("stream", index))
    T.ops._launch(torch.device("cuda:0"), call, 1, 2)
    assert events == [(1, 2, ("stream", 0))]
    del events[:]
    T.ops._launch(torch.device("cuda:1"), call, 3)
    assert events == [("guard", 1), "enter", (3, ("stream", 1)), "exit"]
    for device, want in ((torch.device("cuda:0"), []), (torch.device("cuda:1"), [("guard", 1), "enter", "exit"])):
        del events[:]
        with pytest.raises(ValueError, match="sfm_pyramid_variant"):
            T.ops._launch(device, lambda stream: T._lib.lib.sfm_pyramid_variant(7))
        assert events == want
