"""No GPU needed: the table of entry points tests/test_buffer_contracts_gpu.py covers, held against the prototypes of
include/sfmwarp.h, and the arena helper itself (util.Arena) on a host tensor."""
import ast
import os
import re

import numpy as np
import pytest
import torch

import abi_header
import test_buffer_contracts_gpu as T
from util import SENTINEL, Arena



def takes_a_device_pointer(params):
    """a float / void pointer or a descriptor (which binds device pointers); `const char *` and friends do not count"""
    return bool(re.search(r"\b(float|void)\b[^,]*\*", params)) or bool(re.search(r"\bSfm(Loss|WarpPyramid|PhotoError)Desc\b", params))


def defined_tests(module="test_buffer_contracts_gpu.py"):
    """the ids ("name", or "file.py::name" for another module) of the test functions a GPU test module defines, read from its source:
    importing some of them touches the device"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), module)) as f:
        tree = ast.parse(f.read())
    prefix = "" if module == "test_buffer_contracts_gpu.py" else module + "::"
    return {prefix + node.name for node in tree.body if isinstance(node, ast.FunctionDef) and node.name.startswith("test_")}


def test_every_entry_point_with_a_device_pointer_is_covered():
    protos = abi_header.prototypes()
    assert len(protos) >= 30 and "sfm_loss_fwd_bwd" in protos and "sfm_scale_arrays" in protos, sorted(protos)
    need = {n for n, p in protos.items() if takes_a_device_pointer(p)}
    # read the descriptor's integers on the host, launch nothing
    host_only = {"sfm_loss_workspace_bytes", "sfm_loss_plan_info", "sfm_warp_pyramid_bwd_workspace_bytes"}
    assert host_only <= need
    need -= host_only
    assert T.EXEMPT <= need, "an exempt name is not (or no longer) an entry point with a pointer argument"
    assert set(T.COVERED) == need - T.EXEMPT, (sorted(need - T.EXEMPT - set(T.COVERED)), sorted(set(T.COVERED) - need))
    assert not (set(T.COVERED) & T.EXEMPT)
    for name, test in T.COVERED.items():
        assert test in defined_tests(*test.split("::")[:-1]), (name, test)
    # the operator cases are named test ids: every operator entry point of the table appears in them
    short = {i.split("-")[0] for i in T.OP_IDS}
    for name in T.COVERED:
        if T.COVERED[name] == "test_op_guards_and_inputs":
            assert name[len("sfm_"):].replace("_fwd", "").replace("resize", "resize") in {s.replace("_fwd", "") for s in short} or \
                name[len("sfm_"):] in short, name


def test_fused_case_list_covers_what_it_must():
    cases = T.FUSED_CASES
    assert len(cases) >= 40
    for shape in ((1, 3, 3, 1, 1), (1, 5, 61, 2, 1), (9, 16, 24, 2, 2), (3, 33, 40, 8, 1), (2, 70, 36, 2, 2), (2, 37, 71, 3, 3), (4, 128, 416, 2, 4)):
        assert len({c.mode for c in cases if c.shape == shape}) >= 3, shape
        assert {c.layout for c in cases if c.shape == shape} == {"planar", "hwc"}, shape
    assert {c.inputs for c in cases} >= {"out_of_view", "behind"}
    assert {c.mode for c in cases} == set(T.MODES) and {c.variant for c in cases} == {0, 3, 4, 5}
    assert {c.dsrc for c in cases} == {"no", "all", "sub"} and {c.warped for c in cases} == {True, False}
    assert any(T.dsrc_flags(c)[:3] == [True, False, True] for c in cases)
    oracle = [c for c in cases if c.oracle]
    assert len(oracle) >= 6 and {c.mode for c in oracle} == set(T.MODES)
    assert {c.layout for c in oracle} == {"planar", "hwc"} and {c.proj for c in oracle} == {"fast", "reference_order"}
    assert any(c.step for c in cases)
    # sfm_loss_proj_bwd: the library's own kernel choice on the three small shapes, every mode, both layouts and projections, with and
    # without d_src, and behind sfm_step_fwd_bwd too
    proj = T.PROJ_CASES
    assert len(proj) == 12 and {c.shape for c in proj} == {(1, 3, 3, 1, 1), (1, 5, 61, 2, 1), (2, 37, 71, 3, 3)} and {c.variant for c in proj} == {0}
    assert {c.mode for c in proj} == set(T.MODES) and {c.layout for c in proj} == {"planar", "hwc"}
    assert {c.proj for c in proj} == {"fast", "reference_order"} and {c.dsrc for c in proj} == {"no", "all", "sub"}
    assert {e for c in proj for e in T.proj_entries_of(c)} == {("bwd", 0), ("fwd_bwd", 1), ("step_fwd_bwd", 1)}
    assert T.COVERED["sfm_loss_proj_bwd"] == "test_fused_proj_bwd_after_every_gradient_entry"


def test_arena_places_guards_and_names_the_damage():
    dev = torch.device("cpu")
    ar = Arena(dev, [("a", (3, 61), 4), ("b", (5,), 12), ("ws", 768, "ws"), ("c", (2, 2, 7), 8)], row_floats=2000)
    base = ar.words.data_ptr()
    assert ar.guard == 16128 and base % 256 == 0
    assert (ar.ptr("a") % 16, ar.ptr("b") % 16, ar.ptr("c") % 16, ar.ptr("ws") % 256) == (4, 12, 8, 0)
    spans = sorted((ar.ptr(n) - base, ar.ptr(n) - base + ar.nbytes(n)) for n in ("a", "b", "ws", "c"))
    assert spans[0][0] >= ar.guard and all(b[0] - a[1] >= ar.guard for a, b in zip(spans, spans[1:]))
    assert 4 * ar.words.numel() - spans[-1][1] >= ar.guard and ar.nbytes("ws") == 768
    assert np.isnan(ar.view("a").numpy()).all() and ar.view("a").shape == (3, 61)
    ar.check()
    ar.set("a", np.arange(183, dtype=np.float32))
    ar.snapshot("a")
    ar.unchanged("a")
    assert ar.sentinels_left("a") == 0 and ar.sentinels_left("b") == 5
    ar.check()                                          # writing INSIDE a buffer is no damage
    first, n = ar.where["b"][:2]
    ar.words[first + n + 2] = 0                         # the third word past the end of b
    with pytest.raises(AssertionError, match=r"b: 1 words written AFTER it, first at byte offset \+8 past its end"):
        ar.check("case")
    ar.words[first + n + 2] = SENTINEL
    ar.words[ar.where["ws"][0] - 1] = 7
    with pytest.raises(AssertionError, match=r"ws: 1 words written BEFORE it, nearest at byte offset -4"):
        ar.check()
    ar.words[ar.where["ws"][0] - 1] = SENTINEL
    ar.check()
    ar.view("a")[1, 2] = 5.0
    with pytest.raises(AssertionError, match="input 'a' was written"):
        ar.unchanged("a")
    ar.fill_bits("ws", 0xFFFFFFFF)
    assert (ar.bits("ws") == -1).all() and ar.sentinels_left("ws") == 0
