"""Every operator entry point of include/sfmwarp.h validates its arguments before any HIP call, so what it answers to a bad call --
return code, message text, and WHICH check fires when several apply -- can be pinned without a GPU.  tests/golden/ops_rejects.json
holds those answers for each NULL argument, each shape bound at its edge and one past it, calls with two faults at once, and the
accepted calls that return before a launch (tests/golden/make_ops_rejects.py wrote it and refuses any row that would launch).
Here the table is replayed against the library as built and compared exactly."""
import importlib.util
import json
import os

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ops_rejects", os.path.join(GOLD, "make_ops_rejects.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "ops_rejects.json")) as f:
        return json.load(f)


def test_the_cases_are_the_fixtures(gold):
    assert [r[:2] for r in gold] == [[name, args] for name, args in T.cases()]


def test_the_fixture_covers_every_operator_entry_point(gold):
    """ENTRIES (what the table holds) and PINNED_ELSEWHERE (pinned by the CPU tests of their own feature) are together every
    operator symbol of the binding: a new entry point lands in one of the two, or this fails"""
    operators = {n for n in T._lib.SYMBOLS if not n.startswith(("sfm_loss_", "sfm_step_")) and n not in ("sfm_abi_version", "sfm_last_error")}
    assert set(T.ENTRIES) | set(T.PINNED_ELSEWHERE) == operators and not set(T.ENTRIES) & set(T.PINNED_ELSEWHERE)
    assert T.ENTRIES == sorted({r[0] for r in gold})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, path in T.PINNED_ELSEWHERE.items():
        assert os.path.isfile(os.path.join(root, path)), path
        with open(os.path.join(root, path)) as f:
            assert name in f.read(), (name, path)
    for name in T.ENTRIES:
        codes = [r[2] for r in gold if r[0] == name]
        assert codes, name
        if name == "sfm_warp_pyramid_bwd_workspace_bytes":      # (a size: 0 with a message for a descriptor the backward refuses)
            assert 0 in codes and max(codes) >= 256
        elif name != "sfm_warp_bwd_workspace_bytes":              # (a size, not a code: it cannot reject)
            assert min(codes) < 0 and 0 in codes, (name, "needs a rejected and an accepted call")
    texts = {r[3] for r in gold if r[2] == 0 and r[0] not in T.SIZES}
    assert len(texts) == 1, "an accepted call leaves the message alone: the sentinel"
    assert texts == {r[3] for r in gold if r[0] in T.SIZES and r[2] > 0}, "and so does an answered size"


def test_no_row_would_launch(gold):
    for name, args, rc, _ in gold:
        assert not T.would_launch(name, args) and (rc <= 0 or name in T.SIZES), (name, args, rc)


def test_every_call_answers_as_pinned(gold):
    bad = []
    for name, args, rc, text in gold:
        got = T.call(name, args)
        if got != (rc, text):
            bad.append("%s%r: pinned %d %r, now %d %r" % (name, tuple(args), rc, text, got[0], got[1]))
    assert not bad, "%d of %d rows differ:\n%s" % (len(bad), len(gold), "\n".join(bad[:10]))
