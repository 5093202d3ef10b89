"""The host side of the fused loss decides, per descriptor and entry point, the work decomposition and WHICH kernel family runs at
how many waves per SIMD.  Families compute the same bits (the three-waves-per-SIMD build of the small L1 launches differs from the
four-wave build in speed only), so nothing but this table notices a launch that silently changes family.
tests/golden/plan_table.npz pins those decisions for a fixed grid of descriptors (tests/golden/make_plan_table.py); here the rows
are recomputed by the library as built and compared integer for integer.  Nothing is launched, no GPU is needed."""
import importlib.util
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_plan_table", os.path.join(GOLD, "make_plan_table.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

TUNING = [k for k in os.environ if k.startswith("SFM_")]      # (read once per process by the library: cannot be unset here)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "plan_table.npz"))


@pytest.fixture(scope="module")
def now():
    assert not TUNING, "the plan table holds for a library without tuning overrides; unset %s" % TUNING
    return T.tables()


def _entry_cols(rows):
    return rows.reshape(len(rows), len(T.ENTRIES), T.ENTRY_COLS)


def test_the_grid_is_the_fixtures(gold, now):
    assert gold["params"].shape == now["params"].shape and (gold["params"] == now["params"]).all()
    assert len(now["params"]) >= 15552
    assert list(gold["rejected"]) == list(now["rejected"])


def test_every_plan_is_the_pinned_one(gold, now):
    assert gold["rows"].shape == now["rows"].shape
    bad = np.flatnonzero((gold["rows"] != now["rows"]).any(axis=1) | (gold["workspace_bytes"] != now["workspace_bytes"]))
    if len(bad):
        k = int(bad[0])
        names = ["workspace"] + ["%s.%s" % (e, c) for e in ("fwd", "bwd", "fwd_bwd")
                                 for c in ["rc", "items"] + ["s%d.%s" % (s, f) for s in range(T.MAX_S) for f in ("strips", "chunks", "rows", "tiles")]
                                 + ["family", "waves_per_simd"]]
        want = [int(gold["workspace_bytes"][k])] + [int(v) for v in gold["rows"][k]]
        got = [int(now["workspace_bytes"][k])] + [int(v) for v in now["rows"][k]]
        diff = ["%s: pinned %d, now %d" % (n, w, g) for n, w, g in zip(names, want, got) if w != g]
        pytest.fail("%d of %d descriptors differ; the first: %s -- %s" % (len(bad), len(gold["rows"]), T.describe(gold["params"][k]), "; ".join(diff)))


def test_rejected_descriptors_return_the_pinned_codes(gold, now):
    for what, want, got in zip(gold["rejected"], gold["rejected_codes"], now["rejected_codes"]):
        assert want < 0 and got == want, (str(what), int(want), int(got))


def test_the_fixture_exercises_every_family(gold):
    """A table that no longer reaches a family would pin nothing about it."""
    e = _entry_cols(gold["rows"])
    assert (e[:, :, 0] == 0).all(), "every descriptor of the grid is accepted"
    assert (gold["workspace_bytes"] > 0).all()
    family, waves = e[:, :, -2], e[:, :, -1]
    assert sorted(set(family.ravel())) == list(range(len(T.FAMILIES)))
    grad = np.array([g for g, _ in T.ENTRIES], bool)
    gf, gw = family[:, grad], waves[:, grad]
    for name, sel in (("wide", gf == 1), ("pair", gf == 2), ("four-wave base", (gf == 0) & (gw == 4)), ("three-wave base", (gf == 0) & (gw == 3))):
        assert sel.any(), "no gradient launch of the table runs the %s kernels" % name
    assert (gw[gf == 1] == 3).all() and (gw[gf == 2] == 2).all()
    assert (family[:, ~grad] != 1).all() and (family[:, ~grad] != 2).all() and (family[:, ~grad] != 4).all()      # gradient-only families
