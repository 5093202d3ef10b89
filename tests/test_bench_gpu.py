"""A plain `python bench.py --gpus 1 --steps K --warmup W` measures the headline alone: exactly K timed steps, no secondary keys, no
CPU baseline.  `--dump-outputs DIR` writes what the last timed step computed, and two runs with the same arguments compute the same."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args),
                       capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_plain_run_times_k_steps_and_dumps_its_outputs(dev, tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    lines = [_run("--steps", "7", "--warmup", "3", "--dump-outputs", str(d)) for d in dirs]
    d = lines[0]
    assert d["steps"] == 7 and d["timing"]["timed_steps"] == 7 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["warped_px_per_gpu_step"] / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"] + 0.1
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    for key in ("cpu_baseline", "cfg3", "other_layout", "graph_ms_per_step", "cfg3_d_src"):      # measured with --full only
        assert key not in d, key
    assert d["pre_warm_ms_per_step"] is None
    B, n_src, n_scales = d["config"]["per_gpu_batch"], d["config"]["n_src"], d["config"]["n_scales"]
    names = ["loss5"] + ["d_disp_s%d" % s for s in range(n_scales)] + ["d_pose_%d" % i for i in range(n_src)]
    assert sorted(p.name for p in dirs[0].iterdir()) == sorted(n + ".npy" for n in names)
    got = [{n: np.load(str(dd / (n + ".npy"))) for n in names} for dd in dirs]
    for n in names:
        assert got[0][n].dtype == np.float32 and np.isfinite(got[0][n]).all(), n
    assert got[0]["loss5"].shape == (5,) and got[0]["d_pose_0"].shape == (B, 6)
    assert got[0]["d_disp_s0"].shape == (B, 1, d["config"]["H"], d["config"]["W"])
    np.testing.assert_allclose(got[0]["loss5"], d["loss5"], rtol=1e-5, atol=1e-6)      # the line's scalars are the dumped step's
    # the same arguments, the same inputs: the second run computes what the first did (to the order of float atomics)
    for n in names:
        np.testing.assert_allclose(got[1][n], got[0][n], rtol=0, atol=1e-5 * max(float(np.abs(got[0][n]).max()), 1e-30), err_msg=n)
