"""bench.py on one GPU: a plain run reports the headline and nothing that needs work of its own; --full adds the update
accountings, the stress sub-record and the host-pointer pass.  Both test the same map: their dumped results are identical."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = ["--grid", "64", "--frames", "2", "--steps", "2", "--warmup", "1", "--update-repeats", "2", "--stress", "96", "--cpu-sample", "0"]
FULL_ONLY = ("update_ms_per_frame", "update_ms_per_frame_synchronous", "update_ms_per_frame_with_inverse", "update_phases_ms",
             "deferred_inverse_ms", "update_roofline", "value_host_api", "stress", "cpu_baseline")


def _bench(tmp_path, name, extra):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out)] + SMALL + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return line, np.load(out / "test_result.npy"), np.load(out / "query_index.npy")


def test_plain_run_reports_the_headline_and_full_adds_the_rest(tmp_path):
    plain, res_p, idx_p = _bench(tmp_path, "plain", [])
    full, res_f, idx_f = _bench(tmp_path, "full", ["--full"])
    for d in (plain, full):
        assert d["metric"] == "sdf_test_points_per_sec" and d["unit"] == "points/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["steps"] == 2 and d["warmup"] == 1
        assert d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 64 ** 3) < 1e-6 * 64 ** 3
        assert d["roofline"]["k4_ms_per_step"] > 0
    assert plain["full"] is False and full["full"] is True
    assert not [k for k in FULL_ONLY if k in plain], [k for k in FULL_ONLY if k in plain]
    assert all(k in full for k in FULL_ONLY)
    assert full["update_repeats"] == 2 and full["value_host_api"] > 0
    assert full["stress"]["finite"] and full["stress"]["clusters"] == 96
    # one fusion (plain) and the last of 2 x 2 fusions (--full) give the same map and the same results, bit for bit
    assert plain["config"] == full["config"] and plain["gp_evals_per_point"] == full["gp_evals_per_point"]
    assert np.array_equal(idx_p, idx_f)
    assert res_p.shape == (64 ** 3, 8) and np.array_equal(res_p.view(np.uint32), res_f.view(np.uint32))
