"""bench.py's plain run (-m gpu): the result line carries the headline figure and nothing measured behind the timed region, and
--dump-outputs writes what the last timed step returned, equal to the same call on the same seeded pair."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import cloud

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path):
    n = 20000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--points", str(n),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "query-points/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 2 * n / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for key in ("device_ms_per_step", "end_to_end_numpy", "cpu_baseline", "parity", "configs"):
        assert key not in d, key                                      # --full only
    assert sorted(os.listdir(tmp_path / "out")) == ["chamfer.npy"]
    got = np.load(tmp_path / "out" / "chamfer.npy")
    assert got.dtype == np.float32 and got.shape == ()
    import point_cloud_utils_amd as pcu
    ch = pcu.chamfer_distance(cloud(1000, n, np.float32), cloud(1001, n, np.float32))     # bench.py's rank-0 pair
    assert got == ch and float(got) == d["chamfer"]
