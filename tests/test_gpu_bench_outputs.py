"""bench.py's plain run and --dump-outputs: the line carries the headline
figures and none of the --full line items, --steps sets the number of timed
frames, and the dumped frame is the reference's own image of the workload
(tests/golden/manifest.json sha256_rgb), so two builds can be compared output
for output."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO, manifest

WORKLOAD = "medium_1920x1080_d2"


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_frame(tmp_path):
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup",
                          "1", "--frames-per-launch", "2", "--workload", WORKLOAD, "--dump-outputs",
                          str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=150, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 5 and line["config"]["launch_frames"] == [2, 2, 1]  # --steps frames were timed
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region: equal up to the line's rounding
    # (ms_per_step to 1e-4 ms, value to 1e-2 Mrays/s)
    rate = line["config"]["rays_per_frame"] / line["ms_per_step"] / 1e3
    tol = 0.5e-4 / line["ms_per_step"] + 0.5e-2 / line["value"] + 1e-5
    assert abs(rate - line["value"]) <= tol * line["value"]
    # a plain run measures nothing else
    for k in ("cpu_baseline", "cpu_baseline_all_cores", "e2e", "single_frame", "moving_camera"):
        assert k not in line
    assert line["also"] == {} and line["config"]["golden_check"] is None

    m = manifest()[WORKLOAD]
    frame = np.load(tmp_path / "dump" / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (m["height"], m["width"], 3)
    assert hashlib.sha256(frame.astype(np.uint8).tobytes()).hexdigest() == m["sha256_rgb"]
    rays = np.load(tmp_path / "dump" / "ray_counts.npy")
    assert rays.dtype == np.float64 and rays.shape == (3,)
    # the last timed launch held one frame: its counts are one frame's
    assert int(rays.sum()) == line["config"]["rays_per_frame"]
    assert [int(x) for x in rays] == [m["rays"][k] for k in ("primary", "shadow", "reflect")]
