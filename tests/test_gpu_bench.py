"""GPU: what a plain bench.py run does against a --full one.  A plain run sets up, warms up, times its steps, dumps and prints
the line; everything else it measures or checks (sustained, roofline, entry points, f-rows, cpu_baseline and parity, other
workloads) runs only under --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--gaussians", "100000", "--views", "4", "--resolution", "640x360"]


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_nothing_else(hip_device, tmp_path):
    line = _bench(["--dump-outputs", str(tmp_path / "dump")])
    assert line["metric"] and line["unit"] == "views/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    # views/s of the timed steps: 4 views per step
    assert abs(line["value"] - 4 / (line["ms_per_step"] * 1e-3)) <= 1e-2 * line["value"]
    for key in ("sustained", "roofline", "parity", "entry_points", "other_workloads", "f_rows", "cpu_baseline"):
        assert line[key] is None, key
    assert line["dumped_outputs"]["files"] > 0
    g = np.load(tmp_path / "dump" / "grad_means3D.npy")
    assert g.shape == (100_000, 3) and np.abs(g).max() > 0


def test_full_run_goes_on_after_the_timed_steps(hip_device):
    line = _bench(["--full", "--no-cpu-baseline", "--no-extras", "--no-live-pmc", "--sustain-seconds", "0.2"])
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["sustained"]["steps"] >= 2 and line["sustained"]["views_per_s"] > 0
    assert line["roofline"]["launches"] > 0 and line["roofline"]["kernel"]
    assert line["cpu_baseline"] is None and line["entry_points"] is None
