"""bench.py without --full: it stages the scene, warms up, times its steps and prints the headline line -- none of the sections
that take runs of their own (points of view, CPU baseline, config 3, the reference's layout, counter passes, the tile-split bound)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("povs", "cpu_baseline", "config3", "reference_layout", "seating_without_viewpoint", "ms_per_step_seating_without_viewpoint", "flatten_build_s", "tile_split_bound")
FULL_ONLY_ROOFLINE = ("stages", "measured_stream_read_gbps", "binding", "counters", "traffic_detail", "pmc_errors")


def test_a_plain_bench_run_prints_the_headline_and_nothing_it_does_not_need(grt):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["metric"].startswith("Mrays/s")
    assert out["steps"] == 6 and out["warmup"] == 2 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # the headline counts the closest-hit rays of the 6 timed samples over their wall time
    assert out["config"]["rays_per_step"] > 1920 * 1080
    assert abs(out["value"] - out["config"]["rays_per_step"] / out["ms_per_step"] / 1e3) <= 0.01 * out["value"]
    assert not [key for key in FULL_ONLY if key in out], sorted(out)
    assert not [key for key in FULL_ONLY_ROOFLINE if key in out["roofline"]], sorted(out["roofline"])
    assert out["roofline"]["launches"] > 0   # from the per-launch events of the timed region itself
