"""bench.py as a command: a plain run measures the headline figure alone; --full adds the roofline and the CPU baseline.
Every run is a fresh child process (bench.py initialises the GPU itself)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _bench(*argv, timeout=300):
    return subprocess.run([sys.executable, BENCH, *argv], cwd=REPO, capture_output=True, text=True, timeout=timeout)


def _line(proc):
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


def test_shape_table_needs_full(tmp_path):
    table = tmp_path / "t.shapes"
    proc = _bench("--shape-table", str(table), timeout=120)
    assert proc.returncode == 2 and "--full" in proc.stderr, proc.stderr
    assert not table.exists()


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_full_adds_the_rest(tmp_path):
    common = ("--workload", "dit_s4", "--batch", "32", "--steps", "2", "--warmup", "1")
    plain = _line(_bench(*common, "--dump-outputs", str(tmp_path / "dump")))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain
    assert plain["metric"] == "training images/sec" and plain["unit"] == "images/sec" and plain["dtype"] == "bf16"
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert "roofline" not in plain and "cpu_baseline" not in plain
    assert sorted(os.listdir(tmp_path / "dump")) == ["ema_weights_sample.npy", "loss.npy", "mse.npy", "weights_sample.npy"]

    table = tmp_path / "t.shapes"
    full = _line(_bench(*common, "--full", "--shape-table", str(table)))
    assert full["roofline"]["launches_per_step"] > 0 and full["roofline"]["achieved"] > 0
    assert full["cpu_baseline"]["value"] > 0
    assert table.stat().st_size > 0
