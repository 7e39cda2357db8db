"""The benchmark's command line: a plain run times exactly ``--steps`` steps
and prints the rate alone; ``--dump-outputs`` writes what the last timed step
computed.  One small run (c3_small: the c3 geometry at 4M rows) in a process
of its own, as the benchmark is run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c3_small",
                          "--steps", "5", "--warmup", "2", "--dump-outputs", str(out)],
                         capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["unit"] == "Lloyd it/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 5 and line["steps_ran"] == 5 and line["warmup"] == 2
    assert line["ms_per_step"] > 0.0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-12)
    # what --full measures is not in a plain line
    for key in ("roofline", "kernel_avg_ms", "first_iter", "cpu_baseline"):
        assert key not in line

    n, d, k = line["config"]["N"], line["config"]["d"], line["config"]["k"]
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["centroids", "cluster_sizes", "labels", "max_shift"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["centroids"].shape == (k, d) and np.all(np.isfinite(got["centroids"]))
    assert got["cluster_sizes"].shape == (k,) and got["cluster_sizes"].sum() == n
    assert got["max_shift"].shape == (1,) and got["max_shift"][0] >= 0.0
    lab = got["labels"]
    assert 0 < len(lab) <= n and np.all(lab == np.floor(lab)) and lab.min() >= 0 and lab.max() < k
