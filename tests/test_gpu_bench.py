"""-m gpu: the plain benchmark run (`bench.py --gpus 1 --steps K --warmup W`): the contract's keys on its line, value and
ms_per_step of the same K steps, nothing of --full, and --dump-outputs writing the same arrays in two runs with the same
arguments (seeded inputs, in-kernel Philox jitter from fixed seeds, fixed-order reductions)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--dump-outputs", out_dir], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_plain_bench_run_reports_its_steps_and_dumps_reproducible_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _plain_run(a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 5 and line["warmup"] == 2 and line["higher_is_better"] is True
    assert abs(line["value"] - 8 * 512 * 128 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-6
    for k in ("ms_per_step_windows", "sclk_mhz", "kernels_us", "roofline", "aux_hash", "cpu_baseline"):
        assert k not in line, k
    _plain_run(b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"loss_combined.npy", "prediction_rgbds.npy", "param__linears_0_weight.npy"} <= set(names)
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 << 20
    assert np.isfinite(np.load(os.path.join(a, "loss_combined.npy")))
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, y), n
