"""bench.py on one GPU: a plain run prints the headline line only and, with --dump-outputs, the same fields from the same
seeded inputs every time; --full adds the per-kernel times, the roofline and the CPU baselines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    # 360x180x36 = 2.33 M cells: every 3-D field is sampled (2 M points of 4 bytes), eta is written whole
    lines = [_bench("--steps", "3", "--warmup", "1", "--size", "360", "180", "36", "--dump-outputs", str(tmp_path / d))
             for d in ("a", "b")]
    for out in lines:
        assert out["steps"] == 3 and out["warmup"] == 1 and out["finite"]
        assert (out["metric"], out["unit"], out["higher_is_better"], out["dtype"]) == ("model time-steps/sec", "steps/s", True, "f32")
        assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-6
        assert not {"roofline", "kernels_ms_per_launch", "cpu_baseline", "cpu_baseline_config1"} & set(out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["S.npy", "T.npy", "eta.npy", "u.npy", "v.npy", "w.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), n
        total += a.nbytes
    assert np.load(tmp_path / "a" / "eta.npy").shape[:2] == (360, 180)
    assert np.load(tmp_path / "a" / "u.npy").shape == ((8 << 20) // 4,)
    assert total <= 64 << 20


def test_full_run_adds_kernel_times_roofline_and_cpu_baselines():
    out = _bench("--steps", "3", "--warmup", "1", "--size", "128", "64", "8", "--full")
    assert out["steps"] == 3 and out["finite"] and out["value"] > 0
    assert out["kernels_ms_per_launch"] and out["roofline"]["bound"] == "hbm" and out["roofline"]["achieved"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline_config1"]["value"] > 0
