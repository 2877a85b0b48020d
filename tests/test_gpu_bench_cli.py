"""-m gpu: the command line of bench.py — a plain run prints the headline alone, --full adds what takes runs of its own, and
--dump-outputs writes what the last timed step computed, the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "64", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_every_time(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(a))
    assert all(k in d for k in HEADLINE) and d["steps"] == 3 and d["warmup"] == 2 and d["config"]["graph"]
    assert d["value"] == pytest.approx(1.0 / (d["ms_per_step"] * 1e-3))
    assert not any(k in d for k in ("roofline", "secondary", "cpu_baseline")), sorted(d)
    _bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(b))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"loss.npy", "logits.npy", "params.npy", "grads.npy", "param_stats.npy", "grad_stats.npy"} <= set(names), names
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
    assert float(np.load(a / "loss.npy")[0]) == pytest.approx(d["config"]["final_loss"])


def test_full_run_adds_the_roofline_and_the_cpu_baseline():
    d = _bench("--steps", "2", "--warmup", "1", "--full", "--cpu-size", "32")
    assert all(k in d for k in HEADLINE) and d["steps"] == 2
    assert d["roofline"]["kernel"].startswith(("k_conv3_rw", "k_wgrad_r32")) and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] in ("port", "reference")
