"""bench.py on one GPU: the plain run's result line and --dump-outputs (the walkers of the timed steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "3",
                        "--walkers", "1024", *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_and_dumped_walkers(tmp_path):
    """A plain run times the headline steps only (no secondary leg in its line); its dumped walkers are the same, bit for
    bit, in a second run and in a --full run, whose legs in front of the timed region must not change them."""
    out = _bench("--dump-outputs", str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 6 and out["warmup"] == 3 and out["value"] > 0 and out["higher_is_better"] is True
    assert out["ms_per_step"] == pytest.approx(1024 * 1e3 / out["value"], rel=1e-9)
    assert out["roofline_force"] is None and out["cpu_baseline"] is None
    assert not any(k in out for k in ("debiased", "e2e", "small_batch"))
    a = np.load(tmp_path / "a" / "walkers.npy")
    assert a.dtype == np.float32 and a.shape == (1024, 39) and np.isfinite(a).all()
    _bench("--dump-outputs", str(tmp_path / "b"))
    full = _bench("--full", "--no-cpu-baseline", "--no-e2e", "--no-small-batch", "--force-evals", "4",
                  "--dump-outputs", str(tmp_path / "c"))
    assert full["debiased"]["value"] > 0 and full["roofline_force"]["walkers"] == 1024
    for other in ("b", "c"):
        assert np.array_equal(a, np.load(tmp_path / other / "walkers.npy")), other
