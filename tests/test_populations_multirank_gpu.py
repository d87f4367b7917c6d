"""``populations`` over two ranks on the GPU box (one MI355X): two rank processes share cuda:0 over gloo, started like
the ranks of tests/test_multirank_gpu.py.  2 ranks x 2 populations x 64 walkers must equal the 1-rank 4-population run --
bitwise in the not-debiased regime; resampling counts, ``resampled`` and ``log_z`` in the debiased one -- and a rank
issues no collective per step or per event: none of ``_Comm.shared_uniform`` / ``exchange_rows``, and only the
end-of-run ``all_gather`` calls (tools/rehearse_populations.py counts them)."""
import os
import re
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return env


def test_two_ranks_reproduce_one_rank_without_per_step_collectives():
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(ROOT, "tools", "rehearse_populations.py")],
                       capture_output=True, text=True, timeout=600, env=_env())
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("populations debias=")]
    assert len(lines) == 8 and all("DIFFERENT" not in ln for ln in lines), r.stdout
    for ln in lines:
        assert "counts equal" in ln and "resampled equal" in ln and "n_unique equal" in ln and "log_z equal" in ln, ln
        assert "shared_uniform" not in ln and "exchange_rows" not in ln, ln
        gathers = int(re.search(r"'all_gather': (\d+)", ln).group(1))
        if ln.startswith("populations debias=False"):
            assert "x bitwise" in ln and "logw bitwise" in ln, ln
            assert gathers == 3 + int("resample_at_end" in ln), ln  # walkers, event log, term moments (+ the end weights)
        else:
            assert gathers == 5, ln  # walkers, event log, two moment buffers, the stacked log-weights
