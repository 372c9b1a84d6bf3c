"""Data parallelism of ppsci.arch.FNO1d: a world-2 gloo run gives the 1-rank gradient on the same global batch (batch data
parallelism like FNO / LNO, dp_reduce = "mean").  Launched the way tests/test_distributed.py:_run launches its worker; the workers
run the kernels under the CPU SIMT emulator."""
import os
import subprocess
import sys

import numpy as np

from tests.common import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_give_the_single_rank_gradient(tmp_path):
    from tests.test_distributed import _free_port

    worker = os.path.join(ROOT, "tests", "geofno_dp_worker.py")
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    out = str(tmp_path)
    subprocess.run([sys.executable, worker, out], check=True, env=env, cwd=ROOT, timeout=600, stdout=subprocess.DEVNULL)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                    "--master-port", _free_port(), worker, out], check=True, env=env, cwd=ROOT, timeout=600,
                   stdout=subprocess.DEVNULL)
    one, two = np.load(os.path.join(out, "geofno_w1.npz")), np.load(os.path.join(out, "geofno_w2.npz"))
    e = rel(two["grad"], one["grad"])
    print(f"two ranks vs one: {e:.2e}")
    assert e <= 5e-5
