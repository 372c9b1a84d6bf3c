"""PCGrad under data parallelism: every rank fills its [K, P] per-loss gradient matrix from its shard, ONE all-reduce (sum) of
the whole matrix per step, then the same surgery on every rank -- so a 2-rank run reproduces the 1-rank run on the concatenated
batch.  Gloo, world_size 2, kernels under the CPU SIMT emulator (the style and the tolerance of tests/test_distributed.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> str:
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


def _run(outdir, world, kind, dp_reduce="sum"):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    worker = os.path.join(ROOT, "tests", "mtl_dp_worker.py")
    if world == 1:
        cmd = [sys.executable, worker, outdir, kind, dp_reduce]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", _free_port(), worker, outdir, kind, dp_reduce]
    subprocess.run(cmd, check=True, env=env, cwd=ROOT, timeout=600, stdout=subprocess.DEVNULL)
    return [np.load(os.path.join(outdir, f"result_w{world}_r{r}.npz")) for r in range(world)]


def test_pcgrad_two_ranks_reproduce_single_rank(tmp_path):
    """The two ranks' numpy generators are in different states (tests/mtl_dp_worker.py): both apply rank 0's projection orders,
    so their parameter copies stay identical, and equal the one-rank run seeded like rank 0."""
    (one,) = _run(str(tmp_path), 1, "pcgrad")
    two, two_r1 = _run(str(tmp_path), 2, "pcgrad")
    np.testing.assert_array_equal(two["params"], two_r1["params"])  # the ranks train ONE model
    np.testing.assert_allclose(two["params"], one["params"], rtol=0, atol=2e-6)
    assert np.abs(one["params"]).max() > 0 and np.isfinite(two["loss"])
    # one collective per step, and it carries the whole matrix (rows padded to 16 bytes) with its slots
    K, P = two["G"].shape
    assert K == 3 and int(two["buf"]) >= K * P + 3 * K + 1
    assert list(two["allreduce"]) == [int(two["buf"])] * 4 and len(one["allreduce"]) == 0
    # the rows conflict (otherwise the surgery would be the plain sum and this test would say nothing about it)
    gram = two["G"].astype(np.float64) @ two["G"].astype(np.float64).T
    assert (gram[np.triu_indices(K, 1)] < 0).any()


@pytest.mark.parametrize("dp_reduce", ["sum", "mean"])
def test_relobralo_two_ranks_reproduce_single_rank(tmp_path, dp_reduce):
    """beta = 0.5: rho is a real coin flip, drawn from generators in different states on the two ranks; the loss values travel in
    the slots of the one all-reduce.  dp_reduce = "mean" trains on 1 / world of the summed loss: lmbda is a function of loss
    RATIOS (up to eps = 1e-8 next to losses of 1e-1 .. 1), so it is compared with the same one-rank run, and the logged total is
    half of it."""
    (one,) = _run(str(tmp_path), 1, "relobralo")
    two, two_r1 = _run(str(tmp_path), 2, "relobralo", dp_reduce)
    np.testing.assert_array_equal(two["params"], two_r1["params"])
    np.testing.assert_array_equal(two["lmbda"], two_r1["lmbda"])
    assert list(two["allreduce"]) == [int(two["buf"])] * 4  # still ONE collective per step
    np.testing.assert_allclose(two["lmbda"], one["lmbda"], rtol=2e-4)
    assert np.abs(two["lmbda"] - 1).max() > 1e-3
    if dp_reduce == "sum":
        np.testing.assert_allclose(two["params"], one["params"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(two["loss"], one["loss"], rtol=1e-5)
    else:
        np.testing.assert_allclose(two["loss"], 0.5 * one["loss"], rtol=2e-4)
