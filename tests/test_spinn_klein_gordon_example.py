"""examples/spinn_klein_gordon.py trains through Solver at a tiny size: a general PDE constraint (u^2), five Dirichlet faces on the
four-coefficient kernels and an initial-velocity face (u_t) in one Solver, then predict(expr_dict=...) on the test grid."""
import os
import runpy
import sys

from tests.common import make_dev_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = make_dev_fixture()


def test_klein_gordon_example_runs(dev, tmp_path, monkeypatch):
    args = ["epochs=1", "iters_per_epoch=3", "nc=6", "nc_test=5", "r=4", "num_layers=2", "hidden_size=16", "log_freq=1",
            "resample_every=2", f"output_dir={tmp_path}/out"]
    monkeypatch.setattr(sys, "argv", ["spinn_klein_gordon.py"] + args)
    runpy.run_path(os.path.join(ROOT, "examples", "spinn_klein_gordon.py"), run_name="__main__")
    log = open(os.path.join(str(tmp_path), "out", "train.log")).read()
    assert "IC_t" in log and "residual rms" in log
