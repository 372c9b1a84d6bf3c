"""The device-only halves of tests/test_fpde.py: the fPINN step at N = 2000 (1.38 M auxiliary points) and the example's
training run.  No emulator variant: both are sized for the MI355X."""
import numpy as np
import pytest

from tests.test_fpde import _check_step, _example


@pytest.fixture(autouse=True)
def dev():
    from paddlescience_amd import _lib, device

    _lib._inject_for_tests(None)
    device.set_device(None)
    yield "gpu"


@pytest.mark.gpu
def test_fpde_step_at_2000_points(dev, tmp_path, monkeypatch):
    """N = 2000: 1.38 M auxiliary points (dense, M would need 11 GB): the step runs, matches float64 sparse autograd, and two
    steps from the same state give bitwise the same loss and gradient."""
    ex, cfg, solver = _example(tmp_path, NPOINT_INTERIOR=2000, epochs=1)
    eq = solver.equation["fpde"]
    assert len(eq.train_x["x"]) > 1_300_000
    cc, loss, grad = _check_step(solver, eq, 2000, monkeypatch, ref_device="cuda")
    solver.engine.forward_backward([cc.fused])
    assert cc.fused.losses()["fpde"] == loss
    assert np.array_equal(solver.engine.grad.detach().cpu().numpy().astype(np.float64), grad)


# ---- the example ---------------------------------------------------------------------------------------------------------
EXAMPLE_EPOCHS = 1000  # (chosen on the first device run: see DESIGN.md section 4.4)


@pytest.mark.gpu
def test_example_trains(dev, tmp_path):
    ex, cfg, solver = _example(tmp_path, epochs=EXAMPLE_EPOCHS)
    _, first = solver.eval()
    solver.train()
    _, last = solver.eval()
    l0, l1 = first["L2Rel_Metric"]["L2Rel.u"], last["L2Rel_Metric"]["L2Rel.u"]
    assert l1 < l0 / 10, (l0, l1)
