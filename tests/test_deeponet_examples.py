"""The DeepONets through the project's training interface (Solver, constraints, validators, datasets): multi-column branch
keys from the dataset to the executor, residuals on trunk-key derivatives, the errors of what the operator nets do not
carry, and examples/deeponet_antiderivative.py learning its operator."""
import os
import sys

import numpy as np
import pytest
import sympy as sp
import torch

import ppsci
from tests.common import make_dev_fixture, rel
from tests.test_deeponet import _exec, _loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = make_dev_fixture()


def _chip_solver(tmp_path, inputs, label, exprs):
    z, model, order, names, _ = _loaded("chip_swish")
    inp = {k: v.numpy() for k, v in inputs.items()}
    cfg = {"dataset": {"name": "IterableNamedArrayDataset", "input": inp, "label": label}}
    cst = ppsci.constraint.SupervisedConstraint(cfg, ppsci.loss.MSELoss("mean"), exprs, name="EQ")
    solver = ppsci.solver.Solver(model, {"EQ": cst}, str(tmp_path), ppsci.optimizer.Adam(1e-3)(model), epochs=1,
                                 iters_per_epoch=1)
    return z, model, solver


def test_residual_through_solver_matches_executor(dev, tmp_path):
    """ChipDeepONets: loss of hessian(T, x) + hessian(T, y) - label with [N, 12] / [N, 6] branch keys from the dataset; the
    loss term against the reference-run fixture's second-derivative streams, the gradient against the executor (itself
    pinned to the reference by tests/test_deeponet.py) driven with the same loss adjoint."""
    _, _, _, _, inputs = _loaded("chip_swish")
    n = int(inputs["x"].shape[0])
    x, y = sp.symbols("x y")
    T = sp.Function("T")(x, y)
    lab = np.random.default_rng(3).standard_normal((n, 1)).astype(np.float32)
    z, model, solver = _chip_solver(tmp_path, inputs, {"lap": lab}, {"lap": T.diff(x, 2) + T.diff(y, 2)})
    fused = solver._compiled["EQ"].fused
    solver.engine.forward_backward([fused])
    U = z["chip_swish/U"][0]  # value, T_x, T_y, T_xx, T_yy (float64, the reference's own autodiff)
    r = U[3] + U[4] - lab[:, 0]
    assert fused.losses()["lap"] == pytest.approx(float(np.mean(r * r)), rel=1e-4)
    ex, _ = _exec(model, 2, inputs)
    Uex = torch.zeros((ex.S, n), dtype=torch.float32, device=model.flat_params.device)
    ex.forward(model.flat_params, Uex)
    Ud = Uex.cpu().numpy().astype(np.float64)
    rd = Ud[3] + Ud[4] - lab[:, 0]
    Ubar = np.zeros((ex.S, n), np.float32)
    Ubar[3] = Ubar[4] = 2.0 * rd / n
    g = torch.zeros(model.n_params, dtype=torch.float32, device=Uex.device)
    ex.backward(model.flat_params, torch.as_tensor(Ubar).to(Uex.device), g)
    assert rel(solver.engine.grad.cpu().numpy(), g.cpu().numpy()) < 1e-4
    res = solver.predict({k: v.numpy() for k, v in inputs.items()}, {"lap": T.diff(x, 2) + T.diff(y, 2)}, batch_size=None,
                         return_numpy=True)
    assert rel(res["lap"][:, 0], U[3] + U[4]) < 1e-5
    before = model.flat_params.clone()
    solver.train()
    assert not torch.equal(before, model.flat_params)
    o_, k_ = model._offsets["branch_act.beta"]  # registered, never called: untouched by the optimizer
    assert torch.equal(before[o_:o_ + k_], model.flat_params[o_:o_ + k_])


def test_branch_key_errors(tmp_path):
    _, _, _, _, inputs = _loaded("chip_swish")
    n = int(inputs["x"].shape[0])
    lab = {"r": np.zeros((n, 1), np.float32)}
    with pytest.raises(NotImplementedError, match="branch key"):  # derivative along a branch key
        _chip_solver(tmp_path, inputs, lab, {"r": lambda out: ppsci.autodiff.jacobian(out["T"], out["bctype"])})
    with pytest.raises(NotImplementedError, match="branch key"):  # a 12-column key as a per-point value
        _chip_solver(tmp_path, inputs, lab, {"r": lambda out: out["T"] * out["u"]})


def _example(tmp_path, **over):
    sys.path.insert(0, ROOT)
    from examples import deeponet_antiderivative as ex

    cfg = dict(ex.DEFAULTS, output_dir=str(tmp_path), log_freq=10 ** 6, eval_during_train=False, save_freq=0)
    cfg.update(over)
    return ex.build(cfg)


def test_antiderivative_example_learns(dev, tmp_path):
    """G_eval L2Rel falls at least 5-fold from its initial value at the reference's data size on the device.  The emulator
    run is 300 steps on 256 samples (0.25 s a step there) and must cut it 3-fold: that short run reaches 4.4-fold."""
    if dev == "emu":
        solver, fold = _example(tmp_path, n_train=256, n_test=200, epochs=300, learning_rate=3e-3), 3.0
    else:
        solver, fold = _example(tmp_path, epochs=2000, learning_rate=3e-3), 5.0
    l0 = solver.eval()[0]
    solver.train()
    l1 = solver.eval()[0]
    assert l1 < l0 / fold, (l0, l1)
