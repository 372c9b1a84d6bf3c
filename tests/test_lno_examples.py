"""ppsci.arch.LNO through the public API: Solver steps against tests/golden/lno.npz (the reference's own run), learning measured
against the reference's float64 AdamW run, the brusselator3d example port.  (The two-rank run is tests/test_lno_distributed.py: it has no device variant.)"""
import os

import numpy as np
import pytest
import torch

from tests.common import make_dev_fixture, rel
from tests.test_lno import GOLD, make_model

dev = make_dev_fixture()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solver(model, x, y, tmp_path, steps, reduction="sum", lr=5e-3, bs=None):
    import ppsci

    cfg = {"dataset": {"name": "NamedArrayDataset", "input": {"input": x}, "label": {"output": y}},
           "batch_size": bs or len(x), "sampler": {"name": "BatchSampler", "shuffle": False, "drop_last": True}}
    cst = ppsci.constraint.SupervisedConstraint(cfg, ppsci.loss.L2RelLoss(reduction), name="Sup")
    opt = ppsci.optimizer.AdamW(lr, weight_decay=1e-4)(model)
    return ppsci.solver.Solver(model, {"Sup": cst}, str(tmp_path), opt, epochs=steps, iters_per_epoch=1, log_freq=1)


def _rel_loss64(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    b = x.shape[0]
    return float((np.linalg.norm((x - y).reshape(b, -1), axis=1) / np.linalg.norm(y.reshape(b, -1), axis=1)).sum())


def test_one_solver_step_matches_the_reference(tmp_path):
    """Loss of the first step against the fixture (the reference's loss before training, 3e-5), engine.grad against the executor
    driven with the same cotangent (5e-5), L2RelLoss.value_and_grad against the torch fallback it replaces."""
    import ppsci

    model = make_model("small")
    x, y = GOLD["small/train_x"], GOLD["small/train_y"]
    solver = _solver(model, x, y, tmp_path, 1, lr=1e-9)
    solver.train()
    loss = solver.last_losses["loss"]
    print(f"loss {loss!r} reference {float(GOLD['small/train_loss'][0])!r}")
    assert abs(loss - GOLD["small/train_loss"][0]) <= 3e-5 * GOLD["small/train_loss"][0]
    grad = solver.engine.grad.cpu().numpy().copy()
    # the same gradient from the executor alone, with the loss's adjoint formed in float64 on the host
    other = make_model("small")
    nat = other.native()
    d = other.flat_params.device
    out = nat.forward(torch.tensor(x).to(d)).cpu().numpy().astype(np.float64)
    b = len(x)
    diff = (out - y).reshape(b, -1)
    gy = diff / (np.linalg.norm(diff, axis=1, keepdims=True) * np.linalg.norm(y.reshape(b, -1).astype(np.float64), axis=1, keepdims=True))
    nat.backward(torch.tensor(gy.reshape(out.shape), dtype=torch.float32).to(d))
    e = rel(grad, other.flat_grad.cpu().numpy())
    print(f"engine.grad vs executor: {e:.2e}")
    assert e <= 5e-5
    # value_and_grad against torch's autograd on L2RelLoss.forward
    lossfn = ppsci.loss.L2RelLoss("sum", weight=0.7)
    yt, lt = torch.tensor(out, dtype=torch.float32).to(d), torch.tensor(y).to(d)
    val, g = lossfn.value_and_grad(yt, lt, "output")
    yr = yt.clone().requires_grad_(True)
    ref = lossfn({"output": yr}, {"output": lt})["output"]
    (gr,) = torch.autograd.grad(ref, yr)
    assert abs(float(val["output"]) - float(ref)) <= 3e-5 * abs(float(ref))
    assert rel(g.cpu().numpy(), gr.cpu().numpy()) <= 5e-5
    assert tuple(g.shape) == tuple(yt.shape)


def test_learning_against_the_reference(tmp_path):
    """From the fixture's weights on the fixture's batch, 30 AdamW steps through Solver remove at least half of the loss decrease
    the reference's float64 run achieved (measured on this framework's emulator: see DESIGN.md 4.10)."""
    model = make_model("small")
    x, y = GOLD["small/train_x"], GOLD["small/train_y"]
    l0, l30 = (float(v) for v in GOLD["small/train_loss"])
    solver = _solver(model, x, y, tmp_path, 30)
    solver.train()
    d = model.flat_params.device
    out = model({"input": torch.tensor(x).to(d)})["output"].cpu().numpy()
    mine = _rel_loss64(out, y)
    frac = (l0 - mine) / (l0 - l30)
    print(f"reference {l0:.4f} -> {l30:.4f}; here L(30) = {mine:.4f}: {frac:.3f} of the reference's decrease")
    assert mine <= l0 - 0.5 * (l0 - l30)


def test_brusselator_example_trains(dev, tmp_path):
    from examples import brusselator3d_lno as ex

    cfg = dict(ex.DEFAULTS, output_dir=str(tmp_path), epochs=2, iters_per_epoch=2, eval_during_train=False, save_freq=0, log_freq=1)
    if dev == "emu":  # a reduced size on the emulator, the yaml's on the device
        cfg.update(NUM_T=9, ORIG_R=11, n_train=8, n_test=6, batch_size=4, width=4, modes=(3, 2, 2), hidden_features=16)
    else:
        cfg.update(n_train=100, n_test=50)
    solver = ex.build(cfg)
    model = solver.model
    before = model.flat_params.cpu().numpy().copy()
    solver.train()
    assert np.isfinite(solver.last_losses["loss"])
    after = model.flat_params.cpu().numpy()
    assert np.isfinite(after).all() and np.abs(after - before).max() > 0
    target, group = solver.eval()
    assert np.isfinite(target) and "L2Rel.output" in group["sup_validator"]
    # the training step's buffer set survived the evaluation at another batch size
    assert model.native().generation == 0
