"""Geo-FNO on the catheter design problem, after the train and eval modes of /root/reference/examples/catheter/catheter.py
(+ conf/catheter.yaml): FNO1d, L2RelLoss("sum"), Adam with weight decay on a Step schedule, the L2Rel validator, the loss-history
plot and the evaluation figures, with the yaml's literals.  `export` / `inference` are not ported.

The reference reads x / y / density .npy files, which are not available offline; this port computes arrays with getdata's shape
conventions (inputs [n, s, 2] = the wall's abscissa and height, labels [n, s, 1] = the log of a density) from a stated recipe:

  * abscissa x = linspace(-500, 0, s); wall height y(x) = 20 + h tri(x; L_p, x2, x3): periodic triangular ridges of period
    L_p ~ U(60, 250), rising over the fraction x2 ~ U(0.15, 0.5) and falling over x3 ~ U(0.15, 0.5) of a period, height
    h ~ U(20, 30), one draw per sample from numpy's default_rng(seed);
  * label (a log-density: bacteria enter at x = 0 and swim upstream): label(x) = - 6 / 500 * integral_x^0 r(x') dx' + 0.3 tri(x)
    with r = (100 - 2 y) / 60, the channel's width over 60, the integral as a cumulative trapezoid sum from the right end: a
    smooth functional of the curve that is causal from the right, plus a local term.

    python examples/catheter_geofno.py epochs=1001
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppsci  # noqa: E402
from examples._args import parse  # noqa: E402
from ppsci.utils import logger  # noqa: E402

DEFAULTS = dict(seed=42, output_dir="./output_catheter", n_train=1000, n_test=100, s=2001, modes=64, width=64, padding=100,
                input_channel=2, output_np=2001, epochs=1001, learning_rate=0.001, step_size=100, gamma=0.5, weight_decay=1e-4,
                eval_during_train=True, batch_size=20, save_freq=100, eval_freq=100, log_freq=100, plot_samples=(0, 8))


def getdata(n: int, s: int, seed: int):
    """(inputs [n, s, 2], labels [n, s, 1], parameters [4, n]) of the recipe in the module docstring (catheter.py:32-75 keeps
    these shapes)."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-500.0, 0.0, s)
    Lp, x2, x3, h = rng.uniform(60, 250, (n, 1)), rng.uniform(0.15, 0.5, (n, 1)), rng.uniform(0.15, 0.5, (n, 1)), rng.uniform(20, 30, (n, 1))
    ph = np.mod(-x[None] / Lp, 1.0)
    tri = np.clip(np.minimum(ph / x2, (x2 + x3 - ph) / x3), 0.0, 1.0)
    y = 20.0 + h * tri
    r = (100.0 - 2.0 * y) / 60.0
    dx = x[1] - x[0]
    seg = 0.5 * (r[:, 1:] + r[:, :-1]) * dx
    integral = np.concatenate([np.cumsum(seg[:, ::-1], 1)[:, ::-1], np.zeros((n, 1))], 1)  # integral_x^0 r
    label = -6.0 / 500.0 * integral + 0.3 * tri
    inputs = np.stack([np.broadcast_to(x[None], y.shape), y], -1).astype(np.float32)
    return inputs, label[..., None].astype(np.float32), np.concatenate([Lp, x2, x3, h], 1).T


def build(cfg):
    ppsci.utils.misc.set_random_seed(cfg["seed"])
    os.makedirs(cfg["output_dir"], exist_ok=True)
    inputs_train, labels_train, _ = getdata(cfg["n_train"], cfg["s"], cfg["seed"])
    inputs_test, labels_test, _ = getdata(cfg["n_test"], cfg["s"], cfg["seed"] + 1)
    sup_constraint = ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "NamedArrayDataset", "input": {"input": inputs_train}, "label": {"output": labels_train}},
         "batch_size": cfg["batch_size"], "sampler": {"name": "BatchSampler", "drop_last": False, "shuffle": True}},
        ppsci.loss.L2RelLoss("sum"), name="sup_constraint")
    model = ppsci.arch.FNO1d(modes=cfg["modes"], width=cfg["width"], padding=cfg["padding"], input_channel=cfg["input_channel"],
                             output_np=cfg["output_np"])
    iters_per_epoch = max(int(cfg["n_train"] / cfg["batch_size"]), 1)
    scheduler = ppsci.optimizer.lr_scheduler.Step(epochs=cfg["epochs"], iters_per_epoch=iters_per_epoch,
                                                  learning_rate=cfg["learning_rate"], step_size=cfg["step_size"], gamma=cfg["gamma"])
    optimizer = ppsci.optimizer.Adam(scheduler(), weight_decay=cfg["weight_decay"])(model)
    validator = ppsci.validate.SupervisedValidator(
        {"dataset": {"name": "NamedArrayDataset", "input": {"input": inputs_test}, "label": {"output": labels_test}},
         "batch_size": cfg["batch_size"]},
        ppsci.loss.L2RelLoss("sum"), metric={"L2Rel": ppsci.metric.L2Rel()}, name="L2Rel_Validator")
    return ppsci.solver.Solver(model, {sup_constraint.name: sup_constraint}, cfg["output_dir"], optimizer, epochs=cfg["epochs"],
                               iters_per_epoch=iters_per_epoch, eval_with_no_grad=True, eval_during_train=cfg["eval_during_train"],
                               validator={"validator1": validator}, save_freq=cfg["save_freq"], eval_freq=cfg["eval_freq"],
                               log_freq=cfg["log_freq"], seed=cfg["seed"])


def evaluate(cfg, model):
    """catheter.py:182-239: per plotted sample the relative error and a figure of the wall, the label and the prediction."""
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    x_test, y_test, _ = getdata(cfg["n_test"], cfg["s"], cfg["seed"] + 1)
    xx = np.linspace(-500, 0, cfg["output_np"])
    errors, paths = [], []
    for sample_id in cfg["plot_samples"]:
        if sample_id >= len(x_test):
            continue
        mesh = x_test[sample_id]
        pred = model({"input": x_test[sample_id:sample_id + 1]})["output"].detach().cpu().numpy().flatten()
        ref = y_test[sample_id].flatten()
        if len(ref) != len(pred):
            ref = np.interp(xx, mesh[:, 0], ref)
        errors.append(float(np.linalg.norm(pred - ref) / np.linalg.norm(ref)))
        logger.info(f"sample {sample_id}: rel. error is {errors[-1]:.4e}")
        plt.figure(figsize=(5, 4))
        plt.plot(mesh[:, 0], mesh[:, 1], color="C1", label="Channel geometry")
        plt.plot(mesh[:, 0], 100 - mesh[:, 1], color="C1")
        every = max(len(xx) // 10, 1)
        plt.plot(xx, 50 + 10 * ref, "--o", color="red", markevery=every, label="Reference (50 + 10 log density)")
        plt.plot(xx, 50 + 10 * pred, "--*", color="C2", fillstyle="none", markevery=every, label="Predicted")
        plt.xlabel(r"x")
        plt.legend()
        plt.tight_layout()
        paths.append(os.path.join(cfg["output_dir"], f"Validation.{sample_id}.pdf"))
        plt.savefig(paths[-1])
        plt.close()
    return errors, paths


def export(cfg):
    raise NotImplementedError("catheter_geofno: export is not ported (no static-graph export on this backend)")


def inference(cfg):
    raise NotImplementedError("catheter_geofno: inference through an exported model is not ported")


if __name__ == "__main__":
    cfg = parse(dict(DEFAULTS))
    os.makedirs(cfg["output_dir"], exist_ok=True)
    logger.init_logger("ppsci", os.path.join(cfg["output_dir"], "train.log"))
    solver = build(cfg)
    solver.train()
    solver.plot_loss_history(by_epoch=True, smooth_step=1)
    solver.eval()
    evaluate(cfg, solver.model)
