"""Fractional Poisson on the unit disk, after /root/reference/examples/fpde/fractional_poisson_2d.py (train mode, + conf/
fractional_poisson_2d.yaml): (-Δ)^(α/2) u = f with α = 1.8, exact solution |1 - r²|^(1 + α/2).

The interior constraint's dataset transform (a FunctionalTransform config) grows its 100 Hammersley points by their ~690
auxiliary points each (FractionalPoisson.get_x); the residual couples every point to its own auxiliary points through a
constant sparse matrix, which runs as two CSR matrix-vector launches around the per-point programs.  The output transform
(1 - x² - y²) u puts the boundary condition into the network; the 1-point boundary constraint is the reference's.

    python examples/fractional_poisson_2d.py epochs=20000
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppsci  # noqa: E402
from examples._args import parse  # noqa: E402
from ppsci.utils import logger  # noqa: E402

DEFAULTS = dict(seed=42, output_dir="./output_fractional_poisson_2d", epochs=20000, iters_per_epoch=1, ALPHA=1.8,
                NPOINT_INTERIOR=100, NPOINT_BC=1, NPOINT_EVAL=1000, resolution=[8, 100], num_layers=4, hidden_size=20,
                learning_rate=1e-3, log_freq=100, eval_during_train=True, eval_freq=1000, plot=True)


def build(cfg):
    ppsci.utils.misc.set_random_seed(cfg["seed"])
    model = ppsci.arch.MLP(("x", "y"), ("u",), cfg["num_layers"], cfg["hidden_size"], "tanh")

    def output_transform(in_, out):
        return {"u": (1 - (in_["x"] ** 2 + in_["y"] ** 2)) * out["u"]}

    model.register_output_transform(output_transform)
    geom = {"disk": ppsci.geometry.Disk((0, 0), 1)}
    equation = {"fpde": ppsci.equation.FractionalPoisson(cfg["ALPHA"], geom["disk"], list(cfg["resolution"]))}

    def u_solution_func(out):
        return np.abs(1 - (out["x"] ** 2 + out["y"] ** 2)) ** (1 + cfg["ALPHA"] / 2)

    def input_data_fpde_transform(input, weight, label):
        """The sampling points of the fractional integrals behind the collocation points (numpy arrays here)."""
        points = np.concatenate((input["x"], input["y"]), axis=1)
        x = equation["fpde"].get_x(points)
        return {**input, **x}, weight, label

    fpde_constraint = ppsci.constraint.InteriorConstraint(
        equation["fpde"].equations, {"fpde": 0}, geom["disk"],
        {"dataset": {"name": "IterableNamedArrayDataset",
                     "transforms": ({"FunctionalTransform": {"transform_func": input_data_fpde_transform}},)},
         "batch_size": cfg["NPOINT_INTERIOR"], "iters_per_epoch": cfg["iters_per_epoch"]},
        ppsci.loss.MSELoss("mean"), random="Hammersley",
        criteria=lambda x, y: ~geom["disk"].on_boundary(np.hstack((x, y))), name="FPDE")
    bc = ppsci.constraint.BoundaryConstraint(
        {"u": lambda out: out["u"]}, {"u": u_solution_func}, geom["disk"],
        {"dataset": {"name": "IterableNamedArrayDataset"}, "batch_size": cfg["NPOINT_BC"],
         "iters_per_epoch": cfg["iters_per_epoch"]},
        ppsci.loss.MSELoss("mean"), criteria=lambda x, y: np.isclose(x, -1), name="BC")
    optimizer = ppsci.optimizer.Adam(cfg["learning_rate"])(model)
    l2rel_metric = ppsci.validate.GeometryValidator(
        {"u": lambda out: out["u"]}, {"u": u_solution_func}, geom["disk"],
        {"dataset": "IterableNamedArrayDataset", "total_size": cfg["NPOINT_EVAL"]}, ppsci.loss.MSELoss(),
        metric={"L2Rel": ppsci.metric.L2Rel()}, name="L2Rel_Metric")
    return ppsci.solver.Solver(model, {fpde_constraint.name: fpde_constraint, bc.name: bc}, cfg["output_dir"], optimizer,
                               epochs=cfg["epochs"], iters_per_epoch=cfg["iters_per_epoch"], log_freq=cfg["log_freq"],
                               eval_during_train=cfg["eval_during_train"], eval_freq=cfg["eval_freq"], equation=equation,
                               validator={l2rel_metric.name: l2rel_metric})


def plot(cfg, solver):
    """Prediction next to the exact solution on a polar grid (fractional_poisson_2d.py:180-197 of the reference)."""
    from matplotlib import cm
    from matplotlib import pyplot as plt

    theta = np.arange(0, 2 * math.pi, 0.04, dtype="float32")
    rho = np.arange(0, 1, 0.005, dtype="float32")
    mt, mr = np.meshgrid(theta, rho)
    x, y = mr * np.cos(mt), mr * np.sin(mt)
    input_data = {"x": x.reshape([-1, 1]), "y": y.reshape([-1, 1])}
    label = (np.abs(1 - (input_data["x"] ** 2 + input_data["y"] ** 2)) ** (1 + cfg["ALPHA"] / 2)).reshape([x.shape[0], -1])
    pred = solver.predict(input_data, return_numpy=True)["u"].reshape([x.shape[0], -1])
    fig = plt.figure()
    for k, (data, title) in enumerate(((pred, r"$u(x,y)$, prediction"), (label, r"$u(x,y)$, label"))):
        ax = fig.add_subplot(121 + k, projection="3d")
        surf = ax.plot_surface(x, y, data, cmap=cm.jet, linewidth=0, antialiased=False)
        ax.set_zlim(0, 1.2)
        ax.set_xlabel("x")
        ax.set_ylabel("y")
        ax.set_title(title)
        fig.colorbar(surf, ax=ax, aspect=5, orientation="horizontal")
    fig.subplots_adjust(wspace=0.5, hspace=0.5)
    plt.savefig(os.path.join(cfg["output_dir"], "fractional_poisson_2d_result.png"), dpi=400)
    plt.close(fig)


if __name__ == "__main__":
    cfg = parse(dict(DEFAULTS))
    logger.init_logger("ppsci", os.path.join(cfg["output_dir"], "train.log"))
    solver = build(cfg)
    solver.train()
    solver.eval()
    if cfg["plot"]:
        plot(cfg, solver)
