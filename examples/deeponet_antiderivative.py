"""DeepONet learning the antiderivative operator, after the train mode of /root/reference/examples/operator_learning/
deeponet.py (+ conf/deeponet.yaml): G(u)(y) = integral_0^y u(s) ds.

The reference downloads its npz; this port writes its own in the same key format (X_train0 [N, 100] = u at 100 sensors,
X_train1 [N, 1] = y, y_train [N, 1] = G(u)(y); X_test* / y_test likewise) from a stated recipe:

  * u: random smooth functions on [0, 1], a Gaussian random field with squared-exponential covariance (length scale 0.2),
    sampled on a fine grid of 1 001 points; the branch input is u at 100 equispaced sensors;
  * G(u)(y): cumulative trapezoid of u on the fine grid, linearly interpolated at one random y per sample.

The branch key `u` reaches the network as an [N, 100] array.  The reference config uses relu, which the layer-by-layer
stream kernels do not carry; this port uses tanh in both nets.

    python examples/deeponet_antiderivative.py epochs=10000
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppsci  # noqa: E402
from examples._args import parse  # noqa: E402
from ppsci.utils import logger  # noqa: E402

DEFAULTS = dict(seed=2023, output_dir="./output_deeponet", epochs=10000, iters_per_epoch=1, learning_rate=1e-3,
                n_train=10000, n_test=2000, num_loc=100, num_features=40, branch_num_layers=1, trunk_num_layers=1,
                branch_hidden_size=40, trunk_hidden_size=40, branch_activation="tanh", trunk_activation="tanh",
                log_freq=500, eval_during_train=True, eval_freq=500, save_freq=0)


def make_npz(path: str, n: int, num_loc: int, seed: int, prefix: str) -> None:
    """Writes {X_<prefix>0, X_<prefix>1, y_<prefix>} (see the module docstring for the recipe)."""
    rng = np.random.default_rng(seed)
    fine = np.linspace(0.0, 1.0, 1001)
    d = fine[:, None] - fine[None, :]
    cov = np.exp(-0.5 * d * d / 0.2 ** 2) + 1e-8 * np.eye(fine.size)
    chol = np.linalg.cholesky(cov)
    u = (chol @ rng.standard_normal((fine.size, n))).T  # [n, 1001]
    G = np.concatenate([np.zeros((n, 1)), np.cumsum(0.5 * (u[:, 1:] + u[:, :-1]) * np.diff(fine), axis=1)], axis=1)
    sensors = np.linspace(0.0, 1.0, num_loc)
    idx = np.round(sensors * (fine.size - 1)).astype(int)
    y = rng.uniform(0.0, 1.0, n)
    g = np.array([np.interp(y[i], fine, G[i]) for i in range(n)])
    np.savez(path, **{f"X_{prefix}0": u[:, idx].astype(np.float32), f"X_{prefix}1": y[:, None].astype(np.float32),
                      f"y_{prefix}": g[:, None].astype(np.float32)})


def build(cfg):
    ppsci.utils.misc.set_random_seed(cfg["seed"])
    os.makedirs(cfg["output_dir"], exist_ok=True)
    train_path = os.path.join(cfg["output_dir"], "antiderivative_train.npz")
    test_path = os.path.join(cfg["output_dir"], "antiderivative_test.npz")
    make_npz(train_path, cfg["n_train"], cfg["num_loc"], cfg["seed"], "train")
    make_npz(test_path, cfg["n_test"], cfg["num_loc"], cfg["seed"] + 1, "test")
    model = ppsci.arch.DeepONet("u", "y", "G", cfg["num_loc"], cfg["num_features"], cfg["branch_num_layers"],
                                cfg["trunk_num_layers"], cfg["branch_hidden_size"], cfg["trunk_hidden_size"],
                                branch_activation=cfg["branch_activation"], trunk_activation=cfg["trunk_activation"],
                                use_bias=True)
    sup_constraint = ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "IterableNPZDataset", "file_path": train_path, "input_keys": ("u", "y"), "label_keys": ("G",),
                     "alias_dict": {"u": "X_train0", "y": "X_train1", "G": "y_train"}}},
        ppsci.loss.MSELoss(), {"G": lambda out: out["G"]})
    sup_validator = ppsci.validate.SupervisedValidator(
        {"dataset": {"name": "IterableNPZDataset", "file_path": test_path, "input_keys": ("u", "y"), "label_keys": ("G",),
                     "alias_dict": {"u": "X_test0", "y": "X_test1", "G": "y_test"}}},
        ppsci.loss.MSELoss(), {"G": lambda out: out["G"]}, metric={"L2Rel": ppsci.metric.L2Rel()}, name="G_eval")
    optimizer = ppsci.optimizer.Adam(cfg["learning_rate"])(model)
    return ppsci.solver.Solver(model, {sup_constraint.name: sup_constraint}, cfg["output_dir"], optimizer, None,
                               cfg["epochs"], cfg["iters_per_epoch"], save_freq=cfg["save_freq"], eval_freq=cfg["eval_freq"],
                               log_freq=cfg["log_freq"], seed=cfg["seed"], validator={sup_validator.name: sup_validator},
                               eval_during_train=cfg["eval_during_train"])


if __name__ == "__main__":
    cfg = parse(dict(DEFAULTS))
    os.makedirs(cfg["output_dir"], exist_ok=True)
    logger.init_logger("ppsci", os.path.join(cfg["output_dir"], "train.log"))
    solver = build(cfg)
    solver.train()
    solver.eval()
