"""Laplace neural operator on a forced reaction system, after the train mode of /root/reference/examples/brusselator3d/
brusselator3d.py (+ conf/brusselator3d.yaml): the model, optimizer (AdamW, Step schedule by epoch), constraint, validator and
metric with the yaml's literals; the example's own min-max encode / decode and its three grid channels (`cat_grid`).

The reference reads brusselator3d_dataset.npz, which is not available offline; this port computes arrays in the same key format
(inputs_* [n, NUM_T] forcing time series, outputs_* [n, NUM_T, ORIG_R, ORIG_R] response fields) from a stated recipe:

  * forcing  f(t) = a sin(w t + p) exp(-d t) on t = linspace(0, 19, NUM_T), a ~ U(0.5, 2), w ~ U(0.3, 1.5), p ~ U(0, 2 pi),
    d ~ U(0, 0.1), one draw per sample from numpy's default_rng(seed);
  * response u'' + 0.6 u' + u + 0.2 u^3 = f, u(0) = u'(0) = 0, explicit (symplectic) Euler with 16 substeps per interval and
    f linear in between; the field is u(t) (1 + 0.2 sin(2 pi x) cos(2 pi y)) on the ORIG_R x ORIG_R unit grid.

As `DataFuncs.transform` does, the forcing is tiled over the ORIG_R x ORIG_R grid and both are subsampled by RESOLUTION (28 -> 14).

    python examples/brusselator3d_lno.py epochs=300
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppsci  # noqa: E402
from examples._args import parse  # noqa: E402
from ppsci.utils import logger  # noqa: E402

DEFAULTS = dict(seed=2024, output_dir="./output_brusselator3d", NUM_T=39, ORIG_R=28, RESOLUTION=2, n_train=800, n_test=200,
                width=8, modes=(4, 4, 4), in_features=4, hidden_features=64, activation="relu", use_norm=True, use_grid=False,
                epochs=300, batch_size=50, iters_per_epoch=16, learning_rate=0.005, gamma=0.5, step_size=100, weight_decay=1e-4,
                log_freq=20, save_freq=20, eval_freq=20, eval_during_train=True)


def make_data(n: int, nt: int, r: int, seed: int):
    """(inputs [n, nt], outputs [n, nt, r, r]) of the recipe in the module docstring."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 19.0, nt)
    a, w, p, d = rng.uniform(0.5, 2, (n, 1)), rng.uniform(0.3, 1.5, (n, 1)), rng.uniform(0, 2 * np.pi, (n, 1)), rng.uniform(0, 0.1, (n, 1))
    f = a * np.sin(w * t[None] + p) * np.exp(-d * t[None])
    sub = 16
    h = (t[1] - t[0]) / sub
    u, v = np.zeros(n), np.zeros(n)
    resp = np.zeros((n, nt))
    for k in range(nt - 1):
        for s in range(sub):
            fk = f[:, k] + (f[:, k + 1] - f[:, k]) * (s / sub)
            v = v + h * (fk - 0.6 * v - u - 0.2 * u ** 3)
            u = u + h * v
        resp[:, k + 1] = u
    x = np.linspace(0.0, 1.0, r)
    shape = 1 + 0.2 * np.sin(2 * np.pi * x)[:, None] * np.cos(2 * np.pi * x)[None, :]
    return f.astype(np.float32), (resp[:, :, None, None] * shape[None, None]).astype(np.float32)


class DataFuncs:
    """brusselator3d.py:20-86 (transform, encode / decode, cat_grid)."""

    def __init__(self, orig_r: int, r: int, nt: int):
        self.orig_r, self.r, self.nt = orig_r, r, nt
        self.s = int((orig_r - 1) / r + 1)
        x = np.linspace(0, 1, orig_r)
        self.tt, self.xx, self.yy = np.meshgrid(np.linspace(0, 1, nt), x, x, indexing="ij")

    @staticmethod
    def get_mean_std(data):
        lo, hi = np.min(data), np.max(data)
        return (lo + hi) / 2, (hi - lo) / 2

    def _grid(self, grid, num):
        g = np.tile(grid, (num, 1, 1, 1))[:, :, ::self.r, ::self.r][:, :, :self.s, :self.s]
        return np.reshape(g, (num, self.nt, self.s, self.s, 1))

    def cat_grid(self, data):
        n = data.shape[0]
        return np.concatenate([data, self._grid(self.tt, n), self._grid(self.xx, n), self._grid(self.yy, n)], axis=-1).astype(data.dtype)

    def transform(self, data, key="input"):
        if key == "input":
            data = np.transpose(np.tile(np.expand_dims(data, 0), (self.orig_r, self.orig_r, 1, 1)), (2, 3, 0, 1))
        data = data[:, :, ::self.r, ::self.r][:, :, :self.s, :self.s]
        return np.reshape(data, (data.shape[0], self.nt, self.s, self.s, 1))


def build(cfg):
    ppsci.utils.misc.set_random_seed(cfg["seed"])
    os.makedirs(cfg["output_dir"], exist_ok=True)
    funcs = DataFuncs(cfg["ORIG_R"], cfg["RESOLUTION"], cfg["NUM_T"])
    in_tr, out_tr = make_data(cfg["n_train"], cfg["NUM_T"], cfg["ORIG_R"], cfg["seed"])
    in_te, out_te = make_data(cfg["n_test"], cfg["NUM_T"], cfg["ORIG_R"], cfg["seed"] + 1)
    in_train, label_train = funcs.transform(in_tr, "input"), funcs.transform(out_tr, "label")
    in_val, label_val = funcs.transform(in_te, "input"), funcs.transform(out_te, "label")
    in_mean, in_std = funcs.get_mean_std(in_train)
    lab_mean, lab_std = (float(v) for v in funcs.get_mean_std(label_train))
    input_constraint, input_validator = (in_train - in_mean) / in_std, (in_val - in_mean) / in_std
    if not cfg["use_grid"]:
        input_constraint, input_validator = funcs.cat_grid(input_constraint), funcs.cat_grid(input_validator)
    T = np.linspace(0, 19, cfg["NUM_T"]).reshape(1, -1)
    X = np.linspace(0, 1, cfg["ORIG_R"]).reshape(1, -1)[:, :funcs.s]
    model = ppsci.arch.LNO(("input",), ("output",), cfg["width"], tuple(cfg["modes"]), T, (X, X.copy()), cfg["in_features"],
                           cfg["hidden_features"], cfg["activation"], cfg["use_norm"], cfg["use_grid"])
    lr = ppsci.optimizer.lr_scheduler.Step(cfg["epochs"], cfg["iters_per_epoch"], cfg["learning_rate"], cfg["step_size"],
                                           cfg["gamma"], by_epoch=True)()
    optimizer = ppsci.optimizer.AdamW(lr, weight_decay=cfg["weight_decay"])(model)
    sup_constraint = ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "NamedArrayDataset", "input": {"input": input_constraint.astype(np.float32)},
                     "label": {"output": ((label_train - lab_mean) / lab_std).astype(np.float32)}},
         "batch_size": cfg["batch_size"], "sampler": {"name": "BatchSampler", "drop_last": False, "shuffle": True}},
        ppsci.loss.L2RelLoss("sum"), name="sup_constraint")
    sup_validator = ppsci.validate.SupervisedValidator(
        {"dataset": {"name": "NamedArrayDataset", "input": {"input": input_validator.astype(np.float32)},
                     "label": {"output": label_val.astype(np.float32)}}, "batch_size": cfg["batch_size"]},
        ppsci.loss.L2RelLoss("sum"), {"output": lambda out: out["output"] * lab_std + lab_mean},
        metric={"L2Rel": ppsci.metric.L2Rel()}, name="sup_validator")
    return ppsci.solver.Solver(model, {sup_constraint.name: sup_constraint}, cfg["output_dir"], optimizer, lr, cfg["epochs"],
                               cfg["iters_per_epoch"], save_freq=cfg["save_freq"], eval_freq=cfg["eval_freq"],
                               log_freq=cfg["log_freq"], seed=cfg["seed"], validator={sup_validator.name: sup_validator},
                               eval_during_train=cfg["eval_during_train"])


if __name__ == "__main__":
    cfg = parse(dict(DEFAULTS))
    os.makedirs(cfg["output_dir"], exist_ok=True)
    logger.init_logger("ppsci", os.path.join(cfg["output_dir"], "train.log"))
    solver = build(cfg)
    solver.train()
    solver.eval()
