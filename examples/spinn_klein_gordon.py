"""SPINN on the non-linear Klein-Gordon equation  u_tt - u_xx - u_yy + u^2 = f  on [0, 1] x [-1, 1]^2, in the style of
examples/spinn_helmholtz3d.py, with the residual written as a user of the reference writes it: `hvp_revrev` through
`model.forward_tensor` (/root/reference/ppsci/equation/pde/helmholtz.py:27-41, :86-88).

Manufactured solution u* = cos(2 t) sin(pi x) sin(pi y): f = (2 pi^2 - 4) u* + u*^2, u = 0 on the four space faces,
u(0) = sin(pi x) sin(pi y) and u_t(0) = 0; f and the initial / boundary data are computed on the host.  The PDE constraint (u^2)
and the initial-velocity face (u_t) run on the general grid kernels, the five Dirichlet faces on the four-coefficient ones.

    python examples/spinn_klein_gordon.py nc=32 iters_per_epoch=2000
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppsci  # noqa: E402
from examples._args import parse  # noqa: E402
from ppsci.autodiff import jvp  # noqa: E402
from ppsci.equation.pde.helmholtz import hvp_revrev  # noqa: E402
from ppsci.utils import logger  # noqa: E402

dtype = "float32"


def exact_u(t, x, y):
    return np.cos(2.0 * t) * np.sin(np.pi * x) * np.sin(np.pi * y)


def source_term(t, x, y):
    u = exact_u(t, x, y)
    return (2.0 * np.pi**2 - 4.0) * u + u * u


def main():
    cfg = parse(dict(seed=111, output_dir="./output_spinn_kg", epochs=1, iters_per_epoch=2000, nc=32, nc_test=50, r=32,
                     num_layers=4, hidden_size=64, learning_rate=1e-3, gamma=0.9, decay_steps=1000, log_freq=100,
                     resample_every=100))
    ppsci.utils.misc.set_random_seed(cfg["seed"])
    logger.init_logger("ppsci", os.path.join(cfg["output_dir"], "train.log"))
    model = ppsci.arch.SPINN(("t", "x", "y"), ("u",), cfg["r"], cfg["num_layers"], cfg["hidden_size"], "tanh")
    f = model.forward_tensor

    def klein_gordon(d):
        t, x, y = d["t"], d["x"], d["y"]
        u__t__t = hvp_revrev(lambda t_: f(t_, x, y), (t,))
        u__x__x = hvp_revrev(lambda x_: f(t, x_, y), (x,))
        u__y__y = hvp_revrev(lambda y_: f(t, x, y_), (y,))
        return u__t__t - u__x__x - u__y__y + d["u"] * d["u"]

    def u__t(d):
        t, x, y = d["t"], d["x"], d["y"]
        return jvp(lambda t_: f(t_, x, y), (t,))[1][0]

    state = {"iter": 0}

    def gen():
        nc = cfg["nc"]
        tc = np.random.uniform(0.0, 1.0, [nc, 1]).astype(dtype)
        xc, yc = (np.random.uniform(-1.0, 1.0, [nc, 1]).astype(dtype) for _ in range(2))
        tm, xm, ym = np.meshgrid(tc, xc, yc, indexing="ij")
        zero, one, mone = (np.asarray([[v]], dtype) for v in (0.0, 1.0, -1.0))
        state.update(tc=tc, xc=xc, yc=yc, fc=source_term(tm, xm, ym)[..., None].astype(dtype), t0=(zero, xc, yc),
                     faces=[(zero, xc, yc), (tc, one, yc), (tc, mone, yc), (tc, xc, one), (tc, xc, mone)])

    gen()

    def interior():
        state["iter"] += 1
        if state["iter"] % cfg["resample_every"] == 0:
            gen()
        return {"t": state["tc"], "x": state["xc"], "y": state["yc"], "fc": state["fc"]}

    def grid_of(d, fn):
        tm, xm, ym = np.meshgrid(d["t"], d["x"], d["y"], indexing="ij")
        return fn(tm, xm, ym)[..., None].astype(dtype)

    keys = ("t", "x", "y")
    constraint = {"PDE": ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "ContinuousNamedArrayDataset", "input": interior, "label": lambda d: {"klein_gordon": d["fc"]}},
         "shard_in_engine": True},
        output_expr={"klein_gordon": klein_gordon}, loss=ppsci.loss.MSELoss("mean"), name="PDE")}
    for i in range(5):  # u on the initial face and on the four space faces (the exact solution vanishes on the latter)
        constraint[f"BC{i}"] = ppsci.constraint.SupervisedConstraint(
            {"dataset": {"name": "ContinuousNamedArrayDataset", "input": (lambda i=i: dict(zip(keys, state["faces"][i]))),
                         "label": lambda d: {"u": grid_of(d, exact_u)}},
             "shard_in_engine": True},
            output_expr={"u": lambda out: out["u"]}, loss=ppsci.loss.MSELoss("mean"), name=f"BC{i}")
    constraint["IC_t"] = ppsci.constraint.SupervisedConstraint(  # initial velocity u_t(0, x, y) = 0
        {"dataset": {"name": "ContinuousNamedArrayDataset", "input": lambda: dict(zip(keys, state["t0"])),
                     "label": lambda d: {"u__t": np.zeros([1, len(d["x"]), len(d["y"]), 1], dtype)}},
         "shard_in_engine": True},
        output_expr={"u__t": u__t}, loss=ppsci.loss.MSELoss("mean"), name="IC_t")
    sched = ppsci.optimizer.lr_scheduler.ExponentialDecay(cfg["epochs"], cfg["iters_per_epoch"], cfg["learning_rate"],
                                                          cfg["gamma"], cfg["decay_steps"])()
    optimizer = ppsci.optimizer.Adam(sched)(model)
    solver = ppsci.solver.Solver(model, constraint, cfg["output_dir"], optimizer, sched, cfg["epochs"], cfg["iters_per_epoch"],
                                 log_freq=cfg["log_freq"])
    solver.train()
    tt = np.linspace(0.0, 1.0, cfg["nc_test"], dtype=dtype).reshape(-1, 1)
    ss = np.linspace(-1.0, 1.0, cfg["nc_test"], dtype=dtype).reshape(-1, 1)
    tm, xm, ym = np.meshgrid(tt, ss, ss, indexing="ij")
    u_gt = exact_u(tm, xm, ym).reshape(-1)
    pred = solver.predict({"t": tt, "x": ss, "y": ss}, expr_dict={"klein_gordon": klein_gordon}, batch_size=None, return_numpy=True)
    u = pred["u"].reshape(-1)
    res = pred["klein_gordon"].reshape(-1) - source_term(tm, xm, ym).reshape(-1)
    logger.message(f"l2_err = {np.linalg.norm(u - u_gt) / np.linalg.norm(u_gt):.4f}, rmse = {np.sqrt(np.mean((u - u_gt) ** 2)):.4f}, "
                   f"residual rms = {np.sqrt(np.mean(res ** 2)):.4f}")


if __name__ == "__main__":
    main()
