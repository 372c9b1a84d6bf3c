"""Shared by the SPINN general-path tests: the cases of tests/golden/spinn_jet.npz (make_spinn_jet_golden.py: the reference's own
SPINN under hvp_revrev / nested jvp, float64) as models, closures and constraints of the public API."""
import os

import numpy as np

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "spinn_jet.npz"))
# (case, residual) pairs of the fixture
PAIRS = [("A", "kg"), ("A", "burgers"), ("A", "sg"), ("B", "kg"), ("C", "kg"), ("C", "burgers"), ("C", "sg"), ("D", "burgers"),
         ("E", "sg"), ("F", "ut")]
KEYS = ("t", "x", "y")


def closures(model):
    """The fixture's residuals in the reference's idiom: hvp_revrev / jvp through model.forward_tensor."""
    from ppsci.autodiff import jvp
    from ppsci.equation.pde.helmholtz import hvp_revrev

    f = model.forward_tensor

    def second(t, x, y):
        return (hvp_revrev(lambda t_: f(t_, x, y), (t,)), hvp_revrev(lambda x_: f(t, x_, y), (x,)),
                hvp_revrev(lambda y_: f(t, x, y_), (y,)))

    def kg(d):
        t, x, y = d["t"], d["x"], d["y"]
        u_tt, u_xx, u_yy = second(t, x, y)
        return u_tt - u_xx - u_yy + d["u"] * d["u"]

    def burgers(d):
        t, x, y = d["t"], d["x"], d["y"]
        _, u_xx, u_yy = second(t, x, y)
        u_t = jvp(lambda t_: f(t_, x, y), (t,))[1][0]
        u_x = jvp(lambda x_: f(t, x_, y), (x,))[1][0]
        return u_t + d["u"] * u_x - 0.01 * (u_xx + u_yy)

    def sg(d):
        t, x, y = d["t"], d["x"], d["y"]
        u_tt, u_xx, u_yy = second(t, x, y)
        u_xy = jvp(lambda y_: jvp(lambda x_: f(t, x_, y_), (x,))[1][0], (y,))[1]
        return u_tt - u_xx - u_yy + d["u"].sin() + x * u_xy

    def ut(d):
        t, x, y = d["t"], d["x"], d["y"]
        return jvp(lambda t_: f(t_, x, y), (t,))[1][0]

    return {"kg": kg, "burgers": burgers, "sg": sg, "ut": ut}


def make_model(c):
    import ppsci

    r, nl, hid = (int(v) for v in G[f"{c}/config"])
    model = ppsci.arch.SPINN(KEYS, ("u",), r, nl, hid, str(G[f"{c}/activation"]))
    state = {}
    for k in G.files:
        if k.startswith(f"{c}/param/"):
            _, _, b, n = k.split("/", 3)
            state[f"branch_nets.{b}.{n}"] = G[k].astype(np.float32)
    missing, unexpected = model.set_state_dict(state)
    assert not missing and not unexpected
    return model


def grad_ref(prefix, model):
    """The fixture's gradient under `prefix` ("A/kg", "G") in the order of the flat gradient (= state-dict order)."""
    out = []
    for name in model._names:
        b, n = name.split(".", 2)[1], name.split(".", 2)[2]
        out.append(np.asarray(G[f"{prefix}/grad/{b}/{n}"], dtype=np.float64).ravel())
    return np.concatenate(out)


def coords(c):
    return {k: G[f"{c}/{k}"].astype(np.float32) for k in KEYS}


def constraint(model, c, e, name="PDE", loss=None):
    """SupervisedConstraint of case c's grid, label and weight on residual e (or several: a tuple, every key with the case's label
    and weight grids) of `model`; MSELoss("mean") unless `loss` is given."""
    import ppsci

    es = (e,) if isinstance(e, str) else tuple(e)
    data = coords(c)
    label, weight = G[f"{c}/label"].astype(np.float32), G[f"{c}/weight"].astype(np.float32)
    return ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "ContinuousNamedArrayDataset", "input": lambda: data, "label": lambda d: {k: label for k in es},
                     "weight": lambda d: {k: weight for k in es}}},
        output_expr={k: closures(model)[k] for k in es}, loss=loss or ppsci.loss.MSELoss("mean"), name=name)


def solver_for(model, csts, out_dir, **kw):
    import ppsci

    opt = ppsci.optimizer.Adam(1e-3)(model)
    kw.setdefault("epochs", 1)
    kw.setdefault("iters_per_epoch", 1)
    return ppsci.solver.Solver(model, csts, str(out_dir), opt, **kw)


def bind_all(solver, csts):
    ccs = []
    for name, cst in csts.items():
        cc = solver._compiled[name]
        inp, lab, w = next(cst.data_iter)
        cc.bind(inp, lab, w)
        ccs.append(cc)
    return ccs
