"""Front end of the general SPINN path: the same residual written with hvp_revrev, with nested jvp and with model.derivative
lowers to one program and one stream table (host only), and what the path does not run is refused with the cause."""
import numpy as np
import pytest

from tests.common import make_dev_fixture
from tests.spinn_jet_cases import KEYS, closures, constraint, make_model, solver_for

dev = make_dev_fixture()


def lowered(model, expr):
    """(Lowered, JetTable) of one residual under a weighted label."""
    from paddlescience_amd import graph
    from paddlescience_amd.arch.spinn import JetTable
    from paddlescience_amd.compile import loss_terms
    from paddlescience_amd.graph import Sym

    data = {k: Sym.input(k) for k in KEYS}
    data.update(model(data))
    v = expr(data)
    v = v._as_sym() if hasattr(v, "_as_sym") else v
    jet = JetTable(model)
    return graph.lower({"e": v}, loss_terms(["e"], ["e"], None, 0, scale=1.0), jet=jet), jet


def _lower(model, expr):
    low, jet = lowered(model, expr)
    return low.program.instrs, low.program.res, jet.orders, low.aux_names


def test_three_spellings_lower_to_one_program(dev):
    from ppsci.autodiff import jvp

    model = make_model("A")
    f = model.forward_tensor

    def nested(d):  # hvp_revrev's two jvp calls written out, and u_xy over two different primals
        t, x, y = d["t"], d["x"], d["y"]
        u_tt = jvp(lambda t_: jvp(lambda t__: f(t__, x, y), (t_,))[1], (t,))[1][0]
        u_xx = jvp(lambda x_: jvp(lambda x__: f(t, x__, y), (x_,))[1], (x,))[1][0]
        u_yy = jvp(lambda y_: jvp(lambda y__: f(t, x, y__), (y_,))[1], (y,))[1][0]
        u_xy = jvp(lambda x_: jvp(lambda y_: f(t, x_, y_), (y,))[1][0], (x,))[1]
        return u_tt - u_xx - u_yy + d["u"].sin() + x * u_xy

    def direct(d):
        D = model.derivative
        return D("t", "t") - D("x", "x") - D("y", "y") + D().sin() + d["x"] * D("y", "x")

    a, b, c = _lower(model, closures(model)["sg"]), _lower(model, nested), _lower(model, direct)
    assert a == b == c
    assert a[2] == [(2, 0, 0), (0, 2, 0), (0, 0, 2), (0, 0, 0), (0, 1, 1)]  # distinct order triples in order of first use
    assert model.second_derivative("x").c.tolist() == model.derivative("x", "x").c.tolist()


def test_a_linear_form_keeps_the_four_coefficient_kernels(dev, tmp_path):
    """A residual that stays a GridLinear compiles as before; one non-linear term sends the whole constraint down the general path."""
    import ppsci
    from paddlescience_amd.spinn_engine import SpinnConstraint, SpinnJetConstraint

    model = make_model("A")
    data = {k: np.linspace(0, 1, n, dtype=np.float32).reshape(-1, 1) for k, n in zip(KEYS, (3, 4, 5))}
    lab = np.zeros((3, 4, 5, 1), np.float32)

    def cst(expr):
        return ppsci.constraint.SupervisedConstraint(
            {"dataset": {"name": "ContinuousNamedArrayDataset", "input": lambda: data, "label": lambda d: {"e": lab}}},
            output_expr={"e": expr}, loss=ppsci.loss.MSELoss("mean"), name="c")

    lin = solver_for(model, {"c": cst(lambda d: 4.0 * d["u"] + model.second_derivative("t") - model.derivative("x", "x"))}, tmp_path)
    assert type(lin._compiled["c"]) is SpinnConstraint
    assert lin._compiled["c"].coeffs.tolist() == [4.0, 1.0, -1.0, 0.0]
    gen = solver_for(model, {"c": cst(lambda d: 4.0 * d["u"] + model.second_derivative("t") * d["u"])}, tmp_path)
    assert type(gen._compiled["c"]) is SpinnJetConstraint


def test_refusals_name_the_cause(dev, tmp_path):
    from paddlescience_amd import graph
    from paddlescience_amd.graph import Sym
    from ppsci.autodiff import jacobian, jvp

    model = make_model("A")
    data = {k: Sym.input(k) for k in KEYS}
    data.update(model(data))
    # per-axis order 3
    with pytest.raises(NotImplementedError, match=r"order 3 along axis 'x'"):
        model.derivative("x", "x", "x")
    with pytest.raises(NotImplementedError, match=r"order 3 along axis 'x'"):
        graph.diff(model.derivative("x", "x", "y"), "x")
    # 17 distinct streams
    D = model.derivative
    triples = [(a, b, c) for a in range(3) for b in range(3) for c in range(3)][:17]

    def many(d):
        out = 0.0
        for a, b, c in triples:
            out = out + D(*(("t",) * a + ("x",) * b + ("y",) * c)) * d["u"]
        return out

    with pytest.raises(NotImplementedError, match="more than 16 distinct derivative streams"):
        solver_for(model, {"PDE": _with_expr(model, many)}, tmp_path)
    # a learnable equation parameter
    with pytest.raises(NotImplementedError, match="learnable equation parameter 'nu'"):
        solver_for(model, {"PDE": _with_expr(model, lambda d: Sym.param("nu", 0) * d["u"] * d["u"])}, tmp_path)
    # jacobian on a SPINN output
    with pytest.raises(NotImplementedError, match="sums over the two other axes"):
        jacobian(data["u"], data["x"])
    with pytest.raises(NotImplementedError, match="jvp"):
        jacobian(data["u"] * data["u"], data["x"])
    # numeric input to jvp
    with pytest.raises(TypeError, match="Numeric tensors carry no derivative graph"):
        jvp(lambda x_: model.forward_tensor(data["t"], x_, data["y"]), (np.zeros((3, 1), np.float32),))


def _with_expr(model, expr):
    cst = constraint(model, "A", "kg")
    cst.output_expr = {"kg": expr}
    return cst
