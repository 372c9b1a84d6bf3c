"""Non-linear residuals on first, second and mixed derivatives of a SPINN, against fixtures produced by the REFERENCE's own
code (tests/golden/make_spinn_jet_golden.py: ppsci/arch/spinn.py under helmholtz.hvp_revrev and nested
paddle.incubate.autograd.jvp, float64), through the public API: ppsci.arch.SPINN, closures written with ppsci.autodiff.jvp /
hvp_revrev, SupervisedConstraint with label and weight grids, Solver, engine.forward_backward and predict(expr_dict=...).

Bounds (tests/test_golden_spinn.py): u rel-L2 <= 5e-6, loss rel <= 3e-5, gradient rel-L2 <= 1e-4; residual grid rel-L2 <= the
larger of 5e-6 and twice the reference's own float32 error recorded in the fixture."""
import os

import numpy as np
import pytest

from tests.common import make_dev_fixture, rel
from tests.spinn_jet_cases import G, PAIRS, closures, constraint, coords, grad_ref, make_model, solver_for, bind_all

dev = make_dev_fixture()
H = np.load(os.path.join(os.path.dirname(__file__), "golden", "spinn.npz"))  # the Helmholtz cases of the linear path


@pytest.mark.parametrize("c,e", PAIRS)
def test_reference_parity(c, e, dev, tmp_path):
    from paddlescience_amd.spinn_engine import SpinnJetConstraint

    model = make_model(c)
    csts = {"PDE": constraint(model, c, e)}
    solver = solver_for(model, csts, tmp_path)
    (cc,) = bind_all(solver, csts)
    assert isinstance(cc, SpinnJetConstraint)
    solver.engine.forward_backward([cc])
    loss, lref = cc.loss(), float(G[f"{c}/{e}/loss"])
    e_g = rel(solver.engine.grad.cpu().numpy(), grad_ref(f"{c}/{e}", model))
    pred = solver.predict(coords(c), expr_dict={e: closures(model)[e]}, batch_size=None, return_numpy=True)
    e_u = rel(pred["u"], G[f"{c}/u"])
    print(f"[{dev}] {c}/{e}: loss rel {abs(loss - lref) / lref:.2e}, grad rel-L2 {e_g:.2e}, u rel-L2 {e_u:.2e}")
    assert pred[e].shape == G[f"{c}/u"].shape
    if f"{c}/{e}/residual" in G.files:
        e_r, bound = rel(pred[e], G[f"{c}/{e}/residual"]), max(5e-6, 2.0 * float(G[f"{c}/{e}/err32"][0]))
        print(f"[{dev}] {c}/{e}: residual rel-L2 {e_r:.2e} (bound {bound:.1e})")
        assert e_r <= bound
    assert loss == pytest.approx(lref, rel=3e-5)
    assert e_g < 1e-4
    assert e_u < 5e-6


def _case_g(tmp_path, **kw):
    model = make_model("A")
    csts = {"PDE": constraint(model, "A", "kg", "PDE"), "face": constraint(model, "F", "ut", "face")}
    return model, csts, solver_for(model, csts, tmp_path, **kw)


def test_two_constraints_one_gradient(dev, tmp_path):
    """Case G: a general PDE constraint and a Neumann face (one-point axis) share the gradient."""
    model, csts, solver = _case_g(tmp_path)
    ccs = bind_all(solver, csts)
    solver.engine.forward_backward(ccs)
    loss = sum(cc.loss() for cc in ccs)
    e_g = rel(solver.engine.grad.cpu().numpy(), grad_ref("G", model))
    print(f"[{dev}] G: loss rel {abs(loss - float(G['G/loss'])) / float(G['G/loss']):.2e}, grad rel-L2 {e_g:.2e}")
    assert loss == pytest.approx(float(G["G/loss"]), rel=3e-5)
    assert e_g < 1e-4


def test_several_keys_in_one_constraint(dev, tmp_path):
    """Case A's three residuals as three keys of ONE constraint (one program, one stream table, three loss columns): every
    loss term is the fixture's, the gradient the sum of the fixture's three."""
    model = make_model("A")
    es = ("kg", "burgers", "sg")
    csts = {"PDE": constraint(model, "A", es)}
    solver = solver_for(model, csts, tmp_path)
    (cc,) = bind_all(solver, csts)
    solver.engine.forward_backward([cc])
    got = cc.losses()
    for e in es:
        assert got[e] == pytest.approx(float(G[f"A/{e}/loss"]), rel=3e-5)
    assert cc.loss() == pytest.approx(sum(got.values()))
    assert rel(solver.engine.grad.cpu().numpy(), sum(grad_ref(f"A/{e}", model) for e in es)) < 1e-4


def test_absolute_value_loss_kind(dev, tmp_path):
    """MAELoss("mean") with the weight grid on case A's kg and burgers: mean(w |r - label|) of the fixture's float64 residual
    grids (loss rel <= 3e-5, the bound of the MSE terms: the same sums without the square)."""
    import ppsci

    model = make_model("A")
    es = ("kg", "burgers")
    csts = {"PDE": constraint(model, "A", es, loss=ppsci.loss.MAELoss("mean"))}
    solver = solver_for(model, csts, tmp_path)
    (cc,) = bind_all(solver, csts)
    solver.engine.forward_backward([cc])
    w, lab = G["A/weight"].astype(np.float64), G["A/label"].astype(np.float64)
    for e in es:
        ref = float(np.mean(w * np.abs(G[f"A/{e}/residual"] - lab)))
        assert cc.losses()[e] == pytest.approx(ref, rel=3e-5)
    assert np.isfinite(solver.engine.grad.cpu().numpy()).all() and float(solver.engine.grad.abs().sum()) > 0


@pytest.mark.parametrize("c", sorted({k.split("/")[0] for k in H.files}))
def test_linear_residual_through_the_general_path(c, dev, tmp_path, monkeypatch):
    """PPSCI_SPINN_JET=1: the Helmholtz cases of the existing spinn.npz pass test_golden_spinn.py's bounds on the general path."""
    import ppsci
    from paddlescience_amd.spinn_engine import SpinnJetConstraint

    monkeypatch.setenv("PPSCI_SPINN_JET", "1")
    r, nl, hid, k = H[f"{c}/config"]
    model = ppsci.arch.SPINN(("x", "y", "z"), ("u",), int(r), int(nl), int(hid), "tanh")
    state = {f"branch_nets.{q.split('/', 3)[2]}.{q.split('/', 3)[3]}": H[q].astype(np.float32) for q in H.files
             if q.startswith(f"{c}/param/")}
    assert model.set_state_dict(state) == ([], [])
    gref = np.concatenate([H[f"{c}/grad/{n.split('.', 2)[1]}/{n.split('.', 2)[2]}"].ravel() for n in model._names])
    eq = ppsci.equation.Helmholtz(3, float(k))
    eq.model = model
    xs = {a: H[f"{c}/{a}"].astype(np.float32) for a in "xyz"}
    data = dict(xs, uc=H[f"{c}/label"].astype(np.float32))
    pde = ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "ContinuousNamedArrayDataset", "input": lambda: data, "label": lambda d: {"helmholtz": d["uc"]}}},
        output_expr=eq.equations, loss=ppsci.loss.MSELoss("mean"), name="PDE")
    solver = solver_for(model, {"PDE": pde}, tmp_path, equation={"Helmholtz": eq})
    cc = solver._compiled["PDE"]
    assert isinstance(cc, SpinnJetConstraint)
    inp, lab, _ = next(pde.data_iter)
    cc.bind(inp, lab)
    solver.engine.forward_backward([cc])
    assert cc.loss() == pytest.approx(float(H[f"{c}/loss"]), rel=3e-5)
    assert rel(solver.engine.grad.cpu().numpy(), gref) < 1e-4
    pred = solver.predict(xs, expr_dict=dict(eq.equations), batch_size=None, return_numpy=True)
    assert rel(pred["u"], H[f"{c}/u"]) < 5e-6
    assert rel(pred["helmholtz"], H[f"{c}/residual"]) < 5e-6


def test_gradient_is_bitwise_repeatable(dev, tmp_path):
    """Case C (full and ragged tiles on every axis, tile reverse sweep of the branch nets): two passes, the same bits."""
    model = make_model("C")
    csts = {"PDE": constraint(model, "C", "sg")}
    solver = solver_for(model, csts, tmp_path)
    ccs = bind_all(solver, csts)
    solver.engine.forward_backward(ccs)
    g1, l1 = solver.engine.grad.cpu().numpy().copy(), ccs[0].loss()
    solver.engine.forward_backward(ccs)
    g2, l2 = solver.engine.grad.cpu().numpy().copy(), ccs[0].loss()
    assert l1 == l2 and np.array_equal(g1, g2)


def test_graph_replay_trains_like_eager_launches(dev, tmp_path, monkeypatch):
    """Three Solver.train steps of case G: the losses with HIP-graph replay equal those with PPSCI_HIP_GRAPH=0, bit for bit
    (on the emulator both runs launch eagerly: the check is then that training is repeatable)."""
    hist = []
    for graph in ("1", "0"):
        monkeypatch.setenv("PPSCI_HIP_GRAPH", graph)
        _, _, solver = _case_g(tmp_path / graph, iters_per_epoch=3, log_freq=1)
        solver.train()
        hist.append([v for _, v in solver.train_loss_info["loss"]])
    assert len(hist[0]) == 3 and hist[0] == hist[1]


def test_slab_sharding_sums_to_one_rank(dev, tmp_path):
    """Case C bound as rank 0 and rank 1 of a world of 2 (two constraint objects, no process group): losses and gradients sum to
    the one-rank result; the weight grid is sliced with the label grid."""
    model = make_model("C")
    cst = constraint(model, "C", "kg")
    solver = solver_for(model, {"PDE": cst}, tmp_path)
    inp, lab, w = next(cst.data_iter)
    res = []
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        cc = solver.engine.compile_constraint("PDE", cst, solver.device)
        cc.world, cc.rank = world, rank
        cc.bind(inp, lab, w)
        solver.engine.forward_backward([cc])
        res.append((cc.loss(), solver.engine.grad.cpu().numpy().astype(np.float64)))
        if world == 2:
            nt = len(inp["t"][rank::2])
            assert cc.shape[0] == nt and cc.aux[0].numel() == cc.aux[1].numel() == nt * cc.shape[1] * cc.shape[2]
    (l, g), (l0, g0), (l1, g1) = res
    print(f"[{dev}] slabs: loss rel {abs(l0 + l1 - l) / l:.2e}, grad rel-L2 {rel(g0 + g1, g):.2e}")
    assert abs(l0 + l1 - l) <= 1e-6 * l
    assert rel(g0 + g1, g) <= 1e-6


def test_learning(dev, tmp_path):
    """From case G's weights, 30 Adam steps through Solver lose at least half of what the reference's float64 run loses
    (the criterion of tests/test_lno_examples.py)."""
    ref = G["G/train_loss"]
    model, csts, solver = _case_g(tmp_path, iters_per_epoch=30, log_freq=30)
    ccs = bind_all(solver, csts)
    solver.engine.forward_backward(ccs)
    l0 = sum(cc.loss() for cc in ccs)
    solver.train()
    solver.engine.forward_backward(ccs)
    l30 = sum(cc.loss() for cc in ccs)
    print(f"[{dev}] learning: {l0:.6f} -> {l30:.6f}; reference {ref[0]:.6f} -> {ref[30]:.6f}; ratio {(l0 - l30) / (ref[0] - ref[30]):.4f}")
    assert l0 == pytest.approx(float(ref[0]), rel=3e-5)
    assert l0 - l30 >= 0.5 * (ref[0] - ref[30])
