"""PCGrad / Relobralo / AGDA (ppsci.loss.mtl): parity with fixtures recorded from the reference's own code
(tests/golden/mtl.npz, make_mtl_golden.py), and through the Solver against the fp64 oracle (per-term gradients by autograd through
the restated reference network, then PCGrad's projections on the vectors / Relobralo's rule restated here), on the net and data of
tests/test_loss_aggregators.py with a third, conflicting loss key."""
import itertools
import os

import numpy as np
import pytest
import torch

import ppsci
from oracle import ref_torch as R
from oracle import taylor_np as T
from paddlescience_amd import device
from paddlescience_amd import hotpath as hp
from ppsci.autodiff import jacobian
from tests.common import make_dev_fixture, set_model_weights
from tests.test_grad_surgery_kernels import EPS32, _gram_c, _rule_tol, ref_rule

dev = make_dev_fixture()
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mtl.npz"))
KEYS = ("laplace", "u", "ux")


# ------------------------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("beta,tau", [(0.0, 1.0), (0.0, 0.1), (1.0, 1.0), (1.0, 0.1)])
def test_relobralo_rule_matches_reference_fixture(beta, tau):
    tag = f"relobralo/beta{beta:g}_tau{tau:g}"
    seq = GOLD[tag + "/losses"]
    agg = ppsci.loss.mtl.Relobralo(3, alpha=0.95, beta=beta, tau=tau)
    for step in range(len(seq)):
        total = agg({f"l{k}": float(seq[step, k]) for k in range(3)}, step)
        np.testing.assert_allclose(agg.lmbda, GOLD[tag + "/lmbda"][step], rtol=1e-6)
        np.testing.assert_allclose(total, GOLD[tag + "/total"][step], rtol=1e-6)
        np.testing.assert_array_equal(agg.weights(), np.ones(3) if step == 0 else agg.lmbda)
    np.testing.assert_allclose(agg.losses_init, GOLD[tag + "/losses_init"], rtol=1e-7)
    np.testing.assert_allclose(agg.losses_prev, GOLD[tag + "/losses_prev"], rtol=1e-7)


def test_pcgrad_kernels_match_reference_fixture(dev):
    """The surgery + combine kernels on the fixture's vectors, for all six orders, against what the reference's _refine_grads
    returned.  Gram, C / w and the combination each under the bound of tests/test_grad_surgery_kernels.py; the end result under
    the same error pushed through the rule: a Gram entry off by (c eps32 sum|ab|) moves a projection coefficient by at most
    that over Gram[k][k] (rho below), the K updates of a row amplify it by ((1 + R)^K - 1) like the rule's own rounding."""
    d = device.get_device()
    g32, orders, ref_out = GOLD["pcgrad/G"], GOLD["pcgrad/orders"], GOLD["pcgrad/out"]
    K, n = g32.shape
    g64 = g32.astype(np.float64)
    gram64 = g64 @ g64.T
    absdot = (np.abs(g64)[:, None, :] * np.abs(g64)[None, :, :]).sum(-1)
    G = torch.tensor(g32, device=d)
    ws = torch.zeros(hp.grad_surgery_workspace_bytes(K, n) // 4, dtype=torch.int32, device=d)
    gram, coef, w, out = (torch.zeros(m, device=d) for m in (K * K, K * K, K, n))
    outs = []
    for order, ref in zip(orders, ref_out):
        # the fp64 rule on the fp64 Gram IS the reference's algorithm
        C64, w64 = ref_rule(gram64, list(order))
        np.testing.assert_allclose(w64 @ g64, ref, rtol=0, atol=1e-12)
        hp.grad_surgery(G, gram, ws, [int(o) for o in order], coef, w)
        hp.grad_combine(G, out, w_dev=w)
        got = gram.cpu().numpy().astype(np.float64).reshape(K, K)
        assert (np.abs(got - gram64) <= _gram_c(n) * EPS32 * absdot).all()
        C_ref, w_ref = ref_rule(got, list(order))
        tc, tw = _rule_tol(got, list(order))
        assert (np.abs(coef.cpu().numpy().reshape(K, K) - C_ref) <= tc).all() and (np.abs(w.cpu().numpy() - w_ref) <= tw).all()
        tw = tw.max()
        A = np.abs(C64).max()
        Rr = max(np.abs(gram64[:, k]).max() / gram64[k, k] for k in range(K))
        rho = max(absdot[:, k].max() / gram64[k, k] for k in range(K))
        w_tol = tw + K * K * A * ((1 + Rr) ** K - 1) * _gram_c(n) * EPS32 * rho
        o = out.cpu().numpy().astype(np.float64)
        bound = w_tol * np.abs(g64).sum(0) + (K + 1) * EPS32 * (np.abs(w64)[:, None] * np.abs(g64)).sum(0)
        print(f"order {order}: max err {np.abs(o - ref).max():.2e}, bound min {bound.min():.2e}")
        assert (np.abs(o - ref) <= bound).all()
        outs.append(o)
    assert max(np.abs(a - b).max() for a, b in itertools.combinations(outs, 2)) > 1e-2  # the order matters


# ------------------------------------------------------------------------------------------------ through the Solver
def _setup(tmp_path, agg_factory, opt_factory=None, epochs=4, model_factory=None, **solver_kw):
    net = T.make_net(2, [16, 16], 1, bias_scale=0.1)
    if model_factory is None:
        model = ppsci.arch.MLP(("x", "y"), ("u",), 2, 16, "tanh")
        set_model_weights(model, net)
    else:
        model = model_factory()
    N = 40
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, (N, 2)).astype(np.float32)
    lab_u = (np.cos(X[:, :1]) * np.cosh(X[:, 1:])).astype(np.float32)
    eq = ppsci.equation.Laplace(dim=2)
    cfg = {"dataset": {"name": "IterableNamedArrayDataset", "input": {"x": X[:, :1], "y": X[:, 1:]},
                       "label": {"laplace": np.zeros((N, 1), np.float32), "u": lab_u, "ux": np.full((N, 1), -2.0, np.float32)}}}
    exprs = {**eq.equations, "u": lambda out: out["u"], "ux": lambda out: jacobian(out["u"], out["x"])}
    cst = ppsci.constraint.SupervisedConstraint(cfg, ppsci.loss.MSELoss("mean"), exprs, name="EQ")
    opt = (opt_factory or (lambda m: ppsci.optimizer.Adam(1e-3)(m)))(model)
    agg = agg_factory(model)
    solver = ppsci.solver.Solver(model, {"EQ": cst}, str(tmp_path), opt, epochs=epochs, iters_per_epoch=1, log_freq=1,
                                 loss_aggregator=agg, **solver_kw)
    return solver, model, net, X, lab_u, agg


@pytest.fixture
def shuffle_log(monkeypatch):
    """np.random.shuffle, recording what every call left behind (PCGrad draws one per step)."""
    log, real = [], np.random.shuffle

    def recording(x):
        real(x)
        log.append(list(x))

    monkeypatch.setattr(np.random, "shuffle", recording)
    return log


def _oracle(net, X, lab_u, combine, steps=4):
    """fp64: per-term gradients at the current parameters, `combine(step, losses, grads) -> total gradient`, Adam."""
    omodel = R.MLP(("x", "y"), ("u",), net.astype(np.float32).astype(np.float64))
    params = list(omodel.parameters())
    flat = np.concatenate([p.detach().numpy().ravel() for p in params])
    adam = R.Adam(flat.size, 1e-3)
    x = {"x": torch.tensor(X[:, :1].astype(np.float64), requires_grad=True),
         "y": torch.tensor(X[:, 1:].astype(np.float64), requires_grad=True)}
    for step in range(steps):
        out = omodel(x)
        ux = torch.autograd.grad(out["u"].sum(), x["x"], create_graph=True)[0]
        uy = torch.autograd.grad(out["u"].sum(), x["y"], create_graph=True)[0]
        lap = torch.autograd.grad(ux.sum(), x["x"], create_graph=True)[0] + torch.autograd.grad(uy.sum(), x["y"], create_graph=True)[0]
        terms = [(lap ** 2).mean(), ((out["u"] - torch.tensor(lab_u.astype(np.float64))) ** 2).mean(), ((ux + 2.0) ** 2).mean()]
        gs = [np.concatenate([(torch.zeros_like(p) if g is None else g).numpy().ravel() for g, p in
                              zip(torch.autograd.grad(t, params, retain_graph=True, allow_unused=True), params)]) for t in terms]
        flat = adam.step(flat, combine(step, np.array([float(t.detach()) for t in terms]), gs))
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                p.copy_(torch.from_numpy(flat[off:off + k].reshape(p.shape)))
                off += k
    return flat


def _pcgrad_combine(orders):
    def combine(step, losses, gs):
        order = [KEYS.index(k) for k in orders[step]]
        gram = np.array([[a @ b for b in gs] for a in gs])
        assert (gram[np.triu_indices(3, 1)] < 0).any(), "no conflict in this step: it would test nothing"
        total = np.zeros_like(gs[0])
        for i in order:  # pcgrad.py:94-104 on the vectors
            gi = gs[i].copy()
            for k in order:
                gi = gi - min((gi @ gs[k]) / (gs[k] @ gs[k]), 0.0) * gs[k]
            total += gi
        return total

    return combine


class _RelobraloOracle:
    """relobralo.py:100-125 restated with rho fixed to beta (beta in {0, 1}: paddle.bernoulli is deterministic there)."""

    def __init__(self, beta, alpha=0.95, tau=1.0, eps=1e-8):
        self.beta, self.alpha, self.tau, self.eps = beta, alpha, tau, eps
        self.lmbda = np.ones(3)

    def bal(self, a, b):
        z = a / (self.tau * b + self.eps)
        e = np.exp(z - z.max())
        return 3 * e / e.sum()

    def __call__(self, step, L, gs):
        if step == 0:
            self.init, w = L.copy(), np.ones(3)
        else:
            hist = self.beta * self.lmbda + (1 - self.beta) * self.bal(L, self.init)
            self.lmbda = w = self.alpha * hist + (1 - self.alpha) * self.bal(L, self.prev)
        self.prev = L.copy()
        self.total = float((w * L).sum())
        return sum(wk * g for wk, g in zip(w, gs))


def test_pcgrad_through_solver_matches_oracle(dev, tmp_path, shuffle_log):
    np.random.seed(0)
    solver, model, net, X, lab_u, agg = _setup(tmp_path, ppsci.loss.mtl.PCGrad)
    solver.train()
    assert len(shuffle_log) == 4 and all(sorted(o) == sorted(KEYS) for o in shuffle_log)
    flat = _oracle(net, X, lab_u, _pcgrad_combine(shuffle_log))
    np.testing.assert_allclose(model.flat_params.cpu().numpy(), flat, rtol=0, atol=3e-5)
    # the logged total is the plain sum of the raw terms; the per-constraint entry is their sum too
    assert set(solver.last_losses) == {"loss", "EQ"}
    np.testing.assert_allclose(solver.last_losses["loss"], solver.last_losses["EQ"], rtol=1e-6)
    assert not ppsci.loss.mtl.PCGrad.should_persist


@pytest.mark.parametrize("beta", [1.0, 0.0])
def test_relobralo_through_solver_matches_oracle(beta, dev, tmp_path):
    solver, model, net, X, lab_u, agg = _setup(tmp_path, lambda m: ppsci.loss.mtl.Relobralo(3, beta=beta))
    solver.train()
    orc = _RelobraloOracle(beta)
    flat = _oracle(net, X, lab_u, orc)
    np.testing.assert_allclose(agg.lmbda, orc.lmbda, rtol=2e-4)
    np.testing.assert_allclose(model.flat_params.cpu().numpy(), flat, rtol=0, atol=3e-5)
    # logged: sum_k lambda_k L_k of the last step; the per-constraint entry stays the raw sum
    np.testing.assert_allclose(solver.last_losses["loss"], orc.total, rtol=2e-4)
    np.testing.assert_allclose(solver.last_losses["EQ"], orc.prev.sum(), rtol=2e-4)


def test_relobralo_first_step_logs_the_plain_sum(dev, tmp_path):
    solver, *_ = _setup(tmp_path, lambda m: ppsci.loss.mtl.Relobralo(3, beta=1.0), epochs=1)
    solver.train()
    np.testing.assert_allclose(solver.last_losses["loss"], solver.last_losses["EQ"], rtol=1e-6)


def test_reparametrised_rows_sum_to_the_plain_step(dev, tmp_path):
    """Factored layers (random_weight): the rows of the matrix are the PULLED-BACK per-key gradients and the combination lands in
    a buffer of its own.  Relobralo's first step weights every row with 1, so it must be the Sum step: the sum of the pulled-back
    rows against the pull-back of the summed gradient (linear, so equal up to fp32 summation order: a relative d of a few eps32,
    below 1e-6).  Adam's first step moves a parameter by lr g / (|g| + eps), which such a d changes by at most lr d = 1e-9; the
    rest of atol is the rounding of the parameter itself, an ulp of a value below 2: 1.2e-7."""
    def rwf():
        ppsci.utils.misc.set_random_seed(11)
        return ppsci.arch.MLP(("x", "y"), ("u",), 2, 16, "tanh", random_weight={"mean": 0.5, "std": 0.1})

    res = []
    for fac in (lambda m: ppsci.loss.mtl.Sum(), lambda m: ppsci.loss.mtl.Relobralo(3, beta=1.0)):
        solver, model, *_ = _setup(tmp_path, fac, epochs=1, model_factory=rwf)
        assert solver._reparam
        p0 = model.flat_params.cpu().numpy().copy()
        solver.train()
        res.append(model.flat_params.cpu().numpy().copy())
    assert solver._mtl["out"].data_ptr() != solver.engine.grad.data_ptr()
    np.testing.assert_allclose(res[1], res[0], rtol=0, atol=1e-9 + 1.2e-7)
    assert np.abs(res[0] - p0).max() > 5e-4
    # PCGrad on the same model: the fused Adam of grad_combine and optimizer.step agree on the trainable buffer too
    out = []
    for fac in (None, lambda m: ppsci.optimizer.AdamW(1e-3, weight_decay=0.0)(m)):
        np.random.seed(0)
        solver, model, *_ = _setup(tmp_path, ppsci.loss.mtl.PCGrad, fac, epochs=2, model_factory=rwf)
        solver.train()
        out.append(model.flat_params.cpu().numpy().copy())
    np.testing.assert_allclose(out[0], out[1], rtol=0, atol=1e-6)
    assert np.abs(out[0] - p0).max() > 5e-4


def test_fused_adam_and_optimizer_step_agree(dev, tmp_path):
    """grad_combine applies a plain Adam itself; any other optimizer takes the combined gradient through optimizer.step.
    AdamW without decay is the same update up to (a) the bias corrections -- ppsci_adam_step forms them from the float32 betas,
    AdamW from the Python floats: 1 - beta2 differs by a relative 1.3e-5, a step of at most lr = 1e-3 by 1.3e-8 -- and (b) the
    rounding of the update itself, which the AdamW kernel does not pin to one fmaf form: an ulp of a parameter below 2 in
    magnitude, 2.4e-7.  Four steps: atol = 4 (1.3e-8 + 2.4e-7) = 1e-6."""
    res = []
    for fac in (None, lambda m: ppsci.optimizer.AdamW(1e-3, weight_decay=0.0)(m)):
        np.random.seed(0)
        solver, model, *_ = _setup(tmp_path, ppsci.loss.mtl.PCGrad, fac)
        solver.train()
        assert solver.optimizer.t == 4
        res.append(model.flat_params.cpu().numpy().copy())
    np.testing.assert_allclose(res[0], res[1], rtol=0, atol=1e-6)
    assert np.abs(res[0] - T.flat_params(T.make_net(2, [16, 16], 1, bias_scale=0.1)).astype(np.float32)).max() > 1e-3


def test_no_fast_path_under_pcgrad(dev, tmp_path, monkeypatch):
    """The one-launch step (forward -> loss -> backward -> Adam in one kernel) has no place for per-loss gradients: with Sum the
    Solver takes it on this configuration, with PCGrad it does not, and no engine launch carries the optimizer."""
    from paddlescience_amd.engine import Engine
    from paddlescience_amd.solver.solver import Solver

    taken, adams = [], []
    real_fast, real_launch = Solver._step_in_one_launch, Engine.step_one_launch
    monkeypatch.setattr(Solver, "_step_in_one_launch", lambda self, *a: taken.append(real_fast(self, *a)) or taken[-1])
    monkeypatch.setattr(Engine, "step_one_launch", lambda self, c, adam=None: adams.append(adam) or real_launch(self, c, adam))
    solver, *_ = _setup(tmp_path / "sum", lambda m: ppsci.loss.mtl.Sum(), epochs=2)
    solver.train()
    assert taken == [True, True] and all(a is not None for a in adams)
    del taken[:], adams[:]
    solver, *_ = _setup(tmp_path / "pcgrad", ppsci.loss.mtl.PCGrad, epochs=2)
    solver.train()
    assert not any(taken) and all(a is None for a in adams)
    assert solver._step_in_one_launch([c.fused for c in solver._compiled.values()], 1.0) is False


def test_relobralo_checkpoint_round_trip(dev, tmp_path):
    fac = lambda m: ppsci.loss.mtl.Relobralo(3, beta=0.0, tau=0.5)  # noqa: E731
    assert ppsci.loss.mtl.Relobralo.should_persist
    full, m_full, *_, agg_full = _setup(tmp_path / "full", fac, epochs=4)
    full.train()
    part, *_, agg_part = _setup(tmp_path / "part", fac, epochs=2, save_freq=1)
    part.train()
    ck = os.path.join(str(tmp_path / "part"), "checkpoints", "epoch_2")
    res, m_res, *_, agg_res = _setup(tmp_path / "part", fac, epochs=4, checkpoint_path=ck)
    for k in ("losses_init", "losses_prev", "lmbda"):
        np.testing.assert_array_equal(getattr(agg_res, k), getattr(agg_part, k))
        assert set(agg_res.state_dict()) == {"losses_init", "losses_prev", "lmbda"}
    assert not np.array_equal(agg_res.lmbda, np.ones(3))
    res.train()
    np.testing.assert_array_equal(m_res.flat_params.cpu().numpy(), m_full.flat_params.cpu().numpy())
    np.testing.assert_array_equal(agg_res.lmbda, agg_full.lmbda)


# ------------------------------------------------------------------------------------------------ what is not built raises
def test_refusals(dev, tmp_path):
    from paddlescience_amd.equation.pde.base import EqParamStore

    PCGrad, Relobralo = ppsci.loss.mtl.PCGrad, ppsci.loss.mtl.Relobralo
    with pytest.raises(NotImplementedError, match="Lf_smooth_kM"):
        ppsci.loss.mtl.AGDA(None)
    spinn = ppsci.arch.SPINN(("x", "y", "z"), ("u",), r=4, num_layers=2, hidden_size=16, activation="tanh")
    with pytest.raises(NotImplementedError, match="fused PINN engine"):
        ppsci.solver.Solver(spinn, None, str(tmp_path), loss_aggregator=PCGrad(spinn))
    fno = ppsci.arch.TFNO2dNet(("x",), ("y",), 4, 4, hidden_channels=8, lifting_channels=16, projection_channels=16, n_layers=2)
    with pytest.raises(NotImplementedError, match="fused PINN engine"):
        ppsci.solver.Solver(fno, None, str(tmp_path), loss_aggregator=Relobralo(2))
    with pytest.raises(NotImplementedError, match="L-BFGS"):
        _setup(tmp_path, PCGrad, lambda m: ppsci.optimizer.LBFGS()(m))
    with pytest.raises(NotImplementedError, match="update_freq > 1"):
        _setup(tmp_path, lambda m: Relobralo(3), update_freq=2)
    EqParamStore.reset()
    try:
        model = ppsci.arch.MLP(("t_f",), ("eta",), 2, 16, "tanh")
        eq = ppsci.equation.Vibration(1.5, 0.3, -0.2)
        opt = ppsci.optimizer.Adam(1e-3)((model, eq))
        with pytest.raises(NotImplementedError, match="learnable equation parameters"):
            ppsci.solver.Solver(model, None, str(tmp_path), opt, equation={"VIV": eq}, loss_aggregator=PCGrad(model))
    finally:
        EqParamStore.reset()
