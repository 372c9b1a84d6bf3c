"""ppsci.equation.FractionalPoisson (/root/reference/ppsci/equation/fpde/fractional_poisson.py) and what it runs on:

  * the host restatement against the reference's own arrays (tests/golden/fpde.npz, tests/golden/make_fpde_golden.py);
  * ppsci_csr_matvec (csrc/coupling.hip) against numpy, on the emulator and the device;
  * the coupled step of the fPINN example through Solver: loss and parameter gradient against float64 autograd of the same
    sparse residual; at N = 2000 (1.38 M auxiliary points, where a dense matrix would need 11 GB) also bitwise repeatable;
  * dataset `transforms` configs (FunctionalTransform), which the example builds its batch with.

The residual of the fractional Laplacian is a difference of terms up to ~10^4 times larger than itself (Grünwald–Letnikov
weights times h^-α, h ~ 1 / resolution[-1]): at resolution [8, 100] merely evaluating the network in float32 instead of
float64 moves the loss by up to 1e-5, the kernels' float32 by several 1e-5.  Where that is so, the float64 comparisons allow
a multiple of the spread that a float32 evaluation of the same reference shows (_check_step), and the tolerances of the Volterra test
(test_batch_reductions.test_volterra_coupled_residual_matches_autograd) otherwise."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import ppsci
from tests.common import make_dev_fixture, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fpde.npz")
CASES = {"a18_r8x100": (1.8, [8, 100]), "a18_r4x20": (1.8, [4, 20]), "a05_r8x100": (0.5, [8, 100]), "a05_r4x20": (0.5, [4, 20])}

dev = make_dev_fixture()


# ---- the host restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_points_and_matrix_match_the_reference(case):
    z = np.load(GOLD)
    alpha, res = CASES[case]
    grid = "r" + "x".join(map(str, res))
    eq = ppsci.equation.FractionalPoisson(alpha, ppsci.geometry.Disk((0, 0), 1), res)
    tx = eq.get_x(z["x0"])
    assert eq.get_x(z["x0"] + 0.01) is tx  # cached, as in the reference
    xs = np.concatenate([tx["x"], tx["y"]], 1)
    ref_x = z[f"{grid}_x"]
    assert xs.shape == ref_x.shape
    assert np.all(np.abs(xs - ref_x) <= 1e-6 * np.maximum(np.abs(ref_x), 1e-30) + 1e-12)
    M = eq.int_mat
    assert M.shape == tuple(z[f"{grid}_shape"])
    assert np.array_equal(M.row_of_entries(), z[f"{grid}_rows"]) and np.array_equal(M.col_idx, z[f"{grid}_cols"])
    assert np.all(np.abs(M.vals - z[f"{case}_vals"]) <= 1e-6 * np.abs(z[f"{case}_vals"]))
    # the residual of the exact solution: a cancellation, compared on the scale of its terms (the reference sums in float32)
    u = (np.abs(1 - (xs ** 2).sum(1, keepdims=True)) ** (1 + alpha / 2)).astype(np.float32)
    r = eq.equations["fpde"]({"x": tx["x"], "y": tx["y"], "u": u})
    ref = z[f"{case}_resid"]
    assert r.shape == ref.shape == (len(z["x0"]),)
    terms = abs(eq._factor()) * np.bincount(M.row_of_entries(), np.abs(M.vals.astype(np.float64) * u[M.col_idx, 0]))
    assert np.all(np.abs(r - ref) <= 1e-5 * terms), np.max(np.abs(r - ref) / terms)
    # tensors: the same value, differentiable
    ut = torch.tensor(u.astype(np.float64), requires_grad=True)
    rt = eq.equations["fpde"]({"x": torch.tensor(tx["x"]).double(), "y": torch.tensor(tx["y"]).double(), "u": ut})
    assert np.all(np.abs(rt.detach().numpy() - ref) <= 1e-5 * terms)
    rt.sum().backward()
    assert ut.grad is not None and float(ut.grad.abs().sum()) > 0


def test_what_is_refused_says_why():
    disk = ppsci.geometry.Disk((0, 0), 1)
    with pytest.raises(NotImplementedError, match="2-D Disk"):
        ppsci.equation.FractionalPoisson(1.8, ppsci.geometry.Rectangle((0, 0), (1, 1)), [8, 100])
    eq = ppsci.equation.FractionalPoisson(1.8, disk, [4, 20])
    with pytest.raises(ValueError, match="boundary"):
        eq.get_x(np.array([[0.1, 0.2], [1.0, 0.0]], np.float32))


# ---- the kernel ----------------------------------------------------------------------------------------------------------
def _csr(rng, rows, cols, lengths):
    from paddlescience_amd import graph

    ptr = np.zeros(rows + 1, np.int64)
    np.cumsum(lengths, out=ptr[1:])
    return graph.CsrMatrix(ptr, rng.integers(0, cols, int(ptr[-1])), rng.standard_normal(int(ptr[-1])).astype(np.float32),
                           (rows, cols))


def _dense(M):
    D = np.zeros(M.shape)
    np.add.at(D, (M.row_of_entries(), M.col_idx), M.vals.astype(np.float64))
    return D


def test_csr_matvec_against_numpy(dev):
    from paddlescience_amd import hotpath as hp

    d = "cpu" if dev == "emu" else "cuda"
    rng = np.random.default_rng(7)
    # long rows (a wave per row): empty rows, single entries, a row longer than 64 x 4, rows around the wave width
    lengths = rng.integers(0, 90, 41)
    lengths[[0, 5, 40]] = 0
    lengths[[3, 17]] = 1
    lengths[11] = 300
    lengths[12] = 64
    long_ = _csr(rng, 41, 500, lengths)
    assert long_.nnz >= 16 * 41
    short = long_.transpose()  # ~1 entry per row, many empty rows (the thread-per-row variant)
    assert short.nnz < 16 * short.shape[0] and np.any(np.diff(short.row_ptr) == 0)
    for M in (long_, short):
        rows, cols = M.shape
        x = rng.standard_normal(cols).astype(np.float32)
        s = rng.uniform(0.5, 2.0, cols).astype(np.float32)
        t = lambda a: torch.as_tensor(a).to(d)  # noqa: E731
        args = (t(M.row_ptr), t(M.col_idx), t(M.vals), cols)
        for xscale in (None, s):
            y1 = torch.full((rows + 3,), 7.0, device=d)
            y2 = torch.full((rows + 3,), 7.0, device=d)
            hp.csr_matvec(*args, x=t(x), y=y1, alpha=-0.37, xscale=None if xscale is None else t(xscale))
            hp.csr_matvec(*args, x=t(x), y=y2, alpha=-0.37, xscale=None if xscale is None else t(xscale))
            want = -0.37 * (_dense(M) @ (x.astype(np.float64) * (1.0 if xscale is None else xscale)))
            got = y1.cpu().numpy()
            assert np.allclose(got[:rows], want, rtol=1e-5, atol=1e-5 * np.abs(want).max()), np.abs(got[:rows] - want).max()
            assert np.all(got[rows:] == 7.0)  # nothing written behind the last row
            assert torch.equal(y1, y2)  # bitwise repeatable


def test_csr_matvec_refuses_bad_arguments(dev):
    import ctypes

    from paddlescience_amd import _lib as L

    d = "cpu" if dev == "emu" else "cuda"
    ptr = torch.tensor([0, 1], dtype=torch.int32, device=d)
    col = torch.tensor([0], dtype=torch.int32, device=d)
    val = torch.ones(1, device=d)
    x, y = torch.ones(1, device=d), torch.zeros(1, device=d)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    f = L.lib().ppsci_csr_matvec
    ok = (1, 1, 1, p(ptr), p(col), p(val), p(x), None, 1.0, p(y), None)
    assert f(*ok) == 0
    bad = [(0,) + ok[1:], ok[:1] + (0,) + ok[2:], ok[:2] + (-1,) + ok[3:], ok[:2] + (1 << 31,) + ok[3:],
           ok[:1] + (1 << 31,) + ok[2:], ok[:3] + (None,) + ok[4:], ok[:4] + (None,) + ok[5:], ok[:5] + (None,) + ok[6:],
           ok[:6] + (None,) + ok[7:], ok[:9] + (None,) + ok[10:]]
    for args in bad:
        assert f(*args) == -1  # PPSCI_E_INVALID
        assert b"csr_matvec" in L.lib().ppsci_last_error()


def test_csr_matrix_checks_its_indices():
    from paddlescience_amd import graph

    with pytest.raises(ValueError, match="column index"):
        graph.CsrMatrix([0, 1], [3], [1.0], (1, 3))
    with pytest.raises(ValueError, match="row_ptr"):
        graph.CsrMatrix([0, 2, 1], [0, 1], [1.0, 2.0], (2, 3))


# ---- the coupled step through Solver --------------------------------------------------------------------------------------
def _example(tmp_path, **over):
    sys.path.insert(0, ROOT)
    from examples import fractional_poisson_2d as ex

    cfg = dict(ex.DEFAULTS, output_dir=str(tmp_path), log_freq=10 ** 6, eval_during_train=False, plot=False)
    cfg.update(over)
    return ex, cfg, ex.build(cfg)


def _ref_loss_grad(model, eq, batch, n, dtype, device="cpu"):
    """The reference's FPDE loss  mean((c (M u)[:N] - rhs)^2)  by autograd in `dtype` (u from the same weights, the output
    transform applied), with the sparse product as a gather-scatter over the matrix's COO entries."""
    ps = [p.detach().to(device=device, dtype=dtype) for p in model.parameters()]
    for p in ps:
        p.requires_grad_(True)
    X = torch.tensor(np.concatenate([batch["x"], batch["y"]], 1), dtype=dtype, device=device)
    h = X
    for i in range(0, len(ps) - 2, 2):
        h = torch.tanh(h @ ps[i] + ps[i + 1])
    u = (1 - (X[:, :1] ** 2 + X[:, 1:] ** 2)) * (h @ ps[-2] + ps[-1])
    M = eq.int_mat
    rows = torch.tensor(M.row_of_entries(), device=device)
    cols = torch.tensor(M.col_idx.astype(np.int64), device=device)
    Mu = torch.zeros(n, dtype=dtype, device=device).index_add_(0, rows, torch.tensor(M.vals, device=device).to(dtype) * u[cols, 0])
    a = eq.alpha
    k = 2 ** a * math.gamma(2 + a / 2) * math.gamma(1 + a / 2)
    r = eq._factor() * Mu - k * (1 - (1 + a / 2) * (X[:n] ** 2).sum(1))
    loss = (r * r).mean()
    grad = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, ps)])
    return float(loss.detach()), grad.detach().cpu().numpy().astype(np.float64)


def _check_step(solver, eq, n, monkeypatch, tol_loss=2e-5, tol_grad=5e-5, ref_device="cpu"):
    from paddlescience_amd import hotpath as hp

    calls = []
    real = hp.csr_matvec
    monkeypatch.setattr(hp, "csr_matvec", lambda *a, **k: (calls.append(k.get("xscale") is not None), real(*a, **k))[1])
    cc = solver._compiled["FPDE"]
    assert cc.low.couplings and any("fractional_poisson_matrix" in s for s in cc.specialised_to)
    (it,), (M,) = cc.low.couplings.items, cc.fused.couplings["M"]
    # the sparse path: device CSR of M and M^T, no dense [N, batch] matrix anywhere
    assert isinstance(M, dict) and M["M"]["vals"].numel() == eq.int_mat.nnz == M["MT"]["vals"].numel()
    # the host matrix went to the device and was let go: no record of the constraint still holds it
    assert it.matrix is None and all(c.matrix is None for c in cc.fused.couplings["items"])
    for m, dev_m in ((eq.int_mat, M["M"]), (eq.int_mat.transpose(), M["MT"])):
        for f in ("row_ptr", "col_idx", "vals"):
            assert np.array_equal(dev_m[f].cpu().numpy(), getattr(m, f)), f
    big = [t for t in list(M["M"].values()) + list(M["MT"].values()) if isinstance(t, torch.Tensor)]
    assert all(t.numel() < n * it.cols for t in big)
    solver.engine.forward_backward([cc.fused])
    assert sorted(set(calls)) == [False, True]  # forward product and the transposed one, both through ppsci_csr_matvec
    loss = cc.fused.losses()["fpde"]
    grad = solver.engine.grad.detach().cpu().numpy().astype(np.float64)
    batch = eq.train_x
    l64, g64 = _ref_loss_grad(solver.model, eq, batch, n, torch.float64, ref_device)
    l32, g32 = _ref_loss_grad(solver.model, eq, batch, n, torch.float32, ref_device)
    # the kernels evaluate the network in float32 in an order of their own (a few ulps from torch's), which the stencil
    # amplifies like the rounding itself: 16x the spread of torch's float32 evaluation (measured 9x at N = 100, [8, 100])
    tl = max(tol_loss, 16 * abs(l32 / l64 - 1.0))
    tg = max(tol_grad, 16 * rel(g32, g64))
    assert abs(loss / l64 - 1.0) < tl, (loss, l64, tl)
    assert rel(grad, g64) < tg, (rel(grad, g64), tg)
    return cc, loss, grad


def test_fpde_step_matches_autograd(dev, tmp_path, monkeypatch):
    n, res = (12, [4, 20]) if dev == "emu" else (100, [8, 100])
    ex, cfg, solver = _example(tmp_path, NPOINT_INTERIOR=n, resolution=res, epochs=1)
    eq = solver.equation["fpde"]
    assert len(eq.train_x["x"]) > 20 * n
    _check_step(solver, eq, n, monkeypatch, ref_device="cpu" if dev == "emu" else "cuda")
    # a batch that is not the one get_x() built is refused at trace time
    other = ppsci.equation.FractionalPoisson(cfg["ALPHA"], ppsci.geometry.Disk((0, 0), 1), res)
    other.get_x(np.array([[0.1, 0.2], [-0.3, 0.4]], np.float32))
    cst = ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "IterableNamedArrayDataset", "input": dict(eq.train_x), "label": {"fpde": np.zeros((n, 1), np.float32)}},
         "batch_size": len(eq.train_x["x"]), "iters_per_epoch": 1},
        ppsci.loss.MSELoss("mean"), other.equations, name="FPDE")
    with pytest.raises(ValueError, match="not the one get_x"):
        ppsci.solver.Solver(solver.model, {"FPDE": cst}, str(tmp_path / "o"), ppsci.optimizer.Adam(1e-3)(solver.model), epochs=1,
                            iters_per_epoch=1)


# ---- dataset transforms --------------------------------------------------------------------------------------------------
def test_dataset_transform_configs():
    from paddlescience_amd.data import dataset

    inp = {"x": np.arange(4, dtype=np.float32).reshape(4, 1)}
    lab = {"u": np.ones((4, 1), np.float32)}

    def grow(i, l, w):
        i["x"] = np.concatenate([i["x"], i["x"] + 10])
        w["u"] = 0.5
        return i, l, w

    ds = dataset.build_dataset({"name": "IterableNamedArrayDataset", "input": dict(inp), "label": lab,
                                "transforms": ({"FunctionalTransform": {"transform_func": grow}},)})
    assert isinstance(ds.transforms, ppsci.data.transform.Compose)
    i, l, w = next(iter(ds))
    assert i["x"].shape == (8, 1) and float(i["x"][-1, 0]) == 13.0 and w == {"u": 0.5}
    assert ds.input["x"].shape == (4, 1)  # the transform worked on copies
    # a callable passes through unchanged
    f = ppsci.data.transform.FunctionalTransform(grow)
    ds2 = dataset.build_dataset({"name": "NamedArrayDataset", "input": dict(inp), "label": lab, "transforms": f})
    assert ds2.transforms is f
    assert ds2[np.arange(2)][0]["x"].shape == (4, 1)
    # any other transform raises, naming it
    with pytest.raises(NotImplementedError, match="Scale"):
        dataset.build_dataset({"name": "NamedArrayDataset", "input": dict(inp), "label": lab,
                               "transforms": [{"Scale": {"scale": {"x": 2.0}}}]})
