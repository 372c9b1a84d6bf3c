"""ppsci.arch.DeepONet / HEDeepONets / ChipDeepONets (arch/deeponet.py) on the layer-by-layer path and the head kernels of
csrc/pirate.hip, on the CPU SIMT emulator and (-m gpu) on the device:

  * parity with tests/golden/deeponet.npz, produced by the reference's own model code in float64: every output stream
    (value, first and second derivatives along the trunk keys) and the gradient of a fixed cotangent contraction with
    respect to every parameter;
  * parameter names / order, state-dict round trip, the unused registered activations under Adam, predict shapes and the
    NotImplementedError envelope;
  * ppsci_onet_pack / ppsci_onet_head_fwd / _bwd through ctypes against numpy (J = 1, 2, 3; S = 1, 3, 5; N not a multiple
    of 16), and a finite-difference check of the swish beta gradient."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ppsci
from paddlescience_amd import _lib as L
from paddlescience_amd import hotpath as hp
from paddlescience_amd.arch import deeponet as D
from tests.common import make_dev_fixture, rel

dev = make_dev_fixture()

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeponet.npz")

CASES = {
    "deeponet_tanh": ("DeepONet", dict(u_key="u", y_key="y", G_key="G", num_loc=100, num_features=16, branch_num_layers=2,
                                       trunk_num_layers=2, branch_hidden_size=32, trunk_hidden_size=32,
                                       branch_activation="tanh", trunk_activation="tanh"), 2),
    "he_swish": ("HEDeepONets", dict(heat_input_keys=("qm_h",), cold_input_keys=("qm_c",), trunk_input_keys=("x", "t"),
                                     output_keys=("T_h", "T_c", "T_w"), heat_num_loc=1, cold_num_loc=1, num_features=8,
                                     branch_num_layers=2, trunk_num_layers=3, branch_hidden_size=32, trunk_hidden_size=32,
                                     branch_activation="swish", trunk_activation="swish"), 1),
    "chip_swish": ("ChipDeepONets", dict(branch_input_keys=("u",), BCtype_input_keys=("bctype",), BC_input_keys=("bc",),
                                         trunk_input_keys=("x", "y"), output_keys=("T",), num_loc=12, bctype_loc=1,
                                         BC_num_loc=6, num_features=12, branch_num_layers=2, BC_num_layers=2,
                                         trunk_num_layers=2, branch_hidden_size=32, BC_hidden_size=16,
                                         trunk_hidden_size=32, branch_activation="swish", BC_activation="sin",
                                         trunk_activation="swish"), 2),
}


def _gold():
    return np.load(GOLD)


def _build(name):
    cls, kw, order = CASES[name]
    return getattr(ppsci.arch, cls)(**kw), order


def _loaded(name):
    z = _gold()
    model, order = _build(name)
    names = [str(n) for n in z[f"{name}/names"]]
    model.set_state_dict({n: z[f"{name}/param/{n}"] for n in names})
    inputs = {k.split("/")[-1]: torch.as_tensor(z[k].astype(np.float32)) for k in z.files if k.startswith(f"{name}/in/")}
    return z, model, order, names, inputs


def _exec(model, order, inputs, train=True):
    dt = len(model.trunk_keys)
    dirs = np.eye(dt).tolist()
    n = int(inputs[model.trunk_keys[0]].shape[0])
    ex = model.make_exec(dirs, dt if order == 2 else 0, n, train)
    dev_ = model.flat_params.device
    ex.set_inputs({k: v.to(dev_) for k, v in inputs.items()})
    return ex, n


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_reference(name, dev):
    """Outputs <= 5e-6 rel, every derivative stream <= 1e-5 rel-L2, gradient rel-L2 <= 1e-4 (BASELINE §4)."""
    z, model, order, names, inputs = _loaded(name)
    ex, n = _exec(model, order, inputs)
    Uref = z[f"{name}/U"]  # [n_out][S][N]
    n_out, S = Uref.shape[0], Uref.shape[1]
    assert ex.S == S
    U = torch.zeros((n_out * S, n), dtype=torch.float32, device=model.flat_params.device)
    ex.forward(model.flat_params, U)
    Ud = U.cpu().numpy().reshape(n_out, S, n)
    for o in range(n_out):
        assert rel(Ud[o, 0], Uref[o, 0]) < 5e-6
        for s in range(1, S):
            assert rel(Ud[o, s], Uref[o, s]) < 1e-5, (o, s)
    cot = torch.as_tensor(z[f"{name}/cot"].reshape(n_out * S, n).astype(np.float32)).to(U.device)
    grad = torch.full((model.n_params,), float("nan"), dtype=torch.float32, device=U.device)
    ex.backward(model.flat_params, cot, grad)
    g = grad.cpu().numpy()
    gref = np.concatenate([z[f"{name}/grad/{nm}"].reshape(-1) for nm in names])
    assert rel(g, gref) < 1e-4
    for nm in names:
        o_, k_ = model._offsets[nm]
        gr = z[f"{name}/grad/{nm}"].reshape(-1)
        if np.linalg.norm(gr) == 0:
            assert np.all(g[o_:o_ + k_] == 0), nm
        else:
            assert rel(g[o_:o_ + k_], gr) < 1e-3, nm
    # model(dict) / predict: values only, [N, 1] per output
    out = model({k: v.numpy() for k, v in inputs.items()})
    for o, k in enumerate(model.output_keys):
        assert tuple(out[k].shape) == (n, 1)
        assert rel(out[k].cpu().numpy()[:, 0], Uref[o, 0]) < 5e-6


def test_parameter_names_and_order():
    z = _gold()
    for name in CASES:
        model, _ = _build(name)
        names = [str(n) for n in z[f"{name}/names"]]
        assert [n for n, _ in model.named_parameters()] == names
        for n, v in model.named_parameters():
            assert tuple(v.shape) == z[f"{name}/param/{n}"].shape, n
    he, _ = _build("he_swish")
    assert he.unused == ["heat_act.beta", "cold_act.beta"]
    chip, _ = _build("chip_swish")
    assert chip.unused == ["branch_act.beta"]  # BC_activation = sin: bc_act has no parameter


def test_state_dict_and_pdparams_round_trip(tmp_path):
    from paddlescience_amd.utils import save_load

    z, model, order, names, inputs = _loaded("he_swish")
    sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    save_load.save_checkpoint(model, None, {"metric": 0.0, "epoch": 1}, output_dir=str(tmp_path), prefix="he")
    other, _ = _build("he_swish")
    assert not np.array_equal(other.state_dict()["trunk_net.last_fc.weight"].cpu().numpy(), sd["trunk_net.last_fc.weight"])
    save_load.load_pretrain(other, os.path.join(str(tmp_path), "checkpoints", "he"))
    for k, v in other.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), sd[k]), k


def test_unused_activation_parameters_stay_put_under_adam(dev):
    z, model, order, names, inputs = _loaded("he_swish")
    ex, n = _exec(model, order, inputs)
    U = torch.zeros((3 * ex.S, n), dtype=torch.float32, device=model.flat_params.device)
    ex.forward(model.flat_params, U)
    grad = torch.zeros(model.n_params, dtype=torch.float32, device=U.device)
    ex.backward(model.flat_params, torch.ones_like(U) * 0.01, grad)
    m, v = torch.zeros_like(grad), torch.zeros_like(grad)
    before = model.flat_params.clone()
    hp.adam_step(model.flat_params, grad, m, v, 1e-2, 1)
    after = model.flat_params
    for nm in model.unused:
        o_, k_ = model._offsets[nm]
        assert torch.equal(before[o_:o_ + k_], after[o_:o_ + k_]), nm
    o_, k_ = model._offsets["trunk_act.beta"]
    assert not torch.equal(before[o_:o_ + k_], after[o_:o_ + k_])


def test_not_implemented_envelope():
    kw = dict(CASES["deeponet_tanh"][1])
    for bad in (dict(branch_weight_norm=True), dict(trunk_skip_connection=True), dict(trunk_activation="relu"),
                dict(branch_activation="stan")):
        with pytest.raises(NotImplementedError):
            ppsci.arch.DeepONet(**{**kw, **bad})
    model = ppsci.arch.DeepONet(**kw)
    with pytest.raises(NotImplementedError):  # a direction over (u, y) is not a trunk direction
        model.make_exec([[1.0, 0.0]], 0, 32)
    with pytest.raises(NotImplementedError):
        D.OnetExec(model, hp.StreamSpec([[1.0]], 1, n3=1), 32)
    model.register_input_transform(lambda x: x)
    with pytest.raises(NotImplementedError):
        model({"u": np.zeros((4, 100), np.float32), "y": np.zeros((4, 1), np.float32)})


def test_standalone_mlp_still_refuses_multi_column():
    with pytest.raises(NotImplementedError):
        ppsci.arch.MLP(("u",), ("b",), 2, 32, input_dim=100)


def test_build_model():
    cls, kw, _ = CASES["chip_swish"]
    m = ppsci.arch.build_model({cls: kw})
    assert isinstance(m, ppsci.arch.ChipDeepONets)


@pytest.mark.gpu
def test_two_identical_steps_are_bitwise_equal(dev):
    if dev != "gpu":
        pytest.skip("device only")
    z, model, order, names, inputs = _loaded("chip_swish")
    ex, n = _exec(model, order, inputs)
    U = torch.zeros((ex.S, n), dtype=torch.float32, device=model.flat_params.device)
    cot = torch.as_tensor(z["chip_swish/cot"].reshape(ex.S, n).astype(np.float32)).to(U.device)
    outs = []
    for _ in range(2):
        g = torch.zeros(model.n_params, dtype=torch.float32, device=U.device)
        ex.forward(model.flat_params, U)
        ex.backward(model.flat_params, cot, g)
        torch.cuda.synchronize()
        outs.append((U.clone(), g.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------ kernels through ctypes
def _act_np(act, z, beta):
    """value and z-derivatives 1..3 in float64; for swish also d/dbeta of (s, d1, d2)."""
    if act == "tanh":
        s = np.tanh(z)
        d1 = 1 - s * s
        return s, d1, -2 * s * d1, d1 * (6 * s * s - 2), None
    g = 1 / (1 + np.exp(-beta * z))
    g1 = g * (1 - g)
    g2 = g1 * (1 - 2 * g)
    g3 = g1 * (1 - 6 * g1)
    s = z * g
    d1 = g + beta * z * g1
    d2 = 2 * beta * g1 + beta * beta * z * g2
    d3 = 3 * beta * beta * g2 + beta ** 3 * z * g3
    return s, d1, d2, d3, (z * z * g1, 2 * z * g1 + beta * z * z * g2, 2 * g1 + 4 * beta * z * g2 + beta * beta * z * z * g3)


def _head_np(J, p, n_out, n1, n2, act, N, Z, tb, B, bb, beta, b):
    """Reference forward in float64: U [n_out, S, N]."""
    S = 1 + n1 + n2
    F = p * n_out
    z0 = Z[0, :, :N] + tb[:, None]
    s, d1, d2, _, _ = _act_np(act, z0, beta)
    A = [s] + [d1 * Z[1 + q, :, :N] for q in range(n1)] + \
        [d2 * Z[1 + q, :, :N] ** 2 + d1 * Z[1 + n1 + q, :, :N] for q in range(n2)]
    w = np.ones((F, N))
    for j in range(J):
        w = w * (B[j][:, :N] + bb[j][:, None])
    U = np.zeros((n_out, S, N))
    for o in range(n_out):
        sl = slice(o * p, (o + 1) * p)
        for si in range(S):
            U[o, si] = (w[sl] * A[si][sl]).sum(0)
        U[o, 0] += b[o]
    return U


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _run_head(J, p, n_out, n1, n2, act, N, Z, tb, B, bb, beta, b, Ubar=None):
    lib = L.lib()
    d = L.OnetHeadDesc()
    NP = (N + 15) // 16 * 16
    d.J, d.p, d.n_out, d.n1, d.n2, d.act, d.N, d.NP = J, p, n_out, n1, n2, L.ACT[act], N, NP
    S, F = 1 + n1 + n2, p * n_out
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(hp_dev())  # noqa: E731
    Zt, tbt, bt = dv(Z), dv(tb), dv(b)
    Bt, bbt = [dv(x) for x in B], [dv(x) for x in bb]
    betat = dv(np.array([beta]))
    Bp = (C.c_void_p * 3)(*[x.data_ptr() for x in Bt])
    bbp = (C.c_void_p * 3)(*[x.data_ptr() for x in bbt])
    U = torch.zeros((n_out * S, N), dtype=torch.float32, device=Zt.device)
    L.check(lib.ppsci_onet_head_fwd(C.byref(d), _ptr(Zt), _ptr(tbt), Bp, bbp, _ptr(betat), _ptr(bt), _ptr(U), hp._stream_ptr(U)))
    if Ubar is None:
        return U.cpu().numpy().astype(np.float64).reshape(n_out, S, N), None
    ch = int(lib.ppsci_onet_head_chunks(NP))
    Ub = dv(Ubar.reshape(n_out * S, N))
    Zbar = torch.full((S, F, NP), float("nan"), device=Zt.device)
    Bbar = [torch.full((F, NP), float("nan"), device=Zt.device) for _ in range(J)]
    ptb = torch.zeros((ch, F), device=Zt.device)
    pbb = torch.zeros((J, ch, F), device=Zt.device)
    pbeta = torch.zeros(F * ch, device=Zt.device)
    pb = torch.zeros((ch, n_out), device=Zt.device)
    Bbp = (C.c_void_p * 3)(*[x.data_ptr() for x in Bbar])
    L.check(lib.ppsci_onet_head_bwd(C.byref(d), _ptr(Zt), _ptr(tbt), Bp, bbp, _ptr(betat), _ptr(Ub), _ptr(Zbar), Bbp, _ptr(ptb),
                                    _ptr(pbb), _ptr(pbeta), _ptr(pb), hp._stream_ptr(U)))
    f = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    return (U.cpu().numpy().astype(np.float64).reshape(n_out, S, N),
            dict(Zbar=f(Zbar), Bbar=[f(x) for x in Bbar], tb=f(ptb).sum(0), bb=f(pbb).sum(1), beta=f(pbeta).sum(), b=f(pb).sum(0)))


def hp_dev():
    from paddlescience_amd.device import get_device

    return get_device()


def _head_inputs(rng, J, p, n_out, S, N):
    NP = (N + 15) // 16 * 16
    F = p * n_out
    Z = np.zeros((S, F, NP))
    Z[:, :, :N] = rng.standard_normal((S, F, N)) * 0.7
    B = []
    for _ in range(J):
        x = np.zeros((F, NP))
        x[:, :N] = rng.standard_normal((F, N))
        B.append(x)
    return Z, rng.standard_normal(F) * 0.1, B, [rng.standard_normal(F) * 0.1 for _ in range(J)], rng.standard_normal(n_out)


@pytest.mark.parametrize("J,S,act", [(1, 1, "tanh"), (2, 3, "swish"), (3, 5, "swish"), (1, 5, "tanh"), (3, 3, "tanh")])
def test_head_kernels_against_numpy(J, S, act, dev):
    N, p = 37 if S == 5 else 300, 5
    n_out = 3 if J == 2 else 1
    n1, n2 = {1: (0, 0), 3: (2, 0), 5: (2, 2)}[S]
    rng = np.random.default_rng(J * 10 + S)
    Z, tb, B, bb, b = _head_inputs(rng, J, p, n_out, S, N)
    beta = 1.3
    Ubar = rng.standard_normal((n_out, S, N))
    U, g = _run_head(J, p, n_out, n1, n2, act, N, Z, tb, B, bb, beta, b, Ubar)
    assert rel(U, _head_np(J, p, n_out, n1, n2, act, N, Z, tb, B, bb, beta, b)) < 1e-5
    # reverse in float64 by autograd on the numpy formulas' torch twin
    tZ = torch.tensor(Z[:, :, :N], requires_grad=True)
    ttb = torch.tensor(tb, requires_grad=True)
    tB = [torch.tensor(x[:, :N], requires_grad=True) for x in B]
    tbb = [torch.tensor(x, requires_grad=True) for x in bb]
    tbeta = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    tb_ = torch.tensor(b, requires_grad=True)
    z0 = tZ[0] + ttb[:, None]
    if act == "tanh":
        fz = lambda z: torch.tanh(z)  # noqa: E731
    else:
        fz = lambda z: z * torch.sigmoid(tbeta * z)  # noqa: E731
    # streams of act(z) along direction q: d/de and d2/de2 of act(z0 + e z1 + e^2/2 z2) at e = 0
    firsts, seconds = [], []
    for q in range(n1):
        zq2 = tZ[1 + n1 + q] if q < n2 else torch.zeros_like(z0)
        e = torch.zeros_like(z0, requires_grad=True)
        y = fz(z0 + e * tZ[1 + q] + 0.5 * e * e * zq2)
        d1 = torch.autograd.grad(y.sum(), e, create_graph=True)[0]
        firsts.append(d1)
        if q < n2:
            seconds.append(torch.autograd.grad(d1.sum(), e, create_graph=True)[0])
    streams = [fz(z0)] + firsts + seconds
    w = tB[0] + tbb[0][:, None]
    for j in range(1, J):
        w = w * (tB[j] + tbb[j][:, None])
    loss = 0.0
    for o in range(n_out):
        sl = slice(o * p, (o + 1) * p)
        for si in range(S):
            val = (w[sl] * streams[si][sl]).sum(0) + (tb_[o] if si == 0 else 0.0)
            loss = loss + (val * torch.tensor(Ubar[o, si])).sum()
    gr = torch.autograd.grad(loss, [tZ, ttb] + tB + tbb + [tbeta, tb_], allow_unused=True)
    assert rel(g["Zbar"][:, :, :N], gr[0].numpy()) < 1e-5
    assert np.all(g["Zbar"][:, :, N:] == 0)
    assert rel(g["tb"], gr[1].numpy()) < 1e-5
    for j in range(J):
        assert rel(g["Bbar"][j][:, :N], gr[2 + j].numpy()) < 1e-5
        assert np.all(g["Bbar"][j][:, N:] == 0)
        assert rel(g["bb"][j], gr[2 + J + j].numpy()) < 1e-5
    if act == "swish":
        assert g["beta"] == pytest.approx(float(gr[2 + 2 * J]), rel=1e-4)
    assert rel(g["b"], gr[-1].numpy()) < 1e-6


def test_swish_beta_gradient_finite_difference(dev):
    """d/dbeta of <Ubar, U(beta)> from the reverse kernel against a central difference of the forward kernel (float64 sums
    of float32 outputs)."""
    J, p, n_out, n1, n2, N = 2, 4, 3, 1, 1, 45
    rng = np.random.default_rng(3)
    Z, tb, B, bb, b = _head_inputs(rng, J, p, n_out, 3, N)
    Ubar = rng.standard_normal((n_out, 3, N))
    beta, h = 0.9, 1e-2
    _, g = _run_head(J, p, n_out, n1, n2, "swish", N, Z, tb, B, bb, beta, b, Ubar)
    up, _ = _run_head(J, p, n_out, n1, n2, "swish", N, Z, tb, B, bb, beta + h, b)
    um, _ = _run_head(J, p, n_out, n1, n2, "swish", N, Z, tb, B, bb, beta - h, b)
    fd = float(((up - um) * Ubar).sum() / (2 * h))
    assert g["beta"] == pytest.approx(fd, rel=2e-3)


def test_pack_against_numpy(dev):
    lib = L.lib()
    N, m = 45, 7
    NP = 48
    src = np.random.default_rng(1).standard_normal((N, m)).astype(np.float32)
    s = torch.as_tensor(src).to(hp_dev())
    dst = torch.full((m, NP), float("nan"), device=s.device)
    L.check(lib.ppsci_onet_pack(m, N, NP, _ptr(s), _ptr(dst), hp._stream_ptr(dst)))
    out = dst.cpu().numpy()
    assert np.array_equal(out[:, :N], src.T)
    assert np.all(out[:, N:] == 0)


def test_bad_arguments_are_refused(dev):
    lib = L.lib()
    d = L.OnetHeadDesc()
    d.J, d.p, d.n_out, d.n1, d.n2, d.act, d.N, d.NP = 4, 4, 1, 0, 0, L.ACT["tanh"], 10, 16
    nul = (C.c_void_p * 3)()
    assert lib.ppsci_onet_head_fwd(C.byref(d), None, None, nul, nul, None, None, None, None) != 0  # J > 3
    assert "onet_head_fwd" in lib.ppsci_last_error().decode()
    d.J, d.act = 1, L.ACT["relu"]
    assert lib.ppsci_onet_head_fwd(C.byref(d), None, None, nul, nul, None, None, None, None) != 0
    assert "activation" in lib.ppsci_last_error().decode()
    d.act, d.NP = L.ACT["tanh"], 12
    assert lib.ppsci_onet_head_bwd(C.byref(d), None, None, nul, nul, None, None, None, nul, None, None, None, None, None) != 0
    assert lib.ppsci_onet_pack(0, 10, 16, None, None, None) != 0
    assert "onet_pack" in lib.ppsci_last_error().decode()
    assert lib.ppsci_pirate_act_fwd(L.PIRATE_GATE, L.ACT["swish"], 16, 32, 32, 1, 1, None, None, None, None, None, None, None,
                                    None) != 0
