"""ppsci.arch.LNO (arch/lno.py, lno_engine.py, csrc/lno.inc) against the REFERENCE's own Laplace neural operator: tests/golden/lno.npz
holds, per case, what /root/reference/ppsci/arch/lno.py computed in float64 (tests/golden/make_lno_golden.py).  Tolerances are
the project's kernel-level ones: rel-L2 2e-6 on values, 5e-6 on gradients, each tensor on its own."""
import os

import numpy as np
import pytest
import torch

from tests.common import make_dev_fixture, rel

dev = make_dev_fixture()

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "lno.npz"))

GRIDS = {
    "yaml": lambda: (np.linspace(0, 19, 39).reshape(1, 39), np.linspace(0, 1, 28).reshape(1, 28)[:, :14],
                     np.linspace(0, 1, 28).reshape(1, 28)[:, :14]),
    "small": lambda: (np.linspace(0, 2, 8).reshape(1, 8), np.linspace(0, 1, 6).reshape(1, 6), np.linspace(0, 1.5, 5).reshape(1, 5)),
}
GRIDS["grid"] = GRIDS["small"]
KW = {
    "yaml": dict(width=8, modes=(4, 4, 4), in_features=4, hidden_features=64, activation="relu", use_norm=True, use_grid=False),
    "small": dict(width=4, modes=(3, 2, 2), in_features=2, hidden_features=16, activation="sin", use_norm=False, use_grid=False),
    "grid": dict(width=4, modes=(3, 2, 2), in_features=5, hidden_features=16, activation="tanh", use_norm=True, use_grid=True),
}


def make_model(case, **over):
    import ppsci

    T, X, Y = GRIDS[case]()
    model = ppsci.arch.LNO(("input",), ("output",), T=T, data=(X, Y), **{**KW[case], **over})
    state = {str(n): torch.tensor(GOLD[f"{case}/param/{n}"], dtype=torch.float32) for n in GOLD[f"{case}/names"]}
    model.set_state_dict(state)
    return model


def to_dev(a, model):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(model.flat_params.device)


@pytest.mark.parametrize("case", ["yaml", "small", "grid"])
def test_output_and_gradients_match_the_reference(case):
    model = make_model(case)
    nat = model.native()
    x = to_dev(GOLD[f"{case}/x"], model)
    y = nat.forward(x)
    e = rel(y.cpu().numpy(), GOLD[f"{case}/y"])
    print(f"{case}: output rel-L2 {e:.2e}")
    worst = {"output": e}
    nat.backward(to_dev(GOLD[f"{case}/w"], model))
    named = dict(model.named_parameters())
    for n in GOLD[f"{case}/names"]:
        n = str(n)
        worst[n] = rel(named[n].grad.cpu().numpy(), GOLD[f"{case}/grad/{n}"])
        print(f"{case}: d/d{n} rel-L2 {worst[n]:.2e}")
    worst["input"] = rel(nat.gx.cpu().numpy().reshape(GOLD[f"{case}/grad_x"].shape), GOLD[f"{case}/grad_x"])
    print(f"{case}: d/dinput rel-L2 {worst['input']:.2e}")
    assert worst.pop("output") <= 2e-6
    bad = {k: v for k, v in worst.items() if not v <= 5e-6}
    assert not bad, bad


def test_laplace_layer_parts():
    """x1 (steady-state part) and x2 (transient part) of lno.py:160-187 separately."""
    model = make_model("small")
    nat = model.native()
    nat.forward(to_dev(GOLD["small/x"], model))  # (allocates the buffer set of this shape)
    z = to_dev(GOLD["small/lap_z"], model).reshape(3, 4, -1).contiguous()
    out = torch.empty_like(z)
    nat.laplace_forward(z, out, x1_only=True)
    e1 = rel(out.cpu().numpy().reshape(GOLD["small/lap_x1"].shape), GOLD["small/lap_x1"])
    nat.laplace_forward(z, out, x2_only=True)
    e2 = rel(out.cpu().numpy().reshape(GOLD["small/lap_x2"].shape), GOLD["small/lap_x2"])
    nat.laplace_forward(z, out)
    e = rel(out.cpu().numpy().reshape(GOLD["small/lap_x1"].shape), GOLD["small/lap_x1"] + GOLD["small/lap_x2"])
    print(f"laplace: x1 {e1:.2e}, x2 {e2:.2e}, x1 + x2 {e:.2e}")
    assert e1 <= 2e-6 and e2 <= 2e-6 and e <= 2e-6


@pytest.mark.parametrize("n", [5, 6, 8, 14, 39])
def test_dft_against_numpy(n):
    """Forward, adjoint and inverse along three axes of sizes (n, 3, 4) in each position, real and complex input."""
    from paddlescience_amd import _lib as L
    from paddlescience_amd import device, lno_engine
    from paddlescience_amd.hotpath import _p, _stream_ptr

    d = device.get_device()
    rng = np.random.default_rng(n)
    for shape in ((n, 3, 4), (3, n, 4), (4, 3, n)):
        N = int(np.prod(shape))
        tw = torch.tensor(lno_engine.twiddles(shape)).to(d)
        xc = rng.standard_normal((2, *shape)) + 1j * rng.standard_normal((2, *shape))
        planes = torch.tensor(np.stack([xc.real, xc.imag], 1).reshape(2, 2, N), dtype=torch.float32).to(d)
        real = torch.tensor(xc.real.reshape(2, N), dtype=torch.float32).to(d)
        out = torch.empty((2, 2, N), dtype=torch.float32, device=d)

        def run(mode, src, sign, scale, out_real=0, dst=out):
            L.check(L.lib().ppsci_lno_dft3(2, *shape, mode, _p(src), 1, None, 0, 0, 0, 1.0, None, _p(tw), sign, out_real, 0, scale, 0,
                                           _p(dst), _stream_ptr(dst)))
            r = dst.cpu().numpy().astype(np.float64)
            return r if out_real else (r[:, 0] + 1j * r[:, 1]).reshape(2, *shape)

        def rel(a, b):  # (tests.common.rel keeps the real part only)
            a, b = np.asarray(a), np.asarray(b)
            return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))

        ax = (1, 2, 3)
        assert rel(run(1, planes, -1, 1.0), np.fft.fftn(xc, axes=ax)) <= 2e-6
        assert rel(run(0, real, -1, 1.0), np.fft.fftn(xc.real, axes=ax)) <= 2e-6
        assert rel(run(1, planes, 1, 1.0), np.fft.ifftn(xc, axes=ax) * N) <= 2e-6  # the adjoint of the forward transform
        assert rel(run(1, planes, 1, 1.0 / N), np.fft.ifftn(xc, axes=ax)) <= 2e-6
        ro = torch.empty((2, N), dtype=torch.float32, device=d)
        assert rel(run(1, planes, 1, 1.0 / N, 1, ro).reshape(2, *shape), np.fft.ifftn(xc, axes=ax).real) <= 2e-6


@pytest.mark.parametrize("N", [64, 240, 1001])
def test_instance_norm_against_numpy(N):
    from paddlescience_amd import _lib as L
    from paddlescience_amd import device
    from paddlescience_amd.hotpath import _p, _stream_ptr

    d = device.get_device()
    rng = np.random.default_rng(N)
    planes = 5
    x = (rng.standard_normal((planes, N)) * 3e4 + rng.uniform(-1e4, 1e4, (planes, 1))).astype(np.float32)  # the Laplace output's scale
    gy = rng.standard_normal((planes, N)).astype(np.float32)
    add = rng.standard_normal((planes, N)).astype(np.float32)
    xt, gt, at = (torch.tensor(v).to(d) for v in (x, gy, add))
    y, st, gx = torch.empty_like(xt), torch.empty((planes, 2), device=d), torch.empty_like(xt)
    L.check(L.lib().ppsci_lno_inorm_fwd(planes, N, 1e-5, _p(xt), _p(y), _p(st), _stream_ptr(y)))
    L.check(L.lib().ppsci_lno_inorm_bwd(planes, N, _p(y), _p(gt), _p(st), _p(at), _p(gx), _stream_ptr(y)))
    x64, g64 = x.astype(np.float64), gy.astype(np.float64)
    mean, var = x64.mean(1, keepdims=True), x64.var(1, keepdims=True)
    rstd = 1 / np.sqrt(var + 1e-5)
    yo = (x64 - mean) * rstd
    go = rstd * (g64 - g64.mean(1, keepdims=True) - yo * (g64 * yo).mean(1, keepdims=True)) + add
    assert rel(y.cpu().numpy(), yo) <= 2e-6
    assert rel(gx.cpu().numpy(), go) <= 5e-6


@pytest.mark.parametrize("act", ["relu", "sin", "tanh", "gelu", "silu"])
def test_head_against_numpy(act):
    """y = fc2(act(fc1(x1 + conv(h)))) per point and its reverse; B * N = 2 * 333 points: not a multiple of 64."""
    from paddlescience_amd import _lib as L
    from paddlescience_amd import device
    from paddlescience_amd.hotpath import _p, _stream_ptr

    d = device.get_device()
    rng = np.random.default_rng(3)
    B, N, Cw, Hd = 2, 333, 3, 19
    f = lambda *s: rng.standard_normal(s)
    x1, h, Wc, bc, W1, b1, W2, b2, gy = f(B, Cw, N), f(B, Cw, N), f(Cw, Cw) * .5, f(Cw) * .1, f(Cw, Hd) * .5, f(Hd) * .1, f(Hd) * .3, f(1), f(B, N)
    x1, h, Wc, bc, W1, b1, W2, b2, gy = (v.astype(np.float32).astype(np.float64) for v in (x1, h, Wc, bc, W1, b1, W2, b2, gy))
    t = {k: torch.tensor(v, dtype=torch.float32).to(d).contiguous() for k, v in dict(x1=x1, h=h, Wc=Wc, bc=bc, W1=W1, b1=b1, W2=W2, b2=b2, gy=gy).items()}
    y = torch.empty((B, N), device=d)
    st = _stream_ptr(y)
    L.check(L.lib().ppsci_lno_head_fwd(B, N, Cw, Hd, L.ACT[act], _p(t["x1"]), _p(t["h"]), _p(t["Wc"]), _p(t["bc"]), _p(t["W1"]),
                                       _p(t["b1"]), _p(t["W2"]), _p(t["b2"]), _p(y), st))
    rows = int(L.lib().ppsci_lno_point_rows(B * N))
    cols = Cw * Cw + Cw + Cw * Hd + 2 * Hd + 1
    gx1, gh, part = torch.empty((B, Cw, N), device=d), torch.empty((B, Cw, N), device=d), torch.empty((rows, cols), device=d)
    L.check(L.lib().ppsci_lno_head_bwd(B, N, Cw, Hd, L.ACT[act], _p(t["x1"]), _p(t["h"]), _p(t["Wc"]), _p(t["bc"]), _p(t["W1"]),
                                       _p(t["b1"]), _p(t["W2"]), _p(t["gy"]), _p(gx1), _p(gh), _p(part), st))
    # float64 restatement with torch's autograd
    T = {k: torch.tensor(v, requires_grad=True) for k, v in dict(x1=x1, h=h, Wc=Wc, bc=bc, W1=W1, b1=b1, W2=W2, b2=b2).items()}
    u = T["x1"] + torch.einsum("oi,bis->bos", T["Wc"], T["h"]) + T["bc"][None, :, None]
    zz = torch.einsum("bcs,cj->bsj", u, T["W1"]) + T["b1"]
    fn = dict(relu=torch.relu, sin=torch.sin, tanh=torch.tanh, gelu=torch.nn.functional.gelu, silu=torch.nn.functional.silu)[act]
    yo = fn(zz) @ T["W2"] + T["b2"]
    (yo * torch.tensor(gy)).sum().backward()
    assert rel(y.cpu().numpy(), yo.detach().numpy()) <= 2e-6
    assert rel(gx1.cpu().numpy(), T["x1"].grad.numpy()) <= 5e-6
    assert rel(gh.cpu().numpy(), T["h"].grad.numpy()) <= 5e-6
    got = part.cpu().numpy().astype(np.float64).sum(0)
    want = np.concatenate([T[k].grad.numpy().reshape(-1) for k in ("Wc", "bc", "W1", "b1", "W2", "b2")])
    off = 0
    for k in ("Wc", "bc", "W1", "b1", "W2", "b2"):
        n = T[k].numel()
        assert rel(got[off:off + n], want[off:off + n]) <= 5e-6, k
        off += n


def test_two_reverse_passes_are_bitwise_identical():
    model = make_model("grid")
    nat = model.native()
    x, w = to_dev(GOLD["grid/x"], model), to_dev(GOLD["grid/w"], model)
    grads = []
    for _ in range(2):
        model.flat_grad.zero_()
        nat.forward(x)
        nat.backward(w)
        grads.append((model.flat_grad.cpu().numpy().copy(), nat.gx.cpu().numpy().copy()))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1])
    assert np.abs(grads[0][0]).min() > 0  # every parameter receives a gradient


@pytest.mark.parametrize("case", ["yaml", "grid"])
def test_parameter_names_and_state_dict_are_the_references(case, tmp_path):
    model = make_model(case)
    named = list(model.named_parameters())
    assert [n for n, _ in named] == [str(n) for n in GOLD[f"{case}/names"]]
    for n, p in named:
        assert tuple(p.shape) == GOLD[f"{case}/param/{n}"].shape, n
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD[f"{case}/state_keys"]]
    for k in sd:
        if ".t_" in k or ".lambda_" in k:
            ref = GOLD[f"{case}/buffer/{k}"]
            assert tuple(sd[k].shape) == ref.shape, k
            assert rel(sd[k].cpu().numpy(), ref) <= 1e-6, k
    # one flat buffer in the order of named_parameters()
    off = 0
    for _, p in named:
        assert p.data_ptr() == model.flat_params.data_ptr() + 4 * off
        off += p.numel()
    assert off == model.flat_params.numel() == model.num_params
    # a checkpoint written by save_checkpoint loads back bit-identically
    from paddlescience_amd.utils import save_load

    save_load.save_checkpoint(model, None, {"metric": 0.0, "epoch": 1}, output_dir=str(tmp_path), prefix="lno")
    other = make_model(case)
    with torch.no_grad():
        other.flat_params.mul_(0.5)
    save_load.load_pretrain(other, os.path.join(str(tmp_path), "checkpoints", "lno"))
    assert np.array_equal(other.flat_params.cpu().numpy(), model.flat_params.cpu().numpy())


def test_second_batch_shape_keeps_the_first_buffer_set():
    model = make_model("small")
    nat = model.native()
    x = to_dev(GOLD["small/x"], model)
    y3 = nat.forward(x).clone()
    keep = nat.alpha.data_ptr()
    y1 = nat.forward(x[:1].contiguous()).clone()
    assert nat.generation == 0 and nat.alpha.data_ptr() != keep
    nat.forward(x)
    assert nat.alpha.data_ptr() == keep and nat.generation == 0
    assert np.array_equal(y1.cpu().numpy(), y3[:1].cpu().numpy())


def test_what_is_not_built_raises():
    import ppsci

    T, X, Y = GRIDS["small"]()
    with pytest.raises(NotImplementedError, match="the reference's own forward only runs for three"):
        ppsci.arch.LNO(("input",), ("output",), 4, (3, 2), T, (X,))
    with pytest.raises(NotImplementedError, match="more than one output key"):
        ppsci.arch.LNO(("input",), ("u", "v"), 4, (3, 2, 2), T, (X, Y))
    with pytest.raises(NotImplementedError, match="no trainable activation"):
        ppsci.arch.LNO(("input",), ("output",), 4, (3, 2, 2), T, (X, Y), activation="swish")
    model = make_model("small")
    model.register_input_transform(lambda d: d)
    from paddlescience_amd.operator_engine import OperatorConstraint
    from paddlescience_amd import loss

    cst = OperatorConstraint("c", model, {}, loss.L2RelLoss("sum"), model.flat_params.device, ["output"], 3)
    cst.bind({"input": GOLD["small/x"]}, {"output": GOLD["small/y"].astype(np.float32)})
    with pytest.raises(NotImplementedError, match="registered input / output transforms"):
        cst.forward_backward_native(model.native())
