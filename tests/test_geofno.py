"""ppsci.arch.FNO1d (arch/geofno.py, geofno_engine.py, csrc/fno1d.inc) against the REFERENCE's own 1-D Fourier neural operator:
tests/golden/geofno.npz holds, per case, what /root/reference/ppsci/arch/geofno.py computed in float64
(tests/golden/make_geofno_golden.py).  The bound of each tensor is the larger of the project's kernel-level tolerance (DESIGN.md
section 5: rel-L2 2e-6 on values, 5e-6 on gradients) and TWICE the error of the reference's own float32 run against its float64
run, which the fixture records (`<case>/ref32_err/<name>`): float32 itself is not always inside the project tolerance on this
network, and the factor two allows for another summation order."""
import os

import numpy as np
import pytest
import torch

from tests.common import make_dev_fixture, rel
from tests.geofno_common import CASES, draw_inputs, draw_params, sample_index

dev = make_dev_fixture()

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "geofno.npz"))


def make_model(case, **over):
    import ppsci

    c = CASES[case]
    model = ppsci.arch.FNO1d(**{**c["kw"], **over})
    shapes = [tuple(int(v) for v in str(s).split(",")) for s in GOLD[f"{case}/shapes"]]
    vals = draw_params(list(zip([str(n) for n in GOLD[f"{case}/names"]], shapes)), c["kw"]["width"], c["seed"])
    model.set_state_dict({k: torch.tensor(v, dtype=torch.float32) for k, v in vals.items()})
    return model


def to_dev(a, model):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(model.flat_params.device)


def bound(case, name, tol):
    return max(tol, 2.0 * float(GOLD[f"{case}/ref32_err/{name}"]))


@pytest.mark.parametrize("case", ["yaml", "odd", "nyq", "trunc"])
def test_output_and_gradients_match_the_reference(case):
    """(`yaml`, the catheter shape, takes 15 s on the emulator: it runs there too.)"""
    model = make_model(case)
    nat = model.native()
    x, w = draw_inputs(case)
    y = nat.forward(to_dev(x, model))
    errs = {"output": (rel(y.cpu().numpy(), GOLD[f"{case}/y"]), bound(case, "output", 2e-6))}
    nat.backward(to_dev(w, model))
    named = dict(model.named_parameters())
    for n in GOLD[f"{case}/names"]:
        n = str(n)
        g = named[n].grad.cpu().numpy().astype(np.float64)
        if f"{case}/grad/{n}" in GOLD:
            errs[n] = (rel(g, GOLD[f"{case}/grad/{n}"]), bound(case, n, 5e-6))
        else:  # a large tensor of the catheter model: its norm and a fixed index sample
            idx = sample_index(n, g.size)
            ref_norm = float(GOLD[f"{case}/grad_norm/{n}"])
            errs[n] = (rel(g.ravel()[idx], GOLD[f"{case}/grad_sample/{n}"]), bound(case, n, 5e-6))
            errs[n + " (norm)"] = (abs(np.linalg.norm(g.ravel()) - ref_norm) / ref_norm, bound(case, n, 5e-6))
    errs["input"] = (rel(nat.gx.cpu().numpy(), GOLD[f"{case}/grad/input"]), bound(case, "input", 5e-6))
    for k, (e, b) in errs.items():
        print(f"{case}: {k} rel-L2 {e:.2e} (bound {b:.2e}, float32 reference {float(GOLD[case + '/ref32_err/' + k.split(' ')[0]]):.2e})")
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("case", ["odd", "nyq"])
def test_parameter_names_and_state_dict_are_the_references(case, tmp_path):
    model = make_model(case)
    named = list(model.named_parameters())
    assert [n for n, _ in named] == [str(n) for n in GOLD[f"{case}/names"]]
    for (n, p), s in zip(named, GOLD[f"{case}/shapes"]):
        assert ",".join(str(v) for v in p.shape) == str(s), n
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD[f"{case}/state_keys"]]
    # one flat buffer in the order of named_parameters()
    off = 0
    for _, p in named:
        assert p.data_ptr() == model.flat_params.data_ptr() + 4 * off
        off += p.numel()
    assert off == model.flat_params.numel() == model.num_params
    # a checkpoint written by save_checkpoint loads back bit-identically
    from paddlescience_amd.utils import save_load

    save_load.save_checkpoint(model, None, {"metric": 0.0, "epoch": 1}, output_dir=str(tmp_path), prefix="geofno")
    other = make_model(case)
    with torch.no_grad():
        other.flat_params.mul_(0.5)
    save_load.load_pretrain(other, os.path.join(str(tmp_path), "checkpoints", "geofno"))
    assert np.array_equal(other.flat_params.cpu().numpy(), model.flat_params.cpu().numpy())


def test_default_constructor_is_the_catheter_model():
    import ppsci

    model = ppsci.arch.FNO1d()
    assert (model.modes1, model.width, model.padding, model.output_np, model.input_keys, model.output_keys) == \
        (64, 64, 100, 2001, ("input",), ("output",))
    assert [n for n, _ in model.named_parameters()] == [str(n) for n in GOLD["yaml/names"]]
    for k in range(5):  # geofno.py:33-46: rand / (in * out)
        for part in ("real", "imag"):
            v = getattr(getattr(model, f"conv{k}"), f"weights1_{part}").detach().cpu().numpy()
            assert v.min() >= 0 and v.max() <= 1 / 64 ** 2 and v.mean() > 0.4 / 64 ** 2
    assert float(model.fc0.bias.detach().abs().max()) == 0 and float(model.w0.bias.detach().abs().max()) == 0


def test_what_is_not_built_raises():
    import ppsci

    with pytest.raises(NotImplementedError, match=r"x\[\.\.\., :-padding\], which is empty"):
        ppsci.arch.FNO1d(padding=0)
    model = make_model("odd")
    x, _ = draw_inputs("odd")
    with pytest.raises(ValueError, match="exceeds 5 = s // 2 \\+ 1"):
        model.native().forward(to_dev(x[:, :8], model))  # 6 modes, 8 points
    with pytest.raises(ValueError, match=r"must be \[B, s, 2\]"):
        model.native().forward(to_dev(x[..., :1], model))
    model.register_input_transform(lambda d: d)
    from paddlescience_amd import loss
    from paddlescience_amd.operator_engine import OperatorConstraint

    cst = OperatorConstraint("c", model, {}, loss.L2RelLoss("sum"), model.flat_params.device, ["output"], 3)
    cst.bind({"input": x}, {"output": GOLD["odd/y"].astype(np.float32)})
    with pytest.raises(NotImplementedError, match="registered input / output transforms"):
        cst.forward_backward_native(model.native())


def test_input_length_is_free_and_call_outside_training_is_native():
    """The input length is whatever the batch has (here 50 points into output_np = 29); model(dict) runs the same kernels."""
    model = make_model("odd")
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, 50, 2)).astype(np.float32)
    out = model({"input": x})["output"]
    assert tuple(out.shape) == (2, 29, 1) and np.isfinite(out.cpu().numpy()).all()
    assert np.array_equal(out.cpu().numpy(), model.native().forward(to_dev(x, model)).cpu().numpy())


def test_two_reverse_passes_are_bitwise_identical():
    model = make_model("odd")
    nat = model.native()
    x, w = draw_inputs("odd")
    x, w = to_dev(x, model), to_dev(w, model)
    grads = []
    for _ in range(2):
        model.flat_grad.zero_()
        nat.forward(x)
        nat.backward(w)
        grads.append((model.flat_grad.cpu().numpy().copy(), nat.gx.cpu().numpy().copy()))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1])
    # every parameter tensor receives a gradient (single entries are exactly zero by construction: irfft ignores the imaginary
    # part of the DC coefficient, so dL/d weights1_imag[:, :, 0] = 0)
    assert all(float(p.grad.abs().max()) > 0 for _, p in model.named_parameters())


def test_second_batch_shape_keeps_the_first_buffer_set():
    model = make_model("odd")
    nat = model.native()
    x = to_dev(draw_inputs("odd")[0], model)
    y3 = nat.forward(x).clone()
    keep = nat.Y.data_ptr()
    y1 = nat.forward(x[:1].contiguous()).clone()
    assert nat.generation == 0 and nat.Y.data_ptr() != keep
    nat.forward(x)
    assert nat.Y.data_ptr() == keep and nat.generation == 0
    assert np.array_equal(y1.cpu().numpy(), y3[:1].cpu().numpy())


# ---------------------------------------------------------------------------------------------- kernels against numpy in double
LK, NK, CK, MK, BK = 97, 61, 8, 5, 3


def _kernel_env():
    from paddlescience_amd import _lib as L
    from paddlescience_amd import device, geofno_engine
    from paddlescience_amd.hotpath import _p, _stream_ptr

    return L, device.get_device(), geofno_engine, _p, _stream_ptr


def test_tables_against_numpy_fft():
    from paddlescience_amd import geofno_engine as E

    rng = np.random.default_rng(0)
    for L_in, n, M in ((LK, NK, MK), (40, 40, 21), (37, 8, 6), (12, 12, 7)):
        Ta, Ts = E.tables(L_in, n, M)
        x = rng.standard_normal((4, L_in))
        X = x @ Ta.astype(np.float64)
        ref = np.fft.rfft(x)[:, :M]
        assert rel(X[:, 0::2], ref.real) <= 1e-6 and rel(X[:, 1::2], ref.imag) <= 1e-6
        Y = rng.standard_normal((4, M)) + 1j * rng.standard_normal((4, M))
        full = np.zeros((4, max(n // 2 + 1, M)), dtype=np.complex128)
        full[:, :M] = Y
        want = np.fft.irfft(full[:, :n // 2 + 1], n=n)
        Yri = np.empty((4, 2 * M))
        Yri[:, 0::2], Yri[:, 1::2] = Y.real, Y.imag
        assert rel(Yri @ Ts.astype(np.float64), want) <= 1e-6


@pytest.mark.parametrize("S", [1, 3])
def test_analysis_kernel_and_its_k_split(S):
    L, d, E, _p, _stream_ptr = _kernel_env()
    rng = np.random.default_rng(1)
    Ta, _ = E.tables(LK, NK, MK)
    ldx = LK + 3  # (rows longer than the transformed part, as for the cropped field of the last layer)
    x = rng.standard_normal((BK * CK, ldx)).astype(np.float32)
    xt, Tt = torch.tensor(x).to(d), torch.tensor(Ta).to(d)
    part = torch.zeros((S, BK * CK, 2 * MK), device=d)
    L.check(L.lib().ppsci_fno1d_analysis(BK * CK, LK, 2 * MK, S, ldx, _p(xt), _p(Tt), _p(part), _stream_ptr(part)))
    got = part.cpu().numpy().astype(np.float64)
    want = x[:, :LK].astype(np.float64) @ Ta.astype(np.float64)
    assert rel(got.sum(0), want) <= 2e-6
    if S > 1:
        for s in range(S):  # slice s holds rows [K s / S, K (s + 1) / S) of the table
            k0, k1 = LK * s // S, LK * (s + 1) // S
            assert rel(got[s], x[:, k0:k1].astype(np.float64) @ Ta[k0:k1].astype(np.float64)) <= 2e-6


def _gelu(v):
    from math import erf, sqrt

    return 0.5 * v * (1 + np.vectorize(erf)(v / sqrt(2)))


def _dgelu(v):
    from math import erf, sqrt

    return 0.5 * (1 + np.vectorize(erf)(v / sqrt(2))) + v * np.exp(-0.5 * v * v) / np.sqrt(2 * np.pi)


def test_fused_layer_kernel_in_both_directions():
    """v = Y Ts + Wc x + bc, out = gelu(v) at L = 97 -> n = 61 (columns of x beyond its length read as zero), and the reverse
    data path dx = (Xbar Ta^T + Wc^T gv) gelu'(v_below) with a zero tail, C = 8, M = 5."""
    L, d, E, _p, _stream_ptr = _kernel_env()
    rng = np.random.default_rng(2)
    Ta, Ts = E.tables(LK, NK, MK)
    f32 = lambda a: np.asarray(a).astype(np.float32)
    Y, Wc, bc, x = f32(rng.standard_normal((BK, CK, 2 * MK))), f32(rng.standard_normal((CK, CK)) / 3), f32(rng.standard_normal(CK)), \
        f32(rng.standard_normal((BK, CK, LK)))
    t = {k: torch.tensor(v).to(d) for k, v in dict(Y=Y, Wc=Wc, bc=bc, x=x, Ts=Ts, TaT=Ta.T.copy()).items()}
    v, out = torch.empty((BK, CK, NK), device=d), torch.empty((BK, CK, NK), device=d)

    def launch(**kw):
        desc = L.Fno1dLayerDesc()
        for k, val in kw.items():
            setattr(desc, k, val.data_ptr() if isinstance(val, torch.Tensor) else val)
        return L.lib().ppsci_fno1d_layer(desc, _stream_ptr(v))

    L.check(launch(B=BK, R=CK, K1=2 * MK, A1=t["Y"], a1_bs=CK * 2 * MK, T=t["Ts"], ldt=NK, K2=CK, A2=t["Wc"], a2_rs=CK, a2_cs=1, X2=t["x"],
                   x2_bs=CK * LK, x2_ld=LK, x2_len=LK, bias=t["bc"], v=v, out=out, o_bs=CK * NK, o_ld=NK, act=1, Lc=NK, Lout=NK))
    want = np.einsum("bok,kl->bol", Y.astype(np.float64), Ts.astype(np.float64)) \
        + np.einsum("oi,bil->bol", Wc.astype(np.float64), x[:, :, :NK].astype(np.float64)) + bc[None, :, None]
    assert rel(v.cpu().numpy(), want) <= 2e-6 and rel(out.cpu().numpy(), _gelu(want)) <= 2e-6
    # reverse: rows = input channels, A2 = Wc^T through its strides, gelu' of the layer below, zeros on columns [LK - 7, LK)
    Xb, gv, vb = f32(rng.standard_normal((BK, CK, 2 * MK))), f32(rng.standard_normal((BK, CK, LK))), f32(rng.standard_normal((BK, CK, LK)))
    tb = {k: torch.tensor(a).to(d) for k, a in dict(Xb=Xb, gv=gv, vb=vb).items()}
    dx = torch.full((BK, CK, LK), 7.0, device=d)
    Lc = LK - 7
    L.check(launch(B=BK, R=CK, K1=2 * MK, A1=tb["Xb"], a1_bs=CK * 2 * MK, T=t["TaT"], ldt=LK, K2=CK, A2=t["Wc"], a2_rs=1, a2_cs=CK,
                   X2=tb["gv"], x2_bs=CK * LK, x2_ld=LK, x2_len=LK, dact_v=tb["vb"], dv_bs=CK * LK, dv_ld=LK, out=dx, o_bs=CK * LK, o_ld=LK,
                   act=0, Lc=Lc, Lout=LK))
    want = (np.einsum("bik,kl->bil", Xb.astype(np.float64), Ta.T.astype(np.float64))
            + np.einsum("oi,bol->bil", Wc.astype(np.float64), gv.astype(np.float64))) * _dgelu(vb.astype(np.float64))
    want[:, :, Lc:] = 0
    got = dx.cpu().numpy()
    assert rel(got, want) <= 5e-6 and np.all(got[:, :, Lc:] == 0)


def test_interpolation_epilogue_and_its_adjoint():
    """<interp(x), g> == <x, interp^T(g)> through the layer kernel's two epilogues, and interp against numpy."""
    L, d, E, _p, _stream_ptr = _kernel_env()
    rng = np.random.default_rng(3)
    s, n = 37, 29
    i0, tt, first = E.interp_tables(s, n)
    x = rng.standard_normal((BK, CK, s + 4)).astype(np.float32)
    g = rng.standard_normal((BK, CK, n)).astype(np.float32)
    zero = np.zeros((BK, CK, 2), dtype=np.float32)
    T1 = np.zeros((2, max(s, n)), dtype=np.float32)
    t = {k: torch.tensor(v).to(d) for k, v in dict(x=x, g=g, zero=zero, T1=T1, i0=i0, tt=tt, first=first).items()}
    up, down = torch.empty((BK, CK, n), device=d), torch.empty((BK, CK, s), device=d)

    def launch(**kw):
        desc = L.Fno1dLayerDesc()
        for k, val in kw.items():
            setattr(desc, k, val.data_ptr() if isinstance(val, torch.Tensor) else val)
        L.check(L.lib().ppsci_fno1d_layer(desc, _stream_ptr(up)))

    common = dict(B=BK, R=CK, K1=2, A1=t["zero"], a1_bs=CK * 2, T=t["T1"], ldt=max(s, n), K2=0, act=0, ip_i0=t["i0"], ip_t=t["tt"])
    launch(**common, ip_src=t["x"], ip_bs=CK * (s + 4), ip_ld=s + 4, out=up, o_bs=CK * n, o_ld=n, Lc=n, Lout=n)
    launch(**common, ia_src=t["g"], ia_bs=CK * n, ia_ld=n, ia_first=t["first"], out=down, o_bs=CK * s, o_ld=s, Lc=s, Lout=s)
    pos = np.linspace(0, s - 1, n)
    want = np.stack([[np.interp(pos, np.arange(s), row[:s]) for row in smp] for smp in x.astype(np.float64)])
    assert rel(up.cpu().numpy(), want) <= 2e-6
    lhs = float((up.cpu().numpy().astype(np.float64) * g).sum())
    rhs = float((down.cpu().numpy().astype(np.float64) * x[:, :, :s]).sum())
    assert abs(lhs - rhs) <= 5e-6 * max(abs(lhs), 1.0)


def test_bad_arguments_are_reported_and_nothing_runs():
    L, d, E, _p, _stream_ptr = _kernel_env()
    lib = L.lib()
    buf = torch.zeros(4096, device=d)
    p, st = _p(buf), _stream_ptr(buf)

    def bad(rc, needle):
        assert rc != 0
        assert needle in lib.ppsci_last_error().decode()

    bad(lib.ppsci_fno1d_lift_fwd(0, 4, 8, 2, 4, p, p, p, p, st), "fno1d_lift_fwd")
    bad(lib.ppsci_fno1d_lift_fwd(1, 9, 8, 2, 4, p, p, p, p, st), "fno1d_lift_fwd")  # padded length below the input's
    bad(lib.ppsci_fno1d_lift_bwd(1, 4, 8, 2, 4, p, p, None, p, p, st), "fno1d_lift_bwd")
    bad(lib.ppsci_fno1d_analysis(4, 8, 4, 9, 8, p, p, p, st), "fno1d_analysis")   # more slices than K
    bad(lib.ppsci_fno1d_analysis(4, 8, 4, 1, 7, p, p, p, st), "fno1d_analysis")   # row stride below K
    bad(lib.ppsci_fno1d_mix(1, 4, 2, 1, 2, p, None, p, p, p, st), "fno1d_mix")
    bad(lib.ppsci_fno1d_mix(1, 4, 2, 1, 0, p, None, None, p, p, st), "fno1d_mix")
    bad(lib.ppsci_fno1d_mix_wgrad(1, 4, 0, p, p, p, p, st), "fno1d_mix_wgrad")
    bad(lib.ppsci_fno1d_wgrad(1, 4, 4, 8, 24, 1, p, 32, 8, p, 32, 8, p, st), "fno1d_wgrad")   # chunk not a multiple of 16
    bad(lib.ppsci_fno1d_wgrad(1, 129, 4, 8, 16, 1, p, 32, 8, p, 32, 8, p, st), "fno1d_wgrad")
    bad(lib.ppsci_fno1d_head_pre(1, 4, 8, p, None, p, p, p, st), "fno1d_head_pre")
    desc = L.Fno1dLayerDesc()
    bad(lib.ppsci_fno1d_layer(desc, st), "fno1d_layer")
    desc.B, desc.R, desc.K2, desc.Lc, desc.Lout, desc.o_ld = 1, 129, 4, 8, 8, 8
    desc.A2 = desc.X2 = desc.out = p
    desc.x2_len = 8
    bad(lib.ppsci_fno1d_layer(desc, st), "at most 128 rows")
    assert lib.ppsci_fno1d_layer_supported(64, 128, 64) == 1 and lib.ppsci_fno1d_layer_supported(129, 0, 4) == 0
    assert float(buf.abs().max()) == 0


# ---------------------------------------------------------------------------------------------- training through Solver
def _solver(model, tmp_path, steps):
    import ppsci

    x, y = GOLD["train/x"], GOLD["train/y"]
    cfg = {"dataset": {"name": "NamedArrayDataset", "input": {"input": x}, "label": {"output": y}},
           "batch_size": len(x), "sampler": {"name": "BatchSampler", "shuffle": False, "drop_last": True}}
    cst = ppsci.constraint.SupervisedConstraint(cfg, ppsci.loss.L2RelLoss("sum"), name="Sup")
    opt = ppsci.optimizer.Adam(1e-3, weight_decay=1e-4)(model)
    return ppsci.solver.Solver(model, {"Sup": cst}, str(tmp_path), opt, epochs=steps, iters_per_epoch=1, log_freq=1)


def _curve(tmp_path, steps=30):
    solver = _solver(make_model("odd"), tmp_path, steps)
    solver.train()
    return np.array([v for _, v in solver.train_loss_info["loss"]], dtype=np.float64), solver


def test_training_follows_the_reference_loss_curve(tmp_path):
    """30 Adam steps (lr 1e-3, weight_decay 1e-4, L2RelLoss("sum")) from the fixture's parameters on its batch of 8: the loss at
    every step stays within FOUR times the deviation of the reference's own float32 run from its float64 run at that step
    (`train/ref32_dev`; Adam's division by sqrt(v) amplifies rounding, hence a wider margin than for the gradients).

    MEASURED: worst ratio 1.07 on the emulator (step 3), 1.00 on an MI355X; at 17 of the 30 steps the loss here is the very float32 number of the reference's float32
    run.  Two things this test found on the way are fixed in the code: Adam(weight_decay) took its bias corrections from the exact
    betas while its kernel holds them in float32 (a drift to ratio 120), and the field-loss kernels summed in fp32, which left the
    loss up to one float32 unit in the last place from the float32 nearest to its exact value (ratio 6.2 at step 2, where four times
    the recorded deviation is less than that unit); they now carry sums, terms and total in double and round once."""
    mine, _ = _curve(tmp_path)
    ref, dev32 = GOLD["train/loss64"], GOLD["train/ref32_dev"]
    assert len(mine) == 30
    ratio = np.abs(mine - ref) / dev32
    for k in range(30):
        print(f"step {k:2d}: loss {mine[k]:.7f} reference {ref[k]:.7f} |diff| {abs(mine[k] - ref[k]):.2e} float32 reference {dev32[k]:.2e} "
              f"ratio {ratio[k]:.2f}")
    print(f"worst ratio {ratio.max():.2f} at step {int(ratio.argmax())}")
    assert np.all(ratio <= 4.0), f"worst ratio {ratio.max():.2f} at step {int(ratio.argmax())}"


def test_eager_and_captured_steps_agree(tmp_path, monkeypatch):
    captured, _ = _curve(tmp_path / "a", 6)
    monkeypatch.setenv("PPSCI_HIP_GRAPH", "0")
    eager, solver = _curve(tmp_path / "b", 6)
    assert np.array_equal(captured, eager)
    assert solver.model.native().generation == 0
