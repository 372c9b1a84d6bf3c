"""arch/layer_by_layer.py, what PirateNet, ModifiedMLP, LayerwiseMLP and the DeepONets share: repeated steps of the two executors
tests/test_determinism.py does not cover (bitwise-equal gradients, the same partial-sum buffers in every pass), the flat
parameter store (state dict, rehome, seeded initialisation) and the engine's `layer_by_layer` route."""
import os

import numpy as np
import pytest
import sympy as sp
import torch

import ppsci
from paddlescience_amd.arch.layer_by_layer import LayerExec, LayerLayout
from tests.common import make_dev_fixture

dev = make_dev_fixture()

RWF = {"mean": 1.0, "std": 0.1}
HE = dict(heat_input_keys=("qm_h",), cold_input_keys=("qm_c",), trunk_input_keys=("x", "t"), output_keys=("T_h", "T_c", "T_w"),
          heat_num_loc=1, cold_num_loc=1, num_features=8, branch_num_layers=2, trunk_num_layers=3, branch_hidden_size=32,
          trunk_hidden_size=32, branch_activation="swish", trunk_activation="swish")


def _build(kind):
    """Hidden 32 behind a Fourier embedding of dim 16 (c0 != H), period embedding, factored layers, two outputs."""
    kw = dict(periods={"x": (2.0, False)}, fourier={"dim": 16, "scale": 1.0}, random_weight=RWF)
    if kind == "pirate":
        return ppsci.arch.PirateNet(("t", "x"), ("u", "v"), 2, 16, "tanh", periods={"x": (2.0, False)},
                                    fourier={"dim": 16, "scale": 2.0}, random_weight=RWF)
    if kind == "modified":
        return ppsci.arch.ModifiedMLP(("t", "x"), ("u", "v"), 2, 32, "tanh", **kw)
    if kind == "layerwise":
        return ppsci.arch.MLP(("t", "x"), ("u", "v"), 2, 32, "silu", **kw)
    return ppsci.arch.HEDeepONets(**HE)


def _fused(model, inp, eqs, tmp_path):
    n = next(iter(inp.values())).shape[0]
    lab = {k: np.random.default_rng(6).standard_normal((n, 1)).astype(np.float32) * 0.1 for k in eqs}
    cfg = {"dataset": {"name": "IterableNamedArrayDataset", "input": inp, "label": lab}}
    cst = ppsci.constraint.SupervisedConstraint(cfg, ppsci.loss.MSELoss("mean"), eqs, name="EQ")
    solver = ppsci.solver.Solver(model, {"EQ": cst}, str(tmp_path), ppsci.optimizer.Adam(1e-3)(model), epochs=1, iters_per_epoch=1)
    return solver, solver._compiled["EQ"].fused


def _points(n, keys):
    X = np.random.default_rng(5).uniform(-1, 1, (n, len(keys))).astype(np.float32)
    return {k: X[:, j:j + 1] for j, k in enumerate(keys)}


def _residual(outputs=("u", "v")):
    t, x = sp.symbols("t x")
    u, v = (sp.Function(k)(t, x) for k in outputs)
    return {"r": u.diff(t) + 0.3 * u.diff(x, 2) + v}  # one first-order and one second-order stream


@pytest.mark.parametrize("kind", ["modified", "layerwise"])
def test_repeated_steps_are_bitwise_equal_and_reuse_their_partial_buffers(kind, dev, tmp_path):
    ppsci.utils.misc.set_random_seed(7)
    model = _build(kind)
    assert type(model).__name__ == {"modified": "ModifiedMLP", "layerwise": "LayerwiseMLP"}[kind]
    n = 33
    solver, fused = _fused(model, _points(n, ("t", "x")), _residual(), tmp_path)
    ex = fused.nets[0]["exec"]
    assert isinstance(ex, LayerExec) and ex.NP == 48 and ex.S == 1 + ex.n1 + ex.n2 and ex.n1 >= 1 and ex.n2 == 1
    assert model.c0 == 16 != model.hidden and model._rwf
    if kind == "modified":
        assert ex.batched and ex.XB0 is not None and tuple(ex.XB0.shape) == (ex.S, 16, 48)
    else:
        assert not ex.batched
    handed, hand_out = [], ex._pbuf

    def recording(size, what):
        buf = hand_out(size, what)
        handed.append(buf.data_ptr())
        return buf

    ex._pbuf = recording
    grads, passes, allocated = [], [], []
    for _ in range(2):
        handed.clear()
        solver.engine.forward_backward([fused])
        grads.append(solver.engine.grad.detach().cpu().numpy().copy())
        passes.append(list(handed))
        allocated.append(len(ex._pbufs))
    assert np.abs(grads[0]).max() > 0 and grads[0].tobytes() == grads[1].tobytes()
    o, k = model._offsets["linears.1.weight_g"]  # (reached through the factored layers' pull-back)
    assert np.abs(grads[0][o:o + k]).max() > 0
    assert len(passes[0]) > 4 and passes[0] == passes[1] and allocated[0] == allocated[1]
    if ex.batched:  # every producer its own buffer
        assert len(set(passes[0])) == len(passes[0]) == allocated[0]
    else:  # the layers share the scratch: nothing is handed out of a per-producer list
        assert allocated[0] == 0 and set(passes[0]) <= {t.data_ptr() for t in ex._scratch.values() if t is not None}


def test_state_dict_round_trip_with_zero_dim_entries(dev):
    np.random.seed(1)
    a = _build("onet")
    np.random.seed(2)
    b = _build("onet")
    assert not torch.equal(a.flat_params, b.flat_params)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in a.state_dict().items()}
    zero_dim = [k for k, v in sd.items() if v.ndim == 0]
    assert "trunk_act.beta" in zero_dim and "heat_net.acts.0.beta" in zero_dim
    sd["trunk_act.beta"] = np.full((1,), 1.25, np.float32)  # a 0-d entry stored as [1]
    sd["extra"] = np.zeros(3, np.float32)
    del sd["b"]
    assert b.set_state_dict(sd) == (["b"], ["extra"])
    for k, v in b.state_dict().items():
        if k == "trunk_act.beta":
            assert v.dim() == 0 and float(v) == 1.25
        elif k != "b":
            assert np.array_equal(v.cpu().numpy(), sd[k]), k
    with pytest.raises(ValueError, match="shape mismatch for trunk_net.last_fc.bias"):
        b.set_state_dict({"trunk_net.last_fc.bias": np.zeros(5, np.float32)})
    with pytest.raises(ValueError, match="shape mismatch for trunk_act.beta"):
        b.set_state_dict({"trunk_act.beta": np.zeros(2, np.float32)})


@pytest.mark.parametrize("kind", ["pirate", "onet"])
def test_rehome_keeps_values_and_rebinds_views(kind, dev):
    np.random.seed(3)
    model = _build(kind)
    n = model.n_params
    before = model.flat_params.clone()
    names = [k for k, _ in model.named_parameters()]
    big = torch.full((n + 24,), 7.0, dtype=torch.float32, device=before.device)
    model.rehome(big[8:8 + n])
    assert model.flat_params.data_ptr() == big.data_ptr() + 32 and model.kernel_params is model.flat_params
    assert torch.equal(big[8:8 + n], before) and bool((big[:8] == 7).all()) and bool((big[8 + n:] == 7).all())
    assert [k for k, _ in model.named_parameters()] == names
    for k, v in model.named_parameters():
        o, c = model._offsets[k]
        assert v.data_ptr() == big.data_ptr() + 4 * (8 + o) and v.numel() == c, k
    model.parameters()[-1].fill_(0.5)  # a view writes the list's buffer
    o, c = model._offsets[names[-1]]
    assert bool((big[8 + o:8 + o + c] == 0.5).all())


# (number of parameters, sum |p|, sum p[i] * (i % 97 + 1)) in float64 of the seeded models as they were before the three
# initialisers became one.  A changed order of the draws from numpy's global RNG moves both sums in the first digits; 1e-6
# leaves room for nothing but numpy's float32 exp (the factored layers' g) differing in the last bit between CPUs.
CHECKSUMS = {
    "pirate": (2366, 549.1514109547388, 28753.050463895885),
    "modified": (2908, 522.3278908686698, 23621.604560428346),
    "layerwise": (1756, 288.38548059343884, 12093.205556521738),
    "onet": (6837, 1046.4074954448224, 275.9083396852511),
}


@pytest.mark.parametrize("kind", list(CHECKSUMS))
def test_seeded_construction_draws_in_the_same_order(kind, dev):
    ppsci.utils.misc.set_random_seed(1234)
    p = _build(kind).flat_params.detach().cpu().numpy().astype(np.float64)
    size, abs_sum, weighted = CHECKSUMS[kind]
    assert p.size == size
    assert float(np.abs(p).sum()) == pytest.approx(abs_sum, rel=1e-6)
    assert float(np.dot(p, (np.arange(p.size) % 97 + 1).astype(np.float64))) == pytest.approx(weighted, rel=1e-6)


@pytest.mark.parametrize("kind", list(CHECKSUMS))
def test_engine_takes_the_layer_by_layer_route(kind, dev, tmp_path):
    np.random.seed(4)
    model = _build(kind)
    n = 19
    if kind == "onet":
        inp = dict(_points(n, ("x", "t")), qm_h=np.full((n, 1), 0.3, np.float32), qm_c=np.full((n, 1), 0.6, np.float32))
        eqs = _residual(("T_h", "T_w"))
    else:
        inp, eqs = _points(n, ("t", "x")), _residual()
    assert isinstance(model.layout, LayerLayout) and model.layout.layer_by_layer and model.layout.desc(None) is None
    _, fused = _fused(model, inp, eqs, tmp_path)
    net = fused.nets[0]
    assert isinstance(net["exec"], LayerExec) and net["exec"].model is model
    assert net["desc"] is None and net["stash"] is None and net["grad_rows"] == 1
    assert tuple(net["grad_partials"].shape) == (1, model.n_params) and net["layout"].n_params == model.n_params


def test_nothing_reads_the_old_flag():
    import paddlescience_amd

    root = os.path.dirname(os.path.abspath(paddlescience_amd.__file__))
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(d, f)) as fh:
                    assert "is_pirate" not in fh.read(), os.path.join(d, f)
