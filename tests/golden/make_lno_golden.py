"""Generates tests/golden/lno.npz by executing the REFERENCE's own Laplace neural operator (ppsci/arch/lno.py: Laplace, LNO,
with base.py and activation.py) in float64 under the torch-backed paddle shim (tests/golden/_paddle_shim.py + the FFT / einsum /
complex / Conv3D / InstanceNorm3D / buffer additions below; the shim file itself is not edited).

    python tests/golden/make_lno_golden.py

Cases: (a) `yaml`: the model of examples/brusselator3d/conf/brusselator3d.yaml at B = 1 on 39 x 14 x 14 with its T / X / Y grids;
(b) `small`: 8 x 6 x 5, C = 4, modes (3, 2, 2), 16 hidden features, sin, no norm, B = 3; (c) `grid`: as (b) with use_grid, use_norm
and tanh.  Per case: the reference's named_parameters() (names, shapes, values drawn float32-representable here) and
state_dict() keys, the buffers, the input (float32), the output, a random cotangent w and, for L = sum(w * y), the gradient of
every parameter and of the input; for (b) also the Laplace layer's x1 and x2 on its input, and the loss before / after 30 AdamW
steps (lr 5e-3, weight_decay 1e-4, L2RelLoss("sum")) of the reference model on a fixed batch of 8 samples in float64."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

D = torch.float64
MIN_POLE_GAP = 5e-4


def grids_yaml():
    return (np.linspace(0, 19, 39).reshape(1, 39), np.linspace(0, 1, 28).reshape(1, 28)[:, :14],
            np.linspace(0, 1, 28).reshape(1, 28)[:, :14])


def grids_small():
    return (np.linspace(0, 2, 8).reshape(1, 8), np.linspace(0, 1, 6).reshape(1, 6), np.linspace(0, 1.5, 5).reshape(1, 5))


CASES = {
    "yaml": dict(grids=grids_yaml, B=1, fd=4, seed=11,
                 kw=dict(width=8, modes=(4, 4, 4), in_features=4, hidden_features=64, activation="relu", use_norm=True,
                         use_grid=False)),
    "small": dict(grids=grids_small, B=3, fd=2, seed=12,
                  kw=dict(width=4, modes=(3, 2, 2), in_features=2, hidden_features=16, activation="sin", use_norm=False,
                          use_grid=False)),
    "grid": dict(grids=grids_small, B=3, fd=2, seed=13,
                 kw=dict(width=4, modes=(3, 2, 2), in_features=5, hidden_features=16, activation="tanh", use_norm=True,
                         use_grid=True)),
}


def install_lno_shim():
    import _paddle_shim as S

    S.import_hotpath()
    paddle = sys.modules["paddle"]
    nn = sys.modules["paddle.nn"]
    fft = types.ModuleType("paddle.fft")
    fft.fftn = lambda x, s=None, axes=None: torch.fft.fftn(x, s=s, dim=axes)
    fft.ifftn = lambda x, s=None, axes=None: torch.fft.ifftn(x, s=s, dim=axes)
    fft.fftfreq = lambda n, d=1.0: torch.fft.fftfreq(n, d, dtype=D)
    sys.modules["paddle.fft"] = fft
    paddle.fft = fft
    paddle.complex64 = torch.complex128  # fixture precision
    paddle.einsum = torch.einsum
    paddle.as_complex = lambda x: torch.view_as_complex(x.contiguous())
    paddle.real = lambda x: x.real
    paddle.exp = torch.exp
    paddle.subtract = lambda a, b: a - b
    paddle.divide = lambda a, b: a / b
    paddle.to_tensor = lambda v, dtype=None, **k: torch.as_tensor(v, dtype=dtype if isinstance(dtype, torch.dtype) else D)
    paddle.linspace = lambda start, stop, num: torch.linspace(start, stop, num, dtype=D)
    paddle.transpose = lambda x, perm: x.permute(*perm)
    torch.Tensor.astype = lambda self, dt: self.to(dt)
    torch.Tensor.tile = lambda self, reps: self.repeat(*reps)

    def register_buffer(self, name, tensor, persistable=True):
        self.__dict__.setdefault("_bufs", {})[name] = tensor
        object.__setattr__(self, name, tensor)

    S.Layer.register_buffer = register_buffer

    def plist_append(self, p):
        self._params[str(len(self._plist))] = p
        self._plist.append(p)
        return self

    S.ParameterList.append = plist_append
    S.ParameterList.__getitem__ = lambda self, i: self._plist[i]

    class Conv3D(S.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, data_format="NCDHW", **k):
            super().__init__()
            assert kernel_size == 1 and data_format == "NCDHW"
            w = torch.zeros(out_channels, in_channels, 1, 1, 1, dtype=D, requires_grad=True)
            w._is_param = True
            b = torch.zeros(out_channels, dtype=D, requires_grad=True)
            b._is_param = True
            self.weight, self.bias = w, b

        def forward(self, x):
            w = self.weight.reshape(self.weight.shape[0], self.weight.shape[1])
            return torch.einsum("oi,bi...->bo...", w, x) + self.bias.reshape(1, -1, 1, 1, 1)

    class InstanceNorm3D(S.Layer):
        def __init__(self, num_features, epsilon=1e-5, weight_attr=None, bias_attr=None, **k):
            super().__init__()
            assert weight_attr is False and bias_attr is False
            self.eps = epsilon

        def forward(self, x):
            return torch.nn.functional.instance_norm(x, eps=self.eps)

    nn.Conv3D, nn.InstanceNorm3D = Conv3D, InstanceNorm3D
    init = sys.modules["ppsci.utils.initializer"]

    def uniform_(t, a=0.0, b=1.0):
        # (Laplace._init_weights RETURNS this call's result: fill and hand the same tensor back)
        with torch.no_grad():
            t.uniform_(a, b)
        return t

    init.uniform_ = uniform_
    return importlib.import_module("ppsci.arch.lno"), S


def state_keys(layer, prefix=""):
    """paddle's Layer.state_dict order: own parameters, own persistable buffers, then the sublayers."""
    out = [prefix + k for k in layer._params]
    out += [prefix + k for k in layer.__dict__.get("_bufs", {})]
    for n, s in layer._subs.items():
        out += state_keys(s, prefix + n + ".")
    return out


def draw(named, C, rng, use_norm):
    """Poles and residues as the reference initialises them; fc / conv weights He-like.  Without the instance norms the Laplace
    layer's output reaches fc1 at its raw scale of ~1e3-1e4, where an fp32 input alone (relative rounding 6e-8) moves a
    sin / tanh pre-activation by 1e-4 or more: fc1.weight starts 1e-3 smaller there and is then normalised by `unit_preact`, so
    that the comparison measures the kernels and not the conditioning of sin(1e3 x)."""
    out = {}
    for name, p in named:
        shp = tuple(p.shape)
        if name == "fc1.weight" and not use_norm:
            v = 1e-3 * rng.normal(0.0, np.sqrt(2.0 / (shp[0] + shp[1])), shp)
        elif "weights_" in name:  # the reference's initialisation, lno.py:54, :80-81
            v = rng.uniform(0.0, 1.0 / (C * C), shp)
        elif name.endswith("bias"):
            v = rng.normal(0.0, 0.1, shp)
        elif name == "conv.weight":
            v = rng.normal(0.0, np.sqrt(1.0 / shp[1]), shp)
        else:
            v = rng.normal(0.0, np.sqrt(2.0 / (shp[0] + shp[1])), shp)
        out[name] = np.asarray(v).astype(np.float32).astype(np.float64)
    return out


def unit_preact(model, vals, x):
    """Rescales fc1.weight (float32-representable) so that the reference's own fc1 output, without its bias, has rms 1 on the
    case's input: the activation is evaluated where networks evaluate it, whatever scale the Laplace layer's output has."""
    with torch.no_grad():
        h = model.transpoe_to_NCDHW(model.fc0(x))
        u = model.transpoe_to_NDHWC(model.laplace(h) + model.conv(h))
        rms = float((u @ model.fc1.weight).pow(2).mean().sqrt())
        vals["fc1.weight"] = (vals["fc1.weight"] / rms).astype(np.float32).astype(np.float64)
        model.fc1.weight.copy_(torch.tensor(vals["fc1.weight"]))


def pole_gap(model):
    lp = model.laplace
    gap = np.inf
    for d in range(3):
        mu = torch.complex(lp.weights_pole_real[d][..., 0], lp.weights_pole_imag[d][..., 0]).detach()
        lam = lp.lambdas[d].reshape(-1, 1, 1, 1)
        gap = min(gap, float((lam - mu).abs().min()))
    return gap


def build(mod, c):
    T, X, Y = (torch.tensor(g, dtype=D) for g in c["grids"]())
    model = mod.LNO(("input",), ("output",), T=T, data=(X, Y), **c["kw"])
    named = list(model.named_parameters())
    vals = draw(named, c["kw"]["width"], np.random.default_rng(c["seed"]), c["kw"]["use_norm"])
    with torch.no_grad():
        for n, p in named:
            p.copy_(torch.tensor(vals[n]))
    return model, named, vals


def rel_loss(x, y):
    b = x.shape[0]
    return (torch.linalg.norm((x - y).reshape(b, -1), dim=1) / torch.linalg.norm(y.reshape(b, -1), dim=1)).sum()


def main():
    mod, S = install_lno_shim()
    out = {}
    for name, c in CASES.items():
        model, named, vals = build(mod, c)
        gap = pole_gap(model)
        # (min |lambda - mu| bounds |A_d| by 2000 and with it the conditioning of the comparison; the seeds in CASES satisfy it)
        assert gap >= MIN_POLE_GAP, f"{name}: min |lambda - mu| = {gap:.3e}: pick another seed"
        rng = np.random.default_rng(1000 + c["seed"])
        n = [g.shape[1] for g in c["grids"]()]
        x32 = rng.uniform(-1, 1, (c["B"], *n, c["fd"])).astype(np.float32)
        x = torch.tensor(x32.astype(np.float64), requires_grad=True)
        if not c["kw"]["use_norm"]:
            unit_preact(model, vals, x.detach())
        y = model({"input": x})["output"]
        w = rng.standard_normal(tuple(y.shape))
        params = [p for _, p in named]
        grads = torch.autograd.grad((y * torch.tensor(w)).sum(), params + [x])
        out[f"{name}/names"] = np.array([k for k, _ in named])
        out[f"{name}/state_keys"] = np.array(state_keys(model))
        out[f"{name}/pole_gap"] = np.array(gap)
        for (k, _), g in zip(named, grads):
            out[f"{name}/param/{k}"] = vals[k]
            out[f"{name}/grad/{k}"] = g.detach().numpy()
        for k, b in model.laplace.__dict__["_bufs"].items():
            out[f"{name}/buffer/laplace.{k}"] = b.detach().numpy()
        out[f"{name}/x"] = x32
        out[f"{name}/y"] = y.detach().numpy()
        out[f"{name}/w"] = w
        out[f"{name}/grad_x"] = grads[-1].detach().numpy()
        print(name, len(named), "params, pole gap", f"{gap:.3e}", "|y|", float(y.abs().max()))
        if name != "small":
            continue
        # the Laplace layer alone, its two parts separately (lno.py:160-187)
        z32 = rng.uniform(-1, 1, (c["B"], c["kw"]["width"], *n)).astype(np.float32)
        z = torch.tensor(z32.astype(np.float64))
        lap = model.laplace
        alpha = torch.fft.fftn(z, dim=[-3, -2, -1])
        r1, r2 = lap.output_PR(alpha)
        x1 = torch.fft.ifftn(r1, s=tuple(z.shape[-3:])).real
        full = lap(z)
        out[f"{name}/lap_z"] = z32
        out[f"{name}/lap_x1"] = x1.detach().numpy()
        out[f"{name}/lap_x2"] = (full - x1).detach().numpy()
        # learning: 30 AdamW steps of the reference model on a fixed batch of 8 (a smooth forcing -> response pair)
        tg = np.linspace(0, 1, n[0])
        amp, ph = rng.uniform(0.5, 1.5, (8, 1)), rng.uniform(0, np.pi, (8, 1))
        forcing = amp * np.sin(2 * np.pi * tg[None] + ph)                                       # [8, n1]
        resp = np.cumsum(forcing, 1) / n[0] + 0.3 * forcing ** 2                               # a causal, mildly non-linear map
        xs = np.stack([np.broadcast_to(forcing[:, :, None, None], (8, *n)),
                       np.broadcast_to(np.linspace(0, 1, n[1])[None, None, :, None], (8, *n))], -1).astype(np.float32)
        ys = (resp[:, :, None, None] * (1 + 0.2 * np.linspace(0, 1, n[2]))[None, None, None, :]
              * np.ones((1, 1, n[1], 1)))[..., None].astype(np.float32)
        xt, yt = torch.tensor(xs.astype(np.float64)), torch.tensor(ys.astype(np.float64))
        opt = torch.optim.AdamW(params, lr=5e-3, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8)
        hist = []
        for step in range(31):
            loss = rel_loss(model({"input": xt})["output"], yt)
            hist.append(float(loss))
            if step == 30:
                break
            opt.zero_grad()
            loss.backward()
            opt.step()
        assert hist[30] <= 0.8 * hist[0], f"the reference run must lose at least 20 % of its loss: {hist[0]} -> {hist[30]}"
        out[f"{name}/train_x"], out[f"{name}/train_y"] = xs, ys
        out[f"{name}/train_loss"] = np.array([hist[0], hist[30]])
        print("  training:", hist[0], "->", hist[30])
    np.savez_compressed(os.path.join(HERE, "lno.npz"), **out)
    print("lno.npz", os.path.getsize(os.path.join(HERE, "lno.npz")), "bytes")


if __name__ == "__main__":
    main()
