"""Generates tests/golden/geofno.npz by executing the REFERENCE's own 1-D Fourier neural operator (ppsci/arch/geofno.py:
SpectralConv1d, FNO1d) under the torch-backed paddle shim (tests/golden/_paddle_shim.py + the FFT / einsum / complex / Conv1D /
pad / interpolate additions below; the shim file itself is not edited), in float64 and -- for the tolerances -- in float32.

    python tests/golden/make_geofno_golden.py

Cases (tests/geofno_common.CASES): `yaml` (the catheter model, B = 2, s = 2001), `odd` (odd and prime lengths, a length-changing
irfft), `nyq` (the Nyquist mode of the last layer is kept), `trunc` (spectrum truncated at n // 2 + 1 < modes).  Per case: the
reference's named_parameters() names and shapes and state_dict() keys, the output for the input and parameters that
geofno_common draws from the case's seed, and for L = sum(w * y) the gradient of every parameter and of the input.  The `yaml`
case keeps the small gradient tensors whole and, of each spectral-weight and w*.weight gradient, its norm and a fixed index
sample.  `<case>/ref32_err/<name>`: the rel-L2 error of the reference's float32 run of the same tensors against its float64
run (names: output, input, every parameter).  `train/*`: the reference model's L2RelLoss("sum") at each of 30 Adam steps (lr
1e-3, weight_decay 1e-4 as paddle's coupled L2 decay) on one fixed batch of 8 samples at the `odd` shape, in float64 and in
float32, and their difference `train/ref32_dev`."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.geofno_common import CASES, draw_inputs, draw_params, sample_index  # noqa: E402

CUR = [torch.float64]  # the precision of the run in progress (the shim's DTYPE follows it)


def install_geofno_shim():
    import _paddle_shim as S

    S.import_hotpath()
    paddle = sys.modules["paddle"]
    nn = sys.modules["paddle.nn"]
    F = sys.modules["paddle.nn.functional"]
    init = sys.modules["paddle.nn.initializer"]

    class Spectrum(torch.Tensor):
        """paddle's Tensor.real() / .imag() are methods."""

        def real(self):
            return torch.real(self.as_subclass(torch.Tensor))

        def imag(self):
            return torch.imag(self.as_subclass(torch.Tensor))

    fft = types.ModuleType("paddle.fft")
    fft.rfft = lambda x: torch.fft.rfft(x).as_subclass(Spectrum)
    fft.irfft = lambda x, n=None: torch.fft.irfft(x.as_subclass(torch.Tensor), n=n)
    sys.modules["paddle.fft"] = fft
    paddle.fft = fft
    paddle.rand = lambda shape: torch.rand(tuple(shape), dtype=CUR[0])
    paddle.zeros = lambda shape, dtype=None: torch.zeros(tuple(shape), dtype=CUR[0])
    paddle.complex = torch.complex
    paddle.einsum = lambda eq, *ops: torch.einsum(eq, *[o.as_subclass(torch.Tensor) for o in ops])
    paddle.unsqueeze = lambda x, axis: torch.unsqueeze(x, axis)
    paddle.as_complex = lambda x: torch.view_as_complex(x.contiguous())
    paddle.transpose = lambda x, perm: x.permute(*perm)
    plain_transpose = torch.Tensor.transpose
    torch.Tensor.transpose = lambda self, *a, perm=None: self.permute(*perm) if perm is not None else plain_transpose(self, *a)
    init.Assign = type("Assign", (), {"__init__": lambda self, value: None})  # (the values are set by the generator)
    F.gelu = lambda x, approximate=False: torch.nn.functional.gelu(x)
    F.pad = lambda x, pad, mode="constant", value=0.0, data_format="NCL": torch.nn.functional.pad(x, tuple(int(p) for p in pad), mode, value)
    F.interpolate = lambda x, size, mode, align_corners: torch.nn.functional.interpolate(x, size=list(size), mode=mode,
                                                                                        align_corners=align_corners)

    class Conv1D(S.Layer):
        def __init__(self, in_channels, out_channels, kernel_size, **k):
            super().__init__()
            assert kernel_size == 1
            w = torch.zeros(out_channels, in_channels, 1, dtype=CUR[0], requires_grad=True)
            w._is_param = True
            b = torch.zeros(out_channels, dtype=CUR[0], requires_grad=True)
            b._is_param = True
            self.weight, self.bias = w, b

        def forward(self, x):
            return torch.einsum("oi,bil->bol", self.weight[:, :, 0], x) + self.bias.reshape(1, -1, 1)

    nn.Conv1D = Conv1D
    return importlib.import_module("ppsci.arch.geofno"), S


def state_keys(layer, prefix=""):
    """paddle's Layer.state_dict order: own parameters, then the sublayers."""
    out = [prefix + k for k in layer._params]
    for n, s in layer._subs.items():
        out += state_keys(s, prefix + n + ".")
    return out


def build(mod, S, c, dtype, vals=None):
    CUR[0] = S.DTYPE = dtype
    model = mod.FNO1d(**c["kw"])
    named = list(model.named_parameters())
    if vals is None:
        vals = draw_params([(k, p.shape) for k, p in named], c["kw"]["width"], c["seed"])
    with torch.no_grad():
        for k, p in named:
            assert p.dtype == dtype, (k, p.dtype)
            p.copy_(torch.tensor(vals[k]).to(dtype))
    return model, named, vals


def run(mod, S, c, dtype, x32, w):
    model, named, vals = build(mod, S, c, dtype)
    x = torch.tensor(x32.astype(np.float64)).to(dtype).requires_grad_(True)
    y = model({"input": x})["output"]
    assert y.dtype == dtype
    grads = torch.autograd.grad((y * torch.tensor(w).to(dtype)).sum(), [p for _, p in named] + [x])
    res = {"output": y.detach().double().numpy(), "input": grads[-1].double().numpy()}
    for (k, _), g in zip(named, grads):
        res[k] = g.double().numpy()
    return model, named, res


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def rel_loss(x, y):
    b = x.shape[0]
    return (torch.linalg.norm((x - y).reshape(b, -1), dim=1) / torch.linalg.norm(y.reshape(b, -1), dim=1)).sum()


def train_batch(c):
    """8 smooth wall curves of 37 points and a causal, mildly non-linear functional of them on 29 points."""
    rng = np.random.default_rng(77)
    s, n = c["s"], c["kw"]["output_np"]
    t = np.linspace(0, 1, s)
    amp, ph = rng.uniform(0.5, 1.5, (8, 1)), rng.uniform(0, np.pi, (8, 1))
    curve = amp * np.sin(2 * np.pi * t[None] + ph)
    resp = np.cumsum(curve, 1) / s + 0.3 * curve ** 2
    lab = np.stack([np.interp(np.linspace(0, 1, n), t, r) for r in resp])
    xs = np.stack([curve, np.broadcast_to(t[None], curve.shape)], -1).astype(np.float32)
    return xs, lab[..., None].astype(np.float32)


def train(mod, S, c, dtype, xs, ys):
    model, named, _ = build(mod, S, c, dtype)
    xt, yt = torch.tensor(xs.astype(np.float64)).to(dtype), torch.tensor(ys.astype(np.float64)).to(dtype)
    # paddle.optimizer.Adam(weight_decay=c) spelled out: g += c p (L2Decay), then Adam with bias correction.  (torch.optim.Adam
    # counts its steps with `step += 1`, which the shim turns into a rebinding: its bias correction would stay at step 1.)
    params = [p for _, p in named]
    lr, wd, b1, b2, eps = 1e-3, 1e-4, 0.9, 0.999, 1e-8
    m, v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    hist = []
    for t in range(1, 31):
        loss = rel_loss(model({"input": xt})["output"], yt)
        hist.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, params)
        with torch.no_grad():
            for p, g, mi, vi in zip(params, grads, m, v):
                g = g + wd * p
                mi.mul_(b1).add_(g, alpha=1 - b1)
                vi.mul_(b2).addcmul_(g, g, value=1 - b2)
                p.sub_(lr * (mi / (1 - b1 ** t)) / ((vi / (1 - b2 ** t)).sqrt() + eps))
    return np.array(hist, dtype=np.float64)


def main():
    mod, S = install_geofno_shim()
    out = {}
    for name, c in CASES.items():
        x32, w = draw_inputs(name)
        model, named, r64 = run(mod, S, c, torch.float64, x32, w)
        _, _, r32 = run(mod, S, c, torch.float32, x32, w)
        out[f"{name}/names"] = np.array([k for k, _ in named])
        out[f"{name}/shapes"] = np.array([",".join(str(v) for v in p.shape) for _, p in named])
        out[f"{name}/state_keys"] = np.array(state_keys(model))
        out[f"{name}/y"] = r64["output"]
        worst = 0.0
        for k in r64:
            e = rel(r32[k], r64[k])
            worst = max(worst, e)
            out[f"{name}/ref32_err/{k}"] = np.array(e)
            if k == "output":
                continue
            if name == "yaml" and ("weights1" in k or (k.startswith("w") and k.endswith(".weight"))):
                idx = sample_index(k, r64[k].size)
                out[f"{name}/grad_norm/{k}"] = np.array(np.linalg.norm(r64[k].ravel()))
                out[f"{name}/grad_sample/{k}"] = r64[k].ravel()[idx]
            else:
                out[f"{name}/grad/{k}"] = r64[k]
        print(name, len(named), "params, |y| max", float(np.abs(r64["output"]).max()), "float32 reference: output",
              f"{rel(r32['output'], r64['output']):.2e}", "worst", f"{worst:.2e}")
    c = CASES["odd"]
    xs, ys = train_batch(c)
    h64, h32 = train(mod, S, c, torch.float64, xs, ys), train(mod, S, c, torch.float32, xs, ys)
    out["train/x"], out["train/y"] = xs, ys
    out["train/loss64"], out["train/loss32"], out["train/ref32_dev"] = h64, h32, np.abs(h32 - h64)
    print("training:", h64[0], "->", h64[-1], "float32 deviation", np.abs(h32 - h64).min(), "..", np.abs(h32 - h64).max())
    np.savez_compressed(os.path.join(HERE, "geofno.npz"), **out)
    print("geofno.npz", os.path.getsize(os.path.join(HERE, "geofno.npz")), "bytes")


if __name__ == "__main__":
    main()
