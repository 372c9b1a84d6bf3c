"""Times one steady-state FNO1d (Geo-FNO) step -- executor forward, reverse (with its gradient row sums) and the fused Adam update
of the flat parameter buffer -- with HIP events, at the shape of examples/catheter_geofno.py by default:

    python tools/geofno_step.py [--batch 20] [--points 2001] [--width 64] [--modes 64] [--padding 100] [--steps 100] [--warmup 20]
Prints one JSON line (ms per step, launches per step).  --torch-baseline times a restatement of the same step with torch's
library operators (rfft / einsum / irfft / conv1d / interpolate, autograd, torch.optim.Adam) on the same device instead: a figure
to put beside the first one, never imported by the package."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ppsci  # noqa: E402
from paddlescience_amd import hotpath as hp  # noqa: E402


def torch_step(model, a, dev):
    """The reference forward (geofno.py:167-205) in torch operators on copies of the model's parameters."""
    F = torch.nn.functional
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters()}
    opt = torch.optim.Adam(list(P.values()), lr=1e-4)
    M, n, pad = a.modes, a.output_np, a.padding

    def spectral(h, k, size):
        W = torch.complex(P[f"conv{k}.weights1_real"], P[f"conv{k}.weights1_imag"])
        ft = torch.fft.rfft(h)
        out = torch.zeros(h.shape[0], h.shape[1], h.shape[-1] // 2 + 1, dtype=torch.complex64, device=dev)
        out[:, :, :M] = torch.einsum("bix,iox->box", ft[:, :, :M], W)
        return torch.fft.irfft(out, n=size)

    def forward(x):
        h = F.pad((x @ P["fc0.weight"] + P["fc0.bias"]).permute(0, 2, 1), (0, pad))
        for k in range(4):
            h = F.gelu(spectral(h, k, h.shape[-1]) + F.conv1d(h, P[f"w{k}.weight"], P[f"w{k}.bias"]))
        h = h[..., :-pad]
        h = spectral(h, 4, n) + F.interpolate(h, size=[n], mode="linear", align_corners=True)
        return F.gelu(h.permute(0, 2, 1) @ P["fc1.weight"] + P["fc1.bias"]) @ P["fc2.weight"] + P["fc2.bias"]

    def step(x, gy):
        opt.zero_grad(set_to_none=True)
        forward(x).backward(gy)
        opt.step()

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--points", type=int, default=2001)
    ap.add_argument("--output-np", type=int, default=2001)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--padding", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-baseline", action="store_true")
    a = ap.parse_args()
    model = ppsci.arch.FNO1d(modes=a.modes, width=a.width, padding=a.padding, output_np=a.output_np)
    dev = model.flat_params.device
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.uniform(-1, 1, (a.batch, a.points, 2)).astype(np.float32)).to(dev)
    gy = torch.full((a.batch, a.output_np, 1), 1e-3, dtype=torch.float32, device=dev)
    if a.torch_baseline:
        tstep = torch_step(model, a, dev)
        step = lambda t: tstep(x, gy)  # noqa: E731
        launches = None
    else:
        nat = model.native()
        m, v = torch.zeros_like(model.flat_params), torch.zeros_like(model.flat_params)

        def step(t):
            nat.forward(x)
            nat.backward(gy)
            hp.adam_step(model.flat_params, model.flat_grad, m, v, 1e-4, t)

        # forward: lift, 5 x (analysis, mix, layer), head; reverse: head_pre, head layer, fc1 rows, 5 x (analysis, mix, spectral weight
        # gradient, layer), 4 x convolution rows, lift, row sums; + Adam
        launches = (1 + 15 + 1) + (3 + 20 + 4 + 1 + 1) + 1
    for t in range(1, a.warmup + 1):
        step(t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(a.warmup + 1, a.warmup + a.steps + 1):
        step(t)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(shape=[a.batch, a.points, 2], output_np=a.output_np, width=a.width, modes=a.modes, padding=a.padding,
                          torch_baseline=bool(a.torch_baseline), ms_per_step=round(e0.elapsed_time(e1) / a.steps, 4), steps=a.steps,
                          launches_per_step=launches, n_params=int(model.flat_params.numel()))))


if __name__ == "__main__":
    main()
