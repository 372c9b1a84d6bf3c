"""Times one steady-state LNO step -- executor forward, reverse (with its gradient row sums) and the fused Adam update of the
flat parameter buffer -- with HIP events, at the shape of examples/brusselator3d_lno.py by default:

    python tools/lno_step.py [--batch 50] [--grid 39 14 14] [--width 8] [--modes 4 4 4] [--hidden 64] [--steps 200] [--warmup 50]
Prints one JSON line (ms per step, launches per step)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ppsci  # noqa: E402
from paddlescience_amd import hotpath as hp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--grid", type=int, nargs=3, default=[39, 14, 14])
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--modes", type=int, nargs=3, default=[4, 4, 4])
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--in-features", type=int, default=4)
    ap.add_argument("--activation", default="relu")
    ap.add_argument("--no-norm", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    n1, n2, n3 = a.grid
    T, X, Y = (np.linspace(0, hi, n).reshape(1, n) for hi, n in ((19, n1), (0.5, n2), (0.5, n3)))
    model = ppsci.arch.LNO(("input",), ("output",), a.width, tuple(a.modes), T, (X, Y), a.in_features, a.hidden, a.activation,
                           not a.no_norm)
    dev = model.flat_params.device
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.uniform(-1, 1, (a.batch, n1, n2, n3, a.in_features)).astype(np.float32)).to(dev)
    gy = torch.full((a.batch, n1, n2, n3, 1), 1e-3, dtype=torch.float32, device=dev)
    nat = model.native()
    m, v = torch.zeros_like(model.flat_params), torch.zeros_like(model.flat_params)

    def step(t):
        nat.forward(x)
        nat.backward(gy)
        hp.adam_step(model.flat_params, model.flat_grad, m, v, 1e-4, t)

    for t in range(1, a.warmup + 1):
        step(t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(a.warmup + 1, a.warmup + a.steps + 1):
        step(t)
    e1.record()
    torch.cuda.synchronize()
    # forward: lift, (norm), tables, dft, H, dft, analysis, channel sum, synthesis, (norm), head; reverse: head, (norm), dft, analysis,
    # channel sum, analysis, hbar, analysis, rho, synthesis, dft, (norm), lift, row sums; + Adam
    launches = (9 + (0 if a.no_norm else 2)) + (12 + (0 if a.no_norm else 2)) + 1
    print(json.dumps(dict(shape=[a.batch, n1, n2, n3], width=a.width, modes=a.modes, hidden=a.hidden,
                          ms_per_step=round(e0.elapsed_time(e1) / a.steps, 4), steps=a.steps, launches_per_step=launches,
                          n_params=int(model.flat_params.numel()))))


if __name__ == "__main__":
    main()
