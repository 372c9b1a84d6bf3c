"""Times one steady-state DeepONet step -- executor forward, reverse and the fused Adam update of the flat parameter
buffer -- with HIP events, at two shapes:

    he        the reference heat-exchanger config: four batches of 1000 points, branch 1 -> 256 x 9 -> 300 (x 2),
              trunk 2 -> 128 x 6 -> 300, swish, first-order streams in x and t (S = 3)
    deeponet  the reference DeepONet config: batch 10 000, m = 100 sensors, 40 x 1, tanh here (values only, S = 1)

    python tools/deeponet_step.py [--shape he|deeponet] [--steps 200] [--warmup 50]
Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ppsci  # noqa: E402
from paddlescience_amd import hotpath as hp  # noqa: E402


def build(shape):
    if shape == "he":
        model = ppsci.arch.HEDeepONets(("qm_h",), ("qm_c",), ("x", "t"), ("T_h", "T_c", "T_w"), 1, 1, 100, 9, 6, 256, 128,
                                       branch_activation="swish", trunk_activation="swish")
        batches, n, dirs, n2 = 4, 1000, [[1.0, 0.0], [0.0, 1.0]], 0
        rng = np.random.default_rng(0)
        inputs = {"qm_h": rng.uniform(0, 1, (n, 1)), "qm_c": rng.uniform(0, 1, (n, 1)), "x": rng.uniform(0, 1, (n, 1)),
                  "t": rng.uniform(0, 1, (n, 1))}
    else:
        model = ppsci.arch.DeepONet("u", "y", "G", 100, 40, 1, 1, 40, 40)
        batches, n, dirs, n2 = 1, 10000, [], 0
        rng = np.random.default_rng(0)
        inputs = {"u": rng.uniform(-1, 1, (n, 100)), "y": rng.uniform(0, 1, (n, 1))}
    dev = model.flat_params.device
    inputs = {k: torch.as_tensor(v.astype(np.float32)).to(dev) for k, v in inputs.items()}
    execs = []
    for _ in range(batches):
        ex = model.make_exec(dirs, n2, n)
        ex.set_inputs(inputs)
        execs.append(ex)
    return model, execs, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["he", "deeponet", "both"], default="both")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    for shape in (["he", "deeponet"] if a.shape == "both" else [a.shape]):
        model, execs, n = build(shape)
        dev = model.flat_params.device
        U = [torch.zeros((model.n_out * ex.S, n), dtype=torch.float32, device=dev) for ex in execs]
        Ubar = [torch.full_like(u, 1e-3) for u in U]
        grads = [torch.zeros(model.n_params, dtype=torch.float32, device=dev) for _ in execs]
        g = torch.zeros(model.n_params, dtype=torch.float32, device=dev)
        m, v = torch.zeros_like(g), torch.zeros_like(g)

        def step(t):
            for ex, u, ub, gr in zip(execs, U, Ubar, grads):
                ex.forward(model.flat_params, u, True)
                ex.backward(model.flat_params, ub, gr)
            if len(grads) > 1:
                hp.reduce_rows(torch.stack(grads), len(grads), model.n_params, g, False)
            else:
                g.copy_(grads[0])
            hp.adam_step(model.flat_params, g, m, v, 1e-4, t)

        for t in range(1, a.warmup + 1):
            step(t)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(a.warmup + 1, a.warmup + a.steps + 1):
            step(t)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        print(json.dumps(dict(shape=shape, ms_per_step=round(ms, 4), steps=a.steps, batches=len(execs), n=n, S=execs[0].S,
                              n_params=model.n_params)))


if __name__ == "__main__":
    main()
