"""The training step of a SPINN constraint on the GENERAL grid path (csrc/spinn_jet.inc + the epilogue VM) in isolation: the nets
of bench.py's SPINN configuration (3 x ModifiedMLP 1 -> 64 x 4 -> 32, tanh) on the 128^3 grid, timed with HIP events over 200
steps after 50, with the launches per step and the HBM bytes per step that follow from the shapes.

    python tools/spinn_jet_step.py                 Klein-Gordon residual u_tt - u_xx - u_yy + u*u (4 streams)
    python tools/spinn_jet_step.py --helmholtz     the Helmholtz residual on the four-coefficient path and on the general path
                                                   (PPSCI_SPINN_JET=1), same process, alternating blocks of steps
    python tools/spinn_jet_step.py --steps 50 --warmup 10 --nc 128     (for a profiler run)
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ppsci  # noqa: E402
from paddlescience_amd.engine import step_with_adam  # noqa: E402
from ppsci.equation.pde.helmholtz import hvp_revrev  # noqa: E402

# launches of one step of one constraint (one rank, plain Adam: the row sums and the update are one launch)
LAUNCHES = {"general": ["modmlp_fwd (3 nets)", "spinn_jet_fwd", "epilogue", "spinn_jet_bwd", "spinn_jet_fbar_sum", "modmlp_bwd (3 nets)",
                        "reduce_rows_multi_adam"],
            "linear": ["modmlp_fwd (3 nets)", "spinn_grid_fwd", "spinn_grid_bwd", "spinn_fbar_sum", "modmlp_bwd (3 nets)",
                       "reduce_rows_multi_adam"]}


def hbm_bytes(path, total, nq, n_aux):
    """Grid traffic per step from the shapes (the factor tables and the nets' few hundred points stay in cache)."""
    if path == "linear":  # label read, adjoint written once and read by the three axes
        return 4 * total * (1 + 1 + 3)
    # U written and read, Ubar written and read by the three axes, the label / weight grids read
    return 4 * total * (nq * (1 + 1 + 1 + 3) + n_aux)


def build(model, tmp, nc, which, general):
    rng = np.random.default_rng(42)
    keys = model.input_keys
    data = {k: rng.uniform(-1, 1, (nc, 1)).astype(np.float32) for k in keys}
    lab = {which: rng.standard_normal((nc, nc, nc, 1)).astype(np.float32)}
    f = model.forward_tensor
    if which == "helmholtz":
        eq = ppsci.equation.Helmholtz(3, 1.0)
        eq.model = model
        exprs = eq.equations
    else:
        def kg(d):
            a, b, c = (d[k] for k in keys)
            return (hvp_revrev(lambda a_: f(a_, b, c), (a,)) - hvp_revrev(lambda b_: f(a, b_, c), (b,))
                    - hvp_revrev(lambda c_: f(a, b, c_), (c,)) + d["u"] * d["u"])
        exprs = {which: kg}
    os.environ["PPSCI_SPINN_JET"] = "1" if general else "0"
    pde = ppsci.constraint.SupervisedConstraint(
        {"dataset": {"name": "ContinuousNamedArrayDataset", "input": lambda: data, "label": lambda d: lab}},
        output_expr=exprs, loss=ppsci.loss.MSELoss("mean"), name="PDE")
    opt = ppsci.optimizer.Adam(1e-3)(model)
    solver = ppsci.solver.Solver(model, {"PDE": pde}, os.path.join(tmp, f"{which}{int(general)}"), opt, epochs=1, iters_per_epoch=1)
    cc = solver._compiled["PDE"]
    cc.bind(data, lab)
    return lambda: step_with_adam(solver.engine, [cc], opt, model.flat_params), cc


def timed(step, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps  # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--helmholtz", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--nc", type=int, default=128)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "spinn_jet_step.py times the device kernels"
    np.random.seed(111)
    total = a.nc ** 3
    with tempfile.TemporaryDirectory() as tmp:
        if not a.helmholtz:
            model = ppsci.arch.SPINN(("t", "x", "y"), ("u",), 32, 4, 64, "tanh")
            step, cc = build(model, tmp, a.nc, "klein_gordon", True)
            for _ in range(a.warmup):
                step()
            ms = timed(step, a.steps)
            nq, n_aux = len(cc.jet.orders), len(cc.aux)
            out = {"residual": "klein_gordon", "grid": a.nc, "streams": nq, "ms_per_step": ms, "points_per_s": total / ms * 1e3,
                   "launches_per_step": len(LAUNCHES["general"]), "launches": LAUNCHES["general"],
                   "hbm_bytes_per_step": hbm_bytes("general", total, nq, n_aux),
                   "hbm_gb_per_s_at_step_time": hbm_bytes("general", total, nq, n_aux) / ms / 1e6}
        else:
            model = ppsci.arch.SPINN(("x", "y", "z"), ("u",), 32, 4, 64, "tanh")
            lin, _ = build(model, tmp, a.nc, "helmholtz", False)
            gen, cc = build(model, tmp, a.nc, "helmholtz", True)
            for _ in range(a.warmup):
                lin()
                gen()
            blocks, per = 4, max(1, a.steps // 4)
            t = {"linear": [], "general": []}
            for _ in range(blocks):  # alternating blocks: both paths see the same clocks and neighbours
                t["linear"].append(timed(lin, per))
                t["general"].append(timed(gen, per))
            nq, n_aux = len(cc.jet.orders), len(cc.aux)
            out = {"residual": "helmholtz", "grid": a.nc, "streams": nq,
                   "linear": {"ms_per_step": float(np.mean(t["linear"])), "blocks": t["linear"],
                              "launches_per_step": len(LAUNCHES["linear"]), "hbm_bytes_per_step": hbm_bytes("linear", total, 0, 0)},
                   "general": {"ms_per_step": float(np.mean(t["general"])), "blocks": t["general"],
                               "launches_per_step": len(LAUNCHES["general"]),
                               "hbm_bytes_per_step": hbm_bytes("general", total, nq, n_aux)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
