"""A/B of the shape-specialised fused tile kernel that keeps the forward sweep's split planes for the reverse sweep (KEEP,
csrc/taylor_fused.inc) against the specialised kernel that recomputes them, IN ONE PROCESS (same card, same clocks: the drift
between processes cancels): the primary config (Allen-Cahn, 4 x 64 tanh, 100 000 points), one engine and one plan per setting of
ppsci_set_fused_keep_planes, alternating blocks of launches timed with HIP events.

    python tools/fused_keep_ab.py [points] [pairs] [launches per block]      (defaults 100000 10 40)

One JSON line per block pair and quantity ("main": run_main, the tile kernel alone; "step": whole train_steps) with the medians
and the min / max of both blocks, then one summary line per quantity with the verdict of the rule
    keep median < recompute median in EVERY pair, and by more than the larger min-max spread of the two series of medians."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from paddlescience_amd import _lib as L  # noqa: E402
from paddlescience_amd import hotpath as hp  # noqa: E402
from paddlescience_amd.engine import Engine, FusedConstraint  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 10
block = int(sys.argv[3]) if len(sys.argv) > 3 else 40
dev = torch.device("cuda", 0)
flat = bench.bench_weights(2, [64] * 4, 1)
X = np.random.default_rng(42).uniform([0, -1], [1, 1], (n, 2)).astype(np.float32)
lay = hp.NetLayout(2, 4, 64, 1, "tanh")


def make(keep):
    L.lib().ppsci_set_fused_keep_planes(keep)  # read when the launch is planned (the first train_step)
    xs = [torch.tensor(X[:, j].copy(), device=dev) for j in range(2)]
    cst = FusedConstraint("EQ", lay, hp.StreamSpec([[0.0, 1.0], [1.0, 0.0]], 1), bench.allen_cahn_program(n), xs, [], ["allen_cahn"])
    eng = Engine(lay, torch.tensor(flat, device=dev))
    for _ in range(5):
        eng.train_step([cst], 1e-3)
    torch.cuda.synchronize()
    assert cst._step_plan.specialised and cst._step_plan.keep_planes == bool(keep), "the plan did not take the kernel the switch asks for"
    return eng, cst


sides = {"recompute": make(0), "keep": make(1)}
L.lib().ppsci_set_fused_keep_planes(1)


def stats(ts):
    us = np.asarray(ts) * 1e6
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(us.min()), 2), "max_us": round(float(us.max()), 2)}


for _ in range(5):  # clocks and caches warm before the first timed block (both sides alike)
    for eng, cst in sides.values():
        bench.time_events_list(cst._step_plan.run_main, block)
summary = {}
for what in ("main", "step"):
    med = {"recompute": [], "keep": []}
    for pair in range(pairs):
        row = {"what": what, "pair": pair, "points": n, "launches": block}
        for side, (eng, cst) in sides.items():
            fn = cst._step_plan.run_main if what == "main" else (lambda e=eng, c=cst: e.train_step([c], 1e-3))
            fn()
            row[side] = stats(bench.time_events_list(fn, block))
            med[side].append(row[side]["median_us"])
        print(json.dumps(row), flush=True)
    g, s = np.asarray(med["recompute"]), np.asarray(med["keep"])
    spread = max(float(g.max() - g.min()), float(s.max() - s.min()))
    summary[what] = {"what": what, "summary": True, "recompute_median_us": round(float(np.median(g)), 2),
                     "keep_median_us": round(float(np.median(s)), 2), "spread_us": round(spread, 2),
                     "lower_in_every_pair": bool((s < g).all()), "min_gain_us": round(float((g - s).min()), 2),
                     "gain_claimed": bool((s < g).all() and float((g - s).min()) > spread)}
    print(json.dumps(summary[what]), flush=True)
