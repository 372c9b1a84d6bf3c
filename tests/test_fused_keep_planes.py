"""Kept split planes in the shape-specialised fused tile kernel (csrc/taylor_fused.inc, template parameter KEEP).

A KEEP kernel writes the split planes of h_{L-3}, which the forward sweep publishes for the GEMM of layer L-2, a second time into
a third exchange buffer `kx`; reverse layer L-2 reads them there as the A operand of its Wbar GEMM instead of evaluating,
splitting and publishing h_{L-3} from the stash again.  At even depth the recomputed h_0 of reverse layer 1 goes to `kx` as well
and the WAR barrier in front of a tile's first publish is gone.  `ppsci_set_fused_keep_planes(0)` keeps every plan on the
specialised kernel that recomputes.  Checked here:
  * switch on against switch off: parameters after two steps, both gradients and both loss-term vectors are EQUAL
    (np.array_equal); the plan reports keep_planes True / False and specialised True in both;
  * two runs with the switch on are bit-identical;
  * plans that cannot keep planes report False and equal the switch-off result: S = 5 (the carve-up does not fit), L = 2 (nothing
    to keep), a plan with optional outputs (the generic kernel);
  * switch on agrees with the separate launches within the bound of tests/test_fused_specialised.py.
Nets: the primary one (even depth: the dropped barrier); odd depth with H < 64 (nothing left to recompute, `kx` written behind
the layer's barrier); L = 5 (two of three layers still recompute); S = 1.
Sizes: one ragged tile; 101 points on two workgroups (7 tiles, 4 + 3: `kx` is reused across tiles and the tile boundary runs
without its barrier); the neighbour test's 90 points on 4 workgroups (emulator) / 8 213 points on the full grid (device).
Reference: /root/reference/ppsci/solver/train.py:82-184 (one training step), equation/pde/allen_cahn.py:56-64."""
import numpy as np
import pytest
import torch

from paddlescience_amd import _lib as L
from paddlescience_amd import device
from paddlescience_amd import hotpath as hp
from paddlescience_amd.engine import Engine, FusedConstraint
from tests.common import make_dev_fixture, rel
from tests.test_one_launch import _program, _weights

dev = make_dev_fixture()

CASES = [  # (hidden layers, width, program)
    (4, 64, "allen_cahn"),  # primary; even depth, so the dropped barrier
    (3, 50, "allen_cahn"),  # odd depth, H < 64, nothing left to recompute
    (5, 64, "allen_cahn"),  # two of three layers still recomputed
    (3, 40, "value"),       # S = 1
]
INELIGIBLE = [  # (hidden layers, width, program, optional outputs)
    (3, 50, "laplace", False),    # S = 5
    (2, 40, "value", False),      # L = 2
    (4, 64, "allen_cahn", True),  # optional outputs: the generic kernel
]


def _sizes(dev):
    return [(5, 0), (101, 2)] + ([(90, 4)] if dev != "gpu" else [(8213, 0)])


def _constraint(d, kind, lay, n, seed):
    rng = np.random.default_rng(seed)
    ed, streams, n_aux = _program(kind, n)
    xs = [torch.tensor(rng.random(n, dtype=np.float32) * 2 - 1, device=d) for _ in range(2)]
    aux = [torch.tensor(rng.random(n, dtype=np.float32) + 0.5, device=d) for _ in range(n_aux)]
    return FusedConstraint(kind, lay, streams, ed, xs, aux, [f"k{i}" for i in range(ed.n_res)])


def _run(d, lay, kind, n, flat, steps, keep, max_grid=0, fused=True, step_outputs=False):
    lib = L.lib()
    lib.ppsci_set_fused_keep_planes(keep)
    lib.ppsci_set_max_grid(max_grid)
    try:
        params = torch.tensor(flat, device=d)
        eng = Engine(lay, params)
        eng.one_launch = fused
        c = _constraint(d, kind, lay, n, 101)
        c.step_outputs = step_outputs
        grads, losses = [], []
        for _ in range(steps):
            eng.train_step([c], 1e-2)
            grads.append(eng.grad.detach().cpu().numpy().copy())
            losses.append(c.loss_terms.detach().cpu().numpy().copy())
        plan = c._step_plan if fused else None
        return dict(p=params.detach().cpu().numpy(), g=grads, l=losses, keep=plan.keep_planes if plan else None,
                    spec=plan.specialised if plan else None)
    finally:
        lib.ppsci_set_fused_keep_planes(1)
        lib.ppsci_set_max_grid(0)


_REF = {}


def _pair(dev, depth, width, kind, n, max_grid, step_outputs=False):
    """(switch on, switch off), two steps each; computed once per case and size."""
    key = (dev, depth, width, kind, n, max_grid, step_outputs)
    if key not in _REF:
        d = device.get_device()
        lay = hp.NetLayout(2, depth, width, 1, "tanh")
        flat = _weights(lay, 13)
        _REF[key] = (_run(d, lay, kind, n, flat, 2, 1, max_grid, step_outputs=step_outputs),
                     _run(d, lay, kind, n, flat, 2, 0, max_grid, step_outputs=step_outputs), lay, flat)
    return _REF[key]


def _differing(a, b):
    rows = [("p", a["p"], b["p"])] + [(f"g{i}", x, y) for i, (x, y) in enumerate(zip(a["g"], b["g"]))] + \
           [(f"l{i}", x, y) for i, (x, y) in enumerate(zip(a["l"], b["l"]))]
    for k, x, y in rows:
        print(f"{k}: rel {rel(x, y):.3e}")
    return [k for k, x, y in rows if not np.array_equal(x, y)]


@pytest.mark.parametrize("depth,width,kind", CASES)
def test_kept_planes_equal_recomputed(dev, depth, width, kind):
    for n, max_grid in _sizes(dev):
        a, b, _, _ = _pair(dev, depth, width, kind, n, max_grid)
        assert a["keep"] is True and b["keep"] is False
        assert a["spec"] is True and b["spec"] is True
        assert np.isfinite(a["p"]).all() and np.abs(a["g"][0]).max() > 0
        diff = _differing(a, b)
        assert diff == [], f"n={n}: {diff} differ between kept and recomputed planes"


@pytest.mark.parametrize("depth,width,kind", CASES)
def test_kept_planes_are_reproducible(dev, depth, width, kind):
    for n, max_grid in _sizes(dev):
        a, _, lay, flat = _pair(dev, depth, width, kind, n, max_grid)
        c = _run(device.get_device(), lay, kind, n, flat, 2, 1, max_grid)
        assert c["keep"] is True
        assert np.array_equal(a["p"], c["p"]) and all(np.array_equal(x, y) for x, y in zip(a["g"] + a["l"], c["g"] + c["l"]))


@pytest.mark.parametrize("depth,width,kind,outputs", INELIGIBLE)
def test_ineligible_plans_recompute(dev, depth, width, kind, outputs):
    for n, max_grid in _sizes(dev)[:2]:
        a, b, _, _ = _pair(dev, depth, width, kind, n, max_grid, outputs)
        assert a["keep"] is False and b["keep"] is False
        assert a["spec"] is (not outputs) and b["spec"] is (not outputs)
        assert np.abs(a["g"][0]).max() > 0
        diff = _differing(a, b)
        assert diff == [], f"n={n}: {diff} differ between the two settings of a switch that does not apply"


@pytest.mark.parametrize("depth,width,kind", CASES)
def test_kept_planes_agree_with_the_separate_launches(dev, depth, width, kind):
    d = device.get_device()
    n, max_grid = _sizes(dev)[-1]
    a, _, lay, flat = _pair(dev, depth, width, kind, n, max_grid)
    s = _run(d, lay, kind, n, flat, 1, 1, fused=False)
    e = rel(a["g"][0], s["g"][0])
    print(f"n={n}: gradient rel-L2 against the separate launches {e:.3e}")
    assert e < 3e-6
