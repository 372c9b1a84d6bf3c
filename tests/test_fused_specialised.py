"""Shape-specialised instantiations of the fused tile kernel (csrc/taylor_fused.inc, template parameters D_RAW / M).

A plan whose residual program is a compile-time table, whose net has two raw inputs and one output and which requests none of
the optional outputs (U, dL/dU, residual values) runs an instantiation with that shape as compile-time constants: the same
arithmetic in the same order behind the same barriers, with an LDS carve-up of immediates and without the optional-output
code.  `ppsci_set_fused_specialised(0)` keeps every plan on the generic kernel.  Checked here:
  * switch on against switch off: parameters, the gradients of both steps and the loss terms are EQUAL (np.array_equal), on the
    emulator and on the device; the plan reports which kernel it runs;
  * two runs with the switch on are bit-identical (run-to-run reproducibility, as tests/test_determinism.py);
  * what must stay on the generic kernel does: a plan with optional outputs, a three-input net, the switch at 0;
  * the specialised kernel agrees with the separate launches within the bound of tests/test_static_programs.py.
Cases: even and odd depth (the even-depth WAR barrier is a code path of its own), H < padded width, S = 4 / 5 / 1.
Sizes: one ragged tile; several tiles with unequal counts per workgroup and a ragged last one.
Reference: /root/reference/ppsci/solver/train.py:82-184 (one training step), equation/pde/allen_cahn.py:56-64, laplace.py:40-55."""
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
    (4, 64, "allen_cahn"),  # the primary benchmark's net: S = 4, even depth
    (3, 50, "laplace"),     # S = 5 (N1 = 2, N2 = 2), odd depth, H < 64, two terms, aux arrays, an input operand
    (2, 40, "value"),       # S = 1
    (5, 64, "allen_cahn"),  # L = 5
]


def _sizes(dev):
    # emulator (4 "CUs"): 6 tiles on 4 workgroups (max_grid) -- two workgroups run two tiles, the last tile holds 10 points;
    # device: 514 tiles on 512 workgroups -- two run two tiles, the last tile holds 5 points; and one ragged tile
    return [(90, 4), (5, 0)] if dev != "gpu" else [(8213, 0), (5, 0)]


def _constraint(d, kind, lay, n, seed, n_in=2):
    rng = np.random.default_rng(seed)
    ed, streams, n_aux = _program(kind, n)
    xs = [torch.tensor(rng.random(n, dtype=np.float32) * 2 - 1, device=d) for _ in range(n_in)]
    aux = [torch.tensor(rng.random(n, dtype=np.float32) + 0.5, device=d) for _ in range(n_aux)]
    return FusedConstraint(kind, lay, streams, ed, xs, aux, [f"k{i}" for i in range(ed.n_res)])


def _run(d, lay, kind, n, flat, steps, spec, max_grid=0, fused=True, step_outputs=False, n_in=2):
    lib = L.lib()
    lib.ppsci_set_fused_specialised(spec)
    lib.ppsci_set_max_grid(max_grid)
    try:
        params = torch.tensor(flat, device=d)
        eng = Engine(lay, params)
        eng.one_launch = fused
        c = _constraint(d, kind, lay, n, 101, n_in)
        c.step_outputs = step_outputs
        grads, losses = [], []
        for _ in range(steps):
            eng.train_step([c], 1e-2)
            grads.append(eng.grad.detach().cpu().numpy().copy())
            losses.append(c.loss_terms.detach().cpu().numpy().copy())
        plan = c._step_plan if fused else None
        return dict(p=params.detach().cpu().numpy(), g=grads, l=losses, spec=plan.specialised if plan else None,
                    name=plan.static_program if plan else None)
    finally:
        lib.ppsci_set_fused_specialised(1)
        lib.ppsci_set_max_grid(0)


_REF = {}


def _pair(dev, depth, width, kind, n, max_grid):
    """(switch on, switch off), two steps each; computed once per case and size."""
    key = (dev, depth, width, kind, n)
    if key not in _REF:
        d = device.get_device()
        lay = hp.NetLayout(2, depth, width, 1, "tanh")
        flat = _weights(lay, 13)
        _REF[key] = (_run(d, lay, kind, n, flat, 2, 1, max_grid), _run(d, lay, kind, n, flat, 2, 0, max_grid), lay, flat)
    return _REF[key]


@pytest.mark.parametrize("depth,width,kind", CASES)
def test_specialised_equals_generic(dev, depth, width, kind):
    for n, max_grid in _sizes(dev):
        a, b, _, _ = _pair(dev, depth, width, kind, n, max_grid)
        assert a["name"] != "" and a["name"] == b["name"]
        assert a["spec"] is True and b["spec"] is False
        assert np.isfinite(a["p"]).all() and np.abs(a["g"][0]).max() > 0
        diff = [k for k, x, y in [("p", a["p"], b["p"])] + [(f"g{i}", x, y) for i, (x, y) in enumerate(zip(a["g"], b["g"]))] +
                [(f"l{i}", x, y) for i, (x, y) in enumerate(zip(a["l"], b["l"]))] if not np.array_equal(x, y)]
        for k, x, y in [("p", a["p"], b["p"]), ("g0", a["g"][0], b["g"][0]), ("g1", a["g"][1], b["g"][1])]:
            print(f"n={n} {k}: rel {rel(x, y):.3e}")
        assert diff == [], f"n={n}: {diff} differ between the specialised and the generic kernel"


@pytest.mark.parametrize("depth,width,kind", CASES)
def test_specialised_is_reproducible(dev, depth, width, kind):
    for n, max_grid in _sizes(dev):
        a, _, lay, flat = _pair(dev, depth, width, kind, n, max_grid)
        c = _run(device.get_device(), lay, kind, n, flat, 2, 1, max_grid)
        assert c["spec"] is True
        assert np.array_equal(a["p"], c["p"]) and all(np.array_equal(x, y) for x, y in zip(a["g"] + a["l"], c["g"] + c["l"]))


@pytest.mark.parametrize("depth,width,kind", CASES)
def test_specialised_agrees_with_the_separate_launches(dev, depth, width, kind):
    d = device.get_device()
    n, max_grid = _sizes(dev)[0]
    a, _, lay, flat = _pair(dev, depth, width, kind, n, max_grid)
    s = _run(d, lay, kind, n, flat, 1, 1, fused=False)
    assert rel(a["g"][0], s["g"][0]) < 3e-6


def test_fallbacks_to_the_generic_kernel(dev):
    d = device.get_device()
    n = 90 if dev != "gpu" else 8213
    lay = hp.NetLayout(2, 4, 64, 1, "tanh")
    flat = _weights(lay, 13)
    a, b, _, _ = _pair(dev, 4, 64, "allen_cahn", *_sizes(dev)[0])
    # optional outputs requested: the generic kernel writes them
    o = _run(d, lay, "allen_cahn", n, flat, 1, 1, _sizes(dev)[0][1], step_outputs=True)
    assert o["spec"] is False and o["name"] == a["name"] and np.array_equal(o["g"][0], b["g"][0])
    # the switch at 0
    assert b["spec"] is False
    # three raw inputs: no (3, .) instantiation
    lay3 = hp.NetLayout(3, 2, 40, 1, "tanh")
    flat3 = _weights(lay3, 7)
    t = _run(d, lay3, "value", n, flat3, 1, 1, n_in=3)
    s = _run(d, lay3, "value", n, flat3, 1, 1, fused=False, n_in=3)
    assert t["spec"] is False and rel(t["g"][0], s["g"][0]) < 3e-6
