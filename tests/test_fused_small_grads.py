"""The small gradients of the fused tile kernel (csrc/taylor_fused.inc: W0, the biases, W_last, b_last) against the separate
launches, PER PARAMETER TENSOR: the whole-vector rel-L2 of tests/test_fused_step.py is dominated by the hidden matrices and
would not see a wrong bias sum.  The bias gradients are per-lane sums over all tiles of a workgroup, reduced over the 16
points of a tile once behind the tile loop; ppsci_set_max_grid(2) makes a workgroup carry them over several tiles and gives
the two workgroups unequal numbers of tiles.

Both sides are fp32 sums in different orders.  Bound per tensor: the larger of 3e-6 (the first-step bound of
test_fused_step_matches_separate_launches) and 4x the worst per-tensor figure of the build WITHOUT the per-lane sums at these
shapes.  That build, on the emulator, worst tensor of each case (tail 0 and tail 3 give the same figures):
    tanh 4x64 allen_cahn 67: 2.19e-07 (linears.1.weight; biases <= 7.5e-08)    tanh 3x50 laplace 83: 2.18e-07 (last_fc.bias)
    sin 5x33 streams:1,1 70: 8.78e-08 (linears.0.bias)                          silu 2x40 allen_cahn 67: 1.07e-07 (linears.1.weight)
On the MI355X the same build's worst tensor over all cases is 1.05e-07.  4 x 2.19e-07 = 8.8e-07 < 3e-6, so the bound is 3e-6.
(With the per-lane sums the worst figures are the same; the bias tensors of the first case go from 6.6 / 7.5 / 6.9 / 6.7e-08
to 5.8 / 6.7 / 7.5 / 6.5e-08.)"""
import numpy as np
import pytest
import torch

from paddlescience_amd import _lib as L
from paddlescience_amd import device
from paddlescience_amd import hotpath as hp
from paddlescience_amd.engine import Engine
from tests.common import make_dev_fixture, rel
from tests.test_one_launch import _constraint, _weights

dev = make_dev_fixture()

BOUND = 3e-6


def _run(d, lay, kind, n, flat, fused, steps, tail=-1):
    lib = L.lib()
    lib.ppsci_set_max_grid(2)
    lib.ppsci_set_step_tail(tail)
    try:
        params = torch.tensor(flat, device=d)
        eng = Engine(lay, params)
        eng.one_launch = fused
        c = _constraint(d, kind, lay, n, 100)
        if fused:
            assert c.one_launch_ready() and c._step_kind == hp.STEP_FUSED_TILE
        grads = []
        for _ in range(steps):
            eng.train_step([c], 1e-2)
            grads.append(eng.grad.detach().cpu().numpy().copy())
        return params.detach().cpu().numpy(), grads
    finally:
        lib.ppsci_set_max_grid(0)
        lib.ppsci_set_step_tail(-1)


def _tensors(lay, flat):
    out, off = [], 0
    for name, shp in lay.param_shapes():
        k = int(np.prod(shp))
        out.append((name, flat[off:off + k]))
        off += k
    assert off == flat.size
    return out


CASES = [
    # (activation, hidden layers, width, program, points)
    ("tanh", 4, 64, "allen_cahn", 67),   # 5 tiles on 2 workgroups (3 + 2), the last tile with 3 valid points
    ("tanh", 3, 50, "laplace", 83),      # odd L, width < padded width
    ("sin", 5, 33, "streams:1,1", 70),   # S = 3: the kernel with the program on the VM
    ("silu", 2, 40, "allen_cahn", 67),
]

_SEPARATE = {}  # the separate launches' first-step gradient of a case: computed once, shared by both tail modes


@pytest.mark.parametrize("tail", [0, 3])
@pytest.mark.parametrize("act,depth,width,kind,n", CASES)
def test_small_gradients_match_separate_launches_per_tensor(dev, act, depth, width, kind, n, tail):
    d = device.get_device()
    lay = hp.NetLayout(2, depth, width, 1, act)
    flat = _weights(lay, 7)
    key = (dev, act, depth, width, kind, n)
    if key not in _SEPARATE:
        _SEPARATE[key] = _run(d, lay, kind, n, flat, False, 1)[1][0]
    g_sep = _SEPARATE[key]
    g_one = _run(d, lay, kind, n, flat, True, 1, tail)[1][0]
    figures = [(name, rel(a, b)) for (name, a), (_, b) in zip(_tensors(lay, g_one), _tensors(lay, g_sep))]
    print(f"per-tensor rel-L2 {act} {depth}x{width} {kind} n={n} tail={tail}: " + ", ".join(f"{k}={v:.2e}" for k, v in figures))
    assert all(np.abs(b).max() > 0 for _, b in _tensors(lay, g_sep))  # every tensor has a gradient to compare
    for name, v in figures:
        assert v < BOUND, (name, v)


def test_small_gradients_are_deterministic(dev):
    """The per-lane sums change the summation order (tiles per lane first, then the 16 lanes) but keep it fixed: two runs of
    the 67-point case give the same bits after 3 steps."""
    d = device.get_device()
    lay = hp.NetLayout(2, 4, 64, 1, "tanh")
    flat = _weights(lay, 7)
    for tail in (0, 3):
        p_a, g_a = _run(d, lay, "allen_cahn", 67, flat, True, 3, tail)
        p_b, g_b = _run(d, lay, "allen_cahn", 67, flat, True, 3, tail)
        assert np.array_equal(p_a, p_b) and all(np.array_equal(x, y) for x, y in zip(g_a, g_b))
        assert np.isfinite(p_a).all() and rel(p_a, flat) > 1e-4
