"""The kernel behind the fused tile kernel (step tail 3, csrc/wgrad_reduce.hip) in its two mappings: one 1 024-thread
workgroup per 16 x 16 block of a hidden matrix (ppsci_set_tail_split(1)) and, the default, four 256-thread workgroups per
block.  The split keeps every column's summation order -- row groups, the four chains, the order of the 16 row groups --
so parameters, gradient, Adam moments and loss terms are equal to the last bit, not to a tolerance."""
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


def _run(d, lay, kind, n, flat, split, steps):
    lib = L.lib()
    lib.ppsci_set_step_tail(3)
    lib.ppsci_set_tail_split(split)
    try:
        params = torch.tensor(flat, device=d)
        eng = Engine(lay, params)
        c = _constraint(d, kind, lay, n, 100)
        assert c.one_launch_ready() and c._step_kind == hp.STEP_FUSED_TILE
        grads, losses = [], []
        for _ in range(steps):
            eng.train_step([c], 1e-2)
            grads.append(eng.grad.detach().cpu().numpy().copy())
            losses.append(c.loss_terms.detach().cpu().numpy().copy())
        return (params.detach().cpu().numpy(), eng.m.detach().cpu().numpy(), eng.v.detach().cpu().numpy(), grads, losses)
    finally:
        lib.ppsci_set_step_tail(-1)
        lib.ppsci_set_tail_split(0)


CASES = [
    # (activation, hidden layers, width, program, points) -- rows of the tail kernel = workgroups of the tile kernel = tiles here
    ("tanh", 4, 64, "allen_cahn", 1000),  # 63 rows: fewer than one 64-row stride
    ("tanh", 4, 64, "allen_cahn", 2080),  # 130 rows = 2 x 64 + 2: a ragged stride
    ("tanh", 3, 50, "laplace", 900),      # width < padded width: masked lanes
    ("tanh", 2, 64, "streams:0,0", 300),  # a single hidden matrix
]


@pytest.mark.parametrize("act,depth,width,kind,n", CASES)
def test_split_tail_equals_one_workgroup_per_block(dev, act, depth, width, kind, n):
    d = device.get_device()
    lay = hp.NetLayout(2, depth, width, 1, act)
    flat = _weights(lay, 7)
    steps = 3
    if dev != "gpu":  # the emulator runs a few hundred points per second
        n, steps = n // 6 + 3, 2
    p1, m1, v1, g1, l1 = _run(d, lay, kind, n, flat, 1, steps)
    p0, m0, v0, g0, l0 = _run(d, lay, kind, n, flat, 0, steps)
    for s in range(steps):
        assert np.array_equal(g0[s], g1[s]), (s, rel(g0[s], g1[s]))
        assert np.array_equal(l0[s], l1[s]), (s, l0[s], l1[s])
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert np.array_equal(p0, p1), rel(p0, p1)
    assert np.isfinite(p0).all() and rel(p0, flat) > 1e-4 and np.abs(g0[0]).max() > 0  # the update is not a no-op


def test_split_tail_fragments_follow_every_parameter_write(dev):
    """tests/test_fused_step.py test_tail_kernel_fragments_follow_every_parameter_write with the split mapping named: the
    fragments the four workgroups of a block leave behind are those of a weight split in front of every step."""
    d = device.get_device()
    lay = hp.NetLayout(2, 4, 64, 1, "tanh")
    flat = _weights(lay, 11)
    n = 150 if dev != "gpu" else 20_000

    def run(force_split):
        L.lib().ppsci_set_step_tail(3)
        L.lib().ppsci_set_tail_split(0)
        try:
            params = torch.tensor(flat, device=d)
            eng = Engine(lay, params)
            c = _constraint(d, "allen_cahn", lay, n, 100)
            kept = []
            for step in range(5):
                if force_split:
                    hp.note_param_write()
                plan = getattr(c, "_step_plan", None)
                kept.append(plan is not None and plan._frag_token == (hp._PARAM_WRITES[0], params._version))
                eng.train_step([c], 1e-2)
            return params.detach().cpu().numpy(), kept
        finally:
            L.lib().ppsci_set_step_tail(-1)

    p_keep, kept = run(False)
    p_split, never = run(True)
    assert kept == [False, True, True, True, True] and not any(never)
    assert np.array_equal(p_keep, p_split) and rel(p_keep, flat) > 1e-4
