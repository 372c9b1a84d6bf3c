"""Kernel level: ppsci_spinn_jet_fwd / ppsci_spinn_jet_bwd (csrc/spinn_jet.inc) against a float64 einsum of the same float32
operands, with worst-case rounding bounds (u = 2^-24, the unit roundoff of fp32):
  forward   |U - U64| <= (R + 2) u sum_r |F0 F1 F2|: a length-R dot product (R products, R - 1 sums) with one extra rounding in
            the operand F0*F1;
  reverse   |Fbar - Fbar64| <= (T + 2) u sum |Ubar F_b F_c| with T = (streams feeding the element) * n_b * n_c summed terms, each
            term carrying two products.
An indexing error is O(1) against either.  Shapes: the fixture's cases A, B, C and F (less than a tile on every axis; rank 3;
full plus ragged tiles on every axis with rank 32; a one-point axis), all 27 order triples split over two calls."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests.common import make_dev_fixture

dev = make_dev_fixture()
U32 = 2.0 ** -24
SHAPES = {"A": ((7, 5, 6), 4), "B": ((4, 9, 3), 3), "C": ((17, 33, 19), 32), "F": ((1, 9, 5), 4)}
TRIPLES = list(itertools.product(range(3), repeat=3))
CALLS = (TRIPLES[:14], TRIPLES[14:])


def _desc(shape, rank, orders):
    from paddlescience_amd import _lib as L

    d = L.SpinnJetDesc()
    d.n[0], d.n[1], d.n[2] = shape
    d.rank, d.nq = rank, len(orders)
    for q, t in enumerate(orders):
        for a in range(3):
            d.ord[q][a] = t[a]
    return d


def _factors(shape, rank, seed):
    """[3][n][R] per axis, asymmetric between the axes (own scale and offset each) and between the streams."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((3, n, rank)) * (0.5 + a) + 0.3 * a).astype(np.float32) for a, n in enumerate(shape)]


def _dev_tensor(a):
    from paddlescience_amd.device import get_device

    return torch.from_numpy(np.ascontiguousarray(a)).to(get_device())


def _fwd(shape, rank, orders, Ft):
    from paddlescience_amd import _lib as L
    from paddlescience_amd.hotpath import _p, _stream_ptr

    U = torch.full((len(orders), shape[0] * shape[1] * shape[2]), float("nan"), dtype=torch.float32, device=Ft[0].device)
    L.check(L.lib().ppsci_spinn_jet_fwd(C.byref(_desc(shape, rank, orders)), _p(Ft[0]), _p(Ft[1]), _p(Ft[2]), _p(U), _stream_ptr(U)))
    return U.cpu().numpy().reshape(len(orders), *shape)


def _bwd(shape, rank, orders, Ft, Ubar):
    from paddlescience_amd import _lib as L
    from paddlescience_amd.hotpath import _p, _stream_ptr

    d = _desc(shape, rank, orders)
    scratch = torch.zeros(max(4, int(L.lib().ppsci_spinn_jet_scratch_floats(C.byref(d)))), dtype=torch.float32, device=Ubar.device)
    Fbar = [torch.full((3, n, rank), float("nan"), dtype=torch.float32, device=Ubar.device) for n in shape]
    L.check(L.lib().ppsci_spinn_jet_bwd(C.byref(d), _p(Ft[0]), _p(Ft[1]), _p(Ft[2]), _p(Ubar), _p(scratch), _p(Fbar[0]), _p(Fbar[1]),
                                        _p(Fbar[2]), _stream_ptr(Ubar)))
    return [f.cpu().numpy() for f in Fbar]


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_forward_against_float64_einsum(case, dev):
    shape, rank = SHAPES[case]
    F = _factors(shape, rank, 7 + ord(case))
    Ft = [_dev_tensor(f) for f in F]
    F64 = [f.astype(np.float64) for f in F]
    worst = 0.0
    for orders in CALLS:
        U = _fwd(shape, rank, orders, Ft)
        for q, (a, b, c) in enumerate(orders):
            ref = np.einsum("ir,jr,kr->ijk", F64[0][a], F64[1][b], F64[2][c])
            mag = np.einsum("ir,jr,kr->ijk", np.abs(F64[0][a]), np.abs(F64[1][b]), np.abs(F64[2][c]))
            ratio = np.abs(U[q] - ref) / ((rank + 2) * U32 * mag)
            assert np.isfinite(U[q]).all()
            worst = max(worst, float(ratio.max()))
    print(f"[{dev}] forward {case}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_reverse_against_float64_einsum(case, dev):
    shape, rank = SHAPES[case]
    F = _factors(shape, rank, 11 + ord(case))
    Ft = [_dev_tensor(f) for f in F]
    F64 = [f.astype(np.float64) for f in F]
    rng = np.random.default_rng(3 + ord(case))
    subs = {0: "ijk,jr,kr->ir", 1: "ijk,ir,kr->jr", 2: "ijk,ir,jr->kr"}
    worst = 0.0
    for orders in CALLS:
        Ubar = rng.standard_normal((len(orders),) + shape).astype(np.float32)
        Ub = _dev_tensor(Ubar.reshape(len(orders), -1))
        got = _bwd(shape, rank, orders, Ft, Ub)
        again = _bwd(shape, rank, orders, Ft, Ub)
        for ax in range(3):
            assert np.array_equal(got[ax], again[ax]), "two calls must give the same bits"
            o1, o2 = [x for x in range(3) if x != ax]
            ref, mag, terms = np.zeros((3, shape[ax], rank)), np.zeros((3, shape[ax], rank)), np.zeros(3)
            for q, t in enumerate(orders):
                g = Ubar[q].astype(np.float64)
                ref[t[ax]] += np.einsum(subs[ax], g, F64[o1][t[o1]], F64[o2][t[o2]])
                mag[t[ax]] += np.einsum(subs[ax], np.abs(g), np.abs(F64[o1][t[o1]]), np.abs(F64[o2][t[o2]]))
                terms[t[ax]] += shape[o1] * shape[o2]
            assert np.isfinite(got[ax]).all()
            fed = terms > 0  # an order no stream of this call has along the axis receives exact zeros
            assert not got[ax][~fed].any()
            ratio = np.abs(got[ax][fed] - ref[fed]) / ((terms[fed, None, None] + 2) * U32 * mag[fed])
            worst = max(worst, float(ratio.max()))
    print(f"[{dev}] reverse {case}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_bad_descriptors_are_refused_with_a_message(dev):
    from paddlescience_amd import _lib as L
    from paddlescience_amd.hotpath import _p

    shape, rank = (4, 3, 5), 4
    Ft = [_dev_tensor(f) for f in _factors(shape, rank, 1)]
    U = torch.zeros((1, 60), dtype=torch.float32, device=Ft[0].device)
    scratch = torch.zeros(4096, dtype=torch.float32, device=U.device)
    Fb = [torch.zeros((3, n, rank), dtype=torch.float32, device=U.device) for n in shape]
    lib = L.lib()

    def both(d, f0=Ft[0], u=U):
        rcs = [lib.ppsci_spinn_jet_fwd(C.byref(d), _p(f0), _p(Ft[1]), _p(Ft[2]), _p(u), None)]
        msgs = [lib.ppsci_last_error().decode()]
        rcs.append(lib.ppsci_spinn_jet_bwd(C.byref(d), _p(f0), _p(Ft[1]), _p(Ft[2]), _p(u), _p(scratch), _p(Fb[0]), _p(Fb[1]), _p(Fb[2]),
                                           None))
        msgs.append(lib.ppsci_last_error().decode())
        return rcs, msgs

    for what, d, kw in (("streams", _desc(shape, rank, []), {}), ("order 3", _desc(shape, rank, [(0, 3, 0)]), {}),
                        ("rank 0", _desc(shape, 0, [(0, 0, 0)]), {}), ("rank 65", _desc(shape, 65, [(0, 0, 0)]), {}),
                        ("null pointer", _desc(shape, rank, [(0, 0, 0)]), {"f0": None}),
                        ("null pointer", _desc(shape, rank, [(0, 0, 0)]), {"u": None})):
        rcs, msgs = both(d, **kw)
        assert all(rc != 0 for rc in rcs), what
        assert all(what.split()[0] in m for m in msgs), (what, msgs)
    assert lib.ppsci_spinn_jet_scratch_floats(C.byref(_desc(shape, rank, []))) == 0
    assert lib.ppsci_spinn_jet_scratch_floats(C.byref(_desc(shape, rank, [(1, 1, 1)]))) > 0
