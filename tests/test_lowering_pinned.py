"""What the lowering front end emits (compile.lower_constraint -> graph.lower), pinned case by case against
tests/golden/lowering_pins.json: the crc32 of every epilogue program (residual program, reduction / coupling passes, the stream
programs of an input transform), the stream set, the column tables and the typed rows the engine is fed.  tools/
gen_static_programs.py matches programs word for word, so the instruction ORDER is part of the contract; the file was
written by the lowering as it stood before it was split into stages and is not regenerated from later code.

Host code only: nothing here builds a library, runs a kernel or starts a process.

    python tests/test_lowering_pinned.py --write     # rewrite the file (only to add a case)
"""
import json
import os
import re
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import ppsci  # noqa: E402
from paddlescience_amd import compile as cp  # noqa: E402
from paddlescience_amd import device, graph  # noqa: E402
from ppsci.autodiff import hessian, jacobian  # noqa: E402
from tests import spinn_jet_cases as T_JET  # noqa: E402
from tests import test_equations as T_EQ  # noqa: E402
from tests import test_reference_expressions as T_REF  # noqa: E402
from tests import test_spinn_jet_frontend as T_JET_FRONT  # noqa: E402

PINS = os.path.join(ROOT, "tests", "golden", "lowering_pins.json")


# ---- one record per lowering --------------------------------------------------------------------------------------------------
def _crc(prog) -> int:
    return zlib.crc32(bytes(prog.build()))


def _matrix_crc(M) -> int:
    return M.crc() if isinstance(M, graph.CsrMatrix) else zlib.crc32(np.ascontiguousarray(M, dtype=np.float32).tobytes())


def _aux_names(names):
    """Coupling columns carry the coupling's name: numbered by order of appearance within the case, whatever was traced
    before it in the process."""
    seen = []

    def sub(m):
        if m.group(0) not in seen:
            seen.append(m.group(0))
        return f"couple{seen.index(m.group(0))}"

    return [re.sub(r"couple\d+(_[0-9a-f]{8})?$", sub, n) for n in names]


def record(low, jet=None) -> dict:
    rec = {"program": _crc(low.program), "streams": repr(low.streams) if jet is None else [list(t) for t in jet.orders],
           "input_names": list(low.input_names), "aux_names": _aux_names(low.aux_names), "loss_keys": list(low.loss_keys),
           "value_index": dict(low.value_index), "param_slots": list(low.param_slots),
           "causal": [[c.row, c.label_aux, c.weight_aux, c.area_aux, c.factor_aux] for c in low.causal],
           "periodic": [[p.row, p.label_aux] for p in low.periodic], "reductions": None, "couplings": None}
    if low.reductions:
        rec["reductions"] = {"k": low.reductions.k, "p1": _crc(low.reductions.p1), "p3": _crc(low.reductions.p3)}
    if low.couplings:
        rec["couplings"] = {"pv": _crc(low.couplings.pv), "p3": _crc(low.couplings.p3), "items": [
            {"rows": c.rows, "cols": c.cols, "res_row": c.res_row, "weight_aux": c.weight_aux, "rhs_aux": c.rhs_aux,
             "vbar_aux": c.vbar_aux, "factor": c.factor, "matrix": _matrix_crc(c.matrix)} for c in low.couplings.items]}
    rec["nets"] = [{"row0": s.row0, "inputs": s.inputs, "spec": repr(s.spec),
                    "pre": None if s.pre is None else [[_crc(pg), r0, rows] for pg, r0, rows in s.pre]} for s in low.nets]
    return rec


def _term(**kw):
    return graph.LossTerm(**kw)


def _constraint(model, exprs, input_keys, label_keys=None, weight_keys=(), loss=None, n=16, **kw):
    """The device-free half of a CompiledConstraint of batch size n."""
    label_keys = list(exprs) if label_keys is None else list(label_keys)
    loss = loss or ppsci.loss.MSELoss("mean")
    return cp.lower_constraint(model, exprs, tuple(input_keys), label_keys, list(weight_keys), loss, n, kw.pop("n_global", n), **kw).low


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _mlp(inputs, outputs=("u",)):
    return ppsci.arch.MLP(tuple(inputs), tuple(outputs), 2, 16, "tanh")


def _dn(d, var, k):
    e = d["u"]
    for _ in range(k):
        e = jacobian(e, d[var])
    return e


def _static_programs():
    """Every API entry of tools/gen_static_programs.cases(), as the generator itself lowers it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_static_programs as G

    lows, real = [], graph.lower

    def spy(*a, **k):
        lows.append(real(*a, **k))
        return lows[-1]

    graph.lower = spy
    try:
        names = [c[0] for c in G.cases()]
    finally:
        graph.lower = real
    api = names[len(names) - len(lows):]  # (the hand-built programs come first and are not lowered)
    assert len(api) == 12 and api[0] == "allen_cahn"
    return {f"static:{n}": record(low) for n, low in zip(api, lows)}


def _derivative_sets():
    out = {}
    for k in (1, 2, 3, 4):
        out[f"pure:{k}"] = _constraint(_mlp("xy"), {"r": lambda d, k=k: _dn(d, "x", k)}, "xy")
    out["mixed:u_xy"] = _constraint(_mlp("xy"), {"r": lambda d: jacobian(jacobian(d["u"], d["x"]), d["y"])}, "xy")
    # (a == lo for u_xxy, a != lo for u_xyy: one stream along x - y serves both, with opposite signs)
    out["mixed:u_xxy+u_xyy"] = _constraint(_mlp("xy"), {"xxy": lambda d: jacobian(hessian(d["u"], d["x"]), d["y"]),
                                                       "xyy": lambda d: jacobian(hessian(d["u"], d["y"]), d["x"])}, "xy")
    bi = ppsci.equation.Biharmonic(2, 1.0, 1.0)
    m = _mlp("xy")
    out["mixed:biharmonic2d"] = _constraint(m, T_EQ.equation_exprs(m, bi), "xy")
    ns = ppsci.equation.NavierStokes(0.01, 1.0, 3, True)
    m = _mlp("txyz", "uvwp")
    out["streams:navier_stokes3d_t"] = _constraint(m, T_EQ.equation_exprs(m, ns), "txyz")
    # three directions, one of them to third order: the (4, 4, 4, 4) kernels with one zero padding direction
    out["streams:padded"] = _constraint(_mlp("xyz"), {"r": lambda d: _dn(d, "x", 3) + _dn(d, "y", 2) + _dn(d, "z", 1)}, "xyz")
    model, exprs, keys = T_REF.case_biharmonic_moments()
    out["mixed:shear_forces"] = _constraint(model, exprs, keys)
    return out


def _several_nets():
    out = {}
    for name, case in (("elasticity", T_EQ.case_elasticity), ("heat_exchanger", T_EQ.case_heat_exchanger)):
        model, eq, keys = case()
        out[f"nets:{name}"] = _constraint(model, T_EQ.equation_exprs(model, eq), keys, n=64)
    model, exprs, keys = T_REF.case_hpinns()
    out["nets:hpinns"] = _constraint(model, exprs, keys)
    import ppsci.functional as F

    m = _mlp(("sx", "y"))  # 2 inputs x 5 streams = 10 rows: two stream programs
    m.register_input_transform(lambda d: {"sx": F.sin(1.7 * d["x"] + 0.3), "y": d["y"]})
    out["nets:input_transform"] = _constraint(m, {"r": lambda d: hessian(d["u"], d["x"]) + hessian(d["u"], d["y"]) * d["x"]}, "xy", n=8)
    return out


def _slots_and_batch_terms():
    out = {}
    out["param"] = _constraint(_mlp("tx"), {"r": lambda d: jacobian(d["u"], d["t"]) - graph.Sym.param("nu", 0) * hessian(d["u"], d["x"])
                                            + graph.Sym.param("k", 2) * d["u"]}, "tx")
    out["reductions"] = _constraint(_mlp("xy"), {"centred": lambda d: d["u"] - d["u"].mean(),
                                                 "scaled": lambda d: jacobian(d["u"], d["x"]) * (d["u"] * d["y"]).sum()}, "xy", n=10)
    rng = np.random.default_rng(0)
    dense = rng.standard_normal((4, 12)).astype(np.float32)
    out["coupling:dense"] = _constraint(_mlp("x"), {"v": lambda d: graph.couple(jacobian(d["u"], d["x"]) + d["u"], dense, d["u"])},
                                        "x", n=12)
    csr = graph.CsrMatrix.from_coo([0, 0, 1, 2, 2, 2], [1, 7, 3, 0, 4, 5], rng.standard_normal(6).astype(np.float32), (3, 8))

    def frac(d):
        return graph.couple(-d["x"], csr, d["u"], factor=-0.25)

    out["coupling:csr"] = _constraint(_mlp("x"), {"f": frac}, "x", n=8)
    outs = cp.trace_exprs(_mlp("x"), ("x",), {"f": frac}, (), None, [])
    out["coupling:csr_no_label"] = graph.lower(outs, [_term(key="f", weight="weight:f", scale=0.125)])
    # both couplings in one constraint: two names, two columns each
    m = _mlp("x", "uv")
    out["coupling:two"] = _constraint(m, {"f": lambda d: graph.couple(-d["x"], csr, d["u"], factor=-0.25),
                                          "g": lambda d: graph.couple(d["v"], dense[:3, :8], d["v"])}, "x", n=8)
    return out


def _loss_rows():
    lap = {"r": lambda d: hessian(d["u"], d["x"]) + hessian(d["u"], d["y"])}
    both = dict(lap, u=lambda d: d["u"])
    return {
        "loss:weight": _constraint(_mlp("xy"), both, "xy", weight_keys=["u"]),
        "loss:sum": _constraint(_mlp("xy"), lap, "xy", loss=ppsci.loss.MSELoss("sum")),
        "loss:area": _constraint(_mlp("xy"), both, ("x", "y", "area"), weight_keys=["r"]),
        "loss:causal": _constraint(_mlp("tx"), {"r": lambda d: jacobian(d["u"], d["t"]) - hessian(d["u"], d["x"])}, ("t", "x", "area"),
                                   weight_keys=["r"], loss=ppsci.loss.CausalMSELoss(4, tol=0.5)),
        "loss:periodic": _constraint(_mlp("xy"), both, "xy", loss=ppsci.loss.PeriodicMSELoss("mean")),
        "loss:l1": _constraint(_mlp("xy"), both, "xy", loss=ppsci.loss.L1Loss("mean")),
        "loss:l2rel": _constraint(_mlp("xy"), lap, "xy", loss=ppsci.loss.L2RelLoss("mean")),
        "loss:extra_outputs": _constraint(_mlp("xy"), dict(both, ux=lambda d: jacobian(d["u"], d["x"])), "xy", label_keys=["r"],
                                          extra_outputs=("ux", "u")),
        "loss:raw_output_label": _constraint(_mlp("xy", "uv"), lap, "xy", label_keys=["r", "v"]),
        "loss:row_slice": _constraint(_mlp("x"), {"u0": lambda d: d["u"][0:1], "ux_end": lambda d: jacobian(d["u"], d["x"])[15:16]}, "x"),
    }


def _spinn_jet():
    model = T_JET.make_model("A")
    low, jet = T_JET_FRONT.lowered(model, T_JET.closures(model)["sg"])
    return {"spinn_jet:sg": record(low, jet)}


def all_records() -> dict:
    device.set_device("cpu")  # (the parameters of the throw-away models live on the host)
    try:
        out = _static_programs()
        for group in (_derivative_sets, _several_nets, _slots_and_batch_terms, _loss_rows):
            out.update({k: record(low) for k, low in group().items()})
        out.update(_spinn_jet())
    finally:
        device.set_device(None)
    return json.loads(json.dumps(out))  # (tuples as lists, as the file has them)


CASES = ([f"static:{n}" for n in ("allen_cahn", "allen_cahn_w", "laplace2d", "laplace2d_w", "laplace3d", "poisson2d", "value_u",
                                   "value_u_w", "value_u_tx", "navier_stokes2d", "value_uv", "navier_stokes2d_t")]
         + ["pure:1", "pure:2", "pure:3", "pure:4", "mixed:u_xy", "mixed:u_xxy+u_xyy", "mixed:biharmonic2d",
            "streams:navier_stokes3d_t", "streams:padded", "mixed:shear_forces", "nets:elasticity", "nets:heat_exchanger",
            "nets:hpinns", "nets:input_transform", "param", "reductions", "coupling:dense", "coupling:csr", "coupling:csr_no_label",
            "coupling:two", "loss:weight", "loss:sum", "loss:area", "loss:causal", "loss:periodic", "loss:l1", "loss:l2rel",
            "loss:extra_outputs", "loss:raw_output_label", "loss:row_slice", "spinn_jet:sg"])


@pytest.fixture(scope="module")
def records():
    return all_records()


def test_every_case_is_pinned(records):
    assert sorted(records) == sorted(CASES) == sorted(json.load(open(PINS)))


@pytest.mark.parametrize("case", CASES)
def test_lowering_is_what_was_pinned(records, case):
    want = json.load(open(PINS))[case]
    got = records[case]
    for field in want:
        assert got[field] == want[field], (case, field)
    assert got == want


def test_the_cases_reach_the_branches_they_are_there_for(records):
    r = records
    assert "n2=3, n3=0, n4=0" in r["streams:navier_stokes3d_t"]["streams"] and r["streams:navier_stokes3d_t"]["streams"].count("[") == 5
    assert "[0.0, 0.0, 0.0]]" in r["streams:padded"]["streams"] and "n4=4" in r["streams:padded"]["streams"]  # a zero direction
    assert "n4=" in r["mixed:biharmonic2d"]["streams"] and "-1.0" in r["mixed:biharmonic2d"]["streams"]  # u_xxyy: x - y
    assert len(r["nets:elasticity"]["nets"]) == 2 and len(r["nets:heat_exchanger"]["nets"]) == 3
    assert sorted(len(n["inputs"]) for n in r["nets:heat_exchanger"]["nets"]) == [2, 3, 3]
    pre = r["nets:input_transform"]["nets"][0]["pre"]
    assert [p[1:] for p in pre] == [[0, 8], [8, 2]]
    assert r["param"]["param_slots"] == [0, 2]
    assert r["reductions"]["reductions"]["k"] == 2
    assert [(c["rows"], c["cols"]) for c in r["coupling:two"]["couplings"]["items"]] == [(3, 8), (3, 8)]
    assert r["coupling:two"]["aux_names"].count("__couple_rhs__couple1") == 1
    assert r["coupling:csr"]["program"] != r["coupling:csr_no_label"]["program"]
    assert r["loss:causal"]["causal"] and r["loss:periodic"]["periodic"]
    assert r["loss:extra_outputs"]["loss_keys"] == ["r", "ux", "u"]


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: python tests/test_lowering_pinned.py --write")
    with open(PINS, "w") as f:
        json.dump(all_records(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {PINS}")
