"""Symbolic per-point expression graph: the front-end that lowers a constraint's expressions to
(derivative stream set, epilogue program) for the fused HIP kernels.

Why it exists: the reference evaluates `model(x)`, `jacobian(u, x)`, `hessian(u, x)` and the
operator tree eagerly on paddle tensors with a dynamic autograd graph
(/root/reference/ppsci/autodiff/ad.py, ppsci/utils/symbolic.py:184-504, expression.py:96-102).
Here the same Python calls are made ONCE on proxy tensors (`Sym`); the recorded graph is then
compiled into
  * the set of network derivatives the Taylor-mode kernel must carry (hotpath.StreamSpec), and
  * a postfix program for the epilogue VM (hotpath.Program), incl. the MSE terms of
    ppsci/loss/mse.py:82-105.
Derivatives of arbitrary recorded expressions are obtained by symbolic differentiation down to the
network-output leaves (`net` -> `der`), which is what repeated `paddle.grad(..., create_graph=True)`
computes numerically (ad.py:73-75).
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import weakref
import zlib
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L
from . import hotpath as hp

Number = Union[int, float]

_UNARY_OPS = {
    "sin": L.OP_SIN, "cos": L.OP_COS, "tanh": L.OP_TANH, "exp": L.OP_EXP, "log": L.OP_LOG, "sqrt": L.OP_SQRT,
    "abs": L.OP_ABS, "sinh": L.OP_SINH, "cosh": L.OP_COSH, "tan": L.OP_TAN, "neg": L.OP_NEG, "sign": L.OP_SIGN,
    "heaviside": L.OP_HEAVISIDE, "detach": L.OP_DETACH,
    "asin": L.OP_ASIN, "acos": L.OP_ACOS, "atan": L.OP_ATAN, "asinh": L.OP_ASINH, "acosh": L.OP_ACOSH,
    "atanh": L.OP_ATANH, "erf": L.OP_ERF, "lgamma": L.OP_LGAMMA, "ceil": L.OP_CEIL, "floor": L.OP_FLOOR,
}
_BINARY_OPS = {"add": L.OP_ADD, "sub": L.OP_SUB, "mul": L.OP_MUL, "div": L.OP_DIV, "pow": L.OP_POW,
               "max": L.OP_MAX, "min": L.OP_MIN, "atan2": L.OP_ATAN2}


class Sym:
    """A per-point scalar field ([N, 1] in the reference).  Immutable; hash-consed by structure: the table holds its nodes
    weakly (a node keeps its arguments and its model alive, so the ids in a key cannot be recycled while its entry exists),
    and a trace that is dropped takes its nodes -- and the models they hold -- with it."""

    __slots__ = ("kind", "name", "value", "model", "comp", "dirs", "op", "args", "matrix", "_key", "__weakref__")
    _cache: "weakref.WeakValueDictionary[tuple, Sym]" = weakref.WeakValueDictionary()

    def __new__(cls, kind, name=None, value=None, model=None, comp=None, dirs=(), op=None, args=(), matrix=None):
        key = (kind, name, None if value is None else float(np.float32(value)), id(model) if model is not None else None,
               comp, tuple(dirs), op, tuple(id(a) for a in args))
        hit = cls._cache.get(key)
        if hit is not None:
            return hit
        self = object.__new__(cls)
        self.kind, self.name, self.model, self.comp = kind, name, model, comp
        self.value = None if value is None else float(np.float32(value))  # ConstantNode: fp32 (symbolic.py:448-454)
        self.dirs, self.op, self.args = tuple(dirs), op, tuple(args)
        self.matrix = matrix  # `couple` nodes: the constant matrix (in the key by its crc -- the name -- and its shape)
        self._key = key
        cls._cache[key] = self
        return self

    # ---- constructors
    @staticmethod
    def input(name: str) -> "Sym":
        return Sym("in", name=name)

    @staticmethod
    def aux(name: str) -> "Sym":
        return Sym("aux", name=name)

    @staticmethod
    def param(name: str, slot: int) -> "Sym":
        """A learnable equation parameter (ParameterNode, symbolic.py:471-485): one scalar for all points."""
        return Sym("param", name=name, comp=int(slot))

    @staticmethod
    def const(v: Number) -> "Sym":
        return Sym("const", value=float(v))

    @staticmethod
    def net(model, comp: int, dirs: Sequence[str] = ()) -> "Sym":
        return Sym("net", model=model, comp=comp, dirs=tuple(sorted(dirs)))

    # ---- reference-tensor look-alike surface
    @property
    def shape(self):
        return [-1, 1]

    def detach(self) -> "Sym":
        return apply("detach", self)

    def __repr__(self):
        if self.kind == "in":
            return self.name
        if self.kind == "aux":
            return f"aux:{self.name}"
        if self.kind == "param":
            return f"param:{self.name}"
        if self.kind == "const":
            return repr(self.value)
        if self.kind == "net":
            k = self.model.output_keys[self.comp]
            return k + "".join(f"__{d}" for d in self.dirs)
        if self.kind == "rows":
            return f"{self.args[0]!r}[{self.comp[0]}:{'' if self.comp[1] is None else self.comp[1]}]"
        return f"{self.op}({', '.join(map(repr, self.args))})"

    # ---- arithmetic
    def __add__(self, o): return apply("add", self, _lift(o))
    def __radd__(self, o): return apply("add", _lift(o), self)
    def __sub__(self, o): return apply("sub", self, _lift(o))
    def __rsub__(self, o): return apply("sub", _lift(o), self)
    def __mul__(self, o): return apply("mul", self, _lift(o))
    def __rmul__(self, o): return apply("mul", _lift(o), self)
    def __truediv__(self, o): return apply("div", self, _lift(o))
    def __rtruediv__(self, o): return apply("div", _lift(o), self)
    def __pow__(self, o): return apply("pow", self, _lift(o))
    def __rpow__(self, o): return apply("pow", _lift(o), self)
    def __neg__(self): return apply("neg", self)
    def __pos__(self): return self

    # ---- values at trace time: data-dependent Python control flow (see `batch_values`)
    def _scalar(self, what: str):
        v = concrete_values(self, what)
        if v.size != 1:
            raise TypeError(f"{what} of a traced expression with {v.size} values: only one-element values convert to Python scalars")
        _TRACE.concretized.append(f"{what}({self!r}) = {float(v.reshape(-1)[0])!r}")
        return v.reshape(-1)[0]

    def __bool__(self):
        return bool(self._scalar("bool") != 0)

    def __float__(self):
        return float(self._scalar("float"))

    def __int__(self):
        return int(self._scalar("int"))

    def item(self):
        return float(self._scalar("item"))

    def _indicator(self, o, what):
        """The comparison as a traced per-point 0 / 1 value (what the reference's bool tensor stands for in
        `paddle.where(cond, a, b)`; examples/chip_heat/chip_heat.py:217-232): built from the VM's heaviside (x > 0 ? 1 : 0)
        and abs, derivative zero."""
        d = self - _lift(o)
        one = Sym.const(1.0)
        if what == "gt":
            return apply("heaviside", d)
        if what == "lt":
            return apply("heaviside", -d)
        if what == "ge":
            return one - apply("heaviside", -d)
        if what == "le":
            return one - apply("heaviside", d)
        if what == "eq":
            return one - apply("heaviside", apply("abs", d))
        return apply("heaviside", apply("abs", d))  # ne

    def _compare(self, o, f, what):
        if not isinstance(o, (Sym, int, float, np.floating, np.integer)):
            return NotImplemented
        if _TRACE.values is None:
            # No fixed batch to look at: the comparison itself is traced.  bool() of it still raises (see _scalar).
            return self._indicator(o, what)
        try:
            ov = concrete_values(o, what) if isinstance(o, Sym) else np.float32(o)
            v = f(concrete_values(self, what), ov)
        except TypeError:
            # a fixed batch, but the compared values depend on the network: no answer at trace time, a traced indicator
            return self._indicator(o, what)
        # (the ANSWER is part of the record: ranks of a data-parallel job see different shards and must not silently compile
        # different programs, compile.check_trace_decisions)
        if v.size == 1:
            ans = bool(v.reshape(-1)[0])
            _TRACE.concretized.append(f"{what}({self!r}) = {ans!r}")
            return ans
        # One answer per point of the fixed batch.  As a Python value it is the bool array the reference's tensor holds (its
        # use -- indexing, any(), all() -- specialises the trace to this batch, so it is recorded when it is LOOKED at);
        # handed to functional.where it is the traced indicator, which holds for any batch and specialises nothing.
        return _BatchMask(v, self, o, what)

    def __lt__(self, o): return self._compare(o, np.less, "lt")
    def __le__(self, o): return self._compare(o, np.less_equal, "le")
    def __gt__(self, o): return self._compare(o, np.greater, "gt")
    def __ge__(self, o): return self._compare(o, np.greater_equal, "ge")

    def __eq__(self, o):
        # two traced values: as a Python truth value, identity (nodes are hash-consed: the same structure IS the same object --
        # what `in` / dict lookups of this module rely on); as the condition of functional.where, the per-point comparison.
        # A number: the comparison of the reference's tensors, on the batch the trace is specialised to
        if isinstance(o, Sym):
            return _IdentityAnswer(self is o, self, o, "eq")
        return self._compare(o, np.equal, "eq")

    def __ne__(self, o):
        if isinstance(o, Sym):
            return _IdentityAnswer(self is not o, self, o, "ne")
        return self._compare(o, np.not_equal, "ne")

    __hash__ = object.__hash__

    def __getitem__(self, key):
        """`expr[a:b]`: ROWS a..b of the batch (examples/euler_beam/euler_beam.py:49-54 picks the boundary point each condition
        belongs to).  Legal as the whole of an output expression -- compile.CompiledConstraint turns a one-row slice into a
        per-point weight mask (see there) -- or under float() / bool() / a comparison (its value at trace time).  Anything
        else with it raises."""
        if isinstance(key, (int, np.integer)):  # x[k]: the reference's [1]-shaped row k
            key = slice(int(key), int(key) + 1 if int(key) != -1 else None)
        if isinstance(key, slice) and key.step in (None, 1) and all(isinstance(v, (int, type(None))) for v in (key.start, key.stop)):
            return Sym("rows", comp=(key.start or 0, key.stop), args=(self,))
        raise TypeError("a traced expression can only be indexed by a row x[k] or a contiguous row slice x[a:b]")

    # ---- batch reductions (tensor.mean() / .sum() in a user expression: utils/expression.py:96-102 runs arbitrary tensor code)
    def _reduce(self, op: str, axis, keepdim) -> "Sym":
        if axis not in (None, 0, (0,), [0], (0, 1), [0, 1]):
            raise NotImplementedError(f"{op}(axis={axis!r}) of a traced [N, 1] value: only the reduction over the batch")
        if self.kind == "rows":
            raise TypeError("a batch reduction of a row slice is not lowered (reduce the whole column)")
        if self.kind == "reduce" or (op == "mean" and self.kind == "const"):
            return self  # (already one scalar for the whole batch)
        return Sym("reduce", op=op, args=(self,))

    def mean(self, axis=None, keepdim=False):
        """One scalar for the whole batch (broadcast back over the points wherever it is used).  Lowered as a two-pass
        program (graph.lower): the sum is taken by a first launch and read as a parameter slot by the residual program;
        its adjoint is carried back to every point by a third launch.  Over the GLOBAL batch under data parallelism."""
        return self._reduce("mean", axis, keepdim)

    def sum(self, axis=None, keepdim=False):  # noqa: A003
        return self._reduce("sum", axis, keepdim)

    def sin(self): return apply("sin", self)
    def cos(self): return apply("cos", self)
    def tanh(self): return apply("tanh", self)
    def exp(self): return apply("exp", self)
    def log(self): return apply("log", self)
    def sqrt(self): return apply("sqrt", self)
    def abs(self): return apply("abs", self)
    def pow(self, o): return apply("pow", self, _lift(o))


# ---- the batch a trace is specialised to ------------------------------------------------------------------------------
# The reference evaluates expressions on real tensors, so Python may branch on their values (`if float(d["x"][0]) == 0:`,
# utils/expression.py:96-102 just calls the user function).  A trace cannot follow a value that changes from step to step;
# but a constraint whose batch is FIXED (full batch, no shuffling: the boundary / initial-condition sets such code looks
# at) has one answer for every step.  `batch_values(...)` gives the trace those values: float() / bool() / comparisons
# of expressions of the INPUT columns evaluate on them (fp32, the reference's dtype), the branch taken is the one the
# reference takes on every step, and the trace stays a per-point program for the kernels.  Values that depend on the
# network (they change as it trains) still raise.  `_TRACE.concretized` records what was asked, so that the caller can
# refuse to reuse such a trace for a batch with other values.
class _IdentityAnswer:
    """`symA == symB` / `symA != symB`: truthy by node identity; `.indicator()` is the traced per-point comparison."""
    __slots__ = ("_ans", "_a", "_b", "_what")

    def __init__(self, ans: bool, a: "Sym", b: "Sym", what: str):
        self._ans, self._a, self._b, self._what = bool(ans), a, b, what

    def __bool__(self):
        return self._ans

    def __eq__(self, other):
        return self._ans == bool(other)

    def __hash__(self):
        return hash(self._ans)

    def __repr__(self):
        return repr(self._ans)

    def indicator(self) -> "Sym":
        return self._a._indicator(self._b, self._what)


class _BatchMask(np.ndarray):
    """The per-point answers of a comparison on the fixed batch of a static constraint (a bool array), which also
    remembers the comparison: `functional.where` takes the traced indicator instead of the values."""

    def __new__(cls, values: np.ndarray, a: "Sym", b, what: str):
        obj = np.asarray(values, dtype=bool).view(cls)
        obj._cmp = (a, b, what)
        obj._noted = False
        return obj

    def __array_finalize__(self, obj):
        self._cmp = getattr(obj, "_cmp", None)
        self._noted = getattr(obj, "_noted", True)

    def _note(self):
        if not self._noted and self._cmp is not None:
            a, _, what = self._cmp
            v = np.asarray(self)
            _TRACE.concretized.append(f"{what}({a!r}) = {int(v.sum())} of {v.size} true, crc {zlib.crc32(np.packbits(v).tobytes()):08x}")
            self._noted = True

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        for x in inputs:
            if isinstance(x, _BatchMask):
                x._note()
        inputs = tuple(np.asarray(x) if isinstance(x, _BatchMask) else x for x in inputs)
        return getattr(ufunc, method)(*inputs, **kwargs)

    def __array_function__(self, func, types, args, kwargs):
        self._note()
        strip = lambda x: np.asarray(x) if isinstance(x, _BatchMask) else x  # noqa: E731
        return func(*[strip(a) for a in args], **{k: strip(v) for k, v in kwargs.items()})

    def __getitem__(self, key):
        self._note()
        return np.asarray(self)[key]

    def __bool__(self):
        self._note()
        return bool(np.asarray(self))

    def __iter__(self):
        self._note()
        return iter(np.asarray(self))

    def tolist(self):
        self._note()
        return np.asarray(self).tolist()

    def indicator(self) -> "Sym":
        a, b, what = self._cmp
        return a._indicator(b, what)


class _TraceState:
    values: Optional[Dict[str, np.ndarray]] = None
    concretized: List[str] = []


_TRACE = _TraceState()


@contextlib.contextmanager
def batch_values(values: Optional[Dict[str, object]]):
    """values: column name -> array of the bound batch (None: no specialisation, value requests raise)."""
    def host(a):
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        return a.astype(np.float32).reshape(-1)

    prev = (_TRACE.values, _TRACE.concretized)
    _TRACE.values = None if values is None else {k: host(v) for k, v in values.items()}
    _TRACE.concretized = []
    try:
        yield _TRACE
    finally:
        _TRACE.values, _TRACE.concretized = prev


_NUMPY_OPS = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power, "max": np.maximum,
              "min": np.minimum, "atan2": np.arctan2, "sin": np.sin, "cos": np.cos, "tanh": np.tanh, "exp": np.exp,
              "log": np.log, "sqrt": np.sqrt, "abs": np.abs, "sinh": np.sinh, "cosh": np.cosh, "tan": np.tan,
              "neg": np.negative, "sign": np.sign, "detach": lambda v: v, "asin": np.arcsin, "acos": np.arccos,
              "atan": np.arctan, "asinh": np.arcsinh, "acosh": np.arccosh, "atanh": np.arctanh, "ceil": np.ceil,
              "floor": np.floor}


def concrete_values(s: "Sym", what: str = "value") -> np.ndarray:
    """fp32 values of an expression of the input columns on the batch the trace is specialised to."""
    if _TRACE.values is None:
        raise TypeError(f"{what}() of the traced expression {s!r}: data-dependent Python control flow can only be followed for a "
                        "constraint whose batch is fixed (one full batch, no shuffling); this one changes every iteration")
    if s.kind in ("in", "aux"):
        if s.name not in _TRACE.values:
            raise TypeError(f"{what}() of {s!r}: the bound batch has no column {s.name!r}")
        return _TRACE.values[s.name]
    if s.kind == "const":
        return np.float32(s.value).reshape(1)
    if s.kind == "rows":
        a, b = s.comp
        return concrete_values(s.args[0], what)[a:b]
    if s.kind == "reduce":
        v = concrete_values(s.args[0], what).astype(np.float32)
        return np.asarray(v.mean(dtype=np.float32) if s.op == "mean" else v.sum(dtype=np.float32), dtype=np.float32).reshape(1)
    if s.kind == "op" and s.op in _NUMPY_OPS:
        with np.errstate(all="ignore"):
            return np.asarray(_NUMPY_OPS[s.op](*[concrete_values(a, what) for a in s.args]), dtype=np.float32)
    raise TypeError(f"{what}() of the traced expression {s!r}: it depends on the network (or a learnable parameter), whose value "
                    "changes every step -- data-dependent Python control flow on it cannot be lowered to the fused HIP path")


# ---- batch coupling by a constant matrix ------------------------------------------------------------------------------
# `lhs[:len(rhs)] - paddle.mm(int_mat, v)` (ppsci/equation/ide/volterra.py:66-77): rows i < R of the batch get the residual
# lhs_i - sum_q M[i, q] v_q, the other rows (the quadrature points) carry no residual.  Only legal as a WHOLE output expression:
# lower() turns it into a per-point program around two small matrix-vector launches (engine.FusedConstraint._forward_couplings).
# M is dense (Volterra: a few hundred entries) or a CsrMatrix (the fractional Laplacian, ppsci/equation/fpde/
# fractional_poisson.py:57-82: ~690 nonzeros per row of 100 k to 1.4 M columns), and may carry a scalar factor c (the residual is
# lhs - c M v, the factor applied by the kernel's alpha, not rounded into the entries).  The matrix travels on the `couple`
# node and from there into the Coupling record of lower(); CompiledConstraint uploads it and drops the host copy.
COUPLE_RHS_PREFIX, COUPLE_VBAR_PREFIX = "__couple_rhs__", "__couple_vbar__"


class CsrMatrix:
    """A constant [rows, cols] float32 matrix in CSR with int32 indices, checked on the host (the kernel trusts the indices)."""

    def __init__(self, row_ptr, col_idx, vals, shape):
        self.shape = (int(shape[0]), int(shape[1]))
        self.row_ptr = np.ascontiguousarray(np.asarray(row_ptr, dtype=np.int64))
        self.col_idx = np.ascontiguousarray(np.asarray(col_idx, dtype=np.int64))
        self.vals = np.ascontiguousarray(np.asarray(vals, dtype=np.float32))
        rows, cols = self.shape
        nnz = len(self.vals)
        if rows <= 0 or cols <= 0 or len(self.row_ptr) != rows + 1 or len(self.col_idx) != nnz:
            raise ValueError(f"CsrMatrix: inconsistent CSR arrays for shape {self.shape}")
        if nnz >= 2 ** 31 or cols >= 2 ** 31:
            raise ValueError(f"CsrMatrix: {nnz} nonzeros / {cols} columns exceed int32 indices")
        if self.row_ptr[0] != 0 or self.row_ptr[-1] != nnz or np.any(np.diff(self.row_ptr) < 0):
            raise ValueError("CsrMatrix: row_ptr must rise from 0 to nnz")
        if nnz and (self.col_idx.min() < 0 or self.col_idx.max() >= cols):
            raise ValueError(f"CsrMatrix: a column index outside [0, {cols})")
        self.row_ptr, self.col_idx = self.row_ptr.astype(np.int32), self.col_idx.astype(np.int32)

    @property
    def nnz(self) -> int:
        return len(self.vals)

    @staticmethod
    def from_coo(rows, cols, vals, shape) -> "CsrMatrix":
        """Entries sorted by row; within a row they keep their given order (which is the summation order)."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        order = np.argsort(rows, kind="stable")
        ptr = np.zeros(int(shape[0]) + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=int(shape[0])), out=ptr[1:])
        return CsrMatrix(ptr, np.asarray(cols, np.int64).reshape(-1)[order], np.asarray(vals, np.float32).reshape(-1)[order],
                         shape)

    def row_of_entries(self) -> np.ndarray:
        return np.repeat(np.arange(self.shape[0], dtype=np.int64), np.diff(self.row_ptr))

    def transpose(self) -> "CsrMatrix":
        """M^T in CSR; row q of it lists the entries of column q of M by increasing row (the dense transposed order)."""
        return CsrMatrix.from_coo(self.col_idx, self.row_of_entries(), self.vals, (self.shape[1], self.shape[0]))

    def crc(self) -> int:
        c = zlib.crc32(self.row_ptr.tobytes())
        c = zlib.crc32(self.col_idx.tobytes(), c)
        return zlib.crc32(self.vals.tobytes(), c)


def couple(lhs, matrix, v, factor: Optional[float] = None) -> "Sym":
    """lhs - factor * (M v) on the first M.shape[0] rows of the batch; `matrix` is a [rows, batch] array or a CsrMatrix."""
    if isinstance(matrix, CsrMatrix):
        M, crc = matrix, matrix.crc()
    else:
        M = np.ascontiguousarray(np.asarray(matrix, dtype=np.float32))
        if M.ndim != 2:
            raise ValueError(f"couple(): a [rows, batch] matrix is needed, got shape {M.shape}")
        crc = zlib.crc32(M.tobytes())
    return Sym("couple", name=f"couple_{crc:08x}", value=None if factor is None else float(factor),
               comp=(int(M.shape[0]), int(M.shape[1])), args=(_lift(lhs), _lift(v)), matrix=M)


def _lift(v) -> Sym:
    if isinstance(v, Sym):
        return v
    if isinstance(v, (int, float, np.floating, np.integer)):
        return Sym.const(float(v))
    if isinstance(v, np.ndarray) and v.size == 1:
        return Sym.const(float(v.reshape(-1)[0]))
    if hasattr(v, "_as_sym"):  # arch.spinn.GridLinear meeting a traced expression: it continues as an ordinary graph
        return v._as_sym()
    raise TypeError(f"cannot mix a traced expression with {type(v)}")


def is_const(s: Sym, v: Optional[float] = None) -> bool:
    return s.kind == "const" and (v is None or s.value == v)


def apply(op: str, *args: Sym) -> Sym:
    """Builds an op node.  Only exact algebraic identities with 0/1 are folded (they do not change the
    fp32 result), so the reference's operation order is preserved."""
    if any(a.kind == "rows" for a in args):
        raise TypeError("arithmetic on a row slice of the batch is not a per-point program")
    if any(a.kind == "couple" for a in args):
        raise TypeError("a batch-coupled residual (graph.couple) must be the whole output expression")
    if op in _BINARY_OPS:
        a, b = args
        if op == "add":
            if is_const(a, 0.0):
                return b
            if is_const(b, 0.0):
                return a
        elif op == "sub":
            if is_const(b, 0.0):
                return a
        elif op == "mul":
            if is_const(a, 0.0) or is_const(b, 0.0):
                return Sym.const(0.0)
            if is_const(a, 1.0):
                return b
            if is_const(b, 1.0):
                return a
        elif op == "div":
            if is_const(b, 1.0):
                return a
        elif op == "pow":
            if is_const(b, 1.0):
                return a
        if a.kind == "const" and b.kind == "const" and op in ("add", "sub", "mul"):
            f = {"add": np.add, "sub": np.subtract, "mul": np.multiply}[op]
            return Sym.const(float(f(np.float32(a.value), np.float32(b.value))))
        return Sym("op", op=op, args=(a, b))
    if op in _UNARY_OPS:
        (a,) = args
        if op == "neg" and a.kind == "const":
            return Sym.const(-a.value)
        return Sym("op", op=op, args=(a,))
    raise NotImplementedError(f"operation {op!r} is not supported by the epilogue VM")


# ----------------------------------------------------------------------------- differentiation
def net_raw_vars(model) -> Tuple[str, ...]:
    """The data-dict variables a network's outputs depend on: its input keys, or -- with a registered input
    transform -- the raw variables its input features are built from."""
    feats = getattr(model, "_traced_features", None)
    branch = getattr(model, "branch_keys", None)
    if branch:  # operator nets (arch/deeponet.py): the branch keys are [N, m] tensors of the executor, not stream variables
        return tuple(k for k in model.input_keys if k not in branch)
    if not feats:
        return tuple(model.input_keys)
    names: List[str] = []
    for n in _walk(list(feats.values())):
        if n.kind in ("in", "aux") and n.name not in names:
            names.append(n.name)
    return tuple(names)


def directional(e: Sym, d, order: int) -> Sym:
    """order-th derivative of e along direction d: a variable name, a pair (a, b) for the direction a + b, or a triple
    (a, b, -1.0) for a - b."""
    if isinstance(d, tuple):
        a, b = d[0], d[1]
        sgn = float(d[2]) if len(d) > 2 else 1.0
        if order <= 2 and sgn == 1.0:
            if order == 1:
                return diff(e, a) + diff(e, b)
            ea = diff(e, a)
            return diff(ea, a) + 2.0 * diff(ea, b) + diff(diff(e, b), b)
        out = e
        for _ in range(order):
            out = diff(out, a) + sgn * diff(out, b)
        return out
    out = e
    for _ in range(order):
        out = diff(out, d)
    return out


def diff(e: Sym, var: str) -> Sym:
    """d e / d var, symbolically (what jacobian() obtains numerically in the reference)."""
    k = e.kind
    if k in ("in", "aux"):  # (aux: a dataset column that is not a network input -- raw variable of an input transform, nu, sdf, ...)
        return Sym.const(1.0 if e.name == var else 0.0)
    if k in ("const", "param"):
        return Sym.const(0.0)
    if k == "couple":
        raise NotImplementedError("derivative of a batch-coupled residual w.r.t. a per-point variable")
    if k == "reduce":
        raise NotImplementedError(f"derivative of the batch reduction {e!r} w.r.t. the per-point variable {var!r}: differentiate "
                                  "first, reduce afterwards")
    if k == "net":
        if var in (getattr(e.model, "branch_keys", None) or ()):
            raise NotImplementedError(f"derivative of {type(e.model).__name__} output {e!r} w.r.t. its branch key {var!r}: "
                                      "derivatives run along the trunk keys only")
        if var not in net_raw_vars(e.model):
            return Sym.const(0.0)
        axis_max = getattr(e.model, "max_axis_order", None)
        if axis_max is not None:  # separable nets: any mixed derivative, bounded per axis by the branch nets' streams
            if e.dirs.count(var) >= axis_max:
                raise NotImplementedError(
                    f"derivative order {e.dirs.count(var) + 1} along axis {var!r} of the {type(e.model).__name__} output {e!r}: "
                    f"the branch nets carry orders 0..{axis_max} per axis")
        elif len(e.dirs) >= 4:
            raise NotImplementedError(
                f"derivative order {len(e.dirs) + 1} of a network output ({e!r} w.r.t. {var}) is beyond the fused "
                "HIP kernels (orders 0..4)")
        return Sym.net(e.model, e.comp, e.dirs + (var,))
    op, a = e.op, e.args
    if op == "detach":
        return Sym.const(0.0)
    if op == "add":
        return diff(a[0], var) + diff(a[1], var)
    if op == "sub":
        return diff(a[0], var) - diff(a[1], var)
    if op == "mul":
        return diff(a[0], var) * a[1] + a[0] * diff(a[1], var)
    if op == "div":
        return diff(a[0], var) / a[1] - e * diff(a[1], var) / a[1]
    if op == "neg":
        return -diff(a[0], var)
    if op == "pow":
        da, db = diff(a[0], var), diff(a[1], var)
        out = Sym.const(0.0)
        if not is_const(da, 0.0):
            out = out + a[1] * apply("pow", a[0], a[1] - 1.0) * da
        if not is_const(db, 0.0):
            out = out + e * apply("log", a[0]) * db
        return out
    if op == "atan2":  # atan2(y, x)
        den = a[0] * a[0] + a[1] * a[1]
        return (a[1] * diff(a[0], var) - a[0] * diff(a[1], var)) / den
    d = diff(a[0], var)
    if is_const(d, 0.0) or op in ("sign", "heaviside", "ceil", "floor"):
        return Sym.const(0.0)
    if op not in _UNARY_DIFF:
        raise NotImplementedError(f"derivative of {op!r}")
    return _UNARY_DIFF[op](e, a[0], d)


# d f(a) / d var of the elementwise functions, from e = f(a), a and d = d a / d var
_UNARY_DIFF = {
    "asin": lambda e, a, d: d / apply("sqrt", 1.0 - a * a),
    "acos": lambda e, a, d: -(d / apply("sqrt", 1.0 - a * a)),
    "atan": lambda e, a, d: d / (1.0 + a * a),
    "asinh": lambda e, a, d: d / apply("sqrt", a * a + 1.0),
    "acosh": lambda e, a, d: d / apply("sqrt", a * a - 1.0),
    "atanh": lambda e, a, d: d / (1.0 - a * a),
    "erf": lambda e, a, d: apply("exp", -(a * a)) * (2.0 / math.sqrt(math.pi)) * d,
    "sin": lambda e, a, d: apply("cos", a) * d,
    "cos": lambda e, a, d: -(apply("sin", a) * d),
    "tanh": lambda e, a, d: (1.0 - e * e) * d,
    "exp": lambda e, a, d: e * d,
    "log": lambda e, a, d: d / a,
    "sqrt": lambda e, a, d: d / (2.0 * e),
    "abs": lambda e, a, d: apply("sign", a) * d,
    "sinh": lambda e, a, d: apply("cosh", a) * d,
    "cosh": lambda e, a, d: apply("sinh", a) * d,
    "tan": lambda e, a, d: (1.0 + e * e) * d,
}


# ----------------------------------------------------------------------------- lowering
def _walk(roots: Iterable[Sym]) -> List[Sym]:
    seen, order = set(), []

    def rec(n: Sym):
        if id(n) in seen:
            return
        seen.add(id(n))
        for a in n.args:
            rec(a)
        order.append(n)

    for r in roots:
        rec(r)
    return order


# (n1, n2, n3, n4) combinations the kernels are instantiated for (taylor_fwd.inc / taylor_bwd.inc): first-order
# directions, and how many of the FIRST of them also carry second / third / fourth-order streams
_INSTANTIATED = [(0, 0, 0, 0), (1, 1, 0, 0), (2, 0, 0, 0), (2, 1, 0, 0), (2, 2, 0, 0), (3, 2, 0, 0), (3, 3, 0, 0),
                 (4, 3, 0, 0),  # unsteady 3-D NavierStokes: first derivatives along x, y, z, t, second along x, y, z
                 (1, 1, 1, 0), (1, 1, 1, 1), (2, 2, 2, 2), (4, 4, 4, 4)]


@dataclasses.dataclass(frozen=True)
class LossTerm:
    """One loss term, as lower() takes it: the output `key` against the aux columns named here (compile.loss_terms)."""
    key: str
    label: Optional[str] = None
    weight: Optional[str] = None
    area: Optional[str] = None
    scale: float = 1.0
    kind: int = 0  # hotpath.LOSS_*
    causal: Optional[str] = None  # CausalMSELoss: the aux column that carries the causal factor
    periodic: bool = False


@dataclasses.dataclass(frozen=True)
class NetSlot:
    """One network of the constraint and its block of rows of U."""
    model: object
    spec: hp.StreamSpec  # in ITS input order
    row0: int  # first row of U
    inputs: Optional[List[int]]  # indices of its inputs among the constraint's (None under an input transform)
    pre: Optional[List[tuple]] = None  # stream programs of an input transform: (Program, first feature row, rows)


@dataclasses.dataclass(frozen=True)
class CausalRow:
    """CausalMSELoss: a residual row and its label / weight / area / causal-factor aux columns (-1: none)."""
    row: int
    label_aux: int
    weight_aux: int
    area_aux: int
    factor_aux: int


@dataclasses.dataclass(frozen=True)
class PeriodicRow:
    """Periodic*Loss: the label column of this residual row receives the partner half's values."""
    row: int
    label_aux: int


@dataclasses.dataclass(frozen=True)
class Coupling:
    """One batch coupling lhs[:rows] - factor * (M v): its residual row and aux columns, and M itself until it is uploaded."""
    name: str
    rows: int
    cols: int
    res_row: int
    weight_aux: int
    rhs_aux: int
    vbar_aux: int
    factor: float
    matrix: object = None


@dataclasses.dataclass(frozen=True)
class CouplingPlan:
    items: Tuple[Coupling, ...]
    pv: hp.Program  # value pass: v of every coupling into a row of a [C, N] buffer
    p3: hp.Program  # adjoint pass: the residual program + one LINEAR term per coupling on v


@dataclasses.dataclass(frozen=True)
class ReductionPlan:
    k: int
    p1: hp.Program  # pass 1: the summands alone, one LINEAR term each
    p3: hp.Program  # pass 3: the residual program + one LINEAR term per summand, seeded with dL/dR_k


@dataclasses.dataclass
class Lowered:
    """Result of lowering: everything engine.FusedConstraint needs except the device arrays."""
    model: object
    streams: Optional[hp.StreamSpec]
    program: hp.Program
    input_names: List[str]
    aux_names: List[str]
    loss_keys: List[str]
    value_index: Dict[str, int]  # output name -> program value index
    nets: List[NetSlot]
    causal: List[CausalRow]
    periodic: List[PeriodicRow]
    param_slots: List[int]  # slots of the learnable equation parameters the program reads
    couplings: Optional[CouplingPlan] = None
    reductions: Optional[ReductionPlan] = None


def _check_separable(nodes, losses, jet) -> None:
    """What a separable net's grid path (spinn_engine.SpinnJetConstraint) does not run, refused with the reason."""
    what = type(jet.model).__name__
    for n in nodes:
        if n.kind == "param":
            raise NotImplementedError(f"learnable equation parameter {n.name!r} in a {what} residual: the grid path has no "
                                      "reduction for its gradient")
        if n.kind == "reduce":
            raise NotImplementedError(f"batch reduction {n!r} in a {what} residual: the grid is evaluated in one point-wise pass")
        if n.kind == "couple":
            raise NotImplementedError(f"batch coupling {n.name!r} in a {what} residual: the grid is evaluated in one point-wise pass")
        if n.kind == "rows":
            raise NotImplementedError(f"row slice {n!r} of a {what} residual: the output is a tensor-product grid, not a batch column")
        if n.kind == "net" and n.model is not jet.model:
            raise NotImplementedError(f"a second network in a {what} residual")
    for ls in losses:
        if ls.periodic:
            raise NotImplementedError(f"periodic loss on a {what} grid: its pairs are halves of a batch column")
        if ls.causal:
            raise NotImplementedError(f"causal loss on a {what} grid: its windows are chunks of a batch column")
        if ls.area:
            raise NotImplementedError(f"area column on a {what} grid")


def _validate(nodes, roots, n_global) -> Tuple[List[Sym], List[Sym], list]:
    """The batch reductions (Sym.mean / Sym.sum), the batch couplings (couple) and the networks (ModelList members, in
    order of appearance) among `nodes`, checked."""
    reduces = [n for n in nodes if n.kind == "reduce"]
    if reduces:
        if any(n.kind == "param" for n in nodes):
            raise NotImplementedError("batch reductions together with learnable equation parameters (both use the parameter slots)")
        if len(reduces) > L.MAX_EPARAM:
            raise NotImplementedError(f"more than {L.MAX_EPARAM} batch reductions in the expressions of one constraint")
        if any(m.kind == "reduce" for r in reduces for m in _walk([r.args[0]])):
            raise NotImplementedError("a batch reduction inside a batch reduction (e.g. a variance written with two means): "
                                      "one level is lowered")
        if any(r.op == "mean" for r in reduces) and not n_global:
            raise NotImplementedError("mean() over the batch needs the global batch size")
    couples = [n for n in nodes if n.kind == "couple"]
    if couples:
        if reduces:
            raise NotImplementedError("batch couplings together with batch reductions")
        if any(id(c) not in {id(r) for r in roots} for c in couples) or any(a.kind == "couple" for n in nodes for a in n.args):
            raise NotImplementedError("a batch-coupled residual must be the whole output expression")
    model_list = list({id(n.model): n.model for n in nodes if n.kind == "net"}.values())
    for mm in model_list:  # operator nets: a multi-column branch key is no per-point variable of the residual program
        cols = getattr(mm, "branch_cols", None) or {}
        for n in nodes:
            if n.kind in ("in", "aux") and cols.get(n.name, 1) != 1:
                raise NotImplementedError(f"expression reads the {cols[n.name]}-column branch key {n.name!r} of "
                                          f"{type(mm).__name__}: only one-column keys are per-point values")
    return reduces, couples, model_list


def _pure_streams(dirs) -> Optional[Tuple[list, bool]]:
    """The pure directional streams (all of order len(dirs)) the derivative `dirs` of a network output is assembled from, in
    the order the program loads them -- a direction is a variable, (a, b) for a + b or (a, b, -1.0) for a - b -- or None
    where the kernels carry no such set.  Read by the stream plan (which directions, to which order) and by
    _Emitter._net (the arithmetic on the loaded streams):
        u_ab   = (D2_{a+b} - D2_a - D2_b) / 2
        u_aab  = (D3_{a+b} - D3_{a-b} - 2 D3_b) / 6        (D3_{a+-b} = u_aaa +- 3 u_aab + 3 u_abb +- u_bbb)
        u_aabb = (D4_{a+b} + D4_{a-b} - 2 D4_a - 2 D4_b) / 12
    The flag is for u_aab: the difference stream is kept along lo - hi of the sorted pair (D3 along b - a is minus D3 along
    a - b: one stream serves u_aab and u_abb), and the flag says that this IS a - b."""
    vs, k = sorted(set(dirs)), len(dirs)
    if len(vs) == 1:
        return [vs[0]], True
    if k == 2:  # (a + b and b + a are ONE direction: one key)
        return [(vs[0], vs[1]), vs[0], vs[1]], True
    if k == 4 and len(vs) == 2 and dirs.count(vs[0]) == 2:
        return [(vs[0], vs[1]), (vs[0], vs[1], -1.0), vs[0], vs[1]], True
    if k == 3 and len(vs) == 2:  # (the shear forces of examples/biharmonic2d/biharmonic2d.py:325-336: d/dx (u_xx + u_yy))
        a, b = (vs[0], vs[1]) if dirs.count(vs[0]) == 2 else (vs[1], vs[0])
        return [(vs[0], vs[1]), (vs[0], vs[1], -1.0), b], a == vs[0]
    return None


@dataclasses.dataclass(frozen=True)
class _StreamPlan:
    """The derivative streams of one lowering: the constraint's input variables, the directions in stream order (higher
    orders first), their vectors padded to the instantiated (n1, n2, n3, n4) `counts`, and the StreamSpec (None: a jet)."""
    in_keys: List[str]
    dir_names: List[object]
    dirs_vec: List[List[float]]
    counts: Tuple[int, int, int, int]
    streams: Optional[hp.StreamSpec]

    @property
    def S(self) -> int:
        return self.streams.S if self.streams is not None else 1


def _plan_streams(nodes, model_list, jet) -> _StreamPlan:
    # order[d] = highest pure derivative order needed along direction d
    order: Dict[object, int] = {}
    for n in nodes:
        if n.kind != "net" or not n.dirs or jet is not None:
            continue
        pure = _pure_streams(n.dirs)
        if pure is None:
            raise NotImplementedError(
                f"mixed derivative {n!r}: beyond pure derivatives the fused HIP kernels carry u_ab, u_aab and u_aabb")
        for d in pure[0]:
            order[d] = max(order.get(d, 0), len(n.dirs))
    in_keys: List[str] = []  # union of the members' inputs: the constraint's input arrays
    for mm in model_list:
        in_keys += [k for k in net_raw_vars(mm) if k not in in_keys]
    if jet is not None:
        in_keys = list(jet.model.input_keys)

    def rank(d):  # variables in input order first, then the combined directions
        return (0, in_keys.index(d)) if isinstance(d, str) else (1, repr(d))

    dir_names: List[object] = sorted(order, key=lambda d: (-order[d], rank(d)))  # higher orders first: prefix property
    n1, n2, n3, n4 = (sum(1 for d in dir_names if order[d] >= k) for k in (1, 2, 3, 4))
    choice = None
    for c in _INSTANTIATED:
        if c[0] >= n1 and c[1] >= n2 and c[2] >= n3 and c[3] >= n4 and (choice is None or (c[2:], c[:2]) < (choice[2:], choice[:2])):
            choice = c
    if choice is None:
        raise NotImplementedError(f"derivative set with {n1} directions / {n2} second / {n3} third / {n4} fourth-order "
                                  f"streams exceeds the instantiated kernels {_INSTANTIATED}")
    dirs_vec: List[List[float]] = []
    for d in dir_names:
        v = [0.0] * len(in_keys)
        if isinstance(d, tuple):
            v[in_keys.index(d[0])] = 1.0
            v[in_keys.index(d[1])] = float(d[2]) if len(d) > 2 else 1.0
        else:
            v[in_keys.index(d)] = 1.0
        dirs_vec.append(v)
    while len(dirs_vec) < choice[0]:  # padding directions are zero vectors: their streams vanish identically
        dirs_vec.append([0.0] * len(in_keys))
    streams = hp.StreamSpec(dirs_vec, *choice[1:]) if jet is None else None
    return _StreamPlan(in_keys, dir_names, dirs_vec, choice, streams)


def _net_slots(model_list, plan: _StreamPlan) -> Tuple[List[NetSlot], Dict[int, list]]:
    """Every member carries the same stream set; its direction vectors are expressed in ITS input order (a variable a
    member does not take contributes nothing: its derivative along it is zero), and its streams are a block of rows of the
    constraint's U / Ubar arrays.  Also: id(model) -> per-feature stream expressions of a registered input transform."""
    slots, features, rows = [], {}, 0
    n1p, n2p, n3p, n4p = plan.counts
    padded = list(plan.dir_names) + [None] * (n1p - len(plan.dir_names))
    for mm in model_list:
        feats = getattr(mm, "_traced_features", None)
        if feats:
            # a registered input transform: the network's inputs are functions phi_k of the raw variables; the
            # kernels take phi_k and its derivative streams along the directions as [S, N] blocks (EMBED_STREAMS)
            idx = None
            blocks = []
            for k in mm.input_keys:
                phi = feats[k]
                rows_k = [phi] + [Sym.const(0.0) if d is None else directional(phi, d, 1) for d in padded]
                for kk, npk in ((2, n2p), (3, n3p), (4, n4p)):
                    rows_k += [Sym.const(0.0) if d is None else directional(phi, d, kk) for d in padded[:npk]]
                blocks.append(rows_k)
            features[id(mm)] = blocks
            spec = hp.StreamSpec([[0.0] * len(mm.input_keys) for _ in range(n1p)], n2p, n3p, n4p)
        else:
            idx = [plan.in_keys.index(k) for k in net_raw_vars(mm)]
            spec = hp.StreamSpec([[v[j] for j in idx] for v in plan.dirs_vec], n2p, n3p, n4p)
        slots.append(NetSlot(mm, spec, rows, idx))
        rows += len(mm.output_keys) * plan.S
    return slots, features


class _Emitter:
    """Writes traced nodes into epilogue programs.  One per lowering: its programs share the aux-column table (inputs that
    are not network inputs, e.g. parameters of a boundary function, are shipped as aux arrays) and the parameter slots."""

    def __init__(self, plan: _StreamPlan, slots: Sequence[NetSlot], reduces, couples, jet):
        self.plan, self.jet = plan, jet
        self.row0 = {id(s.model): s.row0 for s in slots}
        self.red_slot = {id(r): k for k, r in enumerate(reduces)}  # reduction k is read from parameter slot k
        self.couple_name = {id(c): f"couple{k}" for k, c in enumerate(couples)}
        self.dir_index = {d: i for i, d in enumerate(plan.dir_names)}
        self.input_names: List[str] = list(plan.in_keys)
        self.aux_names: List[str] = []
        self.param_slots = set()

    def aux_index(self, name: str) -> int:
        if name not in self.aux_names:
            self.aux_names.append(name)
        return self.aux_names.index(name)

    def emit(self, prog: hp.Program, nodes, val: Dict[int, int], pointwise: bool = False) -> None:
        """`nodes` (in dependency order) into `prog`; val: node id -> value index.  pointwise: inputs, aux arrays, constants
        and operators only (the stream programs of an input transform)."""
        for n in nodes:
            if n.kind in ("in", "aux"):
                v = prog.ld_in(self.input_names.index(n.name)) if n.name in self.input_names else prog.ld_aux(self.aux_index(n.name))
            elif n.kind == "const":
                v = prog.const(n.value)
            elif pointwise and n.kind in ("net", "param"):
                raise NotImplementedError("an input transform may only use the data-dict variables")
            elif n.kind == "param":
                v = prog.ld_param(n.comp)
                self.param_slots.add(n.comp)
            elif n.kind == "reduce":
                v = prog.ld_param(self.red_slot[id(n)])
            elif n.kind == "couple":  # lhs - (M v): the product is an aux column written between two launches
                v = prog.op(L.OP_SUB, val[id(n.args[0])], prog.ld_aux(self.aux_index(COUPLE_RHS_PREFIX + self.couple_name[id(n)])))
            elif n.kind == "net":
                v = prog.ld_u(self.jet.row(n)) if self.jet is not None else self._net(prog, n)
            elif n.op in _BINARY_OPS:
                v = prog.op(_BINARY_OPS[n.op], val[id(n.args[0])], val[id(n.args[1])])
            else:
                v = prog.op(_UNARY_OPS[n.op], val[id(n.args[0])])
            val[id(n)] = v

    def _net(self, prog: hp.Program, n: Sym) -> int:
        """A network output or derivative from the streams of its member (rows of a member start at a multiple of S); the
        identities of the mixed ones are stated at _pure_streams."""
        S, k = self.plan.S, len(n.dirs)
        q0 = (n.comp + self.row0[id(n.model)] // S) * S
        if k == 0:
            return prog.ld_u(q0)
        n1p, n2p, n3p, _ = self.plan.counts
        base = q0 + (1, 1 + n1p, 1 + n1p + n2p, 1 + n1p + n2p + n3p)[k - 1]
        streams, a_minus_b = _pure_streams(n.dirs)
        s = [prog.ld_u(base + self.dir_index[d]) for d in streams]
        if len(s) == 1:
            return s[0]
        if k == 2:
            t = prog.op(L.OP_SUB, prog.op(L.OP_SUB, s[0], s[1]), s[2])
            return prog.op(L.OP_MUL, prog.const(0.5), t)
        if k == 3:
            t = prog.op(L.OP_SUB if a_minus_b else L.OP_ADD, s[0], s[1])
            t = prog.op(L.OP_SUB, t, prog.op(L.OP_MUL, prog.const(2.0), s[2]))
            return prog.op(L.OP_MUL, prog.const(1.0 / 6.0), t)
        two = prog.const(2.0)
        t = prog.op(L.OP_SUB, prog.op(L.OP_SUB, prog.op(L.OP_ADD, s[0], s[1]), prog.op(L.OP_MUL, two, s[2])),
                    prog.op(L.OP_MUL, two, s[3]))
        return prog.op(L.OP_MUL, prog.const(1.0 / 12.0), t)


def _emit_losses(em: _Emitter, prog: hp.Program, val, outputs, losses, extra_outputs):
    """Residual row k of the program is losses[k]; `extra_outputs` follow as scale-0 rows.  Returns the row names, the
    causal and periodic rows and, per coupled output (node id), its (residual row, weight aux)."""
    loss_keys, causal, periodic, couple_rows = [], [], [], {}
    for ls in losses:
        out = outputs[ls.key]
        lab, w, ar = (em.aux_index(name) if name else -1 for name in (ls.label, ls.weight, ls.area))
        if ls.causal:
            # the residual's area slot carries exp(-tol * running loss) * area, written by ppsci_causal_weights
            cw = em.aux_index(ls.causal)
            causal.append(CausalRow(len(loss_keys), lab, w, ar, cw))
            prog.n_aux = max(prog.n_aux, ar + 1)
            ar = cw
        if ls.periodic:
            periodic.append(PeriodicRow(len(loss_keys), lab))
        value = val[id(out)]
        if out.kind == "couple":
            if ls.kind != 0 or ls.causal or ls.periodic or ar >= 0 or w < 0:
                raise NotImplementedError("a batch-coupled residual is lowered under MSELoss (no area column), with its row mask "
                                          "as the weight column")
            couple_rows[id(out)] = (len(loss_keys), w)
            # the term's difference d = lhs - M v - label is formed BY THE PROGRAM (the residual row then holds d, which is what
            # the transposed product of the reverse sweep needs: vbar = -M^T (2 scale w d))
            if lab >= 0:
                value, lab = prog.op(L.OP_SUB, value, prog.ld_aux(lab)), -1
        prog.residual(value, lab, w, ar, ls.scale, ls.kind)
        loss_keys.append(ls.key)
    for name in extra_outputs:
        prog.residual(val[id(outputs[name])], -1, -1, -1, 0.0)
        loss_keys.append(name)
    return loss_keys, causal, periodic, couple_rows


def _reduction_plan(em: _Emitter, prog: hp.Program, val, reduces, n_global) -> ReductionPlan:
    # pass 1: the summands alone, one LINEAR term each (scale 1 / N_global for a mean): its "loss terms" ARE the reductions
    p1 = hp.Program(prog.n_streams, prog.n_in)
    v1: Dict[int, int] = {}
    em.emit(p1, _walk([r.args[0] for r in reduces]), v1)
    coef = [1.0 / float(n_global) if r.op == "mean" else 1.0 for r in reduces]
    for r, c in zip(reduces, coef):
        p1.residual(v1[id(r.args[0])], -1, -1, -1, c, hp.LOSS_LINEAR)
    # pass 3: the residual program again + one LINEAR term per summand whose seed is c_k x dL/dR_k (a device value, written
    # by pass 2's block sums): with R held fixed, the gradient of  L(U, R) + sum_k Rbar_k c_k sum_p v_k(p)  w.r.t. U is
    # the gradient of the reference's loss, in which R depends on every point
    p3 = prog.copy()
    if len(p3.res) + len(reduces) > L.MAX_RES:
        raise NotImplementedError(f"{len(p3.res)} loss terms + {len(reduces)} batch reductions exceed the {L.MAX_RES} term "
                                  "slots of one epilogue program")
    for k, (r, c) in enumerate(zip(reduces, coef)):
        p3.residual(val[id(r.args[0])], -1, -1, -1, c, hp.LOSS_LINEAR, scale_param=k + 1)
    return ReductionPlan(len(reduces), p1, p3)


def _coupling_plan(em: _Emitter, prog: hp.Program, val, couples, couple_rows) -> CouplingPlan:
    if any(id(c) not in couple_rows for c in couples):
        raise NotImplementedError("a batch-coupled output needs a loss term (it has no values outside its rows)")
    # value program: v of every coupling into a row of a [C, N] buffer (scale-0 terms: values only)
    pv = hp.Program(prog.n_streams, prog.n_in)
    vv: Dict[int, int] = {}
    em.emit(pv, _walk([c.args[1] for c in couples]), vv)
    for c in couples:
        pv.residual(vv[id(c.args[1])], -1, -1, -1, 0.0)
    # adjoint program: the residual program + one LINEAR term per coupling on v, weighted per point by
    # vbar = -M^T (2 scale w r) (an aux column written between the launches): with rhs held fixed, the gradient of
    # L(U, rhs) + sum_q vbar_q v_q  w.r.t. U is the gradient of the reference's loss, in which rhs = M v(U)
    p3 = prog.copy()
    if len(p3.res) + len(couples) > L.MAX_RES:
        raise NotImplementedError(f"{len(p3.res)} loss terms + {len(couples)} batch couplings exceed the {L.MAX_RES} term slots")
    items = []
    for c in couples:
        name = em.couple_name[id(c)]
        vb = em.aux_index(COUPLE_VBAR_PREFIX + name)
        p3.n_aux = max(p3.n_aux, vb + 1)
        p3.residual(val[id(c.args[1])], -1, vb, -1, 1.0, hp.LOSS_LINEAR)
        row, w = couple_rows[id(c)]
        items.append(Coupling(name, c.comp[0], c.comp[1], row, w, em.aux_names.index(COUPLE_RHS_PREFIX + name), vb,
                              1.0 if c.value is None else c.value, c.matrix))
    return CouplingPlan(tuple(items), pv, p3)


def _feature_programs(em: _Emitter, features: Dict[int, list], n_in: int) -> Dict[int, list]:
    """Stream programs of the input transforms: <= MAX_RES output rows per program, rows in (feature, stream) order."""
    pre = {}
    for mid, blocks in features.items():
        flat_rows = [e for rows_k in blocks for e in rows_k]
        progs = []
        for r0 in range(0, len(flat_rows), L.MAX_RES):
            chunk = flat_rows[r0:r0 + L.MAX_RES]
            pg = hp.Program(0, n_in)
            pval: Dict[int, int] = {}
            em.emit(pg, _walk(chunk), pval, pointwise=True)
            for e in chunk:
                pg.residual(pval[id(e)], -1, -1, -1, 0.0)
            progs.append((pg, r0, len(chunk)))
        pre[mid] = progs
    return pre


def lower(outputs: Dict[str, Sym], losses: Sequence[LossTerm], extra_outputs: Sequence[str] = (),
          n_global: Optional[int] = None, jet=None) -> Lowered:
    """outputs: name -> traced expression.  Residual row k of the epilogue corresponds to losses[k]; `extra_outputs` are
       appended as scale-0 residual rows so that eval / predict can read their values.
       jet: the stream choice of a separable net (arch.spinn.JetTable) instead of the Taylor kernels' direction set: U row q is
       the q-th distinct per-axis order triple the program reads, in order of first use; the program is emitted as for any
       other model."""
    losses = [ls if isinstance(ls, LossTerm) else LossTerm(**ls) for ls in losses]  # (callers that still pass key -> value rows)
    roots = list(outputs.values())
    nodes = _walk(roots)
    if jet is not None:
        _check_separable(nodes, losses, jet)
    reduces, couples, model_list = _validate(nodes, roots, n_global)
    plan = _plan_streams(nodes, model_list, jet)
    slots, features = _net_slots([] if jet is not None else model_list, plan)
    em = _Emitter(plan, slots, reduces, couples, jet)
    prog = hp.Program(sum(len(s.model.output_keys) for s in slots) * plan.S, len(plan.in_keys))
    val: Dict[int, int] = {}
    em.emit(prog, nodes, val)
    if jet is not None:
        prog.n_streams = len(jet.orders)
    loss_keys, causal, periodic, couple_rows = _emit_losses(em, prog, val, outputs, losses, extra_outputs)
    param_slots = sorted(em.param_slots)
    # (the aux columns are numbered in order of first use: residual program, loss terms, coupling adjoints, stream programs)
    reductions = _reduction_plan(em, prog, val, reduces, n_global) if reduces else None
    couplings = _coupling_plan(em, prog, val, couples, couple_rows) if couples else None
    pre = _feature_programs(em, features, len(plan.in_keys))
    return Lowered(model_list[0] if model_list else None, plan.streams, prog, em.input_names, em.aux_names, loss_keys,
                   {k: val[id(v)] for k, v in outputs.items()}, [dataclasses.replace(s, pre=pre.get(id(s.model))) for s in slots],
                   causal, periodic, param_slots, couplings, reductions)
