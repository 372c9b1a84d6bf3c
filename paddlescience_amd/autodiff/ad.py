"""ppsci.autodiff surface (/root/reference/ppsci/autodiff/ad.py) on traced expressions.

In the reference `jacobian(ys, xs)` is one `paddle.grad(ys, xs, create_graph=True)` reverse sweep and
`hessian` two of them (ad.py:56-77, 181-236), cached per (ys, xs) object pair until `clear()`
(ad.py:326-341).  Here ys / xs are `graph.Sym` proxies: the derivative is taken symbolically down to
network-output leaves, which the Taylor-mode HIP kernel then evaluates in its forward pass.  The
call signatures, the cache-by-identity behaviour and the error conditions follow the reference."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union


from ..graph import Sym, diff


def _check_x(x):
    if not isinstance(x, Sym) or x.kind not in ("in", "aux"):
        raise TypeError(
            "jacobian/hessian: `xs` must be input variables of the data dict (e.g. out['x']); got "
            f"{x!r}.  Numeric tensors carry no autograd graph on the fused HIP path.")


def _separable_output(ys):
    """The separable net (ppsci.arch.SPINN) `ys` is an output of, or None."""
    if hasattr(ys, "_as_sym"):
        return ys.model
    if isinstance(ys, Sym):
        from ..graph import _walk

        for n in _walk([ys]):
            if n.kind == "net" and getattr(n.model, "max_axis_order", None) is not None:
                return n.model
    return None


def _refuse_separable(what: str, ys) -> None:
    m = _separable_output(ys)
    if m is not None:
        raise NotImplementedError(
            f"{what} on a {type(m).__name__} output: in the reference paddle.grad(u[Nx,Ny,Nz,1], x[Nx,1]) sums over the two other "
            "axes of the grid, it is not a per-point derivative.  Write the derivative with ppsci.autodiff.jvp, "
            "ppsci.equation.pde.helmholtz.hvp_revrev or model.derivative(...), as the reference's SPINN examples do.")


class Jacobians:
    def __init__(self):
        self.Js: Dict[Tuple[int, int], tuple] = {}

    def _one(self, ys: Sym, x: Sym, i: int, j: Optional[int]) -> Sym:
        _check_x(x)
        if not 0 <= i < 1:
            raise ValueError(f"i({i}) should in range [0, 1).")
        if j is not None and not 0 <= j < 1:
            raise ValueError(f"j({j}) should in range [0, 1).")
        key = (id(ys), id(x))
        if key not in self.Js:  # (the entry holds its operands: the ids of a key are not reused while it exists)
            self.Js[key] = (diff(ys, x.name), ys, x)
        return self.Js[key][0]

    def __call__(self, ys: Sym, xs: Union[Sym, List[Sym]], i: int = 0, j: Optional[int] = None,
                 retain_graph: Optional[bool] = None, create_graph: bool = True):
        _refuse_separable("jacobian", ys)
        if not isinstance(ys, Sym):
            raise TypeError("jacobian: `ys` must be a traced expression (output of model(...) or an expression of it); numeric "
                            "tensors carry no derivative graph here -- derivatives are streams of the Taylor-mode kernels")
        if not isinstance(xs, (list, tuple)):
            return self._one(ys, xs, i, j)
        return [self._one(ys, x, i, j) for x in xs]

    def _clear(self):
        self.Js = {}


class Hessians:
    def __init__(self, jac: Jacobians):
        self.Hs: Dict[Tuple[int, int, Optional[int]], tuple] = {}
        self._jac = jac

    def __call__(self, ys: Sym, xs: Sym, component: Optional[int] = None, i: int = 0, j: int = 0,
                 grad_y: Optional[Sym] = None, retain_graph: Optional[bool] = None, create_graph: bool = True) -> Sym:
        _refuse_separable("hessian", ys)
        if component is not None:  # every traced field is [N, 1]  (ad.py:214-218)
            raise ValueError(f"component{component} should be set to None when dim_y(1)=1.")
        key = (id(ys), id(xs), component)
        if key not in self.Hs:
            if grad_y is None:
                grad_y = self._jac(ys, xs, i=0, j=None)
            self.Hs[key] = (grad_y, ys, xs)
        return self._jac(self.Hs[key][0], xs, i, j)

    def _clear(self):
        self.Hs = {}


jacobian = Jacobians()
hessian = Hessians(jacobian)


def jvp(func, xs, v=None):
    """paddle.incubate.autograd.jvp on traced inputs, with the default unit tangents: returns (outputs, tangents) of
    `func(*xs)`; `func` may return one traced value or a list of them (then both results are lists).  The tangent of an output
    is its symbolic derivative along each primal's variable, summed over the primals -- what forward mode computes numerically
    in the reference (equation/pde/helmholtz.py:27-41 nests two of them for a second derivative)."""
    if v is not None:
        raise NotImplementedError("jvp: explicit tangents; traced derivatives are taken along the unit tangents (the default)")
    primals = tuple(xs) if isinstance(xs, (list, tuple)) else (xs,)
    for x in primals:
        if not isinstance(x, Sym) or x.kind not in ("in", "aux"):
            raise TypeError(
                f"jvp: primals must be input variables of the traced data dict (e.g. data['x']); got {type(x).__name__}.  Numeric "
                "tensors carry no derivative graph here: derivatives are streams of the HIP kernels, chosen while the expression "
                "is traced")
    out = func(*primals)
    is_seq = isinstance(out, (list, tuple))

    def tangent(o):
        o = o._as_sym() if hasattr(o, "_as_sym") else o
        if not isinstance(o, Sym):
            raise TypeError(f"jvp: `func` must return traced values, got {type(o).__name__}")
        t = diff(o, primals[0].name)
        for x in primals[1:]:
            t = t + diff(o, x.name)
        return t

    outs = list(out) if is_seq else [out]
    tans = [tangent(o) for o in outs]
    return (outs, tans) if is_seq else (outs[0], tans[0])


def clear():
    """Drop the cached Jacobians / Hessians (ad.py:326-341)."""
    jacobian._clear()
    hessian._clear()
