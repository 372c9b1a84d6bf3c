"""ppsci.arch.SPINN (/root/reference/ppsci/arch/spinn.py:29-180) with ModifiedMLP branch nets
(/root/reference/ppsci/arch/mlp.py:318-527) on the HIP kernels of csrc/spinn.hip.

One branch net per input axis maps a coordinate [N_a,1] to r*m features; the output on the tensor-product
grid is u[i,j,k] = sum_r fx[i,r] fy[j,r] fz[k,r] (spinn.py:140-167).  All parameters live in one flat fp32
buffer (branch 0, branch 1, branch 2; inside a branch in `parameters()` order).  Linear layers are
re-initialised glorot-normal with zero bias like SPINN._init_weights (spinn.py:107-111).

Traced use (expression compilation) returns `GridLinear` proxies: linear combinations of
{u, u_xx, u_yy, u_zz}, which is what Helmholtz / Poisson-type residuals on a separable net need and what the
four-coefficient grid kernels run.  Anything else -- u*u, u*u_x, sin(u), a mixed derivative, a coordinate factor --
continues as an ordinary `Sym` graph over the per-axis derivative streams (orders 0..2 per axis) and runs on the
general grid kernels of csrc/spinn_jet.inc with the epilogue VM between them."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from ..device import get_device
from ..utils import initializer
from ..graph import Sym
from ..hotpath import _p, _stream_ptr
from . import activation as act_mod
from .base import Arch


class GridLinear:
    """cu*u + cxx*u_xx + cyy*u_yy + czz*u_zz on the tensor-product grid of a SPINN.

    A residual that stays of this form runs on the four-coefficient grid kernels.  Any other operation -- a product of two
    forms, a function, meeting a traced expression -- continues with the ordinary expression graph of the same form (`sym`,
    kept in the order the user wrote it), which is lowered for the general grid path (csrc/spinn_jet.inc)."""

    def __init__(self, model, cu=0.0, cxx=0.0, cyy=0.0, czz=0.0):
        self.model, self.c = model, np.array([cu, cxx, cyy, czz], dtype=np.float64)
        # the same form as an expression graph, built in the order the user wrote it (what a promotion continues with)
        keys = model.input_keys
        self.sym = Sym.const(0.0)
        for q, c in enumerate(self.c):
            if c != 0.0:
                self.sym = self.sym + float(c) * Sym.net(model, 0, () if q == 0 else (keys[q - 1],) * 2)

    def _new(self, c, sym):
        g = GridLinear.__new__(GridLinear)
        g.model, g.c, g.sym = self.model, c, sym
        return g

    def _as_sym(self) -> Sym:
        return self.sym

    @property
    def shape(self):
        return [-1, 1]

    def __add__(self, o):
        if isinstance(o, GridLinear):
            return self._new(self.c + o.c, self.sym + o.sym)
        if isinstance(o, (int, float)) and o == 0:
            return self
        return self.sym + o

    def __radd__(self, o):
        if isinstance(o, (int, float)) and o == 0:
            return self
        return o + self.sym

    def __sub__(self, o):
        if isinstance(o, GridLinear):
            return self._new(self.c - o.c, self.sym - o.sym)
        return self.sym - o

    def __rsub__(self, o):
        return o - self.sym

    def __mul__(self, k):
        if isinstance(k, (int, float, np.floating)):
            return self._new(self.c * float(k), self.sym * float(k))
        return self.sym * k

    def __rmul__(self, k):
        if isinstance(k, (int, float, np.floating)):
            return self._new(self.c * float(k), float(k) * self.sym)
        return k * self.sym

    def __neg__(self):
        return self._new(-self.c, -self.sym)

    def __truediv__(self, o):
        return self.sym / o

    def __rtruediv__(self, o):
        return o / self.sym

    def __pow__(self, o):
        return self.sym ** o

    def __rpow__(self, o):
        return o ** self.sym

    def __getattr__(self, name):  # u.sin(), u.tanh(), u.detach(), ...: the traced tensor surface of graph.Sym
        if name.startswith("_") or not hasattr(Sym, name):
            raise AttributeError(name)
        return getattr(self.sym, name)


class JetTable:
    """The stream choice of one SPINN constraint for graph.lower: the distinct per-axis order triples (a, b, c) in {0,1,2}^3
    its residual program reads, in order of first use.  Row q of the grid arrays U / Ubar is triple q."""

    def __init__(self, model):
        self.model, self.orders = model, []

    def row(self, n: Sym) -> int:
        keys = self.model.input_keys
        t = tuple(n.dirs.count(k) for k in keys)
        for k, o in zip(keys, t):
            if o > 2:
                raise NotImplementedError(f"derivative order {o} along axis {k!r} of a SPINN output: the branch nets carry orders 0..2")
        if t not in self.orders:
            if len(self.orders) >= L.SPINN_MAX_JET:
                raise NotImplementedError(f"the residuals of one SPINN constraint read more than {L.SPINN_MAX_JET} distinct "
                                          f"derivative streams (PPSCI_SPINN_MAX_JET); split the constraint")
            self.orders.append(t)
        return self.orders.index(t)


class ModifiedMLPSpec:
    """Shape of a one-input ModifiedMLP branch as the kernels see it."""

    def __init__(self, num_layers: int, hidden_size: int, d_out: int, activation: str):
        self.desc = L.ModMlpDesc()
        self.desc.n_hidden, self.desc.width, self.desc.d_out = num_layers, hidden_size, d_out
        self.desc.activation = L.ACT[activation]
        self.L, self.H, self.R = num_layers, hidden_size, d_out

    def param_shapes(self) -> List[Tuple[str, Tuple[int, ...]]]:
        H, out = self.H, []
        out += [("embed_u.0.weight", (1, H)), ("embed_u.0.bias", (H,)), ("embed_v.0.weight", (1, H)), ("embed_v.0.bias", (H,))]
        fin = 1
        for l in range(self.L):
            out += [(f"linears.{l}.weight", (fin, H)), (f"linears.{l}.bias", (H,))]
            fin = H
        out += [("last_fc.weight", (H, self.R)), ("last_fc.bias", (self.R,))]
        return out

    @property
    def n_params(self) -> int:
        return int(sum(int(np.prod(s)) for _, s in self.param_shapes()))


class SPINN(Arch):
    max_axis_order = 2  # per-axis derivative order of the branch nets' streams (graph.diff)

    def __init__(self, input_keys: Tuple[str, ...], output_keys: Tuple[str, ...], r: int, num_layers: int,
                 hidden_size: Union[int, Tuple[int, ...]], activation: str = "tanh", skip_connection: bool = False,
                 weight_norm: bool = False, periods=None, fourier=None, random_weight=None):
        super().__init__()
        if len(input_keys) != 3 or len(output_keys) != 1:
            raise NotImplementedError("the HIP SPINN path covers 3 input axes and one output: the reference's forward_tensor(x, y, z) "
                                      "is fixed at three axes and its multi-output slicing returns the whole rank "
                                      "(spinn.py:140-167)")
        if skip_connection or weight_norm or periods or fourier or random_weight or not isinstance(hidden_size, int):
            raise NotImplementedError("SPINN options beyond plain ModifiedMLP branches have no HIP kernel yet")
        self.input_keys, self.output_keys, self.r = tuple(input_keys), tuple(output_keys), r
        self.activation = act_mod.get_activation(activation)
        if self.activation not in ("tanh", "silu", "sin"):
            raise NotImplementedError(f"SPINN branch nets: activation {activation!r} has no HIP kernel (tanh, silu, sin)")
        self.spec = ModifiedMLPSpec(num_layers, hidden_size, r * len(output_keys), self.activation)
        self.branch_params = self.spec.n_params
        self.flat_params = torch.zeros(3 * self.branch_params, dtype=torch.float32, device=get_device())
        self._names, self._views = [], []
        for b in range(3):
            off = b * self.branch_params
            for name, shp in self.spec.param_shapes():
                n = int(np.prod(shp))
                self._names.append(f"branch_nets.{b}.{name}")
                v = self.flat_params[off:off + n].view(*shp)
                self._views.append(v)
                if len(shp) == 2:  # SPINN._init_weights (spinn.py:107-111): glorot_normal_ weights, zero biases
                    initializer.glorot_normal_(v)
                off += n

    def branch(self, b: int) -> torch.Tensor:
        return self.flat_params[b * self.branch_params:(b + 1) * self.branch_params]

    def parameters(self):
        return list(self._views)

    def state_dict(self):
        return dict(zip(self._names, self._views))

    def set_state_dict(self, state):
        for n, v in zip(self._names, self._views):
            if n in state:
                v.copy_(torch.as_tensor(np.asarray(state[n]), dtype=torch.float32))
        return [n for n in self._names if n not in state], [n for n in state if n not in self._names]

    # ---- kernels
    def branch_forward(self, b: int, x: torch.Tensor, stash: Optional[torch.Tensor] = None) -> torch.Tensor:
        n = x.numel()
        F = torch.empty((3, n, self.spec.R), dtype=torch.float32, device=x.device)
        L.check(L.lib().ppsci_modmlp_fwd(C.byref(self.spec.desc), _p(self.branch(b)), n, _p(x), _p(F), _p(stash),
                                         _stream_ptr(x)))
        return F

    def _coords(self, x: Dict[str, object]) -> List[torch.Tensor]:
        dev = self.flat_params.device
        out = []
        for k in self.input_keys:
            v = x[k]
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float32))
            out.append(v.to(device=dev, dtype=torch.float32).contiguous().view(-1))
        return out

    def forward(self, x: Dict[str, object]):
        if any(isinstance(v, Sym) for v in x.values()):
            return {self.output_keys[0]: GridLinear(self, cu=1.0)}
        xs = self._coords(x)
        Fs = [self.branch_forward(b, xs[b]) for b in range(3)]
        d = L.SpinnGridDesc()
        d.n[0], d.n[1], d.n[2] = (t.numel() for t in xs)
        d.rank, d.cu, d.cxx, d.cyy, d.czz, d.scale = self.spec.R, 1.0, 0.0, 0.0, 0.0, 0.0
        total = xs[0].numel() * xs[1].numel() * xs[2].numel()
        res = torch.empty(total, dtype=torch.float32, device=xs[0].device)
        part = torch.empty(int(L.lib().ppsci_spinn_grid_partial_rows(C.byref(d))), dtype=torch.float32, device=res.device)
        L.check(L.lib().ppsci_spinn_grid_fwd(C.byref(d), _p(Fs[0]), _p(Fs[1]), _p(Fs[2]), None, _p(res), None, _p(part),
                                             _stream_ptr(res)))
        u = res.view(xs[0].numel(), xs[1].numel(), xs[2].numel(), 1)
        out = {self.output_keys[0]: u}
        if self._output_transform is not None:
            out = self._output_transform(x, out)
        return out

    def forward_tensor(self, x, y, z):
        return [self.forward({self.input_keys[0]: x, self.input_keys[1]: y, self.input_keys[2]: z})[self.output_keys[0]]]

    def second_derivative(self, axis_key: str) -> GridLinear:
        i = self.input_keys.index(axis_key)
        c = [0.0, 0.0, 0.0, 0.0]
        c[1 + i] = 1.0
        return GridLinear(self, *c)

    def derivative(self, *axis_keys: str):
        """The derivative of the output along the given axes on the tensor-product grid, as a traced expression:
        derivative("x") is u_x, derivative("x", "y") u_xy, derivative() u.  Per-axis order <= 2 (the branch nets' streams).
        u and the pure second derivatives stay linear forms (GridLinear), so that a residual made of them alone keeps the
        four-coefficient kernels."""
        for k in axis_keys:
            if k not in self.input_keys:
                raise KeyError(f"SPINN.derivative: {k!r} is not an input axis {self.input_keys}")
        for k in self.input_keys:
            if axis_keys.count(k) > self.max_axis_order:
                raise NotImplementedError(f"SPINN.derivative: order {axis_keys.count(k)} along axis {k!r}; the branch nets carry "
                                          f"orders 0..{self.max_axis_order} per axis")
        if len(axis_keys) == 0:
            return GridLinear(self, cu=1.0)
        if len(axis_keys) == 2 and axis_keys[0] == axis_keys[1]:
            return self.second_derivative(axis_keys[0])
        return Sym.net(self, 0, axis_keys)
