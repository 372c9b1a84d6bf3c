"""Training engine for separable PINNs (ppsci.arch.SPINN): per constraint
  3 x modmlp_fwd  ->  spinn_grid_fwd (residual + MSE + adjoint)  ->  spinn_grid_bwd  ->  3 x modmlp_bwd,
then one fixed-order reduction per branch into the flat gradient, one all-reduce, one fused Adam.
Counterpart of the generic engine.py for BASELINE config 5 (examples/spinn/helmholtz3d.py of the
reference: one PDE constraint on the nc^3 grid + six boundary faces).  Data parallelism shards the
points of one axis rank-strided (each rank owns an [nx/W, ny, nz] slab of the interior grid); branch nets are replicated.
SpinnEngine and its two constraint kinds implement the engine contract stated in engine.py's docstring."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import autodiff, graph
from . import hotpath as hp
import os

from .arch.spinn import GridLinear, JetTable
from .compile import LABEL_PREFIX, WEIGHT_PREFIX, loss_terms
from .engine import StepGraph, run_on_streams
from .hotpath import _p, _stream_ptr


def _fp(a):
    """What bind() takes for "the same array as last time": the object and three sampled values."""
    f = np.asarray(a).reshape(-1)
    n = f.shape[0]
    return (id(a), n, float(f[0]), float(f[n // 2]), float(f[n - 1])) if n else (id(a), 0)


def _alloc_branches(c, shape) -> None:
    """Both constraint kinds' buffers for the three branch nets: points, factors, their adjoints, the stash, the gradient rows
    (one per 16-point tile on the MFMA tile kernel of the reverse sweep, one per point otherwise).  With equal point counts the
    rows interleave as [n][3][P]: one reduce_rows(n, 3P) sums all three into the flat gradient (branch b: grad[bP:(b+1)P])."""
    m = c.model
    R, P = m.spec.R, m.branch_params
    f32 = dict(dtype=torch.float32, device=c.device)
    c.x = [torch.zeros(n, **f32) for n in shape]
    c.F = [torch.zeros((3, n, R), **f32) for n in shape]
    c.Fbar = [torch.zeros((3, n, R), **f32) for n in shape]
    c.stash = [torch.zeros(int(L.lib().ppsci_modmlp_stash_floats(C.byref(m.spec.desc), n)), **f32) for n in shape]
    grows = [int(L.lib().ppsci_modmlp_bwd_rows(C.byref(m.spec.desc), n)) for n in shape]
    c.gjoint = len(set(shape)) == 1
    if c.gjoint:
        c.gpart_all = torch.zeros((grows[0], 3 * P), **f32)
        c.gpart = [c.gpart_all.view(-1)[b * P:] for b in range(3)]  # row 0 of branch b; rows are 3P apart
    else:
        c.gpart = [torch.zeros((r, P), **f32) for r in grows]


class SpinnConstraint:
    def __init__(self, name: str, model, coeffs: np.ndarray, label_key: str, scale_fn, device, world: int = 1,
                 rank: int = 0):
        self.name, self.model, self.label_key = name, model, label_key
        self.coeffs = np.asarray(coeffs, dtype=np.float64)
        self.scale_fn = scale_fn  # total_points -> loss scale
        self.device, self.world, self.rank = device, world, rank
        self.shape = None
        self._last_ids = [None] * 4
        self._uploaded = [None] * 4
        self._version = 0  # bumped whenever the device buffers are re-allocated (captured graphs hold addresses)

    def _alloc(self, shape):
        m, dev = self.model, self.device
        self.shape = tuple(shape)
        self._version += 1
        self._last_ids, self._uploaded = [None] * 4, [None] * 4
        nx, ny, nz = shape
        R = m.spec.R
        f32 = dict(dtype=torch.float32, device=dev)
        _alloc_branches(self, shape)
        total = nx * ny * nz
        self.label = torch.zeros(total, **f32)
        self.gadj = torch.zeros(total, **f32)
        self.desc = L.SpinnGridDesc()
        self.desc.n[0], self.desc.n[1], self.desc.n[2] = nx, ny, nz
        self.desc.rank = R
        self.desc.cu, self.desc.cxx, self.desc.cyy, self.desc.czz = (float(c) for c in self.coeffs)
        self.lrows = int(L.lib().ppsci_spinn_grid_partial_rows(C.byref(self.desc)))
        self.lpart = torch.zeros(self.lrows, **f32)
        self.bscratch = torch.zeros(max(4, int(L.lib().ppsci_spinn_grid_bwd_scratch_floats(C.byref(self.desc)))), **f32)
        self.loss_term = torch.zeros(1, **f32)

    lcols = 1  # columns of `lpart` / entries of `loss_term` (one loss key)
    step_obj = property(lambda self: self)

    @property
    def scale_key(self):  # what a captured step holds by value besides the buffers
        return float(self.desc.scale)

    def losses(self) -> Dict[str, float]:
        return {self.label_key: self.loss()}

    def bind(self, input: Dict[str, np.ndarray], label: Dict[str, np.ndarray], weight: Optional[Dict[str, np.ndarray]] = None):
        if weight:
            raise NotImplementedError("per-point weights on the four-coefficient SPINN path (the solver compiles a weighted "
                                      "constraint for the general path)")
        keys = self.model.input_keys
        arrs = [np.asarray(input[k], dtype=np.float32).reshape(-1) for k in keys]
        lab = np.asarray(label[self.label_key], dtype=np.float32)
        gshape = tuple(a.shape[0] for a in arrs)
        rep = 1.0
        if self.world > 1:
            # rank-strided slab along the first axis that has at least `world` points (x for the interior grid,
            # y or z for the boundary faces whose x-axis is a single point); a grid smaller than that on every
            # axis is evaluated by all ranks and weighted 1/world so that the SUM all-reduce stays exact
            ax = next((i for i, n in enumerate(gshape) if n >= self.world), None)
            if ax is None:
                rep = 1.0 / self.world
            else:
                arrs[ax] = arrs[ax][self.rank::self.world]
                idx = [slice(None)] * 3
                idx[ax] = slice(self.rank, None, self.world)
                lab = lab.reshape(gshape)[tuple(idx)]
        shape = tuple(a.shape[0] for a in arrs)
        if self.shape != shape:
            self._alloc(shape)
        # The reference re-uploads every iteration.  Here an array is uploaded only when it changed: the same
        # object with the same sampled values is taken as unchanged (in-place edits that keep first / middle /
        # last are not seen); a new object is compared in full with a private copy of what was uploaded last.
        srcs = [input[k] for k in keys] + [label[self.label_key]]
        vals = arrs + [lab.reshape(-1)]
        dsts = list(self.x) + [self.label]
        for j, (src, val, dst) in enumerate(zip(srcs, vals, dsts)):
            fp = _fp(src)
            if fp == self._last_ids[j]:
                continue
            self._last_ids[j] = fp
            val = np.ascontiguousarray(val)
            old = self._uploaded[j]
            if old is not None and old.shape == val.shape and np.array_equal(old, val):
                continue
            self._uploaded[j] = val.copy()
            dst.copy_(torch.from_numpy(val))
        total_global = gshape[0] * gshape[1] * gshape[2]
        self.desc.scale = float(self.scale_fn(total_global)) * rep

    def forward(self, train: bool, reduce_loss: bool = True):
        """reduce_loss=False: the per-workgroup loss rows stay in `lpart`; the caller sums them (SpinnEngine: together with the
        gradient rows, one launch)."""
        m, lib = self.model, L.lib()
        vp = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])  # noqa: E731
        L.check(lib.ppsci_modmlp_fwd_batch(C.byref(m.spec.desc), 3, vp([m.branch(b) for b in range(3)]),
                                           (C.c_int64 * 3)(*[t.numel() for t in self.x]), vp(self.x), vp(self.F),
                                           vp(self.stash) if train else None, _stream_ptr(self.x[0])))
        L.check(lib.ppsci_spinn_grid_fwd(C.byref(self.desc), _p(self.F[0]), _p(self.F[1]), _p(self.F[2]), _p(self.label), None,
                                         _p(self.gadj) if train else None, _p(self.lpart), _stream_ptr(self.label)))
        if reduce_loss:
            hp.reduce_rows(self.lpart, self.lrows, 1, self.loss_term, False)

    def backward(self):
        m, lib = self.model, L.lib()
        vp = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])  # noqa: E731
        if (os.environ.get("PPSCI_SPINN_PARTS", "0") == "1"
                and lib.ppsci_modmlp_bwd_parts_supported(C.byref(m.spec.desc), C.byref(self.desc))):
            # the grid kernel leaves its per-group partials of dL/dF in the scratch; the branch nets' tile kernel sums them on load.
            # OFF by default -- measured on MI355X (128^3, 3 x 128 points): 0.0983 ms per step with it, 0.0914 without: the 24
            # tile workgroups read 128 KB of partials each in front of their latency chain, which costs more than the ~5 us launch
            # of spinn_fbar_sum_kernel (384 workgroups) it saves.  Kept as a tested option for larger point counts.
            L.check(lib.ppsci_spinn_grid_bwd(C.byref(self.desc), _p(self.F[0]), _p(self.F[1]), _p(self.F[2]), _p(self.gadj),
                                             _p(self.bscratch), None, None, None, _stream_ptr(self.gadj)))
            L.check(lib.ppsci_modmlp_bwd_batch_parts(C.byref(m.spec.desc), C.byref(self.desc), vp([m.branch(b) for b in range(3)]),
                                                     vp(self.x), _p(self.bscratch), vp(self.stash), vp(self.gpart),
                                                     3 * m.branch_params if self.gjoint else 0, _stream_ptr(self.x[0])))
            return
        L.check(lib.ppsci_spinn_grid_bwd(C.byref(self.desc), _p(self.F[0]), _p(self.F[1]), _p(self.F[2]), _p(self.gadj),
                                         _p(self.bscratch), _p(self.Fbar[0]), _p(self.Fbar[1]), _p(self.Fbar[2]),
                                         _stream_ptr(self.gadj)))
        L.check(lib.ppsci_modmlp_bwd_batch(C.byref(m.spec.desc), 3, vp([m.branch(b) for b in range(3)]),
                                           (C.c_int64 * 3)(*[t.numel() for t in self.x]), vp(self.x), vp(self.Fbar),
                                           vp(self.stash), vp(self.gpart), 3 * m.branch_params if self.gjoint else 0,
                                           _stream_ptr(self.x[0])))

    def loss(self) -> float:
        return float(self.loss_term.cpu()[0])


class SpinnJetConstraint:
    """A constraint whose residuals are NOT a linear form of {u, u_xx, u_yy, u_zz}: per step
      3 x modmlp_fwd  ->  spinn_jet_fwd (the derivative streams the program reads, as rows U[nq][nx*ny*nz])
                      ->  ppsci_epilogue over the grid points (residual program, loss terms, adjoint rows Ubar)
                      ->  spinn_jet_bwd  ->  3 x modmlp_bwd.
    `low` is the graph.Lowered of the traced expressions (graph.lower with the arch.spinn.JetTable `jet` as its stream choice).
    Same attributes as SpinnConstraint, so that SpinnEngine and the solver treat both alike; `lpart` has one column per loss
    key and `loss_term` one entry per key."""

    def __init__(self, name: str, model, low, jet, label_keys: Sequence[str], scale_fns, device, world: int = 1, rank: int = 0):
        self.name, self.model, self.low, self.jet = name, model, low, jet
        self.label_keys = list(label_keys)
        self.label_key = self.label_keys[0] if self.label_keys else None
        self.scale_fns = list(scale_fns)  # per loss term: total_points -> loss scale
        self.device, self.world, self.rank = device, world, rank
        self.program = low.program
        if not jet.orders:
            raise NotImplementedError(f"constraint {name}: the expressions do not read the network")
        # what each aux row of the program is: ("label" | "weight", key)
        self.aux_src = []
        for a in low.aux_names:
            if a.startswith(LABEL_PREFIX):
                self.aux_src.append(("label", a[len(LABEL_PREFIX):]))
            elif a.startswith(WEIGHT_PREFIX):
                self.aux_src.append(("weight", a[len(WEIGHT_PREFIX):]))
            else:
                raise NotImplementedError(f"constraint {name}: the expression reads {a!r}, which is neither an input axis of the "
                                          "SPINN nor a label / weight grid")
        self.in_used = sorted({a for op, a, _, _ in self.program.instrs if op == L.OP_LD_IN})
        self.shape = None
        self._version = 0
        self._scales = None
        self.edesc = None

    step_obj = property(lambda self: self)

    @property
    def lcols(self) -> int:
        return len(self.program.res)

    @property
    def scale_key(self):
        return self._scales

    def _alloc(self, shape):
        m, dev = self.model, self.device
        self.shape = tuple(shape)
        self._version += 1
        self._last_ids, self._uploaded = {}, {}
        R = m.spec.R
        f32 = dict(dtype=torch.float32, device=dev)
        total = shape[0] * shape[1] * shape[2]
        nq = len(self.jet.orders)
        _alloc_branches(self, shape)
        self.jdesc = L.SpinnJetDesc()
        self.jdesc.n[0], self.jdesc.n[1], self.jdesc.n[2] = shape
        self.jdesc.rank, self.jdesc.nq = R, nq
        for q, t in enumerate(self.jet.orders):
            for a in range(3):
                self.jdesc.ord[q][a] = t[a]
        self.U = torch.zeros((nq, total), **f32)
        self.Ubar = torch.zeros((nq, total), **f32)
        # the inputs the program loads, expanded to the grid; the others are never read (any valid pointer)
        self.xgrid = {j: torch.zeros(total, **f32) for j in self.in_used}
        self.aux = [torch.zeros(total, **f32) for _ in self.aux_src]
        self.lrows = hp.epilogue_partial_rows(total)
        self.lpart = torch.zeros((self.lrows, max(1, self.lcols)), **f32)
        self.loss_term = torch.zeros(max(1, self.lcols), **f32)
        self.resid = None  # [n_res][total], allocated by predict-style use (values())
        self.bscratch = torch.zeros(max(4, int(L.lib().ppsci_spinn_jet_scratch_floats(C.byref(self.jdesc)))), **f32)

    @staticmethod
    def _grid_array(a, gshape, what):
        """A label / weight as a grid: an [nx,ny,nz(,1)] array or a scalar."""
        a = np.asarray(a, dtype=np.float32)
        if a.size == 1:
            return np.broadcast_to(a.reshape(()), gshape)
        if a.size != gshape[0] * gshape[1] * gshape[2]:
            raise ValueError(f"{what}: {a.shape} is neither a scalar nor a grid of {gshape} points")
        return a.reshape(gshape)

    def bind(self, input: Dict[str, np.ndarray], label: Dict[str, np.ndarray], weight: Optional[Dict[str, np.ndarray]] = None):
        keys = self.model.input_keys
        arrs = [np.asarray(input[k], dtype=np.float32).reshape(-1) for k in keys]
        gshape = tuple(a.shape[0] for a in arrs)
        srcs = {"label": label or {}, "weight": weight or {}}
        grids = []
        for kind, k in self.aux_src:
            if k not in srcs[kind]:
                raise KeyError(f"constraint {self.name}: no {kind} for {k!r}")
            grids.append(self._grid_array(srcs[kind][k], gshape, f"{kind} {k!r}"))
        rep = 1.0
        if self.world > 1:  # the rank-strided slab rule of SpinnConstraint.bind, applied to the label AND weight grids
            ax = next((i for i, n in enumerate(gshape) if n >= self.world), None)
            if ax is None:
                rep = 1.0 / self.world
            else:
                arrs[ax] = arrs[ax][self.rank::self.world]
                idx = [slice(None)] * 3
                idx[ax] = slice(self.rank, None, self.world)
                grids = [g[tuple(idx)] for g in grids]
        shape = tuple(a.shape[0] for a in arrs)
        if self.shape != shape:
            self._alloc(shape)

        def upload(slot, src, make, dst):
            """`make()` -> `dst` unless `src` is unchanged since the last upload into `slot` (SpinnConstraint.bind's rule)."""
            fp = _fp(src)
            if fp == self._last_ids.get(slot):
                return False
            self._last_ids[slot] = fp
            val = np.ascontiguousarray(make(), dtype=np.float32).reshape(-1)
            old = self._uploaded.get(slot)
            if old is not None and old.shape == val.shape and np.array_equal(old, val):
                return False
            self._uploaded[slot] = val.copy()
            dst.copy_(torch.from_numpy(val))
            return True

        for j, k in enumerate(keys):
            if upload(("x", j), input[k], lambda j=j: arrs[j], self.x[j]) or ("g", j) not in self._last_ids:
                if j in self.xgrid:  # coordinate j as a value of the program: once per bind of new coordinates
                    self._last_ids[("g", j)] = True
                    view = [1, 1, 1]
                    view[j] = shape[j]
                    self.xgrid[j].copy_(self.x[j].view(*view).expand(*shape).reshape(-1))
        for i, ((kind, k), g) in enumerate(zip(self.aux_src, grids)):
            upload(("aux", i), srcs[kind][k], lambda g=g: g, self.aux[i])
        total_global = gshape[0] * gshape[1] * gshape[2]
        scales = tuple(float(f(total_global)) * rep for f in self.scale_fns)
        if scales != self._scales or self.edesc is None:
            self._scales = scales
            res = self.program.res
            for k, sc in enumerate(scales):
                res[k] = res[k][:4] + (sc,) + res[k][5:]
            self.edesc = self.program.build()

    def _epilogue_args(self):
        return [self.xgrid.get(j, self.x[0]) for j in range(len(self.model.input_keys))]

    def forward(self, train: bool, reduce_loss: bool = True, want_resid: bool = False):
        m, lib = self.model, L.lib()
        vp = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])  # noqa: E731
        st = _stream_ptr(self.x[0])
        L.check(lib.ppsci_modmlp_fwd_batch(C.byref(m.spec.desc), 3, vp([m.branch(b) for b in range(3)]),
                                           (C.c_int64 * 3)(*[t.numel() for t in self.x]), vp(self.x), vp(self.F),
                                           vp(self.stash) if train else None, st))
        L.check(lib.ppsci_spinn_jet_fwd(C.byref(self.jdesc), _p(self.F[0]), _p(self.F[1]), _p(self.F[2]), _p(self.U), st))
        if want_resid and self.resid is None:
            self.resid = torch.zeros((max(1, self.lcols), self.U.shape[1]), dtype=torch.float32, device=self.device)
        hp.epilogue(self.edesc, self.U.shape[1], self._epilogue_args(), self.U, self.aux, self.resid if want_resid else None,
                    self.Ubar if train else None, self.lpart)
        if reduce_loss:
            hp.reduce_rows(self.lpart, self.lrows, self.lcols, self.loss_term, False)

    def backward(self):
        m, lib = self.model, L.lib()
        vp = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])  # noqa: E731
        st = _stream_ptr(self.x[0])
        L.check(lib.ppsci_spinn_jet_bwd(C.byref(self.jdesc), _p(self.F[0]), _p(self.F[1]), _p(self.F[2]), _p(self.Ubar),
                                        _p(self.bscratch), _p(self.Fbar[0]), _p(self.Fbar[1]), _p(self.Fbar[2]), st))
        L.check(lib.ppsci_modmlp_bwd_batch(C.byref(m.spec.desc), 3, vp([m.branch(b) for b in range(3)]),
                                           (C.c_int64 * 3)(*[t.numel() for t in self.x]), vp(self.x), vp(self.Fbar),
                                           vp(self.stash), vp(self.gpart), 3 * m.branch_params if self.gjoint else 0, st))

    def losses(self) -> Dict[str, float]:
        t = self.loss_term.cpu()
        return {k: float(t[i]) for i, k in enumerate(self.label_keys)}

    def loss(self) -> float:
        return float(sum(self.losses().values()))

    def values(self) -> Dict[str, torch.Tensor]:
        """The residual rows of the last forward(want_resid=True), as [nx,ny,nz,1] grids per output name."""
        return {k: self.resid[i].view(*self.shape, 1) for i, k in enumerate(self.low.loss_keys)}


def jet_constraint(name, model, vals, label_keys, weight_keys, loss, device, world=1, rank=0, extra_outputs=()):
    """Lowers traced SPINN expressions with graph.lower (the program builder of every other model) on a stream table of
    per-axis derivative orders."""
    if len(label_keys) + len(extra_outputs) > L.MAX_RES:
        raise NotImplementedError(f"constraint {name}: {len(label_keys) + len(extra_outputs)} expression keys; one epilogue "
                                  f"program holds {L.MAX_RES} (PPSCI_MAX_RES)")
    if weight_keys and hasattr(loss, "batch_weight"):
        raise NotImplementedError(f"constraint {name}: {type(loss).__name__} with weight grids on a SPINN grid: the reference "
                                  "broadcasts its per-sample errors against the weight column of a batch, which a grid has not")
    outputs = {}
    for k, v in vals.items():
        v = v._as_sym() if hasattr(v, "_as_sym") else v
        outputs[k] = v if isinstance(v, graph.Sym) else graph._lift(v)
    losses = loss_terms(label_keys, weight_keys, loss, 0, scale=1.0)  # (the scales are set per bind: scale_fns)
    jet = JetTable(model)
    try:
        low = graph.lower(outputs, losses, extra_outputs, jet=jet)
    except NotImplementedError as e:
        raise NotImplementedError(f"constraint {name}: {e}") from None
    return SpinnJetConstraint(name, model, low, jet, label_keys, [(lambda total, k=k: loss.term_scale(k, total)) for k in label_keys],
                              device, world, rank)


class SpinnEngine:
    per_key_pass = False

    def __init__(self, model):
        self._predict_cache: Dict[int, tuple] = {}
        self.model = model
        self.grad = torch.zeros_like(model.flat_params)
        self.world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
        self.dp_reduce = "sum"
        self._step_graph = StepGraph(self.grad.is_cuda and os.environ.get("PPSCI_HIP_GRAPH", "1") != "0")
        self.multi_stream = os.environ.get("PPSCI_MULTI_STREAM", "1") != "0"
        self._streams: list = []

    def _segments(self, constraints: Sequence[SpinnConstraint]):
        """The row reductions that end the step of ONE constraint, as (source, destination, rows, cols) pointers: the loss
        rows and the gradient rows of the three branch nets."""
        P = self.model.branch_params
        c0 = constraints[0]
        segs = [(c0.lpart.data_ptr(), c0.loss_term.data_ptr(), c0.lrows, c0.lcols)]
        if c0.gjoint:
            segs.append((c0.gpart_all.data_ptr(), self.grad.data_ptr(), c0.gpart_all.shape[0], 3 * P))
        else:
            segs += [(c0.gpart[b].data_ptr(), self.grad[b * P:(b + 1) * P].data_ptr(), c0.gpart[b].shape[0], P) for b in range(3)]
        return segs

    def forward_backward_deferred(self, constraints: Sequence[SpinnConstraint]):
        """forward_backward WITHOUT the reduction launch behind it, for a caller that sums the rows and applies Adam in one
        launch (hp.reduce_rows_multi_adam; solver.Solver._reduce_and_adam_in_one_launch): returns the pending reductions.
        None: several constraints share the gradient (their rows accumulate: the reductions stay separate launches) -- the
        step was run in full."""
        if len(constraints) != 1:
            self.forward_backward(constraints)
            return None
        key = tuple((id(c), c._version, c.scale_key) for c in constraints) + ("deferred",)
        self._step_graph.run(key, lambda: self._forward_backward_eager(constraints, reduce=False))
        return self._segments(constraints)

    def flush_deferred(self, segs) -> None:
        hp.reduce_rows_multi(segs, self.grad)

    def _forward_backward_eager(self, constraints: Sequence[SpinnConstraint], reduce: bool = True):
        P = self.model.branch_params
        if self.multi_stream and len(constraints) > 1 and self.grad.is_cuda:
            # the PDE grid and the six boundary faces are independent until their gradients are summed
            run_on_streams(self._streams, [(lambda c=c: (c.forward(True, False), c.backward())) for c in constraints])
        else:
            for c in constraints:
                c.forward(True, False)
                c.backward()
        if not reduce:
            return
        # ONE launch (ppsci_reduce_rows_multi) sums every constraint's loss rows and the FIRST constraint's gradient rows -- segments
        # with different destinations; the other constraints' gradient rows are added behind it, one launch each, in order (they
        # share a destination).  Helmholtz3D's single PDE constraint: two launches (this one + Adam) instead of three.
        segs = [(c.lpart, c.loss_term, c.lrows, c.lcols) for c in constraints]
        c0 = constraints[0]
        if c0.gjoint:
            segs.append((c0.gpart_all, self.grad[:3 * P], c0.gpart_all.shape[0], 3 * P))
        else:
            segs += [(c0.gpart[b], self.grad[b * P:(b + 1) * P], c0.gpart[b].shape[0], P) for b in range(3)]
        hp.reduce_rows_multi([(src.data_ptr(), dst.data_ptr(), rows, cols) for src, dst, rows, cols in segs], self.grad)
        for c in constraints[1:]:
            if c.gjoint:
                hp.reduce_rows(c.gpart_all, c.gpart_all.shape[0], 3 * P, self.grad[:3 * P], True)
                continue
            for b in range(3):
                hp.reduce_rows(c.gpart[b], c.gpart[b].shape[0], P, self.grad[b * P:(b + 1) * P], True)

    def forward_backward(self, constraints: Sequence[SpinnConstraint]):
        # A step is ~12 launches per constraint of a few microseconds each (seven constraints in the reference's
        # Helmholtz3D example): launch-bound from Python, so the whole sequence is one replayed HIP graph.  The
        # residual scale and the grid shape are captured by value, hence part of the key.
        key = tuple((id(c), c._version, c.scale_key) for c in constraints)
        self._step_graph.run(key, lambda: self._forward_backward_eager(constraints))

    def invalidate_graphs(self) -> None:
        self._step_graph.clear()

    def allreduce(self, buf: Optional[torch.Tensor] = None):
        if self.world > 1:
            torch.distributed.all_reduce(self.grad if buf is None else buf, op=torch.distributed.ReduceOp.SUM)


    def compile_constraint(self, name: str, cst, device, world: int = 1, rank: int = 0):
        """A user constraint on a separable net.  One residual that is a linear form of {u, u_xx, u_yy, u_zz} without weights keeps
        the four-coefficient grid kernels (arch.spinn.GridLinear -> SpinnConstraint); everything else -- several keys, weight grids,
        non-linear residuals, first and mixed derivatives -- is lowered to an epilogue program over the derivative streams it
        reads (SpinnJetConstraint).  PPSCI_SPINN_JET=1 sends a linear form down the general path too (A/B timing, tests)."""
        model = self.model
        ds = getattr(cst.data_loader, "dataset", cst.data_loader)
        label_keys = list(ds.label_keys)
        if hasattr(ds, "weight_fn"):  # ContinuousNamedArrayDataset
            w0 = ds.weight_fn(ds.input_fn()) if callable(ds.weight_fn) else None
            weight_keys = list(w0.keys()) if w0 else []
        else:
            weight_keys = list((getattr(ds, "weight", None) or {}).keys())
        data = {k: graph.Sym.input(k) for k in model.input_keys}
        data.update(model(data))
        vals = {k: (cst.output_expr[k](data) if k in cst.output_expr else data[k]) for k in label_keys}
        autodiff.clear()
        loss = cst.loss
        key = label_keys[0] if label_keys else None
        linear = (len(label_keys) == 1 and not weight_keys and isinstance(vals[key], GridLinear)
                  and getattr(loss, "term_kind", 0) == 0 and os.environ.get("PPSCI_SPINN_JET", "0") != "1")
        if linear:
            sc = SpinnConstraint(name, model, vals[key].c, key, lambda total, k=key: loss.term_scale(k, total), device, world, rank)
        else:
            sc = jet_constraint(name, model, vals, label_keys, weight_keys, loss, device, world, rank)
        sc.batch_size = 0
        sc.label_keys = label_keys
        return sc

    def predict(self, input_dict, expr_dict, batch_size, return_numpy: bool, device):
        """The model on the tensor-product grid of the coordinate vectors (helmholtz3d.py:205-213; every rank: the grid it is given)
        and `expr_dict` on the same grid through the general path (forward sweep, stream contraction, the epilogue's residual
        rows, no adjoint), as [nx,ny,nz,1] arrays next to the model outputs."""
        out = self.model(input_dict)
        if expr_dict is not None:
            ck = id(expr_dict)
            if ck not in self._predict_cache:
                data = {k: graph.Sym.input(k) for k in self.model.input_keys}
                data.update(self.model(data))
                vals = {k: f(data) for k, f in expr_dict.items()}
                autodiff.clear()
                # (the dict is kept with its constraint: its id stays unique for as long as the cache entry lives)
                self._predict_cache[ck] = (jet_constraint("predict", self.model, vals, [], [], None, device,
                                                          extra_outputs=tuple(expr_dict)), expr_dict)
            cc = self._predict_cache[ck][0]
            cc.bind({k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in input_dict.items()}, {})
            cc.forward(False, False, want_resid=True)
            out = dict(out, **{k: v.clone() for k, v in cc.values().items()})
        return {k: v.detach().cpu().numpy() for k, v in out.items()} if return_numpy else out
