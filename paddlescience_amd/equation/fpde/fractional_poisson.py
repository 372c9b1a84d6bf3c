"""ppsci.equation.FractionalPoisson (/root/reference/ppsci/equation/fpde/fractional_poisson.py:30-196): the fractional Poisson
problem  (-Δ)^(α/2) u = f  on the unit disk (fPINN, the Grünwald–Letnikov discretisation of the directional fractional
derivatives, integrated over the directions with Gauss–Legendre quadrature).

The batch of the constraint is  [the N collocation points | the auxiliary points of point 1 | ... | of point N]  (the
example's dataset transform builds it with `get_x`, examples/fpde/fractional_poisson_2d.py:86-113): along each of the
`resolution[0]` Gauss directions, the points from x_i backwards to the boundary in steps of about 1 / resolution[-1], shifted
by one step (first order).  Residual i < N is
    c (M u)_i - 2^α Γ(2 + α/2) Γ(1 + α/2) (1 - (1 + α/2) |x_i|²),    c = Γ((1-α)/2) Γ((2+α)/2) / (2 π^1.5),
with a constant [N, N + A] matrix M whose row i holds the Grünwald–Letnikov weights of point i's own auxiliary points: ~690
nonzeros per row at resolution [8, 100], one per auxiliary column.  It is traced as a sparse graph.couple (CSR products on
the device, engine.FusedConstraint._forward_couplings) -- dense, M would take 11 GB at N = 2000."""
from __future__ import annotations

import math
import zlib
from typing import Tuple

import numpy as np

from ...utils import misc
from ..pde.base import PDE


class FractionalPoisson(PDE):
    dtype = "float32"

    def __init__(self, alpha: float, geom, resolution: Tuple[int, ...]):
        super().__init__()
        from ...geometry import Disk

        if not isinstance(geom, Disk):
            # the reference's 1-D branch and its 3-D branch (which needs a sphere geometry) are not built here
            raise NotImplementedError(f"FractionalPoisson is built for a 2-D Disk; got {type(geom).__name__} (the 1-D and 3-D "
                                      "directions of the reference are not implemented)")
        self.alpha = alpha
        self.geom = geom
        self.resolution = resolution
        self._w_init = self._init_weights()

        def compute_fpde_func(out):
            from ... import graph

            x, y, u = out["x"], out["y"], out["u"]
            a = self.alpha
            c = self._factor()
            k = 2 ** a * math.gamma(2 + a / 2) * math.gamma(1 + a / 2)
            if isinstance(x, graph.Sym):
                self._check_batch(graph.concrete_values(x, "FractionalPoisson's auxiliary points"),
                                  graph.concrete_values(y, "FractionalPoisson's auxiliary points"))
                graph._TRACE.concretized.append(f"fractional_poisson_matrix({x!r}, {y!r}) crc {self.int_mat.crc():08x}")
                rhs = k * (1 - (1 + a / 2) * (x ** 2 + y ** 2))
                # c (M u) - rhs  as  lhs - factor (M u)  with lhs = -rhs, factor = -c (the same float32 result: rounding is
                # symmetric in the sign)
                return graph.couple(-rhs, self.int_mat, u, factor=-c)
            # real tensors / arrays (evaluating the equation outside a compiled constraint): the reference's value, [N]
            n = len(self.x0)
            rows = self.int_mat.row_of_entries()
            import torch

            if isinstance(u, torch.Tensor):
                vals = torch.as_tensor(self.int_mat.vals, device=u.device).to(u.dtype)
                cols = torch.as_tensor(self.int_mat.col_idx.astype(np.int64), device=u.device)
                lhs = torch.zeros(n, dtype=u.dtype, device=u.device).index_add_(
                    0, torch.as_tensor(rows, device=u.device), vals * u[:, 0][cols])
                xx, yy = x[:n, 0], y[:n, 0]
            else:
                u = np.asarray(u, dtype=np.float32).reshape(-1)
                lhs = np.bincount(rows, weights=self.int_mat.vals.astype(np.float64) * u[self.int_mat.col_idx],
                                  minlength=n).astype(np.float32)
                xx, yy = np.asarray(x).reshape(-1)[:n], np.asarray(y).reshape(-1)[:n]
            lhs = lhs * c
            return lhs - k * (1 - (1 + a / 2) * (xx ** 2 + yy ** 2))

        self.add_equation("fpde", compute_fpde_func)

    def _factor(self) -> float:
        a = self.alpha
        return math.gamma((1 - a) / 2) * math.gamma((2 + a) / 2) / (2 * np.pi ** 1.5)

    def _init_weights(self) -> np.ndarray:
        """Grünwald–Letnikov weights w_j = w_{j-1} (j - 1 - α) / j, w_0 = 1, for as many steps as the diameter can take."""
        n = self._dynamic_dist2npts(self.geom.diam) + 1
        w = [1.0]
        for j in range(1, n):
            w.append(w[-1] * (j - 1 - self.alpha) / j)
        return np.array(w, dtype=self.dtype)

    def get_x(self, x_f):
        """[points | their auxiliary points] as {"x", "y"} columns; computed once, the cached batch returned afterwards."""
        if hasattr(self, "train_x"):
            return self.train_x
        self.x0 = x_f
        if np.any(self.geom.on_boundary(self.x0)):
            raise ValueError("x0 contains boundary points.")
        gauss_x, gauss_w = np.polynomial.legendre.leggauss(self.resolution[0])
        gauss_x, gauss_w = gauss_x.astype(self.dtype), gauss_w.astype(self.dtype)
        thetas = np.pi * gauss_x + np.pi
        dirns = np.vstack((np.cos(thetas), np.sin(thetas))).T
        dirn_w = np.pi * gauss_w
        aux, self.w = [], []
        for x0i in self.x0:
            xs, ws = [], []
            for dirn, dw in zip(dirns, dirn_w):
                pts = self.background_points(x0i, dirn, self._dynamic_dist2npts, 0)
                wts = dw * np.linalg.norm(pts[1] - pts[0]) ** (-self.alpha) * self.get_weight(len(pts) - 1)
                pts, wts = self.modify_first_order(pts, wts)
                xs.append(pts)
                ws.append(wts)
            aux.append(np.vstack(xs))
            self.w.append(np.hstack(ws))
        self.x = np.vstack([self.x0] + aux)
        self.int_mat = self._get_int_matrix(self.x0)
        self.train_x = misc.convert_to_dict(self.x, ("x", "y"))
        self._batch_crc = (len(self.x), _crc(self.train_x["x"]), _crc(self.train_x["y"]))
        return self.train_x

    def get_weight(self, n: int) -> np.ndarray:
        return self._w_init[: n + 1]

    def background_points(self, x, dirn, dist2npt, shift):
        """x, x - h d, x - 2 h d, ... to the boundary along -d: n = max(dist2npt(distance), 1) steps of equal length h."""
        dirn = dirn / np.linalg.norm(dirn)
        dx = self.distance2boundary_unitdirn(x, -dirn)
        n = max(dist2npt(dx), 1)
        h = dx / n
        return x - np.arange(-shift, n - shift + 1, dtype=self.dtype)[:, None] * h * dirn

    def distance2boundary_unitdirn(self, x, dirn):
        """Distance from x (inside) to the circle along the unit direction: the positive root of the line-circle intersection."""
        xc = x - self.geom.center
        ad = np.dot(xc, dirn)
        return (-ad + (ad ** 2 - np.sum(xc * xc, axis=-1) + self.geom.radius ** 2) ** 0.5).astype(self.dtype)

    def modify_first_order(self, x, w):
        """Shift the nodes one step forward (x + h d first, the boundary node dropped); without the first node when it falls
        outside the domain."""
        x = np.vstack(([2 * x[0] - x[1]], x[:-1]))
        if not self.geom.is_inside(x[0:1])[0]:
            return x[1:], w[1:]
        return x, w

    def _dynamic_dist2npts(self, dx) -> int:
        return int(math.ceil(self.resolution[-1] * dx))

    def _get_int_matrix(self, x: np.ndarray):
        """Row i: the weights of point i's auxiliary points, at their consecutive columns behind the N collocation points."""
        from ...graph import CsrMatrix

        n = x.shape[0]
        counts = np.array([len(wi) for wi in self.w], dtype=np.int64)
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(counts, out=ptr[1:])
        vals = np.hstack([np.asarray(wi) for wi in self.w]).astype(self.dtype)
        return CsrMatrix(ptr, n + np.arange(ptr[-1], dtype=np.int64), vals, (n, self.x.shape[0]))

    def _check_batch(self, xv, yv) -> None:
        if not hasattr(self, "train_x"):
            raise ValueError("FractionalPoisson: the constraint's batch must be the one get_x() built (get_x was never called)")
        got = (len(np.asarray(xv).reshape(-1)), _crc(np.asarray(xv, np.float32).reshape(-1, 1)),
               _crc(np.asarray(yv, np.float32).reshape(-1, 1)))
        if got != self._batch_crc:
            raise ValueError(f"FractionalPoisson: the constraint's batch ({got[0]} points, crc {got[1]:08x}/{got[2]:08x}) is not "
                             f"the one get_x() built ({self._batch_crc[0]} points, crc "
                             f"{self._batch_crc[1]:08x}/{self._batch_crc[2]:08x})")


def _crc(a: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).tobytes())
