"""ppsci.equation.Helmholtz (/root/reference/ppsci/equation/pde/helmholtz.py:44-95): k^2 u + u_xx + u_yy + u_zz
on a separable net.  The reference obtains each u_ii with `hvp_revrev` -- two nested
`paddle.incubate.autograd.jvp` through `model.forward_tensor` with unit tangents (:27-41, :86-88); here the
same quantity is the second-derivative stream of the corresponding branch net (SPINN.second_derivative)."""
from typing import Callable, Dict, Optional, Tuple

from ...autodiff import jvp
from .base import PDE


def hvp_revrev(f: Callable, primals: Tuple[object, ...]):
    """helmholtz.py:27-41: the second derivative of f along the primals as two nested jvp calls (unit tangents).  On traced
    inputs, e.g. hvp_revrev(lambda x_: model.forward_tensor(x_, y, z), (x,)) is u_xx of a SPINN on its grid."""
    g = lambda primals: jvp(f, primals)[1]  # noqa: E731
    tangents_out = jvp(g, primals)[1]
    return tangents_out[0]


class Helmholtz(PDE):
    def __init__(self, dim: int, k: float, detach_keys: Optional[Tuple[str, ...]] = None):
        super().__init__()
        self.dim, self.k, self.detach_keys = dim, k, detach_keys
        self.model = None  # set by the user script (examples/spinn/helmholtz3d.py:122)

        def helmholtz(data_dict: Dict[str, object]):
            u = data_dict["u"]
            keys = ("x", "y", "z")[: self.dim]
            out = (self.k**2) * u
            for key in keys:
                out = out + self.model.second_derivative(key)
            return out

        self.add_equation("helmholtz", helmholtz)
        self._apply_detach()
