"""ppsci.equation.fpde (/root/reference/ppsci/equation/fpde/__init__.py)."""
from .fractional_poisson import FractionalPoisson  # noqa: F401

__all__ = ["FractionalPoisson"]
