from .ad import clear, hessian, jacobian, jvp  # noqa: F401

__all__ = ["jacobian", "hessian", "jvp", "clear"]
