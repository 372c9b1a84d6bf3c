"""optimizer.fused_adam_args: the one answer to "may a kernel apply this optimizer's step in its own launch?" -- the argument
dict for a plain Adam, None for everything that puts something between the gradient and the update or is no Adam at all."""
import types

import pytest
import torch

from paddlescience_amd import optimizer as O
from paddlescience_amd.optimizer.optimizer import fused_adam_args


class _Net:
    def __init__(self):
        self.flat_params = torch.zeros(6)

    def parameters(self):
        return [self.flat_params[:4], self.flat_params[4:]]


def _with_equation_parameters(net):
    from paddlescience_amd import device
    from paddlescience_amd.equation.pde.base import EqParamStore

    eq = types.SimpleNamespace(learnable_parameters=[object()], equations={})
    device.set_device("cpu")  # the store of the equation parameters is a small tensor on the current device
    try:
        EqParamStore.reset()
        return O.Adam(2e-3)((net, eq))
    finally:
        EqParamStore.reset()
        device.set_device(None)


CLOSED = {
    "adam_grad_clip": lambda net: O.Adam(2e-3, grad_clip=O.ClipGradByNorm(1.0))(net),
    "adam_weight_decay": lambda net: O.Adam(2e-3, weight_decay=1e-4)(net),
    "adam_equation_parameters": _with_equation_parameters,
    "adamw": lambda net: O.AdamW(2e-3)(net),
    "sgd": lambda net: O.SGD(2e-3)(net),
    "momentum": lambda net: O.Momentum(2e-3, 0.9)(net),
    "rmsprop": lambda net: O.RMSProp(2e-3)(net),
    "lbfgs": lambda net: O.LBFGS()(net),
}


def test_plain_adam_gives_the_kernel_arguments():
    opt = O.Adam(2e-3, beta1=0.8, beta2=0.95, epsilon=1e-6)(_Net())
    opt.t = 4
    args = fused_adam_args(opt, 0.5, opt.t + 1)
    assert set(args) == {"m", "v", "lr", "beta1", "beta2", "eps", "grad_scale", "t"}
    assert args["m"] is opt.m and args["v"] is opt.v
    assert (args["lr"], args["beta1"], args["beta2"], args["eps"]) == (opt.get_lr(), opt.beta1, opt.beta2, opt.epsilon)
    assert (args["lr"], args["beta1"], args["beta2"], args["eps"]) == (2e-3, 0.8, 0.95, 1e-6)
    assert args["grad_scale"] == 0.5 and args["t"] == 5 and opt.t == 4


@pytest.mark.parametrize("name", list(CLOSED))
def test_everything_else_is_refused(name):
    opt = CLOSED[name](_Net())
    if name == "adam_equation_parameters":
        assert opt.eq_store is not None
    assert fused_adam_args(opt, 1.0, 1) is None
