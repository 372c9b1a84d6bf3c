"""What the operator models (arch/fno.py, arch/uno.py, arch/lno.py, arch/geofno.py) share: they hold PARAMETERS only, as views
into one flat fp32 buffer, and every forward -- training, eval, predict, validators -- runs in the model's executor
(native_executor.NativeExecutor), the only implementation of the network."""
from __future__ import annotations

import importlib
from typing import Optional

import torch

from . import base


class OperatorArch(base.Arch, torch.nn.Module):
    """The parameters live in ONE flat fp32 buffer (`flat_params`, module parameters are views into it) so that the
    data-parallel all-reduce and the fused Adam kernel act on a single tensor, as for the PINN path.  A subclass builds its
    module tree, names its executor and ends its constructor with `self.to_device(get_device())`."""

    is_operator = True  # Solver: the operator engine (hand-written forward + backward in the executor)
    channel_axis = 1    # the axis the fields of several input keys are concatenated along ([B, C, ...]; -1: channel-last)
    _executor = ""      # "<engine module>.<class>" under paddlescience_amd: imported on first use, not with arch/

    def __init__(self):
        torch.nn.Module.__init__(self)
        base.Arch.__init__(self)
        self.flat_params: Optional[torch.Tensor] = None
        self.flat_grad: Optional[torch.Tensor] = None

    # ---- flat parameter buffer ---------------------------------------------------------------
    def to_device(self, device):
        """Moves the model and (re)packs every parameter as a view into `flat_params` / `flat_grad`."""
        torch.nn.Module.to(self, device)
        self._native = None  # (its buffers live on the old device)
        ps = [p for p in torch.nn.Module.parameters(self)]
        n = sum(p.numel() for p in ps)
        flat = torch.empty(n, dtype=torch.float32, device=device)
        grad = torch.zeros(n, dtype=torch.float32, device=device)
        off = 0
        for p in ps:
            k = p.numel()
            flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = flat[off:off + k].view_as(p.data)
            p.grad = grad[off:off + k].view_as(p.data)
            off += k
        self.flat_params, self.flat_grad = flat, grad
        return self

    def parameters(self, recurse: bool = True):
        return list(torch.nn.Module.parameters(self, recurse))

    def state_dict(self, *args, **kwargs):
        return {k: v.detach().clone() for k, v in torch.nn.Module.state_dict(self, *args, **kwargs).items()}

    def set_state_dict(self, state):
        own = torch.nn.Module.state_dict(self)
        with torch.no_grad():
            for k, v in state.items():
                own[k].copy_(torch.as_tensor(v).to(own[k].device))

    def train(self, mode: bool = True):
        torch.nn.Module.train(self, mode)
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    # ---- forward -----------------------------------------------------------------------------
    def native(self):
        """The kernels' executor for this model (buffers per input shape); shared by training, eval and predict."""
        nat = getattr(self, "_native", None)
        if nat is None:
            module, cls = self._executor.split(".")
            nat = self._native = getattr(importlib.import_module(f"..{module}", __package__), cls)(self)
        return nat

    def forward_tensor(self, x: torch.Tensor) -> torch.Tensor:
        """The network on one input tensor (shapes: the class docstring) -> a fresh tensor; the executor owns its buffers."""
        return self.native().forward(x.to(dtype=torch.float32).contiguous()).clone()

    def forward(self, x):
        if self._input_transform is not None:
            x = self._input_transform(x)
        dev = self.flat_params.device
        xs = [torch.as_tensor(x[k], dtype=torch.float32).to(dev) for k in self.input_keys]
        xt = xs[0] if len(xs) == 1 else torch.cat(xs, dim=self.channel_axis)
        out = {self.output_keys[0]: self.forward_tensor(xt)}
        if self._output_transform is not None:
            out = self._output_transform(x, out)
        return out

    __call__ = torch.nn.Module.__call__
