"""ppsci.arch.LNO, the Laplace neural operator of /root/reference/ppsci/arch/lno.py, on this framework's kernels.

Like arch/fno.py the class holds PARAMETERS only, in the reference's module tree and under its names: `fc0`, `laplace`
(complex residues `weights_residue_real / _imag` [C, C, m1, m2, m3, 1], complex poles per axis `weights_pole_real / _imag[d]`
[C, C, m_d, 1], the grids `t_d` and `lambda_d = 2 pi i fftfreq(n_d, dt_d)` as buffers), `conv` (1x1x1, C -> C), `fc1`, `fc2`.
Forward and backward run in `lno_engine.LnoNative` on the kernels of csrc/lno.inc; nothing of the network is on an autograd tape.

What the reference's forward does (lno.py:280-300), for reading the executor against:

    h  = fc0(x [+ grid channels])                    channel-last -> [B, C, n1, n2, n3]
    x1 = norm(laplace(norm(h)))                       use_norm=False: laplace(h); norm = InstanceNorm3D without affine
    y  = fc2(act(fc1(x1 + conv(h))))                  one output feature per grid point

Input `[B, n1, n2, n3, in_features]`, output `[B, n1, n2, n3, 1]`."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import activation as act_mod
from .operator_base import OperatorArch

# the activations of arch/activation.py that lno_head_* evaluates (no trainable activation parameters in the head kernel)
HEAD_ACTIVATIONS = ("tanh", "silu", "sin", "cos", "sigmoid", "gelu", "relu", "leaky_relu", "elu", "selu", "identity")


class _Linear(torch.nn.Module):
    """Parameters of nn.Linear in the reference's layout: weight [in, out], bias [out]; U(+-1/sqrt(in)) like arch/fno.Conv1x1."""

    def __init__(self, fin: int, fout: int):
        super().__init__()
        k = 1.0 / math.sqrt(fin)
        self.weight = torch.nn.Parameter((torch.rand(fin, fout) * 2 - 1) * k)
        self.bias = torch.nn.Parameter((torch.rand(fout) * 2 - 1) * k)


class _Conv1(torch.nn.Module):
    """Parameters of nn.Conv3D(C, C, kernel_size=1): weight [out, in, 1, 1, 1], bias [out]."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        k = 1.0 / math.sqrt(cin)
        self.weight = torch.nn.Parameter((torch.rand(cout, cin, 1, 1, 1) * 2 - 1) * k)
        self.bias = torch.nn.Parameter((torch.rand(cout) * 2 - 1) * k)


def _grid(v, name: str) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64))
    if t.ndim != 2 or t.shape[0] != 1 or t.shape[1] < 2:
        raise ValueError(f"LNO: {name} must have shape [1, n] with n >= 2, got {tuple(t.shape)}")
    return t


class Laplace(torch.nn.Module):
    """Parameters and buffers of lno.py:31-93 (pole-residue transfer function); residues and poles U(0, 1 / C^2)."""

    def __init__(self, in_channels: int, out_channels: int, modes: Tuple[int, ...], T, data):
        super().__init__()
        from ..utils import initializer

        self.modes, self.dims = tuple(modes), len(modes)
        self.scale = 1 / (in_channels * out_channels)

        def new(shape):
            return torch.nn.Parameter(initializer.uniform_(torch.empty(shape), 0, self.scale))

        shape = (in_channels, out_channels) + self.modes + (1,)
        # (the residues are assigned after the pole lists in the reference, but as plain attributes they precede the
        # sublayers' parameters in named_parameters(): the order tests/golden/lno.npz records)
        self.weights_residue_real = new(shape)
        self.weights_residue_imag = new(shape)
        pr, pi = [], []
        for d in range(self.dims):
            pr.append(new((in_channels, out_channels, self.modes[d], 1)))
            pi.append(new((in_channels, out_channels, self.modes[d], 1)))
        for d, g in enumerate((T,) + tuple(data)):
            g = _grid(g, f"grid {d}")
            dt = float(g[0, 1] - g[0, 0])
            omega = np.fft.fftfreq(g.shape[1], dt) * 2 * np.pi
            self.register_buffer(f"t_{d}", g.to(torch.float32))
            self.register_buffer(f"lambda_{d}", torch.complex(torch.zeros(len(omega)), torch.tensor(omega, dtype=torch.float32))
                                 .reshape(-1, 1, 1, 1))
        self.weights_pole_real = torch.nn.ParameterList(pr)
        self.weights_pole_imag = torch.nn.ParameterList(pi)


class LNO(OperatorArch):
    """ppsci.arch.LNO (lno.py:190-313); constructor arguments in the reference's order.  `forward_tensor`:
    [B, n1, n2, n3, data channels] -> [B, n1, n2, n3, 1]."""

    _executor = "lno_engine.LnoNative"
    channel_axis = -1  # input keys are concatenated along the LAST axis (channel-last fields)

    def __init__(self, input_keys: Tuple[str, ...], output_keys: Tuple[str, ...], width: int, modes: Tuple[int, ...], T,
                 data: Optional[Tuple] = None, in_features: int = 1, hidden_features: int = 64, activation: str = "sin",
                 use_norm: bool = True, use_grid: bool = False):
        OperatorArch.__init__(self)
        self.input_keys, self.output_keys = tuple(input_keys), tuple(output_keys)
        self.width, self.modes, self.dims = int(width), tuple(int(v) for v in modes), len(modes)
        assert self.dims <= 3, "Only 3 dims and lower of modes are supported now."
        data = () if data is None else tuple(data)
        assert self.dims == len(data) + 1, f"Dims of modes is {self.dims} but only {len(data)} dims(except T) of data received."
        if self.dims != 3:
            raise NotImplementedError(f"LNO with {self.dims} mode axes: the reference's own forward only runs for three (it "
                                      "transforms over axes [-3, -2, -1] and get_grid unpacks four sizes); the kernels are 3-D")
        if len(self.output_keys) != 1:
            raise NotImplementedError("LNO with more than one output key: fc2 has one output feature")
        act = act_mod.get_activation(activation)
        if act not in HEAD_ACTIVATIONS:
            raise NotImplementedError(f"LNO(activation={activation!r}): the head kernel carries no trainable activation "
                                      f"parameters (built: {HEAD_ACTIVATIONS})")
        self.activation = act
        self.in_features, self.hidden_features = int(in_features), int(hidden_features)
        self.use_norm, self.use_grid = bool(use_norm), bool(use_grid)
        if self.use_grid and self.in_features <= 3:
            raise ValueError("LNO(use_grid=True): in_features counts the three grid channels and at least one data channel")
        self.norm_eps = 1e-5  # nn.InstanceNorm3D's default
        self.fc0 = _Linear(self.in_features, self.width)
        self.laplace = Laplace(self.width, self.width, self.modes, T, data)
        self.conv = _Conv1(self.width, self.width)
        self.fc1 = _Linear(self.width, self.hidden_features)
        self.fc2 = _Linear(self.hidden_features, 1)
        from ..device import get_device

        self.to_device(get_device())
