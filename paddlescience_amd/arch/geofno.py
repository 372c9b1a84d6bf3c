"""ppsci.arch.FNO1d, the 1-D Fourier neural operator of Geo-FNO (/root/reference/ppsci/arch/geofno.py), on this framework's kernels.

Like arch/lno.py the class holds PARAMETERS only, in the reference's module tree and under its names: `fc0` (Linear, weight
[in, C]), `conv0 .. conv4` (SpectralConv1d: `weights1_real / weights1_imag` [C, C, modes]), `w0 .. w3` (Conv1D, weight [C, C, 1]),
`fc1` [C, 128], `fc2` [128, 1].  Forward and backward run in `geofno_engine.Fno1dNative` on the kernels of csrc/fno1d.inc; nothing
of the network is on an autograd tape.

What the reference's forward does (geofno.py:167-205), for reading the executor against:

    x = pad(fc0(x)^T, `padding` zeros on the right)            [B, s, in] -> [B, C, s + padding]
    x = gelu(conv_k(x) + w_k(x))            k = 0 .. 3          conv_k = irfft(first `modes` of rfft(x) times W_k, n = length)
    x = x[..., :-padding]                                      [B, C, s]
    x = conv4(x, output_np) + interpolate(x, output_np)        linear, align_corners=True; no activation
    y = fc2(gelu(fc1(x^T)))                                    [B, output_np, 1]

irfft ignores the imaginary part of the DC coefficient and, for an even length with that mode kept, of the Nyquist coefficient, and
drops coefficients beyond n // 2 + 1; rfft of a length-L signal has L // 2 + 1 coefficients, so `modes` may not exceed that (the
reference fails on its slice assignment there)."""
from __future__ import annotations

import math
from typing import Tuple

import torch

from .operator_base import OperatorArch

HIDDEN = 128  # fc1's output features (geofno.py:153)


class _Linear(torch.nn.Module):
    """Parameters of nn.Linear: weight [in, out], bias [out]; Paddle's defaults (Xavier-uniform weight, zero bias)."""

    def __init__(self, fin: int, fout: int):
        super().__init__()
        from ..utils import initializer

        self.weight = torch.nn.Parameter(initializer.xavier_uniform_(torch.empty(fin, fout), reverse=True))
        self.bias = torch.nn.Parameter(initializer.zeros_(torch.empty(fout)))


class _Conv1(torch.nn.Module):
    """Parameters of nn.Conv1D(C, C, 1): weight [out, in, 1], bias [out]; Paddle's defaults (N(0, sqrt(2 / (k * in))) weight, zero
    bias)."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        from ..utils import initializer

        self.weight = torch.nn.Parameter(initializer.normal_(torch.empty(cout, cin, 1), 0.0, math.sqrt(2.0 / cin)))
        self.bias = torch.nn.Parameter(initializer.zeros_(torch.empty(cout)))


class SpectralConv1d(torch.nn.Module):
    """Parameters of geofno.py:21-46: real and imaginary parts U(0, 1) / (in * out)."""

    def __init__(self, in_channels: int, out_channels: int, modes1: int):
        super().__init__()
        from ..utils import initializer

        self.in_channels, self.out_channels, self.modes1 = in_channels, out_channels, modes1
        self.scale = 1 / (in_channels * out_channels)
        shape = (in_channels, out_channels, modes1)
        self.weights1_real = torch.nn.Parameter(initializer.uniform_(torch.empty(shape), 0, 1) * self.scale)
        self.weights1_imag = torch.nn.Parameter(initializer.uniform_(torch.empty(shape), 0, 1) * self.scale)


class FNO1d(OperatorArch):
    """ppsci.arch.FNO1d (geofno.py:95-205); constructor arguments in the reference's order.  `forward_tensor`:
    [B, s, input_channel] -> [B, output_np, 1]."""

    _executor = "geofno_engine.Fno1dNative"
    channel_axis = -1  # input keys are concatenated along the LAST axis (channel-last fields)

    def __init__(self, input_key: Tuple[str, ...] = ("input",), output_key: Tuple[str, ...] = ("output",), modes: int = 64,
                 width: int = 64, padding: int = 100, input_channel: int = 2, output_np: int = 2001):
        OperatorArch.__init__(self)
        self.input_keys, self.output_keys = tuple(input_key), tuple(output_key)
        if len(self.output_keys) != 1:
            raise NotImplementedError("FNO1d with more than one output key: fc2 has one output feature")
        self.output_np, self.modes1, self.width, self.padding = int(output_np), int(modes), int(width), int(padding)
        self.input_channel, self.hidden_features = int(input_channel), HIDDEN
        if self.padding == 0:
            raise NotImplementedError("FNO1d(padding=0): the reference crops with x[..., :-padding], which is empty for 0")
        if self.padding < 0 or self.modes1 < 1 or self.width < 1 or self.input_channel < 1 or self.output_np < 1:
            raise ValueError("FNO1d: modes, width, padding, input_channel and output_np must be positive")
        self.fc0 = _Linear(self.input_channel, self.width)
        for k in range(5):
            setattr(self, f"conv{k}", SpectralConv1d(self.width, self.width, self.modes1))
        for k in range(4):
            setattr(self, f"w{k}", _Conv1(self.width, self.width))
        self.fc1 = _Linear(self.width, HIDDEN)
        self.fc2 = _Linear(HIDDEN, 1)
        from ..device import get_device

        self.to_device(get_device())
