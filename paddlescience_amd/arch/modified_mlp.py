"""ppsci.arch.ModifiedMLP (/root/reference/ppsci/arch/mlp.py:318-528; Wang, Teng & Perdikaris 2020) on HIP kernels, layer by
layer with the machinery of arch/layer_by_layer.py and PirateNet's gated executor:

    x0 = [period-embedded inputs]  (or  [cos(B e) ; sin(B e)]  with `fourier`)
    U, V = act(W_u x0 + b_u), act(W_v x0 + b_v)
    y <- act(W_l y + b_l);  y <- y * U + (1 - y) * V        for every hidden layer (the first one reads x0)
    out = W_L y + b_L

Dense layers are `ppsci_pw_conv` GEMMs over all Taylor streams; bias + activation + gate and their reverse are
`ppsci_pirate_act_*` (csrc/pirate.hip).  Trainable tensors in the reference's `parameters()` order and names:
[fourier_emb.kernel], embed_u.0.*, embed_v.0.*, linears.i.*, last_fc.* (`weight`/`bias`, or `weight_v`/`weight_g`/`bias` with
`random_weight`).  Not available (raise): weight_norm, skip_connection, learnable activations, derivative order > 2, input
transforms.  (SPINN's one-input branch nets use their own fused kernels, csrc/spinn.hip.)"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from .. import _lib as L
from .layer_by_layer import StreamMLP
from .piratenet import PirateExec


class ModifiedMLP(StreamMLP):
    def __init__(
        self,
        input_keys: Tuple[str, ...],
        output_keys: Tuple[str, ...],
        num_layers: int,
        hidden_size: int,
        activation: str = "tanh",
        skip_connection: bool = False,
        weight_norm: bool = False,
        input_dim: Optional[int] = None,
        output_dim: Optional[int] = None,
        periods: Optional[Dict[str, Tuple[float, bool]]] = None,
        fourier: Optional[Dict[str, Union[float, int]]] = None,
        random_weight: Optional[Dict[str, float]] = None,
    ):
        if not isinstance(hidden_size, int):
            raise ValueError(f"hidden_size should be int, but got {type(hidden_size)}")  # mlp.py:374-375
        if not isinstance(num_layers, int):
            raise ValueError("num_layers should be an int")  # mlp.py:371-372
        if weight_norm or skip_connection:
            raise NotImplementedError("ModifiedMLP(weight_norm / skip_connection) has no HIP kernel path")
        super().__init__("ModifiedMLP", input_keys, output_keys, activation, input_dim, output_dim, periods, fourier, random_weight)
        self.hidden, self.num_gated_layers = int(hidden_size), int(num_layers)
        H = self.hidden
        layers = self._lin("embed_u.0", self.c0, H) + self._lin("embed_v.0", self.c0, H)
        for i in range(self.num_gated_layers):
            layers += self._lin(f"linears.{i}", self.c0 if i == 0 else H, H)
        self._finish(layers + self._lin("last_fc", H, len(self.output_keys)), self.num_gated_layers)

    def linear_names(self):
        return ["embed_u.0", "embed_v.0"] + [f"linears.{i}" for i in range(self.num_gated_layers)] + ["last_fc"]

    def _make_exec(self, spec, n, inputs=None, train=True):
        return ModifiedExec(self, spec, n, inputs, train)


class ModifiedExec(PirateExec):
    """forward / backward launch sequences of ModifiedMLP over PirateExec's buffers and helpers."""

    def _alloc_layers(self) -> None:
        self.layers = [dict(Z=self._blk(), O=self._blk()) for _ in range(self.model.num_gated_layers)]

    def forward(self, params: torch.Tensor, Urows: torch.Tensor, train: bool) -> None:
        H, c0 = self.H, self.c0
        self._materialize(params)
        self._embed_fwd(params, self.X0)
        self._dense(self.X0, self._w(params, "embed_u.0"), c0, H, self.ZU)
        self._act_fwd(L.PIRATE_ACT, self.ZU, self._t(params, "embed_u.0.bias"), self.U)
        self._dense(self.X0, self._w(params, "embed_v.0"), c0, H, self.ZV)
        self._act_fwd(L.PIRATE_ACT, self.ZV, self._t(params, "embed_v.0.bias"), self.V)
        y, fin = self.X0, c0
        for i, lay in enumerate(self.layers):
            self._dense(y, self._w(params, f"linears.{i}"), fin, H, lay["Z"])
            self._act_fwd(L.PIRATE_GATE, lay["Z"], self._t(params, f"linears.{i}.bias"), lay["O"], U=self.U, V=self.V)
            y, fin = lay["O"], H
        self._dense(y, self._w(params, "last_fc"), fin, self.m, self.Y)
        self._out_fwd(self.Y, params, Urows)

    def backward(self, params: torch.Tensor, Ubar_rows: torch.Tensor, grad: torch.Tensor) -> None:
        self._begin_reverse()
        m, H, c0 = self.model, self.H, self.c0
        grad = grad.view(-1)
        nl = len(self.layers)
        self._out_bwd(Ubar_rows, self.Ybar, grad)
        ylast, flast = (self.layers[-1]["O"], H) if nl else (self.X0, c0)
        self._wgrad(ylast, self.Ybar, flast, self.m, "last_fc", params, grad)
        xb0 = self.XB0 if self.XB0 is not None else self.XB[1]  # adjoint of x0
        ybar = self.OB if nl else xb0
        self._dense_t(self.Ybar, self._w(params, "last_fc"), flast, self.m, ybar)
        self.UB.zero_()
        self.VB.zero_()
        wrote_x0 = nl == 0
        for i in range(nl - 1, -1, -1):
            lay = self.layers[i]
            yin, fin = (self.layers[i - 1]["O"], H) if i > 0 else (self.X0, c0)
            self._act_bwd(L.PIRATE_GATE, lay["Z"], f"linears.{i}.bias", self.OB, params, grad, U=self.U, V=self.V)
            self._wgrad(yin, self.ZB, fin, H, f"linears.{i}", params, grad)
            if i > 0:
                self._dense_t(self.ZB, self._w(params, f"linears.{i}"), fin, H, self.OB)
            elif m.half:  # the adjoint of x0 is only needed for the Fourier kernel's gradient
                self._dense_t(self.ZB, self._w(params, f"linears.{i}"), fin, H, xb0)
                wrote_x0 = True
        for name, Z, B_ in (("embed_u.0", self.ZU, self.UB), ("embed_v.0", self.ZV, self.VB)):
            self._act_bwd(L.PIRATE_ACT, Z, name + ".bias", B_, params, grad)
            self._wgrad(self.X0, self.ZB, c0, H, name, params, grad)
            if m.half:
                self._dense_t(self.ZB, self._w(params, name), c0, H, xb0, accumulate=wrote_x0)
                wrote_x0 = True
        if m.half:
            self._embed_bwd(params, xb0, grad)
        self._flush_sums(self.ZB)
