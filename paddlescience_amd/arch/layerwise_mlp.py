"""ppsci.arch.MLP configurations OUTSIDE the envelope of the fused single-kernel sweep (taylor_fwd / taylor_bwd: hidden width
<= 256, `fourier.dim == hidden_size`, per-layer widths only with plain layers), run layer by layer on Taylor streams with
the machinery of arch/layer_by_layer.py: every dense layer is one MFMA GEMM over all streams (`ppsci_pw_conv`), bias + activation
and their reverse are `ppsci_pirate_act_*` (mode ACT), the period / Fourier embedding is `ppsci_pirate_embed_*`.

`ppsci.arch.MLP(...)` returns an instance of this class for

    * a hidden width above 256 (any width whose 16-row weight block fits LDS: up to 2 560),
    * a Fourier embedding whose dim differs from hidden_size, or with an activation other than tanh,
    * per-layer widths together with `random_weight` or `fourier`,

with the reference's parameter names and order (mlp.py:196-277): [fourier_emb.kernel], linears.i.{weight,bias} or
{weight_v,weight_g,bias}, last_fc.*.  Derivative orders 0-2; not available here either: weight_norm, skip_connection, learnable
activations (stan / swish), siren, input transforms."""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from .layer_by_layer import ACTS, LayerExec, Stack, StreamMLP


def wants_layerwise(num_layers, hidden_size, activation="tanh", skip_connection=False, weight_norm=False, input_dim=None,
                    output_dim=None, periods=None, fourier=None, random_weight=None) -> bool:
    """True when the fused kernels cannot run this MLP but the layer-by-layer path can."""
    if isinstance(hidden_size, (tuple, list)):
        hidden = [int(h) for h in hidden_size]
    elif isinstance(hidden_size, int) and isinstance(num_layers, int):
        hidden = [hidden_size] * num_layers
    else:
        return False
    if not hidden or weight_norm or skip_connection or str(activation).lower() not in ACTS:
        return False
    ragged = len(set(hidden)) != 1
    if max(hidden) > 256:
        return max(hidden) <= 2560
    if fourier and (int(fourier["dim"]) != hidden[0] or ragged or str(activation).lower() != "tanh"):
        return True
    return bool(ragged and random_weight)


class LayerwiseMLP(StreamMLP):
    def __init__(self, input_keys, output_keys, num_layers, hidden_size, activation: str = "tanh", skip_connection: bool = False,
                 weight_norm: bool = False, input_dim: Optional[int] = None, output_dim: Optional[int] = None,
                 periods: Optional[Dict[str, Tuple[float, bool]]] = None, fourier: Optional[Dict[str, Union[float, int]]] = None,
                 random_weight: Optional[Dict[str, float]] = None):
        if isinstance(hidden_size, (tuple, list)):
            if num_layers is not None:
                raise ValueError("num_layers should be None when hidden_size is specified")
            self.widths = [int(h) for h in hidden_size]
        else:
            self.widths = [int(hidden_size)] * int(num_layers)
        if weight_norm or skip_connection:
            raise NotImplementedError("layer-by-layer MLP: weight_norm / skip_connection are not available")
        super().__init__("layer-by-layer MLP", input_keys, output_keys, activation, input_dim, output_dim, periods, fourier,
                         random_weight)
        self.hidden = max(self.widths)
        layers, fin = [], self.c0
        for i, w in enumerate(self.widths):
            layers += self._lin(f"linears.{i}", fin, w)
            fin = w
        self._finish(layers + self._lin("last_fc", fin, len(self.output_keys)), len(self.widths))

    def linear_names(self):
        return [f"linears.{i}" for i in range(len(self.widths))] + ["last_fc"]

    def _make_exec(self, spec, n, inputs=None, train=True):
        return PlainExec(self, spec, n, inputs, train)


class PlainExec(LayerExec):
    """x0 -> (GEMM, bias + activation) per hidden layer -> GEMM: one plain stack behind the embedding."""

    # Sums are taken at once, from scratch that all layers share, and every factored layer has its own launch: partial
    # buffers kept to the end of the pass would be wchunks * fin * fout floats per layer (gigabytes at width 2 560), and
    # ppsci_reduce_rows_multi adds a [rows >= 512, cols <= 8] block in another order than ppsci_reduce_rows does.
    batched = False

    def __init__(self, model: LayerwiseMLP, spec, n: int, inputs=None, train: bool = True):
        super().__init__(model, spec, n, inputs, model.label, model.input_keys, model.d0, model.half, model._embed, model._omega)
        self.st = Stack("", model.c0, list(model.widths), self.m, model.activation, self.S, self.NP, self.f32)
        if train:
            self._begin_reverse()

    def _alloc_train(self):
        super()._alloc_train()
        st = self.st
        st.alloc_train()
        wmax = max(a * b for a, b in zip([st.d_in] + st.widths, st.widths + [st.d_out]))
        zeros = lambda k: torch.zeros(k, **self.f32)  # noqa: E731
        self._scratch = dict(b=zeros(self.achunks * max(st.widths)), w=zeros(self.wchunks * wmax),
                             g=zeros(wmax) if self.model._rwf else None)

    def forward(self, params: torch.Tensor, Urows: torch.Tensor, train: bool) -> None:
        self._materialize(params)
        self._embed_fwd(params, self.st.X)
        self._stack_fwd(self.st, params, self.n1, self.n2)
        self._out_fwd(self.st.Y, params, Urows)

    def backward(self, params: torch.Tensor, Ubar_rows: torch.Tensor, grad: torch.Tensor) -> None:
        self._begin_reverse()
        grad = grad.view(-1)
        self._out_bwd(Ubar_rows, self.st.Ybar, grad)
        xbar = self._stack_bwd(self.st, params, grad, self.n1, self.n2, self.wchunks, bool(self.half))
        if self.half:  # the adjoint of x0 is only needed for the Fourier kernel's gradient
            self._embed_bwd(params, xbar, grad)
