"""ppsci.arch.PirateNet (/root/reference/ppsci/arch/mlp.py:530-820) on HIP kernels, layer by layer.

PirateNet's gates multiply the streams of three tensors (f * U + (1 - f) * V), which the register-resident single-kernel
MLP sweep (taylor_fwd / taylor_bwd) cannot hold; here every dense layer is one MFMA GEMM over all Taylor streams at once
(`ppsci_pw_conv`, [S, C, NP] = its [B, C, P]) and the stages in between -- period / Fourier embedding, bias + activation
fused with the gate or with the residual connection, and their hand-written reverse -- are the kernels of csrc/pirate.hip.
The residual expressions, losses and the optimizer are the same fused path as for ppsci.arch.MLP: `PirateExec` is what
`engine.FusedConstraint` runs in place of `taylor_fwd` / `taylor_bwd` for this architecture.

Trainable tensors, in the reference's `parameters()` order and with its names (one flat fp32 device buffer):
    fourier_emb.kernel                                       [d0, dim/2]
    embed_u.0.{weight,bias} | {weight_v,weight_g,bias}       nn.Linear | RandomWeightFactorization
    embed_v.0. ...
    blocks.i.alpha [1], blocks.i.linear{1,2,3}. ...
    last_fc. ...
Not available (raise): weight_norm, learnable activations (stan / swish), derivative order > 2, a `fourier` embedding
whose dim differs from hidden_size (the reference's own block arithmetic needs them equal), input transforms."""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from .. import _lib as L
from .. import hotpath as hp
from .layer_by_layer import LayerExec, StreamMLP


class PirateNet(StreamMLP):
    def __init__(
        self,
        input_keys: Tuple[str, ...],
        output_keys: Tuple[str, ...],
        num_blocks: int,
        hidden_size: int,
        activation: str = "tanh",
        weight_norm: bool = False,
        input_dim: Optional[int] = None,
        output_dim: Optional[int] = None,
        periods: Optional[Dict[str, Tuple[float, bool]]] = None,
        fourier: Optional[Dict[str, Union[float, int]]] = None,
        random_weight: Optional[Dict[str, float]] = None,
    ):
        if not isinstance(hidden_size, int):
            raise ValueError(f"hidden_size should be int, but got {type(hidden_size)}")  # mlp.py:693-694
        if not isinstance(num_blocks, int):
            raise ValueError("num_blocks should be an int")  # mlp.py:690-691
        if weight_norm:
            raise NotImplementedError("PirateNet(weight_norm=True) has no HIP kernel path")
        super().__init__("PirateNet", input_keys, output_keys, activation, input_dim, output_dim, periods, fourier, random_weight)
        self.num_blocks, self.hidden = int(num_blocks), int(hidden_size)
        if not fourier:
            raise NotImplementedError("PirateNet without a `fourier` embedding: the blocks add tensors of width "
                                      "hidden_size to the embedded input (mlp.py:614-621), so the reference itself only "
                                      "runs when the two agree; give fourier={'dim': hidden_size, 'scale': ...}")
        if int(fourier["dim"]) != self.hidden:
            raise NotImplementedError("fourier['dim'] must equal hidden_size (PirateNetBlock adds them, mlp.py:614-621)")
        H = self.hidden
        layers = self._lin("embed_u.0", H, H) + self._lin("embed_v.0", H, H)
        for i in range(self.num_blocks):
            layers.append((f"blocks.{i}.alpha", (1,)))
            for j in (1, 2, 3):
                layers += self._lin(f"blocks.{i}.linear{j}", H, H)
        self._finish(layers + self._lin("last_fc", H, len(self.output_keys)), 3 * self.num_blocks + 1)

    def linear_names(self):
        out = ["embed_u.0", "embed_v.0"]
        for i in range(self.num_blocks):
            out += [f"blocks.{i}.linear{j}" for j in (1, 2, 3)]
        return out + ["last_fc"]

    def _make_exec(self, spec, n, inputs=None, train=True):
        return PirateExec(self, spec, n, inputs, train)


class PirateExec(LayerExec):
    """Buffers and launch sequence of PirateNet; ModifiedExec runs its own sequence over the same buffers and helpers."""

    def __init__(self, model: StreamMLP, spec: hp.StreamSpec, n: int, inputs=None, train: bool = True):
        super().__init__(model, spec, n, inputs, model.label, model.input_keys, model.d0, model.half, model._embed, model._omega)
        self.H, self.c0 = model.hidden, model.c0  # c0: channels of x0 (PirateNet: = hidden; ModifiedMLP: d0 or fourier dim)
        self.act = L.ACT[model.activation]
        self.X0, self.ZU, self.ZV, self.U, self.V = self._blk(self.c0), self._blk(), self._blk(), self._blk(), self._blk()
        self._alloc_layers()
        self.Y = self._blk(self.m)
        if train:
            self._begin_reverse()

    def _blk(self, c: Optional[int] = None) -> torch.Tensor:
        return torch.zeros((self.S, c or self.H, self.NP), **self.f32)

    def _alloc_layers(self) -> None:
        blk = self._blk
        self.blocks = [dict(Z1=blk(), O1=blk(), Z2=blk(), O2=blk(), Z3=blk(), X=blk()) for _ in range(self.model.num_blocks)]

    def _act_fwd(self, mode, z, bias, out, **gate):
        self._act(mode, self.act, self.H, self.n1, self.n2, z, bias, out, **gate)

    # ---- forward
    def forward(self, params: torch.Tensor, Urows: torch.Tensor, train: bool) -> None:
        H = self.H
        self._materialize(params)
        self._embed_fwd(params, self.X0)
        self._dense(self.X0, self._w(params, "embed_u.0"), H, H, self.ZU)
        self._act_fwd(L.PIRATE_ACT, self.ZU, self._t(params, "embed_u.0.bias"), self.U)
        self._dense(self.X0, self._w(params, "embed_v.0"), H, H, self.ZV)
        self._act_fwd(L.PIRATE_ACT, self.ZV, self._t(params, "embed_v.0.bias"), self.V)
        x = self.X0
        for i, b in enumerate(self.blocks):
            pre = f"blocks.{i}."
            self._dense(x, self._w(params, pre + "linear1"), H, H, b["Z1"])
            self._act_fwd(L.PIRATE_GATE, b["Z1"], self._t(params, pre + "linear1.bias"), b["O1"], U=self.U, V=self.V)
            self._dense(b["O1"], self._w(params, pre + "linear2"), H, H, b["Z2"])
            self._act_fwd(L.PIRATE_GATE, b["Z2"], self._t(params, pre + "linear2.bias"), b["O2"], U=self.U, V=self.V)
            self._dense(b["O2"], self._w(params, pre + "linear3"), H, H, b["Z3"])
            self._act_fwd(L.PIRATE_RES, b["Z3"], self._t(params, pre + "linear3.bias"), b["X"], x=x,
                          alpha=self._t(params, pre + "alpha"))
            x = b["X"]
        self._dense(x, self._w(params, "last_fc"), H, self.m, self.Y)
        self._out_fwd(self.Y, params, Urows)

    # ---- reverse
    def _alloc_train(self):
        super()._alloc_train()
        blk = self._blk
        self.Ybar = blk(self.m)
        self.XB = [blk(), blk()]  # adjoint of the running block input / output (ping-pong)
        self.OB, self.ZB, self.UB, self.VB = blk(), blk(), blk(), blk()
        self.XB0 = blk(self.c0) if self.c0 != self.H else None  # adjoint of x0 when its width differs from the hidden one

    def _act_bwd(self, mode, z, bias_name, obar, params, grad, **gate):
        if mode == L.PIRATE_GATE:
            gate.update(ubar=self.UB, vbar=self.VB)
        self._act_rev(mode, self.act, self.H, self.n1, self.n2, z, bias_name, obar, self.ZB, params, grad, **gate)

    def backward(self, params: torch.Tensor, Ubar_rows: torch.Tensor, grad: torch.Tensor) -> None:
        self._begin_reverse()
        H = self.H
        grad = grad.view(-1)
        # last_fc
        self._out_bwd(Ubar_rows, self.Ybar, grad)
        xlast = self.blocks[-1]["X"] if self.blocks else self.X0
        self._wgrad(xlast, self.Ybar, H, self.m, "last_fc", params, grad)
        cur = 0
        self._dense_t(self.Ybar, self._w(params, "last_fc"), H, self.m, self.XB[cur])
        self.UB.zero_()
        self.VB.zero_()
        for i in range(len(self.blocks) - 1, -1, -1):
            b, pre = self.blocks[i], f"blocks.{i}."
            xin = self.blocks[i - 1]["X"] if i > 0 else self.X0
            nxt = 1 - cur
            # x' = alpha h + (1 - alpha) x;  h = act(W3 o2 + b3)
            self._act_bwd(L.PIRATE_RES, b["Z3"], pre + "linear3.bias", self.XB[cur], params, grad, x=xin,
                          alpha_name=pre + "alpha", xbar=self.XB[nxt])
            self._wgrad(b["O2"], self.ZB, H, H, pre + "linear3", params, grad)
            self._dense_t(self.ZB, self._w(params, pre + "linear3"), H, H, self.OB)
            # o2 = gate(act(W2 o1 + b2))
            self._act_bwd(L.PIRATE_GATE, b["Z2"], pre + "linear2.bias", self.OB, params, grad, U=self.U, V=self.V)
            self._wgrad(b["O1"], self.ZB, H, H, pre + "linear2", params, grad)
            self._dense_t(self.ZB, self._w(params, pre + "linear2"), H, H, self.OB)
            # o1 = gate(act(W1 x + b1))
            self._act_bwd(L.PIRATE_GATE, b["Z1"], pre + "linear1.bias", self.OB, params, grad, U=self.U, V=self.V)
            self._wgrad(xin, self.ZB, H, H, pre + "linear1", params, grad)
            self._dense_t(self.ZB, self._w(params, pre + "linear1"), H, H, self.XB[nxt], accumulate=True)
            cur = nxt
        # embeddings U = act(W_u x0 + b_u), V = act(W_v x0 + b_v): their adjoints were accumulated by the gates
        for name, Z, B_ in (("embed_u.0", self.ZU, self.UB), ("embed_v.0", self.ZV, self.VB)):
            self._act_bwd(L.PIRATE_ACT, Z, name + ".bias", B_, params, grad)
            self._wgrad(self.X0, self.ZB, H, H, name, params, grad)
            self._dense_t(self.ZB, self._w(params, name), H, H, self.XB[cur], accumulate=True)
        self._embed_bwd(params, self.XB[cur], grad)
        self._flush_sums(self.ZB)
