"""What the point networks that run layer by layer on Taylor streams share: PirateNet, ModifiedMLP, LayerwiseMLP and the
DeepONets.  Every dense layer is one MFMA GEMM over all streams (`ppsci_pw_conv`, [S, C, NP] = its [B, C, P]),
bias + activation and their reverse are `ppsci_pirate_act_*`, the period / Fourier embedding is `ppsci_pirate_embed_*`
(csrc/pirate.hip).

    FlatParamArch   (name, shape) parameters in one flat fp32 device buffer; state dict; traced / numeric forward
    StreamMLP       the constructor prologue, layer shapes and initialiser of the three MLP-like models
    LayerLayout     what compile / engine need to know about such a network
    LayerExec       buffers and launch helpers of one (network, stream set, batch size), the plain stack included"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from .. import hotpath as hp
from ..device import get_device
from ..graph import Sym
from . import activation as act_mod
from .base import Arch

_p = hp._p
_sp = hp._stream_ptr
ACTS = ("tanh", "silu", "sigmoid", "sin", "cos", "gelu")


class LayerLayout:
    """What compile / engine need to know about the network (the role hotpath.NetLayout plays for MLP)."""

    layer_by_layer = True  # engine.FusedConstraint: make_exec's executor stands in for taylor_fwd / taylor_bwd

    def __init__(self, model: "FlatParamArch", d_raw: int, d_out: int, n_hidden: int, width: int, embed=None, omega=None):
        self.model = model
        self.d_raw, self.d_out, self.n_hidden, self.width = d_raw, d_out, n_hidden, width
        self.embed, self.omega = embed, omega

    @property
    def n_params(self) -> int:
        return self.model.n_params

    def desc(self, streams):
        return None

    def make_exec(self, spec: hp.StreamSpec, n: int, inputs) -> "LayerExec":
        return self.model._make_exec(spec, n, inputs)


class FlatParamArch(Arch):
    """A model whose trainable tensors are (name, shape) pairs in ONE flat fp32 device buffer, in the reference's
    `parameters()` order and with its names.  A subclass hands `_store` its shapes and supplies
    `_make_exec(spec, n, inputs=None, train=True)` and `_check_transforms()` (which registered transforms it refuses);
    `_rows` where a batch is not one column per input key."""

    reparam = False  # factorised layers are materialised inside the executor; gradients come out in the trainable layout
    _rwf: Optional[Dict[str, float]] = None  # random weight factorisation: the MLP-like models' option

    def _store(self, shapes: List[Tuple[str, Tuple[int, ...]]]) -> None:
        self._shapes = shapes
        self._bind_views(torch.zeros(max(1, sum(int(np.prod(s)) for _, s in shapes)), dtype=torch.float32, device=get_device()))
        self._frozen = False
        self._predict_exec: Dict[int, "LayerExec"] = {}  # numeric forward: one executor per batch size

    def _bind_views(self, flat: torch.Tensor) -> None:
        self.flat_params = self.kernel_params = flat
        self._names, self._views, self._offsets = [], [], {}
        off = 0
        for name, shp in self._shapes:
            n = int(np.prod(shp))
            self._names.append(name)
            self._views.append(flat[off:off + n].view(tuple(shp)))
            self._offsets[name] = (off, n)
            off += n
        self._byname = dict(zip(self._names, self._views))

    def rehome(self, flat: torch.Tensor, flat_grad=None, kernel=None) -> None:
        """ModelList: move the trainable parameters into `flat` (a slice of the list's buffer), keeping their values."""
        assert flat.numel() == self.flat_params.numel()
        flat.copy_(self.flat_params)
        self._bind_views(flat)

    @property
    def n_params(self) -> int:
        return int(self.flat_params.numel())

    def parameters(self) -> List[torch.Tensor]:
        return list(self._views)

    def named_parameters(self):
        return list(zip(self._names, self._views))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(zip(self._names, self._views))

    def set_state_dict(self, state):
        missing = [n for n in self._names if n not in state]
        unexpected = [n for n in state if n not in self._names]
        for n, v in zip(self._names, self._views):
            if n in state:
                src = state[n]
                src = torch.as_tensor(np.asarray(src.detach().cpu() if isinstance(src, torch.Tensor) else src), dtype=torch.float32)
                if v.dim() == 0 and src.numel() == 1:  # a 0-d beta stored as [1]
                    src = src.reshape(())
                if tuple(src.shape) != tuple(v.shape):
                    raise ValueError(f"shape mismatch for {n}: {tuple(src.shape)} vs {tuple(v.shape)}")
                v.copy_(src)
        return missing, unexpected

    def materialize(self) -> torch.Tensor:
        return self.flat_params

    def pull_back(self, grad: torch.Tensor) -> torch.Tensor:
        return grad

    # ---- forward
    def _rows(self, ins: Dict[str, torch.Tensor]) -> int:
        """Batch size of a numeric call (every input key is one column of it)."""
        return ins[self.input_keys[0]].numel()

    def _forward_numeric(self, x: Dict[str, object]) -> Dict[str, torch.Tensor]:
        dev = self.flat_params.device
        ins = {}
        for k in self.input_keys:
            if k not in x:
                raise KeyError(f"input {k!r} of {type(self).__name__} is missing")
            v = x[k]
            if not isinstance(v, torch.Tensor):
                v = torch.as_tensor(np.asarray(v), dtype=torch.float32)
            ins[k] = v.to(device=dev, dtype=torch.float32).contiguous()
        n = self._rows(ins)
        ex = self._predict_exec.get(n)
        if ex is None:
            if len(self._predict_exec) > 4:
                self._predict_exec.clear()
            ex = self._predict_exec[n] = self._make_exec(hp.StreamSpec([], 0), n, train=False)
        ex.set_inputs(ins)
        U = torch.empty((len(self.output_keys), n), dtype=torch.float32, device=dev)
        ex.forward(self.flat_params, U, False)
        return {k: U[i].view(n, 1) for i, k in enumerate(self.output_keys)}

    def forward(self, x: Dict[str, object]) -> Dict[str, object]:  # mlp.py:802-820
        self._check_transforms()
        if any(isinstance(v, Sym) for v in x.values()):
            for k in self.input_keys:  # a constraint's trace: the outputs are network nodes of the expression graph
                v = x.get(k)
                if not (isinstance(v, Sym) and v.kind == "in" and v.name == k):
                    raise NotImplementedError(f"network input {k!r} must be the raw variable of the data dict")
            y = {k: Sym.net(self, i) for i, k in enumerate(self.output_keys)}
        else:
            y = self._forward_numeric(x)
        if self._output_transform is not None:
            y = self._output_transform(x, y)
        return y


class StreamMLP(FlatParamArch):
    """The part PirateNet, ModifiedMLP and LayerwiseMLP share: period / Fourier embedding of the input keys into x0
    (`c0` channels), then linear layers that are nn.Linear or RandomWeightFactorization.  `label` names the model in errors;
    a subclass refuses its own options first, then lists its layers (`_lin`, `linear_names`) and calls `_finish`."""

    def __init__(self, label: str, input_keys, output_keys, activation, input_dim, output_dim, periods, fourier, random_weight):
        super().__init__()
        self.label = label
        self.input_keys, self.output_keys = tuple(input_keys), tuple(output_keys)
        if input_dim is not None and int(input_dim) != len(self.input_keys):
            raise NotImplementedError("multi-column inputs (input_dim != number of input keys)")
        if output_dim is not None and int(output_dim) != len(self.output_keys):
            raise NotImplementedError("multi-column outputs (output_dim != number of output keys)")
        self.activation = act_mod.get_activation(activation)
        if self.activation not in ACTS:
            raise NotImplementedError(f"{label} activation {activation!r}: the stream kernels carry {ACTS}")
        if len(self.input_keys) > L.MAX_IN or len(self.output_keys) > L.MAX_OUT:
            raise NotImplementedError(f"at most {L.MAX_IN} inputs / {L.MAX_OUT} outputs")
        self.periods, self.fourier = periods, fourier
        self._rwf = dict(random_weight) if random_weight else None
        self._embed = [L.EMBED_NONE] * len(self.input_keys)
        self._omega = [0.0] * len(self.input_keys)
        if periods:
            from .mlp import PeriodEmbedding

            self.period_emb = PeriodEmbedding(periods)
            for k, w in self.period_emb.freqs_dict.items():
                j = self.input_keys.index(k)
                self._embed[j], self._omega[j] = L.EMBED_PERIOD, w
        self.d0 = len(self.input_keys) + sum(1 for e in self._embed if e == L.EMBED_PERIOD)
        self.half = 0
        if fourier:
            if int(fourier["dim"]) % 2 != 0:
                raise ValueError(f"out_features must be even, but got {fourier['dim']}.")  # mlp.py:120-121
            self.half = int(fourier["dim"]) // 2
        self.c0 = 2 * self.half if self.half else self.d0  # width of x0

    def _check_transforms(self) -> None:
        if self._input_transform is not None:
            raise NotImplementedError("PirateNet with a registered input transform")

    def _lin(self, name: str, fin: int, fout: int) -> List[Tuple[str, Tuple[int, ...]]]:
        if self._rwf:
            return [(f"{name}.weight_v", (fin, fout)), (f"{name}.weight_g", (fout,)), (f"{name}.bias", (fout,))]
        return [(f"{name}.weight", (fin, fout)), (f"{name}.bias", (fout,))]

    def _finish(self, layers: List[Tuple[str, Tuple[int, ...]]], n_hidden: int) -> None:
        self._store(([("fourier_emb.kernel", (self.d0, self.half))] if self.half else []) + layers)
        self.layout = LayerLayout(self, len(self.input_keys), len(self.output_keys), n_hidden, self.hidden, self._embed, self._omega)
        self._init_parameters()

    def _init_parameters(self):
        """Same draws as the reference's constructors, from numpy's global RNG (ppsci.utils.misc.set_random_seed), the
        Fourier kernel first, then linear_names() in order: FourierEmbedding Normal(std=scale) (mlp.py:123-126); nn.Linear
        Xavier-uniform / zero bias; RandomWeightFactorization glorot normal v, g = exp(N(mean, std)), v <- v / g
        (mlp.py:78-85).  Everything else stays 0 (PirateNet's alpha, mlp.py:590-595)."""
        t = self._byname
        if self.half:
            k = t["fourier_emb.kernel"]
            k.copy_(torch.from_numpy(np.random.normal(0.0, float(self.fourier["scale"]), size=tuple(k.shape)).astype(np.float32)))
        for name in self.linear_names():
            w = t[name + (".weight_v" if self._rwf else ".weight")]
            fin, fout = w.shape
            if self._rwf:
                vv = np.random.normal(0.0, math.sqrt(2.0 / (fin + fout)), size=(fin, fout)).astype(np.float32)
                gg = np.exp(np.random.normal(self._rwf["mean"], self._rwf["std"], size=(fout,)).astype(np.float32))
                w.copy_(torch.from_numpy(vv / gg))
                t[name + ".weight_g"].copy_(torch.from_numpy(gg))
            else:
                lim = math.sqrt(6.0 / (fin + fout))
                w.copy_(torch.from_numpy(np.random.uniform(-lim, lim, size=(fin, fout)).astype(np.float32)))
            t[name + ".bias"].zero_()


class Stack:
    """Buffers of one plain stack x -> (GEMM, bias + activation) per hidden layer -> GEMM at S streams; its parameters are
    `pre`linears.i.*, `pre`acts.i.beta (swish) and `pre`last_fc.*.  Y is the last_fc output without its bias."""

    def __init__(self, pre: str, d_in: int, widths: List[int], d_out: int, act: str, S: int, NP: int, f32):
        self.pre, self.d_in, self.widths, self.d_out, self.act, self.S, self.NP, self.f32 = pre, d_in, widths, d_out, act, S, NP, f32
        blk = lambda c: torch.zeros((S, c, NP), **f32)  # noqa: E731
        self.X, self.Y = blk(d_in), blk(d_out)
        self.Z = [blk(w) for w in widths]
        self.A = [blk(w) for w in widths]

    def alloc_train(self) -> None:
        cmax = max(self.widths + [self.d_in])  # OB also takes the adjoint of X, where the caller asks for it
        self.OB, self.ZB = (torch.zeros(self.S * cmax * self.NP, **self.f32) for _ in range(2))
        self.Ybar = torch.zeros((self.S, self.d_out, self.NP), **self.f32)


class LayerExec:
    """Buffers and launch sequence of one (network, stream set, batch size); what engine.FusedConstraint runs in place of
    taylor_fwd / taylor_bwd: forward(params, Urows, train) fills the row block [d_out * S, N]; backward(params, Ubar_rows,
    grad) fully overwrites the flat [n_params] row `grad` with d loss / d (trainable parameters).

    `keys` are the per-point input columns the streams run along; `inputs` their [N] device columns, read in place --
    without them the executor owns the columns and set_inputs fills them.  A subclass allocates its activations, ends its
    constructor with `if train: self._begin_reverse()`, and writes forward / backward from the helpers below."""

    # Every producer of a reverse pass keeps its OWN partial-sum buffer to the end of the pass, where _flush_sums adds them
    # all up in one launch per 16 (dozens of reductions of ~6 us each are launch latency, not work); factored layers are
    # materialised / pulled back 16 per launch as well.  False (PlainExec): each sum is taken at once from scratch shared
    # by all layers, and every factored layer has a launch of its own.
    batched = True

    def __init__(self, model: FlatParamArch, spec: hp.StreamSpec, n: int, inputs: Optional[Sequence[torch.Tensor]], label: str,
                 keys: Sequence[str], d0: int, half: int = 0, embed=(), omega=()):
        if getattr(spec, "n3", 0) or getattr(spec, "n4", 0):
            raise NotImplementedError(f"{label}: derivative order > 2")
        self.model, self.spec, self.n, self.keys = model, spec, int(n), tuple(keys)
        self.n1, self.n2 = len(spec.dirs), int(spec.n2)
        self.S = 1 + self.n1 + self.n2
        self.NP = (self.n + 15) // 16 * 16
        self.m, self.half = len(model.output_keys), half
        self.f32 = dict(dtype=torch.float32, device=model.flat_params.device)
        self.inputs = list(inputs) if inputs is not None else [torch.zeros(self.n, **self.f32) for _ in self.keys]
        if len(self.inputs) != len(self.keys) or any(t.numel() != self.n for t in self.inputs):
            raise ValueError(f"{label}: expected {len(self.keys)} input columns of {self.n} values")
        d = self.desc = L.PirateEmbedDesc()
        d.d_raw, d.d0, d.half, d.n1, d.n2 = len(self.keys), d0, half, self.n1, self.n2
        for j, (e, w) in enumerate(zip(embed, omega)):
            d.embed[j], d.omega[j] = e, w
        for q, v in enumerate(spec.dirs):
            for j in range(d.d_raw):
                d.dirs[q][j] = float(v[j])
        d.N, d.NP = self.n, self.NP
        self._in_ptrs = (C.c_void_p * d.d_raw)(*[t.data_ptr() for t in self.inputs])
        # effective weights of the factorised layers (v * g): [fin, fout] row-major, what the GEMMs read
        self.weff = {}
        if model._rwf:
            for name in model.linear_names():
                fin, fout = model._byname[name + ".weight_v"].shape
                self.weff[name] = torch.zeros(fin * fout, **self.f32)
        self._pbufs: List[torch.Tensor] = []
        self._train_ready = False

    def set_inputs(self, x: Dict[str, torch.Tensor]) -> None:
        """Copies a batch into the executor's own input columns ([N] or [N, 1] per key)."""
        for dst, k in zip(self.inputs, self.keys):
            v = x[k]
            if v.numel() != self.n:
                raise ValueError(f"input key {k!r}: expected {self.n} values, got shape {tuple(v.shape)}")
            dst.copy_(v.reshape(-1))

    # ---- parameters
    def _t(self, params: torch.Tensor, name: str) -> torch.Tensor:
        """The tensor `name` inside a flat parameter (or gradient) row."""
        off, n = self.model._offsets[name]
        return params[off:off + n]

    def _w(self, params: torch.Tensor, name: str) -> torch.Tensor:
        return self.weff[name] if self.model._rwf else self._t(params, name + ".weight")

    def _materialize(self, params: torch.Tensor) -> None:
        m = self.model
        if not m._rwf:
            return
        jobs = [(L.LINEAR_RWF, *m._byname[name + ".weight_v"].shape, self._t(params, name + ".weight_v"),
                 self._t(params, name + ".weight_g"), None, self.weff[name], None) for name in m.linear_names()]
        if self.batched:
            hp.linear_multi(jobs, False, params)
        else:
            for job in jobs:
                hp.linear_materialize(*job)

    # ---- launches
    def _dense(self, x, W, fin, fout, out, accumulate=False, S=None):
        # out[s, o, p] = sum_i W[i, o] x[s, i, p]: nn.Linear weight [in, out] used as the transposed conv weight
        L.check(L.lib().ppsci_pw_conv(S or self.S, fin, fout, self.NP, _p(x), _p(W), 1, None, None, 1 if accumulate else 0,
                                      _p(out), None, _sp(out)))

    def _dense_t(self, gy, W, fin, fout, out, accumulate=False, S=None):
        # data gradient: out[s, i, p] (+)= sum_o W[i, o] gy[s, o, p]  (W [fin, fout] read as a conv weight [Co = fin, Ci = fout])
        L.check(L.lib().ppsci_pw_conv(S or self.S, fout, fin, self.NP, _p(gy), _p(W), 0, None, None, 1 if accumulate else 0,
                                      _p(out), None, _sp(out)))

    def _act(self, mode, act, c, n1, n2, z, bias, out, U=None, V=None, x=None, alpha=None):
        """out = bias + activation of z over c channels, alone (ACT), gated by U, V (GATE) or mixed with x by alpha (RES);
        `alpha` is also where ACT takes swish's beta."""
        L.check(L.lib().ppsci_pirate_act_fwd(mode, act, c, self.n, self.NP, n1, n2, _p(z), _p(bias), _p(U), _p(V), _p(x), _p(alpha),
                                             _p(out), _sp(out)))

    def _act_rev(self, mode, act, c, n1, n2, z, bias_name, obar, zbar, params, grad, U=None, V=None, x=None, alpha_name=None,
                 ubar=None, vbar=None, xbar=None):
        """Reverse of _act: obar -> zbar (and ubar / vbar / xbar), the bias' and alpha's gradients into `grad`."""
        alpha = self._t(params, alpha_name) if alpha_name else None
        pb = self._pbuf(self.achunks * c, "b")
        palpha = self._pbuf(c * self.achunks, "a") if alpha_name else None
        L.check(L.lib().ppsci_pirate_act_bwd(mode, act, c, self.n, self.NP, n1, n2, _p(z), _p(self._t(params, bias_name)), _p(U),
                                             _p(V), _p(x), _p(alpha), _p(obar), _p(zbar), _p(ubar), _p(vbar), _p(xbar), _p(pb),
                                             _p(palpha), _sp(zbar)))
        self._sum(pb, self.achunks, c, self._t(grad, bias_name))
        if alpha_name:
            self._sum(palpha, c * self.achunks, 1, self._t(grad, alpha_name))

    def _wgrad(self, x, zbar, fin, fout, name, params, grad, S=None, wchunks=None):
        """d loss / d W[i, o] = sum_{s,p} x[s,i,p] zbar[s,o,p] -> the layer's trainable tensors in `grad`."""
        S, wchunks, cols = S or self.S, wchunks or self.wchunks, fin * fout
        pw = self._pbuf(wchunks * cols, "w")
        # (conv roles swapped: "x" = zbar with Ci = fout, "gy" = x with Co = fin, so the partial blocks are [fin, fout])
        L.check(L.lib().ppsci_pw_conv_wgrad(S, fout, fin, self.NP, _p(zbar), _p(x), _p(pw), None, _sp(pw)))
        if self.model._rwf:
            gw = self._pbuf(cols, "g")
            self._sum(pw, wchunks, cols, gw)
            job = (L.LINEAR_RWF, fin, fout, self._t(params, name + ".weight_v"), self._t(params, name + ".weight_g"), gw, None,
                   self._t(grad, name + ".weight_v"), self._t(grad, name + ".weight_g"), None)
            if self.batched:
                self._pullbacks.append(job)
            else:
                hp.linear_pullback(*job)
        else:
            self._sum(pw, wchunks, cols, self._t(grad, name + ".weight"))

    def _embed_fwd(self, params, X0) -> None:
        kern = self._t(params, "fourier_emb.kernel") if self.half else None
        L.check(L.lib().ppsci_pirate_embed_fwd(C.byref(self.desc), self._in_ptrs, _p(kern), _p(X0), _sp(X0)))

    def _embed_bwd(self, params, xbar, grad) -> None:
        """The Fourier kernel's gradient from the adjoint of x0."""
        L.check(L.lib().ppsci_pirate_embed_bwd(C.byref(self.desc), self._in_ptrs, _p(self._t(params, "fourier_emb.kernel")),
                                               _p(xbar), _p(self.pB), _sp(self.pB)))
        self._sum(self.pB, self.echunks, self.pB.shape[1], self._t(grad, "fourier_emb.kernel"))

    def _out_fwd(self, Y, params, Urows) -> None:
        L.check(L.lib().ppsci_pirate_out_fwd(self.S, self.m, self.n, self.NP, _p(Y), _p(self._t(params, "last_fc.bias")),
                                             _p(Urows), _sp(Urows)))

    def _out_bwd(self, Ubar_rows, Ybar, grad) -> None:
        L.check(L.lib().ppsci_pirate_out_bwd(self.S, self.m, self.n, self.NP, _p(Ubar_rows), _p(Ybar), _sp(Ybar)))
        ob, _ = self.model._offsets["last_fc.bias"]
        for o in range(self.m):  # bias gradient = sum over points of the value-stream adjoint
            self._sum(Ubar_rows[o * self.S], self.n, 1, grad[ob + o:ob + o + 1])

    # ---- the reverse pass' sums
    def _alloc_train(self) -> None:
        lib = L.lib()
        self.achunks = int(lib.ppsci_pirate_act_chunks(self.NP))
        self.wchunks = int(lib.ppsci_pw_conv_wgrad_chunks(self.S, self.NP))
        self.echunks = int(lib.ppsci_pirate_embed_chunks(self.n))
        self.pB = torch.zeros((self.echunks, max(1, self.desc.d0 * self.half)), **self.f32)

    def _begin_reverse(self) -> None:
        """The reverse buffers exist (allocated on first use) and no sum is pending."""
        if not self._train_ready:
            self._alloc_train()
            self._train_ready = True
        self._pcall, self._psegs, self._pullbacks = 0, [], []

    def _pbuf(self, n: int, kind: str) -> torch.Tensor:
        """Partial-sum buffer of the pass' next producer: the same one, at the same address, in every pass."""
        if not self.batched:
            return self._scratch[kind][:n]
        i = self._pcall
        self._pcall += 1
        if i == len(self._pbufs):
            self._pbufs.append(torch.zeros(n, **self.f32))
        assert self._pbufs[i].numel() >= n
        return self._pbufs[i]

    def _sum(self, part: torch.Tensor, rows: int, cols: int, dst: torch.Tensor) -> None:
        if self.batched:
            self._psegs.append((part.data_ptr(), dst.data_ptr(), rows, cols))
        else:
            hp.reduce_rows(part, rows, cols, dst, False)

    def _flush_sums(self, like: torch.Tensor) -> None:
        hp.reduce_rows_multi(self._psegs, like)
        self._psegs = []
        if self._pullbacks:  # the trainable tensors behind the summed kernel-layout gradients, 16 layers per launch
            hp.linear_multi(self._pullbacks, True, like)
        self._pullbacks = []

    # ---- the plain stack
    def _stack_fwd(self, st: Stack, params, n1: int, n2: int) -> None:
        """st.X -> st.Y."""
        act, swish = L.ACT[st.act], st.act == "swish"
        y, fin = st.X, st.d_in
        for i, w in enumerate(st.widths):
            name = f"{st.pre}linears.{i}"
            self._dense(y, self._w(params, name), fin, w, st.Z[i], S=st.S)
            self._act(L.PIRATE_ACT, act, w, n1, n2, st.Z[i], self._t(params, name + ".bias"), st.A[i],
                      alpha=self._t(params, f"{st.pre}acts.{i}.beta") if swish else None)
            y, fin = st.A[i], w
        self._dense(y, self._w(params, st.pre + "last_fc"), fin, st.d_out, st.Y, S=st.S)

    def _stack_bwd(self, st: Stack, params, grad, n1: int, n2: int, wchunks: int, to_input: bool) -> torch.Tensor:
        """st.Ybar (adjoint of st.Y) -> the weight / bias / beta gradients of the stack; returns the adjoint of st.X, which
        is computed only when `to_input`."""
        act, swish, S, NP = L.ACT[st.act], st.act == "swish", st.S, self.NP
        fout = st.widths[-1]
        self._wgrad(st.A[-1], st.Ybar, fout, st.d_out, st.pre + "last_fc", params, grad, S, wchunks)
        ob = st.OB[: S * fout * NP]
        self._dense_t(st.Ybar, self._w(params, st.pre + "last_fc"), fout, st.d_out, ob, S=S)
        for i in range(len(st.widths) - 1, -1, -1):
            w, name = st.widths[i], f"{st.pre}linears.{i}"
            yin, fin = (st.A[i - 1], st.widths[i - 1]) if i > 0 else (st.X, st.d_in)
            zb = st.ZB[: S * w * NP]
            self._act_rev(L.PIRATE_ACT, act, w, n1, n2, st.Z[i], name + ".bias", ob, zb, params, grad,
                          alpha_name=f"{st.pre}acts.{i}.beta" if swish else None)
            self._wgrad(yin, zb, fin, w, name, params, grad, S, wchunks)
            if i > 0 or to_input:
                ob = st.OB[: S * fin * NP]
                self._dense_t(zb, self._w(params, name), fin, w, ob, S=S)
        return ob
