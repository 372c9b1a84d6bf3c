"""ppsci.arch.DeepONet, HEDeepONets and ChipDeepONets (/root/reference/ppsci/arch/deeponet.py, he_deeponets.py,
chip_deeponets.py) on HIP kernels, layer by layer.

With p = num_features, n_out outputs, F = p * n_out and J branch nets (1 DeepONet, 2 HE: heat / cold, 3 Chip: branch, BC,
BCtype):

    B_j = branch_j(u_j)                  plain MLP on a key of m_j columns, value only (it does not see the trunk inputs)
    A   = trunk_act(trunk(y))            MLP on the trunk keys, on Taylor streams (value, n1 first, n2 pure second)
    G_o = sum_{k < p} prod_j B_j[o p + k] * A[o p + k] + b[o]

Every dense layer is one MFMA GEMM (`ppsci_pw_conv`) over all streams ([S, C, NP] = its [B, C, P]); bias + activation and
their reverse are `ppsci_pirate_act_*` (mode ACT, swish with its trainable beta included); the branch keys reach the GEMMs
through `ppsci_onet_pack`; the product and its reverse, with the trunk activation's Taylor propagation, are
`ppsci_onet_head_fwd/_bwd` (csrc/pirate.hip).  A derivative stream of G runs along the trunk keys only.

Trainable tensors: one flat fp32 device buffer, in the reference's `named_parameters()` order and with its names (a layer's
own parameters first, then its sublayers in registration order): b, <branch>.linears.i.{weight,bias}, <branch>.acts.i.beta
(swish), <branch>.last_fc.*, ..., trunk_net.*, trunk_act.beta and the activations the reference registers but never calls
(heat_act / cold_act, bc_act / branch_act).  Those have no gradient: Adam leaves them bit-identical.

Not available (raise NotImplementedError): weight norm, skip connections, activations other than tanh, silu, sigmoid, sin,
cos, gelu and swish, derivative order > 2, derivatives with respect to a branch key, input / output transforms."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from .. import hotpath as hp
from . import activation as act_mod
from .layer_by_layer import FlatParamArch, LayerExec, LayerLayout, Stack, _p, _sp

ONET_ACTS = ("tanh", "silu", "sigmoid", "sin", "cos", "gelu", "swish")


def _widths(num_layers, hidden_size) -> List[int]:
    if isinstance(hidden_size, (tuple, list)):
        if num_layers is not None:
            raise ValueError("num_layers should be None when hidden_size is specified")  # mlp.py:204-208
        return [int(h) for h in hidden_size]
    if not isinstance(num_layers, int):
        raise ValueError("num_layers should be an int when hidden_size is an int")  # mlp.py:209-213
    return [int(hidden_size)] * num_layers


class _Sub:
    """One plain mlp.MLP of the operator net: names, shapes and launch sequence (forward / reverse at S streams)."""

    def __init__(self, prefix: str, keys: Tuple[str, ...], d_in: int, widths: List[int], activation: str, d_out: int,
                 skip_connection: bool, weight_norm: bool):
        if skip_connection:
            raise NotImplementedError(f"{prefix}: skip_connection has no layer-by-layer kernel path")
        if weight_norm:
            raise NotImplementedError(f"{prefix}: weight_norm has no layer-by-layer kernel path")
        if not widths:
            raise NotImplementedError(f"{prefix}: an MLP without hidden layers")
        act = act_mod.get_activation(activation)
        if act not in ONET_ACTS:
            raise NotImplementedError(f"{prefix}: activation {activation!r}; the stream kernels carry {ONET_ACTS}")
        self.prefix, self.keys, self.d_in, self.widths, self.act, self.d_out = prefix, tuple(keys), int(d_in), widths, act, int(d_out)

    def shapes(self) -> List[Tuple[str, Tuple[int, ...]]]:
        out, fin = [], self.d_in
        for i, w in enumerate(self.widths):
            out += [(f"{self.prefix}.linears.{i}.weight", (fin, w)), (f"{self.prefix}.linears.{i}.bias", (w,))]
            fin = w
        if self.act == "swish":
            out += [(f"{self.prefix}.acts.{i}.beta", ()) for i in range(len(self.widths))]
        return out + [(f"{self.prefix}.last_fc.weight", (fin, self.d_out)), (f"{self.prefix}.last_fc.bias", (self.d_out,))]


def _act_shapes(name: str, activation: str) -> List[Tuple[str, Tuple[int, ...]]]:
    return [(f"{name}.beta", ())] if act_mod.get_activation(activation) == "swish" else []


class _OnetBase(FlatParamArch):
    """Shapes, initialisation and executor inputs of the three operator nets."""

    def _setup(self, subs: List[_Sub], trunk: _Sub, trunk_act: str, act_params: List[Tuple[str, Tuple[int, ...]]],
               n_out: int, p: int, use_bias: bool):
        self.subs, self.trunk, self.n_out, self.p, self.use_bias = subs, trunk, int(n_out), int(p), bool(use_bias)
        if len(self.output_keys) > L.MAX_OUT or len(trunk.keys) > L.MAX_IN:
            raise NotImplementedError(f"at most {L.MAX_IN} trunk inputs / {L.MAX_OUT} outputs")
        self.trunk_act = act_mod.get_activation(trunk_act)
        if self.trunk_act not in ONET_ACTS:
            raise NotImplementedError(f"trunk_act {trunk_act!r}: the head kernel carries {ONET_ACTS}")
        self.trunk_keys = tuple(trunk.keys)
        self.branch_keys = tuple(k for s in subs for k in s.keys)
        # columns of every branch key: a net on one key reads input_dim columns of it; a net on several keys, one each
        self.branch_cols = {k: (s.d_in if len(s.keys) == 1 else 1) for s in subs for k in s.keys}
        for s in subs:
            if len(s.keys) > 1 and len(s.keys) != s.d_in:
                raise NotImplementedError(f"{s.prefix}: several input keys whose columns add up to input_dim = {s.d_in}: "
                                          "only one key of input_dim columns, or input_dim one-column keys")
        shapes: List[Tuple[str, Tuple[int, ...]]] = [("b", (self.n_out,))] if use_bias else []
        for s in getattr(self, "_order_subs", subs):  # registration order of the reference's sub-layers
            shapes += s.shapes()
        shapes += trunk.shapes()
        shapes += _act_shapes("trunk_act", trunk_act) + act_params
        self._store(shapes)
        self._init_parameters()
        self.layout = OnetLayout(self)
        # parameters the forward never reads (unused registered activations): no gradient, never moved by Adam
        self.unused = [n for n, _ in act_params]

    def _init_parameters(self):
        """nn.Linear: Xavier-uniform weight, zero bias (from numpy's global RNG, ppsci.utils.misc.set_random_seed);
        Swish beta = 1 (activation.py:50-55); b = 0 (deeponet.py:123-127)."""
        t = self._byname
        for name, shp in self._shapes:
            if name.endswith(".weight"):
                fin, fout = shp
                lim = math.sqrt(6.0 / (fin + fout))
                t[name].copy_(torch.from_numpy(np.random.uniform(-lim, lim, size=shp).astype(np.float32)))
            elif name.endswith(".beta"):
                t[name].fill_(1.0)
            else:
                t[name].zero_()

    # ---- executors
    def make_exec(self, dirs: Sequence[Sequence[float]], n2: int, n: int, train: bool = True) -> "OnetExec":
        """Executor at 1 + len(dirs) + n2 streams: `dirs` are direction vectors over the TRUNK keys (derivatives along a
        branch key are outside this model)."""
        return self._make_exec(hp.StreamSpec([list(map(float, d)) for d in dirs], int(n2)), int(n), train=train)

    def _make_exec(self, spec, n, inputs=None, train=True, branch=None):
        return OnetExec(self, spec, n, inputs, branch, train)

    def _rows(self, ins: Dict[str, torch.Tensor]) -> int:
        n = int(ins[self.trunk_keys[0]].shape[0])
        for k in self.branch_keys:
            if int(ins[k].shape[0]) != n:
                raise ValueError(f"branch key {k!r} has {int(ins[k].shape[0])} rows, the trunk keys {n}")
        return n

    def _check_transforms(self) -> None:
        if self._input_transform is not None or self._output_transform is not None:
            raise NotImplementedError(f"{type(self).__name__} with a registered input / output transform")


class DeepONet(_OnetBase):
    """deeponet.py:28-154."""

    def __init__(self, u_key: str, y_key: str, G_key: str, num_loc: int, num_features: int, branch_num_layers: int,
                 trunk_num_layers: int, branch_hidden_size: Union[int, Tuple[int, ...]],
                 trunk_hidden_size: Union[int, Tuple[int, ...]], branch_skip_connection: bool = False,
                 trunk_skip_connection: bool = False, branch_activation: str = "tanh", trunk_activation: str = "tanh",
                 branch_weight_norm: bool = False, trunk_weight_norm: bool = False, use_bias: bool = True):
        super().__init__()
        self.u_key, self.y_key = u_key, y_key
        self.input_keys, self.output_keys = (u_key, y_key), (G_key,)
        branch = _Sub("branch_net", (u_key,), num_loc, _widths(branch_num_layers, branch_hidden_size), branch_activation,
                      num_features, branch_skip_connection, branch_weight_norm)
        trunk = _Sub("trunk_net", (y_key,), 1, _widths(trunk_num_layers, trunk_hidden_size), trunk_activation, num_features,
                     trunk_skip_connection, trunk_weight_norm)
        self._setup([branch], trunk, trunk_activation, [], 1, num_features, use_bias)


class HEDeepONets(_OnetBase):
    """he_deeponets.py:26-197: heat and cold branch nets, three outputs on slices o*p:(o+1)*p of the features."""

    def __init__(self, heat_input_keys: Tuple[str, ...], cold_input_keys: Tuple[str, ...], trunk_input_keys: Tuple[str, ...],
                 output_keys: Tuple[str, ...], heat_num_loc: int, cold_num_loc: int, num_features: int,
                 branch_num_layers: int, trunk_num_layers: int, branch_hidden_size: Union[int, Tuple[int, ...]],
                 trunk_hidden_size: Union[int, Tuple[int, ...]], branch_skip_connection: bool = False,
                 trunk_skip_connection: bool = False, branch_activation: str = "tanh", trunk_activation: str = "tanh",
                 branch_weight_norm: bool = False, trunk_weight_norm: bool = False, use_bias: bool = True):
        super().__init__()
        self.trunk_input_keys, self.heat_input_keys, self.cold_input_keys = tuple(trunk_input_keys), tuple(heat_input_keys), tuple(cold_input_keys)
        self.input_keys = self.trunk_input_keys + self.heat_input_keys + self.cold_input_keys
        self.output_keys = tuple(output_keys)
        if len(self.output_keys) != 3:
            raise ValueError("HEDeepONets has three outputs (he_deeponets.py:166-193)")
        self.num_features = num_features
        F = num_features * 3
        bw = _widths(branch_num_layers, branch_hidden_size)
        heat = _Sub("heat_net", self.heat_input_keys, heat_num_loc, bw, branch_activation, F, branch_skip_connection, branch_weight_norm)
        cold = _Sub("cold_net", self.cold_input_keys, cold_num_loc, list(bw), branch_activation, F, branch_skip_connection,
                    branch_weight_norm)
        trunk = _Sub("trunk_net", self.trunk_input_keys, len(self.trunk_input_keys), _widths(trunk_num_layers, trunk_hidden_size),
                     trunk_activation, F, trunk_skip_connection, trunk_weight_norm)
        self._setup([heat, cold], trunk, trunk_activation,
                    _act_shapes("heat_act", branch_activation) + _act_shapes("cold_act", branch_activation), 3, num_features,
                    use_bias)


class ChipDeepONets(_OnetBase):
    """chip_deeponets.py:26-214: branch, BC and BCtype nets, one output."""

    def __init__(self, branch_input_keys: Tuple[str, ...], BCtype_input_keys: Tuple[str, ...], BC_input_keys: Tuple[str, ...],
                 trunk_input_keys: Tuple[str, ...], output_keys: Tuple[str, ...], num_loc: int, bctype_loc: int,
                 BC_num_loc: int, num_features: int, branch_num_layers: int, BC_num_layers: int, trunk_num_layers: int,
                 branch_hidden_size: Union[int, Tuple[int, ...]], BC_hidden_size: Union[int, Tuple[int, ...]],
                 trunk_hidden_size: Union[int, Tuple[int, ...]], branch_skip_connection: bool = False,
                 BC_skip_connection: bool = False, trunk_skip_connection: bool = False, branch_activation: str = "tanh",
                 BC_activation: str = "tanh", trunk_activation: str = "tanh", branch_weight_norm: bool = False,
                 BC_weight_norm: bool = False, trunk_weight_norm: bool = False, use_bias: bool = True):
        super().__init__()
        self.trunk_input_keys, self.branch_input_keys = tuple(trunk_input_keys), tuple(branch_input_keys)
        self.BCtype_input_keys, self.BC_input_keys = tuple(BCtype_input_keys), tuple(BC_input_keys)
        self.input_keys = self.trunk_input_keys + self.branch_input_keys + self.BC_input_keys + self.BCtype_input_keys
        self.output_keys = tuple(output_keys)
        if len(self.output_keys) != 1:
            raise ValueError("ChipDeepONets has one output (chip_deeponets.py:207-209)")
        bcw = _widths(BC_num_layers, BC_hidden_size)
        branch = _Sub("branch_net", self.branch_input_keys, num_loc, _widths(branch_num_layers, branch_hidden_size),
                      branch_activation, num_features, branch_skip_connection, branch_weight_norm)
        bctype = _Sub("BCtype_net", self.BCtype_input_keys, bctype_loc, bcw, BC_activation, num_features, BC_skip_connection,
                      BC_weight_norm)
        bc = _Sub("BC_net", self.BC_input_keys, BC_num_loc, list(bcw), BC_activation, num_features, BC_skip_connection,
                  BC_weight_norm)
        trunk = _Sub("trunk_net", self.trunk_input_keys, len(self.trunk_input_keys), _widths(trunk_num_layers, trunk_hidden_size),
                     trunk_activation, num_features, trunk_skip_connection, trunk_weight_norm)
        self._order_subs = [branch, bctype, bc]  # registration order (chip_deeponets.py:124-169)
        self._setup([branch, bc, bctype], trunk, trunk_activation,
                    _act_shapes("bc_act", BC_activation) + _act_shapes("branch_act", branch_activation), 1, num_features,
                    use_bias)


class OnetLayout(LayerLayout):
    """The layout of an operator net: `d_raw` counts the trunk keys only -- the constraint's input columns and derivative
    directions; the branch keys reach the executor as [N, m] tensors bound by compile.CompiledConstraint (`with_branch`),
    never through the epilogue program's input table."""

    def __init__(self, model: "_OnetBase", branch: Optional[Dict[str, torch.Tensor]] = None):
        super().__init__(model, len(model.trunk_keys), model.n_out, len(model.trunk.widths), max(model.trunk.widths))
        self.branch = branch

    def with_branch(self, branch: Dict[str, torch.Tensor]) -> "OnetLayout":
        return OnetLayout(self.model, branch)

    def make_exec(self, spec: hp.StreamSpec, n: int, inputs) -> "OnetExec":
        if self.branch is None:
            raise RuntimeError("the branch-key tensors of the constraint are not bound (compile.CompiledConstraint)")
        return self.model._make_exec(spec, n, inputs, branch=self.branch)


class OnetExec(LayerExec):
    """Buffers and launch sequence of one (operator net, stream set, batch size): the branch nets are plain stacks at
    S = 1, the trunk net one at all streams; forward fills U [n_out * S, N] (pirate_out_fwd's layout)."""

    def __init__(self, model: _OnetBase, spec: hp.StreamSpec, n: int, inputs: Optional[Sequence[torch.Tensor]] = None,
                 branch: Optional[Dict[str, torch.Tensor]] = None, train: bool = True):
        """inputs: the trunk keys' [N] device columns, read in place (engine.FusedConstraint's); branch: key -> [N, m]
        device tensor, packed at every forward (compile.CompiledConstraint's).  Without them the executor owns both and
        set_inputs fills them."""
        dt = len(model.trunk_keys)
        if any(len(v) != dt for v in spec.dirs):
            raise NotImplementedError(f"{type(model).__name__}: a derivative direction must span the trunk keys "
                                      f"{model.trunk_keys} only (derivatives along a branch key are outside this model)")
        super().__init__(model, spec, n, inputs, type(model).__name__, model.trunk_keys, dt)  # no period / Fourier embedding
        stack = lambda s, S: Stack(s.prefix + ".", s.d_in, s.widths, s.d_out, s.act, S, self.NP, self.f32)  # noqa: E731
        self.branches = [(s, stack(s, 1)) for s in model.subs]
        self.trunk = stack(model.trunk, self.S)
        self.branch_in: Dict[str, torch.Tensor] = {}
        for k, c in model.branch_cols.items():
            v = branch.get(k) if branch is not None else None
            if v is None:
                v = torch.zeros((self.n, c), **self.f32)
            elif tuple(v.shape) != (self.n, c) or not v.is_contiguous() or v.dtype != torch.float32:
                raise ValueError(f"branch key {k!r}: expected a contiguous float32 [{self.n}, {c}] tensor")
            self.branch_in[k] = v
        h = self.hdesc = L.OnetHeadDesc()
        h.J, h.p, h.n_out, h.n1, h.n2, h.act, h.N, h.NP = len(model.subs), model.p, model.n_out, self.n1, self.n2, \
            L.ACT[model.trunk_act], self.n, self.NP
        self._B_ptrs = (C.c_void_p * L.ONET_MAX_J)(*[b.Y.data_ptr() for _, b in self.branches])
        if train:
            self._begin_reverse()

    def _alloc_train(self):
        lib = L.lib()
        m, F = self.model, self.model.p * self.model.n_out
        for st in [self.trunk] + [b for _, b in self.branches]:
            st.alloc_train()
        self._Bbar_ptrs = (C.c_void_p * L.ONET_MAX_J)(*[b.Ybar.data_ptr() for _, b in self.branches])
        self.hchunks = int(lib.ppsci_onet_head_chunks(self.NP))
        self.achunks = int(lib.ppsci_pirate_act_chunks(self.NP))
        self.p_tb = torch.zeros(self.hchunks * F, **self.f32)
        self.p_bb = torch.zeros(len(self.branches) * self.hchunks * F, **self.f32)
        self.p_beta = torch.zeros(F * self.hchunks, **self.f32)
        self.p_b = torch.zeros(self.hchunks * m.n_out, **self.f32)

    # ---- inputs
    def set_inputs(self, x: Dict[str, torch.Tensor]) -> None:
        """Copies a batch into the executor's input buffers. Trunk keys: [N] or [N, 1]; branch keys: [N, m] row-major."""
        super().set_inputs(x)
        for k, dst in self.branch_in.items():
            v = x[k]
            if v.shape[0] != self.n or v.numel() != dst.numel():
                raise ValueError(f"branch key {k!r}: expected [{self.n}, {dst.shape[1]}], got shape {tuple(v.shape)}")
            dst.copy_(v.reshape(dst.shape))

    def _pack(self) -> None:
        """Branch keys [N, m] -> the planar [m][NP] input block of their branch net (the concat of mlp.py:314)."""
        lib = L.lib()
        for s, b in self.branches:
            c0 = 0
            for k in s.keys:
                v = self.branch_in[k]
                mcol = int(v.shape[1])
                L.check(lib.ppsci_onet_pack(mcol, self.n, self.NP, _p(v), C.c_void_p(b.X.data_ptr() + 4 * c0 * self.NP),
                                            _sp(b.X)))
                c0 += mcol

    def _head_args(self, params):
        bb = (C.c_void_p * L.ONET_MAX_J)(*[self._t(params, f"{s.prefix}.last_fc.bias").data_ptr() for s, _ in self.branches])
        beta = self._t(params, "trunk_act.beta") if self.model.trunk_act == "swish" else None
        return bb, beta

    # ---- forward / reverse
    def forward(self, params: torch.Tensor, Urows: torch.Tensor, train: bool = True) -> None:
        """Urows [n_out * S, N].  The forward keeps the same buffers whether `train` or not, because the reverse recomputes
        what it needs from them."""
        m, lib = self.model, L.lib()
        assert Urows.numel() == m.n_out * self.S * self.n
        self._pack()
        for _, b in self.branches:
            self._stack_fwd(b, params, 0, 0)
        t = self.trunk
        self._embed_fwd(params, t.X)
        self._stack_fwd(t, params, self.n1, self.n2)
        bb, beta = self._head_args(params)
        L.check(lib.ppsci_onet_head_fwd(C.byref(self.hdesc), _p(t.Y), _p(self._t(params, "trunk_net.last_fc.bias")),
                                        self._B_ptrs, bb, _p(beta), _p(self._t(params, "b")) if m.use_bias else None,
                                        _p(Urows), _sp(Urows)))

    def _sub_bwd(self, st: Stack, params, grad, n1: int, n2: int) -> None:
        """The sub-net's gradients from st.Ybar (no input adjoint)."""
        self._stack_bwd(st, params, grad, n1, n2, int(L.lib().ppsci_pw_conv_wgrad_chunks(st.S, self.NP)), False)

    def backward(self, params: torch.Tensor, Ubar_rows: torch.Tensor, grad: torch.Tensor) -> None:
        """The unused activation parameters get 0."""
        self._begin_reverse()
        m, lib = self.model, L.lib()
        grad = grad.view(-1)
        assert Ubar_rows.numel() == m.n_out * self.S * self.n and grad.numel() == m.n_params
        for name in m.unused:
            self._t(grad, name).zero_()
        t, F = self.trunk, m.p * m.n_out
        bb, beta = self._head_args(params)
        L.check(lib.ppsci_onet_head_bwd(C.byref(self.hdesc), _p(t.Y), _p(self._t(params, "trunk_net.last_fc.bias")),
                                        self._B_ptrs, bb, _p(beta), _p(Ubar_rows), _p(t.Ybar), self._Bbar_ptrs, _p(self.p_tb),
                                        _p(self.p_bb), _p(self.p_beta), _p(self.p_b) if m.use_bias else None, _sp(t.Ybar)))
        self._sum(self.p_tb, self.hchunks, F, self._t(grad, "trunk_net.last_fc.bias"))
        for j, (s, _) in enumerate(self.branches):
            self._sum(self.p_bb[j * self.hchunks * F:], self.hchunks, F, self._t(grad, f"{s.prefix}.last_fc.bias"))
        if m.trunk_act == "swish":
            self._sum(self.p_beta, F * self.hchunks, 1, self._t(grad, "trunk_act.beta"))
        if m.use_bias:
            self._sum(self.p_b, self.hchunks, m.n_out, self._t(grad, "b"))
        self._sub_bwd(t, params, grad, self.n1, self.n2)
        for _, b in self.branches:
            self._sub_bwd(b, params, grad, 0, 0)
        self._flush_sums(t.Ybar)
