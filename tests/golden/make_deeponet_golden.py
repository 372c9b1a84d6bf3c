"""Generates tests/golden/deeponet.npz by executing the REFERENCE's own DeepONet, HEDeepONets and ChipDeepONets
(ppsci/arch/deeponet.py, he_deeponets.py, chip_deeponets.py, with mlp.py, activation.py and autodiff/ad.py) in float64
under the torch-backed paddle shim (tests/golden/_paddle_shim.py).

Per case: the named parameters in the reference's order with seeded values, the inputs, every output's value and its first
and pure second derivatives along each trunk key (ad.jacobian / ad.hessian), fixed random cotangents C and the gradient of
sum_{o, s} <C[o, s], stream s of output o> with respect to every parameter (zero for the parameters forward never reads).

    python tests/golden/make_deeponet_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

N = 203  # not a multiple of 16 nor of the 256-point workgroup

CASES = {
    # deeponet.yaml in small: m = 100 sensors, one trunk coordinate, G_y and G_yy
    "deeponet_tanh": dict(cls="DeepONet", order=2,
                          kw=dict(u_key="u", y_key="y", G_key="G", num_loc=100, num_features=16, branch_num_layers=2,
                                  trunk_num_layers=2, branch_hidden_size=32, trunk_hidden_size=32,
                                  branch_activation="tanh", trunk_activation="tanh"),
                          branch={"u": 100}, trunk=("y",)),
    # heat_exchanger.yaml in small: swish everywhere, three outputs, first order in x and t
    "he_swish": dict(cls="HEDeepONets", order=1,
                     kw=dict(heat_input_keys=("qm_h",), cold_input_keys=("qm_c",), trunk_input_keys=("x", "t"),
                             output_keys=("T_h", "T_c", "T_w"), heat_num_loc=1, cold_num_loc=1, num_features=8,
                             branch_num_layers=2, trunk_num_layers=3, branch_hidden_size=32, trunk_hidden_size=32,
                             branch_activation="swish", trunk_activation="swish"),
                     branch={"qm_h": 1, "qm_c": 1}, trunk=("x", "t")),
    # chip_heat.yaml in small: J = 3, T_xx + T_yy
    "chip_swish": dict(cls="ChipDeepONets", order=2,
                       kw=dict(branch_input_keys=("u",), BCtype_input_keys=("bctype",), BC_input_keys=("bc",),
                               trunk_input_keys=("x", "y"), output_keys=("T",), num_loc=12, bctype_loc=1, BC_num_loc=6,
                               num_features=12, branch_num_layers=2, BC_num_layers=2, trunk_num_layers=2,
                               branch_hidden_size=32, BC_hidden_size=16, trunk_hidden_size=32, branch_activation="swish",
                               BC_activation="sin", trunk_activation="swish"),
                       branch={"u": 12, "bctype": 1, "bc": 6}, trunk=("x", "y")),
}


def draw(named, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for name, p in named:
        shp = tuple(p.shape)
        if name.endswith("beta"):
            v = rng.uniform(0.6, 1.6, shp)
        elif name.endswith("bias") or name == "b":
            v = rng.normal(0.0, 0.1, shp)
        else:
            fin, fout = shp
            v = rng.normal(0.0, np.sqrt(2.0 / (fin + fout)), shp)
        out[name] = np.asarray(v).astype(np.float32).astype(np.float64)
    return out


def main():
    import importlib

    import _paddle_shim as S

    mods = S.import_hotpath()
    ad = mods["ad"]
    paddle = sys.modules["paddle"]
    paddle.einsum = torch.einsum
    paddle.sum = lambda x, axis=None, keepdim=False: torch.sum(x, dim=axis, keepdim=keepdim)
    paddle.reshape = lambda x, shape: torch.reshape(x, tuple(shape))
    classes = {n: getattr(importlib.import_module(f"ppsci.arch.{f}"), n)
               for n, f in (("DeepONet", "deeponet"), ("HEDeepONets", "he_deeponets"), ("ChipDeepONets", "chip_deeponets"))}
    out = {}
    for ci, (name, c) in enumerate(CASES.items()):
        model = classes[c["cls"]](**c["kw"])
        named = list(model.named_parameters())
        vals = draw(named, 700 + ci)
        with torch.no_grad():
            for n, p in named:
                p.copy_(torch.tensor(vals[n]))
        rng = np.random.default_rng(7000 + ci)
        data = {}
        for k, m in c["branch"].items():
            data[k] = torch.tensor(rng.uniform(-1, 1, (N, m)).astype(np.float32).astype(np.float64))
        for k in c["trunk"]:
            data[k] = torch.tensor(rng.uniform(0, 1, (N, 1)).astype(np.float32).astype(np.float64), requires_grad=True)
        outs = model(data)
        okeys = list(model.output_keys)
        streams = []  # [n_out][S][N]: value, d/dk for k in trunk, d2/dk2 for k in trunk (order 2)
        for o in okeys:
            g = outs[o]
            rows = [g]
            rows += [ad.jacobian(g, data[k]) for k in c["trunk"]]
            if c["order"] == 2:
                rows += [ad.hessian(g, data[k]) for k in c["trunk"]]
            streams.append(rows)
        S_ = len(streams[0])
        cot = rng.standard_normal((len(okeys), S_, N)) * 0.1
        total = 0.0
        for o in range(len(okeys)):
            for s in range(S_):
                total = total + (streams[o][s][:, 0] * torch.tensor(cot[o, s])).sum()
        params = [p for _, p in named]
        grads = torch.autograd.grad(total, params, allow_unused=True)
        ad.clear()
        out[f"{name}/names"] = np.array([n for n, _ in named])
        for n, p in named:
            out[f"{name}/param/{n}"] = vals[n]
        for (n, _), g in zip(named, grads):
            out[f"{name}/grad/{n}"] = np.zeros(vals[n].shape) if g is None else g.detach().numpy()
        for k, v in data.items():
            out[f"{name}/in/{k}"] = v.detach().numpy()
        out[f"{name}/U"] = np.array([[r.detach().numpy()[:, 0] for r in rows] for rows in streams])
        out[f"{name}/cot"] = cot
        print(name, len(named), "params", np.array(out[f"{name}/U"]).shape)
    np.savez_compressed(os.path.join(HERE, "deeponet.npz"), **out)


if __name__ == "__main__":
    main()
