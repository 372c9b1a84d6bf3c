"""Generates tests/golden/uno.npz by executing the REFERENCE's own UNO code (/root/reference/ppsci/arch/unonet.py on
fno_block.py: FNOBlocks with output_scaling_factor, FactorizedSpectralConv.forward incl. irfftn(s=), resample, skip_connection,
DomainPadding) in this container, PaddlePaddle replaced by the torch-backed shim of make_fno_golden.py, in float64.

    python tests/golden/make_uno_golden.py

Per case: explicit parameters (drawn here, under the names of paddlescience_amd.arch.uno), the input batch, the network output and
d(mean squared output error)/d(parameters) through the reference's graph."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _paddle_shim as S  # noqa: E402
import make_fno_golden as G  # noqa: E402

D = torch.float64

from uno_cases import CASES  # noqa: E402


def install():
    fno_block, _ = G.install_fno_shim()
    F = sys.modules["paddle.nn.functional"]
    nn = sys.modules["paddle.nn"]

    def interpolate(x, size=None, scale_factor=None, mode="nearest", align_corners=False, **k):
        return torch.nn.functional.interpolate(x, size=tuple(size) if isinstance(size, (list, tuple)) else size,
                                               scale_factor=scale_factor, mode=mode, align_corners=align_corners)

    F.interpolate = interpolate
    fno_block.F.interpolate = interpolate

    class LayerDict(S.Layer):
        def __init__(self, d=None):
            super().__init__()
            self._d = {}
            for k, v in (d or {}).items():
                self[k] = v

        def __setitem__(self, k, v):
            self._d[k] = v
            self._subs[k] = v

        def __getitem__(self, k):
            return self._d[k]

    nn.LayerDict = LayerDict
    # validate_scaling_factor (fno_block.py:446-462) accepts a nested scaling factor only as a list of omegaconf ListConfig --
    # what the hydra config of examples/neuraloperator/train_uno.py hands over; plain nested lists come back as None (no
    # rescaling at all).  The fixtures follow the configured behaviour: python lists stand in for ListConfig here.
    import types

    sys.modules["omegaconf"].listconfig = types.SimpleNamespace(ListConfig=list)
    unonet = importlib.import_module("ppsci.arch.unonet")
    return fno_block, unonet


def shapes_of(c, in_channels=3, out_channels=1):
    n = len(c["outs"])
    skips = c["skips"] if c["skips"] is not None else {n - i - 1: i for i in range(n // 2)}
    sh = {"lifting.fcs.0.weight": (c["lift"], in_channels, 1, 1), "lifting.fcs.0.bias": (c["lift"],),
          "lifting.fcs.1.weight": (c["hidden"], c["lift"], 1, 1), "lifting.fcs.1.bias": (c["hidden"],)}
    prev = c["hidden"]
    for i in range(n):
        if i in skips:
            prev += c["outs"][skips[i]]
        co = c["outs"][i]
        mx, my = c["modes"][i][0], c["modes"][i][1] // 2 + 1
        sh[f"fno_blocks.{i}.convs.0.weight_real"] = (prev, co, mx, my)
        sh[f"fno_blocks.{i}.convs.0.weight_imag"] = (prev, co, mx, my)
        sh[f"fno_blocks.{i}.convs.0.bias"] = (co, 1, 1)
        if c.get("fno_skip", "linear") == "linear":  # (identity: the skip branch has no parameters)
            sh[f"fno_blocks.{i}.fno_skips.0.weight"] = (co, prev, 1, 1)
        if c["norm"]:
            sh[f"fno_blocks.{i}.norm.0.weight"] = (co,)
            sh[f"fno_blocks.{i}.norm.0.bias"] = (co,)
        if i in skips.values():
            sh[f"horizontal_skips.{i}.weight"] = (co, co, 1, 1)
        prev = co
    sh["projection.fcs.0.weight"] = (c["proj"], prev, 1, 1)
    sh["projection.fcs.0.bias"] = (c["proj"],)
    sh["projection.fcs.1.weight"] = (out_channels, c["proj"], 1, 1)
    sh["projection.fcs.1.bias"] = (out_channels,)
    return sh, skips


def leaves_of(model, c, skips):
    """name -> the reference model's leaf tensor (the spectral biases are [n_layers = 1, C, 1, 1] parameters: index 0)."""
    out = {}
    for name, mlp in (("lifting", model.lifting), ("projection", model.projection)):
        for i, fc in enumerate(mlp.fcs):
            out[f"{name}.fcs.{i}.weight"], out[f"{name}.fcs.{i}.bias"] = fc.weight, fc.bias
    for i, blk in enumerate(model.fno_blocks):
        out[f"fno_blocks.{i}.convs.0.weight_real"] = blk.convs.weight[0].real
        out[f"fno_blocks.{i}.convs.0.weight_imag"] = blk.convs.weight[0].imag
        out[f"fno_blocks.{i}.convs.0.bias"] = blk.convs.bias
        if c.get("fno_skip", "linear") == "linear":
            out[f"fno_blocks.{i}.fno_skips.0.weight"] = blk.fno_skips[0].weight
        if c["norm"]:
            out[f"fno_blocks.{i}.norm.0.weight"], out[f"fno_blocks.{i}.norm.0.bias"] = blk.norm[0].weight, blk.norm[0].bias
        if i in skips.values():
            out[f"horizontal_skips.{i}.weight"] = model.horizontal_skips[str(i)].weight
    return out


def main():
    fno_block, unonet = install()
    out = {}
    for cname, c in CASES.items():
        rng = np.random.default_rng(len(cname) * 1327)
        n = len(c["outs"])
        model = unonet.UNONet(("x",), ("y",), 3, 1, c["hidden"], lifting_channels=c["lift"], projection_channels=c["proj"],
                              n_layers=n, uno_out_channels=c["outs"], uno_n_modes=c["modes"], uno_scalings=c["scal"],
                              horizontal_skips_map=c["skips"], norm=c["norm"], domain_padding=c["pad"],
                              domain_padding_mode=c["pad_mode"], fft_norm=c["fft_norm"], fno_skip=c.get("fno_skip", "linear"))
        shapes, skips = shapes_of(c)
        leaves = leaves_of(model, c, skips)
        assert set(leaves) == set(shapes), set(leaves) ^ set(shapes)
        P = {}
        for k, sh in shapes.items():
            fan = max(1, int(np.prod(sh[1:])) if len(sh) > 1 else 1)
            if "weight_" in k:
                scale = (2.0 / (sh[0] + sh[1])) ** 0.5
            else:
                scale = 0.5 if k.endswith("bias") else 1.0 / np.sqrt(fan)
            v = rng.standard_normal(sh) * scale
            if ".norm." in k and k.endswith("weight"):
                v = 1.0 + 0.2 * rng.standard_normal(sh)
            P[k] = torch.tensor(v.astype(np.float32).astype(np.float64))
        with torch.no_grad():
            for k, leaf in leaves.items():
                if k.endswith("convs.0.bias"):
                    leaf[0].copy_(P[k])
                else:
                    leaf.copy_(P[k])
        B, H, W = c["B"], c["H"], c["W"]
        x = torch.tensor(rng.standard_normal((B, 3, H, W)).astype(np.float32).astype(np.float64))
        y = model({"x": x})["y"]
        tgt = torch.tensor(rng.standard_normal(tuple(y.shape)).astype(np.float32).astype(np.float64))
        loss = ((y - tgt) ** 2).mean()
        names = list(leaves)
        grads = torch.autograd.grad(loss, [leaves[k] for k in names])
        for k, g in zip(names, grads):
            out[f"{cname}/grad/{k}"] = (g[0] if k.endswith("convs.0.bias") else g).numpy()
        for k, v in P.items():
            out[f"{cname}/param/{k}"] = v.numpy()
        out[f"{cname}/x"], out[f"{cname}/target"], out[f"{cname}/y"] = x.numpy(), tgt.numpy(), y.detach().numpy()
        out[f"{cname}/loss"] = np.asarray(float(loss.detach()))
        print(cname, "y", tuple(y.shape), "loss", float(loss.detach()))
    np.savez_compressed(os.path.join(HERE, "uno.npz"), **out)
    print("wrote", os.path.join(HERE, "uno.npz"), len(out), "arrays")


if __name__ == "__main__":
    main()
