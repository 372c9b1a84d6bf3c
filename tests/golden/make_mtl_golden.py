"""Generates tests/golden/mtl.npz by executing the REFERENCE's own PCGrad._refine_grads (ppsci/loss/mtl/pcgrad.py:94-120) and
Relobralo.__call__ (ppsci/loss/mtl/relobralo.py:90-127) in float64 under the torch-backed paddle shim.

  pcgrad/G [3, P], pcgrad/orders [6, 3], pcgrad/out [6, P]: fixed gradient vectors of a two-Linear model (3 -> 5 -> 2, P = 32), and
      for each of the six orders the flat sum of the projected gradients when the list is handed over in that order (what
      PCGrad.backward does after its shuffle); the vectors conflict pairwise, so the order matters.
  relobralo/<case>/losses [6, 3], lmbda [6, 3], total [6], losses_init [3], losses_prev [3]: six steps of a fixed loss sequence
      at beta in {0, 1} (the two values at which paddle.bernoulli is deterministic) and tau in {1.0, 0.1}.

    python tests/golden/make_mtl_golden.py
"""
import importlib
import itertools
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def install():
    """The shim + the few paddle calls of the two aggregators it does not carry (patched here, the shim stays as it is)."""
    import _paddle_shim as S
    import _ref_import as RI

    paddle = S.install()
    f64 = dict(dtype=S.DTYPE)
    paddle.zeros = lambda shape, dtype=None: torch.zeros(tuple(shape), **f64)
    paddle.ones = lambda shape, dtype=None: torch.ones(tuple(shape), **f64)
    paddle.sum = torch.sum
    paddle.stack = lambda xs, axis=0: torch.stack(list(xs), dim=axis)
    paddle.reshape = lambda x, shape: torch.reshape(x, tuple(shape))
    paddle.bernoulli = torch.bernoulli
    paddle.assign = lambda src, dst: dst.copy_(src)
    S.Layer.register_buffer = lambda self, name, t: object.__setattr__(self, name, t)
    pkg = types.ModuleType("ppsci.loss.mtl")
    pkg.__path__ = [os.path.join(RI.REF, "ppsci", "loss", "mtl")]
    sys.modules["ppsci.loss.mtl"] = pkg
    pkg.base = importlib.import_module("ppsci.loss.mtl.base")
    return S, importlib.import_module("ppsci.loss.mtl.pcgrad"), importlib.import_module("ppsci.loss.mtl.relobralo")


def pcgrad_vectors(P):
    rng = np.random.default_rng(21)
    g0 = rng.standard_normal(P)
    e1 = 0.5 * rng.standard_normal(P)
    g1 = -0.5 * g0 + e1
    g2 = -0.4 * g0 - 1.5 * e1 + 0.1 * rng.standard_normal(P)
    return np.stack([g0, g1, g2]).astype(np.float32).astype(np.float64)


def main():
    S, pcgrad, relobralo = install()
    out = {}
    # ---- PCGrad
    model = S.Sequential(S.Linear(3, 5), S.Linear(5, 2))
    for p in model.parameters():
        p.stop_gradient = False  # (trainable: LossAggregator.__init__ counts them, base.py:46-48)
    P = sum(p.numel() for p in model.parameters())
    G = pcgrad_vectors(P)
    gram = G @ G.T
    assert (gram[np.triu_indices(3, 1)] < 0).all(), gram
    orders = np.asarray(list(itertools.permutations(range(3))), dtype=np.int64)
    res = []
    for order in orders:
        agg = pcgrad.PCGrad(model)
        agg.forward({f"l{k}": torch.zeros(()) for k in order})
        proj = agg._refine_grads([torch.tensor(G[k]) for k in order])
        res.append(np.concatenate([p.detach().numpy().ravel() for p in proj]))
    out["pcgrad/G"], out["pcgrad/orders"], out["pcgrad/out"] = G.astype(np.float32), orders, np.stack(res)
    assert max(np.abs(a - b).max() for a in res for b in res) > 1e-2
    # ---- Relobralo
    rng = np.random.default_rng(22)
    seq = (np.array([2.0, 0.3, 0.05]) * np.exp(-0.3 * np.arange(6))[:, None] * rng.uniform(0.7, 1.3, (6, 3)))
    seq = seq.astype(np.float32).astype(np.float64)
    for beta in (0.0, 1.0):
        for tau in (1.0, 0.1):
            agg = relobralo.Relobralo(3, alpha=0.95, beta=beta, tau=tau)
            lm, tot = [], []
            for step in range(6):
                t = agg({f"l{k}": torch.tensor(seq[step, k]) for k in range(3)}, step)
                lm.append(agg.lmbda.detach().numpy().copy())
                tot.append(float(t))
            tag = f"relobralo/beta{beta:g}_tau{tau:g}"
            out[tag + "/losses"], out[tag + "/lmbda"], out[tag + "/total"] = seq, np.stack(lm), np.asarray(tot)
            out[tag + "/losses_init"], out[tag + "/losses_prev"] = agg.losses_init.numpy().copy(), agg.losses_prev.numpy().copy()
            print(tag, "lmbda", lm[-1], "total", tot[-1])
    np.savez_compressed(os.path.join(HERE, "mtl.npz"), **out)


if __name__ == "__main__":
    main()
