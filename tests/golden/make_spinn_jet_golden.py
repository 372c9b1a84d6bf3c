"""Generates tests/golden/spinn_jet.npz by executing the REFERENCE's own SPINN code (ppsci/arch/spinn.py, arch/mlp.py
ModifiedMLP, equation/pde/helmholtz.py hvp_revrev) under the torch-backed paddle shim, on residuals that are NOT linear in
{u, u_xx, u_yy, u_zz}: closures written with `helm.hvp_revrev` and `paddle.incubate.autograd.jvp`, as a user of the reference
writes them (the shim and its jvp are make_spinn_golden.py's).

    python tests/golden/make_spinn_jet_golden.py

Everything is computed in float64 and once more in float32 (S.DTYPE = torch.float32, same float32-representable parameters and
data): the relative-L2 distance of the float32 run from the float64 run is stored per residual / loss / gradient -- it is the
reference's own float32 error, from which the tests' residual bound is taken.

Residuals on SPINN(("t", "x", "y"), ("u",)), loss = MSELoss("mean") with a weight grid w in [0.5, 1.5]:
    kg       u_tt - u_xx - u_yy + u*u                       (Klein-Gordon)
    burgers  u_t + u*u_x - 0.01*(u_xx + u_yy)
    sg       u_tt - u_xx - u_yy + sin(u) + x*u_xy           (reads a coordinate and a mixed stream)
    ut       u_t                                            (a Neumann face)
Per case <c> and residual <e>: <c>/param/<b>/<name>, <c>/t|x|y, <c>/label, <c>/weight, <c>/u, <c>/<e>/loss, <c>/<e>/grad/<b>/<name>,
<c>/<e>/err32 = (residual, loss, gradient), <c>/<e>/residual for grids under 1 000 points and for kg of case C.
Case G = case A's kg plus case F's face as a second constraint of the same net (A's): total loss, summed gradient, and the loss
of 30 Adam steps (lr 1e-3, restated below) of the float64 run from the fixture weights."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _paddle_shim as S  # noqa: E402
from make_spinn_golden import install  # noqa: E402

CASES = {
    # name: (r, num_layers, hidden, activation, (nt, nx, ny), residuals)
    "A": (4, 3, 16, "tanh", (7, 5, 6), ("kg", "burgers", "sg")),
    "B": (3, 2, 8, "tanh", (4, 9, 3), ("kg",)),
    "C": (32, 2, 32, "tanh", (17, 33, 19), ("kg", "burgers", "sg")),
    "D": (16, 2, 32, "silu", (16, 16, 16), ("burgers",)),
    "E": (4, 2, 16, "sin", (5, 4, 6), ("sg",)),
    "F": (4, 2, 16, "tanh", (1, 9, 5), ("ut",)),
}
MAX_BYTES = 740 * 1024  # the largest operator fixture committed (lno.npz)


def residuals(paddle, helm, model):
    jvp = paddle.incubate.autograd.jvp
    f = model.forward_tensor

    def second(t, x, y):
        return (helm.hvp_revrev(lambda t_: f(t_, x, y), (t,)), helm.hvp_revrev(lambda x_: f(t, x_, y), (x,)),
                helm.hvp_revrev(lambda y_: f(t, x, y_), (y,)))

    def kg(d):
        t, x, y = d["t"], d["x"], d["y"]
        u_tt, u_xx, u_yy = second(t, x, y)
        return u_tt - u_xx - u_yy + d["u"] * d["u"]

    def burgers(d):
        t, x, y = d["t"], d["x"], d["y"]
        _, u_xx, u_yy = second(t, x, y)
        u_t = jvp(lambda t_: f(t_, x, y), (t,))[1][0]
        u_x = jvp(lambda x_: f(t, x_, y), (x,))[1][0]
        return u_t + d["u"] * u_x - 0.01 * (u_xx + u_yy)

    def sg(d):
        t, x, y = d["t"], d["x"], d["y"]
        u_tt, u_xx, u_yy = second(t, x, y)
        u_xy = jvp(lambda y_: jvp(lambda x_: f(t, x_, y_), (x,))[1][0], (y,))[1]
        return u_tt - u_xx - u_yy + paddle.sin(d["u"]) + x.reshape([1, -1, 1, 1]) * u_xy

    def ut(d):
        t, x, y = d["t"], d["x"], d["y"]
        return jvp(lambda t_: f(t_, x, y), (t,))[1][0]

    return {"kg": kg, "burgers": burgers, "sg": sg, "ut": ut}


def build(spinn, cfg, params, dtype):
    r, nl, hid, act = cfg
    S.DTYPE = dtype
    model = spinn.SPINN(("t", "x", "y"), ("u",), r, nl, hid, act)
    named = []
    with torch.no_grad():
        for b, net in enumerate(model.branch_nets):
            for n, p in net.named_parameters():
                p.copy_(torch.tensor(params[(b, n)], dtype=dtype))
                named.append((b, n, p))
    return model, named


def evaluate(paddle, helm, model, named, coords, label, weight, which, dtype, want_grad=True):
    xs = [torch.tensor(c, dtype=dtype) for c in coords]
    data = {"t": xs[0], "x": xs[1], "y": xs[2]}
    data.update(model(data))
    res = residuals(paddle, helm, model)[which](data)
    loss = (torch.tensor(weight, dtype=dtype) * (res - torch.tensor(label, dtype=dtype)) ** 2).mean()
    if not want_grad:
        return data["u"].detach(), res.detach(), loss, None
    grads = torch.autograd.grad(loss, [p for _, _, p in named], allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for (_, _, p), g in zip(named, grads)]
    return data["u"].detach(), res.detach(), loss, grads


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def main():
    spinn, helm = install()
    paddle = sys.modules["paddle"]
    out, keep = {}, {}
    for c, (r, nl, hid, act, shape, which) in CASES.items():
        rng = np.random.default_rng(1000 + ord(c))
        S.DTYPE = torch.float64
        probe = spinn.SPINN(("t", "x", "y"), ("u",), r, nl, hid, act)
        params = {}
        for b, net in enumerate(probe.branch_nets):
            for n, p in net.named_parameters():
                fan_in = p.shape[0] if p.ndim == 2 else 1
                scale = (1.0 / np.sqrt(fan_in)) if p.ndim == 2 else 0.1
                params[(b, n)] = (rng.standard_normal(tuple(p.shape)) * scale).astype(np.float32)
                out[f"{c}/param/{b}/{n}"] = params[(b, n)]
        coords = [rng.uniform(lo, 1, (n, 1)).astype(np.float32) for lo, n in zip((0, -1, -1), shape)]
        label = rng.standard_normal(shape + (1,)).astype(np.float32)
        weight = rng.uniform(0.5, 1.5, shape + (1,)).astype(np.float32)
        for k, a in zip("txy", coords):
            out[f"{c}/{k}"] = a
        out[f"{c}/label"], out[f"{c}/weight"] = label, weight
        out[f"{c}/config"] = np.asarray([r, nl, hid])
        out[f"{c}/activation"] = np.asarray(act)
        keep[c] = (params, coords, label, weight)
        for e in which:
            m64, n64 = build(spinn, (r, nl, hid, act), params, torch.float64)
            u, res, loss, grads = evaluate(paddle, helm, m64, n64, coords, label, weight, e, torch.float64)
            m32, n32 = build(spinn, (r, nl, hid, act), params, torch.float32)
            _, res32, loss32, grads32 = evaluate(paddle, helm, m32, n32, coords, label, weight, e, torch.float32)
            g64 = np.concatenate([g.numpy().ravel() for g in grads])
            g32 = np.concatenate([g.numpy().ravel() for g in grads32])
            err = (rel(res32.numpy(), res.numpy()), abs(float(loss32.detach()) - float(loss.detach())) / abs(float(loss.detach())), rel(g32, g64))
            big = int(np.prod(shape)) >= 1000  # u and the gradients of the large grids are stored float32 (size): 6e-8, against
            rt = np.float32 if big else np.float64  # the tests' 5e-6 / 1e-4
            out[f"{c}/u"] = u.numpy().astype(rt)
            out[f"{c}/{e}/loss"] = np.asarray(float(loss.detach()))
            out[f"{c}/{e}/err32"] = np.asarray(err)
            for (b, n, _), g in zip(n64, grads):
                out[f"{c}/{e}/grad/{b}/{n}"] = g.numpy().astype(rt)
            if not big or (c, e) == ("C", "kg"):
                out[f"{c}/{e}/residual"] = res.numpy()
            print(c, e, "loss", float(loss.detach()), "fp32 vs fp64 (residual, loss, grad)", err)
    # ---- G: A's kg on A's grid + the Neumann face of F (its coordinates, label and weight) on A's net; one gradient
    S.DTYPE = torch.float64
    r, nl, hid, act, _, _ = CASES["A"]
    params, coordsA, labelA, weightA = keep["A"]
    _, coordsF, labelF, weightF = keep["F"]
    model, named = build(spinn, (r, nl, hid, act), params, torch.float64)

    def total_loss():
        _, _, l1, _ = evaluate(paddle, helm, model, named, coordsA, labelA, weightA, "kg", torch.float64, False)
        _, _, l2, _ = evaluate(paddle, helm, model, named, coordsF, labelF, weightF, "ut", torch.float64, False)
        return l1 + l2

    loss = total_loss()
    grads = torch.autograd.grad(loss, [p for _, _, p in named])
    out["G/loss"] = np.asarray(float(loss.detach()))
    for (b, n, _), g in zip(named, grads):
        out[f"G/grad/{b}/{n}"] = g.numpy()
    # Adam (paddle.optimizer.Adam's update: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), p -= lr_t m / (sqrt(v) + eps sqrt(1 - b2^t)))
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    ps = [p for _, _, p in named]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    hist = []
    for t in range(1, 32):
        loss = total_loss()
        hist.append(float(loss.detach()))
        if t == 31:
            break
        gs = torch.autograd.grad(loss, ps)
        with torch.no_grad():
            for p, g, m, v in zip(ps, gs, ms, vs):
                m.mul_(b1).add_((1 - b1) * g)
                v.mul_(b2).add_((1 - b2) * g * g)
                lr_t = lr * np.sqrt(1 - b2**t) / (1 - b1**t)
                p.sub_(lr_t * m / (v.sqrt() + eps * np.sqrt(1 - b2**t)))
    out["G/train_loss"] = np.asarray(hist)
    print("G loss", hist[0], "-> after 30 Adam steps", hist[30])
    path = os.path.join(HERE, "spinn_jet.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote spinn_jet.npz", len(out), "arrays", size, "bytes")
    assert size < MAX_BYTES, f"{size} bytes: the fixture must stay below {MAX_BYTES}"


if __name__ == "__main__":
    main()
