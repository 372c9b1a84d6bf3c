"""ppsci_grad_surgery / ppsci_grad_combine (csrc/grad_surgery.inc) against fp64 numpy: Gram matrix, the PCGrad rule in Gram
space, the weighted combination with and without the Adam update, determinism, the ticket counter, argument checks.

Tolerances (none is tuned to an output):
  Gram:    |got - ref64| <= c eps32 sum_j |a_j b_j|,  c = S + 18: the summation depth of the kernel (grad_surgery.inc) -- a serial
           fmaf chain of S elements per thread, 6 butterfly levels + 3 additions over the waves inside a workgroup, the same once
           more over the workgroups' partial rows.  S <= 4 ceil(per / 1024) + 1, per = columns per workgroup (a thread takes 4
           columns per trip of the float4 loop and at most one of the scalar tail; the scalar loop takes ceil(per / 256) <= that).
  C, w:    rational functions of Gram: compared with the fp64 rule evaluated on the fp32 Gram THE KERNEL RETURNED, which separates
           them from the summation error, under a RUNNING bound that follows the rule step by step (_rule_tol): an update of
           C[i][k] is a K-term fmaf chain (K eps32 sum_m |C[i][m] Gram[m][k]|, plus the errors row i already carries, each times
           |Gram[m][k]|), a division and a subtraction (one eps32 each); where the bound on a projection coefficient exceeds the
           coefficient, its sign -- the branch -- is open and the coefficient itself joins the bound.  w_m sums K entries.  The test
           also asserts that this bound stays below 64 K^2 eps32 max|w|: it is a few ulp of K^2 operations, not a free pass.
  combine: a product and K - 1 fmaf:  |got - ref64| <= (K + 1) eps32 sum_k |w_k G[k][j]|."""
import itertools

import numpy as np
import pytest
import torch

from paddlescience_amd import _lib as L
from paddlescience_amd import device
from paddlescience_amd import hotpath as hp
from tests.common import make_dev_fixture

dev = make_dev_fixture()
EPS32 = float(np.finfo(np.float32).eps)  # 2^-23
CHUNK, MAX_GRID = 2048, 256  # the launch rule of grad_surgery.inc (GS_CHUNK, GS_MAX_GRID)


def _blocks(K, n):
    """Workgroup count read from the library: the workspace is a 64-byte header + one row of K(K+1)/2 floats per workgroup."""
    return (hp.grad_surgery_workspace_bytes(K, n) - 64) // (4 * (K * (K + 1) // 2))


def _gram_c(n):
    grid = min(max((n + CHUNK - 1) // CHUNK, 1), MAX_GRID)
    per = (((n + grid - 1) // grid) + 3) & ~3
    return 4 * ((per + 1023) // 1024) + 1 + 18


def _vectors(K, n, seed):
    """Rows built to conflict: g1 = -0.5 g0 + e1, g2 against both, every further row against its predecessor."""
    rng = np.random.default_rng(seed)
    g = np.zeros((K, n))
    g[0] = rng.standard_normal(n) + (2.0 if n == 1 else 0.0)
    e1 = 0.5 * rng.standard_normal(n) if n > 1 else np.zeros(n)
    if K > 1:
        g[1] = -0.5 * g[0] + e1
    if K > 2:
        g[2] = -0.4 * g[0] - 1.5 * e1 + 0.1 * rng.standard_normal(n) * (n > 1)
    for k in range(3, K):
        g[k] = -0.3 * g[k - 1] + 0.5 * rng.standard_normal(n) * (n > 1) + 0.2 * g[k - 3]
    return g.astype(np.float32)


def ref_rule(gram, order):
    """The PCGrad rule in Gram space, fp64: C and w (zero rows are skipped as projection targets)."""
    K = len(gram)
    C = np.eye(K)
    for i in range(K):
        for k in order:
            if gram[k, k] == 0:
                continue
            pd = (C[i] @ gram[:, k]) / gram[k, k]
            if pd < 0:
                C[i, k] -= pd
    return C, C.sum(0)


def ref_pcgrad_vectors(g, order):
    """pcgrad.py:94-104 restated on fp64 vectors: the projections themselves, no Gram matrix."""
    out = np.zeros(g.shape[1])
    for i in range(len(g)):
        gi = g[i].copy()
        for k in order:
            gi = gi - min((gi @ g[k]) / (g[k] @ g[k]), 0.0) * g[k]
        out += gi
    return out


def _rule_tol(gram, order):
    """Running bound on the fp32 rule's error, following the values the rule actually takes: (EC, Ew) with |C_fp32 - C_ref| <= EC
    entrywise and |w_fp32 - w_ref| <= Ew, C_ref / w_ref the fp64 rule on the same Gram.  u = eps32 (twice the unit roundoff)."""
    K, u = len(gram), EPS32
    C, E = np.eye(K), np.zeros((K, K))
    for i in range(K):
        for k in order:
            gkk = gram[k, k]
            if gkk == 0:
                continue
            col = np.abs(gram[:, k])
            dot = C[i] @ gram[:, k]
            d_dot = E[i] @ col + K * u * (np.abs(C[i]) @ col)  # inherited error + a K-term fmaf chain
            pd, d_pd = dot / gkk, d_dot / gkk + u * abs(dot / gkk)  # + the division
            if pd < 0:
                C[i, k] -= pd
            if abs(pd) <= d_pd:  # the sign of pd is not certain in fp32: either branch may have been taken
                E[i, k] += abs(pd) + d_pd
            elif pd < 0:
                E[i, k] += d_pd + u * abs(C[i, k])  # + the subtraction
    return E, E.sum(0) + K * u * np.abs(C).sum(0)


def _dev_matrix(g32, ld, d):
    K, n = g32.shape
    G = torch.full((K, ld), float("nan"), dtype=torch.float32, device=d)  # columns n .. ld-1 are never to be read
    G[:, :n] = torch.tensor(g32, device=d)
    return G


def _surgery(G, n, K, order, d, mode=L.MTL_PCGRAD, ws=None):
    gram, coef, w = (torch.full((m,), -7.0, device=d) for m in (K * K, K * K, K))
    ws = torch.zeros(hp.grad_surgery_workspace_bytes(K, n) // 4, dtype=torch.int32, device=d) if ws is None else ws
    hp.grad_surgery(G, gram, ws, order, coef, w, mode=mode, n=n)
    return gram, coef, w, ws


CASES = [(n, pad, K) for n in (1, 63, 257, 5003) for pad in (0, 3) for K in (1, 2, 3, 8)]
CASES += [(5003, 1, 3), (5003, 1, 8)]  # ld = 5004: the float4 path over several workgroups, with a scalar tail


@pytest.mark.parametrize("n,pad,K", CASES)
def test_surgery_and_combine(n, pad, K, dev):
    d = device.get_device()
    ld = n + pad
    assert _blocks(K, n) == {1: 1, 63: 1, 257: 1, 5003: 3}[n]  # a single workgroup (no ticket) and several (last-one-out)
    g32 = _vectors(K, n, 100 * K + n)
    g64 = g32.astype(np.float64)
    gram64 = g64 @ g64.T
    if K >= 2:
        assert (gram64[np.triu_indices(K, 1)] < 0).any(), "the case holds no conflict: it would test nothing"
    order = list(np.random.default_rng(n + K).permutation(K))
    G = _dev_matrix(g32, ld, d)

    gram, coef, w, ws = _surgery(G, n, K, order, d)
    # ---- determinism and the ticket: a second call on the SAME workspace gives the same bits
    assert int(ws[0]) == 0
    gram2, coef2, w2, _ = _surgery(G, n, K, order, d, ws=ws)
    assert int(ws[0]) == 0
    for a, b in ((gram, gram2), (coef, coef2), (w, w2)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    # ---- Gram
    got = gram.cpu().numpy().astype(np.float64).reshape(K, K)
    bound = _gram_c(n) * EPS32 * (np.abs(g64)[:, None, :] * np.abs(g64)[None, :, :]).sum(-1)
    err = np.abs(got - gram64)
    print(f"gram: max err / bound = {(err / bound).max():.3f} (c = {_gram_c(n)})")
    assert (err <= bound).all()
    assert np.array_equal(got, got.T)
    # ---- C and w: the fp64 rule on the returned Gram
    C_ref, w_ref = ref_rule(got, order)
    tc, tw = _rule_tol(got, order)
    C_got, w_got = coef.cpu().numpy().reshape(K, K), w.cpu().numpy()
    print(f"C: max err {np.abs(C_got - C_ref).max():.2e} (bound {tc.max():.2e}); w: {np.abs(w_got - w_ref).max():.2e} (bound {tw.max():.2e})")
    assert (np.abs(C_got - C_ref) <= tc).all() and (np.abs(w_got - w_ref) <= tw).all()
    assert tw.max() <= 64 * K * K * EPS32 * max(1.0, np.abs(w_ref).max())  # the bound itself stays at a few ulp of K^2 operations
    # the Gram-space rule IS the reference's projection of the vectors (fp64 on both sides: the derivation, not the kernel)
    C64, w64 = ref_rule(gram64, order)
    direct = ref_pcgrad_vectors(g64, order)
    assert np.abs(w64 @ g64 - direct).max() <= 1e-12 * max(1.0, np.abs(direct).max())

    # ---- combine: weights from the device and from the host, same bits; out[n:] untouched
    def combine(**kw):
        out = torch.full((ld,), 5.0, device=d)
        hp.grad_combine(G, out, n=n, **kw)
        return out

    out_dev = combine(w_dev=w)
    out_host = combine(w_host=[float(x) for x in w_got])
    o = out_dev.cpu().numpy()
    assert np.array_equal(o, out_host.cpu().numpy()) and np.array_equal(o, combine(w_dev=w).cpu().numpy())
    assert (o[n:] == 5.0).all()
    wf = w_got.astype(np.float64)
    cb = (K + 1) * EPS32 * (np.abs(wf)[:, None] * np.abs(g64)).sum(0)
    assert (np.abs(o[:n] - wf @ g64) <= cb).all()
    # ---- combine + Adam == combine, then hp.adam_step on the combined gradient, bit for bit
    rng = np.random.default_rng(7)
    p0, m0, v0 = (torch.tensor(x.astype(np.float32), device=d) for x in
                  (rng.standard_normal(ld), 0.1 * rng.standard_normal(ld), 0.01 * rng.random(ld)))
    p_ref, m_ref, v_ref = p0[:n].clone(), m0[:n].clone(), v0[:n].clone()
    hp.adam_step(p_ref, out_dev[:n].clone(), m_ref, v_ref, 1e-2, 3, grad_scale=0.5)
    for kw in (dict(w_dev=w), dict(w_host=[float(x) for x in w_got])):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        out = combine(params=p, adam=dict(m=m, v=v, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.5, t=3), **kw)
        assert np.array_equal(out.cpu().numpy(), o)
        for a, b, a0 in ((p, p_ref, p0), (m, m_ref, m0), (v, v_ref, v0)):
            assert np.array_equal(a[:n].cpu().numpy(), b.cpu().numpy())
            assert np.array_equal(a[n:].cpu().numpy(), a0[n:].cpu().numpy())
        assert not np.array_equal(p[:n].cpu().numpy(), p0[:n].cpu().numpy())


def test_projection_order_matters(dev):
    d = device.get_device()
    K, n = 3, 257
    g32 = _vectors(K, n, 3)
    G = _dev_matrix(g32, n, d)
    ws, ws_ref = [], []
    for order in itertools.permutations(range(K)):
        gram, coef, w, _ = _surgery(G, n, K, list(order), d)
        got = gram.cpu().numpy().astype(np.float64).reshape(K, K)
        C_ref, w_ref = ref_rule(got, order)
        tc, tw = _rule_tol(got, order)
        assert (np.abs(w.cpu().numpy() - w_ref) <= tw).all() and (np.abs(coef.cpu().numpy().reshape(K, K) - C_ref) <= tc).all()
        ws.append(w.cpu().numpy())
        ws_ref.append(w_ref)
    spread_ref = max(np.abs(a - b).max() for a in ws_ref for b in ws_ref)
    assert spread_ref > 1e-2, "no two orders differ in the reference: the case would test nothing"
    assert max(np.abs(a - b).max() for a in ws for b in ws) > 0.5 * spread_ref


def test_zero_row_is_skipped(dev):
    d = device.get_device()
    K, n = 3, 63
    g32 = _vectors(K, n, 11)
    g32[1] = 0.0
    G = _dev_matrix(g32, n + 3, d)
    gram, coef, w, _ = _surgery(G, n, K, [1, 2, 0], d)
    got = gram.cpu().numpy().astype(np.float64).reshape(K, K)
    assert (got[1] == 0).all() and (got[:, 1] == 0).all()
    C, wv = coef.cpu().numpy().reshape(K, K), w.cpu().numpy()
    assert np.isfinite(C).all() and np.isfinite(wv).all()
    assert np.array_equal(C[1], [0.0, 1.0, 0.0]) and np.array_equal(C[:, 1], [0.0, 1.0, 0.0])
    C_ref, w_ref = ref_rule(got, [1, 2, 0])
    tc, tw = _rule_tol(got, [1, 2, 0])
    assert (np.abs(C - C_ref) <= tc).all() and (np.abs(wv - w_ref) <= tw).all()
    assert got[0, 2] < 0  # the other two still conflict
    out = torch.zeros(n, device=d)
    hp.grad_combine(G, out, w_dev=w, n=n)
    assert np.isfinite(out.cpu().numpy()).all()


def test_gram_only(dev):
    d = device.get_device()
    K, n = 3, 5003
    g32 = _vectors(K, n, 5)
    G = _dev_matrix(g32, n, d)
    gram, coef, w, ws = _surgery(G, n, K, None, d, mode=L.MTL_GRAM_ONLY)
    full = _surgery(G, n, K, [0, 1, 2], d)[0]
    assert np.array_equal(gram.cpu().numpy(), full.cpu().numpy())  # the same summation, whatever follows it
    assert (coef.cpu().numpy() == -7.0).all() and (w.cpu().numpy() == -7.0).all() and int(ws[0]) == 0
    hp.grad_surgery(G, gram, ws, None, None, None, mode=L.MTL_GRAM_ONLY, n=n)  # the outputs it does not write may be absent


def test_invalid_arguments_launch_nothing(dev):
    d = device.get_device()
    K, n = 3, 63
    G = _dev_matrix(_vectors(K, n, 1), n, d)
    big = torch.zeros((9, n), device=d)
    gram, coef, w = torch.full((81,), -7.0, device=d), torch.full((81,), -7.0, device=d), torch.full((9,), -7.0, device=d)
    ws = torch.zeros(hp.grad_surgery_workspace_bytes(K, n) // 4, dtype=torch.int32, device=d)
    out = torch.full((2 * n,), 5.0, device=d)
    lib = L.lib()
    st = hp._stream_ptr(G)
    order = (hp.C.c_int32 * 3)(0, 1, 2)
    w_host = (hp.C.c_float * 3)(1, 1, 1)
    p, nb = hp._p, ws.numel() * 4

    def surgery(K_=K, n_=n, ld=n, od=order, mode=L.MTL_PCGRAD, g=gram, c=coef, w_=w, ws_=ws, nb_=nb, G_=G):
        return lib.ppsci_grad_surgery(K_, n_, p(G_), ld, od, mode, p(g), p(c), p(w_), p(ws_), nb_, st)

    def combine(K_=K, n_=n, ld=n, wd=None, wh=w_host, o=out, params=None, adam=None, G_=G):
        return lib.ppsci_grad_combine(K_, n_, p(G_), ld, p(wd), wh, p(o), p(params), adam, st)

    aa = L.AdamArgs(None, None, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1)
    bad = [
        (lambda: surgery(K_=0), "grad_surgery: invalid"), (lambda: surgery(K_=9, G_=big), "grad_surgery: invalid"),
        (lambda: surgery(ld=n - 1), "grad_surgery: invalid"), (lambda: surgery(n_=0), "grad_surgery: invalid"),
        (lambda: surgery(mode=2), "grad_surgery: invalid"), (lambda: surgery(od=None), "grad_surgery: invalid"),
        (lambda: surgery(c=None), "grad_surgery: invalid"), (lambda: surgery(w_=None), "grad_surgery: invalid"),
        (lambda: surgery(g=None), "grad_surgery: invalid"), (lambda: surgery(ws_=None), "grad_surgery: invalid"),
        (lambda: surgery(nb_=nb - 4), "workspace"), (lambda: surgery(nb_=0), "workspace"),
        (lambda: surgery(od=(hp.C.c_int32 * 3)(0, 0, 1)), "permutation"),
        (lambda: surgery(od=(hp.C.c_int32 * 3)(0, 1, 3)), "permutation"),
        (lambda: surgery(od=(hp.C.c_int32 * 3)(0, -1, 2)), "permutation"),
        (lambda: combine(K_=0), "grad_combine: invalid"), (lambda: combine(K_=9, G_=big), "grad_combine: invalid"),
        (lambda: combine(ld=n - 1), "grad_combine: invalid"), (lambda: combine(n_=0), "grad_combine: invalid"),
        (lambda: combine(o=None), "grad_combine: invalid"),
        (lambda: combine(wd=w, wh=w_host), "exactly one"), (lambda: combine(wd=None, wh=None), "exactly one"),
        (lambda: combine(adam=hp.C.byref(aa)), "Adam update needs"),
    ]
    for call, needle in bad:
        assert call() == -1 and needle in lib.ppsci_last_error().decode(), needle
    if str(d) != "cpu":
        torch.cuda.synchronize()
    for t, fill in ((gram, -7.0), (coef, -7.0), (w, -7.0), (out, 5.0)):
        assert (t.cpu().numpy() == fill).all()
    assert (ws.cpu().numpy() == 0).all()
    # the Python wrappers turn the status into an exception
    with pytest.raises(RuntimeError, match="permutation"):
        hp.grad_surgery(G, gram, ws, [0, 0, 1], coef, w)
    with pytest.raises(RuntimeError, match="exactly one"):
        hp.grad_combine(G, out)
    assert (out.cpu().numpy() == 5.0).all()
