"""Native forward + backward of ppsci.arch.LNO (/root/reference/ppsci/arch/lno.py) on the kernels of csrc/lno.inc, composed by
hand in both directions -- no autograd graph, no library operator, no FFT library.

With N = n1 n2 n3 grid points, C = width, pair = (i, o), tables A_d[pair][m][p] = 1 / (lambda_d[p] - mu_d[pair][m]) and
E_d[pair][m][s] = exp(mu_d[pair][m] t_d[s]) (ppsci_lno_tables), z the Laplace layer's input:

    forward                                                          kernel                        lno.py
    h      = fc0(x [+ grid])                                          ppsci_lno_lift_fwd            :281-285
    z      = IN(h)                       (use_norm)                   ppsci_lno_inorm_fwd           :288
    alpha  = F z                                                      ppsci_lno_dft3                :161
    H      = sum_mnk rho A_1 A_2 A_3                                  ppsci_lno_synthesis           :154 (eq1)
    x1     = Re F^-1 (sum_i alpha_i H_io)                             ppsci_lno_dft3 (mix on load)  :154, :164-167
    Gam    = sum_pqr alpha A_1 A_2 A_3      per (b, i, o)             ppsci_lno_analysis            :155 (eq2)
    gamma  = - sum_i rho_io Gam_bio                                   ppsci_lno_channel_sum         :155
    x2     = 1/N Re sum_o sum_mnk gamma_bo E_1 E_2 E_3 [o, o']        ppsci_lno_synthesis (added)   :169-186
    x1n    = IN(x1 + x2)                 (use_norm)                   ppsci_lno_inorm_fwd           :288
    y      = fc2(act(fc1(x1n + conv(h))))                             ppsci_lno_head_fwd            :292-299

    reverse (g = dL/d(Laplace output), real; every stage above is multilinear)
    ghat   = F g                                                      ppsci_lno_dft3
    Q      = sum_s g conj(E_1 E_2 E_3)  per (b, o', o); dL/dmu via E  ppsci_lno_analysis (+ reverse chain, cotangent gamma / N)
    gbar   = 1/N sum_o' Q_bo'o          (= dL/dgamma)                 ppsci_lno_channel_sum
    dL/dmu via A in Gam                                               ppsci_lno_analysis (reverse chain, cotangent -conj(rho) gbar)
    Hbar   = 1/N sum_b conj(alpha_bi) ghat_bo                         ppsci_lno_hbar
    Gp     = sum_pqr Hbar conj(A_1 A_2 A_3); dL/dmu via A in H        ppsci_lno_analysis (+ reverse chain, cotangent rho)
    dL/drho = Gp - sum_b conj(Gam) gbar                               ppsci_lno_rho_grad
    abar2  = sum_o sum_mnk (-conj(rho) gbar) conj(A_1 A_2 A_3)        ppsci_lno_synthesis (complex planes)
    dL/dz  = Re F^H (1/N sum_o conj(H_io) ghat_bo + abar2)            ppsci_lno_dft3 (mix on load)

The three dL/dmu contributions land in rows [0, B), [B, 2B) and 2B of one partial matrix per pole tensor; those, the head's and
fc0's partial rows are summed by ONE ppsci_reduce_rows_multi launch (fixed order: gradients are bitwise repeatable).  The
contract is native_executor.NativeExecutor's (`forward`, `backward`, `gx`, `generation`, one buffer set per input shape kept alive)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .hotpath import _p, _require_device, _stream_ptr
from .native_executor import NativeExecutor, grads_adjacent


def supports(model) -> Optional[str]:
    from .arch import lno

    if not isinstance(model, lno.LNO):
        return "not an LNO"
    if not L.lib().ppsci_lno_head_supported(model.width, model.hidden_features):
        return f"width {model.width} with {model.hidden_features} hidden features does not fit the head kernel's LDS"
    return None


def _ptrs(ts):
    return L.ptr_array([t.data_ptr() for t in ts])


def twiddles(ns) -> np.ndarray:
    """[sum n_d][2] = (cos, sin)(2 pi k / n_d), in double."""
    rows = []
    for n in ns:
        k = np.arange(n, dtype=np.float64)
        rows.append(np.stack([np.cos(2 * np.pi * k / n), np.sin(2 * np.pi * k / n)], 1))
    return np.concatenate(rows, 0).astype(np.float32)


class LnoNative(NativeExecutor):
    """Buffer sets per input shape (batch, n1, n2, n3), `backward`, the deferred weight-gradient sums: native_executor.NativeExecutor."""

    label, supports = "LNO", staticmethod(supports)

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B: int, n1: int, n2: int, n3: int) -> None:
        m = self.m
        lp = m.laplace
        dev = m.flat_params.device
        f = dict(dtype=torch.float32, device=dev)
        Cw, Hd = m.width, m.hidden_features
        n, md = (n1, n2, n3), m.modes
        for d in range(3):
            if getattr(lp, f"t_{d}").shape[1] != n[d]:
                raise ValueError(f"LNO: axis {d} of the input has {n[d]} points, the grid it was built with "
                                 f"{getattr(lp, f't_{d}').shape[1]}")
        if not L.lib().ppsci_lno_supported(n1, n2, n3, *md):
            raise NotImplementedError(f"LNO: a {n1} x {n2} x {n3} plane with {md} modes does not fit the kernels' LDS")
        N, M, CC = n1 * n2 * n3, md[0] * md[1] * md[2], Cw * Cw
        self.n, self.N, self.M, self.B = n, N, M, B
        self.n_c, self.m_c = (C.c_int * 3)(*n), (C.c_int * 3)(*md)
        self.tw = torch.tensor(twiddles(n), **f)
        self.omega = [getattr(lp, f"lambda_{d}").imag.reshape(-1).to(**f).contiguous() for d in range(3)]
        self.tg = [getattr(lp, f"t_{d}").reshape(-1).to(**f).contiguous() for d in range(3)]
        self.A = [torch.empty((CC, md[d], n[d], 2), **f) for d in range(3)]
        self.E = [torch.empty((CC, md[d], n[d], 2), **f) for d in range(3)]
        self.h = torch.empty((B, Cw, N), **f)
        self.z = torch.empty((B, Cw, N), **f) if m.use_norm else self.h
        self.st1 = torch.empty((B * Cw, 2), **f)
        self.st2 = torch.empty((B * Cw, 2), **f)
        self.alpha = torch.empty((B * Cw, 2, N), **f)
        self.H = torch.empty((CC, 2, N), **f)
        self.lap = torch.empty((B, Cw, N), **f)           # x1 + x2
        self.x1n = torch.empty((B, Cw, N), **f) if m.use_norm else self.lap
        self.Gam = torch.empty((B * CC, M, 2), **f)
        self.gamma = torch.empty((B * Cw, M, 2), **f)
        self.y = torch.empty((B, N), **f)
        # reverse
        self.g_x1n = torch.empty((B, Cw, N), **f)
        self.g_lap = torch.empty((B, Cw, N), **f) if m.use_norm else self.g_x1n
        self.g_hc = torch.empty((B, Cw, N), **f)          # the convolution's share of dL/dh
        self.g_z = torch.empty((B, Cw, N), **f)
        self.g_h = torch.empty((B, Cw, N), **f) if m.use_norm else None
        self.ghat = torch.empty((B * Cw, 2, N), **f)
        self.Q = torch.empty((B * CC, M, 2), **f)
        self.gbar = torch.empty((B * Cw, M, 2), **f)
        self.Hbar = torch.empty((CC, 2, N), **f)
        self.Gp = torch.empty((CC, M, 2), **f)
        self.abar2 = torch.empty((B * Cw, 2, N), **f)
        self.mu_rows = 2 * B + 1
        self.mu_re = [torch.zeros((self.mu_rows, CC * md[d]), **f) for d in range(3)]
        self.mu_im = [torch.zeros((self.mu_rows, CC * md[d]), **f) for d in range(3)]
        self.rows = int(L.lib().ppsci_lno_point_rows(B * N))
        self.fd = m.in_features - (3 if m.use_grid else 0)
        self.p_lift = torch.empty((self.rows, m.in_features * Cw + Cw), **f)
        self.p_head = torch.empty((self.rows, CC + Cw + Cw * Hd + 2 * Hd + 1), **f)
        self.gx = torch.empty((B, N, self.fd), **f)
        # the six head tensors are summed as ONE row segment: they follow each other in the flat gradient buffer
        if not grads_adjacent(m.conv.weight, m.conv.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias):
            raise RuntimeError("LNO: conv / fc1 / fc2 gradients are not contiguous in the flat buffer")
        if not grads_adjacent(m.fc0.weight, m.fc0.bias):
            raise RuntimeError("LNO: fc0 gradients are not contiguous in the flat buffer")

    def _desc(self, nb, ncp, nc2, pair_cp, pair_c2, conj_t=0, coef=(0, 0, 0), mult_conj=0, gscale=1.0):
        d = L.LnoTriDesc()
        for k in range(3):
            d.n[k], d.m[k] = self.n[k], self.m.modes[k]
        d.nb, d.ncp, d.nc2, d.C, d.pair_cp, d.pair_c2, d.conj_t = nb, ncp, nc2, self.m.width, pair_cp, pair_c2, conj_t
        d.coef_b, d.coef_cp, d.coef_c2 = coef
        d.mult_conj, d.gscale = mult_conj, gscale
        return d

    def _dft(self, planes, in_mode, src, out, sign, out_real, scale=1.0, H=None, pair=(0, 0), conj_h=0, mix_scale=1.0, add=None,
             accumulate=0, zero_dc=0):
        n1, n2, n3 = self.n
        L.check(L.lib().ppsci_lno_dft3(planes, n1, n2, n3, in_mode, _p(src), self.m.width, _p(H), pair[0], pair[1], conj_h,
                                       mix_scale, _p(add), _p(self.tw), sign, out_real, accumulate, scale, zero_dc, _p(out), _stream_ptr(out)))

    # ------------------------------------------------------------------ forward
    def laplace_forward(self, z: torch.Tensor, out: torch.Tensor, x2_only: bool = False, x1_only: bool = False,
                        centred: bool = False) -> None:
        """out [B, C, N] = Laplace(z) (lno.py:160-187); the two flags leave one of its two parts out (tests); centred: every
        plane of z has zero mean by construction."""
        m, lib = self.m, L.lib()
        lp = m.laplace
        B, Cw, N, M = self.B, m.width, self.N, self.M
        st = _stream_ptr(out)
        pr, pi = list(lp.weights_pole_real), list(lp.weights_pole_imag)
        rr, ri = lp.weights_residue_real, lp.weights_residue_imag
        L.check(lib.ppsci_lno_tables(Cw, self.n_c, self.m_c, _ptrs(pr), _ptrs(pi), _ptrs(self.omega), _ptrs(self.tg), _ptrs(self.A),
                                     _ptrs(self.E), st))
        # (behind the instance norm z has zero mean: its frequency-0 coefficient is exactly 0, not the fp32 noise of a sum)
        self._dft(B * Cw, 0, z, self.alpha, -1, 0, zero_dc=2 if centred else 0)
        if not x2_only:
            L.check(lib.ppsci_lno_synthesis(C.byref(self._desc(1, Cw * Cw, 1, 1, 0)), _ptrs(self.A), None, _p(rr), _p(ri), 0, 0, 1.0,
                                            _p(self.H), st))
            self._dft(B * Cw, 2, self.alpha, out, 1, 1, scale=1.0 / N, H=self.H, pair=(1, Cw))  # pair = (i = c2, o = cp)
            if x1_only:
                return
        L.check(lib.ppsci_lno_analysis(C.byref(self._desc(B, Cw, Cw, Cw, 1)), _p(self.alpha), 0, _ptrs(self.A), _p(self.Gam), None,
                                       None, None, 0, None, None, None, 0, st))
        L.check(lib.ppsci_lno_channel_sum(B, Cw, M, _p(self.Gam), _p(rr), _p(ri), -1.0, _p(self.gamma), st))
        # plane (b, o' = cp), loop o = c2: coefficients gamma[b, o], tables E[o, o']
        L.check(lib.ppsci_lno_synthesis(C.byref(self._desc(B, Cw, Cw, 1, Cw, coef=(Cw, 0, 1))), _ptrs(self.E), _p(self.gamma), None,
                                        None, 1, 0 if x2_only else 1, 1.0 / N, _p(out), st))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, n1, n2, n3, data channels] on the device -> y [B, n1, n2, n3, 1] (a buffer owned by the executor)."""
        m, lib = self.m, L.lib()
        _require_device(x)
        if x.ndim != 5:
            raise ValueError(f"LNO: the input must be [B, n1, n2, n3, channels], got {tuple(x.shape)}")
        B, n1, n2, n3, fd = x.shape
        if self.shape != (B, n1, n2, n3):
            self._switch((B, n1, n2, n3))
        if fd != self.fd:
            raise ValueError(f"LNO: {fd} input channels, in_features = {m.in_features}" + (" (with 3 grid channels)" if m.use_grid else ""))
        Cw, N, Hd = m.width, self.N, m.hidden_features
        self.x_in = x.contiguous()
        st = _stream_ptr(self.y)
        L.check(lib.ppsci_lno_lift_fwd(B, n1, n2, n3, fd, 1 if m.use_grid else 0, Cw, _p(self.x_in), _p(m.fc0.weight), _p(m.fc0.bias),
                                       _p(self.h), st))
        if m.use_norm:
            L.check(lib.ppsci_lno_inorm_fwd(B * Cw, N, m.norm_eps, _p(self.h), _p(self.z), _p(self.st1), st))
        self.laplace_forward(self.z, self.lap, centred=m.use_norm)
        if m.use_norm:
            L.check(lib.ppsci_lno_inorm_fwd(B * Cw, N, m.norm_eps, _p(self.lap), _p(self.x1n), _p(self.st2), st))
        L.check(lib.ppsci_lno_head_fwd(B, N, Cw, Hd, L.ACT[m.activation], _p(self.x1n), _p(self.h), _p(m.conv.weight), _p(m.conv.bias),
                                       _p(m.fc1.weight), _p(m.fc1.bias), _p(m.fc2.weight), _p(m.fc2.bias), _p(self.y), st))
        return self.y.view(B, n1, n2, n3, 1)

    # ------------------------------------------------------------------ backward
    def laplace_backward(self, g: torch.Tensor, gz: torch.Tensor, accumulate: bool = False, centred: bool = False) -> None:
        """g = dL/d(Laplace output) [B, C, N] -> gz = dL/dz (accumulate: added to gz); pole partial rows and the residue
        gradients are written.  centred: an instance norm's reverse follows, which takes the mean of gz out."""
        m, lib = self.m, L.lib()
        lp = m.laplace
        B, Cw, N, M = self.B, m.width, self.N, self.M
        st = _stream_ptr(gz)
        rr, ri = lp.weights_residue_real, lp.weights_residue_imag
        mre, mim = _ptrs(self.mu_re), _ptrs(self.mu_im)
        self._dft(B * Cw, 0, g, self.ghat, -1, 0)
        # plane (b, o' = cp), loop o = c2, tables conj(E[o, o']); cotangent of Q[b, o', o] is gamma[b, o] / N
        L.check(lib.ppsci_lno_analysis(C.byref(self._desc(B, Cw, Cw, 1, Cw, conj_t=1, coef=(Cw, 0, 1), gscale=1.0 / N)), _p(g), 1,
                                       _ptrs(self.E), _p(self.Q), _p(self.gamma), None, None, 1, _ptrs(self.tg), mre, mim, B, st))
        # gbar[b, o] = 1/N sum_o' Q[b, o', o]
        L.check(lib.ppsci_lno_channel_sum(B, Cw, M, _p(self.Q), None, None, 1.0 / N, _p(self.gbar), st))
        # plane (b, i = cp), loop o = c2, tables A[i, o]; cotangent of Gam[b, i, o] is -conj(rho[i, o]) gbar[b, o]
        L.check(lib.ppsci_lno_analysis(C.byref(self._desc(B, Cw, Cw, Cw, 1, coef=(Cw, 0, 1), mult_conj=1, gscale=-1.0)), _p(self.alpha),
                                       0, _ptrs(self.A), None, _p(self.gbar), _p(rr), _p(ri), 0, None, mre, mim, 0, st))
        L.check(lib.ppsci_lno_hbar(B, Cw, N, _p(self.alpha), _p(self.ghat), 1.0 / N, _p(self.Hbar), st))
        # planes = pairs, tables conj(A[pair]); Gp = dL/drho through H, cotangent rho for the poles
        L.check(lib.ppsci_lno_analysis(C.byref(self._desc(1, Cw * Cw, 1, 1, 0, conj_t=1)), _p(self.Hbar), 0, _ptrs(self.A), _p(self.Gp),
                                       None, _p(rr), _p(ri), 0, None, mre, mim, 2 * B, st))
        L.check(lib.ppsci_lno_rho_grad(B, Cw, M, _p(self.Gam), _p(self.gbar), _p(self.Gp), _p(rr.grad), _p(ri.grad), st))
        L.check(lib.ppsci_lno_synthesis(C.byref(self._desc(B, Cw, Cw, Cw, 1, conj_t=1, coef=(Cw, 0, 1), mult_conj=1, gscale=-1.0)),
                                        _ptrs(self.A), _p(self.gbar), _p(rr), _p(ri), 0, 0, 1.0, _p(self.abar2), st))
        # plane (b, i = cp): 1/N sum_o conj(H[i, o]) ghat[b, o] + abar2, then Re F^H
        self._dft(B * Cw, 2, self.ghat, gz, 1, 1, H=self.H, pair=(Cw, 1), conj_h=1, mix_scale=1.0 / N, add=self.abar2,
                  accumulate=1 if accumulate else 0, zero_dc=1 if centred else 0)
        for d in range(3):
            cols = self.mu_re[d].shape[1]
            self._wsegs.append((self.mu_re[d].data_ptr(), lp.weights_pole_real[d].grad.data_ptr(), self.mu_rows, cols))
            self._wsegs.append((self.mu_im[d].data_ptr(), lp.weights_pole_imag[d].grad.data_ptr(), self.mu_rows, cols))

    def _backward(self, gy: torch.Tensor) -> None:
        """gy = dL/dy [B, n1, n2, n3, 1]; writes dL/d(parameter) into every parameter's `.grad` (views of flat_grad) and
        dL/dx into `self.gx` [B, N, data channels]."""
        m, lib = self.m, L.lib()
        B, (n1, n2, n3) = self.B, self.n
        Cw, N, Hd = m.width, self.N, m.hidden_features
        gy = gy.contiguous().view(B, N)
        st = _stream_ptr(self.y)
        L.check(lib.ppsci_lno_head_bwd(B, N, Cw, Hd, L.ACT[m.activation], _p(self.x1n), _p(self.h), _p(m.conv.weight), _p(m.conv.bias),
                                       _p(m.fc1.weight), _p(m.fc1.bias), _p(m.fc2.weight), _p(gy), _p(self.g_x1n), _p(self.g_hc),
                                       _p(self.p_head), st))
        self._wsegs.append((self.p_head.data_ptr(), m.conv.weight.grad.data_ptr(), self.rows, self.p_head.shape[1]))
        if m.use_norm:
            L.check(lib.ppsci_lno_inorm_bwd(B * Cw, N, _p(self.x1n), _p(self.g_x1n), _p(self.st2), None, _p(self.g_lap), st))
        if m.use_norm:
            self.laplace_backward(self.g_lap, self.g_z, centred=True)
            L.check(lib.ppsci_lno_inorm_bwd(B * Cw, N, _p(self.z), _p(self.g_z), _p(self.st1), _p(self.g_hc), _p(self.g_h), st))
            gh = self.g_h
        else:  # no norm in between: the Laplace layer's share of dL/dh is added to the convolution's
            self.laplace_backward(self.g_lap, self.g_hc, accumulate=True)
            gh = self.g_hc
        L.check(lib.ppsci_lno_lift_bwd(B, n1, n2, n3, self.fd, 1 if m.use_grid else 0, Cw, _p(self.x_in), _p(m.fc0.weight), _p(gh),
                                       _p(self.gx), _p(self.p_lift), st))
        self._wsegs.append((self.p_lift.data_ptr(), m.fc0.weight.grad.data_ptr(), self.rows, self.p_lift.shape[1]))
