"""Native forward + backward of ppsci.arch.FNO1d (/root/reference/ppsci/arch/geofno.py) on the kernels of csrc/fno1d.inc, composed
by hand in both directions -- no autograd graph, no library operator, no FFT library.

With C = width, M = modes, s the input length, L = s + padding, n = output_np, tables Ta [len][2M] (analysis) and Ts [2M][len]
(synthesis, irfft's conventions folded in) per (input length, output length) built once per shape (`tables`):

    forward                                                               kernel                   geofno.py
    x0     = pad(fc0(x)^T)                                                 ppsci_fno1d_lift_fwd     :170-173
    X_k    = x_k Ta           (S slices over the length)                   ppsci_fno1d_analysis     :71
    Y_k    = sum_i X_k[i] W_k[i, o]   (adds the slices, keeps X_k)         ppsci_fno1d_mix          :82-84
    v_k    = Y_k Ts + Wc_k x_k + bc_k;  x_{k+1} = gelu(v_k)   k = 0..3     ppsci_fno1d_layer        :88-90, :175-193
    u      = Y_4 Ts' + interp(x_4[:, :, :s])                               ppsci_fno1d_layer        :195-198
    z      = fc1(u);  y = fc2(gelu(z))                                     ppsci_fno1d_layer (head) :201-203

    reverse (gv_k = dL/dv_k)
    gz     = gy w2 gelu'(z);  fc2 partial rows                             ppsci_fno1d_head_pre
    gu     = W1 gz                                                         ppsci_fno1d_layer
    fc1 partial rows = u gz^T, sum gz                                      ppsci_fno1d_wgrad
    Ybar_k = gv_k Ts^T                                                     ppsci_fno1d_analysis
    Xbar_k = sum_o Ybar_k[o] conj(W_k[i, o])  (keeps Ybar_k)               ppsci_fno1d_mix (conj)
    dW_k   = sum_b conj(X_k) Ybar_k                                        ppsci_fno1d_mix_wgrad
    w_k partial rows = gv_k x_k^T, sum gv_k                                ppsci_fno1d_wgrad
    gv_{k-1} = (Xbar_k Ta^T + Wc_k^T gv_k) gelu'(v_{k-1})                  ppsci_fno1d_layer  (k = 4: + interp^T(gu), zero on the pad)
    gx, fc0 partial rows                                                   ppsci_fno1d_lift_bwd

Both v_k and x_{k+1} = gelu(v_k) are stored: the reverse pass needs v_k for gelu' and x_k for the convolution's weight gradient, and
the next layer reads x_{k+1} twice (analysis, layer), so recomputing the erf on load would cost three evaluations per element to
save one 4 B write.  The partial rows are summed by ONE ppsci_reduce_rows_multi launch (fixed order: gradients are bitwise
repeatable).  The contract is native_executor.NativeExecutor's (`forward`, `backward`, `gx`, `generation`, one buffer set per
input shape kept alive, the deferred weight-gradient sums)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .hotpath import _p, _require_device, _stream_ptr
from .native_executor import NativeExecutor, grads_adjacent

WGRAD_CHUNK = 256   # points per partial row of the dense weight gradients (ppsci_fno1d_wgrad)
ANA_WORKGROUPS = 256  # the analysis GEMM splits its K axis until it launches about this many workgroups


def supports(model) -> Optional[str]:
    from .arch import geofno

    if not isinstance(model, geofno.FNO1d):
        return "not an FNO1d"
    lib = L.lib()
    Cw, M, Hd = model.width, model.modes1, model.hidden_features
    if not (lib.ppsci_fno1d_layer_supported(Cw, 2 * M, Cw) and lib.ppsci_fno1d_layer_supported(Hd, 0, Cw)
            and lib.ppsci_fno1d_layer_supported(Cw, 0, Hd)):
        return f"width {Cw} with {M} modes does not fit the layer kernel (at most 128 rows, its A operands in LDS)"
    return None


def tables(L_in: int, n: int, M: int):
    """(Ta [L_in][2M], Ts [2M][n]) as float32, phases reduced in integer arithmetic and evaluated in double.
    Ta: columns (2m, 2m + 1) = (cos, -sin)(2 pi l m / L_in): x Ta = the first M coefficients of rfft(x).
    Ts: rows (2m, 2m + 1) = c_m / n (cos, -sin)(2 pi l m / n): Y Ts = irfft(Y, n) -- c = 1 for DC and Nyquist, whose imaginary rows
    are zero, 2 otherwise; rows of modes beyond n // 2 are zero."""
    m = np.arange(M, dtype=np.int64)
    ph = 2 * np.pi * ((np.arange(L_in, dtype=np.int64)[:, None] * m[None, :]) % L_in).astype(np.float64) / L_in
    Ta = np.empty((L_in, 2 * M), dtype=np.float64)
    Ta[:, 0::2], Ta[:, 1::2] = np.cos(ph), -np.sin(ph)
    ph = 2 * np.pi * ((m[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n).astype(np.float64) / n
    edge = (m == 0) | (2 * m == n)
    c = np.where(edge, 1.0, 2.0) * (m <= n // 2) / n
    Ts = np.empty((2 * M, n), dtype=np.float64)
    Ts[0::2], Ts[1::2] = c[:, None] * np.cos(ph), np.where(edge, 0.0, -c)[:, None] * np.sin(ph)
    return Ta.astype(np.float32), Ts.astype(np.float32)


def interp_tables(s: int, n: int):
    """F.interpolate(mode="linear", align_corners=True) from s to n points: out[j] = (1 - t[j]) in[i0[j]] + t[j] in[i0[j] + 1] with
    i0 + t = j (s - 1) / (n - 1) in exact integer arithmetic and i0 <= s - 2; first[i] = the first j with i0[j] >= i, i = 0 .. s."""
    j = np.arange(n, dtype=np.int64)
    den = max(n - 1, 1)
    i0, rem = (j * (s - 1)) // den, (j * (s - 1)) % den
    t = rem.astype(np.float64) / den
    last = i0 >= s - 1
    i0, t = np.where(last, s - 2, i0), np.where(last, 1.0, t)
    first = np.searchsorted(i0, np.arange(s + 1), side="left")
    return i0.astype(np.int32), t.astype(np.float32), first.astype(np.int32)


class Fno1dNative(NativeExecutor):
    """Buffer sets per input shape (batch, s), `backward`, the deferred weight-gradient sums: native_executor.NativeExecutor."""

    label, supports = "FNO1d", staticmethod(supports)

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B: int, s: int) -> None:
        m = self.m
        dev = m.flat_params.device
        f = dict(dtype=torch.float32, device=dev)
        Cw, M, Hd, n = m.width, m.modes1, m.hidden_features, m.output_np
        Lp = s + m.padding
        if s < 2:
            raise ValueError(f"FNO1d: the input has {s} point(s); the linear interpolation needs at least 2")
        if M > s // 2 + 1:
            raise ValueError(f"FNO1d: modes = {M} exceeds {s // 2 + 1} = s // 2 + 1, the number of rfft coefficients of the cropped "
                             f"field of {s} points (the reference fails on its slice assignment there)")
        self.B, self.s, self.Lp, self.n = B, s, Lp, n

        def dev_t(a):
            return torch.tensor(a).to(dev).contiguous()

        Ta, Ts = tables(Lp, Lp, M)
        self.Ta, self.Ts, self.TaT, self.TsT = dev_t(Ta), dev_t(Ts), dev_t(Ta.T.copy()), dev_t(Ts.T.copy())
        Ta4, Ts4 = tables(s, n, M)
        self.Ta4, self.Ts4, self.Ta4T, self.Ts4T = dev_t(Ta4), dev_t(Ts4), dev_t(Ta4.T.copy()), dev_t(Ts4.T.copy())
        i0, t, first = interp_tables(s, n)
        self.ip_i0, self.ip_t, self.ia_first = dev_t(i0), dev_t(t), dev_t(first)
        R = B * Cw
        self.S = self._slices(R, Lp)
        self.x = [torch.empty((B, Cw, Lp), **f) for _ in range(5)]   # x_k, the input of layer k
        self.v = [torch.empty((B, Cw, Lp), **f) for _ in range(4)]   # pre-activations of layers 0..3
        self.Xs = [torch.empty((R, 2 * M), **f) for _ in range(5)]   # spectra of x_k (kept for dL/dW_k)
        self.part = torch.empty((self.S, R, 2 * M), **f)
        self.Y = torch.empty((R, 2 * M), **f)
        self.u = torch.empty((B, Cw, n), **f)
        self.z = torch.empty((B, Hd, n), **f)
        self.y = torch.empty((B, n), **f)
        # reverse
        self.gz = torch.empty((B, Hd, n), **f)
        self.gu = torch.empty((B, Cw, n), **f)
        self.gv = [torch.empty((B, Cw, Lp), **f) for _ in range(2)]
        self.Ybs = torch.empty((R, 2 * M), **f)
        self.Xb = torch.empty((R, 2 * M), **f)
        self.gx = torch.empty((B, s, m.input_channel), **f)
        nch = lambda length: (length + WGRAD_CHUNK - 1) // WGRAD_CHUNK
        self.p_w = [torch.empty((B * nch(Lp), Cw * Cw + Cw), **f) for _ in range(4)]
        self.p_fc1 = torch.empty((B * nch(n), Cw * Hd + Hd), **f)
        self.p_fc2 = torch.empty((B * ((n + 255) // 256), Hd + 1), **f)
        self.lift_rows = int(L.lib().ppsci_fno1d_point_rows(B * s))
        self.p_lift = torch.empty((self.lift_rows, m.input_channel * Cw + Cw), **f)
        for mod in [m.fc0, m.fc1, m.fc2] + [getattr(m, f"w{k}") for k in range(4)]:
            if not grads_adjacent(mod.weight, mod.bias):
                raise RuntimeError("FNO1d: a layer's weight and bias gradients are not contiguous in the flat buffer")

    @staticmethod
    def _slices(rows: int, K: int) -> int:
        tiles = (rows + 63) // 64
        return max(1, min(K // 64, (ANA_WORKGROUPS + tiles - 1) // tiles))

    # ------------------------------------------------------------------ kernel calls
    def _analysis(self, x: torch.Tensor, K: int, ldx: int, T: torch.Tensor) -> int:
        R, N2 = self.B * self.m.width, 2 * self.m.modes1
        S = min(self.S, self._slices(R, K))
        L.check(L.lib().ppsci_fno1d_analysis(R, K, N2, S, ldx, _p(x), _p(T), _p(self.part), _stream_ptr(x)))
        return S

    def _mix(self, S: int, conj: int, keep: torch.Tensor, conv, out: torch.Tensor) -> None:
        m = self.m
        L.check(L.lib().ppsci_fno1d_mix(self.B, m.width, m.modes1, S, conj, _p(self.part), _p(keep), _p(conv.weights1_real),
                                        _p(conv.weights1_imag), _p(out), _stream_ptr(out)))

    def _layer(self, st, **kw) -> None:
        d = L.Fno1dLayerDesc()
        d.B = self.B
        for k, v in kw.items():
            setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        L.check(L.lib().ppsci_fno1d_layer(C.byref(d), st))

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, s, input_channel] on the device -> y [B, output_np, 1] (a buffer owned by the executor)."""
        m, lib = self.m, L.lib()
        _require_device(x)
        if x.ndim != 3 or x.shape[2] != m.input_channel:
            raise ValueError(f"FNO1d: the input must be [B, s, {m.input_channel}], got {tuple(x.shape)}")
        B, s, fin = x.shape
        if self.shape != (B, s):
            self._switch((B, s))
        Cw, M, Hd, n, Lp = m.width, m.modes1, m.hidden_features, self.n, self.Lp
        self.x_in = x.contiguous()
        st = _stream_ptr(self.y)
        L.check(lib.ppsci_fno1d_lift_fwd(B, s, Lp, fin, Cw, _p(self.x_in), _p(m.fc0.weight), _p(m.fc0.bias), _p(self.x[0]), st))
        for k in range(4):
            S = self._analysis(self.x[k], Lp, Lp, self.Ta)
            self._mix(S, 0, self.Xs[k], getattr(m, f"conv{k}"), self.Y)
            w = getattr(m, f"w{k}")
            self._layer(st, R=Cw, K1=2 * M, A1=self.Y, a1_bs=Cw * 2 * M, T=self.Ts, ldt=Lp, K2=Cw, A2=w.weight, a2_rs=Cw, a2_cs=1,
                        X2=self.x[k], x2_bs=Cw * Lp, x2_ld=Lp, x2_len=Lp, bias=w.bias, v=self.v[k], out=self.x[k + 1], o_bs=Cw * Lp,
                        o_ld=Lp, act=1, Lc=Lp, Lout=Lp)
        S = self._analysis(self.x[4], s, Lp, self.Ta4)
        self._mix(S, 0, self.Xs[4], m.conv4, self.Y)
        self._layer(st, R=Cw, K1=2 * M, A1=self.Y, a1_bs=Cw * 2 * M, T=self.Ts4, ldt=n, K2=0, ip_src=self.x[4], ip_bs=Cw * Lp, ip_ld=Lp,
                    ip_i0=self.ip_i0, ip_t=self.ip_t, out=self.u, o_bs=Cw * n, o_ld=n, act=0, Lc=n, Lout=n)
        self._layer(st, R=Hd, K1=0, K2=Cw, A2=m.fc1.weight, a2_rs=1, a2_cs=Hd, X2=self.u, x2_bs=Cw * n, x2_ld=n, x2_len=n,
                    bias=m.fc1.bias, v=self.z, o_bs=Hd * n, o_ld=n, act=1, hw2=m.fc2.weight, hb2=m.fc2.bias, hy=self.y, Lc=n, Lout=n)
        return self.y.view(B, n, 1)

    # ------------------------------------------------------------------ backward
    def _backward(self, gy: torch.Tensor) -> None:
        """gy = dL/dy [B, output_np, 1]; writes dL/d(parameter) into every parameter's `.grad` (views of flat_grad) and dL/dx
        into `self.gx` [B, s, input_channel]."""
        m, lib = self.m, L.lib()
        B, s, Lp, n = self.B, self.s, self.Lp, self.n
        Cw, M, Hd = m.width, m.modes1, m.hidden_features
        gy = gy.contiguous().view(B, n)
        st = _stream_ptr(self.y)
        L.check(lib.ppsci_fno1d_head_pre(B, Hd, n, _p(self.z), _p(gy), _p(m.fc2.weight), _p(self.gz), _p(self.p_fc2), st))
        self._wsegs.append((self.p_fc2.data_ptr(), m.fc2.weight.grad.data_ptr(), self.p_fc2.shape[0], Hd + 1))
        self._layer(st, R=Cw, K1=0, K2=Hd, A2=m.fc1.weight, a2_rs=Hd, a2_cs=1, X2=self.gz, x2_bs=Hd * n, x2_ld=n, x2_len=n, out=self.gu,
                    o_bs=Cw * n, o_ld=n, act=0, Lc=n, Lout=n)
        L.check(lib.ppsci_fno1d_wgrad(B, Cw, Hd, n, WGRAD_CHUNK, 2, _p(self.u), Cw * n, n, _p(self.gz), Hd * n, n, _p(self.p_fc1), st))
        self._wsegs.append((self.p_fc1.data_ptr(), m.fc1.weight.grad.data_ptr(), self.p_fc1.shape[0], Cw * Hd + Hd))
        # the last spectral layer and the interpolation beside it; what it stores is gv_3 (zero on the padded tail: the crop)
        S = self._analysis(self.gu, n, n, self.Ts4T)
        self._mix(S, 1, self.Ybs, m.conv4, self.Xb)
        L.check(lib.ppsci_fno1d_mix_wgrad(B, Cw, M, _p(self.Xs[4]), _p(self.Ybs), _p(m.conv4.weights1_real.grad),
                                          _p(m.conv4.weights1_imag.grad), st))
        gv, nxt = self.gv
        self._layer(st, R=Cw, K1=2 * M, A1=self.Xb, a1_bs=Cw * 2 * M, T=self.Ta4T, ldt=s, K2=0, ia_src=self.gu, ia_bs=Cw * n, ia_ld=n,
                    ia_first=self.ia_first, ip_i0=self.ip_i0, ip_t=self.ip_t, dact_v=self.v[3], dv_bs=Cw * Lp, dv_ld=Lp, out=gv,
                    o_bs=Cw * Lp, o_ld=Lp, act=0, Lc=s, Lout=Lp)
        for k in range(3, -1, -1):
            w, conv = getattr(m, f"w{k}"), getattr(m, f"conv{k}")
            L.check(lib.ppsci_fno1d_wgrad(B, Cw, Cw, Lp, WGRAD_CHUNK, 1, _p(gv), Cw * Lp, Lp, _p(self.x[k]), Cw * Lp, Lp,
                                          _p(self.p_w[k]), st))
            self._wsegs.append((self.p_w[k].data_ptr(), w.weight.grad.data_ptr(), self.p_w[k].shape[0], Cw * Cw + Cw))
            S = self._analysis(gv, Lp, Lp, self.TsT)
            self._mix(S, 1, self.Ybs, conv, self.Xb)
            L.check(lib.ppsci_fno1d_mix_wgrad(B, Cw, M, _p(self.Xs[k]), _p(self.Ybs), _p(conv.weights1_real.grad),
                                              _p(conv.weights1_imag.grad), st))
            below = dict(dact_v=self.v[k - 1], dv_bs=Cw * Lp, dv_ld=Lp) if k > 0 else {}
            self._layer(st, R=Cw, K1=2 * M, A1=self.Xb, a1_bs=Cw * 2 * M, T=self.TaT, ldt=Lp, K2=Cw, A2=w.weight, a2_rs=1, a2_cs=Cw,
                        X2=gv, x2_bs=Cw * Lp, x2_ld=Lp, x2_len=Lp, out=nxt, o_bs=Cw * Lp, o_ld=Lp, act=0, Lc=Lp, Lout=Lp, **below)
            gv, nxt = nxt, gv
        L.check(lib.ppsci_fno1d_lift_bwd(B, s, Lp, m.input_channel, Cw, _p(self.x_in), _p(m.fc0.weight), _p(gv), _p(self.gx),
                                         _p(self.p_lift), st))
        self._wsegs.append((self.p_lift.data_ptr(), m.fc0.weight.grad.data_ptr(), self.lift_rows, self.p_lift.shape[1]))
