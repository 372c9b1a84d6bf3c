// fno1d.inc -- kernels of ppsci.arch.FNO1d (Geo-FNO); included by uno.hip.
//
//   /root/reference/ppsci/arch/geofno.py:68-92     SpectralConv1d.forward  rfft -> first `modes` coefficients x complex [C, C] -> irfft(n)
//   /root/reference/ppsci/arch/geofno.py:167-205   FNO1d.forward           fc0, pad, 4 x gelu(spectral + 1x1 conv), crop, spectral + linear
//                                                                          interpolation, fc1 -> gelu -> fc2
//
// Activations are [B][C][L] fp32.  Only M = modes of the L/2 + 1 coefficients are kept (64 of 1051 at the catheter shape), so both
// transforms are GEMMs against tables built once per shape on the host in double (geofno_engine.tables):
//
//   X[b,i,:]  = x[b,i,0:L] . Ta                  Ta [L][2M] = (cos, -sin)(2 pi l m / L)                fno1d_ana (split over K = L)
//   Y[b,o,m]  = sum_i X[b,i,m] W[i,o,m]          complex, per mode                                    fno1d_mix
//   v[b,o,l]  = sum_k Y[b,o,k] Ts[k,l] + sum_i Wc[o,i] x[b,i,l] + bc[o]                               fno1d_layer: ONE GEMM, K = 2M + C
//   out       = gelu(v)                          Ts [2M][n] = c_m / n (cos, -sin)(2 pi l m / n)       (its epilogue)
//
// The reverse pass runs the SAME three kernels with transposed tables: Ybar = gv . Ts^T (fno1d_ana), Xbar = Ybar . conj(W)^T
// (fno1d_mix), dx = Xbar . Ta^T + Wc^T gv (fno1d_layer, whose epilogue multiplies by gelu'(v) of the layer below, so that what it
// stores is already that layer's gv).  The head (fc1 -> gelu -> fc2) is the layer kernel with 128 rows and a row reduction in its
// epilogue.  GEMMs are on v_mfma_f32_16x16x4_f32; lengths need not be multiples of anything (every operand load is guarded).
// Every sum runs in a fixed order and no kernel uses atomics: results are bitwise repeatable.  Parameter gradients of the dense
// layers are partial rows per (sample, chunk of points), summed by ppsci_reduce_rows_multi (wgrad_reduce.hip).

#define F1_T 256
#define F1_TS (F1_T + 1)
#define F1_MAXR 128  // rows of the layer kernel's GEMM (width, or fc1's 128 outputs): 8 accumulator tiles per wave

static int f1_launch_ok(const char* what) {
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("%s: launch failed", what);
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// exact (erf) GELU and its derivative (F.gelu(approximate=False), geofno.py:178)
__device__ __forceinline__ float f1_gelu(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float f1_dgelu(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * expf(-0.5f * z * z);
}

// ------------------------------------------------------------------------------------------------ lift: fc0 + transpose + zero pad
struct F1LiftArgs {
  const float* x;   // [B][s][fin]
  const float* W;   // [fin][C]
  const float* bias;
  float* h;         // forward out [B][C][Lp]: fc0 on l < s, zero on s <= l < Lp
  const float* gh;  // reverse in  [B][C][Lp] (the padded tail is ignored: the crop's adjoint)
  float* gx;        // reverse out [B][s][fin]
  float* partials;  // reverse out [grid][fin * C + C]
  long long P;      // forward: B * Lp; reverse: B * s
  int s, Lp, fin, C;
};

__global__ void __launch_bounds__(F1_T) fno1d_lift_fwd_kernel(F1LiftArgs a) {
  for (long long g = (long long)blockIdx.x * F1_T + threadIdx.x; g < a.P; g += (long long)gridDim.x * F1_T) {
    const long long b = g / a.Lp;
    const int l = (int)(g - b * a.Lp);
    const float* xp = a.x + (b * a.s + (l < a.s ? l : 0)) * a.fin;
    for (int c = 0; c < a.C; ++c) {
      float v = 0.f;
      if (l < a.s) {
        v = a.bias[c];
        for (int f = 0; f < a.fin; ++f) v = fmaf(xp[f], a.W[f * a.C + c], v);
      }
      a.h[(b * a.C + c) * a.Lp + l] = v;
    }
  }
}

// tiles of 256 points; x and gh of a tile in LDS, then one thread per (f, c) sums its product over the tile's points in order and
// adds it to the workgroup's row (LDS), written out once at the end (the scheme of lno_lift_bwd_kernel)
__global__ void __launch_bounds__(F1_T) fno1d_lift_bwd_kernel(F1LiftArgs a) {
  PPSCI_DYN_SMEM(smem);
  float* xs = smem;                 // [fin][256]
  float* gs = xs + a.fin * F1_TS;   // [C][256]
  float* acc = gs + a.C * F1_TS;    // [fin * C + C]
  const int tid = threadIdx.x;
  const int cols = a.fin * a.C + a.C;
  for (int e = tid; e < cols; e += F1_T) acc[e] = 0.f;
  const long long tiles = (a.P + F1_T - 1) / F1_T;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long g = tile * F1_T + tid;
    const bool live = g < a.P;
    const long long b = live ? g / a.s : 0;
    const int l = live ? (int)(g - b * a.s) : 0;
    __syncthreads();
    for (int f = 0; f < a.fin; ++f) xs[f * F1_TS + tid] = live ? a.x[g * a.fin + f] : 0.f;
    for (int c = 0; c < a.C; ++c) gs[c * F1_TS + tid] = live ? a.gh[(b * a.C + c) * a.Lp + l] : 0.f;
    if (live) {
      for (int f = 0; f < a.fin; ++f) {
        float v = 0.f;
        for (int c = 0; c < a.C; ++c) v = fmaf(a.W[f * a.C + c], gs[c * F1_TS + tid], v);
        a.gx[g * a.fin + f] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < cols; e += F1_T) {
      float v = 0.f;
      if (e < a.fin * a.C) {
        const int f = e / a.C, c = e - f * a.C;
        for (int p = 0; p < F1_T; ++p) v = fmaf(xs[f * F1_TS + p], gs[c * F1_TS + p], v);
      } else {
        const int c = e - a.fin * a.C;
        for (int p = 0; p < F1_T; ++p) v += gs[c * F1_TS + p];
      }
      acc[e] += v;
    }
  }
  __syncthreads();
  for (int e = tid; e < cols; e += F1_T) a.partials[(long long)blockIdx.x * cols + e] = acc[e];
}

extern "C" int64_t ppsci_fno1d_point_rows(int64_t points) {
  const int64_t tiles = (points + F1_T - 1) / F1_T;
  const int64_t cap = 2 * PPSCI_NUM_CU;
  return tiles < 1 ? 1 : (tiles < cap ? tiles : cap);
}

static int f1_lift_fill(F1LiftArgs& a, const char* what, int B, int s, int Lp, int fin, int C) {
  if (B < 1 || s < 1 || Lp < s || fin < 1 || C < 1 || (long long)B * Lp >= (1ll << 31)) {
    ppsci_set_error("%s: invalid argument", what);
    return PPSCI_E_INVALID;
  }
  a = F1LiftArgs{};
  a.s = s, a.Lp = Lp, a.fin = fin, a.C = C;
  return PPSCI_OK;
}

extern "C" int ppsci_fno1d_lift_fwd(int B, int s, int Lp, int fin, int C, const float* x, const float* W, const float* bias, float* h,
                                    void* stream) {
  F1LiftArgs a;
  const int rc = f1_lift_fill(a, "fno1d_lift_fwd", B, s, Lp, fin, C);
  if (rc != PPSCI_OK) return rc;
  if (!x || !W || !bias || !h) {
    ppsci_set_error("fno1d_lift_fwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  a.x = x, a.W = W, a.bias = bias, a.h = h, a.P = (long long)B * Lp;
  long long grid = (a.P + F1_T - 1) / F1_T;
  if (grid > 8192) grid = 8192;
  PPSCI_LAUNCH(fno1d_lift_fwd_kernel, F1LiftArgs, (int)grid, F1_T, 0, stream, a);
  return f1_launch_ok("fno1d_lift_fwd");
}

extern "C" int ppsci_fno1d_lift_bwd(int B, int s, int Lp, int fin, int C, const float* x, const float* W, const float* gh, float* gx,
                                    float* partials, void* stream) {
  F1LiftArgs a;
  const int rc = f1_lift_fill(a, "fno1d_lift_bwd", B, s, Lp, fin, C);
  if (rc != PPSCI_OK) return rc;
  if (!x || !W || !gh || !gx || !partials) {
    ppsci_set_error("fno1d_lift_bwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  a.x = x, a.W = W, a.gh = gh, a.gx = gx, a.partials = partials, a.P = (long long)B * s;
  const long long lds = ((long long)(fin + C) * F1_TS + (long long)fin * C + C) * 4;
  if (lds > PPSCI_LDS_LIMIT_BYTES - 1024) {
    ppsci_set_error("fno1d_lift_bwd: %d input and %d output channels do not fit LDS", fin, C);
    return PPSCI_E_UNSUPPORTED;
  }
  if (PPSCI_SET_MAX_LDS(fno1d_lift_bwd_kernel, lds) != 0) {
    ppsci_set_error("fno1d_lift_bwd: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  PPSCI_LAUNCH(fno1d_lift_bwd_kernel, F1LiftArgs, (int)ppsci_fno1d_point_rows(a.P), F1_T, (int)lds, stream, a);
  return f1_launch_ok("fno1d_lift_bwd");
}

// ------------------------------------------------------------------------------------------------ analysis: tall-skinny split-K GEMM
struct F1AnaArgs {
  const float* x;   // row r at x + r * ldx, K values
  const float* T;   // [K][N2]
  float* part;      // [S][R][N2]: slice s holds the sum over k in [K s / S, K (s + 1) / S)
  long long ldx;
  int R, K, N2, S, RT;
};

// A workgroup = 64 rows (16 per wave) x up to 128 columns x one K slice.  Lane (g, c) reads FOUR consecutive k of its row (the
// 16 lanes of a row group read 64 contiguous bytes per row) and feeds them to four MFMAs, so the k index of MFMA step t is
// k0 + 4 g + t: a permutation of the slice, the same in every run.
__global__ void __launch_bounds__(F1_T) fno1d_ana_kernel(F1AnaArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  int bid = blockIdx.x;
  const int rt = bid % a.RT;
  bid /= a.RT;
  const int s = bid % a.S, cg = bid / a.S;
  const int row = rt * 64 + wave * 16 + c;
  const bool rok = row < a.R;
  const float* xr = a.x + (long long)(rok ? row : 0) * a.ldx;
  const int k_lo = (int)((long long)a.K * s / a.S), k_hi = (int)((long long)a.K * (s + 1) / a.S);
  const int j0 = cg * 128;
  const int nbn = (a.N2 - j0 + 15) / 16 < 8 ? (a.N2 - j0 + 15) / 16 : 8;
  f32x4 acc[8];
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = k_lo; k0 < k_hi; k0 += 16) {
    float xv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = k0 + 4 * g + t;
      xv[t] = (rok && k < k_hi) ? xr[k] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = k0 + 4 * g + t;
      const bool kok = k < k_hi;
      const float* tr = a.T + (long long)(kok ? k : 0) * a.N2;
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        if (nb < nbn) {
          const int j = j0 + 16 * nb + c;
          const float bv = (kok && j < a.N2) ? tr[j] : 0.f;
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[t], bv, acc[nb], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) {
    const int j = j0 + 16 * nb + c;
    if (nb < nbn && j < a.N2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = rt * 64 + wave * 16 + 4 * g + r;
        if (rr < a.R) a.part[((long long)s * a.R + rr) * a.N2 + j] = acc[nb][r];
      }
    }
  }
}

extern "C" int ppsci_fno1d_analysis(int R, int K, int N2, int S, int64_t ldx, const float* x, const float* T, float* part,
                                    void* stream) {
  if (R < 1 || K < 1 || N2 < 1 || S < 1 || S > K || ldx < K || !x || !T || !part) {
    ppsci_set_error("fno1d_analysis: invalid argument");
    return PPSCI_E_INVALID;
  }
  F1AnaArgs a{x, T, part, (long long)ldx, R, K, N2, S, (R + 63) / 64};
  const long long grid = (long long)a.RT * S * ((N2 + 127) / 128);
  if (grid >= (1ll << 31)) {
    ppsci_set_error("fno1d_analysis: %lld workgroups", grid);
    return PPSCI_E_UNSUPPORTED;
  }
  PPSCI_LAUNCH(fno1d_ana_kernel, F1AnaArgs, (int)grid, F1_T, 0, stream, a);
  return f1_launch_ok("fno1d_analysis");
}

// ------------------------------------------------------------------------------------------------ per-mode complex channel mix
#define F1_MC 4  // modes per workgroup
struct F1MixArgs {
  const float* part;  // [S][B * C][2M]: the analysis kernel's slices, summed here in ascending order
  float* sum;         // [B * C][2M]: that sum, kept for the weight gradient (or NULL)
  const float* wr;    // [C][C][M] (in, out, mode)
  const float* wi;
  float* out;         // [B * C][2M]
  int B, C, M, S, conj;
};

// conj = 0:  out[b,o,m] = sum_i in[b,i,m] W[i,o,m]          (geofno.py:48-66)
// conj = 1:  out[b,i,m] = sum_o in[b,o,m] conj(W[i,o,m])    (its adjoint w.r.t. the spectrum)
__global__ void __launch_bounds__(F1_T) fno1d_mix_kernel(F1MixArgs a) {
  PPSCI_DYN_SMEM(smem);  // [C][F1_MC][2]
  const int tid = threadIdx.x;
  const int mchunks = (a.M + F1_MC - 1) / F1_MC;
  const int b = blockIdx.x / mchunks, m0 = (blockIdx.x - b * mchunks) * F1_MC;
  const int N2 = 2 * a.M;
  const long long RN = (long long)a.B * a.C * N2;
  for (int idx = tid; idx < a.C * 2 * F1_MC; idx += F1_T) {
    const int ci = idx / (2 * F1_MC), q = idx - ci * 2 * F1_MC;
    const int col = 2 * m0 + q;
    float v = 0.f;
    if (col < N2) {
      const long long off = ((long long)b * a.C + ci) * N2 + col;
      for (int s = 0; s < a.S; ++s) v += a.part[s * RN + off];
      if (a.sum) a.sum[off] = v;
    }
    smem[idx] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < a.C * F1_MC; idx += F1_T) {
    const int co = idx / F1_MC, mm = idx - co * F1_MC, m = m0 + mm;
    if (m >= a.M) continue;
    float re = 0.f, im = 0.f;
    for (int ci = 0; ci < a.C; ++ci) {
      const float xr = smem[(ci * F1_MC + mm) * 2], xi = smem[(ci * F1_MC + mm) * 2 + 1];
      const long long w = (a.conj ? ((long long)co * a.C + ci) : ((long long)ci * a.C + co)) * a.M + m;
      const float wr = a.wr[w], wi = a.conj ? -a.wi[w] : a.wi[w];
      re = fmaf(xr, wr, re), re = fmaf(-xi, wi, re);
      im = fmaf(xr, wi, im), im = fmaf(xi, wr, im);
    }
    float* o = a.out + ((long long)b * a.C + co) * N2 + 2 * m;
    o[0] = re, o[1] = im;
  }
}

extern "C" int ppsci_fno1d_mix(int B, int C, int M, int S, int conj, const float* part, float* sum, const float* wr, const float* wi,
                               float* out, void* stream) {
  if (B < 1 || C < 1 || M < 1 || S < 1 || !part || !wr || !wi || !out || (conj != 0 && conj != 1)) {
    ppsci_set_error("fno1d_mix: invalid argument");
    return PPSCI_E_INVALID;
  }
  const long long lds = (long long)C * F1_MC * 2 * 4;
  if (lds > PPSCI_LDS_LIMIT_BYTES - 1024) {
    ppsci_set_error("fno1d_mix: %d channels do not fit LDS", C);
    return PPSCI_E_UNSUPPORTED;
  }
  F1MixArgs a{part, sum, wr, wi, out, B, C, M, S, conj};
  if (PPSCI_SET_MAX_LDS(fno1d_mix_kernel, lds) != 0) {
    ppsci_set_error("fno1d_mix: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  PPSCI_LAUNCH(fno1d_mix_kernel, F1MixArgs, B * ((M + F1_MC - 1) / F1_MC), F1_T, (int)lds, stream, a);
  return f1_launch_ok("fno1d_mix");
}

struct F1MixWgArgs {
  const float* X;   // [B * C][2M] spectrum of the layer's input
  const float* Yb;  // [B * C][2M] cotangent of the mixed spectrum
  float* gwr;       // [C][C][M]
  float* gwi;
  int B, C, M;
};

// dL/dW[i,o,m] = sum_b conj(X[b,i,m]) Ybar[b,o,m], b ascending in one thread
__global__ void __launch_bounds__(F1_T) fno1d_mix_wgrad_kernel(F1MixWgArgs a) {
  const long long total = (long long)a.C * a.C * a.M;
  for (long long e = (long long)blockIdx.x * F1_T + threadIdx.x; e < total; e += (long long)gridDim.x * F1_T) {
    const int m = (int)(e % a.M);
    const long long io = e / a.M;
    const int o = (int)(io % a.C), i = (int)(io / a.C);
    float re = 0.f, im = 0.f;
    for (int b = 0; b < a.B; ++b) {
      const float* x = a.X + (((long long)b * a.C + i) * a.M + m) * 2;
      const float* y = a.Yb + (((long long)b * a.C + o) * a.M + m) * 2;
      re = fmaf(x[0], y[0], re), re = fmaf(x[1], y[1], re);
      im = fmaf(x[0], y[1], im), im = fmaf(-x[1], y[0], im);
    }
    a.gwr[e] = re, a.gwi[e] = im;
  }
}

extern "C" int ppsci_fno1d_mix_wgrad(int B, int C, int M, const float* X, const float* Yb, float* gwr, float* gwi, void* stream) {
  if (B < 1 || C < 1 || M < 1 || !X || !Yb || !gwr || !gwi) {
    ppsci_set_error("fno1d_mix_wgrad: invalid argument");
    return PPSCI_E_INVALID;
  }
  F1MixWgArgs a{X, Yb, gwr, gwi, B, C, M};
  long long grid = ((long long)C * C * M + F1_T - 1) / F1_T;
  if (grid > 8192) grid = 8192;
  PPSCI_LAUNCH(fno1d_mix_wgrad_kernel, F1MixWgArgs, (int)grid, F1_T, 0, stream, a);
  return f1_launch_ok("fno1d_mix_wgrad");
}

// ------------------------------------------------------------------------------------------------ the fused layer kernel
// One workgroup = one sample b and 64 columns l (16 per wave); it produces ALL R rows of
//   acc[r][l] = sum_{k < K1} A1[b][r][k] T[k][l]  +  sum_{c < K2} A2[r][c] X2[b][c][l]
// with the A operands of both blocks in LDS ([k][R + 16]: the 16 rows of a fragment in consecutive banks, the four k of an MFMA
// step 16 banks apart) and the B operands read where they lie (lane c = column l: 64 contiguous bytes per k).  Epilogue per
// element, in this order: + bias[r]; + the 2-tap linear interpolation of ip_src (or its adjoint, ia_src); store v; times
// gelu'(dact_v); gelu; store out; head: y[b][l] = sum_r hw2[r] gelu(.) + hb2.  Columns Lc <= l < Lout are written as zeros.
struct F1LayerArgs {
  ppsci_fno1d_layer_desc d;
  int K1p, K2p, RS;
};

__global__ void __launch_bounds__(F1_T) fno1d_layer_kernel(F1LayerArgs a) {
  PPSCI_DYN_SMEM(smem);
  const ppsci_fno1d_layer_desc& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int RS = a.RS, Kt = a.K1p + a.K2p;
  float* As = smem;            // [K1p + K2p][RS]
  float* red = As + Kt * RS;   // [4 waves][4][16]
  const int tiles = (d.Lout + 63) / 64;
  const int b = blockIdx.x / tiles, l0 = (blockIdx.x - b * tiles) * 64;
  for (int idx = tid; idx < Kt * RS; idx += F1_T) As[idx] = 0.f;
  __syncthreads();
  if (d.K1 > 0) {
    const float* A1 = d.A1 + (long long)b * d.a1_bs;
    for (int idx = tid; idx < d.R * d.K1; idx += F1_T) {
      const int r = idx / d.K1, k = idx - r * d.K1;
      As[k * RS + r] = A1[idx];
    }
  }
  for (int idx = tid; idx < d.R * d.K2; idx += F1_T) {
    const int r = idx / d.K2, k = idx - r * d.K2;
    As[(a.K1p + k) * RS + r] = d.A2[(long long)r * d.a2_rs + (long long)k * d.a2_cs];
  }
  __syncthreads();
  const int l = l0 + wave * 16 + c;
  const bool lok = l < d.Lc;
  const int rbn = (d.R + 15) / 16;
  f32x4 acc[8];
#pragma unroll
  for (int rb = 0; rb < 8; ++rb) acc[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K1p; k0 += 4) {
    const int k = k0 + g;
    const float bv = (lok && k < d.K1) ? d.T[(long long)k * d.ldt + l] : 0.f;
    const float* ar = As + k * RS + c;
#pragma unroll
    for (int rb = 0; rb < 8; ++rb)
      if (rb < rbn) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[16 * rb], bv, acc[rb], 0, 0, 0);
  }
  if (d.K2 > 0) {
    const float* X2 = d.X2 + (long long)b * d.x2_bs;
    const bool xok = lok && l < d.x2_len;
    for (int k0 = 0; k0 < a.K2p; k0 += 4) {
      const int k = k0 + g;
      const float bv = (xok && k < d.K2) ? X2[(long long)k * d.x2_ld + l] : 0.f;
      const float* ar = As + (a.K1p + k) * RS + c;
#pragma unroll
      for (int rb = 0; rb < 8; ++rb)
        if (rb < rbn) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[16 * rb], bv, acc[rb], 0, 0, 0);
    }
  }
  // epilogue: lane (g, c) holds rows 16 rb + 4 g + r of column l
  float ysum = 0.f;
  int i0 = 0, j_lo = 0, j_hi = 0;
  float tt = 0.f;
  if (lok && d.ip_src) i0 = d.ip_i0[l], tt = d.ip_t[l];
  if (lok && d.ia_src) j_lo = d.ia_first[l > 0 ? l - 1 : 0], j_hi = d.ia_first[l + 1];
#pragma unroll
  for (int rb = 0; rb < 8; ++rb) {
    if (rb >= rbn) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * rb + 4 * g + r;
      if (row >= d.R || l >= d.Lout) continue;
      float val = 0.f;
      if (lok) {
        val = acc[rb][r];
        if (d.bias) val += d.bias[row];
        if (d.ip_src) {
          const float* sp = d.ip_src + (long long)b * d.ip_bs + (long long)row * d.ip_ld + i0;
          val += fmaf(tt, sp[1] - sp[0], sp[0]);
        }
        if (d.ia_src) {
          const float* sp = d.ia_src + (long long)b * d.ia_bs + (long long)row * d.ia_ld;
          float sacc = 0.f;
          for (int j = j_lo; j < j_hi; ++j) {
            const float t = d.ip_t[j];
            sacc = fmaf(d.ip_i0[j] == l ? 1.f - t : t, sp[j], sacc);
          }
          val += sacc;
        }
        if (d.v) d.v[(long long)b * d.o_bs + (long long)row * d.o_ld + l] = val;
        if (d.dact_v) val *= f1_dgelu(d.dact_v[(long long)b * d.dv_bs + (long long)row * d.dv_ld + l]);
        if (d.act) val = f1_gelu(val);
        if (d.hy) ysum = fmaf(d.hw2[row], val, ysum);
      }
      if (d.out) d.out[(long long)b * d.o_bs + (long long)row * d.o_ld + l] = val;
    }
  }
  if (d.hy) {  // (uniform over the workgroup)
    red[(wave * 4 + g) * 16 + c] = ysum;
    __syncthreads();
    if (g == 0 && lok) {
      const float* rp = red + wave * 64 + c;
      d.hy[(long long)b * d.Lout + l] = ((rp[0] + rp[16]) + (rp[32] + rp[48])) + d.hb2[0];
    }
  }
}

static long long f1_layer_lds(const ppsci_fno1d_layer_desc* d, int* K1p, int* K2p, int* RS) {
  *K1p = (d->K1 + 3) & ~3, *K2p = (d->K2 + 3) & ~3;
  *RS = ((d->R + 15) & ~15) + 16;
  return ((long long)(*K1p + *K2p) * *RS + 256) * 4;
}

extern "C" int ppsci_fno1d_layer_supported(int R, int K1, int K2) {
  if (R < 1 || R > F1_MAXR || K1 < 0 || K2 < 0 || K1 + K2 < 1) return 0;
  ppsci_fno1d_layer_desc d{};
  d.R = R, d.K1 = K1, d.K2 = K2;
  int a, b, c;
  return f1_layer_lds(&d, &a, &b, &c) <= PPSCI_LDS_LIMIT_BYTES - 1024 ? 1 : 0;
}

extern "C" int ppsci_fno1d_layer(const ppsci_fno1d_layer_desc* d, void* stream) {
  if (!d || d->B < 1 || d->R < 1 || d->K1 < 0 || d->K2 < 0 || d->K1 + d->K2 < 1 || d->Lc < 1 || d->Lout < d->Lc ||
      (d->K1 > 0 && (!d->A1 || !d->T || d->ldt < d->Lc)) || (d->K2 > 0 && (!d->A2 || !d->X2 || d->x2_len < 1)) || (!d->out && !d->v && !d->hy) ||
      ((d->out || d->v) && d->o_ld < d->Lout) || (d->ip_src && (!d->ip_i0 || !d->ip_t)) ||
      (d->ia_src && (!d->ia_first || !d->ip_i0 || !d->ip_t)) || (d->hy && (!d->hw2 || !d->hb2)) ||
      (long long)d->B * ((d->Lout + 63) / 64) >= (1ll << 31)) {
    ppsci_set_error("fno1d_layer: invalid argument");
    return PPSCI_E_INVALID;
  }
  if (!ppsci_fno1d_layer_supported(d->R, d->K1, d->K2)) {
    ppsci_set_error("fno1d_layer: %d rows with K = %d + %d do not fit the kernel (at most %d rows, A operands in LDS)", d->R, d->K1, d->K2,
                    F1_MAXR);
    return PPSCI_E_UNSUPPORTED;
  }
  F1LayerArgs a;
  a.d = *d;
  const long long lds = f1_layer_lds(d, &a.K1p, &a.K2p, &a.RS);
  if (PPSCI_SET_MAX_LDS(fno1d_layer_kernel, lds) != 0) {
    ppsci_set_error("fno1d_layer: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  PPSCI_LAUNCH(fno1d_layer_kernel, F1LayerArgs, d->B * ((d->Lout + 63) / 64), F1_T, (int)lds, stream, a);
  return f1_launch_ok("fno1d_layer");
}

// ------------------------------------------------------------------------------------------------ dense weight gradients
struct F1WgArgs {
  const float* P;   // [B][R1][ldp]
  const float* Q;   // [B][R2][ldq]
  float* partials;  // [B * nchunks][R1 * R2 + (bias_of ? R1 or R2 : 0)]
  long long p_bs, q_bs;
  int ldp, ldq, R1, R2, len, chunk, nchunks, bias_of;  // bias_of 1: row sums of P follow the matrix, 2: row sums of Q
};

// Row (b, chunk) of the partial matrix: G[r1][r2] = sum_{l in chunk} P[b][r1][l] Q[b][r2][l] on the fp32 MFMA (k = l, four
// consecutive l per lane as in fno1d_ana_kernel) and the row sums that are the bias gradient.  Wave w owns the row blocks
// w, w + 4, ... of G; the sums over l are in a fixed order.
__global__ void __launch_bounds__(F1_T) fno1d_wgrad_kernel(F1WgArgs a) {
  __shared__ float red[4][F1_MAXR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int b = blockIdx.x / a.nchunks, ch = blockIdx.x - b * a.nchunks;
  const int l_lo = ch * a.chunk, l_hi = l_lo + a.chunk < a.len ? l_lo + a.chunk : a.len;
  const float* P = a.P + (long long)b * a.p_bs;
  const float* Q = a.Q + (long long)b * a.q_bs;
  const int nb1 = (a.R1 + 15) / 16, nb2 = (a.R2 + 15) / 16;
  const int cols = a.R1 * a.R2 + (a.bias_of == 1 ? a.R1 : (a.bias_of == 2 ? a.R2 : 0));
  float* out = a.partials + (long long)blockIdx.x * cols;
  const int passes = (nb1 + 3) / 4;  // (uniform over the workgroup: every wave runs every pass, MFMAs included)
  for (int ps = 0; ps < passes; ++ps) {
    const int rb1 = ps * 4 + wave;
    const int r1 = 16 * rb1 + c;
    const bool r1ok = rb1 < nb1 && r1 < a.R1;
    const float* pr = P + (long long)(r1ok ? r1 : 0) * a.ldp;
    f32x4 acc[8];
    float psum = 0.f, qsum[8];
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f}, qsum[nb] = 0.f;
    for (int l0 = l_lo; l0 < l_hi; l0 += 16) {
      float pv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int l = l0 + 4 * g + t;
        pv[t] = (r1ok && l < l_hi) ? pr[l] : 0.f;
        psum += pv[t];
      }
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        if (nb < nb2) {
          const int r2 = 16 * nb + c;
          const float* qr = Q + (long long)(r2 < a.R2 ? r2 : 0) * a.ldq;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int l = l0 + 4 * g + t;
            const float qv = (r2 < a.R2 && l < l_hi) ? qr[l] : 0.f;
            qsum[nb] += qv;
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[t], qv, acc[nb], 0, 0, 0);
          }
        }
      }
    }
    if (rb1 < nb1) {
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        const int r2 = 16 * nb + c;
        if (nb < nb2 && r2 < a.R2) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rr = 16 * rb1 + 4 * g + r;
            if (rr < a.R1) out[(long long)rr * a.R2 + r2] = acc[nb][r];
          }
        }
      }
    }
    // bias gradient: the four lane groups hold the sums over l = 4 g + t (mod 16) of their row
    __syncthreads();
    if (a.bias_of == 1 && rb1 < nb1) red[g][16 * rb1 + c] = psum;
    if (a.bias_of == 2 && ps == 0 && wave == 0) {
#pragma unroll
      for (int nb = 0; nb < 8; ++nb)
        if (nb < nb2) red[g][16 * nb + c] = qsum[nb];
    }
    __syncthreads();
    if (a.bias_of == 1) {
      for (int r = tid; r < 64; r += F1_T) {
        const int rr = 64 * ps + r;
        if (rr < a.R1) out[(long long)a.R1 * a.R2 + rr] = (red[0][rr] + red[1][rr]) + (red[2][rr] + red[3][rr]);
      }
    } else if (a.bias_of == 2 && ps == 0) {
      for (int r = tid; r < a.R2; r += F1_T) out[(long long)a.R1 * a.R2 + r] = (red[0][r] + red[1][r]) + (red[2][r] + red[3][r]);
    }
  }
}

extern "C" int ppsci_fno1d_wgrad(int B, int R1, int R2, int len, int chunk, int bias_of, const float* P, int64_t p_bs, int ldp,
                                 const float* Q, int64_t q_bs, int ldq, float* partials, void* stream) {
  if (B < 1 || R1 < 1 || R2 < 1 || R1 > F1_MAXR || R2 > F1_MAXR || len < 1 || chunk < 16 || (chunk & 15) || bias_of < 0 || bias_of > 2 ||
      !P || !Q || !partials || ldp < len || ldq < len) {
    ppsci_set_error("fno1d_wgrad: invalid argument (at most %d rows a side, chunks of a multiple of 16 points)", F1_MAXR);
    return PPSCI_E_INVALID;
  }
  F1WgArgs a{P, Q, partials, (long long)p_bs, (long long)q_bs, ldp, ldq, R1, R2, len, chunk, (len + chunk - 1) / chunk, bias_of};
  PPSCI_LAUNCH(fno1d_wgrad_kernel, F1WgArgs, B * a.nchunks, F1_T, 0, stream, a);
  return f1_launch_ok("fno1d_wgrad");
}

// ------------------------------------------------------------------------------------------------ head reverse, first stage
struct F1HeadPreArgs {
  const float* z;   // [B][Hd][n] pre-activation of fc1
  const float* gy;  // [B][n]
  const float* w2;  // [Hd]
  float* gz;        // [B][Hd][n] = gy w2[j] gelu'(z)
  float* partials;  // [B * nchunks][Hd + 1]: fc2.weight (sum_l gy gelu(z)), fc2.bias (sum_l gy)
  int B, Hd, n, nchunks;
};

__global__ void __launch_bounds__(F1_T) fno1d_head_pre_kernel(F1HeadPreArgs a) {
  __shared__ float vals[16 * F1_TS];
  __shared__ float p1[16 * 16];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.nchunks, l = (blockIdx.x - b * a.nchunks) * F1_T + tid;
  const bool live = l < a.n;
  const float gy = live ? a.gy[(long long)b * a.n + l] : 0.f;
  float* out = a.partials + (long long)blockIdx.x * (a.Hd + 1);
  for (int j0 = 0; j0 <= a.Hd; j0 += 16) {  // (j = Hd is the fc2.bias column: the plain sum of gy)
    for (int jj = 0; jj < 16; ++jj) {
      const int j = j0 + jj;
      float v = 0.f;
      if (j < a.Hd && live) {
        const long long off = ((long long)b * a.Hd + j) * a.n + l;
        const float z = a.z[off];
        a.gz[off] = gy * a.w2[j] * f1_dgelu(z);
        v = gy * f1_gelu(z);
      } else if (j == a.Hd) {
        v = gy;
      }
      vals[jj * F1_TS + tid] = v;
    }
    __syncthreads();
    {
      const int jj = tid >> 4, part = tid & 15;
      float s = 0.f;
      for (int q = 0; q < 16; ++q) s += vals[jj * F1_TS + part * 16 + q];
      p1[tid] = s;
    }
    __syncthreads();
    if (tid < 16 && j0 + tid <= a.Hd) {
      float s = 0.f;
      for (int q = 0; q < 16; ++q) s += p1[tid * 16 + q];
      out[j0 + tid] = s;
    }
    __syncthreads();
  }
}

extern "C" int ppsci_fno1d_head_pre(int B, int Hd, int n, const float* z, const float* gy, const float* w2, float* gz, float* partials,
                                    void* stream) {
  if (B < 1 || Hd < 1 || n < 1 || !z || !gy || !w2 || !gz || !partials) {
    ppsci_set_error("fno1d_head_pre: invalid argument");
    return PPSCI_E_INVALID;
  }
  F1HeadPreArgs a{z, gy, w2, gz, partials, B, Hd, n, (n + F1_T - 1) / F1_T};
  PPSCI_LAUNCH(fno1d_head_pre_kernel, F1HeadPreArgs, B * a.nchunks, F1_T, 0, stream, a);
  return f1_launch_ok("fno1d_head_pre");
}
