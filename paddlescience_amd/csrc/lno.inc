// lno.inc -- kernels of the Laplace neural operator (ppsci.arch.LNO); included by uno.hip.
//
//   /root/reference/ppsci/arch/lno.py:136-158   Laplace.output_PR   pole-residue transfer function, both einsums
//   /root/reference/ppsci/arch/lno.py:160-187   Laplace.forward     fftn -> steady-state part x1 (ifftn) + transient part x2 (exp)
//   /root/reference/ppsci/arch/lno.py:280-300   LNO.forward_tensor  fc0, InstanceNorm3D, 1x1x1 convolution, fc1 -> act -> fc2
//
// Grid n1 x n2 x n3 (N points), C channels, modes m1 x m2 x m3 (M coefficients), pair = (i, o) of C x C channels.  Tables per
// axis d: A_d[pair][m][p] = 1 / (i omega_d[p] - mu_d[pair][m]), E_d[pair][m][s] = exp(mu_d[pair][m] t_d[s]).
//
//   alpha      = F z                                       lno_dft3 (real in, complex out)
//   H[pair]    = sum_mnk rho A_1 A_2 A_3                   lno_tri_syn on the C x C planes (no batch)
//   x1         = Re F^-1 (sum_i alpha_i H_io)              lno_dft3 (channel mix on load, real part out)
//   Gam[b,i,o] = sum_pqr alpha A_1 A_2 A_3                 lno_tri (analysis)
//   gamma[b,o] = - sum_i rho_io Gam[b,i,o]                 lno_csum
//   x2[b,o']   = 1/N Re sum_o sum_mnk gamma[b,o] E_1 E_2 E_3    lno_tri_syn
//
// Both three-axis contractions are chains of three one-axis products with the plane in LDS; the analysis kernel also runs the
// chain backwards for a given cotangent of its coefficients and leaves dL/dmu_d of ITS (batch, pair) in a partial row, so every
// parameter gradient is a fixed-order sum (ppsci_reduce_rows_multi) -- no atomics anywhere.  Complex planes are stored as
// [plane][2][N] (real plane, imaginary plane): unit-stride LDS and HBM accesses for both parts.  Coefficient tensors are
// [..][M][2].  Every sum runs over its index in ascending order in one thread: results do not depend on the launch geometry.
// At the shapes of the reference's example (B = 50, 39 x 14 x 14, C = 8, 4 x 4 x 4 modes) C is far too small for MFMA to matter:
// plain VALU multiply-add loops on fp32 data with double accumulators (DESIGN.md 4.10 has the measured times).

#define LNO_T 256
// the plane kernels (DFT, analysis, synthesis): one workgroup holds a CU's LDS, so it brings 16 waves to hide the LDS latency of its
// dependent multiply-add chains
#define LNO_TP 1024
// row stride of the [channel][256 points] LDS tiles of the per-point kernels: the reducing threads read the same point of
// different rows at once, which a stride of 256 floats puts into one bank
#define LNO_TS (LNO_T + 1)

struct lno_c {
  float re, im;
};
__device__ __forceinline__ lno_c lno_mul(lno_c a, lno_c b) { return lno_c{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
// Accumulator of the complex sums.  A_d at frequency 0 is 1 / mu_d, 1e2-1e3 times its other entries (1e6 and more for the product
// of three), so the planes hold values of 1e4-1e5 built from O(1) inputs and the parameter gradients are small sums of such
// terms: the sums run in double (the fp32 products are exact in it) and are rounded once, at the store.
struct lno_acc {
  double re, im;
  __device__ __forceinline__ operator lno_c() const { return lno_c{(float)re, (float)im}; }
};
// acc += a * b
__device__ __forceinline__ void lno_fma(lno_acc& acc, lno_c a, lno_c b) {
  acc.re += (double)a.re * (double)b.re - (double)a.im * (double)b.im;
  acc.im += (double)a.re * (double)b.im + (double)a.im * (double)b.re;
}
__device__ __forceinline__ lno_c lno_conj(lno_c a) { return lno_c{a.re, -a.im}; }

static int lno_launch_ok(const char* what) {
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("%s: launch failed", what);
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// ------------------------------------------------------------------------------------------------ tables
struct LnoTablesArgs {
  const float* mu_re[3];
  const float* mu_im[3];
  const float* omega[3];
  const float* t[3];
  float* A[3];
  float* E[3];
  int n[3], m[3];
  int CC;
};

__global__ void __launch_bounds__(LNO_T) lno_tables_kernel(LnoTablesArgs a) {
  for (int d = 0; d < 3; ++d) {
    const int n = a.n[d], m = a.m[d];
    const long long total = (long long)a.CC * m * n;
    for (long long e = (long long)blockIdx.x * LNO_T + threadIdx.x; e < total; e += (long long)gridDim.x * LNO_T) {
      const int p = (int)(e % n);
      const long long pm = e / n;  // pair * m + mode
      const float mr = a.mu_re[d][pm], mi = a.mu_im[d][pm];
      // 1 / (i w - mu) = 1 / (x + i y), x = -mu_r, y = w - mu_i
      const float x = -mr, y = a.omega[d][p] - mi;
      const float inv = 1.f / (x * x + y * y);
      a.A[d][e * 2] = x * inv;
      a.A[d][e * 2 + 1] = -y * inv;
      const float tt = a.t[d][p];
      const float mag = expf(mr * tt);
      a.E[d][e * 2] = mag * cosf(mi * tt);
      a.E[d][e * 2 + 1] = mag * sinf(mi * tt);
    }
  }
}

extern "C" int ppsci_lno_tables(int C, const int* n, const int* m, const float* const* mu_re, const float* const* mu_im,
                                const float* const* omega, const float* const* t, float* const* A, float* const* E, void* stream) {
  if (C < 1 || !n || !m || !mu_re || !mu_im || !omega || !t || !A || !E) {
    ppsci_set_error("lno_tables: invalid argument");
    return PPSCI_E_INVALID;
  }
  LnoTablesArgs a;
  long long most = 0;
  for (int d = 0; d < 3; ++d) {
    if (n[d] < 2 || m[d] < 1 || !mu_re[d] || !mu_im[d] || !omega[d] || !t[d] || !A[d] || !E[d]) {
      ppsci_set_error("lno_tables: invalid argument (axis %d)", d);
      return PPSCI_E_INVALID;
    }
    a.mu_re[d] = mu_re[d], a.mu_im[d] = mu_im[d], a.omega[d] = omega[d], a.t[d] = t[d], a.A[d] = A[d], a.E[d] = E[d];
    a.n[d] = n[d], a.m[d] = m[d];
    const long long tot = (long long)C * C * m[d] * n[d];
    most = tot > most ? tot : most;
  }
  a.CC = C * C;
  long long grid = (most + LNO_T - 1) / LNO_T;
  if (grid > 1024) grid = 1024;
  PPSCI_LAUNCH(lno_tables_kernel, LnoTablesArgs, (int)grid, LNO_T, 0, stream, a);
  return lno_launch_ok("lno_tables");
}

// ------------------------------------------------------------------------------------------------ dense 3-D DFT of a plane in LDS
struct LnoDftArgs {
  const float* in;    // real planes [planes][N], complex planes [planes][2][N]; the MIX source alpha [nb * C][2][N]
  const float* H;     // MIX: [C*C][2][N]
  const float* add;   // MIX: complex planes [planes][2][N] added behind the mix, or NULL
  const float* tw;    // [n1 + n2 + n3][2]: (cos, sin)(2 pi k / n_d), computed in double on the host
  float* out;         // real [planes][N] or complex [planes][2][N]
  int n1, n2, n3, planes;
  int in_mode;        // 0 real, 1 complex, 2 MIX: X[f] = mix_scale * sum_c2 alpha[b, c2][f] * (conj) H[cp*pair_cp + c2*pair_c2][f] (+ add)
  int C, pair_cp, pair_c2, conj_h;
  float mix_scale;
  int sign;           // -1: e^{-i..} (forward), +1: e^{+i..} (adjoint / inverse)
  int out_real, accumulate;
  float out_scale;
  int zero_dc;        // 1: element 0 of the INPUT plane (a spectrum) is taken as 0; 2: element 0 of the OUTPUT plane (a spectrum) is written as 0
};

__global__ void __launch_bounds__(LNO_TP) lno_dft3_kernel(LnoDftArgs a) {
  PPSCI_DYN_SMEM(smem);
  const int N = a.n1 * a.n2 * a.n3;
  float* buf[2][2] = {{smem, smem + N}, {smem + 2 * N, smem + 3 * N}};
  float* tw = smem + 4 * N;
  const int tid = threadIdx.x;
  const int ntw = a.n1 + a.n2 + a.n3;
  const float sg = a.sign < 0 ? -1.f : 1.f;
  for (int i = tid; i < ntw; i += LNO_TP) {
    tw[2 * i] = a.tw[2 * i];
    tw[2 * i + 1] = sg * a.tw[2 * i + 1];
  }
  for (int pl = blockIdx.x; pl < a.planes; pl += gridDim.x) {
    __syncthreads();  // the buffers change hands between planes; the twiddles are complete
    if (a.in_mode == 0) {
      const float* x = a.in + (long long)pl * N;
      for (int f = tid; f < N; f += LNO_TP) buf[0][0][f] = x[f], buf[0][1][f] = 0.f;
    } else if (a.in_mode == 1) {
      const float* x = a.in + (long long)pl * 2 * N;
      for (int f = tid; f < N; f += LNO_TP) buf[0][0][f] = x[f], buf[0][1][f] = x[N + f];
    } else {
      const int b = pl / a.C, cp = pl - b * a.C;
      for (int f = tid; f < N; f += LNO_TP) {
        lno_acc s{0., 0.};
        for (int c2 = 0; c2 < a.C; ++c2) {
          const float* al = a.in + ((long long)b * a.C + c2) * 2 * N;
          const float* h = a.H + (long long)(cp * a.pair_cp + c2 * a.pair_c2) * 2 * N;
          lno_c hv{h[f], h[N + f]};
          if (a.conj_h) hv.im = -hv.im;
          lno_fma(s, lno_c{al[f], al[N + f]}, hv);
        }
        s.re *= a.mix_scale, s.im *= a.mix_scale;
        if (a.add) {
          const float* ad = a.add + (long long)pl * 2 * N;
          s.re += ad[f], s.im += ad[N + f];
        }
        buf[0][0][f] = s.re, buf[0][1][f] = s.im;
      }
    }
    if (a.zero_dc == 1 && tid == 0) buf[0][0][0] = 0.f, buf[0][1][0] = 0.f;  // (thread 0 loaded element 0 itself)
    __syncthreads();
    int cur = 0;
    for (int d = 0; d < 3; ++d) {
      const int n = d == 0 ? a.n1 : (d == 1 ? a.n2 : a.n3);
      const int stride = d == 0 ? a.n2 * a.n3 : (d == 1 ? a.n3 : 1);
      const float* w = tw + 2 * (d == 0 ? 0 : (d == 1 ? a.n1 : a.n1 + a.n2));
      const float* sr = buf[cur][0];
      const float* si = buf[cur][1];
      float* dr = buf[cur ^ 1][0];
      float* di = buf[cur ^ 1][1];
      for (int f = tid; f < N; f += LNO_TP) {
        const int p = (f / stride) % n;
        const int base = f - p * stride;
        lno_acc s{0., 0.};
        int k = 0;  // (p * j) mod n
        for (int j = 0; j < n; ++j) {
          lno_fma(s, lno_c{sr[base + j * stride], si[base + j * stride]}, lno_c{w[2 * k], w[2 * k + 1]});
          k += p;
          if (k >= n) k -= n;
        }
        dr[f] = s.re, di[f] = s.im;
      }
      __syncthreads();
      cur ^= 1;
    }
    if (a.out_real) {
      float* y = a.out + (long long)pl * N;
      for (int f = tid; f < N; f += LNO_TP) {
        const float v = buf[cur][0][f] * a.out_scale;
        y[f] = a.accumulate ? y[f] + v : v;
      }
    } else {
      float* y = a.out + (long long)pl * 2 * N;
      for (int f = tid; f < N; f += LNO_TP) {
        const bool z = a.zero_dc == 2 && f == 0;
        y[f] = z ? 0.f : buf[cur][0][f] * a.out_scale, y[N + f] = z ? 0.f : buf[cur][1][f] * a.out_scale;
      }
    }
  }
}

static long long lno_dft_lds(int n1, int n2, int n3) { return (4ll * n1 * n2 * n3 + 2ll * (n1 + n2 + n3)) * 4; }

extern "C" int ppsci_lno_dft3(int planes, int n1, int n2, int n3, int in_mode, const float* in, int C, const float* H, int pair_cp,
                              int pair_c2, int conj_h, float mix_scale, const float* add, const float* tw, int sign, int out_real,
                              int accumulate, float out_scale, int zero_dc, float* out, void* stream) {
  if (planes < 1 || n1 < 1 || n2 < 1 || n3 < 1 || !in || !tw || !out || in_mode < 0 || in_mode > 2 || (sign != 1 && sign != -1) ||
      (in_mode == 2 && (!H || C < 1 || planes % C != 0)) || (accumulate && !out_real) || zero_dc < 0 || zero_dc > 2 || (zero_dc == 2 && out_real)) {
    ppsci_set_error("lno_dft3: invalid argument");
    return PPSCI_E_INVALID;
  }
  const long long lds = lno_dft_lds(n1, n2, n3);
  if (lds > PPSCI_LDS_LIMIT_BYTES - 1024) {
    ppsci_set_error("lno_dft3: a %d x %d x %d complex plane and its copy do not fit LDS", n1, n2, n3);
    return PPSCI_E_UNSUPPORTED;
  }
  if (PPSCI_SET_MAX_LDS(lno_dft3_kernel, lds) != 0) {
    ppsci_set_error("lno_dft3: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  LnoDftArgs a{in, H, add, tw, out, n1, n2, n3, planes, in_mode, C, pair_cp, pair_c2, conj_h ? 1 : 0, mix_scale, sign,
               out_real ? 1 : 0, accumulate ? 1 : 0, out_scale, zero_dc};
  const int grid = planes < 4 * PPSCI_NUM_CU ? planes : 4 * PPSCI_NUM_CU;
  PPSCI_LAUNCH(lno_dft3_kernel, LnoDftArgs, grid, LNO_TP, (int)lds, stream, a);
  return lno_launch_ok("lno_dft3");
}

// ------------------------------------------------------------------------------------------------ three-axis contractions
struct LnoTriArgs {
  const float* X;       // analysis: planes [nb * ncp] (complex [2][N], or real [N] with x_real)
  const float* T[3];    // tables [C*C][m_d][n_d][2]
  const float* tg[3];   // grids t_d (kind 1)
  int n[3], m[3];
  int nb, ncp, nc2;
  int pair_cp, pair_c2;          // pair = cp * pair_cp + c2 * pair_c2
  int x_real, conj_t;
  float* G;                      // analysis: [(plane * nc2 + c2)][M][2] or NULL
  // coefficients c[mnk] = gscale * coef[b * coef_b + cp * coef_cp + c2 * coef_c2][mnk] * (conj) mult[pair][mnk]; a NULL factor is 1
  const float* coef;
  int coef_b, coef_cp, coef_c2;
  const float* mult_re;
  const float* mult_im;
  int mult_conj;
  float gscale;
  // analysis with adjoint: dL/dmu_d partial rows [rows][CC * m_d], row = row0 + b
  int adjoint, kind;             // kind 0: dT/dmu = T^2 (A tables), 1: dT/dmu = t T (E tables)
  float* mu_re[3];
  float* mu_im[3];
  int row0, CC;
  // synthesis output
  float* out;                    // real [planes][N] or complex [planes][2][N]
  int out_real, accumulate;
  float out_scale;
};

__device__ __forceinline__ lno_c lno_coef(const LnoTriArgs& a, int b, int cp, int c2, int pair, int e, int M) {
  lno_c c{a.gscale, 0.f};
  if (a.coef) {
    const float* q = a.coef + ((long long)(b * a.coef_b + cp * a.coef_cp + c2 * a.coef_c2) * M + e) * 2;
    c = lno_c{a.gscale * q[0], a.gscale * q[1]};
  }
  if (a.mult_re) {
    lno_c r{a.mult_re[(long long)pair * M + e], a.mult_im[(long long)pair * M + e]};
    if (a.mult_conj) r.im = -r.im;
    c = lno_mul(c, r);
  }
  return c;
}

// LDS (floats): matrices 2 * sum m_d n_d | (analysis) X 2N, S1, S12, Gb, S12b, S1b, Mbar | (synthesis) acc 2N, c, U3, U2
struct LnoTriLds {
  int mat[3], x, s1, s12, gb, s12b, s1b, mbar[3], total;
};
__host__ __device__ static inline LnoTriLds lno_tri_layout(const int* n, const int* m) {
  LnoTriLds L;
  int o = 0;
  for (int d = 0; d < 3; ++d) L.mat[d] = o, o += 2 * m[d] * n[d];
  L.x = o, o += 2 * n[0] * n[1] * n[2];
  L.s1 = o, o += 2 * m[0] * n[1] * n[2];
  L.s12 = o, o += 2 * m[0] * m[1] * n[2];
  L.gb = o, o += 2 * m[0] * m[1] * m[2];
  L.s12b = o, o += 2 * m[0] * m[1] * n[2];
  L.s1b = o, o += 2 * m[0] * n[1] * n[2];
  for (int d = 0; d < 3; ++d) L.mbar[d] = o, o += 2 * m[d] * n[d];
  L.total = o;
  return L;
}

__device__ __forceinline__ void lno_load_mats(const LnoTriArgs& a, const LnoTriLds& L, float* smem, int pair) {
  for (int d = 0; d < 3; ++d) {
    const int cnt = a.m[d] * a.n[d];
    const float* T = a.T[d] + (long long)pair * cnt * 2;
    float* M = smem + L.mat[d];
    for (int e = threadIdx.x; e < cnt; e += LNO_TP) {
      M[e] = T[2 * e];
      M[cnt + e] = a.conj_t ? -T[2 * e + 1] : T[2 * e + 1];
    }
  }
}

// Analysis G[mnk] = sum_pqr M1[m,p] M2[n,q] M3[k,r] X[pqr] per (plane, c2), M_d = (conj) T_d[pair]; with `adjoint` also the reverse
// chain for the cotangent c[mnk] of G: dL/dM_d, folded into dL/dmu_d.
__global__ void __launch_bounds__(LNO_TP) lno_tri_kernel(LnoTriArgs a) {
  PPSCI_DYN_SMEM(smem);
  const LnoTriLds L = lno_tri_layout(a.n, a.m);
  const int n1 = a.n[0], n2 = a.n[1], n3 = a.n[2], m1 = a.m[0], m2 = a.m[1], m3 = a.m[2];
  const int N = n1 * n2 * n3, M = m1 * m2 * m3, n23 = n2 * n3;
  const int tid = threadIdx.x;
  float *Xr = smem + L.x, *Xi = Xr + N;
  float *S1r = smem + L.s1, *S1i = S1r + m1 * n23;
  float *S12r = smem + L.s12, *S12i = S12r + m1 * m2 * n3;
  float *Gbr = smem + L.gb, *Gbi = Gbr + M;
  float *S12br = smem + L.s12b, *S12bi = S12br + m1 * m2 * n3;
  float *S1br = smem + L.s1b, *S1bi = S1br + m1 * n23;
  const float *M1r = smem + L.mat[0], *M1i = M1r + m1 * n1;
  const float *M2r = smem + L.mat[1], *M2i = M2r + m2 * n2;
  const float *M3r = smem + L.mat[2], *M3i = M3r + m3 * n3;
  const int planes = a.nb * a.ncp;
  for (int pl = blockIdx.x; pl < planes; pl += gridDim.x) {
    const int b = pl / a.ncp, cp = pl - b * a.ncp;
    __syncthreads();
    if (a.x_real) {
      const float* x = a.X + (long long)pl * N;
      for (int f = tid; f < N; f += LNO_TP) Xr[f] = x[f], Xi[f] = 0.f;
    } else {
      const float* x = a.X + (long long)pl * 2 * N;
      for (int f = tid; f < N; f += LNO_TP) Xr[f] = x[f], Xi[f] = x[N + f];
    }
    for (int c2 = 0; c2 < a.nc2; ++c2) {
      const int pair = cp * a.pair_cp + c2 * a.pair_c2;
      __syncthreads();  // the previous iteration's readers of the matrices and intermediates are done
      lno_load_mats(a, L, smem, pair);
      __syncthreads();
      for (int e = tid; e < m1 * n23; e += LNO_TP) {  // S1[m, q, r] = sum_p M1[m, p] X[p, q, r]
        const int m = e / n23, qr = e - m * n23;
        lno_acc s{0., 0.};
        for (int p = 0; p < n1; ++p) lno_fma(s, lno_c{M1r[m * n1 + p], M1i[m * n1 + p]}, lno_c{Xr[p * n23 + qr], Xi[p * n23 + qr]});
        S1r[e] = s.re, S1i[e] = s.im;
      }
      __syncthreads();
      for (int e = tid; e < m1 * m2 * n3; e += LNO_TP) {  // S12[m, n, r] = sum_q M2[n, q] S1[m, q, r]
        const int r = e % n3, mn = e / n3, nn = mn % m2, m = mn / m2;
        lno_acc s{0., 0.};
        for (int q = 0; q < n2; ++q)
          lno_fma(s, lno_c{M2r[nn * n2 + q], M2i[nn * n2 + q]}, lno_c{S1r[(m * n2 + q) * n3 + r], S1i[(m * n2 + q) * n3 + r]});
        S12r[e] = s.re, S12i[e] = s.im;
      }
      __syncthreads();
      for (int e = tid; e < M; e += LNO_TP) {  // G[m, n, k] = sum_r M3[k, r] S12[m, n, r]
        const int k = e % m3, mn = e / m3;
        if (a.G) {
          lno_acc s{0., 0.};
          for (int r = 0; r < n3; ++r) lno_fma(s, lno_c{M3r[k * n3 + r], M3i[k * n3 + r]}, lno_c{S12r[mn * n3 + r], S12i[mn * n3 + r]});
          float* g = a.G + (((long long)pl * a.nc2 + c2) * M + e) * 2;
          g[0] = s.re, g[1] = s.im;
        }
        if (a.adjoint) {
          const lno_c c = lno_coef(a, b, cp, c2, pair, e, M);
          Gbr[e] = c.re, Gbi[e] = c.im;
        }
      }
      if (!a.adjoint) continue;
      __syncthreads();
      float *B1r = smem + L.mbar[0], *B1i = B1r + m1 * n1;
      float *B2r = smem + L.mbar[1], *B2i = B2r + m2 * n2;
      float *B3r = smem + L.mbar[2], *B3i = B3r + m3 * n3;
      for (int e = tid; e < m3 * n3; e += LNO_TP) {  // M3bar[k, r] = sum_mn conj(S12[m, n, r]) Gbar[m, n, k]
        const int k = e / n3, r = e - k * n3;
        lno_acc s{0., 0.};
        for (int mn = 0; mn < m1 * m2; ++mn) lno_fma(s, lno_c{S12r[mn * n3 + r], -S12i[mn * n3 + r]}, lno_c{Gbr[mn * m3 + k], Gbi[mn * m3 + k]});
        B3r[e] = s.re, B3i[e] = s.im;
      }
      for (int e = tid; e < m1 * m2 * n3; e += LNO_TP) {  // S12bar[m, n, r] = sum_k conj(M3[k, r]) Gbar[m, n, k]
        const int r = e % n3, mn = e / n3;
        lno_acc s{0., 0.};
        for (int k = 0; k < m3; ++k) lno_fma(s, lno_c{M3r[k * n3 + r], -M3i[k * n3 + r]}, lno_c{Gbr[mn * m3 + k], Gbi[mn * m3 + k]});
        S12br[e] = s.re, S12bi[e] = s.im;
      }
      __syncthreads();
      for (int e = tid; e < m2 * n2; e += LNO_TP) {  // M2bar[n, q] = sum_{m, r} conj(S1[m, q, r]) S12bar[m, n, r]
        const int nn = e / n2, q = e - nn * n2;
        lno_acc s{0., 0.};
        for (int m = 0; m < m1; ++m)
          for (int r = 0; r < n3; ++r)
            lno_fma(s, lno_c{S1r[(m * n2 + q) * n3 + r], -S1i[(m * n2 + q) * n3 + r]},
                    lno_c{S12br[(m * m2 + nn) * n3 + r], S12bi[(m * m2 + nn) * n3 + r]});
        B2r[e] = s.re, B2i[e] = s.im;
      }
      for (int e = tid; e < m1 * n23; e += LNO_TP) {  // S1bar[m, q, r] = sum_n conj(M2[n, q]) S12bar[m, n, r]
        const int r = e % n3, mq = e / n3, q = mq % n2, m = mq / n2;
        lno_acc s{0., 0.};
        for (int nn = 0; nn < m2; ++nn)
          lno_fma(s, lno_c{M2r[nn * n2 + q], -M2i[nn * n2 + q]}, lno_c{S12br[(m * m2 + nn) * n3 + r], S12bi[(m * m2 + nn) * n3 + r]});
        S1br[e] = s.re, S1bi[e] = s.im;
      }
      __syncthreads();
      for (int e = tid; e < m1 * n1; e += LNO_TP) {  // M1bar[m, p] = sum_qr conj(X[p, q, r]) S1bar[m, q, r]
        const int m = e / n1, p = e - m * n1;
        lno_acc s{0., 0.};
        for (int qr = 0; qr < n23; ++qr) lno_fma(s, lno_c{Xr[p * n23 + qr], -Xi[p * n23 + qr]}, lno_c{S1br[m * n23 + qr], S1bi[m * n23 + qr]});
        B1r[e] = s.re, B1i[e] = s.im;
      }
      __syncthreads();
      // dL/dmu_d[m] = sum_p conj(dT/dmu[m, p]) Tbar[m, p];  T = (conj) M, Tbar = (conj) Mbar
      for (int e = tid; e < m1 + m2 + m3; e += LNO_TP) {
        const int d = e < m1 ? 0 : (e < m1 + m2 ? 1 : 2);
        const int m = e - (d == 0 ? 0 : (d == 1 ? m1 : m1 + m2));
        const int n = a.n[d], md = a.m[d];
        const float *Mr = smem + L.mat[d], *Mi = Mr + md * n;
        const float *Br = smem + L.mbar[d], *Bi = Br + md * n;
        lno_acc s{0., 0.};
        for (int p = 0; p < n; ++p) {
          lno_c T{Mr[m * n + p], Mi[m * n + p]}, Tb{Br[m * n + p], Bi[m * n + p]};
          if (a.conj_t) T.im = -T.im, Tb.im = -Tb.im;
          lno_c dT = a.kind == 0 ? lno_mul(T, T) : lno_c{a.tg[d][p] * T.re, a.tg[d][p] * T.im};
          lno_fma(s, lno_conj(dT), Tb);
        }
        const long long at = (long long)(a.row0 + b) * a.CC * md + (long long)pair * md + m;
        a.mu_re[d][at] = s.re;
        a.mu_im[d][at] = s.im;
      }
    }
  }
}

// Synthesis out[pqr] (+)= out_scale * sum_c2 sum_mnk c[mnk] M1[m,p] M2[n,q] M3[k,r] per plane (the real part with out_real).
__global__ void __launch_bounds__(LNO_TP) lno_tri_syn_kernel(LnoTriArgs a) {
  PPSCI_DYN_SMEM(smem);
  const LnoTriLds L = lno_tri_layout(a.n, a.m);
  const int n1 = a.n[0], n2 = a.n[1], n3 = a.n[2], m1 = a.m[0], m2 = a.m[1], m3 = a.m[2];
  const int N = n1 * n2 * n3, M = m1 * m2 * m3, n23 = n2 * n3;
  const int tid = threadIdx.x;
  float *Ar = smem + L.x, *Ai = Ar + N;  // accumulated plane
  float *U2r = smem + L.s1, *U2i = U2r + m1 * n23;
  float *U3r = smem + L.s12, *U3i = U3r + m1 * m2 * n3;
  float *Cr = smem + L.gb, *Ci = Cr + M;
  const float *M1r = smem + L.mat[0], *M1i = M1r + m1 * n1;
  const float *M2r = smem + L.mat[1], *M2i = M2r + m2 * n2;
  const float *M3r = smem + L.mat[2], *M3i = M3r + m3 * n3;
  const int planes = a.nb * a.ncp;
  for (int pl = blockIdx.x; pl < planes; pl += gridDim.x) {
    const int b = pl / a.ncp, cp = pl - b * a.ncp;
    __syncthreads();
    for (int f = tid; f < N; f += LNO_TP) Ar[f] = 0.f, Ai[f] = 0.f;
    for (int c2 = 0; c2 < a.nc2; ++c2) {
      const int pair = cp * a.pair_cp + c2 * a.pair_c2;
      __syncthreads();
      lno_load_mats(a, L, smem, pair);
      for (int e = tid; e < M; e += LNO_TP) {
        const lno_c c = lno_coef(a, b, cp, c2, pair, e, M);
        Cr[e] = c.re, Ci[e] = c.im;
      }
      __syncthreads();
      for (int e = tid; e < m1 * m2 * n3; e += LNO_TP) {  // U3[m, n, r] = sum_k M3[k, r] c[m, n, k]
        const int r = e % n3, mn = e / n3;
        lno_acc s{0., 0.};
        for (int k = 0; k < m3; ++k) lno_fma(s, lno_c{M3r[k * n3 + r], M3i[k * n3 + r]}, lno_c{Cr[mn * m3 + k], Ci[mn * m3 + k]});
        U3r[e] = s.re, U3i[e] = s.im;
      }
      __syncthreads();
      for (int e = tid; e < m1 * n23; e += LNO_TP) {  // U2[m, q, r] = sum_n M2[n, q] U3[m, n, r]
        const int r = e % n3, mq = e / n3, q = mq % n2, m = mq / n2;
        lno_acc s{0., 0.};
        for (int nn = 0; nn < m2; ++nn)
          lno_fma(s, lno_c{M2r[nn * n2 + q], M2i[nn * n2 + q]}, lno_c{U3r[(m * m2 + nn) * n3 + r], U3i[(m * m2 + nn) * n3 + r]});
        U2r[e] = s.re, U2i[e] = s.im;
      }
      __syncthreads();
      for (int f = tid; f < N; f += LNO_TP) {  // plane[p, q, r] += sum_m M1[m, p] U2[m, q, r]  (this thread owns point f)
        const int p = f / n23, qr = f - p * n23;
        lno_acc s{Ar[f], Ai[f]};
        for (int m = 0; m < m1; ++m) lno_fma(s, lno_c{M1r[m * n1 + p], M1i[m * n1 + p]}, lno_c{U2r[m * n23 + qr], U2i[m * n23 + qr]});
        Ar[f] = s.re, Ai[f] = s.im;
      }
    }
    if (a.out_real) {
      float* y = a.out + (long long)pl * N;
      for (int f = tid; f < N; f += LNO_TP) {
        const float v = Ar[f] * a.out_scale;
        y[f] = a.accumulate ? y[f] + v : v;
      }
    } else {
      float* y = a.out + (long long)pl * 2 * N;
      for (int f = tid; f < N; f += LNO_TP) y[f] = Ar[f] * a.out_scale, y[N + f] = Ai[f] * a.out_scale;
    }
  }
}

extern "C" int ppsci_lno_supported(int n1, int n2, int n3, int m1, int m2, int m3) {
  if (n1 < 2 || n2 < 2 || n3 < 2 || m1 < 1 || m2 < 1 || m3 < 1) return 0;
  const int n[3] = {n1, n2, n3}, m[3] = {m1, m2, m3};
  const long long tri = (long long)lno_tri_layout(n, m).total * 4;
  const long long lim = PPSCI_LDS_LIMIT_BYTES - 1024;
  return (lno_dft_lds(n1, n2, n3) <= lim && tri <= lim && (long long)n1 * n2 * n3 < (1ll << 24)) ? 1 : 0;
}

static int lno_tri_fill(LnoTriArgs& a, const char* what, const ppsci_lno_tri_desc* d, const float* const* T, const float* coef,
                        const float* mult_re, const float* mult_im) {
  if (!d || !T || d->nb < 1 || d->ncp < 1 || d->nc2 < 1 || d->C < 1 || (mult_re == nullptr) != (mult_im == nullptr)) {
    ppsci_set_error("%s: invalid argument", what);
    return PPSCI_E_INVALID;
  }
  if (!ppsci_lno_supported(d->n[0], d->n[1], d->n[2], d->m[0], d->m[1], d->m[2])) {
    ppsci_set_error("%s: a %d x %d x %d plane with %d x %d x %d modes does not fit LDS", what, d->n[0], d->n[1], d->n[2], d->m[0],
                    d->m[1], d->m[2]);
    return PPSCI_E_UNSUPPORTED;
  }
  // every pair index the launch forms must address a table entry
  const long long top = (long long)(d->ncp - 1) * d->pair_cp + (long long)(d->nc2 - 1) * d->pair_c2;
  if (d->pair_cp < 0 || d->pair_c2 < 0 || top >= (long long)d->C * d->C) {
    ppsci_set_error("%s: pair index out of range", what);
    return PPSCI_E_INVALID;
  }
  a = LnoTriArgs{};
  for (int k = 0; k < 3; ++k) {
    if (!T[k]) {
      ppsci_set_error("%s: invalid argument (table %d)", what, k);
      return PPSCI_E_INVALID;
    }
    a.T[k] = T[k], a.n[k] = d->n[k], a.m[k] = d->m[k];
  }
  a.nb = d->nb, a.ncp = d->ncp, a.nc2 = d->nc2, a.pair_cp = d->pair_cp, a.pair_c2 = d->pair_c2, a.conj_t = d->conj_t ? 1 : 0;
  a.coef = coef, a.coef_b = d->coef_b, a.coef_cp = d->coef_cp, a.coef_c2 = d->coef_c2;
  a.mult_re = mult_re, a.mult_im = mult_im, a.mult_conj = d->mult_conj ? 1 : 0, a.gscale = d->gscale;
  a.CC = d->C * d->C;
  return PPSCI_OK;
}

static int lno_tri_launch(bool syn, LnoTriArgs& a, void* stream) {
  const long long lds = (long long)lno_tri_layout(a.n, a.m).total * 4;
  const int planes = a.nb * a.ncp;
  const int grid = planes < 4 * PPSCI_NUM_CU ? planes : 4 * PPSCI_NUM_CU;
  if (syn) {
    if (PPSCI_SET_MAX_LDS(lno_tri_syn_kernel, lds) != 0) {
      ppsci_set_error("lno_synthesis: cannot raise dynamic LDS to %lld B", lds);
      return PPSCI_E_LAUNCH;
    }
    PPSCI_LAUNCH(lno_tri_syn_kernel, LnoTriArgs, grid, LNO_TP, (int)lds, stream, a);
    return lno_launch_ok("lno_synthesis");
  }
  if (PPSCI_SET_MAX_LDS(lno_tri_kernel, lds) != 0) {
    ppsci_set_error("lno_analysis: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  PPSCI_LAUNCH(lno_tri_kernel, LnoTriArgs, grid, LNO_TP, (int)lds, stream, a);
  return lno_launch_ok("lno_analysis");
}

extern "C" int ppsci_lno_analysis(const ppsci_lno_tri_desc* d, const float* X, int x_real, const float* const* T, float* G,
                                  const float* coef, const float* mult_re, const float* mult_im, int kind, const float* const* tg,
                                  float* const* mu_re, float* const* mu_im, int row0, void* stream) {
  LnoTriArgs a;
  const int rc = lno_tri_fill(a, "lno_analysis", d, T, coef, mult_re, mult_im);
  if (rc != PPSCI_OK) return rc;
  const bool adj = mu_re != nullptr;
  if (!X || (!G && !adj) || (adj && (!mu_im || row0 < 0 || (kind != 0 && kind != 1) || (kind == 1 && !tg)))) {
    ppsci_set_error("lno_analysis: invalid argument");
    return PPSCI_E_INVALID;
  }
  a.X = X, a.x_real = x_real ? 1 : 0, a.G = G, a.adjoint = adj ? 1 : 0, a.kind = kind, a.row0 = row0;
  for (int k = 0; k < 3 && adj; ++k) {
    if (!mu_re[k] || !mu_im[k] || (kind == 1 && !tg[k])) {
      ppsci_set_error("lno_analysis: invalid argument (gradient rows %d)", k);
      return PPSCI_E_INVALID;
    }
    a.mu_re[k] = mu_re[k], a.mu_im[k] = mu_im[k], a.tg[k] = kind == 1 ? tg[k] : nullptr;
  }
  return lno_tri_launch(false, a, stream);
}

extern "C" int ppsci_lno_synthesis(const ppsci_lno_tri_desc* d, const float* const* T, const float* coef, const float* mult_re,
                                   const float* mult_im, int out_real, int accumulate, float out_scale, float* out, void* stream) {
  LnoTriArgs a;
  const int rc = lno_tri_fill(a, "lno_synthesis", d, T, coef, mult_re, mult_im);
  if (rc != PPSCI_OK) return rc;
  if (!out || (!coef && !mult_re) || (accumulate && !out_real)) {
    ppsci_set_error("lno_synthesis: invalid argument");
    return PPSCI_E_INVALID;
  }
  a.out = out, a.out_real = out_real ? 1 : 0, a.accumulate = accumulate ? 1 : 0, a.out_scale = out_scale;
  return lno_tri_launch(true, a, stream);
}

// ------------------------------------------------------------------------------------------------ small channel sums
struct LnoSumArgs {
  const float* src;      // [(b * C + j) * C + o][M][2]
  const float* mult_re;  // [(j * C + o)][M] or NULL
  const float* mult_im;
  float* dst;            // [(b * C + o)][M][2]
  int B, C, M;
  float scale;
};
// dst[b, o] = scale * sum_j src[b, j, o] * mult[j, o]
__global__ void __launch_bounds__(LNO_T) lno_csum_kernel(LnoSumArgs a) {
  const long long total = (long long)a.B * a.C * a.M;
  for (long long t = (long long)blockIdx.x * LNO_T + threadIdx.x; t < total; t += (long long)gridDim.x * LNO_T) {
    const int e = (int)(t % a.M);
    const long long bo = t / a.M;
    const int o = (int)(bo % a.C);
    const long long b = bo / a.C;
    lno_acc s{0., 0.};
    for (int j = 0; j < a.C; ++j) {
      const float* q = a.src + ((((long long)b * a.C + j) * a.C + o) * a.M + e) * 2;
      lno_c r{1.f, 0.f};
      if (a.mult_re) r = lno_c{a.mult_re[((long long)j * a.C + o) * a.M + e], a.mult_im[((long long)j * a.C + o) * a.M + e]};
      lno_fma(s, lno_c{q[0], q[1]}, r);
    }
    a.dst[t * 2] = a.scale * s.re;
    a.dst[t * 2 + 1] = a.scale * s.im;
  }
}

extern "C" int ppsci_lno_channel_sum(int B, int C, int M, const float* src, const float* mult_re, const float* mult_im, float scale,
                                     float* dst, void* stream) {
  if (B < 1 || C < 1 || M < 1 || !src || !dst || (mult_re == nullptr) != (mult_im == nullptr)) {
    ppsci_set_error("lno_channel_sum: invalid argument");
    return PPSCI_E_INVALID;
  }
  LnoSumArgs a{src, mult_re, mult_im, dst, B, C, M, scale};
  long long grid = ((long long)B * C * M + LNO_T - 1) / LNO_T;
  if (grid > 1024) grid = 1024;
  PPSCI_LAUNCH(lno_csum_kernel, LnoSumArgs, (int)grid, LNO_T, 0, stream, a);
  return lno_launch_ok("lno_channel_sum");
}

struct LnoRhoArgs {
  const float* Gam;   // [(b * C + i) * C + o][M][2]
  const float* gbar;  // [(b * C + o)][M][2]
  const float* Gp;    // [(i * C + o)][M][2]
  float* g_re;        // [(i * C + o)][M]
  float* g_im;
  int B, C, M;
};
// d rho[i, o] = Gp[i, o] - sum_b conj(Gam[b, i, o]) gbar[b, o]
__global__ void __launch_bounds__(LNO_T) lno_rho_grad_kernel(LnoRhoArgs a) {
  const long long total = (long long)a.C * a.C * a.M;
  for (long long t = (long long)blockIdx.x * LNO_T + threadIdx.x; t < total; t += (long long)gridDim.x * LNO_T) {
    const int e = (int)(t % a.M);
    const long long io = t / a.M;
    const int o = (int)(io % a.C);
    lno_acc s{0., 0.};
    for (int b = 0; b < a.B; ++b) {
      const float* g = a.Gam + (((long long)b * a.C * a.C + io) * a.M + e) * 2;
      const float* q = a.gbar + ((((long long)b * a.C + o) * a.M) + e) * 2;
      lno_fma(s, lno_c{g[0], -g[1]}, lno_c{q[0], q[1]});
    }
    a.g_re[t] = a.Gp[t * 2] - s.re;
    a.g_im[t] = a.Gp[t * 2 + 1] - s.im;
  }
}

extern "C" int ppsci_lno_rho_grad(int B, int C, int M, const float* Gam, const float* gbar, const float* Gp, float* g_re, float* g_im,
                                  void* stream) {
  if (B < 1 || C < 1 || M < 1 || !Gam || !gbar || !Gp || !g_re || !g_im) {
    ppsci_set_error("lno_rho_grad: invalid argument");
    return PPSCI_E_INVALID;
  }
  LnoRhoArgs a{Gam, gbar, Gp, g_re, g_im, B, C, M};
  long long grid = ((long long)C * C * M + LNO_T - 1) / LNO_T;
  if (grid > 1024) grid = 1024;
  PPSCI_LAUNCH(lno_rho_grad_kernel, LnoRhoArgs, (int)grid, LNO_T, 0, stream, a);
  return lno_launch_ok("lno_rho_grad");
}

struct LnoHbarArgs {
  const float* alpha;  // [(b * C + i)][2][N]
  const float* ghat;   // [(b * C + o)][2][N]
  float* hbar;         // [(i * C + o)][2][N]
  int B, C, N;
  float scale;
};
// Hbar[i, o][f] = scale * sum_b conj(alpha[b, i][f]) ghat[b, o][f]
__global__ void __launch_bounds__(LNO_T) lno_hbar_kernel(LnoHbarArgs a) {
  const long long total = (long long)a.C * a.C * a.N;
  for (long long t = (long long)blockIdx.x * LNO_T + threadIdx.x; t < total; t += (long long)gridDim.x * LNO_T) {
    const int f = (int)(t % a.N);
    const int io = (int)(t / a.N);
    const int i = io / a.C, o = io - i * a.C;
    lno_acc s{0., 0.};
    for (int b = 0; b < a.B; ++b) {
      const float* al = a.alpha + ((long long)b * a.C + i) * 2 * a.N;
      const float* g = a.ghat + ((long long)b * a.C + o) * 2 * a.N;
      lno_fma(s, lno_c{al[f], -al[a.N + f]}, lno_c{g[f], g[a.N + f]});
    }
    a.hbar[(long long)io * 2 * a.N + f] = a.scale * s.re;
    a.hbar[(long long)io * 2 * a.N + a.N + f] = a.scale * s.im;
  }
}

extern "C" int ppsci_lno_hbar(int B, int C, int N, const float* alpha, const float* ghat, float scale, float* hbar, void* stream) {
  if (B < 1 || C < 1 || N < 1 || !alpha || !ghat || !hbar) {
    ppsci_set_error("lno_hbar: invalid argument");
    return PPSCI_E_INVALID;
  }
  LnoHbarArgs a{alpha, ghat, hbar, B, C, N, scale};
  long long grid = ((long long)C * C * N + LNO_T - 1) / LNO_T;
  if (grid > 8192) grid = 8192;
  PPSCI_LAUNCH(lno_hbar_kernel, LnoHbarArgs, (int)grid, LNO_T, 0, stream, a);
  return lno_launch_ok("lno_hbar");
}

// ------------------------------------------------------------------------------------------------ instance norm
// sum of one value per thread over the workgroup, in a fixed tree order; every thread gets the result.  The statistics run in
// double: the planes the second norm sees hold values of 1e4-1e5, and the reverse subtracts two projections from the gradient,
// which leaves a small remainder of large numbers.
__device__ __forceinline__ double lno_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = LNO_T / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

struct LnoNormArgs {
  const float* x;    // forward: input planes; reverse: the normalised OUTPUT planes
  const float* gy;   // reverse
  const float* add;  // reverse: added to the result, or NULL
  float* y;          // forward: output; reverse: dL/dx
  float* stats;      // [planes][2]: mean, 1 / sqrt(var + eps)
  int planes, N;
  float eps;
};

__global__ void __launch_bounds__(LNO_T) lno_inorm_fwd_kernel(LnoNormArgs a) {
  __shared__ double red[LNO_T];
  const int tid = threadIdx.x;
  for (int pl = blockIdx.x; pl < a.planes; pl += gridDim.x) {
    const float* x = a.x + (long long)pl * a.N;
    double s = 0.;
    for (int f = tid; f < a.N; f += LNO_T) s += (double)x[f];
    const double mean = lno_block_sum(s, red) / (double)a.N;
    double v = 0.;
    for (int f = tid; f < a.N; f += LNO_T) {
      const double dx = (double)x[f] - mean;
      v += dx * dx;
    }
    const double var = lno_block_sum(v, red) / (double)a.N;  // biased, as InstanceNorm
    const double rstd = 1. / sqrt(var + (double)a.eps);
    float* y = a.y + (long long)pl * a.N;
    for (int f = tid; f < a.N; f += LNO_T) y[f] = (float)(((double)x[f] - mean) * rstd);
    if (tid == 0) a.stats[2 * pl] = (float)mean, a.stats[2 * pl + 1] = (float)rstd;
  }
}

// dL/dx = rstd * (gy - mean(gy) - y * mean(gy * y)) (+ add)
__global__ void __launch_bounds__(LNO_T) lno_inorm_bwd_kernel(LnoNormArgs a) {
  __shared__ double red[LNO_T];
  const int tid = threadIdx.x;
  for (int pl = blockIdx.x; pl < a.planes; pl += gridDim.x) {
    const float* y = a.x + (long long)pl * a.N;
    const float* gy = a.gy + (long long)pl * a.N;
    double s = 0., sy = 0.;
    for (int f = tid; f < a.N; f += LNO_T) {
      s += (double)gy[f];
      sy += (double)gy[f] * (double)y[f];
    }
    const double m1 = lno_block_sum(s, red) / (double)a.N;
    const double m2 = lno_block_sum(sy, red) / (double)a.N;
    const double rstd = (double)a.stats[2 * pl + 1];
    float* gx = a.y + (long long)pl * a.N;
    const float* ad = a.add ? a.add + (long long)pl * a.N : nullptr;
    for (int f = tid; f < a.N; f += LNO_T) {
      const double g = rstd * ((double)gy[f] - m1 - (double)y[f] * m2);
      gx[f] = (float)(ad ? g + (double)ad[f] : g);
    }
  }
}

extern "C" int ppsci_lno_inorm_fwd(int planes, int N, float eps, const float* x, float* y, float* stats, void* stream) {
  if (planes < 1 || N < 1 || !x || !y || !stats) {
    ppsci_set_error("lno_inorm_fwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  LnoNormArgs a{x, nullptr, nullptr, y, stats, planes, N, eps};
  const int grid = planes < 8 * PPSCI_NUM_CU ? planes : 8 * PPSCI_NUM_CU;
  PPSCI_LAUNCH(lno_inorm_fwd_kernel, LnoNormArgs, grid, LNO_T, 0, stream, a);
  return lno_launch_ok("lno_inorm_fwd");
}

extern "C" int ppsci_lno_inorm_bwd(int planes, int N, const float* y, const float* gy, const float* stats, const float* add, float* gx,
                                   void* stream) {
  if (planes < 1 || N < 1 || !y || !gy || !stats || !gx) {
    ppsci_set_error("lno_inorm_bwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  LnoNormArgs a{y, gy, add, gx, const_cast<float*>(stats), planes, N, 0.f};
  const int grid = planes < 8 * PPSCI_NUM_CU ? planes : 8 * PPSCI_NUM_CU;
  PPSCI_LAUNCH(lno_inorm_bwd_kernel, LnoNormArgs, grid, LNO_T, 0, stream, a);
  return lno_launch_ok("lno_inorm_bwd");
}

// ------------------------------------------------------------------------------------------------ per-point layers
// value and derivative of the head's activation (activation.py:139-154 without the ones that carry parameters)
__device__ __forceinline__ void lno_act(int act, float z, float& s, float& d) {
  switch (act) {
    case PPSCI_ACT_TANH: s = tanhf(z), d = 1.f - s * s; break;
    case PPSCI_ACT_SILU: {
      const float g = 1.f / (1.f + expf(-z));
      s = z * g, d = g * (1.f + z * (1.f - g));
    } break;
    case PPSCI_ACT_SIN: s = sinf(z), d = cosf(z); break;
    case PPSCI_ACT_COS: s = cosf(z), d = -sinf(z); break;
    case PPSCI_ACT_SIGMOID: s = 1.f / (1.f + expf(-z)), d = s * (1.f - s); break;
    case PPSCI_ACT_GELU: {
      const float cdf = 0.5f * (1.f + erff(z * 0.70710678118654752f));
      s = z * cdf, d = cdf + z * 0.39894228040143268f * expf(-0.5f * z * z);
    } break;
    case PPSCI_ACT_RELU: s = z > 0.f ? z : 0.f, d = z > 0.f ? 1.f : 0.f; break;
    case PPSCI_ACT_LEAKY_RELU: s = z > 0.f ? z : 0.01f * z, d = z > 0.f ? 1.f : 0.01f; break;
    case PPSCI_ACT_ELU: s = z > 0.f ? z : expf(z) - 1.f, d = z > 0.f ? 1.f : expf(z); break;
    case PPSCI_ACT_SELU: {
      const float al = 1.6732632423543772f, sc = 1.0507009873554805f;
      s = sc * (z > 0.f ? z : al * (expf(z) - 1.f)), d = sc * (z > 0.f ? 1.f : al * expf(z));
    } break;
    default: s = z, d = 1.f; break;
  }
}

static bool lno_act_ok(int act) {
  return act == PPSCI_ACT_TANH || act == PPSCI_ACT_SILU || act == PPSCI_ACT_SIN || act == PPSCI_ACT_COS || act == PPSCI_ACT_SIGMOID ||
         act == PPSCI_ACT_GELU || act == PPSCI_ACT_RELU || act == PPSCI_ACT_LEAKY_RELU || act == PPSCI_ACT_ELU ||
         act == PPSCI_ACT_SELU || act == PPSCI_ACT_IDENTITY;
}

struct LnoLiftArgs {
  const float* x;   // [B][N][fd] channel-last data channels
  const float* W;   // [fin][C], fin = fd + (grid ? 3 : 0)
  const float* bias;
  float* h;         // forward out [B][C][N]
  const float* gh;  // reverse in  [B][C][N]
  float* gx;        // reverse out [B][N][fd] or NULL
  float* partials;  // reverse out [grid][fin * C + C]
  long long P;      // B * N
  int N, n1, n2, n3, fd, fin, C, grid;
};

// input channel f of point (b, s): a data channel or one of the three linspace(0, 1, n_d) coordinates (lno.py:256-270)
__device__ __forceinline__ float lno_lift_in(const LnoLiftArgs& a, long long g, int s, int f) {
  if (f < a.fd) return a.x[g * a.fd + f];
  const int d = f - a.fd;
  const int n23 = a.n2 * a.n3;
  const int i = d == 0 ? s / n23 : (d == 1 ? (s / a.n3) % a.n2 : s % a.n3);
  const int n = d == 0 ? a.n1 : (d == 1 ? a.n2 : a.n3);
  return (float)i / (float)(n - 1);
}

__global__ void __launch_bounds__(LNO_T) lno_lift_fwd_kernel(LnoLiftArgs a) {
  for (long long g = (long long)blockIdx.x * LNO_T + threadIdx.x; g < a.P; g += (long long)gridDim.x * LNO_T) {
    const long long b = g / a.N;
    const int s = (int)(g - b * a.N);
    for (int c = 0; c < a.C; ++c) {
      float v = a.bias[c];
      for (int f = 0; f < a.fin; ++f) v = fmaf(lno_lift_in(a, g, s, f), a.W[f * a.C + c], v);
      a.h[(b * a.C + c) * a.N + s] = v;
    }
  }
}

// tiles of 256 points; x and gh of a tile in LDS, then one thread per (f, c) sums its product over the tile's points in order and
// adds it to the workgroup's row (LDS), written out once at the end
__global__ void __launch_bounds__(LNO_T) lno_lift_bwd_kernel(LnoLiftArgs a) {
  PPSCI_DYN_SMEM(smem);
  float* xs = smem;                       // [fin][256]
  float* gs = xs + a.fin * LNO_TS;        // [C][256]
  double* acc = (double*)(smem + (((a.fin + a.C) * LNO_TS + 1) & ~1));  // [fin * C + C], 8-byte aligned
  const int tid = threadIdx.x;
  const int cols = a.fin * a.C + a.C;
  for (int e = tid; e < cols; e += LNO_T) acc[e] = 0.;
  const long long tiles = (a.P + LNO_T - 1) / LNO_T;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long g = tile * LNO_T + tid;
    const bool live = g < a.P;
    const long long b = live ? g / a.N : 0;
    const int s = live ? (int)(g - b * a.N) : 0;
    __syncthreads();
    for (int f = 0; f < a.fin; ++f) xs[f * LNO_TS + tid] = live ? lno_lift_in(a, g, s, f) : 0.f;
    for (int c = 0; c < a.C; ++c) gs[c * LNO_TS + tid] = live ? a.gh[(b * a.C + c) * a.N + s] : 0.f;
    if (a.gx && live) {
      for (int f = 0; f < a.fd; ++f) {
        float v = 0.f;
        for (int c = 0; c < a.C; ++c) v = fmaf(a.W[f * a.C + c], gs[c * LNO_TS + tid], v);
        a.gx[g * a.fd + f] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < cols; e += LNO_T) {
      double v = 0.;  // (a bias gradient is the small sum of many large terms of both signs behind an instance norm)
      if (e < a.fin * a.C) {
        const int f = e / a.C, c = e - f * a.C;
        for (int p = 0; p < LNO_T; ++p) v += (double)xs[f * LNO_TS + p] * (double)gs[c * LNO_TS + p];
      } else {
        const int c = e - a.fin * a.C;
        for (int p = 0; p < LNO_T; ++p) v += (double)gs[c * LNO_TS + p];
      }
      acc[e] += v;
    }
  }
  __syncthreads();
  for (int e = tid; e < cols; e += LNO_T) a.partials[(long long)blockIdx.x * cols + e] = (float)acc[e];
}

extern "C" int64_t ppsci_lno_point_rows(int64_t points) {
  const int64_t tiles = (points + LNO_T - 1) / LNO_T;
  const int64_t cap = 2 * PPSCI_NUM_CU;
  return tiles < 1 ? 1 : (tiles < cap ? tiles : cap);
}

static int lno_lift_fill(LnoLiftArgs& a, const char* what, int B, int n1, int n2, int n3, int fd, int use_grid, int C) {
  if (B < 1 || n1 < 2 || n2 < 2 || n3 < 2 || fd < 1 || C < 1 || (long long)n1 * n2 * n3 >= (1ll << 24)) {
    ppsci_set_error("%s: invalid argument", what);
    return PPSCI_E_INVALID;
  }
  a = LnoLiftArgs{};
  a.N = n1 * n2 * n3, a.P = (long long)B * a.N, a.n1 = n1, a.n2 = n2, a.n3 = n3, a.fd = fd, a.fin = fd + (use_grid ? 3 : 0), a.C = C,
  a.grid = use_grid ? 1 : 0;
  return PPSCI_OK;
}

extern "C" int ppsci_lno_lift_fwd(int B, int n1, int n2, int n3, int fd, int use_grid, int C, const float* x, const float* W,
                                  const float* bias, float* h, void* stream) {
  LnoLiftArgs a;
  const int rc = lno_lift_fill(a, "lno_lift_fwd", B, n1, n2, n3, fd, use_grid, C);
  if (rc != PPSCI_OK) return rc;
  if (!x || !W || !bias || !h) {
    ppsci_set_error("lno_lift_fwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  a.x = x, a.W = W, a.bias = bias, a.h = h;
  long long grid = (a.P + LNO_T - 1) / LNO_T;
  if (grid > 8192) grid = 8192;
  PPSCI_LAUNCH(lno_lift_fwd_kernel, LnoLiftArgs, (int)grid, LNO_T, 0, stream, a);
  return lno_launch_ok("lno_lift_fwd");
}

extern "C" int ppsci_lno_lift_bwd(int B, int n1, int n2, int n3, int fd, int use_grid, int C, const float* x, const float* W,
                                  const float* gh, float* gx, float* partials, void* stream) {
  LnoLiftArgs a;
  const int rc = lno_lift_fill(a, "lno_lift_bwd", B, n1, n2, n3, fd, use_grid, C);
  if (rc != PPSCI_OK) return rc;
  if (!x || !W || !gh || !partials) {
    ppsci_set_error("lno_lift_bwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  a.x = x, a.W = W, a.gh = gh, a.gx = gx, a.partials = partials;
  const long long lds = ((long long)(a.fin + C) * LNO_TS + 1 + 2ll * (a.fin * C + C)) * 4;
  if (lds > PPSCI_LDS_LIMIT_BYTES - 1024) {
    ppsci_set_error("lno_lift_bwd: %d input and %d output channels do not fit LDS", a.fin, C);
    return PPSCI_E_UNSUPPORTED;
  }
  if (PPSCI_SET_MAX_LDS(lno_lift_bwd_kernel, lds) != 0) {
    ppsci_set_error("lno_lift_bwd: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  PPSCI_LAUNCH(lno_lift_bwd_kernel, LnoLiftArgs, (int)ppsci_lno_point_rows(a.P), LNO_T, (int)lds, stream, a);
  return lno_launch_ok("lno_lift_bwd");
}

// Head: u = x1 + conv(h) (1x1x1 convolution C -> C with bias), y = fc2(act(fc1(u))) per grid point.
#define LNO_HCHUNK 16
struct LnoHeadArgs {
  const float* x1;   // [B][C][N]
  const float* h;    // [B][C][N]
  const float* Wc;   // [C][C] (out, in)
  const float* bc;   // [C]
  const float* W1;   // [C][Hd] (in, out)
  const float* b1;   // [Hd]
  const float* W2;   // [Hd]
  const float* b2;   // [1]
  float* y;          // forward out [B][N]
  const float* gy;   // reverse in  [B][N]
  float* gx1;        // reverse out [B][C][N]: dL/dx1 = dL/du
  float* gh;         // reverse out [B][C][N]: the convolution's share of dL/dh
  float* partials;   // reverse out [grid][C*C + C + C*Hd + Hd + Hd + 1]
  long long P;
  int N, C, Hd, act;
};

__device__ __forceinline__ void lno_head_u(const LnoHeadArgs& a, bool live, long long b, int s, float* us, float* hs) {
  const int tid = threadIdx.x;
  for (int c = 0; c < a.C; ++c) hs[c * LNO_TS + tid] = live ? a.h[(b * a.C + c) * a.N + s] : 0.f;
  for (int c = 0; c < a.C; ++c) {
    float v = live ? a.x1[(b * a.C + c) * a.N + s] + a.bc[c] : 0.f;
    for (int i = 0; i < a.C; ++i) v = fmaf(a.Wc[c * a.C + i], hs[i * LNO_TS + tid], v);
    us[c * LNO_TS + tid] = v;
  }
}

__global__ void __launch_bounds__(LNO_T) lno_head_fwd_kernel(LnoHeadArgs a) {
  PPSCI_DYN_SMEM(smem);
  float* us = smem;
  float* hs = us + a.C * LNO_TS;
  const int tid = threadIdx.x;
  const long long tiles = (a.P + LNO_T - 1) / LNO_T;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long g = tile * LNO_T + tid;
    const bool live = g < a.P;
    const long long b = live ? g / a.N : 0;
    const int s = live ? (int)(g - b * a.N) : 0;
    lno_head_u(a, live, b, s, us, hs);  // (each thread reads only its own column of us / hs: no barrier)
    float y = a.b2[0];
    for (int j = 0; j < a.Hd; ++j) {
      float z = a.b1[j];
      for (int c = 0; c < a.C; ++c) z = fmaf(us[c * LNO_TS + tid], a.W1[c * a.Hd + j], z);
      float sv, dv;
      lno_act(a.act, z, sv, dv);
      y = fmaf(a.W2[j], sv, y);
    }
    if (live) a.y[g] = y;
  }
}

__global__ void __launch_bounds__(LNO_T) lno_head_bwd_kernel(LnoHeadArgs a) {
  PPSCI_DYN_SMEM(smem);
  const int C = a.C, Hd = a.Hd, tid = threadIdx.x;
  float* us = smem;                         // [C][256]  u, later reused for h
  float* gus = us + C * LNO_TS;             // [C][256]  dL/du
  float* dzs = gus + C * LNO_TS;            // [LNO_HCHUNK][256]
  float* azs = dzs + LNO_HCHUNK * LNO_TS;   // [LNO_HCHUNK][256]
  float* gys = azs + LNO_HCHUNK * LNO_TS;   // [256]
  float* acc = gys + LNO_TS;
  const int oWc = 0, obc = C * C, oW1 = obc + C, ob1 = oW1 + C * Hd, oW2 = ob1 + Hd, ob2 = oW2 + Hd, cols = ob2 + 1;
  for (int e = tid; e < cols; e += LNO_T) acc[e] = 0.f;
  const long long tiles = (a.P + LNO_T - 1) / LNO_T;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long g = tile * LNO_T + tid;
    const bool live = g < a.P;
    const long long b = live ? g / a.N : 0;
    const int s = live ? (int)(g - b * a.N) : 0;
    __syncthreads();
    lno_head_u(a, live, b, s, us, gus);  // (gus as scratch for h)
    for (int c = 0; c < C; ++c) gus[c * LNO_TS + tid] = 0.f;
    const float gy = live ? a.gy[g] : 0.f;
    gys[tid] = gy;
    for (int j0 = 0; j0 < Hd; j0 += LNO_HCHUNK) {
      const int nj = Hd - j0 < LNO_HCHUNK ? Hd - j0 : LNO_HCHUNK;
      for (int jj = 0; jj < nj; ++jj) {
        const int j = j0 + jj;
        float z = a.b1[j];
        for (int c = 0; c < C; ++c) z = fmaf(us[c * LNO_TS + tid], a.W1[c * Hd + j], z);
        float sv, dv;
        lno_act(a.act, z, sv, dv);
        const float dz = a.W2[j] * gy * dv;
        dzs[jj * LNO_TS + tid] = dz;
        azs[jj * LNO_TS + tid] = sv * gy;
        for (int c = 0; c < C; ++c) gus[c * LNO_TS + tid] = fmaf(a.W1[c * Hd + j], dz, gus[c * LNO_TS + tid]);
      }
      __syncthreads();
      for (int e = tid; e < nj * (C + 2); e += LNO_T) {
        const int jj = e / (C + 2), v = e - jj * (C + 2), j = j0 + jj;
        float sum = 0.f;
        if (v < C) {
          for (int p = 0; p < LNO_T; ++p) sum = fmaf(dzs[jj * LNO_TS + p], us[v * LNO_TS + p], sum);
          acc[oW1 + v * Hd + j] += sum;
        } else if (v == C) {
          for (int p = 0; p < LNO_T; ++p) sum += dzs[jj * LNO_TS + p];
          acc[ob1 + j] += sum;
        } else {
          for (int p = 0; p < LNO_T; ++p) sum += azs[jj * LNO_TS + p];
          acc[oW2 + j] += sum;
        }
      }
      __syncthreads();
    }
    // u = x1 + Wc h + bc: dL/dx1 = dL/du, dL/dh = Wc^T dL/du; us now holds h for the convolution's weight gradient
    for (int c = 0; c < C; ++c) us[c * LNO_TS + tid] = live ? a.h[(b * C + c) * a.N + s] : 0.f;
    if (live) {
      for (int c = 0; c < C; ++c) a.gx1[(b * C + c) * a.N + s] = gus[c * LNO_TS + tid];
      for (int i = 0; i < C; ++i) {
        float v = 0.f;
        for (int o = 0; o < C; ++o) v = fmaf(a.Wc[o * C + i], gus[o * LNO_TS + tid], v);
        a.gh[(b * C + i) * a.N + s] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < C * C + C + 1; e += LNO_T) {
      float sum = 0.f;
      if (e < C * C) {
        const int o = e / C, i = e - o * C;
        for (int p = 0; p < LNO_T; ++p) sum = fmaf(gus[o * LNO_TS + p], us[i * LNO_TS + p], sum);
        acc[oWc + e] += sum;
      } else if (e < C * C + C) {
        const int o = e - C * C;
        for (int p = 0; p < LNO_T; ++p) sum += gus[o * LNO_TS + p];
        acc[obc + o] += sum;
      } else {
        for (int p = 0; p < LNO_T; ++p) sum += gys[p];
        acc[ob2] += sum;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < cols; e += LNO_T) a.partials[(long long)blockIdx.x * cols + e] = acc[e];
}

static int lno_head_fill(LnoHeadArgs& a, const char* what, int B, int N, int C, int Hd, int act) {
  if (B < 1 || N < 1 || C < 1 || Hd < 1) {
    ppsci_set_error("%s: invalid argument", what);
    return PPSCI_E_INVALID;
  }
  if (!lno_act_ok(act)) {
    ppsci_set_error("%s: activation %d has no LNO head kernel (it carries trainable parameters)", what, act);
    return PPSCI_E_UNSUPPORTED;
  }
  a = LnoHeadArgs{};
  a.P = (long long)B * N, a.N = N, a.C = C, a.Hd = Hd, a.act = act;
  return PPSCI_OK;
}

static long long lno_head_bwd_lds(int C, int Hd) {
  return ((long long)(2 * C + 2 * LNO_HCHUNK + 1) * LNO_TS + C * C + C + (long long)C * Hd + 2 * Hd + 1) * 4;
}

extern "C" int ppsci_lno_head_supported(int C, int Hd) {
  return (C >= 1 && Hd >= 1 && lno_head_bwd_lds(C, Hd) <= PPSCI_LDS_LIMIT_BYTES - 1024) ? 1 : 0;
}

extern "C" int ppsci_lno_head_fwd(int B, int N, int C, int Hd, int act, const float* x1, const float* h, const float* Wc,
                                  const float* bc, const float* W1, const float* b1, const float* W2, const float* b2, float* y,
                                  void* stream) {
  LnoHeadArgs a;
  const int rc = lno_head_fill(a, "lno_head_fwd", B, N, C, Hd, act);
  if (rc != PPSCI_OK) return rc;
  if (!x1 || !h || !Wc || !bc || !W1 || !b1 || !W2 || !b2 || !y || !ppsci_lno_head_supported(C, Hd)) {
    ppsci_set_error("lno_head_fwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  a.x1 = x1, a.h = h, a.Wc = Wc, a.bc = bc, a.W1 = W1, a.b1 = b1, a.W2 = W2, a.b2 = b2, a.y = y;
  const long long lds = (long long)2 * C * LNO_TS * 4;
  if (PPSCI_SET_MAX_LDS(lno_head_fwd_kernel, lds) != 0) {
    ppsci_set_error("lno_head_fwd: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  long long grid = (a.P + LNO_T - 1) / LNO_T;
  if (grid > 8192) grid = 8192;
  PPSCI_LAUNCH(lno_head_fwd_kernel, LnoHeadArgs, (int)grid, LNO_T, (int)lds, stream, a);
  return lno_launch_ok("lno_head_fwd");
}

extern "C" int ppsci_lno_head_bwd(int B, int N, int C, int Hd, int act, const float* x1, const float* h, const float* Wc,
                                  const float* bc, const float* W1, const float* b1, const float* W2, const float* gy, float* gx1,
                                  float* gh, float* partials, void* stream) {
  LnoHeadArgs a;
  const int rc = lno_head_fill(a, "lno_head_bwd", B, N, C, Hd, act);
  if (rc != PPSCI_OK) return rc;
  if (!x1 || !h || !Wc || !bc || !W1 || !b1 || !W2 || !gy || !gx1 || !gh || !partials) {
    ppsci_set_error("lno_head_bwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  if (!ppsci_lno_head_supported(C, Hd)) {
    ppsci_set_error("lno_head_bwd: width %d with %d hidden features does not fit LDS", C, Hd);
    return PPSCI_E_UNSUPPORTED;
  }
  a.x1 = x1, a.h = h, a.Wc = Wc, a.bc = bc, a.W1 = W1, a.b1 = b1, a.W2 = W2, a.gy = gy, a.gx1 = gx1, a.gh = gh, a.partials = partials;
  const long long lds = lno_head_bwd_lds(C, Hd);
  if (PPSCI_SET_MAX_LDS(lno_head_bwd_kernel, lds) != 0) {
    ppsci_set_error("lno_head_bwd: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  PPSCI_LAUNCH(lno_head_bwd_kernel, LnoHeadArgs, (int)ppsci_lno_point_rows(a.P), LNO_T, (int)lds, stream, a);
  return lno_launch_ok("lno_head_bwd");
}
