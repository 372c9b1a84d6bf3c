// spinn_jet.inc -- the general tensor-product contraction of a separable PINN (included by spinn.hip).
//
// Replaces, for a residual that is NOT a linear form of {u, u_xx, u_yy, u_zz},
//   SPINN.forward_tensor           /root/reference/ppsci/arch/spinn.py:140-167
//   hvp_revrev / nested jvp        /root/reference/ppsci/equation/pde/helmholtz.py:27-41
// which the reference runs once per derivative on the full grid, each pass materialising [N,N,N,r].
//
// On a separable net  d^(a+b+c) u / dx^a dy^b dz^c (i,j,k) = sum_r fx^(a)[i,r] fy^(b)[j,r] fz^(c)[k,r]:  every derivative
// with per-axis order <= 2 is a contraction of the value / first / second streams F[3][n][R] the branch nets already carry.
// A constraint names the nq <= PPSCI_SPINN_MAX_JET order triples its program reads ("streams"); the forward kernel writes them
// as the rows U[nq][nx*ny*nz] that ppsci_epilogue reads, the reverse kernel contracts the adjoint rows Ubar[nq][..] back into
// Fbar[3][n][R] of the three axes.  The residual arithmetic itself is the epilogue VM's.
//
// Both kernels keep the shape of the MFMA kernels of the linear path above (v_mfma_f32_16x16x4_f32, same lane <-> index maps);
// what differs is that a stream's operands are picked by its order triple instead of being folded with four coefficients.
// Any rank 1 .. 64 runs: a rank that is no multiple of 4 is zero-padded while the operands are loaded / staged.

struct JetArgs {
  ppsci_spinn_jet_desc d;
  const float* F[3];  // per axis [3][n_a][R]
  float* U;           // fwd out: [nq][nx*ny*nz]
  const float* Ubar;  // bwd in : [nq][nx*ny*nz]
  float* Fpart;       // bwd scratch: per axis [n_a][groups][3][R]
  float* Fbar3[3];    // bwd out: per axis [3][n_a][R]
  long long poff3[3];
  int ngrp3[3];
  int wg3[3];
  int RP;             // padded LDS row stride of the staged factor tables
};

// four consecutive rank entries r4 .. r4 + 3 of one factor row (zero beyond the rank; one 16-byte load when rows are aligned)
__device__ __forceinline__ f32x4 jet_ld4(const float* row, int r4, int R, bool ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!ok) return v;
  if ((R & 3) == 0) {
    if (r4 < R) v = *(const f32x4*)&row[r4];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (r4 + e < R) v[e] = row[r4 + e];
  }
  return v;
}

#define JET_CHUNK 4  // streams whose A operands and accumulators a wave holds at a time

// Forward: one wave = (i, 16 rows j, every GRID_CS-th 16-column tile of k).  Per chunk of JET_CHUNK streams the A operand
// fx^(a)[i,r] fy^(b)[j,r] is computed once into registers; per tile of k the B fragments fz^(c)[k,r] are loaded once per order
// c the chunk uses and shared by its streams; one accumulator tile per stream.  Consecutive lanes = consecutive k: 64 B stores.
template <int NS>
__global__ void __launch_bounds__(GRID_BLOCK) spinn_jet_fwd_kernel(JetArgs a) {
  const int R = a.d.rank, nx = a.d.n[0], ny = a.d.n[1], nz = a.d.n[2], nq = a.d.nq;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int njb = (ny + 15) / 16;
  const int wid = blockIdx.x * (GRID_BLOCK / 64) + wave;
  if (wid >= nx * njb * GRID_CS) return;
  const int cs = wid % GRID_CS, ij = wid / GRID_CS;
  const int i = ij / njb, j0 = (ij % njb) * 16;
  const long long total = (long long)nx * ny * nz;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < nq; q0 += JET_CHUNK) {
    f32x4 A[JET_CHUNK][NS];
    bool need0 = false, need1 = false, need2 = false;  // orders of fz the chunk reads
    {
      const int j = j0 + c;
#pragma unroll
      for (int s = 0; s < JET_CHUNK; ++s) {
        const int q = q0 + s;
        const bool live = q < nq;
        const int oa = live ? a.d.ord[q][0] : 0, ob = live ? a.d.ord[q][1] : 0;
        const int oz = live ? a.d.ord[q][2] : -1;
        need0 |= oz == 0; need1 |= oz == 1; need2 |= oz == 2;
        const float* rx = a.F[0] + ((long long)oa * nx + i) * R;
        const float* ry = a.F[1] + ((long long)ob * ny + (j < ny ? j : 0)) * R;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          const int r4 = 16 * t + 4 * g;
          A[s][t] = jet_ld4(rx, r4, R, live && j < ny) * jet_ld4(ry, r4, R, live && j < ny);
        }
      }
    }
    for (int k0 = 16 * cs; k0 < nz; k0 += 16 * GRID_CS) {
      const int k = k0 + c;
      f32x4 B[3][NS];
#pragma unroll
      for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int t = 0; t < NS; ++t)
          B[o][t] = (o == 0 ? need0 : o == 1 ? need1 : need2) ? jet_ld4(a.F[2] + ((long long)o * nz + (k < nz ? k : 0)) * R, 16 * t + 4 * g, R, k < nz) : zero4;
#pragma unroll
      for (int s = 0; s < JET_CHUNK; ++s) {
        const int q = q0 + s;
        if (q >= nq) break;
        const int oc = a.d.ord[q][2];  // wave-uniform: three copies of the chain instead of a register array indexed at run time
        f32x4 acc = zero4;
        if (oc == 0) {
#pragma unroll
          for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[s][t][e], B[0][t][e], acc, 0, 0, 0);
        } else if (oc == 1) {
#pragma unroll
          for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[s][t][e], B[1][t][e], acc, 0, 0, 0);
        } else {
#pragma unroll
          for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[s][t][e], B[2][t][e], acc, 0, 0, 0);
        }
        float* Uq = a.U + (long long)q * total;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int j = j0 + 4 * g + rr;
          if (j < ny && k < nz) Uq[((long long)i * ny + j) * nz + k] = acc[rr];
        }
      }
    }
  }
}

// T[i, r] = sum_kc g(i, kc) * f[kc, r] for one stream and one row jb: 16 rows i (lane column cl holds row i0 + cl of the A
// operand), NT rank tiles.  VEC: kc is the contiguous axis and rows are 16-byte aligned -- one float4 load per 16-wide slab and
// lane; otherwise four strided loads (ax = 2: consecutive lanes are consecutive i, 64 B runs).  The loads of a whole 128-wide
// slab group are issued together, ahead of the MFMA chain.
template <int NT, bool VEC>
__device__ __forceinline__ void jet_bwd_gemm(const float* gp, long long sc, bool rowok, int nc, int ncp, int g, int cl,
                                             const float* fq, int RP, f32x4 t[NT]) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) t[nt] = zero4;
#pragma unroll 1
  for (int k0 = 0; k0 < ncp; k0 += 16 * GRID_QSLAB) {
    f32x4 av[GRID_QSLAB];
#pragma unroll
    for (int s = 0; s < GRID_QSLAB; ++s) {
      const int kc = k0 + 16 * s + 4 * g;
      if (VEC) {
        av[s] = (rowok && kc < nc) ? *(const f32x4*)&gp[kc] : zero4;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) av[s][e] = (rowok && kc + e < nc) ? gp[(long long)(kc + e) * sc] : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < GRID_QSLAB; ++s) {
      if (k0 + 16 * s < ncp) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kr = k0 + 16 * s + 4 * g + e;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            t[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][e], fq[kr * RP + 16 * nt + cl], t[nt], 0, 0, 0);
        }
      }
    }
  }
}

// Reverse, all three axes in one launch: for axis `ax` with the others (b, c), c the faster-varying,
//     Fbar_ax[d][i,r] = sum_{q: ord_q[ax] = d} sum_jb F_b[ord_q[b]][jb,r] * ( sum_kc Ubar_q[i,jb,kc] * F_c[ord_q[c]][kc,r] ).
// One wave = (16 consecutive indices i on `ax`, one index jb); one workgroup = 4 such jb of the same i block.  Per stream the
// inner sum is a GEMM (M = 16 i, N = R, K = n_c) against the factor table of order ord_q[c], all three orders staged once per
// workgroup in LDS (row stride = 4 mod 32 floats); the outer factor is applied elementwise in the D layout into one of three
// accumulators.  The 4 waves' sums are added through LDS in wave order, the workgroup partials [n_a][groups][3][R] are summed by
// spinn_jet_fbar_sum_kernel in a fixed order: no atomics, two passes give the same bits.
template <int NT>
__global__ void __launch_bounds__(GRID_BLOCK) spinn_jet_bwd_kernel(JetArgs a) {
  PPSCI_DYN_SMEM(sm);
  int bx = blockIdx.x, ax = 0;
  while (ax < 2 && bx >= a.wg3[ax]) { bx -= a.wg3[ax]; ++ax; }
  const int ngrp = a.ngrp3[ax];
  float* Fpart = a.Fpart + a.poff3[ax];
  const int R = a.d.rank, nq = a.d.nq;
  const int b = ax == 0 ? 1 : 0, c = ax == 2 ? 1 : 2;
  const int na = a.d.n[ax], nb = a.d.n[b], nc = a.d.n[c];
  const int RP = a.RP;
  const int ncp = (nc + 15) & ~15;
  long long stride[3];
  stride[2] = 1; stride[1] = a.d.n[2]; stride[0] = (long long)a.d.n[1] * a.d.n[2];
  const long long total = stride[0] * a.d.n[0];
  const bool vec = stride[c] == 1 && (a.d.n[2] & 3) == 0;
  float* fc = sm;  // [3][ncp][RP]; reused as the exchange [4 waves][3][NT][4][64] once the GEMMs are done
#pragma unroll 4
  for (int t = threadIdx.x; t < 3 * ncp * RP; t += GRID_BLOCK) {
    const int o = t / (ncp * RP), rem = t - o * ncp * RP, kc = rem / RP, r = rem - kc * RP;
    fc[t] = (kc < nc && r < R) ? a.F[c][((long long)o * nc + kc) * R + r] : 0.f;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, cl = lane & 15;
  const int i0 = (bx / ngrp) * 16, grp = bx % ngrp;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[3][NT];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) v[d][nt] = zero4;
  const int irow = i0 + cl;
  const int jb = grp * (GRID_BLOCK / 64) + wave;
  if (jb < nb) {
#pragma unroll 1
    for (int q = 0; q < nq; ++q) {
      const int oa = a.d.ord[q][ax], ob = a.d.ord[q][b], oc = a.d.ord[q][c];
      const float* fq = fc + oc * ncp * RP;
      const float* gp = a.Ubar + (long long)q * total + (long long)(irow < na ? irow : 0) * stride[ax] + (long long)jb * stride[b];
      f32x4 t[NT];
      // (the lane group is hidden from the optimiser per stream: the 32 LDS addresses of a slab group are otherwise hoisted out
      // of this loop into registers of their own -- 256 VGPRs, one wave per SIMD -- instead of being recomputed)
      int gq = g;
      PPSCI_OPAQUE(gq);
      if (vec) jet_bwd_gemm<NT, true>(gp, 1, irow < na, nc, ncp, gq, cl, fq, RP, t);
      else jet_bwd_gemm<NT, false>(gp, stride[c], irow < na, nc, ncp, gq, cl, fq, RP, t);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int r = 16 * nt + cl;
        const float y = r < R ? a.F[b][((long long)ob * nb + jb) * R + r] : 0.f;
        if (oa == 0) v[0][nt] += y * t[nt];
        else if (oa == 1) v[1][nt] += y * t[nt];
        else v[2][nt] += y * t[nt];
      }
    }
  }
  __syncthreads();  // every wave is done with the factor tables: their LDS becomes the exchange
  float* ex = sm;
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) ex[(((wave * 3 + d) * NT + nt) * 4 + rr) * 64 + lane] = v[d][nt][rr];
  __syncthreads();
#pragma unroll 1
  for (int e = threadIdx.x; e < 3 * NT * 4 * 64; e += GRID_BLOCK) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < GRID_BLOCK / 64; ++w) sum += ex[w * 3 * NT * 4 * 64 + e];
    const int l = e & 63, qq = e >> 6, rr = qq & 3, nt = (qq >> 2) % NT, d = qq / (4 * NT);
    const int i = i0 + 4 * (l >> 4) + rr, r = 16 * nt + (l & 15);
    if (i < na && r < R) Fpart[(((long long)i * ngrp + grp) * 3 + d) * R + r] = sum;
  }
}

// One workgroup per index i of one axis: thread = (column of the [3][R] partial row, one of FSUM_PARTS interleaved group subsets),
// the subsets combined through LDS in a fixed order.
__global__ void __launch_bounds__(GRID_BLOCK) spinn_jet_fbar_sum_kernel(JetArgs a) {
  PPSCI_DYN_SMEM(red);  // [FSUM_PARTS][3R]
  int bx = blockIdx.x, ax = 0;
  while (ax < 2 && bx >= a.wg3[ax]) { bx -= a.wg3[ax]; ++ax; }
  const int ngrp = a.ngrp3[ax], R = a.d.rank, na = a.d.n[ax], i = bx, C3 = 3 * R;
  const float* Fpart = a.Fpart + a.poff3[ax];
  for (int e = threadIdx.x; e < C3 * FSUM_PARTS; e += GRID_BLOCK) {
    const int part = e / C3, col = e % C3;
    const float* p = Fpart + (long long)i * ngrp * C3 + col;
    float s = 0.f;
#pragma unroll 4
    for (int gi = part; gi < ngrp; gi += FSUM_PARTS) s += p[(long long)gi * C3];
    red[e] = s;
  }
  __syncthreads();
  for (int col = threadIdx.x; col < C3; col += GRID_BLOCK) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < FSUM_PARTS; ++q) s += red[q * C3 + col];
    const int d = col / R, r = col - d * R;
    a.Fbar3[ax][((long long)d * na + i) * R + r] = s;
  }
}

// ------------------------------------------------------------------------------------ C ABI
#define JET_MAX_RANK 64  // four 16-wide rank tiles per wave, as the MFMA kernels of the linear path

static int jet_check(const char* who, const ppsci_spinn_jet_desc* d) {
  if (!d) {
    ppsci_set_error("%s: null descriptor", who);
    return PPSCI_E_INVALID;
  }
  if (d->n[0] < 1 || d->n[1] < 1 || d->n[2] < 1) {
    ppsci_set_error("%s: grid %d x %d x %d: every axis needs at least one point", who, d->n[0], d->n[1], d->n[2]);
    return PPSCI_E_INVALID;
  }
  if (d->rank < 1 || d->rank > JET_MAX_RANK) {
    ppsci_set_error("%s: rank %d outside 1 .. %d", who, d->rank, JET_MAX_RANK);
    return PPSCI_E_INVALID;
  }
  if (d->nq < 1 || d->nq > PPSCI_SPINN_MAX_JET) {
    ppsci_set_error("%s: %d streams outside 1 .. %d", who, d->nq, PPSCI_SPINN_MAX_JET);
    return PPSCI_E_INVALID;
  }
  for (int q = 0; q < d->nq; ++q)
    for (int ax = 0; ax < 3; ++ax)
      if (d->ord[q][ax] < 0 || d->ord[q][ax] > 2) {
        ppsci_set_error("%s: stream %d has order %d along axis %d (the branch nets carry orders 0 .. 2)", who, q, d->ord[q][ax], ax);
        return PPSCI_E_INVALID;
      }
  return PPSCI_OK;
}

static int jet_bwd_groups(const ppsci_spinn_jet_desc* d, int ax) {
  const int b = ax == 0 ? 1 : 0;
  return (d->n[b] + GRID_BLOCK / 64 - 1) / (GRID_BLOCK / 64);
}

extern "C" int ppsci_spinn_jet_fwd(const ppsci_spinn_jet_desc* d, const float* Fx, const float* Fy, const float* Fz, float* U,
                                   void* stream) {
  if (jet_check("spinn_jet_fwd", d) != PPSCI_OK) return PPSCI_E_INVALID;
  if (!Fx || !Fy || !Fz || !U) {
    ppsci_set_error("spinn_jet_fwd: null pointer");
    return PPSCI_E_INVALID;
  }
  JetArgs a;
  memset(&a, 0, sizeof(a));
  a.d = *d;
  a.F[0] = Fx; a.F[1] = Fy; a.F[2] = Fz;
  a.U = U;
  const long long waves = (long long)d->n[0] * ((d->n[1] + 15) / 16) * GRID_CS;
  const long long wg = (waves + GRID_BLOCK / 64 - 1) / (GRID_BLOCK / 64);
  if (waves > 0x7fffffffLL) {
    ppsci_set_error("spinn_jet_fwd: grid too large");
    return PPSCI_E_UNSUPPORTED;
  }
  if (d->rank <= 16) PPSCI_LAUNCH(spinn_jet_fwd_kernel<1>, JetArgs, (int)wg, GRID_BLOCK, 0, stream, a);
  else if (d->rank <= 32) PPSCI_LAUNCH(spinn_jet_fwd_kernel<2>, JetArgs, (int)wg, GRID_BLOCK, 0, stream, a);
  else PPSCI_LAUNCH(spinn_jet_fwd_kernel<4>, JetArgs, (int)wg, GRID_BLOCK, 0, stream, a);
  int e = PPSCI_LAST_LAUNCH_ERROR();
  if (e != 0) { ppsci_set_error("spinn_jet_fwd: launch failed (%d)", e); return PPSCI_E_LAUNCH; }
  return PPSCI_OK;
}

extern "C" int64_t ppsci_spinn_jet_scratch_floats(const ppsci_spinn_jet_desc* d) {
  if (jet_check("spinn_jet_scratch_floats", d) != PPSCI_OK) return 0;
  long long m = 0;
  for (int ax = 0; ax < 3; ++ax) m += (long long)d->n[ax] * jet_bwd_groups(d, ax) * 3 * d->rank;
  return m;
}

extern "C" int ppsci_spinn_jet_bwd(const ppsci_spinn_jet_desc* d, const float* Fx, const float* Fy, const float* Fz,
                                   const float* Ubar, float* scratch, float* Fbar_x, float* Fbar_y, float* Fbar_z, void* stream) {
  if (jet_check("spinn_jet_bwd", d) != PPSCI_OK) return PPSCI_E_INVALID;
  if (!Fx || !Fy || !Fz || !Ubar || !scratch || !Fbar_x || !Fbar_y || !Fbar_z) {
    ppsci_set_error("spinn_jet_bwd: null pointer");
    return PPSCI_E_INVALID;
  }
  JetArgs a;
  memset(&a, 0, sizeof(a));
  a.d = *d;
  a.F[0] = Fx; a.F[1] = Fy; a.F[2] = Fz;
  a.Ubar = Ubar;
  a.Fpart = scratch;
  a.Fbar3[0] = Fbar_x; a.Fbar3[1] = Fbar_y; a.Fbar3[2] = Fbar_z;
  const int rp = ((d->rank + 15) / 16) * 16;
  a.RP = (rp % 32 == 0) ? rp + 4 : rp + 20;  // row stride = 4 mod 32
  const int nt = d->rank <= 16 ? 1 : d->rank <= 32 ? 2 : 4;
  long long wg = 0, off = 0;
  int nsum = 0, ncmax = 0;
  for (int ax = 0; ax < 3; ++ax) {
    const int c = ax == 2 ? 1 : 2;
    a.ngrp3[ax] = jet_bwd_groups(d, ax);
    const long long w = (long long)((d->n[ax] + 15) / 16) * a.ngrp3[ax];
    if (w > 0x3fffffffLL) {
      ppsci_set_error("spinn_jet_bwd: grid too large");
      return PPSCI_E_UNSUPPORTED;
    }
    a.wg3[ax] = (int)w;
    a.poff3[ax] = off;
    off += (long long)d->n[ax] * a.ngrp3[ax] * 3 * d->rank;
    wg += w;
    nsum += d->n[ax];
    if (d->n[c] > ncmax) ncmax = d->n[c];
  }
  if (wg > 0x7fffffffLL) {
    ppsci_set_error("spinn_jet_bwd: grid too large");
    return PPSCI_E_UNSUPPORTED;
  }
  const long long ncp = (ncmax + 15) & ~15;
  const long long tab = 3 * ncp * a.RP, exch = (long long)(GRID_BLOCK / 64) * 3 * nt * 4 * 64;
  const size_t lds = (size_t)(tab > exch ? tab : exch) * sizeof(float);
  if (lds > (size_t)PPSCI_LDS_LIMIT_BYTES) {
    ppsci_set_error("spinn_jet_bwd: axis of %d points x rank %d does not fit LDS", ncmax, d->rank);
    return PPSCI_E_UNSUPPORTED;
  }
  int se;
  if (nt == 1) {
    se = PPSCI_SET_MAX_LDS(spinn_jet_bwd_kernel<1>, lds);
    if (se == 0) PPSCI_LAUNCH(spinn_jet_bwd_kernel<1>, JetArgs, (int)wg, GRID_BLOCK, lds, stream, a);
  } else if (nt == 2) {
    se = PPSCI_SET_MAX_LDS(spinn_jet_bwd_kernel<2>, lds);
    if (se == 0) PPSCI_LAUNCH(spinn_jet_bwd_kernel<2>, JetArgs, (int)wg, GRID_BLOCK, lds, stream, a);
  } else {
    se = PPSCI_SET_MAX_LDS(spinn_jet_bwd_kernel<4>, lds);
    if (se == 0) PPSCI_LAUNCH(spinn_jet_bwd_kernel<4>, JetArgs, (int)wg, GRID_BLOCK, lds, stream, a);
  }
  if (se != 0) {
    ppsci_set_error("spinn_jet_bwd: cannot raise dynamic LDS to %zu B", lds);
    return PPSCI_E_LAUNCH;
  }
  int e = PPSCI_LAST_LAUNCH_ERROR();
  if (e != 0) { ppsci_set_error("spinn_jet_bwd: launch failed (%d)", e); return PPSCI_E_LAUNCH; }
  a.wg3[0] = d->n[0]; a.wg3[1] = d->n[1]; a.wg3[2] = d->n[2];
  PPSCI_LAUNCH(spinn_jet_fbar_sum_kernel, JetArgs, nsum, GRID_BLOCK, (size_t)FSUM_PARTS * 3 * d->rank * sizeof(float), stream, a);
  e = PPSCI_LAST_LAUNCH_ERROR();
  if (e != 0) { ppsci_set_error("spinn_jet_fbar_sum: launch failed (%d)", e); return PPSCI_E_LAUNCH; }
  return PPSCI_OK;
}
