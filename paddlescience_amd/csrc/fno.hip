// fno.hip -- the non-spectral part of an FNO block and of the lifting / projection channel MLPs, forward AND
// hand-written backward, so that a TFNO training step runs no library GEMM / normalisation / activation kernels and
// no autograd graph:
//
//   fno_block.MLP (1x1 convolutions)           /root/reference/ppsci/arch/fno_block.py:263-320
//   FNOBlocks skip connection (linear, 1x1)    /root/reference/ppsci/arch/fno_block.py:190-226
//   forward_with_postactivation                /root/reference/ppsci/arch/fno_block.py:1191-1220
//                                              x <- act( norm(SpectralConv(x)) + skip(x) ), GroupNorm(1 group)
//
// Data layout: NCHW as the reference ([B, C, P] with P = H*W contiguous).
//
// * ppsci_pw_conv:   out[b,o,p] = sum_i W[o,i] x[b,i,p] (+ bias[o]) -- one 1x1 convolution = one GEMM per sample,
//   [Co x Ci] . [Ci x P], on v_mfma_f32_16x16x4_f32.  A wave owns 64 consecutive pixels: its B operands are float4
//   loads (lane (g,c) reads pixels 4c..4c+3 of channel row k+g: 256 contiguous bytes per row), one float4 = the
//   same k-step of four 16-pixel MFMA column tiles; the A operands (weights) sit in LDS in fragment order.  The
//   epilogue adds the bias and optionally applies GELU (writing both the pre-activation and the activation), or
//   multiplies with GELU'(z) of the producing layer (data gradient of the previous activation), or accumulates.
//   With `transpose` the same kernel computes the data gradient gx[b,i,p] = sum_o W[o,i] gy[b,o,p].
// * ppsci_pw_conv_wgrad: gW[o,i] = sum_{b,p} gy[b,o,p] x[b,i,p], gb[o] = sum gy -- contraction over pixels: both
//   operands are float4 loads along pixels; per-chunk partial blocks, summed in a fixed order by ppsci_reduce_rows.
// * ppsci_gn_*: GroupNorm with one group (per-sample statistics over C*P) fused with the spectral bias, the affine
//   map, the skip addition and GELU; backward with per-row sums, a tiny fixed-order finalisation and one apply pass.
// All reductions have a fixed order (no float atomics): bit-reproducible.
#include "taylor_tile.h"  // ppsci_split / PPSCI_XDL: fp32 GEMMs on the bf16 (XDL) matrix pipe
#include "dft_kept.h"     // the apply kernels of the block tail can transform the plane they have just produced

#ifndef PPSCI_EMU
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>
#include <string.h>

extern "C" void ppsci_set_error(const char* fmt, ...);

// GELU(t) = t Phi(t) (the erf form the reference's F.gelu uses) and its derivative Phi(t) + t phi(t).
// Phi(t) = (1 + erf(t / sqrt 2)) / 2 with erf by Abramowitz & Stegun 7.1.26:
//   erf(x) = 1 - (a1 u + ... + a5 u^5) exp(-x^2),  u = 1 / (1 + p x),  x >= 0,   |error| <= 1.5e-7,
// i.e. v_rcp + five v_fma + ONE v_exp -- and exp(-x^2) = exp(-t^2 / 2) is the Gaussian of phi(t) as well, so the
// derivative costs no second exponential.  ocml's erff is ~45 VALU instructions with branches (plus expf for phi):
// with it the kernels that evaluate GELU per loaded element (the projection's and lifting's hidden tensors are functions
// of stored ones, ppsci_pw_virtual) were VALU-bound (measured: lifting forward 74 us, its data gradient 77 us).  The
// absolute error is below fp32 rounding of 1 + erf; relative to the reference's fp64-checked outputs the FNO parity
// tests see no change at their 1e-5 / 2e-4 thresholds.
__device__ __forceinline__ void fno_gelu_parts(float t, float& cdf, float& gauss) {
  const float x = fabsf(t) * 0.7071067811865476f;
  gauss = __expf(-x * x);
  const float u = __builtin_amdgcn_rcpf(1.f + 0.3275911f * x);
  const float poly = u * (0.254829592f + u * (-0.284496736f + u * (1.421413741f + u * (-1.453152027f + u * 1.061405429f))));
  const float h = 0.5f * poly * gauss;  // (1 - erf(|x|)) / 2
  cdf = t >= 0.f ? 1.f - h : h;
}
__device__ __forceinline__ float fno_gelu(float t) {
  float cdf, gs;
  fno_gelu_parts(t, cdf, gs);
  return t * cdf;
}
__device__ __forceinline__ float fno_gelu_grad(float t) {
  float cdf, gs;
  fno_gelu_parts(t, cdf, gs);
  return cdf + t * 0.3989422804014327f * gs;
}

// Four neighbouring pixels p .. p + 3 of one [.., P] row, zero beyond `lim`.  al (P a multiple of 4, 16-byte aligned
// buffers: every FNO resolution that is not an odd DomainPadding size): one 16-byte access, all four or none; otherwise
// element by element (rows of such planes do not start on 16-byte boundaries).
__device__ __forceinline__ f32x4 fno_ld4(const float* row, long long p, long long lim, bool al) {
  f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (al) {
    if (p + 3 < lim) v = *(const f32x4*)&row[p];
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (p + t < lim) v[t] = row[p + t];
  }
  return v;
}
__device__ __forceinline__ void fno_st4(float* row, long long p, long long lim, bool al, f32x4 v) {
  if (al) {
    if (p + 3 < lim) *(f32x4*)&row[p] = v;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (p + t < lim) row[p + t] = v[t];
  }
}

// N = 1, 2 or 4 neighbouring pixels (components N.. of the result are zero); al: P a multiple of N
template <int N>
__device__ __forceinline__ f32x4 fno_ldn(const float* row, long long p, long long lim, bool al) {
  if constexpr (N == 4) return fno_ld4(row, p, lim, al);
  f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (N == 2 && al) {
    if (p + 1 < lim) {
      const f32x2 w = *(const f32x2*)&row[p];
      v[0] = w[0], v[1] = w[1];
    }
  } else {
#pragma unroll
    for (int t = 0; t < N; ++t)
      if (p + t < lim) v[t] = row[p + t];
  }
  return v;
}
template <int N>
__device__ __forceinline__ void fno_stn(float* row, long long p, long long lim, bool al, f32x4 v) {
  if constexpr (N == 4) {
    fno_st4(row, p, lim, al, v);
  } else if (N == 2 && al) {
    if (p + 1 < lim) *(f32x2*)&row[p] = (f32x2){v[0], v[1]};
  } else {
#pragma unroll
    for (int t = 0; t < N; ++t)
      if (p + t < lim) row[p + t] = v[t];
  }
}

// ------------------------------------------------------------------------------------------ 1x1 convolution
struct PwArgs {
  const float* x;      // [B, Cin, P]
  const float* W;      // [Co, Ci] row-major (torch Conv2d weight [Co, Ci, 1, 1]); transpose: used as [Ci x Co]
  const float* bias;   // [Cout] or null
  const float* zmul;   // [B, Cout, P] or null: out *= GELU'(zmul)
  float* out;          // [B, Cout, P]: pre-activation (or the plain result)
  float* act;          // [B, Cout, P] or null: GELU(out)
  int B, Cin, Cout, P, ldw, transpose, accumulate;
  int kq;              // ceil(Cin / 16)
  int nob;             // ceil(Cout / 16)
  int vec;             // 16-byte staging path (dimensions and pointers aligned)
  int co0, CoutT;      // this workgroup computes output channels [co0, co0 + Cout) of CoutT (weights that do not fit LDS
                       // at once are processed in slabs of output channels)
  int nslab, slab_rows;  // > 1 slabs in ONE launch: workgroup b works on slab b % nslab (co0 = slab * slab_rows)
  // operands that are functions of a stored tensor (ppsci_pw_virtual): xmode for the input x, zmode for zmul
  int xmode, zmode, K0;
  const float* x0;     // [B, K0, P]
  const float* W0;     // [C, K0]
  const float* b0;     // [C] or null
  int vrows, vt_off;   // virtual operands: C, and where its table {W0 row, zero padded} [C] | {b0} [C] starts in LDS (floats)
};

// GELU(W0 x0 + b0) at this lane's N pixels, w0 = row k of W0 (zero beyond K0), bk = b0[k], x0q: the K0 <= 4 rows of x0
// there (zero beyond K0); `grad`: GELU' of it
template <int N = 4>
__device__ __forceinline__ f32x4 pw_virtual(f32x4 w0, float bk, const f32x4 (&x0q)[4], bool grad) {
  f32x4 z = (f32x4){bk, bk, bk, bk};
#pragma unroll
  for (int i = 0; i < 4; ++i) z += w0[i] * x0q[i];
#pragma unroll
  for (int t = 0; t < N; ++t) z[t] = grad ? fno_gelu_grad(z[t]) : fno_gelu(z[t]);
  return z;
}

// the B operand of channel k (< Cin, else zero) at this lane's 4 pixels
// VM (compile time, so that the plain convolution's load loop has no branches): 0 plain operands, 1 x = GELU(stored),
// 2 x = GELU(W0 x0 + b0), 3 zmul = GELU'(W0 x0 + b0)
template <int N, int VM>
__device__ __forceinline__ f32x4 pw_bop(const PwArgs& a, const float* xb, int k, int p0, bool al, const f32x4 (&x0q)[4],
                                        const f32x4* w0t, const float* b0t) {
  if constexpr (VM == 2) return k < a.Cin ? pw_virtual<N>(w0t[k], b0t[k], x0q, false) : (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 v;
  if constexpr (N == 4) {
    // (one select per load on flags computed once per item: the compiler keeps the eight loads of a k-step together)
    const bool pok = al && p0 + 3 < a.P;
    if (al) v = (pok && k < a.Cin) ? *(const f32x4*)&xb[(long long)k * a.P + p0] : (f32x4){0.f, 0.f, 0.f, 0.f};
    else v = k < a.Cin ? fno_ld4(xb + (long long)k * a.P, p0, a.P, false) : (f32x4){0.f, 0.f, 0.f, 0.f};
  } else {
    v = k < a.Cin ? fno_ldn<N>(xb + (long long)k * a.P, p0, a.P, al) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if constexpr (VM == 1) {
#pragma unroll
    for (int t = 0; t < N; ++t) v[t] = fno_gelu(v[t]);
  }
  return v;
}

#define PW_OC_MAX 4  // output-channel blocks (of 16) per work item: 4 with 4 waves per workgroup, or -- when the weight
                     // slab leaves room for ONE workgroup per CU -- 2 with 8 waves, so that every SIMD holds two waves and
                     // one wave's MFMA chains cover the other's operand waits
#define PW_STAGE 16  // weight float4s in flight per thread while staging

template <int PW_OC, int PW_WAVES, int NPX, int VM, bool AL>
__global__ void __launch_bounds__(64 * PW_WAVES, 2) pw_conv_kernel(PwArgs a) {
  PPSCI_DYN_SMEM(smem);  // weight fragments: [(ob * kq + q) * 64 + lane] float4
  // several output-channel slabs in one launch: neighbouring workgroups take different slabs, so that the weight stage
  // of one workgroup on a CU overlaps the MFMA phase of another (64 KB slabs: two or more workgroups per CU)
  const int slab = (int)blockIdx.x % a.nslab, wg = (int)blockIdx.x / a.nslab, nwg = (int)gridDim.x / a.nslab;
  a.co0 = slab * a.slab_rows;
  a.Cout = a.CoutT - a.co0 < a.slab_rows ? a.CoutT - a.co0 : a.slab_rows;
  a.nob = (a.Cout + 15) / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  if constexpr (PPSCI_XDL) {
    // XDL: K = 32 steps.  Fragment (ob, q2) of lane (g, c): Weff[o = 16ob + c][k = 32 q2 + 8g + j], j = 0..7, split into
    // three bf16 planes of 16 bytes per lane: smem[((ob * kq2 + q2) * 3 + plane) * 64 + lane] (u32x4).  The split is
    // done here, once per workgroup and slab (a thread reads its eight weights: two float4 along k, or eight rows when
    // the matrix is used transposed).
    const int kq2 = (a.Cin + 31) / 32;
    u32x4* fr = (u32x4*)smem;
    for (int idx = tid; idx < a.nob * kq2 * 64; idx += blockDim.x) {
      const int l = idx & 63, q2 = (idx >> 6) % kq2, ob = (idx >> 6) / kq2;
      const int o = 16 * ob + (l & 15), k0 = 32 * q2 + 8 * (l >> 4);
      f32x4 w0 = (f32x4){0.f, 0.f, 0.f, 0.f}, w1 = w0;
      if (o < a.Cout) {
        if (!a.transpose && a.vec && k0 + 7 < a.Cin) {
          const float* src = &a.W[(long long)(a.co0 + o) * a.ldw + k0];
          w0 = *(const f32x4*)src;
          w1 = *(const f32x4*)(src + 4);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            const float w = k < a.Cin ? (a.transpose ? a.W[(long long)k * a.ldw + a.co0 + o] : a.W[(long long)(a.co0 + o) * a.ldw + k]) : 0.f;
            if (j < 4) w0[j] = w;
            else w1[j - 4] = w;
          }
        }
      }
      const ppsci_split4 s0 = ppsci_split(w0), s1 = ppsci_split(w1);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        fr[((long long)(ob * kq2 + q2) * 3 + pl) * 64 + l] = (u32x4){s0.p[pl][0], s0.p[pl][1], s1.p[pl][0], s1.p[pl][1]};
    }
  } else
  // stage W as A-operand fragments: comp r of lane (g,c) for (ob, q): Weff[o = 16ob + c][k = 16q + 4r + g].
  // Fast paths (no integer division, 16-byte coalesced global loads, 16 loads in flight per thread): a thread reads
  // four consecutive elements along the matrix' contiguous axis and scatters them to the four lanes / components
  // they belong to.
  if (a.vec && tid < 256) {
    const int hi = tid >> 4, lo = tid & 15;  // 16 rows x 16 float4 columns per pass (the first 256 threads)
    // A thread's float4s are enumerated (outer, inner): outer = output block (plain) / k-slab q (transposed), inner =
    // its float4 column lo, lo + 16, ...; PW_STAGE of them are loaded before the first LDS write.
    const int nouter = a.transpose ? a.kq : a.nob;
    const int ninner = a.transpose ? (4 * a.nob + 15 - lo) / 16 : (4 * a.kq + 15 - lo) / 16;  // columns lo + 16 j < 4 * n
    const int k4n = a.Cin >> 2, o4n = a.Cout >> 2;  // Cout (slab) is a multiple of 4 on the transposed path
    int eo = 0, ej = 0;  // running (outer, inner) of the next float4 to load
    const int total = nouter * ninner;
    for (int e0 = 0; e0 < total; e0 += PW_STAGE) {
      f32x4 buf[PW_STAGE];
      int lo_o = eo, lo_j = ej;
#pragma unroll
      for (int u = 0; u < PW_STAGE; ++u) {
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (e0 + u < total) {
          const int c4 = lo + 16 * lo_j;
          if (!a.transpose) {  // W[o][k], contiguous along k: float4 = k 16q + 4r .. + 3 (g = 0..3) of row o
            const int o = 16 * lo_o + hi;
            if (o < a.Cout && c4 < k4n) v = *(const f32x4*)&a.W[(long long)(a.co0 + o) * a.ldw + 4 * c4];
          } else {  // W[k][o], contiguous along o: float4 = o 16ob + 4c4' .. + 3 of row k
            const int k = 16 * lo_o + hi;
            if (k < a.Cin && c4 < o4n) v = *(const f32x4*)&a.W[(long long)k * a.ldw + a.co0 + 4 * c4];
          }
          if (++lo_j == ninner) { lo_j = 0; ++lo_o; }
        }
        buf[u] = v;
      }
#pragma unroll
      for (int u = 0; u < PW_STAGE; ++u) {
        if (e0 + u < total) {
          const int c4 = lo + 16 * ej;
          if (!a.transpose) {  // -> lanes (g, c = hi), component r
            const int q = c4 >> 2, r = c4 & 3;
            float* dst = smem + ((long long)(eo * a.kq + q) * 64 + hi) * 4 + r;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) dst[gg * 64] = buf[u][gg];
          } else {  // -> lanes (g2, c0 + e), same (q, r)
            const int r = hi >> 2, g2 = hi & 3, ob = c4 >> 2, c0 = (c4 & 3) * 4;
            float* dst = smem + ((long long)(ob * a.kq + eo) * 64 + g2 * 16 + c0) * 4 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e * 4] = buf[u][e];
          }
          if (++ej == ninner) { ej = 0; ++eo; }
        }
      }
    }
  } else if (!a.vec) {
    for (int idx = tid; idx < a.nob * a.kq * 64; idx += blockDim.x) {
      const int l = idx & 63, q = (idx >> 6) % a.kq, ob = (idx >> 6) / a.kq;
      const int o = 16 * ob + (l & 15);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * q + 4 * r + (l >> 4);
        float w = 0.f;
        if (o < a.Cout && k < a.Cin)
          w = a.transpose ? a.W[(long long)k * a.ldw + a.co0 + o] : a.W[(long long)(a.co0 + o) * a.ldw + k];
        v[r] = w;
      }
      *(f32x4*)&smem[(long long)idx * 4] = v;
    }
  }
  // virtual operands: rows of W0 (zero padded to 4) and b0 behind the weight fragments
  f32x4* w0t = (f32x4*)(smem + a.vt_off);
  float* b0t = (float*)(w0t + a.vrows);
  for (int k = tid; VM >= 2 && k < a.vrows; k += (int)blockDim.x) {
    f32x4 w = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < a.K0) w[q] = a.W0[(long long)k * a.K0 + q];
    w0t[k] = w;
    b0t[k] = a.b0 ? a.b0[k] : 0.f;
  }
  __syncthreads();
  constexpr int CH = 16 * NPX;  // pixels per work item: NPX per lane (see ppsci_pw_conv: 4, or fewer for more waves)
  const long long chunks_per_b = (a.P + CH - 1) / CH;
  const long long nchunk = (long long)a.B * chunks_per_b;
  // work item = (16 NPX-pixel chunk, group of PW_OC output blocks): the waves of a workgroup take neighbouring groups of
  // the same chunk (its B operands then come from L1), and wide layers on few pixels still fill the chip
  const int ngrp = (a.nob + PW_OC - 1) / PW_OC;
  const long long nitem = nchunk * ngrp;
  for (long long item = (long long)wg * PW_WAVES + wave; item < nitem; item += (long long)nwg * PW_WAVES) {
    const long long ch = item / ngrp;
    const int ob0 = (int)(item - ch * ngrp) * PW_OC;
    const int b = (int)(ch / chunks_per_b);
    const int p0 = (int)(ch - (long long)b * chunks_per_b) * CH + NPX * c;  // this lane's NPX pixels
    constexpr bool al = AL;  // P a multiple of NPX: one 4 NPX-byte access (all pixels or none); see fno_ld4
    const float* xb = a.x + (long long)b * a.Cin * a.P;
    f32x4 x0q[4];  // rows of x0 at this lane's pixels (virtual operands)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      x0q[i] = (VM >= 2 && i < a.K0) ? fno_ldn<NPX>(a.x0 + ((long long)b * a.K0 + i) * a.P, p0, a.P, al)
                                     : (f32x4){0.f, 0.f, 0.f, 0.f};
    {
      f32x4 acc[PW_OC][4];
#pragma unroll
      for (int j = 0; j < PW_OC; ++j)
#pragma unroll
        for (int t = 0; t < NPX; ++t) acc[j][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (PPSCI_XDL) {
        // K = 32 step q2: lane (g, c) loads channels 32 q2 + 8g + j (j = 0..7), pixels p0..p0+3 (eight float4, each a
        // 256-byte run per channel row over the 16 lanes of a group); pixel t of the float4s is the B operand of column
        // tile t: its eight values are split into three bf16 planes in registers, then six products per (block, tile).
        const int kq2 = (a.Cin + 31) / 32;
        const u32x4* fr = (const u32x4*)smem;
        f32x4 xn[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 8 * g + j;
          xn[j] = pw_bop<NPX, VM>(a, xb, k, p0, al, x0q, w0t, b0t);
        }
        for (int q2 = 0; q2 < kq2; ++q2) {
          u32x4 bp[4][3];  // [tile][plane]
#pragma unroll
          for (int t = 0; t < NPX; ++t) {
            const ppsci_split4 s0 = ppsci_split((f32x4){xn[0][t], xn[1][t], xn[2][t], xn[3][t]});
            const ppsci_split4 s1 = ppsci_split((f32x4){xn[4][t], xn[5][t], xn[6][t], xn[7][t]});
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) bp[t][pl] = (u32x4){s0.p[pl][0], s0.p[pl][1], s1.p[pl][0], s1.p[pl][1]};
          }
          if (q2 + 1 < kq2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int k = 32 * (q2 + 1) + 8 * g + j;
              xn[j] = pw_bop<NPX, VM>(a, xb, k, p0, al, x0q, w0t, b0t);
            }
          }
#pragma unroll
          for (int j = 0; j < PW_OC; ++j) {
            if (ob0 + j < a.nob) {
              const u32x4* f = &fr[((long long)((ob0 + j) * kq2 + q2) * 3) * 64 + lane];
              const u32x4 ap[3] = {f[0], f[64], f[128]};
#pragma unroll
              for (int q = 0; q < PPSCI_XDL_NPROD; ++q)
#pragma unroll
                for (int t = 0; t < NPX; ++t)
                  acc[j][t] = ppsci_xdl32aa(ap[ppsci_xdl_pa[q]], bp[t][ppsci_xdl_pb[q]], acc[j][t]);
            }
          }
        }
      } else {
      f32x4 xn[4];  // k-step r: channel 16q + 4r + g, pixels p0..p0+3; loaded one q ahead of its MFMA chains
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 4 * r + g;
        xn[r] = pw_bop<NPX, VM>(a, xb, k, p0, al, x0q, w0t, b0t);
      }
      for (int q = 0; q < a.kq; ++q) {
        f32x4 xv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[r] = xn[r];
        if (q + 1 < a.kq) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * (q + 1) + 4 * r + g;
            xn[r] = pw_bop<NPX, VM>(a, xb, k, p0, al, x0q, w0t, b0t);
          }
        }
#pragma unroll
        for (int j = 0; j < PW_OC; ++j) {
          if (ob0 + j < a.nob) {
            const f32x4 w4 = *(const f32x4*)&smem[((long long)((ob0 + j) * a.kq + q) * 64 + lane) * 4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int t = 0; t < NPX; ++t) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[r], xv[r][t], acc[j][t], 0, 0, 0);
          }
        }
      }
      }
      // D_t[row = 4g + rr][col = c]: channel 16(ob0+j) + 4g + rr, pixel p0 + t
#pragma unroll
      for (int j = 0; j < PW_OC; ++j) {
        if (ob0 + j >= a.nob) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int o = 16 * (ob0 + j) + 4 * g + rr;
          if (o >= a.Cout || p0 >= a.P) continue;
          const long long off = ((long long)b * a.CoutT + a.co0 + o) * a.P;  // this row
          f32x4 v = (f32x4){acc[j][0][rr], acc[j][1][rr], acc[j][2][rr], acc[j][3][rr]};
          if (a.bias) v += a.bias[a.co0 + o];
          if constexpr (VM == 3) {
            v *= pw_virtual<NPX>(w0t[a.co0 + o], b0t[a.co0 + o], x0q, true);
          } else if (a.zmul) {
            const f32x4 z = fno_ldn<NPX>(a.zmul + off, p0, a.P, al);
#pragma unroll
            for (int t = 0; t < NPX; ++t) v[t] *= fno_gelu_grad(z[t]);
          }
          if (a.accumulate) v += fno_ldn<NPX>(a.out + off, p0, a.P, al);
          fno_stn<NPX>(a.out + off, p0, a.P, al, v);
          if (a.act) {
            f32x4 y;
#pragma unroll
            for (int t = 0; t < NPX; ++t) y[t] = fno_gelu(v[t]);
            fno_stn<NPX>(a.act + off, p0, a.P, al, y);
          }
        }
      }
    }
  }
}

// Testing / tuning knob: pixels per lane of the 1x1 convolution (1, 2, 4); 0 = chosen from the problem size.
static int g_pw_npx = 0;
extern "C" void ppsci_set_pw_pixels_per_lane(int npx) { g_pw_npx = npx; }

static int pw_virtual_check(const ppsci_pw_virtual* v, const char* what) {
  if (!v || v->mode == 0 || v->mode == 1) return PPSCI_OK;
  if (v->mode != 2 || !v->x0 || !v->W0 || v->K0 < 1 || v->K0 > 4) {
    ppsci_set_error("%s: invalid virtual operand (mode 2 needs x0, W0 and 1 <= K0 <= 4)", what);
    return PPSCI_E_INVALID;
  }
  return PPSCI_OK;
}

static int pw_conv_run(int B, int Cin, int Cout, int P, const float* x, const ppsci_pw_virtual* xv, const float* W,
                       int transpose, const float* bias, const float* zmul, const ppsci_pw_virtual* zv, int accumulate,
                       float* out, float* act, void* stream);

extern "C" int ppsci_pw_conv(int B, int Cin, int Cout, int P, const float* x, const float* W, int transpose,
                             const float* bias, const float* zmul, int accumulate, float* out, float* act, void* stream) {
  return pw_conv_run(B, Cin, Cout, P, x, nullptr, W, transpose, bias, zmul, nullptr, accumulate, out, act, stream);
}

extern "C" int ppsci_pw_conv_v(int B, int Cin, int Cout, int P, const float* x, const ppsci_pw_virtual* xv, const float* W,
                               int transpose, const float* bias, const float* zmul, const ppsci_pw_virtual* zv,
                               int accumulate, float* out, float* act, void* stream) {
  return pw_conv_run(B, Cin, Cout, P, x, xv, W, transpose, bias, zmul, zv, accumulate, out, act, stream);
}

static int pw_conv_run(int B, int Cin, int Cout, int P, const float* x, const ppsci_pw_virtual* xv, const float* W,
                       int transpose, const float* bias, const float* zmul, const ppsci_pw_virtual* zv, int accumulate,
                       float* out, float* act, void* stream) {
  const int xmode = xv ? xv->mode : 0, zmode = zv ? zv->mode : 0;
  if (B < 1 || Cin < 1 || Cout < 1 || P < 1 || (!x && xmode != 2) || !W || !out || zmode == 1 ||
      pw_virtual_check(xv, "pw_conv") != PPSCI_OK || pw_virtual_check(zv, "pw_conv") != PPSCI_OK) {
    ppsci_set_error("pw_conv: invalid argument");
    return PPSCI_E_INVALID;
  }
  if (xmode != 0 && zmode == 2) {
    ppsci_set_error("pw_conv: a virtual zmul together with a virtual / GELU x operand has no kernel instance");
    return PPSCI_E_UNSUPPORTED;
  }
  PwArgs a;
  memset(&a, 0, sizeof(a));
  a.xmode = xmode, a.zmode = zmode;
  if (xmode == 2) a.x0 = xv->x0, a.W0 = xv->W0, a.b0 = xv->b0, a.K0 = xv->K0;
  if (zmode == 2) a.x0 = zv->x0, a.W0 = zv->W0, a.b0 = zv->b0, a.K0 = zv->K0;
  a.x = x, a.W = W, a.bias = bias, a.zmul = zmul, a.out = out, a.act = act;
  a.B = B, a.Cin = Cin, a.Cout = Cout, a.P = P, a.transpose = transpose, a.accumulate = accumulate;
  a.ldw = transpose ? Cout : Cin;  // W is [Co, Ci] = [rows, ldw]; transposed use: rows = Cin(of this call), ld = Cout
  a.kq = (Cin + 15) / 16;
  a.CoutT = Cout;
  // output-channel slabs: the A fragments of one slab (16-row blocks x kq x 1 KiB) must fit LDS.  Everything in one
  // workgroup's LDS when it is small (<= 64 KiB: FNO layers); otherwise slabs of about 64 KiB -- all of them in ONE
  // launch, two or more workgroups per CU with 8 waves each: the weight stage of one overlaps the MFMAs of the other.
  const int nob_all = (Cout + 15) / 16;
  // bytes of one 16-row block of fragments: fp32 16 B per lane and 16-channel slab; XDL three 16-byte planes per
  // lane and 32-channel slab
  const long long blk = PPSCI_XDL ? (long long)((Cin + 31) / 32) * 3 * 64 * 16 : (long long)a.kq * 64 * 16;
  if (blk > PPSCI_LDS_LIMIT_BYTES) {
    ppsci_set_error("pw_conv: a 16 x %d weight block does not fit LDS", Cin);
    return PPSCI_E_UNSUPPORTED;
  }
  int nob_slab = nob_all;
  if ((long long)nob_all * blk > 64 * 1024) {
    nob_slab = (int)(64 * 1024 / blk);
    nob_slab = nob_slab / 4 * 4;  // whole 4-block groups
    if (nob_slab < 4) nob_slab = (int)(PPSCI_LDS_LIMIT_BYTES / blk) >= 4 ? 4 : (int)(PPSCI_LDS_LIMIT_BYTES / blk);
    const int nslab0 = (nob_all + nob_slab - 1) / nob_slab;
    int per = (nob_all + nslab0 - 1) / nslab0;  // balanced
    per = (per + 3) / 4 * 4;
    if (per < nob_slab) nob_slab = per;
  }
  const int nslab = (nob_all + nob_slab - 1) / nob_slab;
  a.nslab = nslab;
  a.slab_rows = 16 * nob_slab;
  long long lds = (long long)nob_slab * blk;
  if (xmode == 2 || zmode == 2) {
    a.vrows = xmode == 2 ? Cin : Cout;
    a.vt_off = (int)(lds / 4);
    lds += 20LL * a.vrows;
  }
  // the 16-byte staging path needs every slab's first column / row aligned
  a.vec = ((reinterpret_cast<uintptr_t>(W) & 15) == 0 && (a.ldw & 3) == 0 &&
           (transpose ? (Cout & 3) == 0 : (Cin & 3) == 0)) ? 1 : 0;
  long long resident = PPSCI_LDS_LIMIT_BYTES / (lds > 0 ? lds : 1);
  if (resident < 1) resident = 1;
  if (resident > 4) resident = 4;
  // one workgroup per CU (a slab above 80 KiB): 8 waves of 2-block items so that every SIMD still holds two waves; otherwise
  // 4 waves of 4-block items (a 64-row slab = one item per chunk: the B operand is streamed once per slab)
  const bool wide = resident == 1;
  // (XDL: a work item always takes 4 output blocks, so that one split of the B operand feeds 96 MFMAs)
  const int oc = (wide && !PPSCI_XDL) ? 2 : 4, waves = wide ? 8 : 4;
  // pixels per lane (work item = 16 npx pixels): 4 (16-byte accesses) unless that leaves fewer than two waves per SIMD.
  // Measured on the 16 x 64 x 64 TFNO step (1024 items of 64 pixels at 4 per lane): round 4, step 0.844 ms at 4, 0.854 at 2,
  // 0.890 at 1; end of round 5, with the rest of the step shorter: 0.576 ms at 4, 0.562 at 2, 0.588 at 1 -- two waves per SIMD
  // now pay for the eight-byte accesses.
  const long long groups = (nob_slab + oc - 1) / oc;
  const long long want = 8LL * PPSCI_NUM_CU;
  int npx = g_pw_npx;
  const int vm = zmode == 2 ? 3 : xmode;
  if (vm != 0) {
    // the operand-evaluating instances: 4 pixels per lane; x = GELU(W0 x0 + b0) (mode 2: bound by the GELU arithmetic, whose
    // latencies a second wave hides) also 2 when 4 leave one wave per SIMD: lifting forward 31.2 -> 27.3 us (mode 1 got slower)
    npx = 4;
    if (vm == 2 && g_pw_npx != 4 && (long long)B * ((P + 63) / 64) * groups * nslab < want) npx = 2;
  } else if (npx != 1 && npx != 2 && npx != 4) {
    npx = 4;
    while (npx > 2 && (long long)B * ((P + 16 * npx - 1) / (16 * npx)) * groups * nslab < want) npx >>= 1;
    while (npx > 1 && (long long)B * ((P + 16 * npx - 1) / (16 * npx)) * groups * nslab < PPSCI_NUM_CU) npx >>= 1;
  }
  // rows of P pixels start on 4 npx-byte boundaries: the aligned instances; otherwise element accesses, 4 pixels per lane
  const bool aligned = (P % npx) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (!aligned) npx = 4;
  const long long nchunk = (long long)B * ((P + 16 * npx - 1) / (16 * npx));
  const long long nitem = nchunk * groups;  // per slab
  long long wg_slab = (nitem + waves - 1) / waves;
  const long long cap = resident * PPSCI_NUM_CU / nslab > 0 ? resident * PPSCI_NUM_CU / nslab : 1;
  if (wg_slab > cap) wg_slab = cap;
  const long long grid = wg_slab * nslab;
  int se = 0;
#define PW_LAUNCH(OC, WV, NPX, VM, AL)                                                                               \
  do {                                                                                                               \
    se = PPSCI_SET_MAX_LDS((pw_conv_kernel<OC, WV, NPX, VM, AL>), (int)lds);                                         \
    if (se == 0) PPSCI_LAUNCH((pw_conv_kernel<OC, WV, NPX, VM, AL>), PwArgs, (int)grid, 64 * WV, (int)lds, stream, a); \
  } while (0)
#define PW_LAUNCH_ALL(OC, WV)                                \
  do {                                                       \
    if (!aligned) {                                          \
      if (vm == 1) PW_LAUNCH(OC, WV, 4, 1, false);           \
      else if (vm == 2) PW_LAUNCH(OC, WV, 4, 2, false);      \
      else if (vm == 3) PW_LAUNCH(OC, WV, 4, 3, false);      \
      else PW_LAUNCH(OC, WV, 4, 0, false);                   \
    } else if (vm == 2 && npx == 2) PW_LAUNCH(OC, WV, 2, 2, true); \
    else if (vm == 1) PW_LAUNCH(OC, WV, 4, 1, true);         \
    else if (vm == 2) PW_LAUNCH(OC, WV, 4, 2, true);         \
    else if (vm == 3) PW_LAUNCH(OC, WV, 4, 3, true);         \
    else if (npx == 4) PW_LAUNCH(OC, WV, 4, 0, true);        \
    else if (npx == 2) PW_LAUNCH(OC, WV, 2, 0, true);        \
    else PW_LAUNCH(OC, WV, 1, 0, true);                      \
  } while (0)
  if (wide) {
    constexpr int OCW = PPSCI_XDL ? 4 : 2;
    PW_LAUNCH_ALL(OCW, 8);
  } else {
    PW_LAUNCH_ALL(4, 4);
  }
#undef PW_LAUNCH_ALL
#undef PW_LAUNCH
  if (se != 0) {
    ppsci_set_error("pw_conv: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("pw_conv: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// ------------------------------------------------------------------------------------------ weight gradient
struct PwWArgs {
  const float* x;   // [B, Ci, P]
  const float* gy;  // [B, Co, P]
  float* part;      // [nchunk][Co*Ci]: per-chunk partial of gW (row-major [Co, Ci])
  float* part_b;    // [nchunk][Co] or null: per-chunk partial of gb
  int B, Ci, Co, P, nib, nob, cpix, chunks_per_b;
  long long ldp, ldpb;  // row strides of part / part_b (floats)
  int xmode, K0;      // x as a function of a stored tensor (ppsci_pw_virtual)
  const float* x0;
  const float* W0;
  const float* b0;
};

// four pixels p .. p + 3 (< lim) of input-channel row i of the weight gradient's x operand
// (w0, bk: row i of W0 and b0[i] of a virtual operand, loaded once per wave)
template <int XM>
__device__ __forceinline__ f32x4 pww_x(const PwWArgs& a, const float* xrow, int b, f32x4 w0, float bk, int p, int lim, bool al) {
  if constexpr (XM == 2) {
    f32x4 x0q[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      x0q[q] = q < a.K0 ? fno_ld4(a.x0 + ((long long)b * a.K0 + q) * a.P, p, lim, al) : (f32x4){0.f, 0.f, 0.f, 0.f};
    return pw_virtual(w0, bk, x0q, false);
  }
  f32x4 v = fno_ld4(xrow, p, lim, al);
  if constexpr (XM == 1) {
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = fno_gelu(v[t]);
  }
  return v;
}

// one wave per (pixel chunk, TB x TB group of 16 x 16 blocks) = a 16TB x 16TB tile of gW; cpix pixels of one sample per chunk
// (a multiple of 16).  TB*TB accumulators per wave: every operand float4 feeds TB MFMA chains -- the kernel is bound by
// the L2 traffic of its operands (each wave streams 2 * 16TB rows x cpix pixels), which per flop falls as 1 / TB.
// TB = 2 for small layers (a 32 x 32 FNO layer is ONE tile), TB = 4 from 128 x 128 on.
// WV = 4 (small layers, 256-pixel chunks): four waves per work item, a quarter of the chunk's pixels each, summed in wave order
// through LDS -- an FNO batch of 16 x 4 096 pixels is only 256 chunks, a quarter of the chip's SIMDs at one wave per chunk
// (10.7 us per 32 x 32 weight gradient), and smaller chunks would multiply the partial rows the reduction has to read.
template <int TB, int XM, bool AL, int WV = 1>
__global__ void __launch_bounds__(64 * WV, 2) pw_wgrad_kernel(PwWArgs a) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int wv = WV > 1 ? (int)(threadIdx.x >> 6) : 0;
  const int nibt = (a.nib + TB - 1) / TB, nobt = (a.nob + TB - 1) / TB;
  int id = blockIdx.x;
  const int ib = TB * (id % nibt);
  id /= nibt;
  const int ob = TB * (id % nobt);
  const int ch = id / nobt;
  const int b = ch / a.chunks_per_b;
  const int pc0 = (ch - b * a.chunks_per_b) * a.cpix;        // the chunk
  const int p0 = pc0 + wv * (a.cpix / WV);                    // this wave's share of it
  const float* gr[TB];
  const float* xr[TB];
  int xi[TB];
  f32x4 w0r[TB];
  float b0r[TB];
  float mo[TB], mi[TB];
#pragma unroll
  for (int u = 0; u < TB; ++u) {
    const int o = 16 * (ob + u) + c, i = 16 * (ib + u) + c;
    gr[u] = a.gy + ((long long)b * a.Co + (o < a.Co ? o : 0)) * a.P;
    xi[u] = i < a.Ci ? i : 0;
    xr[u] = a.x + ((long long)b * a.Ci + xi[u]) * a.P;
    w0r[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    b0r[u] = 0.f;
    if constexpr (XM == 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < a.K0) w0r[u][q] = a.W0[(long long)xi[u] * a.K0 + q];
      b0r[u] = a.b0 ? a.b0[xi[u]] : 0.f;
    }
    mo[u] = o < a.Co ? 1.f : 0.f;
    mi[u] = i < a.Ci ? 1.f : 0.f;
  }
  f32x4 acc[TB][TB];
#pragma unroll
  for (int u = 0; u < TB; ++u)
#pragma unroll
    for (int v = 0; v < TB; ++v) acc[u][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum[TB];
#pragma unroll
  for (int u = 0; u < TB; ++u) bsum[u] = 0.f;
  const int pend = p0 + a.cpix / WV < a.P ? p0 + a.cpix / WV : a.P;
  constexpr bool al = AL;  // P a multiple of 4 (and 16-byte aligned operands): see fno_ld4; the remainder loop zero-fills beyond pend
  int pbeg = p0;
  if constexpr (PPSCI_XDL) {
    // K = 32 pixels per step: lane (g, c) holds pixels p + 8g .. + 7 of its row for both operands (two float4 each),
    // split into three bf16 planes; six products per 16 x 16 block.  A 16-pixel remainder takes the fp32 loop below.
    for (; al && pbeg + 32 <= pend; pbeg += 32) {
      u32x4 gp[TB][3], xp[TB][3];
#pragma unroll
      for (int u = 0; u < TB; ++u) {
        const f32x4 g0 = *(const f32x4*)&gr[u][pbeg + 8 * g] * mo[u], g1 = *(const f32x4*)&gr[u][pbeg + 8 * g + 4] * mo[u];
        const f32x4 x0 = pww_x<XM>(a, xr[u], b, w0r[u], b0r[u], pbeg + 8 * g, pend, true) * mi[u],
                    x1 = pww_x<XM>(a, xr[u], b, w0r[u], b0r[u], pbeg + 8 * g + 4, pend, true) * mi[u];
        bsum[u] += ((g0[0] + g0[1]) + (g0[2] + g0[3])) + ((g1[0] + g1[1]) + (g1[2] + g1[3]));
        const ppsci_split4 a0 = ppsci_split(g0), a1 = ppsci_split(g1), b0 = ppsci_split(x0), b1 = ppsci_split(x1);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          gp[u][pl] = (u32x4){a0.p[pl][0], a0.p[pl][1], a1.p[pl][0], a1.p[pl][1]};
          xp[u][pl] = (u32x4){b0.p[pl][0], b0.p[pl][1], b1.p[pl][0], b1.p[pl][1]};
        }
      }
#pragma unroll
      for (int q = 0; q < PPSCI_XDL_NPROD; ++q)
#pragma unroll
        for (int u = 0; u < TB; ++u)
#pragma unroll
          for (int v = 0; v < TB; ++v) acc[u][v] = ppsci_xdl32aa(gp[u][ppsci_xdl_pa[q]], xp[v][ppsci_xdl_pb[q]], acc[u][v]);
    }
  }
  for (int p = pbeg; p < pend; p += 16) {
    // k-step r <-> pixel p + 4g + r for both operands
    f32x4 gv[TB], xv[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      gv[u] = fno_ld4(gr[u], p + 4 * g, pend, al) * mo[u];
      xv[u] = pww_x<XM>(a, xr[u], b, w0r[u], b0r[u], p + 4 * g, pend, al) * mi[u];
    }
#pragma unroll
    for (int u = 0; u < TB; ++u) {
#pragma unroll
      for (int v = 0; v < TB; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[u][v] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[u][r], xv[v][r], acc[u][v], 0, 0, 0);
      bsum[u] += (gv[u][0] + gv[u][1]) + (gv[u][2] + gv[u][3]);
    }
  }
  if constexpr (WV > 1) {  // waves 1 .. WV-1 hand their sums to wave 0, which adds them in wave order
    __shared__ float red[WV - 1][TB * TB * 4 + TB][64];
    if (wv > 0) {
#pragma unroll
      for (int u = 0; u < TB; ++u) {
#pragma unroll
        for (int v = 0; v < TB; ++v)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) red[wv - 1][(u * TB + v) * 4 + rr][lane] = acc[u][v][rr];
        red[wv - 1][TB * TB * 4 + u][lane] = bsum[u];
      }
    }
    __syncthreads();
    if (wv > 0) return;
#pragma unroll
    for (int w = 0; w < WV - 1; ++w)
#pragma unroll
      for (int u = 0; u < TB; ++u) {
#pragma unroll
        for (int v = 0; v < TB; ++v)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) acc[u][v][rr] += red[w][(u * TB + v) * 4 + rr][lane];
        bsum[u] += red[w][TB * TB * 4 + u][lane];
      }
  }
  float* prow = a.part + (long long)ch * a.ldp;
  // D[row = 4g + rr][col = c] = gW[o = 16ob + 4g + rr][i = 16ib + c]
#pragma unroll
  for (int u = 0; u < TB; ++u)
#pragma unroll
    for (int v = 0; v < TB; ++v) {
      const int i = 16 * (ib + v) + c;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int oo = 16 * (ob + u) + 4 * g + rr;
        if (oo < a.Co && i < a.Ci) prow[(long long)oo * a.Ci + i] = acc[u][v][rr];
      }
    }
  if (ib == 0 && a.part_b) {
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      float bs = bsum[u];
      bs += __shfl_xor(bs, 16, 64);
      bs += __shfl_xor(bs, 32, 64);
      const int o = 16 * (ob + u) + c;
      if (g == 0 && o < a.Co) a.part_b[(long long)ch * a.ldpb + o] = bs;
    }
  }
}

// pixels per chunk: 256 -- a 32x32 layer on a 16 x 64 x 64 batch is then 256 waves of 16 MFMA rounds instead of 64 waves
// of 64 (the kernel is latency-bound per wave); the partial rows are summed by ppsci_reduce_rows' tall variant
#define PW_WGRAD_CPIX 256
extern "C" int64_t ppsci_pw_conv_wgrad_chunks(int B, int P) {
  const int cpix = P >= PW_WGRAD_CPIX ? PW_WGRAD_CPIX : P;
  return (int64_t)B * ((P + cpix - 1) / cpix);
}

// part_w: [chunks][Co*Ci], part_b: [chunks][Co] (or null); sum each with ppsci_reduce_rows(part, chunks, cols, out)
static int pw_wgrad_run(int B, int Ci, int Co, int P, const float* x, const ppsci_pw_virtual* xv, const float* gy,
                        float* partials, float* partials_b, int64_t ld_partials, void* stream);

extern "C" int ppsci_pw_conv_wgrad(int B, int Ci, int Co, int P, const float* x, const float* gy, float* partials,
                                   float* partials_b, void* stream) {
  return pw_wgrad_run(B, Ci, Co, P, x, nullptr, gy, partials, partials_b, 0, stream);
}

extern "C" int ppsci_pw_conv_wgrad_v(int B, int Ci, int Co, int P, const float* x, const ppsci_pw_virtual* xv,
                                     const float* gy, float* partials, float* partials_b, int64_t ld_partials,
                                     void* stream) {
  return pw_wgrad_run(B, Ci, Co, P, x, xv, gy, partials, partials_b, ld_partials, stream);
}

static int pw_wgrad_run(int B, int Ci, int Co, int P, const float* x, const ppsci_pw_virtual* xv, const float* gy,
                        float* partials, float* partials_b, int64_t ld_partials, void* stream) {
  const int xmode = xv ? xv->mode : 0;
  if (B < 1 || Ci < 1 || Co < 1 || P < 1 || (!x && xmode != 2) || !gy || !partials ||
      pw_virtual_check(xv, "pw_conv_wgrad") != PPSCI_OK) {
    ppsci_set_error("pw_conv_wgrad: invalid argument");
    return PPSCI_E_INVALID;
  }
  PwWArgs a;
  memset(&a, 0, sizeof(a));
  a.xmode = xmode;
  if (xmode == 2) a.x0 = xv->x0, a.W0 = xv->W0, a.b0 = xv->b0, a.K0 = xv->K0;
  a.x = x, a.gy = gy, a.part = partials, a.part_b = partials_b;
  if (ld_partials != 0 && ld_partials < (int64_t)Co * Ci) {
    ppsci_set_error("pw_conv_wgrad: ld_partials smaller than a row");
    return PPSCI_E_INVALID;
  }
  a.ldp = ld_partials ? ld_partials : (long long)Co * Ci;
  a.ldpb = ld_partials ? ld_partials : Co;
  a.B = B, a.Ci = Ci, a.Co = Co, a.P = P;
  a.nib = (Ci + 15) / 16, a.nob = (Co + 15) / 16;
  a.cpix = P >= PW_WGRAD_CPIX ? PW_WGRAD_CPIX : P;
  a.chunks_per_b = (P + a.cpix - 1) / a.cpix;
  const bool aligned = (P & 3) == 0 && (reinterpret_cast<uintptr_t>(gy) & 15) == 0 &&
                       (xmode == 2 ? (reinterpret_cast<uintptr_t>(xv->x0) & 15) == 0 : (reinterpret_cast<uintptr_t>(x) & 15) == 0);
#define PWW_LAUNCH(TB)                                                                                          \
  do {                                                                                                          \
    if (aligned) {                                                                                              \
      if (xmode == 2) PPSCI_LAUNCH((pw_wgrad_kernel<TB, 2, true>), PwWArgs, (int)grid, 64, 0, stream, a);       \
      else if (xmode == 1) PPSCI_LAUNCH((pw_wgrad_kernel<TB, 1, true>), PwWArgs, (int)grid, 64, 0, stream, a);  \
      else PPSCI_LAUNCH((pw_wgrad_kernel<TB, 0, true>), PwWArgs, (int)grid, 64, 0, stream, a);                  \
    } else {                                                                                                    \
      if (xmode == 2) PPSCI_LAUNCH((pw_wgrad_kernel<TB, 2, false>), PwWArgs, (int)grid, 64, 0, stream, a);      \
      else if (xmode == 1) PPSCI_LAUNCH((pw_wgrad_kernel<TB, 1, false>), PwWArgs, (int)grid, 64, 0, stream, a); \
      else PPSCI_LAUNCH((pw_wgrad_kernel<TB, 0, false>), PwWArgs, (int)grid, 64, 0, stream, a);                 \
    }                                                                                                           \
  } while (0)
  if (Ci >= 128 && Co >= 128) {
    const long long grid = (long long)B * a.chunks_per_b * ((a.nob + 3) / 4) * ((a.nib + 3) / 4);
    PWW_LAUNCH(4);
  } else {
    const long long grid = (long long)B * a.chunks_per_b * ((a.nob + 1) / 2) * ((a.nib + 1) / 2);
    if (a.cpix == PW_WGRAD_CPIX && aligned && grid < 4096) {  // few work items: four waves each (see the kernel)
      if (xmode == 2) PPSCI_LAUNCH((pw_wgrad_kernel<2, 2, true, 4>), PwWArgs, (int)grid, 256, 0, stream, a);
      else if (xmode == 1) PPSCI_LAUNCH((pw_wgrad_kernel<2, 1, true, 4>), PwWArgs, (int)grid, 256, 0, stream, a);
      else PPSCI_LAUNCH((pw_wgrad_kernel<2, 0, true, 4>), PwWArgs, (int)grid, 256, 0, stream, a);
    } else
      PWW_LAUNCH(2);
  }
#undef PWW_LAUNCH
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("pw_conv_wgrad: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// ------------------------------------------------------------------------------------------ GroupNorm(1 group) block tail
// forward:  u = v + sbias[c];  xh = (u - mean_b) * rstd_b;  t = xh * gamma[c] + beta[c] + skip;  y = gelu ? GELU(t) : t
// (norm == 0: t = u + skip)
struct GnArgs {
  const float* v;      // [B, C, P] spectral convolution output (before its bias)
  const float* sbias;  // [C] spectral bias
  const float* gamma;  // [C] (norm only)
  const float* beta;   // [C]
  const float* skip;   // [B, C, P] or null
  float* t;            // [B, C, P] pre-activation
  float* y;            // [B, C, P] or null (== t when there is no activation)
  float* rows;         // [B*C][4] per row: forward the fp32 mean mr, sum (u - mr)^2, sum (u - mr); backward sum gt, sum gt*xh, sum xh
  float* stats;        // [B][2]: mean, rstd
  const float* gout;   // backward: dL/dy
  const float* gout2;  // backward: a second addend of dL/dy, or null (the spectral branch's share of the next block)
  float* gt;           // backward: dL/dt (also the gradient of the skip branch)
  float* gv;           // backward: dL/dv
  float* ggamma;       // backward: [C] dL/dgamma (norm only), [C] dL/dbeta (norm only), [C] dL/d(spectral bias);
  float* gbeta;        //           each may be null
  float* gsbias;
  int B, C, P, norm, gelu;
  float eps;
  DftArgs d;           // DFT instances: the kept modes of the plane this workgroup produces (y forward, gv backward) -> d.dst
  DftArgs di;          // INV instance of the backward's first pass: the second gradient addend arrives as kept modes (di.src)
};

// puts four neighbouring values of the row into the LDS plane [H][W + 1] of the transform
__device__ __forceinline__ void gn_to_plane(float* pl, int W, int p, int P, f32x4 v) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (p + k < P) pl[p + k + (p + k) / W] = v[k];
}

// sums of two doubles over the 256 threads, fixed-shape tree in LDS (red: 512 doubles); results in every thread
__device__ __forceinline__ void fno_block_sum_d2(double& u, double& v, double* red) {
  __syncthreads();
  red[threadIdx.x] = u;
  red[256 + threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      red[256 + threadIdx.x] += red[256 + threadIdx.x + w];
    }
    __syncthreads();
  }
  u = red[0];
  v = red[256];
}

// one workgroup (256 threads) per (b, c) row
template <bool AL>
__global__ void __launch_bounds__(256) gn_rowstats_kernel(GnArgs a) {
  __shared__ float red[4];
  const int row = blockIdx.x, c = row % a.C;
  const float* vr = a.v + (long long)row * a.P;
  const float sb = a.sbias ? a.sbias[c] : 0.f;
  float s1 = 0.f;
  constexpr bool al = AL;
  for (int p = threadIdx.x * 4; p < a.P; p += 1024) {
    f32x4 u = fno_ld4(vr, p, a.P, al) + sb;
    if (!al) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k >= a.P) u[k] = 0.f;
    }
    s1 += (u[0] + u[1]) + (u[2] + u[3]);
  }
  // The variance comes from squared deviations, never from sum(u^2) - P mean^2 (which loses (mean / std)^2 ulps: a field
  // with an offset).  mr: the row mean as far as fp32 sums give it; a second sweep over the row (hot in cache) takes the
  // deviations about it.  The row's exact mean is mr + d1 / P, its squared deviations about that are d2 - d1^2 / P.
  const float mr = ppsci_block_sum256(s1, red) / (float)a.P;
  float d1 = 0.f, d2 = 0.f;
  for (int p = threadIdx.x * 4; p < a.P; p += 1024) {
    f32x4 dd = (fno_ld4(vr, p, a.P, al) + sb) - mr;
    if (!al) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k >= a.P) dd[k] = 0.f;
    }
    d1 += (dd[0] + dd[1]) + (dd[2] + dd[3]);
    d2 += (dd[0] * dd[0] + dd[1] * dd[1]) + (dd[2] * dd[2] + dd[3] * dd[3]);
  }
  d1 = ppsci_block_sum256(d1, red);
  d2 = ppsci_block_sum256(d2, red);
  if (threadIdx.x == 0) {
    a.rows[(long long)row * 4 + 0] = mr;
    a.rows[(long long)row * 4 + 1] = d2;
    a.rows[(long long)row * 4 + 2] = d1;
  }
}

// one workgroup per (b, c) row.  The statistics of sample b are finished HERE from the row sums (C pairs, in double, a
// fixed-shape tree) -- by every workgroup of the sample in parallel instead of a one-workgroup kernel between the row
// pass and this one (that kernel was a 5 us serial chain); the workgroup of channel 0 stores them for the backward pass.
template <bool AL, bool DFT>
__global__ void __launch_bounds__(256) gn_apply_kernel(GnArgs a) {
  __shared__ double red[512];
  PPSCI_DYN_SMEM(smem);  // DFT: tw | th | plane | T | partial sums (dft_kept.h)
  float* tw = smem;
  float* th = tw + 2 * a.d.W * a.d.my;
  float* pl = th + 2 * a.d.H * a.d.mx;
  float* T = pl + a.d.H * (a.d.W + 1);
  if constexpr (DFT) dft_twiddles(a.d, tw);  // (in flight during the statistics below)
  const int row = blockIdx.x, c = row % a.C, b = row / a.C;
  const long long base = (long long)row * a.P;
  float mean = 0.f, rstd = 1.f;
  if (a.norm) {
    // the C rows of the sample merged in double: row c has the mean m_c = mr + d1 / P and the squared deviations
    // M2_c = d2 - d1^2 / P about it (gn_rowstats_kernel; dft_inv_row_stats in dft_kept.h), and
    //   var = (sum_c M2_c + P sum_c (m_c - m)^2) / n,  the row means taken relative to row 0's (K)
    const double Pd = (double)a.P;
    const float* r0 = a.rows + (long long)b * a.C * 4;
    const double K = (double)r0[0] + (double)r0[2] / Pd;
    double s = 0.0, q = 0.0;
    for (int cc = threadIdx.x; cc < a.C; cc += 256) {
      const double mr = (double)r0[cc * 4 + 0], d2 = (double)r0[cc * 4 + 1], d1 = (double)r0[cc * 4 + 2];
      const double dm = (mr + d1 / Pd) - K;
      s += dm;
      q += (d2 - d1 * d1 / Pd) + Pd * dm * dm;
    }
    fno_block_sum_d2(s, q, red);
    const double n = (double)a.C * Pd, m = K + s / (double)a.C;
    double var = (q - Pd * s * s / (double)a.C) / n;
    if (var < 0.0) var = 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    if (c == 0 && threadIdx.x == 0) {
      a.stats[2 * b + 0] = mean;
      a.stats[2 * b + 1] = rstd;
    }
  }
  constexpr bool al = AL;
  const float sb = a.sbias ? a.sbias[c] : 0.f;
  const float sc = a.norm ? rstd * a.gamma[c] : 1.f, sh = a.norm ? a.beta[c] : 0.f;
  for (int p = threadIdx.x * 4; p < a.P; p += 1024) {
    f32x4 u = fno_ld4(a.v + base, p, a.P, al) + sb;
    if (a.norm) u = (u - mean) * sc + sh;
    if (a.skip) u += fno_ld4(a.skip + base, p, a.P, al);
    fno_st4(a.t + base, p, a.P, al, u);
    if (a.y) {
      f32x4 y = u;
      if (a.gelu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fno_gelu(u[k]);
      }
      fno_st4(a.y + base, p, a.P, al, y);
      if constexpr (DFT) gn_to_plane(pl, a.d.W, p, a.P, y);
    }
  }
  if constexpr (DFT) {  // y is the next block's input: its kept modes now, from LDS, instead of a transform launch that reads it back
    __syncthreads();
    dft_fwd_stages(a.d, tw, th, pl, T, a.d.dst + (long long)row * a.d.mx * a.d.my * 2);
  }
}

// backward pass 1: gt = gout * GELU'(t); row sums of gt, gt * xh, xh
template <bool AL, bool INV>
__global__ void __launch_bounds__(256) gn_bwd_rows_kernel(GnArgs a) {
  __shared__ float red[4];
  const int row = blockIdx.x, c = row % a.C, b = row / a.C;
  const long long base = (long long)row * a.P;
  // INV: the second addend of dL/dy is the inverse transform of this plane's kept modes (the spectral branch's gradient of
  // the block behind): evaluated here into LDS instead of a transform launch that writes the plane for this kernel to read
  PPSCI_DYN_SMEM(smem);  // tw | th | Z | T | plane [H][W]
  float* pl2 = nullptr;
  if constexpr (INV) {
    float* tw = smem;
    float* th = tw + 2 * a.di.W * a.di.my;
    float* Z = th + 2 * a.di.H * a.di.mx;
    float* T = Z + 2 * a.di.mx * a.di.my;
    pl2 = T + 2 * a.di.H * a.di.my;
    const int nm2 = 2 * a.di.mx * a.di.my;
    const float* z = a.di.src + (long long)row * nm2;
    for (int e = threadIdx.x; e < nm2; e += 256) Z[e] = z[e];
    dft_twiddles(a.di, tw);
    __syncthreads();
    float* const out = pl2;
    const int W_ = a.di.W;
    dft_inv_stages(a.di, tw, th, Z, T, [&](int hh, int w, float val) { out[hh * W_ + w] = val; });
    __syncthreads();
  }
  const float sb = a.sbias ? a.sbias[c] : 0.f;
  const float mean = a.norm ? a.stats[2 * b] : 0.f, rstd = a.norm ? a.stats[2 * b + 1] : 1.f;
  float r1 = 0.f, r2 = 0.f, r3 = 0.f;
  constexpr bool al = AL;
  for (int p = threadIdx.x * 4; p < a.P; p += 1024) {
    f32x4 g4 = fno_ld4(a.gout + base, p, a.P, al);  // zero beyond the row: such elements add nothing to r1, r2
    if (a.gout2) g4 += fno_ld4(a.gout2 + base, p, a.P, al);
    if constexpr (INV) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < a.P) g4[k] += pl2[p + k];
    }
    if (a.gelu) {
      const f32x4 t4 = fno_ld4(a.t + base, p, a.P, al);
#pragma unroll
      for (int k = 0; k < 4; ++k) g4[k] *= fno_gelu_grad(t4[k]);
    }
    fno_st4(a.gt + base, p, a.P, al, g4);
    f32x4 xh = (fno_ld4(a.v + base, p, a.P, al) + sb - mean) * rstd;
    if (!al) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k >= a.P) xh[k] = 0.f;
    }
    r1 += (g4[0] + g4[1]) + (g4[2] + g4[3]);
    r2 += (g4[0] * xh[0] + g4[1] * xh[1]) + (g4[2] * xh[2] + g4[3] * xh[3]);
    r3 += (xh[0] + xh[1]) + (xh[2] + xh[3]);
  }
  r1 = ppsci_block_sum256(r1, red);
  r2 = ppsci_block_sum256(r2, red);
  r3 = ppsci_block_sum256(r3, red);
  if (threadIdx.x == 0) {
    a.rows[(long long)row * 4 + 0] = r1;
    a.rows[(long long)row * 4 + 1] = r2;
    a.rows[(long long)row * 4 + 2] = r3;
  }
}

// backward pass 2, one workgroup per (b, c) row: gv = rstd (gamma gt - m1 - xh m2)   (norm == 0: gv = gt), with
// m1 = sum_c gamma r1 / n, m2 = sum_c gamma r2 / n of sample b finished here from the row sums of pass 1 (as in
// gn_apply_kernel).  The workgroups of sample 0 also write the parameter gradients of their channel c:
//   dgamma[c] = sum_b r2[b,c],  dbeta[c] = sum_b r1[b,c],
//   dsbias[c] = sum_b rstd_b (gamma_c r1[b,c] - P m1_b - r3[b,c] m2_b)     (= sum over b and p of gv; norm == 0: sum_b r1)
// -- m1_b, m2_b of every sample again from the row sums: 16 threads per sample, 16 samples at a time, all in a fixed order.
// (Round 3 had a one-workgroup kernel between the passes for all of this: 9.9 us of serial double-precision loops.)
template <bool AL, bool DFT>
__global__ void __launch_bounds__(256) gn_bwd_apply_kernel(GnArgs a) {
  __shared__ double red[512];
  PPSCI_DYN_SMEM(smem);  // DFT: tw | th | plane | T | partial sums (dft_kept.h)
  float* tw = smem;
  float* th = tw + 2 * a.d.W * a.d.my;
  float* pl = th + 2 * a.d.H * a.d.mx;
  float* T = pl + a.d.H * (a.d.W + 1);
  if constexpr (DFT) dft_twiddles(a.d, tw);
  const int row = blockIdx.x, c = row % a.C, b = row / a.C;
  const long long base = (long long)row * a.P;
  const double n = (double)a.C * a.P;
  constexpr bool al = AL;
  if (!a.norm) {
    for (int p = threadIdx.x * 4; p < a.P; p += 1024) {
      const f32x4 g4 = fno_ld4(a.gt + base, p, a.P, al);
      if (a.gv) fno_st4(a.gv + base, p, a.P, al, g4);
      if constexpr (DFT) gn_to_plane(pl, a.d.W, p, a.P, g4);
    }
  } else {
    double s1 = 0.0, s2 = 0.0;
    for (int cc = threadIdx.x; cc < a.C; cc += 256) {
      const double gm = (double)a.gamma[cc];
      s1 += gm * (double)a.rows[((long long)b * a.C + cc) * 4 + 0];
      s2 += gm * (double)a.rows[((long long)b * a.C + cc) * 4 + 1];
    }
    fno_block_sum_d2(s1, s2, red);
    const float m1 = (float)(s1 / n), m2 = (float)(s2 / n);
    const float mean = a.stats[2 * b], rstd = a.stats[2 * b + 1];
    const float sb = a.sbias ? a.sbias[c] : 0.f, gm = a.gamma[c];
    for (int p = threadIdx.x * 4; p < a.P; p += 1024) {
      const f32x4 g4 = fno_ld4(a.gt + base, p, a.P, al);
      const f32x4 xh = (fno_ld4(a.v + base, p, a.P, al) + sb - mean) * rstd;
      const f32x4 gv4 = (g4 * gm - m1 - xh * m2) * rstd;
      if (a.gv) fno_st4(a.gv + base, p, a.P, al, gv4);
      if constexpr (DFT) gn_to_plane(pl, a.d.W, p, a.P, gv4);
    }
  }
  if constexpr (DFT) {  // dL/dv only feeds the spectral branch's transform: its kept modes (output rows) straight from LDS
    __syncthreads();
    dft_fwd_stages(a.d, tw, th, pl, T, a.d.dst + (long long)row * a.d.mx * a.d.my * 2);
  }
  if (b != 0) return;
  // parameter gradients of channel c (uniform branch: the whole workgroup)
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  double dg = 0.0, db = 0.0, dsb = 0.0;  // valid in the group leaders (l16 == 0)
  for (int b0 = 0; b0 < a.B; b0 += 16) {
    const int bb = b0 + grp;
    double s1 = 0.0, s2 = 0.0;
    if (a.norm && bb < a.B)
      for (int cc = l16; cc < a.C; cc += 16) {
        const double gm = (double)a.gamma[cc];
        s1 += gm * (double)a.rows[((long long)bb * a.C + cc) * 4 + 0];
        s2 += gm * (double)a.rows[((long long)bb * a.C + cc) * 4 + 1];
      }
    __syncthreads();
    red[threadIdx.x] = s1;
    red[256 + threadIdx.x] = s2;
    __syncthreads();
    for (int w = 8; w > 0; w >>= 1) {  // over the 16 threads of a sample
      if (l16 < w) {
        red[threadIdx.x] += red[threadIdx.x + w];
        red[256 + threadIdx.x] += red[256 + threadIdx.x + w];
      }
      __syncthreads();
    }
    if (l16 == 0 && bb < a.B) {
      const double r1 = a.rows[((long long)bb * a.C + c) * 4 + 0], r2 = a.rows[((long long)bb * a.C + c) * 4 + 1],
                   r3 = a.rows[((long long)bb * a.C + c) * 4 + 2];
      dg += r2;
      db += r1;
      if (a.norm) {
        const double rstd = a.stats[2 * bb + 1], m1 = red[threadIdx.x] / n, m2 = red[256 + threadIdx.x] / n;
        dsb += rstd * ((double)a.gamma[c] * r1 - (double)a.P * m1 - r3 * m2);
      } else {
        dsb += r1;
      }
    }
  }
  __syncthreads();
  if (l16 == 0) {
    red[grp] = dg;
    red[16 + grp] = db;
    red[32 + grp] = dsb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < 16; ++k) {
      t0 += red[k];
      t1 += red[16 + k];
      t2 += red[32 + k];
    }
    if (a.ggamma) a.ggamma[c] = (float)t0;
    if (a.gbeta) a.gbeta[c] = (float)t1;
    if (a.gsbias) a.gsbias[c] = (float)t2;
  }
}

static int gn_check(int B, int C, int P) {
  if (B < 1 || C < 1 || P < 1) {
    ppsci_set_error("fno block tail: invalid shape");
    return PPSCI_E_INVALID;
  }
  return PPSCI_OK;
}

// rows: [B*C*4] floats of scratch; stats: [4*B] floats (mean, rstd per sample; the backward appends two more per sample)
static int gn_dft_args(DftArgs* d, int P, int H, int W, int mx, int my, int rows, float* dst, long long* lds) {
  if (H * W != P || !ppsci_dft2_kept_supported(H, W, mx, my)) {
    ppsci_set_error("fno block tail: the kept-mode transform does not take %d x %d planes with %d x %d modes", H, W, mx, my);
    return PPSCI_E_UNSUPPORTED;
  }
  memset(d, 0, sizeof(*d));
  d->tab = ppsci_dft_table(H, W, mx, my, rows);
  if (!d->tab) {
    ppsci_set_error("fno block tail: cannot build the twiddle table");
    return PPSCI_E_LAUNCH;
  }
  d->dst = dst, d->H = H, d->W = W, d->mx = mx, d->my = my, d->c0 = (H - mx) / 2, d->rows = rows;
  *lds = 4LL * dft_fwd_lds_floats(H, W, mx, my);
  return PPSCI_OK;
}

static int fno_tail_fwd_run(int B, int C, int P, int norm, int gelu, float eps, const float* v, const float* sbias,
                            const float* gamma, const float* beta, const float* skip, float* rows, float* stats, float* t,
                            float* y, int have_rows, int H, int W, int mx, int my, float* X_next, void* stream);

extern "C" int ppsci_fno_tail_fwd(int B, int C, int P, int norm, int gelu, float eps, const float* v, const float* sbias,
                                  const float* gamma, const float* beta, const float* skip, float* rows, float* stats,
                                  float* t, float* y, void* stream) {
  return fno_tail_fwd_run(B, C, P, norm, gelu, eps, v, sbias, gamma, beta, skip, rows, stats, t, y, 0, 0, 0, 0, 0, nullptr, stream);
}

// ppsci_fno_tail_fwd with: have_rows != 0 -- `rows` already holds the row statistics of v + sbias (ppsci_dft2_kept_inv_stats wrote
// them): no statistics pass;  X_next != NULL -- the apply kernel also emits the kept modes (input rows) of y, the next
// block's input ([B*C, modes_x, modes_y, 2]; H * W == P, ppsci_dft2_kept_supported): no transform launch reads y back.
extern "C" int ppsci_fno_tail_fwd_ex(int B, int C, int P, int norm, int gelu, float eps, const float* v, const float* sbias,
                                     const float* gamma, const float* beta, const float* skip, float* rows, float* stats,
                                     float* t, float* y, int have_rows, int H, int W, int modes_x, int modes_y, float* X_next,
                                     void* stream) {
  return fno_tail_fwd_run(B, C, P, norm, gelu, eps, v, sbias, gamma, beta, skip, rows, stats, t, y, have_rows, H, W, modes_x,
                          modes_y, X_next, stream);
}

static int fno_tail_fwd_run(int B, int C, int P, int norm, int gelu, float eps, const float* v, const float* sbias,
                            const float* gamma, const float* beta, const float* skip, float* rows, float* stats, float* t,
                            float* y, int have_rows, int H, int W, int mx, int my, float* X_next, void* stream) {
  if (gn_check(B, C, P) != PPSCI_OK || !v || !t || !rows || !stats || (norm && (!gamma || !beta)) || (X_next && !y)) {
    ppsci_set_error("fno_tail_fwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  GnArgs a;
  memset(&a, 0, sizeof(a));
  long long lds = 0;
  if (X_next) {
    int rc = gn_dft_args(&a.d, P, H, W, mx, my, 0, X_next, &lds);
    if (rc != PPSCI_OK) return rc;
  }
  const DftArgs dsave = a.d;
  a.v = v, a.sbias = sbias, a.gamma = gamma, a.beta = beta, a.skip = skip, a.rows = rows, a.stats = stats, a.t = t, a.y = y;
  a.B = B, a.C = C, a.P = P, a.norm = norm, a.gelu = gelu, a.eps = eps;
  a.d = dsave;
  // (16-byte accesses when every row starts on a 16-byte boundary; element accesses otherwise)
  const bool aligned = (P & 3) == 0 && ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(skip) |
                                         reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const bool stats_pass = norm && !have_rows;
  int se = 0;
#define GN_FWD(AL)                                                                                       \
  do {                                                                                                   \
    if (stats_pass) PPSCI_LAUNCH(gn_rowstats_kernel<AL>, GnArgs, B * C, 256, 0, stream, a);              \
    if (X_next) {                                                                                        \
      se = PPSCI_SET_MAX_LDS((gn_apply_kernel<AL, true>), (int)lds);                                     \
      if (se == 0) PPSCI_LAUNCH((gn_apply_kernel<AL, true>), GnArgs, B * C, 256, (int)lds, stream, a);   \
    } else {                                                                                             \
      PPSCI_LAUNCH((gn_apply_kernel<AL, false>), GnArgs, B * C, 256, 0, stream, a);                      \
    }                                                                                                    \
  } while (0)
  if (aligned) GN_FWD(true);
  else GN_FWD(false);
#undef GN_FWD
  if (se != 0) {
    ppsci_set_error("fno_tail_fwd: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("fno_tail_fwd: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// ggamma / gbeta / gsbias: [C] each (null to skip); gt: dL/dt (= gradient of the skip branch); gv: dL/dv
static int fno_tail_bwd_run(int B, int C, int P, int norm, int gelu, const float* v, const float* sbias, const float* gamma,
                            const float* t, const float* gout, const float* gout2, float* rows, float* stats, float* gt,
                            float* gv, float* ggamma, float* gbeta, float* gsbias, int H, int W, int mx, int my, float* ghat,
                            const float* gout2_modes, void* stream);

extern "C" int ppsci_fno_tail_bwd(int B, int C, int P, int norm, int gelu, const float* v, const float* sbias,
                                  const float* gamma, const float* t, const float* gout, const float* gout2, float* rows,
                                  float* stats, float* gt, float* gv, float* ggamma, float* gbeta, float* gsbias,
                                  void* stream) {
  return fno_tail_bwd_run(B, C, P, norm, gelu, v, sbias, gamma, t, gout, gout2, rows, stats, gt, gv, ggamma, gbeta, gsbias, 0, 0,
                          0, 0, nullptr, nullptr, stream);
}

// ppsci_fno_tail_bwd with ghat != NULL: the second pass also emits the kept modes (OUTPUT rows) of gv = dL/dv, which is what
// the spectral branch's backward transforms first ([B*C, modes_x, modes_y, 2]); gv itself may then be NULL (never stored).
// gout2_modes != NULL (then gout2 must be NULL): the second addend of dL/dy as kept modes (INPUT rows; unscaled, as
// ppsci_dft2_kept_inv takes them) -- the first pass evaluates its inverse transform per plane in LDS.
extern "C" int ppsci_fno_tail_bwd_ex(int B, int C, int P, int norm, int gelu, const float* v, const float* sbias,
                                     const float* gamma, const float* t, const float* gout, const float* gout2, float* rows,
                                     float* stats, float* gt, float* gv, float* ggamma, float* gbeta, float* gsbias, int H,
                                     int W, int modes_x, int modes_y, float* ghat, const float* gout2_modes, void* stream) {
  return fno_tail_bwd_run(B, C, P, norm, gelu, v, sbias, gamma, t, gout, gout2, rows, stats, gt, gv, ggamma, gbeta, gsbias, H, W,
                          modes_x, modes_y, ghat, gout2_modes, stream);
}

static int fno_tail_bwd_run(int B, int C, int P, int norm, int gelu, const float* v, const float* sbias, const float* gamma,
                            const float* t, const float* gout, const float* gout2, float* rows, float* stats, float* gt,
                            float* gv, float* ggamma, float* gbeta, float* gsbias, int H, int W, int mx, int my, float* ghat,
                            const float* gout2_modes, void* stream) {
  if (gn_check(B, C, P) != PPSCI_OK || !v || !gout || !rows || !stats || !gt || (!gv && !ghat) || (gelu && !t) ||
      (norm && !gamma) || (gout2 && gout2_modes)) {
    ppsci_set_error("fno_tail_bwd: invalid argument");
    return PPSCI_E_INVALID;
  }
  GnArgs a;
  memset(&a, 0, sizeof(a));
  long long lds = 0;
  if (ghat) {
    int rc = gn_dft_args(&a.d, P, H, W, mx, my, 1, ghat, &lds);
    if (rc != PPSCI_OK) return rc;
  }
  long long lds_i = 0;
  if (gout2_modes) {
    int rc = gn_dft_args(&a.di, P, H, W, mx, my, 0, nullptr, &lds_i);
    if (rc != PPSCI_OK) return rc;
    a.di.src = gout2_modes;
    lds_i = 4LL * (dft_inv_lds_floats(H, W, mx, my) + (long long)H * W);
  }
  const DftArgs di_save = a.di;
  a.v = v, a.sbias = sbias, a.gamma = gamma, a.t = (float*)t, a.gout = gout, a.gout2 = gout2, a.rows = rows, a.stats = stats;
  a.gt = gt, a.gv = gv, a.ggamma = ggamma, a.gbeta = gbeta, a.gsbias = gsbias;
  a.B = B, a.C = C, a.P = P, a.norm = norm, a.gelu = gelu;
  a.di = di_save;
  const bool aligned = (P & 3) == 0 && ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(gout) |
                                         reinterpret_cast<uintptr_t>(gout2) | reinterpret_cast<uintptr_t>(gt) |
                                         reinterpret_cast<uintptr_t>(gv)) & 15) == 0;
  int se = 0;
#define GN_BWD(AL)                                                                                           \
  do {                                                                                                       \
    if (gout2_modes) {                                                                                       \
      se = PPSCI_SET_MAX_LDS((gn_bwd_rows_kernel<AL, true>), (int)lds_i);                                    \
      if (se == 0) PPSCI_LAUNCH((gn_bwd_rows_kernel<AL, true>), GnArgs, B * C, 256, (int)lds_i, stream, a);  \
    } else {                                                                                                 \
      PPSCI_LAUNCH((gn_bwd_rows_kernel<AL, false>), GnArgs, B * C, 256, 0, stream, a);                       \
    }                                                                                                        \
    if (se != 0) break;                                                                                      \
    if (ghat) {                                                                                              \
      se = PPSCI_SET_MAX_LDS((gn_bwd_apply_kernel<AL, true>), (int)lds);                                     \
      if (se == 0) PPSCI_LAUNCH((gn_bwd_apply_kernel<AL, true>), GnArgs, B * C, 256, (int)lds, stream, a);   \
    } else {                                                                                                 \
      PPSCI_LAUNCH((gn_bwd_apply_kernel<AL, false>), GnArgs, B * C, 256, 0, stream, a);                      \
    }                                                                                                        \
  } while (0)
  if (aligned) GN_BWD(true);
  else GN_BWD(false);
#undef GN_BWD
  if (se != 0) {
    ppsci_set_error("fno_tail_bwd: cannot raise dynamic LDS to %lld B", lds);
    return PPSCI_E_LAUNCH;
  }
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("fno_tail_bwd: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}


// ------------------------------------------------------------------------------------------ DomainPadding
// ------------------------------------------------------------------------------------------ projection MLP, hidden gradient
// The projection MLP ends in a convolution to out_channels = 1 (Darcy; <= 4 here): the gradient of its hidden pre-activation,
//   gz2[c][p] = GELU'(z2[c][p]) * sum_j W2[j][c] gy[j][p],
// is an elementwise product with a rank-m factor, not a GEMM.  ppsci_pw_conv (transpose, GELU' epilogue) spent 31 us on it -- a
// K = 1 contraction through the MFMA tiles -- for 17 MB read + 17 MB written; this kernel streams it.
struct ProjGArgs {
  const float *z2, *W2, *gy;
  float* out;
  int B, C, m, P;
};
__global__ void __launch_bounds__(256) proj_hidden_grad_kernel(ProjGArgs a) {
  const long long q4 = (long long)a.P / 4, total = (long long)a.B * a.C * q4;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / q4;  // b * C + c
    const int p = (int)(idx - row * q4) * 4;
    const int b = (int)(row / a.C), c = (int)(row - (long long)b * a.C);
    const f32x4 z = *(const f32x4*)&a.z2[row * a.P + p];
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.m; ++j) g += *(const f32x4*)&a.gy[((long long)b * a.m + j) * a.P + p] * a.W2[(long long)j * a.C + c];
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = g[t] * fno_gelu_grad(z[t]);
    *(f32x4*)&a.out[row * a.P + p] = o;
  }
}

extern "C" int ppsci_fno_proj_hidden_grad(int B, int C, int m, int P, const float* z2, const float* W2, const float* gy, float* out,
                                          void* stream) {
  if (B < 1 || C < 1 || m < 1 || P < 1 || !z2 || !W2 || !gy || !out) {
    ppsci_set_error("fno_proj_hidden_grad: invalid argument");
    return PPSCI_E_INVALID;
  }
  if (m > 4 || (P & 3) != 0 || ((reinterpret_cast<uintptr_t>(z2) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(out)) & 15) != 0) {
    ppsci_set_error("fno_proj_hidden_grad: built for <= 4 output channels and 16-byte aligned rows (m = %d, P = %d)", m, P);
    return PPSCI_E_UNSUPPORTED;
  }
  ProjGArgs a{z2, W2, gy, out, B, C, m, P};
  const long long total = (long long)B * C * (P / 4);
  long long grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  PPSCI_LAUNCH(proj_hidden_grad_kernel, ProjGArgs, (int)grid, 256, 0, stream, a);
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("fno_proj_hidden_grad: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// ------------------------------------------------------------------------------------------ lifting MLP, first layer, backward
// The lifting MLP of FNONet (/root/reference/ppsci/arch/fno_block.py MLP(in -> lifting_channels -> hidden), tfnonet.py:95-110):
//   a1 = GELU(z1),  z1 = W0 x0 + b0  (K0 <= 4 input channels, C1 = 256 lifting channels),   x_lift = W1 a1 + b1.
// Its first layer's weight gradient needs  gz1[c][p] = GELU'(z1[c][p]) * sum_k W1[k][c] gx[k][p]  -- a [B, 256, P] tensor,
// 8 x a block tensor (67 MB at batch 16, 64 x 64), which up to round 5 one launch wrote (ppsci_pw_conv_v, transpose, virtual
// GELU') and the next read back (ppsci_pw_conv_wgrad_v): 37 + 30 us of a 0.65 ms TFNO step.  This kernel forms gz1 in
// registers and reduces it against the K0 input channels at once:
//   part[chunk][c * K0 + i] = sum_{p in chunk} gz1[c][p] x0[i][p],     part_b[chunk][c] = sum_{p in chunk} gz1[c][p]
// with the chunks (256 pixels of one sample) and the row layout of ppsci_pw_conv_wgrad, so the same fixed-order row
// reduction finishes it.  One workgroup of 16 waves per chunk and 256 channels; the gradient tile gx[:, chunk] is staged in LDS.
#define LIFT0_CHMAX 64
#define LIFT0_WAVES 16  // waves (blocks of 16 channels) per workgroup (8 -- two workgroups per CU -- measured slower: 34.0 against 31.6 us;
                        // the kernel is bound by the GELU' arithmetic, ~40 VALU instructions per element, as the launch it replaces was)
struct Lift0Args {
  const float *x0, *W0, *b0, *W1, *gx;
  const float* gx2;  // or null: a second addend of gx (the spectral branch's share of the first block's input gradient)
  float *part, *part_b;
  float* part1;   // or null: [chunks][ld1] rows of the SECOND layer's gradient, [Ch * C1] weights then [Ch] biases
  long long ldp, ldpb, ld1;
  int B, K0, C1, Ch, P, cpix, chunks_per_b;
};
template <int NS>  // K = 4 steps of the contraction: hidden width <= 4 NS
__global__ void __launch_bounds__(64 * LIFT0_WAVES) lift0_wgrad_kernel(Lift0Args a) {
  // wave w of the 16: channels [16 w, 16 w + 16) of this workgroup's 256; the hidden gradient's first factor
  //   G[c][p] = sum_k W1[k][c] gx[k][p]   as 16 x 16 tiles on the fp32 MFMA (K = 4 per instruction: A[i = c16][k = g] = W1[4 s + g][c],
  //   B[k = g][n = c16] = gx[4 s + g][p]; D: lane (g, c16) holds channels 4 g + r of pixel c16),
  // then per element GELU'(z1), the products with the K0 inputs, sums over the chunk's pixels per lane and, at the end, over the 16
  // lanes of a group (fixed butterfly).  (A first version did the contraction on the VALU with one thread per channel and the tile
  // read as LDS broadcasts: 58 us, LDS- and VALU-bound; the launches it replaces took 37 + 30 us.)
  PPSCI_DYN_SMEM(smem);
  const int LD = a.cpix + 17;                     // row stride of the k-major tile (odd: rows k, k + 1 start one bank apart)
  float* gxs = smem;                              // [4 NS][LD], rows >= Ch zero
  float* xs = gxs + 4 * NS * LD;                  // [4][cpix]
  float* a1s = xs + 4 * a.cpix;                   // [waves][2 tiles][16 channels][17]: GELU(z1) of a tile, wave-private
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  constexpr int CB = 16 * LIFT0_WAVES;          // channels per workgroup (grid = chunks x channel blocks)
  const int ncb = (a.C1 + CB - 1) / CB;
  const int chunk = (int)blockIdx.x / ncb, cb = (int)blockIdx.x - chunk * ncb;
  const int b = chunk / a.chunks_per_b, p0 = (chunk - b * a.chunks_per_b) * a.cpix;
  const int cp = a.P - p0 < a.cpix ? a.P - p0 : a.cpix;
  const int cbase = cb * CB + wave * 16;
  const int ca = cbase + c16;                     // the channel whose W1 column this lane feeds into A
  float af[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) af[s] = (ca < a.C1 && 4 * s + g < a.Ch) ? a.W1[(long long)(4 * s + g) * a.C1 + ca] : 0.f;
  float w0[4][4], b0v[4];                         // of the four channels this lane holds in D
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = cbase + 4 * g + r;
    b0v[r] = (c < a.C1 && a.b0 != nullptr) ? a.b0[c] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) w0[r][i] = (c < a.C1 && i < a.K0) ? a.W0[(long long)c * a.K0 + i] : 0.f;
  }
  for (int idx = tid; idx < 4 * NS * LD; idx += 64 * LIFT0_WAVES) {  // (the rows' padding as well: the second contraction reads a
    const int k = idx / LD, p = idx - k * LD;                             //  whole 16-pixel tile behind the chunk's last pixel)
    float v = 0.f;
    if (k < a.Ch && p < cp) {
      const long long off = ((long long)b * a.Ch + k) * a.P + p0 + p;
      v = a.gx[off];
      if (a.gx2 != nullptr) v += a.gx2[off];
    }
    gxs[k * LD + p] = v;
  }
  for (int idx = tid; idx < 4 * a.cpix; idx += 64 * LIFT0_WAVES) {
    const int i = idx / a.cpix, p = idx - i * a.cpix;
    xs[i * a.cpix + p] = (i < a.K0 && p < cp) ? a.x0[((long long)b * a.K0 + i) * a.P + p0 + p] : 0.f;
  }
  __syncthreads();
  float ab[4] = {0.f, 0.f, 0.f, 0.f}, aw[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) aw[r][i] = 0.f;
  // second layer's weight gradient (a.part1): O[c][k] = sum_p GELU(z1[c][p]) gx[k][p] for the wave's 16 channels, NS / 4 blocks
  // of 16 k; on the MFMA with A[i = c][kk = pixel] (from the wave's scratch, transposed on the way) and B[kk = pixel][n = k]
  constexpr int KB = NS / 4;
  const bool second = a.part1 != nullptr;
  f32x4 O[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) O[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float* const sc0 = a1s + (wave * 2 + 0) * (16 * 17);
  float* const sc1 = a1s + (wave * 2 + 1) * (16 * 17);
  // Two pixel tiles per iteration: their B operands are requested first (2 x Ch / 4 independent LDS reads), then two independent
  // MFMA chains run interleaved, then the pointwise part of both.  (Columns of pixels beyond the chunk take row 0 of the tile and
  // are dropped at `gz`.  A software pipeline -- the next tile's MFMAs in front of this tile's pointwise part -- measured slower:
  // 34.6 against 31.9 us.)
  for (int pt = 0; pt * 16 < cp; pt += 2) {
    const int px0 = pt * 16 + c16, px1 = px0 + 16;
    const bool v0 = px0 < cp, v1 = px1 < cp;
    const int q0 = v0 ? px0 : 0, q1 = v1 ? px1 : 0;
    float bv0[NS], bv1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
    {
      bv0[s] = gxs[(4 * s + g) * LD + q0];  // (rows Ch .. 4 NS - 1 of the tile are zeros, and so are their A values)
      bv1[s] = gxs[(4 * s + g) * LD + q1];
    }
    float xv0[4], xv1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xv0[i] = xs[i * a.cpix + q0], xv1[i] = xs[i * a.cpix + q1];
    f32x4 D0 = {0.f, 0.f, 0.f, 0.f}, D1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
    {
      D0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], bv0[s], D0, 0, 0, 0);
      D1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], bv1[s], D1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z0 = b0v[r] + w0[r][0] * xv0[0] + w0[r][1] * xv0[1] + w0[r][2] * xv0[2] + w0[r][3] * xv0[3];
      const float z1 = b0v[r] + w0[r][0] * xv1[0] + w0[r][1] * xv1[1] + w0[r][2] * xv1[2] + w0[r][3] * xv1[3];
      float c0, s0, c1, s1;
      fno_gelu_parts(z0, c0, s0);
      fno_gelu_parts(z1, c1, s1);
      const float gz0 = v0 ? D0[r] * (c0 + z0 * 0.3989422804014327f * s0) : 0.f;  // (fno_gelu_grad)
      const float gz1 = v1 ? D1[r] * (c1 + z1 * 0.3989422804014327f * s1) : 0.f;
      if (second) {  // GELU(z1) of the two tiles, [channel][pixel] in the wave's scratch
        sc0[(4 * g + r) * 17 + c16] = v0 ? z0 * c0 : 0.f;
        sc1[(4 * g + r) * 17 + c16] = v1 ? z1 * c1 : 0.f;
      }
      ab[r] += gz0;
      ab[r] += gz1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        aw[r][i] += gz0 * xv0[i];
        aw[r][i] += gz1 * xv1[i];
      }
    }
    if (second) {
      ppsci_wave_sync();  // the scratch is complete (written and read by this wave only)
#pragma unroll
      for (int st = 0; st < 4; ++st) {  // K = 4 pixels per step, both tiles
        const float a0 = sc0[c16 * 17 + 4 * st + g], a1v = sc1[c16 * 17 + 4 * st + g];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
          const float b0 = gxs[(16 * kb + c16) * LD + pt * 16 + 4 * st + g];
          const float b1 = gxs[(16 * kb + c16) * LD + pt * 16 + 16 + 4 * st + g];  // (the row's padding / zeros beyond the chunk)
          O[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, O[kb], 0, 0, 0);
          O[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v, b1, O[kb], 0, 0, 0);
        }
      }
      ppsci_wave_sync();  // (the next iteration rewrites the scratch)
    }
  }
  // sums over the 16 pixel lanes of each group: DPP row shifts (the total lands in the group's last lane; 80 ds_bpermute through
  // the LDS crossbar -- shared by the 16 waves -- took their place before)
#define LIFT0_ROWSUM(v)                                                                                                   \
  do {                                                                                                                    \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));   \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));   \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));   \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));   \
  } while (0)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    LIFT0_ROWSUM(ab[r]);
#pragma unroll
    for (int i = 0; i < 4; ++i) LIFT0_ROWSUM(aw[r][i]);
  }
#undef LIFT0_ROWSUM
  if (c16 == 15) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = cbase + 4 * g + r;
      if (c < a.C1) {
        for (int i = 0; i < a.K0; ++i) a.part[(long long)chunk * a.ldp + (long long)c * a.K0 + i] = aw[r][i];
        if (a.part_b != nullptr) a.part_b[(long long)chunk * a.ldpb + c] = ab[r];
      }
    }
  }
  if (second) {
    // O: lane (g, c16) holds channels cbase + 4 g + r (rows), k = 16 kb + c16 (column); weight layout [Ch][C1]
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int k = 16 * kb + c16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = cbase + 4 * g + r;
        if (k < a.Ch && c < a.C1) a.part1[(long long)chunk * a.ld1 + (long long)k * a.C1 + c] = O[kb][r];
      }
    }
    if (cb == 0 && tid < a.Ch) {  // the second layer's bias gradient: sum of gx over the chunk's pixels (in pixel order)
      float sb = 0.f;
      for (int p = 0; p < cp; ++p) sb += gxs[tid * LD + p];
      a.part1[(long long)chunk * a.ld1 + (long long)a.Ch * a.C1 + tid] = sb;
    }
  }
}

// Pixels of one sample per workgroup.  A workgroup walks its chunk two 16-pixel tiles at a time (a chain of MFMA + pointwise + MFMA
// per pair), so the launch takes as long as ONE chunk however many there are: 45 us with 256-pixel chunks for 65 536 pixels (256
// workgroups) and 41 us for 8 192 pixels (32 workgroups, an eighth of the chip).  Small problems therefore take shorter chunks -- the
// largest of 256 / 128 / 64 pixels that still gives 128 workgroups, 64 otherwise -- at the price of more partial rows for the one
// reduction launch at the end of the backward pass; at 256 workgroups and more the 256-pixel chunk stays (measured on MI355X:
// 128-pixel chunks at the TFNO shape 0.539 vs 0.533 ms per step, at the SFNO shape 0.522 vs 0.536).
static int lift0_cpix(int B, int P) {
  for (int c = 256; c > 64; c >>= 1)
    if (P >= c && (long long)B * ((P + c - 1) / c) >= 128) return c;
  return P >= 64 ? 64 : P;
}
extern "C" int64_t ppsci_fno_lift0_wgrad_chunks(int B, int P) {
  const int cpix = lift0_cpix(B, P);
  return (int64_t)B * ((P + cpix - 1) / cpix);
}

extern "C" int ppsci_fno_lift0_wgrad(int B, int K0, int C1, int Ch, int P, const float* x0, const float* W0, const float* b0,
                                     const float* W1, const float* gx, const float* gx2, float* partials, float* partials_b,
                                     int64_t ld_partials, float* partials1, int64_t ld_partials1, void* stream) {
  if (B < 1 || K0 < 1 || C1 < 1 || Ch < 1 || P < 1 || !x0 || !W0 || !W1 || !gx || !partials) {
    ppsci_set_error("fno_lift0_wgrad: invalid argument");
    return PPSCI_E_INVALID;
  }
  if (K0 > 4 || Ch > LIFT0_CHMAX || (Ch & 3) != 0) {
    ppsci_set_error("fno_lift0_wgrad: built for <= 4 input channels and a hidden width that is a multiple of 4, <= %d (K0 = %d, Ch = %d)",
                    LIFT0_CHMAX, K0, Ch);
    return PPSCI_E_UNSUPPORTED;
  }
  if (ld_partials != 0 && ld_partials < (int64_t)C1 * K0) {
    ppsci_set_error("fno_lift0_wgrad: ld_partials smaller than a row");
    return PPSCI_E_INVALID;
  }
  if (partials1 != nullptr && (Ch > 32 || ld_partials1 < (int64_t)Ch * C1 + Ch)) {
    ppsci_set_error("fno_lift0_wgrad: the second layer's gradient is built for a hidden width <= 32 and rows of Ch * C1 + Ch floats");
    return PPSCI_E_UNSUPPORTED;
  }
  Lift0Args a;
  a.x0 = x0, a.W0 = W0, a.b0 = b0, a.W1 = W1, a.gx = gx, a.gx2 = gx2, a.part = partials, a.part_b = partials_b;
  a.part1 = partials1, a.ld1 = ld_partials1;
  a.ldp = ld_partials ? ld_partials : (long long)C1 * K0;
  a.ldpb = ld_partials ? ld_partials : C1;
  a.B = B, a.K0 = K0, a.C1 = C1, a.Ch = Ch, a.P = P;
  a.cpix = lift0_cpix(B, P);
  a.chunks_per_b = (P + a.cpix - 1) / a.cpix;
  const int lds = ((Ch <= 32 ? 32 : 64) * (a.cpix + 17) + 4 * a.cpix + LIFT0_WAVES * 2 * 16 * 17) * 4;
  const int grid = B * a.chunks_per_b * ((C1 + 16 * LIFT0_WAVES - 1) / (16 * LIFT0_WAVES));
  if (Ch <= 32) {
    if (PPSCI_SET_MAX_LDS(lift0_wgrad_kernel<8>, lds) != 0) {
      ppsci_set_error("fno_lift0_wgrad: cannot raise dynamic LDS to %d B", lds);
      return PPSCI_E_LAUNCH;
    }
    PPSCI_LAUNCH(lift0_wgrad_kernel<8>, Lift0Args, grid, 64 * LIFT0_WAVES, lds, stream, a);
  } else {
    if (PPSCI_SET_MAX_LDS(lift0_wgrad_kernel<16>, lds) != 0) {
      ppsci_set_error("fno_lift0_wgrad: cannot raise dynamic LDS to %d B", lds);
      return PPSCI_E_LAUNCH;
    }
    PPSCI_LAUNCH(lift0_wgrad_kernel<16>, Lift0Args, grid, 64 * LIFT0_WAVES, lds, stream, a);
  }
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("fno_lift0_wgrad: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// fno_block.DomainPadding (/root/reference/ppsci/arch/fno_block.py:19-140): zero rows / columns around every [H, W] plane
// between the lifting layer and the FNO blocks, removed again in front of the projection.  unpad == 0: dst [n, hp, wp] =
// src [n, h, w] placed at (oh, ow), zero elsewhere; unpad == 1: dst [n, h, w] = src [n, hp, wp] window at (oh, ow).
// The backward of one is the other.
struct PadArgs {
  const float* src;
  float* dst;
  int n, h, w, hp, wp, oh, ow, unpad;
};
__global__ void __launch_bounds__(256) pad2d_kernel(PadArgs a) {
  const long long total = a.unpad ? (long long)a.n * a.h * a.w : (long long)a.n * a.hp * a.wp;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    if (a.unpad) {
      const int j = (int)(idx % a.w), i = (int)((idx / a.w) % a.h);
      const long long pl = idx / ((long long)a.w * a.h);
      a.dst[idx] = a.src[(pl * a.hp + i + a.oh) * a.wp + j + a.ow];
    } else {
      const int j = (int)(idx % a.wp), i = (int)((idx / a.wp) % a.hp);
      const long long pl = idx / ((long long)a.wp * a.hp);
      const int ii = i - a.oh, jj = j - a.ow;
      a.dst[idx] = (ii >= 0 && ii < a.h && jj >= 0 && jj < a.w) ? a.src[(pl * a.h + ii) * a.w + jj] : 0.f;
    }
  }
}
extern "C" int ppsci_pad2d(int n, int h, int w, int hp, int wp, int oh, int ow, int unpad, const float* src, float* dst,
                           void* stream) {
  if (n < 1 || h < 1 || w < 1 || hp < h + oh || wp < w + ow || oh < 0 || ow < 0 || !src || !dst) {
    ppsci_set_error("pad2d: invalid argument");
    return PPSCI_E_INVALID;
  }
  PadArgs a{src, dst, n, h, w, hp, wp, oh, ow, unpad};
  const long long total = unpad ? (long long)n * h * w : (long long)n * hp * wp;
  long long grid = (total + 255) / 256;
  if (grid > 4096) grid = 4096;
  PPSCI_LAUNCH(pad2d_kernel, PadArgs, (int)grid, 256, 0, stream, a);
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("pad2d: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}
