// grad_surgery.inc -- per-loss gradient matrix kernels of the PCGrad / Relobralo loss aggregators; included from
// epilogue_optim.hip (behind AdamArgs / ppsci_adam_one / ppsci_set_error).
//
// PCGrad (/root/reference/ppsci/loss/mtl/pcgrad.py:62-120) projects every per-loss gradient g_i against every ORIGINAL
// g_k, k in a shuffled order:  g_i <- g_i - min(<g_i, g_k> / <g_k, g_k>, 0) g_k,  and sums the results.  Every projected
// g_i stays in span{g_k}, so the rule lives in Gram space: with g_i = sum_m C[i][m] g_m (C = I at the start),
//   <g_i, g_k> = sum_m C[i][m] Gram[m][k],   C[i][k] -= min(that / Gram[k][k], 0),   result = sum_m w_m g_m,  w_m = sum_i C[i][m].
// The flat vectors are read twice: once for the Gram matrix (grad_surgery_kernel, which also runs the K x K rule on one thread
// of its last workgroup) and once for the weighted combination (grad_combine_kernel, with the Adam update behind it).
//
// Deviation from the reference, on purpose: a loss whose gradient is exactly zero (Gram[k][k] == 0) is skipped as a projection
// target; the reference divides by it and every gradient becomes NaN.
//
// Determinism: no float atomics.  Gram[a][b] is summed in a fixed shape that depends on (n, vec) only:
//   thread: a serial fmaf chain over its S elements; with `per` columns per workgroup S <= 4 ceil(per / 1024) + 1 (four columns
//           per trip of the float4 loop + at most one of the scalar tail; the scalar loop alone takes ceil(per / 256), which is
//           no more) -- 9 while n <= GS_CHUNK * GS_MAX_GRID;
//   wave: 6 butterfly levels;  workgroup: its 4 waves in order (3 additions);
//   grid: ONE partial per thread of the last workgroup (grid <= GS_MAX_GRID = GS_BLOCK), 6 butterfly levels, 4 waves in order.
// Depth d = S + 6 + 3 + 6 + 3 = S + 18 roundings per term, so  |Gram - exact| <= (S + 18) u sum_j |a_j b_j| (1 + O(u)),
// u = 2^-24.  The tests bound it with  c = S + 18  and eps32 = 2^-23 (a factor 2 of slack over the first-order bound).
#define GS_BLOCK 256
#define GS_CHUNK 2048     // columns per workgroup the launch rule aims at
#define GS_MAX_GRID 256   // == GS_BLOCK: the last workgroup reads one partial row per thread
#define GS_WS_HEADER 64   // bytes in front of the partial rows: the ticket counter (kept zero between calls)

struct GradSurgeryArgs {
  const float* G;
  long long n, ld, per;  // per: columns per workgroup (a multiple of 4)
  int mode, vec;
  unsigned order;        // order[s] in bits 4s .. 4s+3
  float *gram, *coef, *w, *partials;
  unsigned* counter;
};

static int gs_grid(long long n) {
  const long long g = (n + GS_CHUNK - 1) / GS_CHUNK;
  return (int)(g < 1 ? 1 : (g > GS_MAX_GRID ? GS_MAX_GRID : g));
}

template <int K>
__device__ __forceinline__ void gs_add(float (&acc)[K * (K + 1) / 2], const float (&g)[K]) {
  int p = 0;
#pragma unroll
  for (int a = 0; a < K; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b, ++p) acc[p] = __builtin_fmaf(g[a], g[b], acc[p]);
}

// LDS (floats): [0, 4 * NP) wave sums; [192, 256) Gram; [256, 320) C
#define GS_LDS_FLOATS 320
template <int K>
__global__ void __launch_bounds__(GS_BLOCK) grad_surgery_kernel(GradSurgeryArgs a) {
  PPSCI_DYN_SMEM(red);
  constexpr int NP = K * (K + 1) / 2;
  const int tid = threadIdx.x, wv = tid >> 6;
  const long long lo = (long long)blockIdx.x * a.per;
  const long long hi = lo + a.per < a.n ? lo + a.per : a.n;
  float acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.f;
  long long tail = lo;  // first column of the scalar part
  if (a.vec && hi > lo) {
    tail = lo + ((hi - lo) & ~3LL);
    for (long long j = lo + 4 * tid; j < tail; j += 4 * GS_BLOCK) {
      f32x4 r[K];
#pragma unroll
      for (int k = 0; k < K; ++k) r[k] = *(const f32x4*)(a.G + k * a.ld + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float g[K];
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = r[k][e];
        gs_add<K>(acc, g);
      }
    }
  }
  for (long long j = tail + tid; j < hi; j += GS_BLOCK) {
    float g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = a.G[k * a.ld + j];
    gs_add<K>(acc, g);
  }
  // ---- workgroup sum: butterfly, then the waves in order
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float v = acc[p];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) red[p * 4 + wv] = v;
  }
  ppsci_block_sync_lds();
  if (tid < NP) {
    float t = red[tid * 4];
    for (int w = 1; w < GS_BLOCK / 64; ++w) t += red[tid * 4 + w];
    ppsci_store_agent(&a.partials[(long long)blockIdx.x * NP + tid], t);  // another workgroup reads it in this launch
  }
  // ---- the workgroup that finishes LAST sums all rows (ticket: epilogue_vm.h epi_finale, taylor_step_tail.h); the rows were
  // written with agent-scope stores and have completed before the ticket is taken (ppsci_block_sync_mem)
  ppsci_block_sync_mem();
  if (gridDim.x > 1) {
    if (tid == 0) ((unsigned*)red)[0] = atomicAdd(a.counter, 1u);
    ppsci_block_sync_lds();
    const unsigned ticket = ((const unsigned*)red)[0];
    ppsci_block_sync_lds();
    if (ticket != gridDim.x - 1) return;
    if (tid == 0) *a.counter = 0u;  // every workgroup has taken its ticket: ready for the next call
  }
  ppsci_acquire_agent();  // the acquire half of __threadfence(): nothing stale from this CU's / XCD's caches
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float v = tid < (int)gridDim.x ? a.partials[(long long)tid * NP + p] : 0.f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) red[p * 4 + wv] = v;
  }
  ppsci_block_sync_lds();
  float* const gm = red + 192;
  float* const cm = red + 256;
  if (tid < NP) {
    float t = red[tid * 4];
    for (int w = 1; w < GS_BLOCK / 64; ++w) t += red[tid * 4 + w];
    int ra = 0;  // pair index -> (ra, rb), rb <= ra
    while ((ra + 1) * (ra + 2) / 2 <= tid) ++ra;
    const int rb = tid - ra * (ra + 1) / 2;
    gm[ra * K + rb] = t;
    gm[rb * K + ra] = t;
  }
  ppsci_block_sync_lds();
  if (tid < K * K) a.gram[tid] = gm[tid];
  if (a.mode == PPSCI_MTL_GRAM_ONLY) return;
  if (tid < K * K) cm[tid] = (tid / K == tid % K) ? 1.f : 0.f;
  ppsci_block_sync_lds();
  if (tid == 0) {
    for (int i = 0; i < K; ++i)
      for (int s = 0; s < K; ++s) {
        const int k = (int)((a.order >> (4 * s)) & 15u);
        const float gkk = gm[k * K + k];
        if (gkk == 0.f) continue;  // a zero gradient is no projection target (the reference divides by it: NaN)
        float dot = cm[i * K] * gm[k];
        for (int m = 1; m < K; ++m) dot = __builtin_fmaf(cm[i * K + m], gm[m * K + k], dot);
        const float pd = dot / gkk;
        if (pd < 0.f) cm[i * K + k] -= pd;
      }
  }
  ppsci_block_sync_lds();
  if (tid < K * K) a.coef[tid] = cm[tid];
  if (tid < K) {
    float t = cm[tid];
    for (int i = 1; i < K; ++i) t += cm[i * K + tid];
    a.w[tid] = t;
  }
}

extern "C" int64_t ppsci_grad_surgery_workspace_bytes(int K, int64_t n) {
  if (K < 1 || K > PPSCI_MTL_MAX_LOSSES || n < 1) return 0;
  return GS_WS_HEADER + (int64_t)gs_grid(n) * (K * (K + 1) / 2) * (int64_t)sizeof(float);
}

extern "C" int ppsci_grad_surgery(int K, int64_t n, const float* G, int64_t ld, const int32_t* order, int mode,
                                  float* gram_out, float* coef_out, float* w_out, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  if (K < 1 || K > PPSCI_MTL_MAX_LOSSES || n < 1 || ld < n || !G || !gram_out || !workspace ||
      (mode != PPSCI_MTL_PCGRAD && mode != PPSCI_MTL_GRAM_ONLY) ||
      (mode == PPSCI_MTL_PCGRAD && (!coef_out || !w_out || !order))) {
    ppsci_set_error("grad_surgery: invalid argument (1 <= K <= %d, ld >= n >= 1, mode, output pointers)", PPSCI_MTL_MAX_LOSSES);
    return PPSCI_E_INVALID;
  }
  if (workspace_bytes < ppsci_grad_surgery_workspace_bytes(K, n) || ((uintptr_t)workspace & 3) != 0) {
    ppsci_set_error("grad_surgery: workspace of %lld bytes, ppsci_grad_surgery_workspace_bytes asks for %lld",
                    (long long)workspace_bytes, (long long)ppsci_grad_surgery_workspace_bytes(K, n));
    return PPSCI_E_INVALID;
  }
  unsigned packed = 0, seen = 0;
  if (mode == PPSCI_MTL_PCGRAD) {
    for (int s = 0; s < K; ++s) {
      if (order[s] < 0 || order[s] >= K || (seen >> order[s] & 1u)) {
        ppsci_set_error("grad_surgery: order is not a permutation of 0 .. %d", K - 1);
        return PPSCI_E_INVALID;
      }
      seen |= 1u << order[s];
      packed |= (unsigned)order[s] << (4 * s);
    }
  }
  const int grid = gs_grid(n);
  GradSurgeryArgs a;
  a.G = G;
  a.n = n;
  a.ld = ld;
  a.per = (((n + grid - 1) / grid) + 3) & ~3LL;
  a.mode = mode;
  a.vec = (((uintptr_t)G & 15) == 0 && (ld % 4 == 0 || K == 1)) ? 1 : 0;
  a.order = packed;
  a.gram = gram_out;
  a.coef = coef_out;
  a.w = w_out;
  a.counter = (unsigned*)workspace;
  a.partials = (float*)((char*)workspace + GS_WS_HEADER);
  const size_t lds = GS_LDS_FLOATS * sizeof(float);
  switch (K) {
    case 1: PPSCI_LAUNCH(grad_surgery_kernel<1>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
    case 2: PPSCI_LAUNCH(grad_surgery_kernel<2>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
    case 3: PPSCI_LAUNCH(grad_surgery_kernel<3>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
    case 4: PPSCI_LAUNCH(grad_surgery_kernel<4>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
    case 5: PPSCI_LAUNCH(grad_surgery_kernel<5>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
    case 6: PPSCI_LAUNCH(grad_surgery_kernel<6>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
    case 7: PPSCI_LAUNCH(grad_surgery_kernel<7>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
    default: PPSCI_LAUNCH(grad_surgery_kernel<8>, GradSurgeryArgs, grid, GS_BLOCK, lds, stream, a); break;
  }
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("grad_surgery: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

// ---- out[j] = sum_k w_k G[k][j]  (k = 0 .. K-1 in order: w_0 G_0, then one fmaf per further row), optionally the Adam update
// of parameter j from it in the same launch (ppsci_adam_one: the arithmetic of ppsci_adam_step, bit for bit)
struct GradCombineArgs {
  const float* G;
  long long n, ld;
  int K, vec, do_adam;
  const float* w_dev;
  float w[PPSCI_MTL_MAX_LOSSES];
  float* out;
  AdamArgs adam;
};

__device__ __forceinline__ float gc_one(const GradCombineArgs& a, const float (&w)[PPSCI_MTL_MAX_LOSSES], long long j) {
  float s = w[0] * a.G[j];
#pragma unroll
  for (int k = 1; k < PPSCI_MTL_MAX_LOSSES; ++k)
    if (k < a.K) s = __builtin_fmaf(w[k], a.G[k * a.ld + j], s);
  return s;
}

__global__ void __launch_bounds__(256) grad_combine_kernel(GradCombineArgs a) {
  float w[PPSCI_MTL_MAX_LOSSES];
#pragma unroll
  for (int k = 0; k < PPSCI_MTL_MAX_LOSSES; ++k) w[k] = k < a.K ? (a.w_dev ? a.w_dev[k] : a.w[k]) : 0.f;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n4 = a.vec ? a.n >> 2 : 0;
  if (t < n4) {  // float4 path: every row start is 16-byte aligned
    const long long j = 4 * t;
    f32x4 s = *(const f32x4*)(a.G + j) * w[0];
#pragma unroll
    for (int k = 1; k < PPSCI_MTL_MAX_LOSSES; ++k)
      if (k < a.K) {
        const f32x4 g = *(const f32x4*)(a.G + k * a.ld + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = __builtin_fmaf(w[k], g[e], s[e]);
      }
    *(f32x4*)(a.out + j) = s;
    if (a.do_adam) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ppsci_adam_one(a.adam, j + e, s[e]);
    }
    return;
  }
  const long long j = 4 * n4 + (t - n4);  // scalar tail (or everything, without the alignment)
  if (j >= a.n) return;
  const float s = gc_one(a, w, j);
  a.out[j] = s;
  if (a.do_adam) ppsci_adam_one(a.adam, j, s);
}

extern "C" int ppsci_grad_combine(int K, int64_t n, const float* G, int64_t ld, const float* w_dev, const float* w_host,
                                  float* out, float* params, const ppsci_adam_args* adam, void* stream) {
  if (K < 1 || K > PPSCI_MTL_MAX_LOSSES || n < 1 || ld < n || !G || !out) {
    ppsci_set_error("grad_combine: invalid argument (1 <= K <= %d, ld >= n >= 1, G, out)", PPSCI_MTL_MAX_LOSSES);
    return PPSCI_E_INVALID;
  }
  if ((w_dev != nullptr) == (w_host != nullptr)) {
    ppsci_set_error("grad_combine: exactly one of w_dev (device) and w_host (host) carries the weights");
    return PPSCI_E_INVALID;
  }
  if (adam && (!params || !adam->m || !adam->v || adam->step_t < 1)) {
    ppsci_set_error("grad_combine: the Adam update needs params, m, v and step_t >= 1");
    return PPSCI_E_INVALID;
  }
  GradCombineArgs a;
  memset(&a, 0, sizeof(a));
  a.G = G;
  a.n = n;
  a.ld = ld;
  a.K = K;
  a.vec = ((((uintptr_t)G | (uintptr_t)out) & 15) == 0 && (ld % 4 == 0 || K == 1)) ? 1 : 0;
  a.w_dev = w_dev;
  if (w_host)
    for (int k = 0; k < K; ++k) a.w[k] = w_host[k];
  a.out = out;
  if (adam) {
    // (the bias corrections exactly as ppsci_adam_step forms them)
    const double b1t = pow((double)adam->beta1, (double)adam->step_t), b2t = pow((double)adam->beta2, (double)adam->step_t);
    const double c2 = sqrt(1.0 - b2t);
    a.do_adam = 1;
    a.adam = AdamArgs{params, out, adam->m, adam->v, n, (float)(adam->lr * c2 / (1.0 - b1t)), adam->beta1, adam->beta2,
                      (float)(adam->eps * c2), adam->grad_scale};
  }
  const long long n4 = a.vec ? n >> 2 : 0;
  const long long nthr = n4 + (n - 4 * n4);
  PPSCI_LAUNCH(grad_combine_kernel, GradCombineArgs, (int)((nthr + 255) / 256), 256, 0, stream, a);
  if (PPSCI_LAST_LAUNCH_ERROR() != 0) {
    ppsci_set_error("grad_combine: launch failed");
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}
