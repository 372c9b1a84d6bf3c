// taylor_fused.inc -- the whole training step of one constraint, tile by tile, with NOTHING of a tile leaving the CU:
// forward Taylor streams -> last linear -> residual program + loss seeds (epilogue VM) -> reverse sweep, for padded
// width 64 (NB = 4) on the bf16 (XDL) matrix pipe.  Included once per activation (taylor_fused_<act>.hip).
//
// One iteration of /root/reference/ppsci/solver/train.py:82-184 for one constraint --
//   model forward + derivative sweeps + expression + loss   (utils/expression.py:89-126, loss/mse.py:82-105)
//   total_loss.backward()                                    (train.py:158)
//   optimizer.step()                                         (train.py:175, optimizer/optimizer.py:225-248)
// The separate kernels (taylor_fwd -> epilogue -> taylor_bwd_wx) hand the activation stash of every hidden layer
// (4.1 KB per point: 410 MB per 100 000 Allen-Cahn points) through HBM: written once, read once, 518x the algorithmic
// bytes of the step, and the forward kernel is bound by those stores.  Here
//   * one WORKGROUP of NB waves owns a 16-point tile from its inputs to its gradient contribution; wave w owns feature
//     block w of every hidden layer (the feature-split model of taylor_fwd_wx.inc / taylor_bwd_wx.inc);
//   * the stash is L x S float4 REGISTERS per lane (the wave's own block of every layer: 64 registers at 4 x 64, S = 4);
//   * U, dL/dU and the tile's inputs live in LDS; the epilogue VM (epilogue_vm.h, EPI_RF_FUSED) runs on 16 lanes of
//     wave 0 between the two sweeps -- the MSE seed of a point depends on that point only, so nothing grid-wide sits
//     between forward and reverse;
//   * Wbar stays in registers for the whole launch, as in taylor_bwd_wx.inc ((L-1) x NB x 4 registers);
//   * the launch ends with the reduction tree of taylor_step_tail.h (gradient, loss terms and Adam by the workgroup that
//     finishes last) or, for large grids, leaves the workgroups' rows to the two reduction kernels (StepTail::external).
// HBM traffic per step: the inputs, the optional U / dL/dU / residual rows, the pre-split weight fragments (L2) and
// one 48 KB row per workgroup.
#include "taylor_tile.h"
#include "taylor_step_tail.h"
#include "epi_static.h"

#include <stdlib.h>
#include <string.h>
#include <type_traits>

#ifndef PPSCI_FUSED_STATIC
#define PPSCI_FUSED_STATIC 0  // 1 (taylor_fused_static_<act>.hip): this unit instantiates the kernels of compile-time residual programs
#endif
// Which instantiations keep the bias gradients as per-lane sums over the launch (LANE_BIAS in the kernel): those whose register
// budget holds the L x 4 accumulators next to the L x S float4 of the stash without new scratch bytes -- read off the
// compiler's resource table of every instantiation (DESIGN 4.2): L (S + 1) <= 20 for the tanh kernels of compile-time
// programs (the primary config, 4 x 64 with S = 4, is at 20: 233 -> 253 VGPRs, no scratch), <= 12 for all others (the other
// activations' derivative chains and the VM's parking of wave 0 leave less room).  The rest keep the per-tile sums.
// -D'PPSCI_FUSED_LANE_BIAS(L,S,ACT,STATIC)=false': per-tile sums everywhere (A/B builds).
#ifndef PPSCI_FUSED_LANE_BIAS
#define PPSCI_FUSED_LANE_BIAS(L, S, ACT, STATIC) ((L) * ((S) + 1) <= (((STATIC) && (ACT) == PPSCI_ACT_TANH) ? 20 : 12))
#endif
#define PPSCI_FUSED_EPI_SCRATCH ((PPSCI_MAX_RES + PPSCI_MAX_EPARAM) * 16)  // epi_finale's LDS (floats)
#define PPSCI_FUSED_SPEC_TAB (64 + PPSCI_MAX_RES + PPSCI_MAX_DIRS * PPSCI_FUSED_MAX_IN)  // shape-specialised kernels: LDS table floats
#define PPSCI_FUSED_MAX_IN 4  // raw inputs held in registers per lane (x, y, z, t); nets with more take the separate launches
// KEEP kernels of even depth (taylor_fused_kernel): 1 = the h_0 planes that reverse layer 1 recomputes go to the keep buffer `kx`
// too, so that nothing of a tile's last Wbar GEMM reads `hx` and the WAR barrier in front of the next tile's first publish is
// gone; 0 = they go to `hx` and the barrier stays (A/B builds; the kept planes of layer L-2 do not depend on this)
#ifndef PPSCI_FUSED_KEEP_H0
#define PPSCI_FUSED_KEEP_H0 1
#endif
// x[j] for a runtime j out of the register array (a select chain: dynamic indexing would put the array into scratch)
#define PPSCI_FUSED_XJ(x, j) ((j) == 0 ? (x)[0] : ((j) == 1 ? (x)[1] : ((j) == 2 ? (x)[2] : (x)[3])))

// -DPPSCI_FUSED_TIMERS (tools/fused_phases.py, never in the product build): every wave sums the shader cycles it spends in
// each phase of a tile (s_memtime stamps) and leaves the sums in the residual output buffer, 16 floats per wave.
#ifdef PPSCI_FUSED_TIMERS
#define PPSCI_FT(k)                                             \
  {                                                             \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    tacc[k] += now_ - tlast;                                    \
    tlast = now_;                                               \
  }
#else
#define PPSCI_FT(k)
#endif

// -DPPSCI_ABL_BUILD (tools/fused_ablate.sh, never in the product build; the mask is chosen at run time by PPSCI_ABL=<bits>
// among the instantiated single-bit masks): the kernel WITHOUT one of its parts, for
// timing only (the results are wrong) -- what the kernel's time is made of, measured instead of read off per-phase clocks
// (which charge every LDS / scalar-load wait to the phase that happens to hit it).
//   0 reverse layer 0 (W0 gradient)   1 forward layer 0   2 bias / last-layer row sums + LDS atomics   3 Wbar GEMM phase
//   4 hbar MFMAs   5 forward MFMAs   6 the three-term splits (a cheap stand-in)   7 activation evaluation (stand-in)
//   8 the residual program   9 the forward / reverse LDS publishes (stores)
#define PPSCI_ABL(n) (((ABL) >> (n)) & 1)
template <int ABL>
__device__ __forceinline__ ppsci_split4 ppsci_fused_split(f32x4 x) {
  if (PPSCI_ABL(6)) {
    ppsci_split4 o;
    o.p[0] = (u32x2){__builtin_bit_cast(unsigned, x[0]), __builtin_bit_cast(unsigned, x[1])};
    o.p[1] = (u32x2){__builtin_bit_cast(unsigned, x[2]), __builtin_bit_cast(unsigned, x[3])};
    o.p[2] = o.p[0];
    return o;
  }
  return ppsci_split(x);
}

// -DPPSCI_DBG_DUMP (tools/build_variant.py + tools/det_probe7.py): the top layer's zbar, its row sums, the activation derivatives and
// hbar of the layer below, per workgroup, into a buffer set with ppsci_dbg_set() -- how the packed-multiply finding was located.
#ifdef PPSCI_DBG_DUMP
__device__ float* ppsci_dbg_buf = nullptr;
extern "C" int ppsci_dbg_set(float* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(ppsci_dbg_buf), &p, sizeof(p)); }
#define PPSCI_DBG_STRIDE 16384
#endif

// (pointwise arithmetic on whole float4 registers: ppsci_act_from_stash4, taylor_tile.h)

// LDS floats of one workgroup
static inline long long ppsci_fused_floats(const ppsci_mlp_desc& d, const ppsci_derived& q, int S, int n_instr) {
  const int m = d.d_out, pad4m = ((m + 3) / 4) * 4;
  long long fl = 2LL * ((q.d0 + d.n_hidden + m) * q.HP + pad4m);  // W0s Bs WLs BLs | gW0 gB gWL gBL
  fl += (q.NB + 1) * m * S * PPSCI_TILE;                           // tin: dL/dU of the tile, one copy per wave (compile-time programs:
                                                                   // every wave evaluates the program itself) | uls: its stream values
  fl += q.NB * d.d_raw * PPSCI_TILE;                               // tinx: the tile's inputs (LD_IN, reverse layer 0), one copy per wave
  fl += (long long)q.NB * m * S * PPSCI_TILE;                      // red: last-linear partial sums per wave
  fl += PPSCI_FUSED_EPI_SCRATCH + PPSCI_MAX_RES * PPSCI_TILE;      // loss reduction scratch | per-lane loss sums
  fl += 2LL * n_instr * PPSCI_TILE;                                // VM register file
  fl += EPI_FAST_WORDS + PPSCI_MAX_RES + PPSCI_MAX_RES * PPSCI_TILE;  // tables of the pre-decoded program | residual values of the tile
  fl += 2LL * S * q.NB * 3 * 64 * 2;                               // zx | hx: split planes, [S][NB][3][64] x 8 bytes
  fl += PPSCI_MAX_DIRS * q.HP;                                     // dz0: layer-0 pre-activations of the first-derivative streams (raw inputs)
  return fl;
}

// LDS floats of one workgroup of a shape-specialised kernel (the kernel's carve-up with its compile-time shape): what a STATIC
// plan never touches is left out -- the VM register file, `uls`, `rres` and all of the program tables but the constants and scales
// KEEP: a third exchange buffer `kx` behind `hx`; to stay within half a CU, `ered` (used behind the tile loop only) aliases `zx`
// and `dz0` holds the N1 rows that are used instead of PPSCI_MAX_DIRS
template <int NB, int LH, int N1, int N2, int D_RAW, int M, bool KEEP = false>
static constexpr long long ppsci_fused_floats_spec() {
  constexpr int S = 1 + N1 + N2, HP = 16 * NB, pad4m = ((M + 3) / 4) * 4;
  long long fl = 2LL * ((D_RAW + LH + M) * HP + pad4m);        // W0s Bs WLs BLs | gW0 gB gWL gBL
  fl += 2LL * NB * M * S * PPSCI_TILE;                         // tin | red
  fl += NB * D_RAW * PPSCI_TILE;                               // tinx
  fl += (KEEP ? 0 : PPSCI_FUSED_EPI_SCRATCH) + PPSCI_MAX_RES * PPSCI_TILE;  // ered | lacc
  fl += PPSCI_FUSED_SPEC_TAB;                                  // constants | scales | directions
  fl += (KEEP ? 3LL : 2LL) * S * NB * 3 * 64 * 2;              // zx | hx (| kx)
  fl += (KEEP ? N1 : PPSCI_MAX_DIRS) * HP;                     // dz0
  return fl;
}
// KEEP is instantiated where there is a layer to keep planes for and two workgroups of the larger carve-up share a CU
template <int NB, int LH, int N1, int N2, int D_RAW, int M>
static constexpr bool ppsci_fused_keep_fits() {
  return LH >= 3 && 4 * ppsci_fused_floats_spec<NB, LH, N1, N2, D_RAW, M, true>() <= PPSCI_LDS_LIMIT_BYTES / 2;
}

// STATIC: the kernel of plans whose residual program is a compile-time table (args.e.static_id > 0, epi_static.h) AND whose
// inputs are all raw (no period embedding, no input streams: taylor_api.hip fill_step) -- it holds neither the VM nor the
// interpreter (their registers, the parking of the stash around them, the barrier behind them) nor the general layer 0;
// !STATIC: the program runs on the VM (pre-decoded) or on the interpreter, on wave 0.
// D_RAW, M > 0 (shape-specialised, STATIC only): the number of raw inputs and of net outputs are compile-time -- the loops over
// them, every offset of the LDS carve-up (ppsci_fused_floats_spec) and the guards of the optional outputs (U, dL/dU, residual
// values: such plans take the D_RAW = M = 0 kernel) leave the tile loop, and with them the uniform values the compiler kept
// alive for them across the loop in spilled SGPRs.  Same arithmetic, order, barriers and exchange layouts.
// KEEP (shape-specialised kernels with L >= 3): h_{L-3} is split once per tile instead of twice -- the
// split planes of h_{L-3}, which forward layer L-2 publishes (paired layout) for its GEMM, are written a second time into a third
// exchange buffer `kx` in the unpaired layout [S][NB][3][64]; reverse layer L-2 reads them there as the A operand of its Wbar
// GEMM instead of evaluating, splitting and publishing h_{L-3} from the stash again (for l = L-1 the forward sweep's last
// publish already serves: HPAIR).  Same values, same MFMA sequence, same barriers in the reverse sweep.  The hazard table of the
// three buffers is in DESIGN 4.2.
template <int NB, int LH, int N1, int N2, int ACT, bool STATIC, int ABL = 0, int D_RAW = 0, int M = 0, bool KEEP = false>
__global__ void __launch_bounds__(64 * NB, 2) taylor_fused_kernel(StepArgs args) {
  constexpr int S = 1 + N1 + N2;
  constexpr bool SPEC = D_RAW > 0;
  static_assert(!SPEC || (STATIC && M > 0 && D_RAW <= PPSCI_FUSED_MAX_IN), "shape-specialised kernels are STATIC kernels");
  static_assert(!KEEP || (SPEC && LH >= 3 && ABL == 0), "planes are kept by shape-specialised kernels with a layer L-2 >= 1");
  // even depth: reverse layer 1 publishes its recomputed h_0 into kx (free there: its readers, Wbar_{L-2}, are behind that layer's
  // first barrier for every wave) -- then nothing of a tile's last Wbar GEMM reads hx, where the next tile's first publish goes
  constexpr bool KEEP_H0 = KEEP && PPSCI_FUSED_KEEP_H0 != 0 && (LH % 2) == 0 && LH >= 4;
  constexpr int HP = 16 * NB;
  constexpr int W = NB;
  constexpr int L = LH;
  constexpr int NKP = NB / 2;
  constexpr bool LANE_BIAS = PPSCI_FUSED_LANE_BIAS(LH, S, ACT, STATIC);
  static_assert(NB == 4, "one feature block per wave, both k-pairs of a layer's fragments held in registers");
  PPSCI_DYN_SMEM(smem);
  const FwdArgs& a = args.f;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int H = a.d.width, m = SPEC ? M : a.d.d_out, d0 = SPEC ? D_RAW : a.q.d0, d_raw = SPEC ? D_RAW : a.d.d_raw;
  const int pad4m = ((m + 3) / 4) * 4;
  const int n_instr = SPEC ? 0 : args.e.e.n_instr;

  float* W0s = smem;
  float* Bs = W0s + d0 * HP;
  float* WLs = Bs + L * HP;
  float* BLs = WLs + m * HP;
  float* gW0 = BLs + pad4m;
  float* gB = gW0 + d0 * HP;
  float* gWL = gB + L * HP;
  float* gBL = gWL + m * HP;
  float* tin = gBL + pad4m;                        // [W][m*S][16] dL/dU of the tile (the VM: copy 0; compile-time programs: copy `wave`)
  float* uls = tin + W * m * S * PPSCI_TILE;       // [m*S][16] U of the tile (pre-decoded programs with a VGPR register file)
  float* tinx = uls + (SPEC ? 0 : m * S * PPSCI_TILE);  // [W][d_raw][16] inputs of the tile as the residual program / reverse layer 0 read them
  float* red = tinx + W * d_raw * PPSCI_TILE;      // [W][m*S][16] last-linear partial sums
  float* ered = red + W * m * S * PPSCI_TILE;      // epi_finale scratch (KEEP: no region of its own, see below)
  float* lacc = ered + (KEEP ? 0 : PPSCI_FUSED_EPI_SCRATCH);  // [PPSCI_MAX_RES][16] loss sums of the VM lanes
  float* rf = lacc + PPSCI_MAX_RES * PPSCI_TILE;   // VM register file: values [n][16] | adjoints [n][16]
  unsigned* ftab = (unsigned*)(rf + 2 * n_instr * PPSCI_TILE);  // tables of the pre-decoded program (epi_fast_init)
  float* rres = (float*)(ftab + EPI_FAST_WORDS + PPSCI_MAX_RES);  // [PPSCI_MAX_RES][16] residual values of the tile
  // (SPEC: no uls / rf / rres; of the tables only the 64 constants, the PPSCI_MAX_RES scales and the N1 x D_RAW directions)
  u32x2* zx = (u32x2*)(SPEC ? (float*)ftab + PPSCI_FUSED_SPEC_TAB : rres + PPSCI_MAX_RES * PPSCI_TILE);  // [S][NB][3][64] split planes (paired layout): zbar_l; forward: h of odd layers
  u32x2* hx = zx + S * NB * 3 * 64;                     // the same: h_{l-1};                             forward: h of even layers
  u32x2* kx = hx + S * NB * 3 * 64;                     // KEEP: [S][NB][3][64] split planes (unpaired): h_{L-3} of the forward sweep
  float* dz0 = (float*)(hx + (KEEP ? 2 : 1) * S * NB * 3 * 64);  // [N1][HP]: z_0 of the first-derivative streams when every input is raw (below)
  // KEEP: epi_finale's scratch is zx -- it runs behind the tile loop and the __syncthreads() in front of the row stores, when no
  // wave reads an exchange buffer any more
  if constexpr (KEEP) ered = (float*)zx;
  static_assert(!KEEP || PPSCI_FUSED_EPI_SCRATCH * 4 <= S * NB * 3 * 64 * 8, "ered must fit into zx");
  f32x4* zsave = (f32x4*)hx;  // [L][S][64]: wave 0 parks its stash here while it runs the residual program (both exchange
                              // buffers are idle between the sweeps; L x S KiB <= the S x NB x 1.5 KiB of one for L <= 6)
  static_assert(L * S * 64 * 16 <= S * NB * 3 * 64 * 8, "zsave must fit into hx");
  // the parked Wbar accumulators of wave 0 (register-file VM) must fit into zx | hx
  constexpr bool VM_REGS_OK = (L - 1) * NB * 64 * 16 <= S * NB * 3 * 64 * 8;  // (wacc -> zx, the stash -> hx)
  float* prow = args.b.partials + (long long)blockIdx.x * ppsci_small_params(a.d, a.q);

  for (int idx = tid; idx < d0 * HP; idx += nthr) {
    const int k = idx / HP, f = idx - k * HP;
    W0s[idx] = (f < H) ? a.params[a.q.offW[0] + k * H + f] : 0.f;
  }
  for (int idx = tid; idx < L * HP; idx += nthr) {
    const int l = idx / HP, f = idx - l * HP;
    Bs[idx] = (f < H) ? a.params[a.q.offB[l] + f] : 0.f;
  }
  for (int idx = tid; idx < m * HP; idx += nthr) {
    const int cc = idx / HP, f = idx - cc * HP;
    WLs[idx] = (f < H) ? a.params[a.q.offW[L] + f * m + cc] : 0.f;
  }
  for (int idx = tid; idx < pad4m; idx += nthr) BLs[idx] = idx < m ? a.params[a.q.offB[L] + idx] : 0.f;
  // Every input raw (no period embedding, no caller-supplied input streams -- the common case): the layer-0 pre-activation
  // of a first-derivative stream is sum_j W0[j][f] dirs[i][j], the same for every point; of a second-derivative stream, 0.
  // One table per launch instead of d_raw x N1 multiply-adds (and as many descriptor look-ups) per tile.
  bool raw_only = true;
  if constexpr (!SPEC)
    for (int j = 0; j < d_raw; ++j) raw_only = raw_only && a.d.embed[j] == PPSCI_EMBED_NONE;
  if (raw_only)
    for (int idx = tid; idx < N1 * HP; idx += nthr) {
      const int i = idx / HP, f = idx - i * HP;
      float acc = 0.f;
      for (int j = 0; j < d_raw; ++j) acc += ((f < H) ? a.params[a.q.offW[0] + j * H + f] : 0.f) * a.d.dirs[i][j];
      dz0[idx] = acc;
    }
  const int nacc_small = (d0 + L + m) * HP + pad4m;  // gW0 .. gBL are contiguous
  for (int idx = tid; idx < nacc_small; idx += nthr) gW0[idx] = 0.f;
  for (int idx = tid; idx < PPSCI_MAX_RES * PPSCI_TILE; idx += nthr) lacc[idx] = 0.f;
  if constexpr (SPEC) {
    for (int k = tid; k < 64; k += nthr) ftab[k] = args.e.fast[192 + k];
    for (int k = tid; k < PPSCI_MAX_RES; k += nthr) ftab[64 + k] = __builtin_bit_cast(unsigned, args.e.e.res[k].scale);
    for (int k = tid; k < N1 * D_RAW; k += nthr) ((float*)ftab)[64 + PPSCI_MAX_RES + k] = a.d.dirs[k / D_RAW][k % D_RAW];
  } else if (args.e.fast != nullptr) epi_fast_init(args.e, ftab, rf + (lane & 15), PPSCI_TILE, tid, nthr, wave == 0 && lane < PPSCI_TILE);

  // The raw inputs of a tile arrive in REGISTERS: every lane holds the (up to PPSCI_FUSED_MAX_IN) inputs of ITS point c,
  // requested during the previous tile's reverse sweep (an HBM round trip that nothing of that tile depends on).  Wave 0
  // puts them into LDS for the residual program and the reverse sweep's layer 0 (ordered by the two barriers around the
  // program); there is no barrier between one tile's reverse sweep and the next tile's first layer.
  float xr[PPSCI_FUSED_MAX_IN];  // top of a tile: ITS inputs; from the reverse sweep on: the next tile's (in flight)
  const auto fetch_x = [&](int tile_, float (&dst)[PPSCI_FUSED_MAX_IN]) {
    const long long p_ = (long long)tile_ * PPSCI_TILE + c;
    const bool ok_ = tile_ < a.ntiles && p_ < a.N;
#pragma unroll
    for (int j = 0; j < PPSCI_FUSED_MAX_IN; ++j) dst[j] = (j < d_raw && ok_) ? a.x[j < d_raw ? j : 0][p_] : 0.f;
  };
  fetch_x(a.tile0 + (int)blockIdx.x, xr);
  __syncthreads();
  // compile-time residual programs (epi_static.h): the constants of the load table and the terms' scales, entry k in lane k
  const int static_id = STATIC ? args.e.static_id : 0;
  float st_cvals = 0.f, st_scales = 0.f;
  if constexpr (SPEC) {
    st_cvals = __builtin_bit_cast(float, ftab[lane & 63]);
    st_scales = __builtin_bit_cast(float, ftab[64 + (lane & (PPSCI_MAX_RES - 1))]);
  } else if constexpr (STATIC) {
    st_cvals = __builtin_bit_cast(float, ftab[192 + (lane & 63)]);
    st_scales = __builtin_bit_cast(float, ftab[EPI_FAST_WORDS + (lane & (PPSCI_MAX_RES - 1))]);
  }
  const float* const dirs_s = (const float*)ftab + 64 + PPSCI_MAX_RES;  // SPEC: [N1][D_RAW] directions (reverse layer 0)

  // running sums of Wbar_{l+1}[all input blocks ib][own output block], l = 0 .. L-2
  f32x4 wacc[L - 1][NB];
#pragma unroll
  for (int l = 0; l < L - 1; ++l)
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) wacc[l][ib] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // LANE_BIAS: the bias gradients stay per-lane sums over all tiles of the workgroup (hb[0] of layer l behind its pointwise
  // adjoint; the points of a ragged tile that do not exist carry zero seeds) and are summed over the 16 points ONCE, behind
  // the tile loop -- instead of four dependent DPP adds per register and an LDS atomic per tile and layer, directly in front
  // of the split and publish of zbar_l.  L x 4 registers; instantiations that have no room for them keep the per-tile sums.
  f32x4 bacc[LANE_BIAS ? L : 1];
#pragma unroll
  for (int l = 0; l < (LANE_BIAS ? L : 1); ++l) bacc[l] = (f32x4){0.f, 0.f, 0.f, 0.f};

#ifdef PPSCI_FUSED_TIMERS
  if (tid < 16) ((unsigned*)ered)[tid] = 0u;
  unsigned long long tacc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tlast = __builtin_amdgcn_s_memtime();
#endif
  for (int it = 0; it < a.iters; ++it) {
    const int tile = a.tile0 + it * (int)gridDim.x + (int)blockIdx.x;  // uniform over the workgroup
    if (tile >= a.ntiles) break;
    PPSCI_FT(0)
    // SPEC: the lane index is opaque once per tile -- the masks derived from it (c == 15, g == 0, lane < 16) are then one compare
    // where they are used instead of SGPR pairs kept (spilled) across the whole loop
    int lane_t = lane;
    if constexpr (SPEC) PPSCI_OPAQUE(lane_t);
    const int lane = lane_t, g = lane >> 4, c = lane & 15;
    // compile-time programs: every wave has its own copy of dL/dU and of the tile's inputs (no barrier between the sweeps)
    const float* tx = STATIC ? tinx + wave * (d_raw * PPSCI_TILE) : tinx;
    float* const tinw = STATIC ? tin + wave * (m * S * PPSCI_TILE) : tin;
    // ... and the aux arrays its program reads (labels, weights, LD_AUX operands) are requested here, a forward sweep ahead
    float auxv[EPI_STATIC_MAX_AUX];
#pragma unroll
    for (int k = 0; k < EPI_STATIC_MAX_AUX; ++k) auxv[k] = 0.f;
    if (STATIC && args.e.e.n_aux > 0) {
      const long long p_ = (long long)tile * PPSCI_TILE + c;
      const long long pp_ = p_ < a.N ? p_ : 0;
#pragma unroll
      for (int k = 0; k < EPI_STATIC_MAX_AUX; ++k)
        if (k < args.e.e.n_aux) auxv[k] = args.e.aux[k][pp_];
    }
    // the stash: pre-activation streams of the own block of every hidden layer (value slot: tanh(z) for tanh nets, else z)
    f32x4 zst[L][S];
    f32x4 h[S];

    // ================================================================== forward
    // ---- layer 0 (K = d0, VALU)
#pragma unroll
    for (int s = 0; s < S; ++s) h[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
      const long long p = (long long)tile * PPSCI_TILE + c;
      const long long pp = p < a.N ? p : 0;
      const float vm = p < a.N ? 1.f : 0.f;
      int k = 0;
      if (PPSCI_ABL(1)) h[0] += xr[0] * 0.01f;
      if ((STATIC || raw_only) && !PPSCI_ABL(1)) {  // (STATIC kernels are planned for raw inputs only: run_fused)
#pragma unroll
        for (int j = 0; j < PPSCI_FUSED_MAX_IN; ++j)
          if (j < d_raw) h[0] += *(const f32x4*)&W0s[j * HP + 16 * wave + 4 * g] * xr[j];
#pragma unroll
        for (int i = 0; i < N1; ++i) h[1 + i] = *(const f32x4*)&dz0[i * HP + 16 * wave + 4 * g];
      } else
      for (int j = 0; j < ((PPSCI_ABL(1) || STATIC) ? 0 : d_raw); ++j) {
        const float xj = PPSCI_FUSED_XJ(xr, j);
        const int e = a.d.embed[j];
        const int ncol = (e == PPSCI_EMBED_PERIOD) ? 2 : 1;
        float sn = 0.f, cs = 0.f;
        const float w = a.d.omega[j];
        if (e == PPSCI_EMBED_PERIOD) {
          sn = sinf(w * xj);
          cs = cosf(w * xj);
        }
        for (int qq = 0; qq < ncol; ++qq, ++k) {
          float val, d1v[N1 > 0 ? N1 : 1], d2v[N2 > 0 ? N2 : 1];
          if (e != PPSCI_EMBED_PERIOD) {
            val = xj;
#pragma unroll
            for (int i = 0; i < N1; ++i) d1v[i] = a.d.dirs[i][j];
#pragma unroll
            for (int i = 0; i < N2; ++i) d2v[i] = 0.f;
            if (e == PPSCI_EMBED_STREAMS) {  // x[j] is an [S, N] block: the caller's input streams (input transforms)
#pragma unroll
              for (int i = 0; i < N1; ++i) d1v[i] = vm * a.x[j][(long long)(1 + i) * a.N + pp];
#pragma unroll
              for (int i = 0; i < N2; ++i) d2v[i] = vm * a.x[j][(long long)(1 + N1 + i) * a.N + pp];
            }
          } else {
            val = (qq == 0) ? cs : sn;
            const float dv = (qq == 0) ? -w * sn : w * cs;
            const float ddv = (qq == 0) ? -w * w * cs : -w * w * sn;
#pragma unroll
            for (int i = 0; i < N1; ++i) d1v[i] = dv * a.d.dirs[i][j];
#pragma unroll
            for (int i = 0; i < N2; ++i) d2v[i] = ddv * a.d.dirs[i][j] * a.d.dirs[i][j];
          }
          const f32x4 w4 = *(const f32x4*)&W0s[k * HP + 16 * wave + 4 * g];
          h[0] += w4 * val;
#pragma unroll
          for (int i = 0; i < N1; ++i) h[1 + i] += w4 * d1v[i];
#pragma unroll
          for (int i = 0; i < N2; ++i) h[1 + N1 + i] += w4 * d2v[i];
        }
      }
      h[0] += *(const f32x4*)&Bs[16 * wave + 4 * g];
    }

    PPSCI_FT(1)
    // One hidden layer of the forward sweep; `l` is a compile-time constant so that the stash is indexed statically.
    //   l > 0: publish the split own block of h_{l-1} (odd l -> zx, even l -> hx: alternating buffers need ONE barrier per
    //   layer), z_l[own] = W_l^T h_{l-1} over all input blocks (A = pre-split fragments of W_l^T from L2, both k-pairs
    //   requested before the split), then: skip quirk, stash, activation.
    auto fwd_layer = [&](auto lc) {
      constexpr int l = decltype(lc)::value;
      int lanel = lane;
      PPSCI_OPAQUE(lanel);
      const int g = lanel >> 4;
      const int xcl = ppsci_xchunk(lanel >> 4, lanel & 15);
      if constexpr (l > 0) {
        // STATIC kernels (no stash parking in the exchange buffers between the sweeps): the LAST publish of the forward sweep --
        // the split planes of h_{L-2} -- lands in hx, where the reverse sweep's first layer reads them as the A operand of its
        // Wbar GEMM: no second evaluation, split and publish of h_{L-2} there.  For even L the first
        // publish of a tile then goes to hx as well, which the previous tile's last Wbar GEMM may still be reading in another
        // wave: one barrier in front of it (behind the layer-0 arithmetic: nobody waits long).
        // KEEP_H0: that GEMM reads kx instead, and kx is written behind this sweep's barriers only: no barrier here.
        u32x2* xb = STATIC ? (((L - 1 - l) & 1) ? zx : hx) : ((l & 1) ? zx : hx);
        if constexpr (STATIC && l == 1 && (L % 2) == 0 && !KEEP_H0) ppsci_block_sync_lds();
        // KEEP, l == L-2: the planes go to kx as well (unpaired, as the reverse publish of this layer wrote them into hx).  L == 3:
        // this is the tile's first publish and there is no barrier between it and the previous tile's last Wbar GEMM, which
        // reads kx in other waves -- the copy is written BEHIND this layer's barrier (from registers), not in front of it.
        constexpr bool KFWD = KEEP && l == L - 2, KLATE = KFWD && l == 1;
        ppsci_split4 spk[KLATE ? S : 1];
        const u32x4* gf = (const u32x4*)a.xfrag + (long long)(l - 1) * PPSCI_GFRAG_PER_LAYER(NB) + lanel;
        u32x4 Ak[NKP][3];
#pragma unroll
        for (int kp = 0; kp < NKP; ++kp)
#pragma unroll
          for (int q = 0; q < 3; ++q) Ak[kp][q] = gf[((wave * NKP + kp) * 3 + q) * 64];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const ppsci_split4 sp = ppsci_fused_split<ABL>(h[s]);
#pragma unroll
          for (int q = 0; q < 3; ++q)
            if (!PPSCI_ABL(9) || (sp.p[q][0] == 0x12345u && sp.p[q][1] == 0x54321u)) xb[ppsci_xpair(NB, s, wave, q, xcl)] = sp.p[q];
          if constexpr (KLATE) spk[s] = sp;
          else if constexpr (KFWD) {
#pragma unroll
            for (int q = 0; q < 3; ++q) kx[((s * NB + wave) * 3 + q) * 64 + xcl] = sp.p[q];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        ppsci_block_sync_lds();
        if constexpr (KLATE) {
#pragma unroll
          for (int s = 0; s < S; ++s)
#pragma unroll
            for (int q = 0; q < 3; ++q) kx[((s * NB + wave) * 3 + q) * 64 + xcl] = spk[s].p[q];
        }
        PPSCI_FT(2)
        h[0] = *(const f32x4*)&Bs[l * HP + 16 * wave + 4 * g];
#pragma unroll
        for (int s = 1; s < S; ++s) h[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // products grouped by the plane of B (small terms first): (A_h B_l) | (A_m B_m) (A_h B_m) | (A_l B_h) (A_m B_h) (A_h B_h);
        // the B operands of group g + 1 are requested BEFORE the MFMAs of group g (one group = one LDS round trip that
        // would otherwise be exposed six times per layer: the scheduler is not allowed to hoist them, see sched_barrier)
        {
          u32x4 bq[2][S];
          const auto load_b = [&](int grp, u32x4 (&dst)[S]) {
            const int kp = grp / 3, pb = 2 - grp % 3;
#pragma unroll
            for (int s = 0; s < S; ++s) dst[s] = *(const u32x4*)&xb[ppsci_xpair(NB, s, 2 * kp, pb, xcl)];  // both halves: one ds_read_b128
          };
          load_b(0, bq[0]);
#pragma unroll
          for (int grp = 0; grp < 3 * NKP; ++grp) {
            const int kp = grp / 3, pb = 2 - grp % 3;
            if (grp + 1 < 3 * NKP) load_b(grp + 1, bq[(grp + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pa = 2 - pb; pa >= 0; --pa)
#pragma unroll
              for (int s = 0; s < S; ++s) {
                const u32x4 bb = bq[grp & 1][s];
                if (PPSCI_ABL(5)) h[s][0] += __builtin_bit_cast(float, bb[0] ^ Ak[kp][pa][0]) * 1e-30f;
                else
                h[s] = ppsci_xdl32a(Ak[kp][pa], (u32x2){bb[0], bb[1]}, (u32x2){bb[2], bb[3]}, h[s]);
              }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      PPSCI_FT(3)
      const float zs = ppsci_zscale(a.d, l);
      if (zs != 1.f) {
#pragma unroll
        for (int s = 0; s < S; ++s) h[s] *= zs;
      }
#pragma unroll
      for (int s = 1; s < S; ++s) zst[l][s] = h[s];
      {
        f32x4 SV, F1, F2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv, d1, d2, d3;
          if (PPSCI_ABL(7)) sv = 0.5f * h[0][r], d1 = 0.5f, d2 = 0.1f, d3 = 0.f;
          else
          ppsci_act_eval<ACT>(h[0][r], sv, d1, d2, d3);
          SV[r] = sv, F1[r] = d1, F2[r] = d2;
        }
        zst[l][0] = (ACT == PPSCI_ACT_TANH) ? SV : h[0];
        h[0] = SV;
#pragma unroll
        for (int i = 0; i < N1; ++i) {  // (whole float4 registers: see ppsci_act_from_stash4)
          const f32x4 zi = h[1 + i];
          h[1 + i] = F1 * zi;
          if (i < N2) h[1 + N1 + i] = F2 * zi * zi + F1 * h[1 + N1 + i];
        }
      }
    };
    fwd_layer(std::integral_constant<int, 0>{});
    fwd_layer(std::integral_constant<int, 1>{});
    if constexpr (L > 2) fwd_layer(std::integral_constant<int, 2>{});
    if constexpr (L > 3) fwd_layer(std::integral_constant<int, 3>{});
    if constexpr (L > 4) fwd_layer(std::integral_constant<int, 4>{});

    PPSCI_FT(4)
    // ---- last linear (N = m): partial sums over the own features; the waves' partials meet in LDS
    for (int cc = 0; cc < m; ++cc) {
      const f32x4 w4 = *(const f32x4*)&WLs[cc * HP + 16 * wave + 4 * g];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const f32x4 t = w4 * h[s];
        float part = (t[0] + t[1]) + (t[2] + t[3]);
        part = ppsci_group_sum4(part);
        if (g == 0) red[(wave * (m * S) + cc * S + s) * PPSCI_TILE + c] = part;
      }
    }
    ppsci_block_sync_lds();

    PPSCI_FT(5)
    // ================================================================== residual program, loss terms, seeds
    // Compile-time program (epi_static.h): EVERY wave sums the waves' partials for the point of each of its lanes and runs
    // the straight-line program itself; dL/dU goes to the wave's own copy of `tin` -- no serial wave, no barrier.
    if constexpr (STATIC) {
      epi_static_dispatch<N1, N2>(static_id, [&](auto tag) {
        using P = typename decltype(tag)::type;
        const long long p = (long long)tile * PPSCI_TILE + c;
        const bool valid = p < a.N;
        float u[P::MS], ub[P::MS], rval[P::NR], lt[P::NR], ld[P::NR];
        epi_static_for<0, P::MS>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          float v = (q % S == 0) ? BLs[q / S] : 0.f;
#pragma unroll
          for (int w = 0; w < W; ++w) v += red[(w * P::MS + q) * PPSCI_TILE + c];
          u[q] = v;
        });
        if (PPSCI_ABL(8)) {
          epi_static_for<0, P::MS>([&](auto qc) { ub[decltype(qc)::value] = u[decltype(qc)::value] * 1e-3f; });
          epi_static_for<0, P::NR>([&](auto kc) { rval[decltype(kc)::value] = lt[decltype(kc)::value] = ld[decltype(kc)::value] = u[0]; });
        } else
        epi_static_eval<P, PPSCI_FUSED_MAX_IN>(u, xr, auxv, st_cvals, st_scales, valid, ub, rval, lt, ld);
        if (lane < PPSCI_TILE) {
          epi_static_for<0, P::MS>([&](auto qc) { tinw[decltype(qc)::value * PPSCI_TILE + lane] = ub[decltype(qc)::value]; });
          float* const txw = tinx + wave * (d_raw * PPSCI_TILE);
#pragma unroll
          for (int j = 0; j < PPSCI_FUSED_MAX_IN; ++j)
            if (j < d_raw) txw[j * PPSCI_TILE + lane] = xr[j];
          if (wave == 0 && valid)
            epi_static_for<0, P::NR>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              lacc[k * PPSCI_TILE + lane] = EPI_STATIC_FMA(lt[k], ld[k], lacc[k * PPSCI_TILE + lane]);
            });
          if (!SPEC && wave == 1 && valid) {  // optional outputs, by a wave that does not carry the loss sums (SPEC: none planned)
            if (a.U != nullptr) epi_static_for<0, P::MS>([&](auto qc) { a.U[(long long)decltype(qc)::value * a.N + p] = u[decltype(qc)::value]; });
            if (args.e.Ubar != nullptr)
              epi_static_for<0, P::MS>([&](auto qc) { args.e.Ubar[(long long)decltype(qc)::value * a.N + p] = ub[decltype(qc)::value]; });
            if (args.e.resid != nullptr)
              epi_static_for<0, P::NR>([&](auto kc) { args.e.resid[(long long)decltype(kc)::value * a.N + p] = rval[decltype(kc)::value]; });
          }
        }
        ppsci_wave_sync();  // (the wave's other lanes read its copies below)
      });
    } else {
    // (lanes 0..15 of wave 0; the other waves write U for the caller meanwhile, when it is wanted)
    if (a.U != nullptr && wave != 0) {  // (the wave that runs the program must not queue behind these stores)
      for (int idx = tid - 64; idx < m * S * PPSCI_TILE; idx += nthr - 64) {
        const int q = idx >> 4, cpt = idx & 15;
        float v = (q % S == 0) ? BLs[q / S] : 0.f;
#pragma unroll
        for (int w = 0; w < W; ++w) v += red[(w * (m * S) + q) * PPSCI_TILE + cpt];
        const long long pt = (long long)tile * PPSCI_TILE + cpt;
        if (pt < a.N) a.U[(long long)q * a.N + pt] = v;
      }
    }
    PPSCI_FT(13)
    if (wave == 0 && lane < PPSCI_TILE) {  // LD_IN operands of the residual program (written and read by this wave only)
#pragma unroll
      for (int j = 0; j < PPSCI_FUSED_MAX_IN; ++j)
        if (j < d_raw) tinx[j * PPSCI_TILE + lane] = xr[j];
    }
    if (wave == 0 && args.e.fast != nullptr) {
      // (the workgroup's other waves wait for this one: it goes first among the waves of its SIMD)
      ppsci_setprio(3);
      // pre-decoded program (adds / subtracts / products only): a few dozen branch-free steps, points on lanes 0..15
      const EpiFastRegs efr = epi_fast_regs(ftab, lane);
#ifdef PPSCI_FUSED_TIMERS
      if (tid == 0) ((unsigned*)ered)[15] = (unsigned)__builtin_amdgcn_s_memtime();
#endif
      const long long p = (long long)tile * PPSCI_TILE + (lane & 15);
      const bool valid = p < a.N;
      EpiFused fx;
      fx.red = red;
      fx.bl = BLs;
      fx.tinx = tx;
      fx.tin = tin;
      fx.rres = args.e.resid != nullptr ? rres : nullptr;
      fx.dbg = (unsigned*)ered;
      fx.W = W;
      fx.mS = m * S;
      fx.S = S;
      if (VM_REGS_OK && n_instr <= EPI_FAST_NREG) {
        // The VM's register file takes 2 x EPI_FAST_NREG registers: wave 0 parks its Wbar accumulators in LDS meanwhile
        // (the exchange buffers are idle between the sweeps) -- 24 LDS instructions per tile instead of scratch spills.
        f32x4* const wsave = (f32x4*)zx;
#pragma unroll
        for (int l = 0; l < L - 1; ++l)
#pragma unroll
          for (int ib = 0; ib < NB; ++ib) wsave[(l * NB + ib) * 64 + lane] = wacc[l][ib];
        // ... and its stash (zsave = hx): with both parked nothing of the program's working set spills to scratch memory,
        // whose reloads (a vmcnt wait each, in a wave the whole workgroup waits for) cost more than these LDS round trips
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
          for (int s = 0; s < S; ++s) zsave[(l * S + s) * 64 + lane] = zst[l][s];
        __builtin_amdgcn_sched_barrier(0);
        // the tile's stream values, one per lane (the waves' partial sums + the bias), then the program on registers
        for (int idx = lane; idx < m * S * PPSCI_TILE; idx += 64) {
          const int q = idx >> 4, cpt = idx & 15;
          float v = (q % S == 0) ? BLs[q / S] : 0.f;
#pragma unroll
          for (int w = 0; w < W; ++w) v += red[(w * (m * S) + q) * PPSCI_TILE + cpt];
          uls[idx] = v;
        }
        epi_tile_fast_regs<false>(args.e, efr, lane < PPSCI_TILE, p, valid ? p : 0, valid, lane & 15, lacc + (lane & 15), PPSCI_TILE,
                                  &fx, uls);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int l = 0; l < L - 1; ++l)
#pragma unroll
          for (int ib = 0; ib < NB; ++ib) wacc[l][ib] = wsave[(l * NB + ib) * 64 + lane];
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
          for (int s = 0; s < S; ++s) zst[l][s] = zsave[(l * S + s) * 64 + lane];
      } else
        epi_tile_fast(args.e, efr, rf + (lane & 15), rf + n_instr * PPSCI_TILE + (lane & 15), PPSCI_TILE, lane < PPSCI_TILE, p,
                      valid ? p : 0, valid, lane & 15, lacc + (lane & 15), &fx);
      ppsci_setprio(0);
    } else if (wave == 0) {
      // The generic interpreter (~40 opcodes, some of them libm calls) wants ~140 registers of its own; next to the
      // stash and the Wbar accumulators that spills.  Wave 0 therefore parks its stash in LDS around it (32 LDS
      // instructions per tile for one wave) -- a spill to LDS under our control instead of scratch memory.
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int s = 0; s < S; ++s) zsave[(l * S + s) * 64 + lane] = zst[l][s];
      if (lane < PPSCI_TILE) {
        const long long p = (long long)tile * PPSCI_TILE + lane;
        const bool valid = p < a.N;
        float lsum[PPSCI_MAX_RES], padj[PPSCI_MAX_EPARAM];
#pragma unroll
        for (int k = 0; k < PPSCI_MAX_RES; ++k) lsum[k] = lacc[k * PPSCI_TILE + lane];
#pragma unroll
        for (int k = 0; k < PPSCI_MAX_EPARAM; ++k) padj[k] = 0.f;
        EpiFused fx;
        fx.red = red;
        fx.bl = BLs;
        fx.tinx = tx;
        fx.tin = tin;
        fx.rres = nullptr;
        fx.dbg = nullptr;
        fx.W = W;
        fx.mS = m * S;
        fx.S = S;
#ifndef PPSCI_FX_NOVM
        epi_point<EPI_RF_FUSED>(args.e, rf + lane, rf + n_instr * PPSCI_TILE + lane, PPSCI_TILE, n_instr, p, valid ? p : 0, valid,
                                lane, lsum, padj, &fx);
#endif
#pragma unroll
        for (int k = 0; k < PPSCI_MAX_RES; ++k) lacc[k * PPSCI_TILE + lane] = lsum[k];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int s = 0; s < S; ++s) zst[l][s] = zsave[(l * S + s) * 64 + lane];
    }
    PPSCI_FT(14)
    ppsci_block_sync_lds();
    if (wave == 1 && args.e.fast != nullptr) {
      // optional outputs of the pre-decoded program, written by a wave that did not run it: dL/dU and the residual values
      if (args.e.Ubar != nullptr) {
        for (int idx = lane; idx < m * S * PPSCI_TILE; idx += 64) {
          const long long pt = (long long)tile * PPSCI_TILE + (idx & 15);
          if (pt < a.N) args.e.Ubar[(long long)(idx >> 4) * a.N + pt] = tin[idx];
        }
      }
      if (args.e.resid != nullptr) {
        for (int idx = lane; idx < args.e.e.n_res * PPSCI_TILE; idx += 64) {
          const long long pt = (long long)tile * PPSCI_TILE + (idx & 15);
          if (pt < a.N) args.e.resid[(long long)(idx >> 4) * a.N + pt] = rres[idx];
        }
      }
    }
    }  // !STATIC

    fetch_x(tile + (int)gridDim.x, xr);  // the next tile's inputs: in flight during the reverse sweep
    PPSCI_FT(6)
    // ================================================================== reverse
    f32x4 hb[S];  // adjoint of h_l (own block), turned into zbar_l in place (T layout)
#pragma unroll
    for (int s = 0; s < S; ++s) hb[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // ---- adjoint of the last linear (own block)
    for (int cc = 0; cc < m; ++cc) {
      float ub[S];
#pragma unroll
      for (int s = 0; s < S; ++s) ub[s] = tinw[(cc * S + s) * PPSCI_TILE + c];
      const f32x4 w4 = *(const f32x4*)&WLs[cc * HP + 16 * wave + 4 * g];
#pragma unroll
      for (int s = 0; s < S; ++s) hb[s] += w4 * ub[s];
      if (wave == 0 && !PPSCI_ABL(2)) {
        const float sb = ppsci_row_sum16_last(ub[0]);
        if (lane == 15) atomicAdd(&gBL[cc], sb);
      }
    }

    // One layer of the reverse sweep (taylor_bwd_wx.inc, with the stash in registers):
    //   pointwise adjoint -> zbar_l -> split planes to zx                                          | barrier
    //   hbar_{l-1} = W_l zbar_l (B = zx) ; h_{l-1} from the stash -> split planes to hx            | barrier
    //     (not where the forward sweep left them: l = L-1 of STATIC kernels, HPAIR; l = L-2 of KEEP kernels, in kx)
    //   Wbar_l += h_{l-1} (x) zbar_l  (A = hx, all blocks; B = the own block of zx; both through the transpose read)
    auto bwd_layer = [&](auto lc) {
      constexpr int l = decltype(lc)::value;
      const float zs = ppsci_zscale(a.d, l);
      int lanel = lane;
      PPSCI_OPAQUE(lanel);
      const int g = lanel >> 4, c = lanel & 15;
      const int xcl = ppsci_xchunk(lanel >> 4, lanel & 15);                            // writes, plain reads
      const int xtl = ppsci_xchunk(lanel & 3, 4 * (lanel >> 4) + ((lanel & 15) >> 2));  // transpose reads
      const u32x4* gf = (const u32x4*)args.b.xfrag + (long long)(l > 0 ? l - 1 : 0) * PPSCI_GFRAG_PER_LAYER(NB) + lanel;
      u32x4 Ab[NKP][3];
      // ---- pointwise: zbar_l in place of hbar_l (own block); publish its split planes
      {
        f32x4 D1, D2, D3, hv;
        if (PPSCI_ABL(7)) {
          hv = zst[l][0];
          D1 = (f32x4){0.5f, 0.5f, 0.5f, 0.5f}, D2 = (f32x4){0.1f, 0.1f, 0.1f, 0.1f}, D3 = (f32x4){0.01f, 0.01f, 0.01f, 0.01f};
        } else
          ppsci_act_from_stash4<ACT>(zst[l][0], hv, D1, D2, D3);
#ifdef PPSCI_DBG_DUMP
        if (ppsci_dbg_buf != nullptr && l == L - 1) {
          float* q = &ppsci_dbg_buf[(long long)blockIdx.x * PPSCI_DBG_STRIDE + 5120];
          *(f32x4*)&q[(0 * 256 + tid) * 4] = D2;
          *(f32x4*)&q[(1 * 256 + tid) * 4] = D3;
        }
#endif
        if constexpr (l == L - 1) {
          // Wbar_last[f][cc] += sum_pts sum_s h_s[f] * ubar[cc][s]   (own features), h_{L-1} streams from the stash
          f32x4 hc[S];
          hc[0] = hv;
#pragma unroll
          for (int i = 0; i < N1; ++i) {
            hc[1 + i] = D1 * zst[l][1 + i];
            if (i < N2) hc[1 + N1 + i] = D2 * zst[l][1 + i] * zst[l][1 + i] + D1 * zst[l][1 + N1 + i];
          }
          for (int cc = 0; cc < (PPSCI_ABL(2) ? 0 : m); ++cc) {
            f32x4 t = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < S; ++s) t += hc[s] * tinw[(cc * S + s) * PPSCI_TILE + c];
            f32x4 v4;
#pragma unroll
            for (int r = 0; r < 4; ++r) v4[r] = ppsci_row_sum16_last(t[r]);
            if (c == 15) {
#pragma unroll
              for (int r = 0; r < 4; ++r) atomicAdd(&gWL[cc * HP + 16 * wave + 4 * g + r], v4[r]);
            }
          }
        }
#ifdef PPSCI_DBG_DUMP
        if (ppsci_dbg_buf != nullptr && l == L - 1) {
          float* q = &ppsci_dbg_buf[(long long)blockIdx.x * PPSCI_DBG_STRIDE + 12288];
          *(f32x4*)&q[(0 * 256 + tid) * 4] = D2;
          *(f32x4*)&q[(1 * 256 + tid) * 4] = D3;
          *(f32x4*)&q[(2 * 256 + tid) * 4] = D1;
        }
#endif
        {  // (whole float4 registers: see ppsci_act_from_stash4)
          const f32x4 two = {2.f, 2.f, 2.f, 2.f};
          f32x4 accv = D1 * hb[0];
#pragma unroll
          for (int i = 0; i < N1; ++i) {
            const f32x4 zi = zst[l][1 + i];
            const f32x4 hbi = hb[1 + i];
            f32x4 zbi = D1 * hbi;
            accv += D2 * zi * hbi;
            if (i < N2) {
              const f32x4 zii = zst[l][1 + N1 + i];
              const f32x4 hb2 = hb[1 + N1 + i];
              hb[1 + N1 + i] = D1 * hb2;
              zbi += two * D2 * zi * hb2;
              accv += (D3 * zi * zi + D2 * zii) * hb2;
            }
            hb[1 + i] = zbi;
          }
          hb[0] = accv;
        }
        if (zs != 1.f) {  // (skip-connection doubling / Siren scale: a uniform branch; plain nets skip S x 4 multiplications per layer)
#pragma unroll
          for (int s = 0; s < S; ++s) hb[s] *= zs;
        }
#ifdef PPSCI_DBG_DUMP
        if (ppsci_dbg_buf != nullptr && l == L - 1) {
#pragma unroll
          for (int s = 0; s < S; ++s) *(f32x4*)&ppsci_dbg_buf[(long long)blockIdx.x * PPSCI_DBG_STRIDE + (s * 256 + tid) * 4] = hb[s];
        }
#endif
        if constexpr (LANE_BIAS) {
          if (!PPSCI_ABL(2)) bacc[l] += hb[0];
        } else if (!PPSCI_ABL(2)) {
          f32x4 sb4;
#pragma unroll
          for (int r = 0; r < 4; ++r) sb4[r] = ppsci_row_sum16_last(hb[0][r]);
#ifdef PPSCI_DBG_DUMP
          if (ppsci_dbg_buf != nullptr && l == L - 1) *(f32x4*)&ppsci_dbg_buf[(long long)blockIdx.x * PPSCI_DBG_STRIDE + 4096 + tid * 4] = sb4;
#endif
          if (c == 15) {
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(&gB[l * HP + 16 * wave + 4 * g + r], sb4[r]);
          }
        }
        if constexpr (l > 0) {
          // A fragments of W_l (own row block): in flight across the split, the publish and the barrier
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kp = 0; kp < NKP; ++kp)
#pragma unroll
            for (int q = 0; q < 3; ++q) Ab[kp][q] = gf[((wave * NKP + kp) * 3 + q) * 64];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const ppsci_split4 sp = ppsci_fused_split<ABL>(hb[s]);
#pragma unroll
            for (int q = 0; q < 3; ++q)
              if (!PPSCI_ABL(9) || (sp.p[q][0] == 0x12345u && sp.p[q][1] == 0x54321u)) zx[ppsci_xpair(NB, s, wave, q, xcl)] = sp.p[q];
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }

      if constexpr (l > 0) {
        __builtin_amdgcn_sched_barrier(0);
        ppsci_block_sync_lds();  // zx (zbar_l) complete
        PPSCI_FT(7)
        // ---- hbar_{l-1}[own rows] = W_l[own rows, :] zbar_l : the streams are S independent accumulation chains;
        // products grouped by the plane of B: (A_h B_l) | (A_m B_m) (A_h B_m) | (A_l B_h) (A_m B_h) (A_h B_h)
#pragma unroll
        for (int s = 0; s < S; ++s) hb[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
        {  // (operand reads one group ahead of the MFMAs, as in the forward sweep)
          u32x4 bq[2][S];
          const auto load_b = [&](int grp, u32x4 (&dst)[S]) {
            const int kp = grp / 3, pb = 2 - grp % 3;
#pragma unroll
            for (int s = 0; s < S; ++s) dst[s] = *(const u32x4*)&zx[ppsci_xpair(NB, s, 2 * kp, pb, xcl)];  // one ds_read_b128
          };
          load_b(0, bq[0]);
#pragma unroll
          for (int grp = 0; grp < 3 * NKP; ++grp) {
            const int kp = grp / 3, pb = 2 - grp % 3;
            if (grp + 1 < 3 * NKP) load_b(grp + 1, bq[(grp + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pa = 2 - pb; pa >= 0; --pa)
#pragma unroll
              for (int s = 0; s < S; ++s) {
                const u32x4 bb = bq[grp & 1][s];
                if (PPSCI_ABL(4)) hb[s][0] += __builtin_bit_cast(float, bb[0] ^ Ab[kp][pa][0]) * 1e-30f;
                else
                hb[s] = ppsci_xdl32a(Ab[kp][pa], (u32x2){bb[0], bb[1]}, (u32x2){bb[2], bb[3]}, hb[s]);
              }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
#ifdef PPSCI_DBG_DUMP
        if (ppsci_dbg_buf != nullptr && l == L - 1) {
#pragma unroll
          for (int s = 0; s < S; ++s) *(f32x4*)&ppsci_dbg_buf[(long long)blockIdx.x * PPSCI_DBG_STRIDE + 8192 + (s * 256 + tid) * 4] = hb[s];
        }
#endif
        PPSCI_FT(8)
        // ---- h_{l-1} streams of the own block (the A operand of Wbar_l) from the stash of layer l-1 -> hx
        // (STATIC kernels, l == L-1: the forward sweep's last publish IS that operand -- in the paired layout of the B reads)
        // (KEEP kernels, l == L-2: the forward sweep left its planes in kx, in the layout this publish writes; KEEP_H0, l == 1:
        // published into kx instead of hx)
        constexpr bool HPAIR = STATIC && l == L - 1;
        constexpr bool HKEPT = KEEP && l == L - 2;
        u32x2* const ha = (HKEPT || (KEEP_H0 && l == 1)) ? kx : hx;  // A operand of Wbar_l
        if (!PPSCI_ABL(3) && !HPAIR && !HKEPT) {
          f32x4 E1, E2, E3;
          f32x4 hcs[S];
          if (PPSCI_ABL(7)) {
            hcs[0] = zst[l - 1][0];
            E1 = (f32x4){0.5f, 0.5f, 0.5f, 0.5f}, E2 = (f32x4){0.1f, 0.1f, 0.1f, 0.1f};
          } else
            ppsci_act_from_stash4<ACT>(zst[l - 1][0], hcs[0], E1, E2, E3);
#pragma unroll
          for (int i = 0; i < N1; ++i) {
            hcs[1 + i] = E1 * zst[l - 1][1 + i];
            if (i < N2) hcs[1 + N1 + i] = E2 * zst[l - 1][1 + i] * zst[l - 1][1 + i] + E1 * zst[l - 1][1 + N1 + i];
          }
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const ppsci_split4 sp = ppsci_fused_split<ABL>(hcs[s]);
#pragma unroll
            for (int q = 0; q < 3; ++q)
              if (!PPSCI_ABL(9) || (sp.p[q][0] == 0x12345u && sp.p[q][1] == 0x54321u)) ha[((s * NB + wave) * 3 + q) * 64 + xcl] = sp.p[q];
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        // hx (h_{l-1}) complete.  (HPAIR, HKEPT: nothing was published, but the barrier stays: the next layer overwrites zx, which
        // the other waves read -- all blocks -- in the hbar GEMM above)
        if (!PPSCI_ABL(3)) ppsci_block_sync_lds();
        PPSCI_FT(9)
        // ---- Wbar_l[all ib, own column block] += h_{l-1}[ib] (x) zbar_l[own]   (contraction over stream x point)
        // Both operands in N layout through the LDS transpose read; the NB input blocks are NB independent chains.
#pragma unroll 1
        for (int sp = 0; sp + 1 < (PPSCI_ABL(3) ? 0 : S); sp += 2) {
          int zs_ = ppsci_xpair(NB, sp, wave, 0, xtl);                                    // zx: paired layout
          int hs_ = HPAIR ? ppsci_xpair(NB, sp, 0, 0, xtl) : xtl + sp * NB * 3 * 64;      // hx / kx: [S][NB][3][64], or paired
          PPSCI_OPAQUE(zs_);
          PPSCI_OPAQUE(hs_);
          u32x2 zN0[3], zN1[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            zN0[q] = ppsci_lds_read_tr16(&zx[zs_ + q * 128]);
            zN1[q] = ppsci_lds_read_tr16(&zx[zs_ + (NKP * 3 + q) * 128]);
          }
          constexpr int IG = 2;  // input blocks per group: IG independent accumulation chains, 12 IG operand registers,
                                 // requested one group ahead of their MFMAs
          u32x2 hN0[2][IG][3], hN1[2][IG][3];
          const auto load_h = [&](int ig, int buf) {
#pragma unroll
            for (int e = 0; e < IG; ++e)
#pragma unroll
              for (int q = 0; q < 3; ++q) {
                if constexpr (HPAIR) {
                  hN0[buf][e][q] = ppsci_lds_read_tr16(&hx[hs_ + (((ig + e) >> 1) * 3 + q) * 128 + ((ig + e) & 1)]);
                  hN1[buf][e][q] = ppsci_lds_read_tr16(&hx[hs_ + ((NKP + ((ig + e) >> 1)) * 3 + q) * 128 + ((ig + e) & 1)]);
                } else {
                  hN0[buf][e][q] = ppsci_lds_read_tr16(&ha[hs_ + ((ig + e) * 3 + q) * 64]);
                  hN1[buf][e][q] = ppsci_lds_read_tr16(&ha[hs_ + ((NB + ig + e) * 3 + q) * 64]);
                }
              }
          };
          load_h(0, 0);
#pragma unroll
          for (int ig = 0; ig < NB; ig += IG) {
            const int buf = (ig / IG) & 1;
            if (ig + IG < NB) load_h(ig + IG, buf ^ 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < PPSCI_XDL_NPROD; ++q)
#pragma unroll
              for (int e = 0; e < IG; ++e)
                wacc[l - 1][ig + e] = ppsci_xdl32(hN0[buf][e][ppsci_xdl_pa[q]], hN1[buf][e][ppsci_xdl_pa[q]], zN0[ppsci_xdl_pb[q]],
                                                  zN1[ppsci_xdl_pb[q]], wacc[l - 1][ig + e]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        if constexpr (S & 1) {  // the odd last stream: K = 16 steps
          u32x2 zN0[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) zN0[q] = ppsci_lds_read_tr16(&zx[ppsci_xpair(NB, S - 1, wave, q, xtl)]);
          u32x2 hN0[NB][3];
#pragma unroll
          for (int e = 0; e < NB; ++e)
#pragma unroll
            for (int q = 0; q < 3; ++q)
              hN0[e][q] = ppsci_lds_read_tr16(HPAIR ? &hx[ppsci_xpair(NB, S - 1, e, q, xtl)] : &ha[(((S - 1) * NB + e) * 3 + q) * 64 + xtl]);
#pragma unroll
          for (int q = 0; q < PPSCI_XDL_NPROD; ++q)
#pragma unroll
            for (int e = 0; e < NB; ++e)
              wacc[l - 1][e] = ppsci_xdl16(hN0[e][ppsci_xdl_pa[q]], zN0[ppsci_xdl_pb[q]], wacc[l - 1][e]);
          __builtin_amdgcn_sched_barrier(0);
        }
        PPSCI_FT(10)
      } else {
        PPSCI_FT(7)
        // ---- layer 0: Wbar_0[k][own f] += sum_pts sum_s h0_s[k] * zbar_0,s[f]
        const long long p = (long long)tile * PPSCI_TILE + c;
        const long long pp = p < a.N ? p : 0;
        const float vm = p < a.N ? 1.f : 0.f;
        int k = 0;
        if constexpr (STATIC) {
          // raw inputs: column j of W0 sees (x_j, dirs[i][j], 0) as its value / first / second derivative streams
#pragma unroll
          for (int j = 0; j < PPSCI_FUSED_MAX_IN; ++j) {
            if (j < d_raw && !PPSCI_ABL(0)) {
              f32x4 t = hb[0] * tx[j * PPSCI_TILE + c];
#pragma unroll
              for (int i = 0; i < N1; ++i) t += hb[1 + i] * (SPEC ? dirs_s[i * D_RAW + j] : a.d.dirs[i][j]);
              f32x4 v4;
#pragma unroll
              for (int r = 0; r < 4; ++r) v4[r] = ppsci_row_sum16_last(t[r]);
              if (c == 15) {
#pragma unroll
                for (int r = 0; r < 4; ++r) atomicAdd(&gW0[j * HP + 16 * wave + 4 * g + r], v4[r]);
              }
            }
          }
        } else
        for (int j = 0; j < (PPSCI_ABL(0) ? 0 : d_raw); ++j) {
          const float xj = tx[j * PPSCI_TILE + c];  // (written by wave 0 in front of the residual program)
          const int e = a.d.embed[j];
          const int ncol = (e == PPSCI_EMBED_PERIOD) ? 2 : 1;
          const float w = a.d.omega[j];
          float sn = 0.f, cs = 0.f;
          if (e == PPSCI_EMBED_PERIOD) {
            sn = sinf(w * xj);
            cs = cosf(w * xj);
          }
          for (int qq = 0; qq < ncol; ++qq, ++k) {
            float val, d1v[N1 > 0 ? N1 : 1], d2v[N2 > 0 ? N2 : 1];
            if (e != PPSCI_EMBED_PERIOD) {
              val = xj;
#pragma unroll
              for (int i = 0; i < N1; ++i) d1v[i] = a.d.dirs[i][j];
#pragma unroll
              for (int i = 0; i < N2; ++i) d2v[i] = 0.f;
              if (e == PPSCI_EMBED_STREAMS) {
#pragma unroll
                for (int i = 0; i < N1; ++i) d1v[i] = vm * a.x[j][(long long)(1 + i) * a.N + pp];
#pragma unroll
                for (int i = 0; i < N2; ++i) d2v[i] = vm * a.x[j][(long long)(1 + N1 + i) * a.N + pp];
              }
            } else {
              val = (qq == 0) ? cs : sn;
              const float dv = (qq == 0) ? -w * sn : w * cs;
              const float ddv = (qq == 0) ? -w * w * cs : -w * w * sn;
#pragma unroll
              for (int i = 0; i < N1; ++i) d1v[i] = dv * a.d.dirs[i][j];
#pragma unroll
              for (int i = 0; i < N2; ++i) d2v[i] = ddv * a.d.dirs[i][j] * a.d.dirs[i][j];
            }
            f32x4 t = hb[0] * val;
#pragma unroll
            for (int i = 0; i < N1; ++i) t += hb[1 + i] * d1v[i];
#pragma unroll
            for (int i = 0; i < N2; ++i) t += hb[1 + N1 + i] * d2v[i];
            f32x4 v4;
#pragma unroll
            for (int r = 0; r < 4; ++r) v4[r] = ppsci_row_sum16_last(t[r]);
            if (c == 15) {
#pragma unroll
              for (int r = 0; r < 4; ++r) atomicAdd(&gW0[k * HP + 16 * wave + 4 * g + r], v4[r]);
            }
          }
        }
      }
    };
#ifndef PPSCI_FX_NOBWD
    if constexpr (L > 4) bwd_layer(std::integral_constant<int, 4>{});
    if constexpr (L > 3) bwd_layer(std::integral_constant<int, 3>{});
    if constexpr (L > 2) bwd_layer(std::integral_constant<int, 2>{});
    bwd_layer(std::integral_constant<int, 1>{});
#endif
    bwd_layer(std::integral_constant<int, 0>{});

    PPSCI_FT(11)
    // (no barrier here: tin / red are rewritten behind the next tile's own barriers, which every wave reaches only after
    // this tile's reverse sweep; the exchange planes zx / hx / kx likewise -- see the forward layer's comment)
    PPSCI_FT(12)
  }
#ifdef PPSCI_FUSED_TIMERS
  if (lane == 0 && args.t.external && wave != 1) {  // (the tree rows are unused when the reduction kernels follow the launch)
#pragma unroll
    for (int k = 0; k < 16; ++k) args.t.tree[((long long)blockIdx.x * W + wave) * 16 + k] = (float)tacc[k];
    if (wave == 0)  // the program's inner phases go into wave 1's slot (not otherwise reported)
      for (int k = 0; k < 16; ++k) args.t.tree[((long long)blockIdx.x * W + 1) * 16 + k] = (float)((unsigned*)ered)[k];
  }
#endif

  // ---- the wave's weight-gradient column block -> this workgroup's row (block layout of the per-tile dumps); the rows
  // are read by other workgroups later in this launch (reduction tree): agent-scope stores
  {
    f32x4* dst = args.b.wpart + (long long)blockIdx.x * ((L - 1) * NB * NB * 64) + lane;
#pragma unroll
    for (int l = 0; l < L - 1; ++l)
#pragma unroll
      for (int ib = 0; ib < NB; ++ib) {
        f32x4* const q = &dst[((long long)l * NB * NB + ib * NB + wave) * 64];
        // (read by the reduction KERNELS behind the launch: plain coalesced 16-byte stores; read by other workgroups of THIS
        // launch -- the reduction tree --: agent-scope write-through stores, two 8-byte halves each)
        if (args.t.external == 1) *q = wacc[l][ib];
        else ppsci_store_agent4(q, wacc[l][ib]);
      }
  }
  if constexpr (LANE_BIAS) {  // the per-lane bias sums -> gB (zero so far: nothing else writes it in this mode)
#pragma unroll
    for (int l = 0; l < L; ++l) {
      f32x4 sb4;
#pragma unroll
      for (int r = 0; r < 4; ++r) sb4[r] = ppsci_row_sum16_last(bacc[l][r]);
      if (c == 15) *(f32x4*)&gB[l * HP + 16 * wave + 4 * g] = sb4;
    }
  }
  // ---- the workgroup's small accumulators -> its partial row (compact order of ppsci_small_params)
  __syncthreads();
  for (int idx = tid; idx < d0 * H; idx += nthr) {
    const int k = idx / H, f = idx - k * H;
    ppsci_store_agent(&prow[idx], gW0[k * HP + f]);
  }
  for (int idx = tid; idx < L * H; idx += nthr) {
    const int l = idx / H, f = idx - l * H;
    ppsci_store_agent(&prow[d0 * H + idx], gB[l * HP + f]);
  }
  for (int idx = tid; idx < H * m; idx += nthr) {
    const int f = idx / m, cc = idx - f * m;
    ppsci_store_agent(&prow[(d0 + L) * H + idx], gWL[cc * HP + f]);
  }
  for (int idx = tid; idx < m; idx += nthr) ppsci_store_agent(&prow[(d0 + L + m) * H + idx], gBL[idx]);
  // ---- the workgroup's loss terms -> its row of args.e.partials
  {
    float lsum[PPSCI_MAX_RES], padj[PPSCI_MAX_EPARAM];
#pragma unroll
    for (int k = 0; k < PPSCI_MAX_RES; ++k) lsum[k] = (wave == 0 && lane < PPSCI_TILE) ? lacc[k * PPSCI_TILE + lane] : 0.f;
#pragma unroll
    for (int k = 0; k < PPSCI_MAX_EPARAM; ++k) padj[k] = 0.f;
    epi_finale<EPI_RF_FUSED>(args.e, ered, lsum, padj);
  }
  if (args.t.external != 1) ppsci_step_tail(args.t, args.b.d, args.b.q, smem);
}

// ------------------------------------------------------------------------------------ host side
// the shape-specialised instantiation of this unit (PPSCI_FUSED_SPEC_D_RAW / _M, set by the .hip file; STATIC units only)
#if PPSCI_FUSED_STATIC && defined(PPSCI_FUSED_SPEC_D_RAW) && !defined(PPSCI_ABL_BUILD)
#define PPSCI_FUSED_HAS_SPEC 1
#define PPSCI_FUSED_SPEC_KERNEL (taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, true, 0, PPSCI_FUSED_SPEC_D_RAW, PPSCI_FUSED_SPEC_M>)
#else
#define PPSCI_FUSED_HAS_SPEC 0
#endif
// ... and its KEEP twin (PPSCI_FUSED_KEEP_PLANES, set by the .hip file), instantiated where ppsci_fused_keep_fits; not in the timer
// builds, whose per-phase sums live in `ered` during the tile loop
#if PPSCI_FUSED_HAS_SPEC && defined(PPSCI_FUSED_KEEP_PLANES) && PPSCI_FUSED_KEEP_PLANES && !defined(PPSCI_FUSED_TIMERS)
#define PPSCI_FUSED_HAS_KEEP 1
#define PPSCI_FUSED_KEEP_KERNEL (taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, true, 0, PPSCI_FUSED_SPEC_D_RAW, PPSCI_FUSED_SPEC_M, true>)
#else
#define PPSCI_FUSED_HAS_KEEP 0
#endif

template <int NB, int LH, int N1, int N2>
static int launch_fused(StepArgs& a, void* stream, int launch, int* grid_out) {
  constexpr int S = 1 + N1 + N2;
#if PPSCI_FUSED_HAS_SPEC
  constexpr int lds_spec = (int)(ppsci_fused_floats_spec<NB, LH, N1, N2, PPSCI_FUSED_SPEC_D_RAW, PPSCI_FUSED_SPEC_M>() * 4);
#endif
  if (launch == 2) {
#if PPSCI_FUSED_HAS_SPEC
    if (a.t.spec) {  // (chosen by the plan: the shape matches and no optional output is requested)
#if PPSCI_FUSED_HAS_KEEP
      if constexpr (ppsci_fused_keep_fits<NB, LH, N1, N2, PPSCI_FUSED_SPEC_D_RAW, PPSCI_FUSED_SPEC_M>()) {
        if (a.t.keep) PPSCI_LAUNCH(PPSCI_FUSED_KEEP_KERNEL, StepArgs, a.t.grid, 64 * NB, a.t.lds_keep, stream, a);
        else PPSCI_LAUNCH(PPSCI_FUSED_SPEC_KERNEL, StepArgs, a.t.grid, 64 * NB, lds_spec, stream, a);
      } else
#endif
      PPSCI_LAUNCH(PPSCI_FUSED_SPEC_KERNEL, StepArgs, a.t.grid, 64 * NB, lds_spec, stream, a);
      int e = PPSCI_LAST_LAUNCH_ERROR();
      if (e != 0) {
        ppsci_set_error("taylor_fused: launch failed (hip error %d)", e);
        return PPSCI_E_LAUNCH;
      }
      return PPSCI_OK;
    }
#endif
#ifdef PPSCI_ABL_BUILD
    {
      const char* ev = getenv("PPSCI_ABL");
      const int mask = ev ? atoi(ev) : 0;
#define PPSCI_ABL_CASE(M_)                                                                                                          \
  if (mask == (M_)) {                                                                                                               \
    PPSCI_SET_MAX_LDS((taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, PPSCI_FUSED_STATIC != 0, (M_)>), a.t.lds);                    \
    PPSCI_LAUNCH((taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, PPSCI_FUSED_STATIC != 0, (M_)>), StepArgs, a.t.grid, 64 * NB, a.t.lds, \
                 stream, a);                                                                                                        \
    return PPSCI_LAST_LAUNCH_ERROR() != 0 ? PPSCI_E_LAUNCH : PPSCI_OK;                                                              \
  }
      PPSCI_ABL_CASE(1) PPSCI_ABL_CASE(2) PPSCI_ABL_CASE(4) PPSCI_ABL_CASE(8) PPSCI_ABL_CASE(16) PPSCI_ABL_CASE(32) PPSCI_ABL_CASE(64)
      PPSCI_ABL_CASE(128) PPSCI_ABL_CASE(256) PPSCI_ABL_CASE(512)
#undef PPSCI_ABL_CASE
    }
#endif
    PPSCI_LAUNCH((taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, PPSCI_FUSED_STATIC != 0>), StepArgs, a.t.grid, 64 * NB, a.t.lds, stream, a);
    int e = PPSCI_LAST_LAUNCH_ERROR();
    if (e != 0) {
      ppsci_set_error("taylor_fused: launch failed (hip error %d)", e);
      return PPSCI_E_LAUNCH;
    }
    return PPSCI_OK;
  }
  const long long fl = ppsci_fused_floats(a.f.d, a.f.q, S, a.e.e.n_instr);
  if (fl * 4 > PPSCI_LDS_LIMIT_BYTES / 2) {  // two workgroups per CU
    ppsci_set_error("taylor_fused: LDS need %lld B exceeds half a CU", fl * 4);
    return PPSCI_E_UNSUPPORTED;
  }
  const int lds = (int)(fl * 4);
  if (PPSCI_SET_MAX_LDS((taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, PPSCI_FUSED_STATIC != 0>), lds) != 0) {
    ppsci_set_error("taylor_fused: cannot raise dynamic LDS to %d B", lds);
    return PPSCI_E_LAUNCH;
  }
  a.t.spec = a.t.spec_ok = a.t.keep = a.t.keep_ok = a.t.lds_keep = 0;
#if PPSCI_FUSED_HAS_SPEC
  // the shape-specialised kernel runs the plan's grid in no more LDS than planned; whether the plan takes it is decided once its
  // optional outputs are known (ppsci_taylor_step_plan)
  if (a.f.d.d_raw == PPSCI_FUSED_SPEC_D_RAW && a.f.q.d0 == PPSCI_FUSED_SPEC_D_RAW && a.f.d.d_out == PPSCI_FUSED_SPEC_M && lds_spec <= lds &&
      PPSCI_SET_MAX_LDS(PPSCI_FUSED_SPEC_KERNEL, lds_spec) == 0)
    a.t.spec_ok = 1;
#endif
  int per_cu = 1;
  if (PPSCI_OCCUPANCY((taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, PPSCI_FUSED_STATIC != 0>), 64 * NB, lds, &per_cu) != 0 || per_cu < 1) per_cu = 1;
#if PPSCI_FUSED_HAS_KEEP
  // The KEEP kernel needs MORE LDS than planned: it is taken only if as many of its workgroups share a CU as the grid below is
  // computed from -- grid, iters and workspace rows are those of the plan either way.
  if constexpr (ppsci_fused_keep_fits<NB, LH, N1, N2, PPSCI_FUSED_SPEC_D_RAW, PPSCI_FUSED_SPEC_M>()) {
    constexpr int lds_keep = (int)(ppsci_fused_floats_spec<NB, LH, N1, N2, PPSCI_FUSED_SPEC_D_RAW, PPSCI_FUSED_SPEC_M, true>() * 4);
    int pc = 0;
    if (a.t.spec_ok && PPSCI_SET_MAX_LDS(PPSCI_FUSED_KEEP_KERNEL, lds_keep) == 0 &&
        PPSCI_OCCUPANCY(PPSCI_FUSED_KEEP_KERNEL, 64 * NB, lds_keep, &pc) == 0 && pc == per_cu) {
      a.t.keep_ok = 1;
      a.t.lds_keep = lds_keep;
    }
  }
#endif
  const int ntl = a.f.ntiles;
  int grid = ntl < PPSCI_NUM_CU * per_cu ? ntl : PPSCI_NUM_CU * per_cu;
  if (ppsci_get_max_grid() > 0 && grid > ppsci_get_max_grid()) grid = ppsci_get_max_grid();
  if (grid < 1) grid = 1;
  a.f.iters = a.b.iters = a.e.iters = (ntl + grid - 1) / grid;
  a.f.tile0 = a.b.tile0 = 0;
  a.f.resident = a.b.resident = 1;
  a.b.accum = 1;
  a.b.xdl_split = 1;
  a.t.grid = grid;
  a.t.lds = lds;
  a.t.fused = 1;
  if (grid_out) *grid_out = grid;
  if (!launch) return PPSCI_OK;
  PPSCI_LAUNCH((taylor_fused_kernel<NB, LH, N1, N2, PPSCI_ACT_ID, PPSCI_FUSED_STATIC != 0>), StepArgs, grid, 64 * NB, lds, stream, a);
  int e = PPSCI_LAST_LAUNCH_ERROR();
  if (e != 0) {
    ppsci_set_error("taylor_fused: launch failed (hip error %d)", e);
    return PPSCI_E_LAUNCH;
  }
  return PPSCI_OK;
}

template <int N1, int N2, class... Ps>
static constexpr bool fused_has_static(epi_typelist<Ps...>) {
  return (false || ... || (Ps::N1 == N1 && Ps::N2 == N2));
}

template <int NB, int N1, int N2>
static int run_fused(StepArgs& a, void* stream, int launch, int* grid_out) {
  if constexpr (PPSCI_FUSED_STATIC != 0 && !fused_has_static<N1, N2>(EpiStaticPrograms{})) return PPSCI_E_UNSUPPORTED;
  else
  switch (a.f.d.n_hidden) {
    case 2: return launch_fused<NB, 2, N1, N2>(a, stream, launch, grid_out);
    case 3: return launch_fused<NB, 3, N1, N2>(a, stream, launch, grid_out);
    case 4: return launch_fused<NB, 4, N1, N2>(a, stream, launch, grid_out);
    case 5: return launch_fused<NB, 5, N1, N2>(a, stream, launch, grid_out);
    default: return PPSCI_E_UNSUPPORTED;
  }
}

// PPSCI_E_UNSUPPORTED (without an error message): this net / stream set has no fused tile kernel
int PPSCI_FUSED_RUN_NAME(StepArgs& a, void* stream, int launch, int* grid_out) {
#define PPSCI_FUSED_CASE(NB_, N1_, N2_) \
  if (a.f.q.NB == NB_ && a.f.d.n1 == N1_ && a.f.d.n2 == N2_ && a.f.d.n3 == 0) return run_fused<NB_, N1_, N2_>(a, stream, launch, grid_out);
  if (a.f.d.fourier_half > 0 || a.f.d.n_hidden < 2 || a.f.d.n_hidden > 5 || a.f.d.d_raw > PPSCI_FUSED_MAX_IN) return PPSCI_E_UNSUPPORTED;
#ifdef PPSCI_FUSED_ONLY_AC  // one-kernel translation unit for resource-usage experiments (tools/resource_usage.py)
  if (a.f.d.n_hidden == 4 && a.f.d.n1 == 2 && a.f.d.n2 == 1) return launch_fused<4, 4, 2, 1>(a, stream, launch, grid_out);
#else
  PPSCI_FUSED_CASE(4, 0, 0) PPSCI_FUSED_CASE(4, 1, 1) PPSCI_FUSED_CASE(4, 2, 0) PPSCI_FUSED_CASE(4, 2, 1) PPSCI_FUSED_CASE(4, 2, 2)
#endif
#undef PPSCI_FUSED_CASE
  return PPSCI_E_UNSUPPORTED;
}
