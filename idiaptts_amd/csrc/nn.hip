// Dense acoustic-model kernels for gfx950: fp32 MFMA GEMM with fused epilogues, masked MSE,
// Adam.  Replaces the torch.nn.Linear / Tanh / MSELoss / torch.optim.Adam calls the reference
// makes per mini-batch (rnn_dyn/FFWrapper.py:63-73, loss/NamedLoss.py:70-117,
// ModularModelHandlerPyTorch.py:769-820).
//
// GEMMs (exact fp32: v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD = 157 TFLOP/s chip peak): the LDS-DMA
// ring kernel (gemm_ring.h) takes every call whose operands allow 16-byte rows; the register-staged
// kernel gemm_f32_kernel (its body in gemm_staged.h, shared with conv1d.hip) takes the rest, as a
// 128x128 double-buffered tile or a 128x64 tile with a single LDS stage (36.9 KB, 106 VGPRs -> 4
// workgroups per CU) -- see launch_gemm for which runs when.
//   * roofline: MFMA fp32.  FLOPs per valid frame of the 425-512-512-187 model: fwd 1.15 M,
//     fwd+bwd 3.45 M (first-layer input gradient skipped: 3.01 M) -- SURVEY.md section 8d.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "common.h"
#include "gemm_ring.h"
#include "gemm_staged.h"

namespace itts {

constexpr int BN = 128;  // widest tile of the register-staged kernel (TN = 2)

// Global -> registers for one 128(out) x 32(k) tile of an operand, 16 floats per thread.
// Branch-free: out-of-range elements read a clamped (valid) address and are zeroed by a select,
// so all loads of a tile are issued back to back (hipcc otherwise branches around every guarded
// load and waits for each one).  VEC: 16-byte loads; requires ld % 4 == 0 and a 16-B aligned base.
// When the contiguous extent (K for row form, out_dim for col form) is not a multiple of 4 the
// last float4 of a row also reads the 1-3 pad elements between the extent and the pitch: pad
// output columns are never stored, pad K elements meet a zero of the other operand -- so the pad
// only has to be finite (callers keep it zero; see the pitch rule in include/idiaptts_amd.h).
template <bool ROWFORM, bool VEC, int NROWS>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, int64_t ld, int64_t out0,
                                          int64_t out_dim, int64_t k0, int64_t k_end,
                                          float4 (&r)[NROWS / 32]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NROWS / 32; ++i) {
    const int idx = tid + 256 * i;
    int64_t o, k;
    if (ROWFORM) {
      o = out0 + (idx >> 3);
      k = k0 + ((idx & 7) << 2);
    } else {
      k = k0 + idx / (NROWS / 4);
      o = out0 + ((idx % (NROWS / 4)) << 2);
    }
    // contiguous index c (4 consecutive elements), strided index t
    const int64_t c = ROWFORM ? k : o, c_end = ROWFORM ? k_end : out_dim;
    const int64_t t = ROWFORM ? o : k, t_end = ROWFORM ? out_dim : k_end;
    const bool t_ok = t < t_end;
    const int64_t tc = t_ok ? t : 0;
    if (VEC) {
      const bool ok = t_ok && (c < c_end);
      const float4 v = *reinterpret_cast<const float4*>(P + tc * ld + (ok ? c : 0));
      r[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const float* row = P + tc * ld;
      const bool k0ok = t_ok && c < c_end, k1ok = t_ok && c + 1 < c_end, k2ok = t_ok && c + 2 < c_end,
                 k3ok = t_ok && c + 3 < c_end;
      const float a0 = row[k0ok ? c : 0], a1 = row[k1ok ? c + 1 : 0], a2 = row[k2ok ? c + 2 : 0],
                  a3 = row[k3ok ? c + 3 : 0];
      r[i] = make_float4(k0ok ? a0 : 0.f, k1ok ? a1 : 0.f, k2ok ? a2 : 0.f, k3ok ? a3 : 0.f);
    }
  }
}

template <bool A_ROW, bool B_ROW, bool VEC_A, bool VEC_B>
struct DenseLoader {
  const GemmArgs& g;
  template <int NROWS>
  __device__ __forceinline__ void load_a(int64_t out0, int64_t k0, int64_t k_end, float4 (&r)[NROWS / 32]) const {
    load_tile<A_ROW, VEC_A, NROWS>(g.A, g.lda, out0, g.M, k0, k_end, r);
  }
  template <int NROWS>
  __device__ __forceinline__ void load_b(int64_t out0, int64_t k0, int64_t k_end, float4 (&r)[NROWS / 32]) const {
    load_tile<B_ROW, VEC_B, NROWS>(g.B, g.ldb, out0, g.N, k0, k_end, r);
  }
};

// TN = MFMA tiles per wave along N: output tile 128 x (64*TN). TN = 1 halves the tile so that
// narrow outputs (N = 187) and awkward tile counts waste fewer workgroup slots.  AF: activation family.
// DR: the dropout rule of the EPI_BIAS_ACT / EPI_DACT epilogue (dropout.h), or NoDrop.
template <bool A_ROW, bool B_ROW, int EPI, bool VEC_A, bool VEC_B, int TN, int STAGES, int AF, class DR>
__device__ __forceinline__ void gemm_f32_body(const GemmArgs& g, float* lds, const DR& dr) {
  f32x16 acc[2][TN];
  const StagedTile t =
      staged_gemm_tile<A_ROW, B_ROW, TN, STAGES>(g, DenseLoader<A_ROW, B_ROW, VEC_A, VEC_B>{g}, lds, acc);
  const int64_t m0 = t.m0;
  const int n0 = t.n0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  // C/D map of 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* C = g.C + (int64_t)blockIdx.z * g.slab_stride;
  const int cl = lane & 31, rh = lane >> 5;
  if (EPI == EPI_MSE) {
    // Last layer of a training step: y = acc + bias never goes to memory; the masked difference to
    // the target (aux) is squared into the workgroup's partial sum and scaled into C as
    // d loss / d y (masked_mse_kernel's arithmetic: double accumulation of float differences).
    float* stage = lds + wid * (32 * 36);
    const int c4 = (lane & 7) << 2, rq = lane >> 3;
    const int colb = n0 + wn * 32;
    double lsum = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i > 0) {   // the reads of the previous block are done before it is overwritten
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * rh) * 36 + cl] = acc[i][0][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the lanes of this wave exchange the block through LDS
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int col = colb + c4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rl = rq + 8 * q;
        const int64_t row = m0 + wm * 64 + i * 32 + rl;
        const float4 v = *reinterpret_cast<const float4*>(stage + rl * 36 + c4);
        if (row >= g.M || col >= g.N) continue;
        const bool ok = g.row_valid[row] != 0;
        const float vv[4] = {v.x, v.y, v.z, v.w};
        float dz[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float diff = 0.f;
          if (col + e < g.N && ok)
            diff = (vv[e] + (g.bias ? g.bias[col + e] : 0.f)) - g.aux[row * g.ldaux + col + e];
          lsum += (double)diff * (double)diff;
          dz[e] = g.gscale * diff;
        }
        if (col + 3 < g.N) {
          *reinterpret_cast<float4*>(C + row * g.ldc + col) = make_float4(dz[0], dz[1], dz[2], dz[3]);
        } else {
          for (int e = 0; e < 4 && col + e < g.N; ++e) C[row * g.ldc + col + e] = dz[e];
        }
      }
    }
    __shared__ double mse_red[16];
    lsum = block_sum(lsum, mse_red);
    if (threadIdx.x == 0) g.loss_partial[blockIdx.x] = lsum;
    return;
  }
  if (STAGES == 1 && TN == 1 && g.wide_out) {
    // Wide stores: a wave passes each of its 32 x 32 result blocks through its own 4.6 KB of the
    // (now idle) LDS tile and writes rows back as float4 -- 8 store instructions of whole 128-byte
    // row segments per thread instead of 32 dword stores; bias / activation / derivative are applied
    // four columns at a time on the way out.  (The loop's last barrier has retired all tile reads;
    // the staging area is private to the wave, LDS operations of a wave execute in order.)
    float* stage = lds + wid * (32 * 36);
    const int c4 = (lane & 7) << 2, rq = lane >> 3;
    const int colb = n0 + wn * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i > 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * rh) * 36 + cl] = acc[i][0][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the lanes of this wave exchange the block through LDS
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int col = colb + c4;
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      const bool full = col + 3 < g.N;
      if (EPI == EPI_BIAS_ACT && g.bias && full) bv = *reinterpret_cast<const float4*>(g.bias + col);
      uint32_t keep = 0;   // the keep bits of the lane's four float4, ahead of the arithmetic (registers)
      if constexpr (DR::on) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          keep |= dr.keep_bits(m0 + wm * 64 + i * 32 + rq + 8 * q, col) << (4 * q);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rl = rq + 8 * q;
        const int64_t row = m0 + wm * 64 + i * 32 + rl;
        float4 v = *reinterpret_cast<const float4*>(stage + rl * 36 + c4);
        if (row >= g.M || col >= g.N) continue;
        const uint32_t kb = keep >> (4 * q);
        if (full) {
          if (EPI == EPI_BIAS_ACT) {
            v.x = act_fwd_af<AF>(v.x + bv.x, g.act); v.y = act_fwd_af<AF>(v.y + bv.y, g.act);
            v.z = act_fwd_af<AF>(v.z + bv.z, g.act); v.w = act_fwd_af<AF>(v.w + bv.w, g.act);
            if constexpr (DR::on) {
              v.x = dr.apply_bit(v.x, kb & 1u); v.y = dr.apply_bit(v.y, kb & 2u);
              v.z = dr.apply_bit(v.z, kb & 4u); v.w = dr.apply_bit(v.w, kb & 8u);
            }
          }
          if constexpr (EPI == EPI_DACT && DR::on) {
            const float4 a = *reinterpret_cast<const float4*>(g.aux + row * g.ldaux + col);
            v.x = (kb & 1u) ? v.x * (dr.scale * act_grad_af<AF>(a.x * dr.keep, g.act)) : 0.f;
            v.y = (kb & 2u) ? v.y * (dr.scale * act_grad_af<AF>(a.y * dr.keep, g.act)) : 0.f;
            v.z = (kb & 4u) ? v.z * (dr.scale * act_grad_af<AF>(a.z * dr.keep, g.act)) : 0.f;
            v.w = (kb & 8u) ? v.w * (dr.scale * act_grad_af<AF>(a.w * dr.keep, g.act)) : 0.f;
          }
          if (EPI == EPI_DACT && !DR::on) {
            const float4 a = *reinterpret_cast<const float4*>(g.aux + row * g.ldaux + col);
            v.x *= act_grad_af<AF>(a.x, g.act); v.y *= act_grad_af<AF>(a.y, g.act);
            v.z *= act_grad_af<AF>(a.z, g.act); v.w *= act_grad_af<AF>(a.w, g.act);
          }
          *reinterpret_cast<float4*>(C + row * g.ldc + col) = v;
        } else {   // the float4 that straddles N: column by column
          const float vv[4] = {v.x, v.y, v.z, v.w};
          for (int e = 0; e < 4 && col + e < g.N; ++e) {
            float o = vv[e];
            if (EPI == EPI_BIAS_ACT) o = act_fwd_af<AF>(o + (g.bias ? g.bias[col + e] : 0.f), g.act);
            if constexpr (DR::on) {
              if (EPI == EPI_BIAS_ACT) o = dr.apply_bit(o, (kb >> e) & 1u);
              if (EPI == EPI_DACT)
                o = ((kb >> e) & 1u)
                        ? o * (dr.scale * act_grad_af<AF>(g.aux[row * g.ldaux + col + e] * dr.keep, g.act))
                        : 0.f;
            } else {
              if (EPI == EPI_DACT) o *= act_grad_af<AF>(g.aux[row * g.ldaux + col + e], g.act);
            }
            C[row * g.ldc + col + e] = o;
          }
        }
      }
    }
    return;
  }
  staged_epilogue<EPI, TN, AF>(g, t, acc, [](int64_t m) { return m; }, dr);
}

template <bool A_ROW, bool B_ROW, int EPI, bool VEC_A, bool VEC_B, int TN, int STAGES = 2, int AF = AF_BASE>
__global__ __launch_bounds__(256, STAGES == 1 ? 4 : 2) void gemm_f32_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[staged_lds_floats<B_ROW, TN, STAGES>()];
  gemm_f32_body<A_ROW, B_ROW, EPI, VEC_A, VEC_B, TN, STAGES, AF>(g, lds, NoDrop{});
}

// The single-stage row-form kernel with a dropout rule in its epilogue: a kernel of its own, so that the one above
// keeps its arguments and its code.
template <bool B_ROW, int EPI, bool VEC_A, bool VEC_B, int AF>
__global__ __launch_bounds__(256, 4) void gemm_f32_drop_kernel(GemmArgs g, DropRule dr) {
  __shared__ __attribute__((aligned(16))) float lds[staged_lds_floats<B_ROW, 1, 1>()];
  gemm_f32_body<true, B_ROW, EPI, VEC_A, VEC_B, 1, 1, AF>(g, lds, dr);
}

// Which kernel the dense-layer products of this process ran on, per epilogue kind (itts_gemm_path_counts): [0][epi] the
// LDS-DMA ring kernel (a pair launch counts its two products), [1][epi] the register-staged kernel.
static std::atomic<int64_t> g_gemm_path[2][4];

// What the last dense call of this host thread launched (itts_gemm_last_plan): every entry is written at its launch
// site from the template parameters and arguments of that launch.  A dense entry point opens the record (PlanScope);
// launches made for other callers (conv1d.hip and rnn.hip reduce their slabs here too) leave it alone.
constexpr int kPlanMax = 8, kPlanInts = 16;
enum { PLAN_STAGED = 1, PLAN_RING = 2, PLAN_RING_PAIR = 3, PLAN_REDUCE = 4 };
struct GemmPlan {
  int32_t e[kPlanMax][kPlanInts];
  int n;       // entries appended (those beyond kPlanMax are counted, not kept)
  int depth;   // open dense entry points (itts_linear_bwd calls the two separate ones)
};
static thread_local GemmPlan t_plan{};

struct PlanScope {
  PlanScope() { if (t_plan.depth++ == 0) t_plan.n = 0; }
  ~PlanScope() { --t_plan.depth; }
};

static void plan_gemm(int kernel, bool a_row, bool b_row, int epi, int tn, int stages, int wm, bool va, bool vb,
                      bool wide, bool grouped, int splitk, int af, int64_t tiles, int64_t grid, bool drop = false) {
  if (t_plan.depth == 0) return;
  if (t_plan.n < kPlanMax) {
    const int32_t v[kPlanInts] = {kernel, a_row, b_row, epi, tn, stages, wm, va, vb, wide, grouped, splitk, af,
                                  (int32_t)std::min<int64_t>(tiles, INT32_MAX), (int32_t)grid, drop};
    std::copy(v, v + kPlanInts, t_plan.e[t_plan.n]);
  }
  ++t_plan.n;
}

static void plan_reduce(bool vec, bool merged, bool deferred, int S) {
  if (t_plan.depth == 0) return;
  if (t_plan.n < kPlanMax) {
    const int32_t v[kPlanInts] = {PLAN_REDUCE, vec, merged, deferred, S};
    std::copy(v, v + kPlanInts, t_plan.e[t_plan.n]);
  }
  ++t_plan.n;
}

template <bool A_ROW, bool B_ROW, int EPI, int TN, int STAGES, int AF = AF_BASE, class DR = NoDrop>
static int launch_gemm_tn(const GemmArgs& g, int splitk, hipStream_t s, const DR& dr = DR()) {
  g_gemm_path[1][EPI].fetch_add(1, std::memory_order_relaxed);
  const int64_t tiles = ((g.M + BM - 1) / BM) * ((g.N + 64 * TN - 1) / (64 * TN));
  dim3 grid((unsigned)tiles, 1, (unsigned)splitk);
  const bool va = g.vecA, vb = g.vecB;   // pitch and alignment allow 16-byte loads (see load_tile)
  // (the wide-store branch of gemm_f32_kernel: behind the EPI_MSE epilogue, single-stage 128 x 64 tiles only)
  plan_gemm(PLAN_STAGED, A_ROW, B_ROW, EPI, TN, STAGES, 0, va, vb, EPI != EPI_MSE && STAGES == 1 && TN == 1 && g.wide_out,
            false, splitk, AF, tiles * splitk, tiles * splitk, DR::on);
  if constexpr (DR::on) {
    static_assert(A_ROW && TN == 1 && STAGES == 1, "the dropout epilogue exists on the single-stage row-form kernel");
    if (va && vb)
      hipLaunchKernelGGL((gemm_f32_drop_kernel<B_ROW, EPI, true, true, AF>), grid, dim3(256), 0, s, g, dr);
    else if (va)
      hipLaunchKernelGGL((gemm_f32_drop_kernel<B_ROW, EPI, true, false, AF>), grid, dim3(256), 0, s, g, dr);
    else if (vb)
      hipLaunchKernelGGL((gemm_f32_drop_kernel<B_ROW, EPI, false, true, AF>), grid, dim3(256), 0, s, g, dr);
    else
      hipLaunchKernelGGL((gemm_f32_drop_kernel<B_ROW, EPI, false, false, AF>), grid, dim3(256), 0, s, g, dr);
    ITTS_LAUNCH_CHECK();
    return ITTS_OK;
  }
  if (va && vb)
    hipLaunchKernelGGL((gemm_f32_kernel<A_ROW, B_ROW, EPI, true, true, TN, STAGES, AF>), grid, dim3(256), 0, s, g);
  else if (va)
    hipLaunchKernelGGL((gemm_f32_kernel<A_ROW, B_ROW, EPI, true, false, TN, STAGES, AF>), grid, dim3(256), 0, s, g);
  else if (vb)
    hipLaunchKernelGGL((gemm_f32_kernel<A_ROW, B_ROW, EPI, false, true, TN, STAGES, AF>), grid, dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((gemm_f32_kernel<A_ROW, B_ROW, EPI, false, false, TN, STAGES, AF>), grid, dim3(256), 0, s, g);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// Kernel shape choice.  Measured on the acoustic-model GEMMs (MI355X, MfmaUtil from rocprofv3):
//   * row-form A (forward and input-gradient GEMMs: M = frames, short K): 128x64 tiles with ONE LDS
//     stage -- 37 KB and 106 VGPRs, so 4 workgroups per CU instead of 2.  Twice the waves per SIMD
//     cover the barrier / LDS-refill gaps of a K tile: +21 % per-tile rate over the double-buffered
//     128x128 kernel although it needs two barriers per K tile.
//   * col-form A (weight-gradient GEMMs, split-K, long K loops): double-buffered tiles; 128x128
//     reuses operands best, 128x64 quantises better onto the 512 resident slots (256 CUs x 2) and
//     wastes less on narrow outputs -- pick by the slot-quantisation estimate below.  (The
//     single-stage variant spills in col form and is slower.)
static double tile_efficiency(int64_t M, int N, int splitk, int tn, double loop_eff) {
  const int bn = 64 * tn;
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + bn - 1) / bn) * splitk;
  const int64_t rounds = (tiles + 511) / 512;
  const double useful = (double)N / (double)(((N + bn - 1) / bn) * bn);
  return loop_eff * useful * (double)tiles / (double)(rounds * 512);
}

// ---- the LDS-DMA ring kernel (gemm_ring.h) -----------------------------------------------------
// Takes every call whose operands allow 16-byte row accesses (the trainer's buffers all do); the
// register-staged kernel above stays the general path (odd pitches, unaligned bases).
constexpr int kRingGrid = 512;   // persistent workgroups: 2 per CU

template <bool A_ROW, bool B_ROW>
static bool ring_ok(const GemmArgs& g, int splitk, int epi) {
  if (!g.vecA || !g.vecB) return false;
  if (g.lda % 4 || g.ldb % 4 || g.ldc % 4 || g.slab_stride % 4 || !aligned16(g.C)) return false;
  if (epi == EPI_DACT && (g.ldaux % 4 || !aligned16(g.aux))) return false;   // the MSE target is read dword-wise
  const int64_t lim = (int64_t)1 << 30;   // 32-bit byte offsets inside the buffer descriptors
  if (g.M >= lim || g.K >= lim || g.lda >= lim / 256 || g.ldb >= lim / 256 || g.ldc >= lim / 256 ||
      g.ldaux >= lim / 256)
    return false;
  if (!A_ROW && (g.kchunk + 32) * g.lda >= lim) return false;
  if (!B_ROW && (g.kchunk + 32) * g.ldb >= lim) return false;
  if (splitk > 1 && g.kchunk % 32) return false;
  return true;
}

static int ring_group(int tiles_n, int bnt, int64_t K, bool row_row);

template <int WM>
static ring::Args ring_args(const GemmArgs& g, int splitk) {
  constexpr int BMT = 64 * WM, BNT = 32 * (4 / WM);
  ring::Args r{};
  r.A = g.A; r.B = g.B; r.C = g.C; r.bias = g.bias; r.aux = g.aux;
  r.row_valid = g.row_valid; r.loss_partial = g.loss_partial; r.bias_part = g.bias_part;
  r.slab_stride = g.slab_stride; r.bias_part_stride = g.bias_part_stride;
  r.lda = (int)g.lda; r.ldb = (int)g.ldb; r.ldc = (int)g.ldc; r.ldaux = (int)g.ldaux;
  r.M = (int)g.M; r.N = g.N; r.K = (int)g.K; r.kchunk = (int)g.kchunk; r.splitk = splitk;
  r.tiles_m = (int)((g.M + BMT - 1) / BMT);
  r.tiles_n = (g.N + BNT - 1) / BNT;
  r.gn = r.tiles_n;
  r.act = g.act; r.gscale = g.gscale;
  return r;
}

template <bool A_ROW, bool B_ROW, int EPI, int WM, int AF = AF_BASE, class DR = NoDrop>
static int launch_ring_wm(const GemmArgs& g, int splitk, hipStream_t s, const DR& dr = DR()) {
  constexpr int BNT = 32 * (4 / WM);
  g_gemm_path[0][EPI].fetch_add(1, std::memory_order_relaxed);
  ring::Args r = ring_args<WM>(g, splitk);
  r.gn = ring_group(r.tiles_n, BNT, g.K, A_ROW && B_ROW);
  const int64_t ntiles = (int64_t)r.tiles_m * r.tiles_n * splitk;
  ITTS_REQUIRE(ntiles < ((int64_t)1 << 31), "too many tiles");
  const int grid = (int)std::min<int64_t>(kRingGrid, (ntiles + 7) / 8 * 8);
  // (the dropout kernels walk the plain order: the products that gain from groups, the recurrent layers' input
  // projections, carry no dropout of this kind)
  const bool grouped = !DR::on && A_ROW && B_ROW && EPI == ring::EPI_BIAS_ACT && r.gn < r.tiles_n;
  plan_gemm(PLAN_RING, A_ROW, B_ROW, EPI, 0, 0, WM, true, true, false, grouped, splitk, AF, ntiles, grid, DR::on);
  if constexpr (DR::on) {
    hipLaunchKernelGGL((ring::gemm_ring_drop_kernel<A_ROW, B_ROW, EPI, WM, AF>), dim3(grid), dim3(ring::THREADS), 0, s, r,
                       dr);
    ITTS_LAUNCH_CHECK();
    return ITTS_OK;
  }
  if (grouped)
    hipLaunchKernelGGL((ring::gemm_ring_kernel<A_ROW, B_ROW, EPI, WM, A_ROW && B_ROW && EPI == ring::EPI_BIAS_ACT, AF>),
                       dim3(grid), dim3(ring::THREADS), 0, s, r);
  else
    hipLaunchKernelGGL((ring::gemm_ring_kernel<A_ROW, B_ROW, EPI, WM, false, AF>), dim3(grid), dim3(ring::THREADS), 0, s, r);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// Column tiles per group of the tile order (ring::decode_tile).  Forward products (row x row) whose weight
// matrix is larger than an XCD's L2 -- the recurrent layers' [4096 x 1024] input projections, 16 MB -- walk
// groups of ~4 MB of weight panels (4.78 -> 4.54 ms for 73 138 rows, scripts/ring_order_probe.py); every
// other product keeps one group (the weight-gradient products measured 2-3 % slower in groups).
static int ring_group(int tiles_n, int bnt, int64_t K, bool row_row) {
  if (!row_row) return tiles_n;
  const int64_t panel = (int64_t)bnt * K * 4;
  const int64_t gn = std::max<int64_t>(1, ((int64_t)4 << 20) / std::max<int64_t>(panel, 1));
  return (int)std::min<int64_t>(gn, tiles_n);
}

// tile shape of the ring kernel for an [M x N] output: 128 x 64 or 64 x 128, whichever wastes less
static int ring_wm(int64_t M, int N) {
  const double w2 = (double)(((M + 127) / 128) * 128) * (double)(((N + 63) / 64) * 64);
  const double w1 = (double)(((M + 63) / 64) * 64) * (double)(((N + 127) / 128) * 128);
  return w1 < w2 ? 1 : 2;
}

template <bool A_ROW, bool B_ROW, int EPI, int AF, class DR = NoDrop>
static int launch_ring(const GemmArgs& g, int splitk, hipStream_t s, const DR& dr = DR()) {
  if (ring_wm(g.M, g.N) == 1) return launch_ring_wm<A_ROW, B_ROW, EPI, 1, AF, DR>(g, splitk, s, dr);
  return launch_ring_wm<A_ROW, B_ROW, EPI, 2, AF, DR>(g, splitk, s, dr);
}

// weight-gradient GEMM (col x col, split-K slabs) and input-gradient GEMM (row x col, activation
// derivative in the epilogue) of one layer in ONE launch
template <int WM_W, int EPI_X, int AF_X = AF_BASE, class DR = NoDrop>
static int launch_ring_bwd_pair(const GemmArgs& gw, int splitk, const GemmArgs& gx, hipStream_t s, const DR& dr = DR()) {
  g_gemm_path[0][EPI_STORE].fetch_add(1, std::memory_order_relaxed);
  g_gemm_path[0][EPI_X].fetch_add(1, std::memory_order_relaxed);
  const ring::Args rw = ring_args<WM_W>(gw, splitk), rx = ring_args<2>(gx, 1);
  plan_gemm(PLAN_RING_PAIR, false, false, EPI_STORE, 0, 0, WM_W, true, true, false, false, splitk, AF_BASE,
            (int64_t)rw.tiles_m * rw.tiles_n * splitk, kRingGrid);
  plan_gemm(PLAN_RING_PAIR, true, false, EPI_X, 0, 0, 2, true, true, false, false, 1, AF_X,
            (int64_t)rx.tiles_m * rx.tiles_n, kRingGrid, DR::on);
  if constexpr (DR::on) {
    static_assert(EPI_X == EPI_DACT, "the dropout pair is the one with the activation derivative");
    hipLaunchKernelGGL((ring::gemm_ring_pair_drop_kernel<WM_W, AF_X>), dim3(kRingGrid), dim3(ring::THREADS), 0, s, rw, rx,
                       dr);
    ITTS_LAUNCH_CHECK();
    return ITTS_OK;
  }
  hipLaunchKernelGGL((ring::gemm_ring_pair_kernel<false, false, EPI_STORE, WM_W, true, false, EPI_X, 2, AF_X>),
                     dim3(kRingGrid), dim3(ring::THREADS), 0, s, rw, rx);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

template <bool A_ROW, bool B_ROW, int EPI, int AF = AF_BASE, class DR = NoDrop>
static int launch_gemm(GemmArgs g, int splitk, hipStream_t s, const DR& dr = DR()) {
  if (g.M <= 0 || g.N <= 0) return ITTS_OK;
  if (ring_ok<A_ROW, B_ROW>(g, splitk, EPI)) return launch_ring<A_ROW, B_ROW, EPI, AF, DR>(g, splitk, s, dr);
  if constexpr (DR::on) return launch_gemm_tn<A_ROW, B_ROW, EPI, 1, 1, AF, DR>(g, splitk, s, dr);
  if (A_ROW) return launch_gemm_tn<A_ROW, B_ROW, EPI, 1, 1, AF>(g, splitk, s);
  const double e2 = tile_efficiency(g.M, g.N, splitk, 2, 1.0);
  const double e1 = tile_efficiency(g.M, g.N, splitk, 1, 0.90);
  if (e1 > e2) return launch_gemm_tn<A_ROW, B_ROW, EPI, 1, 2, AF>(g, splitk, s);
  return launch_gemm_tn<A_ROW, B_ROW, EPI, 2, 2, AF>(g, splitk, s);
}


// ---- split-K slab reduction (deterministic order) -------------------------------------------
// out[i] = sum_z slabs[z][i].  Memory bound (S x n floats in, n out); a workgroup owns 64 float4
// columns, its 4 waves take every 4th slab each (all loads of a thread independent -> in flight
// together) and the four partial sums meet in LDS in a fixed order.  n % 4 == 0 and 16-byte
// aligned buffers take this path, anything else the scalar tail kernel.
__device__ __forceinline__ void reduce_slabs_vec_body(const float* __restrict__ slabs, int S, int64_t n,
                                                      float* __restrict__ out, int accumulate, int64_t block,
                                                      float4 (*part)[64]) {
  const int tx = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t n4 = n >> 2;
  const int64_t c = block * 64 + tx;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < n4) {
    const float4* p = reinterpret_cast<const float4*>(slabs) + c;
#pragma unroll 8
    for (int z = grp; z < S; z += 4) {
      const float4 v = p[(int64_t)z * n4];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  if (grp > 0) part[grp - 1][tx] = s;
  __syncthreads();
  if (grp == 0 && c < n4) {
#pragma unroll
    for (int g2 = 0; g2 < 3; ++g2) {
      const float4 v = part[g2][tx];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float4* o = reinterpret_cast<float4*>(out) + c;
    if (accumulate) {
      const float4 v = *o;
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *o = s;
  }
}

// same split of the work for buffers that cannot be read as float4 (n % 4 != 0, e.g. 187 biases)
__device__ __forceinline__ void reduce_slabs_scalar_body(const float* __restrict__ slabs, int S, int64_t n,
                                                         float* __restrict__ out, int accumulate,
                                                         int64_t block, float (*part)[64]) {
  const int tx = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t c = block * 64 + tx;
  float s = 0.f;
  if (c < n) {
#pragma unroll 8
    for (int z = grp; z < S; z += 4) s += slabs[(int64_t)z * n + c];
  }
  if (grp > 0) part[grp - 1][tx] = s;
  __syncthreads();
  if (grp == 0 && c < n) {
    s += part[0][tx];
    s += part[1][tx];
    s += part[2][tx];
    out[c] = accumulate ? out[c] + s : s;
  }
}

__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ slabs, int S,
                                                           int64_t n, float* __restrict__ out,
                                                           int accumulate) {
  __shared__ float4 part[3][64];
  reduce_slabs_vec_body(slabs, S, n, out, accumulate, blockIdx.x, part);
}

__global__ __launch_bounds__(256) void reduce_slabs_scalar_kernel(const float* __restrict__ slabs, int S,
                                                                  int64_t n, float* __restrict__ out,
                                                                  int accumulate) {
  __shared__ float part[3][64];
  reduce_slabs_scalar_body(slabs, S, n, out, accumulate, blockIdx.x, part);
}

// Several reductions in ONE launch (itts_defer_reductions / itts_reduce_deferred): a training step
// owes one slab reduction per layer (plus odd-sized bias vectors and the loss partial sums), each a
// 5 us launch of its own that the next GEMM then waits for; queued, they run as segments of one
// grid.  Same arithmetic per element as the single kernels above (bit-identical results).
constexpr int kMaxDeferred = 16;
struct ReduceSeg {
  const void* src;      // slabs (float) or partial sums (double, kind 2)
  void* out;
  int64_t n;            // floats per slab / number of partial sums
  double scale;         // kind 2
  int S;
  int accumulate;
  int kind;             // 0: float4 columns, 1: scalar columns, 2: sum of doubles -> one float
  int first_block;
};
struct ReduceMulti {
  ReduceSeg seg[kMaxDeferred];
  int nseg;
};

__global__ __launch_bounds__(256) void reduce_multi_kernel(ReduceMulti d) {
  __shared__ float4 part4[3][64];
  __shared__ double red[16];
  int i = 0;
  while (i + 1 < d.nseg && (int)blockIdx.x >= d.seg[i + 1].first_block) ++i;
  const ReduceSeg& g = d.seg[i];
  const int64_t block = (int64_t)blockIdx.x - g.first_block;
  if (g.kind == 0) {
    reduce_slabs_vec_body(static_cast<const float*>(g.src), g.S, g.n, static_cast<float*>(g.out), g.accumulate,
                          block, part4);
  } else if (g.kind == 1) {
    reduce_slabs_scalar_body(static_cast<const float*>(g.src), g.S, g.n, static_cast<float*>(g.out),
                             g.accumulate, block, reinterpret_cast<float (*)[64]>(part4));
  } else {
    const double* partial = static_cast<const double*>(g.src);
    double s = 0.0;
    for (int k = threadIdx.x; k < (int)g.n; k += 256) s += partial[k];   // fixed order: deterministic
    s = block_sum(s, red);
    if (threadIdx.x == 0) *static_cast<float*>(g.out) = (float)(s * g.scale);
  }
}

static thread_local bool t_defer = false;
static thread_local ReduceMulti t_pending{};

static int flush_deferred(hipStream_t s) {
  if (t_pending.nseg == 0) return ITTS_OK;
  const ReduceSeg& last = t_pending.seg[t_pending.nseg - 1];
  const int64_t per = last.kind == 0 ? (last.n / 4 + 63) / 64 : (last.kind == 1 ? (last.n + 63) / 64 : 1);
  const int64_t blocks = last.first_block + per;
  hipLaunchKernelGGL(reduce_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t_pending);
  t_pending.nseg = 0;
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

static int queue_deferred(ReduceSeg g, hipStream_t s) {
  if (t_pending.nseg == kMaxDeferred) {
    const int rc = flush_deferred(s);
    if (rc) return rc;
  }
  int64_t first = 0;
  if (t_pending.nseg > 0) {
    const ReduceSeg& p = t_pending.seg[t_pending.nseg - 1];
    first = p.first_block + (p.kind == 0 ? (p.n / 4 + 63) / 64 : (p.kind == 1 ? (p.n + 63) / 64 : 1));
  }
  ITTS_REQUIRE(first < ((int64_t)1 << 30), "too many deferred reduction blocks");
  g.first_block = (int)first;
  t_pending.seg[t_pending.nseg++] = g;
  return ITTS_OK;
}

static int launch_reduce_slabs(const float* slabs, int S, int64_t n, float* out, int accumulate,
                               hipStream_t s, bool merged = false) {
  const bool vec = n % 4 == 0 && aligned16(slabs) && aligned16(out);
  plan_reduce(vec, merged, t_defer, S);
  if (t_defer) {
    ReduceSeg g{};
    g.src = slabs; g.out = out; g.n = n; g.S = S; g.accumulate = accumulate; g.kind = vec ? 0 : 1;
    return queue_deferred(g, s);
  }
  if (vec)
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((n / 4 + 63) / 64)), dim3(256), 0, s, slabs, S,
                       n, out, accumulate);
  else
    hipLaunchKernelGGL(reduce_slabs_scalar_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, slabs,
                       S, n, out, accumulate);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

int reduce_slabs(const float* slabs, int S, int64_t n, float* out, int accumulate, hipStream_t s) {
  return launch_reduce_slabs(slabs, S, n, out, accumulate, s);
}

// The last step of every loss entry point: the workgroups' partial sums, added in a fixed order.
__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ partial, int64_t nb,
                                                         double scale, float* __restrict__ loss) {
  __shared__ double red[16];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += 256) s += partial[i];  // fixed order: deterministic
  s = block_sum(s, red);
  if (threadIdx.x == 0) *loss = (float)(s * scale);
}

int loss_final_sum(const double* partial, int64_t nb, double scale, float* loss, hipStream_t s) {
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, partial, nb, scale, loss);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_defer_reductions(int on) {
  ITTS_REQUIRE(on || t_pending.nseg == 0,
               "queued reductions must be run (itts_reduce_deferred) before deferral is switched off");
  t_defer = on != 0;
  return ITTS_OK;
}

extern "C" int itts_reduce_deferred(void* stream) {
  t_defer = false;
  return flush_deferred(as_stream(stream));
}

template <int AF>
__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                               float* __restrict__ dz, int64_t n, int act) {
  if (AF == AF_BASE) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
      dz[i] = dy[i] * act_grad_from_out(y[i], act);
  } else {
    with_ext_act(act, [&](auto a) {
      for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
           i += (int64_t)gridDim.x * blockDim.x)
        dz[i] = dy[i] * dact1<decltype(a)::value>(y[i]);
    });
  }
}

// ---- masked MSE -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void masked_mse_kernel(
    const float* __restrict__ pred, int64_t ldp, const float* __restrict__ target, int64_t ldt,
    const uint8_t* __restrict__ valid, int64_t M, int D, float gscale, float* __restrict__ grad,
    int64_t ldg, double* __restrict__ partial) {
  __shared__ double red[16];
  const int64_t n = M * D;
  double s = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    const int c = (int)(i - r * D);
    float diff = 0.f;
    if (valid[r]) diff = pred[r * ldp + c] - target[r * ldt + c];
    s += (double)diff * (double)diff;
    if (grad) grad[r * ldg + c] = gscale * diff;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

static int launch_mse_final(const double* partial, int nb, double scale, float* loss, hipStream_t s) {
  if (t_defer) {
    ReduceSeg g{};
    g.src = partial; g.out = loss; g.n = nb; g.scale = scale; g.S = 1; g.kind = 2;
    return queue_deferred(g, s);
  }
  return loss_final_sum(partial, nb, scale, loss, s);
}

// ---- row-weighted elementwise losses (the other NamedLoss types / reductions) ------------------
// loss = sum_r w[r] sum_c e(pred - target), e = squared (kind 0, MSELoss) or absolute (kind 1,
// L1Loss) error; grad = w[r] e'(.) ; elem (optional) = w[r] e(.) per element (reduction 'none').
// The sequence mask and every reduction of NamedLoss._reduce (loss/NamedLoss.py:113-131) are a
// per-row weight: mean_per_frame mask / (frames D), mean_per_sample mask / (len_b B D),
// mean mask / (T B D), sum / none mask.
__global__ __launch_bounds__(256) void weighted_loss_kernel(
    const float* __restrict__ pred, int64_t ldp, const float* __restrict__ target, int64_t ldt,
    const float* __restrict__ w, int64_t M, int D, int kind, float* __restrict__ grad, int64_t ldg,
    float* __restrict__ elem, int64_t lde, double* __restrict__ partial) {
  __shared__ double red[16];
  const int64_t n = M * D;
  double s = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    const int c = (int)(i - r * D);
    const float wr = w[r];
    const float diff = pred[r * ldp + c] - target[r * ldt + c];
    const float e = kind == 0 ? diff * diff : fabsf(diff);
    const float g = kind == 0 ? 2.f * diff : (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));
    const float v = wr == 0.f ? 0.f : wr * e;          // padding may hold anything (also NaN)
    s += (double)v;
    if (grad) grad[r * ldg + c] = wr == 0.f ? 0.f : wr * g;
    if (elem) elem[r * lde + c] = v;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---- Adam ---------------------------------------------------------------------------------------
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, int64_t n, float beta1,
                            float beta2, float eps, float wd, float step_size, float bc2_sqrt,
                            float gscale) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * gscale;
    float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    float mi = m[i], vi = v[i];
    mi = mi + (gi - mi) * (1.f - beta1);         // exp_avg.lerp_(grad, 1-beta1)
    vi = vi * beta2 + (1.f - beta2) * gi * gi;   // mul_(beta2).addcmul_(g, g, 1-beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

// Adam with the gradient clipping in front and the parameter EMA behind it, one pass.
__global__ void adam_fused_kernel(float* __restrict__ p, const float* __restrict__ g,
                                  float* __restrict__ m, float* __restrict__ v, int64_t n,
                                  float beta1, float beta2, float eps, float wd, float step_size,
                                  float bc2_sqrt, float gscale, const float* __restrict__ norm_accum,
                                  int norm_kind, float max_norm, float clip_value,
                                  float* __restrict__ shadow, float one_minus_decay) {
  float coef = gscale;
  if (norm_accum) {
    const float a = norm_accum[0];
    const float total = (norm_kind == 2 ? sqrtf(a) : a) * fabsf(gscale);
    coef *= fminf(1.f, max_norm / (total + 1e-6f));
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * coef;
    if (clip_value > 0.f) gi = fminf(fmaxf(gi, -clip_value), clip_value);
    float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    float mi = m[i], vi = v[i];
    mi = mi + (gi - mi) * (1.f - beta1);
    vi = vi * beta2 + (1.f - beta2) * gi * gi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (shadow) {
      const float si = shadow[i];
      shadow[i] = si - one_minus_decay * (si - pi);
    }
  }
}

// sum x^2 / max |x| of a flat buffer: fixed grid of partials, then one block (deterministic)
constexpr int kNormBlocks = 1024;
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ x, int64_t n,
                                                               int kind, float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float xi = x[i];
    acc = kind == 2 ? acc + xi * xi : fmaxf(acc, fabsf(xi));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(acc, off, 64);
    acc = kind == 2 ? acc + o : fmaxf(acc, o);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    part[blockIdx.x] = kind == 2 ? (red[0] + red[1]) + (red[2] + red[3])
                                 : fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const float* __restrict__ part, int nb,
                                                             int kind, float* __restrict__ out,
                                                             int accumulate) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) acc = kind == 2 ? acc + part[i] : fmaxf(acc, part[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(acc, off, 64);
    acc = kind == 2 ? acc + o : fmaxf(acc, o);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = kind == 2 ? (red[0] + red[1]) + (red[2] + red[3])
                        : fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (accumulate) r = kind == 2 ? out[0] + r : fmaxf(out[0], r);
    out[0] = r;
  }
}

// ---- SGD (torch.optim.SGD: weight decay, momentum, dampening, Nesterov) -------------------------
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                           float* __restrict__ buf, int64_t n, float lr, float momentum,
                           float dampening, float wd, int nesterov, int first, float gscale) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * gscale;
    float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    if (momentum != 0.f) {
      float bi = first ? gi : buf[i] * momentum + (1.f - dampening) * gi;
      buf[i] = bi;
      gi = nesterov ? gi + momentum * bi : bi;
    }
    p[i] = pi - lr * gi;
  }
}

// ---- exponential moving average of the parameters: shadow -= (1-decay) * (shadow - x) ---------
__global__ void ema_kernel(float* __restrict__ shadow, const float* __restrict__ x, int64_t n,
                           float one_minus_decay) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float sh = shadow[i];
    shadow[i] = sh - one_minus_decay * (sh - x[i]);
  }
}

constexpr int kColsumSlices = 256;  // row slices of the bias-gradient column sums

// split-K of a weight-gradient GEMM on the ring kernel: as many slabs as keep the 512 persistent
// workgroups busy, chunks of whole K-steps
static int choose_splitk_ring(int64_t M, int N, int K) {
  const int wm = ring_wm(N, K);
  const int bmt = 64 * wm, bnt = 32 * (4 / wm);
  const int64_t tiles = (int64_t)((N + bmt - 1) / bmt) * ((K + bnt - 1) / bnt);
  int64_t s = std::max<int64_t>(1, kRingGrid / std::max<int64_t>(tiles, 1));
  s = std::min<int64_t>(s, std::max<int64_t>(1, (M + 255) / 256));
  return (int)std::min<int64_t>(s, 128);
}

static int choose_splitk(int64_t M, int N, int K) {
  const int64_t tiles = (int64_t)((N + BM - 1) / BM) * ((K + BN - 1) / BN);
  int64_t s = std::max<int64_t>(1, 512 / std::max<int64_t>(tiles, 1));
  const int64_t max_by_rows = std::max<int64_t>(1, (M + 511) / 512);
  s = std::min(s, max_by_rows);
  return (int)std::min<int64_t>(s, 128);
}

// ---- the products of a dense layer, each written once ------------------------------------------------------------
// DR is NoDrop behind the plain entry point and DropRule behind its _dropout form (the rule: dropout.h), which a
// refusal names.  A rule sits in the epilogue: on the output of the forward, on the previous layer's output in the
// input gradient; the weight and bias gradients take none (their operands dz and x are the dropped values already).
template <class DR>
int linear_fwd(const float* d_x, int64_t ldx, const float* d_w, const float* d_b, float* d_y, int64_t ldy, int64_t M,
               int N, int K, int act, hipStream_t s, const DR& dr) {
  const char* const entry = DR::on ? "itts_linear_fwd_dropout" : "itts_linear_fwd";
  const PlanScope plan_scope;
  ITTS_REQUIRE_AS(entry, d_w && (M == 0 || (d_x && d_y)), "null pointer");
  ITTS_REQUIRE_AS(entry, M >= 0 && N > 0 && K > 0 && ldx >= K && ldy >= N, "bad sizes");
  ITTS_REQUIRE_AS(entry, act >= ITTS_ACT_NONE && act <= ITTS_ACT_HARDSIGMOID, "unknown activation");
  if (M == 0) return ITTS_OK;
  GemmArgs g{};
  g.A = d_x; g.lda = ldx; g.B = d_w; g.ldb = K; g.C = d_y; g.ldc = ldy;
  g.M = M; g.N = N; g.K = K; g.bias = d_b; g.act = act;
  g.kchunk = ((K + BK - 1) / BK) * BK; g.slab_stride = 0;
  g.vecA = (ldx % 4 == 0) && aligned16(d_x);
  g.vecB = (K % 4 == 0) && aligned16(d_w);
  g.wide_out = (ldy % 4 == 0) && aligned16(d_y) && (!d_b || aligned16(d_b));
  if (act_family(act) == AF_EXT) return launch_gemm<true, true, EPI_BIAS_ACT, AF_EXT, DR>(g, 1, s, dr);
  return launch_gemm<true, true, EPI_BIAS_ACT, AF_BASE, DR>(g, 1, s, dr);
}
template int linear_fwd<NoDrop>(const float*, int64_t, const float*, const float*, float*, int64_t, int64_t, int, int,
                                int, hipStream_t, const NoDrop&);

// dx[M,K] = dz[M,N] (row form, reduction N) x w[N,K] (col form: [k=N][out=K]), times the derivative of the previous
// layer's activation where d_yprev, that layer's output, is given
static GemmArgs input_grad_args(const float* d_dz, int64_t lddz, const float* d_w, float* d_dx, int64_t lddx,
                                const float* d_yprev, int64_t ldyp, int act_prev, int64_t M, int N, int K) {
  GemmArgs g{};
  g.A = d_dz; g.lda = lddz; g.B = d_w; g.ldb = K; g.C = d_dx; g.ldc = lddx;
  g.M = M; g.N = K; g.K = N; g.aux = d_yprev; g.ldaux = ldyp; g.act = act_prev;
  g.kchunk = ((N + BK - 1) / BK) * BK; g.slab_stride = 0;
  g.vecA = (lddz % 4 == 0) && aligned16(d_dz);
  g.vecB = (K % 4 == 0) && aligned16(d_w);
  g.wide_out = (lddx % 4 == 0) && aligned16(d_dx) && (!d_yprev || ((ldyp % 4 == 0) && aligned16(d_yprev)));
  return g;
}

template <class DR>
static int linear_bwd_input(const float* d_dz, int64_t lddz, const float* d_w, float* d_dx, int64_t lddx,
                            const float* d_yprev, int64_t ldyp, int act_prev, int64_t M, int N, int K, hipStream_t s,
                            const DR& dr) {
  const char* const entry = DR::on ? "itts_linear_bwd_input_dropout" : "itts_linear_bwd_input";
  const PlanScope plan_scope;
  ITTS_REQUIRE_AS(entry, d_w && (M == 0 || (d_dz && d_dx)), "null pointer");
  ITTS_REQUIRE_AS(entry, !DR::on || d_yprev, "the previous layer's output is needed where it carries dropout");
  ITTS_REQUIRE_AS(entry, M >= 0 && N > 0 && K > 0 && lddz >= N && lddx >= K && (!DR::on || ldyp >= K), "bad sizes");
  ITTS_REQUIRE_AS(entry, !d_yprev || (act_prev >= ITTS_ACT_NONE && act_prev <= ITTS_ACT_HARDSIGMOID),
                  "unknown activation");
  if (M == 0) return ITTS_OK;
  const GemmArgs g = input_grad_args(d_dz, lddz, d_w, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K);
  if (d_yprev) {
    ITTS_REQUIRE_AS(entry, ldyp >= K, "ldyp too small");
    if (act_family(act_prev) == AF_EXT) return launch_gemm<true, false, EPI_DACT, AF_EXT, DR>(g, 1, s, dr);
    return launch_gemm<true, false, EPI_DACT, AF_BASE, DR>(g, 1, s, dr);
  }
  if constexpr (DR::on) return ITTS_OK;   // (not reached: a rule comes with d_yprev)
  else return launch_gemm<true, false, EPI_STORE>(g, 1, s);
}

// The weight-gradient product dw[N,K] = dz^T x (A = dz as col form [k=M][out=N]; B = x as col form [k=M][out=K]) in
// split-K slabs of the workspace, about S of them.  The bias gradient (column sums of dz) comes out of the same
// launch: the workgroups of the first column tile add up their resident dz tiles.  When db follows dw in memory (the
// flat gradient arenas) and both lengths are multiples of 4, one reduction serves both (merged).
struct WgradPlan {
  GemmArgs g;
  int S_eff;
  bool merged;
};

static WgradPlan wgrad_plan(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, const float* d_dw,
                            const float* d_db, int64_t M, int N, int K, void* d_workspace, int S) {
  WgradPlan w{};
  int64_t kchunk = (M + S - 1) / S;
  kchunk = ((kchunk + BK - 1) / BK) * BK;
  w.S_eff = (int)((M + kchunk - 1) / kchunk);
  const int64_t n = (int64_t)N * K;
  w.merged = d_db && d_db == d_dw + n && N % 4 == 0 && n % 4 == 0;
  float* slabs = reinterpret_cast<float*>(d_workspace);
  GemmArgs& g = w.g;
  g.A = d_dz; g.lda = lddz; g.B = d_x; g.ldb = ldx; g.C = slabs; g.ldc = K;
  g.M = N; g.N = K; g.K = M; g.kchunk = kchunk; g.slab_stride = w.merged ? n + N : n;
  g.vecA = (lddz % 4 == 0) && aligned16(d_dz);
  g.vecB = (ldx % 4 == 0) && aligned16(d_x);
  if (d_db) {
    g.bias_part = w.merged ? slabs + n : slabs + (int64_t)w.S_eff * n;
    g.bias_part_stride = w.merged ? g.slab_stride : N;
  }
  return w;
}

// the slabs of wgrad_plan's product, summed into dw and db
static int wgrad_reduce(const WgradPlan& w, float* d_dw, float* d_db, int accumulate, hipStream_t s) {
  const int64_t N = w.g.M, n = N * w.g.N;
  const int rc = launch_reduce_slabs(w.g.C, w.S_eff, w.merged ? n + N : n, d_dw, accumulate, s, w.merged);
  if (rc || w.merged || !d_db) return rc;
  return launch_reduce_slabs(w.g.bias_part, w.S_eff, N, d_db, accumulate, s);
}

// Weight gradient (+ bias gradient) and input gradient of one layer from one call: with operands
// that allow the LDS-DMA kernel the two GEMMs share a launch (gemm_ring_pair_kernel), otherwise
// this is itts_linear_bwd_weight followed by the input gradient above.  Same results either way
// (bit for bit: the tiles, the split-K chunks and their order are those of the separate calls).
template <class DR>
static int linear_bwd(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, const float* d_w, float* d_dw,
                      float* d_db, float* d_dx, int64_t lddx, const float* d_yprev, int64_t ldyp, int act_prev,
                      int64_t M, int N, int K, void* d_workspace, int accumulate, hipStream_t s, const DR& dr) {
  const char* const entry = DR::on ? "itts_linear_bwd_dropout" : "itts_linear_bwd";
  const PlanScope plan_scope;
  ITTS_REQUIRE_AS(entry, d_w && d_dw && d_workspace && (M == 0 || (d_dz && d_x && d_dx)), "null pointer");
  ITTS_REQUIRE_AS(entry, !DR::on || d_yprev, "the previous layer's output is needed where it carries dropout");
  ITTS_REQUIRE_AS(entry, M >= 0 && N > 0 && K > 0 && lddz >= N && ldx >= K && lddx >= K && (!DR::on || ldyp >= K),
                  "bad sizes");
  ITTS_REQUIRE_AS(entry, !d_yprev || ldyp >= K, "ldyp too small");
  ITTS_REQUIRE_AS(entry, !d_yprev || (act_prev >= ITTS_ACT_NONE && act_prev <= ITTS_ACT_HARDSIGMOID),
                  "unknown activation");
  const bool vec_ok = (lddz % 4 == 0) && aligned16(d_dz) && (ldx % 4 == 0) && aligned16(d_x) && (K % 4 == 0) &&
                      aligned16(d_w);
  bool fused = vec_ok && M > 0 && (lddx % 4 == 0) && aligned16(d_dx) &&
               (!d_yprev || ((ldyp % 4 == 0) && aligned16(d_yprev)));
  WgradPlan w{};
  GemmArgs gx{};
  if (fused) {
    w = wgrad_plan(d_dz, lddz, d_x, ldx, d_dw, d_db, M, N, K, d_workspace, choose_splitk_ring(M, N, K));
    gx = input_grad_args(d_dz, lddz, d_w, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K);
    fused = ring_ok<false, false>(w.g, w.S_eff, EPI_STORE) &&
            ring_ok<true, false>(gx, 1, d_yprev ? EPI_DACT : EPI_STORE);
  }
  if (!fused) {
    int rc = itts_linear_bwd_weight(d_dz, lddz, d_x, ldx, d_dw, d_db, M, N, K, d_workspace, accumulate, s);
    if (rc) return rc;
    return linear_bwd_input<DR>(d_dz, lddz, d_w, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K, s, dr);
  }
  int rc = ITTS_OK;
  const int wm = ring_wm(w.g.M, w.g.N);
  if (d_yprev && act_family(act_prev) == AF_EXT)
    rc = wm == 1 ? launch_ring_bwd_pair<1, EPI_DACT, AF_EXT, DR>(w.g, w.S_eff, gx, s, dr)
                 : launch_ring_bwd_pair<2, EPI_DACT, AF_EXT, DR>(w.g, w.S_eff, gx, s, dr);
  else if (d_yprev)
    rc = wm == 1 ? launch_ring_bwd_pair<1, EPI_DACT, AF_BASE, DR>(w.g, w.S_eff, gx, s, dr)
                 : launch_ring_bwd_pair<2, EPI_DACT, AF_BASE, DR>(w.g, w.S_eff, gx, s, dr);
  else if constexpr (!DR::on)   // (a rule comes with d_yprev)
    rc = wm == 1 ? launch_ring_bwd_pair<1, EPI_STORE>(w.g, w.S_eff, gx, s)
                 : launch_ring_bwd_pair<2, EPI_STORE>(w.g, w.S_eff, gx, s);
  if (rc) return rc;
  return wgrad_reduce(w, d_dw, d_db, accumulate, s);
}

}  // namespace itts

using namespace itts;

extern "C" int itts_linear_fwd(const float* d_x, int64_t ldx, const float* d_w, const float* d_b,
                               float* d_y, int64_t ldy, int64_t M, int N, int K, int act,
                               void* stream) {
  return linear_fwd(d_x, ldx, d_w, d_b, d_y, ldy, M, N, K, act, as_stream(stream), NoDrop{});
}

// ---- row gather: pack_padded_sequence / pad_packed_sequence / the h_{t-1} shift of the recurrent layers
// dst row r = src row idx[r] (its first `width` columns), the fill row (or zeros) where idx[r] is outside
// [0, n_src); columns width .. dst_width - 1 of every dst row are zeroed (row pitches of 16 bytes for the
// GEMMs).  One kernel for what the reference leaves to torch.nn.utils.rnn (rnn_dyn/RNNWrapper.py:89-102)
// and autograd: index_select + pad on the way in, index_copy into zeros on the way out, cat + index_select
// for the shifted state.
__global__ __launch_bounds__(256) void rows_gather_kernel(const float* __restrict__ src, int64_t ld_src, int64_t n_src,
                                                          const int64_t* __restrict__ idx, int64_t n_out, int width,
                                                          const float* __restrict__ fill, float* __restrict__ dst,
                                                          int64_t ld_dst, int dst_width, int vec) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), wn = (int64_t)gridDim.x * 4;
  for (int64_t r = w0; r < n_out; r += wn) {          // one wave per row
    const int64_t i = idx[r];
    const float* s = (i >= 0 && i < n_src) ? src + i * ld_src : fill;
    float* d = dst + r * ld_dst;
    if (vec) {
      const int w4 = width >> 2, d4 = dst_width >> 2;
      for (int c = lane; c < d4; c += 64) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < w4 && s) v = reinterpret_cast<const float4*>(s)[c];
        reinterpret_cast<float4*>(d)[c] = v;
      }
    } else {
      for (int c = lane; c < dst_width; c += 64) d[c] = (c < width && s) ? s[c] : 0.f;
    }
  }
}

extern "C" int itts_rows_gather_f32(const float* d_src, int64_t ld_src, int64_t n_src, const int64_t* d_idx,
                                    int64_t n_out, int width, const float* d_fill_row, float* d_dst, int64_t ld_dst,
                                    int dst_width, void* stream) {
  ITTS_REQUIRE(n_out == 0 || (d_idx && d_dst && (d_src || n_src == 0)), "null pointer");
  ITTS_REQUIRE(n_out >= 0 && n_src >= 0 && width >= 0 && dst_width >= width && ld_src >= width && ld_dst >= dst_width,
               "bad sizes");
  if (n_out == 0 || dst_width == 0) return ITTS_OK;
  const int vec = width % 4 == 0 && dst_width % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && aligned16(d_src) &&
                  aligned16(d_dst) && (!d_fill_row || aligned16(d_fill_row));
  const unsigned grid = (unsigned)std::min<int64_t>((n_out + 3) / 4, 16384);
  hipLaunchKernelGGL(rows_gather_kernel, dim3(grid), dim3(256), 0, as_stream(stream), d_src, ld_src, n_src, d_idx, n_out,
                     width, d_fill_row, d_dst, ld_dst, dst_width, vec);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_gemm_path_counts(int64_t out[8]) {
  ITTS_REQUIRE(out != nullptr, "null pointer");
  for (int k = 0; k < 2; ++k)
    for (int e = 0; e < 4; ++e) out[4 * k + e] = g_gemm_path[k][e].load(std::memory_order_relaxed);
  return ITTS_OK;
}

extern "C" int itts_gemm_last_plan(int32_t* out, int max_entries) {
  const int n = std::min(t_plan.n, kPlanMax);
  if (out)
    for (int i = 0; i < std::min(n, max_entries); ++i) std::copy(t_plan.e[i], t_plan.e[i] + kPlanInts, out + i * kPlanInts);
  return t_plan.n;
}

extern "C" int64_t itts_linear_fwd_mse_workspace_bytes(int64_t M, int N) {
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + 63) / 64);
  return std::max<int64_t>(tiles, kRingGrid) * 8;   // one partial sum per tile, or per persistent workgroup
}

// Forward of the output layer fused with NamedLoss(MSELoss, 'mean_per_frame'): d_loss [1] and
// d_dz [M, N] = d loss / d y; y itself is not stored (FFWrapper.py:63-73 followed by
// NamedLoss.py:70-117 in a training step).  Falls back to nothing: the buffers must allow 16-byte
// rows for x, w and dz (the trainer's buffers do); other callers use itts_linear_fwd +
// itts_masked_mse.
extern "C" int itts_linear_fwd_mse(const float* d_x, int64_t ldx, const float* d_w, const float* d_b,
                                   const float* d_target, int64_t ldt, const uint8_t* d_row_valid,
                                   double n_valid, float loss_weight, int64_t M, int N, int K,
                                   float* d_loss, float* d_dz, int64_t lddz, void* d_workspace,
                                   void* stream) {
  const PlanScope plan_scope;
  ITTS_REQUIRE(d_w && d_loss && d_workspace && (M == 0 || (d_x && d_target && d_row_valid && d_dz)),
               "null pointer");
  ITTS_REQUIRE(M >= 0 && N > 0 && K > 0 && ldx >= K && ldt >= N && lddz >= N && n_valid > 0, "bad sizes");
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    ITTS_HIP_CHECK(hipMemsetAsync(d_loss, 0, 4, s));
    return ITTS_OK;
  }
  ITTS_REQUIRE((ldx % 4 == 0) && aligned16(d_x) && (K % 4 == 0) && aligned16(d_w) && (lddz % 4 == 0) &&
                   aligned16(d_dz),
               "x, w and dz need 16-byte aligned rows (use itts_linear_fwd + itts_masked_mse otherwise)");
  GemmArgs g{};
  g.A = d_x; g.lda = ldx; g.B = d_w; g.ldb = K; g.C = d_dz; g.ldc = lddz;
  g.M = M; g.N = N; g.K = K; g.bias = d_b; g.act = 0;
  g.kchunk = ((K + BK - 1) / BK) * BK; g.slab_stride = 0;
  g.vecA = 1; g.vecB = 1; g.wide_out = 1;
  g.aux = d_target; g.ldaux = ldt; g.row_valid = d_row_valid;
  const double scale = (double)loss_weight / (n_valid * (double)N);
  g.gscale = (float)(2.0 * scale);
  g.loss_partial = reinterpret_cast<double*>(d_workspace);
  int64_t tiles = ((M + BM - 1) / BM) * ((N + 63) / 64);
  int rc;
  if (ring_ok<true, true>(g, 1, EPI_MSE)) {
    tiles = std::min<int64_t>(kRingGrid, (tiles + 7) / 8 * 8);   // partial sums per persistent workgroup
    rc = launch_ring_wm<true, true, EPI_MSE, 2>(g, 1, s);
  } else {
    rc = launch_gemm_tn<true, true, EPI_MSE, 1, 1>(g, 1, s);
  }
  if (rc) return rc;
  return launch_mse_final(reinterpret_cast<const double*>(d_workspace), (int)tiles, scale, d_loss, s);
}

extern "C" int itts_act_bwd(const float* d_dy, const float* d_y, float* d_dz, int64_t n_elem,
                            int act, void* stream) {
  ITTS_REQUIRE(d_dy && d_y && d_dz && n_elem >= 0, "bad arguments");
  ITTS_REQUIRE(act >= ITTS_ACT_NONE && act <= ITTS_ACT_HARDSIGMOID, "unknown activation");
  if (n_elem == 0) return ITTS_OK;
  const int blocks = (int)std::min<int64_t>((n_elem + 255) / 256, 4096);
  if (act_family(act) == AF_EXT)
    hipLaunchKernelGGL(act_bwd_kernel<AF_EXT>, dim3(blocks), dim3(256), 0, as_stream(stream), d_dy, d_y,
                       d_dz, n_elem, act);
  else
    hipLaunchKernelGGL(act_bwd_kernel<AF_BASE>, dim3(blocks), dim3(256), 0, as_stream(stream), d_dy, d_y,
                       d_dz, n_elem, act);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_linear_bwd_input(const float* d_dz, int64_t lddz, const float* d_w,
                                     float* d_dx, int64_t lddx, const float* d_yprev,
                                     int64_t ldyp, int act_prev, int64_t M, int N, int K,
                                     void* stream) {
  return linear_bwd_input(d_dz, lddz, d_w, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K, as_stream(stream), NoDrop{});
}

extern "C" int64_t itts_linear_bwd_weight_workspace_bytes(int64_t M, int N, int K) {
  if (M < 0 || N <= 0 || K <= 0) return 0;
  const int s = std::max(choose_splitk(M, N, K), choose_splitk_ring(M, N, K));
  return (int64_t)s * ((int64_t)N * K + N) * 4 + (int64_t)kColsumSlices * N * 4 + 8192;
}

extern "C" int itts_linear_bwd_weight(const float* d_dz, int64_t lddz, const float* d_x,
                                      int64_t ldx, float* d_dw, float* d_db, int64_t M, int N,
                                      int K, void* d_workspace, int accumulate, void* stream) {
  const PlanScope plan_scope;
  ITTS_REQUIRE(d_dw && d_workspace && (M == 0 || (d_dz && d_x)), "null pointer");
  ITTS_REQUIRE(M >= 0 && N > 0 && K > 0 && lddz >= N && ldx >= K, "bad sizes");
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    if (!accumulate) {
      ITTS_HIP_CHECK(hipMemsetAsync(d_dw, 0, (size_t)N * K * 4, s));
      if (d_db) ITTS_HIP_CHECK(hipMemsetAsync(d_db, 0, (size_t)N * 4, s));
    }
    return ITTS_OK;
  }
  const bool vec_ok = (lddz % 4 == 0) && aligned16(d_dz) && (ldx % 4 == 0) && aligned16(d_x) && (K % 4 == 0);
  const WgradPlan w = wgrad_plan(d_dz, lddz, d_x, ldx, d_dw, d_db, M, N, K, d_workspace,
                                 vec_ok ? choose_splitk_ring(M, N, K) : choose_splitk(M, N, K));
  const int rc = launch_gemm<false, false, EPI_STORE>(w.g, w.S_eff, s);
  if (rc) return rc;
  return wgrad_reduce(w, d_dw, d_db, accumulate, s);
}

extern "C" int itts_linear_bwd(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx,
                               const float* d_w, float* d_dw, float* d_db, float* d_dx, int64_t lddx,
                               const float* d_yprev, int64_t ldyp, int act_prev, int64_t M, int N, int K,
                               void* d_workspace, int accumulate, void* stream) {
  return linear_bwd(d_dz, lddz, d_x, ldx, d_w, d_dw, d_db, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K, d_workspace,
                    accumulate, as_stream(stream), NoDrop{});
}

// ---- dropout fused into the dense products (the rule: dropout.h) ---------------------------------
// Each entry point is its plain counterpart with p == 0 (the same launches), and otherwise the same product with the
// rule in the epilogue: on the output of the forward, on the previous layer's output in the input gradient.
// (linear_fwd is sparse_rows.hip's as well, so it is instantiated by name: this form here, where the dropout kernels
// have their place in the library)
template int itts::linear_fwd<DropRule>(const float*, int64_t, const float*, const float*, float*, int64_t, int64_t, int,
                                        int, int, hipStream_t, const DropRule&);
extern "C" int itts_linear_fwd_dropout(const float* d_x, int64_t ldx, const float* d_w, const float* d_b, float* d_y,
                                       int64_t ldy, int64_t M, int N, int K, int act, double p, uint64_t seed,
                                       uint32_t salt, int64_t row_offset, void* stream) {
  ITTS_REQUIRE_DROP_P(p);
  if (p == 0.0) return linear_fwd(d_x, ldx, d_w, d_b, d_y, ldy, M, N, K, act, as_stream(stream), NoDrop{});
  return linear_fwd(d_x, ldx, d_w, d_b, d_y, ldy, M, N, K, act, as_stream(stream),
                    make_drop_rule(p, seed, salt, row_offset));
}

extern "C" int itts_linear_bwd_input_dropout(const float* d_dz, int64_t lddz, const float* d_w, float* d_dx,
                                             int64_t lddx, const float* d_yprev, int64_t ldyp, int act_prev, int64_t M,
                                             int N, int K, double p, uint64_t seed, uint32_t salt, int64_t row_offset,
                                             void* stream) {
  ITTS_REQUIRE_DROP_P(p);
  if (p == 0.0)
    return linear_bwd_input(d_dz, lddz, d_w, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K, as_stream(stream), NoDrop{});
  return linear_bwd_input(d_dz, lddz, d_w, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K, as_stream(stream),
                          make_drop_rule(p, seed, salt, row_offset));
}

extern "C" int itts_linear_bwd_dropout(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, const float* d_w,
                                       float* d_dw, float* d_db, float* d_dx, int64_t lddx, const float* d_yprev,
                                       int64_t ldyp, int act_prev, int64_t M, int N, int K, void* d_workspace,
                                       int accumulate, double p, uint64_t seed, uint32_t salt, int64_t row_offset,
                                       void* stream) {
  ITTS_REQUIRE_DROP_P(p);
  if (p == 0.0)
    return linear_bwd(d_dz, lddz, d_x, ldx, d_w, d_dw, d_db, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K, d_workspace,
                      accumulate, as_stream(stream), NoDrop{});
  return linear_bwd(d_dz, lddz, d_x, ldx, d_w, d_dw, d_db, d_dx, lddx, d_yprev, ldyp, act_prev, M, N, K, d_workspace,
                    accumulate, as_stream(stream), make_drop_rule(p, seed, salt, row_offset));
}

// ---- elementwise dropout: out = in * m * scale (forward and backward alike), or the mask itself ----
// A thread takes four consecutive columns of a row: one Philox call.  Rows may have a pitch; in-place is allowed.
__global__ __launch_bounds__(256) void dropout_apply_kernel(const float* in, int64_t ldi, float* out,
                                                            int64_t ldo, uint8_t* mask, int64_t ldm, int64_t M, int N,
                                                            DropRule dr) {
  const int n4 = (N + 3) >> 2;
  const int64_t total = M * n4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / n4;
    const int col = (int)(i - row * n4) << 2;
    const uint4x w = dr.words(row, col);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (col + e >= N) break;
      if (mask) mask[row * ldm + col + e] = dr.keeps(w.w[e]) ? 1 : 0;
      else out[row * ldo + col + e] = dr.apply(in[row * ldi + col + e], w.w[e]);
    }
  }
}

extern "C" int itts_dropout_apply(const float* d_in, int64_t ldi, void* d_out, int64_t ldo, int64_t M, int N,
                                  int mask_only, double p, uint64_t seed, uint32_t salt, int64_t row_offset,
                                  void* stream) {
  ITTS_REQUIRE_DROP_P(p);
  ITTS_REQUIRE(M >= 0 && N > 0 && ldo >= N && (mask_only || ldi >= N), "bad sizes");
  ITTS_REQUIRE(M == 0 || (d_out && (mask_only || d_in)), "null pointer");
  if (M == 0) return ITTS_OK;
  const int64_t total = M * (int64_t)((N + 3) / 4);
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  const DropRule dr = make_drop_rule(p, seed, salt, row_offset);
  hipLaunchKernelGGL(dropout_apply_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_in, ldi,
                     mask_only ? nullptr : static_cast<float*>(d_out), ldo,
                     mask_only ? static_cast<uint8_t*>(d_out) : nullptr, ldo, M, N, dr);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// dz = dy * m * scale * act'(y), y = d * (1 - p): the way back through the dropout and the activation of a layer whose
// dropped output d nothing multiplies after it (the last layer of a chain).  dz may be dy.
template <int AF>
__global__ __launch_bounds__(256) void dropout_act_bwd_kernel(const float* dy, int64_t lddy, const float* __restrict__ d,
                                                              int64_t ldd, float* dz, int64_t lddz, int64_t M, int N,
                                                              int act, DropRule dr) {
  const int n4 = (N + 3) >> 2;
  const int64_t total = M * n4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / n4;
    const int col = (int)(i - row * n4) << 2;
    const uint4x w = dr.words(row, col);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (col + e >= N) break;
      const float g = dy[row * lddy + col + e];
      dz[row * lddz + col + e] =
          dr.keeps(w.w[e]) ? g * (dr.scale * act_grad_af<AF>(d[row * ldd + col + e] * dr.keep, act)) : 0.f;
    }
  }
}

extern "C" int itts_dropout_act_bwd(const float* d_dy, int64_t lddy, const float* d_d, int64_t ldd, float* d_dz,
                                    int64_t lddz, int64_t M, int N, int act, double p, uint64_t seed, uint32_t salt,
                                    int64_t row_offset, void* stream) {
  ITTS_REQUIRE_DROP_P(p);
  ITTS_REQUIRE(M >= 0 && N > 0 && lddy >= N && ldd >= N && lddz >= N, "bad sizes");
  ITTS_REQUIRE(M == 0 || (d_dy && d_d && d_dz), "null pointer");
  ITTS_REQUIRE(act >= ITTS_ACT_NONE && act <= ITTS_ACT_HARDSIGMOID, "unknown activation");
  if (M == 0) return ITTS_OK;
  const int64_t total = M * (int64_t)((N + 3) / 4);
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  const DropRule dr = make_drop_rule(p, seed, salt, row_offset);
  if (act_family(act) == AF_EXT)
    hipLaunchKernelGGL(dropout_act_bwd_kernel<AF_EXT>, dim3(blocks), dim3(256), 0, as_stream(stream), d_dy, lddy, d_d,
                       ldd, d_dz, lddz, M, N, act, dr);
  else
    hipLaunchKernelGGL(dropout_act_bwd_kernel<AF_BASE>, dim3(blocks), dim3(256), 0, as_stream(stream), d_dy, lddy, d_d,
                       ldd, d_dz, lddz, M, N, act, dr);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

static int mse_blocks(int64_t M, int D) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((M * D + 255) / 256, 2048));
}

extern "C" int64_t itts_masked_mse_workspace_bytes(int64_t M, int D) {
  if (M < 0 || D <= 0) return 0;
  return (int64_t)mse_blocks(M, D) * 8;
}

extern "C" int itts_masked_mse(const float* d_pred, int64_t ldp, const float* d_target,
                               int64_t ldt, const uint8_t* d_row_valid, int64_t M, int D,
                               double n_valid, float loss_weight, float* d_loss, float* d_grad,
                               int64_t ldg, void* d_workspace, void* stream) {
  ITTS_REQUIRE(d_pred && d_target && d_row_valid && d_loss && d_workspace, "null pointer");
  ITTS_REQUIRE(M >= 0 && D > 0 && ldp >= D && ldt >= D && n_valid > 0, "bad sizes");
  ITTS_REQUIRE(!d_grad || ldg >= D, "ldg too small");
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    ITTS_HIP_CHECK(hipMemsetAsync(d_loss, 0, 4, s));
    return ITTS_OK;
  }
  const int nb = mse_blocks(M, D);
  const double scale = (double)loss_weight / (n_valid * (double)D);
  hipLaunchKernelGGL(masked_mse_kernel, dim3(nb), dim3(256), 0, s, d_pred, ldp, d_target, ldt,
                     d_row_valid, M, D, (float)(2.0 * scale), d_grad, ldg,
                     reinterpret_cast<double*>(d_workspace));
  ITTS_LAUNCH_CHECK();
  return launch_mse_final(reinterpret_cast<const double*>(d_workspace), nb, scale, d_loss, s);
}

extern "C" int itts_weighted_loss(const float* d_pred, int64_t ldp, const float* d_target, int64_t ldt,
                                  const float* d_row_weight, int64_t M, int D, int kind,
                                  float* d_loss, float* d_grad, int64_t ldg, float* d_elem,
                                  int64_t lde, void* d_workspace, void* stream) {
  ITTS_REQUIRE(d_pred && d_target && d_row_weight && d_loss && d_workspace, "null pointer");
  ITTS_REQUIRE(M >= 0 && D > 0 && ldp >= D && ldt >= D && (kind == 0 || kind == 1), "bad sizes");
  ITTS_REQUIRE((!d_grad || ldg >= D) && (!d_elem || lde >= D), "leading dimension too small");
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    ITTS_HIP_CHECK(hipMemsetAsync(d_loss, 0, 4, s));
    return ITTS_OK;
  }
  const int nb = mse_blocks(M, D);
  hipLaunchKernelGGL(weighted_loss_kernel, dim3(nb), dim3(256), 0, s, d_pred, ldp, d_target, ldt,
                     d_row_weight, M, D, kind, d_grad, ldg, d_elem, lde,
                     reinterpret_cast<double*>(d_workspace));
  ITTS_LAUNCH_CHECK();
  return loss_final_sum(reinterpret_cast<const double*>(d_workspace), nb, 1.0, d_loss, s);
}

extern "C" int itts_adam_step(float* d_param, const float* d_grad, float* d_exp_avg,
                              float* d_exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int64_t step, float grad_scale,
                              void* stream) {
  ITTS_REQUIRE(d_param && d_grad && d_exp_avg && d_exp_avg_sq, "null pointer");
  ITTS_REQUIRE(n >= 0 && step >= 1, "bad sizes (step counts from 1)");
  if (n == 0) return ITTS_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_param, d_grad,
                     d_exp_avg, d_exp_avg_sq, n, beta1, beta2, eps, weight_decay, step_size,
                     bc2_sqrt, grad_scale);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_grad_norm_accum(const float* d_x, int64_t n, int norm_kind, float* d_accum,
                                    int accumulate, void* d_workspace, void* stream) {
  ITTS_REQUIRE(d_accum && d_workspace && (n == 0 || d_x), "null pointer");
  ITTS_REQUIRE(n >= 0 && (norm_kind == 2 || norm_kind == 0), "norm_kind must be 2 or 0 (infinity)");
  const int nb = (int)std::min<int64_t>((n + 255) / 256, kNormBlocks);
  hipStream_t s = as_stream(stream);
  float* part = static_cast<float*>(d_workspace);
  if (nb > 0) {
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(nb), dim3(256), 0, s, d_x, n, norm_kind, part);
    ITTS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, s, part, nb, norm_kind, d_accum,
                     accumulate);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_adam_step_fused(float* d_param, const float* d_grad, float* d_exp_avg,
                                    float* d_exp_avg_sq, int64_t n, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, int64_t step,
                                    float grad_scale, const float* d_norm_accum, int norm_kind,
                                    float clip_max_norm, float clip_value, float* d_ema_shadow,
                                    float ema_decay, void* stream) {
  ITTS_REQUIRE(d_param && d_grad && d_exp_avg && d_exp_avg_sq, "null pointer");
  ITTS_REQUIRE(n >= 0 && step >= 1, "bad sizes (step counts from 1)");
  ITTS_REQUIRE(!d_norm_accum || ((norm_kind == 2 || norm_kind == 0) && clip_max_norm > 0.f),
               "norm clipping needs norm_kind 2 or 0 and a positive max norm");
  if (n == 0) return ITTS_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(adam_fused_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_param,
                     d_grad, d_exp_avg, d_exp_avg_sq, n, beta1, beta2, eps, weight_decay,
                     (float)(lr / bc1), (float)sqrt(bc2), grad_scale, d_norm_accum, norm_kind,
                     clip_max_norm, clip_value, d_ema_shadow, 1.f - ema_decay);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_sgd_step(float* d_param, const float* d_grad, float* d_momentum_buf, int64_t n,
                             float lr, float momentum, float dampening, float weight_decay,
                             int nesterov, int first_step, float grad_scale, void* stream) {
  ITTS_REQUIRE(d_param && d_grad, "null pointer");
  ITTS_REQUIRE(momentum == 0.f || d_momentum_buf, "momentum needs a buffer");
  ITTS_REQUIRE(n >= 0, "bad size");
  if (n == 0) return ITTS_OK;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(sgd_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_param, d_grad,
                     d_momentum_buf, n, lr, momentum, dampening, weight_decay, nesterov,
                     first_step, grad_scale);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_ema_update(float* d_shadow, const float* d_param, int64_t n, float decay,
                               void* stream) {
  ITTS_REQUIRE(d_shadow && d_param, "null pointer");
  ITTS_REQUIRE(n >= 0, "bad size");
  if (n == 0) return ITTS_OK;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(ema_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_shadow, d_param,
                     n, 1.f - decay);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
