// Register-staged fp32-MFMA GEMM (exact fp32: v_mfma_f32_32x32x2_f32), the body shared by the dense
// layers' general path (nn.hip: gemm_f32_kernel) and the Conv1d implicit GEMM (conv1d.hip:
// conv1d_gemm_kernel).  The two differ only in how an operand tile reaches the registers (a Loader
// with load_a<NROWS> / load_b<NROWS>) and in the output row of a logical row (the epilogue's RowOf).
//   * 128 x (64 TN) output tile per 256-thread workgroup, 4 waves as 2x2, each wave 2 x TN MFMA
//     tiles of 32x32 (TN = 2: 64 accumulator VGPRs), K step 32, LDS double buffered (73.7 KB -> 2
//     workgroups per CU), global loads of tile k+1 in flight during the MFMAs of tile k; or one LDS
//     stage (STAGES = 1: the next tile waits in registers, two barriers per K tile).
//   * an operand is either "row form" [out][k] (k contiguous, e.g. x[M,K], w[N,K]) or "col
//     form" [k][out] (e.g. dz[M,N] as the reduction-major operand of dW).  Row-form tiles are
//     copied to LDS unchanged with a 4-float pad (144-B rows: conflict-free ds_read_b128);
//     col-form tiles are [k][128+4] and read with ds_read_b32 (lanes = consecutive floats).
//   * K permutation instead of an LDS transpose: the MFMA takes k = lane>>5 from each lane;
//     lane half h feeds k = 8g + 4h + j on step j of k-group g, for A and B alike, so one
//     ds_read_b128 per lane supplies four MFMAs.
// A Loader fills float4 r[NROWS / 32] of thread threadIdx.x with the tile at (out0, k0) in the
// layout store_tile expects: row form, element (out0 + idx / 8, k0 + 4 (idx % 8) .. + 3); col form,
// element (k0 + idx / (NROWS / 4), out0 + 4 (idx % (NROWS / 4)) .. + 3), idx = threadIdx.x + 256 i;
// zero beyond k_end and beyond the operand's out extent.
#pragma once
#include <algorithm>

#include "activations.h"
#include "common.h"
#include "dropout.h"

namespace itts {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BK = 32;
constexpr int LD_ROW = BK + 4;             // row-form tile [128][36]
constexpr int TILE_FLOATS = 128 * LD_ROW;  // 4608 >= 32*132 = 4224

// LDS of a kernel: buffer b holds the A tile at 2b * TILE_FLOATS, the B tile at (2b + 1) * TILE_FLOATS;
// one stage (36.9 KB -> 4 workgroups per CU) trims the B tile to its size
template <bool B_ROW, int TN, int STAGES>
constexpr int staged_lds_floats() {
  return STAGES == 1 ? TILE_FLOATS + (B_ROW ? 64 * TN * LD_ROW : BK * (64 * TN + 4)) : 2 * STAGES * TILE_FLOATS;
}

enum { EPI_STORE = 0, EPI_BIAS_ACT = 1, EPI_DACT = 2, EPI_MSE = 3 };

struct GemmArgs {
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  float* C;
  int64_t ldc;
  int64_t M;  // output rows
  int N;      // output cols
  int64_t K;  // reduction length
  const float* bias;
  const float* aux;
  int64_t ldaux;
  int act;
  int64_t kchunk;       // reduction elements per blockIdx.z (multiple of BK)
  int64_t slab_stride;  // floats between split-K slabs of C
  int vecA, vecB;       // 16-B vector loads allowed
  int wide_out;         // C (and bias, aux) allow 16-B accesses: float4 epilogue of the row-form kernel
  // EPI_MSE (last layer of a training step): C receives d loss / d output instead of the output
  const uint8_t* row_valid;   // [M]
  float gscale;               // 2 * loss_weight / (n_valid * D)
  double* loss_partial;       // [grid] sums of squared masked differences, one per workgroup
  // col-form A (weight gradients): column sums of A over this launch's K chunk, i.e. the bias
  // gradient, as a by-product of the workgroups of the first column tile
  float* bias_part;           // [slab][M] or NULL
  int64_t bias_part_stride;
};

template <bool ROWFORM, int NROWS>
__device__ __forceinline__ void store_tile(float* __restrict__ S, const float4 (&r)[NROWS / 32]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NROWS / 32; ++i) {
    const int idx = tid + 256 * i;
    int off;
    if (ROWFORM)
      off = (idx >> 3) * LD_ROW + ((idx & 7) << 2);
    else
      off = (idx / (NROWS / 4)) * (NROWS + 4) + ((idx % (NROWS / 4)) << 2);
    *reinterpret_cast<float4*>(S + off) = r[i];
  }
}

// Fragment of k-group g for the 32 rows starting at `o` (tile-local): 4 k values per lane.
template <bool ROWFORM, int NROWS>
__device__ __forceinline__ float4 read_frag(const float* __restrict__ S, int o, int g, int lane) {
  const int r = lane & 31, h = lane >> 5;
  if (ROWFORM) {
    return *reinterpret_cast<const float4*>(S + (o + r) * LD_ROW + g * 8 + 4 * h);
  } else {
    constexpr int LDC = NROWS + 4;
    const float* p = S + (g * 8 + 4 * h) * LDC + o + r;
    return make_float4(p[0], p[LDC], p[2 * LDC], p[3 * LDC]);
  }
}

struct StagedTile {
  int64_t m0;   // first output row and column of the workgroup's tile
  int n0;
};

// The workgroup's output tile, accumulated over its K chunk (blockIdx.z) into acc[i][j] of wave
// (wm, wn) = (wid >> 1, wid & 1): rows m0 + 64 wm + 32 i, columns n0 + 64 TN wn / 2 + 32 j.  With
// col-form A and g.bias_part, the workgroups of the first column tile also write the column sums of
// A (g.bias_part[blockIdx.z * bias_part_stride + m]).  On return every tile read of LDS is behind a
// barrier: the caller may reuse lds.
template <bool A_ROW, bool B_ROW, int TN, int STAGES, class Loader>
__device__ __forceinline__ StagedTile staged_gemm_tile(const GemmArgs& g, const Loader& ld, float* lds,
                                                       f32x16 (&acc)[2][TN]) {
  constexpr int BNT = 64 * TN;
  // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so give each
  // XCD a contiguous run of tiles that share the same B panel (weights) where possible.
  const int tiles_n = (g.N + BNT - 1) / BNT;
  const int64_t tiles_m = (g.M + BM - 1) / BM;
  const int64_t ntiles = tiles_m * tiles_n;
  int64_t bid = blockIdx.x;
  {
    const int64_t q = ntiles / 8, r = ntiles % 8;
    const int64_t xcd = bid % 8, pos = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  }
  const int64_t tm = bid / tiles_n;
  const int tn = (int)(bid % tiles_n);
  const int64_t m0 = tm * BM;
  const int n0 = tn * BNT;

  const int64_t kbeg = (int64_t)blockIdx.z * g.kchunk;
  const int64_t kend = std::min<int64_t>(g.K, kbeg + g.kchunk);
  const int64_t nkt = (kend - kbeg + BK - 1) / BK;

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const bool do_bias = !A_ROW && g.bias_part != nullptr && tn == 0;
  float bsum = 0.f;
  float4 ra[BM / 32], rb[BNT / 32];
  if (nkt > 0) {
    ld.template load_a<BM>(m0, kbeg, kend, ra);
    ld.template load_b<BNT>(n0, kbeg, kend, rb);
    store_tile<A_ROW, BM>(lds, ra);
    store_tile<B_ROW, BNT>(lds + TILE_FLOATS, rb);
  }
  __syncthreads();

  for (int64_t kt = 0; kt < nkt; ++kt) {
    const int cur = STAGES == 1 ? 0 : (int)(kt & 1);
    const bool more = kt + 1 < nkt;
    if (more) {
      ld.template load_a<BM>(m0, kbeg + (kt + 1) * BK, kend, ra);
      ld.template load_b<BNT>(n0, kbeg + (kt + 1) * BK, kend, rb);
    }
    const float* cA = lds + (2 * cur) * TILE_FLOATS;
    const float* cB = lds + (2 * cur + 1) * TILE_FLOATS;
#pragma unroll
    for (int kg = 0; kg < BK / 8; ++kg) {
      float4 fa[2], fb[TN];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = read_frag<A_ROW, BM>(cA, wm * 64 + i * 32, kg, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = read_frag<B_ROW, BNT>(cB, wn * 32 * TN + j * 32, kg, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
        }
    }
    if (!A_ROW && do_bias) {   // column sums of the A tile ([k][out], pitch BM + 4) while it is resident
      const int o = threadIdx.x & 127, kh = threadIdx.x >> 7;
      const float* ct = cA + (kh * (BK / 2)) * (BM + 4) + o;
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) bsum += ct[kk * (BM + 4)];
    }
    if (STAGES == 1) __syncthreads();   // everyone has read the current tile
    if (more) {
      constexpr int nb = STAGES == 1 ? 0 : 1;
      store_tile<A_ROW, BM>(lds + (2 * (cur ^ nb)) * TILE_FLOATS, ra);
      store_tile<B_ROW, BNT>(lds + (2 * (cur ^ nb) + 1) * TILE_FLOATS, rb);
    }
    __syncthreads();
  }

  if (!A_ROW && do_bias) {   // the two k halves meet in LDS (all tile reads are behind the loop's last barrier)
    const int o = threadIdx.x & 127, kh = threadIdx.x >> 7;
    if (kh == 1) lds[o] = bsum;
    __syncthreads();
    if (kh == 0 && m0 + o < g.M)
      g.bias_part[(int64_t)blockIdx.z * g.bias_part_stride + m0 + o] = bsum + lds[o];
  }
  return StagedTile{m0, n0};
}

// Per-element epilogue of the tile: logical row m (< g.M) goes to row row_of(m) of C (and of aux)
// in slab blockIdx.z; bias + activation of family AF (EPI_BIAS_ACT), times the activation
// derivative through aux (EPI_DACT), or the plain sum (EPI_STORE).
// C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// DR: the dropout rule of the dense layers (dropout.h) on the output (EPI_BIAS_ACT) or on the previous layer's
// output in aux (EPI_DACT); a lane holds one column here, so it takes one word of a Philox call per element.
template <int EPI, int TN, int AF, class RowOf, class DR = NoDrop>
__device__ __forceinline__ void staged_epilogue(const GemmArgs& g, const StagedTile& t, const f32x16 (&acc)[2][TN],
                                                const RowOf& row_of, const DR& dr = DR()) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  float* C = g.C + (int64_t)blockIdx.z * g.slab_stride;
  const int cl = lane & 31, rh = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = t.n0 + wn * 32 * TN + j * 32 + cl;
      if (col >= g.N) continue;
      float bv = 0.f;
      if (EPI == EPI_BIAS_ACT && g.bias) bv = g.bias[col];
      uint32_t keep = 0;   // bit r: element r of the block is kept (worked out ahead of the arithmetic: registers)
      if constexpr (DR::on) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t m = t.m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * rh;
          if (m < g.M) keep |= ((dr.keep_bits(row_of(m), col) >> (col & 3)) & 1u) << r;
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = t.m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * rh;
        if (m >= g.M) continue;
        const int64_t row = row_of(m);
        float v = acc[i][j][r];
        if (EPI == EPI_BIAS_ACT) v = act_fwd_af<AF>(v + bv, g.act);
        if constexpr (DR::on) {
          const uint32_t bit = (keep >> r) & 1u;
          if (EPI == EPI_BIAS_ACT) v = dr.apply_bit(v, bit);
          if (EPI == EPI_DACT)
            v = bit ? v * (dr.scale * act_grad_af<AF>(g.aux[row * g.ldaux + col] * dr.keep, g.act)) : 0.f;
        } else {
          if (EPI == EPI_DACT) v *= act_grad_af<AF>(g.aux[row * g.ldaux + col], g.act);
        }
        C[row * g.ldc + col] = v;
      }
    }
}

}  // namespace itts
