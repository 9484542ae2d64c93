// LayerNorm over the last extent of [N, D] fp32 rows (torch.nn.LayerNorm as an RNNDyn layer group builds it,
// rnn_dyn/FFWrapper.py: `getattr(torch.nn, "LayerNorm")(**kwargs)`), with the group's activation fused:
//   y = act((x - mean) * rstd * gamma + beta),  mean / biased variance over the D columns, rstd = 1 / sqrt(var + eps)
//
// One wave64 owns a row and keeps it in registers: lane l holds the columns 4 (l + 64 j) .. + 3 for j < NJ
// (NJ = 1, 2, 4, 8, 16 for D <= 256 .. 4096), as one 16-byte load per j where pitch and base allow (VEC), as
// four plain loads otherwise -- the SAME columns in the same lane either way, and every sum first over a lane's
// columns in ascending order, then over the wave by the xor butterfly of wave_sum.  So a row's y and dx depend on
// nothing but the row: not on N, not on its place in the batch, not on the alignment of the tensors (the padded
// and the valid-rows path of a layer group give the same bits for the same frame).
// The variance is taken in a second pass over the centred values, which costs nothing with the row in registers
// (E[x^2] - mean^2 loses every digit on unnormalised acoustic features with their large offsets); the centred
// values are centred once more on their own mean, which removes the rounding of the first sum.
//
// A workgroup of four waves takes `rows_per_block(N)` consecutive rows, wave w the rows w, w + 4, ...  The backward
// accumulates dgamma / dbeta per lane over the wave's rows, adds the four waves in wave order through LDS and
// writes ONE slab per workgroup; a second launch sums the slabs in a fixed order.  No atomics: repeated calls
// give identical bits.
//
// Memory-bound: the forward reads and writes N * D * 4 bytes each, the backward reads x and dy (and y under an
// activation) and writes dx; gamma, beta, mean, rstd and the slabs are noise next to that.
#include <algorithm>

#include "activations.h"
#include "common.h"
#include "row4.h"

namespace itts {
namespace {

constexpr int LN_WAVES = 4;
constexpr int LN_THREADS = LN_WAVES * kWave;
constexpr int LN_MAX_D = 4096;
constexpr int LN_ROWS = 32;             // rows per workgroup, times ..
constexpr int64_t LN_MAX_SLABS = 1024;  // .. whatever keeps the slab count at or below this

int64_t rows_per_block(int64_t N) {
  const int64_t span = LN_ROWS * LN_MAX_SLABS;
  return LN_ROWS * std::max<int64_t>(1, (N + span - 1) / span);
}
int64_t slab_count(int64_t N) {
  const int64_t R = rows_per_block(N);
  return (N + R - 1) / R;
}

struct LnFwdArgs {
  const float* x; int64_t ldx;
  const float* gamma; const float* beta;
  float* y; int64_t ldy;
  float* mean; float* rstd;
  int64_t N, rows;
  int D, act;
  float eps;
};

template <int NJ, bool VEC, int AF>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(LnFwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = a.D;
  const int64_t r0 = (int64_t)blockIdx.x * a.rows, r1 = min(a.N, r0 + a.rows);
  float gam[NJ * 4], bet[NJ * 4];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = 4 * (lane + 64 * j);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gam[4 * j + k] = (a.gamma && col + k < D) ? a.gamma[col + k] : 1.f;
      bet[4 * j + k] = (a.beta && col + k < D) ? a.beta[col + k] : 0.f;
    }
  }
  const float fD = (float)D;
  for (int64_t r = r0 + wave; r < r1; r += LN_WAVES) {
    const float* xr = a.x + r * a.ldx;
    float x[NJ * 4];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      load4z_pitch<VEC>(xr, 4 * (lane + 64 * j), D, x + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) s += x[4 * j + k];
    }
    // centre on the rounded mean, then take out the mean of what is left (the rounding of the first sum, which
    // at an offset of 1e4 is a thousand times the float32 spacing of the centred values)
    const float m0 = wave_sum(s) / fD;
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = 4 * (lane + 64 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[4 * j + k] = col + k < D ? x[4 * j + k] - m0 : 0.f;
        c += x[4 * j + k];
      }
    }
    c = wave_sum(c) / fD;
    const float mean = m0 + c;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = 4 * (lane + 64 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[4 * j + k] = col + k < D ? x[4 * j + k] - c : 0.f;
        q += x[4 * j + k] * x[4 * j + k];
      }
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / fD + a.eps);
    float* yr = a.y + r * a.ldy;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        x[4 * j + k] = act_fwd_af<AF>(x[4 * j + k] * rstd * gam[4 * j + k] + bet[4 * j + k], a.act);
      store4<VEC>(yr, 4 * (lane + 64 * j), D, x + 4 * j);
    }
    if (lane == 0) {
      a.mean[r] = mean;
      a.rstd[r] = rstd;
    }
  }
}

struct LnBwdArgs {
  const float* dy; int64_t lddy;
  const float* x; int64_t ldx;
  const float* y; int64_t ldy;      // null without an activation
  const float* mean; const float* rstd;
  const float* gamma;
  float* dx; int64_t lddx;
  float* slabs;                     // [blocks][2][D]: dgamma, dbeta partials; null when neither is wanted
  int64_t N, rows;
  int D, act;
};

template <int NJ, bool VEC, int AF>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_kernel(LnBwdArgs a) {
  constexpr int CAP = NJ * 256;     // columns the instantiation covers
  __shared__ float acc[2 * CAP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = a.D;
  const int64_t r0 = (int64_t)blockIdx.x * a.rows, r1 = min(a.N, r0 + a.rows);
  float gam[NJ * 4], dgam[NJ * 4], dbet[NJ * 4];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = 4 * (lane + 64 * j);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gam[4 * j + k] = (a.gamma && col + k < D) ? a.gamma[col + k] : 1.f;
      dgam[4 * j + k] = dbet[4 * j + k] = 0.f;
    }
  }
  const float fD = (float)D;
  for (int64_t r = r0 + wave; r < r1; r += LN_WAVES) {
    const float mean = a.mean[r], rstd = a.rstd[r];
    const float* xr = a.x + r * a.ldx;
    const float* dyr = a.dy + r * a.lddy;
    float xh[NJ * 4], g[NJ * 4];
    // x - mean, minus its own mean: the stored mean is rounded to float32 (see the forward)
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = 4 * (lane + 64 * j);
      load4z_pitch<VEC>(xr, col, D, xh + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xh[4 * j + k] = col + k < D ? xh[4 * j + k] - mean : 0.f;
        c += xh[4 * j + k];
      }
    }
    c = wave_sum(c) / fD;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = 4 * (lane + 64 * j);
      float y4[4];
      load4z_pitch<VEC>(dyr, col, D, g + 4 * j);
      if (a.y) load4z_pitch<VEC>(a.y + r * a.ldy, col, D, y4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = 4 * j + k;
        xh[i] = col + k < D ? (xh[i] - c) * rstd : 0.f;
        const float dyp = a.y ? g[i] * act_grad_af<AF>(y4[k], a.act) : g[i];      // (dy = 0 beyond column D)
        dgam[i] += dyp * xh[i];
        dbet[i] += dyp;
        g[i] = dyp * gam[i];
        s1 += g[i];
        s2 += g[i] * xh[i];
      }
    }
    s1 = wave_sum(s1) / fD;
    s2 = wave_sum(s2) / fD;
    float* dxr = a.dx + r * a.lddx;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int k = 0; k < 4; ++k) g[4 * j + k] = rstd * (g[4 * j + k] - s1 - xh[4 * j + k] * s2);
      store4<VEC>(dxr, 4 * (lane + 64 * j), D, g + 4 * j);
    }
  }
  if (!a.slabs) return;             // (uniform over the grid)
  // the four waves' partial column sums in wave order, then one slab per workgroup
  for (int w = 0; w < LN_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int col = 4 * (lane + 64 * j);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[col + k] = w == 0 ? dgam[4 * j + k] : acc[col + k] + dgam[4 * j + k];
          acc[CAP + col + k] = w == 0 ? dbet[4 * j + k] : acc[CAP + col + k] + dbet[4 * j + k];
        }
      }
    }
    __syncthreads();
  }
  float* slab = a.slabs + (int64_t)blockIdx.x * 2 * D;
  for (int c = threadIdx.x; c < D; c += LN_THREADS) {
    slab[c] = acc[c];
    slab[D + c] = acc[CAP + c];
  }
}

// dgamma[c] = sum_s slabs[s][0][c], dbeta[c] = sum_s slabs[s][1][c]: 64 columns a workgroup, sixteen groups of
// lanes take the slabs g, g + 16, ... in ascending order, and their sums are added in group order
constexpr int LN_RED_GROUPS = 16;
__global__ __launch_bounds__(64 * LN_RED_GROUPS) void ln_reduce_kernel(const float* __restrict__ slabs, int S, int D,
                                                                      float* dgamma, float* dbeta) {
  __shared__ float part[LN_RED_GROUPS][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + cl;
  float s = 0.f;
  if (q < 2 * D)
    for (int i = g; i < S; i += LN_RED_GROUPS) s += slabs[(int64_t)i * 2 * D + q];
  part[g][cl] = s;
  __syncthreads();
  if (g != 0 || q >= 2 * D) return;
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < LN_RED_GROUPS; ++i) t += part[i][cl];
  if (q < D) {
    if (dgamma) dgamma[q] = t;
  } else if (dbeta) {
    dbeta[q - D] = t;
  }
}

// instantiation by width class, load form and activation family (see activations.h)
#define LN_LAUNCH(kernel, NJ)                                                                       \
  do {                                                                                              \
    if (vec) {                                                                                      \
      if (af == AF_EXT) kernel<NJ, true, AF_EXT><<<grid, LN_THREADS, 0, s>>>(a);                    \
      else kernel<NJ, true, AF_BASE><<<grid, LN_THREADS, 0, s>>>(a);                                \
    } else {                                                                                        \
      if (af == AF_EXT) kernel<NJ, false, AF_EXT><<<grid, LN_THREADS, 0, s>>>(a);                   \
      else kernel<NJ, false, AF_BASE><<<grid, LN_THREADS, 0, s>>>(a);                               \
    }                                                                                               \
  } while (0)

#define LN_DISPATCH(kernel)                                                                         \
  do {                                                                                              \
    if (a.D <= 256) LN_LAUNCH(kernel, 1);                                                           \
    else if (a.D <= 512) LN_LAUNCH(kernel, 2);                                                      \
    else if (a.D <= 1024) LN_LAUNCH(kernel, 4);                                                     \
    else if (a.D <= 2048) LN_LAUNCH(kernel, 8);                                                     \
    else LN_LAUNCH(kernel, 16);                                                                     \
  } while (0)

}  // namespace
}  // namespace itts

using namespace itts;

#define LN_CHECK_WIDTH()                                                                            \
  ITTS_REQUIRE(D >= 1 && D <= LN_MAX_D, "width D = " + std::to_string(D) + " is outside 1 .. " +    \
                                            std::to_string(LN_MAX_D))

extern "C" int64_t itts_layernorm_workspace_bytes(int64_t N, int D) {
  if (N <= 0 || D <= 0) return 0;
  return slab_count(N) * 2 * (int64_t)D * (int64_t)sizeof(float);
}

extern "C" int itts_layernorm_fwd(const float* d_x, int64_t ldx, const float* d_gamma, const float* d_beta,
                                  float* d_y, int64_t ldy, float* d_mean, float* d_rstd, int64_t N, int D,
                                  double eps, int act, void* stream) {
  LN_CHECK_WIDTH();
  ITTS_REQUIRE(N >= 0 && ldx >= D && ldy >= D, "bad sizes");
  ITTS_REQUIRE(eps >= 0.0, "negative eps");
  ITTS_REQUIRE(act >= ITTS_ACT_NONE && act <= ITTS_ACT_HARDSIGMOID, "unknown activation");
  if (N == 0) return ITTS_OK;
  ITTS_REQUIRE(d_x && d_y && d_mean && d_rstd, "null pointer");
  hipStream_t s = as_stream(stream);
  LnFwdArgs a{};
  a.x = d_x; a.ldx = ldx; a.gamma = d_gamma; a.beta = d_beta; a.y = d_y; a.ldy = ldy;
  a.mean = d_mean; a.rstd = d_rstd; a.N = N; a.rows = rows_per_block(N); a.D = D; a.act = act;
  a.eps = (float)eps;
  const bool vec = rows16(d_x, ldx) && rows16(d_y, ldy);
  const int af = act_family(act);
  const dim3 grid((unsigned)slab_count(N));
  LN_DISPATCH(ln_fwd_kernel);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_layernorm_bwd(const float* d_dy, int64_t lddy, const float* d_x, int64_t ldx,
                                  const float* d_y, int64_t ldy, const float* d_mean, const float* d_rstd,
                                  const float* d_gamma, float* d_dx, int64_t lddx, float* d_dgamma,
                                  float* d_dbeta, int64_t N, int D, int act, void* d_workspace, void* stream) {
  LN_CHECK_WIDTH();
  ITTS_REQUIRE(N >= 0 && lddy >= D && ldx >= D && lddx >= D, "bad sizes");
  ITTS_REQUIRE(act >= ITTS_ACT_NONE && act <= ITTS_ACT_HARDSIGMOID, "unknown activation");
  ITTS_REQUIRE(act == ITTS_ACT_NONE || N == 0 || (d_y && ldy >= D), "an activation needs the forward's y");
  const bool want_cols = d_dgamma || d_dbeta;
  hipStream_t s = as_stream(stream);
  if (N == 0) {                     // empty column sums
    if (d_dgamma) ITTS_HIP_CHECK(hipMemsetAsync(d_dgamma, 0, (size_t)D * sizeof(float), s));
    if (d_dbeta) ITTS_HIP_CHECK(hipMemsetAsync(d_dbeta, 0, (size_t)D * sizeof(float), s));
    return ITTS_OK;
  }
  ITTS_REQUIRE(d_dy && d_x && d_mean && d_rstd && d_dx, "null pointer");
  ITTS_REQUIRE(!want_cols || d_workspace, "dgamma / dbeta need the workspace");
  LnBwdArgs a{};
  a.dy = d_dy; a.lddy = lddy; a.x = d_x; a.ldx = ldx;
  a.y = act != ITTS_ACT_NONE ? d_y : nullptr; a.ldy = ldy;
  a.mean = d_mean; a.rstd = d_rstd; a.gamma = d_gamma; a.dx = d_dx; a.lddx = lddx;
  a.slabs = want_cols ? reinterpret_cast<float*>(d_workspace) : nullptr;
  a.N = N; a.rows = rows_per_block(N); a.D = D; a.act = act;
  const bool vec = rows16(d_dy, lddy) && rows16(d_x, ldx) && rows16(d_dx, lddx) && (!a.y || rows16(d_y, ldy));
  const int af = act_family(act);
  const int S = (int)slab_count(N);
  const dim3 grid((unsigned)S);
  LN_DISPATCH(ln_bwd_kernel);
  ITTS_LAUNCH_CHECK();
  if (want_cols) {
    ln_reduce_kernel<<<dim3((2 * D + 63) / 64), 64 * LN_RED_GROUPS, 0, s>>>(a.slabs, S, D, d_dgamma, d_dbeta);
    ITTS_LAUNCH_CHECK();
  }
  return ITTS_OK;
}
