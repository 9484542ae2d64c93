// All-pass frequency warping of cepstral rows, the reference's vocal-tract-length layer (layers/AllPassWarp.py:
// `bmm(feature, warp_matrix)` per block of N coefficients, the first coefficient of blocks 0..2 halved before and
// doubled after, layers/AllPassWarpLayer.py: de-normalisation before and normalisation after) -- without the
// reference's [N, N, 2N] factorial table and without any warp matrix in memory.  For one row with factor a,
//   W[0][0] = 1,  W[0][c] = 0,  W[r][0] = a W[r-1][0],  W[r][c] = W[r-1][c-1] + a (W[r-1][c] - W[r][c-1])
// (the reference's own gen_warp_matrix_recursively, equal to the table's closed form), and dW/da along the same
// lines:  dW[r][0] = a dW[r-1][0] + W[r-1][0],
//         dW[r][c] = dW[r-1][c-1] + (W[r-1][c] - W[r][c-1]) + a (dW[r-1][c] - dW[r][c-1]).
// Every entry is bounded by 1 for |a| < 1, so float32 holds at any N (the table's coefficients reach 7.8e42 at N = 60).
//
// One lane owns a row (a frame), one wave64 workgroup 64 consecutive rows.  An entry needs its left, upper and
// upper-left neighbours, so the matrix can be swept column by column or row by row with ONE column / row of state,
// kept in LDS as [index][lane]: a wave's access is 64 consecutive floats, conflict-free.
//   forward  y_b[c]  = sum_r x_b'[r] W[r][c]:  columns outside, r inside; the sums of up to three blocks in registers
//   backward dx_b'[r] = sum_c g_b'[c] W[r][c], da = sum_b sum_r x_b'[r] (sum_c g_b'[c] dW[r][c]):  rows outside, c inside
// Each entry is the same expression of the same neighbours in both sweeps.  The 64 rows of x (and of dy) of up to
// three blocks are staged through LDS tiles [block][row][N | 1] -- global loads and stores run along rows, the odd
// pitch makes `tile[lane][i]` conflict-free -- with normalisation and the halving applied on the way in and out; the
// forward collects y in a second tile, the backward overwrites x_b'[r] by dx_b'[r] once row r has used it.  More
// than three blocks go in groups, W swept again per group.  The backward recomputes W and dW from a: nothing but x
// and a is kept from the forward.  A row's da is summed by its own lane in a fixed order: no atomics, repeated calls
// give identical bits.
#include "allpass.h"

namespace itts {
namespace {

constexpr int AP_MAX_GROUP = 3;  // blocks whose sums a lane carries through one sweep (static, delta, delta-delta)

__host__ __device__ inline int ap_pitch(int N) { return N | 1; }

// blocks per sweep: as few sweeps as AP_MAX_GROUP allows, the blocks spread evenly over them (4 -> 2 + 2)
int ap_group(int nb) {
  const int sweeps = (nb + AP_MAX_GROUP - 1) / AP_MAX_GROUP;
  return (nb + sweeps - 1) / sweeps;
}

// One tile row per iteration, lane c of it: columns b * N + c of row f0 + f for the NBG blocks from b0 on, as
//   scale_in(v) = (v * sd + mean), halved at c == 0 of blocks 0..2        (IS_GRAD false: x)
//   scale_in(v) = (v / sd), doubled at c == 0 of blocks 0..2              (IS_GRAD true: dy)
// Rows past the last and blocks past nb are zeros.
template <int NBG, bool IS_GRAD>
__device__ __forceinline__ void ap_stage_in(const AllpassArgs& p, const float* __restrict__ src, int64_t ld,
                                            int64_t f0, int nf, int b0, float* tile) {
  const int lane = threadIdx.x, N = p.N, P = ap_pitch(N);
  if (lane >= N) return;
#pragma unroll
  for (int j = 0; j < NBG; ++j) {
    const int b = b0 + j, d = b * N + lane;
    const bool live = b < p.nb;
    const float sd = (live && p.sd) ? p.sd[d] : 1.f;
    const float mean = (live && p.mean && !IS_GRAD) ? p.mean[d] : 0.f;
    const float edge = (lane == 0 && b < 3) ? (IS_GRAD ? 2.f : 0.5f) : 1.f;
    for (int f = 0; f < 64; ++f) {
      float v = 0.f;
      if (live && f < nf) {
        v = src[(f0 + f) * ld + d];
        v = IS_GRAD ? v / sd : v * sd + mean;
        v *= edge;
      }
      tile[(j * 64 + f) * P + lane] = v;
    }
  }
}

// .. and out: y = (v doubled at c == 0 of blocks 0..2 - mean) / sd, or dx = (v halved there) * sd
template <int NBG, bool IS_GRAD>
__device__ __forceinline__ void ap_stage_out(const AllpassArgs& p, float* __restrict__ dst, int64_t ld, int64_t f0,
                                             int nf, int b0, const float* tile) {
  const int lane = threadIdx.x, N = p.N, P = ap_pitch(N);
  if (lane >= N) return;
#pragma unroll
  for (int j = 0; j < NBG; ++j) {
    const int b = b0 + j, d = b * N + lane;
    if (b >= p.nb) break;
    const float sd = p.sd ? p.sd[d] : 1.f;
    const float mean = (p.mean && !IS_GRAD) ? p.mean[d] : 0.f;
    const float edge = (lane == 0 && b < 3) ? (IS_GRAD ? 0.5f : 2.f) : 1.f;
    for (int f = 0; f < nf; ++f) {
      float v = tile[(j * 64 + f) * P + lane] * edge;
      v = IS_GRAD ? v * sd : (v - mean) / sd;
      dst[(f0 + f) * ld + d] = v;
    }
  }
}

template <int NBG>
__global__ __launch_bounds__(kWave) void allpass_fwd_kernel(AllpassArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ap_lds[];
  const int lane = threadIdx.x, N = p.N, P = ap_pitch(N);
  float* col = ap_lds;              // [N][64]: column c - 1 of W, overwritten by column c from the top down
  float* xt = col + N * 64;         // [NBG][64][P]
  float* yt = xt + NBG * 64 * P;    // [NBG][64][P]
  const int64_t f0 = (int64_t)blockIdx.x * 64;
  const int nf = (int)min((int64_t)64, p.M - f0);
  const float a = lane < nf ? p.alpha[f0 + lane] : 0.f;
  for (int b0 = 0; b0 < p.nb; b0 += NBG) {
    __syncthreads();                // (the previous group's tiles are written out)
    ap_stage_in<NBG, false>(p, p.x, p.ldx, f0, nf, b0, xt);
    __syncthreads();
    const float* xl = xt + lane * P;
    float* yl = yt + lane * P;
    float acc[NBG];
    // column 0: W[r][0] = a W[r-1][0]
    float w = 1.f;
#pragma unroll
    for (int j = 0; j < NBG; ++j) acc[j] = 0.f;
    for (int r = 0; r < N; ++r) {
      col[r * 64 + lane] = w;
#pragma unroll
      for (int j = 0; j < NBG; ++j) acc[j] += xl[j * 64 * P + r] * w;
      w *= a;
    }
#pragma unroll
    for (int j = 0; j < NBG; ++j) yl[j * 64 * P] = acc[j];
    for (int c = 1; c < N; ++c) {
      float up_left = col[lane];    // W[r-1][c-1]
      float up = 0.f;               // W[r-1][c], W[0][c] = 0
      col[lane] = 0.f;
#pragma unroll
      for (int j = 0; j < NBG; ++j) acc[j] = 0.f;
      for (int r = 1; r < N; ++r) {
        const float left = col[r * 64 + lane];      // W[r][c-1]
        up = up_left + a * (up - left);
        col[r * 64 + lane] = up;
        up_left = left;
#pragma unroll
        for (int j = 0; j < NBG; ++j) acc[j] += xl[j * 64 * P + r] * up;
      }
#pragma unroll
      for (int j = 0; j < NBG; ++j) yl[j * 64 * P + c] = acc[j];
    }
    __syncthreads();
    ap_stage_out<NBG, false>(p, p.y, p.ldy, f0, nf, b0, yt);
  }
}

template <int NBG>
__global__ __launch_bounds__(kWave) void allpass_bwd_kernel(AllpassArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ap_lds[];
  const int lane = threadIdx.x, N = p.N, P = ap_pitch(N);
  float* wrow = ap_lds;             // [N][64]: row r - 1 of W, overwritten by row r from the left
  float* drow = wrow + N * 64;      // [N][64]: the same of dW
  float* gt = drow + N * 64;        // [NBG][64][P]: g'
  float* xt = gt + NBG * 64 * P;    // [NBG][64][P]: x', entry r replaced by dx'[r] after row r
  const int64_t f0 = (int64_t)blockIdx.x * 64;
  const int nf = (int)min((int64_t)64, p.M - f0);
  const float a = lane < nf ? p.alpha[f0 + lane] : 0.f;
  float da = 0.f;
  for (int b0 = 0; b0 < p.nb; b0 += NBG) {
    __syncthreads();
    ap_stage_in<NBG, true>(p, p.dy, p.lddy, f0, nf, b0, gt);
    ap_stage_in<NBG, false>(p, p.x, p.ldx, f0, nf, b0, xt);
    __syncthreads();
    const float* gl = gt + lane * P;
    float* xl = xt + lane * P;
    // row 0: W = (1, 0, ..), dW = 0: dx'[0] = g'[0], nothing for da
    for (int c = 0; c < N; ++c) {
      wrow[c * 64 + lane] = c == 0 ? 1.f : 0.f;
      drow[c * 64 + lane] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < NBG; ++j) xl[j * 64 * P] = gl[j * 64 * P];
    for (int r = 1; r < N; ++r) {
      float w_ul = wrow[lane], d_ul = drow[lane];   // W[r-1][c-1], dW[r-1][c-1]
      float w = a * w_ul;                           // W[r][c-1], dW[r][c-1]: column 0 first
      float d = a * d_ul + w_ul;
      wrow[lane] = w;
      drow[lane] = d;
      float s[NBG], e[NBG];                         // sum_c g'[c] W[r][c], sum_c g'[c] dW[r][c]
#pragma unroll
      for (int j = 0; j < NBG; ++j) {
        const float g = gl[j * 64 * P];
        s[j] = g * w;
        e[j] = g * d;
      }
      for (int c = 1; c < N; ++c) {
        const float w_up = wrow[c * 64 + lane], d_up = drow[c * 64 + lane];   // W[r-1][c], dW[r-1][c]
        const float t = w_up - w;
        d = d_ul + t + a * (d_up - d);
        w = w_ul + a * t;
        wrow[c * 64 + lane] = w;
        drow[c * 64 + lane] = d;
        w_ul = w_up;
        d_ul = d_up;
#pragma unroll
        for (int j = 0; j < NBG; ++j) {
          const float g = gl[j * 64 * P + c];
          s[j] += g * w;
          e[j] += g * d;
        }
      }
#pragma unroll
      for (int j = 0; j < NBG; ++j) {
        da += xl[j * 64 * P + r] * e[j];
        xl[j * 64 * P + r] = s[j];
      }
    }
    __syncthreads();
    ap_stage_out<NBG, true>(p, p.dx, p.lddx, f0, nf, b0, xt);
  }
  if (lane < nf) p.dalpha[f0 + lane] = da;
}

size_t ap_lds_bytes(int N, int nbg, bool bwd) {
  return ((size_t)(bwd ? 2 : 1) * N * 64 + (size_t)2 * nbg * 64 * ap_pitch(N)) * sizeof(float);
}

template <typename K>
hipError_t ap_launch(K kernel, const AllpassArgs& a, size_t lds, hipStream_t s) {
  hipError_t e = itts::allow_dynamic_lds(reinterpret_cast<const void*>(kernel), lds);
  if (e != hipSuccess) return e;
  kernel<<<dim3((unsigned)((a.M + 63) / 64)), kWave, lds, s>>>(a);
  return hipGetLastError();
}

}  // namespace

hipError_t allpass_launch_fwd(const AllpassArgs& a, hipStream_t s) {
  const int nbg = ap_group(a.nb);
  const size_t lds = ap_lds_bytes(a.N, nbg, false);
  if (nbg == 1) return ap_launch(allpass_fwd_kernel<1>, a, lds, s);
  if (nbg == 2) return ap_launch(allpass_fwd_kernel<2>, a, lds, s);
  return ap_launch(allpass_fwd_kernel<3>, a, lds, s);
}

hipError_t allpass_launch_bwd(const AllpassArgs& a, hipStream_t s) {
  const int nbg = ap_group(a.nb);
  const size_t lds = ap_lds_bytes(a.N, nbg, true);
  if (nbg == 1) return ap_launch(allpass_bwd_kernel<1>, a, lds, s);
  if (nbg == 2) return ap_launch(allpass_bwd_kernel<2>, a, lds, s);
  return ap_launch(allpass_bwd_kernel<3>, a, lds, s);
}

}  // namespace itts
