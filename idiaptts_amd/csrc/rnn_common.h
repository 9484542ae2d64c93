// Shared pieces of the LSTM / GRU / vanilla RNN recurrence kernels (rnn_step.h, rnn_persist.h): the scratch layouts, the
// cell arithmetic -- written here once, called by the step kernels and by the persistent kernels -- and the host helpers.
//
// Memory layouts that make every operand load of a step a fully coalesced 1 KB wave access.
// v_mfma_f32_16x16x4_f32 wants lane (lr = lane & 15, kg = lane >> 4) to hold row lr, k = kg; with
// the K-permutation trick a lane loads 4 consecutive k (16 bytes) per MFMA quartet.  In a row-major
// matrix the 16 rows of a tile are kilobytes apart, so a wave load touches 64 separate 16-byte
// pieces and the L1 serialises them (measured: ~90 clocks per load, 6 us per step for 40 loads).
// Hence:
//   * running state (h, c, the backward pass's carried dG) lives in K-BLOCKED form
//       blocked(b, k) = ((k >> 2) * B + b) * 4 + (k & 3)          [K/4][B][4]
//     so the 16 rows of a tile are 16 consecutive float4;
//   * W_hh is re-tiled once per layer call into [unit group][k block][16 tile rows][4], the exact
//     order the lanes read it.
// These are private scratch layouts inside d_state; the C ABI keeps torch's layouts.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace itts {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ size_t blocked(int b, int k, int B) {
  return ((size_t)(k >> 2) * B + b) * 4 + (k & 3);
}

// The cell's sigmoid and tanh sit on the recurrence's critical path (five of them per LSTM step and
// thread, one after the products): the hardware's exp2 and reciprocal (1 ulp each) instead of the
// library's expf / IEEE division / tanhf -- 4 and 6 instructions against ~30 and ~40.  Absolute error
// below 2e-7 everywhere (tanh is formed as 1 - 2 / (1 + e^{2x}): no relative accuracy near 0, none needed:
// it multiplies a gate); saturates to 0 / 1 / -1 for large arguments like the library forms.
__device__ __forceinline__ float sigmoid_acc(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}
__device__ __forceinline__ float tanh_cell(float x) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * 2.88539008177792681f));
}

// ---- cell arithmetic (one thread = one (batch row, hidden unit)) --------------------------------------------------
// torch.nn.LSTM, gate order i, f, g, o.  p* = the unit's four rows of h_{t-1} W_hh^T, x* = its input projections
// (both biases included); c, h: previous state in, new state out; (ig, fg, gg, og) is what backward needs.
__device__ __forceinline__ void lstm_cell_fwd(float p0, float p1, float p2, float p3, float x0, float x1, float x2,
                                              float x3, float& c, float& h, float& ig, float& fg, float& gg,
                                              float& og) {
  ig = sigmoid_acc(p0 + x0);
  fg = sigmoid_acc(p1 + x1);
  gg = tanh_cell(p2 + x2);
  og = sigmoid_acc(p3 + x3);
  c = fg * c + ig * gg;
  h = og * tanh_cell(c);
}

// torch.nn.GRU, gate order r, z, n:
//   r = sigmoid(gin_r + W_hr h + b_hr)      z = sigmoid(gin_z + W_hz h + b_hz)
//   n = tanh(gin_n + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h
// p* = h_{t-1} W_hh^T, x* = input projections (b_ih included), b* = b_hh; saved for backward: (r, z, n, W_hn h + b_hn)
__device__ __forceinline__ void gru_cell_fwd(float p0, float p1, float p2, float x0, float x1, float x2, float b0,
                                             float b1, float b2, float& h, float& rg, float& zg, float& ng,
                                             float& hnp) {
  rg = sigmoid_acc(x0 + p0 + b0);
  zg = sigmoid_acc(x1 + p1 + b1);
  hnp = p2 + b2;
  ng = tanh_cell(x2 + rg * hnp);
  h = (1.f - zg) * ng + zg * h;
}

// LSTM gate gradients of one step: the saved gates, c_t and c_{t-1}, dh = dy + dG(s + 1) W_hh; carry: the dc that
// step s + 1 left (dc * f there) in, this step's out; d0 .. d3: gradient wrt the pre-activations of i, f, g, o.
__device__ __forceinline__ void lstm_cell_bwd(float ig, float fg, float gg, float og, float ct, float cp, float dh,
                                              float& carry, float& d0, float& d1, float& d2, float& d3) {
  const float tc = tanh_cell(ct);
  const float dcv = dh * og * (1.f - tc * tc) + carry;
  d0 = dcv * gg * ig * (1.f - ig);
  d1 = dcv * cp * fg * (1.f - fg);
  d2 = dcv * ig * (1.f - gg * gg);
  d3 = dh * tc * og * (1.f - og);
  carry = dcv * fg;
}

// GRU gate gradients of one step: the saved (r, z, n, W_hn h + b_hn), h_{t-1}, dydh = dy + dGh(s + 1) W_hh; carry:
// dh * z of step s + 1 in, of this step out.
//   dh   = dydh + carry       dn = dh (1 - z)      dz = dh (h_prev - n)
//   da_n = dn (1 - n^2)       da_r = da_n * hn_pre * r (1 - r)      da_z = dz * z (1 - z)
// dGi = (da_r, da_z, da_n) is the gradient wrt gin, dGh = (da_r, da_z, da_n * r) wrt the hidden projections.
__device__ __forceinline__ void gru_cell_bwd(float rg, float zg, float ng, float hnp, float hp, float dydh,
                                             float& carry, float& dar, float& daz, float& dan, float& danr) {
  const float dh = dydh + carry;
  const float dn = dh * (1.f - zg);
  const float dz = dh * (hp - ng);
  dan = dn * (1.f - ng * ng);
  dar = dan * hnp * rg * (1.f - rg);
  daz = dz * zg * (1.f - zg);
  danr = dan * rg;
  carry = dh * zg;
}

// torch.nn.RNN: h' = act(gin + W_hh h), act = ITTS_ACT_TANH or ITTS_ACT_RELU.  p = the unit's row of h_{t-1} W_hh^T,
// x = its input projection (both biases included).  Nothing is saved: backward takes the derivative from h' itself.
__device__ __forceinline__ float rnn_cell_fwd(float p, float x, int act) {
  const float z = p + x;
  return act == ITTS_ACT_RELU ? (z < 0.f ? 0.f : z) : tanh_cell(z);
}

// Its gradient wrt the pre-activation from the stored output y = h' and dh = dy + dG(s + 1) W_hh: 1 - y^2, or y > 0
// (torch's rule at 0).
__device__ __forceinline__ float rnn_cell_bwd(float y, float dh, int act) {
  return act == ITTS_ACT_RELU ? (y > 0.f ? dh : 0.f) : dh * (1.f - y * y);
}

// Forward tiling of W_hh [ndir][G*H][H] for workgroups of U hidden units, U = 4 with G = 3 or 4 gates, U = 16 with the
// vanilla RNN's one:
//   out[dir][jg = H/U][kb = H/4][lr = gate*U + unit][4] = W[dir][gate*H + jg*U + unit][kb*4 ..]
// tile rows of a missing 4th gate are zero.
static __global__ void rnn_pack_w_fwd_kernel(const float* __restrict__ w, float* __restrict__ out, int ndir,
                                      int G, int H) {
  const int U = G == 1 ? 16 : 4;
  const int64_t n = (int64_t)ndir * (H / U) * (H / 4) * 16;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int lr = (int)(i & 15);
    const int kb = (int)((i >> 4) % (H / 4));
    const int jg = (int)(((i >> 4) / (H / 4)) % (H / U));
    const int d = (int)((i >> 4) / ((int64_t)(H / 4) * (H / U)));
    const int g = lr / U, u = lr % U;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g < G) v = *reinterpret_cast<const float4*>(w + ((size_t)d * G * H + (size_t)g * H + jg * U + u) * H + kb * 4);
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

// Backward tiling (W_hh^T rows of 16 hidden units against the K = G*H gate rows):
//   out[dir][jg = H/16][kb = G*H/4][lr][kk] = W[dir][kb*4 + kk][jg*16 + lr]
static __global__ void rnn_pack_w_bwd_kernel(const float* __restrict__ w, float* __restrict__ out, int ndir,
                                      int G, int H) {
  const int KB = G * H / 4;
  const int64_t n = (int64_t)ndir * (H / 16) * KB * 16;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int lr = (int)(i & 15);
    const int kb = (int)((i >> 4) % KB);
    const int jg = (int)(((i >> 4) / KB) % (H / 16));
    const int d = (int)((i >> 4) / ((int64_t)KB * (H / 16)));
    const float* src = w + ((size_t)d * G * H + (size_t)kb * 4) * H + jg * 16 + lr;
    reinterpret_cast<float4*>(out)[i] = make_float4(src[0], src[H], src[2 * (size_t)H], src[3 * (size_t)H]);
  }
}

// state[parity 0][dir] (blocked) = init[dir][:] broadcast over the batch (zeros when init is NULL)
static __global__ void rnn_init_state_kernel(const float* __restrict__ init, float* __restrict__ st, int ndir,
                                      int B, int H) {
  const int64_t n = (int64_t)ndir * B * H;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i / ((int64_t)B * H));
    const int64_t e = i % ((int64_t)B * H);          // blocked offset inside the direction
    const int j = (int)(e / (4 * (int64_t)B)) * 4 + (int)(e & 3);
    st[i] = init ? init[d * H + j] : 0.f;
  }
}

// out[dir][b][j] = state of row b in the parity written by its last active step, (len_b & 1)
static __global__ void rnn_final_state_kernel(const float* __restrict__ st, const int* __restrict__ lengths,
                                       float* __restrict__ out, int ndir, int B, int H) {
  const int64_t n = (int64_t)ndir * B * H;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % H);
    const int b = (int)((i / H) % B);
    const int d = (int)(i / ((int64_t)B * H));
    out[i] = st[((int64_t)(lengths[b] & 1) * ndir + d) * B * H + blocked(b, j, B)];
  }
}

}  // namespace itts

static inline int rnn_check(const int* h_lengths, int T, int B, int H, int ndir) {
  ITTS_REQUIRE(T >= 1 && B >= 1 && (ndir == 1 || ndir == 2), "bad sizes");
  ITTS_REQUIRE(H >= 16 && H % 16 == 0 && H <= 4096, "hidden size must be a multiple of 16");
  ITTS_REQUIRE(h_lengths != nullptr, "host copy of the lengths is required");
  ITTS_REQUIRE(h_lengths[0] == T && h_lengths[B - 1] >= 1, "T must be the longest length, all lengths >= 1");
  for (int b = 1; b < B; ++b) ITTS_REQUIRE(h_lengths[b] <= h_lengths[b - 1], "rows must be sorted by decreasing length");
  return ITTS_OK;
}

// number of rows still active at recurrence step s (lengths sorted decreasingly); `p` carries the
// previous answer so that a whole sweep costs O(B + T)
static inline int rnn_active_rows(const int* h_lengths, int B, int s, int* p) {
  while (*p > 0 && h_lengths[*p - 1] <= s) --*p;
  while (*p < B && h_lengths[*p] > s) ++*p;
  return *p;
}

static inline dim3 rnn_ew_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)); }

// host copy of the packed-row offsets: row_off[t] = rows active in the steps before t, row_off[T] = N
static inline std::vector<int> rnn_row_offsets(const int* h_lengths, int T, int B) {
  std::vector<int> row_off(T + 1, 0);
  int q = B;
  for (int t = 0; t < T; ++t) row_off[t + 1] = row_off[t] + rnn_active_rows(h_lengths, B, t, &q);
  return row_off;
}
