// Per-step recurrence kernels of the LSTM (G = 4 gates), GRU (G = 3) and vanilla RNN (G = 1) layers and their host
// driver (included by rnn.hip): one launch per time step, both directions in it.  They run every case the persistent
// kernels of rnn_persist.h do not take (other hidden sizes, devices with fewer than 256 CUs, every vanilla RNN layer)
// and every layer call a persistent launch gave up on.  Packed layout, load ordering and the split of the work: rnn.hip.
#pragma once
#include "rnn_common.h"

namespace itts {

constexpr int FW_UNITS = 4;    // hidden units per workgroup in the forward step (G of the 16 tile rows x 4 used)
constexpr int FW_UNITS_1 = 16; // ... of the vanilla RNN: one gate, so every tile row is a unit
constexpr int BW_UNITS = 16;   // hidden units per workgroup in the backward step

struct RnnStepArgs {
  int T, B, H, ndir;
  const int* rev_row;     // [T*B] device: packed row the reverse direction visits at step s for
                          //       row b, row_off[len_b - 1 - s] + b (unused where s >= len_b)
  const float* gin;       // [N, ndir*G*H] input projections (N = sum of lengths); LSTM: both biases included,
                          //       GRU: b_ih only
  const float* wp;        // re-tiled W_hh (rnn_pack_w_fwd_kernel / rnn_pack_w_bwd_kernel)
  const float* bhh;       // GRU: [ndir][3H]
  const float* c0;        // LSTM backward: [ndir][H] or NULL
  float* hs;              // [2 parity][ndir] K-blocked running hidden state; GRU backward: the dh * z carry
  float* cs;              // LSTM: [2 parity][ndir] K-blocked running cell state; backward: the dc * f carry
  float* dgb;             // [2 parity][ndir] K-blocked dG (GRU: dGh) of the step just processed (backward)
  float* y;               // [N, ndir*H] layer output (vanilla RNN backward: input, all it saved)
  float* gates;           // [N, ndir, H, 4] saved for backward, one 16-byte store / load per (frame, unit):
                          //       LSTM (i, f, g, o) after activation, GRU (r, z, n, W_hn h + b_hn)
  float* aux;             // [N, ndir*H]  LSTM: c_t (written forward, read backward); GRU: the h_{t-1} that
                          //       entered step t (backward input)
  // backward
  const float* dy;        // [N, ndir*H]
  float* dg;              // [N, ndir*G*H] LSTM: gradient wrt the pre-activation gates; GRU: dGi, wrt gin
  float* dg2;             // GRU: [N, ndir*3H] dGh, wrt the hidden projections (da_r, da_z, da_n * r)
  int step;
  int ksplit, kiter;      // K is split over `ksplit` waves, `kiter` steps of 16 k each
  int nact, nact_next;    // rows active at this step / at step + 1 (a prefix: rows are sorted)
  int row_base;           // row_off[step], from the host's copy of the lengths (no table read)
  int row_base_prev;      // row_off[step - 1] (LSTM backward: c_{t-1} of the forward direction)
  int act;                // vanilla RNN: ITTS_ACT_TANH or ITTS_ACT_RELU
};

// packed row that row b visits at the step being processed / the one before it (the caller knows that it is
// active): the forward direction's rows follow from the host-side offsets, only the reverse direction reads its table
__device__ __forceinline__ int row_now(const RnnStepArgs& a, int dir, int b) {
  return dir == 0 ? a.row_base + b : a.rev_row[(size_t)a.step * a.B + b];
}
__device__ __forceinline__ int row_before(const RnnStepArgs& a, int dir, int b) {
  return dir == 0 ? a.row_base_prev + b : a.rev_row[(size_t)(a.step - 1) * a.B + b];
}

// ---- forward step -----------------------------------------------------------------------------------
// Workgroup = 4 hidden units x G gates (tile row = gate * 4 + unit; rows 12..15 of the GRU's re-tiled W_hh are
// zero) x every active batch tile.  Its 4 waves split K = H four ways; a wave loads its W_hh fragments once, then
// the h_{t-1} fragments of NT batch tiles of 16 rows, straight from L2 into registers (every element feeds exactly
// one MFMA, so there is no LDS staging).  The partial 16x16 tiles are reduced through LDS and thread
// (tile, row, unit) applies the cell update.
// Grid: (H/4, ndir) -> 256 workgroups for H = 512; W_hh traffic does not grow with the batch.
// What differs between the cells besides the update itself -- each as it was tuned, both kept:
//   * NC accumulator chains per tile: the LSTM gives each component of a float4 its own (an MFMA never waits for
//     its predecessor), the GRU has two (x, z and y, w).  NC decides the rounding of h.
//   * the LSTM requests gin behind tile 0's MFMAs and pulls the next step's rev_row line into L2; the GRU requests
//     gin and b_hh together with the state loads.  No effect on results.
template <int G, int NT>
__global__ __launch_bounds__(256) void rnn_step_fwd_kernel(RnnStepArgs a) {
  constexpr int NC = G == 4 ? 4 : 2;
  __shared__ float P[NT][4][16][17];
  const int H = a.H, B = a.B, GH = G * H;
  const int dir = blockIdx.y;
  const int j0 = blockIdx.x * FW_UNITS;
  const int par = a.step & 1;
  const size_t dsz = (size_t)B * H;
  const size_t cur = ((size_t)par * a.ndir + dir) * dsz, nxt = ((size_t)(par ^ 1) * a.ndir + dir) * dsz;
  const float* hprev = a.hs + cur;
  float* hnext = a.hs + nxt;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  const int ntiles = (a.nact + 15) >> 4;

  // K split over a.ksplit waves, a.kiter steps of 16 k (4 k-blocks) each, in chunks of 8 steps
  const int kiter = wv < a.ksplit ? a.kiter : 0;
  const int kb0 = wv * 4 * a.kiter + kg;                       // this lane's first k-block
  const float4* wp = reinterpret_cast<const float4*>(a.wp) +
                     (((size_t)dir * (H / 4) + blockIdx.x) * (H / 4) + (kiter ? kb0 : 0)) * 16 + lr;
  const float4* hp4 = reinterpret_cast<const float4*>(hprev);

  for (int tb = 0; tb < ntiles; tb += NT) {
    f32x4 acc[NT][NC];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int n = 0; n < NC; ++n) acc[tt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    // elementwise operands of thread (tile q, batch row bl, unit u); their loads are issued behind
    // the first chunk's operand loads (loads return in order)
    const int q = threadIdx.x >> 6, bl = (threadIdx.x >> 2) & 15, u = threadIdx.x & 3;
    const int b = (tb + q) * 16 + bl, j = j0 + u;
    const bool ew = q < NT && b < B && tb + q < ntiles;   // rows of a launched tile
    const bool act = ew && b < a.nact;
    const size_t sidx = ((size_t)blockIdx.x * B + (ew ? b : 0)) * 4 + u;   // blocked(b, j)
    float hp_v = 0.f, cp_v = 0.f, x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f, bh0 = 0.f, bh1 = 0.f, bh2 = 0.f;
    // The packed-row index heads the only dependent load chain of a step (index -> gin row): it
    // is requested before the 40 operand loads, which then cover its latency, and (LSTM) the gin loads
    // that need it are covered by the MFMAs (measured before: the first MFMA waited ~7 000 clocks
    // for index + gin issued behind each other in front of it).
    const int ridx = act ? row_now(a, dir, b) : 0;
    // ... and (LSTM) the table row of the NEXT step is pulled into this XCD's L2 now (256 B that every
    // workgroup of the reverse direction needs: whichever XCD it lands on next time finds it there;
    // cold, that one load was ~6 000 clocks at the head of every step)
    int pf = 0;
    if (G == 4 && tb == 0 && dir == 1 && a.step + 1 < a.T && (int)threadIdx.x < B)
      pf = a.rev_row[(size_t)(a.step + 1) * B + threadIdx.x];
    __builtin_amdgcn_sched_barrier(0);
    size_t r = 0;
    auto load_projections = [&]() {
      r = (size_t)ridx;
      const float* gi = a.gin + r * (size_t)(a.ndir * GH) + (size_t)dir * GH + j;
      x0 = gi[0]; x1 = gi[H]; x2 = gi[2 * H];
      if constexpr (G == 4) {
        x3 = gi[3 * H];
      } else {
        const float* bh = a.bhh + (size_t)dir * GH + j;
        bh0 = bh[0]; bh1 = bh[H]; bh2 = bh[2 * H];
      }
    };
#pragma unroll 1
    for (int c = 0; c < kiter || c == 0; c += 8) {
      float4 bv[8], av[NT][8];
#pragma unroll
      for (int s = 0; s < 8; ++s) bv[s] = wp[(size_t)(c + s < kiter ? 4 * (c + s) : 0) * 16];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int row = (tb + tt) * 16 + lr;
        const float4* hp = hp4 + (size_t)(kiter ? kb0 : 0) * B + (row < B ? row : 0);
#pragma unroll
        for (int s = 0; s < 8; ++s) av[tt][s] = hp[(size_t)(c + s < kiter ? 4 * (c + s) : 0) * B];
      }
      if (c == 0 && ew) {
        hp_v = hprev[sidx];
        if constexpr (G == 4) cp_v = a.cs[cur + sidx];
        else if (act) load_projections();
      }
      __builtin_amdgcn_sched_barrier(0);   // all loads above are in flight before the first MFMA
      // tile-outermost order: the MFMAs of tile 0 start as soon as ITS operands are there, while
      // the loads of the later tiles are still in flight (k-step-outermost, with 2 * NT independent
      // accumulator chains, measured 9 % slower)
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const bool rok = (tb + tt) * 16 + lr < B;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          float4 x = av[tt][s];
          if (!rok || c + s >= kiter) x = make_float4(0.f, 0.f, 0.f, 0.f);
          acc[tt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, bv[s].x, acc[tt][0], 0, 0, 0);
          acc[tt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, bv[s].y, acc[tt][1], 0, 0, 0);
          acc[tt][2 % NC] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, bv[s].z, acc[tt][2 % NC], 0, 0, 0);
          acc[tt][3 % NC] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, bv[s].w, acc[tt][3 % NC], 0, 0, 0);
        }
        if (G == 4 && tt == 0 && c == 0) {
          // the input projections of this element are requested here: the index (the oldest
          // outstanding load) is back once tile 0's operands are, and the remaining tiles' MFMAs
          // cover the latency of these loads
          __builtin_amdgcn_sched_barrier(0);
          if (act) load_projections();
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (tb > 0) __syncthreads();   // P of the previous group has been consumed
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (NC == 4) P[tt][wv][kg * 4 + e][lr] = (acc[tt][0][e] + acc[tt][1][e]) + (acc[tt][2][e] + acc[tt][3][e]);
        else P[tt][wv][kg * 4 + e][lr] = acc[tt][0][e] + acc[tt][1][e];
      }
    }
    __syncthreads();
    if (ew) {
      float hn = hp_v, cn = cp_v;
      if (act) {
        const int qq = q < NT ? q : 0;
        auto proj = [&](int n) {
          return (P[qq][0][bl][n] + P[qq][1][bl][n]) + (P[qq][2][bl][n] + P[qq][3][bl][n]);
        };
        float s0, s1, s2, s3;      // the saved values
        if constexpr (G == 4)
          lstm_cell_fwd(proj(u), proj(4 + u), proj(8 + u), proj(12 + u), x0, x1, x2, x3, cn, hn, s0, s1, s2, s3);
        else
          gru_cell_fwd(proj(u), proj(4 + u), proj(8 + u), x0, x1, x2, bh0, bh1, bh2, hn, s0, s1, s2, s3);
        const size_t oh = r * (size_t)(a.ndir * H) + (size_t)dir * H + j;
        a.y[oh] = hn;
        if (a.gates) {
          reinterpret_cast<float4*>(a.gates)[(r * a.ndir + dir) * H + j] = make_float4(s0, s1, s2, s3);
          if constexpr (G == 4) a.aux[oh] = cn;
        }
      }
      hnext[sidx] = hn;
      if constexpr (G == 4) a.cs[nxt + sidx] = cn;
    }
    if (pf == 0x7fffffff) hnext[0] = 0.f;    // never true: keeps the prefetch load alive
  }
}

// The vanilla RNN's forward step.  One gate: workgroup = 16 hidden units (tile row = unit) x every active batch tile,
// grid (H/16, ndir) -- no tile row is padding (laid out like the GRU, 4 units x 4 gate slots, three quarters of the W_hh
// stream and of the MFMAs would be zeros).  K split, operand loads and their order, tile-outermost MFMAs with four
// chains and the reduction through LDS are those of rnn_step_fwd_kernel; thread (batch row bl, unit n) then applies the
// cell to its element of each of the NT tiles.  A row of a launched tile that is no longer active only has its state
// copied to the other parity.
template <int NT>
__global__ __launch_bounds__(256) void rnn1_step_fwd_kernel(RnnStepArgs a) {
  __shared__ float P[NT][4][16][17];
  const int H = a.H, B = a.B;
  const int dir = blockIdx.y;
  const int par = a.step & 1;
  const size_t dsz = (size_t)B * H;
  const float* hprev = a.hs + ((size_t)par * a.ndir + dir) * dsz;
  float* hnext = a.hs + ((size_t)(par ^ 1) * a.ndir + dir) * dsz;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  const int ntiles = (a.nact + 15) >> 4;

  const int kiter = wv < a.ksplit ? a.kiter : 0;
  const int kb0 = wv * 4 * a.kiter + kg;                       // this lane's first k-block
  const float4* wp = reinterpret_cast<const float4*>(a.wp) +
                     (((size_t)dir * (H / FW_UNITS_1) + blockIdx.x) * (H / 4) + (kiter ? kb0 : 0)) * 16 + lr;
  const float4* hp4 = reinterpret_cast<const float4*>(hprev);
  const int bl = threadIdx.x >> 4, j = blockIdx.x * FW_UNITS_1 + (threadIdx.x & 15);

  for (int tb = 0; tb < ntiles; tb += NT) {
    f32x4 acc[NT][4];
    int ridx[NT];
    float hp_v[NT], x[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[tt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      // the packed-row index heads the only dependent load chain of a step: requested before the operand loads
      const int b = (tb + tt) * 16 + bl;
      ridx[tt] = b < a.nact ? row_now(a, dir, b) : 0;
      hp_v[tt] = 0.f; x[tt] = 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
    for (int c = 0; c < kiter || c == 0; c += 8) {
      float4 bv[8], av[NT][8];
#pragma unroll
      for (int s = 0; s < 8; ++s) bv[s] = wp[(size_t)(c + s < kiter ? 4 * (c + s) : 0) * 16];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int row = (tb + tt) * 16 + lr;
        const float4* hp = hp4 + (size_t)(kiter ? kb0 : 0) * B + (row < B ? row : 0);
#pragma unroll
        for (int s = 0; s < 8; ++s) av[tt][s] = hp[(size_t)(c + s < kiter ? 4 * (c + s) : 0) * B];
      }
      if (c == 0) {
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          const int b = (tb + tt) * 16 + bl;
          if (b < a.nact) x[tt] = a.gin[(size_t)ridx[tt] * (a.ndir * H) + (size_t)dir * H + j];
          else if (b < B && tb + tt < ntiles) hp_v[tt] = hprev[blocked(b, j, B)];
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // all loads above are in flight before the first MFMA
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const bool rok = (tb + tt) * 16 + lr < B;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          float4 v = av[tt][s];
          if (!rok || c + s >= kiter) v = make_float4(0.f, 0.f, 0.f, 0.f);
          acc[tt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, bv[s].x, acc[tt][0], 0, 0, 0);
          acc[tt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, bv[s].y, acc[tt][1], 0, 0, 0);
          acc[tt][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.z, bv[s].z, acc[tt][2], 0, 0, 0);
          acc[tt][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.w, bv[s].w, acc[tt][3], 0, 0, 0);
        }
      }
    }
    if (tb > 0) __syncthreads();   // P of the previous group has been consumed
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        P[tt][wv][kg * 4 + e][lr] = (acc[tt][0][e] + acc[tt][1][e]) + (acc[tt][2][e] + acc[tt][3][e]);
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      const int b = (tb + tt) * 16 + bl, n = threadIdx.x & 15;
      if (b >= B || tb + tt >= ntiles) continue;
      float hn = hp_v[tt];
      if (b < a.nact) {
        hn = rnn_cell_fwd((P[tt][0][bl][n] + P[tt][1][bl][n]) + (P[tt][2][bl][n] + P[tt][3][bl][n]), x[tt], a.act);
        a.y[(size_t)ridx[tt] * (a.ndir * H) + (size_t)dir * H + j] = hn;
      }
      hnext[blocked(b, j, B)] = hn;
    }
  }
}

// ---- backward step ----------------------------------------------------------------------------------
// Processes recurrence step s = a.step (called with s = T-1 ... 0). For row b active at s:
//   dh = dy[t] + dG[t_{s+1}] W_hh   (second term only if the row is active at s+1; GRU: dGh, and + the carry)
//   the cell's gate gradients (rnn_common.h) -> dG[t] and the running carry (LSTM: dc * f in the cs buffers,
//   GRU: dh * z in the hs buffers; parity by step; the vanilla RNN, G = 1, has none and reads only y and dy)
// dG (GRU: dGh) of a step is written twice: row-major for the dW / dX GEMMs and K-blocked into dgb,
// which is what the next launch reads as its MFMA operand.
// Workgroup = 16 hidden units x 16 batch rows; up to 4 G waves split the K = G H gate rows so that
// a wave has at most 8 k-steps (16 operand loads) per chunk, all in flight at once.  A workgroup has at least
// the four waves the cell update needs (16 rows x 16 units), so with the GRU's ksplit = 3 the fourth takes no part
// in the product.
// Grid (H/16 * ceil(nact/16), ndir).
template <int G>
__global__ __launch_bounds__(256 * G) void rnn_step_bwd_kernel(RnnStepArgs a) {
  __shared__ float P[4 * G][16][17];
  const int H = a.H, B = a.B, GH = G * H;
  const int dir = blockIdx.y;
  const int ngroups = H / BW_UNITS;
  const int jg = blockIdx.x % ngroups;
  const int j0 = jg * BW_UNITS;
  const int b0 = (blockIdx.x / ngroups) * 16;
  const int par = a.step & 1;
  const size_t dsz = (size_t)B * H;
  float* carry_buf = G == 4 ? a.cs : a.hs;
  const float* carry_in = carry_buf + ((size_t)(par ^ 1) * a.ndir + dir) * dsz;
  float* carry_out = carry_buf + ((size_t)par * a.ndir + dir) * dsz;
  const float* dgb_in = a.dgb + ((size_t)(par ^ 1) * a.ndir + dir) * G * dsz;
  float* dgb_out = a.dgb + ((size_t)par * a.ndir + dir) * G * dsz;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  const size_t ldg = (size_t)a.ndir * GH, ldh = (size_t)a.ndir * H;

  // dh_rec tile: A = dG of the next recurrence step (rows b0..b0+15, K-blocked), B = W_hh^T rows
  // of our 16 units (re-tiled)
  const int row = b0 + lr;
  const bool has_next = row < a.nact_next;
  const int kiter = wv < a.ksplit ? a.kiter : 0;      // G H gate rows / waves / 16 per step
  const int kb0 = (kiter ? wv * 4 * kiter : 0) + kg;
  const float4* ap = reinterpret_cast<const float4*>(dgb_in) + (size_t)kb0 * B + (row < B ? row : 0);
  const float4* wp = reinterpret_cast<const float4*>(a.wp) +
                     (((size_t)dir * ngroups + jg) * (size_t)(GH / 4) + kb0) * 16 + lr;   // K/4 blocks

  // elementwise operands (thread -> batch row bl, unit n)
  const int bl = (threadIdx.x >> 4) & 15, n = threadIdx.x & 15;
  const int b = b0 + bl, j = j0 + n;
  const bool ew = threadIdx.x < 256 && b < B;
  const bool act = ew && b < a.nact;
  // gs: the saved gates; v1: LSTM c_t, GRU h_{t-1}, RNN y_t; v2: LSTM c_{t-1}
  float4 gs = make_float4(0.f, 0.f, 0.f, 0.f);
  float v1 = 0.f, v2 = 0.f, dyv = 0.f, carry = 0.f;
  // packed-row indices first (see the forward kernel): the saved tensors they address are then
  // requested behind the operand loads, under the MFMAs
  const int ridx = act ? row_now(a, dir, b) : 0;
  const int rpidx = (G == 4 && act && a.step > 0) ? row_before(a, dir, b) : 0;
  __builtin_amdgcn_sched_barrier(0);
  size_t r = 0;

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc2 = {0.f, 0.f, 0.f, 0.f}, acc3 = {0.f, 0.f, 0.f, 0.f};   // four independent chains
#pragma unroll 1
  for (int c = 0; c < kiter || c == 0; c += 8) {
    float4 av[8], bv[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const size_t o = c + s < kiter ? 4 * (c + s) : 0;
      av[s] = ap[o * B];
      bv[s] = wp[o * 16];
    }
    if (c == 0 && act) {
      r = (size_t)ridx;
      if constexpr (G == 1) {
        v1 = a.y[r * ldh + (size_t)dir * H + j];
      } else {
        gs = reinterpret_cast<const float4*>(a.gates)[(r * a.ndir + dir) * H + j];
        v1 = a.aux[r * ldh + (size_t)dir * H + j];
      }
      if constexpr (G == 4)
        v2 = a.step > 0 ? a.aux[(size_t)rpidx * ldh + (size_t)dir * H + j] : (a.c0 ? a.c0[dir * H + j] : 0.f);
      dyv = a.dy[r * ldh + (size_t)dir * H + j];
      if constexpr (G != 1) carry = carry_in[(size_t)b * H + j];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      float4 x = av[s];
      if (!has_next || c + s >= kiter) x = make_float4(0.f, 0.f, 0.f, 0.f);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, bv[s].x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, bv[s].y, acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, bv[s].z, acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, bv[s].w, acc3, 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) P[wv][kg * 4 + q][lr] = (acc0[q] + acc1[q]) + (acc2[q] + acc3[q]);
  __syncthreads();
  if (ew) {
    if (act) {
      float dhr = 0.f;
      for (int w = 0; w < a.ksplit; ++w) dhr += P[w][bl][n];
      float d[4];      // what goes K-blocked to the next launch: dG, GRU dGh
      float* dgo = a.dg + r * ldg + (size_t)dir * GH + j;
      if constexpr (G == 4) {
        lstm_cell_bwd(gs.x, gs.y, gs.z, gs.w, v1, v2, dyv + dhr, carry, d[0], d[1], d[2], d[3]);
        dgo[0] = d[0]; dgo[H] = d[1]; dgo[2 * H] = d[2]; dgo[3 * H] = d[3];
      } else if constexpr (G == 3) {
        float dan;
        gru_cell_bwd(gs.x, gs.y, gs.z, gs.w, v1, dyv + dhr, carry, d[0], d[1], dan, d[2]);
        float* gh = a.dg2 + r * ldg + (size_t)dir * GH + j;
        dgo[0] = d[0]; dgo[H] = d[1]; dgo[2 * H] = dan;
        gh[0] = d[0]; gh[H] = d[1]; gh[2 * H] = d[2];
      } else {
        d[0] = rnn_cell_bwd(v1, dyv + dhr, a.act);
        dgo[0] = d[0];
      }
#pragma unroll
      for (int g = 0; g < G; ++g) dgb_out[blocked(b, g * H + j, B)] = d[g];
    }
    if constexpr (G != 1) carry_out[(size_t)b * H + j] = carry;      // 0 for a row that is not active yet
  }
}

// ---- host driver ------------------------------------------------------------------------------------
// Forward recurrence: one launch per step, kernels[n - 1] taking n batch tiles of 16 rows per pass (NT = 1 .. 4).
// Each workgroup owns `units` hidden units.
static void rnn_fwd_steps(void (*const kernels[4])(RnnStepArgs), int units, RnnStepArgs& a, const int* h_lengths,
                          hipStream_t s) {
  int p = a.B;
  int row_base = 0;
  for (int step = 0; step < a.T; ++step) {
    a.step = step;
    a.nact = rnn_active_rows(h_lengths, a.B, step, &p);
    a.row_base = row_base;          // row_off[step] = rows active in all earlier steps
    row_base += a.nact;
    hipLaunchKernelGGL(kernels[std::min((a.nact + 15) / 16, 4) - 1], dim3(a.H / units, a.ndir), dim3(256), 0, s, a);
  }
}

// Backward recurrence, steps T - 1 .. 0: workgroups of 16 hidden units x one 16-row batch tile, 64 * a.ksplit threads
// each -- and never fewer than the 256 the cell update of a tile takes (the GRU's ksplit = 3: with 192 threads rows
// 12 .. 15 of every tile were left out).
static void rnn_bwd_steps(void (*kernel)(RnnStepArgs), RnnStepArgs& a, const int* h_lengths, hipStream_t s) {
  const std::vector<int> row_off = rnn_row_offsets(h_lengths, a.T, a.B);
  int p = 0, nact_next = 0;
  for (int step = a.T - 1; step >= 0; --step) {
    a.step = step;
    a.nact = rnn_active_rows(h_lengths, a.B, step, &p);
    a.nact_next = nact_next;
    nact_next = a.nact;
    a.row_base = row_off[step];
    a.row_base_prev = step > 0 ? row_off[step - 1] : 0;
    hipLaunchKernelGGL(kernel, dim3((a.H / BW_UNITS) * ((a.nact + 15) / 16), a.ndir),
                       dim3(std::max(64 * a.ksplit, 256)), 0, s, a);
  }
}

// d_state of any cell: [hs | cs (LSTM only) | dgb, G st | re-tiled W_hh, ndir*4H*H (the GRU's forward tiling pads
// the 4th gate; the vanilla RNN's one gate: ndir*H*H)] floats, st = 2*ndir*B*H (two parities)
static inline int64_t rnn_state_bytes(int G, int B, int H, int ndir) {
  if (B <= 0 || H <= 0 || ndir <= 0) return 0;
  const int nst = (G == 4 ? 2 : 1) + G;
  return ((int64_t)nst * 2 * ndir * B * H + (int64_t)ndir * (G == 1 ? 1 : 4) * H * H) * 4;
}
template <int G>
static float* rnn_carve_state(RnnStepArgs& a, void* d_state) {
  const size_t st = (size_t)2 * a.ndir * a.B * a.H;
  a.hs = reinterpret_cast<float*>(d_state);
  a.cs = G == 4 ? a.hs + st : nullptr;
  a.dgb = a.hs + (G == 4 ? 2 : 1) * st;
  float* wp = a.dgb + G * st;
  a.wp = wp;
  return wp;      // (writable: the caller re-tiles W_hh into it)
}

// The forward recurrence of one layer on the step kernels; `a` arrives with the geometry and the tensors of the call.
template <int G>
static int rnn_step_forward(RnnStepArgs a, const float* d_whh, const float* d_h0, const float* d_c0,
                            const int* d_lengths, const int* h_lengths, float* d_hn, float* d_cn, void* d_state,
                            hipStream_t s) {
  const int H = a.H, ndir = a.ndir;
  float* wp = rnn_carve_state<G>(a, d_state);
  const int64_t n = (int64_t)ndir * a.B * H;
  hipLaunchKernelGGL(rnn_pack_w_fwd_kernel, rnn_ew_grid((int64_t)ndir * H * H), dim3(256), 0, s, d_whh, wp, ndir, G, H);
  hipLaunchKernelGGL(rnn_init_state_kernel, rnn_ew_grid(n), dim3(256), 0, s, d_h0, a.hs, ndir, a.B, H);
  if (G == 4) hipLaunchKernelGGL(rnn_init_state_kernel, rnn_ew_grid(n), dim3(256), 0, s, d_c0, a.cs, ndir, a.B, H);
  ITTS_LAUNCH_CHECK();
  a.ksplit = (H % 64 == 0) ? 4 : ((H % 32 == 0) ? 2 : 1);
  a.kiter = H / (16 * a.ksplit);
  if constexpr (G == 1) {
    static void (*const step_kernels[4])(RnnStepArgs) = {rnn1_step_fwd_kernel<1>, rnn1_step_fwd_kernel<2>,
                                                         rnn1_step_fwd_kernel<3>, rnn1_step_fwd_kernel<4>};
    rnn_fwd_steps(step_kernels, FW_UNITS_1, a, h_lengths, s);
  } else {
    static void (*const step_kernels[4])(RnnStepArgs) = {rnn_step_fwd_kernel<G, 1>, rnn_step_fwd_kernel<G, 2>,
                                                         rnn_step_fwd_kernel<G, 3>, rnn_step_fwd_kernel<G, 4>};
    rnn_fwd_steps(step_kernels, FW_UNITS, a, h_lengths, s);
  }
  ITTS_LAUNCH_CHECK();
  if (d_hn) hipLaunchKernelGGL(rnn_final_state_kernel, rnn_ew_grid(n), dim3(256), 0, s, a.hs, d_lengths, d_hn, ndir, a.B, H);
  if (G == 4 && d_cn) hipLaunchKernelGGL(rnn_final_state_kernel, rnn_ew_grid(n), dim3(256), 0, s, a.cs, d_lengths, d_cn, ndir, a.B, H);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// The backward recurrence of one layer on the step kernels: fills a.dg (and the GRU's a.dg2) from a.dy and the saved
// forward tensors; d_d0, if given, receives the gradient of the initial state the carry belongs to (LSTM: c_0,
// GRU: h_0), [ndir][B][H].  The vanilla RNN has no carry and no d_d0.
template <int G>
static int rnn_step_backward(RnnStepArgs a, const float* d_whh, const int* h_lengths, float* d_d0, void* d_state,
                             hipStream_t s) {
  const int H = a.H, ndir = a.ndir;
  float* wp = rnn_carve_state<G>(a, d_state);
  float* carry = G == 4 ? a.cs : a.hs;
  hipLaunchKernelGGL(rnn_pack_w_bwd_kernel, rnn_ew_grid((int64_t)ndir * H * H), dim3(256), 0, s, d_whh, wp, ndir, G, H);
  ITTS_LAUNCH_CHECK();
  if (G != 1) ITTS_HIP_CHECK(hipMemsetAsync(carry, 0, (size_t)2 * ndir * a.B * H * 4, s));   // carry of rows that are not active yet
  a.ksplit = G * ((H % 64 == 0) ? 4 : ((H % 32 == 0) ? 2 : 1));   // waves that share K = G H: G H / 16 k-steps in all
  a.kiter = G * H / 16 / a.ksplit;
  rnn_bwd_steps(rnn_step_bwd_kernel<G>, a, h_lengths, s);
  ITTS_LAUNCH_CHECK();
  // step 0 has every row active and leaves its carry (LSTM dc * f, GRU dh * z), the gradient of the initial
  // state, in the parity-0 carry buffer [ndir][B][H]
  if (G != 1 && d_d0) ITTS_HIP_CHECK(hipMemcpyAsync(d_d0, carry, (size_t)ndir * a.B * H * 4, hipMemcpyDeviceToDevice, s));
  return ITTS_OK;
}

}  // namespace itts
