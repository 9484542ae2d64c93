// Classification: row-weighted softmax cross-entropy with its gradient in one pass over the logits, and the arg-max /
// confusion counts of the accuracy scores (torch.nn.CrossEntropyLoss under loss/NamedLoss.py with squeeze_inputs,
// loss/OneHotCrossEntropyLoss.py, loss/UnWeightedAccuracy.py and model_trainers/ClassificationTrainer.py of the
// reference).  All float32 logits, int64 targets and counts.
//
// The row math, the same in both layouts.  With m the row's largest logit, k the number of logits equal to m and
// s the sum of exp(x - m) over the OTHER logits,
//     lse - m = log1p((k - 1) + s),     softmax_c = (x_c == m ? 1 : exp(x_c - m)) / (k + s),
//     l = cw[t] * (log1p((k - 1) + s) - (x_t - m)),     softmax_t - 1 = -((k + s) - e_t) / (k + s).
// Counting the maxima instead of adding their exp(0) keeps a confidently correct row (s ~ 1e-6, x_t = m) at full
// relative precision: nothing is rounded against 1 before the logarithm, and x_t - m is exactly 0.
//
// Class-contiguous rows [N, C] (pitch ld): a row belongs to G = 1, 2, 4 .. 64 adjacent lanes of a wave, the
// smallest power of two with 4 G >= C, so a wave holds 64 / G rows at once (C <= 4: 64 rows a wave; C = 5 for
// instance: 32).  From C = 257 on the 64 lanes take S = 2, 4, 8 or 16 steps of 256 columns, the row kept in registers
// throughout (S * 4 floats a lane).  Lane i of a row owns the columns 4 (i + G j) .. + 3 of step j -- one 16-byte
// load where pitch and base allow, four plain loads otherwise: the same columns in the same lane either way -- and
// the G lanes combine by the xor butterfly, so a row's loss and gradient depend on the row and on nothing else: not
// on N, not on the row's index, not on the load form.
//
// Class-strided [B, C, T] (class c of frame (b, t) at b C T + c T + t): lanes run along t so that every load and
// store coalesces; the four waves of a workgroup share its 64 frames, each taking a quarter of the classes in ascending
// order, and combine through LDS in wave order.  Up to C = 256 a thread keeps its quarter (64 logits) in registers
// from the maximum to the gradient: the logits are read once; above that they are read again from the caches.
// The target is the arg-max over c of a one-hot tensor of the same layout at frame t + shift (lowest index among
// equal maxima, as torch.max(dim=1)); the frames t >= T - shift of the gradient are written as zeros.
//
// Rows of weight 0 are not read at all.  The weighted row losses are added in double: per lane in ascending row
// order, the lanes of a workgroup by the butterfly and then wave by wave, the workgroups by a second launch in one
// fixed order.  No float atomics: repeated calls give identical bits.  The counts are integers: their atomic adds
// commute.
#include <algorithm>
#include <math.h>

#include "common.h"
#include "row4.h"

namespace itts {
namespace {

constexpr int XE_WAVES = 4;
constexpr int XE_THREADS = XE_WAVES * kWave;
constexpr int64_t XE_MAX_BLOCKS = 4096;
constexpr int XE_MAX_C = 4096;
constexpr int XE_CONF_MAX_C = 1024;    // largest confusion matrix: 1024 x 1024 int64 = 8 MiB

// lanes of a row and steps of 4 * lanes columns
struct RowsPlan {
  int lanes, steps;
};

RowsPlan rows_plan(int C) {
  RowsPlan p{1, 1};
  while (4 * p.lanes < C && p.lanes < kWave) p.lanes *= 2;
  while (4 * p.lanes * p.steps < C) p.steps *= 2;
  return p;
}

int64_t rows_unit(int C) { return XE_WAVES * (int64_t)(kWave / rows_plan(C).lanes); }   // rows a workgroup holds at once
int64_t rows_per_block(int64_t N, int C) {
  const int64_t u = rows_unit(C);
  return u * std::max<int64_t>(1, (N + u * XE_MAX_BLOCKS - 1) / (u * XE_MAX_BLOCKS));
}
int64_t rows_blocks(int64_t N, int C) {
  const int64_t R = rows_per_block(N, C);
  return (N + R - 1) / R;
}

constexpr int XS_SLICES = 4;           // strided form: the waves of a workgroup, a quarter of the classes each
constexpr int XS_FRAMES = kWave;       // .. its frames, one per lane
constexpr int XS_THREADS = XS_SLICES * kWave;
constexpr int XS_KEEP = 64;            // logits a thread keeps in registers: up to 4 * 64 classes
int64_t strided_chunks(int64_t T) { return (T + XS_FRAMES - 1) / XS_FRAMES; }

// l of the header's formula from the row's maximum, the count of maxima, the sum over the others and the target's
// logit
__device__ __forceinline__ float row_loss(float m, float k, float s, float xt, float cwt) {
  return cwt * (log1pf((k - 1.f) + s) - (xt - m));
}

// softmax_c - [c == t] from e = (x_c == m ? 1 : exp(x_c - m)) and den = k + s.  At the target it is minus the OTHER
// classes' share, (den - e) / den, with den - 1 taken as (k - 1) + s where e is 1: a confidently correct row keeps its
// small gradient at full relative precision instead of rounding softmax_t against 1
__device__ __forceinline__ float row_grad(float e, bool target, float k, float s, float den) {
  if (!target) return e / den;
  return -((e == 1.f ? (k - 1.f) + s : den - e) / den);
}

struct XentArgs {
  const float* x; int64_t ld;
  const int64_t* target;
  const float* cw;
  const float* w;
  float* elem;
  float* grad; int64_t ldg;
  double* partial;              // [blocks]
  int64_t N, rows;              // rows: of a workgroup
  int64_t ignore;
  int C;
};

template <int G, int S, bool VEC>
__global__ __launch_bounds__(XE_THREADS) void xent_rows_kernel(XentArgs a) {
  __shared__ double wsum[XE_WAVES];
  constexpr int RPW = kWave / G;                // rows a wave holds at once
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, grp = lane / G;
  const int64_t r0 = (int64_t)blockIdx.x * a.rows, r1 = min(a.N, r0 + a.rows);
  const float ninf = -INFINITY;
  double acc = 0.0;
  for (int64_t rb = r0 + wave * RPW; rb < r1; rb += XE_WAVES * RPW) {
    const int64_t r = rb + grp;
    const bool have = r < r1;
    const float wr = have ? a.w[r] : 0.f;
    const int64_t t = have ? a.target[r] : 0;
    const bool live = have && wr != 0.f && t != a.ignore;       // rows of weight 0 may hold anything: never read
    const bool valid = t >= 0 && t < a.C;
    const float* row = a.x + r * a.ld;
    float v[S][4];
    float m = ninf;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int col = 4 * (sub + G * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[j][k] = ninf;
      if (live) load4<VEC>(row, col, a.C, v[j]);
#pragma unroll
      for (int k = 0; k < 4; ++k) m = fmaxf(m, v[j][k]);        // (columns from C on hold -inf)
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float cnt = 0.f, s = 0.f;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int col = 4 * (sub + G * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x = v[j][k];
        float e = 0.f;
        if (col + k < a.C) {
          if (x == m) { e = 1.f; cnt += 1.f; }
          else { e = expf(x - m); s += e; }
        }
        v[j][k] = e;
      }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      cnt += __shfl_xor(cnt, off, 64);
      s += __shfl_xor(s, off, 64);
    }
    float l = 0.f, scale = 0.f;
    if (live) {
      if (valid) {
        const float cwt = a.cw ? a.cw[t] : 1.f;
        l = wr * row_loss(m, cnt, s, row[t], cwt);
        scale = wr * cwt;
      } else {
        l = NAN;                                               // a target outside [0, C): reported, never dereferenced
      }
    }
    if (a.grad && have) {
      const float den = cnt + s;
      const bool on = live && valid;
      float* grow = a.grad + r * a.ldg;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const int col = 4 * (sub + G * j);
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = on ? scale * row_grad(v[j][k], col + k == t, cnt, s, den) : 0.f;
        store4<VEC>(grow, col, a.C, g);
      }
    }
    if (sub == 0 && have) {
      if (a.elem) a.elem[r] = l;
      acc += (double)l;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// torch's order of an arg-max: a NaN beats every number, the lower index wins among equals (and among NaNs)
__device__ __forceinline__ bool beats(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av > bv || (av == bv && ai < bi);
}

struct XentStridedArgs {
  const float* x;
  const float* onehot;
  const float* cw;
  const float* w;
  float* elem;
  float* grad;
  double* partial;              // [B][chunks]
  int64_t T, Tn;                // frames of the tensors / of the loss (T - shift)
  int64_t ignore;
  int C, shift;
};

// The four waves of a workgroup share 64 frames: lane = frame, wave = a quarter of the classes (c0 .. c1), combined
// through LDS in wave order.  KEEP (C <= 256): a thread's up to 64 logits stay in registers from the maximum to the
// gradient, the logits are read once; else they are read again from the caches.
template <bool KEEP>
__global__ __launch_bounds__(XS_THREADS) void xent_strided_kernel(XentStridedArgs a) {
  __shared__ float sbest[XS_SLICES][XS_FRAMES], smax[XS_SLICES][XS_FRAMES], scnt[XS_SLICES][XS_FRAMES],
      ssum[XS_SLICES][XS_FRAMES];
  __shared__ int sidx[XS_SLICES][XS_FRAMES];
  __shared__ double red[16];
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * XS_FRAMES + lane;
  const int64_t b = blockIdx.y;
  const bool have = t < a.Tn;
  const int64_t r = b * a.Tn + t;
  const int64_t base = b * a.C * a.T + t;
  const int per = (a.C + XS_SLICES - 1) / XS_SLICES;
  const int c0 = min(a.C, slice * per), c1 = min(a.C, c0 + per);
  const float wr = have ? a.w[r] : 0.f;
  const bool mine = have && wr != 0.f;          // (the same in the four waves of a frame)
  // the target: arg-max of the one-hot frame t + shift; an empty slice holds (-inf, no index), which nothing loses to
  float best = -INFINITY;
  int tgt = 0x7fffffff;
  if (mine) {
    const float* hp = a.onehot + base + a.shift;
#pragma unroll 8
    for (int c = c0; c < c1; ++c) {
      const float h = hp[(int64_t)c * a.T];
      if (beats(h, c, best, tgt)) { best = h; tgt = c; }
    }
  }
  sbest[slice][lane] = best;
  sidx[slice][lane] = tgt;
  __syncthreads();
  best = sbest[0][lane];
  tgt = sidx[0][lane];
#pragma unroll
  for (int k = 1; k < XS_SLICES; ++k)
    if (beats(sbest[k][lane], sidx[k][lane], best, tgt)) { best = sbest[k][lane]; tgt = sidx[k][lane]; }
  const bool live = mine && (int64_t)tgt != a.ignore;
  const float* xp = a.x + base;
  float v[XS_KEEP];
  float m = -INFINITY;
  if (live) {
    if (KEEP) {
#pragma unroll
      for (int i = 0; i < XS_KEEP; ++i) {
        v[i] = -INFINITY;
        if (c0 + i < c1) v[i] = xp[(int64_t)(c0 + i) * a.T];
        m = fmaxf(m, v[i]);
      }
    } else {
#pragma unroll 8
      for (int c = c0; c < c1; ++c) m = fmaxf(m, xp[(int64_t)c * a.T]);
    }
  }
  smax[slice][lane] = m;
  __syncthreads();
  m = fmaxf(fmaxf(smax[0][lane], smax[1][lane]), fmaxf(smax[2][lane], smax[3][lane]));
  float cnt = 0.f, s = 0.f;
  if (live) {
    if (KEEP) {
#pragma unroll
      for (int i = 0; i < XS_KEEP; ++i)
        if (c0 + i < c1) {
          if (v[i] == m) { v[i] = 1.f; cnt += 1.f; }
          else { v[i] = expf(v[i] - m); s += v[i]; }
        }
    } else {
#pragma unroll 8
      for (int c = c0; c < c1; ++c) {
        const float x = xp[(int64_t)c * a.T];
        if (x == m) cnt += 1.f;
        else s += expf(x - m);
      }
    }
  }
  scnt[slice][lane] = cnt;
  ssum[slice][lane] = s;
  __syncthreads();
  cnt = ((scnt[0][lane] + scnt[1][lane]) + scnt[2][lane]) + scnt[3][lane];
  s = ((ssum[0][lane] + ssum[1][lane]) + ssum[2][lane]) + ssum[3][lane];
  const float den = cnt + s;
  float l = 0.f, scale = 0.f;
  if (live) {
    const float cwt = a.cw ? a.cw[tgt] : 1.f;
    scale = wr * cwt;
    if (slice == 0) l = wr * row_loss(m, cnt, s, xp[(int64_t)tgt * a.T], cwt);
  }
  if (a.grad && t < a.T) {
    float* gp = a.grad + base;
    if (live) {
      if (KEEP) {
#pragma unroll
        for (int i = 0; i < XS_KEEP; ++i)
          if (c0 + i < c1) gp[(int64_t)(c0 + i) * a.T] = scale * row_grad(v[i], c0 + i == tgt, cnt, s, den);
      } else {
#pragma unroll 8
        for (int c = c0; c < c1; ++c) {
          const float x = xp[(int64_t)c * a.T];
          gp[(int64_t)c * a.T] = scale * row_grad(x == m ? 1.f : expf(x - m), c == tgt, cnt, s, den);
        }
      }
    } else {
#pragma unroll 8
      for (int c = c0; c < c1; ++c) gp[(int64_t)c * a.T] = 0.f;
    }
  }
  if (slice == 0 && have && a.elem) a.elem[r] = l;
  const double tot = block_sum((double)l, red);         // (l is 0 in the waves 1 .. 3)
  if (threadIdx.x == 0) a.partial[b * gridDim.x + blockIdx.x] = tot;
}

template <int G, int S>
void launch_rows(const XentArgs& a, bool vec, int nb, hipStream_t s) {
  if (vec) xent_rows_kernel<G, S, true><<<dim3(nb), XE_THREADS, 0, s>>>(a);
  else xent_rows_kernel<G, S, false><<<dim3(nb), XE_THREADS, 0, s>>>(a);
}

// ---- arg-max and confusion counts ------------------------------------------------------------------------------
struct CountArgs {
  const float* x; int64_t ld;
  const int64_t* target;
  int64_t* pred;
  unsigned long long* correct;
  unsigned long long* conf;
  int64_t N;
  int C;
};

// G = the largest power of two <= min(C, 64) lanes a row: lane i scans the classes i, i + G, .. in ascending order
template <int G>
__global__ __launch_bounds__(XE_THREADS) void class_counts_kernel(CountArgs a) {
  constexpr int RPW = kWave / G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, grp = lane / G;
  const int64_t r = ((int64_t)blockIdx.x * XE_WAVES + wave) * RPW + grp;
  const bool have = r < a.N;
  float bv = 0.f;
  int bi = sub;
  if (have) {
    const float* row = a.x + r * a.ld;
    bv = row[sub];
    for (int c = sub + G; c < a.C; c += G) {
      const float v = row[c];
      if (beats(v, c, bv, bi)) { bv = v; bi = c; }
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (!have || sub != 0) return;
  if (a.pred) a.pred[r] = bi;
  if (!a.target) return;
  const int64_t t = a.target[r];
  if (t < 0 || t >= a.C) return;                   // counted nowhere
  if (a.correct && t == bi) atomicAdd(a.correct, 1ull);
  if (a.conf) atomicAdd(a.conf + t * a.C + bi, 1ull);
}

}  // namespace
}  // namespace itts

using namespace itts;

#define XENT_CHECK_C()                                                                                        \
  ITTS_REQUIRE(C >= 1 && C <= XE_MAX_C, "C = " + std::to_string(C) + " is outside 1 .. " + std::to_string(XE_MAX_C))

extern "C" int itts_xent_plan(int64_t N, int C, int layout, int* lanes, int* steps) {
  if (N < 0 || C < 1 || C > XE_MAX_C || (layout != ITTS_XENT_ROWS && layout != ITTS_XENT_STRIDED)) return -1;
  const RowsPlan p = rows_plan(C);
  if (lanes) *lanes = layout == ITTS_XENT_ROWS ? p.lanes : XS_SLICES;
  if (steps) *steps = layout == ITTS_XENT_ROWS ? p.steps : (C + XS_SLICES - 1) / XS_SLICES;
  return 0;
}

extern "C" int64_t itts_softmax_xent_workspace_bytes(int64_t N, int C) {
  if (N <= 0 || C < 1 || C > XE_MAX_C) return 0;
  return rows_blocks(N, C) * (int64_t)sizeof(double);
}

extern "C" int64_t itts_softmax_xent_strided_workspace_bytes(int B, int64_t T) {
  if (B <= 0 || T <= 0) return 0;
  return B * strided_chunks(T) * (int64_t)sizeof(double);
}

extern "C" int itts_softmax_xent(const float* d_x, int64_t ld, const int64_t* d_target, const float* d_cw,
                                 const float* d_w, int64_t N, int C, int64_t ignore_index, float* d_loss,
                                 float* d_elem, float* d_grad, int64_t ldg, void* d_workspace, void* stream) {
  XENT_CHECK_C();
  ITTS_REQUIRE(N >= 0, "N = " + std::to_string(N) + " is negative");
  ITTS_REQUIRE(ld >= C, "pitch ld = " + std::to_string(ld) + " is below the width " + std::to_string(C));
  if (d_grad) ITTS_REQUIRE(ldg >= C, "pitch ldg = " + std::to_string(ldg) + " is below the width " + std::to_string(C));
  ITTS_REQUIRE(d_loss, "null pointer (d_loss)");
  hipStream_t s = as_stream(stream);
  if (N == 0) {
    ITTS_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(float), s));
    return ITTS_OK;
  }
  ITTS_REQUIRE(d_x && d_target && d_w && d_workspace,
               "null pointer (d_x / d_target / d_w / d_workspace) with N = " + std::to_string(N));
  XentArgs a{};
  a.x = d_x; a.ld = ld; a.target = d_target; a.cw = d_cw; a.w = d_w; a.elem = d_elem; a.grad = d_grad; a.ldg = ldg;
  a.partial = reinterpret_cast<double*>(d_workspace);
  a.N = N; a.rows = rows_per_block(N, C); a.ignore = ignore_index; a.C = C;
  const bool vec = rows16(d_x, ld) && (!d_grad || rows16(d_grad, ldg));
  const int nb = (int)rows_blocks(N, C);
  const RowsPlan p = rows_plan(C);
  switch (p.lanes * 100 + p.steps) {
    case 101: launch_rows<1, 1>(a, vec, nb, s); break;
    case 201: launch_rows<2, 1>(a, vec, nb, s); break;
    case 401: launch_rows<4, 1>(a, vec, nb, s); break;
    case 801: launch_rows<8, 1>(a, vec, nb, s); break;
    case 1601: launch_rows<16, 1>(a, vec, nb, s); break;
    case 3201: launch_rows<32, 1>(a, vec, nb, s); break;
    case 6401: launch_rows<64, 1>(a, vec, nb, s); break;
    case 6402: launch_rows<64, 2>(a, vec, nb, s); break;
    case 6404: launch_rows<64, 4>(a, vec, nb, s); break;
    case 6408: launch_rows<64, 8>(a, vec, nb, s); break;
    case 6416: launch_rows<64, 16>(a, vec, nb, s); break;
    default: ITTS_REQUIRE(false, "no width class for C = " + std::to_string(C));
  }
  ITTS_LAUNCH_CHECK();
  return loss_final_sum(a.partial, nb, 1.0, d_loss, s);
}

extern "C" int itts_softmax_xent_strided(const float* d_x, const float* d_onehot, const float* d_cw,
                                         const float* d_w, int B, int C, int64_t T, int shift,
                                         int64_t ignore_index, float* d_loss, float* d_elem, float* d_grad,
                                         void* d_workspace, void* stream) {
  XENT_CHECK_C();
  ITTS_REQUIRE(B >= 0, "B = " + std::to_string(B) + " is negative");
  ITTS_REQUIRE(B <= 65535, "B = " + std::to_string(B) + " exceeds 65535");
  ITTS_REQUIRE(T >= 1, "T = " + std::to_string(T) + " is not positive");
  ITTS_REQUIRE(shift >= 0 && shift < T,
               "shift = " + std::to_string(shift) + " is outside 0 .. T - 1 = " + std::to_string(T - 1));
  ITTS_REQUIRE(strided_chunks(T) <= 0x7fffffff, "T = " + std::to_string(T) + " is too large");
  ITTS_REQUIRE(d_loss, "null pointer (d_loss)");
  hipStream_t s = as_stream(stream);
  if (B == 0) {
    ITTS_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(float), s));
    return ITTS_OK;
  }
  ITTS_REQUIRE(d_x && d_onehot && d_w && d_workspace,
               "null pointer (d_x / d_onehot / d_w / d_workspace) with B = " + std::to_string(B));
  XentStridedArgs a{};
  a.x = d_x; a.onehot = d_onehot; a.cw = d_cw; a.w = d_w; a.elem = d_elem; a.grad = d_grad;
  a.partial = reinterpret_cast<double*>(d_workspace);
  a.T = T; a.Tn = T - shift; a.ignore = ignore_index; a.C = C; a.shift = shift;
  const int64_t chunks = strided_chunks(T);
  if ((C + XS_SLICES - 1) / XS_SLICES <= XS_KEEP)
    xent_strided_kernel<true><<<dim3((unsigned)chunks, (unsigned)B), XS_THREADS, 0, s>>>(a);
  else
    xent_strided_kernel<false><<<dim3((unsigned)chunks, (unsigned)B), XS_THREADS, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return loss_final_sum(a.partial, chunks * B, 1.0, d_loss, s);
}

template <int G>
static void launch_counts(const CountArgs& a, hipStream_t s) {
  const int64_t rows = XE_WAVES * (int64_t)(kWave / G);
  class_counts_kernel<G><<<dim3((unsigned)((a.N + rows - 1) / rows)), XE_THREADS, 0, s>>>(a);
}

extern "C" int itts_class_counts(const float* d_x, int64_t ld, const int64_t* d_target, int64_t N, int C,
                                 int64_t* d_pred, int64_t* d_correct, int64_t* d_conf, void* stream) {
  XENT_CHECK_C();
  ITTS_REQUIRE(N >= 0, "N = " + std::to_string(N) + " is negative");
  ITTS_REQUIRE(N <= 0x7fffffff, "N = " + std::to_string(N) + " is too large");
  ITTS_REQUIRE(ld >= C, "pitch ld = " + std::to_string(ld) + " is below the width " + std::to_string(C));
  ITTS_REQUIRE(!d_conf || C <= XE_CONF_MAX_C, "a confusion matrix of C = " + std::to_string(C) +
                                                  " classes exceeds the " + std::to_string(XE_CONF_MAX_C) + " it takes");
  ITTS_REQUIRE(!(d_correct || d_conf) || d_target || N == 0, "null pointer (d_target): the counts need the true classes");
  if (N == 0) return ITTS_OK;
  ITTS_REQUIRE(d_x, "null pointer (d_x) with N = " + std::to_string(N));
  CountArgs a{};
  a.x = d_x; a.ld = ld; a.target = d_target; a.pred = d_pred;
  a.correct = reinterpret_cast<unsigned long long*>(d_correct);
  a.conf = reinterpret_cast<unsigned long long*>(d_conf);
  a.N = N; a.C = C;
  hipStream_t s = as_stream(stream);
  if (C >= 64) launch_counts<64>(a, s);
  else if (C >= 32) launch_counts<32>(a, s);
  else if (C >= 16) launch_counts<16>(a, s);
  else if (C >= 8) launch_counts<8>(a, s);
  else if (C >= 4) launch_counts<4>(a, s);
  else if (C >= 2) launch_counts<2>(a, s);
  else launch_counts<1>(a, s);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
