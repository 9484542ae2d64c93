// The WaveNet vocoder network (models/WaveNetWrapper.py:110-132 of the reference, which wraps the external
// wavenet_vocoder package): the gate of a residual layer as a kernel pair for the training stack, and sample-by-sample
// generation of whole batches in ONE launch.
//
// Gate.  x [N, G] holds the dilated convolution's output, halves a | b of H = G / 2 columns; c (optional, [N, G]) the
// projected conditioning, split the same way:  z = tanh(a + ca) * sigmoid(b + cb).  The backward recomputes both
// activations from the saved pre-activations and writes dx [N, G], which is also the gradient of c (c enters by
// addition).  Rows are read as float4 when H and every pitch are multiples of four floats and the bases are 16-byte
// aligned (then the b half is aligned too); otherwise every element goes through the scalar form.
//
// Generation.  One workgroup of 256 lanes owns a tile of up to 16 batch rows for every layer and every step; the
// only synchronisation is the workgroup barrier, nothing outside the workgroup is ever waited on.  Per step:
//   first conv   x0[row] = bf + Wf[:, previous class] (a column gather; scalar input: bf + wf * previous sample),
//                written to layer 0's ring buffer;
//   per layer    A [16 x (k R + cin')] is gathered into LDS: the k taps x[t - (k-1-j) d] from the layer's ring buffer
//                (depth (k-1) d + 1, zeros before the start) and c[b, t] (cin' = cin rounded up to 16, zero filled);
//                A x W1 [k R + cin', G] on v_mfma_f32_16x16x4_f32 with the bias as the initial accumulator; a wave
//                owns the column tiles p and p + H / 16 of the same 16 gate channels, so the gate is formed in
//                registers and z [16 x H] goes to LDS;  z x W2 [H, R + S]: the R "out" columns give
//                x' = (out + x) sqrt(1/2), written to the next layer's ring buffer, the S skip columns accumulate in
//                registers over the layers (a wave owns the same skip tiles in every layer);
//   head         relu(skip) x Wh1, relu, x Wh2 -> the logits / mixture parameters in LDS;
//   draw         mu-law: inverse CDF of the softmax at u[b, t]: the number of classes whose cumulative sum is <= u
//                times the total; mixture of logistics: the mixture by inverse CDF at u[b, t, 0], then
//                clamp(mean + exp(max(log_scale, log_scale_min)) (log u1 - log(1 - u1)), -1, 1), u1 = u[b, t, 1].
// Weight images are packed by the caller, one float4 per lane and MFMA group: image[kb][tile][lane][j] =
// W[16 kb + 4 (lane >> 4) + j][16 tile + (lane & 15)] for a [K, N] operand (K, N multiples of 16): a wave's load of
// one tile and 16 values of k is 1 KiB contiguous, and the A fragment of those 16 k is one float4 LDS read per lane.
// The k order inside a group of 16 is therefore 0, 4, 8, 12, 1, 5, ...; every row sees the same order, and a row of A
// only ever meets its own row of the accumulator: a row's bits do not depend on the batch size or its place in it.
// The kernel draws no random number: generation is a pure function of its inputs.
#include <algorithm>
#include <math.h>
#include <vector>

#include "common.h"
#include "context.h"

namespace itts {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GATE_THREADS = 256;
constexpr int64_t GATE_MAX_GRID = (1 << 24) - 1;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

struct GateArgs {
  const float* x;
  const float* c;       // or NULL
  const float* dz;      // backward only
  float* out;           // z [N, H] (forward) / dx [N, G] (backward)
  int64_t N, ldx, ldc, ldz, ldo;
  int H;
};

template <bool VEC, bool BWD>
__global__ __launch_bounds__(GATE_THREADS) void glu_gate_kernel(GateArgs g) {
  constexpr int W = VEC ? 4 : 1;
  const int per_row = g.H / W;
  const int64_t e = (int64_t)blockIdx.x * GATE_THREADS + threadIdx.x;
  if (e >= g.N * per_row) return;
  const int64_t n = e / per_row;
  const int col = (int)(e - n * per_row) * W;
  float a[W], b[W], d[W];
  const float* xa = g.x + n * g.ldx + col;
  const float* xb = xa + g.H;
  if (VEC) {
    *reinterpret_cast<float4*>(a) = *reinterpret_cast<const float4*>(xa);
    *reinterpret_cast<float4*>(b) = *reinterpret_cast<const float4*>(xb);
  } else {
    a[0] = xa[0];
    b[0] = xb[0];
  }
  if (g.c) {
    const float* ca = g.c + n * g.ldc + col;
    const float* cb = ca + g.H;
    float va[W], vb[W];
    if (VEC) {
      *reinterpret_cast<float4*>(va) = *reinterpret_cast<const float4*>(ca);
      *reinterpret_cast<float4*>(vb) = *reinterpret_cast<const float4*>(cb);
    } else {
      va[0] = ca[0];
      vb[0] = cb[0];
    }
#pragma unroll
    for (int i = 0; i < W; ++i) {
      a[i] += va[i];
      b[i] += vb[i];
    }
  }
  if (BWD) {
    const float* dp = g.dz + n * g.ldz + col;
    if (VEC) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(dp);
    else d[0] = dp[0];
    float da[W], db[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const float t = tanhf(a[i]), s = sigmoidf_(b[i]);
      da[i] = d[i] * (1.f - t * t) * s;
      db[i] = d[i] * t * (s * (1.f - s));
    }
    float* oa = g.out + n * g.ldo + col;
    float* ob = oa + g.H;
    if (VEC) {
      *reinterpret_cast<float4*>(oa) = *reinterpret_cast<const float4*>(da);
      *reinterpret_cast<float4*>(ob) = *reinterpret_cast<const float4*>(db);
    } else {
      oa[0] = da[0];
      ob[0] = db[0];
    }
  } else {
    float z[W];
#pragma unroll
    for (int i = 0; i < W; ++i) z[i] = tanhf(a[i]) * sigmoidf_(b[i]);
    float* oz = g.out + n * g.ldo + col;
    if (VEC) *reinterpret_cast<float4*>(oz) = *reinterpret_cast<const float4*>(z);
    else oz[0] = z[0];
  }
}

// ---- generation ------------------------------------------------------------------------------------------------
constexpr int WN_ROWS = 16;
constexpr int WN_THREADS = 256;
constexpr int WN_MAX_LAYERS = 64;
constexpr int WN_MAX_WIDTH = 512;
constexpr int WN_MAX_CIN = 128;
constexpr int WN_MAX_CLASSES = 256;
constexpr int WN_MAX_MIX = 64;
constexpr int WN_MAX_DILATION = 512;
constexpr size_t WN_MAX_LDS = 160 * 1024;

struct WnArgs {
  const float *wf, *bf;         // first conv: [Cin0, R] (column c of the weight as a row) / [R]
  const float *w1, *b1;         // per layer: image of [KA, G] / [G]
  const float *w2, *b2;         // per layer: image of [H, R + S] / [R + S]
  const float *wh1, *bh1;       // head: image of [S, S] / [S]
  const float *wh2, *bh2;       // image of [S, Cpad] / [Cpad]
  const float* c;               // [B, Tc, cin] or NULL
  const float* u;               // [B, Tout] / [B, Tout, 2]
  const int* len;               // [B] on the device
  float* state;                 // ring buffers, tile_state floats per tile
  void* out;                    // int32 classes / float samples, [B, Tout]
  float* logits;                // [B, Tout, C] or NULL
  int64_t Tc, Tout, tile_state;
  int B, L, k, R, G, H, S, cin, C, Cpad, KA;
  int pitchA, pitchZ, pitchS, pitchL, areaA;
  int scalar, initial_class;
  float lsm;
  int dil[WN_MAX_LAYERS];
  int roff[WN_MAX_LAYERS + 1];  // first slot of layer l's ring buffer; a slot is [16][R]
};

__device__ __forceinline__ f32x4 splat4(float v) { return f32x4{v, v, v, v}; }

// the float4 offset of tile `tile` inside a k-group, or of the wave's first tile `first` for a spare slot
__device__ __forceinline__ int tile_slot(bool valid, int tile, int first) { return (valid ? tile : first) * 64; }

// acc[i] += X [16 x 16 KB] x the column tile toff[i] / 64 of a weight image, for the 8 tile slots of a wave.  Every
// slot names a tile: a wave with fewer tiles repeats its first one in the spare slots (tile_slot) and nobody reads their
// accumulators -- no branch inside the pipeline; a wave without any tile does not call.  W points at the lane's float4
// of (kb 0, tile 0), a k-group further is kbstride float4s on; xs at the lane's float4 of the A tile's k-group 0 in
// LDS.  The weights are the whole traffic of a step and every float4 of them is read exactly once, by one wave, with
// one wave on each SIMD: nothing else hides their latency, so the fragments of D - 1 k-groups ahead are in flight in
// registers while a k-group is multiplied (8 (D - 1) loads; measured at the default widths: 5.8 ms a step without the
// prefetch, 2.7 ms with it).
template <int D>
__device__ __forceinline__ void stream_mfma(f32x4 (&acc)[8], const int (&toff)[8], const f32x4* __restrict__ W, int KB,
                                            int kbstride, const float* xs) {
  f32x4 buf[D][8];
#pragma unroll
  for (int s = 0; s < D - 1; ++s) {
    if (s < KB) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        buf[s][i] = W[(int64_t)s * kbstride + toff[i]];
    }
  }
  for (int kb0 = 0; kb0 < KB; kb0 += D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      const int kb = kb0 + s;
      if (kb < KB) {
        const int kn = kb + D - 1;
        if (kn < KB) {
#pragma unroll
          for (int i = 0; i < 8; ++i)
            buf[(s + D - 1) % D][i] = W[(int64_t)kn * kbstride + toff[i]];
        }
        const f32x4 x = *reinterpret_cast<const f32x4*>(xs + kb * 16);
        // j outside, the tiles inside: consecutive MFMAs go to different accumulators (an accumulator still sees its
        // k in ascending order)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int i = 0; i < 8; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], buf[s][i][j], acc[i], 0, 0, 0);
        }
      }
    }
  }
}

constexpr int WN_PREFETCH = 4;     // k-groups of weight fragments in flight, the one being multiplied included

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// inclusive sum over the lanes of a wave, lane 0 first
__device__ __forceinline__ float wave_scan(float v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(WN_THREADS) void wavenet_generate_kernel(WnArgs a) {
  extern __shared__ __align__(16) float lds[];
  float* At = lds;                      // [16][pitchA]; the head's three tiles afterwards
  float* Zt = lds + a.areaA;            // [16][pitchZ]
  __shared__ int s_len[WN_ROWS];
  __shared__ int s_cls[WN_ROWS];
  __shared__ float s_x[WN_ROWS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);       // the wave: scalar, so that what depends on it branches
  const int lr = lane & 15, kg = lane >> 4;
  const int b0 = blockIdx.x * WN_ROWS;
  const int R = a.R, H = a.H, S = a.S, k = a.k;
  if (tid < WN_ROWS) {
    s_len[tid] = b0 + tid < a.B ? a.len[b0 + tid] : 0;
    s_cls[tid] = a.initial_class;
    s_x[tid] = 0.f;
  }
  __syncthreads();
  int tmax = 0;
  for (int i = 0; i < WN_ROWS; ++i) tmax = max(tmax, s_len[i]);
  float* ring = a.state + (int64_t)blockIdx.x * a.tile_state;
  const int slot = WN_ROWS * R;
  const int NP = H / 16, NT1 = a.G / 16, KB1 = a.KA / 16;
  const int NO = R / 16, NS = S / 16, NT2 = NO + NS, KB2 = H / 16;
  const int NC = a.Cpad / 16;
  const int cpad = a.KA - k * R;
  const float rs = 0.70710678118654752440f;

  for (int t = 0; t < tmax; ++t) {
    {   // first conv into layer 0's ring buffer
      float* dst = ring + (int64_t)(a.roff[0] + t % (a.roff[1] - a.roff[0])) * slot;
      for (int e = tid; e < slot; e += WN_THREADS) {
        const int row = e / R, r = e - row * R;
        float v = a.bf[r];
        if (a.scalar) {
          v = fmaf(a.wf[r], s_x[row], v);
        } else {
          const int pc = s_cls[row];
          if (pc >= 0) v += a.wf[(int64_t)pc * R + r];
        }
        dst[e] = v;
      }
    }
    __syncthreads();
    f32x4 sk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sk[i] = splat4(0.f);

    for (int l = 0; l < a.L; ++l) {
      const int d = a.dil[l], depth = a.roff[l + 1] - a.roff[l];
      for (int j = 0; j < k; ++j) {
        const int tt = t - (k - 1 - j) * d;
        const float* src = ring + (int64_t)(a.roff[l] + (tt >= 0 ? tt % depth : 0)) * slot;
        for (int e = tid * 4; e < slot; e += WN_THREADS * 4) {
          const int row = e / R, r = e - row * R;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (tt >= 0) v = *reinterpret_cast<const float4*>(src + e);
          *reinterpret_cast<float4*>(At + row * a.pitchA + j * R + r) = v;
        }
      }
      for (int e = tid; e < WN_ROWS * cpad; e += WN_THREADS) {
        const int row = e / cpad, ci = e - row * cpad;
        float v = 0.f;
        if (ci < a.cin && t < s_len[row]) v = a.c[((int64_t)(b0 + row) * a.Tc + t) * a.cin + ci];
        At[row * a.pitchA + k * R + ci] = v;
      }
      __syncthreads();

      {   // A x W1, gate: acc[i] is tile p = w + 4 i of the a half, acc[4 + i] the same channels of the b half
        f32x4 acc[8];
        int toff[8];
        const float* bias = a.b1 + (int64_t)l * a.G;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = w + 4 * i;
          toff[i] = tile_slot(p < NP, p, w);
          toff[4 + i] = tile_slot(p < NP, p + NP, w);
          acc[i] = splat4(p < NP ? bias[p * 16 + lr] : 0.f);
          acc[4 + i] = splat4(p < NP ? bias[H + p * 16 + lr] : 0.f);
        }
        if (w < NP)
          stream_mfma<WN_PREFETCH>(acc, toff, reinterpret_cast<const f32x4*>(a.w1 + (int64_t)l * a.KA * a.G) + lane,
                                   KB1, NT1 * 64, At + lr * a.pitchA + 4 * kg);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = w + 4 * i;
          if (p < NP) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              Zt[(kg * 4 + j) * a.pitchZ + p * 16 + lr] = tanhf(acc[i][j]) * sigmoidf_(acc[4 + i][j]);
          }
        }
      }
      __syncthreads();

      {   // z x W2: out (residual update into the next ring buffer) and skip (kept in registers)
        const bool last = l + 1 == a.L;
        f32x4 ao[8];
        int toff_o[8], toff_s[8];
        const float* bias = a.b2 + (int64_t)l * (R + S);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int q = w + 4 * i;
          toff_o[i] = tile_slot(q < NO, q, w);
          toff_s[i] = tile_slot(q < NS, NO + q, NO + w);
          ao[i] = splat4(q < NO ? bias[q * 16 + lr] : 0.f);
          if (q < NS) sk[i] += splat4(bias[R + q * 16 + lr]);
        }
        const f32x4* W = reinterpret_cast<const f32x4*>(a.w2 + (int64_t)l * H * (R + S)) + lane;
        const float* xs = Zt + lr * a.pitchZ + 4 * kg;
        if (w < NO && !last) stream_mfma<WN_PREFETCH>(ao, toff_o, W, KB2, NT2 * 64, xs);
        if (w < NS) stream_mfma<WN_PREFETCH>(sk, toff_s, W, KB2, NT2 * 64, xs);
        if (!last) {
          const int depth1 = a.roff[l + 2] - a.roff[l + 1];
          float* dst = ring + (int64_t)(a.roff[l + 1] + t % depth1) * slot;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int q = w + 4 * i;
            if (q < NO) {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int row = kg * 4 + j, col = q * 16 + lr;
                dst[row * R + col] = (ao[i][j] + At[row * a.pitchA + (k - 1) * R + col]) * rs;
              }
            }
          }
        }
      }
      __syncthreads();
    }

    // head
    float* Hs = At;
    float* H2 = At + WN_ROWS * a.pitchS;
    float* Lg = At + 2 * WN_ROWS * a.pitchS;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = w + 4 * i;
      if (q < NS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Hs[(kg * 4 + j) * a.pitchS + q * 16 + lr] = fmaxf(sk[i][j], 0.f);
      }
    }
    __syncthreads();
    {
      f32x4 ah[8];
      int toff[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int q = w + 4 * i;
        toff[i] = tile_slot(q < NS, q, w);
        ah[i] = splat4(q < NS ? a.bh1[q * 16 + lr] : 0.f);
      }
      if (w < NS)
        stream_mfma<WN_PREFETCH>(ah, toff, reinterpret_cast<const f32x4*>(a.wh1) + lane, NS, NS * 64,
                               Hs + lr * a.pitchS + 4 * kg);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int q = w + 4 * i;
        if (q < NS) {
#pragma unroll
          for (int j = 0; j < 4; ++j) H2[(kg * 4 + j) * a.pitchS + q * 16 + lr] = fmaxf(ah[i][j], 0.f);
        }
      }
    }
    __syncthreads();
    {
      f32x4 al[8];
      int toff[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int q = w + 4 * i;
        toff[i] = tile_slot(i < 4 && q < NC, q, w);
        al[i] = splat4(i < 4 && q < NC ? a.bh2[q * 16 + lr] : 0.f);
      }
      if (w < NC)
        stream_mfma<WN_PREFETCH>(al, toff, reinterpret_cast<const f32x4*>(a.wh2) + lane, NS, NC * 64,
                               H2 + lr * a.pitchS + 4 * kg);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = w + 4 * i;
        if (q < NC) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Lg[(kg * 4 + j) * a.pitchL + q * 16 + lr] = al[i][j];
        }
      }
    }
    __syncthreads();

    // draw: wave w takes rows 4 w .. 4 w + 3
    for (int rr = 0; rr < 4; ++rr) {
      const int row = 4 * w + rr;
      const bool live = t < s_len[row];                 // (wave-uniform)
      const int64_t bt = (int64_t)(b0 + row) * a.Tout + t;
      const float* lg = Lg + row * a.pitchL;
      if (a.logits && live)
        for (int e = lane; e < a.C; e += 64) a.logits[bt * a.C + e] = lg[e];
      if (!a.scalar) {
        float v[4], e4[4];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int cl = 4 * lane + j;
          v[j] = cl < a.C ? lg[cl] : -INFINITY;
          m = fmaxf(m, v[j]);
        }
        m = wave_max(m);
        float run = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          run += 4 * lane + j < a.C ? expf(v[j] - m) : 0.f;
          e4[j] = run;
        }
        const float incl = wave_scan(run, lane);
        const float total = __shfl(incl, 63, 64), excl = incl - run;
        const float thr = (live ? a.u[bt] : 0.5f) * total;
        int n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) n += (4 * lane + j < a.C && excl + e4[j] <= thr) ? 1 : 0;
        n = min(wave_sum_int(n), a.C - 1);
        if (lane == 0) {
          s_cls[row] = n;
          if (live) reinterpret_cast<int*>(a.out)[bt] = n;
        }
      } else {
        const int K = a.C / 3;
        const float v = lane < K ? lg[lane] : -INFINITY;
        const float m = wave_max(v);
        const float e = lane < K ? expf(v - m) : 0.f;
        const float incl = wave_scan(e, lane);
        const float total = __shfl(incl, 63, 64);
        const float thr = (live ? a.u[2 * bt] : 0.5f) * total;
        const int n = min(wave_sum_int((lane < K && incl <= thr) ? 1 : 0), K - 1);
        if (lane == 0) {
          const float u1 = live ? a.u[2 * bt + 1] : 0.5f;
          const float mean = lg[K + n], ls = fmaxf(lg[2 * K + n], a.lsm);
          const float x = fminf(fmaxf(fmaf(expf(ls), logf(u1) - log1pf(-u1), mean), -1.f), 1.f);
          s_x[row] = x;
          if (live) reinterpret_cast<float*>(a.out)[bt] = x;
        }
      }
    }
    __syncthreads();
  }
}

int wn_geometry(const char* func, int layers, int kernel_size, int R, const int* h_dil, int64_t* slots) {
  if (layers < 1 || layers > WN_MAX_LAYERS) {
    set_error(std::string(func) + ": layers = " + std::to_string(layers) + " is outside 1 .. " +
              std::to_string(WN_MAX_LAYERS));
    return ITTS_E_INVALID;
  }
  if (kernel_size != 2 && kernel_size != 3) {
    set_error(std::string(func) + ": kernel_size = " + std::to_string(kernel_size) + " is neither 2 nor 3");
    return ITTS_E_INVALID;
  }
  if (R < 16 || R > WN_MAX_WIDTH || R % 16) {
    set_error(std::string(func) + ": residual_channels = " + std::to_string(R) +
              " is no multiple of 16 in 16 .. " + std::to_string(WN_MAX_WIDTH));
    return ITTS_E_INVALID;
  }
  if (!h_dil) {
    set_error(std::string(func) + ": null pointer (h_dilations)");
    return ITTS_E_INVALID;
  }
  *slots = 0;
  for (int l = 0; l < layers; ++l) {
    if (h_dil[l] < 1 || h_dil[l] > WN_MAX_DILATION) {
      set_error(std::string(func) + ": dilation = " + std::to_string(h_dil[l]) + " of layer " + std::to_string(l) +
                " is outside 1 .. " + std::to_string(WN_MAX_DILATION));
      return ITTS_E_INVALID;
    }
    *slots += (int64_t)(kernel_size - 1) * h_dil[l] + 1;
  }
  return ITTS_OK;
}

int launch_gate(bool bwd, const float* d_x, int64_t ldx, const float* d_c, int64_t ldc, const float* d_dz, int64_t ldz,
                float* d_out, int64_t ldo, int64_t N, int G, hipStream_t s) {
  const int H = G / 2;
  GateArgs g{};
  g.x = d_x; g.c = d_c; g.dz = d_dz; g.out = d_out;
  g.N = N; g.ldx = ldx; g.ldc = ldc; g.ldz = ldz; g.ldo = ldo; g.H = H;
  bool vec = H % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && aligned16(d_x) && aligned16(d_out);
  if (d_c) vec = vec && ldc % 4 == 0 && aligned16(d_c);
  if (bwd) vec = vec && ldz % 4 == 0 && aligned16(d_dz);
  const int64_t work = N * (vec ? H / 4 : H);
  const int64_t blocks = (work + GATE_THREADS - 1) / GATE_THREADS;
  if (blocks > GATE_MAX_GRID) {
    set_error("glu gate: " + std::to_string(blocks) + " workgroups: more than " + std::to_string(GATE_MAX_GRID));
    return ITTS_E_INVALID;
  }
  const dim3 grid((unsigned)blocks);
  if (bwd) {
    if (vec) glu_gate_kernel<true, true><<<grid, GATE_THREADS, 0, s>>>(g);
    else glu_gate_kernel<false, true><<<grid, GATE_THREADS, 0, s>>>(g);
  } else {
    if (vec) glu_gate_kernel<true, false><<<grid, GATE_THREADS, 0, s>>>(g);
    else glu_gate_kernel<false, false><<<grid, GATE_THREADS, 0, s>>>(g);
  }
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

#define GATE_REQUIRE_SHAPE()                                                                                     \
  ITTS_REQUIRE(G >= 2 && G % 2 == 0, "G = " + std::to_string(G) + " is not a positive even number");             \
  ITTS_REQUIRE(N >= 0, "N = " + std::to_string(N) + " is negative");                                            \
  ITTS_REQUIRE(ldx >= G, "ldx = " + std::to_string(ldx) + " is below G = " + std::to_string(G));                 \
  ITTS_REQUIRE(!d_c || ldc >= G, "ldc = " + std::to_string(ldc) + " is below G = " + std::to_string(G))

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int itts_glu_gate_fwd(const float* d_x, int64_t ldx, const float* d_c, int64_t ldc, float* d_z, int64_t ldz,
                                 int64_t N, int G, void* stream) {
  GATE_REQUIRE_SHAPE();
  ITTS_REQUIRE(ldz >= G / 2, "ldz = " + std::to_string(ldz) + " is below G / 2 = " + std::to_string(G / 2));
  if (N == 0) return ITTS_OK;
  ITTS_REQUIRE(d_x && d_z, "null pointer (d_x / d_z) with N = " + std::to_string(N));
  return launch_gate(false, d_x, ldx, d_c, ldc, nullptr, 0, d_z, ldz, N, G, as_stream(stream));
}

extern "C" int itts_glu_gate_bwd(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, const float* d_c,
                                 int64_t ldc, float* d_dx, int64_t lddx, int64_t N, int G, void* stream) {
  GATE_REQUIRE_SHAPE();
  ITTS_REQUIRE(lddz >= G / 2, "lddz = " + std::to_string(lddz) + " is below G / 2 = " + std::to_string(G / 2));
  ITTS_REQUIRE(lddx >= G, "lddx = " + std::to_string(lddx) + " is below G = " + std::to_string(G));
  if (N == 0) return ITTS_OK;
  ITTS_REQUIRE(d_dz && d_x && d_dx, "null pointer (d_dz / d_x / d_dx) with N = " + std::to_string(N));
  return launch_gate(true, d_x, ldx, d_c, ldc, d_dz, lddz, d_dx, lddx, N, G, as_stream(stream));
}

extern "C" int64_t itts_wavenet_state_floats(int B, int layers, int kernel_size, int residual_channels,
                                             const int* h_dilations) {
  int64_t slots = 0;
  if (B < 0 || wn_geometry(__func__, layers, kernel_size, residual_channels, h_dilations, &slots)) return -1;
  return (int64_t)((B + WN_ROWS - 1) / WN_ROWS) * slots * WN_ROWS * residual_channels;
}

extern "C" int itts_wavenet_generate(const float* d_wf, const float* d_bf, const float* d_w1, const float* d_b1,
                                     const float* d_w2, const float* d_b2, const float* d_wh1, const float* d_bh1,
                                     const float* d_wh2, const float* d_bh2, const int* h_dilations, int layers,
                                     int kernel_size, int residual_channels, int gate_channels, int skip_channels,
                                     int cin_channels, int out_channels, int scalar_input, double log_scale_min,
                                     const float* d_c, int64_t Tc, const float* d_u, const int* h_lengths, int B,
                                     int64_t T_out, int initial_class, float* d_state, int64_t state_floats,
                                     void* d_out, float* d_logits, void* stream) {
  const int R = residual_channels, G = gate_channels, S = skip_channels, cin = cin_channels, C = out_channels;
  int64_t slots = 0;
  if (int rc = wn_geometry(__func__, layers, kernel_size, R, h_dilations, &slots)) return rc;
  ITTS_REQUIRE(G >= 32 && G <= WN_MAX_WIDTH && G % 32 == 0,
               "gate_channels = " + std::to_string(G) + " is no multiple of 32 in 32 .. " +
                   std::to_string(WN_MAX_WIDTH));
  ITTS_REQUIRE(S >= 16 && S <= WN_MAX_WIDTH && S % 16 == 0,
               "skip_out_channels = " + std::to_string(S) + " is no multiple of 16 in 16 .. " +
                   std::to_string(WN_MAX_WIDTH));
  ITTS_REQUIRE(cin >= 0 && cin <= WN_MAX_CIN,
               "cin_channels = " + std::to_string(cin) + " is outside 0 .. " + std::to_string(WN_MAX_CIN));
  if (scalar_input)
    ITTS_REQUIRE(C >= 3 && C % 3 == 0 && C / 3 <= WN_MAX_MIX,
                 "out_channels = " + std::to_string(C) + " is not 3 K with K in 1 .. " + std::to_string(WN_MAX_MIX));
  else
    ITTS_REQUIRE(C >= 2 && C <= WN_MAX_CLASSES,
                 "out_channels = " + std::to_string(C) + " is outside 2 .. " + std::to_string(WN_MAX_CLASSES));
  ITTS_REQUIRE(scalar_input ? initial_class == -1 : (initial_class >= -1 && initial_class < C),
               "initial_class = " + std::to_string(initial_class) + " is outside -1 .. out_channels - 1 (-1 with "
               "scalar input)");
  ITTS_REQUIRE(log_scale_min == log_scale_min, "log_scale_min is not a number");
  ITTS_REQUIRE(B >= 0, "B = " + std::to_string(B) + " is negative");
  ITTS_REQUIRE(T_out >= 0, "T_out = " + std::to_string(T_out) + " is negative");
  if (B == 0 || T_out == 0) return ITTS_OK;
  ITTS_REQUIRE(h_lengths, "null pointer (h_lengths)");
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    ITTS_REQUIRE(h_lengths[b] >= 0 && h_lengths[b] <= T_out,
                 "length " + std::to_string(h_lengths[b]) + " of row " + std::to_string(b) +
                     " is outside 0 .. T_out = " + std::to_string(T_out));
    longest = std::max(longest, h_lengths[b]);
  }
  if (longest == 0) return ITTS_OK;
  ITTS_REQUIRE(cin == 0 || (d_c && Tc >= longest),
               "conditioning of " + std::to_string(Tc) + " steps for rows of up to " + std::to_string(longest));
  const int64_t tiles = (B + WN_ROWS - 1) / WN_ROWS;
  const int64_t tile_state = slots * WN_ROWS * R;
  ITTS_REQUIRE(state_floats >= tiles * tile_state, "state of " + std::to_string(state_floats) + " floats, " +
                                                       std::to_string(tiles * tile_state) + " needed");
  ITTS_REQUIRE(d_wf && d_bf && d_w1 && d_b1 && d_w2 && d_b2 && d_wh1 && d_bh1 && d_wh2 && d_bh2 && d_u && d_state &&
                   d_out, "null pointer (weights / d_u / d_state / d_out)");
  ITTS_REQUIRE(aligned16(d_w1) && aligned16(d_w2) && aligned16(d_wh1) && aligned16(d_wh2) && aligned16(d_state),
               "weight images and state must be 16-byte aligned");

  WnArgs a{};
  a.wf = d_wf; a.bf = d_bf; a.w1 = d_w1; a.b1 = d_b1; a.w2 = d_w2; a.b2 = d_b2;
  a.wh1 = d_wh1; a.bh1 = d_bh1; a.wh2 = d_wh2; a.bh2 = d_bh2;
  a.c = d_c; a.u = d_u; a.state = d_state; a.out = d_out; a.logits = d_logits;
  a.Tc = Tc; a.Tout = T_out; a.tile_state = tile_state;
  a.B = B; a.L = layers; a.k = kernel_size; a.R = R; a.G = G; a.H = G / 2; a.S = S; a.cin = cin; a.C = C;
  a.Cpad = (C + 15) / 16 * 16;
  a.KA = kernel_size * R + (cin + 15) / 16 * 16;
  a.pitchA = a.KA + 4; a.pitchZ = a.H + 4; a.pitchS = S + 4; a.pitchL = a.Cpad + 4;
  a.areaA = std::max(WN_ROWS * a.pitchA, 2 * WN_ROWS * a.pitchS + WN_ROWS * a.pitchL);
  a.scalar = scalar_input != 0; a.initial_class = initial_class; a.lsm = (float)log_scale_min;
  int off = 0;
  for (int l = 0; l < layers; ++l) {
    a.dil[l] = h_dilations[l];
    a.roff[l] = off;
    off += (kernel_size - 1) * h_dilations[l] + 1;
  }
  a.roff[layers] = off;
  const size_t lds = (size_t)(a.areaA + WN_ROWS * a.pitchZ) * sizeof(float);
  ITTS_REQUIRE(lds + 256 <= WN_MAX_LDS, "the tile needs " + std::to_string(lds) + " bytes of LDS");

  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  int* d_len = nullptr;
  ITTS_HIP_CHECK(scratch.take(&d_len, (size_t)B));
  if (int rc = staged_upload(d_len, h_lengths, (size_t)B * sizeof(int), s)) return rc;
  a.len = d_len;
  ITTS_HIP_CHECK(itts::allow_dynamic_lds(reinterpret_cast<const void*>(wavenet_generate_kernel), lds));
  wavenet_generate_kernel<<<dim3((unsigned)tiles), WN_THREADS, lds, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
