// Conv1d groups of RNNDyn (rnn_dyn/CNNWrapper.py -> torch.nn.Conv1d + act) on gfx950: a 1-D
// convolution over the time axis of a padded batch, computed as an implicit GEMM on the
// register-staged fp32-MFMA GEMM of the dense layers (gemm_staged.h).  The im2col matrix is never
// written: every K step reads one row shift of the activations straight from global memory (the
// operand loads of Im2colLoader; everything else is the shared body).
//
// Notation: activations are rows; row (b, t) of a tensor with T time steps sits at b * sb + t * st
// (batch_first: sb = T, st = 1; time-major: sb = 1, st = B).  Stride 1, T_out = T_in + 2 pad -
// dil (Kw - 1); a time index outside [0, T_in) reads as zero (the edge of the padded tensor, as
// the reference convolves the padded batch).
//
// The reduction is ordered tap-major with every tap padded to Cp = round_up(C, 4) channels:
// kk = k * Cp + c.  A float4 of the reduction then never straddles two taps, each 16-byte load is
// one row shift of x, and the padded channels are zeroed by a select (x's pad columns are read but
// never used).  The weights are re-laid out per call into [out][Kw * Cp] (a few KB to a few MB):
//   forward       w_t[n][k * Cinp + c]  = w[n][c][k]
//   input grad    w_f[c][k * Coutp + n] = w[n][c][Kw-1-k]   (taps flipped, weight transposed,
//                 pad' = dil (Kw-1) - pad, T_in and T_out swapped: the same correlation on dz)
//   weight grad   C[n][kk] = sum_m dz[m][n] * x_col[m][kk] over the B * T_out rows, split into
//                 chunks of whole K steps, one slab each; a fixed-order reduction sums the slabs and
//                 writes dw back in [Cout][Cin][Kw] (bit-identical run to run).
//
// Tile: 128 x (64 * TN) output per 256-thread workgroup, LDS double buffered (73.7 KB -> 2
// workgroups per CU); forward and input gradient take both operands in row form, the weight
// gradient both in col form.
#include <algorithm>

#include "common.h"
#include "gemm_staged.h"
#include "row4.h"

namespace itts {
namespace conv {

enum { MODE_FWD = 0, MODE_WGRAD = 1 };

// Unsigned division by a runtime constant for n < 2^31: q = (umulhi(n, mul) + n) >> shr.
struct FastDiv {
  uint32_t d, mul, shr;
};
static FastDiv make_fastdiv(uint32_t d) {
  FastDiv f{d, 0, 0};
  while ((1ull << f.shr) < d) ++f.shr;
  f.mul = (uint32_t)(((1ull << 32) * ((1ull << f.shr) - d)) / d + 1);
  return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  return (__umulhi(n, f.mul) + n) >> f.shr;
}

struct Geo {
  int B, T_in, T_out;
  int C, Cp;           // input channels of this product and their per-tap padded count
  int shift0, dil;     // input time = t + k * dil + shift0  (shift0 = -pad)
  int64_t in_sb, in_st, out_sb, out_st;   // row strides of the input and output tensors
  FastDiv div_T, div_Cp;                  // by T_out, by Cp
};

// FWD: A = x (implicit im2col rows), B = packed weights [N][K] (row form).
// WGRAD: A = dz (col form [k = m][out = n]), B = x (implicit im2col, col form [k = m][out = kk]).
struct ConvArgs : GemmArgs {
  Geo geo;
};

// 4 consecutive floats at p (valid address), lanes e with ok[e] false read as zero.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, bool ok, int n_ok) {
  // n_ok: how many of the 4 columns are inside the width (<= 0: none)
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    return make_float4(ok && n_ok > 0 ? v.x : 0.f, ok && n_ok > 1 ? v.y : 0.f, ok && n_ok > 2 ? v.z : 0.f,
                       ok && n_ok > 3 ? v.w : 0.f);
  } else {
    const bool k0 = ok && n_ok > 0, k1 = ok && n_ok > 1, k2 = ok && n_ok > 2, k3 = ok && n_ok > 3;
    const float a0 = k0 ? p[0] : 0.f, a1 = k1 ? p[1] : 0.f, a2 = k2 ? p[2] : 0.f, a3 = k3 ? p[3] : 0.f;
    return make_float4(a0, a1, a2, a3);
  }
}

// Physical row of logical output row m = b * T_out + t of a tensor with row strides (sb, st).
__device__ __forceinline__ int64_t phys_row(uint32_t m, const Geo& g, int64_t sb, int64_t st) {
  const uint32_t b = fdiv(m, g.div_T);
  const int t = (int)(m - b * (uint32_t)g.T_out);
  return (int64_t)b * sb + (int64_t)t * st;
}

// One row of the implicit im2col matrix: 4 reduction elements kk .. kk+3 (same tap) of logical row
// m; zero outside the input's time range, the padded channels and the matrix.
template <bool VEC>
__device__ __forceinline__ float4 im2col4(const float* __restrict__ x, int64_t ldx, const Geo& g, uint32_t m,
                                          bool m_ok, int tap, int c, bool kk_ok) {
  const uint32_t b = fdiv(m, g.div_T);
  const int t = (int)(m - b * (uint32_t)g.T_out);
  const int ti = t + tap * g.dil + g.shift0;
  const bool ok = m_ok && kk_ok && ti >= 0 && ti < g.T_in;
  const int64_t row = ok ? (int64_t)b * g.in_sb + (int64_t)ti * g.in_st : 0;
  return load4<VEC>(x + row * ldx + (ok ? c : 0), ok, g.C - c);
}

// The operand loads of the shared GEMM body (gemm_staged.h).
template <int MODE, bool VEC>
struct Im2colLoader {
  const ConvArgs& a;

  template <int NROWS>
  __device__ __forceinline__ void load_a(int64_t out0, int64_t k0, int64_t k_end, float4 (&r)[NROWS / 32]) const {
    const int tid = threadIdx.x;
    if (MODE == MODE_FWD) {   // row form: rows m (output rows), 4 reduction elements kk per thread
      const int64_t kk = k0 + ((tid & 7) << 2);
      const bool kk_ok = kk < k_end;
      const uint32_t kq = kk_ok ? (uint32_t)kk : 0u;
      const int tap = (int)fdiv(kq, a.geo.div_Cp);
      const int c = (int)(kq - (uint32_t)tap * (uint32_t)a.geo.Cp);
#pragma unroll
      for (int i = 0; i < NROWS / 32; ++i) {
        const int64_t m = out0 + ((tid + 256 * i) >> 3);
        const bool m_ok = m < a.M;
        r[i] = im2col4<VEC>(a.A, a.lda, a.geo, m_ok ? (uint32_t)m : 0u, m_ok, tap, c, kk_ok);
      }
    } else {                  // col form: dz rows m (reduction), 4 output channels n per thread
#pragma unroll
      for (int i = 0; i < NROWS / 32; ++i) {
        const int idx = tid + 256 * i;
        const int64_t m = k0 + idx / (NROWS / 4);
        const int64_t n = out0 + ((idx % (NROWS / 4)) << 2);
        const bool ok = m < k_end && n < a.M;
        const int64_t row = ok ? phys_row((uint32_t)m, a.geo, a.geo.out_sb, a.geo.out_st) : 0;
        r[i] = load4<VEC>(a.A + row * a.lda + (ok ? n : 0), ok, (int)(a.M - n));
      }
    }
  }

  template <int NROWS>
  __device__ __forceinline__ void load_b(int64_t out0, int64_t k0, int64_t k_end, float4 (&r)[NROWS / 32]) const {
    const int tid = threadIdx.x;
    if (MODE == MODE_FWD) {   // packed weights, row form [N][K], K % 4 == 0, 16-byte aligned
#pragma unroll
      for (int i = 0; i < NROWS / 32; ++i) {
        const int idx = tid + 256 * i;
        const int64_t o = out0 + (idx >> 3), k = k0 + ((idx & 7) << 2);
        const bool ok = o < a.N && k < k_end;
        r[i] = load4<true>(a.B + (ok ? o * a.ldb + k : 0), ok, 4);
      }
    } else {                  // implicit im2col, col form [k = m][out = kk]
#pragma unroll
      for (int i = 0; i < NROWS / 32; ++i) {
        const int idx = tid + 256 * i;
        const int64_t m = k0 + idx / (NROWS / 4);
        const int64_t kk = out0 + ((idx % (NROWS / 4)) << 2);
        const bool kk_ok = kk < a.N;
        const uint32_t kq = kk_ok ? (uint32_t)kk : 0u;
        const int tap = (int)fdiv(kq, a.geo.div_Cp);
        const int c = (int)(kq - (uint32_t)tap * (uint32_t)a.geo.Cp);
        const bool m_ok = m < k_end;
        r[i] = im2col4<VEC>(a.B, a.ldb, a.geo, m_ok ? (uint32_t)m : 0u, m_ok, tap, c, kk_ok);
      }
    }
  }
};

// The forward's output rows are those of the padded batch (geo.out_*); the weight gradient's are Cout.
template <int MODE, int EPI, bool VEC, int TN>
__global__ __launch_bounds__(256, 2) void conv1d_gemm_kernel(ConvArgs a) {
  constexpr bool ROW = MODE == MODE_FWD;   // both operands row form (FWD) or both col form (WGRAD)
  __shared__ __attribute__((aligned(16))) float lds[staged_lds_floats<ROW, TN, 2>()];
  f32x16 acc[2][TN];
  const StagedTile t = staged_gemm_tile<ROW, ROW, TN, 2>(a, Im2colLoader<MODE, VEC>{a}, lds, acc);
  // geo by value: captured by reference, hipcc no longer folds ldc into the row strides and spends a
  // 64-bit multiply per stored element (+0.5 % on the forward at the bench shapes)
  if (MODE == MODE_FWD)
    staged_epilogue<EPI, TN, AF_BASE>(a, t, acc, [geo = a.geo](int64_t m) {
      return phys_row((uint32_t)m, geo, geo.out_sb, geo.out_st);
    });
  else
    staged_epilogue<EPI, TN, AF_BASE>(a, t, acc, [](int64_t m) { return m; });
}

// Weights [Cout][Cin][Kw] -> packed [O][Kw * Ip]: forward (O = Cout, I = Cin) w_t[n][k Ip + c] =
// w[n][c][k]; flipped (O = Cin, I = Cout) w_f[c][k Ip + n] = w[n][c][Kw-1-k]; zero in the pad.
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                           int Cout, int Cin, int Kw, int flip) {
  const int O = flip ? Cin : Cout, I = flip ? Cout : Cin, Ip = (I + 3) & ~3;
  const int64_t n = (int64_t)O * Kw * Ip;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(e / ((int64_t)Kw * Ip));
    const int kk = (int)(e - (int64_t)o * Kw * Ip);
    const int k = kk / Ip, i = kk - k * Ip;
    float v = 0.f;
    if (i < I) v = flip ? w[((int64_t)i * Cin + o) * Kw + (Kw - 1 - k)] : w[((int64_t)o * Cin + i) * Kw + k];
    out[e] = v;
  }
}

// dw[n][c][k] (+)= sum over the S slabs, in slab order, of slab[n][k Cp + c]; db likewise from the
// column-sum slabs.  One thread per slab element (coalesced slab reads).
__global__ __launch_bounds__(256) void reduce_wgrad_kernel(const float* __restrict__ slabs, int S, int Cout, int Cin,
                                                           int Kw, int Cp, float* __restrict__ dw,
                                                           const float* __restrict__ bias_part, float* __restrict__ db,
                                                           int accumulate) {
  const int64_t KP = (int64_t)Kw * Cp, n_el = (int64_t)Cout * KP;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n_el + Cout;
       e += (int64_t)gridDim.x * blockDim.x) {
    if (e < n_el) {
      const int n = (int)(e / KP);
      const int kk = (int)(e - n * KP);
      const int k = kk / Cp, c = kk - k * Cp;
      if (c >= Cin) continue;
      float s = 0.f;
      for (int z = 0; z < S; ++z) s += slabs[(int64_t)z * n_el + e];
      float* o = dw + ((int64_t)n * Cin + c) * Kw + k;
      *o = accumulate ? *o + s : s;
    } else if (db) {
      const int n = (int)(e - n_el);
      float s = 0.f;
      for (int z = 0; z < S; ++z) s += bias_part[(int64_t)z * Cout + n];
      db[n] = accumulate ? db[n] + s : s;
    }
  }
}

template <int MODE, int EPI, int TN>
static int launch_tn(const ConvArgs& a, bool vec, int splitk, hipStream_t s) {
  const int64_t tiles = ((a.M + BM - 1) / BM) * ((a.N + 64 * TN - 1) / (64 * TN));
  dim3 grid((unsigned)tiles, 1, (unsigned)splitk);
  if (vec)
    hipLaunchKernelGGL((conv1d_gemm_kernel<MODE, EPI, true, TN>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((conv1d_gemm_kernel<MODE, EPI, false, TN>), grid, dim3(256), 0, s, a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// What a call runs: the tile width (64 * tn columns), the slabs of the reduction (grid z) and the
// reduction elements per slab.  make_plan below is the only place that decides it.
struct Plan {
  int tn, slabs;
  int64_t kchunk;
};

template <int MODE, int EPI>
static int launch(const ConvArgs& a, const Plan& p, bool vec, hipStream_t s) {
  if (p.tn == 1) return launch_tn<MODE, EPI, 1>(a, vec, p.slabs, s);
  return launch_tn<MODE, EPI, 2>(a, vec, p.slabs, s);
}

static int launch_pack(const float* w, float* out, int Cout, int Cin, int Kw, int flip, hipStream_t s) {
  const int O = flip ? Cin : Cout, I = flip ? Cout : Cin;
  const int64_t n = (int64_t)O * Kw * ((I + 3) & ~3);
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, s, w, out, Cout, Cin, Kw, flip);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

static Geo make_geo(int B, int T_in, int T_out, int C, int pad, int dil, int batch_first) {
  Geo g{};
  g.B = B; g.T_in = T_in; g.T_out = T_out; g.C = C; g.Cp = (C + 3) & ~3;
  g.shift0 = -pad; g.dil = dil;
  g.in_sb = batch_first ? T_in : 1; g.in_st = batch_first ? 1 : B;
  g.out_sb = batch_first ? T_out : 1; g.out_st = batch_first ? 1 : B;
  g.div_T = make_fastdiv((uint32_t)T_out);
  g.div_Cp = make_fastdiv((uint32_t)g.Cp);
  return g;
}

static int64_t out_len(int T_in, int Kw, int pad, int dil) {
  return (int64_t)T_in + 2 * (int64_t)pad - (int64_t)dil * (Kw - 1);
}

// Split of the weight gradient's B * T_out rows: enough slabs to give the 256 CUs two workgroups
// each, chunks of at least 8 K steps.
static int wgrad_splitk(int64_t M_rows, int Cout, int Kp) {
  const int64_t tiles = (int64_t)((Cout + BM - 1) / BM) * ((Kp + 127) / 128);
  int64_t s = std::max<int64_t>(1, 512 / std::max<int64_t>(tiles, 1));
  s = std::min<int64_t>(s, std::max<int64_t>(1, (M_rows + 8 * BK - 1) / (8 * BK)));
  return (int)std::min<int64_t>(s, 128);
}

static bool sizes_positive(int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil) {
  return B > 0 && T_in > 0 && Cin > 0 && Cout > 0 && Kw > 0 && dil > 0 && pad >= 0;
}
static bool within_2_31(int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil) {
  return (int64_t)B * T_in < ((int64_t)1 << 31) && (int64_t)B * out_len(T_in, Kw, pad, dil) < ((int64_t)1 << 31) &&
         (int64_t)Kw * (std::max(Cin, Cout) + 3) < ((int64_t)1 << 31);
}
// What CONV_CHECK_GEOMETRY asks of the entry points, for the plan query.
static bool geometry_ok(int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil) {
  return sizes_positive(B, T_in, Cin, Cout, Kw, pad, dil) && out_len(T_in, Kw, pad, dil) > 0 &&
         within_2_31(B, T_in, Cin, Cout, Kw, pad, dil);
}

// The plan of product 0 (forward), 1 (input gradient) or 2 (weight gradient) for a valid geometry.
// The GEMM is M x N over K: forward B*T_out x Cout over Kw * Cinp, input gradient B*T_in x Cin over
// Kw * Coutp, weight gradient Cout x Kw * Cinp over the B*T_out rows in slabs of whole K steps (the
// last slab may be shorter; rounding kchunk up to a K step can leave fewer slabs than wgrad_splitk
// sized the workspace for).  The 64-wide tile where the output is narrow (N <= 64) or where 128-wide
// tiles would leave most of the 256 CUs idle.  (vec, the 16-byte operand loads, selects the kernel
// instantiation but no tile or split today.)
static Plan make_plan(int product, int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil, int vec) {
  (void)vec;
  const int64_t T_out = out_len(T_in, Kw, pad, dil);
  int64_t M, N;
  Plan p{1, 1, 0};
  if (product == 2) {
    const int Kp = Kw * ((Cin + 3) & ~3);
    const int64_t rows = (int64_t)B * T_out;
    const int S = wgrad_splitk(rows, Cout, Kp);
    p.kchunk = (((rows + S - 1) / S + BK - 1) / BK) * BK;
    p.slabs = (int)((rows + p.kchunk - 1) / p.kchunk);
    M = Cout; N = Kp;
  } else {
    const int64_t Kp = (int64_t)Kw * (((product == 0 ? Cin : Cout) + 3) & ~3);
    p.kchunk = ((Kp + BK - 1) / BK) * BK;
    M = (int64_t)B * (product == 0 ? T_out : T_in);
    N = product == 0 ? Cout : Cin;
  }
  const int64_t tiles128 = ((M + BM - 1) / BM) * ((N + 127) / 128) * p.slabs;
  p.tn = (N <= 64 || tiles128 < 256) ? 1 : 2;
  return p;
}

}  // namespace conv
}  // namespace itts

using namespace itts;
using namespace itts::conv;

#define CONV_CHECK_GEOMETRY()                                                                              \
  ITTS_REQUIRE(sizes_positive(B, T_in, Cin, Cout, Kw, pad, dil), "bad sizes");                             \
  ITTS_REQUIRE(out_len(T_in, Kw, pad, dil) > 0, "T_out = T_in + 2 pad - dil (Kw - 1) must be positive");   \
  ITTS_REQUIRE(within_2_31(B, T_in, Cin, Cout, Kw, pad, dil), "sizes beyond 2^31 rows / reduction elements")

extern "C" int itts_conv1d_plan(int product, int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil, int vec,
                                int* tile_cols, int* slabs, int64_t* kchunk) {
  if (product < 0 || product > 2 || !geometry_ok(B, T_in, Cin, Cout, Kw, pad, dil)) return -1;
  const Plan p = make_plan(product, B, T_in, Cin, Cout, Kw, pad, dil, vec);
  if (tile_cols) *tile_cols = 64 * p.tn;
  if (slabs) *slabs = p.slabs;
  if (kchunk) *kchunk = p.kchunk;
  return 0;
}

extern "C" int itts_conv1d_fwd(const float* d_x, int64_t ldx, const float* d_w, const float* d_b, float* d_y,
                               int64_t ldy, int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil,
                               int batch_first, int act, void* stream) {
  ITTS_REQUIRE(d_x && d_w && d_y, "null pointer");
  CONV_CHECK_GEOMETRY();
  ITTS_REQUIRE(ldx >= Cin && ldy >= Cout, "bad row pitch");
  ITTS_REQUIRE(act >= 0 && act <= 2, "unknown activation");
  hipStream_t s = as_stream(stream);
  const int T_out = (int)out_len(T_in, Kw, pad, dil);
  const int Cp = (Cin + 3) & ~3, Kp = Kw * Cp;
  ScratchScope scratch(s);
  float* wt = nullptr;
  ITTS_HIP_CHECK(scratch.take(&wt, (size_t)Cout * Kp));
  int rc = launch_pack(d_w, wt, Cout, Cin, Kw, 0, s);
  if (rc) return rc;
  ConvArgs a{};
  a.A = d_x; a.lda = ldx; a.B = wt; a.ldb = Kp; a.C = d_y; a.ldc = ldy;
  a.M = (int64_t)B * T_out; a.N = Cout; a.K = Kp; a.bias = d_b; a.act = act;
  a.geo = make_geo(B, T_in, T_out, Cin, pad, dil, batch_first);
  const bool vec = rows16(d_x, ldx);
  const Plan p = make_plan(0, B, T_in, Cin, Cout, Kw, pad, dil, vec);
  a.kchunk = p.kchunk;
  rc = launch<MODE_FWD, EPI_BIAS_ACT>(a, p, vec, s);
  if (rc) return rc;
  return ITTS_OK;
}

extern "C" int itts_conv1d_bwd_input(const float* d_dz, int64_t lddz, const float* d_w, float* d_dx, int64_t lddx,
                                     const float* d_yprev, int64_t ldyp, int act_prev, int B, int T_in, int Cin,
                                     int Cout, int Kw, int pad, int dil, int batch_first, void* stream) {
  ITTS_REQUIRE(d_dz && d_w && d_dx, "null pointer");
  CONV_CHECK_GEOMETRY();
  ITTS_REQUIRE(lddz >= Cout && lddx >= Cin && (!d_yprev || ldyp >= Cin), "bad row pitch");
  ITTS_REQUIRE(act_prev >= 0 && act_prev <= 2, "unknown activation");
  hipStream_t s = as_stream(stream);
  const int T_out = (int)out_len(T_in, Kw, pad, dil);
  // dx = the forward correlation on dz: Cout -> Cin channels, T_out -> T_in steps, flipped taps,
  // pad' = dil (Kw - 1) - pad (negative when pad exceeds the kernel span: the range check covers it)
  const int Cp = (Cout + 3) & ~3, Kp = Kw * Cp;
  ScratchScope scratch(s);
  float* wf = nullptr;
  ITTS_HIP_CHECK(scratch.take(&wf, (size_t)Cin * Kp));
  int rc = launch_pack(d_w, wf, Cout, Cin, Kw, 1, s);
  if (rc) return rc;
  ConvArgs a{};
  a.A = d_dz; a.lda = lddz; a.B = wf; a.ldb = Kp; a.C = d_dx; a.ldc = lddx;
  a.M = (int64_t)B * T_in; a.N = Cin; a.K = Kp; a.aux = d_yprev; a.ldaux = ldyp; a.act = act_prev;
  a.geo = make_geo(B, T_out, T_in, Cout, dil * (Kw - 1) - pad, dil, batch_first);
  const bool vec = rows16(d_dz, lddz);
  const Plan p = make_plan(1, B, T_in, Cin, Cout, Kw, pad, dil, vec);
  a.kchunk = p.kchunk;
  rc = d_yprev ? launch<MODE_FWD, EPI_DACT>(a, p, vec, s) : launch<MODE_FWD, EPI_STORE>(a, p, vec, s);
  if (rc) return rc;
  return ITTS_OK;
}

extern "C" int64_t itts_conv1d_bwd_weight_workspace_bytes(int B, int T_in, int Cin, int Cout, int Kw, int pad,
                                                          int dil) {
  if (B <= 0 || T_in <= 0 || Cin <= 0 || Cout <= 0 || Kw <= 0 || dil <= 0 || pad < 0) return 0;
  const int64_t T_out = out_len(T_in, Kw, pad, dil);
  if (T_out <= 0) return 0;
  const int64_t Kp = (int64_t)Kw * ((Cin + 3) & ~3);
  const int S = wgrad_splitk((int64_t)B * T_out, Cout, (int)Kp);
  return (int64_t)S * ((int64_t)Cout * Kp + Cout) * 4 + 256;
}

extern "C" int itts_conv1d_bwd_weight(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, float* d_dw,
                                      float* d_db, int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil,
                                      int batch_first, void* d_workspace, int accumulate, void* stream) {
  ITTS_REQUIRE(d_dz && d_x && d_dw && d_workspace, "null pointer");
  CONV_CHECK_GEOMETRY();
  ITTS_REQUIRE(lddz >= Cout && ldx >= Cin, "bad row pitch");
  hipStream_t s = as_stream(stream);
  const int T_out = (int)out_len(T_in, Kw, pad, dil);
  const int Cp = (Cin + 3) & ~3, Kp = Kw * Cp;
  const int64_t rows = (int64_t)B * T_out;
  const bool vec = rows16(d_dz, lddz) && rows16(d_x, ldx);
  const Plan p = make_plan(2, B, T_in, Cin, Cout, Kw, pad, dil, vec);
  const int S_eff = p.slabs;
  float* slabs = reinterpret_cast<float*>(d_workspace);
  // C[Cout][Kp] = dz^T x_col: A = dz as col form [k = m][out = n]; B = the implicit im2col as col
  // form [k = m][out = kk]
  ConvArgs a{};
  a.A = d_dz; a.lda = lddz; a.B = d_x; a.ldb = ldx; a.C = slabs; a.ldc = Kp;
  a.M = Cout; a.N = Kp; a.K = rows; a.kchunk = p.kchunk; a.slab_stride = (int64_t)Cout * Kp;
  a.bias_part = d_db ? slabs + (int64_t)S_eff * Cout * Kp : nullptr;
  a.bias_part_stride = Cout;
  a.geo = make_geo(B, T_in, T_out, Cin, pad, dil, batch_first);
  int rc = launch<MODE_WGRAD, EPI_STORE>(a, p, vec, s);
  if (rc) return rc;
  const int64_t n = (int64_t)Cout * Kp + Cout;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(reduce_wgrad_kernel, dim3(blocks), dim3(256), 0, s, slabs, S_eff, Cout, Cin, Kw, Cp, d_dw,
                     a.bias_part, d_db, accumulate);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
