// Mel filter-bank inversion (librosa.feature.inverse.mel_to_stft with the reference's arguments).
//
// Replaces (reference call sites):
//   librosa.feature.inverse.mel_to_stft   src/data_preparation/audio/AudioProcessing.py:291-301
//                                         (mfbanks_to_amp_sp, called by decode_sp :321-322 and
//                                         Synthesiser.run_world_synth :58 for sp_type "mfbanks")
//
// Per frame b (n_mels mel bands) the kernel solves the non-negative least-squares problem
// min ||A x - b||^2, x >= 0, for the norm=None mel basis A [n_mels, K] with a fixed FISTA iteration
// (tests/mel_inverse_spec.py):
//   x = clip(pinv(A) b, 0), y = x;  per iteration  g = A^T (A y - b),  x' = max(y - g / L, 0),
//   y = x' + (t - 1) / t' (x' - x);  every `check` iterations it stops once
//   max_k |min(x_k, (A^T (A x - b))_k)| <= tol max_k |(A^T b)_k|,  at the latest after `cap` iterations,
// and writes K x.  One wave owns one frame; all state is fp64 whatever the input and output types.
//
// Layout.  Every FFT bin lies in at most two adjacent filters, m1 and m1 + 1 (the host checks it), so
//   A^T r  is a two-term gather per bin:  g_k = wa_k r[m1_k] + wb_k r[m1_k + 1],
//   A y    is a sum over each filter's bins: filter m takes wb y from the bins with m1 = m - 1 and wa y from
//          the bins with m1 = m; m1 is non-decreasing in k, so these are the contiguous ranges [sb, eb), [eb, ea).
// Lane l holds bins l + 64 q (q < C) of x and y and their (m1, wa, wb) in registers.  A y: every lane
// writes (wa y, wb y) of its bins into the wave's LDS row, then lane l sums filters l, l + 64, ... over
// their ranges in ascending bin order and writes r into a second row (shifted by one, zero at both ends,
// so m1 = -1 and m1 + 1 = n_mels read 0).  A^T r reads that row back.  No workgroup barriers, no atomics:
// a frame's result depends on nothing but its own bands and is the same from run to run.
// The start pinv(A) b reads pinv(A)^T [n_mels, 64 C] (zero-padded) from global memory, once per frame.
#include <cfloat>

#include "context.h"
#include "wave_fft.h"

namespace itts {
namespace {

constexpr int MI_WAVES = 4;        // waves (frames) per workgroup
constexpr int MI_MAX_MELS = 256;   // filter slots: 4 per lane
constexpr int MI_RS = MI_MAX_MELS + 8;

struct MiArgs {
  const void* mel;          // [F, ld_mel] float / double
  int64_t ld_mel;
  void* out;                // [F, ld_out] float / double
  int64_t ld_out;
  int64_t F;
  int K;
  int n_mels;
  int in_f64;
  int out_f64;
  const int* bin_j;         // [64 C]: m1 + 1 per bin (0 .. n_mels), 0 for padding bins
  const double* bin_w;      // [64 C][2]: (wa, wb), zero for padding bins
  const int* filt;          // [n_mels][3]: sb, eb, ea
  const double* pinv_t;     // [n_mels, 64 C]: pinv(A)^T, zero-padded
  double inv_l;             // 1 / lambda_max(A A^T)
  double tol;
  int cap;
  int check;
  int* iters;               // [F] iterations taken, or null
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

template <int C>
__global__ __launch_bounds__(64 * MI_WAVES) void mel_inverse_kernel(MiArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ROW_BYTES = C * 64 * 16 + MI_RS * 8;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = wf::lane_id();
  const int64_t f = (int64_t)blockIdx.x * MI_WAVES + wv;
  if (f >= a.F) return;                                   // wave-uniform; the kernel has no block barrier
  double2* P = reinterpret_cast<double2*>(smem + (size_t)wv * ROW_BYTES);
  double* rs = reinterpret_cast<double*>(smem + (size_t)wv * ROW_BYTES + C * 64 * 16);
  const int nm = a.n_mels, KP = 64 * C;

  int j[C];
  double wa[C], wb[C], x[C], y[C];
#pragma unroll
  for (int q = 0; q < C; ++q) {
    const int k = l + 64 * q;
    j[q] = a.bin_j[k];
    wa[q] = a.bin_w[2 * k];
    wb[q] = a.bin_w[2 * k + 1];
  }
  // this lane's filters m = l + 64 s: bands and bin ranges
  double bm[4];
  int sb[4], eb[4], ea[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int m = l + 64 * s;
    bm[s] = 0.0;
    sb[s] = eb[s] = ea[s] = 0;
    if (m < nm) {
      bm[s] = a.in_f64 ? reinterpret_cast<const double*>(a.mel)[f * a.ld_mel + m]
                       : (double)reinterpret_cast<const float*>(a.mel)[f * a.ld_mel + m];
      sb[s] = a.filt[3 * m];
      eb[s] = a.filt[3 * m + 1];
      ea[s] = a.filt[3 * m + 2];
      rs[m + 1] = bm[s];
    }
  }
  if (l == 0) {
    rs[0] = 0.0;
    rs[nm + 1] = 0.0;
  }
  wf::wave_sync();

  // librosa's start clip(pinv(A) b, 0) and the scale max |A^T b| of the stopping test
  double gmax = 0.0;
#pragma unroll
  for (int q = 0; q < C; ++q) {
    x[q] = 0.0;
    gmax = fmax(gmax, fabs(wa[q] * rs[j[q]] + wb[q] * rs[j[q] + 1]));
  }
  for (int m = 0; m < nm; ++m) {
    const double bv = rs[m + 1];
    const double* row = a.pinv_t + (size_t)m * KP + l;
#pragma unroll
    for (int q = 0; q < C; ++q) x[q] = fma(row[64 * q], bv, x[q]);
  }
#pragma unroll
  for (int q = 0; q < C; ++q) {
    x[q] = fmax(x[q], 0.0);
    y[q] = x[q];
  }
  const double g0 = wave_max(gmax);
  wf::wave_sync();

  // rs[1 + m] = (A v - b)_m
  auto residual = [&](const double* v) {
#pragma unroll
    for (int q = 0; q < C; ++q) P[l + 64 * q] = make_double2(wa[q] * v[q], wb[q] * v[q]);
    wf::wave_sync();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (64 * s >= nm) break;
      const int m = l + 64 * s;
      if (m < nm) {
        double acc = -bm[s];
        const double* pb = reinterpret_cast<const double*>(P) + 1;
        const double* pa = reinterpret_cast<const double*>(P);
        for (int k = sb[s]; k < eb[s]; ++k) acc += pb[2 * k];
        for (int k = eb[s]; k < ea[s]; ++k) acc += pa[2 * k];
        rs[m + 1] = acc;
      }
    }
    wf::wave_sync();
  };

  const double inv_l = a.inv_l, thr = a.tol * g0;
  double t = 1.0;
  int it = 0;
  while (it < a.cap) {
    residual(y);
    const double tn = (1.0 + sqrt(1.0 + 4.0 * t * t)) * 0.5;
    const double beta = (t - 1.0) / tn;
    t = tn;
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const double g = wa[q] * rs[j[q]] + wb[q] * rs[j[q] + 1];
      const double xn = fmax(y[q] - g * inv_l, 0.0);
      y[q] = xn + beta * (xn - x[q]);
      x[q] = xn;
    }
    wf::wave_sync();
    ++it;
    if (it % a.check == 0 && it < a.cap) {
      residual(x);
      double kkt = 0.0;
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const double g = wa[q] * rs[j[q]] + wb[q] * rs[j[q] + 1];
        kkt = fmax(kkt, fabs(fmin(x[q], g)));
      }
      wf::wave_sync();
      if (wave_max(kkt) <= thr) break;
    }
  }

  const double scale = (double)a.K;
#pragma unroll
  for (int q = 0; q < C; ++q) {
    const int k = l + 64 * q;
    if (k < a.K) {
      if (a.out_f64)
        reinterpret_cast<double*>(a.out)[f * a.ld_out + k] = x[q] * scale;
      else
        reinterpret_cast<float*>(a.out)[f * a.ld_out + k] = (float)(x[q] * scale);
    }
  }
  if (a.iters && l == 0) a.iters[f] = it;
}

template <int C>
int launch_mi(const MiArgs& a, hipStream_t s) {
  const size_t lds = (size_t)MI_WAVES * (C * 64 * 16 + MI_RS * 8);
  ITTS_HIP_CHECK(itts::allow_dynamic_lds((const void*)mel_inverse_kernel<C>, lds));
  const int64_t blocks = (a.F + MI_WAVES - 1) / MI_WAVES;
  hipLaunchKernelGGL(mel_inverse_kernel<C>, dim3((unsigned)blocks), dim3(64 * MI_WAVES), lds, s, a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int itts_mel_inverse(const void* d_mel, int64_t n_frames, int n_mels, int64_t ld_mel, int mel_f64,
                                int n_fft, const int* d_bin_j, const double* d_bin_w, const int* d_filt,
                                const double* d_pinv_t, double inv_lipschitz, double tol, int max_iter,
                                int check_every, void* d_out, int64_t ld_out, int out_f64, int* d_iters,
                                void* stream) {
  ITTS_REQUIRE(n_fft == 1024 || n_fft == 2048, "n_fft must be 1024 or 2048");
  ITTS_REQUIRE(n_mels >= 1 && n_mels <= MI_MAX_MELS, "n_mels must be in [1, 256]");
  const int K = n_fft / 2 + 1;
  ITTS_REQUIRE(n_frames >= 0 && n_frames / MI_WAVES < 0x7fffffff, "bad frame count");
  ITTS_REQUIRE(ld_mel >= n_mels, "ld_mel smaller than n_mels");
  ITTS_REQUIRE(ld_out >= K, "ld_out smaller than n_fft / 2 + 1");
  ITTS_REQUIRE(mel_f64 == 0 || mel_f64 == 1, "mel_f64 must be 0 or 1");
  ITTS_REQUIRE(out_f64 == 0 || out_f64 == 1, "out_f64 must be 0 or 1");
  ITTS_REQUIRE(inv_lipschitz > 0.0 && inv_lipschitz <= DBL_MAX, "inv_lipschitz must be positive and finite");
  ITTS_REQUIRE(tol >= 0.0 && tol <= DBL_MAX, "tol must be non-negative and finite");
  ITTS_REQUIRE(max_iter >= 0, "max_iter must not be negative");
  ITTS_REQUIRE(check_every >= 1, "check_every must be positive");
  if (n_frames == 0) return ITTS_OK;
  ITTS_REQUIRE(d_mel && d_bin_j && d_bin_w && d_filt && d_pinv_t && d_out, "null pointer");
  MiArgs a{d_mel, ld_mel, d_out, ld_out, n_frames, K, n_mels, mel_f64, out_f64, d_bin_j, d_bin_w, d_filt,
           d_pinv_t, inv_lipschitz, tol, max_iter, check_every, d_iters};
  hipStream_t s = as_stream(stream);
  return n_fft == 1024 ? launch_mi<9>(a, s) : launch_mi<17>(a, s);
}
