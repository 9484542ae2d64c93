// Corpus audio preparation (the four steps of the reference's scripts/bash_utils.sh that run before gen_data:
// down_sampling, silence_remove, normalize_loudness, high_pass_filter), float64 throughout.  The signals of a batch
// lie back to back in one array behind int64 offsets [n + 1], as everywhere in world.py.
//
// Batched polyphase FIR:  y[m] = sum_k h[k] * xu[m * down + c - k],  xu = the input with up - 1 zeros between its
// samples (never stored), k ascending, every output accumulated by ONE lane in that order, no atomics: an output is
// a fixed sequence of multiply-adds over values that depend on the signal alone, so a signal has the same bits alone
// and at any place of any batch.  Two members:
//   fir_unit_kernel  up = down = 1 (the zero-phase filter: 2 * numtaps multiply-adds per sample, 99 % of the
//                    arithmetic of the whole preparation).  A workgroup of 256 lanes takes 2048 consecutive outputs,
//                    8 per lane in registers.  The tile and its halo of numtaps - 1 values are staged in LDS through
//                    the index map of the pass (below), the taps beside them.  Lane l owns the outputs 8 l .. 8 l + 7
//                    and keeps a window of 15 signal values in registers: eight taps need eight new values, so 16
//                    LDS reads (8 of them broadcasts of a tap) feed 64 multiply-adds.  The tile is stored
//                    transposed, value i at [i % 8][i / 8], so that the 64 lanes of a read touch consecutive doubles
//                    (consecutive outputs per lane would otherwise read with a stride of 8 doubles: 8-way conflicts).
//   resample_kernel  any up / down <= 1024 (scipy.signal.resample_poly): one output per lane, the taps of its phase
//                    h[p + j * up], j ascending, against the signal tile in LDS, 64 values of j per staging round so
//                    that the tile is bounded for every ratio.  Consecutive outputs have different phases, so a tap
//                    is used once per tile and staging taps would buy nothing: they are read in place (the whole
//                    table is at most 164 KB and stays in L2).  61 taps per output at a third of the rate: 1 % of
//                    the filter's work.
//
// Zero-phase filtering = scipy.signal.filtfilt(b, [1], x) with padtype "odd", padlen L = 3 * numtaps, on
// fir_unit_kernel:  ext = [2 x[0] - x[L:0:-1], x, 2 x[-1] - x[-2:-L-2:-1]]  (N = n + 2 L values, read through an
// index map, never stored);  pass 1: y1[e] = sum_k h[k] ext[max(0, e - k)]  (what lies before the first value equals
// it: for an FIR filter that is lfilter_zi's start);  pass 2: the same over y1 reversed;  the result reversed again,
// without L values on each side.  Pass 2 only reads y1[L ..], so pass 1 computes e = L .. N - 1 (n + L values per
// signal, the workspace), and both passes are  out'[o] = sum_k h[k] V(max(0, o + L - k))  with
//   pass 1:  V(t) = ext[t],            out'[o] -> y1[L + o],   o < n + L
//   pass 2:  V(t) = y1[N - 1 - t],     out'[o] -> y[n - 1 - o], o < n
// Both matrix and vector fp64 peak at the same rate on this chip, so a Toeplitz formulation on
// v_mfma_f64_16x16x4_f64 could only save LDS reads, which the register window already brings to one per four
// multiply-adds (the LDS delivers one 64-lane 8-byte read per four cycles per CU, the four SIMDs issue four fp64
// multiply-adds in that time): not built.
//
// Loudness: mean, then the sum of squares of the centred values in a pass of its own (E[x^2] - mean^2 loses every
// digit at an offset, as layernorm.hip argues), then y = (x - mean) * sqrt(n * ref_rms^2 / sumsq).  As there, the
// centred values are centred once more on their own mean c, which takes out the rounding of the first sum and of the
// mean itself (at an offset of 1e4 standard deviations 1e4 times the spacing of the centred values): mean = m0 + c is
// never formed, y = ((x - m0) - c) * scale.  Sums in two fixed-order stages: one partial per 8192 samples counted
// from the signal's start (lane-strided, xor butterfly, waves in order), then the partials in ascending order.
//
// Frame RMS = librosa.feature.rms(y, frame_length, hop_length, center=True): the signal padded by frame_length / 2 on
// both sides with zeros ("constant") or mirrored ("reflect"), one workgroup per frame, sqrt(mean of squares).
#include <algorithm>
#include <vector>

#include "common.h"
#include "context.h"

namespace itts {
namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_MAX_GRID_Y = 65535;
constexpr int64_t AP_MAX_GRID_X = (1 << 24) - 1;   // workgroups of 256 lanes: gridDim.x * blockDim.x stays below 2^32

// ------------------------------------------------------------------------------------------ unit-rate FIR
constexpr int FIR_R = 8;
constexpr int FIR_TILE = FIR_R * AP_THREADS;
constexpr int FIR_MAX_TAPS = 2047;

struct FirArgs {
  const double* x;       // the signals (pass 1)
  double* ws;            // y1: signal s at off[s] + s * L, n + L values
  double* y;             // the result (pass 2)
  const int64_t* off;
  const double* taps;
  int numtaps, nk;       // nk = ceil(numtaps / FIR_R)
  int L;                 // padlen
  int W;                 // columns of the LDS tile
  int sig0;
};

// columns of the transposed tile: 256 lanes + nk tap groups, rounded up to 4 mod 32 (the 8 rows of 32 consecutive
// staging stores then fall on distinct banks)
int fir_columns(int nk) {
  int W = AP_THREADS + nk;
  while (W % 32 != 4) ++W;
  return W;
}

template <int PASS>
__global__ __launch_bounds__(AP_THREADS) void fir_unit_kernel(FirArgs a) {
  extern __shared__ double fir_smem[];
  constexpr int R = FIR_R;
  const int tid = threadIdx.x, W = a.W, nk = a.nk, Kpad = R * nk;
  double* xs = fir_smem;            // [R][W]
  double* hs = fir_smem + R * W;    // [Kpad]
  const int sig = a.sig0 + blockIdx.y;
  const int64_t begin = a.off[sig], n = a.off[sig + 1] - begin, L = a.L;
  const int64_t n_out = PASS == 1 ? n + L : n;
  const int64_t o0 = (int64_t)blockIdx.x * FIR_TILE;
  if (o0 >= n_out) return;
  for (int k = tid; k < Kpad; k += AP_THREADS) hs[k] = k < a.numtaps ? a.taps[k] : 0.0;
  const double* x = a.x + begin;
  double* y1 = a.ws + begin + (int64_t)sig * L;
  const int64_t dom = PASS == 1 ? n + 2 * L : n + L;     // V is defined on [0, dom)
  const int64_t B = o0 + L - (Kpad - 1);                 // V index of tile value 0
  for (int i = tid; i < FIR_TILE + Kpad - 1; i += AP_THREADS) {
    const int64_t t = max(B + i, (int64_t)0);
    double v = 0.0;                                      // (beyond dom: only outputs past the end read it)
    if (t < dom) {
      if (PASS == 1) {
        if (t < L) v = 2.0 * x[0] - x[L - t];
        else if (t < L + n) v = x[t - L];
        else v = 2.0 * x[n - 1] - x[2 * n + L - 2 - t];
      } else {
        v = y1[n + L - 1 - t];
      }
    }
    xs[(i % R) * W + i / R] = v;
  }
  __syncthreads();
  // output o0 + R l + r, tap k = R kk + u: tile value R (l + nk - kk) + (r - u - 1), window slot r - u - 1 + R
  double acc[R], w[2 * R - 1];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
#pragma unroll
  for (int e = R; e < 2 * R - 1; ++e) w[e] = xs[(e - R) * W + tid + nk];
  for (int kk = 0; kk < nk; ++kk) {
    const int col = tid + nk - kk - 1;
    double h[R];
#pragma unroll
    for (int e = 0; e < R; ++e) {
      w[e] = xs[e * W + col];
      h[e] = hs[R * kk + e];
    }
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] += h[u] * w[r - u - 1 + R];
#pragma unroll
    for (int e = R - 2; e >= 0; --e) w[e + R] = w[e];
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t o = o0 + (int64_t)R * tid + r;
    if (o < n_out) {
      if (PASS == 1) y1[o] = acc[r];
      else a.y[begin + n - 1 - o] = acc[r];
    }
  }
}

// ------------------------------------------------------------------------------------------ polyphase resampling
constexpr int RS_JC = 64;        // taps of a phase per staging round
constexpr int RS_SPAN = 4096;    // doubles of signal in LDS
constexpr int RS_MAX_RATE = 1024;

struct ResampleArgs {
  const double* x;
  const int64_t* off;
  const int64_t* out_off;
  const double* taps;
  double* y;
  int numtaps, up, down;
  int T;                 // outputs per workgroup
  int sig0;
};

// outputs per workgroup such that the signal span of a staging round, ((T - 1) * down) / up + 1 + RS_JC, fits
int resample_tile(int up, int down) {
  return (int)std::min<int64_t>(AP_THREADS, 1 + (int64_t)(RS_SPAN - RS_JC - 1) * up / down);
}

__global__ __launch_bounds__(AP_THREADS) void resample_kernel(ResampleArgs a) {
  __shared__ double xs[RS_SPAN];
  const int tid = threadIdx.x;
  const int sig = a.sig0 + blockIdx.y;
  const int64_t begin = a.off[sig], n = a.off[sig + 1] - begin;
  const int64_t obegin = a.out_off[sig], n_out = a.out_off[sig + 1] - obegin;
  const int64_t m0 = (int64_t)blockIdx.x * a.T;
  if (m0 >= n_out) return;
  const int64_t c = (a.numtaps - 1) / 2, up = a.up, down = a.down;
  const int64_t m_last = min(m0 + a.T, n_out) - 1;
  const int64_t i_first = (m0 * down + c) / up, i_last = (m_last * down + c) / up;
  const int64_t m = m0 + tid;
  const bool active = tid < a.T && m < n_out;
  const int64_t am = m * down + c, p = am % up, i0 = am / up;
  const int taps_m = active && p < a.numtaps ? (int)((a.numtaps - 1 - p) / up + 1) : 0;   // j with p + j up < numtaps
  const int taps_max = (int)((a.numtaps - 1) / up + 1);
  const double* x = a.x + begin;
  const int span = (int)(i_last - i_first) + RS_JC;
  double acc = 0.0;
  for (int jc = 0; jc < taps_max; jc += RS_JC) {
    const int64_t base = i_first - jc - (RS_JC - 1);
    __syncthreads();
    for (int i = tid; i < span; i += AP_THREADS) {
      const int64_t g = base + i;
      xs[i] = (g >= 0 && g < n) ? x[g] : 0.0;            // zeros lie outside the signal
    }
    __syncthreads();
    const int j_end = min(jc + RS_JC, taps_m);
    for (int j = jc; j < j_end; ++j) acc += a.taps[p + j * up] * xs[i0 - j - base];
  }
  if (active) a.y[obegin + m] = acc;
}

// ------------------------------------------------------------------------------------------ loudness
constexpr int LD_CHUNK = 8192;

struct LoudArgs {
  const double* x;
  double* y;
  const int64_t* off;
  double* partial;       // [n_signals][pitch]
  double* stat;          // [3][n_signals]: m0, c (mean = m0 + c), scale
  int64_t pitch;
  int n_signals, sig0;
  double ref_rms;
};

// PASS 0: sum x;  1: sum (x - m0);  2: sum ((x - m0) - c)^2
template <int PASS>
__global__ __launch_bounds__(AP_THREADS) void loud_partial_kernel(LoudArgs a) {
  __shared__ double red[16];
  const int sig = a.sig0 + blockIdx.y;
  const int64_t begin = a.off[sig], n = a.off[sig + 1] - begin;
  const int64_t start = (int64_t)blockIdx.x * LD_CHUNK;
  if (start >= n) return;
  const int64_t end = min(n, start + LD_CHUNK);
  const double m0 = PASS >= 1 ? a.stat[sig] : 0.0, c = PASS == 2 ? a.stat[a.n_signals + sig] : 0.0;
  double s = 0.0;
  for (int64_t i = start + threadIdx.x; i < end; i += AP_THREADS) {
    double v = a.x[begin + i];
    if (PASS >= 1) v -= m0;
    if (PASS == 2) {
      v -= c;
      v *= v;
    }
    s += v;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) a.partial[sig * a.pitch + blockIdx.x] = s;
}

// one wave per signal: the partials lane-strided in ascending order, then the butterfly
template <int PASS>
__global__ __launch_bounds__(kWave) void loud_final_kernel(LoudArgs a) {
  const int sig = blockIdx.x;
  const int64_t n = a.off[sig + 1] - a.off[sig];
  if (n == 0) return;
  const int64_t nb = (n + LD_CHUNK - 1) / LD_CHUNK;
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kWave) s += a.partial[sig * a.pitch + b];
  s = wave_sum(s);
  if (threadIdx.x == 0)
    a.stat[PASS * a.n_signals + sig] = PASS == 2 ? sqrt((double)n * a.ref_rms * a.ref_rms / s) : s / (double)n;
}

__global__ __launch_bounds__(AP_THREADS) void loud_apply_kernel(LoudArgs a) {
  const int sig = a.sig0 + blockIdx.y;
  const int64_t begin = a.off[sig], n = a.off[sig + 1] - begin;
  const int64_t start = (int64_t)blockIdx.x * LD_CHUNK;
  if (start >= n) return;
  const int64_t end = min(n, start + LD_CHUNK);
  const double m0 = a.stat[sig], c = a.stat[a.n_signals + sig], scale = a.stat[2 * a.n_signals + sig];
  for (int64_t i = start + threadIdx.x; i < end; i += AP_THREADS)
    a.y[begin + i] = ((a.x[begin + i] - m0) - c) * scale;
}

// ------------------------------------------------------------------------------------------ frame RMS
constexpr int RMS_MAX_FRAME = 1 << 20;

struct RmsArgs {
  const double* x;
  const int64_t* off;
  const int64_t* f_off;
  double* out;
  int frame_length, hop, pad_mode;
  int sig0;
};

__global__ __launch_bounds__(AP_THREADS) void frame_rms_kernel(RmsArgs a) {
  __shared__ double red[16];
  const int sig = a.sig0 + blockIdx.y;
  const int64_t begin = a.off[sig], n = a.off[sig + 1] - begin;
  const int64_t fbegin = a.f_off[sig], nf = a.f_off[sig + 1] - fbegin;
  const int64_t f = blockIdx.x;
  if (f >= nf) return;
  const int64_t start = f * a.hop - a.frame_length / 2;
  const int64_t period = 2 * (n - 1);
  double s = 0.0;
  for (int t = threadIdx.x; t < a.frame_length; t += AP_THREADS) {
    int64_t i = start + t;
    double v = 0.0;
    if (a.pad_mode == ITTS_PAD_REFLECT) {
      if (period == 0) {
        i = 0;
      } else {
        i %= period;
        if (i < 0) i += period;
        if (i >= n) i = period - i;
      }
      v = a.x[begin + i];
    } else if (i >= 0 && i < n) {
      v = a.x[begin + i];
    }
    s += v * v;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) a.out[fbegin + f] = sqrt(s / (double)a.frame_length);
}

// ------------------------------------------------------------------------------------------ host side
// offsets of a batch: ascending from 0; the longest signal
int check_offsets(const char* func, const int64_t* h_off, int n_signals, int64_t* longest) {
  *longest = 0;
  for (int s = 0; s < n_signals; ++s) {
    const int64_t len = h_off[s + 1] - h_off[s];
    if (len < 0 || h_off[0] != 0) {
      set_error(std::string(func) + ": offsets must start at 0 and not decrease (signal " + std::to_string(s) + ")");
      return ITTS_E_INVALID;
    }
    *longest = std::max(*longest, len);
  }
  return ITTS_OK;
}

// a launch HIP would refuse is refused here, by name (hop 1 on hours of audio, millions of signals)
#define AP_REQUIRE_GRID(blocks, what)                                                                             \
  ITTS_REQUIRE((int64_t)(blocks) <= AP_MAX_GRID_X, std::to_string((int64_t)(blocks)) + " workgroups for " + (what) + \
                                                       ": more than " + std::to_string(AP_MAX_GRID_X))

#define AP_REQUIRE_TAPS(numtaps, cap)                                                                             \
  ITTS_REQUIRE((numtaps) >= 1 && (numtaps) % 2 == 1 && (numtaps) <= (cap),                                        \
               "numtaps = " + std::to_string(numtaps) + " must be odd and within 1 .. " + std::to_string(cap))

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int64_t itts_fir_filtfilt_workspace_bytes(int64_t n_total, int n_signals, int numtaps) {
  if (n_total <= 0 || n_signals <= 0 || numtaps < 1) return 0;
  return (n_total + (int64_t)n_signals * 3 * numtaps) * (int64_t)sizeof(double);
}

extern "C" int itts_fir_filtfilt_batch(const double* d_x, const int64_t* h_offsets, int n_signals,
                                       const double* d_taps, int numtaps, double* d_y, void* d_workspace,
                                       void* stream) {
  AP_REQUIRE_TAPS(numtaps, FIR_MAX_TAPS);
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_offsets, "null pointer: h_offsets");
  int64_t longest = 0;
  if (int rc = check_offsets(__func__, h_offsets, n_signals, &longest)) return rc;
  const int64_t L = 3 * (int64_t)numtaps;
  for (int s = 0; s < n_signals; ++s) {
    const int64_t len = h_offsets[s + 1] - h_offsets[s];
    ITTS_REQUIRE(len > L, "signal " + std::to_string(s) + " has " + std::to_string(len) +
                              " samples: the length of the input vector x must be greater than padlen, which is " +
                              std::to_string(L));
  }
  AP_REQUIRE_GRID((longest + L + FIR_TILE - 1) / FIR_TILE, "the longest signal");
  ITTS_REQUIRE(d_x && d_taps && d_y && d_workspace, "null pointer with n_signals = " + std::to_string(n_signals));
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  int64_t* d_off = nullptr;
  if (int rc = upload_i64(h_offsets, n_signals + 1, &d_off, scratch)) return rc;
  FirArgs a{};
  a.x = d_x; a.ws = reinterpret_cast<double*>(d_workspace); a.y = d_y; a.off = d_off; a.taps = d_taps;
  a.numtaps = numtaps; a.nk = (numtaps + FIR_R - 1) / FIR_R; a.L = (int)L; a.W = fir_columns(a.nk);
  const size_t lds = (size_t)(FIR_R * a.W + FIR_R * a.nk) * sizeof(double);
  for (int s0 = 0; s0 < n_signals; s0 += AP_MAX_GRID_Y) {
    a.sig0 = s0;
    const unsigned ny = (unsigned)std::min(AP_MAX_GRID_Y, n_signals - s0);
    fir_unit_kernel<1><<<dim3((unsigned)((longest + L + FIR_TILE - 1) / FIR_TILE), ny), AP_THREADS, lds, s>>>(a);
    ITTS_LAUNCH_CHECK();
    fir_unit_kernel<2><<<dim3((unsigned)((longest + FIR_TILE - 1) / FIR_TILE), ny), AP_THREADS, lds, s>>>(a);
    ITTS_LAUNCH_CHECK();
  }
  return ITTS_OK;
}

extern "C" int itts_resample_poly_batch(const double* d_x, const int64_t* h_offsets, const int64_t* h_out_offsets,
                                        int n_signals, int up, int down, const double* d_taps, int numtaps,
                                        double* d_y, void* stream) {
  ITTS_REQUIRE(up >= 1 && up <= RS_MAX_RATE, "up = " + std::to_string(up) + " is outside 1 .. " +
                                                 std::to_string(RS_MAX_RATE));
  ITTS_REQUIRE(down >= 1 && down <= RS_MAX_RATE, "down = " + std::to_string(down) + " is outside 1 .. " +
                                                     std::to_string(RS_MAX_RATE));
  AP_REQUIRE_TAPS(numtaps, 2 * 10 * RS_MAX_RATE + 1);
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_offsets && h_out_offsets, "null pointer: offsets");
  int64_t longest = 0, longest_out = 0;
  if (int rc = check_offsets(__func__, h_offsets, n_signals, &longest)) return rc;
  if (int rc = check_offsets(__func__, h_out_offsets, n_signals, &longest_out)) return rc;
  for (int s = 0; s < n_signals; ++s) {
    const int64_t n = h_offsets[s + 1] - h_offsets[s], n_out = h_out_offsets[s + 1] - h_out_offsets[s];
    ITTS_REQUIRE(n_out == (n * up + down - 1) / down,
                 "signal " + std::to_string(s) + ": " + std::to_string(n_out) + " output samples, ceil(n * up / down) = " +
                     std::to_string((n * up + down - 1) / down));
  }
  if (longest_out == 0) return ITTS_OK;
  AP_REQUIRE_GRID((longest_out + resample_tile(up, down) - 1) / resample_tile(up, down), "the longest output");
  ITTS_REQUIRE(d_x && d_taps && d_y, "null pointer with n_signals = " + std::to_string(n_signals));
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  std::vector<int64_t> h(2 * (size_t)n_signals + 2);
  std::copy(h_offsets, h_offsets + n_signals + 1, h.begin());
  std::copy(h_out_offsets, h_out_offsets + n_signals + 1, h.begin() + n_signals + 1);
  int64_t* d_off = nullptr;
  if (int rc = upload_i64(h.data(), (int)h.size(), &d_off, scratch)) return rc;
  ResampleArgs a{};
  a.x = d_x; a.off = d_off; a.out_off = d_off + n_signals + 1; a.taps = d_taps; a.y = d_y;
  a.numtaps = numtaps; a.up = up; a.down = down; a.T = resample_tile(up, down);
  for (int s0 = 0; s0 < n_signals; s0 += AP_MAX_GRID_Y) {
    a.sig0 = s0;
    const unsigned ny = (unsigned)std::min(AP_MAX_GRID_Y, n_signals - s0);
    resample_kernel<<<dim3((unsigned)((longest_out + a.T - 1) / a.T), ny), AP_THREADS, 0, s>>>(a);
    ITTS_LAUNCH_CHECK();
  }
  return ITTS_OK;
}

extern "C" int itts_loudness_normalise_batch(const double* d_x, const int64_t* h_offsets, int n_signals,
                                             double ref_rms, double* d_y, void* stream) {
  ITTS_REQUIRE(ref_rms > 0.0, "ref_rms = " + std::to_string(ref_rms) + " must be positive");
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_offsets, "null pointer: h_offsets");
  int64_t longest = 0;
  if (int rc = check_offsets(__func__, h_offsets, n_signals, &longest)) return rc;
  if (longest == 0) return ITTS_OK;
  AP_REQUIRE_GRID(n_signals, "n_signals = " + std::to_string(n_signals));
  ITTS_REQUIRE(d_x && d_y, "null pointer with n_signals = " + std::to_string(n_signals));
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  int64_t* d_off = nullptr;
  if (int rc = upload_i64(h_offsets, n_signals + 1, &d_off, scratch)) return rc;
  LoudArgs a{};
  a.x = d_x; a.y = d_y; a.off = d_off; a.n_signals = n_signals; a.ref_rms = ref_rms;
  a.pitch = (longest + LD_CHUNK - 1) / LD_CHUNK;
  ITTS_HIP_CHECK(scratch.take(&a.partial, (size_t)(a.pitch + 3) * n_signals));
  a.stat = a.partial + a.pitch * n_signals;
  const unsigned nx = (unsigned)a.pitch;
  for (int pass = 0; pass < 3; ++pass) {
    for (int s0 = 0; s0 < n_signals; s0 += AP_MAX_GRID_Y) {
      a.sig0 = s0;
      const dim3 grid(nx, (unsigned)std::min(AP_MAX_GRID_Y, n_signals - s0));
      if (pass == 0) loud_partial_kernel<0><<<grid, AP_THREADS, 0, s>>>(a);
      else if (pass == 1) loud_partial_kernel<1><<<grid, AP_THREADS, 0, s>>>(a);
      else loud_partial_kernel<2><<<grid, AP_THREADS, 0, s>>>(a);
      ITTS_LAUNCH_CHECK();
    }
    const dim3 one_each((unsigned)n_signals);
    if (pass == 0) loud_final_kernel<0><<<one_each, kWave, 0, s>>>(a);
    else if (pass == 1) loud_final_kernel<1><<<one_each, kWave, 0, s>>>(a);
    else loud_final_kernel<2><<<one_each, kWave, 0, s>>>(a);
    ITTS_LAUNCH_CHECK();
  }
  for (int s0 = 0; s0 < n_signals; s0 += AP_MAX_GRID_Y) {
    a.sig0 = s0;
    loud_apply_kernel<<<dim3(nx, (unsigned)std::min(AP_MAX_GRID_Y, n_signals - s0)), AP_THREADS, 0, s>>>(a);
    ITTS_LAUNCH_CHECK();
  }
  return ITTS_OK;
}

extern "C" int itts_frame_rms_batch(const double* d_x, const int64_t* h_offsets, const int64_t* h_frame_offsets,
                                    int n_signals, int frame_length, int hop, int pad_mode, double* d_rms,
                                    void* stream) {
  ITTS_REQUIRE(frame_length >= 1 && frame_length <= RMS_MAX_FRAME,
               "frame_length = " + std::to_string(frame_length) + " is outside 1 .. " + std::to_string(RMS_MAX_FRAME));
  ITTS_REQUIRE(hop >= 1, "hop = " + std::to_string(hop) + " must be at least 1");
  ITTS_REQUIRE(pad_mode == ITTS_PAD_CONSTANT || pad_mode == ITTS_PAD_REFLECT,
               "pad_mode = " + std::to_string(pad_mode) + " is neither ITTS_PAD_CONSTANT nor ITTS_PAD_REFLECT");
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_offsets && h_frame_offsets, "null pointer: offsets");
  int64_t longest = 0, most_frames = 0;
  if (int rc = check_offsets(__func__, h_offsets, n_signals, &longest)) return rc;
  if (int rc = check_offsets(__func__, h_frame_offsets, n_signals, &most_frames)) return rc;
  for (int s = 0; s < n_signals; ++s) {
    const int64_t n = h_offsets[s + 1] - h_offsets[s], nf = h_frame_offsets[s + 1] - h_frame_offsets[s];
    ITTS_REQUIRE(n >= 1, "signal " + std::to_string(s) + " is empty");
    const int64_t padded = n + 2 * (int64_t)(frame_length / 2);
    const int64_t want = padded >= frame_length ? 1 + (padded - frame_length) / hop : 0;
    ITTS_REQUIRE(nf == want, "signal " + std::to_string(s) + ": " + std::to_string(nf) + " frames, the padded signal has " +
                                 std::to_string(want));
  }
  if (most_frames == 0) return ITTS_OK;
  ITTS_REQUIRE(most_frames <= AP_MAX_GRID_X, std::to_string(most_frames) + " frames in one signal: more than " +
                                                 std::to_string(AP_MAX_GRID_X));
  ITTS_REQUIRE(d_x && d_rms, "null pointer with n_signals = " + std::to_string(n_signals));
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  std::vector<int64_t> h(2 * (size_t)n_signals + 2);
  std::copy(h_offsets, h_offsets + n_signals + 1, h.begin());
  std::copy(h_frame_offsets, h_frame_offsets + n_signals + 1, h.begin() + n_signals + 1);
  int64_t* d_off = nullptr;
  if (int rc = upload_i64(h.data(), (int)h.size(), &d_off, scratch)) return rc;
  RmsArgs a{};
  a.x = d_x; a.off = d_off; a.f_off = d_off + n_signals + 1; a.out = d_rms;
  a.frame_length = frame_length; a.hop = hop; a.pad_mode = pad_mode;
  for (int s0 = 0; s0 < n_signals; s0 += AP_MAX_GRID_Y) {
    a.sig0 = s0;
    frame_rms_kernel<<<dim3((unsigned)most_frames, (unsigned)std::min(AP_MAX_GRID_Y, n_signals - s0)), AP_THREADS, 0,
                       s>>>(a);
    ITTS_LAUNCH_CHECK();
  }
  return ITTS_OK;
}
