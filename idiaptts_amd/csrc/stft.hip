// Short-time Fourier transform features: amplitude spectrum, its dB form and mel filter banks.
//
// Replaces (reference call sites):
//   librosa.stft + np.abs / sqrt(K)      src/data_preparation/audio/AudioProcessing.py:156-185
//   librosa.feature.melspectrogram (S=)  AudioProcessing.py:187-226
//   amp_to_db on the result              AudioProcessing.py:334-336, WorldFeatLabelGen.py:865-874
//
// One WAVE per frame on wave_fft.h's fp64 real transform (1024 points: 16 - 24 kHz, 2048: 44.1 / 48 kHz).
// The wave gathers its n_fft samples straight from the utterance -- the centre padding (reflect or
// zeros) is index arithmetic, no padded copy of the signal exists --, multiplies by the window table
// the host built (scipy's periodic window, centred in n_fft), transforms and writes one row:
//   kind 0: |X| / sqrt(K) as float32, kind 1: as float64, kind 2: 20 log10(max(1e-5, float32 of it)),
//   mel:    sum_k |X_k| / sqrt(K) * w_m[k] per filter, float32.
// For the mel form the spectrum goes to the wave's own exchange rows (idle after the transform) and
// lane m sums filter m over its contiguous support: every bin lies in at most two triangles, so the
// supports add up to < 2 K weights and the [T, K] spectrum never leaves the chip.  The sum of one
// filter runs in ascending bin order in one lane: results are the same bits from run to run, and no
// atomics are used anywhere.
// Rows: global frame g of the launch belongs to utterance u (f_off[u] <= g < f_off[u + 1]) and is
// STFT frame g - f_off[u] + first[u] of that utterance -- `first` drops frames in front (the
// reference's trim_to_shortest against the WORLD frame count), so the kernel writes exactly the rows
// the feature matrix keeps.
#include <algorithm>
#include <vector>

#include "context.h"
#include "wave_fft.h"
#include "world_dev.h"

namespace itts {
namespace {

struct StftArgs {
  const double* x;          // samples of all utterances back to back
  const int64_t* x_off;     // [U + 1]
  const int64_t* f_off;     // [U + 1] output rows, f_off[0] = 0
  const int64_t* first;     // [U] first STFT frame written per utterance
  int n_utts;
  int64_t t_total;
  int hop;
  int pad;                  // 0: none (center = False), 1: reflect, 2: zeros
  const double* window;     // [n_fft]
  const double2* tw;        // DeviceContext::tw_compact of n_fft
  int kind;                 // 0, 1, 2 (above) or 3: mel
  void* out;
  int64_t ld_out;
  const int* mel_tab;       // [3 n_mels]: first bin, number of bins, first weight
  const float* mel_w;
  int n_mels;
};

// Sample j of an utterance of xl samples with the padding of np.pad (reflect: period 2 (xl - 1), what
// np.pad's repeated reflection amounts to); never an address outside [0, xl).
__device__ __forceinline__ double padded_sample(const double* __restrict__ x, int64_t xl, int64_t j, int pad) {
  if (pad == 1) {
    if (xl > 1) {
      const int64_t p = 2 * (xl - 1);
      j %= p;
      if (j < 0) j += p;
      if (j >= xl) j = p - j;
    } else {
      j = 0;
    }
  }
  return (j >= 0 && j < xl) ? x[j] : 0.0;
}

// TH threads = TH / 64 frames in flight per workgroup; one workgroup per CU (LDS: table + one exchange buffer per wave)
template <int R, int TH>
__global__ __launch_bounds__(TH) void stft_wave_kernel(StftArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int FFT = 128 * R, H = 64 * R, K = H + 1, NW = TH / 64;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = wf::lane_id();
  typename wf::PlanOf<R>::type P;
  wf::table_init<R>(smem, a.tw);
  char* rows = smem + wf::table_bytes<R>() + (size_t)wv * wf::lds_bytes<R>();
  wf::plan_init(P, a.tw, rows, smem);
  double* S = reinterpret_cast<double*>(rows);       // the exchange rows, free between transforms
  const double scale = sqrt((double)K);
  for (int64_t g = (int64_t)blockIdx.x * NW + wv; g < a.t_total; g += (int64_t)gridDim.x * NW) {
    const int u = __builtin_amdgcn_readfirstlane(wd::find_utt_wave(a.f_off, a.n_utts, g));
    const double* x = a.x + a.x_off[u];
    const int64_t xl = a.x_off[u + 1] - a.x_off[u];
    const int64_t start = (g - a.f_off[u] + a.first[u]) * a.hop - (a.pad ? FFT / 2 : 0);
    // windowed frame through the exchange rows: sample i = l + 64 j (coalesced loads), then the packed layout
    // z[q] = (frame[2 m], frame[2 m + 1]), m = l + 64 q
    const bool inside = start >= 0 && start + FFT <= xl;     // wave-uniform: no padding in this frame
#pragma unroll 2
    for (int j = 0; j < 2 * R; ++j) {
      const int i = l + 64 * j;
      const double v = inside ? x[start + i] : padded_sample(x, xl, start + i, a.pad);
      S[i] = a.window[i] * v;
    }
    wf::wave_sync();
    double2 z[R], xh;
#pragma unroll
    for (int q = 0; q < R; ++q) z[q] = reinterpret_cast<const double2*>(S)[l + 64 * q];
    wf::wave_sync();
    wf::rfft<R>(z, xh, P);
    double amp[R], amph = 0.0;
#pragma unroll
    for (int q = 0; q < R; ++q) amp[q] = sqrt(z[q].x * z[q].x + z[q].y * z[q].y) / scale;
    if (l == 0) amph = sqrt(xh.x * xh.x + xh.y * xh.y) / scale;
    if (a.kind == 3) {
#pragma unroll
      for (int q = 0; q < R; ++q) S[l + 64 * q] = amp[q];
      if (l == 0) S[H] = amph;
      wf::wave_sync();
      float* o = reinterpret_cast<float*>(a.out) + g * a.ld_out;
      for (int m = l; m < a.n_mels; m += 64) {
        const int k0 = a.mel_tab[3 * m], n = a.mel_tab[3 * m + 1], w0 = a.mel_tab[3 * m + 2];
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc += S[k0 + j] * (double)a.mel_w[w0 + j];
        o[m] = (float)acc;
      }
      wf::wave_sync();          // every lane has read the spectrum before the next transform reuses the rows
    } else if (a.kind == 1) {
      double* o = reinterpret_cast<double*>(a.out) + g * a.ld_out;
#pragma unroll
      for (int q = 0; q < R; ++q) o[l + 64 * q] = amp[q];
      if (l == 0) o[H] = amph;
    } else {
      float* o = reinterpret_cast<float*>(a.out) + g * a.ld_out;
      auto cvt = [&](double v) -> float {
        const float f = (float)v;
        return a.kind == 2 ? (float)(20.0 * log10(fmax((double)1e-5f, (double)f))) : f;
      };
#pragma unroll
      for (int q = 0; q < R; ++q) o[l + 64 * q] = cvt(amp[q]);
      if (l == 0) o[H] = cvt(amph);
    }
  }
}

// mel projection of a given amplitude spectrum [T, K] f64: one wave per row, lane m sums filter m as above
__global__ __launch_bounds__(256) void mel_project_kernel(const double* __restrict__ amp, int64_t T, int64_t ld_amp,
                                                          const int* __restrict__ tab, const float* __restrict__ w,
                                                          int n_mels, float* __restrict__ out, int64_t ld_out) {
  const int l = wf::lane_id();
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += (int64_t)gridDim.x * 4) {
    const double* s = amp + t * ld_amp;
    for (int m = l; m < n_mels; m += 64) {
      const int k0 = tab[3 * m], n = tab[3 * m + 1], w0 = tab[3 * m + 2];
      double acc = 0.0;
      for (int j = 0; j < n; ++j) acc += s[k0 + j] * (double)w[w0 + j];
      out[t * ld_out + m] = (float)acc;
    }
  }
}

template <int R, int TH>
int launch_stft(const StftArgs& a, hipStream_t s) {
  int dev = 0, n_cu = 256;
  ITTS_HIP_CHECK(hipGetDevice(&dev));
  ITTS_HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  constexpr int NW = TH / 64;
  const size_t lds = wf::table_bytes<R>() + (size_t)NW * wf::lds_bytes<R>();
  ITTS_REQUIRE(lds <= 160 * 1024, "LDS budget exceeded");
  ITTS_HIP_CHECK(itts::allow_dynamic_lds((const void*)stft_wave_kernel<R, TH>, lds));
  const dim3 grid((unsigned)std::min<int64_t>((a.t_total + NW - 1) / NW, n_cu));
  hipLaunchKernelGGL((stft_wave_kernel<R, TH>), grid, dim3(TH), lds, s, a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// Argument checks shared by the two STFT entry points (no device work before they pass).
int check_frames(const int64_t* h_x_off, const int64_t* h_f_off, const int64_t* h_first, int n_utts, int n_fft,
                 int hop, int pad_mode) {
  ITTS_REQUIRE(h_x_off && h_f_off && h_first && n_utts >= 0, "null offsets");
  ITTS_REQUIRE(n_fft == 1024 || n_fft == 2048, "n_fft must be 1024 or 2048");
  ITTS_REQUIRE(hop > 0, "hop must be positive");
  ITTS_REQUIRE(pad_mode >= 0 && pad_mode <= 2, "pad_mode must be 0 (none), 1 (reflect) or 2 (zeros)");
  ITTS_REQUIRE(n_utts == 0 || h_f_off[0] == 0, "f_off[0] must be 0");
  for (int u = 0; u < n_utts; ++u) {
    const int64_t xl = h_x_off[u + 1] - h_x_off[u], nf = h_f_off[u + 1] - h_f_off[u];
    ITTS_REQUIRE(xl >= 0 && nf >= 0 && h_first[u] >= 0, "offsets must not decrease");
    // the frames of an utterance: 1 + n // hop with the centre padding, 1 + (n - n_fft) // hop without
    const int64_t avail = pad_mode ? 1 + xl / hop : (xl >= n_fft ? 1 + (xl - n_fft) / hop : 0);
    ITTS_REQUIRE(nf == 0 || (xl > 0 && h_first[u] + nf <= avail), "more frames asked for than the signal has");
  }
  return ITTS_OK;
}

int run_stft(StftArgs a, const int64_t* h_x_off, const int64_t* h_f_off, const int64_t* h_first, int n_fft,
             hipStream_t s) {
  DeviceContext* ctx = get_context();
  if (!ctx) return ITTS_E_HIP;
  itts::ScratchScope scratch(s);
  const int U = a.n_utts;
  std::vector<int64_t> h(3 * (size_t)U + 2);
  std::copy(h_x_off, h_x_off + U + 1, h.begin());
  std::copy(h_f_off, h_f_off + U + 1, h.begin() + U + 1);
  std::copy(h_first, h_first + U, h.begin() + 2 * (size_t)U + 2);
  int64_t* d_off = nullptr;
  int rc = upload_i64(h.data(), (int)h.size(), &d_off, scratch);
  if (rc != ITTS_OK) return rc;
  a.x_off = d_off;
  a.f_off = d_off + U + 1;
  a.first = d_off + 2 * U + 2;
  a.tw = ctx->tw_compact[n_fft == 1024 ? 10 : 11];
  rc = n_fft == 1024 ? launch_stft<8, 768>(a, s) : launch_stft<16, 512>(a, s);
  if (rc) return rc;
  return ITTS_OK;
}

int check_mel(const int* d_mel_tab, const float* d_mel_w, int n_mels, int K) {
  ITTS_REQUIRE(d_mel_tab && d_mel_w, "null mel table");
  ITTS_REQUIRE(n_mels >= 1 && n_mels <= K, "n_mels must be in [1, n_fft / 2 + 1]");
  return ITTS_OK;
}

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int itts_stft(const double* d_x, const int64_t* h_x_off, const int64_t* h_f_off, const int64_t* h_first,
                         int n_utts, int n_fft, int hop, int pad_mode, const double* d_window, int out_kind,
                         void* d_out, int64_t ld_out, void* stream) {
  int rc = check_frames(h_x_off, h_f_off, h_first, n_utts, n_fft, hop, pad_mode);
  if (rc) return rc;
  ITTS_REQUIRE(out_kind >= 0 && out_kind <= 2, "out_kind must be 0 (f32), 1 (f64) or 2 (dB, f32)");
  ITTS_REQUIRE(ld_out >= n_fft / 2 + 1, "ld_out smaller than n_fft / 2 + 1");
  if (n_utts == 0 || h_f_off[n_utts] == 0) return ITTS_OK;
  ITTS_REQUIRE(d_x && d_window && d_out, "null pointer");
  StftArgs a{d_x, nullptr, nullptr, nullptr, n_utts, h_f_off[n_utts], hop, pad_mode, d_window, nullptr, out_kind,
             d_out, ld_out, nullptr, nullptr, 0};
  return run_stft(a, h_x_off, h_f_off, h_first, n_fft, as_stream(stream));
}

extern "C" int itts_stft_mel(const double* d_x, const int64_t* h_x_off, const int64_t* h_f_off, const int64_t* h_first,
                             int n_utts, int n_fft, int hop, int pad_mode, const double* d_window,
                             const int* d_mel_tab, const float* d_mel_w, int n_mels, float* d_out, int64_t ld_out,
                             void* stream) {
  int rc = check_frames(h_x_off, h_f_off, h_first, n_utts, n_fft, hop, pad_mode);
  if (rc) return rc;
  rc = check_mel(d_mel_tab, d_mel_w, n_mels, n_fft / 2 + 1);
  if (rc) return rc;
  ITTS_REQUIRE(ld_out >= n_mels, "ld_out smaller than n_mels");
  if (n_utts == 0 || h_f_off[n_utts] == 0) return ITTS_OK;
  ITTS_REQUIRE(d_x && d_window && d_out, "null pointer");
  StftArgs a{d_x, nullptr, nullptr, nullptr, n_utts, h_f_off[n_utts], hop, pad_mode, d_window, nullptr, 3,
             d_out, ld_out, d_mel_tab, d_mel_w, n_mels};
  return run_stft(a, h_x_off, h_f_off, h_first, n_fft, as_stream(stream));
}

extern "C" int itts_mel_project(const double* d_amp, int64_t T, int K, int64_t ld_amp, const int* d_mel_tab,
                                const float* d_mel_w, int n_mels, float* d_out, int64_t ld_out, void* stream) {
  ITTS_REQUIRE(T >= 0 && K >= 2 && ld_amp >= K, "bad sizes");
  int rc = check_mel(d_mel_tab, d_mel_w, n_mels, K);
  if (rc) return rc;
  ITTS_REQUIRE(ld_out >= n_mels, "ld_out smaller than n_mels");
  if (T == 0) return ITTS_OK;
  ITTS_REQUIRE(d_amp && d_out, "null pointer");
  const unsigned blocks = (unsigned)std::min<int64_t>((T + 3) / 4, 4096);
  hipLaunchKernelGGL(mel_project_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_amp, T, ld_amp,
                     d_mel_tab, d_mel_w, n_mels, d_out, ld_out);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
