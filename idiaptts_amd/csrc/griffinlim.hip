// Griffin-Lim phase reconstruction (librosa.griffinlim with the reference's arguments).
//
// Replaces (reference call sites):
//   librosa.griffinlim   src/data_preparation/audio/AudioProcessing.py:279-289 (amp_sp_to_raw)
//                        src/Synthesiser.py:320-351 (run_griffin_lim, run_griffin_lim_on_log)
//
// One launch per iteration fuses  istft -> overlap-add -> / window sum-square -> centre padding -> stft ->
// momentum phase update  for every utterance of the call.  A workgroup owns a tile
// of consecutive frames [f0, f1) of one utterance (tiles never cross utterances):
//   1. it inverse-transforms the tile's frames and a halo of h = ceil(n_fft / hop) - 1 frames on each side
//      (frames outside the utterance skipped), one frame per wave on wave_fft.h's fp64 irfft, and
//      overlap-adds them into an fp64 LDS segment of (f1 - f0 - 1) hop + n_fft samples -- untrimmed
//      istft positions [f0 hop, (f1 - 1) hop + n_fft), exactly what the tile's forward frames read.
//      The windowed frames of a round (one per wave) wait in the waves' exchange rows, and every sample
//      adds its frames in ascending frame order: no atomics, the same bits from run to run and for a
//      tile whatever else is in the batch;
//   2. it divides by the window sum-square, summed per sample from the window table over the frames
//      the utterance has (librosa.filters.window_sumsquare), where that is > float32's tiny;
//   3. either (last pass) it writes the trimmed waveform samples it owns, [f0 hop, min(f1 hop, L)),
//      L = hop (T - 1), or it forward-transforms its own frames from the segment -- the centre padding
//      (reflect / zeros) of the trimmed signal is index arithmetic as in stft.hip's padded_sample --
//      and updates the phases:  a = rebuilt - momentum / (1 + momentum) tprev,  angles = a / (|a| + eps),
//      tprev = rebuilt (in place: only this tile touches its frames' rows), the new angles into the
//      other buffer of a ping-pong pair (neighbouring tiles read the old angles in their halos).
// With float32 spectra the state is complex64 (rebuilt and angles rounded where librosa stores them);
// the transforms and the segment are fp64 in both precisions.
// Tiles: the host splits an utterance of T frames into ceil(T / F) tiles of near-equal size, so a tile
// has at least two frames and every padded index a forward frame reads lies inside its segment (see
// tile_frames); F comes from the LDS left beside the twiddle table and the waves' exchange rows.
#include <algorithm>
#include <cfloat>
#include <vector>

#include "context.h"
#include "wave_fft.h"

namespace itts {
namespace {

constexpr int GL_LDS_BUDGET = 160 * 1024;

struct GlArgs {
  const void* S;            // [Ttot, K] float / double
  const void* ang_in;       // [Ttot, K] float2 / double2
  void* ang_out;            // [Ttot, K]
  void* tprev;              // [Ttot, K], updated in place
  const int64_t* f_off;     // [U + 1] rows of the utterances
  const int64_t* y_off;     // [U + 1] output samples, y_off[u + 1] - y_off[u] = hop (T_u - 1)
  const int64_t* tiles;     // [3 n_tiles]: utterance, first frame, end frame
  const double* window;     // [n_fft]
  const double2* tw;        // DeviceContext::tw_compact of n_fft
  int hop;
  int halo;
  int pad;                  // 1: reflect, 2: zeros
  int seg_cap;              // samples the LDS segment holds
  double coef;              // momentum / (1 + momentum)
  double eps;               // tiny of the state's real type
  int final_pass;           // 1: write the waveform instead of the next phases
  void* y;                  // [y_off[U]] float / double
};

template <bool F64> struct State;
template <> struct State<false> {
  typedef float real;
  typedef float2 cplx;
  static __device__ __forceinline__ double2 load(const cplx* p) { const float2 v = *p; return make_double2(v.x, v.y); }
  static __device__ __forceinline__ double2 round(double2 v) { return make_double2((float)v.x, (float)v.y); }
  static __device__ __forceinline__ void store(cplx* p, double2 v) { *p = make_float2((float)v.x, (float)v.y); }
};
template <> struct State<true> {
  typedef double real;
  typedef double2 cplx;
  static __device__ __forceinline__ double2 load(const cplx* p) { return *p; }
  static __device__ __forceinline__ double2 round(double2 v) { return v; }
  static __device__ __forceinline__ void store(cplx* p, double2 v) { *p = v; }
};

// window sum-square at untrimmed position i of an utterance of T frames, frames added in ascending order
__device__ __forceinline__ double window_sumsq(const double* __restrict__ w, int64_t i, int64_t T, int hop, int n_fft) {
  int64_t t0 = i - n_fft + 1 <= 0 ? 0 : (i - n_fft + hop) / hop;
  const int64_t t1 = std::min<int64_t>(T - 1, i / hop);
  double s = 0.0;
  for (int64_t t = t0; t <= t1; ++t) {
    const double v = w[i - t * hop];
    s += v * v;
  }
  return s;
}

template <int R, int TH, bool F64>
__global__ __launch_bounds__(TH) void griffinlim_kernel(GlArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef State<F64> St;
  typedef typename St::real real;
  typedef typename St::cplx cplx;
  constexpr int FFT = 128 * R, H = 64 * R, K = H + 1, NW = TH / 64;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = wf::lane_id();
  typename wf::PlanOf<R>::type P;
  wf::table_init<R>(smem, a.tw);          // (ends with a barrier)
  char* rows_base = smem + wf::table_bytes<R>();
  char* rows = rows_base + (size_t)wv * wf::lds_bytes<R>();
  wf::plan_init(P, a.tw, rows, smem);
  double* R64 = reinterpret_cast<double*>(rows);          // this wave's exchange rows as doubles
  double* seg = reinterpret_cast<double*>(rows_base + (size_t)NW * wf::lds_bytes<R>());

  const int64_t u = a.tiles[3 * blockIdx.x], f0 = a.tiles[3 * blockIdx.x + 1], f1 = a.tiles[3 * blockIdx.x + 2];
  const int64_t r0 = a.f_off[u], T = a.f_off[u + 1] - r0;
  const int hop = a.hop;
  const int64_t s0 = f0 * hop;                              // untrimmed position of seg[0]
  const int n_seg = (int)((f1 - f0 - 1) * hop + FFT);
  for (int p = threadIdx.x; p < n_seg; p += TH) seg[p] = 0.0;

  // 1. inverse transforms of [ta, tb) and overlap-add, NW frames per round
  const int64_t ta = f0 - a.halo > 0 ? f0 - a.halo : 0;
  const int64_t tb = f1 + a.halo < T ? f1 + a.halo : T;
  const real* S = reinterpret_cast<const real*>(a.S);
  const cplx* A = reinterpret_cast<const cplx*>(a.ang_in);
  for (int64_t base = ta; base < tb; base += NW) {
    const int n_round = (int)std::min<int64_t>(NW, tb - base);
    const int64_t t = base + wv;
    if (wv < n_round) {
      const int64_t g = (r0 + t) * K;
      double2 z[R], xh = make_double2(0.0, 0.0);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int k = l + 64 * q;
        const double s = (double)S[g + k];
        const double2 ang = St::load(A + g + k);
        z[q] = St::round(make_double2(s * ang.x, s * ang.y));
      }
      if (l == 0) {
        const double s = (double)S[g + H];
        const double2 ang = St::load(A + g + H);
        xh = St::round(make_double2(s * ang.x, s * ang.y));
      }
      wf::irfft<R>(z, xh, P);
      // z[q] = (x[2 m], x[2 m + 1]), m = l + 64 q: windowed samples into the rows (buffer free after irfft)
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int m = l + 64 * q;
        reinterpret_cast<double2*>(R64)[m] = make_double2(z[q].x * a.window[2 * m], z[q].y * a.window[2 * m + 1]);
      }
    }
    __syncthreads();
    // seg positions the round touches: [(base - f0) hop, (base + n_round - 1 - f0) hop + FFT) clipped to the segment
    const int64_t rel = (base - f0) * hop;
    const int p_lo = (int)std::max<int64_t>(0, rel);
    const int p_hi = (int)std::min<int64_t>(n_seg, rel + (int64_t)(n_round - 1) * hop + FFT);
    for (int p = p_lo + threadIdx.x; p < p_hi; p += TH) {
      const int64_t d0 = p - rel;                          // offset inside the round's first frame
      const int k_hi = (int)std::min<int64_t>(n_round - 1, d0 / hop);
      const int k_lo = d0 < FFT ? 0 : (int)((d0 - FFT + hop) / hop);
      double acc = seg[p];
      for (int k = k_lo; k <= k_hi; ++k) {
        const double* rk = reinterpret_cast<const double*>(rows_base + (size_t)k * wf::lds_bytes<R>());
        acc += rk[d0 - (int64_t)k * hop];
      }
      seg[p] = acc;
    }
    __syncthreads();
  }

  // 2. window sum-square
  for (int p = threadIdx.x; p < n_seg; p += TH) {
    const double wss = window_sumsq(a.window, s0 + p, T, hop, FFT);
    if (wss > (double)FLT_MIN) seg[p] /= wss;
  }
  __syncthreads();

  const int64_t L = (T - 1) * hop;                         // trimmed signal length
  if (a.final_pass) {
    real* y = reinterpret_cast<real*>(a.y) + a.y_off[u];
    const int64_t j_hi = std::min<int64_t>(f1 * hop, L);
    for (int64_t j = s0 + threadIdx.x; j < j_hi; j += TH) y[j] = (real)seg[j + FFT / 2 - s0];
    return;
  }

  // 3. forward transforms of the tile's own frames and the phase update
  cplx* AO = reinterpret_cast<cplx*>(a.ang_out);
  cplx* TP = reinterpret_cast<cplx*>(a.tprev);
  const double coef = a.coef, eps = a.eps;
  for (int64_t t = f0 + wv; t < f1; t += NW) {
#pragma unroll 2
    for (int j = 0; j < 2 * R; ++j) {
      const int n = l + 64 * j;
      int64_t y_idx = t * hop + n - FFT / 2;              // index into the trimmed signal
      double v;
      if (y_idx < 0 || y_idx >= L) {
        if (a.pad == 1 && L > 1) {
          const int64_t per = 2 * (L - 1);
          y_idx %= per;
          if (y_idx < 0) y_idx += per;
          if (y_idx >= L) y_idx = per - y_idx;
        } else if (a.pad == 1) {
          y_idx = 0;
        } else {
          y_idx = -1;
        }
      }
      if (y_idx >= 0) {
        int64_t p = y_idx + FFT / 2 - s0;
        p = p < 0 ? 0 : (p >= n_seg ? n_seg - 1 : p);       // (never clamps: see tile_frames)
        v = seg[p];
      } else {
        v = 0.0;
      }
      R64[n] = a.window[n] * v;
    }
    wf::wave_sync();
    double2 z[R], xh;
#pragma unroll
    for (int q = 0; q < R; ++q) z[q] = reinterpret_cast<const double2*>(R64)[l + 64 * q];
    wf::wave_sync();
    wf::rfft<R>(z, xh, P);
    cplx* ao = AO + (r0 + t) * K;
    cplx* tpr = TP + (r0 + t) * K;
    auto update = [ao, tpr, coef, eps](int k, double2 x) {
      const double2 rb = St::round(x);
      const double2 tp = St::load(tpr + k);
      const double2 d = make_double2(rb.x - coef * tp.x, rb.y - coef * tp.y);
      const double den = sqrt(d.x * d.x + d.y * d.y) + eps;
      St::store(ao + k, make_double2(d.x / den, d.y / den));
      St::store(tpr + k, rb);
    };
#pragma unroll
    for (int q = 0; q < R; ++q) update(l + 64 * q, z[q]);
    if (l == 0) update(H, xh);
  }
}

template <int R, int TH, bool F64>
int launch_gl(const GlArgs& a, int n_tiles, hipStream_t s) {
  const size_t lds = wf::table_bytes<R>() + (size_t)(TH / 64) * wf::lds_bytes<R>() + (size_t)a.seg_cap * 8;
  ITTS_REQUIRE(lds <= GL_LDS_BUDGET, "LDS budget exceeded");
  ITTS_HIP_CHECK(itts::allow_dynamic_lds((const void*)griffinlim_kernel<R, TH, F64>, lds));
  hipLaunchKernelGGL((griffinlim_kernel<R, TH, F64>), dim3((unsigned)n_tiles), dim3(TH), lds, s, a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// waves per workgroup: 12 for 1024 points (3 per SIMD), 6 for 2048 (the exchange rows are twice as large)
int gl_waves(int n_fft) { return n_fft == 1024 ? 12 : 6; }

// Largest tile (frames) whose segment fits beside the table and the exchange rows; a multiple of the wave
// count when it is at least that.  0 when even the smallest safe tile does not fit.
int tile_frames(int n_fft, int hop) {
  const int nw = gl_waves(n_fft);
  const int fixed = n_fft == 1024 ? wf::table_bytes<8>() + nw * wf::lds_bytes<8>()
                                  : wf::table_bytes<16>() + nw * wf::lds_bytes<16>();
  const int samples = (GL_LDS_BUDGET - fixed) / 8;
  if (samples < n_fft) return 0;
  int F = (samples - n_fft) / hop + 1;
  if (F >= nw) F -= F % nw;
  // An utterance that fits one tile reads every padded index from that tile's segment.  One that does not has
  // tiles of >= F / 2 frames and L >= F hop > n_fft: the reflection is single, the frames that reflect at the
  // start lie in the first tile, and every reflected index lies in the segment of the tile that reads it.
  if (F < 2 || (int64_t)F * hop <= n_fft) return 0;
  return F;
}

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int itts_griffinlim_tile_frames(int n_fft, int hop) {
  if ((n_fft != 1024 && n_fft != 2048) || hop <= 0 || hop > n_fft / 2) return 0;
  return tile_frames(n_fft, hop);
}

extern "C" int itts_griffinlim(const void* d_S, void* d_ang_a, void* d_ang_b, void* d_tprev, const int64_t* h_f_off,
                               int n_utts, int n_fft, int hop, int pad_mode, const double* d_window, int n_iter,
                               double momentum, int is_f64, void* d_y, void* stream) {
  ITTS_REQUIRE(h_f_off && n_utts >= 0, "null offsets");
  ITTS_REQUIRE(n_fft == 1024 || n_fft == 2048, "n_fft must be 1024 or 2048");
  ITTS_REQUIRE(hop > 0 && hop <= n_fft / 2, "hop must be in [1, n_fft / 2]");
  ITTS_REQUIRE(pad_mode == 1 || pad_mode == 2, "pad_mode must be 1 (reflect) or 2 (zeros)");
  ITTS_REQUIRE(n_iter >= 0, "n_iter must not be negative");
  ITTS_REQUIRE(momentum >= 0.0, "momentum must not be negative");
  ITTS_REQUIRE(n_utts == 0 || h_f_off[0] == 0, "f_off[0] must be 0");
  const int F = tile_frames(n_fft, hop);
  ITTS_REQUIRE(F > 0, "hop too small for the LDS segment");
  // tiles: ceil(T / F) per utterance, of near-equal size (>= 2 frames each, since T >= 2)
  std::vector<int64_t> h(2 * (size_t)n_utts + 2);
  std::vector<int64_t> tiles;
  h[0] = 0;
  for (int u = 0; u < n_utts; ++u) {
    const int64_t T = h_f_off[u + 1] - h_f_off[u];
    ITTS_REQUIRE(T >= 2, "every spectrum needs at least 2 frames");
    h[u + 1] = h_f_off[u + 1];
    h[n_utts + 2 + u] = h[n_utts + 1 + u] + (T - 1) * hop;
    const int64_t nt = (T + F - 1) / F;
    for (int64_t k = 0; k < nt; ++k) {
      tiles.push_back(u);
      tiles.push_back(k * T / nt);
      tiles.push_back((k + 1) * T / nt);
    }
  }
  if (n_utts == 0) return ITTS_OK;
  ITTS_REQUIRE(d_S && d_ang_a && d_ang_b && d_tprev && d_window && d_y, "null pointer");
  ITTS_REQUIRE(tiles.size() / 3 <= 0x7fffffff, "too many tiles");
  DeviceContext* ctx = get_context();
  if (!ctx) return ITTS_E_HIP;
  hipStream_t s = as_stream(stream);
  itts::ScratchScope scratch(s);
  const int n_tiles = (int)(tiles.size() / 3);
  h.insert(h.end(), tiles.begin(), tiles.end());
  int64_t* d_off = nullptr;
  int rc = upload_i64(h.data(), (int)h.size(), &d_off, scratch);
  if (rc != ITTS_OK) return rc;
  const int64_t K = n_fft / 2 + 1, rows = h_f_off[n_utts];
  ITTS_HIP_CHECK(hipMemsetAsync(d_tprev, 0, (size_t)rows * K * (is_f64 ? 16 : 8), s));
  GlArgs a{d_S, nullptr, nullptr, d_tprev, d_off, d_off + n_utts + 1, d_off + 2 * (size_t)n_utts + 2, d_window,
           ctx->tw_compact[n_fft == 1024 ? 10 : 11], hop, (n_fft + hop - 1) / hop - 1, pad_mode,
           (int)((F - 1) * (int64_t)hop + n_fft), momentum / (1.0 + momentum), is_f64 ? DBL_MIN : (double)FLT_MIN,
           0, d_y};
  void* buf[2] = {d_ang_a, d_ang_b};
  for (int it = 0; it <= n_iter; ++it) {
    a.ang_in = buf[it & 1];
    a.ang_out = buf[(it + 1) & 1];
    a.final_pass = it == n_iter;
    if (n_fft == 1024)
      rc = is_f64 ? launch_gl<8, 768, true>(a, n_tiles, s) : launch_gl<8, 768, false>(a, n_tiles, s);
    else
      rc = is_f64 ? launch_gl<16, 384, true>(a, n_tiles, s) : launch_gl<16, 384, false>(a, n_tiles, s);
    if (rc) return rc;
  }
  return ITTS_OK;
}
