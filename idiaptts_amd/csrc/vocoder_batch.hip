// Training batches of the sample-level vocoder from a corpus that lives on the device: one launch writes the targets
// and the up-sampled conditioning of B windows (model_trainers/WaveNetVocoderTrainer.py of the reference gets them from
// RawWaveformLabelGen's whole-utterance one-hot, sample_linearly as a preprocessing_fn, a cut to max_frames, a padded
// collate and a transpose: 108 MB through the host for one utterance of 6.6 s).
//
// The corpus is d_x (float64 samples in [-1, 1), utterances back to back) and d_feat (float32 rows of cin conditioning
// features, back to back).  Window b is five int64 of h_windows: the index in d_x of its first sample, its length
// len_b <= W, the first row of its utterance in d_feat, the utterance's T frames, and the place a of its first sample
// in the utterance.  Sample a + j pairs with row a + j of the utterance's m T up-sampled rows (alignment at the front).
//
// Lanes run along t, one lane per output column, workgroups of 256 columns on grid.x and the windows on grid.y: every
// store of a wave is 256 contiguous bytes of one [b, c, :] row.  A lane computes its class once (mulaw_index,
// rawwave.h: the float64 companding of itts_mulaw_encode_f64) and writes its column of mu + 1 values, a 1 at the class;
// without mu it writes (float) x.  Then it places itself once among the utterance's frames (lin_pos at the
// WHOLE utterance's linspace position a + j, so a window equals the slice of sample_linearly of the utterance, bit for
// bit: the same statements, rawwave.h) and writes its column of cin interpolated values; the two feature rows it
// reads are shared by the m lanes of a frame and stay in the caches.  Columns j >= len_b are zeros.  Every element of
// d_target [B, C, W] and d_cond [B, cin, W] is written, nothing else is, and nothing of the corpus outside
// x[first .. first + len) and the T rows of the utterance is read.
//
// The launch writes B W (C + cin) 4 bytes and reads B W 8 bytes of samples plus a few feature rows: it is a store
// stream.  A window's bits depend on its five numbers alone -- not on B, not on its place in the batch; no atomics:
// repeated calls give identical bits.
#include <math.h>

#include "common.h"
#include "context.h"
#include "rawwave.h"

namespace itts {
namespace {

constexpr int VW_THREADS = 256;
constexpr int VW_FIELDS = 5;              // int64 values of a window in h_windows
constexpr int VW_MAX_MU = 4095;           // the strided cross-entropy kernel's 4096 classes
constexpr int VW_MAX_CIN = 128;           // the network's conditioning channels
constexpr int VW_MAX_B = 65535;           // grid.y
constexpr int64_t VW_MAX_GRID_X = (1 << 24) - 1;

struct VwArgs {
  const double* x;
  const float* feat;
  const int64_t* win;           // [B, VW_FIELDS]: first sample, len, first frame row, T, a
  float* target;                // [B, C, W]
  float* cond;                  // [B, cin, W]
  double mu, log1pmu;
  int64_t W;
  int C, cin, m;
  bool onehot;
};

__global__ __launch_bounds__(VW_THREADS) void vocoder_windows_kernel(VwArgs a) {
  const int64_t t = (int64_t)blockIdx.x * VW_THREADS + threadIdx.x;
  if (t >= a.W) return;
  const int64_t b = blockIdx.y;
  const int64_t* w = a.win + b * VW_FIELDS;
  const int64_t first = w[0], len = w[1];
  const bool live = t < len;
  float* tg = a.target + b * a.C * a.W + t;
  if (a.onehot) {
    const int64_t cls = live ? mulaw_index(a.x[first + t], a.mu, a.log1pmu) : -1;
#pragma unroll 8
    for (int c = 0; c < a.C; ++c) tg[c * a.W] = c == cls ? 1.f : 0.f;
  } else {
    tg[0] = live ? (float)a.x[first + t] : 0.f;
  }
  if (a.cin == 0) return;
  float* cd = a.cond + b * a.cin * a.W + t;
  if (!live) {
#pragma unroll 8
    for (int d = 0; d < a.cin; ++d) cd[d * a.W] = 0.f;
    return;
  }
  const int64_t T = w[3];
  const LinPos p = lin_pos(w[4] + t, T, T * a.m);
  const float* f = a.feat + w[2] * a.cin;
#pragma unroll 4
  for (int d = 0; d < a.cin; ++d) cd[d * a.W] = (float)lin_value(f + d, (int64_t)a.cin, p);
}

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int itts_vocoder_windows(const double* d_x, int64_t n_x, const float* d_feat, int64_t n_rows, int cin,
                                    int m, int mu, const int64_t* h_windows, int B, int64_t W, float* d_target,
                                    float* d_cond, void* stream) {
  ITTS_REQUIRE(mu >= 0 && mu <= VW_MAX_MU, "mu = " + std::to_string(mu) + " is outside 0 .. " +
                                               std::to_string(VW_MAX_MU) + " (0: scalar targets)");
  ITTS_REQUIRE(cin >= 0 && cin <= VW_MAX_CIN,
               "cin = " + std::to_string(cin) + " is outside 0 .. " + std::to_string(VW_MAX_CIN));
  ITTS_REQUIRE(m >= 1, "in_to_out_multiplier m = " + std::to_string(m) + " is below 1");
  ITTS_REQUIRE(W >= 1, "W = " + std::to_string(W) + " is not positive");
  ITTS_REQUIRE(B >= 0, "B = " + std::to_string(B) + " is negative");
  ITTS_REQUIRE(B <= VW_MAX_B, "B = " + std::to_string(B) + " exceeds " + std::to_string(VW_MAX_B));
  ITTS_REQUIRE(n_x >= 0, "n_x = " + std::to_string(n_x) + " is negative");
  ITTS_REQUIRE(n_rows >= 0, "n_rows = " + std::to_string(n_rows) + " is negative");
  if (B == 0) return ITTS_OK;
  const int64_t blocks = (W + VW_THREADS - 1) / VW_THREADS;
  ITTS_REQUIRE(blocks <= VW_MAX_GRID_X, "W = " + std::to_string(W) + " is too large");
  ITTS_REQUIRE(h_windows, "null pointer: h_windows");
  for (int b = 0; b < B; ++b) {
    const int64_t* w = h_windows + (int64_t)b * VW_FIELDS;
    const std::string who = "window " + std::to_string(b);
    ITTS_REQUIRE(w[1] >= 1 && w[1] <= W,
                 who + " has len = " + std::to_string(w[1]) + ", outside 1 .. W = " + std::to_string(W));
    ITTS_REQUIRE(w[0] >= 0 && w[0] <= n_x - w[1], who + " reads samples " + std::to_string(w[0]) + " .. " +
                                                      std::to_string(w[0] + w[1]) + " of the " +
                                                      std::to_string(n_x) + " in d_x");
    if (cin == 0) continue;
    ITTS_REQUIRE(w[3] >= 2, who + " has T = " + std::to_string(w[3]) + " frames: linear interpolation needs at least 2");
    // (m T - 1 and every position below it are whole numbers a double holds exactly)
    ITTS_REQUIRE(w[3] <= ((int64_t)1 << 52) / m, who + " has T = " + std::to_string(w[3]) + " frames: m T exceeds 2^52");
    ITTS_REQUIRE(w[2] >= 0 && w[2] <= n_rows - w[3], who + " reads frame rows " + std::to_string(w[2]) + " .. " +
                                                         std::to_string(w[2] + w[3]) + " of the " +
                                                         std::to_string(n_rows) + " in d_feat");
    ITTS_REQUIRE(w[4] >= 0 && w[4] <= w[3] * m - w[1],
                 who + " starts at a = " + std::to_string(w[4]) + " with len = " + std::to_string(w[1]) +
                     ": outside the m T = " + std::to_string(w[3] * m) + " up-sampled rows");
  }
  ITTS_REQUIRE(d_x && d_target, "null pointer (d_x / d_target) with B = " + std::to_string(B));
  ITTS_REQUIRE(cin == 0 || (d_feat && d_cond), "null pointer (d_feat / d_cond) with cin = " + std::to_string(cin));
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  int64_t* d_win = nullptr;
  if (int rc = upload_i64(h_windows, B * VW_FIELDS, &d_win, scratch)) return rc;
  VwArgs a{};
  a.x = d_x; a.feat = d_feat; a.win = d_win; a.target = d_target; a.cond = d_cond;
  a.onehot = mu >= 1;
  a.mu = (double)mu; a.log1pmu = log(1.0 + mu);
  a.W = W; a.C = mu + 1; a.cin = cin; a.m = m;
  vocoder_windows_kernel<<<dim3((unsigned)blocks, (unsigned)B), VW_THREADS, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
