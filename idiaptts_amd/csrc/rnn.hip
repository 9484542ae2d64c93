// (Bi)LSTM, (Bi)GRU and vanilla (Bi)RNN recurrences for padded batches of frame sequences -- the recurrent half of
// the acoustic model of BASELINE config 3 (3 x 512 BiLSTM) and the GRU / RNNTANH / RNNRELU flavours of the recurrent
// groups (`..._BiGRU_...`, `..._BiRNNTANH_...`).  Replaces what torch.nn.LSTM / GRU / RNN do between
// pack_padded_sequence(enforce_sorted=False) and pad_packed_sequence in
// rnn_dyn/RNNWrapper.py:45-107 (cuDNN / MIOpen RNN in the reference).
//
// Split of the work (per layer):
//   * gin = X W_ih^T + bias (LSTM and RNN: b_ih + b_hh, GRU: b_ih) for ALL time steps and both directions is ONE
//     fp32-MFMA GEMM (nn.hip), so are dX, dW_ih, dW_hh and the bias gradients in the backward pass;
//   * only the true recurrence h_{t-1} W_hh^T runs per time step.  Forward and backward: one
//     persistent launch per layer each where it applies (rnn_persist.h: H = 512, every recurrence
//     inside one XCD; LSTM and GRU only).  Otherwise (rnn_step.h): one launch per step, both directions in it: the kernel
//     boundary is the grid-wide dependency (an in-kernel grid barrier ACROSS XCDs costs 2.3-2.5 us
//     on this chip, scripts/handoff_lab).  A workgroup owns a slice of hidden units and
//     streams its W_hh rows and h_{t-1} [B, H] from L2 through v_mfma_f32_16x16x4_f32
//     (exact fp32, same K-permutation trick as the GEMM: one 16-byte load feeds 4 MFMAs).
//   * packed-sequence semantics: row b is active for step s < len_b; the forward direction
//     visits t = s, the reverse direction t = len_b - 1 - s (it starts at each sequence's own
//     last frame); the state of an inactive row is frozen.
//   * packed row layout (what pack_padded_sequence produces): the batch rows are sorted by
//     decreasing length, frame t of row b lives at packed row row_off[t] + b, where
//     row_off[t] = sum_{t' < t} nact(t') and nact(t) = #{b : len_b > t}.  Only valid frames exist,
//     so the GEMMs around the recurrence touch N = sum(len) rows instead of T*B, and step s
//     works on the ceil(nact(s) / 16) batch tiles that still have active rows.  The reverse
//     direction's row at step s, row_off[len_b - 1 - s] + b, comes from a table built once per
//     batch (rev_row[s][b]) so that no step chases lengths -> offsets -> data through memory.
//   * a step is latency bound (one dependent pass over ~10 MB that the previous launch left cold
//     in L2): every operand load of a wave is issued before the first MFMA
//     (__builtin_amdgcn_sched_barrier keeps the scheduler from pairing loads with their MFMAs,
//     which costs ~0.2 us per load when it happens), and every operand load is a contiguous 1 KB
//     wave access thanks to the K-blocked state / re-tiled W_hh layouts of rnn_common.h.
// Gate order (LSTM i, f, g, o; GRU r, z, n), the bias vectors and the cell formulas (rnn_common.h) follow torch.nn.
//
// Every LSTM / GRU entry point: argument checks, the arguments of both kernel families, the persistent attempt, then
// the step driver of rnn_step.h.  The vanilla RNN's: argument checks, then the step driver.

#include "rnn_persist.h"
#include "rnn_step.h"

using namespace itts;

// geometry and tables every call has
static RnnStepArgs step_args(const int* d_rev_row, int T, int B, int H, int ndir) {
  RnnStepArgs a{};
  a.T = T; a.B = B; a.H = H; a.ndir = ndir; a.rev_row = d_rev_row;
  return a;
}

extern "C" int64_t itts_lstm_state_bytes(int B, int H, int ndir) { return rnn_state_bytes(4, B, H, ndir); }
extern "C" int64_t itts_gru_state_bytes(int B, int H, int ndir) { return rnn_state_bytes(3, B, H, ndir); }

// Runs the recurrence of one (bi)directional LSTM layer over T steps (packed rows, see the top).
extern "C" int itts_lstm_layer_fwd(const float* d_gin, const float* d_whh, const float* d_h0,
                                   const float* d_c0, const int* d_lengths, const int* h_lengths,
                                   const int* d_row_off, const int* d_rev_row, int T, int B, int H,
                                   int ndir, float* d_y, float* d_gates, float* d_csave,
                                   float* d_hn, float* d_cn, void* d_state, void* stream) {
  ITTS_REQUIRE(d_gin && d_whh && d_lengths && d_row_off && d_y && d_state, "null pointer");
  ITTS_REQUIRE(ndir == 1 || d_rev_row, "the reverse direction needs its row table");
  ITTS_REQUIRE((d_gates == nullptr) == (d_csave == nullptr),
               "gates / csave must be given together (training) or both NULL (inference)");
  int rc = rnn_check(h_lengths, T, B, H, ndir);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  RnnPersistArgs p{};
  p.gin = d_gin; p.whh = d_whh; p.h0 = d_h0; p.c0 = d_c0; p.lengths = d_lengths; p.row_off = d_row_off;
  p.rev_row = d_rev_row; p.y = d_y; p.gates = d_gates; p.csave = d_csave; p.hn = d_hn; p.cn = d_cn;
  p.T = T; p.B = B; p.ndir = ndir;
  const int done = rnn_persist_forward<4>(p, H, s);
  if (done < 0) return ITTS_E_HIP;
  if (done) return ITTS_OK;
  RnnStepArgs a = step_args(d_rev_row, T, B, H, ndir);
  a.gin = d_gin; a.y = d_y; a.gates = d_gates; a.aux = d_csave;
  return rnn_step_forward<4>(a, d_whh, d_h0, d_c0, d_lengths, h_lengths, d_hn, d_cn, d_state, s);
}

// Backward recurrence: fills d_dg [N, ndir*4H] from d_dy and the saved forward tensors.
extern "C" int itts_lstm_layer_bwd(const float* d_dy, const float* d_whh, const float* d_c0,
                                   const float* d_gates, const float* d_csave, const int* h_lengths,
                                   const int* d_row_off, const int* d_rev_row, int T, int B, int H,
                                   int ndir, float* d_dg, float* d_dc0, void* d_state,
                                   void* stream) {
  ITTS_REQUIRE(d_dy && d_whh && d_gates && d_csave && d_row_off && d_dg && d_state, "null pointer");
  ITTS_REQUIRE(ndir == 1 || d_rev_row, "the reverse direction needs its row table");
  int rc = rnn_check(h_lengths, T, B, H, ndir);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  RnnPersistBwdArgs p{};
  p.dy = d_dy; p.whh = d_whh; p.c0 = d_c0; p.gates = d_gates; p.aux = d_csave; p.row_off = d_row_off;
  p.rev_row = d_rev_row; p.dg = d_dg; p.d0 = d_dc0; p.T = T; p.B = B; p.ndir = ndir;
  const int done = rnn_persist_backward<4>(p, h_lengths, H, s);
  if (done < 0) return ITTS_E_HIP;
  if (done) return ITTS_OK;
  RnnStepArgs a = step_args(d_rev_row, T, B, H, ndir);
  a.c0 = d_c0; a.gates = const_cast<float*>(d_gates); a.aux = const_cast<float*>(d_csave); a.dy = d_dy;
  a.dg = d_dg;
  return rnn_step_backward<4>(a, d_whh, h_lengths, d_dc0, d_state, s);
}

// The same for one (bi)directional GRU layer: b_hh enters the recurrence (it sits inside r * (W_hn h + b_hn)), there
// is no cell state, and d_gates alone says whether the call saves for backward.
extern "C" int itts_gru_layer_fwd(const float* d_gin, const float* d_whh, const float* d_bhh,
                                  const float* d_h0, const int* d_lengths, const int* h_lengths,
                                  const int* d_row_off, const int* d_rev_row, int T, int B, int H,
                                  int ndir, float* d_y, float* d_gates, float* d_hn, void* d_state,
                                  void* stream) {
  ITTS_REQUIRE(d_gin && d_whh && d_bhh && d_lengths && d_row_off && d_y && d_state, "null pointer");
  ITTS_REQUIRE(ndir == 1 || d_rev_row, "the reverse direction needs its row table");
  int rc = rnn_check(h_lengths, T, B, H, ndir);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  RnnPersistArgs p{};
  p.gin = d_gin; p.whh = d_whh; p.bhh = d_bhh; p.h0 = d_h0; p.lengths = d_lengths; p.row_off = d_row_off;
  p.rev_row = d_rev_row; p.y = d_y; p.gates = d_gates; p.hn = d_hn;
  p.T = T; p.B = B; p.ndir = ndir;
  const int done = rnn_persist_forward<3>(p, H, s);
  if (done < 0) return ITTS_E_HIP;
  if (done) return ITTS_OK;
  RnnStepArgs a = step_args(d_rev_row, T, B, H, ndir);
  a.gin = d_gin; a.bhh = d_bhh; a.y = d_y; a.gates = d_gates;
  return rnn_step_forward<3>(a, d_whh, d_h0, nullptr, d_lengths, h_lengths, d_hn, nullptr, d_state, s);
}

// Backward recurrence of the GRU: fills d_dgi and d_dgh [N, ndir*3H] (gradients wrt gin and wrt the hidden
// projections) from d_dy, the saved gates and d_hprev, the h_{t-1} that entered every step.
extern "C" int itts_gru_layer_bwd(const float* d_dy, const float* d_whh, const float* d_gates,
                                  const float* d_hprev, const int* h_lengths,
                                  const int* d_row_off, const int* d_rev_row, int T, int B, int H,
                                  int ndir, float* d_dgi, float* d_dgh, float* d_dh0, void* d_state,
                                  void* stream) {
  ITTS_REQUIRE(d_dy && d_whh && d_gates && d_hprev && d_row_off && d_dgi && d_dgh && d_state, "null pointer");
  ITTS_REQUIRE(ndir == 1 || d_rev_row, "the reverse direction needs its row table");
  int rc = rnn_check(h_lengths, T, B, H, ndir);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  RnnPersistBwdArgs p{};
  p.dy = d_dy; p.whh = d_whh; p.gates = d_gates; p.aux = d_hprev; p.row_off = d_row_off;
  p.rev_row = d_rev_row; p.dg = d_dgi; p.dg2 = d_dgh; p.d0 = d_dh0; p.T = T; p.B = B; p.ndir = ndir;
  const int done = rnn_persist_backward<3>(p, h_lengths, H, s);
  if (done < 0) return ITTS_E_HIP;
  if (done) return ITTS_OK;
  RnnStepArgs a = step_args(d_rev_row, T, B, H, ndir);
  a.gates = const_cast<float*>(d_gates); a.aux = const_cast<float*>(d_hprev); a.dy = d_dy; a.dg = d_dgi; a.dg2 = d_dgh;
  return rnn_step_backward<3>(a, d_whh, h_lengths, d_dh0, d_state, s);
}

// The same for one (bi)directional vanilla RNN layer, h_t = act(gin_t + W_hh h_{t-1}): one gate, no cell state, and
// nothing saved but d_y -- backward takes act' from it.  Step kernels only.
static std::atomic<int64_t> g_rnn_layer_fwd_calls{0}, g_rnn_layer_bwd_calls{0};

extern "C" int64_t itts_rnn_layer_state_bytes(int B, int H, int ndir) { return rnn_state_bytes(1, B, H, ndir); }

extern "C" int itts_rnn_layer_fwd(const float* d_gin, const float* d_whh, const float* d_h0, const int* d_lengths,
                                  const int* h_lengths, const int* d_row_off, const int* d_rev_row, int T, int B,
                                  int H, int ndir, int act, float* d_y, float* d_hn, void* d_state, void* stream) {
  ITTS_REQUIRE(d_gin && d_whh && d_lengths && d_row_off && d_y && d_state, "null pointer");
  ITTS_REQUIRE(ndir == 1 || d_rev_row, "the reverse direction needs its row table");
  ITTS_REQUIRE(act == ITTS_ACT_TANH || act == ITTS_ACT_RELU, "the activation must be ITTS_ACT_TANH or ITTS_ACT_RELU");
  int rc = rnn_check(h_lengths, T, B, H, ndir);
  if (rc) return rc;
  g_rnn_layer_fwd_calls.fetch_add(1, std::memory_order_relaxed);
  RnnStepArgs a = step_args(d_rev_row, T, B, H, ndir);
  a.gin = d_gin; a.y = d_y; a.act = act;
  return rnn_step_forward<1>(a, d_whh, d_h0, nullptr, d_lengths, h_lengths, d_hn, nullptr, d_state, as_stream(stream));
}

// Backward recurrence: fills d_dg [N, ndir*H] (gradient wrt gin, which is also the one wrt the hidden projection)
// from d_dy and the forward's output d_y.
extern "C" int itts_rnn_layer_bwd(const float* d_dy, const float* d_whh, const float* d_y, const int* h_lengths,
                                  const int* d_row_off, const int* d_rev_row, int T, int B, int H, int ndir, int act,
                                  float* d_dg, void* d_state, void* stream) {
  ITTS_REQUIRE(d_dy && d_whh && d_y && d_row_off && d_dg && d_state, "null pointer");
  ITTS_REQUIRE(ndir == 1 || d_rev_row, "the reverse direction needs its row table");
  ITTS_REQUIRE(act == ITTS_ACT_TANH || act == ITTS_ACT_RELU, "the activation must be ITTS_ACT_TANH or ITTS_ACT_RELU");
  int rc = rnn_check(h_lengths, T, B, H, ndir);
  if (rc) return rc;
  g_rnn_layer_bwd_calls.fetch_add(1, std::memory_order_relaxed);
  RnnStepArgs a = step_args(d_rev_row, T, B, H, ndir);
  a.y = const_cast<float*>(d_y); a.dy = d_dy; a.dg = d_dg; a.act = act;
  return rnn_step_backward<1>(a, d_whh, h_lengths, nullptr, d_state, as_stream(stream));
}

// Forward and backward vanilla RNN layer calls of this process that passed their argument checks.  No device is touched.
extern "C" int itts_rnn_layer_counts(int64_t out[2]) {
  ITTS_REQUIRE(out != nullptr, "null pointer");
  out[0] = g_rnn_layer_fwd_calls.load(std::memory_order_relaxed);
  out[1] = g_rnn_layer_bwd_calls.load(std::memory_order_relaxed);
  return ITTS_OK;
}

// Forward ran / declined / gave_up, backward ran / declined / gave_up of the persistent recurrences (rnn_persist.h),
// LSTM and GRU layer calls of this process together.  No device is touched.
extern "C" int itts_rnn_path_counts(int64_t out[6]) {
  ITTS_REQUIRE(out != nullptr, "null pointer");
  const PersistPathCounts* both[2] = {&g_persist_fwd_counts, &g_persist_bwd_counts};
  for (int i = 0; i < 2; ++i) {
    out[3 * i + 0] = both[i]->ran.load(std::memory_order_relaxed);
    out[3 * i + 1] = both[i]->declined.load(std::memory_order_relaxed);
    out[3 * i + 2] = both[i]->gave_up.load(std::memory_order_relaxed);
  }
  return ITTS_OK;
}
