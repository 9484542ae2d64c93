// One time step of an LSTM, GRU or tanh / ReLU RNN layer direction for B rows that each carry a state of their own:
// the step of an autoregressive decoder, which feeds a frame, reads the output and comes back with the states the
// rows were left in.  (The layer entry points of rnn.hip start every row from one shared state.)  The two products
// gi = x W_ih^T + bias and gh = h W_hh^T come from the dense GEMM; this kernel is the cell: one thread per (row,
// hidden unit), the arithmetic of rnn_common.h, any hidden size.  All float32; reads (2 G + 1 or 2) B H floats,
// writes B H (2 B H for the LSTM).
#include "rnn_common.h"

namespace itts {
namespace {

struct CellArgs {
  const float* gi; int64_t ldgi;        // [B, G*H]: LSTM / RNN with b_ih + b_hh, GRU with b_ih
  const float* gh; int64_t ldgh;        // [B, G*H]: no bias
  const float* b_hh;                    // GRU: [3H]
  const float* h; int64_t ldh;          // [B, H]
  const float* c; int64_t ldc;          // LSTM: [B, H]
  float* h_out; int64_t ldho;
  float* c_out; int64_t ldco;
  int64_t n;                            // B * H
  int H, kind, act;
};

__global__ __launch_bounds__(256) void rnn_cell_step_kernel(CellArgs a) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / a.H;
    const int j = (int)(i - b * a.H);
    const float* gi = a.gi + b * a.ldgi + j;
    const float* gh = a.gh + b * a.ldgh + j;
    const size_t H = (size_t)a.H;
    float h = a.h[b * a.ldh + j];
    if (a.kind == ITTS_CELL_LSTM) {
      float c = a.c[b * a.ldc + j], ig, fg, gg, og;
      lstm_cell_fwd(gh[0], gh[H], gh[2 * H], gh[3 * H], gi[0], gi[H], gi[2 * H], gi[3 * H], c, h, ig, fg, gg, og);
      a.c_out[b * a.ldco + j] = c;
    } else if (a.kind == ITTS_CELL_GRU) {
      float rg, zg, ng, hnp;
      gru_cell_fwd(gh[0], gh[H], gh[2 * H], gi[0], gi[H], gi[2 * H], a.b_hh[j], a.b_hh[H + j], a.b_hh[2 * H + j], h,
                   rg, zg, ng, hnp);
    } else {
      h = rnn_cell_fwd(gh[0], gi[0], a.act);
    }
    a.h_out[b * a.ldho + j] = h;
  }
}

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int itts_rnn_cell_step(int kind, int act, const float* d_gi, int64_t ldgi, const float* d_gh, int64_t ldgh,
                                  const float* d_b_hh, const float* d_h, int64_t ldh, const float* d_c, int64_t ldc,
                                  int B, int H, float* d_h_out, int64_t ldho, float* d_c_out, int64_t ldco,
                                  void* stream) {
  ITTS_REQUIRE(kind == ITTS_CELL_LSTM || kind == ITTS_CELL_GRU || kind == ITTS_CELL_RNN,
               "unknown cell kind = " + std::to_string(kind));
  ITTS_REQUIRE(kind != ITTS_CELL_RNN || act == ITTS_ACT_TANH || act == ITTS_ACT_RELU,
               "RNN activation = " + std::to_string(act) + " is neither tanh nor ReLU");
  ITTS_REQUIRE(B >= 0, "B = " + std::to_string(B) + " is negative");
  ITTS_REQUIRE(H >= 1, "H = " + std::to_string(H) + " is not positive");
  const int64_t G = kind == ITTS_CELL_LSTM ? 4 : (kind == ITTS_CELL_GRU ? 3 : 1);
  ITTS_REQUIRE(ldgi >= G * H, "pitch ldgi = " + std::to_string(ldgi) + " is below " + std::to_string(G * H));
  ITTS_REQUIRE(ldgh >= G * H, "pitch ldgh = " + std::to_string(ldgh) + " is below " + std::to_string(G * H));
  ITTS_REQUIRE(ldh >= H && ldho >= H, "pitch ldh / ldho is below H = " + std::to_string(H));
  ITTS_REQUIRE(kind != ITTS_CELL_LSTM || (ldc >= H && ldco >= H), "pitch ldc / ldco is below H = " + std::to_string(H));
  if (B == 0) return ITTS_OK;
  ITTS_REQUIRE(d_gi && d_gh && d_h && d_h_out, "null pointer (d_gi / d_gh / d_h / d_h_out)");
  ITTS_REQUIRE(kind != ITTS_CELL_LSTM || (d_c && d_c_out), "null pointer (d_c / d_c_out): the LSTM carries a cell state");
  ITTS_REQUIRE(kind != ITTS_CELL_GRU || d_b_hh, "null pointer (d_b_hh): the GRU's b_hh sits inside its reset gate");
  CellArgs a{};
  a.gi = d_gi; a.ldgi = ldgi; a.gh = d_gh; a.ldgh = ldgh; a.b_hh = d_b_hh; a.h = d_h; a.ldh = ldh; a.c = d_c;
  a.ldc = ldc; a.h_out = d_h_out; a.ldho = ldho; a.c_out = d_c_out; a.ldco = ldco;
  a.n = (int64_t)B * H; a.H = H; a.kind = kind; a.act = act;
  rnn_cell_step_kernel<<<rnn_ew_grid(a.n), 256, 0, as_stream(stream)>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
