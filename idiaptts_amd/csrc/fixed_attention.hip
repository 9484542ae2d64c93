// Fixed (duration-derived) attention of the encoder-decoder model (enc_dec_dyn/attention/FixedAttention.py of the
// reference): the attention matrix A [B, T, P] of an utterance's phoneme durations is averaged over chunks of
// n = n_frames_per_step frames, Abar [B, K, P], and the context of chunk k is Abar[b, k, :] x enc[b] [P, C].  A hard
// matrix has one non-zero per row of A and at most n per row of Abar, so the product is a gather: the kernels walk
// each row's (column's) non-zeros and never multiply by a zero.  All float32, all bandwidth-bound.
//
// Forward.  One wave per chunk (b, k), four chunks per workgroup.
//   * Abar: a lane owns the four adjacent phonemes 256 j + 4 lane .. + 3 of every tile j of 256 (one 16-byte load
//     where pitch and base allow, four plain loads otherwise: the same phonemes in the same lane either way); the
//     chunk's rows are added in ascending frame order starting from zero and divided by the row count.
//   * The non-zeros of the row are compacted into (p, w) pairs in LDS, p ascending: the position of a lane's pair is
//     what four ballots say lies in front of it.  The count is wave-uniform.
//   * ctx: a lane owns four adjacent channels of every tile of 256; it walks the pairs in order, the first product
//     as w * enc, every further one as fma(w, enc, acc).  A row without non-zeros (a padded frame) gives zeros.
//   A soft (dense) matrix takes the same loop with P pairs.  Skipping a zero weight differs from bmm only where enc
//   holds Inf or NaN in a row of weight zero (0 * Inf = NaN there, nothing here).
//
// Backward.  d_enc[b, p, :] = sum over k ascending of Abar[b, k, p] * dctx[b, k, :], zeros skipped as above.  One wave
// per (b, four adjacent phonemes, tile of 256 channels): it reads its four columns of Abar 64 chunks at a time (lane =
// chunk), and for each phoneme walks the set bits of the ballot of non-zeros in ascending order, broadcasting
// (k, w) from the owning lane.  Every position of d_enc is written, no atomics, one order: an utterance's result
// depends on its own rows only -- not on B, not on its index in the batch, not on the access width.
#include <algorithm>

#include "common.h"
#include "row4.h"

namespace itts {
namespace {

constexpr int FA_WAVES = 4;
constexpr int FA_THREADS = FA_WAVES * kWave;
constexpr int FA_TILE = 4 * kWave;          // phonemes / channels a wave covers per tile (four per lane)
constexpr int FA_MAX_P = 2048;
constexpr int FA_MAX_C = 4096;
constexpr int FA_MAX_N = 64;

// .. of a batch: the utterances' rows too
bool rows16(const float* p, int64_t ld, int64_t utt) { return utt % 4 == 0 && itts::rows16(p, ld); }

struct FaArgs {
  const float* A; int64_t ldA, uttA;        // [B, T, P]: floats from one frame to the next / one utterance to the next
  const float* enc; int64_t ldE, uttE;      // [B, P, C]
  float* abar; int64_t ldM, uttM;           // [B, K, P]
  float* ctx; int64_t ldX, uttX;            // [B, K, C]
  int64_t T, K;
  int P, C, n, kgroups;                     // kgroups = ceil(K / FA_WAVES)
};

template <bool VEC_P, bool VEC_C>
__global__ __launch_bounds__(FA_THREADS) void fixed_attention_fwd_kernel(FaArgs a) {
  extern __shared__ int2 fa_pairs[];        // [FA_WAVES][P]: (p, bits of w)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x / a.kgroups;
  const int64_t k = (int64_t)(blockIdx.x % a.kgroups) * FA_WAVES + wave;
  const bool live = k < a.K;
  int2* pairs = fa_pairs + (size_t)wave * a.P;
  const int64_t t0 = k * a.n;
  const int rows = live ? (int)min((int64_t)a.n, a.T - t0) : 0;
  const uint64_t below = (1ull << lane) - 1ull;
  int count = 0;
  if (live) {
    const float* Ab = a.A + b * a.uttA + t0 * a.ldA;
    float* Mb = a.abar + b * a.uttM + k * a.ldM;
    for (int p0 = 0; p0 < a.P; p0 += FA_TILE) {
      const int p = p0 + 4 * lane;
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < rows; ++r) {
        float v[4];
        load4z<VEC_P>(Ab + r * a.ldA, p, a.P, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += v[q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] = s[q] / (float)rows;
      store4<VEC_P>(Mb, p, a.P, s);
      // pairs of the tile in ascending p = (lane, q) order: those of lower lanes, then the lane's own earlier ones
      uint64_t nz[4];
      int before = 0, total = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        nz[q] = __ballot(p + q < a.P && s[q] != 0.f);
        before += __popcll(nz[q] & below);
        total += __popcll(nz[q]);
      }
      int at = count + before;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((nz[q] >> lane) & 1ull) pairs[at++] = make_int2(p + q, __float_as_int(s[q]));
      count += total;
    }
  }
  __syncthreads();                          // the pairs are read by other lanes than wrote them
  if (!live) return;
  const float* Eb = a.enc + b * a.uttE;
  float* Xb = a.ctx + b * a.uttX + k * a.ldX;
  for (int c0 = 0; c0 < a.C; c0 += FA_TILE) {
    const int col = c0 + 4 * lane;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < count; ++e) {
      const int2 pw = pairs[e];
      const float w = __int_as_float(pw.y);
      float v[4];
      load4z<VEC_C>(Eb + (int64_t)pw.x * a.ldE, col, a.C, v);
      if (e == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = w * v[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fmaf(w, v[q], acc[q]);
      }
    }
    store4<VEC_C>(Xb, col, a.C, acc);
  }
}

struct FaBwdArgs {
  const float* abar; int64_t ldM, uttM;     // [B, K, P]
  const float* dctx; int64_t ldX, uttX;     // [B, K, C]
  float* denc; int64_t ldE, uttE;           // [B, P, C]
  int64_t K;
  int P, C, pgroups;                        // pgroups = ceil(P / (4 * FA_WAVES))
};

template <bool VEC_P, bool VEC_C>
__global__ __launch_bounds__(FA_THREADS) void fixed_attention_bwd_kernel(FaBwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x / a.pgroups;
  const int p = ((int)(blockIdx.x % a.pgroups) * FA_WAVES + wave) * 4;
  if (p >= a.P) return;                     // (no barrier in this kernel)
  const int col = blockIdx.y * FA_TILE + 4 * lane;
  const float* Mb = a.abar + b * a.uttM;
  const float* Xb = a.dctx + b * a.uttX;
  float acc[4][4];
  bool first[4] = {true, true, true, true};
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q][0] = acc[q][1] = acc[q][2] = acc[q][3] = 0.f;
  for (int64_t k0 = 0; k0 < a.K; k0 += kWave) {
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    if (k0 + lane < a.K) load4<VEC_P>(Mb + (k0 + lane) * a.ldM, p, a.P, w);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint64_t nz = __ballot(w[q] != 0.f);
      while (nz) {
        const int src = __ffsll((unsigned long long)nz) - 1;
        nz &= nz - 1ull;
        const float wk = __shfl(w[q], src, 64);
        float v[4];
        load4z<VEC_C>(Xb + (k0 + src) * a.ldX, col, a.C, v);
        if (first[q]) {
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[q][c] = wk * v[c];
          first[q] = false;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[q][c] = fmaf(wk, v[c], acc[q][c]);
        }
      }
    }
  }
  float* Eb = a.denc + b * a.uttE;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (p + q < a.P) store4<VEC_C>(Eb + (int64_t)(p + q) * a.ldE, col, a.C, acc[q]);
}

int64_t chunks(int64_t T, int n, int partial) { return partial ? (T + n - 1) / n : T / n; }

}  // namespace
}  // namespace itts

using namespace itts;

#define FA_CHECK_SIZES()                                                                                        \
  ITTS_REQUIRE(B >= 0, "B = " + std::to_string(B) + " is negative");                                            \
  ITTS_REQUIRE(P >= 1 && P <= FA_MAX_P, "P = " + std::to_string(P) + " is outside 1 .. " + std::to_string(FA_MAX_P)); \
  ITTS_REQUIRE(C >= 1 && C <= FA_MAX_C, "C = " + std::to_string(C) + " is outside 1 .. " + std::to_string(FA_MAX_C))
#define FA_CHECK_PITCH(ld, utt, width, rows)                                                                    \
  ITTS_REQUIRE(ld >= (width), "pitch " #ld " = " + std::to_string(ld) + " is below the width " + std::to_string(width)); \
  ITTS_REQUIRE(B <= 1 || utt >= (int64_t)(rows) * ld || (rows) == 0,                                             \
               "utterance step " #utt " = " + std::to_string(utt) + " is below rows * pitch")

extern "C" int itts_fixed_attention_plan(int B, int64_t T, int P, int C, int n, int partial_last, int64_t* K,
                                         int* fwd_blocks, int* fwd_lds_bytes, int* bwd_blocks_x, int* bwd_blocks_y,
                                         int* vec_p, int* vec_c) {
  if (B < 0 || T < 0 || P < 1 || P > FA_MAX_P || C < 1 || C > FA_MAX_C || n < 1 || n > FA_MAX_N) return -1;
  if (!partial_last && T % n != 0) return -1;
  const int64_t k = chunks(T, n, partial_last);
  const int64_t fb = (int64_t)B * ((k + FA_WAVES - 1) / FA_WAVES);
  const int64_t bb = (int64_t)B * ((P + 4 * FA_WAVES - 1) / (4 * FA_WAVES));
  if (fb > 0x7fffffff || bb > 0x7fffffff) return -1;
  if (K) *K = k;
  if (fwd_blocks) *fwd_blocks = (int)fb;
  if (fwd_lds_bytes) *fwd_lds_bytes = FA_WAVES * P * (int)sizeof(int2);
  if (bwd_blocks_x) *bwd_blocks_x = (int)bb;
  if (bwd_blocks_y) *bwd_blocks_y = (C + FA_TILE - 1) / FA_TILE;
  if (vec_p) *vec_p = P % 4 == 0 ? 1 : 0;       // for dense tensors on 16-byte bases; a call decides from its pointers
  if (vec_c) *vec_c = C % 4 == 0 ? 1 : 0;
  return 0;
}

extern "C" int itts_fixed_attention_fwd(const float* d_A, int64_t ldA, int64_t uttA, const float* d_enc, int64_t ldE,
                                        int64_t uttE, int B, int64_t T, int P, int C, int n, int partial_last,
                                        float* d_abar, int64_t ldM, int64_t uttM, float* d_ctx, int64_t ldX,
                                        int64_t uttX, void* stream) {
  FA_CHECK_SIZES();
  ITTS_REQUIRE(n >= 1 && n <= FA_MAX_N,
               "n_frames_per_step = " + std::to_string(n) + " is outside 1 .. " + std::to_string(FA_MAX_N));
  ITTS_REQUIRE(T >= 0, "T = " + std::to_string(T) + " is negative");
  ITTS_REQUIRE(partial_last || T % n == 0, "T = " + std::to_string(T) + " is not a multiple of n_frames_per_step = " +
                                               std::to_string(n) + " and partial_last is not set");
  const int64_t K = chunks(T, n, partial_last);
  FA_CHECK_PITCH(ldA, uttA, P, T);
  FA_CHECK_PITCH(ldE, uttE, C, P);
  FA_CHECK_PITCH(ldM, uttM, P, K);
  FA_CHECK_PITCH(ldX, uttX, C, K);
  if (B == 0 || K == 0) return ITTS_OK;
  ITTS_REQUIRE(d_A && d_enc && d_abar && d_ctx, "null pointer (d_A / d_enc / d_abar / d_ctx)");
  FaArgs a{};
  a.A = d_A; a.ldA = ldA; a.uttA = uttA; a.enc = d_enc; a.ldE = ldE; a.uttE = uttE;
  a.abar = d_abar; a.ldM = ldM; a.uttM = uttM; a.ctx = d_ctx; a.ldX = ldX; a.uttX = uttX;
  a.T = T; a.K = K; a.P = P; a.C = C; a.n = n;
  a.kgroups = (int)((K + FA_WAVES - 1) / FA_WAVES);
  const int64_t blocks = (int64_t)B * a.kgroups;
  ITTS_REQUIRE(blocks <= 0x7fffffff, "B * chunks = " + std::to_string(blocks) + " workgroups is too large");
  const bool vp = rows16(d_A, ldA, uttA) && rows16(d_abar, ldM, uttM);
  const bool vc = rows16(d_enc, ldE, uttE) && rows16(d_ctx, ldX, uttX);
  const size_t lds = (size_t)FA_WAVES * P * sizeof(int2);
  const dim3 grid((unsigned)blocks);
  hipStream_t s = as_stream(stream);
  if (vp && vc) fixed_attention_fwd_kernel<true, true><<<grid, FA_THREADS, lds, s>>>(a);
  else if (vp) fixed_attention_fwd_kernel<true, false><<<grid, FA_THREADS, lds, s>>>(a);
  else if (vc) fixed_attention_fwd_kernel<false, true><<<grid, FA_THREADS, lds, s>>>(a);
  else fixed_attention_fwd_kernel<false, false><<<grid, FA_THREADS, lds, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_fixed_attention_bwd(const float* d_abar, int64_t ldM, int64_t uttM, const float* d_dctx,
                                        int64_t ldX, int64_t uttX, int B, int64_t K, int P, int C, float* d_denc,
                                        int64_t ldE, int64_t uttE, void* stream) {
  FA_CHECK_SIZES();
  ITTS_REQUIRE(K >= 0, "K = " + std::to_string(K) + " is negative");
  FA_CHECK_PITCH(ldM, uttM, P, K);
  FA_CHECK_PITCH(ldX, uttX, C, K);
  FA_CHECK_PITCH(ldE, uttE, C, P);
  if (B == 0) return ITTS_OK;
  ITTS_REQUIRE(d_denc && (K == 0 || (d_abar && d_dctx)), "null pointer (d_abar / d_dctx / d_denc)");
  FaBwdArgs a{};
  a.abar = d_abar; a.ldM = ldM; a.uttM = uttM; a.dctx = d_dctx; a.ldX = ldX; a.uttX = uttX;
  a.denc = d_denc; a.ldE = ldE; a.uttE = uttE; a.K = K; a.P = P; a.C = C;
  a.pgroups = (P + 4 * FA_WAVES - 1) / (4 * FA_WAVES);
  const int64_t blocks = (int64_t)B * a.pgroups;
  ITTS_REQUIRE(blocks <= 0x7fffffff, "B * phoneme groups = " + std::to_string(blocks) + " workgroups is too large");
  const bool vp = K == 0 || rows16(d_abar, ldM, uttM);
  const bool vc = (K == 0 || rows16(d_dctx, ldX, uttX)) && rows16(d_denc, ldE, uttE);
  const dim3 grid((unsigned)blocks, (unsigned)((C + FA_TILE - 1) / FA_TILE));
  hipStream_t s = as_stream(stream);
  if (vp && vc) fixed_attention_bwd_kernel<true, true><<<grid, FA_THREADS, 0, s>>>(a);
  else if (vp) fixed_attention_bwd_kernel<true, false><<<grid, FA_THREADS, 0, s>>>(a);
  else if (vc) fixed_attention_bwd_kernel<false, true><<<grid, FA_THREADS, 0, s>>>(a);
  else fixed_attention_bwd_kernel<false, false><<<grid, FA_THREADS, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
