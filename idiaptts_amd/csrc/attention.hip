// Multi-head self-attention over a padded batch, forward and backward, float32 on the exact-fp32 matrix core
// (v_mfma_f32_32x32x2_f32): what torch.nn.MultiheadAttention computes inside torch.nn.TransformerEncoderLayer
// between its in-projection and its out-projection.  No [T, T] tensor exists in global memory.
//
// Operands (include/idiaptts_amd.h): qkv [rows, 3 D] = q | k | v per row, head h in columns h dh .. of each third;
// row of (b, t) = b stride_b + t stride_t; query t of utterance b attends keys 0 .. klen[b] - 1 for every t < T.
//
// One tile is 32 keys x 32 queries.  A workgroup is four waves; DHP = dh rounded up to 32 is the width everything is
// computed at (columns dh .. DHP - 1 are zeros in registers and LDS, never read from or written to global memory), so
// any head width that keeps 16-byte rows is taken: the multiples of 4 up to 128.  A head of 8 or 48 columns pays for 32
// or 64.
//
// Forward (one workgroup per 128 queries of one (b, h), a wave per 32 of them, key tiles of 32 through LDS):
//   S^T = K Q^T with the KEY on the accumulator's row and the QUERY on the lane: lane l holds query l % 32 and
//   the keys crow(r, l / 32) = (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15.  A query's row maximum and sum are
//   15 in-lane steps and one exchange with lane l ^ 32: no serial walk over lanes.  The running maximum m and sum l
//   of the online softmax are lane scalars.  The accumulator is then ALREADY the B operand of O^T += V^T P^T, with
//   reduction step j pairing the keys crow(j, 0) and crow(j, 1): P never crosses lanes or LDS.
//   Masked keys are skipped: tiles at and beyond klen are not visited, k / v rows at and beyond klen enter LDS as
//   zeros, and inside the last tile such a key's probability is the constant 0.
//   The order of every sum over keys depends on klen and the tile size only.
//
// Backward: P = exp(S scale - lse) is recomputed; delta = rowsum(dO * O) (first launch); with m the keep mask times
// 1 / (1 - p) (1 without dropout): Pd = m P, dP = m (dO V^T), dS = P (dP - delta), and
//   dV = Pd^T dO, dK = scale dS^T Q     second launch: a wave owns 32 keys (K, V and both sums in registers) and
//                                       sweeps the query tiles from LDS; S and dP with the key on the lane, so
//                                       their accumulators are the B operands of dV^T and dK^T
//   dQ = scale dS K                     third launch: the forward's structure, a wave owns 32 queries
// S and dP are computed in both launches: seven products of 2 T klen dh FLOPs where the form that adds dQ across
// workgroups with atomics has five.  That is the price of sums in one fixed order without any workgroup waiting for
// another: gradients are bitwise reproducible.
//
// Dropout (DropRule, dropout.h) on the probabilities: element (row = (b H + h) T + t, col = key).  The forward and
// the dQ launch hold four consecutive keys of one query per lane: one generator call serves four elements.  The
// dK / dV launch holds one key and 16 queries per lane: a call per element, of which one word is used.
#include <math.h>

#include "common.h"
#include "dropout.h"

namespace itts {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int AT_THREADS = 256;   // four waves
constexpr int AT_TILE = 32;       // keys (queries) per tile: one MFMA extent
constexpr int AT_BLOCK = 128;     // queries (keys) per workgroup: a tile per wave
constexpr int AT_MIN_DH = 4, AT_DH_STEP = 4, AT_MAX_DH = 128, AT_MAX_D = 1024, AT_MAX_T = 32768, AT_MAX_BH = 65535;

struct AttnArgs {
  const float* qkv;
  const float* o;
  const float* dout;
  float* out;
  float* dqkv;
  const int32_t* klen;
  float* lse;
  float* delta;
  int B, T, H, dh;
  int64_t sb, st;
  float scale;
};

// row of the accumulator element r in the half hi = lane / 32 of a 32x32 MFMA
__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int clamped_klen(const AttnArgs& a, int b) {
  const int k = a.klen ? a.klen[b] : a.T;
  return min(max(k, 1), a.T);
}

// Rows t0 .. t0 + 31 of one utterance and head into LDS with a pitch of DHP + 1 floats (column reads for an MFMA
// operand then fall on distinct banks); rows at and beyond `limit` and columns at and beyond dh are zeros.
// `base` is the head's first column in row t = 0; pitch = floats between consecutive t.
template <int DHP>
__device__ __forceinline__ void load_tile(float* lds, const float* __restrict__ base, int64_t pitch, int t0, int limit,
                                          int dh) {
  constexpr int S = DHP + 1, C4 = DHP / 4;
#pragma unroll
  for (int i = threadIdx.x; i < AT_TILE * C4; i += AT_THREADS) {
    const int r = i / C4, c = 4 * (i % C4);
    const int t = t0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < limit && c < dh) v = *reinterpret_cast<const float4*>(base + (int64_t)t * pitch + c);
    float* d = lds + r * S + c;
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
}

// B operand of a product whose reduction runs over the head width: element [2 kk + hi] of the lane's row
template <int DHP>
__device__ __forceinline__ void load_row_operand(float (&reg)[DHP / 2], const float* __restrict__ row, bool valid,
                                                 int hi, int dh) {
#pragma unroll
  for (int kk = 0; kk < DHP / 2; ++kk) {
    const int d = 2 * kk + hi;
    reg[kk] = (valid && d < dh) ? row[d] : 0.f;
  }
}

// acc^T [d][lane's row] as float4 stores: element r of block db is column db * 32 + crow(r, hi)
template <int NDB>
__device__ __forceinline__ void store_acc(float* __restrict__ row, const f32x16 (&acc)[NDB], float f, int hi, int dh) {
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = db * 32 + 8 * g + 4 * hi;
      if (d < dh)
        *reinterpret_cast<float4*>(row + d) = make_float4(acc[db][4 * g] * f, acc[db][4 * g + 1] * f,
                                                          acc[db][4 * g + 2] * f, acc[db][4 * g + 3] * f);
    }
  }
}

template <int NDB, class DR>
__global__ __launch_bounds__(AT_THREADS, 2) void attn_fwd_kernel(AttnArgs a, DR dr) {
  constexpr int DHP = 32 * NDB, S = DHP + 1;
  __shared__ float ks[AT_TILE * S];
  __shared__ float vs[AT_TILE * S];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5, ln = lane & 31;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int D = a.H * a.dh;
  const int64_t ld = 3 * (int64_t)D;
  const int klen = clamped_klen(a, b);
  const int tq = blockIdx.x * AT_BLOCK + wave * AT_TILE + ln;    // the lane's query
  const bool qvalid = tq < a.T;
  const float* qb = a.qkv + a.sb * b * ld + h * a.dh;            // q of (b, t = 0, h)
  const int64_t pitch = a.st * ld;

  float qreg[DHP / 2];
  load_row_operand<DHP>(qreg, qb + (int64_t)tq * pitch, qvalid, hi, a.dh);

  f32x16 oacc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int64_t drow = (int64_t)bh * a.T + tq;

  const int ntiles = (klen + AT_TILE - 1) / AT_TILE;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int key0 = kt * AT_TILE;
    __syncthreads();
    load_tile<DHP>(ks, qb + D, pitch, key0, klen, a.dh);
    load_tile<DHP>(vs, qb + 2 * D, pitch, key0, klen, a.dh);
    __syncthreads();

    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < DHP / 2; ++kk) s = mfma(ks[ln * S + 2 * kk + hi], qreg[kk], s);

    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = key0 + crow(r, hi) < klen ? s[r] * a.scale : -INFINITY;
      tmax = fmaxf(tmax, s[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);          // finite: key0 itself is a valid key
    const float alpha = expf(m - mn);         // 0 in the first tile
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = key0 + crow(r, hi) < klen ? expf(s[r] - mn) : 0.f;
      psum += s[r];
    }
    psum += __shfl_xor(psum, 32, 64);
    l = l * alpha + psum;
    m = mn;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;

    if constexpr (DR::on) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint4x w = dr.words(drow, key0 + 8 * g + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[4 * g + e] = dr.apply(s[4 * g + e], w.w[e]);
      }
    }

#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int j = 0; j < 16; ++j) oacc[db] = mfma(vs[crow(j, hi) * S + db * 32 + ln], s[j], oacc[db]);
  }

  if (!qvalid) return;
  store_acc<NDB>(a.out + (a.sb * b + a.st * tq) * D + h * a.dh, oacc, 1.f / l, hi, a.dh);
  if (hi == 0) a.lse[(int64_t)bh * a.T + tq] = m + logf(l);
}

// delta[b, h, t] = sum_d do * o, one thread per (b, t, h), columns in ascending order
__global__ __launch_bounds__(AT_THREADS) void attn_delta_kernel(AttnArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
  if (idx >= (int64_t)a.B * a.T * a.H) return;
  const int h = (int)(idx % a.H);
  const int64_t bt = idx / a.H;
  const int t = (int)(bt % a.T), b = (int)(bt / a.T);
  const int64_t off = (a.sb * b + a.st * t) * ((int64_t)a.H * a.dh) + h * a.dh;
  const float4* x = reinterpret_cast<const float4*>(a.dout + off);
  const float4* y = reinterpret_cast<const float4*>(a.o + off);
  float sum = 0.f;
  for (int c = 0; c < a.dh / 4; ++c) {
    const float4 u = x[c], v = y[c];
    sum += u.x * v.x;
    sum += u.y * v.y;
    sum += u.z * v.z;
    sum += u.w * v.w;
  }
  a.delta[((int64_t)b * a.H + h) * a.T + t] = sum;
}

template <int NDB, class DR>
__global__ __launch_bounds__(AT_THREADS, 1) void attn_bwd_dkv_kernel(AttnArgs a, DR dr) {
  constexpr int DHP = 32 * NDB, S = DHP + 1;
  __shared__ float qs[AT_TILE * S];
  __shared__ float dos[AT_TILE * S];
  __shared__ float lse_s[AT_TILE];
  __shared__ float del_s[AT_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5, ln = lane & 31;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int D = a.H * a.dh;
  const int64_t ld = 3 * (int64_t)D;
  const int klen = clamped_klen(a, b);
  const int tk = blockIdx.x * AT_BLOCK + wave * AT_TILE + ln;    // the lane's key
  float* dkrow = a.dqkv + (a.sb * b + a.st * tk) * ld + D + h * a.dh;

  f32x16 dk[NDB], dv[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[db][r] = dv[db][r] = 0.f;

  if (blockIdx.x * AT_BLOCK < klen) {      // (uniform over the workgroup) else: masked keys only, zeros
    const float* qb = a.qkv + a.sb * b * ld + h * a.dh;
    const float* dob = a.dout + a.sb * b * D + h * a.dh;
    const int64_t pitch = a.st * ld, dpitch = a.st * (int64_t)D;
    const bool kvalid = tk < klen;
    const bool wave_on = blockIdx.x * AT_BLOCK + wave * AT_TILE < klen;   // (uniform over the wave)
    float kreg[DHP / 2], vreg[DHP / 2];
    load_row_operand<DHP>(kreg, qb + D + (int64_t)tk * pitch, kvalid, hi, a.dh);
    load_row_operand<DHP>(vreg, qb + 2 * D + (int64_t)tk * pitch, kvalid, hi, a.dh);

    const int nq = (a.T + AT_TILE - 1) / AT_TILE;
    for (int qt = 0; qt < nq; ++qt) {
      const int q0 = qt * AT_TILE;
      __syncthreads();
      load_tile<DHP>(qs, qb, pitch, q0, a.T, a.dh);
      load_tile<DHP>(dos, dob, dpitch, q0, a.T, a.dh);
      if (threadIdx.x < AT_TILE) {
        const int t = q0 + threadIdx.x;
        lse_s[threadIdx.x] = t < a.T ? a.lse[(int64_t)bh * a.T + t] : INFINITY;   // p = 0 for a query beyond T
        del_s[threadIdx.x] = t < a.T ? a.delta[(int64_t)bh * a.T + t] : 0.f;
      }
      __syncthreads();
      if (!wave_on) continue;

      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < DHP / 2; ++kk) {
        s = mfma(qs[ln * S + 2 * kk + hi], kreg[kk], s);
        dp = mfma(dos[ln * S + 2 * kk + hi], vreg[kk], dp);
      }
      // s[r], dp[r]: query q0 + crow(r, hi), key tk.  Afterwards s = dS and dp = Pd.
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = crow(r, hi);
        const float p = kvalid ? expf(s[r] * a.scale - lse_s[q]) : 0.f;
        float pd = p, dpv = dp[r];
        if constexpr (DR::on) {
          const uint4x w = dr.words((int64_t)bh * a.T + q0 + q, tk);
          const uint32_t e = (uint32_t)tk & 3u;
          const uint32_t word = e == 0 ? w.w[0] : e == 1 ? w.w[1] : e == 2 ? w.w[2] : w.w[3];
          pd = dr.apply(p, word);
          dpv = dr.apply(dpv, word);
        }
        s[r] = p * (dpv - del_s[q]);
        dp[r] = pd;
      }
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          dv[db] = mfma(dos[crow(j, hi) * S + db * 32 + ln], dp[j], dv[db]);
          dk[db] = mfma(qs[crow(j, hi) * S + db * 32 + ln], s[j], dk[db]);
        }
    }
  }

  if (tk >= a.T) return;
  store_acc<NDB>(dkrow, dk, a.scale, hi, a.dh);
  store_acc<NDB>(dkrow + D, dv, 1.f, hi, a.dh);
}

template <int NDB, class DR>
__global__ __launch_bounds__(AT_THREADS, NDB == 4 ? 1 : 2) void attn_bwd_dq_kernel(AttnArgs a, DR dr) {
  constexpr int DHP = 32 * NDB, S = DHP + 1;
  __shared__ float ks[AT_TILE * S];
  __shared__ float vs[AT_TILE * S];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5, ln = lane & 31;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int D = a.H * a.dh;
  const int64_t ld = 3 * (int64_t)D;
  const int klen = clamped_klen(a, b);
  const int tq = blockIdx.x * AT_BLOCK + wave * AT_TILE + ln;
  const bool qvalid = tq < a.T;
  const float* qb = a.qkv + a.sb * b * ld + h * a.dh;
  const int64_t pitch = a.st * ld;

  float qreg[DHP / 2], doreg[DHP / 2];
  load_row_operand<DHP>(qreg, qb + (int64_t)tq * pitch, qvalid, hi, a.dh);
  load_row_operand<DHP>(doreg, a.dout + (a.sb * b + a.st * tq) * D + h * a.dh, qvalid, hi, a.dh);
  const int64_t drow = (int64_t)bh * a.T + tq;
  const float lse = qvalid ? a.lse[drow] : 0.f;
  const float delta = qvalid ? a.delta[drow] : 0.f;

  f32x16 dq[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[db][r] = 0.f;

  const int ntiles = (klen + AT_TILE - 1) / AT_TILE;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int key0 = kt * AT_TILE;
    __syncthreads();
    load_tile<DHP>(ks, qb + D, pitch, key0, klen, a.dh);
    load_tile<DHP>(vs, qb + 2 * D, pitch, key0, klen, a.dh);
    __syncthreads();

    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < DHP / 2; ++kk) {
      s = mfma(ks[ln * S + 2 * kk + hi], qreg[kk], s);
      dp = mfma(vs[ln * S + 2 * kk + hi], doreg[kk], dp);
    }
    if constexpr (DR::on) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint4x w = dr.words(drow, key0 + 8 * g + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) dp[4 * g + e] = dr.apply(dp[4 * g + e], w.w[e]);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = key0 + crow(r, hi) < klen ? expf(s[r] * a.scale - lse) : 0.f;
      s[r] = p * (dp[r] - delta);
    }
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int j = 0; j < 16; ++j) dq[db] = mfma(ks[crow(j, hi) * S + db * 32 + ln], s[j], dq[db]);
  }

  if (!qvalid) return;
  store_acc<NDB>(a.dqkv + (a.sb * b + a.st * tq) * ld + h * a.dh, dq, a.scale, hi, a.dh);
}

#define AT_LAUNCH(kernel, grid, s, a, dr)                                         \
  do {                                                                            \
    switch (((a).dh + 31) / 32) {                                                 \
      case 1: kernel<1><<<grid, AT_THREADS, 0, s>>>(a, dr); break;                \
      case 2: kernel<2><<<grid, AT_THREADS, 0, s>>>(a, dr); break;                \
      case 3: kernel<3><<<grid, AT_THREADS, 0, s>>>(a, dr); break;                \
      default: kernel<4><<<grid, AT_THREADS, 0, s>>>(a, dr); break;               \
    }                                                                             \
  } while (0)

// the envelope of both entry points, checked before any device work
int attn_check(const char* entry, int B, int T, int H, int dh, int64_t sb, int64_t st, double p) {
  ITTS_REQUIRE_AS(entry, dh >= AT_MIN_DH && dh <= AT_MAX_DH && dh % AT_DH_STEP == 0,
                  "head width dh = " + std::to_string(dh) + " is not a multiple of 4 in 4 .. 128");
  ITTS_REQUIRE_AS(entry, H >= 1, "H = " + std::to_string(H) + " heads");
  ITTS_REQUIRE_AS(entry, (int64_t)H * dh <= AT_MAX_D,
                  "model width D = " + std::to_string((int64_t)H * dh) + " is beyond " + std::to_string(AT_MAX_D));
  ITTS_REQUIRE_AS(entry, B >= 0, "B = " + std::to_string(B));
  ITTS_REQUIRE_AS(entry, T >= 1 && T <= AT_MAX_T, "T = " + std::to_string(T) + " is outside 1 .. " +
                                                      std::to_string(AT_MAX_T));
  ITTS_REQUIRE_AS(entry, (int64_t)B * H <= AT_MAX_BH,
                  "B * H = " + std::to_string((int64_t)B * H) + " is beyond " + std::to_string(AT_MAX_BH));
  ITTS_REQUIRE_AS(entry, sb >= 1 && st >= 1, "row strides " + std::to_string(sb) + ", " + std::to_string(st));
  ITTS_REQUIRE_AS(entry, p >= 0.0 && p < 1.0, "dropout p must be in [0, 1)");
  return ITTS_OK;
}

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int64_t itts_attention_workspace_bytes(int B, int H, int T) {
  if (B <= 0 || H <= 0 || T <= 0) return 0;
  return (int64_t)B * H * T * (int64_t)sizeof(float);
}

extern "C" int itts_attention_fwd(const float* d_qkv, float* d_o, const int32_t* d_klen, float* d_lse, int B, int T,
                                  int H, int dh, int64_t stride_b, int64_t stride_t, double p, uint64_t seed,
                                  uint32_t salt, void* stream) {
  if (int e = attn_check(__func__, B, T, H, dh, stride_b, stride_t, p)) return e;
  if (B == 0) return ITTS_OK;
  ITTS_REQUIRE(d_qkv && d_o && d_lse, "null pointer");
  ITTS_REQUIRE(aligned16(d_qkv) && aligned16(d_o), "qkv and o must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  AttnArgs a{};
  a.qkv = d_qkv; a.out = d_o; a.klen = d_klen; a.lse = d_lse;
  a.B = B; a.T = T; a.H = H; a.dh = dh; a.sb = stride_b; a.st = stride_t;
  a.scale = (float)(1.0 / sqrt((double)dh));
  const dim3 grid((unsigned)((T + AT_BLOCK - 1) / AT_BLOCK), (unsigned)(B * H));
  if (p > 0.0) {
    const DropRule dr = make_drop_rule(p, seed, salt, 0);
    AT_LAUNCH(attn_fwd_kernel, grid, s, a, dr);
  } else {
    AT_LAUNCH(attn_fwd_kernel, grid, s, a, NoDrop{});
  }
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_attention_bwd(const float* d_do, const float* d_qkv, const float* d_o, const int32_t* d_klen,
                                  const float* d_lse, float* d_dqkv, int B, int T, int H, int dh, int64_t stride_b,
                                  int64_t stride_t, double p, uint64_t seed, uint32_t salt, void* stream) {
  if (int e = attn_check(__func__, B, T, H, dh, stride_b, stride_t, p)) return e;
  if (B == 0) return ITTS_OK;
  ITTS_REQUIRE(d_do && d_qkv && d_o && d_lse && d_dqkv, "null pointer");
  ITTS_REQUIRE(aligned16(d_do) && aligned16(d_qkv) && aligned16(d_o) && aligned16(d_dqkv),
               "do, qkv, o and dqkv must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  AttnArgs a{};
  a.qkv = d_qkv; a.o = d_o; a.dout = d_do; a.dqkv = d_dqkv; a.klen = d_klen; a.lse = const_cast<float*>(d_lse);
  a.B = B; a.T = T; a.H = H; a.dh = dh; a.sb = stride_b; a.st = stride_t;
  a.scale = (float)(1.0 / sqrt((double)dh));
  const int64_t n = (int64_t)B * H * T;
  ITTS_HIP_CHECK(scratch.take(&a.delta, (size_t)n));
  attn_delta_kernel<<<dim3((unsigned)((n + AT_THREADS - 1) / AT_THREADS)), AT_THREADS, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  const dim3 grid((unsigned)((T + AT_BLOCK - 1) / AT_BLOCK), (unsigned)(B * H));
  if (p > 0.0) {
    const DropRule dr = make_drop_rule(p, seed, salt, 0);
    AT_LAUNCH(attn_bwd_dkv_kernel, grid, s, a, dr);
    ITTS_LAUNCH_CHECK();
    AT_LAUNCH(attn_bwd_dq_kernel, grid, s, a, dr);
  } else {
    AT_LAUNCH(attn_bwd_dkv_kernel, grid, s, a, NoDrop{});
    ITTS_LAUNCH_CHECK();
    AT_LAUNCH(attn_bwd_dq_kernel, grid, s, a, NoDrop{});
  }
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
