// Utterance-level latents: pooling a padded batch over time, the VAE reparameterisation and its KL term
// (rnn_dyn/Pooling.py, rnn_dyn/VAE.py, loss/VAEKLDLoss.py of the reference).  All float32, all bandwidth-bound.
//
// Pooling, mode MEAN.  The sum of an utterance's t_max rows has ONE order, whatever the launch looks like: time is
// cut into segments of PL_SEG = 128 rows; inside a segment wave w of four sums the rows w, w + 4, ... in ascending
// order, the four wave sums are added as ((s0 + s1) + s2) + s3, and the segment sums are added in ascending
// order, starting from zero.  A lane owns four adjacent columns (one 16-byte load where pitch and base allow, four
// plain loads otherwise: the same columns in the same lane either way).  So y[b] depends on the utterance's rows,
// t_max and nothing else -- not on its batch index, not on n_utts, not on the alignment.
// What n_utts decides is only who adds the segment sums: with enough (utterance, column tile) pairs to fill the
// 256 CUs one workgroup walks all segments of its pair and keeps the total in a register; with few pairs (batches
// of 1 .. 64 utterances) every segment gets a workgroup of its own, writes its sum into the workspace
// [n_utts][segments][width] (1 / 128 of the input's bytes) and a second launch adds them in the same order.
// itts_time_pool_plan reports which of the two a call takes.
//
// No atomics anywhere in this file: repeated calls give identical bits.
#include <algorithm>

#include "common.h"
#include "row4.h"

namespace itts {
namespace {

constexpr int PL_SEG = 128;            // rows of a segment
constexpr int PL_WAVES = 4;
constexpr int PL_THREADS = PL_WAVES * kWave;
constexpr int PL_TILE = 4 * kWave;     // columns of a workgroup's tile (four per lane)
constexpr int64_t PL_FILL = 512;       // (utterance, tile) pairs from which one workgroup per pair fills the GPU
constexpr int64_t PL_MAX_SEGMENTS = 65535;

struct PoolPlan {
  int tiles;         // column tiles of PL_TILE
  int segments;      // time segments of PL_SEG
  bool split;        // one workgroup per segment + the second stage
};

PoolPlan pool_plan(int n_utts, int64_t t_max, int width) {
  PoolPlan p;
  p.tiles = (width + PL_TILE - 1) / PL_TILE;
  p.segments = (int)((t_max + PL_SEG - 1) / PL_SEG);
  p.split = p.segments > 1 && (int64_t)n_utts * p.tiles < PL_FILL;
  return p;
}

struct PoolArgs {
  const float* x; int64_t ldx;
  const int64_t* lens;
  float* y; int64_t ldy;
  float* part;                  // split: [n_utts][segments][width]
  int64_t row_step, utt_step;   // floats from one frame of an utterance to the next / from one utterance to the next
  int64_t T;
  int D, tiles, segments;
};

// the sum of segment `seg` over the tile's columns: valid in thread c for column tile * PL_TILE + c
template <bool VEC>
__device__ __forceinline__ float segment_sum(const float* __restrict__ xb, int64_t row_step, int64_t T, int D,
                                             int col, int seg, float (*lds)[PL_TILE]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t0 = (int64_t)seg * PL_SEG;
  const int n = (int)min((int64_t)PL_SEG, T - t0);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int U = 8;          // loads in flight per lane; the adds stay in row order
  int i = wave;
  for (; i + (U - 1) * PL_WAVES < n; i += U * PL_WAVES) {
    float v[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) load4z<VEC>(xb + (t0 + i + u * PL_WAVES) * row_step, col, D, v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += v[u][k];
  }
  for (; i < n; i += PL_WAVES) {
    float v[4];
    load4z<VEC>(xb + (t0 + i) * row_step, col, D, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += v[k];
  }
  __syncthreads();              // (the previous segment's reads of lds)
#pragma unroll
  for (int k = 0; k < 4; ++k) lds[wave][4 * lane + k] = s[k];
  __syncthreads();
  const int c = threadIdx.x;
  return ((lds[0][c] + lds[1][c]) + lds[2][c]) + lds[3][c];
}

template <bool VEC, bool SPLIT>
__global__ __launch_bounds__(PL_THREADS) void pool_mean_kernel(PoolArgs a) {
  __shared__ float lds[PL_WAVES][PL_TILE];
  const int tile = blockIdx.x % a.tiles;
  const int64_t b = blockIdx.x / a.tiles;
  const int lane = threadIdx.x & 63;
  const int col = tile * PL_TILE + 4 * lane;            // the lane's columns while it loads
  const int c = tile * PL_TILE + threadIdx.x;           // the thread's column once the waves are added
  const float* xb = a.x + b * a.utt_step;
  if (SPLIT) {
    const int seg = blockIdx.y;
    const float v = segment_sum<VEC>(xb, a.row_step, a.T, a.D, col, seg, lds);
    if (c < a.D) a.part[(b * a.segments + seg) * a.D + c] = v;
  } else {
    float tot = 0.f;
    for (int seg = 0; seg < a.segments; ++seg) tot += segment_sum<VEC>(xb, a.row_step, a.T, a.D, col, seg, lds);
    if (c < a.D) a.y[b * a.ldy + c] = tot / (float)a.lens[b];
  }
}

// second stage of the split: the segment sums in ascending order, one thread per (utterance, column)
__global__ __launch_bounds__(256) void pool_mean_finish_kernel(PoolArgs a, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / a.D;
  const int c = (int)(i - b * a.D);
  const float* p = a.part + b * a.segments * a.D + c;
  float tot = 0.f;
  for (int seg = 0; seg < a.segments; ++seg) tot += p[(int64_t)seg * a.D];
  a.y[b * a.ldy + c] = tot / (float)a.lens[b];
}

// the selected row of an utterance: len - 1 clamped into [0, T), or T - 1 without lengths
__device__ __forceinline__ int64_t last_row(const int64_t* lens, int64_t b, int64_t T) {
  if (!lens) return T - 1;
  return min(max(lens[b] - 1, (int64_t)0), T - 1);
}

// mode LAST reads n_utts * width floats: one thread per element
__global__ __launch_bounds__(256) void pool_last_kernel(PoolArgs a, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / a.D;
  const int c = (int)(i - b * a.D);
  a.y[b * a.ldy + c] = a.x[b * a.utt_step + last_row(a.lens, b, a.T) * a.row_step + c];
}

struct PoolBwdArgs {
  const float* dy; int64_t lddy;
  const int64_t* lens;
  float* dx; int64_t lddx;
  int64_t rows, T;              // rows = n_utts * T positions in memory order
  int B, D, batch_first, mode;
};

constexpr int PB_ROWS = 16;     // positions a workgroup writes

// every position of dx: dy[b] / len_b (MEAN), dy[b] at the selected row and zeros elsewhere (LAST)
template <bool VEC>
__global__ __launch_bounds__(256) void pool_bwd_kernel(PoolBwdArgs a) {
  __shared__ int64_t utt[PB_ROWS];
  __shared__ float scale[PB_ROWS];      // MEAN: len_b; LAST: 1 at the selected row, else 0
  const int64_t r0 = (int64_t)blockIdx.x * PB_ROWS;
  const int nr = (int)min((int64_t)PB_ROWS, a.rows - r0);
  if ((int)threadIdx.x < nr) {
    const int64_t r = r0 + threadIdx.x;
    const int64_t b = a.batch_first ? r / a.T : r % a.B;
    const int64_t t = a.batch_first ? r % a.T : r / a.B;
    utt[threadIdx.x] = b;
    scale[threadIdx.x] = a.mode == ITTS_POOL_MEAN ? (float)a.lens[b] : (t == last_row(a.lens, b, a.T) ? 1.f : 0.f);
  }
  __syncthreads();
  const int nq = (a.D + 3) / 4;
  for (int i = threadIdx.x; i < nr * nq; i += 256) {
    const int r = i / nq, col = 4 * (i - r * nq);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const float sc = scale[r];
    if (a.mode == ITTS_POOL_MEAN) {
      load4z<VEC>(a.dy + utt[r] * a.lddy, col, a.D, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = v[k] / sc;
    } else if (sc != 0.f) {
      load4z<VEC>(a.dy + utt[r] * a.lddy, col, a.D, v);
    }
    store4<VEC>(a.dx + (r0 + r) * a.lddx, col, a.D, v);
  }
}

// ---- reparameterisation ------------------------------------------------------------------------------------
struct ReparamArgs {
  const float* h; int64_t ldh;      // [M, 2L]: mu | log_var
  const float* eps; int64_t lde;
  float* z; int64_t ldz;
  const float* dz; int64_t lddz;
  const float* dmu; int64_t lddmu;
  const float* dlv; int64_t lddlv;
  float* dh; int64_t lddh;
  int64_t M;
  int L;
};

template <bool VEC>
__global__ __launch_bounds__(256) void reparam_fwd_kernel(ReparamArgs a) {
  const int nq = (a.L + 3) / 4;
  const int64_t n = a.M * nq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / nq;
    const int col = 4 * (int)(i - r * nq);
    float mu[4], lv[4], e[4];
    load4z<VEC>(a.h + r * a.ldh, col, a.L, mu);
    load4z<VEC>(a.h + r * a.ldh + a.L, col, a.L, lv);
    load4z<VEC>(a.eps + r * a.lde, col, a.L, e);
#pragma unroll
    for (int k = 0; k < 4; ++k) mu[k] = e[k] * expf(0.5f * lv[k]) + mu[k];
    store4<VEC>(a.z + r * a.ldz, col, a.L, mu);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void reparam_bwd_kernel(ReparamArgs a) {
  const int nq = (a.L + 3) / 4;
  const int64_t n = a.M * nq;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / nq;
    const int col = 4 * (int)(i - r * nq);
    float g[4] = {0.f, 0.f, 0.f, 0.f}, gm[4] = {0.f, 0.f, 0.f, 0.f}, gl[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.dmu) load4z<VEC>(a.dmu + r * a.lddmu, col, a.L, gm);
    if (a.dlv) load4z<VEC>(a.dlv + r * a.lddlv, col, a.L, gl);
    if (a.dz) {
      float lv[4], e[4];
      load4z<VEC>(a.dz + r * a.lddz, col, a.L, g);
      load4z<VEC>(a.h + r * a.ldh + a.L, col, a.L, lv);
      load4z<VEC>(a.eps + r * a.lde, col, a.L, e);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gm[k] = g[k] + gm[k];
        gl[k] = 0.5f * g[k] * e[k] * expf(0.5f * lv[k]) + gl[k];
      }
    }
    store4<VEC>(a.dh + r * a.lddh, col, a.L, gm);
    store4<VEC>(a.dh + r * a.lddh + a.L, col, a.L, gl);
  }
}

int elementwise_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096)); }

// ---- KL divergence to the standard normal ---------------------------------------------------------------------
constexpr int KL_WAVES = 4;
constexpr int64_t KL_MAX_BLOCKS = 1024;

int64_t kl_rows_per_block(int64_t M) {
  return KL_WAVES * std::max<int64_t>(1, (M + KL_WAVES * KL_MAX_BLOCKS - 1) / (KL_WAVES * KL_MAX_BLOCKS));
}
int64_t kl_blocks(int64_t M) {
  const int64_t R = kl_rows_per_block(M);
  return (M + R - 1) / R;
}

struct KlArgs {
  const float* mu; int64_t ldmu;
  const float* lv; int64_t ldlv;
  const float* w;
  float* dmu; int64_t lddmu;
  float* dlv; int64_t lddlv;
  float* elem;
  double* partial;              // [blocks]
  int64_t M, rows;
  int L;
};

// One wave per row: lane l takes the columns 4 (l + 64 j) .. + 3 in ascending j, the wave adds by the xor
// butterfly, so a row's KL depends on the row alone.  The block's rows are added in double, per wave in ascending
// row order, the four waves in wave order.
template <bool VEC>
__global__ __launch_bounds__(KL_WAVES * kWave) void kl_kernel(KlArgs a) {
  __shared__ double wsum[KL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * a.rows, r1 = min(a.M, r0 + a.rows);
  double acc = 0.0;
  for (int64_t r = r0 + wave; r < r1; r += KL_WAVES) {
    const float wr = a.w[r];
    float s = 0.f;
    for (int col = 4 * lane; col < a.L; col += 4 * kWave) {
      float m[4], l[4], gm[4], gl[4];
      load4z<VEC>(a.mu + r * a.ldmu, col, a.L, m);
      load4z<VEC>(a.lv + r * a.ldlv, col, a.L, l);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float e = expf(l[k]);
        if (col + k < a.L) s += e + m[k] * m[k] - 1.f - l[k];
        gm[k] = wr == 0.f ? 0.f : wr * m[k];                    // rows of weight 0 may hold anything (also NaN)
        gl[k] = wr == 0.f ? 0.f : 0.5f * wr * (e - 1.f);
      }
      if (a.dmu) store4<VEC>(a.dmu + r * a.lddmu, col, a.L, gm);
      if (a.dlv) store4<VEC>(a.dlv + r * a.lddlv, col, a.L, gl);
    }
    const float kl = wr == 0.f ? 0.f : wr * (0.5f * wave_sum(s));
    if (lane == 0 && a.elem) a.elem[r] = kl;
    acc += (double)kl;
  }
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

}  // namespace
}  // namespace itts

using namespace itts;

#define POOL_CHECK_SIZES()                                                                                    \
  ITTS_REQUIRE(mode == ITTS_POOL_LAST || mode == ITTS_POOL_MEAN, "unknown mode = " + std::to_string(mode));   \
  ITTS_REQUIRE(width >= 1, "width = " + std::to_string(width) + " is not positive");                          \
  ITTS_REQUIRE(t_max >= 1, "t_max = " + std::to_string(t_max) + " is not positive");                          \
  ITTS_REQUIRE(n_utts >= 0, "n_utts = " + std::to_string(n_utts) + " is negative")

// the split form maps the segments onto the grid's second extent
static bool pool_plan_fits(const PoolPlan& p) { return !p.split || p.segments <= PL_MAX_SEGMENTS; }

extern "C" int itts_time_pool_plan(int n_utts, int64_t t_max, int width, int* segments, int* split,
                                   int64_t* workspace_bytes) {
  if (n_utts < 0 || width < 1 || t_max < 1 || t_max > PL_SEG * (int64_t)0x7fffffff) return -1;
  const PoolPlan p = pool_plan(n_utts, t_max, width);
  if (!pool_plan_fits(p)) return -1;
  if (segments) *segments = p.segments;
  if (split) *split = p.split ? 1 : 0;
  if (workspace_bytes)
    *workspace_bytes = p.split ? (int64_t)n_utts * p.segments * width * (int64_t)sizeof(float) : 0;
  return 0;
}

extern "C" int itts_time_pool_fwd(const float* d_x, int64_t ldx, const int64_t* d_lens, int n_utts, int64_t t_max,
                                  int width, int batch_first, int mode, float* d_y, int64_t ldy,
                                  void* d_workspace, void* stream) {
  POOL_CHECK_SIZES();
  ITTS_REQUIRE(ldx >= width, "pitch ldx = " + std::to_string(ldx) + " is below the width " + std::to_string(width));
  ITTS_REQUIRE(ldy >= width, "pitch ldy = " + std::to_string(ldy) + " is below the width " + std::to_string(width));
  ITTS_REQUIRE(mode != ITTS_POOL_MEAN || d_lens || n_utts == 0, "mode MEAN divides by the lengths: d_lens is NULL");
  if (n_utts == 0) return ITTS_OK;
  ITTS_REQUIRE(d_x && d_y, "null pointer (d_x / d_y) with n_utts = " + std::to_string(n_utts));
  hipStream_t s = as_stream(stream);
  PoolArgs a{};
  a.x = d_x; a.ldx = ldx; a.lens = d_lens; a.y = d_y; a.ldy = ldy;
  a.row_step = batch_first ? ldx : (int64_t)n_utts * ldx;
  a.utt_step = batch_first ? t_max * ldx : ldx;
  a.T = t_max; a.D = width;
  const int64_t n = (int64_t)n_utts * width;
  if (mode == ITTS_POOL_LAST) {
    pool_last_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(a, n);
    ITTS_LAUNCH_CHECK();
    return ITTS_OK;
  }
  ITTS_REQUIRE(t_max <= PL_SEG * (int64_t)0x7fffffff, "t_max = " + std::to_string(t_max) + " is too large");
  const PoolPlan p = pool_plan(n_utts, t_max, width);
  ITTS_REQUIRE(pool_plan_fits(p), "t_max = " + std::to_string(t_max) + " exceeds the " +
                                      std::to_string(PL_SEG * PL_MAX_SEGMENTS) + " frames the time-split form takes");
  a.tiles = p.tiles; a.segments = p.segments;
  ITTS_REQUIRE((int64_t)n_utts * p.tiles <= 0x7fffffff, "n_utts = " + std::to_string(n_utts) + " is too large");
  ITTS_REQUIRE(!p.split || d_workspace, "null workspace: this shape sums time in two stages (itts_time_pool_plan)");
  a.part = reinterpret_cast<float*>(d_workspace);
  const bool vec = rows16(d_x, ldx);
  const unsigned gx = (unsigned)(n_utts * p.tiles);
  if (p.split) {
    const dim3 grid(gx, (unsigned)p.segments);
    if (vec) pool_mean_kernel<true, true><<<grid, PL_THREADS, 0, s>>>(a);
    else pool_mean_kernel<false, true><<<grid, PL_THREADS, 0, s>>>(a);
    ITTS_LAUNCH_CHECK();
    pool_mean_finish_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(a, n);
  } else {
    if (vec) pool_mean_kernel<true, false><<<dim3(gx), PL_THREADS, 0, s>>>(a);
    else pool_mean_kernel<false, false><<<dim3(gx), PL_THREADS, 0, s>>>(a);
  }
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_time_pool_bwd(const float* d_dy, int64_t lddy, const int64_t* d_lens, int n_utts, int64_t t_max,
                                  int width, int batch_first, int mode, float* d_dx, int64_t lddx, void* stream) {
  POOL_CHECK_SIZES();
  ITTS_REQUIRE(lddy >= width, "pitch lddy = " + std::to_string(lddy) + " is below the width " + std::to_string(width));
  ITTS_REQUIRE(lddx >= width, "pitch lddx = " + std::to_string(lddx) + " is below the width " + std::to_string(width));
  ITTS_REQUIRE(mode != ITTS_POOL_MEAN || d_lens || n_utts == 0, "mode MEAN divides by the lengths: d_lens is NULL");
  if (n_utts == 0) return ITTS_OK;
  ITTS_REQUIRE(d_dy && d_dx, "null pointer (d_dy / d_dx) with n_utts = " + std::to_string(n_utts));
  PoolBwdArgs a{};
  a.dy = d_dy; a.lddy = lddy; a.lens = d_lens; a.dx = d_dx; a.lddx = lddx;
  a.rows = (int64_t)n_utts * t_max; a.T = t_max; a.B = n_utts; a.D = width;
  a.batch_first = batch_first ? 1 : 0; a.mode = mode;
  const int64_t blocks = (a.rows + PB_ROWS - 1) / PB_ROWS;
  ITTS_REQUIRE(blocks <= 0x7fffffff, "n_utts * t_max = " + std::to_string(a.rows) + " is too large");
  hipStream_t s = as_stream(stream);
  if (rows16(d_dy, lddy) && rows16(d_dx, lddx)) pool_bwd_kernel<true><<<dim3((unsigned)blocks), 256, 0, s>>>(a);
  else pool_bwd_kernel<false><<<dim3((unsigned)blocks), 256, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

#define LATENT_CHECK_ML()                                                                           \
  ITTS_REQUIRE(L >= 1, "latent width L = " + std::to_string(L) + " is not positive");               \
  ITTS_REQUIRE(M >= 0, "M = " + std::to_string(M) + " is negative")
#define LATENT_CHECK_PITCH(ld, min)                                                                 \
  ITTS_REQUIRE(ld >= (min), "pitch " #ld " = " + std::to_string(ld) + " is below the width " + std::to_string(min))

extern "C" int itts_vae_reparam_fwd(const float* d_h, int64_t ldh, const float* d_eps, int64_t lde, float* d_z,
                                    int64_t ldz, int64_t M, int L, void* stream) {
  LATENT_CHECK_ML();
  LATENT_CHECK_PITCH(ldh, 2 * (int64_t)L);
  LATENT_CHECK_PITCH(lde, L);
  LATENT_CHECK_PITCH(ldz, L);
  if (M == 0) return ITTS_OK;
  ITTS_REQUIRE(d_h && d_eps && d_z, "null pointer (d_h / d_eps / d_z) with M = " + std::to_string(M));
  ReparamArgs a{};
  a.h = d_h; a.ldh = ldh; a.eps = d_eps; a.lde = lde; a.z = d_z; a.ldz = ldz; a.M = M; a.L = L;
  const bool vec = L % 4 == 0 && rows16(d_h, ldh) && rows16(d_eps, lde) && rows16(d_z, ldz);
  const int nb = elementwise_blocks(M * ((L + 3) / 4));
  hipStream_t s = as_stream(stream);
  if (vec) reparam_fwd_kernel<true><<<dim3(nb), 256, 0, s>>>(a);
  else reparam_fwd_kernel<false><<<dim3(nb), 256, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_vae_reparam_bwd(const float* d_dz, int64_t lddz, const float* d_dmu, int64_t lddmu,
                                    const float* d_dlv, int64_t lddlv, const float* d_h, int64_t ldh,
                                    const float* d_eps, int64_t lde, float* d_dh, int64_t lddh, int64_t M, int L,
                                    void* stream) {
  LATENT_CHECK_ML();
  LATENT_CHECK_PITCH(lddh, 2 * (int64_t)L);
  if (d_dz) {
    LATENT_CHECK_PITCH(lddz, L);
    LATENT_CHECK_PITCH(ldh, 2 * (int64_t)L);
    LATENT_CHECK_PITCH(lde, L);
  }
  if (d_dmu) LATENT_CHECK_PITCH(lddmu, L);
  if (d_dlv) LATENT_CHECK_PITCH(lddlv, L);
  if (M == 0) return ITTS_OK;
  ITTS_REQUIRE(d_dh, "null pointer (d_dh) with M = " + std::to_string(M));
  ITTS_REQUIRE(!d_dz || (d_h && d_eps), "null pointer (d_h / d_eps): the gradient of z needs both");
  ReparamArgs a{};
  a.h = d_h; a.ldh = ldh; a.eps = d_eps; a.lde = lde; a.dz = d_dz; a.lddz = lddz; a.dmu = d_dmu; a.lddmu = lddmu;
  a.dlv = d_dlv; a.lddlv = lddlv; a.dh = d_dh; a.lddh = lddh; a.M = M; a.L = L;
  const bool vec = L % 4 == 0 && rows16(d_dh, lddh) && (!d_dz || (rows16(d_dz, lddz) && rows16(d_h, ldh) &&
                                                                 rows16(d_eps, lde))) &&
                   (!d_dmu || rows16(d_dmu, lddmu)) && (!d_dlv || rows16(d_dlv, lddlv));
  const int nb = elementwise_blocks(M * ((L + 3) / 4));
  hipStream_t s = as_stream(stream);
  if (vec) reparam_bwd_kernel<true><<<dim3(nb), 256, 0, s>>>(a);
  else reparam_bwd_kernel<false><<<dim3(nb), 256, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int64_t itts_vae_kld_workspace_bytes(int64_t M, int L) {
  if (M <= 0 || L <= 0) return 0;
  return kl_blocks(M) * (int64_t)sizeof(double);
}

extern "C" int itts_vae_kld(const float* d_mu, int64_t ldmu, const float* d_lv, int64_t ldlv, const float* d_w,
                            int64_t M, int L, float* d_loss, float* d_dmu, int64_t lddmu, float* d_dlv,
                            int64_t lddlv, float* d_elem, void* d_workspace, void* stream) {
  LATENT_CHECK_ML();
  LATENT_CHECK_PITCH(ldmu, L);
  LATENT_CHECK_PITCH(ldlv, L);
  if (d_dmu) LATENT_CHECK_PITCH(lddmu, L);
  if (d_dlv) LATENT_CHECK_PITCH(lddlv, L);
  ITTS_REQUIRE(d_loss, "null pointer (d_loss)");
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    ITTS_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(float), s));
    return ITTS_OK;
  }
  ITTS_REQUIRE(d_mu && d_lv && d_w && d_workspace,
               "null pointer (d_mu / d_lv / d_w / d_workspace) with M = " + std::to_string(M));
  KlArgs a{};
  a.mu = d_mu; a.ldmu = ldmu; a.lv = d_lv; a.ldlv = ldlv; a.w = d_w; a.dmu = d_dmu; a.lddmu = lddmu;
  a.dlv = d_dlv; a.lddlv = lddlv; a.elem = d_elem; a.partial = reinterpret_cast<double*>(d_workspace);
  a.M = M; a.rows = kl_rows_per_block(M); a.L = L;
  const bool vec = rows16(d_mu, ldmu) && rows16(d_lv, ldlv) && (!d_dmu || rows16(d_dmu, lddmu)) &&
                   (!d_dlv || rows16(d_dlv, lddlv));
  const int nb = (int)kl_blocks(M);
  if (vec) kl_kernel<true><<<dim3(nb), KL_WAVES * kWave, 0, s>>>(a);
  else kl_kernel<false><<<dim3(nb), KL_WAVES * kWave, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return loss_final_sum(a.partial, nb, 1.0, d_loss, s);
}
