// Dynamic time warping of pairs of feature sequences (Metrics.get_metrics_dtw: MCD-DTW and the scores taken on its
// path; the reference project has no counterpart).  For pair b, x [T1, D] and y [T2, D]:
//   d(i, j) = sqrt(sum_k (x[i, k] - y[j, k])^2),
//   C(0, 0) = d(0, 0),   C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1)),
// a predecessor outside the grid or the band counting as +inf; on equal values the diagonal wins, then (i-1, j), then
// (i, j-1).  Everything is float64: float32 inputs are widened when they are staged, no cost is ever added in fp32.
//
// Forward kernel: ONE workgroup of 256 threads per pair, no workgroup waits on another (no flags, no polling, no
// atomics), every loop bound follows from (T1, T2, D, band) and is the same in all threads of the workgroup.  The grid
// is cut into column blocks of DTW_W = 128 columns (outer loop) and passes of DTW_R = 64 rows (inner loop).  A tile:
//   1. distances: all four waves.  x and y are staged through LDS in slabs of 16 features, k-major; a thread owns 4
//      rows x 8 columns of the tile and keeps their 32 sums of squares in registers across the slabs (12 LDS reads for
//      64 flops a feature).  Reads behind a length or behind D are not issued (the slab holds zeros there).  The
//      square roots go to the LDS tile, column-major so that the lanes of step 2 read adjacent words.
//   2. recurrence: wave 0, lane = row.  At step s lane t takes column s - t; C(i-1, j) comes from the lane above by a
//      lane shift, C(i-1, j-1) is what came the step before, C(i, j-1) is the lane's own last value.  Row r0 - 1 is
//      the boundary row the pass before left in LDS, column c0 - 1 the boundary column the block before left there
//      (T1 values): nothing else of C outlives a tile, and C never goes to HBM.  The decisions (0 diagonal, 1 up,
//      2 left) go to a byte tile in LDS.
//   3. all four waves copy the byte tile to HBM, rows contiguous: one byte per cell, the only HBM traffic per cell.
// Tiles that hold no cell of the band are skipped (their boundaries are set to +inf); cells outside the band inside a
// kept tile are neither taken through step 2 nor stored.
//
// Backtrack kernel: one wave per pair.  The wave loads the 8 x 8 window of decisions up and left of where it stands
// (one byte per lane), walks inside it by lane reads, and loads again when it leaves the window: at most
// T1 + T2 - 1 steps, at least 8 of them per load.  The path is written from the back of its buffer, moved to the
// front, and the rest of the buffer set to -1.
//
// A pair's bits depend on its own rows, lengths and the band only: not on B, its index, or the padded sizes.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "context.h"

namespace itts {
namespace {

constexpr int DTW_R = 64;                   // rows per pass (= lanes of the recurrence wave)
constexpr int DTW_W = 128;                  // columns per block
constexpr int DTW_KC = 16;                  // features per staged slab
constexpr int DTW_THREADS = 256;
constexpr int DTW_MAX_T = 4096;
constexpr int DTW_MAX_D = 128;
constexpr int DTW_TR = 4, DTW_TC = 8;       // cells of a thread in step 1

// LDS of the forward kernel, in doubles (the byte tile and the band limits behind them)
constexpr int DTW_L_TILE = 0;                                   // [W][R] distances
constexpr int DTW_L_COLB = DTW_L_TILE + DTW_W * DTW_R;          // [MAX_T + R] boundary column
constexpr int DTW_L_ROWB = DTW_L_COLB + DTW_MAX_T + DTW_R;      // [W] boundary row
constexpr int DTW_L_XS = DTW_L_ROWB + DTW_W;                    // [KC][R]
constexpr int DTW_L_YS = DTW_L_XS + DTW_KC * DTW_R;             // [KC][W]
constexpr int DTW_L_END = DTW_L_YS + DTW_KC * DTW_W;
constexpr size_t DTW_LDS_BYTES = (size_t)DTW_L_END * sizeof(double) + DTW_R * DTW_W + 2 * DTW_R * sizeof(int);

struct DtwArgs {
  const void* x; int64_t ldx, uttx;         // [B, T1max, D]: elements from one frame / one pair to the next
  const void* y; int64_t ldy, utty;         // [B, T2max, D]
  const int* t1; const int* t2;             // [B] device copies of the lengths
  int D, band;
  uint8_t* dec; int64_t pair_bytes; int pitch;   // decisions: pair b at dec + b * pair_bytes, row i at + i * pitch
  double* cost; int* length;                // [B]
  int* path; int64_t path_rows;             // [B, path_rows, 2] or NULL
};

// Columns of row i inside the band, lo .. hi (clipped to the grid).  centre(i) = round(i (T2-1) / (T1-1)), half up, in
// integers; T1 == 1 has one monotone path, the whole row, and no band.
__host__ __device__ inline void dtw_band_range(int i, int T1, int T2, int band, int* lo, int* hi) {
  if (band < 0 || T1 == 1) { *lo = 0; *hi = T2 - 1; return; }
  const int den = T1 - 1;
  const int centre = (int)((2ll * i * (T2 - 1) + den) / (2ll * den));
  *lo = centre - band > 0 ? centre - band : 0;
  *hi = (int64_t)centre + band < T2 - 1 ? centre + band : T2 - 1;
}

template <typename T>
__global__ __launch_bounds__(DTW_THREADS) void dtw_forward_kernel(DtwArgs a) {
  extern __shared__ double dtw_lds[];
  double* tile = dtw_lds + DTW_L_TILE;
  double* colb = dtw_lds + DTW_L_COLB;
  double* rowb = dtw_lds + DTW_L_ROWB;
  double* xs = dtw_lds + DTW_L_XS;
  double* ys = dtw_lds + DTW_L_YS;
  uint8_t* decb = reinterpret_cast<uint8_t*>(dtw_lds + DTW_L_END);       // [R][W]
  int* rlo = reinterpret_cast<int*>(decb + DTW_R * DTW_W);               // [R] band limits of the pass's rows
  int* rhi = rlo + DTW_R;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T1 = a.t1[b], T2 = a.t2[b], D = a.D, band = a.band;
  const T* X = static_cast<const T*>(a.x) + b * a.uttx;
  const T* Y = static_cast<const T*>(a.y) + b * a.utty;
  uint8_t* dec = a.dec + b * a.pair_bytes;
  const double INF = __builtin_huge_val();
  const int tr = (tid & 15) * DTW_TR, tc = (tid >> 4) * DTW_TC;
  double corner = INF;                       // wave 0: C(r0 - 1, c0 - 1), the boundary column's value the pass before overwrote

  for (int c0 = 0; c0 < T2; c0 += DTW_W) {
    const int ncol = min(DTW_W, T2 - c0);
    for (int r0 = 0; r0 < T1; r0 += DTW_R) {
      const int nrow = min(DTW_R, T1 - r0);
      int lo_first, hi_first, lo_last, hi_last;
      dtw_band_range(r0, T1, T2, band, &lo_first, &hi_first);
      dtw_band_range(r0 + nrow - 1, T1, T2, band, &lo_last, &hi_last);
      const bool keep = hi_last >= c0 && lo_first <= c0 + ncol - 1;       // (the centre does not decrease with i)
      if (!keep) {
        if (wave == 0) {
          const int i = r0 + lane;
          const double old = colb[i];
          corner = __shfl(old, DTW_R - 1, 64);
          colb[i] = INF;
          rowb[lane] = INF;
          rowb[lane + 64] = INF;
        }
        __syncthreads();
        continue;
      }
      // ---- 1. distances of the tile
      double acc[DTW_TR][DTW_TC];
#pragma unroll
      for (int p = 0; p < DTW_TR; ++p)
#pragma unroll
        for (int q = 0; q < DTW_TC; ++q) acc[p][q] = 0.0;
      for (int k0 = 0; k0 < D; k0 += DTW_KC) {
        for (int e = tid; e < DTW_R * DTW_KC; e += DTW_THREADS) {
          const int row = e / DTW_KC, k = e % DTW_KC;
          const int i = r0 + row;
          xs[k * DTW_R + row] = (i < T1 && k0 + k < D) ? (double)X[(int64_t)i * a.ldx + k0 + k] : 0.0;
        }
        for (int e = tid; e < DTW_W * DTW_KC; e += DTW_THREADS) {
          const int col = e / DTW_KC, k = e % DTW_KC;
          const int j = c0 + col;
          ys[k * DTW_W + col] = (j < T2 && k0 + k < D) ? (double)Y[(int64_t)j * a.ldy + k0 + k] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < DTW_KC; ++k) {
          double xv[DTW_TR], yv[DTW_TC];
#pragma unroll
          for (int p = 0; p < DTW_TR; ++p) xv[p] = xs[k * DTW_R + tr + p];
#pragma unroll
          for (int q = 0; q < DTW_TC; ++q) yv[q] = ys[k * DTW_W + tc + q];
#pragma unroll
          for (int p = 0; p < DTW_TR; ++p)
#pragma unroll
            for (int q = 0; q < DTW_TC; ++q) {
              const double df = xv[p] - yv[q];
              acc[p][q] = fma(df, df, acc[p][q]);
            }
        }
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < DTW_TC; ++q)
#pragma unroll
        for (int p = 0; p < DTW_TR; ++p) tile[(tc + q) * DTW_R + tr + p] = sqrt(acc[p][q]);
      __syncthreads();
      // ---- 2. the recurrence, wave 0, lane = row
      if (wave == 0) {
        const int t = lane, i = r0 + t;
        const bool row_ok = i < T1;
        int lo = 0, hi = -1;
        if (row_ok) dtw_band_range(i, T1, T2, band, &lo, &hi);
        rlo[t] = lo;
        rhi[t] = hi;
        const double oldcol = colb[i];                                    // C(i, c0 - 1) when c0 > 0
        const double left0 = (c0 > 0 && row_ok) ? oldcol : INF;
        const double diag0 = (c0 > 0 && i > 0 && row_ok) ? (t == 0 ? corner : colb[i - 1]) : INF;
        corner = __shfl(oldcol, DTW_R - 1, 64);
        double cur = INF, diag = INF, last = INF;
        // what a step needs from LDS besides the lane shift is fetched a step ahead, off the dependency chain: the
        // lane's distance, and (lane 0) the boundary row's value, which lane 63 overwrites 64 steps later at the soonest
        double dist = t == 0 ? tile[0] : 0.0;
        double edge = r0 > 0 ? rowb[0] : INF;
        const int nsteps = nrow + ncol - 1;
        for (int s = 0; s < nsteps; ++s) {
          const int c = s - t, cn = c + 1;
          const double dist_next = (cn >= 0 && cn < ncol) ? tile[cn * DTW_R + t] : 0.0;
          const double edge_next = r0 > 0 ? rowb[min(s + 1, ncol - 1)] : INF;
          double up = __shfl_up(cur, 1, 64);
          if (t == 0) up = edge;
          double left = cur;
          if (c == 0) { left = left0; diag = diag0; }
          const int j = c0 + c;
          const bool in_tile = row_ok && c >= 0 && c < ncol;
          double best = diag;
          int d = 0;
          if (up < best) { best = up; d = 1; }
          if (left < best) { best = left; d = 2; }
          if (i == 0 && j == 0) best = 0.0;
          const bool in_band = in_tile && j >= lo && j <= hi;
          const double nc = in_band ? dist + best : INF;
          if (in_band) decb[t * DTW_W + c] = (uint8_t)d;
          if (in_tile && t == DTW_R - 1) rowb[c] = nc;
          if (c == ncol - 1) last = nc;
          diag = up;
          cur = nc;
          dist = dist_next;
          edge = edge_next;
        }
        if (row_ok) {
          colb[i] = last;                                                 // C(i, c0 + ncol - 1)
          if (i == T1 - 1 && c0 + ncol == T2) a.cost[b] = last;
        }
      }
      __syncthreads();
      // ---- 3. the tile's decisions to HBM
      for (int e = tid; e < DTW_R * DTW_W; e += DTW_THREADS) {
        const int row = e / DTW_W, c = e % DTW_W;
        const int i = r0 + row, j = c0 + c;
        if (row < nrow && c < ncol && j >= rlo[row] && j <= rhi[row]) dec[(int64_t)i * a.pitch + j] = decb[e];
      }
      // (the next tile writes decb, rlo and rhi only behind the barriers of its step 1)
    }
  }
}

__global__ __launch_bounds__(kWave) void dtw_backtrack_kernel(DtwArgs a) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int T1 = a.t1[b], T2 = a.t2[b];
  const uint8_t* dec = a.dec + b * a.pair_bytes;
  int2* path = a.path ? reinterpret_cast<int2*>(a.path) + b * a.path_rows : nullptr;
  const int P = T1 + T2 - 1;
  const double cost = a.cost[b];
  int n = 0;
  if (cost < __builtin_huge_val()) {          // (an end cell the band cuts off, or NaN features: no path)
    int i = T1 - 1, j = T2 - 1;
    bool done = false;
    while (!done) {
      const int wi = i - (lane >> 3), wj = j - (lane & 7);
      const int v = (wi >= 0 && wj >= 0) ? dec[(int64_t)wi * a.pitch + wj] : 0;
      int di = 0, dj = 0;
      while (di < 8 && dj < 8) {
        const int ci = i - di, cj = j - dj;
        if (lane == 0 && path) path[P - 1 - n] = make_int2(ci, cj);
        ++n;
        if (ci == 0 && cj == 0) { done = true; break; }
        int d = __shfl(v, di * 8 + dj, 64);
        if (ci == 0) d = 2;                   // the grid's edges leave one way
        else if (cj == 0) d = 1;
        if (d == 0) { ++di; ++dj; }
        else if (d == 1) ++di;
        else ++dj;
      }
      i -= di;
      j -= dj;
    }
  }
  if (lane == 0) a.length[b] = n;
  if (path) {
    // forward order to the front (a chunk's sources lie at or behind its targets, and behind every earlier chunk's)
    for (int64_t q0 = 0; q0 < a.path_rows; q0 += kWave) {
      const int64_t q = q0 + lane;
      int2 v = make_int2(-1, -1);
      if (q < n) v = path[P - n + q];
      if (q < a.path_rows) path[q] = v;
    }
  }
}

// What one step of a dependency chain costs with nothing else in it (scripts/bench_dtw.py: the floor
// (T1 + T2 - 1) x step that no tiling of the recurrence gets under).  mode 0: 256 threads hand a double to their
// neighbour through LDS with one workgroup barrier a step; mode 1: one wave hands it over by a lane shift, as step 2
// of the forward kernel does.
__global__ __launch_bounds__(DTW_THREADS) void dtw_step_probe_kernel(int mode, int steps, double* out) {
  __shared__ double slot[2][DTW_THREADS];
  const int tid = threadIdx.x;
  double v = (double)tid;
  if (mode == 0) {
    for (int s = 0; s < steps; ++s) {
      slot[s & 1][tid] = v;
      __syncthreads();
      v = fmin(v, slot[s & 1][(tid + DTW_THREADS - 1) % DTW_THREADS]) + 1.0;
    }
  } else if (tid < kWave) {
    for (int s = 0; s < steps; ++s) v = fmin(v, __shfl_up(v, 1, 64)) + 1.0;
  }
  out[tid] = v;
}

bool dtw_sizes_ok(int T1, int T2, int D) {
  return T1 >= 1 && T1 <= DTW_MAX_T && T2 >= 1 && T2 <= DTW_MAX_T && D >= 1 && D <= DTW_MAX_D;
}

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int64_t itts_dtw_workspace_bytes(int B, int T1max, int T2max) {
  if (B < 0 || T1max < 1 || T1max > DTW_MAX_T || T2max < 1 || T2max > DTW_MAX_T) return -1;
  return (int64_t)B * T1max * T2max;
}

extern "C" int itts_dtw_plan(int T1, int T2, int D, int* col_block, int* rows_per_pass, int* cell_bytes_x8) {
  if (!dtw_sizes_ok(T1, T2, D)) return -1;
  if (col_block) *col_block = DTW_W;
  if (rows_per_pass) *rows_per_pass = DTW_R;
  if (cell_bytes_x8) *cell_bytes_x8 = 8;
  return 0;
}

extern "C" int itts_dtw_step_probe(int mode, int steps, double* d_out, void* stream) {
  ITTS_REQUIRE(mode == 0 || mode == 1, "mode = " + std::to_string(mode) + " is not 0 (barrier) or 1 (lane shift)");
  ITTS_REQUIRE(steps >= 0, "steps = " + std::to_string(steps) + " is negative");
  ITTS_REQUIRE(d_out, "null pointer (d_out)");
  dtw_step_probe_kernel<<<dim3(1), DTW_THREADS, 0, as_stream(stream)>>>(mode, steps, d_out);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_dtw_align(const void* d_x, int64_t ldx, int64_t uttx, const void* d_y, int64_t ldy, int64_t utty,
                              int is_f64, const int32_t* h_t1, const int32_t* h_t2, int B, int T1max, int T2max, int D,
                              int band, double* d_cost, int32_t* d_length, int32_t* d_path, int64_t path_rows,
                              void* d_work, int64_t work_bytes, void* stream) {
  ITTS_REQUIRE(B >= 1, "B = " + std::to_string(B) + " is below 1");
  ITTS_REQUIRE(D >= 1 && D <= DTW_MAX_D, "D = " + std::to_string(D) + " is outside 1 .. " + std::to_string(DTW_MAX_D));
  ITTS_REQUIRE(T1max >= 1 && T1max <= DTW_MAX_T,
               "T1max = " + std::to_string(T1max) + " is outside 1 .. " + std::to_string(DTW_MAX_T));
  ITTS_REQUIRE(T2max >= 1 && T2max <= DTW_MAX_T,
               "T2max = " + std::to_string(T2max) + " is outside 1 .. " + std::to_string(DTW_MAX_T));
  ITTS_REQUIRE(h_t1 && h_t2, "null pointer (h_t1 / h_t2)");
  for (int b = 0; b < B; ++b) {
    ITTS_REQUIRE(h_t1[b] >= 1 && h_t1[b] <= T1max, "T1[" + std::to_string(b) + "] = " + std::to_string(h_t1[b]) +
                                                       " is outside 1 .. T1max = " + std::to_string(T1max));
    ITTS_REQUIRE(h_t2[b] >= 1 && h_t2[b] <= T2max, "T2[" + std::to_string(b) + "] = " + std::to_string(h_t2[b]) +
                                                       " is outside 1 .. T2max = " + std::to_string(T2max));
  }
  ITTS_REQUIRE(ldx >= D, "pitch ldx = " + std::to_string(ldx) + " is below D = " + std::to_string(D));
  ITTS_REQUIRE(ldy >= D, "pitch ldy = " + std::to_string(ldy) + " is below D = " + std::to_string(D));
  ITTS_REQUIRE(B == 1 || uttx >= (int64_t)(T1max - 1) * ldx + D,
               "pair step uttx = " + std::to_string(uttx) + " is below a pair's extent");
  ITTS_REQUIRE(B == 1 || utty >= (int64_t)(T2max - 1) * ldy + D,
               "pair step utty = " + std::to_string(utty) + " is below a pair's extent");
  const int64_t need = (int64_t)B * T1max * T2max;
  ITTS_REQUIRE(work_bytes >= need, "work_bytes = " + std::to_string(work_bytes) + " is below the " +
                                       std::to_string(need) + " of itts_dtw_workspace_bytes");
  ITTS_REQUIRE(!d_path || path_rows >= (int64_t)T1max + T2max - 1,
               "path_rows = " + std::to_string(path_rows) + " is below T1max + T2max - 1 = " +
                   std::to_string(T1max + T2max - 1));
  ITTS_REQUIRE(d_x && d_y && d_cost && d_length && d_work, "null pointer (d_x / d_y / d_cost / d_length / d_work)");
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  int* d_len = nullptr;
  ITTS_HIP_CHECK(scratch.take(&d_len, (size_t)2 * B));
  {
    std::vector<int> lens((size_t)2 * B);
    std::copy(h_t1, h_t1 + B, lens.begin());
    std::copy(h_t2, h_t2 + B, lens.begin() + B);
    if (int rc = staged_upload(d_len, lens.data(), lens.size() * sizeof(int), s)) return rc;
  }
  DtwArgs a{};
  a.x = d_x; a.ldx = ldx; a.uttx = uttx; a.y = d_y; a.ldy = ldy; a.utty = utty;
  a.t1 = d_len; a.t2 = d_len + B; a.D = D; a.band = band < 0 ? -1 : band;
  a.dec = static_cast<uint8_t*>(d_work); a.pair_bytes = (int64_t)T1max * T2max; a.pitch = T2max;
  a.cost = d_cost; a.length = d_length; a.path = d_path; a.path_rows = path_rows;
  if (is_f64) {
    ITTS_HIP_CHECK(allow_dynamic_lds(reinterpret_cast<const void*>(&dtw_forward_kernel<double>), DTW_LDS_BYTES));
    dtw_forward_kernel<double><<<dim3((unsigned)B), DTW_THREADS, DTW_LDS_BYTES, s>>>(a);
  } else {
    ITTS_HIP_CHECK(allow_dynamic_lds(reinterpret_cast<const void*>(&dtw_forward_kernel<float>), DTW_LDS_BYTES));
    dtw_forward_kernel<float><<<dim3((unsigned)B), DTW_THREADS, DTW_LDS_BYTES, s>>>(a);
  }
  ITTS_LAUNCH_CHECK();
  dtw_backtrack_kernel<<<dim3((unsigned)B), kWave, 0, s>>>(a);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}
