// MLPG, the stream form: prep -> reduce -> scan -> solve, no wait anywhere.  Included by mlpg.hip only.
#pragma once
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.h"
#include "context.h"
#include "mlpg_math.h"
#include "mlpg_sweeps.h"      // mlpg_factor_block

namespace itts {

// ---- chunk geometry, factor access and the two sweeps of one chunk -------------------------------
// (shared by the reduce and the solve kernel below)
template <int FU_FL>
__device__ __host__ __forceinline__ int fu_num_chunks(int64_t T) { return (int)((T + FU_FL - 1) / FU_FL); }
// the last chunk always holds both re-derived tail frames: a one-frame remainder takes a frame
// from the chunk before it
template <int FU_FL>
__device__ __forceinline__ int64_t fu_chunk_start(int k, int K, int64_t T) {
  int64_t s = (int64_t)k * FU_FL;
  if (k == K - 1 && K > 1 && T - s == 1) s -= 1;
  return k >= K ? T : s;
}

struct FuFac {
  const double* fd;
  const double* fl1;
  const double* fl2;
  int64_t ncv, n_shared;
  MlpgPrec<int64_t> prec;
  int D;
  __device__ __forceinline__ void open(const MlpgArgs& a, int t_max, int d, int64_t T_, double v0, double v1, double v2) {
    const int64_t plane = (int64_t)t_max * a.dim;
    fd = a.scratch + d; fl1 = fd + plane; fl2 = fl1 + plane;
    ncv = a.nconv[d]; n_shared = T_ >= 3 ? T_ - 2 : 0; D = a.dim;
    prec = MlpgPrec<int64_t>{T_, 1.0 / v0, 1.0 / v1, 1.0 / v2};
  }
  __device__ __forceinline__ double F(const double* pl, int64_t j) const {
    return j < 0 ? 0.0 : pl[(j < ncv ? j : ncv) * D];
  }
  // factor of a tail frame (j >= n_shared) from the Cholesky state that reaches it, kept in tl
  __device__ __forceinline__ void derive(int64_t j, double l1p, double l2p, double cprev, double& dd,
                                         double& l1, double& l2, MlpgTail& tl) const {
    mlpg_chol_step<false>(prec.row<false>(j), l1p, l2p, cprev, dd, l1, l2);
    tl.put(j, prec.T, dd, l1, l2);
  }
};

// how many of the chunk's n frames starting at j0 take the shared factor (the rest -- at most the
// utterance's last two -- are re-derived)
__device__ __forceinline__ int fu_shared_frames(const FuFac& c, int64_t j0, int n) {
  const int64_t m = c.n_shared - j0;
  return m <= 0 ? 0 : (m < n ? (int)m : n);
}

// Forward sweep over the chunk [j0, j0 + n) from (s1, s2): y replaces b.  tl: factors of frames T-2, T-1.
template <int FU_FL, bool CONST>
__device__ __forceinline__ void fu_fwd(const FuFac& c, double (&b)[FU_FL], int64_t j0, int n, double s1,
                                       double s2, MlpgTail& tl) {
  double kd = 0.0, k1 = 0.0, k2 = 0.0;
  double l1p, l2p, cprev;
  if (CONST) {
    kd = c.fd[c.ncv * c.D];
    k1 = c.fl1[c.ncv * c.D];
    k2 = c.fl2[c.ncv * c.D];
    l1p = k1; l2p = k2; cprev = k2;
  } else {
    l1p = c.F(c.fl1, j0 - 1); l2p = c.F(c.fl2, j0 - 2); cprev = c.F(c.fl2, j0 - 1);
    if (c.n_shared == 0) l1p = l2p = cprev = 0.0;
  }
  double y1 = s1, y2 = s2;
  // frames that take the shared factor first (unrolled), then the utterance's last two, whose
  // factor is re-derived (a rolled loop: one copy of the square root and divisions in the code)
  const int n_main = CONST ? FU_FL : fu_shared_frames(c, j0, n);
#pragma unroll
  for (int i = 0; i < FU_FL; ++i) {
    if (CONST || i < n_main) {
      const int64_t j = j0 + i;
      double dd, l1, l2;
      if (CONST) {
        dd = kd; l1 = k1; l2 = k2;
      } else {
        const int64_t jc = (j < c.ncv ? j : c.ncv) * c.D;
        dd = c.fd[jc]; l1 = c.fl1[jc]; l2 = c.fl2[jc];
      }
      const double y = (b[i] - l1p * y1 - l2p * y2) * dd;
      b[i] = y;
      y2 = y1; y1 = y;
      l2p = cprev; l1p = l1; cprev = l2;
    }
  }
  if (!CONST) {
#pragma unroll 1
    for (int i = n_main; i < n; ++i) {
      double dd, l1, l2;
      c.derive(j0 + i, l1p, l2p, cprev, dd, l1, l2, tl);
      double bi = 0.0;
#pragma unroll
      for (int r = 0; r < FU_FL; ++r) bi = r == i ? b[r] : bi;
      const double y = (bi - l1p * y1 - l2p * y2) * dd;
#pragma unroll
      for (int r = 0; r < FU_FL; ++r) b[r] = r == i ? y : b[r];
      y2 = y1; y1 = y;
      l2p = cprev; l1p = l1; cprev = l2;
    }
  }
}

// Backward sweep over y (in b): x from (s1, s2) = (x_{j1}, x_{j1+1}) written to `o` (row pitch ldo), when `store`.
template <int FU_FL, bool CONST>
__device__ __forceinline__ void fu_bwd(const FuFac& c, double (&b)[FU_FL], int64_t j0, int n, double s1,
                                       double s2, const MlpgTail& tl, double* o, int64_t ldo, bool store) {
  double kd = 0.0, k1 = 0.0, k2 = 0.0;
  if (CONST) {
    kd = c.fd[c.ncv * c.D];
    k1 = c.fl1[c.ncv * c.D];
    k2 = c.fl2[c.ncv * c.D];
  }
  double x1 = s1, x2 = s2;
#pragma unroll
  for (int i = FU_FL - 1; i >= 0; --i) {
    if (CONST || i < n) {
      const int64_t j = j0 + i;
      double dd, l1, l2;
      if (CONST) {
        dd = kd; l1 = k1; l2 = k2;
      } else if (j < c.n_shared) {
        const int64_t jc = (j < c.ncv ? j : c.ncv) * c.D;
        dd = c.fd[jc]; l1 = c.fl1[jc]; l2 = c.fl2[jc];
      } else {
        tl.get(j, c.prec.T, dd, l1, l2);
      }
      const double x = (b[i] - l1 * x1 - l2 * x2) * dd;
      if (store) o[j * ldo] = x;
      x2 = x1; x1 = x;
    }
  }
}

// b = W^T (mean / var) of the frames [j0, j0 + n) of one utterance (mlpg.py:123) for this lane's
// dimension; f: the lane's column in the utterance's first row, ld the row pitch, D the distance between a row's three
// pieces.  INTERIOR: rows j0-1 .. j0+FL all exist and none is an edge frame (no clamping, no edge variances).
template <int FU_FL, bool INTERIOR>
__device__ __forceinline__ void fu_form_b(const double* f, int64_t ld, int D, int64_t j0, int n, int64_t T,
                                          double v0, double v1, double v2, double (&b)[FU_FL]) {
  const double rv0 = 1.0 / v0, rv1 = 1.0 / v1, rv2 = 1.0 / v2;
  auto rowp = [&](int64_t r) { return f + (INTERIOR ? r : (r < 0 ? 0 : (r >= T ? T - 1 : r))) * ld; };
  double e1[FU_FL + 2], e2[FU_FL + 2];      // mean / var of rows j0-1 .. j0+FU_FL, windows 1 and 2 (0: no such row)
#pragma unroll
  for (int i = -1; i <= FU_FL; ++i) {
    const int64_t r = j0 + i;
    e1[i + 1] = e2[i + 1] = 0.0;
    if (INTERIOR || (i <= n && r >= 0 && r < T)) {
      e1[i + 1] = rowp(r)[D] * (INTERIOR ? rv1 : mlpg_rvar(r, T, rv1));
      e2[i + 1] = rowp(r)[2 * D] * (INTERIOR ? rv2 : mlpg_rvar(r, T, rv2));
    }
  }
#pragma unroll
  for (int i = 0; i < FU_FL; ++i)
    b[i] = (INTERIOR || i < n) ? mlpg_rhs_by_window(rowp(j0 + i)[0] * rv0, e1[i], e1[i + 2], e2[i], e2[i + 1], e2[i + 2]) : 0.0;
}

// ---- dependency-free solve: reduce -> scan -> solve ----------------------------------------------
// A kernel that reads the input once and hands states from workgroup to workgroup spends two thirds
// of its workgroups' life waiting (every wait ends with the slowest load among the waves it depends
// on) while their registers hold the chunk, and the registers bound how much of the batch is in
// flight: 15-19 % of the HBM peak at any batch size.  This form has no
// wait at all.  It rests on two facts: the forward sweep is linear in (b, entry state), and the
// chunk-local backward sweep x = L_cc^-T y has the adjoint form x_0 = (L_cc^-1 e_0) . y,
// x_1 = (L_cc^-1 e_1) . y -- so what the backward sweep of a chunk contributes to the chunk in
// front of it can be accumulated WHILE WALKING FORWARD, as two dot products with the forward
// impulse responses P = L_cc^-1 e_0 and R = L_cc^-1 e_1, without keeping y:
//   reduce  every chunk, from a zero entry state: e_f = (y0_{n-1}, y0_{n-2}), e_b0 = (P.y0, R.y0);
//           one streaming read of the input, four doubles out per (chunk, dimension), no state
//   scan    per (utterance, dimension): s_in(k+1) = M_f s_in(k) + e_f(k), then backwards
//           t_in(k-1) = M_b t_in(k) + e_b0(k) + C s_in(k); the matrices are data-independent --
//           M_f = the entry state's image (a combination of the last two P, R), M_b = the exit
//           state's image (P, R at the last two frames times the factor's off-diagonals),
//           C = [P R]^T [U V] from the Gram sums P.P, P.R, R.R -- one set per dimension for the
//           stationary chunks, recomputed in place for the few others (utterance start / tail)
//   solve   every chunk again, now from its true states: b read back from the output rows (where the
//           reduce kernel left it), y in registers, x stored over b
// HBM bytes per frame: 1496 (input once) + 3 x 496 (b out, b in, x out) + the aggregates (128 B per
// chunk and dimension, written and read once each) = 3.1 kB against 2000 algorithmic; measured with the
// halo rows and partial lines 4.4 kB (profiles/r4_section_traffic.json).
struct alignas(32) StRecord {
  long long t0;      // first frame of the utterance in the batch
  int T;             // its length
  int k0;            // first chunk of this group (index inside the utterance)
  int chunk;         // batch-wide index of that chunk
  int pad[3];
};

struct StreamArgs {
  MlpgArgs a;
  int t_max;
  const StRecord* rec;   // [n_groups] groups of ST_GW consecutive chunks of one utterance
  const int* chunk0;     // [U+1] batch-wide index of every utterance's first chunk
  int n_groups, nblk;
  double* agg;           // [n_chunks][4][Dp]: e_f (2), e_b0 (2)
  double* st;            // [n_chunks][4][Dp]: forward entry state (2), backward entry state (2)
  // the adjoint's mode of the reduce kernel only: b is the incoming gradient itself, dimension d in column gcol0 + d
  const void* gout;      // [Ttot, ld_gout] float32 or float64
  int64_t ld_gout;
  int gcol0;
};

// the incoming gradient of the adjoint's mode, as mlpg_stream_launch takes it (nullptr: the forward solve)
struct StGrad { const void* gout; bool f32; int64_t ld_gout; int gcol0; };

struct FuMats { double Mf[4], Mb[4], C[4]; };

// One forward walk over the chunk [j0, j0 + n) from a zero entry state, nothing kept.
// DATA: e = (y0_{n-1}, y0_{n-2}, P.y0, R.y0).  MATS: the chunk's data-independent matrices.
// PRELOAD (with !CONST): the chunk's factor rows are requested together before the walk instead of
// inside its (lane-divergent) branches -- one trip to memory per chunk instead of one per frame.
template <int FU_FL, bool CONST, bool DATA, bool MATS, bool PRELOAD = false>
__device__ __forceinline__ void fu_reduce(const FuFac& c, const double (&b)[FU_FL], int64_t j0, int n,
                                          MlpgTail& tl, double (&e)[4], FuMats& m) {
  double kd = 0.0, k1 = 0.0, k2 = 0.0;
  double l1p, l2p, cprev;
  // (in two halves: the scan kernel that uses this runs sixteen waves per workgroup, 128 registers each,
  // and 3 x 16 doubles of factor rows on top of the walk's state spilled -- 836 bytes of scratch per lane,
  // 14-17 us for the matrices of ONE chunk; two trips to memory instead of one, no spill)
  constexpr int PH = PRELOAD ? FU_FL / 2 : 1;
  double pd[PH], p1[PH], p2[PH];
  auto preload = [&](int h) {
#pragma unroll
    for (int i = 0; i < PH; ++i) {
      const int64_t j = j0 + h * PH + i;
      const int64_t jc = (j < c.ncv ? j : c.ncv) * c.D;      // always a valid row of the factor
      pd[i] = c.fd[jc]; p1[i] = c.fl1[jc]; p2[i] = c.fl2[jc];
    }
  };
  if (PRELOAD && !CONST) preload(0);
  if (CONST) {
    kd = c.fd[c.ncv * c.D];
    k1 = c.fl1[c.ncv * c.D];
    k2 = c.fl2[c.ncv * c.D];
    l1p = k1; l2p = k2; cprev = k2;
  } else {
    l1p = c.F(c.fl1, j0 - 1); l2p = c.F(c.fl2, j0 - 2); cprev = c.F(c.fl2, j0 - 1);
    if (c.n_shared == 0) l1p = l2p = cprev = 0.0;
  }
  double y1 = 0.0, y2 = 0.0, P1 = 0.0, P2 = 0.0, R1 = 0.0, R2 = 0.0;
  double spy = 0.0, sry = 0.0, spp = 0.0, spr = 0.0, srr = 0.0;
  double rho0u = 0.0, rho0v = 0.0, rho1u = 0.0;      // what the entry state adds to frames 0 and 1
  double l1_last = 0.0, l2_last = 0.0, l2_prev = 0.0;  // own factor entries of frames n-1 and n-2
  const int n_main = CONST ? FU_FL : fu_shared_frames(c, j0, n);
  // one step of the walk; `first` / `second`: frame 0 / 1 of the chunk
  auto step = [&](bool first, bool second, double dd, double l1, double l2, double bi) {
    if (first) { rho0u = -l1p; rho0v = -l2p; }
    if (second) rho1u = -l2p;
    const double P = ((first ? 1.0 : 0.0) - l1p * P1 - l2p * P2) * dd;
    const double R = ((second ? 1.0 : 0.0) - l1p * R1 - l2p * R2) * dd;
    if (DATA) {
      const double y = (bi - l1p * y1 - l2p * y2) * dd;
      spy += P * y; sry += R * y;
      y2 = y1; y1 = y;
    }
    if (MATS) { spp += P * P; spr += P * R; srr += R * R; }
    P2 = P1; P1 = P; R2 = R1; R1 = R;
    l2_prev = l2_last; l1_last = l1; l2_last = l2;
    l2p = cprev; l1p = l1; cprev = l2;
  };
#pragma unroll
  for (int i = 0; i < FU_FL; ++i) {
    if (PRELOAD && !CONST && i == PH) preload(1);
    if (CONST || i < n_main) {
      const int64_t j = j0 + i;
      double dd, l1, l2;
      if (CONST) {
        dd = kd; l1 = k1; l2 = k2;
      } else if (PRELOAD) {
        dd = pd[i % PH]; l1 = p1[i % PH]; l2 = p2[i % PH];
      } else {
        const int64_t jc = (j < c.ncv ? j : c.ncv) * c.D;
        dd = c.fd[jc]; l1 = c.fl1[jc]; l2 = c.fl2[jc];
      }
      step(i == 0, i == 1, dd, l1, l2, DATA ? b[i] : 0.0);
    }
  }
  if (!CONST) {      // the utterance's last two frames: factor re-derived (rolled: one copy)
#pragma unroll 1
    for (int i = n_main; i < n; ++i) {
      double dd, l1, l2;
      c.derive(j0 + i, l1p, l2p, cprev, dd, l1, l2, tl);
      double bi = 0.0;
      if (DATA) {
#pragma unroll
        for (int r = 0; r < FU_FL; ++r) bi = r == i ? b[r] : bi;
      }
      step(i == 0, i == 1, dd, l1, l2, bi);
    }
  }
  if (DATA) { e[0] = y1; e[1] = y2; e[2] = spy; e[3] = sry; }
  if (MATS) {
    m.Mf[0] = rho0u * P1 + rho1u * R1; m.Mf[1] = rho0v * P1;
    m.Mf[2] = rho0u * P2 + rho1u * R2; m.Mf[3] = rho0v * P2;
    m.Mb[0] = -l1_last * P1 - l2_prev * P2; m.Mb[1] = -l2_last * P1;
    m.Mb[2] = -l1_last * R1 - l2_prev * R2; m.Mb[3] = -l2_last * R1;
    m.C[0] = rho0u * spp + rho1u * spr; m.C[1] = rho0v * spp;
    m.C[2] = rho0u * spr + rho1u * srr; m.C[3] = rho0v * spr;
  }
}

// what the reduce and the solve kernel share: which chunk this wave owns, its lane's constants
template <int FU_FL>
struct StChunk {
  int64_t t0, T, j0, j1;
  int K, k, n, chunk, d;
  bool dok, cst;
  double v0, v1, v2;
  FuFac c;
  __device__ __forceinline__ bool open(const StreamArgs& g) {
    const MlpgArgs& a = g.a;
    const int grp = (int)(blockIdx.x / (unsigned)g.nblk), db = (int)(blockIdx.x % (unsigned)g.nblk);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const StRecord rec = g.rec[grp];
    t0 = rec.t0; T = rec.T;
    K = fu_num_chunks<FU_FL>(T);
    k = rec.k0 + w;
    const bool active = k < K;
    if (!active) k = K - 1;          // an idle wave computes on the last chunk's geometry and stores nothing
    chunk = rec.chunk + w;
    const int D = a.dim;
    dok = db * 64 + lane < D;
    d = dok ? db * 64 + lane : D - 1;
    j0 = fu_chunk_start<FU_FL>(k, K, T); j1 = fu_chunk_start<FU_FL>(k + 1, K, T);
    n = (int)(j1 - j0);
    v0 = a.var[d]; v1 = a.var[D + d]; v2 = a.var[2 * D + d];
    c.open(a, g.t_max, d, T, v0, v1, v2);
    const bool cst_lane = (j0 - 2 >= c.ncv) && (j1 <= c.n_shared) && n == FU_FL;
    cst = __all(cst_lane);
    return active;
  }
};

// Stages the rows [jlo, jhi) of one utterance -- the three 64-column pieces (static, delta,
// delta-delta) of this workgroup's dimension block -- into LDS as tile[row][w * 64 + lane], with
// every thread of the workgroup loading: the pieces of a row are contiguous in memory, so the loads
// are full-width (16 bytes per lane when the row pitch, the first column and the dimension count are
// even) and a row that two neighbouring chunks need is fetched once.  The waves then form b from
// LDS through fu_form_b with pitch ST_W.
constexpr int ST_W = 192;      // doubles per staged row
constexpr int ST_FL = 16;      // frames per chunk
constexpr int ST_GW = 2;       // chunks (= waves) per workgroup of the reduce kernel
constexpr int ST_GS = 4;       // chunks per workgroup of the solve kernel (no LDS there: four waves)

template <int NTHR, int MAXR>
__device__ __forceinline__ void st_stage_rows(const MlpgArgs& a, int db, int64_t t0, int64_t jlo, int rows,
                                              double* tile) {
  const int D = a.dim;
  const int dblk = D - db * 64 < 64 ? D - db * 64 : 64;
  const double* src0 = a.feat + (t0 + jlo) * a.ld_feat + a.col0 + db * 64;
  const bool wide = ((a.ld_feat | (int64_t)a.col0 | (int64_t)D) & 1) == 0 &&
                    (reinterpret_cast<uintptr_t>(a.feat) & 15) == 0;
  if (wide) {
    constexpr int CPR = 96;                               // 16-byte chunks per staged row
    constexpr int NLD = (MAXR * CPR + NTHR - 1) / NTHR;
    double2 v[NLD];
    const int total = rows * CPR;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = (int)threadIdx.x + i * NTHR;
      const int row = idx / CPR, rem = idx - row * CPR, w = rem >> 5, c = rem & 31;
      v[i] = make_double2(0.0, 0.0);
      if (idx < total && 2 * c < dblk)
        v[i] = *reinterpret_cast<const double2*>(src0 + (int64_t)row * a.ld_feat + w * D + 2 * c);
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = (int)threadIdx.x + i * NTHR;
      const int row = idx / CPR, rem = idx - row * CPR, w = rem >> 5, c = rem & 31;
      if (idx < total) *reinterpret_cast<double2*>(tile + row * ST_W + w * 64 + 2 * c) = v[i];
    }
  } else {
    constexpr int CPR = 192;
    constexpr int NLD = (MAXR * CPR + NTHR - 1) / NTHR;
    const int total = rows * CPR;
    for (int i0 = 0; i0 < NLD; i0 += 8) {
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int idx = (int)threadIdx.x + (i0 + i) * NTHR;
        const int row = idx / CPR, rem = idx - row * CPR, w = rem >> 6, c = rem & 63;
        v[i] = 0.0;
        if (idx < total && c < dblk) v[i] = src0[(int64_t)row * a.ld_feat + w * D + c];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int idx = (int)threadIdx.x + (i0 + i) * NTHR;
        const int row = idx / CPR, rem = idx - row * CPR, w = rem >> 6, c = rem & 63;
        if (idx < total) tile[row * ST_W + w * 64 + c] = v[i];
      }
    }
  }
}

// First launch of the stream path: the shared factor (blocks < nblk) and, beside it, one record per
// group of ST_GW (reduce kernel) and of ST_GS (solve kernel) chunks, expanded from the per-utterance tables
__global__ __launch_bounds__(64) void mlpg_prep_kernel(MlpgArgs a, int t_max, int nblk,
                                                       const int* __restrict__ chunk0,
                                                       const int* __restrict__ group_a,
                                                       const int* __restrict__ group_b,
                                                       StRecord* __restrict__ rec_a,
                                                       StRecord* __restrict__ rec_b) {
  if ((int)blockIdx.x < nblk) {        // the shared Cholesky factor of 64 dimensions
    mlpg_factor_block(a, t_max, blockIdx.x);
    return;
  }
  const int u = blockIdx.x - nblk;
  const int64_t t0 = a.offsets[u];
  const int T = (int)(a.offsets[u + 1] - t0);
  const int c0 = chunk0[u];
  const int a0 = group_a[u], na = group_a[u + 1] - a0;
  const int b0 = group_b[u], nb = group_b[u + 1] - b0;
  for (int i = threadIdx.x; i < na + nb; i += 64) {
    const bool second = i >= na;
    const int gi = second ? i - na : i, gw = second ? ST_GS : ST_GW;
    StRecord r{};
    r.t0 = t0;
    r.T = T;
    r.k0 = gi * gw;
    r.chunk = c0 + gi * gw;
    (second ? rec_b : rec_a)[(second ? b0 : a0) + gi] = r;
  }
}

// frames [jlo, jhi) a group of GW chunks starting at chunk k0 needs (one halo row on either side)
template <int FU_FL, int GW>
__device__ __forceinline__ void st_group_rows(const StRecord& rec, int64_t& jlo, int& rows) {
  const int64_t T = rec.T;
  const int K = fu_num_chunks<FU_FL>(T);
  const int kend = rec.k0 + GW < K ? rec.k0 + GW : K;
  jlo = fu_chunk_start<FU_FL>(rec.k0, K, T) - 1;
  if (jlo < 0) jlo = 0;
  int64_t jhi = fu_chunk_start<FU_FL>(kend, K, T) + 1;
  if (jhi > T) jhi = T;
  rows = (int)(jhi - jlo);
}

constexpr int ST_TILE_ROWS = ST_GW * ST_FL + 2;
static_assert(ST_TILE_ROWS * ST_W * sizeof(double) <= 64 * 1024, "the staged tile fits the default dynamic-LDS limit");

// TG = void: the forward solve, b formed from the three staged column blocks.  TG = float / double: the adjoint's
// mode, z = P^-1 g -- b is the incoming gradient itself (g.gout, widened in the load): a gradient row is D contiguous
// values, a wave's load of a frame is one segment already, so nothing is staged and no LDS is asked for.
template <typename TG>
__global__ __launch_bounds__(ST_GW * 64) void mlpg_reduce_kernel(StreamArgs g) {
  constexpr int FU_FL = ST_FL;
  constexpr bool ADJ = !std::is_void<TG>::value;
  const MlpgArgs& a = g.a;
  StChunk<FU_FL> q;
  const bool active = q.open(g);      // its loads (constants, factor) fly together with the staging loads
  double b[FU_FL];
  if constexpr (ADJ) {
    if (!active) return;
    using TL = typename std::conditional<ADJ, TG, double>::type;
    const TL* gin = static_cast<const TL*>(g.gout) + q.t0 * g.ld_gout + g.gcol0 + q.d;
#pragma unroll
    for (int i = 0; i < FU_FL; ++i) b[i] = (q.cst || i < q.n) ? (double)gin[(q.j0 + i) * g.ld_gout] : 0.0;
  } else {
    extern __shared__ __attribute__((aligned(16))) double st_tile[];
    int64_t jlo = 0;
    {
      const int grp = (int)(blockIdx.x / (unsigned)g.nblk), db = (int)(blockIdx.x % (unsigned)g.nblk);
      const StRecord rec = g.rec[grp];
      int rows;
      st_group_rows<FU_FL, ST_GW>(rec, jlo, rows);
      st_stage_rows<ST_GW * 64, ST_TILE_ROWS>(a, db, rec.t0, jlo, rows, st_tile);
      __syncthreads();
    }
    if (!active) return;
    const double* f = st_tile - jlo * ST_W + (threadIdx.x & 63);      // b from the staged rows: the tile's pitch and piece offsets
    if (q.cst) fu_form_b<FU_FL, true>(f, ST_W, 64, q.j0, q.n, q.T, q.v0, q.v1, q.v2, b);
    else fu_form_b<FU_FL, false>(f, ST_W, 64, q.j0, q.n, q.T, q.v0, q.v1, q.v2, b);
  }
  // b goes to the output rows: the solve kernel reads 496 B per frame from there instead of forming
  // b again from 1 488 B of input (and overwrites it with x, chunk by chunk, in place)
  if (q.dok) {
    double* o = a.out + q.t0 * a.ld_out + a.ocol0 + q.d;
#pragma unroll
    for (int i = 0; i < FU_FL; ++i)
      if (q.cst || i < q.n) o[(q.j0 + i) * a.ld_out] = b[i];
  }
  if (q.K == 1) return;               // a one-chunk utterance has nobody to hand a state to
  double e[4];
  MlpgTail tl;
  FuMats unused;
  if (q.cst) fu_reduce<FU_FL, true, true, false>(q.c, b, q.j0, q.n, tl, e, unused);
  else fu_reduce<FU_FL, false, true, false>(q.c, b, q.j0, q.n, tl, e, unused);
  if (q.dok) {
    const int64_t Dp = (int64_t)g.nblk * 64;
    double* o = g.agg + (int64_t)q.chunk * 4 * Dp + (blockIdx.x % (unsigned)g.nblk) * 64 + (threadIdx.x & 63);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[(int64_t)i * Dp] = e[i];
  }
}

// the data-independent matrices of chunk k of an utterance (any chunk; not inlined: the scan kernel
// calls it from many places and must stay small enough for the instruction cache)
template <int FU_FL>
__device__ __forceinline__ void st_chunk_mats(const FuFac& c, int K, int64_t T, int k, FuMats& m) {
  double none[FU_FL], e4[4];
  MlpgTail tl;
  const int64_t j0 = fu_chunk_start<FU_FL>(k, K, T), j1 = fu_chunk_start<FU_FL>(k + 1, K, T);
  fu_reduce<FU_FL, false, false, true, true>(c, none, j0, (int)(j1 - j0), tl, e4, m);
}

// The plain sequential scan of one (utterance, 64 dimensions) by one wave: the road the scan
// kernel takes when the factor settles so slowly that the utterance has more non-stationary
// leading chunks than the workgroup has waves to give them.  Correct for anything; not fast.
template <int FU_FL>
__device__ __noinline__ void st_scan_sequential(const FuFac& c, int K, int64_t T, const double* ag, double* st,
                                                int64_t Dp, bool dok) {
  auto lane_cst = [&](int k) {
    const int64_t j0 = fu_chunk_start<FU_FL>(k, K, T), j1 = fu_chunk_start<FU_FL>(k + 1, K, T);
    return (j0 - 2 >= c.ncv) && (j1 <= c.n_shared) && (int)(j1 - j0) == FU_FL;
  };
  FuMats mc;
  {
    double none[FU_FL], e4[4];
    MlpgTail tl;
    fu_reduce<FU_FL, true, false, true>(c, none, 0, FU_FL, tl, e4, mc);
  }
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < K; ++k) {
    if (dok) { st[((int64_t)k * 4 + 0) * Dp] = s1; st[((int64_t)k * 4 + 1) * Dp] = s2; }
    FuMats m = mc;
    if (!__all(lane_cst(k))) st_chunk_mats<FU_FL>(c, K, T, k, m);
    const double n1 = m.Mf[0] * s1 + m.Mf[1] * s2 + ag[((int64_t)k * 4 + 0) * Dp];
    const double n2 = m.Mf[2] * s1 + m.Mf[3] * s2 + ag[((int64_t)k * 4 + 1) * Dp];
    s1 = n1; s2 = n2;
  }
  double t1 = 0.0, t2 = 0.0;
  for (int k = K - 1; k >= 0; --k) {
    const double si0 = dok ? st[((int64_t)k * 4 + 0) * Dp] : 0.0, si1 = dok ? st[((int64_t)k * 4 + 1) * Dp] : 0.0;
    if (dok) { st[((int64_t)k * 4 + 2) * Dp] = t1; st[((int64_t)k * 4 + 3) * Dp] = t2; }
    FuMats m = mc;
    if (!__all(lane_cst(k))) st_chunk_mats<FU_FL>(c, K, T, k, m);
    const double e0 = ag[((int64_t)k * 4 + 2) * Dp] + m.C[0] * si0 + m.C[1] * si1;
    const double e1 = ag[((int64_t)k * 4 + 3) * Dp] + m.C[2] * si0 + m.C[3] * si1;
    const double n1 = m.Mb[0] * t1 + m.Mb[1] * t2 + e0;
    const double n2 = m.Mb[2] * t1 + m.Mb[3] * t2 + e1;
    t1 = n1; t2 = n2;
  }
}

// One workgroup per (utterance, 64 dimensions): the two affine recurrences over the utterance's
// chunks, as a two-level scan.  The chunks are cut into SW segments in time order, one per wave:
// every non-stationary chunk (the leading ones until all lanes' factors have settled, the last
// two) is a segment of its own, whose wave computes that chunk's matrices; the stationary middle
// is split evenly over the remaining waves, which only ever multiply by the one stationary set.
// A wave folds its segment into (A, q); the SW aggregates meet in LDS; every wave takes the state
// that enters its segment and walks the segment again, now storing.  The chain a wave runs is
// ~K / SW chunks long instead of K, and the aggregates of SB chunks are requested together.
constexpr int ST_SW = 16;      // waves (= segments) per workgroup of the scan kernel

__global__ __launch_bounds__(ST_SW * 64) void mlpg_scan_kernel(StreamArgs g) {
  constexpr int FU_FL = ST_FL;
  constexpr int SW = ST_SW;
  __shared__ double lds_s[SW][6][64];
  const MlpgArgs& a = g.a;
  const int u = (int)(blockIdx.x / (unsigned)g.nblk), db = (int)(blockIdx.x % (unsigned)g.nblk);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int D = a.dim;
  const bool dok = db * 64 + lane < D;
  const int d = dok ? db * 64 + lane : D - 1;
  const int64_t T = a.offsets[u + 1] - a.offsets[u];
  if (T <= 0) return;
  const int K = fu_num_chunks<FU_FL>(T);
  const int64_t Dp = (int64_t)g.nblk * 64;
  const int64_t col = (int64_t)db * 64 + lane;
  const int64_t base = g.chunk0[u];
  double* st = g.st + base * 4 * Dp + col;
  const double* ag = g.agg + base * 4 * Dp + col;
  if (K == 1) {
    if (dok && w == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) st[(int64_t)i * Dp] = 0.0;
    }
    return;
  }
  const double v0 = a.var[d], v1 = a.var[D + d], v2 = a.var[2 * D + d];
  FuFac c;
  c.open(a, g.t_max, d, T, v0, v1, v2);
  auto lane_cst = [&](int k) {
    const int64_t j0 = fu_chunk_start<FU_FL>(k, K, T), j1 = fu_chunk_start<FU_FL>(k + 1, K, T);
    return (j0 - 2 >= c.ncv) && (j1 <= c.n_shared) && (int)(j1 - j0) == FU_FL;
  };
  // segments: [0, n_lead) one leading chunk each | n_mid waves over [n_lead, tail0) | the last chunks
  int k_settled = 0;                      // first chunk that is stationary for every lane
  while (k_settled < K && !__all(lane_cst(k_settled))) ++k_settled;
  const int tail0 = K - 2 > 0 ? K - 2 : 0;
  const int n_tail = K - tail0;                                    // 1 or 2
  const int n_lead = k_settled < tail0 ? k_settled : tail0;
  if (n_lead > SW - n_tail - 1) {     // see st_scan_sequential
    if (w == 0) st_scan_sequential<FU_FL>(c, K, T, ag, st, Dp, dok);
    return;
  }
  const int n_mid = SW - n_lead - n_tail;
  const int mid_chunks = tail0 - n_lead;
  const int L = (mid_chunks + n_mid - 1) / (n_mid > 0 ? n_mid : 1);
  int k_lo, k_hi;                          // this wave's segment
  const bool single = w < n_lead || w >= n_lead + n_mid;
  if (w < n_lead) { k_lo = w; k_hi = w + 1; }
  else if (w >= n_lead + n_mid) { k_lo = tail0 + (w - n_lead - n_mid); k_hi = k_lo + 1; }
  else {
    const int mw = w - n_lead;
    k_lo = n_lead + mw * L; k_hi = k_lo + L;
    if (k_lo > tail0) k_lo = tail0;
    if (k_hi > tail0) k_hi = tail0;
  }
  FuMats mm;      // single-chunk wave: that chunk's matrices; middle wave: the stationary set
  if (single) {
    st_chunk_mats<FU_FL>(c, K, T, k_lo, mm);
  } else {
    double none[FU_FL], e4[4];
    MlpgTail tl;
    fu_reduce<FU_FL, true, false, true>(c, none, 0, FU_FL, tl, e4, mm);
  }
  auto mats = [&](int, FuMats& m) { m = mm; };
  constexpr int SB = 8;

  // ---- forward: s_in(k + 1) = M_f(k) s_in(k) + e_f(k)
  double A[4] = {1.0, 0.0, 0.0, 1.0}, q[2] = {0.0, 0.0};
  for (int kb = k_lo; kb < k_hi; kb += SB) {
    double ef[SB][2];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      const int k = kb + i < k_hi ? kb + i : k_hi - 1;
      ef[i][0] = ag[((int64_t)k * 4 + 0) * Dp];
      ef[i][1] = ag[((int64_t)k * 4 + 1) * Dp];
    }
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      if (kb + i < k_hi) {
        FuMats m;
        mats(kb + i, m);
        const double a0 = m.Mf[0] * A[0] + m.Mf[1] * A[2], a1 = m.Mf[0] * A[1] + m.Mf[1] * A[3];
        const double a2 = m.Mf[2] * A[0] + m.Mf[3] * A[2], a3 = m.Mf[2] * A[1] + m.Mf[3] * A[3];
        const double q0 = m.Mf[0] * q[0] + m.Mf[1] * q[1] + ef[i][0];
        const double q1 = m.Mf[2] * q[0] + m.Mf[3] * q[1] + ef[i][1];
        A[0] = a0; A[1] = a1; A[2] = a2; A[3] = a3; q[0] = q0; q[1] = q1;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) lds_s[w][i][lane] = A[i];
  lds_s[w][4][lane] = q[0];
  lds_s[w][5][lane] = q[1];
  __syncthreads();
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < w; ++i) {
    const double n1 = lds_s[i][0][lane] * s1 + lds_s[i][1][lane] * s2 + lds_s[i][4][lane];
    const double n2 = lds_s[i][2][lane] * s1 + lds_s[i][3][lane] * s2 + lds_s[i][5][lane];
    s1 = n1; s2 = n2;
  }
  for (int kb = k_lo; kb < k_hi; kb += SB) {
    double ef[SB][2];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      const int k = kb + i < k_hi ? kb + i : k_hi - 1;
      ef[i][0] = ag[((int64_t)k * 4 + 0) * Dp];
      ef[i][1] = ag[((int64_t)k * 4 + 1) * Dp];
    }
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      const int k = kb + i;
      if (k < k_hi) {
        if (dok) { st[((int64_t)k * 4 + 0) * Dp] = s1; st[((int64_t)k * 4 + 1) * Dp] = s2; }
        FuMats m;
        mats(k, m);
        const double n1 = m.Mf[0] * s1 + m.Mf[1] * s2 + ef[i][0];
        const double n2 = m.Mf[2] * s1 + m.Mf[3] * s2 + ef[i][1];
        s1 = n1; s2 = n2;
      }
    }
  }
  // ---- backward: t_in(k - 1) = M_b(k) t_in(k) + e_b0(k) + C(k) s_in(k)
  // (a lane reads back the s_in it stored above: same thread, same address, program order)
  A[0] = 1.0; A[1] = 0.0; A[2] = 0.0; A[3] = 1.0; q[0] = q[1] = 0.0;
  for (int kb = k_hi - 1; kb >= k_lo; kb -= SB) {
    double eb[SB][2], si[SB][2];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      const int k = kb - i >= k_lo ? kb - i : k_lo;
      eb[i][0] = ag[((int64_t)k * 4 + 2) * Dp];
      eb[i][1] = ag[((int64_t)k * 4 + 3) * Dp];
      si[i][0] = dok ? st[((int64_t)k * 4 + 0) * Dp] : 0.0;
      si[i][1] = dok ? st[((int64_t)k * 4 + 1) * Dp] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      if (kb - i >= k_lo) {
        FuMats m;
        mats(kb - i, m);
        const double e0 = eb[i][0] + m.C[0] * si[i][0] + m.C[1] * si[i][1];
        const double e1 = eb[i][1] + m.C[2] * si[i][0] + m.C[3] * si[i][1];
        const double a0 = m.Mb[0] * A[0] + m.Mb[1] * A[2], a1 = m.Mb[0] * A[1] + m.Mb[1] * A[3];
        const double a2 = m.Mb[2] * A[0] + m.Mb[3] * A[2], a3 = m.Mb[2] * A[1] + m.Mb[3] * A[3];
        const double q0 = m.Mb[0] * q[0] + m.Mb[1] * q[1] + e0;
        const double q1 = m.Mb[2] * q[0] + m.Mb[3] * q[1] + e1;
        A[0] = a0; A[1] = a1; A[2] = a2; A[3] = a3; q[0] = q0; q[1] = q1;
      }
    }
  }
  __syncthreads();      // every wave has read the forward segment aggregates
#pragma unroll
  for (int i = 0; i < 4; ++i) lds_s[w][i][lane] = A[i];
  lds_s[w][4][lane] = q[0];
  lds_s[w][5][lane] = q[1];
  __syncthreads();
  double t1 = 0.0, t2 = 0.0;
  for (int i = SW - 1; i > w; --i) {
    const double n1 = lds_s[i][0][lane] * t1 + lds_s[i][1][lane] * t2 + lds_s[i][4][lane];
    const double n2 = lds_s[i][2][lane] * t1 + lds_s[i][3][lane] * t2 + lds_s[i][5][lane];
    t1 = n1; t2 = n2;
  }
  for (int kb = k_hi - 1; kb >= k_lo; kb -= SB) {
    double eb[SB][2], si[SB][2];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      const int k = kb - i >= k_lo ? kb - i : k_lo;
      eb[i][0] = ag[((int64_t)k * 4 + 2) * Dp];
      eb[i][1] = ag[((int64_t)k * 4 + 3) * Dp];
      si[i][0] = dok ? st[((int64_t)k * 4 + 0) * Dp] : 0.0;
      si[i][1] = dok ? st[((int64_t)k * 4 + 1) * Dp] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      const int k = kb - i;
      if (k >= k_lo) {
        if (dok) { st[((int64_t)k * 4 + 2) * Dp] = t1; st[((int64_t)k * 4 + 3) * Dp] = t2; }
        FuMats m;
        mats(k, m);
        const double e0 = eb[i][0] + m.C[0] * si[i][0] + m.C[1] * si[i][1];
        const double e1 = eb[i][1] + m.C[2] * si[i][0] + m.C[3] * si[i][1];
        const double n1 = m.Mb[0] * t1 + m.Mb[1] * t2 + e0;
        const double n2 = m.Mb[2] * t1 + m.Mb[3] * t2 + e1;
        t1 = n1; t2 = n2;
      }
    }
  }
}

__global__ __launch_bounds__(ST_GS * 64) void mlpg_solve_kernel(StreamArgs g) {
  constexpr int FU_FL = ST_FL;
  const MlpgArgs& a = g.a;
  StChunk<FU_FL> q;
  if (!q.open(g)) return;
  const int64_t Dp = (int64_t)g.nblk * 64;
  const double* st = g.st + (int64_t)q.chunk * 4 * Dp + (blockIdx.x % (unsigned)g.nblk) * 64 + (threadIdx.x & 63);
  const double s1 = st[0], s2 = st[Dp], t1 = st[2 * Dp], t2 = st[3 * Dp];
  double* o = a.out + q.t0 * a.ld_out + a.ocol0 + q.d;
  double b[FU_FL];      // left in the output rows by the reduce kernel
#pragma unroll
  for (int i = 0; i < FU_FL; ++i) b[i] = (q.cst || i < q.n) ? o[(q.j0 + i) * a.ld_out] : 0.0;
  MlpgTail tl;
  if (q.cst) {
    fu_fwd<FU_FL, true>(q.c, b, q.j0, q.n, s1, s2, tl);
    fu_bwd<FU_FL, true>(q.c, b, q.j0, q.n, t1, t2, tl, o, a.ld_out, q.dok);
  } else {
    fu_fwd<FU_FL, false>(q.c, b, q.j0, q.n, s1, s2, tl);
    fu_bwd<FU_FL, false>(q.c, b, q.j0, q.n, t1, t2, tl, o, a.ld_out, q.dok);
  }
}

// reduce -> scan -> solve (see above).  grad: the adjoint's mode (the reduce kernel takes b from it, a.feat is not read;
// a.out is then the z plane).  after(g): queued behind the solve, while the records (g.rec: the solve kernel's groups of
// ST_GS chunks) and the offsets are still there.
template <typename After>
static int mlpg_stream_launch(MlpgArgs a, const int64_t* h_offsets, int n_utts, int dim, int64_t t_max,
                              ScratchScope& scratch, const StGrad* grad, After after) {
  hipStream_t s = scratch.stream();
  // per utterance: first chunk and first group (batch-wide indices); the per-group records are
  // expanded from them on the device (at 4 096 utterances the host would otherwise build and
  // upload 2.4 - 4.9 MB of records per call)
  constexpr int FL = ST_FL, GW = ST_GW, GS = ST_GS;
  std::vector<int> tab(3 * (size_t)(n_utts + 1), 0);
  int* chunk0 = tab.data();
  int* group0 = tab.data() + (n_utts + 1);
  int* sgroup0 = tab.data() + 2 * (n_utts + 1);
  int n_chunks = 0, n_groups = 0, n_sgroups = 0;
  for (int u = 0; u < n_utts; ++u) {
    const int64_t T = h_offsets[u + 1] - h_offsets[u];
    chunk0[u] = n_chunks;
    group0[u] = n_groups;
    sgroup0[u] = n_sgroups;
    const int K = T > 0 ? fu_num_chunks<FL>(T) : 0;
    n_chunks += K;
    n_groups += (K + GW - 1) / GW;
    n_sgroups += (K + GS - 1) / GS;
  }
  chunk0[n_utts] = n_chunks;
  group0[n_utts] = n_groups;
  sgroup0[n_utts] = n_sgroups;
  const int nblk = (dim + 63) / 64;
  const size_t rrec_bytes = (size_t)n_groups * sizeof(StRecord);
  const size_t rec_bytes = rrec_bytes + (size_t)n_sgroups * sizeof(StRecord);
  // [records | offsets (int64) | chunk / group tables (int) | aggregates | entry states]; offsets and
  // tables travel in ONE upload
  const size_t off_bytes = ((size_t)(n_utts + 1) * sizeof(int64_t) + 31) / 32 * 32;
  const size_t c0_bytes = off_bytes + (tab.size() * sizeof(int) + 31) / 32 * 32;
  const size_t plane_bytes = (size_t)n_chunks * 4 * nblk * 64 * sizeof(double);
  char* blk = nullptr;
  ITTS_HIP_CHECK(scratch.take(&blk, rec_bytes + c0_bytes + 2 * plane_bytes));
  {
    std::vector<char> host(off_bytes + tab.size() * sizeof(int), 0);
    std::memcpy(host.data(), h_offsets, (size_t)(n_utts + 1) * sizeof(int64_t));
    std::memcpy(host.data() + off_bytes, tab.data(), tab.size() * sizeof(int));
    const int rc = itts::staged_upload(blk + rec_bytes, host.data(), host.size(), s);
    if (rc) return rc;
  }
  a.offsets = reinterpret_cast<const int64_t*>(blk + rec_bytes);
  const int* d_tab = reinterpret_cast<const int*>(blk + rec_bytes + off_bytes);
  hipLaunchKernelGGL(mlpg_prep_kernel, dim3((unsigned)(nblk + n_utts)), dim3(64), 0, s, a, (int)t_max,
                     nblk, d_tab, d_tab + (n_utts + 1), d_tab + 2 * (n_utts + 1),
                     reinterpret_cast<StRecord*>(blk), reinterpret_cast<StRecord*>(blk + rrec_bytes));
  StreamArgs g;
  g.a = a;
  g.t_max = (int)t_max;
  g.rec = reinterpret_cast<const StRecord*>(blk);
  g.chunk0 = d_tab;
  g.n_groups = n_groups;
  g.nblk = nblk;
  g.agg = reinterpret_cast<double*>(blk + rec_bytes + c0_bytes);
  g.st = g.agg + plane_bytes / sizeof(double);
  g.gout = grad ? grad->gout : nullptr;
  g.ld_gout = grad ? grad->ld_gout : 0;
  g.gcol0 = grad ? grad->gcol0 : 0;
  const dim3 grid((unsigned)((size_t)n_groups * nblk));
  const size_t tile_bytes = (size_t)ST_TILE_ROWS * ST_W * sizeof(double);
  if (!grad) hipLaunchKernelGGL(mlpg_reduce_kernel<void>, grid, dim3(GW * 64), tile_bytes, s, g);
  else if (grad->f32) hipLaunchKernelGGL(mlpg_reduce_kernel<float>, grid, dim3(GW * 64), 0, s, g);
  else hipLaunchKernelGGL(mlpg_reduce_kernel<double>, grid, dim3(GW * 64), 0, s, g);
  hipLaunchKernelGGL(mlpg_scan_kernel, dim3((unsigned)(n_utts * nblk)), dim3(ST_SW * 64), 0, s, g);
  g.rec = reinterpret_cast<const StRecord*>(blk + rrec_bytes);
  g.n_groups = n_sgroups;
  hipLaunchKernelGGL(mlpg_solve_kernel, dim3((unsigned)((size_t)n_sgroups * nblk)), dim3(GS * 64), 0, s,
                     g);
  after(g);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

static int mlpg_stream_launch(MlpgArgs a, const int64_t* h_offsets, int n_utts, int dim, int64_t t_max,
                              ScratchScope& scratch) {
  return mlpg_stream_launch(a, h_offsets, n_utts, dim, t_max, scratch, nullptr, [](const StreamArgs&) {});
}

}  // namespace itts
