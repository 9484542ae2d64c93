// MLPG, the sequential form: the shared Cholesky factor (mlpg_factor_kernel) and the two sweeps frame by frame
// (mlpg_kernel), for batches of short utterances.  Included by mlpg.hip only.
#pragma once
#include "mlpg_math.h"

namespace itts {

// The Cholesky factor of P depends on the variances and on the frame index only (not on the
// data), and -- because the delta variances are constant except in the first and last frame --
// it is the SAME for every utterance up to frame T-3.  mlpg_factor_kernel computes that shared
// factor once per dimension for the longest utterance ("T = infinity": edge variance at frame 0
// only); the per-utterance solve reads it and only re-derives the last two frames.  The solve is
// then two first-order-dependent sweeps of ~3 FMAs per frame instead of a sqrt and three
// divisions per frame in the dependency chain.
__device__ __forceinline__ void mlpg_factor_block(const MlpgArgs& a, int t_max, int block) {
  const int d = block * 64 + threadIdx.x;
  if (d >= a.dim) return;
  const int D = a.dim;
  const double v0 = a.var[d], v1 = a.var[D + d], v2 = a.var[2 * D + d];
  const MlpgPrec<int> prec{0, 1.0 / v0, 1.0 / v1, 1.0 / v2};
  const int64_t plane = (int64_t)t_max * D;
  double* fd = a.scratch + d;
  double* fl1 = fd + plane;
  double* fl2 = fl1 + plane;
  double l1p = 0.0, l2p = 0.0, cprev = 0.0;
  int j = 0;
  for (; j < t_max; ++j) {
    // this loop is a pure latency chain (one wave per 64 dimensions) in front of every solve
    double inv, l1, l2;
    mlpg_chol_step<true>(prec.row<true>(j), l1p, l2p, cprev, inv, l1, l2);
    fd[(int64_t)j * D] = inv;        // reciprocal: the solve multiplies instead of dividing
    fl1[(int64_t)j * D] = l1;
    fl2[(int64_t)j * D] = l2;
    // once the state repeats: stop (the solve clamps its factor index to this frame; later frames reuse this factor)
    const bool fixed = mlpg_factor_settled(j, l1, l2, l1p, l2p, cprev);
    l2p = cprev;
    l1p = l1;
    cprev = l2;
    if (fixed) break;
  }
  a.nconv[d] = j < t_max ? j : t_max - 1;
}

__global__ __launch_bounds__(64) void mlpg_factor_kernel(MlpgArgs a, int t_max) {
  mlpg_factor_block(a, t_max, blockIdx.x);
}

// Latency-bound sequential sweeps: what limits throughput is the number of independent chains in
// flight, so a workgroup carries only LANES (16) dimensions -- a quarter-filled wave per
// workgroup, 128-B row segments -- which quadruples the waves (and outstanding loads) per batch.
constexpr int MLPG_LANES = 16;
__global__ __launch_bounds__(MLPG_LANES) void mlpg_kernel(MlpgArgs a, int t_max) {
  const int d = blockIdx.x * MLPG_LANES + threadIdx.x;
  const int u = blockIdx.y;
  if (d >= a.dim) return;
  const int64_t t0 = a.offsets[u];
  const int64_t T = a.offsets[u + 1] - t0;
  if (T <= 0) return;
  const int D = a.dim;
  const double v0 = a.var[d], v1 = a.var[D + d], v2 = a.var[2 * D + d];
  const MlpgPrec<int64_t> prec{T, 1.0 / v0, 1.0 / v1, 1.0 / v2};

  const double* f = a.feat + t0 * a.ld_feat + a.col0 + d;
  double* o = a.out + t0 * a.ld_out + a.ocol0 + d;
  const int64_t plane = (int64_t)t_max * D;
  const double* fd = a.scratch + d;
  const double* fl1 = fd + plane;
  const double* fl2 = fl1 + plane;

  const int64_t ncv = a.nconv[d];
  const double rv0 = 1.0 / v0, rv1 = 1.0 / v1, rv2 = 1.0 / v2;
  // factor of frame j: shared for j <= T-3, re-derived with the true edge variances for the last two frames
  MlpgTail tail;
  const int64_t n_shared = T >= 3 ? T - 2 : 0;

  // b-frames (mean / var, mlpg.py:123) of rows j-1, j, j+1 for windows 1 and 2.
  double p1 = 0.0, p2 = 0.0;  // row j-1
  double c0, c1, c2;          // row j
  c0 = f[0] * rv0;
  c1 = f[D] * mlpg_rvar<double, int64_t>(0, T, rv1);
  c2 = f[2 * D] * mlpg_rvar<double, int64_t>(0, T, rv2);
  // Cholesky state: row j entries L[j,j-1], L[j,j-2]; y[j-1], y[j-2]
  double l1p = 0.0, l2p = 0.0, cprev = 0.0, y1 = 0.0, y2 = 0.0;

  constexpr int PF = 8;  // rows prefetched ahead of the recurrence
  double nb0[PF], nb1[PF], nb2[PF], nd[PF], nl1[PF], nl2[PF];
  auto load_block = [&](int64_t jb, double (&b0)[PF], double (&b1)[PF], double (&b2)[PF],
                        double (&bd)[PF], double (&bl1)[PF], double (&bl2)[PF]) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t t = jb + 1 + i;  // mean row j+1
      const int64_t tc = t < T ? t : T - 1;
      const double* r = f + tc * a.ld_feat;
      b0[i] = r[0];
      b1[i] = r[D];
      b2[i] = r[2 * D];
      const int64_t j = jb + i;      // factor of frame j
      const int64_t jc = j < n_shared ? (j < ncv ? j : ncv) : 0;
      bd[i] = fd[jc * D];
      bl1[i] = fl1[jc * D];
      bl2[i] = fl2[jc * D];
    }
  };
  load_block(0, nb0, nb1, nb2, nd, nl1, nl2);

  for (int64_t jb = 0; jb < T; jb += PF) {
    // issue the loads of the next block before touching the recurrence
    double fb0[PF], fb1[PF], fb2[PF], fbd[PF], fbl1[PF], fbl2[PF];
    load_block(jb + PF, fb0, fb1, fb2, fbd, fbl1, fbl2);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t j = jb + i;
      if (j < T) {
        double n0 = 0.0, n1 = 0.0, n2 = 0.0;
        if (j + 1 < T) {
          n0 = nb0[i] * rv0;
          n1 = nb1[i] * mlpg_rvar(j + 1, T, rv1);
          n2 = nb2[i] * mlpg_rvar(j + 1, T, rv2);
        }
        const double b = mlpg_rhs(c0, p1, n1, p2, c2, n2);
        double dd, l1, l2;  // dd holds 1 / L[j,j]
        if (j < n_shared) {
          dd = nd[i];
          l1 = nl1[i];
          l2 = nl2[i];
        } else {
          mlpg_chol_step<false>(prec.row<false>(j), l1p, l2p, cprev, dd, l1, l2);
          tail.put(j, T, dd, l1, l2);
        }
        const double y = (b - l1p * y1 - l2p * y2) * dd;
        o[j * a.ld_out] = y;
        // advance to row j+1
        l2p = cprev;  // L[j+1,j-1]
        l1p = l1;
        cprev = l2;
        y2 = y1;
        y1 = y;
        p1 = c1;
        p2 = c2;
        c0 = n0;
        c1 = n1;
        c2 = n2;
      }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      nb0[i] = fb0[i]; nb1[i] = fb1[i]; nb2[i] = fb2[i];
      nd[i] = fbd[i]; nl1[i] = fbl1[i]; nl2[i] = fbl2[i];
    }
  }

  // backward substitution L^T x = y
  double x1 = 0.0, x2 = 0.0;
  for (int64_t jb = T - 1; jb >= 0; jb -= PF) {
    double rd[PF], r1[PF], r2[PF], ry[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t j = jb - i;
      if (j >= 0) {
        const int64_t jc = j < n_shared ? (j < ncv ? j : ncv) : 0;
        rd[i] = fd[jc * D];
        r1[i] = fl1[jc * D];
        r2[i] = fl2[jc * D];
        ry[i] = o[j * a.ld_out];
        if (j >= n_shared) tail.get(j, T, rd[i], r1[i], r2[i]);
      } else {
        rd[i] = 1.0;
        r1[i] = r2[i] = ry[i] = 0.0;
      }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t j = jb - i;
      if (j >= 0) {
        const double x = (ry[i] - r1[i] * x1 - r2[i] * x2) * rd[i];
        o[j * a.ld_out] = x;
        x2 = x1;
        x1 = x;
      }
    }
  }
}

}  // namespace itts
