// MLPG, the adjoint: the gradient of a loss with respect to the static / delta / delta-delta means, given its gradient
// with respect to the trajectory.  For fixed variances the trajectory is linear in the means,
//   c = P^-1 sum_w W_w^T (tau_w o mu_w),
// and P is symmetric, so   z = P^-1 g   (one more solve with the SAME factor, right-hand side g itself) and
//   dL/dmu_0[t] = tau_0     z[t]
//   dL/dmu_1[t] = tau_1(t)  0.5 (z[t+1] - z[t-1])
//   dL/dmu_2[t] = tau_2(t)  (z[t-1] - 2 z[t] + z[t+1])          (z outside the utterance counts as 0)
// with tau_w(t) = mlpg_rvar: 1 / var_w, or 1 / kBigVar in the first and last frame for w = 1, 2.
// Two forms, chosen as the forward chooses (mlpg.hip):
//   sweeps  mlpg_adjoint_kernel, modelled on the sequential form (mlpg_kernel, mlpg_sweeps.h): the shared factor planes
//           of mlpg_factor_kernel, the last two frames re-derived (MlpgTail), the windows inside the back-substitution;
//           batches whose longest utterance is under MLPG_SEQ_BELOW frames
//   stream  the forward's prep -> reduce -> scan -> solve (mlpg_stream.h) with the reduce kernel in its adjoint mode
//           (b = g), z left in the plane the sweeps keep y in, then mlpg_adjoint_window_kernel: one pointwise launch
//           that reads rows t-1, t, t+1 of z and stores the three columns of row t
// Included by mlpg.hip only.
#pragma once
#include "mlpg_math.h"
#include "mlpg_stream.h"

namespace itts {

struct MlpgAdjointArgs {
  MlpgArgs a;             // var, offsets, scratch (factor planes), nconv, dim: what mlpg_factor_kernel and the sweeps read
  const void* gout;       // [Ttot, ld_gout] TI: dL/dc of dimension d in column gcol0 + d
  int64_t ld_gout;
  int gcol0;
  void* gfeat;            // [Ttot, ld_gfeat] TO: dL/dmu_w of dimension d in column col0 + w dim + d
  int64_t ld_gfeat;
  int col0;
  double* y;              // [Ttot, dim]: the forward sweep's intermediate (sweeps); z (stream)
};

// As latency-bound as mlpg_kernel (two first-order chains of ~3 dependent FMAs a frame), so the same geometry: 16
// dimensions a workgroup -- a 60-dimension stream of 64 utterances is 256 quarter-filled waves, one per compute unit,
// instead of 64 full ones on a quarter of the chip -- and the rows of the next 8 frames requested before the
// recurrence touches the current 8, in both sweeps.  Measured: about 0.24 us a frame and sweep
// whatever the width, one memory round trip per block -- fine under the forward's 194 frames, 0.75 ms a launch at
// 1 600; long utterances want the stream form's division of an utterance among workgroups, not a deeper prefetch.
constexpr int MLPG_ADJ_LANES = 16;
constexpr int MLPG_ADJ_PF = 8;

// grid: (utterance, block of MLPG_ADJ_LANES dimensions).  TI: type of the incoming gradient, TO: of the one written;
// all arithmetic in double, TO rounded once at the store.
template <typename TI, typename TO>
__global__ __launch_bounds__(MLPG_ADJ_LANES) void mlpg_adjoint_kernel(MlpgAdjointArgs g, int t_max) {
  const MlpgArgs& a = g.a;
  const int d = blockIdx.y * MLPG_ADJ_LANES + threadIdx.x;
  const int u = blockIdx.x;
  if (d >= a.dim) return;
  const int64_t t0 = a.offsets[u];
  const int64_t T = a.offsets[u + 1] - t0;
  if (T <= 0) return;
  const int D = a.dim;
  const double v0 = a.var[d], v1 = a.var[D + d], v2 = a.var[2 * D + d];
  const double rv0 = 1.0 / v0, rv1 = 1.0 / v1, rv2 = 1.0 / v2;
  const MlpgPrec<int64_t> prec{T, rv0, rv1, rv2};

  const TI* gin = static_cast<const TI*>(g.gout) + t0 * g.ld_gout + g.gcol0 + d;
  TO* o = static_cast<TO*>(g.gfeat) + t0 * g.ld_gfeat + g.col0 + d;
  double* yy = g.y + t0 * D + d;
  const int64_t plane = (int64_t)t_max * D;
  const double* fd = a.scratch + d;
  const double* fl1 = fd + plane;
  const double* fl2 = fl1 + plane;
  const int64_t ncv = a.nconv[d];
  // factor of frame j: shared for j <= T-3, re-derived with the true edge variances for the last two frames
  MlpgTail tail;
  const int64_t n_shared = T >= 3 ? T - 2 : 0;
  constexpr int PF = MLPG_ADJ_PF;

  // ---- forward substitution L y = g --------------------------------------------------------------------------------
  double l1p = 0.0, l2p = 0.0, cprev = 0.0, y1 = 0.0, y2 = 0.0;
  double nb[PF], nd[PF], nl1[PF], nl2[PF];
  auto load_fwd = [&](int64_t jb, double (&b)[PF], double (&bd)[PF], double (&bl1)[PF], double (&bl2)[PF]) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t j = jb + i;
      const int64_t tc = j < T ? j : T - 1;
      b[i] = (double)gin[tc * g.ld_gout];
      const int64_t jc = j < n_shared ? (j < ncv ? j : ncv) : 0;
      bd[i] = fd[jc * D];
      bl1[i] = fl1[jc * D];
      bl2[i] = fl2[jc * D];
    }
  };
  load_fwd(0, nb, nd, nl1, nl2);
  for (int64_t jb = 0; jb < T; jb += PF) {
    double fb[PF], fbd[PF], fbl1[PF], fbl2[PF];
    load_fwd(jb + PF, fb, fbd, fbl1, fbl2);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t j = jb + i;
      if (j < T) {
        double dd, l1, l2;  // dd holds 1 / L[j,j]
        if (j < n_shared) {
          dd = nd[i];
          l1 = nl1[i];
          l2 = nl2[i];
        } else {
          mlpg_chol_step<false>(prec.row<false>(j), l1p, l2p, cprev, dd, l1, l2);
          tail.put(j, T, dd, l1, l2);
        }
        const double y = (nb[i] - l1p * y1 - l2p * y2) * dd;
        yy[j * D] = y;
        l2p = cprev;
        l1p = l1;
        cprev = l2;
        y2 = y1;
        y1 = y;
      }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      nb[i] = fb[i]; nd[i] = fbd[i]; nl1[i] = fbl1[i]; nl2[i] = fbl2[i];
    }
  }

  // ---- backward substitution L^T z = y with the windows fused: z[j] completes gradient row j+1 --------------------
  // steps j = T-1 .. -1 (z[-1] = 0 completes row 0); z, z1, z2 = z[j], z[j+1], z[j+2]
  double rd[PF], r1[PF], r2[PF], ry[PF];
  auto load_bwd = [&](int64_t jb, double (&bd)[PF], double (&b1)[PF], double (&b2)[PF], double (&by)[PF]) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t j = jb - i;
      const int64_t jr = j > 0 ? j : 0;      // (rows past the start: loaded in bounds, never used)
      const int64_t jc = jr < n_shared ? (jr < ncv ? jr : ncv) : 0;
      bd[i] = fd[jc * D];
      b1[i] = fl1[jc * D];
      b2[i] = fl2[jc * D];
      by[i] = yy[jr * D];
      if (jr >= n_shared) tail.get(jr, T, bd[i], b1[i], b2[i]);
    }
  };
  load_bwd(T - 1, rd, r1, r2, ry);
  double z1 = 0.0, z2 = 0.0;
  for (int64_t jb = T - 1; jb >= -1; jb -= PF) {
    double pd[PF], p1[PF], p2[PF], py[PF];
    load_bwd(jb - PF, pd, p1, p2, py);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int64_t j = jb - i;
      if (j >= -1) {
        const double z = j >= 0 ? (ry[i] - r1[i] * z1 - r2[i] * z2) * rd[i] : 0.0;
        const int64_t r = j + 1;
        if (r < T) {
          TO* row = o + r * g.ld_gfeat;
          row[0] = (TO)(rv0 * z1);
          row[D] = (TO)(mlpg_rvar(r, T, rv1) * (0.5 * (z2 - z)));
          row[2 * D] = (TO)(mlpg_rvar(r, T, rv2) * (z - 2.0 * z1 + z2));
        }
        z2 = z1;
        z1 = z;
      }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      rd[i] = pd[i]; r1[i] = p1[i]; r2[i] = p2[i]; ry[i] = py[i];
    }
  }
}

// ---- the stream form ------------------------------------------------------------------------------------------------
// The three windows over the z plane (g.a.out, pitch g.a.ld_out) the solve kernel left.  Same grid as the solve kernel:
// one workgroup per (group of ST_GS chunks, 64 dimensions), g.rec its records; a wave takes the 16 frames
// [(k0 + w) 16, ..) of its utterance (the pointwise pass has no use for the last chunk's borrowed frame), reads them
// and one row on either side -- 0 outside the utterance -- and stores 3 values a frame in the destination type.
template <typename TO>
__global__ __launch_bounds__(ST_GS * 64) void mlpg_adjoint_window_kernel(StreamArgs g, void* gfeat, int64_t ld_gfeat,
                                                                         int col0) {
  constexpr int FL = ST_FL;
  const MlpgArgs& a = g.a;
  const int grp = (int)(blockIdx.x / (unsigned)g.nblk), db = (int)(blockIdx.x % (unsigned)g.nblk);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int D = a.dim, d = db * 64 + lane;
  if (d >= D) return;
  const StRecord rec = g.rec[grp];
  const int64_t T = rec.T;
  const int64_t j0 = (int64_t)(rec.k0 + w) * FL;
  if (j0 >= T) return;
  const int n = T - j0 < FL ? (int)(T - j0) : FL;
  const double rv0 = 1.0 / a.var[d], rv1 = 1.0 / a.var[D + d], rv2 = 1.0 / a.var[2 * D + d];
  const double* z = a.out + (rec.t0 + j0) * a.ld_out + a.ocol0 + d;
  double zz[FL + 2];      // z of rows j0-1 .. j0+FL
#pragma unroll
  for (int i = -1; i <= FL; ++i) {
    const int64_t r = j0 + i;
    zz[i + 1] = (i <= n && r >= 0 && r < T) ? z[(int64_t)i * a.ld_out] : 0.0;
  }
  TO* o = static_cast<TO*>(gfeat) + (rec.t0 + j0) * ld_gfeat + col0 + d;
#pragma unroll
  for (int i = 0; i < FL; ++i) {
    if (i < n) {
      const int64_t r = j0 + i;
      TO* row = o + (int64_t)i * ld_gfeat;
      row[0] = (TO)(rv0 * zz[i + 1]);
      row[D] = (TO)(mlpg_rvar(r, T, rv1) * (0.5 * (zz[i + 2] - zz[i])));
      row[2 * D] = (TO)(mlpg_rvar(r, T, rv2) * (zz[i] - 2.0 * zz[i + 1] + zz[i + 2]));
    }
  }
}

// g.a: var, scratch (factor planes), nconv, dim as for the sweeps; the offsets travel with the stream form's own tables
static int mlpg_adjoint_stream_launch(const MlpgAdjointArgs& g, bool gout_f32, bool gfeat_f32, const int64_t* h_offsets,
                                      int n_utts, int64_t t_max, ScratchScope& scratch) {
  hipStream_t s = scratch.stream();
  MlpgArgs a = g.a;
  a.out = g.y;      // b, then z
  a.ld_out = a.dim;
  a.ocol0 = 0;
  const StGrad grad{g.gout, gout_f32, g.ld_gout, g.gcol0};
  return mlpg_stream_launch(a, h_offsets, n_utts, a.dim, t_max, scratch, &grad, [&](const StreamArgs& sg) {
    const dim3 grid((unsigned)((size_t)sg.n_groups * sg.nblk)), block(ST_GS * 64);
    if (gfeat_f32) hipLaunchKernelGGL(mlpg_adjoint_window_kernel<float>, grid, block, 0, s, sg, g.gfeat, g.ld_gfeat, g.col0);
    else hipLaunchKernelGGL(mlpg_adjoint_window_kernel<double>, grid, block, 0, s, sg, g.gfeat, g.ld_gfeat, g.col0);
  });
}

}  // namespace itts
