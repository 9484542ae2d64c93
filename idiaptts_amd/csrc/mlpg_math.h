// MLPG: the mathematics every solve form shares, written once (MLPG.generation, idiaptts/misc/mlpg.py:94-127).
// Per dimension and T frames: P x = b with the symmetric pentadiagonal precision matrix
//   P = diag(t0) + W1^T diag(t1) W1 + W2^T diag(t2) W2,   b = W0^T(m0 t0) + W1^T(m1 t1) + W2^T(m2 t2)
// W1 = [-.5 0 .5], W2 = [1 -2 1] Toeplitz, t_w = 1/var_w with the delta variances of the first and last frame forced
// to 1e11 (mlpg.py:114-117), solved by banded Cholesky (what bandmat.linalg.solveh does).
// The library is built with -ffp-contract=on, which fuses within a source expression: an expression split or joined
// here changes the last bit of every form.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MLPG_HD __host__ __device__ __forceinline__
#else
#define MLPG_HD inline
#endif

namespace itts {

constexpr double kBigVar = 100000000000.0;  // mlpg.py:114

struct MlpgArgs {
  const double* feat;
  int64_t ld_feat;
  int col0;
  int dim;
  const double* var;
  const int64_t* offsets;  // device copy, [U+1]
  double* out;
  int64_t ld_out;
  int ocol0;
  double* scratch;  // 3 planes [Ttot, dim]: 1/d, l1, l2 (shared factor) + nconv
  int64_t t_total;
  int* nconv;       // [dim] frame index where the shared factor becomes stationary
};

// ---- the edge-variance model ----------------------------------------------------------------------------------------
template <typename I>
MLPG_HD bool mlpg_edge_frame(I t, I T) { return (t == 0 || t == T - 1); }

// The reciprocal variance the right-hand side multiplies frame t's delta (or delta-delta) entry by: r_in = 1 / var, or
// 1 / kBigVar at the edges.  No zero outside the utterance: callers gate on j > 0 / j + 1 < T.  V: double, or the
// two-double vector of the ring's wide helpers.
template <typename V, typename I>
MLPG_HD V mlpg_rvar(I t, I T, V r_in) { return mlpg_edge_frame(t, T) ? (V)(1.0 / kBigVar) : r_in; }

struct MlpgRow { double pjj, pj1, pj2; };      // P[j,j], P[j+1,j], P[j+2,j]

// The precisions of one dimension over an utterance of T frames (I: the caller's frame index type).  INF selects the
// "T = infinity" view the shared factor is derived in: an edge at frame 0 only, T unused.
template <typename I>
struct MlpgPrec {
  I T;
  double tau0, tau1_in, tau2_in;
  template <bool INF>
  MLPG_HD double tau(double tau_in, I t) const {
    if (INF) return t < 0 ? 0.0 : (t == 0 ? 1.0 / kBigVar : tau_in);
    if (t < 0 || t >= T) return 0.0;
    return mlpg_edge_frame(t, T) ? 1.0 / kBigVar : tau_in;
  }
  template <bool INF>
  MLPG_HD MlpgRow row(I j) const {
    auto tau1 = [&](I t) { return tau<INF>(tau1_in, t); };
    auto tau2 = [&](I t) { return tau<INF>(tau2_in, t); };
    MlpgRow p;
    p.pjj = tau0 + 0.25 * (tau1(j - 1) + tau1(j + 1)) + (tau2(j - 1) + 4.0 * tau2(j) + tau2(j + 1));
    p.pj1 = (INF || j + 1 < T) ? -2.0 * (tau2(j) + tau2(j + 1)) : 0.0;
    p.pj2 = (INF || j + 2 < T) ? (tau2(j + 1) - 0.25 * tau1(j + 1)) : 0.0;
    return p;
  }
};

// ---- the Cholesky step ----------------------------------------------------------------------------------------------
// 1 / sqrt(x) for the pivot of the shared factor: hardware estimate + three Newton steps (nine dependent
// multiply-adds) instead of a square root and a division (~60 dependent instructions) -- the factor is one
// latency chain per dimension in front of every solve, 18-22 us of a 256-utterance call.  The estimate
// carries >= 13 bits, three steps square that past the 53 of a double; the last step's residual form keeps
// the result within an ulp or two of the correctly rounded one (the solve's 1e-10 budget against the
// oracle is nine orders above that).
MLPG_HD double factor_rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rsq(x);
#else
  double y = 1.0 / sqrt(x);              // (host: the steps below leave it where it is, to an ulp)
#endif
  const double h = 0.5 * x;
  y = y * (1.5 - h * y * y);
  y = y * (1.5 - h * y * y);
  const double r = 0.5 - h * y * y;      // residual of the third step
  return y + y * r;
}

// Row j of the factor from the state that reaches it (l1p = L[j,j-1], l2p = L[j,j-2], cprev = L[j+1,j-1]):
// dd = 1 / L[j,j] (the solves multiply instead of dividing), l1 = L[j+1,j], l2 = L[j+2,j].  SHARED: the shared
// factor's pivot (factor_rsqrt); else a re-derived tail frame's (a square root and a division).
template <bool SHARED>
MLPG_HD void mlpg_chol_step(const MlpgRow& p, double l1p, double l2p, double cprev, double& dd, double& l1, double& l2) {
  const double pivot = p.pjj - l1p * l1p - l2p * l2p;
  dd = SHARED ? factor_rsqrt(pivot) : 1.0 / sqrt(pivot);
  l1 = (p.pj1 - cprev * l1p) * dd;
  l2 = p.pj2 * dd;
}

// P is constant for j >= 2 in the T = infinity view, so the recurrence is a fixed map of (l1p, l2p, cprev): once the
// state repeats every later frame has the same factor.  Bit-for-bit repetition may never come -- the rounded map can
// settle into a two-value cycle one ulp wide -- so "repeats to within 2^-50" ends the search.
template <typename I>
MLPG_HD bool mlpg_factor_settled(I j, double l1, double l2, double l1p, double l2p, double cprev) {
  auto same = [](double x, double y) { return fabs(x - y) <= 8.9e-16 * fabs(y); };
  return j >= 3 && same(l1, l1p) && same(l2, cprev) && same(cprev, l2p);
}

// The factor is shared for j <= T-3; the last two frames are re-derived with the true edge variances and kept here
// (T < 3: everything is re-derived, and only frames T-2, T-1 are ever asked for).
struct MlpgTail {
  double d0 = 1.0, d1 = 1.0, l10 = 0.0, l11 = 0.0, l20 = 0.0, l21 = 0.0;      // frame T-2, frame T-1
  template <typename I>
  MLPG_HD void put(I j, I T, double dd, double l1, double l2) {
    if (j == T - 1) { d1 = dd; l11 = l1; l21 = l2; }
    else { d0 = dd; l10 = l1; l20 = l2; }
  }
  template <typename I>
  MLPG_HD void get(I j, I T, double& dd, double& l1, double& l2) const {
    const bool last = j == T - 1;
    const MlpgTail v = *this;      // (values, not a choice between two addresses: the struct then lives in registers)
    dd = last ? v.d1 : v.d0; l1 = last ? v.l11 : v.l10; l2 = last ? v.l21 : v.l20;
  }
};

// ---- the right-hand side --------------------------------------------------------------------------------------------
// b-frame j from the mean / var entries (mlpg.py:123) of rows j-1 (p), j (c), j+1 (n) for windows 0, 1, 2; the caller
// has put zeros where a row does not exist.  V: double or a two-double vector.
template <typename V>
MLPG_HD V mlpg_rhs(V c0, V p1, V n1, V p2, V c2, V n2) {
  return c0 + 0.5 * (p1 - n1) + (p2 - 2.0 * c2 + n2);
}

// The same sum as the stream form accumulates it, window by window.  Another rounding: NOT interchangeable with
// mlpg_rhs bit for bit.
MLPG_HD double mlpg_rhs_by_window(double c0, double p1, double n1, double p2, double c2, double n2) {
  double b = c0;
  b += 0.5 * (p1 - n1);
  b += (p2 - 2.0 * c2 + n2);
  return b;
}

}  // namespace itts
