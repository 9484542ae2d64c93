// The split between a real transform of n samples and the complex transform of n/2 points it runs on, for one
// pair of bins (k, j = n/2 - k).  Written once for the workgroup transforms (world_dev.h) and the wave transforms
// (wave_fft.h), whose results are bit-identical: the build contracts a*b+c within a statement, so the statements
// here -- operands, grouping, order -- are the arithmetic.
#pragma once
#include "common.h"

namespace itts {

// Forward: Z = the complex transform of z[m] = (x[2m], x[2m+1]), w = e^{+2 pi i k / n} -> X[k], X[j].
__device__ __forceinline__ void rsplit_fwd(const double2 zk, const double2 zj, const double2 w, double2& Xk, double2& Xj) {
  const double er = 0.5 * (zk.x + zj.x), ei = 0.5 * (zk.y - zj.y);
  const double dr = 0.5 * (zk.x - zj.x), di = 0.5 * (zk.y + zj.y);
  const double orr = di, oi = -dr;  // O = -i D
  const double wr = w.x, wi = -w.y;  // w^k = e^{-2 pi i k / n}
  const double tr = orr * wr - oi * wi, ti = orr * wi + oi * wr;
  Xk = make_double2(er + tr, ei + ti);
  Xj = make_double2(er - tr, -(ei - ti));
}

// Inverse: X[k], X[j], w = conj(w^k) = e^{+2 pi i k / n} -> Z[k], Z[j] of the complex transform to invert.
__device__ __forceinline__ void rsplit_inv(const double2 xk, const double2 xj, const double2 w, double2& zk, double2& zj) {
  const double er = 0.5 * (xk.x + xj.x), ei = 0.5 * (xk.y - xj.y);
  const double dr = 0.5 * (xk.x - xj.x), di = 0.5 * (xk.y + xj.y);
  const double orr = dr * w.x - di * w.y, oi = dr * w.y + di * w.x;
  zk = make_double2(er - oi, ei + orr);
  zj = make_double2(er + oi, -ei + orr);
}

}  // namespace itts
