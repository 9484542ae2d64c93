// The per-element arithmetic of the raw-waveform readers, written once for mol.hip (whole signals) and
// vocoder_batch.hip (windows of a resident corpus): the two give the same bits because they run the same statements.
#pragma once
#include "common.h"

namespace itts {

// (((sign(x) * log(1 + mu |x|) / log(1 + mu)) + 1) * (mu / 2)) truncated toward zero, every operation rounded on its
// own as numpy does (no fused multiply-add)
__device__ __forceinline__ int64_t mulaw_index(double x, double mu, double log1pmu) {
  const double sgn = (double)((x > 0.0) - (x < 0.0));
  const double lg = log(__dadd_rn(1.0, __dmul_rn(mu, fabs(x))));
  const double q = __ddiv_rn(__dmul_rn(sgn, lg), log1pmu);
  return (int64_t)__dmul_rn(__dadd_rn(q, 1.0), mu / 2.0);
}

// Where output row j of the n_out = m T rows of sample_linearly lies among the T input rows: scipy's
// interp1d(kind="linear") at numpy.linspace(0, T - 1, m T), operation by operation: x_j = j * ((T - 1) / (m T - 1));
// the interval is the one numpy.searchsorted(side="left") names, lo = ceil(x_j) - 1 clipped to 0 .. T - 2 (an x_j that
// is a whole number belongs to the interval on its left, at its end).  The last row is the input's last row (there
// scipy's slope * 1 + y_lo can miss y_hi by an ulp): `last` says so and lo is then T - 1.
struct LinPos {
  int64_t lo;
  double frac;                  // x_j - lo
  bool last;
};

__device__ __forceinline__ LinPos lin_pos(int64_t j, int64_t T, int64_t n_out) {
  LinPos p;
  p.last = j == n_out - 1;
  if (p.last) {
    p.lo = T - 1;
    p.frac = 0.0;
    return p;
  }
  const double step = (double)(T - 1) / (double)(n_out - 1);
  const double pos = __dmul_rn((double)j, step);
  p.lo = max((int64_t)0, min((int64_t)ceil(pos) - 1, T - 2));
  p.frac = pos - (double)p.lo;
  return p;
}

// The value at that place of one column, x pointing at the column's element of row 0 and D values a row:
// slope = y_hi - y_lo in the INPUT's precision (scipy subtracts the float32 rows before it divides by the float64
// abscissae), then slope * (x_j - lo) + y_lo in float64, product and sum rounded on their own.
template <typename TI>
__device__ __forceinline__ double lin_value(const TI* x, int64_t D, const LinPos& p) {
  if (p.last) return (double)x[p.lo * D];
  const TI ylo = x[p.lo * D], yhi = x[(p.lo + 1) * D];
  const TI slope = yhi - ylo;
  return __dadd_rn(__dmul_rn((double)slope, p.frac), (double)ylo);
}

}  // namespace itts
