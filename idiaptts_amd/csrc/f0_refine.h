// WORLD's GetRefinedF0 on one wave, written once for StoneMask (world_f0ap.hip) and Harvest (harvest.hip).
//
// A candidate f0 is refined from three of its periods: the segment times a Blackman-type window and times that
// window's derivative, both spectra at up to six harmonic bins, and the amplitude-weighted instantaneous frequency
// of those bins.  Only the harmonic bins are ever read, so the two FFTs are direct DFT sums.  Three steps:
//   window_pass    (x * w, x * dw) of the segment to the wave's LDS block, the window by one sincos per lane and
//                  rotations
//   harmonic_sums  lanes regroup as 2^HB harmonics x 2^(6-HB) sample phases and sum their bin of both spectra
//   refined_f0     instantaneous frequency per harmonic lane, summed over the harmonics
// The callers keep what differs: which frames and candidates a wave takes, where the rotation values and the DFT
// factors come from (functors), and what they accept of the result.  Every sum here has ONE order -- both
// callers' results are pinned bit for bit by scripts/world_checksum.py.
#pragma once
#include "world_dev.h"

namespace itts {
namespace f0r {
using namespace wd;

// x[i] with i held inside [0, len): the segment repeats the signal's edge samples
template <typename I>
__device__ __forceinline__ double edge_sample(const double* __restrict__ x, I i, I len) {
  i = i < 0 ? 0 : (i > len - 1 ? len - 1 : i);
  return x[i];
}

// The window's two rotations for a window of wlt seconds: {sin, cos of 2 pi 64 / n; sin, cos of 2 pi / n}, n = fs * wlt
// samples.  They depend on n only (Harvest tabulates them per call, StoneMask evaluates them per frame).
__device__ __forceinline__ double4 window_rotations(double fs, double wlt) {
  double rs, rc, ds1, dc1;
  sincospi(2.0 * 64.0 / (fs * wlt), &rs, &rc);
  sincospi(2.0 / (fs * wlt), &ds1, &dc1);
  return make_double4(rs, rc, ds1, dc1);
}

// ws[i] = (x_i w_i, x_i dw_i) for the n (odd) samples of the segment; x_i = fetch(i).  theta: the window angle of
// sample `lane` in half turns, 2 t / wlt with t the sample's time from the window centre; w = 0.42 + 0.5 cos(pi
// theta) + 0.08 cos(2 pi theta).  One sincos per lane, then rotations by 64 samples; the neighbours that the
// derivative window dw_i = -(w_{i+1} - w_{i-1}) / 2 needs are rotations by one sample.
template <typename Fetch>
__device__ __forceinline__ void window_pass(double theta, double4 rot, int n, int lane, Fetch fetch,
                                            double2* __restrict__ ws) {
  double sn, cs;
  sincospi(theta, &sn, &cs);
  const double rs = rot.x, rc = rot.y, ds1 = rot.z, dc1 = rot.w;
  auto win = [](double c) { return 0.42 + 0.5 * c + 0.08 * (2.0 * c * c - 1.0); };
  // four rows of 64 samples per trip, their loads in flight together (one trip to the cache for windows of up
  // to 256 samples instead of one per row)
  for (int i0 = lane; i0 < n; i0 += 256) {
    double xq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xq[q] = fetch(i0 + 64 * q);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + 64 * q;
      if (i < n) {
        const double xv = xq[q];
        const double mw = win(cs);
        const double up = win(cs * dc1 - sn * ds1), dn = win(cs * dc1 + sn * ds1);  // w[i + 1], w[i - 1]
        double dw;
        if (i == 0) dw = -up / 2.0;               // WORLD's first and last element: the neighbour outside counts as 0
        else if (i == n - 1) dw = dn / 2.0;
        else dw = -(up - dn) / 2.0;
        ws[i] = make_double2(xv * mw, xv * dw);
        const double c2 = cs * rc - sn * rs;
        sn = sn * rc + cs * rs;
        cs = c2;
      }
    }
  }
}

struct Spectra {
  double mr, mi, dr, di;   // main-window spectrum M and derivative-window spectrum D at the lane's bin
};

// Lanes = 2^HB harmonics x 2^(6-HB) sample phases: lane (hq, ph) sums the samples ph, ph + P, ... of its harmonic's
// bin, then a butterfly over the phase lanes.  factor() returns exp(-2 pi i bin k / fft) for the lane's next
// sample k (it starts at k = ph and advances by P per call).  Four samples per trip with their factors and LDS
// reads in flight together; the four sums keep ascending sample order.  `active`: the lane's harmonic is one of
// the nh that count (the others only take part in the butterflies).
template <int HB, typename Factor>
__device__ __forceinline__ Spectra harmonic_sums(const double2* __restrict__ ws, int n, int lane, bool active,
                                                 Factor factor) {
  constexpr int P = 1 << (6 - HB);
  double mr = 0.0, mi = 0.0, dr = 0.0, di = 0.0;
  if (active) {
    int i = lane & (P - 1);
    for (; i + 3 * P < n; i += 4 * P) {
      const double2 w0 = factor(), w1 = factor(), w2 = factor(), w3 = factor();
      const double2 s0 = ws[i], s1 = ws[i + P], s2 = ws[i + 2 * P], s3 = ws[i + 3 * P];
      mr += s0.x * w0.x; mi += s0.x * w0.y; dr += s0.y * w0.x; di += s0.y * w0.y;
      mr += s1.x * w1.x; mi += s1.x * w1.y; dr += s1.y * w1.x; di += s1.y * w1.y;
      mr += s2.x * w2.x; mi += s2.x * w2.y; dr += s2.y * w2.x; di += s2.y * w2.y;
      mr += s3.x * w3.x; mi += s3.x * w3.y; dr += s3.y * w3.x; di += s3.y * w3.y;
    }
    for (; i < n; i += P) {
      const double2 w0 = factor();
      const double2 s0 = ws[i];
      mr += s0.x * w0.x; mi += s0.x * w0.y; dr += s0.y * w0.x; di += s0.y * w0.y;
    }
  }
#pragma unroll
  for (int mask = 1; mask < P; mask <<= 1) {
    mr = xor_sum(mr, mask);
    mi = xor_sum(mi, mask);
    dr = xor_sum(dr, mask);
    di = xor_sum(di, mask);
  }
  return Spectra{mr, mi, dr, di};
}

struct Refined {
  double f0;     // sum of amp * inst over the harmonics / (sum of amp * harmonic number + eps)
  double dev;    // SCORE: sum over the harmonics of |inst / harmonic number - f0| / f0 (Harvest's score term)
};

// Instantaneous frequency of harmonic hq + 1 (bin `bin` of an fft-point spectrum) from its lane's spectra, then the
// butterfly over the harmonic lanes: the result is in every lane.
template <int HB, bool SCORE>
__device__ __forceinline__ Refined refined_f0(const Spectra& s, bool active, int bin, int hq, double fs, int fft,
                                              double f0) {
  constexpr int P = 1 << (6 - HB);
  double num = 0.0, den = 0.0, dev = 0.0;
  if (active) {
    const double ps = s.mr * s.mr + s.mi * s.mi;
    const double numer = s.mr * s.di - s.mi * s.dr;
    const double inst = ps == 0.0 ? 0.0 : (double)bin * fs / fft + numer / ps * fs / 2.0 / kPi;
    const double amp = sqrt(ps);
    num = amp * inst;
    den = amp * (hq + 1.0);
    if (SCORE) dev = fabs((inst / (hq + 1.0) - f0) / f0);
  }
#pragma unroll
  for (int mask = P; mask < 64; mask <<= 1) {
    num = xor_sum(num, mask);
    den = xor_sum(den, mask);
    if (SCORE) dev = xor_sum(dev, mask);
  }
  return Refined{num / (den + kEps), dev};
}

}  // namespace f0r
}  // namespace itts
