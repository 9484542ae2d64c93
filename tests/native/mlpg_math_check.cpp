// Host check of csrc/mlpg_math.h: builds P and b of one dimension from the header's pieces, solves with the header's
// own Cholesky step and two sweeps (shared factor + re-derived tail, as the kernels do), and prints that next to a
// dense solve of the same system written out here from MLPG.generation (mlpg.py:94-127) without the header.
// stdin: n_cases, then per case "T v0 v1 v2" and T rows "m0 m1 m2".  stdout: one JSON line per case
// (tests/test_mlpg_math.py compares).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../idiaptts_amd/csrc/mlpg_math.h"

using itts::MlpgPrec;
using itts::MlpgTail;

static std::vector<double> header_solve(int T, const std::vector<double>& m, double v0, double v1, double v2) {
  const MlpgPrec<int> prec{T, 1.0 / v0, 1.0 / v1, 1.0 / v2};
  const double rv0 = 1.0 / v0, rv1 = 1.0 / v1, rv2 = 1.0 / v2;
  const int n_shared = T >= 3 ? T - 2 : 0;
  // the shared factor ("T = infinity"), until it repeats
  std::vector<double> fd, fl1, fl2;
  int ncv = 0;
  {
    double l1p = 0.0, l2p = 0.0, cprev = 0.0;
    for (int j = 0; j < std::max(n_shared, 1); ++j) {
      double dd, l1, l2;
      itts::mlpg_chol_step<true>(prec.row<true>(j), l1p, l2p, cprev, dd, l1, l2);
      fd.push_back(dd); fl1.push_back(l1); fl2.push_back(l2);
      ncv = j;
      if (itts::mlpg_factor_settled(j, l1, l2, l1p, l2p, cprev)) break;
      l2p = cprev; l1p = l1; cprev = l2;
    }
  }
  std::vector<double> x(T);
  MlpgTail tail;
  double l1p = 0.0, l2p = 0.0, cprev = 0.0, y1 = 0.0, y2 = 0.0;
  for (int j = 0; j < T; ++j) {
    const double c0 = m[3 * j] * rv0, c2 = m[3 * j + 2] * itts::mlpg_rvar(j, T, rv2);
    const double p1 = j > 0 ? m[3 * (j - 1) + 1] * itts::mlpg_rvar(j - 1, T, rv1) : 0.0;
    const double p2 = j > 0 ? m[3 * (j - 1) + 2] * itts::mlpg_rvar(j - 1, T, rv2) : 0.0;
    const double n1 = j + 1 < T ? m[3 * (j + 1) + 1] * itts::mlpg_rvar(j + 1, T, rv1) : 0.0;
    const double n2 = j + 1 < T ? m[3 * (j + 1) + 2] * itts::mlpg_rvar(j + 1, T, rv2) : 0.0;
    const double b = itts::mlpg_rhs(c0, p1, n1, p2, c2, n2);
    double dd, l1, l2;
    if (j < n_shared) {
      const int jc = std::min(j, ncv);
      dd = fd[jc]; l1 = fl1[jc]; l2 = fl2[jc];
    } else {
      itts::mlpg_chol_step<false>(prec.row<false>(j), l1p, l2p, cprev, dd, l1, l2);
      tail.put(j, T, dd, l1, l2);
    }
    const double y = (b - l1p * y1 - l2p * y2) * dd;
    x[j] = y;
    l2p = cprev; l1p = l1; cprev = l2;
    y2 = y1; y1 = y;
  }
  double x1 = 0.0, x2 = 0.0;
  for (int j = T - 1; j >= 0; --j) {
    double dd, l1, l2;
    if (j < n_shared) {
      const int jc = std::min(j, ncv);
      dd = fd[jc]; l1 = fl1[jc]; l2 = fl2[jc];
    } else {
      tail.get(j, T, dd, l1, l2);
    }
    const double xj = (x[j] - l1 * x1 - l2 * x2) * dd;
    x[j] = xj;
    x2 = x1; x1 = xj;
  }
  return x;
}

// mlpg.py:94-127 with dense matrices: W_d[t][t + k] = coeff_d[k + 1], P = sum_d W_d^T diag(tau_d) W_d,
// b = sum_d W_d^T (mean_d / var_d), x = P^-1 b by Gaussian elimination with partial pivoting
static std::vector<double> dense_solve(int T, const std::vector<double>& m, double v0, double v1, double v2) {
  const double coeff[3][3] = {{0.0, 1.0, 0.0}, {-0.5, 0.0, 0.5}, {1.0, -2.0, 1.0}};
  const double var_in[3] = {v0, v1, v2};
  std::vector<double> P((size_t)T * T, 0.0), b(T, 0.0);
  for (int d = 0; d < 3; ++d) {
    std::vector<double> W((size_t)T * T, 0.0), var(T, var_in[d]);
    if (d > 0) var[0] = var[T - 1] = 100000000000.0;
    for (int t = 0; t < T; ++t)
      for (int k = -1; k <= 1; ++k)
        if (t + k >= 0 && t + k < T) W[(size_t)t * T + t + k] = coeff[d][k + 1];
    for (int t = 0; t < T; ++t) {
      const double tau = 1.0 / var[t], bf = m[3 * t + d] / var[t];
      for (int i = 0; i < T; ++i) {
        b[i] += W[(size_t)t * T + i] * bf;
        for (int j = 0; j < T; ++j) P[(size_t)i * T + j] += W[(size_t)t * T + i] * tau * W[(size_t)t * T + j];
      }
    }
  }
  for (int c = 0; c < T; ++c) {
    int piv = c;
    for (int r = c + 1; r < T; ++r)
      if (std::fabs(P[(size_t)r * T + c]) > std::fabs(P[(size_t)piv * T + c])) piv = r;
    if (piv != c) {
      for (int j = 0; j < T; ++j) std::swap(P[(size_t)c * T + j], P[(size_t)piv * T + j]);
      std::swap(b[c], b[piv]);
    }
    for (int r = c + 1; r < T; ++r) {
      const double f = P[(size_t)r * T + c] / P[(size_t)c * T + c];
      for (int j = c; j < T; ++j) P[(size_t)r * T + j] -= f * P[(size_t)c * T + j];
      b[r] -= f * b[c];
    }
  }
  std::vector<double> x(T);
  for (int r = T - 1; r >= 0; --r) {
    double s = b[r];
    for (int j = r + 1; j < T; ++j) s -= P[(size_t)r * T + j] * x[j];
    x[r] = s / P[(size_t)r * T + r];
  }
  return x;
}

static void print_vec(const char* name, const std::vector<double>& v, const char* end) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%.17g", i ? ", " : "", v[i]);
  printf("]%s", end);
}

int main() {
  int n_cases = 0;
  if (scanf("%d", &n_cases) != 1) return 2;
  for (int c = 0; c < n_cases; ++c) {
    int T;
    double v0, v1, v2;
    if (scanf("%d %lf %lf %lf", &T, &v0, &v1, &v2) != 4 || T < 1) return 2;
    std::vector<double> m(3 * (size_t)T);
    for (double& e : m)
      if (scanf("%lf", &e) != 1) return 2;
    printf("{\"T\": %d, ", T);
    print_vec("header", header_solve(T, m, v0, v1, v2), ", ");
    print_vec("dense", dense_solve(T, m, v0, v1, v2), "}\n");
  }
  return 0;
}
