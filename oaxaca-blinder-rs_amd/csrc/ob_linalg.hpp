// ob_linalg.hpp -- the small dense solves the estimators run on the host, in nalgebra's operation
// order: the Cholesky factor and solve (logit.rs:88-95, akm.rs:352-364, engine.rs:163-167), the LU
// solve (logistic.rs:95) and try_inverse (distance.rs:48-50). Matrices are k x k column-major. The
// order of the operations is part of the output contract: a result's bytes follow
// from it.
#pragma once
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace ob {

namespace {

// nalgebra Cholesky::new (left-looking, per-element updates in column order, the order of
// ob_device.hpp's wave_cholesky) on the lower triangle of m; the strict upper triangle is neither
// read nor written. false iff a pivot is zero, negative or NaN.
inline bool chol_factor(double* m, int k) {
  for (int j = 0; j < k; ++j) {
    for (int i = j; i < k; ++i) {
      double v = m[i + (size_t)j * k];
      for (int c = 0; c < j; ++c) v = -m[j + (size_t)c * k] * m[i + (size_t)c * k] + v;
      m[i + (size_t)j * k] = v;
    }
    const double diag = m[j + (size_t)j * k];
    if (!(diag != 0.0 && diag >= 0.0)) return false;
    const double den = std::sqrt(diag);
    for (int i = j; i < k; ++i) m[i + (size_t)j * k] = (i == j) ? den : m[i + (size_t)j * k] / den;
  }
  return true;
}

// The back substitution of chol_solve. Dot is nalgebra's: the dot product of the solved entries
// first, then (b[i] - dot) / diag. Sequential subtracts term by term from b[i], then divides; the
// two round differently.
enum class BackSub { Dot, Sequential };

// b = (l l^T)^-1 b for the factor l that chol_factor left in the lower triangle.
inline void chol_solve(const double* l, int k, double* b, BackSub back) {
  for (int i = 0; i < k; ++i) {
    const double coeff = b[i] / l[i + (size_t)i * k];
    for (int r = i + 1; r < k; ++r) b[r] -= coeff * l[r + (size_t)i * k];
    b[i] = coeff;
  }
  for (int i = k - 1; i >= 0; --i) {
    const double* col = l + (size_t)i * k;
    if (back == BackSub::Dot) {
      double part = 0.0;
      for (int r = i + 1; r < k; ++r) part += col[r] * b[r];
      b[i] = (b[i] - part) / col[i];
    } else {
      double v = b[i];
      for (int r = i + 1; r < k; ++r) v -= col[r] * b[r];
      b[i] = v / col[i];
    }
  }
}

// Factor and solve: m's lower triangle becomes its factor, b the solution. false as chol_factor.
inline bool chol_factor_solve(double* m, int k, double* b, BackSub back) {
  if (!chol_factor(m, k)) return false;
  chol_solve(m, k, b, back);
  return true;
}

// nalgebra LU::new (partial pivoting by the largest |entry|; a zero pivot column is skipped) + solve:
// m is full; false iff a diagonal entry of U is zero (logistic.rs:95).
inline bool host_lu_solve(std::vector<double>& m, int k, std::vector<double>& b) {
  for (int i = 0; i < k; ++i) {
    int piv = i;
    for (int r = i + 1; r < k; ++r)
      if (std::fabs(m[r + (size_t)i * k]) > std::fabs(m[piv + (size_t)i * k])) piv = r;
    if (m[piv + (size_t)i * k] == 0.0) continue;
    if (piv != i) {
      for (int c = 0; c < k; ++c) std::swap(m[i + (size_t)c * k], m[piv + (size_t)c * k]);
      std::swap(b[i], b[piv]);
    }
    for (int r = i + 1; r < k; ++r) {
      const double f = m[r + (size_t)i * k] / m[i + (size_t)i * k];
      for (int c = i + 1; c < k; ++c) m[r + (size_t)c * k] -= f * m[i + (size_t)c * k];
      b[r] -= f * b[i];
    }
  }
  for (int i = k - 1; i >= 0; --i) {
    const double diag = m[i + (size_t)i * k];
    if (diag == 0.0) return false;
    double part = b[i];
    for (int c = i + 1; c < k; ++c) part -= m[i + (size_t)c * k] * b[c];
    b[i] = part / diag;
  }
  return true;
}

// determinant of the (d - 1) x (d - 1) minor of m (d <= 4) without row sr and column sc
inline double minor_det(const std::vector<double>& m, int d, int sr, int sc) {
  double a[3][3];
  int ri = 0;
  for (int r = 0; r < d; ++r) {
    if (r == sr) continue;
    int ci = 0;
    for (int c = 0; c < d; ++c) {
      if (c == sc) continue;
      a[ri][ci++] = m[r + (size_t)c * d];
    }
    ++ri;
  }
  switch (d - 1) {
    case 0: return 1.0;
    case 1: return a[0][0];
    case 2: return a[0][0] * a[1][1] - a[1][0] * a[0][1];
    default:
      return a[0][0] * (a[1][1] * a[2][2] - a[2][1] * a[1][2]) - a[0][1] * (a[1][0] * a[2][2] - a[2][0] * a[1][2]) +
             a[0][2] * (a[1][0] * a[2][1] - a[2][0] * a[1][1]);
  }
}

// nalgebra try_inverse: the adjugate over the determinant up to dimension 4 (false when the
// determinant is exactly zero), LU with partial pivoting beyond (false on a zero pivot).
inline bool try_inverse(const std::vector<double>& m, int d, std::vector<double>& inv) {
  inv.assign((size_t)d * d, 0.0);
  if (d <= 4) {
    std::vector<double> cof((size_t)d * d);
    for (int r = 0; r < d; ++r)
      for (int c = 0; c < d; ++c) cof[r + (size_t)c * d] = (((r + c) & 1) ? -1.0 : 1.0) * minor_det(m, d, r, c);
    double det = 0.0;
    for (int c = 0; c < d; ++c) det += m[(size_t)c * d] * cof[(size_t)c * d];
    if (det == 0.0) return false;
    for (int r = 0; r < d; ++r)
      for (int c = 0; c < d; ++c) inv[r + (size_t)c * d] = cof[c + (size_t)r * d] / det;
    return true;
  }
  std::vector<double> a(m);
  for (int i = 0; i < d; ++i) inv[i + (size_t)i * d] = 1.0;
  for (int i = 0; i < d; ++i) {
    int piv = i;
    for (int r = i + 1; r < d; ++r)
      if (std::fabs(a[r + (size_t)i * d]) > std::fabs(a[piv + (size_t)i * d])) piv = r;
    if (a[piv + (size_t)i * d] == 0.0) continue;
    if (piv != i)
      for (int c = 0; c < d; ++c) {
        std::swap(a[i + (size_t)c * d], a[piv + (size_t)c * d]);
        std::swap(inv[i + (size_t)c * d], inv[piv + (size_t)c * d]);
      }
    for (int r = i + 1; r < d; ++r) {
      const double f = a[r + (size_t)i * d] / a[i + (size_t)i * d];
      for (int c = i + 1; c < d; ++c) a[r + (size_t)c * d] -= f * a[i + (size_t)c * d];
      for (int c = 0; c < d; ++c) inv[r + (size_t)c * d] -= f * inv[i + (size_t)c * d];
    }
  }
  for (int i = d - 1; i >= 0; --i) {
    const double diag = a[i + (size_t)i * d];
    if (diag == 0.0) return false;
    for (int c = 0; c < d; ++c) {
      double part = inv[i + (size_t)c * d];
      for (int j = i + 1; j < d; ++j) part -= a[i + (size_t)j * d] * inv[j + (size_t)c * d];
      inv[i + (size_t)c * d] = part / diag;
    }
  }
  return true;
}

}  // namespace

}  // namespace ob
