// ob_tobit.hpp -- the bootstrapped Tobit decomposition of a censored outcome (Bauer and Sinning 2008, 2010;
// DESIGN.md §5.24): limits, row layout and the inverse Mills ratio both sides evaluate (ob_tobit.hip holds the rest;
// ob_builder.cpp routes a handle through the hooks of ob_model.hpp and aggregates its rows).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

struct ob_prepared;
struct ob_results;

namespace ob {

constexpr int kTobitMaxK = 31;  // design columns with the intercept (OB_TOBIT_MAX_K): eta = [delta; theta] has K + 1
constexpr int kTobitTail = 17;  // the scalars after the five K-vectors of the row
// Row (include/oaxaca_boot.h): 6 aggregates | explained_k | unexplained_k | beta_A, beta_B, xbar_A, xbar_B, beta* |
// 3 latent terms | M_AA, M_AB, M_BA, M_BB | ybar_A, ybar_B | sigma_A, sigma_B | 4 censored shares | passes A, B.
inline int tobit_row_len(int k) { return 6 + 7 * k + kTobitTail; }
// The checks every entry point makes before any device work. k: design columns with the intercept.
int tobit_check_shape(int k, int64_t n_a, int64_t n_b);
// The aggregation of ob_prepared_finish on rows of tobit_row_len(k) doubles (ob_builder.cpp; no HIP call). names: the
// k design columns, or NULL for "x0" .. "x<k-1>".
int tobit_finish_rows(const double* point, int k, const char* const* names, const double* rows, const uint8_t* ok,
                      uint64_t n_reps, ob_results** out);

// W. J. Cody's rational approximations of erfc (Math. Comp. 23 (1969); the coefficients and regions of ob_normal.hpp's
// npdf_ncdf, which keeps its own copy so that the probit kernels compile as they did): for y > 0.46875,
// erfc(y) = exp(-y^2) R(y). R is a quotient of two degree-8 polynomials for y <= 4 and the asymptotic series' rational
// form in 1 / y^2 beyond. rcp: the reciprocal of the caller's side (ob_normal.hpp's nd_rcp on the device).
template <class Rcp>
__host__ __device__ inline double tobit_erfc_scaled(double y, Rcp rcp) {
  if (y <= 4.0) {
    double xn = 2.15311535474403846e-8 * y, xd = y;
    xn = (xn + 5.64188496988670089e-1) * y;
    xd = (xd + 1.57449261107098347e01) * y;
    xn = (xn + 8.88314979438837594e00) * y;
    xd = (xd + 1.17693950891312499e02) * y;
    xn = (xn + 6.61191906371416295e01) * y;
    xd = (xd + 5.37181101862009858e02) * y;
    xn = (xn + 2.98635138197400131e02) * y;
    xd = (xd + 1.62138957456669019e03) * y;
    xn = (xn + 8.81952221241769090e02) * y;
    xd = (xd + 3.29079923573345963e03) * y;
    xn = (xn + 1.71204761263407058e03) * y;
    xd = (xd + 4.36261909014324716e03) * y;
    xn = (xn + 2.05107837782607147e03) * y;
    xd = (xd + 3.43936767414372164e03) * y;
    return (xn + 1.23033935479799725e03) * rcp(xd + 1.23033935480374942e03);
  }
  const double iy = rcp(y), ysq = iy * iy;
  double xn = 1.63153871373020978e-2 * ysq, xd = ysq;
  xn = (xn + 3.05326634961232344e-1) * ysq;
  xd = (xd + 2.56852019228982242e00) * ysq;
  xn = (xn + 3.60344899949804439e-1) * ysq;
  xd = (xd + 1.87295284992346725e00) * ysq;
  xn = (xn + 1.25781726111229246e-1) * ysq;
  xd = (xd + 5.27905102951428412e-1) * ysq;
  xn = (xn + 1.60837851487422766e-2) * ysq;
  xd = (xd + 6.05183413124413191e-2) * ysq;
  const double r = ysq * (xn + 6.58749161529837803e-4) * rcp(xd + 2.33520497626869185e-3);
  return (5.6418958354775628695e-1 - r) * iy;
}

// lambda(z) = phi(z) / Phi(z), finite and accurate for every finite z. With x = -z / sqrt 2: Phi(z) = erfc(x) / 2 and
// phi(z) = exp(-x^2) / sqrt(2 pi). Below the cut z < -0.46875 sqrt 2 (x > 0.46875) erfc(x) = exp(-x^2) R(x), so
// lambda = sqrt(2 / pi) / R(x) without the exponential that underflows. Above it Phi >= 0.25 and the quotient is
// taken as it stands from one exponential: erfc(x) by Cody's central region for |x| <= 0.46875, 2 - erfc(-x) beyond.
template <class Rcp>
__host__ __device__ inline double tobit_lambda_with(double z, Rcp rcp) {
  const double x = -z * 0.7071067811865476;
  if (x > 0.46875) return 0.7978845608028654 * rcp(tobit_erfc_scaled(x, rcp));
  const double e = exp(-0.5 * z * z), y = fabs(x);
  double r;  // erfc(x)
  if (y <= 0.46875) {
    const double ysq = y * y;
    double xn = 1.85777706184603153e-1 * ysq, xd = ysq;
    xn = (xn + 3.16112374387056560e00) * ysq;
    xd = (xd + 2.36012909523441209e01) * ysq;
    xn = (xn + 1.13864154151050156e02) * ysq;
    xd = (xd + 2.44024637934444173e02) * ysq;
    xn = (xn + 3.77485237685302021e02) * ysq;
    xd = (xd + 1.28261652607737228e03) * ysq;
    r = 1.0 - x * (xn + 3.20937758913846947e03) * rcp(xd + 2.84423683343917062e03);
  } else {
    r = 2.0 - tobit_erfc_scaled(y, rcp) * e;
  }
  return e * 0.7978845608028654 * rcp(r);  // phi / (erfc / 2)
}

// The host's evaluation (ob_tobit_lambda): the same branches with the division of the language.
inline double tobit_lambda_host(double z) {
  return tobit_lambda_with(z, [](double v) { return 1.0 / v; });
}

}  // namespace ob
