// ob_normal.hpp -- the standard normal pdf and cdf of the probit kernels (ob_heckman.hip) and of the
// mean-probability pass of the binary decomposition (ob_binary.hip): one definition, so that both
// evaluate the same Phi.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// statrs Normal(0, 1): pdf = exp(-z^2 / 2) / sqrt(2 pi), cdf = erfc(-z / sqrt 2) / 2.
// (The constant divisions are multiplications by the reciprocals: a last-bit difference.)
__device__ __forceinline__ double npdf(double z) { return exp(-0.5 * z * z) * 0.3989422804014327; }
__device__ __forceinline__ double ncdf(double z) { return 0.5 * erfc(-z * 0.7071067811865476); }

// pdf and cdf together from one exp(-z^2 / 2) (OB_HK_ERFC=1): erfc(x), x = -z / sqrt 2, by W. J.
// Cody's rational Chebyshev approximations (Math. Comp. 23 (1969), the CALERF regions |x| < 0.46875,
// <= 4, > 4), whose two outer regions are exp(-x^2) times a rational function -- exp(-x^2) is the
// pdf's exp(-z^2 / 2). Checked against scipy's erfc on z in [-12, 12]: at most 3e-14 relative (the
// rounding of z^2 inside the shared exp, amplified at large |z|; about 1e-15 where the clamped
// probabilities are used).
__device__ __forceinline__ double nd_rcp(double v) {  // 1/v within ~1 ulp (as hk_rcp below)
  double r = __builtin_amdgcn_rcp(v);
  r = fma(fma(-v, r, 1.0), r, r);
  return fma(fma(-v, r, 1.0), r, r);
}
__device__ __forceinline__ void npdf_ncdf(double z, double& pdf, double& cdf) {
  const double x = -z * 0.7071067811865476, y = fabs(x);
  const double e = exp(-0.5 * z * z);
  pdf = e * 0.3989422804014327;
  double r;
  if (y <= 0.46875) {
    const double ysq = y * y;
    double xn = 1.85777706184603153e-1 * ysq, xd = ysq;
    xn = (xn + 3.16112374387056560e00) * ysq;
    xd = (xd + 2.36012909523441209e01) * ysq;
    xn = (xn + 1.13864154151050156e02) * ysq;
    xd = (xd + 2.44024637934444173e02) * ysq;
    xn = (xn + 3.77485237685302021e02) * ysq;
    xd = (xd + 1.28261652607737228e03) * ysq;
    cdf = 0.5 * (1.0 - x * (xn + 3.20937758913846947e03) * nd_rcp(xd + 2.84423683343917062e03));
    return;
  }
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
    r = (xn + 1.23033935479799725e03) * nd_rcp(xd + 1.23033935480374942e03) * e;
  } else {
    const double iy = nd_rcp(y), ysq = iy * iy;
    double xn = 1.63153871373020978e-2 * ysq, xd = ysq;
    xn = (xn + 3.05326634961232344e-1) * ysq;
    xd = (xd + 2.56852019228982242e00) * ysq;
    xn = (xn + 3.60344899949804439e-1) * ysq;
    xd = (xd + 1.87295284992346725e00) * ysq;
    xn = (xn + 1.25781726111229246e-1) * ysq;
    xd = (xd + 5.27905102951428412e-1) * ysq;
    xn = (xn + 1.60837851487422766e-2) * ysq;
    xd = (xd + 6.05183413124413191e-2) * ysq;
    r = ysq * (xn + 6.58749161529837803e-4) * nd_rcp(xd + 2.33520497626869185e-3);
    r = (5.6418958354775628695e-1 - r) * iy * e;
  }
  cdf = 0.5 * (x >= 0.0 ? r : 2.0 - r);
}

}  // namespace
