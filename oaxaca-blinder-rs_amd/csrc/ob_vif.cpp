// ob_vif.cpp -- host side and C ABI of the VIF collinearity diagnostic: `calculate_vif`
// (oaxaca_blinder/src/math/diagnostics.rs:29-109) over `ols` (math/ols.rs:44-144).
//
// For predictors x_0..x_{K-1} the reference regresses each x_j on [the others in the given order, the
// intercept LAST] and scores 1 / (1 - r2). Every fit's normal equations are rows and columns of one
// extended Gram G = Xe^T Xe, Xe = [x_0..x_{K-1}, 1] (ob_vif.hip), so the K Cholesky solves run here on
// K x K sub-Grams in the reference's column order and nalgebra's operation order (ob_linalg.hpp), and
// the residual sums come back from one more device pass over the rows.
//
// Kept from the reference: a Cholesky failure of any fit fails the whole call (its INFINITY arm at
// diagnostics.rs:69 matches a message ols never produces); ss_tot == 0 scores +inf; |1 - r2| < 1e-9
// scores +inf. A NaN or infinite value needs no path of its own: it reaches a pivot and fails there.
#include <chrono>
#include <cmath>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "ob_common.hpp"
#include "ob_frame.hpp"
#include "ob_hip.hpp"
#include "ob_linalg.hpp"
#include "ob_vif.hpp"

namespace ob {

int vif_check_shape(int64_t n, int k) {
  if (k < 2)  // diagnostics.rs:33-37
    return fail(OB_E_DIAG, "%sVIF calculation requires at least two predictors.", error_prefix(OB_E_DIAG));
  if (k > kVifMaxK)
    return fail(OB_E_UNSUPPORTED, "VIF: %d predictors, the kernels take at most %d", k, kVifMaxK);
  if (n < 0) return fail(OB_E_INVALID, "bad VIF dimensions");
  if ((double)n <= (double)k)  // ols.rs:98-105: each auxiliary design has k columns
    return fail(OB_E_INSUFFICIENT,
                "%sInsufficient data for OLS calculation: n_obs (%lld) must be strictly greater than k (%d)",
                error_prefix(OB_E_INSUFFICIENT), (long long)n, k);
  if ((n + 15) / 16 > (int64_t)0x7fffffff) return fail(OB_E_UNSUPPORTED, "VIF: too many rows");
  return OB_OK;
}

int vif_solve(const double* gram, int64_t n, int k, double* coef) {
  OB_TRY(vif_check_shape(n, k));
  if (!gram || !coef) return fail(OB_E_INVALID, "null pointer");
  const int k1 = k + 1;
  std::vector<int> idx(k);
  std::vector<double> m((size_t)k * k), rhs(k);
  for (int j = 0; j < k; ++j) {
    // Z = [x_c for c != j in the given order, then the intercept] (diagnostics.rs:43-58)
    int t = 0;
    for (int c = 0; c < k; ++c)
      if (c != j) idx[t++] = c;
    idx[t] = k;
    for (int b = 0; b < k; ++b) {
      for (int a = 0; a < k; ++a) m[a + (size_t)b * k] = gram[idx[a] + (size_t)idx[b] * k1];
      rhs[b] = gram[idx[b] + (size_t)j * k1];
    }
    if (!chol_factor_solve(m.data(), k, rhs.data(), BackSub::Dot))  // ols.rs:107-111
      return fail(OB_E_LINALG,
                  "%sFailed to perform Cholesky decomposition. Matrix may be singular or not positive definite due to "
                  "multicollinearity.",
                  error_prefix(OB_E_LINALG));
    double* col = coef + (size_t)j * k1;
    col[j] = 0.0;
    for (int a = 0; a < k; ++a) col[idx[a]] = rhs[a];
  }
  return OB_OK;
}

// diagnostics.rs:76-100
static void vif_scores(const double* ss_res, const double* ss_tot, int k, double* vif) {
  for (int j = 0; j < k; ++j) {
    if (ss_tot[j] == 0.0) {
      vif[j] = std::numeric_limits<double>::infinity();
      continue;
    }
    const double r2 = 1.0 - ss_res[j] / ss_tot[j];
    const double rest = 1.0 - r2;
    vif[j] = std::fabs(rest) < 1e-9 ? std::numeric_limits<double>::infinity() : 1.0 / rest;
  }
}

// The predictors packed column-major n x k (leading dimension n) in HBM.
static int vif_upload(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int k, DevBuf& dx) {
  OB_HIP(hipSetDevice(ctx->device));
  OB_HIP(dx.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(hipMemcpy2DAsync(dx.p, sizeof(double) * (size_t)n, x, sizeof(double) * (size_t)ldx, sizeof(double) * (size_t)n,
                          (size_t)k, hipMemcpyHostToDevice, ctx->stream));
  return OB_OK;
}

// The shape errors come first, so that they are raised whatever else the call carries.
static int vif_check_host(const void* ctx, const double* x, int64_t ldx, int64_t n, int k) {
  OB_TRY(vif_check_shape(n, k));
  if (!ctx || !x) return fail(OB_E_INVALID, "null pointer");
  if (ldx < n) return fail(OB_E_INVALID, "bad VIF dimensions");
  return OB_OK;
}

// What ob_vif_last_timing reports: the calling thread's last ob_vif / ob_vif_run.
struct VifTiming {
  double gram_ms = 0.0, solve_ms = 0.0, sums_ms = 0.0;
};
static VifTiming& vif_timing() {
  static thread_local VifTiming t;
  return t;
}

static int vif_all(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int k, double* vif) {
  const int k1 = k + 1;
  VifTiming& tm = vif_timing();
  tm = VifTiming();
  DevBuf dx;
  OB_TRY(vif_upload(ctx, x, ldx, n, k, dx));
  std::vector<double> gram((size_t)k1 * k1), coef((size_t)k1 * k), means(k), ss_res(k), ss_tot(k);
  OB_TRY(vif_gram_device(ctx, dx.d(), n, n, k, gram.data(), &tm.gram_ms));
  const auto t0 = std::chrono::steady_clock::now();
  OB_TRY(vif_solve(gram.data(), n, k, coef.data()));
  tm.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int c = 0; c < k; ++c) means[c] = gram[c + (size_t)k * k1] / (double)n;
  OB_TRY(vif_sums_device(ctx, dx.d(), n, n, k, coef.data(), means.data(), ss_res.data(), ss_tot.data(), &tm.sums_ms));
  vif_scores(ss_res.data(), ss_tot.data(), k, vif);
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_vif_gram(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int32_t k, double* gram) {
  OB_TRY(ob::vif_check_host(ctx, x, ldx, n, k));
  if (!gram) return ob::fail(OB_E_INVALID, "null pointer");
  DevBuf dx;
  OB_TRY(ob::vif_upload(ctx, x, ldx, n, k, dx));
  return ob::vif_gram_device(ctx, dx.d(), n, n, k, gram, nullptr);
}

int ob_vif_solve(const double* gram, int64_t n, int32_t k, double* coef) { return ob::vif_solve(gram, n, k, coef); }

int ob_vif_sums(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int32_t k, const double* coef,
                const double* means, double* ss_res, double* ss_tot) {
  OB_TRY(ob::vif_check_host(ctx, x, ldx, n, k));
  if (!coef || !means || !ss_res || !ss_tot) return ob::fail(OB_E_INVALID, "null pointer");
  DevBuf dx;
  OB_TRY(ob::vif_upload(ctx, x, ldx, n, k, dx));
  return ob::vif_sums_device(ctx, dx.d(), n, n, k, coef, means, ss_res, ss_tot, nullptr);
}

int ob_vif(ob_ctx* ctx, const double* x, int64_t ldx, int64_t n, int32_t k, double* vif) {
  OB_TRY(ob::vif_check_host(ctx, x, ldx, n, k));
  if (!vif) return ob::fail(OB_E_INVALID, "null pointer");
  return ob::vif_all(ctx, x, ldx, n, k, vif);
}

int ob_vif_last_timing(double* gram_ms, double* solve_ms, double* sums_ms) {
  const ob::VifTiming& t = ob::vif_timing();
  if (gram_ms) *gram_ms = t.gram_ms;
  if (solve_ms) *solve_ms = t.solve_ms;
  if (sums_ms) *sums_ms = t.sums_ms;
  return OB_OK;
}

int ob_vif_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const char* const* names,
               int32_t n_names, double* vif) {
  using namespace ob;
  if (n_names < 0 || (n_names > 0 && !names)) return fail(OB_E_INVALID, "bad name list");
  std::set<std::string> seen;
  for (int p = 0; p < n_names; ++p) {
    if (!names[p]) return fail(OB_E_INVALID, "null name");
    if (!seen.insert(names[p]).second) return fail(OB_E_INVALID, "duplicate predictor `%s`", names[p]);
  }
  OB_TRY(vif_check_shape(n_rows, n_names));
  Frame f;
  OB_TRY(load_frame(cols, n_cols, n_rows, f));
  const int64_t n = f.nrows;
  std::vector<double> x((size_t)n * n_names);
  for (int p = 0; p < n_names; ++p) {
    const int ci = f.find(names[p]);
    if (ci < 0) return fail(OB_E_COLUMN, "%s%s", error_prefix(OB_E_COLUMN), names[p]);
    const Col& c = f.cols[ci];
    if (c.kind == OB_COL_STR)  // `.cast(&DataType::Float64)?.f64()?` of a string column
      return fail(OB_E_POLARS, "%sinvalid series dtype: expected `Float64`, got `%s` for `%s`", error_prefix(OB_E_POLARS),
                  dtype_name(c.kind), c.name.c_str());
    double* dst = x.data() + (size_t)p * n;
    for (int64_t r = 0; r < n; ++r) {
      if (!c.valid[r])  // deliberate: the reference reads a null regressand as 0.0 and a null regressor as missing
        return fail(OB_E_INVALID, "null value in predictor column `%s` (row %lld)", c.name.c_str(), (long long)r);
      dst[r] = c.kind == OB_COL_I64 ? (double)c.i[r] : c.f[r];
    }
  }
  if (!ctx || !vif) return fail(OB_E_INVALID, "null pointer");
  return vif_all(ctx, x.data(), n, n, n_names, vif);
}

}  // extern "C"
