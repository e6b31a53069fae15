// ob_match.cpp -- C ABI of the reference's matching module over a column frame, with the distance
// pass, the covariance, the transform and the logistic's sums on the MI355X (ob_match.hip, ob_dfl.hip).
//
//   run_matching         matching/engine.rs:113-229
//   match_psm            matching/engine.rs:232-283 (prepare_data: engine.rs:38-95)
//   MahalanobisDistance  matching/distance.rs:30-53
//   LogisticRegression   matching/logistic.rs:31-113
// The one deliberate difference: ties among exactly equidistant controls go to the smaller control
// position (include/oaxaca_boot.h); the reference's depend on its tree's shape.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "ob_common.hpp"
#include "ob_frame.hpp"
#include "ob_linalg.hpp"
#include "ob_match.hpp"

struct ob_match_results {
  std::vector<double> weights, dist2;
  std::vector<int64_t> treated_rows, neighbor_rows;
  int64_t n_treated = 0, n_control = 0;
  int k = 0, iterations = 0, converged = 0;
  double knn_ms = 0.0, prep_ms = 0.0;
};

namespace ob {

namespace {

int polars_not_found(const std::string& name) {
  return fail(OB_E_POLARS, "%snot found: %s", error_prefix(OB_E_POLARS), name.c_str());
}

double col_value(const Col& c, int64_t r) { return c.kind == OB_COL_I64 ? (double)c.i[r] : c.f[r]; }

// 0.0 with the f64 value 1.0 / k added m times in sequence (engine.rs:206-208), for m = 0 .. m_max
std::vector<double> weight_table(int k, uint32_t m_max) {
  std::vector<double> t((size_t)m_max + 1, 0.0);
  const double step = 1.0 / (double)k;
  double w = 0.0;
  for (uint32_t m = 1; m <= m_max; ++m) {
    w += step;
    t[m] = w;
  }
  return t;
}

struct Groups {
  std::vector<int64_t> treated, control;
};

// engine.rs:120-127: rows equal to 1 and rows equal to 0; a null is in neither
int split_groups(const Frame& f, const std::string& treatment, const Col** tcol, Groups& g) {
  const int ti = f.find(treatment);
  if (ti < 0) return polars_not_found(treatment);
  const Col& t = f.cols[ti];
  if (t.kind == OB_COL_STR)
    return fail(OB_E_POLARS, "%scannot compare string column `%s` with a number", error_prefix(OB_E_POLARS),
                t.name.c_str());
  for (int64_t r = 0; r < f.nrows; ++r) {
    if (!t.valid[r]) continue;
    const double v = col_value(t, r);
    if (v == 1.0) g.treated.push_back(r);
    else if (v == 0.0) g.control.push_back(r);
  }
  *tcol = &t;
  return OB_OK;
}

int covariate_columns(const Frame& f, const ob_match_config* cfg, std::vector<const Col*>& out) {
  if (cfg->n_covariates < 0 || (cfg->n_covariates > 0 && !cfg->covariates)) return fail(OB_E_INVALID, "bad name list");
  for (int p = 0; p < cfg->n_covariates; ++p) {
    if (!cfg->covariates[p]) return fail(OB_E_INVALID, "null name");
    const int ci = f.find(cfg->covariates[p]);
    if (ci < 0) return polars_not_found(cfg->covariates[p]);
    const Col& c = f.cols[ci];
    if (c.kind == OB_COL_STR)
      return fail(OB_E_POLARS, "%sstring covariate column `%s` cannot be cast to f64", error_prefix(OB_E_POLARS),
                  c.name.c_str());
    for (int64_t r = 0; r < f.nrows; ++r)
      if (!c.valid[r])  // stricter than the reference, whose to_ndarray would carry the null as NaN
        return fail(OB_E_POLARS, "%snull value in covariate column `%s` (row %lld)", error_prefix(OB_E_POLARS),
                    c.name.c_str(), (long long)r);
    out.push_back(&c);
  }
  return OB_OK;
}

// engine.rs:144-229 from the two groups' rows on: `value(j, row)` is covariate j of a frame row
template <class V>
int match_groups(ob_ctx* ctx, int64_t n_rows, const Groups& g, int dim, int k, bool mahalanobis, V value,
                 ob_match_results* res) {
  const int64_t nt = (int64_t)g.treated.size(), nc = (int64_t)g.control.size();
  std::vector<double> xt((size_t)nt * dim), xc((size_t)nc * dim);
  for (int j = 0; j < dim; ++j) {
    for (int64_t i = 0; i < nt; ++i) xt[(size_t)j * nt + i] = value(j, g.treated[i]);
    for (int64_t i = 0; i < nc; ++i) xc[(size_t)j * nc + i] = value(j, g.control[i]);
  }
  std::vector<uint32_t> counts(nc, 0u);
  res->neighbor_rows.assign((size_t)nt * k, -1);
  res->dist2.assign((size_t)nt * k, 0.0);
  MatchTiming tm;
  OB_TRY(match_knn(ctx, xt.data(), std::max<int64_t>(nt, 1), nt, xc.data(), std::max<int64_t>(nc, 1), nc, dim, k,
                   mahalanobis, res->neighbor_rows.data(), res->dist2.data(), counts.data(), &tm));
  uint32_t m_max = 0;
  for (uint32_t m : counts) m_max = std::max(m_max, m);
  const std::vector<double> table = weight_table(std::max(k, 1), m_max);
  res->weights.assign((size_t)n_rows, 0.0);
  for (int64_t r : g.treated) res->weights[r] = 1.0;                             // engine.rs:215-218
  for (int64_t i = 0; i < nc; ++i) res->weights[g.control[i]] = table[counts[i]];  // engine.rs:221-226
  for (int64_t& v : res->neighbor_rows)
    if (v >= 0) v = g.control[v];
  res->treated_rows = g.treated;
  res->n_treated = nt;
  res->n_control = nc;
  res->k = k;
  res->knn_ms += tm.knn_ms;
  res->prep_ms += tm.prep_ms;
  return OB_OK;
}

int match_run(ob_ctx* ctx, const Frame& f, const ob_match_config* cfg, ob_match_results* res) {
  const int dim = cfg->n_covariates, k = cfg->k;
  if (k < 0) return fail(OB_E_INVALID, "negative k");
  if (dim > OB_MATCH_MAX_DIM)
    return fail(OB_E_UNSUPPORTED, "matching: %d covariates, the kernel takes at most %d", dim, OB_MATCH_MAX_DIM);
  if (k > OB_MATCH_MAX_K)
    return fail(OB_E_UNSUPPORTED, "matching: k = %d, the kernel keeps at most %d neighbours", k, OB_MATCH_MAX_K);
  const int64_t n = f.nrows;
  const Col* tcol = nullptr;
  Groups g;
  OB_TRY(split_groups(f, cfg->treatment, &tcol, g));
  if (cfg->method == OB_MATCH_PSM && (g.treated.empty() || g.control.empty()))  // engine.rs:56-60
    return fail(OB_E_GROUP, "%sOne group is empty", error_prefix(OB_E_GROUP));
  std::vector<const Col*> xcols;
  OB_TRY(covariate_columns(f, cfg, xcols));
  if (cfg->method != OB_MATCH_PSM) {
    if (dim <= 0) return fail(OB_E_INVALID, "matching needs at least one covariate");
    return match_groups(ctx, n, g, dim, k, cfg->method == OB_MATCH_MAHALANOBIS,
                        [&](int j, int64_t r) { return col_value(*xcols[j], r); }, res);
  }
  // prepare_data's outcome checks (engine.rs:78-92), then `.f64()?` of the treatment (engine.rs:255)
  if (!cfg->outcome) return fail(OB_E_INVALID, "PSM needs an outcome column name");
  const int oi = f.find(cfg->outcome);
  if (oi < 0) return polars_not_found(cfg->outcome);
  const Col& oc = f.cols[oi];
  if (oc.kind != OB_COL_F64)
    return fail(OB_E_POLARS, "%sinvalid series dtype: expected `Float64`, got `%s` for `%s`", error_prefix(OB_E_POLARS),
                dtype_name(oc.kind), oc.name.c_str());
  for (const auto* rows : {&g.treated, &g.control})
    for (int64_t r : *rows)
      if (!oc.valid[r]) return fail(OB_E_GROUP, "%sNull values in outcomes", error_prefix(OB_E_GROUP));
  if (tcol->kind != OB_COL_F64)
    return fail(OB_E_POLARS, "%sinvalid series dtype: expected `Float64`, got `%s` for `%s`", error_prefix(OB_E_POLARS),
                dtype_name(tcol->kind), tcol->name.c_str());
  const int kk = dim + 1;
  if (kk > kLogitMaxK)
    return fail(OB_E_UNSUPPORTED, "PSM: %d logistic columns, the kernel takes at most %d (intercept included)", kk,
                kLogitMaxK);
  // intercept and the covariates of ALL rows; the raw treatment value, null as 0.0 (engine.rs:250-260)
  std::vector<double> x((size_t)n * kk), y(n), beta(kk), scores(n);
  std::fill(x.begin(), x.begin() + n, 1.0);
  for (int j = 0; j < dim; ++j)
    for (int64_t r = 0; r < n; ++r) x[(size_t)(j + 1) * n + r] = col_value(*xcols[j], r);
  for (int64_t r = 0; r < n; ++r) y[r] = tcol->valid[r] ? tcol->f[r] : 0.0;
  LogitInfo li;
  OB_TRY(match_logistic(ctx, x.data(), n, y.data(), n, kk, 100, 1e-6, beta.data(), scores.data(), &li));
  res->iterations = li.iterations;
  res->converged = li.converged;
  res->prep_ms += li.ms;
  return match_groups(ctx, n, g, 1, k, false, [&](int, int64_t r) { return scores[r]; }, res);  // engine.rs:276-282
}

}  // namespace

int mahalanobis_factor(const std::vector<double>& s, int d, std::vector<double>& l) {
  std::vector<double> inv;
  if (!try_inverse(s, d, inv))  // distance.rs:48-50
    return fail(OB_E_DIAG, "%sCovariance matrix is singular and cannot be inverted", error_prefix(OB_E_DIAG));
  // nalgebra Cholesky::new on the lower triangle, then l() (engine.rs:163-167)
  l = inv;
  if (!chol_factor(l.data(), d)) return fail(OB_E_DIAG, "%sCholesky decomposition failed", error_prefix(OB_E_DIAG));
  for (int j = 0; j < d; ++j)
    for (int i = 0; i < j; ++i) l[i + (size_t)j * d] = 0.0;
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_knn(ob_ctx* ctx, const double* queries, int64_t ldq, int64_t n_q, const double* controls, int64_t ldc,
           int64_t n_c, int32_t dim, int32_t k, int64_t* idx, double* dist2) {
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer");
  return ob::match_knn(ctx, queries, ldq, n_q, controls, ldc, n_c, dim, k, false, idx, dist2, nullptr, nullptr);
}

int ob_match_logistic(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k,
                      int32_t max_iter, double tol, double* beta, double* probs, int32_t* converged,
                      int32_t* iterations) {
  if (!ctx || !x || !y || !beta) return ob::fail(OB_E_INVALID, "null pointer");
  ob::LogitInfo li;
  OB_TRY(ob::match_logistic(ctx, x, ldx, y, n, k, max_iter, tol, beta, probs, &li));
  if (converged) *converged = li.converged;
  if (iterations) *iterations = li.iterations;
  return OB_OK;
}

int ob_match_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_match_config* cfg,
                 ob_match_results** out) {
  if (!ctx || !cfg || !out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (!cfg->treatment) return ob::fail(OB_E_INVALID, "incomplete matching config");
  if (cfg->method < OB_MATCH_EUCLIDEAN || cfg->method > OB_MATCH_PSM) return ob::fail(OB_E_INVALID, "unknown method");
  ob::Frame f;
  OB_TRY(ob::load_frame(cols, n_cols, n_rows, f));
  auto res = new ob_match_results();
  const int rc = ob::match_run(ctx, f, cfg, res);
  if (rc != OB_OK) {
    delete res;
    return rc;
  }
  *out = res;
  return OB_OK;
}

int ob_match_results_get(const ob_match_results* r, int64_t* n_rows, const double** weights, int64_t* n_treated,
                         int32_t* k_out, const int64_t** treated_rows, const int64_t** neighbor_rows,
                         const double** neighbor_dist2) {
  if (!r) return ob::fail(OB_E_INVALID, "null pointer");
  if (n_rows) *n_rows = (int64_t)r->weights.size();
  if (weights) *weights = r->weights.data();
  if (n_treated) *n_treated = r->n_treated;
  if (k_out) *k_out = r->k;
  if (treated_rows) *treated_rows = r->treated_rows.data();
  if (neighbor_rows) *neighbor_rows = r->neighbor_rows.data();
  if (neighbor_dist2) *neighbor_dist2 = r->dist2.data();
  return OB_OK;
}

int ob_match_results_info(const ob_match_results* r, ob_match_info* out) {
  if (!r || !out) return ob::fail(OB_E_INVALID, "null pointer");
  out->n_treated = r->n_treated;
  out->n_control = r->n_control;
  out->logistic_iterations = r->iterations;
  out->logistic_converged = r->converged;
  out->knn_ms = r->knn_ms;
  out->prep_ms = r->prep_ms;
  return OB_OK;
}

void ob_match_results_free(ob_match_results* r) { delete r; }

}  // extern "C"
