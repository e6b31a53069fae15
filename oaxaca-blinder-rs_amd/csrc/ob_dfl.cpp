// ob_dfl.cpp -- C ABI of DiNardo-Fortin-Lemieux reweighting: `run_dfl` (oaxaca_blinder/src/dfl.rs)
// over a column frame, with the logit's Newton passes and the kernel densities on the MI355X
// (ob_dfl.hip).
//
//   run_dfl              dfl.rs:34-195
//   logit                math/logit.rs:31-118
//   kde                  math/kde.rs:20-41
//   silverman_bandwidth  math/kde.rs:44-59
// Polars semantics kept: unique + sort puts a null first, `.get(0)` of a null is None, a string
// compared with a null is null (so a null group row counts in neither n_a nor n_b while its logit
// target reads the null as ""), and nothing drops rows.
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "ob_common.hpp"
#include "ob_dfl.hpp"
#include "ob_frame.hpp"

struct ob_dfl_results {
  std::vector<double> grid, density_a, density_b, density_cf;
  int64_t n_a = 0, n_b = 0;
  int iterations = 0, converged = 0;
  double bandwidth_a = 0.0, bandwidth_b = 0.0;
  std::string group_a;
  double logit_ms = 0.0, kde_ms = 0.0;
};

namespace ob {

// math/kde.rs:44-59
static double silverman_bandwidth(const double* data, int64_t len) {
  const double n = (double)len;
  double sum = 0.0;
  for (int64_t i = 0; i < len; ++i) sum += data[i];
  const double mean = sum / n;
  double ss = 0.0;
  for (int64_t i = 0; i < len; ++i) ss += (data[i] - mean) * (data[i] - mean);
  const double std_dev = std::sqrt(ss / (n - 1.0));
  std::vector<double> sorted(data, data + len);
  std::stable_sort(sorted.begin(), sorted.end());  // partial_cmp order; NaNs are the caller's problem
  const double q1 = sorted[(size_t)(n * 0.25)];
  const double q3 = sorted[(size_t)(n * 0.75)];
  const double a = std::fmin(std_dev, (q3 - q1) / 1.34);  // f64::min ignores a NaN (n = 1)
  return 0.9 * a * std::pow(n, -0.2);
}

static int polars_not_found(const std::string& name) {
  return fail(OB_E_POLARS, "%snot found: %s", error_prefix(OB_E_POLARS), name.c_str());
}

static std::vector<std::string> levels_of(const Col& c, bool* has_null) {
  std::vector<std::string> lv;
  *has_null = false;
  for (size_t r = 0; r < c.s.size(); ++r) {
    if (c.valid[r]) lv.push_back(c.s[r]);
    else *has_null = true;
  }
  std::sort(lv.begin(), lv.end());
  lv.erase(std::unique(lv.begin(), lv.end()), lv.end());
  return lv;
}

// grid[i] = min + i * step exactly as two rounded operations (dfl.rs:171-172)
#pragma STDC FP_CONTRACT OFF
static void make_grid(double min_val, double max_val, int grid_size, std::vector<double>& grid) {
  const double range = max_val - min_val;
  const double step = range / (double)grid_size;
  grid.resize(grid_size);
  for (int i = 0; i < grid_size; ++i) {
    const volatile double t = (double)i * step;
    grid[i] = min_val + t;
  }
}

static int dfl_run(ob_ctx* ctx, const Frame& f, const ob_dfl_config* cfg, ob_dfl_results** out) {
  const std::string outcome = cfg->outcome, group = cfg->group, reference = cfg->reference_group;
  const int grid_size = cfg->grid_size == 0 ? 100 : cfg->grid_size;  // dfl.rs:170
  if (grid_size < 0) return fail(OB_E_INVALID, "negative grid_size");
  const int64_t n = f.nrows;
  // 1. target: 1 on group A's rows (dfl.rs:43-68)
  const int gi = f.find(group);
  if (gi < 0) return polars_not_found(group);
  const Col& g = f.cols[gi];
  if (g.kind != OB_COL_STR)
    return fail(OB_E_POLARS, "%sinvalid series dtype: expected `String`, got `%s` for `%s`", error_prefix(OB_E_POLARS),
                dtype_name(g.kind), g.name.c_str());
  bool g_null = false;
  const auto glev = levels_of(g, &g_null);
  // the sorted unique values with a null (if any) in front; .get(i) of the null is None
  auto uniq_get = [&](size_t i, const std::string& dflt) -> std::string {
    if (g_null) {
      if (i == 0) return dflt;
      --i;
    }
    return i < glev.size() ? glev[i] : dflt;
  };
  std::string name_a = uniq_get(0, reference);
  if (name_a == reference) name_a = uniq_get(1, "");
  std::vector<double> y(n);
  int64_t n_a = 0, n_b = 0;
  for (int64_t r = 0; r < n; ++r) {
    y[r] = ((g.valid[r] ? g.s[r] : std::string()) == name_a) ? 1.0 : 0.0;
    if (g.valid[r] && g.s[r] == name_a) ++n_a;     // dfl.rs:119-125
    if (g.valid[r] && g.s[r] == reference) ++n_b;  // dfl.rs:126-132
  }
  // design: intercept, then per predictor its dummies or its f64 cast (dfl.rs:75-103)
  struct XCol {
    const Col* src;
    std::string level;  // OB_COL_STR: the dummy's level
  };
  std::vector<XCol> xcols;
  if (cfg->n_predictors < 0 || (cfg->n_predictors > 0 && !cfg->predictors)) return fail(OB_E_INVALID, "bad name list");
  for (int p = 0; p < cfg->n_predictors; ++p) {
    if (!cfg->predictors[p]) return fail(OB_E_INVALID, "null name");
    const int ci = f.find(cfg->predictors[p]);
    if (ci < 0) return polars_not_found(cfg->predictors[p]);
    const Col& c = f.cols[ci];
    for (int64_t r = 0; r < n; ++r)
      if (!c.valid[r])  // stricter than the reference, whose to_ndarray would carry the null as NaN
        return fail(OB_E_POLARS, "%snull value in predictor column `%s` (row %lld)", error_prefix(OB_E_POLARS),
                    c.name.c_str(), (long long)r);
    if (c.kind == OB_COL_STR) {
      bool has_null = false;
      const auto lv = levels_of(c, &has_null);
      for (size_t l = 1; l < lv.size(); ++l) xcols.push_back({&c, lv[l]});
    } else {
      xcols.push_back({&c, std::string()});
    }
  }
  const int64_t k = 1 + (int64_t)xcols.size();
  if (k > kLogitMaxK)
    return fail(OB_E_UNSUPPORTED, "DFL: %lld logit columns, the kernel takes at most %d (intercept included)",
                (long long)k, kLogitMaxK);
  if (n_a == 0 || n_b == 0)  // stricter than the reference, which would divide by zero or index an empty vector
    return fail(OB_E_GROUP, "%sDFL needs rows in both groups: %lld in `%s`, %lld in reference `%s`",
                error_prefix(OB_E_GROUP), (long long)n_a, name_a.c_str(), (long long)n_b, reference.c_str());
  std::vector<double> x((size_t)n * k);
  std::fill(x.begin(), x.begin() + n, 1.0);
  for (size_t c = 0; c < xcols.size(); ++c) {
    double* dst = x.data() + (c + 1) * (size_t)n;
    const Col& s = *xcols[c].src;
    if (s.kind == OB_COL_STR) {
      for (int64_t r = 0; r < n; ++r) dst[r] = s.s[r] == xcols[c].level ? 1.0 : 0.0;
    } else if (s.kind == OB_COL_I64) {
      for (int64_t r = 0; r < n; ++r) dst[r] = (double)s.i[r];
    } else {
      std::copy(s.f.begin(), s.f.end(), dst);
    }
  }
  // 2. propensity score (dfl.rs:111-112)
  std::vector<double> beta(k), probs(n);
  LogitInfo li;
  OB_TRY(dfl_logit(ctx, x.data(), n, y.data(), n, (int)k, 100, 1e-6, beta.data(), probs.data(), &li));
  // 3. weights (dfl.rs:118-160)
  const double nn = (double)n;
  const double ratio_marginal = ((double)n_b / nn) / ((double)n_a / nn);
  const int oi = f.find(outcome);
  if (oi < 0) return polars_not_found(outcome);
  const Col& oc = f.cols[oi];
  if (oc.kind != OB_COL_F64)  // `.f64()?` (dfl.rs:139)
    return fail(OB_E_POLARS, "%sinvalid series dtype: expected `Float64`, got `%s` for `%s`", error_prefix(OB_E_POLARS),
                dtype_name(oc.kind), outcome.c_str());
  std::vector<double> w_cf, out_a, out_b;
  for (int64_t r = 0; r < n; ++r) {
    if (!oc.valid[r]) return fail(OB_E_GROUP, "%sNull outcome encountered in DFL", error_prefix(OB_E_GROUP));
    if (y[r] == 0.0) {
      double p = probs[r];
      p = p < 0.0001 ? 0.0001 : (p > 0.9999 ? 0.9999 : p);
      w_cf.push_back((p / (1.0 - p)) * ratio_marginal);
      out_b.push_back(oc.f[r]);
    } else {
      out_a.push_back(oc.f[r]);
    }
  }
  // 4. densities (dfl.rs:164-187)
  double min_val = std::numeric_limits<double>::infinity(), max_val = -min_val;
  for (int64_t r = 0; r < n; ++r) {
    min_val = std::fmin(min_val, oc.f[r]);
    max_val = std::fmax(max_val, oc.f[r]);
  }
  auto res = new ob_dfl_results();
  make_grid(min_val, max_val, grid_size, res->grid);
  res->bandwidth_a = silverman_bandwidth(out_a.data(), (int64_t)out_a.size());
  res->bandwidth_b = silverman_bandwidth(out_b.data(), (int64_t)out_b.size());
  double wsum = 0.0;
  for (double w : w_cf) wsum += w;
  std::vector<double> wn(w_cf.size());
  for (size_t i = 0; i < w_cf.size(); ++i) wn[i] = w_cf[i] / wsum;  // kde.rs:24-26
  res->density_a.resize(grid_size);
  res->density_b.resize(grid_size);
  res->density_cf.resize(grid_size);
  double ms[3] = {0.0, 0.0, 0.0};
  int rc = dfl_kde(ctx, out_a.data(), nullptr, (int64_t)out_a.size(), res->grid.data(), grid_size, res->bandwidth_a,
                   res->density_a.data(), &ms[0]);
  if (rc == OB_OK)
    rc = dfl_kde(ctx, out_b.data(), nullptr, (int64_t)out_b.size(), res->grid.data(), grid_size, res->bandwidth_b,
                 res->density_b.data(), &ms[1]);
  if (rc == OB_OK)
    rc = dfl_kde(ctx, out_b.data(), wn.data(), (int64_t)out_b.size(), res->grid.data(), grid_size, res->bandwidth_b,
                 res->density_cf.data(), &ms[2]);
  if (rc != OB_OK) {
    delete res;
    return rc;
  }
  res->n_a = n_a;
  res->n_b = n_b;
  res->iterations = li.iterations;
  res->converged = li.converged;
  res->group_a = name_a;
  res->logit_ms = li.ms;
  res->kde_ms = ms[0] + ms[1] + ms[2];
  *out = res;
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_logit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k, int32_t max_iter,
             double tol, double* beta, double* probs, int32_t* converged, int32_t* iterations) {
  if (!ctx || !x || !y || !beta) return ob::fail(OB_E_INVALID, "null pointer");
  ob::LogitInfo li;
  OB_TRY(ob::dfl_logit(ctx, x, ldx, y, n, k, max_iter, tol, beta, probs, &li));
  if (converged) *converged = li.converged;
  if (iterations) *iterations = li.iterations;
  return OB_OK;
}

int ob_kde(ob_ctx* ctx, const double* data, const double* weights, int64_t n, const double* grid, int64_t n_grid,
           double bandwidth, double* density) {
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer");
  if (!weights || n <= 0) return ob::dfl_kde(ctx, data, nullptr, n, grid, n_grid, bandwidth, density, nullptr);
  double sum = 0.0;
  for (int64_t i = 0; i < n; ++i) sum += weights[i];
  std::vector<double> wn(n);
  for (int64_t i = 0; i < n; ++i) wn[i] = weights[i] / sum;  // kde.rs:24-26
  return ob::dfl_kde(ctx, data, wn.data(), n, grid, n_grid, bandwidth, density, nullptr);
}

int ob_silverman_bandwidth(const double* data, int64_t n, double* out) {
  if (!out || n <= 0 || !data) return ob::fail(OB_E_INVALID, "silverman_bandwidth needs at least one value");
  *out = ob::silverman_bandwidth(data, n);
  return OB_OK;
}

int ob_dfl_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_dfl_config* cfg,
               ob_dfl_results** out) {
  if (!ctx || !cfg || !out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (!cfg->outcome || !cfg->group || !cfg->reference_group) return ob::fail(OB_E_INVALID, "incomplete DFL config");
  ob::Frame f;
  OB_TRY(ob::load_frame(cols, n_cols, n_rows, f));
  return ob::dfl_run(ctx, f, cfg, out);
}

int ob_dfl_results_get(const ob_dfl_results* r, int64_t* n_grid, const double** grid, const double** density_a,
                       const double** density_b, const double** density_b_counterfactual) {
  if (!r) return ob::fail(OB_E_INVALID, "null pointer");
  if (n_grid) *n_grid = (int64_t)r->grid.size();
  if (grid) *grid = r->grid.data();
  if (density_a) *density_a = r->density_a.data();
  if (density_b) *density_b = r->density_b.data();
  if (density_b_counterfactual) *density_b_counterfactual = r->density_cf.data();
  return OB_OK;
}

int ob_dfl_results_info(const ob_dfl_results* r, ob_dfl_info* out) {
  if (!r || !out) return ob::fail(OB_E_INVALID, "null pointer");
  out->n_a = r->n_a;
  out->n_b = r->n_b;
  out->logit_iterations = r->iterations;
  out->logit_converged = r->converged;
  out->bandwidth_a = r->bandwidth_a;
  out->bandwidth_b = r->bandwidth_b;
  out->group_a = r->group_a.c_str();
  out->logit_ms = r->logit_ms;
  out->kde_ms = r->kde_ms;
  return OB_OK;
}

void ob_dfl_results_free(ob_dfl_results* r) { delete r; }

}  // extern "C"
