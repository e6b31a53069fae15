// ob_akm.cpp -- C ABI of the reference's AKM module over a column frame, with the group means, the
// Gram and the R^2 sums on the MI355X (ob_akm.hip).
//
//   find_largest_connected_set  akm.rs:151-234   (host: union-find over the worker-firm graph)
//   solve_akm                   akm.rs:236-449
//   demean_vector               akm.rs:452-527
//   recover_fe                  akm.rs:530-621
// The one deliberate difference: among components with equally many nodes the one holding the
// smallest sorted worker id is kept (include/oaxaca_boot.h); the reference's pick follows HashMap
// iteration order.
#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "ob_akm.hpp"
#include "ob_common.hpp"
#include "ob_frame.hpp"
#include "ob_linalg.hpp"

struct ob_akm_set {
  std::vector<uint8_t> keep;
  std::vector<int32_t> widx, fidx;         // per kept row
  std::vector<std::string> wids, fids;     // sorted kept ids
  int64_t n_components = 0;
};

struct ob_akm_results {
  std::vector<double> beta, alpha, psi;
  std::vector<std::string> wids, fids;
  std::vector<const char*> wptr, fptr;
  std::vector<int32_t> demean_iters;
  double r2 = 0.0;
  int64_t n_kept = 0, n_components = 0;
  int32_t recover_iters = 0, launches = 0;
  double demean_ms = 0.0, ols_ms = 0.0, recover_ms = 0.0;
};

namespace ob {

namespace {

const char kNotEnough[] = "Not enough data: ";  // AkmError's Display (akm.rs:20-33)

int convergence_failed(const std::string& what) {
  return fail(OB_E_CONVERGENCE, "Convergence failed: %s. Try increasing max_iters or checking for collinearity.",
              what.c_str());
}

struct UnionFind {  // akm.rs:114-148
  std::vector<int32_t> parent, size;
  explicit UnionFind(size_t n) : parent(n), size(n, 1) { std::iota(parent.begin(), parent.end(), 0); }
  int32_t find(int32_t i) {
    int32_t root = i;
    while (parent[root] != root) root = parent[root];
    while (parent[i] != root) {
      const int32_t next = parent[i];
      parent[i] = root;
      i = next;
    }
    return root;
  }
  void unite(int32_t i, int32_t j) {
    int32_t a = find(i), b = find(j);
    if (a == b) return;
    if (size[a] < size[b]) std::swap(a, b);
    parent[b] = a;
    size[a] += size[b];
  }
};

// The id column cast to strings: ids = the sorted distinct non-null values, code[r] = the position of
// row r's id in them (-1: null). An integer column is cast value by value to its decimal string.
int encode_ids(const Col& c, int64_t n, std::vector<std::string>& ids, std::vector<int32_t>& code) {
  if (c.kind == OB_COL_F64)
    return fail(OB_E_UNSUPPORTED, "AKM: id column `%s` is Float64; ids are strings or integers", c.name.c_str());
  code.assign((size_t)n, -1);
  std::vector<int32_t> rank;  // first-appearance number -> sorted position
  std::vector<int32_t> first((size_t)n, -1);
  std::vector<std::string> seen;
  if (c.kind == OB_COL_I64) {
    std::unordered_map<int64_t, int32_t> map;
    for (int64_t r = 0; r < n; ++r) {
      if (!c.valid[r]) continue;
      auto it = map.find(c.i[r]);
      if (it == map.end()) {
        if (seen.size() >= (size_t)INT32_MAX) return fail(OB_E_UNSUPPORTED, "AKM: 2^31 or more nodes");
        it = map.emplace(c.i[r], (int32_t)seen.size()).first;
        seen.push_back(std::to_string((long long)c.i[r]));
      }
      first[r] = it->second;
    }
  } else {
    std::unordered_map<std::string, int32_t> map;
    for (int64_t r = 0; r < n; ++r) {
      if (!c.valid[r]) continue;
      auto it = map.find(c.s[r]);
      if (it == map.end()) {
        if (seen.size() >= (size_t)INT32_MAX) return fail(OB_E_UNSUPPORTED, "AKM: 2^31 or more nodes");
        it = map.emplace(c.s[r], (int32_t)seen.size()).first;
        seen.push_back(c.s[r]);
      }
      first[r] = it->second;
    }
  }
  std::vector<int32_t> by(seen.size());
  std::iota(by.begin(), by.end(), 0);
  std::sort(by.begin(), by.end(), [&](int32_t a, int32_t b) { return seen[a] < seen[b]; });  // byte order, as polars
  rank.resize(seen.size());
  ids.resize(seen.size());
  for (size_t k = 0; k < by.size(); ++k) {
    rank[by[k]] = (int32_t)k;
    ids[k] = std::move(seen[by[k]]);
  }
  for (int64_t r = 0; r < n; ++r)
    if (first[r] >= 0) code[r] = rank[first[r]];
  return OB_OK;
}

int connected_set(const Frame& f, const char* worker_col, const char* firm_col, ob_akm_set* out) {
  const int64_t n = f.nrows;
  if (n >= (int64_t)INT32_MAX) return fail(OB_E_UNSUPPORTED, "AKM: 2^31 or more rows");
  const int wi = f.find(worker_col), fi = f.find(firm_col);
  if (wi < 0) return fail(OB_E_COLUMN, "%s%s", error_prefix(OB_E_COLUMN), worker_col);
  if (fi < 0) return fail(OB_E_COLUMN, "%s%s", error_prefix(OB_E_COLUMN), firm_col);
  std::vector<std::string> wall, fall;
  std::vector<int32_t> wcode, fcode;
  OB_TRY(encode_ids(f.cols[wi], n, wall, wcode));
  OB_TRY(encode_ids(f.cols[fi], n, fall, fcode));
  const int64_t nw = (int64_t)wall.size(), nf = (int64_t)fall.size();
  if (nw + nf >= (int64_t)INT32_MAX) return fail(OB_E_UNSUPPORTED, "AKM: 2^31 or more nodes");
  UnionFind uf((size_t)(nw + nf));
  for (int64_t r = 0; r < n; ++r)
    if (wcode[r] >= 0 && fcode[r] >= 0) uf.unite(wcode[r], (int32_t)(nw + fcode[r]));
  // node counts per root; the winner: most nodes, then the smallest worker position
  std::vector<int32_t> nodes((size_t)(nw + nf), 0), min_worker((size_t)(nw + nf), INT32_MAX);
  int64_t comps = 0;
  for (int64_t i = 0; i < nw + nf; ++i) {
    const int32_t root = uf.find((int32_t)i);
    if (nodes[root]++ == 0) ++comps;
    if (i < nw) min_worker[root] = std::min(min_worker[root], (int32_t)i);
  }
  int32_t best = -1;
  for (int64_t i = 0; i < nw + nf; ++i) {
    if (nodes[i] == 0) continue;
    if (best < 0 || nodes[i] > nodes[best] || (nodes[i] == nodes[best] && min_worker[i] < min_worker[best]))
      best = (int32_t)i;
  }
  out->n_components = comps;
  out->keep.assign((size_t)n, 0);
  int64_t kept = 0;
  for (int64_t r = 0; r < n; ++r)
    if (wcode[r] >= 0 && fcode[r] >= 0 && uf.find(wcode[r]) == best) {
      out->keep[r] = 1;
      ++kept;
    }
  if (kept == 0) return fail(OB_E_INSUFFICIENT, "%sNo connected set found", kNotEnough);  // akm.rs:94-98
  // dense indices over the kept ids, which keep their sorted order (akm.rs:246-303)
  std::vector<int32_t> wmap((size_t)nw, -1), fmap((size_t)nf, -1);
  for (int64_t r = 0; r < n; ++r)
    if (out->keep[r]) wmap[wcode[r]] = fmap[fcode[r]] = 0;
  for (int64_t i = 0; i < nw; ++i)
    if (wmap[i] == 0) {
      wmap[i] = (int32_t)out->wids.size();
      out->wids.push_back(wall[i]);
    }
  for (int64_t i = 0; i < nf; ++i)
    if (fmap[i] == 0) {
      fmap[i] = (int32_t)out->fids.size();
      out->fids.push_back(fall[i]);
    }
  out->widx.reserve((size_t)kept);
  out->fidx.reserve((size_t)kept);
  for (int64_t r = 0; r < n; ++r)
    if (out->keep[r]) {
      out->widx.push_back(wmap[wcode[r]]);
      out->fidx.push_back(fmap[fcode[r]]);
    }
  return OB_OK;
}

int check_indices(const int32_t* idx, int64_t n, int64_t n_groups, const char* what) {
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= n_groups)
      return fail(OB_E_INVALID, "AKM: %s index %d of row %lld is outside [0, %lld)", what, idx[i], (long long)i,
                  (long long)n_groups);
  return OB_OK;
}

int check_sizes(int64_t n, int64_t n_workers, int64_t n_firms) {
  if (n < 0 || n_workers < 0 || n_firms < 0) return fail(OB_E_INVALID, "AKM: negative size");
  if (n >= (int64_t)INT32_MAX) return fail(OB_E_UNSUPPORTED, "AKM: 2^31 or more rows");
  if (n_workers + n_firms >= (int64_t)INT32_MAX) return fail(OB_E_UNSUPPORTED, "AKM: 2^31 or more nodes");
  return OB_OK;
}

struct PlanHolder {
  AkmPlan* p = nullptr;
  ~PlanHolder() { akm_plan_free(p); }
};

int akm_run(ob_ctx* ctx, const Frame& f, const ob_akm_config* cfg, ob_akm_results* res) {
  const int k = cfg->n_controls;
  if (k < 0 || (k > 0 && !cfg->controls)) return fail(OB_E_INVALID, "bad name list");
  if (k > OB_AKM_MAX_CONTROLS)
    return fail(OB_E_UNSUPPORTED, "AKM: %d controls, the engine takes at most %d", k, OB_AKM_MAX_CONTROLS);
  const double tol = cfg->tolerance == 0.0 ? 1e-8 : cfg->tolerance;
  const int64_t max_iters = cfg->max_iters < 0 ? 1000 : cfg->max_iters;
  ob_akm_set set;
  OB_TRY(connected_set(f, cfg->worker_col, cfg->firm_col, &set));
  const int64_t n = (int64_t)set.widx.size();
  const int64_t nw = (int64_t)set.wids.size(), nf = (int64_t)set.fids.size();
  // the outcome and the controls of the kept rows, side by side per row (akm.rs:305-318)
  std::vector<const Col*> cols;
  for (int j = 0; j <= k; ++j) {
    const char* name = j == 0 ? cfg->outcome : cfg->controls[j - 1];
    if (!name) return fail(OB_E_INVALID, "null name");
    const int ci = f.find(name);
    if (ci < 0) return fail(OB_E_COLUMN, "%s%s", error_prefix(OB_E_COLUMN), name);
    const Col& c = f.cols[ci];
    if (c.kind != OB_COL_F64)
      return fail(OB_E_POLARS, "%sinvalid series dtype: expected `Float64`, got `%s` for `%s`",
                  error_prefix(OB_E_POLARS), dtype_name(c.kind), c.name.c_str());
    cols.push_back(&c);
  }
  const int nc = k + 1;
  std::vector<double> batch((size_t)n * nc);
  int64_t o = 0;
  for (int64_t r = 0; r < f.nrows; ++r) {
    if (!set.keep[r]) continue;
    if (!cols[0]->valid[r]) return fail(OB_E_INSUFFICIENT, "%sNull outcome encountered", kNotEnough);
    batch[(size_t)o * nc] = cols[0]->f[r];
    for (int j = 1; j < nc; ++j) batch[(size_t)o * nc + j] = cols[j]->valid[r] ? cols[j]->f[r] : 0.0;
    ++o;
  }
  PlanHolder plan;
  OB_TRY(akm_plan_create(ctx, n, set.widx.data(), set.fidx.data(), nw, nf, &plan.p));
  res->demean_iters.assign(nc, 0);
  std::vector<int32_t> conv(nc, 0);
  int launches = 0;
  OB_TRY(akm_demean(plan.p, batch.data(), nc, tol, max_iters, nullptr, res->demean_iters.data(), conv.data(),
                    &res->demean_ms, &launches));
  res->launches = launches;
  for (int j = 0; j < nc; ++j)
    if (!conv[j])  // akm.rs:519-524; the outcome first, then the controls in order
      return convergence_failed("demean_vector failed to converge within " + std::to_string((long long)max_iters) +
                                " iterations");
  res->beta.assign(k, 0.0);
  double ms = 0.0;
  if (k > 0) {  // akm.rs:352-364
    std::vector<double> g((size_t)nc * nc), xtx((size_t)k * k);
    OB_TRY(akm_gram(plan.p, g.data(), &ms));
    res->ols_ms += ms;
    for (int a = 0; a < k; ++a) {
      res->beta[a] = g[(size_t)(a + 1) * nc];
      for (int b = 0; b < k; ++b) xtx[a + (size_t)b * k] = g[(size_t)(a + 1) * nc + b + 1];
    }
    // the back substitution subtracts term by term, which is not nalgebra's order
    if (!chol_factor_solve(xtx.data(), k, res->beta.data(), BackSub::Sequential))
      return convergence_failed("OLS design matrix is singular");
  }
  OB_TRY(akm_residual(plan.p, res->beta.data(), &ms));
  res->ols_ms += ms;
  res->alpha.assign((size_t)nw, 0.0);
  res->psi.assign((size_t)nf, 0.0);
  int32_t fe_conv = 0;
  OB_TRY(akm_recover(plan.p, nullptr, tol, max_iters, res->alpha.data(), res->psi.data(), &res->recover_iters, &fe_conv,
                     &res->recover_ms));
  if (!fe_conv)  // akm.rs:604-609
    return convergence_failed("recover_fe failed to converge within " + std::to_string((long long)max_iters) +
                              " iterations");
  double tss = 0.0, rss = 0.0;
  OB_TRY(akm_r2(plan.p, res->beta.data(), &tss, &rss, &ms));
  res->ols_ms += ms;
  res->r2 = 1.0 - (rss / tss);
  res->wids = std::move(set.wids);
  res->fids = std::move(set.fids);
  for (const auto& s : res->wids) res->wptr.push_back(s.c_str());
  for (const auto& s : res->fids) res->fptr.push_back(s.c_str());
  res->n_kept = n;
  res->n_components = set.n_components;
  return OB_OK;
}

}  // namespace

}  // namespace ob

extern "C" {

int ob_akm_connected_set(const ob_column* cols, int32_t n_cols, int64_t n_rows, const char* worker_col,
                         const char* firm_col, ob_akm_set** out) {
  if (!out || !worker_col || !firm_col) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  ob::Frame f;
  OB_TRY(ob::load_frame(cols, n_cols, n_rows, f));
  auto set = new ob_akm_set();
  const int rc = ob::connected_set(f, worker_col, firm_col, set);
  if (rc != OB_OK) {
    delete set;
    return rc;
  }
  *out = set;
  return OB_OK;
}

int ob_akm_set_get(const ob_akm_set* s, int64_t* n_rows, const uint8_t** keep, int64_t* n_kept,
                   const int32_t** worker_idx, const int32_t** firm_idx, int64_t* n_workers, int64_t* n_firms,
                   int64_t* n_components) {
  if (!s) return ob::fail(OB_E_INVALID, "null pointer");
  if (n_rows) *n_rows = (int64_t)s->keep.size();
  if (keep) *keep = s->keep.data();
  if (n_kept) *n_kept = (int64_t)s->widx.size();
  if (worker_idx) *worker_idx = s->widx.data();
  if (firm_idx) *firm_idx = s->fidx.data();
  if (n_workers) *n_workers = (int64_t)s->wids.size();
  if (n_firms) *n_firms = (int64_t)s->fids.size();
  if (n_components) *n_components = s->n_components;
  return OB_OK;
}

const char* ob_akm_set_id(const ob_akm_set* s, int32_t which, int64_t i) {
  if (!s || i < 0) return nullptr;
  const auto& ids = which == 0 ? s->wids : s->fids;
  return i < (int64_t)ids.size() ? ids[(size_t)i].c_str() : nullptr;
}

void ob_akm_set_free(ob_akm_set* s) { delete s; }

int ob_akm_demean(ob_ctx* ctx, const double* v, int64_t ldv, int64_t n, int32_t n_cols, const int32_t* worker_idx,
                  const int32_t* firm_idx, int64_t n_workers, int64_t n_firms, double tol, int64_t max_iters,
                  double* out, int32_t* iterations, int32_t* converged) {
  if (!ctx || n_cols < 1 || ldv < n || (n && (!v || !out || !worker_idx || !firm_idx)))
    return ob::fail(OB_E_INVALID, "bad demean arguments");
  if (n_cols > OB_AKM_MAX_CONTROLS + 1)
    return ob::fail(OB_E_UNSUPPORTED, "AKM: %d columns, the engine takes at most %d", n_cols, OB_AKM_MAX_CONTROLS + 1);
  OB_TRY(ob::check_sizes(n, n_workers, n_firms));
  OB_TRY(ob::check_indices(worker_idx, n, n_workers, "worker"));
  OB_TRY(ob::check_indices(firm_idx, n, n_firms, "firm"));
  std::vector<double> batch((size_t)n * n_cols), res((size_t)n * n_cols);
  for (int c = 0; c < n_cols; ++c)
    for (int64_t r = 0; r < n; ++r) batch[(size_t)r * n_cols + c] = v[(size_t)c * ldv + r];
  ob::PlanHolder plan;
  OB_TRY(ob::akm_plan_create(ctx, n, worker_idx, firm_idx, n_workers, n_firms, &plan.p));
  OB_TRY(ob::akm_demean(plan.p, batch.data(), n_cols, tol, max_iters, res.data(), iterations, converged, nullptr,
                        nullptr));
  for (int c = 0; c < n_cols; ++c)
    for (int64_t r = 0; r < n; ++r) out[(size_t)c * ldv + r] = res[(size_t)r * n_cols + c];
  return OB_OK;
}

int ob_akm_recover_fe(ob_ctx* ctx, const double* r, int64_t n, const int32_t* worker_idx, const int32_t* firm_idx,
                      int64_t n_workers, int64_t n_firms, double tol, int64_t max_iters, double* alpha, double* psi,
                      int32_t* iterations, int32_t* converged) {
  if (!ctx || (n && (!r || !worker_idx || !firm_idx)) || (n_workers > 0 && !alpha) || (n_firms > 0 && !psi))
    return ob::fail(OB_E_INVALID, "bad recover_fe arguments");
  OB_TRY(ob::check_sizes(n, n_workers, n_firms));
  OB_TRY(ob::check_indices(worker_idx, n, n_workers, "worker"));
  OB_TRY(ob::check_indices(firm_idx, n, n_firms, "firm"));
  ob::PlanHolder plan;
  OB_TRY(ob::akm_plan_create(ctx, n, worker_idx, firm_idx, n_workers, n_firms, &plan.p));
  static const double zero = 0.0;
  return ob::akm_recover(plan.p, n ? r : &zero, tol, max_iters, alpha, psi, iterations, converged, nullptr);
}

int ob_akm_run(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_akm_config* cfg,
               ob_akm_results** out) {
  if (!ctx || !cfg || !out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (!cfg->outcome || !cfg->worker_col || !cfg->firm_col) return ob::fail(OB_E_INVALID, "incomplete AKM config");
  ob::Frame f;
  OB_TRY(ob::load_frame(cols, n_cols, n_rows, f));
  auto res = new ob_akm_results();
  const int rc = ob::akm_run(ctx, f, cfg, res);
  if (rc != OB_OK) {
    delete res;
    return rc;
  }
  *out = res;
  return OB_OK;
}

int ob_akm_results_get(const ob_akm_results* r, int32_t* n_controls, const double** beta, int64_t* n_workers,
                       const char* const** worker_ids, const double** worker_effects, int64_t* n_firms,
                       const char* const** firm_ids, const double** firm_effects, double* r2) {
  if (!r) return ob::fail(OB_E_INVALID, "null pointer");
  if (n_controls) *n_controls = (int32_t)r->beta.size();
  if (beta) *beta = r->beta.data();
  if (n_workers) *n_workers = (int64_t)r->alpha.size();
  if (worker_ids) *worker_ids = r->wptr.data();
  if (worker_effects) *worker_effects = r->alpha.data();
  if (n_firms) *n_firms = (int64_t)r->psi.size();
  if (firm_ids) *firm_ids = r->fptr.data();
  if (firm_effects) *firm_effects = r->psi.data();
  if (r2) *r2 = r->r2;
  return OB_OK;
}

int ob_akm_results_info(const ob_akm_results* r, ob_akm_info* out) {
  if (!r || !out) return ob::fail(OB_E_INVALID, "null pointer");
  out->n_rows_kept = r->n_kept;
  out->n_workers = (int64_t)r->alpha.size();
  out->n_firms = (int64_t)r->psi.size();
  out->n_components = r->n_components;
  out->demean_iterations = r->demean_iters.data();
  out->n_demean = (int32_t)r->demean_iters.size();
  out->recover_iterations = r->recover_iters;
  out->launches_per_iteration = r->launches;
  out->demean_ms = r->demean_ms;
  out->ols_ms = r->ols_ms;
  out->recover_ms = r->recover_ms;
  return OB_OK;
}

void ob_akm_results_free(ob_akm_results* r) { delete r; }

}  // extern "C"
