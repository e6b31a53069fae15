// ob_jackknife.cpp -- the host pieces of the jackknife / BCa inference: the stratified
// acceleration, jackknife standard error and bias from the device pass's power sums, the BCa interval over
// replicate values, the array entry points of the C ABI and the builder's (a prepared run's jackknife, finish
// and run with BCa intervals). Of the array entry points only ob_jackknife and ob_jackknife_rows need a GPU.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ob_builder.hpp"
#include "ob_common.hpp"
#include "ob_host.hpp"
#include "ob_jackknife.hpp"
#include "ob_model.hpp"

namespace ob {

static thread_local double g_jack_ms = 0.0;

int jackknife_check_shape(int k, int64_t n_a, int64_t n_b, int n_norm, int n_y, int heckman, int want_rows) {
  if (k < 1 || n_a < 0 || n_b < 0 || n_norm < 0 || n_y < 0) return fail(OB_E_INVALID, "bad jackknife dimensions");
  if (heckman) return fail(OB_E_UNSUPPORTED, "jackknife: Heckman selection panels are outside its scope");
  if (n_norm > 0) return fail(OB_E_UNSUPPORTED, "jackknife: normalized categoricals are outside its scope");
  if (n_y > 1) return fail(OB_E_UNSUPPORTED, "jackknife: one outcome at a time");
  if (k > kJackMaxK)
    return fail(OB_E_UNSUPPORTED, "jackknife: %d design columns exceed OB_JACK_MAX_K = %d", k, kJackMaxK);
  if (want_rows && n_a + n_b > kJackMaxRows)
    return fail(OB_E_UNSUPPORTED, "jackknife: the rows output takes at most 2^24 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k + 1)
      return fail(OB_E_INSUFFICIENT,
                  "%sInsufficient data for a leave-one-out fit: n_obs (%lld) must be strictly greater than k + 1 (%d)",
                  error_prefix(OB_E_INSUFFICIENT), (long long)n, k + 1);
  return OB_OK;
}

void jackknife_finish(const double* sums, const int64_t kept[2], int c, double* stats) {
  for (int j = 0; j < c; ++j) {
    double u2 = 0.0, u3 = 0.0, se2 = 0.0, bias = 0.0;
    for (int g = 0; g < 2; ++g) {
      if (kept[g] <= 0) continue;
      const double m = (double)kept[g];
      const double* s = sums + ((size_t)g * c + j) * 3;
      const double dbar = s[0] / m;
      const double g2 = s[1] - m * dbar * dbar;
      const double g3 = -(s[2] - 3.0 * dbar * s[1] + 2.0 * m * dbar * dbar * dbar);
      u2 += g2;
      u3 += g3;
      se2 += (m - 1.0) / m * g2;
      bias += (m - 1.0) * dbar;
    }
    const double den = 6.0 * std::pow(std::max(u2, 0.0), 1.5);
    stats[3 * j] = den > 0.0 ? u3 / den : 0.0;
    stats[3 * j + 1] = std::sqrt(std::max(se2, 0.0));
    stats[3 * j + 2] = bias;
  }
}

static inline bool nan_last(double a, double b) {  // the order of ob_host.cpp's bootstrap_stats
  if (std::isnan(a)) return false;
  if (std::isnan(b)) return true;
  return a < b;
}

void bca_stats(const double* v, int64_t n, double point, double accel, double level, double out[6]) {
  out[0] = out[1] = out[2] = out[3] = out[4] = NAN;
  out[5] = 0.0;
  if (n <= 0) {
    out[5] = 1.0;
    return;
  }
  const double nf = (double)n;
  int64_t below = 0, equal = 0;
  for (int64_t i = 0; i < n; ++i) {
    below += v[i] < point;
    equal += v[i] == point;
  }
  const double p0 = ((double)below + 0.5 * (double)equal) / nf;
  if (!(p0 > 0.0 && p0 < 1.0)) {
    out[5] = 2.0;
    return;
  }
  const double z0 = ob_normal_inverse_cdf(p0);
  out[2] = z0;
  if (!std::isfinite(accel)) {
    out[5] = 3.0;
    return;
  }
  const double alpha[2] = {(1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0};
  int64_t idx[2];
  for (int e = 0; e < 2; ++e) {
    const double q = z0 + ob_normal_inverse_cdf(alpha[e]);
    const double den = 1.0 - accel * q;
    if (!(den > 0.0)) {
      out[5] = 4.0;
      out[3] = out[4] = NAN;
      return;
    }
    const double ap = 0.5 * std::erfc(-(z0 + q / den) / std::sqrt(2.0));
    out[3 + e] = ap;
    idx[e] = std::min<int64_t>((int64_t)std::floor(ap * nf), n - 1);
  }
  std::vector<double> s(v, v + n);
  std::nth_element(s.begin(), s.begin() + idx[1], s.end(), nan_last);
  out[1] = s[idx[1]];
  if (idx[0] < idx[1]) std::nth_element(s.begin(), s.begin() + idx[0], s.begin() + idx[1], nan_last);
  out[0] = s[idx[0]];
}

}  // namespace ob

extern "C" {

int ob_jackknife_check_shape(int32_t k, int64_t n_a, int64_t n_b, int32_t n_norm, int32_t n_y, int32_t heckman,
                             int32_t want_rows) {
  return ob::jackknife_check_shape(k, n_a, n_b, n_norm, n_y, heckman, want_rows);
}

static int jack_check_panel(const ob_panel* p, int ref_mode, int want_rows) {
  if (!p) return ob::fail(OB_E_INVALID, "null pointer");
  if (ref_mode < OB_REF_GROUP_A || ref_mode > OB_REF_NEUMARK)
    return ob::fail(OB_E_INVALID, "unknown reference coefficients %d", ref_mode);
  return ob::jackknife_check_shape(p->heckman ? p->k - 1 : p->k, p->n[0], p->n[1], p->norm.n_norm, p->n_y, p->heckman,
                                   want_rows);
}

int ob_jackknife(ob_panel* panel, int ref_mode, ob_jackknife_out* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  OB_TRY(jack_check_panel(panel, ref_mode, 0));
  const int c = 6 + 2 * panel->k;
  if (out->capacity < c || !out->point || !out->sums || !out->stats)
    return ob::fail(OB_E_INVALID, "jackknife: the output arrays must hold %d components", c);
  ob::JackResult r;
  OB_TRY(ob::jackknife_device(panel, ref_mode, r, nullptr, nullptr));
  ob::g_jack_ms = r.ms;
  out->n_components = c;
  for (int g = 0; g < 2; ++g) {
    out->n_used[g] = r.kept[g];
    out->n_dropped[g] = r.dropped[g];
  }
  std::copy(r.point.begin(), r.point.end(), out->point);
  std::copy(r.sums.begin(), r.sums.end(), out->sums);
  ob::jackknife_finish(out->sums, out->n_used, c, out->stats);
  return OB_OK;
}

int ob_jackknife_rows(ob_panel* panel, int ref_mode, double* theta, uint8_t* kept, int64_t* n_dropped) {
  OB_TRY(jack_check_panel(panel, ref_mode, 1));
  if (!theta || !kept) return ob::fail(OB_E_INVALID, "null pointer");
  ob::JackResult r;
  OB_TRY(ob::jackknife_device(panel, ref_mode, r, theta, kept));
  ob::g_jack_ms = r.ms;
  if (n_dropped) {
    n_dropped[0] = r.dropped[0];
    n_dropped[1] = r.dropped[1];
  }
  return OB_OK;
}

int ob_jackknife_last_timing(double* pass_ms) {
  if (pass_ms) *pass_ms = ob::g_jack_ms;
  return OB_OK;
}

int ob_jackknife_finish(const double* sums, const int64_t* n_used, int32_t n_components, double* stats) {
  if (n_components < 0 || (n_components > 0 && (!sums || !stats)) || !n_used || n_used[0] < 0 || n_used[1] < 0)
    return ob::fail(OB_E_INVALID, "bad arguments");
  ob::jackknife_finish(sums, n_used, n_components, stats);
  return OB_OK;
}

int ob_bca_stats(const double* estimates, int64_t n, double point_estimate, double accel, double level, double out[6]) {
  if (!out || n < 0 || (n > 0 && !estimates)) return ob::fail(OB_E_INVALID, "bad arguments");
  if (!(level > 0.0 && level < 1.0)) return ob::fail(OB_E_INVALID, "the confidence level must lie in (0, 1)");
  ob::bca_stats(estimates, n, point_estimate, accel, level, out);
  return OB_OK;
}

int ob_aggregate_bca(const double* rows, const uint8_t* ok, uint64_t n_reps, int32_t row_len, const int32_t* cols,
                     int32_t n_cols, const double* point, const double* accel, double level, double* out) {
  if (n_cols < 0 || row_len <= 0 || (n_cols > 0 && (!cols || !out || !point || !accel)) || (n_reps > 0 && (!rows || !ok)))
    return ob::fail(OB_E_INVALID, "bad arguments");
  if (!(level > 0.0 && level < 1.0)) return ob::fail(OB_E_INVALID, "the confidence level must lie in (0, 1)");
  for (int32_t c = 0; c < n_cols; ++c)
    if (cols[c] < 0 || cols[c] >= row_len) return ob::fail(OB_E_INVALID, "column %d out of range", cols[c]);
  std::vector<double> v;
  v.reserve(n_reps);
  for (int32_t c = 0; c < n_cols; ++c) {
    v.clear();
    for (uint64_t r = 0; r < n_reps; ++r)
      if (ok[r]) v.push_back(rows[r * (uint64_t)row_len + cols[c]]);
    ob::bca_stats(v.data(), (int64_t)v.size(), point[c], accel[c], level, out + 6 * (size_t)c);
  }
  return OB_OK;
}

}  // extern "C"

// ---- the builder's entry points (handles of ob_builder.hpp) ------------------------------------------------
namespace ob {

// ob::finish, then every component's interval through bca_stats over the same pooled values that aggregate()
// gave bootstrap_stats (a detailed component pools the columns that share its name, builder.rs:963-971).
int finish_bca(const ob_prepared* pr, const double* rows, const uint8_t* ok, uint64_t n_reps, double level,
               ob_results** out) {
  OB_TRY(finish(pr, 0, rows, ok, n_reps, out));
  ob_results* res = *out;
  const int k = pr->k, rl = pr->row_len;  // n_norm = 0: kd = k
  const int tables[4][2] = {{OB_TABLE_TWO_FOLD, 0}, {OB_TABLE_THREE_FOLD, 2}, {OB_TABLE_DETAILED_EXPLAINED, 6},
                            {OB_TABLE_DETAILED_UNEXPLAINED, 6 + k}};
  std::vector<double> v;
  std::vector<int> cols;
  for (const auto& t : tables) {
    std::vector<ob_results::Comp>& comps = res->tables[t[0]];
    const bool detailed = t[1] >= 6;
    for (size_t i = 0; i < comps.size(); ++i) {
      const int own = t[1] + (int)i;
      cols.clear();
      if (detailed) {
        for (int q = 0; q < k; ++q)
          if (pr->detail_names[q] == pr->detail_names[i]) cols.push_back(t[1] + q);
      } else {
        cols.push_back(own);
      }
      v.clear();
      for (uint64_t r = 0; r < n_reps; ++r)
        if (ok[r])
          for (int c : cols) v.push_back(rows[r * (uint64_t)rl + c]);
      const double* js = pr->jack_stats.data() + 3 * (size_t)own;
      double b6[6];
      bca_stats(v.data(), (int64_t)v.size(), comps[i].estimate, js[0], level, b6);
      comps[i].ci_lower = b6[0];
      comps[i].ci_upper = b6[1];
      const double jk[5] = {js[0], js[1], js[2], b6[2], b6[5]};
      std::copy(jk, jk + 5, comps[i].jack);
    }
  }
  res->has_jack = true;
  return OB_OK;
}

// The checks of ob_prepared_jackknife and ob_prepared_finish_bca, before any device work.
static int prepared_jack_check(const ob_prepared* p) {
  if (!p) return fail(OB_E_INVALID, "null pointer");
  if (p->cluster)  // delete-one-row is the wrong jackknife under clustering
    return fail(OB_E_UNSUPPORTED, "jackknife: a clustered run takes the delete-one-cluster pass "
                                  "(ob_prepared_cluster_jackknife, ob_prepared_finish_cluster_bca)");
  if (p->model)
    return fail(OB_E_UNSUPPORTED, "jackknife: %s (BCa included) are outside its scope", model_name(p->model_kind).plural);
  const bool heck = !p->selection_names.empty();
  return jackknife_check_shape(heck ? p->k - 1 : p->k, p->n_a, p->n_b, p->n_base > 0 || !p->cfg.normalize.empty(),
                               p->n_y, heck, 0);
}

static int prepared_jack_run(ob_prepared* p) {
  if (p->has_jack) return OB_OK;
  const int c = 6 + 2 * p->k;
  std::vector<double> point(c), sums((size_t)6 * c);
  p->jack_stats.assign((size_t)3 * c, 0.0);
  ob_jackknife_out o = {};
  o.capacity = c;
  o.point = point.data();
  o.sums = sums.data();
  o.stats = p->jack_stats.data();
  OB_TRY(ob_jackknife(p->panel, p->ref, &o));
  p->jack.c = c;
  p->jack.point = point;
  p->jack.sums = sums;
  for (int g = 0; g < 2; ++g) {
    p->jack.kept[g] = o.n_used[g];
    p->jack.dropped[g] = o.n_dropped[g];
  }
  p->has_jack = true;
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_prepared_jackknife(ob_prepared* p, ob_jackknife_out* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  OB_TRY(ob::prepared_jack_check(p));
  const int c = 6 + 2 * p->k;
  if (out->capacity < c || !out->point || !out->sums || !out->stats)
    return ob::fail(OB_E_INVALID, "jackknife: the output arrays must hold %d components", c);
  OB_TRY(ob::prepared_jack_run(p));
  out->n_components = c;
  for (int g = 0; g < 2; ++g) {
    out->n_used[g] = p->jack.kept[g];
    out->n_dropped[g] = p->jack.dropped[g];
  }
  std::copy(p->jack.point.begin(), p->jack.point.end(), out->point);
  std::copy(p->jack.sums.begin(), p->jack.sums.end(), out->sums);
  std::copy(p->jack_stats.begin(), p->jack_stats.end(), out->stats);
  return OB_OK;
}

int ob_prepared_finish_bca(ob_prepared* p, const double* rows, const uint8_t* ok, uint64_t n_reps, double level,
                           ob_results** out) {
  if (!p || !out || (n_reps && (!rows || !ok))) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (!(level > 0.0 && level < 1.0)) return ob::fail(OB_E_INVALID, "the confidence level must lie in (0, 1)");
  OB_TRY(ob::prepared_jack_check(p));
  OB_TRY(ob::prepared_jack_run(p));
  return ob::finish_bca(p, rows, ok, n_reps, level, out);
}

int ob_builder_run_bca(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                       double level, ob_results** out) {
  if (!ctx || !out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (!(level > 0.0 && level < 1.0)) return ob::fail(OB_E_INVALID, "the confidence level must lie in (0, 1)");
  ob::Frame f;
  ob::Config c;
  OB_TRY(ob::config_from(cfg, c));
  if (c.has_selection) return ob::fail(OB_E_UNSUPPORTED, "jackknife: Heckman selection panels are outside its scope");
  if (!c.normalize.empty()) return ob::fail(OB_E_UNSUPPORTED, "jackknife: normalized categoricals are outside its scope");
  OB_TRY(ob::load_frame(cols, n_cols, n_rows, f));
  ob_prepared* pr = nullptr;
  OB_TRY(ob::prepare(ctx, f, c, &pr));
  int rc = ob::prepared_jack_check(pr);
  std::vector<double> rows((size_t)c.reps * pr->row_len);
  std::vector<uint8_t> ok(c.reps, 0);
  if (rc == OB_OK && c.reps > 0) rc = ob_boot_run(pr->panel, pr->seed, 0, c.reps, pr->ref, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::prepared_jack_run(pr);
  if (rc == OB_OK) rc = ob::finish_bca(pr, rows.data(), ok.data(), c.reps, level, out);
  ob_prepared_destroy(pr);
  return rc;
}

int ob_results_jackknife(const ob_results* r, int32_t table, int32_t i, double* out) {
  if (!r || !out || table < 0 || table > 4 || i < 0 || i >= (int)r->tables[table].size())
    return ob::fail(OB_E_INVALID, "bad arguments");
  if (!r->has_jack || table == OB_TABLE_DETAILED_SELECTION)
    return ob::fail(OB_E_INVALID, "this result carries no jackknife statistics");
  std::copy(r->tables[table][i].jack, r->tables[table][i].jack + 5, out);
  return OB_OK;
}

}  // extern "C"
