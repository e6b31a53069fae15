// ob_cluster.cpp -- the host side of the cluster bootstrap: cluster ids -> dense ids in
// order of first appearance, per group a stable permutation of its rows by cluster id with CSR offsets,
// the limits checked before any device work, and the host-only entry points of the C ABI.
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "ob_builder.hpp"
#include "ob_cluster.hpp"
#include "ob_common.hpp"

namespace ob {

int cluster_check_shape(int64_t n_clusters, int k1) {
  if (n_clusters < 0 || k1 < 2 || k1 > 122) return fail(OB_E_INVALID, "bad cluster dimensions");
  if (n_clusters < 2)
    return fail(OB_E_INSUFFICIENT, "%scluster bootstrap: %lld cluster(s); resampling needs at least 2",
                error_prefix(OB_E_INSUFFICIENT), (long long)n_clusters);
  if (n_clusters >= kClusterMax)
    return fail(OB_E_UNSUPPORTED, "cluster bootstrap: %lld clusters; the limit is 2^24 - 1", (long long)n_clusters);
  const uint64_t e_pad = (uint64_t)(((int64_t)k1 * (k1 + 1) / 2 + 15) / 16 * 16);
  if ((uint64_t)n_clusters * 2 * (e_pad + 1) * sizeof(double) > kClusterQBytes)
    return fail(OB_E_UNSUPPORTED, "cluster bootstrap: the per-cluster Grams of %lld clusters x %d columns exceed 8 GiB",
                (long long)n_clusters, k1);
  return OB_OK;
}

int cluster_index(const Col& ids, const int32_t* group, int64_t n_rows, bool stratified, ClusterIndex& out) {
  if (ids.kind != OB_COL_STR && ids.kind != OB_COL_I64)
    return fail(OB_E_INVALID, "cluster column `%s` has dtype `%s`: a string or an integer column is expected",
                ids.name.c_str(), dtype_name(ids.kind));
  out = ClusterIndex();
  out.stratified = stratified ? 1 : 0;
  out.dense.assign((size_t)n_rows, -1);
  std::unordered_map<std::string, int32_t> by_str;
  std::unordered_map<int64_t, int32_t> by_int;
  std::vector<uint8_t> in_group;  // per cluster: bit 0 has rows in A, bit 1 in B
  std::vector<int64_t> first_row;
  for (int64_t r = 0; r < n_rows; ++r) {
    const int g = group[r];
    if ((g != 0 && g != 1) || !ids.valid[r]) continue;
    if (in_group.size() >= (size_t)kClusterMax)
      return fail(OB_E_UNSUPPORTED, "cluster bootstrap: more than 2^24 - 1 clusters");
    const int32_t next = (int32_t)in_group.size();
    const int32_t id = ids.kind == OB_COL_STR ? by_str.emplace(ids.s[r], next).first->second
                                              : by_int.emplace(ids.i[r], next).first->second;
    if (id == next) {
      in_group.push_back(0);
      first_row.push_back(r);
    }
    in_group[id] |= (uint8_t)(1 << g);
    out.dense[r] = id;
  }
  const int64_t nc = (int64_t)in_group.size();
  auto label = [&](int32_t id) {
    const int64_t r = first_row[id];
    return ids.kind == OB_COL_STR ? ids.s[r] : std::to_string(ids.i[r]);
  };
  if (stratified) {  // every cluster in exactly one group; A's clusters first, each side in first-appearance order
    std::vector<int32_t> renum((size_t)nc);
    int32_t na = 0;
    for (int32_t c = 0; c < nc; ++c) {
      if (in_group[c] == 3)
        return fail(OB_E_INVALID, "stratified cluster bootstrap: cluster `%s` of column `%s` has rows in both groups",
                    label(c).c_str(), ids.name.c_str());
      if (in_group[c] == 1) renum[c] = na++;
    }
    int32_t nb = na;
    for (int32_t c = 0; c < nc; ++c)
      if (in_group[c] == 2) renum[c] = nb++;
    for (auto& d : out.dense)
      if (d >= 0) d = renum[d];
    std::vector<uint8_t> ig((size_t)nc);
    for (int32_t c = 0; c < nc; ++c) ig[renum[c]] = in_group[c];
    in_group.swap(ig);
  }
  out.n_clusters = nc;
  for (int64_t c = 0; c < nc; ++c) {
    out.c_a += in_group[c] & 1;
    out.c_b += (in_group[c] >> 1) & 1;
  }
  std::vector<int64_t> total((size_t)nc, 0);
  for (int g = 0; g < 2; ++g) {  // counting sort of the group's kept rows by cluster id: stable
    std::vector<int64_t>& off = out.off[g];
    off.assign((size_t)nc + 1, 0);
    int64_t ng = 0;
    for (int64_t r = 0; r < n_rows; ++r)
      if (group[r] == g && out.dense[r] >= 0) {
        ++off[out.dense[r] + 1];
        ++ng;
      }
    for (int64_t c = 0; c < nc; ++c) {
      total[c] += off[c + 1];
      off[c + 1] += off[c];
    }
    out.perm[g].assign((size_t)ng, 0);
    std::vector<int64_t> fill(off.begin(), off.end() - 1);
    int64_t pos = 0;
    for (int64_t r = 0; r < n_rows; ++r)
      if (group[r] == g && out.dense[r] >= 0) out.perm[g][fill[out.dense[r]]++] = pos++;
  }
  for (int64_t c = 0; c < nc; ++c) out.max_rows = std::max(out.max_rows, total[c]);
  return OB_OK;
}

// ---- the delete-one-cluster jackknife: the checks, the handle's pass and its statistics -------
static thread_local double g_cluster_jack_ms = 0.0;
void cluster_jack_set_timing(double ms) { g_cluster_jack_ms = ms; }

int cluster_jack_check_shape(int k, int64_t n_clusters, int n_norm, int n_y, int heckman, int want_rows) {
  if (k < 1 || n_clusters < 0 || n_norm < 0 || n_y < 0) return fail(OB_E_INVALID, "bad cluster jackknife dimensions");
  if (heckman) return fail(OB_E_UNSUPPORTED, "cluster jackknife: Heckman selection panels are outside its scope");
  if (n_norm > 0) return fail(OB_E_UNSUPPORTED, "cluster jackknife: normalized categoricals are outside its scope");
  if (n_y > 1) return fail(OB_E_UNSUPPORTED, "cluster jackknife: one outcome at a time");
  if (k > kClusterJackMaxK)
    return fail(OB_E_UNSUPPORTED, "cluster jackknife: %d design columns exceed OB_CLUSTER_JACK_MAX_K = %d", k,
                kClusterJackMaxK);
  if (n_clusters >= kClusterMax)
    return fail(OB_E_UNSUPPORTED, "cluster jackknife: %lld clusters; the limit is 2^24 - 1", (long long)n_clusters);
  (void)want_rows;  // the rows output goes back batch by batch into the caller's C x row_len array: no further limit
  if (n_clusters < 2)
    return fail(OB_E_INSUFFICIENT, "%scluster jackknife: %lld cluster(s); deleting one needs at least 2",
                error_prefix(OB_E_INSUFFICIENT), (long long)n_clusters);
  return OB_OK;
}

// The checks of the prepared entry points, before any device work.
static int prepared_cluster_jack_check(const ob_prepared* p, int want_rows) {
  if (!p) return fail(OB_E_INVALID, "null pointer");
  if (!p->cluster) return fail(OB_E_INVALID, "this prepared run is not clustered");
  // no clustered handle of these kinds exists today; BCa for them stays out of scope when one does
  if (p->model)
    return fail(OB_E_UNSUPPORTED, "cluster jackknife: binary, reweighted and distribution-regression decompositions "
                                  "(BCa included) are outside its scope");
  if (!cluster_hooks().jack || !cluster_hooks().info) return fail(OB_E_UNSUPPORTED, "this build carries no cluster jackknife");
  ob_cluster_info ci;
  cluster_hooks().info(p->cluster, &ci);
  const bool heck = !p->selection_names.empty();
  return cluster_jack_check_shape(heck ? p->k - 1 : p->k, ci.n_clusters, p->n_base > 0 || !p->cfg.normalize.empty(), p->n_y,
                                  heck, want_rows);
}

// Fewer than 2 kept clusters in a stratum that has any leaves no jackknife variance there.
int cluster_jack_enough(const JackResult& r) {
  for (int s = 0; s < 2; ++s)
    if (r.kept[s] + r.dropped[s] > 0 && r.kept[s] < 2)
      return fail(OB_E_INSUFFICIENT, "%scluster jackknife: %lld of %lld clusters of stratum %d have a fit without them; 2 are needed",
                  error_prefix(OB_E_INSUFFICIENT), (long long)r.kept[s], (long long)(r.kept[s] + r.dropped[s]), s);
  return OB_OK;
}

static int prepared_cluster_jack_run(ob_prepared* p) {
  if (p->has_jack) return OB_OK;
  JackResult r;
  OB_TRY(cluster_hooks().jack(p, r, nullptr, nullptr, nullptr));
  g_cluster_jack_ms = r.ms;
  OB_TRY(cluster_jack_enough(r));
  p->jack_stats.assign((size_t)3 * r.c, 0.0);
  jackknife_finish(r.sums.data(), r.kept, r.c, p->jack_stats.data());  // a stratum is a group to it
  p->jack = r;
  p->has_jack = true;
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_cluster_jackknife_check_shape(int32_t k, int64_t n_clusters, int32_t n_norm, int32_t n_y, int32_t heckman,
                                     int32_t want_rows) {
  return ob::cluster_jack_check_shape(k, n_clusters, n_norm, n_y, heckman, want_rows);
}

int ob_prepared_cluster_jackknife(ob_prepared* p, ob_jackknife_out* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  OB_TRY(ob::prepared_cluster_jack_check(p, 0));
  const int c = 6 + 2 * p->k;
  if (out->capacity < c || !out->point || !out->sums || !out->stats)
    return ob::fail(OB_E_INVALID, "cluster jackknife: the output arrays must hold %d components", c);
  OB_TRY(ob::prepared_cluster_jack_run(p));
  out->n_components = c;
  for (int s = 0; s < 2; ++s) {
    out->n_used[s] = p->jack.kept[s];
    out->n_dropped[s] = p->jack.dropped[s];
  }
  std::copy(p->jack.point.begin(), p->jack.point.end(), out->point);
  std::copy(p->jack.sums.begin(), p->jack.sums.end(), out->sums);
  std::copy(p->jack_stats.begin(), p->jack_stats.end(), out->stats);
  return OB_OK;
}

int ob_prepared_cluster_jackknife_rows(ob_prepared* p, double* theta, uint8_t* kept, int64_t* n_dropped,
                                       double* deviations) {
  OB_TRY(ob::prepared_cluster_jack_check(p, 1));
  if (!theta || !kept) return ob::fail(OB_E_INVALID, "null pointer");
  ob::JackResult r;
  OB_TRY(ob::cluster_hooks().jack(p, r, theta, kept, deviations));
  ob::g_cluster_jack_ms = r.ms;
  if (n_dropped) {
    n_dropped[0] = r.dropped[0];
    n_dropped[1] = r.dropped[1];
  }
  return OB_OK;  // no statistics are formed here: a stratum with fewer than 2 kept clusters is there to be inspected
}

int ob_prepared_finish_cluster_bca(ob_prepared* p, const double* rows, const uint8_t* ok, uint64_t n_reps, double level,
                                   ob_results** out) {
  if (!p || !out || (n_reps && (!rows || !ok))) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (!(level > 0.0 && level < 1.0)) return ob::fail(OB_E_INVALID, "the confidence level must lie in (0, 1)");
  OB_TRY(ob::prepared_cluster_jack_check(p, 0));
  OB_TRY(ob::prepared_cluster_jack_run(p));
  return ob::finish_bca(p, rows, ok, n_reps, level, out);
}

int ob_builder_run_clustered_bca(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                 const ob_builder_config* cfg, const ob_cluster_config* ccfg, double level,
                                 ob_results** out) {
  if (!ctx || !out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (!(level > 0.0 && level < 1.0)) return ob::fail(OB_E_INVALID, "the confidence level must lie in (0, 1)");
  ob::Config c;
  OB_TRY(ob::config_from(cfg, c));
  if (c.has_selection) return ob::fail(OB_E_UNSUPPORTED, "cluster jackknife: Heckman selection panels are outside its scope");
  if (!c.normalize.empty())
    return ob::fail(OB_E_UNSUPPORTED, "cluster jackknife: normalized categoricals are outside its scope");
  ob_prepared* pr = nullptr;
  OB_TRY(ob_builder_prepare_clustered(ctx, cols, n_cols, n_rows, cfg, ccfg, &pr));
  int rc = ob::prepared_cluster_jack_check(pr, 0);
  const uint64_t reps = pr->cfg.reps;
  std::vector<double> rows((size_t)reps * pr->row_len);
  std::vector<uint8_t> ok(reps, 0);
  if (rc == OB_OK && reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::prepared_cluster_jack_run(pr);
  if (rc == OB_OK) rc = ob::finish_bca(pr, rows.data(), ok.data(), reps, level, out);
  ob_prepared_destroy(pr);
  return rc;
}

int ob_cluster_jackknife_last_timing(double* pass_ms) {
  if (pass_ms) *pass_ms = ob::g_cluster_jack_ms;
  return OB_OK;
}

int ob_cluster_check_shape(int64_t n_clusters, int32_t k1) { return ob::cluster_check_shape(n_clusters, k1); }

int ob_cluster_index(const ob_column* ids, const int32_t* group, int64_t n_rows, int32_t stratified, int32_t* dense,
                     int64_t* perm_a, int64_t* perm_b, int64_t* off_a, int64_t* off_b, ob_cluster_info* info) {
  if (!ids || n_rows < 0 || (n_rows > 0 && !group)) return ob::fail(OB_E_INVALID, "null pointer");
  ob::Frame f;
  OB_TRY(ob::load_frame(ids, 1, n_rows, f));
  ob::ClusterIndex ix;
  OB_TRY(ob::cluster_index(f.cols[0], group, n_rows, stratified != 0, ix));
  if (dense) std::copy(ix.dense.begin(), ix.dense.end(), dense);
  int64_t* perm[2] = {perm_a, perm_b};
  int64_t* off[2] = {off_a, off_b};
  for (int g = 0; g < 2; ++g) {
    if (perm[g]) std::copy(ix.perm[g].begin(), ix.perm[g].end(), perm[g]);
    if (off[g]) std::copy(ix.off[g].begin(), ix.off[g].end(), off[g]);
  }
  if (info) *info = {ix.n_clusters, ix.c_a, ix.c_b, ix.max_rows, ix.stratified};
  return OB_OK;
}

int ob_prepared_cluster_info(const ob_prepared* prep, ob_cluster_info* out) {
  if (!prep || !out) return ob::fail(OB_E_INVALID, "null pointer");
  if (!prep->cluster) return ob::fail(OB_E_INVALID, "this prepared run is not clustered");
  ob::cluster_hooks().info(prep->cluster, out);
  return OB_OK;
}

}  // extern "C"
