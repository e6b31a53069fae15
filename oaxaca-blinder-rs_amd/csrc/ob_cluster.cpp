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

}  // namespace ob

extern "C" {

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
