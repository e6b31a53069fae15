// ob_cluster.hpp -- the cluster bootstrap: the host cluster index of ob_cluster.cpp and
// the device passes of ob_cluster.hip (per-cluster Grams Q, the OBRC-1 counts, counts x Q on the f64
// matrix units), with the state a clustered ob_prepared carries.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ob_engine.hpp"
#include "ob_frame.hpp"

struct ob_prepared;

namespace ob {

constexpr int64_t kClusterMax = (int64_t)1 << 24;      // C stays below it (OBRC-1's rejection bound)
constexpr uint64_t kClusterQBytes = (uint64_t)8 << 30;  // Q: C * 2 * (e_pad + 1) doubles at most

// Dense ids in order of first appearance, per group a stable permutation by cluster id with CSR offsets.
struct ClusterIndex {
  int64_t n_clusters = 0, c_a = 0, c_b = 0, max_rows = 0;
  int stratified = 0;
  std::vector<int32_t> dense;     // per frame row, -1: in neither group or a null id
  std::vector<int64_t> perm[2];   // positions among the group's kept rows
  std::vector<int64_t> off[2];    // [C + 1]
};

int cluster_check_shape(int64_t n_clusters, int k1);
// ids over the frame's rows; group[r] = 0 / 1 or anything else for a row in neither group.
int cluster_index(const Col& ids, const int32_t* group, int64_t n_rows, bool stratified, ClusterIndex& out);

struct ClusterState;  // device side (ob_cluster.hip)
// Uploads the index of a prepared run's panel (the rows of the index are the panel's, group by group).
int cluster_attach(ob_prepared* pr, const ClusterIndex& idx);
void cluster_free(ClusterState* s);
void cluster_info(const ClusterState* s, ob_cluster_info* out);
int cluster_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                        hipStream_t stream);
int cluster_boot_host(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok);

// ob_builder.cpp reaches the cluster code through these hooks only, so that it still links without
// ob_cluster.cpp / ob_cluster.hip (the sanitizer build of the host code, tests/asan). ob_cluster.hip installs
// them when the library loads; without them a clustered call is OB_E_UNSUPPORTED.
struct ClusterHooks {
  int (*index)(const Col& ids, const int32_t* group, int64_t n_rows, bool stratified, int k1, ClusterIndex& out) = nullptr;
  int (*attach)(ob_prepared* pr, const ClusterIndex& idx) = nullptr;
  void (*free_state)(ClusterState* s) = nullptr;
  void (*info)(const ClusterState* s, ob_cluster_info* out) = nullptr;
  int (*boot_device)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                     hipStream_t stream) = nullptr;
  int (*boot_host)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok) = nullptr;
};
ClusterHooks& cluster_hooks();  // ob_builder.cpp

// ob_engine.hip: the solve of engine_boot over reduced Grams [ns][2][e_pad], every outcome; rep_rows
// ([ns][2], or NULL for the panel's own row counts) are the replicates' rows per group.
int engine_solve_grams(ob_panel* p, const double* d_gram, const uint32_t* d_rep_rows, uint32_t ns, uint64_t n_reps,
                       uint64_t s0, int ref_mode, double* d_rows, uint8_t* d_ok, hipStream_t s);

}  // namespace ob
