// ob_cluster.hpp -- the cluster bootstrap: the host cluster index of ob_cluster.cpp and
// the device passes of ob_cluster.hip (per-cluster Grams Q, the OBRC-1 counts, counts x Q on the f64
// matrix units), with the state a clustered ob_prepared carries.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ob_engine.hpp"
#include "ob_frame.hpp"
#include "ob_jackknife.hpp"

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

// ---- the delete-one-cluster jackknife (ob_cluster_jack.hip, host pieces in ob_cluster.cpp) ----
constexpr int kClusterJackMaxK = OB_CLUSTER_JACK_MAX_K;

// What the pass reads of a clustered handle (ob_cluster.hip). cluster_view forms Q if no boot has yet.
struct ClusterView {
  const double* q = nullptr;        // device [C][2][e_pad]
  const uint32_t* qrows = nullptr;  // device [C][2]
  uint32_t n_clusters = 0, n_clusters_a = 0;
  int stratified = 0;
};
int cluster_view(ob_prepared* pr, hipStream_t s, ClusterView& out);
// d_total[width] = sum_c Q[c] (Q: device, [C][width]), in cluster order in ob_cluster_apply's runs of 8,192 (a
// function of C alone).
int cluster_sum_q(const double* d_q, uint32_t n_clusters, int width, double* d_total, hipStream_t s);
// ob_cluster_guard_kernel over rows s0 .. s0 + ns of a call of n_reps.
int cluster_guard(const ob_panel* p, const uint32_t* d_rep_rows, uint32_t ns, uint64_t n_reps, uint64_t s0, double* d_rows,
                  uint8_t* d_ok, hipStream_t s);

// The checks every cluster-jackknife entry point makes before any device work. k: design columns with the intercept.
int cluster_jack_check_shape(int k, int64_t n_clusters, int n_norm, int n_y, int heckman, int want_rows);
// The point estimate the pass starts from, on the host. One outcome: k1 = k + 1.
struct ClusterPoint {
  int k = 0, k1 = 0, e_pad = 0, weighted = 0, ref_mode = 0;
  uint32_t n[2] = {0, 0};
  const double* gram = nullptr;  // the two extended Grams [2][e_pad]
  const double* tail = nullptr;  // beta_A, beta_B, xbar_A, xbar_B, beta* (5 k)
};
// The `sums` pass on arrays. out.kept / out.dropped / out.sums are per STRATUM: all C clusters as stratum 0 in
// joint mode, A's then B's clusters in stratified mode; out.point is theta_hat recomputed from pt. kept (host, C
// bytes) and dev (host, C x (6 + 2K): every cluster's deviations themselves, NaN where dropped) may be NULL.
int cluster_jack_pass(ob_ctx* ctx, const ClusterView& cv, const ClusterPoint& pt, JackResult& out, uint8_t* kept,
                      double* dev);
// The `rows` output on arrays: theta (host, C x row_len) from the panel's solve kernel; kept holds the pass's mask
// on entry and the final one on return; out.kept / out.dropped are recounted.
int cluster_jack_rows(ob_panel* p, const ClusterView& cv, const ClusterPoint& pt, double* theta, uint8_t* kept,
                      JackResult& out);
// Both over a clustered handle: theta and kept NULL for the `sums` output alone.
int cluster_jack_device(ob_prepared* pr, JackResult& out, double* theta, uint8_t* kept, double* dev);
// ob_cluster.cpp: fewer than 2 kept clusters in a stratum that has any is OB_E_INSUFFICIENT; the thread's last pass time
int cluster_jack_enough(const JackResult& r);
void cluster_jack_set_timing(double ms);

// ob_builder.cpp reaches the cluster code through these hooks only, so that it still links without
// ob_cluster.cpp / ob_cluster.hip (the sanitizer build of the host code, tests/asan). ob_cluster.hip installs
// them when the library loads (ob_cluster_jack.hip its own, `jack`); without them a clustered call is
// OB_E_UNSUPPORTED.
struct ClusterHooks {
  int (*jack)(ob_prepared* pr, JackResult& out, double* theta, uint8_t* kept, double* dev) = nullptr;
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
