// ob_rifq.hpp -- the per-replicate RIF of a quantile over resample counts: limits and the
// checks every entry point makes before any device work (ob_rifq.hip holds the kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ob_prepared;

namespace ob {

constexpr int kRifqMaxK = 32;    // design columns with the intercept
constexpr int kRifqMaxTaus = 8;  // quantiles of one pass
// Values per (chunk, replicate) of the density pass: kRifqMaxTaus slots of sum c phi((q_t - y) / bw), then sum c v_a
// for a < k over v = [1, x_1 .. x_{k-1}].
inline int rifq_sums_len(int k) { return kRifqMaxTaus + k; }
// tau in (0, 1), strictly increasing, at most kRifqMaxTaus of them.
int rifq_check_taus(const double* taus, int n_taus);
// k: design columns with the intercept; a group needs more than k rows and at least two.
int rifq_check_shape(int k, int n_taus, const double* taus, int64_t n_a, int64_t n_b);

// The arguments of ob_rifq.hip's kernels (ob_rifs.hip fills them for its quantile ranges).
struct RifqArgs {
  const double* cols[2];  // per group [k][ld]: y (ascending) | x_1 .. x_{k-1}
  int64_t ld[2];
  uint32_t n[2];
  uint32_t tile0[2];      // first tile of the group in m1 / the count images
  double mu0[2];          // the original sample's mean: the centre of the spread sums
  double npow[2];         // n_g^-0.2
  double taus[ob::kRifqMaxTaus];
  int k, n_taus, n_groups;
  uint32_t tiles_total;
  const uint32_t* m1;      // [replicate][tile] level-1 counts
  const uint32_t* counts;  // level-2 count images (ob_engine.hpp, the f64 Gram's layout); NULL: every row once
  uint32_t nb_rep, part_pad, n_reps;
  const uint32_t* chunks;  // [chunk][3] = (g, t0, t1)
  int n_chunks;
  // search -> density, patch: per (replicate, group)
  double* sq;     // [rep][g][T] quantiles
  uint32_t* sp;   // [rep][g][T] p_t
  double* sbw;    // [rep][g][3] bandwidth, mean, sd
  double* partial;  // [chunk][part_pad][kRifqMaxTaus + k]
  // patch outputs, per (replicate, group, tau)
  double* of;     // density after the floor
  double* onle;   // N_le
  uint8_t* ofl;   // 1 = the density was floored
  double* ot;     // [..][k] masked sums T_a
  double* ogy;    // [..][k + 1] G[a, y] for a < k, then G[y, y]
};
// The search, density and patch kernels over the replicates of `a` (every buffer set), enqueued on s; e[0] .. e[3]
// are recorded before the search and after each kernel.
int rifq_run(const RifqArgs& a, hipStream_t s, hipEvent_t* e);

}  // namespace ob
