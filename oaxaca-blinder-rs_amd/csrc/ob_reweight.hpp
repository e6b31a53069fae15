// ob_reweight.hpp -- the reweighted Oaxaca-Blinder decomposition with a bootstrapped propensity logit
// (Fortin, Lemieux and Firpo 2011, section 5): limits and row layout (ob_reweight.hip holds the
// rest; ob_builder.cpp routes a handle through the hooks of ob_model.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct ob_prepared;

namespace ob {

constexpr int kReweightMaxK = 32;  // design columns with the intercept (OB_REWEIGHT_MAX_K)
// Row (include/oaxaca_boot.h): 7 aggregates | 4 K detailed | beta_A, beta_B, beta_C, xbar_A, xbar_B, xbar_C,
// gamma (K each) | ybar_A, ybar_B, ybar_C | effective sample size | logit passes.
inline int reweight_row_len(int k) { return 7 + 11 * k + 5; }
// The checks every entry point makes before any device work. k: design columns with the intercept.
int reweight_check_shape(int k, int64_t n_a, int64_t n_b);

// The propensity logit of one batch of replicates, for the front ends that fit it (ob_reweight.hip, ob_density.hip):
// Newton from gamma = 0 over the stacked rows of both groups with D = 1[A] and weights c w, the clamp, the Cholesky
// step and the stopping rule of DESIGN.md §5.14, every replicate stopping on its own. cols[g]: [y | x_1 .. x_{k-1} |
// w] x ld[g], zero past n[g]; counts: the level-2 count images of the batch's first replicate block (NULL: every row
// once); chunks: [n_chunks][3] = (g, t0, t1).
struct LogitBatch {
  const double* cols[2];
  int64_t ld[2];
  uint32_t n[2];
  uint32_t tiles0;  // tiles of group A (the count images hold A's tiles first)
  int k;
  const uint32_t* counts;
  uint32_t nb_rep;  // 64-replicate blocks of the images
  const uint32_t* chunks;
  int n_chunks;
  uint32_t n_reps, part_pad;  // part_pad >= n_reps: the replicate stride of partial
  double* gamma;              // out [n_reps][k]
  uint32_t* flags;            // out [n_reps]: kLogitDoneBit | kLogitFailedBit
  uint32_t* passes;           // out [n_reps]: Newton passes taken
  uint32_t* active;           // one word of workspace
  double* partial;            // workspace [n_chunks][part_pad][reweight_logit_vals(k)]
};
constexpr uint32_t kLogitDoneBit = 1u, kLogitFailedBit = 2u;  // a replicate that is not done after the loop did not converge
struct LogitTimes {
  int32_t passes = 0, launches = 0;  // the longest batch's rounds; pass kernels over all batches
  double ms = 0.0;                   // the pass kernels (the steps not included)
};
size_t reweight_logit_vals(int k);
// Adds to *t. The host waits once per round (the count of replicates still iterating).
int reweight_logit_batch(const LogitBatch& b, hipStream_t s, LogitTimes* t);

// The decomposition of a statistic keeps this row and the same hooks: its handle is a reweighted
// handle whose outcome columns are the weighted RIFs in A, B and C, fixed at the point estimate (a replicate
// refits the logit and the three regressions and does not recompute the statistic).

}  // namespace ob
