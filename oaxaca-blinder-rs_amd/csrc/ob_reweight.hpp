// ob_reweight.hpp -- the reweighted Oaxaca-Blinder decomposition with a bootstrapped propensity logit
// (Fortin, Lemieux and Firpo 2011, section 5): limits and row layout (ob_reweight.hip holds the
// rest; ob_builder.cpp routes a handle through the hooks of ob_model.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ob_prepared;

namespace ob {

constexpr int kReweightMaxK = 32;  // design columns with the intercept (OB_REWEIGHT_MAX_K)
// Row (include/oaxaca_boot.h): 7 aggregates | 4 K detailed | beta_A, beta_B, beta_C, xbar_A, xbar_B, xbar_C,
// gamma (K each) | ybar_A, ybar_B, ybar_C | effective sample size | logit passes.
inline int reweight_row_len(int k) { return 7 + 11 * k + 5; }
// The checks every entry point makes before any device work. k: design columns with the intercept.
int reweight_check_shape(int k, int64_t n_a, int64_t n_b);

// The decomposition of a statistic keeps this row and the same hooks: its handle is a reweighted
// handle whose outcome columns are the weighted RIFs in A, B and C, fixed at the point estimate (a replicate
// refits the logit and the three regressions and does not recompute the statistic).

}  // namespace ob
