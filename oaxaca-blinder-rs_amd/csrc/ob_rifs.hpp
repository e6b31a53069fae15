// ob_rifs.hpp -- the per-replicate RIF of the variance, the Gini and quantile ranges over resample counts
// (DESIGN.md §5.19): limits and the checks every entry point makes before any device work (ob_rifs.hip holds the
// kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ob_common.hpp"
#include "ob_rifq.hpp"

struct ob_prepared;

namespace ob {

constexpr int kRifsMaxK = kRifqMaxK;  // design columns with the intercept
constexpr int kRifsMaxStats = 8;      // statistics of one pass
constexpr int kRifsMaxReps = 16384;   // replicates of one ob_rifs_pass

// The statistics of a pass and the distinct quantiles, ascending, that its ranges share.
struct RifsPlan {
  int n_specs = 0, n_taus = 0;
  int stat[kRifsMaxStats] = {};
  int hi[kRifsMaxStats] = {}, lo[kRifsMaxStats] = {};  // a range's quantiles as indices into taus
  double taus[kRifqMaxTaus] = {};
  bool variance = false, gini = false, range = false;
};
// More than kRifsMaxStats statistics, or more than kRifqMaxTaus distinct quantiles over the ranges:
// OB_E_UNSUPPORTED; an unknown statistic or bad range parameters: OB_E_INVALID.
int rifs_plan(const ob_rif_spec* specs, int n_specs, RifsPlan& out);
// k: design columns with the intercept; a group needs more than k rows and at least two.
int rifs_check_shape(int k, const ob_rif_spec* specs, int n_specs, int64_t n_a, int64_t n_b);

}  // namespace ob
