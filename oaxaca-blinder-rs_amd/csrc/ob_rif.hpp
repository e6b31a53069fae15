// ob_rif.hpp -- RIF statistics: the argument checks of ob_host.cpp, the device pass of
// ob_rif.hip and the hook through which ob_builder.cpp reaches it.
#pragma once
#include <cstdint>

#include "ob_common.hpp"

struct ob_ctx;

namespace ob {

constexpr int kRifThreads = 256;                         // threads of a scan block
constexpr int kRifItems = 4;                             // consecutive sorted values per thread
constexpr int kRifScanBlock = kRifThreads * kRifItems;   // sorted values per scan block and per sum piece
constexpr int64_t kRifMaxRows = (int64_t)1 << 28;        // the panel's own row limit per group

// ob_host.cpp, host only: the statistic and its parameters; then n, the values and what the Gini needs of them.
int rif_spec_check(const ob_rif_spec* specs, int n_specs);
int rif_input_check(const double* y, int64_t n, const ob_rif_spec* specs, int n_specs);

// The weighted pass: rif_wspec_check also accepts OB_RIF_QUANTILE; rif_input_check_weighted adds
// the weights' checks (finite, non-negative, a positive sum) and makes the Gini's over the rows with w > 0.
int rif_wspec_check(const ob_rif_spec* specs, int n_specs);
int rif_input_check_weighted(const double* y, const double* w, int64_t n, const ob_rif_spec* specs, int n_specs);

// ob_rif.hip: one group's outcome, every statistic from one sort. rif: [n_specs][n] in y's row order,
// stats: [n_specs]. Adds its HIP-event times to the thread's ob_rif_timing; reset = start it from zero.
int rif_device(ob_ctx* ctx, const double* y, int64_t n, const ob_rif_spec* specs, int n_specs, double* rif,
               double* stats, bool reset);
// The same with weights w[n] (host memory, as y): the kernels wrif_* of ob_rif.hip.
int rif_device_weighted(ob_ctx* ctx, const double* y, const double* w, int64_t n, const ob_rif_spec* specs,
                        int n_specs, double* rif, double* stats, bool reset);

// ob_builder.cpp reaches the device pass through this hook only, so that it still links without ob_rif.hip
// (the sanitizer build of the host code, tests/asan). ob_rif.hip installs it when the library loads.
struct RifHooks {
  int (*device)(ob_ctx* ctx, const double* y, int64_t n, const ob_rif_spec* specs, int n_specs, double* rif,
                double* stats, bool reset) = nullptr;
  int (*device_weighted)(ob_ctx* ctx, const double* y, const double* w, int64_t n, const ob_rif_spec* specs,
                         int n_specs, double* rif, double* stats, bool reset) = nullptr;
};
RifHooks& rif_hooks();  // ob_builder.cpp

}  // namespace ob
