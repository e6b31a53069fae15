// ob_dfl.hpp -- device entry points of the DFL reweighting path (ob_dfl.hip), called by the C ABI
// in ob_dfl.cpp. All pointers are host pointers; the routines stage them in HBM themselves.
#pragma once
#include <cstdint>

#include "ob_engine.hpp"

namespace ob {

// Columns (intercept included) the logit kernel takes: four 16-column MFMA blocks.
constexpr int kLogitMaxK = 64;

struct LogitInfo {
  int converged = 0;
  int iterations = 0;
  double ms = 0.0;  // HIP-event time of the Newton-pass launches (pass + reduce), summed
};

// math/logit.rs:31-118 with the n x K pass on the GPU. x: column-major n x k, ldx >= n; y: 0/1;
// beta[k] out; probs[n] out or NULL.
int dfl_logit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int k, int max_iter, double tol,
              double* beta, double* probs, LogitInfo* info);

// math/kde.rs:31-38 on the GPU. wnorm: the normalised weights (kde.rs:24-29) or NULL for 1 / n.
// ms (may be NULL) receives the HIP-event time of the launches.
int dfl_kde(ob_ctx* ctx, const double* data, const double* wnorm, int64_t n, const double* grid, int64_t n_grid,
            double bandwidth, double* density, double* ms);

}  // namespace ob
