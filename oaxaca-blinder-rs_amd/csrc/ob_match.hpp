// ob_match.hpp -- device entry points of the matching path (ob_match.hip, and the matching
// logistic that shares ob_dfl.hip's Newton pass), called by the C ABI in ob_match.cpp. All pointers
// are host pointers; the routines stage them in HBM themselves.
#pragma once
#include <cstdint>
#include <vector>

#include "ob_dfl.hpp"

namespace ob {

struct MatchTiming {
  double knn_ms = 0.0;   // HIP-event time of the distance pass and its merge
  double prep_ms = 0.0;  // HIP-event time of the staging, covariance, transform, checks and packing
};

// The min(k, n_c) nearest controls of each query by the key (squared distance, position)
// (matching/engine.rs:178-209 without the tree). q: column-major n_q x dim, ldq >= n_q; c: column-major
// n_c x dim, ldc >= n_c. mahalanobis: both are first multiplied by the lower Cholesky factor of the
// inverse of c's covariance (engine.rs:148-176). idx / dist2: [n_q][k], -1 / +inf past min(k, n_c);
// counts (may be NULL): [n_c], how often each control was chosen.
int match_knn(ob_ctx* ctx, const double* q, int64_t ldq, int64_t n_q, const double* c, int64_t ldc, int64_t n_c, int dim,
              int k, bool mahalanobis, int64_t* idx, double* dist2, uint32_t* counts, MatchTiming* timing);

// matching/logistic.rs:31-113 with the n x K pass on the GPU (ob_dfl.hip): no probability clamp, a
// 1e-6 ridge, an LU solve; probs[n] (may be NULL) are the scores at the final beta.
int match_logistic(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int k, int max_iter,
                   double tol, double* beta, double* probs, LogitInfo* info);

// Host: s (d x d column-major, the covariance) -> l, the lower Cholesky factor of its inverse
// (distance.rs:48-50, engine.rs:163-167). OB_E_DIAG with the reference's messages.
int mahalanobis_factor(const std::vector<double>& s, int d, std::vector<double>& l);

}  // namespace ob
