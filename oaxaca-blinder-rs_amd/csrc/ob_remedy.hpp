// ob_remedy.hpp -- pay-equity remediation (engine/src/analysis.rs:309-869) and the defensibility check of
// edited raises (engine/src/defensibility.rs): the device passes of ob_remedy.hip and the host pieces of
// ob_remedy.cpp. The device routines take DEVICE pointers to the
// stacked rows (group A's first), so that a caller uploads them once; everything else is a host pointer.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ob_engine.hpp"

// What ob_remedy_results_get hands out: one entry per returned adjustment, ordered by original index
// (ob_remedy_run, ob_remedy_allocate) or in request order (ob_remedy_defend, ob_remedy_defend_rows).
struct ob_remedy_results {
  std::vector<int64_t> index, row;
  std::vector<double> adjustment, current_wage, new_wage, fair_wage, lower, upper;
  std::vector<int32_t> group;
  std::vector<std::string> names;       // ob_remedy_run: the design's columns
  std::vector<const char*> name_ptrs;
  std::vector<double> beta, contrib;    // contrib: n_adjustments x k row-major, or empty
  ob_remedy_info info = {};
  // ob_remedy_defend and ob_remedy_defend_rows only: one entry per kept adjustment in REQUEST order
  std::vector<int32_t> defensible;
  ob_defend_info dinfo = {};
  bool defend = false;
};

namespace ob {

// Design columns the score kernel takes: K + 1 <= 121 columns of [cov | beta] are eight 16-column MFMA
// blocks, and the Gram over [features, y, 1] has K + 1 <= OB_VIF_MAX_K + 1 columns.
constexpr int kRemedyMaxK = OB_REMEDY_MAX_K;

// The argument checks every entry point makes before any device work. k: design columns.
int remedy_check_shape(int64_t n, int k);

// analysis.rs:502-513: the request's confidence clamped to [0.50, 0.999] (0.95 when NaN) -> z.
double remedy_z_score(double confidence_level);

// fair, lev: device, n entries. dy: device, n_rss entries (may be NULL with n_rss = 0). beta[k] and
// cov[k * k]: host. dcontrib: device n x k column-major, or NULL. ms (may be NULL): HIP-event time.
int remedy_score_device(ob_ctx* ctx, const double* dx, int64_t ldx, const double* dy, int64_t n, int64_t n_rss, int k,
                        const double* beta, const double* cov, double* dfair, double* dlev, double* rss,
                        double* dcontrib, double* ms);

// dy, dfair, dlev: device, n_a + n_b stacked entries. index: host, or NULL.
int remedy_allocate_device(ob_ctx* ctx, const double* dy, const double* dfair, const double* dlev, int64_t n_a,
                           int64_t n_b, const int64_t* index, double sigma2, const ob_remedy_request& rq,
                           ob_remedy_results& out);

// defensibility.rs:199-365 over the stacked rows. dy, dfair, dlev: device, n_a + n_b entries. rows (each in
// [0, n_a + n_b), checked again here before anything is launched) and values: host, m entries in request order.
// Fills out's arrays in request order (index = row; the frame entry rewrites it), defensible, dinfo and info.
int remedy_defend_device(ob_ctx* ctx, const double* dy, const double* dfair, const double* dlev, int64_t n_a,
                         int64_t n_b, const int64_t* rows, const double* values, int64_t m, double sigma2,
                         double confidence_level, ob_remedy_results& out);

// Frontier passes (analysis.rs:871-1153) over the stacked rows: dgap and dpre hold, per row, the gap to pay (0
// for a non-candidate) and the exclusive prefix P_i of the gaps before it in descending order. xty: host,
// (k + 1) x s row-major, X_p'Y for X_p = [1, group dummy, features]. beta: host, (k + 1) x s column-major.
int remedy_front_xty_device(ob_ctx* ctx, const double* dx, int64_t ldx, const double* dy, const double* dgap,
                            const double* dpre, int64_t n, int64_t n_a, int k, int s, double step, double* xty, double* ms);
int remedy_front_rss_device(ob_ctx* ctx, const double* dx, int64_t ldx, const double* dy, const double* dgap,
                            const double* dpre, int64_t n, int64_t n_a, int k, int s, double step, const double* beta,
                            double* rss, double* ms);

}  // namespace ob
