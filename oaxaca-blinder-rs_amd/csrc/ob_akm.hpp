// ob_akm.hpp -- device entry points of the AKM two-way fixed-effects path (ob_akm.hip), called by
// the C ABI in ob_akm.cpp. All pointers are host pointers; an AkmPlan owns what lives in HBM.
#pragma once
#include <cstdint>
#include <vector>

#include "ob_common.hpp"

struct ob_ctx;

namespace ob {

// Group-size schedule of the segmented-mean kernels, by a group's row count alone:
// up to kAkmLaneMax rows one lane owns the group, up to kAkmWaveMax one wave, beyond that one block.
constexpr int kAkmLaneMax = 32;
constexpr int kAkmWaveMax = 2048;
constexpr int kAkmPollDefault = 8;  // iterations between two reads of the done flags (option akm_poll)

struct AkmPlan;  // the two CSR groupings of the rows and the batch buffers, on the device

// widx / fidx: n dense indices in [0, n_workers) / [0, n_firms), checked by the caller.
int akm_plan_create(ob_ctx* ctx, int64_t n, const int32_t* widx, const int32_t* fidx, int64_t n_workers,
                    int64_t n_firms, AkmPlan** out);
void akm_plan_free(AkmPlan* p);

// demean_vector (akm.rs:452-527) of n_cols columns in one batch. v: row-major n x n_cols (the columns
// of a row side by side). out (may be NULL): the same layout. iterations / converged: per column;
// converged[c] = iterations[c] < max_iters, the reference's test after its loop. The raw and the
// demeaned batch stay in the plan for akm_gram, akm_residual and akm_r2. launches (may be NULL): kernel
// launches per iteration.
int akm_demean(AkmPlan* p, const double* v, int n_cols, double tol, int64_t max_iters, double* out,
               int32_t* iterations, int32_t* converged, double* ms, int* launches);
// g: n_cols x n_cols, g[a * n_cols + b] = sum_i v_ia v_ib over the demeaned batch.
int akm_gram(AkmPlan* p, double* g, double* ms);
// r = column 0 of the raw batch minus the other columns times beta[n_cols - 1]; kept in the plan.
int akm_residual(AkmPlan* p, const double* beta, double* ms);
// recover_fe (akm.rs:530-621) with the psi[0] normalisation. r NULL: the plan's residual.
// alpha[n_workers], psi[n_firms] (either may be NULL) are copied out; both stay in the plan.
int akm_recover(AkmPlan* p, const double* r, double tol, int64_t max_iters, double* alpha, double* psi,
                int32_t* iterations, int32_t* converged, double* ms);
// akm.rs:393-415 over the raw batch, beta and the plan's alpha / psi.
int akm_r2(AkmPlan* p, const double* beta, double* tss, double* rss, double* ms);

}  // namespace ob
