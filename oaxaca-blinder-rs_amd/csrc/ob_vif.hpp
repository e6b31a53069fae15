// ob_vif.hpp -- the VIF collinearity diagnostic (math/diagnostics.rs:29-109): the device passes of
// ob_vif.hip and the host solves of ob_vif.cpp. The device routines take DEVICE pointers to the
// column-major predictors, so that ob_vif uploads them once for both passes; everything else is a
// host pointer.
#pragma once
#include <cstdint>

#include "ob_engine.hpp"

namespace ob {

// Predictors the kernels take: K + 1 <= 121 columns are eight 16-column MFMA blocks.
constexpr int kVifMaxK = OB_VIF_MAX_K;

// G = Xe^T Xe for Xe = [x_0..x_{k-1}, 1]: gram[(k + 1)^2] column-major on the host, both triangles.
// dx: device, column-major n x k with leading dimension ldx >= n. ms (may be NULL): HIP-event time.
int vif_gram_device(ob_ctx* ctx, const double* dx, int64_t ldx, int64_t n, int k, double* gram, double* ms);

// ss_res[j] = sum_i (x_ij - xe_i . coef_j)^2 and ss_tot[j] = sum_i (x_ij - means[j])^2 for every j.
// coef: host, (k + 1) x k column-major.
int vif_sums_device(ob_ctx* ctx, const double* dx, int64_t ldx, int64_t n, int k, const double* coef,
                    const double* means, double* ss_res, double* ss_tot, double* ms);

// The k auxiliary fits from one Gram (host only): coef (k + 1) x k column-major, coef[j][j] = 0.
int vif_solve(const double* gram, int64_t n, int k, double* coef);

// The argument checks every entry point makes before any device work.
int vif_check_shape(int64_t n, int k);

}  // namespace ob
