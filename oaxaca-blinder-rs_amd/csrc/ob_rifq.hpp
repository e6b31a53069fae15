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


struct RifqState;  // device side of a prepared refit run (ob_rifq.hip)

// ob_builder.cpp reaches the refit through these hooks only (as it does the binary code), so that it links without
// ob_rifq.hip. ob_rifq.hip installs them when the library loads.
struct RifqHooks {
  int (*boot_device)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                     hipStream_t stream) = nullptr;
  int (*boot_host)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok) = nullptr;
  void (*free_state)(RifqState* s) = nullptr;
};
RifqHooks& rifq_hooks();  // ob_builder.cpp

}  // namespace ob
