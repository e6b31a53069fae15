// ob_binary.hpp -- the bootstrapped probit Oaxaca-Blinder decomposition of a 0/1 outcome (Fairlie 1999,
// Yun 2004, Bauer-Sinning 2008): limits, row layout and the hooks through which
// ob_builder.cpp routes a handle that ob_builder_prepare_binary made (ob_binary.hip holds the rest).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ob_prepared;

namespace ob {

constexpr int kBinaryMaxK = 32;  // design columns with the intercept: the probit kernels' limit
// Row: 6 aggregates | explained_k | unexplained_k | beta_A, beta_B, xbar_A, xbar_B, beta* | 6 mean
// probabilities | ybar_A, ybar_B (include/oaxaca_boot.h).
inline int binary_row_len(int k) { return 6 + 7 * k + 8; }
// Values per (chunk, replicate, group) of the mean-probability pass: sum c Phi(x'beta) for beta_A,
// beta_B, beta*; sum c y; sum c; sum c x_j for j < k (x_0 = 1).
__host__ __device__ inline int binary_sums_len(int k) { return 5 + k; }
// The checks every entry point makes before any device work. k: design columns with the intercept.
int binary_check_shape(int k, int64_t n_a, int64_t n_b);

struct BinaryState;  // device side of a prepared binary run (ob_binary.hip)

// ob_builder.cpp reaches the binary code through these hooks only (as it does the cluster code), so
// that it links without ob_binary.hip. ob_binary.hip installs them when the library loads.
struct BinaryHooks {
  int (*boot_device)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                     hipStream_t stream) = nullptr;
  int (*boot_host)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok) = nullptr;
  void (*free_state)(BinaryState* s) = nullptr;
};
BinaryHooks& binary_hooks();  // ob_builder.cpp

}  // namespace ob
