// ob_binary.hpp -- the bootstrapped probit Oaxaca-Blinder decomposition of a 0/1 outcome (Fairlie 1999,
// Yun 2004, Bauer-Sinning 2008): limits and row layout (ob_binary.hip holds
// the rest; ob_builder.cpp routes a handle through the hooks of ob_model.hpp).
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

}  // namespace ob
