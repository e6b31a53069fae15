// ob_dr.hpp -- the distribution-regression decomposition of quantile gaps (Chernozhukov, Fernandez-Val and Melly
// 2013): limits, row layout, and what a prepared handle keeps on the host (ob_dr.hip
// holds the rest; ob_builder.cpp routes a handle through the hooks of ob_model.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

struct ob_prepared;
struct ob_results;

namespace ob {

constexpr int kDrMaxK = 32;     // design columns with the intercept (OB_DR_MAX_K)
constexpr int kDrMaxT = 64;     // thresholds (OB_DR_MAX_T)
constexpr int kDrMaxQ = 32;     // quantiles (OB_DR_MAX_Q)
constexpr int kDrMaxVec = 128;  // coefficient vectors of a distribution pass (OB_DR_MAX_VECTORS)
// Row (include/oaxaca_boot.h): [3][n_q] quantile effects | [3][n_q] quantiles | [3][T] distribution effects |
// [4][T] F_AA, F_BB, F_AB, F_BA | the longest pass count.
inline int dr_row_len(int T, int nq) { return 6 * nq + 7 * T + 1; }
// The checks every entry point makes before any device work.
int dr_check_shape(int k, int64_t n_a, int64_t n_b, int T, int nq);

// Host side of a prepared run: what dr_finish and ob_prepared_dr_info read.
struct DrInfo {
  std::vector<double> thresholds, taus, beta;  // [T], [n_q], [2][T][k]
  std::vector<int32_t> passes;                 // [2][T]
  std::vector<uint8_t> edge;                   // [3][n_q]
  int32_t n_requested = 0, n_out_of_range = 0;
};

// Rearranges f [T] (ascending) and inverts it at taus by linear interpolation on the threshold grid
// (ob_builder.cpp). rearranged and edge may be null. Returns the number of taus that hit an edge case.
int dr_quantiles(const double* f, const double* thr, int T, const double* taus, int nq, double* q, double* rearranged,
                 uint8_t* edge);

// finish() on rows of dr_row_len(T, nq) doubles and their point row (ob_builder.cpp).
int dr_finish_rows(const double* point, int T, int nq, const double* rows, const uint8_t* ok, uint64_t n_reps,
                   ob_results** out);

}  // namespace ob
