// ob_jackknife.hpp -- the leave-one-out (jackknife) pass over a resident panel and the BCa interval it
// feeds: the device pass of ob_jackknife.hip and the host statistics of
// ob_jackknife.cpp. C = 6 + 2K components per row, in the order of a replicate row's first C columns.
#pragma once
#include <cstdint>
#include <vector>

#include "ob_engine.hpp"

namespace ob {

constexpr int kJackMaxK = OB_JACK_MAX_K;
constexpr int64_t kJackMaxRows = (int64_t)1 << 24;  // the `rows` output only

// The checks every entry point makes before any device work. k: design columns with the intercept.
int jackknife_check_shape(int k, int64_t n_a, int64_t n_b, int n_norm, int n_y, int heckman, int want_rows);

// What one pass returns on the host. sums: [2][C][3] = sum d, sum d^2, sum d^3 over a group's kept rows.
struct JackResult {
  int c = 0;
  int64_t kept[2] = {0, 0}, dropped[2] = {0, 0};
  std::vector<double> point, sums;
  double ms = 0.0;
};

// The pass. theta (host, (n_a + n_b) x C row-major) and kept (host, n_a + n_b bytes): the `rows` output,
// or both NULL for the `sums` output.
int jackknife_device(ob_panel* p, int ref_mode, JackResult& out, double* theta, uint8_t* kept);

// stats: [C][3] = accel, jack_se, jack_bias from sums [2][C][3] and the kept rows per group.
void jackknife_finish(const double* sums, const int64_t kept[2], int c, double* stats);

// out = {ci_lower, ci_upper, z0, alpha_lo', alpha_hi', flag} over the n values v.
void bca_stats(const double* v, int64_t n, double point, double accel, double level, double out[6]);

}  // namespace ob
