// ob_heckman.hpp -- the Heckman two-step stage of a bootstrap segment (ob_heckman.hip), run after
// the selected-row Gram (weights := [s == 1]) has been reduced by the engine.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// Panel column layout of a Heckman panel (per group, [col][ld]):
//   x_1..x_p | y | ind = [s == 1] (the Gram's weight column) | s | z_1..z_{ks-1} | (w)
struct ob_heck_seg {
  const double* cols[2];
  int64_t ld[2];
  uint32_t n[2];
  uint32_t tiles0;
  int p, ks, weighted;  // ks = 1 + selection predictors; weighted: the w column is present
  int sz_col;           // panel column of s (z_1.. follow it): p + 2 in the layout above
  // resampling: level-2 count images (NULL = every row once: the point estimate) and chunks
  const uint32_t* counts;
  int counts_i8;  // 1: the i8 Gram's A-fragment images (ob_count_kernel<true>), 0: the f64 Gram's
  uint32_t nb_rep;
  const uint32_t* chunks;
  int n_chunks;
  uint32_t rep_pad, n_reps;
  // the selected-row extended Gram [rep][2][e_pad] over v = ind * [1, x, y]
  const double* gram;
  int e_pad, k1;
  // workspace
  double* gamma;     // [2][rep_pad][ks]
  uint32_t* hflags;  // [2][rep_pad]
  double* partial;   // [chunk][rep_pad][max(probit, sums) values]; the wide path (ks > 8): [chunk][part_pad][..]
  uint32_t part_pad; // wide path: replicates per chunk of `partial` (>= n_reps)
  uint32_t* active;  // one word
  // output rows (ob_heck_row_len) and status
  int ref_mode;
  double* rows;
  uint8_t* ok;
  int row_len;
  int raw_status;  // 1: ok[] receives the status code (ob_heck_status)
  int max_iter;    // probit iterations (probit.rs: 100)
  double tol;      // a replicate stops once ||step|| < tol (probit.rs: 1e-6)
};

enum ob_heck_status {
  OB_HS_CHOLESKY = 0,  // outcome OLS: Cholesky failed (NalgebraError)
  OB_HS_OK = 1,
  OB_HS_ZERO_WEIGHT = 2,   // Weighted/Cotton: no weight in either group
  OB_HS_NO_OUTCOMES = 3,   // "No observed outcomes in group"
  OB_HS_INSUFFICIENT = 4,  // outcome OLS: selected rows <= K + 1
  OB_HS_PROBIT = 5,        // "Failed to solve Hessian system in Probit"
};

namespace ob {
// ks up to kHeckMaxKs runs the register-resident kernels (lane = replicate); wider selection
// equations, up to kHeckWideMaxKs columns, run the MFMA kernels (ob_heck_wide_kernel).
constexpr int kHeckMaxKs = 8;
constexpr int kHeckWideMaxKs = 32;
// Slots of the selection means in the sums layout: 8 on the narrow path whatever ks, else ks.
__host__ __device__ inline int heck_sel_slots(int ks) { return ks <= kHeckMaxKs ? kHeckMaxKs : ks; }
// Values per (chunk, replicate) of the sums kernel for K = p + 1 outcome columns.
__host__ __device__ inline int heck_sums_len(int k, int ks) { return 5 + heck_sel_slots(ks) + k; }
__host__ __device__ inline int heck_probit_len(int ks) { return ks * (ks + 1) / 2 + ks; }
__host__ __device__ inline int heck_row_len(int k, int ks) { return 6 + 7 * (k + 1) + ks; }
// Largest p the register-resident sums kernel takes (13 + K <= 64); the wide path keeps it.
constexpr int kHeckMaxP = 50;
// Kernel timings of one segment (HIP events on the segment's stream).
struct ob_heck_times {
  double probit_ms = 0.0;  // ob_probit_kernel, summed over the iterations
  int probit_launches = 0;
  double sums_ms = 0.0;    // ob_heck_sums_kernel
};
// Runs the probit iterations, the IMR sums and the two-step solve for one segment; on return
// (after a stream sync) rows/ok are final. iters: the probit iterations run; tm (optional): the
// kernel timings, added to.
int heckman_segment(const ob_heck_seg& h, hipStream_t s, int* iters, ob_heck_times* tm = nullptr);
// The probit stage alone: Fisher scoring from gamma = 0 on the panel columns s (sz_col), z_1.. that
// follow it, over the segment's counts and chunks. On return (after a stream sync) gamma and hflags
// (bit 0 done, bit 1 failed: the Hessian could not be solved) are final. Reads none of p, weighted,
// gram, rows, ok, ref_mode. heckman_segment and the binary decomposition (ob_binary.hip) call it.
int probit_stage(const ob_heck_seg& h, hipStream_t s, int* iters, ob_heck_times* tm = nullptr);
constexpr uint32_t kProbitDone = 1u, kProbitFailed = 2u;  // hflags bits
// Values of `partial` per (chunk, replicate) that a segment of this shape needs.
inline size_t heck_partial_len(int k, int ks) {
  const int a = heck_probit_len(ks), b = heck_sums_len(k, ks);
  return (size_t)(a > b ? a : b);
}
}  // namespace ob
