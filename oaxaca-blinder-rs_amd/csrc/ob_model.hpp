// ob_model.hpp -- what the model front ends on top of the engine's resampler share: the hooks
// through which ob_builder.cpp routes a prepared handle, the segmented boot driver, the staging of a frame entry
// point, the host side of the two refits, and the count images of the array entry points. The front ends are
// ob_binary.hip, ob_reweight.hip, ob_dr.hip, ob_rifq.hip, ob_rifs.hip, ob_nopo.hip, ob_density.hip and ob_tobit.hip; ob_model.hip holds
// the rest.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "ob_builder.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_spec.h"

namespace ob {

enum ModelKind : int { kModelNone = 0, kModelBinary, kModelReweight, kModelDr, kModelRifq, kModelRifs, kModelNopo, kModelDensity,
                 kModelTobit, kModelKinds };

// ob_builder.cpp reaches a front end through these hooks only, so that it links without the front end's file,
// which installs them when the library loads. state: the front end's own struct behind ob_prepared::model.
struct ModelHooks {
  int (*boot_device)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                     hipStream_t stream) = nullptr;
  int (*boot_host)(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok) = nullptr;
  void (*free_state)(void* state) = nullptr;
};
ModelHooks& model_hooks(int kind);  // ob_builder.cpp
inline bool model_install(int kind, const ModelHooks& h) {
  model_hooks(kind) = h;
  return true;
}

// A kind's name in messages: "<label>: ..." and "jackknife: <plural> (BCa included) ...".
struct ModelName {
  const char *label, *plural;
};
inline const ModelName& model_name(int kind) {
  static const ModelName names[kModelKinds] = {
      {"", ""},
      {"binary decomposition", "binary decompositions"},
      {"reweighted decomposition", "reweighted decompositions"},
      {"distribution regression", "distribution-regression decompositions"},
      {"quantile refit", "refitted quantile decompositions"},
      {"statistics refit", "refitted statistic decompositions"},
      {"matching decomposition", "matching decompositions"},
      {"density decomposition", "density decompositions"},
      {"tobit decomposition", "tobit decompositions"},
  };
  return names[kind];
}
// The refusal of an entry point that does not take a handle of this kind ("sharded runs are", ..).
inline int model_refuse(int kind, const char* what) {
  return fail(OB_E_UNSUPPORTED, "%s: %s outside its scope", model_name(kind).label, what);
}

// The state of a handle of `kind`, else null. Each front end wraps it in a typed accessor of its own.
template <class S>
S* model_state(const ob_prepared* pr, int kind) {
  return pr && pr->model_kind == kind ? static_cast<S*>(pr->model) : nullptr;
}

// ---- the segmented boot ------------------------------------------------------------------------------------------

// How a front end boots: the segment's length is min(n_reps, seg_reps, what keeps its count images within
// count_budget bytes, in whole blocks of 64).
struct BootPlan {
  uint64_t seg_reps, count_budget;
  bool draws;  // the driver draws a segment's counts (engine_counts); false: the segment callback does
  // once, after engine_order and before the first segment: workspace for segments of at most seg_pad replicates
  std::function<int(uint32_t seg_pad)> begin;
};
// Today's plans: 4096 replicates a segment for binary, reweight and dr, 2048 for the refits (which draw their own
// counts, for the point pass's sake); 8 GiB of count images for all.
constexpr uint64_t kFitSegReps = 4096, kRefitSegReps = 2048, kCountBudget = 8ull << 30;

// Replicates [s0, s0 + ns) of the call on stream s. nb_rep, rep_pad: engine_counts' (0 where the callback draws).
using SegmentFn = std::function<int(uint64_t s0, uint32_t ns, uint32_t nb_rep, uint32_t rep_pad, hipStream_t s)>;

// The boot of a handle of `kind`: the pointer and replicate-id checks, the device and stream, engine_order, the
// segment loop, engine_counts' overflow word, engine_mark on every path after the order. rows_set: the caller's
// destinations are non-null.
int boot_segmented(ob_prepared* pr, int kind, const BootPlan& plan, uint64_t first_rep, uint64_t n_reps, bool rows_set,
                   hipStream_t stream, const SegmentFn& segment);

// Replicates per batch of a segment of rep_pad: whole 64-replicate blocks whose chunk partials (rep_bytes a
// replicate) stay within 1 GiB, at least one block (sub_block: a batch below 64 replicates where not even one block
// fits, which dr's kernels take); option hk_batch forces at most that many blocks. Rows do not depend on it.
uint32_t boot_batch_reps(size_t rep_bytes, uint32_t rep_pad, bool sub_block = false);

// batch(b0, nb) over a segment's ns replicates in batches of hb, until one fails.
template <class F>
int boot_batches(uint32_t ns, uint32_t hb, F&& batch) {
  int rc = OB_OK;
  for (uint32_t b0 = 0; b0 < ns && rc == OB_OK; b0 += hb) rc = batch(b0, std::min(hb, ns - b0));
  return rc;
}

// ModelHooks::boot_host of every front end: device rows [n_y][n_reps][row_len] and ok, the kind's boot_device,
// the copy back.
int model_boot_host(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok);

// ---- staging -----------------------------------------------------------------------------------------------------

// The design of a frame entry point (ob::data_matrices), freed with the object.
struct Matrices {
  ob_matrices* m = nullptr;
  int64_t n[2] = {0, 0};
  int32_t k = 0;
  const double *x[2] = {nullptr, nullptr}, *y[2] = {nullptr, nullptr};  // x: n x k column-major, column 0 the intercept
  Matrices() = default;
  Matrices(const Matrices&) = delete;
  Matrices& operator=(const Matrices&) = delete;
  ~Matrices();
  int load(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg, bool want_w);
  const double* w(int g) const { return matrices_weights(m, g); }
};

// The frame, then every named column (outcome, group, predictors, categoricals, the weights where `weights`): it
// exists, holds no null and, where `finite`, no non-finite f64; where `weights_nonneg`, no negative weight either
// (OB_E_INVALID here, before the design's own check of the weights answers OB_E_GROUP).
int stage_named(const ob_column* cols, int32_t n_cols, int64_t n_rows, const Config& c, int kind, bool weights,
                bool finite, bool weights_nonneg = false);

// A handle of `kind` over m with the common fields set (the seed drawn where the configuration has none); it owns
// `state` from here on.
ob_prepared* model_handle(ob_ctx* ctx, const Config& c, const Matrices& m, int kind, void* state, int row_len, int n_y);
// The end of a prepare: the handle to the caller, or destroyed where the build failed.
int model_built(ob_prepared* pr, int rc, ob_prepared** out);

// A group's [y | x_1 .. x_{k-1} | extra columns] x ld on the device, zero past n and in the extra columns.
// x: n x k column-major with ld n, column 0 (the intercept) skipped.
int upload_group(DevBuf& dst, int64_t ld, int64_t n, int k, int extra, const double* y, const double* x);
// Column `col` of an uploaded group: w, or ones where w is null.
int upload_weights(DevBuf& dst, int64_t ld, int64_t n, int col, const double* w);
// The panel of binary, reweight and dr: the resampler over the groups' row counts and the outcome alone.
int outcome_panel(ob_ctx* ctx, const Matrices& m, ob_panel** out);
// The panel's chunk table on the device.
int upload_chunks(ob_panel* p, DevBuf& dst, int* n_chunks);

// ---- the refits (ob_rifq.hip, ob_rifs.hip) ------------------------------------------------------------------------

// Each group's rows in stable ascending order of y.
struct SortedGroups {
  std::vector<int32_t> perm[2];  // sorted position -> row of the group before the sort
  std::vector<double> x[2], y[2];  // x: n x k column-major
  double mu0[2] = {0.0, 0.0}, npow[2] = {0.0, 0.0};  // mean of y, n^-0.2
};
void sort_groups(const Matrices& m, SortedGroups& out);
// The refit's panel over the sorted rows (the resampler, the Gram, the chunk table and the solve).
int refit_panel(ob_ctx* ctx, const Config& c, const Matrices& m, const SortedGroups& sg, ob_panel** out);

// One segment of a refit: the counts (the OBRS-3 stream, or unit counts for the point pass), the f64 Gram and its
// reduce, the model's kernels (launch), then per output the y-pairs patched into the Grams, the engine's solve and the
// row with its tail (tail), and the one host wait of a segment: the floor flags and the timings.
struct RefitSegment {
  bool point;
  uint64_t first_rep;  // of this segment
  uint32_t ns;
  uint64_t n_total, s0;  // rows / ok: [n_out][n_total] blocks, this segment at s0
  double* d_rows;
  uint8_t* d_ok;
};
struct RefitOut {
  const double* gy;        // [rep][2][n_out][k + 1] G[a, y] for a < k, then G[y, y]
  const uint8_t* floored;  // [rep][2][n_out]
};
// What a refit supplies: its outputs, the buffers of the solve, its kernels over the counts just drawn and the
// kernel that writes output t's rows from the solved OLS rows.
struct RefitModel {
  int n_out;
  DevBuf *solved, *sok;
  int64_t* n_floored;  // the segment's floored densities are added
  std::function<int(uint32_t nb_rep, uint32_t rep_pad, RefitOut* out)> launch;
  std::function<void(int t, const double* solved, const uint8_t* sok, double* rows, uint8_t* ok)> tail;
};
struct RefitTimes {
  float gram_ms = 0.f, solve_ms = 0.f;  // counts and Gram; the store / solve / tail loop
};
int refit_segment(ob_prepared* pr, const RefitSegment& sg, const RefitModel& md, hipStream_t s, RefitTimes* times);
// The point pass: segment(d_rows, d_ok) over unit counts between engine_order and engine_mark, the rows into
// pr->point_row [n_y][row_len], every ok checked.
int refit_point(ob_prepared* pr, const std::function<int(double* d_rows, uint8_t* d_ok, hipStream_t s)>& segment);
// rifq_store_kernel (ob_rifq.hip): output t's y-pairs gy [rep][2][n_out][k + 1] over those of the reduced Grams
// [rep][2][e_pad] of v = [1, x, y].
int rifq_store(const double* gy, int k, uint32_t n_reps, int n_out, int t, double* gram, int e_pad, hipStream_t s);

// ---- the array entry points ---------------------------------------------------------------------------------------

// The chunk table (g, t0, t1) of one group of `tiles` tiles in at most max_chunks chunks, appended.
inline void group_chunks(uint32_t g, uint32_t tiles, uint32_t max_chunks, std::vector<uint32_t>& chunks) {
  const uint32_t nc = std::min(tiles, max_chunks);
  for (uint32_t c = 0; c < nc; ++c) {
    chunks.push_back(g);
    chunks.push_back((uint32_t)((uint64_t)tiles * c / nc));
    chunks.push_back((uint32_t)((uint64_t)tiles * (c + 1) / nc));
  }
}

// u8 counts [n_reps][n] (rep_stride = n; 0: every replicate counts the rows alike) of one group into the engine's
// f64-Gram count images (ob_engine.hpp) and, where m1 is set, its [replicate][tile] sums with row stride m1_ld.
// img, m1: at the group's first tile, zeroed by the caller; nb_rep = ceil(n_reps / 64). No HIP call.
inline void pack_count_images(const uint8_t* counts, int64_t n, int64_t rep_stride, uint32_t n_reps, uint32_t nb_rep,
                              uint32_t* img, uint32_t* m1, size_t m1_ld) {
  for (uint32_t r = 0; r < n_reps; ++r)
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t c = counts[(size_t)r * rep_stride + i];
      if (!c) continue;
      const size_t tl = (size_t)(i / OB_TILE_ROWS), within = (size_t)(i % OB_TILE_ROWS), sub = within >> 6, qq = within & 63;
      img[((tl * nb_rep + (r >> 6)) * 4 + sub) * kCimgWords + (r & 63u) * kCimgStride + (qq >> 2)] |= c << (8 * (qq & 3));
      if (m1) m1[(size_t)r * m1_ld + tl] += c;
    }
}

// The argument checks ob_rifq_pass and ob_rifs_pass share, after their own (the null outputs, the statistics, the
// replicate range); `what` names the entry point.
int refit_pass_check(const char* what, const double* y_sorted, int64_t n, const uint8_t* counts, int32_t n_reps,
                     const double* x, int64_t ldx, int32_t p, bool gini);

// The inputs of a refit pass over one sorted group on the device (the host images live as long: the copies are
// asynchronous).
struct RefitPassInput {
  DevBuf cols, chunks, counts, m1;
  std::vector<uint32_t> table, img, sums;
  uint32_t tiles = 0, n_chunks = 0, nb_rep = 0, rep_pad = 0;
  int64_t ld = 0;
  double mu0 = 0.0;
  int upload(const double* y_sorted, int64_t n, const uint8_t* counts_h, int32_t n_reps, const double* x, int64_t ldx,
             int k, hipStream_t s);
};

}  // namespace ob
