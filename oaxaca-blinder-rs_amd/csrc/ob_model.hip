// ob_model.hip -- the code the model front ends share (ob_model.hpp). No kernel lives here.
#include "ob_model.hpp"

#include <cmath>
#include <numeric>
#include <random>

#include "ob_cluster.hpp"  // engine_solve_grams
#include "ob_options.hpp"

namespace ob {

// ---- the segmented boot ------------------------------------------------------------------------------------------

int boot_segmented(ob_prepared* pr, int kind, const BootPlan& plan, uint64_t first_rep, uint64_t n_reps, bool rows_set,
                   hipStream_t stream, const SegmentFn& segment) {
  if (!model_state<void>(pr, kind) || (n_reps && !rows_set)) return fail(OB_E_INVALID, "null pointer");
  if (n_reps == 0) return OB_OK;
  if (first_rep + n_reps > 0xFFFFFFFFull)
    return fail(OB_E_INVALID, "replicate ids must stay below 2^32 - 1 (OBRS-3 counter word)");
  ob_panel* p = pr->panel;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = stream ? stream : p->ctx->stream;
  OB_TRY(engine_order(p, s));
  const uint32_t tiles = p->ntiles[0] + p->ntiles[1];
  const uint64_t batch_bytes = (uint64_t)std::max(tiles, 1u) * 4 * kCimgWords * sizeof(uint32_t);
  const uint64_t seg_cap = std::max<uint64_t>(64, (plan.count_budget / batch_bytes) * 64);
  const uint64_t seg = std::min<uint64_t>(n_reps, std::min<uint64_t>(plan.seg_reps, seg_cap));
  if (plan.begin) OB_TRY(plan.begin((uint32_t)((seg + 63) / 64 * 64)));
  OB_HIP(hipMemsetAsync(p->d_flags + 2, 0, sizeof(uint32_t), s));  // engine_counts' overflow word
  int rc = OB_OK;
  for (uint64_t s0 = 0; s0 < n_reps && rc == OB_OK; s0 += seg) {
    const uint32_t ns = (uint32_t)std::min<uint64_t>(seg, n_reps - s0);
    uint32_t nb_rep = 0, rep_pad = 0;
    if (plan.draws) rc = engine_counts(p, pr->seed, first_rep + s0, ns, s, &nb_rep, &rep_pad);
    if (rc == OB_OK) rc = segment(s0, ns, nb_rep, rep_pad, s);
  }
  uint32_t flag = 0;
  if (rc == OB_OK && hipMemcpyAsync(&flag, p->d_flags + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = fail(OB_E_HIP, "copy of the overflow word failed");
  if (rc == OB_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(OB_E_HIP, "stream synchronize failed");
  const int rm = engine_mark(p, s);
  if (rc != OB_OK) return rc;
  if (flag & 1u) return fail(OB_E_OVERFLOW, "a resampled row was drawn more than 255 times in one replicate");
  return rm;
}

uint32_t boot_batch_reps(size_t rep_bytes, uint32_t rep_pad, bool sub_block) {
  constexpr size_t kPartialBudget = (size_t)1 << 30;  // bytes of chunk partials per batch (as heck_batch)
  size_t reps = kPartialBudget / std::max<size_t>(rep_bytes, 1);
  reps = reps >= 64 ? reps / 64 * 64 : (sub_block ? std::max<size_t>(reps, 1) : 64);
  const int forced = opt_int(Opt::HkBatch, 0);
  if (forced > 0) reps = std::min<size_t>(reps, (size_t)forced * 64);
  return (uint32_t)std::min<size_t>(rep_pad, reps);
}

int model_boot_host(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok) {
  if (!pr || !pr->model || (n_reps && (!rows || !ok))) return fail(OB_E_INVALID, "null pointer");
  if (n_reps == 0) return OB_OK;
  OB_HIP(hipSetDevice(pr->panel->ctx->device));
  const size_t n_out = (size_t)pr->n_y;
  DevBuf d_rows, d_ok;
  OB_HIP(d_rows.alloc(sizeof(double) * n_out * n_reps * pr->row_len));
  OB_HIP(d_ok.alloc(n_out * n_reps));
  OB_TRY(model_hooks(pr->model_kind).boot_device(pr, first_rep, n_reps, d_rows.d(), d_ok.as<uint8_t>(), nullptr));
  OB_HIP(hipMemcpy(rows, d_rows.p, sizeof(double) * n_out * n_reps * pr->row_len, hipMemcpyDeviceToHost));
  OB_HIP(hipMemcpy(ok, d_ok.p, n_out * n_reps, hipMemcpyDeviceToHost));
  return OB_OK;
}

// ---- staging -----------------------------------------------------------------------------------------------------

Matrices::~Matrices() { ob_matrices_free(m); }

int Matrices::load(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg, bool want_w) {
  OB_TRY(data_matrices(cols, n_cols, n_rows, cfg, want_w, &m));
  OB_TRY(ob_matrices_dims(m, &n[0], &n[1], &k));
  return ob_matrices_get(m, &x[0], &y[0], &x[1], &y[1]);
}

int stage_named(const ob_column* cols, int32_t n_cols, int64_t n_rows, const Config& c, int kind, bool weights,
                bool finite, bool weights_nonneg) {
  Frame f;
  OB_TRY(load_frame(cols, n_cols, n_rows, f));
  std::vector<std::string> named = {c.outcome, c.group};
  named.insert(named.end(), c.predictors.begin(), c.predictors.end());
  named.insert(named.end(), c.categorical.begin(), c.categorical.end());
  if (weights && c.has_weights) named.push_back(c.weights);
  const char* label = model_name(kind).label;
  for (const std::string& name : named) {
    const int i = f.find(name);
    if (i < 0) return fail(OB_E_COLUMN, "%s%s", error_prefix(OB_E_COLUMN), name.c_str());
    const Col& col = f.cols[i];
    for (int64_t r = 0; r < f.nrows; ++r) {
      if (!col.valid[r])
        return fail(OB_E_INVALID, "%s: column `%s` has a null in row %lld", label, name.c_str(), (long long)r);
      if (finite && col.kind == OB_COL_F64 && !std::isfinite(col.f[r]))
        return fail(OB_E_INVALID, "%s: column `%s` has a non-finite value in row %lld", label, name.c_str(), (long long)r);
    }
  }
  if (weights && weights_nonneg && c.has_weights) {
    const Col& wc = f.cols[f.find(c.weights)];
    for (int64_t r = 0; r < f.nrows; ++r)
      if ((wc.kind == OB_COL_F64 && wc.f[r] < 0.0) || (wc.kind == OB_COL_I64 && wc.i[r] < 0))
        return fail(OB_E_INVALID, "%s: column `%s` has a negative weight in row %lld", label, c.weights.c_str(), (long long)r);
  }
  return OB_OK;
}

ob_prepared* model_handle(ob_ctx* ctx, const Config& c, const Matrices& m, int kind, void* state, int row_len, int n_y) {
  ob_prepared* pr = new ob_prepared();
  pr->model_kind = kind;
  pr->model = state;
  pr->ctx = ctx;
  pr->cfg = c;
  pr->ref = c.ref;
  if (c.has_seed) {
    pr->seed = c.seed;
  } else {
    std::random_device rd;
    pr->seed = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
  }
  pr->k = m.k;
  pr->n_base = 0;
  pr->row_len = row_len;
  for (int32_t j = 0; j < m.k; ++j) pr->names.emplace_back(ob_matrices_name(m.m, j));
  pr->detail_names = pr->names;
  pr->n_a = m.n[0];
  pr->n_b = m.n[1];
  pr->n_y = n_y;
  pr->n_resid = 0;
  return pr;
}

int model_built(ob_prepared* pr, int rc, ob_prepared** out) {
  if (rc != OB_OK) {
    ob_prepared_destroy(pr);
    return rc;
  }
  *out = pr;
  return OB_OK;
}

int upload_group(DevBuf& dst, int64_t ld, int64_t n, int k, int extra, const double* y, const double* x) {
  const size_t bytes = sizeof(double) * (size_t)(k + extra) * ld;
  OB_HIP(dst.alloc(bytes));
  OB_HIP(hipMemset(dst.p, 0, bytes));
  OB_HIP(hipMemcpy(dst.p, y, sizeof(double) * n, hipMemcpyHostToDevice));
  if (k > 1)
    OB_HIP(hipMemcpy2D(dst.d() + ld, sizeof(double) * ld, x + n, sizeof(double) * n, sizeof(double) * n, k - 1,
                       hipMemcpyHostToDevice));
  return OB_OK;
}

int upload_weights(DevBuf& dst, int64_t ld, int64_t n, int col, const double* w) {
  const std::vector<double> unit(w ? 0 : (size_t)n, 1.0);
  OB_HIP(hipMemcpy(dst.d() + (size_t)col * ld, w ? w : unit.data(), sizeof(double) * n, hipMemcpyHostToDevice));
  return OB_OK;
}

int outcome_panel(ob_ctx* ctx, const Matrices& m, ob_panel** out) {
  ob_panel_desc pd{};
  pd.p = 0;
  pd.n_y = 1;
  pd.a = {m.n[0], nullptr, m.n[0], m.y[0], nullptr};
  pd.b = {m.n[1], nullptr, m.n[1], m.y[1], nullptr};
  return ob_panel_create(ctx, &pd, out);
}

int upload_chunks(ob_panel* p, DevBuf& dst, int* n_chunks) {
  int32_t nc = 0;
  OB_TRY(ob_debug_chunks(p, nullptr, 0, &nc));
  std::vector<uint32_t> table((size_t)3 * nc);
  OB_TRY(ob_debug_chunks(p, table.data(), nc, &nc));
  *n_chunks = nc;
  OB_HIP(dst.alloc(sizeof(uint32_t) * table.size()));
  OB_HIP(hipMemcpy(dst.p, table.data(), sizeof(uint32_t) * table.size(), hipMemcpyHostToDevice));
  return OB_OK;
}

// ---- the refits --------------------------------------------------------------------------------------------------

void sort_groups(const Matrices& m, SortedGroups& out) {
  const int32_t k = m.k;
  for (int g = 0; g < 2; ++g) {
    const int64_t n = m.n[g];
    out.perm[g].resize((size_t)n);
    std::iota(out.perm[g].begin(), out.perm[g].end(), 0);
    const double* y = m.y[g];
    std::stable_sort(out.perm[g].begin(), out.perm[g].end(), [y](int32_t a, int32_t b) { return y[a] < y[b]; });
    out.x[g].resize((size_t)n * k);
    out.y[g].resize((size_t)n);
    double mu = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const int32_t r = out.perm[g][(size_t)i];
      out.y[g][(size_t)i] = y[r];
      mu += y[r];
      for (int32_t j = 0; j < k; ++j) out.x[g][(size_t)j * n + i] = m.x[g][(size_t)j * n + r];
    }
    out.mu0[g] = mu / (double)n;
    out.npow[g] = std::pow((double)n, -0.2);
  }
}

int refit_panel(ob_ctx* ctx, const Config& c, const Matrices& m, const SortedGroups& sg, ob_panel** out) {
  ob_panel_desc pd{};
  pd.p = m.k - 1;
  pd.n_num = (int32_t)c.predictors.size();
  pd.n_y = 1;
  pd.a = {m.n[0], sg.x[0].data() + m.n[0], m.n[0], sg.y[0].data(), nullptr};
  pd.b = {m.n[1], sg.x[1].data() + m.n[1], m.n[1], sg.y[1].data(), nullptr};
  return ob_panel_create(ctx, &pd, out);
}

int refit_segment(ob_prepared* pr, const RefitSegment& sg, const RefitModel& md, hipStream_t s, RefitTimes* times) {
  ob_panel* p = pr->panel;
  const int rl0 = p->row_len, rl = pr->row_len;
  Events<4> ev;  // start | Gram end | the model's kernels' end | solve end
  OB_HIP(ev.create());
  OB_HIP(hipEventRecord(ev.e[0], s));
  uint32_t nb_rep = 0, rep_pad = 0;
  if (sg.point) OB_TRY(engine_unit_counts(p, s, &nb_rep, &rep_pad));
  else OB_TRY(engine_counts(p, pr->seed, sg.first_rep, sg.ns, s, &nb_rep, &rep_pad));
  OB_TRY(engine_gram_f64(p, sg.ns, s));
  OB_HIP(md.solved->alloc(sizeof(double) * (size_t)rep_pad * rl0));
  OB_HIP(md.sok->alloc(rep_pad));
  OB_HIP(hipEventRecord(ev.e[1], s));
  RefitOut o{};
  OB_TRY(md.launch(nb_rep, rep_pad, &o));
  OB_HIP(hipEventRecord(ev.e[2], s));
  for (int t = 0; t < md.n_out; ++t) {
    OB_TRY(rifq_store(o.gy, pr->k, sg.ns, md.n_out, t, p->d_gram, p->e_pad, s));
    OB_TRY(engine_solve_grams(p, p->d_gram, nullptr, sg.ns, sg.ns, 0, pr->ref, md.solved->d(), md.sok->as<uint8_t>(), s));
    md.tail(t, md.solved->d(), md.sok->as<uint8_t>(), sg.d_rows + ((size_t)t * sg.n_total + sg.s0) * rl,
            sg.d_ok + (size_t)t * sg.n_total + sg.s0);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(ev.e[3], s));
  std::vector<uint8_t> fl((size_t)sg.ns * 2 * md.n_out);
  OB_HIP(hipMemcpyAsync(fl.data(), o.floored, fl.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));  // the one host wait of a segment: the floor flags and the timings
  float gram_ms = 0.f, solve_ms = 0.f;
  OB_HIP(hipEventElapsedTime(&gram_ms, ev.e[0], ev.e[1]));
  OB_HIP(hipEventElapsedTime(&solve_ms, ev.e[2], ev.e[3]));
  times->gram_ms += gram_ms;
  times->solve_ms += solve_ms;
  for (uint8_t v : fl) *md.n_floored += v ? 1 : 0;
  return OB_OK;
}

int refit_point(ob_prepared* pr, const std::function<int(double* d_rows, uint8_t* d_ok, hipStream_t s)>& segment) {
  ob_panel* p = pr->panel;
  hipStream_t s = pr->ctx->stream;
  const size_t T = (size_t)pr->n_y;
  DevBuf d_rows, d_ok;
  OB_HIP(d_rows.alloc(sizeof(double) * T * pr->row_len));
  OB_HIP(d_ok.alloc(T));
  OB_TRY(engine_order(p, s));
  OB_TRY(segment(d_rows.d(), d_ok.as<uint8_t>(), s));
  OB_TRY(engine_mark(p, s));
  pr->point_row.assign(T * pr->row_len, 0.0);
  std::vector<uint8_t> okh(T, 0);
  OB_HIP(hipMemcpy(pr->point_row.data(), d_rows.p, sizeof(double) * T * pr->row_len, hipMemcpyDeviceToHost));
  OB_HIP(hipMemcpy(okh.data(), d_ok.p, T, hipMemcpyDeviceToHost));
  for (uint8_t v : okh)
    if (!v)
      return fail(OB_E_LINALG, "%s%s: the point estimate's regression could not be solved", error_prefix(OB_E_LINALG),
                  model_name(pr->model_kind).label);
  return OB_OK;
}

// ---- the array entry points --------------------------------------------------------------------------------------

int refit_pass_check(const char* what, const double* y_sorted, int64_t n, const uint8_t* counts, int32_t n_reps,
                     const double* x, int64_t ldx, int32_t p, bool gini) {
  if (!counts && n_reps != 1) return fail(OB_E_INVALID, "%s: the point pass (no counts) is one replicate", what);
  if (n < 2) return fail(OB_E_INSUFFICIENT, "%s needs at least 2 rows, got %lld", what, (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(OB_E_UNSUPPORTED, "%s takes fewer than 2^31 rows", what);
  if (p > 0 && ldx < n) return fail(OB_E_INVALID, "%s: ldx = %lld is below n = %lld", what, (long long)ldx, (long long)n);
  bool positive = false;
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(y_sorted[i])) return fail(OB_E_INVALID, "%s: y must be finite", what);
    if (i && y_sorted[i] < y_sorted[i - 1]) return fail(OB_E_INVALID, "%s: y must be in ascending order", what);
    if (gini && y_sorted[i] < 0.0) return fail(OB_E_INVALID, "%s: the Gini takes no negative y", what);
    positive = positive || y_sorted[i] > 0.0;
  }
  if (gini && !positive) return fail(OB_E_INVALID, "%s: the Gini needs a positive y", what);
  for (int64_t j = 0; j < (int64_t)p; ++j)
    for (int64_t i = 0; i < n; ++i)
      if (!std::isfinite(x[j * ldx + i])) return fail(OB_E_INVALID, "%s: x must be finite", what);
  if (counts)
    for (int32_t r = 0; r < n_reps; ++r) {  // a replicate is a resample of n draws: the ranks are those of n
      int64_t sum = 0;
      for (int64_t i = 0; i < n; ++i) sum += counts[(size_t)r * n + i];
      if (sum != n)
        return fail(OB_E_INVALID, "%s: the counts of replicate %d sum to %lld, not to n = %lld", what, r, (long long)sum,
                    (long long)n);
    }
  return OB_OK;
}

int RefitPassInput::upload(const double* y_sorted, int64_t n, const uint8_t* counts_h, int32_t n_reps, const double* x,
                           int64_t ldx, int k, hipStream_t s) {
  tiles = (uint32_t)((n + OB_TILE_ROWS - 1) / OB_TILE_ROWS);
  ld = (int64_t)tiles * OB_TILE_ROWS;
  nb_rep = ((uint32_t)n_reps + 63u) / 64u;
  rep_pad = nb_rep * 64u;
  table.clear();
  group_chunks(0u, tiles, 128u, table);
  n_chunks = (uint32_t)(table.size() / 3);
  mu0 = 0.0;
  for (int64_t i = 0; i < n; ++i) mu0 += y_sorted[i];
  mu0 /= (double)n;
  OB_HIP(cols.alloc(sizeof(double) * (size_t)ld * k));
  OB_HIP(hipMemsetAsync(cols.p, 0, sizeof(double) * (size_t)ld * k, s));
  OB_HIP(hipMemcpyAsync(cols.p, y_sorted, sizeof(double) * n, hipMemcpyHostToDevice, s));
  for (int j = 1; j < k; ++j)
    OB_HIP(hipMemcpyAsync(cols.d() + (size_t)j * ld, x + (size_t)(j - 1) * ldx, sizeof(double) * n, hipMemcpyHostToDevice, s));
  OB_HIP(chunks.alloc(sizeof(uint32_t) * table.size()));
  OB_HIP(hipMemcpyAsync(chunks.p, table.data(), sizeof(uint32_t) * table.size(), hipMemcpyHostToDevice, s));
  if (!counts_h) return OB_OK;
  // the engine's layouts: f64-Gram count images and [replicate][tile] counts
  img.assign((size_t)tiles * nb_rep * 4 * kCimgWords, 0u);
  sums.assign((size_t)n_reps * tiles, 0u);
  pack_count_images(counts_h, n, n, (uint32_t)n_reps, nb_rep, img.data(), sums.data(), tiles);
  OB_HIP(counts.alloc(sizeof(uint32_t) * img.size()));
  OB_HIP(hipMemcpyAsync(counts.p, img.data(), sizeof(uint32_t) * img.size(), hipMemcpyHostToDevice, s));
  OB_HIP(m1.alloc(sizeof(uint32_t) * sums.size()));
  OB_HIP(hipMemcpyAsync(m1.p, sums.data(), sizeof(uint32_t) * sums.size(), hipMemcpyHostToDevice, s));
  return OB_OK;
}

}  // namespace ob
