// ob_nopo.hip -- Nopo's exact-matching decomposition with a bootstrapped common support (Nopo 2008, Stata's
// `nopomatch`). No counterpart in the reference crate.
//
// Per replicate (the resample enters through the engine's level-2 count images, as in ob_binary.hip):
//   ob_nopo_cell_kernel   wave per (row chunk, 64 replicates), lane per replicate: the running sums N = sum c w and
//                         S = sum c (w y) of each fragment (one cell within one chunk) in row order, stored to the
//                         table [fragment][N | S][replicate] at the fragment's end;
//   ob_nopo_row_kernel    lane per replicate: the cells in id order, a cell's fragments in chunk order for A and
//                         for B, the support, the aggregates and the row of include/oaxaca_boot.h.
// The point pass is the same code with every row counted once (counts == NULL).
//
// Each group's rows stand in stable ascending order of cell id (ob::nopo_stage, ob_builder.cpp), so a cell is one run
// of rows and the fragment boundaries are the same for every replicate: the 64 lanes of a wave walk the rows together
// and branch together. Per group the device holds [w | w y] x ld, zero past n.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ob_builder.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_model.hpp"
#include "ob_nopo.hpp"
#include "ob_options.hpp"
#include "ob_spec.h"

namespace {

struct NopoArgs {
  const double* w[2];           // [ld]
  const double* wy[2];          // [ld]
  uint32_t n[2];
  const uint32_t* frag_end[2];  // [fragments of the group + 1]
  uint32_t frag0[2];            // the group's first fragment in the table
  const uint32_t* chunk_first;  // [chunk] its first fragment, within its group
  const uint32_t* chunks;       // [chunk][3] = (g, t0, t1)
  uint32_t tiles0;
  const uint32_t* counts;       // the batch's first 64-replicate block of the count images, or NULL
  uint32_t nb_rep;
  double* table;                // [fragment][2][hb]
  uint32_t hb;                  // replicates of the table: whole blocks of 64
  uint32_t n_reps;              // of the batch
  const uint32_t* cell_first[2];  // [n_cells + 1]
  int32_t n_cells;
  double* rows;
  uint8_t* ok;
};

// Block = one wave = (row chunk, 64-replicate block); lane = replicate. Per 64-row sub-tile the wave copies the
// block's image (4,352 contiguous bytes) to LDS with coalesced loads, the next sub-tile's loads in flight while this
// one is summed; a lane then reads its own 16 count words (stride 17: no bank conflict). w, w y and the fragment ends
// are wave-uniform. The sums are plain f64 multiplies and adds in row order (no FMA: N of unit weights is an exact
// integer, and a whole-cell fragment has the bytes of a serial sum). Nothing is shared between lanes: a replicate's
// table entries depend on the panel and the replicate alone.
__global__ __launch_bounds__(64) void ob_nopo_cell_kernel(const NopoArgs a) {
  __shared__ uint32_t img[2][kCimgWords];
  const uint32_t lane = threadIdx.x;
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const uint32_t n = a.n[g], rb = blockIdx.y;
  const double* __restrict__ w = a.w[g];
  const double* __restrict__ wy = a.wy[g];
  const uint32_t* __restrict__ fend = a.frag_end[g];
  const uint32_t row0 = t0 * OB_TILE_ROWS, row1 = min(t1 * OB_TILE_ROWS, n);
  if (row0 >= row1) return;
  const uint32_t n_sub = (row1 - row0 + 63u) / 64u;
  uint32_t f = a.chunk_first[chunk], end = fend[f];
  double* out = a.table + (size_t)(a.frag0[g] + f) * 2 * a.hb + (size_t)rb * 64 + lane;
  const bool unit = a.counts == nullptr;
  const size_t tile_base = g ? a.tiles0 : 0u;
  auto image = [&](uint32_t s) {  // sub-tile s of the chunk: rows row0 + 64 s ..
    const uint32_t r = row0 + s * 64u;
    return a.counts + (((tile_base + r / OB_TILE_ROWS) * a.nb_rep + rb) * 4 + (r % OB_TILE_ROWS) / 64u) * kCimgWords;
  };
  uint32_t pre[kCimgStride];
  if (!unit) {
    const uint32_t* src = image(0);
#pragma unroll
    for (int i = 0; i < kCimgStride; ++i) pre[i] = src[i * 64 + lane];
  }
  double N = 0.0, S = 0.0;
  for (uint32_t s = 0; s < n_sub; ++s) {
    uint32_t* buf = img[s & 1u];
    if (!unit) {
#pragma unroll
      for (int i = 0; i < kCimgStride; ++i) buf[i * 64 + lane] = pre[i];
    }
    __syncthreads();
    if (!unit && s + 1 < n_sub) {
      const uint32_t* src = image(s + 1);
#pragma unroll
      for (int i = 0; i < kCimgStride; ++i) pre[i] = src[i * 64 + lane];
    }
    const uint32_t r0 = row0 + s * 64u, nr = min(64u, row1 - r0);
    const uint32_t* mine = buf + lane * kCimgStride;
    for (uint32_t q = 0; 4 * q < nr; ++q) {
      const uint32_t word = unit ? 0x01010101u : mine[q];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t i = 4 * q + j;
        if (i >= nr) break;  // uniform
        const uint32_t r = r0 + i;
        const double c = (double)((word >> (8 * j)) & 255u);
        N = __dadd_rn(N, __dmul_rn(c, w[r]));
        S = __dadd_rn(S, __dmul_rn(c, wy[r]));
        if (r + 1 == end) {  // uniform: the fragment's last row
          out[0] = N;
          out[a.hb] = S;
          N = 0.0;
          S = 0.0;
          ++f;
          out += (size_t)2 * a.hb;
          end = fend[f];
        }
      }
    }
  }
}

// Lane = replicate, one wave per 64 of them. The table reads are coalesced across the lanes; the cell and fragment
// walk is wave-uniform, the support decision per lane. Sums of products are formed without FMA, as the cell pass's.
__global__ __launch_bounds__(64) void ob_nopo_row_kernel(const NopoArgs a) {
  const uint32_t rep = blockIdx.x * 64 + threadIdx.x;  // below hb: the table's reads stay inside it
  const double* tab = a.table + rep;
  const size_t hb = a.hb;
  const uint32_t* __restrict__ cfa = a.cell_first[0];
  const uint32_t* __restrict__ cfb = a.cell_first[1];
  double NA = 0.0, SA = 0.0, NB = 0.0, SB = 0.0;      // all cells
  double NAs = 0.0, SAs = 0.0, NBs = 0.0, SBs = 0.0;  // support cells
  double NAo = 0.0, SAo = 0.0, NBo = 0.0, SBo = 0.0;  // the others
  double cf = 0.0, nsup = 0.0;
  uint32_t fa = cfa[0], fb = cfb[0];
  for (int32_t x = 0; x < a.n_cells; ++x) {
    const uint32_t fa1 = cfa[x + 1], fb1 = cfb[x + 1];
    double na = 0.0, sa = 0.0, nb = 0.0, sb = 0.0;
    for (; fa < fa1; ++fa) {
      const double* t = tab + (size_t)(a.frag0[0] + fa) * 2 * hb;
      na += t[0];
      sa += t[hb];
    }
    for (; fb < fb1; ++fb) {
      const double* t = tab + (size_t)(a.frag0[1] + fb) * 2 * hb;
      nb += t[0];
      sb += t[hb];
    }
    NA += na;
    SA += sa;
    NB += nb;
    SB += sb;
    if (na > 0.0 && nb > 0.0) {
      NAs += na;
      SAs += sa;
      NBs += nb;
      SBs += sb;
      cf = __dadd_rn(cf, __dmul_rn(nb, sa / na));
      nsup += 1.0;
    } else {
      NAo += na;
      SAo += sa;
      NBo += nb;
      SBo += sb;
    }
  }
  if (rep >= a.n_reps) return;
  double* row = a.rows + (size_t)rep * ob::kNopoRowLen;
  if (!(nsup > 0.0 && NA > 0.0 && NB > 0.0)) {
    for (int i = 0; i < ob::kNopoRowLen; ++i) row[i] = __builtin_nan("");
    a.ok[rep] = 0;
    return;
  }
  const double eas = SAs / NAs, ebs = SBs / NBs, c = cf / NBs;
  row[0] = SA / NA - SB / NB;
  row[1] = eas - c;
  row[2] = c - ebs;
  row[3] = NAo == 0.0 ? 0.0 : __dmul_rn(NAo / NA, SAo / NAo - eas);
  row[4] = NBo == 0.0 ? 0.0 : __dmul_rn(NBo / NB, ebs - SBo / NBo);
  row[5] = SA / NA;
  row[6] = SB / NB;
  row[7] = eas;
  row[8] = ebs;
  row[9] = c;
  row[10] = NAs / NA;
  row[11] = NBs / NB;
  row[12] = nsup;
  a.ok[rep] = 1;
}

thread_local ob_nopo_timing g_timing = {};

// The cell pass (and, with rows set, the row pass) over one batch; the batch's kernel times are added to g_timing.
int nopo_batch(const NopoArgs& a, int n_chunks, hipStream_t s) {
  Events<3> ev;
  OB_HIP(ev.create());
  const uint32_t blocks = (a.n_reps + 63u) / 64u;
  if ((size_t)blocks * 64 > a.hb) return ob::fail(OB_E_INVALID, "matching decomposition: bad batch");
  OB_HIP(hipEventRecord(ev.e[0], s));
  hipLaunchKernelGGL(ob_nopo_cell_kernel, dim3(n_chunks, blocks), dim3(64), 0, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], s));
  if (a.rows) {
    hipLaunchKernelGGL(ob_nopo_row_kernel, dim3(blocks), dim3(64), 0, s, a);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(ev.e[2], s));
  OB_HIP(hipEventSynchronize(ev.e[2]));
  float m0 = 0.f, m1 = 0.f;
  OB_HIP(hipEventElapsedTime(&m0, ev.e[0], ev.e[1]));
  OB_HIP(hipEventElapsedTime(&m1, ev.e[1], ev.e[2]));
  g_timing.cell_ms += m0;
  g_timing.row_ms += m1;
  return OB_OK;
}

int upload_u32(DevBuf& dst, const std::vector<uint32_t>& v) {
  OB_HIP(dst.alloc(sizeof(uint32_t) * v.size()));
  OB_HIP(hipMemcpy(dst.p, v.data(), sizeof(uint32_t) * v.size(), hipMemcpyHostToDevice));
  return OB_OK;
}

// One group's [w | w y] x ld, zero past n (w NULL: ones).
int upload_wy(DevBuf& dst, int64_t ld, int64_t n, const double* y, const double* w) {
  std::vector<double> h((size_t)2 * ld, 0.0);
  for (int64_t i = 0; i < n; ++i) {
    h[(size_t)i] = w ? w[i] : 1.0;
    h[(size_t)(ld + i)] = w ? w[i] * y[i] : y[i];
  }
  OB_HIP(dst.alloc(sizeof(double) * h.size()));
  OB_HIP(hipMemcpy(dst.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  return OB_OK;
}

}  // namespace

namespace ob {

// Device side of a prepared run, and the point pass's cell table on the host (ob_prepared_nopo_info). The handle's
// ob_panel (no predictors, the sorted outcome alone) is the resampler and the owner of the chunk table.
struct NopoState {
  DevBuf cols[2];  // [w | w y] x ld
  DevBuf chunks, chunk_first, frag_end[2], cell_first[2], table;
  int n_chunks = 0;
  int32_t n_cells = 0;
  uint32_t n_frag[2] = {0, 0};
  std::vector<uint32_t> cell_first_h[2];
  // ob_prepared_nopo_info
  int64_t n_rows = 0;
  int32_t n_support = 0;
  std::vector<int64_t> n_cell[2];
  std::vector<double> w_cell[2], mean_cell[2];
  std::vector<uint8_t> in_support;
  std::vector<int32_t> row_cell;
};

static NopoState* nopo_state(const ob_prepared* pr) { return model_state<NopoState>(pr, kModelNopo); }

static size_t nopo_rep_bytes(const NopoState* st) { return ((size_t)st->n_frag[0] + st->n_frag[1]) * 2 * sizeof(double); }

static NopoArgs nopo_args(const ob_prepared* pr, const NopoState* st) {
  const ob_panel* p = pr->panel;
  NopoArgs a{};
  for (int g = 0; g < 2; ++g) {
    a.w[g] = st->cols[g].d();
    a.wy[g] = st->cols[g].d() + p->ld[g];
    a.n[g] = p->n[g];
    a.frag_end[g] = st->frag_end[g].as<uint32_t>();
    a.cell_first[g] = st->cell_first[g].as<uint32_t>();
  }
  a.frag0[0] = 0;
  a.frag0[1] = st->n_frag[0];
  a.chunk_first = st->chunk_first.as<uint32_t>();
  a.chunks = st->chunks.as<uint32_t>();
  a.tiles0 = p->ntiles[0];
  a.n_cells = st->n_cells;
  return a;
}

// The point pass: unit counts, one replicate; the row into pr->point_row and the cell table into the state.
static int nopo_point(ob_prepared* pr, NopoState* st) {
  ob_panel* p = pr->panel;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = p->ctx->stream;
  const size_t nf = (size_t)st->n_frag[0] + st->n_frag[1];
  OB_HIP(st->table.alloc(nopo_rep_bytes(st) * 64));
  DevBuf d_row, d_ok;
  OB_HIP(d_row.alloc(sizeof(double) * kNopoRowLen));
  OB_HIP(d_ok.alloc(1));
  NopoArgs a = nopo_args(pr, st);
  a.counts = nullptr;
  a.nb_rep = 1;
  a.table = st->table.d();
  a.hb = 64;
  a.n_reps = 1;
  a.rows = d_row.d();
  a.ok = d_ok.as<uint8_t>();
  OB_TRY(engine_order(p, s));
  const int rc = nopo_batch(a, st->n_chunks, s);
  OB_TRY(engine_mark(p, s));
  OB_TRY(rc);
  uint8_t okh = 0;
  pr->point_row.assign((size_t)kNopoRowLen, 0.0);
  std::vector<double> tab(nf * 2 * 64);
  OB_HIP(hipMemcpyAsync(pr->point_row.data(), d_row.p, sizeof(double) * kNopoRowLen, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(&okh, d_ok.p, 1, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(tab.data(), st->table.p, sizeof(double) * tab.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  if (!okh)
    return fail(OB_E_INSUFFICIENT, "%smatching decomposition: no common support", error_prefix(OB_E_INSUFFICIENT));
  // the cell table, a cell's fragments in chunk order as ob_nopo_row_kernel adds them
  st->in_support.assign((size_t)st->n_cells, 0);
  for (int g = 0; g < 2; ++g) {
    st->w_cell[g].assign((size_t)st->n_cells, 0.0);
    st->mean_cell[g].assign((size_t)st->n_cells, 0.0);
    const size_t f0 = g ? st->n_frag[0] : 0;
    for (int32_t x = 0; x < st->n_cells; ++x) {
      double nn = 0.0, ss = 0.0;
      for (uint32_t f = st->cell_first_h[g][(size_t)x]; f < st->cell_first_h[g][(size_t)x + 1]; ++f) {
        nn += tab[(f0 + f) * 2 * 64];
        ss += tab[((f0 + f) * 2 + 1) * 64];
      }
      st->w_cell[g][(size_t)x] = nn;
      st->mean_cell[g][(size_t)x] = nn > 0.0 ? ss / nn : NAN;
    }
  }
  st->n_support = 0;
  for (int32_t x = 0; x < st->n_cells; ++x) {
    st->in_support[(size_t)x] = st->w_cell[0][(size_t)x] > 0.0 && st->w_cell[1][(size_t)x] > 0.0;
    st->n_support += st->in_support[(size_t)x];
  }
  return OB_OK;
}

static int nopo_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                            hipStream_t stream) {
  NopoState* st = nopo_state(pr);
  ob_panel* p = pr ? pr->panel : nullptr;
  const BootPlan plan{kFitSegReps, kCountBudget, false, [&](uint32_t pad) -> int {
                        g_timing = {};
                        OB_HIP(st->table.alloc(nopo_rep_bytes(st) * boot_batch_reps(nopo_rep_bytes(st), pad)));
                        return OB_OK;
                      }};
  return boot_segmented(pr, kModelNopo, plan, first_rep, n_reps, d_rows && d_ok, stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t, uint32_t, hipStream_t s) -> int {
    Events<2> ev;  // the segment's counts (the driver leaves the draw to the segment, for the timing's sake)
    OB_HIP(ev.create());
    uint32_t nb_rep = 0, rep_pad = 0;
    OB_HIP(hipEventRecord(ev.e[0], s));
    OB_TRY(engine_counts(p, pr->seed, first_rep + s0, ns, s, &nb_rep, &rep_pad));
    OB_HIP(hipEventRecord(ev.e[1], s));
    const uint32_t hb = boot_batch_reps(nopo_rep_bytes(st), rep_pad);
    NopoArgs a = nopo_args(pr, st);
    a.nb_rep = nb_rep;
    a.table = st->table.d();
    a.hb = hb;
    OB_TRY(boot_batches(ns, hb, [&](uint32_t b0, uint32_t nb) {
      NopoArgs ab = a;
      ab.counts = p->d_counts + (size_t)(b0 / 64) * 4 * kCimgWords;
      ab.n_reps = nb;
      ab.rows = d_rows + (s0 + b0) * kNopoRowLen;
      ab.ok = d_ok + s0 + b0;
      return nopo_batch(ab, st->n_chunks, s);
    }));
    float ms = 0.f;  // (every batch has waited for its end: the events are complete)
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    g_timing.counts_ms += ms;
    return OB_OK;
  });
}

// installs the builder's hooks when the library loads (ob_model.hpp)
static const bool g_nopo_hooks_installed = model_install(
    kModelNopo, {nopo_boot_device, model_boot_host, [](void* s) { delete static_cast<NopoState*>(s); }});

static int nopo_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                        ob_prepared** out) {
  Config c;
  NopoStaged sg;
  OB_TRY(nopo_stage(cols, n_cols, n_rows, cfg, c, sg, false));
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  Matrices m;  // the sorted outcome for outcome_panel and the row counts for the handle; no design
  for (int g = 0; g < 2; ++g) {
    m.n[g] = (int64_t)sg.g[g].y.size();
    m.y[g] = sg.g[g].y.data();
  }
  NopoState* st = new NopoState();
  st->n_cells = sg.n_cells;
  st->n_rows = n_rows;
  ob_prepared* pr = model_handle(ctx, c, m, kModelNopo, st, kNopoRowLen, 1);
  auto build = [&]() -> int {
    OB_TRY(outcome_panel(ctx, m, &pr->panel));
    OB_TRY(upload_chunks(pr->panel, st->chunks, &st->n_chunks));
    std::vector<uint32_t> table((size_t)3 * st->n_chunks);
    int32_t nc = 0;
    OB_TRY(ob_debug_chunks(pr->panel, table.data(), st->n_chunks, &nc));
    NopoFrags fr[2];
    for (int g = 0; g < 2; ++g) {
      nopo_fragments(sg.g[g].cell, sg.n_cells, table.data(), st->n_chunks, (uint32_t)g, fr[g]);
      st->n_frag[g] = (uint32_t)fr[g].n();
      st->cell_first_h[g] = fr[g].cell_first;
      OB_TRY(upload_u32(st->frag_end[g], fr[g].end));
      OB_TRY(upload_u32(st->cell_first[g], fr[g].cell_first));
      OB_TRY(upload_wy(st->cols[g], pr->panel->ld[g], m.n[g], sg.g[g].y.data(), sg.g[g].w.empty() ? nullptr : sg.g[g].w.data()));
      st->n_cell[g].assign((size_t)sg.n_cells, 0);
      for (int32_t x : sg.g[g].cell) ++st->n_cell[g][(size_t)x];
    }
    std::vector<uint32_t> first;  // per chunk of the table: the groups' chunks stand in the table in their own order
    size_t next[2] = {0, 0};
    for (int ch = 0; ch < st->n_chunks; ++ch) {
      const uint32_t g = table[(size_t)3 * ch];
      first.push_back(fr[g].chunk_first[next[g]++]);
    }
    OB_TRY(upload_u32(st->chunk_first, first));
    st->row_cell = sg.row_cell;
    g_timing = {};
    return nopo_point(pr, st);
  };
  return model_built(pr, build(), out);
}

}  // namespace ob

extern "C" {

int ob_nopo_last_timing(ob_nopo_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

int ob_builder_prepare_nopo(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                            const ob_builder_config* cfg, ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::nopo_prepare(ctx, cols, n_cols, n_rows, cfg, out);
}

int ob_builder_run_nopo(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                        ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::nopo_prepare(ctx, cols, n_cols, n_rows, cfg, &pr));
  const uint64_t reps = pr->cfg.reps;
  std::vector<double> rows((size_t)reps * pr->row_len);
  std::vector<uint8_t> ok(reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::finish(pr, 0, rows.data(), ok.data(), reps, out);
  ob_prepared_destroy(pr);
  return rc;
}

int ob_prepared_nopo_info(const ob_prepared* prep, ob_nopo_info* out) {
  const ob::NopoState* st = ob::nopo_state(prep);
  if (!st || !out) return ob::fail(OB_E_INVALID, "not a matching-decomposition handle");
  out->n_cells = st->n_cells;
  out->n_support_cells = st->n_support;
  out->n_rows = st->n_rows;
  out->n_a = prep->n_a;
  out->n_b = prep->n_b;
  out->n_cell_a = st->n_cell[0].data();
  out->n_cell_b = st->n_cell[1].data();
  out->w_a = st->w_cell[0].data();
  out->w_b = st->w_cell[1].data();
  out->mean_a = st->mean_cell[0].data();
  out->mean_b = st->mean_cell[1].data();
  out->in_support = st->in_support.data();
  out->row_cell = st->row_cell.data();
  return OB_OK;
}

// The cell pass alone (include/oaxaca_boot.h): one group of rows in ascending order of cell, a chunk table of its own.
int ob_nopo_sums(ob_ctx* ctx, const double* y, const double* w, const int32_t* cell, int64_t n, int32_t n_cells,
                 const uint8_t* counts, int32_t n_reps, double* n_sums, double* s_sums) {
  if (!y || !cell || !n_sums || !s_sums) return ob::fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || n_cells <= 0 || n_reps < 1)
    return ob::fail(OB_E_INVALID, "ob_nopo_sums needs n > 0 rows, n_cells > 0 and n_reps >= 1");
  if (!counts && n_reps != 1) return ob::fail(OB_E_INVALID, "ob_nopo_sums: the point pass (no counts) is one replicate");
  if (n >= ((int64_t)1 << 31)) return ob::fail(OB_E_UNSUPPORTED, "ob_nopo_sums takes fewer than 2^31 rows");
  if (n_cells > ob::kNopoMaxCells)
    return ob::fail(OB_E_UNSUPPORTED, "ob_nopo_sums takes at most %lld cells", (long long)ob::kNopoMaxCells);
  for (int64_t i = 0; i < n; ++i) {
    if (cell[i] < 0 || cell[i] >= n_cells || (i && cell[i] < cell[i - 1]))
      return ob::fail(OB_E_INVALID, "ob_nopo_sums: cell ids must lie in [0, n_cells) in ascending order");
    if (!std::isfinite(y[i]) || (w && !(w[i] >= 0.0 && std::isfinite(w[i]))))
      return ob::fail(OB_E_INVALID, "ob_nopo_sums: y must be finite and w finite and not negative");
  }
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint32_t tiles = (uint32_t)((n + OB_TILE_ROWS - 1) / OB_TILE_ROWS), nb_rep = ((uint32_t)n_reps + 63u) / 64u;
  const int64_t ld = (int64_t)tiles * OB_TILE_ROWS;
  std::vector<uint32_t> chunks;
  ob::group_chunks(0u, tiles, 128u, chunks);
  const int n_chunks = (int)(chunks.size() / 3);
  ob::NopoFrags fr;
  ob::nopo_fragments(std::vector<int32_t>(cell, cell + n), n_cells, chunks.data(), n_chunks, 0u, fr);
  const size_t rep_bytes = fr.n() * 2 * sizeof(double);
  const uint32_t hb = ob::boot_batch_reps(rep_bytes, nb_rep * 64u);
  DevBuf d_cols, d_chunks, d_first, d_end, d_counts, d_table;
  OB_TRY(upload_wy(d_cols, ld, n, y, w));
  OB_TRY(upload_u32(d_chunks, chunks));
  OB_TRY(upload_u32(d_first, fr.chunk_first));
  OB_TRY(upload_u32(d_end, fr.end));
  OB_HIP(d_table.alloc(rep_bytes * hb));
  std::vector<uint32_t> img;
  if (counts) {
    img.assign((size_t)tiles * nb_rep * 4 * kCimgWords, 0u);
    ob::pack_count_images(counts, n, n, (uint32_t)n_reps, nb_rep, img.data(), nullptr, 0);
    OB_HIP(d_counts.alloc(sizeof(uint32_t) * img.size()));
    OB_HIP(hipMemcpy(d_counts.p, img.data(), sizeof(uint32_t) * img.size(), hipMemcpyHostToDevice));
  }
  NopoArgs a{};
  a.w[0] = d_cols.d();
  a.wy[0] = d_cols.d() + ld;
  a.n[0] = (uint32_t)n;
  a.frag_end[0] = d_end.as<uint32_t>();
  a.chunk_first = d_first.as<uint32_t>();
  a.chunks = d_chunks.as<uint32_t>();
  a.tiles0 = tiles;
  a.nb_rep = nb_rep;
  a.table = d_table.d();
  a.hb = hb;
  g_timing = {};
  std::vector<double> tab(fr.n() * 2 * hb);
  return ob::boot_batches((uint32_t)n_reps, hb, [&](uint32_t b0, uint32_t nb) -> int {
    NopoArgs ab = a;
    ab.counts = counts ? d_counts.as<uint32_t>() + (size_t)(b0 / 64) * 4 * kCimgWords : nullptr;
    ab.n_reps = nb;
    OB_TRY(nopo_batch(ab, n_chunks, s));
    OB_HIP(hipMemcpy(tab.data(), d_table.p, sizeof(double) * tab.size(), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < nb; ++r)
      for (int32_t x = 0; x < n_cells; ++x) {  // a cell's fragments in chunk order, as ob_nopo_row_kernel
        double nn = 0.0, ss = 0.0;
        for (uint32_t f = fr.cell_first[(size_t)x]; f < fr.cell_first[(size_t)x + 1]; ++f) {
          nn += tab[(size_t)f * 2 * hb + r];
          ss += tab[((size_t)f * 2 + 1) * hb + r];
        }
        n_sums[(size_t)(b0 + r) * n_cells + x] = nn;
        s_sums[(size_t)(b0 + r) * n_cells + x] = ss;
      }
    return OB_OK;
  });
}

}  // extern "C"
