// ob_density.hip -- the bootstrapped DFL density decomposition (DiNardo, Fortin and Lemieux 1996):
// the densities of the outcome in A, in B and in B reweighted to A's covariates, on a grid, with the propensity logit
// refitted per replicate. The reference crate's dfl.rs gives the three curves once; this is the front end that gives
// them per bootstrap replicate, under the builder's frame conventions and with sample weights.
//
// Per batch of replicates (the resample enters through the engine's level-2 count images, as in ob_reweight.hip):
//   the logit            ob::reweight_logit_batch: the Newton loop of the reweighted decomposition, unchanged;
//   ob_dn_kernel         block per (row chunk, 32 replicates): the weighted Gaussian kernel sums of the chunk's rows at
//                        every grid point as (weight rows) x (kernel values) on v_mfma_f64_16x16x4_f64. The weight
//                        rows c w and, on B's chunks, c w psi are formed in LDS from the count word and x'gamma; a
//                        lane forms its kernel value phi((g_j - y_i) / h) from the staged y and the grid in LDS.
//                        Neither operand is ever stored in HBM;
//   ob_dn_finish_kernel  wave per replicate: the chunk partials in chunk order, the three densities, the three
//                        differences, the effective sample size, the row and ok.
// The point pass is the same code with every row counted once (counts == NULL).
//
// Panel of a run, per group [col][ld]: y | x_1 .. x_{K-1} | w (ones without sample weights), as a reweighted run's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "ob_builder.hpp"
#include "ob_density.hpp"
#include "ob_device.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_model.hpp"
#include "ob_options.hpp"
#include "ob_reweight.hpp"
#include "ob_spec.h"

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;
constexpr int kDB = 256;               // threads of a pass block
constexpr int kDS = 65;                // doubles per staged column (ob_rw_kernel's)
constexpr int kDRT = 2;                // replicate tiles of 16 per block: an exp feeds kDRT (A) or 2 kDRT (B) MFMAs
constexpr int kDReps = 16 * kDRT;      // replicates per block
constexpr int kDWS = kDReps + 16;      // doubles per row of a weight image: the four rows a lane group reads 4 i + rl
                                       // lie 48 doubles apart, on different halves of the 64 banks
constexpr int kDMaxU = ob::kDensityMaxGrid / 64;  // grid tiles per wave: 16 tiles of 16 columns over 4 waves
constexpr double kInvSqrt2Pi = 0.3989422804014326779399460599343819;

struct DnArgs {
  const double* cols[2];  // [y | x_1 .. x_{k-1} | w] x ld, zero past n
  int64_t ld[2];
  uint32_t n[2];
  uint32_t tiles0;         // tiles of group A (the count images hold A's tiles first)
  int k;
  const uint32_t* counts;  // level-2 count images of the batch's first replicate block (NULL: every row once)
  uint32_t nb_rep;         // 64-replicate blocks of the images
  const uint32_t* chunks;  // [chunk][3] = (g, t0, t1)
  int n_chunks;
  uint32_t n_reps, part_pad;
  const double* gamma;     // [replicate][k] (NULL: psi = 1 on every chunk)
  const uint32_t* flags;   // [replicate] ob::kLogitDoneBit | ob::kLogitFailedBit (NULL: every logit is taken as converged)
  const uint32_t* passes;  // [replicate]
  const double* grid;      // [G]
  int G;
  double h[2];             // the bandwidth of each group's chunks
  double* partial;         // [chunk][part_pad][dn_nv(G)]
  double* rows;
  uint8_t* ok;
  int row_len;
};

// Values per (chunk, replicate): sum c w phi at the G grid points | sum c w psi phi at the G grid points (B's chunks
// with a gamma) | sum c w | sum c w psi | sum c (w psi)^2 (psi = 1 where the chunk has none).
__host__ __device__ inline int dn_nv(int G) { return 2 * G + 3; }

inline size_t dn_lds(int k) {
  return sizeof(double) * ((size_t)(k + 1) * kDS + 2 * 64 * kDWS + (size_t)kDReps * (k | 1) + ob::kDensityMaxGrid);
}

// Block = (row chunk, 32 replicates), 4 waves; the staging frame of ob_rw_kernel. Per 64-row sub-tile:
//   stage  y, x_1 .. x_{k-1}, w of the sub-tile -> LDS [col][65], one coalesced load per column;
//   A      thread = (replicate slots t & 15 and 16 + (t & 15), rows 4 (t >> 4) .. + 3: one count word per slot):
//          on B's chunks x'gamma from the staged columns and the slot's gamma (LDS [32][k | 1]), p, the clamp and
//          psi = p / (1 - p) in ob_rw_kernel's expression; the weights c w and c w psi -> LDS [operand][row][48];
//   B      wave w owns the grid tiles w, w + 4, ..: at most 4 tiles x 2 operands x 2 replicate tiles of
//          accumulators. Per 4-row step a lane forms each tile's kernel value phi((g_j - y_i) / h) once, from the
//          staged y and its grid point (a register), and feeds it to the 2 (A's chunks) or 4 (B's) MFMAs of the tile.
//          Padding grid columns contribute zeros; rows past n have count zero.
// A wave owns its tiles over the whole chunk, so there is no block sum: every partial is one accumulator element,
// summed over the chunk's rows in row order. An output element of the MFMA depends on its own A row and B column
// only, so a replicate's partials do not depend on its slot in the block, on its neighbours, on the batch or on
// first_rep. The three denominators are kept per thread and added in row-group order. No atomics.
__global__ __launch_bounds__(kDB) void ob_dn_kernel(const DnArgs a) {
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const int k = a.k, gs = k | 1, ncol = k + 1, wcol = k * kDS, G = a.G;
  const bool psi = g == 1 && a.gamma != nullptr;
  double* stg = dsm;                    // [ncol][kDS]: y, x_1 .. x_{k-1}, w
  double* wl = stg + ncol * kDS;        // [2][64 rows][kDWS]
  double* gm = wl + 2 * 64 * kDWS;      // [kDReps][gs] gamma
  double* gr = gm + kDReps * gs;        // [G] the grid
  double* red = wl;                     // after the last sub-tile: [3][16 row groups][kDReps]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep0 = blockIdx.y * kDReps;
  if (rep0 >= a.n_reps) return;
  if (psi)
    for (int i = tid; i < kDReps * k; i += kDB) {
      const int rr = i / k, j = i - rr * k;
      gm[rr * gs + j] = rep0 + rr < a.n_reps ? a.gamma[(size_t)(rep0 + rr) * k + j] : 0.0;
    }
  for (int i = tid; i < G; i += kDB) gr[i] = a.grid[i];
  __syncthreads();
  const int NT = (G + 15) / 16;  // grid tiles
  const double inv_h = 1.0 / a.h[g];
  const int e16 = lane & 15, rl = lane >> 4;
  double gj[kDMaxU];   // this lane's grid point of each of the wave's tiles
  bool live[kDMaxU];   // false: a padding column
#pragma unroll
  for (int u = 0; u < kDMaxU; ++u) {
    const int j = 16 * (wave + 4 * u) + e16;
    live[u] = j < G;
    gj[u] = live[u] ? gr[j] : 0.0;
  }
  d4 acc0[kDMaxU][kDRT], acc1[kDMaxU][kDRT];
#pragma unroll
  for (int u = 0; u < kDMaxU; ++u)
#pragma unroll
    for (int t = 0; t < kDRT; ++t) {
      acc0[u][t] = d4{0.0, 0.0, 0.0, 0.0};
      acc1[u][t] = d4{0.0, 0.0, 0.0, 0.0};
    }
  double s0[kDRT], s1[kDRT], s2[kDRT];  // c w, c w psi, c (w psi)^2 of this thread's rows
#pragma unroll
  for (int t = 0; t < kDRT; ++t) s0[t] = s1[t] = s2[t] = 0.0;
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's operand reads
      for (int i = tid; i < ncol * 64; i += kDB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kDS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < kDRT; ++t) {
        const int slot = 16 * t + r16;
        const uint32_t rep = rep0 + slot;
        uint32_t word = 0;  // counts of rows 4 q .. 4 q + 3 (the f64 Gram's count-image layout, ob_engine.hpp)
        if (rep < a.n_reps) {
          const size_t tt = (g ? a.tiles0 : 0u) + tile;
          word = a.counts ? a.counts[((tt * a.nb_rep + (rep >> 6)) * 4 + sw) * kCimgWords + (rep & 63u) * kCimgStride + q]
                          : 0x01010101u;
        }
        double zg[4] = {0.0, 0.0, 0.0, 0.0};
        if (word && psi) {
          const double g0 = gm[slot * gs];
#pragma unroll
          for (int i = 0; i < 4; ++i) zg[i] = g0;
          for (int j = 1; j < k; ++j) {
            const double gv = gm[slot * gs + j];
            const double* xj = stg + j * kDS + 4 * q;
#pragma unroll
            for (int i = 0; i < 4; ++i) zg[i] += xj[i] * gv;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t row = 4 * q + i;
          const uint32_t cu = row < nr ? (word >> (8 * i)) & 255u : 0u;
          double w0 = 0.0, w1 = 0.0;
          if (cu) {
            const double c = (double)cu, w = stg[wcol + row];
            double wp = w;
            if (psi) {
              double p = 1.0 / (1.0 + exp(-zg[i]));  // ob_rw_kernel's expression (a NaN stays a NaN)
              p = p < 1e-10 ? 1e-10 : (p > 1.0 - 1e-10 ? 1.0 - 1e-10 : p);
              wp = w * (p / (1.0 - p));
            }
            w0 = c * w;
            w1 = c * wp;
            s0[t] += w0;
            s1[t] += w1;
            s2[t] += c * (wp * wp);
          }
          wl[row * kDWS + slot] = w0;
          wl[(64 + row) * kDWS + slot] = w1;
        }
      }
      __syncthreads();
#pragma unroll 2
      for (int i = 0; i < 16; ++i) {
        const int row = 4 * i + rl;
        double a0[kDRT], a1[kDRT];
#pragma unroll
        for (int t = 0; t < kDRT; ++t) {
          a0[t] = wl[row * kDWS + 16 * t + e16];
          a1[t] = wl[(64 + row) * kDWS + 16 * t + e16];
        }
        const double yv = stg[row];
#pragma unroll
        for (int u = 0; u < kDMaxU; ++u)
          if (wave + 4 * u < NT) {
            const double z = (gj[u] - yv) * inv_h;
            const double b = live[u] ? exp(-0.5 * (z * z)) * kInvSqrt2Pi : 0.0;
#pragma unroll
            for (int t = 0; t < kDRT; ++t) {
              acc0[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[t], b, acc0[u][t], 0, 0, 0);
              if (psi) acc1[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[t], b, acc1[u][t], 0, 0, 0);
            }
          }
      }
    }
  }
  // lane (rl, e16), element r of acc[u][t]: replicate rep0 + 16 t + rl + 4 r, grid point 16 (wave + 4 u) + e16
  const int nv = dn_nv(G);
  double* out = a.partial + (size_t)chunk * a.part_pad * nv;
#pragma unroll
  for (int u = 0; u < kDMaxU; ++u)
    if (wave + 4 * u < NT && live[u])
#pragma unroll
      for (int t = 0; t < kDRT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t rp = rep0 + 16 * t + rl + 4 * r;
          if (rp < a.n_reps) {
            const int j = 16 * (wave + 4 * u) + e16;
            out[(size_t)rp * nv + j] = acc0[u][t][r];
            if (psi) out[(size_t)rp * nv + G + j] = acc1[u][t][r];
          }
        }
  __syncthreads();  // the last sub-tile's operand reads: red lies over wl
#pragma unroll
  for (int t = 0; t < kDRT; ++t) {
    const int slot = 16 * t + r16;
    red[(0 * 16 + q) * kDReps + slot] = s0[t];
    red[(1 * 16 + q) * kDReps + slot] = s1[t];
    red[(2 * 16 + q) * kDReps + slot] = s2[t];
  }
  __syncthreads();
  if (tid < 3 * kDReps) {  // the sums that are not an accumulator's: row groups in order
    const int s = tid / kDReps, slot = tid - s * kDReps;
    double v = 0.0;
    for (int qq = 0; qq < 16; ++qq) v += red[(s * 16 + qq) * kDReps + slot];
    if (rep0 + slot < a.n_reps) out[(size_t)(rep0 + slot) * nv + 2 * G + s] = v;
  }
}

// One wave per replicate: the chunk partials of each group in chunk order, f_A, f_B and f_C at every grid point, the
// three differences, gamma, the effective sample size and the pass count. A replicate whose logit failed or did not
// converge, or one of whose groups has sum c w = 0, gets ok = 0 and a NaN row.
__global__ __launch_bounds__(64) void ob_dn_finish_kernel(const DnArgs a) {
  const int lane = threadIdx.x, k = a.k, G = a.G, nv = dn_nv(G);
  const uint32_t rep = blockIdx.x;
  if (rep >= a.n_reps) return;
  double* row = a.rows + (size_t)rep * a.row_len;
  const uint32_t fl = a.flags ? a.flags[rep] : ob::kLogitDoneBit;
  double da = 0.0, db = 0.0, dc = 0.0, dc2 = 0.0;  // every lane adds the denominators, in chunk order
  for (int c = 0; c < a.n_chunks; ++c) {
    const double* part = a.partial + ((size_t)c * a.part_pad + rep) * nv + 2 * G;
    if (a.chunks[3 * c] == 0) {
      da += part[0];
    } else {
      db += part[0];
      dc += part[1];
      dc2 += part[2];
    }
  }
  const bool failed = !(fl & ob::kLogitDoneBit) || (fl & ob::kLogitFailedBit) || !(da > 0.0) || !(db > 0.0) || !(dc > 0.0);
  if (failed) {
    for (int i = lane; i < a.row_len; i += 64) row[i] = __builtin_nan("");
    if (lane == 0) a.ok[rep] = 0;
    return;
  }
  const double ha = a.h[0] * da, hb = a.h[1] * db, hc = a.h[1] * dc;
  for (int j = lane; j < G; j += 64) {
    double na = 0.0, nb = 0.0, nc = 0.0;
    for (int c = 0; c < a.n_chunks; ++c) {
      const double* part = a.partial + ((size_t)c * a.part_pad + rep) * nv;
      if (a.chunks[3 * c] == 0) {
        na += part[j];
      } else {
        nb += part[j];
        nc += part[G + j];
      }
    }
    const double fa = na / ha, fb = nb / hb, fc = nc / hc;
    row[j] = fa;
    row[G + j] = fb;
    row[2 * G + j] = fc;
    row[3 * G + j] = fa - fb;
    row[4 * G + j] = fc - fb;
    row[5 * G + j] = fa - fc;
  }
  for (int j = lane; j < k; j += 64) row[6 * G + j] = a.gamma[(size_t)rep * k + j];
  if (lane == 0) {
    row[6 * G + k] = dc * dc / dc2;
    row[6 * G + k + 1] = (double)a.passes[rep];
    a.ok[rep] = 1;
  }
}

hipError_t launch_density(const DnArgs& a, hipStream_t s) {
  const size_t lds = dn_lds(a.k);
  hipError_t e = hipFuncSetAttribute((const void*)ob_dn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ob_dn_kernel, dim3(a.n_chunks, (a.n_reps + kDReps - 1) / kDReps), dim3(kDB), lds, s, a);
  return hipGetLastError();
}

thread_local ob_density_timing g_timing = {};

const char* const kLogitFailedText = "%sFailed to solve Information Matrix in Logit. Perfect separation?";  // logit.rs:92

}  // namespace

namespace ob {

int density_check_shape(int k, int64_t n_a, int64_t n_b, int G) {
  if (k < 1 || n_a < 0 || n_b < 0)
    return fail(OB_E_INVALID, "density decomposition: bad shape (k = %d, n_a = %lld, n_b = %lld)", k, (long long)n_a,
                (long long)n_b);
  if (G < 2) return fail(OB_E_INVALID, "density decomposition: the grid needs at least two points, got %d", G);
  if (G > kDensityMaxGrid)
    return fail(OB_E_UNSUPPORTED, "density decomposition: at most %d grid points, got %d", kDensityMaxGrid, G);
  if (k > kReweightMaxK)
    return fail(OB_E_UNSUPPORTED, "density decomposition: at most %d design columns with the intercept, got %d",
                kReweightMaxK, k);
  if (n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31))
    return fail(OB_E_UNSUPPORTED, "density decomposition: groups take fewer than 2^31 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k)
      return fail(OB_E_INSUFFICIENT, "%sdensity decomposition: a group's rows (%lld) must exceed the design columns (%d)",
                  error_prefix(OB_E_INSUFFICIENT), (long long)n, k);
  return OB_OK;
}

// dfl.rs:164-172: g_j = min + j (max - min) / G; the product is rounded before the sum, as the reference's is.
static void density_default_grid(double lo, double hi, int G, std::vector<double>& grid) {
  const double step = (hi - lo) / (double)G;
  grid.resize((size_t)G);
  for (int j = 0; j < G; ++j) {
    const volatile double t = (double)j * step;
    grid[(size_t)j] = lo + t;
  }
}

// The checks of a configuration that need no data; *G: the grid size it asks for (NULL: every default).
static int density_config_check(const ob_density_config* dc, int* G) {
  const int32_t gsz = dc ? dc->grid_size : 0;
  if (gsz < 0) return fail(OB_E_INVALID, "density decomposition: negative grid_size");
  if (dc && dc->grid && gsz == 0) return fail(OB_E_INVALID, "density decomposition: a grid needs its grid_size");
  *G = gsz == 0 ? 100 : gsz;
  if (*G < 2) return fail(OB_E_INVALID, "density decomposition: the grid needs at least two points, got %d", *G);
  if (*G > kDensityMaxGrid)
    return fail(OB_E_UNSUPPORTED, "density decomposition: at most %d grid points, got %d", kDensityMaxGrid, *G);
  if (dc && dc->grid)
    for (int j = 0; j < *G; ++j)
      if (!std::isfinite(dc->grid[j]) || (j > 0 && !(dc->grid[j] > dc->grid[j - 1])))
        return fail(OB_E_INVALID, "density decomposition: the grid must be finite and strictly increasing");
  for (double h : {dc ? dc->bandwidth_a : 0.0, dc ? dc->bandwidth_b : 0.0})
    if (h != 0.0 && !(std::isfinite(h) && h > 0.0))
      return fail(OB_E_INVALID, "density decomposition: a bandwidth must be finite and > 0 (0: Silverman's), got %g", h);
  return OB_OK;
}

// Device side of a prepared density run (the handle's ob_panel is the resampler, as a reweighted handle's).
struct DensityState {
  int k = 0, G = 0;
  std::vector<double> grid;
  double h[2] = {0.0, 0.0};
  DevBuf cols[2];  // [y | x_1 .. x_{k-1} | w] x ld
  DevBuf chunks, d_grid, gamma, flags, passes, lpart, partial;
  int n_chunks = 0;
};

static DensityState* density_state(const ob_prepared* pr) { return model_state<DensityState>(pr, kModelDensity); }

// Replicates per batch (boot_batch_reps) for the chunk partials of a replicate: the logit's and the pass's.
static uint32_t dn_batch_reps(const DensityState* st, uint32_t rep_pad) {
  return boot_batch_reps((size_t)st->n_chunks * (reweight_logit_vals(st->k) + dn_nv(st->G)) * sizeof(double), rep_pad);
}

// Workspace for batches of hb replicates.
static int dn_ensure(DensityState* st, uint32_t hb) {
  OB_HIP(st->gamma.alloc(sizeof(double) * (size_t)hb * st->k));
  OB_HIP(st->flags.alloc(sizeof(uint32_t) * ((size_t)hb + 1)));
  OB_HIP(st->passes.alloc(sizeof(uint32_t) * (size_t)hb));
  OB_HIP(st->lpart.alloc(sizeof(double) * (size_t)st->n_chunks * hb * reweight_logit_vals(st->k)));
  OB_HIP(st->partial.alloc(sizeof(double) * (size_t)st->n_chunks * hb * dn_nv(st->G)));
  return OB_OK;
}

// The stages over one batch of nb replicates (or the point pass): the shared Newton loop, the density pass, the rows.
static int dn_batch(const ob_prepared* pr, const DensityState* st, uint32_t hb, const uint32_t* counts, uint32_t nb_rep,
                    uint32_t nb, double* rows, uint8_t* ok, hipStream_t s) {
  const ob_panel* p = pr->panel;
  LogitBatch lb{};
  DnArgs a{};
  for (int g = 0; g < 2; ++g) {
    lb.cols[g] = a.cols[g] = st->cols[g].d();
    lb.ld[g] = a.ld[g] = p->ld[g];
    lb.n[g] = a.n[g] = p->n[g];
    a.h[g] = st->h[g];
  }
  lb.tiles0 = a.tiles0 = p->ntiles[0];
  lb.k = a.k = st->k;
  lb.counts = a.counts = counts;
  lb.nb_rep = a.nb_rep = nb_rep;
  lb.chunks = a.chunks = st->chunks.as<uint32_t>();
  lb.n_chunks = a.n_chunks = st->n_chunks;
  lb.n_reps = a.n_reps = nb;
  lb.part_pad = a.part_pad = hb;
  lb.gamma = st->gamma.d();
  lb.flags = st->flags.as<uint32_t>();
  lb.active = lb.flags + hb;
  lb.passes = st->passes.as<uint32_t>();
  lb.partial = st->lpart.d();
  a.gamma = lb.gamma;
  a.flags = lb.flags;
  a.passes = lb.passes;
  a.grid = st->d_grid.d();
  a.G = st->G;
  a.partial = st->partial.d();
  a.rows = rows;
  a.ok = ok;
  a.row_len = pr->row_len;
  LogitTimes lt;
  OB_TRY(reweight_logit_batch(lb, s, &lt));
  g_timing.logit_ms += lt.ms;
  g_timing.logit_launches += lt.launches;
  g_timing.logit_passes = std::max(g_timing.logit_passes, lt.passes);
  Events<3> ev;
  OB_HIP(ev.create());
  OB_HIP(hipEventRecord(ev.e[0], s));
  OB_HIP(launch_density(a, s));
  OB_HIP(hipEventRecord(ev.e[1], s));
  hipLaunchKernelGGL(ob_dn_finish_kernel, dim3(nb), dim3(64), 0, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[2], s));
  OB_HIP(hipEventSynchronize(ev.e[2]));
  float m0 = 0.f, m1 = 0.f;
  OB_HIP(hipEventElapsedTime(&m0, ev.e[0], ev.e[1]));
  OB_HIP(hipEventElapsedTime(&m1, ev.e[1], ev.e[2]));
  g_timing.density_ms += m0;
  g_timing.finish_ms += m1;
  return OB_OK;
}

static int dn_point(ob_prepared* pr, DensityState* st) {
  ob_panel* p = pr->panel;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = p->ctx->stream;
  OB_TRY(dn_ensure(st, 64));
  DevBuf d_row, d_ok;
  OB_HIP(d_row.alloc(sizeof(double) * pr->row_len));
  OB_HIP(d_ok.alloc(1));
  OB_TRY(dn_batch(pr, st, 64, nullptr, 1, 1, d_row.d(), d_ok.as<uint8_t>(), s));
  uint8_t okh = 0;
  pr->point_row.assign((size_t)pr->row_len, 0.0);
  OB_HIP(hipMemcpyAsync(pr->point_row.data(), d_row.p, sizeof(double) * pr->row_len, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(&okh, d_ok.p, 1, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  if (!okh) return fail(OB_E_LINALG, kLogitFailedText, error_prefix(OB_E_LINALG));
  return OB_OK;
}

static int dn_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                          hipStream_t stream) {
  DensityState* st = density_state(pr);
  if (!st || (n_reps && (!d_rows || !d_ok))) return fail(OB_E_INVALID, "null pointer");
  uint32_t hb = 0;
  const BootPlan plan{kFitSegReps, kCountBudget, true, [&](uint32_t seg_pad) {
                        g_timing = {};
                        hb = dn_batch_reps(st, seg_pad);
                        return dn_ensure(st, hb);
                      }};
  return boot_segmented(pr, kModelDensity, plan, first_rep, n_reps, d_rows && d_ok, stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t nb_rep, uint32_t, hipStream_t s) {
    return boot_batches(ns, hb, [&](uint32_t b0, uint32_t nb) {  // hb is a multiple of 64: whole image blocks
      return dn_batch(pr, st, hb, pr->panel->d_counts + (size_t)(b0 / 64) * 4 * kCimgWords, nb_rep, nb,
                      d_rows + (s0 + b0) * pr->row_len, d_ok + s0 + b0, s);
    });
  });
}

// installs the builder's hooks when the library loads (ob_model.hpp)
static const bool g_density_hooks_installed = model_install(
    kModelDensity, {dn_boot_device, model_boot_host, [](void* s) { delete static_cast<DensityState*>(s); }});

// Every check of the frame entry points, before any device work and before the context is read: the grid and the
// bandwidths asked for, settings outside the scope, nulls, non-finite values and negative weights in named columns,
// the design (ob::data_matrices), the shape, each group's positive weight, the grid and bandwidths that result. On
// success m holds the design matrices and the groups' weights.
static int dn_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                    const ob_density_config* dc, Config& c, Matrices& m, std::vector<double>& grid, double h[2]) {
  const char* label = model_name(kModelDensity).label;
  OB_TRY(config_from(cfg, c));
  if (!c.normalize.empty()) return model_refuse(kModelDensity, "normalized categoricals are");
  if (c.has_selection || !c.selection_predictors.empty()) return model_refuse(kModelDensity, "Heckman selection settings are");
  if (c.has_cluster) return model_refuse(kModelDensity, "the cluster bootstrap is");
  int G = 0;
  OB_TRY(density_config_check(dc, &G));
  OB_TRY(stage_named(cols, n_cols, n_rows, c, kModelDensity, true, true));
  if (c.has_weights) {
    Frame f;
    OB_TRY(load_frame(cols, n_cols, n_rows, f));
    const Col& wc = f.cols[f.find(c.weights)];
    for (int64_t r = 0; r < f.nrows; ++r)
      if ((wc.kind == OB_COL_F64 && wc.f[r] < 0.0) || (wc.kind == OB_COL_I64 && wc.i[r] < 0))
        return fail(OB_E_INVALID, "%s: column `%s` has a negative weight in row %lld", label, c.weights.c_str(), (long long)r);
  }
  OB_TRY(m.load(cols, n_cols, n_rows, cfg, true));
  if (m.k > kReweightMaxK) OB_TRY(density_check_shape(m.k, m.n[0], m.n[1], G));
  if (m.n[0] == 0 || m.n[1] == 0) return fail(OB_E_GROUP, "%sOne group has no data", error_prefix(OB_E_GROUP));
  OB_TRY(density_check_shape(m.k, m.n[0], m.n[1], G));
  for (int g = 0; g < 2; ++g) {
    if (!m.w(g)) continue;
    double sw = 0.0;
    for (int64_t i = 0; i < m.n[g]; ++i) sw += m.w(g)[i];
    if (!(sw > 0.0))
      return fail(OB_E_INSUFFICIENT, "%s%s: a group has no positive weight", error_prefix(OB_E_INSUFFICIENT), label);
  }
  if (dc && dc->grid) {
    grid.assign(dc->grid, dc->grid + G);
  } else {
    double lo = std::numeric_limits<double>::infinity(), hi = -lo;
    for (int g = 0; g < 2; ++g)
      for (int64_t i = 0; i < m.n[g]; ++i) {
        lo = std::fmin(lo, m.y[g][i]);
        hi = std::fmax(hi, m.y[g][i]);
      }
    if (!(hi > lo)) return fail(OB_E_INVALID, "%s: the outcome is constant, so the default grid has one point", label);
    density_default_grid(lo, hi, G, grid);
  }
  for (int g = 0; g < 2; ++g) {
    h[g] = dc ? (g ? dc->bandwidth_b : dc->bandwidth_a) : 0.0;
    if (h[g] == 0.0) OB_TRY(ob_silverman_bandwidth(m.y[g], m.n[g], &h[g]));
    if (!(std::isfinite(h[g]) && h[g] > 0.0))
      return fail(OB_E_INVALID, "%s: Silverman's bandwidth of group %s is %g; give one that is finite and > 0", label,
                  g ? "B" : "A", h[g]);
  }
  return OB_OK;
}

static int dn_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_density_config* dc, ob_prepared** out) {
  Config c;
  Matrices m;
  std::vector<double> grid;
  double h[2];
  OB_TRY(dn_stage(cols, n_cols, n_rows, cfg, dc, c, m, grid, h));
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  const int k = m.k, G = (int)grid.size();
  DensityState* st = new DensityState();
  st->k = k;
  st->G = G;
  st->grid = grid;
  st->h[0] = h[0];
  st->h[1] = h[1];
  ob_prepared* pr = model_handle(ctx, c, m, kModelDensity, st, density_row_len(k, G), 1);
  auto build = [&]() -> int {
    OB_TRY(outcome_panel(ctx, m, &pr->panel));
    ob_panel* p = pr->panel;
    for (int g = 0; g < 2; ++g) {  // [y | x_1 .. | w] x ld
      OB_TRY(upload_group(st->cols[g], p->ld[g], m.n[g], k, 1, m.y[g], m.x[g]));
      OB_TRY(upload_weights(st->cols[g], p->ld[g], m.n[g], k, m.w(g)));
    }
    OB_TRY(upload_chunks(p, st->chunks, &st->n_chunks));
    OB_HIP(st->d_grid.alloc(sizeof(double) * G));
    OB_HIP(hipMemcpy(st->d_grid.p, grid.data(), sizeof(double) * G, hipMemcpyHostToDevice));
    g_timing = {};
    return dn_point(pr, st);
  };
  return model_built(pr, build(), out);
}

}  // namespace ob

extern "C" {

int ob_density_row_len(int32_t k, int32_t grid_size) {
  return k < 1 || grid_size < 2 || grid_size > OB_DENSITY_MAX_GRID ? 0 : ob::density_row_len(k, grid_size);
}

int ob_density_check_shape(int32_t k, int64_t n_a, int64_t n_b, int32_t grid_size) {
  return ob::density_check_shape(k, n_a, n_b, grid_size);
}

int ob_density_last_timing(ob_density_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

int ob_density_grid(const double* y, int64_t n, int32_t grid_size, double* out) {
  if (!y || !out) return ob::fail(OB_E_INVALID, "null pointer");
  const int G = grid_size == 0 ? 100 : grid_size;
  if (G < 2 || n < 1) return ob::fail(OB_E_INVALID, "ob_density_grid needs n >= 1 and at least two grid points");
  if (G > OB_DENSITY_MAX_GRID)
    return ob::fail(OB_E_UNSUPPORTED, "density decomposition: at most %d grid points, got %d", OB_DENSITY_MAX_GRID, G);
  double lo = std::numeric_limits<double>::infinity(), hi = -lo;
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(y[i])) return ob::fail(OB_E_INVALID, "ob_density_grid: y has a non-finite value in row %lld", (long long)i);
    lo = std::fmin(lo, y[i]);
    hi = std::fmax(hi, y[i]);
  }
  std::vector<double> grid;
  ob::density_default_grid(lo, hi, G, grid);
  std::copy(grid.begin(), grid.end(), out);
  return OB_OK;
}

int ob_builder_prepare_density(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                               const ob_builder_config* cfg, const ob_density_config* dc, ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::dn_prepare(ctx, cols, n_cols, n_rows, cfg, dc, out);
}

int ob_builder_run_density(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                           const ob_builder_config* cfg, const ob_density_config* dc, ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::dn_prepare(ctx, cols, n_cols, n_rows, cfg, dc, &pr));
  const uint64_t reps = pr->cfg.reps;
  std::vector<double> rows((size_t)reps * pr->row_len);
  std::vector<uint8_t> ok(reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::finish(pr, 0, rows.data(), ok.data(), reps, out);
  ob_prepared_destroy(pr);
  return rc;
}

int ob_prepared_density_info(const ob_prepared* prep, ob_density_info* out) {
  if (!prep || !out) return ob::fail(OB_E_INVALID, "null pointer");
  const ob::DensityState* st = ob::density_state(prep);
  if (!st) return ob::fail(OB_E_INVALID, "not a handle of a density decomposition");
  out->grid_size = st->G;
  out->k = st->k;
  out->grid = st->grid.data();
  out->bandwidth_a = st->h[0];
  out->bandwidth_b = st->h[1];
  out->n_a = prep->n_a;
  out->n_b = prep->n_b;
  return OB_OK;
}

// The density pass alone over one group of rows (include/oaxaca_boot.h): with gammas the rows are B's (both weight
// rows; the psi-weighted one is returned), without them A's.
int ob_density_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                    int64_t n, int32_t k, const double* gammas, int32_t m, const double* grid, int32_t grid_size, double h,
                    double* num, double* den, double* den2) {
  const char* what = "ob_density_pass";
  if (!x || !y || !grid || !num || !den || !den2) return ob::fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || k < 1) return ob::fail(OB_E_INVALID, "%s needs n > 0 rows and k >= 1 columns, got n = %lld, k = %d", what, (long long)n, k);
  if (k > ob::kReweightMaxK) return ob::fail(OB_E_UNSUPPORTED, "%s takes at most %d columns, got %d", what, ob::kReweightMaxK, k);
  if (m < 1 || m > OB_DENSITY_MAX_VECTORS || (!gammas && m != 1))
    return ob::fail(OB_E_INVALID, "%s takes 1 to %d coefficient vectors (1 without gammas), got %d", what, OB_DENSITY_MAX_VECTORS, m);
  if (grid_size < 2) return ob::fail(OB_E_INVALID, "%s: the grid needs at least two points, got %d", what, grid_size);
  if (grid_size > OB_DENSITY_MAX_GRID)
    return ob::fail(OB_E_UNSUPPORTED, "%s: at most %d grid points, got %d", what, OB_DENSITY_MAX_GRID, grid_size);
  for (int32_t j = 0; j < grid_size; ++j)
    if (!std::isfinite(grid[j])) return ob::fail(OB_E_INVALID, "%s: the grid must be finite", what);
  if (!(std::isfinite(h) && h > 0.0)) return ob::fail(OB_E_INVALID, "%s: the bandwidth must be finite and > 0, got %g", what, h);
  if (ldx < n) return ob::fail(OB_E_INVALID, "%s: ldx = %lld is below n = %lld", what, (long long)ldx, (long long)n);
  if (n >= ((int64_t)1 << 31)) return ob::fail(OB_E_UNSUPPORTED, "%s takes fewer than 2^31 rows", what);
  for (int64_t i = 0; i < n; ++i)  // the pass takes x_0 = 1 as given
    if (x[i] != 1.0) return ob::fail(OB_E_UNSUPPORTED, "%s: column 0 of x must be the intercept (all ones)", what);
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int G = grid_size, nv = dn_nv(G);
  const uint32_t g = gammas ? 1u : 0u, nn = (uint32_t)n, tiles = (nn + OB_TILE_ROWS - 1) / OB_TILE_ROWS;
  const int64_t ld = (int64_t)tiles * OB_TILE_ROWS;
  std::vector<uint32_t> chunks;
  ob::group_chunks(g, tiles, 64u, chunks);
  const int n_chunks = (int)(chunks.size() / 3);
  DevBuf d_cols, d_chunks, d_gamma, d_grid, d_partial, d_counts;
  const size_t bytes = sizeof(double) * (size_t)ld * (k + 1);
  OB_HIP(d_cols.alloc(bytes));
  OB_HIP(hipMemsetAsync(d_cols.p, 0, bytes, s));
  OB_HIP(hipMemcpyAsync(d_cols.p, y, sizeof(double) * nn, hipMemcpyHostToDevice, s));
  for (int j = 1; j < k; ++j)
    OB_HIP(hipMemcpyAsync(d_cols.d() + (size_t)j * ld, x + (size_t)j * ldx, sizeof(double) * nn, hipMemcpyHostToDevice, s));
  const std::vector<double> unit(w ? 0 : (size_t)nn, 1.0);
  OB_HIP(hipMemcpyAsync(d_cols.d() + (size_t)k * ld, w ? w : unit.data(), sizeof(double) * nn, hipMemcpyHostToDevice, s));
  OB_HIP(d_chunks.alloc(sizeof(uint32_t) * chunks.size()));
  OB_HIP(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(uint32_t) * chunks.size(), hipMemcpyHostToDevice, s));
  if (gammas) {
    OB_HIP(d_gamma.alloc(sizeof(double) * (size_t)m * k));
    OB_HIP(hipMemcpyAsync(d_gamma.p, gammas, sizeof(double) * (size_t)m * k, hipMemcpyHostToDevice, s));
  }
  OB_HIP(d_grid.alloc(sizeof(double) * G));
  OB_HIP(hipMemcpyAsync(d_grid.p, grid, sizeof(double) * G, hipMemcpyHostToDevice, s));
  OB_HIP(d_partial.alloc(sizeof(double) * (size_t)n_chunks * 64 * nv));
  OB_HIP(hipMemsetAsync(d_partial.p, 0, sizeof(double) * (size_t)n_chunks * 64 * nv, s));
  std::vector<uint32_t> img;  // one 64-replicate block of the f64 Gram's count images (ob_engine.hpp)
  if (counts) {               // every replicate counts the rows alike
    img.assign((size_t)tiles * 4 * kCimgWords, 0u);
    ob::pack_count_images(counts, n, 0, (uint32_t)m, 1, img.data(), nullptr, 0);
    OB_HIP(d_counts.alloc(sizeof(uint32_t) * img.size()));
    OB_HIP(hipMemcpyAsync(d_counts.p, img.data(), sizeof(uint32_t) * img.size(), hipMemcpyHostToDevice, s));
  }
  DnArgs a{};
  a.cols[g] = d_cols.d();
  a.ld[g] = ld;
  a.n[g] = nn;
  a.h[g] = h;
  a.tiles0 = 0;  // the images hold this group's tiles alone
  a.k = k;
  a.counts = counts ? d_counts.as<uint32_t>() : nullptr;
  a.nb_rep = 1;
  a.chunks = d_chunks.as<uint32_t>();
  a.n_chunks = n_chunks;
  a.n_reps = (uint32_t)m;
  a.part_pad = 64;
  a.gamma = gammas ? d_gamma.d() : nullptr;
  a.grid = d_grid.d();
  a.G = G;
  a.partial = d_partial.d();
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipEventRecord(ev.e[0], s));
  OB_HIP(launch_density(a, s));
  OB_HIP(hipEventRecord(ev.e[1], s));
  std::vector<double> part((size_t)n_chunks * 64 * nv);
  OB_HIP(hipMemcpyAsync(part.data(), d_partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  g_timing = {};
  g_timing.density_ms = ms;
  const int off = gammas ? G : 0, dslot = gammas ? 1 : 0;
  for (int32_t r = 0; r < m; ++r) {  // chunk order, as the finish kernel
    double d1 = 0.0, d2 = 0.0;
    std::vector<double> acc((size_t)G, 0.0);
    for (int c = 0; c < n_chunks; ++c) {
      const double* p = part.data() + ((size_t)c * 64 + r) * nv;
      for (int j = 0; j < G; ++j) acc[(size_t)j] += p[off + j];
      d1 += p[2 * G + dslot];
      d2 += p[2 * G + 2];
    }
    std::copy(acc.begin(), acc.end(), num + (size_t)r * G);
    den[r] = d1;
    den2[r] = d2;
  }
  return OB_OK;
}

}  // extern "C"
