// ob_reweight.hip -- the reweighted Oaxaca-Blinder decomposition with a bootstrapped propensity logit (Fortin,
// Lemieux and Firpo 2011, section 5). No counterpart in the reference crate (dfl.rs stops at
// densities).
//
// Per batch of replicates (the resample enters through the engine's level-2 count images, as in ob_binary.hip):
//   ob_rw_kernel        block per (row chunk, 16 replicates), one kernel with a weight mode:
//                         logit   sum c w p (1 - p) x x' and sum c w (D - p) x of one Newton pass,
//                         Gram    the extended Grams of A and B with weights c w,
//                         GramPsi the extended Gram of B with weights c w psi, psi = p / (1 - p),
//                       all as (weight row) x (pair products) on v_mfma_f64_16x16x4_f64; the index x'gamma and
//                       the weight are formed inside the tile, never stored in HBM;
//   ob_rw_step_kernel   wave per replicate: chunk partials in chunk order, Cholesky, step, stopping rule, the
//                       replicate's done flag and pass count;
//   ob_rw_row_kernel    wave per replicate: the three Grams in chunk order, three Cholesky solves, the means, the
//                       terms of include/oaxaca_boot.h's row.
// The point pass is the same code with every row counted once (counts == NULL).
//
// The factor P(B) / P(A) of dfl.rs:116 is left out of psi: every quantity of the row is a ratio of psi-weighted
// sums, in which it cancels.
//
// Panel of a reweighted run, per group [col][ld]: y | x_1 .. x_{K-1} | w (ones without sample weights).
//
// The decomposition of a statistic is the same code on other outcome columns: after the point
// logit ob_rw_psi_kernel writes w psi-hat for B's rows, three weighted RIF passes (ob_rif.hip) give RIF_A, RIF_B
// and RIF_C, and the panel of T statistics becomes
//   A: RIF_A^0 | x_1 .. x_{K-1} | w | RIF_A^1 .. RIF_A^{T-1}
//   B: RIF_B^0 | x_1 .. x_{K-1} | w | RIF_B^1 .. RIF_B^{T-1} | RIF_C^0 .. RIF_C^{T-1}
// RwArgs::ycol / ycol_c name the column that ob_rw_kernel stages into the y slot under Gram / GramPsi; both are 0
// for the mean. The RIFs are fixed at the point estimate: a replicate refits the logit and the three regressions
// and does not recompute the statistic. Per batch the logit runs once; the two Gram modes and the row kernel run
// once per statistic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ob_builder.hpp"
#include "ob_device.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_model.hpp"
#include "ob_options.hpp"
#include "ob_pairpass.hpp"
#include "ob_reweight.hpp"
#include "ob_rif.hpp"
#include "ob_spec.h"

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;
constexpr int kRB = 256;     // threads of a pass block
constexpr int kRS = 65;      // doubles per staged column: a tile's 16 column reads spread over the banks
constexpr int kRReps = 16;   // replicates per block
constexpr int kRMaxU = 9;    // column tiles per wave: 36 tiles at K = 32 (561 pairs of the extended Gram)
constexpr int kRMaxK = ob::kReweightMaxK;
constexpr uint32_t kRwDone = ob::kLogitDoneBit, kRwFailed = ob::kLogitFailedBit;
constexpr int kModeLogit = 0, kModeGram = 1, kModeGramPsi = 2;

struct RwArgs {
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
  double* gamma;           // [replicate][k]
  uint32_t* flags;         // [replicate] kRwDone | kRwFailed
  uint32_t* passes;        // [replicate] Newton passes taken
  uint32_t* active;        // replicates still iterating after a step
  double* partial;         // [chunk][part_pad][rw_nv(k, mode)] of the logit pass / the c w Grams
  double* partial_c;       // [chunk][part_pad][rw_nv(k, kModeGramPsi)] (B's chunks only)
  double* rows;
  uint8_t* ok;
  int row_len;
  int mode;
  double tol;
  int ycol, ycol_c;        // the column staged into the y slot under Gram / GramPsi (0: the mean's y)
};

// Values per (chunk, replicate): the packed lower triangle (entry j (j + 1) / 2 + i, i <= j) of the k x k
// information matrix then the k gradient entries; or that of the (k + 1) x (k + 1) extended Gram of
// v = [x_0 .. x_{k-1}, y], followed under GramPsi by sum c (w psi)^2.
__host__ __device__ inline int rw_nv(int k, int mode) {
  if (mode == kModeLogit) return k * (k + 1) / 2 + k;
  return (k + 1) * (k + 2) / 2 + (mode == kModeGramPsi ? 1 : 0);
}

inline size_t rw_lds(int k) {
  return sizeof(double) * ((size_t)(k + 2) * kRS + 2 * 64 * kRReps + (size_t)kRReps * (k | 1) + 16 * kRReps);
}

// Block = (row chunk, 16 replicates), 4 waves; the layout of ob_heck_wide_kernel. Per 64-row sub-tile:
//   stage  the k + 1 columns of the sub-tile -> LDS [col][65] (+ a column of ones for x_0), one coalesced load
//          per column, shared by the block;
//   A      thread = (replicate t & 15, rows 4 (t >> 4) .. + 3: one count word): x'gamma from the staged columns
//          and the replicate's gamma (LDS [16][k | 1]), p, the clamp, the mode's weight -> LDS [operand][row][16];
//   B      wave w owns the column tiles w, w + 4, ..: at most 9 accumulators of 16 replicates x 16 columns. Per
//          4-row step a lane reads its A values once and forms each tile's B value as the product of two staged
//          columns (never stored in HBM).
// A wave owns its tiles over the whole chunk, so there is no block sum: every partial is one accumulator
// element, summed over the chunk's rows in row order. An output element of the MFMA depends on its own A row
// and B column only, so a replicate's partials do not depend on its slot in the block, on its neighbours, on
// the batch or on first_rep. No atomics.
__global__ __launch_bounds__(kRB) void ob_rw_kernel(const RwArgs a) {
  extern __shared__ __attribute__((aligned(16))) double rsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const int mode = a.mode;
  if (mode == kModeGramPsi && g == 0) return;  // the counterfactual sample is B's rows
  const int ycol = mode == kModeGramPsi ? a.ycol_c : a.ycol;
  const int k = a.k, gs = k | 1, ncol = k + 1;
  const int ones = ncol * kRS, wcol = k * kRS;
  double* stg = rsm;                    // [ncol + 1][kRS]: y, x_1 .. x_{k-1}, w, ones
  double* wl = stg + (ncol + 1) * kRS;  // [2][64 rows][16 replicates]
  double* gm = wl + 2 * 64 * kRReps;    // [16][gs] gamma
  double* red = gm + kRReps * gs;       // GramPsi: [16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep0 = blockIdx.y * kRReps, rep = rep0 + r16;
  bool act = rep < a.n_reps;
  if (mode == kModeLogit && act) act = !(a.flags[rep] & kRwDone);
  if (!__syncthreads_or(act)) return;
  if (mode != kModeGram)
    for (int i = tid; i < kRReps * k; i += kRB) {
      const int rr = i / k, j = i - rr * k;
      gm[rr * gs + j] = rep0 + rr < a.n_reps ? a.gamma[(size_t)(rep0 + rr) * k + j] : 0.0;
    }
  if (tid < 64) stg[ones + tid] = 1.0;
  // this lane's column of each of the wave's tiles: the two staged columns whose product is the B value, and
  // the slot of the partial it lands in (-1: padding). v_j: x_0 = ones, x_j = column j, y = column 0.
  const int dim = mode == kModeLogit ? k : k + 1;
  const int NP = dim * (dim + 1) / 2;
  const int nt0 = (NP + 15) / 16;                           // tiles of operand 0: the pair products
  const int nt1 = mode == kModeLogit ? (k + 15) / 16 : 0;  // tiles of operand 1: the gradient's columns
  const int NT = nt0 + nt1;
  int oa[kRMaxU], ob2[kRMaxU], dst[kRMaxU];
#pragma unroll
  for (int u = 0; u < kRMaxU; ++u) {
    const int c = wave + 4 * u, e16 = lane & 15;
    oa[u] = ones;
    ob2[u] = ones;
    dst[u] = -1;
    if (c < nt0) {
      const int idx = 16 * c + e16;
      if (idx < NP) {
        const int j = tri_row(idx), i = idx - j * (j + 1) / 2;
        oa[u] = j == 0 ? ones : (j < k ? j * kRS : 0);
        ob2[u] = i == 0 ? ones : (i < k ? i * kRS : 0);
        dst[u] = idx;
      }
    } else if (c < NT) {
      const int idx = 16 * (c - nt0) + e16;
      if (idx < k) {
        oa[u] = idx ? idx * kRS : ones;
        dst[u] = NP + idx;
      }
    }
  }
  d4 acc[kRMaxU];
#pragma unroll
  for (int u = 0; u < kRMaxU; ++u) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
  double s1 = 0.0;  // GramPsi: c (w psi)^2 of this thread's rows
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const uint32_t rb = rep >> 6, R = rep & 63;
  const double dA = g == 0 ? 1.0 : 0.0;  // D = 1[A]
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's operand reads (and the gamma loads)
      for (int i = tid; i < ncol * 64; i += kRB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kRS + r] = (uint32_t)r < nr ? X[(size_t)(c ? c : ycol) * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      uint32_t word = 0;  // counts of rows 4 q .. 4 q + 3 (the f64 Gram's count-image layout, ob_engine.hpp)
      if (act) {
        const size_t tt = (g ? a.tiles0 : 0u) + tile;
        word = a.counts ? a.counts[((tt * a.nb_rep + rb) * 4 + sw) * kCimgWords + R * kCimgStride + q] : 0x01010101u;
      }
      double zg[4] = {0.0, 0.0, 0.0, 0.0};
      if (word && mode != kModeGram) {
        const double g0 = gm[r16 * gs];
#pragma unroll
        for (int i = 0; i < 4; ++i) zg[i] = g0;
        for (int j = 1; j < k; ++j) {
          const double gj = gm[r16 * gs + j];
          const double* xj = stg + j * kRS + 4 * q;
#pragma unroll
          for (int i = 0; i < 4; ++i) zg[i] += xj[i] * gj;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t row = 4 * q + i;
        const uint32_t cu = row < nr ? (word >> (8 * i)) & 255u : 0u;
        double w0 = 0.0, w1 = 0.0;
        if (cu) {
          const double c = (double)cu, w = stg[wcol + row], cw = c * w;
          if (mode == kModeGram) {
            w0 = cw;
          } else {
            double p = 1.0 / (1.0 + exp(-zg[i]));  // logit.rs:15-17, :45 (a NaN stays a NaN)
            p = p < 1e-10 ? 1e-10 : (p > 1.0 - 1e-10 ? 1.0 - 1e-10 : p);
            if (mode == kModeLogit) {
              w0 = cw * (p * (1.0 - p));
              w1 = cw * (dA - p);
            } else {
              const double wp = w * (p / (1.0 - p));
              w0 = c * wp;
              s1 += c * (wp * wp);
            }
          }
        }
        wl[row * kRReps + r16] = w0;
        wl[64 * kRReps + row * kRReps + r16] = w1;
      }
      __syncthreads();
      const int rl = lane >> 4;
#pragma unroll 2
      for (int i = 0; i < 16; ++i) {
        const double a0 = wl[i * 64 + lane], a1 = wl[64 * kRReps + i * 64 + lane];
        const int row = 4 * i + rl;
#pragma unroll
        for (int u = 0; u < kRMaxU; ++u)
          if (wave + 4 * u < NT)
            acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(wave + 4 * u < nt0 ? a0 : a1, stg[oa[u] + row] * stg[ob2[u] + row],
                                                          acc[u], 0, 0, 0);
      }
    }
  }
  // lane (rl, e16), element r of acc[u]: replicate rep0 + rl + 4 r, the tile's column e16
  const int nv = rw_nv(k, mode);
  double* out = (mode == kModeGramPsi ? a.partial_c : a.partial) + (size_t)chunk * a.part_pad * nv;
#pragma unroll
  for (int u = 0; u < kRMaxU; ++u)
    if (wave + 4 * u < NT && dst[u] >= 0)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t rp = rep0 + (lane >> 4) + 4 * r;
        if (rp < a.n_reps) out[(size_t)rp * nv + dst[u]] = acc[u][r];
      }
  if (mode == kModeGramPsi) {  // the sum that is not linear in psi: row groups in order
    red[q * kRReps + r16] = s1;
    __syncthreads();
    if (tid < 16) {
      double v = 0.0;
      for (int qq = 0; qq < 16; ++qq) v += red[qq * kRReps + r16];
      if (rep < a.n_reps) out[(size_t)rep * nv + NP] = v;
    }
  }
}

// out[i] = w_i psi-hat_i for the n rows of one group at the point gamma: the expression of ob_rw_kernel's tile (the
// index summed in column order from the intercept, the clamp, psi = p / (1 - p)). The weights of sample C.
__global__ __launch_bounds__(kRB) void ob_rw_psi_kernel(const double* X, int64_t ld, uint32_t n, int k, const double* gamma,
                                                        double* out) {
  const uint32_t i = blockIdx.x * kRB + threadIdx.x;
  if (i >= n) return;
  double z = gamma[0];
  for (int j = 1; j < k; ++j) z += X[(size_t)j * ld + i] * gamma[j];
  double p = 1.0 / (1.0 + exp(-z));
  p = p < 1e-10 ? 1e-10 : (p > 1.0 - 1e-10 ? 1.0 - 1e-10 : p);
  out[i] = X[(size_t)k * ld + i] * (p / (1.0 - p));
}

// One wave per replicate, after a logit pass: the chunk partials of both groups in chunk order, the Cholesky
// factor of the information matrix, the step, the stopping rule (logit.rs:88-105). A replicate that has
// converged keeps its gamma and its pass count while the batch runs on.
__global__ __launch_bounds__(64) void ob_rw_step_kernel(const RwArgs a) {
  __shared__ double m[kRMaxK * kRMaxK], step[kRMaxK];
  const int lane = threadIdx.x, k = a.k;
  const uint32_t rep = blockIdx.x;
  if (a.flags[rep] & kRwDone) return;
  gather_partials(a.partial, a.part_pad, rep, rw_nv(k, kModeLogit), a.chunks, a.n_chunks, -1, k, lane, m, step);
  __syncthreads();
  const bool chol = wave_cholesky(m, k, lane);
  __syncthreads();
  if (!chol) {
    if (lane == 0) {
      a.flags[rep] = kRwDone | kRwFailed;
      a.passes[rep] += 1;
    }
    return;
  }
  wave_chol_solve(m, k, step, lane);
  __syncthreads();
  if (lane == 0) {
    double nrm = 0.0;
    for (int i = 0; i < k; ++i) {
      a.gamma[(size_t)rep * k + i] += step[i];
      nrm += step[i] * step[i];
    }
    a.passes[rep] += 1;
    if (sqrt(nrm) < a.tol)
      a.flags[rep] = kRwDone;
    else
      atomicAdd(a.active, 1u);
  }
}

// One wave per replicate: the three extended Grams from their chunk partials in chunk order, the three (W)LS
// fits by Cholesky (ob::chol_factor's operation order, wave_cholesky), the means, the terms, the row. A
// replicate whose logit failed or did not converge, or one of whose fits has no Cholesky factor, gets ok = 0
// and a NaN row.
__global__ __launch_bounds__(64) void ob_rw_row_kernel(const RwArgs a) {
  constexpr int M1 = kRMaxK + 1;
  __shared__ double G[3][M1 * (M1 + 1) / 2];
  __shared__ double m[kRMaxK * kRMaxK];
  __shared__ double beta[3][kRMaxK], xbar[3][kRMaxK];
  __shared__ double ess_den;
  const int lane = threadIdx.x, k = a.k, E = (k + 1) * (k + 2) / 2;
  const uint32_t rep = blockIdx.x;
  if (rep >= a.n_reps) return;
  double* row = a.rows + (size_t)rep * a.row_len;
  const uint32_t fl = a.flags[rep];
  bool failed = !(fl & kRwDone) || (fl & kRwFailed);
  if (!failed) {
    for (int i = lane; i < 3 * E + 1; i += 64) {
      const int f = i / E, e = i - f * E;  // f: A, B, C; i == 3 E: sum c (w psi)^2
      const uint32_t g = f == 0 ? 0u : 1u;
      const int nv = rw_nv(k, f == 2 || f == 3 ? kModeGramPsi : kModeGram);
      const double* part = f >= 2 ? a.partial_c : a.partial;
      const int slot = f == 3 ? E : e;
      double v = 0.0;
      for (int c = 0; c < a.n_chunks; ++c)
        if (a.chunks[3 * c] == g) v += part[((size_t)c * a.part_pad + rep) * nv + slot];
      if (f == 3)
        ess_den = v;
      else
        G[f][e] = v;
    }
    __syncthreads();
    for (int f = 0; f < 3 && !failed; ++f) {
      const double* Gf = G[f];
      for (int e = lane; e < k * (k + 1) / 2; e += 64) {
        const int j = tri_row(e), i = e - j * (j + 1) / 2;
        m[j + i * k] = Gf[e];
        m[i + j * k] = Gf[e];
      }
      const int yrow = k * (k + 1) / 2;  // entries (i, k): x_i y
      const double s0 = Gf[0];
      for (int j = lane; j < k; j += 64) {
        beta[f][j] = Gf[yrow + j];
        xbar[f][j] = Gf[j * (j + 1) / 2] / s0;
      }
      __syncthreads();
      const bool chol = wave_cholesky(m, k, lane);
      __syncthreads();
      if (!chol || !(s0 > 0.0)) {
        failed = true;
        break;
      }
      wave_chol_solve(m, k, beta[f], lane);
      __syncthreads();
    }
  }
  if (failed) {
    for (int i = lane; i < a.row_len; i += 64) row[i] = __builtin_nan("");
    if (lane == 0) a.ok[rep] = 0;
    return;
  }
  const double *ba = beta[0], *bb = beta[1], *bc = beta[2], *xa = xbar[0], *xb = xbar[1], *xc = xbar[2];
  double* det = row + 7;
  double* tail = det + 4 * k;
  for (int j = lane; j < k; j += 64) {
    det[j] = (xc[j] - xb[j]) * bb[j];
    det[k + j] = xc[j] * (bc[j] - bb[j]);
    det[2 * k + j] = xa[j] * (ba[j] - bc[j]);
    det[3 * k + j] = (xa[j] - xc[j]) * bc[j];
    tail[j] = ba[j];
    tail[k + j] = bb[j];
    tail[2 * k + j] = bc[j];
    tail[3 * k + j] = xa[j];
    tail[4 * k + j] = xb[j];
    tail[5 * k + j] = xc[j];
    tail[6 * k + j] = a.gamma[(size_t)rep * k + j];
  }
  if (lane == 0) {  // the aggregates, in column order
    const int yrow = k * (k + 1) / 2;
    double faa = 0.0, fbb = 0.0, fcc = 0.0, pe = 0.0, se = 0.0, pu = 0.0, re = 0.0;
    for (int j = 0; j < k; ++j) {
      faa += xa[j] * ba[j];
      fbb += xb[j] * bb[j];
      fcc += xc[j] * bc[j];
      pe += (xc[j] - xb[j]) * bb[j];
      se += xc[j] * (bc[j] - bb[j]);
      pu += xa[j] * (ba[j] - bc[j]);
      re += (xa[j] - xc[j]) * bc[j];
    }
    const double ya = G[0][yrow] / G[0][0], yb = G[1][yrow] / G[1][0], yc = G[2][yrow] / G[2][0];
    row[OB_RW_ROW_TOTAL_GAP] = ya - yb;
    row[OB_RW_ROW_COMPOSITION] = fcc - fbb;
    row[OB_RW_ROW_STRUCTURE] = faa - fcc;
    row[OB_RW_ROW_PURE_EXPLAINED] = pe;
    row[OB_RW_ROW_SPECIFICATION_ERROR] = se;
    row[OB_RW_ROW_PURE_UNEXPLAINED] = pu;
    row[OB_RW_ROW_REWEIGHTING_ERROR] = re;
    double* sc = tail + 7 * k;
    sc[0] = ya;
    sc[1] = yb;
    sc[2] = yc;
    sc[3] = G[2][0] * G[2][0] / ess_den;
    sc[4] = (double)a.passes[rep];
    a.ok[rep] = 1;
  }
}

hipError_t launch_pass(const RwArgs& a, int mode, hipStream_t s) {
  const size_t lds = rw_lds(a.k);
  hipError_t e = hipFuncSetAttribute((const void*)ob_rw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  RwArgs arg = a;
  arg.mode = mode;
  hipLaunchKernelGGL(ob_rw_kernel, dim3(a.n_chunks, (a.n_reps + kRReps - 1) / kRReps), dim3(kRB), lds, s, arg);
  return hipGetLastError();
}

thread_local ob_reweight_timing g_timing = {};
constexpr int kRwMaxPasses = 100;

// The Newton loop of one batch (or of the point pass), every replicate stopping on its own: gamma from 0, one
// logit pass and one step per round until no replicate is left iterating, at most kRwMaxPasses rounds. Shared with
// ob_density.hip through ob::reweight_logit_batch.
int rw_logit_loop(const RwArgs& a, hipStream_t s, ob::LogitTimes* t) {
  if (a.k < 1 || a.k > kRMaxK || a.n_reps < 1 || a.part_pad < a.n_reps) return ob::fail(OB_E_INVALID, "reweight batch: bad shape");
  OB_HIP(hipMemsetAsync(a.gamma, 0, sizeof(double) * (size_t)a.n_reps * a.k, s));
  OB_HIP(hipMemsetAsync(a.flags, 0, sizeof(uint32_t) * a.n_reps, s));
  OB_HIP(hipMemsetAsync(a.passes, 0, sizeof(uint32_t) * a.n_reps, s));
  int it = 0;
  float ms = 0.f;
  OB_TRY(newton_rounds(
      a.active, kRwMaxPasses, s, [&] { return launch_pass(a, kModeLogit, s); },
      [&] {
        hipLaunchKernelGGL(ob_rw_step_kernel, dim3(a.n_reps), dim3(64), 0, s, a);
        return hipGetLastError();
      },
      &it, &ms));
  t->ms += ms;
  t->launches += it;
  t->passes = std::max(t->passes, (int32_t)it);
  return OB_OK;
}

// The stages over one batch (or the point pass): the Newton loop, then per statistic (once for the mean,
// n_stats = 0) the Grams and the rows. rows / ok: one destination per statistic (NULL: a's own).
int rw_batch(const RwArgs& a, hipStream_t s, int n_stats = 0, double* const* rows = nullptr,
             uint8_t* const* ok = nullptr) {
  ob::LogitTimes lt;
  OB_TRY(rw_logit_loop(a, s, &lt));
  g_timing.logit_ms += lt.ms;
  g_timing.logit_launches += lt.launches;
  g_timing.logit_passes = std::max(g_timing.logit_passes, lt.passes);
  Events<5> ev;
  OB_HIP(ev.create());
  for (int t = 0; t < std::max(n_stats, 1); ++t) {
    RwArgs b = a;
    if (n_stats > 0) {
      b.ycol = t ? a.k + t : 0;
      b.ycol_c = a.k + n_stats + t;
    }
    if (rows) {
      b.rows = rows[t];
      b.ok = ok[t];
    }
    OB_HIP(hipEventRecord(ev.e[2], s));
    OB_HIP(launch_pass(b, kModeGram, s));
    OB_HIP(launch_pass(b, kModeGramPsi, s));
    OB_HIP(hipEventRecord(ev.e[3], s));
    hipLaunchKernelGGL(ob_rw_row_kernel, dim3(b.n_reps), dim3(64), 0, s, b);
    OB_HIP(hipGetLastError());
    OB_HIP(hipEventRecord(ev.e[4], s));
    OB_HIP(hipEventSynchronize(ev.e[4]));
    float m0 = 0.f, m1 = 0.f;
    OB_HIP(hipEventElapsedTime(&m0, ev.e[2], ev.e[3]));
    OB_HIP(hipEventElapsedTime(&m1, ev.e[3], ev.e[4]));
    g_timing.gram_ms += m0;
    g_timing.row_ms += m1;
  }
  return OB_OK;
}

// Doubles of chunk partials per replicate and chunk: the logit pass and the c w Grams share one buffer.
size_t partial_vals(int k) { return std::max<size_t>(rw_nv(k, kModeLogit), rw_nv(k, kModeGram)); }
size_t partial_c_vals(int k) { return rw_nv(k, kModeGramPsi); }

const char* const kLogitFailed = "%sFailed to solve Information Matrix in Logit. Perfect separation?";  // logit.rs:92

}  // namespace

namespace ob {

int reweight_check_shape(int k, int64_t n_a, int64_t n_b) {
  if (k < 1 || n_a < 0 || n_b < 0)
    return fail(OB_E_INVALID, "reweighted decomposition: bad shape (k = %d, n_a = %lld, n_b = %lld)", k, (long long)n_a,
                (long long)n_b);
  if (k > kReweightMaxK)
    return fail(OB_E_UNSUPPORTED, "reweighted decomposition: at most %d design columns with the intercept, got %d",
                kReweightMaxK, k);
  if (n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31))
    return fail(OB_E_UNSUPPORTED, "reweighted decomposition: groups take fewer than 2^31 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k)
      return fail(OB_E_INSUFFICIENT,
                  "%sreweighted decomposition: a group's rows (%lld) must exceed the design columns (%d)",
                  error_prefix(OB_E_INSUFFICIENT), (long long)n, k);
  return OB_OK;
}

size_t reweight_logit_vals(int k) { return (size_t)rw_nv(k, kModeLogit); }

int reweight_logit_batch(const LogitBatch& b, hipStream_t s, LogitTimes* t) {
  RwArgs h{};
  for (int g = 0; g < 2; ++g) {
    h.cols[g] = b.cols[g];
    h.ld[g] = b.ld[g];
    h.n[g] = b.n[g];
  }
  h.tiles0 = b.tiles0;
  h.k = b.k;
  h.counts = b.counts;
  h.nb_rep = b.nb_rep;
  h.chunks = b.chunks;
  h.n_chunks = b.n_chunks;
  h.n_reps = b.n_reps;
  h.part_pad = b.part_pad;
  h.gamma = b.gamma;
  h.flags = b.flags;
  h.passes = b.passes;
  h.active = b.active;
  h.partial = b.partial;
  h.tol = 1e-6;
  return rw_logit_loop(h, s, t);
}

// Device side of a prepared reweighted run. The handle's ob_panel (no predictors, the outcome alone) is the
// resampler: engine_counts draws a segment's count images for its row counts, and its chunk table is the one
// the passes walk.
struct ReweightState {
  int k = 0;
  DevBuf cols[2];  // [y | x_1 .. x_{k-1} | w] x ld
  DevBuf chunks, gamma, flags, passes, partial, partial_c;
  int n_chunks = 0;
  // the decomposition of statistics (§5.15): 0 for the mean; the specs, nu_A, nu_B, nu_C and the point row of each
  int n_stats = 0;
  std::vector<ob_rif_spec> specs;
  std::vector<double> nu;  // [n_stats][3]
  std::vector<std::vector<double>> point_rows;
};

static ReweightState* reweight_state(const ob_prepared* pr) { return model_state<ReweightState>(pr, kModelReweight); }

static RwArgs rw_args(const ob_prepared* pr, const ReweightState* st) {
  const ob_panel* p = pr->panel;
  RwArgs h{};
  for (int g = 0; g < 2; ++g) {
    h.cols[g] = st->cols[g].d();
    h.ld[g] = p->ld[g];
    h.n[g] = p->n[g];
  }
  h.tiles0 = p->ntiles[0];
  h.k = st->k;
  h.chunks = st->chunks.as<uint32_t>();
  h.n_chunks = st->n_chunks;
  h.row_len = pr->row_len;
  h.tol = 1e-6;
  return h;
}

// Replicates per batch (boot_batch_reps) for the chunk partials and Grams of a replicate.
static uint32_t rw_batch_reps(const ReweightState* st, uint32_t rep_pad) {
  return boot_batch_reps((size_t)st->n_chunks * (partial_vals(st->k) + partial_c_vals(st->k)) * sizeof(double), rep_pad);
}

// Workspace for batches of hb replicates.
static int rw_ensure(ReweightState* st, uint32_t hb) {
  OB_HIP(st->gamma.alloc(sizeof(double) * (size_t)hb * st->k));
  OB_HIP(st->flags.alloc(sizeof(uint32_t) * ((size_t)hb + 1)));
  OB_HIP(st->passes.alloc(sizeof(uint32_t) * (size_t)hb));
  OB_HIP(st->partial.alloc(sizeof(double) * (size_t)st->n_chunks * hb * partial_vals(st->k)));
  OB_HIP(st->partial_c.alloc(sizeof(double) * (size_t)st->n_chunks * hb * partial_c_vals(st->k)));
  return OB_OK;
}

static void rw_bind(RwArgs& h, const ReweightState* st, uint32_t hb) {
  h.part_pad = hb;
  h.gamma = st->gamma.d();
  h.flags = st->flags.as<uint32_t>();
  h.active = h.flags + hb;
  h.passes = st->passes.as<uint32_t>();
  h.partial = st->partial.d();
  h.partial_c = st->partial_c.d();
}

static int rw_point(ob_prepared* pr, ReweightState* st) {
  ob_panel* p = pr->panel;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = p->ctx->stream;
  OB_TRY(rw_ensure(st, 64));
  const int nt = std::max(st->n_stats, 1);
  DevBuf d_row, d_ok;
  OB_HIP(d_row.alloc(sizeof(double) * pr->row_len * nt));
  OB_HIP(d_ok.alloc((size_t)nt));
  RwArgs h = rw_args(pr, st);
  rw_bind(h, st, 64);
  h.counts = nullptr;
  h.nb_rep = 1;
  h.n_reps = 1;
  std::vector<double*> rows(nt);
  std::vector<uint8_t*> oks(nt);
  for (int t = 0; t < nt; ++t) {
    rows[t] = d_row.d() + (size_t)t * pr->row_len;
    oks[t] = d_ok.as<uint8_t>() + t;
  }
  OB_TRY(rw_batch(h, s, st->n_stats, rows.data(), oks.data()));
  std::vector<uint8_t> okh((size_t)nt, 0);
  std::vector<double> all((size_t)pr->row_len * nt);
  OB_HIP(hipMemcpyAsync(all.data(), d_row.p, sizeof(double) * all.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(okh.data(), d_ok.p, (size_t)nt, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  for (int t = 0; t < nt; ++t)
    if (!okh[t]) return fail(OB_E_LINALG, kLogitFailed, error_prefix(OB_E_LINALG));
  st->point_rows.assign(nt, {});
  for (int t = 0; t < nt; ++t) {
    const auto r0 = all.begin() + (size_t)t * pr->row_len;
    st->point_rows[t].assign(r0, r0 + pr->row_len);
  }
  pr->point_row = st->point_rows[0];
  return OB_OK;
}

// d_rows / d_ok: one destination per statistic of the handle (one for the mean); the multi-destination form is
// reweight's alone, so the driver sees only whether the first pair is set.
static int rw_boot_impl(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* const* d_rows, uint8_t* const* d_ok,
                        hipStream_t stream) {
  ReweightState* st = reweight_state(pr);
  uint32_t hb = 0;
  const BootPlan plan{kFitSegReps, kCountBudget, true, [&](uint32_t seg_pad) {
                        g_timing = {};
                        hb = rw_batch_reps(st, seg_pad);
                        return rw_ensure(st, hb);
                      }};
  return boot_segmented(pr, kModelReweight, plan, first_rep, n_reps, d_rows[0] && d_ok[0], stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t nb_rep, uint32_t, hipStream_t s) {
    return boot_batches(ns, hb, [&](uint32_t b0, uint32_t nb) {  // hb is a multiple of 64: whole image blocks
      RwArgs h = rw_args(pr, st);
      rw_bind(h, st, hb);
      h.counts = pr->panel->d_counts + (size_t)(b0 / 64) * 4 * kCimgWords;
      h.nb_rep = nb_rep;
      h.n_reps = nb;
      double* rows[OB_REWEIGHT_MAX_STATS];
      uint8_t* oks[OB_REWEIGHT_MAX_STATS];
      for (int t = 0; t < std::max(st->n_stats, 1); ++t) {
        rows[t] = d_rows[t] + (s0 + b0) * pr->row_len;
        oks[t] = d_ok[t] + s0 + b0;
      }
      return rw_batch(h, s, st->n_stats, rows, oks);
    });
  });
}

static int rw_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                          hipStream_t stream) {
  const ReweightState* st = reweight_state(pr);
  if (!st || (n_reps && (!d_rows || !d_ok))) return fail(OB_E_INVALID, "null pointer");
  if (st->n_stats > 1) return fail(OB_E_INVALID, "a handle of several statistics boots through its own driver");
  double* const rows[1] = {d_rows};
  uint8_t* const oks[1] = {d_ok};
  return rw_boot_impl(pr, first_rep, n_reps, rows, oks, stream);
}

// installs the builder's hooks when the library loads (ob_model.hpp)
static const bool g_reweight_hooks_installed = model_install(
    kModelReweight, {rw_boot_device, model_boot_host, [](void* s) { delete static_cast<ReweightState*>(s); }});

// Every check of the frame entry points, before any device work and before the context is read: settings
// outside the scope, nulls and non-finite values in named columns, the design (ob::data_matrices), the shape.
// On success m holds the design matrices and the groups' weights.
static int rw_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg, Config& c,
                    Matrices& m) {
  OB_TRY(config_from(cfg, c));
  if (!c.normalize.empty()) return model_refuse(kModelReweight, "normalized categoricals are");
  if (c.has_selection || !c.selection_predictors.empty()) return model_refuse(kModelReweight, "Heckman selection settings are");
  OB_TRY(stage_named(cols, n_cols, n_rows, c, kModelReweight, true, true));
  OB_TRY(m.load(cols, n_cols, n_rows, cfg, true));
  if (m.k > kReweightMaxK) OB_TRY(reweight_check_shape(m.k, m.n[0], m.n[1]));
  if (m.n[0] == 0 || m.n[1] == 0) return fail(OB_E_GROUP, "%sOne group has no data", error_prefix(OB_E_GROUP));
  return reweight_check_shape(m.k, m.n[0], m.n[1]);
}

// The statistics of a prepared handle: with gamma-hat of the point pass on the device, w psi-hat for B's rows, the
// three weighted RIF passes (one sort each serves every statistic), and the RIF columns of the panel.
static int rw_fill_statistics(ob_prepared* pr, ReweightState* st, const double* ya, const double* wa, const double* yb,
                              const double* wb) {
  ob_panel* p = pr->panel;
  const int k = st->k, T = (int)st->specs.size();
  const int64_t n_a = pr->n_a, n_b = pr->n_b;
  hipStream_t s = p->ctx->stream;
  DevBuf d_wc;
  OB_HIP(d_wc.alloc(sizeof(double) * (size_t)n_b));
  hipLaunchKernelGGL(ob_rw_psi_kernel, dim3(blocks_for(n_b)), dim3(kRB), 0, s, st->cols[1].d(), p->ld[1], (uint32_t)n_b, k,
                     st->gamma.d(), d_wc.d());
  OB_HIP(hipGetLastError());
  std::vector<double> wc((size_t)n_b);
  OB_HIP(hipMemcpyAsync(wc.data(), d_wc.p, sizeof(double) * (size_t)n_b, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  std::vector<double> ra((size_t)T * n_a), rb((size_t)T * n_b), rc((size_t)T * n_b), nu((size_t)3 * T);
  OB_TRY(rif_device_weighted(p->ctx, ya, wa, n_a, st->specs.data(), T, ra.data(), nu.data(), true));
  OB_TRY(rif_device_weighted(p->ctx, yb, wb, n_b, st->specs.data(), T, rb.data(), nu.data() + T, false));
  OB_TRY(rif_device_weighted(p->ctx, yb, wc.data(), n_b, st->specs.data(), T, rc.data(), nu.data() + 2 * T, false));
  st->nu.assign((size_t)3 * T, 0.0);
  for (int t = 0; t < T; ++t) {
    for (int f = 0; f < 3; ++f) st->nu[(size_t)3 * t + f] = nu[(size_t)f * T + t];
    const size_t col = t ? (size_t)(k + t) : 0, col_c = (size_t)(k + T + t);
    OB_HIP(hipMemcpy(st->cols[0].d() + col * p->ld[0], ra.data() + (size_t)t * n_a, sizeof(double) * n_a, hipMemcpyHostToDevice));
    OB_HIP(hipMemcpy(st->cols[1].d() + col * p->ld[1], rb.data() + (size_t)t * n_b, sizeof(double) * n_b, hipMemcpyHostToDevice));
    OB_HIP(hipMemcpy(st->cols[1].d() + col_c * p->ld[1], rc.data() + (size_t)t * n_b, sizeof(double) * n_b, hipMemcpyHostToDevice));
  }
  return OB_OK;
}

// n_specs = 0: the mean (ob_builder_prepare_reweighted).
static int rw_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_rif_spec* specs, int32_t n_specs, ob_prepared** out) {
  if (n_specs > 0) {
    OB_TRY(rif_wspec_check(specs, n_specs));
    if (n_specs > OB_REWEIGHT_MAX_STATS)
      return fail(OB_E_UNSUPPORTED, "reweighted decomposition: at most %d statistics in one run, got %d",
                  OB_REWEIGHT_MAX_STATS, n_specs);
  }
  Config c;
  Matrices m;
  OB_TRY(rw_stage(cols, n_cols, n_rows, cfg, c, m));
  const int k = m.k;
  std::vector<double> unit[2];  // the RIF passes' weights of a builder without sample weights
  const double* wrif[2] = {m.w(0), m.w(1)};
  if (n_specs > 0) {
    for (int g = 0; g < 2; ++g)
      if (!wrif[g]) {
        unit[g].assign((size_t)m.n[g], 1.0);
        wrif[g] = unit[g].data();
      }
    OB_TRY(rif_input_check_weighted(m.y[0], wrif[0], m.n[0], specs, n_specs));
    OB_TRY(rif_input_check_weighted(m.y[1], wrif[1], m.n[1], specs, n_specs));
  }
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  ReweightState* st = new ReweightState();
  st->k = k;
  ob_prepared* pr = model_handle(ctx, c, m, kModelReweight, st, reweight_row_len(k), 1);
  auto build = [&]() -> int {
    OB_TRY(outcome_panel(ctx, m, &pr->panel));
    ob_panel* p = pr->panel;
    for (int g = 0; g < 2; ++g) {  // [y | x_1 .. | w | the RIF columns (file header)] x ld
      const int extra = n_specs > 0 ? (g ? 2 * n_specs - 1 : n_specs - 1) : 0;
      OB_TRY(upload_group(st->cols[g], p->ld[g], m.n[g], k, 1 + extra, m.y[g], m.x[g]));
      OB_TRY(upload_weights(st->cols[g], p->ld[g], m.n[g], k, m.w(g)));
    }
    OB_TRY(upload_chunks(p, st->chunks, &st->n_chunks));
    g_timing = {};
    OB_TRY(rw_point(pr, st));
    if (n_specs == 0) return OB_OK;
    // the pass above gave gamma-hat (its fits, on y itself, are dropped); now the RIF columns and the point rows
    st->specs.assign(specs, specs + n_specs);
    OB_TRY(rw_fill_statistics(pr, st, m.y[0], wrif[0], m.y[1], wrif[1]));
    st->n_stats = n_specs;
    return rw_point(pr, st);
  };
  return model_built(pr, build(), out);
}

// The array pieces: one launch of ob_rw_kernel in `mode` over up to two groups of rows (gx[g]: n_g x k
// column-major with ld n_g, column 0 the intercept), every one of the n_gammas replicates counting the rows as
// `counts` does. sums [n_gammas][rw_nv(k, mode)]: the chunk partials added in chunk order.
static int rw_piece(ob_ctx* ctx, int mode, int k, const std::vector<double> (&gx)[2], const std::vector<double> (&gy)[2],
                    const std::vector<double> (&gw)[2], const std::vector<uint8_t> (&gc)[2], bool counted,
                    const double* gammas, int n_gammas, std::vector<double>& sums) {
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  uint32_t n[2], tiles[2];
  int64_t ld[2];
  std::vector<uint32_t> chunks;
  for (int g = 0; g < 2; ++g) {
    n[g] = (uint32_t)gy[g].size();
    tiles[g] = (n[g] + OB_TILE_ROWS - 1) / OB_TILE_ROWS;
    ld[g] = (int64_t)tiles[g] * OB_TILE_ROWS;
    group_chunks((uint32_t)g, tiles[g], 64u, chunks);
  }
  const int n_chunks = (int)(chunks.size() / 3), nv = rw_nv(k, mode);
  DevBuf d_cols[2], d_chunks, d_gamma, d_flags, d_partial, d_counts;
  for (int g = 0; g < 2; ++g) {
    const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(ld[g], 1) * (k + 1);
    OB_HIP(d_cols[g].alloc(bytes));
    OB_HIP(hipMemsetAsync(d_cols[g].p, 0, bytes, s));
    if (!n[g]) continue;
    OB_HIP(hipMemcpyAsync(d_cols[g].p, gy[g].data(), sizeof(double) * n[g], hipMemcpyHostToDevice, s));
    for (int j = 1; j < k; ++j)
      OB_HIP(hipMemcpyAsync(d_cols[g].d() + (size_t)j * ld[g], gx[g].data() + (size_t)j * n[g], sizeof(double) * n[g],
                            hipMemcpyHostToDevice, s));
    OB_HIP(hipMemcpyAsync(d_cols[g].d() + (size_t)k * ld[g], gw[g].data(), sizeof(double) * n[g], hipMemcpyHostToDevice, s));
  }
  OB_HIP(d_chunks.alloc(sizeof(uint32_t) * chunks.size()));
  OB_HIP(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(uint32_t) * chunks.size(), hipMemcpyHostToDevice, s));
  OB_HIP(d_gamma.alloc(sizeof(double) * (size_t)n_gammas * k));
  OB_HIP(hipMemcpyAsync(d_gamma.p, gammas, sizeof(double) * (size_t)n_gammas * k, hipMemcpyHostToDevice, s));
  OB_HIP(d_flags.alloc(sizeof(uint32_t) * 64));
  OB_HIP(hipMemsetAsync(d_flags.p, 0, sizeof(uint32_t) * 64, s));
  OB_HIP(d_partial.alloc(sizeof(double) * (size_t)n_chunks * 64 * nv));
  OB_HIP(hipMemsetAsync(d_partial.p, 0, sizeof(double) * (size_t)n_chunks * 64 * nv, s));
  std::vector<uint32_t> img;  // one 64-replicate block of the f64 Gram's count images (ob_engine.hpp)
  if (counted) {
    img.assign((size_t)(tiles[0] + tiles[1]) * 4 * kCimgWords, 0u);
    for (int g = 0; g < 2; ++g)  // every replicate counts the rows alike
      pack_count_images(gc[g].data(), n[g], 0, (uint32_t)n_gammas, 1, img.data() + (size_t)(g ? tiles[0] : 0u) * 4 * kCimgWords,
                        nullptr, 0);
    OB_HIP(d_counts.alloc(sizeof(uint32_t) * img.size()));
    OB_HIP(hipMemcpyAsync(d_counts.p, img.data(), sizeof(uint32_t) * img.size(), hipMemcpyHostToDevice, s));
  }
  RwArgs h{};
  for (int g = 0; g < 2; ++g) {
    h.cols[g] = d_cols[g].d();
    h.ld[g] = ld[g];
    h.n[g] = n[g];
  }
  h.tiles0 = tiles[0];
  h.k = k;
  h.counts = counted ? d_counts.as<uint32_t>() : nullptr;
  h.nb_rep = 1;
  h.chunks = d_chunks.as<uint32_t>();
  h.n_chunks = n_chunks;
  h.n_reps = (uint32_t)n_gammas;
  h.part_pad = 64;
  h.gamma = d_gamma.d();
  h.flags = d_flags.as<uint32_t>();
  h.partial = d_partial.d();
  h.partial_c = d_partial.d();
  OB_HIP(launch_pass(h, mode, s));
  std::vector<double> part((size_t)n_chunks * 64 * nv);
  OB_HIP(hipMemcpyAsync(part.data(), d_partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  sums.assign((size_t)n_gammas * nv, 0.0);
  for (int c = 0; c < n_chunks; ++c) {  // chunk order, as the step and row kernels
    if (mode == kModeGramPsi && chunks[3 * c] == 0) continue;
    for (int r = 0; r < n_gammas; ++r)
      for (int e = 0; e < nv; ++e) sums[(size_t)r * nv + e] += part[((size_t)c * 64 + r) * nv + e];
  }
  return OB_OK;
}

// The argument checks the two array pieces share (before any device work).
static int rw_piece_check(const char* what, const double* x, int64_t ldx, const double* second, int64_t n, int32_t k,
                          const uint8_t* counts, const double* gammas, int32_t n_gammas, const void* out0, const void* out1) {
  if (!x || !second || !gammas || !out0 || !out1) return fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || k < 1) return fail(OB_E_INVALID, "%s needs n > 0 rows and k >= 1 columns, got n = %lld, k = %d", what, (long long)n, k);
  if (k > kReweightMaxK) return fail(OB_E_UNSUPPORTED, "%s takes at most %d columns, got %d", what, kReweightMaxK, k);
  if (n_gammas < 1 || n_gammas > 64) return fail(OB_E_INVALID, "%s takes 1 to 64 coefficient vectors, got %d", what, n_gammas);
  if (ldx < n) return fail(OB_E_INVALID, "%s: ldx = %lld is below n = %lld", what, (long long)ldx, (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(OB_E_UNSUPPORTED, "%s takes fewer than 2^31 rows", what);
  for (int64_t i = 0; i < n; ++i)  // the pass takes x_0 = 1 as given
    if (x[i] != 1.0) return fail(OB_E_UNSUPPORTED, "%s: column 0 of x must be the intercept (all ones)", what);
  (void)counts;
  return OB_OK;
}

// Copies the rows `take` selects into group g of the piece's inputs.
static void rw_gather(const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts, int64_t n, int k,
                      const std::vector<int64_t>& take, std::vector<double>& gx, std::vector<double>& gy,
                      std::vector<double>& gw, std::vector<uint8_t>& gc) {
  (void)n;
  const size_t m = take.size();
  gx.assign(m * k, 0.0);
  gy.assign(m, 0.0);
  gw.assign(m, 1.0);
  gc.assign(m, 1);
  for (size_t i = 0; i < m; ++i) {
    const int64_t r = take[i];
    for (int j = 0; j < k; ++j) gx[(size_t)j * m + i] = x[(size_t)j * ldx + r];
    if (y) gy[i] = y[r];
    if (w) gw[i] = w[r];
    if (counts) gc[i] = counts[r];
  }
}

}  // namespace ob

extern "C" {

int ob_reweight_row_len(int32_t k) { return k < 1 ? 0 : ob::reweight_row_len(k); }

int ob_reweight_check_shape(int32_t k, int64_t n_a, int64_t n_b) { return ob::reweight_check_shape(k, n_a, n_b); }

int ob_reweight_last_timing(ob_reweight_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

int ob_builder_prepare_reweighted(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                  const ob_builder_config* cfg, ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::rw_prepare(ctx, cols, n_cols, n_rows, cfg, nullptr, 0, out);
}

int ob_builder_prepare_reweighted_statistic(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                            const ob_builder_config* cfg, const ob_rif_spec* spec, ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  OB_TRY(ob::rif_wspec_check(spec, 1));
  return ob::rw_prepare(ctx, cols, n_cols, n_rows, cfg, spec, 1, out);
}

int ob_prepared_reweight_statistics(const ob_prepared* prep, double out[3]) {
  if (!prep || !out) return ob::fail(OB_E_INVALID, "null pointer");
  const ob::ReweightState* st = ob::reweight_state(prep);
  if (!st || st->n_stats != 1) return ob::fail(OB_E_INVALID, "not a handle of a reweighted statistic");
  for (int f = 0; f < 3; ++f) out[f] = st->nu[f];
  return OB_OK;
}

int ob_builder_run_reweighted_statistics(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                         const ob_builder_config* cfg, const ob_rif_spec* specs, int32_t n_specs,
                                         ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  for (int32_t t = 0; t < n_specs && t < OB_REWEIGHT_MAX_STATS; ++t) out[t] = nullptr;
  OB_TRY(ob::rif_wspec_check(specs, n_specs));
  ob_prepared* pr = nullptr;
  OB_TRY(ob::rw_prepare(ctx, cols, n_cols, n_rows, cfg, specs, n_specs, &pr));
  const uint64_t reps = pr->cfg.reps;
  const size_t rl = (size_t)pr->row_len;
  auto run = [&]() -> int {
    std::vector<double> rows((size_t)n_specs * reps * rl);
    std::vector<uint8_t> ok((size_t)n_specs * reps, 0);
    if (reps > 0) {
      OB_HIP(hipSetDevice(pr->panel->ctx->device));
      DevBuf d_rows, d_ok;
      OB_HIP(d_rows.alloc(sizeof(double) * rows.size()));
      OB_HIP(d_ok.alloc(ok.size()));
      double* rp[OB_REWEIGHT_MAX_STATS];
      uint8_t* op[OB_REWEIGHT_MAX_STATS];
      for (int32_t t = 0; t < n_specs; ++t) {
        rp[t] = d_rows.d() + (size_t)t * reps * rl;
        op[t] = d_ok.as<uint8_t>() + (size_t)t * reps;
      }
      OB_TRY(ob::rw_boot_impl(pr, 0, reps, rp, op, nullptr));
      OB_HIP(hipMemcpy(rows.data(), d_rows.p, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
      OB_HIP(hipMemcpy(ok.data(), d_ok.p, ok.size(), hipMemcpyDeviceToHost));
    }
    for (int32_t t = 0; t < n_specs; ++t) {  // finish() reads the handle's point row: statistic t's
      pr->point_row = ob::reweight_state(pr)->point_rows[t];
      OB_TRY(ob::finish(pr, 0, rows.data() + (size_t)t * reps * rl, ok.data() + (size_t)t * reps, reps, &out[t]));
    }
    return OB_OK;
  };
  const int rc = run();
  ob_prepared_destroy(pr);
  if (rc != OB_OK)
    for (int32_t t = 0; t < n_specs; ++t) {
      delete out[t];
      out[t] = nullptr;
    }
  return rc;
}

int ob_builder_run_reweighted(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                              const ob_builder_config* cfg, ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::rw_prepare(ctx, cols, n_cols, n_rows, cfg, nullptr, 0, &pr));
  const uint64_t reps = pr->cfg.reps;
  std::vector<double> rows((size_t)reps * pr->row_len);
  std::vector<uint8_t> ok(reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::finish(pr, 0, rows.data(), ok.data(), reps, out);
  ob_prepared_destroy(pr);
  return rc;
}

// One logit pass alone (include/oaxaca_boot.h). The rows with d = 1 form group A and the others group B, as the
// stacked logit of a run sees them.
int ob_reweight_logit_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* d, const double* w,
                           const uint8_t* counts, int64_t n, int32_t k, const double* gammas, int32_t n_gammas,
                           double* info, double* grad) {
  OB_TRY(ob::rw_piece_check("ob_reweight_logit_pass", x, ldx, d, n, k, counts, gammas, n_gammas, info, grad));
  std::vector<int64_t> take[2];
  for (int64_t i = 0; i < n; ++i) {
    if (d[i] != 0.0 && d[i] != 1.0) return ob::fail(OB_E_INVALID, "ob_reweight_logit_pass: d must be exactly 0.0 or 1.0, got %g", d[i]);
    take[d[i] == 1.0 ? 0 : 1].push_back(i);
  }
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  std::vector<double> gx[2], gy[2], gw[2];
  std::vector<uint8_t> gc[2];
  for (int g = 0; g < 2; ++g) ob::rw_gather(x, ldx, nullptr, w, counts, n, k, take[g], gx[g], gy[g], gw[g], gc[g]);
  std::vector<double> sums;
  OB_TRY(ob::rw_piece(ctx, kModeLogit, k, gx, gy, gw, gc, counts != nullptr, gammas, n_gammas, sums));
  const int NH = k * (k + 1) / 2, nv = NH + k;
  for (int r = 0; r < n_gammas; ++r) {
    for (int j = 0; j < k; ++j) {
      for (int i = 0; i <= j; ++i) {
        const double v = sums[(size_t)r * nv + j * (j + 1) / 2 + i];
        info[((size_t)r * k + j) * k + i] = v;
        info[((size_t)r * k + i) * k + j] = v;
      }
      grad[(size_t)r * k + j] = sums[(size_t)r * nv + NH + j];
    }
  }
  return OB_OK;
}

// The psi-weighted extended Gram alone (include/oaxaca_boot.h): the rows form group B.
int ob_reweight_gram(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                     int64_t n, int32_t k, const double* gammas, int32_t n_gammas, double* gram, double* ess_den) {
  OB_TRY(ob::rw_piece_check("ob_reweight_gram", x, ldx, y, n, k, counts, gammas, n_gammas, gram, ess_den));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  std::vector<int64_t> take(n);
  for (int64_t i = 0; i < n; ++i) take[i] = i;
  std::vector<double> gx[2], gy[2], gw[2];
  std::vector<uint8_t> gc[2];
  ob::rw_gather(x, ldx, y, w, counts, n, k, take, gx[1], gy[1], gw[1], gc[1]);
  std::vector<double> sums;
  OB_TRY(ob::rw_piece(ctx, kModeGramPsi, k, gx, gy, gw, gc, counts != nullptr, gammas, n_gammas, sums));
  const int k1 = k + 1, E = k1 * (k1 + 1) / 2, nv = E + 1;
  for (int r = 0; r < n_gammas; ++r) {
    for (int j = 0; j < k1; ++j)
      for (int i = 0; i <= j; ++i) {
        const double v = sums[(size_t)r * nv + j * (j + 1) / 2 + i];
        gram[((size_t)r * k1 + j) * k1 + i] = v;
        gram[((size_t)r * k1 + i) * k1 + j] = v;
      }
    ess_den[r] = sums[(size_t)r * nv + E];
  }
  return OB_OK;
}

}  // extern "C"
