// ob_dr.hip -- the distribution-regression decomposition of quantile gaps (Chernozhukov, Fernandez-Val and Melly
// 2013, "Inference on counterfactual distributions"). No counterpart in the reference crate.
//
// Per batch of replicates (the resample enters through the engine's level-2 count images, as in ob_reweight.hip):
//   ob_dr_kernel       block per (row chunk, 16 thresholds, replicate): sum c w p (1 - p) x x' and
//                      sum c w (d - p) x of one Newton pass of the 16 logits of d = 1[y <= c_t], as (weight row) x
//                      (pair products) on v_mfma_f64_16x16x4_f64. d, the index x'beta and the weights are formed in
//                      the tile from the staged y and design columns, never stored in HBM; the 16 fits share one
//                      count word per four rows;
//   ob_dr_step_kernel  wave per (replicate, group, threshold): chunk partials in chunk order, Cholesky, step,
//                      stopping rule, the fit's done flag and pass count;
//   ob_dr_cdf_kernel   block per (row chunk, replicate): sum c w L(x'beta_v) for all 2 T coefficient vectors and
//                      sum c w, on the vector units;
//   ob_dr_row_kernel   wave per replicate: the chunks in order, the four F vectors, the rearrangement (a rank sort
//                      of at most 64 values), the inversion at every tau, the effects, ok.
// The point pass is the same code with every row counted once (counts == NULL).
//
// Panel, per group [col][ld]: y | x_1 .. x_{K-1} | w (ones without sample weights), ob_reweight.hip's.
// Coefficients [replicate][group][T][K]; flags and pass counts [replicate][group][T].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ob_builder.hpp"
#include "ob_device.hpp"
#include "ob_dr.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_model.hpp"
#include "ob_options.hpp"
#include "ob_pairpass.hpp"
#include "ob_spec.h"

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;
constexpr int kDB = 256;    // threads of a pass block
constexpr int kDS = 65;     // doubles per staged column: a tile's 16 column reads spread over the banks
constexpr int kDFits = 16;  // thresholds per block
constexpr int kDMaxU = 9;   // column tiles per wave: 33 pair tiles and 2 gradient tiles at K = 32
constexpr int kDMaxK = ob::kDrMaxK;
constexpr int kDMaxT = ob::kDrMaxT;
constexpr uint32_t kDrDone = 1u, kDrFailed = 2u;
constexpr int kFHalf = 128;  // vectors per row half of a distribution-pass block
constexpr int kFRows = 8;    // rows a thread of the distribution pass carries at once

struct DrArgs {
  const double* cols[2];  // [y | x_1 .. x_{k-1} | w] x ld, zero past n
  int64_t ld[2];
  uint32_t n[2];
  uint32_t tiles0;         // tiles of group A (the count images hold A's tiles first)
  int k, T, nq, m;         // m: coefficient vectors of the distribution pass (2 T in a run)
  const uint32_t* counts;  // level-2 count images of the segment (NULL: every row once)
  uint32_t nb_rep;         // 64-replicate blocks of the images
  uint32_t img0;           // the image slot of the batch's replicate 0
  const uint32_t* chunks;  // [chunk][3] = (g, t0, t1)
  int n_chunks;
  uint32_t n_reps, part_pad;
  const double* thr;   // [T]
  const double* taus;  // [nq]
  double* beta;        // [replicate][2][T][k]
  uint32_t* flags;     // [replicate][2][T] kDrDone | kDrFailed
  uint32_t* passes;    // [replicate][2][T] Newton passes taken
  uint32_t* active;    // fits still iterating after a step
  double* partial;     // [chunk][part_pad][T][k (k + 1) / 2 + k]
  double* fpart;       // [chunk][part_pad][m + 1]
  double* rows;
  uint8_t* ok;
  int row_len;
  double tol;
};

__host__ __device__ inline int dr_nv(int k) { return k * (k + 1) / 2 + k; }

__device__ __forceinline__ double dr_sigmoid(double z) {
  double p = 1.0 / (1.0 + exp(-z));
  return p < 1e-10 ? 1e-10 : (p > 1.0 - 1e-10 ? 1.0 - 1e-10 : p);
}

inline size_t dr_lds(int k) {
  return sizeof(double) * ((size_t)(k + 2) * kDS + 2 * 64 * kDFits + (size_t)kDFits * (k | 1));
}

// Block = (row chunk, 16 thresholds, replicate), 4 waves; ob_rw_kernel's layout with the batch axis turned from
// the replicate to the threshold. Per 64-row sub-tile:
//   stage  y, the k - 1 design columns and w of the sub-tile -> LDS [col][65] (+ a column of ones for x_0);
//   A      thread = (threshold t & 15, rows 4 (t >> 4) .. + 3: one count word, the same for the 16 fits):
//          x'beta from the staged columns and the fit's beta (LDS [16][k | 1]), d = (y <= c_t), the clamped p,
//          the weights c w p (1 - p) and c w (d - p) -> LDS [operand][row][16];
//   B      wave w owns the column tiles w, w + 4, ..: at most 9 accumulators of 16 fits x 16 columns. Per 4-row
//          step a lane reads its A values once and forms each tile's B value as the product of two staged
//          columns.
// A wave owns its tiles over the whole chunk, so there is no block sum: every partial is one accumulator element,
// summed over the chunk's rows in row order. An output element of the MFMA depends on its own A row and B column
// only, so a fit's partials do not depend on its neighbours, on the batch or on first_rep. No atomics.
__global__ __launch_bounds__(kDB) void ob_dr_kernel(const DrArgs a) {
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const int k = a.k, T = a.T, gs = k | 1, ncol = k + 1;
  const int ones = ncol * kDS, wcol = k * kDS;
  double* stg = dsm;                    // [ncol + 1][kDS]: y, x_1 .. x_{k-1}, w, ones
  double* wl = stg + (ncol + 1) * kDS;  // [2][64 rows][16 fits]
  double* bt = wl + 2 * 64 * kDFits;    // [16][gs] beta
  const int t16 = tid & 15, q = tid >> 4;
  const uint32_t rep = blockIdx.z;
  const int thr0 = blockIdx.y * kDFits, t = thr0 + t16;
  const size_t fit0 = ((size_t)rep * 2 + g) * T;
  const bool act = t < T && !(a.flags[fit0 + (t < T ? t : 0)] & kDrDone);
  if (!__syncthreads_or(act)) return;  // the 16 fits are all done
  for (int i = tid; i < kDFits * k; i += kDB) {
    const int rr = i / k, j = i - rr * k;
    bt[rr * gs + j] = thr0 + rr < T ? a.beta[(fit0 + thr0 + rr) * k + j] : 0.0;
  }
  if (tid < 64) stg[ones + tid] = 1.0;
  const double ct = t < T ? a.thr[t] : 0.0;
  // this lane's column of each of the wave's tiles: the two staged columns whose product is the B value, and the
  // slot of the partial it lands in (-1: padding). x_0 = ones, x_j = column j.
  const int NP = k * (k + 1) / 2;
  const int nt0 = (NP + 15) / 16;  // tiles of operand 0: the pair products
  const int nt1 = (k + 15) / 16;   // tiles of operand 1: the gradient's columns
  const int NT = nt0 + nt1;
  int oa[kDMaxU], ob2[kDMaxU], dst[kDMaxU];
#pragma unroll
  for (int u = 0; u < kDMaxU; ++u) {
    const int c = wave + 4 * u, e16 = lane & 15;
    oa[u] = ones;
    ob2[u] = ones;
    dst[u] = -1;
    if (c < nt0) {
      const int idx = 16 * c + e16;
      if (idx < NP) {
        const int j = tri_row(idx), i = idx - j * (j + 1) / 2;
        oa[u] = j == 0 ? ones : j * kDS;
        ob2[u] = i == 0 ? ones : i * kDS;
        dst[u] = idx;
      }
    } else if (c < NT) {
      const int idx = 16 * (c - nt0) + e16;
      if (idx < k) {
        oa[u] = idx ? idx * kDS : ones;
        dst[u] = NP + idx;
      }
    }
  }
  d4 acc[kDMaxU];
#pragma unroll
  for (int u = 0; u < kDMaxU; ++u) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const uint32_t img = a.img0 + rep, rb = img >> 6, R = img & 63;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's operand reads (and the beta loads)
      for (int i = tid; i < ncol * 64; i += kDB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kDS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      uint32_t word = 0;  // counts of rows 4 q .. 4 q + 3 (the f64 Gram's count-image layout, ob_engine.hpp)
      if (act) {
        const size_t tt = (g ? a.tiles0 : 0u) + tile;
        word = a.counts ? a.counts[((tt * a.nb_rep + rb) * 4 + sw) * kCimgWords + R * kCimgStride + q] : 0x01010101u;
      }
      double zg[4] = {0.0, 0.0, 0.0, 0.0};
      if (word) {
        const double b0 = bt[t16 * gs];
#pragma unroll
        for (int i = 0; i < 4; ++i) zg[i] = b0;
        for (int j = 1; j < k; ++j) {
          const double bj = bt[t16 * gs + j];
          const double* xj = stg + j * kDS + 4 * q;
#pragma unroll
          for (int i = 0; i < 4; ++i) zg[i] += xj[i] * bj;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t row = 4 * q + i;
        const uint32_t cu = row < nr ? (word >> (8 * i)) & 255u : 0u;
        double w0 = 0.0, w1 = 0.0;
        if (cu) {
          const double cw = (double)cu * stg[wcol + row];
          const double p = dr_sigmoid(zg[i]);
          const double dd = stg[row] <= ct ? 1.0 : 0.0;
          w0 = cw * (p * (1.0 - p));
          w1 = cw * (dd - p);
        }
        wl[row * kDFits + t16] = w0;
        wl[64 * kDFits + row * kDFits + t16] = w1;
      }
      __syncthreads();
      const int rl = lane >> 4;
#pragma unroll 2
      for (int i = 0; i < 16; ++i) {
        const double a0 = wl[i * 64 + lane], a1 = wl[64 * kDFits + i * 64 + lane];
        const int row = 4 * i + rl;
#pragma unroll
        for (int u = 0; u < kDMaxU; ++u)
          if (wave + 4 * u < NT)
            acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(wave + 4 * u < nt0 ? a0 : a1, stg[oa[u] + row] * stg[ob2[u] + row],
                                                          acc[u], 0, 0, 0);
      }
    }
  }
  // lane (rl, e16), element r of acc[u]: threshold thr0 + rl + 4 r, the tile's column e16
  const int nv = dr_nv(k);
  double* out = a.partial + ((size_t)chunk * a.part_pad + rep) * T * nv;
#pragma unroll
  for (int u = 0; u < kDMaxU; ++u)
    if (wave + 4 * u < NT && dst[u] >= 0)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tt = thr0 + (lane >> 4) + 4 * r;
        if (tt < T) out[(size_t)tt * nv + dst[u]] = acc[u][r];
      }
}

// One wave per (replicate, group, threshold), after a logit pass: the chunk partials of the group in chunk order,
// the Cholesky factor of the information matrix, the step, the stopping rule (ob_rw_step_kernel's, per fit). A
// fit that has converged keeps its beta and its pass count while the batch runs on.
__global__ __launch_bounds__(64) void ob_dr_step_kernel(const DrArgs a) {
  __shared__ double m[kDMaxK * kDMaxK], step[kDMaxK];
  const int lane = threadIdx.x, k = a.k, T = a.T;
  const size_t fit = blockIdx.x;
  if (a.flags[fit] & kDrDone) return;
  const uint32_t t = (uint32_t)(fit % T), g = (uint32_t)((fit / T) & 1), rep = (uint32_t)(fit / (2 * (size_t)T));
  gather_partials(a.partial, (size_t)a.part_pad * T, (size_t)rep * T + t, dr_nv(k), a.chunks, a.n_chunks, (int)g, k, lane, m,
                  step);
  __syncthreads();
  const bool chol = wave_cholesky(m, k, lane);
  __syncthreads();
  if (!chol) {
    if (lane == 0) {
      a.flags[fit] = kDrDone | kDrFailed;
      a.passes[fit] += 1;
    }
    return;
  }
  wave_chol_solve(m, k, step, lane);
  __syncthreads();
  if (lane == 0) {
    double nrm = 0.0;
    for (int i = 0; i < k; ++i) {
      a.beta[fit * k + i] += step[i];
      nrm += step[i] * step[i];
    }
    a.passes[fit] += 1;
    if (sqrt(nrm) < a.tol)
      a.flags[fit] = kDrDone;
    else
      atomicAdd(a.active, 1u);
  }
}

inline size_t dr_cdf_lds(int k, int m) {
  return sizeof(double) * ((size_t)k * kDS + 64 + (size_t)k * m + 2 * (kFHalf + 1) + 2);
}

// Block = (row chunk, replicate), 256 threads: thread = (vector v = t & 127, row half h = t >> 7). Per 64-row
// sub-tile the design columns go to LDS once and c w of each row is formed once; a thread then carries x'beta_v
// for eight rows at a time (beta_v from LDS [k][m], the column values broadcast), and adds c w L(x'beta_v) in row
// order. The index is formed on the vector units: a K-deep f64 MFMA would leave the exp, one per (row, vector)
// and about twenty times the K multiply-adds, as the bound all the same, and would need the rows x vectors tile
// staged a second time for it. A thread's sum runs over its half's rows of the whole chunk; the two halves are
// added in a fixed order. No atomics.
__global__ __launch_bounds__(kDB) void ob_dr_cdf_kernel(const DrArgs a) {
  extern __shared__ __attribute__((aligned(16))) double fsm[];
  const int tid = threadIdx.x, v = tid & (kFHalf - 1), h = tid >> 7;
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const uint32_t rep = blockIdx.y;
  const int k = a.k, m = a.m;
  double* stg = fsm;            // [k][kDS]: column j at j (slot 0 unused: x_0 = 1)
  double* cwl = stg + k * kDS;  // [64] c w
  double* bt = cwl + 64;        // [k][m]
  double* red = bt + k * m;     // [2][kFHalf + 1] | [2]
  for (int i = tid; i < k * m; i += kDB) {
    const int j = i / m, vv = i - j * m;
    bt[i] = a.beta[((size_t)rep * m + vv) * k + j];
  }
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const uint32_t img = a.img0 + rep, rb = img >> 6, R = img & 63;
  double acc = 0.0, scw = 0.0;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();
      for (int i = tid; i < (k - 1) * 64; i += kDB) {
        const int c = 1 + (i >> 6), r = i & 63;
        stg[c * kDS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      if (tid < 64) {
        double cw = 0.0;
        if ((uint32_t)tid < nr) {
          const size_t tt = (g ? a.tiles0 : 0u) + tile;
          const uint32_t word =
              a.counts ? a.counts[((tt * a.nb_rep + rb) * 4 + sw) * kCimgWords + R * kCimgStride + (tid >> 2)] : 0x01010101u;
          const uint32_t cu = (word >> (8 * (tid & 3))) & 255u;
          if (cu) cw = (double)cu * X[(size_t)k * ld + r0 + tid];
        }
        cwl[tid] = cw;
      }
      __syncthreads();
      if (v < m) {
        for (int rg = 0; rg < 32 / kFRows; ++rg) {
          const int base = 32 * h + kFRows * rg;
          if ((uint32_t)base >= nr) break;
          double z[kFRows];
          const double b0 = bt[v];
#pragma unroll
          for (int i = 0; i < kFRows; ++i) z[i] = b0;
          for (int j = 1; j < k; ++j) {
            const double bj = bt[j * m + v];
            const double* xj = stg + j * kDS + base;
#pragma unroll
            for (int i = 0; i < kFRows; ++i) z[i] += xj[i] * bj;
          }
#pragma unroll
          for (int i = 0; i < kFRows; ++i) {
            const double cw = cwl[base + i];
            if (cw != 0.0) acc += cw * dr_sigmoid(z[i]);
            scw += cw;
          }
        }
      }
    }
  }
  red[h * (kFHalf + 1) + v] = acc;
  if (v == 0) red[2 * (kFHalf + 1) + h] = scw;
  __syncthreads();
  double* out = a.fpart + ((size_t)chunk * a.part_pad + rep) * (m + 1);
  if (tid < m) out[tid] = red[tid] + red[kFHalf + 1 + tid];
  if (tid == 0) out[m] = red[2 * (kFHalf + 1)] + red[2 * (kFHalf + 1) + 1];
}

// One wave per replicate: the distribution partials in chunk order, the four F vectors, the rearrangement of
// F_AA, F_BB and F_C (a rank sort: position = the number of smaller values, ties by index), the inversion at every
// tau, the effects, the row. A replicate one of whose fits failed or did not converge gets ok = 0 and a NaN row.
__global__ __launch_bounds__(64) void ob_dr_row_kernel(const DrArgs a) {
  __shared__ double F[4][kDMaxT], S[3][kDMaxT], Q[3][ob::kDrMaxQ], wsum[2];
  const int lane = threadIdx.x, T = a.T, nq = a.nq, m = 2 * T;
  const uint32_t rep = blockIdx.x;
  if (rep >= a.n_reps) return;
  double* row = a.rows + (size_t)rep * a.row_len;
  bool bad = false;
  uint32_t mp = 0;
  for (int i = lane; i < m; i += 64) {
    const uint32_t fl = a.flags[(size_t)rep * m + i];
    bad = bad || !(fl & kDrDone) || (fl & kDrFailed);
    mp = max(mp, a.passes[(size_t)rep * m + i]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mp = max(mp, (uint32_t)__shfl_xor((int)mp, off));
  if (lane < 2) {
    double s = 0.0;
    for (int c = 0; c < a.n_chunks; ++c)
      if (a.chunks[3 * c] == (uint32_t)lane) s += a.fpart[((size_t)c * a.part_pad + rep) * (m + 1) + m];
    wsum[lane] = s;
    bad = bad || !(s > 0.0);
  }
  __syncthreads();
  if (__any(bad)) {
    for (int i = lane; i < a.row_len; i += 64) row[i] = __builtin_nan("");
    if (lane == 0) a.ok[rep] = 0;
    return;
  }
  if (lane < T) {
    for (int f = 0; f < 4; ++f) {  // AA, BB, AB, BA: (rows j, coefficients gv)
      const uint32_t j = (f == 1 || f == 3) ? 1u : 0u, gv = (f == 1 || f == 2) ? 1u : 0u;
      double s = 0.0;
      for (int c = 0; c < a.n_chunks; ++c)
        if (a.chunks[3 * c] == j) s += a.fpart[((size_t)c * a.part_pad + rep) * (m + 1) + gv * T + lane];
      F[f][lane] = s / wsum[j];
    }
  }
  __syncthreads();
  if (lane < T) {
    for (int f = 0; f < 3; ++f) {
      const double x = F[f][lane];
      int rank = 0;
      for (int s = 0; s < T; ++s) {
        const double y = F[f][s];
        rank += (y < x || (y == x && s < lane)) ? 1 : 0;
      }
      S[f][rank] = x;
    }
  }
  __syncthreads();
  for (int idx = lane; idx < 3 * nq; idx += 64) {
    const int f = idx / nq, qi = idx - f * nq;
    const double tau = a.taus[qi];
    const double* s = S[f];
    int t = 0;
    while (t < T && !(s[t] >= tau)) ++t;
    double qv;
    if (t == T)
      qv = a.thr[T - 1];
    else if (t == 0)
      qv = a.thr[0];
    else
      qv = a.thr[t - 1] + (tau - s[t - 1]) * (a.thr[t] - a.thr[t - 1]) / (s[t] - s[t - 1]);
    Q[f][qi] = qv;
  }
  __syncthreads();
  double* qe = row;                      // [3][nq]: total, composition, structure
  double* qs = row + 3 * nq;             // [3][nq]: Q_A, Q_B, Q_C
  double* de = row + 6 * nq;             // [3][T]
  double* fr = row + 6 * nq + 3 * T;     // [4][T]
  for (int qi = lane; qi < nq; qi += 64) {
    const double qa = Q[0][qi], qb = Q[1][qi], qc = Q[2][qi];
    qe[qi] = qa - qb;
    qe[nq + qi] = qc - qb;
    qe[2 * nq + qi] = qa - qc;
    qs[qi] = qa;
    qs[nq + qi] = qb;
    qs[2 * nq + qi] = qc;
  }
  if (lane < T) {
    const double faa = F[0][lane], fbb = F[1][lane], fc = F[2][lane];
    de[lane] = faa - fbb;
    de[T + lane] = fc - fbb;
    de[2 * T + lane] = faa - fc;
    for (int f = 0; f < 4; ++f) fr[f * T + lane] = F[f][lane];
  }
  if (lane == 0) {
    row[6 * nq + 7 * T] = (double)mp;
    a.ok[rep] = 1;
  }
}

hipError_t launch_pass(const DrArgs& a, hipStream_t s) {
  const size_t lds = dr_lds(a.k);
  hipError_t e = hipFuncSetAttribute((const void*)ob_dr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ob_dr_kernel, dim3(a.n_chunks, (a.T + kDFits - 1) / kDFits, a.n_reps), dim3(kDB), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_cdf(const DrArgs& a, hipStream_t s) {
  const size_t lds = dr_cdf_lds(a.k, a.m);
  hipError_t e = hipFuncSetAttribute((const void*)ob_dr_cdf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ob_dr_cdf_kernel, dim3(a.n_chunks, a.n_reps), dim3(kDB), lds, s, a);
  return hipGetLastError();
}

thread_local ob_dr_timing g_timing = {};
constexpr int kDrMaxPasses = 100;
constexpr uint32_t kDrMaxBatch = 32768;  // replicates of a batch: the grid's z extent

// The stages over one batch (or the point pass): the Newton loop, each fit stopping on its own, then the
// distribution pass and the rows.
int dr_batch(const DrArgs& a, hipStream_t s) {
  if (a.k < 1 || a.k > kDMaxK || a.T < 2 || a.T > kDMaxT || a.n_reps < 1 || a.part_pad < a.n_reps || a.n_reps > kDrMaxBatch)
    return ob::fail(OB_E_INVALID, "distribution regression batch: bad shape");
  Events<3> ev;
  OB_HIP(ev.create());
  const size_t fits = (size_t)a.n_reps * 2 * a.T;
  OB_HIP(hipMemsetAsync(a.beta, 0, sizeof(double) * fits * a.k, s));
  OB_HIP(hipMemsetAsync(a.flags, 0, sizeof(uint32_t) * fits, s));
  OB_HIP(hipMemsetAsync(a.passes, 0, sizeof(uint32_t) * fits, s));
  int it = 0;
  float ms = 0.f;
  OB_TRY(newton_rounds(
      a.active, kDrMaxPasses, s, [&] { return launch_pass(a, s); },
      [&] {
        hipLaunchKernelGGL(ob_dr_step_kernel, dim3((unsigned)fits), dim3(64), 0, s, a);
        return hipGetLastError();
      },
      &it, &ms));
  g_timing.pass_ms += ms;
  g_timing.launches += it;
  g_timing.passes = std::max(g_timing.passes, (int32_t)it);
  OB_HIP(hipEventRecord(ev.e[0], s));
  OB_HIP(launch_cdf(a, s));
  OB_HIP(hipEventRecord(ev.e[1], s));
  hipLaunchKernelGGL(ob_dr_row_kernel, dim3(a.n_reps), dim3(64), 0, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[2], s));
  OB_HIP(hipEventSynchronize(ev.e[2]));
  float m0 = 0.f, m1 = 0.f;
  OB_HIP(hipEventElapsedTime(&m0, ev.e[0], ev.e[1]));
  OB_HIP(hipEventElapsedTime(&m1, ev.e[1], ev.e[2]));
  g_timing.cdf_ms += m0;
  g_timing.row_ms += m1;
  return OB_OK;
}

const char* const kDrFitFailed =
    "%sdistribution regression: a threshold logit of the point pass did not converge or has no Cholesky factor (a "
    "threshold that nobody or everybody of a group lies under?)";

}  // namespace

namespace ob {

int dr_check_shape(int k, int64_t n_a, int64_t n_b, int T, int nq) {
  if (k < 1 || n_a < 0 || n_b < 0)
    return fail(OB_E_INVALID, "distribution regression: bad shape (k = %d, n_a = %lld, n_b = %lld)", k, (long long)n_a,
                (long long)n_b);
  if (k > kDrMaxK)
    return fail(OB_E_UNSUPPORTED, "distribution regression: at most %d design columns with the intercept, got %d", kDrMaxK, k);
  if (T > kDrMaxT) return fail(OB_E_UNSUPPORTED, "distribution regression: at most %d thresholds, got %d", kDrMaxT, T);
  if (nq > kDrMaxQ) return fail(OB_E_UNSUPPORTED, "distribution regression: at most %d quantiles, got %d", kDrMaxQ, nq);
  if (T < 2) return fail(OB_E_INVALID, "distribution regression: at least two thresholds, got %d", T);
  if (nq < 1) return fail(OB_E_INVALID, "distribution regression: at least one quantile, got %d", nq);
  if (n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31))
    return fail(OB_E_UNSUPPORTED, "distribution regression: groups take fewer than 2^31 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k)
      return fail(OB_E_INSUFFICIENT, "%sdistribution regression: a group's rows (%lld) must exceed the design columns (%d)",
                  error_prefix(OB_E_INSUFFICIENT), (long long)n, k);
  return OB_OK;
}

// The thresholds of a count: ob::rif's interpolated order statistic of the sorted pooled outcome at evenly spaced
// levels, exact duplicates removed.
static int dr_count_thresholds(std::vector<double> s, int T, double lo, double hi, std::vector<double>& out) {
  std::sort(s.begin(), s.end());
  const double nf = (double)s.size();
  out.clear();
  for (int i = 0; i < T; ++i) {
    const double level = lo + (hi - lo) * (double)i / (double)(T - 1);
    const double h = (nf - 1.0) * level, hf = std::floor(h), hc = std::ceil(h), frac = h - hf;
    const double q = (hf == hc) ? s[(int64_t)hf] : s[(int64_t)hf] + frac * (s[(int64_t)hc] - s[(int64_t)hf]);
    if (out.empty() || q != out.back()) out.push_back(q);
  }
  return OB_OK;
}

// The checks of an ob_dr_config that need no data.
static int dr_config_check(const ob_dr_config* dr) {
  if (!dr) return fail(OB_E_INVALID, "null pointer: ob_dr_config");
  if (dr->n_thresholds > kDrMaxT)
    return fail(OB_E_UNSUPPORTED, "distribution regression: at most %d thresholds, got %d", kDrMaxT, dr->n_thresholds);
  if (dr->n_quantiles > kDrMaxQ)
    return fail(OB_E_UNSUPPORTED, "distribution regression: at most %d quantiles, got %d", kDrMaxQ, dr->n_quantiles);
  if (dr->n_thresholds < 2) return fail(OB_E_INVALID, "distribution regression: at least two thresholds, got %d", dr->n_thresholds);
  if (dr->n_quantiles < 1 || !dr->quantiles)
    return fail(OB_E_INVALID, "distribution regression: at least one quantile, got %d", dr->n_quantiles);
  for (int32_t i = 0; i < dr->n_quantiles; ++i)
    if (!(dr->quantiles[i] > 0.0 && dr->quantiles[i] < 1.0))
      return fail(OB_E_INVALID, "distribution regression: quantile %d (%g) lies outside (0, 1)", i, dr->quantiles[i]);
  if (dr->thresholds) {
    for (int32_t t = 0; t < dr->n_thresholds; ++t)
      if (!std::isfinite(dr->thresholds[t]) || (t > 0 && !(dr->thresholds[t] > dr->thresholds[t - 1])))
        return fail(OB_E_INVALID, "distribution regression: thresholds must be finite and strictly increasing (entry %d)", t);
  } else if (!(dr->lo >= 0.0 && dr->hi <= 1.0 && dr->lo < dr->hi)) {
    return fail(OB_E_INVALID, "distribution regression: the threshold levels need 0 <= lo < hi <= 1, got [%g, %g]", dr->lo,
                dr->hi);
  }
  return OB_OK;
}

// Device side of a prepared run. The handle's ob_panel (no predictors, the outcome alone) is the resampler:
// engine_counts draws a segment's count images for its row counts, and its chunk table is the one the passes walk.
struct DrState {
  int k = 0, T = 0, nq = 0;
  DevBuf cols[2];  // [y | x_1 .. x_{k-1} | w] x ld
  DevBuf chunks, thr, taus, beta, flags, passes, partial, fpart;
  int n_chunks = 0;
};

static DrState* dr_state(const ob_prepared* pr) { return model_state<DrState>(pr, kModelDr); }

static DrArgs dr_args(const ob_prepared* pr, const DrState* st) {
  const ob_panel* p = pr->panel;
  DrArgs h{};
  for (int g = 0; g < 2; ++g) {
    h.cols[g] = st->cols[g].d();
    h.ld[g] = p->ld[g];
    h.n[g] = p->n[g];
  }
  h.tiles0 = p->ntiles[0];
  h.k = st->k;
  h.T = st->T;
  h.nq = st->nq;
  h.m = 2 * st->T;
  h.chunks = st->chunks.as<uint32_t>();
  h.n_chunks = st->n_chunks;
  h.thr = st->thr.d();
  h.taus = st->taus.d();
  h.row_len = pr->row_len;
  h.tol = 1e-6;
  return h;
}

static size_t dr_rep_bytes(const DrState* st) {  // chunk partials of one replicate
  return (size_t)st->n_chunks * ((size_t)st->T * dr_nv(st->k) + 2 * st->T + 1) * sizeof(double);
}

// Replicates per batch (boot_batch_reps), below 64 where one replicate's partials are that large (the kernels take
// any batch through img0), and at most the grid's z extent.
static uint32_t dr_batch_reps(const DrState* st, uint32_t rep_pad) {
  return std::min(boot_batch_reps(dr_rep_bytes(st), rep_pad, true), kDrMaxBatch);
}

static int dr_ensure(DrState* st, uint32_t hb) {
  const size_t fits = (size_t)hb * 2 * st->T;
  OB_HIP(st->beta.alloc(sizeof(double) * fits * st->k));
  OB_HIP(st->flags.alloc(sizeof(uint32_t) * (fits + 1)));
  OB_HIP(st->passes.alloc(sizeof(uint32_t) * fits));
  OB_HIP(st->partial.alloc(sizeof(double) * (size_t)st->n_chunks * hb * st->T * dr_nv(st->k)));
  OB_HIP(st->fpart.alloc(sizeof(double) * (size_t)st->n_chunks * hb * (2 * st->T + 1)));
  return OB_OK;
}

static void dr_bind(DrArgs& h, const DrState* st, uint32_t hb) {
  h.part_pad = hb;
  h.beta = st->beta.d();
  h.flags = st->flags.as<uint32_t>();
  h.active = h.flags + (size_t)hb * 2 * st->T;
  h.passes = st->passes.as<uint32_t>();
  h.partial = st->partial.d();
  h.fpart = st->fpart.d();
}

static int dr_point(ob_prepared* pr, DrState* st) {
  ob_panel* p = pr->panel;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = p->ctx->stream;
  OB_TRY(dr_ensure(st, 1));
  DevBuf d_row, d_ok;
  OB_HIP(d_row.alloc(sizeof(double) * pr->row_len));
  OB_HIP(d_ok.alloc(1));
  DrArgs h = dr_args(pr, st);
  dr_bind(h, st, 1);
  h.counts = nullptr;
  h.nb_rep = 1;
  h.n_reps = 1;
  h.rows = d_row.d();
  h.ok = d_ok.as<uint8_t>();
  OB_TRY(dr_batch(h, s));
  uint8_t okh = 0;
  const size_t fits = (size_t)2 * st->T;
  std::vector<double> row((size_t)pr->row_len), beta(fits * st->k);
  std::vector<uint32_t> passes(fits);
  OB_HIP(hipMemcpyAsync(row.data(), d_row.p, sizeof(double) * row.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(&okh, d_ok.p, 1, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(beta.data(), st->beta.p, sizeof(double) * beta.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(passes.data(), st->passes.p, sizeof(uint32_t) * fits, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  if (!okh) return fail(OB_E_LINALG, kDrFitFailed, error_prefix(OB_E_LINALG));
  pr->point_row = row;
  DrInfo& info = pr->dr_info;
  info.beta = beta;
  info.passes.assign(passes.begin(), passes.end());
  // the edge cases of the point estimate, from the row's own F values
  const int T = st->T, nq = st->nq;
  info.edge.assign((size_t)3 * nq, 0);
  info.n_out_of_range = 0;
  std::vector<double> q((size_t)nq);
  const double* fr = row.data() + 6 * nq + 3 * T;
  for (int f = 0; f < 3; ++f)
    info.n_out_of_range +=
        dr_quantiles(fr + (size_t)f * T, info.thresholds.data(), T, info.taus.data(), nq, q.data(), nullptr, info.edge.data() + (size_t)f * nq);
  return OB_OK;
}

static int dr_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                          hipStream_t stream) {
  DrState* st = dr_state(pr);
  uint32_t hb = 0;
  const BootPlan plan{kFitSegReps, kCountBudget, true, [&](uint32_t seg_pad) {
                        g_timing = {};
                        hb = dr_batch_reps(st, seg_pad);
                        return dr_ensure(st, hb);
                      }};
  return boot_segmented(pr, kModelDr, plan, first_rep, n_reps, d_rows && d_ok, stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t nb_rep, uint32_t, hipStream_t s) {
    return boot_batches(ns, hb, [&](uint32_t b0, uint32_t nb) {
      DrArgs h = dr_args(pr, st);
      dr_bind(h, st, hb);
      h.counts = pr->panel->d_counts;
      h.nb_rep = nb_rep;
      h.img0 = b0;
      h.n_reps = nb;
      h.rows = d_rows + (s0 + b0) * pr->row_len;
      h.ok = d_ok + s0 + b0;
      return dr_batch(h, s);
    });
  });
}

// installs the builder's hooks when the library loads (ob_model.hpp)
static const bool g_dr_hooks_installed =
    model_install(kModelDr, {dr_boot_device, model_boot_host, [](void* s) { delete static_cast<DrState*>(s); }});

// Every check of the frame entry points, before any device work and before the context is read: the thresholds
// and quantiles, settings outside the scope, nulls and non-finite values in named columns, the design
// (ob::data_matrices), the shape. On success m holds the design matrices and the groups' weights.
static int dr_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                    const ob_dr_config* dr, Config& c, Matrices& m) {
  OB_TRY(config_from(cfg, c));
  if (!c.normalize.empty()) return model_refuse(kModelDr, "normalized categoricals are");
  if (c.has_selection || !c.selection_predictors.empty()) return model_refuse(kModelDr, "Heckman selection settings are");
  if (c.has_cluster) return model_refuse(kModelDr, "the cluster bootstrap is");
  OB_TRY(dr_config_check(dr));
  OB_TRY(stage_named(cols, n_cols, n_rows, c, kModelDr, true, true));
  OB_TRY(m.load(cols, n_cols, n_rows, cfg, true));
  if (m.k > kDrMaxK) OB_TRY(dr_check_shape(m.k, m.n[0], m.n[1], dr->n_thresholds, dr->n_quantiles));
  if (m.n[0] == 0 || m.n[1] == 0) return fail(OB_E_GROUP, "%sOne group has no data", error_prefix(OB_E_GROUP));
  return dr_check_shape(m.k, m.n[0], m.n[1], dr->n_thresholds, dr->n_quantiles);
}

static int dr_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_dr_config* dr, ob_prepared** out) {
  Config c;
  Matrices m;
  OB_TRY(dr_stage(cols, n_cols, n_rows, cfg, dr, c, m));
  const int k = m.k;
  std::vector<double> thr;
  if (dr->thresholds) {
    thr.assign(dr->thresholds, dr->thresholds + dr->n_thresholds);
  } else {
    std::vector<double> pooled(m.y[0], m.y[0] + m.n[0]);
    pooled.insert(pooled.end(), m.y[1], m.y[1] + m.n[1]);
    OB_TRY(dr_count_thresholds(std::move(pooled), dr->n_thresholds, dr->lo, dr->hi, thr));
    if (thr.size() < 2)
      return fail(OB_E_INVALID, "distribution regression: fewer than two distinct thresholds are left of %d", dr->n_thresholds);
  }
  const int T = (int)thr.size(), nq = dr->n_quantiles;
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  DrState* st = new DrState();
  st->k = k;
  st->T = T;
  st->nq = nq;
  ob_prepared* pr = model_handle(ctx, c, m, kModelDr, st, dr_row_len(T, nq), 1);
  pr->dr_info.thresholds = thr;
  pr->dr_info.taus.assign(dr->quantiles, dr->quantiles + nq);
  pr->dr_info.n_requested = dr->n_thresholds;
  auto build = [&]() -> int {
    OB_TRY(outcome_panel(ctx, m, &pr->panel));
    ob_panel* p = pr->panel;
    for (int g = 0; g < 2; ++g) {  // [y | x_1 .. | w] x ld
      OB_TRY(upload_group(st->cols[g], p->ld[g], m.n[g], k, 1, m.y[g], m.x[g]));
      OB_TRY(upload_weights(st->cols[g], p->ld[g], m.n[g], k, m.w(g)));
    }
    OB_TRY(upload_chunks(p, st->chunks, &st->n_chunks));
    OB_HIP(st->thr.alloc(sizeof(double) * T));
    OB_HIP(hipMemcpy(st->thr.p, thr.data(), sizeof(double) * T, hipMemcpyHostToDevice));
    OB_HIP(st->taus.alloc(sizeof(double) * nq));
    OB_HIP(hipMemcpy(st->taus.p, dr->quantiles, sizeof(double) * nq, hipMemcpyHostToDevice));
    g_timing = {};
    return dr_point(pr, st);
  };
  return model_built(pr, build(), out);
}

// The array pieces: one launch of a pass kernel over one group of n rows (x: n x k column-major with ld ldx, column
// 0 the intercept) counted as `counts` does, with the chunk partials added in chunk order as the step and row
// kernels add them. cdf = false: the logit pass of T thresholds, sums [T][dr_nv(k)]; cdf = true: the distribution
// pass of m vectors, sums [m + 1].
static int dr_piece(ob_ctx* ctx, bool cdf, int k, const double* x, int64_t ldx, const double* y, const double* w,
                    const uint8_t* counts, int64_t n64, const double* thr, int T, const double* betas, int m,
                    std::vector<double>& sums) {
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint32_t n = (uint32_t)n64, tiles = (n + OB_TILE_ROWS - 1) / OB_TILE_ROWS;
  const int64_t ld = (int64_t)tiles * OB_TILE_ROWS;
  std::vector<uint32_t> chunks;
  group_chunks(0u, tiles, 64u, chunks);
  const int n_chunks = (int)(chunks.size() / 3), nv = dr_nv(k);
  const int n_vec = cdf ? m : T;
  const size_t per = cdf ? (size_t)m + 1 : (size_t)T * nv;
  DevBuf d_cols, d_chunks, d_beta, d_flags, d_partial, d_counts, d_thr;
  const size_t bytes = sizeof(double) * (size_t)ld * (k + 1);
  OB_HIP(d_cols.alloc(bytes));
  OB_HIP(hipMemsetAsync(d_cols.p, 0, bytes, s));
  if (y) OB_HIP(hipMemcpyAsync(d_cols.p, y, sizeof(double) * n, hipMemcpyHostToDevice, s));
  for (int j = 1; j < k; ++j)
    OB_HIP(hipMemcpyAsync(d_cols.d() + (size_t)j * ld, x + (size_t)j * ldx, sizeof(double) * n, hipMemcpyHostToDevice, s));
  const std::vector<double> unit(w ? 0 : (size_t)n, 1.0);
  OB_HIP(hipMemcpyAsync(d_cols.d() + (size_t)k * ld, w ? w : unit.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
  OB_HIP(d_chunks.alloc(sizeof(uint32_t) * chunks.size()));
  OB_HIP(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(uint32_t) * chunks.size(), hipMemcpyHostToDevice, s));
  // the logit pass reads the fits of group 0 at [0][T][k]; the distribution pass reads [m][k]
  const size_t nbeta = (size_t)std::max(n_vec, 2 * T) * k;
  OB_HIP(d_beta.alloc(sizeof(double) * nbeta));
  OB_HIP(hipMemsetAsync(d_beta.p, 0, sizeof(double) * nbeta, s));
  OB_HIP(hipMemcpyAsync(d_beta.p, betas, sizeof(double) * (size_t)n_vec * k, hipMemcpyHostToDevice, s));
  OB_HIP(d_flags.alloc(sizeof(uint32_t) * 2 * kDMaxT));
  OB_HIP(hipMemsetAsync(d_flags.p, 0, sizeof(uint32_t) * 2 * kDMaxT, s));
  OB_HIP(d_partial.alloc(sizeof(double) * (size_t)n_chunks * per));
  OB_HIP(hipMemsetAsync(d_partial.p, 0, sizeof(double) * (size_t)n_chunks * per, s));
  OB_HIP(d_thr.alloc(sizeof(double) * kDMaxT));
  if (thr) OB_HIP(hipMemcpyAsync(d_thr.p, thr, sizeof(double) * T, hipMemcpyHostToDevice, s));
  std::vector<uint32_t> img;  // one 64-replicate block of the f64 Gram's count images (ob_engine.hpp), slot 0
  if (counts) {
    img.assign((size_t)tiles * 4 * kCimgWords, 0u);
    pack_count_images(counts, n, n, 1, 1, img.data(), nullptr, 0);
    OB_HIP(d_counts.alloc(sizeof(uint32_t) * img.size()));
    OB_HIP(hipMemcpyAsync(d_counts.p, img.data(), sizeof(uint32_t) * img.size(), hipMemcpyHostToDevice, s));
  }
  DrArgs h{};
  h.cols[0] = d_cols.d();
  h.cols[1] = d_cols.d();
  h.ld[0] = ld;
  h.n[0] = n;
  h.tiles0 = tiles;
  h.k = k;
  h.T = T;
  h.m = m;
  h.counts = counts ? d_counts.as<uint32_t>() : nullptr;
  h.nb_rep = 1;
  h.chunks = d_chunks.as<uint32_t>();
  h.n_chunks = n_chunks;
  h.n_reps = 1;
  h.part_pad = 1;
  h.thr = d_thr.d();
  h.beta = d_beta.d();
  h.flags = d_flags.as<uint32_t>();
  h.partial = d_partial.d();
  h.fpart = d_partial.d();
  OB_HIP(cdf ? launch_cdf(h, s) : launch_pass(h, s));
  std::vector<double> part((size_t)n_chunks * per);
  OB_HIP(hipMemcpyAsync(part.data(), d_partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  sums.assign(per, 0.0);
  for (int c = 0; c < n_chunks; ++c)  // chunk order, as the step and row kernels
    for (size_t e = 0; e < per; ++e) sums[e] += part[(size_t)c * per + e];
  return OB_OK;
}

// The argument checks the two array pieces share (before any device work).
static int dr_piece_check(const char* what, const double* x, int64_t ldx, int64_t n, int32_t k, const double* betas,
                          int32_t n_vec, int32_t max_vec, const void* out0, const void* out1) {
  if (!x || !betas || !out0 || !out1) return fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || k < 1) return fail(OB_E_INVALID, "%s needs n > 0 rows and k >= 1 columns, got n = %lld, k = %d", what, (long long)n, k);
  if (k > kDrMaxK) return fail(OB_E_UNSUPPORTED, "%s takes at most %d columns, got %d", what, kDrMaxK, k);
  if (n_vec > max_vec) return fail(OB_E_UNSUPPORTED, "%s takes at most %d coefficient vectors, got %d", what, max_vec, n_vec);
  if (n_vec < 1) return fail(OB_E_INVALID, "%s takes at least one coefficient vector, got %d", what, n_vec);
  if (ldx < n) return fail(OB_E_INVALID, "%s: ldx = %lld is below n = %lld", what, (long long)ldx, (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(OB_E_UNSUPPORTED, "%s takes fewer than 2^31 rows", what);
  for (int64_t i = 0; i < n; ++i)  // the pass takes x_0 = 1 as given
    if (x[i] != 1.0) return fail(OB_E_UNSUPPORTED, "%s: column 0 of x must be the intercept (all ones)", what);
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_dr_row_len(int32_t n_thresholds, int32_t n_quantiles) {
  return n_thresholds < 2 || n_quantiles < 1 ? 0 : ob::dr_row_len(n_thresholds, n_quantiles);
}

int ob_dr_check_shape(int32_t k, int64_t n_a, int64_t n_b, int32_t n_thresholds, int32_t n_quantiles) {
  return ob::dr_check_shape(k, n_a, n_b, n_thresholds, n_quantiles);
}

int ob_dr_last_timing(ob_dr_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

int ob_dr_thresholds(const double* y, int64_t n, int32_t n_thresholds, double lo, double hi, double* out, int32_t* n_kept) {
  if (!y || !out || !n_kept) return ob::fail(OB_E_INVALID, "null pointer");
  if (n_thresholds > OB_DR_MAX_T)
    return ob::fail(OB_E_UNSUPPORTED, "distribution regression: at most %d thresholds, got %d", OB_DR_MAX_T, n_thresholds);
  if (n_thresholds < 2 || n < 1) return ob::fail(OB_E_INVALID, "ob_dr_thresholds needs n >= 1 and at least two thresholds");
  if (!(lo >= 0.0 && hi <= 1.0 && lo < hi))
    return ob::fail(OB_E_INVALID, "distribution regression: the threshold levels need 0 <= lo < hi <= 1, got [%g, %g]", lo, hi);
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(y[i])) return ob::fail(OB_E_INVALID, "ob_dr_thresholds: y has a non-finite value in row %lld", (long long)i);
  std::vector<double> thr;
  OB_TRY(ob::dr_count_thresholds(std::vector<double>(y, y + n), n_thresholds, lo, hi, thr));
  std::copy(thr.begin(), thr.end(), out);
  *n_kept = (int32_t)thr.size();
  return OB_OK;
}

int ob_builder_prepare_dr(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                          const ob_dr_config* dr, ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::dr_prepare(ctx, cols, n_cols, n_rows, cfg, dr, out);
}

int ob_builder_run_dr(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_dr_config* dr, ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::dr_prepare(ctx, cols, n_cols, n_rows, cfg, dr, &pr));
  const uint64_t reps = pr->cfg.reps;
  std::vector<double> rows((size_t)reps * pr->row_len);
  std::vector<uint8_t> ok(reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::finish(pr, 0, rows.data(), ok.data(), reps, out);
  ob_prepared_destroy(pr);
  return rc;
}

int ob_prepared_dr_info(const ob_prepared* prep, ob_dr_info* out) {
  if (!prep || !out) return ob::fail(OB_E_INVALID, "null pointer");
  if (prep->model_kind != ob::kModelDr) return ob::fail(OB_E_INVALID, "not a handle of a distribution-regression decomposition");
  const ob::DrInfo& i = prep->dr_info;
  out->n_thresholds = (int32_t)i.thresholds.size();
  out->n_quantiles = (int32_t)i.taus.size();
  out->k = prep->k;
  out->n_requested = i.n_requested;
  out->n_out_of_range = i.n_out_of_range;
  out->thresholds = i.thresholds.data();
  out->quantiles = i.taus.data();
  out->beta = i.beta.data();
  out->passes = i.passes.data();
  out->out_of_range = i.edge.data();
  return OB_OK;
}

int ob_dr_logit_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                     int64_t n, int32_t k, const double* thresholds, int32_t n_thresholds, const double* betas, double* info,
                     double* grad) {
  if (!y || !thresholds) return ob::fail(OB_E_INVALID, "null pointer");
  OB_TRY(ob::dr_piece_check("ob_dr_logit_pass", x, ldx, n, k, betas, n_thresholds, OB_DR_MAX_T, info, grad));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  std::vector<double> sums;
  OB_TRY(ob::dr_piece(ctx, false, k, x, ldx, y, w, counts, n, thresholds, n_thresholds, betas, 0, sums));
  const int NH = k * (k + 1) / 2, nv = NH + k;
  for (int r = 0; r < n_thresholds; ++r) {
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

int ob_dr_cdf(ob_ctx* ctx, const double* x, int64_t ldx, const double* w, const uint8_t* counts, int64_t n, int32_t k,
              const double* betas, int32_t m, double* sums, double* wsum) {
  OB_TRY(ob::dr_piece_check("ob_dr_cdf", x, ldx, n, k, betas, m, OB_DR_MAX_VECTORS, sums, wsum));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  std::vector<double> s;
  OB_TRY(ob::dr_piece(ctx, true, k, x, ldx, nullptr, w, counts, n, nullptr, 2, betas, m, s));
  std::copy(s.begin(), s.begin() + m, sums);
  *wsum = s[m];
  return OB_OK;
}

}  // extern "C"
