// ob_tobit.hip -- the bootstrapped Tobit decomposition of a censored outcome (Bauer and Sinning 2008, 2010; DESIGN.md
// §5.24). No counterpart in the reference crate.
//
// Per group the censored-normal model y = max(lower, min(upper, x'beta + sigma eps)) is fitted in Olsen's parameters
// eta = [delta; theta], delta = beta / sigma, theta = 1 / sigma, in which the log-likelihood is concave. With
// v = [x; -y] and u = theta y - x'delta = -v'eta a row's score is s v and its share of -H is h v v' (s, h by the row's
// censoring class), so a Newton pass is ob_rw_kernel's logit pass at dimension K + 1, with one scalar more:
// N_unc = sum c w over the uncensored rows, whose terms N_unc / theta and N_unc / theta^2 the step adds.
//
// Per batch of replicates (the resample enters through the engine's level-2 count images, as in ob_reweight.hip):
//   ob_tobit_kernel        block per (row chunk, 16 replicates): sum c w h v v' and sum c w s v of one pass as (weight
//                          row) x (pair products) on v_mfma_f64_16x16x4_f64; u, the class, s and h are formed inside
//                          the tile, never stored in HBM;
//   ob_tobit_step_kernel   wave per (replicate, group): chunk partials in chunk order, the N_unc terms, Cholesky, the
//                          step, the guard on theta, the stopping rule, the done / failed bits and the pass count;
//   ob_tobit_means_kernel  block per (row chunk, 16 replicates): sum c w m(x'beta_h, sigma_h) for h = A, B, sum c w y,
//                          sum c w, the censored sums and sum c w x_j;
//   ob_tobit_row_kernel    wave per replicate: chunk partials in chunk order, the terms, the row and ok.
// The point pass is the same code with every row counted once (counts == NULL).
//
// Panel of a Tobit run, per group [col][ld]: y | x_1 .. x_{K-1} | w (ones without sample weights).
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
#include "ob_linalg.hpp"
#include "ob_model.hpp"
#include "ob_normal.hpp"
#include "ob_options.hpp"
#include "ob_pairpass.hpp"
#include "ob_spec.h"
#include "ob_tobit.hpp"

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;
constexpr int kTB = 256;     // threads of a pass or means block
constexpr int kTS = 65;      // doubles per staged column (as ob_rw_kernel)
constexpr int kTReps = 16;   // replicates per block
constexpr int kTMaxU = 9;    // column tiles per wave: 35 tiles at K = 31 (528 pairs and 32 gradient columns)
constexpr int kTMaxD = ob::kTobitMaxK + 1;  // the dimension of eta
constexpr uint32_t kTbDone = 1u, kTbFailed = 2u;  // OB_TOBIT_DONE, OB_TOBIT_FAILED
constexpr int kTbMaxPasses = 100;  // OB_TOBIT_MAX_PASSES
constexpr int kTbMaxHalvings = 30;
constexpr int kTVals = 40;   // per-thread sums of the means pass, padded to whole rounds of kTRound
constexpr int kTRound = 8;

struct TbArgs {
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
  double* eta;             // [group][part_pad][k + 1]
  uint32_t* flags;         // [group][part_pad] kTbDone | kTbFailed
  uint32_t* passes;        // [group][part_pad] Newton passes taken
  uint32_t* active;        // fits still iterating after a step
  double* partial;         // [chunk][part_pad][tb_nv(k)] of a pass / [..][tb_mv(k)] of the means
  double* rows;
  uint8_t* ok;
  int row_len, ref;
  double tol, lower, upper;
  int has_lower, has_upper;
};

// Values per (chunk, replicate) of a pass: the packed lower triangle (entry j (j + 1) / 2 + i, i <= j) of
// sum c w h v v' over v = [x_0 .. x_{k-1}, -y], the k + 1 entries of sum c w s v, N_unc = sum c w and the count sum
// sum c over the uncensored rows.
__host__ __device__ inline int tb_nv(int k) { return (k + 1) * (k + 2) / 2 + (k + 1) + 2; }
// Of the means pass: sum c w m under A's and B's parameters, sum c w y, sum c w, the left and right censored
// sum c w, sum c w x_j for 1 <= j < k.
__host__ __device__ inline int tb_mv(int k) { return 5 + k; }

__device__ __forceinline__ double tb_lambda(double z) {
  return ob::tobit_lambda_with(z, [](double v) { return nd_rcp(v); });
}

// 0 uncensored, 1 at the lower limit, 2 at the upper limit.
__device__ __forceinline__ int tb_class(double y, const TbArgs& a) {
  if (a.has_lower && y == a.lower) return 1;
  if (a.has_upper && y == a.upper) return 2;
  return 0;
}

inline size_t tb_lds(int k) {
  return sizeof(double) * ((size_t)(k + 2) * kTS + 2 * 64 * kTReps + (size_t)kTReps * ((k + 1) | 1) + 2 * 16 * kTReps);
}

// Block = (row chunk, 16 replicates), 4 waves: the layout of ob_rw_kernel. Per 64-row sub-tile:
//   stage  the k + 1 columns of the sub-tile -> LDS [col][65] (+ a column of ones for x_0);
//   A      thread = (replicate t & 15, rows 4 (t >> 4) .. + 3: one count word): x'delta from the staged columns and
//          the replicate's eta (LDS [16][(k + 1) | 1]), u, the class, h and s -> LDS [operand][row][16];
//   B      wave w owns the column tiles w, w + 4, ..; a tile's B value is the product of two staged columns. The
//          sign of v's last entry (-y) is applied once, to the accumulator, when the partial is written.
// A wave owns its tiles over the whole chunk, so every partial is one accumulator element summed over the chunk's
// rows in row order; the two scalars are summed per thread and then over the 16 row groups in order. A replicate's
// partials do not depend on its slot in the block, on its neighbours, on the batch or on first_rep. No atomics.
__global__ __launch_bounds__(kTB, 2) void ob_tobit_kernel(const TbArgs a) {
  extern __shared__ __attribute__((aligned(16))) double tsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const int k = a.k, D = k + 1, gs = D | 1, ncol = k + 1;
  const int ones = ncol * kTS, wcol = k * kTS;
  double* stg = tsm;                    // [ncol + 1][kTS]: y, x_1 .. x_{k-1}, w, ones
  double* wl = stg + (ncol + 1) * kTS;  // [2][64 rows][16 replicates]
  double* et = wl + 2 * 64 * kTReps;    // [16][gs] eta
  double* red = et + kTReps * gs;       // [2][16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep0 = blockIdx.y * kTReps, rep = rep0 + r16;
  const size_t fit0 = (size_t)g * a.part_pad;
  bool act = rep < a.n_reps;
  if (act) act = !(a.flags[fit0 + rep] & kTbDone);
  if (!__syncthreads_or(act)) return;
  for (int i = tid; i < kTReps * D; i += kTB) {
    const int rr = i / D, j = i - rr * D;
    et[rr * gs + j] = rep0 + rr < a.n_reps ? a.eta[(fit0 + rep0 + rr) * D + j] : 0.0;
  }
  if (tid < 64) stg[ones + tid] = 1.0;
  // this lane's column of each of the wave's tiles: the two staged columns whose product is the B value, packed into
  // one word (the low and the high half) so that the tile loop keeps one register a tile. v_j: x_0 = ones,
  // x_j = column j, y = column 0.
  const int NP = D * (D + 1) / 2;
  const int nt0 = (NP + 15) / 16;  // tiles of operand 0: the pair products
  const int nt1 = (D + 15) / 16;   // tiles of operand 1: the gradient's columns
  const int NT = nt0 + nt1;
  auto vcol = [&](int j) { return j == 0 ? ones : (j < k ? j * kTS : 0); };
  uint32_t ops[kTMaxU];
#pragma unroll
  for (int u = 0; u < kTMaxU; ++u) {
    const int c = wave + 4 * u, e16 = lane & 15;
    int o0 = ones, o1 = ones;
    if (c < nt0) {
      const int idx = 16 * c + e16;
      if (idx < NP) {
        const int j = tri_row(idx), i = idx - j * (j + 1) / 2;
        o0 = vcol(j);
        o1 = vcol(i);
      }
    } else if (c < NT) {
      const int idx = 16 * (c - nt0) + e16;
      if (idx < D) o0 = vcol(idx);
    }
    ops[u] = (uint32_t)o0 | ((uint32_t)o1 << 16);
  }
  d4 acc[kTMaxU];
#pragma unroll
  for (int u = 0; u < kTMaxU; ++u) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
  double nunc = 0.0, cunc = 0.0;  // sum c w and sum c over this thread's uncensored rows
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const uint32_t rb = rep >> 6, R = rep & 63;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's operand reads (and the eta loads)
      for (int i = tid; i < ncol * 64; i += kTB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kTS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      uint32_t word = 0;  // counts of rows 4 q .. 4 q + 3 (the f64 Gram's count-image layout, ob_engine.hpp)
      if (act) {
        const size_t tt = (g ? a.tiles0 : 0u) + tile;
        word = a.counts ? a.counts[((tt * a.nb_rep + rb) * 4 + sw) * kCimgWords + R * kCimgStride + q] : 0x01010101u;
      }
      double lin[4] = {0.0, 0.0, 0.0, 0.0};
      if (word) {
        const double d0 = et[r16 * gs];
#pragma unroll
        for (int i = 0; i < 4; ++i) lin[i] = d0;
        for (int j = 1; j < k; ++j) {
          const double dj = et[r16 * gs + j];
          const double* xj = stg + j * kTS + 4 * q;
#pragma unroll
          for (int i = 0; i < 4; ++i) lin[i] += xj[i] * dj;
        }
      }
      const double theta = et[r16 * gs + k];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t row = 4 * q + i;
        const uint32_t cu = row < nr ? (word >> (8 * i)) & 255u : 0u;
        double w0 = 0.0, w1 = 0.0;
        if (cu) {
          const double c = (double)cu, y = stg[row], cw = c * stg[wcol + row];
          const double u = theta * y - lin[i];
          const int cls = tb_class(y, a);
          if (cls == 0) {
            w0 = cw;
            w1 = cw * u;
            nunc += cw;
            cunc += c;
          } else {  // one evaluation of lambda serves both limits: at z = u on the left, at z = -u on the right
            const double z = cls == 1 ? u : -u, lam = tb_lambda(z);
            w0 = cw * (lam * (lam + z));
            w1 = cw * (cls == 1 ? -lam : lam);
          }
        }
        wl[row * kTReps + r16] = w0;
        wl[64 * kTReps + row * kTReps + r16] = w1;
      }
      __syncthreads();
      const int rl = lane >> 4;
#pragma unroll 2
      for (int i = 0; i < 16; ++i) {
        const double a0 = wl[i * 64 + lane], a1 = wl[64 * kTReps + i * 64 + lane];
        const int row = 4 * i + rl;
#pragma unroll
        for (int u = 0; u < kTMaxU; ++u)
          if (wave + 4 * u < NT)
            acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(wave + 4 * u < nt0 ? a0 : a1,
                                                          stg[(ops[u] & 0xFFFFu) + row] * stg[(ops[u] >> 16) + row], acc[u], 0, 0, 0);
      }
    }
  }
  // lane (rl, e16), element r of acc[u]: replicate rep0 + rl + 4 r, the tile's column e16. The slot of the partial
  // (none: padding) and the sign of -y are worked out here, once, and not kept over the chunk.
  const int nv = tb_nv(k);
  double* out = a.partial + (size_t)chunk * a.part_pad * nv;
#pragma unroll
  for (int u = 0; u < kTMaxU; ++u) {
    const int c = wave + 4 * u, e16 = lane & 15;
    if (c >= NT) continue;
    int dst = -1;
    bool neg = false;
    if (c < nt0) {
      const int idx = 16 * c + e16;
      if (idx < NP) {
        const int j = tri_row(idx), i = idx - j * (j + 1) / 2;
        dst = idx;
        neg = (j == k) != (i == k);
      }
    } else {
      const int idx = 16 * (c - nt0) + e16;
      if (idx < D) {
        dst = NP + idx;
        neg = idx == k;
      }
    }
    if (dst < 0) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t rp = rep0 + (lane >> 4) + 4 * r;
      if (rp < a.n_reps) out[(size_t)rp * nv + dst] = neg ? -acc[u][r] : acc[u][r];
    }
  }
  __syncthreads();
  red[q * kTReps + r16] = nunc;
  red[16 * kTReps + q * kTReps + r16] = cunc;
  __syncthreads();
  if (tid < 2 * kTReps) {
    const int which = tid >> 4;
    double v = 0.0;
    for (int qq = 0; qq < 16; ++qq) v += red[which * 16 * kTReps + qq * kTReps + r16];
    if (rep < a.n_reps) out[(size_t)rep * nv + NP + D + which] = v;
  }
}

// Every fit of the batch to its group's start, not done, no pass taken. start [2][k + 1].
__global__ __launch_bounds__(64) void ob_tobit_init_kernel(const TbArgs a, const double* start, int n_groups) {
  const uint32_t rep = blockIdx.x * 64 + threadIdx.x;
  if (rep >= a.n_reps) return;
  const int D = a.k + 1;
  for (int g = 0; g < n_groups; ++g) {
    const size_t fit = (size_t)g * a.part_pad + rep;
    for (int j = 0; j < D; ++j) a.eta[fit * D + j] = start[g * D + j];
    a.flags[fit] = 0u;
    a.passes[fit] = 0u;
  }
}

// One wave per (replicate, group), after a pass: the group's chunk partials in chunk order, the N_unc terms, the
// Cholesky factor of -H, the step. A fit whose resample holds an uncensored count sum of at most K is dropped before
// its first step (the counterpart of InsufficientData): failed, eta at its start, no pass counted. The guard: while
// theta + d theta <= 0 the whole step is halved, at most kTbMaxHalvings times; a step that stays outside, or that is
// not finite, fails the fit and is not taken. The stopping rule is ob_rw_step_kernel's on the step taken. A fit that
// has converged keeps its eta and its pass count while the batch runs on.
__global__ __launch_bounds__(64) void ob_tobit_step_kernel(const TbArgs a) {
  __shared__ double m[kTMaxD * kTMaxD], step[kTMaxD + 2];
  const int lane = threadIdx.x, k = a.k, D = k + 1;
  const uint32_t rep = blockIdx.x, g = blockIdx.y;
  const size_t fit = (size_t)g * a.part_pad + rep;
  if (a.flags[fit] & kTbDone) return;
  gather_partials(a.partial, a.part_pad, rep, tb_nv(k), a.chunks, a.n_chunks, (int)g, D, lane, m, step);
  __syncthreads();
  const double nunc = step[D], cunc = step[D + 1];
  if (!(cunc > (double)k)) {
    if (lane == 0) a.flags[fit] = kTbDone | kTbFailed;
    return;
  }
  double* eta = a.eta + fit * D;
  const double theta = eta[k];
  if (lane == 0) {
    m[k + k * D] += nunc / (theta * theta);
    step[k] += nunc / theta;
  }
  __syncthreads();
  const bool chol = wave_cholesky(m, D, lane);
  __syncthreads();
  if (!chol) {
    if (lane == 0) {
      a.flags[fit] = kTbDone | kTbFailed;
      a.passes[fit] += 1;
    }
    return;
  }
  wave_chol_solve(m, D, step, lane);
  __syncthreads();
  if (lane == 0) {
    double scale = 1.0;
    int halvings = 0;
    while (theta + scale * step[k] <= 0.0 && halvings < kTbMaxHalvings) {
      scale *= 0.5;
      ++halvings;
    }
    double nrm = 0.0;
    for (int i = 0; i < D; ++i) {
      const double d = scale * step[i];
      nrm += d * d;
    }
    a.passes[fit] += 1;
    if (!(nrm < INFINITY) || !(theta + scale * step[k] > 0.0)) {  // (a NaN norm compares false)
      a.flags[fit] = kTbDone | kTbFailed;
      return;
    }
    for (int i = 0; i < D; ++i) eta[i] += scale * step[i];
    if (sqrt(nrm) < a.tol)
      a.flags[fit] = kTbDone;
    else
      atomicAdd(a.active, 1u);
  }
}

// E[y | x] of the censored normal at index xb and scale sg: a Phi(z_a) + b (1 - Phi(z_b)) + (Phi(z_b) - Phi(z_a)) xb
// + sg (phi(z_a) - phi(z_b)), the terms of an absent limit dropped. The upper tail is Phi(-z_b).
__device__ __forceinline__ double tb_mean(double xb, double sg, const TbArgs& a) {
  double Pa = 0.0, pa = 0.0, Qb = 0.0, pb = 0.0, t = 0.0;
  if (a.has_lower) {
    npdf_ncdf((a.lower - xb) / sg, pa, Pa);
    t += a.lower * Pa;
  }
  if (a.has_upper) {
    npdf_ncdf(-((a.upper - xb) / sg), pb, Qb);
    t += a.upper * Qb;
  }
  t += (1.0 - Pa - Qb) * xb;
  t += sg * (pa - pb);
  return t;
}

// Block = (row chunk, 16 replicates), 4 waves; thread = (replicate t & 15, rows 4 (t >> 4) .. + 3 of each 64-row
// sub-tile): ob_binary_means_kernel's layout. The two parameter vectors of a replicate are beta = delta / theta and
// sigma = 1 / theta of its two fits (LDS [replicate][vector][(k + 1) | 1], sigma last). A thread owns its rows over the
// whole chunk; at the end the 16 row groups of a replicate are added in row-group order through LDS. No atomics.
__global__ __launch_bounds__(kTB) void ob_tobit_means_kernel(const TbArgs a) {
  extern __shared__ __attribute__((aligned(16))) double msm[];
  const int tid = threadIdx.x;
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const int k = a.k, D = k + 1, gs = D | 1, nv = tb_mv(k), ncol = k + 1;
  double* stg = msm;                   // [k + 1][kTS]: y, x_1 .. x_{k-1}, w
  double* bt = stg + ncol * kTS;       // [16][2][gs]
  double* red = bt + kTReps * 2 * gs;  // [kTRound][16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep0 = blockIdx.y * kTReps, rep = rep0 + r16;
  const bool act = rep < a.n_reps;
  for (int i = tid; i < kTReps * 2 * D; i += kTB) {
    const int rr = i / (2 * D), rem = i - rr * 2 * D, v = rem / D, j = rem - v * D;
    double val = 0.0;
    if (rep0 + rr < a.n_reps) {
      const double* eta = a.eta + ((size_t)v * a.part_pad + rep0 + rr) * D;
      val = j < k ? eta[j] / eta[k] : 1.0 / eta[k];
    }
    bt[(rr * 2 + v) * gs + j] = val;
  }
  double acc[2] = {0.0, 0.0}, sy = 0.0, sc = 0.0, sl = 0.0, sr = 0.0;
  double xs[ob::kTobitMaxK - 1];
#pragma unroll
  for (int j = 0; j < ob::kTobitMaxK - 1; ++j) xs[j] = 0.0;
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const uint32_t rb = rep >> 6, R = rep & 63;
  const double* b0 = bt + (r16 * 2 + 0) * gs;
  const double* b1 = bt + (r16 * 2 + 1) * gs;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's reads (and the parameter loads)
      for (int i = tid; i < ncol * 64; i += kTB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kTS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      uint32_t word = 0;
      if (act) {
        const size_t tt = (g ? a.tiles0 : 0u) + tile;
        word = a.counts ? a.counts[((tt * a.nb_rep + rb) * 4 + sw) * kCimgWords + R * kCimgStride + q] : 0x01010101u;
      }
      double cd[4];  // c w
#pragma unroll
      for (int i = 0; i < 4; ++i)
        cd[i] = (uint32_t)(4 * q + i) < nr ? (double)((word >> (8 * i)) & 255u) * stg[k * kTS + 4 * q + i] : 0.0;
      if (word == 0) continue;  // (uniform control flow resumes at the barrier)
      double zg[2][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        zg[0][i] = b0[0];
        zg[1][i] = b1[0];
      }
#pragma unroll
      for (int j = 1; j < ob::kTobitMaxK; ++j)
        if (j < k) {
          const double* zj = stg + j * kTS + 4 * q;
          const double g0 = b0[j], g1 = b1[j];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double z = zj[i];
            zg[0][i] += z * g0;
            zg[1][i] += z * g1;
            xs[j - 1] += cd[i] * z;
          }
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if ((uint32_t)(4 * q + i) >= nr || ((word >> (8 * i)) & 255u) == 0u) continue;
        const double y = stg[4 * q + i];
        acc[0] += cd[i] * tb_mean(zg[0][i], b0[k], a);
        acc[1] += cd[i] * tb_mean(zg[1][i], b1[k], a);
        sy += cd[i] * y;
        sc += cd[i];
        const int cls = tb_class(y, a);
        if (cls == 1) sl += cd[i];
        if (cls == 2) sr += cd[i];
      }
    }
  }
  double vals[kTVals];
#pragma unroll
  for (int i = 0; i < kTVals; ++i) vals[i] = 0.0;
  vals[0] = acc[0];
  vals[1] = acc[1];
  vals[2] = sy;
  vals[3] = sc;
  vals[4] = sl;
  vals[5] = sr;
#pragma unroll
  for (int j = 1; j < ob::kTobitMaxK; ++j) vals[5 + j] = xs[j - 1];
  double* out = a.partial + (size_t)chunk * a.part_pad * nv;
#pragma unroll
  for (int rd = 0; rd < kTVals / kTRound; ++rd) {
    if (rd * kTRound >= nv) break;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTRound; ++i) red[(i * 16 + q) * kTReps + r16] = vals[rd * kTRound + i];
    __syncthreads();
    if (tid < kTRound * kTReps) {
      const int vi = tid >> 4, slot = rd * kTRound + vi;
      double v = 0.0;
      for (int qq = 0; qq < 16; ++qq) v += red[(vi * 16 + qq) * kTReps + r16];
      if (slot < nv && act) out[(size_t)rep * nv + slot] = v;
    }
  }
}

inline size_t tb_means_lds(int k) {
  return sizeof(double) * ((size_t)(k + 1) * kTS + (size_t)kTReps * 2 * ((k + 1) | 1) + (size_t)kTRound * 16 * kTReps);
}

// One wave per replicate: the means partials of both groups in chunk order, then the terms of include/oaxaca_boot.h's
// Tobit row. A replicate one of whose fits failed or did not converge, or one of whose groups has sum c w = 0, gets
// ok = 0 and a NaN row.
__global__ __launch_bounds__(64) void ob_tobit_row_kernel(const TbArgs a) {
  __shared__ double S[2 * (5 + ob::kTobitMaxK)];
  __shared__ double beta[2][kTMaxD];
  __shared__ double den[3];
  const int lane = threadIdx.x, k = a.k, D = k + 1, nv = tb_mv(k);
  const uint32_t rep = blockIdx.x;
  if (rep >= a.n_reps) return;
  for (int i = lane; i < 2 * nv; i += 64) {
    const uint32_t g = (uint32_t)(i / nv);
    const int j = i - (int)g * nv;
    double v = 0.0;
    for (int c = 0; c < a.n_chunks; ++c)
      if (a.chunks[3 * c] == g) v += a.partial[((size_t)c * a.part_pad + rep) * nv + j];
    S[i] = v;
  }
  for (int i = lane; i < 2 * D; i += 64) {
    const int g = i / D, j = i - g * D;
    const double* eta = a.eta + ((size_t)g * a.part_pad + rep) * D;
    beta[g][j] = j < k ? eta[j] / eta[k] : 1.0 / eta[k];
  }
  __syncthreads();
  double* row = a.rows + (size_t)rep * a.row_len;
  const uint32_t fa = a.flags[rep], fb = a.flags[(size_t)a.part_pad + rep];
  const double* SA = S;
  const double* SB = S + nv;
  const double na = SA[3], nb = SB[3];
  const bool failed = !(fa & kTbDone) || (fa & kTbFailed) || !(fb & kTbDone) || (fb & kTbFailed) || !(na > 0.0) || !(nb > 0.0);
  if (failed) {
    for (int i = lane; i < a.row_len; i += 64) row[i] = __builtin_nan("");
    if (lane == 0) a.ok[rep] = 0;
    return;
  }
  const double *ba = beta[0], *bb = beta[1];
  const double* bs = a.ref == OB_REF_GROUP_A ? ba : bb;
  const double maa = SA[0] / na, mab = SA[1] / na, mba = SB[0] / nb, mbb = SB[1] / nb;
  const double mas = a.ref == OB_REF_GROUP_A ? maa : mab, mbs = a.ref == OB_REF_GROUP_A ? mba : mbb;
  const double total = maa - mbb, expl = mas - mbs;
  const double ua = maa - mas, ub = mbs - mbb;
  auto xbar = [&](const double* Sg, double ng, int j) { return j == 0 ? 1.0 : Sg[5 + j] / ng; };
  if (lane == 0) {  // Yun's denominators, in column order: also the latent terms
    double de = 0.0, da = 0.0, db = 0.0;
    for (int j = 0; j < k; ++j) {
      const double xa = xbar(SA, na, j), xb = xbar(SB, nb, j);
      de += (xa - xb) * bs[j];
      da += xa * (ba[j] - bs[j]);
      db += xb * (bs[j] - bb[j]);
    }
    den[0] = de;
    den[1] = da;
    den[2] = db;
  }
  __syncthreads();
  const double de = den[0], da = den[1], db = den[2];
  double* tail = row + 6 + 2 * k;
  for (int j = lane; j < k; j += 64) {
    const double xa = xbar(SA, na, j), xb = xbar(SB, nb, j);
    // a part whose denominator is exactly 0 contributes 0.0 (U_A under GroupA, U_B under GroupB)
    const double te = de == 0.0 ? 0.0 : expl * ((xa - xb) * bs[j]) / de;
    const double ta = da == 0.0 ? 0.0 : ua * (xa * (ba[j] - bs[j])) / da;
    const double tb = db == 0.0 ? 0.0 : ub * (xb * (bs[j] - bb[j])) / db;
    row[6 + j] = te;
    row[6 + k + j] = ta + tb;
    tail[j] = ba[j];
    tail[k + j] = bb[j];
    tail[2 * k + j] = xa;
    tail[3 * k + j] = xb;
    tail[4 * k + j] = bs[j];
  }
  if (lane == 0) {
    const double endow = mab - mbb, coef = mba - mbb;
    row[0] = expl;
    row[1] = total - expl;
    row[2] = endow;
    row[3] = coef;
    row[4] = total - endow - coef;
    row[5] = total;
    double* sc = tail + 5 * k;
    sc[0] = de;
    sc[1] = da + db;
    sc[2] = de + (da + db);
    sc[3] = maa;
    sc[4] = mab;
    sc[5] = mba;
    sc[6] = mbb;
    sc[7] = SA[2] / na;
    sc[8] = SB[2] / nb;
    sc[9] = ba[k];
    sc[10] = bb[k];
    sc[11] = SA[4] / na;
    sc[12] = SA[5] / na;
    sc[13] = SB[4] / nb;
    sc[14] = SB[5] / nb;
    sc[15] = (double)a.passes[rep];
    sc[16] = (double)a.passes[(size_t)a.part_pad + rep];
    a.ok[rep] = 1;
  }
}

hipError_t launch_pass(const TbArgs& a, hipStream_t s) {
  const size_t lds = tb_lds(a.k);
  hipError_t e = hipFuncSetAttribute((const void*)ob_tobit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ob_tobit_kernel, dim3(a.n_chunks, (a.n_reps + kTReps - 1) / kTReps), dim3(kTB), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_means(const TbArgs& a, hipStream_t s) {
  const size_t lds = tb_means_lds(a.k);
  hipError_t e = hipFuncSetAttribute((const void*)ob_tobit_means_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ob_tobit_means_kernel, dim3(a.n_chunks, (a.n_reps + kTReps - 1) / kTReps), dim3(kTB), lds, s, a);
  return hipGetLastError();
}

thread_local ob_tobit_timing g_timing = {};

bool tb_args_ok(const TbArgs& a) {
  return a.k >= 1 && a.k <= ob::kTobitMaxK && a.n_reps >= 1 && a.part_pad >= a.n_reps && a.n_chunks >= 1;
}

// The Newton loop of one batch (or of the point pass), every fit stopping on its own: eta from start [2][k + 1], one
// pass and one step per round until no fit is left iterating, at most kTbMaxPasses rounds. The host waits once per
// round (the count of fits still iterating).
int tb_fit_loop(const TbArgs& a, const double* start, int n_groups, hipStream_t s) {
  if (!tb_args_ok(a)) return ob::fail(OB_E_INVALID, "tobit batch: bad shape");
  hipLaunchKernelGGL(ob_tobit_init_kernel, dim3((a.n_reps + 63) / 64), dim3(64), 0, s, a, start, n_groups);
  OB_HIP(hipGetLastError());
  int it = 0;
  float ms = 0.f;
  OB_TRY(newton_rounds(
      a.active, kTbMaxPasses, s, [&] { return launch_pass(a, s); },
      [&] {
        hipLaunchKernelGGL(ob_tobit_step_kernel, dim3(a.n_reps, n_groups), dim3(64), 0, s, a);
        return hipGetLastError();
      },
      &it, &ms));
  g_timing.pass_ms += ms;
  g_timing.pass_launches += it;
  g_timing.passes = std::max(g_timing.passes, (int32_t)it);
  return OB_OK;
}

// The stages over one batch (or the point pass): the fits, the means, the rows.
int tb_batch(const TbArgs& a, const double* start, hipStream_t s) {
  OB_TRY(tb_fit_loop(a, start, 2, s));
  Events<3> ev;
  OB_HIP(ev.create());
  OB_HIP(hipEventRecord(ev.e[0], s));
  OB_HIP(launch_means(a, s));
  OB_HIP(hipEventRecord(ev.e[1], s));
  hipLaunchKernelGGL(ob_tobit_row_kernel, dim3(a.n_reps), dim3(64), 0, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[2], s));
  OB_HIP(hipEventSynchronize(ev.e[2]));
  float m0 = 0.f, m1 = 0.f;
  OB_HIP(hipEventElapsedTime(&m0, ev.e[0], ev.e[1]));
  OB_HIP(hipEventElapsedTime(&m1, ev.e[1], ev.e[2]));
  g_timing.means_ms += m0;
  g_timing.row_ms += m1;
  return OB_OK;
}

size_t partial_vals(int k) { return std::max<size_t>(tb_nv(k), tb_mv(k)); }

// The limits of a configuration (NULL: none), checked without data.
struct Limits {
  double lower = 0.0, upper = 0.0;
  int has_lower = 0, has_upper = 0;
};
int limits_from(const ob_tobit_config* tc, Limits& L) {
  L = Limits();
  if (!tc) return OB_OK;
  L.has_lower = tc->has_lower != 0;
  L.has_upper = tc->has_upper != 0;
  L.lower = L.has_lower ? tc->lower : 0.0;
  L.upper = L.has_upper ? tc->upper : 0.0;
  if ((L.has_lower && !std::isfinite(L.lower)) || (L.has_upper && !std::isfinite(L.upper)))
    return ob::fail(OB_E_INVALID, "tobit decomposition: a limit must be finite");
  if (L.has_lower && L.has_upper && L.lower >= L.upper)
    return ob::fail(OB_E_INVALID, "tobit decomposition: lower (%g) must be below upper (%g)", L.lower, L.upper);
  return OB_OK;
}
void limits_into(const Limits& L, TbArgs& h) {
  h.lower = L.lower;
  h.upper = L.upper;
  h.has_lower = L.has_lower;
  h.has_upper = L.has_upper;
}

// The outcome's range and the uncensored rows of one group: *n_unc, and n_cens[2] the rows at the two limits.
int limits_check_rows(const char* what, const Limits& L, const double* y, int64_t n, int64_t* n_unc, int64_t n_cens[2]) {
  n_cens[0] = n_cens[1] = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (L.has_lower && y[i] < L.lower)
      return ob::fail(OB_E_INVALID, "%s: outcome %g in row %lld lies below the lower limit %g", what, y[i], (long long)i, L.lower);
    if (L.has_upper && y[i] > L.upper)
      return ob::fail(OB_E_INVALID, "%s: outcome %g in row %lld lies above the upper limit %g", what, y[i], (long long)i, L.upper);
    if (L.has_lower && y[i] == L.lower)
      ++n_cens[0];
    else if (L.has_upper && y[i] == L.upper)
      ++n_cens[1];
  }
  *n_unc = n - n_cens[0] - n_cens[1];
  return OB_OK;
}

// The start of a point fit: the group's (weighted) least squares on all rows, delta = beta / s, theta = 1 / s with
// s^2 = sum w r^2 / sum w. x: n x k column-major with ld ldx, column 0 the intercept. false: no Cholesky factor, or
// s is not positive and finite.
bool ols_start(const double* x, int64_t ldx, const double* y, const double* w, int64_t n, int k, double* eta) {
  std::vector<double> m((size_t)k * k, 0.0), b((size_t)k, 0.0);
  for (int j = 0; j < k; ++j)
    for (int i = j; i < k; ++i) {
      double v = 0.0;
      for (int64_t r = 0; r < n; ++r) v += (w ? w[r] : 1.0) * x[(size_t)i * ldx + r] * x[(size_t)j * ldx + r];
      m[i + (size_t)j * k] = v;
    }
  for (int j = 0; j < k; ++j) {
    double v = 0.0;
    for (int64_t r = 0; r < n; ++r) v += (w ? w[r] : 1.0) * x[(size_t)j * ldx + r] * y[r];
    b[j] = v;
  }
  if (!ob::chol_factor_solve(m.data(), k, b.data(), ob::BackSub::Dot)) return false;
  double rss = 0.0, sw = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    double f = 0.0;
    for (int j = 0; j < k; ++j) f += x[(size_t)j * ldx + r] * b[j];
    const double wr = w ? w[r] : 1.0;
    rss += wr * (y[r] - f) * (y[r] - f);
    sw += wr;
  }
  const double s = std::sqrt(rss / sw);
  if (!(s > 0.0) || !std::isfinite(s)) return false;
  for (int j = 0; j < k; ++j) eta[j] = b[j] / s;
  eta[k] = 1.0 / s;
  return true;
}

const char* const kTobitFailed = "%stobit decomposition: the censored-normal fit of the point estimate failed";

}  // namespace

namespace ob {

int tobit_check_shape(int k, int64_t n_a, int64_t n_b) {
  if (k < 1 || n_a < 0 || n_b < 0)
    return fail(OB_E_INVALID, "tobit decomposition: bad shape (k = %d, n_a = %lld, n_b = %lld)", k, (long long)n_a,
                (long long)n_b);
  if (k > kTobitMaxK)
    return fail(OB_E_UNSUPPORTED, "tobit decomposition: at most %d design columns with the intercept, got %d", kTobitMaxK, k);
  if (n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31))
    return fail(OB_E_UNSUPPORTED, "tobit decomposition: groups take fewer than 2^31 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k)
      return fail(OB_E_INSUFFICIENT, "%stobit decomposition: a group's uncensored rows (%lld) must exceed the design columns (%d)",
                  error_prefix(OB_E_INSUFFICIENT), (long long)n, k);
  return OB_OK;
}

// Device side of a prepared Tobit run. The handle's ob_panel (no predictors, the outcome alone) is the resampler:
// engine_counts draws a segment's count images for its row counts, and its chunk table is the one the passes walk.
struct TobitState {
  int k = 0;
  Limits lim;
  DevBuf cols[2];  // [y | x_1 .. x_{k-1} | w] x ld
  DevBuf chunks, eta, flags, passes, partial, start;
  int n_chunks = 0;
  std::vector<double> eta_hat;  // [2][k + 1] the point fits
  int64_t n_cens[2][2] = {{0, 0}, {0, 0}};
  int32_t point_passes[2] = {0, 0};
};

static TobitState* tobit_state(const ob_prepared* pr) { return model_state<TobitState>(pr, kModelTobit); }

static TbArgs tb_args(const ob_prepared* pr, const TobitState* st) {
  const ob_panel* p = pr->panel;
  TbArgs h{};
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
  h.ref = pr->ref;
  h.tol = 1e-6;
  limits_into(st->lim, h);
  return h;
}

static uint32_t tb_batch_reps(const TobitState* st, uint32_t rep_pad) {
  return boot_batch_reps((size_t)st->n_chunks * partial_vals(st->k) * sizeof(double), rep_pad);
}

// Workspace for batches of hb replicates.
static int tb_ensure(TobitState* st, uint32_t hb) {
  OB_HIP(st->eta.alloc(sizeof(double) * 2 * (size_t)hb * (st->k + 1)));
  OB_HIP(st->flags.alloc(sizeof(uint32_t) * (2 * (size_t)hb + 1)));
  OB_HIP(st->passes.alloc(sizeof(uint32_t) * 2 * (size_t)hb));
  OB_HIP(st->partial.alloc(sizeof(double) * (size_t)st->n_chunks * hb * partial_vals(st->k)));
  return OB_OK;
}

static void tb_bind(TbArgs& h, const TobitState* st, uint32_t hb) {
  h.part_pad = hb;
  h.eta = st->eta.d();
  h.flags = st->flags.as<uint32_t>();
  h.active = h.flags + 2 * (size_t)hb;
  h.passes = st->passes.as<uint32_t>();
  h.partial = st->partial.d();
}

// The point pass from the OLS starts; afterwards st->start holds the point fits, from which every replicate starts.
static int tb_point(ob_prepared* pr, TobitState* st, const double* start) {
  ob_panel* p = pr->panel;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = p->ctx->stream;
  const int D = st->k + 1;
  OB_TRY(tb_ensure(st, 64));
  OB_HIP(st->start.alloc(sizeof(double) * 2 * D));
  OB_HIP(hipMemcpyAsync(st->start.p, start, sizeof(double) * 2 * D, hipMemcpyHostToDevice, s));
  DevBuf d_row, d_ok;
  OB_HIP(d_row.alloc(sizeof(double) * pr->row_len));
  OB_HIP(d_ok.alloc(1));
  TbArgs h = tb_args(pr, st);
  tb_bind(h, st, 64);
  h.counts = nullptr;
  h.nb_rep = 1;
  h.n_reps = 1;
  h.rows = d_row.d();
  h.ok = d_ok.as<uint8_t>();
  OB_TRY(tb_batch(h, st->start.d(), s));
  uint8_t okh = 0;
  pr->point_row.assign((size_t)pr->row_len, 0.0);
  st->eta_hat.assign((size_t)2 * D, 0.0);
  OB_HIP(hipMemcpyAsync(pr->point_row.data(), d_row.p, sizeof(double) * pr->row_len, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(&okh, d_ok.p, 1, hipMemcpyDeviceToHost, s));
  for (int g = 0; g < 2; ++g)
    OB_HIP(hipMemcpyAsync(st->eta_hat.data() + (size_t)g * D, st->eta.d() + (size_t)g * 64 * D, sizeof(double) * D,
                          hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  if (!okh) return fail(OB_E_LINALG, kTobitFailed, error_prefix(OB_E_LINALG));
  for (int g = 0; g < 2; ++g) st->point_passes[g] = (int32_t)pr->point_row[(size_t)pr->row_len - 2 + g];
  OB_HIP(hipMemcpy(st->start.p, st->eta_hat.data(), sizeof(double) * 2 * D, hipMemcpyHostToDevice));
  return OB_OK;
}

static int tb_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                          hipStream_t stream) {
  TobitState* st = tobit_state(pr);
  uint32_t hb = 0;
  const BootPlan plan{kFitSegReps, kCountBudget, true, [&](uint32_t seg_pad) {
                        g_timing = {};
                        hb = tb_batch_reps(st, seg_pad);
                        return tb_ensure(st, hb);
                      }};
  return boot_segmented(pr, kModelTobit, plan, first_rep, n_reps, d_rows && d_ok, stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t nb_rep, uint32_t, hipStream_t s) {
    return boot_batches(ns, hb, [&](uint32_t b0, uint32_t nb) {  // hb is a multiple of 64: whole image blocks
      TbArgs h = tb_args(pr, st);
      tb_bind(h, st, hb);
      h.counts = pr->panel->d_counts + (size_t)(b0 / 64) * 4 * kCimgWords;
      h.nb_rep = nb_rep;
      h.n_reps = nb;
      h.rows = d_rows + (s0 + b0) * pr->row_len;
      h.ok = d_ok + s0 + b0;
      return tb_batch(h, st->start.d(), s);
    });
  });
}

// installs the builder's hooks when the library loads (ob_model.hpp)
static const bool g_tobit_hooks_installed = model_install(
    kModelTobit, {tb_boot_device, model_boot_host, [](void* s) { delete static_cast<TobitState*>(s); }});

// Every check of the frame entry points, before any device work and before the context is read: the limits, settings
// outside the scope, nulls, non-finite values and negative weights in named columns, the design (ob::data_matrices),
// the outcome's range, the shape and each group's uncensored rows. On success m holds the design matrices and the
// groups' weights, n_cens the rows at the limits.
static int tb_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                    const ob_tobit_config* tc, Config& c, Matrices& m, Limits& L, int64_t n_cens[2][2]) {
  const char* label = model_name(kModelTobit).label;
  OB_TRY(config_from(cfg, c));
  if (!c.normalize.empty()) return model_refuse(kModelTobit, "normalized categoricals are");
  if (c.has_selection || !c.selection_predictors.empty()) return model_refuse(kModelTobit, "Heckman selection settings are");
  if (c.has_cluster) return model_refuse(kModelTobit, "the cluster bootstrap is");
  if (c.ref != OB_REF_GROUP_A && c.ref != OB_REF_GROUP_B)
    return model_refuse(kModelTobit, "reference coefficients other than GroupA and GroupB (sigma* has no agreed definition for them) are");
  OB_TRY(limits_from(tc, L));
  OB_TRY(stage_named(cols, n_cols, n_rows, c, kModelTobit, true, true, true));
  OB_TRY(m.load(cols, n_cols, n_rows, cfg, true));
  if (m.k > kTobitMaxK) OB_TRY(tobit_check_shape(m.k, m.n[0], m.n[1]));
  if (m.n[0] == 0 || m.n[1] == 0) return fail(OB_E_GROUP, "%sOne group has no data", error_prefix(OB_E_GROUP));
  int64_t n_unc[2];
  for (int g = 0; g < 2; ++g) OB_TRY(limits_check_rows(label, L, m.y[g], m.n[g], &n_unc[g], n_cens[g]));
  return tobit_check_shape(m.k, n_unc[0], n_unc[1]);
}

static int tb_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_tobit_config* tc, ob_prepared** out) {
  Config c;
  Matrices m;
  Limits L;
  int64_t n_cens[2][2];
  OB_TRY(tb_stage(cols, n_cols, n_rows, cfg, tc, c, m, L, n_cens));
  const int k = m.k, D = k + 1;
  std::vector<double> start((size_t)2 * D);
  for (int g = 0; g < 2; ++g)
    if (!ols_start(m.x[g], m.n[g], m.y[g], m.w(g), m.n[g], k, start.data() + (size_t)g * D))
      return fail(OB_E_LINALG, kTobitFailed, error_prefix(OB_E_LINALG));
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  TobitState* st = new TobitState();
  st->k = k;
  st->lim = L;
  std::memcpy(st->n_cens, n_cens, sizeof(n_cens));
  ob_prepared* pr = model_handle(ctx, c, m, kModelTobit, st, tobit_row_len(k), 1);
  auto build = [&]() -> int {
    OB_TRY(outcome_panel(ctx, m, &pr->panel));
    ob_panel* p = pr->panel;
    for (int g = 0; g < 2; ++g) {
      OB_TRY(upload_group(st->cols[g], p->ld[g], m.n[g], k, 1, m.y[g], m.x[g]));
      OB_TRY(upload_weights(st->cols[g], p->ld[g], m.n[g], k, m.w(g)));
    }
    OB_TRY(upload_chunks(p, st->chunks, &st->n_chunks));
    g_timing = {};
    return tb_point(pr, st, start.data());
  };
  return model_built(pr, build(), out);
}

// ---- the array entry points ---------------------------------------------------------------------------------------

// Up to two groups of rows on the device as a run holds them, with count images for n_reps replicates (counts[g]:
// [n_reps][n_g] bytes, rep_stride n_g, or 0 for one image that every replicate shares; NULL: every row once).
struct TbArrays {
  DevBuf cols[2], chunks, eta, flags, passes, partial, counts, start, rows, ok;
  std::vector<uint32_t> table, img;
  uint32_t n[2] = {0, 0}, tiles[2] = {0, 0}, part_pad = 64;
  int64_t ld[2] = {0, 0};
  int n_chunks = 0;
  TbArgs h{};
};
struct TbGroup {
  const double *x, *y, *w;  // x: n x k column-major with ld ldx, column 0 the intercept
  int64_t ldx, n;
  const uint8_t* counts;
  int64_t rep_stride;
};

static int tb_arrays(ob_ctx* ctx, int k, const Limits& L, const TbGroup (&gr)[2], bool counted, uint32_t n_reps,
                     TbArrays& A) {
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int D = k + 1;
  for (int g = 0; g < 2; ++g) {
    A.n[g] = (uint32_t)gr[g].n;
    A.tiles[g] = (A.n[g] + OB_TILE_ROWS - 1) / OB_TILE_ROWS;
    A.ld[g] = (int64_t)A.tiles[g] * OB_TILE_ROWS;
    group_chunks((uint32_t)g, A.tiles[g], 64u, A.table);
  }
  A.n_chunks = (int)(A.table.size() / 3);
  const uint32_t nb_rep = (n_reps + 63) / 64;
  A.part_pad = nb_rep * 64;
  for (int g = 0; g < 2; ++g) {
    const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(A.ld[g], 1) * (k + 1);
    OB_HIP(A.cols[g].alloc(bytes));
    OB_HIP(hipMemsetAsync(A.cols[g].p, 0, bytes, s));
    if (!A.n[g]) continue;
    const size_t nb = sizeof(double) * A.n[g];
    OB_HIP(hipMemcpyAsync(A.cols[g].p, gr[g].y, nb, hipMemcpyHostToDevice, s));
    for (int j = 1; j < k; ++j)
      OB_HIP(hipMemcpyAsync(A.cols[g].d() + (size_t)j * A.ld[g], gr[g].x + (size_t)j * gr[g].ldx, nb, hipMemcpyHostToDevice, s));
    OB_HIP(hipStreamSynchronize(s));  // the unit weights below live on this frame
    const std::vector<double> unit(gr[g].w ? 0 : (size_t)A.n[g], 1.0);
    OB_HIP(hipMemcpy(A.cols[g].d() + (size_t)k * A.ld[g], gr[g].w ? gr[g].w : unit.data(), nb, hipMemcpyHostToDevice));
  }
  OB_HIP(A.chunks.alloc(sizeof(uint32_t) * A.table.size()));
  OB_HIP(hipMemcpyAsync(A.chunks.p, A.table.data(), sizeof(uint32_t) * A.table.size(), hipMemcpyHostToDevice, s));
  OB_HIP(A.eta.alloc(sizeof(double) * 2 * (size_t)A.part_pad * D));
  OB_HIP(hipMemsetAsync(A.eta.p, 0, sizeof(double) * 2 * (size_t)A.part_pad * D, s));
  OB_HIP(A.flags.alloc(sizeof(uint32_t) * (2 * (size_t)A.part_pad + 1)));
  OB_HIP(hipMemsetAsync(A.flags.p, 0, sizeof(uint32_t) * (2 * (size_t)A.part_pad + 1), s));
  OB_HIP(A.passes.alloc(sizeof(uint32_t) * 2 * (size_t)A.part_pad));
  OB_HIP(hipMemsetAsync(A.passes.p, 0, sizeof(uint32_t) * 2 * (size_t)A.part_pad, s));
  const size_t pbytes = sizeof(double) * (size_t)A.n_chunks * A.part_pad * partial_vals(k);
  OB_HIP(A.partial.alloc(pbytes));
  OB_HIP(hipMemsetAsync(A.partial.p, 0, pbytes, s));
  if (counted) {
    A.img.assign((size_t)(A.tiles[0] + A.tiles[1]) * nb_rep * 4 * kCimgWords, 0u);
    for (int g = 0; g < 2; ++g)
      if (A.n[g])
        pack_count_images(gr[g].counts, A.n[g], gr[g].rep_stride, n_reps, nb_rep,
                          A.img.data() + (size_t)(g ? A.tiles[0] : 0u) * nb_rep * 4 * kCimgWords, nullptr, 0);
    OB_HIP(A.counts.alloc(sizeof(uint32_t) * A.img.size()));
    OB_HIP(hipMemcpyAsync(A.counts.p, A.img.data(), sizeof(uint32_t) * A.img.size(), hipMemcpyHostToDevice, s));
  }
  TbArgs& h = A.h;
  for (int g = 0; g < 2; ++g) {
    h.cols[g] = A.cols[g].d();
    h.ld[g] = A.ld[g];
    h.n[g] = A.n[g];
  }
  h.tiles0 = A.tiles[0];
  h.k = k;
  h.counts = counted ? A.counts.as<uint32_t>() : nullptr;
  h.nb_rep = nb_rep;
  h.chunks = A.chunks.as<uint32_t>();
  h.n_chunks = A.n_chunks;
  h.n_reps = n_reps;
  h.part_pad = A.part_pad;
  h.eta = A.eta.d();
  h.flags = A.flags.as<uint32_t>();
  h.active = h.flags + 2 * (size_t)A.part_pad;
  h.passes = A.passes.as<uint32_t>();
  h.partial = A.partial.d();
  h.tol = 1e-6;
  limits_into(L, h);
  return OB_OK;
}

// The argument checks the array pieces share (before any device work).
static int tb_piece_check(const char* what, const double* x, int64_t ldx, const double* y, const double* w, int64_t n, int32_t k,
                          const Limits& L) {
  if (!x || !y) return fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || k < 1) return fail(OB_E_INVALID, "%s needs n > 0 rows and k >= 1 columns, got n = %lld, k = %d", what, (long long)n, k);
  if (k > kTobitMaxK) return fail(OB_E_UNSUPPORTED, "%s takes at most %d columns, got %d", what, kTobitMaxK, k);
  if (ldx < n) return fail(OB_E_INVALID, "%s: ldx = %lld is below n = %lld", what, (long long)ldx, (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(OB_E_UNSUPPORTED, "%s takes fewer than 2^31 rows", what);
  for (int64_t i = 0; i < n; ++i)  // the pass takes x_0 = 1 as given
    if (x[i] != 1.0) return fail(OB_E_UNSUPPORTED, "%s: column 0 of x must be the intercept (all ones)", what);
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(y[i])) return fail(OB_E_INVALID, "%s: outcome in row %lld is not finite", what, (long long)i);
    if (w && !(w[i] >= 0.0 && std::isfinite(w[i])))
      return fail(OB_E_INVALID, "%s: weight in row %lld is negative or not finite", what, (long long)i);
  }
  int64_t n_unc, n_cens[2];
  return limits_check_rows(what, L, y, n, &n_unc, n_cens);
}

static int tb_etas_check(const char* what, const double* etas, int32_t n_etas, int k) {
  if (!etas) return fail(OB_E_INVALID, "null pointer");
  for (int32_t r = 0; r < n_etas; ++r) {
    for (int j = 0; j <= k; ++j)
      if (!std::isfinite(etas[(size_t)r * (k + 1) + j])) return fail(OB_E_INVALID, "%s: a parameter is not finite", what);
    if (!(etas[(size_t)r * (k + 1) + k] > 0.0)) return fail(OB_E_INVALID, "%s: theta must be positive", what);
  }
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_tobit_row_len(int32_t k) { return k < 1 ? 0 : ob::tobit_row_len(k); }

int ob_tobit_check_shape(int32_t k, int64_t n_a, int64_t n_b) { return ob::tobit_check_shape(k, n_a, n_b); }

int ob_tobit_last_timing(ob_tobit_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

int ob_tobit_lambda(const double* z, int64_t n, double* out) {
  if (!z || !out || n < 0) return ob::fail(OB_E_INVALID, "null pointer");
  for (int64_t i = 0; i < n; ++i) out[i] = ob::tobit_lambda_host(z[i]);
  return OB_OK;
}

int ob_builder_prepare_tobit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                             const ob_builder_config* cfg, const ob_tobit_config* tc, ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::tb_prepare(ctx, cols, n_cols, n_rows, cfg, tc, out);
}

int ob_builder_run_tobit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                         const ob_tobit_config* tc, ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::tb_prepare(ctx, cols, n_cols, n_rows, cfg, tc, &pr));
  const uint64_t reps = pr->cfg.reps;
  std::vector<double> rows((size_t)reps * pr->row_len);
  std::vector<uint8_t> ok(reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::finish(pr, 0, rows.data(), ok.data(), reps, out);
  ob_prepared_destroy(pr);
  return rc;
}

int ob_prepared_tobit_info(const ob_prepared* prep, ob_tobit_info* out) {
  if (!prep || !out) return ob::fail(OB_E_INVALID, "null pointer");
  const ob::TobitState* st = ob::tobit_state(prep);
  if (!st) return ob::fail(OB_E_INVALID, "not a handle of a tobit decomposition");
  out->k = st->k;
  out->lower = st->lim.lower;
  out->upper = st->lim.upper;
  out->has_lower = st->lim.has_lower;
  out->has_upper = st->lim.has_upper;
  out->n_a = prep->n_a;
  out->n_b = prep->n_b;
  out->n_left_a = st->n_cens[0][0];
  out->n_right_a = st->n_cens[0][1];
  out->n_left_b = st->n_cens[1][0];
  out->n_right_b = st->n_cens[1][1];
  out->eta = st->eta_hat.data();
  out->passes_a = st->point_passes[0];
  out->passes_b = st->point_passes[1];
  return OB_OK;
}

// One pass alone over one group of rows (include/oaxaca_boot.h).
int ob_tobit_pass(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                  int64_t n, int32_t k, const ob_tobit_config* tc, const double* etas, int32_t n_etas, double* info,
                  double* grad, double* n_unc) {
  if (!info || !grad || !n_unc) return ob::fail(OB_E_INVALID, "null pointer");
  Limits L;
  OB_TRY(limits_from(tc, L));
  OB_TRY(ob::tb_piece_check("ob_tobit_pass", x, ldx, y, w, n, k, L));
  if (n_etas < 1 || n_etas > 64) return ob::fail(OB_E_INVALID, "ob_tobit_pass takes 1 to 64 parameter vectors, got %d", n_etas);
  OB_TRY(ob::tb_etas_check("ob_tobit_pass", etas, n_etas, k));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  const int D = k + 1, NH = D * (D + 1) / 2, nv = tb_nv(k);
  ob::TbArrays A;
  const ob::TbGroup gr[2] = {{x, y, w, ldx, n, counts, 0}, {nullptr, nullptr, nullptr, 0, 0, nullptr, 0}};
  OB_TRY(ob::tb_arrays(ctx, k, L, gr, counts != nullptr, (uint32_t)n_etas, A));
  hipStream_t s = ctx->stream;
  OB_HIP(hipMemcpyAsync(A.eta.p, etas, sizeof(double) * (size_t)n_etas * D, hipMemcpyHostToDevice, s));
  OB_HIP(launch_pass(A.h, s));
  std::vector<double> part((size_t)A.n_chunks * A.part_pad * nv);
  OB_HIP(hipMemcpyAsync(part.data(), A.partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  for (int r = 0; r < n_etas; ++r) {
    std::vector<double> sum((size_t)nv, 0.0);
    for (int c = 0; c < A.n_chunks; ++c)  // chunk order, as the step kernel
      for (int e = 0; e < nv; ++e) sum[e] += part[((size_t)c * A.part_pad + r) * nv + e];
    const double theta = etas[(size_t)r * D + k], nu = sum[NH + D];
    for (int j = 0; j < D; ++j) {
      for (int i = 0; i <= j; ++i) {
        double v = sum[j * (j + 1) / 2 + i];
        if (j == k && i == k) v += nu / (theta * theta);
        info[((size_t)r * D + j) * D + i] = v;
        info[((size_t)r * D + i) * D + j] = v;
      }
      grad[(size_t)r * D + j] = sum[NH + j] + (j == k ? nu / theta : 0.0);
    }
    n_unc[r] = nu;
  }
  return OB_OK;
}

// The fits alone over one group of rows (include/oaxaca_boot.h).
int ob_tobit_fit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, int64_t n, int32_t k,
                 const ob_tobit_config* tc, const uint8_t* counts, int32_t n_reps, const double* eta0, double* eta,
                 uint32_t* flags, uint32_t* passes) {
  if (!eta || !flags || !passes) return ob::fail(OB_E_INVALID, "null pointer");
  Limits L;
  OB_TRY(limits_from(tc, L));
  OB_TRY(ob::tb_piece_check("ob_tobit_fit", x, ldx, y, w, n, k, L));
  if (n_reps < 1 || n_reps > OB_TOBIT_MAX_ARRAY_REPS)
    return ob::fail(OB_E_INVALID, "ob_tobit_fit takes 1 to %d replicates, got %d", OB_TOBIT_MAX_ARRAY_REPS, n_reps);
  const int D = k + 1;
  std::vector<double> start((size_t)2 * D, 0.0);
  if (eta0) {
    OB_TRY(ob::tb_etas_check("ob_tobit_fit", eta0, 1, k));
    std::copy(eta0, eta0 + D, start.begin());
  } else if (!ols_start(x, ldx, y, w, n, k, start.data())) {
    return ob::fail(OB_E_LINALG, "%sob_tobit_fit: the least-squares start failed", ob::error_prefix(OB_E_LINALG));
  }
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  ob::TbArrays A;
  const ob::TbGroup gr[2] = {{x, y, w, ldx, n, counts, n}, {nullptr, nullptr, nullptr, 0, 0, nullptr, 0}};
  OB_TRY(ob::tb_arrays(ctx, k, L, gr, counts != nullptr, (uint32_t)n_reps, A));
  hipStream_t s = ctx->stream;
  OB_HIP(A.start.alloc(sizeof(double) * 2 * D));
  OB_HIP(hipMemcpyAsync(A.start.p, start.data(), sizeof(double) * 2 * D, hipMemcpyHostToDevice, s));
  g_timing = {};
  OB_TRY(tb_fit_loop(A.h, A.start.d(), 1, s));
  OB_HIP(hipMemcpyAsync(eta, A.eta.p, sizeof(double) * (size_t)n_reps * D, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(flags, A.flags.p, sizeof(uint32_t) * n_reps, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(passes, A.passes.p, sizeof(uint32_t) * n_reps, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  return OB_OK;
}

// The means pass alone over one group of rows (include/oaxaca_boot.h).
int ob_tobit_means(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, const double* w, const uint8_t* counts,
                   int64_t n, int32_t k, const ob_tobit_config* tc, const double* etas, double* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  Limits L;
  OB_TRY(limits_from(tc, L));
  OB_TRY(ob::tb_piece_check("ob_tobit_means", x, ldx, y, w, n, k, L));
  OB_TRY(ob::tb_etas_check("ob_tobit_means", etas, 2, k));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  const int D = k + 1, nv = tb_mv(k);
  ob::TbArrays A;
  const ob::TbGroup gr[2] = {{x, y, w, ldx, n, counts, 0}, {nullptr, nullptr, nullptr, 0, 0, nullptr, 0}};
  OB_TRY(ob::tb_arrays(ctx, k, L, gr, counts != nullptr, 1, A));
  hipStream_t s = ctx->stream;
  for (int v = 0; v < 2; ++v)  // replicate 0 of the two parameter blocks
    OB_HIP(hipMemcpyAsync(A.eta.d() + (size_t)v * A.part_pad * D, etas + (size_t)v * D, sizeof(double) * D, hipMemcpyHostToDevice, s));
  OB_HIP(launch_means(A.h, s));
  std::vector<double> part((size_t)A.n_chunks * A.part_pad * nv);
  OB_HIP(hipMemcpyAsync(part.data(), A.partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  std::vector<double> sum((size_t)nv, 0.0);
  for (int c = 0; c < A.n_chunks; ++c)  // chunk order, as the row kernel
    for (int j = 0; j < nv; ++j) sum[j] += part[(size_t)c * A.part_pad * nv + j];
  const double cw = sum[3];
  out[0] = sum[0] / cw;
  out[1] = sum[1] / cw;
  out[2] = sum[2] / cw;
  out[3] = cw;
  out[4] = sum[4] / cw;
  out[5] = sum[5] / cw;
  out[6] = 1.0;
  for (int j = 1; j < k; ++j) out[6 + j] = sum[5 + j] / cw;
  return OB_OK;
}

// Fits, means and rows over two groups of rows with given counts (include/oaxaca_boot.h).
int ob_tobit_rows(ob_ctx* ctx, int32_t k, const ob_tobit_config* tc, int32_t reference_coeffs, const double* xa, int64_t ldxa,
                  const double* ya, const double* wa, int64_t na, const uint8_t* counts_a, const double* xb, int64_t ldxb,
                  const double* yb, const double* wb, int64_t nb, const uint8_t* counts_b, int32_t n_reps, double* rows,
                  uint8_t* ok) {
  if (!rows || !ok) return ob::fail(OB_E_INVALID, "null pointer");
  Limits L;
  OB_TRY(limits_from(tc, L));
  OB_TRY(ob::tb_piece_check("ob_tobit_rows", xa, ldxa, ya, wa, na, k, L));
  OB_TRY(ob::tb_piece_check("ob_tobit_rows", xb, ldxb, yb, wb, nb, k, L));
  if (reference_coeffs != OB_REF_GROUP_A && reference_coeffs != OB_REF_GROUP_B)
    return ob::model_refuse(ob::kModelTobit, "reference coefficients other than GroupA and GroupB are");
  if ((counts_a == nullptr) != (counts_b == nullptr)) return ob::fail(OB_E_INVALID, "ob_tobit_rows: counts for one group only");
  if (n_reps < 1 || n_reps > OB_TOBIT_MAX_ARRAY_REPS || (!counts_a && n_reps != 1))
    return ob::fail(OB_E_INVALID, "ob_tobit_rows takes 1 to %d replicates (1 without counts), got %d", OB_TOBIT_MAX_ARRAY_REPS, n_reps);
  const int D = k + 1, rl = ob::tobit_row_len(k);
  std::vector<double> start((size_t)2 * D, 0.0);
  if (!ols_start(xa, ldxa, ya, wa, na, k, start.data()) || !ols_start(xb, ldxb, yb, wb, nb, k, start.data() + D))
    return ob::fail(OB_E_LINALG, "%sob_tobit_rows: the least-squares start failed", ob::error_prefix(OB_E_LINALG));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  ob::TbArrays A;
  const ob::TbGroup gr[2] = {{xa, ya, wa, ldxa, na, counts_a, na}, {xb, yb, wb, ldxb, nb, counts_b, nb}};
  OB_TRY(ob::tb_arrays(ctx, k, L, gr, counts_a != nullptr, (uint32_t)n_reps, A));
  hipStream_t s = ctx->stream;
  OB_HIP(A.start.alloc(sizeof(double) * 2 * D));
  OB_HIP(hipMemcpyAsync(A.start.p, start.data(), sizeof(double) * 2 * D, hipMemcpyHostToDevice, s));
  OB_HIP(A.rows.alloc(sizeof(double) * (size_t)n_reps * rl));
  OB_HIP(A.ok.alloc((size_t)n_reps));
  A.h.rows = A.rows.d();
  A.h.ok = A.ok.as<uint8_t>();
  A.h.row_len = rl;
  A.h.ref = reference_coeffs;
  g_timing = {};
  OB_TRY(tb_batch(A.h, A.start.d(), s));
  OB_HIP(hipMemcpyAsync(rows, A.rows.p, sizeof(double) * (size_t)n_reps * rl, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(ok, A.ok.p, (size_t)n_reps, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  return OB_OK;
}

}  // extern "C"
