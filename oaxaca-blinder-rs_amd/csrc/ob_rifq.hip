// ob_rifq.hip -- the RIF of a quantile refitted on a resample, without a sort per replicate.
//
// A group's rows stand in stable ascending order of y; a replicate is its OBRS-3 counts c_i over those rows (the
// engine's level-1 tile counts and level-2 count images). The RIF of quantile tau on the expanded resample
// (rif.rs:14-88) takes two values, A - B [y_i <= q], so its regression needs only
//   rifq_search_kernel    block per (replicate, group): the order statistics Y(k) of the resample at the ranks of
//                         every tau and of the two quartiles (a scan of the tile counts, then of the one tile's 256
//                         u8 counts), q_t, p_t = upper_bound(y, q_t), the centred mean / sd and the bandwidth;
//   rifq_density_kernel   block per (row chunk, 16 replicates), the hot pass, in the shape of
//                         ob_binary_means_kernel: sum c phi((q_t - y) / bw) for every tau and sum c v_a over
//                         v = [1, x], the columns staged once per 64-row sub-tile and shared by replicates and taus;
//   rifq_patch_kernel     wave per (replicate, group, tau): the chunk partials in chunk order, the masked sums
//                         T_a = sum_{i < p_t} c_i v_ia (whole chunks from the density pass's totals, the one chunk
//                         that p_t cuts row by row), f, A, B and the y-pairs of the extended Gram.
// The point pass is the same code with every row counted once (counts == NULL). No floating-point atomics: every
// sum has an order fixed by the group's size, so a replicate's values have the same bytes alone, in any batch and
// among any other taus.
//
// q must equal the reference's bitwise (the indicator then never depends on a rounding), so nothing in this file
// contracts a multiply and an add into an FMA.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ob_builder.hpp"
#include "ob_cluster.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_model.hpp"
#include "ob_rifq.hpp"
#include "ob_spec.h"

namespace {

constexpr int kQB = 256;     // threads of a search or density block
constexpr int kQS = 65;      // doubles per staged column
constexpr int kQReps = 16;   // replicates per density block
constexpr int kQVals = 40;   // per-thread sums (kRifqMaxTaus + kRifqMaxK), whole rounds of kQRound
constexpr int kQRound = 8;   // sums reduced per round of the block's final ordered sum
constexpr int kQRanks = 2 * ob::kRifqMaxTaus + 2;
static_assert(kQVals == ob::kRifqMaxTaus + ob::kRifqMaxK && kQVals % kQRound == 0, "sum slots");

using ob::RifqArgs;  // ob_rifq.hpp

// c of sorted position `row` of group g in replicate rep.
__device__ __forceinline__ uint32_t rifq_count(const RifqArgs& a, int g, uint32_t rep, uint32_t row) {
  if (!a.counts) return 1u;
  const uint32_t tile = a.tile0[g] + (row >> OB_TILE_SHIFT), within = row & (OB_TILE_ROWS - 1u);
  const uint32_t sw = within >> 6, qq = within & 63u;
  const uint32_t word = a.counts[(((size_t)tile * a.nb_rep + (rep >> 6)) * 4 + sw) * kCimgWords +
                                 (rep & 63u) * kCimgStride + (qq >> 2)];
  return (word >> (8 * (qq & 3u))) & 255u;
}

// Y(k): the y of the first sorted position whose inclusive count prefix exceeds k.
__device__ double rifq_order_stat(const RifqArgs& a, int g, uint32_t rep, uint32_t k) {
  const double* y = a.cols[g];
  const uint32_t n = a.n[g];
  if (!a.counts) return y[min(k, n - 1u)];
  const uint32_t ntiles = (n + OB_TILE_ROWS - 1u) >> OB_TILE_SHIFT;
  const uint32_t* m1 = a.m1 + (size_t)rep * a.tiles_total + a.tile0[g];
  uint32_t cum = 0, tile = 0;
  for (; tile + 1 < ntiles; ++tile) {
    const uint32_t m = m1[tile];
    if (cum + m > k) break;
    cum += m;
  }
  const uint32_t r0 = tile << OB_TILE_SHIFT, r1 = min(n, r0 + OB_TILE_ROWS);
  for (uint32_t row = r0; row < r1; ++row) {
    cum += rifq_count(a, g, rep, row);
    if (cum > k) return y[row];
  }
  return y[n - 1u];  // counts that sum below n (refused by every caller)
}

__global__ __launch_bounds__(kQB) void rifq_search_kernel(const RifqArgs a) {
  __shared__ double red[2][kQB];
  __shared__ double yv[kQRanks];
  const int tid = threadIdx.x, g = blockIdx.y, T = a.n_taus;
  const uint32_t rep = blockIdx.x, n = a.n[g];
  const double* y = a.cols[g];
  const double mu0 = a.mu0[g], nf = (double)n;
  // spread sums about the original mean: thread t owns row t of every tile, the block adds in a fixed tree
  double s1 = 0.0, s2 = 0.0;
  for (uint32_t row = tid; row < n; row += kQB) {
    const uint32_t c = rifq_count(a, g, rep, row);
    if (c) {
      const double d = y[row] - mu0, cd = (double)c * d;
      s1 += cd;
      s2 += cd * d;
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  for (int w = kQB / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
    }
    __syncthreads();
  }
  // ranks: floor(h_t), ceil(h_t) of every tau, then the quartiles ceil(p n) - 1
  if (tid < 2 * T + 2) {
    uint32_t k;
    if (tid < 2 * T) {
      const double h = (nf - 1.0) * a.taus[tid >> 1];
      k = (uint32_t)((tid & 1) ? ceil(h) : floor(h));
    } else {
      const double c = ceil((tid == 2 * T ? 0.25 : 0.75) * nf);
      k = c < 1.0 ? 0u : (uint32_t)c - 1u;
    }
    yv[tid] = rifq_order_stat(a, g, rep, min(k, n - 1u));
  }
  __syncthreads();
  const size_t rg = (size_t)rep * a.n_groups + g;
  if (tid < T) {
    const double h = (nf - 1.0) * a.taus[tid], hf = floor(h), frac = h - hf;
    const double y0 = yv[2 * tid], y1 = yv[2 * tid + 1];
    const double q = hf == ceil(h) ? y0 : y0 + frac * (y1 - y0);
    uint32_t lo = 0, hi = n;  // p = upper_bound(y, q)
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (y[mid] <= q) lo = mid + 1u;
      else hi = mid;
    }
    a.sq[rg * T + tid] = q;
    a.sp[rg * T + tid] = lo;
  }
  if (tid == 0) {
    const double S1 = red[0][0], S2 = red[1][0];
    const double mean = mu0 + S1 / nf;
    double var = (S2 - S1 * S1 / nf) / (nf - 1.0);
    if (!(var > 0.0)) var = 0.0;
    const double sd = sqrt(var), iqr = yv[2 * T + 1] - yv[2 * T];
    double spread = iqr > 1e-8 ? fmin(sd, iqr / 1.34) : sd;
    if (spread < 1e-8) spread = 1.0;
    a.sbw[rg * 3] = 0.9 * spread * a.npow[g];
    a.sbw[rg * 3 + 1] = mean;
    a.sbw[rg * 3 + 2] = sd;
  }
}

// Block = (row chunk, 16 replicates), 4 waves; thread = (replicate t & 15, rows 4 (t >> 4) .. + 3 of each 64-row
// sub-tile: one count word). Per sub-tile the block stages the k columns once (LDS [col][65]); a counted row adds
// c phi((q_t - y) / bw) for every tau and c v_a into registers. A thread owns its rows over the whole chunk; at the
// end the 16 row groups of a replicate are added in row-group order through LDS, so a replicate's partials depend
// on the chunk and on the replicate alone.
__global__ __launch_bounds__(kQB) void rifq_density_kernel(const RifqArgs a) {
  extern __shared__ __attribute__((aligned(16))) double qsm[];
  const int tid = threadIdx.x, k = a.k, T = a.n_taus, nv = ob::kRifqMaxTaus + k;
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  double* stg = qsm;                               // [k][kQS]
  double* qs = stg + k * kQS;                      // [16][kRifqMaxTaus + 1]: q_t, then 1 / bw
  double* red = qs + kQReps * (ob::kRifqMaxTaus + 1);  // [kQRound][16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep0 = blockIdx.y * kQReps, rep = rep0 + r16;
  const bool act = rep < a.n_reps;
  if (tid < kQReps * (ob::kRifqMaxTaus + 1)) {
    const int rr = tid / (ob::kRifqMaxTaus + 1), j = tid - rr * (ob::kRifqMaxTaus + 1);
    const size_t rg = (size_t)(rep0 + rr) * a.n_groups + g;
    double v = 0.0;
    if (rep0 + rr < a.n_reps) v = j < T ? a.sq[rg * T + j] : (j == ob::kRifqMaxTaus ? a.sbw[rg * 3] : 0.0);
    qs[tid] = v;
  }
  double dens[ob::kRifqMaxTaus], xs[ob::kRifqMaxK];
#pragma unroll
  for (int t = 0; t < ob::kRifqMaxTaus; ++t) dens[t] = 0.0;
#pragma unroll
  for (int j = 0; j < ob::kRifqMaxK; ++j) xs[j] = 0.0;
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const double* myq = qs + r16 * (ob::kRifqMaxTaus + 1);
  const double inv_sqrt_2pi = 1.0 / sqrt(2.0 * 3.14159265358979323846);
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's reads (and the quantile loads)
      for (int i = tid; i < k * 64; i += kQB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kQS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      uint32_t word = 0;
      if (act) {
        if (!a.counts)
          word = 0x01010101u;
        else
          word = a.counts[((((size_t)a.tile0[g] + tile) * a.nb_rep + (rep >> 6)) * 4 + sw) * kCimgWords +
                          (rep & 63u) * kCimgStride + q];
      }
      double cd[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) cd[i] = (uint32_t)(4 * q + i) < nr ? (double)((word >> (8 * i)) & 255u) : 0.0;
      if (cd[0] + cd[1] + cd[2] + cd[3] == 0.0) continue;  // (uniform control flow resumes at the barrier)
      xs[0] += cd[0] + cd[1] + cd[2] + cd[3];
#pragma unroll
      for (int j = 1; j < ob::kRifqMaxK; ++j)
        if (j < k) {
          const double* zj = stg + j * kQS + 4 * q;
#pragma unroll
          for (int i = 0; i < 4; ++i) xs[j] += cd[i] * zj[i];
        }
      const double bw = myq[ob::kRifqMaxTaus];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (cd[i] == 0.0) continue;
        const double yi = stg[4 * q + i];
#pragma unroll
        for (int t = 0; t < ob::kRifqMaxTaus; ++t)
          if (t < T) {
            const double u = (myq[t] - yi) / bw, e = -0.5 * (u * u);
            if (e > -746.0) dens[t] += cd[i] * (inv_sqrt_2pi * exp(e));  // below: exp underflows to exactly 0
          }
      }
    }
  }
  // slots: [0, kRifqMaxTaus) the density sums, then c v_0 = c, c v_1 ..
  double vals[kQVals];
#pragma unroll
  for (int t = 0; t < ob::kRifqMaxTaus; ++t) vals[t] = dens[t];
#pragma unroll
  for (int j = 0; j < ob::kRifqMaxK; ++j) vals[ob::kRifqMaxTaus + j] = xs[j];
  double* out = a.partial + (size_t)chunk * a.part_pad * nv;
#pragma unroll
  for (int rd = 0; rd < kQVals / kQRound; ++rd) {
    if (rd * kQRound >= nv) break;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kQRound; ++i) red[(i * 16 + q) * kQReps + r16] = vals[rd * kQRound + i];
    __syncthreads();
    if (tid < kQRound * kQReps) {
      const int vi = tid >> 4, slot = rd * kQRound + vi;
      double v = 0.0;
      for (int qq = 0; qq < 16; ++qq) v += red[(vi * 16 + qq) * kQReps + r16];
      if (slot < nv && act) out[(size_t)rep * nv + slot] = v;
    }
  }
}

inline size_t density_lds(int k) {
  return sizeof(double) * ((size_t)k * kQS + (size_t)kQReps * (ob::kRifqMaxTaus + 1) + (size_t)kQRound * 16 * kQReps);
}

// One wave per (replicate, group, tau).
__global__ __launch_bounds__(64) void rifq_patch_kernel(const RifqArgs a) {
  __shared__ double sh[ob::kRifqMaxK];
  const int lane = threadIdx.x, k = a.k, T = a.n_taus, nv = ob::kRifqMaxTaus + k;
  const uint32_t rep = blockIdx.x;
  const int g = blockIdx.y / T, t = blockIdx.y - g * T;
  const size_t rg = (size_t)rep * a.n_groups + g;
  const uint32_t n = a.n[g], p = a.sp[rg * T + t];
  // chunk order: lane a < k carries column a's total S_a and the whole chunks below p; lane k the density sum
  double S = 0.0, Tw = 0.0;
  uint32_t cut0 = 0, cut1 = 0;  // rows [cut0, cut1): the part below p of the chunk that p cuts
  for (int c = 0; c < a.n_chunks; ++c) {
    if (a.chunks[3 * c] != (uint32_t)g) continue;
    const uint32_t r0 = a.chunks[3 * c + 1] * OB_TILE_ROWS, r1 = min(n, a.chunks[3 * c + 2] * OB_TILE_ROWS);
    const double* part = a.partial + ((size_t)c * a.part_pad + rep) * nv;
    if (lane < k) {
      const double v = part[ob::kRifqMaxTaus + lane];
      S += v;
      if (r1 <= p) Tw += v;
    } else if (lane == k) {
      S += part[t];
    }
    if (r0 < p && p < r1) {
      cut0 = r0;
      cut1 = p;
    }
  }
  double acc[ob::kRifqMaxK];
#pragma unroll
  for (int j = 0; j < ob::kRifqMaxK; ++j) acc[j] = 0.0;
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  for (uint32_t row = cut0 + lane; row < cut1; row += 64) {
    const uint32_t c = rifq_count(a, g, rep, row);
    if (!c) continue;
    const double cd = (double)c;
    acc[0] += cd;
#pragma unroll
    for (int j = 1; j < ob::kRifqMaxK; ++j)
      if (j < k) acc[j] += cd * X[(size_t)j * ld + row];
  }
#pragma unroll
  for (int j = 0; j < ob::kRifqMaxK; ++j)
    if (j < k) {
      double v = acc[j];
      for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
      if (lane == 0) sh[j] = v;
    }
  __syncthreads();
  const double D = __shfl(S, k, 64);  // k <= 32 < 64
  const double q = a.sq[rg * T + t], bw = a.sbw[rg * 3], nf = (double)n, tau = a.taus[t];
  double f = D / (nf * bw);
  const bool floored = f < 1e-8;
  if (floored) f = 1e-8;
  const double B = 1.0 / f, A = q + tau * B;
  const size_t o = rg * T + t;
  const double Ta = lane < k ? Tw + sh[lane] : 0.0;
  const double nle = __shfl(Ta, 0, 64);
  if (lane < k) {
    a.ot[o * k + lane] = Ta;
    if (a.ogy) a.ogy[o * (k + 1) + lane] = A * S - B * Ta;
  }
  if (lane == 0) {
    a.of[o] = f;
    a.onle[o] = nle;
    a.ofl[o] = floored ? 1 : 0;
    if (a.ogy) a.ogy[o * (k + 1) + k] = A * A * nf - (2.0 * A * B - B * B) * nle;
  }
}

// Writes tau t's y-pairs over those of the reduced extended Grams [rep][2][e_pad] of v = [1, x, y] (k1 = k + 1).
__global__ __launch_bounds__(256) void rifq_store_kernel(const RifqArgs a, int t, double* gram, int e_pad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, per = 2u * (uint32_t)(a.k + 1);
  if (i >= a.n_reps * per) return;
  const uint32_t rep = i / per, rem = i - rep * per, g = rem / (a.k + 1), j = rem - g * (a.k + 1);
  const size_t o = ((size_t)rep * 2 + g) * a.n_taus + t;
  gram[((size_t)rep * 2 + g) * e_pad + ob_pair_index((int)j, a.k, a.k + 1)] = a.ogy[o * (a.k + 1) + j];
}

// The solved OLS rows [rep][rl0] of tau t into the caller's rows [rep][rl0 + 6], with the tail q_A, q_B, f_A, f_B,
// N_le,A, N_le,B.
__global__ __launch_bounds__(64) void rifq_tail_kernel(const RifqArgs a, int t, const double* solved, const uint8_t* sok,
                                                       int rl0, double* rows, uint8_t* ok) {
  const uint32_t rep = blockIdx.x;
  double* row = rows + (size_t)rep * (rl0 + 6);
  for (int i = threadIdx.x; i < rl0; i += 64) row[i] = solved[(size_t)rep * rl0 + i];
  if (threadIdx.x < 2) {
    const size_t o = ((size_t)rep * 2 + threadIdx.x) * a.n_taus + t;
    row[rl0 + threadIdx.x] = a.sq[o];
    row[rl0 + 2 + threadIdx.x] = a.of[o];
    row[rl0 + 4 + threadIdx.x] = a.onle[o];
  }
  if (threadIdx.x == 0) ok[rep] = sok[rep];
}

thread_local ob_rifq_timing g_timing = {};

// The three kernels over the replicates of `a` (every buffer set), enqueued; e[0] .. e[3] are recorded before the
// search and after each kernel. rifq_times adds their ms once the stream has reached e[3].
int rifq_launch(const RifqArgs& a, hipStream_t s, hipEvent_t* e) {
  OB_HIP(hipEventRecord(e[0], s));
  hipLaunchKernelGGL(rifq_search_kernel, dim3(a.n_reps, a.n_groups), dim3(kQB), 0, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(e[1], s));
  const size_t lds = density_lds(a.k);
  OB_HIP(hipFuncSetAttribute((const void*)rifq_density_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(rifq_density_kernel, dim3(a.n_chunks, (a.n_reps + kQReps - 1) / kQReps), dim3(kQB), lds, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(e[2], s));
  hipLaunchKernelGGL(rifq_patch_kernel, dim3(a.n_reps, a.n_groups * a.n_taus), dim3(64), 0, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(e[3], s));
  return OB_OK;
}

int rifq_times(hipEvent_t* e) {
  float m[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < 3; ++i) OB_HIP(hipEventElapsedTime(&m[i], e[i], e[i + 1]));
  g_timing.search_ms += m[0];
  g_timing.density_ms += m[1];
  g_timing.patch_ms += m[2];
  return OB_OK;
}

}  // namespace

namespace ob {

// ob_rifs.hip runs the same kernels for its quantile ranges.
int rifq_run(const RifqArgs& a, hipStream_t s, hipEvent_t* e) { return rifq_launch(a, s, e); }

int rifq_store(const double* gy, int k, uint32_t n_reps, int n_out, int t, double* gram, int e_pad, hipStream_t s) {
  RifqArgs a{};  // rifq_store_kernel reads these four
  a.k = k;
  a.n_reps = n_reps;
  a.n_taus = n_out;
  a.ogy = const_cast<double*>(gy);
  hipLaunchKernelGGL(rifq_store_kernel, dim3(blocks_for((int64_t)n_reps * 2 * (k + 1))), dim3(256), 0, s, a, t, gram, e_pad);
  OB_HIP(hipGetLastError());
  return OB_OK;
}

int rifq_check_taus(const double* taus, int n_taus) {
  if (!taus || n_taus < 1) return fail(OB_E_INVALID, "quantile refit: no quantiles");
  if (n_taus > kRifqMaxTaus)
    return fail(OB_E_UNSUPPORTED, "quantile refit: at most %d quantiles a pass, got %d", kRifqMaxTaus, n_taus);
  for (int t = 0; t < n_taus; ++t) {
    if (!(taus[t] > 0.0 && taus[t] < 1.0)) return fail(OB_E_INVALID, "quantile refit: tau must lie in (0, 1), got %g", taus[t]);
    if (t && !(taus[t] > taus[t - 1])) return fail(OB_E_INVALID, "quantile refit: the quantiles must be strictly increasing");
  }
  return OB_OK;
}

int rifq_check_shape(int k, int n_taus, const double* taus, int64_t n_a, int64_t n_b) {
  if (k < 1 || n_a < 0 || n_b < 0)
    return fail(OB_E_INVALID, "quantile refit: bad shape (k = %d, n_a = %lld, n_b = %lld)", k, (long long)n_a, (long long)n_b);
  if (k > kRifqMaxK)
    return fail(OB_E_UNSUPPORTED, "quantile refit: at most %d design columns with the intercept, got %d", kRifqMaxK, k);
  OB_TRY(rifq_check_taus(taus, n_taus));
  if (n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31))
    return fail(OB_E_UNSUPPORTED, "quantile refit: groups take fewer than 2^31 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k || n < 2)
      return fail(OB_E_INSUFFICIENT, "quantile refit: a group's rows (%lld) must exceed the design columns (%d) and be at least 2",
                  (long long)n, k);
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_rifq_row_len(int32_t k, int32_t n_base) { return k < 1 || n_base < 0 ? 0 : ob_row_len(k, n_base) + 6; }

int ob_rifq_check_shape(int32_t k, int32_t n_taus, const double* taus, int64_t n_a, int64_t n_b) {
  return ob::rifq_check_shape(k, n_taus, taus, n_a, n_b);
}

int ob_rifq_last_timing(ob_rifq_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

// The three kernels over one group whose rows the caller sorted (include/oaxaca_boot.h).
int ob_rifq_pass(ob_ctx* ctx, const double* y_sorted, int64_t n, const uint8_t* counts, int32_t n_reps,
                 const double* taus, int32_t n_taus, const double* x, int64_t ldx, int32_t p, double* q, double* bw,
                 double* f, double* n_le, double* t, double* gy, uint8_t* floored) {
  if (!y_sorted || !q || !bw || !f || !n_le || !t) return ob::fail(OB_E_INVALID, "null pointer");
  if (p < 0 || (p > 0 && !x)) return ob::fail(OB_E_INVALID, "ob_rifq_pass: p = %d predictor columns need x", p);
  const int k = p + 1;
  if (k > ob::kRifqMaxK)
    return ob::fail(OB_E_UNSUPPORTED, "ob_rifq_pass: at most %d design columns with the intercept, got %d", ob::kRifqMaxK, k);
  OB_TRY(ob::rifq_check_taus(taus, n_taus));
  // the order of the shared checks differs from ob_rifs_pass in this one place: the rows before the replicates
  if (n < 2) return ob::fail(OB_E_INSUFFICIENT, "ob_rifq_pass needs at least 2 rows, got %lld", (long long)n);
  if (n >= ((int64_t)1 << 31)) return ob::fail(OB_E_UNSUPPORTED, "ob_rifq_pass takes fewer than 2^31 rows");
  if (p > 0 && ldx < n) return ob::fail(OB_E_INVALID, "ob_rifq_pass: ldx = %lld is below n = %lld", (long long)ldx, (long long)n);
  if (n_reps < 1 || n_reps > 16384) return ob::fail(OB_E_INVALID, "ob_rifq_pass takes 1 to 16384 replicates, got %d", n_reps);
  OB_TRY(ob::refit_pass_check("ob_rifq_pass", y_sorted, n, counts, n_reps, x, ldx, p, false));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  ob::RefitPassInput in;
  OB_TRY(in.upload(y_sorted, n, counts, n_reps, x, ldx, k, s));
  const int T = n_taus, nv = ob::rifq_sums_len(k);
  DevBuf d_partial, d_sq, d_sp, d_sbw, d_f, d_nle, d_fl, d_t, d_gy;
  OB_HIP(d_partial.alloc(sizeof(double) * (size_t)in.n_chunks * in.rep_pad * nv));
  const size_t nrt = (size_t)n_reps * T;
  OB_HIP(d_sq.alloc(sizeof(double) * nrt));
  OB_HIP(d_sp.alloc(sizeof(uint32_t) * nrt));
  OB_HIP(d_sbw.alloc(sizeof(double) * 3 * (size_t)n_reps));
  OB_HIP(d_f.alloc(sizeof(double) * nrt));
  OB_HIP(d_nle.alloc(sizeof(double) * nrt));
  OB_HIP(d_fl.alloc(nrt));
  OB_HIP(d_t.alloc(sizeof(double) * nrt * k));
  OB_HIP(d_gy.alloc(sizeof(double) * nrt * (k + 1)));
  RifqArgs a{};
  a.cols[0] = in.cols.d();
  a.ld[0] = in.ld;
  a.n[0] = (uint32_t)n;
  a.tile0[0] = 0;
  a.mu0[0] = in.mu0;
  a.npow[0] = std::pow((double)n, -0.2);
  for (int i = 0; i < T; ++i) a.taus[i] = taus[i];
  a.k = k;
  a.n_taus = T;
  a.n_groups = 1;
  a.tiles_total = in.tiles;
  a.m1 = counts ? in.m1.as<uint32_t>() : nullptr;
  a.counts = counts ? in.counts.as<uint32_t>() : nullptr;
  a.nb_rep = in.nb_rep;
  a.part_pad = in.rep_pad;
  a.n_reps = (uint32_t)n_reps;
  a.chunks = in.chunks.as<uint32_t>();
  a.n_chunks = (int)in.n_chunks;
  a.sq = d_sq.d();
  a.sp = d_sp.as<uint32_t>();
  a.sbw = d_sbw.d();
  a.partial = d_partial.d();
  a.of = d_f.d();
  a.onle = d_nle.d();
  a.ofl = d_fl.as<uint8_t>();
  a.ot = d_t.d();
  a.ogy = d_gy.d();
  g_timing = {};
  Events<4> ev;
  OB_HIP(ev.create());
  OB_TRY(rifq_launch(a, s, ev.e));
  OB_HIP(hipEventSynchronize(ev.e[3]));
  OB_TRY(rifq_times(ev.e));
  std::vector<double> sbw(3 * (size_t)n_reps);
  std::vector<uint8_t> fl(nrt);
  OB_HIP(hipMemcpyAsync(q, d_sq.p, sizeof(double) * nrt, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(sbw.data(), d_sbw.p, sizeof(double) * sbw.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(f, d_f.p, sizeof(double) * nrt, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(n_le, d_nle.p, sizeof(double) * nrt, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(t, d_t.p, sizeof(double) * nrt * k, hipMemcpyDeviceToHost, s));
  if (gy) OB_HIP(hipMemcpyAsync(gy, d_gy.p, sizeof(double) * nrt * (k + 1), hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(fl.data(), d_fl.p, nrt, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  for (int32_t r = 0; r < n_reps; ++r) bw[r] = sbw[3 * (size_t)r];
  if (floored) std::memcpy(floored, fl.data(), nrt);
  return OB_OK;
}

}  // extern "C"

namespace ob {

// Device side of a prepared refit run. The handle's ob_panel holds the groups' rows in stable ascending order of y
// (x_1 .. x_p, then y): it is the resampler and the owner of the Gram, the chunk table and the solve.
struct RifqState {
  int k = 0, n_taus = 0;
  double taus[kRifqMaxTaus] = {};
  DevBuf cols[2];  // [y | x_1 .. x_{k-1}] x ld
  DevBuf sq, sp, sbw, partial, of, onle, ofl, ot, ogy, solved, sok;
  SortedGroups sorted;                   // perm, mu0, npow (x and y are dropped once uploaded)
  std::vector<double> point_q, point_f;  // [2][T]
  int64_t n_floored = 0;                 // floored densities of the point pass and of every boot since
};

static RifqState* rifq_state(const ob_prepared* pr) { return model_state<RifqState>(pr, kModelRifq); }

// One segment (refit_segment) with the three refit kernels and rifq_tail_kernel.
static int rifq_segment(ob_prepared* pr, const RefitSegment& sg, hipStream_t s) {
  RifqState* st = rifq_state(pr);
  ob_panel* p = pr->panel;
  const int k = st->k, T = st->n_taus, rl0 = p->row_len;
  Events<4> ev;
  OB_HIP(ev.create());
  RifqArgs a{};
  RefitModel md{T, &st->solved, &st->sok, &st->n_floored, nullptr, nullptr};
  md.launch = [&](uint32_t nb_rep, uint32_t rep_pad, RefitOut* out) -> int {
    const int n_chunks = (int)(p->chunks.size() / 3);
    const size_t nrt = (size_t)rep_pad * 2 * T;
    OB_HIP(st->sq.alloc(sizeof(double) * nrt));
    OB_HIP(st->sp.alloc(sizeof(uint32_t) * nrt));
    OB_HIP(st->sbw.alloc(sizeof(double) * 3 * 2 * rep_pad));
    OB_HIP(st->partial.alloc(sizeof(double) * (size_t)n_chunks * rep_pad * rifq_sums_len(k)));
    OB_HIP(st->of.alloc(sizeof(double) * nrt));
    OB_HIP(st->onle.alloc(sizeof(double) * nrt));
    OB_HIP(st->ofl.alloc(nrt));
    OB_HIP(st->ot.alloc(sizeof(double) * nrt * k));
    OB_HIP(st->ogy.alloc(sizeof(double) * nrt * (k + 1)));
    for (int g = 0; g < 2; ++g) {
      a.cols[g] = st->cols[g].d();
      a.ld[g] = p->ld[g];
      a.n[g] = p->n[g];
      a.mu0[g] = st->sorted.mu0[g];
      a.npow[g] = st->sorted.npow[g];
    }
    a.tile0[0] = 0;
    a.tile0[1] = p->ntiles[0];
    for (int t = 0; t < T; ++t) a.taus[t] = st->taus[t];
    a.k = k;
    a.n_taus = T;
    a.n_groups = 2;
    a.tiles_total = p->ntiles[0] + p->ntiles[1];
    a.m1 = p->d_m1;
    a.counts = p->d_counts;
    a.nb_rep = nb_rep;
    a.part_pad = rep_pad;
    a.n_reps = sg.ns;
    a.chunks = p->d_chunks;
    a.n_chunks = n_chunks;
    a.sq = st->sq.d();
    a.sp = st->sp.as<uint32_t>();
    a.sbw = st->sbw.d();
    a.partial = st->partial.d();
    a.of = st->of.d();
    a.onle = st->onle.d();
    a.ofl = st->ofl.as<uint8_t>();
    a.ot = st->ot.d();
    a.ogy = st->ogy.d();
    *out = {a.ogy, a.ofl};
    return rifq_launch(a, s, ev.e);
  };
  md.tail = [&](int t, const double* solved, const uint8_t* sok, double* rows, uint8_t* ok) {
    hipLaunchKernelGGL(rifq_tail_kernel, dim3(sg.ns), dim3(64), 0, s, a, t, solved, sok, rl0, rows, ok);
  };
  RefitTimes tm;
  OB_TRY(refit_segment(pr, sg, md, s, &tm));
  g_timing.gram_ms += tm.gram_ms;
  g_timing.solve_ms += tm.solve_ms;
  return rifq_times(ev.e);
}

static int rifq_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                            hipStream_t stream) {
  const BootPlan plan{kRefitSegReps, kCountBudget, false, [](uint32_t) {
                        g_timing = {};
                        return OB_OK;
                      }};
  return boot_segmented(pr, kModelRifq, plan, first_rep, n_reps, d_rows && d_ok, stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t, uint32_t, hipStream_t s) {
                          return rifq_segment(pr, {false, first_rep + s0, ns, n_reps, s0, d_rows, d_ok}, s);
                        });
}

static const bool g_rifq_hooks_installed = model_install(
    kModelRifq, {rifq_boot_device, model_boot_host, [](void* s) { delete static_cast<RifqState*>(s); }});

// Every check of the frame entry points, before any device work and before the context is read.
static int rifq_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const double* taus, int32_t n_taus, Config& c, Matrices& m) {
  OB_TRY(config_from(cfg, c));
  OB_TRY(rifq_check_taus(taus, n_taus));
  if (c.has_weights) return model_refuse(kModelRifq, "sample weights are");
  if (!c.normalize.empty()) return model_refuse(kModelRifq, "normalized categoricals are");
  if (c.has_selection || !c.selection_predictors.empty()) return model_refuse(kModelRifq, "Heckman selection settings are");
  if (c.has_cluster) return model_refuse(kModelRifq, "a cluster bootstrap is");
  OB_TRY(stage_named(cols, n_cols, n_rows, c, kModelRifq, false, false));
  OB_TRY(m.load(cols, n_cols, n_rows, cfg, false));
  OB_TRY(rifq_check_shape(m.k, n_taus, taus, m.n[0], m.n[1]));
  for (int g = 0; g < 2; ++g) {
    for (int64_t i = 0; i < m.n[g]; ++i)
      if (!std::isfinite(m.y[g][i])) return fail(OB_E_INVALID, "quantile refit: a non-finite value in the outcome");
    for (int64_t i = 0; i < m.n[g] * m.k; ++i)
      if (!std::isfinite(m.x[g][i])) return fail(OB_E_INVALID, "quantile refit: a non-finite value in a predictor");
  }
  return OB_OK;
}

static int rifq_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                        const double* taus, int32_t n_taus, ob_prepared** out) {
  Config c;
  Matrices m;
  OB_TRY(rifq_stage(cols, n_cols, n_rows, cfg, taus, n_taus, c, m));
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  const int k = m.k;
  RifqState* st = new RifqState();
  ob_prepared* pr = model_handle(ctx, c, m, kModelRifq, st, ob_row_len(k, 0) + 6, n_taus);
  st->k = k;
  st->n_taus = n_taus;
  for (int t = 0; t < n_taus; ++t) st->taus[t] = taus[t];
  SortedGroups& sg = st->sorted;
  sort_groups(m, sg);
  auto build = [&]() -> int {
    OB_TRY(refit_panel(ctx, c, m, sg, &pr->panel));
    for (int g = 0; g < 2; ++g)
      OB_TRY(upload_group(st->cols[g], pr->panel->ld[g], m.n[g], k, 0, sg.y[g].data(), sg.x[g].data()));
    // the point pass: the boot's own kernels over unit counts
    g_timing = {};
    OB_TRY(refit_point(pr, [&](double* d_rows, uint8_t* d_ok, hipStream_t s) {
      return rifq_segment(pr, {true, 0, 1, 1, 0, d_rows, d_ok}, s);
    }));
    const size_t T = (size_t)n_taus;
    const int rl0 = pr->row_len - 6;
    st->point_q.resize(2 * T);
    st->point_f.resize(2 * T);
    for (size_t t = 0; t < T; ++t)
      for (int g = 0; g < 2; ++g) {
        st->point_q[(size_t)g * T + t] = pr->point_row[t * pr->row_len + rl0 + g];
        st->point_f[(size_t)g * T + t] = pr->point_row[t * pr->row_len + rl0 + 2 + g];
      }
    return OB_OK;
  };
  const int rc = build();
  for (int g = 0; g < 2; ++g) {
    sg.x[g] = {};
    sg.y[g] = {};
  }
  return model_built(pr, rc, out);
}

}  // namespace ob

extern "C" {

int ob_builder_prepare_quantiles_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                       const ob_builder_config* cfg, const double* taus, int32_t n_taus,
                                       ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::rifq_prepare(ctx, cols, n_cols, n_rows, cfg, taus, n_taus, out);
}

int ob_builder_decompose_quantiles_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                         const ob_builder_config* cfg, const double* taus, int32_t n_taus,
                                         ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  for (int32_t t = 0; t < std::max(n_taus, 0) && t < ob::kRifqMaxTaus; ++t) out[t] = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::rifq_prepare(ctx, cols, n_cols, n_rows, cfg, taus, n_taus, &pr));
  const uint64_t reps = pr->cfg.reps;
  const size_t T = (size_t)n_taus;
  std::vector<double> rows(T * reps * pr->row_len);
  std::vector<uint8_t> ok(T * reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  for (size_t t = 0; t < T && rc == OB_OK; ++t)
    rc = ob::finish(pr, (int)t, rows.data() + t * reps * pr->row_len, ok.data() + t * reps, reps, &out[t]);
  if (rc != OB_OK)
    for (size_t t = 0; t < T; ++t) {
      ob_results_free(out[t]);
      out[t] = nullptr;
    }
  ob_prepared_destroy(pr);
  return rc;
}

int ob_prepared_rifq_info(const ob_prepared* prep, ob_rifq_info* out) {
  if (!prep || !out) return ob::fail(OB_E_INVALID, "null pointer");
  const ob::RifqState* st = ob::rifq_state(prep);
  if (!st) return ob::fail(OB_E_INVALID, "the handle was not prepared for a quantile refit");
  *out = {st->n_taus, st->k, prep->n_a, prep->n_b, st->n_floored, st->taus, st->sorted.perm[0].data(),
          st->sorted.perm[1].data(), st->point_q.data(), st->point_f.data()};
  return OB_OK;
}

int ob_prepared_finish_tau(ob_prepared* prep, int32_t t, const double* rows, const uint8_t* ok, uint64_t n_reps,
                           ob_results** out) {
  if (!prep || !out || (n_reps && (!rows || !ok))) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  if (prep->model_kind != ob::kModelRifq && prep->model_kind != ob::kModelRifs)
    return ob::fail(OB_E_INVALID, "the handle was not prepared for a quantile refit");
  // n_y: a quantile refit's taus, a statistics refit's statistics
  if (t < 0 || t >= prep->n_y) return ob::fail(OB_E_INVALID, "quantile index %d out of range", t);
  return ob::finish(prep, t, rows, ok, n_reps, out);
}

}  // extern "C"
