// ob_heckman.hip -- the Heckman two-step per replicate (builder .heckman_selection):
//   probit of s on [1, z] by Fisher scoring from 0 (math/probit.rs:25-170),
//   IMR lambda = phi/Phi on the selected rows, OLS of y on [1, x, lambda] over them
//   (heckman.rs:38-108, estimation.rs:114-260), beta* and the decomposition over K + 1 terms,
//   and the selection terms theta_ref delta_ref gamma_ref,j (zbar_A,j - zbar_B,j) (builder.rs:477-534).
//
// A replicate's resample enters through the same level-2 count images as the Gram kernel: every
// sum below is sum_i c_i f(row i). The selected-row normal matrix [X'X | X'y] is the engine's
// extended Gram with weights [s == 1]; only the IMR column needs per-replicate transcendental work.
//
// Kernels (one block per (row chunk, 64-replicate batch) unless noted; lane = replicate, wave =
// 64-row sub-tile of each 256-row tile, so a wave's panel reads are uniform and count reads are
// one word per 4 rows):
//   ob_probit_kernel<KS>      per iteration: sum c w z z', sum c lambda z (w, lambda per probit.rs)
//   ob_probit_step_kernel<KS> thread per (replicate, group): chunk sums in a fixed order, the
//                             nalgebra Cholesky step (LU fallback), convergence flag
//   ob_heck_sums_kernel<NB>   sum c lambda [1, x, y], c lambda^2, c lambda (lambda + z'gamma) over
//                             selected rows; sum c z, c w y, c w over all rows
//   ob_heck_solve_kernel      wave per replicate: [X'X, X'lambda; lambda'X, lambda'lambda] Cholesky,
//                             beta*, decomposition, selection terms
// Selection equations of more than 8 columns (ks = 9..32) run the probit pass and the sums on the
// f64 matrix units instead (ob_heck_wide_kernel, ob_probit_wide_step_kernel, further down).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "ob_device.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_normal.hpp"
#include "ob_heckman.hpp"
#include "ob_options.hpp"
#include "ob_pairpass.hpp"
#include "ob_spec.h"

namespace {

constexpr int kHB = 256;
constexpr uint32_t kDone = ob::kProbitDone, kFailed = ob::kProbitFailed;

// The probit and sums kernels take pdf and cdf from npdf_ncdf (one exp per row; probit launch 11.8
// -> 9.0 ms at configs[1] + selection, profiles/r04_ab_heckman_erfc.txt) unless option hk_erfc = 0
// (ob_set_option), which keeps the library's erfc beside a second exp.
inline bool hk_cody() { return ob::opt_int(ob::Opt::HkErfc, 1) != 0; }

// 1/v within ~1 ulp: v_rcp_f64 and two Newton steps instead of the IEEE division sequence (the
// operands are normal numbers: clamped probabilities).
__device__ __forceinline__ double hk_rcp(double v) {
  double r = __builtin_amdgcn_rcp(v);
  r = fma(fma(-v, r, 1.0), r, r);
  return fma(fma(-v, r, 1.0), r, r);
}

// f64::clamp: NaN stays NaN.
__device__ __forceinline__ double clamp_phi(double v) {
  return v < 1e-10 ? 1e-10 : (v > 1.0 - 1e-10 ? 1.0 - 1e-10 : v);
}

struct Lanes {
  uint32_t g, t0, t1, rep, rb;
  int wave, lane;
};

__device__ __forceinline__ Lanes lanes(const ob_heck_seg& a) {
  Lanes l;
  l.lane = threadIdx.x & 63;
  l.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x;
  l.rb = blockIdx.y;
  l.g = a.chunks[3 * chunk];
  l.t0 = a.chunks[3 * chunk + 1];
  l.t1 = a.chunks[3 * chunk + 2];
  l.rep = l.rb * 64 + l.lane;
  return l;
}

// This lane's count words for the wave's sub-tile of a tile (NULL: every row once). f64 Gram
// images: 16 consecutive words at lane * 17. I8 images (ob_count_kernel<true>, the A fragments of
// ob_gram_i8.hip: per sub-tile [16-replicate block][lane][16 B], lane = replicate 16 m + (l & 15),
// rows 16 (l >> 4) + j): the lane's rows 16 q .. 16 q + 15 are the 16-byte unit 16 q past the
// returned one (count_word).
__device__ __forceinline__ const uint32_t* count_row(const ob_heck_seg& a, const Lanes& l, uint32_t tile) {
  if (!a.counts) return nullptr;
  const size_t tt = (l.g ? a.tiles0 : 0u) + tile;
  if (a.counts_i8)
    return a.counts + ((tt * a.nb_rep + l.rb) * 1024 + l.wave * 256 + (l.lane >> 4) * 64 + (l.lane & 15)) * 4;
  return a.counts + ((tt * a.nb_rep + l.rb) * 4 + l.wave) * kCimgWords + l.lane * kCimgStride;
}

// Count bytes of the lane's rows ri .. ri + 3 of its sub-tile (ri % 4 == 0).
__device__ __forceinline__ uint32_t count_word(const ob_heck_seg& a, const uint32_t* cw, uint32_t ri) {
  if (!cw) return 0x01010101u;
  return a.counts_i8 ? cw[(ri >> 4) * 64 + ((ri >> 2) & 3u)] : cw[ri >> 2];
}

// Fixed-order block sum of acc over the 4 waves into LDS row `lane` (wave 3 + 2 + 1, then + 0).
template <int N>
__device__ __forceinline__ void block_sum(double (&acc)[N], double* red, const Lanes& l) {
#pragma unroll 1
  for (int w = 3; w >= 1; --w) {
    if (l.wave == w)
#pragma unroll
      for (int i = 0; i < N; ++i) red[l.lane * (N + 1) + i] = (w == 3 ? 0.0 : red[l.lane * (N + 1) + i]) + acc[i];
    __syncthreads();
  }
  if (l.wave == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = red[l.lane * (N + 1) + i] + acc[i];
}

// The wave's 64-row sub-tile of `ncol` consecutive panel columns (from `src`) -> LDS [col][64]: one
// coalesced load per column instead of a scalar load per row and column; the wave then reads its
// rows at uniform LDS addresses. Wave-local (LDS operations of one wave complete in order).
__device__ __forceinline__ void wave_stage(double* stg, const double* src, int64_t ld, uint32_t r0, uint32_t nr,
                                           int ncol, int lane) {
  __builtin_amdgcn_wave_barrier();
  for (int c = 0; c < ncol; ++c) stg[c * 64 + lane] = (uint32_t)lane < nr ? src[(size_t)c * ld + r0 + lane] : 0.0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int KS, bool CODY>
__global__ __launch_bounds__(kHB) void ob_probit_kernel(const ob_heck_seg a) {
  constexpr int NH = KS * (KS + 1) / 2, NP = NH + KS;
  __shared__ double red[64 * (NP + 1)];
  __shared__ double stage[4 * KS * 64];  // per wave: s, z_1..z_{KS-1} of its sub-tile
  const Lanes l = lanes(a);
  const size_t st = (size_t)l.g * a.rep_pad + l.rep;
  const bool act = l.rep < a.n_reps && !(a.hflags[st] & kDone);
  if (!__syncthreads_or(act)) return;
  double gam[KS];
#pragma unroll
  for (int j = 0; j < KS; ++j) gam[j] = act ? a.gamma[st * KS + j] : 0.0;
  double acc[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) acc[i] = 0.0;
  const double* X = a.cols[l.g];
  const int64_t ld = a.ld[l.g];
  const uint32_t n = a.n[l.g];
  const double* SZ = X + (size_t)a.sz_col * ld;  // s, then z_1..z_{KS-1}: consecutive columns
  double* stg = stage + l.wave * (KS * 64);
  for (uint32_t tile = l.t0; tile < l.t1; ++tile) {
    const uint32_t r0 = tile * OB_TILE_ROWS + l.wave * 64;
    if (r0 >= n) break;
    const uint32_t nr = min(64u, n - r0);
    wave_stage(stg, SZ, ld, r0, nr, KS, l.lane);
    const uint32_t* cw = count_row(a, l, tile);
    uint32_t word = 0;
    for (uint32_t ri = 0; ri < nr; ++ri) {
      if ((ri & 3) == 0) word = count_word(a, cw, ri);
      const uint32_t cu = (word >> ((ri & 3) * 8)) & 255u;
      if (!act || cu == 0) continue;
      const double c = (double)cu;
      double z[KS];
      z[0] = 1.0;
#pragma unroll
      for (int j = 1; j < KS; ++j) z[j] = stg[j * 64 + ri];
      double zg = 0.0;
#pragma unroll
      for (int j = 0; j < KS; ++j) zg += z[j] * gam[j];
      double phi, bp;
      if constexpr (CODY) {
        npdf_ncdf(zg, phi, bp);
        bp = clamp_phi(bp);
      } else {
        phi = npdf(zg);
        bp = clamp_phi(ncdf(zg));
      }
      // one reciprocal: r = 1 / (Phi (1 - Phi)), so 1 / Phi = (1 - Phi) r, 1 / (1 - Phi) = Phi r and
      // the weight phi^2 / (Phi (1 - Phi)) = phi^2 r
      const double qb = 1.0 - bp, r = hk_rcp(bp * qb);
      const double lam = stg[ri] > 0.5 ? phi * (qb * r) : -phi * (bp * r);  // probit.rs:66-70
      const double cwt = c * (phi * phi * r), cl = c * lam;  // sqrt_w^2 of probit.rs:75-76
      int e = 0;
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        const double t = cwt * z[j];
#pragma unroll
        for (int k = 0; k <= j; ++k) acc[e++] += t * z[k];
      }
#pragma unroll
      for (int j = 0; j < KS; ++j) acc[NH + j] += cl * z[j];
    }
  }
  block_sum(acc, red, l);
  if (l.wave == 0 && l.rep < a.n_reps)
#pragma unroll
    for (int i = 0; i < NP; ++i) a.partial[((size_t)blockIdx.x * a.rep_pad + l.rep) * NP + i] = acc[i];
}

// nalgebra LU (partial pivoting on the first largest |pivot|) + solve; false if U is singular.
template <int KS>
__device__ bool lu_solve(double (&m)[KS * KS], double (&b)[KS]) {
  int perm[KS];
#pragma unroll
  for (int i = 0; i < KS; ++i) perm[i] = i;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < KS; ++i) {
    int piv = i;
    double best = fabs(m[i + i * KS]);
#pragma unroll
    for (int r = i + 1; r < KS; ++r)
      if (fabs(m[r + i * KS]) > best) {
        best = fabs(m[r + i * KS]);
        piv = r;
      }
    // select-based swaps keep every index compile-time (registers, no scratch)
#pragma unroll
    for (int r = i + 1; r < KS; ++r)
      if (r == piv) {
#pragma unroll
        for (int c = 0; c < KS; ++c) {
          const double t = m[i + c * KS];
          m[i + c * KS] = m[r + c * KS];
          m[r + c * KS] = t;
        }
        const int t = perm[i];
        perm[i] = perm[r];
        perm[r] = t;
      }
    const double d = m[i + i * KS];
    if (d == 0.0) {
      ok = false;
      continue;
    }
#pragma unroll
    for (int r = i + 1; r < KS; ++r) m[r + i * KS] /= d;
#pragma unroll
    for (int c = i + 1; c < KS; ++c)
#pragma unroll
      for (int r = i + 1; r < KS; ++r) m[r + c * KS] += -m[i + c * KS] * m[r + i * KS];
  }
  if (!ok) return false;
  double x[KS];
#pragma unroll
  for (int i = 0; i < KS; ++i) {
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < KS; ++r)
      if (perm[i] == r) v = b[r];
    x[i] = v;
  }
#pragma unroll
  for (int i = 0; i < KS; ++i)
#pragma unroll
    for (int r = i + 1; r < KS; ++r) x[r] += -x[i] * m[r + i * KS];
#pragma unroll
  for (int i = KS - 1; i >= 0; --i) {
    x[i] /= m[i + i * KS];
#pragma unroll
    for (int r = 0; r < i; ++r) x[r] += -x[i] * m[r + i * KS];
  }
#pragma unroll
  for (int i = 0; i < KS; ++i) b[i] = x[i];
  return true;
}

template <int KS>
__global__ __launch_bounds__(64) void ob_probit_step_kernel(const ob_heck_seg a) {
  constexpr int NH = KS * (KS + 1) / 2, NP = NH + KS;
  const uint32_t rep = blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
  if (rep >= a.n_reps) return;
  const size_t st = (size_t)g * a.rep_pad + rep;
  const uint32_t fl = a.hflags[st];
  if (fl & kDone) return;
  double sum[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) sum[i] = 0.0;
  for (int c = 0; c < a.n_chunks; ++c) {
    if (a.chunks[3 * c] != g) continue;
    const double* pp = a.partial + ((size_t)c * a.rep_pad + rep) * NP;
#pragma unroll
    for (int i = 0; i < NP; ++i) sum[i] += pp[i];
  }
  // -H = sum c w z z' + 1e-9 I (probit.rs:95-118), g = sum c lambda z
  double m[KS * KS], l[KS * KS], b[KS];
  int e = 0;
#pragma unroll
  for (int j = 0; j < KS; ++j)
#pragma unroll
    for (int k = 0; k <= j; ++k) {
      m[j + k * KS] = sum[e];
      m[k + j * KS] = sum[e];
      ++e;
    }
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    m[j + j * KS] += 1e-9;
    b[j] = sum[NH + j];
  }
#pragma unroll
  for (int i = 0; i < KS * KS; ++i) l[i] = m[i];
  bool chol = true;
#pragma unroll
  for (int j = 0; j < KS; ++j) {  // nalgebra Cholesky::new order
#pragma unroll
    for (int i = j; i < KS; ++i) {
      double v = l[i + j * KS];
#pragma unroll
      for (int c = 0; c < j; ++c) v = -l[j + c * KS] * l[i + c * KS] + v;
      l[i + j * KS] = v;
    }
    const double diag = l[j + j * KS];
    if (!(diag != 0.0 && diag >= 0.0)) chol = false;
    const double den = sqrt(diag);
#pragma unroll
    for (int i = j + 1; i < KS; ++i) l[i + j * KS] /= den;
    l[j + j * KS] = den;
  }
  double step[KS];
#pragma unroll
  for (int i = 0; i < KS; ++i) step[i] = b[i];
  if (chol) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const double coeff = step[i] / l[i + i * KS];
#pragma unroll
      for (int r = i + 1; r < KS; ++r) step[r] -= coeff * l[r + i * KS];
      step[i] = coeff;
    }
#pragma unroll
    for (int i = KS - 1; i >= 0; --i) {
      double part = 0.0;
#pragma unroll
      for (int r = i + 1; r < KS; ++r) part += l[r + i * KS] * step[r];
      step[i] = (step[i] - part) / l[i + i * KS];
    }
  } else if (!lu_solve<KS>(m, step)) {  // probit.rs:124-137: -(H^-1 g) = (-H)^-1 g
    a.hflags[st] = kDone | kFailed;
    return;
  }
  double nrm = 0.0;
#pragma unroll
  for (int i = 0; i < KS; ++i) {
    a.gamma[st * KS + i] += step[i];
    nrm += step[i] * step[i];
  }
  if (sqrt(nrm) < a.tol)
    a.hflags[st] = kDone;
  else
    atomicAdd(a.active, 1u);
}

// Staged columns per row of the sums kernel: x_1..x_p, y, [s == 1], s, z_1..z_{ks-1}, (w).
__host__ __device__ inline int heck_sums_cols(int p, int ks, int weighted) { return p + 2 + ks + (weighted ? 1 : 0); }

template <int NB, bool CODY>
__global__ __launch_bounds__(kHB) void ob_heck_sums_kernel(const ob_heck_seg a) {
  extern __shared__ __attribute__((aligned(16))) double hsm[];
  double* red = hsm;  // [64][NB + 1], then the waves' staged sub-tiles
  const Lanes l = lanes(a);
  const bool act = l.rep < a.n_reps;
  if (!__syncthreads_or(act)) return;
  const int K = a.p + 1, ks = a.ks, nhs = ob::heck_sums_len(K, ks);
  const size_t st = (size_t)l.g * a.rep_pad + l.rep;
  double gam[ob::kHeckMaxKs];
#pragma unroll
  for (int j = 0; j < ob::kHeckMaxKs; ++j) gam[j] = (act && j < ks) ? a.gamma[st * ks + j] : 0.0;
  double acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) acc[i] = 0.0;
  const double* X = a.cols[l.g];
  const int64_t ld = a.ld[l.g];
  const uint32_t n = a.n[l.g];
  const int ncol = heck_sums_cols(a.p, ks, a.weighted), cy = a.p, cind = a.p + 1, cz = a.p + 2, cw8 = a.p + 2 + ks;
  double* stg = hsm + 64 * (NB + 1) + l.wave * (ncol * 64);
  for (uint32_t tile = l.t0; tile < l.t1; ++tile) {
    const uint32_t r0 = tile * OB_TILE_ROWS + l.wave * 64;
    if (r0 >= n) break;
    const uint32_t nr = min(64u, n - r0);
    wave_stage(stg, X, ld, r0, nr, ncol, l.lane);
    const uint32_t* cw = count_row(a, l, tile);
    uint32_t word = 0;
    for (uint32_t ri = 0; ri < nr; ++ri) {
      if ((ri & 3) == 0) word = count_word(a, cw, ri);
      const uint32_t cu = (word >> ((ri & 3) * 8)) & 255u;
      if (!act || cu == 0) continue;
      const double c = (double)cu;
      double z[ob::kHeckMaxKs];
      z[0] = 1.0;
#pragma unroll
      for (int j = 1; j < ob::kHeckMaxKs; ++j) z[j] = j < ks ? stg[(cz + j) * 64 + ri] : 0.0;
      double zg = 0.0;
#pragma unroll
      for (int j = 0; j < ob::kHeckMaxKs; ++j)
        if (j < ks) zg += z[j] * gam[j];
#pragma unroll
      for (int j = 0; j < ob::kHeckMaxKs; ++j) acc[5 + j] += c * z[j];  // selection means (all rows)
      const double y = stg[cy * 64 + ri], w = a.weighted ? stg[cw8 * 64 + ri] : 1.0;
      acc[3] += c * w * y;  // total gap (builder.rs:676-684, all rows)
      acc[4] += c * w;
      if (stg[cind * 64 + ri] == 1.0) {  // heckman.rs:56-69: lambda = phi / Phi, 0 when Phi < 1e-10
        double pd, bp;
        if constexpr (CODY) {
          npdf_ncdf(zg, pd, bp);
        } else {
          pd = npdf(zg);
          bp = ncdf(zg);
        }
        const double lam = bp < 1e-10 ? 0.0 : pd * hk_rcp(bp);
        const double cl = c * lam;
        acc[0] += cl * y;
        acc[1] += cl * lam;
        acc[2] += cl * (lam + zg);
        acc[13] += cl;
#pragma unroll
        for (int j = 1; j < NB - 13; ++j)
          if (j < K) acc[13 + j] += cl * stg[(j - 1) * 64 + ri];
      }
    }
  }
  block_sum(acc, red, l);
  if (l.wave == 0 && act)
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (i < nhs) a.partial[((size_t)blockIdx.x * a.rep_pad + l.rep) * nhs + i] = acc[i];
}

size_t heck_solve_lds(const ob_heck_seg& a) {
  const int K = a.p + 1, kp = K + 1;
  return sizeof(double) * ((size_t)kp * kp + 7 * (size_t)kp + 2 * (size_t)ob::heck_sums_len(K, a.ks) + 4);
}

// Sums layout (per group): [0] c lam y, [1] c lam^2, [2] c lam (lam + z'g), [3] c w y, [4] c w,
// [5..5+S) c z_j, [5+S..5+S+K) c lam x_j (x_0 = 1); S = heck_sel_slots(ks): 8 for ks <= 8, else ks.
__global__ __launch_bounds__(64) void ob_heck_solve_kernel(const ob_heck_seg a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int lane = threadIdx.x;
  const uint32_t rep = blockIdx.x;
  if (rep >= a.n_reps) return;
  const int K = a.p + 1, kp = K + 1, ks = a.ks, nhs = ob::heck_sums_len(K, ks), lx = 5 + ob::heck_sel_slots(ks);
  const uint32_t ppad = a.part_pad;  // == rep_pad on the narrow path
  double* M = sm;
  double* rhs = M + kp * kp;
  double* beta_a = rhs + kp;
  double* beta_b = beta_a + kp;
  double* xam = beta_b + kp;
  double* xbm = xam + kp;
  double* bstar = xbm + kp;
  double* S = bstar + kp;      // [2][nhs]
  double* delta = S + 2 * nhs;  // [2]
  for (int i = lane; i < 2 * nhs; i += 64) {
    const uint32_t g = (uint32_t)(i / nhs);
    const int j = i % nhs;
    double v = 0.0;
    for (int c = 0; c < a.n_chunks; ++c)
      if (a.chunks[3 * c] == g) v += a.partial[((size_t)c * ppad + rep) * nhs + j];
    S[i] = v;
  }
  __syncthreads();
  const double* GA = a.gram + (size_t)rep * 2 * a.e_pad;
  const double* GB = GA + a.e_pad;
  double* row = a.rows + (size_t)rep * a.row_len;
  uint8_t status = OB_HS_OK;
  if (GA[0] == 0.0 || GB[0] == 0.0) status = OB_HS_NO_OUTCOMES;  // estimation.rs:124-125
  for (int g = 0; g < 2 && status == OB_HS_OK; ++g) {
    if (a.hflags[(size_t)g * a.rep_pad + rep] & kFailed) {
      status = OB_HS_PROBIT;
      break;
    }
    const double* G = g ? GB : GA;
    const double* Sg = S + g * nhs;
    const double nsel = G[0];
    if (nsel <= (double)kp) {  // ols.rs:98-104
      status = OB_HS_INSUFFICIENT;
      break;
    }
    for (int i = lane; i < kp * kp; i += 64) {
      const int r = i % kp, c = i / kp;
      double v;
      if (r < K && c < K)
        v = gpair(G, r, c, a.k1);
      else if (r == K && c == K)
        v = Sg[1];
      else
        v = Sg[lx + (r == K ? c : r)];
      M[r + c * kp] = v;
    }
    for (int i = lane; i < kp; i += 64) rhs[i] = i < K ? gpair(G, i, K, a.k1) : Sg[0];
    __syncthreads();
    if (!wave_cholesky(M, kp, lane)) {
      status = OB_HS_CHOLESKY;
      break;
    }
    wave_chol_solve(M, kp, rhs, lane);
    double* beta = g ? beta_b : beta_a;
    double* xm = g ? xbm : xam;
    for (int i = lane; i < kp; i += 64) {
      beta[i] = rhs[i];
      xm[i] = i < K ? gpair(G, 0, i, a.k1) / nsel : Sg[lx] / nsel;  // row means + IMR mean
    }
    if (lane == 0) delta[g] = -Sg[2] / nsel;  // heckman.rs:92-99
    __syncthreads();
  }
  if (status == OB_HS_OK) {  // beta* (builder.rs:536-621; Pooled/Neumark are refused on the host)
    if (a.ref_mode == OB_REF_GROUP_A || a.ref_mode == OB_REF_GROUP_B) {
      const double* src = a.ref_mode == OB_REF_GROUP_A ? beta_a : beta_b;
      for (int i = lane; i < kp; i += 64) bstar[i] = src[i];
    } else {
      const double sa = S[4], sb = S[nhs + 4];
      const double tot = sa + sb;
      if (tot == 0.0) {
        status = OB_HS_ZERO_WEIGHT;
      } else {
        const double wA = sa / tot, wB = 1.0 - wA;
        for (int i = lane; i < kp; i += 64) bstar[i] = beta_a[i] * wA + beta_b[i] * wB;
      }
    }
  }
  __syncthreads();
  if (lane == 0) {
    if (status != OB_HS_OK) {
      for (int i = 0; i < a.row_len; ++i) row[i] = __builtin_nan("");
    } else {
      double* dex = row + 6;
      double* dun = row + 6 + kp;
      double expl = 0.0, ta = 0.0, tb = 0.0, endow = 0.0, coef = 0.0, inter = 0.0;
      for (int j = 0; j < kp; ++j) {  // decomposition.rs:56-89
        const double dx = xam[j] - xbm[j], db = beta_a[j] - beta_b[j];
        expl += dx * bstar[j];
        ta += xam[j] * beta_a[j];
        tb += xbm[j] * beta_b[j];
        endow += dx * beta_b[j];
        coef += xbm[j] * db;
        inter += dx * db;
      }
      for (int j = 0; j < kp; ++j) {  // decomposition.rs:92-122
        dex[j] = (xam[j] - xbm[j]) * bstar[j];
        dun[j] = xam[j] * (beta_a[j] - bstar[j]) + xbm[j] * (bstar[j] - beta_b[j]);
      }
      row[0] = expl;
      row[1] = (ta - tb) - expl;
      row[2] = endow;
      row[3] = coef;
      row[4] = inter;
      row[5] = S[3] / S[4] - S[nhs + 3] / S[nhs + 4];
      double* tail = row + 6 + 2 * kp;
      for (int j = 0; j < kp; ++j) {
        tail[j] = beta_a[j];
        tail[kp + j] = beta_b[j];
        tail[2 * kp + j] = xam[j];
        tail[3 * kp + j] = xbm[j];
        tail[4 * kp + j] = bstar[j];
      }
      // selection terms (builder.rs:510-530): A's (theta, delta, gamma) for GroupA, else B's
      const int gr = a.ref_mode == OB_REF_GROUP_A ? 0 : 1;
      const double theta = gr ? beta_b[K] : beta_a[K];
      const double* gam = a.gamma + ((size_t)gr * a.rep_pad + rep) * ks;
      double* sel = tail + 5 * kp;
      for (int j = 0; j < ks; ++j) {
        const double za = S[5 + j] / S[5], zb = S[nhs + 5 + j] / S[nhs + 5];
        sel[j] = theta * delta[gr] * gam[j] * (za - zb);
      }
    }
    a.ok[rep] = a.raw_status ? status : (uint8_t)(status == OB_HS_OK);
  }
}

// ---- The wide path: 8 < ks <= 32 selection columns ------------------------------------------------
// Once the weights are known a probit pass is a GEMM: with W[r, i] = c_ri phi^2 / (Phi (1 - Phi)) and
// L[r, i] = c_ri lambda_ri, the Hessian sums are W . P with P[i, (j, k)] = z_ij z_ik and the gradient
// sums are L . Z. ob_heck_wide_kernel runs both on v_mfma_f64_16x16x4_f64 (A = 16 replicates x 4 rows,
// B = 4 rows x 16 columns); the IMR sums are the same kernel with A = c (all rows: c z_j, c w y, c w)
// and A = c lambda (selected rows: c lambda [y, 1, x]).
//
// Block = (row chunk, 16 replicates), 4 waves. Per 64-row sub-tile:
//   stage  the columns of the sub-tile -> LDS [col][65] (+ a column of ones for z_0 and the single
//          column products), one coalesced load per column, shared by the block;
//   A      thread = (replicate t & 15, rows 4 (t >> 4) .. + 3: one count word): z'gamma, phi, Phi, the
//          clamp and the one reciprocal exactly as ob_probit_kernel, -> LDS [operand][row][16];
//   B      wave w owns the column tiles w, w + 4, ..: at most 9 accumulators of 16 replicates x 16
//          columns (35 tiles at ks = 32). Per 4-row step a lane reads its two A values once and forms
//          each tile's B value as the product of two staged columns (never stored in HBM).
// A tile takes one A operand, so the Hessian pairs (ks (ks + 1) / 2) and the gradient (ks) fill
// separate tiles, padded to 16. A wave owns its tiles over the whole chunk, so there is no block
// sum: every partial is one accumulator element, summed over the chunk's rows in row order. An output
// element of the MFMA depends on its own A row and B column only, so a replicate's partials do not
// depend on its slot in the block or on its neighbours.
using d4 = __attribute__((ext_vector_type(4))) double;
constexpr int kWS = 65;      // doubles per staged column: a tile's 16 column reads spread over the banks
constexpr int kWReps = 16;   // replicates per block
constexpr int kWMaxU = 9;    // column tiles per wave

inline size_t wide_lds(const ob_heck_seg& a, bool sums) {
  const int ncol = sums ? heck_sums_cols(a.p, a.ks, a.weighted) : a.ks;
  return sizeof(double) * ((size_t)(ncol + 1) * kWS + 2 * 64 * kWReps + (size_t)kWReps * (a.ks | 1) + (sums ? 512 : 0));
}

template <bool SUMS, bool CODY>
__global__ __launch_bounds__(kHB) void ob_heck_wide_kernel(const ob_heck_seg a) {
  extern __shared__ __attribute__((aligned(16))) double wsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const int ks = a.ks, K = a.p + 1, gs = ks | 1;
  const int ncol = SUMS ? heck_sums_cols(a.p, ks, a.weighted) : ks;
  const int zc0 = SUMS ? a.p + 2 : 0;  // staged column of s; z_j is zc0 + j
  const int ones = ncol * kWS;
  double* stg = wsm;                    // [ncol + 1][kWS]
  double* wl = stg + (ncol + 1) * kWS;  // [2][64 rows][16 replicates]
  double* gm = wl + 2 * 64 * kWReps;    // [16][gs] gamma
  double* red = gm + kWReps * gs;       // SUMS: [2][16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep0 = blockIdx.y * kWReps, rep = rep0 + r16;
  bool act = rep < a.n_reps;
  if (!SUMS && act) act = !(a.hflags[(size_t)g * a.rep_pad + rep] & kDone);
  if (!__syncthreads_or(act)) return;
  for (int i = tid; i < kWReps * ks; i += kHB) {
    const int rr = i / ks, j = i - rr * ks;
    gm[rr * gs + j] = rep0 + rr < a.n_reps ? a.gamma[((size_t)g * a.rep_pad + rep0 + rr) * ks + j] : 0.0;
  }
  if (tid < 64) stg[ones + tid] = 1.0;
  // this lane's column of each of the wave's tiles: the two staged columns whose product is the B
  // value, and the slot of the partial it lands in (-1: padding)
  const int NH = ks * (ks + 1) / 2;
  const int nt0 = SUMS ? (ks + 2 + 15) / 16 : (NH + 15) / 16;  // tiles of operand 0 (W; c)
  const int nt1 = SUMS ? (K + 1 + 15) / 16 : (ks + 15) / 16;   // tiles of operand 1 (L; c lambda)
  const int NT = nt0 + nt1, lx = 5 + ob::heck_sel_slots(ks);
  int oa[kWMaxU], ob2[kWMaxU], dst[kWMaxU];
#pragma unroll
  for (int u = 0; u < kWMaxU; ++u) {
    const int c = wave + 4 * u, e16 = lane & 15;
    oa[u] = ones;
    ob2[u] = ones;
    dst[u] = -1;
    if (c < nt0) {
      const int idx = 16 * c + e16;
      if constexpr (!SUMS) {
        if (idx < NH) {
          const int j = tri_row(idx), k = idx - j * (j + 1) / 2;
          oa[u] = j ? j * kWS : ones;
          ob2[u] = k ? k * kWS : ones;
          dst[u] = idx;
        }
      } else {
        const int wcol = a.weighted ? (a.p + 2 + ks) * kWS : ones;
        if (idx < ks) {  // c z_j
          oa[u] = idx ? (zc0 + idx) * kWS : ones;
          dst[u] = 5 + idx;
        } else if (idx == ks) {  // c w y
          oa[u] = wcol;
          ob2[u] = a.p * kWS;
          dst[u] = 3;
        } else if (idx == ks + 1) {  // c w
          oa[u] = wcol;
          dst[u] = 4;
        }
      }
    } else if (c < NT) {
      const int idx = 16 * (c - nt0) + e16;
      if constexpr (!SUMS) {
        if (idx < ks) {
          oa[u] = idx ? idx * kWS : ones;
          dst[u] = NH + idx;
        }
      } else {
        if (idx == 0) {  // c lambda y
          oa[u] = a.p * kWS;
          dst[u] = 0;
        } else if (idx <= K) {  // c lambda x_j, x_0 = 1
          oa[u] = idx > 1 ? (idx - 2) * kWS : ones;
          dst[u] = lx + idx - 1;
        }
      }
    }
  }
  d4 acc[kWMaxU];
#pragma unroll
  for (int u = 0; u < kWMaxU; ++u) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
  double s1 = 0.0, s2 = 0.0;  // SUMS: c lambda^2, c lambda (lambda + z'gamma) of this thread's rows
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const double* src = SUMS ? X : X + (size_t)a.sz_col * ld;
  const uint32_t rb = rep >> 6, R = rep & 63;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's operand reads
      for (int i = tid; i < ncol * 64; i += kHB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kWS + r] = (uint32_t)r < nr ? src[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      uint32_t word = 0;  // counts of rows 4 q .. 4 q + 3 (count_row / count_word's two layouts)
      if (act) {
        const size_t tt = (g ? a.tiles0 : 0u) + tile;
        if (!a.counts)
          word = 0x01010101u;
        else if (a.counts_i8)
          word = a.counts[((tt * a.nb_rep + rb) * 1024 + sw * 256 + (R >> 4) * 64 + (R & 15)) * 4 + (q >> 2) * 64 + (q & 3)];
        else
          word = a.counts[((tt * a.nb_rep + rb) * 4 + sw) * kCimgWords + R * kCimgStride + q];
      }
      double zg[4];
      if (word) {
        const double g0 = gm[r16 * gs];
#pragma unroll
        for (int i = 0; i < 4; ++i) zg[i] = g0;
        for (int j = 1; j < ks; ++j) {
          const double gj = gm[r16 * gs + j];
          const double* zj = stg + (zc0 + j) * kWS + 4 * q;
#pragma unroll
          for (int i = 0; i < 4; ++i) zg[i] += zj[i] * gj;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t row = 4 * q + i;
        const uint32_t cu = row < nr ? (word >> (8 * i)) & 255u : 0u;
        double w0 = 0.0, w1 = 0.0;
        if (cu) {
          const double c = (double)cu;
          if constexpr (!SUMS) {
            double phi, bp;
            if constexpr (CODY) {
              npdf_ncdf(zg[i], phi, bp);
              bp = clamp_phi(bp);
            } else {
              phi = npdf(zg[i]);
              bp = clamp_phi(ncdf(zg[i]));
            }
            const double qb = 1.0 - bp, r = hk_rcp(bp * qb);  // as ob_probit_kernel
            const double lam = stg[row] > 0.5 ? phi * (qb * r) : -phi * (bp * r);
            w0 = c * (phi * phi * r);
            w1 = c * lam;
          } else {
            w0 = c;
            if (stg[(a.p + 1) * kWS + row] == 1.0) {  // as ob_heck_sums_kernel
              double pd, bp;
              if constexpr (CODY) {
                npdf_ncdf(zg[i], pd, bp);
              } else {
                pd = npdf(zg[i]);
                bp = ncdf(zg[i]);
              }
              const double lam = bp < 1e-10 ? 0.0 : pd * hk_rcp(bp);
              w1 = c * lam;
              s1 += w1 * lam;
              s2 += w1 * (lam + zg[i]);
            }
          }
        }
        wl[row * kWReps + r16] = w0;
        wl[64 * kWReps + row * kWReps + r16] = w1;
      }
      __syncthreads();
      const int rl = lane >> 4;
#pragma unroll 2
      for (int i = 0; i < 16; ++i) {
        const double a0 = wl[i * 64 + lane], a1 = wl[64 * kWReps + i * 64 + lane];
        const int row = 4 * i + rl;
#pragma unroll
        for (int u = 0; u < kWMaxU; ++u)
          if (wave + 4 * u < NT)
            acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(wave + 4 * u < nt0 ? a0 : a1, stg[oa[u] + row] * stg[ob2[u] + row],
                                                          acc[u], 0, 0, 0);
      }
    }
  }
  // lane (rl, e16), element r of acc[u]: replicate rep0 + rl + 4 r, the tile's column e16
  const int nv = SUMS ? ob::heck_sums_len(K, ks) : NH + ks;
  double* out = a.partial + (size_t)chunk * a.part_pad * nv;
#pragma unroll
  for (int u = 0; u < kWMaxU; ++u)
    if (wave + 4 * u < NT && dst[u] >= 0)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t rp = rep0 + (lane >> 4) + 4 * r;
        if (rp < a.n_reps) out[(size_t)rp * nv + dst[u]] = acc[u][r];
      }
  if constexpr (SUMS) {  // the two sums that are not linear in lambda: row groups in order
    red[q * kWReps + r16] = s1;
    red[256 + q * kWReps + r16] = s2;
    __syncthreads();
    if (tid < 32) {
      const int which = tid >> 4;
      double v = 0.0;
      for (int qq = 0; qq < 16; ++qq) v += red[which * 256 + qq * kWReps + r16];
      if (rep < a.n_reps) out[(size_t)rep * nv + 1 + which] = v;
    }
  }
}

// nalgebra LU (partial pivoting on the first largest |pivot|) + solve on one lane, m (n x n
// col-major) and b in LDS, x and perm scratch; false if U is singular (lu_solve with a runtime n).
__device__ bool lu_solve_lds(double* m, double* b, double* x, int* perm, int n) {
  for (int i = 0; i < n; ++i) perm[i] = i;
  bool ok = true;
  for (int i = 0; i < n; ++i) {
    int piv = i;
    double best = fabs(m[i + i * n]);
    for (int r = i + 1; r < n; ++r)
      if (fabs(m[r + i * n]) > best) {
        best = fabs(m[r + i * n]);
        piv = r;
      }
    if (piv != i) {
      for (int c = 0; c < n; ++c) {
        const double t = m[i + c * n];
        m[i + c * n] = m[piv + c * n];
        m[piv + c * n] = t;
      }
      const int t = perm[i];
      perm[i] = perm[piv];
      perm[piv] = t;
    }
    const double d = m[i + i * n];
    if (d == 0.0) {
      ok = false;
      continue;
    }
    for (int r = i + 1; r < n; ++r) m[r + i * n] /= d;
    for (int c = i + 1; c < n; ++c)
      for (int r = i + 1; r < n; ++r) m[r + c * n] += -m[i + c * n] * m[r + i * n];
  }
  if (!ok) return false;
  for (int i = 0; i < n; ++i) x[i] = b[perm[i]];
  for (int i = 0; i < n; ++i)
    for (int r = i + 1; r < n; ++r) x[r] += -x[i] * m[r + i * n];
  for (int i = n - 1; i >= 0; --i) {
    x[i] /= m[i + i * n];
    for (int r = 0; r < i; ++r) x[r] += -x[i] * m[r + i * n];
  }
  for (int i = 0; i < n; ++i) b[i] = x[i];
  return true;
}

// ob_probit_step_kernel for the wide path: one wave per (replicate, group).
__global__ __launch_bounds__(64) void ob_probit_wide_step_kernel(const ob_heck_seg a) {
  constexpr int M = ob::kHeckWideMaxKs;
  __shared__ double m[M * M], l[M * M], b[M], step[M], x[M];
  __shared__ int perm[M];
  __shared__ int solved;
  const int lane = threadIdx.x, ks = a.ks;
  const uint32_t rep = blockIdx.x, g = blockIdx.y;
  const size_t st = (size_t)g * a.rep_pad + rep;
  if (a.hflags[st] & kDone) return;
  gather_partials(a.partial, a.part_pad, rep, ks * (ks + 1) / 2 + ks, a.chunks, a.n_chunks, (int)g, ks, lane, m, step);
  __syncthreads();
  // -H = sum c w z z' + 1e-9 I (probit.rs:95-118), g = sum c lambda z; Cholesky factors the copy l, the LU fallback takes m and b
  for (int i = lane; i < ks * ks; i += 64) {
    if (i % (ks + 1) == 0) m[i] += 1e-9;
    l[i] = m[i];
  }
  for (int i = lane; i < ks; i += 64) b[i] = step[i];
  __syncthreads();
  const bool chol = wave_cholesky(l, ks, lane);
  __syncthreads();
  if (chol) {
    wave_chol_solve(l, ks, step, lane);
  } else {  // probit.rs:124-137: -(H^-1 g) = (-H)^-1 g
    if (lane == 0) {
      solved = lu_solve_lds(m, b, x, perm, ks) ? 1 : 0;
      for (int i = 0; i < ks; ++i) step[i] = b[i];
    }
    __syncthreads();
    if (!solved) {
      if (lane == 0) a.hflags[st] = kDone | kFailed;
      return;
    }
  }
  __syncthreads();
  if (lane == 0) {
    double nrm = 0.0;
    for (int i = 0; i < ks; ++i) {
      a.gamma[st * ks + i] += step[i];
      nrm += step[i] * step[i];
    }
    if (sqrt(nrm) < a.tol)
      a.hflags[st] = kDone;
    else
      atomicAdd(a.active, 1u);
  }
}

hipError_t launch_wide(const ob_heck_seg& a, bool sums, hipStream_t s) {
  const bool cody = hk_cody();
  const void* fn = sums ? (cody ? (const void*)ob_heck_wide_kernel<true, true> : (const void*)ob_heck_wide_kernel<true, false>)
                        : (cody ? (const void*)ob_heck_wide_kernel<false, true> : (const void*)ob_heck_wide_kernel<false, false>);
  const size_t lds = wide_lds(a, sums);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  void* args[] = {const_cast<ob_heck_seg*>(&a)};
  e = hipLaunchKernel(fn, dim3(a.n_chunks, (a.n_reps + kWReps - 1) / kWReps), dim3(kHB), args, lds, s);
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t probit_iter_wide(const ob_heck_seg& a, hipStream_t s, hipEvent_t* ev) {
  if (ev) (void)hipEventRecord(ev[0], s);
  hipError_t e = launch_wide(a, false, s);
  if (e != hipSuccess) return e;
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(ob_probit_wide_step_kernel, dim3(a.n_reps, 2), dim3(64), 0, s, a);
  return hipGetLastError();
}

template <int KS>
hipError_t launch_probit_iter(const ob_heck_seg& a, hipStream_t s, hipEvent_t* ev) {
  if (ev) (void)hipEventRecord(ev[0], s);
  if (hk_cody())
    hipLaunchKernelGGL((ob_probit_kernel<KS, true>), dim3(a.n_chunks, a.rep_pad / 64), dim3(kHB), 0, s, a);
  else
    hipLaunchKernelGGL((ob_probit_kernel<KS, false>), dim3(a.n_chunks, a.rep_pad / 64), dim3(kHB), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(ob_probit_step_kernel<KS>, dim3(a.rep_pad / 64, 2), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t probit_iter(const ob_heck_seg& a, hipStream_t s, hipEvent_t* ev) {
  if (a.ks > ob::kHeckMaxKs) return probit_iter_wide(a, s, ev);
  switch (a.ks) {
    case 1: return launch_probit_iter<1>(a, s, ev);
    case 2: return launch_probit_iter<2>(a, s, ev);
    case 3: return launch_probit_iter<3>(a, s, ev);
    case 4: return launch_probit_iter<4>(a, s, ev);
    case 5: return launch_probit_iter<5>(a, s, ev);
    case 6: return launch_probit_iter<6>(a, s, ev);
    case 7: return launch_probit_iter<7>(a, s, ev);
    default: return launch_probit_iter<8>(a, s, ev);
  }
}

}  // namespace

namespace ob {

// The Fisher-scoring loop of a segment from gamma = 0 (probit.rs:48-147), each replicate stopping on
// its own. On return (after a stream sync) gamma and hflags are final; the outcome fields of the
// segment (p, gram, rows, ok) are not read. The probit stage of heckman_segment, of ob_probit and of
// the binary decomposition (ob_binary.hip).
int probit_stage(const ob_heck_seg& a, hipStream_t s, int* iters, ob_heck_times* tm) {
  if (a.ks < 1 || a.ks > kHeckWideMaxKs || a.rep_pad % 64 != 0 || a.part_pad < a.n_reps ||
      (a.ks <= kHeckMaxKs && a.part_pad != a.rep_pad))
    return ob::fail(OB_E_INVALID, "probit stage: bad shape");
  Events<2> evs;  // around each probit pass when tm is given
  if (tm) OB_HIP(evs.create());
  hipEvent_t* const ev = evs.e;
  if (a.part_pad == a.rep_pad) {
    OB_HIP(hipMemsetAsync(a.gamma, 0, sizeof(double) * 2 * a.rep_pad * a.ks, s));
    OB_HIP(hipMemsetAsync(a.hflags, 0, sizeof(uint32_t) * 2 * a.rep_pad, s));
  } else {  // a batch of a wider segment (bases moved to its first replicate): its own replicates only
    const size_t n64 = ((size_t)a.n_reps + 63) / 64 * 64;
    for (size_t g = 0; g < 2; ++g) {
      OB_HIP(hipMemsetAsync(a.gamma + g * a.rep_pad * a.ks, 0, sizeof(double) * n64 * a.ks, s));
      OB_HIP(hipMemsetAsync(a.hflags + g * a.rep_pad, 0, sizeof(uint32_t) * n64, s));
    }
  }
  int it = 0;
  while (it < a.max_iter) {
    OB_HIP(hipMemsetAsync(a.active, 0, sizeof(uint32_t), s));
    OB_HIP(probit_iter(a, s, tm ? ev : nullptr));
    ++it;
    uint32_t active = 0;
    OB_HIP(hipMemcpyAsync(&active, a.active, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OB_HIP(hipStreamSynchronize(s));
    if (tm) {
      float ms = 0.f;
      OB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
      tm->probit_ms += ms;
      tm->probit_launches += 1;
    }
    if (active == 0) break;
  }
  if (iters) *iters = it;
  return OB_OK;
}

int heckman_segment(const ob_heck_seg& a, hipStream_t s, int* iters, ob_heck_times* tm) {
  const bool wide = a.ks > kHeckMaxKs;
  if (a.ks < 1 || a.ks > kHeckWideMaxKs || a.p > kHeckMaxP || a.rep_pad % 64 != 0 || a.part_pad < a.n_reps ||
      (!wide && a.part_pad != a.rep_pad))
    return ob::fail(OB_E_INVALID, "heckman segment: bad shape");
  Events<2> ev;  // around the sums pass
  if (tm) OB_HIP(ev.create());
  OB_TRY(probit_stage(a, s, iters, tm));
  if (wide) {  // the IMR sums on the MFMA kernel, then the same solve
    if (tm) OB_HIP(hipEventRecord(ev.e[0], s));
    OB_HIP(launch_wide(a, true, s));
    if (tm) OB_HIP(hipEventRecord(ev.e[1], s));
    const size_t lds = heck_solve_lds(a);
    OB_HIP(hipFuncSetAttribute((const void*)ob_heck_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ob_heck_solve_kernel, dim3(a.n_reps), dim3(64), lds, s, a);
    OB_HIP(hipGetLastError());
    if (tm) {
      float ms = 0.f;
      OB_HIP(hipEventSynchronize(ev.e[1]));
      OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
      tm->sums_ms += ms;
    }
    return OB_OK;
  }
  const dim3 grid(a.n_chunks, a.rep_pad / 64);
  const int nhs = heck_sums_len(a.p + 1, a.ks);
  const int nb = nhs <= 32 ? 32 : (nhs <= 40 ? 40 : 64);
  const size_t lds_sums =
      sizeof(double) * (64 * (size_t)(nb + 1) + 4 * 64 * (size_t)heck_sums_cols(a.p, a.ks, a.weighted));
  const bool cody = hk_cody();
  auto sums = [&](auto nbc, auto cc) {
    constexpr int NB = decltype(nbc)::value;
    constexpr bool C = decltype(cc)::value;
    return (const void*)ob_heck_sums_kernel<NB, C>;
  };
  using T = std::true_type;
  using F = std::false_type;
  const void* fn = nb == 32   ? (cody ? sums(std::integral_constant<int, 32>{}, T{}) : sums(std::integral_constant<int, 32>{}, F{}))
                   : nb == 40 ? (cody ? sums(std::integral_constant<int, 40>{}, T{}) : sums(std::integral_constant<int, 40>{}, F{}))
                              : (cody ? sums(std::integral_constant<int, 64>{}, T{}) : sums(std::integral_constant<int, 64>{}, F{}));
  OB_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sums));
  if (tm) OB_HIP(hipEventRecord(ev.e[0], s));
  void* args[] = {const_cast<ob_heck_seg*>(&a)};
  OB_HIP(hipLaunchKernel(fn, grid, dim3(kHB), args, lds_sums, s));
  OB_HIP(hipGetLastError());
  if (tm) OB_HIP(hipEventRecord(ev.e[1], s));
  const size_t lds = heck_solve_lds(a);
  OB_HIP(hipFuncSetAttribute((const void*)ob_heck_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ob_heck_solve_kernel, dim3(a.n_reps), dim3(64), lds, s, a);
  OB_HIP(hipGetLastError());
  if (tm) {  // the events die with this call: read the sums pass now
    float ms = 0.f;
    OB_HIP(hipEventSynchronize(ev.e[1]));
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    tm->sums_ms += ms;
  }
  return OB_OK;
}

}  // namespace ob

// math/probit.rs::probit on unresampled rows (include/oaxaca_boot.h): a one-replicate, one-group
// segment of the kernels above over the panel [y | x_1 .. x_{k-1}], every row counted once.
extern "C" int ob_probit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k,
                         int32_t max_iter, double tol, double* beta, int32_t* converged, int32_t* iterations) {
  if (!x || !y || !beta) return ob::fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || k < 1) return ob::fail(OB_E_INVALID, "ob_probit needs n > 0 rows and k >= 1 columns, got n = %lld, k = %d", (long long)n, k);
  if (k > ob::kHeckWideMaxKs)
    return ob::fail(OB_E_UNSUPPORTED, "ob_probit takes at most %d columns, got %d", ob::kHeckWideMaxKs, k);
  if (ldx < n) return ob::fail(OB_E_INVALID, "ob_probit: ldx = %lld is below n = %lld", (long long)ldx, (long long)n);
  if (n >= ((int64_t)1 << 31)) return ob::fail(OB_E_UNSUPPORTED, "ob_probit takes fewer than 2^31 rows");
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  for (int64_t i = 0; i < n; ++i)  // the kernels take z_0 = 1 as given
    if (x[i] != 1.0) return ob::fail(OB_E_UNSUPPORTED, "ob_probit: column 0 of x must be the intercept (all ones)");
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint32_t tiles = (uint32_t)((n + OB_TILE_ROWS - 1) / OB_TILE_ROWS), nc = std::min<uint32_t>(tiles, 128u);
  std::vector<uint32_t> chunks;
  for (uint32_t c = 0; c < nc; ++c) {
    chunks.push_back(0u);
    chunks.push_back((uint32_t)((uint64_t)tiles * c / nc));
    chunks.push_back((uint32_t)((uint64_t)tiles * (c + 1) / nc));
  }
  const uint32_t rep_pad = 64;
  DevBuf d_cols, d_chunks, d_gamma, d_flags, d_partial;
  OB_HIP(d_cols.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(d_chunks.alloc(sizeof(uint32_t) * chunks.size()));
  OB_HIP(d_gamma.alloc(sizeof(double) * 2 * rep_pad * k));
  OB_HIP(d_flags.alloc(sizeof(uint32_t) * (2 * rep_pad + 1)));
  OB_HIP(d_partial.alloc(sizeof(double) * (size_t)nc * rep_pad * ob::heck_probit_len(k)));
  OB_HIP(hipMemcpyAsync(d_cols.p, y, sizeof(double) * n, hipMemcpyHostToDevice, s));
  for (int j = 1; j < k; ++j)
    OB_HIP(hipMemcpyAsync(d_cols.d() + (size_t)j * n, x + (size_t)j * ldx, sizeof(double) * n, hipMemcpyHostToDevice, s));
  OB_HIP(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(uint32_t) * chunks.size(), hipMemcpyHostToDevice, s));
  ob_heck_seg h{};
  h.cols[0] = d_cols.d();
  h.ld[0] = n;
  h.n[0] = (uint32_t)n;
  h.tiles0 = tiles;
  h.ks = k;
  h.sz_col = 0;
  h.nb_rep = 1;
  h.chunks = d_chunks.as<uint32_t>();
  h.n_chunks = (int)nc;
  h.rep_pad = rep_pad;
  h.part_pad = rep_pad;
  h.n_reps = 1;
  h.gamma = d_gamma.d();
  h.hflags = d_flags.as<uint32_t>();
  h.active = h.hflags + 2 * rep_pad;
  h.partial = d_partial.d();
  h.max_iter = max_iter;
  h.tol = tol;
  int it = 0;
  OB_TRY(ob::probit_stage(h, s, &it, nullptr));
  uint32_t fl = 0;
  OB_HIP(hipMemcpyAsync(beta, h.gamma, sizeof(double) * k, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(&fl, h.hflags, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  if (fl & kFailed) return ob::fail(OB_E_LINALG, "Failed to solve Hessian system in Probit");
  if (converged) *converged = (fl & kDone) ? 1 : 0;
  if (iterations) *iterations = it;
  return OB_OK;
}

namespace {
__global__ void ob_normal_kernel(const double* z, int64_t n, double* pdf, double* cdf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p, c;
  npdf_ncdf(z[i], p, c);
  pdf[i] = p;
  cdf[i] = c;
}
}  // namespace

// Test hook (include/oaxaca_boot.h): npdf_ncdf, the probit's phi and Phi (Cody's erfc with one
// shared exponential), evaluated on the device at z[0 .. n).
extern "C" int ob_debug_normal(int device, const double* z, int64_t n, double* pdf, double* cdf) {
  if (n < 0 || (n && (!z || !pdf || !cdf))) return ob::fail(OB_E_INVALID, "bad arguments");
  if (n == 0) return OB_OK;
  OB_HIP(hipSetDevice(device));
  double* d = nullptr;
  OB_HIP(hipMalloc(&d, sizeof(double) * 3 * (size_t)n));
  int rc = OB_OK;
  do {
    if (hipMemcpy(d, z, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) { rc = ob::fail(OB_E_HIP, "copy"); break; }
    hipLaunchKernelGGL(ob_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, n, d + n, d + 2 * n);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { rc = ob::fail(OB_E_HIP, "launch"); break; }
    if (hipMemcpy(pdf, d + n, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cdf, d + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = ob::fail(OB_E_HIP, "copy back");
  } while (0);
  (void)hipFree(d);
  return rc;
}
