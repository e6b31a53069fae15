// ob_dfl.hip -- device kernels of DiNardo-Fortin-Lemieux reweighting (dfl.rs:34-195):
//
//   ob_logit_pass_kernel   one Newton pass of math/logit.rs:43-82 over column-major X: p = clamp(
//                          sigmoid(x beta)), the information matrix X^T diag(p (1 - p)) X and the
//                          gradient X^T (y - p), as per-wave partial sums
//   ob_ordered_sum_kernel  the partials of one sum added in unit order, then a fixed LDS tree
//                          (ob_device.hpp)
//   ob_logit_probs_kernel  p at a given beta (logit.rs:108-110, the unconverged exit)
//   ob_kde_kernel          sum_i w_i exp(-u^2 / 2), u = (x_g - d_i) / h (math/kde.rs:31-38), four
//                          grid points per thread over one chunk of the data
//   ob_kde_finish_kernel   the chunks of one grid point added in order, scaled by 1 / (sqrt(2 pi) h)
//
// The logit pass is a weighted SYRK with a short inner dimension: each wave owns 64-row sub-tiles,
// stages a sub-tile's K columns in its own LDS slice with lane = row (coalesced 512-byte column
// reads, x beta accumulated on the way), then reads the slice back in the operand shape of
// v_mfma_f64_16x16x4_f64 (lane = 4 rows x 16 columns): A = p (1 - p) x of column block I, B = x of
// column block J, one accumulator per block pair I <= J. The gradient rides on the A operand's
// loads (one VALU fma per column block and step). No floating atomics anywhere: a wave's sums are a
// function of its rows only, every partial lands in its own slot, and the reduce adds them in a
// fixed order, so two calls on the same input give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ob_device.hpp"
#include "ob_dfl.hpp"
#include "ob_hip.hpp"
#include "ob_linalg.hpp"
#include "ob_match.hpp"

namespace {

typedef double ob_d4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kLgWaves = kBlock / 64;
constexpr int kLgStride = 66;      // doubles per staged column: 64 rows + 2, so the 16 columns x 2 rows
                                   // a half-wave reads as an MFMA operand fall in 32 distinct 8-byte banks
constexpr int kLgRowVecs = 128;    // per wave: p (1 - p) and y - p of the sub-tile's 64 rows
constexpr int kLgMaxUnits = 4096;  // waves that carry partial sums (a function of n only)
constexpr int kKdeGp = 4;          // grid points per thread
constexpr int kKdeMaxChunks = 1024;

struct LogitArgs {
  const double* x;  // column-major n x k
  int64_t ldx;
  const double* y;
  const double* beta;
  double* probs;    // or nullptr
  int64_t n;
  int k;
  uint32_t nsub;    // 64-row sub-tiles
  uint32_t spu;     // sub-tiles per unit (wave)
  uint32_t units;
  double* partial;  // [k (k + 1) / 2 + k][units]
};

// LDS operations of one wave complete in issue order; waiting for the wave's own ones orders the
// lane = row writes before the operand-shaped reads of other lanes (and back).
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// logit.rs:15-17,45: sigmoid then clamp (a NaN stays a NaN, as f64::clamp keeps it). CLAMP = false is
// matching/logistic.rs:51,111, which has no clamp.
template <bool CLAMP = true>
__device__ __forceinline__ double logit_prob(double z) {
  const double p = 1.0 / (1.0 + exp(-z));
  if (!CLAMP) return p;
  return p < 1e-10 ? 1e-10 : (p > 1.0 - 1e-10 ? 1.0 - 1e-10 : p);
}

template <int NCB, bool CLAMP = true>
__global__ __launch_bounds__(kBlock) void ob_logit_pass_kernel(const LogitArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NC = 16 * NCB;
  constexpr int NP = NCB * (NCB + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t unit = blockIdx.x * kLgWaves + wave;
  if (unit >= a.units) return;  // whole waves only: no block barrier below
  double* xs = lds + (size_t)wave * (NC * kLgStride + kLgRowVecs);
  double* ws = xs + NC * kLgStride;
  double* rs = ws + 64;
  for (int c = a.k; c < NC; ++c) xs[c * kLgStride + lane] = 0.0;  // columns past K stay zero
  ob_d4 acc[NP];
  double g[NCB];
#pragma unroll
  for (int q = 0; q < NP; ++q) acc[q] = (ob_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < NCB; ++i) g[i] = 0.0;
  const int kq = lane >> 4, li = lane & 15;
  const uint32_t s0 = unit * a.spu, s1 = min(a.nsub, s0 + a.spu);
  for (uint32_t s = s0; s < s1; ++s) {
    const int64_t row = (int64_t)s * 64 + lane;
    const bool live = row < a.n;
    double eta = 0.0;
#pragma unroll 4
    for (int c = 0; c < a.k; ++c) {
      const double v = live ? a.x[(size_t)c * a.ldx + row] : 0.0;
      xs[c * kLgStride + lane] = v;
      eta = fma(v, a.beta[c], eta);
    }
    const double p = logit_prob<CLAMP>(eta);
    ws[lane] = live ? p * (1.0 - p) : 0.0;
    rs[lane] = live ? a.y[row] - p : 0.0;
    if (live && a.probs) a.probs[row] = p;
    wave_lds_sync();
#pragma unroll 2
    for (int ks = 0; ks < 16; ++ks) {
      const int r = 4 * ks + kq;
      const double wv = ws[r], rv = rs[r];
      double xv[NCB], av[NCB];
#pragma unroll
      for (int i = 0; i < NCB; ++i) {
        xv[i] = xs[(16 * i + li) * kLgStride + r];
        g[i] = fma(xv[i], rv, g[i]);
        av[i] = xv[i] * wv;
      }
      int q = 0;
#pragma unroll
      for (int i = 0; i < NCB; ++i)
#pragma unroll
        for (int j = i; j < NCB; ++j, ++q)
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], xv[j], acc[q], 0, 0, 0);
    }
    wave_lds_sync();
  }
  // D(I, J)[i][j] sits in lane (i % 4) * 16 + j, element i / 4: pair (16 I + i, 16 J + j), upper triangle
  const int k = a.k;
  int q = 0;
#pragma unroll
  for (int i = 0; i < NCB; ++i)
#pragma unroll
    for (int j = i; j < NCB; ++j, ++q) {
      const int b = 16 * j + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * i + kq + 4 * r;
        if (c <= b && b < k) {
          const int e = c * k - c * (c - 1) / 2 + (b - c);
          a.partial[(size_t)e * a.units + unit] = acc[q][r];
        }
      }
    }
  const int ep = k * (k + 1) / 2;
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    double v = g[i];  // rows = kq (mod 4) of column 16 i + li: add the four row classes
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    const int c = 16 * i + li;
    if (kq == 0 && c < k) a.partial[(size_t)(ep + c) * a.units + unit] = v;
  }
}

template <bool CLAMP = true>
__global__ __launch_bounds__(kBlock) void ob_logit_probs_kernel(const double* x, int64_t ldx, const double* beta,
                                                                 int64_t n, int k, double* probs) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= n) return;
  double eta = 0.0;
  for (int c = 0; c < k; ++c) eta = fma(x[(size_t)c * ldx + row], beta[c], eta);
  probs[row] = logit_prob<CLAMP>(eta);
}

// blockIdx.x: group of kKdeGp grid points, blockIdx.y: data chunk. partial: [n_grid][nchunks].
__global__ __launch_bounds__(kBlock) void ob_kde_kernel(const double* data, const double* w, double w_uniform,
                                                         int64_t n, const double* grid, int64_t n_grid, double h,
                                                         int64_t chunk, uint32_t nchunks, double* partial) {
  __shared__ double red[kBlock / 64][kKdeGp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g0 = (int64_t)blockIdx.x * kKdeGp;
  double xg[kKdeGp], acc[kKdeGp];
#pragma unroll
  for (int q = 0; q < kKdeGp; ++q) {
    xg[q] = grid[min(g0 + q, n_grid - 1)];
    acc[q] = 0.0;
  }
  const int64_t i0 = (int64_t)blockIdx.y * chunk, i1 = min(n, i0 + chunk);
  for (int64_t i = i0 + tid; i < i1; i += kBlock) {
    const double d = data[i];
    const double wi = w ? w[i] : w_uniform;
#pragma unroll
    for (int q = 0; q < kKdeGp; ++q) {
      const double u = (xg[q] - d) / h;
      acc[q] = fma(wi, exp(-0.5 * u * u), acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < kKdeGp; ++q) {
    double v = acc[q];  // not wave_sum(): the call schedules this kernel differently
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (tid < kKdeGp && g0 + tid < n_grid) {
    double s = red[0][tid];
    for (int wv = 1; wv < kBlock / 64; ++wv) s += red[wv][tid];
    partial[(size_t)(g0 + tid) * nchunks + blockIdx.y] = s;
  }
}

__global__ __launch_bounds__(kBlock) void ob_kde_finish_kernel(const double* partial, uint32_t nchunks, int64_t n_grid,
                                                                double h, double* density) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n_grid) return;
  double s = 0.0;
  for (uint32_t c = 0; c < nchunks; ++c) s += partial[(size_t)g * nchunks + c];
  density[g] = s * 0.3989422804014327 / h;  // 1 / sqrt(2 pi): gaussian_kernel's factor (kde.rs:4-6)
}

template <int NCB, bool CLAMP = true>
int launch_logit_pass(const LogitArgs& a, hipStream_t s) {
  const size_t lds = sizeof(double) * kLgWaves * (16 * NCB * kLgStride + kLgRowVecs);
  OB_HIP(hipFuncSetAttribute((const void*)ob_logit_pass_kernel<NCB, CLAMP>,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((ob_logit_pass_kernel<NCB, CLAMP>), dim3((a.units + kLgWaves - 1) / kLgWaves), dim3(kBlock), lds, s, a);
  OB_HIP(hipGetLastError());
  return OB_OK;
}

// The Newton loop of both logits. MATCH = false: math/logit.rs:31-118 (dfl_logit). MATCH = true:
// matching/logistic.rs:31-113 (match_logistic): no clamp, a 1e-6 ridge, LU, scores at the final beta.
template <bool MATCH>
int logit_newton(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int k, int max_iter, double tol,
                 double* beta, double* probs, ob::LogitInfo* info) {
  using namespace ob;
  if (!ctx || !x || !y || !beta || !info) return fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || k <= 0 || ldx < n || max_iter < 0) return fail(OB_E_INVALID, "bad logit dimensions");
  if (k > kLogitMaxK)
    return fail(OB_E_UNSUPPORTED, "logit: %d columns, the kernel takes at most %d (intercept included)", k, kLogitMaxK);
  if ((n + 63) / 64 > (int64_t)0x7fffffff) return fail(OB_E_UNSUPPORTED, "logit: too many rows");
  *info = LogitInfo();
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int ne = k * (k + 1) / 2 + k;
  LogitArgs a = {};
  a.nsub = (uint32_t)((n + 63) / 64);
  a.spu = (a.nsub + kLgMaxUnits - 1) / kLgMaxUnits;
  a.units = (a.nsub + a.spu - 1) / a.spu;
  DevBuf dx, dy, db, dp, dpart, dsum;
  OB_HIP(dx.alloc(sizeof(double) * (size_t)n * k));
  OB_HIP(dy.alloc(sizeof(double) * (size_t)n));
  OB_HIP(db.alloc(sizeof(double) * k));
  OB_HIP(dp.alloc(sizeof(double) * (size_t)n));
  OB_HIP(dpart.alloc(sizeof(double) * (size_t)ne * a.units));
  OB_HIP(dsum.alloc(sizeof(double) * ne));
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipMemcpy2DAsync(dx.p, sizeof(double) * (size_t)n, x, sizeof(double) * (size_t)ldx, sizeof(double) * (size_t)n,
                          (size_t)k, hipMemcpyHostToDevice, st));
  OB_HIP(hipMemcpyAsync(dy.p, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  a.x = dx.d();
  a.ldx = n;
  a.y = dy.d();
  a.beta = db.d();
  a.probs = dp.d();
  a.n = n;
  a.k = k;
  a.partial = dpart.d();
  const int ncb = (k + 15) / 16;
  std::vector<double> b(k, 0.0), sums(ne), m((size_t)k * k), step(k);
  bool converged = false;
  int iterations = max_iter;
  for (int iter = 0; iter < max_iter; ++iter) {
    OB_HIP(hipMemcpyAsync(db.p, b.data(), sizeof(double) * k, hipMemcpyHostToDevice, st));
    OB_HIP(hipEventRecord(ev.e[0], st));
    switch (ncb) {
      case 1: OB_TRY((launch_logit_pass<1, !MATCH>(a, st))); break;
      case 2: OB_TRY((launch_logit_pass<2, !MATCH>(a, st))); break;
      case 3: OB_TRY((launch_logit_pass<3, !MATCH>(a, st))); break;
      default: OB_TRY((launch_logit_pass<4, !MATCH>(a, st))); break;
    }
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(ne), dim3(kSumBlock), 0, st, dpart.d(), a.units, dsum.d());
    OB_HIP(hipGetLastError());
    OB_HIP(hipEventRecord(ev.e[1], st));
    OB_HIP(hipMemcpyAsync(sums.data(), dsum.p, sizeof(double) * ne, hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    info->ms += ms;
    // information matrix X^T W X (lower triangle from the upper-triangle pair sums) and gradient
    for (int c = 0; c < k; ++c)
      for (int r = c; r < k; ++r) m[r + (size_t)c * k] = sums[c * k - c * (c - 1) / 2 + (r - c)];
    for (int c = 0; c < k; ++c) step[c] = sums[k * (k + 1) / 2 + c];
    if (MATCH) {
      for (int c = 0; c < k; ++c) {
        for (int r = 0; r < c; ++r) m[r + (size_t)c * k] = m[c + (size_t)r * k];
        m[c + (size_t)c * k] += 1e-6;  // logistic.rs:89-91
      }
      if (!host_lu_solve(m, k, step))  // logistic.rs:95
        return fail(OB_E_DIAG, "%sHessian is singular", error_prefix(OB_E_DIAG));
    } else if (!chol_factor_solve(m.data(), k, step.data(), BackSub::Dot)) {  // logit.rs:88-95
      return fail(OB_E_LINALG, "%sFailed to solve Information Matrix in Logit. Perfect separation?",
                  error_prefix(OB_E_LINALG));
    }
    double nrm = 0.0;
    for (int c = 0; c < k; ++c) {
      b[c] += step[c];
      nrm += step[c] * step[c];
    }
    if (std::sqrt(nrm) < tol) {  // logit.rs:98-105: the probabilities stay those of this iteration's start
      converged = true;
      iterations = iter + 1;
      break;
    }
  }
  if ((MATCH || !converged) && probs) {  // logit.rs:108-110; logistic.rs:109-112 always scores at the final beta
    OB_HIP(hipMemcpyAsync(db.p, b.data(), sizeof(double) * k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ob_logit_probs_kernel<!MATCH>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dx.d(),
                       n, db.d(), n, k, dp.d());
    OB_HIP(hipGetLastError());
  }
  if (probs) OB_HIP(hipMemcpyAsync(probs, dp.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  std::copy(b.begin(), b.end(), beta);
  info->converged = converged ? 1 : 0;
  info->iterations = iterations;
  return OB_OK;
}

}  // namespace

namespace ob {

int dfl_logit(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int k, int max_iter, double tol,
              double* beta, double* probs, LogitInfo* info) {
  return logit_newton<false>(ctx, x, ldx, y, n, k, max_iter, tol, beta, probs, info);
}

int match_logistic(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int k, int max_iter,
                   double tol, double* beta, double* probs, LogitInfo* info) {
  return logit_newton<true>(ctx, x, ldx, y, n, k, max_iter, tol, beta, probs, info);
}

int dfl_kde(ob_ctx* ctx, const double* data, const double* wnorm, int64_t n, const double* grid, int64_t n_grid,
            double bandwidth, double* density, double* ms_out) {
  if (ms_out) *ms_out = 0.0;
  if (!ctx || n < 0 || n_grid < 0 || (n && !data) || (n_grid && (!grid || !density)))
    return fail(OB_E_INVALID, "bad kde arguments");
  if (n_grid == 0) return OB_OK;
  if (n == 0) {  // an empty sum (kde.rs:32-37)
    for (int64_t g = 0; g < n_grid; ++g) density[g] = 0.0 / bandwidth;
    return OB_OK;
  }
  const int64_t ggroups = (n_grid + kKdeGp - 1) / kKdeGp;
  if (ggroups > (int64_t)0x7fffffff) return fail(OB_E_UNSUPPORTED, "kde: too many grid points");
  // chunks of the data: enough blocks to fill the chip when the grid is short (a function of n and n_grid only)
  const int64_t want = std::max<int64_t>(1, 4096 / ggroups);
  const uint32_t nchunks0 = (uint32_t)std::min<int64_t>(std::min<int64_t>((n + kBlock - 1) / kBlock, want), kKdeMaxChunks);
  const int64_t chunk = (n + nchunks0 - 1) / nchunks0;
  const uint32_t nchunks = (uint32_t)((n + chunk - 1) / chunk);
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dd, dw, dg, dpart, dout;
  OB_HIP(dd.alloc(sizeof(double) * (size_t)n));
  if (wnorm) OB_HIP(dw.alloc(sizeof(double) * (size_t)n));
  OB_HIP(dg.alloc(sizeof(double) * (size_t)n_grid));
  OB_HIP(dpart.alloc(sizeof(double) * (size_t)n_grid * nchunks));
  OB_HIP(dout.alloc(sizeof(double) * (size_t)n_grid));
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipMemcpyAsync(dd.p, data, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  if (wnorm) OB_HIP(hipMemcpyAsync(dw.p, wnorm, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  OB_HIP(hipMemcpyAsync(dg.p, grid, sizeof(double) * (size_t)n_grid, hipMemcpyHostToDevice, st));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(ob_kde_kernel, dim3((unsigned)ggroups, nchunks), dim3(kBlock), 0, st, dd.d(),
                     wnorm ? dw.d() : (const double*)nullptr, 1.0 / (double)n, n, dg.d(), n_grid, bandwidth, chunk,
                     nchunks, dpart.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_kde_finish_kernel, dim3((unsigned)((n_grid + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     dpart.d(), nchunks, n_grid, bandwidth, dout.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], st));
  OB_HIP(hipMemcpyAsync(density, dout.p, sizeof(double) * (size_t)n_grid, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  if (ms_out) *ms_out = ms;
  return OB_OK;
}

}  // namespace ob
