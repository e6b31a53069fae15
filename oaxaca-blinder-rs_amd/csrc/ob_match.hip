// ob_match.hip -- device kernels of nearest-neighbour matching (matching/engine.rs:113-229):
//
//   ob_knn_kernel           every (query, control) squared distance of one control chunk in the
//                           kdtree crate's order, 0 + t_0 t_0 + t_1 t_1 + ... with separate multiplies
//                           and adds, and the chunk's k best by (distance, position) in registers
//   ob_knn_merge_kernel     the chunks' lists of one query merged by the same key
//   ob_match_count_kernel   how often each control was chosen (integer atomics)
//   ob_match_cov_kernel     centred cross-products of the control rows (distance.rs:36-44), per-block
//   ob_ordered_sum_kernel   the blocks' partials of one cross-product added in a fixed order
//                           (ob_device.hpp)
//   ob_match_xl_kernel      X L, the Mahalanobis transform (engine.rs:174-175)
//   ob_match_pack_kernel    controls to row-major rows padded to the kernel's dimension bucket
//   ob_match_finite_kernel  the stricter rule: a non-finite coordinate is an error
//
// The distance pass is the difference form on the f64 VALU: one thread owns one query
// with its coordinates in registers; the control coordinates are uniform across the block, so they
// arrive by scalar loads and feed the VALU as scalar operands. A thread's list is a function of its
// query and of the chunk bounds, which depend on the input sizes only; the merge reads the chunks in
// order. No floating atomics anywhere, so two calls on the same input give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <type_traits>
#include <vector>

#include "ob_device.hpp"
#include "ob_hip.hpp"
#include "ob_match.hpp"
#include "ob_options.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kKnnFill = 2048;       // blocks wanted before the controls are split into chunks
constexpr int kKnnMaxChunks = 256;
constexpr int kKnnMinChunk = 256;    // controls per chunk at least
constexpr int kCovRows = 64;         // rows per LDS tile
constexpr int kCovStride = kCovRows + 1;
constexpr int kCovMaxBlocks = 512;
constexpr int kCovAcc = OB_MATCH_MAX_DIM * OB_MATCH_MAX_DIM / kBlock;  // pair sums per thread

struct KnnArgs {
  const double* q;  // column-major n_q x dim, ld = n_q
  const double* c;  // row-major n_c x DP, columns past dim are zero
  int64_t n_q;
  int32_t n_c;
  int dim, k;
  int32_t chunk;    // controls per chunk
  uint32_t nchunks;
  double* pd;       // [nchunks][k][n_q]
  int32_t* pi;
};

// One slot bubbles towards the front by the key (distance, position); static indices only, so the
// list stays in registers.
template <int KB>
__device__ __forceinline__ void knn_insert(double (&bd)[KB], int32_t (&bi)[KB], double d, int32_t j) {
  if (!(d < bd[KB - 1] || (d == bd[KB - 1] && j < bi[KB - 1]))) return;
  bd[KB - 1] = d;
  bi[KB - 1] = j;
#pragma unroll
  for (int p = KB - 1; p > 0; --p) {
    const bool sw = bd[p] < bd[p - 1] || (bd[p] == bd[p - 1] && bi[p] < bi[p - 1]);
    const double dl = sw ? bd[p] : bd[p - 1], dh = sw ? bd[p - 1] : bd[p];
    const int32_t il = sw ? bi[p] : bi[p - 1], ih = sw ? bi[p - 1] : bi[p];
    bd[p - 1] = dl;
    bd[p] = dh;
    bi[p - 1] = il;
    bi[p] = ih;
  }
}

// blockIdx.x: 256 queries, blockIdx.y: control chunk.
template <int DP, int KB>
__global__ __launch_bounds__(kBlock) void ob_knn_kernel(const KnnArgs a) {
#pragma clang fp contract(off)  // the reference's sum has no FMA (kdtree's squared_euclidean)
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = row < a.n_q;
  double x[DP];
#pragma unroll
  for (int c = 0; c < DP; ++c) x[c] = (live && c < a.dim) ? a.q[(size_t)c * a.n_q + row] : 0.0;
  double bd[KB];
  int32_t bi[KB];
#pragma unroll
  for (int s = 0; s < KB; ++s) {
    bd[s] = std::numeric_limits<double>::infinity();
    bi[s] = INT_MAX;
  }
  const int32_t j0 = (int32_t)min((int64_t)a.n_c, (int64_t)blockIdx.y * a.chunk);
  const int32_t j1 = (int32_t)min((int64_t)a.n_c, (int64_t)j0 + a.chunk);
  const double* __restrict__ cp = a.c + (size_t)j0 * DP;
#pragma unroll 2
  for (int32_t j = j0; j < j1; ++j, cp += DP) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < DP; ++c) {  // a padded column adds 0 * 0 = +0, which changes nothing
      const double t = x[c] - cp[c];
      const double t2 = t * t;
      s = s + t2;
    }
    if (s <= bd[KB - 1]) knn_insert<KB>(bd, bi, s, j);
  }
  if (!live) return;
#pragma unroll
  for (int s = 0; s < KB; ++s)
    if (s < a.k) {
      const size_t o = ((size_t)blockIdx.y * a.k + s) * (size_t)a.n_q + row;
      a.pd[o] = bd[s];
      a.pi[o] = bi[s];
    }
}

template <int KB>
__global__ __launch_bounds__(kBlock) void ob_knn_merge_kernel(const double* pd, const int32_t* pi, uint32_t nchunks,
                                                               int64_t n_q, int k, int64_t* idx, double* dist2) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= n_q) return;
  double bd[KB];
  int32_t bi[KB];
#pragma unroll
  for (int s = 0; s < KB; ++s) {
    bd[s] = std::numeric_limits<double>::infinity();
    bi[s] = INT_MAX;
  }
  for (uint32_t ch = 0; ch < nchunks; ++ch)
    for (int s = 0; s < k; ++s) {
      const size_t o = ((size_t)ch * k + s) * (size_t)n_q + row;
      const int32_t j = pi[o];
      if (j == INT_MAX) break;  // the chunk had fewer than k controls
      knn_insert<KB>(bd, bi, pd[o], j);
    }
#pragma unroll
  for (int s = 0; s < KB; ++s)
    if (s < k) {
      const bool none = bi[s] == INT_MAX;
      idx[(size_t)row * k + s] = none ? (int64_t)-1 : (int64_t)bi[s];
      dist2[(size_t)row * k + s] = none ? std::numeric_limits<double>::infinity() : bd[s];
    }
}

__global__ __launch_bounds__(kBlock) void ob_match_count_kernel(const int64_t* idx, int64_t total, int64_t n_c,
                                                                 uint32_t* counts) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= total) return;
  const int64_t j = idx[t];
  if (j >= 0 && j < n_c) atomicAdd(&counts[j], 1u);
}

// dst[row][c] = c < dim ? src[c][row] : 0, dst rows DP wide. One thread per destination entry.
__global__ __launch_bounds__(kBlock) void ob_match_pack_kernel(const double* src, int64_t n, int dim, int dp,
                                                                double* dst) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n * dp) return;
  const int64_t row = t / dp;
  const int c = (int)(t - row * dp);
  dst[t] = c < dim ? src[(size_t)c * n + row] : 0.0;
}

__global__ __launch_bounds__(kBlock) void ob_match_finite_kernel(const double* v, int64_t total, uint32_t* flag) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t < total && !__builtin_isfinite(v[t])) atomicOr(flag, 1u);
}

// partial[e][block] for e = c1 * d + c2: sum over the block's rows of (x[c1] - mean[c1]) (x[c2] - mean[c2]).
// Block b takes the 64-row tiles b, b + gridDim.x, ...; a thread adds its pairs' rows in order.
__global__ __launch_bounds__(kBlock) void ob_match_cov_kernel(const double* x, int64_t n, int d, const double* mean,
                                                               double* partial) {
  __shared__ double t[OB_MATCH_MAX_DIM * kCovStride];
  const int tid = threadIdx.x, dd = d * d;
  double acc[kCovAcc];
#pragma unroll
  for (int q = 0; q < kCovAcc; ++q) acc[q] = 0.0;
  const int64_t ntiles = (n + kCovRows - 1) / kCovRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
    for (int i = tid; i < kCovRows * d; i += kBlock) {
      const int r = i & (kCovRows - 1), c = i / kCovRows;
      const int64_t row = tile * kCovRows + r;
      t[c * kCovStride + r] = row < n ? x[(size_t)c * n + row] - mean[c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kCovAcc; ++q) {
      const int e = tid + q * kBlock;
      if (e < dd) {
        const double* a = t + (e / d) * kCovStride;
        const double* b = t + (e % d) * kCovStride;
        double s = acc[q];
        for (int r = 0; r < kCovRows; ++r) s = fma(a[r], b[r], s);
        acc[q] = s;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kCovAcc; ++q) {
    const int e = tid + q * kBlock;
    if (e < dd) partial[(size_t)e * gridDim.x + blockIdx.x] = acc[q];
  }
}

// out[c][row] = sum_j x[j][row] l[j][c] (both column-major, l is d x d). blockIdx.y: the column c.
__global__ __launch_bounds__(kBlock) void ob_match_xl_kernel(const double* x, int64_t n, int d, const double* l,
                                                              double* out) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= n) return;
  const int c = blockIdx.y;
  double s = 0.0;
  for (int j = 0; j < d; ++j) s = fma(x[(size_t)j * n + row], l[j + (size_t)c * d], s);
  out[(size_t)c * n + row] = s;
}

// Calls f with k's bucket of the neighbour list, 1, 4, 8 or 16, as a compile-time constant.
template <class F>
void with_k_bucket(int k, F f) {
  if (k <= 1) f(std::integral_constant<int, 1>());
  else if (k <= 4) f(std::integral_constant<int, 4>());
  else if (k <= 8) f(std::integral_constant<int, 8>());
  else f(std::integral_constant<int, 16>());
}

template <int DP>
int launch_knn(const KnnArgs& a, dim3 grid, hipStream_t s) {
  with_k_bucket(a.k, [&](auto kb) {
    hipLaunchKernelGGL((ob_knn_kernel<DP, decltype(kb)::value>), grid, dim3(kBlock), 0, s, a);
  });
  OB_HIP(hipGetLastError());
  return OB_OK;
}

// The padded dimension the distance kernel is compiled for.
int dim_bucket(int dim) {
  for (int b : {4, 8, 16, 20, 32, 48}) if (dim <= b) return b;
  return 64;
}

// Replaces the column-major compact x (n x d) by x l on the device.
int transform(hipStream_t st, DevBuf& x, int64_t n, int d, const double* dl) {
  if (n == 0) return OB_OK;
  DevBuf out;
  OB_HIP(out.alloc(sizeof(double) * (size_t)n * d));
  hipLaunchKernelGGL(ob_match_xl_kernel, dim3(blocks_for(n), d), dim3(kBlock), 0, st, x.d(), n, d, dl, out.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipStreamSynchronize(st));
  std::swap(x.p, out.p);
  std::swap(x.cap, out.cap);
  return OB_OK;
}

}  // namespace

namespace ob {

int match_knn(ob_ctx* ctx, const double* q, int64_t ldq, int64_t n_q, const double* c, int64_t ldc, int64_t n_c, int dim,
              int k, bool mahalanobis, int64_t* idx, double* dist2, uint32_t* counts, MatchTiming* timing) {
  if (timing) *timing = MatchTiming();
  if (!ctx || n_q < 0 || n_c < 0 || k < 0 || dim <= 0 || ldq < n_q || ldc < n_c || (n_q && !q) || (n_c && !c) ||
      (n_q && k && (!idx || !dist2)))
    return fail(OB_E_INVALID, "bad knn arguments");
  if (dim > OB_MATCH_MAX_DIM)
    return fail(OB_E_UNSUPPORTED, "matching: %d covariates, the kernel takes at most %d", dim, OB_MATCH_MAX_DIM);
  if (k > OB_MATCH_MAX_K)
    return fail(OB_E_UNSUPPORTED, "matching: k = %d, the kernel keeps at most %d neighbours", k, OB_MATCH_MAX_K);
  if (n_c > (int64_t)INT_MAX - 1 || n_q > ((int64_t)1 << 38))
    return fail(OB_E_UNSUPPORTED, "matching: too many rows");
  if (mahalanobis && n_c < 2)  // distance.rs:32-34
    return fail(OB_E_DIAG, "%sNot enough data points to calculate covariance", error_prefix(OB_E_DIAG));
  for (int64_t i = 0; i < n_q * k; ++i) {
    idx[i] = -1;
    dist2[i] = std::numeric_limits<double>::infinity();
  }
  if (counts) std::fill(counts, counts + n_c, 0u);
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events<3> ev;
  OB_HIP(ev.create());
  DevBuf dq, dc, dflag;
  OB_HIP(dq.alloc(sizeof(double) * (size_t)n_q * dim));
  OB_HIP(dc.alloc(sizeof(double) * (size_t)n_c * dim));
  OB_HIP(dflag.alloc(sizeof(uint32_t)));
  OB_HIP(hipEventRecord(ev.e[0], st));
  OB_HIP(hipMemsetAsync(dflag.p, 0, sizeof(uint32_t), st));
  if (n_q)
    OB_HIP(hipMemcpy2DAsync(dq.p, sizeof(double) * (size_t)n_q, q, sizeof(double) * (size_t)ldq,
                              sizeof(double) * (size_t)n_q, (size_t)dim, hipMemcpyHostToDevice, st));
  if (n_c)
    OB_HIP(hipMemcpy2DAsync(dc.p, sizeof(double) * (size_t)n_c, c, sizeof(double) * (size_t)ldc,
                              sizeof(double) * (size_t)n_c, (size_t)dim, hipMemcpyHostToDevice, st));
  if (mahalanobis) {
    // mean on the host in row order, centred cross-products on the device (distance.rs:36-44)
    std::vector<double> mean(dim), s((size_t)dim * dim), l;
    for (int j = 0; j < dim; ++j) {
      double sum = 0.0;
      for (int64_t r = 0; r < n_c; ++r) sum += c[(size_t)j * ldc + r];
      mean[j] = sum / (double)n_c;
    }
    const unsigned nblk = (unsigned)std::min<int64_t>((n_c + kCovRows - 1) / kCovRows, kCovMaxBlocks);
    DevBuf dmean, dpart, dsum, dl;
    OB_HIP(dmean.alloc(sizeof(double) * dim));
    OB_HIP(dpart.alloc(sizeof(double) * (size_t)dim * dim * nblk));
    OB_HIP(dsum.alloc(sizeof(double) * (size_t)dim * dim));
    OB_HIP(dl.alloc(sizeof(double) * (size_t)dim * dim));
    OB_HIP(hipMemcpyAsync(dmean.p, mean.data(), sizeof(double) * dim, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ob_match_cov_kernel, dim3(nblk), dim3(kBlock), 0, st, dc.d(), n_c, dim, dmean.d(), dpart.d());
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(dim * dim), dim3(kSumBlock), 0, st, dpart.d(), nblk, dsum.d());
    OB_HIP(hipGetLastError());
    OB_HIP(hipMemcpyAsync(s.data(), dsum.p, sizeof(double) * (size_t)dim * dim, hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    for (double& v : s) v /= (double)(n_c - 1);
    OB_TRY(mahalanobis_factor(s, dim, l));
    OB_HIP(hipMemcpyAsync(dl.p, l.data(), sizeof(double) * (size_t)dim * dim, hipMemcpyHostToDevice, st));
    OB_TRY(transform(st, dq, n_q, dim, dl.d()));
    OB_TRY(transform(st, dc, n_c, dim, dl.d()));
  }
  if (n_q * dim)
    hipLaunchKernelGGL(ob_match_finite_kernel, dim3(blocks_for(n_q * dim)), dim3(kBlock), 0, st, dq.d(), n_q * dim,
                       dflag.as<uint32_t>());
  if (n_c * dim)
    hipLaunchKernelGGL(ob_match_finite_kernel, dim3(blocks_for(n_c * dim)), dim3(kBlock), 0, st, dc.d(), n_c * dim,
                       dflag.as<uint32_t>());
  OB_HIP(hipGetLastError());
  uint32_t flag = 0;
  OB_HIP(hipMemcpyAsync(&flag, dflag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  if (flag)
    return fail(OB_E_DIAG, "%snon-finite covariate in a treated or control row%s", error_prefix(OB_E_DIAG),
                mahalanobis ? " after the Mahalanobis transform" : "");
  if (n_q == 0 || n_c == 0 || k == 0) return OB_OK;  // engine.rs:196-209 selects nothing

  // chunks of the controls: enough blocks to fill the chip when the queries are few (a function of
  // n_q and n_c only, or of the match_chunks option that the tests use to force either path)
  const int64_t qblocks = (n_q + kBlock - 1) / kBlock;
  int64_t want = std::min<int64_t>(std::max<int64_t>(1, kKnnFill / qblocks),
                                   std::min<int64_t>(kKnnMaxChunks, std::max<int64_t>(1, n_c / kKnnMinChunk)));
  const int forced = opt_int(Opt::MatchChunks, 0);
  if (forced > 0) want = std::min<int64_t>(std::min<int64_t>(forced, n_c), 65535);
  const int64_t chunk = (n_c + want - 1) / want;
  const uint32_t nchunks = (uint32_t)((n_c + chunk - 1) / chunk);
  const int dp = dim_bucket(dim);
  DevBuf dpack, dpd, dpi, didx, ddist, dcnt;
  OB_HIP(dpack.alloc(sizeof(double) * (size_t)n_c * dp));
  OB_HIP(dpd.alloc(sizeof(double) * (size_t)nchunks * k * n_q));
  OB_HIP(dpi.alloc(sizeof(int32_t) * (size_t)nchunks * k * n_q));
  OB_HIP(didx.alloc(sizeof(int64_t) * (size_t)n_q * k));
  OB_HIP(ddist.alloc(sizeof(double) * (size_t)n_q * k));
  hipLaunchKernelGGL(ob_match_pack_kernel, dim3(blocks_for(n_c * dp)), dim3(kBlock), 0, st, dc.d(), n_c, dim, dp,
                     dpack.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], st));
  KnnArgs a = {};
  a.q = dq.d();
  a.c = dpack.d();
  a.n_q = n_q;
  a.n_c = (int32_t)n_c;
  a.dim = dim;
  a.k = k;
  a.chunk = (int32_t)chunk;
  a.nchunks = nchunks;
  a.pd = dpd.d();
  a.pi = dpi.as<int32_t>();
  const dim3 grid((unsigned)qblocks, nchunks);
  switch (dp) {
    case 4: OB_TRY(launch_knn<4>(a, grid, st)); break;
    case 8: OB_TRY(launch_knn<8>(a, grid, st)); break;
    case 16: OB_TRY(launch_knn<16>(a, grid, st)); break;
    case 20: OB_TRY(launch_knn<20>(a, grid, st)); break;
    case 32: OB_TRY(launch_knn<32>(a, grid, st)); break;
    case 48: OB_TRY(launch_knn<48>(a, grid, st)); break;
    default: OB_TRY(launch_knn<64>(a, grid, st)); break;
  }
  int64_t* oidx = didx.as<int64_t>();
  with_k_bucket(k, [&](auto kb) {
    hipLaunchKernelGGL(ob_knn_merge_kernel<decltype(kb)::value>, dim3((unsigned)qblocks), dim3(kBlock), 0, st, a.pd,
                       a.pi, nchunks, n_q, k, oidx, ddist.d());
  });
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[2], st));
  if (counts) {
    OB_HIP(dcnt.alloc(sizeof(uint32_t) * (size_t)n_c));
    OB_HIP(hipMemsetAsync(dcnt.p, 0, sizeof(uint32_t) * (size_t)n_c, st));
    hipLaunchKernelGGL(ob_match_count_kernel, dim3(blocks_for(n_q * k)), dim3(kBlock), 0, st, oidx, n_q * k, n_c,
                       dcnt.as<uint32_t>());
    OB_HIP(hipGetLastError());
    OB_HIP(hipMemcpyAsync(counts, dcnt.p, sizeof(uint32_t) * (size_t)n_c, hipMemcpyDeviceToHost, st));
  }
  OB_HIP(hipMemcpyAsync(idx, didx.p, sizeof(int64_t) * (size_t)n_q * k, hipMemcpyDeviceToHost, st));
  OB_HIP(hipMemcpyAsync(dist2, ddist.p, sizeof(double) * (size_t)n_q * k, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  if (timing) {
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    timing->prep_ms = ms;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
    timing->knn_ms = ms;
  }
  return OB_OK;
}

}  // namespace ob
