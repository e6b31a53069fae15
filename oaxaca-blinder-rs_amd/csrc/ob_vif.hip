// ob_vif.hip -- device passes of the VIF collinearity diagnostic (math/diagnostics.rs:29-109). The
// reference runs K auxiliary OLS fits of n rows each; all of them share one extended Gram, so two
// n K^2 passes on the f64 matrix units do the same work:
//
//   ob_vif_gram_kernel     G = Xe^T Xe for Xe = [x_0..x_{K-1}, 1] over column-major X, upper triangle,
//                          as per-block partial sums
//   ob_vif_resid_kernel    R = Xe B' for B' = [I; 0] - B, B the (K + 1) x K coefficients of the host
//                          solves (so r_ij = x_ij - xe_i . B_j, an explicit residual, never G_jj - b'beta),
//                          squared and summed per column in the epilogue
//   ob_vif_sstot_kernel    sum_i (x_ij - mean_j)^2 per column
//   ob_ordered_sum_kernel  the partials of one sum added in unit order, then a fixed LDS tree
//                          (ob_device.hpp)
//
// The Gram is a SYRK with up to 8 column blocks of 16: 36 block pairs, 144 f64 x 4 accumulators, more
// than one wave holds. A block of four waves stages a 64-row sub-tile of every column ONCE in LDS
// (lane = row, coalesced 512-byte column reads, the stride of ob_dfl.hip) and deals the block pairs
// round-robin over its waves, at most 9 accumulators each; every wave reads its operands from the
// shared tile in the shape of v_mfma_f64_16x16x4_f64. X is read from HBM once, not once per wave.
//
// The residual pass keeps B' (at most 124 x 144 f64) in LDS for the whole block and streams X through
// registers in the A-operand shape (16 rows x 4 columns per step, 128-byte segments), never through
// LDS: a wave owns a 16-row block, walks the K + 1 columns four at a time and feeds up to 8 column-block
// accumulators, squares them and keeps per-lane column sums across its row blocks.
//
// No floating atomics: a wave's sums are a function of its rows only, every partial lands in its own
// slot, the unit counts follow from the shape alone, and the reduce adds in a fixed order, so two
// calls on the same input give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ob_device.hpp"
#include "ob_hip.hpp"
#include "ob_vif.hpp"

namespace {

typedef double ob_d4 __attribute__((ext_vector_type(4)));

constexpr int kGrBlock = 256;
constexpr int kGrWaves = kGrBlock / 64;
constexpr int kGrStride = 66;     // doubles per staged column: 64 rows + 2 (ob_dfl.hip's kLgStride)
constexpr int kGrMaxAcc = 9;      // block pairs per wave: ceil(36 / 4)
constexpr int kGrMaxUnits = 512;  // blocks that carry partial sums (a function of n only)
constexpr int kRsBlock = 512;
constexpr int kRsWaves = kRsBlock / 64;
constexpr int kRsMaxJb = 8;       // 16-column blocks of the K residual columns
constexpr int kRsMaxUnits = 512;
constexpr int kRsRedCols = 16 * kRsMaxJb;
constexpr int kTtBlock = 256;
constexpr int kTtMaxUnits = 256;

struct GramArgs {
  const double* x;  // device, column-major n x k
  int64_t ldx;
  int64_t n;
  int k;
  int ncb;          // 16-column blocks of the k + 1 columns
  uint32_t nsub;    // 64-row sub-tiles
  uint32_t spu;     // sub-tiles per unit (block)
  uint32_t units;
  double* partial;  // [(k + 1)(k + 2) / 2][units]
};

__global__ __launch_bounds__(kGrBlock) void ob_vif_gram_kernel(const GramArgs a) {
  extern __shared__ __attribute__((aligned(16))) double xs[];  // [16 ncb][kGrStride]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, li = lane & 15;
  const int k = a.k, k1 = a.k + 1, ncb = a.ncb, np = ncb * (ncb + 1) / 2;
  const uint32_t unit = blockIdx.x;
  // this wave's block pairs: q = wave, wave + 4, .. in the row-major order of the upper triangle
  int bi[kGrMaxAcc], bj[kGrMaxAcc];
  ob_d4 acc[kGrMaxAcc];
#pragma unroll
  for (int t = 0; t < kGrMaxAcc; ++t) {
    int rem = wave + kGrWaves * t, i = 0;
    if (rem < np)
      while (rem >= ncb - i) {
        rem -= ncb - i;
        ++i;
      }
    bi[t] = i;
    bj[t] = i + rem;
    acc[t] = (ob_d4){0.0, 0.0, 0.0, 0.0};
  }
  const int nacc = wave < np ? (np - wave + kGrWaves - 1) / kGrWaves : 0;
  for (int c = k1 + wave; c < 16 * ncb; c += kGrWaves) xs[c * kGrStride + lane] = 0.0;  // columns past K + 1 stay zero
  const uint32_t s0 = unit * a.spu, s1 = min(a.nsub, s0 + a.spu);
  for (uint32_t s = s0; s < s1; ++s) {
    const int64_t row = (int64_t)s * 64 + lane;
    const bool live = row < a.n;
    for (int c = wave; c < k1; c += kGrWaves)
      xs[c * kGrStride + lane] = live ? (c < k ? a.x[(size_t)c * a.ldx + row] : 1.0) : 0.0;
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < 16; ++ks) {
      const int r = li * kGrStride + 4 * ks + kq;
#pragma unroll
      for (int t = 0; t < kGrMaxAcc; ++t)
        if (t < nacc)
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[16 * bi[t] * kGrStride + r], xs[16 * bj[t] * kGrStride + r],
                                                        acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  // D(I, J)[i][j] sits in lane (i % 4) * 16 + j, element i / 4: pair (16 I + i, 16 J + j), upper triangle
#pragma unroll
  for (int t = 0; t < kGrMaxAcc; ++t)
    if (t < nacc) {
      const int b = 16 * bj[t] + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * bi[t] + kq + 4 * r;
        if (c <= b && b < k1) {
          const int e = c * k1 - c * (c - 1) / 2 + (b - c);
          a.partial[(size_t)e * a.units + unit] = acc[t][r];
        }
      }
    }
}

struct ResidArgs {
  const double* x;
  int64_t ldx;
  int64_t n;
  int k;
  const double* bp;  // device, B' row-major [4 ns][ldb], zero outside (k + 1) x k
  int ns;            // steps of 4 columns over the k + 1 columns
  int njb;           // 16-column blocks of the k residual columns
  int ldb;           // 16 (njb | 1): rows 16 doubles apart mod 32, so the two rows a half-wave reads share no bank
  int64_t nrb;       // 16-row blocks
  uint32_t gpu;      // groups of kRsWaves row blocks per unit (block)
  uint32_t units;
  double* partial;   // [k][units]
};

__global__ __launch_bounds__(kRsBlock) void ob_vif_resid_kernel(const ResidArgs a) {
  extern __shared__ __attribute__((aligned(16))) double bs[];  // [4 ns][ldb], then red[kRsWaves][kRsRedCols]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, li = lane & 15;
  const int nb = 4 * a.ns * a.ldb;
  double* red = bs + nb;
  for (int i = tid; i < nb; i += kRsBlock) bs[i] = a.bp[i];
  __syncthreads();
  double ss[kRsMaxJb];
#pragma unroll
  for (int jb = 0; jb < kRsMaxJb; ++jb) ss[jb] = 0.0;
  const int64_t g0 = (int64_t)blockIdx.x * a.gpu;
  for (uint32_t g = 0; g < a.gpu; ++g) {
    const int64_t rb = (g0 + g) * kRsWaves + wave;
    if (rb >= a.nrb) break;  // whole waves only: no block barrier inside the loop
    const int64_t row = rb * 16 + li;
    const bool live = row < a.n;
    ob_d4 acc[kRsMaxJb];
#pragma unroll
    for (int jb = 0; jb < kRsMaxJb; ++jb) acc[jb] = (ob_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < a.ns; ++s) {
      const int c = 4 * s + kq;
      double av = 0.0;
      if (live) av = c < a.k ? a.x[(size_t)c * a.ldx + row] : (c == a.k ? 1.0 : 0.0);
      const double* brow = bs + c * a.ldb + li;
#pragma unroll
      for (int jb = 0; jb < kRsMaxJb; ++jb)
        if (jb < a.njb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[16 * jb], acc[jb], 0, 0, 0);
    }
#pragma unroll
    for (int jb = 0; jb < kRsMaxJb; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) ss[jb] = fma(acc[jb][r], acc[jb][r], ss[jb]);
  }
  // lane (kq, li) holds rows = kq (mod 4) of column 16 jb + li: add the four row classes, then the waves in order
#pragma unroll
  for (int jb = 0; jb < kRsMaxJb; ++jb) {
    double v = ss[jb];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (kq == 0) red[wave * kRsRedCols + 16 * jb + li] = v;
  }
  __syncthreads();
  if (tid < a.k) {
    double s = red[tid];
    for (int w = 1; w < kRsWaves; ++w) s += red[w * kRsRedCols + tid];
    a.partial[(size_t)tid * a.units + blockIdx.x] = s;
  }
}

// blockIdx.x: chunk of the rows, blockIdx.y: column. partial: [k][units].
__global__ __launch_bounds__(kTtBlock) void ob_vif_sstot_kernel(const double* x, int64_t ldx, int64_t n,
                                                                 const double* means, int64_t chunk, uint32_t units,
                                                                 double* partial) {
  __shared__ double red[kTtBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.y;
  const double m = means[j];
  const double* col = x + (size_t)j * ldx;
  const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  double s = 0.0;
  for (int64_t i = i0 + tid; i < i1; i += kTtBlock) {
    const double d = col[i] - m;
    s = fma(d, d, s);
  }
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < kTtBlock / 64; ++w) t += red[w];
    partial[(size_t)j * units + blockIdx.x] = t;
  }
}

}  // namespace

namespace ob {

int vif_gram_device(ob_ctx* ctx, const double* dx, int64_t ldx, int64_t n, int k, double* gram, double* ms_out) {
  if (ms_out) *ms_out = 0.0;
  if (!ctx || !dx || !gram) return fail(OB_E_INVALID, "null pointer");
  OB_TRY(vif_check_shape(n, k));
  if (ldx < n) return fail(OB_E_INVALID, "bad VIF dimensions");
  const int k1 = k + 1, ne = k1 * (k1 + 1) / 2;
  GramArgs a = {};
  a.x = dx;
  a.ldx = ldx;
  a.n = n;
  a.k = k;
  a.ncb = (k1 + 15) / 16;
  a.nsub = (uint32_t)((n + 63) / 64);
  a.spu = (a.nsub + kGrMaxUnits - 1) / kGrMaxUnits;
  a.units = (a.nsub + a.spu - 1) / a.spu;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dpart, dsum;
  OB_HIP(dpart.alloc(sizeof(double) * (size_t)ne * a.units));
  OB_HIP(dsum.alloc(sizeof(double) * ne));
  a.partial = dpart.d();
  Events<2> ev;
  OB_HIP(ev.create());
  const size_t lds = sizeof(double) * 16 * a.ncb * kGrStride;
  OB_HIP(hipFuncSetAttribute((const void*)ob_vif_gram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(ob_vif_gram_kernel, dim3(a.units), dim3(kGrBlock), lds, st, a);
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(ne), dim3(kSumBlock), 0, st, dpart.d(), a.units, dsum.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], st));
  std::vector<double> sums(ne);
  OB_HIP(hipMemcpyAsync(sums.data(), dsum.p, sizeof(double) * ne, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  if (ms_out) {
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    *ms_out = ms;
  }
  for (int c = 0; c < k1; ++c)
    for (int b = c; b < k1; ++b) {
      const double v = sums[c * k1 - c * (c - 1) / 2 + (b - c)];
      gram[c + (size_t)b * k1] = v;
      gram[b + (size_t)c * k1] = v;
    }
  return OB_OK;
}

int vif_sums_device(ob_ctx* ctx, const double* dx, int64_t ldx, int64_t n, int k, const double* coef,
                    const double* means, double* ss_res, double* ss_tot, double* ms_out) {
  if (ms_out) *ms_out = 0.0;
  if (!ctx || !dx || !coef || !means || !ss_res || !ss_tot) return fail(OB_E_INVALID, "null pointer");
  OB_TRY(vif_check_shape(n, k));
  if (ldx < n) return fail(OB_E_INVALID, "bad VIF dimensions");
  const int k1 = k + 1;
  ResidArgs a = {};
  a.x = dx;
  a.ldx = ldx;
  a.n = n;
  a.k = k;
  a.ns = (k1 + 3) / 4;
  a.njb = (k + 15) / 16;
  a.ldb = 16 * (a.njb | 1);
  a.nrb = (n + 15) / 16;
  const int64_t ngroups = (a.nrb + kRsWaves - 1) / kRsWaves;
  a.gpu = (uint32_t)((ngroups + kRsMaxUnits - 1) / kRsMaxUnits);
  a.units = (uint32_t)((ngroups + a.gpu - 1) / a.gpu);
  // B' = [I; 0] - B: the residual x_ij - xe_i . B_j as one product (B's diagonal is the fit's own zero)
  const size_t nb = (size_t)4 * a.ns * a.ldb;
  std::vector<double> bp(nb, 0.0);
  for (int j = 0; j < k; ++j)
    for (int c = 0; c < k1; ++c) bp[(size_t)c * a.ldb + j] = (c == j ? 1.0 : 0.0) - coef[c + (size_t)j * k1];
  const uint32_t tu0 = (uint32_t)std::min<int64_t>((n + kTtBlock - 1) / kTtBlock, kTtMaxUnits);
  const int64_t chunk = (n + tu0 - 1) / tu0;
  const uint32_t tunits = (uint32_t)((n + chunk - 1) / chunk);
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dbp, dmean, dpr, dpt, dsum;
  OB_HIP(dbp.alloc(sizeof(double) * nb));
  OB_HIP(dmean.alloc(sizeof(double) * k));
  OB_HIP(dpr.alloc(sizeof(double) * (size_t)k * a.units));
  OB_HIP(dpt.alloc(sizeof(double) * (size_t)k * tunits));
  OB_HIP(dsum.alloc(sizeof(double) * 2 * k));
  a.bp = dbp.d();
  a.partial = dpr.d();
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipMemcpyAsync(dbp.p, bp.data(), sizeof(double) * nb, hipMemcpyHostToDevice, st));
  OB_HIP(hipMemcpyAsync(dmean.p, means, sizeof(double) * k, hipMemcpyHostToDevice, st));
  const size_t lds = sizeof(double) * (nb + (size_t)kRsWaves * kRsRedCols);
  OB_HIP(hipFuncSetAttribute((const void*)ob_vif_resid_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(ob_vif_resid_kernel, dim3(a.units), dim3(kRsBlock), lds, st, a);
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_vif_sstot_kernel, dim3(tunits, k), dim3(kTtBlock), 0, st, dx, ldx, n, dmean.d(), chunk, tunits,
                     dpt.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(k), dim3(kSumBlock), 0, st, dpr.d(), a.units, dsum.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(k), dim3(kSumBlock), 0, st, dpt.d(), tunits, dsum.d() + k);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], st));
  std::vector<double> sums(2 * (size_t)k);
  OB_HIP(hipMemcpyAsync(sums.data(), dsum.p, sizeof(double) * 2 * k, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  if (ms_out) {
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    *ms_out = ms;
  }
  std::copy(sums.begin(), sums.begin() + k, ss_res);
  std::copy(sums.begin() + k, sums.end(), ss_tot);
  return OB_OK;
}

}  // namespace ob
