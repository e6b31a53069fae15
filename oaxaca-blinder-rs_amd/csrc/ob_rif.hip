// ob_rif.hip -- the device pass of the RIF statistics: variance, Gini, quantile ranges.
//
// One group's outcome y[n] is sorted once (rocPRIM's stable merge sort of (y, row); its radix sort reads an
// environment variable, which the shipped library must not); everything below runs over the sorted values in
// blocks of kRifScanBlock = 1024 (256 threads x 4 consecutive values), a function of n alone:
//   rif_scan_local_kernel    inclusive scan inside a block (thread-serial, 64-lane Hillis-Steele, the four waves
//                            in order) and the block's total
//   ob_ordered_sum_kernel    the block totals added in a fixed order: sum y
//   rif_scan_totals_kernel   one block scans the block totals in block order: the carries
//   rif_rank_kernel          adds the carries; marks the end of every tie run (y[i + 1] != y[i]) and gives each
//                            row r(i) = #{y_j <= y_i}, the position after its run's last element
//   rif_pieces_kernel        per block sum (y - mu)^2 and sum GL_i, GL_i = scan[r(i) - 1] / n, in a fixed order;
//                            ob_ordered_sum_kernel adds the blocks
//   rif_quantile_kernel      OB_RIF_IQR: the two type-7 quantiles, the quartiles and the Silverman bandwidth
//   rif_kde_kernel / _finish the two Gaussian densities: a sibling of ob_kde_kernel (ob_dfl.hip) whose grid and
//                            bandwidth are read from device memory; chunk sums added in chunk order
//   rif_scatter_kernel       the RIF of every sorted position written to its row, and the statistic
// No floating-point atomics; the order of every sum depends on n alone, and since it runs over the sorted values
// the result does not depend on the row order of y either.
//
// The weighted pass (ob_rif_stat_weighted) stands beside it: its own kernels wrif_* below in the
// same block structure, sharing only the sort, rif_iota_kernel, wave_scan, rif_scan_totals_kernel and
// rif_kde_finish_kernel, none of which it changes. The unweighted kernels and their launch sequence are as they
// were, so the bytes of ob_rif_stat are too.
//   wrif_gather_kernel       ws[i] = w[row[i]] and the block's total; ob_ordered_sum_kernel adds them: W
//   wrif_scan_local_kernel   wt = ws n / W; the inclusive scans of wt and wt y inside a block, and their totals
//   wrif_rank_kernel         adds both carries; r(i) as rif_rank_kernel's, so S_i = scan_w[r(i) - 1]
//   wrif_pieces_kernel       per block sum wt (y - mu)^2 and sum wt GL
//   wrif_search_kernel       Y(t): the first sorted position whose run-end S >= t, for the quantiles' and the
//                            quartiles' t; then the quantiles and the bandwidth (one block)
//   wrif_kde_kernel          the two densities with wt on every term
//   wrif_scatter_kernel      the RIF of every sorted position written to its row, and the statistic
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include <rocprim/device/device_merge_sort.hpp>

#include "ob_device.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_rif.hpp"

namespace {

using namespace ob;

constexpr int kT = kRifThreads, kI = kRifItems, kB = kRifScanBlock;
constexpr int kWaves = kT / 64;
constexpr uint32_t kKdeMaxChunks = 1024;

// dq: what the quantile pieces leave for the later kernels
enum { kQHi = 0, kQLo = 1, kBw = 2, kDensHi = 3, kDensLo = 4, kDq = 8 };

// Inclusive scan over the wave's 64 lanes; the additions of a lane depend on its index alone.
__device__ __forceinline__ double wave_scan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

__global__ __launch_bounds__(kT) void rif_iota_kernel(uint32_t n, uint32_t* idx) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i < n) idx[i] = i;
}

__global__ __launch_bounds__(kT) void rif_scan_local_kernel(const double* ys, uint32_t n, double* scan, double* btot) {
  __shared__ double wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t base = blockIdx.x * (uint32_t)kB + (uint32_t)tid * kI;
  double v[kI], run = 0.0;
#pragma unroll
  for (int j = 0; j < kI; ++j) {
    run += base + j < n ? ys[base + j] : 0.0;
    v[j] = run;
  }
  const double inc = wave_scan(run, lane);
  double before = __shfl_up(inc, 1);
  if (lane == 0) before = 0.0;
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  double pre = 0.0;
  for (int w = 0; w < wave; ++w) pre += wtot[w];
  const double off = pre + before;
#pragma unroll
  for (int j = 0; j < kI; ++j)
    if (base + j < n) scan[base + j] = off + v[j];
  if (tid == kT - 1) btot[blockIdx.x] = pre + inc;
}

// One block: carry[b] = btot[0] + .. + btot[b - 1], 256 blocks a round, the rounds in order.
__global__ __launch_bounds__(kT) void rif_scan_totals_kernel(const double* btot, uint32_t nb, double* carry) {
  __shared__ double wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double running = 0.0;  // the same value in every thread
  for (uint32_t b0 = 0; b0 < nb; b0 += kT) {
    const uint32_t b = b0 + tid;
    const double inc = wave_scan(b < nb ? btot[b] : 0.0, lane);
    double before = __shfl_up(inc, 1);
    if (lane == 0) before = 0.0;
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    double pre = 0.0;
    for (int w = 0; w < wave; ++w) pre += wtot[w];
    if (b < nb) carry[b] = running + (pre + before);
    double total = wtot[0];
    for (int w = 1; w < kWaves; ++w) total += wtot[w];
    running += total;
    __syncthreads();  // wtot is rewritten in the next round
  }
}

__global__ __launch_bounds__(kT) void rif_rank_kernel(const double* ys, uint32_t n, const double* carry, double* scan,
                                                       uint32_t* rank) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  scan[i] += carry[i / kB];
  const double y = ys[i];
  uint32_t r = i + 1;
  if (i + 1 < n && ys[i + 1] == y) {  // not a run end: the first position above i + 1 whose value exceeds y
    uint32_t lo = i + 2, hi = n;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (ys[mid] <= y) lo = mid + 1;
      else hi = mid;
    }
    r = lo;
  }
  rank[i] = r;
}

// The block's two sums: thread-serial over its 4 values, the 64-lane butterfly, the four waves in order.
__global__ __launch_bounds__(kT) void rif_pieces_kernel(const double* ys, uint32_t n, const double* scan,
                                                         const uint32_t* rank, const double* sums, uint32_t nb,
                                                         double* part) {
  __shared__ double red[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t base = blockIdx.x * (uint32_t)kB + (uint32_t)tid * kI;
  const double nf = (double)n, mu = sums[0] / nf;
  double s2 = 0.0, sg = 0.0;
#pragma unroll
  for (int j = 0; j < kI; ++j) {
    const uint32_t i = base + j;
    if (i < n) {
      const double d = ys[i] - mu;
      s2 += d * d;
      sg += scan[rank[i] - 1] / nf;
    }
  }
  s2 = wave_sum(s2);
  sg = wave_sum(sg);
  if (lane == 0) {
    red[0][wave] = s2;
    red[1][wave] = sg;
  }
  __syncthreads();
  if (tid < 2) {
    double s = red[tid][0];
    for (int w = 1; w < kWaves; ++w) s += red[tid][w];
    part[(size_t)tid * nb + blockIdx.x] = s;
  }
}

// math/rif.rs:14-88 up to the bandwidth, from the sorted values and the ordered sums. One thread.
__device__ double rif_type7(const double* ys, double nf, double tau) {
  const double h = (nf - 1.0) * tau, hf = floor(h), hc = ceil(h), frac = h - hf;
  const double lo = ys[(uint32_t)hf];
  return hf == hc ? lo : lo + frac * (ys[(uint32_t)hc] - lo);
}

__global__ void rif_quantile_kernel(const double* ys, uint32_t n, const double* sums, double tau_hi, double tau_lo,
                                    double* dq) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double nf = (double)n;
  const double sd = sqrt(sums[1] / (nf - 1.0));
  int64_t i75 = (int64_t)ceil(0.75 * nf), i25 = (int64_t)ceil(0.25 * nf);
  i75 = i75 == 0 ? 0 : i75 - 1;
  i25 = i25 == 0 ? 0 : i25 - 1;
  const double iqr = ys[min(i75, (int64_t)n - 1)] - ys[min(i25, (int64_t)n - 1)];
  double spread = iqr > 1e-8 ? fmin(sd, iqr / 1.34) : sd;
  if (spread < 1e-8) spread = 1.0;
  dq[kQHi] = rif_type7(ys, nf, tau_hi);
  dq[kQLo] = rif_type7(ys, nf, tau_lo);
  dq[kBw] = 0.9 * spread * pow(nf, -0.2);
}

// blockIdx.x: chunk of the sorted values; both grid points in one block. partial: [2][nchunks].
__global__ __launch_bounds__(kT) void rif_kde_kernel(const double* ys, uint32_t n, const double* dq, uint32_t chunk,
                                                      uint32_t nchunks, double* partial) {
  __shared__ double red[kWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double q0 = dq[kQHi], q1 = dq[kQLo], bw = dq[kBw];
  const double c = 0.3989422804014327;  // 1 / sqrt(2 pi)
  const uint32_t i0 = blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  double a0 = 0.0, a1 = 0.0;
  for (uint32_t i = i0 + tid; i < i1; i += kT) {
    const double y = ys[i];
    const double u0 = (q0 - y) / bw, u1 = (q1 - y) / bw;
    a0 += c * exp(-0.5 * (u0 * u0));
    a1 += c * exp(-0.5 * (u1 * u1));
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (lane == 0) {
    red[wave][0] = a0;
    red[wave][1] = a1;
  }
  __syncthreads();
  if (tid < 2) {
    double s = red[0][tid];
    for (int w = 1; w < kWaves; ++w) s += red[w][tid];
    partial[(size_t)tid * nchunks + blockIdx.x] = s;
  }
}

__global__ void rif_kde_finish_kernel(const double* partial, uint32_t nchunks, uint32_t n, double* dq) {
  const int g = threadIdx.x;
  if (blockIdx.x != 0 || g >= 2) return;
  double s = 0.0;
  for (uint32_t c = 0; c < nchunks; ++c) s += partial[(size_t)g * nchunks + c];
  double dens = s / ((double)n * dq[kBw]);
  if (dens < 1e-8) dens = 1e-8;
  dq[kDensHi + g] = dens;
}

__global__ __launch_bounds__(kT) void rif_scatter_kernel(const double* ys, const uint32_t* row, uint32_t n,
                                                          const double* scan, const uint32_t* rank, const double* sums,
                                                          const double* dq, int stat, double tau_hi, double tau_lo,
                                                          double* out, double* statistic) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const double nf = (double)n, y = ys[i], mu = sums[0] / nf;
  double v, st;
  if (stat == OB_RIF_VARIANCE) {
    const double d = y - mu;
    v = d * d;
    st = sums[1] / nf;
  } else if (stat == OB_RIF_GINI) {
    const double r = sums[2] / nf, p = (double)rank[i] / nf, gl = scan[rank[i] - 1] / nf;
    v = 1.0 + (2.0 * r / (mu * mu)) * y - (2.0 / mu) * (y * (1.0 - p) + gl);
    st = 1.0 - 2.0 * r / mu;
  } else {
    const double qh = dq[kQHi], ql = dq[kQLo];
    const double hi = qh + (tau_hi - (y <= qh ? 1.0 : 0.0)) / dq[kDensHi];
    const double lo = ql + (tau_lo - (y <= ql ? 1.0 : 0.0)) / dq[kDensLo];
    v = hi - lo;
    st = qh - ql;
  }
  const uint32_t r = row[i];
  if (r < n) out[r] = v;
  if (i == 0) *statistic = st;
}

// ---- the weighted pass -------------------------------------------------------------------------------------
enum { kSW = 0, kSMu = 1, kSVar = 2, kSGl = 3 };  // sums: W, sum wt y, sum wt (y - mu)^2, sum wt GL

// The block's total of v in a fixed order: the 64-lane butterfly, the four waves in order. red: [kWaves].
__device__ __forceinline__ double wrif_block_sum(double v, double* red, int tid) {
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < kWaves; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(kT) void wrif_gather_kernel(const double* w, const uint32_t* row, uint32_t n, double* ws,
                                                          double* btot) {
  __shared__ double red[kWaves];
  const int tid = threadIdx.x;
  const uint32_t base = blockIdx.x * (uint32_t)kB + (uint32_t)tid * kI;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kI; ++j) {
    const uint32_t i = base + j;
    if (i < n) {
      const uint32_t r = row[i];
      const double v = r < n ? w[r] : 0.0;
      ws[i] = v;
      s += v;
    }
  }
  s = wrif_block_sum(s, red, tid);
  if (tid == 0) btot[blockIdx.x] = s;
}

// rif_scan_local_kernel over two series at once: wt and wt y. btot: [2][nb].
__global__ __launch_bounds__(kT) void wrif_scan_local_kernel(const double* ys, const double* ws, uint32_t n,
                                                              const double* sums, uint32_t nb, double* wt, double* scanw,
                                                              double* scany, double* btot) {
  __shared__ double wtot[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t base = blockIdx.x * (uint32_t)kB + (uint32_t)tid * kI;
  const double nf = (double)n, W = sums[kSW];
  double vw[kI], vy[kI], runw = 0.0, runy = 0.0;
#pragma unroll
  for (int j = 0; j < kI; ++j) {
    double t = 0.0, ty = 0.0;
    if (base + j < n) {
      t = ws[base + j] * nf / W;
      ty = t * ys[base + j];
      wt[base + j] = t;
    }
    runw += t;
    runy += ty;
    vw[j] = runw;
    vy[j] = runy;
  }
  const double incw = wave_scan(runw, lane), incy = wave_scan(runy, lane);
  double beforew = __shfl_up(incw, 1), beforey = __shfl_up(incy, 1);
  if (lane == 0) beforew = beforey = 0.0;
  if (lane == 63) {
    wtot[0][wave] = incw;
    wtot[1][wave] = incy;
  }
  __syncthreads();
  double prew = 0.0, prey = 0.0;
  for (int w = 0; w < wave; ++w) {
    prew += wtot[0][w];
    prey += wtot[1][w];
  }
  const double offw = prew + beforew, offy = prey + beforey;
#pragma unroll
  for (int j = 0; j < kI; ++j)
    if (base + j < n) {
      scanw[base + j] = offw + vw[j];
      scany[base + j] = offy + vy[j];
    }
  if (tid == kT - 1) {
    btot[blockIdx.x] = prew + incw;
    btot[(size_t)nb + blockIdx.x] = prey + incy;
  }
}

// carry: [2][nb]
__global__ __launch_bounds__(kT) void wrif_rank_kernel(const double* ys, uint32_t n, const double* carry, uint32_t nb,
                                                        double* scanw, double* scany, uint32_t* rank) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  scanw[i] += carry[i / kB];
  scany[i] += carry[(size_t)nb + i / kB];
  const double y = ys[i];
  uint32_t r = i + 1;
  if (i + 1 < n && ys[i + 1] == y) {
    uint32_t lo = i + 2, hi = n;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (ys[mid] <= y) lo = mid + 1;
      else hi = mid;
    }
    r = lo;
  }
  rank[i] = r;
}

// part: [2][nb]
__global__ __launch_bounds__(kT) void wrif_pieces_kernel(const double* ys, const double* wt, uint32_t n,
                                                          const double* scany, const uint32_t* rank, const double* sums,
                                                          uint32_t nb, double* part) {
  __shared__ double red[2][kWaves];
  const int tid = threadIdx.x;
  const uint32_t base = blockIdx.x * (uint32_t)kB + (uint32_t)tid * kI;
  const double nf = (double)n, mu = sums[kSMu] / nf;
  double s2 = 0.0, sg = 0.0;
#pragma unroll
  for (int j = 0; j < kI; ++j) {
    const uint32_t i = base + j;
    if (i < n) {
      const double d = ys[i] - mu, t = wt[i];
      s2 += t * (d * d);
      sg += t * (scany[rank[i] - 1] / nf);
    }
  }
  s2 = wrif_block_sum(s2, red[0], tid);
  sg = wrif_block_sum(sg, red[1], tid);
  if (tid == 0) {
    part[blockIdx.x] = s2;
    part[(size_t)nb + blockIdx.x] = sg;
  }
}

// Y(t): the sorted value at the first position whose run-end S >= t; the last value when no position has one.
__device__ double wrif_y_at(const double* ys, const double* scanw, const uint32_t* rank, uint32_t n, double t) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (scanw[rank[mid] - 1] >= t) hi = mid;
    else lo = mid + 1;
  }
  return ys[min(lo, n - 1)];
}

// One block: threads 0 .. 5 search Y for the two quantiles' t and the quartiles'; thread 0 forms the quantiles and
// the bandwidth as rif_quantile_kernel does. tau_lo <= 0: one quantile only (OB_RIF_QUANTILE).
__global__ __launch_bounds__(64) void wrif_search_kernel(const double* ys, const double* scanw, const uint32_t* rank,
                                                          uint32_t n, const double* sums, double tau_hi, double tau_lo,
                                                          double* dq) {
  __shared__ double yv[6], fr[2];
  const int tid = threadIdx.x;
  const double nf = (double)n;
  if (blockIdx.x != 0) return;
  if (tid < 6) {
    double t;
    if (tid < 4) {
      const double tau = tid < 2 ? tau_hi : tau_lo;
      const double h = (nf - 1.0) * tau, lo = floor(h);
      t = (tid & 1) ? fmin(lo + 2.0, nf) : lo + 1.0;
      if (!(tid & 1)) fr[tid >> 1] = h - lo;
    } else {
      t = fmin(fmax(ceil((tid == 4 ? 0.75 : 0.25) * nf), 1.0), nf);
    }
    yv[tid] = (tid >= 2 && tid < 4 && !(tau_lo > 0.0)) ? 0.0 : wrif_y_at(ys, scanw, rank, n, t);
  }
  __syncthreads();
  if (tid != 0) return;
  const double sd = sqrt(sums[kSVar] / (nf - 1.0));
  const double iqr = yv[4] - yv[5];
  double spread = iqr > 1e-8 ? fmin(sd, iqr / 1.34) : sd;
  if (spread < 1e-8) spread = 1.0;
  dq[kQHi] = fr[0] == 0.0 ? yv[0] : yv[0] + fr[0] * (yv[1] - yv[0]);
  dq[kQLo] = !(tau_lo > 0.0) ? 0.0 : (fr[1] == 0.0 ? yv[2] : yv[2] + fr[1] * (yv[3] - yv[2]));
  dq[kBw] = 0.9 * spread * pow(nf, -0.2);
}

// rif_kde_kernel with wt on every term.
__global__ __launch_bounds__(kT) void wrif_kde_kernel(const double* ys, const double* wt, uint32_t n, const double* dq,
                                                       uint32_t chunk, uint32_t nchunks, double* partial) {
  __shared__ double red[kWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double q0 = dq[kQHi], q1 = dq[kQLo], bw = dq[kBw];
  const double c = 0.3989422804014327;  // 1 / sqrt(2 pi)
  const uint32_t i0 = blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  double a0 = 0.0, a1 = 0.0;
  for (uint32_t i = i0 + tid; i < i1; i += kT) {
    const double y = ys[i], t = wt[i];
    const double u0 = (q0 - y) / bw, u1 = (q1 - y) / bw;
    a0 += t * (c * exp(-0.5 * (u0 * u0)));
    a1 += t * (c * exp(-0.5 * (u1 * u1)));
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (lane == 0) {
    red[wave][0] = a0;
    red[wave][1] = a1;
  }
  __syncthreads();
  if (tid < 2) {
    double s = red[0][tid];
    for (int w = 1; w < kWaves; ++w) s += red[w][tid];
    partial[(size_t)tid * nchunks + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kT) void wrif_scatter_kernel(const double* ys, const uint32_t* row, uint32_t n,
                                                           const double* scanw, const double* scany, const uint32_t* rank,
                                                           const double* sums, const double* dq, int stat, double tau_hi,
                                                           double tau_lo, double* out, double* statistic) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const double nf = (double)n, y = ys[i], mu = sums[kSMu] / nf;
  double v, st;
  if (stat == OB_RIF_VARIANCE) {
    const double d = y - mu;
    v = d * d;
    st = sums[kSVar] / nf;
  } else if (stat == OB_RIF_GINI) {
    const double r = sums[kSGl] / nf, f = scanw[rank[i] - 1] / nf, gl = scany[rank[i] - 1] / nf;
    v = 1.0 + (2.0 * r / (mu * mu)) * y - (2.0 / mu) * (y * (1.0 - f) + gl);
    st = 1.0 - 2.0 * r / mu;
  } else {
    const double qh = dq[kQHi];
    const double hi = qh + (tau_hi - (y <= qh ? 1.0 : 0.0)) / dq[kDensHi];
    if (stat == OB_RIF_QUANTILE) {
      v = hi;
      st = qh;
    } else {
      const double ql = dq[kQLo];
      const double lo = ql + (tau_lo - (y <= ql ? 1.0 : 0.0)) / dq[kDensLo];
      v = hi - lo;
      st = qh - ql;
    }
  }
  const uint32_t r = row[i];
  if (r < n) out[r] = v;
  if (i == 0) *statistic = st;
}

thread_local ob_rif_timing g_timing = {};

}  // namespace

namespace ob {

int rif_device(ob_ctx* ctx, const double* y, int64_t n64, const ob_rif_spec* specs, int n_specs, double* rif,
               double* stats, bool reset) {
  if (reset) g_timing = ob_rif_timing{};
  if (!ctx || !y || !specs || !rif || !stats) return fail(OB_E_INVALID, "null pointer");
  if (n64 < 2 || n64 > kRifMaxRows || n_specs < 1) return fail(OB_E_INVALID, "bad RIF dimensions");
  const uint32_t n = (uint32_t)n64;
  const uint32_t nb = (n + kB - 1) / kB;       // scan blocks = sum pieces
  const unsigned grid = blocks_for((int64_t)n);  // one thread per value
  const uint32_t nchunks0 = std::min<uint32_t>((n + kT - 1) / kT, kKdeMaxChunks);
  const uint32_t chunk = (n + nchunks0 - 1) / nchunks0;
  const uint32_t nchunks = (n + chunk - 1) / chunk;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dy, dys, drow0, drow, dscan, drank, dout, dbtot, dcarry, dpart, dsums, ddq, dkde, dstat, dtmp;
  const size_t nd = sizeof(double) * (size_t)n, nu = sizeof(uint32_t) * (size_t)n;
  OB_HIP(dy.alloc(nd));
  OB_HIP(dys.alloc(nd));
  OB_HIP(drow0.alloc(nu));
  OB_HIP(drow.alloc(nu));
  OB_HIP(dscan.alloc(nd));
  OB_HIP(drank.alloc(nu));
  OB_HIP(dout.alloc(nd));
  OB_HIP(dbtot.alloc(sizeof(double) * nb));
  OB_HIP(dcarry.alloc(sizeof(double) * nb));
  OB_HIP(dpart.alloc(sizeof(double) * 2 * nb));
  OB_HIP(dsums.alloc(sizeof(double) * 4));
  OB_HIP(ddq.alloc(sizeof(double) * kDq));
  OB_HIP(dkde.alloc(sizeof(double) * 2 * nchunks));
  OB_HIP(dstat.alloc(sizeof(double)));
  size_t tmp_bytes = 0;
  OB_HIP(rocprim::merge_sort(nullptr, tmp_bytes, dy.d(), dys.d(), drow0.as<uint32_t>(), drow.as<uint32_t>(),
                                   (size_t)n, rocprim::less<double>(), st));
  OB_HIP(dtmp.alloc(tmp_bytes));
  Events<6> ev;
  OB_HIP(ev.create());
  OB_HIP(hipMemcpyAsync(dy.p, y, nd, hipMemcpyHostToDevice, st));
  OB_HIP(hipMemsetAsync(ddq.p, 0, sizeof(double) * kDq, st));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(rif_iota_kernel, dim3(grid), dim3(kT), 0, st, n, drow0.as<uint32_t>());
  OB_HIP(hipGetLastError());
  OB_HIP(rocprim::merge_sort(dtmp.p, tmp_bytes, dy.d(), dys.d(), drow0.as<uint32_t>(), drow.as<uint32_t>(),
                                   (size_t)n, rocprim::less<double>(), st));
  OB_HIP(hipEventRecord(ev.e[1], st));
  hipLaunchKernelGGL(rif_scan_local_kernel, dim3(nb), dim3(kT), 0, st, dys.d(), n, dscan.d(), dbtot.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(1), dim3(kSumBlock), 0, st, dbtot.d(), nb, dsums.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rif_scan_totals_kernel, dim3(1), dim3(kT), 0, st, dbtot.d(), nb, dcarry.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rif_rank_kernel, dim3(grid), dim3(kT), 0, st, dys.d(), n, dcarry.d(), dscan.d(),
                     drank.as<uint32_t>());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(rif_pieces_kernel, dim3(nb), dim3(kT), 0, st, dys.d(), n, dscan.d(), drank.as<uint32_t>(),
                     dsums.d(), nb, dpart.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(2), dim3(kSumBlock), 0, st, dpart.d(), nb, dsums.d() + 1);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[2], st));
  OB_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  g_timing.sort_ms += ms;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
  g_timing.scan_ms += ms;
  for (int s = 0; s < n_specs; ++s) {
    const ob_rif_spec& sp = specs[s];
    OB_HIP(hipEventRecord(ev.e[3], st));
    if (sp.stat == OB_RIF_IQR) {
      hipLaunchKernelGGL(rif_quantile_kernel, dim3(1), dim3(64), 0, st, dys.d(), n, dsums.d(), sp.p0, sp.p1, ddq.d());
      OB_HIP(hipGetLastError());
      hipLaunchKernelGGL(rif_kde_kernel, dim3(nchunks), dim3(kT), 0, st, dys.d(), n, ddq.d(), chunk, nchunks, dkde.d());
      OB_HIP(hipGetLastError());
      hipLaunchKernelGGL(rif_kde_finish_kernel, dim3(1), dim3(64), 0, st, dkde.d(), nchunks, n, ddq.d());
      OB_HIP(hipGetLastError());
    }
    OB_HIP(hipEventRecord(ev.e[4], st));
    hipLaunchKernelGGL(rif_scatter_kernel, dim3(grid), dim3(kT), 0, st, dys.d(), drow.as<uint32_t>(), n, dscan.d(),
                       drank.as<uint32_t>(), dsums.d(), ddq.d(), (int)sp.stat, sp.p0, sp.p1, dout.d(), dstat.d());
    OB_HIP(hipGetLastError());
    OB_HIP(hipEventRecord(ev.e[5], st));
    OB_HIP(hipMemcpyAsync(rif + (size_t)s * n, dout.p, nd, hipMemcpyDeviceToHost, st));
    OB_HIP(hipMemcpyAsync(stats + s, dstat.p, sizeof(double), hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    OB_HIP(hipEventElapsedTime(&ms, ev.e[3], ev.e[4]));
    g_timing.kde_ms += ms;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[4], ev.e[5]));
    g_timing.scatter_ms += ms;
  }
  return OB_OK;
}

// The weighted sibling of rif_device: y and w on the host, every statistic of the call from one sort.
int rif_device_weighted(ob_ctx* ctx, const double* y, const double* w, int64_t n64, const ob_rif_spec* specs,
                        int n_specs, double* rif, double* stats, bool reset) {
  if (reset) g_timing = ob_rif_timing{};
  if (!ctx || !y || !w || !specs || !rif || !stats) return fail(OB_E_INVALID, "null pointer");
  if (n64 < 2 || n64 > kRifMaxRows || n_specs < 1) return fail(OB_E_INVALID, "bad RIF dimensions");
  const uint32_t n = (uint32_t)n64;
  const uint32_t nb = (n + kB - 1) / kB;
  const unsigned grid = blocks_for((int64_t)n);
  const uint32_t nchunks0 = std::min<uint32_t>((n + kT - 1) / kT, kKdeMaxChunks);
  const uint32_t chunk = (n + nchunks0 - 1) / nchunks0;
  const uint32_t nchunks = (n + chunk - 1) / chunk;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dy, dys, dw, dws, dwt, drow0, drow, dscanw, dscany, drank, dout, dbtot, dcarry, dpart, dsums, ddq, dkde, dstat,
      dtmp;
  const size_t nd = sizeof(double) * (size_t)n, nu = sizeof(uint32_t) * (size_t)n;
  OB_HIP(dy.alloc(nd));
  OB_HIP(dys.alloc(nd));
  OB_HIP(dw.alloc(nd));
  OB_HIP(dws.alloc(nd));
  OB_HIP(dwt.alloc(nd));
  OB_HIP(drow0.alloc(nu));
  OB_HIP(drow.alloc(nu));
  OB_HIP(dscanw.alloc(nd));
  OB_HIP(dscany.alloc(nd));
  OB_HIP(drank.alloc(nu));
  OB_HIP(dout.alloc(nd));
  OB_HIP(dbtot.alloc(sizeof(double) * 2 * nb));
  OB_HIP(dcarry.alloc(sizeof(double) * 2 * nb));
  OB_HIP(dpart.alloc(sizeof(double) * 2 * nb));
  OB_HIP(dsums.alloc(sizeof(double) * 4));
  OB_HIP(ddq.alloc(sizeof(double) * kDq));
  OB_HIP(dkde.alloc(sizeof(double) * 2 * nchunks));
  OB_HIP(dstat.alloc(sizeof(double)));
  size_t tmp_bytes = 0;
  OB_HIP(rocprim::merge_sort(nullptr, tmp_bytes, dy.d(), dys.d(), drow0.as<uint32_t>(), drow.as<uint32_t>(),
                                   (size_t)n, rocprim::less<double>(), st));
  OB_HIP(dtmp.alloc(tmp_bytes));
  Events<6> ev;
  OB_HIP(ev.create());
  OB_HIP(hipMemcpyAsync(dy.p, y, nd, hipMemcpyHostToDevice, st));
  OB_HIP(hipMemcpyAsync(dw.p, w, nd, hipMemcpyHostToDevice, st));
  OB_HIP(hipMemsetAsync(ddq.p, 0, sizeof(double) * kDq, st));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(rif_iota_kernel, dim3(grid), dim3(kT), 0, st, n, drow0.as<uint32_t>());
  OB_HIP(hipGetLastError());
  OB_HIP(rocprim::merge_sort(dtmp.p, tmp_bytes, dy.d(), dys.d(), drow0.as<uint32_t>(), drow.as<uint32_t>(),
                                   (size_t)n, rocprim::less<double>(), st));
  OB_HIP(hipEventRecord(ev.e[1], st));
  hipLaunchKernelGGL(wrif_gather_kernel, dim3(nb), dim3(kT), 0, st, dw.d(), drow.as<uint32_t>(), n, dws.d(), dbtot.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(1), dim3(kSumBlock), 0, st, dbtot.d(), nb, dsums.d() + kSW);
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(wrif_scan_local_kernel, dim3(nb), dim3(kT), 0, st, dys.d(), dws.d(), n, dsums.d(), nb, dwt.d(),
                     dscanw.d(), dscany.d(), dbtot.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(1), dim3(kSumBlock), 0, st, dbtot.d() + nb, nb, dsums.d() + kSMu);
  OB_HIP(hipGetLastError());
  for (int e = 0; e < 2; ++e) {
    hipLaunchKernelGGL(rif_scan_totals_kernel, dim3(1), dim3(kT), 0, st, dbtot.d() + (size_t)e * nb, nb,
                       dcarry.d() + (size_t)e * nb);
    OB_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(wrif_rank_kernel, dim3(grid), dim3(kT), 0, st, dys.d(), n, dcarry.d(), nb, dscanw.d(), dscany.d(),
                     drank.as<uint32_t>());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(wrif_pieces_kernel, dim3(nb), dim3(kT), 0, st, dys.d(), dwt.d(), n, dscany.d(), drank.as<uint32_t>(),
                     dsums.d(), nb, dpart.d());
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(2), dim3(kSumBlock), 0, st, dpart.d(), nb, dsums.d() + kSVar);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[2], st));
  OB_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  g_timing.sort_ms += ms;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
  g_timing.scan_ms += ms;
  for (int s = 0; s < n_specs; ++s) {
    const ob_rif_spec& sp = specs[s];
    const double tau_lo = sp.stat == OB_RIF_IQR ? sp.p1 : 0.0;
    OB_HIP(hipEventRecord(ev.e[3], st));
    if (sp.stat == OB_RIF_IQR || sp.stat == OB_RIF_QUANTILE) {
      hipLaunchKernelGGL(wrif_search_kernel, dim3(1), dim3(64), 0, st, dys.d(), dscanw.d(), drank.as<uint32_t>(), n,
                         dsums.d(), sp.p0, tau_lo, ddq.d());
      OB_HIP(hipGetLastError());
      hipLaunchKernelGGL(wrif_kde_kernel, dim3(nchunks), dim3(kT), 0, st, dys.d(), dwt.d(), n, ddq.d(), chunk, nchunks,
                         dkde.d());
      OB_HIP(hipGetLastError());
      hipLaunchKernelGGL(rif_kde_finish_kernel, dim3(1), dim3(64), 0, st, dkde.d(), nchunks, n, ddq.d());
      OB_HIP(hipGetLastError());
    }
    OB_HIP(hipEventRecord(ev.e[4], st));
    hipLaunchKernelGGL(wrif_scatter_kernel, dim3(grid), dim3(kT), 0, st, dys.d(), drow.as<uint32_t>(), n, dscanw.d(),
                       dscany.d(), drank.as<uint32_t>(), dsums.d(), ddq.d(), (int)sp.stat, sp.p0, tau_lo, dout.d(),
                       dstat.d());
    OB_HIP(hipGetLastError());
    OB_HIP(hipEventRecord(ev.e[5], st));
    OB_HIP(hipMemcpyAsync(rif + (size_t)s * n, dout.p, nd, hipMemcpyDeviceToHost, st));
    OB_HIP(hipMemcpyAsync(stats + s, dstat.p, sizeof(double), hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    OB_HIP(hipEventElapsedTime(&ms, ev.e[3], ev.e[4]));
    g_timing.kde_ms += ms;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[4], ev.e[5]));
    g_timing.scatter_ms += ms;
  }
  return OB_OK;
}

// installs the builder's hook when the library loads (ob_rif.hpp)
static const bool g_rif_hook_installed = [] {
  rif_hooks().device = rif_device;
  rif_hooks().device_weighted = rif_device_weighted;
  return true;
}();

}  // namespace ob

extern "C" {

int ob_rif_stat(ob_ctx* ctx, const double* y, int64_t n, const ob_rif_spec* spec, double* rif_out,
                double* statistic_out) {
  OB_TRY(ob::rif_input_check(y, n, spec, 1));
  if (!ctx || !rif_out || !statistic_out) return ob::fail(OB_E_INVALID, "null pointer");
  return ob::rif_device(ctx, y, n, spec, 1, rif_out, statistic_out, true);
}

int ob_rif_stat_weighted(ob_ctx* ctx, const double* y, const double* w, int64_t n, const ob_rif_spec* spec,
                         double* rif_out, double* statistic_out) {
  OB_TRY(ob::rif_input_check_weighted(y, w, n, spec, 1));
  if (!ctx || !rif_out || !statistic_out) return ob::fail(OB_E_INVALID, "null pointer");
  return ob::rif_device_weighted(ctx, y, w, n, spec, 1, rif_out, statistic_out, true);
}

int32_t ob_rif_scan_block(void) { return ob::kRifScanBlock; }

int ob_rif_last_timing(ob_rif_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

}  // extern "C"
