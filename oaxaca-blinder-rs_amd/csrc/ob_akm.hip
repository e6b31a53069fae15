// ob_akm.hip -- device kernels of the AKM worker and firm fixed-effects model (akm.rs:236-621):
//
//   akm_demean_kernel<FIRM>  one half-step of demean_vector for a batch of columns: a group's column
//                            sums, its means, and the rows of the group rewritten, in one launch
//   akm_flag_kernel          each column's ||v - prev||_2 from the firm pass's per-block partials, the
//                            stopping rule and the per-column done flag
//   akm_fe_kernel            one half-step of recover_fe: a group's mean of r_i - other[idx_i]
//   akm_fe_flag_kernel       the (alpha, psi) change norm and the stopping rule
//   akm_shift_kernel         the psi[0] normalisation
//   akm_gram_kernel          V'V of the demeaned batch, per-block partials
//   akm_rowsum_kernel        sum y, tss and rss terms, per-block partials
//   ob_ordered_sum_kernel    partials added in a fixed order (ob_device.hpp)
//   akm_resid_kernel         r = y - X beta
//
// Rows are grouped twice, by worker and by firm, as CSR lists of row positions (ascending inside a
// group). A group is summed by one lane (up to kAkmLaneMax rows), one wave (up to kAkmWaveMax) or one
// 256-thread block, chosen by its row count alone; the order of every f64 sum is a function of the
// input's sizes and group layout, and there is no floating atomic, so a call repeated on the same
// input returns the same bytes. A column's arithmetic never looks at another column, so a column
// gives the same bytes alone or in any batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ob_akm.hpp"
#include "ob_device.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_options.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 8;          // columns of the batch a thread carries at a time
constexpr int kGramRows = 64;     // rows per LDS tile of the Gram
constexpr int kGramMaxC = 65;     // outcome + OB_AKM_MAX_CONTROLS
constexpr int kGramStride = kGramRows + 1;
constexpr int kGramAcc = (kGramMaxC * kGramMaxC + kBlock - 1) / kBlock;
constexpr int kGramMaxBlocks = 512;
constexpr int kSumMaxBlocks = 1024;

// One grouping of the rows. order lists the group ids block-per-group first (largest first), then
// wave-per-group, then lane-per-group; blocks of a launch take them in that order.
struct Seg {
  const int32_t* ptr;    // n_groups + 1
  const int32_t* rows;   // n
  const int32_t* order;  // n_groups
  int32_t n_large, n_medium, n_small;
};

enum { kRoleBlock = 0, kRoleWave = 1, kRoleLane = 2 };

// The role of this block and the group of this thread (-1: none). Block-uniform role.
__device__ __forceinline__ int seg_role(const Seg& s, int* group) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int mblocks = (s.n_medium + kWaves - 1) / kWaves;
  if (b < s.n_large) {
    *group = s.order[b];
    return kRoleBlock;
  }
  if (b < s.n_large + mblocks) {
    const int slot = (b - s.n_large) * kWaves + (tid >> 6);
    *group = slot < s.n_medium ? s.order[s.n_large + slot] : -1;
    return kRoleWave;
  }
  const int64_t slot = (int64_t)(b - s.n_large - mblocks) * kBlock + tid;
  *group = slot < s.n_small ? s.order[(int64_t)s.n_large + s.n_medium + slot] : -1;
  return kRoleLane;
}

// Every thread receives the waves' sums added in wave order. red: kWaves doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s += red[w];
  return s;
}

// FIRM = false: io[row][c] = in[row][c] - mean_c(worker of row).
// FIRM = true:  new = in[row][c] - mean_c(firm of row); dpart[block][c] = sum (new - io[row][c])^2 over
//               the block's rows; io[row][c] = new. (in: the worker pass's output, io: prev, then v.)
template <bool FIRM>
__global__ __launch_bounds__(kBlock) void akm_demean_kernel(const Seg s, int ncols, const double* __restrict__ in,
                                                             double* io, const int32_t* __restrict__ done,
                                                             double* dpart) {
#pragma clang fp contract(off)
  __shared__ double red[kWaves];
  __shared__ double dred[kWaves][kTile];
  int g;
  const int role = seg_role(s, &g);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int p0 = 0, p1 = 0;
  if (g >= 0) {
    p0 = s.ptr[g];
    p1 = s.ptr[g + 1];
  }
  // this thread's rows are p0 + first, p0 + first + step, ...
  const int first = role == kRoleLane ? 0 : (role == kRoleWave ? lane : tid);
  const int step = role == kRoleLane ? 1 : (role == kRoleWave ? 64 : kBlock);
  const double cnt = (double)(p1 - p0);
  for (int c0 = 0; c0 < ncols; c0 += kTile) {
    bool act[kTile];
    bool any = false;
#pragma unroll
    for (int j = 0; j < kTile; ++j) {
      act[j] = c0 + j < ncols && done[min(c0 + j, ncols - 1)] == 0;
      any = any || act[j];
    }
    if (!any) continue;  // the same for every thread of the grid
    double acc[kTile], d2[kTile];
#pragma unroll
    for (int j = 0; j < kTile; ++j) acc[j] = d2[j] = 0.0;
#pragma unroll 2
    for (int p = p0 + first; p < p1; p += step) {
      const double* src = in + (size_t)s.rows[p] * ncols + c0;
#pragma unroll
      for (int j = 0; j < kTile; ++j)
        if (act[j]) acc[j] += src[j];
    }
    if (role == kRoleWave) {
#pragma unroll
      for (int j = 0; j < kTile; ++j) acc[j] = wave_sum(acc[j]);
    } else if (role == kRoleBlock) {
#pragma unroll
      for (int j = 0; j < kTile; ++j) acc[j] = block_sum(acc[j], red);
    }
    if (p1 > p0) {
#pragma unroll
      for (int j = 0; j < kTile; ++j) acc[j] = acc[j] / cnt;
    }
#pragma unroll 2
    for (int p = p0 + first; p < p1; p += step) {
      const size_t o = (size_t)s.rows[p] * ncols + c0;
#pragma unroll
      for (int j = 0; j < kTile; ++j)
        if (act[j]) {
          const double nv = in[o + j] - acc[j];
          if (FIRM) {
            const double d = nv - io[o + j];
            d2[j] += d * d;
          }
          io[o + j] = nv;
        }
    }
    if (FIRM) {
#pragma unroll
      for (int j = 0; j < kTile; ++j) d2[j] = wave_sum(d2[j]);
      __syncthreads();
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kTile; ++j) dred[wave][j] = d2[j];
      }
      __syncthreads();
      if (tid < kTile && c0 + tid < ncols && done[c0 + tid] == 0) {
        double t = dred[0][tid];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += dred[w][tid];
        dpart[(size_t)blockIdx.x * ncols + c0 + tid] = t;
      }
    }
  }
}

// state of a loop: iters[c], done[c]. One block per column.
__global__ __launch_bounds__(kBlock) void akm_flag_kernel(const double* dpart, int nblocks, int ncols, double tol,
                                                           int32_t max_iters, int32_t* iters, int32_t* done) {
  __shared__ double red[kBlock];
  const int c = blockIdx.x, tid = threadIdx.x;
  if (done[c] != 0) return;
  double v = 0.0;
  for (int b = tid; b < nblocks; b += kBlock) v += dpart[(size_t)b * ncols + c];
  red[tid] = v;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double diff = sqrt(red[0]);
    const int32_t it = iters[c] + 1;
    iters[c] = it;
    if (!(diff > tol) || it >= max_iters) done[c] = 1;  // while diff > tol && iter < max_iters
  }
}

// mine[g] = mean over the group's rows of r[row] - other[oidx[row]] (an empty group keeps its
// value); dpart[block] = sum over the block's groups of (new - old)^2.
__global__ __launch_bounds__(kBlock) void akm_fe_kernel(const Seg s, const double* __restrict__ r,
                                                         const int32_t* __restrict__ oidx,
                                                         const double* __restrict__ other, double* mine,
                                                         const int32_t* __restrict__ done, double* dpart) {
#pragma clang fp contract(off)
  __shared__ double red[kWaves];
  if (done[0] != 0) return;
  int g;
  const int role = seg_role(s, &g);
  const int tid = threadIdx.x, lane = tid & 63;
  int p0 = 0, p1 = 0;
  if (g >= 0) {
    p0 = s.ptr[g];
    p1 = s.ptr[g + 1];
  }
  const int first = role == kRoleLane ? 0 : (role == kRoleWave ? lane : tid);
  const int step = role == kRoleLane ? 1 : (role == kRoleWave ? 64 : kBlock);
  double acc = 0.0;
#pragma unroll 4
  for (int p = p0 + first; p < p1; p += step) {
    const int row = s.rows[p];
    acc += r[row] - other[oidx[row]];
  }
  if (role == kRoleWave) acc = wave_sum(acc);
  else if (role == kRoleBlock) acc = block_sum(acc, red);
  double d2 = 0.0;
  if (p1 > p0 && first == 0) {  // the group's owner: its lane, lane 0 of its wave, thread 0 of its block
    const double nv = acc / (double)(p1 - p0), d = nv - mine[g];
    mine[g] = nv;
    d2 = d * d;
  }
  d2 = block_sum(d2, red);
  if (tid == 0) dpart[blockIdx.x] = d2;
}

__global__ __launch_bounds__(kBlock) void akm_fe_flag_kernel(const double* dpart, int nblocks, double tol,
                                                              int32_t max_iters, int32_t* iters, int32_t* done) {
  __shared__ double red[kBlock];
  const int tid = threadIdx.x;
  if (done[0] != 0) return;
  double v = 0.0;
  for (int b = tid; b < nblocks; b += kBlock) v += dpart[b];
  red[tid] = v;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double diff = sqrt(red[0]);
    const int32_t it = iters[0] + 1;
    iters[0] = it;
    if (!(diff > tol) || it >= max_iters) done[0] = 1;
  }
}

// x[i] += sign * ref[0]; ref is a copy, not an entry of x.
__global__ __launch_bounds__(kBlock) void akm_shift_kernel(double* x, int64_t n, const double* ref, double sign) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) x[i] += sign * ref[0];
}

// partial[e][block] for e = a * c + b: sum over the block's rows of v[row][a] v[row][b]. Block b takes
// the 64-row tiles b, b + gridDim.x, ...; a thread adds its pairs' rows in order.
__global__ __launch_bounds__(kBlock) void akm_gram_kernel(const double* __restrict__ v, int64_t n, int c,
                                                           double* partial) {
  __shared__ double t[kGramMaxC * kGramStride];
  const int tid = threadIdx.x, cc = c * c;
  double acc[kGramAcc];
#pragma unroll
  for (int q = 0; q < kGramAcc; ++q) acc[q] = 0.0;
  const int64_t ntiles = (n + kGramRows - 1) / kGramRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
    for (int i = tid; i < kGramRows * c; i += kBlock) {
      const int r = i / c, col = i - r * c;
      const int64_t row = tile * kGramRows + r;
      t[col * kGramStride + r] = row < n ? v[(size_t)row * c + col] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kGramAcc; ++q) {
      const int e = tid + q * kBlock;
      if (e < cc) {
        const double* a = t + (e / c) * kGramStride;
        const double* b = t + (e % c) * kGramStride;
        double sum = acc[q];
        for (int r = 0; r < kGramRows; ++r) sum = fma(a[r], b[r], sum);
        acc[q] = sum;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kGramAcc; ++q) {
    const int e = tid + q * kBlock;
    if (e < cc) partial[(size_t)e * gridDim.x + blockIdx.x] = acc[q];
  }
}

enum { kSumY = 0, kSumTss = 1, kSumRss = 2 };

// partial[block] = this block's rows (block-strided) of y, (y - mean)^2 or (y - pred)^2 with
// pred = x beta + alpha[w] + psi[f] (akm.rs:396-413).
template <int KIND>
__global__ __launch_bounds__(kBlock) void akm_rowsum_kernel(const double* __restrict__ raw, int64_t n, int c,
                                                             double mean, const double* __restrict__ beta,
                                                             const int32_t* __restrict__ widx,
                                                             const int32_t* __restrict__ fidx,
                                                             const double* __restrict__ alpha,
                                                             const double* __restrict__ psi, double* partial) {
#pragma clang fp contract(off)
  __shared__ double red[kWaves];
  double acc = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < n; row += (int64_t)gridDim.x * kBlock) {
    const double* x = raw + (size_t)row * c;
    if (KIND == kSumY) {
      acc += x[0];
    } else if (KIND == kSumTss) {
      const double d = x[0] - mean;
      acc += d * d;
    } else {
      double pred = alpha[widx[row]] + psi[fidx[row]];
      if (c > 1) {
        double xb = 0.0;
        for (int j = 1; j < c; ++j) xb += x[j] * beta[j - 1];
        pred = xb + alpha[widx[row]] + psi[fidx[row]];
      }
      const double d = x[0] - pred;
      acc += d * d;
    }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// r[row] = y - x_1 beta_1 - x_2 beta_2 ... in control order (akm.rs:374-381)
__global__ __launch_bounds__(kBlock) void akm_resid_kernel(const double* __restrict__ raw, int64_t n, int c,
                                                            const double* __restrict__ beta, double* r) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= n) return;
  const double* x = raw + (size_t)row * c;
  double v = x[0];
  for (int j = 1; j < c; ++j) v -= x[j] * beta[j - 1];
  r[row] = v;
}

// The elapsed time of a stretch of one stream.
struct Timer {
  Events<2> ev;
  hipStream_t st = nullptr;
  hipError_t start(hipStream_t s) {
    st = s;
    const hipError_t e = ev.create();
    return e == hipSuccess ? hipEventRecord(ev.e[0], st) : e;
  }
  // the stream must be idle after this
  hipError_t stop(double* ms) {
    hipError_t e = hipEventRecord(ev.e[1], st);
    if (e == hipSuccess) e = hipEventSynchronize(ev.e[1]);
    float f = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&f, ev.e[0], ev.e[1]);
    if (ms) *ms = f;
    return e;
  }
};

struct Grouping {
  DevBuf ptr, rows, order;
  Seg seg = {};
  unsigned blocks = 0;
};

}  // namespace

namespace ob {

struct AkmPlan {
  ob_ctx* ctx = nullptr;
  int64_t n = 0, n_workers = 0, n_firms = 0;
  int ncols = 0;
  Grouping w, f;
  DevBuf widx, fidx;
  DevBuf raw, v, mid, r, alpha, psi, dpart, state, scratch, small;
};

namespace {

// Counting sort of the row positions by group, and the schedule lists.
int build_grouping(hipStream_t st, int64_t n, const int32_t* idx, int64_t n_groups, Grouping& g) {
  std::vector<int32_t> ptr((size_t)n_groups + 1, 0), rows((size_t)n), order;
  for (int64_t i = 0; i < n; ++i) ++ptr[(size_t)idx[i] + 1];
  for (int64_t k = 0; k < n_groups; ++k) ptr[k + 1] += ptr[k];
  {
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) rows[(size_t)fill[idx[i]]++] = (int32_t)i;
  }
  std::vector<int32_t> large, medium, small;
  for (int64_t k = 0; k < n_groups; ++k) {
    const int32_t cnt = ptr[k + 1] - ptr[k];
    if (cnt > kAkmWaveMax) large.push_back((int32_t)k);
    else if (cnt > kAkmLaneMax) medium.push_back((int32_t)k);
    else small.push_back((int32_t)k);
  }
  std::stable_sort(large.begin(), large.end(),
                   [&](int32_t a, int32_t b) { return ptr[a + 1] - ptr[a] > ptr[b + 1] - ptr[b]; });
  order = large;
  order.insert(order.end(), medium.begin(), medium.end());
  order.insert(order.end(), small.begin(), small.end());
  const int64_t blocks = (int64_t)large.size() + ((int64_t)medium.size() + kWaves - 1) / kWaves +
                         ((int64_t)small.size() + kBlock - 1) / kBlock;
  OB_HIP(g.ptr.alloc(sizeof(int32_t) * ptr.size()));
  OB_HIP(g.rows.alloc(sizeof(int32_t) * rows.size()));
  OB_HIP(g.order.alloc(sizeof(int32_t) * order.size()));
  OB_HIP(hipMemcpyAsync(g.ptr.p, ptr.data(), sizeof(int32_t) * ptr.size(), hipMemcpyHostToDevice, st));
  if (n) OB_HIP(hipMemcpyAsync(g.rows.p, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice, st));
  if (n_groups)
    OB_HIP(hipMemcpyAsync(g.order.p, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, st));
  OB_HIP(hipStreamSynchronize(st));  // the host vectors go away
  g.seg.ptr = g.ptr.as<int32_t>();
  g.seg.rows = g.rows.as<int32_t>();
  g.seg.order = g.order.as<int32_t>();
  g.seg.n_large = (int32_t)large.size();
  g.seg.n_medium = (int32_t)medium.size();
  g.seg.n_small = (int32_t)small.size();
  g.blocks = (unsigned)blocks;
  return OB_OK;
}

int poll_interval() { return std::max(1, opt_int(Opt::AkmPoll, kAkmPollDefault)); }

// state: [iters[m], done[m]] as int32; zeroed, then max_iters = 0 marks every loop done at once
int init_state(AkmPlan* p, int m, int64_t max_iters, hipStream_t st) {
  OB_HIP(p->state.alloc(sizeof(int32_t) * 2 * (size_t)m));
  std::vector<int32_t> h(2 * (size_t)m, 0);
  if (max_iters <= 0) std::fill(h.begin() + m, h.end(), 1);
  OB_HIP(hipMemcpyAsync(p->state.p, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice, st));
  OB_HIP(hipStreamSynchronize(st));
  return OB_OK;
}

}  // namespace

int akm_plan_create(ob_ctx* ctx, int64_t n, const int32_t* widx, const int32_t* fidx, int64_t n_workers,
                    int64_t n_firms, AkmPlan** out) {
  *out = nullptr;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  AkmPlan* p = new AkmPlan();
  p->ctx = ctx;
  p->n = n;
  p->n_workers = n_workers;
  p->n_firms = n_firms;
  int rc = build_grouping(st, n, widx, n_workers, p->w);
  if (rc == OB_OK) rc = build_grouping(st, n, fidx, n_firms, p->f);
  auto upload = [&](DevBuf& b, const int32_t* src) -> int {
    OB_HIP(b.alloc(sizeof(int32_t) * (size_t)n));
    if (n) OB_HIP(hipMemcpyAsync(b.p, src, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    OB_HIP(hipStreamSynchronize(st));
    return OB_OK;
  };
  if (rc == OB_OK) rc = upload(p->widx, widx);
  if (rc == OB_OK) rc = upload(p->fidx, fidx);
  if (rc != OB_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return OB_OK;
}

void akm_plan_free(AkmPlan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  delete p;
}

int akm_demean(AkmPlan* p, const double* v, int n_cols, double tol, int64_t max_iters, double* out,
               int32_t* iterations, int32_t* converged, double* ms, int* launches) {
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int64_t n = p->n;
  const size_t bytes = sizeof(double) * (size_t)n * n_cols;
  p->ncols = n_cols;
  if (launches) *launches = 3;
  const int32_t cap = (int32_t)std::min<int64_t>(std::max<int64_t>(max_iters, 0), INT32_MAX);
  OB_HIP(p->raw.alloc(bytes));
  OB_HIP(p->v.alloc(bytes));
  OB_HIP(p->mid.alloc(bytes));
  OB_HIP(p->dpart.alloc(sizeof(double) * (size_t)std::max(p->f.blocks, 1u) * n_cols));
  if (n) OB_HIP(hipMemcpyAsync(p->raw.p, v, bytes, hipMemcpyHostToDevice, st));
  if (n) OB_HIP(hipMemcpyAsync(p->v.p, p->raw.p, bytes, hipMemcpyDeviceToDevice, st));
  // mid holds the worker pass's output; a frozen column of it is neither written nor read again
  OB_HIP(hipMemsetAsync(p->dpart.p, 0, p->dpart.cap, st));
  OB_TRY(init_state(p, n_cols, cap, st));
  int32_t* iters = p->state.as<int32_t>();
  int32_t* done = iters + n_cols;
  Timer tm;
  OB_HIP(tm.start(st));
  std::vector<int32_t> h(2 * (size_t)n_cols, 0);
  const int poll = poll_interval();
  for (int64_t it = 0; it < cap;) {
    const int64_t burst = std::min<int64_t>(poll, cap - it);
    for (int64_t b = 0; b < burst; ++b) {
      if (p->w.blocks)
        hipLaunchKernelGGL(akm_demean_kernel<false>, dim3(p->w.blocks), dim3(kBlock), 0, st, p->w.seg, n_cols,
                           p->v.d(), p->mid.d(), done, (double*)nullptr);
      if (p->f.blocks)
        hipLaunchKernelGGL(akm_demean_kernel<true>, dim3(p->f.blocks), dim3(kBlock), 0, st, p->f.seg, n_cols,
                           p->mid.d(), p->v.d(), done, p->dpart.d());
      hipLaunchKernelGGL(akm_flag_kernel, dim3(n_cols), dim3(kBlock), 0, st, p->dpart.d(), (int)p->f.blocks, n_cols,
                         tol, cap, iters, done);
    }
    OB_HIP(hipGetLastError());
    it += burst;
    OB_HIP(hipMemcpyAsync(h.data(), p->state.p, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    if (std::all_of(h.begin() + n_cols, h.end(), [](int32_t d) { return d != 0; })) break;
  }
  OB_HIP(tm.stop(ms));
  for (int c = 0; c < n_cols; ++c) {
    if (iterations) iterations[c] = h[c];
    if (converged) converged[c] = (int64_t)h[c] < max_iters ? 1 : 0;  // akm.rs:519
  }
  if (out && n) {
    OB_HIP(hipMemcpyAsync(out, p->v.p, bytes, hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
  }
  return OB_OK;
}

int akm_gram(AkmPlan* p, double* g, double* ms) {
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int c = p->ncols;
  if (c < 1 || c > kGramMaxC) return fail(OB_E_INVALID, "akm_gram: bad column count");
  const unsigned nblk = (unsigned)std::max<int64_t>(1, std::min<int64_t>((p->n + kGramRows - 1) / kGramRows, kGramMaxBlocks));
  OB_HIP(p->scratch.alloc(sizeof(double) * (size_t)c * c * nblk));
  OB_HIP(p->small.alloc(sizeof(double) * (size_t)c * c));
  Timer tm;
  OB_HIP(tm.start(st));
  hipLaunchKernelGGL(akm_gram_kernel, dim3(nblk), dim3(kBlock), 0, st, p->v.d(), p->n, c, p->scratch.d());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(c * c), dim3(kSumBlock), 0, st, p->scratch.d(), nblk, p->small.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipMemcpyAsync(g, p->small.p, sizeof(double) * (size_t)c * c, hipMemcpyDeviceToHost, st));
  OB_HIP(tm.stop(ms));
  return OB_OK;
}

namespace {

// beta on the device, after alpha and psi in no buffer of theirs: the tail of `small`
int upload_beta(AkmPlan* p, const double* beta, hipStream_t st, double** dbeta) {
  const int k = p->ncols - 1;
  OB_HIP(p->small.alloc(sizeof(double) * (size_t)kGramMaxC * kGramMaxC));
  if (k > 0) OB_HIP(hipMemcpyAsync(p->small.p, beta, sizeof(double) * k, hipMemcpyHostToDevice, st));
  OB_HIP(hipStreamSynchronize(st));
  *dbeta = p->small.d();
  return OB_OK;
}

}  // namespace

int akm_residual(AkmPlan* p, const double* beta, double* ms) {
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  double* dbeta = nullptr;
  OB_TRY(upload_beta(p, beta, st, &dbeta));
  OB_HIP(p->r.alloc(sizeof(double) * (size_t)p->n));
  Timer tm;
  OB_HIP(tm.start(st));
  if (p->n)
    hipLaunchKernelGGL(akm_resid_kernel, dim3(blocks_for(p->n)), dim3(kBlock), 0, st, p->raw.d(), p->n, p->ncols, dbeta,
                       p->r.d());
  OB_HIP(hipGetLastError());
  OB_HIP(tm.stop(ms));
  return OB_OK;
}

int akm_recover(AkmPlan* p, const double* r, double tol, int64_t max_iters, double* alpha, double* psi,
                int32_t* iterations, int32_t* converged, double* ms) {
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int64_t n = p->n, nw = p->n_workers, nf = p->n_firms;
  const int32_t cap = (int32_t)std::min<int64_t>(std::max<int64_t>(max_iters, 0), INT32_MAX);
  OB_HIP(p->r.alloc(sizeof(double) * (size_t)n));
  if (r && n) OB_HIP(hipMemcpyAsync(p->r.p, r, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  OB_HIP(p->alpha.alloc(sizeof(double) * (size_t)nw));
  OB_HIP(p->psi.alloc(sizeof(double) * (size_t)nf));
  OB_HIP(hipMemsetAsync(p->alpha.p, 0, p->alpha.cap, st));
  OB_HIP(hipMemsetAsync(p->psi.p, 0, p->psi.cap, st));
  const unsigned nb = p->w.blocks + p->f.blocks;
  OB_HIP(p->dpart.alloc(sizeof(double) * (size_t)std::max(nb, 1u)));
  OB_HIP(hipMemsetAsync(p->dpart.p, 0, p->dpart.cap, st));
  OB_TRY(init_state(p, 1, cap, st));
  int32_t* iters = p->state.as<int32_t>();
  int32_t* done = iters + 1;
  Timer tm;
  OB_HIP(tm.start(st));
  int32_t h[2] = {0, cap <= 0 ? 1 : 0};
  const int poll = poll_interval();
  for (int64_t it = 0; it < cap;) {
    const int64_t burst = std::min<int64_t>(poll, cap - it);
    for (int64_t b = 0; b < burst; ++b) {
      if (p->w.blocks)
        hipLaunchKernelGGL(akm_fe_kernel, dim3(p->w.blocks), dim3(kBlock), 0, st, p->w.seg, p->r.d(),
                           p->fidx.as<int32_t>(), p->psi.d(), p->alpha.d(), done, p->dpart.d());
      if (p->f.blocks)
        hipLaunchKernelGGL(akm_fe_kernel, dim3(p->f.blocks), dim3(kBlock), 0, st, p->f.seg, p->r.d(),
                           p->widx.as<int32_t>(), p->alpha.d(), p->psi.d(), done, p->dpart.d() + p->w.blocks);
      hipLaunchKernelGGL(akm_fe_flag_kernel, dim3(1), dim3(kBlock), 0, st, p->dpart.d(), (int)nb, tol, cap, iters, done);
    }
    OB_HIP(hipGetLastError());
    it += burst;
    OB_HIP(hipMemcpyAsync(h, p->state.p, sizeof(h), hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    if (h[1] != 0) break;
  }
  if (iterations) *iterations = h[0];
  const bool ok = (int64_t)h[0] < max_iters;  // akm.rs:604
  if (converged) *converged = ok ? 1 : 0;
  if (ok && nf > 0) {  // akm.rs:611-618
    OB_HIP(p->scratch.alloc(sizeof(double)));
    OB_HIP(hipMemcpyAsync(p->scratch.p, p->psi.p, sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(akm_shift_kernel, dim3(blocks_for(nf)), dim3(kBlock), 0, st, p->psi.d(), nf, p->scratch.d(), -1.0);
    if (nw)
      hipLaunchKernelGGL(akm_shift_kernel, dim3(blocks_for(nw)), dim3(kBlock), 0, st, p->alpha.d(), nw, p->scratch.d(),
                         1.0);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(tm.stop(ms));
  if (alpha && nw) OB_HIP(hipMemcpyAsync(alpha, p->alpha.p, sizeof(double) * (size_t)nw, hipMemcpyDeviceToHost, st));
  if (psi && nf) OB_HIP(hipMemcpyAsync(psi, p->psi.p, sizeof(double) * (size_t)nf, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  return OB_OK;
}

int akm_r2(AkmPlan* p, const double* beta, double* tss, double* rss, double* ms) {
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  const int64_t n = p->n;
  const int c = p->ncols;
  double* dbeta = nullptr;
  OB_TRY(upload_beta(p, beta, st, &dbeta));
  const unsigned nblk = (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks_for(n), kSumMaxBlocks));
  OB_HIP(p->scratch.alloc(sizeof(double) * ((size_t)nblk + 1)));
  double* part = p->scratch.d();
  double* total = part + nblk;
  Timer tm;
  OB_HIP(tm.start(st));
  auto finish = [&](double* host) -> int {
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(1), dim3(kSumBlock), 0, st, part, nblk, total);
    OB_HIP(hipGetLastError());
    OB_HIP(hipMemcpyAsync(host, total, sizeof(double), hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    return OB_OK;
  };
  double ysum = 0.0;
  hipLaunchKernelGGL(akm_rowsum_kernel<kSumY>, dim3(nblk), dim3(kBlock), 0, st, p->raw.d(), n, c, 0.0, dbeta,
                     p->widx.as<int32_t>(), p->fidx.as<int32_t>(), p->alpha.d(), p->psi.d(), part);
  OB_TRY(finish(&ysum));
  const double mean = ysum / (double)n;
  hipLaunchKernelGGL(akm_rowsum_kernel<kSumTss>, dim3(nblk), dim3(kBlock), 0, st, p->raw.d(), n, c, mean, dbeta,
                     p->widx.as<int32_t>(), p->fidx.as<int32_t>(), p->alpha.d(), p->psi.d(), part);
  OB_TRY(finish(tss));
  hipLaunchKernelGGL(akm_rowsum_kernel<kSumRss>, dim3(nblk), dim3(kBlock), 0, st, p->raw.d(), n, c, mean, dbeta,
                     p->widx.as<int32_t>(), p->fidx.as<int32_t>(), p->alpha.d(), p->psi.d(), part);
  OB_TRY(finish(rss));
  OB_HIP(tm.stop(ms));
  return OB_OK;
}

}  // namespace ob
