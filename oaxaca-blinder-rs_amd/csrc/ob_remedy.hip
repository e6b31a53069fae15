// ob_remedy.hip -- device passes of the pay-equity remediation (engine/src/analysis.rs:309-869,
// optimize_inner). The reference walks the employees one by one: a K-term dot product for the fair
// wage, a K x K quadratic form for the leverage, a sort of all gaps and a sequential running budget.
// Here:
//
//   ob_remedy_score_kernel     R = Xe B' for Xe = [1, x_0..x_{K-2}] over column-major x and B' = [C | beta]
//                              (C = (X_A'X_A)^-1): columns 0..K-1 of R are T = Xe C, column K is the fair
//                              wage. The epilogue dots each row of T with xe_i (the leverage, analysis.rs:523),
//                              squares the explicit residuals y_i - fair_i of the first n_rss rows (:480-481)
//                              and, on request, writes the contributions xe_ij beta_j (:723-742)
//   ob_remedy_classify_kernel  per push position (all of B, then all of A, :556-684): interval, target, diff,
//                              a 2-bit class, and per-block sums and candidate counts
//   ob_remedy_offsets_kernel   exclusive scan of the candidate counts
//   ob_remedy_compact_kernel   the candidates in push order: the order-preserving 64-bit image of diff and
//                              the push position
//   ob_remedy_radix_*_kernel   a stable LSD radix sort, 4 bits a pass, of the inverted image: descending diff,
//                              ties in push order (:709-713). rocPRIM's sort is not used: it reads an
//                              environment variable, and the shipped library reads none
//   ob_remedy_prefix_kernel    P_c within a tile of 256 sorted candidates, an inclusive Kogge-Stone scan
//   ob_remedy_tiles_kernel     the tile totals before each tile, added one by one in tile order
//   ob_remedy_pay_kernel       pay_c = clamp(budget - P_c, 0, diff_c) (greedy, :745-757) or diff_c * ratio
//                              (equitable, :790-802), and the keys of the final order
//   (the same sort by original index, ascending: :834)
//   ob_remedy_gather_kernel    the result arrays in that order
//
// check_defensibility_inner (engine/src/defensibility.rs:199-365) over the same stacked rows:
//   ob_defend_first_kernel     first[row] = the first request position that names the row (32-bit atomicMin)
//   ob_defend_adjust_kernel    per proposed adjustment, in request order: current and new wage, the fair-wage
//                              interval, is_defensible; block partials of the values (total_cost)
//   ob_defend_rows_kernel      per stacked row: the wage after its first adjustment, and block partials of the
//                              seven group sums behind the gaps and required_budget
//
// The score kernel follows ob_vif_resid_kernel: B' (at most 120 x 144 f64) stays in LDS for the whole
// block, X streams through registers in the A-operand shape of v_mfma_f64_16x16x4_f64, a wave owns a
// 16-row block and feeds up to 8 column-block accumulators. The epilogue reads the same 16 x K tile of x
// once more in the accumulator's shape (rows kq + 4 r, column 16 jb + li), which the first read left in
// cache.
//
// No floating atomics: every partial lands in its own slot and the reduce adds in a fixed order, so two
// calls on the same input give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ob_device.hpp"
#include "ob_hip.hpp"
#include "ob_remedy.hpp"

namespace {

typedef double ob_d4 __attribute__((ext_vector_type(4)));

constexpr int kScBlock = 512;
constexpr int kScWaves = kScBlock / 64;
constexpr int kScMaxJb = 8;  // 16-column blocks of the K + 1 columns of [C | beta]
constexpr int kScMaxUnits = 512;
constexpr int kAlBlock = 256;  // threads, and rows, of a block of the allocation kernels; the tile of P_c
constexpr int kAlWaves = kAlBlock / 64;

struct ScoreArgs {
  const double* x;  // device, column-major n x (k - 1)
  int64_t ldx;
  const double* y;  // device, n_rss entries
  int64_t n, n_rss;
  int k;             // design columns, the implicit intercept first
  const double* bp;  // device, B' row-major [4 ns][ldb]: row c = [C[c][0..k), beta[c]], zero outside
  int ns;            // steps of 4 design columns
  int njb;           // 16-column blocks of the k + 1 columns of B'
  int ldb;           // 16 (njb | 1), as ob_vif_resid_kernel
  int64_t nrb;       // 16-row blocks
  uint32_t gpu;      // groups of kScWaves row blocks per unit (block)
  uint32_t units;
  double* fair;
  double* lev;
  double* contrib;  // n x k column-major, or NULL
  double* partial;  // [units]: squared residuals
};

__global__ __launch_bounds__(kScBlock) void ob_remedy_score_kernel(const ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) double bs[];  // [4 ns][ldb], then red[kScWaves]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, li = lane & 15;
  const int k = a.k;
  const int nb = 4 * a.ns * a.ldb;
  double* red = bs + nb;
  for (int i = tid; i < nb; i += kScBlock) bs[i] = a.bp[i];
  __syncthreads();
  const int fj = k >> 4, fl = k & 15;  // the fair wage's column block and lane
  double ss = 0.0;
  const int64_t g0 = (int64_t)blockIdx.x * a.gpu;
  for (uint32_t g = 0; g < a.gpu; ++g) {
    const int64_t rb = (g0 + g) * kScWaves + wave;
    if (rb >= a.nrb) break;  // whole waves only: no block barrier inside the loop
    const int64_t row = rb * 16 + li;
    const bool live = row < a.n;
    ob_d4 acc[kScMaxJb];
#pragma unroll
    for (int jb = 0; jb < kScMaxJb; ++jb) acc[jb] = (ob_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < a.ns; ++s) {
      const int c = 4 * s + kq;
      double av = 0.0;
      if (live) av = c == 0 ? 1.0 : (c < k ? a.x[(size_t)(c - 1) * a.ldx + row] : 0.0);
      const double* brow = bs + c * a.ldb + li;
#pragma unroll
      for (int jb = 0; jb < kScMaxJb; ++jb)
        if (jb < a.njb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[16 * jb], acc[jb], 0, 0, 0);
    }
    // lane (kq, li), element r of acc[jb]: row 16 rb + kq + 4 r, column 16 jb + li
    double h[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int jb = 0; jb < kScMaxJb; ++jb) {
      if (jb >= a.njb) continue;
      const int col = 16 * jb + li;
      const double bcol = col < k ? bs[col * a.ldb + k] : 0.0;  // beta[col]
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row2 = rb * 16 + kq + 4 * r;
        if (row2 >= a.n) continue;
        if (col < k) {
          const double xv = col == 0 ? 1.0 : a.x[(size_t)(col - 1) * a.ldx + row2];
          h[r] = fma(acc[jb][r], xv, h[r]);
          if (a.contrib) a.contrib[(size_t)col * a.n + row2] = xv * bcol;
        } else if (jb == fj && li == fl) {
          const double f = acc[jb][r];
          a.fair[row2] = f;
          if (row2 < a.n_rss) {
            const double e = a.y[row2] - f;
            ss = fma(e, e, ss);
          }
        }
      }
    }
    // a row's K terms sit in the 16 lanes of its kq: add them with the xor butterfly at 1, 2, 4, 8
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = h[r];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 8);
      const int64_t row2 = rb * 16 + kq + 4 * r;
      if (li == 0 && row2 < a.n) a.lev[row2] = v;
    }
  }
  ss = wave_sum(ss);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < kScWaves; ++w) t += red[w];
    a.partial[blockIdx.x] = t;
  }
}

enum : uint8_t { kDropped = 0, kForensic = 1, kEligible = 2 };

struct ClassArgs {
  const double *y, *fair, *lev;  // device, stacked: A's n_a rows, then B's n_b
  int64_t n_a, n_b, n_push;      // push positions: all of B, then (if visited) all of A
  double sigma2, z, min_pct;
  int range_target, forensic, both;
  double *lower, *upper, *diff;  // [n_push]
  uint8_t* cls;                  // [n_push]
  double* partial;               // [2][blocks]: net_residual_sum_b, total_need
  uint32_t* count;               // [blocks]
  uint32_t blocks;
};

__device__ __forceinline__ int64_t push_row(int64_t q, int64_t n_a, int64_t n_b) { return q < n_b ? n_a + q : q - n_b; }

__global__ __launch_bounds__(kAlBlock) void ob_remedy_classify_kernel(const ClassArgs a) {
  __shared__ double red[2][kAlWaves];
  __shared__ uint32_t cnt[kAlWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = (int64_t)blockIdx.x * kAlBlock + tid;
  double net = 0.0, need = 0.0;
  bool cand = false;
  if (q < a.n_push) {
    const bool is_b = q < a.n_b;
    const int64_t row = push_row(q, a.n_a, a.n_b);
    const double actual = a.y[row], fair = a.fair[row];
    double lo = fair, up = fair;
    if (!(a.sigma2 <= 1e-9)) {  // analysis.rs:516-530
      const double margin = a.z * sqrt(a.sigma2 * (1.0 + a.lev[row]));
      lo = fair - margin;
      up = fair + margin;
    }
    // B's target follows RangeTarget (:568-576); A's diff is always against the midpoint (:635)
    const double target = !is_b || a.range_target == OB_REMEDY_MIDPOINT ? fair : (a.range_target == OB_REMEDY_LOWER ? lo : up);
    const double diff = target - actual;
    bool elig = false;
    if (diff > 1e-6) {
      const double gap_pct = fabs(actual) > 1e-6 ? diff / actual : 0.0;
      elig = (is_b || a.both) && gap_pct >= a.min_pct;
    }
    const uint8_t c = elig ? kEligible : (a.forensic ? kForensic : kDropped);
    a.lower[q] = lo;
    a.upper[q] = up;
    a.diff[q] = diff;
    a.cls[q] = c;
    if (is_b) net = diff;  // :581, every row of B and none of A
    if (elig) need = diff;
    cand = c != kDropped;
  }
  net = wave_sum(net);
  need = wave_sum(need);
  const uint32_t nc = (uint32_t)__popcll(__ballot(cand));
  if (lane == 0) {
    red[0][wave] = net;
    red[1][wave] = need;
    cnt[wave] = nc;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = red[0][0], s1 = red[1][0];
    uint32_t c = cnt[0];
    for (int w = 1; w < kAlWaves; ++w) {
      s0 += red[0][w];
      s1 += red[1][w];
      c += cnt[w];
    }
    a.partial[blockIdx.x] = s0;
    a.partial[(size_t)a.blocks + blockIdx.x] = s1;
    a.count[blockIdx.x] = c;
  }
}

// offs[b] = count[0] + .. + count[b - 1], offs[blocks] = the total. One block.
__global__ __launch_bounds__(kAlBlock) void ob_remedy_offsets_kernel(const uint32_t* count, uint32_t blocks, uint32_t* offs) {
  __shared__ uint32_t part[kAlBlock];
  const int tid = threadIdx.x;
  const uint32_t chunk = (blocks + kAlBlock - 1) / kAlBlock;
  const uint32_t b0 = min(blocks, tid * chunk), b1 = min(blocks, b0 + chunk);
  uint32_t s = 0;
  for (uint32_t b = b0; b < b1; ++b) s += count[b];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int t = 0; t < kAlBlock; ++t) {
      const uint32_t v = part[t];
      part[t] = run;
      run += v;
    }
    offs[blocks] = run;
  }
  __syncthreads();
  uint32_t run = part[tid];
  for (uint32_t b = b0; b < b1; ++b) {
    offs[b] = run;
    run += count[b];
  }
}

// Larger diff, SMALLER key (the sort is ascending); -0.0 and +0.0 share one key, as partial_cmp sees them.
__device__ __forceinline__ uint64_t diff_key(double d) {
  const uint64_t b = (uint64_t)__double_as_longlong(d + 0.0);
  return (b >> 63) ? b : ~(b | 0x8000000000000000ull);
}

constexpr int kRxBins = 16;  // 4 bits a pass

// One pass of the sort, first half: counts[d * blocks + b] = keys of block b whose digit at `shift` is d.
__global__ __launch_bounds__(kAlBlock) void ob_remedy_radix_count_kernel(const uint64_t* key, uint32_t m, int shift,
                                                                         uint32_t blocks, uint32_t* counts) {
  __shared__ uint32_t cnt[kAlWaves][kRxBins];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t c = blockIdx.x * kAlBlock + tid;
  const bool live = c < m;
  const int d = live ? (int)((key[c] >> shift) & (kRxBins - 1)) : 0;
#pragma unroll
  for (int b = 0; b < kRxBins; ++b) {
    const uint64_t mb = __ballot(live && d == b);
    if (lane == 0) cnt[wave][b] = (uint32_t)__popcll(mb);
  }
  __syncthreads();
  if (tid < kRxBins) {
    uint32_t s = 0;
    for (int w = 0; w < kAlWaves; ++w) s += cnt[w][tid];
    counts[(size_t)tid * blocks + blockIdx.x] = s;
  }
}

// Second half: offs is the exclusive scan of counts (digit-major, then block); within a block the keys of
// one digit keep their order (earlier waves first, then the lane rank), so the pass is stable.
__global__ __launch_bounds__(kAlBlock) void ob_remedy_radix_scatter_kernel(const uint64_t* key, const uint32_t* val, uint32_t m,
                                                                           int shift, uint32_t blocks, const uint32_t* offs,
                                                                           uint64_t* key_out, uint32_t* val_out) {
  __shared__ uint32_t cnt[kAlWaves][kRxBins];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t c = blockIdx.x * kAlBlock + tid;
  const bool live = c < m;
  const uint64_t kv = live ? key[c] : 0;
  const int d = (int)((kv >> shift) & (kRxBins - 1));
  uint64_t mine = 0;
#pragma unroll
  for (int b = 0; b < kRxBins; ++b) {
    const uint64_t mb = __ballot(live && d == b);
    if (d == b) mine = mb;
    if (lane == 0) cnt[wave][b] = (uint32_t)__popcll(mb);
  }
  __syncthreads();
  if (live) {
    uint32_t pos = offs[(size_t)d * blocks + blockIdx.x] + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += cnt[w][d];
    key_out[pos] = kv;
    val_out[pos] = val[c];
  }
}

__global__ __launch_bounds__(kAlBlock) void ob_remedy_compact_kernel(const double* diff, const uint8_t* cls, int64_t n_push,
                                                                     const uint32_t* offs, uint64_t* key, uint32_t* val) {
  __shared__ uint32_t cnt[kAlWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = (int64_t)blockIdx.x * kAlBlock + tid;
  const bool cand = q < n_push && cls[q] != kDropped;
  const uint64_t m = __ballot(cand);
  if (lane == 0) cnt[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  if (cand) {
    uint32_t pos = offs[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += cnt[w];
    key[pos] = diff_key(diff[q]);
    val[pos] = (uint32_t)q;
  }
}

// pre[c]: the eligible diffs before c within its tile. tot[t]: the tile's total.
__global__ __launch_bounds__(kAlBlock) void ob_remedy_prefix_kernel(const double* diff, const uint8_t* cls, const uint32_t* sval,
                                                                    uint32_t m, double* pre, double* tot) {
  __shared__ double s[kAlBlock];
  const int tid = threadIdx.x;
  const uint32_t c = blockIdx.x * kAlBlock + tid;
  double v = 0.0;
  if (c < m) {
    const uint32_t q = sval[c];
    if (cls[q] == kEligible) v = diff[q];
  }
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < kAlBlock; off <<= 1) {
    const double t = tid >= off ? s[tid - off] : 0.0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  if (c < m) pre[c] = tid ? s[tid - 1] : 0.0;
  if (tid == 0) tot[blockIdx.x] = s[kAlBlock - 1];
}

__global__ void ob_remedy_tiles_kernel(double* tot, uint32_t tiles) {
  if (blockIdx.x || threadIdx.x) return;
  double run = 0.0;
  for (uint32_t t = 0; t < tiles; ++t) {
    const double v = tot[t];
    tot[t] = run;
    run += v;
  }
}

struct PayArgs {
  const double* diff;
  const uint8_t* cls;
  const uint32_t* sval;
  uint32_t m;
  const double *pre, *tileoff;
  int strategy;
  double budget, ratio;
  const int64_t* index;  // device, stacked rows, or NULL
  int64_t n_a, n_b;
  double* pay;      // [m], sorted order
  double* partial;  // [tiles]
  uint64_t* key2;   // [m]: original index
  uint32_t* val2;   // [m]: sorted position
};

__global__ __launch_bounds__(kAlBlock) void ob_remedy_pay_kernel(const PayArgs a) {
  __shared__ double red[kAlWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t c = blockIdx.x * kAlBlock + tid;
  double pay = 0.0;
  if (c < a.m) {
    const uint32_t q = a.sval[c];
    const double d = a.diff[q];
    if (a.cls[q] == kEligible) {
      if (a.strategy == OB_REMEDY_EQUITABLE) {
        pay = d * a.ratio;
      } else {
        const double remaining = a.budget - (a.tileoff[blockIdx.x] + a.pre[c]);
        pay = remaining > 0.0 ? fmin(d, remaining) : 0.0;
      }
    }
    a.pay[c] = pay;
    const int64_t row = push_row(q, a.n_a, a.n_b);
    a.key2[c] = (uint64_t)(a.index ? a.index[row] : row);
    a.val2[c] = c;
  }
  pay = wave_sum(pay);
  if (lane == 0) red[wave] = pay;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < kAlWaves; ++w) t += red[w];
    a.partial[blockIdx.x] = t;
  }
}

struct GatherArgs {
  const uint64_t* skey2;
  const uint32_t *sval2, *sval;
  uint32_t m;
  const double *pay, *y, *fair, *lower, *upper;
  int64_t n_a, n_b;
  int64_t *index, *row;
  double *adjustment, *current, *new_wage, *fair_out, *lower_out, *upper_out;
  int32_t* group;
};

__global__ __launch_bounds__(kAlBlock) void ob_remedy_gather_kernel(const GatherArgs a) {
  const uint32_t o = blockIdx.x * kAlBlock + threadIdx.x;
  if (o >= a.m) return;
  const uint32_t c = a.sval2[o], q = a.sval[c];
  const int64_t row = push_row(q, a.n_a, a.n_b);
  const double pay = a.pay[c], cur = a.y[row];
  a.index[o] = (int64_t)a.skey2[o];
  a.row[o] = row;
  a.group[o] = q < a.n_b ? 1 : 0;
  a.adjustment[o] = pay;
  a.current[o] = cur;
  a.new_wage[o] = cur + pay;  // :761
  a.fair_out[o] = a.fair[row];
  a.lower_out[o] = a.lower[q];
  a.upper_out[o] = a.upper[q];
}

// ---- efficient frontier (analysis.rs:871-1153) -------------------------------------------------------------
// Pooled design X_p = [1, group dummy (A = 0, B = 1), features]; Y[:, s] = y + pay_s with pay_s[i] =
// clamp(b_s - P_i, 0, gap_i), b_s = s * step, recomputed per tile and never stored (:1119-1141 in closed form).
constexpr int kFrStride = 66;    // doubles per staged column, as ob_vif_gram_kernel
constexpr int kFrMaxAcc = 16;    // block pairs per wave: 8 design blocks x 8 step blocks over 4 waves
constexpr int kFrMaxUnits = 512;

struct FrontArgs {
  const double* x;  // device, column-major n x (k - 1) features, A's rows first
  int64_t ldx;
  const double *y, *gap, *pre;  // device, n entries: wage, the gap to pay (0 for a non-candidate), P_i
  int64_t n, n_a;
  int k1;        // pooled design columns: k + 1
  int s;         // budgets: steps + 1
  double step;
  int nxb, nsb;  // 16-column blocks of the k1 design columns and of the s budgets
  uint32_t nsub, spu, units;
  double* partial;  // [k1 * s][units]
};

__device__ __forceinline__ double front_design(const FrontArgs& a, int c, int64_t row) {
  return c == 0 ? 1.0 : (c == 1 ? (row >= a.n_a ? 1.0 : 0.0) : a.x[(size_t)(c - 2) * a.ldx + row]);
}

__device__ __forceinline__ double front_pay(double budget, double pre, double gap) {
  const double remaining = budget - pre;
  return remaining > 0.0 ? fmin(remaining, gap) : 0.0;
}

// X_p' Y as per-block partials: a 64-row sub-tile of X_p's columns and of the s columns of Y is staged once in
// LDS (lane = row, coalesced column reads) and the (design block, step block) pairs are dealt over the waves.
__global__ __launch_bounds__(kAlBlock) void ob_remedy_front_xty_kernel(const FrontArgs a) {
  extern __shared__ __attribute__((aligned(16))) double xs[];  // [16 (nxb + nsb)][kFrStride]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, li = lane & 15;
  const int np = a.nxb * a.nsb, ncol = 16 * (a.nxb + a.nsb), y0 = 16 * a.nxb;
  ob_d4 acc[kFrMaxAcc];
#pragma unroll
  for (int t = 0; t < kFrMaxAcc; ++t) acc[t] = (ob_d4){0.0, 0.0, 0.0, 0.0};
  const int nacc = wave < np ? (np - wave + kAlWaves - 1) / kAlWaves : 0;
  for (int c = wave; c < ncol; c += kAlWaves) xs[c * kFrStride + lane] = 0.0;  // the padding columns stay zero
  __syncthreads();
  const uint32_t s0 = blockIdx.x * a.spu, s1 = min(a.nsub, s0 + a.spu);
  for (uint32_t sub = s0; sub < s1; ++sub) {
    const int64_t row = (int64_t)sub * 64 + lane;
    const bool live = row < a.n;
    for (int c = wave; c < a.k1; c += kAlWaves) xs[c * kFrStride + lane] = live ? front_design(a, c, row) : 0.0;
    const double yv = live ? a.y[row] : 0.0, gv = live ? a.gap[row] : 0.0, pv = live ? a.pre[row] : 0.0;
    for (int s = wave; s < a.s; s += kAlWaves)
      xs[(y0 + s) * kFrStride + lane] = live ? yv + front_pay((double)s * a.step, pv, gv) : 0.0;
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < 16; ++ks) {
      const int r = li * kFrStride + 4 * ks + kq;
#pragma unroll
      for (int t = 0; t < kFrMaxAcc; ++t)
        if (t < nacc) {
          const int q = wave + kAlWaves * t;
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[16 * (q / a.nsb) * kFrStride + r],
                                                        xs[(y0 + 16 * (q % a.nsb)) * kFrStride + r], acc[t], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  // D(I, J)[i][j] sits in lane (i % 4) * 16 + j, element i / 4: design column 16 I + i, budget 16 J + j
#pragma unroll
  for (int t = 0; t < kFrMaxAcc; ++t)
    if (t < nacc) {
      const int q = wave + kAlWaves * t;
      const int sj = 16 * (q % a.nsb) + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * (q / a.nsb) + kq + 4 * r;
        if (c < a.k1 && sj < a.s) a.partial[((size_t)c * a.s + sj) * a.units + blockIdx.x] = acc[t][r];
      }
    }
}

struct FrontRssArgs {
  FrontArgs f;
  const double* bp;  // device, row-major [4 ns][ldb]: row c = beta_s[c] over the budgets s, zero outside
  int ns, njb, ldb;
  int64_t nrb;
  uint32_t gpu, runits;
  double* rpartial;  // [s][runits]
};

// rss_s = sum_i (y_i + pay_si - x_pi . beta_s)^2 for every s from explicit residuals, in the shape of
// ob_vif_resid_kernel: the coefficients in LDS, X_p through registers, a wave per 16-row block.
__global__ __launch_bounds__(kScBlock) void ob_remedy_front_rss_kernel(const FrontRssArgs a) {
  extern __shared__ __attribute__((aligned(16))) double bs[];  // [4 ns][ldb], then red[kScWaves][16 kScMaxJb]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, li = lane & 15;
  const int nb = 4 * a.ns * a.ldb;
  double* red = bs + nb;
  for (int i = tid; i < nb; i += kScBlock) bs[i] = a.bp[i];
  __syncthreads();
  double ss[kScMaxJb];
#pragma unroll
  for (int jb = 0; jb < kScMaxJb; ++jb) ss[jb] = 0.0;
  const int64_t g0 = (int64_t)blockIdx.x * a.gpu;
  for (uint32_t g = 0; g < a.gpu; ++g) {
    const int64_t rb = (g0 + g) * kScWaves + wave;
    if (rb >= a.nrb) break;  // whole waves only
    const int64_t row = rb * 16 + li;
    const bool live = row < a.f.n;
    ob_d4 acc[kScMaxJb];
#pragma unroll
    for (int jb = 0; jb < kScMaxJb; ++jb) acc[jb] = (ob_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < a.ns; ++s) {
      const int c = 4 * s + kq;
      const double av = live && c < a.f.k1 ? front_design(a.f, c, row) : 0.0;
      const double* brow = bs + c * a.ldb + li;
#pragma unroll
      for (int jb = 0; jb < kScMaxJb; ++jb)
        if (jb < a.njb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[16 * jb], acc[jb], 0, 0, 0);
    }
    // lane (kq, li), element r of acc[jb]: row 16 rb + kq + 4 r, budget 16 jb + li
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row2 = rb * 16 + kq + 4 * r;
      if (row2 >= a.f.n) continue;
      const double yv = a.f.y[row2], gv = a.f.gap[row2], pv = a.f.pre[row2];
#pragma unroll
      for (int jb = 0; jb < kScMaxJb; ++jb) {
        const int sj = 16 * jb + li;
        if (jb < a.njb && sj < a.f.s) {
          const double e = yv + front_pay((double)sj * a.f.step, pv, gv) - acc[jb][r];
          ss[jb] = fma(e, e, ss[jb]);
        }
      }
    }
  }
#pragma unroll
  for (int jb = 0; jb < kScMaxJb; ++jb) {
    double v = ss[jb];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (kq == 0) red[wave * 16 * kScMaxJb + 16 * jb + li] = v;
  }
  __syncthreads();
  if (tid < a.f.s) {
    double t = red[tid];
    for (int w = 1; w < kScWaves; ++w) t += red[w * 16 * kScMaxJb + tid];
    a.rpartial[(size_t)tid * a.runits + blockIdx.x] = t;
  }
}

// ---- defensibility (engine/src/defensibility.rs:199-365) ---------------------------------------------------
// The reference looks every row's adjustment up by walking the whole result list (:292-301, :343-349) and stops at
// the first hit. Here first[row] = the smallest request position that names the row, by an integer atomicMin
// (order-free, so deterministic), and one pass over the rows reads its adjustment through that map.
// A row nobody names keeps 0xffffffff, above every position (m < 2^31 - 1).
constexpr int kDfSums = 7;  // the row sums; total_cost is the per-adjustment kernel's

__global__ __launch_bounds__(kAlBlock) void ob_defend_first_kernel(const uint32_t* row, uint32_t m, uint32_t* first) {
  const uint32_t j = blockIdx.x * kAlBlock + threadIdx.x;
  if (j < m) atomicMin(&first[row[j]], j);
}

// defensibility.rs:156-165, apart from ob_remedy_classify_kernel's copy on purpose: that one's bytes are pinned by
// the optimize tests.
__device__ __forceinline__ void defend_interval(double fair, double lev, double sigma2, double z, double& lo, double& up) {
  lo = fair;
  up = fair;
  if (!(sigma2 <= 1e-9)) {
    const double margin = z * sqrt(sigma2 * (1.0 + lev));
    lo = fair - margin;
    up = fair + margin;
  }
}

struct DefendAdjArgs {
  const double *y, *fair, *lev;  // device, stacked rows
  const uint32_t* row;           // [m] stacked row of each adjustment, request order
  const double* value;           // [m]
  uint32_t m;
  double sigma2, z;
  double *current, *new_wage, *fair_out, *lower, *upper;  // [m]
  int32_t* flag;                                           // [m] is_defensible
  double* partial;                                         // [blocks]: the values (total_cost)
};

__global__ __launch_bounds__(kAlBlock) void ob_defend_adjust_kernel(const DefendAdjArgs a) {
  __shared__ double red[kAlWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t j = blockIdx.x * kAlBlock + tid;
  double v = 0.0;
  if (j < a.m) {
    const uint32_t row = a.row[j];
    v = a.value[j];
    const double cur = a.y[row], fair = a.fair[row];
    const double nw = cur + v;  // :222
    double lo, up;
    defend_interval(fair, a.lev[row], a.sigma2, a.z, lo, up);
    a.current[j] = cur;
    a.new_wage[j] = nw;
    a.fair_out[j] = fair;
    a.lower[j] = lo;
    a.upper[j] = up;
    a.flag[j] = nw >= lo - 1.0 ? 1 : 0;  // :225
  }
  v = wave_sum(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < kAlWaves; ++w) t += red[w];
    a.partial[blockIdx.x] = t;
  }
}

struct DefendRowArgs {
  const double *y, *fair;  // device, stacked: A's n_a rows, then B's
  const uint32_t* first;   // [n]
  const double* value;     // [m]
  uint32_t m;
  int64_t n_a, n;
  double* partial;  // [kDfSums][blocks]: sum_A y, sum_A new, sum_B y, sum_B new, sum_B (fair - y), sum_B (fair - new),
                    // sum_B max(fair - y, 0)
  uint32_t blocks;
};

__global__ __launch_bounds__(kAlBlock) void ob_defend_rows_kernel(const DefendRowArgs a) {
  __shared__ double red[kDfSums][kAlWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * kAlBlock + tid;
  double s[kDfSums];
#pragma unroll
  for (int q = 0; q < kDfSums; ++q) s[q] = 0.0;
  if (i < a.n) {
    const double y = a.y[i];
    const uint32_t f = a.first[i];
    const double nw = f < a.m ? y + a.value[f] : y;  // the first adjustment of the row decides (:296-301)
    if (i < a.n_a) {
      s[0] = y;
      s[1] = nw;
    } else {
      const double fair = a.fair[i];
      s[2] = y;
      s[3] = nw;
      s[4] = fair - y;
      s[5] = fair - nw;
      if (fair > y) s[6] = fair - y;  // :272
    }
  }
#pragma unroll
  for (int q = 0; q < kDfSums; ++q) {
    const double t = wave_sum(s[q]);
    if (lane == 0) red[q][wave] = t;
  }
  __syncthreads();
  if (tid < kDfSums) {
    double t = red[tid][0];
    for (int w = 1; w < kAlWaves; ++w) t += red[tid][w];
    a.partial[(size_t)tid * a.blocks + blockIdx.x] = t;
  }
}

}  // namespace

namespace ob {

int remedy_front_xty_device(ob_ctx* ctx, const double* dx, int64_t ldx, const double* dy, const double* dgap,
                            const double* dpre, int64_t n, int64_t n_a, int k, int s, double step, double* xty,
                            double* ms_out) {
  if (ms_out) *ms_out = 0.0;
  const int k1 = k + 1;
  FrontArgs a = {};
  a.x = dx; a.ldx = ldx; a.y = dy; a.gap = dgap; a.pre = dpre; a.n = n; a.n_a = n_a; a.k1 = k1; a.s = s; a.step = step;
  a.nxb = (k1 + 15) / 16;
  a.nsb = (s + 15) / 16;
  if (a.nxb > 8 || a.nsb > 8) return fail(OB_E_UNSUPPORTED, "frontier: too many columns or steps");
  a.nsub = (uint32_t)((n + 63) / 64);
  a.spu = (a.nsub + kFrMaxUnits - 1) / kFrMaxUnits;
  a.units = (a.nsub + a.spu - 1) / a.spu;
  const int ne = k1 * s;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dpart, dsum;
  OB_HIP(dpart.alloc(sizeof(double) * (size_t)ne * a.units));
  OB_HIP(dsum.alloc(sizeof(double) * ne));
  a.partial = dpart.d();
  Events<2> ev;
  OB_HIP(ev.create());
  const size_t lds = sizeof(double) * 16 * (a.nxb + a.nsb) * kFrStride;
  OB_HIP(hipFuncSetAttribute((const void*)ob_remedy_front_xty_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(ob_remedy_front_xty_kernel, dim3(a.units), dim3(kAlBlock), lds, st, a);
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(ne), dim3(kSumBlock), 0, st, dpart.d(), a.units, dsum.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], st));
  OB_HIP(hipMemcpyAsync(xty, dsum.p, sizeof(double) * ne, hipMemcpyDeviceToHost, st));  // [c][s]
  OB_HIP(hipStreamSynchronize(st));
  if (ms_out) {
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    *ms_out = ms;
  }
  return OB_OK;
}

int remedy_front_rss_device(ob_ctx* ctx, const double* dx, int64_t ldx, const double* dy, const double* dgap,
                            const double* dpre, int64_t n, int64_t n_a, int k, int s, double step, const double* beta,
                            double* rss, double* ms_out) {
  if (ms_out) *ms_out = 0.0;
  const int k1 = k + 1;
  FrontRssArgs a = {};
  a.f.x = dx; a.f.ldx = ldx; a.f.y = dy; a.f.gap = dgap; a.f.pre = dpre; a.f.n = n; a.f.n_a = n_a; a.f.k1 = k1; a.f.s = s;
  a.f.step = step;
  a.ns = (k1 + 3) / 4;
  a.njb = (s + 15) / 16;
  if (a.njb > kScMaxJb || k1 > 124) return fail(OB_E_UNSUPPORTED, "frontier: too many columns or steps");
  a.ldb = 16 * (a.njb | 1);
  a.nrb = (n + 15) / 16;
  const int64_t ngroups = (a.nrb + kScWaves - 1) / kScWaves;
  a.gpu = (uint32_t)((ngroups + kScMaxUnits - 1) / kScMaxUnits);
  a.runits = (uint32_t)((ngroups + a.gpu - 1) / a.gpu);
  const size_t nb = (size_t)4 * a.ns * a.ldb;
  std::vector<double> bp(nb, 0.0);
  for (int c = 0; c < k1; ++c)
    for (int j = 0; j < s; ++j) bp[(size_t)c * a.ldb + j] = beta[c + (size_t)j * k1];  // beta: k1 x s column-major
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dbp, dpart, dsum;
  OB_HIP(dbp.alloc(sizeof(double) * nb));
  OB_HIP(dpart.alloc(sizeof(double) * (size_t)s * a.runits));
  OB_HIP(dsum.alloc(sizeof(double) * s));
  a.bp = dbp.d();
  a.rpartial = dpart.d();
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipMemcpyAsync(dbp.p, bp.data(), sizeof(double) * nb, hipMemcpyHostToDevice, st));
  const size_t lds = sizeof(double) * (nb + (size_t)kScWaves * 16 * kScMaxJb);
  OB_HIP(hipFuncSetAttribute((const void*)ob_remedy_front_rss_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(ob_remedy_front_rss_kernel, dim3(a.runits), dim3(kScBlock), lds, st, a);
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(s), dim3(kSumBlock), 0, st, dpart.d(), a.runits, dsum.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], st));
  OB_HIP(hipMemcpyAsync(rss, dsum.p, sizeof(double) * s, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  if (ms_out) {
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    *ms_out = ms;
  }
  return OB_OK;
}

}  // namespace ob

namespace {

}  // namespace

namespace ob {

// Stable ascending sort of (key, val) pairs on the low `bits` bits of the keys. The pairs ping-pong
// between (k0, v0) and (k1, v1); rk and rv point at the sorted ones. counts: 16 tiles entries, offs: one more.
static int remedy_radix_sort(hipStream_t st, uint64_t* k0, uint32_t* v0, uint64_t* k1, uint32_t* v1, uint32_t m, int bits,
                             uint32_t* counts, uint32_t* offs, uint64_t*& rk, uint32_t*& rv) {
  const uint32_t tiles = (m + kAlBlock - 1) / kAlBlock;
  rk = k0;
  rv = v0;
  for (int shift = 0; shift < bits; shift += 4) {
    uint64_t* ko = rk == k0 ? k1 : k0;
    uint32_t* vo = rv == v0 ? v1 : v0;
    hipLaunchKernelGGL(ob_remedy_radix_count_kernel, dim3(tiles), dim3(kAlBlock), 0, st, rk, m, shift, tiles, counts);
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_remedy_offsets_kernel, dim3(1), dim3(kAlBlock), 0, st, counts, kRxBins * tiles, offs);
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_remedy_radix_scatter_kernel, dim3(tiles), dim3(kAlBlock), 0, st, rk, rv, m, shift, tiles, offs, ko,
                       vo);
    OB_HIP(hipGetLastError());
    rk = ko;
    rv = vo;
  }
  return OB_OK;
}

int remedy_score_device(ob_ctx* ctx, const double* dx, int64_t ldx, const double* dy, int64_t n, int64_t n_rss, int k,
                        const double* beta, const double* cov, double* dfair, double* dlev, double* rss,
                        double* dcontrib, double* ms_out) {
  if (ms_out) *ms_out = 0.0;
  if (rss) *rss = 0.0;
  OB_TRY(remedy_check_shape(n, k));
  if (!ctx || !beta || !cov || !dfair || !dlev || (k > 1 && !dx)) return fail(OB_E_INVALID, "null pointer");
  if (ldx < n || n_rss < 0 || n_rss > n || (n_rss > 0 && !dy)) return fail(OB_E_INVALID, "bad remedy dimensions");
  if (n == 0) return OB_OK;
  ScoreArgs a = {};
  a.x = dx;
  a.ldx = ldx;
  a.y = dy;
  a.n = n;
  a.n_rss = n_rss;
  a.k = k;
  a.ns = (k + 3) / 4;
  a.njb = (k + 1 + 15) / 16;
  a.ldb = 16 * (a.njb | 1);
  a.nrb = (n + 15) / 16;
  const int64_t ngroups = (a.nrb + kScWaves - 1) / kScWaves;
  a.gpu = (uint32_t)((ngroups + kScMaxUnits - 1) / kScMaxUnits);
  a.units = (uint32_t)((ngroups + a.gpu - 1) / a.gpu);
  a.fair = dfair;
  a.lev = dlev;
  a.contrib = dcontrib;
  const size_t nb = (size_t)4 * a.ns * a.ldb;
  std::vector<double> bp(nb, 0.0);
  for (int c = 0; c < k; ++c) {
    for (int j = 0; j < k; ++j) bp[(size_t)c * a.ldb + j] = cov[c + (size_t)j * k];
    bp[(size_t)c * a.ldb + k] = beta[c];
  }
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dbp, dpart, dsum;
  OB_HIP(dbp.alloc(sizeof(double) * nb));
  OB_HIP(dpart.alloc(sizeof(double) * a.units));
  OB_HIP(dsum.alloc(sizeof(double)));
  a.bp = dbp.d();
  a.partial = dpart.d();
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipMemcpyAsync(dbp.p, bp.data(), sizeof(double) * nb, hipMemcpyHostToDevice, st));
  const size_t lds = sizeof(double) * (nb + kScWaves);
  OB_HIP(hipFuncSetAttribute((const void*)ob_remedy_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  OB_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(ob_remedy_score_kernel, dim3(a.units), dim3(kScBlock), lds, st, a);
  OB_HIP(hipGetLastError());
  hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(1), dim3(kSumBlock), 0, st, dpart.d(), a.units, dsum.d());
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[1], st));
  double sum = 0.0;
  OB_HIP(hipMemcpyAsync(&sum, dsum.p, sizeof(double), hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));  // bp is read by the copy above until here
  if (ms_out) {
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    *ms_out = ms;
  }
  if (rss) *rss = sum;
  return OB_OK;
}

int remedy_allocate_device(ob_ctx* ctx, const double* dy, const double* dfair, const double* dlev, int64_t n_a,
                           int64_t n_b, const int64_t* index, double sigma2, const ob_remedy_request& rq,
                           ob_remedy_results& out) {
  if (!ctx || !dy || !dfair || !dlev) return fail(OB_E_INVALID, "null pointer");
  const int64_t n = n_a + n_b;
  const bool forensic = rq.forensic_mode != 0, both = rq.adjust_both_groups != 0;
  const int64_t n_push = n_b + (both || forensic ? n_a : 0);  // analysis.rs:631
  ob_remedy_info& info = out.info;
  info = ob_remedy_info();
  info.n_a = n_a;
  info.n_b = n_b;
  info.sigma_squared = sigma2;
  info.z_score = remedy_z_score(rq.confidence_level);
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events<4> ev;
  OB_HIP(ev.create());
  DevBuf dlower, dupper, ddiff, dcls, dpart, dcount, doffs, dsum, dindex;
  double sums[2] = {0.0, 0.0};
  uint32_t m = 0;
  const uint32_t blocks = (uint32_t)((n_push + kAlBlock - 1) / kAlBlock);
  if (index) {
    OB_HIP(dindex.alloc(sizeof(int64_t) * (size_t)n));
    OB_HIP(hipMemcpyAsync(dindex.p, index, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
  }
  OB_HIP(hipEventRecord(ev.e[0], st));
  if (n_push > 0) {
    OB_HIP(dlower.alloc(sizeof(double) * (size_t)n_push));
    OB_HIP(dupper.alloc(sizeof(double) * (size_t)n_push));
    OB_HIP(ddiff.alloc(sizeof(double) * (size_t)n_push));
    OB_HIP(dcls.alloc((size_t)n_push));
    OB_HIP(dpart.alloc(sizeof(double) * 2 * blocks));
    OB_HIP(dcount.alloc(sizeof(uint32_t) * blocks));
    OB_HIP(doffs.alloc(sizeof(uint32_t) * ((size_t)blocks + 1)));
    OB_HIP(dsum.alloc(sizeof(double) * 2));
    ClassArgs c = {};
    c.y = dy;
    c.fair = dfair;
    c.lev = dlev;
    c.n_a = n_a;
    c.n_b = n_b;
    c.n_push = n_push;
    c.sigma2 = sigma2;
    c.z = info.z_score;
    c.min_pct = rq.min_gap_pct;
    c.range_target = rq.range_target;
    c.forensic = forensic;
    c.both = both;
    c.lower = dlower.d();
    c.upper = dupper.d();
    c.diff = ddiff.d();
    c.cls = dcls.as<uint8_t>();
    c.partial = dpart.d();
    c.count = dcount.as<uint32_t>();
    c.blocks = blocks;
    hipLaunchKernelGGL(ob_remedy_classify_kernel, dim3(blocks), dim3(kAlBlock), 0, st, c);
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(2), dim3(kSumBlock), 0, st, dpart.d(), blocks, dsum.d());
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_remedy_offsets_kernel, dim3(1), dim3(kAlBlock), 0, st, dcount.as<uint32_t>(), blocks,
                       doffs.as<uint32_t>());
    OB_HIP(hipGetLastError());
    OB_HIP(hipMemcpyAsync(sums, dsum.p, sizeof(sums), hipMemcpyDeviceToHost, st));
    OB_HIP(hipMemcpyAsync(&m, doffs.as<uint32_t>() + blocks, sizeof(m), hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
  }
  const double net = sums[0], need = sums[1];
  const double budget = rq.budget > 0.0 ? rq.budget : need * 1.00001;  // analysis.rs:697-703
  info.net_residual_sum_b = net;
  info.required_budget = need;
  info.effective_budget = budget;
  info.n_adjustments = m;
  double cost = 0.0;
  if (m > 0) {
    const uint32_t tiles = (m + kAlBlock - 1) / kAlBlock;
    DevBuf dkey, dval, dskey, dsval, drcnt, droff, dpre, dtot, dpay, dppart, dkey2, dval2, dskey2, dsval2, dcost;
    DevBuf oindex, orow, ogroup, oadj, ocur, onew, ofair, olower, oupper;
    OB_HIP(dkey.alloc(sizeof(uint64_t) * m));
    OB_HIP(dval.alloc(sizeof(uint32_t) * m));
    OB_HIP(dskey.alloc(sizeof(uint64_t) * m));
    OB_HIP(dsval.alloc(sizeof(uint32_t) * m));
    OB_HIP(dpre.alloc(sizeof(double) * m));
    OB_HIP(dtot.alloc(sizeof(double) * tiles));
    OB_HIP(dpay.alloc(sizeof(double) * m));
    OB_HIP(dppart.alloc(sizeof(double) * tiles));
    OB_HIP(dkey2.alloc(sizeof(uint64_t) * m));
    OB_HIP(dval2.alloc(sizeof(uint32_t) * m));
    OB_HIP(dskey2.alloc(sizeof(uint64_t) * m));
    OB_HIP(dsval2.alloc(sizeof(uint32_t) * m));
    OB_HIP(dcost.alloc(sizeof(double)));
    OB_HIP(oindex.alloc(sizeof(int64_t) * m));
    OB_HIP(orow.alloc(sizeof(int64_t) * m));
    OB_HIP(ogroup.alloc(sizeof(int32_t) * m));
    for (DevBuf* b : {&oadj, &ocur, &onew, &ofair, &olower, &oupper}) OB_HIP(b->alloc(sizeof(double) * m));
    OB_HIP(drcnt.alloc(sizeof(uint32_t) * kRxBins * tiles));
    OB_HIP(droff.alloc(sizeof(uint32_t) * ((size_t)kRxBins * tiles + 1)));
    uint64_t *skey = nullptr, *skey2 = nullptr;
    uint32_t *sval = nullptr, *sval2 = nullptr;
    hipLaunchKernelGGL(ob_remedy_compact_kernel, dim3(blocks), dim3(kAlBlock), 0, st, ddiff.d(), dcls.as<uint8_t>(), n_push,
                       doffs.as<uint32_t>(), dkey.as<uint64_t>(), dval.as<uint32_t>());
    OB_HIP(hipGetLastError());
    OB_HIP(hipEventRecord(ev.e[1], st));
    // stable, descending: ties keep push order, all of B then all of A (analysis.rs:709-713)
    OB_TRY(remedy_radix_sort(st, dkey.as<uint64_t>(), dval.as<uint32_t>(), dskey.as<uint64_t>(), dsval.as<uint32_t>(), m, 64,
                             drcnt.as<uint32_t>(), droff.as<uint32_t>(), skey, sval));
    OB_HIP(hipEventRecord(ev.e[2], st));
    hipLaunchKernelGGL(ob_remedy_prefix_kernel, dim3(tiles), dim3(kAlBlock), 0, st, ddiff.d(), dcls.as<uint8_t>(),
                       sval, m, dpre.d(), dtot.d());
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_remedy_tiles_kernel, dim3(1), dim3(64), 0, st, dtot.d(), tiles);
    OB_HIP(hipGetLastError());
    PayArgs p = {};
    p.diff = ddiff.d();
    p.cls = dcls.as<uint8_t>();
    p.sval = sval;
    p.m = m;
    p.pre = dpre.d();
    p.tileoff = dtot.d();
    p.strategy = rq.strategy;
    p.budget = budget;
    p.ratio = need > 0.0 ? std::fmin(budget / need, 1.0) : 0.0;  // analysis.rs:790-794
    p.index = index ? dindex.as<int64_t>() : nullptr;
    p.n_a = n_a;
    p.n_b = n_b;
    p.pay = dpay.d();
    p.partial = dppart.d();
    p.key2 = dkey2.as<uint64_t>();
    p.val2 = dval2.as<uint32_t>();
    hipLaunchKernelGGL(ob_remedy_pay_kernel, dim3(tiles), dim3(kAlBlock), 0, st, p);
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(1), dim3(kSumBlock), 0, st, dppart.d(), tiles, dcost.d());
    OB_HIP(hipGetLastError());
    OB_TRY(remedy_radix_sort(st, dkey2.as<uint64_t>(), dval2.as<uint32_t>(), dskey2.as<uint64_t>(), dsval2.as<uint32_t>(), m,
                             index ? 64 : 32, drcnt.as<uint32_t>(), droff.as<uint32_t>(), skey2, sval2));  // analysis.rs:834
    GatherArgs g = {};
    g.skey2 = skey2;
    g.sval2 = sval2;
    g.sval = sval;
    g.m = m;
    g.pay = dpay.d();
    g.y = dy;
    g.fair = dfair;
    g.lower = dlower.d();
    g.upper = dupper.d();
    g.n_a = n_a;
    g.n_b = n_b;
    g.index = oindex.as<int64_t>();
    g.row = orow.as<int64_t>();
    g.group = ogroup.as<int32_t>();
    g.adjustment = oadj.d();
    g.current = ocur.d();
    g.new_wage = onew.d();
    g.fair_out = ofair.d();
    g.lower_out = olower.d();
    g.upper_out = oupper.d();
    hipLaunchKernelGGL(ob_remedy_gather_kernel, dim3(tiles), dim3(kAlBlock), 0, st, g);
    OB_HIP(hipGetLastError());
    OB_HIP(hipEventRecord(ev.e[3], st));
    out.index.resize(m);
    out.row.resize(m);
    out.group.resize(m);
    OB_HIP(hipMemcpyAsync(out.index.data(), oindex.p, sizeof(int64_t) * m, hipMemcpyDeviceToHost, st));
    OB_HIP(hipMemcpyAsync(out.row.data(), orow.p, sizeof(int64_t) * m, hipMemcpyDeviceToHost, st));
    OB_HIP(hipMemcpyAsync(out.group.data(), ogroup.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
    std::vector<double>* hv[6] = {&out.adjustment, &out.current_wage, &out.new_wage, &out.fair_wage, &out.lower, &out.upper};
    DevBuf* dv[6] = {&oadj, &ocur, &onew, &ofair, &olower, &oupper};
    for (int i = 0; i < 6; ++i) {
      hv[i]->resize(m);
      OB_HIP(hipMemcpyAsync(hv[i]->data(), dv[i]->p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    }
    OB_HIP(hipMemcpyAsync(&cost, dcost.p, sizeof(double), hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    info.classify_ms = ms;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
    info.order_ms = ms;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
    info.allocate_ms = ms;
  }
  info.total_cost = cost;
  // analysis.rs:847-857
  const double nt = (double)n_b;
  info.original_unexplained_gap = nt > 0.0 ? -net / nt : 0.0;
  info.new_unexplained_gap = nt > 0.0 ? -(net - cost) / nt : info.original_unexplained_gap;
  return OB_OK;
}

int remedy_defend_device(ob_ctx* ctx, const double* dy, const double* dfair, const double* dlev, int64_t n_a,
                         int64_t n_b, const int64_t* rows, const double* values, int64_t m64, double sigma2,
                         double confidence_level, ob_remedy_results& out) {
  const int64_t n = n_a + n_b;
  if (!ctx || (n > 0 && (!dy || !dfair || !dlev)) || (m64 > 0 && (!rows || !values))) return fail(OB_E_INVALID, "null pointer");
  if (m64 < 0 || m64 >= (int64_t)0x7fffffff || n >= (int64_t)0x7fffffff - 256) return fail(OB_E_UNSUPPORTED, "defend: too many rows or adjustments");
  const uint32_t m = (uint32_t)m64;
  out.defend = true;
  ob_defend_info& info = out.dinfo;
  info = ob_defend_info();
  info.n_a = n_a;
  info.n_b = n_b;
  info.n_adjustments = m;
  info.sigma_squared = sigma2;
  info.z_score = remedy_z_score(confidence_level);
  std::vector<uint32_t> row32(m);
  for (uint32_t j = 0; j < m; ++j) {
    if (rows[j] < 0 || rows[j] >= n) return fail(OB_E_INVALID, "adjustment %u names stacked row %lld outside [0, %lld)", j, (long long)rows[j], (long long)n);
    row32[j] = (uint32_t)rows[j];
  }
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events<4> ev;
  OB_HIP(ev.create());
  const uint32_t rblocks = (uint32_t)((n + kAlBlock - 1) / kAlBlock), ablocks = (m + kAlBlock - 1) / kAlBlock;
  DevBuf dfirst, drow, dval, dpart, dsum, dapart, ocur, onew, ofair, olower, oupper, oflag;
  OB_HIP(dfirst.alloc(sizeof(uint32_t) * (size_t)n));
  OB_HIP(drow.alloc(sizeof(uint32_t) * (size_t)m));
  OB_HIP(dval.alloc(sizeof(double) * (size_t)m));
  OB_HIP(dpart.alloc(sizeof(double) * (size_t)kDfSums * rblocks));
  OB_HIP(dapart.alloc(sizeof(double) * (size_t)ablocks));
  OB_HIP(dsum.alloc(sizeof(double) * (kDfSums + 1)));
  for (DevBuf* b : {&ocur, &onew, &ofair, &olower, &oupper}) OB_HIP(b->alloc(sizeof(double) * (size_t)m));
  OB_HIP(oflag.alloc(sizeof(int32_t) * (size_t)m));
  OB_HIP(hipMemsetAsync(dsum.p, 0, sizeof(double) * (kDfSums + 1), st));
  if (m > 0) {
    OB_HIP(hipMemcpyAsync(drow.p, row32.data(), sizeof(uint32_t) * (size_t)m, hipMemcpyHostToDevice, st));
    OB_HIP(hipMemcpyAsync(dval.p, values, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, st));
  }
  OB_HIP(hipEventRecord(ev.e[0], st));
  if (n > 0) OB_HIP(hipMemsetAsync(dfirst.p, 0xff, sizeof(uint32_t) * (size_t)n, st));  // no position
  if (m > 0) {
    hipLaunchKernelGGL(ob_defend_first_kernel, dim3(ablocks), dim3(kAlBlock), 0, st, drow.as<uint32_t>(), m, dfirst.as<uint32_t>());
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(ev.e[1], st));
  if (m > 0) {
    DefendAdjArgs a = {};
    a.y = dy;
    a.fair = dfair;
    a.lev = dlev;
    a.row = drow.as<uint32_t>();
    a.value = dval.d();
    a.m = m;
    a.sigma2 = sigma2;
    a.z = info.z_score;
    a.current = ocur.d();
    a.new_wage = onew.d();
    a.fair_out = ofair.d();
    a.lower = olower.d();
    a.upper = oupper.d();
    a.flag = oflag.as<int32_t>();
    a.partial = dapart.d();
    hipLaunchKernelGGL(ob_defend_adjust_kernel, dim3(ablocks), dim3(kAlBlock), 0, st, a);
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(1), dim3(kSumBlock), 0, st, dapart.d(), ablocks, dsum.d() + kDfSums);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(ev.e[2], st));
  if (n > 0) {
    DefendRowArgs r = {};
    r.y = dy;
    r.fair = dfair;
    r.first = dfirst.as<uint32_t>();
    r.value = dval.d();
    r.m = m;
    r.n_a = n_a;
    r.n = n;
    r.partial = dpart.d();
    r.blocks = rblocks;
    hipLaunchKernelGGL(ob_defend_rows_kernel, dim3(rblocks), dim3(kAlBlock), 0, st, r);
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(kDfSums), dim3(kSumBlock), 0, st, dpart.d(), rblocks, dsum.d());
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(ev.e[3], st));
  double s[kDfSums + 1] = {};
  OB_HIP(hipMemcpyAsync(s, dsum.p, sizeof(s), hipMemcpyDeviceToHost, st));
  std::vector<double>* hv[5] = {&out.current_wage, &out.new_wage, &out.fair_wage, &out.lower, &out.upper};
  DevBuf* dv[5] = {&ocur, &onew, &ofair, &olower, &oupper};
  for (int i = 0; i < 5; ++i) {
    hv[i]->resize(m);
    if (m > 0) OB_HIP(hipMemcpyAsync(hv[i]->data(), dv[i]->p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
  }
  out.defensible.resize(m);
  if (m > 0) OB_HIP(hipMemcpyAsync(out.defensible.data(), oflag.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));  // row32 and values are read by the copies above until here
  out.row.assign(rows, rows + m);
  out.index = out.row;
  out.adjustment.assign(values, values + m);
  out.group.resize(m);
  for (uint32_t j = 0; j < m; ++j) out.group[j] = rows[j] >= n_a ? 1 : 0;
  float ms = 0.f;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  info.scatter_ms = ms;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
  info.adjust_ms = ms;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
  info.rows_ms = ms;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[3]));
  info.defend_ms = ms;
  // defensibility.rs:316-365: a count of zero gives 0.0
  const double ca = (double)n_a, cb = (double)n_b;
  info.original_gap = (ca > 0.0 ? s[0] / ca : 0.0) - (cb > 0.0 ? s[2] / cb : 0.0);
  info.new_gap = (ca > 0.0 ? s[1] / ca : 0.0) - (cb > 0.0 ? s[3] / cb : 0.0);
  info.original_unexplained_gap = cb > 0.0 ? s[4] / cb : 0.0;
  info.new_unexplained_gap = cb > 0.0 ? s[5] / cb : 0.0;
  info.required_budget = s[6];
  info.total_cost = s[kDfSums];
  for (int q = 0; q < kDfSums; ++q) info.sums[q] = s[q];
  // what ob_remedy_results_info reports of a defensibility handle
  out.info = ob_remedy_info();
  out.info.n_a = n_a;
  out.info.n_b = n_b;
  out.info.n_adjustments = m;
  out.info.total_cost = info.total_cost;
  out.info.required_budget = info.required_budget;
  out.info.original_unexplained_gap = info.original_unexplained_gap;
  out.info.new_unexplained_gap = info.new_unexplained_gap;
  out.info.original_gap = info.original_gap;
  out.info.new_gap = info.new_gap;
  out.info.z_score = info.z_score;
  out.info.sigma_squared = sigma2;
  return OB_OK;
}

}  // namespace ob
