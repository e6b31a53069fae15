// ob_cluster.hip -- the device passes of the cluster bootstrap.
//
//   ob_cluster_gram_kernel    Q[c][g][e]: the extended Gram of cluster c's rows in group g, read from the
//                             raw panel through the cluster permutation. One wave per (cluster, group, 256
//                             pairs): a lane owns 4 pairs, the wave stages 16 rows at a time in its own LDS
//                             slice. Rows go in permuted order; every 256 rows the running piece is added to
//                             the total, so the bytes depend on the cluster's rows alone.
//   ob_cluster_counts_kernel  k[rep][c] (u32) from OBRC-1 (ob_spec.h): one thread per Philox call (4 draws);
//                             a block-wide LDS histogram per replicate while C fits, global atomics beyond.
//   ob_cluster_rows_kernel    the replicate's rows per group, sum_c k[rep][c] rows[c][g] (integers).
//   ob_cluster_apply_kernel   out[rep][n] = sum_c k[rep][c] Q[c][n] on v_mfma_f64_16x16x4_f64: a block owns
//                             64 replicates x 128 columns, wave w the 16 replicates w, with both operands
//                             staged in LDS 32 clusters at a time (the counts converted to f64 there). C is
//                             walked in cluster order in runs of kApSplit = 8192 (grid z); with more than one
//                             run the partial sums land in [run][rep][n] and ob_cluster_reduce_kernel adds them
//                             in run order. Nothing in a replicate's sum depends on the batch or on first_rep.
//   ob_cluster_guard_kernel   ok = 0 and a NaN row for a replicate in which a group has rows <= K (ols.rs:98-105).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ob_builder.hpp"
#include "ob_cluster.hpp"
#include "ob_device.hpp"
#include "ob_hip.hpp"
#include "ob_spec.h"

namespace {

typedef double ob_d4 __attribute__((ext_vector_type(4)));

// ---- Q ----------------------------------------------------------------------------------------------------
constexpr int kCgRows = 16;      // rows a wave stages per step
constexpr int kCgPiece = 256;    // rows per piece
constexpr int kCgPairs = 256;    // pairs per work item: 4 per lane

struct CgArgs {
  const double* cols[2];   // [x_1..x_p, y_1.., (w)] x ld per group (the panel's d_cols layout)
  int64_t ld[2];
  const uint32_t* perm[2];
  const uint32_t* off[2];
  int ngroups, k1, e, e_pad, n_ep, weighted, wcol;
  uint32_t n_clusters;
  double* q;        // [C][ngroups][e_pad]
  uint32_t* qrows;  // [C][ngroups]
};

__global__ __launch_bounds__(256) void ob_cluster_gram_kernel(const CgArgs a) {
  extern __shared__ __attribute__((aligned(16))) double cg_sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t item = (uint64_t)blockIdx.x * 4 + w;
  if (item >= (uint64_t)a.n_clusters * a.ngroups * a.n_ep) return;  // no block-wide barrier below
  const int ep = (int)(item % a.n_ep);
  const uint64_t cg = item / a.n_ep;
  const int g = (int)(cg % a.ngroups);
  const uint32_t c = (uint32_t)(cg / a.ngroups);
  double* vs = cg_sm + (size_t)w * kCgRows * a.k1;
  int pa[4], pb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // pair e -> (a, b), a <= b, a-major (ob_pair_index)
    int e = ep * kCgPairs + j * 64 + lane;
    if (e >= a.e) e = 0;  // a padding pair: computed as pair 0, stored as zero
    int r = 0;
    while (e >= a.k1 - r) {
      e -= a.k1 - r;
      ++r;
    }
    pa[j] = r;
    pb[j] = r + e;
  }
  const double* cols = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t r0 = a.off[g][c], r1 = a.off[g][c + 1];
  double tot[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t p0 = r0; p0 < r1; p0 += kCgPiece) {
    const uint32_t p1 = min(p0 + (uint32_t)kCgPiece, r1);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t s0 = p0; s0 < p1; s0 += kCgRows) {
      const int nr = (int)min((uint32_t)kCgRows, p1 - s0);
      ob_sync<true>();  // the previous step's reads are done
      for (int idx = lane; idx < nr * a.k1; idx += 64) {
        const int col = idx / nr, i = idx - col * nr;
        const size_t row = a.perm[g][s0 + i];
        double v = col == 0 ? 1.0 : cols[(size_t)(col - 1) * ld + row];
        if (a.weighted) v *= sqrt(cols[(size_t)a.wcol * ld + row]);  // sqrt(w) [1, x, y] (ols.rs:68-78)
        vs[i * a.k1 + col] = v;
      }
      ob_sync<true>();
      for (int i = 0; i < nr; ++i) {
        const double* v = vs + i * a.k1;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fma(v[pa[j]], v[pb[j]], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) tot[j] += acc[j];
  }
  double* q = a.q + ((size_t)c * a.ngroups + g) * a.e_pad;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = ep * kCgPairs + j * 64 + lane;
    if (e < a.e_pad) q[e] = e < a.e ? tot[j] : 0.0;
  }
  if (ep == 0 && lane == 0) a.qrows[(size_t)c * a.ngroups + g] = r1 - r0;
}

// ---- counts -----------------------------------------------------------------------------------------------
constexpr uint32_t kCcLdsMax = 12288;  // clusters whose u32 histogram fits one block's LDS (48 KB)

struct CcArgs {
  uint32_t m0, m1, base1, n_clusters;  // draws of stratum 0 / 1, stratum 1's first cluster
  uint32_t first_rep, key0, key1;
  uint32_t* counts;  // [rep][C]
};

__device__ __forceinline__ void cc_call(const CcArgs& a, uint32_t q, uint32_t s, uint32_t rep, uint32_t* hist) {
  const uint32_t m = s ? a.m1 : a.m0;
  const ob_u32x4 u0 = ob_philox(q, rep, s, OB_TAG_OBC, a.key0, a.key1);
  for (uint32_t h = 0; h < 4; ++h) {
    const uint32_t j = 4 * q + h;
    if (j < m) atomicAdd(&hist[ob_cluster_draw(u0, j, rep, s, m, a.key0, a.key1) + (s ? a.base1 : 0u)], 1u);
  }
}

template <bool LDS>
__global__ __launch_bounds__(256) void ob_cluster_counts_kernel(const CcArgs a) {
  extern __shared__ uint32_t cc_hist[];
  const uint32_t r = LDS ? blockIdx.x : blockIdx.y;
  const uint32_t rep = a.first_rep + r;
  const uint32_t calls0 = (a.m0 + 3) / 4, calls1 = (a.m1 + 3) / 4;
  uint32_t* out = a.counts + (size_t)r * a.n_clusters;
  if constexpr (LDS) {
    for (uint32_t c = threadIdx.x; c < a.n_clusters; c += 256) cc_hist[c] = 0;
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < calls0 + calls1; q += 256)
      cc_call(a, q < calls0 ? q : q - calls0, q < calls0 ? 0u : 1u, rep, cc_hist);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < a.n_clusters; c += 256) out[c] = cc_hist[c];
  } else {  // the launch zeroed counts
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q < calls0 + calls1) cc_call(a, q < calls0 ? q : q - calls0, q < calls0 ? 0u : 1u, rep, out);
  }
}

// rows[rep][g] = sum_c k[rep][c] qrows[c][g]: one wave per replicate, integer sums (any order).
__global__ __launch_bounds__(256) void ob_cluster_rows_kernel(const uint32_t* counts, const uint32_t* qrows,
                                                              uint32_t n_clusters, uint32_t n_reps, uint32_t* rows) {
  const int lane = threadIdx.x & 63;
  const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_reps) return;
  unsigned long long sa = 0, sb = 0;
  for (uint32_t c = lane; c < n_clusters; c += 64) {
    const unsigned long long k = counts[(size_t)r * n_clusters + c];
    sa += k * qrows[2 * (size_t)c];
    sb += k * qrows[2 * (size_t)c + 1];
  }
  for (int off = 32; off > 0; off >>= 1) {
    sa += __shfl_xor(sa, off);
    sb += __shfl_xor(sb, off);
  }
  if (lane == 0) {
    rows[2 * (size_t)r] = (uint32_t)min(sa, 0xFFFFFFFFull);
    rows[2 * (size_t)r + 1] = (uint32_t)min(sb, 0xFFFFFFFFull);
  }
}

// ---- counts x Q ---------------------------------------------------------------------------------------------
constexpr int kApM = 64, kApN = 128, kApK = 32;
constexpr int kApAs = 80;    // doubles per staged A row (64 replicates + 16: rows 128 bytes apart in the banks)
constexpr int kApBs = 144;   // doubles per staged B row (128 columns + 16)
constexpr uint32_t kApSplit = 8192;  // clusters per run: the split points depend on C alone

struct CaArgs {
  const uint32_t* counts;  // [rep][C]
  const double* q;         // [C][width]
  double* out;             // [rep][width], or [run][n_reps][width] with more than one run
  uint32_t n_reps, n_clusters;
  int width;
};

__global__ __launch_bounds__(256) void ob_cluster_apply_kernel(const CaArgs a) {
  __shared__ __attribute__((aligned(16))) double As[kApK * kApAs];
  __shared__ __attribute__((aligned(16))) double Bs[kApK * kApBs];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, kq = lane >> 4;
  const uint32_t rep0 = blockIdx.y * kApM;
  const int n0 = blockIdx.x * kApN;
  const uint32_t c_beg = blockIdx.z * kApSplit, c_end = min(a.n_clusters, c_beg + kApSplit);
  ob_d4 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = ob_d4{0.0, 0.0, 0.0, 0.0};
  for (uint32_t c0 = c_beg; c0 < c_end; c0 += kApK) {
#pragma unroll
    for (int i = 0; i < kApM * kApK / 256; ++i) {  // A: 64 replicates x 32 clusters, 128-byte runs of a replicate
      const int idx = i * 256 + tid, m = idx >> 5, kk = idx & 31;
      const uint32_t rep = rep0 + m, c = c0 + kk;
      const uint32_t v = (rep < a.n_reps && c < c_end) ? a.counts[(size_t)rep * a.n_clusters + c] : 0u;
      As[kk * kApAs + m] = (double)v;
    }
#pragma unroll
    for (int i = 0; i < kApK * kApN / 256; ++i) {  // B: 32 clusters x 128 columns
      const int idx = i * 256 + tid, kk = idx >> 7, n = idx & 127;
      const uint32_t c = c0 + kk;
      const int col = n0 + n;
      Bs[kk * kApBs + n] = (c < c_end && col < a.width) ? a.q[(size_t)c * a.width + col] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kApK / 4; ++ks) {
      const double av = As[(ks * 4 + kq) * kApAs + w * 16 + li];
      const double* brow = Bs + (ks * 4 + kq) * kApBs + li;
#pragma unroll
      for (int t = 0; t < 8; ++t)
        if (n0 + t * 16 < a.width) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[t * 16], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  // D[i][j] sits in lane (i % 4) * 16 + j, element i / 4 (the layout ob_vif.hip reads)
  double* out = a.out + (size_t)blockIdx.z * a.n_reps * a.width;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int col = n0 + t * 16 + li;
    if (col >= a.width) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t rep = rep0 + w * 16 + 4 * r + kq;
      if (rep < a.n_reps) out[(size_t)rep * a.width + col] = acc[t][r];
    }
  }
}

// out[i] = partial[0][i] + partial[1][i] + ... in run order.
__global__ __launch_bounds__(256) void ob_cluster_reduce_kernel(const double* partial, uint32_t nsplit, size_t n,
                                                                double* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = partial[i];
  for (uint32_t z = 1; z < nsplit; ++z) s += partial[(size_t)z * n + i];
  out[i] = s;
}

__global__ __launch_bounds__(256) void ob_cluster_guard_kernel(const uint32_t* rep_rows, uint32_t k, uint32_t ns,
                                                               int n_y, uint64_t n_reps, uint64_t s0, int row_len,
                                                               double* rows, uint8_t* ok) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ns * (uint32_t)n_y) return;
  const uint32_t r = i % ns, t = i / ns;
  if (rep_rows[2 * (size_t)r] > k && rep_rows[2 * (size_t)r + 1] > k) return;
  const size_t at = (size_t)t * n_reps + s0 + r;
  ok[at] = 0;
  for (int j = 0; j < row_len; ++j) rows[at * row_len + j] = __builtin_nan("");
}

// ---- launches ---------------------------------------------------------------------------------------------
uint32_t apply_runs(uint32_t n_clusters) { return (n_clusters + kApSplit - 1) / kApSplit; }

int launch_gram(const CgArgs& a, hipStream_t s) {
  const size_t lds = sizeof(double) * 4 * kCgRows * a.k1;
  const uint64_t items = (uint64_t)a.n_clusters * a.ngroups * a.n_ep;
  const uint64_t blocks = (items + 3) / 4;
  if (blocks > 0x7FFFFFFFull) return ob::fail(OB_E_UNSUPPORTED, "cluster bootstrap: too many cluster work items");
  hipLaunchKernelGGL(ob_cluster_gram_kernel, dim3((unsigned)blocks), dim3(256), lds, s, a);
  OB_HIP(hipGetLastError());
  return OB_OK;
}

int launch_counts(const CcArgs& a, uint32_t n_reps, hipStream_t s) {
  if (a.n_clusters <= kCcLdsMax) {
    hipLaunchKernelGGL(ob_cluster_counts_kernel<true>, dim3(n_reps), dim3(256), sizeof(uint32_t) * a.n_clusters, s, a);
  } else {
    OB_HIP(hipMemsetAsync(a.counts, 0, sizeof(uint32_t) * (size_t)n_reps * a.n_clusters, s));
    const uint32_t calls = (a.m0 + 3) / 4 + (a.m1 + 3) / 4;
    hipLaunchKernelGGL(ob_cluster_counts_kernel<false>, dim3((calls + 255) / 256, n_reps), dim3(256), 0, s, a);
  }
  OB_HIP(hipGetLastError());
  return OB_OK;
}

// out [n_reps][width]; partial: [runs][n_reps][width] when apply_runs(C) > 1 (else unused).
int launch_apply(const uint32_t* counts, const double* q, uint32_t n_reps, uint32_t n_clusters, int width,
                 double* partial, double* out, hipStream_t s) {
  const uint32_t runs = apply_runs(n_clusters);
  CaArgs a{counts, q, runs > 1 ? partial : out, n_reps, n_clusters, width};
  const dim3 grid((unsigned)((width + kApN - 1) / kApN), (n_reps + kApM - 1) / kApM, runs);
  hipLaunchKernelGGL(ob_cluster_apply_kernel, grid, dim3(256), 0, s, a);
  OB_HIP(hipGetLastError());
  if (runs > 1) {
    const size_t n = (size_t)n_reps * width;
    hipLaunchKernelGGL(ob_cluster_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       (const double*)partial, runs, n, out);
    OB_HIP(hipGetLastError());
  }
  return OB_OK;
}

thread_local ob_cluster_timing g_timing = {};

}  // namespace

namespace ob {

constexpr uint64_t kClBatchBudget = (uint64_t)1 << 30;  // bytes of counts + partial sums + Grams per batch
constexpr uint64_t kClBatchMax = 16384;

struct ClusterState {
  ob_cluster_info info = {};
  uint32_t n_clusters = 0, m0 = 0, m1 = 0, base1 = 0;
  DevBuf perm[2], off[2], q, qrows;
  bool q_ready = false;
  DevBuf counts, partial, gram, rep_rows, rows_tmp, ok_tmp;
  Events<6> ev;  // Q start / end, then a batch's counts start, counts end, apply end, solve end
  bool ev_ready = false;
};

void cluster_free(ClusterState* s) { delete s; }

void cluster_info(const ClusterState* s, ob_cluster_info* out) { *out = s->info; }

int cluster_attach(ob_prepared* pr, const ClusterIndex& idx) {
  ob_panel* p = pr->panel;
  if ((int64_t)idx.perm[0].size() != (int64_t)p->n[0] || (int64_t)idx.perm[1].size() != (int64_t)p->n[1])
    return fail(OB_E_INVALID, "internal: the cluster index does not cover the panel's rows");
  OB_HIP(hipSetDevice(p->ctx->device));
  ClusterState* cs = new ClusterState();
  pr->cluster = cs;  // freed with the handle, also on the errors below
  cs->info = {idx.n_clusters, idx.c_a, idx.c_b, idx.max_rows, idx.stratified};
  cs->n_clusters = (uint32_t)idx.n_clusters;
  cs->m0 = idx.stratified ? (uint32_t)idx.c_a : (uint32_t)idx.n_clusters;
  cs->m1 = idx.stratified ? (uint32_t)idx.c_b : 0u;
  cs->base1 = (uint32_t)idx.c_a;
  std::vector<uint32_t> tmp;
  for (int g = 0; g < 2; ++g) {
    tmp.assign(idx.perm[g].begin(), idx.perm[g].end());
    OB_HIP(cs->perm[g].alloc(sizeof(uint32_t) * tmp.size()));
    OB_HIP(hipMemcpy(cs->perm[g].p, tmp.data(), sizeof(uint32_t) * tmp.size(), hipMemcpyHostToDevice));
    tmp.assign(idx.off[g].begin(), idx.off[g].end());
    OB_HIP(cs->off[g].alloc(sizeof(uint32_t) * tmp.size()));
    OB_HIP(hipMemcpy(cs->off[g].p, tmp.data(), sizeof(uint32_t) * tmp.size(), hipMemcpyHostToDevice));
  }
  OB_HIP(cs->q.alloc(sizeof(double) * (size_t)cs->n_clusters * 2 * p->e_pad));
  OB_HIP(cs->qrows.alloc(sizeof(uint32_t) * (size_t)cs->n_clusters * 2));
  return OB_OK;
}

// Q and the clusters' row counts: one pass over the panel, the first time a clustered handle needs them.
static int cluster_ensure_q(ob_prepared* pr, hipStream_t s, bool timed, ob_cluster_timing& tm) {
  ob_panel* p = pr->panel;
  ClusterState* cs = pr->cluster;
  const uint32_t nc = cs->n_clusters;
  if (!cs->q_ready) {
    CgArgs ga{};
    for (int g = 0; g < 2; ++g) {
      ga.cols[g] = p->d_cols[g];
      ga.ld[g] = p->ld[g];
      ga.perm[g] = cs->perm[g].as<uint32_t>();
      ga.off[g] = cs->off[g].as<uint32_t>();
    }
    ga.ngroups = 2;
    ga.k1 = p->k1;
    ga.e = p->e;
    ga.e_pad = p->e_pad;
    ga.n_ep = (p->e_pad + kCgPairs - 1) / kCgPairs;
    ga.weighted = p->weighted;
    ga.wcol = p->p + p->n_y;
    ga.n_clusters = nc;
    ga.q = cs->q.d();
    ga.qrows = cs->qrows.as<uint32_t>();
    if (timed) OB_HIP(hipEventRecord(cs->ev.e[0], s));
    OB_TRY(launch_gram(ga, s));
    if (timed) {
      OB_HIP(hipEventRecord(cs->ev.e[1], s));
      OB_HIP(hipEventSynchronize(cs->ev.e[1]));
      float t = 0.f;
      OB_HIP(hipEventElapsedTime(&t, cs->ev.e[0], cs->ev.e[1]));
      tm.gram_ms = t;
    }
    cs->q_ready = true;
  }
  return OB_OK;
}

static int cluster_boot(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                        hipStream_t stream, bool timed) {
  ob_panel* p = pr->panel;
  ClusterState* cs = pr->cluster;
  if (n_reps == 0) return OB_OK;
  if (first_rep + n_reps > 0x100000000ull)
    return fail(OB_E_INVALID, "replicate ids must stay below 2^32 (OBRC-1 counter word)");
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = stream ? stream : p->ctx->stream;
  OB_TRY(engine_order(p, s));
  if (!p->timing_pending) std::memset(&p->timing, 0, sizeof(p->timing));
  if (timed && !cs->ev_ready) {
    OB_HIP(cs->ev.create());
    cs->ev_ready = true;
  }
  const uint32_t nc = cs->n_clusters, runs = apply_runs(nc);
  const int width = 2 * p->e_pad;
  ob_cluster_timing tm = {};
  OB_TRY(cluster_ensure_q(pr, s, timed, tm));
  // batch: counts, partial sums and Grams within kClBatchBudget, so a run of any length needs bounded memory
  const uint64_t per_rep = (uint64_t)nc * 4 + (uint64_t)width * 8 * (runs > 1 ? runs + 1 : 1) + 8;
  const uint64_t batch = std::min<uint64_t>(std::min(n_reps, kClBatchMax),
                                            std::max<uint64_t>(16, kClBatchBudget / per_rep / 16 * 16));
  OB_HIP(cs->counts.alloc(sizeof(uint32_t) * batch * nc));
  OB_HIP(cs->gram.alloc(sizeof(double) * batch * width));
  OB_HIP(cs->rep_rows.alloc(sizeof(uint32_t) * batch * 2));
  if (runs > 1) OB_HIP(cs->partial.alloc(sizeof(double) * batch * width * runs));
  CcArgs ca{cs->m0, cs->m1, cs->base1, nc, 0u, (uint32_t)pr->seed, (uint32_t)(pr->seed >> 32),
            cs->counts.as<uint32_t>()};
  for (uint64_t s0 = 0; s0 < n_reps; s0 += batch) {
    const uint32_t ns = (uint32_t)std::min<uint64_t>(batch, n_reps - s0);
    ca.first_rep = (uint32_t)(first_rep + s0);
    if (timed) OB_HIP(hipEventRecord(cs->ev.e[2], s));
    OB_TRY(launch_counts(ca, ns, s));
    hipLaunchKernelGGL(ob_cluster_rows_kernel, dim3((ns + 3) / 4), dim3(256), 0, s, cs->counts.as<uint32_t>(),
                       cs->qrows.as<uint32_t>(), nc, ns, cs->rep_rows.as<uint32_t>());
    OB_HIP(hipGetLastError());
    if (timed) OB_HIP(hipEventRecord(cs->ev.e[3], s));
    OB_TRY(launch_apply(cs->counts.as<uint32_t>(), cs->q.d(), ns, nc, width, cs->partial.d(), cs->gram.d(), s));
    if (timed) OB_HIP(hipEventRecord(cs->ev.e[4], s));
    OB_TRY(engine_solve_grams(p, cs->gram.d(), cs->rep_rows.as<uint32_t>(), ns, n_reps, s0, pr->ref, d_rows, d_ok, s));
    hipLaunchKernelGGL(ob_cluster_guard_kernel, dim3((ns * (uint32_t)p->n_y + 255) / 256), dim3(256), 0, s,
                       cs->rep_rows.as<uint32_t>(), (uint32_t)p->k, ns, p->n_y, n_reps, s0, p->row_len, d_rows, d_ok);
    OB_HIP(hipGetLastError());
    if (timed) {  // a host boot: its batches are timed one by one (the events are reused)
      OB_HIP(hipEventRecord(cs->ev.e[5], s));
      OB_HIP(hipEventSynchronize(cs->ev.e[5]));
      float t[3] = {0.f, 0.f, 0.f};
      for (int i = 0; i < 3; ++i) OB_HIP(hipEventElapsedTime(&t[i], cs->ev.e[2 + i], cs->ev.e[3 + i]));
      tm.counts_ms += t[0];
      tm.apply_ms += t[1];
      tm.solve_ms += t[2];
    }
  }
  if (timed) g_timing = tm;
  p->timing_pending = true;  // ob_panel_sync waits for this stream
  p->last_stream = s;
  return engine_mark(p, s);
}

int cluster_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                        hipStream_t stream) {
  if (n_reps && (!d_rows || !d_ok)) return fail(OB_E_INVALID, "null pointer");
  return cluster_boot(pr, first_rep, n_reps, d_rows, d_ok, stream, false);
}

static int hook_index(const Col& ids, const int32_t* group, int64_t n_rows, bool stratified, int k1, ClusterIndex& out) {
  OB_TRY(cluster_index(ids, group, n_rows, stratified, out));
  return cluster_check_shape(out.n_clusters, k1);
}

int cluster_boot_host(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* rows, uint8_t* ok) {
  if (n_reps && (!rows || !ok)) return fail(OB_E_INVALID, "null pointer");
  if (n_reps == 0) return OB_OK;
  if (first_rep + n_reps > 0x100000000ull)
    return fail(OB_E_INVALID, "replicate ids must stay below 2^32 (OBRC-1 counter word)");
  ob_panel* p = pr->panel;
  ClusterState* cs = pr->cluster;
  OB_HIP(hipSetDevice(p->ctx->device));
  const size_t nrow = (size_t)n_reps * p->n_y;
  OB_HIP(cs->rows_tmp.alloc(sizeof(double) * nrow * p->row_len));
  OB_HIP(cs->ok_tmp.alloc(nrow));
  OB_TRY(cluster_boot(pr, first_rep, n_reps, cs->rows_tmp.d(), cs->ok_tmp.as<uint8_t>(), nullptr, true));
  OB_TRY(engine_collect(p));
  OB_HIP(hipMemcpy(rows, cs->rows_tmp.p, sizeof(double) * nrow * p->row_len, hipMemcpyDeviceToHost));
  OB_HIP(hipMemcpy(ok, cs->ok_tmp.p, nrow, hipMemcpyDeviceToHost));
  return OB_OK;
}

// ---- what the delete-one-cluster jackknife reads of a clustered handle (ob_cluster_jack.hip) -------------------
int cluster_view(ob_prepared* pr, hipStream_t s, ClusterView& out) {
  ClusterState* cs = pr->cluster;
  ob_cluster_timing tm = {};
  OB_TRY(cluster_ensure_q(pr, s, false, tm));
  out.q = cs->q.d();
  out.qrows = cs->qrows.as<uint32_t>();
  out.n_clusters = cs->n_clusters;
  out.n_clusters_a = (uint32_t)cs->info.n_clusters_a;
  out.stratified = cs->info.stratified;
  return OB_OK;
}

int cluster_sum_q(const double* d_q, uint32_t nc, int width, double* d_total, hipStream_t s) {
  const std::vector<uint32_t> ones(nc, 1u);  // every cluster once: ob_cluster_apply's sum, one replicate wide
  DevBuf counts, partial;
  OB_HIP(counts.alloc(sizeof(uint32_t) * nc));
  OB_HIP(hipMemcpyAsync(counts.p, ones.data(), sizeof(uint32_t) * nc, hipMemcpyHostToDevice, s));
  if (apply_runs(nc) > 1) OB_HIP(partial.alloc(sizeof(double) * width * apply_runs(nc)));
  OB_TRY(launch_apply(counts.as<uint32_t>(), d_q, 1, nc, width, partial.d(), d_total, s));
  OB_HIP(hipStreamSynchronize(s));  // `ones` and the buffers are in use until here
  return OB_OK;
}

int cluster_guard(const ob_panel* p, const uint32_t* d_rep_rows, uint32_t ns, uint64_t n_reps, uint64_t s0, double* d_rows,
                  uint8_t* d_ok, hipStream_t s) {
  hipLaunchKernelGGL(ob_cluster_guard_kernel, dim3((ns * (uint32_t)p->n_y + 255) / 256), dim3(256), 0, s, d_rep_rows,
                     (uint32_t)p->k, ns, p->n_y, n_reps, s0, p->row_len, d_rows, d_ok);
  OB_HIP(hipGetLastError());
  return OB_OK;
}

// installs the builder's hooks when the library loads (ob_cluster.hpp)
static const bool g_hooks_installed = [] {
  ClusterHooks& h = cluster_hooks();
  h.index = hook_index;
  h.attach = cluster_attach;
  h.free_state = cluster_free;
  h.info = cluster_info;
  h.boot_device = cluster_boot_device;
  h.boot_host = cluster_boot_host;
  return true;
}();

}  // namespace ob

// ---- the array-level entry points ---------------------------------------------------------------------------
extern "C" {

int ob_cluster_gram(ob_ctx* ctx, const double* x, int64_t n, int64_t ldx, int32_t p, const double* y, const double* w,
                    const int64_t* perm, const int64_t* off, int64_t n_clusters, double* q, uint32_t* rows) {
  if (!ctx || !y || !perm || !off || !q || !rows || (p > 0 && !x)) return ob::fail(OB_E_INVALID, "null pointer");
  if (p < 0 || p > 120) return ob::fail(OB_E_UNSUPPORTED, "predictor columns must be in [0, 120], got %d", p);
  if (n < 1 || n > ((int64_t)1 << 28) || ldx < n) return ob::fail(OB_E_INVALID, "bad row count or ldx");
  if (n_clusters < 1 || n_clusters >= ob::kClusterMax) return ob::fail(OB_E_INVALID, "bad cluster count");
  if (off[0] != 0 || off[n_clusters] != n) return ob::fail(OB_E_INVALID, "offsets must run from 0 to n");
  for (int64_t c = 0; c < n_clusters; ++c)
    if (off[c + 1] < off[c]) return ob::fail(OB_E_INVALID, "offsets must not decrease");
  for (int64_t i = 0; i < n; ++i)
    if (perm[i] < 0 || perm[i] >= n) return ob::fail(OB_E_INVALID, "permutation entry %lld out of range", (long long)i);
  const int k1 = p + 2, e = k1 * (k1 + 1) / 2, e_pad = (e + 15) / 16 * 16;
  OB_HIP(hipSetDevice(ctx->device));
  const int ncols = p + 1 + (w ? 1 : 0);
  DevBuf dcols, dperm, doff, dq, drows;
  OB_HIP(dcols.alloc(sizeof(double) * (size_t)ncols * n));
  if (p > 0)
    OB_HIP(hipMemcpy2D(dcols.p, sizeof(double) * n, x, sizeof(double) * ldx, sizeof(double) * n, p, hipMemcpyHostToDevice));
  OB_HIP(hipMemcpy(dcols.d() + (size_t)p * n, y, sizeof(double) * n, hipMemcpyHostToDevice));
  if (w) OB_HIP(hipMemcpy(dcols.d() + (size_t)(p + 1) * n, w, sizeof(double) * n, hipMemcpyHostToDevice));
  std::vector<uint32_t> tmp(perm, perm + n);
  OB_HIP(dperm.alloc(sizeof(uint32_t) * n));
  OB_HIP(hipMemcpy(dperm.p, tmp.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  tmp.assign(off, off + n_clusters + 1);
  OB_HIP(doff.alloc(sizeof(uint32_t) * tmp.size()));
  OB_HIP(hipMemcpy(doff.p, tmp.data(), sizeof(uint32_t) * tmp.size(), hipMemcpyHostToDevice));
  OB_HIP(dq.alloc(sizeof(double) * (size_t)n_clusters * e_pad));
  OB_HIP(drows.alloc(sizeof(uint32_t) * n_clusters));
  CgArgs a{};
  a.cols[0] = dcols.d();
  a.ld[0] = n;
  a.perm[0] = dperm.as<uint32_t>();
  a.off[0] = doff.as<uint32_t>();
  a.ngroups = 1;
  a.k1 = k1;
  a.e = e;
  a.e_pad = e_pad;
  a.n_ep = (e_pad + kCgPairs - 1) / kCgPairs;
  a.weighted = w ? 1 : 0;
  a.wcol = p + 1;
  a.n_clusters = (uint32_t)n_clusters;
  a.q = dq.d();
  a.qrows = drows.as<uint32_t>();
  OB_TRY(launch_gram(a, ctx->stream));
  OB_HIP(hipStreamSynchronize(ctx->stream));
  OB_HIP(hipMemcpy(q, dq.p, sizeof(double) * (size_t)n_clusters * e_pad, hipMemcpyDeviceToHost));
  OB_HIP(hipMemcpy(rows, drows.p, sizeof(uint32_t) * n_clusters, hipMemcpyDeviceToHost));
  return OB_OK;
}

int ob_cluster_counts(ob_ctx* ctx, uint64_t seed, uint64_t first_rep, uint32_t n_reps, int64_t n_clusters_a,
                      int64_t n_clusters_b, int32_t stratified, uint32_t* counts) {
  if (!ctx || !counts) return ob::fail(OB_E_INVALID, "null pointer");
  const int64_t nc = n_clusters_a + n_clusters_b;
  if (n_clusters_a < 0 || n_clusters_b < 0 || nc < 1 || nc >= ob::kClusterMax)
    return ob::fail(OB_E_INVALID, "bad cluster counts");
  if (n_reps == 0) return OB_OK;
  if (first_rep + n_reps > 0x100000000ull)
    return ob::fail(OB_E_INVALID, "replicate ids must stay below 2^32 (OBRC-1 counter word)");
  if ((uint64_t)n_reps * (uint64_t)nc > ((uint64_t)1 << 30)) return ob::fail(OB_E_UNSUPPORTED, "counts above 4 GiB");
  OB_HIP(hipSetDevice(ctx->device));
  DevBuf d;
  OB_HIP(d.alloc(sizeof(uint32_t) * (size_t)n_reps * nc));
  CcArgs a{stratified ? (uint32_t)n_clusters_a : (uint32_t)nc, stratified ? (uint32_t)n_clusters_b : 0u,
           (uint32_t)n_clusters_a, (uint32_t)nc, (uint32_t)first_rep, (uint32_t)seed, (uint32_t)(seed >> 32),
           d.as<uint32_t>()};
  OB_TRY(launch_counts(a, n_reps, ctx->stream));
  OB_HIP(hipStreamSynchronize(ctx->stream));
  OB_HIP(hipMemcpy(counts, d.p, sizeof(uint32_t) * (size_t)n_reps * nc, hipMemcpyDeviceToHost));
  return OB_OK;
}

int ob_cluster_apply(ob_ctx* ctx, const uint32_t* counts, uint32_t n_reps, int64_t n_clusters, const double* q,
                     int32_t width, double* out) {
  if (!ctx || !counts || !q || !out) return ob::fail(OB_E_INVALID, "null pointer");
  if (n_clusters < 1 || n_clusters >= ob::kClusterMax) return ob::fail(OB_E_INVALID, "bad cluster count");
  if (width < 16 || width % 16 != 0 || width > 2 * 7504) return ob::fail(OB_E_INVALID, "width must be a multiple of 16");
  if (n_reps == 0) return OB_OK;
  const uint32_t runs = apply_runs((uint32_t)n_clusters);
  if ((uint64_t)n_reps * (uint64_t)n_clusters > ((uint64_t)1 << 30) ||
      (uint64_t)n_reps * (uint64_t)width * (runs + 1) > ((uint64_t)1 << 29))
    return ob::fail(OB_E_UNSUPPORTED, "arrays above 4 GiB");
  OB_HIP(hipSetDevice(ctx->device));
  DevBuf dc, dq, dout, dpart;
  OB_HIP(dc.alloc(sizeof(uint32_t) * (size_t)n_reps * n_clusters));
  OB_HIP(dq.alloc(sizeof(double) * (size_t)n_clusters * width));
  OB_HIP(dout.alloc(sizeof(double) * (size_t)n_reps * width));
  if (runs > 1) OB_HIP(dpart.alloc(sizeof(double) * (size_t)n_reps * width * runs));
  OB_HIP(hipMemcpy(dc.p, counts, sizeof(uint32_t) * (size_t)n_reps * n_clusters, hipMemcpyHostToDevice));
  OB_HIP(hipMemcpy(dq.p, q, sizeof(double) * (size_t)n_clusters * width, hipMemcpyHostToDevice));
  OB_TRY(launch_apply(dc.as<uint32_t>(), dq.d(), n_reps, (uint32_t)n_clusters, width, dpart.d(), dout.d(), ctx->stream));
  OB_HIP(hipStreamSynchronize(ctx->stream));
  OB_HIP(hipMemcpy(out, dout.p, sizeof(double) * (size_t)n_reps * width, hipMemcpyDeviceToHost));
  return OB_OK;
}

int ob_cluster_last_timing(ob_cluster_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

}  // extern "C"
