// ob_jackknife.hip -- the leave-one-out pass behind the BCa interval. The reference has
// no counterpart: its intervals are the floor-index percentiles of inference.rs:21-31. Deleting row i of
// group g and refitting is, by Sherman-Morrison on the group's Gram G_g = sum w x x',
//
//   t_i = G_g^-1 x_i,  h_i = w_i x_i't_i,  e_i = y_i - x_i'beta_g,  beta_g(i) = beta_g - t_i w_i e_i / (1 - h_i)
//
// with the means of the rows that stay, (S_g - w_i x_i) / (W_g - w_i), and for Pooled / Neumark the same
// update of the pooled fit on z_i = [x_i, 1[g = A]] (builder.rs:547-590). From these the C = 6 + 2K
// components of decomposition.rs:56-122 follow in O(K) per row, the other group staying at its point
// estimate; the algebra is ob_solve_kernel's (ob_engine.hip), restated here for a lane that owns a
// coefficient of four rows instead of a wave that owns a replicate.
//
//   ob_jackknife_kernel<NJB, ROWS>  the shape of ob_remedy_score_kernel: B' = [G_g^-1 | beta_g] stays in LDS
//     for the whole block (a block serves one group), X streams through registers in the A-operand shape
//     of v_mfma_f64_16x16x4_f64, a wave owns a run of 16-row blocks and feeds NJB column-block accumulators;
//     for Pooled a second product with B'_P = [P^-1 (design columns, then the indicator's) | beta_P], which
//     shares LDS when both fit and is read through the cache otherwise. The epilogue reads the 16 x K tile
//     of x again in the accumulator's shape (rows kq + 4 r, column 16 jb + li).
//       ROWS = false (sums): per wave, the power sums of d = theta_(i) - theta_hat over its kept rows go to
//         the wave's own slot; ob_ordered_sum_kernel adds the slots in a fixed order. Nothing n x C is stored.
//         d is formed from the changes themselves (jack_delta), never as a difference of two theta.
//       ROWS = true: theta_(i) of every row and a kept byte, for tests and small panels.
//
// No floating atomics: two calls on the same panel return the same bytes. The kept and
// dropped counts are integer atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ob_device.hpp"
#include "ob_hip.hpp"
#include "ob_jackknife.hpp"
#include "ob_linalg.hpp"

namespace {

typedef double ob_d4 __attribute__((ext_vector_type(4)));

constexpr int kJkBlock = 256;
constexpr int kJkWaves = kJkBlock / 64;
constexpr int kJkMaxJb = 8;           // 16-column blocks of the K + 2 columns of B'_P
constexpr int kJkUnitsPerGroup = 1024;  // waves (units) a group's rows are dealt over, at most
constexpr int kJkCst = 7;             // per-column constants: beta_A, beta_B, S_A, S_B, xbar_A, xbar_B, beta_P
constexpr int kJkPad = 128;           // their stride
constexpr size_t kJkLds = 160 * 1024;
#define OB_JACK_TINY 0x1p-40  // 1 - h at or below this: the fit without the row has no solution

struct JackArgs {
  const double* cols[2];  // the panel's columns: x_1..x_p, y, (w), each ld entries
  int64_t ld[2];
  int64_t n[2];
  int p, k, weighted, ref, pooled;
  int ns, nsp, ldb;       // steps of 4 design columns (group, pooled); leading dimension of every B'
  const double* bg[2];    // device, row-major [4 ns][ldb]: row c = [G_g^-1[c][0..k), beta_g[c]], zero outside
  const double* bpool;    // device, row-major [4 nsp][ldb]: row c (design order, the indicator as row k) =
                          // [P^-1[c][0..k), P^-1[c][indicator], beta_P[c]], zero outside
  int pool_lds;           // the pooled B' is staged in LDS behind the group's
  const double* cst;      // device [kJkCst][kJkPad]
  double wsum[2], ysum[2], ybar[2];  // W_g (n_g when unweighted), sum w y, the point estimate's mean outcome
  uint32_t blocks0;       // blocks of group A (group B's follow)
  uint32_t units[2];      // waves with work, per group
  uint32_t rbu[2];        // 16-row blocks per wave
  int c;                  // 6 + 2 k
  double* rows;           // ROWS: (n_a + n_b) x c row-major
  uint8_t* kept;          // ROWS: n_a + n_b
  double* partial[2];     // sums: [3 c][units[g]]
  unsigned long long* counts;  // [2][2]: kept, dropped per group
};

__device__ __forceinline__ double row_sum16(double v) {  // over the 16 lanes of a kq: xor butterfly at 1, 2, 4, 8
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// One coefficient of one row: decomposition.rs:56-122 from the group's own (bw, xw) and the other group's (bo, xo)
// values and the reference coefficient bst. s: the lane's running six sums.
__device__ __forceinline__ void jack_column(int g, double bw, double bo, double xw, double xo, double bst_pool, int ref,
                                            double w_a, double w_b, double s[6], double& dex, double& dun) {
  const double xa = g == 0 ? xw : xo, xb = g == 0 ? xo : xw;
  const double ba = g == 0 ? bw : bo, bb = g == 0 ? bo : bw;
  double bst;
  if (ref == OB_REF_GROUP_A) bst = ba;
  else if (ref == OB_REF_GROUP_B) bst = bb;
  else if (ref == OB_REF_WEIGHTED) bst = ba * w_a + bb * w_b;
  else bst = bst_pool;
  const double dx = xa - xb, db = ba - bb;
  s[0] += dx * bst;
  s[1] += xa * ba;
  s[2] += xb * bb;
  s[3] += dx * bb;
  s[4] += xb * db;
  s[5] += dx * db;
  dex = dx * bst;
  dun = xa * (ba - bst) + xb * (bst - bb);
}

// The same coefficient's DEVIATIONS from the point estimate, for the sums path. With u' = u + du every product of
// decomposition.rs:56-122 changes by u'v' - uv = du v' + u dv, and the changes themselves are at hand: the own
// group's mean moves by dxo = w (xbar - x_i) / (W - w), its beta by dbo = -t w e / (1 - h), the reference coefficient
// by dbs. Taking theta_(i) - theta_hat as a difference instead would carry the rounding of theta_hat (an ulp of the
// mean outcome for `unexplained`) into every row alike, and jack_bias multiplies that by m_g - 1.
// pa, pb, qa, qb, ps: the point estimate's beta_A, beta_B, xbar_A, xbar_B, beta*. s: the six sums' deviations.
__device__ __forceinline__ void jack_delta(int g, double pa, double pb, double qa, double qb, double ps, double dxo,
                                           double dbo, double dbs, double s[6], double& dex, double& dun) {
  const double dxa = g == 0 ? dxo : 0.0, dxb = g == 0 ? 0.0 : dxo;
  const double dba = g == 0 ? dbo : 0.0, dbb = g == 0 ? 0.0 : dbo;
  const double na = pa + dba, nb = pb + dbb, ns = ps + dbs;  // the values without the row
  const double pdx = qa - qb, ddx = dxa - dxb, ddb = dba - dbb, ndb = (pa - pb) + ddb;
  dex = ddx * ns + pdx * dbs;
  dun = dxa * (na - ns) + qa * (dba - dbs) + dxb * (ns - nb) + qb * (dbs - dbb);
  s[0] += dex;
  s[1] += dxa * na + qa * dba;
  s[2] += dxb * nb + qb * dbb;
  s[3] += ddx * nb + pdx * dbb;
  s[4] += dxb * ndb + qb * ddb;
  s[5] += ddx * ndb + pdx * ddb;
}

template <int NJB, bool ROWS>
__global__ __launch_bounds__(kJkBlock) void ob_jackknife_kernel(const JackArgs a) {
  extern __shared__ __attribute__((aligned(16))) double bs[];  // [4 ns][ldb], then (pool_lds) [4 nsp][ldb]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, li = lane & 15;
  const int g = blockIdx.x < a.blocks0 ? 0 : 1;
  const uint32_t bi = g ? blockIdx.x - a.blocks0 : blockIdx.x;
  const int k = a.k, ldb = a.ldb;
  const bool pooled = a.pooled != 0;
  const int nb = 4 * a.ns * ldb;
  for (int i = tid; i < nb; i += kJkBlock) bs[i] = a.bg[g][i];
  const double* bpl = a.bpool;
  if (pooled && a.pool_lds) {
    const int nbp = 4 * a.nsp * ldb;
    for (int i = tid; i < nbp; i += kJkBlock) bs[nb + i] = a.bpool[i];
    bpl = bs + nb;
  }
  __syncthreads();
  const uint32_t unit = bi * kJkWaves + wave;
  if (unit >= a.units[g]) return;  // whole waves only, after the block's one barrier
  const int64_t n = a.n[g], ld = a.ld[g];
  const double* X = a.cols[g];
  const double* Y = X + (size_t)a.p * ld;
  const double* Wt = a.weighted ? Y + ld : nullptr;
  const int64_t row_off = g ? a.n[0] : 0;
  const int64_t nrb = (n + 15) / 16;
  const int64_t rb0 = (int64_t)unit * a.rbu[g], rb1 = min(nrb, rb0 + (int64_t)a.rbu[g]);
  const double wg = a.wsum[g], yo = a.ybar[1 - g];
  const double* b_own = a.cst + (size_t)g * kJkPad;
  const double* b_oth = a.cst + (size_t)(1 - g) * kJkPad;
  const double* s_own = a.cst + (size_t)(2 + g) * kJkPad;
  const double* x_oth = a.cst + (size_t)(4 + (1 - g)) * kJkPad;
  const double* b_pool = a.cst + (size_t)6 * kJkPad;
  double sx[NJB][3], su[NJB][3], s6[6][3];
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
    for (int t = 0; t < 3; ++t) sx[jb][t] = su[jb][t] = 0.0;
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int t = 0; t < 3; ++t) s6[q][t] = 0.0;
  uint32_t n_keep = 0, n_drop = 0;
  const double* b_a = a.cst;
  const double* b_b = a.cst + (size_t)kJkPad;
  const double* x_a = a.cst + (size_t)4 * kJkPad;
  const double* x_b = a.cst + (size_t)5 * kJkPad;
  const double w_tot = a.wsum[0] + a.wsum[1];
  const double w_a0 = a.wsum[0] / w_tot, w_b0 = 1.0 - w_a0;  // the point estimate's Cotton weights
  for (int64_t rb = rb0; rb < rb1; ++rb) {
    const int64_t row = rb * 16 + li;
    const bool live = row < n;
    ob_d4 acc[NJB], accp[NJB];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) acc[jb] = accp[jb] = (ob_d4){0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < a.ns; ++s) {
      const int c = 4 * s + kq;
      double av = 0.0;
      if (live) av = c == 0 ? 1.0 : (c < k ? X[(size_t)(c - 1) * ld + row] : 0.0);
      const double* brow = bs + c * ldb + li;
#pragma unroll
      for (int jb = 0; jb < NJB; ++jb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[16 * jb], acc[jb], 0, 0, 0);
    }
    if (pooled) {
      for (int s = 0; s < a.nsp; ++s) {
        const int c = 4 * s + kq;
        double av = 0.0;
        if (live) av = c == 0 ? 1.0 : (c < k ? X[(size_t)(c - 1) * ld + row] : (c == k && g == 0 ? 1.0 : 0.0));
        const double* brow = bpl + c * ldb + li;
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb)
          accp[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[16 * jb], accp[jb], 0, 0, 0);
      }
    }
    // lane (kq, li), element r of acc[jb]: row 16 rb + kq + 4 r, column 16 jb + li. Columns below k: t_i;
    // column k: the fitted value (pooled: the indicator's entry of P^-1 z_i); pooled column k + 1: z_i'beta_P
    double h[4] = {0.0, 0.0, 0.0, 0.0}, hp[4] = {0.0, 0.0, 0.0, 0.0};
    double f[4] = {0.0, 0.0, 0.0, 0.0}, fp[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
      const int col = 16 * jb + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row2 = rb * 16 + kq + 4 * r;
        if (row2 >= n) continue;
        if (col < k) {
          const double xv = col == 0 ? 1.0 : X[(size_t)(col - 1) * ld + row2];
          h[r] = fma(acc[jb][r], xv, h[r]);
          if (pooled) hp[r] = fma(accp[jb][r], xv, hp[r]);
        } else if (col == k) {
          f[r] = acc[jb][r];
          if (pooled && g == 0) hp[r] += accp[jb][r];  // the indicator is 1 on A's rows
        } else if (col == k + 1) {
          if (pooled) fp[r] = accp[jb][r];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h[r] = row_sum16(h[r]);
      f[r] = row_sum16(f[r]);
      if (pooled) {
        hp[r] = row_sum16(hp[r]);
        fp[r] = row_sum16(fp[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row2 = rb * 16 + kq + 4 * r;
      const bool valid = row2 < n;
      const double w = valid ? (Wt ? Wt[row2] : 1.0) : 0.0;
      const double y = valid ? Y[row2] : 0.0;
      const double om = 1.0 - w * h[r], wm = wg - w;
      const double omp = 1.0 - w * hp[r];
      bool keep = valid && om > OB_JACK_TINY && wm > 0.0;
      if (pooled) keep = keep && omp > OB_JACK_TINY;
      const double c1 = w * (y - f[r]) / om;
      const double c2 = pooled ? w * (y - fp[r]) / omp : 0.0;
      double w_a = 0.0, w_b = 0.0;
      if (a.ref == OB_REF_WEIGHTED) {  // builder.rs:591-619 without the row
        const double sa = a.wsum[0] - (g == 0 ? w : 0.0), sb = a.wsum[1] - (g == 1 ? w : 0.0);
        w_a = sa / (sa + sb);
        w_b = 1.0 - w_a;
      }
      // sums path: the row's share of its group's weight, and the change of the Cotton weights
      const double rw = w / wm;
      const double d_wa = (g == 0 ? -(w * a.wsum[1]) : w * a.wsum[0]) / ((w_tot - w) * w_tot);
      const double w_own = wm / (w_tot - w);
      double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int jb = 0; jb < NJB; ++jb) {
        const int col = 16 * jb + li;
        if (col >= k) continue;
        const double xv = valid ? (col == 0 ? 1.0 : X[(size_t)(col - 1) * ld + row2]) : 0.0;
        double dex, dun;
        if (ROWS) {
          const double bw = b_own[col] - acc[jb][r] * c1, bo = b_oth[col];
          const double xw = (s_own[col] - w * xv) / wm, xo = x_oth[col];
          jack_column(g, bw, bo, xw, xo, b_pool[col] - accp[jb][r] * c2, a.ref, w_a, w_b, s, dex, dun);
          if (valid) {
            double* out = a.rows + (size_t)(row_off + row2) * a.c + 6 + col;
            out[0] = keep ? dex : __builtin_nan("");
            out[k] = keep ? dun : __builtin_nan("");
          }
        } else {
          const double pa = b_a[col], pb = b_b[col];
          const double dxo = rw * ((g == 0 ? x_a[col] : x_b[col]) - xv), dbo = -(acc[jb][r] * c1);
          double ps, dbs;
          if (a.ref == OB_REF_GROUP_A) {
            ps = pa;
            dbs = g == 0 ? dbo : 0.0;
          } else if (a.ref == OB_REF_GROUP_B) {
            ps = pb;
            dbs = g == 0 ? 0.0 : dbo;
          } else if (a.ref == OB_REF_WEIGHTED) {
            ps = pa * w_a0 + pb * w_b0;
            dbs = dbo * w_own + (pa - pb) * d_wa;
          } else {
            ps = b_pool[col];
            dbs = -(accp[jb][r] * c2);
          }
          jack_delta(g, pa, pb, x_a[col], x_b[col], ps, dxo, dbo, dbs, s, dex, dun);
        }
        if (!ROWS && keep) {
          const double d0 = dex, d1 = dun;
          sx[jb][0] += d0;
          sx[jb][1] = fma(d0, d0, sx[jb][1]);
          sx[jb][2] = fma(d0 * d0, d0, sx[jb][2]);
          su[jb][0] += d1;
          su[jb][1] = fma(d1, d1, su[jb][1]);
          su[jb][2] = fma(d1 * d1, d1, su[jb][2]);
        }
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) s[q] = row_sum16(s[q]);
      // rows: theta_(i) itself; sums: its deviation (s holds deviations there)
      const double ym = ROWS ? (a.ysum[g] - w * y) / wm : rw * (a.ybar[g] - y);
      const double th[6] = {s[0], (s[1] - s[2]) - s[0], s[3], s[4], s[5],
                            ROWS ? (g == 0 ? ym - yo : yo - ym) : (g == 0 ? ym : -ym)};
      if (ROWS) {
        if (valid && li == 0) {
          double* out = a.rows + (size_t)(row_off + row2) * a.c;
#pragma unroll
          for (int q = 0; q < 6; ++q) out[q] = keep ? th[q] : __builtin_nan("");
          a.kept[row_off + row2] = keep ? 1 : 0;
        }
      } else if (keep) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const double d = th[q];
          s6[q][0] += d;
          s6[q][1] = fma(d, d, s6[q][1]);
          s6[q][2] = fma(d * d, d, s6[q][2]);
        }
      }
      if (valid && li == 0) {
        if (keep) ++n_keep;
        else ++n_drop;
      }
    }
  }
  if (!ROWS) {
    // the four kq of a lane column hold different rows of the same coefficient: add them at 16, 32
    double* part = a.partial[g];
    const size_t nu = a.units[g];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
      const int col = 16 * jb + li;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        double v = sx[jb][t], u = su[jb][t];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        u += __shfl_xor(u, 16);
        u += __shfl_xor(u, 32);
        if (kq == 0 && col < k) {
          part[((size_t)(6 + col) * 3 + t) * nu + unit] = v;
          part[((size_t)(6 + k + col) * 3 + t) * nu + unit] = u;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        double v = s6[q][t];  // the same in the 16 lanes of a kq
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lane == 0) part[((size_t)q * 3 + t) * nu + unit] = v;
      }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_keep += __shfl_xor(n_keep, off);
    n_drop += __shfl_xor(n_drop, off);
  }
  if (lane == 0) {
    if (n_keep) atomicAdd(&a.counts[2 * g], (unsigned long long)n_keep);
    if (n_drop) atomicAdd(&a.counts[2 * g + 1], (unsigned long long)n_drop);
  }
}

template <int NJB>
int jack_launch(const JackArgs& a, bool rows, uint32_t blocks, size_t lds, hipStream_t st) {
  if (rows) {
    OB_HIP(hipFuncSetAttribute((const void*)ob_jackknife_kernel<NJB, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    hipLaunchKernelGGL((ob_jackknife_kernel<NJB, true>), dim3(blocks), dim3(kJkBlock), lds, st, a);
  } else {
    OB_HIP(hipFuncSetAttribute((const void*)ob_jackknife_kernel<NJB, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    hipLaunchKernelGGL((ob_jackknife_kernel<NJB, false>), dim3(blocks), dim3(kJkBlock), lds, st, a);
  }
  OB_HIP(hipGetLastError());
  return OB_OK;
}

// m^-1 (k x k column-major) from the Cholesky factor that chol_factor left in m's lower triangle.
void inverse_from_factor(const std::vector<double>& l, int k, std::vector<double>& inv) {
  inv.assign((size_t)k * k, 0.0);
  for (int c = 0; c < k; ++c) {
    double* col = inv.data() + (size_t)c * k;
    col[c] = 1.0;
    ob::chol_solve(l.data(), k, col, ob::BackSub::Dot);
  }
}

}  // namespace

namespace ob {

int jackknife_device(ob_panel* p, int ref_mode, JackResult& out, double* theta, uint8_t* kept) {
  const bool rows = theta != nullptr;
  const int k = p->k, k1 = p->k1, c = 6 + 2 * k;
  const int ref = ref_mode == OB_REF_COTTON ? OB_REF_WEIGHTED : (ref_mode == OB_REF_NEUMARK ? OB_REF_POOLED : ref_mode);
  const bool pooled = ref == OB_REF_POOLED;
  out = JackResult();
  out.c = c;
  // the point estimate: theta_hat, beta_A, beta_B, the means, and the two extended Grams it reduced
  std::vector<double> row((size_t)p->row_len);
  OB_TRY(ob_point_estimate(p, ref_mode, row.data(), nullptr));
  if (!p->pe_gram_ready) return fail(OB_E_INVALID, "jackknife: the point estimate left no Gram");
  ob_ctx* ctx = p->ctx;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::vector<double> gram((size_t)2 * p->e_pad);
  OB_HIP(hipMemcpyAsync(gram.data(), p->d_pe + p->pe_gram_off, sizeof(double) * gram.size(), hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  out.point.assign(row.begin(), row.begin() + c);
  const double* tail = row.data() + c;  // beta_a, beta_b, xa_mean, xb_mean, beta_star (n_norm = 0: kd = k)
  const int yc = p->p + 1;
  auto gp = [&](int g, int r, int q) {
    const double* G = gram.data() + (size_t)g * p->e_pad;
    return r <= q ? G[ob_pair_index(r, q, k1)] : G[ob_pair_index(q, r, k1)];
  };
  const char* msg_chol =
      "%sFailed to perform Cholesky decomposition. Matrix may be singular or not positive definite due to "
      "multicollinearity.";
  JackArgs a = {};
  const int ncol = k + 2;  // the pooled B' is the widest: K columns of P^-1, the indicator's, beta_P
  const int njb_need = (ncol + 15) / 16;
  const int njb = njb_need <= 1 ? 1 : (njb_need <= 2 ? 2 : (njb_need <= 4 ? 4 : 8));
  a.ns = (k + 3) / 4;
  a.nsp = (k + 1 + 3) / 4;
  a.ldb = 16 * (njb | 1);
  const size_t nb = (size_t)4 * a.ns * a.ldb, nbp = (size_t)4 * a.nsp * a.ldb;
  std::vector<double> bg[2], bpool, cst((size_t)kJkCst * kJkPad, 0.0);
  for (int g = 0; g < 2; ++g) {
    std::vector<double> m((size_t)k * k), inv;
    for (int q = 0; q < k; ++q)
      for (int r = 0; r < k; ++r) m[r + (size_t)q * k] = gp(g, r, q);
    if (!chol_factor(m.data(), k)) return fail(OB_E_LINALG, msg_chol, error_prefix(OB_E_LINALG));
    inverse_from_factor(m, k, inv);
    bg[g].assign(nb, 0.0);
    for (int r = 0; r < k; ++r) {
      for (int q = 0; q < k; ++q) bg[g][(size_t)r * a.ldb + q] = inv[r + (size_t)q * k];
      bg[g][(size_t)r * a.ldb + k] = tail[g * k + r];
    }
    a.wsum[g] = p->weighted ? gp(g, 0, 0) : (double)p->n[g];
    a.ysum[g] = gp(g, 0, yc);
    a.ybar[g] = a.ysum[g] / gp(g, 0, 0);
    for (int j = 0; j < k; ++j) {
      cst[(size_t)g * kJkPad + j] = tail[g * k + j];
      cst[(size_t)(2 + g) * kJkPad + j] = gp(g, 0, j);
      cst[(size_t)(4 + g) * kJkPad + j] = tail[(2 + g) * k + j];
    }
  }
  if (pooled) {  // builder.rs:547-590, with the indicator moved from 1 + n_num to the end (a permutation only)
    const int kp = k + 1;
    std::vector<double> m((size_t)kp * kp), rhs(kp), inv;
    for (int q = 0; q < kp; ++q)
      for (int r = 0; r < kp; ++r) {
        double v;
        if (r == k && q == k) v = gp(0, 0, 0);
        else if (r == k || q == k) v = gp(0, 0, r == k ? q : r);
        else v = gp(0, r, q) + gp(1, r, q);
        m[r + (size_t)q * kp] = v;
      }
    for (int r = 0; r < kp; ++r) rhs[r] = r == k ? gp(0, 0, yc) : gp(0, r, yc) + gp(1, r, yc);
    if (!chol_factor(m.data(), kp)) return fail(OB_E_LINALG, msg_chol, error_prefix(OB_E_LINALG));
    chol_solve(m.data(), kp, rhs.data(), BackSub::Dot);
    inverse_from_factor(m, kp, inv);
    bpool.assign(nbp, 0.0);
    for (int r = 0; r < kp; ++r) {
      for (int q = 0; q < kp; ++q) bpool[(size_t)r * a.ldb + q] = inv[r + (size_t)q * kp];  // column k: the indicator's
      bpool[(size_t)r * a.ldb + kp] = rhs[r];
    }
    for (int j = 0; j < k; ++j) cst[(size_t)6 * kJkPad + j] = rhs[j];
  }
  for (int g = 0; g < 2; ++g) {
    a.cols[g] = p->d_cols[g];
    a.ld[g] = p->ld[g];
    a.n[g] = p->n[g];
    const int64_t nrb = ((int64_t)p->n[g] + 15) / 16;
    a.rbu[g] = (uint32_t)std::max<int64_t>(1, (nrb + kJkUnitsPerGroup - 1) / kJkUnitsPerGroup);
    a.units[g] = (uint32_t)((nrb + a.rbu[g] - 1) / a.rbu[g]);
  }
  a.p = p->p;
  a.k = k;
  a.weighted = p->weighted;
  a.ref = ref;
  a.pooled = pooled ? 1 : 0;
  a.c = c;
  a.blocks0 = (a.units[0] + kJkWaves - 1) / kJkWaves;
  const uint32_t blocks = a.blocks0 + (a.units[1] + kJkWaves - 1) / kJkWaves;
  a.pool_lds = pooled && sizeof(double) * (nb + nbp) <= kJkLds ? 1 : 0;
  const size_t lds = sizeof(double) * (nb + (a.pool_lds ? nbp : 0));
  if (lds > kJkLds) return fail(OB_E_UNSUPPORTED, "jackknife: the design does not fit in LDS");
  const int64_t n_all = (int64_t)p->n[0] + p->n[1];
  DevBuf dbg[2], dbp, dcst, dpart[2], dsum, dcnt, drows, dkept;
  for (int g = 0; g < 2; ++g) {
    OB_HIP(dbg[g].alloc(sizeof(double) * nb));
    OB_HIP(hipMemcpyAsync(dbg[g].p, bg[g].data(), sizeof(double) * nb, hipMemcpyHostToDevice, st));
    a.bg[g] = dbg[g].d();
  }
  if (pooled) {
    OB_HIP(dbp.alloc(sizeof(double) * nbp));
    OB_HIP(hipMemcpyAsync(dbp.p, bpool.data(), sizeof(double) * nbp, hipMemcpyHostToDevice, st));
    a.bpool = dbp.d();
  }
  OB_HIP(dcst.alloc(sizeof(double) * cst.size()));
  OB_HIP(hipMemcpyAsync(dcst.p, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice, st));
  a.cst = dcst.d();
  OB_HIP(dcnt.alloc(sizeof(unsigned long long) * 4));
  OB_HIP(hipMemsetAsync(dcnt.p, 0, sizeof(unsigned long long) * 4, st));
  a.counts = dcnt.as<unsigned long long>();
  if (rows) {
    OB_HIP(drows.alloc(sizeof(double) * (size_t)n_all * c));
    OB_HIP(dkept.alloc((size_t)n_all));
    a.rows = drows.d();
    a.kept = dkept.as<uint8_t>();
  } else {
    OB_HIP(dsum.alloc(sizeof(double) * 2 * 3 * c));
    for (int g = 0; g < 2; ++g) {
      OB_HIP(dpart[g].alloc(sizeof(double) * (size_t)3 * c * a.units[g]));
      a.partial[g] = dpart[g].d();
    }
  }
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipEventRecord(ev.e[0], st));
  switch (njb) {
    case 1: OB_TRY(jack_launch<1>(a, rows, blocks, lds, st)); break;
    case 2: OB_TRY(jack_launch<2>(a, rows, blocks, lds, st)); break;
    case 4: OB_TRY(jack_launch<4>(a, rows, blocks, lds, st)); break;
    default: OB_TRY(jack_launch<kJkMaxJb>(a, rows, blocks, lds, st)); break;
  }
  if (!rows)
    for (int g = 0; g < 2; ++g) {
      hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(3 * c), dim3(kSumBlock), 0, st, (const double*)dpart[g].d(),
                         a.units[g], dsum.d() + (size_t)g * 3 * c);
      OB_HIP(hipGetLastError());
    }
  OB_HIP(hipEventRecord(ev.e[1], st));
  unsigned long long counts[4] = {0, 0, 0, 0};
  OB_HIP(hipMemcpyAsync(counts, dcnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
  if (rows) {
    OB_HIP(hipMemcpyAsync(theta, drows.p, sizeof(double) * (size_t)n_all * c, hipMemcpyDeviceToHost, st));
    OB_HIP(hipMemcpyAsync(kept, dkept.p, (size_t)n_all, hipMemcpyDeviceToHost, st));
  } else {
    out.sums.assign((size_t)2 * 3 * c, 0.0);
    OB_HIP(hipMemcpyAsync(out.sums.data(), dsum.p, sizeof(double) * out.sums.size(), hipMemcpyDeviceToHost, st));
  }
  OB_HIP(hipStreamSynchronize(st));  // the host arrays above are read by the copies until here
  float ms = 0.f;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  out.ms = ms;
  for (int g = 0; g < 2; ++g) {
    out.kept[g] = (int64_t)counts[2 * g];
    out.dropped[g] = (int64_t)counts[2 * g + 1];
  }
  return OB_OK;
}

}  // namespace ob
