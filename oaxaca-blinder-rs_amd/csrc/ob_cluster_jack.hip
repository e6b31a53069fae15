// ob_cluster_jack.hip -- the delete-one-cluster jackknife of a clustered run, the
// leave-one-out pass behind BCa intervals and the cluster-robust jackknife standard error. Everything it reads
// is resident in a clustered ob_prepared: the per-cluster extended Grams Q[c][g], the clusters' row counts and
// the point estimate. Deleting cluster c downdates group g's Gram by Q^xx_c, a matrix of rank up to K, so the
// Sherman-Morrison update of ob_jackknife.hip does not serve; with M = G_g - Q^xx_c and r_c = b_c - Q^xx_c beta_g
//
//   beta_g(c) - beta_g = -M^-1 r_c,     xbar_g(c) - xbar_g = (W_c xbar_g - S_c) / (W_g - W_c)
//
// exactly, the same downdate of the pooled Gram (the indicator as its last column) for Pooled / Neumark and the
// Cotton weights from W_g - W_c (row counts without weights).
//
//   ob_cluster_jack_kernel  the `sums` path. One wave per cluster, four waves per block, every wave walks its
//     stratum's clusters in cluster order at a stride of the launch's waves (a function of C alone). M and the
//     pooled matrix sit in the wave's own LDS slice, column-major at a column stride of 33 doubles; the factorisation and the two
//     triangular solves are wave-cooperative (ob_device.hpp's, with the leading dimension and the pivot rule
//     added). A lane owns a coefficient: the deviations d = theta_(c) - theta_hat of the 6 + 2K components come
//     from the changes themselves (the product rule of ob_jackknife.hip's jack_delta, here with both groups
//     moving at once), the six aggregates are butterflies. Per wave and component the power sums of d over its
//     kept clusters go to the wave's own slot; ob_ordered_sum_kernel adds a stratum's slots in a fixed order.
//     No floating atomics: two calls return the same bytes. Kept and dropped counts are integer atomics.
//   ob_cluster_loo_kernel   the `rows` path. out[i][g] = T_g - Q[c][g] in the [ns][2][e_pad] layout the solve
//     kernel reads (T_g = sum_c Q[c][g] in ob_cluster_apply's order) and rep_rows = n_g - rows_c,g; a group the
//     cluster has no row in receives the point estimate's own Gram, so its beta and means are the point
//     estimate's bitwise. ob_solve_kernel and ob_cluster_guard_kernel then give theta_(c) in the solve's algebra.
//
// A cluster is DROPPED when n_g - rows_c,g <= K for a group it touches (the reference's InsufficientData), when
// W_g - W_c <= 0, or when a pivot of M (of the pooled downdate) is at most 2^-40 times the same pivot of the
// point estimate's factor: the fit without the cluster has no solution.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ob_builder.hpp"
#include "ob_cluster.hpp"
#include "ob_device.hpp"
#include "ob_hip.hpp"
#include "ob_linalg.hpp"

namespace {

constexpr int kCjWaves = 4;          // waves (clusters in flight) per block
constexpr int kCjLd = 33;            // doubles between the columns of a wave's matrices
constexpr int kCjVec = 40;           // the wave's right-hand side (K + 1 <= 33 entries)
constexpr int kCjMaxBlocks = 1024;   // 4,096 slots per stratum at most
constexpr int kCjPad = 64;           // stride of the per-column constants
// rows of the constants: beta_A, beta_B, xbar_A, xbar_B, beta*, the pivot floors of G_A, G_B and the pooled Gram, beta_P
enum { kCjBetaA = 0, kCjBetaB, kCjXbarA, kCjXbarB, kCjStar, kCjFloorA, kCjFloorB, kCjFloorP, kCjBetaP, kCjCst };
constexpr uint64_t kCjBatchBudget = (uint64_t)1 << 30;  // bytes of downdated Grams per batch of the rows path
constexpr uint64_t kCjBatchMax = 16384;

struct CjArgs {
  const double* q;        // [C][2][e_pad]
  const uint32_t* qrows;  // [C][2]
  uint32_t s_beg[2], s_end[2];  // the strata's cluster ranges
  int n_strata;
  int k, k1, e_pad, ref, pooled, weighted;
  const double* gram;     // the point estimate's extended Grams [2][e_pad]
  const double* pg;       // Pooled: its Gram, (k + 1) x (k + 1) column-major, the indicator last
  const double* cst;      // [kCjCst][kCjPad]
  double wsum[2], ybar[2];  // W_g (n_g without weights), the point estimate's mean outcome
  uint32_t n[2];
  uint32_t units;         // waves of the launch = slots per stratum
  int wave_doubles;       // LDS doubles per wave
  int c;                  // 6 + 2 k
  double* partial;        // [2][3 c][units]
  unsigned long long* counts;  // [2][2]: kept, dropped per stratum
  uint8_t* kept;          // optional [C]
  double* dev;            // optional [C][c]: every cluster's deviations d themselves (NaN for a dropped one)
};

// ob_device.hpp's wave_cholesky (nalgebra's order) on a matrix of leading dimension ld, with the pivot rule:
// false as soon as pivot j is not above floor[j] (a zero, negative or NaN pivot included, floor >= 0).
__device__ bool cj_cholesky(double* m, int n, int ld, const double* floor, int lane) {
  for (int j = 0; j < n; ++j) {
    for (int i = j + lane; i < n; i += 64) {
      double v = m[i + j * ld];
      for (int c = 0; c < j; ++c) v = -m[j + c * ld] * m[i + c * ld] + v;
      m[i + j * ld] = v;
    }
    ob_sync<true>();
    const double diag = m[j + j * ld];
    if (!(diag > floor[j])) return false;
    const double den = sqrt(diag);
    ob_sync<true>();
    for (int i = j + lane; i < n; i += 64) m[i + j * ld] = (i == j) ? den : m[i + j * ld] / den;
    ob_sync<true>();
  }
  return true;
}

// ob_device.hpp's wave_chol_solve on a factor of leading dimension ld.
__device__ void cj_solve(const double* l, int n, int ld, double* b, int lane) {
  for (int i = 0; i < n; ++i) {
    const double coeff = b[i] / l[i + i * ld];
    ob_sync<true>();
    for (int r = i + 1 + lane; r < n; r += 64) b[r] -= coeff * l[r + i * ld];
    if (lane == 0) b[i] = coeff;
    ob_sync<true>();
  }
  for (int i = n - 1; i >= 0; --i) {
    double part = 0.0;
    for (int r = i + 1 + lane; r < n; r += 64) part += l[r + i * ld] * b[r];
    part = wave_sum(part);
    if (lane == 0) b[i] = (b[i] - part) / l[i + i * ld];
    ob_sync<true>();
  }
}

// Entry (u, v) of what deleting the cluster takes from the pooled Gram: design columns first, the indicator
// (1 on A's rows) as column k. qa / qb: the cluster's Q in A / B, NULL where it has no row.
__device__ __forceinline__ double cj_pool_take(const double* qa, const double* qb, int u, int v, int k, int k1) {
  if (u == k || v == k) {
    if (!qa) return 0.0;
    return (u == k && v == k) ? qa[0] : gpair(qa, 0, u == k ? v : u, k1);
  }
  return (qa ? gpair(qa, u, v, k1) : 0.0) + (qb ? gpair(qb, u, v, k1) : 0.0);
}

__global__ __launch_bounds__(kCjWaves * 64) void ob_cluster_jack_kernel(const CjArgs a) {
  extern __shared__ __attribute__((aligned(16))) double cj_sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t unit = blockIdx.x * kCjWaves + w;  // below a.units: the grid is units / kCjWaves blocks
  const int k = a.k, kp = k + 1, k1 = a.k1, yc = k;  // one outcome: v = [1, x, y]
  double* M = cj_sm + (size_t)w * a.wave_doubles;    // k x k, then (pooled) (k + 1) x (k + 1), then the rhs
  double* P = M + k * kCjLd;
  double* rhs = P + (a.pooled ? kp * kCjLd : 0);
  const bool mine = lane < k;
  const double pa = mine ? a.cst[kCjBetaA * kCjPad + lane] : 0.0, pb = mine ? a.cst[kCjBetaB * kCjPad + lane] : 0.0;
  const double qa = mine ? a.cst[kCjXbarA * kCjPad + lane] : 0.0, qb = mine ? a.cst[kCjXbarB * kCjPad + lane] : 0.0;
  const double ps = mine ? a.cst[kCjStar * kCjPad + lane] : 0.0;
  const double w_tot = a.wsum[0] + a.wsum[1];
  for (int s = 0; s < a.n_strata; ++s) {
    double sx[3] = {0.0, 0.0, 0.0}, su[3] = {0.0, 0.0, 0.0}, s6[6][3];
#pragma unroll
    for (int q = 0; q < 6; ++q) s6[q][0] = s6[q][1] = s6[q][2] = 0.0;
    uint32_t n_keep = 0, n_drop = 0;
    for (uint64_t c = (uint64_t)a.s_beg[s] + unit; c < a.s_end[s]; c += a.units) {
      bool keep = true;
      double db[2] = {0.0, 0.0}, dx[2] = {0.0, 0.0}, dy[2] = {0.0, 0.0}, wc[2] = {0.0, 0.0};
      const double* qg[2] = {nullptr, nullptr};
      for (int g = 0; g < 2 && keep; ++g) {
        const uint32_t rows = a.qrows[2 * c + g];
        if (rows == 0) continue;  // the group stays at the point estimate: no solve, every change 0.0
        if (a.n[g] - rows <= (uint32_t)k) {
          keep = false;
          break;
        }
        const double* Q = a.q + (2 * c + g) * (size_t)a.e_pad;
        const double* G = a.gram + (size_t)g * a.e_pad;
        qg[g] = Q;
        wc[g] = a.weighted ? Q[0] : (double)rows;
        const double wm = a.wsum[g] - wc[g];
        if (!(wm > 0.0)) {
          keep = false;
          break;
        }
        for (int i = lane; i < k * k; i += 64) {
          const int r = i % k, cc = i / k;
          M[r + cc * kCjLd] = gpair(G, r, cc, k1) - gpair(Q, r, cc, k1);
        }
        if (mine) {  // r_c = b_c - Q^xx_c beta_g
          const double* beta = a.cst + (size_t)(g ? kCjBetaB : kCjBetaA) * kCjPad;
          double v = gpair(Q, lane, yc, k1);
          for (int j = 0; j < k; ++j) v = fma(-gpair(Q, lane, j, k1), beta[j], v);
          rhs[lane] = v;
        }
        ob_sync<true>();
        if (!cj_cholesky(M, k, kCjLd, a.cst + (size_t)(g ? kCjFloorB : kCjFloorA) * kCjPad, lane)) {
          keep = false;
          break;
        }
        cj_solve(M, k, kCjLd, rhs, lane);
        if (mine) {
          db[g] = -rhs[lane];
          dx[g] = (wc[g] * (g ? qb : qa) - gpair(Q, 0, lane, k1)) / wm;
        }
        dy[g] = (wc[g] * a.ybar[g] - gpair(Q, 0, yc, k1)) / wm;
        ob_sync<true>();  // rhs and M are read: the next fill may overwrite them
      }
      double dbs = 0.0;
      if (keep) {
        if (a.ref == OB_REF_GROUP_A) {
          dbs = db[0];
        } else if (a.ref == OB_REF_GROUP_B) {
          dbs = db[1];
        } else if (a.ref == OB_REF_WEIGHTED) {  // builder.rs:591-619 without the cluster
          const double rest = w_tot - wc[0] - wc[1];
          const double w_a = (a.wsum[0] - wc[0]) / rest;
          const double d_wa = (a.wsum[0] * wc[1] - wc[0] * a.wsum[1]) / (rest * w_tot);
          dbs = db[0] * w_a + db[1] * (1.0 - w_a) + (pa - pb) * d_wa;
        } else {  // Pooled / Neumark: the same downdate of the pooled fit
          const double* beta = a.cst + (size_t)kCjBetaP * kCjPad;
          for (int i = lane; i < kp * kp; i += 64) {
            const int u = i % kp, v = i / kp;
            P[u + v * kCjLd] = a.pg[u + v * kp] - cj_pool_take(qg[0], qg[1], u, v, k, k1);
          }
          if (lane < kp) {
            double v = lane == k ? (qg[0] ? gpair(qg[0], 0, yc, k1) : 0.0)
                                 : (qg[0] ? gpair(qg[0], lane, yc, k1) : 0.0) + (qg[1] ? gpair(qg[1], lane, yc, k1) : 0.0);
            for (int j = 0; j < kp; ++j) v = fma(-cj_pool_take(qg[0], qg[1], lane, j, k, k1), beta[j], v);
            rhs[lane] = v;
          }
          ob_sync<true>();
          if (!cj_cholesky(P, kp, kCjLd, a.cst + (size_t)kCjFloorP * kCjPad, lane)) {
            keep = false;
          } else {
            cj_solve(P, kp, kCjLd, rhs, lane);
            if (mine) dbs = -rhs[lane];  // the indicator's coefficient (entry k) is dropped
          }
          ob_sync<true>();
        }
      }
      if (keep) {
        // decomposition.rs:56-122 as deviations: u'v' - uv = du v' + u dv for every product
        const double dxa = dx[0], dxb = dx[1], dba = db[0], dbb = db[1];
        const double na = pa + dba, nb = pb + dbb, ns = ps + dbs;  // the values without the cluster
        const double pdx = qa - qb, ddx = dxa - dxb, ddb = dba - dbb, ndb = (pa - pb) + ddb;
        const double dex = ddx * ns + pdx * dbs;
        const double dun = dxa * (na - ns) + qa * (dba - dbs) + dxb * (ns - nb) + qb * (dbs - dbb);
        const double t0 = wave_sum(dex);
        const double t1 = wave_sum(dxa * na + qa * dba);
        const double t2 = wave_sum(dxb * nb + qb * dbb);
        const double t3 = wave_sum(ddx * nb + pdx * dbb);
        const double t4 = wave_sum(dxb * ndb + qb * ddb);
        const double t5 = wave_sum(ddx * ndb + pdx * ddb);
        const double th[6] = {t0, (t1 - t2) - t0, t3, t4, t5, dy[0] - dy[1]};
        sx[0] += dex;
        sx[1] = fma(dex, dex, sx[1]);
        sx[2] = fma(dex * dex, dex, sx[2]);
        su[0] += dun;
        su[1] = fma(dun, dun, su[1]);
        su[2] = fma(dun * dun, dun, su[2]);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const double d = th[q];
          s6[q][0] += d;
          s6[q][1] = fma(d, d, s6[q][1]);
          s6[q][2] = fma(d * d, d, s6[q][2]);
        }
        ++n_keep;
        if (a.dev) {
          double* o = a.dev + c * (size_t)a.c;
          if (mine) {
            o[6 + lane] = dex;
            o[6 + k + lane] = dun;
          }
          if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) o[q] = th[q];
          }
        }
      } else {
        ++n_drop;
        if (a.dev)
          for (int j = lane; j < a.c; j += 64) a.dev[c * (size_t)a.c + j] = __builtin_nan("");
      }
      if (a.kept && lane == 0) a.kept[c] = keep ? 1 : 0;
    }
    double* part = a.partial + (size_t)s * 3 * a.c * a.units;
    if (mine) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        part[((size_t)(6 + lane) * 3 + t) * a.units + unit] = sx[t];
        part[((size_t)(6 + k + lane) * 3 + t) * a.units + unit] = su[t];
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int t = 0; t < 3; ++t) part[((size_t)q * 3 + t) * a.units + unit] = s6[q][t];
      if (n_keep) atomicAdd(&a.counts[2 * s], (unsigned long long)n_keep);
      if (n_drop) atomicAdd(&a.counts[2 * s + 1], (unsigned long long)n_drop);
    }
  }
}

// out[i][g][e] = T_g[e] - Q[c0 + i][g][e], or the point estimate's Gram where the cluster has no row in g;
// rep_rows[i][g] = n_g - rows of the cluster in g. One thread per entry.
__global__ __launch_bounds__(256) void ob_cluster_loo_kernel(const double* q, const uint32_t* qrows, const double* total,
                                                             const double* point, uint32_t c0, uint32_t ns, int e_pad,
                                                             uint32_t n_a, uint32_t n_b, double* out, uint32_t* rep_rows) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t width = 2 * (size_t)e_pad;
  if (i >= (size_t)ns * width) return;
  const size_t r = i / width, col = i - r * width;
  const int g = col >= (size_t)e_pad ? 1 : 0;
  const size_t c = (size_t)c0 + r;
  const uint32_t rows = qrows[2 * c + g];
  out[i] = rows ? total[col] - q[c * width + col] : point[col];
  if (col == (size_t)g * e_pad) rep_rows[2 * r + g] = (g ? n_b : n_a) - rows;
}

}  // namespace


namespace ob {

int cluster_jack_pass(ob_ctx* ctx, const ClusterView& cv, const ClusterPoint& pt, JackResult& out, uint8_t* kept,
                      double* dev) {
  const int k = pt.k, k1 = pt.k1, kp = k + 1, c = 6 + 2 * k, e_pad = pt.e_pad;
  if (k < 1 || k > kClusterJackMaxK || k1 != k + 1) return fail(OB_E_UNSUPPORTED, "cluster jackknife: the panel is outside its scope");
  const int ref_mode = pt.ref_mode;
  const int ref = ref_mode == OB_REF_COTTON ? OB_REF_WEIGHTED : (ref_mode == OB_REF_NEUMARK ? OB_REF_POOLED : ref_mode);
  const bool pooled = ref == OB_REF_POOLED;
  out = JackResult();
  out.c = c;
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const double* gram = pt.gram;
  const double* tail = pt.tail;  // beta_a, beta_b, xa_mean, xb_mean, beta_star
  const int yc = k;
  auto gp = [&](int g, int r, int q) {
    const double* G = gram + (size_t)g * e_pad;
    return r <= q ? G[ob_pair_index(r, q, k1)] : G[ob_pair_index(q, r, k1)];
  };
  const char* msg_chol =
      "%sFailed to perform Cholesky decomposition. Matrix may be singular or not positive definite due to "
      "multicollinearity.";
  const double tiny = 0x1p-40;  // §5.10's condition: a pivot this far below the point estimate's is no pivot
  CjArgs a = {};
  std::vector<double> cst((size_t)kCjCst * kCjPad, 0.0), pg;
  for (int g = 0; g < 2; ++g) {
    std::vector<double> m((size_t)k * k);
    for (int q = 0; q < k; ++q)
      for (int r = 0; r < k; ++r) m[r + (size_t)q * k] = gp(g, r, q);
    if (!chol_factor(m.data(), k)) return fail(OB_E_LINALG, msg_chol, error_prefix(OB_E_LINALG));
    for (int j = 0; j < k; ++j) {
      const double l = m[j + (size_t)j * k];
      cst[(size_t)(kCjFloorA + g) * kCjPad + j] = tiny * (l * l);
      cst[(size_t)(kCjBetaA + g) * kCjPad + j] = tail[g * k + j];
      cst[(size_t)(kCjXbarA + g) * kCjPad + j] = tail[(2 + g) * k + j];
      cst[(size_t)kCjStar * kCjPad + j] = tail[4 * k + j];
    }
    a.wsum[g] = pt.weighted ? gp(g, 0, 0) : (double)pt.n[g];
    a.ybar[g] = gp(g, 0, yc) / gp(g, 0, 0);
    a.n[g] = pt.n[g];
  }
  if (pooled) {  // builder.rs:547-590 with the indicator moved to the end (a permutation only, as in §5.10)
    pg.assign((size_t)kp * kp, 0.0);
    std::vector<double> rhs(kp);
    for (int q = 0; q < kp; ++q)
      for (int r = 0; r < kp; ++r) {
        double v;
        if (r == k && q == k) v = gp(0, 0, 0);
        else if (r == k || q == k) v = gp(0, 0, r == k ? q : r);
        else v = gp(0, r, q) + gp(1, r, q);
        pg[r + (size_t)q * kp] = v;
      }
    for (int r = 0; r < kp; ++r) rhs[r] = r == k ? gp(0, 0, yc) : gp(0, r, yc) + gp(1, r, yc);
    std::vector<double> m(pg);
    if (!chol_factor(m.data(), kp)) return fail(OB_E_LINALG, msg_chol, error_prefix(OB_E_LINALG));
    chol_solve(m.data(), kp, rhs.data(), BackSub::Dot);
    for (int j = 0; j < kp; ++j) {
      const double l = m[j + (size_t)j * kp];
      cst[(size_t)kCjFloorP * kCjPad + j] = tiny * (l * l);
      cst[(size_t)kCjBetaP * kCjPad + j] = rhs[j];
      if (j < k) cst[(size_t)kCjStar * kCjPad + j] = rhs[j];
    }
  }
  // theta_hat from the same values (decomposition.rs:56-122); a prepared handle replaces it by its point row
  out.point.assign(c, 0.0);
  {
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < k; ++j) {
      const double ba = tail[j], bb = tail[k + j], xa = tail[2 * k + j], xb = tail[3 * k + j];
      const double bs = cst[(size_t)kCjStar * kCjPad + j], dx = xa - xb, db = ba - bb;
      s[0] += dx * bs;
      s[1] += xa * ba;
      s[2] += xb * bb;
      s[3] += dx * bb;
      s[4] += xb * db;
      s[5] += dx * db;
      out.point[6 + j] = dx * bs;
      out.point[6 + k + j] = xa * (ba - bs) + xb * (bs - bb);
    }
    const double six[6] = {s[0], (s[1] - s[2]) - s[0], s[3], s[4], s[5], a.ybar[0] - a.ybar[1]};
    std::copy(six, six + 6, out.point.begin());
  }
  const uint32_t nc = cv.n_clusters;
  a.q = cv.q;
  a.qrows = cv.qrows;
  a.n_strata = cv.stratified ? 2 : 1;
  a.s_beg[0] = 0;
  a.s_end[0] = cv.stratified ? cv.n_clusters_a : nc;
  a.s_beg[1] = a.s_end[0];
  a.s_end[1] = nc;
  const uint32_t widest = std::max(a.s_end[0] - a.s_beg[0], a.s_end[1] - a.s_beg[1]);
  const uint32_t blocks = std::min<uint32_t>(std::max<uint32_t>((widest + kCjWaves - 1) / kCjWaves, 1u), kCjMaxBlocks);
  a.units = blocks * kCjWaves;
  a.k = k;
  a.k1 = k1;
  a.e_pad = e_pad;
  a.ref = ref;
  a.pooled = pooled ? 1 : 0;
  a.weighted = pt.weighted;
  a.c = c;
  a.wave_doubles = k * kCjLd + (pooled ? kp * kCjLd : 0) + kCjVec;
  const size_t lds = sizeof(double) * kCjWaves * (size_t)a.wave_doubles;
  DevBuf dgram, dpg, dcst, dpart, dsum, dcnt, dkeep, ddev;
  OB_HIP(dgram.alloc(sizeof(double) * 2 * e_pad));
  OB_HIP(hipMemcpyAsync(dgram.p, gram, sizeof(double) * 2 * e_pad, hipMemcpyHostToDevice, st));
  a.gram = dgram.d();
  if (pooled) {
    OB_HIP(dpg.alloc(sizeof(double) * pg.size()));
    OB_HIP(hipMemcpyAsync(dpg.p, pg.data(), sizeof(double) * pg.size(), hipMemcpyHostToDevice, st));
    a.pg = dpg.d();
  }
  OB_HIP(dcst.alloc(sizeof(double) * cst.size()));
  OB_HIP(hipMemcpyAsync(dcst.p, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice, st));
  a.cst = dcst.d();
  OB_HIP(dpart.alloc(sizeof(double) * 2 * 3 * c * (size_t)a.units));
  a.partial = dpart.d();
  OB_HIP(dsum.alloc(sizeof(double) * 2 * 3 * c));
  OB_HIP(hipMemsetAsync(dsum.p, 0, sizeof(double) * 2 * 3 * c, st));
  OB_HIP(dcnt.alloc(sizeof(unsigned long long) * 4));
  OB_HIP(hipMemsetAsync(dcnt.p, 0, sizeof(unsigned long long) * 4, st));
  a.counts = dcnt.as<unsigned long long>();
  if (kept) {
    OB_HIP(dkeep.alloc(nc));
    a.kept = dkeep.as<uint8_t>();
  }
  if (dev) {
    OB_HIP(ddev.alloc(sizeof(double) * (size_t)nc * c));
    a.dev = ddev.d();
  }
  Events<2> ev;
  OB_HIP(ev.create());
  OB_HIP(hipEventRecord(ev.e[0], st));
  OB_HIP(hipFuncSetAttribute((const void*)ob_cluster_jack_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ob_cluster_jack_kernel, dim3(blocks), dim3(kCjWaves * 64), lds, st, a);
  OB_HIP(hipGetLastError());
  for (int s = 0; s < a.n_strata; ++s) {
    hipLaunchKernelGGL(ob_ordered_sum_kernel<>, dim3(3 * c), dim3(kSumBlock), 0, st,
                       (const double*)(dpart.d() + (size_t)s * 3 * c * a.units), a.units, dsum.d() + (size_t)s * 3 * c);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(ev.e[1], st));
  unsigned long long counts[4] = {0, 0, 0, 0};
  OB_HIP(hipMemcpyAsync(counts, dcnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
  out.sums.assign((size_t)2 * 3 * c, 0.0);
  OB_HIP(hipMemcpyAsync(out.sums.data(), dsum.p, sizeof(double) * out.sums.size(), hipMemcpyDeviceToHost, st));
  if (kept) OB_HIP(hipMemcpyAsync(kept, dkeep.p, nc, hipMemcpyDeviceToHost, st));
  if (dev) OB_HIP(hipMemcpyAsync(dev, ddev.p, sizeof(double) * (size_t)nc * c, hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));  // the host arrays above are read or written by the copies until here
  float ms = 0.f;
  OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  out.ms = ms;
  for (int s = 0; s < 2; ++s) {
    out.kept[s] = (int64_t)counts[2 * s];
    out.dropped[s] = (int64_t)counts[2 * s + 1];
  }
  return OB_OK;
}

// theta_(c) itself, in the solve kernel's algebra, batch by batch; kept: in, the sums pass's mask; out, the final one.
int cluster_jack_rows(ob_panel* p, const ClusterView& cv, const ClusterPoint& pt, double* theta, uint8_t* kept,
                      JackResult& out) {
  const uint32_t nc = cv.n_clusters;
  const int e_pad = p->e_pad, width = 2 * e_pad, rl = p->row_len;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  DevBuf dgram, dtot, dloo, drr, drows, dok;
  OB_HIP(dgram.alloc(sizeof(double) * width));
  OB_HIP(hipMemcpyAsync(dgram.p, pt.gram, sizeof(double) * width, hipMemcpyHostToDevice, st));
  OB_HIP(dtot.alloc(sizeof(double) * width));
  OB_TRY(cluster_sum_q(cv.q, nc, width, dtot.d(), st));
  const uint64_t per = (uint64_t)width * 8 + (uint64_t)rl * 8 + 16;
  const uint64_t batch = std::min<uint64_t>(std::min<uint64_t>(nc, kCjBatchMax),
                                            std::max<uint64_t>(16, kCjBatchBudget / per / 16 * 16));
  OB_HIP(dloo.alloc(sizeof(double) * batch * width));
  OB_HIP(drr.alloc(sizeof(uint32_t) * batch * 2));
  OB_HIP(drows.alloc(sizeof(double) * batch * rl));
  OB_HIP(dok.alloc(batch));
  std::vector<uint8_t> ok(batch);
  out.kept[0] = out.kept[1] = out.dropped[0] = out.dropped[1] = 0;
  const uint32_t s_end0 = cv.stratified ? cv.n_clusters_a : nc;
  for (uint64_t s0 = 0; s0 < nc; s0 += batch) {  // a batch's rows go back to the host before the next one runs
    const uint32_t ns = (uint32_t)std::min<uint64_t>(batch, nc - s0);
    const size_t items = (size_t)ns * width;
    hipLaunchKernelGGL(ob_cluster_loo_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, cv.q, cv.qrows,
                       (const double*)dtot.d(), (const double*)dgram.d(), (uint32_t)s0, ns, e_pad, p->n[0], p->n[1],
                       dloo.d(), drr.as<uint32_t>());
    OB_HIP(hipGetLastError());
    OB_TRY(engine_solve_grams(p, dloo.d(), drr.as<uint32_t>(), ns, ns, 0, pt.ref_mode, drows.d(), dok.as<uint8_t>(), st));
    OB_TRY(cluster_guard(p, drr.as<uint32_t>(), ns, ns, 0, drows.d(), dok.as<uint8_t>(), st));
    OB_HIP(hipMemcpyAsync(theta + (size_t)s0 * rl, drows.p, sizeof(double) * (size_t)ns * rl, hipMemcpyDeviceToHost, st));
    OB_HIP(hipMemcpyAsync(ok.data(), dok.p, ns, hipMemcpyDeviceToHost, st));
    OB_HIP(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < ns; ++i) {  // the pivot rule of the sums path holds here as well
      const size_t cl = (size_t)s0 + i;
      const bool keep = ok[i] && kept[cl];
      kept[cl] = keep ? 1 : 0;
      (keep ? out.kept : out.dropped)[cv.stratified && cl >= s_end0 ? 1 : 0] += 1;
      if (!keep)
        for (int j = 0; j < rl; ++j) theta[cl * rl + j] = NAN;
    }
  }
  return OB_OK;
}

int cluster_jack_device(ob_prepared* pr, JackResult& out, double* theta, uint8_t* kept, double* dev) {
  ob_panel* p = pr->panel;
  if (p->k > kClusterJackMaxK || p->n_y != 1) return fail(OB_E_UNSUPPORTED, "cluster jackknife: the panel is outside its scope");
  const int c = 6 + 2 * p->k;
  // the point estimate: theta_hat, beta_A, beta_B, the means, and the two extended Grams it reduced
  std::vector<double> row((size_t)p->row_len);
  OB_TRY(ob_point_estimate(p, pr->ref, row.data(), nullptr));
  if (!p->pe_gram_ready) return fail(OB_E_INVALID, "cluster jackknife: the point estimate left no Gram");
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t st = p->ctx->stream;
  OB_TRY(engine_order(p, st));
  std::vector<double> gram((size_t)2 * p->e_pad);
  OB_HIP(hipMemcpyAsync(gram.data(), p->d_pe + p->pe_gram_off, sizeof(double) * gram.size(), hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  ClusterPoint pt;
  pt.k = p->k;
  pt.k1 = p->k1;
  pt.e_pad = p->e_pad;
  pt.weighted = p->weighted;
  pt.ref_mode = pr->ref;
  pt.n[0] = p->n[0];
  pt.n[1] = p->n[1];
  pt.gram = gram.data();
  pt.tail = row.data() + c;  // n_norm = 0: kd = k
  ClusterView cv;
  OB_TRY(cluster_view(pr, st, cv));
  OB_TRY(cluster_jack_pass(p->ctx, cv, pt, out, kept, dev));
  out.point.assign(row.begin(), row.begin() + c);
  if (theta) OB_TRY(cluster_jack_rows(p, cv, pt, theta, kept, out));
  return engine_mark(p, st);
}

// installs the cluster jackknife's hook when the library loads (ob_cluster.hpp)
static const bool g_jack_hook_installed = [] {
  cluster_hooks().jack = cluster_jack_device;
  return true;
}();

}  // namespace ob

// ---- the array-level entry points ---------------------------------------------------------------------------
namespace {

// Q [C][2][e_pad] and rows [C][2] of the caller on the device, as a ClusterView.
struct CjUpload {
  DevBuf q, rows;
  ob::ClusterView cv;
};

int cj_upload(ob_ctx* ctx, const double* q, const uint32_t* rows, int64_t nc, int64_t nca, int stratified, int e_pad,
              CjUpload& u) {
  OB_HIP(hipSetDevice(ctx->device));
  OB_HIP(u.q.alloc(sizeof(double) * (size_t)nc * 2 * e_pad));
  OB_HIP(u.rows.alloc(sizeof(uint32_t) * (size_t)nc * 2));
  OB_HIP(hipMemcpy(u.q.p, q, sizeof(double) * (size_t)nc * 2 * e_pad, hipMemcpyHostToDevice));
  OB_HIP(hipMemcpy(u.rows.p, rows, sizeof(uint32_t) * (size_t)nc * 2, hipMemcpyHostToDevice));
  u.cv.q = u.q.d();
  u.cv.qrows = u.rows.as<uint32_t>();
  u.cv.n_clusters = (uint32_t)nc;
  u.cv.n_clusters_a = (uint32_t)nca;
  u.cv.stratified = stratified ? 1 : 0;
  return OB_OK;
}

}  // namespace

extern "C" {

int ob_cluster_jackknife(ob_ctx* ctx, const double* q, const uint32_t* rows, int64_t n_clusters, int64_t n_clusters_a,
                         int32_t stratified, int32_t p, int32_t weighted, int64_t n_a, int64_t n_b, const double* gram,
                         const double* tail, int ref_mode, ob_jackknife_out* out) {
  if (p < 0 || p > 120) return ob::fail(OB_E_INVALID, "bad predictor count");
  OB_TRY(ob::cluster_jack_check_shape(p + 1, n_clusters, 0, 1, 0, 0));
  if (!ctx || !q || !rows || !gram || !tail || !out) return ob::fail(OB_E_INVALID, "null pointer");
  if (ref_mode < OB_REF_GROUP_A || ref_mode > OB_REF_NEUMARK)
    return ob::fail(OB_E_INVALID, "unknown reference coefficients %d", ref_mode);
  if (n_clusters_a < 0 || n_clusters_a > n_clusters || n_a < 1 || n_b < 1 || n_a >= ((int64_t)1 << 31) ||
      n_b >= ((int64_t)1 << 31))
    return ob::fail(OB_E_INVALID, "bad cluster or row counts");
  const int k = p + 1, c = 6 + 2 * k, k1 = k + 1, e_pad = (k1 * (k1 + 1) / 2 + 15) / 16 * 16;
  if (out->capacity < c || !out->point || !out->sums || !out->stats)
    return ob::fail(OB_E_INVALID, "cluster jackknife: the output arrays must hold %d components", c);
  OB_TRY(ob::cluster_check_shape(n_clusters, k1));  // Q within 8 GiB
  for (int64_t i = 0; i < n_clusters; ++i)  // a cluster never holds more rows than its group
    if (rows[2 * i] > (uint64_t)n_a || rows[2 * i + 1] > (uint64_t)n_b)
      return ob::fail(OB_E_INVALID, "cluster %lld has more rows than its group", (long long)i);
  CjUpload u;
  OB_TRY(cj_upload(ctx, q, rows, n_clusters, n_clusters_a, stratified, e_pad, u));
  ob::ClusterPoint pt;
  pt.k = k;
  pt.k1 = k1;
  pt.e_pad = e_pad;
  pt.weighted = weighted ? 1 : 0;
  pt.ref_mode = ref_mode;
  pt.n[0] = (uint32_t)n_a;
  pt.n[1] = (uint32_t)n_b;
  pt.gram = gram;
  pt.tail = tail;
  ob::JackResult r;
  OB_TRY(ob::cluster_jack_pass(ctx, u.cv, pt, r, nullptr, nullptr));
  ob::cluster_jack_set_timing(r.ms);
  OB_TRY(ob::cluster_jack_enough(r));
  out->n_components = c;
  for (int s = 0; s < 2; ++s) {
    out->n_used[s] = r.kept[s];
    out->n_dropped[s] = r.dropped[s];
  }
  std::copy(r.point.begin(), r.point.end(), out->point);
  std::copy(r.sums.begin(), r.sums.end(), out->sums);
  ob::jackknife_finish(out->sums, out->n_used, c, out->stats);
  return OB_OK;
}

int ob_cluster_jackknife_rows(ob_panel* panel, const double* q, const uint32_t* rows, int64_t n_clusters,
                              int64_t n_clusters_a, int32_t stratified, int ref_mode, double* theta, uint8_t* kept,
                              int64_t* n_dropped, double* deviations) {
  if (!panel) return ob::fail(OB_E_INVALID, "null pointer");
  OB_TRY(ob::cluster_jack_check_shape(panel->heckman ? panel->k - 1 : panel->k, n_clusters, panel->norm.n_norm, panel->n_y,
                                      panel->heckman, 1));
  if (!q || !rows || !theta || !kept) return ob::fail(OB_E_INVALID, "null pointer");
  if (ref_mode < OB_REF_GROUP_A || ref_mode > OB_REF_NEUMARK)
    return ob::fail(OB_E_INVALID, "unknown reference coefficients %d", ref_mode);
  if (n_clusters_a < 0 || n_clusters_a > n_clusters) return ob::fail(OB_E_INVALID, "bad cluster counts");
  OB_TRY(ob::cluster_check_shape(n_clusters, panel->k1));  // Q within 8 GiB
  for (int64_t i = 0; i < n_clusters; ++i)
    if (rows[2 * i] > panel->n[0] || rows[2 * i + 1] > panel->n[1])
      return ob::fail(OB_E_INVALID, "cluster %lld has more rows than its group", (long long)i);
  const int c = 6 + 2 * panel->k;
  std::vector<double> row((size_t)panel->row_len);
  OB_TRY(ob_point_estimate(panel, ref_mode, row.data(), nullptr));
  if (!panel->pe_gram_ready) return ob::fail(OB_E_INVALID, "cluster jackknife: the point estimate left no Gram");
  OB_HIP(hipSetDevice(panel->ctx->device));
  hipStream_t st = panel->ctx->stream;
  OB_TRY(ob::engine_order(panel, st));
  std::vector<double> gram((size_t)2 * panel->e_pad);
  OB_HIP(hipMemcpyAsync(gram.data(), panel->d_pe + panel->pe_gram_off, sizeof(double) * gram.size(), hipMemcpyDeviceToHost, st));
  OB_HIP(hipStreamSynchronize(st));
  CjUpload u;
  OB_TRY(cj_upload(panel->ctx, q, rows, n_clusters, n_clusters_a, stratified, panel->e_pad, u));
  ob::ClusterPoint pt;
  pt.k = panel->k;
  pt.k1 = panel->k1;
  pt.e_pad = panel->e_pad;
  pt.weighted = panel->weighted;
  pt.ref_mode = ref_mode;
  pt.n[0] = panel->n[0];
  pt.n[1] = panel->n[1];
  pt.gram = gram.data();
  pt.tail = row.data() + c;
  ob::JackResult r;
  OB_TRY(ob::cluster_jack_pass(panel->ctx, u.cv, pt, r, kept, deviations));
  ob::cluster_jack_set_timing(r.ms);
  OB_TRY(ob::cluster_jack_rows(panel, u.cv, pt, theta, kept, r));
  if (n_dropped) {
    n_dropped[0] = r.dropped[0];
    n_dropped[1] = r.dropped[1];
  }
  return ob::engine_mark(panel, st);
}

}  // extern "C"
