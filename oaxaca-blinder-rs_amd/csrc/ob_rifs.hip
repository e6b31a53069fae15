// ob_rifs.hip -- the RIF of the variance, the Gini and quantile ranges refitted on a resample, without a sort or an
// n-length column per replicate.
//
// Setting of ob_rifq.hip: a group's rows stand in stable ascending order of y; a replicate is its OBRS-3 counts c_i
// over those rows (the engine's level-1 tile counts and level-2 count images). Per statistic the regression needs
// its value nu and the y-pairs G[a, RIF], G[RIF, RIF] of the extended Gram over [1, x, RIF]:
//   rifs_moment_kernel   block per (row chunk, 16 replicates), in the shape of rifq_density_kernel: the variance sums
//                        M0_a, M1_a, M2_a, M3, M4 about the sample's own mean and the chunk's sum c y;
//   rifs_scan_kernel     wave per replicate: the chunk totals (sum c, sum c y) into exclusive chunk carries;
//   rifs_gini_kernel     same block shape: a scan over the replicate's 16 row groups gives every row its inclusive
//                        prefixes Cin, Sin, carried from sub-tile to sub-tile and started by the chunk carry; the sums
//                        over z_i = y_i (1 - Cin_i / n) + Sin_i / n;
//   rifs_tie_kernel      wave per (replicate, group): the tie-run term E of the Gini's R in run order;
//   rifs_finish_kernel   wave per (replicate, group, statistic): the chunk partials in chunk order, then nu and the
//                        y-pairs. A quantile range combines the outputs of ob_rifq.hip's kernels here.
// The point pass is the same code with every row counted once (counts == NULL). No floating-point atomics: every sum
// has an order fixed by the group's size and the chunk table, so a replicate's values have the same bytes alone, in
// any batch and for a statistic alone or among others.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ob_builder.hpp"
#include "ob_cluster.hpp"
#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_model.hpp"
#include "ob_rif.hpp"
#include "ob_rifq.hpp"
#include "ob_rifs.hpp"
#include "ob_spec.h"

namespace {

constexpr int kSB = 256;    // threads of a moment or Gini block
constexpr int kSS = 65;     // doubles per staged column
constexpr int kSReps = 16;  // replicates per block
constexpr int kSRound = 8;  // sums reduced per round of the block's final ordered sum

struct RifsArgs {
  const double* cols[2];  // per group [k][ld]: y (ascending) | x_1 .. x_{k-1}
  int64_t ld[2];
  uint32_t n[2];
  uint32_t tile0[2];  // first tile of the group in the count images
  double mu0[2];      // the original sample's mean: the centre of the variance sums
  int k, n_groups, n_specs, n_taus;
  int stat[ob::kRifsMaxStats], hi[ob::kRifsMaxStats], lo[ob::kRifsMaxStats];
  double taus[ob::kRifqMaxTaus];
  const uint32_t* counts;  // level-2 count images (ob_engine.hpp, the f64 Gram's layout); NULL: every row once
  uint32_t nb_rep, part_pad, n_reps;
  const uint32_t* chunks;  // [chunk][3] = (g, t0, t1), ascending within a group
  int n_chunks;
  double* mpart;  // [chunk][part_pad][3k + 3]: M0_a, M1_a, M2_a, M3, M4, sum c y
  double* carry;  // [chunk][part_pad][2]: sum c, sum c y of the group's chunks before this one
  double* gpart;  // [chunk][part_pad][2k + 4]: Z_a, sum c v_a y, sum c z^2, sum c y z, sum c Sin, sum c y^2
  const uint32_t* runs;  // [run][3] = (g, row0, row1): the tie runs of more than one row, in row order
  int n_runs;
  double* tie;  // [rep][g] E
  // ob_rifq.hip's outputs per (replicate, group, tau), for the ranges
  const double *sq, *of, *onle, *qgy;
  const uint8_t* qfl;
  // outputs per (replicate, group, statistic)
  double* nu;
  double* gy;  // [..][k + 1] G[a, RIF] for a < k, then G[RIF, RIF]
  uint8_t* sok;
  uint8_t* fl;
};

// The count word of rows 4 q .. 4 q + 3 of sub-tile sw of the group's tile `tile`, replicate rep.
__device__ __forceinline__ uint32_t rifs_word(const RifsArgs& a, int g, uint32_t rep, uint32_t tile, uint32_t sw, uint32_t q) {
  if (!a.counts) return 0x01010101u;
  return a.counts[((((size_t)a.tile0[g] + tile) * a.nb_rep + (rep >> 6)) * 4 + sw) * kCimgWords + (rep & 63u) * kCimgStride + q];
}

// The block's final sum: the 16 row groups of a replicate added in row-group order through LDS, kSRound sums a round.
// Slot s of the KM-wide register layout (BL blocks of KM columns, then the scalars) lands at its place among the
// k-wide partials; the slots past the NS scalars pad the last round.
template <int KM, int BL, int NS, int NVP>
__device__ __forceinline__ void rifs_block_sum(const double (&vals)[NVP], double* red, double* out, int k, int tid, bool act) {
  const int r16 = tid & 15, q = tid >> 4;
#pragma unroll
  for (int rd = 0; rd < NVP / kSRound; ++rd) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSRound; ++i) red[(i * 16 + q) * kSReps + r16] = vals[rd * kSRound + i];
    __syncthreads();
    if (tid < kSRound * kSReps) {
      const int vi = tid >> 4, slot = rd * kSRound + vi;
      double v = 0.0;
      for (int qq = 0; qq < 16; ++qq) v += red[(vi * 16 + qq) * kSReps + r16];
      int dst = -1;
      if (slot < BL * KM) {
        const int b = slot / KM, j = slot - b * KM;
        if (j < k) dst = b * k + j;
      } else if (slot < BL * KM + NS) {
        dst = BL * k + (slot - BL * KM);
      }
      if (dst >= 0 && act) out[dst] = v;
    }
  }
}

// Block = (row chunk, 16 replicates), 4 waves; thread = (replicate t & 15, rows 4 (t >> 4) .. + 3 of each 64-row
// sub-tile: one count word). Per sub-tile the block stages the k columns once (LDS [col][65]); a counted row adds its
// terms into registers. A thread owns its rows over the whole chunk.
template <int KM>
__global__ __launch_bounds__(kSB) void rifs_moment_kernel(const RifsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ssm[];
  constexpr int NV = 3 * KM + 3, NVP = (NV + kSRound - 1) / kSRound * kSRound;
  const int tid = threadIdx.x, k = a.k;
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  double* stg = ssm;            // [k][kSS]
  double* red = stg + k * kSS;  // [kSRound][16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep = blockIdx.y * kSReps + r16;
  const bool act = rep < a.n_reps;
  double m0[KM], m1[KM], m2[KM], m3 = 0.0, m4 = 0.0, sy = 0.0;
#pragma unroll
  for (int j = 0; j < KM; ++j) m0[j] = m1[j] = m2[j] = 0.0;
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const double mu0 = a.mu0[g];
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's reads
      for (int i = tid; i < k * 64; i += kSB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kSS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      const uint32_t word = act ? rifs_word(a, g, rep, tile, sw, q) : 0u;
      double cd[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) cd[i] = (uint32_t)(4 * q + i) < nr ? (double)((word >> (8 * i)) & 255u) : 0.0;
      if (cd[0] + cd[1] + cd[2] + cd[3] == 0.0) continue;  // (uniform control flow resumes at the barrier)
      double w1[4], w2[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double yi = stg[4 * q + i], d = yi - mu0;
        w1[i] = cd[i] * d;
        w2[i] = w1[i] * d;
        const double w3 = w2[i] * d;
        m3 += w3;
        m4 += w3 * d;
        sy += cd[i] * yi;
      }
      m0[0] += cd[0] + cd[1] + cd[2] + cd[3];
      m1[0] += w1[0] + w1[1] + w1[2] + w1[3];
      m2[0] += w2[0] + w2[1] + w2[2] + w2[3];
#pragma unroll
      for (int j = 1; j < KM; ++j)
        if (j < k) {
          const double* zj = stg + j * kSS + 4 * q;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            m0[j] += cd[i] * zj[i];
            m1[j] += w1[i] * zj[i];
            m2[j] += w2[i] * zj[i];
          }
        }
    }
  }
  double vals[NVP];
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    vals[j] = m0[j];
    vals[KM + j] = m1[j];
    vals[2 * KM + j] = m2[j];
  }
  vals[3 * KM] = m3;
  vals[3 * KM + 1] = m4;
  vals[3 * KM + 2] = sy;
#pragma unroll
  for (int i = NV; i < NVP; ++i) vals[i] = 0.0;
  double* out = a.mpart + ((size_t)chunk * a.part_pad + (act ? rep : 0u)) * (3 * k + 3);
  rifs_block_sum<KM, 3, 3, NVP>(vals, red, out, k, tid, act);
}

// One wave per replicate, lane g < n_groups: the chunk totals of (sum c, sum c y) into exclusive carries, chunk order.
__global__ __launch_bounds__(64) void rifs_scan_kernel(const RifsArgs a) {
  const uint32_t rep = blockIdx.x;
  const int g = threadIdx.x, nvm = 3 * a.k + 3;
  if (g >= a.n_groups) return;
  double c = 0.0, s = 0.0;
  for (int ch = 0; ch < a.n_chunks; ++ch) {
    if (a.chunks[3 * ch] != (uint32_t)g) continue;
    const size_t o = (size_t)ch * a.part_pad + rep;
    a.carry[o * 2] = c;
    a.carry[o * 2 + 1] = s;
    c += a.mpart[o * nvm];
    s += a.mpart[o * nvm + nvm - 1];
  }
}

// The moment kernel's block shape. Per sub-tile a thread puts its four rows' (sum c, sum c y) into LDS, and every
// thread of a replicate adds the 16 row groups in row-group order: the prefix of the groups before its own starts its
// rows, the total carries to the next sub-tile. The thread is serial over its four rows.
template <int KM>
__global__ __launch_bounds__(kSB) void rifs_gini_kernel(const RifsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ssm[];
  constexpr int NV = 2 * KM + 4, NVP = (NV + kSRound - 1) / kSRound * kSRound;
  const int tid = threadIdx.x, k = a.k;
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  double* stg = ssm;                           // [k][kSS]
  double* red = stg + k * kSS;                 // [kSRound][16 row groups][16 replicates]
  double* scn = red + kSRound * 16 * kSReps;   // [2][16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep = blockIdx.y * kSReps + r16;
  const bool act = rep < a.n_reps;
  double zs[KM], ys[KM], zz = 0.0, yz = 0.0, cs = 0.0, yy = 0.0;
#pragma unroll
  for (int j = 0; j < KM; ++j) zs[j] = ys[j] = 0.0;
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const double nf = (double)n;
  double carC = 0.0, carS = 0.0;
  if (act) {
    carC = a.carry[((size_t)chunk * a.part_pad + rep) * 2];
    carS = a.carry[((size_t)chunk * a.part_pad + rep) * 2 + 1];
  }
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's reads of stg and scn
      for (int i = tid; i < k * 64; i += kSB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kSS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      const uint32_t word = act ? rifs_word(a, g, rep, tile, sw, q) : 0u;
      double cd[4], cy[4], yi[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cd[i] = (uint32_t)(4 * q + i) < nr ? (double)((word >> (8 * i)) & 255u) : 0.0;
        yi[i] = stg[4 * q + i];
        cy[i] = cd[i] * yi[i];
      }
      const double sc = cd[0] + cd[1] + cd[2] + cd[3];
      scn[q * kSReps + r16] = sc;
      scn[(16 + q) * kSReps + r16] = ((cy[0] + cy[1]) + cy[2]) + cy[3];
      __syncthreads();
      double C = 0.0, S = 0.0;
      for (int qq = 0; qq < 16; ++qq) {
        if (qq == q) {
          C = carC;
          S = carS;
        }
        carC += scn[qq * kSReps + r16];
        carS += scn[(16 + qq) * kSReps + r16];
      }
      if (sc == 0.0) continue;  // (the barriers above are behind; the next one is the loop's first)
      double wz[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        C += cd[i];
        S += cy[i];
        const double z = yi[i] * (1.0 - C / nf) + S / nf;
        wz[i] = cd[i] * z;
        zz += wz[i] * z;
        yz += wz[i] * yi[i];
        cs += cd[i] * S;
        yy += cy[i] * yi[i];
      }
      zs[0] += wz[0] + wz[1] + wz[2] + wz[3];
      ys[0] += cy[0] + cy[1] + cy[2] + cy[3];
#pragma unroll
      for (int j = 1; j < KM; ++j)
        if (j < k) {
          const double* zj = stg + j * kSS + 4 * q;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            zs[j] += wz[i] * zj[i];
            ys[j] += cy[i] * zj[i];
          }
        }
    }
  }
  double vals[NVP];
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    vals[j] = zs[j];
    vals[KM + j] = ys[j];
  }
  vals[2 * KM] = zz;
  vals[2 * KM + 1] = yz;
  vals[2 * KM + 2] = cs;
  vals[2 * KM + 3] = yy;
#pragma unroll
  for (int i = NV; i < NVP; ++i) vals[i] = 0.0;
  double* out = a.gpart + ((size_t)chunk * a.part_pad + (act ? rep : 0u)) * (2 * k + 4);
  rifs_block_sum<KM, 2, 4, NVP>(vals, red, out, k, tid, act);
}

inline size_t moment_lds(int k) { return sizeof(double) * ((size_t)k * kSS + (size_t)kSRound * 16 * kSReps); }
inline size_t gini_lds(int k) { return moment_lds(k) + sizeof(double) * 2 * 16 * kSReps; }

// One wave per (replicate, group): E = sum over the tie runs, in run order, of y_run (m_run^2 - sum c^2) / 2. The
// run's two sums are whole numbers below 2^53, so the order in which the lanes add them does not matter.
__global__ __launch_bounds__(64) void rifs_tie_kernel(const RifsArgs a) {
  const int lane = threadIdx.x, g = blockIdx.y;
  const uint32_t rep = blockIdx.x;
  double E = 0.0;
  for (int r = 0; r < a.n_runs; ++r) {
    if (a.runs[3 * r] != (uint32_t)g) continue;
    const uint32_t row0 = a.runs[3 * r + 1], row1 = a.runs[3 * r + 2];
    double m = 0.0, s2 = 0.0;
    for (uint32_t row = row0 + lane; row < row1; row += 64) {
      const uint32_t within = row & (OB_TILE_ROWS - 1u), qq = within & 63u;
      const uint32_t word = rifs_word(a, g, rep, row >> OB_TILE_SHIFT, within >> 6, qq >> 2);
      const double c = (double)((word >> (8 * (qq & 3u))) & 255u);
      m += c;
      s2 += c * c;
    }
    for (int w = 32; w > 0; w >>= 1) {
      m += __shfl_xor(m, w, 64);
      s2 += __shfl_xor(s2, w, 64);
    }
    E += a.cols[g][row0] * ((m * m - s2) * 0.5);
  }
  if (lane == 0) a.tie[(size_t)rep * a.n_groups + g] = E;
}

// One wave per (replicate, group, statistic). Lanes add the columns' chunk partials in chunk order (lane a, a + 64),
// then lane a < k forms G[a, RIF] and lane 0 nu and G[RIF, RIF].
__global__ __launch_bounds__(64) void rifs_finish_kernel(const RifsArgs a) {
  __shared__ double sh[3 * ob::kRifsMaxK + 3];
  __shared__ double sm0[ob::kRifsMaxK];
  const int lane = threadIdx.x, k = a.k, S = a.n_specs;
  const uint32_t rep = blockIdx.x;
  const int g = blockIdx.y / S, s = blockIdx.y - g * S, stat = a.stat[s];
  const size_t rg = (size_t)rep * a.n_groups + g, o = rg * S + s;
  const double nf = (double)a.n[g];
  const int nvm = 3 * k + 3, nvg = 2 * k + 4;
  double ga = 0.0, grr = 0.0, nu = 0.0;
  bool ok = true, floored = false;
  if (stat == OB_RIF_IQR) {
    const int T = a.n_taus, h = a.hi[s], l = a.lo[s];
    const size_t oh = rg * T + h, ol = rg * T + l;
    const double qh = a.sq[oh], ql = a.sq[ol], Bh = 1.0 / a.of[oh], Bl = 1.0 / a.of[ol];
    const double Ah = qh + a.taus[h] * Bh, Al = ql + a.taus[l] * Bl, nh = a.onle[oh], nl = a.onle[ol];
    if (lane < k) ga = a.qgy[oh * (k + 1) + lane] - a.qgy[ol * (k + 1) + lane];
    nu = qh - ql;
    const double cross = Ah * Al * nf - Ah * Bl * nl - Al * Bh * nh + Bh * Bl * nl;
    grr = a.qgy[oh * (k + 1) + k] + a.qgy[ol * (k + 1) + k] - 2.0 * cross;
    floored = a.qfl[oh] || a.qfl[ol];
  } else {
    const bool var = stat == OB_RIF_VARIANCE;
    const int nv = var ? nvm : nvg;
    const double* part = var ? a.mpart : a.gpart;
    for (int slot = lane; slot < nv; slot += 64) {
      double v = 0.0;
      for (int c = 0; c < a.n_chunks; ++c)
        if (a.chunks[3 * c] == (uint32_t)g) v += part[((size_t)c * a.part_pad + rep) * nv + slot];
      sh[slot] = v;
    }
    if (!var && lane < k) {  // the Gini's M0_a from the moment pass
      double v = 0.0;
      for (int c = 0; c < a.n_chunks; ++c)
        if (a.chunks[3 * c] == (uint32_t)g) v += a.mpart[((size_t)c * a.part_pad + rep) * nvm + lane];
      sm0[lane] = v;
    }
    __syncthreads();
    if (var) {
      const double M10 = sh[k], M20 = sh[2 * k], M3 = sh[3 * k], M4 = sh[3 * k + 1];
      const double dl = M10 / nf, d2 = dl * dl;
      nu = (M20 - nf * d2) / nf;
      if (lane < k) ga = sh[2 * k + lane] - 2.0 * dl * sh[k + lane] + d2 * sh[lane];
      grr = M4 - 4.0 * dl * M3 + 6.0 * d2 * M20 - 4.0 * (d2 * dl) * M10 + (d2 * d2) * nf;
    } else {
      const double Z0 = sh[0], Y0 = sh[k], zz = sh[2 * k], yz = sh[2 * k + 1], cs = sh[2 * k + 2], yy = sh[2 * k + 3];
      const double mu = Y0 / nf;
      ok = mu > 0.0;
      if (ok) {
        const double R = (cs + a.tie[rg]) / (nf * nf);
        const double al = 2.0 * R / (mu * mu), be = 2.0 / mu;
        nu = 1.0 - 2.0 * R / mu;
        if (lane < k) ga = sm0[lane] + al * sh[k + lane] - be * sh[lane];
        grr = nf + al * al * yy + be * be * zz + 2.0 * al * Y0 - 2.0 * be * Z0 - 2.0 * al * be * yz;
      } else {
        nu = NAN;
      }
    }
  }
  if (lane < k) a.gy[o * (k + 1) + lane] = ga;
  if (lane == 0) {
    a.gy[o * (k + 1) + k] = grr;
    a.nu[o] = nu;
    a.sok[o] = ok ? 1 : 0;
    a.fl[o] = floored ? 1 : 0;
  }
}

// The solved OLS rows [rep][rl0] of statistic t into the caller's rows [rep][rl0 + 2], with the tail nu_A, nu_B.
__global__ __launch_bounds__(64) void rifs_tail_kernel(const RifsArgs a, int t, const double* solved, const uint8_t* sok,
                                                       int rl0, double* rows, uint8_t* ok) {
  const uint32_t rep = blockIdx.x;
  double* row = rows + (size_t)rep * (rl0 + 2);
  for (int i = threadIdx.x; i < rl0; i += 64) row[i] = solved[(size_t)rep * rl0 + i];
  const size_t o0 = ((size_t)rep * 2) * a.n_specs + t, o1 = ((size_t)rep * 2 + 1) * a.n_specs + t;
  if (threadIdx.x < 2) row[rl0 + threadIdx.x] = a.nu[threadIdx.x ? o1 : o0];
  if (threadIdx.x == 0) ok[rep] = sok[rep] && a.sok[o0] && a.sok[o1] ? 1 : 0;
}

thread_local ob_rifs_timing g_timing = {};

// The device buffers of a pass: the partials, the quantile pass's buffers for the ranges and the outputs.
struct RifsWork {
  DevBuf mpart, carry, gpart, tie, nu, gy, sok, fl;
  DevBuf sq, sp, sbw, qpart, of, onle, ofl, ot, qgy;
};

// Every kernel the plan needs over the replicates of `a` (geometry, counts, chunks and runs set), enqueued on s, with
// the buffers of w. qa: the quantile pass's arguments with the same geometry (its m1 set); used when the plan has a
// range. e: 11 events, e[0] .. e[6] around the stages (rifq | moment | scan | gini | tie | finish).
int rifs_launch(RifsArgs& a, ob::RifqArgs& qa, const ob::RifsPlan& pl, RifsWork& w, hipStream_t s, hipEvent_t* e) {
  const int k = a.k, G = a.n_groups, S = pl.n_specs, T = pl.n_taus;
  const size_t pp = a.part_pad, nrs = pp * G * S;
  a.n_specs = S;
  a.n_taus = T;
  for (int i = 0; i < S; ++i) {
    a.stat[i] = pl.stat[i];
    a.hi[i] = pl.hi[i];
    a.lo[i] = pl.lo[i];
  }
  for (int i = 0; i < T; ++i) a.taus[i] = pl.taus[i];
  OB_HIP(w.nu.alloc(sizeof(double) * nrs));
  OB_HIP(w.gy.alloc(sizeof(double) * nrs * (k + 1)));
  OB_HIP(w.sok.alloc(nrs));
  OB_HIP(w.fl.alloc(nrs));
  a.nu = w.nu.d();
  a.gy = w.gy.d();
  a.sok = w.sok.as<uint8_t>();
  a.fl = w.fl.as<uint8_t>();
  OB_HIP(hipEventRecord(e[0], s));
  if (pl.range) {
    const size_t nrt = pp * G * T;
    OB_HIP(w.sq.alloc(sizeof(double) * nrt));
    OB_HIP(w.sp.alloc(sizeof(uint32_t) * nrt));
    OB_HIP(w.sbw.alloc(sizeof(double) * 3 * G * pp));
    OB_HIP(w.qpart.alloc(sizeof(double) * (size_t)a.n_chunks * pp * ob::rifq_sums_len(k)));
    OB_HIP(w.of.alloc(sizeof(double) * nrt));
    OB_HIP(w.onle.alloc(sizeof(double) * nrt));
    OB_HIP(w.ofl.alloc(nrt));
    OB_HIP(w.ot.alloc(sizeof(double) * nrt * k));
    OB_HIP(w.qgy.alloc(sizeof(double) * nrt * (k + 1)));
    for (int i = 0; i < T; ++i) qa.taus[i] = pl.taus[i];
    qa.n_taus = T;
    qa.sq = w.sq.d();
    qa.sp = w.sp.as<uint32_t>();
    qa.sbw = w.sbw.d();
    qa.partial = w.qpart.d();
    qa.of = w.of.d();
    qa.onle = w.onle.d();
    qa.ofl = w.ofl.as<uint8_t>();
    qa.ot = w.ot.d();
    qa.ogy = w.qgy.d();
    OB_TRY(ob::rifq_run(qa, s, e + 7));
    a.sq = qa.sq;
    a.of = qa.of;
    a.onle = qa.onle;
    a.qgy = qa.ogy;
    a.qfl = qa.ofl;
  }
  OB_HIP(hipEventRecord(e[1], s));
  const dim3 grid(a.n_chunks, (a.n_reps + kSReps - 1) / kSReps);
  if (pl.variance || pl.gini) {
    OB_HIP(w.mpart.alloc(sizeof(double) * (size_t)a.n_chunks * pp * (3 * k + 3)));
    a.mpart = w.mpart.d();
    const size_t lds = moment_lds(k);
    if (k <= 8) {
      OB_HIP(hipFuncSetAttribute((const void*)rifs_moment_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(rifs_moment_kernel<8>, grid, dim3(kSB), lds, s, a);
    } else {
      OB_HIP(hipFuncSetAttribute((const void*)rifs_moment_kernel<ob::kRifsMaxK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(rifs_moment_kernel<ob::kRifsMaxK>, grid, dim3(kSB), lds, s, a);
    }
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(e[2], s));
  if (pl.gini) {
    OB_HIP(w.carry.alloc(sizeof(double) * (size_t)a.n_chunks * pp * 2));
    OB_HIP(w.gpart.alloc(sizeof(double) * (size_t)a.n_chunks * pp * (2 * k + 4)));
    OB_HIP(w.tie.alloc(sizeof(double) * pp * G));
    a.carry = w.carry.d();
    a.gpart = w.gpart.d();
    a.tie = w.tie.d();
    hipLaunchKernelGGL(rifs_scan_kernel, dim3(a.n_reps), dim3(64), 0, s, a);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(e[3], s));
  if (pl.gini) {
    const size_t lds = gini_lds(k);
    if (k <= 8) {
      OB_HIP(hipFuncSetAttribute((const void*)rifs_gini_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(rifs_gini_kernel<8>, grid, dim3(kSB), lds, s, a);
    } else {
      OB_HIP(hipFuncSetAttribute((const void*)rifs_gini_kernel<ob::kRifsMaxK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(rifs_gini_kernel<ob::kRifsMaxK>, grid, dim3(kSB), lds, s, a);
    }
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(e[4], s));
  if (pl.gini) {
    hipLaunchKernelGGL(rifs_tie_kernel, dim3(a.n_reps, G), dim3(64), 0, s, a);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipEventRecord(e[5], s));
  hipLaunchKernelGGL(rifs_finish_kernel, dim3(a.n_reps, G * S), dim3(64), 0, s, a);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(e[6], s));
  return OB_OK;
}

// Adds the ms of the stages that ran once the stream has reached e[6].
int rifs_times(hipEvent_t* e, const ob::RifsPlan& pl) {
  float m[6] = {};
  for (int i = 0; i < 6; ++i) OB_HIP(hipEventElapsedTime(&m[i], e[i], e[i + 1]));
  if (pl.range) g_timing.rifq_ms += m[0];
  if (pl.variance || pl.gini) g_timing.moment_ms += m[1];
  if (pl.gini) {
    g_timing.scan_ms += m[2];
    g_timing.gini_ms += m[3];
    g_timing.tie_ms += m[4];
  }
  g_timing.finish_ms += m[5];
  return OB_OK;
}

// The tie runs of more than one row of a group's ascending y, appended as (g, row0, row1).
void tie_runs(const double* y, int64_t n, uint32_t g, std::vector<uint32_t>& runs) {
  for (int64_t i = 0; i < n;) {
    int64_t j = i + 1;
    while (j < n && y[j] == y[i]) ++j;
    if (j - i > 1) {
      runs.push_back(g);
      runs.push_back((uint32_t)i);
      runs.push_back((uint32_t)j);
    }
    i = j;
  }
}

}  // namespace

namespace ob {

int rifs_plan(const ob_rif_spec* specs, int n_specs, RifsPlan& out) {
  out = RifsPlan();
  if (!specs || n_specs < 1) return fail(OB_E_INVALID, "statistics refit: no statistic given");
  if (n_specs > kRifsMaxStats)
    return fail(OB_E_UNSUPPORTED, "statistics refit: at most %d statistics a pass, got %d", kRifsMaxStats, n_specs);
  OB_TRY(rif_spec_check(specs, n_specs));
  std::vector<double> taus;
  for (int s = 0; s < n_specs; ++s)
    if (specs[s].stat == OB_RIF_IQR) {
      taus.push_back(specs[s].p0);
      taus.push_back(specs[s].p1);
    }
  std::sort(taus.begin(), taus.end());
  taus.erase(std::unique(taus.begin(), taus.end()), taus.end());
  if ((int)taus.size() > kRifqMaxTaus)
    return fail(OB_E_UNSUPPORTED, "statistics refit: at most %d distinct quantiles over all ranges, got %d", kRifqMaxTaus,
                (int)taus.size());
  out.n_specs = n_specs;
  out.n_taus = (int)taus.size();
  for (size_t i = 0; i < taus.size(); ++i) out.taus[i] = taus[i];
  for (int s = 0; s < n_specs; ++s) {
    out.stat[s] = specs[s].stat;
    out.variance = out.variance || specs[s].stat == OB_RIF_VARIANCE;
    out.gini = out.gini || specs[s].stat == OB_RIF_GINI;
    if (specs[s].stat == OB_RIF_IQR) {
      out.range = true;
      out.hi[s] = (int)(std::lower_bound(taus.begin(), taus.end(), specs[s].p0) - taus.begin());
      out.lo[s] = (int)(std::lower_bound(taus.begin(), taus.end(), specs[s].p1) - taus.begin());
    }
  }
  return OB_OK;
}

int rifs_check_shape(int k, const ob_rif_spec* specs, int n_specs, int64_t n_a, int64_t n_b) {
  if (k < 1 || n_a < 0 || n_b < 0)
    return fail(OB_E_INVALID, "statistics refit: bad shape (k = %d, n_a = %lld, n_b = %lld)", k, (long long)n_a, (long long)n_b);
  if (k > kRifsMaxK)
    return fail(OB_E_UNSUPPORTED, "statistics refit: at most %d design columns with the intercept, got %d", kRifsMaxK, k);
  RifsPlan pl;
  OB_TRY(rifs_plan(specs, n_specs, pl));
  if (n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31))
    return fail(OB_E_UNSUPPORTED, "statistics refit: groups take fewer than 2^31 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k || n < 2)
      return fail(OB_E_INSUFFICIENT, "statistics refit: a group's rows (%lld) must exceed the design columns (%d) and be at least 2",
                  (long long)n, k);
  return OB_OK;
}

}  // namespace ob

extern "C" {

int ob_rifs_row_len(int32_t k, int32_t n_base) { return k < 1 || n_base < 0 ? 0 : ob_row_len(k, n_base) + 2; }

int ob_rifs_check_shape(int32_t k, const ob_rif_spec* specs, int32_t n_specs, int64_t n_a, int64_t n_b) {
  return ob::rifs_check_shape(k, specs, n_specs, n_a, n_b);
}

int ob_rifs_last_timing(ob_rifs_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

// The kernels over one group whose rows the caller sorted (include/oaxaca_boot.h).
int ob_rifs_pass(ob_ctx* ctx, const double* y_sorted, int64_t n, const uint8_t* counts, int32_t n_reps,
                 const ob_rif_spec* specs, int32_t n_specs, const double* x, int64_t ldx, int32_t p, double* nu,
                 double* gy, uint8_t* floored, uint8_t* ok) {
  if (!y_sorted || !nu || !gy) return ob::fail(OB_E_INVALID, "null pointer");
  if (p < 0 || (p > 0 && !x)) return ob::fail(OB_E_INVALID, "ob_rifs_pass: p = %d predictor columns need x", p);
  const int k = p + 1;
  if (k > ob::kRifsMaxK)
    return ob::fail(OB_E_UNSUPPORTED, "ob_rifs_pass: at most %d design columns with the intercept, got %d", ob::kRifsMaxK, k);
  ob::RifsPlan pl;
  OB_TRY(ob::rifs_plan(specs, n_specs, pl));
  if (n_reps > ob::kRifsMaxReps)
    return ob::fail(OB_E_UNSUPPORTED, "ob_rifs_pass takes at most %d replicates a call, got %d", ob::kRifsMaxReps, n_reps);
  if (n_reps < 1) return ob::fail(OB_E_INVALID, "ob_rifs_pass takes at least one replicate, got %d", n_reps);
  OB_TRY(ob::refit_pass_check("ob_rifs_pass", y_sorted, n, counts, n_reps, x, ldx, p, pl.gini));
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  ob::RefitPassInput in;
  OB_TRY(in.upload(y_sorted, n, counts, n_reps, x, ldx, k, s));
  const int S = n_specs;
  std::vector<uint32_t> runs;
  if (pl.gini) tie_runs(y_sorted, n, 0u, runs);
  DevBuf d_runs;
  OB_HIP(d_runs.alloc(sizeof(uint32_t) * runs.size()));
  if (!runs.empty()) OB_HIP(hipMemcpyAsync(d_runs.p, runs.data(), sizeof(uint32_t) * runs.size(), hipMemcpyHostToDevice, s));
  RifsArgs a{};
  ob::RifqArgs qa{};
  a.cols[0] = qa.cols[0] = in.cols.d();
  a.ld[0] = qa.ld[0] = in.ld;
  a.n[0] = qa.n[0] = (uint32_t)n;
  a.mu0[0] = qa.mu0[0] = in.mu0;
  qa.npow[0] = std::pow((double)n, -0.2);
  a.k = qa.k = k;
  a.n_groups = qa.n_groups = 1;
  qa.tiles_total = in.tiles;
  qa.m1 = counts ? in.m1.as<uint32_t>() : nullptr;
  a.counts = qa.counts = counts ? in.counts.as<uint32_t>() : nullptr;
  a.nb_rep = qa.nb_rep = in.nb_rep;
  a.part_pad = qa.part_pad = in.rep_pad;
  a.n_reps = qa.n_reps = (uint32_t)n_reps;
  a.chunks = qa.chunks = in.chunks.as<uint32_t>();
  a.n_chunks = qa.n_chunks = (int)in.n_chunks;
  a.runs = d_runs.as<uint32_t>();
  a.n_runs = (int)(runs.size() / 3);
  g_timing = {};
  RifsWork w;
  Events<11> ev;
  OB_HIP(ev.create());
  OB_TRY(rifs_launch(a, qa, pl, w, s, ev.e));
  OB_HIP(hipEventSynchronize(ev.e[6]));
  OB_TRY(rifs_times(ev.e, pl));
  // the device rows are [rep][1][S]: the caller's layout
  const size_t nrs = (size_t)n_reps * S;
  std::vector<uint8_t> fl(nrs), okh(nrs);
  OB_HIP(hipMemcpyAsync(nu, w.nu.p, sizeof(double) * nrs, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(gy, w.gy.p, sizeof(double) * nrs * (k + 1), hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(fl.data(), w.fl.p, nrs, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(okh.data(), w.sok.p, nrs, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  if (floored) std::memcpy(floored, fl.data(), nrs);
  if (ok) std::memcpy(ok, okh.data(), nrs);
  return OB_OK;
}

}  // extern "C"

namespace ob {

// Device side of a prepared refit run. The handle's ob_panel holds the groups' rows in stable ascending order of y
// (x_1 .. x_p, then y): it is the resampler and the owner of the Gram, the chunk table and the solve.
struct RifsState {
  int k = 0;
  RifsPlan plan;
  std::vector<ob_rif_spec> specs;
  DevBuf cols[2];  // [y | x_1 .. x_{k-1}] x ld
  DevBuf runs, solved, sok;
  int n_runs = 0;
  RifsWork work;
  SortedGroups sorted;           // perm, mu0, npow (x and y are dropped once uploaded)
  std::vector<double> point_nu;  // [2][S]
  int64_t n_floored = 0;         // floored densities of the point pass and of every boot since
};

static RifsState* rifs_state(const ob_prepared* pr) { return model_state<RifsState>(pr, kModelRifs); }

// One segment (refit_segment) with the plan's kernels and rifs_tail_kernel.
static int rifs_segment(ob_prepared* pr, const RefitSegment& sg, hipStream_t s) {
  RifsState* st = rifs_state(pr);
  ob_panel* p = pr->panel;
  const int k = st->k, rl0 = p->row_len;
  Events<11> ev;  // rifs_launch's
  OB_HIP(ev.create());
  RifsArgs a{};
  RefitModel md{st->plan.n_specs, &st->solved, &st->sok, &st->n_floored, nullptr, nullptr};
  md.launch = [&](uint32_t nb_rep, uint32_t rep_pad, RefitOut* out) -> int {
    RifqArgs qa{};
    for (int g = 0; g < 2; ++g) {
      a.cols[g] = qa.cols[g] = st->cols[g].d();
      a.ld[g] = qa.ld[g] = p->ld[g];
      a.n[g] = qa.n[g] = p->n[g];
      a.mu0[g] = qa.mu0[g] = st->sorted.mu0[g];
      qa.npow[g] = st->sorted.npow[g];
    }
    a.tile0[1] = qa.tile0[1] = p->ntiles[0];
    a.k = qa.k = k;
    a.n_groups = qa.n_groups = 2;
    qa.tiles_total = p->ntiles[0] + p->ntiles[1];
    qa.m1 = p->d_m1;
    a.counts = qa.counts = p->d_counts;
    a.nb_rep = qa.nb_rep = nb_rep;
    a.part_pad = qa.part_pad = rep_pad;
    a.n_reps = qa.n_reps = sg.ns;
    a.chunks = qa.chunks = p->d_chunks;
    a.n_chunks = qa.n_chunks = (int)(p->chunks.size() / 3);
    a.runs = st->runs.as<uint32_t>();
    a.n_runs = st->n_runs;
    OB_TRY(rifs_launch(a, qa, st->plan, st->work, s, ev.e));
    *out = {a.gy, a.fl};
    return OB_OK;
  };
  md.tail = [&](int t, const double* solved, const uint8_t* sok, double* rows, uint8_t* ok) {
    hipLaunchKernelGGL(rifs_tail_kernel, dim3(sg.ns), dim3(64), 0, s, a, t, solved, sok, rl0, rows, ok);
  };
  RefitTimes tm;
  OB_TRY(refit_segment(pr, sg, md, s, &tm));
  g_timing.gram_ms += tm.gram_ms;
  g_timing.solve_ms += tm.solve_ms;
  return rifs_times(ev.e, st->plan);
}

static int rifs_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                            hipStream_t stream) {
  const BootPlan plan{kRefitSegReps, kCountBudget, false, [](uint32_t) {
                        g_timing = {};
                        return OB_OK;
                      }};
  return boot_segmented(pr, kModelRifs, plan, first_rep, n_reps, d_rows && d_ok, stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t, uint32_t, hipStream_t s) {
                          return rifs_segment(pr, {false, first_rep + s0, ns, n_reps, s0, d_rows, d_ok}, s);
                        });
}

static const bool g_rifs_hooks_installed = model_install(
    kModelRifs, {rifs_boot_device, model_boot_host, [](void* s) { delete static_cast<RifsState*>(s); }});

// Every check of the frame entry points, before any device work and before the context is read.
static int rifs_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                      const ob_rif_spec* specs, int32_t n_specs, Config& c, RifsPlan& pl, Matrices& m) {
  OB_TRY(config_from(cfg, c));
  OB_TRY(rifs_plan(specs, n_specs, pl));
  if (c.has_weights) return model_refuse(kModelRifs, "sample weights are");
  if (!c.normalize.empty()) return model_refuse(kModelRifs, "normalized categoricals are");
  if (c.has_selection || !c.selection_predictors.empty()) return model_refuse(kModelRifs, "Heckman selection settings are");
  if (c.has_cluster) return model_refuse(kModelRifs, "a cluster bootstrap is");
  OB_TRY(stage_named(cols, n_cols, n_rows, c, kModelRifs, false, false));
  OB_TRY(m.load(cols, n_cols, n_rows, cfg, false));
  OB_TRY(rifs_check_shape(m.k, specs, n_specs, m.n[0], m.n[1]));
  for (int g = 0; g < 2; ++g) {
    bool positive = false;
    for (int64_t i = 0; i < m.n[g]; ++i) {
      const double y = m.y[g][i];
      if (!std::isfinite(y)) return fail(OB_E_INVALID, "statistics refit: a non-finite value in the outcome");
      if (pl.gini && y < 0.0) return fail(OB_E_INVALID, "statistics refit: the Gini takes no negative outcome");
      positive = positive || y > 0.0;
    }
    if (pl.gini && !positive) return fail(OB_E_INVALID, "statistics refit: the Gini needs a positive outcome in each group");
    for (int64_t i = 0; i < m.n[g] * m.k; ++i)
      if (!std::isfinite(m.x[g][i])) return fail(OB_E_INVALID, "statistics refit: a non-finite value in a predictor");
  }
  return OB_OK;
}

static int rifs_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                        const ob_rif_spec* specs, int32_t n_specs, ob_prepared** out) {
  Config c;
  RifsPlan pl;
  Matrices m;
  OB_TRY(rifs_stage(cols, n_cols, n_rows, cfg, specs, n_specs, c, pl, m));
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  const int k = m.k;
  RifsState* st = new RifsState();
  ob_prepared* pr = model_handle(ctx, c, m, kModelRifs, st, ob_row_len(k, 0) + 2, n_specs);
  st->k = k;
  st->plan = pl;
  st->specs.assign(specs, specs + n_specs);
  SortedGroups& sg = st->sorted;
  sort_groups(m, sg);
  std::vector<uint32_t> runs;
  for (int g = 0; g < 2 && pl.gini; ++g) tie_runs(sg.y[g].data(), m.n[g], (uint32_t)g, runs);
  st->n_runs = (int)(runs.size() / 3);
  auto build = [&]() -> int {
    OB_TRY(refit_panel(ctx, c, m, sg, &pr->panel));
    for (int g = 0; g < 2; ++g)
      OB_TRY(upload_group(st->cols[g], pr->panel->ld[g], m.n[g], k, 0, sg.y[g].data(), sg.x[g].data()));
    OB_HIP(st->runs.alloc(sizeof(uint32_t) * runs.size()));
    if (!runs.empty()) OB_HIP(hipMemcpy(st->runs.p, runs.data(), sizeof(uint32_t) * runs.size(), hipMemcpyHostToDevice));
    // the point pass: the boot's own kernels over unit counts
    g_timing = {};
    OB_TRY(refit_point(pr, [&](double* d_rows, uint8_t* d_ok, hipStream_t s) {
      return rifs_segment(pr, {true, 0, 1, 1, 0, d_rows, d_ok}, s);
    }));
    const size_t S = (size_t)n_specs;
    const int rl0 = pr->row_len - 2;
    st->point_nu.resize(2 * S);
    for (size_t t = 0; t < S; ++t)
      for (int g = 0; g < 2; ++g) st->point_nu[(size_t)g * S + t] = pr->point_row[t * pr->row_len + rl0 + g];
    return OB_OK;
  };
  const int rc = build();
  for (int g = 0; g < 2; ++g) {
    sg.x[g] = {};
    sg.y[g] = {};
  }
  return model_built(pr, rc, out);
}

}  // namespace ob

extern "C" {

int ob_builder_prepare_statistics_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                        const ob_builder_config* cfg, const ob_rif_spec* specs, int32_t n_specs,
                                        ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::rifs_prepare(ctx, cols, n_cols, n_rows, cfg, specs, n_specs, out);
}

int ob_builder_decompose_statistics_refit(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                                          const ob_builder_config* cfg, const ob_rif_spec* specs, int32_t n_specs,
                                          ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  for (int32_t t = 0; t < std::max(n_specs, 0) && t < ob::kRifsMaxStats; ++t) out[t] = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::rifs_prepare(ctx, cols, n_cols, n_rows, cfg, specs, n_specs, &pr));
  const uint64_t reps = pr->cfg.reps;
  const size_t S = (size_t)n_specs;
  std::vector<double> rows(S * reps * pr->row_len);
  std::vector<uint8_t> ok(S * reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  for (size_t t = 0; t < S && rc == OB_OK; ++t)
    rc = ob::finish(pr, (int)t, rows.data() + t * reps * pr->row_len, ok.data() + t * reps, reps, &out[t]);
  if (rc != OB_OK)
    for (size_t t = 0; t < S; ++t) {
      ob_results_free(out[t]);
      out[t] = nullptr;
    }
  ob_prepared_destroy(pr);
  return rc;
}

int ob_prepared_rifs_info(const ob_prepared* prep, ob_rifs_info* out) {
  if (!prep || !out) return ob::fail(OB_E_INVALID, "null pointer");
  const ob::RifsState* st = ob::rifs_state(prep);
  if (!st) return ob::fail(OB_E_INVALID, "the handle was not prepared for a statistics refit");
  *out = {st->plan.n_specs, st->k, prep->n_a, prep->n_b, st->n_floored, st->specs.data(), st->sorted.perm[0].data(),
          st->sorted.perm[1].data(), st->point_nu.data()};
  return OB_OK;
}

}  // extern "C"
