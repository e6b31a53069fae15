// ob_binary.hip -- the bootstrapped probit Oaxaca-Blinder decomposition of a 0/1 outcome (Fairlie 1999,
// Yun 2004, Bauer-Sinning 2008). No counterpart in the reference crate.
//
// Per replicate (the resample enters through the engine's level-2 count images, as in ob_heckman.hip):
//   probit of y on X = [1, x] in each group: ob::probit_stage, the Heckman path's Fisher scoring;
//   ob_binary_bstar_kernel   thread per replicate: beta_A, beta_B and beta* (ref_mode) side by side;
//   ob_binary_means_kernel   block per (row chunk, 16 replicates): sum c Phi(x'beta) for the three
//                            vectors, sum c y, sum c, sum c x_j -- the six counterfactual mean
//                            probabilities and the count-weighted covariate means of the replicate;
//   ob_binary_row_kernel     wave per replicate: chunk partials in chunk order, the two-fold and
//                            three-fold terms, Yun's detailed terms, the row.
// The point pass is the same code with every row counted once (counts == NULL).
//
// Panel of a binary run, per group [col][ld]: y | x_1 .. x_{K-1} -- the probit kernels' s | z layout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ob_binary.hpp"
#include "ob_builder.hpp"
#include "ob_engine.hpp"
#include "ob_heckman.hpp"
#include "ob_hip.hpp"
#include "ob_model.hpp"
#include "ob_normal.hpp"
#include "ob_options.hpp"
#include "ob_spec.h"

namespace {

constexpr int kBB = 256;     // threads of a means block
constexpr int kBS = 65;      // doubles per staged column (as ob_heck_wide_kernel)
constexpr int kBReps = 16;   // replicates per means block
constexpr int kBVals = 40;   // per-thread sums, padded to whole rounds of kBRound
constexpr int kBRound = 8;   // sums reduced per round of the block's final ordered sum

// betas [replicate][3][k]: beta_A, beta_B, beta*. Weighted / Cotton: the row-share average of
// ob_solve_kernel (wA = n_A / (n_A + n_B), wB = 1 - wA; a group's resample keeps its row count).
__global__ __launch_bounds__(64) void ob_binary_bstar_kernel(const ob_heck_seg a, double* betas) {
  const uint32_t rep = blockIdx.x * 64 + threadIdx.x;
  if (rep >= a.n_reps) return;
  const int k = a.ks;
  const double* ga = a.gamma + (size_t)rep * k;
  const double* gb = a.gamma + ((size_t)a.rep_pad + rep) * k;
  double* out = betas + (size_t)rep * 3 * k;
  const double sa = (double)a.n[0], sb = (double)a.n[1];
  const double wA = sa / (sa + sb), wB = 1.0 - wA;
  for (int j = 0; j < k; ++j) {
    const double ba = ga[j], bb = gb[j];
    out[j] = ba;
    out[k + j] = bb;
    out[2 * k + j] = a.ref_mode == OB_REF_GROUP_A ? ba : (a.ref_mode == OB_REF_GROUP_B ? bb : ba * wA + bb * wB);
  }
}

// Block = (row chunk, 16 replicates), 4 waves; thread = (replicate t & 15, rows 4 (t >> 4) .. + 3 of
// each 64-row sub-tile: one count word). Per sub-tile the block stages the K columns once (coalesced,
// LDS [col][65]); a thread forms its four rows' three indices from the staged columns and its
// replicate's coefficients (LDS [replicate][vector][K | 1]), applies Phi to the counted rows and adds
// c Phi, c y, c and c x_j into registers. A thread owns its rows over the whole chunk; at the end the
// 16 row groups of a replicate are added in row-group order through LDS. So a replicate's partials
// depend on the chunk and on the replicate alone: not on its slot in the block, its neighbours, the
// batch or first_rep. No atomics.
template <bool CODY>
__global__ __launch_bounds__(kBB) void ob_binary_means_kernel(const ob_heck_seg a, const double* betas) {
  extern __shared__ __attribute__((aligned(16))) double bsm[];
  const int tid = threadIdx.x;
  const uint32_t chunk = blockIdx.x, g = a.chunks[3 * chunk], t0 = a.chunks[3 * chunk + 1], t1 = a.chunks[3 * chunk + 2];
  const int k = a.ks, gs = k | 1, nv = ob::binary_sums_len(k);
  double* stg = bsm;                  // [k][kBS]: y, x_1 .. x_{k-1}
  double* bt = stg + k * kBS;         // [16][3][gs]
  double* red = bt + kBReps * 3 * gs;  // [kBRound][16 row groups][16 replicates]
  const int r16 = tid & 15, q = tid >> 4;
  const uint32_t rep0 = blockIdx.y * kBReps, rep = rep0 + r16;
  const bool act = rep < a.n_reps;
  for (int i = tid; i < kBReps * 3 * k; i += kBB) {
    const int rr = i / (3 * k), rem = i - rr * 3 * k, v = rem / k, j = rem - v * k;
    bt[(rr * 3 + v) * gs + j] = rep0 + rr < a.n_reps ? betas[((size_t)(rep0 + rr) * 3 + v) * k + j] : 0.0;
  }
  double acc[3] = {0.0, 0.0, 0.0}, sy = 0.0, sc = 0.0;
  double xs[ob::kBinaryMaxK - 1];
#pragma unroll
  for (int j = 0; j < ob::kBinaryMaxK - 1; ++j) xs[j] = 0.0;
  const double* X = a.cols[g];
  const int64_t ld = a.ld[g];
  const uint32_t n = a.n[g];
  const uint32_t rb = rep >> 6, R = rep & 63;
  const double* b0 = bt + (r16 * 3 + 0) * gs;
  const double* b1 = bt + (r16 * 3 + 1) * gs;
  const double* b2 = bt + (r16 * 3 + 2) * gs;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    for (uint32_t sw = 0; sw < 4; ++sw) {
      const uint32_t r0 = tile * OB_TILE_ROWS + sw * 64;
      if (r0 >= n) break;
      const uint32_t nr = min(64u, n - r0);
      __syncthreads();  // the previous sub-tile's reads (and the coefficient loads)
      for (int i = tid; i < k * 64; i += kBB) {
        const int c = i >> 6, r = i & 63;
        stg[c * kBS + r] = (uint32_t)r < nr ? X[(size_t)c * ld + r0 + r] : 0.0;
      }
      __syncthreads();
      uint32_t word = 0;  // counts of rows 4 q .. 4 q + 3 (the two image layouts of ob_heckman.hip)
      if (act) {
        const size_t tt = (g ? a.tiles0 : 0u) + tile;
        if (!a.counts)
          word = 0x01010101u;
        else if (a.counts_i8)
          word = a.counts[((tt * a.nb_rep + rb) * 1024 + sw * 256 + (R >> 4) * 64 + (R & 15)) * 4 + (q >> 2) * 64 + (q & 3)];
        else
          word = a.counts[((tt * a.nb_rep + rb) * 4 + sw) * kCimgWords + R * kCimgStride + q];
      }
      double cd[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) cd[i] = (uint32_t)(4 * q + i) < nr ? (double)((word >> (8 * i)) & 255u) : 0.0;
      if (cd[0] + cd[1] + cd[2] + cd[3] == 0.0) continue;  // (uniform control flow resumes at the barrier)
      double zg[3][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        zg[0][i] = b0[0];
        zg[1][i] = b1[0];
        zg[2][i] = b2[0];
      }
#pragma unroll
      for (int j = 1; j < ob::kBinaryMaxK; ++j)
        if (j < k) {
          const double* zj = stg + j * kBS + 4 * q;
          const double g0 = b0[j], g1 = b1[j], g2 = b2[j];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double z = zj[i];
            zg[0][i] += z * g0;
            zg[1][i] += z * g1;
            zg[2][i] += z * g2;
            xs[j - 1] += cd[i] * z;
          }
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (cd[i] == 0.0) continue;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          double ph;
          if constexpr (CODY) {
            double pd;
            npdf_ncdf(zg[v][i], pd, ph);
          } else {
            ph = ncdf(zg[v][i]);
          }
          acc[v] += cd[i] * ph;
        }
        sy += cd[i] * stg[4 * q + i];
        sc += cd[i];
      }
    }
  }
  // slots: [0, 3) c Phi, [3] c y, [4] c, [5] c x_0 = c, [6 ..) c x_j
  double vals[kBVals];
#pragma unroll
  for (int i = 0; i < kBVals; ++i) vals[i] = 0.0;
  vals[0] = acc[0];
  vals[1] = acc[1];
  vals[2] = acc[2];
  vals[3] = sy;
  vals[4] = sc;
  vals[5] = sc;
#pragma unroll
  for (int j = 0; j < ob::kBinaryMaxK - 1; ++j) vals[6 + j] = xs[j];
  double* out = a.partial + (size_t)chunk * a.part_pad * nv;
#pragma unroll
  for (int rd = 0; rd < kBVals / kBRound; ++rd) {
    if (rd * kBRound >= nv) break;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kBRound; ++i) red[(i * 16 + q) * kBReps + r16] = vals[rd * kBRound + i];
    __syncthreads();
    if (tid < kBRound * kBReps) {
      const int vi = tid >> 4, slot = rd * kBRound + vi;
      double v = 0.0;
      for (int qq = 0; qq < 16; ++qq) v += red[(vi * 16 + qq) * kBReps + r16];
      if (slot < nv && act) out[(size_t)rep * nv + slot] = v;
    }
  }
}

inline size_t means_lds(int k) {
  return sizeof(double) * ((size_t)k * kBS + (size_t)kBReps * 3 * (k | 1) + (size_t)kBRound * 16 * kBReps);
}

// One wave per replicate: the chunk partials of both groups in chunk order, then the terms of
// include/oaxaca_boot.h's binary row. A replicate whose probit failed in either group (the Hessian
// could not be solved) gets ok = 0 and a NaN row.
__global__ __launch_bounds__(64) void ob_binary_row_kernel(const ob_heck_seg a, const double* betas) {
  __shared__ double S[2 * (5 + ob::kBinaryMaxK)];
  __shared__ double den[3];
  const int lane = threadIdx.x, k = a.ks, nv = ob::binary_sums_len(k);
  const uint32_t rep = blockIdx.x;
  if (rep >= a.n_reps) return;
  for (int i = lane; i < 2 * nv; i += 64) {
    const uint32_t g = (uint32_t)(i / nv);
    const int j = i - (int)g * nv;
    double v = 0.0;
    for (int c = 0; c < a.n_chunks; ++c)
      if (a.chunks[3 * c] == g) v += a.partial[((size_t)c * a.part_pad + rep) * nv + j];
    S[i] = v;
  }
  __syncthreads();
  double* row = a.rows + (size_t)rep * a.row_len;
  const bool failed = ((a.hflags[rep] | a.hflags[(size_t)a.rep_pad + rep]) & ob::kProbitFailed) != 0;
  if (failed) {
    for (int i = lane; i < a.row_len; i += 64) row[i] = __builtin_nan("");
    if (lane == 0) a.ok[rep] = 0;
    return;
  }
  const double* SA = S;
  const double* SB = S + nv;
  const double na = SA[4], nb = SB[4];
  const double* ba = betas + (size_t)rep * 3 * k;
  const double* bb = ba + k;
  const double* bs = bb + k;
  const double paa = SA[0] / na, pab = SA[1] / na, pas = SA[2] / na;  // P(A, beta_A), P(A, beta_B), P(A, beta*)
  const double pba = SB[0] / nb, pbb = SB[1] / nb, pbs = SB[2] / nb;
  const double total = paa - pbb, expl = pas - pbs;
  const double ua = paa - pas, ub = pbs - pbb;
  if (lane == 0) {  // Yun's denominators, in column order
    double de = 0.0, da = 0.0, db = 0.0;
    for (int j = 0; j < k; ++j) {
      const double xa = SA[5 + j] / na, xb = SB[5 + j] / nb;
      de += (xa - xb) * bs[j];
      da += xa * (ba[j] - bs[j]);
      db += xb * (bs[j] - bb[j]);
    }
    den[0] = de;
    den[1] = da;
    den[2] = db;
  }
  __syncthreads();
  const double de = den[0], da = den[1], db = den[2];
  double* tail = row + 6 + 2 * k;
  for (int j = lane; j < k; j += 64) {
    const double xa = SA[5 + j] / na, xb = SB[5 + j] / nb;
    // a part whose denominator is exactly 0 contributes 0.0 (U_A under GroupA, U_B under GroupB)
    const double te = de == 0.0 ? 0.0 : expl * ((xa - xb) * bs[j]) / de;
    const double ta = da == 0.0 ? 0.0 : ua * (xa * (ba[j] - bs[j])) / da;
    const double tb = db == 0.0 ? 0.0 : ub * (xb * (bs[j] - bb[j])) / db;
    row[6 + j] = te;
    row[6 + k + j] = ta + tb;
    tail[j] = ba[j];
    tail[k + j] = bb[j];
    tail[2 * k + j] = xa;
    tail[3 * k + j] = xb;
    tail[4 * k + j] = bs[j];
  }
  if (lane == 0) {
    const double endow = pab - pbb, coef = pba - pbb;
    row[0] = expl;
    row[1] = total - expl;
    row[2] = endow;
    row[3] = coef;
    row[4] = total - endow - coef;
    row[5] = total;
    double* pr = tail + 5 * k;
    pr[0] = paa;
    pr[1] = pab;
    pr[2] = pas;
    pr[3] = pba;
    pr[4] = pbb;
    pr[5] = pbs;
    pr[6] = SA[3] / na;
    pr[7] = SB[3] / nb;
    a.ok[rep] = 1;
  }
}

hipError_t launch_means(const ob_heck_seg& a, const double* betas, hipStream_t s) {
  const bool cody = ob::opt_int(ob::Opt::HkErfc, 1) != 0;  // the Phi the probit used
  const void* fn = cody ? (const void*)ob_binary_means_kernel<true> : (const void*)ob_binary_means_kernel<false>;
  const size_t lds = means_lds(a.ks);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  ob_heck_seg arg = a;
  void* args[] = {&arg, &betas};
  e = hipLaunchKernel(fn, dim3(a.n_chunks, (a.n_reps + kBReps - 1) / kBReps), dim3(kBB), args, lds, s);
  return e != hipSuccess ? e : hipGetLastError();
}

thread_local ob_binary_timing g_timing = {};

// The three stages over one batch of a segment (or the point pass): probit, beta*, means, rows.
int binary_batch(const ob_heck_seg& a, double* betas, hipStream_t s) {
  if (a.ks < 1 || a.ks > ob::kBinaryMaxK) return ob::fail(OB_E_INVALID, "binary segment: bad shape");
  Events<3> ev;
  OB_HIP(ev.create());
  int it = 0;
  ob::ob_heck_times ht;
  OB_TRY(ob::probit_stage(a, s, &it, &ht));
  hipLaunchKernelGGL(ob_binary_bstar_kernel, dim3((a.n_reps + 63) / 64), dim3(64), 0, s, a, betas);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[0], s));
  OB_HIP(launch_means(a, betas, s));
  OB_HIP(hipEventRecord(ev.e[1], s));
  hipLaunchKernelGGL(ob_binary_row_kernel, dim3(a.n_reps), dim3(64), 0, s, a, (const double*)betas);
  OB_HIP(hipGetLastError());
  OB_HIP(hipEventRecord(ev.e[2], s));
  OB_HIP(hipEventSynchronize(ev.e[2]));
  float m0 = 0.f, m1 = 0.f;
  OB_HIP(hipEventElapsedTime(&m0, ev.e[0], ev.e[1]));
  OB_HIP(hipEventElapsedTime(&m1, ev.e[1], ev.e[2]));
  g_timing.probit_ms += ht.probit_ms;
  g_timing.probit_launches += ht.probit_launches;
  g_timing.probit_iterations = std::max(g_timing.probit_iterations, (int32_t)it);
  g_timing.means_ms += m0;
  g_timing.epilogue_ms += m1;
  return OB_OK;
}

size_t partial_vals(int k) { return std::max<size_t>(ob::heck_probit_len(k), ob::binary_sums_len(k)); }

}  // namespace

namespace ob {

int binary_check_shape(int k, int64_t n_a, int64_t n_b) {
  if (k < 1 || n_a < 0 || n_b < 0)
    return fail(OB_E_INVALID, "binary decomposition: bad shape (k = %d, n_a = %lld, n_b = %lld)", k, (long long)n_a,
                (long long)n_b);
  if (k > kBinaryMaxK)
    return fail(OB_E_UNSUPPORTED, "binary decomposition: at most %d design columns with the intercept, got %d",
                kBinaryMaxK, k);
  if (n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31))
    return fail(OB_E_UNSUPPORTED, "binary decomposition: groups take fewer than 2^31 rows");
  for (int64_t n : {n_a, n_b})
    if (n <= (int64_t)k)
      return fail(OB_E_INSUFFICIENT, "%sbinary decomposition: a group's rows (%lld) must exceed the design columns (%d)",
                  error_prefix(OB_E_INSUFFICIENT), (long long)n, k);
  return OB_OK;
}

// Device side of a prepared binary run. The handle's ob_panel (no predictors, the outcome alone) is
// the resampler: engine_counts draws a segment's count images for its row counts, and its chunk
// table is the one the passes walk.
struct BinaryState {
  int k = 0;
  DevBuf cols[2];  // [y | x_1 .. x_{k-1}] x ld
  DevBuf chunks, gamma, flags, partial, betas;
  int n_chunks = 0;
};

static BinaryState* binary_state(const ob_prepared* pr) { return model_state<BinaryState>(pr, kModelBinary); }

static ob_heck_seg binary_seg(const ob_prepared* pr, const BinaryState* st) {
  const ob_panel* p = pr->panel;
  ob_heck_seg h{};
  for (int g = 0; g < 2; ++g) {
    h.cols[g] = st->cols[g].d();
    h.ld[g] = p->ld[g];
    h.n[g] = p->n[g];
  }
  h.tiles0 = p->ntiles[0];
  h.p = st->k - 1;
  h.ks = st->k;
  h.sz_col = 0;
  h.chunks = st->chunks.as<uint32_t>();
  h.n_chunks = st->n_chunks;
  h.ref_mode = pr->ref;
  h.row_len = pr->row_len;
  h.max_iter = 100;
  h.tol = 1e-6;
  return h;
}

// Workspace for segments of rep_pad replicates run in batches of hb.
static int binary_ensure(BinaryState* st, uint32_t rep_pad, uint32_t hb) {
  OB_HIP(st->gamma.alloc(sizeof(double) * 2 * rep_pad * st->k));
  OB_HIP(st->flags.alloc(sizeof(uint32_t) * (2 * (size_t)rep_pad + 1)));
  OB_HIP(st->betas.alloc(sizeof(double) * 3 * (size_t)rep_pad * st->k));
  OB_HIP(st->partial.alloc(sizeof(double) * (size_t)st->n_chunks * hb * partial_vals(st->k)));
  return OB_OK;
}

// Replicates per batch: the register-resident probit kernels (k <= 8) take a segment whole (their
// partials are [chunk][rep_pad]); the wide ones run boot_batch_reps' batches. Rows do not depend on it.
static uint32_t binary_batch_reps(const BinaryState* st, uint32_t rep_pad) {
  if (st->k <= kHeckMaxKs) return rep_pad;
  return boot_batch_reps((size_t)st->n_chunks * partial_vals(st->k) * sizeof(double), rep_pad);
}

static int binary_point(ob_prepared* pr, BinaryState* st) {
  ob_panel* p = pr->panel;
  OB_HIP(hipSetDevice(p->ctx->device));
  hipStream_t s = p->ctx->stream;
  OB_TRY(binary_ensure(st, 64, 64));
  DevBuf d_row, d_ok;
  OB_HIP(d_row.alloc(sizeof(double) * pr->row_len));
  OB_HIP(d_ok.alloc(1));
  ob_heck_seg h = binary_seg(pr, st);
  h.counts = nullptr;
  h.nb_rep = 1;
  h.rep_pad = 64;
  h.part_pad = 64;
  h.n_reps = 1;
  h.gamma = st->gamma.d();
  h.hflags = st->flags.as<uint32_t>();
  h.active = h.hflags + 2 * 64;
  h.partial = st->partial.d();
  h.rows = d_row.d();
  h.ok = d_ok.as<uint8_t>();
  OB_TRY(binary_batch(h, st->betas.d(), s));
  uint8_t okh = 0;
  pr->point_row.assign((size_t)pr->row_len, 0.0);
  OB_HIP(hipMemcpyAsync(pr->point_row.data(), d_row.p, sizeof(double) * pr->row_len, hipMemcpyDeviceToHost, s));
  OB_HIP(hipMemcpyAsync(&okh, d_ok.p, 1, hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  if (!okh) return fail(OB_E_LINALG, "%sFailed to solve Hessian system in Probit", error_prefix(OB_E_LINALG));
  return OB_OK;
}

static int binary_boot_device(ob_prepared* pr, uint64_t first_rep, uint64_t n_reps, double* d_rows, uint8_t* d_ok,
                              hipStream_t stream) {
  BinaryState* st = binary_state(pr);
  ob_panel* p = pr ? pr->panel : nullptr;
  uint32_t seg_pad = 0;  // the flags are laid out for the longest segment (binary alone keeps per-segment flags)
  const BootPlan plan{kFitSegReps, kCountBudget, true, [&](uint32_t pad) {
                        g_timing = {};
                        seg_pad = pad;
                        return binary_ensure(st, pad, binary_batch_reps(st, pad));
                      }};
  return boot_segmented(pr, kModelBinary, plan, first_rep, n_reps, d_rows && d_ok, stream,
                        [&](uint64_t s0, uint32_t ns, uint32_t nb_rep, uint32_t rep_pad, hipStream_t s) {
    ob_heck_seg hs = binary_seg(pr, st);
    hs.counts = p->d_counts;
    hs.counts_i8 = 0;
    hs.nb_rep = nb_rep;
    hs.rep_pad = rep_pad;
    hs.active = st->flags.as<uint32_t>() + 2 * (size_t)seg_pad;
    hs.partial = st->partial.d();
    const uint32_t hb = binary_batch_reps(st, rep_pad);
    return boot_batches(ns, hb, [&](uint32_t b0, uint32_t nb) {  // every per-replicate base moved to b0
      ob_heck_seg hb_seg = hs;
      hb_seg.n_reps = nb;
      hb_seg.part_pad = hb;
      hb_seg.counts = hs.counts + (size_t)(b0 / 64) * 4 * kCimgWords;
      hb_seg.gamma = st->gamma.d() + (size_t)b0 * st->k;
      hb_seg.hflags = st->flags.as<uint32_t>() + b0;
      hb_seg.rows = d_rows + (s0 + b0) * pr->row_len;
      hb_seg.ok = d_ok + s0 + b0;
      return binary_batch(hb_seg, st->betas.d() + (size_t)b0 * 3 * st->k, s);
    });
  });
}

// installs the builder's hooks when the library loads (ob_model.hpp)
static const bool g_binary_hooks_installed = model_install(
    kModelBinary, {binary_boot_device, model_boot_host, [](void* s) { delete static_cast<BinaryState*>(s); }});

// Every check of the frame entry points, before any device work and before the context is read:
// settings outside the scope, nulls in named columns, the design (ob::data_matrices), the
// outcome's values, the shape. On success m holds the design matrices.
static int binary_stage(const ob_column* cols, int32_t n_cols, int64_t n_rows, const ob_builder_config* cfg,
                        int32_t model, Config& c, Matrices& m) {
  OB_TRY(config_from(cfg, c));
  if (model == OB_BINARY_LOGIT)
    return fail(OB_E_UNSUPPORTED, "binary decomposition: the logit link is outside the engine's scope (the "
                                  "per-replicate fit kernels are probit's)");
  if (model != OB_BINARY_PROBIT) return fail(OB_E_INVALID, "binary decomposition: unknown model %d", model);
  if (c.has_weights) return model_refuse(kModelBinary, "sample weights are");
  if (!c.normalize.empty()) return model_refuse(kModelBinary, "normalized categoricals are");
  if (c.has_selection || !c.selection_predictors.empty()) return model_refuse(kModelBinary, "Heckman selection settings are");
  if (c.ref == OB_REF_POOLED || c.ref == OB_REF_NEUMARK)
    return model_refuse(kModelBinary, "pooled reference coefficients need a third, stacked probit and are");
  OB_TRY(stage_named(cols, n_cols, n_rows, c, kModelBinary, false, false));
  OB_TRY(m.load(cols, n_cols, n_rows, cfg, false));
  if (m.k > kBinaryMaxK) OB_TRY(binary_check_shape(m.k, m.n[0], m.n[1]));
  for (int g = 0; g < 2; ++g) {
    const int64_t n = m.n[g];
    int64_t ones = 0;
    for (int64_t i = 0; i < n; ++i) {
      const double y = m.y[g][i];
      if (y != 0.0 && y != 1.0) return fail(OB_E_INVALID, "binary decomposition: the outcome must be exactly 0.0 or 1.0, got %g", y);
      ones += y == 1.0 ? 1 : 0;
    }
    if (n == 0) return fail(OB_E_GROUP, "%sOne group has no data", error_prefix(OB_E_GROUP));
    if (ones == 0 || ones == n)
      return fail(OB_E_INVALID, "binary decomposition: the outcome of group %c is constant", g ? 'B' : 'A');
  }
  return binary_check_shape(m.k, m.n[0], m.n[1]);
}

static int binary_prepare(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                          const ob_builder_config* cfg, int32_t model, ob_prepared** out) {
  Config c;
  Matrices m;
  OB_TRY(binary_stage(cols, n_cols, n_rows, cfg, model, c, m));
  if (!ctx) return fail(OB_E_INVALID, "null pointer: ctx");
  BinaryState* st = new BinaryState();
  st->k = m.k;
  ob_prepared* pr = model_handle(ctx, c, m, kModelBinary, st, binary_row_len(m.k), 1);
  auto build = [&]() -> int {
    OB_TRY(outcome_panel(ctx, m, &pr->panel));
    for (int g = 0; g < 2; ++g) OB_TRY(upload_group(st->cols[g], pr->panel->ld[g], m.n[g], m.k, 0, m.y[g], m.x[g]));
    OB_TRY(upload_chunks(pr->panel, st->chunks, &st->n_chunks));
    g_timing = {};
    return binary_point(pr, st);
  };
  return model_built(pr, build(), out);
}

}  // namespace ob

extern "C" {

int ob_binary_row_len(int32_t k) { return k < 1 ? 0 : ob::binary_row_len(k); }

int ob_binary_check_shape(int32_t k, int64_t n_a, int64_t n_b) { return ob::binary_check_shape(k, n_a, n_b); }

int ob_binary_last_timing(ob_binary_timing* out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = g_timing;
  return OB_OK;
}

int ob_prepared_point_row(const ob_prepared* prep, const double** data, int64_t* len) {
  if (!prep || !data || !len) return ob::fail(OB_E_INVALID, "null pointer");
  *data = prep->point_row.data();
  *len = (int64_t)prep->point_row.size();
  return OB_OK;
}

int ob_builder_prepare_binary(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                              const ob_builder_config* cfg, int32_t model, ob_prepared** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  return ob::binary_prepare(ctx, cols, n_cols, n_rows, cfg, model, out);
}

int ob_builder_run_binary(ob_ctx* ctx, const ob_column* cols, int32_t n_cols, int64_t n_rows,
                          const ob_builder_config* cfg, int32_t model, ob_results** out) {
  if (!out) return ob::fail(OB_E_INVALID, "null pointer");
  *out = nullptr;
  ob_prepared* pr = nullptr;
  OB_TRY(ob::binary_prepare(ctx, cols, n_cols, n_rows, cfg, model, &pr));
  const uint64_t reps = pr->cfg.reps;
  std::vector<double> rows((size_t)reps * pr->row_len);
  std::vector<uint8_t> ok(reps, 0);
  int rc = OB_OK;
  if (reps > 0) rc = ob_prepared_boot(pr, 0, reps, rows.data(), ok.data());
  if (rc == OB_OK) rc = ob::finish(pr, 0, rows.data(), ok.data(), reps, out);
  ob_prepared_destroy(pr);
  return rc;
}

// The mean-probability pass alone (include/oaxaca_boot.h): one group, one replicate whose counts are
// given (NULL: every row once), the three coefficient vectors betas [3][k].
int ob_binary_means(ob_ctx* ctx, const double* x, int64_t ldx, const double* y, int64_t n, int32_t k,
                    const uint8_t* counts, const double* betas, double* out) {
  if (!x || !y || !betas || !out) return ob::fail(OB_E_INVALID, "null pointer");
  if (n <= 0 || k < 1)
    return ob::fail(OB_E_INVALID, "ob_binary_means needs n > 0 rows and k >= 1 columns, got n = %lld, k = %d", (long long)n, k);
  if (k > ob::kBinaryMaxK)
    return ob::fail(OB_E_UNSUPPORTED, "ob_binary_means takes at most %d columns, got %d", ob::kBinaryMaxK, k);
  if (ldx < n) return ob::fail(OB_E_INVALID, "ob_binary_means: ldx = %lld is below n = %lld", (long long)ldx, (long long)n);
  if (n >= ((int64_t)1 << 31)) return ob::fail(OB_E_UNSUPPORTED, "ob_binary_means takes fewer than 2^31 rows");
  for (int64_t i = 0; i < n; ++i)  // the pass takes x_0 = 1 as given
    if (x[i] != 1.0) return ob::fail(OB_E_UNSUPPORTED, "ob_binary_means: column 0 of x must be the intercept (all ones)");
  if (counts) {
    bool any = false;
    for (int64_t i = 0; i < n && !any; ++i) any = counts[i] != 0;
    if (!any) return ob::fail(OB_E_INVALID, "ob_binary_means: every count is zero");
  }
  if (!ctx) return ob::fail(OB_E_INVALID, "null pointer: ctx");
  OB_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint32_t tiles = (uint32_t)((n + OB_TILE_ROWS - 1) / OB_TILE_ROWS), nc = std::min<uint32_t>(tiles, 128u);
  const int64_t ld = (int64_t)tiles * OB_TILE_ROWS;
  std::vector<uint32_t> chunks;
  for (uint32_t c = 0; c < nc; ++c) {
    chunks.push_back(0u);
    chunks.push_back((uint32_t)((uint64_t)tiles * c / nc));
    chunks.push_back((uint32_t)((uint64_t)tiles * (c + 1) / nc));
  }
  const int nv = ob::binary_sums_len(k);
  DevBuf d_cols, d_chunks, d_betas, d_partial, d_counts;
  OB_HIP(d_cols.alloc(sizeof(double) * (size_t)ld * k));
  OB_HIP(hipMemsetAsync(d_cols.p, 0, sizeof(double) * (size_t)ld * k, s));
  OB_HIP(d_chunks.alloc(sizeof(uint32_t) * chunks.size()));
  OB_HIP(d_betas.alloc(sizeof(double) * 3 * k));
  OB_HIP(d_partial.alloc(sizeof(double) * (size_t)nc * 64 * nv));
  OB_HIP(hipMemcpyAsync(d_cols.p, y, sizeof(double) * n, hipMemcpyHostToDevice, s));
  for (int j = 1; j < k; ++j)
    OB_HIP(hipMemcpyAsync(d_cols.d() + (size_t)j * ld, x + (size_t)j * ldx, sizeof(double) * n, hipMemcpyHostToDevice, s));
  OB_HIP(hipMemcpyAsync(d_chunks.p, chunks.data(), sizeof(uint32_t) * chunks.size(), hipMemcpyHostToDevice, s));
  OB_HIP(hipMemcpyAsync(d_betas.p, betas, sizeof(double) * 3 * k, hipMemcpyHostToDevice, s));
  std::vector<uint32_t> img;  // replicate 0 of a one-batch f64-Gram count image (ob_engine.hpp)
  if (counts) {
    img.assign((size_t)tiles * 4 * kCimgWords, 0u);
    for (int64_t i = 0; i < n; ++i) {
      const size_t t = (size_t)(i / OB_TILE_ROWS), within = (size_t)(i % OB_TILE_ROWS), sub = within >> 6, qq = within & 63;
      img[(t * 4 + sub) * kCimgWords + (qq >> 2)] |= (uint32_t)counts[i] << (8 * (qq & 3));
    }
    OB_HIP(d_counts.alloc(sizeof(uint32_t) * img.size()));
    OB_HIP(hipMemcpyAsync(d_counts.p, img.data(), sizeof(uint32_t) * img.size(), hipMemcpyHostToDevice, s));
  }
  ob_heck_seg h{};
  h.cols[0] = d_cols.d();
  h.ld[0] = ld;
  h.n[0] = (uint32_t)n;
  h.tiles0 = tiles;
  h.ks = k;
  h.counts = counts ? d_counts.as<uint32_t>() : nullptr;
  h.nb_rep = 1;
  h.chunks = d_chunks.as<uint32_t>();
  h.n_chunks = (int)nc;
  h.rep_pad = 64;
  h.part_pad = 64;
  h.n_reps = 1;
  h.partial = d_partial.d();
  OB_HIP(launch_means(h, d_betas.d(), s));
  std::vector<double> part((size_t)nc * 64 * nv);
  OB_HIP(hipMemcpyAsync(part.data(), d_partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
  OB_HIP(hipStreamSynchronize(s));
  std::vector<double> sum(nv, 0.0);
  for (uint32_t c = 0; c < nc; ++c)  // chunk order, as ob_binary_row_kernel
    for (int j = 0; j < nv; ++j) sum[j] += part[(size_t)c * 64 * nv + j];
  const double cnt = sum[4];
  for (int v = 0; v < 3; ++v) out[v] = sum[v] / cnt;
  out[3] = sum[3] / cnt;
  out[4] = cnt;
  for (int j = 0; j < k; ++j) out[5 + j] = sum[5 + j] / cnt;
  return OB_OK;
}

}  // extern "C"
