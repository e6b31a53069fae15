// ob_pairpass.hpp -- what the Newton front ends around the pair-product pass kernels (ob_heck_wide_kernel,
// ob_rw_kernel, ob_dr_kernel, ob_tobit_kernel) share: tri_row, the head of their step kernels and
// the host loop that runs pass and step until no fit is left iterating. The pass kernels themselves stay apart.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ob_engine.hpp"
#include "ob_hip.hpp"
#include "ob_spec.h"

namespace {

// Row j of the packed lower triangle that holds entry e = j (j + 1) / 2 + i, i <= j.
__device__ __forceinline__ int tri_row(int e) {
  int j = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
  while ((j + 1) * (j + 2) / 2 <= e) ++j;
  while (j * (j + 1) / 2 > e) --j;
  return j;
}

// The head of a step kernel, by one wave: the nv partials of one fit, each summed over the chunks in chunk order
// (g >= 0: only the chunks of group g), the first D (D + 1) / 2 into both triangles of m [D x D], the rest into
// step. The partial of chunk c is partial[(c * chunk_stride + fit) * nv ..]. The caller synchronizes.
__device__ __forceinline__ void gather_partials(const double* partial, size_t chunk_stride, size_t fit, int nv,
                                                const uint32_t* chunks, int n_chunks, int g, int D, int lane, double* m,
                                                double* step) {
  const int NH = D * (D + 1) / 2;
  for (int e = lane; e < nv; e += 64) {
    double v = 0.0;
    for (int c = 0; c < n_chunks; ++c)
      if (g < 0 || chunks[3 * c] == (uint32_t)g) v += partial[((size_t)c * chunk_stride + fit) * nv + e];
    if (e < NH) {
      const int j = tri_row(e), i = e - j * (j + 1) / 2;
      m[j + i * D] = v;
      m[i + j * D] = v;
    } else {
      step[e - NH] = v;
    }
  }
}

// The Newton rounds of one batch: clear `active`, run pass() between two events, run step(), read `active` back (the
// round's one stream wait), until no fit is left iterating or max_passes rounds have run. pass and step return a
// hipError_t. *rounds: the rounds taken; *pass_ms: the passes' time, added up.
template <class Pass, class Step>
int newton_rounds(uint32_t* d_active, int max_passes, hipStream_t s, Pass pass, Step step, int* rounds, float* pass_ms) {
  Events<2> ev;
  OB_HIP(ev.create());
  int it = 0;
  float total = 0.f;
  while (it < max_passes) {
    OB_HIP(hipMemsetAsync(d_active, 0, sizeof(uint32_t), s));
    OB_HIP(hipEventRecord(ev.e[0], s));
    OB_HIP(pass());
    OB_HIP(hipEventRecord(ev.e[1], s));
    OB_HIP(step());
    ++it;
    uint32_t active = 0;
    OB_HIP(hipMemcpyAsync(&active, d_active, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OB_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    OB_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    total += ms;
    if (active == 0) break;
  }
  *rounds = it;
  *pass_ms = total;
  return OB_OK;
}

}  // namespace
