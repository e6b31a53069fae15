// ob_hip.hpp -- host-side HIP plumbing shared by the launch code: the error macro, a device buffer
// and an event set that free themselves, and the grid size of a 256-thread launch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ob_common.hpp"

#define OB_HIP(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return ob::fail(OB_E_HIP, "HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, \
                      __LINE__);                                                         \
  } while (0)

// One hipMalloc that frees itself. alloc keeps an allocation that is already large enough.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (p && cap >= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
  double* d() const { return as<double>(); }
};

// N events that destroy themselves.
template <int N>
struct Events {
  hipEvent_t e[N] = {};
  ~Events() {
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
  }
  hipError_t create() {
    for (hipEvent_t& v : e) {
      const hipError_t rc = hipEventCreate(&v);
      if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
  }
};

// Blocks of 256 threads that cover n items.
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }
