// msh_probe_common.h — the host plumbing the device probes of tests/probe share (msh_probe.hip, msh_gprobe.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace probe {

constexpr int TPB = 256;
typedef unsigned long long u64;

#define PROBE_TRY(x)                 \
  do {                               \
    const hipError_t e_ = (x);       \
    if (e_ != hipSuccess) return e_; \
  } while (0)

struct Dev {  // device buffers of one call, freed on every way out
  static constexpr int CAP = 8;
  void* p[CAP] = {};
  int n = 0;
  ~Dev() {
    for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
  }
  hipError_t get(void** out, size_t bytes) {
    if (n >= CAP) return hipErrorInvalidValue;
    const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e == hipSuccess) p[n++] = *out;
    return e;
  }
  hipError_t put(void** out, const void* src, size_t bytes) {
    const hipError_t e = get(out, bytes);
    return e != hipSuccess ? e : hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice);
  }
};

inline unsigned blocks(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

inline hipError_t finish(void* host, const void* dev, size_t bytes) {
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  return hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
}

}  // namespace probe
