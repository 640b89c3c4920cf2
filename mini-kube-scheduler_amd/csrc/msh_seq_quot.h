// msh_seq_quot.h — the exact-quotient arithmetic of the scored sequential-commit kernels, in one place: float
// reciprocals with a one-step correction, the weight-sum magic, and the two float64 scores that follow upstream's
// operations one rounding at a time. Every function is host and device code alike, so tests/probe/msh_probe.hip
// runs each over its whole documented domain on the device and the pure integer ones on the host as well. A
// reciprocal is always the caller's: the kernels form it on the device (IEEE division or v_rcp_f32) and pass it in.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace msh {

// num * 100 / c for 0 <= num <= c, 1 <= c <= 2^55, rc = 100 / c rounded to float.
__host__ __device__ __forceinline__ uint32_t quot100(int64_t num, int64_t c, float rc) {
  const uint32_t lo = (uint32_t)((uint64_t)num & 0xFFFFFFFFull), hi = (uint32_t)((uint64_t)num >> 32);
  const float nf = __builtin_fmaf((float)hi, 4294967296.0f, (float)lo);
  uint32_t s = (uint32_t)(nf * rc);                           // within 1 of the quotient
  const int64_t rm = num * 100 - (int64_t)(uint64_t)s * c;  // in [-c, 2c)
  s += rm >= c ? 1u : 0u;
  s -= rm < 0 ? 1u : 0u;
  return s;
}

// 100 * a / m for 0 <= a <= 65,535, 1 <= m <= 65,535, rm = 1 / m as a float (any rounding within a few ulp):
// 100 * a < 2^24 is exact in a float, the product is within 1 of the quotient, one correction step either way.
// Only the quotients of feasible nodes are used, where a <= m.
__host__ __device__ __forceinline__ uint32_t quot_u16(uint32_t a, uint32_t m, float rm) {
  const uint32_t num = 100u * a;
  uint32_t q = (uint32_t)((float)num * rm);
  const int32_t r = (int32_t)num - (int32_t)(q * m);  // in [-m, 2m)
  q += r >= (int32_t)m ? 1u : 0u;
  q -= r < 0 ? 1u : 0u;
  return q;
}

// raw_z of msh_seq_soft.hip's head comment for a count c in [0, 2^25], w = log(size + 2) <= log 66 and
// skew1 = max_skew - 1 in [0, 2^24): the product and the sum rounded separately (contraction off: no fused
// multiply-add), then half away from zero. y < 2^28 and y - trunc(y) is exact, so the comparison with 0.5 is Go's
// math.Round.
__host__ __device__ __forceinline__ int32_t soft_raw(int32_t c, double w, int32_t skew1) {
#pragma clang fp contract(off)
  const double x = (double)c * w;
  const double y = x + (double)skew1;
  const double t = __builtin_trunc(y);
  return (int32_t)t + (y - t >= 0.5 ? 1 : 0);
}

// 100 * a / m, truncated, for 0 <= a <= m, 1 <= m < 2^28 (the bound of raw above; MSH_SPREAD_SOFT_MAX keeps it),
// rm = 1 / float(m) within an ulp. The true quotient x is in [0, 100]; float(a), the factor 100, float(m), the
// reciprocal and the product each err by at most 2^-23 relative, so the estimate is within 100 * 5 * 2^-23 < 2^-14
// of x and its floor is floor(x) or one off, and only next to an integer. The remainder is taken in 64 bits
// (100 * a < 2^35, q * m <= 101 * 2^28) and corrects one step either way: exact.
__host__ __device__ __forceinline__ uint32_t quot_soft(uint32_t a, uint32_t m, float rm) {
  uint32_t q = (uint32_t)((float)a * 100.0f * rm);
  const int64_t r = (int64_t)(100ull * a) - (int64_t)((uint64_t)q * m);  // in [-m, 2m)
  q += r >= (int64_t)m ? 1u : 0u;
  q -= r < 0 ? 1u : 0u;
  return q;
}

// BS of msh_seq_balanced.hip's head comment for 0 <= q_r <= 2^56 and 0 <= c_r <= 2^55: two conversions and one
// division per resource, the clamp, then v_add_f64 (the difference), v_add_f64 (1 - |d|, the modulus an operand
// modifier), v_mul_f64 and a truncating convert. f_r is in [0, 1], so the product is in [0, 100].
__host__ __device__ __forceinline__ uint32_t balanced_bs(int64_t q0, int64_t c0, int64_t q1, int64_t c1) {
#pragma clang fp contract(off)
  const double x0 = (double)q0 / (double)c0, x1 = (double)q1 / (double)c1;
  const double f0 = (c0 == 0 || x0 > 1.0) ? 1.0 : x0;
  const double f1 = (c1 == 0 || x1 > 1.0) ? 1.0 : x1;
  const double d = f0 - f1;
  const double u = 1.0 - __builtin_fabs(d);
  return (uint32_t)(int32_t)(u * 100.0);
}

// ceil(2^31 / sum) for the sum of the resource weights, 1 <= sum <= 400
__host__ __device__ __forceinline__ uint32_t wsum_magic(uint32_t sum) {
  return (uint32_t)(((uint64_t(1) << 31) + sum - 1) / sum);
}

// acc / sum for acc <= 100 * sum with magic = wsum_magic(sum): (acc * magic) >> 31 as the high half of a product
__host__ __device__ __forceinline__ uint32_t wsum_div(uint32_t acc, uint32_t magic) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(acc * 2u, magic);
#else
  return (uint32_t)(((uint64_t)(acc * 2u) * magic) >> 32);
#endif
}

}  // namespace msh
