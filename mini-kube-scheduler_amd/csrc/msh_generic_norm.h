// msh_generic_norm.h — generic_kernel's pure per-pair helpers (msh_generic.hip), in one place: NormalizeScore by the
// exact reciprocal and the three key types' term, mask and maximum. tests/probe/msh_gprobe.hip runs
// each alone over its documented domain on the device; a host build (tests/probe/msh_probe_host.cpp, which defines
// MSH_GEN_HOST_ONLY) takes the double paths, whose arithmetic is IEEE on both sides, and leaves out what exists on
// the device only (the 24-bit multiply of the 32-bit keys, v_bitop3 and v_max_f64).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#if !defined(MSH_GEN_HOST_ONLY)
#include "msh_device.h"
#endif
#define MSH_GEN_FN __host__ __device__ __forceinline__

namespace msh {

constexpr double GEN_RCP_BIAS = 1.0 + 0x1p-49;

// NormalizeScore of one raw score given the pod's extent of that plugin over its feasible nodes
// (mx, mn): upstream helper.DefaultNormalizeScore(MaxNodeScore = 100, reverse) — maxCount starts at 0,
// an all-zero list is left alone (reverse: all 100) — or min-max (0 when max == min).
MSH_GEN_FN int64_t gen_normalize(int64_t raw, int32_t mode, int64_t mx, int64_t mn) {
  switch (mode) {
    case 1: {
      const int64_t m = mx > 0 ? mx : 0;
      return m == 0 ? raw : 100 * raw / m;
    }
    case 2: {
      const int64_t m = mx > 0 ? mx : 0;
      return m == 0 ? 100 : 100 - 100 * raw / m;
    }
    case 3: return mx == mn ? 0 : (raw - mn) * 100 / (mx - mn);
    default: return raw;
  }
}

// The NormalizeScore parameters of one normalizing column (mode md: 1 DEFAULT, 2 REVERSE, 3 MIN-MAX) for the extents
// (mx, mn) of a class with a feasible node: the reciprocal r and the offset b of col_term's q = (100 raw - b) x r.
MSH_GEN_FN void gen_norm_params(int32_t md, int64_t mx, int64_t mn, double* r, double* b) {
  *r = 0.0;
  *b = 0.0;
  if (md == 3) {                  // min-max: (raw - mn) x 100 / (mx - mn), 0 when mx == mn
    if (mx != mn) {
      *r = (1.0 / (double)(mx - mn)) * GEN_RCP_BIAS;
      *b = 100.0 * (double)mn;
    }
  } else {  // DefaultNormalizeScore: 100 raw / max(mx, 0); DEFAULT leaves an all-zero list (m = 0 -> raw)
    const int64_t m = mx > 0 ? mx : 0;
    if (m != 0) *r = (1.0 / (double)m) * GEN_RCP_BIAS;
    else if (md == 1) *r = 0.01 * GEN_RCP_BIAS;
    // REVERSE with m == 0: r = 0, 100 - 0 = 100 for every node
  }
}

#if !defined(MSH_GEN_HOST_ONLY)
// v_max_f64 as the instruction (fmax adds a NaN canonicalisation per operand): IEEE mode,
// a quiet NaN operand yields the other one
__device__ __forceinline__ double vmax_f64(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// v with its high dword ORed with m: m all-ones turns it into a quiet NaN (exponent and quiet bit set)
__device__ __forceinline__ double nan_if(double v, uint32_t x, uint32_t nt) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t hi = bop3_or_and((uint32_t)(b >> 32), x, nt);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | (uint32_t)b);
}
#endif

// Per-pair key of the main pass (KT): uint32_t (32-bit totals, biased by 2^31) or uint64_t (biased by
// 2^63), 0 = infeasible; or double (the total, |total| < 2^53), NaN = infeasible (v_max_f64 skips it).
template <int KT>
using GKey = typename std::conditional<KT == 0, uint32_t,
                                       typename std::conditional<KT == 1, uint64_t, double>::type>::type;

#if !defined(MSH_GEN_HOST_ONLY)
template <int KT>
__device__ __forceinline__ GKey<KT> key_mask(GKey<KT> t, uint32_t xm, uint32_t nt) {
  if constexpr (KT == 2) {
    return nan_if(t, xm, nt);
  } else if constexpr (KT == 1) {
    const uint32_t lo = bop3_andn_of_and((uint32_t)t, xm, nt), hi = bop3_andn_of_and((uint32_t)(t >> 32), xm, nt);
    return ((uint64_t)hi << 32) | lo;
  } else {
    return bop3_andn_of_and(t, xm, nt);
  }
}
#endif

// The contribution of normalizing column c to a pair's total: w x trunc((v - b) x r), v = 100 x raw.
template <int KT, bool SUB>
MSH_GEN_FN GKey<KT> col_term(double v, double b, double r, GKey<KT> cw) {
  const double q = (SUB ? v - b : v) * r;
  if constexpr (KT == 2) {
    // |trunc(q) x w| is within the host's 2^53 bound on a feasible pair: exact (the others are masked)
    return __builtin_trunc(q) * cw;
  } else if constexpr (KT == 1) {
    // |q| < 2^40 on a feasible pair; an infeasible pair's value is clamped, converted and masked out
    const int64_t n = (int64_t)__builtin_fmin(__builtin_fmax(q, -0x1p62), 0x1p62);
    return (uint64_t)n * cw;
  } else {
#if !defined(MSH_GEN_HOST_ONLY)
    // |n| and |w| below 2^23 on a feasible pair (the host's bound, GenericArgs::w64): the signed 24-bit
    // multiply (full rate, where v_mul_lo_u32 is quarter rate); v_cvt_i32_f64 saturates on the others.
    // That operand range is guaranteed ONLY by generic_args' c24 check (msh_capi.cpp): every normalizing
    // column's weight and normalized-score bound below 2^23, else the launch takes 64-bit keys. A new term
    // multiplied here must be added to that check.
    const int32_t n = (int32_t)q;
    return (uint32_t)__mul24(n, (int32_t)cw);
#else
    static_assert(KT != 0, "the 32-bit keys' term is device code");
#endif
  }
}

}  // namespace msh
