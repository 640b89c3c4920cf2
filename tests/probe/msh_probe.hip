// msh_probe.hip — test infrastructure: runs the helpers of csrc/msh_seq_quot.h over their documented domains on the
// device and reports to tests/test_quot_probe_gpu.py through plain C entry points (libmsh_probe.so, loaded with
// ctypes). Every reciprocal is formed on the device by the expression the kernels use.
// The exhaustive entry points fill a report of REP_WORDS uint64_t:
//   [0] inputs on which the helper differs from the device's integer `/` of the same operands
//   [1] inputs whose remainder before the correction step lies outside [-m, 2m) (the one-step claim)
//   [2], [3] the same two counts over the inputs with a > m alone (quot_u16; else 0)
//   [4 ..] REP_TUPLES mismatches of the documented domain as (numerator, divisor, got, want), in the order the
//          threads met them; then one word that counts how many were offered
//   [last] the inputs evaluated: the host checks it against the size of the domain
// The *_raw entry points return the helper's outputs for inputs chosen by the host, which judges them itself.
// Every entry point returns 0 or the hipError_t that stopped it.
#include "../../mini-kube-scheduler_amd/csrc/msh_seq_quot.h"
#include "msh_probe_common.h"

namespace {

using namespace probe;

constexpr int REP_TUPLES = 8;
constexpr int REP_WORDS = 4 + 4 * REP_TUPLES + 2;
constexpr int REP_OFFERED = REP_WORDS - 2, REP_SEEN = REP_WORDS - 1;

// One thread's tallies, added to the report once at its end; a mismatch's tuple is taken while fewer than
// REP_TUPLES are recorded (rep[REP_OFFERED] counts them).
struct Tally {
  uint32_t mis = 0, out = 0, mis_beyond = 0, out_beyond = 0, seen = 0;
  __device__ __forceinline__ void see(u64* rep, bool outside, bool mismatch, bool beyond, u64 a, u64 m, u64 got,
                                      u64 want) {
    seen += 1u;
    out += outside ? 1u : 0u;
    out_beyond += outside && beyond ? 1u : 0u;
    mis += mismatch ? 1u : 0u;
    mis_beyond += mismatch && beyond ? 1u : 0u;
    if (mismatch && !beyond && *(volatile u64*)&rep[REP_OFFERED] < (u64)REP_TUPLES) {
      const u64 at = atomicAdd(&rep[REP_OFFERED], 1ull);
      if (at < (u64)REP_TUPLES) {
        u64* t = rep + 4 + 4 * at;
        t[0] = a;
        t[1] = m;
        t[2] = got;
        t[3] = want;
      }
    }
  }
  // every lane of a full wave: the wave's sums, for one lane to flush
  __device__ __forceinline__ void wave_sum() {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      mis += (uint32_t)__shfl_xor((int)mis, off);
      out += (uint32_t)__shfl_xor((int)out, off);
      mis_beyond += (uint32_t)__shfl_xor((int)mis_beyond, off);
      out_beyond += (uint32_t)__shfl_xor((int)out_beyond, off);
      seen += (uint32_t)__shfl_xor((int)seen, off);
    }
  }
  __device__ __forceinline__ void flush(u64* rep) {
    uint32_t v[4] = {mis, out, mis_beyond, out_beyond};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (v[k]) atomicAdd(&rep[k], (u64)v[k]);
    }
    atomicAdd(&rep[REP_SEEN], (u64)seen);
  }
};

__device__ __forceinline__ float nudged(float r, int ulps) {
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, r) + (uint32_t)ulps);
}
// the preference kernels' 1 / m
__device__ __forceinline__ float rcp_u32(uint32_t m, int ulps) { return nudged(__builtin_amdgcn_rcpf((float)m), ulps); }
// quot100's two reciprocals: ScoreArgmax::node_res (form 0) and BalScore::weighted_rs (form 1)
__device__ __forceinline__ float rcp100(int64_t c, int form) {
  return form == 0 ? 100.0f / (float)c : 100.0f * __builtin_amdgcn_rcpf((float)(double)c);
}

// ---- quot_u16: every a in [0, 65535] (x) for m = blockIdx.y + 1 ----
__global__ __launch_bounds__(TPB) void k_quot_u16(int ulps, u64* rep) {
  const uint32_t a = blockIdx.x * TPB + threadIdx.x, m = blockIdx.y + 1u;
  if (a > 65535u || m > 65535u) return;  // no thread of the launch (65536 / TPB blocks by 65535)
  const float rm = rcp_u32(m, ulps);
  const uint32_t got = msh::quot_u16(a, m, rm), want = 100u * a / m;
  const uint32_t q0 = (uint32_t)((float)(100u * a) * rm);  // quot_u16's estimate
  const int64_t r = (int64_t)(100u * a) - (int64_t)q0 * (int64_t)m;
  Tally t;
  t.see(rep, r < -(int64_t)m || r >= 2 * (int64_t)m, got != want, a > m, a, m, got, want);
  t.wave_sum();  // a > m may miss by the million: one atomic per wave
  if ((threadIdx.x & 63u) == 0u) t.flush(rep);
}

__global__ __launch_bounds__(TPB) void k_quot_u16_raw(const uint32_t* a, const uint32_t* m, int64_t n, int ulps,
                                                      uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = msh::quot_u16(a[i], m[i], rcp_u32(m[i], ulps));
}

// ---- quot_soft: one m per thread; per k in 0..100 the numerators ceil(k m / 100) and that +-1 within [0, m] ----
__device__ __forceinline__ void soft_one(uint32_t a, uint32_t m, float rm, u64* rep, Tally& t) {
  const uint32_t got = msh::quot_soft(a, m, rm), want = (uint32_t)(100ull * a / m);
  const uint32_t q0 = (uint32_t)((float)a * 100.0f * rm);  // quot_soft's estimate
  const int64_t r = (int64_t)(100ull * a) - (int64_t)((uint64_t)q0 * m);
  t.see(rep, r < -(int64_t)m || r >= 2 * (int64_t)m, got != want, false, a, m, got, want);
}

__global__ __launch_bounds__(TPB) void k_quot_soft(uint32_t m_lo, uint32_t m_hi, int ulps, u64* rep) {
  const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x + m_lo;
  const bool in = i < m_hi;
  const uint32_t m = in ? (uint32_t)i : 1u;  // a lane past the range stays for the wave's sum and tallies nothing
  const float rm = rcp_u32(m, ulps);
  const uint32_t mq = m / 100u, mr = m % 100u;  // ceil(k m / 100) = k mq + ceil(k mr / 100), k mr < 10^4
  Tally t;
  soft_one(0u, m, rm, rep, t);
  soft_one(m, m, rm, rep, t);
  for (uint32_t k = 0; k <= 100u; ++k) {
    const uint32_t b = k * mq + (k * mr + 99u) / 100u;  // <= m
    if (b > 0u) soft_one(b - 1u, m, rm, rep, t);
    soft_one(b, m, rm, rep, t);
    if (b < m) soft_one(b + 1u, m, rm, rep, t);
  }
  if (!in) t = Tally();
  t.wave_sum();
  if ((threadIdx.x & 63u) == 0u) t.flush(rep);
}

__global__ __launch_bounds__(TPB) void k_quot_soft_raw(const uint32_t* a, const uint32_t* m, int64_t n, int ulps,
                                                       uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = msh::quot_soft(a[i], m[i], rcp_u32(m[i], ulps));
}

// ---- quot100: one divisor of the host's list per thread, the same numerators ----
__device__ __forceinline__ void q100_one(int64_t num, int64_t c, float rc, u64* rep, Tally& t) {
  const uint32_t got = msh::quot100(num, c, rc), want = (uint32_t)(num * 100 / c);
  const uint32_t lo = (uint32_t)((uint64_t)num & 0xFFFFFFFFull), hi = (uint32_t)((uint64_t)num >> 32);
  const uint32_t s0 = (uint32_t)(__builtin_fmaf((float)hi, 4294967296.0f, (float)lo) * rc);  // quot100's estimate
  const int64_t r = num * 100 - (int64_t)(uint64_t)s0 * c;
  t.see(rep, r < -c || r >= 2 * c, got != want, false, (u64)num, (u64)c, got, want);
}

__global__ __launch_bounds__(TPB) void k_quot100(const int64_t* cs, int64_t nc, int form, u64* rep) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int64_t ci = i < nc ? cs[i] : 0;
  const bool in = ci >= 1 && ci <= (int64_t(1) << 55);
  const int64_t c = in ? ci : 1;  // as k_quot_soft's
  const float rc = rcp100(c, form);
  Tally t;
  q100_one(0, c, rc, rep, t);
  q100_one(c, c, rc, rep, t);
  for (int64_t k = 0; k <= 100; ++k) {
    const int64_t b = (k * c + 99) / 100;  // k c < 2^62; <= c
    if (b > 0) q100_one(b - 1, c, rc, rep, t);
    q100_one(b, c, rc, rep, t);
    if (b < c) q100_one(b + 1, c, rc, rep, t);
  }
  if (!in) t = Tally();
  t.wave_sum();
  if ((threadIdx.x & 63u) == 0u) t.flush(rep);
}

__global__ __launch_bounds__(TPB) void k_quot100_raw(const int64_t* num, const int64_t* c, int64_t n, int form,
                                                     uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = msh::quot100(num[i], c[i], rcp100(c[i], form));
}

// ---- wsum_div: sum = blockIdx.y + 1 in 1..400, acc (x) in 0..100 sum; out at 50 s (s - 1) + (s - 1) + acc ----
constexpr uint32_t WSUM_MAX = 400u;
constexpr int64_t WSUM_OUT = 50ll * WSUM_MAX * (WSUM_MAX + 1) + WSUM_MAX;  // sum over s of (100 s + 1)

__global__ __launch_bounds__(TPB) void k_wsum(u64* rep, uint32_t* out) {
  const uint32_t acc = blockIdx.x * TPB + threadIdx.x, sum = blockIdx.y + 1u;
  const bool in = sum <= WSUM_MAX && acc <= 100u * sum;  // a lane past the range stays for the wave's sum
  const uint32_t got = msh::wsum_div(in ? acc : 0u, msh::wsum_magic(sum)), want = (in ? acc : 0u) / sum;
  Tally t;
  if (in) t.see(rep, false, got != want, false, acc, sum, got, want);
  t.wave_sum();
  if ((threadIdx.x & 63u) == 0u) t.flush(rep);
  if (in) out[50u * sum * (sum - 1u) + (sum - 1u) + acc] = got;
}

// ---- soft_raw and balanced_bs: outputs only, the host holds the reference ----
__global__ __launch_bounds__(TPB) void k_soft_raw(int32_t c_lo, int64_t n, double w, int32_t skew1, int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = msh::soft_raw((int32_t)(c_lo + i), w, skew1);
}

__global__ __launch_bounds__(TPB) void k_balanced_bs(const int64_t* q, int64_t n, uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = msh::balanced_bs(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
}

// ---- host plumbing ----
hipError_t new_report(Dev& d, u64** rep) {
  PROBE_TRY(d.get((void**)rep, REP_WORDS * sizeof(u64)));
  return hipMemset(*rep, 0, REP_WORDS * sizeof(u64));
}

template <class T, class K>
hipError_t raw_pairs(K kernel, const T* a, const T* m, int64_t n, int arg, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  Dev d;
  T *da, *dm;
  uint32_t* dout;
  PROBE_TRY(d.put((void**)&da, a, n * sizeof(T)));
  PROBE_TRY(d.put((void**)&dm, m, n * sizeof(T)));
  PROBE_TRY(d.get((void**)&dout, n * sizeof(uint32_t)));
  hipLaunchKernelGGL(kernel, dim3(blocks(n)), dim3(TPB), 0, 0, da, dm, n, arg, dout);
  return finish(out, dout, n * sizeof(uint32_t));
}

}  // namespace

extern "C" {

int msh_probe_rep_words(void) { return REP_WORDS; }
int64_t msh_probe_wsum_out(void) { return WSUM_OUT; }

int msh_probe_quot_u16(int ulps, uint64_t* rep) {
  Dev d;
  u64* drep;
  PROBE_TRY(new_report(d, &drep));
  hipLaunchKernelGGL(k_quot_u16, dim3(65536 / TPB, 65535), dim3(TPB), 0, 0, ulps, drep);
  return finish(rep, drep, REP_WORDS * sizeof(u64));
}

int msh_probe_quot_u16_raw(const uint32_t* a, const uint32_t* m, int64_t n, int ulps, uint32_t* out) {
  return raw_pairs(k_quot_u16_raw, a, m, n, ulps, out);
}

// every m in [m_lo, m_hi), 1 <= m_lo, m_hi <= 2^28
int msh_probe_quot_soft(uint32_t m_lo, uint32_t m_hi, int ulps, uint64_t* rep) {
  if (m_lo < 1u || m_hi > (1u << 28) || m_lo > m_hi) return hipErrorInvalidValue;
  Dev d;
  u64* drep;
  PROBE_TRY(new_report(d, &drep));
  if (m_hi > m_lo)
    hipLaunchKernelGGL(k_quot_soft, dim3(blocks((int64_t)m_hi - m_lo)), dim3(TPB), 0, 0, m_lo, m_hi, ulps, drep);
  return finish(rep, drep, REP_WORDS * sizeof(u64));
}

int msh_probe_quot_soft_raw(const uint32_t* a, const uint32_t* m, int64_t n, int ulps, uint32_t* out) {
  return raw_pairs(k_quot_soft_raw, a, m, n, ulps, out);
}

// the divisors cs[nc], each in [1, 2^55] (others are passed over); form 0: 100 / float(c), form 1: 100 * rcp
int msh_probe_quot100(const int64_t* cs, int64_t nc, int form, uint64_t* rep) {
  Dev d;
  u64* drep;
  int64_t* dcs;
  PROBE_TRY(new_report(d, &drep));
  PROBE_TRY(d.put((void**)&dcs, cs, (nc > 0 ? nc : 0) * sizeof(int64_t)));
  if (nc > 0) hipLaunchKernelGGL(k_quot100, dim3(blocks(nc)), dim3(TPB), 0, 0, dcs, nc, form, drep);
  return finish(rep, drep, REP_WORDS * sizeof(u64));
}

int msh_probe_quot100_raw(const int64_t* num, const int64_t* c, int64_t n, int form, uint32_t* out) {
  return raw_pairs(k_quot100_raw, num, c, n, form, out);
}

// out[msh_probe_wsum_out()]: wsum_div(acc, wsum_magic(sum)) at 50 sum (sum - 1) + (sum - 1) + acc
int msh_probe_wsum(uint64_t* rep, uint32_t* out) {
  Dev d;
  u64* drep;
  uint32_t* dout;
  PROBE_TRY(new_report(d, &drep));
  PROBE_TRY(d.get((void**)&dout, WSUM_OUT * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_wsum, dim3(blocks(100 * WSUM_MAX + 1), WSUM_MAX), dim3(TPB), 0, 0, drep, dout);
  PROBE_TRY(finish(out, dout, WSUM_OUT * sizeof(uint32_t)));
  return hipMemcpy(rep, drep, REP_WORDS * sizeof(u64), hipMemcpyDeviceToHost);
}

// out[c_hi - c_lo + 1]: soft_raw(c, w, skew1) for c in [c_lo, c_hi]
int msh_probe_soft_raw(int32_t c_lo, int32_t c_hi, double w, int32_t skew1, int32_t* out) {
  if (c_lo < 0 || c_hi < c_lo) return hipErrorInvalidValue;
  const int64_t n = (int64_t)c_hi - c_lo + 1;
  Dev d;
  int32_t* dout;
  PROBE_TRY(d.get((void**)&dout, n * sizeof(int32_t)));
  hipLaunchKernelGGL(k_soft_raw, dim3(blocks(n)), dim3(TPB), 0, 0, c_lo, n, w, skew1, dout);
  return finish(out, dout, n * sizeof(int32_t));
}

// quads[n][4] = (q0, c0, q1, c1)
int msh_probe_balanced_bs(const int64_t* quads, int64_t n, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  Dev d;
  int64_t* dq;
  uint32_t* dout;
  PROBE_TRY(d.put((void**)&dq, quads, 4 * n * sizeof(int64_t)));
  PROBE_TRY(d.get((void**)&dout, n * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_balanced_bs, dim3(blocks(n)), dim3(TPB), 0, 0, dq, n, dout);
  return finish(out, dout, n * sizeof(uint32_t));
}

}  // extern "C"
