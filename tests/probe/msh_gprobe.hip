// msh_gprobe.hip — test infrastructure: the batch kernels' pure helpers on the device, each alone, reporting to
// tests/test_generic_probe_gpu.py through plain C entry points of libmsh_probe.so (ctypes): csrc/msh_generic_norm.h
// (generic_kernel's NormalizeScore by reciprocal, its three key types' term, mask and maximum) and msh_device.h's
// decodes and bit helpers. The reciprocal and the offset are formed on the device by gen_norm_params, the
// expression generic_kernel calls.
// msh_gprobe_quot fills a report of G_WORDS uint64_t:
//   [0] evaluations whose term differs from the device's int64 `/` of the same operands
//   [1] evaluations on which gen_normalize differs from that `/`
//   [2 ..] G_TUPLES mismatches as (mode, raw, mx, mn, got, want), in the order the threads met them; then one word
//          that counts how many were offered
//   [last] the evaluations made: the host checks it against the size of the domain
// The *_raw entry points return the helpers' outputs for inputs chosen by the host, which judges them itself.
// Every entry point returns 0 or the hipError_t that stopped it.
#include "../../mini-kube-scheduler_amd/csrc/msh_generic_norm.h"
#include "msh_probe_common.h"

namespace {

using namespace probe;
using msh::GKey;

constexpr int G_TUPLES = 8, G_TW = 6;
constexpr int G_WORDS = 2 + G_TW * G_TUPLES + 2;
constexpr int G_OFFERED = G_WORDS - 2, G_SEEN = G_WORDS - 1;
constexpr int64_t RAW_LO = -(int64_t(1) << 31), RAW_HI = int64_t(1) << 31;  // msh_upload_score_column's range
constexpr u64 D_MAX = u64(1) << 32;                                         // RAW_HI - RAW_LO
// 32-bit keys hold a term below 2^23 (col_term's comment): the raws at RAW_LO are theirs when 100 * 2^31 / d is
constexpr u64 K32_NEG_D = 25600;

// a weight, a key and a total in each key type
template <int KT>
__device__ __forceinline__ GKey<KT> key_of(int64_t w) {
  if constexpr (KT == 2) return (double)w;
  else return (GKey<KT>)w;
}
template <int KT>
__device__ __forceinline__ GKey<KT> key_bits(u64 b) {
  if constexpr (KT == 2) return __builtin_bit_cast(double, b);
  else return (GKey<KT>)b;
}
template <int KT>
__device__ __forceinline__ u64 bits_key(GKey<KT> k) {
  if constexpr (KT == 2) return __builtin_bit_cast(u64, k);
  else return (u64)k;
}
template <int KT>
__device__ __forceinline__ bool is_total(GKey<KT> k, int64_t want) {
  if constexpr (KT == 2) return k == (double)want;
  else if constexpr (KT == 1) return (int64_t)k == want;
  else return (int64_t)(int32_t)k == want;
}
template <int KT>
__device__ __forceinline__ int64_t total_of(GKey<KT> k) {  // for the report and the raw outputs
  if constexpr (KT == 2) return (int64_t)__builtin_fmin(__builtin_fmax(k, -0x1p62), 0x1p62);
  else if constexpr (KT == 1) return (int64_t)k;
  else return (int64_t)(int32_t)k;
}

struct GTally {
  uint32_t mis = 0, misn = 0, seen = 0;
  __device__ __forceinline__ void see(u64* rep, bool mismatch, bool norm_mismatch, int mode, int64_t raw, int64_t mx,
                                      int64_t mn, int64_t got, int64_t want) {
    seen += 1u;
    mis += mismatch ? 1u : 0u;
    misn += norm_mismatch ? 1u : 0u;
    if ((mismatch || norm_mismatch) && *(volatile u64*)&rep[G_OFFERED] < (u64)G_TUPLES) {
      const u64 at = atomicAdd(&rep[G_OFFERED], 1ull);
      if (at < (u64)G_TUPLES) {
        u64* t = rep + 2 + G_TW * at;
        t[0] = (u64)mode;
        t[1] = (u64)raw;
        t[2] = (u64)mx;
        t[3] = (u64)mn;
        t[4] = (u64)got;
        t[5] = (u64)want;
      }
    }
  }
  // every lane of a full wave: the wave's sums, for one lane to flush
  __device__ __forceinline__ void wave_sum() {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      mis += (uint32_t)__shfl_xor((int)mis, off);
      misn += (uint32_t)__shfl_xor((int)misn, off);
      seen += (uint32_t)__shfl_xor((int)seen, off);
    }
  }
  __device__ __forceinline__ void flush(u64* rep) {
    if (mis) atomicAdd(&rep[0], (u64)mis);
    if (misn) atomicAdd(&rep[1], (u64)misn);
    atomicAdd(&rep[G_SEEN], (u64)seen);
  }
};

// (r, b) of one class as generic_kernel forms them, r then moved by `ulps`; unbiased: r without GEN_RCP_BIAS,
// probe-local code, the error this probe exists to see
__device__ __forceinline__ void params(int mode, int64_t mx, int64_t mn, int ulps, int unbiased, double* r,
                                       double* b) {
  msh::gen_norm_params(mode, mx, mn, r, b);
  if (unbiased) *r = 1.0 / (double)(mode == 3 ? mx - mn : mx);
  *r = __builtin_bit_cast(double, __builtin_bit_cast(u64, *r) + (u64)(int64_t)ulps);
}

// One normalized score: the term of weight 1 (REVERSE: 100 and the term of weight -1, as the kernel's keys hold
// it), the device's int64 `/`, and gen_normalize.
template <int KT, int MODE>
__device__ __forceinline__ GKey<KT> norm_term(int64_t raw, double r, double b) {
  const double v = 100.0 * (double)raw;  // class_term's
  if constexpr (MODE == 3) return msh::col_term<KT, true>(v, b, r, key_of<KT>(1));
  else if constexpr (MODE == 1) return msh::col_term<KT, false>(v, b, r, key_of<KT>(1));
  else return key_of<KT>(100) + msh::col_term<KT, false>(v, b, r, key_of<KT>(-1));
}
template <int MODE>
__device__ __forceinline__ int64_t norm_want(int64_t raw, int64_t mx, int64_t mn) {
  if constexpr (MODE == 3) return (raw - mn) * 100 / (mx - mn);
  else if constexpr (MODE == 1) return 100 * raw / mx;
  else return 100 - 100 * raw / mx;
}
template <int KT, int MODE>
__device__ __forceinline__ void quot_one(int64_t raw, int64_t mx, int64_t mn, double r, double b, u64* rep,
                                         GTally& t) {
  const GKey<KT> got = norm_term<KT, MODE>(raw, r, b);
  const int64_t want = norm_want<MODE>(raw, mx, mn);
  t.see(rep, !is_total<KT>(got, want), msh::gen_normalize(raw, MODE, mx, mn) != want, MODE, raw, mx, mn,
        total_of<KT>(got), want);
}

// the boundary set of d (tests/quot_probe.py's head comment) as raws base + sign * a
template <int KT, int MODE>
__device__ __forceinline__ void sweep(u64 d, int64_t base, int64_t sign, int64_t mx, int64_t mn, double r, double b,
                                      u64* rep, GTally& t) {
  const u64 dq = d / 100u, dr = d % 100u;  // ceil(k d / 100) = k dq + ceil(k dr / 100)
  quot_one<KT, MODE>(base, mx, mn, r, b, rep, t);
  quot_one<KT, MODE>(base + sign * (int64_t)d, mx, mn, r, b, rep, t);
  for (u64 k = 0; k <= 100u; ++k) {
    const u64 a = k * dq + (k * dr + 99u) / 100u;  // <= d
    if (a > 0u) quot_one<KT, MODE>(base + sign * (int64_t)(a - 1u), mx, mn, r, b, rep, t);
    quot_one<KT, MODE>(base + sign * (int64_t)a, mx, mn, r, b, rep, t);
    if (a < d) quot_one<KT, MODE>(base + sign * (int64_t)(a + 1u), mx, mn, r, b, rep, t);
  }
}

// DEFAULT / REVERSE of maximum d: the boundary set, its negatives, RAW_LO and its two neighbours, and the three raws
// around the quotient boundary nearest to RAW_LO (kept at or above it)
template <int KT, int MODE>
__device__ __forceinline__ void default_like(u64 d, int ulps, int unbiased, u64* rep, GTally& t) {
  const int64_t mx = (int64_t)d, mn = INT64_MAX;  // the kernel's mn of a launch without a MIN-MAX column
  double r, b;
  params(MODE, mx, mn, ulps, unbiased, &r, &b);
  sweep<KT, MODE>(d, 0, 1, mx, mn, r, b, rep, t);
  sweep<KT, MODE>(d, 0, -1, mx, mn, r, b, rep, t);
  if (KT != 0 || d > K32_NEG_D) {
    const u64 k0 = (100ull << 31) / d;
    const int64_t e = -(int64_t)((k0 * d + 99u) / 100u);  // the largest raw at or above RAW_LO whose quotient is -k0
#pragma unroll
    for (int64_t o = 0; o < 3; ++o) {
      quot_one<KT, MODE>(RAW_LO + o, mx, mn, r, b, rep, t);
      quot_one<KT, MODE>(max(e - 1 + o, RAW_LO), mx, mn, r, b, rep, t);
    }
  }
}

// One divisor per thread: ds[i], or d_lo + i when ds is null. Divisors outside [1, 2^32] are passed over.
template <int KT>
__global__ __launch_bounds__(TPB) void k_gquot(const u64* ds, u64 d_lo, int64_t nd, int ulps, int unbiased, u64* rep) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const u64 di = i < nd ? (ds ? ds[i] : d_lo + (u64)i) : 0u;
  const bool in = di >= 1u && di <= D_MAX;
  const u64 d = in ? di : 1u;  // a lane past the range stays for the wave's sum and tallies nothing
  GTally t;
  // MIN-MAX over [mn, mn + d]: mn = RAW_LO, 0 where d <= RAW_HI, and the largest, RAW_HI - d
  const int64_t mns[3] = {RAW_LO, 0, RAW_HI - (int64_t)d};
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    if (o == 1 && d > (u64)RAW_HI) continue;
    const int64_t mn = mns[o], mx = mn + (int64_t)d;
    double r, b;
    params(3, mx, mn, ulps, unbiased, &r, &b);
    sweep<KT, 3>(d, mn, 1, mx, mn, r, b, rep, t);
  }
  default_like<KT, 1>(d, ulps, unbiased, rep, t);
  default_like<KT, 2>(d, ulps, unbiased, rep, t);
  if (!in) t = GTally();
  t.wave_sum();
  if ((threadIdx.x & 63u) == 0u) t.flush(rep);
}

template <int KT>
__global__ __launch_bounds__(TPB) void k_gquot_raw(const int32_t* mode, const int64_t* raw, const int64_t* mx,
                                                   const int64_t* mn, int64_t n, int ulps, int64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  double r, b;
  params(mode[i], mx[i], mn[i], ulps, 0, &r, &b);
  out[i] = mode[i] == 3   ? total_of<KT>(norm_term<KT, 3>(raw[i], r, b))
           : mode[i] == 1 ? total_of<KT>(norm_term<KT, 1>(raw[i], r, b))
                          : total_of<KT>(norm_term<KT, 2>(raw[i], r, b));
}

// col_term on the host's operands; the weight and the result as the key's bits
template <int KT>
__global__ __launch_bounds__(TPB) void k_term_raw(const double* v, const double* b, const double* r, const u64* cw,
                                                  int64_t n, int sub, u64* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = bits_key<KT>(sub ? msh::col_term<KT, true>(v[i], b[i], r[i], key_bits<KT>(cw[i]))
                            : msh::col_term<KT, false>(v[i], b[i], r[i], key_bits<KT>(cw[i])));
}

template <int KT>
__global__ __launch_bounds__(TPB) void k_key_mask_raw(const u64* t, const uint32_t* xm, const uint32_t* nt, int64_t n,
                                                      u64* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = bits_key<KT>(msh::key_mask<KT>(key_bits<KT>(t[i]), xm[i], nt[i]));
}

__global__ __launch_bounds__(TPB) void k_vmax_raw(const double* a, const double* b, int64_t n, double* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = msh::vmax_f64(a[i], b[i]);
}

// in[i][8] = (im, ix, ia, pd_valid, has_nn_score, nn_prescore, mode, weight); out[i][10] = decode_pod's (node, score,
// status), decode_ident's (modes 0 and 1; else -9), decode_classes' (tm, tx, status) for has_m = im >= 0 and
// has_x = ix >= 0, and whether decode_ident differs from decode_pod
constexpr int DEC_IN = 8, DEC_OUT = 10;
__global__ __launch_bounds__(TPB) void k_decode_raw(const int64_t* in, int64_t n, int64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int64_t* q = in + DEC_IN * i;
  int64_t* o = out + DEC_OUT * i;
  msh::PluginParams pp;
  pp.has_nu_filter = 1;
  pp.has_nn_score = (int32_t)q[4];
  pp.nn_prescore = (int32_t)q[5];
  pp.mode = (int32_t)q[6];
  pp.weight = q[7];
  const bool pdv = q[3] != 0;
  int32_t idx, st;
  int64_t sc;
  msh::decode_pod(q[0], q[1], q[2], pdv, pp, &idx, &sc, &st);
  o[0] = idx;
  o[1] = sc;
  o[2] = st;
  o[3] = o[4] = o[5] = -9;
  o[9] = 0;
  if (pp.mode <= 1) {
    int32_t idx2, st2;
    int64_t sc2;
    msh::decode_ident(q[0], q[2], pdv, msh::make_ident_decode(pp), &idx2, &sc2, &st2);
    o[3] = idx2;
    o[4] = sc2;
    o[5] = st2;
    o[9] = idx2 != idx || sc2 != sc || st2 != st;
  }
  int64_t tm, tx;
  msh::decode_classes(q[0] >= 0, q[1] >= 0, pdv, pp, &tm, &tx, &st);
  o[6] = tm;
  o[7] = tx;
  o[8] = st;
}

__global__ __launch_bounds__(TPB) void k_lowbit_raw(const uint32_t* x, int64_t n, uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = msh::lowbit(x[i]);
}

// h[i][PLANE_GW]: a group's hit words (one of them set: hits_first's contract)
__global__ __launch_bounds__(TPB) void k_hits_first_raw(const uint32_t* h, const uint32_t* g, int64_t n,
                                                        uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  uint32_t w[msh::PLANE_GW];
#pragma unroll
  for (int c = 0; c < msh::PLANE_GW; ++c) w[c] = h[msh::PLANE_GW * i + c];
  out[i] = msh::hits_first(w, g[i]);
}

// out[f][n], f in msh_device.h's order of the seven bop3_* forms
constexpr int BOP3_FORMS = 7;
__global__ __launch_bounds__(TPB) void k_bop3_raw(const uint32_t* a, const uint32_t* b, const uint32_t* c, int64_t n,
                                                  uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[0 * n + i] = msh::bop3_andn(a[i], b[i]);
  out[1 * n + i] = msh::bop3_and3(a[i], b[i], c[i]);
  out[2 * n + i] = msh::bop3_or_andn(a[i], b[i], c[i]);
  out[3 * n + i] = msh::bop3_andn_and(a[i], b[i], c[i]);
  out[4 * n + i] = msh::bop3_or_xor(a[i], b[i], c[i]);
  out[5 * n + i] = msh::bop3_andn_of_and(a[i], b[i], c[i]);
  out[6 * n + i] = msh::bop3_or_and(a[i], b[i], c[i]);
}

// ---- host plumbing: n elements per input array, outputs of out_bytes ----
struct In {
  const void* host;
  size_t bytes;
};
template <int NIN, class Launch>
hipError_t run_raw(const In (&in)[NIN], void* out, size_t out_bytes, Launch launch) {
  Dev d;
  void* din[NIN];
  void* dout;
  for (int k = 0; k < NIN; ++k) PROBE_TRY(d.put(&din[k], in[k].host, in[k].bytes));
  PROBE_TRY(d.get(&dout, out_bytes));
  PROBE_TRY(hipMemset(dout, 0xEE, out_bytes));
  launch(din, dout);
  return finish(out, dout, out_bytes);
}

#define KT_SWITCH(kt, CALL) \
  switch (kt) {             \
    case 0: CALL(0); break; \
    case 1: CALL(1); break; \
    default: CALL(2); break; \
  }

}  // namespace

extern "C" {

int msh_gprobe_rep_words(void) { return G_WORDS; }

// kt 0, 1, 2: the key type. The divisors ds[nd], or every d in [d_lo, d_lo + nd) when ds is null.
int msh_gprobe_quot(int kt, const uint64_t* ds, uint64_t d_lo, int64_t nd, int ulps, int unbiased, uint64_t* rep) {
  if (kt < 0 || kt > 2 || nd < 0) return hipErrorInvalidValue;
  Dev d;
  u64 *drep, *dds = nullptr;
  PROBE_TRY(d.get((void**)&drep, G_WORDS * sizeof(u64)));
  PROBE_TRY(hipMemset(drep, 0, G_WORDS * sizeof(u64)));
  if (ds) PROBE_TRY(d.put((void**)&dds, ds, nd * sizeof(u64)));
  if (nd > 0) {
#define CALL(K) hipLaunchKernelGGL(k_gquot<K>, dim3(blocks(nd)), dim3(TPB), 0, 0, dds, (u64)d_lo, nd, ulps, unbiased, drep)
    KT_SWITCH(kt, CALL)
#undef CALL
  }
  return finish(rep, drep, G_WORDS * sizeof(u64));
}

int msh_gprobe_quot_raw(int kt, const int32_t* mode, const int64_t* raw, const int64_t* mx, const int64_t* mn,
                        int64_t n, int ulps, int64_t* out) {
  if (kt < 0 || kt > 2) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  const In in[4] = {{mode, n * sizeof(int32_t)}, {raw, n * sizeof(int64_t)}, {mx, n * sizeof(int64_t)},
                    {mn, n * sizeof(int64_t)}};
  return run_raw(in, out, n * sizeof(int64_t), [&](void** p, void* o) {
#define CALL(K)                                                                                                    \
  hipLaunchKernelGGL(k_gquot_raw<K>, dim3(blocks(n)), dim3(TPB), 0, 0, (const int32_t*)p[0], (const int64_t*)p[1], \
                     (const int64_t*)p[2], (const int64_t*)p[3], n, ulps, (int64_t*)o)
    KT_SWITCH(kt, CALL)
#undef CALL
  });
}

int msh_gprobe_term_raw(int kt, int sub, const double* v, const double* b, const double* r, const uint64_t* cw,
                        int64_t n, uint64_t* out) {
  if (kt < 0 || kt > 2) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  const In in[4] = {{v, n * sizeof(double)}, {b, n * sizeof(double)}, {r, n * sizeof(double)}, {cw, n * sizeof(u64)}};
  return run_raw(in, out, n * sizeof(u64), [&](void** p, void* o) {
#define CALL(K)                                                                                                 \
  hipLaunchKernelGGL(k_term_raw<K>, dim3(blocks(n)), dim3(TPB), 0, 0, (const double*)p[0], (const double*)p[1], \
                     (const double*)p[2], (const u64*)p[3], n, sub, (u64*)o)
    KT_SWITCH(kt, CALL)
#undef CALL
  });
}

int msh_gprobe_key_mask_raw(int kt, const uint64_t* t, const uint32_t* xm, const uint32_t* nt, int64_t n,
                            uint64_t* out) {
  if (kt < 0 || kt > 2) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  const In in[3] = {{t, n * sizeof(u64)}, {xm, n * sizeof(uint32_t)}, {nt, n * sizeof(uint32_t)}};
  return run_raw(in, out, n * sizeof(u64), [&](void** p, void* o) {
#define CALL(K)                                                                                                \
  hipLaunchKernelGGL(k_key_mask_raw<K>, dim3(blocks(n)), dim3(TPB), 0, 0, (const u64*)p[0], (const uint32_t*)p[1], \
                     (const uint32_t*)p[2], n, (u64*)o)
    KT_SWITCH(kt, CALL)
#undef CALL
  });
}

int msh_gprobe_vmax_raw(const double* a, const double* b, int64_t n, double* out) {
  if (n <= 0) return hipSuccess;
  const In in[2] = {{a, n * sizeof(double)}, {b, n * sizeof(double)}};
  return run_raw(in, out, n * sizeof(double), [&](void** p, void* o) {
    hipLaunchKernelGGL(k_vmax_raw, dim3(blocks(n)), dim3(TPB), 0, 0, (const double*)p[0], (const double*)p[1], n,
                       (double*)o);
  });
}

int msh_gprobe_decode_cols(int* in_cols, int* out_cols) {
  *in_cols = DEC_IN;
  *out_cols = DEC_OUT;
  return 0;
}

int msh_gprobe_decode_raw(const int64_t* in, int64_t n, int64_t* out) {
  if (n <= 0) return hipSuccess;
  const In ins[1] = {{in, DEC_IN * n * sizeof(int64_t)}};
  return run_raw(ins, out, DEC_OUT * n * sizeof(int64_t), [&](void** p, void* o) {
    hipLaunchKernelGGL(k_decode_raw, dim3(blocks(n)), dim3(TPB), 0, 0, (const int64_t*)p[0], n, (int64_t*)o);
  });
}

int msh_gprobe_lowbit_raw(const uint32_t* x, int64_t n, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  const In in[1] = {{x, n * sizeof(uint32_t)}};
  return run_raw(in, out, n * sizeof(uint32_t), [&](void** p, void* o) {
    hipLaunchKernelGGL(k_lowbit_raw, dim3(blocks(n)), dim3(TPB), 0, 0, (const uint32_t*)p[0], n, (uint32_t*)o);
  });
}

// h[n][8] hit words, g[n] group numbers; the words per group and the nodes per group for the host
int msh_gprobe_group_shape(int* words, int* nodes) {
  *words = msh::PLANE_GW;
  *nodes = msh::GROUP_NODES;
  return 0;
}

int msh_gprobe_hits_first_raw(const uint32_t* h, const uint32_t* g, int64_t n, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  const In in[2] = {{h, msh::PLANE_GW * n * sizeof(uint32_t)}, {g, n * sizeof(uint32_t)}};
  return run_raw(in, out, n * sizeof(uint32_t), [&](void** p, void* o) {
    hipLaunchKernelGGL(k_hits_first_raw, dim3(blocks(n)), dim3(TPB), 0, 0, (const uint32_t*)p[0],
                       (const uint32_t*)p[1], n, (uint32_t*)o);
  });
}

// out[7][n]: andn(a, b), and3, or_andn, andn_and, or_xor, andn_of_and, or_and of (a, b, c)
int msh_gprobe_bop3_raw(const uint32_t* a, const uint32_t* b, const uint32_t* c, int64_t n, uint32_t* out) {
  if (n <= 0) return hipSuccess;
  const In in[3] = {{a, n * sizeof(uint32_t)}, {b, n * sizeof(uint32_t)}, {c, n * sizeof(uint32_t)}};
  return run_raw(in, out, BOP3_FORMS * n * sizeof(uint32_t), [&](void** p, void* o) {
    hipLaunchKernelGGL(k_bop3_raw, dim3(blocks(n)), dim3(TPB), 0, 0, (const uint32_t*)p[0], (const uint32_t*)p[1],
                       (const uint32_t*)p[2], n, (uint32_t*)o);
  });
}

}  // extern "C"
