// msh_probe_host.cpp — test infrastructure: the host build of csrc/msh_seq_quot.h's pure integer code
// (libmsh_probe_host.so, no device code, no GPU call), the candidate filter of the soft_raw decider search of
// tests/test_quot_probe.py, and the double paths of csrc/msh_generic_norm.h (the 8-byte key types) over
// msh_gprobe.hip's numerators for tests/test_generic_probe.py: evidence about the arithmetic, not about the device.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#define MSH_GEN_HOST_ONLY
#include "../../mini-kube-scheduler_amd/csrc/msh_generic_norm.h"
#include "../../mini-kube-scheduler_amd/csrc/msh_seq_quot.h"

namespace {

constexpr int64_t RAW_LO = -(int64_t(1) << 31), RAW_HI = int64_t(1) << 31;

struct HTally {
  uint64_t mis = 0, misn = 0, seen = 0, first[6] = {0, 0, 0, 0, 0, 0};
  bool have = false;
};

template <int KT>
int64_t total_of(msh::GKey<KT> k) {
  if constexpr (KT == 2) return (int64_t)std::fmin(std::fmax(k, -0x1p62), 0x1p62);
  else return (int64_t)k;
}
template <int KT>
msh::GKey<KT> key_of(int64_t w) {
  if constexpr (KT == 2) return (double)w;
  else return (uint64_t)w;
}

template <int KT>
void quot_one(int mode, int64_t raw, int64_t mx, int64_t mn, double r, double b, HTally& t) {
  const double v = 100.0 * (double)raw;
  int64_t got, want;
  if (mode == 3) {
    got = total_of<KT>(msh::col_term<KT, true>(v, b, r, key_of<KT>(1)));
    want = (raw - mn) * 100 / (mx - mn);
  } else if (mode == 1) {
    got = total_of<KT>(msh::col_term<KT, false>(v, b, r, key_of<KT>(1)));
    want = 100 * raw / mx;
  } else {
    got = total_of<KT>(key_of<KT>(100) + msh::col_term<KT, false>(v, b, r, key_of<KT>(-1)));
    want = 100 - 100 * raw / mx;
  }
  const bool bad = got != want, badn = msh::gen_normalize(raw, mode, mx, mn) != want;
  t.seen += 1;
  t.mis += bad;
  t.misn += badn;
  if ((bad || badn) && !t.have) {
    const int64_t f[6] = {mode, raw, mx, mn, got, want};
    std::memcpy(t.first, f, sizeof f);
    t.have = true;
  }
}

template <int KT>
void sweep(int mode, uint64_t d, int64_t base, int64_t sign, int64_t mx, int64_t mn, double r, double b, HTally& t) {
  quot_one<KT>(mode, base, mx, mn, r, b, t);
  quot_one<KT>(mode, base + sign * (int64_t)d, mx, mn, r, b, t);
  for (uint64_t k = 0; k <= 100u; ++k) {
    const uint64_t a = (k * d + 99u) / 100u;
    if (a > 0u) quot_one<KT>(mode, base + sign * (int64_t)(a - 1u), mx, mn, r, b, t);
    quot_one<KT>(mode, base + sign * (int64_t)a, mx, mn, r, b, t);
    if (a < d) quot_one<KT>(mode, base + sign * (int64_t)(a + 1u), mx, mn, r, b, t);
  }
}

void params(int mode, int64_t mx, int64_t mn, int ulps, int unbiased, double* r, double* b) {
  msh::gen_norm_params(mode, mx, mn, r, b);
  if (unbiased) *r = 1.0 / (double)(mode == 3 ? mx - mn : mx);
  uint64_t bits;
  std::memcpy(&bits, r, 8);
  bits += (uint64_t)(int64_t)ulps;
  std::memcpy(r, &bits, 8);
}

// msh_gprobe.hip's k_gquot for one divisor (the 8-byte key types)
template <int KT>
void divisor(uint64_t d, int ulps, int unbiased, HTally& t) {
  const int64_t mns[3] = {RAW_LO, 0, RAW_HI - (int64_t)d};
  double r, b;
  for (int o = 0; o < 3; ++o) {
    if (o == 1 && d > (uint64_t)RAW_HI) continue;
    const int64_t mn = mns[o], mx = mn + (int64_t)d;
    params(3, mx, mn, ulps, unbiased, &r, &b);
    sweep<KT>(3, d, mn, 1, mx, mn, r, b, t);
  }
  for (int mode = 1; mode <= 2; ++mode) {
    const int64_t mx = (int64_t)d, mn = INT64_MAX;
    params(mode, mx, mn, ulps, unbiased, &r, &b);
    sweep<KT>(mode, d, 0, 1, mx, mn, r, b, t);
    sweep<KT>(mode, d, 0, -1, mx, mn, r, b, t);
    const uint64_t k0 = (100ull << 31) / d;
    const int64_t e = -(int64_t)((k0 * d + 99u) / 100u);
    for (int64_t o = 0; o < 3; ++o) {
      quot_one<KT>(mode, RAW_LO + o, mx, mn, r, b, t);
      quot_one<KT>(mode, std::max(e - 1 + o, RAW_LO), mx, mn, r, b, t);
    }
  }
}

}  // namespace

extern "C" {

// Every sum in 1..max_sum and acc in 0..100 sum: the count of acc / sum != wsum_div(acc, wsum_magic(sum)), the first
// one in first[3] = (acc, sum, got); out, when not null, as msh_probe_wsum's.
int64_t msh_host_wsum(uint32_t max_sum, uint32_t* first, uint32_t* out) {
  int64_t bad = 0;
  for (uint32_t sum = 1; sum <= max_sum; ++sum) {
    const uint32_t magic = msh::wsum_magic(sum);
    for (uint32_t acc = 0; acc <= 100u * sum; ++acc) {
      const uint32_t got = msh::wsum_div(acc, magic);
      if (out) out[50u * sum * (sum - 1u) + (sum - 1u) + acc] = got;
      if (got != acc / sum && bad++ == 0) {
        first[0] = acc;
        first[1] = sum;
        first[2] = got;
      }
    }
  }
  return bad;
}

uint32_t msh_host_wsum_magic(uint32_t sum) { return msh::wsum_magic(sum); }

// The counts c in [c_lo, c_hi] whose product fl(c w) has a fraction within eps of 0.5, into out[cap]; returns how
// many there are (more than cap: the list is cut).
int64_t msh_host_half_candidates(double w, int32_t c_lo, int32_t c_hi, double eps, int32_t* out, int64_t cap) {
  int64_t n = 0;
  for (int64_t c = c_lo; c <= c_hi; ++c) {
    const double x = (double)c * w;
    if (std::fabs(x - std::floor(x) - 0.5) <= eps) {
      if (n < cap) out[n] = (int32_t)c;
      ++n;
    }
  }
  return n;
}

int32_t msh_host_soft_raw(int32_t c, double w, int32_t skew1) { return msh::soft_raw(c, w, skew1); }

// msh_gprobe_quot's evaluations on the host for kt 1 or 2, over `threads` threads: rep[9] = (mismatches of the term,
// mismatches of gen_normalize, evaluations, the first mismatch as (mode, raw, mx, mn, got, want)). Divisors outside
// [1, 2^32] are passed over.
int msh_host_gquot(int kt, const uint64_t* ds, uint64_t d_lo, int64_t nd, int ulps, int unbiased, int threads,
                   uint64_t* rep) {
  if ((kt != 1 && kt != 2) || nd < 0 || threads < 1) return 1;
  std::vector<HTally> ts(threads);
  std::vector<std::thread> pool;
  for (int w = 0; w < threads; ++w)
    pool.emplace_back([&, w] {
      for (int64_t i = w; i < nd; i += threads) {
        const uint64_t d = ds ? ds[i] : d_lo + (uint64_t)i;
        if (d < 1u || d > (uint64_t(1) << 32)) continue;
        if (kt == 1) divisor<1>(d, ulps, unbiased, ts[w]);
        else divisor<2>(d, ulps, unbiased, ts[w]);
      }
    });
  for (auto& th : pool) th.join();
  std::memset(rep, 0, 9 * sizeof(uint64_t));
  bool have = false;
  for (const HTally& t : ts) {
    rep[0] += t.mis;
    rep[1] += t.misn;
    rep[2] += t.seen;
    if (t.have && !have) {
      std::memcpy(rep + 3, t.first, sizeof t.first);
      have = true;
    }
  }
  return 0;
}

}  // extern "C"
