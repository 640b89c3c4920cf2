// msh_probe_host.cpp — test infrastructure: the host build of csrc/msh_seq_quot.h's pure integer code
// (libmsh_probe_host.so, no device code, no GPU call), and the candidate filter of the soft_raw decider search of
// tests/test_quot_probe.py.
#include <cmath>
#include <cstdint>

#include "../../mini-kube-scheduler_amd/csrc/msh_seq_quot.h"

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

}  // extern "C"
