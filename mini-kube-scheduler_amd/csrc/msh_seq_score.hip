// msh_seq_score.hip — the scored resource-fit form of the sequential-commit kernel: msh_schedule_sequential_fit on
// a ctx whose msh_set_resource_score mode is LEAST_ALLOCATED or MOST_ALLOCATED (upstream's
// NodeResourcesLeastAllocated / NodeResourcesMostAllocated, noderesources/least_allocated.go, most_allocated.go).
// Feasibility, status and the commit are seq_fit_kernel's (msh_seq_fit.hip); the total of a feasible node i for pod
// j is NodeNumber's total plus weight x RS(j, i),
//   q_r = used[r][i] + req[r][j], c_r = alloc[r][i],
//   s_r = 0 when c_r == 0 or q_r > c_r, else (c_r - q_r) * 100 / c_r (LEAST) or q_r * 100 / c_r (MOST),
//   RS  = (sum_r s_r * rw[r]) / (sum_r rw[r]),
// in int64 with truncating division, and the pod goes to the first maximum in List order. RS moves with every
// commit, so the reduction is an arg-max, not seq_fit_kernel's "first feasible node of a class". The frame is
// msh_seq_frame.h's; this file is its ScoreArgmax policy:
//  * besides the frame's free amounts alloc - used a thread keeps the allocatable amount c (the divisor,
//    loop-invariant) and 100 / c as a float, per node and resource, and writes used back from them;
//  * the numerator comes from what the lane holds: c - q = free - req (negative exactly when q > c), q = c - that;
//  * the quotient num * 100 / c (0..100) is a float estimate, float(num) x (100 / c), which is within 1 of the
//    quotient (relative error below 2^-21 against a quotient of at most 100), and one integer correction step on
//    the remainder num * 100 - s * c makes it exact. Amounts are at most 2^55, so num * 100 stays inside int64;
//  * the weighted mean divides by the launch-uniform sum of the resource weights (at most 400) by a multiply and a
//    shift (wsum_magic); a resource of weight 0 is skipped by a uniform branch;
//  * NodeNumber's part of a total has one value for the feasible matches and one for the feasible non-matches, and
//    the two depend only on which of the classes are present (decode_classes), so per pod it is enough to reduce
//    two packed keys, the best match and the best non-match: (RS + 1) << 16 | (0xFFFF - node), 0 = none. The
//    largest key is the largest RS and, among equals, the lowest node. Lanes take the maximum over their nodes, the
//    wave by DPP (wave_reduce), the workgroup by the frame's meet with an LDS atomic maximum;
//  * on the uniform path the two candidates' totals are compared: the larger wins, the lower node at a tie.
// Table limit: 16 waves x 64 lanes x NPL nodes with NPL = 4 up to two resources (4,096 nodes) and 2 for three or
// four (2,048), half of seq_fit_kernel's: the allocatable amounts double a node's registers
// (msh_seq_fit_max_nodes reports both).
#include "msh_seq_frame.h"

namespace msh {

namespace {
// num * 100 / c for 0 <= num <= c, 1 <= c <= 2^55, rc = 100 / c rounded to float.
__device__ __forceinline__ uint32_t quot100(int64_t num, int64_t c, float rc) {
  const uint32_t lo = (uint32_t)((uint64_t)num & 0xFFFFFFFFull), hi = (uint32_t)((uint64_t)num >> 32);
  const float nf = __builtin_fmaf((float)hi, 4294967296.0f, (float)lo);
  uint32_t s = (uint32_t)(nf * rc);                           // within 1 of the quotient
  const int64_t rm = num * 100 - (int64_t)(uint64_t)s * c;  // in [-c, 2c)
  s += rm >= c ? 1u : 0u;
  s -= rm < 0 ? 1u : 0u;
  return s;
}

template <int NR, int NPL, bool MOST>
struct ScoreArgmax : FramePolicy {
  static constexpr int K = 2, SLOT = 2;  // [best match key, best non-match key]
  static constexpr uint32_t IDENT = 0u;
  __device__ static __forceinline__ void meet(uint32_t* slot, uint32_t v) { atomicMax(slot, v); }

  const PluginParams pp;
  const int64_t weight;
  const uint32_t magic;
  uint32_t rw[NR];
  int64_t al[NR][NPL];
  float rc[NR][NPL];
  __device__ __forceinline__ explicit ScoreArgmax(const FitScoreArgs& sa)
      : pp(sa.f.s.pp), weight(sa.weight), magic(sa.wsum_magic) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      rw[r] = (uint32_t)sa.rw[r];
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        al[r][k] = 0;
        rc[r][k] = 0.0f;
      }
    }
  }

  __device__ __forceinline__ void node_res(int r, int k, int64_t alloc) {
    al[r][k] = alloc;
    rc[r][k] = alloc > 0 ? 100.0f / (float)alloc : 0.0f;
  }
  __device__ __forceinline__ int64_t alloc(const FitArgs&, int r, int k, int32_t) const { return al[r][k]; }

  __device__ __forceinline__ void eval(const FrameNodes<NR, NPL>& n, const FramePod<NR>& pod, uint32_t (&v)[K]) const {
    const uint32_t kbase = 0xFFFFu - (uint32_t)n.i0;  // node i0 + k packs as kbase - k
    uint32_t km = 0u, kx = 0u;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      bool ok = ((pod.av >> k) & 1u) != 0 && n.rem[k] > 0;
      uint32_t acc = 0u;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t d = n.fr[r][k] - pod.rq[r];  // c - q
        ok = ok && (pod.zr[r] || d >= 0);
        if (rw[r] != 0u) {  // launch-uniform
          const int64_t c = al[r][k];
          const bool none = c == 0 || d < 0;  // upstream: capacity 0 or requested > capacity scores 0
          const int64_t num = none ? 0 : (MOST ? c - d : d);
          const uint32_t s = quot100(num, c, rc[r][k]);
          acc += (none ? 0u : s) * rw[r];
        }
      }
      const uint32_t rs = __umulhi(acc * 2u, magic);  // acc / sum of the weights
      const uint32_t key = ok ? (((rs + 1u) << 16) | (kbase - (uint32_t)k)) : 0u;
      const bool mt = ((n.codes >> (4 * k)) & 15u) == pod.pc;
      km = umax(km, mt ? key : 0u);
      kx = umax(kx, mt ? 0u : key);
    }
    v[0] = wave_reduce(km, umax);
    v[1] = wave_reduce(kx, umax);
  }

  // the two candidates' totals are compared: the larger wins, the lower node at a tie
  __device__ __forceinline__ void decode(const uint32_t (&v)[K], uint32_t pc, int32_t* sel, int64_t* sc,
                                         int32_t* st) const {
    const uint32_t km = v[0], kx = v[1];
    const bool has_m = km != 0u, has_x = kx != 0u;
    int64_t tm, tx;
    decode_classes(has_m, has_x, pc != CODE_NONE_POD, pp, &tm, &tx, st);
    tm += weight * (int64_t)((km >> 16) - 1u);
    tx += weight * (int64_t)((kx >> 16) - 1u);
    const int32_t im = (int32_t)(0xFFFFu - (km & 0xFFFFu)), ix = (int32_t)(0xFFFFu - (kx & 0xFFFFu));
    const bool pick_m = has_m && (!has_x || tm > tx || (tm == tx && im < ix));
    *sel = *st == 0 ? (pick_m ? im : ix) : -1;
    *sc = *st == 0 ? (pick_m ? tm : tx) : 0;
  }
};
}  // namespace

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_score_kernel(FitScoreArgs sa) {
  ScoreArgmax<NR, NPL, MOST> p(sa);
  seq_frame<NR, NPL, NW>(sa.f, p);
}

namespace {
// nodes per thread, up to two resources and three or four: half of seq_fit_kernel's, since a node also keeps its
// allocatable amounts and their reciprocals (64 + 16 VGPRs of node state either way; with seq_fit_kernel's 8 / 4
// the 16-wave instances, 128 VGPRs per wave, spill 148-192 bytes per lane to scratch)
struct ScoreFamily {
  static constexpr int NPL2 = 4, NPL4 = 2;
  template <int NR, int NPL, int NW>
  static auto kernel(const FitScoreArgs& a) {
    return a.most ? seq_score_kernel<NR, NPL, NW, true> : seq_score_kernel<NR, NPL, NW, false>;
  }
};
}  // namespace

int32_t seq_score_max_nodes(int32_t nres) { return seq_frame_max_nodes<ScoreFamily>(nres); }

hipError_t launch_seq_score(const FitScoreArgs& a, hipStream_t s, std::string* err) {
  if (a.f.s.n_pods == 0) return hipSuccess;
  return launch_seq_frame<ScoreFamily>(a, a.f, "scored resource-fit", 0, s, err);
}

}  // namespace msh
