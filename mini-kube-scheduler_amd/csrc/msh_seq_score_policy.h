// msh_seq_score_policy.h — ScoreArgmax, the resource-score policy of the register-resident sequential-commit
// kernels: the per-node state and evaluation of upstream's NodeResourcesLeastAllocated / MostAllocated score on
// top of msh_seq_frame.h's node state. seq_score_kernel (msh_seq_score.hip) runs it on seq_frame;
// seq_spread_score_kernel (msh_seq_spread_score.hip) runs the same state, eval and decode inside its own body,
// with the topology-spread verdict folded into the pod's availability bits before eval. See msh_seq_score.hip for
// the arithmetic.
#pragma once

#include "msh_seq_frame.h"
#include "msh_seq_quot.h"

namespace msh {

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
  // weight, rw_[FIT_MAX_RES] and magic: FitScoreArgs' weight, rw and wsum_magic
  __device__ __forceinline__ ScoreArgmax(const PluginParams& pp_, int64_t weight_, const int32_t* rw_, uint32_t magic_)
      : pp(pp_), weight(weight_), magic(magic_) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      rw[r] = (uint32_t)rw_[r];
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        al[r][k] = 0;
        rc[r][k] = 0.0f;
      }
    }
  }
  __device__ __forceinline__ explicit ScoreArgmax(const FitScoreArgs& sa)
      : ScoreArgmax(sa.f.s.pp, sa.weight, sa.rw, sa.wsum_magic) {}

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
      const uint32_t rs = wsum_div(acc, magic);  // acc / sum of the weights
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

}  // namespace msh
