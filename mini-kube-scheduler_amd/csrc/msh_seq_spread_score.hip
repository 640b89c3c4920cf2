// msh_seq_spread_score.hip — the scored topology-spread form of the sequential-commit kernel
// (msh_schedule_sequential_spread_scored on a ctx whose msh_set_resource_score mode is LEAST_ALLOCATED or
// MOST_ALLOCATED): seq_spread_kernel's feasible set (msh_seq_spread.hip: upstream's PodTopologySpread filter,
// DoNotSchedule, as one more conjunct) with seq_score_kernel's totals and arg-max (msh_seq_score.hip: NodeNumber's
// total plus weight x the LeastAllocated / MostAllocated score, the first maximum in List order).
// The score half is ScoreArgmax itself (msh_seq_score_policy.h): its per-node state (al, rc), its eval (the packed
// keys (RS + 1) << 16 | (0xFFFF - node) of the best match and the best non-match, the wave maximum by wave_reduce),
// its LDS atomicMax meet and its decode (decode_classes and the comparison of the two totals). Nothing of it is
// repeated here. The body around it is the frame's (msh_seq_frame.h) with seq_spread_kernel's additions, written
// out as that kernel's is: the frame header has no hooks for a further pod column, a per-pod mask or a commit to
// LDS, and adding them would have touched the three kernels that are built on it.
//  * zone ids: 8 bits per node in one 64-bit register pair, and the has-a-zone bits hz, as in seq_spread_kernel
//    (NPL <= 4 here, so 32 bits would do; the pair costs one register and keeps the two kernels' code alike).
//  * counts: cnt[g][z] and max_skew[g] in dynamic LDS for the launch (G x 260 bytes), loaded by the prologue,
//    cnt written back by the epilogue.
//  * per grouped pod (g wave-uniform; a value outside [0, G) became -1 when the lanes loaded the block, so LDS is
//    never indexed with a pod's raw value): lane z reads cnt[g][z], one wave minimum over the lanes of Zset, one
//    ballot gives the 64-bit mask `allowed`. The conjunct (allowed >> zone(k)) & 1 enters ScoreArgmax::eval's `ok`
//    through the pod's availability bits: av &= hz & (the allowed bits of the lane's NPL nodes), NPL shifts of a
//    64-bit value per grouped pod. An ungrouped pod skips all of it on a uniform branch.
//  * NodeNumber's normalizer extents come from which classes have a feasible node (decode_classes), so they are
//    taken over the spread-filtered list without further work.
//  * the commit: the frame's, and the thread that holds the selected node adds 1 to cnt[g][zone].
// The race is seq_spread_kernel's and so is the answer: a step whose pod is grouped and PLACED (both
// workgroup-uniform) ends with a second lds_barrier() after the commit when NW > 1, a wavefront fence with one
// wave. The two-copy count scheme that would remove the second barrier was not tried here either.
// Table limits and instances are seq_score_kernel's: NPL = 4 for up to two resources (4,096 nodes), 2 for three or
// four (2,048), on 1, 4 or 16 waves; a table of one or three resources runs the next larger instance.
#include "msh_seq_score_policy.h"

namespace msh {

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_spread_score_kernel(SpreadScoreArgs ssa) {
  static_assert(32 % NPL == 0 && NPL <= 8, "a thread's nodes lie in one word, their zones in 64 bits");
  using P = ScoreArgmax<NR, NPL, MOST>;
  constexpr int K = P::K;
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ uint32_t xs[3][P::SLOT];
  extern __shared__ int32_t lcnt[];  // [G][SPREAD_ZONES] counts, then [G] max_skew
  const SpreadArgs& sa = ssa.s;
  const FitArgs& fa = sa.f;
  const SeqArgs& a = fa.s;
  const int lane = threadIdx.x & (WAVE - 1);
  const int32_t t = (int32_t)threadIdx.x;
  const int32_t slots = a.n_words * 32;
  const int32_t i0 = t * NPL;
  const bool held = i0 < slots;  // then all NPL nodes are slots of the table (NPL divides 32)
  const int32_t nres = fa.nres;
  const int32_t max_pods = a.max_pods;
  const int32_t G = sa.n_groups;
  int32_t* lskew = lcnt + G * SPREAD_ZONES;
  const bool in_zset = ((sa.zset >> lane) & 1ull) != 0;  // lane z: zone z occurs on a node

  P p(a.pp, ssa.weight, ssa.rw, ssa.wsum_magic);
  FrameNodes<NR, NPL> n;
  n.i0 = i0;
  uint64_t zones = 0ull;  // node k's zone id in bits 8k .. 8k + 5
  uint32_t hz = 0u;       // bit k: node k has a zone
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    n.rem[k] = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) n.fr[r][k] = 0;
  }
  if (held) {
    const int32_t w = i0 >> 5, sh = i0 & 31;
    const uint32_t* g = a.planes + (size_t)(w / PLANE_GW) * GROUP_DWORDS + w % PLANE_GW;
    const uint32_t d0 = (g[0] >> sh) & KMASK, d1 = (g[PLANE_GW] >> sh) & KMASK;
    const uint32_t d2 = (g[2 * PLANE_GW] >> sh) & KMASK, d3 = (g[3 * PLANE_GW] >> sh) & KMASK;
    n.av1 = (g[PLANE_V * PLANE_GW] >> sh) & KMASK;
    n.av0 = n.av1 & ~(g[PLANE_X * PLANE_GW] >> sh);
    n.codes = 0u;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      n.codes |= (((d0 >> k) & 1u) | (((d1 >> k) & 1u) << 1) | (((d2 >> k) & 1u) << 2) | (((d3 >> k) & 1u) << 3)) << (4 * k);
      const int32_t i = i0 + k;
      int32_t c = a.counts[i];
      if (a.fold) {
        for (int q = 1; q < a.count_replicas; ++q) {
          c += a.counts[q * a.count_stride + i];
          a.counts[q * a.count_stride + i] = 0;
        }
      }
      n.rem[k] = (a.cap ? min(a.cap[i], max_pods) : max_pods) - c;
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nres) {
          const int64_t al = fa.alloc[r * fa.res_stride + i];
          n.fr[r][k] = al - fa.used[r * fa.res_stride + i];
          p.node_res(r, k, al);
        }
      const int32_t z = sa.zone[i];
      const bool has = z >= 0 && z < SPREAD_ZONES;
      zones |= (uint64_t)(has ? (uint32_t)z : 0u) << (8 * k);
      hz |= (has ? 1u : 0u) << k;
    }
  }
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) lcnt[e] = sa.cnt[e];
  for (int32_t e = t; e < G; e += NW * WAVE) lskew[e] = sa.max_skew[e];
  if (NW > 1 && threadIdx.x < 3 * P::SLOT) (&xs[0][0])[threadIdx.x] = P::IDENT;
  __syncthreads();
  int sl = 0;

  const int32_t n_pods = a.n_pods;
  // Pods in lanes, 64 at a time (every wave loads the block), one block ahead; clamped index: no branch
  int32_t dn = 0, tn = 0, gn = -1;
  int64_t rn[NR];
  auto load_raw = [&](int32_t j0) {
    const int32_t jj = min(j0 + lane, n_pods - 1);
    dn = a.pod_digit[jj];
    tn = a.pod_tol[jj];
    gn = sa.pod_group[jj];
#pragma unroll
    for (int r = 0; r < NR; ++r) rn[r] = r < nres ? fa.pod_req[(int64_t)r * n_pods + jj] : 0;
  };
  load_raw(0);
  for (int32_t jb = 0; jb < n_pods; jb += WAVE) {
    // this block's lane values: the code | ~tolerates << 4, the group (anything outside [0, G): -1, ungrouped)
    // and the requests' halves
    const bool dig = dn >= 0 && dn <= 9;
    const uint32_t pkv = (dig ? (uint32_t)dn : CODE_NONE_POD) | (tn != 0 ? 0u : 16u);
    const int32_t gv = (uint32_t)gn < (uint32_t)G ? gn : -1;
    int32_t rlo[NR], rhi[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      rlo[r] = (int32_t)(uint32_t)((uint64_t)rn[r] & 0xFFFFFFFFull);
      rhi[r] = (int32_t)(uint32_t)((uint64_t)rn[r] >> 32);
    }
    load_raw(jb + WAVE);
    const int32_t je = min(jb + WAVE, n_pods);
    for (int32_t j = jb; j < je; ++j) {
      const int jl = j - jb;
      const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)pkv, jl);
      const int32_t pg = __builtin_amdgcn_readlane(gv, jl);  // in [-1, G)
      FramePod<NR> pod;
      pod.pc = pk & 15u;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(rlo[r], jl);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(rhi[r], jl);
        pod.rq[r] = (int64_t)(((uint64_t)hi << 32) | lo);
        pod.zr[r] = pod.rq[r] == 0;
      }
      pod.av = (pk & 16u) ? n.av0 : n.av1;
      if (pg >= 0) {  // wave-uniform
        const int32_t c = lcnt[pg * SPREAD_ZONES + lane];
        const int32_t skew = __builtin_amdgcn_readfirstlane(lskew[pg]);
        const int32_t minc = wave_reduce(in_zset ? c : INT32_MAX, [](int32_t x, int32_t y) { return min(x, y); });
        // cnt + 1 - minc <= max_skew without leaving int32: 0 <= minc <= c on a lane of Zset, 1 <= max_skew
        const unsigned long long allowed = __ballot(in_zset && c - minc <= skew - 1);
        uint32_t za = 0u;  // bit k: node k's zone is allowed
#pragma unroll
        for (int k = 0; k < NPL; ++k)
          za |= (uint32_t)((allowed >> ((uint32_t)(zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1))) & 1ull) << k;
        pod.av &= hz & za;
      }
      uint32_t v[K];
      p.eval(n, pod, v);
      if constexpr (NW > 1) {
        if (lane == 0) {
#pragma unroll
          for (int c = 0; c < K; ++c) P::meet(&xs[sl][c], v[c]);
        }
        lds_barrier();
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = (uint32_t)__builtin_amdgcn_readfirstlane((int)xs[sl][c]);
        // the slot read one step ago is free now and is next added to two steps ahead: wave 0 resets it in between
        if (threadIdx.x < P::SLOT) xs[sl == 0 ? 2 : sl - 1][threadIdx.x] = P::IDENT;
        sl = sl == 2 ? 0 : sl + 1;
      }
      int32_t sel, st;
      int64_t sc;
      p.decode(v, pod.pc, &sel, &sc, &st);
      if (t == 0) {
        a.out_idx[j] = sel;
        if (a.out_score) a.out_score[j] = sc;
        a.out_status[j] = st;
      }
      if (st == 0) {  // commit, seen by the next pod's decision: one pod and its requests off the node
        const int32_t own = sel / NPL, ks = sel % NPL;
        if (t == own) {
#pragma unroll
          for (int k = 0; k < NPL; ++k)
            if (k == ks) {
              asm volatile("");  // a scalar branch per k, not selects over all NPL nodes (see seq_frame)
              n.rem[k] -= 1;
#pragma unroll
              for (int r = 0; r < NR; ++r) n.fr[r][k] -= pod.rq[r];
            }
          // a grouped pod was placed on a node with a zone (hz): one more pod of the group in that zone
          if (pg >= 0) lcnt[pg * SPREAD_ZONES + ((uint32_t)(zones >> (8 * ks)) & (uint32_t)(SPREAD_ZONES - 1))] += 1;
        }
        if (pg >= 0) {  // workgroup-uniform: the write above and the next step's row reads, a barrier apart
          if constexpr (NW > 1) lds_barrier();
          else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
      }
    }
  }
  if (held) {
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int32_t i = i0 + k;
      a.counts[i] = (a.cap ? min(a.cap[i], max_pods) : max_pods) - n.rem[k];
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nres) fa.used[r * fa.res_stride + i] = p.alloc(fa, r, k, i) - n.fr[r][k];
    }
  }
  __syncthreads();
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) sa.cnt[e] = lcnt[e];
}

namespace {
struct SpreadScoreFamily {
  static constexpr int NPL2 = 4, NPL4 = 2;  // seq_score_kernel's
  template <int NR, int NPL, int NW>
  static auto kernel(const SpreadScoreArgs& a) {
    return a.most ? seq_spread_score_kernel<NR, NPL, NW, true> : seq_spread_score_kernel<NR, NPL, NW, false>;
  }
};
}  // namespace

int32_t seq_spread_score_max_nodes(int32_t nres) { return seq_frame_max_nodes<SpreadScoreFamily>(nres); }

hipError_t launch_seq_spread_score(const SpreadScoreArgs& a, hipStream_t s, std::string* err) {
  if (a.s.f.s.n_pods == 0) return hipSuccess;
  if (a.s.n_groups < 0 || a.s.n_groups > SPREAD_MAX_GROUPS || a.s.f.nres < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.s.n_groups * (SPREAD_ZONES + 1) * sizeof(int32_t);  // at most 33,280 bytes
  return launch_seq_frame<SpreadScoreFamily>(a, a.s.f, "scored topology-spread", lds, s, err);
}

}  // namespace msh
