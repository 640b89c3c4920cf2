// msh_seq_spread.hip — the topology-spread form of the sequential-commit kernel (msh_schedule_sequential_spread):
// seq_fit_kernel's frame (msh_seq_frame.h: thread t holds NPL consecutive nodes with their free amounts, remaining
// pod count, codes and availability bits; pods arrive by readlane from the 64-pod block the lanes loaded; one
// LDS-only barrier per pod with more than one wave) with upstream's PodTopologySpread filter (DoNotSchedule) as
// one more conjunct. It is the first conjunct here that one commit changes for many nodes at once: every node of
// the chosen zone and, through the minimum, every node of every zone.
// The kernel body is still a copy of the frame, not a policy on it. Written as FirstFeasible with the conjunct as
// hooks it gave the same results, but the compiler then dropped the branch that lets a wave none of whose lanes
// holds a candidate node skip that node's compares, and the C5 launches ran 2.2-3.1% slower (151.9 against 147.3 ms
// ungrouped, 170.6 against 166.9 ms grouped, profiles/seq_frame_refactor.json). The reduction, the launcher ladder
// and the table-limit message are the frame header's.
//  * zone ids: each thread packs the zone ids of its NPL nodes into one 64-bit register pair, 8 bits per node,
//    and keeps one bit per node for "has a zone" (hz). A node without a zone holds id 0 and a clear hz bit; a
//    grouped pod's availability bits are ANDed with hz, so such a node never tests as allowed, whatever the mask.
//  * counts: cnt[g][z] (G x 64 int32, 32 KB at G = 128) and max_skew[g] live in LDS for the launch: the prologue
//    loads them, the epilogue writes cnt back.
//  * per grouped pod (g wave-uniform, from the lanes that loaded the block; any value outside [0, G) was turned
//    into -1 there, so LDS is never indexed with it): lane z reads cnt[g][z]; lanes outside Zset contribute
//    INT32_MAX to a wave minimum (wave_reduce); allowed = ballot(z in Zset && cnt - minc <=
//    max_skew - 1) is one 64-bit wave-uniform mask, and per node the extra conjunct is (allowed >> zone) & 1. No
//    per-lane gather of cnt[g][zone(node)]. An ungrouped pod takes allowed = ~0 and every hz bit set.
//  * the commit: the thread that holds the selected node knows its zone and adds 1 to cnt[g][zone].
// The race, and what is done about it. With NW > 1 the frame has one barrier per pod: pod j's commit is written
// after barrier j, in the interval in which the other waves read pod j + 1's row. So a step whose pod is grouped
// and PLACED (both workgroup-uniform: every thread decodes the same status) ends with a second lds_barrier()
// after the commit; a step that commits nothing to cnt writes nothing and needs none. Every read of a row is
// then separated from every write of it by a barrier. With one wave the LDS operations of the wave are in order
// and no barrier is needed.
// Table limits and instances are seq_fit_kernel's: NPL = 8 for up to two resources (8,192 nodes), 4 for three or
// four (4,096); a table of no, one or three resources runs the next larger instance with zero requests.
#include "msh_seq_frame.h"

namespace msh {

template <int NR, int NPL, int NW, bool KX>
__global__ __launch_bounds__(NW * WAVE) void seq_spread_kernel(SpreadArgs sa) {
  static_assert(32 % NPL == 0 && NPL * 4 <= 32 && NPL <= 8, "a thread's nodes lie in one word, their zones in 64 bits");
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ uint32_t xs[3][3];      // [slot][first match, first feasible, first feasible non-match]
  extern __shared__ int32_t lcnt[];  // [G][SPREAD_ZONES] counts, then [G] max_skew
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

  int64_t fr[NR][NPL];
  int32_t rem[NPL];
  uint32_t codes = 0xFFFFFFFFu;  // code 15: never a match
  uint32_t av0 = 0u, av1 = 0u;
  uint64_t zones = 0ull;  // node k's zone id in bits 8k .. 8k + 5
  uint32_t hz = 0u;       // bit k: node k has a zone
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    rem[k] = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) fr[r][k] = 0;
  }
  if (held) {
    const int32_t w = i0 >> 5, sh = i0 & 31;
    const uint32_t* g = a.planes + (size_t)(w / PLANE_GW) * GROUP_DWORDS + w % PLANE_GW;
    const uint32_t d0 = (g[0] >> sh) & KMASK, d1 = (g[PLANE_GW] >> sh) & KMASK;
    const uint32_t d2 = (g[2 * PLANE_GW] >> sh) & KMASK, d3 = (g[3 * PLANE_GW] >> sh) & KMASK;
    av1 = (g[PLANE_V * PLANE_GW] >> sh) & KMASK;
    av0 = av1 & ~(g[PLANE_X * PLANE_GW] >> sh);
    codes = 0u;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      codes |= (((d0 >> k) & 1u) | (((d1 >> k) & 1u) << 1) | (((d2 >> k) & 1u) << 2) | (((d3 >> k) & 1u) << 3)) << (4 * k);
      const int32_t i = i0 + k;
      int32_t c = a.counts[i];
      if (a.fold) {
        for (int q = 1; q < a.count_replicas; ++q) {
          c += a.counts[q * a.count_stride + i];
          a.counts[q * a.count_stride + i] = 0;
        }
      }
      rem[k] = (a.cap ? min(a.cap[i], max_pods) : max_pods) - c;
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nres) fr[r][k] = fa.alloc[r * fa.res_stride + i] - fa.used[r * fa.res_stride + i];
      const int32_t z = sa.zone[i];
      const bool has = z >= 0 && z < SPREAD_ZONES;
      zones |= (uint64_t)(has ? (uint32_t)z : 0u) << (8 * k);
      hz |= (has ? 1u : 0u) << k;
    }
  }
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) lcnt[e] = sa.cnt[e];
  for (int32_t e = t; e < G; e += NW * WAVE) lskew[e] = sa.max_skew[e];
  if (NW > 1 && threadIdx.x < 9) (&xs[0][0])[threadIdx.x] = NONE;
  __syncthreads();
  int sl = 0;

  PluginParams pp = a.pp;
  const IdentDecode idec = make_ident_decode(pp);
  const uint32_t base = (uint32_t)i0;
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
      const uint32_t pc = pk & 15u;
      const int32_t pg = __builtin_amdgcn_readlane(gv, jl);  // in [-1, G)
      int64_t rq[NR];
      bool zr[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(rlo[r], jl);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(rhi[r], jl);
        rq[r] = (int64_t)(((uint64_t)hi << 32) | lo);
        zr[r] = rq[r] == 0;
      }
      uint32_t av = (pk & 16u) ? av0 : av1;
      unsigned long long allowed = ~0ull;
      if (pg >= 0) {  // wave-uniform
        const int32_t c = lcnt[pg * SPREAD_ZONES + lane];
        const int32_t skew = __builtin_amdgcn_readfirstlane(lskew[pg]);
        const int32_t minc = wave_reduce(in_zset ? c : INT32_MAX, [](int32_t x, int32_t y) { return min(x, y); });
        // cnt + 1 - minc <= max_skew without leaving int32: 0 <= minc <= c on a lane of Zset, 1 <= max_skew
        allowed = __ballot(in_zset && c - minc <= skew - 1);
        av &= hz;
      }
      uint32_t cm = NONE, ca = NONE, cx = NONE;
#pragma unroll
      for (int k = NPL - 1; k >= 0; --k) {  // descending: the lane's first node wins
        const uint32_t zk = (uint32_t)(zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1);
        bool ok = ((av >> k) & 1u) != 0 && rem[k] > 0 && ((allowed >> zk) & 1ull) != 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) ok = ok && (zr[r] || rq[r] <= fr[r][k]);
        const bool mt = ((codes >> (4 * k)) & 15u) == pc;
        ca = ok ? base + (uint32_t)k : ca;
        cm = (ok && mt) ? base + (uint32_t)k : cm;
        if (KX) cx = (ok && !mt) ? base + (uint32_t)k : cx;
      }
      cm = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_first(cm));
      ca = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_first(ca));
      if (KX) cx = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_first(cx));
      if constexpr (NW > 1) {
        if (lane == 0) {
          atomicMin(&xs[sl][0], cm);
          atomicMin(&xs[sl][1], ca);
          if (KX) atomicMin(&xs[sl][2], cx);
        }
        lds_barrier();
        cm = (uint32_t)__builtin_amdgcn_readfirstlane((int)xs[sl][0]);
        ca = (uint32_t)__builtin_amdgcn_readfirstlane((int)xs[sl][1]);
        if (KX) cx = (uint32_t)__builtin_amdgcn_readfirstlane((int)xs[sl][2]);
        // the slot read one step ago is free now (every reader passed this step's barrier) and is next
        // folded into two steps ahead (after the next barrier): wave 0 resets it in between
        if (threadIdx.x < 3) xs[sl == 0 ? 2 : sl - 1][threadIdx.x] = NONE;
        sl = sl == 2 ? 0 : sl + 1;
      }
      const int64_t im = cm != NONE ? (int64_t)cm : -1;
      const int64_t ia = ca != NONE ? (int64_t)ca : -1;
      int32_t sel, st;
      int64_t sc;
      if (KX) decode_pod(im, cx != NONE ? (int64_t)cx : -1, ia, pc != CODE_NONE_POD, pp, &sel, &sc, &st);
      else decode_ident(im, ia, pc != CODE_NONE_POD, idec, &sel, &sc, &st);
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
              rem[k] -= 1;
#pragma unroll
              for (int r = 0; r < NR; ++r) fr[r][k] -= rq[r];
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
      a.counts[i] = (a.cap ? min(a.cap[i], max_pods) : max_pods) - rem[k];
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nres) fa.used[r * fa.res_stride + i] = fa.alloc[r * fa.res_stride + i] - fr[r][k];
    }
  }
  __syncthreads();
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) sa.cnt[e] = lcnt[e];
}

namespace {
struct SpreadFamily {
  static constexpr int NPL2 = 8, NPL4 = 4;  // seq_fit_kernel's
  template <int NR, int NPL, int NW>
  static auto kernel(const SpreadArgs& a) {
    return needs_kx(a.f.s.pp) ? seq_spread_kernel<NR, NPL, NW, true> : seq_spread_kernel<NR, NPL, NW, false>;
  }
};
}  // namespace

int32_t seq_spread_max_nodes(int32_t nres) { return seq_frame_max_nodes<SpreadFamily>(nres); }

hipError_t launch_seq_spread(const SpreadArgs& a, hipStream_t s, std::string* err) {
  if (a.f.s.n_pods == 0) return hipSuccess;
  if (a.n_groups < 0 || a.n_groups > SPREAD_MAX_GROUPS) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.n_groups * (SPREAD_ZONES + 1) * sizeof(int32_t);  // at most 33,280 bytes
  return launch_seq_frame<SpreadFamily>(a, a.f, "topology-spread", lds, s, err);
}

}  // namespace msh
