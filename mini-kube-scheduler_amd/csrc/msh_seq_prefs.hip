// msh_seq_prefs.hip — the preference form of the sequential-commit kernel (msh_schedule_sequential_prefs): the
// scored class form (msh_seq_classes.hip) with the scoring halves of two upstream plugins added to every feasible
// node's total,
//   NodeAffinity   (pkg/scheduler/framework/plugins/nodeaffinity/node_affinity.go, Score and NormalizeScore):
//                  A = the summed weights of the pod's matching preferred terms, na = 100 * A / max A;
//   TaintToleration (plugins/tainttoleration/taint_toleration.go, Score and NormalizeScore): T = the node's
//                  intolerable PreferNoSchedule taints, nt = 100 - 100 * T / max T (DefaultNormalizeScore, reversed),
// both maxima over the pod's feasible nodes, which change with every commit: they are taken per pod, here.
// The raw values are static per (pod class, node). The library keeps them on the device class-major, one record
// per (class, thread): A | T << 16 of the thread's NPL nodes (one aligned vector load) and one dword of admit bits,
// the class-bits column's verdict for those nodes (PrefRow). The kernel therefore holds no class words in
// registers, unlike seq_classes_body: the pod's record takes their place, and the record of pod j + 1 is requested
// while pod j is decided (its class is in the lane block already, the first pod of the next block included: the
// blocks are loaded one ahead), so no step waits on memory.
// Per pod, on top of seq_classes_body's scored step:
//  1. the feasibility bits of the lane's nodes (PrefScore::feasible: ScoreArgmax::eval's conjuncts);
//  2. for a pod whose class has a nonzero raw value somewhere (amask / tmask, wave-uniform): the wave's maxima of A
//     and T over the feasible held nodes (wave_reduce), met across waves by atomicMax in LDS slots of their own,
//     ms[3][2], one lds_barrier, a uniform read. The slots rotate as xs does (msh_seq_frame.h) but on the count of
//     pods that run this phase, msl: a pod that skips it neither adds to a slot nor advances msl, so every wave
//     sees the same slot for the same pod. The reset is xs's: after barrier s of this phase the slot read at s - 1
//     is free (every wave has arrived at barrier s since its read) and is next added to at s + 2, behind barrier
//     s + 1. A pod that skips the phase has A = T = 0 on every node: na = 0, nt = 100;
//  3. na and nt, exact integer quotients by a wave-uniform divisor (quot_u16), the resource score
//     (PrefScore::weighted_rs: ScoreArgmax's state, quot100 and weight-sum magic) and the key
//     ((W_res * rs + w_aff * na + w_taint * nt + 1) << 16) | (kbase - k); the sum is at most 65,534 (host check).
// The meet, decode's status and NodeNumber totals, the output, the commit and a grouped pod's second barrier are
// seq_classes_body's. decode adds the key's sum to NodeNumber's class total as it is: the weights are in the key.
// Resource score mode NONE runs the same instances with every resource weight 0 (rs = 0, W_res = 0).
// Table limits: seq_score_kernel's (NPL = 4 up to two resources, 2 above: 4,096 / 2,048 nodes); registers in
// profiles/prefs_regs.json.
#include "msh_seq_score_policy.h"

namespace msh {

template <int NR, int NPL, bool MOST>
struct PrefScore : ScoreArgmax<NR, NPL, MOST> {
  using Base = ScoreArgmax<NR, NPL, MOST>;
  static constexpr int K = Base::K;
  const uint32_t wres;  // the resource score's plugin weight, 0 in mode NONE
  __device__ __forceinline__ PrefScore(const SpreadScoreArgs& ss)
      : Base(ss.s.f.s.pp, 1, ss.rw, ss.wsum_magic), wres((uint32_t)ss.weight) {}

  // ScoreArgmax::eval's feasibility alone: bit k says node k takes the pod (the compares of FirstFeasible::eval)
  __device__ __forceinline__ uint32_t feasible(const FrameNodes<NR, NPL>& n, const FramePod<NR>& pod) const {
    uint32_t okm = 0u;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      bool ok = ((pod.av >> k) & 1u) != 0 && n.rem[k] > 0;
#pragma unroll
      for (int r = 0; r < NR; ++r) ok = ok && (pod.zr[r] || pod.rq[r] <= n.fr[r][k]);
      okm |= (ok ? 1u : 0u) << k;
    }
    return okm;
  }

  // ScoreArgmax::eval's resource score of node k, times the plugin weight: W_res * rs
  __device__ __forceinline__ uint32_t weighted_rs(const FrameNodes<NR, NPL>& n, const FramePod<NR>& pod, int k) const {
    uint32_t acc = 0u;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (this->rw[r] != 0u) {  // launch-uniform
        const int64_t d = n.fr[r][k] - pod.rq[r];  // c - q
        const int64_t c = this->al[r][k];
        const bool none = c == 0 || d < 0;  // upstream: capacity 0 or requested > capacity scores 0
        const int64_t num = none ? 0 : (MOST ? c - d : d);
        const uint32_t s = quot100(num, c, this->rc[r][k]);
        acc += (none ? 0u : s) * this->rw[r];
      }
    return wsum_div(acc, this->magic) * wres;
  }

  // ScoreArgmax::decode with the key's sum taken as it is
  __device__ __forceinline__ void decode(const uint32_t (&v)[K], uint32_t pc, int32_t* sel, int64_t* sc,
                                         int32_t* st) const {
    const uint32_t km = v[0], kx = v[1];
    const bool has_m = km != 0u, has_x = kx != 0u;
    int64_t tm, tx;
    decode_classes(has_m, has_x, pc != CODE_NONE_POD, this->pp, &tm, &tx, st);
    tm += (int64_t)((km >> 16) - 1u);
    tx += (int64_t)((kx >> 16) - 1u);
    const int32_t im = (int32_t)(0xFFFFu - (km & 0xFFFFu)), ix = (int32_t)(0xFFFFu - (kx & 0xFFFFu));
    const bool pick_m = has_m && (!has_x || tm > tx || (tm == tx && im < ix));
    *sel = *st == 0 ? (pick_m ? im : ix) : -1;
    *sc = *st == 0 ? (pick_m ? tm : tx) : 0;
  }
};

// What a thread loads per pod, its record of the class: the A | T << 16 of its NPL nodes, then their admit bits
// (bit k: node k admits the class), padded to 2 * NPL dwords so that the values are one aligned vector load.
// PrefArgs::rows holds PREF_THREADS records per class, thread t's at t: the table does not depend on the node count,
// and a thread that holds no node reads a record of zeros.
template <int NPL>
struct alignas(4 * NPL) PrefRow {
  uint32_t v[NPL];
  uint32_t adm;
  uint32_t pad[NPL - 1];
};

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_prefs_kernel(PrefArgs pa) {
  static_assert(NPL == 2 || NPL == 4, "a row is one 8- or 16-byte load per thread");
  using P = PrefScore<NR, NPL, MOST>;
  constexpr int K = P::K;
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ uint32_t xs[3][P::SLOT];
  __shared__ uint32_t ms[3][2];  // [max A, max T] of the pods that run the maxima phase
  extern __shared__ int32_t lcnt[];  // [G][SPREAD_ZONES] counts, then [G] max_skew
  P p(pa.ss);
  const SpreadArgs& sa = pa.ss.s;
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
  const int32_t C = pa.rows ? pa.n_classes : 0;  // without a table every pod is of class -1
  int32_t* lskew = lcnt + G * SPREAD_ZONES;
  const bool in_zset = ((sa.zset >> lane) & 1ull) != 0;  // lane z: zone z occurs on a node
  const uint32_t w_aff = pa.w_aff, w_taint = pa.w_taint;

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
      const int32_t z = sa.zone ? sa.zone[i] : -1;
      const bool has = z >= 0 && z < SPREAD_ZONES;
      zones |= (uint64_t)(has ? (uint32_t)z : 0u) << (8 * k);
      hz |= (has ? 1u : 0u) << k;
    }
  }
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) lcnt[e] = sa.cnt[e];
  for (int32_t e = t; e < G; e += NW * WAVE) lskew[e] = sa.max_skew[e];
  if (NW > 1 && threadIdx.x < 3 * P::SLOT) (&xs[0][0])[threadIdx.x] = P::IDENT;
  if (NW > 1 && threadIdx.x < 3 * 2) (&ms[0][0])[threadIdx.x] = 0u;
  __syncthreads();
  int sl = 0, msl = 0;

  // the row of class c (wave-uniform) for the thread's nodes and their admit bits; class -1: zeros, all admitted
  uint32_t row_n[NPL];
  uint32_t adm_n = KMASK;
  auto fetch = [&](int32_t c) {
    if (c >= 0) {
      const PrefRow<NPL>* rc = reinterpret_cast<const PrefRow<NPL>*>(pa.rows) + c * PREF_THREADS;  // uniform
      const PrefRow<NPL>& rec = rc[(uint32_t)t];
#pragma unroll
      for (int k = 0; k < NPL; ++k) row_n[k] = rec.v[k];
      adm_n = rec.adm;
    } else {
#pragma unroll
      for (int k = 0; k < NPL; ++k) row_n[k] = 0u;
      adm_n = KMASK;
    }
  };

  const int32_t n_pods = a.n_pods;
  // Pods in lanes, 64 at a time (every wave loads the block), one block ahead; clamped index: no branch
  int32_t dn = 0, tn = 0, gn = -1, cn = -1;
  int64_t rn[NR];
  auto load_raw = [&](int32_t j0) {
    const int32_t jj = min(j0 + lane, n_pods - 1);
    dn = a.pod_digit[jj];
    tn = a.pod_tol[jj];
    gn = sa.pod_group ? sa.pod_group[jj] : -1;
    cn = pa.pod_class ? pa.pod_class[jj] : -1;
#pragma unroll
    for (int r = 0; r < NR; ++r) rn[r] = r < nres ? fa.pod_req[(int64_t)r * n_pods + jj] : 0;
  };
  load_raw(0);
  fetch(__builtin_amdgcn_readfirstlane((uint32_t)cn < (uint32_t)C ? cn : -1));  // pod 0's row
  for (int32_t jb = 0; jb < n_pods; jb += WAVE) {
    // this block's lane values: the code | ~tolerates << 4, the group (anything outside [0, G): -1, ungrouped),
    // the class (anything outside [0, C): -1, no class) and the requests' halves
    const bool dig = dn >= 0 && dn <= 9;
    const uint32_t pkv = (dig ? (uint32_t)dn : CODE_NONE_POD) | (tn != 0 ? 0u : 16u);
    const int32_t gv = (uint32_t)gn < (uint32_t)G ? gn : -1;
    const int32_t cv = (uint32_t)cn < (uint32_t)C ? cn : -1;
    int32_t rlo[NR], rhi[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      rlo[r] = (int32_t)(uint32_t)((uint64_t)rn[r] & 0xFFFFFFFFull);
      rhi[r] = (int32_t)(uint32_t)((uint64_t)rn[r] >> 32);
    }
    load_raw(jb + WAVE);
    // the class of the next block's first pod (past the end: the last pod's, fetched and not used)
    const int32_t cv1 = __builtin_amdgcn_readfirstlane((uint32_t)cn < (uint32_t)C ? cn : -1);
    const int32_t je = min(jb + WAVE, n_pods);
    for (int32_t j = jb; j < je; ++j) {
      const int jl = j - jb;
      const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)pkv, jl);
      const int32_t pg = __builtin_amdgcn_readlane(gv, jl);   // in [-1, G)
      const int32_t pcl = __builtin_amdgcn_readlane(cv, jl);  // in [-1, C), C <= 64
      // this pod's row arrived during the last step; the next pod's is requested now
      uint32_t row[NPL];
#pragma unroll
      for (int k = 0; k < NPL; ++k) row[k] = row_n[k];
      const uint32_t adm = adm_n;
      fetch(jl + 1 < WAVE ? __builtin_amdgcn_readlane(cv, (jl + 1) & (WAVE - 1)) : cv1);
      FramePod<NR> pod;
      pod.pc = pk & 15u;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(rlo[r], jl);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(rhi[r], jl);
        pod.rq[r] = (int64_t)(((uint64_t)hi << 32) | lo);
        pod.zr[r] = pod.rq[r] == 0;
      }
      pod.av = ((pk & 16u) ? n.av0 : n.av1) & adm;
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
      const uint32_t okm = p.feasible(n, pod);
      uint32_t sum[NPL];  // the preference terms, then the whole weighted sum
      const bool any_a = pcl >= 0 && ((pa.amask >> (uint32_t)pcl) & 1ull) != 0;  // wave-uniform, as pcl is
      const bool any_t = pcl >= 0 && ((pa.tmask >> (uint32_t)pcl) & 1ull) != 0;
      if (any_a || any_t) {
        uint32_t ma = 0u, mt = 0u;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const bool ok = ((okm >> k) & 1u) != 0;
          ma = umax(ma, ok ? row[k] & 0xFFFFu : 0u);
          mt = umax(mt, ok ? row[k] >> 16 : 0u);
        }
        ma = any_a ? wave_reduce(ma, umax) : 0u;
        mt = any_t ? wave_reduce(mt, umax) : 0u;
        if constexpr (NW > 1) {
          if (lane == 0) {
            if (ma != 0u) atomicMax(&ms[msl][0], ma);
            if (mt != 0u) atomicMax(&ms[msl][1], mt);
          }
          lds_barrier();
          ma = (uint32_t)__builtin_amdgcn_readfirstlane((int)ms[msl][0]);
          mt = (uint32_t)__builtin_amdgcn_readfirstlane((int)ms[msl][1]);
          // the slot read one phase ago is free now and is next added to two phases ahead (see the head comment)
          if (threadIdx.x < 2) ms[msl == 0 ? 2 : msl - 1][threadIdx.x] = 0u;
          msl = msl == 2 ? 0 : msl + 1;
        }
        // a maximum of 0 divides as 1: every feasible node then holds 0, na = 0 and nt = 100
        const uint32_t da = umax(ma, 1u), dt = umax(mt, 1u);
        const float ra = __builtin_amdgcn_rcpf((float)da), rt = __builtin_amdgcn_rcpf((float)dt);
#pragma unroll
        for (int k = 0; k < NPL; ++k)
          sum[k] = w_aff * quot_u16(row[k] & 0xFFFFu, da, ra) + w_taint * (100u - quot_u16(row[k] >> 16, dt, rt));
      } else {
#pragma unroll
        for (int k = 0; k < NPL; ++k) sum[k] = w_taint * 100u;
      }
      // the resource score after the maxima's barrier, not before: nothing of it is then live across the wait
#pragma unroll
      for (int k = 0; k < NPL; ++k) sum[k] += p.weighted_rs(n, pod, k);
      const uint32_t kbase = 0xFFFFu - (uint32_t)n.i0;  // node i0 + k packs as kbase - k
      uint32_t km = 0u, kx = 0u;
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const uint32_t key = ((okm >> k) & 1u) ? (((sum[k] + 1u) << 16) | (kbase - (uint32_t)k)) : 0u;
        const bool mt = ((n.codes >> (4 * k)) & 15u) == pod.pc;
        km = umax(km, mt ? key : 0u);
        kx = umax(kx, mt ? 0u : key);
      }
      uint32_t v[K];
      v[0] = wave_reduce(km, umax);
      v[1] = wave_reduce(kx, umax);
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
struct PrefFamily {
  static constexpr int NPL2 = 4, NPL4 = 2;  // seq_score_kernel's
  template <int NR, int NPL, int NW>
  static auto kernel(const PrefArgs& a) {
    return a.ss.most ? seq_prefs_kernel<NR, NPL, NW, true> : seq_prefs_kernel<NR, NPL, NW, false>;
  }
};
}  // namespace

static_assert(PREF_THREADS == SEQ_FRAME_MAX_WAVES * WAVE, "one record per thread of the largest instance");

int32_t seq_prefs_max_nodes(int32_t nres) { return seq_frame_max_nodes<PrefFamily>(nres); }
int32_t seq_prefs_npl(int32_t nres) { return nres <= 2 ? PrefFamily::NPL2 : PrefFamily::NPL4; }

hipError_t launch_seq_prefs(const PrefArgs& a, hipStream_t s, std::string* err) {
  const SpreadArgs& sa = a.ss.s;
  if (sa.f.s.n_pods == 0) return hipSuccess;
  if (sa.n_groups < 0 || sa.n_groups > SPREAD_MAX_GROUPS || a.n_classes < 0 || a.n_classes > CLASS_MAX) return hipErrorInvalidValue;
  if (100ull * ((uint64_t)a.ss.weight + a.w_aff + a.w_taint) > 65534ull) return hipErrorInvalidValue;  // the key's sum
  const size_t lds = (size_t)sa.n_groups * (SPREAD_ZONES + 1) * sizeof(int32_t);  // at most 33,280 bytes
  return launch_seq_frame<PrefFamily>(a, sa.f, "preference", lds, s, err);
}

}  // namespace msh
