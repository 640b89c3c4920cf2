// msh_seq_frame.h — the register-resident frame of the per-node sequential-commit kernels seq_fit_kernel
// (msh_seq_fit.hip) and seq_score_kernel (msh_seq_score.hip). One workgroup walks the batch in order, one pod per
// step, no speculation; what a kernel adds to the frame is a policy type (FramePolicy's hooks), and each
// translation unit keeps only its policy and its thin __global__ wrappers. seq_spread_kernel (msh_seq_spread.hip)
// still carries its own copy of the frame (moved onto this one it ran 2-3% slower, see there) and shares
// wave_reduce, the launcher ladder and the table-limit message. seq_body (msh_seq_kernel.h) works on bit-sliced
// planes, a different frame.
//  * Node state. Thread t holds NPL consecutive nodes, t * NPL .. t * NPL + NPL - 1 (lanes and waves in List
//    order, all NPL in one 32-node word), and for each the free amount alloc - used per resource (int64, NR x NPL
//    register pairs), the remaining pod count eff - count (int32, eff = min(cap, max_pods)), the NodeNumber code
//    (4 bits, NPL codes in one register) and the two availability bits (V & ~X for pods that do not tolerate the
//    unschedulable taint, V for those that do), all taken in the prologue from the planes, counts, capacity
//    column and resource table. A table of fewer resources than NR runs with the spare free amounts and requests
//    zero; a zero request never rejects, also on a node whose alloc a patch lowered below used (negative free).
//    Values stay within int64: alloc, used and the requests are in [0, 2^62].
//  * The fold contract. SeqArgs::fold says that count replicas 1.. may hold counts (a no-capacity launch added
//    to them). The one thread that holds node i then reads the node's count as the sum over the replicas and
//    zeroes replicas 1..: the epilogue writes the whole count to replica 0, so after the launch replica 0 alone
//    holds it, which is what launch_count_fold leaves. Nothing else in the launch reads the replicas.
//  * Pods. Every wave loads the 64-pod block into its lanes, one block ahead, with the index clamped to the last
//    pod (no branch); per pod the code, ~tolerates and the requests are read wave-uniform by readlane.
//  * Per pod the policy evaluates the lane's nodes and reduces over the wave to K wave-uniform values. With more
//    than one wave, lane 0 of each wave folds them into slot sl of xs[3][.] (the policy's atomic) and every wave
//    reads the slot after one LDS-only barrier. Why three slots and when one may be reset: at step s every wave
//    adds to slot s mod 3 before barrier s and reads it after. Slot (s - 1) mod 3 was last read after barrier
//    s - 1 by waves that have all arrived at barrier s since, so once past barrier s nobody reads it again; it is
//    next added to at step s + 2, by waves that have passed barrier s + 1. The first threads of wave 0 reset it
//    between the two, after barrier s and before they arrive at barrier s + 1. Two slots would not do: the reset
//    of slot s - 1 and step s + 1's adds to the same slot would fall between the same two barriers.
//  * The policy decodes the met values into (node, score, status); thread 0 stores them. A placement is committed
//    before the next pod is decided: the one thread that holds the selected node (own = sel / NPL, every thread
//    decodes the same sel) takes one pod and the requests off it. The owner's registers are the only copy of the
//    node's state, so no barrier is needed for it.
//  * The epilogue writes count = eff - remaining and used = alloc - free back.
// Launch: as few waves as hold the table, 1, 4 or SEQ_FRAME_MAX_WAVES = 16, and the two-resource instance with
// NPL2 nodes per thread up to two resources, the four-resource one with NPL4 above (launch_seq_frame).
#pragma once

#include "msh_seq_kernel.h"

namespace msh {

constexpr int SEQ_FRAME_MAX_WAVES = 16;

// The wave's reduction by `op` (commutative, associative; every lane active), wave-uniform: four DPP steps leave
// every row of 16 lanes with its result, the four rows meet on the scalar side.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
  static_assert(sizeof(T) == sizeof(int), "one DPP register");
  v = op(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = op(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = op(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = op(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
  const T a = (T)__builtin_amdgcn_readlane((int)v, 0), b = (T)__builtin_amdgcn_readlane((int)v, 16);
  const T c = (T)__builtin_amdgcn_readlane((int)v, 32), d = (T)__builtin_amdgcn_readlane((int)v, 48);
  return op(op(a, b), op(c, d));
}

// What the frame keeps per thread, and per pod, as the policies see it.
template <int NR, int NPL>
struct FrameNodes {
  int64_t fr[NR][NPL];             // free amount alloc - used
  int32_t rem[NPL];                // remaining pod count
  uint32_t codes = 0xFFFFFFFFu;    // node k's code in bits 4k .. 4k + 3 (15: never a match)
  uint32_t av0 = 0u, av1 = 0u;     // bit k: node k takes a pod that does not / does tolerate the taint
  int32_t i0;                      // the thread's first node
};
template <int NR>
struct FramePod {
  uint32_t pc;     // the pod's code (CODE_NONE_POD without a digit)
  uint32_t av;     // the availability bits of the pod's tolerates class
  int64_t rq[NR];  // the requests
  bool zr[NR];     // ... that are zero
};

// The hooks, with what a policy that adds nothing does. A policy also gives K (values met per pod), SLOT (>= K,
// uint32 per xs slot), IDENT and meet (the reduction's identity and LDS atomic), eval and decode.
struct FramePolicy {
  // prologue, per held node and resource of the table
  __device__ __forceinline__ void node_res(int r, int k, int64_t alloc) {}
  // the allocatable amount for used = alloc - free
  __device__ __forceinline__ int64_t alloc(const FitArgs& fa, int r, int k, int32_t i) const {
    return fa.alloc[r * fa.res_stride + i];
  }
};

template <int NR, int NPL, int NW, class P>
__device__ __forceinline__ void seq_frame(const FitArgs& fa, P& p) {
  static_assert(32 % NPL == 0 && NPL * 4 <= 32, "a thread's nodes lie in one word, their codes in one register");
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  constexpr int K = P::K;
  __shared__ uint32_t xs[3][P::SLOT];
  const SeqArgs& a = fa.s;
  const int lane = threadIdx.x & (WAVE - 1);
  const int32_t t = (int32_t)threadIdx.x;
  const int32_t slots = a.n_words * 32;
  const int32_t i0 = t * NPL;
  const bool held = i0 < slots;  // then all NPL nodes are slots of the table (NPL divides 32)
  const int32_t nres = fa.nres;
  const int32_t max_pods = a.max_pods;

  FrameNodes<NR, NPL> n;
  n.i0 = i0;
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
    }
  }
  if (NW > 1) {
    if (threadIdx.x < 3 * P::SLOT) (&xs[0][0])[threadIdx.x] = P::IDENT;
    __syncthreads();
  }
  int sl = 0;

  const int32_t n_pods = a.n_pods;
  // Pods in lanes, 64 at a time (every wave loads the block), one block ahead; clamped index: no branch
  int32_t dn = 0, tn = 0;
  int64_t rn[NR];
  auto load_raw = [&](int32_t j0) {
    const int32_t jj = min(j0 + lane, n_pods - 1);
    dn = a.pod_digit[jj];
    tn = a.pod_tol[jj];
#pragma unroll
    for (int r = 0; r < NR; ++r) rn[r] = r < nres ? fa.pod_req[(int64_t)r * n_pods + jj] : 0;
  };
  load_raw(0);
  for (int32_t jb = 0; jb < n_pods; jb += WAVE) {
    // this block's lane values: the code | ~tolerates << 4, and the requests' halves
    const bool dig = dn >= 0 && dn <= 9;
    const uint32_t pkv = (dig ? (uint32_t)dn : CODE_NONE_POD) | (tn != 0 ? 0u : 16u);
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
              // ks is wave-uniform: a scalar branch per k. The empty asm keeps the compiler from turning the block
              // into selects, which every lane of every wave would then execute for all NPL nodes
              asm volatile("");
              n.rem[k] -= 1;
#pragma unroll
              for (int r = 0; r < NR; ++r) n.fr[r][k] -= pod.rq[r];
            }
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
}

// The "first feasible node of a class" policy of seq_fit_kernel: per resource one v_cmp_le_i64 against the free amount ORed with the
// request's "is zero" mask, ANDed with the availability bit and remaining count > 0; the lane's first feasible
// match, node and (KX: REVERSE / MINMAX) non-match, the wave's by wave_first, the workgroup's by an LDS minimum;
// decode_pod / decode_ident give status, node and score.
template <bool KX>
struct FirstFeasible : FramePolicy {
  static constexpr uint32_t NONE = 0xFFFFFFFFu;
  static constexpr int K = KX ? 3 : 2, SLOT = 3;  // [first match, first feasible, first feasible non-match]
  static constexpr uint32_t IDENT = NONE;
  __device__ static __forceinline__ void meet(uint32_t* slot, uint32_t v) { atomicMin(slot, v); }

  PluginParams pp;
  IdentDecode idec;
  __device__ __forceinline__ explicit FirstFeasible(const PluginParams& pp_) : pp(pp_), idec(make_ident_decode(pp_)) {}

  template <int NR, int NPL>
  __device__ __forceinline__ void eval(const FrameNodes<NR, NPL>& n, const FramePod<NR>& pod, uint32_t (&v)[K]) const {
    const uint32_t base = (uint32_t)n.i0;
    uint32_t cm = NONE, ca = NONE, cx = NONE;
#pragma unroll
    for (int k = NPL - 1; k >= 0; --k) {  // descending: the lane's first node wins
      bool ok = ((pod.av >> k) & 1u) != 0 && n.rem[k] > 0;
#pragma unroll
      for (int r = 0; r < NR; ++r) ok = ok && (pod.zr[r] || pod.rq[r] <= n.fr[r][k]);
      const bool mt = ((n.codes >> (4 * k)) & 15u) == pod.pc;
      ca = ok ? base + (uint32_t)k : ca;
      cm = (ok && mt) ? base + (uint32_t)k : cm;
      if (KX) cx = (ok && !mt) ? base + (uint32_t)k : cx;
    }
    v[0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_first(cm));
    v[1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_first(ca));
    if constexpr (KX) v[2] = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_first(cx));
  }

  __device__ __forceinline__ void decode(const uint32_t (&v)[K], uint32_t pc, int32_t* sel, int64_t* sc,
                                         int32_t* st) const {
    const int64_t im = v[0] != NONE ? (int64_t)v[0] : -1;
    const int64_t ia = v[1] != NONE ? (int64_t)v[1] : -1;
    if constexpr (KX) decode_pod(im, v[2] != NONE ? (int64_t)v[2] : -1, ia, pc != CODE_NONE_POD, pp, sel, sc, st);
    else decode_ident(im, ia, pc != CODE_NONE_POD, idec, sel, sc, st);
  }
};

// The launcher ladder. A family gives the nodes per thread NPL2 (up to two resources) and NPL4 (three or four),
// and kernel<NR, NPL, NW>(args), the instance to launch.
template <class Fam>
constexpr int32_t seq_frame_max_nodes(int32_t nres) {
  return SEQ_FRAME_MAX_WAVES * WAVE * (nres <= 2 ? Fam::NPL2 : Fam::NPL4);
}

// as few waves as hold the table: 1, 4 or 16
template <class Fam, int NR, int NPL, class Args>
hipError_t launch_seq_frame_nr(const Args& a, int32_t n_nodes, size_t lds, hipStream_t s) {
  auto go = [&](auto kern, int nw) {
    MSH_TIMED_LAUNCH(kern, dim3(1), dim3(nw * WAVE), lds, s, a);
    return hipGetLastError();
  };
  if (n_nodes <= 1 * WAVE * NPL) return go(Fam::template kernel<NR, NPL, 1>(a), 1);
  if (n_nodes <= 4 * WAVE * NPL) return go(Fam::template kernel<NR, NPL, 4>(a), 4);
  return go(Fam::template kernel<NR, NPL, SEQ_FRAME_MAX_WAVES>(a), SEQ_FRAME_MAX_WAVES);
}

// `form` names the family in the table-limit message; lds: dynamic LDS bytes
template <class Fam, class Args>
hipError_t launch_seq_frame(const Args& a, const FitArgs& fa, const char* form, size_t lds, hipStream_t s,
                            std::string* err) {
  if (fa.s.n_nodes > seq_frame_max_nodes<Fam>(fa.nres)) {
    if (err) *err = seq_table_limit_message(form, seq_frame_max_nodes<Fam>(fa.nres), fa.nres);
    return hipErrorInvalidValue;
  }
  if (fa.nres <= 2) return launch_seq_frame_nr<Fam, 2, Fam::NPL2>(a, fa.s.n_nodes, lds, s);
  return launch_seq_frame_nr<Fam, 4, Fam::NPL4>(a, fa.s.n_nodes, lds, s);
}

}  // namespace msh
