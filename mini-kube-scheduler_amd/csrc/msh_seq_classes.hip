// msh_seq_classes.hip — the class forms of the sequential-commit kernel (msh_schedule_sequential_classes): the
// topology-spread form and the scored topology-spread form with one more static conjunct, the per-class node
// mask. The host groups the pods of a call into at most 64 classes of identical node constraints (nodeSelector,
// required node affinity, taint tolerations, nodeName); the ctx holds one uint64 per node whose bit c says that
// the node admits pods of class c (msh_upload_node_class_bits); a pod of class c >= 0 is feasible on node i only
// if bit c of bits[i] is set. It is the av0 / av1 idea of the frame (two classes: tolerates the unschedulable
// taint or not) with 64 classes.
// One body serves both forms. It is the frame's (msh_seq_frame.h) with seq_spread_score_kernel's additions, written
// out as that kernel's is, and the policy decides what is met per pod: FirstFeasible (the frame header's, the
// unscored form: first feasible match / node / non-match) or ScoreArgmax (msh_seq_score_policy.h, the scored
// form). Both conjuncts enter the policy's eval through the pod's availability bits, so eval, the reduction,
// decode and the commit are the policies' and the frame's, untouched:
//  * zone: av &= hz & (the allowed bits of the lane's NPL nodes), as in seq_spread_score_kernel. The unscored
//    form therefore runs FirstFeasible with the conjunct folded into av and not seq_spread_kernel's body with
//    `allowed` inside the compare loop; the results are the same (tests/test_classes_gpu.py compares both with
//    _spread on the same inputs).
//  * class: each thread keeps the uint64 of each of its NPL nodes in registers (2 x NPL VGPRs, the register
//    layout). The pod's class pcl is wave-uniform (readlane at the top of the step; a value outside [0, C) became
//    -1 when the lanes loaded the block, so nothing is ever indexed or shifted with a pod's raw value), and per
//    classed pod the thread does NPL 64-bit right shifts by pcl, one AND and one shift-OR each:
//    av &= bits of (cb[k] >> pcl) & 1. The operands are the static registers and pcl: nothing of it depends on a
//    commit, so it is issued ahead of eval's compares against the free amounts, which do. A pod of class -1
//    skips it on a wave-uniform branch. No LDS and no barrier is added.
//  * a null zone column (hz = 0: no node has a zone) and a null pod_group (every pod ungrouped) are taken in the
//    prologue and in the block loader and cost nothing per pod; the host then passes n_groups = 0.
// The race on cnt[g][z] and the second barrier of a grouped, PLACED step are seq_spread_kernel's.
// Table limits and instances: the unscored form has seq_fit_kernel's (NPL = 8 up to two resources, 4 above:
// 8,192 / 4,096 nodes), the scored form seq_score_kernel's (NPL = 4 / 2: 4,096 / 2,048), on 1, 4 or 16 waves.
// The class registers fit at those limits without scratch (profiles/classes_regs.json).
#include "msh_seq_score_policy.h"

namespace msh {

template <int NR, int NPL, int NW, class P>
__device__ __forceinline__ void seq_classes_body(const ClassArgs& ca, P& p) {
  static_assert(32 % NPL == 0 && NPL <= 8, "a thread's nodes lie in one word, their zones in 64 bits");
  constexpr int K = P::K;
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ uint32_t xs[3][P::SLOT];
  extern __shared__ int32_t lcnt[];  // [G][SPREAD_ZONES] counts, then [G] max_skew
  const SpreadArgs& sa = ca.ss.s;
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
  const int32_t C = ca.class_bits ? ca.n_classes : 0;  // without a column every pod is of class -1
  int32_t* lskew = lcnt + G * SPREAD_ZONES;
  const bool in_zset = ((sa.zset >> lane) & 1ull) != 0;  // lane z: zone z occurs on a node

  FrameNodes<NR, NPL> n;
  n.i0 = i0;
  uint64_t zones = 0ull;  // node k's zone id in bits 8k .. 8k + 5
  uint32_t hz = 0u;       // bit k: node k has a zone
  uint64_t cb[NPL];       // node k's class bits
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    n.rem[k] = 0;
    cb[k] = 0ull;
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
      if (C > 0) cb[k] = ca.class_bits[i];
    }
  }
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) lcnt[e] = sa.cnt[e];
  for (int32_t e = t; e < G; e += NW * WAVE) lskew[e] = sa.max_skew[e];
  if (NW > 1 && threadIdx.x < 3 * P::SLOT) (&xs[0][0])[threadIdx.x] = P::IDENT;
  __syncthreads();
  int sl = 0;

  const int32_t n_pods = a.n_pods;
  // Pods in lanes, 64 at a time (every wave loads the block), one block ahead; clamped index: no branch
  int32_t dn = 0, tn = 0, gn = -1, cn = -1;
  int64_t rn[NR];
  auto load_raw = [&](int32_t j0) {
    const int32_t jj = min(j0 + lane, n_pods - 1);
    dn = a.pod_digit[jj];
    tn = a.pod_tol[jj];
    gn = sa.pod_group ? sa.pod_group[jj] : -1;
    cn = ca.pod_class ? ca.pod_class[jj] : -1;
#pragma unroll
    for (int r = 0; r < NR; ++r) rn[r] = r < nres ? fa.pod_req[(int64_t)r * n_pods + jj] : 0;
  };
  load_raw(0);
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
    const int32_t je = min(jb + WAVE, n_pods);
    for (int32_t j = jb; j < je; ++j) {
      const int jl = j - jb;
      const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)pkv, jl);
      const int32_t pg = __builtin_amdgcn_readlane(gv, jl);   // in [-1, G)
      const int32_t pcl = __builtin_amdgcn_readlane(cv, jl);  // in [-1, C), C <= 64
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
      if (pcl >= 0) {  // wave-uniform: the class bits of the lane's nodes, from static registers and pcl alone
        uint32_t cm = 0u;
#pragma unroll
        for (int k = 0; k < NPL; ++k) cm |= (uint32_t)((cb[k] >> (uint32_t)pcl) & 1ull) << k;
        pod.av &= cm;
      }
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

template <int NR, int NPL, int NW, bool KX>
__global__ __launch_bounds__(NW * WAVE) void seq_classes_kernel(ClassArgs ca) {
  FirstFeasible<KX> p(ca.ss.s.f.s.pp);
  seq_classes_body<NR, NPL, NW>(ca, p);
}

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_classes_score_kernel(ClassArgs ca) {
  ScoreArgmax<NR, NPL, MOST> p(ca.ss.s.f.s.pp, ca.ss.weight, ca.ss.rw, ca.ss.wsum_magic);
  seq_classes_body<NR, NPL, NW>(ca, p);
}

namespace {
struct ClassFamily {
  static constexpr int NPL2 = 8, NPL4 = 4;  // seq_fit_kernel's
  template <int NR, int NPL, int NW>
  static auto kernel(const ClassArgs& a) {
    return needs_kx(a.ss.s.f.s.pp) ? seq_classes_kernel<NR, NPL, NW, true> : seq_classes_kernel<NR, NPL, NW, false>;
  }
};
struct ClassScoreFamily {
  static constexpr int NPL2 = 4, NPL4 = 2;  // seq_score_kernel's
  template <int NR, int NPL, int NW>
  static auto kernel(const ClassArgs& a) {
    return a.ss.most ? seq_classes_score_kernel<NR, NPL, NW, true> : seq_classes_score_kernel<NR, NPL, NW, false>;
  }
};
}  // namespace

int32_t seq_classes_max_nodes(int32_t nres, bool scored) {
  return scored ? seq_frame_max_nodes<ClassScoreFamily>(nres) : seq_frame_max_nodes<ClassFamily>(nres);
}

hipError_t launch_seq_classes(const ClassArgs& a, bool scored, hipStream_t s, std::string* err) {
  const SpreadArgs& sa = a.ss.s;
  if (sa.f.s.n_pods == 0) return hipSuccess;
  if (sa.n_groups < 0 || sa.n_groups > SPREAD_MAX_GROUPS || a.n_classes < 0 || a.n_classes > CLASS_MAX) return hipErrorInvalidValue;
  if (scored && sa.f.nres < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)sa.n_groups * (SPREAD_ZONES + 1) * sizeof(int32_t);  // at most 33,280 bytes
  if (scored) return launch_seq_frame<ClassScoreFamily>(a, sa.f, "scored class-mask", lds, s, err);
  return launch_seq_frame<ClassFamily>(a, sa.f, "class-mask", lds, s, err);
}

}  // namespace msh
