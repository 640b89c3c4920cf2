// msh_seq_podaffinity.hip — the inter-pod affinity form of the sequential-commit kernel
// (msh_schedule_sequential_podaffinity with a profile column): the balanced-allocation form (msh_seq_balanced.hip)
// with the required half of upstream's InterPodAffinity filter (v1.22, pkg/scheduler/framework/plugins/
// interpodaffinity/filtering.go) as one more conjunct of the availability bits. The balanced kernel is not edited
// for it: its quotients, score policy, per-pod record and step are repeated here and the step below is its step
// plus what follows. See msh_seq_soft.hip for the phases, the slots and the barriers; the one change to them is
// the condition of the post-commit barrier.
// State: two words per node, present[i] (the OR of the match bits of the pods committed to node i) and repel[i]
// (the OR of their anti-affinity terms). The register file is full (the balanced kernel's 16-wave instances sit at
// 126..128 VGPRs), so none of it lives in registers: the node words are in LDS, 8 bytes per held node, thread t's
// NPL pairs consecutive (one or two wide reads), and only the step of a pod with a nonzero profile reads them, a
// workgroup-uniform branch. The prologue fills them from PodAffinityArgs::state and derives
//   presentZ[z], repelZ[z]: the OR of the words over the nodes of zone z
//   any: the OR of present & HM over every node, ORed with present & ZM over the zoned nodes
// by LDS atomics (HM / ZM: the masks of the hostname / zone terms). Nothing zone-level is stored between calls.
// Per pod of profile q >= 0 (M = match, AA = anti, AF = the affinity term's bit or 0; broadcast LDS reads, uniform)
// and held node k, with P = (present & HM) | (zoned ? presentZ[zone] & ZM : 0) and R likewise from repel:
//   ok = (P & AA) == 0 && (R & M) == 0
//        && (AF == 0 || ((AF & HM || zoned) && (P & AF || ((any & AF) == 0 && (M & AF) != 0))))
// one node at a time into NPL bits that are ANDed into pod.av before anything else reads it: the status order, the
// normalizer's extents, the preference maxima, a soft group's Zs, the scores, the first maximum and the commit are
// all taken over the reduced feasible set. The hard spread minimum stays over Zset. The profile id rides in bits
// 8.. of the class lane value, so no new register lives across the inner loop.
// Commit: the owner thread ORs M and AA into the node's words, into the zone's words when the node has a zone, and
// the term bits with a topology key on that node into `any`; the next step's reads are behind the post-commit
// barrier, taken when the pod is grouped or has M | AA != 0 (never twice; one wave: the wavefront fence). The
// epilogue writes the node words back.
// LDS: PaShared (static; 8 * NW * 64 * NPL bytes of node words, the profiles, the zone words) plus the balanced
// kernel's dynamic counts. The largest instance with more than about 100 spread groups would pass 64 KiB; the host
// refuses that call (seq_podaffinity_lds, seq_check) and no launch opts in to more.
// Bounds and table limits: the balanced kernel's; w_balanced may be 0 here and the table may then hold fewer than two
// resources (the term is skipped, a launch-uniform branch). Registers in profiles/podaffinity_regs.json.
#include "msh_seq_score_policy.h"

namespace msh {
namespace {

// BalScore of msh_seq_balanced.hip
template <int NR, int NPL, bool MOST>
struct PaScore : ScoreArgmax<NR, NPL, MOST> {
  using Base = ScoreArgmax<NR, NPL, MOST>;
  static constexpr int K = Base::K;
  const uint32_t wres;  // the resource score's plugin weight, 0 in mode NONE
  __device__ __forceinline__ PaScore(const SpreadScoreArgs& ss)
      : Base(ss.s.f.s.pp, 1, ss.rw, ss.wsum_magic), wres((uint32_t)ss.weight) {}

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

  __device__ __forceinline__ uint32_t weighted_rs(const FrameNodes<NR, NPL>& n, const FramePod<NR>& pod, int k) const {
    uint32_t acc = 0u;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (this->rw[r] != 0u) {  // launch-uniform
        const int64_t d = n.fr[r][k] - pod.rq[r];  // c - q
        const int64_t c = this->al[r][k];
        const bool none = c == 0 || d < 0;  // upstream: capacity 0 or requested > capacity scores 0
        const int64_t num = none ? 0 : (MOST ? c - d : d);
        const uint32_t s = quot100(num, c, 100.0f * __builtin_amdgcn_rcpf((float)(double)c));
        acc += (none ? 0u : s) * this->rw[r];
      }
    return wsum_div(acc, this->magic) * wres;
  }

  __device__ __forceinline__ uint32_t balanced(const FrameNodes<NR, NPL>& n, const FramePod<NR>& pod, int k) const {
    static_assert(NR >= 2, "the balanced score reads two resources");
    const int64_t c0 = this->al[0][k], c1 = this->al[1][k];
    return balanced_bs(c0 - n.fr[0][k] + pod.rq[0], c0, c1 - n.fr[1][k] + pod.rq[1], c1);
  }

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

// BalRow of msh_seq_balanced.hip: the record of PrefArgs::rows
template <int NPL>
struct alignas(4 * NPL) PaRow {
  uint32_t v[NPL];
  uint32_t adm;
  uint32_t pad[NPL - 1];
};

// The kernel's static LDS, one object so that its size is the figure the host's budget check adds up.
template <int NPL, int NW, int SLOT>
struct alignas(16) PaShared {
  uint2 nw[NW * WAVE * NPL];          // node i's (present, repel) at i: thread t's NPL pairs are consecutive
  uint4 prof[PODAFF_MAX_PROFILES];    // profile q: (match, anti, the affinity term's bit or 0, unused)
  double lw[SPREAD_ZONES + 1];        // log(size + 2)
  uint32_t pz[2][SPREAD_ZONES];       // presentZ, repelZ
  uint32_t lzone[NW * WAVE];          // thread t's zone ids, node k's in bits 8k .. 8k + 5
  uint32_t xs[3][SLOT];
  uint32_t ms[3][4];                  // [max A, max T, Zs lo, Zs hi] of the pods that run the shared phase
  uint32_t any;
};

}  // namespace

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_podaffinity_kernel(PodAffinityArgs pq) {
  static_assert(NPL == 2 || NPL == 4, "a row is one 8- or 16-byte load per thread");
  using P = PaScore<NR, NPL, MOST>;
  constexpr int K = P::K;
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ PaShared<NPL, NW, P::SLOT> sh;
  extern __shared__ int32_t lcnt[];  // [G][SPREAD_ZONES] counts, then [G] max_skew, negated for a soft group
  const BalancedArgs& ba = pq.ba;
  const SoftArgs& so = ba.so;
  const PrefArgs& pa = so.p;
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
  const int32_t Q = pq.pod_profile ? pq.n_profiles : 0;
  const uint32_t HM = pq.host_mask, ZM = pq.zone_mask;
  int32_t* lskew = lcnt + G * SPREAD_ZONES;
  const bool in_zset = ((sa.zset >> lane) & 1ull) != 0;  // lane z: zone z occurs on a node
  const uint32_t w_aff = pa.w_aff, w_taint = pa.w_taint, w_spread = so.w_spread, w_bal = ba.w_balanced;
  const bool zs_lo = (uint32_t)sa.zset != 0u, zs_hi = (sa.zset >> 32) != 0ull;  // the halves the table's zones touch

  FrameNodes<NR, NPL> n;
  n.i0 = i0;
  uint32_t zones0 = 0u;  // node k's zone id in bits 8k .. 8k + 5
  uint32_t hz0 = 0u;    // bit k: node k has a zone
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    n.rem[k] = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) n.fr[r][k] = 0;
  }
  // the zone words and `any` start at zero, a barrier before the first atomic below
  for (int32_t e = t; e < 2 * SPREAD_ZONES; e += NW * WAVE) (&sh.pz[0][0])[e] = 0u;  // one wave is 64 threads
  if (threadIdx.x == 0) sh.any = 0u;
  __syncthreads();
  if (held) {
    const int32_t w = i0 >> 5, sft = i0 & 31;
    const uint32_t* g = a.planes + (size_t)(w / PLANE_GW) * GROUP_DWORDS + w % PLANE_GW;
    const uint32_t d0 = (g[0] >> sft) & KMASK, d1 = (g[PLANE_GW] >> sft) & KMASK;
    const uint32_t d2 = (g[2 * PLANE_GW] >> sft) & KMASK, d3 = (g[3 * PLANE_GW] >> sft) & KMASK;
    n.av1 = (g[PLANE_V * PLANE_GW] >> sft) & KMASK;
    n.av0 = n.av1 & ~(g[PLANE_X * PLANE_GW] >> sft);
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
      zones0 |= (has ? (uint32_t)z : 0u) << (8 * k);
      hz0 |= (has ? 1u : 0u) << k;
      // the node's words, and their part in the derived ones
      const uint2 wd = pq.state[i];
      sh.nw[i] = wd;
      if (has) {
        if (wd.x) atomicOr(&sh.pz[0][z], wd.x);
        if (wd.y) atomicOr(&sh.pz[1][z], wd.y);
      }
      const uint32_t av = (wd.x & HM) | (has ? wd.x & ZM : 0u);
      if (av) atomicOr(&sh.any, av);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NPL; ++k) sh.nw[i0 + k] = make_uint2(0u, 0u);  // i0 + k < NW * WAVE * NPL
  }
  // the four bit sets of the thread's nodes in one register through the loop (see msh_seq_balanced.hip)
  sh.lzone[t] = zones0;  // read back by the same thread only: no barrier needed for it
  uint32_t nb = (n.codes & 0xFFFFu) | (n.av0 << 16) | (n.av1 << 20) | (hz0 << 24);
  asm volatile("" : "+v"(nb));
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) lcnt[e] = sa.cnt[e];
  for (int32_t e = t; e < G; e += NW * WAVE) {  // G <= SPREAD_MAX_GROUPS = 128: two words of mode bits
    const int32_t sk = sa.max_skew[e];
    lskew[e] = (((e < 64 ? so.soft[0] : so.soft[1]) >> (e & 63)) & 1ull) != 0 ? -sk : sk;
  }
  if (G > 0 && so.zone_weight)  // the weights are there when the ctx holds a soft group; no other pod reads lw
    for (int32_t e = t; e <= SPREAD_ZONES; e += NW * WAVE) sh.lw[e] = so.zone_weight[e];
  for (int32_t e = t; e < PODAFF_MAX_PROFILES; e += NW * WAVE)
    sh.prof[e] = e < Q ? pq.profiles[e] : make_uint4(0u, 0u, 0u, 0u);
  if (NW > 1 && threadIdx.x < 3 * P::SLOT) (&sh.xs[0][0])[threadIdx.x] = P::IDENT;
  if (NW > 1 && threadIdx.x < 3 * 4) (&sh.ms[0][0])[threadIdx.x] = 0u;
  __syncthreads();
  int sl = 0, msl = 0;

  // the row of class c (wave-uniform) for the thread's nodes and their admit bits; class -1: zeros, all admitted
  uint32_t row_n[NPL];
  uint32_t adm_n = KMASK;
  auto fetch = [&](int32_t c) {
    if (c >= 0) {
      const PaRow<NPL>* rc = reinterpret_cast<const PaRow<NPL>*>(pa.rows) + c * PREF_THREADS;  // uniform
      const PaRow<NPL>& rec = rc[(uint32_t)t];
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
  // Pods in lanes, 64 at a time, the classes one block ahead (see msh_seq_balanced.hip)
  int32_t cn = -1;
  auto load_class = [&](int32_t j0) { cn = pa.pod_class ? pa.pod_class[min(j0 + lane, n_pods - 1)] : -1; };
  load_class(0);
  fetch(__builtin_amdgcn_readfirstlane((uint32_t)cn < (uint32_t)C ? cn : -1));  // pod 0's row
  for (int32_t jb = 0; jb < n_pods; jb += WAVE) {
    // this block's lane values: the code | ~tolerates << 4, the group (anything outside [0, G): -1, ungrouped),
    // the class and the profile (anything outside [0, C) / [0, Q): -1) and the requests' halves
    const int32_t jj = min(jb + lane, n_pods - 1);
    const int32_t dn = a.pod_digit[jj], tn = a.pod_tol[jj], gn = sa.pod_group ? sa.pod_group[jj] : -1;
    const int32_t qn = pq.pod_profile ? pq.pod_profile[jj] : -1;
    const bool dig = dn >= 0 && dn <= 9;
    const uint32_t pkv = (dig ? (uint32_t)dn : CODE_NONE_POD) | (tn != 0 ? 0u : 16u);
    const int32_t gv = (uint32_t)gn < (uint32_t)G ? gn : -1;
    // class + 1 in bits 0 .. 7, profile + 1 in bits 8 .. 15: one lane value for both
    const int32_t cv = (int32_t)(((uint32_t)cn < (uint32_t)C ? (uint32_t)cn + 1u : 0u) |
                                 (((uint32_t)qn < (uint32_t)Q ? (uint32_t)qn + 1u : 0u) << 8));
    int32_t rlo[NR], rhi[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t rq = r < nres ? fa.pod_req[(int64_t)r * n_pods + jj] : 0;
      rlo[r] = (int32_t)(uint32_t)((uint64_t)rq & 0xFFFFFFFFull);
      rhi[r] = (int32_t)(uint32_t)((uint64_t)rq >> 32);
    }
    load_class(jb + WAVE);
    // the class of the next block's first pod (past the end: the last pod's, fetched and not used)
    const int32_t cv1 = __builtin_amdgcn_readfirstlane((uint32_t)cn < (uint32_t)C ? cn : -1);
    const int32_t je = min(jb + WAVE, n_pods);
    for (int32_t j = jb; j < je; ++j) {
      const int jl = j - jb;
      const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)pkv, jl);
      const int32_t pg = __builtin_amdgcn_readlane(gv, jl);  // in [-1, G)
      const uint32_t cq = (uint32_t)__builtin_amdgcn_readlane(cv, jl);
      const int32_t pcl = (int32_t)(cq & 0xFFu) - 1;  // in [-1, C), C <= 64
      const int32_t ppr = (int32_t)(cq >> 8) - 1;     // in [-1, Q), Q <= 64
      // this pod's row arrived during the last step; the next pod's is requested now
      uint32_t row[NPL];
#pragma unroll
      for (int k = 0; k < NPL; ++k) row[k] = row_n[k];
      const uint32_t adm = adm_n;
      const uint32_t cq1 = (uint32_t)__builtin_amdgcn_readlane(cv, (jl + 1) & (WAVE - 1));
      fetch(jl + 1 < WAVE ? (int32_t)(cq1 & 0xFFu) - 1 : cv1);
      FramePod<NR> pod;
      pod.pc = pk & 15u;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(rlo[r], jl);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(rhi[r], jl);
        pod.rq[r] = (int64_t)(((uint64_t)hi << 32) | lo);
        pod.zr[r] = pod.rq[r] == 0;
      }
      pod.av = ((pk & 16u) ? nb >> 16 : nb >> 20) & adm;  // adm holds no bit above KMASK
      const uint32_t hz = (nb >> 24) & KMASK;
      // the profile's record: a uniform address, one broadcast read
      uint32_t M = 0u, AA = 0u, AF = 0u;
      if (ppr >= 0) {
        const uint4 rec = sh.prof[ppr];
        M = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.x);
        AA = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.y);
        AF = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.z);
      }
      const bool affine = (M | AA | AF) != 0u;
      const uint32_t zones = (pg >= 0 || affine) ? sh.lzone[t] : 0u;  // workgroup-uniform branch
      if (affine) {  // workgroup-uniform: the inter-pod conjunct, one node at a time
        const uint32_t anyw = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.any);
        const bool first = (anyw & AF) == 0u && (M & AF) != 0u;  // the first pod of a self-affine series
        const bool af_host = (AF & HM) != 0u;
        uint32_t okp = 0u;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const uint2 wd = sh.nw[i0 + k];
          const bool zoned = ((hz >> k) & 1u) != 0;
          const uint32_t z = (zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1);
          const uint32_t P = (wd.x & HM) | (zoned ? sh.pz[0][z] & ZM : 0u);
          const uint32_t R = (wd.y & HM) | (zoned ? sh.pz[1][z] & ZM : 0u);
          bool ok = (P & AA) == 0u && (R & M) == 0u;
          ok = ok && (AF == 0u || ((af_host || zoned) && ((P & AF) != 0u || first)));
          okp |= (ok ? 1u : 0u) << k;
          asm volatile("" : "+v"(okp));  // one node's bit is complete before the next node's words are read
        }
        pod.av &= okp;
      }
      // the group's max_skew, negated for a soft group (workgroup-uniform): a soft pod passes no filter
      const int32_t skew = pg >= 0 ? __builtin_amdgcn_readfirstlane(lskew[pg]) : 0;
      const bool soft = skew < 0;
      if (skew > 0) {  // a hard group: the filter
        const int32_t c = lcnt[pg * SPREAD_ZONES + lane];
        const int32_t minc = wave_reduce(in_zset ? c : INT32_MAX, [](int32_t x, int32_t y) { return min(x, y); });
        // cnt + 1 - minc <= max_skew without leaving int32: 0 <= minc <= c on a lane of Zset, 1 <= max_skew
        const unsigned long long allowed = __ballot(in_zset && c - minc <= skew - 1);
        uint32_t za = 0u;  // bit k: node k's zone is allowed
#pragma unroll
        for (int k = 0; k < NPL; ++k)
          za |= (uint32_t)((allowed >> ((zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1))) & 1ull) << k;
        pod.av &= hz & za;
      }
      const uint32_t okm = p.feasible(n, pod);
      uint32_t sum[NPL];  // the preference terms, then the whole weighted sum
      const bool any_a = pcl >= 0 && ((pa.amask >> (uint32_t)pcl) & 1ull) != 0;  // wave-uniform, as pcl is
      const bool any_t = pcl >= 0 && ((pa.tmask >> (uint32_t)pcl) & 1ull) != 0;
      uint32_t zlo = 0u, zhi = 0u;  // Zs, wave-uniform after the phase
      if (any_a || any_t || soft) {
        uint32_t ma = 0u, mt = 0u;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const bool ok = ((okm >> k) & 1u) != 0;
          ma = umax(ma, ok ? row[k] & 0xFFFFu : 0u);
          mt = umax(mt, ok ? row[k] >> 16 : 0u);
        }
        ma = any_a ? wave_reduce(ma, umax) : 0u;
        mt = any_t ? wave_reduce(mt, umax) : 0u;
        if (soft) {
          uint64_t zm = 0ull;  // the zones of the thread's feasible zoned nodes
#pragma unroll
          for (int k = 0; k < NPL; ++k)
            zm |= (uint64_t)((okm & hz) >> k & 1u) << ((zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1));
          const auto bor = [](uint32_t x, uint32_t y) { return x | y; };
          zlo = zs_lo ? wave_reduce((uint32_t)zm, bor) : 0u;
          zhi = zs_hi ? wave_reduce((uint32_t)(zm >> 32), bor) : 0u;
        }
        if constexpr (NW > 1) {
          if (lane == 0) {
            if (ma != 0u) atomicMax(&sh.ms[msl][0], ma);
            if (mt != 0u) atomicMax(&sh.ms[msl][1], mt);
            if (zlo != 0u) atomicOr(&sh.ms[msl][2], zlo);
            if (zhi != 0u) atomicOr(&sh.ms[msl][3], zhi);
          }
          lds_barrier();
          ma = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.ms[msl][0]);
          mt = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.ms[msl][1]);
          zlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.ms[msl][2]);
          zhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.ms[msl][3]);
          // the slot read one phase ago is free now and is next added to two phases ahead (see msh_seq_soft.hip)
          if (threadIdx.x < 4) sh.ms[msl == 0 ? 2 : msl - 1][threadIdx.x] = 0u;
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
      // the resource score and the balanced term after the maxima's barrier, not before: nothing of them is then
      // live across the wait. Without a balanced weight (launch-uniform) the table may hold fewer than two resources.
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        sum[k] += p.weighted_rs(n, pod, k);
        if (w_bal != 0u) sum[k] += w_bal * p.balanced(n, pod, k);
        asm volatile("" : "+v"(sum[k]));  // one node's sum is complete before the next node's is used
      }
      const uint64_t zs = ((uint64_t)zhi << 32) | zlo;
      if (soft && zs != 0ull) {  // workgroup-uniform; with Zs empty ns = 0 on every node
        const double w = sh.lw[__builtin_popcountll(zs)];  // a uniform address: one broadcast read
        const bool in_zs = ((zs >> lane) & 1ull) != 0;
        // the counts are read behind the phase's barrier, not before it: one register less across the wait
        const int32_t raw = soft_raw(lcnt[pg * SPREAD_ZONES + lane], w, -skew - 1);
        const int32_t mx = wave_reduce(in_zs ? raw : 0, [](int32_t x, int32_t y) { return max(x, y); });
        const int32_t mn = wave_reduce(in_zs ? raw : INT32_MAX, [](int32_t x, int32_t y) { return min(x, y); });
        const uint32_t dm = (uint32_t)max(mx, 1);
        const uint32_t q = quot_soft((uint32_t)(mx + mn - (in_zs ? raw : mn)), dm, __builtin_amdgcn_rcpf((float)dm));
        const int32_t ns = in_zs ? (int32_t)(mx == 0 ? 100u : q) : 0;  // lane z: zone z's normalised score
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const int32_t zk = (int32_t)((zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1));
          const uint32_t nk = (uint32_t)__builtin_amdgcn_ds_bpermute(zk << 2, ns);  // every lane is active here
          sum[k] += ((hz >> k) & 1u) ? w_spread * nk : 0u;
        }
      }
      const uint32_t kbase = 0xFFFFu - (uint32_t)n.i0;  // node i0 + k packs as kbase - k
      uint32_t km = 0u, kx = 0u;
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const uint32_t key = ((okm >> k) & 1u) ? (((sum[k] + 1u) << 16) | (kbase - (uint32_t)k)) : 0u;
        const bool mt = ((nb >> (4 * k)) & 15u) == pod.pc;
        km = umax(km, mt ? key : 0u);
        kx = umax(kx, mt ? 0u : key);
      }
      uint32_t v[K];
      v[0] = wave_reduce(km, umax);
      v[1] = wave_reduce(kx, umax);
      if constexpr (NW > 1) {
        if (lane == 0) {
#pragma unroll
          for (int c = 0; c < K; ++c) P::meet(&sh.xs[sl][c], v[c]);
        }
        lds_barrier();
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.xs[sl][c]);
        // the slot read one step ago is free now and is next added to two steps ahead: wave 0 resets it in between
        if (threadIdx.x < P::SLOT) sh.xs[sl == 0 ? 2 : sl - 1][threadIdx.x] = P::IDENT;
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
        const bool marks = (M | AA) != 0u;  // the pod leaves bits behind
        if (t == own) {
#pragma unroll
          for (int k = 0; k < NPL; ++k)
            if (k == ks) {
              asm volatile("");  // a scalar branch per k, not selects over all NPL nodes (see seq_frame)
              n.rem[k] -= 1;
#pragma unroll
              for (int r = 0; r < NR; ++r) n.fr[r][k] -= pod.rq[r];
            }
          const bool zoned = ((hz >> ks) & 1u) != 0;
          const uint32_t z = (zones >> (8 * ks)) & (uint32_t)(SPREAD_ZONES - 1);
          // a grouped pod placed on a node with a zone: one more pod of the group in that zone
          if (pg >= 0 && zoned) lcnt[pg * SPREAD_ZONES + z] += 1;
          if (marks) {  // the node's words, its zone's, and the terms that now have a pod under their key
            uint2 wd = sh.nw[sel];
            wd.x |= M;
            wd.y |= AA;
            sh.nw[sel] = wd;
            if (zoned) {
              sh.pz[0][z] |= M;
              sh.pz[1][z] |= AA;
            }
            sh.any |= (M & HM) | (zoned ? M & ZM : 0u);
          }
        }
        if (pg >= 0 || marks) {  // workgroup-uniform: the writes above and the next step's reads, a barrier apart
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
  if (held) {
#pragma unroll
    for (int k = 0; k < NPL; ++k) pq.state[i0 + k] = sh.nw[i0 + k];
  }
  for (int32_t e = t; e < G * SPREAD_ZONES; e += NW * WAVE) sa.cnt[e] = lcnt[e];
}

namespace {
struct PodAffinityFamily {
  static constexpr int NPL2 = 4, NPL4 = 2;  // seq_balanced_kernel's
  template <int NR, int NPL, int NW>
  static auto kernel(const PodAffinityArgs& a) {
    return a.ba.so.p.ss.most ? seq_podaffinity_kernel<NR, NPL, NW, true> : seq_podaffinity_kernel<NR, NPL, NW, false>;
  }
};

// the static LDS of the instance the ladder picks (launch_seq_frame_nr's thresholds)
template <int NPL>
size_t pa_static_lds(int32_t n_nodes) {
  constexpr int SLOT = ScoreArgmax<2, NPL, false>::SLOT;  // the same for every NR and mode
  if (n_nodes <= 1 * WAVE * NPL) return sizeof(PaShared<NPL, 1, SLOT>);
  if (n_nodes <= 4 * WAVE * NPL) return sizeof(PaShared<NPL, 4, SLOT>);
  return sizeof(PaShared<NPL, SEQ_FRAME_MAX_WAVES, SLOT>);
}
}  // namespace

static_assert(PREF_THREADS == SEQ_FRAME_MAX_WAVES * WAVE, "one record per thread of the largest instance");
static_assert(SPREAD_MAX_GROUPS == 128, "SoftArgs::soft is two words");
static_assert(PODAFF_MAX_PROFILES <= 255 && CLASS_MAX <= 255,
              "class + 1 and profile + 1 share a lane value, a byte each");

int32_t seq_podaffinity_max_nodes(int32_t nres) { return seq_frame_max_nodes<PodAffinityFamily>(nres); }
int32_t seq_podaffinity_npl(int32_t nres) { return nres <= 2 ? PodAffinityFamily::NPL2 : PodAffinityFamily::NPL4; }

size_t seq_podaffinity_lds(int32_t nres, int32_t n_nodes, int32_t n_groups, size_t* per_group) {
  const size_t fixed = nres <= 2 ? pa_static_lds<PodAffinityFamily::NPL2>(n_nodes)
                                 : pa_static_lds<PodAffinityFamily::NPL4>(n_nodes);
  const size_t each = (size_t)(SPREAD_ZONES + 1) * sizeof(int32_t);
  if (per_group) *per_group = each;
  return fixed + (size_t)n_groups * each;
}

hipError_t launch_seq_podaffinity(const PodAffinityArgs& a, hipStream_t s, std::string* err) {
  const SoftArgs& so = a.ba.so;
  const SpreadArgs& sa = so.p.ss.s;
  if (sa.f.s.n_pods == 0) return hipSuccess;
  if (sa.n_groups < 0 || sa.n_groups > SPREAD_MAX_GROUPS || so.p.n_classes < 0 || so.p.n_classes > CLASS_MAX)
    return hipErrorInvalidValue;
  if (a.n_profiles < 0 || a.n_profiles > PODAFF_MAX_PROFILES || !a.state) return hipErrorInvalidValue;
  if (a.pod_profile && a.n_profiles > 0 && !a.profiles) return hipErrorInvalidValue;
  if (sa.f.nres < (a.ba.w_balanced ? 2 : 0) || sa.f.nres > FIT_MAX_RES) return hipErrorInvalidValue;  // q_0 and q_1
  if (100ull * ((uint64_t)so.p.ss.weight + so.p.w_aff + so.p.w_taint + so.w_spread + a.ba.w_balanced) > 65534ull)
    return hipErrorInvalidValue;  // the key's sum
  if ((so.soft[0] | so.soft[1]) != 0ull && !so.zone_weight) return hipErrorInvalidValue;
  if (seq_podaffinity_lds(sa.f.nres, sa.f.s.n_nodes, sa.n_groups, nullptr) > PODAFF_LDS_MAX)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)sa.n_groups * (SPREAD_ZONES + 1) * sizeof(int32_t);
  return launch_seq_frame<PodAffinityFamily>(a, sa.f, "inter-pod affinity", lds, s, err);
}

}  // namespace msh
