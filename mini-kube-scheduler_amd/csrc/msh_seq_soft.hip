// msh_seq_soft.hip — the soft-spread form of the sequential-commit kernel (msh_schedule_sequential_soft on a ctx
// with a SCHEDULE_ANYWAY group): the preference form (msh_seq_prefs.hip) with the scoring half of upstream's
// PodTopologySpread (pkg/scheduler/framework/plugins/podtopologyspread/scoring.go, one constraint per group, the
// zone key) for the pods of a soft group. The preference kernel is not edited for it: its per-pod record, score
// policy are repeated here (SoftRow, SoftScore; the quotients are msh_seq_quot.h's) and the step below is its step plus
// what follows. A group's mode travels in the sign of its max_skew in LDS (SoftArgs::soft; negative: soft).
// Per pod of a soft group g (workgroup-uniform, as the group is):
//  1. no spread filter: the hard groups' `allowed` ballot is skipped and hz is not ANDed into pod.av, so the feasible
//     set F is an ungrouped pod's and nodes without a zone stay in it;
//  2. the zones of the feasible zoned nodes, Zs: every thread ORs 1 << zone over okm & hz, one wave OR per half that
//     the table's zones touch, then atomicOr into two more dwords of the maxima slot, ms[3][4] = [max A, max T, Zs lo,
//     Zs hi]. It is the phase and the barrier of the A / T maxima: a pod runs it if any_a || any_t || soft, so a
//     soft pod costs one barrier more than its preference step, or none if its class has a raw value. The slots
//     rotate on msl, the count of pods that ran the phase, exactly as before: a pod that skips the phase neither
//     adds to a slot nor advances msl, so every wave sees the same slot for the same pod. After barrier s of the
//     phase the slot read at s - 1 is free (every wave has arrived at barrier s since its read), all four dwords of
//     it are zeroed by wave 0's first four threads, and it is next added to at s + 2, behind barrier s + 1. Zero is
//     the identity of max over unsigned values and of OR, so one reset serves all four;
//  3. on lane z of Zs: raw_z = Round(double(cnt[g][z]) * log(size + 2) + double(max_skew - 1)), size = |Zs|, the
//     weights a table of the host's std::log (copied to LDS in the prologue), the product and the sum two IEEE double
//     operations with contraction off, Round half away from zero as Go's math.Round (soft_raw); mx and mn over Zs by
//     wave_reduce; ns_z = 100 if mx == 0, else 100 * (mx + mn - raw_z) / mx truncated (quot_soft, exact);
//  4. node k's term: ns of lane zone[k] by ds_bpermute, 0 without a zone, times w_spread, added to the sum. The key
//     holds 100 * (W_res + w_aff + w_taint + w_spread) <= 65,534 (host check).
// With Zs empty every ns is 0. A pod of a hard group or of none runs the preference step unchanged (ns = 0).
// Commit: the group's count of the selected node's zone goes up only if that node has a zone (a soft pod may land
// on one without); the barrier after a grouped pod's commit stays, workgroup-uniform.
// Bounds (host checks): counts during a call <= 2^25, max_skew of a soft group <= 2^24, so raw < 2^28.
// Table limits: the preference kernel's; registers in profiles/soft_spread_regs.json.
#include "msh_seq_score_policy.h"

namespace msh {

template <int NR, int NPL, bool MOST>
struct SoftScore : ScoreArgmax<NR, NPL, MOST> {
  using Base = ScoreArgmax<NR, NPL, MOST>;
  static constexpr int K = Base::K;
  const uint32_t wres;  // the resource score's plugin weight, 0 in mode NONE
  __device__ __forceinline__ SoftScore(const SpreadScoreArgs& ss)
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
struct alignas(4 * NPL) SoftRow {
  uint32_t v[NPL];
  uint32_t adm;
  uint32_t pad[NPL - 1];
};

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_soft_kernel(SoftArgs so) {
  static_assert(NPL == 2 || NPL == 4, "a row is one 8- or 16-byte load per thread");
  using P = SoftScore<NR, NPL, MOST>;
  constexpr int K = P::K;
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ uint32_t xs[3][P::SLOT];
  __shared__ uint32_t ms[3][4];  // [max A, max T, Zs lo, Zs hi] of the pods that run the shared phase
  __shared__ double lw[SPREAD_ZONES + 1];  // log(size + 2)
  extern __shared__ int32_t lcnt[];  // [G][SPREAD_ZONES] counts, then [G] max_skew, negated for a soft group
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
  int32_t* lskew = lcnt + G * SPREAD_ZONES;
  const bool in_zset = ((sa.zset >> lane) & 1ull) != 0;  // lane z: zone z occurs on a node
  const uint32_t w_aff = pa.w_aff, w_taint = pa.w_taint, w_spread = so.w_spread;
  const bool zs_lo = (uint32_t)sa.zset != 0u, zs_hi = (sa.zset >> 32) != 0ull;  // the halves the table's zones touch

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
  for (int32_t e = t; e < G; e += NW * WAVE) {  // G <= SPREAD_MAX_GROUPS = 128: two words of mode bits
    const int32_t sk = sa.max_skew[e];
    lskew[e] = (((e < 64 ? so.soft[0] : so.soft[1]) >> (e & 63)) & 1ull) != 0 ? -sk : sk;
  }
  if (G > 0)
    for (int32_t e = t; e <= SPREAD_ZONES; e += NW * WAVE) lw[e] = so.zone_weight[e];
  if (NW > 1 && threadIdx.x < 3 * P::SLOT) (&xs[0][0])[threadIdx.x] = P::IDENT;
  if (NW > 1 && threadIdx.x < 3 * 4) (&ms[0][0])[threadIdx.x] = 0u;
  __syncthreads();
  int sl = 0, msl = 0;

  // the row of class c (wave-uniform) for the thread's nodes and their admit bits; class -1: zeros, all admitted
  uint32_t row_n[NPL];
  uint32_t adm_n = KMASK;
  auto fetch = [&](int32_t c) {
    if (c >= 0) {
      const SoftRow<NPL>* rc = reinterpret_cast<const SoftRow<NPL>*>(pa.rows) + c * PREF_THREADS;  // uniform
      const SoftRow<NPL>& rec = rc[(uint32_t)t];
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
          za |= (uint32_t)((allowed >> ((uint32_t)(zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1))) & 1ull) << k;
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
            zm |= (uint64_t)((okm & hz) >> k & 1u) << ((uint32_t)(zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1));
          const auto bor = [](uint32_t x, uint32_t y) { return x | y; };
          zlo = zs_lo ? wave_reduce((uint32_t)zm, bor) : 0u;
          zhi = zs_hi ? wave_reduce((uint32_t)(zm >> 32), bor) : 0u;
        }
        if constexpr (NW > 1) {
          if (lane == 0) {
            if (ma != 0u) atomicMax(&ms[msl][0], ma);
            if (mt != 0u) atomicMax(&ms[msl][1], mt);
            if (zlo != 0u) atomicOr(&ms[msl][2], zlo);
            if (zhi != 0u) atomicOr(&ms[msl][3], zhi);
          }
          lds_barrier();
          ma = (uint32_t)__builtin_amdgcn_readfirstlane((int)ms[msl][0]);
          mt = (uint32_t)__builtin_amdgcn_readfirstlane((int)ms[msl][1]);
          zlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)ms[msl][2]);
          zhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)ms[msl][3]);
          // the slot read one phase ago is free now and is next added to two phases ahead (see the head comment)
          if (threadIdx.x < 4) ms[msl == 0 ? 2 : msl - 1][threadIdx.x] = 0u;
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
      const uint64_t zs = ((uint64_t)zhi << 32) | zlo;
      if (soft && zs != 0ull) {  // workgroup-uniform; with Zs empty ns = 0 on every node
        const double w = lw[__builtin_popcountll(zs)];  // a uniform address: one broadcast read
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
          const int32_t zk = (int32_t)((uint32_t)(zones >> (8 * k)) & (uint32_t)(SPREAD_ZONES - 1));
          const uint32_t nk = (uint32_t)__builtin_amdgcn_ds_bpermute(zk << 2, ns);  // every lane is active here
          sum[k] += ((hz >> k) & 1u) ? w_spread * nk : 0u;
        }
      }
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
          // a grouped pod placed on a node with a zone: one more pod of the group in that zone (a pod of a hard
          // group always lands on one, a soft pod need not)
          if (pg >= 0 && ((hz >> ks) & 1u)) lcnt[pg * SPREAD_ZONES + ((uint32_t)(zones >> (8 * ks)) & (uint32_t)(SPREAD_ZONES - 1))] += 1;
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
struct SoftFamily {
  static constexpr int NPL2 = 4, NPL4 = 2;  // seq_prefs_kernel's
  template <int NR, int NPL, int NW>
  static auto kernel(const SoftArgs& a) {
    return a.p.ss.most ? seq_soft_kernel<NR, NPL, NW, true> : seq_soft_kernel<NR, NPL, NW, false>;
  }
};
}  // namespace

static_assert(PREF_THREADS == SEQ_FRAME_MAX_WAVES * WAVE, "one record per thread of the largest instance");
static_assert(SPREAD_MAX_GROUPS == 128, "SoftArgs::soft is two words");

int32_t seq_soft_max_nodes(int32_t nres) { return seq_frame_max_nodes<SoftFamily>(nres); }
int32_t seq_soft_npl(int32_t nres) { return nres <= 2 ? SoftFamily::NPL2 : SoftFamily::NPL4; }

hipError_t launch_seq_soft(const SoftArgs& a, hipStream_t s, std::string* err) {
  const SpreadArgs& sa = a.p.ss.s;
  if (sa.f.s.n_pods == 0) return hipSuccess;
  if (sa.n_groups < 0 || sa.n_groups > SPREAD_MAX_GROUPS || a.p.n_classes < 0 || a.p.n_classes > CLASS_MAX) return hipErrorInvalidValue;
  if (100ull * ((uint64_t)a.p.ss.weight + a.p.w_aff + a.p.w_taint + a.w_spread) > 65534ull) return hipErrorInvalidValue;  // the key's sum
  if (sa.n_groups > 0 && !a.zone_weight) return hipErrorInvalidValue;
  const size_t lds = (size_t)sa.n_groups * (SPREAD_ZONES + 1) * sizeof(int32_t);  // at most 33,280 bytes
  return launch_seq_frame<SoftFamily>(a, sa.f, "soft-spread", lds, s, err);
}

}  // namespace msh
