// msh_tiebreak.hip — MSH_TIEBREAK_RANDOM: a seeded, reproducible uniform choice among the nodes that
// hold a pod's maximum total (the reference's selectHost reservoir scan, minisched.go:304-325, as a
// counter-based draw). pair_pick_kernel replaces pair_kernel / pair_lds_kernel on the batch entry
// points of a ctx in RANDOM mode; a ctx in MSH_TIEBREAK_FIRST never launches it.
//
// The first-max kernels only ever look for the first hit of a class. Picking the k-th of c tied nodes
// takes two passes over the bit planes (msh_internal.h PLANE_* layout), every (pod, node) pair
// evaluated from the planes in both:
//   A (count)   per 32-node word, fe = V & ~(X & nT) and dm = OR_k (D_k ^ P_k); cf += popc(fe),
//               cm += popc(fe & ~dm) (v_bcnt_u32_b32 adds into its second operand: one VALU each).
//   decide      status and score from decode_pod on the classes' presence; the tie set from the same
//               case analysis (tie_kind below); k = mulhi(u, c), u = the pod's SplitMix64 draw.
//   B (select)  the groups again in List order, the popcount of the tie set's words added to a prefix
//               until prefix + popc(group) > k; the lane keeps that group and k - prefix, and after
//               the loop walks its group's eight words the same way and finds the set bit of the
//               rank left by five halving steps.
// One pod per lane, PK_BPW 64-pod blocks per wave (a group's planes are read once and applied to
// both), blockIdx.y = the batch of a multi-batch launch, as pair_lds_kernel lays pods out.
#include "msh_device.h"

#include <algorithm>

namespace msh {

namespace {

constexpr int PK_BPW = 2;         // 64-pod blocks per wave
constexpr int PK_WAVES = 4;       // waves per workgroup: tables up to PK_SMALL_GROUPS groups in LDS, and global planes
constexpr int PK_WAVES_BIG = 16;  // larger LDS tables: one copy of up to 78 KB serves 16 waves
constexpr int PK_SMALL_GROUPS = 128;  // 32,768 nodes, 24 KB of LDS per workgroup

// The high 32 bits of SplitMix64 at position `counter` of the stream seeded with `seed`
// (include/minisched_hip.h, "Tie-break").
__device__ __forceinline__ uint32_t draw_u32(uint64_t seed, uint64_t counter) {
  uint64_t z = seed + (counter + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 32);
}

// The planes of group g into VGPRs: wave-uniform addresses (LDS: broadcast reads; global: through L2).
__device__ __forceinline__ void pick_group(uint32_t (&pl)[PLANE_N][PLANE_GW], const uint4* __restrict__ tab, int32_t g) {
  const uint4* q = tab + (size_t)g * (GROUP_DWORDS / 4);
#pragma unroll
  for (int k = 0; k < PLANE_N; ++k) {
    const uint4 lo = q[2 * k], hi = q[2 * k + 1];
    pl[k][0] = lo.x; pl[k][1] = lo.y; pl[k][2] = lo.z; pl[k][3] = lo.w;
    pl[k][4] = hi.x; pl[k][5] = hi.y; pl[k][6] = hi.z; pl[k][7] = hi.w;
  }
}

// dm of word w: a set bit = the node's NodeNumber code differs from the pod's.
__device__ __forceinline__ uint32_t pick_miss(const uint32_t (&pl)[PLANE_N][PLANE_GW], int w, uint32_t P0, uint32_t P1,
                                              uint32_t P2, uint32_t P3) {
  uint32_t t = pl[0][w] ^ P0;
  t = bop3_or_xor(t, pl[1][w], P1);
  t = bop3_or_xor(t, pl[2][w], P2);
  return bop3_or_xor(t, pl[3][w], P3);
}

// The tie set's word w: fe & ((dm ^ inv) | all), inv = all-ones when the set is the matches, all = all-ones
// when it is every feasible node.
__device__ __forceinline__ uint32_t tie_word(const uint32_t (&pl)[PLANE_N][PLANE_GW], int w, uint32_t P0, uint32_t P1,
                                             uint32_t P2, uint32_t P3, uint32_t nT, uint32_t inv, uint32_t all) {
  const uint32_t fe = bop3_andn_of_and(pl[PLANE_V][w], pl[PLANE_X][w], nT);  // V & ~(X & nT)
  return fe & bop3_or_xor(all, pick_miss(pl, w, P0, P1, P2, P3), inv);
}

// The position of set bit number r (0-based, r < popc(x)) of x: five halving steps, no lane-divergent loop.
__device__ __forceinline__ uint32_t select_bit(uint32_t x, uint32_t r) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t sh = 16; sh >= 1; sh >>= 1) {
    const uint32_t c = (uint32_t)__popc(x & ((1u << sh) - 1u));
    const bool up = r >= c;
    r -= up ? c : 0u;
    x = up ? x >> sh : x;
    pos += up ? sh : 0u;
  }
  return pos;
}

// The tie set of a PLACED pod from the classes present among its feasible nodes (cm matches, cx
// non-matches), the case analysis of decode_pod carried from "first of the class" to "the class":
//   NONE / DEFAULT         matches score 10w / 100w, the rest 0: the matches if cm > 0, else all feasible
//   REVERSE                non-matches 100w, matches 0:         the non-matches if any, else all feasible
//                          (every feasible node is then a match)
//   MINMAX                 matches 100w, non-matches 0 when both classes are present; one class alone
//                          normalizes to 0 everywhere:          the matches if both, else all feasible
//   no NodeNumber score    every total 0:                       all feasible
// 0 = the feasible matches, 1 = the feasible non-matches, 2 = every feasible node.
__device__ __forceinline__ int tie_kind(const PluginParams& pp, uint32_t cm, uint32_t cx) {
  if (!pp.has_nn_score) return 2;
  if (pp.mode == 2) return cx ? 1 : 2;
  if (pp.mode == 3) return (cm && cx) ? 0 : 2;
  return cm ? 0 : 2;
}

template <bool LDSP, int W>
__global__ __launch_bounds__(W * WAVE) void pair_pick_kernel(PickArgs a) {
  extern __shared__ uint4 s_tab[];  // LDSP: n_groups * GROUP_DWORDS / 4
  const BatchDesc& d = a.d[blockIdx.y];
  const int32_t np = d.n_pods;
  const int32_t wg0 = (int32_t)blockIdx.x * (W * PK_BPW * WAVE);  // first pod of this workgroup
  if (wg0 >= np) return;  // the whole workgroup lies past its batch's end
  const uint4* __restrict__ g_tab = reinterpret_cast<const uint4*>(a.planes);
  const int32_t n_groups = a.n_groups;
  if constexpr (LDSP) {
    const int32_t nq = n_groups * (GROUP_DWORDS / 4);
    for (int32_t i = threadIdx.x; i < nq; i += W * WAVE) s_tab[i] = g_tab[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t P0[PK_BPW], P1[PK_BPW], P2[PK_BPW], P3[PK_BPW], nT[PK_BPW];
  int32_t jj[PK_BPW];
  bool digit[PK_BPW];
  bool any_act = false;
#pragma unroll
  for (int b = 0; b < PK_BPW; ++b) {
    const int32_t j = wg0 + (wv * PK_BPW + b) * WAVE + lane;
    uint32_t c = CODE_NONE_POD, t = 0u;
    if (j < np) {
      const int dq = d.pod_digit[j];
      c = (dq >= 0 && dq <= 9) ? (uint32_t)dq : CODE_NONE_POD;  // NodeNumber.PreScore: Atoi of the last byte
      t = d.pod_tol[j] ? 1u : 0u;
    }
    jj[b] = j;
    digit[b] = c != CODE_NONE_POD;
    P0[b] = 0u - (c & 1u);
    P1[b] = 0u - ((c >> 1) & 1u);
    P2[b] = 0u - ((c >> 2) & 1u);
    P3[b] = 0u - (c >> 3);
    nT[b] = t ? 0u : 0xFFFFFFFFu;
    any_act = any_act || __ballot(j < np) != 0;
  }
  if (!any_act) return;  // wave-uniform; no barrier below

  // ---- pass A: per pod, the feasible nodes (cf) and the feasible matches (cm) ----
  uint32_t cf[PK_BPW], cm[PK_BPW];
#pragma unroll
  for (int b = 0; b < PK_BPW; ++b) cf[b] = cm[b] = 0u;
  for (int32_t g = 0; g < n_groups; ++g) {
    uint32_t pl[PLANE_N][PLANE_GW];
    if constexpr (LDSP) pick_group(pl, s_tab, g);
    else pick_group(pl, g_tab, g);
#pragma unroll
    for (int b = 0; b < PK_BPW; ++b) {
#pragma unroll
      for (int w = 0; w < PLANE_GW; ++w) {
        const uint32_t fe = bop3_andn_of_and(pl[PLANE_V][w], pl[PLANE_X][w], nT[b]);  // V & ~(X & nT)
        const uint32_t dm = pick_miss(pl, w, P0[b], P1[b], P2[b], P3[b]);
        cf[b] += (uint32_t)__popc(fe);
        cm[b] += (uint32_t)__popc(bop3_andn(fe, dm));
      }
    }
  }

  // ---- decide: status / score as decode_pod gives them, the tie set and the rank k in it ----
  int32_t ost[PK_BPW];
  int64_t osc[PK_BPW];
  uint32_t kk[PK_BPW], inv[PK_BPW], all[PK_BPW];
  bool done[PK_BPW];
#pragma unroll
  for (int b = 0; b < PK_BPW; ++b) {
    const uint32_t cx = cf[b] - cm[b];
    int32_t oi;
    decode_pod(cm[b] ? 0 : -1, cx ? 0 : -1, cf[b] ? 0 : -1, digit[b], a.pp, &oi, &osc[b], &ost[b]);
    const int kind = tie_kind(a.pp, cm[b], cx);
    const uint32_t c = kind == 0 ? cm[b] : (kind == 1 ? cx : cf[b]);
    // pod j draws at counter base + j whatever its status; k = (u * c) >> 32 < c
    kk[b] = __umulhi(draw_u32(a.seed, a.draw_base[blockIdx.y] + (uint64_t)(uint32_t)jj[b]), c);
    inv[b] = kind == 0 ? 0xFFFFFFFFu : 0u;  // the tie set's word = fe & ((dm ^ inv) | all)
    all[b] = kind == 2 ? 0xFFFFFFFFu : 0u;
    done[b] = jj[b] >= np || ost[b] != 0;   // nothing to select
  }

  // ---- pass B: the group that holds the tie set's k-th node, and the rank left inside it ----
  // (the hit test once per group, not per word: the per-word form, 16 VALU per word with its selects, ran
  // the C3 launch at 4.2x the first-max kernel, profiles/tiebreak_c3_perword.json)
  uint32_t prefix[PK_BPW], selg[PK_BPW], selr[PK_BPW];
#pragma unroll
  for (int b = 0; b < PK_BPW; ++b) prefix[b] = selg[b] = selr[b] = 0u;
  for (int32_t g = 0; g < n_groups; ++g) {
    bool open = false;  // lanes stop at different groups: the loop stays wave-uniform and ends with the last lane
#pragma unroll
    for (int b = 0; b < PK_BPW; ++b) open = open || __ballot(!done[b]) != 0;
    if (!open) break;
    uint32_t pl[PLANE_N][PLANE_GW];
    if constexpr (LDSP) pick_group(pl, s_tab, g);
    else pick_group(pl, g_tab, g);
#pragma unroll
    for (int b = 0; b < PK_BPW; ++b) {
      uint32_t cnt = 0u;
#pragma unroll
      for (int w = 0; w < PLANE_GW; ++w) cnt += (uint32_t)__popc(tie_word(pl, w, P0[b], P1[b], P2[b], P3[b], nT[b], inv[b], all[b]));
      const bool hit = !done[b] && prefix[b] + cnt > kk[b];
      selg[b] = hit ? (uint32_t)g : selg[b];
      selr[b] = hit ? kk[b] - prefix[b] : selr[b];
      done[b] = done[b] || hit;
      prefix[b] += cnt;
    }
  }
  // inside the lane's own group (a per-lane address: once per pod): the word that holds rank selr, then the
  // set bit of the rank left, by halving steps
  uint32_t node[PK_BPW];
#pragma unroll
  for (int b = 0; b < PK_BPW; ++b) {
    uint32_t pl[PLANE_N][PLANE_GW];
    if constexpr (LDSP) pick_group(pl, s_tab, (int32_t)selg[b]);
    else pick_group(pl, g_tab, (int32_t)selg[b]);
    uint32_t pre = 0u, selw = 0u, rank = 0u, wsel = 0u;
    bool found = false;
#pragma unroll
    for (int w = 0; w < PLANE_GW; ++w) {
      const uint32_t tw = tie_word(pl, w, P0[b], P1[b], P2[b], P3[b], nT[b], inv[b], all[b]);
      const uint32_t cnt = (uint32_t)__popc(tw);
      const bool hit = !found && pre + cnt > selr[b];
      selw = hit ? tw : selw;
      rank = hit ? selr[b] - pre : rank;
      wsel = hit ? (uint32_t)w : wsel;
      found = found || hit;
      pre += cnt;
    }
    node[b] = selg[b] * GROUP_NODES + wsel * 32u + select_bit(selw, rank);
  }

#pragma unroll
  for (int b = 0; b < PK_BPW; ++b) {
    const int32_t j = jj[b];
    if (j < np) {
      d.out_idx[j] = ost[b] == 0 ? (int32_t)node[b] : -1;
      if (d.out_score) d.out_score[j] = osc[b];
      d.out_status[j] = ost[b];
    }
  }
}

template <bool LDSP, int W>
hipError_t launch_pick(const PickArgs& a, int32_t maxp, hipStream_t s) {
  const int32_t per_wg = W * PK_BPW * WAVE;
  const dim3 grid((unsigned)((maxp + per_wg - 1) / per_wg), (unsigned)a.nb), blk(W * WAVE);
  const size_t bytes = LDSP ? (size_t)a.n_groups * GROUP_DWORDS * sizeof(uint32_t) : 0;
  if (bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pair_pick_kernel<LDSP, W>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  MSH_TIMED_LAUNCH((pair_pick_kernel<LDSP, W>), grid, blk, (unsigned)bytes, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_pair_pick(const PickArgs& a, hipStream_t s) {
  if (a.nb <= 0 || a.nb > MULTI_MAX) return hipErrorInvalidValue;
  int32_t maxp = 0;
  for (int b = 0; b < a.nb; ++b) maxp = std::max(maxp, a.d[b].n_pods);
  if (maxp == 0) return hipSuccess;
  // the planes in LDS while the table fits (the limit of launch_pairs for pair_lds_kernel), else from
  // global memory through L2
  if (a.n_groups <= PK_SMALL_GROUPS) return launch_pick<true, PK_WAVES>(a, maxp, s);
  if (a.n_groups <= TIEBREAK_LDS_MAX_GROUPS) return launch_pick<true, PK_WAVES_BIG>(a, maxp, s);
  return launch_pick<false, PK_WAVES>(a, maxp, s);
}

}  // namespace msh
