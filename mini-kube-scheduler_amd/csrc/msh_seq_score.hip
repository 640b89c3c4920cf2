// msh_seq_score.hip — the scored resource-fit form of the sequential-commit kernel: msh_schedule_sequential_fit on
// a ctx whose msh_set_resource_score mode is LEAST_ALLOCATED or MOST_ALLOCATED (upstream's
// NodeResourcesLeastAllocated / NodeResourcesMostAllocated, noderesources/least_allocated.go, most_allocated.go).
// Feasibility, status and the commit are seq_fit_kernel's (msh_seq_fit.hip); the total of a feasible node i for pod
// j is NodeNumber's total plus weight x RS(j, i),
//   q_r = used[r][i] + req[r][j], c_r = alloc[r][i],
//   s_r = 0 when c_r == 0 or q_r > c_r, else (c_r - q_r) * 100 / c_r (LEAST) or q_r * 100 / c_r (MOST),
//   RS  = (sum_r s_r * rw[r]) / (sum_r rw[r]),
// in int64 with truncating division, and the pod goes to the first maximum in List order. RS moves with every
// commit, so the reduction is an arg-max, not seq_fit_kernel's "first feasible node of a class":
//  * thread t holds NPL consecutive nodes as in seq_fit_kernel, and besides the free amounts alloc - used the
//    allocatable amount c (the divisor, loop-invariant) and 100 / c as a float, per node and resource;
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
//    wave by DPP, the workgroup by an LDS atomic maximum into triple-buffered slots behind one LDS-only barrier
//    (as seq_fit_kernel's minimum);
//  * on the uniform path the two candidates' totals are compared: the larger wins, the lower node at a tie.
// Table limit: 16 waves x 64 lanes x NPL nodes with NPL = 4 up to two resources (4,096 nodes) and 2 for three or
// four (2,048), half of seq_fit_kernel's: the allocatable amounts double a node's registers
// (msh_seq_fit_max_nodes reports both).
#include "msh_seq_kernel.h"

namespace msh {

namespace {
// The wave's maximum (unsigned, every lane active), wave-uniform: four DPP steps leave every row of 16 lanes with
// its maximum, the four rows meet on the scalar side.
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return umax(umax(a, b), umax(c, d));
}

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
}  // namespace

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_score_kernel(FitScoreArgs sa) {
  static_assert(32 % NPL == 0 && NPL * 4 <= 32, "a thread's nodes lie in one word, their codes in one register");
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ uint32_t xs[3][2];  // [slot][best match key, best non-match key]
  const FitArgs& fa = sa.f;
  const SeqArgs& a = fa.s;
  const int lane = threadIdx.x & (WAVE - 1);
  const int32_t t = (int32_t)threadIdx.x;
  const int32_t slots = a.n_words * 32;
  const int32_t i0 = t * NPL;
  const bool held = i0 < slots;  // then all NPL nodes are slots of the table (NPL divides 32)
  const int32_t nres = fa.nres;
  const int32_t max_pods = a.max_pods;

  int64_t fr[NR][NPL], al[NR][NPL];
  float rc[NR][NPL];
  int32_t rem[NPL];
  uint32_t codes = 0xFFFFFFFFu;  // code 15: never a match
  uint32_t av0 = 0u, av1 = 0u;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    rem[k] = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      fr[r][k] = 0;
      al[r][k] = 0;
      rc[r][k] = 0.0f;
    }
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
        if (r < nres) {
          al[r][k] = fa.alloc[r * fa.res_stride + i];
          fr[r][k] = al[r][k] - fa.used[r * fa.res_stride + i];
          rc[r][k] = al[r][k] > 0 ? 100.0f / (float)al[r][k] : 0.0f;
        }
    }
  }
  if (NW > 1) {
    if (threadIdx.x < 6) (&xs[0][0])[threadIdx.x] = 0u;
    __syncthreads();
  }
  int sl = 0;

  const PluginParams pp = a.pp;
  const int64_t weight = sa.weight;
  const uint32_t magic = sa.wsum_magic;
  uint32_t rw[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) rw[r] = (uint32_t)sa.rw[r];
  const uint32_t kbase = 0xFFFFu - (uint32_t)i0;  // node i0 + k packs as kbase - k
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
      const uint32_t pc = pk & 15u;
      int64_t rq[NR];
      bool zr[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(rlo[r], jl);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(rhi[r], jl);
        rq[r] = (int64_t)(((uint64_t)hi << 32) | lo);
        zr[r] = rq[r] == 0;
      }
      const uint32_t av = (pk & 16u) ? av0 : av1;
      uint32_t km = 0u, kx = 0u;
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        bool ok = ((av >> k) & 1u) != 0 && rem[k] > 0;
        uint32_t acc = 0u;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int64_t d = fr[r][k] - rq[r];  // c - q
          ok = ok && (zr[r] || d >= 0);
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
        const bool mt = ((codes >> (4 * k)) & 15u) == pc;
        km = umax(km, mt ? key : 0u);
        kx = umax(kx, mt ? 0u : key);
      }
      km = wave_umax(km);
      kx = wave_umax(kx);
      if constexpr (NW > 1) {
        if (lane == 0) {
          atomicMax(&xs[sl][0], km);
          atomicMax(&xs[sl][1], kx);
        }
        lds_barrier();
        km = (uint32_t)__builtin_amdgcn_readfirstlane((int)xs[sl][0]);
        kx = (uint32_t)__builtin_amdgcn_readfirstlane((int)xs[sl][1]);
        // the slot read one step ago is free now (every reader passed this step's barrier) and is next
        // folded into two steps ahead (after the next barrier): wave 0 resets it in between
        if (threadIdx.x < 2) xs[sl == 0 ? 2 : sl - 1][threadIdx.x] = 0u;
        sl = sl == 2 ? 0 : sl + 1;
      }
      const bool has_m = km != 0u, has_x = kx != 0u;
      int64_t tm, tx;
      int32_t st;
      decode_classes(has_m, has_x, pc != CODE_NONE_POD, pp, &tm, &tx, &st);
      tm += weight * (int64_t)((km >> 16) - 1u);
      tx += weight * (int64_t)((kx >> 16) - 1u);
      const int32_t im = (int32_t)(0xFFFFu - (km & 0xFFFFu)), ix = (int32_t)(0xFFFFu - (kx & 0xFFFFu));
      const bool pick_m = has_m && (!has_x || tm > tx || (tm == tx && im < ix));
      const int32_t sel = st == 0 ? (pick_m ? im : ix) : -1;
      if (t == 0) {
        a.out_idx[j] = sel;
        if (a.out_score) a.out_score[j] = st == 0 ? (pick_m ? tm : tx) : 0;
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
        if (r < nres) fa.used[r * fa.res_stride + i] = al[r][k] - fr[r][k];
    }
  }
}

namespace {
// nodes per thread, up to two resources and three or four: half of seq_fit_kernel's, since a node also keeps its
// allocatable amounts and their reciprocals (64 + 16 VGPRs of node state either way; with seq_fit_kernel's 8 / 4
// the 16-wave instances, 128 VGPRs per wave, spill 148-192 bytes per lane to scratch)
constexpr int SCORE_NPL2 = 4, SCORE_NPL4 = 2;
constexpr int SCORE_MAX_WAVES = 16;

template <int NR, int NPL, int NW>
hipError_t launch_score_nw(const FitScoreArgs& a, hipStream_t s) {
  auto least = seq_score_kernel<NR, NPL, NW, false>;
  auto most = seq_score_kernel<NR, NPL, NW, true>;
  if (a.most) MSH_TIMED_LAUNCH(most, dim3(1), dim3(NW * WAVE), 0, s, a);
  else MSH_TIMED_LAUNCH(least, dim3(1), dim3(NW * WAVE), 0, s, a);
  return hipGetLastError();
}

// as few waves as hold the table: 1, 4 or 16
template <int NR, int NPL>
hipError_t launch_score_nr(const FitScoreArgs& a, hipStream_t s) {
  const int32_t n = a.f.s.n_nodes;
  if (n <= 1 * WAVE * NPL) return launch_score_nw<NR, NPL, 1>(a, s);
  if (n <= 4 * WAVE * NPL) return launch_score_nw<NR, NPL, 4>(a, s);
  return launch_score_nw<NR, NPL, SCORE_MAX_WAVES>(a, s);
}
}  // namespace

int32_t seq_score_max_nodes(int32_t nres) { return SCORE_MAX_WAVES * WAVE * (nres <= 2 ? SCORE_NPL2 : SCORE_NPL4); }

hipError_t launch_seq_score(const FitScoreArgs& a, hipStream_t s, std::string* err) {
  if (a.f.s.n_pods == 0) return hipSuccess;
  if (a.f.s.n_nodes > seq_score_max_nodes(a.f.nres)) {
    if (err)
      *err = "the scored resource-fit form keeps the node state in registers: at most " +
             std::to_string(seq_score_max_nodes(a.f.nres)) + " nodes per device with " + std::to_string(a.f.nres) +
             (a.f.nres == 1 ? " resource" : " resources");
    return hipErrorInvalidValue;
  }
  if (a.f.nres <= 2) return launch_score_nr<2, SCORE_NPL2>(a, s);
  return launch_score_nr<4, SCORE_NPL4>(a, s);
}

}  // namespace msh
