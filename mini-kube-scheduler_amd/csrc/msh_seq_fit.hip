// msh_seq_fit.hip — the resource-fit form of the sequential-commit kernel (msh_schedule_sequential_fit): the
// capacity form's in-order loop (msh_seq_cap.hip) with one more conjunct in feasibility, upstream's
// NodeResourcesFit: pod j fits node i only when, for every resource r it asks for, req[r][j] <= alloc[r][i] -
// used[r][i]. Feasibility is then a true (pod, node) predicate over 64-bit quantities, so the node state is not
// the availability planes of seq_capu_kernel but per-node registers:
//  * thread t of the one workgroup holds NPL consecutive nodes, t * NPL .. t * NPL + NPL - 1 (lanes and waves in
//    List order), and for each the free amount alloc - used per resource (int64, NR x NPL register pairs), the
//    remaining pod count eff - count (int32), the NodeNumber code (4 bits) and the two availability bits
//    (V & ~X for pods that do not tolerate the unschedulable taint, V for those that do), all taken from the
//    existing planes, counts, capacity column and resource table in the prologue;
//  * per pod (code, ~tolerates and the requests wave-uniform, read from the lanes that loaded the 64-pod block)
//    every lane evaluates its NPL nodes: per resource one v_cmp_le_i64 against the free amount ORed with the
//    request's "is zero" mask, ANDed with the availability bit and remaining count > 0; the lane's first feasible
//    match, non-match (REVERSE / MINMAX) and node, the wave's first by wave_first, the workgroup's by an LDS
//    minimum behind one LDS-only barrier (NW > 1; triple-buffered slots as in seq_body);
//  * decode_pod / decode_ident give status, node and score; thread 0 stores them, and the thread that holds the
//    selected node subtracts the requests and one pod. One pod per step: no speculation.
// The epilogue writes used = alloc - free and count = eff - remaining back. A zero request never rejects, also on
// a node whose alloc a patch lowered below used (negative free). Values stay within int64: alloc, used and the
// requests are in [0, 2^62].
// Table limit: NW <= 16 waves x 64 lanes x NPL nodes, NPL = 8 for up to two resources (8,192 nodes) and 4 for
// three or four (4,096), so that a lane's free amounts are 32 VGPRs in either case. A table of one or three
// resources runs the two- or four-resource instance with the spare resources' requests and free amounts zero.
#include "msh_seq_kernel.h"

namespace msh {

template <int NR, int NPL, int NW, bool KX>
__global__ __launch_bounds__(NW * WAVE) void seq_fit_kernel(FitArgs fa) {
  static_assert(32 % NPL == 0 && NPL * 4 <= 32, "a thread's nodes lie in one word, their codes in one register");
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  constexpr uint32_t KMASK = (1u << NPL) - 1u;
  __shared__ uint32_t xs[3][3];  // [slot][first match, first feasible, first feasible non-match]
  const SeqArgs& a = fa.s;
  const int lane = threadIdx.x & (WAVE - 1);
  const int32_t t = (int32_t)threadIdx.x;
  const int32_t slots = a.n_words * 32;
  const int32_t i0 = t * NPL;
  const bool held = i0 < slots;  // then all NPL nodes are slots of the table (NPL divides 32)
  const int32_t nres = fa.nres;
  const int32_t max_pods = a.max_pods;

  int64_t fr[NR][NPL];
  int32_t rem[NPL];
  uint32_t codes = 0xFFFFFFFFu;  // code 15: never a match
  uint32_t av0 = 0u, av1 = 0u;
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
    }
  }
  if (NW > 1) {
    if (threadIdx.x < 9) (&xs[0][0])[threadIdx.x] = NONE;
    __syncthreads();
  }
  int sl = 0;

  PluginParams pp = a.pp;
  const IdentDecode idec = make_ident_decode(pp);
  const uint32_t base = (uint32_t)i0;
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
      uint32_t cm = NONE, ca = NONE, cx = NONE;
#pragma unroll
      for (int k = NPL - 1; k >= 0; --k) {  // descending: the lane's first node wins
        bool ok = ((av >> k) & 1u) != 0 && rem[k] > 0;
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
}

namespace {
constexpr int FIT_NPL2 = 8, FIT_NPL4 = 4;  // nodes per thread: up to two resources, three or four
constexpr int FIT_MAX_WAVES = 16;

template <int NR, int NPL, int NW>
hipError_t launch_fit_nw(const FitArgs& a, hipStream_t s) {
  auto kx = seq_fit_kernel<NR, NPL, NW, true>;
  auto id = seq_fit_kernel<NR, NPL, NW, false>;
  if (needs_kx(a.s.pp)) MSH_TIMED_LAUNCH(kx, dim3(1), dim3(NW * WAVE), 0, s, a);
  else MSH_TIMED_LAUNCH(id, dim3(1), dim3(NW * WAVE), 0, s, a);
  return hipGetLastError();
}

// as few waves as hold the table: 1, 4 or 16
template <int NR, int NPL>
hipError_t launch_fit_nr(const FitArgs& a, hipStream_t s) {
  const int32_t n = a.s.n_nodes;
  if (n <= 1 * WAVE * NPL) return launch_fit_nw<NR, NPL, 1>(a, s);
  if (n <= 4 * WAVE * NPL) return launch_fit_nw<NR, NPL, 4>(a, s);
  return launch_fit_nw<NR, NPL, FIT_MAX_WAVES>(a, s);
}

__global__ void res_patch_kernel(const int32_t* idx, const int64_t* alloc, const int64_t* used, int32_t count,
                                 int32_t nres, int64_t stride, int64_t* d_alloc, int64_t* d_used) {
  const int32_t e = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= count * nres) return;
  const int32_t r = e / count, k = e % count;
  if (alloc) d_alloc[r * stride + idx[k]] = alloc[e];
  if (used) d_used[r * stride + idx[k]] = used[e];
}
}  // namespace

int32_t seq_fit_max_nodes(int32_t nres) { return FIT_MAX_WAVES * WAVE * (nres <= 2 ? FIT_NPL2 : FIT_NPL4); }

hipError_t launch_seq_fit(const FitArgs& a, hipStream_t s, std::string* err) {
  if (a.s.n_pods == 0) return hipSuccess;
  if (a.s.n_nodes > seq_fit_max_nodes(a.nres)) {
    if (err)
      *err = "the resource-fit form keeps the node state in registers: at most " +
             std::to_string(seq_fit_max_nodes(a.nres)) + " nodes per device with " + std::to_string(a.nres) +
             (a.nres == 1 ? " resource" : " resources");
    return hipErrorInvalidValue;
  }
  if (a.nres <= 2) return launch_fit_nr<2, FIT_NPL2>(a, s);
  return launch_fit_nr<4, FIT_NPL4>(a, s);
}

hipError_t launch_res_patch(const int32_t* idx, const int64_t* alloc, const int64_t* used, int32_t count, int32_t nres,
                            int64_t stride, int64_t* d_alloc, int64_t* d_used, hipStream_t s) {
  const int32_t total = count * nres;
  if (total <= 0) return hipSuccess;
  res_patch_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(idx, alloc, used, count, nres, stride,
                                                                              d_alloc, d_used);
  return hipGetLastError();
}

}  // namespace msh
