// msh_seq_fit.hip — the resource-fit form of the sequential-commit kernel (msh_schedule_sequential_fit): the
// capacity form's in-order loop (msh_seq_cap.hip) with one more conjunct in feasibility, upstream's
// NodeResourcesFit: pod j fits node i only when, for every resource r it asks for, req[r][j] <= alloc[r][i] -
// used[r][i]. Feasibility is then a true (pod, node) predicate over 64-bit quantities, so the node state is not
// the availability planes of seq_capu_kernel but per-node registers: the frame of msh_seq_frame.h, with its
// FirstFeasible policy and nothing added.
// Table limit: 16 waves x 64 lanes x NPL nodes, NPL = 8 for up to two resources (8,192 nodes) and 4 for three or
// four (4,096), so that a lane's free amounts are 32 VGPRs in either case.
#include "msh_seq_frame.h"

namespace msh {

template <int NR, int NPL, int NW, bool KX>
__global__ __launch_bounds__(NW * WAVE) void seq_fit_kernel(FitArgs fa) {
  FirstFeasible<KX> p(fa.s.pp);
  seq_frame<NR, NPL, NW>(fa, p);
}

namespace {
struct FitFamily {
  static constexpr int NPL2 = 8, NPL4 = 4;  // nodes per thread: up to two resources, three or four
  template <int NR, int NPL, int NW>
  static auto kernel(const FitArgs& a) {
    return needs_kx(a.s.pp) ? seq_fit_kernel<NR, NPL, NW, true> : seq_fit_kernel<NR, NPL, NW, false>;
  }
};

__global__ void res_patch_kernel(const int32_t* idx, const int64_t* alloc, const int64_t* used, int32_t count,
                                 int32_t nres, int64_t stride, int64_t* d_alloc, int64_t* d_used) {
  const int32_t e = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= count * nres) return;
  const int32_t r = e / count, k = e % count;
  if (alloc) d_alloc[r * stride + idx[k]] = alloc[e];
  if (used) d_used[r * stride + idx[k]] = used[e];
}
}  // namespace

int32_t seq_fit_max_nodes(int32_t nres) { return seq_frame_max_nodes<FitFamily>(nres); }

hipError_t launch_seq_fit(const FitArgs& a, hipStream_t s, std::string* err) {
  if (a.s.n_pods == 0) return hipSuccess;
  return launch_seq_frame<FitFamily>(a, a, "resource-fit", 0, s, err);
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
