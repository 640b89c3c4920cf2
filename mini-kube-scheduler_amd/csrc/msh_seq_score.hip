// msh_seq_score.hip — the scored resource-fit form of the sequential-commit kernel: msh_schedule_sequential_fit on
// a ctx whose msh_set_resource_score mode is LEAST_ALLOCATED or MOST_ALLOCATED (upstream's
// NodeResourcesLeastAllocated / NodeResourcesMostAllocated, noderesources/least_allocated.go, most_allocated.go).
// Feasibility, status and the commit are seq_fit_kernel's (msh_seq_fit.hip); the total of a feasible node i for pod
// j is NodeNumber's total plus weight x RS(j, i),
//   q_r = used[r][i] + req[r][j], c_r = alloc[r][i],
//   s_r = 0 when c_r == 0 or q_r > c_r, else (c_r - q_r) * 100 / c_r (LEAST) or q_r * 100 / c_r (MOST),
//   RS  = (sum_r s_r * rw[r]) / (sum_r rw[r]),
// in int64 with truncating division, and the pod goes to the first maximum in List order. RS moves with every
// commit, so the reduction is an arg-max, not seq_fit_kernel's "first feasible node of a class". The frame is
// msh_seq_frame.h's; the kernel is its ScoreArgmax policy (msh_seq_score_policy.h, which seq_spread_score_kernel
// uses too):
//  * besides the frame's free amounts alloc - used a thread keeps the allocatable amount c (the divisor,
//    loop-invariant) and 100 / c as a float, per node and resource, and writes used back from them;
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
//    wave by DPP (wave_reduce), the workgroup by the frame's meet with an LDS atomic maximum;
//  * on the uniform path the two candidates' totals are compared: the larger wins, the lower node at a tie.
// Table limit: 16 waves x 64 lanes x NPL nodes with NPL = 4 up to two resources (4,096 nodes) and 2 for three or
// four (2,048), half of seq_fit_kernel's: the allocatable amounts double a node's registers
// (msh_seq_fit_max_nodes reports both).
#include "msh_seq_score_policy.h"

namespace msh {

template <int NR, int NPL, int NW, bool MOST>
__global__ __launch_bounds__(NW * WAVE) void seq_score_kernel(FitScoreArgs sa) {
  ScoreArgmax<NR, NPL, MOST> p(sa);
  seq_frame<NR, NPL, NW>(sa.f, p);
}

namespace {
// nodes per thread, up to two resources and three or four: half of seq_fit_kernel's, since a node also keeps its
// allocatable amounts and their reciprocals (64 + 16 VGPRs of node state either way; with seq_fit_kernel's 8 / 4
// the 16-wave instances, 128 VGPRs per wave, spill 148-192 bytes per lane to scratch)
struct ScoreFamily {
  static constexpr int NPL2 = 4, NPL4 = 2;
  template <int NR, int NPL, int NW>
  static auto kernel(const FitScoreArgs& a) {
    return a.most ? seq_score_kernel<NR, NPL, NW, true> : seq_score_kernel<NR, NPL, NW, false>;
  }
};
}  // namespace

int32_t seq_score_max_nodes(int32_t nres) { return seq_frame_max_nodes<ScoreFamily>(nres); }

hipError_t launch_seq_score(const FitScoreArgs& a, hipStream_t s, std::string* err) {
  if (a.f.s.n_pods == 0) return hipSuccess;
  return launch_seq_frame<ScoreFamily>(a, a.f, "scored resource-fit", 0, s, err);
}

}  // namespace msh
