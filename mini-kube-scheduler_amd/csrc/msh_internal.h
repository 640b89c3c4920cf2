// msh_internal.h — shared between the C-ABI (msh_capi.cpp) and the gfx950 kernels (msh_prep.hip,
// msh_pair.hip, msh_generic.hip, msh_seq.hip). Not part of the public ABI (include/minisched_hip.h is).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace msh {

constexpr int32_t MAX_NODES = 0xFFFFFE;          // nodes per context (2^24 - 2)
constexpr int WAVE = 64;
constexpr int32_t GKEY_MAX = 0x7FFFFFFF;         // global (sharded) int32 key = GKEY_MAX - global_idx
constexpr uint32_t NOFIT = 0x80000000u;          // "no node" as a node index (above every real one)

// Per-ctx plugin set as the kernels see it (minisched/initialize.go:80-123 lists).
struct PluginParams {
  int32_t has_nu_filter;  // "NodeUnschedulable" in filter list
  int32_t has_nn_score;   // "NodeNumber" in score list
  int32_t nn_prescore;    // "NodeNumber" in prescore list (state written)
  int32_t mode;           // NodeNumber normalize mode (msh_normalize)
  int64_t weight;         // NodeNumber weight
};

// Whether the argmax needs the "first feasible NON-match" per pod (reverse / min-max
// normalization); otherwise the first feasible node of the pod's class suffices.
inline bool needs_kx(const PluginParams& pp) {
  return pp.has_nn_score && pp.nn_prescore && (pp.mode == 2 || pp.mode == 3);
}

// Device facts and launch choices, resolved once in msh_create / msh_create_ex (never on the launch
// path). The overrides come only from msh_create_ex's msh_options (tests and A/B measurement); the
// library reads no environment variable.
struct DeviceInfo {
  int cus = 256;
  int bits_slices = 0;   // msh_options.pair_slices: pair_kernel slice waves per pod block (1, 2, 4) and
                         // generic_kernel waves per pod group, 0 = auto
  int seq_waves = 0;     // msh_options.seq_waves: sequential scanning waves, 0 = auto
  // msh_options.batch_kernel: 0 = the per-pair bit-plane kernels for the reference's plugins (default);
  // 1 = generic_kernel for every plugin list (A/B and cross-check)
  int batch_kernel = 0;
  // msh_options.pair_planes, where pair_kernel's node planes come from: 0 = auto (LDS-staged for tables
  // up to PAIR_LDS_BIG_GROUPS groups and launches that fill the chip, scalar loads otherwise), 1 = scalar
  // loads into SGPRs, 2 = LDS-staged (tables that fit)
  int pair_planes = 0;
  // msh_options.pair_noax: the LDS-staged form scans group 0 first and drops the non-match / feasible
  // reduction from the scan of the other groups when group 0 has settled it for every lane of the
  // wave (1), or scans group 0 last and never drops it (0). -1 = auto: 1 for REVERSE / MINMAX (78.1
  // against 89.0 us per 32-batch C3 launch), 0 for the identity-like modes (77.3-78.3 against
  // 80.9-81.2), profiles/r4_ab_pair_planes.txt. The identity-like modes no longer carry a feasible
  // reduction in the LDS form (the first feasible node comes from the scalar unit): the option is still
  // accepted and has no effect on them
  int pair_noax = -1;
  // msh_options.pair_fold: the identity-like modes' LDS-staged form in 4-wave workgroups moves a
  // workgroup's class-0 pods (not tolerating, code bit 3 clear) to its first blocks and scans the blocks
  // of class 0 only with X | D3 built on the scalar unit (1, the default: 65.7-68.0 against 71.4-73.2 us
  // per 32-batch C3 launch), or scans every block with the general chain in launch order (0): DESIGN.md §4.2
  int pair_fold = 1;
  // msh_options.seq_split, without a capacity: the per-pair batch kernel with the commit epilogue (auto,
  // 2), the sequential kernel's 64-pod blocks of consecutive pods, one workgroup each (1), or the whole
  // batch in one workgroup, in order (serial, 0)
  int seq_split = 2;
  int seq_pod_waves = 0;  // msh_options.seq_pod_waves: pod waves per pod-block workgroup (1, 2, 4, 8), 0 = auto
  int gen_f53 = 1;    // msh_options.gen_keys: generic_kernel's double keys for 64-bit totals below 2^53 (1) or uint64_t (0)
  int gen_nnkey = 1;  // msh_options.gen_nnkey: generic_kernel's compare-free NodeNumber key (1) or the select (0)
};

// NodeNumber codes: a node's suffix digit 0..9, or CODE_NONE_NODE when its name has no digit
// suffix (and for padding slots); a pod's digit, or CODE_NONE_POD. The two "none" codes differ
// from each other and from every digit, so they never match.
constexpr uint32_t CODE_NONE_NODE = 15u;
constexpr uint32_t CODE_NONE_POD = 14u;

// Bit-sliced node table (the input of every batch / sequential kernel). Node i is bit (i mod 32)
// of word i / 32; words come in groups of PLANE_GW (256 nodes), and a group holds PLANE_N planes
// of PLANE_GW words each, plane-major, so one scalar load brings one plane of a whole group:
//   planes[(g * PLANE_N + k) * PLANE_GW + j] = plane k of word g * PLANE_GW + j
//   k = 0..3  bit k of the node's NodeNumber code (digit 0..9, or 15: no digit / padding)
//   k = 4     X: NodeUnschedulable rejects the node for pods that do not tolerate the
//             unschedulable taint (Spec.Unschedulable with the filter in the list)
//   k = 5     V: the slot holds a real node (i < n), i.e. it is feasible for tolerating pods
// 0.75 B per node. A (pod, node) pair is a feasible digit match exactly when, in the node's bit,
//   (X & ~tol) | (D0 ^ P0) | (D1 ^ P1) | (D2 ^ P2) | (D3 ^ P3) == 0
// with P_k = all-ones when bit k of the pod's code is set.
constexpr int PLANE_GW = 8;
constexpr int PLANE_N = 6;
constexpr int PLANE_X = 4, PLANE_V = 5;
constexpr int GROUP_NODES = PLANE_GW * 32;
constexpr int GROUP_DWORDS = PLANE_GW * PLANE_N;
constexpr int32_t NODE_PAD = 1024;  // tables are padded to whole 1,024-node prep blocks (4 groups)

// ---- launchers (msh_prep.hip, msh_pair.hip, msh_generic.hip, msh_seq.hip) ----
// The bit planes of the whole table from the uploaded columns (n nodes, n_pad slots).
hipError_t launch_node_prep(const uint8_t* d_unsched, const int8_t* d_digit, int32_t n, int32_t n_pad,
                            int32_t has_nu, uint32_t* d_planes, hipStream_t s);
// A rewrite's copy of the published table version (the uploaded columns and the planes, n_words 32-node
// words), with up to PATCH_INLINE msh_patch_nodes entries (idx | unsched << 32 | (uint8)digit << 40)
// applied on the way: the patched words' planes are rebuilt, nothing else is (O(N / 32) threads).
constexpr int PATCH_INLINE = 64;
struct TableCopyArgs {
  const uint8_t* src_unsched;
  const int8_t* src_digit;
  const uint32_t* src_planes;
  uint8_t* dst_unsched;
  int8_t* dst_digit;
  uint32_t* dst_planes;
  int32_t n, n_words, has_nu, count;
  unsigned long long inl[PATCH_INLINE];
};
hipError_t launch_table_copy(const TableCopyArgs& a, hipStream_t s);
// A larger patch: its entries scattered into the copied columns (the full prep re-runs after it).
hipError_t launch_patch_scatter(const unsigned long long* d_entries, int32_t count, uint8_t* d_unsched,
                                int8_t* d_digit, hipStream_t s);

constexpr int64_t EXPORT_NONE = INT64_MIN;  // msh_export_results: no score recorded
hipError_t launch_export(const uint8_t* d_unsched, const int8_t* d_digit, int32_t n,
                         const int8_t* d_pod_digit, const uint8_t* d_pod_tol, int32_t p,
                         const PluginParams& pp, uint8_t* d_filter, int64_t* d_raw, int64_t* d_fin,
                         hipStream_t s);

// One batch of a (multi-batch) launch: its own pod columns and outputs.
struct BatchDesc {
  const int8_t* pod_digit;
  const uint8_t* pod_tol;
  int32_t* out_idx;
  int64_t* out_score;  // may be null
  int32_t* out_status;
  int32_t n_pods;
  int32_t reserved;
};
constexpr int32_t PAIR_FLAG_FOLD = 2;  // PairCommon::noax, identity-like modes: DeviceInfo::pair_fold
constexpr int MULTI_MAX = 32;  // batches per launch (kernel-argument descriptors, 40 B each: ~1.3 KB)

// The per-pair kernel (pair_kernel): nb (1..MULTI_MAX) batches in one launch, or (shard) the
// per-pod shard keys of ONE batch, d[0].
struct PairCommon {
  const uint32_t* planes;  // bit-sliced node table (PLANE_* layout), n_groups groups
  int32_t n_groups;
  int32_t g_full;          // groups [0, g_full) hold real nodes only (no padding slot)
  int32_t gps;             // groups per slice wave (set by the launcher)
  int32_t noax;            // pair_lds_kernel: group 0 may settle the non-match reduction (launcher); the
                           // identity-like instances read PAIR_FLAG_FOLD of it and nothing else
  int32_t nb;
  PluginParams pp;
  int64_t node_base;       // shard mode: global index of local node 0
  int32_t* keys;           // shard mode: [2 * d[0].n_pods] keys (first feasible match, non-match)
  // sequential mode without a capacity (one batch): every placed pod adds 1 to its node's count in
  // replica (64-pod block mod SEQ_COUNT_REPLICAS) of these SEQ_COUNT_REPLICAS arrays; null otherwise
  int32_t* counts;
  int64_t count_stride;
};
// The kernel arguments with room for NB batch descriptors: the host builds PairArgs (MULTI_MAX); a
// one-batch launch passes PairArgsN<1> (136 B of arguments instead of 1,624 B: the argument copy of a
// 1.6 KB block costs ~3-4 us of host time per hipLaunchKernel)
template <int NB>
struct PairArgsN : PairCommon {
  BatchDesc d[NB];
};
using PairArgs = PairArgsN<MULTI_MAX>;
hipError_t launch_pairs(PairArgs& a, bool shard, const DeviceInfo& dev, hipStream_t s);

// MSH_TIEBREAK_RANDOM (msh_tiebreak.hip, pair_pick_kernel): nb (1..MULTI_MAX) batches in one launch; pod j
// of batch b draws at position draw_base[b] + j of the SplitMix64 stream seeded with `seed`.
struct PickArgs {
  const uint32_t* planes;  // bit-sliced node table (PLANE_* layout), n_groups groups
  int32_t n_groups;
  int32_t nb;
  PluginParams pp;
  uint64_t seed;
  BatchDesc d[MULTI_MAX];
  uint64_t draw_base[MULTI_MAX];
};
// The planes are staged in LDS up to this many groups, launch_pairs' limit for pair_lds_kernel
// (PAIR_LDS_BIG_GROUPS, msh_pair.hip: 106,496 nodes, 78 KB per workgroup); larger tables are read from
// global memory.
constexpr int TIEBREAK_LDS_MAX_GROUPS = 416;
hipError_t launch_pair_pick(const PickArgs& a, hipStream_t s);

hipError_t launch_decode_keys(const int8_t* pod_digit, int32_t p, const int32_t* keys, PluginParams pp,
                              int32_t* out_idx, int64_t* out_score, int32_t* out_status, hipStream_t s);

// Device groups (msh_group_*, msh_prep.hip): the merge on the home device over every shard's per-pod
// buffers (peer-mapped pointers, one per shard, List order of the shards).
constexpr int GROUP_MAX = 16;  // MSH_GROUP_MAX_SHARDS
struct GroupPtrs {
  const int32_t* keys[GROUP_MAX];  // shard keys, 2p each (group_keys_decode)
  const int64_t* v[GROUP_MAX];     // extents (group_max_i64) or best totals (group_best_merge)
  const int32_t* idx[GROUP_MAX];   // best global indices (group_best_merge)
  int32_t n;
};
// element-wise MAX of the shards' keys, then decode_pod (msh_decode_keys_device's decode)
hipError_t launch_group_keys_decode(const GroupPtrs& g, const int8_t* pod_digit, int32_t p, PluginParams pp,
                                    int32_t* out_idx, int64_t* out_score, int32_t* out_status, hipStream_t s);
// element-wise MAX of the shards' len int64 (the generic extents: maxima and negated minima)
hipError_t launch_group_max_i64(const GroupPtrs& g, int64_t len, int64_t* out, hipStream_t s);
// per pod: the largest total, then the lowest global index among the shards holding it
hipError_t launch_group_best_merge(const GroupPtrs& g, int32_t p, int64_t* out_total, int32_t* out_idx,
                                   hipStream_t s);

// ---- generic score pipeline (any score plugin list; generic_kernel) ----
constexpr int GEN_MAX_SCORE = 5;  // score plugins per list: NodeNumber + up to four score columns
constexpr int GEN_COLS = 4;       // score-column plugins MSH_PLUGIN_SCORE_COLUMN0..3
struct GenericArgs {
  const uint8_t* unsched;  // the uploaded node columns, List order (n_nodes valid)
  const int8_t* digit;
  const int64_t* cols;     // GEN_COLS x col_stride raw column values, List order
  int64_t col_stride;
  int32_t n_nodes;
  int32_t has_nu;          // NodeUnschedulable in the filter list
  int32_t tile;            // nodes per LDS tile (set by the launcher)
  int32_t slices;          // waves per pod group (set by the launcher)
  int32_t nn_score;        // NodeNumber in the score list
  int32_t nn_prescore;     // NodeNumber in the prescore list (its PreScore state is written)
  int32_t nn_mode;         // NodeNumber's msh_normalize
  int64_t nn_weight;
  int32_t ncol;            // score-column plugins in the list
  // the columns with a normalizer, in list order: column id, list position (among the columns), mode,
  // weight; and the columns without one (their weight x raw is a node-only sum)
  int32_t nnc, ncc[GEN_COLS], npos[GEN_COLS], nmode[GEN_COLS];
  int64_t nw[GEN_COLS];
  int32_t nts, tcc[GEN_COLS];
  int64_t tw[GEN_COLS];
  int32_t need_ext;        // some plugin normalizes: the extent pass runs
  int32_t w64;             // 64-bit totals (the host could not bound every feasible total within 31 bits, or a
                           // normalizing column's weight or normalized score reaches 2^23)
  int32_t f53;             // every feasible |total| below 2^53: 8-byte keys as doubles (exact integers)
  int32_t nn24;            // NodeNumber's two weighted values differ by less than 2^24 (32-bit keys: no compare)
  int32_t nb;              // batches (mode 0: up to MULTI_MAX; sharded modes: 1)
  int64_t node_base;       // sharded modes: global index of local node 0
  int64_t* ext;            // mode 1: out, mode 2: in; [2 (1 + ncol)][p] per-pod extents, mins negated
  int64_t* best_total;     // mode 2 out: per pod, the shard's best total (INT64_MIN: no feasible node)
  int32_t* best_idx;       // mode 2 out: its global node index (INT32_MAX: none)
  BatchDesc d[MULTI_MAX];
};
// mode 0: schedule nb batches; 1: per-pod extents over this shard; 2: per-pod best over this shard.
hipError_t launch_generic(GenericArgs& a, int mode, const DeviceInfo& dev, hipStream_t s);
hipError_t launch_generic_candidates(int32_t p, const int64_t* local_total, const int64_t* merged_total, int32_t* idx,
                                     hipStream_t s);
hipError_t launch_generic_decode(const int8_t* pod_digit, int32_t p, const int64_t* best_total, const int32_t* best_idx,
                                 int32_t nn_score, int32_t nn_prescore, int32_t* out_idx, int64_t* out_score,
                                 int32_t* out_status, hipStream_t s);

struct SeqArgs {
  const uint32_t* planes;    // bit-sliced node table (PLANE_* layout)
  int32_t n_words;           // n_pad / 32
  int32_t n_nodes;
  const int8_t* pod_digit;
  const uint8_t* pod_tol;
  int32_t n_pods;
  PluginParams pp;
  int32_t max_pods;
  // per-node assigned pods, count_replicas arrays of count_stride: a node's count is its sum over the
  // replicas (pod blocks add to replica blockIdx % SEQ_COUNT_REPLICAS); read at start, updated
  int32_t* counts;
  int64_t count_stride;
  int32_t count_replicas;    // 1, or SEQ_COUNT_REPLICAS (pod blocks need them all)
  int32_t fold;              // one workgroup: first fold replicas 1.. into replica 0 (some hold counts)
  int32_t* out_idx;
  int64_t* out_score;
  int32_t* out_status;
  int32_t pods_per_block;    // set by the launcher: pods per workgroup (the whole batch when one workgroup)
  // per-node capacities (msh_upload_node_capacity), n_words * 32 entries with the padding slots 0, or null:
  // node i takes pods while its count is below min(cap[i], max_pods); max_pods is INT32_MAX when the call
  // gives no scalar capacity. Wave-uniform: the launchers pick the per-node kernel instances by it.
  const int32_t* cap;
};

// No-capacity sequential launches (pair_kernel's commit epilogue, seq_kernel's pod blocks) add their
// commits to one of this many count replicas: a digit's pods all land on its first feasible match, and
// device atomics from every wave onto one address queue. Per C5 launch (pair_kernel<4, .., true>,
// profiles/ab/r6_seq_pair_replicas.txt): 16 replicas 15.5 us, 64 8.5 us, 256 8.5 us (6.99 without the
// epilogue). Tables up to SEQ_SPLIT_MAX_NODES only, so larger ones keep one count array.
constexpr int SEQ_COUNT_REPLICAS = 64;
constexpr int32_t SEQ_SPLIT_MAX_NODES = 4 * 64 * 4 * 32;  // four scanning waves x 64 lanes x 4 words
// Workgroups launch_sequential runs the batch on: 64-pod blocks without a capacity on tables whose
// counts fit LDS (DeviceInfo::seq_split), else 1.
int32_t seq_blocks(const SeqArgs& a, const DeviceInfo& dev);
// counts[i] (replica 0) = the node's sum over the replicas, the others zeroed, for i < n
hipError_t launch_count_fold(int32_t* counts, int64_t stride, int32_t replicas, int32_t n, hipStream_t s);

hipError_t launch_sequential(const SeqArgs& a, const DeviceInfo& dev, hipStream_t s, std::string* err);
// The capacity form (msh_seq_cap.hip): nw scanning waves with rs words per lane, one workgroup.
hipError_t launch_seq_capacity(const SeqArgs& a, int nw, int rs, hipStream_t s);
// The resource-fit form (msh_seq_fit.hip, msh_schedule_sequential_fit): the capacity form's in-order loop with
// per-node int64 free amounts. s.max_pods is INT32_MAX when neither a scalar nor a capacity column limits the
// pod count; s.fold as for the other one-workgroup forms.
constexpr int FIT_MAX_RES = 4;  // MSH_MAX_RESOURCES
struct FitArgs {
  SeqArgs s;
  int32_t nres;            // 1..FIT_MAX_RES
  int64_t res_stride;      // entries between two resources' rows of alloc / used (>= s.n_words * 32, padding 0)
  const int64_t* alloc;    // [nres][res_stride]
  int64_t* used;           // [nres][res_stride]: read at the start, written back at the end
  const int64_t* pod_req;  // [nres][s.n_pods]
};
// What a call past a register-resident form's table limit is refused with (the launchers and the host checks):
// form is "resource-fit", "scored resource-fit", "topology-spread", "scored topology-spread", "class-mask" or
// "scored class-mask", limit its seq_*_max_nodes(nres).
inline std::string seq_table_limit_message(const char* form, int32_t limit, int32_t nres) {
  return std::string("the ") + form + " form keeps the node state in registers: at most " + std::to_string(limit) +
         " nodes per device with " + std::to_string(nres) + (nres == 1 ? " resource" : " resources");
}
// Nodes the resource-fit kernel holds for a table of nres resources (8,192 up to two, 4,096 for three or four).
int32_t seq_fit_max_nodes(int32_t nres);
hipError_t launch_seq_fit(const FitArgs& a, hipStream_t s, std::string* err);
// The scored resource-fit form (msh_seq_score.hip; msh_set_resource_score with a mode other than NONE): the same
// loop, with upstream's NodeResourcesLeastAllocated / MostAllocated score of every feasible node added to the
// NodeNumber total, so each pod is a true arg-max over the table. Every amount must be <= 2^55 (checked on the host).
struct FitScoreArgs {
  FitArgs f;
  int32_t most;             // 0: LeastAllocated, 1: MostAllocated
  int64_t weight;           // the plugin weight, [1, 2^32]
  int32_t rw[FIT_MAX_RES];  // resource weights in [0, 100], 0 for a resource that is not scored and for r >= f.nres
  uint32_t wsum_magic;      // ceil(2^31 / sum of rw): x / sum = (x * magic) >> 31 exactly for x <= 100 * sum
};
int32_t seq_score_max_nodes(int32_t nres);
hipError_t launch_seq_score(const FitScoreArgs& a, hipStream_t s, std::string* err);
// The topology-spread form (msh_seq_spread.hip, msh_schedule_sequential_spread): the resource-fit loop with
// upstream's PodTopologySpread filter. f.nres may be 0 (no table: alloc, used and pod_req are not read).
constexpr int SPREAD_ZONES = 64;        // MSH_MAX_ZONES
constexpr int SPREAD_MAX_GROUPS = 128;  // MSH_MAX_SPREAD_GROUPS
struct SpreadArgs {
  FitArgs f;
  const int32_t* zone;       // [f.s.n_words * 32]: the node's zone id in [0, SPREAD_ZONES), -1 without one (padding too)
  const int32_t* pod_group;  // [f.s.n_pods]: any value outside [0, n_groups) is an ungrouped pod
  int32_t n_groups;          // 0..SPREAD_MAX_GROUPS
  const int32_t* max_skew;   // [n_groups], each >= 1
  int32_t* cnt;              // [n_groups][SPREAD_ZONES]: read at the start, written back at the end
  uint64_t zset;             // bit z: zone z occurs on a node of the table
};
// Nodes the topology-spread kernel holds for a table of nres resources (0..FIT_MAX_RES): the resource-fit limits.
int32_t seq_spread_max_nodes(int32_t nres);
hipError_t launch_seq_spread(const SpreadArgs& a, hipStream_t s, std::string* err);
// The scored topology-spread form (msh_seq_spread_score.hip, msh_schedule_sequential_spread_scored on a ctx whose
// resource score mode is not NONE): the topology-spread feasible set with the scored resource-fit form's totals.
// s.f.nres is 1..FIT_MAX_RES; every amount must be <= 2^55 (checked on the host).
struct SpreadScoreArgs {
  SpreadArgs s;
  int32_t most;             // as FitScoreArgs
  int64_t weight;
  int32_t rw[FIT_MAX_RES];
  uint32_t wsum_magic;
};
// Nodes the scored topology-spread kernel holds for a table of nres resources: the scored resource-fit limits.
int32_t seq_spread_score_max_nodes(int32_t nres);
hipError_t launch_seq_spread_score(const SpreadScoreArgs& a, hipStream_t s, std::string* err);
// The class forms (msh_seq_classes.hip, msh_schedule_sequential_classes): the topology-spread form (scored: the
// scored topology-spread form, ss's setting; else ss.most, weight, rw and wsum_magic are not read) with the
// per-class node mask as one more conjunct. ss.s.zone may be null (no node has a zone) and ss.s.pod_group may be
// null (every pod ungrouped; n_groups is then 0).
constexpr int CLASS_MAX = 64;  // MSH_MAX_POD_CLASSES
struct ClassArgs {
  SpreadScoreArgs ss;
  const uint64_t* class_bits;  // [ss.s.f.s.n_words * 32]: bit c: the node admits pods of class c (padding 0), or null
  const int32_t* pod_class;    // [ss.s.f.s.n_pods]: any value outside [0, n_classes) is a pod without a class, or null
  int32_t n_classes;           // 0..CLASS_MAX
};
// Nodes the class kernels hold: the topology-spread limits unscored, the scored topology-spread limits scored.
int32_t seq_classes_max_nodes(int32_t nres, bool scored);
hipError_t launch_seq_classes(const ClassArgs& a, bool scored, hipStream_t s, std::string* err);
// The preference form (msh_seq_prefs.hip, msh_schedule_sequential_prefs with a nonzero preference weight): the
// scored class form's feasible set and totals plus w_aff * na + w_taint * nt, the normalised preferred node affinity
// and PreferNoSchedule scores, both normalised per pod over its feasible nodes. The class conjunct comes from
// `admit`, not from a column of words. Resource score mode NONE: ss.weight 0, ss.rw all 0, ss.wsum_magic 0, and
// ss.s.f.nres may be 0. 100 * (ss.weight + w_aff + w_taint) must be <= 65,534 (the packed key; checked on the host).
constexpr int PREF_THREADS = 1024;  // the records of a class in the device table: one per thread of the largest instance
struct PrefArgs {
  SpreadScoreArgs ss;
  // [n_classes][PREF_THREADS] records of 2 * npl dwords, npl = seq_prefs_npl(ss.s.f.nres): record t holds
  // A | T << 16 of nodes t * npl .. t * npl + npl - 1, then their admit bits in one dword (bit k: node t * npl + k
  // admits the class), then padding; slots past the table 0. 16-byte aligned, or null (no pod has a class)
  const uint32_t* rows;
  const int32_t* pod_class;  // [ss.s.f.s.n_pods]: any value outside [0, n_classes) is a pod without a class, or null
  int32_t n_classes;         // 0..CLASS_MAX
  uint64_t amask, tmask;     // bit c: class c has a nonzero A / T on some node
  uint32_t w_aff, w_taint;   // the weights, [0, 100]
};
// Nodes the preference kernel holds: the scored limits in every resource score mode; and its nodes per thread.
int32_t seq_prefs_max_nodes(int32_t nres);
int32_t seq_prefs_npl(int32_t nres);
hipError_t launch_seq_prefs(const PrefArgs& a, hipStream_t s, std::string* err);
// The soft-spread form (msh_seq_soft.hip, msh_schedule_sequential_soft on a ctx with a SCHEDULE_ANYWAY group): the
// preference form, except that a pod of a soft group passes no spread filter and every feasible node with a zone
// gets w_spread * ns added, ns upstream's normalised PodTopologySpread score over the zones of the pod's feasible
// nodes. 100 * (p.ss.weight + p.w_aff + p.w_taint + w_spread) must be <= 65,534, every count of a soft group during
// the call <= 2 * SPREAD_SOFT_MAX and every soft group's max_skew <= SPREAD_SOFT_MAX (checked on the host).
constexpr int32_t SPREAD_SOFT_MAX = 1 << 24;  // MSH_SPREAD_SOFT_MAX
struct SoftArgs {
  PrefArgs p;
  uint64_t soft[SPREAD_MAX_GROUPS / 64];  // bit g: group g is SCHEDULE_ANYWAY
  uint32_t w_spread;                      // the weight, [0, 100]
  const double* zone_weight;              // [SPREAD_ZONES + 1]: log(size + 2), the host's std::log (device memory)
};
// Nodes the soft-spread kernel holds: the preference kernel's.
int32_t seq_soft_max_nodes(int32_t nres);
int32_t seq_soft_npl(int32_t nres);
hipError_t launch_seq_soft(const SoftArgs& a, hipStream_t s, std::string* err);
// The balanced-allocation form (msh_seq_balanced.hip, msh_schedule_sequential_balanced with a nonzero w_balanced):
// the soft-spread form with w_balanced * BS added to every feasible node's total, BS upstream's
// NodeResourcesBalancedAllocation score of the table's first two resources, evaluated in IEEE double. so.soft may be
// all zero (no SCHEDULE_ANYWAY group; so.zone_weight may then be null). so.p.ss.s.f.nres is 2..FIT_MAX_RES,
// 100 * (so.p.ss.weight + so.p.w_aff + so.p.w_taint + so.w_spread + w_balanced) must be <= 65,534 and every amount
// <= 2^55 in every resource score mode (checked on the host).
struct BalancedArgs {
  SoftArgs so;
  uint32_t w_balanced;  // the weight, [1, 100]
};
// Nodes the balanced-allocation kernel holds: the soft-spread kernel's.
int32_t seq_balanced_max_nodes(int32_t nres);
int32_t seq_balanced_npl(int32_t nres);
hipError_t launch_seq_balanced(const BalancedArgs& a, hipStream_t s, std::string* err);
// The inter-pod affinity form (msh_seq_podaffinity.hip, msh_schedule_sequential_podaffinity with a profile column):
// the balanced-allocation form with the required InterPodAffinity filter as one more conjunct of the feasible set.
// ba.w_balanced may be 0 (ba.so.p.ss.s.f.nres is then 0..FIT_MAX_RES and the amounts' bound applies only with a
// resource score). The static and dynamic LDS together must not pass PODAFF_LDS_MAX (checked on the host).
constexpr int PODAFF_MAX_TERMS = 32;     // MSH_MAX_AFFINITY_TERMS
constexpr int PODAFF_MAX_PROFILES = 64;  // MSH_MAX_POD_PROFILES
constexpr size_t PODAFF_LDS_MAX = 65536;
struct PodAffinityArgs {
  BalancedArgs ba;
  uint2* state;               // [n_words * 32] (present, repel): read at the start, written back at the end
  const int32_t* pod_profile; // [n_pods]: any value outside [0, n_profiles) is a pod without a profile, or null
  const uint4* profiles;      // [n_profiles] (match, anti, 1 << aff or 0, unused)
  int32_t n_profiles;         // 0..PODAFF_MAX_PROFILES
  uint32_t host_mask, zone_mask;  // the terms whose topology is the node / the zone
};
// Nodes the kernel holds and its nodes per thread: the balanced-allocation kernel's.
int32_t seq_podaffinity_max_nodes(int32_t nres);
int32_t seq_podaffinity_npl(int32_t nres);
// The LDS bytes of a launch on a table of n_nodes with nres resources and n_groups spread groups in the call, static
// and dynamic together; *per_group (optional): what one more group adds.
size_t seq_podaffinity_lds(int32_t nres, int32_t n_nodes, int32_t n_groups, size_t* per_group);
hipError_t launch_seq_podaffinity(const PodAffinityArgs& a, hipStream_t s, std::string* err);
// alloc / used [r * stride + idx[k]] = v[r * count + k] for the non-null arrays (device-visible memory)
hipError_t launch_res_patch(const int32_t* idx, const int64_t* alloc, const int64_t* used, int32_t count, int32_t nres,
                            int64_t stride, int64_t* d_alloc, int64_t* d_used, hipStream_t s);
// Pod waves per pod-block workgroup without a capacity (one scanning wave): each walks 64 / this many pods.
constexpr int SEQ_POD_WAVES = 1;  // measured: 1 / 2 / 4 / 8 waves 11.6 / 14.2 / 13.2 / 18.3 us per C5 launch (profiles/ab/r6_seq_pod_waves.jsonl)
int seq_pod_waves(const DeviceInfo& dev);

// Launch timing (msh_timing_begin / _end): the next hot-kernel launch on this thread (batch, multi-
// batch, generic, sequential kernels) records `start` / `stop` at the kernel's own start and end.
void set_launch_events(hipEvent_t start, hipEvent_t stop);
bool launch_events_pending();

}  // namespace msh
