// msh_ctx.h — the msh_ctx behind include/minisched_hip.h and the host helpers its translation units
// share (msh_capi.cpp: single-device entry points; msh_capi_seq.cpp: the grouped sequential-commit entry points
// and the columns they read; msh_shard.cpp: node-sharded merge, RCCL communicator and device groups). Not part
// of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/minisched_hip.h"
#include "msh_internal.h"
#include "msh_seq_quot.h"

// One version of the node-side device tables (List order, padded to cap nodes).
struct NodeTable {
  size_t cap = 0;
  uint8_t* d_unsched = nullptr;  // the uploaded columns (read by generic_kernel and the export as they are)
  int8_t* d_digit = nullptr;
  uint32_t* d_planes = nullptr;  // bit-sliced node table (msh_internal.h PLANE_* layout): pair / seq kernels
  // score-column plugins (generic pipeline): GEN_COLS x cap int64, column k valid when col_ok[k], with the
  // range of its values (host side: the generic launch bounds the totals from it)
  int64_t* d_cols = nullptr;
  bool col_ok[msh::GEN_COLS] = {};
  int64_t col_lo[msh::GEN_COLS] = {}, col_hi[msh::GEN_COLS] = {};
  // launches that read this version: one event per caller stream, re-recorded after each launch
  std::vector<std::pair<hipStream_t, hipEvent_t>> readers;
};

// The merge buffers of the node-sharded entry points (msh_schedule_nodeshard_device), per ctx: the
// shard keys (2p int32), or the generic form's extents, totals and indices, grown on demand.
struct ShardScratch {
  size_t pods = 0, ext = 0;   // capacities: pods, extent entries
  int32_t* keys = nullptr;    // 2 x pods
  int64_t* ext_buf = nullptr; // ext
  int64_t* total = nullptr;   // pods: this shard's best totals
  int64_t* merged = nullptr;  // pods: the merged maximum
  int32_t* idx = nullptr;     // pods: best global index (merged by MIN)
  // the last node-sharded launch (its stream and completion event): the next one on another stream waits
  // for it, a reallocation waits for it on the host
  hipStream_t last_stream = nullptr;
  hipEvent_t last_ev = nullptr;
  bool in_flight = false;
};

struct msh_ctx {
  int device = 0;
  std::string err;
  msh::DeviceInfo dev;
  hipStream_t stream = nullptr;  // used by the synchronous host-buffer entry points

  // plugin descriptor
  std::vector<int32_t> filter_ids, prescore_ids, score_ids, normalize;
  std::vector<int64_t> weights;
  msh::PluginParams pp{1, 1, 1, 0, 1};
  // tie-break among the maximum totals (msh_set_tiebreak): the mode, and in RANDOM mode the seed and
  // the position of the next batch's first draw (advanced by p at each batch submission)
  int32_t tiebreak_mode = MSH_TIEBREAK_FIRST;
  uint64_t tie_seed = 0, tie_counter = 0;

  // node table: two versions. Launches read tab[cur]; a rewrite (upload, patch, plugin change,
  // score column) builds the other version on prep_stream and then publishes it, so it never waits
  // for launches in flight on the version they read (only for those of two rewrites ago, on the
  // version it overwrites, long done in practice).
  bool have_nodes = false;
  int32_t n_nodes = 0, n_pad = 0;
  NodeTable tab[2];
  int cur = 0;
  // sequential-mode state (not versioned: carried from call to call): pods committed per node, and
  // the sequential launches in flight that update it
  // (counts_replicas arrays of counts_cap: msh::SEQ_COUNT_REPLICAS for tables pod blocks can take, else
  // 1; counts_dirty: replicas 1.. may hold counts, folded into replica 0 by the next one-workgroup
  // launch or count read)
  int32_t* d_counts = nullptr;
  size_t counts_cap = 0;
  int32_t counts_replicas = 1;
  bool counts_dirty = false;
  // the capacity column (msh_upload_node_capacity): cap_cap int32 on the device (the padding slots 0) and
  // its host copy (n_nodes entries, what msh_node_capacity returns); dropped by msh_upload_nodes
  int32_t* d_cap = nullptr;
  size_t cap_cap = 0;
  bool have_cap = false;
  std::vector<int32_t> h_cap;
  // the resource table (msh_upload_node_resources): nres rows of res_cap int64 each for alloc and for used
  // (row r at r * res_cap, the padding slots 0), on the device only: used changes with every commit of
  // msh_schedule_sequential_fit, so msh_node_resources reads both back; dropped by msh_upload_nodes
  int64_t* d_alloc = nullptr;
  int64_t* d_used = nullptr;
  size_t res_cap = 0;
  int32_t res_rows = 0;  // rows allocated (>= nres)
  int32_t nres = 0;
  bool have_res = false;
  // the resource score of msh_schedule_sequential_fit (msh_set_resource_score; policy, like the plugin lists: it
  // outlives tables): mode, plugin weight, the resources it was set for and their weights. res_max: the largest
  // amount any upload or patch has written into the table since the last msh_upload_node_resources (the table
  // itself is on the device only), which bounds every alloc and used whatever was committed since: a scored
  // call needs it within MSH_RESOURCE_SCORE_MAX
  int32_t rs_mode = MSH_RESOURCE_SCORE_NONE;
  int64_t rs_weight = 1;
  int32_t rs_nres = 0;
  int32_t rs_w[MSH_MAX_RESOURCES] = {};
  int64_t res_max = 0;
  // topology spread (msh_schedule_sequential_spread), unversioned like the counts. The zone column
  // (msh_upload_node_zones): zone_cap int32 on the device (-1 in the padding slots), its host copy and Zset, the
  // ids that occur on a node; dropped by msh_upload_nodes. The groups (msh_set_spread_groups): sp_groups of them
  // with their max_skew on the host and in d_skew. The counts cnt[g][z], on the device only (every spread commit
  // changes them): d_skew and d_spread_cnt are allocated whole (MSH_MAX_SPREAD_GROUPS rows) at first use.
  int32_t* d_zone = nullptr;
  size_t zone_cap = 0;
  bool have_zone = false;
  std::vector<int32_t> h_zone;
  uint64_t zset = 0;
  int32_t sp_groups = 0;
  std::vector<int32_t> h_skew;
  int32_t* d_skew = nullptr;
  int32_t* d_spread_cnt = nullptr;
  // soft topology spread (msh_schedule_sequential_soft): each group's mode (sp_groups of them, host only: a launch
  // takes the soft groups as two words of kernel argument), how many are SCHEDULE_ANYWAY, the score's weight, and
  // sp_cnt_bound, an upper bound of every count cnt[g][z]: the largest value a patch wrote since the counts were last
  // zeroed plus the pods submitted to grouped calls since then. d_zone_weight: the 65 values log(size + 2) on the
  // device, uploaded by the first soft launch.
  std::vector<uint8_t> h_spmode;
  int32_t sp_soft = 0;
  int32_t w_spread = 0;
  int64_t sp_cnt_bound = 0;
  double* d_zone_weight = nullptr;
  // NodeResourcesBalancedAllocation (msh_schedule_sequential_balanced): the plugin weight, 0 = the call is _soft
  int32_t w_balanced = 0;
  // the per-class node masks (msh_upload_node_class_bits), unversioned like the capacity column: class_cap uint64
  // on the device (the padding slots 0), the host copy (n_nodes words, what msh_node_class_bits returns) and the
  // number of classes C the column was uploaded for; dropped by msh_upload_nodes. Only
  // msh_schedule_sequential_classes reads it.
  uint64_t* d_class = nullptr;
  size_t class_cap = 0;
  bool have_class = false;
  int32_t n_classes = 0;
  std::vector<uint64_t> h_class;
  // the per-class preference values (msh_upload_node_class_prefs): the host copies, [pref_classes][n_nodes] each (what
  // msh_node_class_prefs returns), and the weights of msh_set_preference_weights; dropped by msh_upload_nodes. The
  // device table that msh_schedule_sequential_prefs reads is derived from them and from the class masks (rows A | T
  // << 16 of pref_stride dwords, then the admit bits, pref_dev_classes classes) and rebuilt by the first call after
  // either column changed (pref_dirty); pref_amask / pref_tmask: the classes with a nonzero A / T on some node.
  bool have_prefs = false;
  int32_t pref_classes = 0;
  std::vector<uint16_t> h_pref_a, h_pref_t;
  int32_t w_aff = 0, w_taint = 0;
  uint32_t* d_pref = nullptr;
  size_t pref_cap = 0;  // dwords
  bool pref_dirty = true;
  int32_t pref_dev_classes = 0;
  int64_t pref_stride = 0;
  uint64_t pref_amask = 0, pref_tmask = 0;
  // required inter-pod affinity (msh_schedule_sequential_podaffinity): the terms' topologies and their masks, the
  // pod profiles on the host and as the kernel's records in d_pa_prof (MSH_MAX_POD_PROFILES of them, allocated at
  // first use), and the state, (present, repel) per node, on the device only (every commit changes it): pa_cap pairs,
  // valid when pa_have_state, else all zero and written as such by the next reader or writer (pa_state_ready).
  // msh_upload_nodes and msh_set_pod_affinity_terms zero the state by dropping the flag; nothing else does.
  int32_t pa_terms = 0;
  std::vector<uint8_t> h_pa_topo;
  uint32_t pa_host_mask = 0, pa_zone_mask = 0;
  int32_t pa_profiles = 0;
  std::vector<uint32_t> h_pa_match, h_pa_anti;
  std::vector<int32_t> h_pa_aff;
  uint4* d_pa_prof = nullptr;
  uint2* d_pa_state = nullptr;
  size_t pa_cap = 0;
  bool pa_have_state = false;
  // per caller stream, the event of its last sequential launch: an alias of a table version's reader
  // event (not owned here; track_launch)
  std::vector<std::pair<hipStream_t, hipEvent_t>> seq_inflight;
  // the rewrites' own stream, created with the device's highest priority: HIP gives each priority
  // its own hardware queues, so a rewrite never queues behind other streams' kernels that happen to
  // share a hardware queue with it (GPU_MAX_HW_QUEUES per priority)
  hipStream_t prep_stream = nullptr;
  bool generic = false;  // the score list names a score-column plugin

  // host-path buffers
  size_t pod_cap = 0;
  int8_t* d_pd = nullptr;         // device scratch for the pod columns
  uint8_t* d_pt = nullptr;
  size_t stage_cap = 0;
  unsigned char* h_stage = nullptr;  // page-locked: digit p | tol p | idx 4p | score 8p | status 4p
  // msh_schedule_batch_async: a ring of MSH_ASYNC_DEPTH events on the ctx's stream; ticket t's event
  // is async_ev[t % MSH_ASYNC_DEPTH]; every ticket <= async_done has completed
  hipEvent_t async_ev[MSH_ASYNC_DEPTH] = {};
  uint64_t async_issued = 0, async_done = 0;
  size_t patch_cap = 0;
  unsigned long long* d_patch = nullptr;  // msh_patch_nodes entries
  std::vector<unsigned long long> h_patch;
  // page-locked staging of node columns / patch entries (uploads copy from it, never from pageable
  // memory: a pageable copy may wait for more than this ctx's stream)
  size_t nstage_cap = 0;
  unsigned char* h_nstage = nullptr;
  // msh_timing_begin / _end: kernel start / stop event pairs for the next hot-kernel launches
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;
  size_t t_next = 0;

  // node-sharded mode (msh_shard.cpp): the RCCL communicator (ncclComm_t; null: a world of one) and
  // the merge buffers
  void* comm = nullptr;
  int32_t comm_world = 0, comm_rank = 0;
  ShardScratch shard;
};

namespace msh::capi {

int fail(msh_ctx* c, int code, const std::string& msg);
int hip_fail(msh_ctx* c, hipError_t e, const char* what);

#define MSH_HIP(ctx, call)                                          \
  do {                                                              \
    hipError_t e_ = (call);                                         \
    if (e_ != hipSuccess) return ::msh::capi::hip_fail(ctx, e_, #call); \
  } while (0)

NodeTable& cur_table(msh_ctx* c);
// Launch-path check: the tables are always published ready (rewrites are synchronous).
int ready(msh_ctx* c);
// After a launch on caller stream s that reads the current table version (seq: and updates the
// sequential-mode counts).
int track_launch(msh_ctx* c, hipStream_t s, bool seq = false);
// pair_kernel's arguments for the current table (the batches are filled in by the caller).
msh::PairArgs pair_args(msh_ctx* c);
// generic_kernel's arguments for the current table and plugin list (MSH_ERR_STATE: a column missing).
int generic_args(msh_ctx* c, msh::GenericArgs& g);
// The generic pipeline runs the batch entry points when the score list names a score column (or for
// every list with msh_options.batch_kernel = 1).
bool use_generic(const msh_ctx* c);
// MSH_OK in MSH_TIEBREAK_FIRST mode; in RANDOM mode MSH_ERR_UNSUPPORTED with a message naming `entry`, an
// entry point the random tie-break does not cover (checked before any device work).
int refuse_random(msh_ctx* c, const char* entry);

// One hot-kernel launch under msh_timing_begin: arms the next event pair for the launcher on this
// thread; a launcher that launched nothing leaves it unused.
struct TimedLaunch {
  msh_ctx* c;
  bool armed = false;
  explicit TimedLaunch(msh_ctx* ctx);
  ~TimedLaunch();
};

// The ctx's device current for the call, the caller's restored after it (no switch at all in the
// common case of a caller already on that device).
struct DeviceGuard {
  int prev = -1, want;
  explicit DeviceGuard(int d) : want(d) {
    if (hipGetDevice(&prev) != hipSuccess || prev != d) (void)hipSetDevice(d);
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
  }
};

// Host-buffer I/O of one synchronous call: pod columns and outputs in page-locked host memory, read
// and written by the kernel; then, for a pageable caller, outputs copied from the stage into the
// caller's arrays.
struct HostIO {
  int8_t* d_pd = nullptr;
  uint8_t* d_pt = nullptr;
  int32_t* o_idx = nullptr;    // what the kernel writes (device-visible)
  int64_t* o_score = nullptr;
  int32_t* o_status = nullptr;
  int32_t* h_idx = nullptr;    // page-locked destination: the caller's arrays or the stage
  int64_t* h_score = nullptr;
  int32_t* h_status = nullptr;
  bool staged = false;
};
int host_io_begin(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol, int32_t* out_idx,
                  int64_t* out_score, int32_t* out_status, HostIO& io);
int host_io_end(msh_ctx* c, int32_t p, int32_t* out_idx, int64_t* out_score, int32_t* out_status, const HostIO& io);

// Device-visible address of page-locked host memory (msh_host_alloc'd or registered), or nullptr.
void* pinned_device_ptr(const void* p);

// Host wait for the launches recorded in `evs` (their events are kept for reuse).
void wait_events(const std::vector<std::pair<hipStream_t, hipEvent_t>>& evs);
// Order prep_stream after the sequential launches in flight (device-side waits): they update the counts and
// columns that a read, reset or re-upload touches next.
int after_seq(msh_ctx* c);
// The page-locked node staging buffer, at least `bytes` long (free on entry: every user finishes its copies).
int node_stage(msh_ctx* c, size_t bytes);

// What every sequential-commit call shares (seq_device / seq_host in msh_capi.cpp, the grouped forms in
// msh_capi_seq.cpp).
// The table, pod column, count, capacity and output fields of a.s for the ctx as it stands; max_pods and fold are
// the caller's (the plain call's rules differ from the one-workgroup forms').
void seq_args_fill(msh_ctx* c, msh::SeqArgs& a, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                   int32_t* d_out_idx, int64_t* d_out_score, int32_t* d_out_status);
// The ctx's resource score setting (mode LEAST or MOST) for a scored launch with nres resources: A is
// msh::FitScoreArgs or msh::SpreadScoreArgs, which carry the same four fields.
template <class A>
void resource_score_setting(const msh_ctx* c, int32_t nres, A& a) {
  a.most = c->rs_mode == MSH_RESOURCE_SCORE_MOST_ALLOCATED ? 1 : 0;
  a.weight = c->rs_weight;
  uint32_t sum = 0;
  for (int32_t r = 0; r < msh::FIT_MAX_RES; ++r) sum += (uint32_t)(a.rw[r] = r < nres ? c->rs_w[r] : 0);
  a.wsum_magic = msh::wsum_magic(sum);
}
// The requests of a host call, [nres][p]: each within [0, 2^62]; with a resource score (scored), then with the
// balanced score, within 2^55.
int check_requests(msh_ctx* c, int32_t nres, int32_t p, const int64_t* pod_req, bool scored, bool balanced);
// One sequential launch of a ctx at a time: each commits into (and a fold rewrites) the same counts, so stream s
// first waits for the ctx's sequential launches in flight on other streams.
int seq_serialize(msh_ctx* c, hipStream_t s);
// The commit callback for every placed pod of a finished host call, in pod order.
void commit_callbacks(msh_commit_cb cb, void* user, int32_t p, const int32_t* out_idx, const int64_t* out_score,
                      const int32_t* out_status);

}  // namespace msh::capi

// msh_shard.cpp: releases the ctx's communicator and merge buffers (msh_destroy).
void msh_shard_release(msh_ctx* c);
