/*
 * minisched_hip.h — C-ABI of libminisched_hip.so, the MI355X (gfx950) scheduling core.
 *
 * This is the drop-in boundary for the reference's per-pod hot path
 * (shopetan/mini-kube-scheduler, Go, k8s v1.22.0):
 *
 *   minisched/minisched.go:32-87   Scheduler.scheduleOne (selection part)
 *   minisched/minisched.go:115-151 RunFilterPlugins   -> feasibility stage
 *   minisched/minisched.go:153-162 RunPreScorePlugins -> per-pod prescore (pod digit)
 *   minisched/minisched.go:164-199 RunScorePlugins    -> score + normalize + sum stage
 *   minisched/minisched.go:304-325 selectHost         -> argmax stage (first max, see below)
 *   minisched/plugins/score/nodenumber/nodenumber.go:50-100  NodeNumber PreScore/Score
 *   k8s.io/kubernetes@v1.22.0 .../nodeunschedulable Filter (wired minisched/initialize.go:193-202)
 *
 * The reference evaluates ONE pod against a freshly LISTed []v1.Node per cycle.
 * Here a whole batch of pods is evaluated against a device-resident node table.
 * A cgo binding replaces scheduleOne's :40-80 segment for a batch
 * drained from activeQ; Permit/Bind stay per pod on the host.
 *
 * Conventions
 *  - Every function returns an int: MSH_OK (0) or a negative msh_err code.
 *    Per-pod outcomes are NOT errors: they go to out_status (MSH_PLACED /
 *    MSH_FIT_ERROR / MSH_SCORE_ERROR), mirroring minisched.go:50-80 + ErrorFunc :283-298.
 *  - Host pointers are caller-owned; the library copies them in/out and keeps
 *    no pointer past the call. "_device" entry points take device pointers and a
 *    hipStream_t passed as void* (NULL = the null stream) and are asynchronous.
 *  - A ctx is bound to one device and is not thread-safe; every entry point
 *    calls hipSetDevice(ctx->device) first (cgo calls land on arbitrary OS threads).
 *  - Node tables are in the reference's LIST order: byte-wise sorted node names
 *    (etcd key order, minisched.go:40). msh_pack_nodes produces that order.
 *  - Tie-break: the reference's selectHost reservoir-samples ties with math/rand
 *    (minisched.go:316-321), so every node with the maximum total is equally likely. A ctx has
 *    two modes (msh_set_tiebreak). MSH_TIEBREAK_FIRST, the default, is deterministic: the
 *    LOWEST node index among the maximum total score (first max in List order).
 *    MSH_TIEBREAK_RANDOM picks uniformly among the maxima from a seeded, counter-based draw:
 *    the same distribution as the reservoir scan, reproducible from (seed, counter). It is not
 *    the same stream as Go's global math/rand, which depends on the process's whole call
 *    history and cannot be reproduced without Go.
 */
#ifndef MINISCHED_HIP_H
#define MINISCHED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSH_ABI_VERSION 8

/* ---- error codes (return values) ---- */
typedef enum msh_err {
  MSH_OK = 0,
  MSH_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, bad plugin id, ...) */
  MSH_ERR_NO_DEVICE = -2,   /* no HIP device / bad device ordinal */
  MSH_ERR_HIP = -3,         /* a HIP runtime call failed (message in msh_last_error) */
  MSH_ERR_STATE = -4,       /* call order: e.g. schedule before msh_upload_nodes */
  MSH_ERR_UNSUPPORTED = -5, /* plugin combination / size the device path does not implement */
  MSH_ERR_NOMEM = -6
} msh_err;

/* ---- per-pod outcome (out_status) ---- */
typedef enum msh_status {
  MSH_PLACED = 0,      /* selectHost returned a node (minisched.go:80-87) */
  MSH_FIT_ERROR = 1,   /* no feasible node: *framework.FitError (minisched.go:143-148) */
  MSH_SCORE_ERROR = 2  /* a Score plugin failed (minisched.go:70-75); e.g. NodeNumber with
                          no PreScore state (nodenumber.go:74-77) */
} msh_status;

/* ---- device plugin ids (framework.Plugin.Name() -> id) ---- */
typedef enum msh_plugin_id {
  MSH_PLUGIN_NODE_UNSCHEDULABLE = 1, /* "NodeUnschedulable" (Filter) */
  MSH_PLUGIN_NODE_NUMBER = 2,        /* "NodeNumber" (PreScore, Score) */
  /* Score-column plugins (ABI v5, build extension): a score plugin whose Score(pod, node) is an
   * int64 the host computed per node (msh_upload_score_column), e.g. a node-only scorer evaluated
   * once per snapshot. Score lists with one of these run on the generic pipeline (an explicit
   * int64 score per pair, per-plugin NormalizeScore over the feasible list, weights, first max):
   * the batch entry points and the node-sharded msh_generic_* entry points (shard keys, sequential
   * mode and the export: MSH_ERR_UNSUPPORTED). */
  MSH_PLUGIN_SCORE_COLUMN0 = 16,
  MSH_PLUGIN_SCORE_COLUMN1 = 17,
  MSH_PLUGIN_SCORE_COLUMN2 = 18,
  MSH_PLUGIN_SCORE_COLUMN3 = 19
} msh_plugin_id;

/* ---- per-score-plugin normalize stage ----
 * NONE reproduces the reference (NodeNumber.ScoreExtensions() == nil, nodenumber.go:98-100).
 * The others are build extensions (parity unpinned by the reference), applied once per
 * pod over the feasible list (upstream framework order: Score -> NormalizeScore -> weight):
 *   DEFAULT         upstream helper.DefaultNormalizeScore(MaxNodeScore=100, reverse=false)
 *   DEFAULT_REVERSE upstream helper.DefaultNormalizeScore(MaxNodeScore=100, reverse=true)
 *   MINMAX          100*(s-min)/(max-min) over the feasible list; 0 when max==min           */
typedef enum msh_normalize {
  MSH_NORMALIZE_NONE = 0,
  MSH_NORMALIZE_DEFAULT = 1,
  MSH_NORMALIZE_DEFAULT_REVERSE = 2,
  MSH_NORMALIZE_MINMAX = 3
} msh_normalize;

typedef struct msh_ctx msh_ctx;

/* Library ABI version (MSH_ABI_VERSION). */
int msh_abi_version(void);

/* Number of visible HIP devices (0 on a machine without a GPU). */
int msh_device_count(int* out_count);

/* Page-locked host memory (hipHostMalloc) for the host-buffer entry points' pod columns and
 * outputs. With buffers from here (or registered with HIP) msh_schedule_batch / _sequential copy
 * nothing on the host and issue no DMA: the kernel reads the pod columns from these buffers and
 * writes idx / score / status straight into them over PCIe (zero-copy). Pageable buffers work too;
 * they are staged through a page-locked buffer of the ctx. A cgo caller allocates its batch buffers
 * here once and reuses them. msh_host_free(NULL) is a no-op. */
int msh_host_alloc(size_t bytes, void** out_ptr);
void msh_host_free(void* ptr);

/* Create/destroy a context on `device`. Default plugin set = the reference's
 * (initialize.go:80-123): filter=[NodeUnschedulable], prescore=[NodeNumber],
 * score=[NodeNumber] weight 1, normalize NONE. msh_create picks every kernel automatically; the
 * library reads no environment variable. msh_destroy first waits for the launches this ctx queued
 * with the *_device entry points (they read the ctx's tables), not for the rest of the device. */
int msh_create(int device, msh_ctx** out_ctx);
void msh_destroy(msh_ctx* ctx);

/* Kernel-selection overrides (ABI v8), for parity tests and A/B measurement only: a scheduler calls
 * msh_create. Every field's 0 is the automatic choice, so a zeroed struct (with struct_size set) is
 * msh_create. A value outside a field's set is MSH_ERR_INVALID (message in msh_last_error(NULL)).
 * Results never depend on the options; only which kernel instance computes them does. */
typedef struct msh_options {
  int32_t struct_size;  /* sizeof(msh_options) */
  int32_t batch_kernel; /* 0 auto | 1 generic_kernel (explicit int64 score per pair) for every plugin list */
  int32_t pair_planes;  /* 0 auto | 1 node planes by scalar loads | 2 staged in LDS (tables that fit) */
  int32_t pair_noax;    /* 0 auto | 1 LDS form: group 0 first, settled reductions dropped | 2 group 0 last
                         * (REVERSE / MINMAX; NONE / DEFAULT have no such reduction: accepted, no effect) */
  int32_t pair_slices;  /* 0 auto | 1, 2, 4 slice waves per 64-pod block (and generic_kernel pod group) */
  int32_t seq_waves;    /* 0 auto | 1, 4, 15, 16 scanning waves of the sequential kernel (raised when too few) */
  int32_t seq_split;    /* 0 auto (no capacity: the batch kernel + counts) | 1 one workgroup walks the
                           whole batch | 2 64-pod blocks of consecutive pods, one workgroup each */
  int32_t seq_pod_waves; /* 0 auto | 1, 2, 4, 8 waves sharing a 64-pod block (one scanning wave, no capacity) */
  int32_t gen_keys;     /* 0 auto (64-bit totals below 2^53 as double keys) | 1 uint64 keys */
  int32_t gen_nnkey;    /* 0 auto (compare-free NodeNumber key) | 1 compare + select */
  int32_t pair_fold;    /* 0 auto (LDS form, NONE / DEFAULT, 4-wave workgroups: non-tolerating pods of digits 0-7
                         * first, their blocks scanned with X | D3 from the scalar unit) | 1 off: every block
                         * takes the general chain, in launch order */
} msh_options;
int msh_create_ex(int device, const msh_options* opts, msh_ctx** out_ctx);

/* Message for the last failing call on this ctx ("" if none). Valid until the next call. With a
 * NULL ctx: the message of the last failed msh_create on the calling thread. */
const char* msh_last_error(const msh_ctx* ctx);

/* Plugin lists (Scheduler.filterPlugins / preScorePlugins / scorePlugins,
 * minisched/initialize.go:25-27). Ids must be unique within a list (the reference keys
 * score maps by plugin Name(), minisched.go:173, so duplicates collapse; rejected here).
 * weights[i] in [1, 2^32]; "TODO: plugin weight" (minisched.go:187): weight 1 == reference.
 * msh_set_plugins: prescore list = the score plugins that implement PreScore. */
int msh_set_plugins(msh_ctx* ctx, const int32_t* filter_ids, int32_t nf,
                    const int32_t* score_ids, const int64_t* weights, int32_t ns);
int msh_set_plugins_ex(msh_ctx* ctx, const int32_t* filter_ids, int32_t nf,
                       const int32_t* prescore_ids, int32_t npre,
                       const int32_t* score_ids, const int64_t* weights,
                       const int32_t* normalize, int32_t ns);

/* ---- tie-break among the maximum totals (added after v8, additive) ----
 * MSH_TIEBREAK_FIRST: the first maximum in List order (the default; what every earlier version does).
 * MSH_TIEBREAK_RANDOM, for a pod whose status is MSH_PLACED:
 *   tie set  T = the feasible nodes whose total equals the pod's maximum total, in List order, c = |T|;
 *   choice   the pod goes to the k-th node of T (0-based), k = (u * c) >> 32 in 64 bits (c < 2^24);
 *   draw     u = the high 32 bits of SplitMix64 at position `counter`:
 *              z = seed + (counter + 1) * 0x9E3779B97F4A7C15      (mod 2^64)
 *              z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *              z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *              z =  z ^ (z >> 31);   u = z >> 32
 *   counter  pod j of a call draws at base + j, base = the ctx's draw counter when the call is
 *            submitted (async and _device calls included); the call then advances the counter by p,
 *            whatever the pods' statuses. In msh_schedule_batches_device batch i starts where batch
 *            i - 1 ended.
 * out_score and out_status are exactly FIRST mode's: the tie-break only chooses among equal totals. The
 * choice is uniform over T up to a bias below c / 2^32.
 * msh_get_tiebreak returns the live counter: a caller checkpoints (seed, counter) and replays a batch,
 * or gives a pod-sharded rank counter = the index of its first pod, and that rank places its slice
 * exactly as one GPU would place it within the whole batch.
 * RANDOM is honoured by msh_schedule_batch, msh_schedule_batch_async, msh_schedule_batch_device and
 * msh_schedule_batches_device, for every plugin list without a score column (with or without the
 * NodeUnschedulable filter, NodeNumber in or out of the prescore and score lists, every normalize mode,
 * every weight). While the ctx is in RANDOM mode these return MSH_ERR_UNSUPPORTED (the message names
 * the entry point), do no device work and leave the counter alone: msh_schedule_sequential and
 * msh_schedule_sequential_device; msh_shard_keys_device, msh_decode_keys_device and the
 * msh_generic_*_device entry points; msh_schedule_nodeshard and msh_schedule_nodeshard_device;
 * msh_group_schedule_batch when any shard is in RANDOM mode; a batch whose score list names a score
 * column; and every batch of a ctx created with msh_options.batch_kernel = 1.
 * msh_set_tiebreak: a mode outside the enum is MSH_ERR_INVALID. */
typedef enum msh_tiebreak { MSH_TIEBREAK_FIRST = 0, MSH_TIEBREAK_RANDOM = 1 } msh_tiebreak;
int msh_set_tiebreak(msh_ctx* ctx, int32_t mode, uint64_t seed, uint64_t counter);
int msh_get_tiebreak(const msh_ctx* ctx, int32_t* out_mode, uint64_t* out_seed, uint64_t* out_counter);

/* Node table in List order (name-sorted). unsched[i] = node.Spec.Unschedulable (0/1);
 * digit[i] = last byte of node.Name as '0'..'9' -> 0..9, else -1 (nodenumber.go:81-87).
 * 0 <= n < 2^24. Replaces the per-cycle Nodes().List (minisched.go:40). */
int msh_upload_nodes(msh_ctx* ctx, int32_t n, const uint8_t* unsched, const int8_t* digit);
int msh_num_nodes(const msh_ctx* ctx, int32_t* out_n);

/* The per-node scores of score-column plugin `plugin_id` (MSH_PLUGIN_SCORE_COLUMN0..3), n = the
 * uploaded node count, List order, each in [-2^31, 2^31]. An msh_upload_nodes drops every column
 * (its nodes are gone); a batch whose score list names a column not uploaded since is
 * MSH_ERR_STATE. Totals are Go int64 arithmetic: weight x normalized score summed with wrap-around. */
int msh_upload_score_column(msh_ctx* ctx, int32_t plugin_id, int32_t n, const int64_t* scores);

/* Per-pair plugin results for a small batch: the matrices the simulator's result store
 * turns into pod annotations (scheduler/plugin/resultstore/store.go:170-234, recorded by the
 * wrapped plugins in scheduler/plugin/plugins.go:278-325). Row j, column i (List order):
 *   out_filter[j*n+i] = 1 if node i passes the filter plugins for pod j ("passed"), else 0;
 *   out_score[j*n+i]  = NodeNumber.Score raw value (AddScoreResult);
 *   out_final[j*n+i]  = NormalizeScore(raw) * weight (AddNormalizedScoreResult ->
 *                       applyWeightOnScore, store.go:231-234);
 * score/final = MSH_EXPORT_NONE (INT64_MIN) where no score is recorded (node filtered out, or
 * the pod never reaches Score). Host buffers; p*n <= 2^28. Debug path, not the hot path. */
#define MSH_EXPORT_NONE ((int64_t)(-9223372036854775807LL - 1))
int msh_export_results(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                       uint8_t* out_filter, int64_t* out_score, int64_t* out_final);

/* In-place update of `count` entries of the uploaded table (an informer Update event that
 * leaves the List order alone, e.g. a cordon flipping Spec.Unschedulable; eventhandler.go:45-50).
 * idx[k] in [0, n) and pairwise distinct; unsched[k] / digit[k] as in msh_upload_nodes.
 * O(count) host->device traffic; the per-node pod counts of sequential mode are kept.
 * Adds and deletes shift List positions: re-upload with msh_upload_nodes. */
int msh_patch_nodes(msh_ctx* ctx, int32_t count, const int32_t* idx, const uint8_t* unsched,
                    const int8_t* digit);

/* Batched hot path: p pods against the uploaded node table.
 * pod_digit[j] = last byte of pod.Name as digit or -1 (nodenumber.go:50-55);
 * pod_tol[j]   = pod tolerates taint {node.kubernetes.io/unschedulable, NoSchedule} (0/1).
 * Outputs per pod: out_idx (node index, -1 unless PLACED), out_score (total int64 score of
 * the selected node, 0 unless PLACED), out_status (msh_status). Synchronous. Host buffers:
 * page-locked ones (msh_host_alloc) take the zero-copy path, pageable ones are staged.
 * out_score may be NULL, here and in every entry point below that takes one (ABI v4): the scores
 * are then not written, 8 of the 16 output bytes per pod (a binding that only places pods, as
 * scheduleOne does after selectHost, needs the node and the status). */
int msh_schedule_batch(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                       int32_t* out_idx, int64_t* out_score, int32_t* out_status);

/* Asynchronous host-buffer batch (ABI v5): msh_schedule_batch for page-locked buffers (msh_host_alloc
 * or registered with HIP; pageable ones are MSH_ERR_INVALID) that returns once the batch is launched.
 * The kernel reads the pod columns and writes the outputs over PCIe as in the synchronous call; they
 * are valid once msh_wait(ctx, ticket) returns MSH_OK. A caller packs batch i + 1 (msh_pack_pods)
 * while batch i runs, the pipeline a cgo caller draining activeQ batch after batch (minisched.go:28-34)
 * runs. Batches of one ctx complete in submission order; at most MSH_ASYNC_DEPTH are in flight (a
 * further submission first waits for the oldest). The caller must not touch a batch's buffers before
 * its msh_wait. Tickets are positive and increase by one per call. */
#define MSH_ASYNC_DEPTH 4
int msh_schedule_batch_async(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                             int32_t* out_idx, int64_t* out_score, int32_t* out_status, uint64_t* out_ticket);
/* Wait for batch `ticket` (and every earlier one) of msh_schedule_batch_async. A ticket the ctx
 * never handed out is MSH_ERR_INVALID; an already completed one returns at once. */
int msh_wait(msh_ctx* ctx, uint64_t ticket);

/* Same, device-resident inputs/outputs, asynchronous on `stream` (hipStream_t).
 * Launches on different streams may overlap (independent batches pipelined): each needs its own
 * pod and output buffers. The node table is double-buffered: an upload, patch, score-column upload or
 * filter-list change rebuilds the version no launch reads, on the ctx's own high-priority stream,
 * and publishes it before the call returns (the rebuild is synchronous; launches made after it read
 * the new version, launches already queued keep reading the old one). The ctx records an event on
 * `stream` after each launch; a rebuild waits on the host only for the launches of two rebuilds ago,
 * which read the version it overwrites, and never for other ctxs' or the caller's other work. */
int msh_schedule_batch_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                              const uint8_t* d_pod_tol, int32_t* d_out_idx,
                              int64_t* d_out_score, int32_t* d_out_status, void* stream);

/* Several independent batches in one submission (ABI v5): what a caller draining a deep activeQ
 * (minisched.go:28-34, one scheduleOne per pod) hands over when it has more than one batch ready,
 * e.g. consecutive next_batch drains. batches[i] describes batch i exactly as the arguments of
 * msh_schedule_batch_device (device pointers, out_score may be NULL); the descriptor array itself
 * is host memory, read during the call. Up to MSH_BATCHES_PER_LAUNCH batches share one kernel
 * launch (a larger nb takes ceil(nb / MSH_BATCHES_PER_LAUNCH) launches, in order, on `stream`),
 * which spreads the launch cost and the kernel's fill and drain over them. Results are identical to
 * nb msh_schedule_batch_device calls. Asynchronous, like msh_schedule_batch_device. */
#define MSH_BATCHES_PER_LAUNCH 32
typedef struct msh_batch {
  int32_t p;
  int32_t reserved; /* 0 */
  const int8_t* pod_digit;
  const uint8_t* pod_tol;
  int32_t* out_idx;
  int64_t* out_score;
  int32_t* out_status;
} msh_batch;
int msh_schedule_batches_device(msh_ctx* ctx, int32_t nb, const msh_batch* batches, void* stream);

/* Sequential-commit mode (one pod at a time, node state committed between placements).
 * The node table stays in the registers of a workgroup: up to 368,640 nodes without a capacity,
 * 262,144 with one (larger tables: MSH_ERR_UNSUPPORTED).
 * The commit increments the selected node's assigned-pod count on the device (the
 * NodeInfo.AddPod analogue). max_pods_per_node > 0 additionally makes a node infeasible
 * once it holds that many pods (build extension): one workgroup walks the whole batch. 0 =
 * reference semantics, where no commit feeds a later decision and the placements equal
 * msh_schedule_batch's: tables up to 32,768 nodes then run on the per-pair batch kernel, whose waves
 * add their placed pods to the counts (a no-capacity shortcut: the pods are not decided in order, exact
 * because the counts are the same in any order). msh_options.seq_split = 2 runs 64-pod blocks of
 * consecutive pods instead, one workgroup each, concurrently, the pods within a block in order; = 1
 * walks the whole batch in one workgroup, in order, as a capacity does.
 * `commit_cb` (may be NULL) is replayed on the host after the device run, in
 * placement order, once per PLACED pod. The counts carry over from call to call; sequential launches
 * of one ctx on different streams are ordered by the library (each waits for the ones in flight). */
typedef void (*msh_commit_cb)(void* user, int32_t pod, int32_t node_idx, int64_t score);
int msh_schedule_sequential(msh_ctx* ctx, int32_t p, const int8_t* pod_digit,
                            const uint8_t* pod_tol, int32_t max_pods_per_node,
                            int32_t* out_idx, int64_t* out_score, int32_t* out_status,
                            msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                                   const uint8_t* d_pod_tol, int32_t max_pods_per_node,
                                   int32_t* d_out_idx, int64_t* d_out_score,
                                   int32_t* d_out_status, void* stream);
/* Per-node assigned-pod counts accumulated by the sequential commits (n entries). */
int msh_node_pod_counts(msh_ctx* ctx, int32_t* out_counts);
int msh_reset_node_pod_counts(msh_ctx* ctx);

/* Per-node pod capacity for sequential-commit mode (a node's status.allocatable.pods; additive in ABI 8).
 * The column. A ctx may hold a capacity column cap[i], one int32 per uploaded node, in List order,
 *   0 <= cap[i] <= INT32_MAX. Node i is infeasible for every pod while count[i] >= cap[i], where count[i]
 *   is the assigned-pod count sequential mode already keeps. cap[i] = 0 means the node never takes a pod.
 *   INT32_MAX is in effect unlimited; there is no sentinel.
 * Effective capacity. With a column present, msh_schedule_sequential and msh_schedule_sequential_device
 *   use eff[i] = cap[i] when max_pods_per_node == 0, and eff[i] = min(cap[i], max_pods_per_node) when it
 *   is positive. They always run the in-order capacity form: one workgroup walks the whole batch, exactly
 *   as a positive max_pods_per_node does. Statuses, scores and the first-maximum tie-break are those of
 *   the existing capacity mode: a pod whose class has no available node is MSH_FIT_ERROR, and a pod that
 *   ends in MSH_SCORE_ERROR commits nothing.
 * No column. Without a column every call behaves exactly as before, kernel instance included.
 * Lifetime. msh_upload_nodes drops the column, as it drops score columns, because its nodes are gone.
 *   msh_patch_nodes and msh_reset_node_pod_counts keep it. Counts carry over from call to call. A patch
 *   that lowers cap[i] to or below count[i] makes the node full for the next call; raising it makes the
 *   node available again.
 * Batch entry points ignore the column: they make no commit.
 * Limits. The table limit of the capacity form, 262,144 nodes, applies as soon as a column is present
 *   (larger tables: MSH_ERR_UNSUPPORTED). MSH_TIEBREAK_RANDOM and score-column lists stay refused in
 *   sequential mode.
 * Both writers are synchronous and ordered after the ctx's sequential launches in flight; neither rebuilds
 * the node table.
 * msh_upload_node_capacity: n != the uploaded node count, or a negative entry: MSH_ERR_INVALID; before
 *   msh_upload_nodes: MSH_ERR_STATE.
 * msh_patch_node_capacity: cap[k] replaces the capacity of node idx[k]; idx in [0, n), pairwise distinct
 *   (MSH_ERR_INVALID otherwise, as a negative entry); no column: MSH_ERR_STATE.
 * msh_clear_node_capacity: back to "no column".
 * msh_node_capacity: *out_present = 1 and the n capacities in out_cap (may be NULL) with a column, else
 *   *out_present = 0 and out_cap untouched. */
int msh_upload_node_capacity(msh_ctx* ctx, int32_t n, const int32_t* cap);
int msh_patch_node_capacity(msh_ctx* ctx, int32_t count, const int32_t* idx, const int32_t* cap);
int msh_clear_node_capacity(msh_ctx* ctx);
int msh_node_capacity(const msh_ctx* ctx, int32_t* out_cap, int32_t* out_present);

/* Resource requests for sequential-commit mode (upstream's NodeResourcesFit as a build extension, in the same
 * sense as the pod capacity; additive in ABI 8).
 * The table. A ctx may hold a resource table of nres resources, 1 <= nres <= MSH_MAX_RESOURCES. Per uploaded
 *   node i and resource r it holds two int64: alloc[r][i], the node's allocatable amount, and used[r][i], the
 *   sum of the committed requests (NodeInfo.Requested), both in [0, MSH_RESOURCE_MAX] = [0, 2^62]. Arrays are
 *   resource-major, a[r * n + i], in List order. Units are the caller's (milli-cpu, bytes, ...).
 * msh_schedule_sequential_fit / _fit_device: the in-order loop of the capacity form with one more conjunct in
 *   feasibility. Pods are decided strictly in order; pod j carries requests req[r][j] (pod_req[r * p + j], each
 *   in [0, 2^62]). Node i is feasible for pod j iff the filter list passes (unchanged), count[i] < eff[i] (eff
 *   as msh_schedule_sequential uses it, from max_pods_per_node and / or the capacity column; with neither there
 *   is no count limit), and for every r with req[r][j] > 0: req[r][j] <= alloc[r][i] - used[r][i]. So a zero
 *   request never rejects, even where a patch has lowered alloc below used, and an exact fit passes. Status,
 *   score and the first-maximum tie-break over the feasible set are the capacity form's: MSH_FIT_ERROR when no
 *   node is feasible, otherwise MSH_SCORE_ERROR (which commits nothing), otherwise MSH_PLACED, whose commit
 *   adds 1 to count[sel] and req[r][j] to used[r][sel] for every r. used and the counts carry over from call to
 *   call, across a mix of _fit and plain sequential calls too.
 * The device form is asynchronous, as msh_schedule_sequential_device, and does not validate d_pod_req: values
 *   outside [0, 2^62] are the caller's error (the host form returns MSH_ERR_INVALID for them).
 * Refusals: no resource table: MSH_ERR_STATE; nres != the table's: MSH_ERR_INVALID; MSH_TIEBREAK_RANDOM and a
 *   score-column list: MSH_ERR_UNSUPPORTED, as in sequential mode; a table past the kernel's limit:
 *   MSH_ERR_UNSUPPORTED. The limit: the node state lives in the registers of one workgroup, 8,192 nodes for a
 *   table of one or two resources, 4,096 for three or four.
 * Unchanged calls. msh_schedule_sequential* and every batch entry point ignore the table: their pods request
 *   nothing and commit nothing to used. With no table every existing call behaves as before, kernel instance
 *   included.
 * Lifetime and ordering are the capacity column's: msh_upload_nodes drops the table; msh_patch_nodes and
 *   msh_reset_node_pod_counts keep it and do not touch used (used changes only through commits, an upload or a
 *   patch). The writers and the reader are synchronous, ordered after the ctx's sequential launches in flight,
 *   and do not rebuild the node table. A patch of used is how a caller accounts for a deleted pod, or for pods
 *   bound before the scheduler started.
 * msh_upload_node_resources: used NULL = zeros. n != the uploaded node count, nres outside
 *   1..MSH_MAX_RESOURCES, a value outside [0, 2^62]: MSH_ERR_INVALID; before msh_upload_nodes: MSH_ERR_STATE.
 * msh_patch_node_resources: alloc[r * count + k] / used[r * count + k] replace node idx[k]'s values (NULL: keep
 *   that array); idx in [0, n), pairwise distinct, values in range, not both arrays NULL (MSH_ERR_INVALID
 *   otherwise); no table: MSH_ERR_STATE.
 * msh_clear_node_resources: back to "no table".
 * msh_node_resources: *out_present = 1, *out_nres (may be NULL) and the nres * n values in out_alloc / out_used
 *   (each may be NULL) with a table; else *out_present = 0 and the arrays untouched.
 * A failed call changes nothing. */
#define MSH_MAX_RESOURCES 4
#define MSH_RESOURCE_MAX ((int64_t)1 << 62)
int msh_upload_node_resources(msh_ctx* ctx, int32_t n, int32_t nres, const int64_t* alloc, const int64_t* used);
int msh_patch_node_resources(msh_ctx* ctx, int32_t count, const int32_t* idx, const int64_t* alloc,
                             const int64_t* used);
int msh_clear_node_resources(msh_ctx* ctx);
int msh_node_resources(msh_ctx* ctx, int32_t* out_nres, int64_t* out_alloc, int64_t* out_used,
                       int32_t* out_present);
int msh_schedule_sequential_fit(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                int32_t nres, const int64_t* pod_req, int32_t max_pods_per_node,
                                int32_t* out_idx, int64_t* out_score, int32_t* out_status,
                                msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_fit_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                                       const uint8_t* d_pod_tol, int32_t nres, const int64_t* d_pod_req,
                                       int32_t max_pods_per_node, int32_t* d_out_idx, int64_t* d_out_score,
                                       int32_t* d_out_status, void* stream);

/* Resource-aware scoring for msh_schedule_sequential_fit / _fit_device (upstream's NodeResourcesLeastAllocated,
 * noderesources/least_allocated.go, in the v1.22 default profile, and NodeResourcesMostAllocated,
 * most_allocated.go, as a build extension in the same sense as the resource table; additive in ABI 8).
 * The setting. msh_set_resource_score(ctx, mode, weight, nres, res_weights): mode NONE (the default: every call
 *   behaves as without this section, kernel instance included; the other arguments are not read and may be 0 /
 *   NULL), LEAST_ALLOCATED (spread: emptier nodes score higher) or MOST_ALLOCATED (pack). weight is the plugin
 *   weight, in [1, 2^32] as a score weight of msh_set_plugins; nres in 1..MSH_MAX_RESOURCES; res_weights[r] in
 *   [0, 100] with at least one positive. A resource of weight 0 is fitted but not scored (upstream's default
 *   scores cpu and memory only). Anything else: MSH_ERR_INVALID. The setting is policy, like the plugin lists: it
 *   survives msh_upload_nodes, msh_clear_node_resources and every patch. msh_get_resource_score returns it (every
 *   out pointer may be NULL; out_res_weights takes MSH_MAX_RESOURCES values, 0 past nres).
 * Semantics with a mode other than NONE, for pod j in order:
 *   The feasible set and the status are exactly msh_schedule_sequential_fit's: MSH_FIT_ERROR with no feasible
 *   node, otherwise MSH_SCORE_ERROR when NodeNumber scores without its PreScore state (commits nothing), otherwise
 *   MSH_PLACED. For a feasible node i, total(i) = T(i) + weight * RS(j, i), where T(i) is the total the ctx's
 *   plugin lists give it in msh_schedule_sequential_fit (NodeNumber at its weight, in every normalize mode over the
 *   feasible list; 0 with an empty score list) and, in Go int64 arithmetic (division truncates; every operand is
 *   non-negative), with q_r = used[r][i] + req[r][j] (used before this pod's commit: upstream's
 *   calculateResourceAllocatableRequest adds the pod's request) and c_r = alloc[r][i]:
 *     LEAST: s_r = (c_r == 0 || q_r > c_r) ? 0 : ((c_r - q_r) * 100) / c_r
 *     MOST:  s_r = (c_r == 0 || q_r > c_r) ? 0 : (q_r * 100) / c_r
 *     RS = (sum_r s_r * res_weights[r]) / (sum_r res_weights[r]), over the r of positive weight.
 *   q_r > c_r happens for a zero request on a node whose alloc a patch lowered below used. The pod goes to the first
 *   maximum of total in List order; out_score and commit_cb get that total; the commit is unchanged.
 *   The library substitutes no "non-zero request" defaults: a caller that wants upstream's 100 milli-cpu / 200 MiB
 *   for a pod that requests nothing puts them into pod_req.
 * Range. (c - q) * 100 must stay inside int64, so a scored call needs every amount within
 *   MSH_RESOURCE_SCORE_MAX = 2^55. The table is on the device only, so the ctx keeps the largest value any upload or
 *   patch has written since the last msh_upload_node_resources; commits cannot exceed it (a positive request is
 *   placed only where used + req <= alloc). While that bound is above the limit a scored call returns
 *   MSH_ERR_UNSUPPORTED (the message names the limit). The host form returns MSH_ERR_INVALID for a request above
 *   the limit; the device form does not validate, as before.
 * Refusals of a scored call: nres of the setting != the table's: MSH_ERR_STATE; no table: MSH_ERR_STATE;
 *   MSH_TIEBREAK_RANDOM and score-column lists: MSH_ERR_UNSUPPORTED; a table past the scored form's node limit:
 *   MSH_ERR_UNSUPPORTED with the limit in the message. A node also keeps its allocatable amounts in registers, so
 *   the scored limit is half the unscored one: 4,096 nodes for one or two resources, 2,048 for three or four.
 *   msh_seq_fit_max_nodes reports the limit for a table of nres resources, unscored (scored = 0: 8,192 / 4,096)
 *   or scored (scored != 0).
 * Everything else ignores the setting, as it ignores the table: msh_schedule_sequential*, every batch, shard,
 *   group and export entry point.
 * A failed call changes nothing. */
typedef enum msh_resource_score {
  MSH_RESOURCE_SCORE_NONE = 0, /* default: every call behaves as without a resource score */
  MSH_RESOURCE_SCORE_LEAST_ALLOCATED = 1,
  MSH_RESOURCE_SCORE_MOST_ALLOCATED = 2
} msh_resource_score;
#define MSH_RESOURCE_SCORE_MAX ((int64_t)1 << 55)
int msh_set_resource_score(msh_ctx* ctx, int32_t mode, int64_t weight, int32_t nres, const int32_t* res_weights);
int msh_get_resource_score(const msh_ctx* ctx, int32_t* out_mode, int64_t* out_weight, int32_t* out_nres,
                           int32_t* out_res_weights);
int msh_seq_fit_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t scored, int32_t* out_max_nodes);

/* Pod topology spread for sequential-commit mode (upstream's PodTopologySpread filter with whenUnsatisfiable:
 * DoNotSchedule, in the v1.22 default profile, as a build extension in the same sense as the resource table;
 * additive in ABI 8). It is the one constraint here in which a commit changes the verdict of many nodes at once:
 * every node of the chosen zone and, through the minimum, every node of every zone.
 * The zone column. zone[i], one int32 per uploaded node in List order: a zone id in [0, MSH_MAX_ZONES), or -1 for a
 *   node that lacks the topology key. Zset is the set of ids that occur on at least one node. It is fixed by the
 *   upload: it does not depend on cordons, capacities or free resources (upstream's minimum runs over domains, not
 *   over feasible nodes).
 * Spread groups. G groups, 0 <= G <= MSH_MAX_SPREAD_GROUPS, each with max_skew[g] in [1, INT32_MAX]. A group is one
 *   (selector, constraint) pair: a pod of group g both matches the selector and carries the constraint (the
 *   Deployment case, upstream's selfMatchNum = 1).
 * Spread counts. cnt[g][z], int32: the committed pods of group g on nodes of zone z. Ctx state like the pod counts
 *   and used: unversioned, carried from call to call.
 * msh_schedule_sequential_spread / _spread_device: msh_schedule_sequential_fit with one more per-pod input,
 *   pod_group[j] in [-1, G). Pods are decided strictly in order. For a pod of group -1 everything is exactly
 *   _fit's. For a pod of group g >= 0 node i is feasible iff it is feasible for _fit (filter list, count[i] <
 *   eff[i], requests), zone[i] >= 0, and cnt[g][zone[i]] + 1 - minc(g) <= max_skew[g], where minc(g) is the minimum
 *   of cnt[g][z] over the z of Zset. With Zset empty no node is feasible for a grouped pod. Status, score, the
 *   first-maximum tie-break over the feasible set and the commit are _fit's; a MSH_PLACED pod of group g >= 0 also
 *   adds 1 to cnt[g][zone[sel]]. MSH_FIT_ERROR and MSH_SCORE_ERROR commit nothing.
 * The resource table is optional here: nres = 0 (pod_req may be NULL) checks and commits no requests, with or
 *   without a table on the ctx; nres > 0 behaves as in _fit and must equal the table's.
 * Everything else ignores zones, groups and spread counts: msh_schedule_sequential*, _fit*, and every batch, shard,
 *   group and export entry point make no spread commit and apply no spread check.
 * Refusals of a spread call. No zone column: MSH_ERR_STATE (as no node table, and no resource table with nres > 0).
 *   Host form: a group outside [-1, G) (so any group >= 0 with G = 0), a request outside [0, 2^62]:
 *   MSH_ERR_INVALID. MSH_TIEBREAK_RANDOM, a score-column list, a resource score other than NONE:
 *   MSH_ERR_UNSUPPORTED with a message that names the reason (scoring together with spread is not implemented). This
 *   refusal of a scored ctx stays: msh_schedule_sequential_spread_scored (below) is the call that takes one. A
 *   table past the limit: MSH_ERR_UNSUPPORTED with the limit in the message. The limits are _fit's: 8,192 nodes
 *   for up to two resources, 4,096 for three or four; msh_seq_spread_max_nodes reports them for nres in 0..4.
 * The device form is asynchronous, as msh_schedule_sequential_fit_device, and validates neither d_pod_req nor
 *   d_pod_group: the kernel treats every group value outside [0, G) as -1, an ungrouped pod.
 * Lifetime. msh_upload_nodes drops the zone column and zeroes the spread counts (the groups, policy like the plugin
 *   lists, stay). msh_upload_node_zones replaces the column and zeroes the counts: a node's zone changed under its
 *   pods. msh_set_spread_groups replaces G and max_skew and zeroes the counts when G changes; with the same G it
 *   only updates the skews. msh_patch_nodes, msh_reset_node_pod_counts and the capacity and resource writers keep
 *   all of it. The writers and readers are synchronous, ordered after the ctx's sequential launches in flight, and
 *   do not rebuild the node table.
 * msh_upload_node_zones: n != the uploaded node count, a value outside [-1, MSH_MAX_ZONES): MSH_ERR_INVALID; before
 *   msh_upload_nodes: MSH_ERR_STATE. msh_clear_node_zones: back to "no column" (the counts stay until the next
 *   upload). msh_node_zones: *out_present and, with a column, its n values in out_zone (may be NULL).
 * msh_set_spread_groups: G outside [0, MSH_MAX_SPREAD_GROUPS], a skew below 1: MSH_ERR_INVALID.
 *   msh_get_spread_groups: *out_G and the G skews (each pointer may be NULL).
 * msh_spread_counts: the G * MSH_MAX_ZONES counts, out_cnt[g * MSH_MAX_ZONES + z] (nothing is written with G = 0).
 * msh_patch_spread_counts: value[k] replaces cnt[g[k]][z[k]]: how a caller accounts for a deleted pod, or for pods
 *   bound before the scheduler started. g in [0, G), z in [0, MSH_MAX_ZONES), value >= 0, the (g, z) pairs pairwise
 *   distinct (MSH_ERR_INVALID otherwise). msh_reset_spread_counts: every count to 0.
 * A failed call changes nothing. */
#define MSH_MAX_ZONES 64
#define MSH_MAX_SPREAD_GROUPS 128
int msh_upload_node_zones(msh_ctx* ctx, int32_t n, const int32_t* zone);
int msh_clear_node_zones(msh_ctx* ctx);
int msh_node_zones(const msh_ctx* ctx, int32_t* out_zone, int32_t* out_present);
int msh_set_spread_groups(msh_ctx* ctx, int32_t G, const int32_t* max_skew);
int msh_get_spread_groups(const msh_ctx* ctx, int32_t* out_G, int32_t* out_max_skew);
int msh_spread_counts(msh_ctx* ctx, int32_t* out_cnt);
int msh_patch_spread_counts(msh_ctx* ctx, int32_t count, const int32_t* g, const int32_t* z, const int32_t* value);
int msh_reset_spread_counts(msh_ctx* ctx);
int msh_seq_spread_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t* out_max_nodes);
int msh_schedule_sequential_spread(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                   const int32_t* pod_group, int32_t nres, const int64_t* pod_req,
                                   int32_t max_pods_per_node, int32_t* out_idx, int64_t* out_score,
                                   int32_t* out_status, msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_spread_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                                          const uint8_t* d_pod_tol, const int32_t* d_pod_group, int32_t nres,
                                          const int64_t* d_pod_req, int32_t max_pods_per_node, int32_t* d_out_idx,
                                          int64_t* d_out_score, int32_t* d_out_status, void* stream);

/* Topology spread together with a resource score (upstream's v1.22 default profile on one pod: NodeResourcesFit as
 * a filter, NodeResourcesLeastAllocated as a score, PodTopologySpread as a filter; additive in ABI 8).
 * msh_schedule_sequential_spread_scored / _spread_scored_device take msh_schedule_sequential_spread's arguments and
 * are the superset call: a caller may use them whatever the ctx's resource score mode is.
 * With mode NONE the call behaves as msh_schedule_sequential_spread / _spread_device in every respect: the same
 *   kernel instance, limits and refusals, nres = 0 included.
 * With LEAST_ALLOCATED / MOST_ALLOCATED the two sections above compose. Pods are decided strictly in order; for pod
 *   j with pg = pod_group[j]:
 *   The feasible set is _spread's: the filter list, count[i] < eff[i], every positive request fits, and for
 *   pg >= 0 also zone[i] >= 0 and cnt[pg][zone[i]] + 1 - minc(pg) <= max_skew[pg], minc over Zset.
 *   The status is _spread's: MSH_FIT_ERROR with no feasible node, otherwise MSH_SCORE_ERROR when NodeNumber scores
 *   without its PreScore state (commits nothing), otherwise MSH_PLACED.
 *   A feasible node's total is the scored _fit call's, T(i) + weight * RS(j, i), exactly as written under
 *   msh_set_resource_score (q = used + req before this pod's commit, truncating int64, a zero capacity or q > c
 *   scores 0, resources of weight 0 are fitted but not scored). NodeNumber's normalizer extents are taken over the
 *   feasible list, which is the spread-filtered one.
 *   The pod goes to the first maximum of total in List order; out_score and commit_cb get that total.
 *   The commit: count[sel] += 1, used[r][sel] += req[r][j], and for pg >= 0 cnt[pg][zone[sel]] += 1.
 * Refusals of a scored call, in this order. MSH_TIEBREAK_RANDOM, a score-column list: MSH_ERR_UNSUPPORTED. No node
 *   table, no zone column, no resource table: MSH_ERR_STATE. nres != the table's: MSH_ERR_INVALID. nres != the
 *   setting's (so nres = 0 with a score set): MSH_ERR_STATE. A table past the limit: MSH_ERR_UNSUPPORTED with the
 *   limit in the message; the limits are the scored _fit call's, 4,096 nodes for one or two resources, 2,048 for
 *   three or four. The ctx's largest written amount above MSH_RESOURCE_SCORE_MAX: MSH_ERR_UNSUPPORTED. Host form: a
 *   group outside [-1, G), a request outside [0, 2^62] or above MSH_RESOURCE_SCORE_MAX: MSH_ERR_INVALID.
 * msh_seq_spread_scored_max_nodes reports the limit of the call as the ctx is set now, for nres in 0..4: the scored
 *   limits with a mode other than NONE, msh_seq_spread_max_nodes' with NONE.
 * The device form is asynchronous and ordered with the ctx's other sequential launches as _spread_device is; it
 *   validates neither d_pod_req nor d_pod_group, and the kernel treats every group value outside [0, G) as -1.
 * A failed call changes nothing. */
int msh_seq_spread_scored_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t* out_max_nodes);
int msh_schedule_sequential_spread_scored(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                          const int32_t* pod_group, int32_t nres, const int64_t* pod_req,
                                          int32_t max_pods_per_node, int32_t* out_idx, int64_t* out_score,
                                          int32_t* out_status, msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_spread_scored_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                                                 const uint8_t* d_pod_tol, const int32_t* d_pod_group, int32_t nres,
                                                 const int64_t* d_pod_req, int32_t max_pods_per_node,
                                                 int32_t* d_out_idx, int64_t* d_out_score, int32_t* d_out_status,
                                                 void* stream);

/* Static node filters: per-class node masks (upstream's nodeSelector, required NodeAffinity, TaintToleration for
 * NoSchedule / NoExecute taints and NodeName; additive in ABI 8). The verdict of each of these filters for a (pod,
 * node) pair depends only on the pod's spec and the node's labels, taints and name, never on a commit. The host
 * groups the pods of a call into at most MSH_MAX_POD_CLASSES classes of identical constraints and gives the ctx, per
 * node, 64 bits: bit c is set if the node admits pods of class c.
 * The column. bits[i], one uint64 per uploaded node in List order, for C classes, 1 <= C <= MSH_MAX_POD_CLASSES; a
 *   set bit at or above C is MSH_ERR_INVALID, n different from the uploaded node count MSH_ERR_INVALID, a call before
 *   msh_upload_nodes MSH_ERR_STATE.
 * Lifetime and ordering are the capacity column's. msh_upload_nodes drops the column; msh_patch_nodes, the count,
 *   capacity, resource and zone writers and the count resets keep it. The writers and the reader are synchronous and
 *   ordered after the ctx's sequential launches in flight; none of them rebuilds the node table.
 *   msh_patch_node_class_bits replaces the whole words of nodes idx[k] (pairwise distinct, in range; with no column
 *   MSH_ERR_STATE). msh_clear_node_class_bits returns to "no column". msh_node_class_bits reports *out_present, and
 *   with a column *out_C and the n words (out_C and out_bits may be NULL).
 * msh_schedule_sequential_classes / _classes_device are the superset call: msh_schedule_sequential_spread_scored's
 *   contract and arguments with one more per-pod input, pod_class[j] in [-1, C).
 *   A pod of class -1 is decided exactly as _spread_scored decides it. For a pod of class c >= 0, node i is feasible
 *   iff it is feasible for _spread_scored and bit c of bits[i] is set. Everything downstream is taken over this
 *   feasible set: the status order (MSH_FIT_ERROR, then MSH_SCORE_ERROR, then MSH_PLACED), NodeNumber's normalizer
 *   extents, the resource score, the first maximum in List order and the commit. A class does not change what a
 *   commit writes. The spread minimum stays over Zset, as upstream's does.
 *   pod_class == NULL: every pod has class -1 and no column is needed; with pod_group non-NULL the call is then
 *   _spread_scored itself, the same kernel instance. pod_class non-NULL without a column: MSH_ERR_STATE.
 *   pod_group == NULL is allowed here and only here: every pod is ungrouped and no zone column is required. With
 *   pod_group non-NULL the zone column is required, as in _spread.
 * Refusals are _spread_scored's, in its order (the class column's MSH_ERR_STATE follows the zone column's). Host
 *   form: also a class outside [-1, C): MSH_ERR_INVALID. The device form validates nothing: the kernel treats every
 *   class value outside [0, C) as -1, so no memory is indexed with a pod's raw value.
 * Node limits are those of the kernel form that runs: msh_seq_classes_max_nodes reports _spread's limits with score
 *   mode NONE (8,192 nodes up to two resources, 4,096 above) and the scored limits otherwise (4,096 / 2,048).
 * Every other entry point ignores the column. A failed call changes nothing. */
#define MSH_MAX_POD_CLASSES 64
int msh_upload_node_class_bits(msh_ctx* ctx, int32_t n, int32_t C, const uint64_t* bits);
int msh_patch_node_class_bits(msh_ctx* ctx, int32_t count, const int32_t* idx, const uint64_t* bits);
int msh_clear_node_class_bits(msh_ctx* ctx);
int msh_node_class_bits(msh_ctx* ctx, int32_t* out_C, uint64_t* out_bits, int32_t* out_present);
int msh_seq_classes_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t* out_max_nodes);
int msh_schedule_sequential_classes(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                    const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                    const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                    int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_classes_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                                           const uint8_t* d_pod_tol, const int32_t* d_pod_group,
                                           const int32_t* d_pod_class, int32_t nres, const int64_t* d_pod_req,
                                           int32_t max_pods_per_node, int32_t* d_out_idx, int64_t* d_out_score,
                                           int32_t* d_out_status, void* stream);

/* Preferred node affinity and PreferNoSchedule scores (the scoring halves of upstream's NodeAffinity and
 * TaintToleration, v1.22: nodeaffinity/node_affinity.go Score / NormalizeScore, tainttoleration/taint_toleration.go
 * Score / NormalizeScore; additive in ABI 8). Two raw values per (pod class, node), static as the class masks are:
 *   A[c][i]: the summed weights of the class's preferredDuringSchedulingIgnoredDuringExecution terms that match node i;
 *   T[c][i]: the number of node i's PreferNoSchedule taints that the class does not tolerate.
 * Their normalisation is not static: upstream normalises over the pod's feasible nodes, which change with every
 * commit, so the kernel takes both maxima per pod.
 * The column. affinity and taints are [C][n], class-major, nodes in List order, 1 <= C <= MSH_MAX_POD_CLASSES;
 *   either may be NULL (all zero). n different from the uploaded node count is MSH_ERR_INVALID, a call before
 *   msh_upload_nodes MSH_ERR_STATE.
 * Lifetime and ordering are the class masks'. msh_upload_nodes drops the column; msh_patch_nodes, the count, capacity,
 *   resource, zone and class-mask writers and the count resets keep it. The writers and the reader are synchronous
 *   and ordered after the ctx's sequential launches in flight. msh_patch_node_class_prefs replaces the values of
 *   nodes idx[k] for every class (arrays [C][count]; a NULL array writes zeros; indices pairwise distinct and in
 *   range; with no column MSH_ERR_STATE). msh_clear_node_class_prefs returns to "no column". msh_node_class_prefs
 *   reports *out_present, and with a column *out_C and the two [C][n] arrays (each may be NULL).
 * The class space is shared with the class masks: when both columns are present at a call their C must be equal,
 *   else MSH_ERR_STATE. A preference column without class masks means every node admits every class; class masks
 *   without a preference column mean A = T = 0.
 * msh_set_preference_weights: the plugin weights w_affinity and w_taint, each in [0, 100] (else MSH_ERR_INVALID),
 *   default 0 / 0.
 * msh_schedule_sequential_prefs / _prefs_device take msh_schedule_sequential_classes' arguments and contract. Per
 *   pod, with F its feasible set exactly as _classes defines it:
 *     maxA = max over F of A; na_i = 0 if maxA == 0, else floor(100 * A_i / maxA);
 *     maxT = max over F of T; nt_i = 100 if maxT == 0, else 100 - floor(100 * T_i / maxT);
 *     total_i = _classes's total_i + w_affinity * na_i + w_taint * nt_i,
 *   the first maximum in List order wins and out_score is that total. A pod of class -1, and every pod when no
 *   preference column is present, has A = T = 0: na = 0 and nt = 100 on every node, so out_score still carries
 *   w_taint * 100. The status order and the commit are _classes's.
 *   With both weights 0 the call is _classes itself, bit for bit, the same kernel instance.
 *   Resource score mode NONE is allowed (the resource term is 0; nres may be 0).
 * Refusals are _classes's, in its order (the class masks are not required by themselves), then: pod_class non-NULL
 *   with neither column present, or both with unequal C: MSH_ERR_STATE; 100 * (W_res + w_affinity + w_taint) > 65,534,
 *   W_res the resource score's plugin weight (0 in mode NONE): MSH_ERR_UNSUPPORTED (the packed key cannot hold the
 *   sum). The device form treats every class value outside [0, C) as -1.
 * Node limits: msh_seq_prefs_max_nodes, 4,096 nodes up to two resources and 2,048 above, in every score mode.
 * Every other entry point ignores the column and the weights. A failed call changes nothing. */
int msh_upload_node_class_prefs(msh_ctx* ctx, int32_t n, int32_t C, const uint16_t* affinity, const uint16_t* taints);
int msh_patch_node_class_prefs(msh_ctx* ctx, int32_t count, const int32_t* idx, const uint16_t* affinity,
                               const uint16_t* taints);
int msh_clear_node_class_prefs(msh_ctx* ctx);
int msh_node_class_prefs(msh_ctx* ctx, int32_t* out_C, uint16_t* out_affinity, uint16_t* out_taints,
                         int32_t* out_present);
int msh_set_preference_weights(msh_ctx* ctx, int32_t w_affinity, int32_t w_taint);
int msh_preference_weights(const msh_ctx* ctx, int32_t* out_w_affinity, int32_t* out_w_taint);
int msh_seq_prefs_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t* out_max_nodes);
int msh_schedule_sequential_prefs(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                  const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                  const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                  int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_prefs_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                         const int32_t* d_pod_group, const int32_t* d_pod_class, int32_t nres,
                                         const int64_t* d_pod_req, int32_t max_pods_per_node, int32_t* d_out_idx,
                                         int64_t* d_out_score, int32_t* d_out_status, void* stream);

/* Soft topology spread: PodTopologySpread's scoring half, whenUnsatisfiable: ScheduleAnyway (upstream v1.22,
 * podtopologyspread/scoring.go, one constraint per group and the zone key; additive in ABI 8).
 * Group modes. msh_set_spread_group_modes gives each of the ctx's G spread groups a mode, MSH_SPREAD_DO_NOT_SCHEDULE
 *   (the default of every group: the hard filter) or MSH_SPREAD_SCHEDULE_ANYWAY. G different from the current group
 *   count, or a value above 1: MSH_ERR_INVALID. msh_get_spread_group_modes reads *out_G and the G modes back (either
 *   may be NULL). msh_set_spread_groups with a different G resets every mode to the default, with the same G it keeps
 *   them. Counts, zones and skews keep their lifetime rules.
 * msh_set_spread_score_weight: the plugin weight w_spread in [0, 100] (else MSH_ERR_INVALID), default 0.
 * msh_schedule_sequential_soft / _soft_device take msh_schedule_sequential_prefs' arguments and contract. A pod whose
 *   group g is SCHEDULE_ANYWAY passes through no spread filter: its feasible set F is the one of an ungrouped pod of
 *   its class, nodes with zone < 0 included. With Zs the zones of the zoned nodes in F and size = |Zs|:
 *     raw_z = Round(double(cnt[g][z]) * log(size + 2) + double(max_skew[g] - 1)) for z in Zs, the product and the sum
 *       two separately rounded IEEE double operations (no fused multiply-add), Round half away from zero, the 65
 *       values log(size + 2) computed once by the library's std::log (msh_spread_soft_weight returns them; size
 *       outside [0, MSH_MAX_ZONES] or a NULL output: MSH_ERR_INVALID);
 *     mx = max raw_z, mn = min raw_z over Zs;
 *     ns_i = 100 if mx == 0 else 100 * (mx + mn - raw_zone[i]) / mx, truncated, for i in F with zone[i] >= 0;
 *     ns_i = 0 for i in F with zone[i] < 0, and on every node when Zs is empty;
 *     total_i = _prefs' total_i + w_spread * ns_i,
 *   the first maximum in List order wins and out_score is that total. An ungrouped pod and a pod of a
 *   DO_NOT_SCHEDULE group have ns = 0 everywhere and are decided exactly as _prefs decides them. The commit is
 *   _prefs'; a placed pod of a soft group adds 1 to cnt[g][zone[sel]] only when zone[sel] >= 0.
 *   With no SCHEDULE_ANYWAY group on the ctx the call is _prefs itself, bit for bit, the same kernel instance,
 *   whatever w_spread is. With one, the checks are those of a _prefs call with a nonzero preference weight (the class
 *   masks are not required by themselves) whatever the preference weights are.
 * Refusals are _prefs', in its order, then: 100 * (W_res + w_affinity + w_taint + w_spread) > 65,534:
 *   MSH_ERR_UNSUPPORTED; and, for a call with pod groups, MSH_ERR_UNSUPPORTED when a spread count may exceed
 *   MSH_SPREAD_SOFT_MAX (the library keeps an upper bound: the largest count at the last msh_patch_spread_counts,
 *   0 when the counts were zeroed, plus the pods submitted to calls with groups since), when p exceeds it, or when
 *   a SCHEDULE_ANYWAY group's max_skew does.
 * Node limits: msh_seq_soft_max_nodes, _prefs' limits.
 * The other calls that take pod_group (_spread, _spread_scored, _classes, _prefs) refuse with MSH_ERR_UNSUPPORTED and
 *   a message naming msh_schedule_sequential_soft when the ctx holds a SCHEDULE_ANYWAY group and pod_group is
 *   non-NULL; with every mode at its default nothing about them changes. A failed call changes nothing. */
#define MSH_SPREAD_DO_NOT_SCHEDULE 0
#define MSH_SPREAD_SCHEDULE_ANYWAY 1
#define MSH_SPREAD_SOFT_MAX (1 << 24)
int msh_set_spread_group_modes(msh_ctx* ctx, int32_t G, const uint8_t* mode);
int msh_get_spread_group_modes(const msh_ctx* ctx, int32_t* out_G, uint8_t* out_mode);
int msh_set_spread_score_weight(msh_ctx* ctx, int32_t w_spread);
int msh_spread_score_weight(const msh_ctx* ctx, int32_t* out_w_spread);
int msh_spread_soft_weight(int32_t size, double* out);
int msh_seq_soft_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t* out_max_nodes);
int msh_schedule_sequential_soft(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                 const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                 const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                 int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_soft_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                        const int32_t* d_pod_group, const int32_t* d_pod_class, int32_t nres,
                                        const int64_t* d_pod_req, int32_t max_pods_per_node, int32_t* d_out_idx,
                                        int64_t* d_out_score, int32_t* d_out_status, void* stream);

/* NodeResourcesBalancedAllocation in sequential-commit mode (upstream v1.22, noderesources/balanced_allocation.go,
 * the volume feature gate off; additive in ABI 8).
 * msh_set_balanced_score: the plugin weight w_balanced in [0, 100] (else MSH_ERR_INVALID), default 0;
 *   msh_balanced_score reads it back (out_w may be NULL).
 * msh_schedule_sequential_balanced / _balanced_device take msh_schedule_sequential_soft's arguments and contract and
 *   add w_balanced * BS to the total of every feasible node, for every pod (classed or not, grouped or not, with
 *   zero requests or not). For pod j against node i, with r in {0, 1} the table's first two resources (cpu and
 *   memory by convention):
 *     q_r = used_r[i] + pod_req[j][r],  c_r = alloc_r[i]
 *     f_r = c_r == 0 ? 1.0 : (double)q_r / (double)c_r;  if (f_r > 1.0) f_r = 1.0
 *     BS  = (int64_t)((1.0 - fabs(f_0 - f_1)) * 100.0)
 *   in IEEE double exactly as written: the conversions round to nearest even, the division, the difference, the
 *   subtraction from 1 and the product are each rounded once, the last conversion truncates. BS is in [0, 100].
 *   (Exact rational arithmetic gives other values: 0/1 against 4/5 is 19 here, not 20.) No default is substituted
 *   for a zero request. The first maximum in List order wins and out_score is the total, as in _soft. The call works
 *   in every resource score mode, MSH_RESOURCE_SCORE_NONE included.
 *   With w_balanced == 0 the call is _soft itself, the same outputs and state. With w_balanced > 0 the checks are
 *   those of a _soft call on a ctx with a SCHEDULE_ANYWAY group (whether or not the ctx holds one; the bounds on
 *   counts and skews apply only if it does), and in addition:
 *     no resource table, a table with fewer than two resources, or nres different from the table's: MSH_ERR_STATE;
 *     an amount of the table above MSH_RESOURCE_SCORE_MAX (the ctx's bound over uploads and patches):
 *       MSH_ERR_UNSUPPORTED; a request above it (host form): MSH_ERR_INVALID;
 *     100 * (W_res + w_affinity + w_taint + w_spread + w_balanced) > 65,534: MSH_ERR_UNSUPPORTED;
 *     a table above msh_seq_balanced_max_nodes(nres): MSH_ERR_UNSUPPORTED.
 *   Random tie-break and score-column plugin lists are refused as in _soft. A failed call changes nothing.
 * Node limits: msh_seq_balanced_max_nodes, _soft's limits (4,096 nodes up to two resources, 2,048 above).
 * No other entry point reads w_balanced. */
int msh_set_balanced_score(msh_ctx* ctx, int32_t w_balanced);
int msh_balanced_score(const msh_ctx* ctx, int32_t* out_w);
int msh_seq_balanced_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t* out_max_nodes);
int msh_schedule_sequential_balanced(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                     const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                     const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                     int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_balanced_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                                            const uint8_t* d_pod_tol, const int32_t* d_pod_group,
                                            const int32_t* d_pod_class, int32_t nres, const int64_t* d_pod_req,
                                            int32_t max_pods_per_node, int32_t* d_out_idx, int64_t* d_out_score,
                                            int32_t* d_out_status, void* stream);

/* Required inter-pod affinity and anti-affinity in sequential-commit mode (upstream v1.22,
 * interpodaffinity/filtering.go: the filter; the preferred, scoring half of the plugin is not implemented;
 * additive in ABI 8).
 * Terms. A ctx holds T terms, 0 <= T <= MSH_MAX_AFFINITY_TERMS. A term is a (label selector + namespaces, topology
 *   key) pair as the host sees it; the device sees its topology alone: MSH_TOPOLOGY_HOSTNAME (the domain is the node
 *   itself) or MSH_TOPOLOGY_ZONE (the domain is the node's id in the zone column, msh_upload_node_zones; a node
 *   with zone -1 lacks the key).
 *   msh_set_pod_affinity_terms(T, topo): sets the terms, drops the profiles and zeroes the state; T = 0 is "no
 *   terms". T outside [0, 32] or a topo value above 1: MSH_ERR_INVALID. msh_get_pod_affinity_terms reads them back
 *   (either output may be NULL).
 * Profiles. A ctx holds Q pod profiles, 0 <= Q <= MSH_MAX_POD_PROFILES. Profile q is match[q] (bit t: a pod of the
 *   profile satisfies term t by its labels and namespace), anti[q] (the pod's own required anti-affinity terms) and
 *   aff[q] in [-1, T) (its one required affinity term, -1: none). Upstream counts only the existing pods that match
 *   all of a pod's affinity terms, so a pod with more than one is not expressible here and must not be approximated.
 *   msh_set_pod_profiles(Q, match, anti, aff): a bit at or above T, aff outside [-1, T) or Q outside [0, 64]:
 *   MSH_ERR_INVALID; on a ctx without terms: MSH_ERR_STATE. msh_get_pod_profiles reads them back.
 * State. Two words per node: present[i], the OR of match over the pods committed to node i, and repel[i], the OR of
 *   anti over them. Nothing zone-level is stored: a launch derives presentZ[z] / repelZ[z] (the OR over the nodes of
 *   zone z) and `any` (the OR of present & HM over every node and of present & ZM over the nodes with a zone; HM /
 *   ZM: the hostname / zone terms) from the words and the zone column as they are.
 *   msh_upload_pod_affinity_state(n, present, repel): either pointer may be NULL (zeros); n other than the node
 *   count: MSH_ERR_INVALID. msh_patch_pod_affinity_state(count, idx, present, repel): whole words of nodes idx[k]
 *   (pairwise distinct, within the table; a NULL array writes zeros). msh_pod_affinity_state reads both columns
 *   (either output may be NULL). A bit at or above T: MSH_ERR_INVALID; any of the three on a ctx without terms:
 *   MSH_ERR_STATE. Lifetime and ordering are the class masks' (synchronous, ordered after the sequential launches in
 *   flight), except that msh_upload_nodes zeroes the state and keeps the terms and profiles; every other writer
 *   keeps all three.
 * msh_schedule_sequential_podaffinity / _podaffinity_device take msh_schedule_sequential_balanced's arguments and
 *   contract with one more per-pod column after pod_class, pod_profile[j] in [-1, Q) (-1: the pod reads and writes
 *   none of the state). For a pod of profile q with M = match[q], AA = anti[q], AF = aff[q] >= 0 ? 1 << aff[q] : 0,
 *   and node i with P_i = (present[i] & HM) | (zone[i] >= 0 ? presentZ[zone[i]] & ZM : 0), R_i likewise from repel,
 *   node i passes when
 *     (P_i & AA) == 0                                   the pod's own anti-affinity
 *     (R_i & M) == 0                                    the placed pods' anti-affinity (symmetric)
 *     AF == 0, or node i has the term's topology key (a zone term fails on a node without a zone) and either
 *       (P_i & AF) != 0 or the first-pod exception holds: (any & AF) == 0 && (M & AF) != 0.
 *   The conjunct narrows the feasible set before anything else reads it: the status order, NodeNumber's extents, the
 *   preference maxima, a soft group's zones, the scores, the first maximum and the commit are taken over what is
 *   left; the hard spread minimum stays over the zones of the table. No feasible node: MSH_FIT_ERROR. A placed pod
 *   ORs M into present[sel] and AA into repel[sel], seen by the next pod.
 *   pod_profile == NULL is _balanced itself: the same kernel, outputs, state and refusals. With a profile column the
 *   refusals are _balanced's in its order, where the checks that belong to the packed key (the classes' columns, the
 *   weights' sum with w_spread and w_balanced) always apply and those that belong to the balanced term (a table of
 *   two resources, every amount within 2^55 in mode NONE) apply with w_balanced > 0 only: the form works with
 *   w_balanced == 0 and in resource score mode NONE. Then, in this order: no terms or no profiles: MSH_ERR_STATE; a
 *   zone term on a ctx without a zone column: MSH_ERR_STATE; a launch whose workgroup memory (the node words, 8
 *   bytes per held node, beside 260 bytes per spread group of the call) would pass 65,536 bytes:
 *   MSH_ERR_UNSUPPORTED with the largest group count that fits in the message (only a table above 1,024 nodes with
 *   up to two resources is ever affected: it takes 102 groups of the 128). The host form refuses a profile outside
 *   [-1, Q) with MSH_ERR_INVALID; the device form treats it as -1. A failed call changes nothing.
 * Node limits: msh_seq_podaffinity_max_nodes, _balanced's. No other entry point reads the terms, profiles or state. */
#define MSH_MAX_AFFINITY_TERMS 32
#define MSH_MAX_POD_PROFILES 64
#define MSH_TOPOLOGY_HOSTNAME 0
#define MSH_TOPOLOGY_ZONE 1
int msh_set_pod_affinity_terms(msh_ctx* ctx, int32_t T, const uint8_t* topo);
int msh_get_pod_affinity_terms(const msh_ctx* ctx, int32_t* out_T, uint8_t* out_topo);
int msh_set_pod_profiles(msh_ctx* ctx, int32_t Q, const uint32_t* match, const uint32_t* anti, const int32_t* aff);
int msh_get_pod_profiles(const msh_ctx* ctx, int32_t* out_Q, uint32_t* out_match, uint32_t* out_anti, int32_t* out_aff);
int msh_upload_pod_affinity_state(msh_ctx* ctx, int32_t n, const uint32_t* present, const uint32_t* repel);
int msh_patch_pod_affinity_state(msh_ctx* ctx, int32_t count, const int32_t* idx, const uint32_t* present,
                                 const uint32_t* repel);
int msh_pod_affinity_state(msh_ctx* ctx, uint32_t* out_present, uint32_t* out_repel);
int msh_seq_podaffinity_max_nodes(const msh_ctx* ctx, int32_t nres, int32_t* out_max_nodes);
int msh_schedule_sequential_podaffinity(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                        const int32_t* pod_group, const int32_t* pod_class,
                                        const int32_t* pod_profile, int32_t nres, const int64_t* pod_req,
                                        int32_t max_pods_per_node, int32_t* out_idx, int64_t* out_score,
                                        int32_t* out_status, msh_commit_cb commit_cb, void* user);
int msh_schedule_sequential_podaffinity_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                                               const uint8_t* d_pod_tol, const int32_t* d_pod_group,
                                               const int32_t* d_pod_class, const int32_t* d_pod_profile,
                                               int32_t nres, const int64_t* d_pod_req, int32_t max_pods_per_node,
                                               int32_t* d_out_idx, int64_t* d_out_score, int32_t* d_out_status,
                                               void* stream);

/* ---- node-sharded mode (a cluster's node table split over devices) ----
 * Each shard holds a contiguous slice [node_base, node_base + n) of the global List order and
 * produces int32 keys, key = 0x7FFFFFFF - global_idx (0 = none), so that the element-wise MAX
 * over shards (one RCCL allreduce MAX) is the global first node. Layout (ABI v7), msh_shard_keys_len
 * = 2p entries, every entry a property of pod j alone (evaluated per (pod, node) pair of the shard):
 *   keys[j]      first feasible node whose NodeNumber score is 10 for pod j (feasible match)
 *   keys[p + j]  REVERSE / MINMAX normalize: first feasible node whose NodeNumber score is 0 for pod j
 *                (feasible non-match); every other mode: first feasible node for pod j
 * 8 B per pod cross the interconnect (selectHost over the merged keys replaces minisched.go:304-325
 * across shards; the first feasible node is the larger of the two keys in either case). msh_decode_keys_device then
 * produces idx/score/status exactly as msh_schedule_batch over the whole table. Score-column plugin
 * lists use msh_generic_extents_device / msh_generic_best_device / msh_generic_decode_device below. */
int msh_shard_keys_len(const msh_ctx* ctx, int32_t p, int32_t* out_len);
int msh_shard_keys_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                          const uint8_t* d_pod_tol, int64_t node_base, int32_t* d_keys,
                          void* stream);
int msh_decode_keys_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit,
                           const uint8_t* d_pod_tol, const int32_t* d_keys,
                           int32_t* d_out_idx, int64_t* d_out_score, int32_t* d_out_status,
                           void* stream);
/* Kept for ABI compatibility: always 0 since ABI v7 (keys[p + j] is per pod, never per pod class). */
int msh_keys_slot1_is_any(const msh_ctx* ctx, int32_t* out_flag);

/* ---- node-sharded generic pipeline (ABI v7): any plugin list, score-column lists included ----
 * Each shard (a contiguous List-order slice, as above) computes per pod its best (int64 total, global
 * node index) over its nodes; the merge is two all-reduces, MAX over the totals, then MIN over the
 * indices of the shards that hold the maximum (the global first maximum: selectHost,
 * minisched.go:304-325, across shards). A plugin that normalizes needs the pod's extent (max, min of
 * its raw scores) over the feasible nodes of EVERY shard before any total is formed:
 *   1. len = msh_generic_ext_len(ctx, p); when len > 0: msh_generic_extents_device on every shard into
 *      len int64 (the minima stored negated), then one all-reduce MAX of them;
 *   2. msh_generic_best_device(..., d_ext (the merged extents, or NULL when len == 0), node_base,
 *      d_total, d_idx): this shard's best per pod (INT64_MIN / INT32_MAX: no feasible node here);
 *   3. d_merged = copy of d_total, all-reduce MAX over d_merged;
 *   4. msh_generic_candidates_device(p, d_total, d_merged, d_idx): d_idx[j] = INT32_MAX unless this
 *      shard holds pod j's maximum; then all-reduce MIN over d_idx;
 *   5. msh_generic_decode_device(..., d_merged, d_idx, outputs): idx / score / status exactly as
 *      msh_schedule_batch over the whole table (FitError when no shard has a feasible node).
 * Device pointers, asynchronous on `stream` (hipStream_t as void*, NULL = the null stream). */
int msh_generic_ext_len(const msh_ctx* ctx, int32_t p, int64_t* out_len);
int msh_generic_extents_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                               int64_t* d_ext, void* stream);
int msh_generic_best_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                            const int64_t* d_ext, int64_t node_base, int64_t* d_best_total, int32_t* d_best_idx,
                            void* stream);
int msh_generic_candidates_device(msh_ctx* ctx, int32_t p, const int64_t* d_local_total, const int64_t* d_merged_total,
                                  int32_t* d_best_idx, void* stream);
int msh_generic_decode_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit, const int64_t* d_merged_total,
                              const int32_t* d_merged_idx, int32_t* d_out_idx, int64_t* d_out_score,
                              int32_t* d_out_status, void* stream);

/* ---- node-sharded scheduling with the merge inside the library (ABI v8) ----
 * The entry points above leave the cross-shard merge to the caller. These own it, in the two shapes a
 * scheduler process takes; both give exactly msh_schedule_batch over the whole List-order table
 * (selectHost's first maximum, minisched.go:304-325, across shards), for every plugin list.
 *
 * (1) One process per GPU: an RCCL communicator inside the ctx (librccl.so.1, loaded on the first
 *     msh_comm_* call). Rank 0 makes an id with msh_comm_unique_id; the caller ships its
 *     MSH_COMM_ID_BYTES bytes to every rank over any channel (a Go scheduler: its own RPC or a file);
 *     every rank then calls msh_comm_init (collective: it returns once all `world` ranks have joined).
 *     msh_schedule_nodeshard_device runs, on `stream`: the shard kernel over this ctx's slice, the
 *     all-reduce(s) over xGMI (ncclAllReduce on the same stream), and the decode; every rank ends with
 *     every pod's decision. The reference plugins take one all-reduce(MAX) of 8 B per pod; a list with
 *     score columns or a normalizer takes the generic form's three (extents MAX, totals MAX, indices
 *     MIN). All ranks must make the same sequence of calls with the same p. A ctx without a
 *     communicator runs the same path as a world of one. node_base = the global List index of this
 *     ctx's first node. The ctx's merge buffers are shared by its node-sharded launches: a launch on
 *     another stream first waits for the previous one. */
#define MSH_COMM_ID_BYTES 128
int msh_comm_unique_id(uint8_t* out_id); /* out_id: MSH_COMM_ID_BYTES bytes (ncclGetUniqueId) */
int msh_comm_init(msh_ctx* ctx, const uint8_t* id, int32_t world, int32_t rank);
/* world / rank of the ctx's communicator (world 0, rank 0 when msh_comm_init has not been called). */
int msh_comm_info(const msh_ctx* ctx, int32_t* out_world, int32_t* out_rank);
int msh_schedule_nodeshard_device(msh_ctx* ctx, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                  int64_t node_base, int32_t* d_out_idx, int64_t* d_out_score,
                                  int32_t* d_out_status, void* stream);
/* The same from host buffers (the cgo form), synchronous: the pod columns go to the device and the
 * decisions come back as in msh_schedule_batch. */
int msh_schedule_nodeshard(msh_ctx* ctx, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                           int64_t node_base, int32_t* out_idx, int64_t* out_score, int32_t* out_status);

/* (2) One process driving several devices (the reference's single scheduling loop, minisched.go:28-30,
 *     with its node table split over the node's GPUs): a group of shard ctxs, shards[k] holding the k-th
 *     contiguous slice of the List order (node_base = the node counts of shards[0..k) at call time).
 *     The ctxs stay owned by the caller (destroy the group first) and may sit on any devices, the same
 *     one included; shards on different devices need peer access to shards[0]'s device (xGMI; else
 *     MSH_ERR_UNSUPPORTED at msh_group_create). Every shard must hold the same plugin lists (checked per
 *     call: MSH_ERR_STATE). msh_group_schedule_batch: the pod columns are copied to every shard device,
 *     each shard runs its kernel on its own stream, and the merge runs on shards[0]'s device as one
 *     kernel that reads every shard's per-pod result over xGMI (peer loads) and decodes; a list with
 *     normalizers first merges the per-pod extents the same way and every shard reads them back. Host
 *     buffers, synchronous. Up to MSH_GROUP_MAX_SHARDS shards. */
#define MSH_GROUP_MAX_SHARDS 16
typedef struct msh_group msh_group;
int msh_group_create(msh_ctx* const* shards, int32_t n, msh_group** out_group);
void msh_group_destroy(msh_group* group);
const char* msh_group_last_error(const msh_group* group); /* NULL group: the last failed msh_group_create */
int msh_group_schedule_batch(msh_group* group, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                             int32_t* out_idx, int64_t* out_score, int32_t* out_status);

/* ---- kernel timing (measurement hook) ----
 * msh_timing_begin arms up to max_launches (1..4096) event pairs: each following hot-kernel launch of
 * this ctx made from this thread (the batch, multi-batch, generic and sequential kernels) records its
 * pair at the kernel's own start and completion (hipExtLaunchKernelGGL), the interval a kernel trace
 * (rocprofv3) reports, without the stream gaps around it. msh_timing_end waits for the recorded
 * launches and returns their count, summed and longest duration (ms), and disarms. Launches past
 * max_launches are not timed. Not needed by a scheduler; used by bench.py's roofline. */
int msh_timing_begin(msh_ctx* ctx, int32_t max_launches);
int msh_timing_end(msh_ctx* ctx, int32_t* out_launches, double* out_total_ms, double* out_max_ms);

/* ---- snapshot packer (host, no device needed) ----
 * Names are given as one byte blob + n+1 offsets (name i = blob[off[i]:off[i+1]]).
 * msh_pack_nodes sorts nodes byte-wise by name (the apiserver LIST order), and writes
 * out_order[k] = input index of the k-th node in List order, plus the SoA columns.
 * Empty names are rejected (the reference would panic on name[len-1:]). Duplicate names
 * are rejected (apiserver names are unique). */
int msh_pack_nodes(int32_t n, const char* names, const int64_t* name_off,
                   const uint8_t* unschedulable, int32_t* out_order, uint8_t* out_unsched,
                   int8_t* out_digit);

/* One toleration of pod.Spec.Tolerations (k8s.io/api core/v1 Toleration). NULL == "". */
typedef struct msh_toleration {
  const char* key;
  const char* op;     /* "", "Equal", "Exists" */
  const char* value;
  const char* effect; /* "", "NoSchedule", "PreferNoSchedule", "NoExecute" */
} msh_toleration;

/* Pods: digit from the name's last byte; tolerates from tolerations
 * [tol_off[j], tol_off[j+1]) of `tols` (upstream v1helper.TolerationsTolerateTaint with the
 * taint {Key: node.kubernetes.io/unschedulable, Effect: NoSchedule}). */
int msh_pack_pods(int32_t p, const char* names, const int64_t* name_off,
                  const msh_toleration* tols, const int64_t* tol_off, int8_t* out_digit,
                  uint8_t* out_tol);

/* Single-toleration predicate (Toleration.ToleratesTaint against the unschedulable taint). */
int msh_toleration_tolerates_unschedulable(const msh_toleration* t);

#ifdef __cplusplus
}
#endif

#endif /* MINISCHED_HIP_H */
