// msh_capi_seq.cpp — the grouped sequential-commit entry points of include/minisched_hip.h
// (msh_schedule_sequential_{spread, spread_scored, classes, prefs, soft, balanced, podaffinity} and their _device
// forms) and the ctx state only they read: zones, spread groups, modes, weights and counts, the class masks, the class
// preferences and the inter-pod affinity terms, profiles and state. The plain and resource-fit calls are in
// msh_capi.cpp, which also holds the helpers both share (msh_ctx.h).
//
// The fourteen entry points differ in one thing, the kernel form they launch. Each describes its arguments as a
// SeqCall and names the Form it stands for; seq_resolve decides the form that runs, seq_check holds the refusals
// of all forms in one ordered list, and seq_grouped_device / seq_grouped_host are the one device and host path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/minisched_hip.h"
#include "msh_ctx.h"
#include "msh_internal.h"

using namespace msh::capi;

// Topology spread (msh_schedule_sequential_spread): the zone column, the groups and the counts cnt[g][z]. None of
// it is versioned; the writers and readers go through prep_stream behind the sequential launches in flight, which
// read all of it at their start and write the counts at their end, and finish before they return.
namespace {
constexpr size_t SPREAD_CNT_BYTES = (size_t)MSH_MAX_SPREAD_GROUPS * MSH_MAX_ZONES * sizeof(int32_t);

// d_skew and d_spread_cnt: allocated whole and zeroed at first use
int spread_alloc(msh_ctx* c) {
  if (!c->d_skew) MSH_HIP(c, hipMalloc(&c->d_skew, MSH_MAX_SPREAD_GROUPS * sizeof(int32_t)));
  if (c->d_spread_cnt) return MSH_OK;
  int32_t* cn = nullptr;
  MSH_HIP(c, hipMalloc(&cn, SPREAD_CNT_BYTES));
  hipError_t e = hipMemsetAsync(cn, 0, SPREAD_CNT_BYTES, c->prep_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->prep_stream);
  if (e != hipSuccess) {
    (void)hipFree(cn);
    return hip_fail(c, e, "spread counts");
  }
  c->d_spread_cnt = cn;
  return MSH_OK;
}

int spread_zero_counts(msh_ctx* c) {
  MSH_HIP(c, hipMemsetAsync(c->d_spread_cnt, 0, SPREAD_CNT_BYTES, c->prep_stream));
  c->sp_cnt_bound = 0;
  return MSH_OK;
}

}  // namespace

int msh_upload_node_zones(msh_ctx* c, int32_t n, const int32_t* zone) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (n != c->n_nodes)
    return fail(c, MSH_ERR_INVALID, "zone column of " + std::to_string(n) + " entries for " +
                                        std::to_string(c->n_nodes) + " uploaded nodes");
  if (n > 0 && !zone) return fail(c, MSH_ERR_INVALID, "null zone array");
  uint64_t zset = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (zone[i] < -1 || zone[i] >= MSH_MAX_ZONES)
      return fail(c, MSH_ERR_INVALID, "zone outside [-1, MSH_MAX_ZONES) at node " + std::to_string(i));
    if (zone[i] >= 0) zset |= uint64_t(1) << zone[i];
  }
  DeviceGuard g(c->device);
  int rc = spread_alloc(c);
  if (rc != MSH_OK) return rc;
  if ((size_t)c->n_pad > c->zone_cap) {
    int32_t* dz = nullptr;
    MSH_HIP(c, hipMalloc(&dz, (size_t)c->n_pad * sizeof(int32_t)));
    wait_events(c->seq_inflight);
    (void)hipFree(c->d_zone);
    c->d_zone = dz;
    c->zone_cap = (size_t)c->n_pad;
    c->have_zone = false;
  }
  if ((rc = after_seq(c)) != MSH_OK) return rc;
  const size_t bytes = (size_t)c->n_pad * sizeof(int32_t);
  if ((rc = node_stage(c, bytes)) != MSH_OK) return rc;
  c->have_zone = false;  // a failed copy leaves no column
  int32_t* st = reinterpret_cast<int32_t*>(c->h_nstage);
  std::fill(st, st + c->n_pad, -1);  // the padding slots never hold a node
  if (n > 0) std::copy(zone, zone + n, st);
  MSH_HIP(c, hipMemcpyAsync(c->d_zone, st, bytes, hipMemcpyHostToDevice, c->prep_stream));
  if ((rc = spread_zero_counts(c)) != MSH_OK) return rc;  // a node's zone changed under its pods
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  c->h_zone.assign(zone, zone + n);
  c->zset = zset;
  c->have_zone = true;
  return MSH_OK;
}

int msh_clear_node_zones(msh_ctx* c) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  c->have_zone = false;  // launches in flight keep reading the device column, which stays allocated
  c->h_zone.clear();
  c->zset = 0;
  return MSH_OK;
}

int msh_node_zones(const msh_ctx* c, int32_t* out_zone, int32_t* out_present) {
  if (!c || !out_present) return MSH_ERR_INVALID;
  *out_present = c->have_zone ? 1 : 0;
  if (c->have_zone && out_zone) std::copy(c->h_zone.begin(), c->h_zone.end(), out_zone);
  return MSH_OK;
}

int msh_set_spread_groups(msh_ctx* c, int32_t G, const int32_t* max_skew) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (G < 0 || G > MSH_MAX_SPREAD_GROUPS) return fail(c, MSH_ERR_INVALID, "G outside [0, MSH_MAX_SPREAD_GROUPS]");
  if (G > 0 && !max_skew) return fail(c, MSH_ERR_INVALID, "null max_skew array");
  for (int32_t k = 0; k < G; ++k)
    if (max_skew[k] < 1) return fail(c, MSH_ERR_INVALID, "max_skew below 1 at group " + std::to_string(k));
  DeviceGuard g(c->device);
  int rc = spread_alloc(c);
  if (rc != MSH_OK) return rc;
  if ((rc = after_seq(c)) != MSH_OK) return rc;
  if (G > 0) {
    if ((rc = node_stage(c, (size_t)G * sizeof(int32_t))) != MSH_OK) return rc;
    std::memcpy(c->h_nstage, max_skew, (size_t)G * sizeof(int32_t));
    MSH_HIP(c, hipMemcpyAsync(c->d_skew, c->h_nstage, (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice,
                              c->prep_stream));
  }
  if (G != c->sp_groups && (rc = spread_zero_counts(c)) != MSH_OK) return rc;  // the rows mean other groups now
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  if (G != c->sp_groups) {  // other groups: every mode back to the default
    c->h_spmode.assign((size_t)G, (uint8_t)MSH_SPREAD_DO_NOT_SCHEDULE);
    c->sp_soft = 0;
  }
  c->sp_groups = G;
  c->h_skew.assign(max_skew, max_skew + G);
  return MSH_OK;
}

int msh_set_spread_group_modes(msh_ctx* c, int32_t G, const uint8_t* mode) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (G != c->sp_groups)
    return fail(c, MSH_ERR_INVALID, "modes for " + std::to_string(G) + " groups, msh_set_spread_groups set " +
                                        std::to_string(c->sp_groups));
  if (G > 0 && !mode) return fail(c, MSH_ERR_INVALID, "null mode array");
  int32_t soft = 0;
  for (int32_t k = 0; k < G; ++k) {
    if (mode[k] > MSH_SPREAD_SCHEDULE_ANYWAY)
      return fail(c, MSH_ERR_INVALID, "mode above MSH_SPREAD_SCHEDULE_ANYWAY at group " + std::to_string(k));
    soft += mode[k] == MSH_SPREAD_SCHEDULE_ANYWAY ? 1 : 0;
  }
  c->h_spmode.assign(mode, mode + G);  // host only: a launch takes the modes as kernel arguments
  c->sp_soft = soft;
  return MSH_OK;
}

int msh_get_spread_group_modes(const msh_ctx* c, int32_t* out_G, uint8_t* out_mode) {
  if (!c) return MSH_ERR_INVALID;
  if (out_G) *out_G = c->sp_groups;
  if (out_mode)
    for (int32_t k = 0; k < c->sp_groups; ++k)
      out_mode[k] = (size_t)k < c->h_spmode.size() ? c->h_spmode[(size_t)k] : (uint8_t)MSH_SPREAD_DO_NOT_SCHEDULE;
  return MSH_OK;
}

int msh_set_spread_score_weight(msh_ctx* c, int32_t w_spread) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (w_spread < 0 || w_spread > 100) return fail(c, MSH_ERR_INVALID, "spread score weight outside [0, 100]");
  c->w_spread = w_spread;
  return MSH_OK;
}

int msh_spread_score_weight(const msh_ctx* c, int32_t* out_w_spread) {
  if (!c) return MSH_ERR_INVALID;
  if (out_w_spread) *out_w_spread = c->w_spread;
  return MSH_OK;
}

namespace {
// upstream's topologyNormalizingWeight for size = 0..MSH_MAX_ZONES zones, log(size + 2): this library's std::log,
// computed once; the kernel multiplies by these values and msh_spread_soft_weight returns them
const double* soft_weights() {
  static const std::array<double, MSH_MAX_ZONES + 1> w = [] {
    std::array<double, MSH_MAX_ZONES + 1> t{};
    for (int32_t k = 0; k <= MSH_MAX_ZONES; ++k) t[(size_t)k] = std::log((double)(k + 2));
    return t;
  }();
  return w.data();
}
}  // namespace

int msh_spread_soft_weight(int32_t size, double* out) {
  if (!out || size < 0 || size > MSH_MAX_ZONES) return MSH_ERR_INVALID;
  *out = soft_weights()[size];
  return MSH_OK;
}

int msh_get_spread_groups(const msh_ctx* c, int32_t* out_G, int32_t* out_max_skew) {
  if (!c) return MSH_ERR_INVALID;
  if (out_G) *out_G = c->sp_groups;
  if (out_max_skew) std::copy(c->h_skew.begin(), c->h_skew.end(), out_max_skew);
  return MSH_OK;
}

int msh_spread_counts(msh_ctx* c, int32_t* out_cnt) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (c->sp_groups == 0) return MSH_OK;
  if (!out_cnt) return fail(c, MSH_ERR_INVALID, "null output");
  DeviceGuard g(c->device);
  int rc = after_seq(c);  // sequential launches of this ctx in flight update the counts
  if (rc != MSH_OK) return rc;
  MSH_HIP(c, hipMemcpyAsync(out_cnt, c->d_spread_cnt, (size_t)c->sp_groups * MSH_MAX_ZONES * sizeof(int32_t),
                            hipMemcpyDeviceToHost, c->prep_stream));
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  return MSH_OK;
}

int msh_patch_spread_counts(msh_ctx* c, int32_t count, const int32_t* gi, const int32_t* zi, const int32_t* value) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (count < 0) return fail(c, MSH_ERR_INVALID, "negative patch count");
  if (count == 0) return MSH_OK;
  if (!gi || !zi || !value) return fail(c, MSH_ERR_INVALID, "null patch arrays");
  std::vector<int32_t> keys((size_t)count);
  for (int32_t k = 0; k < count; ++k) {
    if (gi[k] < 0 || gi[k] >= c->sp_groups)
      return fail(c, MSH_ERR_INVALID, "group outside [0, G) at patch entry " + std::to_string(k));
    if (zi[k] < 0 || zi[k] >= MSH_MAX_ZONES)
      return fail(c, MSH_ERR_INVALID, "zone outside [0, MSH_MAX_ZONES) at patch entry " + std::to_string(k));
    if (value[k] < 0) return fail(c, MSH_ERR_INVALID, "negative count at patch entry " + std::to_string(k));
    keys[(size_t)k] = gi[k] * MSH_MAX_ZONES + zi[k];
  }
  std::vector<int32_t> sorted(keys);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return fail(c, MSH_ERR_INVALID, "duplicate (group, zone) pair");
  DeviceGuard g(c->device);
  int rc = after_seq(c);
  if (rc != MSH_OK) return rc;
  // the table (32 KB) through the page-locked stage: read, patched on the host, written back
  if ((rc = node_stage(c, SPREAD_CNT_BYTES)) != MSH_OK) return rc;
  int32_t* st = reinterpret_cast<int32_t*>(c->h_nstage);
  MSH_HIP(c, hipMemcpyAsync(st, c->d_spread_cnt, SPREAD_CNT_BYTES, hipMemcpyDeviceToHost, c->prep_stream));
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  for (int32_t k = 0; k < count; ++k) st[keys[(size_t)k]] = value[k];
  MSH_HIP(c, hipMemcpyAsync(c->d_spread_cnt, st, SPREAD_CNT_BYTES, hipMemcpyHostToDevice, c->prep_stream));
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  // the whole table is at hand: its largest count, exactly
  c->sp_cnt_bound = *std::max_element(st, st + (size_t)c->sp_groups * MSH_MAX_ZONES);
  return MSH_OK;
}

int msh_reset_spread_counts(msh_ctx* c) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->d_spread_cnt) return MSH_OK;  // never used: nothing to zero
  DeviceGuard g(c->device);
  int rc = after_seq(c);
  if (rc != MSH_OK) return rc;
  if ((rc = spread_zero_counts(c)) != MSH_OK) return rc;
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  return MSH_OK;
}

int msh_seq_spread_max_nodes(const msh_ctx* c, int32_t nres, int32_t* out_max_nodes) {
  if (!c || !out_max_nodes || nres < 0 || nres > MSH_MAX_RESOURCES) return MSH_ERR_INVALID;
  *out_max_nodes = msh::seq_spread_max_nodes(nres);
  return MSH_OK;
}

int msh_seq_spread_scored_max_nodes(const msh_ctx* c, int32_t nres, int32_t* out_max_nodes) {
  if (!c || !out_max_nodes || nres < 0 || nres > MSH_MAX_RESOURCES) return MSH_ERR_INVALID;
  *out_max_nodes = c->rs_mode != MSH_RESOURCE_SCORE_NONE ? msh::seq_spread_score_max_nodes(nres)
                                                         : msh::seq_spread_max_nodes(nres);
  return MSH_OK;
}

// The per-class node masks (msh_schedule_sequential_classes). The column is the capacity column's in lifetime and
// ordering: unversioned, written through prep_stream behind the sequential launches in flight, which read it at
// their start, and each writer finishes before it returns.
namespace {
// a device column of n_pad words; a larger one is allocated before the old one is let go, so a failure changes nothing
int class_reserve(msh_ctx* c) {
  if ((size_t)c->n_pad <= c->class_cap) return MSH_OK;
  uint64_t* d = nullptr;
  MSH_HIP(c, hipMalloc(&d, (size_t)c->n_pad * sizeof(uint64_t)));
  wait_events(c->seq_inflight);
  (void)hipFree(c->d_class);
  c->d_class = d;
  c->class_cap = (size_t)c->n_pad;
  c->have_class = false;  // the old column went with its buffer
  c->pref_dirty = true;
  c->h_class.clear();
  c->n_classes = 0;
  return MSH_OK;
}

// the whole column from `bits` (n_nodes words; the padding slots 0: they never hold a node)
int class_write_all(msh_ctx* c, const uint64_t* bits) {
  const size_t bytes = (size_t)c->n_nodes * sizeof(uint64_t);
  int rc = node_stage(c, bytes);
  if (rc != MSH_OK) return rc;
  if ((rc = after_seq(c)) != MSH_OK) return rc;
  MSH_HIP(c, hipMemsetAsync(c->d_class, 0, c->class_cap * sizeof(uint64_t), c->prep_stream));
  if (bytes > 0) {
    std::memcpy(c->h_nstage, bits, bytes);
    MSH_HIP(c, hipMemcpyAsync(c->d_class, c->h_nstage, bytes, hipMemcpyHostToDevice, c->prep_stream));
  }
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  return MSH_OK;
}

bool class_bits_above(uint64_t w, int32_t C) { return C < MSH_MAX_POD_CLASSES && (w >> C) != 0; }
}  // namespace

int msh_upload_node_class_bits(msh_ctx* c, int32_t n, int32_t C, const uint64_t* bits) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (n != c->n_nodes)
    return fail(c, MSH_ERR_INVALID, "class column of " + std::to_string(n) + " entries for " +
                                        std::to_string(c->n_nodes) + " uploaded nodes");
  if (C < 1 || C > MSH_MAX_POD_CLASSES) return fail(c, MSH_ERR_INVALID, "C outside [1, MSH_MAX_POD_CLASSES]");
  if (n > 0 && !bits) return fail(c, MSH_ERR_INVALID, "null class bits array");
  for (int32_t i = 0; i < n; ++i)
    if (class_bits_above(bits[i], C))
      return fail(c, MSH_ERR_INVALID, "a bit at or above C = " + std::to_string(C) + " is set at node " + std::to_string(i));
  DeviceGuard g(c->device);
  int rc = class_reserve(c);
  if (rc != MSH_OK) return rc;
  std::vector<uint64_t> h(bits, bits + n);
  c->have_class = false;  // a failed copy leaves no column
  c->pref_dirty = true;   // the preference table holds the masks' verdicts
  if ((rc = class_write_all(c, h.data())) != MSH_OK) return rc;
  c->h_class.swap(h);
  c->n_classes = C;
  c->have_class = true;
  return MSH_OK;
}

int msh_patch_node_class_bits(msh_ctx* c, int32_t count, const int32_t* idx, const uint64_t* bits) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (!c->have_class) return fail(c, MSH_ERR_STATE, "msh_upload_node_class_bits has not been called");
  if (count < 0) return fail(c, MSH_ERR_INVALID, "negative patch count");
  if (count == 0) return MSH_OK;
  if (!idx || !bits) return fail(c, MSH_ERR_INVALID, "null patch arrays");
  std::vector<int32_t> sorted(idx, idx + count);
  std::sort(sorted.begin(), sorted.end());
  if (sorted.front() < 0 || sorted.back() >= c->n_nodes)
    return fail(c, MSH_ERR_INVALID, "patch index outside [0, n)");
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return fail(c, MSH_ERR_INVALID, "duplicate patch index");
  for (int32_t k = 0; k < count; ++k)
    if (class_bits_above(bits[k], c->n_classes))
      return fail(c, MSH_ERR_INVALID, "a bit at or above C = " + std::to_string(c->n_classes) +
                                          " is set at patch entry " + std::to_string(k));
  DeviceGuard g(c->device);
  // the patched column whole: 64 KB at the largest table a class call takes, one copy
  std::vector<uint64_t> h(c->h_class);
  for (int32_t k = 0; k < count; ++k) h[(size_t)idx[k]] = bits[k];
  c->pref_dirty = true;
  int rc = class_write_all(c, h.data());
  if (rc != MSH_OK) {
    c->have_class = false;  // the device column is in an unknown state
    return rc;
  }
  c->h_class.swap(h);
  return MSH_OK;
}

int msh_clear_node_class_bits(msh_ctx* c) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  c->have_class = false;  // launches in flight keep reading the device column, which stays allocated
  c->pref_dirty = true;
  c->h_class.clear();
  c->n_classes = 0;
  return MSH_OK;
}

int msh_node_class_bits(msh_ctx* c, int32_t* out_C, uint64_t* out_bits, int32_t* out_present) {
  if (!c || !out_present) return MSH_ERR_INVALID;
  c->err.clear();
  *out_present = c->have_class ? 1 : 0;
  if (out_C) *out_C = c->have_class ? c->n_classes : 0;
  if (c->have_class && out_bits) std::copy(c->h_class.begin(), c->h_class.end(), out_bits);
  return MSH_OK;
}

int msh_seq_classes_max_nodes(const msh_ctx* c, int32_t nres, int32_t* out_max_nodes) {
  if (!c || !out_max_nodes || nres < 0 || nres > MSH_MAX_RESOURCES) return MSH_ERR_INVALID;
  *out_max_nodes = msh::seq_classes_max_nodes(nres, c->rs_mode != MSH_RESOURCE_SCORE_NONE);
  return MSH_OK;
}

// The per-class preference values (msh_schedule_sequential_prefs). The host copies are the column; the device table
// the kernel reads is derived from them and from the class masks by the first call after either changed
// (prefs_table), so the writers touch no device memory and cannot leave the device in an unknown state.
namespace {
void prefs_drop(msh_ctx* c) {
  c->have_prefs = false;
  c->pref_classes = 0;
  c->h_pref_a.clear();
  c->h_pref_t.clear();
  c->pref_dirty = true;
}

// The device table for the ctx's columns and a kernel of npl nodes per thread (msh::PrefArgs::rows): classes x
// PREF_THREADS records of 2 * npl dwords. Ordered after the sequential launches in flight, which read the old one
// until they end; synchronous.
int prefs_table(msh_ctx* c, int32_t npl) {
  const int32_t C = c->have_prefs ? c->pref_classes : (c->have_class ? c->n_classes : 0);
  if (!c->pref_dirty && c->pref_dev_classes == C && c->pref_stride == 2 * npl) return MSH_OK;
  const size_t rec = 2 * (size_t)npl, per_class = rec * msh::PREF_THREADS, total = per_class * (size_t)C;
  std::vector<uint32_t> h(total, 0u);
  uint64_t am = 0, tm = 0;
  const size_t n = (size_t)c->n_nodes;
  for (int32_t k = 0; k < C; ++k) {
    uint32_t* row = h.data() + per_class * (size_t)k;
    for (size_t i = 0; i < n; ++i) {
      const uint32_t av = c->have_prefs && !c->h_pref_a.empty() ? c->h_pref_a[(size_t)k * n + i] : 0u;
      const uint32_t tv = c->have_prefs && !c->h_pref_t.empty() ? c->h_pref_t[(size_t)k * n + i] : 0u;
      const bool admits = !c->have_class || ((c->h_class[i] >> k) & 1ull) != 0;
      uint32_t* r = row + (i / (size_t)npl) * rec;
      r[i % (size_t)npl] = av | (tv << 16);
      r[npl] |= (admits ? 1u : 0u) << (i % (size_t)npl);
      if (av) am |= 1ull << k;
      if (tv) tm |= 1ull << k;
    }
  }
  wait_events(c->seq_inflight);
  if (total > c->pref_cap) {
    uint32_t* d = nullptr;
    MSH_HIP(c, hipMalloc(&d, total * sizeof(uint32_t)));
    (void)hipFree(c->d_pref);
    c->d_pref = d;
    c->pref_cap = total;
    c->pref_dirty = true;  // the old table went with its buffer
  }
  if (total) MSH_HIP(c, hipMemcpy(c->d_pref, h.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->pref_dev_classes = C;
  c->pref_stride = 2 * npl;
  c->pref_amask = am;
  c->pref_tmask = tm;
  c->pref_dirty = false;
  return MSH_OK;
}
}  // namespace

int msh_upload_node_class_prefs(msh_ctx* c, int32_t n, int32_t C, const uint16_t* affinity, const uint16_t* taints) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (n != c->n_nodes)
    return fail(c, MSH_ERR_INVALID, "preference column of " + std::to_string(n) + " entries per class for " +
                                        std::to_string(c->n_nodes) + " uploaded nodes");
  if (C < 1 || C > MSH_MAX_POD_CLASSES) return fail(c, MSH_ERR_INVALID, "C outside [1, MSH_MAX_POD_CLASSES]");
  const size_t len = (size_t)C * (size_t)n;
  std::vector<uint16_t> a, t;  // an absent array stays empty: all zero
  if (affinity) a.assign(affinity, affinity + len);
  if (taints) t.assign(taints, taints + len);
  c->h_pref_a.swap(a);
  c->h_pref_t.swap(t);
  c->pref_classes = C;
  c->have_prefs = true;
  c->pref_dirty = true;
  return MSH_OK;
}

int msh_patch_node_class_prefs(msh_ctx* c, int32_t count, const int32_t* idx, const uint16_t* affinity,
                               const uint16_t* taints) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (!c->have_prefs) return fail(c, MSH_ERR_STATE, "msh_upload_node_class_prefs has not been called");
  if (count < 0) return fail(c, MSH_ERR_INVALID, "negative patch count");
  if (count == 0) return MSH_OK;
  if (!idx) return fail(c, MSH_ERR_INVALID, "null patch indices");
  std::vector<int32_t> sorted(idx, idx + count);
  std::sort(sorted.begin(), sorted.end());
  if (sorted.front() < 0 || sorted.back() >= c->n_nodes)
    return fail(c, MSH_ERR_INVALID, "patch index outside [0, n)");
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return fail(c, MSH_ERR_INVALID, "duplicate patch index");
  const size_t n = (size_t)c->n_nodes, C = (size_t)c->pref_classes;
  auto apply = [&](std::vector<uint16_t>& col, const uint16_t* v) {  // a null array writes zeros
    if (col.empty() && !v) return;
    if (col.empty()) col.assign(C * n, 0);
    for (size_t k = 0; k < C; ++k)
      for (int32_t e = 0; e < count; ++e) col[k * n + (size_t)idx[e]] = v ? v[k * (size_t)count + (size_t)e] : 0;
  };
  apply(c->h_pref_a, affinity);
  apply(c->h_pref_t, taints);
  c->pref_dirty = true;
  return MSH_OK;
}

int msh_clear_node_class_prefs(msh_ctx* c) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  prefs_drop(c);  // launches in flight keep reading the device table, which stays allocated
  return MSH_OK;
}

int msh_node_class_prefs(msh_ctx* c, int32_t* out_C, uint16_t* out_affinity, uint16_t* out_taints,
                         int32_t* out_present) {
  if (!c || !out_present) return MSH_ERR_INVALID;
  c->err.clear();
  *out_present = c->have_prefs ? 1 : 0;
  if (out_C) *out_C = c->have_prefs ? c->pref_classes : 0;
  if (!c->have_prefs) return MSH_OK;
  const size_t len = (size_t)c->pref_classes * (size_t)c->n_nodes;
  auto give = [&](const std::vector<uint16_t>& col, uint16_t* out) {
    if (!out) return;
    if (col.empty()) std::fill(out, out + len, (uint16_t)0);
    else std::copy(col.begin(), col.end(), out);
  };
  give(c->h_pref_a, out_affinity);
  give(c->h_pref_t, out_taints);
  return MSH_OK;
}

int msh_set_preference_weights(msh_ctx* c, int32_t w_affinity, int32_t w_taint) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (w_affinity < 0 || w_affinity > 100 || w_taint < 0 || w_taint > 100)
    return fail(c, MSH_ERR_INVALID, "preference weight outside [0, 100]");
  c->w_aff = w_affinity;
  c->w_taint = w_taint;
  return MSH_OK;
}

int msh_preference_weights(const msh_ctx* c, int32_t* out_w_affinity, int32_t* out_w_taint) {
  if (!c) return MSH_ERR_INVALID;
  if (out_w_affinity) *out_w_affinity = c->w_aff;
  if (out_w_taint) *out_w_taint = c->w_taint;
  return MSH_OK;
}

int msh_seq_prefs_max_nodes(const msh_ctx* c, int32_t nres, int32_t* out_max_nodes) {
  if (!c || !out_max_nodes || nres < 0 || nres > MSH_MAX_RESOURCES) return MSH_ERR_INVALID;
  *out_max_nodes = msh::seq_prefs_max_nodes(nres);
  return MSH_OK;
}

namespace {
// the classes of a prefs call: the columns' common C (0 without a column)
int32_t prefs_classes(const msh_ctx* c) { return c->have_prefs ? c->pref_classes : (c->have_class ? c->n_classes : 0); }

// the weights log(size + 2) on the device, uploaded once (synchronous)
int soft_weights_device(msh_ctx* c) {
  if (c->d_zone_weight) return MSH_OK;
  double* d = nullptr;
  const size_t bytes = (size_t)(MSH_MAX_ZONES + 1) * sizeof(double);
  MSH_HIP(c, hipMalloc(&d, bytes));
  const hipError_t e = hipMemcpy(d, soft_weights(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(c, e, "spread score weights");
  }
  c->d_zone_weight = d;
  return MSH_OK;
}
}  // namespace

int msh_seq_soft_max_nodes(const msh_ctx* c, int32_t nres, int32_t* out_max_nodes) {
  if (!c || !out_max_nodes || nres < 0 || nres > MSH_MAX_RESOURCES) return MSH_ERR_INVALID;
  *out_max_nodes = msh::seq_soft_max_nodes(nres);
  return MSH_OK;
}

int msh_set_balanced_score(msh_ctx* c, int32_t w_balanced) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (w_balanced < 0 || w_balanced > 100) return fail(c, MSH_ERR_INVALID, "balanced score weight outside [0, 100]");
  c->w_balanced = w_balanced;
  return MSH_OK;
}

int msh_balanced_score(const msh_ctx* c, int32_t* out_w) {
  if (!c) return MSH_ERR_INVALID;
  if (out_w) *out_w = c->w_balanced;
  return MSH_OK;
}

int msh_seq_balanced_max_nodes(const msh_ctx* c, int32_t nres, int32_t* out_max_nodes) {
  if (!c || !out_max_nodes || nres < 0 || nres > MSH_MAX_RESOURCES) return MSH_ERR_INVALID;
  *out_max_nodes = msh::seq_balanced_max_nodes(nres);
  return MSH_OK;
}

// Required inter-pod affinity (msh_schedule_sequential_podaffinity): the terms and profiles (host copies; the
// profiles also as the kernel's records on the device) and the per-node state, which is on the device only. The
// state is the class masks' in ordering: written through prep_stream behind the sequential launches in flight, which
// read it at their start and write it at their end, and each writer finishes before it returns.
namespace {
bool pa_bits_above(uint32_t w, int32_t T) { return T < MSH_MAX_AFFINITY_TERMS && (w >> T) != 0; }

// The device buffers, and the state column valid for the table as it stands: n_pad pairs, zeros where
// msh_upload_nodes or msh_set_pod_affinity_terms dropped it. Synchronous.
int pa_state_ready(msh_ctx* c) {
  if ((size_t)c->n_pad > c->pa_cap) {  // only after an upload of a larger table, which dropped the state
    uint2* d = nullptr;
    MSH_HIP(c, hipMalloc(&d, (size_t)c->n_pad * sizeof(uint2)));
    wait_events(c->seq_inflight);
    (void)hipFree(c->d_pa_state);
    c->d_pa_state = d;
    c->pa_cap = (size_t)c->n_pad;
    c->pa_have_state = false;
  }
  if (c->pa_have_state) return MSH_OK;
  int rc = after_seq(c);
  if (rc != MSH_OK) return rc;
  MSH_HIP(c, hipMemsetAsync(c->d_pa_state, 0, c->pa_cap * sizeof(uint2), c->prep_stream));
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  c->pa_have_state = true;
  return MSH_OK;
}

int pa_need_terms(msh_ctx* c) {
  if (c->pa_terms == 0) return fail(c, MSH_ERR_STATE, "msh_set_pod_affinity_terms has not been called");
  return MSH_OK;
}

// the whole column (n_pad pairs) into the page-locked stage
int pa_state_fetch(msh_ctx* c, uint2** out) {
  int rc = pa_state_ready(c);
  if (rc != MSH_OK) return rc;
  const size_t bytes = (size_t)c->n_pad * sizeof(uint2);
  if ((rc = node_stage(c, bytes)) != MSH_OK) return rc;
  if ((rc = after_seq(c)) != MSH_OK) return rc;
  MSH_HIP(c, hipMemcpyAsync(c->h_nstage, c->d_pa_state, bytes, hipMemcpyDeviceToHost, c->prep_stream));
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  *out = reinterpret_cast<uint2*>(c->h_nstage);
  return MSH_OK;
}

// ... and back from it
int pa_state_store(msh_ctx* c) {
  const size_t bytes = (size_t)c->n_pad * sizeof(uint2);
  MSH_HIP(c, hipMemcpyAsync(c->d_pa_state, c->h_nstage, bytes, hipMemcpyHostToDevice, c->prep_stream));
  MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  return MSH_OK;
}
}  // namespace

int msh_set_pod_affinity_terms(msh_ctx* c, int32_t T, const uint8_t* topo) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (T < 0 || T > MSH_MAX_AFFINITY_TERMS) return fail(c, MSH_ERR_INVALID, "T outside [0, MSH_MAX_AFFINITY_TERMS]");
  if (T > 0 && !topo) return fail(c, MSH_ERR_INVALID, "null topology array");
  uint32_t hm = 0, zm = 0;
  for (int32_t t = 0; t < T; ++t) {
    if (topo[t] > MSH_TOPOLOGY_ZONE)
      return fail(c, MSH_ERR_INVALID, "topology above MSH_TOPOLOGY_ZONE at term " + std::to_string(t));
    (topo[t] == MSH_TOPOLOGY_ZONE ? zm : hm) |= uint32_t(1) << t;
  }
  c->pa_terms = T;
  c->h_pa_topo.assign(topo, topo + T);
  c->pa_host_mask = hm;
  c->pa_zone_mask = zm;
  c->pa_profiles = 0;  // the profiles named the old terms
  c->h_pa_match.clear();
  c->h_pa_anti.clear();
  c->h_pa_aff.clear();
  c->pa_have_state = false;  // and so did the state: zeros, written by the next reader (launches in flight end first)
  return MSH_OK;
}

int msh_get_pod_affinity_terms(const msh_ctx* c, int32_t* out_T, uint8_t* out_topo) {
  if (!c) return MSH_ERR_INVALID;
  if (out_T) *out_T = c->pa_terms;
  if (out_topo) std::copy(c->h_pa_topo.begin(), c->h_pa_topo.end(), out_topo);
  return MSH_OK;
}

int msh_set_pod_profiles(msh_ctx* c, int32_t Q, const uint32_t* match, const uint32_t* anti, const int32_t* aff) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (int rc = pa_need_terms(c); rc != MSH_OK) return rc;
  if (Q < 0 || Q > MSH_MAX_POD_PROFILES) return fail(c, MSH_ERR_INVALID, "Q outside [0, MSH_MAX_POD_PROFILES]");
  if (Q > 0 && (!match || !anti || !aff)) return fail(c, MSH_ERR_INVALID, "null profile arrays");
  const int32_t T = c->pa_terms;
  for (int32_t q = 0; q < Q; ++q) {
    if (pa_bits_above(match[q], T) || pa_bits_above(anti[q], T))
      return fail(c, MSH_ERR_INVALID,
                  "a bit at or above T = " + std::to_string(T) + " is set at profile " + std::to_string(q));
    if (aff[q] < -1 || aff[q] >= T)
      return fail(c, MSH_ERR_INVALID, "affinity term outside [-1, T) at profile " + std::to_string(q));
  }
  DeviceGuard g(c->device);
  int rc = MSH_OK;
  if (!c->d_pa_prof) MSH_HIP(c, hipMalloc(&c->d_pa_prof, MSH_MAX_POD_PROFILES * sizeof(uint4)));
  if (Q > 0) {  // the kernel's records, behind the launches in flight, which read the old ones at their start
    if ((rc = node_stage(c, (size_t)Q * sizeof(uint4))) != MSH_OK) return rc;
    if ((rc = after_seq(c)) != MSH_OK) return rc;
    uint4* st = reinterpret_cast<uint4*>(c->h_nstage);
    for (int32_t q = 0; q < Q; ++q) st[q] = make_uint4(match[q], anti[q], aff[q] >= 0 ? uint32_t(1) << aff[q] : 0u, 0u);
    MSH_HIP(c, hipMemcpyAsync(c->d_pa_prof, st, (size_t)Q * sizeof(uint4), hipMemcpyHostToDevice, c->prep_stream));
    MSH_HIP(c, hipStreamSynchronize(c->prep_stream));
  }
  c->pa_profiles = Q;
  c->h_pa_match.assign(match, match + Q);
  c->h_pa_anti.assign(anti, anti + Q);
  c->h_pa_aff.assign(aff, aff + Q);
  return MSH_OK;
}

int msh_get_pod_profiles(const msh_ctx* c, int32_t* out_Q, uint32_t* out_match, uint32_t* out_anti, int32_t* out_aff) {
  if (!c) return MSH_ERR_INVALID;
  if (out_Q) *out_Q = c->pa_profiles;
  if (out_match) std::copy(c->h_pa_match.begin(), c->h_pa_match.end(), out_match);
  if (out_anti) std::copy(c->h_pa_anti.begin(), c->h_pa_anti.end(), out_anti);
  if (out_aff) std::copy(c->h_pa_aff.begin(), c->h_pa_aff.end(), out_aff);
  return MSH_OK;
}

int msh_upload_pod_affinity_state(msh_ctx* c, int32_t n, const uint32_t* present, const uint32_t* repel) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (int rc = pa_need_terms(c); rc != MSH_OK) return rc;
  if (n != c->n_nodes)
    return fail(c, MSH_ERR_INVALID, "state columns of " + std::to_string(n) + " entries for " +
                                        std::to_string(c->n_nodes) + " uploaded nodes");
  for (int32_t i = 0; i < n; ++i)
    if ((present && pa_bits_above(present[i], c->pa_terms)) || (repel && pa_bits_above(repel[i], c->pa_terms)))
      return fail(c, MSH_ERR_INVALID,
                  "a bit at or above T = " + std::to_string(c->pa_terms) + " is set at node " + std::to_string(i));
  DeviceGuard g(c->device);
  int rc = pa_state_ready(c);
  if (rc != MSH_OK) return rc;
  if ((rc = node_stage(c, (size_t)c->n_pad * sizeof(uint2))) != MSH_OK) return rc;
  if ((rc = after_seq(c)) != MSH_OK) return rc;
  uint2* st = reinterpret_cast<uint2*>(c->h_nstage);
  for (int32_t i = 0; i < c->n_pad; ++i)  // the padding slots never hold a node
    st[i] = i < n ? make_uint2(present ? present[i] : 0u, repel ? repel[i] : 0u) : make_uint2(0u, 0u);
  rc = pa_state_store(c);
  if (rc != MSH_OK) c->pa_have_state = false;  // the device column is in an unknown state: zeros
  return rc;
}

int msh_patch_pod_affinity_state(msh_ctx* c, int32_t count, const int32_t* idx, const uint32_t* present,
                                 const uint32_t* repel) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (int rc = pa_need_terms(c); rc != MSH_OK) return rc;
  if (count < 0) return fail(c, MSH_ERR_INVALID, "negative patch count");
  if (count == 0) return MSH_OK;
  if (!idx) return fail(c, MSH_ERR_INVALID, "null patch indices");
  std::vector<int32_t> sorted(idx, idx + count);
  std::sort(sorted.begin(), sorted.end());
  if (sorted.front() < 0 || sorted.back() >= c->n_nodes)
    return fail(c, MSH_ERR_INVALID, "patch index outside [0, n)");
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return fail(c, MSH_ERR_INVALID, "duplicate patch index");
  for (int32_t k = 0; k < count; ++k)
    if ((present && pa_bits_above(present[k], c->pa_terms)) || (repel && pa_bits_above(repel[k], c->pa_terms)))
      return fail(c, MSH_ERR_INVALID, "a bit at or above T = " + std::to_string(c->pa_terms) +
                                          " is set at patch entry " + std::to_string(k));
  DeviceGuard g(c->device);
  // the column through the page-locked stage: read, patched on the host, written back
  uint2* st = nullptr;
  int rc = pa_state_fetch(c, &st);
  if (rc != MSH_OK) return rc;
  for (int32_t k = 0; k < count; ++k) st[idx[k]] = make_uint2(present ? present[k] : 0u, repel ? repel[k] : 0u);
  rc = pa_state_store(c);
  if (rc != MSH_OK) c->pa_have_state = false;
  return rc;
}

int msh_pod_affinity_state(msh_ctx* c, uint32_t* out_present, uint32_t* out_repel) {
  if (!c) return MSH_ERR_INVALID;
  c->err.clear();
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (int rc = pa_need_terms(c); rc != MSH_OK) return rc;
  DeviceGuard g(c->device);
  uint2* st = nullptr;
  int rc = pa_state_fetch(c, &st);
  if (rc != MSH_OK) return rc;
  for (int32_t i = 0; i < c->n_nodes; ++i) {
    if (out_present) out_present[i] = st[i].x;
    if (out_repel) out_repel[i] = st[i].y;
  }
  return MSH_OK;
}

int msh_seq_podaffinity_max_nodes(const msh_ctx* c, int32_t nres, int32_t* out_max_nodes) {
  if (!c || !out_max_nodes || nres < 0 || nres > MSH_MAX_RESOURCES) return MSH_ERR_INVALID;
  *out_max_nodes = msh::seq_podaffinity_max_nodes(nres);
  return MSH_OK;
}

// The one path of the grouped calls.
namespace {
// What every grouped entry point receives. The pointers are device-visible memory in a _device call and host memory
// in a host call. out_score is optional; so are pod_group and pod_class, except that the spread forms need groups.
struct SeqCall {
  int32_t p;
  const int8_t* pod_digit;
  const uint8_t* pod_tol;
  const int32_t* pod_group;
  const int32_t* pod_class;
  int32_t nres;
  const int64_t* pod_req;
  int32_t max_pods_per_node;
  int32_t* out_idx;
  int64_t* out_score;
  int32_t* out_status;
  const char* entry = nullptr;  // the name that messages carry (seq_resolve)
  const int32_t* pod_profile = nullptr;  // msh_schedule_sequential_podaffinity alone; optional
};

// The kernel forms, in the order the features were stacked: each takes what the one before it takes and adds a term
// (the resource score, the class masks, the preference scores, the soft spread score, the balanced score, the
// inter-pod affinity filter).
enum class Form { Spread, SpreadScored, Classes, Prefs, Soft, Balanced, PodAffinity };

const char* entry_name(Form f, bool host) {
  static const char* const names[][2] = {
      {"msh_schedule_sequential_spread_device", "msh_schedule_sequential_spread"},
      {"msh_schedule_sequential_spread_scored_device", "msh_schedule_sequential_spread_scored"},
      {"msh_schedule_sequential_classes_device", "msh_schedule_sequential_classes"},
      {"msh_schedule_sequential_prefs_device", "msh_schedule_sequential_prefs"},
      {"msh_schedule_sequential_soft_device", "msh_schedule_sequential_soft"},
      {"msh_schedule_sequential_balanced_device", "msh_schedule_sequential_balanced"},
      {"msh_schedule_sequential_podaffinity_device", "msh_schedule_sequential_podaffinity"}};
  return names[(int)f][host ? 1 : 0];
}

// The form that runs for a call on entry point `asked`, and in k.entry the name its messages carry. A form with
// nothing to add to any pod is the form below it, the same kernel instance; this is the only place that decides it.
// The name follows the form down, as if each entry point had called the public one below it, with two exceptions
// that callers may have seen in messages and that stay: see the two marked lines.
Form seq_resolve(Form asked, const msh_ctx* c, SeqCall& k, bool host) {
  Form f = asked, named = asked;
  // no profile column: _balanced itself. With one the form stays whatever the weights are: its kernel serves them all
  if (f == Form::PodAffinity && !k.pod_profile) f = named = Form::Balanced;
  if (f == Form::Balanced && c->w_balanced == 0) f = named = Form::Soft;  // no balanced term
  if (f == Form::Soft && c->sp_soft == 0) f = named = Form::Prefs;        // no SCHEDULE_ANYWAY group, whatever w_spread is
  if (f == Form::Prefs && c->w_aff == 0 && c->w_taint == 0) {             // no preference term
    f = Form::Classes;
    if (host) named = Form::Classes;  // the host call reports as _classes; the device call keeps the _prefs_device name
  }
  // no classes in the call: _spread_scored's kernel under the name so far (never _spread_scored's own). Only here
  // does a class entry point reach a spread form, with the group column a spread form requires (seq_check).
  if (f == Form::Classes && !k.pod_class && k.pod_group) f = Form::SpreadScored;
  k.entry = entry_name(named, host);
  return f;
}

// What a grouped call needs, checked before any device work and before anything is written. One ordered list for
// all forms; a line that belongs to some forms only is guarded by the form:
//    1  null pointers: digit, tol, idx, status; the group column on the spread forms; the requests when nres > 0
//    2  negative p or max_pods_per_node
//    3  nres outside [0, MSH_MAX_RESOURCES]
//    4  below Soft: groups in the call (the spread forms: always) on a ctx with a SCHEDULE_ANYWAY group
//    5  the random tie-break
//    6  a score-column plugin list
//    7  Spread: a resource score on the ctx
//    8  no nodes
//    9  groups in the call and no zone column
//   10  Classes: classes in the call and no class column
//   11  no resource table, where requests, a resource score or Balanced need one
//   12  Balanced: a table of fewer than two resources; requests for fewer resources than the table's
//   13  requests for another number of resources than the table's
//   14  a resource score set for another number of resources than the call's
//   15  the form's table limit (the spread forms and Classes: the scored instance's with a resource score)
//   16  an amount above 2^55 in the table, with a resource score, then for Balanced
//   17  from Prefs on: classes in the call with neither column; the two columns with unequal C
//   18  from Prefs on: the key sum of the resource and preference weights; from Soft on: with the spread weight;
//       Balanced: with the balanced weight
//   19  Soft, and Balanced on a ctx with a SCHEDULE_ANYWAY group, with groups in the call: the count bound, p and
//       the soft groups' max_skew above MSH_SPREAD_SOFT_MAX
//   20  PodAffinity: no terms or no profiles
//   21  PodAffinity: a zone term and no zone column
//   22  PodAffinity: the launch's LDS, static and dynamic, above 64 KiB
// PodAffinity takes Balanced's lines; those of the balanced term itself (11, 12 and 16 in mode NONE) with a nonzero
// w_balanced only, 19 on a ctx with a SCHEDULE_ANYWAY group.
// No two of the forms order a pair of these differently, so the guards select lines and never reorder them.
int seq_check(msh_ctx* c, Form form, const SeqCall& k, bool host) {
  const bool spread = form <= Form::SpreadScored, keyed = form >= Form::Prefs, soft = form >= Form::Soft,
             affine = form == Form::PodAffinity, balanced = form == Form::Balanced || (affine && c->w_balanced > 0);
  const bool grouped = spread || k.pod_group != nullptr, classed = k.pod_class != nullptr;
  const int32_t p = k.p, nres = k.nres;
  const bool null_column = !k.pod_digit || !k.pod_tol || !k.out_idx || !k.out_status || (spread && !k.pod_group);
  if (p > 0 && (null_column || (nres > 0 && !k.pod_req)))
    return fail(c, MSH_ERR_INVALID, host ? "null host pointer" : "null device pointer");
  if (p < 0 || k.max_pods_per_node < 0) return fail(c, MSH_ERR_INVALID, "negative argument");
  if (nres < 0 || nres > MSH_MAX_RESOURCES) return fail(c, MSH_ERR_INVALID, "nres outside [0, MSH_MAX_RESOURCES]");
  // a SCHEDULE_ANYWAY group's pods would go through the hard filter anywhere but in the soft forms: an explicit
  // error, never a fallback
  if (!soft && grouped && c->sp_soft > 0)
    return fail(c, MSH_ERR_UNSUPPORTED,
                std::string(k.entry) + ": the ctx holds " + std::to_string(c->sp_soft) +
                    " SCHEDULE_ANYWAY spread group(s) (msh_set_spread_group_modes); a call with pod groups must be "
                    "msh_schedule_sequential_soft");
  if (int rc = refuse_random(c, k.entry); rc != MSH_OK) return rc;
  if (c->generic) return fail(c, MSH_ERR_UNSUPPORTED, "score-column plugins run on the batch entry points only");
  const bool scored = c->rs_mode != MSH_RESOURCE_SCORE_NONE;
  if (form == Form::Spread && scored)
    return fail(c, MSH_ERR_UNSUPPORTED,
                std::string(k.entry) + ": a resource score (msh_set_resource_score) together with topology spread is "
                                       "not implemented (MSH_RESOURCE_SCORE_NONE restores the unscored form)");
  if (!c->have_nodes) return fail(c, MSH_ERR_STATE, "msh_upload_nodes has not been called");
  if (grouped && !c->have_zone) return fail(c, MSH_ERR_STATE, "msh_upload_node_zones has not been called");
  if (form == Form::Classes && classed && !c->have_class)
    return fail(c, MSH_ERR_STATE, "msh_upload_node_class_bits has not been called");
  // the balanced score reads the table's first two resources in every resource score mode
  if ((balanced || nres || scored) && !c->have_res)
    return fail(c, MSH_ERR_STATE, "msh_upload_node_resources has not been called");
  if (balanced && c->nres < 2)
    return fail(c, MSH_ERR_STATE, "the balanced score needs a resource table with at least two resources, the "
                                  "table has " + std::to_string(c->nres));
  if (balanced && nres != c->nres)
    return fail(c, MSH_ERR_STATE, "the balanced score needs the requests of all " + std::to_string(c->nres) +
                                      " resources of the table, the call has " + std::to_string(nres));
  if (nres && nres != c->nres)
    return fail(c, MSH_ERR_INVALID, "requests for " + std::to_string(nres) + " resources against a table of " +
                                        std::to_string(c->nres));
  if (scored && nres != c->rs_nres)
    return fail(c, MSH_ERR_STATE, "msh_set_resource_score was given " + std::to_string(c->rs_nres) +
                                      " resources, the call has " + std::to_string(nres));
  int32_t lim = 0;
  const char* what = nullptr;
  switch (form) {
    case Form::Spread:
    case Form::SpreadScored:
      lim = scored ? msh::seq_spread_score_max_nodes(nres) : msh::seq_spread_max_nodes(nres);
      what = scored ? "scored topology-spread" : "topology-spread";
      break;
    case Form::Classes:
      lim = msh::seq_classes_max_nodes(nres, scored);
      what = scored ? "scored class-mask" : "class-mask";
      break;
    case Form::Prefs: lim = msh::seq_prefs_max_nodes(nres), what = "preference"; break;
    case Form::Soft: lim = msh::seq_soft_max_nodes(nres), what = "soft-spread"; break;
    case Form::Balanced: lim = msh::seq_balanced_max_nodes(nres), what = "balanced-allocation"; break;
    case Form::PodAffinity: lim = msh::seq_podaffinity_max_nodes(nres), what = "inter-pod affinity"; break;
  }
  if (c->n_nodes > lim) return fail(c, MSH_ERR_UNSUPPORTED, msh::seq_table_limit_message(what, lim, nres));
  if ((scored || balanced) && c->res_max > MSH_RESOURCE_SCORE_MAX)
    return fail(c, MSH_ERR_UNSUPPORTED,
                std::string(scored ? "a resource score" : "the balanced score") +
                    " needs every amount of the table within MSH_RESOURCE_SCORE_MAX = 2^55; an upload or patch wrote " +
                    std::to_string(c->res_max));
  if (!keyed) return MSH_OK;
  if (classed && !c->have_class && !c->have_prefs)
    return fail(c, MSH_ERR_STATE, "pod classes with neither msh_upload_node_class_prefs nor msh_upload_node_class_bits");
  if (classed && c->have_class && c->have_prefs && c->n_classes != c->pref_classes)
    return fail(c, MSH_ERR_STATE, "the class masks were uploaded for C = " + std::to_string(c->n_classes) +
                                      ", the preference values for C = " + std::to_string(c->pref_classes));
  // the weighted sums the packed key must hold: the shortest first, each form's own terms added
  const struct {
    bool applies;
    const char* terms;
    int32_t weight;
  } sums[] = {{true, "the resource score and the two preference scores", 0},
              {soft, "the resource score, the two preference scores and the spread score", c->w_spread},
              {balanced, "the resource score, the two preference scores, the spread score and the balanced score",
               c->w_balanced}};
  int64_t wsum = (scored ? c->rs_weight : 0) + c->w_aff + c->w_taint;
  for (const auto& s : sums) {
    if (!s.applies) break;
    wsum += s.weight;
    if (100 * wsum > 65534)
      return fail(c, MSH_ERR_UNSUPPORTED, std::string("the weights of ") + s.terms + " sum to " + std::to_string(wsum) +
                                              ": the packed key holds 100 x 655 at most");
  }
  // the counts' bounds belong to the soft groups' term: a balanced call on a ctx without one runs none of it
  if (soft && k.pod_group && (form == Form::Soft || c->sp_soft > 0)) {
    const char* above = ", above MSH_SPREAD_SOFT_MAX = 2^24";
    if (c->sp_cnt_bound > MSH_SPREAD_SOFT_MAX)
      return fail(c, MSH_ERR_UNSUPPORTED, "a spread count may have reached " + std::to_string(c->sp_cnt_bound) + above +
                                              " (msh_reset_spread_counts zeroes them)");
    if (p > MSH_SPREAD_SOFT_MAX)
      return fail(c, MSH_ERR_UNSUPPORTED, "a soft-spread call takes at most MSH_SPREAD_SOFT_MAX = 2^24 pods");
    for (int32_t g = 0; g < c->sp_groups; ++g)
      if (c->h_spmode[(size_t)g] == MSH_SPREAD_SCHEDULE_ANYWAY && c->h_skew[(size_t)g] > MSH_SPREAD_SOFT_MAX)
        return fail(c, MSH_ERR_UNSUPPORTED, "SCHEDULE_ANYWAY group " + std::to_string(g) + " has max_skew " +
                                                std::to_string(c->h_skew[(size_t)g]) + above);
  }
  if (!affine) return MSH_OK;
  if (c->pa_terms == 0)
    return fail(c, MSH_ERR_STATE, "pod profiles in the call and msh_set_pod_affinity_terms has not been called");
  if (c->pa_profiles == 0)
    return fail(c, MSH_ERR_STATE, "pod profiles in the call and msh_set_pod_profiles has not been called");
  if (c->pa_zone_mask != 0 && !c->have_zone)
    return fail(c, MSH_ERR_STATE,
                "an affinity term has the zone topology and msh_upload_node_zones has not been called");
  // the node words share the workgroup's LDS with the spread counts of the call's groups; no launch opts in to more
  // than the 64 KiB every kernel may have
  const int32_t G = k.pod_group ? c->sp_groups : 0;
  size_t each = 0;
  const size_t fixed = msh::seq_podaffinity_lds(nres, c->n_nodes, 0, &each);
  if (fixed + (size_t)G * each > msh::PODAFF_LDS_MAX)
    return fail(c, MSH_ERR_UNSUPPORTED,
                std::string(k.entry) + ": " + std::to_string(c->n_nodes) + " nodes with " + std::to_string(nres) +
                    " resources and " + std::to_string(G) + " spread groups need " +
                    std::to_string(fixed + (size_t)G * each) + " bytes of workgroup memory, above 65536: at most " +
                    std::to_string((msh::PODAFF_LDS_MAX - fixed) / each) + " spread groups fit at this table size");
  return MSH_OK;
}

// The argument block every grouped kernel starts from, for the ctx as it stands (the class forms: a null pod_group
// goes with no groups, and the zone column may be absent).
void spread_args(msh_ctx* c, const SeqCall& k, msh::SpreadArgs& sa) {
  msh::SeqArgs& a = sa.f.s;
  seq_args_fill(c, a, k.p, k.pod_digit, k.pod_tol, k.out_idx, k.out_score, k.out_status);
  // the pod count limit as the resource-fit form takes it: the column and / or the scalar, or none
  a.max_pods = k.max_pods_per_node == 0 ? INT32_MAX : k.max_pods_per_node;
  a.fold = c->counts_dirty ? 1 : 0;
  sa.f.nres = k.nres;
  sa.f.res_stride = (int64_t)c->res_cap;
  sa.f.alloc = k.nres ? c->d_alloc : nullptr;
  sa.f.used = k.nres ? c->d_used : nullptr;
  sa.f.pod_req = k.nres ? k.pod_req : nullptr;
  sa.zone = c->have_zone ? c->d_zone : nullptr;
  sa.pod_group = k.pod_group;
  sa.n_groups = k.pod_group ? c->sp_groups : 0;
  sa.max_skew = c->d_skew;
  sa.cnt = c->d_spread_cnt;
  sa.zset = c->have_zone ? c->zset : 0;
}

// The device path: `form` resolved, k's pointers device-visible. Asynchronous on `stream`.
int seq_launch(msh_ctx* c, Form form, const SeqCall& k, void* stream) {
  c->err.clear();
  int rc = seq_check(c, form, k, false);
  if (rc != MSH_OK) return rc;
  if (k.p == 0) return MSH_OK;
  DeviceGuard g(c->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool scored = c->rs_mode != MSH_RESOURCE_SCORE_NONE;  // never on Form::Spread: seq_check refused it
  static_assert(msh::SPREAD_SOFT_MAX == MSH_SPREAD_SOFT_MAX, "the kernel's bound is the header's");
  if (form >= Form::Prefs) {  // what the form reads besides the ctx's columns (synchronous, before the block is filled)
    const int32_t npl = form == Form::PodAffinity ? msh::seq_podaffinity_npl(k.nres)
                        : form == Form::Balanced  ? msh::seq_balanced_npl(k.nres)
                        : form == Form::Soft      ? msh::seq_soft_npl(k.nres)
                                                  : msh::seq_prefs_npl(k.nres);
    if (k.pod_class && (rc = prefs_table(c, npl)) != MSH_OK) return rc;
    if (form >= Form::Soft && (form == Form::Soft || c->sp_soft > 0) && (rc = soft_weights_device(c)) != MSH_OK) return rc;
    if (form == Form::PodAffinity && (rc = pa_state_ready(c)) != MSH_OK) return rc;
  }
  // The blocks nest (PodAffinityArgs > BalancedArgs > SoftArgs > PrefArgs > SpreadScoreArgs > SpreadArgs): the
  // innermost two are what the spread and class forms take. Unscored: weight 0, every resource weight 0 and the
  // magic 0, so rs = 0.
  msh::PodAffinityArgs pq{};
  msh::BalancedArgs& ba = pq.ba;
  msh::SoftArgs& so = ba.so;
  msh::PrefArgs& pa = so.p;
  msh::SpreadScoreArgs& ss = pa.ss;
  spread_args(c, k, ss.s);
  if (scored) resource_score_setting(c, k.nres, ss);
  if ((rc = seq_serialize(c, s)) != MSH_OK) return rc;
  std::string err;
  hipError_t e = hipSuccess;
  const char* kernel = nullptr;
  {
    TimedLaunch tl(c);
    switch (form) {
      case Form::Spread:
      case Form::SpreadScored:
        kernel = scored ? "seq_spread_score_kernel" : "seq_spread_kernel";
        e = scored ? msh::launch_seq_spread_score(ss, s, &err) : msh::launch_seq_spread(ss.s, s, &err);
        break;
      case Form::Classes: {
        msh::ClassArgs ca{};
        ca.ss = ss;
        ca.class_bits = k.pod_class ? c->d_class : nullptr;
        ca.pod_class = k.pod_class;
        ca.n_classes = k.pod_class ? c->n_classes : 0;
        kernel = scored ? "seq_classes_score_kernel" : "seq_classes_kernel";
        e = msh::launch_seq_classes(ca, scored, s, &err);
        break;
      }
      case Form::Prefs:
      case Form::Soft:
      case Form::Balanced:
      case Form::PodAffinity:
        pa.rows = k.pod_class ? c->d_pref : nullptr;
        pa.pod_class = k.pod_class;
        pa.n_classes = k.pod_class ? c->pref_dev_classes : 0;
        pa.amask = k.pod_class ? c->pref_amask : 0;
        pa.tmask = k.pod_class ? c->pref_tmask : 0;
        pa.w_aff = (uint32_t)c->w_aff;
        pa.w_taint = (uint32_t)c->w_taint;
        if (form == Form::Prefs) {
          kernel = "seq_prefs_kernel";
          e = msh::launch_seq_prefs(pa, s, &err);
          break;
        }
        for (int32_t g2 = 0; k.pod_group && g2 < c->sp_groups; ++g2)
          if (c->h_spmode[(size_t)g2] == MSH_SPREAD_SCHEDULE_ANYWAY) so.soft[g2 >> 6] |= uint64_t(1) << (g2 & 63);
        so.w_spread = (uint32_t)c->w_spread;
        so.zone_weight = c->d_zone_weight;
        ba.w_balanced = (uint32_t)c->w_balanced;
        if (form == Form::PodAffinity) {
          pq.state = c->d_pa_state;
          pq.pod_profile = k.pod_profile;
          pq.profiles = c->d_pa_prof;
          pq.n_profiles = c->pa_profiles;
          pq.host_mask = c->pa_host_mask;
          pq.zone_mask = c->pa_zone_mask;
          kernel = "seq_podaffinity_kernel";
          e = msh::launch_seq_podaffinity(pq, s, &err);
          break;
        }
        kernel = form == Form::Balanced ? "seq_balanced_kernel" : "seq_soft_kernel";
        e = form == Form::Balanced ? msh::launch_seq_balanced(ba, s, &err) : msh::launch_seq_soft(so, s, &err);
        break;
    }
  }
  if (e != hipSuccess) {
    if (!err.empty()) return fail(c, MSH_ERR_UNSUPPORTED, err);
    return hip_fail(c, e, kernel);
  }
  c->counts_dirty = false;               // the one workgroup folded the replicas
  if (k.pod_group) c->sp_cnt_bound += k.p;  // each pod may have raised one count by one
  return track_launch(c, s, true);
}

int seq_grouped_device(msh_ctx* c, Form asked, SeqCall k, void* stream) {
  const Form form = seq_resolve(asked, c, k, false);
  return seq_launch(c, form, k, stream);
}

// The host path: validation of what a device call cannot see (the groups, classes and requests themselves), the
// columns through page-locked memory, seq_launch on the ctx's stream, the outputs back, the commit callbacks.
int seq_grouped_host(msh_ctx* c, Form asked, SeqCall k, msh_commit_cb commit_cb, void* user) {
  const Form form = seq_resolve(asked, c, k, true);
  c->err.clear();
  int rc = seq_check(c, form, k, true);
  if (rc != MSH_OK) return rc;
  const int32_t p = k.p;
  for (int32_t j = 0; k.pod_group && j < p; ++j)
    if (k.pod_group[j] < -1 || k.pod_group[j] >= c->sp_groups)
      return fail(c, MSH_ERR_INVALID, "pod " + std::to_string(j) + ": group " + std::to_string(k.pod_group[j]) +
                                          " outside [-1, G) with G = " + std::to_string(c->sp_groups));
  // _classes reads the mask column alone; the forms above it the columns' common C
  const int32_t C = form == Form::Classes ? c->n_classes : prefs_classes(c);
  for (int32_t j = 0; k.pod_class && j < p; ++j)
    if (k.pod_class[j] < -1 || k.pod_class[j] >= C)
      return fail(c, MSH_ERR_INVALID, "pod " + std::to_string(j) + ": class " + std::to_string(k.pod_class[j]) +
                                          " outside [-1, C) with C = " + std::to_string(C));
  for (int32_t j = 0; form == Form::PodAffinity && j < p; ++j)
    if (k.pod_profile[j] < -1 || k.pod_profile[j] >= c->pa_profiles)
      return fail(c, MSH_ERR_INVALID, "pod " + std::to_string(j) + ": profile " + std::to_string(k.pod_profile[j]) +
                                          " outside [-1, Q) with Q = " + std::to_string(c->pa_profiles));
  const bool balanced = form == Form::Balanced || (form == Form::PodAffinity && c->w_balanced > 0);
  if ((rc = check_requests(c, k.nres, p, k.pod_req, c->rs_mode != MSH_RESOURCE_SCORE_NONE, balanced)) != MSH_OK)
    return rc;
  if (p == 0) return MSH_OK;
  DeviceGuard g(c->device);
  HostIO io;
  if ((rc = host_io_begin(c, p, k.pod_digit, k.pod_tol, k.out_idx, k.out_score, k.out_status, io)) != MSH_OK) return rc;
  // the requests, the groups and (outside the spread forms, which have none) the classes and the profiles through the
  // page-locked node stage, which the kernel reads itself (free here: every writer that uses it has finished its
  // copies, and this call ends only when the kernel has)
  const size_t rbytes = (size_t)k.nres * (size_t)p * sizeof(int64_t), cbytes = (size_t)p * sizeof(int32_t);
  if ((rc = node_stage(c, rbytes + (form <= Form::SpreadScored ? 1 : 3) * cbytes)) != MSH_OK) return rc;
  int32_t* sg = reinterpret_cast<int32_t*>(c->h_nstage + rbytes);
  int32_t* sc = reinterpret_cast<int32_t*>(c->h_nstage + rbytes + cbytes);
  if (rbytes) std::memcpy(c->h_nstage, k.pod_req, rbytes);
  if (k.pod_group) std::memcpy(sg, k.pod_group, cbytes);
  int32_t* sq = reinterpret_cast<int32_t*>(c->h_nstage + rbytes + 2 * cbytes);
  if (k.pod_class) std::memcpy(sc, k.pod_class, cbytes);
  if (k.pod_profile) std::memcpy(sq, k.pod_profile, cbytes);
  const SeqCall d{p, io.d_pd, io.d_pt, k.pod_group ? sg : nullptr, k.pod_class ? sc : nullptr, k.nres,
                  reinterpret_cast<const int64_t*>(c->h_nstage), k.max_pods_per_node, io.o_idx, io.o_score, io.o_status,
                  k.entry, k.pod_profile ? sq : nullptr};
  if ((rc = seq_launch(c, form, d, c->stream)) != MSH_OK) return rc;
  if ((rc = host_io_end(c, p, k.out_idx, k.out_score, k.out_status, io)) != MSH_OK) return rc;
  commit_callbacks(commit_cb, user, p, k.out_idx, k.out_score, k.out_status);
  return MSH_OK;
}
}  // namespace

int msh_schedule_sequential_spread_device(msh_ctx* c, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                          const int32_t* d_pod_group, int32_t nres, const int64_t* d_pod_req,
                                          int32_t max_pods_per_node, int32_t* d_out_idx, int64_t* d_out_score,
                                          int32_t* d_out_status, void* stream) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, d_pod_digit, d_pod_tol, d_pod_group, nullptr, nres, d_pod_req, max_pods_per_node,
                  d_out_idx, d_out_score, d_out_status};
  return seq_grouped_device(c, Form::Spread, k, stream);
}

int msh_schedule_sequential_spread(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                   const int32_t* pod_group, int32_t nres, const int64_t* pod_req,
                                   int32_t max_pods_per_node, int32_t* out_idx, int64_t* out_score,
                                   int32_t* out_status, msh_commit_cb commit_cb, void* user) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, pod_digit, pod_tol, pod_group, nullptr, nres, pod_req, max_pods_per_node,
                  out_idx, out_score, out_status};
  return seq_grouped_host(c, Form::Spread, k, commit_cb, user);
}

int msh_schedule_sequential_spread_scored_device(msh_ctx* c, int32_t p, const int8_t* d_pod_digit,
                                                 const uint8_t* d_pod_tol, const int32_t* d_pod_group, int32_t nres,
                                                 const int64_t* d_pod_req, int32_t max_pods_per_node,
                                                 int32_t* d_out_idx, int64_t* d_out_score, int32_t* d_out_status,
                                                 void* stream) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, d_pod_digit, d_pod_tol, d_pod_group, nullptr, nres, d_pod_req, max_pods_per_node,
                  d_out_idx, d_out_score, d_out_status};
  return seq_grouped_device(c, Form::SpreadScored, k, stream);
}

int msh_schedule_sequential_spread_scored(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                          const int32_t* pod_group, int32_t nres, const int64_t* pod_req,
                                          int32_t max_pods_per_node, int32_t* out_idx, int64_t* out_score,
                                          int32_t* out_status, msh_commit_cb commit_cb, void* user) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, pod_digit, pod_tol, pod_group, nullptr, nres, pod_req, max_pods_per_node,
                  out_idx, out_score, out_status};
  return seq_grouped_host(c, Form::SpreadScored, k, commit_cb, user);
}

int msh_schedule_sequential_classes_device(msh_ctx* c, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                           const int32_t* d_pod_group, const int32_t* d_pod_class, int32_t nres,
                                           const int64_t* d_pod_req, int32_t max_pods_per_node, int32_t* d_out_idx,
                                           int64_t* d_out_score, int32_t* d_out_status, void* stream) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, d_pod_digit, d_pod_tol, d_pod_group, d_pod_class, nres, d_pod_req, max_pods_per_node,
                  d_out_idx, d_out_score, d_out_status};
  return seq_grouped_device(c, Form::Classes, k, stream);
}

int msh_schedule_sequential_classes(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                    const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                    const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                    int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, pod_digit, pod_tol, pod_group, pod_class, nres, pod_req, max_pods_per_node,
                  out_idx, out_score, out_status};
  return seq_grouped_host(c, Form::Classes, k, commit_cb, user);
}

int msh_schedule_sequential_prefs_device(msh_ctx* c, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                         const int32_t* d_pod_group, const int32_t* d_pod_class, int32_t nres,
                                         const int64_t* d_pod_req, int32_t max_pods_per_node, int32_t* d_out_idx,
                                         int64_t* d_out_score, int32_t* d_out_status, void* stream) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, d_pod_digit, d_pod_tol, d_pod_group, d_pod_class, nres, d_pod_req, max_pods_per_node,
                  d_out_idx, d_out_score, d_out_status};
  return seq_grouped_device(c, Form::Prefs, k, stream);
}

int msh_schedule_sequential_prefs(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                  const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                  const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                  int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, pod_digit, pod_tol, pod_group, pod_class, nres, pod_req, max_pods_per_node,
                  out_idx, out_score, out_status};
  return seq_grouped_host(c, Form::Prefs, k, commit_cb, user);
}

int msh_schedule_sequential_soft_device(msh_ctx* c, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                        const int32_t* d_pod_group, const int32_t* d_pod_class, int32_t nres,
                                        const int64_t* d_pod_req, int32_t max_pods_per_node, int32_t* d_out_idx,
                                        int64_t* d_out_score, int32_t* d_out_status, void* stream) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, d_pod_digit, d_pod_tol, d_pod_group, d_pod_class, nres, d_pod_req, max_pods_per_node,
                  d_out_idx, d_out_score, d_out_status};
  return seq_grouped_device(c, Form::Soft, k, stream);
}

int msh_schedule_sequential_soft(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                 const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                 const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                 int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, pod_digit, pod_tol, pod_group, pod_class, nres, pod_req, max_pods_per_node,
                  out_idx, out_score, out_status};
  return seq_grouped_host(c, Form::Soft, k, commit_cb, user);
}

int msh_schedule_sequential_balanced_device(msh_ctx* c, int32_t p, const int8_t* d_pod_digit, const uint8_t* d_pod_tol,
                                            const int32_t* d_pod_group, const int32_t* d_pod_class, int32_t nres,
                                            const int64_t* d_pod_req, int32_t max_pods_per_node, int32_t* d_out_idx,
                                            int64_t* d_out_score, int32_t* d_out_status, void* stream) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, d_pod_digit, d_pod_tol, d_pod_group, d_pod_class, nres, d_pod_req, max_pods_per_node,
                  d_out_idx, d_out_score, d_out_status};
  return seq_grouped_device(c, Form::Balanced, k, stream);
}

int msh_schedule_sequential_balanced(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                     const int32_t* pod_group, const int32_t* pod_class, int32_t nres,
                                     const int64_t* pod_req, int32_t max_pods_per_node, int32_t* out_idx,
                                     int64_t* out_score, int32_t* out_status, msh_commit_cb commit_cb, void* user) {
  if (!c) return MSH_ERR_INVALID;
  const SeqCall k{p, pod_digit, pod_tol, pod_group, pod_class, nres, pod_req, max_pods_per_node,
                  out_idx, out_score, out_status};
  return seq_grouped_host(c, Form::Balanced, k, commit_cb, user);
}

int msh_schedule_sequential_podaffinity_device(msh_ctx* c, int32_t p, const int8_t* d_pod_digit,
                                               const uint8_t* d_pod_tol, const int32_t* d_pod_group, const int32_t* d_pod_class,
                                               const int32_t* d_pod_profile, int32_t nres, const int64_t* d_pod_req,
                                               int32_t max_pods_per_node, int32_t* d_out_idx, int64_t* d_out_score,
                                               int32_t* d_out_status, void* stream) {
  if (!c) return MSH_ERR_INVALID;
  SeqCall k{p, d_pod_digit, d_pod_tol, d_pod_group, d_pod_class, nres, d_pod_req, max_pods_per_node,
            d_out_idx, d_out_score, d_out_status};
  k.pod_profile = d_pod_profile;
  return seq_grouped_device(c, Form::PodAffinity, k, stream);
}

int msh_schedule_sequential_podaffinity(msh_ctx* c, int32_t p, const int8_t* pod_digit, const uint8_t* pod_tol,
                                        const int32_t* pod_group, const int32_t* pod_class, const int32_t* pod_profile,
                                        int32_t nres, const int64_t* pod_req, int32_t max_pods_per_node,
                                        int32_t* out_idx, int64_t* out_score, int32_t* out_status,
                                        msh_commit_cb commit_cb, void* user) {
  if (!c) return MSH_ERR_INVALID;
  SeqCall k{p, pod_digit, pod_tol, pod_group, pod_class, nres, pod_req, max_pods_per_node,
            out_idx, out_score, out_status};
  k.pod_profile = pod_profile;
  return seq_grouped_host(c, Form::PodAffinity, k, commit_cb, user);
}
