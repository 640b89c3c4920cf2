"""Host-side mirror of minisched.Scheduler's selection path, driving the gfx950 device path.

Reference (shopetan/mini-kube-scheduler, Go):
  Scheduler struct + plugin lists   minisched/initialize.go:18-29, :80-123
  scheduleOne (selection part)      minisched/minisched.go:32-87
  RunFilterPlugins / RunPreScorePlugins / RunScorePlugins / selectHost
                                    minisched/minisched.go:115-199, :304-325
  ErrorFunc routing                 minisched/minisched.go:283-298

`DeviceContext` wraps one msh_ctx (one GPU). `Scheduler` keeps the reference's plugin
configuration by plugin *name* (framework.Plugin.Name()), maps the names the device path
implements to device ids, and schedules a whole batch of pods in one call. Unknown plugin
names raise MshError(MSH_ERR_UNSUPPORTED): there is no silent host fallback.
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Any, Callable, Iterable, Mapping, Sequence

import numpy as np

from . import _native as N
from . import constraints as K
from .framework import (NODE_NUMBER, NODE_UNSCHEDULABLE, SCORE_COLUMNS, Normalize, Outcome, ScheduleResult)
from .snapshot import NodeTable, PodTable, _get, _tol_field, node_allocatable, pack_nodes, pack_pods, pod_requests

FILTER_IDS = {NODE_UNSCHEDULABLE: N.MSH_PLUGIN_NODE_UNSCHEDULABLE}
SCORE_IDS = {NODE_NUMBER: N.MSH_PLUGIN_NODE_NUMBER,
             **{name: N.MSH_PLUGIN_SCORE_COLUMN0 + k for k, name in enumerate(SCORE_COLUMNS)}}
# Only NodeNumber implements PreScore (nodenumber.go:50-64); a score column has none, so naming one in
# the prescore list is MSH_ERR_UNSUPPORTED here exactly as in msh_set_plugins_ex.
PRESCORE_IDS = {NODE_NUMBER: N.MSH_PLUGIN_NODE_NUMBER}
# msh_tiebreak by name and by value (DeviceContext.set_tiebreak, Scheduler(tie_break=...))
TIEBREAK_MODES = {"first": N.MSH_TIEBREAK_FIRST, "random": N.MSH_TIEBREAK_RANDOM,
                  N.MSH_TIEBREAK_FIRST: N.MSH_TIEBREAK_FIRST, N.MSH_TIEBREAK_RANDOM: N.MSH_TIEBREAK_RANDOM}
# msh_resource_score by name and by value (DeviceContext.set_resource_score, Scheduler(resource_score=...))
RESOURCE_SCORE_MODES = {"none": N.MSH_RESOURCE_SCORE_NONE, "least": N.MSH_RESOURCE_SCORE_LEAST_ALLOCATED,
                        "most": N.MSH_RESOURCE_SCORE_MOST_ALLOCATED,
                        **{v: v for v in (N.MSH_RESOURCE_SCORE_NONE, N.MSH_RESOURCE_SCORE_LEAST_ALLOCATED,
                                          N.MSH_RESOURCE_SCORE_MOST_ALLOCATED)}}
_U64 = (1 << 64) - 1


@dataclass(frozen=True)
class ScorePluginConfig:
    name: str
    weight: int = 1
    normalize: Normalize = Normalize.NONE


def pinned_empty(shape, dtype) -> np.ndarray:
    """A numpy array over page-locked host memory (msh_host_alloc): pod columns and outputs in
    such arrays take the zero-copy path of msh_schedule_batch / msh_schedule_sequential. The
    memory is freed (msh_host_free) when the array and every view of it are gone."""
    dt = np.dtype(dtype)
    nbytes = max(int(np.prod(shape, dtype=np.int64)) * dt.itemsize, 1)
    lib = N.lib()
    ptr = C.c_void_p()
    N.check(lib.msh_host_alloc(nbytes, C.byref(ptr)))
    raw = (C.c_uint8 * nbytes).from_address(ptr.value)
    weakref.finalize(raw, lib.msh_host_free, ptr)
    return np.frombuffer(raw, np.uint8, count=int(np.prod(shape, dtype=np.int64)) * dt.itemsize).view(dt).reshape(shape)


def _same_len(what: str, *arrays) -> int:
    n = len(arrays[0])
    if any(len(a) != n for a in arrays[1:]):
        raise ValueError(f"{what}: column length mismatch {[len(a) for a in arrays]}")
    return n


def _ids(names: Sequence[str], table: dict, what: str) -> np.ndarray:
    out = []
    for n in names:
        if n not in table:
            raise N.MshError(N.MSH_ERR_UNSUPPORTED, f"{what} plugin {n!r} has no device implementation")
        out.append(table[n])
    return np.array(out, np.int32)


class DeviceContext:
    """One msh_ctx bound to one HIP device.

    `options` (tests and A/B measurement only): msh_options overrides for msh_create_ex, e.g.
    {"batch_kernel": "generic", "seq_waves": 16, "seq_split": "serial"} (names in _native.OPTION_NAMES,
    ints as they are; a value outside a field's set is MSH_ERR_INVALID from the library)."""

    def __init__(self, device: int = 0, options: dict | None = None):
        self._lib = N.lib()
        self._fast = N.fast()
        h = C.c_void_p()
        opts = N.make_options(options)
        if opts is None:
            rc = self._lib.msh_create(device, C.byref(h))
        else:
            rc = self._lib.msh_create_ex(device, C.byref(opts), C.byref(h))
        if rc != N.MSH_OK:
            raw = self._lib.msh_last_error(None)
            raise N.MshError(rc, raw.decode() if raw else "")
        self.handle = h
        self.device = device
        self.n_nodes = 0

    # -- lifecycle --
    def close(self) -> None:
        if self.handle:
            self._lib.msh_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        N.check(rc, self.handle)

    def _hv(self):
        """The ctx handle as an int for the fast-call module (None once closed: MSH_ERR_INVALID)."""
        return self.handle.value if self.handle else None

    # -- configuration --
    def set_plugins(self, filters: Sequence[str], prescore: Sequence[str],
                    score: Sequence[ScorePluginConfig]) -> None:
        f = _ids(filters, FILTER_IDS, "filter")
        pre = _ids(prescore, PRESCORE_IDS, "prescore")
        s = _ids([c.name for c in score], SCORE_IDS, "score")
        w = np.array([int(c.weight) for c in score], np.int64)
        nm = np.array([int(c.normalize) for c in score], np.int32)
        self._check(self._lib.msh_set_plugins_ex(self.handle, N.ptr(f), len(f), N.ptr(pre), len(pre),
                                                 N.ptr(s), N.ptr(w), N.ptr(nm), len(s)))

    def set_tiebreak(self, mode, seed: int = 0, counter: int = 0) -> None:
        """msh_set_tiebreak: "first" (the first maximum in List order, the default) or "random" (a
        uniform choice among the maxima, drawn from SplitMix64(seed) at counter + the pod's position;
        the counter advances by p per batch call). The integers MSH_TIEBREAK_* pass too."""
        m = TIEBREAK_MODES.get(mode) if isinstance(mode, (str, int)) and not isinstance(mode, bool) else None
        if m is None:
            raise N.MshError(N.MSH_ERR_INVALID, f"tie-break mode {mode!r}: not 'first' (0) or 'random' (1)")
        self._check(self._lib.msh_set_tiebreak(self.handle, m, int(seed) & _U64, int(counter) & _U64))

    def tiebreak(self) -> tuple[int, int, int]:
        """msh_get_tiebreak: (mode, seed, counter), the counter where the next batch's first pod draws."""
        m, s, c = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.msh_get_tiebreak(self.handle, C.byref(m), C.byref(s), C.byref(c)))
        return m.value, s.value, c.value

    def upload_nodes(self, unsched: np.ndarray, digit: np.ndarray) -> None:
        unsched = np.ascontiguousarray(unsched, np.uint8)
        digit = np.ascontiguousarray(digit, np.int8)
        n = _same_len("upload_nodes", unsched, digit)
        self._check(self._lib.msh_upload_nodes(self.handle, n, N.ptr(unsched), N.ptr(digit)))
        self.n_nodes = len(unsched)

    def upload_score_column(self, name: str, scores: np.ndarray) -> None:
        """msh_upload_score_column: the per-node int64 scores (List order) of score-column plugin
        `name` ("ScoreColumn0".."ScoreColumn3")."""
        if name not in SCORE_COLUMNS:
            raise ValueError(f"{name!r} is not a score-column plugin")
        scores = np.ascontiguousarray(scores, np.int64)
        self._check(self._lib.msh_upload_score_column(self.handle, SCORE_IDS[name], len(scores), N.ptr(scores)))

    def patch_nodes(self, idx: np.ndarray, unsched: np.ndarray, digit: np.ndarray) -> None:
        """In-place update of table entries (List order unchanged): msh_patch_nodes."""
        idx = np.ascontiguousarray(idx, np.int32)
        unsched = np.ascontiguousarray(unsched, np.uint8)
        digit = np.ascontiguousarray(digit, np.int8)
        if not (len(idx) == len(unsched) == len(digit)):
            raise ValueError("idx / unsched / digit length mismatch")
        self._check(self._lib.msh_patch_nodes(self.handle, len(idx), N.ptr(idx), N.ptr(unsched), N.ptr(digit)))

    def export_results(self, pod_digit: np.ndarray, pod_tol: np.ndarray):
        """Per-pair plugin results [p, n]: (filter uint8, raw score int64, final score int64);
        scores are N.MSH_EXPORT_NONE where none is recorded (msh_export_results)."""
        pod_digit = np.ascontiguousarray(pod_digit, np.int8)
        pod_tol = np.ascontiguousarray(pod_tol, np.uint8)
        p, n = _same_len("export_results", pod_digit, pod_tol), int(self.n_nodes)
        filt = np.empty((p, n), np.uint8)
        raw = np.empty((p, n), np.int64)
        fin = np.empty((p, n), np.int64)
        self._check(self._lib.msh_export_results(self.handle, p, N.ptr(pod_digit), N.ptr(pod_tol),
                                                 N.ptr(filt), N.ptr(raw), N.ptr(fin)))
        return filt, raw, fin

    # -- host-buffer entry points --
    @staticmethod
    def _outputs(p: int, out, scores: bool = True):
        if out is None:
            return np.empty(p, np.int32), (np.empty(p, np.int64) if scores else None), np.empty(p, np.int32)
        idx, score, status = out
        if not scores:
            score = None
        for a, dt in ((idx, np.int32), (score, np.int64), (status, np.int32)):
            if a is None and dt is np.int64:
                continue
            if a.dtype != dt or len(a) < p or not a.flags["C_CONTIGUOUS"]:
                raise ValueError("out: (int32 idx, int64 score or None, int32 status), C-contiguous, >= p entries")
        return idx, score, status

    def schedule_batch(self, pod_digit: np.ndarray, pod_tol: np.ndarray, out=None, scores: bool = True):
        """msh_schedule_batch. `out` = (idx, score, status) arrays to fill (e.g. pinned_empty ones:
        with page-locked columns and outputs the call copies nothing on the host). scores=False
        (or out with score None): scores are not written and (idx, None, status) comes back."""
        pod_digit = np.ascontiguousarray(pod_digit, np.int8)
        pod_tol = np.ascontiguousarray(pod_tol, np.uint8)
        p = _same_len("schedule_batch", pod_digit, pod_tol)
        idx, score, status = self._outputs(p, out, scores)
        rc = self._fast.schedule_batch_host(self._hv(), pod_digit, pod_tol, idx, score, status)
        if rc:
            self._check(rc)
        return idx, score, status

    def schedule_batch_async(self, pod_digit: np.ndarray, pod_tol: np.ndarray, out, scores: bool = True) -> int:
        """msh_schedule_batch_async: page-locked columns and outputs (pinned_empty arrays) only; returns
        the ticket. The outputs are valid after wait(ticket); keep every array alive and untouched
        until then."""
        p = _same_len("schedule_batch_async", pod_digit, pod_tol)
        idx, score, status = self._outputs(p, out, scores)
        rc, ticket = self._fast.schedule_batch_host_async(self._hv(), pod_digit, pod_tol, idx, score, status)
        if rc:
            self._check(rc)
        return ticket

    def wait(self, ticket: int) -> None:
        """msh_wait: batch `ticket` of schedule_batch_async (and every earlier one) has completed."""
        rc = self._fast.wait(self._hv(), int(ticket))
        if rc:
            self._check(rc)

    def timing_begin(self, max_launches: int) -> None:
        """msh_timing_begin: the next hot-kernel launches of this ctx (from this thread) record their
        own start / stop (the kernel-trace interval)."""
        self._check(self._lib.msh_timing_begin(self.handle, int(max_launches)))

    def timing_end(self) -> tuple[int, float, float]:
        """msh_timing_end: (launches timed, summed ms, longest ms)."""
        n, tot, mx = C.c_int32(), C.c_double(), C.c_double()
        self._check(self._lib.msh_timing_end(self.handle, C.byref(n), C.byref(tot), C.byref(mx)))
        return n.value, tot.value, mx.value

    def schedule_sequential(self, pod_digit: np.ndarray, pod_tol: np.ndarray, max_pods_per_node: int = 0,
                            on_commit: Callable[[int, int, int], None] | None = None, out=None):
        pod_digit = np.ascontiguousarray(pod_digit, np.int8)
        pod_tol = np.ascontiguousarray(pod_tol, np.uint8)
        p = _same_len("schedule_sequential", pod_digit, pod_tol)
        idx, score, status = self._outputs(p, out)
        cb = N.COMMIT_CB(lambda _u, j, i, s: on_commit(j, i, s)) if on_commit else N.COMMIT_CB()
        self._check(self._lib.msh_schedule_sequential(self.handle, p, N.ptr(pod_digit), N.ptr(pod_tol),
                                                      int(max_pods_per_node), N.ptr(idx), N.ptr(score),
                                                      N.ptr(status), cb, None))
        return idx, score, status

    def node_pod_counts(self) -> np.ndarray:
        out = np.zeros(self.n_nodes, np.int32)
        self._check(self._lib.msh_node_pod_counts(self.handle, N.ptr(out) if self.n_nodes else None))
        return out

    def reset_node_pod_counts(self) -> None:
        self._check(self._lib.msh_reset_node_pod_counts(self.handle))

    # -- per-node pod capacity for sequential mode (a node's status.allocatable.pods) --
    @staticmethod
    def _capacities(cap) -> np.ndarray:
        a = np.asarray(cap)
        if a.size and (a.dtype.kind not in "iu" or a.min() < -N.INT32_MAX - 1 or a.max() > N.INT32_MAX):
            raise ValueError("capacities are integers within int32")
        return np.ascontiguousarray(a, np.int32)

    def upload_node_capacity(self, cap) -> None:
        """msh_upload_node_capacity: one int32 per uploaded node, List order, 0 <= cap <= INT32_MAX (0: the
        node never takes a pod; INT32_MAX: in effect unlimited). With a column the sequential calls stop at
        min(cap[i], max_pods_per_node) per node (the column alone for max_pods_per_node = 0), always in the
        in-order capacity form. upload_nodes drops the column; patch_nodes and reset_node_pod_counts keep it;
        the batch entry points ignore it."""
        cap = self._capacities(cap)
        self._check(self._lib.msh_upload_node_capacity(self.handle, len(cap), N.ptr(cap)))

    def patch_node_capacity(self, idx, cap) -> None:
        """msh_patch_node_capacity: cap[k] replaces node idx[k]'s capacity (distinct indices within the table;
        a column must be present). No table rebuild."""
        idx = np.ascontiguousarray(idx, np.int32)
        cap = self._capacities(cap)
        if len(idx) != len(cap):
            raise ValueError("idx / cap length mismatch")
        self._check(self._lib.msh_patch_node_capacity(self.handle, len(idx), N.ptr(idx), N.ptr(cap)))

    def clear_node_capacity(self) -> None:
        """msh_clear_node_capacity: back to "no column"."""
        self._check(self._lib.msh_clear_node_capacity(self.handle))

    def node_capacity(self) -> np.ndarray | None:
        """msh_node_capacity: the column (int32, List order), or None when no column is present."""
        present = C.c_int32(0)
        out = np.zeros(self.n_nodes, np.int32)
        self._check(self._lib.msh_node_capacity(self.handle, N.ptr(out) if self.n_nodes else None, C.byref(present)))
        return out if present.value else None

    # -- resource requests for sequential mode (NodeResourcesFit: allocatable, used, requests) --
    @staticmethod
    def _amounts(a, ndim: int = 2) -> np.ndarray:
        a = np.asarray(a)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("resource amounts are integers")
        if a.ndim != ndim:
            raise ValueError(f"resource amounts are shaped (nres, n): got {a.shape}")
        if a.size and (int(a.min()) < -(1 << 63) or int(a.max()) >= (1 << 63)):
            raise ValueError("resource amounts are within int64")
        return np.ascontiguousarray(a, np.int64)

    def upload_node_resources(self, alloc, used=None) -> None:
        """msh_upload_node_resources: alloc (and used, default zeros) shaped (nres, n), int64 in [0, 2^62], List
        order. upload_nodes drops the table; patch_nodes and reset_node_pod_counts keep it; only
        schedule_sequential_fit reads it and commits to used."""
        alloc = self._amounts(alloc)
        if used is not None:
            used = self._amounts(used)
            if used.shape != alloc.shape:
                raise ValueError("alloc / used shape mismatch")
        nres, n = alloc.shape
        self._check(self._lib.msh_upload_node_resources(self.handle, n, nres, N.ptr(alloc), N.ptr(used)))

    def patch_node_resources(self, idx, alloc=None, used=None) -> None:
        """msh_patch_node_resources: alloc[:, k] / used[:, k] (shaped (nres, len(idx)); None keeps that array)
        replace node idx[k]'s values. A patch of used accounts for a deleted pod, or for pods bound elsewhere."""
        idx = np.ascontiguousarray(idx, np.int32)
        alloc = None if alloc is None else self._amounts(alloc)
        used = None if used is None else self._amounts(used)
        for a in (alloc, used):
            if a is not None and a.shape[1] != len(idx):
                raise ValueError("idx / values length mismatch")
        self._check(self._lib.msh_patch_node_resources(self.handle, len(idx), N.ptr(idx), N.ptr(alloc), N.ptr(used)))

    def clear_node_resources(self) -> None:
        """msh_clear_node_resources: back to "no table"."""
        self._check(self._lib.msh_clear_node_resources(self.handle))

    def node_resources(self) -> tuple[np.ndarray, np.ndarray] | None:
        """msh_node_resources: (alloc, used), each (nres, n) int64, or None when no table is present."""
        present, nres = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.msh_node_resources(self.handle, C.byref(nres), None, None, C.byref(present)))
        if not present.value:
            return None
        alloc = np.zeros((nres.value, self.n_nodes), np.int64)
        used = np.zeros((nres.value, self.n_nodes), np.int64)
        self._check(self._lib.msh_node_resources(self.handle, C.byref(nres), N.ptr(alloc), N.ptr(used),
                                                 C.byref(present)))
        return alloc, used

    def schedule_sequential_fit(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_req, max_pods_per_node: int = 0,
                                on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_fit: schedule_sequential with per-pod requests pod_req shaped (nres, p): a
        node is feasible only while every requested amount fits alloc - used; a placement adds them to used."""
        pod_digit = np.ascontiguousarray(pod_digit, np.int8)
        pod_tol = np.ascontiguousarray(pod_tol, np.uint8)
        p = _same_len("schedule_sequential_fit", pod_digit, pod_tol)
        pod_req = self._amounts(pod_req)
        if pod_req.shape[1] != p:
            raise ValueError("pod_req is shaped (nres, p)")
        idx, score, status = self._outputs(p, out)
        cb = N.COMMIT_CB(lambda _u, j, i, s: on_commit(j, i, s)) if on_commit else N.COMMIT_CB()
        self._check(self._lib.msh_schedule_sequential_fit(self.handle, p, N.ptr(pod_digit), N.ptr(pod_tol),
                                                          pod_req.shape[0], N.ptr(pod_req), int(max_pods_per_node),
                                                          N.ptr(idx), N.ptr(score), N.ptr(status), cb, None))
        return idx, score, status

    def schedule_sequential_fit_device(self, p: int, d_pod_digit: int, d_pod_tol: int, nres: int, d_pod_req: int,
                                       max_pods_per_node: int, d_idx: int, d_score: int, d_status: int,
                                       stream: int = 0) -> None:
        """msh_schedule_sequential_fit_device (asynchronous on `stream`; d_pod_req is not validated)."""
        self._check(self._lib.msh_schedule_sequential_fit_device(self.handle, int(p), d_pod_digit, d_pod_tol, int(nres),
                                                                 d_pod_req, int(max_pods_per_node), d_idx,
                                                                 d_score or None, d_status, stream or None))

    # -- resource-aware scoring of schedule_sequential_fit (NodeResourcesLeastAllocated / MostAllocated) --
    def set_resource_score(self, mode, weight: int = 1, resource_weights=None) -> None:
        """msh_set_resource_score: "none" (the default), "least" (spread: emptier nodes score higher) or "most"
        (pack), or the integers MSH_RESOURCE_SCORE_*. weight is the plugin weight; resource_weights one weight in
        [0, 100] per resource of the table (0: fitted but not scored), None = 1 for each resource of the table
        now on the device. Only schedule_sequential_fit / _fit_device read the setting; it survives
        upload_nodes."""
        m = RESOURCE_SCORE_MODES.get(mode) if isinstance(mode, (str, int)) and not isinstance(mode, bool) else None
        if m is None:
            raise N.MshError(N.MSH_ERR_INVALID, f"resource score mode {mode!r}: not 'none' (0), 'least' (1) or 'most' (2)")
        if m == N.MSH_RESOURCE_SCORE_NONE:
            self._check(self._lib.msh_set_resource_score(self.handle, m, 0, 0, None))
            return
        if resource_weights is None:
            present, nres = C.c_int32(0), C.c_int32(0)
            self._check(self._lib.msh_node_resources(self.handle, C.byref(nres), None, None, C.byref(present)))
            if not present.value:
                raise N.MshError(N.MSH_ERR_STATE, "resource_weights=None takes the table's resources: no table is present")
            resource_weights = [1] * nres.value
        w = np.ascontiguousarray(resource_weights, np.int32)
        if w.ndim != 1:
            raise ValueError("resource_weights: one weight per resource")
        self._check(self._lib.msh_set_resource_score(self.handle, m, int(weight), len(w), N.ptr(w)))

    def resource_score(self) -> tuple[int, int, list[int]]:
        """msh_get_resource_score: (mode, weight, the resource weights it was set with)."""
        m, w, nres = C.c_int32(), C.c_int64(), C.c_int32()
        rw = np.zeros(N.MAX_RESOURCES, np.int32)
        self._check(self._lib.msh_get_resource_score(self.handle, C.byref(m), C.byref(w), C.byref(nres), N.ptr(rw)))
        return m.value, w.value, rw[: nres.value].tolist()

    def seq_fit_max_nodes(self, nres: int, scored: bool = False) -> int:
        """msh_seq_fit_max_nodes: the largest table schedule_sequential_fit takes with nres resources, without
        (scored=False) or with a resource score."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_fit_max_nodes(self.handle, int(nres), 1 if scored else 0, C.byref(out)))
        return out.value

    # -- pod topology spread for sequential mode (PodTopologySpread, DoNotSchedule: zones, groups, counts) --
    @staticmethod
    def _int32s(a, what: str) -> np.ndarray:
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError(f"{what}: a one-dimensional integer array")
        if a.size and (int(a.min()) < -N.INT32_MAX - 1 or int(a.max()) > N.INT32_MAX):
            raise ValueError(f"{what}: integers within int32")
        return np.ascontiguousarray(a, np.int32)

    def upload_node_zones(self, zone) -> None:
        """msh_upload_node_zones: one zone id per uploaded node, List order, in [0, MAX_ZONES) or -1 for a node
        without the topology key. Replaces the column and zeroes the spread counts. upload_nodes drops it;
        patch_nodes, reset_node_pod_counts and the capacity and resource writers keep it."""
        zone = self._int32s(zone, "zones")
        self._check(self._lib.msh_upload_node_zones(self.handle, len(zone), N.ptr(zone)))

    def clear_node_zones(self) -> None:
        """msh_clear_node_zones: back to "no column"."""
        self._check(self._lib.msh_clear_node_zones(self.handle))

    def node_zones(self) -> np.ndarray | None:
        """msh_node_zones: the column (int32, List order), or None when no column is present."""
        present = C.c_int32(0)
        out = np.zeros(self.n_nodes, np.int32)
        self._check(self._lib.msh_node_zones(self.handle, N.ptr(out) if self.n_nodes else None, C.byref(present)))
        return out if present.value else None

    def set_spread_groups(self, max_skew) -> None:
        """msh_set_spread_groups: one max_skew >= 1 per spread group, at most MAX_SPREAD_GROUPS of them (an empty
        list: no groups). Another number of groups zeroes the spread counts; the same number only updates the skews."""
        sk = self._int32s(max_skew, "max_skew")
        self._check(self._lib.msh_set_spread_groups(self.handle, len(sk), N.ptr(sk) if len(sk) else None))

    def spread_groups(self) -> np.ndarray:
        """msh_get_spread_groups: the groups' max_skew (int32, one per group)."""
        g = C.c_int32(0)
        self._check(self._lib.msh_get_spread_groups(self.handle, C.byref(g), None))
        out = np.zeros(g.value, np.int32)
        self._check(self._lib.msh_get_spread_groups(self.handle, C.byref(g), N.ptr(out) if g.value else None))
        return out

    def spread_counts(self) -> np.ndarray:
        """msh_spread_counts: cnt[g][z] shaped (G, MAX_ZONES), int32: the committed pods of group g in zone z."""
        g = len(self.spread_groups())
        out = np.zeros((g, N.MAX_ZONES), np.int32)
        self._check(self._lib.msh_spread_counts(self.handle, N.ptr(out) if g else None))
        return out

    def patch_spread_counts(self, g, z, value) -> None:
        """msh_patch_spread_counts: value[k] replaces cnt[g[k]][z[k]] (distinct pairs, values >= 0): accounts for a
        deleted pod, or for pods bound elsewhere."""
        g, z, value = (self._int32s(a, "spread count patch") for a in (g, z, value))
        if not len(g) == len(z) == len(value):
            raise ValueError("g / z / value length mismatch")
        self._check(self._lib.msh_patch_spread_counts(self.handle, len(g), N.ptr(g), N.ptr(z), N.ptr(value)))

    def reset_spread_counts(self) -> None:
        """msh_reset_spread_counts: every spread count to 0."""
        self._check(self._lib.msh_reset_spread_counts(self.handle))

    def seq_spread_max_nodes(self, nres: int = 0) -> int:
        """msh_seq_spread_max_nodes: the largest table schedule_sequential_spread takes with nres (0..4) resources."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_spread_max_nodes(self.handle, int(nres), C.byref(out)))
        return out.value

    def schedule_sequential_spread(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_group, pod_req=None,
                                   max_pods_per_node: int = 0,
                                   on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_spread: schedule_sequential_fit with a spread group per pod (-1: none). A pod of
        group g is placed only on a node with a zone where cnt[g][zone] + 1 - min over the table's zones of cnt[g]
        stays within max_skew[g]; a placement adds 1 to cnt[g][zone]. pod_req (nres, p) as in
        schedule_sequential_fit, or None: no requests are checked or committed."""
        return self._grouped_host("schedule_sequential_spread", pod_digit, pod_tol, pod_group, None, pod_req,
                                  max_pods_per_node, on_commit, out, classes=False)

    def _grouped_host(self, name: str, pod_digit, pod_tol, pod_group, pod_class, pod_req, max_pods_per_node, on_commit,
                      out, classes: bool = True, extra: tuple = ()):
        """msh_<name>, a host entry point of the grouped sequential calls. classes=False: a spread form, which has
        no pod_class argument and requires pod_group. extra: the pointers of further optional per-pod columns, which
        follow pod_class."""
        pod_digit = np.ascontiguousarray(pod_digit, np.int8)
        pod_tol = np.ascontiguousarray(pod_tol, np.uint8)
        cols = [pod_digit, pod_tol]
        if pod_group is not None or not classes:
            pod_group = self._int32s(pod_group, "pod_group")
            cols.append(pod_group)
        if pod_class is not None:
            pod_class = self._int32s(pod_class, "pod_class")
            cols.append(pod_class)
        p = _same_len(name, *cols)
        nres = 0
        if pod_req is not None:
            pod_req = self._amounts(pod_req)
            if pod_req.shape[1] != p:
                raise ValueError("pod_req is shaped (nres, p)")
            nres = pod_req.shape[0]
        idx, score, status = self._outputs(p, out)
        cb = N.COMMIT_CB(lambda _u, j, i, s: on_commit(j, i, s)) if on_commit else N.COMMIT_CB()
        optional = ((N.ptr(pod_group), N.ptr(pod_class)) if classes else (N.ptr(pod_group),)) + tuple(extra)
        self._check(getattr(self._lib, "msh_" + name)(
            self.handle, p, N.ptr(pod_digit), N.ptr(pod_tol), *optional, nres, N.ptr(pod_req) if nres else None,
            int(max_pods_per_node), N.ptr(idx), N.ptr(score), N.ptr(status), cb, None))
        return idx, score, status

    def _grouped_device(self, name: str, p, d_pod_digit, d_pod_tol, d_optional, nres, d_pod_req, max_pods_per_node,
                        d_idx, d_score, d_status, stream) -> None:
        """msh_<name>_device; d_optional: (d_pod_group,) for a spread form, else (d_pod_group, d_pod_class) and for
        the inter-pod affinity form d_pod_profile after them."""
        self._check(getattr(self._lib, f"msh_{name}_device")(
            self.handle, int(p), d_pod_digit, d_pod_tol, *(d or None for d in d_optional), int(nres), d_pod_req or None,
            int(max_pods_per_node), d_idx, d_score or None, d_status, stream or None))

    def schedule_sequential_spread_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_pod_group: int, nres: int,
                                          d_pod_req: int, max_pods_per_node: int, d_idx: int, d_score: int,
                                          d_status: int, stream: int = 0) -> None:
        """msh_schedule_sequential_spread_device (asynchronous on `stream`; d_pod_req and d_pod_group are not
        validated: a group outside [0, G) is an ungrouped pod)."""
        self._grouped_device("schedule_sequential_spread", p, d_pod_digit, d_pod_tol, (d_pod_group,),
                             nres, d_pod_req, max_pods_per_node, d_idx, d_score, d_status, stream)

    # -- topology spread together with a resource score (the superset call of the sequential entry points) --
    def seq_spread_scored_max_nodes(self, nres: int = 0) -> int:
        """msh_seq_spread_scored_max_nodes: the largest table schedule_sequential_spread_scored takes with nres
        (0..4) resources as the ctx is set now: the scored limits with a resource score, seq_spread_max_nodes'
        without."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_spread_scored_max_nodes(self.handle, int(nres), C.byref(out)))
        return out.value

    def schedule_sequential_spread_scored(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_group, pod_req=None,
                                          max_pods_per_node: int = 0,
                                          on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_spread_scored: schedule_sequential_spread on a ctx that may hold a resource
        score. With set_resource_score("least" / "most") the feasible set is schedule_sequential_spread's and a
        feasible node's total is the scored schedule_sequential_fit's (NodeNumber plus weight x the Least /
        MostAllocated score); pod_req is then required. With "none" it is schedule_sequential_spread."""
        return self._grouped_host("schedule_sequential_spread_scored", pod_digit, pod_tol, pod_group, None, pod_req,
                                  max_pods_per_node, on_commit, out, classes=False)

    def schedule_sequential_spread_scored_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_pod_group: int,
                                                 nres: int, d_pod_req: int, max_pods_per_node: int, d_idx: int,
                                                 d_score: int, d_status: int, stream: int = 0) -> None:
        """msh_schedule_sequential_spread_scored_device (asynchronous on `stream`; d_pod_req and d_pod_group are
        not validated: a group outside [0, G) is an ungrouped pod)."""
        self._grouped_device("schedule_sequential_spread_scored", p, d_pod_digit, d_pod_tol, (d_pod_group,),
                             nres, d_pod_req, max_pods_per_node, d_idx, d_score, d_status, stream)

    # -- static node filters: per-class node masks (nodeSelector, required affinity, taints, nodeName) --
    @staticmethod
    def _class_bits(bits) -> np.ndarray:
        a = np.asarray(bits)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("class bits: a one-dimensional integer array")
        if a.size and a.dtype != np.uint64 and (int(a.min()) < 0 or int(a.max()) >= 1 << 64):
            raise ValueError("class bits: integers within uint64")
        return np.ascontiguousarray(a, np.uint64)

    def upload_node_class_bits(self, n_classes: int, bits) -> None:
        """msh_upload_node_class_bits: one uint64 per uploaded node, List order; bit c < n_classes is set if the node
        admits pods of class c (1 <= n_classes <= MAX_POD_CLASSES, no bit at or above n_classes). upload_nodes drops
        the column; patch_nodes, the count, capacity, resource and zone writers keep it; only
        schedule_sequential_classes reads it."""
        bits = self._class_bits(bits)
        self._check(self._lib.msh_upload_node_class_bits(self.handle, len(bits), int(n_classes), N.ptr(bits)))

    def patch_node_class_bits(self, idx, bits) -> None:
        """msh_patch_node_class_bits: bits[k] replaces node idx[k]'s whole word (distinct indices within the table;
        a column must be present). No table rebuild."""
        idx = np.ascontiguousarray(idx, np.int32)
        bits = self._class_bits(bits)
        if len(idx) != len(bits):
            raise ValueError("idx / bits length mismatch")
        self._check(self._lib.msh_patch_node_class_bits(self.handle, len(idx), N.ptr(idx), N.ptr(bits)))

    def clear_node_class_bits(self) -> None:
        """msh_clear_node_class_bits: back to "no column"."""
        self._check(self._lib.msh_clear_node_class_bits(self.handle))

    def node_class_bits(self) -> tuple[int, np.ndarray] | None:
        """msh_node_class_bits: (n_classes, the column as uint64 in List order), or None when no column is present."""
        present, nc = C.c_int32(0), C.c_int32(0)
        out = np.zeros(self.n_nodes, np.uint64)
        self._check(self._lib.msh_node_class_bits(self.handle, C.byref(nc), N.ptr(out) if self.n_nodes else None,
                                                  C.byref(present)))
        return (nc.value, out) if present.value else None

    def seq_classes_max_nodes(self, nres: int = 0) -> int:
        """msh_seq_classes_max_nodes: the largest table schedule_sequential_classes takes with nres (0..4) resources
        as the ctx is set now: the scored limits with a resource score, seq_spread_max_nodes' without."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_classes_max_nodes(self.handle, int(nres), C.byref(out)))
        return out.value

    def schedule_sequential_classes(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_group=None, pod_class=None,
                                    pod_req=None, max_pods_per_node: int = 0,
                                    on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_classes: schedule_sequential_spread_scored with a class per pod (-1: none). A pod of
        class c >= 0 is placed only on a node whose bit c is set in the class column; everything else (status, the
        normalizer's extents, the score, the tie-break, the commit) is taken over that feasible set. pod_class None:
        no pod has a class and no column is needed. pod_group None: no pod has a group and no zone column is
        needed."""
        return self._grouped_host("schedule_sequential_classes", pod_digit, pod_tol, pod_group, pod_class, pod_req,
                                  max_pods_per_node, on_commit, out)

    def schedule_sequential_classes_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_pod_group: int,
                                           d_pod_class: int, nres: int, d_pod_req: int, max_pods_per_node: int,
                                           d_idx: int, d_score: int, d_status: int, stream: int = 0) -> None:
        """msh_schedule_sequential_classes_device (asynchronous on `stream`; d_pod_group and d_pod_class may be 0;
        nothing is validated: a group outside [0, G) is an ungrouped pod, a class outside [0, C) a pod without one)."""
        self._grouped_device("schedule_sequential_classes", p, d_pod_digit, d_pod_tol, (d_pod_group, d_pod_class),
                             nres, d_pod_req, max_pods_per_node, d_idx, d_score, d_status, stream)

    # -- preferred node affinity and PreferNoSchedule scores: per-class raw values --
    def _pref_array(self, a, n_classes: int, width: int, what: str) -> np.ndarray | None:
        if a is None:
            return None
        v = np.asarray(a)
        if v.shape != (n_classes, width) or (v.size and v.dtype.kind not in "iu"):
            raise ValueError(f"{what}: an integer array shaped (n_classes, {width})")
        if v.size and (int(v.min()) < 0 or int(v.max()) > 0xFFFF):
            raise ValueError(f"{what}: values within uint16")
        return np.ascontiguousarray(v, np.uint16)

    def upload_node_class_prefs(self, n_classes: int, affinity=None, taints=None) -> None:
        """msh_upload_node_class_prefs: the raw preferred-affinity sums and PreferNoSchedule counts, each shaped
        (n_classes, n_nodes) in List order, or None (all zero). upload_nodes drops the column; every other writer keeps
        it; only schedule_sequential_prefs reads it."""
        a = self._pref_array(affinity, int(n_classes), self.n_nodes, "affinity")
        t = self._pref_array(taints, int(n_classes), self.n_nodes, "taints")
        self._check(self._lib.msh_upload_node_class_prefs(self.handle, self.n_nodes, int(n_classes), N.ptr(a), N.ptr(t)))

    def patch_node_class_prefs(self, idx, affinity=None, taints=None) -> None:
        """msh_patch_node_class_prefs: the values of nodes idx[k] for every class, each array shaped (n_classes,
        len(idx)) or None (zeros)."""
        idx = np.ascontiguousarray(idx, np.int32)
        col = self.node_class_prefs()
        nc = col[0] if col is not None else 0
        a = self._pref_array(affinity, nc, len(idx), "affinity") if col is not None else None
        t = self._pref_array(taints, nc, len(idx), "taints") if col is not None else None
        self._check(self._lib.msh_patch_node_class_prefs(self.handle, len(idx), N.ptr(idx), N.ptr(a), N.ptr(t)))

    def clear_node_class_prefs(self) -> None:
        """msh_clear_node_class_prefs: back to "no column"."""
        self._check(self._lib.msh_clear_node_class_prefs(self.handle))

    def node_class_prefs(self) -> tuple[int, np.ndarray, np.ndarray] | None:
        """msh_node_class_prefs: (n_classes, affinity, taints), the arrays shaped (n_classes, n_nodes), or None when
        no column is present."""
        present, nc = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.msh_node_class_prefs(self.handle, C.byref(nc), None, None, C.byref(present)))
        if not present.value:
            return None
        a = np.zeros((nc.value, self.n_nodes), np.uint16)
        t = np.zeros((nc.value, self.n_nodes), np.uint16)
        self._check(self._lib.msh_node_class_prefs(self.handle, C.byref(nc), N.ptr(a) if a.size else None,
                                                   N.ptr(t) if t.size else None, C.byref(present)))
        return nc.value, a, t

    def set_preference_weights(self, affinity: int = 0, taint: int = 0) -> None:
        """msh_set_preference_weights: the plugin weights of the two preference scores, each in [0, 100]."""
        self._check(self._lib.msh_set_preference_weights(self.handle, int(affinity), int(taint)))

    def preference_weights(self) -> tuple[int, int]:
        a, t = C.c_int32(), C.c_int32()
        self._check(self._lib.msh_preference_weights(self.handle, C.byref(a), C.byref(t)))
        return a.value, t.value

    def seq_prefs_max_nodes(self, nres: int = 0) -> int:
        """msh_seq_prefs_max_nodes: the largest table schedule_sequential_prefs takes with nres (0..4) resources."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_prefs_max_nodes(self.handle, int(nres), C.byref(out)))
        return out.value

    def schedule_sequential_prefs(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_group=None, pod_class=None,
                                  pod_req=None, max_pods_per_node: int = 0,
                                  on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_prefs: schedule_sequential_classes with w_affinity * na + w_taint * nt added to
        every feasible node's total, na and nt normalised per pod over its feasible nodes. With both weights 0 it is
        schedule_sequential_classes."""
        return self._grouped_host("schedule_sequential_prefs", pod_digit, pod_tol, pod_group, pod_class, pod_req,
                                  max_pods_per_node, on_commit, out)

    def schedule_sequential_prefs_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_pod_group: int,
                                         d_pod_class: int, nres: int, d_pod_req: int, max_pods_per_node: int,
                                         d_idx: int, d_score: int, d_status: int, stream: int = 0) -> None:
        """msh_schedule_sequential_prefs_device (asynchronous on `stream`; as schedule_sequential_classes_device)."""
        self._grouped_device("schedule_sequential_prefs", p, d_pod_digit, d_pod_tol, (d_pod_group, d_pod_class),
                             nres, d_pod_req, max_pods_per_node, d_idx, d_score, d_status, stream)

    # -- soft topology spread (whenUnsatisfiable: ScheduleAnyway) --
    def set_spread_group_modes(self, modes) -> None:
        """msh_set_spread_group_modes: one mode per spread group, SPREAD_DO_NOT_SCHEDULE (0, the default: the hard
        filter) or SPREAD_SCHEDULE_ANYWAY (1: no filter, the spread score). The length must be the group count."""
        m = np.asarray(modes)
        if m.ndim != 1 or (m.size and (m.dtype.kind not in "iub" or m.min() < 0 or m.max() > 255)):
            raise ValueError("modes is a flat array of 0 / 1")
        m = np.ascontiguousarray(m, np.uint8)
        self._check(self._lib.msh_set_spread_group_modes(self.handle, len(m), N.ptr(m) if len(m) else None))

    def spread_group_modes(self) -> np.ndarray:
        """msh_get_spread_group_modes: the groups' modes (uint8, one per group)."""
        g = C.c_int32(0)
        self._check(self._lib.msh_get_spread_group_modes(self.handle, C.byref(g), None))
        out = np.zeros(g.value, np.uint8)
        self._check(self._lib.msh_get_spread_group_modes(self.handle, C.byref(g), N.ptr(out) if g.value else None))
        return out

    def set_spread_score_weight(self, weight: int = 0) -> None:
        """msh_set_spread_score_weight: the plugin weight of the soft spread score, in [0, 100]."""
        self._check(self._lib.msh_set_spread_score_weight(self.handle, int(weight)))

    def spread_score_weight(self) -> int:
        w = C.c_int32()
        self._check(self._lib.msh_spread_score_weight(self.handle, C.byref(w)))
        return w.value

    def seq_soft_max_nodes(self, nres: int = 0) -> int:
        """msh_seq_soft_max_nodes: the largest table schedule_sequential_soft takes with nres (0..4) resources."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_soft_max_nodes(self.handle, int(nres), C.byref(out)))
        return out.value

    def schedule_sequential_soft(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_group=None, pod_class=None,
                                 pod_req=None, max_pods_per_node: int = 0,
                                 on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_soft: schedule_sequential_prefs, except that a pod of a SCHEDULE_ANYWAY group passes
        no spread filter and w_spread * ns is added to every feasible node with a zone, ns upstream's normalised
        PodTopologySpread score over the zones of the pod's feasible nodes. With no such group it is
        schedule_sequential_prefs."""
        return self._grouped_host("schedule_sequential_soft", pod_digit, pod_tol, pod_group, pod_class, pod_req,
                                  max_pods_per_node, on_commit, out)

    def schedule_sequential_soft_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_pod_group: int,
                                        d_pod_class: int, nres: int, d_pod_req: int, max_pods_per_node: int,
                                        d_idx: int, d_score: int, d_status: int, stream: int = 0) -> None:
        """msh_schedule_sequential_soft_device (asynchronous on `stream`; as schedule_sequential_prefs_device)."""
        self._grouped_device("schedule_sequential_soft", p, d_pod_digit, d_pod_tol, (d_pod_group, d_pod_class),
                             nres, d_pod_req, max_pods_per_node, d_idx, d_score, d_status, stream)

    # -- NodeResourcesBalancedAllocation --
    def set_balanced_score(self, weight: int = 0) -> None:
        """msh_set_balanced_score: the plugin weight of the balanced-allocation score, in [0, 100]."""
        self._check(self._lib.msh_set_balanced_score(self.handle, int(weight)))

    def balanced_score(self) -> int:
        w = C.c_int32()
        self._check(self._lib.msh_balanced_score(self.handle, C.byref(w)))
        return w.value

    def seq_balanced_max_nodes(self, nres: int = 0) -> int:
        """msh_seq_balanced_max_nodes: the largest table schedule_sequential_balanced takes with nres (0..4) resources."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_balanced_max_nodes(self.handle, int(nres), C.byref(out)))
        return out.value

    def schedule_sequential_balanced(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_group=None, pod_class=None,
                                     pod_req=None, max_pods_per_node: int = 0,
                                     on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_balanced: schedule_sequential_soft with w_balanced * BS added to every feasible
        node's total, BS upstream's NodeResourcesBalancedAllocation score of the table's first two resources after
        the pod, evaluated in float64 as upstream does. With the weight 0 it is schedule_sequential_soft."""
        return self._grouped_host("schedule_sequential_balanced", pod_digit, pod_tol, pod_group, pod_class, pod_req,
                                  max_pods_per_node, on_commit, out)

    def schedule_sequential_balanced_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_pod_group: int,
                                            d_pod_class: int, nres: int, d_pod_req: int, max_pods_per_node: int,
                                            d_idx: int, d_score: int, d_status: int, stream: int = 0) -> None:
        """msh_schedule_sequential_balanced_device (asynchronous on `stream`; as schedule_sequential_soft_device)."""
        self._grouped_device("schedule_sequential_balanced", p, d_pod_digit, d_pod_tol, (d_pod_group, d_pod_class),
                             nres, d_pod_req, max_pods_per_node, d_idx, d_score, d_status, stream)

    # -- required inter-pod affinity and anti-affinity --
    @staticmethod
    def _words32(a, what: str) -> np.ndarray:
        v = np.asarray(a)
        if v.ndim != 1 or (v.size and v.dtype.kind not in "iu"):
            raise ValueError(f"{what}: a one-dimensional integer array")
        if v.size and (int(v.min()) < 0 or int(v.max()) > 0xFFFFFFFF):
            raise ValueError(f"{what}: integers within uint32")
        return np.ascontiguousarray(v, np.uint32)

    def set_pod_affinity_terms(self, topologies=()) -> None:
        """msh_set_pod_affinity_terms: one topology per term (TOPOLOGY_HOSTNAME or TOPOLOGY_ZONE), at most
        MAX_AFFINITY_TERMS. Sets the terms, drops the profiles and zeroes the state; an empty list is "no terms"."""
        t = np.asarray(topologies)
        if t.ndim != 1 or (t.size and (t.dtype.kind not in "iub" or t.min() < 0 or t.max() > 255)):
            raise ValueError("topologies is a flat array of 0 / 1")
        t = np.ascontiguousarray(t, np.uint8)
        self._check(self._lib.msh_set_pod_affinity_terms(self.handle, len(t), N.ptr(t) if len(t) else None))

    def pod_affinity_terms(self) -> np.ndarray:
        """msh_get_pod_affinity_terms: the terms' topologies (uint8, one per term)."""
        n = C.c_int32(0)
        self._check(self._lib.msh_get_pod_affinity_terms(self.handle, C.byref(n), None))
        out = np.zeros(n.value, np.uint8)
        self._check(self._lib.msh_get_pod_affinity_terms(self.handle, C.byref(n), N.ptr(out) if n.value else None))
        return out

    def set_pod_profiles(self, match=(), anti=(), aff=()) -> None:
        """msh_set_pod_profiles: per profile the terms a pod of it satisfies (match, a uint32 of term bits), its own
        required anti-affinity terms (anti) and its one required affinity term (aff, -1: none). At most
        MAX_POD_PROFILES; the ctx must hold terms."""
        m, a = self._words32(match, "match"), self._words32(anti, "anti")
        f = self._int32s(aff, "aff")
        if not len(m) == len(a) == len(f):
            raise ValueError("match / anti / aff length mismatch")
        q = len(m)
        self._check(self._lib.msh_set_pod_profiles(self.handle, q, N.ptr(m) if q else None, N.ptr(a) if q else None,
                                                   N.ptr(f) if q else None))

    def pod_profiles(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """msh_get_pod_profiles: (match, anti, aff)."""
        n = C.c_int32(0)
        self._check(self._lib.msh_get_pod_profiles(self.handle, C.byref(n), None, None, None))
        m, a, f = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32), np.zeros(n.value, np.int32)
        if n.value:
            self._check(self._lib.msh_get_pod_profiles(self.handle, C.byref(n), N.ptr(m), N.ptr(a), N.ptr(f)))
        return m, a, f

    def upload_pod_affinity_state(self, present=None, repel=None) -> None:
        """msh_upload_pod_affinity_state: per node (List order) the OR of the match bits (present) and of the
        anti-affinity terms (repel) of the pods it holds; None: zeros. upload_nodes zeroes the state; every other
        writer keeps it; only schedule_sequential_podaffinity reads it."""
        pr = None if present is None else self._words32(present, "present")
        rp = None if repel is None else self._words32(repel, "repel")
        for v in (pr, rp):
            if v is not None and len(v) != self.n_nodes:
                raise ValueError("one state word per uploaded node")
        self._check(self._lib.msh_upload_pod_affinity_state(self.handle, self.n_nodes, N.ptr(pr), N.ptr(rp)))

    def patch_pod_affinity_state(self, idx, present=None, repel=None) -> None:
        """msh_patch_pod_affinity_state: whole words of nodes idx[k] (distinct, within the table); None: zeros."""
        idx = np.ascontiguousarray(idx, np.int32)
        pr = None if present is None else self._words32(present, "present")
        rp = None if repel is None else self._words32(repel, "repel")
        for v in (pr, rp):
            if v is not None and len(v) != len(idx):
                raise ValueError("idx / state length mismatch")
        self._check(self._lib.msh_patch_pod_affinity_state(self.handle, len(idx), N.ptr(idx), N.ptr(pr), N.ptr(rp)))

    def pod_affinity_state(self) -> tuple[np.ndarray, np.ndarray]:
        """msh_pod_affinity_state: (present, repel), uint32 per node in List order."""
        pr, rp = np.zeros(self.n_nodes, np.uint32), np.zeros(self.n_nodes, np.uint32)
        self._check(self._lib.msh_pod_affinity_state(self.handle, N.ptr(pr) if self.n_nodes else None,
                                                     N.ptr(rp) if self.n_nodes else None))
        return pr, rp

    def seq_podaffinity_max_nodes(self, nres: int = 0) -> int:
        """msh_seq_podaffinity_max_nodes: the largest table schedule_sequential_podaffinity takes with nres (0..4)
        resources."""
        out = C.c_int32()
        self._check(self._lib.msh_seq_podaffinity_max_nodes(self.handle, int(nres), C.byref(out)))
        return out.value

    def schedule_sequential_podaffinity(self, pod_digit: np.ndarray, pod_tol: np.ndarray, pod_group=None,
                                        pod_class=None, pod_profile=None, pod_req=None, max_pods_per_node: int = 0,
                                        on_commit: Callable[[int, int, int], None] | None = None, out=None):
        """msh_schedule_sequential_podaffinity: schedule_sequential_balanced with a profile per pod (-1: none). A pod
        of profile q is placed only where the required inter-pod affinity and anti-affinity filter passes: no pod in
        the node's topology domain matches one of its anti-affinity terms, it matches no anti-affinity term of a pod
        there, and a pod matching its affinity term is in the domain (or it is the first of a self-affine series).
        Each placement is committed to the state before the next pod. pod_profile None: schedule_sequential_balanced."""
        extra = None
        if pod_profile is not None:
            extra = self._int32s(pod_profile, "pod_profile")
            if len(extra) != len(np.asarray(pod_digit)):
                raise ValueError("schedule_sequential_podaffinity: pod_profile length mismatch")
        return self._grouped_host("schedule_sequential_podaffinity", pod_digit, pod_tol, pod_group, pod_class, pod_req,
                                  max_pods_per_node, on_commit, out, extra=(N.ptr(extra),))

    def schedule_sequential_podaffinity_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_pod_group: int,
                                               d_pod_class: int, d_pod_profile: int, nres: int, d_pod_req: int,
                                               max_pods_per_node: int, d_idx: int, d_score: int, d_status: int,
                                               stream: int = 0) -> None:
        """msh_schedule_sequential_podaffinity_device (asynchronous on `stream`; as schedule_sequential_balanced_device;
        a profile outside [0, Q) is a pod without one)."""
        self._grouped_device("schedule_sequential_podaffinity", p, d_pod_digit, d_pod_tol,
                             (d_pod_group, d_pod_class, d_pod_profile), nres, d_pod_req, max_pods_per_node, d_idx,
                             d_score, d_status, stream)

    # -- device-resident entry points (integer device addresses, hipStream_t as int) --
    # The per-batch device entry points go through the CPython fast-call module (csrc/msh_pyfast.c):
    # ctypes argument conversion cost ~0.9 us per call next to a ~2.6 us launch.
    def schedule_batch_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_idx: int, d_score: int,
                              d_status: int, stream: int = 0) -> None:
        rc = self._fast.schedule_batch_device(self._hv(), p, d_pod_digit, d_pod_tol, d_idx, d_score,
                                              d_status, stream or None)
        if rc:
            self._check(rc)

    @staticmethod
    def batch_descs(batches: Sequence[tuple]) -> "C.Array":
        """An msh_batch array for schedule_batches_device from (p, d_pod_digit, d_pod_tol, d_idx,
        d_score or 0, d_status) tuples of device addresses; build it once and reuse it."""
        arr = (N.Batch * len(batches))()
        for i, (p, pd, pt, oi, os_, ost) in enumerate(batches):
            arr[i] = N.Batch(int(p), 0, pd, pt, oi, os_ or None, ost)
        return arr

    def schedule_batches_device(self, descs, nb: int | None = None, stream: int = 0) -> None:
        """msh_schedule_batches_device over an msh_batch array (batch_descs): up to
        N.BATCHES_PER_LAUNCH batches per kernel launch, asynchronous on `stream`."""
        nb = len(descs) if nb is None else nb
        rc = self._fast.schedule_batches_device(self._hv(), nb, C.addressof(descs), stream or None)
        if rc:
            self._check(rc)

    def schedule_sequential_device(self, p: int, d_pod_digit: int, d_pod_tol: int, max_pods_per_node: int,
                                   d_idx: int, d_score: int, d_status: int, stream: int = 0) -> None:
        rc = self._fast.schedule_sequential_device(self._hv(), p, d_pod_digit, d_pod_tol,
                                                   int(max_pods_per_node), d_idx, d_score, d_status, stream or None)
        if rc:
            self._check(rc)

    def shard_keys_len(self, p: int) -> int:
        """int32 entries msh_shard_keys_device writes for p pods: 2p (ABI v7)."""
        v = C.c_int32(0)
        self._check(self._lib.msh_shard_keys_len(self.handle, int(p), C.byref(v)))
        return int(v.value)

    def shard_keys_device(self, p: int, d_pod_digit: int, d_pod_tol: int, node_base: int, d_keys: int,
                          stream: int = 0) -> None:
        rc = self._fast.shard_keys_device(self._hv(), p, d_pod_digit, d_pod_tol, int(node_base), d_keys,
                                          stream or None)
        if rc:
            self._check(rc)

    def decode_keys_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_keys: int, d_idx: int,
                           d_score: int, d_status: int, stream: int = 0) -> None:
        rc = self._fast.decode_keys_device(self._hv(), p, d_pod_digit, d_pod_tol, d_keys, d_idx, d_score, d_status,
                                           stream or None)
        if rc:
            self._check(rc)

    def keys_slot1_is_any(self) -> bool:
        v = C.c_int32(0)
        self._check(self._lib.msh_keys_slot1_is_any(self.handle, C.byref(v)))
        return bool(v.value)

    # -- node-sharded scheduling with the merge in the library (ABI v8: RCCL communicator) --
    @staticmethod
    def comm_unique_id() -> bytes:
        """msh_comm_unique_id: the MSH_COMM_ID_BYTES id rank 0 makes and ships to every rank."""
        buf = (C.c_uint8 * N.COMM_ID_BYTES)()
        N.check(N.lib().msh_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, comm_id: bytes, world: int, rank: int) -> None:
        """msh_comm_init (collective over the `world` ranks)."""
        if len(comm_id) != N.COMM_ID_BYTES:
            raise ValueError(f"a comm id is {N.COMM_ID_BYTES} bytes")
        buf = (C.c_uint8 * N.COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._check(self._lib.msh_comm_init(self.handle, buf, int(world), int(rank)))

    def comm_info(self) -> tuple[int, int]:
        w, r = C.c_int32(), C.c_int32()
        self._check(self._lib.msh_comm_info(self.handle, C.byref(w), C.byref(r)))
        return w.value, r.value

    def schedule_nodeshard_device(self, p: int, d_pod_digit: int, d_pod_tol: int, node_base: int, d_idx: int,
                                  d_score: int, d_status: int, stream: int = 0) -> None:
        """msh_schedule_nodeshard_device: shard kernel, all-reduce(s) over the communicator, decode, on
        `stream`; every rank ends with the global decisions."""
        rc = self._fast.schedule_nodeshard_device(self._hv(), p, d_pod_digit, d_pod_tol, int(node_base), d_idx,
                                                  d_score, d_status, stream or None)
        if rc:
            self._check(rc)

    def schedule_nodeshard(self, pod_digit: np.ndarray, pod_tol: np.ndarray, node_base: int, out=None):
        """msh_schedule_nodeshard: the host-buffer form (synchronous)."""
        pod_digit = np.ascontiguousarray(pod_digit, np.int8)
        pod_tol = np.ascontiguousarray(pod_tol, np.uint8)
        p = _same_len("schedule_nodeshard", pod_digit, pod_tol)
        idx, score, status = self._outputs(p, out)
        self._check(self._lib.msh_schedule_nodeshard(self.handle, p, N.ptr(pod_digit), N.ptr(pod_tol), int(node_base),
                                                     N.ptr(idx), N.ptr(score), N.ptr(status)))
        return idx, score, status

    # -- node-sharded generic pipeline (msh_generic_*: any plugin list, score columns included) --
    def generic_ext_len(self, p: int) -> int:
        """int64 entries of the per-pod extents msh_generic_extents_device writes (0: no plugin
        normalizes, nothing to merge before the bests)."""
        v = C.c_int64(0)
        self._check(self._lib.msh_generic_ext_len(self.handle, int(p), C.byref(v)))
        return int(v.value)

    def generic_extents_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_ext: int, stream: int = 0) -> None:
        self._check(self._lib.msh_generic_extents_device(self.handle, int(p), d_pod_digit, d_pod_tol, d_ext,
                                                         stream or None))

    def generic_best_device(self, p: int, d_pod_digit: int, d_pod_tol: int, d_ext: int, node_base: int,
                            d_best_total: int, d_best_idx: int, stream: int = 0) -> None:
        self._check(self._lib.msh_generic_best_device(self.handle, int(p), d_pod_digit, d_pod_tol, d_ext or None,
                                                      int(node_base), d_best_total, d_best_idx, stream or None))

    def generic_candidates_device(self, p: int, d_local_total: int, d_merged_total: int, d_best_idx: int,
                                  stream: int = 0) -> None:
        self._check(self._lib.msh_generic_candidates_device(self.handle, int(p), d_local_total, d_merged_total,
                                                            d_best_idx, stream or None))

    def generic_decode_device(self, p: int, d_pod_digit: int, d_merged_total: int, d_merged_idx: int, d_idx: int,
                              d_score: int, d_status: int, stream: int = 0) -> None:
        self._check(self._lib.msh_generic_decode_device(self.handle, int(p), d_pod_digit, d_merged_total,
                                                        d_merged_idx, d_idx, d_score or None, d_status,
                                                        stream or None))


class DeviceGroup:
    """msh_group: shard ctxs in List order (ctxs[k] holds the k-th contiguous slice of the node table), any
    devices; the merge runs on ctxs[0]'s device. The ctxs stay owned by the caller: close the group first."""

    def __init__(self, ctxs: Sequence[DeviceContext]):
        self._lib = N.lib()
        self.ctxs = list(ctxs)
        arr = (C.c_void_p * len(self.ctxs))(*[c.handle for c in self.ctxs])
        h = C.c_void_p()
        rc = self._lib.msh_group_create(arr, len(self.ctxs), C.byref(h))
        if rc != N.MSH_OK:
            raw = self._lib.msh_group_last_error(None)
            raise N.MshError(rc, raw.decode() if raw else "")
        self.handle = h

    def close(self) -> None:
        if self.handle:
            self._lib.msh_group_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def schedule_batch(self, pod_digit: np.ndarray, pod_tol: np.ndarray, scores: bool = True):
        """msh_group_schedule_batch: the decisions over the whole (sharded) table."""
        pod_digit = np.ascontiguousarray(pod_digit, np.int8)
        pod_tol = np.ascontiguousarray(pod_tol, np.uint8)
        p = _same_len("group schedule_batch", pod_digit, pod_tol)
        idx, score, status = np.empty(p, np.int32), (np.empty(p, np.int64) if scores else None), np.empty(p, np.int32)
        rc = self._lib.msh_group_schedule_batch(self.handle, p, N.ptr(pod_digit), N.ptr(pod_tol), N.ptr(idx),
                                                N.ptr(score), N.ptr(status))
        if rc != N.MSH_OK:
            raw = self._lib.msh_group_last_error(self.handle)
            raise N.MshError(rc, raw.decode() if raw else "")
        return idx, score, status


class Scheduler:
    """Batched mirror of minisched.Scheduler (initialize.go:18-29).

    Defaults are the reference's hardcoded plugin lists (initialize.go:80-123):
    filter=[NodeUnschedulable], preScore=[NodeNumber], score=[NodeNumber] (weight 1,
    no NormalizeScore: nodenumber.go:98-100). tie_break="random" (with tie_seed) picks uniformly
    among the maximum-score nodes like the reference's selectHost; the default "first" takes the
    first maximum in List order.

    Nodes may carry an allocatable-pods value: the attribute `allocatable_pods`, or
    status.allocatable.pods of a k8s-shaped dict (snapshot.node_allocatable_pods). When any node of the
    snapshot carries one, schedule_sequential uploads the capacity column (None: INT32_MAX, in effect
    unlimited) and every node stops at its own limit; schedule_batch ignores it.

    resources (default None: nothing changes) names the resources schedule_sequential accounts for, e.g.
    ("cpu", "memory"), at most four: it then uploads the snapshot's status.allocatable amounts once per snapshot
    (cpu in milli-units, everything else in units; a node lacking a value counts as 0) and places each pod only
    where its requests (snapshot.pod_requests) still fit, committing them to the node (upstream's
    NodeResourcesFit; DeviceContext.schedule_sequential_fit). schedule_batch ignores them.

    resource_score ("least" or "most"; default None: NodeNumber alone scores) adds upstream's
    NodeResourcesLeastAllocated (spread) or NodeResourcesMostAllocated (pack) score of the pod's requests against
    each feasible node to schedule_sequential's totals, at plugin weight resource_score_weight. resource_weights
    is a mapping from resource name to weight, or a sequence aligned with `resources` (default: 1 each; 0: fitted
    but not scored). It needs `resources`. The library substitutes no defaults for pods that request nothing.

    zones and spread_groups (default None; given together) add upstream's PodTopologySpread filter (DoNotSchedule) to
    schedule_sequential: `zones` names the node label that holds the topology domain (e.g.
    "topology.kubernetes.io/zone"; at most 64 distinct values, a node without the label takes no grouped pod),
    `spread_groups` maps a group name to its max_skew, and a pod belongs to the group named by its `spread_label`
    label (default "app"), or to none. A grouped pod is placed only where its group's count in the node's zone stays
    within max_skew of the group's emptiest zone (DeviceContext.schedule_sequential_spread); with `resources` the
    requests are fitted too, and with resource_score the feasible nodes are scored as above
    (DeviceContext.schedule_sequential_spread_scored, the call schedule_sequential makes whenever groups are
    configured). schedule_batch ignores them.

    The static node filters of the default profile need no configuration: schedule_sequential reads spec.nodeName,
    spec.nodeSelector, the required node affinity and spec.tolerations of every pod and the name, labels and
    spec.taints of every node (constraints.node_admits), groups the pods into at most 64 classes of equal
    constraints per node snapshot and, whenever some pod of the call has a class that some node does not admit,
    makes the class call (DeviceContext.schedule_sequential_classes) with whatever else is configured. A call
    whose pods are admitted everywhere is made exactly as before. schedule_batch ignores them.

    The two preference scores are off by default. With preferred_affinity_weight or prefer_no_schedule_weight nonzero
    (each in [0, 100]) a pod's class is keyed by its constraints and its preferences (constraints.class_key +
    constraints.preference_key), a class gets an id if some node does not admit it or if one of its raw values
    (constraints.preferred_affinity_score, constraints.prefer_no_schedule_count) is nonzero on some node, both
    columns are uploaded for the same classes, and a call in which some pod has such a preference is made with
    DeviceContext.schedule_sequential_prefs; every other call takes the paths above.

    balanced_allocation_weight (in [0, 100], default 0) is NodeResourcesBalancedAllocation's plugin weight. It needs
    `resources` with at least two names, the first two being the ones upstream balances (cpu and memory). With a
    nonzero weight every schedule_sequential call is DeviceContext.schedule_sequential_balanced, with the classes,
    groups and requests that the paths above would have passed.

    Required inter-pod affinity and anti-affinity need no configuration: schedule_sequential reads
    spec.affinity.podAffinity / podAntiAffinity.requiredDuringSchedulingIgnoredDuringExecution of every pod
    (constraints.check_pod_affinity). The topologyKey of a term is kubernetes.io/hostname (every node is its own
    domain) or the `zones` label. Per node snapshot the scheduler keeps the distinct terms (at most 32), the profiles
    of the pods of the call (at most 64: which terms a pod's labels and namespace satisfy, its anti-affinity terms and
    its one affinity term) and a record of the pods it placed; when a call brings a new term it sets the device's
    tables again, recomputes the per-node state from the record and uploads it; when it brings only a new profile it
    sets the profiles alone, which keeps the device's state. Once the snapshot has a term,
    every pod of every later call gets a profile from its labels and the call is
    DeviceContext.schedule_sequential_podaffinity with whatever else is configured. Only pods placed by this scheduler
    against the snapshot are in the record: pods that were bound before it are the caller's to enter through
    DeviceContext.patch_pod_affinity_state, after the first call that brought the terms and again after any call
    that brings a new one (the bit of a term is its position in Scheduler.pod_affinity_terms()). The preferred
    (scoring) half of the plugin is not implemented. schedule_batch ignores all of it.
    """

    def __init__(self, filter_plugins: Sequence[str] = (NODE_UNSCHEDULABLE,),
                 pre_score_plugins: Sequence[str] = (NODE_NUMBER,),
                 score_plugins: Sequence[ScorePluginConfig | str] = (NODE_NUMBER,),
                 device: int = 0, ctx: DeviceContext | None = None, *, tie_break="first", tie_seed: int = 0,
                 resources: Sequence[str] | None = None, resource_score=None, resource_score_weight: int = 1,
                 resource_weights=None, zones: str | None = None, spread_groups: Mapping[str, int] | None = None,
                 spread_label: str = "app", preferred_affinity_weight: int = 0, prefer_no_schedule_weight: int = 0,
                 balanced_allocation_weight: int = 0):
        self.resources = None if resources is None else tuple(resources)
        w = balanced_allocation_weight
        if isinstance(w, bool) or not isinstance(w, int) or not 0 <= w <= 100:
            raise ValueError("balanced_allocation_weight: an integer in [0, 100]")
        if w and (resources is None or len(self.resources) < 2):
            raise ValueError("balanced_allocation_weight needs resources with at least two names (cpu and memory first)")
        self.balanced_allocation_weight = w
        for w in (preferred_affinity_weight, prefer_no_schedule_weight):
            if isinstance(w, bool) or not isinstance(w, int) or not 0 <= w <= 100:
                raise ValueError("preferred_affinity_weight / prefer_no_schedule_weight: integers in [0, 100]")
        self.preferred_affinity_weight = preferred_affinity_weight
        self.prefer_no_schedule_weight = prefer_no_schedule_weight
        self._prefs_on = bool(preferred_affinity_weight or prefer_no_schedule_weight)
        if (zones is None) != (spread_groups is None):
            raise ValueError("zones and spread_groups go together")
        if spread_groups is not None:
            if len(spread_groups) > N.MAX_SPREAD_GROUPS:
                raise ValueError(f"spread_groups: at most {N.MAX_SPREAD_GROUPS} groups")
            if any(isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= N.INT32_MAX for v in spread_groups.values()):
                raise ValueError("spread_groups: each max_skew an integer in [1, INT32_MAX]")
        self.zones = zones
        self.spread_label = spread_label
        self.spread_groups = None if spread_groups is None else dict(spread_groups)
        self._group_ids = {} if spread_groups is None else {name: k for k, name in enumerate(self.spread_groups)}
        if self.resources is not None and not 1 <= len(self.resources) <= N.MAX_RESOURCES:
            raise ValueError(f"resources: 1 to {N.MAX_RESOURCES} names")
        rs_weights = self._resource_weights(self.resources, resource_score, resource_weights)
        self.filter_plugins = list(filter_plugins)
        self.pre_score_plugins = list(pre_score_plugins)
        self.score_plugins = [c if isinstance(c, ScorePluginConfig) else ScorePluginConfig(c)
                              for c in score_plugins]
        self.ctx = ctx or DeviceContext(device)
        self.ctx.set_plugins(self.filter_plugins, self.pre_score_plugins, self.score_plugins)
        # selectHost's tie-break (minisched.go:304-325): "first" keeps the first maximum; "random" spreads
        # ties uniformly as the reference does (schedule_sequential then raises MSH_ERR_UNSUPPORTED)
        if tie_break not in ("first", N.MSH_TIEBREAK_FIRST) or tie_seed:
            self.ctx.set_tiebreak(tie_break, tie_seed)
        if rs_weights is not None:
            self.ctx.set_resource_score(resource_score, resource_score_weight, rs_weights)
        if self.spread_groups is not None:
            self.ctx.set_spread_groups(list(self.spread_groups.values()))
        self._zone_synced = False  # the snapshot's zone column is on the device
        self.nodes: NodeTable | None = None
        self._cap_synced = False  # the snapshot's capacity column is on the device
        self._res_synced = False  # the snapshot's allocatable amounts are on the device
        self._node_objs: list[Any] = []  # the snapshot's nodes in List order
        # static node filters (constraints.node_admits): the classes of the pods seen against this snapshot, by
        # constraints.class_key: an id in [0, MAX_POD_CLASSES), or -1 for a class that every node admits
        self._class_ids: dict[str, int] = {}
        self._class_masks: list[np.ndarray] = []  # per id, the nodes (List order) that admit the class
        self._class_synced = False  # the masks are on the device
        # with a preference weight: per id, the raw preferred-affinity sums and PreferNoSchedule counts by node, and the
        # ids with a nonzero raw value somewhere (constraints.preferred_affinity_score / prefer_no_schedule_count)
        self._class_aff: list[np.ndarray] = []
        self._class_pns: list[np.ndarray] = []
        self._class_prefers: set[int] = set()
        if self._prefs_on:
            self.ctx.set_preference_weights(preferred_affinity_weight, prefer_no_schedule_weight)
        if self.balanced_allocation_weight:
            self.ctx.set_balanced_score(self.balanced_allocation_weight)
        self._tainted: bool | None = None  # a node of the snapshot has a NoSchedule / NoExecute taint (None: not looked yet)
        self._pa_reset()

    def _pa_reset(self) -> None:
        """Required inter-pod affinity: the snapshot's terms by constraints.term_key, in the order of their bits, each
        (term, owner namespace, topology); the profiles on the device by (match, anti, aff); the pods placed against
        the snapshot as (node index, pod, bits of its anti-affinity terms' keys); whether the device holds the tables."""
        self._pa_terms: dict[str, tuple[Any, str, int]] = {}
        self._pa_profiles: dict[tuple[int, int, int], int] = {}
        self._pa_placed: list[tuple[int, Any, list[str]]] = []
        self._pa_synced = self._pa_terms_synced = True

    @staticmethod
    def _resource_weights(resources, resource_score, resource_weights) -> list[int] | None:
        """The weights aligned with `resources` for a resource score, None without one (argument errors:
        ValueError, before any device work)."""
        if resource_score is None:
            if resource_weights is not None:
                raise ValueError("resource_weights without resource_score")
            return None
        if resource_score not in RESOURCE_SCORE_MODES or isinstance(resource_score, bool):
            raise ValueError(f"resource_score {resource_score!r}: not 'none', 'least' or 'most'")
        if resources is None:
            raise ValueError("resource_score needs resources")
        if resource_weights is None:
            return [1] * len(resources)
        if isinstance(resource_weights, Mapping):
            unknown = set(resource_weights) - set(resources)
            if unknown:
                raise ValueError(f"resource_weights names {sorted(unknown)}, not among resources {list(resources)}")
            w = [int(resource_weights.get(r, 0)) for r in resources]
        else:
            w = [int(x) for x in resource_weights]
            if len(w) != len(resources):
                raise ValueError("resource_weights: one weight per resource")
        if any(not 0 <= x <= 100 for x in w) or not any(w):
            raise ValueError("resource_weights: each in [0, 100], at least one positive")
        return w

    def close(self) -> None:
        self.ctx.close()

    # Replaces the per-cycle Nodes().List (minisched.go:40) with one device upload.
    def update_nodes(self, nodes: Iterable[Any]) -> NodeTable:
        nodes = list(nodes)
        self.nodes = pack_nodes(nodes)
        self.ctx.upload_nodes(self.nodes.unsched, self.nodes.digit)  # drops the device's columns and resources
        self._cap_synced = False
        self._res_synced = False
        self._zone_synced = False
        self._node_objs = [nodes[i] for i in self.nodes.order]
        self._class_ids, self._class_masks, self._class_synced, self._tainted = {}, [], False, None
        self._class_aff, self._class_pns, self._class_prefers = [], [], set()
        if self._pa_terms:
            self.ctx.set_pod_affinity_terms(())  # the terms belonged to the pods seen against the old snapshot
        self._pa_reset()
        return self.nodes

    def _results(self, pods: PodTable, idx, score, status) -> list[ScheduleResult]:
        assert self.nodes is not None
        n_nodes = len(self.nodes)
        fit_plugins = frozenset(
            # FitError diagnosis: the filter plugins that rejected at least one node. With the
            # device plugin set that is NodeUnschedulable whenever any node exists.
            [self.filter_plugins[0]] if (self.filter_plugins and n_nodes > 0) else [])
        out = []
        for j, name in enumerate(pods.names):
            st = int(status[j])
            if st == N.MSH_PLACED:
                i = int(idx[j])
                out.append(ScheduleResult(name, Outcome.PLACED, self.nodes.names[i], i, int(score[j])))
            elif st == N.MSH_FIT_ERROR:
                out.append(ScheduleResult(name, Outcome.FIT_ERROR, unschedulable_plugins=fit_plugins))
            else:
                out.append(ScheduleResult(name, Outcome.SCORE_ERROR))
        return out

    def schedule_batch(self, pods: Iterable[Any], nodes: Iterable[Any] | None = None) -> list[ScheduleResult]:
        """scheduleOne's selection part for every pod of the batch against one snapshot."""
        if nodes is not None:
            self.update_nodes(nodes)
        if self.nodes is None:
            raise N.MshError(N.MSH_ERR_STATE, "no node snapshot: call update_nodes() first")
        table = pack_pods(pods)
        idx, score, status = self.ctx.schedule_batch(table.digit, table.tolerates)
        return self._results(table, idx, score, status)

    def schedule_sequential(self, pods: Iterable[Any], nodes: Iterable[Any] | None = None,
                            max_pods_per_node: int = 0) -> list[ScheduleResult]:
        """One pod at a time, committing each placement to node state before the next."""
        if nodes is not None:
            self.update_nodes(nodes)
        if self.nodes is None:
            raise N.MshError(N.MSH_ERR_STATE, "no node snapshot: call update_nodes() first")
        pods = list(pods)
        table = pack_pods(pods)
        if self.nodes.allocatable_pods is not None and not self._cap_synced:
            self.ctx.upload_node_capacity(self.nodes.allocatable_pods)
            self._cap_synced = True
        results = self._schedule_sequential(pods, table, max_pods_per_node)
        # the record a later inter-pod term is evaluated against: every pod placed against the snapshot
        for p, r in zip(pods, results):
            if r.outcome == Outcome.PLACED:
                ns = K.pod_namespace(p)
                self._pa_placed.append((r.node_index, p, [K.term_key(t, ns) for t in K.pod_required_pod_anti_affinity(p)]))
        return results

    def _schedule_sequential(self, pods, table, max_pods_per_node: int) -> list[ScheduleResult]:
        """The call schedule_sequential makes for what the scheduler is configured with and what the pods ask for."""
        classes = self.pod_class_ids(pods)
        profiles = self.pod_profile_ids(pods)
        if profiles is not None:  # the snapshot has an inter-pod term: one call, whatever else is configured
            return self._schedule_balanced(pods, table, classes, max_pods_per_node, profiles)
        if self.balanced_allocation_weight:  # every pod has the balanced term: one call, whatever else is configured
            return self._schedule_balanced(pods, table, classes, max_pods_per_node)
        if (classes >= 0).any():  # a pod that some node does not admit: the class call, whatever else is configured
            return self._schedule_classes(pods, table, classes, max_pods_per_node)
        if self.resources is None and self.zones is None:
            idx, score, status = self.ctx.schedule_sequential(table.digit, table.tolerates, max_pods_per_node)
            return self._results(table, idx, score, status)
        if self.zones is not None:
            return self._schedule_spread(pods, table, max_pods_per_node)
        if not self._res_synced:
            alloc = np.array([node_allocatable(n, self.resources) for n in self._node_objs], np.int64)
            self.ctx.upload_node_resources(alloc.reshape(len(self._node_objs), len(self.resources)).T)
            self._res_synced = True
        req = np.array([pod_requests(p, self.resources) for p in pods], np.int64)
        req = req.reshape(len(pods), len(self.resources)).T
        idx, score, status = self.ctx.schedule_sequential_fit(table.digit, table.tolerates, req, max_pods_per_node)
        return self._results(table, idx, score, status)

    def node_zone_ids(self) -> tuple[np.ndarray, list[str]]:
        """The snapshot's zone column (List order; -1: the node lacks the `zones` label) and the zone names by id,
        numbered in the order in which List order first shows them."""
        names: dict[str, int] = {}
        col = np.full(len(self._node_objs), -1, np.int32)
        for i, n in enumerate(self._node_objs):
            v = _get(n, "metadata", "labels", self.zones)
            if v is not None:
                col[i] = names.setdefault(str(v), len(names))
        if len(names) > N.MAX_ZONES:
            raise ValueError(f"{len(names)} distinct values of {self.zones!r}: at most {N.MAX_ZONES} zones")
        return col, list(names)

    def pod_group_ids(self, pods: Sequence[Any]) -> np.ndarray:
        """A pod's spread group: the index in spread_groups of its `spread_label` label's value, else -1."""
        labels = [_get(p, "metadata", "labels", self.spread_label) for p in pods]
        return np.array([-1 if v is None else self._group_ids.get(str(v), -1) for v in labels], np.int32).reshape(len(pods))

    def pod_class_ids(self, pods: Sequence[Any]) -> np.ndarray:
        """A pod's class for the static node filters (constraints.node_admits: NodeName, nodeSelector, required node
        affinity, TaintToleration): pods with equal constraints.class_key share an id, ids persist for the node
        snapshot, and a class that every node admits is -1. More than MAX_POD_CLASSES classes that some node does
        not admit raise ValueError."""
        effects = ("NoSchedule", "NoExecute", "PreferNoSchedule") if self._prefs_on else ("NoSchedule", "NoExecute")
        if self._tainted is None:
            self._tainted = any(_tol_field(t, "effect") in effects for n in self._node_objs for t in K.node_taints(n))
        out = np.full(len(pods), -1, np.int32)
        n_nodes = len(self._node_objs)
        for j, p in enumerate(pods):
            # without taints the tolerations decide nothing: a pod with no other constraint needs no key
            if not self._tainted and not (K.pod_node_name(p) or K.pod_node_selector(p)
                                          or K.pod_affinity_terms(p) is not None
                                          or (self._prefs_on and K.pod_preferred_terms(p))):
                continue
            key = K.class_key(p) + K.preference_key(p) if self._prefs_on else K.class_key(p)
            cid = self._class_ids.get(key)
            if cid is None:
                mask = np.array([K.node_admits(p, n) for n in self._node_objs], bool).reshape(n_nodes)
                cid = -1
                aff = pns = None
                if self._prefs_on:  # with a preference weight a class with a nonzero raw value gets an id too
                    aff = np.array([K.preferred_affinity_score(p, n) for n in self._node_objs], np.int64).reshape(n_nodes)
                    pns = np.array([K.prefer_no_schedule_count(p, n) for n in self._node_objs], np.int64).reshape(n_nodes)
                    if max(aff.max(initial=0), pns.max(initial=0)) > 0xFFFF:
                        raise ValueError("a pod's summed preferred node affinity weights (or PreferNoSchedule taint "
                                         "count) on one node exceed 65,535")
                prefers = self._prefs_on and bool(aff.any() or pns.any())
                if not mask.all() or prefers:
                    if len(self._class_masks) >= N.MAX_POD_CLASSES:
                        raise ValueError(f"more than {N.MAX_POD_CLASSES} classes of node constraints "
                                         f"(MAX_POD_CLASSES) against one node snapshot")
                    cid = len(self._class_masks)
                    self._class_masks.append(mask)
                    self._class_synced = False
                    if self._prefs_on:
                        self._class_aff.append(aff.astype(np.uint16))
                        self._class_pns.append(pns.astype(np.uint16))
                        if prefers:
                            self._class_prefers.add(cid)
                self._class_ids[key] = cid
            out[j] = cid
        return out

    def node_class_bits(self) -> np.ndarray:
        """The snapshot's class column (List order): bit c of word i is set if node i admits class c."""
        bits = np.zeros(len(self._node_objs), np.uint64)
        for c, mask in enumerate(self._class_masks):
            bits |= mask.astype(np.uint64) << np.uint64(c)
        return bits

    def _sync_spread_inputs(self, pods):
        """The zone column and the resource table on the device; the call's requests, or None without resources."""
        if self.zones is not None and not self._zone_synced:
            self.ctx.upload_node_zones(self.node_zone_ids()[0])
            self._zone_synced = True
        req = None
        if self.resources is not None:
            if not self._res_synced:
                alloc = np.array([node_allocatable(n, self.resources) for n in self._node_objs], np.int64)
                self.ctx.upload_node_resources(alloc.reshape(len(self._node_objs), len(self.resources)).T)
                self._res_synced = True
            req = np.array([pod_requests(p, self.resources) for p in pods], np.int64)
            req = req.reshape(len(pods), len(self.resources)).T
        return req

    def _schedule_classes(self, pods, table, classes, max_pods_per_node: int) -> list[ScheduleResult]:
        req = self._sync_spread_inputs(pods)
        if not self._class_synced:
            self.ctx.upload_node_class_bits(len(self._class_masks), self.node_class_bits())
            if self._prefs_on:  # both columns, for the same classes
                self.ctx.upload_node_class_prefs(len(self._class_masks), np.array(self._class_aff, np.uint16),
                                                 np.array(self._class_pns, np.uint16))
            self._class_synced = True
        groups = self.pod_group_ids(pods) if self.zones is not None else None
        if self._class_prefers.intersection(int(c) for c in classes):  # some pod of the call has a preference
            idx, score, status = self.ctx.schedule_sequential_prefs(table.digit, table.tolerates, groups, classes, req,
                                                                    max_pods_per_node)
            return self._results(table, idx, score, status)
        idx, score, status = self.ctx.schedule_sequential_classes(table.digit, table.tolerates, groups, classes, req,
                                                                  max_pods_per_node)
        return self._results(table, idx, score, status)

    def pod_affinity_terms(self) -> list[tuple[Any, str, int]]:
        """The snapshot's inter-pod terms in the order of their bits: (term, owner namespace, topology)."""
        return list(self._pa_terms.values())

    def pod_profile_ids(self, pods: Sequence[Any]) -> np.ndarray | None:
        """A pod's profile for the required inter-pod affinity filter, or None while the snapshot has no term. New
        terms and profiles are registered (ValueError past 32 terms or 64 profiles, and for what
        constraints.check_pod_affinity refuses); the device's tables are then set again by the next call."""
        parsed = [K.check_pod_affinity(p, self.zones) for p in pods]
        terms_now = dict(self._pa_terms)  # committed only when the whole call is valid: a refused call changes nothing
        for p, (aff, anti) in zip(pods, parsed):
            ns = K.pod_namespace(p)
            for t in aff + anti:
                key = K.term_key(t, ns)
                if key not in terms_now:
                    if len(terms_now) >= N.MAX_AFFINITY_TERMS:
                        raise ValueError(f"more than {N.MAX_AFFINITY_TERMS} distinct required pod (anti-)affinity terms "
                                         f"(MAX_AFFINITY_TERMS) against one node snapshot")
                    topo = N.TOPOLOGY_HOSTNAME if _get(t, "topologyKey") == K.HOSTNAME_LABEL else N.TOPOLOGY_ZONE
                    terms_now[key] = (t, ns, topo)
        if not terms_now:
            return None
        profiles_before = dict(self._pa_profiles)
        if len(terms_now) > len(self._pa_terms):  # the profiles' match bits were taken over fewer terms
            self._pa_terms = terms_now
            self._pa_profiles = {}
            self._pa_terms_synced = self._pa_synced = False
        bit = {key: k for k, key in enumerate(self._pa_terms)}
        terms = list(self._pa_terms.values())
        out = np.full(len(pods), -1, np.int32)
        for j, (p, (aff, anti)) in enumerate(zip(pods, parsed)):
            ns = K.pod_namespace(p)
            match = sum(1 << k for k, (t, owner, _) in enumerate(terms) if K.term_matches_pod(t, owner, p))
            own = sum({1 << bit[K.term_key(t, ns)] for t in anti})
            af = bit[K.term_key(aff[0], ns)] if aff else -1
            if not (match or own or af >= 0):
                continue  # the pod reads and writes nothing of the state
            prof = (match, own, af)
            q = self._pa_profiles.get(prof)
            if q is None:
                if len(self._pa_profiles) >= N.MAX_POD_PROFILES:
                    if self._pa_terms_synced:  # no new term: the profiles are again what the device holds
                        self._pa_profiles = profiles_before
                    raise ValueError(f"more than {N.MAX_POD_PROFILES} pod profiles (MAX_POD_PROFILES) against one node "
                                     f"snapshot and term table")
                q = self._pa_profiles[prof] = len(self._pa_profiles)
                self._pa_synced = False
            out[j] = q
        return out

    def pod_affinity_state(self) -> tuple[np.ndarray, np.ndarray]:
        """(present, repel) of the pods placed against the snapshot, for the terms as they stand."""
        n = len(self._node_objs)
        present, repel = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        bit = {key: k for k, key in enumerate(self._pa_terms)}
        terms = list(self._pa_terms.values())
        for i, p, anti_keys in self._pa_placed:
            present[i] |= sum(1 << k for k, (t, owner, _) in enumerate(terms) if K.term_matches_pod(t, owner, p))
            repel[i] |= sum({1 << bit[key] for key in anti_keys})
        return present, repel

    def _sync_pod_affinity(self) -> None:
        """What changed since the last call, on the device. A new term: the terms, the profiles and the state recomputed
        from the record (setting the terms zeroes the device's state, the caller's patches with it). New profiles alone:
        the profiles, which keeps the state."""
        if self._pa_synced:
            return
        if not self._pa_terms_synced:
            self.ctx.set_pod_affinity_terms([topo for _, _, topo in self._pa_terms.values()])
        prof = list(self._pa_profiles)
        self.ctx.set_pod_profiles([m for m, _, _ in prof], [a for _, a, _ in prof], [f for _, _, f in prof])
        if not self._pa_terms_synced and self._pa_placed:
            self.ctx.upload_pod_affinity_state(*self.pod_affinity_state())
        self._pa_synced = self._pa_terms_synced = True

    def _schedule_balanced(self, pods, table, classes, max_pods_per_node: int, profiles=None) -> list[ScheduleResult]:
        """DeviceContext.schedule_sequential_balanced with whatever the scheduler is configured with: the class
        columns if some pod of the snapshot has a class, the groups with zones, the requests always. With profiles:
        DeviceContext.schedule_sequential_podaffinity."""
        req = self._sync_spread_inputs(pods)
        classed = bool(self._class_masks)
        if classed and not self._class_synced:
            self.ctx.upload_node_class_bits(len(self._class_masks), self.node_class_bits())
            if self._prefs_on:  # both columns, for the same classes
                self.ctx.upload_node_class_prefs(len(self._class_masks), np.array(self._class_aff, np.uint16),
                                                 np.array(self._class_pns, np.uint16))
            self._class_synced = True
        groups = self.pod_group_ids(pods) if self.zones is not None else None
        if profiles is None:
            idx, score, status = self.ctx.schedule_sequential_balanced(table.digit, table.tolerates, groups,
                                                                       classes if classed else None, req, max_pods_per_node)
            return self._results(table, idx, score, status)
        if self.zones is None and any(topo == N.TOPOLOGY_ZONE for _, _, topo in self._pa_terms.values()):
            raise ValueError("a pod (anti-)affinity term on a zone needs the scheduler's `zones` label")
        self._sync_pod_affinity()
        idx, score, status = self.ctx.schedule_sequential_podaffinity(table.digit, table.tolerates, groups,
                                                                      classes if classed else None, profiles, req,
                                                                      max_pods_per_node)
        return self._results(table, idx, score, status)

    def _schedule_spread(self, pods, table, max_pods_per_node: int) -> list[ScheduleResult]:
        req = self._sync_spread_inputs(pods)
        idx, score, status = self.ctx.schedule_sequential_spread_scored(table.digit, table.tolerates,
                                                                        self.pod_group_ids(pods), req, max_pods_per_node)
        return self._results(table, idx, score, status)
