"""A CPU stand-in for DeviceContext that holds the uploaded columns and answers every schedule_sequential* call that
Scheduler makes through podaffinity_ref.per_pod, the superset column reference (checked against the kernels by the GPU
tests of each entry point). What an entry point does not have is switched off, as the mirrors of the GPU tests map it:
the plain call reads no resources, _fit adds the table and the resource score, _spread_scored the groups, _classes the
class column, _prefs the two preference weights, _balanced the balanced weight, _podaffinity the profiles. The setters,
uploads and read-backs are the ones Scheduler touches; `calls` records every name in order. Test infrastructure only.

A call the library would refuse (groups without a zone column, classes without a class column, a resource score
without requests, profiles without terms) is an AssertionError here: the differential never expects one."""
from __future__ import annotations

import numpy as np

import node_capacity_ref as CR
import podaffinity_ref as PA
import spread_ref as S

MODES = {"none": PA.NONE, "least": PA.LEAST, "most": PA.MOST, 0: 0, 1: 1, 2: 2}


class ColumnCtx:
    def __init__(self, O):
        self.O = O
        self.calls: list[str] = []
        self.ps = O.PluginSet()
        self.n_nodes = 0
        self.u = self.nd = None
        self.mode, self.weight, self.rw = PA.NONE, 1, []
        self.skew: list[int] = []
        self.w = (0, 0)
        self.wb = 0
        self.topo: list[int] = []
        self.prof = ((), (), ())
        self._drop()

    def _drop(self):
        """What upload_nodes drops: every column and the counts; the settings, terms and profiles stay."""
        n = self.n_nodes
        self.cap = self.alloc = self.used = self.zone = self.bits = self.A = self.T = None
        self.C = self.PC = 0
        self.counts = np.zeros(n, np.int32)
        self.cnt = np.zeros((len(self.skew), S.MAX_ZONES), np.int32)
        self.st = PA.State(n, self.topo, *self.prof)

    # -- configuration and uploads --
    def set_plugins(self, filters, prescore, score):
        self.calls.append("set_plugins")
        self.ps = self.O.PluginSet(list(filters), list(prescore), [c.name for c in score], [int(c.weight) for c in score],
                                   [int(c.normalize) for c in score])

    def set_tiebreak(self, mode, seed=0, counter=0):
        self.calls.append("set_tiebreak")
        assert mode in ("first", 0), "the sequential calls refuse the random tie-break"

    def upload_nodes(self, unsched, digit):
        self.calls.append("upload_nodes")
        self.u, self.nd = np.array(unsched, np.uint8), np.array(digit, np.int8)
        self.n_nodes = len(self.u)
        self._drop()

    def upload_node_capacity(self, cap):
        self.calls.append("upload_node_capacity")
        assert len(cap) == self.n_nodes
        self.cap = np.array(cap, np.int64)

    def upload_node_resources(self, alloc, used=None):
        self.calls.append("upload_node_resources")
        self.alloc = np.array(alloc, np.int64)
        assert self.alloc.ndim == 2 and self.alloc.shape[1] == self.n_nodes
        self.used = np.zeros_like(self.alloc) if used is None else np.array(used, np.int64)

    def set_resource_score(self, mode, weight=1, resource_weights=None):
        self.calls.append("set_resource_score")
        self.mode, self.weight, self.rw = MODES[mode], int(weight), [int(x) for x in resource_weights]

    def set_spread_groups(self, max_skew):
        self.calls.append("set_spread_groups")
        self.skew = [int(x) for x in max_skew]
        self.cnt = np.zeros((len(self.skew), S.MAX_ZONES), np.int32)

    def upload_node_zones(self, zone):
        self.calls.append("upload_node_zones")
        assert len(zone) == self.n_nodes
        self.zone = np.array(zone, np.int32)
        self.cnt[:] = 0

    def upload_node_class_bits(self, n_classes, bits):
        self.calls.append("upload_node_class_bits")
        assert len(bits) == self.n_nodes and 1 <= n_classes <= 64
        self.C, self.bits = int(n_classes), np.array(bits, np.uint64)

    def upload_node_class_prefs(self, n_classes, affinity=None, taints=None):
        self.calls.append("upload_node_class_prefs")
        shape = (int(n_classes), self.n_nodes)
        self.PC = int(n_classes)
        self.A = np.zeros(shape, np.int64) if affinity is None else np.array(affinity, np.int64).reshape(shape)
        self.T = np.zeros(shape, np.int64) if taints is None else np.array(taints, np.int64).reshape(shape)

    def set_preference_weights(self, affinity=0, taint=0):
        self.calls.append("set_preference_weights")
        self.w = (int(affinity), int(taint))

    def set_balanced_score(self, weight=0):
        self.calls.append("set_balanced_score")
        self.wb = int(weight)

    def set_pod_affinity_terms(self, topologies=()):
        self.calls.append("set_pod_affinity_terms")
        self.topo, self.prof = [int(t) for t in topologies], ((), (), ())
        self.st = PA.State(self.n_nodes, self.topo)

    def set_pod_profiles(self, match=(), anti=(), aff=()):
        self.calls.append("set_pod_profiles")
        assert self.topo, "profiles need terms"
        self.prof = (list(match), list(anti), list(aff))
        self.st.set_profiles(*self.prof)

    def upload_pod_affinity_state(self, present=None, repel=None):
        self.calls.append("upload_pod_affinity_state")
        assert self.topo
        self.st.present[:] = 0 if present is None else np.asarray(present, np.int64)
        self.st.repel[:] = 0 if repel is None else np.asarray(repel, np.int64)

    # -- read-backs --
    def node_pod_counts(self):
        return self.counts.copy()

    def node_resources(self):
        return None if self.alloc is None else (self.alloc.copy(), self.used.copy())

    def spread_counts(self):
        return self.cnt.copy()

    def pod_affinity_state(self):
        return self.st.present.astype(np.uint32), self.st.repel.astype(np.uint32)

    def pod_affinity_terms(self):
        return np.array(self.topo, np.uint8)

    def close(self):
        pass

    # -- the sequential entry points --
    def _run(self, name, pd, pt, grp, cls, prf, req, scalar, scored=True, prefs=False, balanced=False):
        self.calls.append(name)
        n, p = self.n_nodes, len(pd)
        assert self.u is not None, "upload_nodes has not been called"
        if self.cap is None:
            eff = np.full(n, scalar, np.int64) if scalar > 0 else S.no_limit(n)
        else:
            eff = CR.effective(self.cap, scalar)
        mode = self.mode if scored else PA.NONE
        if req is None:
            assert mode == PA.NONE and not (balanced and self.wb), f"{name}: a score that needs requests, and none given"
            a, us, rq = S.no_res(n, p)
        else:
            assert self.alloc is not None, f"{name}: requests without a resource table"
            a, us, rq = self.alloc, self.used, np.asarray(req, np.int64)
            assert rq.shape == (a.shape[0], p)
        assert grp is None or self.zone is not None or not len(self.skew), f"{name}: groups without a zone column"
        assert cls is None or self.bits is not None or self.A is not None, f"{name}: classes without a column"
        if prf is not None:
            assert self.topo and len(self.st.match), f"{name}: profiles without terms or profiles"
            assert not any(self.topo) or self.zone is not None, f"{name}: a zone term without a zone column"
        w = self.w if prefs else (0, 0)
        state = self.st if prf is not None else PA.State(n, [])
        out = PA.per_pod(self.O, self.u, self.nd, np.asarray(pd, np.int8), np.asarray(pt, np.uint8), self.ps, eff, a, us,
                         rq, self.zone, grp, self.skew, mode, self.weight, self.rw, self.bits if cls is not None else None,
                         max(self.C, self.PC), cls, self.A if prefs else None, self.T if prefs else None, *w, None, 0,
                         self.wb if balanced else 0, state, prf, self.counts, self.cnt)
        idx, score, status, self.counts, us, self.cnt = out
        if req is not None:
            self.used = us
        return idx, score, status

    def schedule_sequential(self, pd, pt, max_pods_per_node=0):
        return self._run("schedule_sequential", pd, pt, None, None, None, None, max_pods_per_node, scored=False)

    def schedule_sequential_fit(self, pd, pt, req, max_pods_per_node=0):
        return self._run("schedule_sequential_fit", pd, pt, None, None, None, req, max_pods_per_node)

    def schedule_sequential_spread_scored(self, pd, pt, grp, req=None, max_pods_per_node=0):
        return self._run("schedule_sequential_spread_scored", pd, pt, grp, None, None, req, max_pods_per_node)

    def schedule_sequential_classes(self, pd, pt, grp=None, cls=None, req=None, max_pods_per_node=0):
        return self._run("schedule_sequential_classes", pd, pt, grp, cls, None, req, max_pods_per_node)

    def schedule_sequential_prefs(self, pd, pt, grp=None, cls=None, req=None, max_pods_per_node=0):
        return self._run("schedule_sequential_prefs", pd, pt, grp, cls, None, req, max_pods_per_node, prefs=True)

    def schedule_sequential_balanced(self, pd, pt, grp=None, cls=None, req=None, max_pods_per_node=0):
        return self._run("schedule_sequential_balanced", pd, pt, grp, cls, None, req, max_pods_per_node, prefs=True,
                         balanced=True)

    def schedule_sequential_podaffinity(self, pd, pt, grp=None, cls=None, prf=None, req=None, max_pods_per_node=0):
        return self._run("schedule_sequential_podaffinity", pd, pt, grp, cls, prf, req, max_pods_per_node, prefs=True,
                         balanced=True)
