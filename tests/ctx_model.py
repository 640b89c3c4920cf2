"""A plain model of one msh_ctx: what include/minisched_hip.h documents a context to carry from call to call, as
numpy arrays and Python ints, with one method per operation. Test infrastructure only.

Every operation returns ("ok", outputs) or ("err", code); on an error the model is left untouched. Placements come
only from the references the suite already has: oracle.c_schedule_batch (FIRST mode, score columns included),
tiebreak_ref.pick (RANDOM mode), node_capacity_ref.via_oracle / serial (plain sequential calls),
resource_fit_ref.per_pod / serial (unscored _fit calls) and resource_score_ref.per_pod / serial (scored ones). The
model adds the bookkeeping between them: which table the call sees, which counts / capacities / amounts it starts
from, which refusal comes first, and what every read-back returns afterwards.

`mutant` (a name of MUTANTS) makes one deliberate mistake of the kind a library bug in that bookkeeping would make;
tests/test_ctx_model.py shows that the fixed trace set tells every mutant from the true model.
"""
from __future__ import annotations

import copy

import numpy as np

import node_capacity_ref as C
import resource_fit_ref as R
import resource_score_ref as S
import tiebreak_ref as T

OK, INVALID, STATE, UNSUPPORTED = 0, -1, -4, -5  # msh_err
FIRST, RANDOM = 0, 1                              # msh_tiebreak
COLS = ["ScoreColumn0", "ScoreColumn1", "ScoreColumn2", "ScoreColumn3"]
RESOURCE_MAX, SCORE_MAX = 1 << 62, 1 << 55
SERIAL_PAIRS = 2 * 10**4  # the literal loops below this many (pod, node) pairs, the numpy / C forms above

MUTANTS = (
    "upload_keeps_counts", "upload_keeps_capacity", "upload_keeps_resources", "rewrite_from_previous_version",
    "column_lost_on_patch", "column_lost_on_plugin_change", "filter_change_without_reprep",
    "multi_batch_keeps_counter", "refused_call_advances_counter", "pair_form_commits_nothing",
    "replicas_dropped_not_folded", "used_not_carried_to_scored", "reset_zeroes_used", "patch_lowers_res_max",
    "clear_capacity_stays_in_force", "failed_call_applies",
)


def fit_max_nodes(nres: int, scored: bool) -> int:
    """msh_seq_fit_max_nodes as the header states it."""
    base = 8192 if nres <= 2 else 4096
    return base // 2 if scored else base


def err(code):
    return ("err", code)


class CtxModel:
    def __init__(self, O, mutant: str | None = None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.O, self.mutant = O, mutant
        self.filters, self.prescore = ["NodeUnschedulable"], ["NodeNumber"]
        self.score = [("NodeNumber", 1, 0)]  # (name, weight, normalize)
        self.tb = (FIRST, 0, 0)
        self.have_nodes = False
        self.u = self.nd = None
        self.cols = {}  # k -> int64 column, uploaded since the last msh_upload_nodes
        self.counts = None
        self.cap = None
        self.alloc = self.used = None
        self.res_max = 0
        self.rs = (S.NONE, 1, [])
        # what only mutants read
        self._prev = None            # the table version before the last rewrite
        self._plane_nu = True        # the filter list the planes were last derived from
        self._pending = None         # counts committed by pair-form calls and not folded yet
        self._used_pre = None        # `used` before the last unscored _fit call
        self._cap_force = None       # a cleared column still in force

    def clone(self):
        return copy.copy(self)  # shallow is enough: every operation replaces the arrays it changes

    def _is(self, name):
        return self.mutant == name

    # ---- derived ----
    @property
    def n(self):
        return len(self.u)

    @property
    def generic(self):
        return any(s in COLS for s, _, _ in self.score)

    def _ps(self):
        nu = self._plane_nu if self._is("filter_change_without_reprep") else ("NodeUnschedulable" in self.filters)
        return self.O.PluginSet(filters=["NodeUnschedulable"] if nu else [], prescore=list(self.prescore),
                                score=[s for s, _, _ in self.score], weights=[w for _, w, _ in self.score],
                                normalize=[m for _, _, m in self.score])

    # ---- configuration ----
    def set_plugins(self, filters, prescore, score):
        nu_before = "NodeUnschedulable" in self.filters
        self.filters, self.prescore, self.score = list(filters), list(prescore), [tuple(s) for s in score]
        if self.have_nodes and nu_before != ("NodeUnschedulable" in self.filters):
            self._rewrite(lambda u, nd, cols: None)  # the planes are re-derived: a rewrite of the table
        if self._is("column_lost_on_plugin_change"):
            self.cols = {}
        return ("ok", None)

    def set_tiebreak(self, mode, seed, counter):
        self.tb = (int(mode), int(seed) & T.M64, int(counter) & T.M64)
        return ("ok", None)

    def set_resource_score(self, mode, weight, rw):
        if mode == S.NONE:
            self.rs = (S.NONE, self.rs[1], self.rs[2])
            return ("ok", None)
        rw = [int(x) for x in rw]
        bad = (not 1 <= weight <= 1 << 32 or not 1 <= len(rw) <= 4 or any(not 0 <= x <= 100 for x in rw) or not any(rw))
        if bad and not (self._is("failed_call_applies") and 1 <= len(rw) <= 4):
            return err(INVALID)
        if bad:  # the mutant's applied setting, kept within what a scored call can divide by
            weight, rw = min(max(weight, 1), 1 << 32), [min(max(x, 1), 100) for x in rw]
        self.rs = (int(mode), int(weight), rw)
        return err(INVALID) if bad else ("ok", None)

    # ---- the node table ----
    def _rewrite(self, change):
        """A patch, a score column or a filter-list change: the other table version built from the current one."""
        cur = (self.u, self.nd, self.cols)
        base = self._prev if self._is("rewrite_from_previous_version") and self._prev is not None else cur
        u, nd, cols = base[0].copy(), base[1].copy(), dict(base[2])
        change(u, nd, cols)
        self._prev, (self.u, self.nd, self.cols) = cur, (u, nd, cols)

    def upload_nodes(self, u, nd):
        n = len(u)

        def kept(a, fill=0):  # a mutant's stale array, cut or padded to the new table
            out = np.full(a.shape[:-1] + (n,), fill, a.dtype)
            m = min(n, a.shape[-1])
            out[..., :m] = a[..., :m]
            return out

        stale = self.have_nodes
        if not (stale and self._is("upload_keeps_counts")):
            self.counts = np.zeros(n, np.int32)
        else:
            self.counts = kept(self.counts)
        self.cap = kept(self.cap) if stale and self._is("upload_keeps_capacity") and self.cap is not None else None
        if stale and self._is("upload_keeps_resources") and self.alloc is not None:
            self.alloc, self.used = kept(self.alloc), kept(self.used)
        else:
            self.alloc = self.used = None
        self.u, self.nd, self.cols = np.array(u, np.uint8), np.array(nd, np.int8), {}
        self.have_nodes = True
        self._prev, self._pending, self._used_pre, self._cap_force = None, None, None, None
        self._plane_nu = "NodeUnschedulable" in self.filters
        return ("ok", None)

    def patch_nodes(self, idx, u, nd):
        if not self.have_nodes:
            return err(STATE)

        def change(tu, tnd, cols):
            tu[idx], tnd[idx] = u, nd
            if self._is("column_lost_on_patch"):
                cols.clear()

        self._rewrite(change)
        if len(idx) > 64:  # scattered and fully re-prepped
            self._plane_nu = "NodeUnschedulable" in self.filters
        return ("ok", None)

    def upload_score_column(self, k, scores):
        if not self.have_nodes:
            return err(STATE)
        self._rewrite(lambda u, nd, cols: cols.__setitem__(int(k), np.array(scores, np.int64)))
        return ("ok", None)

    # ---- counts, capacity column, resource table ----
    def reset_node_pod_counts(self):
        if not self.have_nodes:
            return err(STATE)
        self.counts = np.zeros(self.n, np.int32)
        self._pending = None
        if self._is("reset_zeroes_used") and self.used is not None:
            self.used = np.zeros_like(self.used)
        return ("ok", None)

    def upload_node_capacity(self, cap):
        if not self.have_nodes:
            return err(STATE)
        cap = np.array(cap, np.int64)
        bad = bool((cap < 0).any())
        if bad and not self._is("failed_call_applies"):
            return err(INVALID)
        self.cap, self._cap_force = np.maximum(cap, 0), None
        return err(INVALID) if bad else ("ok", None)

    def patch_node_capacity(self, idx, cap):
        if not self.have_nodes or self.cap is None:
            return err(STATE)
        cap = np.array(cap, np.int64)
        bad = bool((cap < 0).any())
        if bad and not self._is("failed_call_applies"):
            return err(INVALID)
        self.cap = self.cap.copy()
        self.cap[idx] = np.maximum(cap, 0)
        return err(INVALID) if bad else ("ok", None)

    def clear_node_capacity(self):
        if self._is("clear_capacity_stays_in_force") and self.cap is not None:
            self._cap_force = self.cap
        self.cap = None
        return ("ok", None)

    def upload_node_resources(self, alloc, used=None):
        if not self.have_nodes:
            return err(STATE)
        self.alloc = np.array(alloc, np.int64)
        self.used = np.zeros_like(self.alloc) if used is None else np.array(used, np.int64)
        self.res_max = int(max(self.alloc.max(initial=0), self.used.max(initial=0)))
        self._used_pre = None
        return ("ok", None)

    def patch_node_resources(self, idx, alloc=None, used=None):
        if not self.have_nodes or self.alloc is None:
            return err(STATE)
        if alloc is None and used is None:
            return err(INVALID)
        top = 0
        if alloc is not None:
            self.alloc = self.alloc.copy()
            self.alloc[:, idx] = alloc
            top = max(top, int(np.max(alloc, initial=0)))
        if used is not None:
            self.used = self.used.copy()
            self.used[:, idx] = used
            top = max(top, int(np.max(used, initial=0)))
        self.res_max = top if self._is("patch_lowers_res_max") else max(self.res_max, top)
        self._used_pre = None
        return ("ok", None)

    def clear_node_resources(self):
        self.alloc = self.used = None
        self._used_pre = None
        return ("ok", None)

    # ---- batch entry points ----
    def _refused(self, code, p):
        if self.tb[0] == RANDOM and self._is("refused_call_advances_counter"):
            self.tb = (RANDOM, self.tb[1], (self.tb[2] + p) & T.M64)
        return err(code)

    def _batch(self, pd, pt, advance=True):
        p = len(pd)
        mode, seed, counter = self.tb
        if mode == RANDOM and self.generic:
            return self._refused(UNSUPPORTED, p)
        if not self.have_nodes:
            return self._refused(STATE, p)
        ps = self._ps()
        if mode == RANDOM:
            out = T.pick(self.u, self.nd, pd, pt, ps, seed, counter)
            if advance:
                self.tb = (mode, seed, (counter + p) & T.M64)
            return ("ok", out)
        if any(s in COLS and COLS.index(s) not in self.cols for s in ps.score):
            return err(STATE)
        return ("ok", self.O.c_schedule_batch(self.u, self.nd, pd, pt, ps, cols=self.cols)[:3])

    def schedule_batch(self, pd, pt):
        return self._batch(pd, pt)

    def schedule_batches_device(self, pd, pt, cuts):
        """The pods cut into consecutive batches at `cuts`: batch i draws where batch i - 1 ended, so the whole
        submission is one batch over all its pods."""
        return self._batch(pd, pt, advance=not self._is("multi_batch_keeps_counter"))

    # ---- sequential-commit mode ----
    def _eff(self, scalar):
        cap = self.cap if self.cap is not None else self._cap_force
        if cap is not None:
            return C.effective(cap, scalar)
        return np.full(self.n, scalar, np.int64) if scalar > 0 else None

    def _fold(self):
        """A call that reads the counts in order: whatever pair-form calls left in the replicas is folded first."""
        if self._pending is not None and self._is("replicas_dropped_not_folded"):
            self.counts = (self.counts - self._pending).astype(np.int32)
        self._pending = None

    @staticmethod
    def _cb(cb, out):
        idx, score, status = out
        return [(int(j), int(idx[j]), int(score[j])) for j in np.flatnonzero(status == 0)] if cb else None

    def schedule_sequential(self, pd, pt, scalar=0, cb=False):
        p = len(pd)
        if self.tb[0] == RANDOM:
            return self._refused(UNSUPPORTED, p)
        if not self.have_nodes:
            return err(STATE)
        if self.generic:
            return err(UNSUPPORTED)
        eff = self._eff(scalar)
        pair_form = eff is None and p > 64
        if not pair_form:
            self._fold()
        k = self.counts.astype(np.int64)
        lim = k + p + 1  # no run of p pods reaches it: "no limit" within the oracle's int32 head-room
        eff = lim if eff is None else np.minimum(eff, lim)
        ref = C.serial if self.n * p <= SERIAL_PAIRS // 10 else C.via_oracle
        idx, score, status, after = ref(self.O, self.u, self.nd, pd, pt, self._ps(), eff, k)
        if pair_form:
            if self._is("pair_form_commits_nothing"):
                after = self.counts
            delta = after.astype(np.int64) - k
            self._pending = delta if self._pending is None else self._pending + delta
        self.counts = np.array(after, np.int32)
        return ("ok", (idx, score, status, self._cb(cb, (idx, score, status))))

    def schedule_sequential_fit(self, pd, pt, req, scalar=0, cb=False):
        p, nres = len(pd), len(req)
        mode, weight, rw = self.rs
        scored = mode != S.NONE
        if self.tb[0] == RANDOM:
            return self._refused(UNSUPPORTED, p)
        if not self.have_nodes:
            return err(STATE)
        if self.generic:
            return err(UNSUPPORTED)
        if self.alloc is None:
            return err(STATE)
        if nres != len(self.alloc):
            return err(INVALID)
        if scored and len(rw) != nres:
            return err(STATE)
        if self.n > fit_max_nodes(nres, scored):
            return err(UNSUPPORTED)
        if scored and self.res_max > SCORE_MAX:
            return err(UNSUPPORTED)
        req = np.asarray(req, np.int64)
        if (req < 0).any() or (req > (SCORE_MAX if scored else RESOURCE_MAX)).any():
            return err(INVALID)
        self._fold()
        eff = self._eff(scalar)
        eff = R.no_limit(self.n) if eff is None else eff
        used = self.used
        if scored and self._used_pre is not None and self._is("used_not_carried_to_scored"):
            used = self._used_pre
        small = self.n * p <= SERIAL_PAIRS
        args = (self.O, self.u, self.nd, pd, pt, self._ps(), eff, self.alloc, used, req)
        if scored:
            out = (S.serial if small else S.per_pod)(*args, mode, weight, rw, self.counts)
        else:
            out = (R.serial if small else R.per_pod)(*args, self.counts)
        idx, score, status, cnt, us = out
        self._used_pre = None if scored else self.used
        self.counts, self.used = np.array(cnt, np.int32), np.array(us, np.int64)
        return ("ok", (idx, score, status, self._cb(cb, (idx, score, status))))

    # ---- read-backs ----
    def node_pod_counts(self):
        if not self.have_nodes:
            return err(STATE)
        self._pending = None  # the read folds the replicas
        return ("ok", self.counts.copy())

    def node_capacity(self):
        return ("ok", None if self.cap is None else self.cap.astype(np.int32))

    def node_resources(self):
        return ("ok", None if self.alloc is None else (self.alloc.copy(), self.used.copy()))

    def tiebreak(self):
        return ("ok", self.tb)

    def resource_score(self):
        return ("ok", (self.rs[0], self.rs[1], list(self.rs[2])))

    READS = ("node_pod_counts", "node_capacity", "node_resources", "tiebreak", "resource_score")

    def apply(self, op, args):
        """One step of a trace. A refused step leaves the model as it was (a mutant may say otherwise)."""
        return getattr(self, op)(**args)


def same_value(a, b) -> bool:
    """Deep equality of two results of CtxModel methods (tuples, lists, arrays, ints, None)."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and bool((a == b).all())
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return (isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b)
                and all(same_value(x, y) for x, y in zip(a, b)))
    return a == b
