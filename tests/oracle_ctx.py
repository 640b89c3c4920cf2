"""Test infrastructure: a DeviceContext stand-in computed by the CPU oracle.

Used only to exercise the HOST logic around the device path (queue, node cache, Permit/Bind,
the loop) on machines without a GPU, and as the checker the GPU pipeline tests compare
against. It is never importable from the product package.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O


class OracleCtx:
    def __init__(self):
        self.plugins = O.PluginSet()
        self.unsched = np.zeros(0, np.uint8)
        self.digit = np.zeros(0, np.int8)
        self.calls: list[tuple] = []
        self.n_nodes = 0

    def close(self) -> None:
        pass

    def set_plugins(self, filters, prescore, score) -> None:
        self.plugins = O.PluginSet(list(filters), list(prescore), [c.name for c in score],
                                   [int(c.weight) for c in score], [int(c.normalize) for c in score])
        self.calls.append(("set_plugins",))

    def upload_nodes(self, unsched, digit) -> None:
        self.unsched = np.array(unsched, np.uint8)
        self.digit = np.array(digit, np.int8)
        self.n_nodes = len(self.unsched)
        self.counts = np.zeros(self.n_nodes, np.int32)  # an upload zeroes the sequential-mode counts
        self.cols = {}                                  # and drops the score columns
        self.calls.append(("upload", len(self.unsched)))

    def patch_nodes(self, idx, unsched, digit) -> None:
        idx = np.asarray(idx, np.int64)
        assert len(np.unique(idx)) == len(idx) and (idx >= 0).all() and (idx < self.n_nodes).all()
        self.unsched[idx] = unsched
        self.digit[idx] = digit
        self.calls.append(("patch", sorted(int(i) for i in idx)))

    def schedule_batch(self, pod_digit, pod_tol):
        idx, score, status, _ = O.c_schedule_batch(self.unsched, self.digit, pod_digit, pod_tol, self.plugins,
                                                   cols=getattr(self, "cols", None))
        self.calls.append(("batch", len(pod_digit)))
        return idx, score, status

    # -- what tests/table_readback.py drives besides the calls above (additive: the methods above return and
    #    append to `calls` what they did) --
    def _counts(self) -> np.ndarray:
        if getattr(self, "counts", None) is None:  # no upload yet
            self.counts = np.zeros(self.n_nodes, np.int32)
        return self.counts

    def upload_score_column(self, name, scores) -> None:
        scores = np.array(scores, np.int64)
        assert len(scores) == self.n_nodes and self.n_nodes > 0
        if getattr(self, "cols", None) is None:
            self.cols = {}
        self.cols[int(name[len("ScoreColumn"):])] = scores

    def schedule_sequential(self, pod_digit, pod_tol, max_pods_per_node=0, on_commit=None, out=None):
        """The C oracle's serial loop; the counts carry over from call to call as the device's do."""
        idx, score, status, counts = O.c_schedule_sequential(self.unsched, self.digit, pod_digit, pod_tol, self.plugins,
                                                             int(max_pods_per_node), self._counts().copy())
        self.counts = np.array(counts[:self.n_nodes], np.int32)
        if on_commit:
            for j in np.flatnonzero(status == O.PLACED):
                on_commit(int(j), int(idx[j]), int(score[j]))
        return idx, score, status

    def node_pod_counts(self) -> np.ndarray:
        return self._counts().copy()

    def reset_node_pod_counts(self) -> None:
        self.counts = np.zeros(self.n_nodes, np.int32)

    def export_results(self, pod_digit, pod_tol):
        """msh_export_results by oracle.py's Python path: per pod the filter verdict of every node, NodeNumber's raw
        score on the feasible ones, and `normalize` of that list times the weight; EXPORT_NONE where the reference
        records no score (a filtered node, or a pod that never reaches Score)."""
        none = -(1 << 63)
        ps = self.plugins
        assert not any(s.startswith("ScoreColumn") for s in ps.score), "export runs on lists without a score column"
        has_nu = "NodeUnschedulable" in ps.filters
        k = ps.score.index("NodeNumber") if "NodeNumber" in ps.score else -1
        p, n = len(pod_digit), self.n_nodes
        filt = np.ones((p, n), np.uint8)
        raw = np.full((p, n), none, np.int64)
        fin = np.full((p, n), none, np.int64)
        for j in range(p):
            pd = int(pod_digit[j])
            if has_nu and not pod_tol[j]:
                filt[j] = self.unsched == 0
            feas = np.flatnonzero(filt[j])
            if k < 0 or "NodeNumber" not in ps.prescore or not 0 <= pd <= 9 or feas.size == 0:
                continue
            lst = [10 if int(d) == pd else 0 for d in self.digit[feas]]
            raw[j, feas] = lst
            fin[j, feas] = [O._wrap64(v * ps.weights[k]) for v in O.normalize(ps.normalize[k], lst)]
        return filt, raw, fin
