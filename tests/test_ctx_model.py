"""Seeded call traces over one context, and what the model (tests/ctx_model.py) says about them, on the CPU.

`traces(seed0, count)` builds lists of (op, args) steps from numpy.random.default_rng(seed): it tracks only what it
needs to pass well-formed arguments (the table size, whether a column / a resource table is present, ...), never a
placement, and knows nothing of the library. tests/test_ctx_trace_gpu.py replays the fixed set TRACE_SET on the
device; here the set itself is checked: that it covers the operations and the transitions between the sequential
forms, that capacity and requests bind, that few steps are refused, and that every mutant of the model (one
deliberate bookkeeping mistake each) is told from the true model by at least three traces. The model is also run on
the sequences scripted in test_resource_score_gpu / test_node_capacity_gpu / test_resource_fit_gpu and reproduces
what those tests expect.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ctx_model as M
import node_capacity_ref as CR
import resource_fit_ref as R
import resource_score_ref as S

TRACE_SEED0, TRACE_COUNT = 20261200, 12  # the fixed set (the count: see test_ctx_trace_gpu's docstring)
LADDER = [1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769]
PLUGIN_COMBOS = [  # test_gpu_parity's five lists
    (["NodeUnschedulable"], ["NodeNumber"], ["NodeNumber"]),
    ([], ["NodeNumber"], ["NodeNumber"]),
    (["NodeUnschedulable"], [], ["NodeNumber"]),
    (["NodeUnschedulable"], ["NodeNumber"], []),
    ([], [], []),
]
WEIGHTS = [1, 3, 1 << 32]
READS = M.CtxModel.READS
SEQ_KINDS = ("pairs", "short", "capacity", "fit")  # plain cap 0 p > 64, plain cap 0 p <= 64, plain with a capacity, _fit
DE_BRUIJN = [0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3]  # cyclic: every ordered pair of 4 symbols once


class Gen:
    """One trace under construction: the steps, and the little the next step's arguments depend on."""

    def __init__(self, rng):
        self.rng, self.steps = rng, []
        self.n = None
        self.nres = None
        self.has_cap = False
        self.random = False
        self.score = [("NodeNumber", 1, 0)]
        self.filters = ["NodeUnschedulable"]
        self.cols = set()
        self.rs = (0, 0)  # (mode, nres)
        self.unit = 1          # the resource table's unit (1 or 2^33)
        self.over55 = False    # an amount past 2^55 written since the last resource upload
        self.over55_at = None  # ... and the node it went to
        self.burst_done = False

    def emit(self, op, **args):
        self.steps.append((op, args))

    @property
    def generic(self):
        return any(s in M.COLS for s, _, _ in self.score)

    # -- draws --
    def pods(self, p, digits=10):
        r = self.rng
        pd = r.integers(-1 if r.random() < 0.25 else 0, digits, p).astype(np.int8)
        return pd, (r.random(p) < 0.4).astype(np.uint8)

    def pod_count(self, kind=None):
        r = self.rng
        long = int(r.integers(180, 261)) if self.n <= 1100 else int(r.integers(100, 131))
        if kind == "pairs":
            return int(r.choice([65, 65, long, int(r.integers(66, 131))]))
        if kind == "short":
            return int(r.choice([1, 63, 64]))
        return int(r.choice([1, 63, 64, 65, long]))

    # -- configuration --
    def plugins(self, kind="nn", toggle_filter=False):
        r = self.rng
        if kind == "nn":
            f, pre, sc = PLUGIN_COMBOS[int(r.choice([0, 0, 0, 1, 1, 2, 3, 4]))]
            score = [(s, int(r.choice(WEIGHTS)), int(r.integers(0, 4))) for s in sc]
        else:  # a list naming ScoreColumn0 / 1: the generic pipeline
            f, pre = (["NodeUnschedulable"] if r.random() < 0.7 else []), ["NodeNumber"]
            names = ["NodeNumber"] * int(r.random() < 0.7) + ["ScoreColumn0"] + ["ScoreColumn1"] * int(r.random() < 0.5)
            score = [(str(s), int(r.choice(WEIGHTS)), int(r.integers(0, 4))) for s in r.permutation(names)]
        if toggle_filter:
            f = [] if self.filters else ["NodeUnschedulable"]
        self.filters, self.score = list(f), score
        self.emit("set_plugins", filters=list(f), prescore=list(pre), score=score)

    def tiebreak(self, random):
        r = self.rng
        self.random = random
        self.emit("set_tiebreak", mode=int(random), seed=int(r.integers(0, 1 << 62)) if random else 0,
                  counter=[0, 5, (1 << 64) - 40][int(r.integers(0, 3))] if random else 0)

    def resource_score(self, mode=None, nres=None, invalid=False):
        r = self.rng
        mode = int(r.integers(1, 3)) if mode is None else mode
        if mode == 0:
            self.rs = (0, self.rs[1])
            return self.emit("set_resource_score", mode=0, weight=0, rw=[])
        nres = (self.nres or 2) if nres is None else nres
        rw = [int(x) for x in r.integers(0, 101, nres)]
        rw[int(r.integers(0, nres))] = int(r.integers(1, 101))
        if invalid:  # every weight 0: MSH_ERR_INVALID, the setting stays
            return self.emit("set_resource_score", mode=mode, weight=1, rw=[0] * nres)
        self.rs = (mode, nres)
        self.emit("set_resource_score", mode=mode, weight=int(r.choice([1, 2, 7, 1 << 32])), rw=rw)

    # -- the table --
    def upload(self, n):
        r = self.rng
        u = (r.random(n) < float(r.choice([0.0, 0.3, 0.6]))).astype(np.uint8)
        nd = r.integers(-1, 10, n).astype(np.int8)
        if n > 1100 and r.random() < 0.5:  # one digit only in the last words: decisions reach the table's end
            nd[: n - 40][nd[: n - 40] == 7] = 8
        self.n, self.nres, self.has_cap, self.cols = n, None, False, set()
        self.unit, self.over55, self.over55_at = 1, False, None
        self.emit("upload_nodes", u=u, nd=nd)

    def patch(self, count=None):
        r = self.rng
        count = int(r.choice([1, 64, 65, max(self.n // 3, 1)])) if count is None else count
        count = min(count, self.n)
        idx = r.choice(self.n, size=count, replace=False).astype(np.int32)
        self.emit("patch_nodes", idx=idx, u=r.integers(0, 2, count).astype(np.uint8),
                  nd=r.integers(-1, 10, count).astype(np.int8))

    def column(self, k):
        r = self.rng
        kind = int(r.integers(0, 4))
        sc = (r.integers(0, 101, self.n) if kind == 0 else r.integers(-50, 51, self.n) if kind == 1
              else r.integers(-(1 << 31), (1 << 31) + 1, self.n) if kind == 2 else np.full(self.n, int(r.integers(-5, 6))))
        self.cols.add(k)
        self.emit("upload_score_column", k=k, scores=sc.astype(np.int64))

    # -- capacity column and resource table --
    def cap_upload(self, negative=False):
        r = self.rng
        cap = (r.choice([0, 1, 2, 3, 10**6], self.n) if r.random() < 0.6 else r.integers(0, 4, self.n)).astype(np.int64)
        if r.random() < 0.2:
            cap[int(r.integers(0, self.n))] = CR.INT32_MAX
        if negative:
            cap[int(r.integers(0, self.n))] = -1
        else:
            self.has_cap = True
        self.emit("upload_node_capacity", cap=cap)

    def cap_patch(self):
        r = self.rng
        count = min(int(r.choice([1, 3, 16, 17, 40])), self.n)
        idx = r.choice(self.n, size=count, replace=False).astype(np.int32)
        self.emit("patch_node_capacity", idx=idx, cap=r.integers(0, 6, count).astype(np.int64))

    def cap_clear(self):
        self.has_cap = False
        self.emit("clear_node_capacity")

    def res_upload(self, nres=None, scarce=True):
        r = self.rng
        nres = int(r.integers(1, 5)) if nres is None else nres
        unit = int(r.choice([1, 1 << 33]))
        alloc = (r.integers(0, 9, (nres, self.n)) if scarce else r.integers(20, 200, (nres, self.n))) * unit
        used = r.integers(0, 3, (nres, self.n)) * unit if r.random() < 0.5 else None
        self.nres, self.unit, self.over55 = nres, unit, False
        self.emit("upload_node_resources", alloc=alloc.astype(np.int64), used=None if used is None else used.astype(np.int64))

    def res_patch(self, what=None):
        r = self.rng
        what = what or str(r.choice(["alloc", "used", "both", "below"]))
        nres = self.nres or 2  # without a table the call is refused before the arrays are read
        unit = self.unit
        count = min(int(r.choice([1, 2, 5, 33])), self.n)
        idx = r.choice(self.n, size=count, replace=False).astype(np.int32)
        a = (r.integers(0, 12, (nres, count)) * unit).astype(np.int64)
        us = (r.integers(0, 4, (nres, count)) * unit).astype(np.int64)
        if what == "below":  # allocatable lowered below used
            a, us = np.full((nres, count), unit, np.int64), np.full((nres, count), 3 * unit, np.int64)
        if what == "over55":  # one amount past MSH_RESOURCE_SCORE_MAX ...
            idx, a, us = idx[:1], np.full((nres, 1), (1 << 55) + 1, np.int64), None
            self.over55_at, self.over55 = idx, self.nres is not None
        if what == "back":    # ... and overwritten: the high-water mark stays
            idx, a, us = self.over55_at, np.full((nres, 1), 5 * unit, np.int64), None
        self.emit("patch_node_resources", idx=idx, alloc=None if what == "used" else a,
                  used=us if what in ("used", "both", "below") else None)

    def res_clear(self):
        self.nres = None
        self.emit("clear_node_resources")

    # -- scheduling --
    def batch(self):
        pd, pt = self.pods(self.pod_count())
        self.emit("schedule_batch", pd=pd, pt=pt)

    def multi(self):
        r = self.rng
        p = max(self.pod_count(), 3)
        pd, pt = self.pods(p)
        k = int(r.integers(1, 4))
        cuts = [0] + sorted(int(x) for x in r.choice(np.arange(1, p), size=k - 1, replace=False)) + [p]
        self.emit("schedule_batches_device", pd=pd, pt=pt, cuts=cuts)

    def seq(self, kind=None, scalar=None):
        r = self.rng
        if scalar is None:
            scalar = int(r.choice([1, 3, 3])) if kind == "capacity" else 0 if kind in ("pairs", "short") else int(r.choice([0, 1, 3]))
        pd, pt = self.pods(self.pod_count(kind), digits=int(r.choice([3, 10])))
        self.emit("schedule_sequential", pd=pd, pt=pt, scalar=scalar, cb=bool(r.random() < 0.3))

    def fit(self, nres=None, scalar=None):
        r = self.rng
        nres = (self.nres or 2) if nres is None else nres
        p = self.pod_count()
        if self.n > 1100:
            p = min(p, 130)
        pd, pt = self.pods(p, digits=int(r.choice([3, 10])))
        req = (r.integers(0, 4, (nres, p)) * self.unit).astype(np.int64)
        self.emit("schedule_sequential_fit", pd=pd, pt=pt, req=req, scalar=int(r.choice([0, 0, 3])) if scalar is None else scalar,
                  cb=bool(r.random() < 0.3))

    def read(self, what=None):
        self.emit("read", what=[str(self.rng.choice(READS))] if what is None else list(what))

    # -- segments: a few steps on the current table --
    def calm(self):
        """FIRST mode and a list without score columns: what every sequential call needs."""
        if self.random:
            self.tiebreak(False)
        if self.generic:
            self.plugins("nn")

    def seg_random(self):
        r = self.rng
        if self.generic:
            self.plugins("nn")
        self.tiebreak(True)
        for _ in range(int(r.integers(3, 6))):
            op = str(r.choice(["batch", "batch", "multi", "multi", "patch", "plugins", "toggle"]))
            {"batch": self.batch, "multi": self.multi, "patch": self.patch, "plugins": self.plugins,
             "toggle": lambda: self.plugins("nn", toggle_filter=True)}[op]()
        if r.random() < 0.6:  # refused in RANDOM mode: the counter stays
            self.seq()
        self.multi()
        self.tiebreak(False)

    def seg_columns(self):
        r = self.rng
        if self.random:
            self.tiebreak(False)
        self.plugins("cols")
        names = [s for s, _, _ in self.score if s in M.COLS]
        if r.random() < 0.25:
            self.batch()  # a column of the list not uploaded since the upload: MSH_ERR_STATE
        for s in names:
            self.column(M.COLS.index(s))
        self.batch()
        self.patch()
        self.column(int(r.integers(0, 2)))
        self.plugins("cols", toggle_filter=True)
        self.patch()
        (self.multi if r.random() < 0.5 else self.batch)()
        if r.random() < 0.3:
            self.seq()  # sequential mode with a score-column list: refused
        for s in [s for s, _, _ in self.score if s in M.COLS]:
            if M.COLS.index(s) not in self.cols:
                self.column(M.COLS.index(s))
        self.multi()
        self.plugins("nn")

    def seg_sequential(self):
        r = self.rng
        self.calm()
        fit_ok = self.n <= 8192
        for _ in range(int(r.integers(6, 10))):
            op = str(r.choice(["seq", "seq", "seq", "cap", "cap", "res", "fit", "fit", "patch", "toggle", "reset", "rs",
                               "batch", "plugins"]))
            if op == "seq":
                self.seq()
            elif op == "cap":
                if not self.has_cap:
                    self.cap_upload(negative=r.random() < 0.1)
                else:
                    (self.cap_patch if r.random() < 0.7 else self.cap_clear)()
                self.seq(scalar=int(r.choice([0, 0, 3])))
            elif op == "res":
                if self.nres is None or r.random() < 0.3:
                    self.res_upload(nres=int(r.integers(1, 5)) if self.n <= 2048 else int(r.integers(1, 3)))
                elif r.random() < 0.8:
                    self.res_patch()
                else:
                    self.res_clear()
            elif op == "fit":
                if not fit_ok and r.random() < 0.8:
                    continue  # past the limit: refused, kept rare
                if self.nres is None and r.random() < 0.85:
                    self.res_upload(nres=int(r.integers(1, 5)) if self.n <= 2048 else int(r.integers(1, 3)))
                if self.rs[0] and (self.rs[1] != self.nres or self.n > M.fit_max_nodes(self.nres or 1, True) or self.over55) \
                        and r.random() < 0.85:
                    self.resource_score(0)
                self.fit()
            elif op == "patch":
                self.patch()
            elif op == "toggle":
                self.plugins("nn", toggle_filter=True)
            elif op == "plugins":
                self.plugins("nn")
            elif op == "reset":
                self.emit("reset_node_pod_counts")
            elif op == "rs":
                self.resource_score(int(r.integers(0, 3)), invalid=r.random() < 0.25)
            else:
                self.batch()

    def burst(self, index):
        """Every ordered pair of the four sequential kinds as adjacent successful steps on this table, unscored and
        scored halves, then a _fit call after nres changed with no msh_upload_nodes in between."""
        r = self.rng
        self.calm()
        if self.score == [] or "NodeNumber" not in [s for s, _, _ in self.score] or r.random() < 0.5:
            self.emit("set_plugins", filters=list(self.filters), prescore=["NodeNumber"],
                      score=[("NodeNumber", int(r.choice(WEIGHTS)), int(r.integers(0, 4)))])
            self.score = [("NodeNumber", 1, 0)]
        if self.has_cap:
            self.cap_clear()
        self.res_upload(scarce=bool(r.random() < 0.5))
        scored_first = (index // 2) % 2 == 1  # not tied to the read-back policy (index % 2)
        self.resource_score(int(r.integers(1, 3)) if scored_first else 0)
        perm = r.permutation(4)
        start = int(r.integers(0, 16))
        walk = [SEQ_KINDS[perm[DE_BRUIJN[(start + k) % 16]]] for k in range(17)]
        for k, kind in enumerate(walk):
            self.seq(kind) if kind != "fit" else self.fit(scalar=0)
            if k == 8:  # the switch: a _fit call straight after a pair-form call on either side of it
                self.seq("pairs")
                self.fit(scalar=0)
                self.resource_score(0 if scored_first else int(r.integers(1, 3)))
                self.seq("pairs")
                self.fit(scalar=0)
                self.read(["node_pod_counts"])
                self.emit("reset_node_pod_counts")
        self.read(["node_pod_counts", "node_resources"])
        if index % 3 == 0:  # 2^55 + 1 written and overwritten: scored calls stay refused until the next upload
            self.resource_score()
            self.res_patch("over55")
            self.res_patch("back")
            self.fit(scalar=0)
        nres = self.nres % 4 + 1
        mismatch = index % 4 in (1, 2)
        if mismatch:
            self.resource_score(nres=self.nres)
        if r.random() < 0.5:
            self.res_clear()
        self.res_upload(nres=nres)
        if mismatch:
            self.fit()  # the resource score was set for the previous table's nres: MSH_ERR_STATE
        if self.rs[0]:
            self.resource_score(nres=self.nres, mode=self.rs[0]) if r.random() < 0.7 else self.resource_score(0)
        self.fit()
        if r.random() < 0.3:
            self.fit(nres=self.nres % 4 + 1)  # requests for another nres than the table's: MSH_ERR_INVALID


    def limits(self, index):
        """The _fit limits, each form in turn over the traces: a successful call on a table of exactly
        msh_seq_fit_max_nodes(nres, scored) nodes, the refusals of RANDOM mode with a table present (a batch with a
        score-column list, then _fit), and the refusal one node past the limit."""
        r = self.rng
        nres, scored = LIMIT_FORMS[index % len(LIMIT_FORMS)]
        lim = M.fit_max_nodes(nres, scored)
        for n in (lim, lim + 1):
            self.upload(n)
            self.calm()
            if self.score == [] or r.random() < 0.3:
                self.plugins("nn")
            self.res_upload(nres=nres)
            if n == lim:
                self.resource_score(int(r.integers(1, 3)) if scored else 0, nres=nres)
                self.seq("pairs")
            self.fit(scalar=0)  # lim: placed; lim + 1: MSH_ERR_UNSUPPORTED
            if n == lim:
                self.fit(scalar=3)
                self.tiebreak(True)
                self.plugins("cols")
                self.batch()  # RANDOM with a score-column list
                self.plugins("nn")
                self.fit()    # _fit in RANDOM mode, a table present
                self.tiebreak(False)
        if index % 2 == 0:  # a setter's failed call changes nothing
            self.resource_score(int(r.integers(1, 3)), nres=nres, invalid=True)
            self.read(["resource_score"])
        self.read(["node_pod_counts", "node_resources"])


# (nres, scored) of the limit segment, by trace index: 8,192 / 4,096 unscored, 4,096 / 2,048 scored
LIMIT_FORMS = [(2, False), (3, False), (1, True), (4, True), (1, False), (4, False), (2, True), (3, True)]


def ladder_walk(rng, index):
    small = [n for n in LADDER if n <= 1025]
    mid = [n for n in LADDER if 1025 < n <= 8193]
    line = [32767, 32768]
    if index % 2 == 0 or index % 4 == 1:  # across the 32,768 line, up and down
        return [int(rng.choice(small)), int(rng.choice(line)), 32769, int(rng.choice(line + mid)), int(rng.choice(small)),
                int(rng.choice(mid))]
    pos = int(rng.integers(0, len(LADDER) - 3))
    walk = []
    for _ in range(6):
        walk.append(LADDER[pos])
        pos = int(np.clip(pos + rng.choice([-4, -2, -1, 1, 2, 3]), 0, len(LADDER) - 4))
    return walk


def make_trace(seed, index):
    rng = np.random.default_rng(seed)
    g = Gen(rng)
    lazy = index % 2 == 1
    g.n = 64
    if index % 3 == 0:  # before the first msh_upload_nodes, a score-column list set: "no nodes" comes first
        g.plugins("cols")
        (g.seq if index % 2 else g.fit)()
        g.plugins("nn")
    elif rng.random() < 0.6:  # before the first msh_upload_nodes
        [g.batch, g.seq, lambda: g.emit("reset_node_pod_counts"), g.cap_upload, g.res_patch, g.multi][int(rng.integers(0, 6))]()
        g.has_cap = False
    walk = ladder_walk(rng, index)
    burst_n = [1023, 1024, 1025][index % 3]
    walk.insert(int(rng.integers(1, len(walk))), burst_n)
    limits_at = int(rng.integers(1, len(walk)))
    for t, n in enumerate(walk):
        if t == limits_at:
            g.limits(index)
        g.upload(n)
        if n == burst_n and not g.burst_done:
            g.burst(index)
            g.burst_done = True
        elif n >= 32767:
            g.calm()
            g.seq("pairs")
            g.seq(str(rng.choice(["short", "capacity"])))
            if rng.random() < 0.5:
                g.cap_upload()
                g.seq()
                g.patch()
                g.cap_patch()
                g.seq("pairs", scalar=0)
                g.cap_clear()
                g.seq(scalar=0)
            g.read(["node_pod_counts"])
            if rng.random() < 0.3:
                g.seg_random()
        else:
            [g.seg_sequential, g.seg_sequential, g.seg_random, g.seg_columns][int(rng.integers(0, 4))]()
        if lazy and rng.random() < 0.4:
            g.read()
    return {"seed": seed, "index": index, "lazy": lazy, "steps": g.steps}


def traces(seed0, count):
    for i in range(count):
        yield make_trace(seed0 + i, i)


def describe(step):
    """One step, compactly: the op and the sizes / scalars that decide its path."""
    op, a = step
    bits = []
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            bits.append(f"{k}{list(v.shape)}")
        elif v is not None:
            bits.append(f"{k}={v}")
    return f"{op}({', '.join(bits)})"


def run_model(O, trace, mutant=None):
    """The model over one trace: per step {"result", "reads"} (reads: None, or {name: value} where the policy reads
    back), plus the final read-backs as a last record."""
    m = M.CtxModel(O, mutant)
    out = []
    for op, args in trace["steps"]:
        if op == "read":
            out.append({"result": None, "reads": {w: getattr(m, w)() for w in args["what"]}})
            continue
        res = m.apply(op, args)
        out.append({"result": res, "reads": None if trace["lazy"] else {w: getattr(m, w)() for w in READS}})
    out.append({"result": None, "reads": {w: getattr(m, w)() for w in READS}})
    return out


@functools.lru_cache(maxsize=None)
def _trace_set():
    return tuple(traces(TRACE_SEED0, TRACE_COUNT))


_EXPECTED = {}


def expected(O, index):
    """The true model's records for trace `index` of the fixed set, computed once per session."""
    if index not in _EXPECTED:
        _EXPECTED[index] = run_model(O, _trace_set()[index])
    return _EXPECTED[index]


# ---------------------------------------------------------------------------------------------------------------
def test_traces_are_deterministic():
    a, b = list(traces(TRACE_SEED0, 3)), list(traces(TRACE_SEED0, 3))
    for x, y in zip(a, b):
        assert [op for op, _ in x["steps"]] == [op for op, _ in y["steps"]]
        assert all(M.same_value(list(p.values()), list(q.values())) for (_, p), (_, q) in zip(x["steps"], y["steps"]))
    assert sum(t["lazy"] for t in _trace_set()) * 2 == TRACE_COUNT


def _seq_kind(m_before, op, args):
    if op == "schedule_sequential_fit":
        return "fit"
    if op != "schedule_sequential":
        return None
    if args["scalar"] > 0 or m_before.cap is not None:
        return "capacity"
    return "pairs" if len(args["pd"]) > 64 else "short"


def refusal_cause(m, op, args):
    """Why the model in state `m` (before the step) refuses (op, args): the documented refusal a trace walked into,
    named from the state and not from the returned code, or None when the step is not refused for one of them."""
    sched = op in ("schedule_batch", "schedule_batches_device", "schedule_sequential", "schedule_sequential_fit")
    seq, fit = op == "schedule_sequential", op == "schedule_sequential_fit"
    if not sched:
        return None
    if m.tb[0] == M.RANDOM:
        if seq or fit:
            return ("_fit in RANDOM mode, a table present" if m.alloc is not None else "_fit in RANDOM mode") if fit \
                else "sequential in RANDOM mode"
        if m.generic:
            return "RANDOM with a score-column list"
    if not m.have_nodes:
        return ("before the first upload, a score-column list set" if m.generic and (seq or fit)
                else "before the first upload")
    if (seq or fit) and m.generic:
        return "sequential with a score-column list"
    if not (seq or fit):
        missing = any(s in M.COLS and M.COLS.index(s) not in m.cols for s, _, _ in m.score)
        return "a missing score column" if m.tb[0] == M.FIRST and missing else None
    if not fit:
        return None
    nres, scored = len(args["req"]), m.rs[0] != 0
    if m.alloc is None:
        return "_fit without a table"
    if nres != len(m.alloc):
        return "_fit with another nres than the table's"
    if scored and len(m.rs[2]) != nres:
        return "a resource score set for another nres"
    if m.n > M.fit_max_nodes(nres, scored):
        return "_fit past the scored limit" if scored else "_fit past the unscored limit"
    if scored and m.res_max > M.SCORE_MAX:
        return "a scored call with res_max above 2^55"
    return None


REFUSALS = ("sequential in RANDOM mode", "_fit in RANDOM mode, a table present", "RANDOM with a score-column list",
            "sequential with a score-column list", "_fit without a table", "_fit with another nres than the table's",
            "a resource score set for another nres", "_fit past the unscored limit", "_fit past the scored limit",
            "a scored call with res_max above 2^55", "a missing score column", "before the first upload",
            "before the first upload, a score-column list set")
FOLDS = ("msh_seq", "seq_fit", "seq_score")  # the kernel family that has to fold the replicas in-kernel


def test_coverage_of_the_fixed_set(oracle):
    alphabet = {"set_plugins", "set_tiebreak", "upload_nodes", "patch_nodes", "upload_score_column", "upload_node_capacity",
                "patch_node_capacity", "clear_node_capacity", "upload_node_resources", "patch_node_resources",
                "clear_node_resources", "set_resource_score", "reset_node_pod_counts", "schedule_batch",
                "schedule_batches_device", "schedule_sequential", "schedule_sequential_fit", "read"}
    seen, refusals = set(), 0
    causes = {}                         # refusal cause -> traces
    steps = placing = seq_ok = 0
    pairs = {}
    folds = {f: set() for f in FOLDS}   # lazy traces in which that family follows a dirty pair-form call
    at_limit = {}                       # (nres, scored) -> traces with a successful _fit on a table of exactly the limit
    fit_nres = {}                       # nres -> successful _fit calls
    ops_ok = {}
    up = down = nres_change = binding = 0
    scored = {False: 0, True: 0}
    for t in _trace_set():
        m = M.CtxModel(oracle)
        prev_kind, prev_n, crossed_up, crossed_down, binds = None, None, False, False, False
        res_fresh, fit_after_change = None, False  # nres at the last msh_upload_nodes / a changed nres since
        dirty = False  # a pair-form call's commits are in the replicas (a lazy trace on a table of <= 32,768 nodes)
        for (op, args), rec in zip(t["steps"], expected(oracle, t["index"])):
            seen.add(op)
            if op == "read":  # no step between two calls, but a read of the counts folds them
                if "node_pod_counts" in args["what"]:
                    prev_kind, dirty = None, False
                continue
            before = m.clone()
            res = m.apply(op, args)
            assert M.same_value(res, rec["result"])
            steps += 1
            ok = res[0] == "ok"
            ops_ok[op] = ops_ok.get(op, 0) + ok
            cause = refusal_cause(before, op, args)
            assert (cause is None) == ok or not op.startswith("schedule"), (t["index"], op, cause, res[0])
            if not ok:
                refusals += 1
                if cause:
                    causes.setdefault(cause, set()).add(t["index"])
            if op == "upload_nodes":
                n = len(args["u"])
                if prev_n is not None:
                    crossed_up |= prev_n <= 32768 < n
                    crossed_down |= n <= 32768 < prev_n
                prev_n, prev_kind, res_fresh, dirty = n, None, "none", False
            if op == "reset_node_pod_counts":
                dirty = False
            if op == "upload_node_resources" and ok:
                res_fresh = len(args["alloc"]) if res_fresh == "none" else ("changed" if res_fresh != len(args["alloc"]) else res_fresh)
            kind = _seq_kind(before, op, args) if op.startswith("schedule_sequential") else None
            if kind and ok:
                seq_ok += 1
                idx, score, status, cb = res[1]
                placing += bool((status == 0).any())
                free = oracle.c_schedule_batch(m.u, m.nd, args["pd"], args["pt"], m._ps())
                binds |= kind in ("capacity", "fit") and bool(((status == 1) & (free[2] == 0)).any() or
                                                                (before.rs[0] == 0 and (idx != free[0]).any()))
                is_scored = before.rs[0] != 0
                if kind == "fit":
                    scored[is_scored] += 1
                    fit_after_change |= res_fresh == "changed"
                    nres = len(args["req"])
                    fit_nres[nres] = fit_nres.get(nres, 0) + 1
                    if m.n == M.fit_max_nodes(nres, is_scored):
                        at_limit.setdefault((nres, is_scored), set()).add(t["index"])
                if kind == "pairs":
                    dirty = t["lazy"] and m.n <= 32768
                elif dirty:
                    folds["msh_seq" if kind != "fit" else "seq_score" if is_scored else "seq_fit"].add(t["index"])
                    dirty = False
                if prev_kind:
                    pairs.setdefault((prev_kind, kind), set()).add(t["index"])
                if cb is not None:
                    assert cb == [(j, int(idx[j]), int(score[j])) for j in range(len(idx)) if status[j] == 0]
            prev_kind = kind if kind and ok else None
        up, down, nres_change, binding = up + crossed_up, down + crossed_down, nres_change + fit_after_change, binding + binds
    assert seen == alphabet, alphabet ^ seen
    for x in SEQ_KINDS:
        for y in SEQ_KINDS:
            assert len(pairs.get((x, y), ())) >= 3, f"({x}, {y}) adjacent in traces {sorted(pairs.get((x, y), ()))}"
    assert refusals <= 0.15 * steps, (refusals, steps)
    assert placing >= 0.8 * seq_ok, (placing, seq_ok)
    assert binding == TRACE_COUNT, f"capacity or requests bind in {binding} of {TRACE_COUNT} traces"
    assert 3 * up >= TRACE_COUNT and 3 * down >= TRACE_COUNT, (up, down)
    assert 3 * nres_change >= TRACE_COUNT, nres_change
    assert min(scored.values()) >= TRACE_COUNT, scored
    # every documented refusal, by its cause in the model's state before the step, in at least one trace; the ones
    # the generator walks into on purpose in at least three
    for cause in REFUSALS:
        assert causes.get(cause), f"never refused for: {cause}; seen {sorted(causes)}"
    for cause in ("_fit in RANDOM mode, a table present", "RANDOM with a score-column list", "_fit past the unscored limit",
                  "_fit past the scored limit", "sequential in RANDOM mode", "before the first upload, a score-column list set"):
        assert len(causes[cause]) >= 3, (cause, sorted(causes[cause]))
    # a successful _fit on a table of exactly the limit: 8,192 (nres <= 2) and 4,096 (nres 3-4) unscored, 4,096 and
    # 2,048 scored
    for form in ((1, False), (2, False), (3, False), (4, False), (1, True), (2, True), (3, True), (4, True)):
        assert at_limit.get(form), f"no successful _fit at the limit of nres={form[0]} scored={form[1]}: {sorted(at_limit)}"
    # the in-kernel fold of every kernel family: a dirty pair-form call, no read of the counts, then that family
    for f in FOLDS:
        assert len(folds[f]) >= 3, f"{f} folds after a dirty call in lazy traces {sorted(folds[f])}"
    assert all(fit_nres.get(k, 0) >= 6 for k in (1, 2, 3, 4)), fit_nres
    assert ops_ok["patch_node_capacity"] >= 6 and ops_ok["patch_node_resources"] >= 6 and ops_ok["clear_node_resources"] >= 3, ops_ok
    print(f"ctx traces: {TRACE_COUNT} traces, {steps} steps, {refusals} refused, {seq_ok} sequential / _fit calls "
          f"({placing} placing), up {up} down {down}, scored {scored}, folds { {f: len(v) for f, v in folds.items()} }, "
          f"_fit by nres {fit_nres}, causes { {c: len(v) for c, v in causes.items()} }")


def _differs(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if not M.same_value(x["result"], y["result"]) or not M.same_value(
                None if x["reads"] is None else list(x["reads"].values()),
                None if y["reads"] is None else list(y["reads"].values())):
            return k
    return None


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_told_apart(oracle, mutant):
    caught = []
    for t in _trace_set():
        if _differs(expected(oracle, t["index"]), run_model(oracle, t, mutant)) is not None:
            caught.append(t["index"])
    assert len(caught) >= 3, f"{mutant}: told apart only in traces {caught}"


def test_lazy_traces_are_what_catches_dropped_replicas(oracle):
    """The read-back after every step folds the counts on the host path: only the lazy half leaves them in the
    replicas across calls."""
    for t in _trace_set():
        hit = _differs(expected(oracle, t["index"]), run_model(oracle, t, "replicas_dropped_not_folded"))
        assert t["lazy"] or hit is None


# ---- the model on the sequences the per-feature GPU tests script ------------------------------------------------
class ModelError(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


class ModelCtx:
    """The model behind DeviceContext's method names, for scripts written against a DeviceContext."""

    def __init__(self, O):
        self.m = M.CtxModel(O)

    def _do(self, op, **args):
        kind, val = self.m.apply(op, args)
        if kind == "err":
            raise ModelError(val)
        return val

    def set_ps(self, ps):
        self._do("set_plugins", filters=ps.filters, prescore=ps.prescore, score=list(zip(ps.score, ps.weights, ps.normalize)))

    def set_tiebreak(self, mode, seed=0, counter=0):
        self._do("set_tiebreak", mode={"first": 0, "random": 1}[mode], seed=seed, counter=counter)

    def set_resource_score(self, mode, weight=1, rw=None):
        mode = {"none": 0, "least": 1, "most": 2}[mode]
        self._do("set_resource_score", mode=mode, weight=weight, rw=[1] * len(self.m.alloc) if rw is None and mode else rw or [])

    def upload_nodes(self, u, nd):
        self._do("upload_nodes", u=u, nd=nd)

    def patch_nodes(self, idx, u, nd):
        self._do("patch_nodes", idx=idx, u=u, nd=nd)

    def upload_node_capacity(self, cap):
        self._do("upload_node_capacity", cap=cap)

    def patch_node_capacity(self, idx, cap):
        self._do("patch_node_capacity", idx=np.asarray(idx), cap=cap)

    def clear_node_capacity(self):
        self._do("clear_node_capacity")

    def upload_node_resources(self, alloc, used=None):
        self._do("upload_node_resources", alloc=alloc, used=used)

    def patch_node_resources(self, idx, alloc=None, used=None):
        self._do("patch_node_resources", idx=np.asarray(idx), alloc=alloc, used=used)

    def clear_node_resources(self):
        self._do("clear_node_resources")

    def reset_node_pod_counts(self):
        self._do("reset_node_pod_counts")

    def schedule_sequential(self, pd, pt, scalar=0):
        return self._do("schedule_sequential", pd=pd, pt=pt, scalar=scalar)[:3]

    def schedule_sequential_fit(self, pd, pt, req, scalar=0):
        return self._do("schedule_sequential_fit", pd=pd, pt=pt, req=np.asarray(req), scalar=scalar)[:3]

    def node_pod_counts(self):
        return self.m.node_pod_counts()[1]

    def node_capacity(self):
        return self.m.node_capacity()[1]

    def node_resources(self):
        return self.m.node_resources()[1]

    def resource_score(self):
        return self.m.resource_score()[1]


def same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "score", "status")):
        assert np.array_equal(g, w), f"{what}: {name}"


def test_model_on_the_capacity_script(oracle):
    """test_node_capacity_gpu.test_carry_over_patches_and_lifetime, the model in the context's place."""
    rng = np.random.default_rng(1 + 70)
    ps = oracle.PluginSet()
    ctx = ModelCtx(oracle)
    ctx.set_ps(ps)
    n, P = 90, 300
    u = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, 10, P).astype(np.int8)
    pt = (rng.random(P) < 0.4).astype(np.uint8)
    cap = rng.integers(1, 6, n)

    def call(a, b, cap, scalar, before, what):
        got = ctx.schedule_sequential(pd[a:b], pt[a:b], scalar)
        wi, ws, wst, after = CR.via_oracle(oracle, u, nd, pd[a:b], pt[a:b], ps, CR.effective(cap, scalar), before)
        same(got, (wi, ws, wst), what)
        assert np.array_equal(ctx.node_pod_counts(), after), what
        return after

    ctx.upload_nodes(u, nd)
    assert ctx.node_capacity() is None
    ctx.upload_node_capacity(cap)
    k = call(0, 100, cap, 0, None, "first call")
    k = call(100, 150, cap, 0, k, "carried counts")
    held = np.flatnonzero(k > 0)[:2]
    room = np.setdiff1d(np.flatnonzero(k == cap), held)[:1]
    cap = cap.copy()
    cap[held[0]], cap[held[1]], cap[room[0]] = k[held[0]], max(k[held[1]] - 1, 0), cap[room[0]] + 2
    ctx.patch_node_capacity(np.concatenate([held, room]), cap[np.concatenate([held, room])])
    assert np.array_equal(ctx.node_capacity(), cap)
    k2 = call(150, 200, cap, 0, k, "after the patch")
    assert (k2[held] == k[held]).all()
    cap[held] += 3
    ctx.patch_node_capacity(held, cap[held])
    k = call(200, 250, cap, 0, k2, "after raising")
    u = u.copy()
    flip = np.arange(0, n, 7, dtype=np.int32)
    u[flip] ^= 1
    ctx.patch_nodes(flip, u[flip], nd[flip])
    assert np.array_equal(ctx.node_capacity(), cap)
    k = call(250, 300, cap, 0, k, "after msh_patch_nodes")
    ctx.reset_node_pod_counts()
    assert np.array_equal(ctx.node_capacity(), cap)
    call(0, 80, cap, 0, None, "after the reset")
    ctx.upload_nodes(u, nd)
    assert ctx.node_capacity() is None
    want = oracle.c_schedule_sequential(u, nd, pd, pt, ps, 0)
    same(ctx.schedule_sequential(pd, pt, 0), want[:3], "after msh_upload_nodes")
    assert np.array_equal(ctx.node_pod_counts(), want[3])
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    ctx.clear_node_capacity()
    assert ctx.node_capacity() is None
    want = oracle.c_schedule_sequential(u, nd, pd, pt, ps, 2)
    same(ctx.schedule_sequential(pd, pt, 2), want[:3], "after msh_clear_node_capacity")
    assert np.array_equal(ctx.node_pod_counts(), want[3])
    with pytest.raises(ModelError) as ei:
        ctx.patch_node_capacity([0], [1])
    assert ei.value.code == M.STATE


def _fit_call(ctx, O, u, nd, pd, pt, ps, alloc, used, req, counts, what, mode=S.NONE, weight=1, rw=None):
    n = len(u)
    rw = [1] * len(alloc) if rw is None else rw
    ctx.set_resource_score({0: "none", 1: "least", 2: "most"}[mode], weight, rw)
    got = ctx.schedule_sequential_fit(pd, pt, req)
    ref = S.serial if n * len(pd) <= 2 * 10**4 else S.per_pod
    wi, ws, wst, cnt, us = ref(O, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, mode, weight, rw, counts)
    same(got, (wi, ws, wst), what)
    assert np.array_equal(ctx.node_pod_counts(), cnt), what
    a, b = ctx.node_resources()
    assert np.array_equal(a, alloc) and np.array_equal(b, us), what
    return cnt, us


def test_model_on_the_resource_fit_script(oracle):
    """test_resource_fit_gpu.test_state_patches_and_lifetime, the model in the context's place."""
    rng = np.random.default_rng(77)
    ps = oracle.PluginSet()
    n, p = 90, 400
    u = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, 10, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    alloc = (rng.integers(0, 9, (2, n)) * 3).astype(np.int64)
    req = rng.integers(0, 4, (2, p)).astype(np.int64)
    ctx = ModelCtx(oracle)
    ctx.upload_nodes(u, nd)
    assert ctx.node_resources() is None
    ctx.set_ps(ps)
    ctx.upload_nodes(u, nd)
    ctx.upload_node_resources(alloc)
    used = np.zeros_like(alloc)
    sl = lambda a, b: (pd[a:b], pt[a:b], req[:, a:b])  # noqa: E731
    cnt, used = _fit_call(ctx, oracle, u, nd, *sl(0, 80)[:2], ps, alloc, used, sl(0, 80)[2], None, "first call")
    cnt, used = _fit_call(ctx, oracle, u, nd, *sl(80, 120)[:2], ps, alloc, used, sl(80, 120)[2], cnt, "carried state")
    a, b, _ = sl(120, 220)
    want = R.per_pod(oracle, u, nd, a, b, ps, R.no_limit(n), alloc, used, np.zeros((2, 100), np.int64), cnt)
    same(ctx.schedule_sequential(a, b, 0), want[:3], "plain call with a table present")
    cnt = want[3]
    assert np.array_equal(ctx.node_resources()[1], used)
    cnt, used = _fit_call(ctx, oracle, u, nd, *sl(220, 260)[:2], ps, alloc, used, sl(220, 260)[2], cnt, "after the plain call")
    busy = np.flatnonzero(used[0] > 0)
    up, down, setu = busy[:2].astype(np.int32), busy[2:4].astype(np.int32), busy[4:6].astype(np.int32)
    alloc[:, up] += 5
    ctx.patch_node_resources(up, alloc=alloc[:, up])
    alloc[:, down] = np.maximum(used[:, down] - 1, 0)
    ctx.patch_node_resources(down, alloc=alloc[:, down])
    used[:, setu[0]] = 0
    used[:, setu[1]] += 2
    ctx.patch_node_resources(setu, used=used[:, setu])
    got_a, got_u = ctx.node_resources()
    assert np.array_equal(got_a, alloc) and np.array_equal(got_u, used)
    cnt, used = _fit_call(ctx, oracle, u, nd, *sl(260, 320)[:2], ps, alloc, used, sl(260, 320)[2], cnt, "after the patches")
    both = np.array([0, n - 1], np.int32)
    alloc[:, both], used[:, both] = 7, 1
    ctx.patch_node_resources(both, alloc[:, both], used[:, both])
    u = u.copy()
    flip = np.arange(0, n, 7, dtype=np.int32)
    u[flip] ^= 1
    ctx.patch_nodes(flip, u[flip], nd[flip])
    cnt, used = _fit_call(ctx, oracle, u, nd, *sl(320, 360)[:2], ps, alloc, used, sl(320, 360)[2], cnt, "after msh_patch_nodes")
    ctx.reset_node_pod_counts()
    _fit_call(ctx, oracle, u, nd, *sl(360, 400)[:2], ps, alloc, used, sl(360, 400)[2], None, "after the count reset")
    ctx.clear_node_resources()
    assert ctx.node_resources() is None
    for drop in ("clear", "upload"):
        if drop == "upload":
            ctx.upload_node_resources(alloc)
            ctx.upload_nodes(u, nd)
            assert ctx.node_resources() is None
        with pytest.raises(ModelError) as ei:
            ctx.schedule_sequential_fit(pd, pt, req)
        assert ei.value.code == M.STATE
        with pytest.raises(ModelError) as ei:
            ctx.patch_node_resources([0], alloc=[[1], [1]])
        assert ei.value.code == M.STATE


def test_model_on_the_resource_score_script(oracle):
    """test_resource_score_gpu.test_carried_state_patches_and_setter, the model in the context's place."""
    rng = np.random.default_rng(77)
    ps = oracle.PluginSet()
    n, p = 90, 400
    u = (rng.random(n) < 0.2).astype(np.uint8)
    nd = rng.integers(-1, 3, n).astype(np.int8)
    pd = rng.integers(0, 3, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    alloc = rng.integers(20, 200, (2, n)).astype(np.int64)
    used = rng.integers(0, 10, (2, n)).astype(np.int64)
    req = rng.integers(0, 4, (2, p)).astype(np.int64)
    ctx = ModelCtx(oracle)
    ctx.set_ps(ps)
    ctx.set_tiebreak("first")
    ctx.upload_nodes(u, nd)
    ctx.upload_node_resources(alloc, used)
    sl = lambda a, b: (pd[a:b], pt[a:b], req[:, a:b])  # noqa: E731
    script = [((0, 80), S.LEAST, 2, [2, 1]), ((80, 120), S.LEAST, 2, [2, 1]), ((120, 160), S.MOST, 2, [2, 1]),
              ((160, 200), S.NONE, 1, None)]
    cnt = None
    for (a, b), mode, w, rw in script:
        x, y, c = sl(a, b)
        cnt, used = _fit_call(ctx, oracle, u, nd, x, y, ps, alloc, used, c, cnt, f"pods {a}:{b}", mode, w, rw)
    ctx.set_resource_score("least", 5, [1, 1])
    a, b, _ = sl(200, 300)
    want = R.per_pod(oracle, u, nd, a, b, ps, R.no_limit(n), alloc, used, np.zeros((2, 100), np.int64), cnt)
    same(ctx.schedule_sequential(a, b, 0), want[:3], "plain call with a resource score set")
    cnt = want[3]
    assert np.array_equal(ctx.node_resources()[1], used)
    x, y, c = sl(300, 330)
    cnt, used = _fit_call(ctx, oracle, u, nd, x, y, ps, alloc, used, c, cnt, "after the plain call", S.LEAST, 5)
    busy = np.flatnonzero(used[0] > 0)
    down, up, zero = busy[:2].astype(np.int32), busy[2:4].astype(np.int32), busy[4:5].astype(np.int32)
    alloc[:, down] = np.maximum(used[:, down] - 1, 0)
    ctx.patch_node_resources(down, alloc=alloc[:, down])
    alloc[:, up] += 500
    ctx.patch_node_resources(up, alloc=alloc[:, up])
    used[:, zero] = 0
    ctx.patch_node_resources(zero, used=used[:, zero])
    x, y, c = sl(330, 365)
    c = c.copy()
    c[:, ::3] = 0
    cnt, used = _fit_call(ctx, oracle, u, nd, x, y, ps, alloc, used, c, cnt, "after the resource patches", S.MOST, 5)
    u = u.copy()
    flip = np.arange(0, n, 7, dtype=np.int32)
    u[flip] ^= 1
    ctx.patch_nodes(flip, u[flip], nd[flip])
    x, y, c = sl(365, 400)
    _fit_call(ctx, oracle, u, nd, x, y, ps, alloc, used, c, cnt, "after msh_patch_nodes", S.LEAST, 5)
    ctx.set_resource_score("most", 9, [4, 0])
    ctx.clear_node_resources()
    ctx.upload_nodes(u, nd)
    assert ctx.resource_score() == (S.MOST, 9, [4, 0])
    ctx.upload_node_resources(alloc)
    ctx.set_resource_score("least")
    assert ctx.resource_score() == (S.LEAST, 1, [1, 1])
