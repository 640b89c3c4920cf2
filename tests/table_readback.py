"""Read the whole node table back through two calls the ABI already has, after every kind of table rewrite.

The table is two byte columns (`unsched`, `digit`) and six bit planes, kept in two versions; an upload, a patch (at
most 64 nodes inline in the copy kernel, more by a scatter and a full prep), a filter-list change and a score-column
upload each build one version from the other. A batch call reports a pod's first feasible match and non-match, so it
sees a few dozen nodes near the head of the list; the two readers here see every node:

  read_planes   `schedule_sequential` with `max_pods_per_node = 1` on zeroed counts and n + 8 identical pods. Tolerating
                pods of digit d fill the nodes of that digit in List order at score 10, then the rest at score 0, and
                the last 8 get a fit error: ten sweeps give every node's digit (none: -1). One sweep of pods that do
                not tolerate fills exactly the nodes whose X bit is clear. An index >= n or a placed count other than n
                is the V plane. The sequential kernels read the planes only.
  read_columns  `export_results` with the same 11 pod kinds: the filter row of the pod that does not tolerate is the
                `unsched` column where the filter is listed, and raw == 10 in the row of digit d marks the nodes of
                that digit. The export kernel reads the columns only.

`TableModel` is the table a context must hold after a list of operations, `run_case` applies such a list to a context
and to the model and reads everything back after every operation, `hand_families` are the written cases and `trace`
draws seeded ones. tests/test_table_readback.py runs all of it over the CPU oracle (`OracleCtx`) and shows that the
readers miss no single-node change and that the cases catch nine wrong models; tests/test_table_readback_gpu.py runs
the same cases on a `DeviceContext`.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

PLACED, FIT_ERROR = 0, 1
EXPORT_NONE = -(1 << 63)
NU, NN = "NodeUnschedulable", "NodeNumber"
SIZES = (1, 33, 1000, 1024, 1025, 2500)
EXTRA_PODS = 8   # pods past n in every sweep: each must get a fit error
INLINE = 64      # a patch of at most this many nodes rides on the copy kernel; more take the scatter path
TRACE_COUNT, TRACE_OPS, TRACE_SEED0 = 12, 25, 7100


class ScoreCfg(NamedTuple):
    """What `set_plugins` reads of a score plugin (ScorePluginConfig's fields)."""
    name: str
    weight: int = 1
    normalize: int = 0


NN_SCORE = [ScoreCfg(NN, 1, 0)]  # the list both readers run on: NodeNumber, weight 1, no normaliser
POD_DIGIT = np.array(list(range(10)) + [0], np.int8)  # the 11 pod kinds of the export: ten that tolerate,
POD_TOL = np.array([1] * 10 + [0], np.uint8)          # and one, of a valid digit, that does not


class ReadbackError(AssertionError):
    """A reader met something no table explains; the message names the nodes."""


def _first(a, k=8):
    return np.asarray(a)[:k].tolist()


# ---------------------------------------------------------------------------------------
# the two readers
# ---------------------------------------------------------------------------------------
def _sweep(ctx, n, digit, tol, what):
    """One sweep of n + 8 identical pods on zeroed counts -> (nodes in placement order, their scores)."""
    ctx.reset_node_pod_counts()
    p = n + EXTRA_PODS
    idx, score, status = (np.array(x) for x in ctx.schedule_sequential(np.full(p, digit, np.int8), np.full(p, tol, np.uint8), 1))
    bad = np.flatnonzero((status != PLACED) & (status != FIT_ERROR))
    if bad.size:
        raise ReadbackError(f"{what}: pods {_first(bad)} have status {_first(status[bad])}, neither placed nor fit error")
    placed = status == PLACED
    if placed[n:].any():
        late = n + np.flatnonzero(placed[n:])
        raise ReadbackError(f"{what}: pods {_first(late)} past n = {n} were placed, on nodes {_first(idx[late])}")
    k = int(placed.sum())
    if not placed[:k].all():
        raise ReadbackError(f"{what}: pod {int(np.flatnonzero(~placed)[0])} got a fit error and a later identical pod was placed")
    if (idx[k:] != -1).any():
        raise ReadbackError(f"{what}: unplaced pods {_first(k + np.flatnonzero(idx[k:] != -1))} name nodes {_first(idx[k:][idx[k:] != -1])}")
    pi, sc = idx[:k].astype(np.int64), score[:k]
    out = (pi < 0) | (pi >= n)
    if out.any():
        raise ReadbackError(f"{what}: node indices {_first(pi[out])} outside [0, {n})")
    twice = np.flatnonzero(np.bincount(pi, minlength=n) > 1)
    if twice.size:
        raise ReadbackError(f"{what}: nodes {_first(twice)} were placed on twice under a capacity of 1")
    odd = (sc != 0) & (sc != 10)
    if odd.any():
        raise ReadbackError(f"{what}: nodes {_first(pi[odd])} have scores {_first(sc[odd])}, neither 0 nor 10")
    if tol and k != n:
        left = np.setdiff1d(np.arange(n), pi)
        raise ReadbackError(f"{what}: {k} pods placed, not n = {n}; nodes {_first(left)} never took a pod")
    m = sc == 10
    if (m[1:] & ~m[:-1]).any() or (np.diff(pi[m]) <= 0).any() or (np.diff(pi[~m]) <= 0).any():
        raise ReadbackError(f"{what}: the placements are not the score-10 nodes in List order, then the score-0 ones")
    return pi, sc


def read_planes(ctx, n, filters):
    """(unsched_seen, digit) of all n nodes as the plane-reading sequential kernels see them: eleven capacity-1
    sweeps. Sets the list (filters, NodeNumber, NodeNumber w = 1) and leaves it set; the counts end zeroed."""
    ctx.set_plugins(list(filters), [NN], NN_SCORE)
    digit = np.full(n, -1, np.int8)
    for d in range(10):
        pi, sc = _sweep(ctx, n, d, 1, f"planes, tolerating sweep of digit {d}")
        hit = pi[sc == 10]
        again = hit[digit[hit] != -1]
        if again.size:
            raise ReadbackError(f"planes: nodes {_first(again)} match digit {d} and digits {_first(digit[again])}")
        digit[hit] = d
    pi, sc = _sweep(ctx, n, 0, 0, "planes, sweep of pods that do not tolerate")
    split = (digit[pi] == 0) != (sc == 10)
    if split.any():
        raise ReadbackError(f"planes: nodes {_first(pi[split])} score {_first(sc[split])} for a digit-0 pod that does not "
                            f"tolerate, and decode to digits {_first(digit[pi[split]])} from the pods that do")
    unsched = np.ones(n, np.uint8)
    unsched[pi] = 0
    ctx.reset_node_pod_counts()
    return unsched, digit


def read_columns(ctx, n, filters):
    """(unsched_seen, digit) of all n nodes as the column-reading export kernel sees them: one export of the 11 pod
    kinds. Sets the same list as read_planes and leaves it set."""
    ctx.set_plugins(list(filters), [NN], NN_SCORE)
    filt, raw, fin = (np.asarray(x) for x in ctx.export_results(POD_DIGIT, POD_TOL))
    if filt.shape != (11, n) or raw.shape != (11, n):
        raise ReadbackError(f"columns: the export has {filt.shape[1:]} nodes per pod, not n = {n}")
    shut = np.flatnonzero((filt[:10] != 1).any(axis=0))
    if shut.size:
        raise ReadbackError(f"columns: nodes {_first(shut)} reject a pod that tolerates: filter {_first(filt[:10, shut].min(axis=0))}")
    odd = np.flatnonzero(((raw[:10] != 0) & (raw[:10] != 10)).any(axis=0))
    if odd.size:
        raise ReadbackError(f"columns: nodes {_first(odd)} have raw scores {_first(raw[:10, odd].T)}, neither 0 nor 10")
    hits = raw[:10] == 10
    again = np.flatnonzero(hits.sum(axis=0) > 1)
    if again.size:
        raise ReadbackError(f"columns: nodes {_first(again)} match more than one digit")
    digit = np.where(hits.any(axis=0), hits.argmax(axis=0), -1).astype(np.int8)
    f = filt[10]
    odd = np.flatnonzero(f > 1)
    if odd.size:
        raise ReadbackError(f"columns: nodes {_first(odd)} have filter verdicts {_first(f[odd])}, neither 0 nor 1")
    want = np.where(f == 1, raw[0], EXPORT_NONE)
    odd = np.flatnonzero(raw[10] != want)
    if odd.size:
        raise ReadbackError(f"columns: nodes {_first(odd)} have raw {_first(raw[10, odd])} for the digit-0 pod that does not "
                            f"tolerate, filter {_first(f[odd])}, and raw {_first(raw[0, odd])} for the one that does")
    if (fin != raw).any():  # weight 1, no normaliser
        odd = np.flatnonzero((fin != raw).any(axis=0))
        raise ReadbackError(f"columns: nodes {_first(odd)} have a final score other than the raw one")
    return (1 - f).astype(np.uint8), digit


READERS = {"planes": read_planes, "columns": read_columns}


# ---------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------
class Refused(Exception):
    """The model refuses the operation; nothing changed."""


class TableModel:
    """The node table a context must hold: two arrays and whether NodeUnschedulable is in the filter list."""

    def __init__(self):
        self.unsched = None  # no upload yet
        self.digit = None
        self.has_nu = True

    @property
    def n(self):
        return None if self.unsched is None else len(self.unsched)

    @property
    def filters(self):
        return [NU] if self.has_nu else []

    @staticmethod
    def _clean(u, d):
        u, d = np.asarray(u), np.asarray(d).astype(np.int64)
        return (u != 0).astype(np.uint8), np.where((d >= 0) & (d <= 9), d, -1).astype(np.int8)

    def upload(self, u, d):
        self.unsched, self.digit = self._clean(u, d)

    def patch(self, idx, u, d):
        idx = np.asarray(idx, np.int64)
        if self.unsched is None or len(np.unique(idx)) != len(idx) or (idx < 0).any() or (idx >= self.n).any():
            raise Refused
        self.unsched[idx], self.digit[idx] = self._clean(u, d)

    def set_filters(self, filters):
        self.has_nu = NU in filters

    def upload_score_column(self, k, scores):
        """A score column leaves both columns and the planes as they are."""
        if self.unsched is None or len(scores) != self.n:
            raise Refused

    def expected(self):
        """What each observer must see: the planes fold the filter list into X, the columns hold `unsched` itself
        and the export kernel applies the filter list when it reads them."""
        seen = self.unsched if self.has_nu else np.zeros_like(self.unsched)
        return {"planes": (seen.copy(), self.digit.copy()), "columns": (seen.copy(), self.digit.copy())}


def describe(op):
    kind = op[0]
    if kind == "upload":
        return f"upload n={len(op[1])}"
    if kind in ("patch", "bad_patch"):
        idx = np.asarray(op[1])
        return f"{kind} of {len(idx)} at {_first(idx, 4)}{'...' if len(idx) > 4 else ''}"
    if kind == "filters":
        return f"filters {list(op[1])}"
    if kind == "column":
        return f"score column {op[1]}"
    if kind in ("batch", "seq"):
        return f"{kind} of {len(op[1])} pods" + (f" cap {op[3]}" if kind == "seq" else "")
    return kind


def compare(got, want, where, observer):
    gu, gd = got
    wu, wd = want
    bad = np.flatnonzero((gu != wu) | (gd != wd))
    assert bad.size == 0, (f"{where}: {observer} differ at {bad.size} nodes, first {_first(bad)}: got (unsched, digit) "
                           f"{list(zip(_first(gu[bad]), _first(gd[bad])))} want {list(zip(_first(wu[bad]), _first(wd[bad])))}")


def read_back(ctx, model, where, observers=("columns", "planes")):
    want = model.expected()
    for name in observers:
        try:
            got = READERS[name](ctx, model.n, model.filters)
        except ReadbackError as e:
            raise ReadbackError(f"{where}: {e}") from None
        compare(got, want[name], where, name)


def run_case(ctx, ops, refused, oracle=None, label=""):
    """Apply `ops` to `ctx` and to a TableModel, and read the whole table back through both observers after every one.

    Operations: ("upload", u, d) ("patch", idx, u, d) ("bad_patch", idx, u, d) ("filters", names) ("column", k, scores)
    ("batch", pd, pt) ("seq", pd, pt, cap) ("release",). `refused` is what the context raises for a call it refuses
    (MshError on a device, AssertionError over the oracle); a bad_patch must raise it and leave every read-back as it was.
    "batch" sets a list with the uploaded score columns around one schedule_batch call and compares it with
    oracle.c_schedule_batch. "seq" is a sequential call compared with oracle.c_schedule_sequential whose counts are then
    held: node_pod_counts is compared after every operation, and since the plane sweeps need the counts zeroed, the planes
    are read again only from ("release",) on; the columns are read after every operation throughout."""
    model = TableModel()
    ctx.set_plugins(model.filters, [NN], NN_SCORE)
    counts, cols, held = None, {}, False
    for k, op in enumerate(ops):
        where = f"{label} op {k} ({describe(op)})"
        kind = op[0]
        if kind == "upload":
            ctx.upload_nodes(op[1], op[2])
            model.upload(op[1], op[2])
            counts, cols, held = np.zeros(model.n, np.int32), {}, False
        elif kind == "patch":
            ctx.patch_nodes(op[1], op[2], op[3])
            model.patch(op[1], op[2], op[3])
        elif kind == "bad_patch":
            try:
                model.patch(op[1], op[2], op[3])
            except Refused:
                pass
            else:
                raise AssertionError(f"{where}: the model accepts this patch")
            try:
                ctx.patch_nodes(op[1], op[2], op[3])
            except refused:
                pass
            else:
                raise AssertionError(f"{where}: the context accepted the patch")
        elif kind == "filters":
            model.set_filters(op[1])
            ctx.set_plugins(model.filters, [NN], NN_SCORE)
        elif kind == "column":
            model.upload_score_column(op[1], op[2])
            ctx.upload_score_column(f"ScoreColumn{op[1]}", op[2])
            cols[op[1]] = np.asarray(op[2], np.int64)
        elif kind == "batch":
            names = [NN] + [f"ScoreColumn{c}" for c in sorted(cols)]
            ctx.set_plugins(model.filters, [NN], [ScoreCfg(s, 1, 0) for s in names])
            got = ctx.schedule_batch(op[1], op[2])
            ps = oracle.PluginSet(model.filters, [NN], names, [1] * len(names), [0] * len(names))
            want = oracle.c_schedule_batch(model.unsched, model.digit, op[1], op[2], ps, cols=cols)
            for g, w, name in zip(got, want, ("idx", "score", "status")):
                bad = np.flatnonzero(np.asarray(g) != w)
                assert bad.size == 0, f"{where}: {name} differs at pods {_first(bad)}: got {_first(np.asarray(g)[bad])} want {_first(w[bad])}"
        elif kind == "seq":
            ctx.set_plugins(model.filters, [NN], NN_SCORE)
            got = ctx.schedule_sequential(op[1], op[2], op[3])
            ps = oracle.PluginSet(model.filters, [NN], [NN], [1], [0])
            *want, counts = oracle.c_schedule_sequential(model.unsched, model.digit, op[1], op[2], ps, op[3], counts.copy())
            counts = np.array(counts, np.int32)
            for g, w, name in zip(got, want, ("idx", "score", "status")):
                bad = np.flatnonzero(np.asarray(g) != w)
                assert bad.size == 0, f"{where}: {name} differs at pods {_first(bad)}: got {_first(np.asarray(g)[bad])} want {_first(w[bad])}"
            held = True
        elif kind == "release":
            held = False
        else:
            raise ValueError(kind)
        if model.n is None:
            continue  # nothing to read before the first upload
        got = np.asarray(ctx.node_pod_counts())
        assert got.shape == counts.shape, f"{where}: node_pod_counts has {len(got)} nodes, not {len(counts)}"
        bad = np.flatnonzero(got != counts)
        assert bad.size == 0, f"{where}: node_pod_counts differs at nodes {_first(bad)}: got {_first(got[bad])} want {_first(counts[bad])}"
        read_back(ctx, model, where, ("columns",) if held else ("columns", "planes"))
        if not held:
            counts[:] = 0  # read_planes leaves them zeroed


# ---------------------------------------------------------------------------------------
# start tables and the written cases
# ---------------------------------------------------------------------------------------
def start_table(n, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    return (rng.random(n) < 0.4).astype(np.uint8), rng.integers(-1, 10, n).astype(np.int8)


def one_node_indices(n):
    """The indices of the one-node patches that exist at this n, without repeats, in order."""
    want = [0, 1, 2, 3, 4, 31, 32, 63, 64, 255, 256, 1023, 1024, n - 1, ((n - 1) // 32) * 32]
    return sorted({i for i in want if 0 <= i < n})


def one_node_case(n, i):
    """Five kinds of change at node i: unsched only, digit only, both, digit to -1 and back, and a patch to the same
    values. The start table is arranged so that every other node of i's word differs from each value written: none has
    the new `unsched`, and none has a digit that i is given, so an entry landing in a wrong lane, dword or slot shows."""
    u, d = start_table(n, i)
    w0 = (i // 32) * 32
    word = np.arange(w0, min(w0 + 32, n))
    u0, d0 = int(u[i]), (int(d[i]) if d[i] >= 0 else 3)
    d[i] = d0
    d1, d2 = (d0 + 3) % 10, (d0 + 7) % 10
    spare = [v for v in range(-1, 10) if v not in (d0, d1, d2, -1)] + [d0]  # the neighbours may keep i's old digit
    rng = np.random.default_rng(n * 4099 + i)
    others = word[word != i]
    u[others] = u0  # ... and its old unsched: the new one, 1 - u0, is then i's alone in the word
    d[others] = rng.choice(spare, len(others))
    one = lambda uu, dd: ("patch", np.array([i], np.int32), np.array([uu], np.uint8), np.array([dd], np.int8))
    return [("upload", u, d),
            one(1 - u0, d0),      # unsched only
            one(1 - u0, d1),      # digit only
            one(u0, d2),          # both
            one(u0, -1),          # digit to -1 ...
            one(u0, d2),          # ... and back
            one(u0, d2)]          # the same values again


def _patch(rng, model_u, model_d, idx):
    """A patch at `idx` that changes every entry: unsched flipped, another digit."""
    idx = np.asarray(idx, np.int32)
    return ("patch", idx, (1 - model_u[idx]).astype(np.uint8),
            ((model_d[idx].astype(np.int64) + 1 + rng.integers(1, 10, len(idx))) % 11 - 1).astype(np.int8))


class _Builder:
    """A case under construction: the ops, with a model alongside so that a patch can be drawn against the table
    it meets."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.m = TableModel()
        self.ops = []

    def upload(self, n, seed=0):
        u, d = start_table(n, seed)
        self.m.upload(u, d)
        self.ops.append(("upload", u, d))
        return self

    def patch(self, idx):
        op = _patch(self.rng, self.m.unsched, self.m.digit, idx)
        self.m.patch(*op[1:])
        self.ops.append(op)
        return self

    def bad_patch(self, idx):
        idx = np.asarray(idx, np.int32)
        self.ops.append(("bad_patch", idx, np.ones(len(idx), np.uint8), np.full(len(idx), 5, np.int8)))
        return self

    def filters(self, names):
        self.m.set_filters(names)
        self.ops.append(("filters", list(names)))
        return self

    def column(self, k):
        self.ops.append(("column", k, self.rng.integers(-50, 50, self.m.n).astype(np.int64)))
        return self

    def batch(self, p=64):
        self.ops.append(("batch", self.rng.integers(-1, 10, p).astype(np.int8), (self.rng.random(p) < 0.5).astype(np.uint8)))
        return self

    def seq(self, p, cap):
        self.ops.append(("seq", self.rng.integers(0, 10, p).astype(np.int8), (self.rng.random(p) < 0.5).astype(np.uint8), cap))
        return self

    def release(self):
        self.ops.append(("release",))
        return self


def many_node_cases(n):
    """(name, ops) of the many-node patches that exist at this n."""
    words = (n + 31) // 32
    out = []
    b = lambda k: _Builder(n * 131 + k)
    for w in sorted({0, words // 2, words - 1}):
        if (w + 1) * 32 <= n:
            out.append((f"all 32 nodes of word {w}", b(w).upload(n, 1).patch(np.arange(32 * w, 32 * w + 32)).ops))
    if words > 64:
        rng = np.random.default_rng(n)
        ws = np.sort(rng.choice(words - 1, 64, replace=False))  # whole words: every slot exists
        idx = ws * 32 + rng.integers(0, 32, 64)
        out.append(("64 entries in 64 words", b(100).upload(n, 2).patch(idx).ops))
    if n >= 128:
        w = max(0, words // 2 - 1)
        out.append(("64 entries packed into two words", b(101).upload(n, 3).patch(np.arange(32 * w, 32 * w + 64)).ops))
        idx = np.sort(np.random.default_rng(n + 1).choice(n, 64, replace=False))[::-1]
        out.append(("64 entries in descending order", b(102).upload(n, 4).patch(idx.copy()).ops))
    if n >= 192:
        p = np.random.default_rng(n + 2).permutation(n)
        out.append(("63, 64 and 65 entries", b(103).upload(n, 5).patch(p[:63]).patch(p[63:127]).patch(p[127:192]).ops))
    out.append(("count = n", b(104).upload(n, 6).patch(np.random.default_rng(n + 3).permutation(n)).ops))
    return out


def sequence_cases():
    """(name, ops) of the written sequences; tables of 1,025 and 2,500 nodes (a V tail in the last word, three blocks)."""
    out = []
    for n in (1025, 2500):
        b = lambda k: _Builder(n * 17 + k)
        p = np.random.default_rng(n + 9).permutation(n)
        a_idx, b_idx, big, big2 = p[:20], p[20:50], p[50:150], p[150:300]
        out.append((f"n={n} patch A then a disjoint patch B", b(0).upload(n, 7).patch(a_idx).patch(b_idx).ops))
        out.append((f"n={n} inline then scattered", b(1).upload(n, 8).patch(a_idx).patch(big).ops))
        out.append((f"n={n} scattered then inline", b(2).upload(n, 9).patch(big).patch(a_idx).patch(big2).ops))
        out.append((f"n={n} patch, filter off, filter on",
                    b(3).upload(n, 10).patch(a_idx).filters([]).filters([NU]).patch(big).filters([]).filters([NU]).ops))
        out.append((f"n={n} filter off, patch without the filter, filter on",
                    b(4).upload(n, 11).filters([]).patch(a_idx).patch(big).filters([NU]).ops))
        out.append((f"n={n} patch, score column, patch",
                    b(5).upload(n, 12).patch(a_idx).column(1).batch().patch(b_idx).batch().column(0).patch(big).batch().ops))
        out.append((f"n={n} a patch between two sequential calls keeps the counts",
                    b(6).upload(n, 13).seq(n // 2, 2).patch(a_idx).seq(n, 2).patch(big).seq(n, 3).release().ops))
    b = _Builder(99)
    b.upload(2500, 14).upload(40, 15).patch([39]).upload(2500, 16).patch([39, 40, 2499])
    out.append(("upload 2500, upload 40, patch 39, upload 2500", b.ops))
    b = _Builder(98)
    b.upload(2500, 17).patch(np.arange(1000, 1100)).upload(40, 18).patch([0, 39]).upload(1025, 19).patch([1024])
    out.append(("shrinking and growing uploads around patches", b.ops))
    return out


def refused_cases():
    """(name, ops): a patch before any upload (the first case: a family runs on one fresh context), a duplicate index, an index of n and an index of -1, alone and among
    valid entries, inline and scattered; the table read back afterwards is the one before."""
    out = []
    for n in (33, 2500):
        b = _Builder(n + 5)
        if n == 33:  # the family's first case meets a fresh context
            b.bad_patch([0])
        b.upload(n, 20).patch([n - 1])
        b.bad_patch([3, 3]).bad_patch([n]).bad_patch([-1])
        b.bad_patch([0, 1, 2, n]).bad_patch([4, -1, 5]).bad_patch(list(range(20)) + [7])
        if n > 100:
            b.bad_patch(list(range(100)) + [n]).bad_patch(list(range(100)) + [50])
        b.patch([0])
        out.append((f"n={n} refused patches", b.ops))
    return out


def seq_waves_case(n=2500):
    """An inline patch at n = 2,500 that touches the first, a middle and the last word, then a scattered one: read on
    each instance of the sequential kernel, which consume the plane layout differently."""
    return _Builder(4242).upload(n, 21).patch([0, 31, 32, 1023, 1024, 1300, n - 4, n - 1]).patch(np.arange(900, 1100)).ops


def hand_families():
    """{family: [(name, ops), ...]}: one family runs on one context."""
    fam = {}
    for n in SIZES:
        fam[f"one_node[{n}]"] = [(f"n={n} node {i}", one_node_case(n, i)) for i in one_node_indices(n)]
        fam[f"many_node[{n}]"] = [(f"n={n} {name}", ops) for name, ops in many_node_cases(n)]
    seqs = sequence_cases()
    fam["sequences[1025]"] = [c for c in seqs if c[0].startswith("n=1025")]
    fam["sequences[2500]"] = [c for c in seqs if c[0].startswith("n=2500")]
    fam["sequences[resize]"] = [c for c in seqs if not c[0].startswith("n=")]
    fam["refused"] = refused_cases()
    return fam


# ---------------------------------------------------------------------------------------
# seeded traces
# ---------------------------------------------------------------------------------------
TRACE_SIZES = (1, 33, 100, 1000, 1024, 1025, 2500)
TRACE_COUNTS = (1, 2, 5, 31, 32, 33, 63, 64, 65, 66, 200)


def trace(seed, ops=TRACE_OPS):
    """One seeded list of `ops` operations at n <= 2,500: uploads up and down the sizes, patches on both sides of the
    inline limit (some of them refused), filter-list changes, score columns with a batch check, and `count = n`."""
    rng = np.random.default_rng(seed)
    b = _Builder(seed)
    b.upload(int(rng.choice(TRACE_SIZES)), seed)
    while len(b.ops) < ops:
        n, r = b.m.n, rng.random()
        if r < 0.12:
            b.upload(int(rng.choice(TRACE_SIZES)), seed + len(b.ops))
        elif r < 0.62:
            c = min(int(rng.choice(TRACE_COUNTS)), n)
            if rng.random() < 0.5:  # a run of neighbours, else spread over the table
                s = int(rng.integers(0, n - c + 1))
                idx = np.arange(s, s + c)
            else:
                idx = rng.choice(n, c, replace=False)
            b.patch(rng.permutation(idx))
        elif r < 0.67:
            b.patch(rng.permutation(n))
        elif r < 0.82:
            b.filters([] if b.m.has_nu else [NU])
        elif r < 0.90:
            b.column(int(rng.integers(0, 4))).batch()
        else:
            c = min(int(rng.choice(TRACE_COUNTS)), n)
            idx = list(rng.choice(n, c, replace=False))
            b.bad_patch(idx + [int(rng.choice([n, -1, idx[0]]))])
    return b.ops[:ops]


def trace_set():
    return [(f"trace seed {TRACE_SEED0 + k}", trace(TRACE_SEED0 + k)) for k in range(TRACE_COUNT)]
