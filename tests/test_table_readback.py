"""The table readers, the model and the written cases of tests/table_readback.py, on the CPU.

The readers are held to the C oracle itself (`OracleCtx`): on start tables of every size, with and without the filter,
they return the model's `expected()`. A capacity-1 sweep costs the oracle n x (n + 8) pod-node visits, 0.5 s for the
eleven of one read-back at n = 2,500, and the cases below make some 900 read-backs, so the bulk runs on `SweepCtx`: an
`OracleCtx` that answers exactly those sweeps (identical pods, capacity 1, zeroed counts, the NodeNumber list) by a closed
form and leaves every other call to the oracle. `test_sweep_closed_form_is_the_oracle` holds the closed form to the C
oracle on every size, every pod kind and both filter lists, and three families run on the plain `OracleCtx` as well.
"""
from __future__ import annotations

import numpy as np
import pytest

import table_readback as T
from oracle_ctx import OracleCtx

NN_ONLY = ([T.NN], [T.NN], [1], [0])


class SweepCtx(OracleCtx):
    def schedule_sequential(self, pod_digit, pod_tol, max_pods_per_node=0, on_commit=None, out=None):
        pd, pt, ps = np.asarray(pod_digit), np.asarray(pod_tol), self.plugins
        sweep = (max_pods_per_node == 1 and len(pd) > 0 and (pd == pd[0]).all() and (pt == pt[0]).all() and 0 <= pd[0] <= 9
                 and (ps.prescore, ps.score, ps.weights, ps.normalize) == NN_ONLY and not self._counts().any())
        if not sweep:
            return super().schedule_sequential(pod_digit, pod_tol, max_pods_per_node, on_commit, out)
        feas = np.ones(self.n_nodes, bool) if ("NodeUnschedulable" not in ps.filters or pt[0]) else self.unsched == 0
        match = feas & (self.digit == pd[0])
        order = np.concatenate([np.flatnonzero(match), np.flatnonzero(feas & ~match)])[:len(pd)]
        k = len(order)
        idx, score, status = np.full(len(pd), -1, np.int32), np.zeros(len(pd), np.int64), np.ones(len(pd), np.int32)
        idx[:k], score[:k], status[:k] = order, np.where(match[order], 10, 0), 0
        self.counts = np.bincount(order, minlength=self.n_nodes).astype(np.int32)
        return idx, score, status


def _run(ctx, ops, oracle, label=""):
    T.run_case(ctx, ops, refused=AssertionError, oracle=oracle, label=label)


@pytest.fixture(scope="module")
def families():
    return T.hand_families()


@pytest.mark.parametrize("n", T.SIZES)
def test_sweep_closed_form_is_the_oracle(oracle, n):
    for seed, filters in ((1, [T.NU]), (2, []), (3, [T.NU])):
        u, d = T.start_table(n, seed)
        if seed == 3:
            u[:] = 1  # nothing feasible for a pod that does not tolerate
        a, b = SweepCtx(), OracleCtx()
        for c in (a, b):
            c.set_plugins(filters, [T.NN], T.NN_SCORE)
            c.upload_nodes(u, d)
        for pd, pt in zip(T.POD_DIGIT.tolist() + [7], T.POD_TOL.tolist() + [0]):
            for p in (n + T.EXTRA_PODS, max(n // 2, 1)):
                for c in (a, b):
                    c.reset_node_pod_counts()
                got = a.schedule_sequential(np.full(p, pd, np.int8), np.full(p, pt, np.uint8), 1)
                want = b.schedule_sequential(np.full(p, pd, np.int8), np.full(p, pt, np.uint8), 1)
                for g, w in zip(got, want):
                    assert (g == w).all(), (n, seed, pd, pt, p)
                assert (a.node_pod_counts() == b.node_pod_counts()).all()


@pytest.mark.parametrize("n", T.SIZES)
def test_readers_invert_the_oracle(oracle, n):
    """Decoding the C oracle's own outputs returns the table: the start tables of the written cases (one per family and
    size; each case's own start table is read back over the oracle when the case runs) and random ones, filter on and off.
    With the filter off the decoded X is all zero."""
    rng = np.random.default_rng(n)
    tables = [T.start_table(n, s) for s in (1, 7, 20)]
    tables += [T.one_node_case(n, i)[0][1:] for i in T.one_node_indices(n)[-2:]]
    tables += [((rng.random(n) < q).astype(np.uint8), rng.integers(-1, 10, n).astype(np.int8)) for q in (0.0, 0.5, 1.0)]
    for u, d in tables if n < 2500 else tables[::2]:
        for filters in ([T.NU], []):
            ctx, m = OracleCtx(), T.TableModel()
            ctx.upload_nodes(u, d)
            m.upload(u, d)
            m.set_filters(filters)
            T.read_back(ctx, m, f"n={n} filters={filters}")
            if not filters:
                assert not T.read_planes(ctx, n, filters)[0].any() and not T.read_columns(ctx, n, filters)[0].any()


def test_readers_raise_on_structure(oracle):
    """Each structural surprise raises and names the nodes."""
    u, d = T.start_table(40, 1)

    class Odd(SweepCtx):
        def __init__(self, how):
            super().__init__()
            self.how = how

        def schedule_sequential(self, *a, **k):
            idx, score, status = super().schedule_sequential(*a, **k)
            if self.how == "index":
                idx[3] = 40
            elif self.how == "twice":
                idx[5] = idx[4]
            elif self.how == "score":
                score[2] = 5
            elif self.how == "count" and a[1][0]:
                idx[39], status[39] = -1, 1
            elif self.how == "late" and a[1][0]:
                idx[41], status[41] = 7, 0
            elif self.how == "status":
                status[-1] = 2
            return idx, score, status

        def export_results(self, *a):
            f, r, o = super().export_results(*a)
            if self.how == "filter":
                f[2, 9] = 0
            elif self.how == "raw":
                r[4, 11] = o[4, 11] = 7
            return f, r, o

    for how, reader, word in (("index", "planes", "outside"), ("twice", "planes", "twice"), ("score", "planes", "neither 0 nor 10"),
                              ("count", "planes", "not n = 40"), ("late", "planes", "past n"), ("status", "planes", "status"),
                              ("filter", "columns", "nodes [9]"), ("raw", "columns", "nodes [11]")):
        ctx = Odd(how)
        ctx.upload_nodes(u, d)
        with pytest.raises(T.ReadbackError, match=word.replace("[", r"\[").replace("]", r"\]")):
            T.READERS[reader](ctx, 40, [T.NU])


def test_completeness_every_single_node_mutant_is_seen(oracle):
    """A 300-node table, every node, `unsched` flipped or `digit` changed to each of its ten other values: both readers
    report a difference at that node and at no other. 3,300 of 3,300."""
    n = 300
    u, d = T.start_table(n, 5)
    caught = 0
    for i in range(n):
        for v in range(-1, 11):  # 10: the unsched flip
            if v == d[i]:
                continue
            u2, d2 = u.copy(), d.copy()
            if v == 10:
                u2[i] ^= 1
            else:
                d2[i] = v
            ctx = SweepCtx()
            ctx.upload_nodes(u2, d2)
            for reader in (T.read_planes, T.read_columns):
                gu, gd = reader(ctx, n, [T.NU])
                assert np.flatnonzero((gu != u) | (gd != d)).tolist() == [i], (i, v, reader.__name__)
            caught += 1
    assert caught == 3300


def _family_names():
    return list(T.hand_families())


@pytest.mark.parametrize("family", _family_names())
def test_hand_cases_pass_over_the_oracle(oracle, families, family):
    ctx = SweepCtx()
    for name, ops in families[family]:
        _run(ctx, ops, oracle, name)


@pytest.mark.parametrize("family", ["one_node[33]", "many_node[1000]", "sequences[1025]", "refused"])
def test_hand_cases_pass_over_the_plain_oracle(oracle, families, family):
    """The same, every sweep by the C oracle's serial loop."""
    ctx = OracleCtx()
    for name, ops in families[family][:4]:
        _run(ctx, ops, oracle, name)


def test_traces_and_seq_waves_case_pass_over_the_oracle(oracle):
    for name, ops in T.trace_set() + [("seq_waves case", T.seq_waves_case())]:
        _run(SweepCtx(), ops, oracle, name)


def test_trace_set_coverage():
    """The 12 traces of 25 operations between them reach every way of producing a table version."""
    sets = T.trace_set()
    assert len(sets) == T.TRACE_COUNT and all(len(ops) == T.TRACE_OPS for _, ops in sets)
    ops = [op for _, t in sets for op in t]
    counts = [len(op[1]) for op in ops if op[0] == "patch"]
    assert any(c <= T.INLINE for c in counts) and any(c > T.INLINE for c in counts) and {63, 64, 65} <= set(counts)
    ns = [len(op[1]) for op in ops if op[0] == "upload"]
    assert max(ns) == 2500 and min(ns) == 1 and any(a > b for a, b in zip(ns, ns[1:]))
    kinds = {op[0] for op in ops}
    assert {"upload", "patch", "bad_patch", "filters", "column", "batch"} <= kinds
    assert [] in [op[1] for op in ops if op[0] == "filters"] and [T.NU] in [op[1] for op in ops if op[0] == "filters"]


# ---------------------------------------------------------------------------------------
# wrong models wired into the oracle context: each must fail a written case
# ---------------------------------------------------------------------------------------
class Mutant(SweepCtx):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self.before = None  # the table before the last patch

    def upload_nodes(self, unsched, digit):
        old_u, old_d, old_n = self.unsched, self.digit, self.n_nodes
        super().upload_nodes(unsched, digit)
        self.before = None
        if self.kind == "upload_keeps_tail" and self.n_nodes < old_n:
            self.unsched = np.concatenate([self.unsched, old_u[self.n_nodes:]])
            self.digit = np.concatenate([self.digit, old_d[self.n_nodes:]])
            self.n_nodes = old_n
            self.counts = np.zeros(old_n, np.int32)

    def set_plugins(self, filters, prescore, score):
        had = "NodeUnschedulable" in self.plugins.filters
        super().set_plugins(filters, prescore, score)
        if self.kind == "filters_forget_patch" and had != ("NodeUnschedulable" in filters) and self.before is not None:
            self.unsched, self.digit = self.before[0].copy(), self.before[1].copy()

    def patch_nodes(self, idx, unsched, digit):
        idx = np.asarray(idx, np.int64)
        assert len(np.unique(idx)) == len(idx) and (idx >= 0).all() and (idx < self.n_nodes).all()
        unsched, digit = np.asarray(unsched, np.uint8), np.asarray(digit, np.int8)
        now = (self.unsched.copy(), self.digit.copy())
        if self.kind == "stale_second_patch" and self.before is not None:
            self.unsched, self.digit = self.before[0].copy(), self.before[1].copy()
        self.before = now
        if self.kind in ("lane_xor_1", "dword_xor_4"):
            j = idx ^ (1 if self.kind == "lane_xor_1" else 4)
            idx = np.where(j < self.n_nodes, j, idx)
        if self.kind == "patch_zeroes_counts":
            self.counts = np.zeros(self.n_nodes, np.int32)
        if (self.kind, len(idx)) in (("skip_64", 64), ("skip_65", 65)):
            return
        if self.kind == "digit_kept_when_unsched_changes":
            digit = np.where(unsched != self.unsched[idx], self.digit[idx], digit)
        self.unsched[idx] = unsched
        self.digit[idx] = digit


MUTANTS = {
    # mutant: (the family searched, a case that must catch it)
    "lane_xor_1": ("one_node[33]", "n=33 node 0"),
    "dword_xor_4": ("one_node[33]", "n=33 node 0"),
    "stale_second_patch": ("sequences[1025]", "n=1025 patch A then a disjoint patch B"),
    "skip_64": ("many_node[1000]", "n=1000 64 entries packed into two words"),
    "skip_65": ("many_node[1000]", "n=1000 63, 64 and 65 entries"),
    "digit_kept_when_unsched_changes": ("one_node[33]", "n=33 node 0"),
    "filters_forget_patch": ("sequences[1025]", "n=1025 patch, filter off, filter on"),
    "upload_keeps_tail": ("sequences[resize]", "upload 2500, upload 40, patch 39, upload 2500"),
    "patch_zeroes_counts": ("sequences[1025]", "n=1025 a patch between two sequential calls keeps the counts"),
}


@pytest.mark.parametrize("kind", list(MUTANTS))
def test_every_wrong_model_fails_a_written_case(oracle, families, kind):
    """Caught by (every case of the family that fails is printed; the one named here must be among them):
      a patch lands at idx ^ 1                      one_node[33], "n=33 node 0" (every one-node case)
      a patch lands at idx ^ 4                      one_node[33], "n=33 node 0" (every one-node case)
      the second patch built on the version before the first
                                                    sequences[1025], "patch A then a disjoint patch B"
      a patch skipped when count == 64              many_node[1000], "64 entries packed into two words"
      a patch skipped when count == 65              many_node[1000], "63, 64 and 65 entries"
      digit left unchanged when unsched changes     one_node[33], "n=33 node 0" (the patch of both)
      set_filters forgets the patch                 sequences[1025], "patch, filter off, filter on"
      a smaller upload keeps the old tail           sequences[resize], "upload 2500, upload 40, patch 39, upload 2500"
      a patch zeroes the pod counts                 sequences[1025], "a patch between two sequential calls keeps the counts"
    """
    family, named = MUTANTS[kind]
    failed = []
    for name, ops in families[family]:
        try:
            _run(Mutant(kind), ops, oracle, name)
        except AssertionError as e:
            failed.append(name)
            print(f"{kind}: {str(e)[:300]}")
    assert named in failed, (kind, failed)


def test_a_batch_call_is_nearly_blind_to_a_cordon_flip(oracle):
    """The record behind this module, not an assertion about the library: on a 5,000-node table, 30 % cordoned, a batch
    of the 22 pod kinds (11 digits, tolerating or not) under NodeNumber at weight 3 with DefaultNormalizeScore changes
    some output for only a few dozen of the 5,000 possible one-node cordon flips. The count is printed."""
    rng = np.random.default_rng(0)
    n = 5000
    u, d = (rng.random(n) < 0.3).astype(np.uint8), rng.integers(-1, 10, n).astype(np.int8)
    pd = np.array(list(range(-1, 10)) * 2, np.int8)
    pt = np.array([0] * 11 + [1] * 11, np.uint8)
    ps = oracle.PluginSet([T.NU], [T.NN], [T.NN], [3], [oracle.NORM_DEFAULT])
    base = oracle.c_schedule_batch(u, d, pd, pt, ps)[:3]
    seen = 0
    for i in range(n):
        u[i] ^= 1
        got = oracle.c_schedule_batch(u, d, pd, pt, ps)[:3]
        u[i] ^= 1
        seen += any((g != b).any() for g, b in zip(got, base))
    print(f"one-node cordon flips a 22-kind batch detects: {seen} of {n} ({100 * seen / n:.2f} %)")
