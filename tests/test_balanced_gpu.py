"""NodeResourcesBalancedAllocation in sequential-commit mode on the GPU (msh_schedule_sequential_balanced and friends;
csrc/msh_seq_balanced.hip).

Every comparison is bit-exact on idx, score, status, node_pod_counts(), the `used` half of node_resources(),
spread_counts(), the class and preference columns, the group modes and the weights. The expected values come from
tests/balanced_ref.py: the plain serial loop for tiny shapes, the numpy per-pod loop otherwise (tests/test_balanced.py
shows on the CPU that the two agree). The kernel holds NPL nodes per thread on 1, 4 or 16 waves; the limits are read
from msh_seq_balanced_max_nodes."""
from __future__ import annotations

import numpy as np
import pytest

import balanced_ref as BR
import classes_ref as KR
import prefs_ref as PR
import soft_spread_ref as SR
import spread_ref as S
from test_balanced import SWEEP_SEEDS, big_quads, decider_triples
from test_classes import case_plugins
from test_classes_gpu import device_call, rand_amounts, rand_case, refused
from test_soft_spread_gpu import SMirror

pytestmark = pytest.mark.gpu
NONE, LEAST, MOST = BR.NONE, BR.LEAST, BR.MOST


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.close()


class BMirror(SMirror):
    """SMirror with the balanced weight."""

    def __init__(self, ctx, msh, O, ps, u, nd, *a, wb=1, **kw):
        super().__init__(ctx, msh, O, ps, u, nd, *a, **kw)
        self.balanced_weight(wb)

    def balanced_weight(self, wb):
        self.wb = wb
        self.ctx.set_balanced_score(wb)

    def expect(self, pd, pt, grp, cls, req=None, scalar=0):
        n, p = len(self.u), len(pd)
        ref = BR.serial if n * p <= 2 * 10**4 else BR.per_pod
        if req is None:
            a, us, rq = S.no_res(n, p)
        else:
            a, us, rq = self.alloc, self.used, np.asarray(req, np.int64)
        return ref(self.O, self.u, self.nd, pd, pt, self.ps, self.eff(scalar), a, us, rq, self.zone, grp, self.skew,
                   self.mode, self.weight, self.rw, self.bits, self.PC or self.C, cls, self.A, self.T, *self.w,
                   self.modes, self.ws, self.wb, self.counts, self.cnt)

    def call(self, pd, pt, grp, cls, req=None, scalar=0, what=""):
        got = self.ctx.schedule_sequential_balanced(pd, pt, grp, cls, req, scalar)
        want = self.expect(pd, pt, grp, cls, req, scalar)
        self.compare(got, want, what)
        self.commit(want, req is not None)
        self.verify(what)
        return want

    def verify(self, what=""):
        super().verify(what)
        assert self.ctx.balanced_score() == self.wb, f"{what}: balanced weight"


def plain(ctx, msh, oracle, alloc, used, cap=None, mode=NONE, weight=1, rw=None, wb=1, **kw):
    """Schedulable nodes without digits (NodeNumber scores 0 everywhere), no zones, groups or classes."""
    n = np.asarray(alloc).shape[1]
    return BMirror(ctx, msh, oracle, oracle.PluginSet(), np.zeros(n, np.uint8), np.full(n, -1, np.int8), None, (),
                   alloc, used, cap, mode, weight, rw, wb=wb, **kw)


def pods(p):
    return np.zeros(p, np.int8), np.ones(p, np.uint8)


def uneven(rng, nres, n, p, unit=1):
    """Uneven nodes against cpu-heavy, memory-heavy and empty pods: the balanced term decides often."""
    alloc = rng.integers(40, 400, (nres, n))
    alloc[0] *= rng.choice([1, 3], n)
    alloc[1] *= rng.choice([1, 3], n)
    used = (rng.random((nres, n)) < 0.3) * rng.integers(0, 40, (nres, n))
    req = rng.integers(0, 5, (nres, p))
    kind = rng.integers(0, 4, p)
    req[0] += np.where(kind == 0, rng.integers(5, 30, p), 0)
    req[1] += np.where(kind == 1, rng.integers(5, 30, p), 0)
    req[:, kind == 3] = 0
    return (alloc * unit).astype(np.int64), (used * unit).astype(np.int64), (req * unit).astype(np.int64)


@pytest.mark.parametrize("nres,mode", [(r, m) for r in (2, 3, 4) for m in (NONE, LEAST, MOST)])
def test_instance_thresholds(msh, oracle, ctx, nres, mode):
    """One table at and one just above each wave threshold of the instance (1, 4 and 16 waves), and the limit, with
    classes, preferences and pods of hard groups, of soft groups and of none mixed; one node past the limit is refused
    with the limit in the message."""
    rng = np.random.default_rng(7000 + 100 * mode + nres)
    lim = ctx.seq_balanced_max_nodes(nres)
    assert lim == ctx.seq_soft_max_nodes(nres) == (4096 if nres <= 2 else 2048)
    ps = oracle.PluginSet(weights=[3], normalize=[(2, 0, 3, 1, 2)[nres]])
    for t, n in enumerate((lim // 16, lim // 16 + 1, lim // 4, lim // 4 + 1, lim)):
        p = int(rng.integers(150, 250)) | 1
        u, nd, pd, pt = rand_case(rng, n, p)
        C = int(rng.choice([3, 17, 64]))
        bits, _ = KR.gen_bits(rng, n, C)
        A, T = PR.gen_prefs(rng, n, C)
        cls = rng.integers(-1, C, p).astype(np.int32)
        zone = rng.integers(-1, (8, 64)[t % 2], n)
        grp = rng.integers(-1, 16, p)
        modes = rng.integers(0, 2, 16).astype(np.uint8)
        modes[:2] = (0, 1)
        alloc, used, req = uneven(rng, nres, n, p, int(rng.choice([1, 2**33])))
        cap = rng.integers(1, 4, n) * (rng.random(n) < min(1.0, 1.2 * p / n))
        m = BMirror(ctx, msh, oracle, ps, u, nd, zone, rng.choice([1, 2, 3], 16), alloc, used, cap, mode,
                    int(rng.choice([1, 7])), rng.integers(1, 101, nres), bits if t % 3 else None, C if t % 3 else 0,
                    A=A, T=T, PC=C, w=(int(rng.integers(0, 101)), int(rng.integers(0, 101))) if t % 4 else (0, 0),
                    modes=modes, ws=int(rng.integers(1, 101)), wb=int(rng.integers(1, 101)))
        m.call(pd, pt, grp, cls, req, what=f"mode={mode} nres={nres} n={n} p={p}")
    n = lim + 1
    m = BMirror(ctx, msh, oracle, ps, np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros(n, np.int32), [1],
                np.ones((nres, n), np.int64), mode=mode, modes=[1])
    msg = refused(msh, msh._native.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_balanced, np.zeros(3, np.int8),
                  np.zeros(3, np.uint8), np.zeros(3, np.int32), None, np.ones((nres, 3), np.int64))
    assert f"{lim:,} nodes".replace(",", "") in msg.replace(",", "")
    m.verify("past the limit")


@pytest.mark.parametrize("unit", [1, 1 << 43])
def test_decider_triples_pick_the_node(msh, oracle, ctx, unit):
    """Every decider (an input on which the float64 rule differs from the exact floor, from float32 or from rounding
    to nearest) on node 2d, a robust node with the larger of the two values on node 2d + 1, and pod d of a class
    that admits only the pair, with nothing requested: the rule's value being the larger, the tie goes to node 2d;
    the near miss's being the larger, node 2d + 1 wins. The near miss would pick the other one each time. Scaled by
    2^43 the fractions are the same doubles and the amounts need both halves of the conversion."""
    triples, robust = decider_triples()
    D = len(triples)
    assert D == 48
    alloc = np.zeros((2, 2 * D), np.int64)
    used = np.zeros((2, 2 * D), np.int64)
    expect = np.zeros(D, np.int32)
    for d, (_, (q0, c0, q1, c1), v, o) in enumerate(triples):
        r0, rc0, r1, rc1 = robust[max(v, o)]
        alloc[:, 2 * d], used[:, 2 * d] = (c0, c1), (q0, q1)
        alloc[:, 2 * d + 1], used[:, 2 * d + 1] = (rc0, rc1), (r0, r1)
        expect[d] = 2 * d if v > o else 2 * d + 1
    bits = np.repeat(np.uint64(1) << np.arange(D, dtype=np.uint64), 2)
    pd, pt = pods(D)
    m = plain(ctx, msh, oracle, alloc * unit, used * unit, mode=NONE, wb=1, bits=bits, C=D)
    want = m.call(pd, pt, None, np.arange(D, dtype=np.int32), np.zeros((2, D), np.int64), what=f"unit {unit}")
    assert np.array_equal(want[0], expect)
    assert np.array_equal(want[1], [max(v, o) for _, _, v, o in triples])


def test_amounts_near_two_to_the_55(msh, oracle, ctx):
    """Amounts that are no doubles, one node each and room for one pod: the pods take the nodes in the order of
    their BS, and every score is a BS."""
    quads = big_quads()
    n = len(quads)
    alloc = np.array([[c0 for _, c0, _, _ in quads], [c1 for _, _, _, c1 in quads]], np.int64)
    used = np.array([[q0 for q0, _, _, _ in quads], [q1 for _, _, q1, _ in quads]], np.int64)
    pd, pt = pods(n)
    for mode in (NONE, MOST):
        m = plain(ctx, msh, oracle, alloc, used, cap=np.ones(n, np.int64), mode=mode, wb=3)
        want = m.call(pd, pt, None, None, np.zeros((2, n), np.int64), what=f"mode {mode}")
        if mode == NONE:
            assert np.array_equal(np.sort(want[1])[::-1], want[1])
            assert sorted(want[1]) == sorted(3 * BR.bs(*q) for q in quads)


def test_a_tie_across_a_wave_boundary_goes_to_the_lower_index(msh, oracle, ctx):
    """Nodes 200 (wave 0) and 270 (wave 1) hold the same, highest BS; node 100 the same BS without room."""
    n = 300
    alloc = np.full((2, n), 100, np.int64)
    used = np.stack([np.zeros(n, np.int64), np.full(n, 60, np.int64)])
    used[:, [100, 200, 270]] = 30
    cap = np.ones(n, np.int64)
    cap[100] = 0
    m = plain(ctx, msh, oracle, alloc, used, cap=cap)
    pd, pt = pods(3)
    want = m.call(pd, pt, None, None, np.full((2, 3), 5, np.int64), what="tie")
    assert list(want[0]) == [200, 270, 0] and list(want[1]) == [100, 100, BR.bs(5, 100, 65, 100)]


def test_balanced_outvotes_least_allocated_and_loses_to_a_larger_weight(msh, oracle, ctx):
    """Node 0 is emptier and lopsided, node 1 fuller and even. LeastAllocated alone takes node 0; with the balanced
    term at equal weights node 1 wins (40 + 100 against 60 + 40); with W_res = 10 node 0 again (640 against 500)."""
    alloc = np.full((2, 2), 100, np.int64)
    used = np.array([[0, 50], [60, 50]], np.int64)
    pd, pt = pods(1)
    req = np.full((2, 1), 10, np.int64)
    for weight, wb, node, score in ((1, 0, 0, 60), (1, 1, 1, 140), (10, 1, 0, 640)):
        m = plain(ctx, msh, oracle, alloc, used, mode=LEAST, weight=weight, rw=[1, 1], wb=wb)
        want = m.call(pd, pt, None, None, req, what=f"W_res {weight}, w_balanced {wb}")
        assert (want[0][0], want[1][0]) == (node, score)


def test_capacity_zero_and_clamped_fractions_on_the_device(msh, oracle, ctx):
    """A resource without capacity (f = 1), a lowered alloc (q > c, clamped), both with pods that request nothing."""
    alloc = np.array([[0, 4, 10, 0], [2, 2, 10, 0]], np.int64)
    used = np.array([[7, 9, 5, 0], [1, 1, 5, 3]], np.int64)
    pd, pt = pods(4)
    m = plain(ctx, msh, oracle, alloc, used, cap=np.ones(4, np.int64))
    want = m.call(pd, pt, None, None, np.zeros((2, 4), np.int64), what="c = 0 and q > c")
    assert list(want[0]) == [2, 3, 0, 1] and list(want[1]) == [100, 100, 50, 50]


def test_used_amounts_are_carried_between_calls(msh, oracle, ctx):
    rng = np.random.default_rng(7100)
    n, p = 333, 120
    alloc, used, req = uneven(rng, 2, n, 2 * p)
    for mode in (NONE, LEAST):
        m = plain(ctx, msh, oracle, alloc, used, mode=mode, wb=2)
        pd, pt = pods(p)
        a = m.call(pd, pt, None, None, req[:, :p], what="first call")
        b = m.call(pd, pt, None, None, req[:, p:], what="second call")
        whole = plain(ctx, msh, oracle, alloc, used, mode=mode, wb=2)
        pd2, pt2 = pods(2 * p)
        w = whole.call(pd2, pt2, None, None, req, what="both at once")
        assert np.array_equal(np.concatenate([a[0], b[0]]), w[0]) and np.array_equal(b[4], w[4])


def test_classes_preferences_and_both_kinds_of_groups_in_one_call(msh, oracle, ctx):
    rng = np.random.default_rng(7200)
    n, p, C = 700, 299, 9
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = uneven(rng, 3, n, p)
    bits, _ = KR.gen_bits(rng, n, C)
    A, T = PR.gen_prefs(rng, n, C)
    cls = rng.integers(-1, C, p).astype(np.int32)
    grp = rng.integers(-1, 4, p).astype(np.int32)
    m = BMirror(ctx, msh, oracle, oracle.PluginSet(weights=[2], normalize=[1]), u, nd, rng.integers(-1, 6, n), [1, 2, 1, 3],
                alloc, used, rng.integers(1, 3, n), MOST, 3, [5, 0, 9], bits, C, A=A, T=T, PC=C, w=(11, 7),
                modes=[0, 1, 1, 0], ws=13, wb=17)
    want = m.call(pd, pt, grp, cls, req, what="everything")
    m.balanced_weight(0)
    m2 = BMirror(ctx, msh, oracle, oracle.PluginSet(weights=[2], normalize=[1]), u, nd, m.zone, [1, 2, 1, 3],
                 alloc, used, m.cap, MOST, 3, [5, 0, 9], bits, C, A=A, T=T, PC=C, w=(11, 7), modes=[0, 1, 1, 0], ws=13, wb=0)
    zero = m2.call(pd, pt, grp, cls, req, what="everything, w_balanced 0")
    assert (want[0] != zero[0]).sum() > 10  # the term decided


def test_weight_zero_is_the_soft_call(msh, oracle, ctx):
    """w_balanced == 0: _balanced is _soft, output for output and state for state, also where a balanced call would be
    refused (one resource, no table)."""
    rng = np.random.default_rng(7300)
    n, p = 500, 150
    u, nd, pd, pt = rand_case(rng, n, p)
    zone, grp = rng.integers(-1, 4, n), rng.integers(-1, 3, p).astype(np.int32)
    ps = oracle.PluginSet(weights=[2], normalize=[2])
    for nres in (2, 1, 0):
        alloc, used, req = rand_amounts(rng, nres, n, p) if nres else (None, None, None)
        outs = []
        for name in ("schedule_sequential_balanced", "schedule_sequential_soft"):
            m = BMirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2, 1], alloc, used, np.full(n, 2), LEAST if nres else NONE, 3,
                        [1] * nres, modes=[0, 1, 1], ws=9, wb=0)
            got = getattr(ctx, name)(pd, pt, grp, None, req)
            want = SMirror.expect(m, pd, pt, grp, None, req)
            m.compare(got, want, f"{name}, nres {nres}")
            m.commit(want, nres > 0)
            m.verify(name)
            outs.append(got)
        assert all(np.array_equal(x, y) for x, y in zip(*outs))


def test_refusals_change_nothing(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(7400)
    n, p = 200, 30
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = uneven(rng, 2, n, p)
    zone = rng.integers(-1, 4, n)
    grp = rng.integers(-1, 2, p).astype(np.int32)
    ps = oracle.PluginSet()
    call = ctx.schedule_sequential_balanced
    for bad in (-1, 101):
        refused(msh, E.MSH_ERR_INVALID, ctx.set_balanced_score, bad)
    # fewer than two resources; no table at all
    m = BMirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2], alloc[:1], used[:1], None, NONE, modes=[0, 1], ws=5, wb=1)
    assert "two resources" in refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, None, req[:1])
    m.verify("one resource")
    m = BMirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2], None, None, None, NONE, modes=[0, 1], ws=5, wb=1)
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, None, None)
    m.verify("no table")
    # nres different from the table's
    m = BMirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2], alloc, used, None, NONE, modes=[0, 1], ws=5, wb=1)
    m.call(pd, pt, grp, None, req, what="before")
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, None, None)
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, None, req[:1])
    # a request past 2^55 (the host form looks at the requests); negative requests as ever
    big = req.copy()
    big[1, 3] = (1 << 55) + 1
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, grp, None, big)
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, grp, None, -req - 1)
    # random tie-break, score columns
    ctx.set_tiebreak("random", 1)
    refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, None, req)
    ctx.set_tiebreak("first")
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig("NodeNumber"), msh.ScorePluginConfig("ScoreColumn0")])
    assert "score-column" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, None, req)
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig("NodeNumber")])
    # the key's sum: 100 * (645 + 2 + 3 + 5 + 1) = 65,600 is refused, 100 * 655 = 65,500 <= 65,534 is taken
    m.weights(2, 3)
    m.score(LEAST, 645, [1, 1])
    assert "656" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, None, req)
    m.verify("after the key refusal")
    m.score(LEAST, 644, [1, 1])
    m.call(pd, pt, grp, None, req, what="655 fits")
    m.balanced_weight(100)
    m.score(LEAST, 546, [1, 1])
    assert "656" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, None, req)
    m.score(LEAST, 545, [1, 1])
    m.call(pd, pt, grp, None, req, what="655 fits, w_balanced 100")
    # an amount of the table past 2^55, in mode NONE too; the same table is taken with w_balanced = 0
    m.score(NONE)
    m.alloc = m.alloc.copy()
    m.alloc[1, 7] = (1 << 55) + 1
    ctx.patch_node_resources(np.array([7], np.int32), alloc=m.alloc[:, [7]])
    assert "2^55" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, None, req)
    m.verify("after the amount refusal")
    m.balanced_weight(0)
    got = call(pd, pt, grp, None, req)
    want = SMirror.expect(m, pd, pt, grp, None, req)
    m.compare(got, want, "w_balanced 0 on the large table")
    m.commit(want)
    m.verify("w_balanced 0 on the large table")


def test_device_form_on_two_streams(msh, oracle, ctx):
    """The device form agrees with the host form's reference: group and class values out of range are pods without
    one; two streams, one after the other on the same counts and amounts."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7500)
    n, p, C = 300, 250, 5
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = uneven(rng, 2, n, p)
    bits, _ = KR.gen_bits(rng, n, C)
    A, T = PR.gen_prefs(rng, n, C)
    cls = rng.choice(np.array([-1, -7, C, 0, 1, 2, 3, 4], np.int32), p)
    grp = rng.choice(np.array([-1, -9, 3, S.INT32_MAX, 0, 1, 2], np.int32), p)
    m = BMirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, rng.integers(-1, 7, n), [1, 1, 2], alloc, used, np.full(n, 3),
                LEAST, 2, [1, 1], bits=bits, C=C, A=A, T=T, PC=C, w=(20, 30), modes=[1, 0, 1], ws=50, wb=40)
    for k in range(2):
        want = m.expect(pd, pt, grp, cls, req)
        got = device_call(torch, ctx.schedule_sequential_balanced_device, pd, pt, grp, cls, req,
                          torch.cuda.Stream(torch.device("cuda:0")))
        m.compare(got, want, f"stream {k}")
        m.commit(want)
        m.verify(f"stream {k}")


SWEEP_CHUNKS = [list(SWEEP_SEEDS)[k:k + 10] for k in range(0, len(SWEEP_SEEDS), 10)]


@pytest.mark.parametrize("seeds", SWEEP_CHUNKS, ids=lambda s: f"{s[0]}-{s[-1]}")
def test_random_sweep(msh, oracle, ctx, seeds):
    torch = pytest.importorskip("torch")
    st = torch.cuda.Stream(torch.device("cuda:0"))
    for seed in seeds:
        c = BR.gen_case(seed)
        made = []
        for form in ("host", "device"):
            m = BMirror(ctx, msh, oracle, case_plugins(oracle, c), c["unsched"], c["node_digit"], c["zone"], c["max_skew"],
                        c["alloc"], c["used"], c["cap"], c["score_mode"], c["rs_weight"], c["rw"], c["bits"],
                        c["C"] if c["bits"] is not None else 0, A=c["A"], T=c["T"], PC=c["C"],
                        w=(c["w_aff"], c["w_taint"]), modes=c["modes"], ws=c["w_spread"], wb=c["w_balanced"])
            args = (c["pod_digit"], c["pod_tol"], c["group"], c["pod_class"], c["req"])
            if form == "host":
                made.append(m.call(*args, what=f"seed {seed}"))
            else:
                got = device_call(torch, ctx.schedule_sequential_balanced_device, *args, st)
                m.compare(got, made[0], f"seed {seed}, device form")
                m.commit(made[0])
                m.verify(f"seed {seed}, device form")


def test_scheduler_end_to_end(msh, oracle):
    """k8s-shaped nodes of three sizes and cpu-heavy, memory-heavy and small pods through
    Scheduler(resource_score="least", balanced_allocation_weight=1), against balanced_ref."""
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    rng = np.random.default_rng(7600)
    n, p = 120, 260
    sizes = (("4", "32Gi"), ("16", "16Gi"), ("8", "16Gi"))
    nodes = []
    for i in range(n):
        cpu, mem = sizes[int(rng.integers(0, 3))]
        nodes.append({"metadata": {"name": f"node{i:04d}"}, "spec": {},
                      "status": {"allocatable": {"cpu": cpu, "memory": mem, "pods": 4}}})
    shapes = (("2", "1Gi"), ("250m", "4Gi"), ("500m", "512Mi"), ("0", "0"))
    pods_ = []
    for j in range(p):
        cpu, mem = shapes[int(rng.integers(0, 4))]
        pods_.append({"metadata": {"name": f"pod{j}"},
                      "spec": {"containers": [{"resources": {"requests": {"cpu": cpu, "memory": mem}}}]}})
    s = msh.Scheduler(resources=("cpu", "memory"), resource_score="least", balanced_allocation_weight=1)
    try:
        res = s.schedule_sequential(pods_, nodes)
        nl = [nodes[i] for i in s.nodes.order]
        table = msh.pack_pods(pods_)
        alloc = np.array([msh.snapshot.node_allocatable(x, ("cpu", "memory")) for x in nl], np.int64).T
        req = np.array([msh.snapshot.pod_requests(x, ("cpu", "memory")) for x in pods_], np.int64).T
        ref = lambda wb: BR.per_pod(oracle, s.nodes.unsched, s.nodes.digit, table.digit, table.tolerates,
                                    oracle.PluginSet(), np.full(n, 4), alloc, np.zeros_like(alloc), req, None, None, (),
                                    LEAST, 1, [1, 1], None, 0, None, None, None, 0, 0, None, 0, wb)
        want = ref(1)
        got_idx = np.array([r.node_index if r.outcome == msh.Outcome.PLACED else -1 for r in res])
        assert np.array_equal(got_idx, want[0])
        got_score = np.array([r.score if r.outcome == msh.Outcome.PLACED else 0 for r in res])
        assert np.array_equal(got_score, want[1])
        assert np.array_equal(s.ctx.node_pod_counts(), want[3])
        assert np.array_equal(s.ctx.node_resources()[1], want[4])
        assert (want[0] != ref(0)[0]).sum() > 30  # the balanced term decided
    finally:
        s.close()
