"""Preferred node affinity and PreferNoSchedule scores in sequential-commit mode on the GPU
(msh_schedule_sequential_prefs and friends; csrc/msh_seq_prefs.hip).

Every comparison is bit-exact on idx, score, status, node_pod_counts(), the `used` half of node_resources(),
spread_counts(), node_class_bits() and node_class_prefs(). The expected values come from tests/prefs_ref.py: the
plain serial loop for tiny shapes, the numpy per-pod loop otherwise (tests/test_prefs.py shows on the CPU that the two
agree). The kernel holds NPL nodes per thread on 1, 4 or 16 waves; the limits are read from msh_seq_prefs_max_nodes."""
from __future__ import annotations

import numpy as np
import pytest

import classes_ref as KR
import prefs_ref as PR
import spread_ref as S
from test_classes import case_plugins
from test_classes_gpu import (MODE_NAMES, Mirror, device_call, mask_bits, rand_amounts, rand_case, refused)
from test_prefs import SWEEP_SEEDS

pytestmark = pytest.mark.gpu
NONE, LEAST, MOST = PR.NONE, PR.LEAST, PR.MOST


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.close()


class PMirror(Mirror):
    """Mirror with the preference column and weights; PC is the column's class count."""

    def __init__(self, ctx, msh, O, ps, u, nd, *a, A=None, T=None, PC=0, w=(1, 1), **kw):
        super().__init__(ctx, msh, O, ps, u, nd, *a, **kw)
        self.A = self.T = None
        self.PC = 0
        self.w = w
        ctx.set_preference_weights(*w)
        if PC:
            self.prefs(PC, A, T)

    def prefs(self, PC, A, T):
        n = len(self.u)
        self.ctx.upload_node_class_prefs(PC, A, T)
        self.PC = PC
        self.A = np.zeros((PC, n), np.uint16) if A is None else np.array(A, np.uint16).reshape(PC, n)
        self.T = np.zeros((PC, n), np.uint16) if T is None else np.array(T, np.uint16).reshape(PC, n)

    def weights(self, w_aff, w_taint):
        self.w = (w_aff, w_taint)
        self.ctx.set_preference_weights(w_aff, w_taint)

    def expect(self, pd, pt, grp, cls, req=None, scalar=0):
        n, p = len(self.u), len(pd)
        ref = PR.serial if n * p <= 2 * 10**4 else PR.per_pod
        if req is None:
            a, us, rq = S.no_res(n, p)
        else:
            a, us, rq = self.alloc, self.used, np.asarray(req, np.int64)
        return ref(self.O, self.u, self.nd, pd, pt, self.ps, self.eff(scalar), a, us, rq, self.zone, grp, self.skew,
                   self.mode, self.weight, self.rw, self.bits, self.PC or self.C, cls, self.A, self.T, *self.w,
                   self.counts, self.cnt)

    def call(self, pd, pt, grp, cls, req=None, scalar=0, what=""):
        got = self.ctx.schedule_sequential_prefs(pd, pt, grp, cls, req, scalar)
        want = self.expect(pd, pt, grp, cls, req, scalar)
        self.compare(got, want, what)
        self.commit(want, req is not None)
        self.verify(what)
        return want

    def verify(self, what=""):
        super().verify(what)
        col = self.ctx.node_class_prefs()
        if not self.PC:
            assert col is None, f"{what}: a preference column appeared"
        else:
            assert col is not None and col[0] == self.PC and np.array_equal(col[1], self.A) \
                and np.array_equal(col[2], self.T), f"{what}: preference column"
        assert self.ctx.preference_weights() == tuple(self.w), f"{what}: weights"


def lim_npl(ctx, nres):
    lim = ctx.seq_prefs_max_nodes(nres)
    return lim, lim // 1024


def plain(ctx, msh, oracle, n, A=None, T=None, cap=None, w=(1, 1), ps=None, PC=1, **kw):
    """n schedulable nodes without digits (NodeNumber scores 0 everywhere) unless ps is given."""
    ps = ps or oracle.PluginSet()
    return PMirror(ctx, msh, oracle, ps, np.zeros(n, np.uint8), np.full(n, -1, np.int8), cap=cap, A=A, T=T, PC=PC, w=w, **kw)


def pods(p, digit=0):
    return np.full(p, digit, np.int8), np.ones(p, np.uint8)


@pytest.mark.parametrize("nres,mode", [(0, NONE)] + [(r, m) for r in (1, 2, 3, 4) for m in (NONE, LEAST, MOST)])
def test_instance_thresholds(msh, oracle, ctx, nres, mode):
    """n = 1, 5, 65, at each wave threshold of the instance and one past it, and the limit; one node past the limit is
    refused with the limit in the message. Sizes past a threshold are no multiple of NPL or 32."""
    rng = np.random.default_rng(1000 * mode + nres)
    lim, npl = lim_npl(ctx, nres)
    assert lim == (4096 if nres <= 2 else 2048)
    ps = oracle.PluginSet(weights=[3], normalize=[(2, 0, 3, 1, 2)[nres]])
    for t, n in enumerate((1, 5, 65, lim // 16, lim // 16 + 1, lim // 4, lim // 4 + 1, lim)):
        p = int(rng.integers(200, 300)) | 1
        u, nd, pd, pt = rand_case(rng, n, p)
        C = int(rng.choice([3, 17, 64]))
        bits, _ = KR.gen_bits(rng, n, C)
        A, T = PR.gen_prefs(rng, n, C)
        cls = rng.integers(-1, C, p).astype(np.int32)
        grouped = t % 2 == 0
        zone = rng.integers(-1, 8, n) if grouped else None
        grp = rng.integers(-1, 16, p) if grouped else None
        alloc = used = req = None
        if nres:
            alloc, used, req = rand_amounts(rng, nres, n, p, int(rng.choice([1, 2**33])))
        cap = rng.integers(0, 4, n) if n < 300 else rng.integers(1, 4, n) * (rng.random(n) < 0.4 * p / n)
        m = PMirror(ctx, msh, oracle, ps, u, nd, zone, rng.choice([1, 2, 3], 16) if grouped else (), alloc, used, cap,
                    mode, int(rng.choice([1, 7])), rng.integers(1, 101, nres), bits if t % 3 else None, C if t % 3 else 0,
                    A=A, T=T, PC=C, w=(int(rng.integers(1, 101)), int(rng.integers(1, 101))))
        m.call(pd, pt, grp, cls, req, what=f"mode={mode} nres={nres} n={n} p={p}")
    n = lim + 1
    m = PMirror(ctx, msh, oracle, ps, np.zeros(n, np.uint8), np.zeros(n, np.int8),
                alloc=np.ones((nres, n), np.int64) if nres else None, mode=mode, PC=1)
    msg = refused(msh, msh._native.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_prefs, np.zeros(3, np.int8),
                  np.zeros(3, np.uint8), None, np.zeros(3, np.int32), np.ones((nres, 3), np.int64) if nres else None)
    assert f"{lim:,} nodes".replace(",", "") in msg.replace(",", "")
    m.verify("past the limit")


@pytest.mark.parametrize("what", ["A by capacity", "A by a resource", "T by capacity", "T by a resource"])
def test_fill_up(msh, oracle, ctx, what):
    """The node holding the class's best raw value fills mid-call; later pods are normalised by the next one. A
    column normalised once would keep scoring the runner-up at 50 (A) or 50 (T) and send the pods elsewhere."""
    n, p = 300, 12
    A = np.zeros((1, n), np.uint16)
    T = np.zeros((1, n), np.uint16)
    if what[0] == "A":
        # after node 200 fills, node 70's 50 is the maximum: na = 100 there
        A[0, 200], A[0, 70] = 100, 50
        full, then, then_score = 200, 70, 3 * 100 + 3 * 100 + 99
    else:
        # node 200 holds the only T = 4 and is preferred for its A; once it is full maxT is 2 and maxA 0: node 70
        # (T = 0) scores nt = 100 as before, the nodes with T = 2 now score 0 instead of 50
        T[0] = 2
        T[0, 200], A[0, 200], T[0, 70] = 4, 100, 0
        full, then, then_score = 200, 70, 3 * 0 + 3 * 100 + 99
    cap = np.full(n, 100)
    alloc = np.full((1, n), 1000, np.int64)
    alloc[0, 5] = 10**6  # LEAST prefers node 5 by a point; the preferences outweigh it
    req = np.full((1, p), 10, np.int64)
    if "capacity" in what:
        cap[full] = 4
    else:
        alloc[0, full] = 45
    m = plain(ctx, msh, oracle, n, A, T, cap, w=(5 if what[0] == "T" else 3, 3), alloc=alloc, mode=LEAST)
    want = m.call(*pods(p), None, np.zeros(p, np.int32), req, what=what)
    assert want[0].tolist() == [full] * 4 + [then] * 8
    assert want[1][4] == then_score


@pytest.mark.parametrize("how", ["unschedulable", "capacity", "request", "zone skew", "class bit"])
def test_the_largest_raw_value_on_an_infeasible_node(msh, oracle, ctx, how):
    """maxA and maxT are taken over the feasible nodes: node 100 holds the largest A and T and is infeasible by one
    conjunct; the others are normalised by node 40's values."""
    n, p = 260, 3
    A = np.zeros((1, n), np.uint16)
    T = np.ones((1, n), np.uint16)
    A[0, 100], A[0, 40], A[0, 41] = 1000, 30, 10
    T[0, 100], T[0, 40] = 9, 0
    u = np.zeros(n, np.uint8)
    cap = np.full(n, 5)
    alloc = np.full((1, n), 100, np.int64)
    zone = skew = grp = bits = None
    if how == "unschedulable":
        u[100] = 1
    elif how == "capacity":
        cap[100] = 0
    elif how == "request":
        alloc[0, 100] = 3
    elif how == "zone skew":  # nodes 100 and 101 in zone 1; node 101 alone takes the priming pod's request
        zone = np.zeros(n, np.int32)
        zone[[100, 101]] = 1
        alloc[0, 101] = 1000
        grp = np.zeros(p, np.int32)
    else:
        bits = np.ones(n, np.uint64)
        bits[100] = 0
    m = PMirror(ctx, msh, oracle, oracle.PluginSet(), u, np.full(n, -1, np.int8), zone,
                [1] if zone is not None else (), alloc, None, cap, NONE, bits=bits, C=1 if bits is not None else 0,
                A=A, T=T, PC=1, w=(2, 1))
    if how == "zone skew":  # zone 1 is one pod ahead: a second pod there would exceed max_skew 1
        first = m.call(np.zeros(1, np.int8), np.zeros(1, np.uint8), np.zeros(1, np.int32), np.full(1, -1, np.int32),
                       np.full((1, 1), 500, np.int64), what="prime")
        assert first[0][0] == 101
    pt = np.zeros(p, np.uint8)
    want = m.call(np.zeros(p, np.int8), pt, grp, np.zeros(p, np.int32), np.full((1, p), 5, np.int64), what=how)
    assert want[0][0] == 40 and want[1][0] == 2 * 100 + 100


@pytest.mark.parametrize("waves", [4, 16])
def test_maximum_and_winner_in_different_waves(msh, oracle, ctx, waves):
    """The node holding maxA is not the winner (its T is worst) and sits in another wave than the winner; also the
    maximum in the last held thread and in node 0."""
    lim, npl = lim_npl(ctx, 2)
    n = lim // 4 if waves == 4 else lim
    rng = np.random.default_rng(waves)
    for amax_at, win_at in ((0, n - 1), (n - 1, 0), (64 * npl + 1, n - 2), (n - 2, 64 * npl - 1)):
        A = rng.integers(0, 20, (1, n)).astype(np.uint16)
        T = np.full((1, n), 3, np.uint16)
        A[0, amax_at], T[0, amax_at] = 200, 6   # na = 100, nt = 0
        A[0, win_at], T[0, win_at] = 150, 0     # na = 75, nt = 100
        m = plain(ctx, msh, oracle, n, A, T, np.full(n, 1), w=(1, 1), alloc=np.full((2, n), 50, np.int64), mode=MOST)
        want = m.call(*pods(5), None, np.zeros(5, np.int32), np.ones((2, 5), np.int64), what=f"max {amax_at} win {win_at}")
        assert want[0][0] == win_at and want[0][1] == amax_at


def test_zero_maxima(msh, oracle, ctx):
    n, p = 130, 6
    rng = np.random.default_rng(5)
    A = np.zeros((4, n), np.uint16)
    T = np.zeros((4, n), np.uint16)
    T[0] = rng.integers(0, 3, n)    # class 0: maxA == 0, maxT > 0
    A[1] = rng.integers(0, 50, n)   # class 1: the reverse
    A[3], T[3] = 7, 2               # class 3: constant rows: every quotient 100 / 0
    m = plain(ctx, msh, oracle, n, A, T, np.full(n, 1), w=(4, 9), PC=4)
    cls = np.array([0, 1, 2, 3, -1, 0] * 4, np.int32)
    want = m.call(*pods(len(cls)), None, cls, what="zero maxima")
    assert (want[1][cls == 2] == 900).all() and (want[1][cls == -1] == 900).all() and (want[1][cls == 3] == 400).all()


@pytest.mark.parametrize("which", ["A", "T"])
def test_truncation(msh, oracle, ctx, which):
    """Quotients 1/3, 2/3, 1/7, 99/100, 65,535/65,535 and 1/65,535: floor(100 x / max) exactly."""
    n = 70
    for num, den in ((1, 3), (2, 3), (1, 7), (99, 100), (65535, 65535), (1, 65535), (65534, 65535), (32768, 65535)):
        col = np.zeros((1, n), np.uint16)
        col[0, 3], col[0, 66] = den, num
        other = np.zeros((1, n), np.uint16)
        cap = np.zeros(n, np.int64)
        cap[[3, 66, 9]] = (1, 1, 1) if which == "A" else (5, 1, 0)
        m = plain(ctx, msh, oracle, n, col if which == "A" else other, col if which == "T" else other, cap, w=(7, 7))
        want = m.call(*pods(2), None, np.zeros(2, np.int32), what=f"{which} {num}/{den}")
        q = 100 * num // den
        if which == "A":
            assert want[0].tolist() == [3, 66] and want[1][0] == 7 * 100 + 700
        else:
            assert want[0][0] == (66 if num < den else 3) and want[1][0] == 7 * (100 - (q if num < den else 100))


def test_weights_and_the_key_limit(msh, oracle, ctx):
    rng = np.random.default_rng(9)
    n, p = 200, 60
    A, T = PR.gen_prefs(rng, n, 6)
    A[0], T[0] = rng.integers(0, 101, n), rng.integers(0, 3, n)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    u, nd, pd, pt = rand_case(rng, n, p)
    cls = rng.integers(-1, 6, p).astype(np.int32)
    for w, wres in (((0, 37), 1), ((37, 0), 1), ((100, 100), 455), ((1, 0), 654)):
        m = PMirror(ctx, msh, oracle, oracle.PluginSet(weights=[1], normalize=[1]), u, nd, None, (), alloc, used,
                    np.full(n, 2), LEAST, wres, [1, 3], A=A, T=T, PC=6, w=w)
        m.call(pd, pt, None, cls, req, what=f"w={w} W_res={wres}")
    m.score(LEAST, 456, [1, 3])
    m.weights(100, 100)
    msg = refused(msh, msh._native.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_prefs, pd, pt, None, cls, req)
    assert "656" in msg
    m.verify("after the refusal")
    for bad in ((-1, 0), (0, 101), (101, 0)):
        refused(msh, msh._native.MSH_ERR_INVALID, ctx.set_preference_weights, *bad)
    assert ctx.preference_weights() == (100, 100)


@pytest.mark.parametrize("nm", [0, 1, 2, 3])
def test_node_number_normalize_modes(msh, oracle, ctx, nm):
    """NodeNumber weight 3: a preference of weight 1 is outvoted by a match (300 or 30 against at most 200), one of
    weight 100 outvotes it."""
    n, p = 140, 40
    rng = np.random.default_rng(20 + nm)
    nd = rng.integers(0, 3, n).astype(np.int8)
    A = rng.integers(0, 101, (2, n)).astype(np.uint16)
    T = rng.integers(0, 3, (2, n)).astype(np.uint16)
    out = []
    for w in ((1, 1), (100, 100)):
        m = PMirror(ctx, msh, oracle, oracle.PluginSet(weights=[3], normalize=[nm]), np.zeros(n, np.uint8), nd,
                    cap=np.full(n, 1), A=A, T=T, PC=2, w=w)
        out.append(m.call(rng.integers(0, 3, p).astype(np.int8), np.ones(p, np.uint8), None,
                          rng.integers(0, 2, p).astype(np.int32), what=f"normalize {nm} w={w}"))
    assert (out[0][2] == PR.PLACED).all()


@pytest.mark.parametrize("waves", [4, 16])
def test_phase_skipping_keeps_the_slots_in_step(msh, oracle, ctx, waves):
    """Consecutive pods alternate between a preferring class, a class without a raw value and no class, in runs of
    1, 2 and 3: the maxima's slots advance only with the pods that use them."""
    lim, npl = lim_npl(ctx, 1)
    n = lim // 4 if waves == 4 else lim - 3
    rng = np.random.default_rng(30 + waves)
    A = np.zeros((3, n), np.uint16)
    T = np.zeros((3, n), np.uint16)
    A[0], T[0] = rng.integers(0, 101, n), rng.integers(0, 3, n)
    T[2] = rng.integers(0, 2, n)
    pat = [0, 1, -1, 0, 0, 1, 2, -1, -1, 0, 2, 2, 2, 1, 0, -1, 0, 1, 1, 0]
    cls = np.array(pat * 10, np.int32)
    p = len(cls)
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    cap = (rng.random(n) < 0.1).astype(np.int64)
    m = PMirror(ctx, msh, oracle, oracle.PluginSet(weights=[1], normalize=[3]), u, nd, None, (), alloc, used, cap, MOST,
                bits=mask_bits({0: rng.random(n) < 0.7, 1: rng.random(n) < 0.5, 2: np.ones(n, bool)}), C=3,
                A=A, T=T, PC=3, w=(5, 11))
    m.call(pd, pt, None, cls, req, what="alternating")


def test_block_boundaries_and_groups(msh, oracle, ctx):
    """More than 128 pods: the class changes exactly at pods 64 and 128 (the prefetched record of a block's first pod),
    and grouped, placed, preferring pods follow one another within a group (both barriers)."""
    lim, npl = lim_npl(ctx, 2)
    n = lim // 16 + 7
    rng = np.random.default_rng(40)
    A, T = PR.gen_prefs(rng, n, 4)
    A[0], A[3] = rng.integers(1, 101, n), rng.integers(1, 101, n)
    p = 200
    cls = np.full(p, -1, np.int32)
    cls[64:128], cls[128:] = 0, 3
    cls[63], cls[127] = 3, 1
    grp = np.zeros(p, np.int32)
    grp[::7] = -1
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    m = PMirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, rng.integers(0, 5, n), [2], alloc, used, np.full(n, 2), LEAST,
                A=A, T=T, PC=4, w=(10, 10))
    want = m.call(pd, pt, grp, cls, req, what="blocks and groups")
    placed = want[2] == PR.PLACED
    assert (placed[:-1] & placed[1:] & (grp[:-1] == 0) & (grp[1:] == 0) & (cls[:-1] >= 0)).sum() > 50


def test_no_feasible_node_and_the_next_pod(msh, oracle, ctx):
    n = 300
    rng = np.random.default_rng(50)
    A = rng.integers(0, 101, (2, n)).astype(np.uint16)
    T = rng.integers(0, 3, (2, n)).astype(np.uint16)
    bits = mask_bits({0: np.zeros(n, bool), 1: np.ones(n, bool)})
    m = plain(ctx, msh, oracle, n, A, T, np.full(n, 1), w=(1, 1), PC=2, bits=bits, C=2)
    cls = np.array([1, 0, 1, 0, 0, 1], np.int32)
    want = m.call(*pods(6), None, cls, what="no feasible node")
    assert (want[2][cls == 0] == PR.FIT_ERROR).all() and (want[2][cls == 1] == PR.PLACED).all()


def test_equivalences(msh, oracle, ctx):
    """Weights 0 is _classes on the same inputs; no column and pod_class None is _spread_scored plus w_taint * 100."""
    rng = np.random.default_rng(60)
    n, p = 500, 150
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    zone, grp = rng.integers(-1, 4, n), rng.integers(-1, 3, p).astype(np.int32)
    bits, _ = KR.gen_bits(rng, n, 5)
    A, T = PR.gen_prefs(rng, n, 5)
    cls = rng.integers(-1, 5, p).astype(np.int32)
    ps = oracle.PluginSet(weights=[2], normalize=[2])
    args = (zone, [1, 2, 1], alloc, used, np.full(n, 2), LEAST, 3, [1, 2])
    m = PMirror(ctx, msh, oracle, ps, u, nd, *args, bits, 5, A=A, T=T, PC=5, w=(0, 0))
    a = m.call(pd, pt, grp, cls, req, what="weights 0")
    m2 = Mirror(ctx, msh, oracle, ps, u, nd, *args, bits, 5)
    b = m2.call(pd, pt, grp, cls, req, what="_classes")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    m3 = PMirror(ctx, msh, oracle, ps, u, nd, *args, w=(13, 7))
    c = m3.call(pd, pt, grp, None, req, what="no column, no classes")
    m4 = Mirror(ctx, msh, oracle, ps, u, nd, *args)
    d = ctx.schedule_sequential_spread_scored(pd, pt, grp, req)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[2], d[2])
    assert np.array_equal(c[1], d[1] + 700 * (d[2] == PR.PLACED))
    ctx.set_preference_weights(0, 0)
    del m4


def test_device_form(msh, oracle, ctx):
    """Class values out of range are pods without a class; two streams, one after the other on the same counts."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(70)
    n, p, C = 300, 250, 5
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    bits, _ = KR.gen_bits(rng, n, C)
    A, T = PR.gen_prefs(rng, n, C)
    A[0] = rng.integers(0, 101, n)
    cls = rng.choice(np.array([-1, -7, C, S.INT32_MAX, 0, 1, 2, 3, 4], np.int32), p)
    m = PMirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, None, (), alloc, used, np.full(n, 3), LEAST, bits=bits, C=C,
                A=A, T=T, PC=C, w=(20, 30))
    for k in range(2):
        want = m.expect(pd, pt, None, cls, req)
        got = device_call(torch, ctx.schedule_sequential_prefs_device, pd, pt, None, cls, req,
                          torch.cuda.Stream(torch.device("cuda:0")))
        m.compare(got, want, f"stream {k}")
        m.commit(want)
        m.verify(f"stream {k}")
    for bad in (-7, C, S.INT32_MAX):
        refused(msh, msh._native.MSH_ERR_INVALID, ctx.schedule_sequential_prefs, pd[:3], pt[:3], None,
                np.array([0, bad, 1], np.int32), req[:, :3])
    m.verify("after the refusals")


def test_refusals_in_order_change_nothing(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(80)
    n, p = 200, 30
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    bits, _ = KR.gen_bits(rng, n, 4)
    A, T = PR.gen_prefs(rng, n, 4)
    m = PMirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, None, [1], alloc, used, bits=bits, C=4, A=A, T=T, PC=4, w=(2, 3))
    cls = rng.integers(-1, 4, p).astype(np.int32)
    call = ctx.schedule_sequential_prefs
    m.call(pd, pt, None, cls, req, what="before")
    # the column's writers
    refused(msh, E.MSH_ERR_INVALID, lambda: ctx._check(ctx._lib.msh_upload_node_class_prefs(ctx.handle, n - 1, 4, None, None)))
    refused(msh, E.MSH_ERR_INVALID, lambda: ctx._check(ctx._lib.msh_upload_node_class_prefs(ctx.handle, n, 0, None, None)))
    refused(msh, E.MSH_ERR_INVALID, lambda: ctx._check(ctx._lib.msh_upload_node_class_prefs(ctx.handle, n, 65, None, None)))
    z = np.zeros((4, 2), np.uint16)
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_node_class_prefs, [0, 0], z, z)
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_node_class_prefs, [0, n], z, z)
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_node_class_prefs, [-1, 0], z, z)
    m.verify("after the refused writers")
    # _classes's refusals, in its order
    grp = np.zeros(p, np.int32)
    ctx.set_tiebreak("random", 1)
    refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, cls, req[:1])   # RANDOM before everything below
    ctx.set_tiebreak("first")
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, cls, req[:1])         # groups without zones, before nres
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, None, cls, req[:1])      # nres != the table's
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, None, cls, -req)
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, None, np.full(p, 4, np.int32), req)
    m.score(LEAST, 1, [1, 1])
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, None, cls, None)           # nres != the setting's
    # then the two of this call: unequal C, neither column, and the key (after the others)
    ctx.upload_node_class_bits(5, bits)
    m.C = 5
    m.score(LEAST, 651, [1, 1])
    assert "C = 5" in refused(msh, E.MSH_ERR_STATE, call, pd, pt, None, cls, req)   # unequal C before the key
    m.classes(4, bits)
    assert "656" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, None, cls, req)
    m.score(LEAST, 1, [1, 1])
    ctx.clear_node_class_bits()
    ctx.clear_node_class_prefs()
    m.bits, m.C, keepA, keepT, m.PC = None, 0, m.A, m.T, 0
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, None, cls, req)            # pod_class with neither column
    refused(msh, E.MSH_ERR_STATE, ctx.patch_node_class_prefs, [0])        # no column to patch
    m.verify("after the refused calls")
    m.call(pd, pt, None, None, req, what="no column, no classes")
    m.prefs(4, keepA, keepT)
    m.call(pd, pt, None, cls, req, what="a preference column alone: every node admits every class")
    c2 = msh.DeviceContext(0)
    try:
        c2.set_preference_weights(1, 1)
        refused(msh, E.MSH_ERR_STATE, lambda: c2._check(c2._lib.msh_upload_node_class_prefs(c2.handle, 0, 1, None, None)))
        refused(msh, E.MSH_ERR_STATE, c2.schedule_sequential_prefs, pd, pt, None, None)
    finally:
        c2.close()


def test_state_rules(msh, oracle, ctx):
    rng = np.random.default_rng(90)
    n, p = 130, 40
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    bits, _ = KR.gen_bits(rng, n, 9)
    A, T = PR.gen_prefs(rng, n, 9)
    A[0] = rng.integers(0, 101, n)
    m = PMirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, rng.integers(0, 3, n), [1], alloc, used, rng.integers(1, 4, n),
                bits=bits, C=9, A=A, T=T, PC=9, w=(6, 4))
    cls = rng.integers(-1, 9, p).astype(np.int32)
    m.call(pd, pt, None, cls, req, what="before")
    # every other writer keeps the column
    ctx.patch_nodes([0], [0], [1])
    m.u[0], m.nd[0] = 0, 1
    ctx.patch_node_capacity([1], [3])
    m.cap[1] = 3
    ctx.patch_node_resources([2], alloc[:, [2]] + 5)
    m.alloc = m.alloc.copy()
    m.alloc[:, 2] += 5
    ctx.upload_node_zones(m.zone)
    m.cnt[:] = 0
    ctx.reset_node_pod_counts()
    m.counts[:] = 0
    m.patch([4, 9], np.array([0, 511], np.uint64))  # the class masks change: the call sees it
    m.verify("after the other writers")
    m.call(pd, pt, np.zeros(p, np.int32), cls, req, what="after the other writers")
    # the other entry points ignore the column and the weights
    got = ctx.schedule_sequential_classes(pd, pt, None, cls, req)
    want = Mirror.expect(m, pd, pt, None, cls, req)
    m.compare(got, want, "_classes ignores the column and the weights")
    m.commit(want)
    m.verify("_classes")
    # patch, read back, and the call sees it
    idx = np.array([7, 0, 100], np.int32)
    pa, pt_ = rng.integers(0, 65536, (9, 3)).astype(np.uint16), rng.integers(0, 4, (9, 3)).astype(np.uint16)
    ctx.patch_node_class_prefs(idx, pa, pt_)
    m.A[:, idx], m.T[:, idx] = pa, pt_
    m.verify("patched")
    m.call(pd, pt, None, cls, req, what="after the patch")
    ctx.patch_node_class_prefs([3], None, np.full((9, 1), 2, np.uint16))  # a None array writes zeros
    m.A[:, 3], m.T[:, 3] = 0, 2
    m.verify("patched with None")
    # clear, then upload_nodes drops it
    ctx.clear_node_class_prefs()
    keepA, keepT, m.PC = m.A, m.T, 0
    m.A = m.T = None
    m.verify("cleared")
    m.call(pd, pt, None, cls, req, what="class masks alone: A = T = 0")
    m.prefs(9, keepA, None)
    assert not ctx.node_class_prefs()[2].any()
    ctx.upload_nodes(u, nd)
    assert ctx.node_class_prefs() is None and ctx.preference_weights() == (6, 4)


SWEEP_CHUNKS = [list(SWEEP_SEEDS)[k:k + 20] for k in range(0, len(SWEEP_SEEDS), 20)]


@pytest.mark.parametrize("seeds", SWEEP_CHUNKS, ids=lambda s: f"{s[0]}-{s[-1]}")
def test_random_sweep(msh, oracle, ctx, seeds):
    for seed in seeds:
        c = PR.gen_case(seed)
        m = PMirror(ctx, msh, oracle, case_plugins(oracle, c), c["unsched"], c["node_digit"], c["zone"], c["max_skew"],
                    c["alloc"], None, c["cap"], c["score_mode"], c["rs_weight"], c["rw"], c["bits"],
                    c["C"] if c["bits"] is not None else 0, A=c["A"], T=c["T"], PC=c["C"], w=(c["w_aff"], c["w_taint"]))
        m.call(c["pod_digit"], c["pod_tol"], c["group"], c["pod_class"], c["req"], what=f"seed {seed}")


def test_scheduler_end_to_end(msh, oracle):
    """k8s-shaped pods and nodes with preferred terms and PreferNoSchedule taints through
    Scheduler(preferred_affinity_weight=1, prefer_no_schedule_weight=1), against constraints.py + prefs_ref."""
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    K = msh.constraints
    rng = np.random.default_rng(100)
    n, p = 150, 260
    zones = ("z0", "z1", "z2")
    nodes = []
    for i in range(n):
        labels = {"pool": ("gpu", "cpu")[int(rng.integers(0, 2))], "zone": zones[int(rng.integers(0, 3))]}
        taints = []
        if rng.random() < 0.3:
            taints.append({"key": "spot", "value": "", "effect": "PreferNoSchedule"})
        if rng.random() < 0.2:
            taints.append({"key": "old", "value": "", "effect": "PreferNoSchedule"})
        if rng.random() < 0.1:
            taints.append({"key": "dedicated", "value": "ml", "effect": "NoSchedule"})
        nodes.append({"metadata": {"name": f"node{i:04d}", "labels": labels}, "spec": {"taints": taints},
                      "status": {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": 2}}})

    def prefer(*terms):
        return {"affinity": {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": w, "preference": {"matchExpressions": [{"key": k, "operator": "In", "values": [v]}]}}
            for w, k, v in terms]}}}
    shapes = [{}, prefer((10, "zone", "z0")), prefer((50, "zone", "z1"), (20, "pool", "gpu")),
              {"tolerations": [{"key": "spot", "operator": "Exists"}]},
              {**prefer((100, "pool", "cpu")), "tolerations": [{"key": "old", "operator": "Exists", "effect": "PreferNoSchedule"}]},
              {"nodeSelector": {"pool": "gpu"}, **prefer((5, "zone", "z2"))}]
    pods_ = []
    for j in range(p):
        spec = dict(shapes[int(rng.integers(0, len(shapes)))])
        spec["containers"] = [{"resources": {"requests": {"cpu": f"{int(rng.integers(0, 3)) * 500}m", "memory": "1Gi"}}}]
        pods_.append({"metadata": {"name": f"pod{j}"}, "spec": spec})
    s = msh.Scheduler(resources=("cpu", "memory"), resource_score="least", preferred_affinity_weight=1,
                      prefer_no_schedule_weight=1)
    try:
        res = s.schedule_sequential(pods_, nodes)
        nl = [nodes[i] for i in s.nodes.order]
        reps = {}
        for x in pods_:
            reps.setdefault(K.class_key(x) + K.preference_key(x), x)
        keys = list(reps)
        bits = np.zeros(n, np.uint64)
        A = np.zeros((len(keys), n), np.int64)
        T = np.zeros((len(keys), n), np.int64)
        for k, kk in enumerate(keys):
            bits |= np.array([K.node_admits(reps[kk], x) for x in nl], bool).astype(np.uint64) << np.uint64(k)
            A[k] = [K.preferred_affinity_score(reps[kk], x) for x in nl]
            T[k] = [K.prefer_no_schedule_count(reps[kk], x) for x in nl]
        cls = np.array([keys.index(K.class_key(x) + K.preference_key(x)) for x in pods_], np.int32)
        table = msh.pack_pods(pods_)
        alloc = np.array([[4000, 8 << 30]] * n, np.int64).T
        req = np.array([msh.snapshot.pod_requests(x, ("cpu", "memory")) for x in pods_], np.int64).T
        want = PR.per_pod(oracle, s.nodes.unsched, s.nodes.digit, table.digit, table.tolerates, oracle.PluginSet(),
                          np.full(n, 2), alloc, np.zeros_like(alloc), req, None, None, (), LEAST, 1, [1, 1], bits,
                          len(keys), cls, A, T, 1, 1)
        got_idx = np.array([r.node_index if r.outcome == msh.Outcome.PLACED else -1 for r in res])
        assert np.array_equal(got_idx, want[0])
        got_score = np.array([r.score if r.outcome == msh.Outcome.PLACED else 0 for r in res])
        assert np.array_equal(got_score, want[1])
        assert np.array_equal(s.ctx.node_pod_counts(), want[3])
        zero = PR.per_pod(oracle, s.nodes.unsched, s.nodes.digit, table.digit, table.tolerates, oracle.PluginSet(),
                          np.full(n, 2), alloc, np.zeros_like(alloc), req, None, None, (), LEAST, 1, [1, 1], bits,
                          len(keys), cls, A, T, 0, 0)
        assert (want[0] != zero[0]).sum() > 30  # the preferences decided
    finally:
        s.close()
