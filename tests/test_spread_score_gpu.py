"""Topology spread together with a resource score in sequential-commit mode on the GPU
(msh_schedule_sequential_spread_scored and friends; csrc/msh_seq_spread_score.hip).

Every comparison is bit-exact on idx, score, status, node_pod_counts(), the `used` half of node_resources() and
spread_counts(). The expected values come from tests/spread_score_ref.py: the plain serial loop for tiny shapes,
the numpy per-pod loop otherwise (tests/test_spread_score.py shows on the CPU that the two agree, and that the
sweep's generator makes both the spread conjunct and the score decide).

The kernel holds NPL nodes per thread on 1, 4 or 16 waves; the limit is read from msh_seq_spread_scored_max_nodes
(1,024 x NPL), never hard-coded."""
from __future__ import annotations

import numpy as np
import pytest

import node_capacity_ref as CR
import spread_ref as S
import spread_score_ref as X
from test_spread_score import SWEEP_SEEDS, case_args, case_plugins

pytestmark = pytest.mark.gpu
I32MAX = S.INT32_MAX
MODE_NAMES = {X.NONE: "none", X.LEAST: "least", X.MOST: "most"}


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.close()


def set_plugins(ctx, msh, ps):
    ctx.set_plugins(ps.filters, ps.prescore,
                    [msh.ScorePluginConfig(s, w, msh.Normalize(m)) for s, w, m in zip(ps.score, ps.weights, ps.normalize)])


def rand_case(rng, n, p, digits=3, p_unsched=0.2):
    """Few digit classes, so that many nodes tie on NodeNumber and the resource score picks among them."""
    u = (rng.random(n) < p_unsched).astype(np.uint8)
    nd = rng.integers(-1, digits, n).astype(np.int8)
    pd = rng.integers(0, digits, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return u, nd, pd, pt


def rand_amounts(rng, nres, n, p, unit=1):
    alloc = (rng.integers(20, 200, (nres, n)) * unit).astype(np.int64)
    used = (rng.integers(0, 10, (nres, n)) * unit).astype(np.int64)
    req = (rng.integers(0, 4, (nres, p)) * unit).astype(np.int64)
    return alloc, used, req


def refused(msh, code, fn, *a, **kw):
    with pytest.raises(msh.MshError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value
    return str(ei.value)


class Mirror:
    """The table on the device and the state the reference carries for it: every call is compared with the
    reference, every read-back with the carried state."""

    def __init__(self, ctx, msh, O, ps, u, nd, zone, skew, alloc=None, used=None, cap=None, mode=X.LEAST, weight=1,
                 rw=None):
        self.ctx, self.O, self.ps, self.u, self.nd = ctx, O, ps, np.asarray(u, np.uint8), np.asarray(nd, np.int8)
        n = len(u)
        set_plugins(ctx, msh, ps)
        ctx.set_tiebreak("first")
        ctx.upload_nodes(u, nd)  # zeroes the counts, drops the columns and the table
        self.alloc = np.zeros((0, n), np.int64) if alloc is None else np.asarray(alloc, np.int64)
        self.used = np.zeros_like(self.alloc) if used is None else np.array(used, np.int64)
        if alloc is not None:
            ctx.upload_node_resources(self.alloc, self.used)
        self.cap = None if cap is None else np.asarray(cap, np.int64)
        if cap is not None:
            ctx.upload_node_capacity(cap)
        self.skew = np.asarray(skew, np.int32)
        ctx.set_spread_groups(self.skew)
        self.zone = np.asarray(zone, np.int32)
        ctx.upload_node_zones(self.zone)  # zeroes the spread counts
        self.counts = np.zeros(n, np.int32)
        self.cnt = np.zeros((len(self.skew), S.MAX_ZONES), np.int32)
        self.score(mode, weight, rw)

    def score(self, mode, weight=1, rw=None):
        self.mode, self.weight = mode, weight
        self.rw = [1] * self.alloc.shape[0] if rw is None else list(rw)
        if mode == X.NONE:
            self.ctx.set_resource_score("none")
        else:
            self.ctx.set_resource_score(MODE_NAMES[mode], weight, self.rw)

    def eff(self, scalar=0):
        n = len(self.u)
        if self.cap is None:
            return np.full(n, scalar, np.int64) if scalar > 0 else S.no_limit(n)
        return CR.effective(self.cap, scalar)

    def expect(self, pd, pt, grp, req=None, scalar=0, mode=None):
        n, p = len(self.u), len(pd)
        mode = self.mode if mode is None else mode
        ref = X.serial if n * p <= 2 * 10**4 else X.per_pod
        if req is None:
            a, us, rq = S.no_res(n, p)
        else:
            a, us, rq = self.alloc, self.used, np.asarray(req, np.int64)
        return ref(self.O, self.u, self.nd, pd, pt, self.ps, self.eff(scalar), a, us, rq, self.zone, grp, self.skew,
                   mode, self.weight, self.rw, self.counts, self.cnt)

    def commit(self, want, with_req=True):
        self.counts, self.cnt = want[3], want[5]
        if with_req:
            self.used = want[4]

    def compare(self, got, want, what):
        for g, w, name in zip(got, want[:3], ("idx", "score", "status")):
            g = np.asarray(g)
            assert np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(g != np.asarray(w))[:5]}"

    def scored(self, pd, pt, grp, req=None, scalar=0, what=""):
        got = self.ctx.schedule_sequential_spread_scored(pd, pt, grp, req, scalar)
        want = self.expect(pd, pt, grp, req, scalar)
        self.compare(got, want, what)
        self.commit(want, req is not None)
        self.verify(what)
        return want

    def verify(self, what=""):
        assert np.array_equal(self.ctx.node_pod_counts(), self.counts), f"{what}: counts"
        if self.alloc.shape[0]:
            a, b = self.ctx.node_resources()
            assert np.array_equal(a, self.alloc), f"{what}: alloc moved"
            assert np.array_equal(b, self.used), f"{what}: used differs at {np.argwhere(b != self.used)[:5].tolist()}"
        got = self.ctx.spread_counts()
        assert np.array_equal(got, self.cnt), f"{what}: spread counts differ at {np.argwhere(got != self.cnt)[:5].tolist()}"


def limit(ctx, nres, mode=X.LEAST):
    ctx.set_resource_score(MODE_NAMES[mode], 1, [1] * nres)
    return ctx.seq_spread_scored_max_nodes(nres)


@pytest.mark.parametrize("mode", [X.LEAST, X.MOST])
@pytest.mark.parametrize("nres", [1, 2, 3, 4])
def test_instance_thresholds(msh, oracle, ctx, nres, mode):
    """n = 1, at each wave threshold, one on either side of it and the limit; one node past the limit is refused."""
    rng = np.random.default_rng(100 * mode + nres)
    lim = limit(ctx, nres, mode)
    assert lim % 1024 == 0 and lim <= 4096
    ps = oracle.PluginSet(weights=[3], normalize=[nres % 4])
    for n in (1, lim // 16 - 1, lim // 16, lim // 16 + 1, lim // 4, lim // 4 + 1, lim):
        p = int(rng.integers(300, 420)) | 1
        u, nd, pd, pt = rand_case(rng, n, p)
        zone = rng.integers(-1, 8, n)
        grp = rng.integers(-1, 16, p)
        alloc, used, req = rand_amounts(rng, nres, n, p, int(rng.choice([1, 2**33])))
        m = Mirror(ctx, msh, oracle, ps, u, nd, zone, rng.choice([1, 2, 3], 16), alloc, used, rng.integers(0, 4, n), mode,
                   int(rng.choice([1, 7])), rng.integers(1, 101, nres))
        want = m.scored(pd, pt, grp, req, what=f"nres={nres} n={n} p={p}")
        if n > 300:
            assert want[0].max() >= n - n // 8  # the pods reached the last wave
    n = lim + 1
    m = Mirror(ctx, msh, oracle, ps, np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros(n, np.int32), [1],
               np.ones((nres, n), np.int64), mode=mode)
    msg = refused(msh, msh._native.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_spread_scored, np.zeros(3, np.int8),
                  np.zeros(3, np.uint8), np.zeros(3, np.int32), np.ones((nres, 3), np.int64))
    assert f"{lim} nodes" in msg
    m.verify("past the limit")


@pytest.mark.parametrize("waves", [4, 16])
@pytest.mark.parametrize("pattern", ["every pod", "two groups", "with ungrouped"])
def test_consecutive_pods_of_one_group(msh, oracle, ctx, waves, pattern):
    """The hazard of the one-barrier frame: pod j's commit to cnt and pod j + 1's read of the same row. Two zones
    at max_skew = 1, so every commit flips the allowed mask; zone A's open nodes lie in wave 0 and zone B's in the
    last wave, so the winning node and the committing thread alternate between the two ends of the workgroup."""
    rng = np.random.default_rng(waves)
    lim = limit(ctx, 2)
    n = lim // 4 if waves == 4 else lim  # the largest table of each instance: its last nodes lie in its last wave
    p = 400
    u = np.ones(n, np.uint8)
    u[:6] = 0
    u[-6:] = 0
    zone = np.where(np.arange(n) < n // 2, 5, 40)
    nd = rng.integers(0, 3, n).astype(np.int8)
    pd = rng.integers(0, 3, p).astype(np.int8)
    pt = np.zeros(p, np.uint8)
    grp = {"every pod": np.zeros(p, np.int32), "two groups": np.arange(p) % 2,
           "with ungrouped": -(np.arange(p) % 2)}[pattern]
    alloc = rng.integers(5000, 9000, (2, n)).astype(np.int64)
    req = rng.integers(0, 9, (2, p)).astype(np.int64)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 1], alloc, cap=np.full(n, 80), mode=X.LEAST)
    want = m.scored(pd, pt, grp, req, what=f"{waves} waves, {pattern}")
    placed = want[0][want[2] == S.PLACED]
    assert (placed < 6).any() and (placed >= n - 6).any()
    # after 2k commits group 0 stands at (k, k): commits 2k and 2k + 1 go to different zones
    sel = (grp == 0) & (want[2] == S.PLACED)
    g0 = (want[0][sel] >= n // 2)[: 2 * (sel.sum() // 2)]
    assert len(g0) >= 100 and (g0[0::2] != g0[1::2]).all()


def test_the_score_decides_within_the_allowed_zones(msh, oracle, ctx):
    """Equal NodeNumber totals, LEAST picks the emptiest allowed node; ties at the maximum on either side of the
    boundary between wave 0 and wave 1 of the 4-wave instance go to the first node in List order."""
    lim = limit(ctx, 1)
    n, wave = lim // 4 - 8, lim // 16  # nodes per wave
    zone = np.arange(n) % 3
    b = wave - wave % 3  # a multiple of 3 just below the boundary: zone(b + k) = k % 3
    low = {b - 1: 2, b: 0, b + 1: 1, b + 4: 1, b + 45: 0}  # node: its zone; the boundary lies inside b .. b + 4
    assert all(zone[i] == z for i, z in low.items()) and b - 1 < wave <= b + 4
    used = np.full((1, n), 500, np.int64)
    used[0, list(low)] = 100
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), np.zeros(n, np.uint8), np.zeros(n, np.int8), zone, [1],
               np.full((1, n), 1000, np.int64), used, mode=X.LEAST)
    ctx.patch_spread_counts([0], [0], [1])  # zone 0 leads by one: barred for the first two pods
    m.cnt[0, 0] = 1
    p = 5
    want = m.scored(np.zeros(p, np.int8), np.zeros(p, np.uint8), np.zeros(p, np.int32), np.full((1, p), 10, np.int64),
                    what="ties across the wave boundary")
    # zones 1, 2 allowed: b - 1, b + 1 and b + 4 tie at 89, the first wins; then zone 1 alone: b + 1 before b + 4;
    # then every zone: b and b + 45 tie with b + 4, b is first
    assert want[0].tolist()[:3] == [b - 1, b + 1, b] and want[1].tolist()[:3] == [10 + 89] * 3


@pytest.mark.parametrize("mode", [X.LEAST, X.MOST])
def test_the_skew_bars_the_arg_max(msh, oracle, ctx, mode):
    """The hand-worked case of tests/test_spread_score.py (LEAST), and a random table on which the best-scored
    node's zone is often over skew; with every zone barred or full the pod is a FIT_ERROR and commits nothing."""
    if mode == X.LEAST:
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(score=[], weights=[], normalize=[]), np.zeros(3, np.uint8),
                   np.zeros(3, np.int8), [0, 0, 1], [1], np.array([[100, 100, 10]]), mode=X.LEAST)
        want = m.scored(np.zeros(6, np.int8), np.zeros(6, np.uint8), np.zeros(6, np.int32), np.full((1, 6), 5, np.int64),
                        what="hand-worked")
        assert want[0].tolist() == [0, 2, 1, 2, 0, -1] and want[1].tolist() == [95, 50, 95, 0, 90, 0]
        assert want[2].tolist() == [0, 0, 0, 0, 0, S.FIT_ERROR]
    rng = np.random.default_rng(60 + mode)
    n, p = 333, 501
    u, nd, pd, pt = rand_case(rng, n, p, digits=1, p_unsched=0.0)
    zone = rng.choice([2, 9, 33], n, p=[0.7, 0.2, 0.1])
    alloc, used, req = rand_amounts(rng, 2, n, p)
    cap = rng.integers(0, 3, n)
    cap[zone == 33] = rng.random((zone == 33).sum()) < 0.2  # the small zone fills: then the minimum pins
    grp = rng.integers(0, 2, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 2], alloc, used, cap, mode)
    fit = m.expect(pd, pt, np.full(p, -1), req)  # the scored _fit placements of the same pods
    want = m.scored(pd, pt, grp, req, what="random")
    moved = (want[0] != fit[0]) & (want[2] == S.PLACED)
    assert moved.sum() >= 10 and ((want[2] == S.FIT_ERROR) & (fit[2] == S.PLACED)).sum() >= 10


@pytest.mark.parametrize("mode", [X.LEAST, X.MOST])
def test_quotients_on_their_boundaries_with_a_grouped_pod(msh, oracle, ctx, mode):
    """For divisors 1, 3, 2^32 + 1 and 2^55 and every k: a node whose numerator is the smallest with
    num * 100 / c == k and one below it; one pod per node, every pod grouped, so each quotient decides a placement
    among the zones the skew allows."""
    alloc, used = [], []
    for c in (1, 3, 2**32 + 1, 2**55):
        for k in (0, 1, 33, 50, 67, 99, 100):
            for num in {-(-k * c // 100), max(-(-k * c // 100) - 1, 0)}:  # ceil(k c / 100) and one below
                free = num if mode == X.LEAST else c - num
                alloc.append(c)
                used.append(c - free)
    n = len(alloc)
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    alloc, used = np.array(alloc, np.int64)[perm].reshape(1, n), np.array(used, np.int64)[perm].reshape(1, n)
    zone = rng.integers(0, 3, n)
    u, nd = np.zeros(n, np.uint8), np.zeros(n, np.int8)
    pd, pt, grp = np.zeros(n, np.int8), np.zeros(n, np.uint8), np.zeros(n, np.int32)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [2], alloc, used, mode=mode)
    want = m.scored(pd, pt, grp, np.zeros((1, n), np.int64), scalar=1, what="zero requests")
    assert (want[2] == S.PLACED).sum() > n // 2 and len(set(want[1].tolist())) > 8
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [2], alloc, np.maximum(used - 1, 0), mode=mode)
    m.scored(pd, pt, grp, np.ones((1, n), np.int64), scalar=1, what="unit requests")


def test_q_above_c_after_a_patch_lowered_alloc(msh, oracle, ctx):
    """A zero request on a node whose alloc a patch lowered below used scores 0 and is not rejected."""
    for mode, idx, score in ((X.LEAST, [1, 0], [100, 0]), (X.MOST, [0, 1], [0, 0])):
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(score=[], weights=[], normalize=[]), np.zeros(2, np.uint8),
                   np.zeros(2, np.int8), [0, 1], [1], np.array([[100, 100]]), np.array([[50, 0]]), mode=mode)
        ctx.patch_node_resources([0], alloc=np.array([[20]]))
        m.alloc = np.array([[20, 100]], np.int64)
        want = m.scored(np.zeros(2, np.int8), np.zeros(2, np.uint8), np.zeros(2, np.int32), np.zeros((1, 2), np.int64),
                        what=f"q > c, mode {mode}")
        assert want[0].tolist() == idx and want[1].tolist() == score and not want[2].any()


@pytest.mark.parametrize("rw", [[1, 0], [0, 5], [3, 1], [100, 1, 0, 7]])
def test_resource_weights(msh, oracle, ctx, rw):
    rng = np.random.default_rng(sum(rw))
    n, p = 150, 333
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, len(rw), n, p)
    if 0 in rw:
        alloc[rw.index(0)] //= 20  # the unscored resource is scarce: it is fitted, so it decides feasibility
    grp = rng.integers(-1, 2, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, rng.integers(-1, 4, n), [1, 2], alloc, used, mode=X.LEAST,
               weight=2, rw=rw)
    m.rw = [1] * len(rw)
    even = m.expect(pd, pt, grp, req)  # the same call with every resource at weight 1
    m.rw = rw
    want = m.scored(pd, pt, grp, req, what=f"rw={rw}")
    assert not np.array_equal(want[0], even[0]) and (want[2] == S.PLACED).any()
    if 0 in rw:
        assert (want[2] == S.FIT_ERROR).any()


def test_normalize_modes_and_a_large_plugin_weight(msh, oracle, ctx):
    rng = np.random.default_rng(9)
    n = 140
    lists = [oracle.PluginSet(weights=[w], normalize=[nm]) for nm in (0, 1, 2, 3) for w in (1, 2**32)]
    lists += [oracle.PluginSet(score=[], weights=[], normalize=[]),                   # the resource score alone
              oracle.PluginSet(prescore=[], score=[], weights=[], normalize=[]),
              oracle.PluginSet(prescore=[]), oracle.PluginSet(filters=[])]            # score errors; no filter
    for k, ps in enumerate(lists):
        u, nd, _, _ = rand_case(rng, n, 0)
        alloc, used, _ = rand_amounts(rng, 2, n, 0)
        m = Mirror(ctx, msh, oracle, ps, u, nd, rng.integers(-1, 4, n), [1, 2], alloc, used, rng.integers(0, 4, n),
                   X.LEAST if k % 2 else X.MOST, weight=2**32 if k % 3 == 0 else 3)
        for p in (0, 1, 63, 65, 129):
            _, _, pd, pt = rand_case(rng, 1, p)
            pd[rng.random(p) < 0.1] = -1
            m.scored(pd, pt, rng.integers(-1, 2, p), rand_amounts(rng, 2, 1, p)[2], what=f"list {k} p={p}")


def test_nodes_without_a_zone(msh, oracle, ctx):
    """Allowed for ungrouped pods, never for grouped ones, however well they score."""
    rng = np.random.default_rng(21)
    n, p = 200, 301
    u, nd, pd, pt = rand_case(rng, n, p, digits=1, p_unsched=0.0)
    zone = rng.integers(0, 3, n)
    zone[::4] = -1
    alloc, used, req = rand_amounts(rng, 1, n, p)
    used[0, ::4] = 0
    alloc[0, ::4] = 10**6  # the unzoned nodes are by far the emptiest: LEAST wants them
    grp = rng.integers(-1, 2, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [2, 3], alloc, used, mode=X.LEAST)
    want = m.scored(pd, pt, grp, req, what="unzoned nodes")
    placed = want[2] == S.PLACED
    assert (zone[want[0][placed & (grp >= 0)]] >= 0).all() and (zone[want[0][placed & (grp < 0)]] < 0).all()
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, np.full(n, -1), [2, 3], alloc, used, mode=X.LEAST)
    want = m.scored(pd, pt, grp, req, what="no zone anywhere")
    assert (want[2][grp >= 0] == S.FIT_ERROR).all() and (want[2][grp < 0] == S.PLACED).all()


@pytest.mark.parametrize("G", [1, 128])
def test_group_range_and_zone_63(msh, oracle, ctx, G):
    rng = np.random.default_rng(G)
    n, p = 200, 401
    u, nd, pd, pt = rand_case(rng, n, p)
    zone = rng.choice([0, 31, 63], n)
    skew = rng.choice([1, I32MAX], G).astype(np.int64)
    skew[0], skew[-1] = 1, (2 if G > 1 else 1)
    grp = rng.choice([0, G - 1, int(rng.integers(0, G))], p)  # both ends of the group range
    alloc, used, req = rand_amounts(rng, 2, n, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, skew, alloc, used, rng.integers(0, 6, n), X.MOST)
    m.scored(pd, pt, grp, req, what=f"G={G}")
    assert m.cnt[0, 63] > 0 and m.cnt[G - 1, 63] > 0


def device_call(torch, ctx, pd, pt, grp, req, stream, fn=None):
    dev = torch.device("cuda:0")
    h = len(pd)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pd, pt, grp)]
    rq = None if req is None else torch.from_numpy(np.ascontiguousarray(req)).to(dev)
    outs = (torch.full((h,), -7, dtype=torch.int32, device=dev), torch.full((h,), -7, dtype=torch.int64, device=dev),
            torch.full((h,), -7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    (fn or ctx.schedule_sequential_spread_scored_device)(
        h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0 if req is None else req.shape[0],
        0 if rq is None else rq.data_ptr(), 0, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
        stream.cuda_stream)
    return outs, (t, rq)


def test_device_form_treats_groups_out_of_range_as_ungrouped(msh, oracle, ctx):
    """Ordinary input of the unvalidated device form: -7, G and 2^30 are ungrouped pods."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(41)
    n, p, G = 300, 333, 3
    u, nd, pd, pt = rand_case(rng, n, p)
    grp = rng.choice([-7, -1, 0, 1, 2, G, 2**30, -2**31], p).astype(np.int32)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, rng.integers(-1, 3, n), [1, 1, 2], alloc, used,
               rng.integers(0, 4, n), X.LEAST)
    want = m.expect(pd, pt, grp, req)
    clean = m.expect(pd, pt, np.where((grp >= 0) & (grp < G), grp, -1), req)
    assert all(np.array_equal(a, b) for a, b in zip(want, clean))
    st = torch.cuda.Stream(torch.device("cuda:0"))
    outs, _keep = device_call(torch, ctx, pd, pt, grp, req, st)
    st.synchronize()
    m.compare([o.cpu().numpy() for o in outs], want, "out-of-range groups")
    m.commit(want)
    m.verify("out-of-range groups")


def test_device_form_on_two_streams(msh, oracle, ctx):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(31)
    n, p, h = 600, 302, 151
    u, nd, pd, pt = rand_case(rng, n, p)
    grp = rng.integers(-1, 2, p).astype(np.int32)
    alloc, used, req = rand_amounts(rng, 3, n, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[3], normalize=[1]), u, nd, rng.integers(-1, 3, n), [1, 1],
               alloc, used, rng.integers(0, 3, n), X.MOST)
    want = m.expect(pd, pt, grp, req)
    streams = [torch.cuda.Stream(torch.device("cuda:0")) for _ in range(2)]
    runs = [device_call(torch, ctx, pd[k * h:(k + 1) * h], pt[k * h:(k + 1) * h], grp[k * h:(k + 1) * h],
                        req[:, k * h:(k + 1) * h], st) for k, st in enumerate(streams)]  # ordered by the library
    for st in streams:
        st.synchronize()
    m.compare([np.concatenate([runs[k][0][q].cpu().numpy() for k in range(2)]) for q in range(3)], want, "two streams")
    m.commit(want)
    m.verify("two streams")


def test_composition_with_the_capacity_column_and_the_scalar(msh, oracle, ctx):
    rng = np.random.default_rng(50)
    n, p = 90, 301
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    zone = rng.integers(0, 3, n)
    grp = rng.integers(-1, 2, p)
    alloc, used, req = rand_amounts(rng, 2, n, p, 2**40 + 1)
    cap = rng.integers(0, 5, n)
    for scalar, col in ((0, cap), (2, cap), (3, None)):
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[3], normalize=[2]), u, nd, zone, [1, 2], alloc, used, col,
                   X.LEAST)
        m.scored(pd, pt, grp, req, scalar=scalar, what=f"scalar {scalar}, column {col is not None}")
        assert (m.counts <= m.eff(scalar)).all() and (col is not None or m.counts.max() == 3)


def test_carried_state_across_calls_and_writers(msh, oracle, ctx):
    rng = np.random.default_rng(77)
    n, p = 120, 480
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    zone = rng.integers(-1, 4, n)
    grp = rng.integers(-1, 3, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 2, 1], alloc, used, rng.integers(2, 9, n), X.LEAST)
    sl = lambda a, b: (pd[a:b], pt[a:b], grp[a:b], req[:, a:b])  # noqa: E731
    m.scored(*sl(0, 70), what="first call")
    m.scored(*sl(70, 130), what="second call, carried state")
    # a scored _fit call in between commits counts and used, never cnt
    a, b, _, c = sl(130, 190)
    w = m.expect(a, b, np.full(60, -1), c)
    m.compare(ctx.schedule_sequential_fit(a, b, c), w, "_fit")
    m.commit(w)
    m.verify("after the scored _fit")
    m.scored(*sl(190, 250), what="after _fit")
    # a patch of the spread counts: a deleted pod, and pods bound elsewhere
    busy = np.argwhere(m.cnt > 0)[:2]
    gi, zi = np.append(busy[:, 0], 2), np.append(busy[:, 1], 63)
    val = np.array([m.cnt[busy[0, 0], busy[0, 1]] - 1, 0, 7])
    ctx.patch_spread_counts(gi, zi, val)
    m.cnt[gi, zi] = val
    m.scored(*sl(250, 310), what="after the count patch")
    # a patch of the table: more room on some nodes, pods deleted from others
    idx = np.arange(0, n, 9, dtype=np.int32)
    m.alloc, m.used = m.alloc.copy(), m.used.copy()
    m.alloc[:, idx] += 50
    m.used[:, idx[::2]] = 0
    ctx.patch_node_resources(idx, alloc=m.alloc[:, idx], used=m.used[:, idx])
    m.scored(*sl(310, 370), what="after the resource patch")
    m.score(X.MOST, 5, [2, 1])  # the setting changes, the state stays
    m.scored(*sl(370, 420), what="MOST")
    ctx.reset_node_pod_counts()
    m.counts[:] = 0
    m.scored(*sl(420, 450), what="after the pod count reset")
    ctx.reset_spread_counts()
    m.cnt[:] = 0
    m.verify("spread count reset")
    m.scored(*sl(450, 480), what="after the spread count reset")


@pytest.mark.parametrize("nres", [0, 2])
def test_mode_none_is_the_spread_call(msh, oracle, ctx, nres):
    """Outputs and state equal msh_schedule_sequential_spread's on the same inputs, nres = 0 included, and the
    limit is that call's."""
    rng = np.random.default_rng(90 + nres)
    n, p = 700, 333
    u, nd, pd, pt = rand_case(rng, n, p)
    zone = rng.integers(-1, 4, n)
    grp = rng.integers(-1, 3, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    cap = rng.integers(0, 3, n)
    got = []
    for call in ("schedule_sequential_spread", "schedule_sequential_spread_scored"):
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 2, 1], alloc, used, cap, X.NONE)
        assert ctx.seq_spread_scored_max_nodes(nres) == ctx.seq_spread_max_nodes(nres)
        out = getattr(ctx, call)(pd, pt, grp, req if nres else None)
        got.append((*out, ctx.node_pod_counts(), ctx.node_resources()[1], ctx.spread_counts()))
    assert all(np.array_equal(a, b) for a, b in zip(*got))
    want = m.expect(pd, pt, grp, req if nres else None)
    m.compare(got[1], want, "mode NONE")
    m.commit(want, bool(nres))
    m.verify("mode NONE")


def test_refusals_change_nothing(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(3)
    n, p = 50, 40
    u, nd, pd, pt = rand_case(rng, n, p)
    zone = rng.integers(-1, 3, n)
    grp = rng.integers(-1, 2, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    ps = oracle.PluginSet()
    m = Mirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2], alloc, used, mode=X.LEAST)
    m.scored(pd, pt, grp, req, what="before the refusals")
    call = ctx.schedule_sequential_spread_scored
    assert "resource score" in refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_spread, pd, pt, grp, req)
    m.verify("the old entry point still refuses a scored ctx")
    # the call's argument errors (host form)
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, np.where(np.arange(p) == 5, 2, grp), req)       # a group == G
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, np.where(np.arange(p) == 5, -2, grp), req)      # a group below -1
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, grp, req[:1])                                   # nres != the table's
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, grp, -req - 1)
    assert "2^55" in refused(msh, E.MSH_ERR_INVALID, call, pd, pt, grp, np.full_like(req, 2**55 + 1))
    refused(msh, E.MSH_ERR_INVALID, call, pd, pt, grp, req, -1)
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, None)                                        # nres = 0 with a score set
    ctx.set_resource_score("least", 1, [1, 1, 1])                                                 # nres != the setting's
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, req)
    m.score(X.LEAST)
    m.verify("argument errors")
    # unsupported combinations, each naming its reason
    ctx.set_tiebreak("random", 11, 5)
    assert "MSH_TIEBREAK_RANDOM" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, req)
    ctx.set_tiebreak("first")
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig("NodeNumber"), msh.ScorePluginConfig("ScoreColumn0")])
    assert "score-column" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, req)
    set_plugins(ctx, msh, ps)
    m.verify("RANDOM and score columns")
    # the 2^55 bound on the table, tripped by a patch; an upload within the limit resets it
    ctx.patch_node_resources([3], alloc=np.full((2, 1), 2**55 + 1, np.int64))
    assert "2^55" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, req)
    ctx.upload_node_resources(m.alloc, m.used)
    m.verify("the table bound")
    m.scored(pd, pt, grp, req, what="between the refusals")
    # state errors: no resource table, no zone column, no nodes
    ctx.clear_node_resources()
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, req)
    ctx.upload_node_resources(m.alloc, m.used)
    ctx.clear_node_zones()
    refused(msh, E.MSH_ERR_STATE, call, pd, pt, grp, req)
    assert np.array_equal(ctx.spread_counts(), m.cnt) and np.array_equal(ctx.node_pod_counts(), m.counts)
    assert np.array_equal(ctx.node_resources()[1], m.used)
    with msh.DeviceContext(0) as fresh:
        fresh.set_resource_score("least", 1, [1, 1])
        refused(msh, E.MSH_ERR_STATE, fresh.schedule_sequential_spread_scored, pd, pt, grp, req)  # no nodes
        refused(msh, E.MSH_ERR_INVALID, fresh.seq_spread_scored_max_nodes, 5)


def test_seeded_sweep(msh, oracle, ctx):
    """40 cases from the shared generator (tests/test_spread_score.py asserts that they are not trivial)."""
    for seed in SWEEP_SEEDS:
        c = X.gen_case(seed)
        cols, _, res, sp = case_args(c)
        m = Mirror(ctx, msh, oracle, case_plugins(oracle, c), cols[0], cols[1], sp[0], sp[2], res[0], None, c["cap"],
                   c["score_mode"], c["rs_weight"], c["rw"])
        m.scored(cols[2], cols[3], sp[1], res[2], what=f"seed {seed}")


def test_scheduler_with_a_resource_score_and_spread_groups(msh, oracle):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    rng = np.random.default_rng(12)
    n, p = 14, 60
    zkey = "topology.kubernetes.io/zone"
    zl = [None if i % 6 == 5 else "abc"[i % 3] for i in range(n)]
    cpus = rng.integers(1, 5, n)
    nodes = [{"metadata": {"name": f"node{i}", "labels": ({zkey: zl[i]} if zl[i] else {})},
              "spec": {"unschedulable": bool(i % 5 == 0)}, "status": {"allocatable": {"cpu": str(cpus[i])}}} for i in range(n)]
    apps = [("web", "db", None, "other")[j % 4] for j in range(p)]
    rc = rng.integers(0, 3, p)
    pods = [{"metadata": {"name": f"pod{j}", "labels": ({"app": apps[j]} if apps[j] else {})},
             "spec": {"containers": [{"resources": {"requests": {"cpu": f"{rc[j] * 500}m"}}}], "tolerations": []}} for j in range(p)]
    s = msh.Scheduler(resources=("cpu",), resource_score="least", zones=zkey, spread_groups={"web": 1, "db": 2})
    try:
        res = s.schedule_sequential(pods, nodes)
        nt = s.nodes
        pos = {nm: k for k, nm in enumerate(nt.names)}
        names: dict = {}
        zone = np.full(n, -1, np.int32)
        alloc = np.zeros((1, n), np.int64)
        for k, nm in enumerate(nt.names):  # zone ids in the order List order first shows them
            i = int(nm[4:])
            if zl[i]:
                zone[k] = names.setdefault(zl[i], len(names))
        for i in range(n):
            alloc[0, pos[f"node{i}"]] = cpus[i] * 1000
        grp = np.array([{"web": 0, "db": 1}.get(a, -1) for a in apps], np.int32)
        pdig = np.array([int(f"pod{j}"[-1]) for j in range(p)], np.int8)
        args = (oracle, nt.unsched, nt.digit, pdig, np.zeros(p, np.uint8), oracle.PluginSet(), S.no_limit(n), alloc,
                np.zeros_like(alloc), np.array([rc * 500], np.int64), zone, grp, [1, 2])
        want = X.serial(*args, X.LEAST, 1, [1])
        assert [int(r.outcome) for r in res] == want[2].tolist()
        assert [r.node_index for r in res] == want[0].tolist() and [r.score for r in res] == want[1].tolist()
        assert (want[2] == S.FIT_ERROR).any() and (want[2] == S.PLACED).any()
        assert not np.array_equal(want[0], S.serial(*args)[0])  # the score moved placements
        assert np.array_equal(s.ctx.spread_counts(), want[5]) and np.array_equal(s.ctx.node_pod_counts(), want[3])
        assert np.array_equal(s.ctx.node_resources()[1], want[4]) and np.array_equal(s.ctx.node_zones(), zone)
    finally:
        s.close()
