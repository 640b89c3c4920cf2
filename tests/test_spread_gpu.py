"""Pod topology spread in sequential-commit mode on the GPU (msh_schedule_sequential_spread and friends).

Every comparison is bit-exact on idx, score, status, node_pod_counts(), the `used` half of node_resources() and
spread_counts(). The expected values come from tests/spread_ref.py: the plain serial loop for tiny shapes, the
numpy per-pod loop otherwise (tests/test_spread.py shows on the CPU that the two agree, and that the sweep's
generator makes the spread conjunct decide).

The kernel (csrc/msh_seq_spread.hip) holds NPL nodes per thread on 1, 4 or 16 waves; the limit is read from
msh_seq_spread_max_nodes (1,024 x NPL), never hard-coded."""
from __future__ import annotations

import numpy as np
import pytest

import node_capacity_ref as CR
import spread_ref as S
from test_spread import SWEEP_SEEDS, sweep_inputs

pytestmark = pytest.mark.gpu
I32MAX = S.INT32_MAX


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


def rand_case(rng, n, p, p_unsched=0.3):
    u = (rng.random(n) < p_unsched).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, 10, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return u, nd, pd, pt


class Mirror:
    """The table on the device and the state the reference carries for it: every call is compared with the
    reference, every read-back with the carried state."""

    def __init__(self, ctx, msh, O, ps, u, nd, zone, skew, alloc=None, cap=None):
        self.ctx, self.O, self.ps, self.u, self.nd = ctx, O, ps, np.asarray(u, np.uint8), np.asarray(nd, np.int8)
        n = len(u)
        set_plugins(ctx, msh, ps)
        ctx.set_tiebreak("first")
        ctx.set_resource_score("none")
        ctx.upload_nodes(u, nd)  # zeroes the counts, drops the columns and the table
        self.alloc = np.zeros((0, n), np.int64) if alloc is None else np.asarray(alloc, np.int64)
        if alloc is not None:
            ctx.upload_node_resources(self.alloc)
        self.cap = None if cap is None else np.asarray(cap, np.int64)
        if cap is not None:
            ctx.upload_node_capacity(cap)
        self.skew = np.asarray(skew, np.int32)
        ctx.set_spread_groups(self.skew)
        self.zone = np.asarray(zone, np.int32)
        ctx.upload_node_zones(self.zone)  # zeroes the spread counts
        self.counts = np.zeros(n, np.int32)
        self.used = np.zeros_like(self.alloc)
        self.cnt = np.zeros((len(self.skew), S.MAX_ZONES), np.int32)

    def eff(self, scalar=0):
        n = len(self.u)
        if self.cap is None:
            return np.full(n, scalar, np.int64) if scalar > 0 else S.no_limit(n)
        return CR.effective(self.cap, scalar)

    def expect(self, pd, pt, grp, req=None, scalar=0):
        n, p = len(self.u), len(pd)
        ref = S.serial if n * p <= 2 * 10**4 else S.per_pod
        if req is None:
            a, us, rq = S.no_res(n, p)
        else:
            a, us, rq = self.alloc, self.used, np.asarray(req, np.int64)
        want = ref(self.O, self.u, self.nd, pd, pt, self.ps, self.eff(scalar), a, us, rq, self.zone, grp, self.skew,
                   self.counts, self.cnt)
        return want

    def commit(self, want, with_req):
        self.counts, self.cnt = want[3], want[5]
        if with_req:
            self.used = want[4]

    def spread(self, pd, pt, grp, req=None, scalar=0, what=""):
        got = self.ctx.schedule_sequential_spread(pd, pt, grp, req, scalar)
        want = self.expect(pd, pt, grp, req, scalar)
        for g, w, name in zip(got, want[:3], ("idx", "score", "status")):
            assert np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(np.asarray(g) != np.asarray(w))[:5]}"
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


def scarce_cap(rng, n, p):
    """Pod capacities that keep the early nodes scarce, so that p pods reach every wave of the table."""
    cap = rng.integers(0, 4, n)
    if n > 300:
        cap[: n - 40] = rng.random(n - 40) < min(1.0, 0.8 * p / n)
    return cap


@pytest.mark.parametrize("nres", [0, 1, 2, 3, 4])
def test_instance_boundaries(msh, oracle, ctx, nres):
    """n at each wave threshold, one past it and the limit, per instance; one node past the limit is refused."""
    rng = np.random.default_rng(200 + nres)
    lim = ctx.seq_spread_max_nodes(nres)
    npl = lim // 1024
    ps = oracle.PluginSet(weights=[3], normalize=[nres % 4])
    for n in (64 * npl, 64 * npl + 1, 256 * npl, 256 * npl + 1, lim):
        p = int(rng.integers(300, 701))
        u, nd, pd, pt = rand_case(rng, n, p)
        zone = rng.integers(-1, 8, n)
        grp = rng.integers(-1, 16, p)
        alloc = (rng.integers(0, 9, (nres, n)) * int(rng.choice([1, 2**33]))).astype(np.int64) if nres else None
        req = None if not nres else (rng.integers(0, 3, (nres, p)) * (alloc.max() // 8)).astype(np.int64)
        m = Mirror(ctx, msh, oracle, ps, u, nd, zone, rng.choice([1, 2, 3], 16), alloc, scarce_cap(rng, n, p))
        want = m.spread(pd, pt, grp, req, what=f"nres={nres} n={n} p={p}")
        if n > 300:
            assert want[0].max() >= n - 40  # the pods reached the last wave
    n = lim + 1
    m = Mirror(ctx, msh, oracle, ps, np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros(n, np.int32), [1],
               np.ones((nres, n), np.int64) if nres else None)
    with pytest.raises(msh.MshError) as ei:
        ctx.schedule_sequential_spread(np.zeros(3, np.int8), np.zeros(3, np.uint8), np.zeros(3, np.int32),
                                       np.ones((nres, 3), np.int64) if nres else None)
    assert ei.value.code == msh._native.MSH_ERR_UNSUPPORTED and f"{lim} nodes" in str(ei.value)
    m.verify("past the limit")


@pytest.mark.parametrize("waves", [4, 16])
@pytest.mark.parametrize("pattern", ["every pod", "two groups", "with ungrouped"])
def test_consecutive_pods_of_one_group(msh, oracle, ctx, waves, pattern):
    """The hazard of the one-barrier frame: pod j's commit to cnt and pod j + 1's read of the same row. Two zones
    at max_skew = 1, so every commit flips the allowed mask; zone A's open nodes lie in wave 0 and zone B's in the
    last wave, so the winning node and the committing thread alternate between the two ends of the workgroup."""
    rng = np.random.default_rng(waves)
    npl = ctx.seq_spread_max_nodes(0) // 1024
    n = 256 * npl if waves == 4 else 1024 * npl  # the largest table of each instance: its last nodes lie in its last wave
    assert n <= ctx.seq_spread_max_nodes(0)
    p = 400
    u = np.ones(n, np.uint8)
    u[:6] = 0
    u[-6:] = 0
    zone = np.where(np.arange(n) < n // 2, 5, 40)
    nd = rng.integers(0, 10, n).astype(np.int8)
    pd = rng.integers(0, 10, p).astype(np.int8)
    pt = np.zeros(p, np.uint8)
    grp = {"every pod": np.zeros(p, np.int32), "two groups": np.arange(p) % 2,
           "with ungrouped": -(np.arange(p) % 2)}[pattern]
    cap = np.full(n, 80)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 1], cap=cap)
    want = m.spread(pd, pt, grp, what=f"{waves} waves, {pattern}")
    placed = want[0][want[2] == S.PLACED]
    assert (placed < 6).any() and (placed >= n - 6).any()
    # after 2k commits group 0 stands at (k, k): commits 2k and 2k + 1 go to different zones
    g0 = (want[0][(grp == 0) & (want[2] == S.PLACED)] >= n // 2)[: 2 * (((grp == 0) & (want[2] == S.PLACED)).sum() // 2)]
    assert len(g0) >= 100 and (g0[0::2] != g0[1::2]).all()


@pytest.mark.parametrize("kind", ["one zone", "all 64", "sparse", "no zone anywhere", "a cordoned zone", "a full zone"])
def test_zones(msh, oracle, ctx, kind):
    rng = np.random.default_rng(len(kind))
    n, p = 330, 300
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    cap = rng.integers(0, 5, n)
    if kind == "one zone":
        zone = np.full(n, 17)
    elif kind == "all 64":
        zone = np.arange(n) % 64
    elif kind == "sparse":
        zone = rng.choice([0, 31, 32, 63], n)
    elif kind == "no zone anywhere":
        zone = np.full(n, -1)
    else:
        zone = rng.choice([3, 4, 9], n, p=[0.45, 0.45, 0.1])
        if kind == "a cordoned zone":
            u[zone == 9] = 1
            pt[:] = 0
        else:
            cap[zone == 9] = 0
            cap[np.flatnonzero(zone == 9)[:2]] = 1  # the zone takes two pods in all
    grp = rng.integers(-1, 3, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[2], normalize=[1]), u, nd, zone, [1, 2, 1], cap=cap)
    want = m.spread(pd, pt, grp, what=kind)
    st = want[2]
    if kind == "no zone anywhere":
        assert (st[grp >= 0] == S.FIT_ERROR).all() and (st[grp < 0] != S.FIT_ERROR).any()
    if kind in ("a cordoned zone", "a full zone"):  # the minimum pins: later pods of the group find nothing
        last = np.flatnonzero((grp == 0) & (st == S.PLACED)).max()
        assert (st[last + 1:][grp[last + 1:] == 0] == S.FIT_ERROR).all() and (grp[last + 1:] == 0).sum() > 20


@pytest.mark.parametrize("G", [1, 128])
def test_group_range(msh, oracle, ctx, G):
    rng = np.random.default_rng(G)
    n, p = 200, 400
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    zone = rng.integers(0, 3, n)
    skew = rng.choice([1, I32MAX], G).astype(np.int64)
    skew[0], skew[-1] = 1, (I32MAX if G > 1 else 1)
    grp = rng.choice([0, G - 1, int(rng.integers(0, G))], p)  # both ends of the group range
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, skew, cap=rng.integers(0, 6, n))
    m.spread(pd, pt, grp, what=f"G={G}")
    assert m.cnt[0].sum() > 0 and m.cnt[G - 1].sum() > 0
    m.skew[:] = I32MAX  # the same G: only the skews change, the counts stay
    ctx.set_spread_groups(m.skew)
    m.spread(pd, pt, grp, what=f"G={G}, no skew limit")


def test_batch_shapes_modes_and_lists(msh, oracle, ctx):
    rng = np.random.default_rng(9)
    n = 140
    lists = [oracle.PluginSet(weights=[w], normalize=[mode]) for mode in (0, 1, 2, 3) for w in (1, 2**32)]
    lists += [oracle.PluginSet(score=[], weights=[], normalize=[]),                   # NodeNumber out of the score list
              oracle.PluginSet(prescore=[], score=[], weights=[], normalize=[]),      # and out of both
              oracle.PluginSet(prescore=[]), oracle.PluginSet(filters=[])]            # score errors; no filter
    for k, ps in enumerate(lists):
        u, nd, _, _ = rand_case(rng, n, 0)
        zone = rng.integers(-1, 4, n)
        m = Mirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2], cap=rng.integers(0, 4, n))
        for p in (0, 1, 63, 64, 65, 129):
            _, _, pd, pt = rand_case(rng, 1, p)
            m.spread(pd, pt, rng.integers(-1, 2, p), what=f"list {k} p={p}")


def test_composition(msh, oracle, ctx):
    """Requests that decide together with the skew, the capacity column with and without the scalar, and 64-bit
    requests near 2^40."""
    rng = np.random.default_rng(50)
    n, p = 90, 300
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    zone = rng.integers(0, 3, n)
    grp = rng.integers(-1, 2, p)
    for unit in (1000, 2**40 - 1, 2**40 + 1):
        alloc = rng.integers(0, 9, (2, n)).astype(np.int64) * unit
        req = rng.integers(0, 3, (2, p)).astype(np.int64) * unit
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 2], alloc)
        want = m.spread(pd, pt, grp, req, what=f"requests x {unit}")
        free = m.expect(pd, pt, grp, np.zeros_like(req))   # the same call with nothing requested
        m2 = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [I32MAX, I32MAX], alloc)
        loose = m2.expect(pd, pt, grp, req)                # and with no skew limit
        assert not np.array_equal(want[0], free[0]) and not np.array_equal(want[0], loose[0])
    cap = rng.integers(0, 5, n)
    for scalar in (0, 2):
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[3], normalize=[2]), u, nd, zone, [1, 2], cap=cap)
        m.spread(pd, pt, grp, scalar=scalar, what=f"column, scalar {scalar}")
        assert (m.counts <= m.eff(scalar)).all()
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 2])
    m.spread(pd, pt, grp, scalar=3, what="scalar alone")
    assert m.counts.max() == 3


def test_carried_state_and_lifetime(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(77)
    n, p = 120, 480
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    zone = rng.integers(-1, 4, n)
    grp = rng.integers(-1, 3, p)
    alloc = rng.integers(2, 9, (2, n)).astype(np.int64) * 4
    req = rng.integers(0, 3, (2, p)).astype(np.int64)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 2, 1], alloc, cap=rng.integers(2, 9, n))
    assert np.array_equal(ctx.node_zones(), zone) and ctx.spread_groups().tolist() == [1, 2, 1]
    sl = lambda a, b: (pd[a:b], pt[a:b], grp[a:b], req[:, a:b])  # noqa: E731
    m.spread(*sl(0, 60), what="first call")
    m.spread(*sl(60, 120), what="second call, carried state")
    # a _fit call and a plain sequential call in between commit counts (and used), never cnt
    a, b, _, c = sl(120, 180)
    w = S.per_pod(oracle, u, nd, a, b, m.ps, m.eff(), m.alloc, m.used, c, zone, np.full(60, -1), m.skew, m.counts, m.cnt)
    got = ctx.schedule_sequential_fit(a, b, c)
    assert all(np.array_equal(x, y) for x, y in zip(got, w[:3]))
    m.commit(w, True)
    m.verify("after _fit")
    a, b, _, _ = sl(180, 240)
    w = S.per_pod(oracle, u, nd, a, b, m.ps, m.eff(), *S.no_res(n, 60), zone, np.full(60, -1), m.skew, m.counts, m.cnt)
    got = ctx.schedule_sequential(a, b, 0)
    assert all(np.array_equal(x, y) for x, y in zip(got, w[:3]))
    m.commit(w, False)
    m.verify("after the plain call")
    m.spread(*sl(240, 300), what="after the other calls")
    # a patch of the counts: a deleted pod, and pods bound elsewhere
    busy = np.argwhere(m.cnt > 0)[:2]
    gi, zi = np.append(busy[:, 0], 2), np.append(busy[:, 1], 63)
    val = np.array([m.cnt[busy[0, 0], busy[0, 1]] - 1, 0, 7])
    ctx.patch_spread_counts(gi, zi, val)
    m.cnt[gi, zi] = val
    m.verify("after the patch")
    m.spread(*sl(300, 360), what="after the count patch")
    # the same G: the skews change, the counts stay; another G: the counts are zeroed
    m.skew = np.array([3, 1, 2], np.int32)
    ctx.set_spread_groups(m.skew)
    m.verify("same G")
    m.spread(*sl(360, 400), what="new skews")
    m.skew = np.array([1, 2, 1, 4], np.int32)
    ctx.set_spread_groups(m.skew)
    m.cnt = np.zeros((4, S.MAX_ZONES), np.int32)
    m.verify("another G")
    m.spread(*sl(400, 430), what="four groups")
    # patches of the table, a count reset and the other writers keep zones, groups and cnt
    flip = np.arange(0, n, 7, dtype=np.int32)
    m.u = m.u.copy()
    m.u[flip] ^= 1
    ctx.patch_nodes(flip, m.u[flip], nd[flip])
    ctx.reset_node_pod_counts()
    m.counts[:] = 0
    ctx.patch_node_capacity([0, 1], [9, 9])
    m.cap[[0, 1]] = 9
    m.verify("after the other writers")
    m.spread(*sl(430, 450), what="after the other writers")
    ctx.reset_spread_counts()
    m.cnt[:] = 0
    m.verify("count reset")
    # a new zone column zeroes the counts; msh_upload_nodes drops the column and zeroes them
    m.spread(*sl(450, 465), what="before the new column")
    m.zone = np.roll(zone, 3).astype(np.int32)
    ctx.upload_node_zones(m.zone)
    m.cnt[:] = 0
    m.verify("new column")
    m.spread(*sl(465, 480), what="after the new column")
    assert m.cnt.any()
    ctx.upload_nodes(u, nd)
    assert ctx.node_zones() is None and not ctx.spread_counts().any() and len(ctx.spread_groups()) == 4
    with pytest.raises(msh.MshError) as ei:
        ctx.schedule_sequential_spread(pd, pt, grp)
    assert ei.value.code == E.MSH_ERR_STATE
    ctx.upload_node_zones(zone)
    ctx.clear_node_zones()
    assert ctx.node_zones() is None
    with pytest.raises(msh.MshError) as ei:
        ctx.schedule_sequential_spread(pd, pt, grp)
    assert ei.value.code == E.MSH_ERR_STATE


def device_call(torch, ctx, pd, pt, grp, req, stream):
    dev = torch.device("cuda:0")
    h = len(pd)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pd, pt, grp)]
    rq = None if req is None else torch.from_numpy(np.ascontiguousarray(req)).to(dev)
    outs = (torch.full((h,), -7, dtype=torch.int32, device=dev), torch.full((h,), -7, dtype=torch.int64, device=dev),
            torch.full((h,), -7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ctx.schedule_sequential_spread_device(h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                          0 if req is None else req.shape[0], 0 if rq is None else rq.data_ptr(), 0,
                                          outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), stream.cuda_stream)
    return outs, (t, rq)


def test_device_form_on_two_streams(msh, oracle, ctx):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(31)
    n, p, h = 600, 300, 150
    u, nd, pd, pt = rand_case(rng, n, p)
    zone = rng.integers(-1, 3, n)
    grp = rng.integers(-1, 2, p).astype(np.int32)
    alloc = rng.integers(0, 9, (3, n)).astype(np.int64)
    req = rng.integers(0, 3, (3, p)).astype(np.int64)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[3], normalize=[1]), u, nd, zone, [1, 1], alloc,
               cap=rng.integers(0, 3, n))
    want = m.expect(pd, pt, grp, req)
    streams = [torch.cuda.Stream(torch.device("cuda:0")) for _ in range(2)]
    runs = [device_call(torch, ctx, pd[k * h:(k + 1) * h], pt[k * h:(k + 1) * h], grp[k * h:(k + 1) * h],
                        req[:, k * h:(k + 1) * h], st) for k, st in enumerate(streams)]  # ordered by the library
    for st in streams:
        st.synchronize()
    got = [np.concatenate([runs[k][0][q].cpu().numpy() for k in range(2)]) for q in range(3)]
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:3]))
    m.commit(want, True)
    m.verify("two streams")


def test_device_form_treats_groups_out_of_range_as_ungrouped(msh, oracle, ctx):
    """Ordinary input of the unvalidated device form: -7, G and 2^30 are ungrouped pods."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(41)
    n, p, G = 300, 200, 3
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    zone = rng.integers(-1, 3, n)
    grp = rng.choice([-7, -1, 0, 1, 2, G, 2**30], p).astype(np.int32)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 1, 2], cap=rng.integers(0, 4, n))
    want = m.expect(pd, pt, grp)
    clean = m.expect(pd, pt, np.where((grp >= 0) & (grp < G), grp, -1))
    assert all(np.array_equal(a, b) for a, b in zip(want, clean))
    st = torch.cuda.Stream(torch.device("cuda:0"))
    outs, _keep = device_call(torch, ctx, pd, pt, grp, None, st)
    st.synchronize()
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, want[:3]))
    m.commit(want, False)
    m.verify("out-of-range groups")


def test_refusals_change_nothing(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(3)
    n, p = 50, 40
    u, nd, pd, pt = rand_case(rng, n, p)
    zone = rng.integers(-1, 3, n)
    grp = rng.integers(-1, 2, p)
    alloc = rng.integers(0, 9, (2, n)).astype(np.int64)
    req = rng.integers(0, 3, (2, p)).astype(np.int64)
    ps = oracle.PluginSet()

    def refused(code, fn, *a, **kw):
        with pytest.raises(msh.MshError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code, ei.value
        return str(ei.value)

    with msh.DeviceContext(0) as fresh:
        refused(E.MSH_ERR_STATE, fresh.upload_node_zones, np.zeros(0, np.int32))   # before msh_upload_nodes
        refused(E.MSH_ERR_INVALID, fresh.patch_spread_counts, [0], [0], [1])       # no groups
        assert fresh.spread_counts().shape == (0, 64) and fresh.seq_spread_max_nodes(0) == ctx.seq_spread_max_nodes(2)
        refused(E.MSH_ERR_INVALID, fresh.seq_spread_max_nodes, 5)
    m = Mirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2], alloc)
    m.spread(pd, pt, grp, req, what="before the refusals")
    call = ctx.schedule_sequential_spread
    # the writers' argument errors
    for bad in (zone[:-1], np.append(zone, 0), np.where(np.arange(n) == 3, 64, zone), np.where(np.arange(n) == 3, -2, zone)):
        refused(E.MSH_ERR_INVALID, ctx.upload_node_zones, bad)
    for bad in ([0, 1], [1, -5], np.ones(129, np.int32)):
        refused(E.MSH_ERR_INVALID, ctx.set_spread_groups, bad)
    for g, z, v in (([0, 0], [1, 1], [1, 1]), ([2], [0], [1]), ([-1], [0], [1]), ([0], [64], [1]), ([0], [-1], [1]),
                    ([0], [0], [-1])):
        refused(E.MSH_ERR_INVALID, ctx.patch_spread_counts, g, z, v)
    assert np.array_equal(ctx.node_zones(), zone) and ctx.spread_groups().tolist() == [1, 2]
    m.verify("writer argument errors")
    # the call's argument errors (host form)
    refused(E.MSH_ERR_INVALID, call, pd, pt, np.where(np.arange(p) == 5, 2, grp), req)       # a group == G
    refused(E.MSH_ERR_INVALID, call, pd, pt, np.where(np.arange(p) == 5, -2, grp), req)      # a group below -1
    refused(E.MSH_ERR_INVALID, call, pd, pt, grp, req[:1])                                   # nres != the table's
    refused(E.MSH_ERR_INVALID, call, pd, pt, grp, -req - 1)
    refused(E.MSH_ERR_INVALID, call, pd, pt, grp, req, -1)
    m.verify("call argument errors")
    ctx.set_spread_groups([])
    refused(E.MSH_ERR_INVALID, call, pd, pt, np.zeros(p, np.int32), req)                     # G == 0 and a grouped pod
    ctx.set_spread_groups(m.skew)
    m.cnt[:] = 0  # G changed twice
    m.verify("G == 0")
    m.spread(pd, pt, grp, req, what="between the refusals")
    # unsupported combinations, each naming its reason
    ctx.set_tiebreak("random", 11, 5)
    assert "MSH_TIEBREAK_RANDOM" in refused(E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, req)
    assert ctx.tiebreak() == (E.MSH_TIEBREAK_RANDOM, 11, 5)
    ctx.set_tiebreak("first")
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig("NodeNumber"), msh.ScorePluginConfig("ScoreColumn0")])
    assert "score-column" in refused(E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, req)
    set_plugins(ctx, msh, ps)
    for mode in ("least", "most"):
        ctx.set_resource_score(mode, 1, [1, 1])
        assert "resource score" in refused(E.MSH_ERR_UNSUPPORTED, call, pd, pt, grp, req)
    ctx.set_resource_score("none")
    m.verify("unsupported combinations")
    # state errors: requests without a table, no zone column
    ctx.clear_node_resources()
    refused(E.MSH_ERR_STATE, call, pd, pt, grp, req)
    ctx.upload_node_resources(m.alloc, m.used)
    ctx.clear_node_zones()
    refused(E.MSH_ERR_STATE, call, pd, pt, grp, req)
    assert np.array_equal(ctx.spread_counts(), m.cnt) and np.array_equal(ctx.node_pod_counts(), m.counts)


def test_seeded_sweep(msh, oracle, ctx):
    """40 cases from the shared generator (tests/test_spread.py asserts that they are not trivial)."""
    for seed in SWEEP_SEEDS:
        c = S.gen_case(seed)
        ps = oracle.PluginSet(weights=[c["weight"]], normalize=[c["mode"]])
        cols, _, res, sp = sweep_inputs(c)
        m = Mirror(ctx, msh, oracle, ps, cols[0], cols[1], sp[0], sp[2], res[0] if c["nres"] else None, c["cap"])
        m.spread(cols[2], cols[3], sp[1], res[2] if c["nres"] else None, what=f"seed {seed}")


def test_scheduler_with_zones_and_spread_groups(msh, oracle):
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
    s = msh.Scheduler(resources=("cpu",), zones=zkey, spread_groups={"web": 1, "db": 2})
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
        want = S.serial(oracle, nt.unsched, nt.digit, pdig, np.zeros(p, np.uint8), oracle.PluginSet(), S.no_limit(n), alloc,
                        np.zeros_like(alloc), np.array([rc * 500], np.int64), zone, grp, [1, 2])
        assert [int(r.outcome) for r in res] == want[2].tolist()
        assert [r.node_index for r in res] == want[0].tolist() and [r.score for r in res] == want[1].tolist()
        assert (want[2] == S.FIT_ERROR).any() and (want[2] == S.PLACED).any()
        assert np.array_equal(s.ctx.spread_counts(), want[5]) and np.array_equal(s.ctx.node_pod_counts(), want[3])
        assert np.array_equal(s.ctx.node_resources()[1], want[4]) and np.array_equal(s.ctx.node_zones(), zone)
    finally:
        s.close()
    with pytest.raises(ValueError):
        msh.Scheduler(zones=zkey)
