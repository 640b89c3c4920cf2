"""Resource-aware scoring in sequential-commit mode on the GPU (msh_set_resource_score; csrc/msh_seq_score.hip).

Every comparison is bit-exact on idx, score, status, node_pod_counts() and the `used` half of node_resources()
against tests/resource_score_ref.py: the literal loop (`serial`) for tiny shapes, the numpy form (`per_pod`)
otherwise. tests/test_resource_score.py checks on the CPU that the two agree. Table limits and the sizes at which
another kernel instance takes over (1, 4 or 16 waves) come from msh_seq_fit_max_nodes: the limit is 1,024 threads x
nodes per thread, the thresholds 64 and 256 threads."""
from __future__ import annotations

import numpy as np
import pytest

import node_capacity_ref as CR
import resource_fit_ref as R
import resource_score_ref as S
from test_resource_score import SWEEP_SIZES, differs_from_unscored, eff_of, sweep

pytestmark = pytest.mark.gpu

MODES = {S.NONE: "none", S.LEAST: "least", S.MOST: "most"}


def rand_case(rng, n, p, digits=3, p_unsched=0.2):
    u = (rng.random(n) < p_unsched).astype(np.uint8)
    nd = rng.integers(-1, digits, n).astype(np.int8)
    pd = rng.integers(0, digits, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return u, nd, pd, pt


def rand_amounts(rng, nres, n, p, unit=1):
    alloc = rng.integers(20, 200, (nres, n)) * unit
    used = rng.integers(0, 10, (nres, n)) * unit
    req = rng.integers(0, 4, (nres, p)) * unit
    return alloc.astype(np.int64), used.astype(np.int64), req.astype(np.int64)


def set_plugins(ctx, msh, ps):
    ctx.set_plugins(ps.filters, ps.prescore,
                    [msh.ScorePluginConfig(s, w, msh.Normalize(m)) for s, w, m in zip(ps.score, ps.weights, ps.normalize)])


def same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "score", "status")):
        assert np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(np.asarray(g) != np.asarray(w))[:5]}"


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.set_resource_score("none")
    c.close()


def start(ctx, msh, ps, u, nd, alloc, used=None):
    set_plugins(ctx, msh, ps)
    ctx.set_tiebreak("first")
    ctx.upload_nodes(u, nd)  # zeroes the counts, drops the column and the table
    ctx.upload_node_resources(alloc, used)
    return np.zeros_like(alloc) if used is None else np.asarray(used, np.int64)


def check(ctx, O, u, nd, pd, pt, ps, eff, alloc, used, req, counts, what, mode, weight=1, rw=None, scalar=0):
    """Sets the resource score, runs one _fit call on the device's table; returns the expected (counts, used)."""
    rw = [1] * len(alloc) if rw is None else rw
    ctx.set_resource_score(MODES[mode], weight, rw)
    ref = S.serial if len(u) * len(pd) <= 2 * 10**4 else S.per_pod
    got = ctx.schedule_sequential_fit(pd, pt, req, scalar)
    wi, ws, wst, cnt, us = ref(O, u, nd, pd, pt, ps, eff, alloc, used, req, mode, weight, rw, counts)
    same(got, (wi, ws, wst), what)
    assert np.array_equal(ctx.node_pod_counts(), cnt), f"{what}: counts"
    a, b = ctx.node_resources()
    assert np.array_equal(a, alloc), f"{what}: alloc moved"
    assert np.array_equal(b, us), f"{what}: used differs at {np.argwhere(b != us)[:5].tolist()}"
    return cnt, us


def refused(msh, code, fn, *a, **kw):
    with pytest.raises(msh.MshError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value
    return str(ei.value)


@pytest.mark.parametrize("mode", [S.LEAST, S.MOST])
@pytest.mark.parametrize("nres", [1, 2, 3, 4])
def test_boundary_sizes(msh, oracle, ctx, nres, mode):
    """One node, both thresholds between kernel instances -1 / +0 / +1, and the limit, 65 pods each."""
    lim = ctx.seq_fit_max_nodes(nres, scored=True)
    assert lim % 1024 == 0 and ctx.seq_fit_max_nodes(nres) == (8192 if nres <= 2 else 4096)
    npl = lim // 1024
    rng = np.random.default_rng(10 * nres + mode)
    ps = oracle.PluginSet(weights=[3], normalize=[nres % 4])
    for n in (1, 64 * npl - 1, 64 * npl, 64 * npl + 1, 256 * npl - 1, 256 * npl, 256 * npl + 1, lim):
        p = 65
        u, nd, pd, pt = rand_case(rng, n, p)
        alloc, used0, req = rand_amounts(rng, nres, n, p, unit=int(rng.choice([1, 2**33])))
        if n > 300:  # the best nodes in the last lanes, so that every wave of the table takes part
            alloc[:, : n - 40] //= 4
        used = start(ctx, msh, ps, u, nd, alloc, used0)
        check(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, f"nres={nres} n={n}", mode,
              rw=[1 + r for r in range(nres)])


@pytest.mark.parametrize("nres", [1, 2, 3, 4])
def test_one_node_past_the_limit_is_refused(msh, oracle, ctx, nres):
    E = msh._native
    lim = ctx.seq_fit_max_nodes(nres, scored=True)
    n = lim + 1
    start(ctx, msh, oracle.PluginSet(), np.zeros(n, np.uint8), np.zeros(n, np.int8), np.ones((nres, n), np.int64))
    ctx.set_resource_score("least", 1, [1] * nres)
    args = (np.zeros(3, np.int8), np.zeros(3, np.uint8), np.ones((nres, 3), np.int64))
    assert f"{lim} nodes" in refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, *args)
    assert ctx.node_pod_counts().sum() == 0 and ctx.node_resources()[1].sum() == 0
    ctx.set_resource_score("none")  # the unscored form still takes the table
    assert (ctx.schedule_sequential_fit(*args)[2] == R.PLACED).all()


def test_every_normalize_mode(msh, oracle, ctx):
    """NodeNumber in every normalize mode at weight 1 and 2^32 against the resource score at weight 1 and 2^32;
    NodeNumber absent; NodeNumber without its PreScore state (score errors); pods without a digit."""
    rng = np.random.default_rng(41)
    n, p = 70, 90
    lists = [oracle.PluginSet(weights=[w], normalize=[m]) for m in (0, 1, 2, 3) for w in (1, 2**32)]
    lists += [oracle.PluginSet(["NodeUnschedulable"], ["NodeNumber"], [], [], []),
              oracle.PluginSet(["NodeUnschedulable"], [], ["NodeNumber"], [1], [0])]
    for k, ps in enumerate(lists):
        for weight in (1, 2**32):
            u, nd, pd, pt = rand_case(rng, n, p)
            pd[rng.random(p) < 0.15] = -1
            alloc, used0, req = rand_amounts(rng, 2, n, p)
            used = start(ctx, msh, ps, u, nd, alloc, used0)
            check(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, f"list {k} weight {weight}",
                  S.LEAST if k % 2 else S.MOST, weight)


@pytest.mark.parametrize("mode", [S.LEAST, S.MOST])
def test_exact_division(msh, oracle, ctx, mode):
    """Quotients on their boundaries: for every divisor c and every k, a node whose numerator is the smallest with
    num * 100 / c == k and one whose numerator is one below it; numerator 0 and numerator c; c = 0; q > c. One pod
    per node (max_pods_per_node = 1), as many pods as nodes: the pods walk the nodes in the order of their exact
    scores, so every node's quotient decides a placement and shows in out_score."""
    cs = [3, 7, 100, 2**32 - 1, 2**32 + 1, 2**53 + 1, 2**55]
    alloc, used = [], []
    for c in cs:
        for k in (0, 1, 33, 50, 67, 99, 100):
            for num in {-(-k * c // 100), max(-(-k * c // 100) - 1, 0)}:  # ceil(k c / 100) and one below
                free = num if mode == S.LEAST else c - num  # LEAST divides free - req, MOST c - free + req
                alloc.append(c)
                used.append(c - free)
    alloc += [0, 0, 5, 2**55 - 1]
    used += [0, 3, 6, 2**55]  # c = 0 twice, q > c twice
    n = len(alloc)
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    alloc, used = np.array(alloc, np.int64)[perm].reshape(1, n), np.array(used, np.int64)[perm].reshape(1, n)
    ps = oracle.PluginSet()
    u, nd = np.zeros(n, np.uint8), np.zeros(n, np.int8)
    pd, pt = np.zeros(n, np.int8), np.zeros(n, np.uint8)
    eff = np.ones(n, np.int64)
    us = start(ctx, msh, ps, u, nd, alloc, used)
    cnt, _ = check(ctx, oracle, u, nd, pd, pt, ps, eff, alloc, us, np.zeros((1, n), np.int64), None, "zero requests",
                   mode, scalar=1)
    assert cnt.tolist() == [1] * n
    # the same numerators reached through a request: used one unit lower where that is possible, every pod asks 1
    low = np.maximum(used - 1, 0)
    us = start(ctx, msh, ps, u, nd, alloc, low)
    check(ctx, oracle, u, nd, pd, pt, ps, eff, alloc, us, np.ones((1, n), np.int64), None, "unit requests", mode, scalar=1)


def test_tie_break_and_spreading(msh, oracle, ctx):
    ps = oracle.PluginSet()
    n, p = 8, 64
    u, nd = np.zeros(n, np.uint8), np.zeros(n, np.int8)
    pd, pt = np.zeros(p, np.int8), np.zeros(p, np.uint8)
    alloc = np.full((2, n), 1000, np.int64)
    req = np.full((2, p), 10, np.int64)
    used = start(ctx, msh, ps, u, nd, alloc)
    cnt, _ = check(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, "LEAST spreads", S.LEAST)
    assert cnt.tolist() == [8] * n
    ctx.set_resource_score("least")
    ctx.upload_node_resources(alloc)
    ctx.reset_node_pod_counts()
    assert ctx.schedule_sequential_fit(pd[:9], pt[:9], req[:, :9])[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    alloc = np.full((2, n), 80, np.int64)  # eight pods of 10 fill a node
    used = start(ctx, msh, ps, u, nd, alloc)
    ctx.set_resource_score("most")
    idx = ctx.schedule_sequential_fit(pd, pt, req)[0]
    assert idx.tolist() == [j // 8 for j in range(p)]  # MOST fills in List order
    used = start(ctx, msh, ps, u, nd, alloc)
    check(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, "MOST packs", S.MOST)
    # the match class and the non-match class tie on total (10 + 50 against 0 + 60): the lower index wins, whichever
    # class it is in
    for nd2, want in (([0, 1], 0), ([1, 0], 0)):
        alloc = np.array([[100, 100]], np.int64)
        used0 = np.array([[50, 40]] if nd2 == [0, 1] else [[40, 50]], np.int64)
        u2 = np.zeros(2, np.uint8)
        used = start(ctx, msh, ps, u2, np.array(nd2, np.int8), alloc, used0)
        ctx.set_resource_score("least")
        got = ctx.schedule_sequential_fit(np.zeros(1, np.int8), np.zeros(1, np.uint8), np.zeros((1, 1), np.int64))
        assert (got[0].tolist(), got[1].tolist()) == ([want], [60])


@pytest.mark.parametrize("rw", [[1, 1], [1, 0], [3, 1], [100, 1, 0, 7]])
def test_resource_weights(msh, oracle, ctx, rw):
    rng = np.random.default_rng(sum(rw))
    nres, n, p = len(rw), 150, 120
    ps = oracle.PluginSet(weights=[2], normalize=[1])
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used0, req = rand_amounts(rng, nres, n, p, unit=7)
    for mode in (S.LEAST, S.MOST):
        used = start(ctx, msh, ps, u, nd, alloc, used0)
        check(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, f"rw={rw}", mode, 3, rw)
    assert ctx.resource_score() == (S.MOST, 3, rw)


@pytest.mark.parametrize("kind", ["scalar", "column", "both"])
def test_with_pod_capacities(msh, oracle, ctx, kind):
    rng = np.random.default_rng(len(kind))
    ps = oracle.PluginSet(weights=[3], normalize=[2])
    n, p = 130, 257
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used0, req = rand_amounts(rng, 2, n, p)
    cap = rng.integers(0, 5, n)
    scalar = 0 if kind == "column" else 2
    used = start(ctx, msh, ps, u, nd, alloc, used0)
    if kind != "scalar":
        ctx.upload_node_capacity(cap)
    eff = np.full(n, scalar, np.int64) if kind == "scalar" else CR.effective(cap, scalar)
    cnt, used = check(ctx, oracle, u, nd, pd, pt, ps, eff, alloc, used, req, None, kind, S.MOST, scalar=scalar)
    assert (cnt <= eff).all()
    check(ctx, oracle, u, nd, pd[:70], pt[:70], ps, eff, alloc, used, req[:, :70], cnt, kind + " again", S.LEAST, scalar=scalar)


def test_carried_state_patches_and_setter(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(77)
    ps = oracle.PluginSet()
    n, p = 90, 400
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used0, req = rand_amounts(rng, 2, n, p)
    eff = R.no_limit(n)
    used = start(ctx, msh, ps, u, nd, alloc, used0)
    sl = lambda a, b: (pd[a:b], pt[a:b], req[:, a:b])  # noqa: E731
    a, b, c = sl(0, 80)
    cnt, used = check(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, None, "first call", S.LEAST, 2, [2, 1])
    a, b, c = sl(80, 120)
    cnt, used = check(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "carried state", S.LEAST, 2, [2, 1])
    a, b, c = sl(120, 160)  # switching the mode between calls
    cnt, used = check(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "switched to MOST", S.MOST, 2, [2, 1])
    a, b, c = sl(160, 200)  # an unscored _fit call in between
    cnt, used = check(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "mode NONE in between", S.NONE)
    # a plain sequential call ignores the setting and the table
    ctx.set_resource_score("least", 5, [1, 1])
    a, b, _ = sl(200, 300)
    want = R.per_pod(oracle, u, nd, a, b, ps, eff, alloc, used, np.zeros((2, 100), np.int64), cnt)
    same(ctx.schedule_sequential(a, b, 0), want[:3], "plain call with a resource score set")
    cnt = want[3]
    assert np.array_equal(ctx.node_resources()[1], used)
    a, b, c = sl(300, 330)
    cnt, used = check(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "after the plain call", S.LEAST, 5)
    # msh_patch_node_resources: alloc lowered below used on two nodes, raised on two, used reset on one
    busy = np.flatnonzero(used[0] > 0)
    down, up, zero = busy[:2].astype(np.int32), busy[2:4].astype(np.int32), busy[4:5].astype(np.int32)
    alloc[:, down] = np.maximum(used[:, down] - 1, 0)
    ctx.patch_node_resources(down, alloc=alloc[:, down])
    alloc[:, up] += 500
    ctx.patch_node_resources(up, alloc=alloc[:, up])
    used[:, zero] = 0
    ctx.patch_node_resources(zero, used=used[:, zero])
    a, b, c = sl(330, 365)
    c = c.copy()
    c[:, ::3] = 0  # zero requests reach the over-committed nodes
    cnt, used = check(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "after the resource patches", S.MOST, 5)
    u = u.copy()
    flip = np.arange(0, n, 7, dtype=np.int32)
    u[flip] ^= 1
    ctx.patch_nodes(flip, u[flip], nd[flip])
    a, b, c = sl(365, 400)
    check(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "after msh_patch_nodes", S.LEAST, 5)
    # the setting is policy: it survives msh_upload_nodes and msh_clear_node_resources
    ctx.set_resource_score("most", 9, [4, 0])
    ctx.clear_node_resources()
    ctx.upload_nodes(u, nd)
    assert ctx.resource_score() == (E.MSH_RESOURCE_SCORE_MOST_ALLOCATED, 9, [4, 0])
    ctx.upload_node_resources(alloc)
    ctx.set_resource_score("least")  # resource_weights=None: 1 for each resource of the table
    assert ctx.resource_score() == (E.MSH_RESOURCE_SCORE_LEAST_ALLOCATED, 1, [1, 1])


def test_device_entry_point_on_two_streams(msh, oracle, ctx):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(31)
    ps = oracle.PluginSet(weights=[3], normalize=[1])
    n, p, h = 600, 300, 150
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used0, req = rand_amounts(rng, 3, n, p)
    used = start(ctx, msh, ps, u, nd, alloc, used0)
    rw = [1, 2, 3]
    ctx.set_resource_score("least", 4, rw)
    wi, ws, wst, cnt, us = S.per_pod(oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, S.LEAST, 4, rw)
    dev = torch.device("cuda:0")
    outs, keep = [], []
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for k in range(2):
        a, b = k * h, (k + 1) * h
        keep.append((torch.from_numpy(pd[a:b].copy()).to(dev), torch.from_numpy(pt[a:b].copy()).to(dev),
                     torch.from_numpy(np.ascontiguousarray(req[:, a:b])).to(dev)))
        outs.append((torch.full((h,), -7, dtype=torch.int32, device=dev), torch.full((h,), -7, dtype=torch.int64, device=dev),
                     torch.full((h,), -7, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for k, st in enumerate(streams):  # the second launch is ordered behind the first by the library
        d_pd, d_pt, d_rq = keep[k]
        oi, osc, ost = outs[k]
        ctx.schedule_sequential_fit_device(h, d_pd.data_ptr(), d_pt.data_ptr(), 3, d_rq.data_ptr(), 0, oi.data_ptr(),
                                           osc.data_ptr(), ost.data_ptr(), st.cuda_stream)
    for st in streams:
        st.synchronize()
    got = [np.concatenate([outs[k][q].cpu().numpy() for k in range(2)]) for q in range(3)]
    same(got, (wi, ws, wst), "two streams")
    assert np.array_equal(ctx.node_pod_counts(), cnt) and np.array_equal(ctx.node_resources()[1], us)


def test_refusals(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(3)
    ps = oracle.PluginSet()
    n, p = 50, 40
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used0, req = rand_amounts(rng, 2, n, p)
    used = start(ctx, msh, ps, u, nd, alloc, used0)
    ctx.set_resource_score("most", 3, [5, 6])
    setting = ctx.resource_score()
    # the setter: a failed call changes nothing
    for args in ((3, 1, [1, 1]), ("least", 0, [1, 1]), ("least", 2**32 + 1, [1, 1]), ("least", 1, []),
                 ("least", 1, [1] * 5), ("least", 1, [0, 0]), ("least", 1, [1, 101]), ("least", 1, [-1, 1])):
        refused(msh, E.MSH_ERR_INVALID, ctx.set_resource_score, *args)
        assert ctx.resource_score() == setting
    assert msh._native.lib().msh_set_resource_score(ctx.handle, 1, 1, 2, None) == E.MSH_ERR_INVALID
    ctx.set_resource_score("least", 2**32, [100, 0])  # the ends of the ranges are inside
    cnt, used = check(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, "before the refusals", S.LEAST)

    def unchanged(what):
        a, b = ctx.node_resources()
        assert np.array_equal(a, alloc) and np.array_equal(b, used) and np.array_equal(ctx.node_pod_counts(), cnt), what

    ctx.set_resource_score("least", 1, [1, 1, 1])  # nres of the setting != the table's
    refused(msh, E.MSH_ERR_STATE, ctx.schedule_sequential_fit, pd, pt, req)
    ctx.set_resource_score("least", 1, [1, 1])
    refused(msh, E.MSH_ERR_INVALID, ctx.schedule_sequential_fit, pd, pt, req + 2**55 + 1)  # a host request past 2^55
    assert "2^55" in refused(msh, E.MSH_ERR_INVALID, ctx.schedule_sequential_fit, pd, pt, np.full_like(req, 2**55 + 1))
    unchanged("argument errors")
    ctx.set_tiebreak("random", 11, 5)
    refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, pd, pt, req)
    ctx.set_tiebreak("first")
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig("NodeNumber"), msh.ScorePluginConfig("ScoreColumn0")])
    refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, pd, pt, req)
    set_plugins(ctx, msh, ps)
    unchanged("RANDOM and score columns")
    # the 2^55 bound, tripped by a patch ...
    big = np.full((2, 1), 2**55 + 1, np.int64)
    ctx.patch_node_resources([3], alloc=big)
    assert "2^55" in refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, pd, pt, req)
    ctx.set_resource_score("none")  # the unscored form takes the table as it is
    ctx.schedule_sequential_fit(pd[:1], pt[:1], np.zeros((2, 1), np.int64))
    ctx.set_resource_score("least", 1, [1, 1])
    ctx.patch_node_resources([3], alloc=alloc[:, [3]])  # the bound is the largest value written since the upload
    refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, pd, pt, req)
    # ... and by an upload; an upload within the limit resets it, 2^55 itself is inside
    top = alloc.copy()
    top[0, 0] = 2**55 + 1
    ctx.upload_node_resources(top)
    refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, pd, pt, req)
    top[0, 0] = 2**55
    ctx.upload_node_resources(top, used)
    ctx.reset_node_pod_counts()
    check(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), top, used, req, None, "2^55 is inside", S.LEAST)
    ctx.clear_node_resources()  # no table
    refused(msh, E.MSH_ERR_STATE, ctx.schedule_sequential_fit, pd, pt, req)


def test_existing_calls_ignore_the_setting(msh, oracle, ctx):
    """Batch and plain sequential calls with a resource score set equal the same calls without; mode NONE equals
    the unscored _fit output on the same inputs."""
    rng = np.random.default_rng(8)
    ps = oracle.PluginSet(weights=[3], normalize=[3])
    n, p = 700, 400
    u, nd, pd, pt = rand_case(rng, n, p, digits=10)
    alloc, used0, req = rand_amounts(rng, 2, n, p)
    set_plugins(ctx, msh, ps)
    results = []
    for setting in ("none", "least"):
        ctx.upload_nodes(u, nd)
        ctx.upload_node_resources(alloc, used0)
        ctx.set_resource_score(setting, 7, [1, 1])
        out = [ctx.schedule_batch(pd, pt)]
        for scalar in (0, 2):
            ctx.reset_node_pod_counts()
            out.append(ctx.schedule_sequential(pd, pt, scalar))
            out.append((ctx.node_pod_counts(),))
        assert np.array_equal(ctx.node_resources()[1], used0)
        if setting != "least":
            ctx.reset_node_pod_counts()
            out.append(ctx.schedule_sequential_fit(pd, pt, req))
            out.append(ctx.node_resources())
        results.append(out)
    assert len(results[1]) == 5
    for a, b in zip(results[0], results[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    want = R.per_pod(oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used0, req)
    same(results[0][-2], want[:3], "mode NONE is the unscored form")
    assert np.array_equal(results[0][-1][1], want[4])


def test_random_sweep(msh, oracle, ctx):
    """The sweep tests/test_resource_score.py draws (fixed seed and count), each case against the reference; at
    least 90% of the cases differ from the unscored reference in some placement (from the CPU references alone)."""
    cases = sweep(oracle)
    assert max(SWEEP_SIZES) <= ctx.seq_fit_max_nodes(4, scored=True)
    differ = 0
    for k, c in enumerate(cases):
        differ += differs_from_unscored(oracle, c)
        used = start(ctx, msh, c["plugins"], c["u"], c["nd"], c["alloc"], c["used"])
        if c["cap"] is not None:
            ctx.upload_node_capacity(c["cap"])
        what = f"case {k}: n={c['n']} p={c['p']} nres={c['nres']} mode={c['mode']} rw={c['rw']} weight={c['weight']}"
        cnt, used = check(ctx, oracle, c["u"], c["nd"], c["pd"], c["pt"], c["plugins"], eff_of(c), c["alloc"], used, c["req"],
                          None, what, c["mode"], c["weight"], c["rw"], scalar=c["scalar"])
        if k % 3 == 0:
            check(ctx, oracle, c["u"], c["nd"], c["pd"], c["pt"], c["plugins"], eff_of(c), c["alloc"], used, c["req"], cnt,
                  what + " again", c["mode"], c["weight"], c["rw"], scalar=c["scalar"])
    assert differ >= 0.9 * len(cases), differ


def test_scheduler_end_to_end(msh, oracle):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    n, p = 6, 24
    nodes = [{"metadata": {"name": f"node{i}"}, "spec": {},
              "status": {"allocatable": {"cpu": "4", "memory": "8Gi"}}} for i in range(n)]
    pods = [{"metadata": {"name": f"pod{j % 3}"},
             "spec": {"containers": [{"resources": {"requests": {"cpu": "500m", "memory": "256Mi"}}}]}} for j in range(p)]
    alloc = np.array([[4000] * n, [8 * 2**30] * n], np.int64)
    req = np.array([[500] * p, [256 * 2**20] * p], np.int64)
    pdig = np.array([j % 3 for j in range(p)], np.int8)
    spread = {}
    for name, mode, rw, kw in (("least", S.LEAST, [1, 1], {}),
                               ("most", S.MOST, [2, 0], dict(resource_score_weight=3, resource_weights={"cpu": 2}))):
        s = msh.Scheduler(resources=("cpu", "memory"), resource_score=name, **kw)
        try:
            res = s.schedule_sequential(pods, nodes)
            nt = s.nodes
            wi, ws, wst, cnt, us = S.serial(oracle, nt.unsched, nt.digit, pdig, np.zeros(p, np.uint8), oracle.PluginSet(),
                                           R.no_limit(n), alloc, np.zeros_like(alloc), req, mode,
                                           kw.get("resource_score_weight", 1), rw)
            assert [r.node_index for r in res] == wi.tolist() and [r.score for r in res] == ws.tolist()
            assert [int(r.outcome) for r in res] == wst.tolist()
            assert np.array_equal(s.ctx.node_pod_counts(), cnt) and np.array_equal(s.ctx.node_resources()[1], us)
            spread[name] = len({r.node_index for r in res})
        finally:
            s.close()
    assert spread["least"] > spread["most"], spread  # spread over more nodes than packed onto
