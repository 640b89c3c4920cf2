"""Resource requests in sequential-commit mode on the GPU (msh_schedule_sequential_fit and friends).

Every comparison is bit-exact on idx, score, status, node_pod_counts() and the `used` half of node_resources().
The expected values come from tests/resource_fit_ref.py: the plain serial loop (`serial`) for tiny shapes, the
numpy per-pod loop (`per_pod`) for mid sizes and the unchanged C oracle through the second-capacity identity
(`via_oracle`) for unit requests. tests/test_resource_fit.py checks on the CPU that the three agree.

The kernel (csrc/msh_seq_fit.hip) holds 8 nodes per thread for one or two resources and 4 for three or four, on
1, 4 or 16 waves: 512 / 2,048 / 8,192 and 256 / 1,024 / 4,096 nodes are its thresholds and limits."""
from __future__ import annotations

import numpy as np
import pytest

import node_capacity_ref as CR
import resource_fit_ref as R

pytestmark = pytest.mark.gpu

MODES_WEIGHTS = [(m, w) for m in (0, 1, 2, 3) for w in (1, 3, 2**32)]
NODE_SIZES = (1, 5, 63, 64, 65, 1023, 1024, 1025)
POD_SIZES = (0, 1, 63, 64, 65, 257)


def limit(nres):
    return 8192 if nres <= 2 else 4096


def thresholds(nres):
    npl = 8 if nres <= 2 else 4
    return (64 * npl, 64 * npl + 1, 256 * npl, 256 * npl + 1, limit(nres))


def rand_case(rng, n, p, p_unsched=0.3, digits=10):
    u = (rng.random(n) < p_unsched).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, digits, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return u, nd, pd, pt


def rand_amounts(rng, nres, n, p, unit=1):
    alloc = rng.integers(0, 9, (nres, n)) * unit
    req = rng.integers(0, 4, (nres, p)) * unit
    return alloc.astype(np.int64), req.astype(np.int64)


def set_plugins(ctx, msh, ps):
    ctx.set_plugins(ps.filters, ps.prescore,
                    [msh.ScorePluginConfig(s, w, msh.Normalize(m)) for s, w, m in zip(ps.score, ps.weights, ps.normalize)])


def same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "score", "status")):
        assert np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(np.asarray(g) != np.asarray(w))[:5]}"


def pick_ref(n, p):
    return R.serial if n * p <= 2 * 10**4 else R.per_pod


def check_fit(ctx, O, u, nd, pd, pt, ps, eff, alloc, used, req, counts, what, scalar=0, ref=None):
    """One _fit call against the table on the device; returns the expected (counts, used) after it."""
    ref = ref or pick_ref(len(u), len(pd))
    got = ctx.schedule_sequential_fit(pd, pt, req, scalar)
    wi, ws, wst, cnt, us = ref(O, u, nd, pd, pt, ps, eff, alloc, used, req, counts)
    same(got, (wi, ws, wst), what)
    assert np.array_equal(ctx.node_pod_counts(), cnt), f"{what}: counts"
    a, b = ctx.node_resources()
    assert np.array_equal(a, alloc), f"{what}: alloc moved"
    assert np.array_equal(b, us), f"{what}: used differs at {np.argwhere(b != us)[:5].tolist()}"
    return cnt, us


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.close()


def start(ctx, msh, ps, u, nd, alloc, used=None):
    set_plugins(ctx, msh, ps)
    ctx.set_tiebreak("first")
    ctx.upload_nodes(u, nd)  # zeroes the counts, drops the column and the table
    ctx.upload_node_resources(alloc, used)
    return np.zeros_like(alloc) if used is None else np.asarray(used, np.int64)


@pytest.mark.parametrize("nres", [1, 2, 3, 4])
def test_boundary_sizes(msh, oracle, ctx, nres):
    """Every listed node count, every size at which another kernel instance takes over, and the limit, each
    with 65 pods; every listed pod count at 65 and 1,025 nodes."""
    rng = np.random.default_rng(100 + nres)
    ps = oracle.PluginSet(weights=[3], normalize=[nres % 4])
    shapes = [(n, 65) for n in NODE_SIZES + thresholds(nres)] + [(n, p) for n in (65, 1025) for p in POD_SIZES]
    for n, p in shapes:
        u, nd, pd, pt = rand_case(rng, n, p)
        alloc, req = rand_amounts(rng, nres, n, p, unit=int(rng.choice([1, 2**33])))
        if n > 1100:  # keep the early nodes scarce so that the pods reach every wave of the table
            alloc[:, : n - 40] //= 8
        used = start(ctx, msh, ps, u, nd, alloc)
        check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, f"nres={nres} n={n} p={p}")


@pytest.mark.parametrize("nres", [1, 2, 3, 4])
def test_one_node_past_the_limit_is_refused(msh, oracle, ctx, nres):
    n = limit(nres) + 1
    ps = oracle.PluginSet()
    start(ctx, msh, ps, np.zeros(n, np.uint8), np.zeros(n, np.int8), np.ones((nres, n), np.int64))
    with pytest.raises(msh.MshError) as ei:
        ctx.schedule_sequential_fit(np.zeros(3, np.int8), np.zeros(3, np.uint8), np.ones((nres, 3), np.int64))
    assert ei.value.code == msh._native.MSH_ERR_UNSUPPORTED and f"{limit(nres)} nodes" in str(ei.value)
    assert ctx.node_pod_counts().sum() == 0 and ctx.node_resources()[1].sum() == 0


def test_random_combinations(msh, oracle, ctx):
    """60 draws from nodes x pods x nres x normalize mode x weight x filter list x prescore list, pods with and
    without a digit and a toleration, a second call on the carried state."""
    rng = np.random.default_rng(60)
    for case in range(60):
        nres = 1 + case % 4
        n = int(rng.choice(NODE_SIZES + thresholds(nres)[:2]))
        p = int(rng.choice(POD_SIZES))
        mode, w = MODES_WEIGHTS[case % 12]
        f = ["NodeUnschedulable"] if rng.random() < 0.7 else []
        pre = ["NodeNumber"] if rng.random() < 0.85 else []  # absent: every feasible pod is a score error
        ps = oracle.PluginSet(f, pre, ["NodeNumber"], [w], [mode])
        u, nd, pd, pt = rand_case(rng, n, p, p_unsched=float(rng.choice([0.0, 0.3, 0.9])), digits=int(rng.choice([2, 10])))
        alloc, req = rand_amounts(rng, nres, n, p, unit=int(rng.choice([1, 2**31, 2**40])))
        used0 = (rng.integers(0, 3, (nres, n)) * (alloc.max() // 8 if alloc.max() else 0)).astype(np.int64)
        used = start(ctx, msh, ps, u, nd, alloc, used0)
        what = f"case {case}: n={n} p={p} nres={nres} mode={mode} w={w} f={f} pre={pre}"
        cnt, used = check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, what)
        if case % 3 == 0:
            check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, cnt, what + " again")


@pytest.mark.parametrize("nres", [1, 2, 4])
def test_64_bit_compares(msh, oracle, ctx, nres):
    """Free amounts and requests around 2^32, 2^40 and at 2^62: an exact fit passes, one unit over fails, and
    pairs whose low dwords order the opposite way from the full values go by the full values."""
    ps = oracle.PluginSet()
    free = [2**32 - 1, 2**32, 2**32 + 1, 2**40 - 1, 2**40, 2**62, 2**33]
    want = [(2**32, 1),       # node 0 is one unit short (and its low dword is the larger one): exact fit on node 1
            (2**32 + 1, 2),   # exact fit on node 2
            (2**32 - 1, 0),   # exact fit on node 0
            (2**40, 4),       # one unit over node 3
            (2**40 - 1, 3),   # exact
            (2**62, 5),       # exact at the top of the range
            (1, -1),          # nothing left on nodes 0..5; node 6 is unschedulable for this pod (below)
            (0, 0),           # a zero request goes by node order
            (2**32 + 5, 6)]   # low dword 5 against node 6's 0: fits by the full value
    n, p = len(free), len(want)
    u = np.zeros(n, np.uint8)
    u[6] = 1
    nd = np.ones(n, np.int8)
    pd = np.ones(p, np.int8)
    pt = np.zeros(p, np.uint8)
    pt[8] = 1
    alloc = np.tile(np.array(free, np.int64), (nres, 1))
    req = np.zeros((nres, p), np.int64)
    req[nres - 1] = [r for r, _ in want]  # the last resource decides; the others ask for nothing
    used = start(ctx, msh, ps, u, nd, alloc)
    idx, _, status = ctx.schedule_sequential_fit(pd, pt, req)
    assert idx.tolist() == [i for _, i in want]
    assert status.tolist() == [R.FIT_ERROR if i < 0 else R.PLACED for _, i in want]
    ctx.upload_node_resources(alloc)
    ctx.reset_node_pod_counts()
    check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, "64-bit", ref=R.serial)


def test_zero_requests(msh, oracle, ctx):
    rng = np.random.default_rng(5)
    ps = oracle.PluginSet()
    n, p = 70, 90
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc = rng.integers(1, 9, (2, n)).astype(np.int64)
    used = start(ctx, msh, ps, u, nd, alloc, alloc.copy())  # every node full
    lowered = np.arange(0, n, 3, dtype=np.int32)
    alloc[:, lowered] -= 1  # alloc below used
    ctx.patch_node_resources(lowered, alloc=alloc[:, lowered])
    req = np.zeros((2, p), np.int64)
    got = ctx.schedule_sequential_fit(pd, pt, req)
    same(got, oracle.c_schedule_sequential(u, nd, pd, pt, ps, 0)[:3], "all-zero pods place on node order alone")
    ctx.reset_node_pod_counts()
    req[0, ::2] = 1  # every second pod asks for one unit of a full table
    cnt, us = check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, "zeros among full nodes")
    assert np.array_equal(us, used) and (ctx.schedule_sequential_fit(pd, pt, req)[2][::2] == R.FIT_ERROR).all()


def test_fills_that_decide(msh, oracle, ctx):
    """Demand about twice the supply: a kernel that ignored the requests could not pass."""
    rng = np.random.default_rng(50200)
    ps = oracle.PluginSet()
    n, p = 50, 200
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.1)
    alloc = rng.integers(0, 9, (2, n)).astype(np.int64) * 1000
    req = rng.integers(1, 4, (2, p)).astype(np.int64) * 1000
    zero = np.zeros((2, n), np.int64)
    wi, ws, wst, _, _ = R.serial(oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, zero, req)
    zi, zs, zst, _, _ = R.serial(oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, zero, np.zeros_like(req))
    assert not np.array_equal(wi, zi)
    assert ((wst == R.FIT_ERROR) & (zst == R.PLACED)).any()  # unschedulable for resources alone
    placed = (wst == R.PLACED) & (zst == R.PLACED)
    level = lambda i, j: nd[i] == pd[j]  # noqa: E731
    assert any(placed[j] and zi[j] < wi[j] and level(zi[j], j) == level(wi[j], j) for j in range(p))  # skipped a node
    used = start(ctx, msh, ps, u, nd, alloc)
    check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, "fills", ref=R.serial)
    # one digit for every pod: consecutive pods contend for the same nodes
    pd1 = np.full(p, 4, np.int8)
    used = start(ctx, msh, ps, u, nd, alloc)
    check_fit(ctx, oracle, u, nd, pd1, pt, ps, R.no_limit(n), alloc, used, req, None, "one digit", ref=R.serial)


def test_precedence(msh, oracle, ctx):
    ps = oracle.PluginSet()
    u, nd = np.zeros(3, np.uint8), np.array([1, 2, 3], np.int8)
    alloc = np.array([[4, 4, 4]], np.int64)
    pd = np.array([-1, -1, 2, -1], np.int8)
    pt = np.zeros(4, np.uint8)
    req = np.array([[9, 1, 4, 4]], np.int64)
    used = start(ctx, msh, ps, u, nd, alloc)
    got = ctx.schedule_sequential_fit(pd, pt, req)
    # no node fits 9: FitError though the pod has no digit; 1 fits: its score errors and commits nothing, so pod 2
    # still finds node 1 whole; pod 3 then fits nodes 0 and 2 only: a score error again
    assert got[2].tolist() == [R.FIT_ERROR, R.SCORE_ERROR, R.PLACED, R.SCORE_ERROR] and got[0].tolist() == [-1, -1, 1, -1]
    assert ctx.node_pod_counts().tolist() == [0, 1, 0] and ctx.node_resources()[1].tolist() == [[0, 4, 0]]
    used = start(ctx, msh, ps, u, nd, alloc)
    check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(3), alloc, used, req, None, "precedence", ref=R.serial)


@pytest.mark.parametrize("kind", ["scalar", "column", "both"])
def test_with_pod_capacities(msh, oracle, ctx, kind):
    rng = np.random.default_rng(len(kind))
    ps = oracle.PluginSet(weights=[3], normalize=[2])
    n, p = 130, 257
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, req = rand_amounts(rng, 2, n, p)
    alloc *= 2
    cap = rng.integers(0, 5, n)
    scalar = 0 if kind == "column" else 2
    used = start(ctx, msh, ps, u, nd, alloc)
    if kind != "scalar":
        ctx.upload_node_capacity(cap)
    eff = np.full(n, scalar, np.int64) if kind == "scalar" else CR.effective(cap, scalar)
    cnt, used = check_fit(ctx, oracle, u, nd, pd, pt, ps, eff, alloc, used, req, None, kind, scalar=scalar)
    assert (cnt <= eff).all()
    check_fit(ctx, oracle, u, nd, pd[:70], pt[:70], ps, eff, alloc, used, req[:, :70], cnt, kind + " again", scalar=scalar)


def test_state_patches_and_lifetime(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(77)
    ps = oracle.PluginSet()
    n, p = 90, 400
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, req = rand_amounts(rng, 2, n, p)
    alloc *= 3
    eff = R.no_limit(n)
    ctx.upload_nodes(u, nd)
    assert ctx.node_resources() is None
    used = start(ctx, msh, ps, u, nd, alloc)
    sl = lambda a, b: (pd[a:b], pt[a:b], req[:, a:b])  # noqa: E731
    a, b, c = sl(0, 80)
    cnt, used = check_fit(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, None, "first call")
    a, b, c = sl(80, 120)
    cnt, used = check_fit(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "second call, carried state")
    # a plain sequential call in between: its pods request nothing, commit counts only (here through the batch
    # kernel's count replicas, which the next _fit call folds)
    a, b, _ = sl(120, 220)
    want = R.per_pod(oracle, u, nd, a, b, ps, eff, alloc, used, np.zeros((2, 100), np.int64), cnt)
    same(ctx.schedule_sequential(a, b, 0), want[:3], "plain call with a table present")
    cnt = want[3]
    assert np.array_equal(ctx.node_resources()[1], used)
    a, b, c = sl(220, 260)
    cnt, used = check_fit(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "after the plain call")
    # patches: raise alloc on two nodes, lower it below used on two, set used on two (one freed, one charged)
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
    a, b, c = sl(260, 320)
    cnt, used = check_fit(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "after the patches")
    both = np.array([0, n - 1], np.int32)
    alloc[:, both], used[:, both] = 7, 1
    ctx.patch_node_resources(both, alloc[:, both], used[:, both])
    # msh_patch_nodes and msh_reset_node_pod_counts keep the table and do not touch used
    u = u.copy()
    flip = np.arange(0, n, 7, dtype=np.int32)
    u[flip] ^= 1
    ctx.patch_nodes(flip, u[flip], nd[flip])
    a, b, c = sl(320, 360)
    cnt, used = check_fit(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, cnt, "after msh_patch_nodes")
    ctx.reset_node_pod_counts()
    a, b, c = sl(360, 400)
    check_fit(ctx, oracle, u, nd, a, b, ps, eff, alloc, used, c, None, "after the count reset")
    # msh_clear_node_resources and msh_upload_nodes drop it
    ctx.clear_node_resources()
    assert ctx.node_resources() is None
    for drop in ("clear", "upload"):
        if drop == "upload":
            ctx.upload_node_resources(alloc)
            ctx.upload_nodes(u, nd)
            assert ctx.node_resources() is None
        with pytest.raises(msh.MshError) as ei:
            ctx.schedule_sequential_fit(pd, pt, req)
        assert ei.value.code == E.MSH_ERR_STATE
        with pytest.raises(msh.MshError) as ei:
            ctx.patch_node_resources([0], alloc=[[1], [1]])
        assert ei.value.code == E.MSH_ERR_STATE


def test_identity_at_size(msh, oracle, ctx):
    """Unit requests on 8,192 nodes x 20,000 pods against the C oracle (resource_fit_ref.via_oracle)."""
    rng = np.random.default_rng(8192)
    ps = oracle.PluginSet()
    n, p = 8192, 20_000
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc = rng.integers(0, 6, (1, n)).astype(np.int64)
    used0 = rng.integers(0, 3, (1, n)).astype(np.int64)
    used = start(ctx, msh, ps, u, nd, alloc, used0)
    check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, np.ones((1, p), np.int64), None,
              "identity at size", ref=R.via_oracle)


def test_device_entry_point_on_two_streams(msh, oracle, ctx):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(31)
    ps = oracle.PluginSet(weights=[3], normalize=[1])
    n, p, h = 600, 300, 150
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, req = rand_amounts(rng, 3, n, p)
    used = start(ctx, msh, ps, u, nd, alloc)
    wi, ws, wst, cnt, us = R.per_pod(oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req)
    dev = torch.device("cuda:0")
    outs, keep = [], []
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for k, st in enumerate(streams):  # the second launch is ordered behind the first by the library
        a, b = k * h, (k + 1) * h
        d_pd, d_pt = torch.from_numpy(pd[a:b].copy()).to(dev), torch.from_numpy(pt[a:b].copy()).to(dev)
        d_rq = torch.from_numpy(np.ascontiguousarray(req[:, a:b])).to(dev)
        oi = torch.full((h,), -7, dtype=torch.int32, device=dev)
        osc = torch.full((h,), -7, dtype=torch.int64, device=dev)
        ost = torch.full((h,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        keep.append((d_pd, d_pt, d_rq))
        outs.append((oi, osc, ost))
    for k, st in enumerate(streams):
        d_pd, d_pt, d_rq = keep[k]
        oi, osc, ost = outs[k]
        ctx.schedule_sequential_fit_device(h, d_pd.data_ptr(), d_pt.data_ptr(), 3, d_rq.data_ptr(), 0, oi.data_ptr(),
                                           osc.data_ptr(), ost.data_ptr(), st.cuda_stream)
    for st in streams:
        st.synchronize()
    got = [np.concatenate([outs[k][q].cpu().numpy() for k in range(2)]) for q in range(3)]
    same(got, (wi, ws, wst), "two streams")
    assert np.array_equal(ctx.node_pod_counts(), cnt) and np.array_equal(ctx.node_resources()[1], us)


def test_errors_and_refusals(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(3)
    with msh.DeviceContext(0) as fresh:
        with pytest.raises(msh.MshError) as ei:  # before msh_upload_nodes
            fresh.upload_node_resources(np.zeros((1, 0), np.int64))
        assert ei.value.code == E.MSH_ERR_STATE
    ps = oracle.PluginSet()
    n, p = 50, 40
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, req = rand_amounts(rng, 2, n, p)
    set_plugins(ctx, msh, ps)
    ctx.upload_nodes(u, nd)

    def refused(code, fn, *a, **kw):
        with pytest.raises(msh.MshError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code, ei.value
        return str(ei.value)

    one = np.ones((2, n), np.int64)
    for bad in (np.ones((2, n - 1)), np.ones((2, n + 1)), np.ones((5, n)), -one, one * 2**62 + 1):
        refused(E.MSH_ERR_INVALID, ctx.upload_node_resources, bad.astype(np.int64))
        assert ctx.node_resources() is None
    refused(E.MSH_ERR_INVALID, ctx.upload_node_resources, one, -one)
    ctx.upload_node_resources(np.full((2, n), 2**62), np.full((2, n), 2**62))  # the range's ends are inside
    used = start(ctx, msh, ps, u, nd, alloc)
    cnt, used = check_fit(ctx, oracle, u, nd, pd, pt, ps, R.no_limit(n), alloc, used, req, None, "before the refusals")

    def unchanged(what):
        a, b = ctx.node_resources()
        assert np.array_equal(a, alloc) and np.array_equal(b, used) and np.array_equal(ctx.node_pod_counts(), cnt), what

    two = np.ones((2, 2), np.int64)
    for idx, kw in (([1, 1], dict(alloc=two)), ([0, n], dict(alloc=two)), ([-1, 0], dict(used=two)),
                    ([0, 1], dict(alloc=-two)), ([0, 1], dict(used=two * 2**62 + 1)), ([0, 1], dict())):
        refused(E.MSH_ERR_INVALID, ctx.patch_node_resources, idx, **kw)
        unchanged(f"patch {idx} {list(kw)}")
    refused(E.MSH_ERR_INVALID, ctx.schedule_sequential_fit, pd, pt, req[:1])                      # nres != the table's
    refused(E.MSH_ERR_INVALID, ctx.schedule_sequential_fit, pd, pt, np.ones((5, p), np.int64))    # nres outside 1..4
    refused(E.MSH_ERR_INVALID, ctx.schedule_sequential_fit, pd, pt, -req - 1)                     # a negative request
    refused(E.MSH_ERR_INVALID, ctx.schedule_sequential_fit, pd, pt, req + 2**62 + 1)
    unchanged("argument errors")
    ctx.set_tiebreak("random", 11, 5)
    assert "msh_schedule_sequential_fit" in refused(E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, pd, pt, req)
    assert ctx.tiebreak() == (E.MSH_TIEBREAK_RANDOM, 11, 5)
    ctx.set_tiebreak("first")
    unchanged("RANDOM")
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig("NodeNumber"), msh.ScorePluginConfig("ScoreColumn0")])
    refused(E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_fit, pd, pt, req)
    set_plugins(ctx, msh, ps)
    unchanged("score column")


def test_existing_calls_ignore_the_table(msh, oracle, ctx):
    rng = np.random.default_rng(8)
    ps = oracle.PluginSet(weights=[3], normalize=[3])
    n, p = 700, 400
    u, nd, pd, pt = rand_case(rng, n, p)
    set_plugins(ctx, msh, ps)
    results = []
    cap = rng.integers(0, 4, n)
    for table in (False, True):
        ctx.upload_nodes(u, nd)
        if table:
            ctx.upload_node_resources(np.zeros((2, n), np.int64))  # nothing would fit a request
        out = [ctx.schedule_batch(pd, pt)]
        for scalar in (0, 2):
            ctx.reset_node_pod_counts()
            out.append(ctx.schedule_sequential(pd, pt, scalar))
            out.append((ctx.node_pod_counts(),))
        ctx.reset_node_pod_counts()
        ctx.upload_node_capacity(cap)
        out.append(ctx.schedule_sequential(pd, pt, 0))
        out.append((ctx.node_pod_counts(),))
        if table:
            assert ctx.node_resources()[1].sum() == 0
        results.append(out)
    for a, b in zip(*results):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_scheduler_with_resources(msh, oracle):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    rng = np.random.default_rng(12)
    n, p = 12, 60
    cpus, mems = rng.integers(0, 5, n), rng.integers(0, 5, n)
    nodes = [{"metadata": {"name": f"node{i}"}, "spec": {"unschedulable": bool(i % 5 == 0)},
              "status": {"allocatable": ({"cpu": str(cpus[i]), "memory": f"{mems[i]}Gi"} if i % 4 else {"cpu": f"{cpus[i] * 1000}m"})}}
             for i in range(n)]
    rc, rm = rng.integers(0, 3, p), rng.integers(0, 3, p)
    pods = [{"metadata": {"name": f"pod{j}"},
             "spec": {"containers": [{"resources": {"requests": {"cpu": f"{rc[j] * 500}m", "memory": f"{rm[j] * 512}Mi"}}}],
                      "tolerations": ([{"key": "node.kubernetes.io/unschedulable", "operator": "Exists", "effect": "NoSchedule"}]
                                      if j % 3 == 0 else [])}} for j in range(p)]
    s = msh.Scheduler(resources=("cpu", "memory"))
    try:
        res = s.schedule_sequential(pods, nodes)
        nt = s.nodes
        pos = {nm: k for k, nm in enumerate(nt.names)}
        alloc = np.zeros((2, n), np.int64)
        for i in range(n):
            alloc[0, pos[f"node{i}"]] = cpus[i] * 1000
            alloc[1, pos[f"node{i}"]] = mems[i] * 2**30 if i % 4 else 0
        req = np.array([rc * 500, rm * 512 * 2**20], np.int64)
        pt = np.array([1 if j % 3 == 0 else 0 for j in range(p)], np.uint8)
        pdig = np.array([int(f"pod{j}"[-1]) for j in range(p)], np.int8)
        wi, ws, wst, cnt, us = R.serial(oracle, nt.unsched, nt.digit, pdig, pt, oracle.PluginSet(), R.no_limit(n), alloc,
                                       np.zeros_like(alloc), req)
        assert [int(r.outcome) for r in res] == wst.tolist()
        assert [r.node_index for r in res] == wi.tolist() and [r.score for r in res] == ws.tolist()
        assert (wst == R.FIT_ERROR).any() and (wst == R.PLACED).any()
        a, b = s.ctx.node_resources()
        assert np.array_equal(a, alloc) and np.array_equal(b, us) and np.array_equal(s.ctx.node_pod_counts(), cnt)
    finally:
        s.close()
