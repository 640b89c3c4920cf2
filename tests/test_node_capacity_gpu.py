"""Per-node pod capacity in sequential-commit mode on the GPU (msh_upload_node_capacity and friends).

Every comparison is bit-exact on idx, score, status and node_pod_counts(). The expected values come from
tests/node_capacity_ref.py: the unchanged C oracle through the uniform-capacity identity (`via_oracle`), or
the plain serial loop (`serial`) for tiny shapes and INT32_MAX capacities. tests/test_node_capacity.py checks
on the CPU that the two agree."""
from __future__ import annotations

import numpy as np
import pytest

import node_capacity_ref as R

pytestmark = pytest.mark.gpu
INT32_MAX = R.INT32_MAX
P = 300


def rand_case(rng, n, p, p_unsched=0.3, digits=10):
    u = (rng.random(n) < p_unsched).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, digits, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return u, nd, pd, pt


def set_plugins(ctx, msh, ps):
    ctx.set_plugins(ps.filters, ps.prescore,
                    [msh.ScorePluginConfig(s, w, msh.Normalize(m)) for s, w, m in zip(ps.score, ps.weights, ps.normalize)])


def same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "score", "status")):
        assert np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(np.asarray(g) != np.asarray(w))[:5]}"


def check_call(ctx, O, u, nd, pd, pt, ps, cap, scalar, before, what, ref=R.via_oracle):
    """One sequential call with the column `cap` on the device; returns the expected counts after it."""
    got = ctx.schedule_sequential(pd, pt, scalar)
    wi, ws, wst, after = ref(O, u, nd, pd, pt, ps, R.effective(cap, scalar), before)
    same(got, (wi, ws, wst), what)
    assert np.array_equal(ctx.node_pod_counts(), after), f"{what}: counts"
    return after


@pytest.fixture(scope="module")
def ctxs(msh):
    """One context per msh_options.seq_waves value, shared by the tests of this file (each test uploads its
    own nodes, which zeroes the counts and drops the column)."""
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    made = {w: msh.DeviceContext(0, {"seq_waves": w}) for w in (0, 1, 4, 16)}
    yield made
    for c in made.values():
        c.close()


# 31 / 33 nodes: around one word; 100: several words in one lane group; 2,100: more than one word per lane on
# one wave (66 words over 64 lanes). Every count is forced at every size: seq_capn_kernel (1) and the 4- and
# 16-wave seq_node_kernel instances, counts in LDS (4) and in device memory (16).
@pytest.mark.parametrize("n", [31, 33, 100, 2100])
@pytest.mark.parametrize("waves", [1, 4, 16])
@pytest.mark.parametrize("norm", [0, 3])  # the identity-like and the KX instances
def test_every_kernel_form(msh, oracle, ctxs, waves, n, norm):
    rng = np.random.default_rng(1000 * waves + n + norm)
    ps = oracle.PluginSet(weights=[3], normalize=[norm])
    ctx = ctxs[waves]
    set_plugins(ctx, msh, ps)
    u, nd, pd, pt = rand_case(rng, n, P)
    cap = rng.choice([0, 1, 2, 3, 10**6], n)
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    k = check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, None, f"waves={waves} n={n}")
    check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 2, k, f"waves={waves} n={n} second call, scalar 2")


# Automatic choice (msh_seq.hip, seq_waves_for: one wave while the padded table has at most 16 words per lane,
# 32,768 nodes; then 16 waves). The counts leave LDS with the 16-wave form (msh_seq_kernel.h, seq_body:
# `constexpr bool LDSC = NW <= 4`), so one node past 32,768 is also the first table whose remaining capacities
# live in device memory; 131,073 nodes is the first at 8 words per lane (launch_seq_nw: `if (rs <= 4)`).
@pytest.mark.parametrize("n", [32_768, 32_769, 131_073])
def test_automatic_forms_at_their_thresholds(msh, oracle, ctxs, n):
    rng = np.random.default_rng(n)
    ps = oracle.PluginSet()
    ctx = ctxs[0]
    set_plugins(ctx, msh, ps)
    u, nd, pd, pt = rand_case(rng, n, P)
    cap = rng.choice([0, 1, 2, 3, 10**6], n)
    nd[: n - 40][nd[: n - 40] == 7] = 8  # digit 7 only in the last words of the table
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    k = check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, None, f"auto n={n}")
    check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, k, f"auto n={n} second call")


@pytest.mark.parametrize("p", [0, 1, 3, 63, 64, 65, 257])
@pytest.mark.parametrize("waves", [1, 4, 16])
def test_fills_inside_one_step(msh, oracle, ctxs, waves, p):
    """Capacity 1 everywhere and one digit for all pods: every commit fills the node the next pod of the same
    step predicted. Then capacities from {0, 1, 2, 3, 10^6}."""
    rng = np.random.default_rng(p)
    ps = oracle.PluginSet()
    ctx = ctxs[waves]
    set_plugins(ctx, msh, ps)
    n = 200
    u, nd, _, pt = rand_case(rng, n, p, p_unsched=0.1)
    pd = np.full(p, 4, np.int8)
    for cap in (np.ones(n, np.int64), rng.choice([0, 1, 2, 3, 10**6], n)):
        ctx.upload_nodes(u, nd)
        ctx.upload_node_capacity(cap)
        check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, None, f"fills waves={waves} p={p}")


@pytest.mark.parametrize("waves", [1, 4, 16])
def test_exhaustion_per_tolerates_class(msh, oracle, ctxs, waves):
    """Total capacity below p: the schedulable nodes run out first, so pods that do not tolerate end in
    MSH_FIT_ERROR while tolerating ones still land on the unschedulable nodes, then those run out too."""
    rng = np.random.default_rng(waves)
    ps = oracle.PluginSet()
    ctx = ctxs[waves]
    set_plugins(ctx, msh, ps)
    n = 70
    u, nd, pd, pt = rand_case(rng, n, P, p_unsched=0.4)
    cap = rng.integers(0, 5, n)
    assert cap.sum() < P and cap[u == 1].sum() > 0
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    want_st = R.via_oracle(oracle, u, nd, pd, pt, ps, cap)[2]
    first_fit = int(np.flatnonzero((want_st == R.FIT_ERROR) & (pt == 0))[0])
    # the case is what it says: a pod that does not tolerate finds nothing while a later tolerating pod is placed
    assert ((want_st[first_fit:] == R.PLACED) & (pt[first_fit:] == 1)).any() and want_st[-1] == R.FIT_ERROR
    after = check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, None, f"exhaustion waves={waves}")
    assert (after <= cap).all()
    check_call(ctx, oracle, u, nd, pd[:10], pt[:10], ps, cap, 0, after, "on the exhausted table")


PLUGIN_SPACE = ([(["NodeUnschedulable"], ["NodeNumber"], ["NodeNumber"], w, m) for m in (0, 1, 2, 3) for w in (1, 3, 2**32)]
                + [(["NodeUnschedulable"], [], ["NodeNumber"], 1, m) for m in (0, 2)]  # score errors commit nothing
                + [([], ["NodeNumber"], ["NodeNumber"], 1, m) for m in (0, 3)]         # no NodeUnschedulable filter
                + [(["NodeUnschedulable"], ["NodeNumber"], [], None, None)])


@pytest.mark.parametrize("waves", [1, 16])
@pytest.mark.parametrize("combo", PLUGIN_SPACE, ids=lambda c: f"{len(c[0])}{len(c[1])}{len(c[2])}w{c[3]}m{c[4]}")
def test_plugin_space(msh, oracle, ctxs, combo, waves):
    f, pre, sc, w, m = combo
    rng = np.random.default_rng(17)
    ps = oracle.PluginSet(f, pre, sc, [w] if sc else [], [m] if sc else [])
    ctx = ctxs[waves]
    set_plugins(ctx, msh, ps)
    n = 150
    u, nd, pd, pt = rand_case(rng, n, P)  # pods without a digit included
    cap = rng.choice([0, 1, 2, 3, 10**6], n)
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    k = check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, None, f"plugins {combo} waves={waves}")
    if not pre and sc:
        assert k.sum() == 0  # every pod with a feasible node ends in MSH_SCORE_ERROR: nothing committed


def test_tiny_shapes_and_int32_max_against_the_serial_loop(msh, oracle, ctxs):
    rng = np.random.default_rng(5)
    ctx = ctxs[0]
    for n, p, norm in ((1, 5, 0), (3, 17, 2), (12, 40, 3), (40, 90, 1)):
        ps = oracle.PluginSet(weights=[2**32], normalize=[norm])
        set_plugins(ctx, msh, ps)
        u, nd, pd, pt = rand_case(rng, n, p)
        cap = rng.choice([0, 1, 2, INT32_MAX], n)
        ctx.upload_nodes(u, nd)
        ctx.upload_node_capacity(cap)
        assert np.array_equal(ctx.node_capacity(), cap)
        k = check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, None, f"tiny n={n}", ref=R.serial)
        check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 3, k, f"tiny n={n} scalar 3", ref=R.serial)


@pytest.mark.parametrize("waves", [1, 4, 16])
def test_scalar_and_column_together(msh, oracle, ctxs, waves):
    rng = np.random.default_rng(waves + 40)
    ps = oracle.PluginSet()
    ctx = ctxs[waves]
    set_plugins(ctx, msh, ps)
    n = 120
    u, nd, pd, pt = rand_case(rng, n, P)
    cap = rng.integers(0, 7, n)
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    after = check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 3, None, f"min(cap, 3) waves={waves}")
    assert after.max() <= 3 and (after <= cap).all()
    # a uniform column M with scalar 0 is today's scalar call with M, bit for bit, counts included
    for m in (1, 4):
        ctx.upload_nodes(u, nd)
        ctx.upload_node_capacity(np.full(n, m))
        a = ctx.schedule_sequential(pd, pt, 0)
        ca = ctx.node_pod_counts()
        ctx.upload_nodes(u, nd)  # drops the column
        b = ctx.schedule_sequential(pd, pt, m)
        same(a, b, f"uniform column {m} against the scalar")
        assert np.array_equal(ca, ctx.node_pod_counts())
        want = oracle.c_schedule_sequential(u, nd, pd, pt, ps, m)
        same(b, want[:3], f"scalar {m} against the oracle")


@pytest.mark.parametrize("waves", [1, 4, 16])
def test_carry_over_patches_and_lifetime(msh, oracle, ctxs, waves):
    rng = np.random.default_rng(waves + 70)
    ps = oracle.PluginSet()
    ctx = ctxs[waves]
    set_plugins(ctx, msh, ps)
    n = 90
    u, nd, pd, pt = rand_case(rng, n, P)
    cap = rng.integers(1, 6, n)
    ctx.upload_nodes(u, nd)
    assert ctx.node_capacity() is None
    ctx.upload_node_capacity(cap)
    k = check_call(ctx, oracle, u, nd, pd[:100], pt[:100], ps, cap, 0, None, "first call")
    k = check_call(ctx, oracle, u, nd, pd[100:150], pt[100:150], ps, cap, 0, k, "second call, carried counts")
    # lower two nodes that hold pods to and below their counts: full for the next call; raise another
    held = np.flatnonzero(k > 0)[:2]
    room = np.setdiff1d(np.flatnonzero(k == cap), held)[:1]  # a full node, given two more slots
    assert len(held) == 2 and len(room) == 1
    cap = cap.copy()
    cap[held[0]], cap[held[1]], cap[room[0]] = k[held[0]], max(k[held[1]] - 1, 0), cap[room[0]] + 2
    ctx.patch_node_capacity(np.concatenate([held, room]), cap[np.concatenate([held, room])])
    assert np.array_equal(ctx.node_capacity(), cap)
    k2 = check_call(ctx, oracle, u, nd, pd[150:200], pt[150:200], ps, cap, 0, k, "after the patch")
    assert (k2[held] == k[held]).all()
    cap[held] += 3  # raised: available again
    ctx.patch_node_capacity(held, cap[held])
    k = check_call(ctx, oracle, u, nd, pd[200:250], pt[200:250], ps, cap, 0, k2, "after raising")
    # msh_patch_nodes keeps the column (and the counts)
    u = u.copy()
    flip = np.arange(0, n, 7, dtype=np.int32)
    u[flip] ^= 1
    ctx.patch_nodes(flip, u[flip], nd[flip])
    assert np.array_equal(ctx.node_capacity(), cap)
    k = check_call(ctx, oracle, u, nd, pd[250:], pt[250:], ps, cap, 0, k, "after msh_patch_nodes")
    # msh_reset_node_pod_counts keeps it too
    ctx.reset_node_pod_counts()
    assert np.array_equal(ctx.node_capacity(), cap)
    check_call(ctx, oracle, u, nd, pd[:80], pt[:80], ps, cap, 0, None, "after the reset")
    # msh_upload_nodes drops it: the next call is the call without a column; so does msh_clear_node_capacity
    ctx.upload_nodes(u, nd)
    assert ctx.node_capacity() is None
    got = ctx.schedule_sequential(pd, pt, 0)
    want = oracle.c_schedule_sequential(u, nd, pd, pt, ps, 0)
    same(got, want[:3], "after msh_upload_nodes")
    assert np.array_equal(ctx.node_pod_counts(), want[3])
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    ctx.clear_node_capacity()
    assert ctx.node_capacity() is None
    got = ctx.schedule_sequential(pd, pt, 2)
    want = oracle.c_schedule_sequential(u, nd, pd, pt, ps, 2)
    same(got, want[:3], "after msh_clear_node_capacity")
    assert np.array_equal(ctx.node_pod_counts(), want[3])
    with pytest.raises(msh.MshError) as ei:
        ctx.patch_node_capacity([0], [1])
    assert ei.value.code == msh._native.MSH_ERR_STATE


def test_both_entry_points(msh, oracle, ctxs):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(91)
    ps = oracle.PluginSet(weights=[3], normalize=[1])
    ctx = ctxs[0]
    set_plugins(ctx, msh, ps)
    n = 500
    u, nd, pd, pt = rand_case(rng, n, P)
    cap = rng.choice([0, 1, 2, 3, 10**6], n)
    wi, ws, wst, after = R.via_oracle(oracle, u, nd, pd, pt, ps, cap)
    # the host-buffer call replays commit_cb in placement order, once per placed pod
    ctx.upload_nodes(u, nd)
    ctx.upload_node_capacity(cap)
    seen = []
    got = ctx.schedule_sequential(pd, pt, 0, on_commit=lambda j, i, s: seen.append((j, i, s)))
    same(got, (wi, ws, wst), "host-buffer call")
    assert seen == [(j, int(wi[j]), int(ws[j])) for j in range(P) if wst[j] == 0]
    # the _device call on a stream of the caller's
    ctx.reset_node_pod_counts()
    dev = torch.device("cuda:0")
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    oi = torch.full((P,), -7, dtype=torch.int32, device=dev)
    osc = torch.full((P,), -7, dtype=torch.int64, device=dev)
    ost = torch.full((P,), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ctx.schedule_sequential_device(P, d_pd.data_ptr(), d_pt.data_ptr(), 0, oi.data_ptr(), osc.data_ptr(),
                                       ost.data_ptr(), st.cuda_stream)
    st.synchronize()
    same((oi.cpu().numpy(), osc.cpu().numpy(), ost.cpu().numpy()), (wi, ws, wst), "_device call")
    assert np.array_equal(ctx.node_pod_counts(), after)


def test_errors(msh, oracle, ctxs):
    E = msh._native
    rng = np.random.default_rng(3)
    with msh.DeviceContext(0) as fresh:
        with pytest.raises(msh.MshError) as ei:  # before msh_upload_nodes
            fresh.upload_node_capacity(np.zeros(0, np.int32))
        assert ei.value.code == E.MSH_ERR_STATE
    ctx = ctxs[0]
    ps = oracle.PluginSet()
    set_plugins(ctx, msh, ps)
    n = 50
    u, nd, pd, pt = rand_case(rng, n, 40)
    ctx.upload_nodes(u, nd)
    for bad in (np.ones(n - 1), np.ones(n + 1), np.r_[np.ones(n - 1), -1]):
        with pytest.raises(msh.MshError) as ei:
            ctx.upload_node_capacity(bad.astype(np.int64))
        assert ei.value.code == E.MSH_ERR_INVALID and ctx.node_capacity() is None
    cap = np.full(n, 2)
    ctx.upload_node_capacity(cap)
    for idx, val in (([1, 1], [3, 3]), ([n], [3]), ([-1], [3]), ([0], [-2])):
        with pytest.raises(msh.MshError) as ei:
            ctx.patch_node_capacity(idx, val)
        assert ei.value.code == E.MSH_ERR_INVALID
    assert np.array_equal(ctx.node_capacity(), cap)
    # RANDOM tie-break and a score-column list stay refused with a column present; nothing moves
    k = check_call(ctx, oracle, u, nd, pd, pt, ps, cap, 0, None, "before the refusals")
    ctx.set_tiebreak("random", 11, 5)
    with pytest.raises(msh.MshError) as ei:
        ctx.schedule_sequential(pd, pt, 0)
    assert ei.value.code == E.MSH_ERR_UNSUPPORTED
    assert ctx.tiebreak() == (E.MSH_TIEBREAK_RANDOM, 11, 5) and np.array_equal(ctx.node_pod_counts(), k)
    ctx.set_tiebreak("first")
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig("NodeNumber"), msh.ScorePluginConfig("ScoreColumn0")])
    with pytest.raises(msh.MshError) as ei:
        ctx.schedule_sequential(pd, pt, 0)
    assert ei.value.code == E.MSH_ERR_UNSUPPORTED and np.array_equal(ctx.node_pod_counts(), k)
    set_plugins(ctx, msh, ps)
    assert np.array_equal(ctx.node_capacity(), cap)
    # the capacity form's table limit applies as soon as a column is present
    big = 262_145
    zu, zd = np.zeros(big, np.uint8), np.zeros(big, np.int8)
    ctx.upload_nodes(zu, zd)
    same(ctx.schedule_sequential(pd, pt, 0), oracle.c_schedule_sequential(zu, zd, pd, pt, ps, 0)[:3],
         "no column: 368,640 nodes fit")
    ctx.upload_node_capacity(np.full(big, 5))
    with pytest.raises(msh.MshError) as ei:
        ctx.schedule_sequential(pd, pt, 0)
    assert ei.value.code == E.MSH_ERR_UNSUPPORTED and "262144 nodes per device with a capacity" in str(ei.value)


def test_batch_entry_points_ignore_the_column(msh, oracle, ctxs):
    rng = np.random.default_rng(8)
    ps = oracle.PluginSet()
    ctx = ctxs[0]
    set_plugins(ctx, msh, ps)
    u, nd, pd, pt = rand_case(rng, 700, 400)
    ctx.upload_nodes(u, nd)
    without = ctx.schedule_batch(pd, pt)
    ctx.upload_node_capacity(np.zeros(700, np.int32))  # no node takes a pod in sequential mode
    same(ctx.schedule_batch(pd, pt), without, "msh_schedule_batch with a column")
    assert ctx.node_pod_counts().sum() == 0  # and it commits nothing


def test_scheduler_uploads_allocatable_pods(msh, oracle):
    class Nd:
        def __init__(self, name, pods=None):
            self.name, self.unschedulable, self.allocatable_pods = name, False, pods

    class Pd:
        def __init__(self, name):
            self.name, self.tolerations = name, ()

    if msh.device_count() < 1:
        pytest.skip("no GPU")
    s = msh.Scheduler()
    try:
        nodes = [Nd("node1", 2), Nd("node2"), Nd("node11", 1)]
        res = s.schedule_sequential([Pd(f"pod{j}1") for j in range(5)], nodes)
        assert [r.node_name for r in res] == ["node1", "node1", "node11", "node2", "node2"]
        assert s.ctx.node_capacity().tolist() == [2, 1, INT32_MAX]
    finally:
        s.close()


@pytest.mark.parametrize("waves", [0, 1, 4, 16])
def test_random_sweep(msh, oracle, ctxs, waves):
    """200 cases in all (50 per seq_waves option), n <= 3,000, p <= 500: random capacities, counts built up by
    an earlier call, plugin lists and an optional scalar, from a fixed seed, against the oracle identity."""
    rng = np.random.default_rng(4000 + waves)
    ctx = ctxs[waves]
    for case in range(50):
        n, p = int(rng.integers(1, 3001)), int(rng.integers(0, 501))
        f = ["NodeUnschedulable"] if rng.random() < 0.8 else []
        pre = ["NodeNumber"] if rng.random() < 0.9 else []
        ps = oracle.PluginSet(f, pre, ["NodeNumber"], [int(rng.choice([1, 3, 2**32]))], [int(rng.integers(0, 4))])
        set_plugins(ctx, msh, ps)
        u, nd, pd, pt = rand_case(rng, n, p, p_unsched=float(rng.choice([0.0, 0.3, 0.9])), digits=int(rng.choice([2, 10])))
        kind = case % 3
        cap = (rng.integers(0, 3, n) if kind == 0 else rng.choice([0, 1, 2, 3, 10**6], n) if kind == 1
               else rng.integers(0, max(2, 2 * p // n + 2), n))
        scalar = int(rng.choice([0, 0, 1, 2, 4]))
        ctx.upload_nodes(u, nd)
        k = None
        if case % 2:  # initial counts from an earlier call under another column
            cap0 = rng.integers(0, 4, n)
            ctx.upload_node_capacity(cap0)
            p0 = p // 2
            k = check_call(ctx, oracle, u, nd, pd[:p0], pt[:p0], ps, cap0, 0, None, f"sweep {waves}/{case} warm")
        ctx.upload_node_capacity(cap)
        check_call(ctx, oracle, u, nd, pd, pt, ps, cap, scalar, k, f"sweep waves={waves} case={case} n={n} p={p}")
