"""The CPU references of pod topology spread in sequential-commit mode (tests/spread_ref.py) against the
references they extend, hand-worked placements, the skew invariant, and the random sweep's generator: by the
reference alone it must produce cases in which the spread conjunct decides, so that the GPU sweep
(tests/test_spread_gpu.py) cannot pass on trivial inputs. The ABI's new symbols are checked for presence here too."""
from __future__ import annotations

import numpy as np

import node_capacity_ref as CR
import resource_fit_ref as R
import spread_ref as S

SWEEP_SEEDS = range(7000, 7040)


def rand_case(rng, n, p):
    u = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, 10, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return u, nd, pd, pt


def test_new_symbols_are_declared_and_bound(msh):
    names = ["msh_upload_node_zones", "msh_clear_node_zones", "msh_node_zones", "msh_set_spread_groups",
             "msh_get_spread_groups", "msh_spread_counts", "msh_patch_spread_counts", "msh_reset_spread_counts",
             "msh_seq_spread_max_nodes", "msh_schedule_sequential_spread", "msh_schedule_sequential_spread_device"]
    lib = msh._native.lib()
    for nm in names:
        assert nm in msh._native.EXPORTED and hasattr(lib, nm), nm
    assert msh._native.MAX_ZONES == S.MAX_ZONES == 64 and msh._native.MAX_SPREAD_GROUPS == 128
    # argument checks that need no device: a NULL ctx is MSH_ERR_INVALID
    inv = msh._native.MSH_ERR_INVALID
    assert lib.msh_upload_node_zones(None, 0, None) == inv
    assert lib.msh_set_spread_groups(None, 0, None) == inv
    assert lib.msh_spread_counts(None, None) == inv
    assert lib.msh_seq_spread_max_nodes(None, 0, None) == inv
    assert lib.msh_schedule_sequential_spread(None, 0, None, None, None, 0, None, 0, None, None, None,
                                              msh._native.COMMIT_CB(), None) == inv
    assert lib.msh_schedule_sequential_spread_device(None, 0, None, None, None, 0, None, 0, None, None, None, None) == inv


def test_ungrouped_equals_the_resource_fit_and_capacity_references(oracle):
    rng = np.random.default_rng(1)
    for case in range(12):
        n, p = int(rng.integers(1, 40)), int(rng.integers(0, 60))
        u, nd, pd, pt = rand_case(rng, n, p)
        ps = oracle.PluginSet(weights=[int(rng.choice([1, 3]))], normalize=[case % 4])
        zone = rng.integers(-1, 4, n)
        grp = np.full(p, -1)
        eff = rng.integers(0, 4, n).astype(np.int64)
        nres = 1 + case % 4
        alloc = rng.integers(0, 9, (nres, n)).astype(np.int64)
        used = rng.integers(0, 3, (nres, n)).astype(np.int64)
        req = rng.integers(0, 4, (nres, p)).astype(np.int64)
        want = R.serial(oracle, u, nd, pd, pt, ps, eff, alloc, used, req)
        for ref in (S.serial, S.per_pod):
            got = ref(oracle, u, nd, pd, pt, ps, eff, alloc, used, req, zone, grp, [1, 2])
            assert all(np.array_equal(a, b) for a, b in zip(got[:5], want)) and not got[5].any()
        a0, u0, r0 = S.no_res(n, p)
        want = CR.serial(oracle, u, nd, pd, pt, ps, eff)
        for ref in (S.serial, S.per_pod):
            got = ref(oracle, u, nd, pd, pt, ps, eff, a0, u0, r0, zone, grp, [])
            assert all(np.array_equal(a, b) for a, b in zip(got[:4], want))


def test_per_pod_equals_serial(oracle):
    rng = np.random.default_rng(2)
    for case in range(30):
        n, p = int(rng.integers(1, 60)), int(rng.integers(0, 120))
        u, nd, pd, pt = rand_case(rng, n, p)
        ps = oracle.PluginSet(["NodeUnschedulable"] if case % 5 else [], ["NodeNumber"] if case % 7 else [],
                              ["NodeNumber"], [int(rng.choice([1, 3, 2**32]))], [case % 4])
        nz = int(rng.choice([1, 2, 3, 8]))
        zone = rng.integers(-1 if case % 3 else 0, nz, n)
        if case == 4:
            zone[:] = -1
        G = int(rng.choice([1, 2, 5]))
        grp = rng.integers(-3, G + 2, p)  # values outside [0, G) count as ungrouped
        skew = rng.choice([1, 2, S.INT32_MAX], G)
        eff = rng.integers(0, 6, n).astype(np.int64) if case % 2 else S.no_limit(n)
        nres = case % 3
        alloc = rng.integers(0, 9, (nres, n)).astype(np.int64)
        used = np.zeros((nres, n), np.int64)
        req = rng.integers(0, 3, (nres, p)).astype(np.int64)
        cnt0 = rng.integers(0, 3, (G, S.MAX_ZONES)) if case % 4 == 0 else None
        a = S.serial(oracle, u, nd, pd, pt, ps, eff, alloc, used, req, zone, grp, skew, None, cnt0)
        b = S.per_pod(oracle, u, nd, pd, pt, ps, eff, alloc, used, req, zone, grp, skew, None, cnt0)
        for x, y, name in zip(a, b, ("idx", "score", "status", "counts", "used", "cnt")):
            assert np.array_equal(x, y), f"case {case}: {name}"


def spread(oracle, zone, grp, skew, eff=None, u=None, pt=None, ps=None):
    n, p = len(zone), len(grp)
    a0, u0, r0 = S.no_res(n, p)
    ps = ps or oracle.PluginSet(score=[], weights=[], normalize=[])  # no score: the first feasible node
    return S.serial(oracle, np.zeros(n, np.uint8) if u is None else u, np.zeros(n, np.int8), np.zeros(p, np.int8),
                    np.zeros(p, np.uint8) if pt is None else pt, ps, S.no_limit(n) if eff is None else eff, a0, u0, r0,
                    zone, grp, skew)


def test_three_zones_max_skew_one(oracle):
    # nodes 0,1 in zone 0; 2,3 in zone 1; 4 in zone 2: the first feasible node, and a zone may lead by one only
    idx, _, st, counts, _, cnt = spread(oracle, [0, 0, 1, 1, 2], [0] * 7, [1])
    assert idx.tolist() == [0, 2, 4, 0, 2, 4, 0] and not st.any()
    assert cnt[0, :3].tolist() == [3, 2, 2] and counts.tolist() == [3, 0, 2, 0, 2]
    # a second group has its own counts; ungrouped pods go to node 0 whatever the counts say
    idx, _, st, _, _, cnt = spread(oracle, [0, 0, 1, 1, 2], [0, 1, -1, 0, 1, -1], [1, 1])
    assert idx.tolist() == [0, 0, 0, 2, 2, 0]
    assert cnt[:, :3].tolist() == [[1, 1, 0], [1, 1, 0]]
    # max_skew 2: zones 0 and 1 each take two while zone 2 is empty, then zone 2 must catch up
    assert spread(oracle, [0, 0, 1, 1, 2], [0] * 6, [2])[0].tolist() == [0, 0, 2, 2, 4, 0]


def test_a_full_zone_pins_the_minimum(oracle):
    # zone 1's only node takes one pod: after it fills, zone 1 stays at 1, zone 0 may reach 2, then nothing fits
    eff = np.array([9, 9, 1], np.int64)
    idx, _, st, _, _, cnt = spread(oracle, [0, 0, 1], [0] * 6, [1], eff=eff)
    assert idx.tolist() == [0, 2, 0, -1, -1, -1]
    assert st.tolist() == [0, 0, 0, S.FIT_ERROR, S.FIT_ERROR, S.FIT_ERROR] and cnt[0, :2].tolist() == [2, 1]
    # the same with the zone cordoned from the start: the minimum is pinned at 0 (Zset ignores cordons)
    u = np.array([0, 0, 1], np.uint8)
    ps = oracle.PluginSet(score=[], weights=[], normalize=[])
    idx, _, st, _, _, _ = spread(oracle, [0, 0, 1], [0, 0, -1, 0], [1], u=u, ps=ps)
    assert idx.tolist() == [0, -1, 0, -1] and st.tolist() == [0, S.FIT_ERROR, 0, S.FIT_ERROR]


def test_a_node_without_a_zone(oracle):
    idx, _, st, _, _, cnt = spread(oracle, [-1, 0, -1, 1], [0, -1, 0, 0], [1])
    assert idx.tolist() == [1, 0, 3, 1] and not st.any() and cnt[0, :2].tolist() == [2, 1]
    # no node has a zone: Zset is empty, no grouped pod fits, ungrouped ones do
    idx, _, st, _, _, cnt = spread(oracle, [-1, -1], [0, -1, 0], [5])
    assert idx.tolist() == [-1, 0, -1] and st.tolist() == [S.FIT_ERROR, 0, S.FIT_ERROR] and not cnt.any()


def test_skew_invariant_after_every_commit(oracle):
    rng = np.random.default_rng(3)
    for case in range(8):
        n, p = 30, 150
        u, nd, pd, pt = rand_case(rng, n, p)
        zone = rng.integers(-1, 4, n)
        zs = S.zset(zone)
        G = 3
        skew = rng.choice([1, 2, 4], G)
        grp = rng.integers(-1, G, p)
        eff = rng.integers(0, 8, n).astype(np.int64)
        a0, u0, r0 = S.no_res(n, p)
        ps = oracle.PluginSet()
        cnt = counts = None
        for j in range(p):  # one pod per call: the state after every commit
            _, _, st, counts, _, cnt = S.serial(oracle, u, nd, pd[j:j + 1], pt[j:j + 1], ps, eff, a0, u0, r0[:, :1],
                                                zone, grp[j:j + 1], skew, counts, cnt)
            for g in range(G):
                assert cnt[g].max() - cnt[g][zs].min() <= skew[g], (case, j, g)


def sweep_inputs(c, ungrouped=False):
    eff = CR.effective(c["cap"])
    grp = np.full(c["p"], -1, np.int32) if ungrouped else c["group"]
    return (c["unsched"], c["node_digit"], c["pod_digit"], c["pod_tol"]), eff, (c["alloc"], np.zeros_like(c["alloc"]),
                                                                                 c["req"]), (c["zone"], grp, c["max_skew"])


def test_the_sweep_generator_makes_spread_decide(oracle):
    moved = new_fit_error = 0
    for seed in SWEEP_SEEDS:
        c = S.gen_case(seed)
        assert c["n"] <= 2048 and c["p"] <= 2000
        ps = oracle.PluginSet(weights=[c["weight"]], normalize=[c["mode"]])
        cols, eff, res, sp = sweep_inputs(c)
        wi, _, wst, *_ = S.per_pod(oracle, *cols, ps, eff, *res, *sp)
        cols, eff, res, sp = sweep_inputs(c, ungrouped=True)
        zi, _, zst, *_ = S.per_pod(oracle, *cols, ps, eff, *res, *sp)
        moved += bool((wi != zi).any())
        new_fit_error += bool(((wst == S.FIT_ERROR) & (zst != S.FIT_ERROR)).any())
    total = len(SWEEP_SEEDS)
    assert 2 * moved >= total, f"{moved} of {total} cases place a pod differently from the ungrouped call"
    assert 4 * new_fit_error >= total, f"{new_fit_error} of {total} cases have a FIT_ERROR the ungrouped call lacks"
