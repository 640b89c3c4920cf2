"""The CPU references of topology spread together with a resource score (tests/spread_score_ref.py) against each
other and against the references they compose (spread_ref, resource_score_ref), hand-worked placements, the skew
invariant, and the random sweep's generator: by the references alone it must produce cases in which both the spread
conjunct and the score decide, so that the GPU sweep (tests/test_spread_score_gpu.py) cannot pass on trivial
inputs. The ABI's new symbols are checked for presence here too."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

import node_capacity_ref as CR
import resource_score_ref as RS
import spread_ref as S
import spread_score_ref as X

SWEEP_SEEDS = range(9000, 9040)
NEW_SYMBOLS = ["msh_seq_spread_scored_max_nodes", "msh_schedule_sequential_spread_scored",
               "msh_schedule_sequential_spread_scored_device"]


def test_new_symbols_are_declared_exported_and_bound(msh):
    header = (Path(__file__).resolve().parent.parent / "include" / "minisched_hip.h").read_text()
    lib = msh._native.lib()
    for nm in NEW_SYMBOLS:
        assert re.search(r"^int " + nm + r"\(", header, re.M), f"{nm} is not declared in the header"
        assert nm in msh._native.EXPORTED and hasattr(lib, nm), nm
    # argument checks that need no device: a NULL ctx is MSH_ERR_INVALID
    inv = msh._native.MSH_ERR_INVALID
    assert lib.msh_seq_spread_scored_max_nodes(None, 0, None) == inv
    assert lib.msh_schedule_sequential_spread_scored(None, 0, None, None, None, 0, None, 0, None, None, None,
                                                     msh._native.COMMIT_CB(), None) == inv
    assert lib.msh_schedule_sequential_spread_scored_device(None, 0, None, None, None, 0, None, 0, None, None, None,
                                                            None) == inv
    for nm in ("seq_spread_scored_max_nodes", "schedule_sequential_spread_scored",
               "schedule_sequential_spread_scored_device"):
        assert hasattr(msh.DeviceContext, nm), nm


def case_args(c, ungrouped=False):
    """gen_case's dict as the references' positional arguments up to max_skew."""
    grp = np.full(c["p"], -1, np.int32) if ungrouped else c["group"]
    return (c["unsched"], c["node_digit"], c["pod_digit"], c["pod_tol"]), CR.effective(c["cap"]), \
        (c["alloc"], np.zeros_like(c["alloc"]), c["req"]), (c["zone"], grp, c["max_skew"])


def case_plugins(oracle, c):
    return oracle.PluginSet(weights=[c["weight"]], normalize=[c["mode"]])


def test_per_pod_equals_serial_on_200_seeds(oracle):
    seen_nres, seen_zero_weight, seen_unzoned = set(), False, False
    for seed in range(200):
        c = X.gen_case(seed, max_n=40, max_p=60)
        assert 1 <= c["n"] <= 2048 and 1 <= c["nres"] <= 4 and 1 <= c["G"] <= 16
        assert 1 <= len(S.zset(c["zone"])) <= 8 or (c["zone"] < 0).all()
        assert c["max_skew"].min() >= 1 and c["max_skew"].max() <= 3
        seen_nres.add(c["nres"])
        seen_zero_weight |= 0 in c["rw"]
        seen_unzoned |= bool((c["zone"] < 0).any())
        cols, eff, res, sp = case_args(c)
        ps = case_plugins(oracle, c)
        cnt0 = np.random.default_rng(seed).integers(0, 3, (c["G"], S.MAX_ZONES)) if seed % 4 == 0 else None
        sc = (c["score_mode"], c["rs_weight"], c["rw"])
        a = X.serial(oracle, *cols, ps, eff, *res, *sp, *sc, None, cnt0)
        b = X.per_pod(oracle, *cols, ps, eff, *res, *sp, *sc, None, cnt0)
        for x, y, name in zip(a, b, ("idx", "score", "status", "counts", "used", "cnt")):
            assert np.array_equal(x, y), f"seed {seed}: {name}"
    assert seen_nres == {1, 2, 3, 4} and seen_zero_weight and seen_unzoned


def test_ungrouped_equals_the_resource_score_reference(oracle):
    for seed in range(300, 330):
        c = X.gen_case(seed, max_n=40, max_p=60)
        cols, eff, res, sp = case_args(c, ungrouped=True)
        ps = case_plugins(oracle, c)
        sc = (c["score_mode"], c["rs_weight"], c["rw"])
        want = RS.serial(oracle, *cols, ps, eff, *res, *sc)
        for ref in (X.serial, X.per_pod):
            got = ref(oracle, *cols, ps, eff, *res, *sp, *sc)
            assert all(np.array_equal(a, b) for a, b in zip(got[:5], want)) and not got[5].any(), seed


def test_mode_none_equals_the_spread_reference(oracle):
    for seed in range(400, 430):
        c = X.gen_case(seed, max_n=40, max_p=60)
        cols, eff, res, sp = case_args(c)
        ps = case_plugins(oracle, c)
        want = S.serial(oracle, *cols, ps, eff, *res, *sp)
        for ref in (X.serial, X.per_pod):
            got = ref(oracle, *cols, ps, eff, *res, *sp, X.NONE, 0, [])
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), seed


def run(oracle, zone, alloc, used, req, skew, mode, cnt=None, ref=X.serial):
    """One group, every pod in it, no NodeNumber score: the total is RS alone at weight 1."""
    n, p = len(zone), len(req)
    ps = oracle.PluginSet(score=[], weights=[], normalize=[])
    return ref(oracle, np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros(p, np.int8), np.zeros(p, np.uint8), ps,
               S.no_limit(n), np.array([alloc], np.int64), np.array([used], np.int64), np.array([req], np.int64), zone,
               np.zeros(p, np.int32), [skew], mode, 1, [1], None, cnt)


def test_the_skew_bars_the_best_scored_node(oracle):
    # nodes 0, 1 (zone 0, 100 units each) and node 2 (zone 1, 10 units); six pods of 5 units, LEAST, max_skew 1.
    # pod 0: RS 95 / 95 / 50, every zone allowed: node 0. pod 1: zone 0 stands at 1 against 0, barred; the best
    # node of zone 1 is node 2 at 50 (the scored _fit call would take node 1 at 95). pod 2: (1, 1), all allowed:
    # node 0 is at (100 - 10) = 90, node 1 at 95, node 2 at 0: node 1. pod 3: zone 0 barred; node 2 takes it at
    # (10 - 10) * 100 / 10 = 0. pod 4: (2, 2); node 2 is full, nodes 0 and 1 tie at 90: node 0. pod 5: zone 0
    # barred at (3, 2), node 2 full: FIT_ERROR, nothing committed.
    for ref in (X.serial, X.per_pod):
        idx, sc, st, counts, used, cnt = run(oracle, [0, 0, 1], [100, 100, 10], [0, 0, 0], [5] * 6, 1, X.LEAST, ref=ref)
        assert idx.tolist() == [0, 2, 1, 2, 0, -1] and sc.tolist() == [95, 50, 95, 0, 90, 0]
        assert st.tolist() == [0, 0, 0, 0, 0, X.FIT_ERROR]
        assert counts.tolist() == [2, 1, 2] and used.tolist() == [[10, 5, 10]] and cnt[0, :2].tolist() == [3, 2]
    fit = RS.serial(oracle, np.zeros(3, np.uint8), np.zeros(3, np.int8), np.zeros(6, np.int8), np.zeros(6, np.uint8),
                    oracle.PluginSet(score=[], weights=[], normalize=[]), S.no_limit(3), np.array([[100, 100, 10]]),
                    np.zeros((1, 3), np.int64), np.array([[5] * 6]), X.LEAST, 1, [1])
    assert fit[0].tolist()[:2] == [0, 1]


def test_the_score_decides_among_the_allowed_zones(oracle):
    # nodes 0 (zone 0), 1 (zone 1), 2 (zone 2), 3 (zone 1), 100 units each, used 0 / 20 / 50 / 40; zone 0 already
    # holds one pod of the group; pods of 10 units, MOST, max_skew 1.
    # pod 0: zone 0 barred (1 + 1 - 0); among zones 1 and 2 MOST gives 30 / 60 / 50: node 2 (the unscored spread
    # call would take node 1, the first feasible). pod 1: zones 0 and 2 barred; node 1 at 30, node 3 at 50: node 3.
    # pod 2: (1, 1, 1), all allowed: 10 / 30 / 70 / 60: node 2.
    cnt0 = np.zeros((1, S.MAX_ZONES), np.int32)
    cnt0[0, 0] = 1
    for ref in (X.serial, X.per_pod):
        idx, sc, st, _, used, cnt = run(oracle, [0, 1, 2, 1], [100] * 4, [0, 20, 50, 40], [10] * 3, 1, X.MOST, cnt0, ref)
        assert idx.tolist() == [2, 3, 2] and sc.tolist() == [60, 50, 70] and not st.any()
        assert used.tolist() == [[0, 20, 70, 50]] and cnt[0, :3].tolist() == [1, 1, 2]
    n, p = 4, 3
    plain = S.serial(oracle, np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros(p, np.int8), np.zeros(p, np.uint8),
                     oracle.PluginSet(score=[], weights=[], normalize=[]), S.no_limit(n), np.array([[100] * 4]),
                     np.array([[0, 20, 50, 40]]), np.array([[10] * 3]), [0, 1, 2, 1], np.zeros(p, np.int32), [1], None, cnt0)
    assert plain[0].tolist()[0] == 1


def test_skew_invariant_after_every_placed_grouped_pod(oracle):
    for seed in range(500, 508):
        c = X.gen_case(seed, max_n=40, max_p=150)
        cols, eff, res, sp = case_args(c)
        u, nd, pd, pt = cols
        alloc, used, req = res
        zone, grp, skew = sp
        zs = S.zset(zone)
        ps = case_plugins(oracle, c)
        cnt = counts = None
        grouped_placed = 0
        for j in range(c["p"]):  # one pod per call: the state after every commit
            _, _, st, counts, used, cnt = X.serial(oracle, u, nd, pd[j:j + 1], pt[j:j + 1], ps, eff, alloc, used,
                                                   req[:, j:j + 1], zone, grp[j:j + 1], skew, c["score_mode"],
                                                   c["rs_weight"], c["rw"], counts, cnt)
            if st[0] == X.PLACED and grp[j] >= 0:
                grouped_placed += 1
                for g in range(c["G"]):
                    assert cnt[g].max() - cnt[g][zs].min() <= skew[g], (seed, j, g)
        assert grouped_placed > 0 or not zs


def test_the_sweep_generator_makes_the_conjunct_and_the_score_decide(oracle):
    """Over the GPU sweep's seeds, at least half of the cases place a pod differently both from the unscored
    spread reference and from the scored fit reference (the same pods ungrouped)."""
    both = 0
    for seed in SWEEP_SEEDS:
        c = X.gen_case(seed)
        assert c["n"] <= 2048 and 300 <= c["p"] <= 2000 and c["p"] % 64
        ps = case_plugins(oracle, c)
        cols, eff, res, sp = case_args(c)
        sc = (c["score_mode"], c["rs_weight"], c["rw"])
        wi = X.per_pod(oracle, *cols, ps, eff, *res, *sp, *sc)[0]
        unscored = S.per_pod(oracle, *cols, ps, eff, *res, *sp)[0]
        fit = RS.per_pod(oracle, *cols, ps, eff, *res, *sc)[0]
        both += bool((wi != unscored).any() and (wi != fit).any())
    total = len(SWEEP_SEEDS)
    assert 2 * both >= total, f"{both} of {total} cases differ from the unscored spread and the scored fit placements"
