"""Preferred node affinity and PreferNoSchedule scores in sequential-commit mode, the parts that need no GPU: the
two CPU references of tests/prefs_ref.py against each other and against classes_ref, two hand-worked placements, the
pure-Python raw values (constraints.preferred_affinity_score, constraints.prefer_no_schedule_count) rule by rule,
the Scheduler's class ids with preferences on and off, the header against the binding, and what the GPU sweep's
generator has to reach."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import classes_ref as KR
import node_capacity_ref as CR
import prefs_ref as PR
import spread_ref as S
from test_classes import (RecordingCtx, case_args, case_plugins, expr, named, node, pod, same, taint, term, tol)

NEW_SYMBOLS = ["msh_upload_node_class_prefs", "msh_patch_node_class_prefs", "msh_clear_node_class_prefs",
               "msh_node_class_prefs", "msh_set_preference_weights", "msh_preference_weights",
               "msh_seq_prefs_max_nodes", "msh_schedule_sequential_prefs", "msh_schedule_sequential_prefs_device"]
SWEEP_SEEDS = range(31000, 31100)


def run(ref, oracle, c, w_aff=None, w_taint=None, trace=None):
    cols, eff, res, sp, sc = case_args(c)
    return ref(oracle, *cols, case_plugins(oracle, c), eff, *res, *sp, *sc, c["bits"], c["C"], c["pod_class"],
               c["A"], c["T"], c["w_aff"] if w_aff is None else w_aff, c["w_taint"] if w_taint is None else w_taint,
               trace=trace)


def test_new_symbols_are_declared_exported_and_bound(msh):
    header = (Path(__file__).resolve().parent.parent / "include" / "minisched_hip.h").read_text()
    lib = msh._native.lib()
    for nm in NEW_SYMBOLS:
        assert re.search(r"^int " + nm + r"\(", header, re.M), f"{nm} is not declared in the header"
        assert nm in msh._native.EXPORTED and hasattr(lib, nm), nm
        assert nm in msh._native._SIGS
    sigs = msh._native._SIGS
    assert len(sigs["msh_schedule_sequential_prefs"][1]) == len(sigs["msh_schedule_sequential_classes"][1])
    assert len(sigs["msh_schedule_sequential_prefs_device"][1]) == len(sigs["msh_schedule_sequential_classes_device"][1])
    inv = msh._native.MSH_ERR_INVALID
    assert lib.msh_upload_node_class_prefs(None, 0, 1, None, None) == inv
    assert lib.msh_patch_node_class_prefs(None, 0, None, None, None) == inv
    assert lib.msh_clear_node_class_prefs(None) == inv
    assert lib.msh_node_class_prefs(None, None, None, None, None) == inv
    assert lib.msh_set_preference_weights(None, 1, 1) == inv
    assert lib.msh_preference_weights(None, None, None) == inv
    assert lib.msh_seq_prefs_max_nodes(None, 0, None) == inv
    for nm in ("preferred_affinity_score", "prefer_no_schedule_count", "preference_key", "class_key", "node_admits"):
        assert callable(getattr(msh.constraints, nm)), nm


def test_per_pod_equals_serial_on_200_seeds(oracle):
    placed = fit = 0
    modes, with_bits = set(), set()
    for seed in range(200):
        c = PR.gen_case(seed, max_n=40, max_p=60)
        a = run(PR.serial, oracle, c)
        b = run(PR.per_pod, oracle, c)
        same(a, b, f"seed {seed}")
        modes.add(c["score_mode"])
        with_bits.add(c["bits"] is None)
        placed += int((a[2] == PR.PLACED).sum())
        fit += int((a[2] == PR.FIT_ERROR).sum())
    assert modes == {PR.NONE, PR.LEAST, PR.MOST} and with_bits == {True, False}
    assert placed > 1000 and fit > 1000


def test_with_weights_zero_the_references_are_classes_ref(oracle):
    for seed in range(60):
        c = PR.gen_case(seed, max_n=40, max_p=60)
        if c["bits"] is None:  # classes_ref has no "column absent, every node admits": all ones says the same
            c["bits"] = np.full(c["n"], np.uint64((1 << c["C"]) - 1), np.uint64)
        cols, eff, res, sp, sc = case_args(c)
        want = KR.serial(oracle, *cols, case_plugins(oracle, c), eff, *res, *sp, *sc, c["bits"], c["C"], c["pod_class"])
        same(run(PR.serial, oracle, c, 0, 0), want, f"serial, seed {seed}")
        same(run(PR.per_pod, oracle, c, 0, 0), want, f"per_pod, seed {seed}")


def tiny(oracle, n, p, cap, A=None, T=None, w_aff=1, w_taint=1, cls=None, bits=None, ref=PR.serial):
    """n plain nodes without digits, p pods of class 0, NodeNumber out of the score list: the preference terms alone."""
    ps = oracle.PluginSet(score=[], weights=[], normalize=[])
    a, us, rq = S.no_res(n, p)
    return ref(oracle, np.zeros(n, np.uint8), np.full(n, -1, np.int8), np.zeros(p, np.int8), np.ones(p, np.uint8), ps,
               CR.effective(np.asarray(cap, np.int64)), a, us, rq, None, None, (), PR.NONE, 0, [], bits, 1,
               np.zeros(p, np.int32) if cls is None else cls, A, T, w_aff, w_taint)


@pytest.mark.parametrize("ref", [PR.serial, PR.per_pod])
def test_hand_worked_fill_up(oracle, ref):
    """Three nodes with A = (100, 50, 10), one pod each. Pod 0: maxA = 100, na = (100, 50, 10), node 0, total 100 + 100.
    Node 0 is full: pod 1 is normalised by 50, na = (-, 100, 20), node 1 with total 200 again. Pod 2: maxA = 10, node 2
    at na = 100. Pod 3 finds nothing. A column normalised once by 100 would have scored pod 1 at 50 + 100."""
    idx, score, status = tiny(oracle, 3, 4, [1, 1, 1], A=[[100, 50, 10]], ref=ref)[:3]
    assert idx.tolist() == [0, 1, 2, -1]
    assert score.tolist() == [200, 200, 200, 0]
    assert status.tolist() == [PR.PLACED] * 3 + [PR.FIT_ERROR]


@pytest.mark.parametrize("ref", [PR.serial, PR.per_pod])
def test_hand_worked_taints_and_truncation(oracle, ref):
    """T = (3, 1, 2, 0) with capacities (9, 1, 1, 1) and w_taint = 2, A = (0, 0, 7, 3) with w_aff = 1.
    Pod 0: maxT = 3, nt = (0, 67, 34, 100); maxA = 7, na = (0, 0, 100, 42): totals (0, 134, 168, 242): node 3.
    Pod 1: node 3 is full; maxT = 3, nt = (0, 67, 34); maxA = 7: totals (0, 134, 168): node 2.
    Pod 2: nodes 0, 1: maxT = 3, nt = (0, 67), maxA = 0: node 1 at 134.
    Pod 3: node 0 alone: maxT = 3, nt = 100 - 100 = 0, total 0."""
    idx, score, status = tiny(oracle, 4, 4, [9, 1, 1, 1], A=[[0, 0, 7, 3]], T=[[3, 1, 2, 0]], w_aff=1, w_taint=2,
                              ref=ref)[:3]
    assert idx.tolist() == [3, 2, 1, 0]
    assert score.tolist() == [242, 168, 134, 0]
    assert (status == PR.PLACED).all()


def test_pods_without_a_preference_still_carry_the_taint_term(oracle):
    for cls in (np.full(3, -1, np.int32), np.zeros(3, np.int32)):
        idx, score, _ = tiny(oracle, 2, 3, [2, 2], A=None, T=None, w_aff=5, w_taint=7, cls=cls)[:3]
        assert idx.tolist() == [0, 0, 1] and score.tolist() == [700, 700, 700]


# ---- constraints.preferred_affinity_score and prefer_no_schedule_count, one table per rule ----

def pref(weight, *exprs, fields=()):
    return {"weight": weight, "preference": term(*exprs, fields=fields)}


def ppod(prefs=None, tolerations=None, **kw):
    p = pod(tolerations=tolerations, **kw)
    if prefs is not None:
        p["spec"].setdefault("affinity", {}).setdefault("nodeAffinity", {})[
            "preferredDuringSchedulingIgnoredDuringExecution"] = prefs
    return p


@pytest.mark.parametrize("prefs,labels,name,want", [
    (None, {"a": "1"}, "n1", 0),
    ([], {"a": "1"}, "n1", 0),
    ([pref(5, expr("a", "In", "1", "2"))], {"a": "2"}, "n1", 5),
    ([pref(5, expr("a", "In", "1", "2"))], {"a": "3"}, "n1", 0),
    ([pref(5, expr("a", "NotIn", "1"))], {}, "n1", 5),                    # NotIn matches an absent label
    ([pref(5, expr("a", "NotIn", "1"))], {"a": "1"}, "n1", 0),
    ([pref(5, expr("a", "Exists"))], {"a": ""}, "n1", 5),
    ([pref(5, expr("a", "Exists"))], {}, "n1", 0),
    ([pref(5, expr("a", "DoesNotExist"))], {}, "n1", 5),
    ([pref(5, expr("a", "DoesNotExist"))], {"a": "x"}, "n1", 0),
    ([pref(5, expr("a", "Gt", "5"))], {"a": "6"}, "n1", 5),
    ([pref(5, expr("a", "Gt", "5"))], {"a": "5"}, "n1", 0),
    ([pref(5, expr("a", "Lt", "5"))], {"a": "-3"}, "n1", 5),
    ([pref(5, expr("a", "Lt", "five"))], {"a": "1"}, "n1", 0),            # an unparsable value
    ([pref(5, expr("a", "Near", "1"))], {"a": "1"}, "n1", 0),             # an unknown operator
    ([pref(5, expr("a", "In", "1"), expr("b", "Exists"))], {"a": "1"}, "n1", 0),            # expressions are ANDed
    ([pref(5, expr("a", "In", "1"), expr("b", "Exists"))], {"a": "1", "b": ""}, "n1", 5),
    ([pref(5, fields=[expr("metadata.name", "In", "n1")])], {}, "n1", 5),                   # matchFields
    ([pref(5, fields=[expr("metadata.name", "In", "n2")])], {}, "n1", 0),
    ([pref(5, fields=[expr("metadata.name", "NotIn", "n2")])], {}, "n1", 5),
    ([pref(5, fields=[expr("metadata.uid", "In", "n1")])], {}, "n1", 0),                    # metadata.name only
    ([pref(5, expr("a", "In", "1"), fields=[expr("metadata.name", "In", "n2")])], {"a": "1"}, "n1", 0),  # ANDed
    ([pref(0, expr("a", "In", "1"))], {"a": "1"}, "n1", 0),                                 # weight 0 is skipped
    ([pref(5)], {"a": "1"}, "n1", 0),                                                       # an empty preference is skipped
    ([pref(5), pref(3, expr("a", "In", "1"))], {"a": "1"}, "n1", 3),
    ([pref(5, expr("a", "In", "1")), pref(3, expr("b", "Exists")), pref(100, expr("c", "Exists"))],
     {"a": "1", "b": ""}, "n1", 8),                                                         # matching terms are summed
    ([pref(100, expr("a", "Exists")), pref(100, expr("a", "In", "1"))], {"a": "1"}, "n1", 200),
])
def test_preferred_affinity_score(msh, prefs, labels, name, want):
    assert msh.constraints.preferred_affinity_score(ppod(prefs), node(name, labels)) == want


def test_the_required_terms_do_not_score_and_the_preferred_do_not_filter(msh):
    K = msh.constraints
    p = ppod([pref(9, expr("a", "In", "1"))], terms=[term(expr("b", "Exists"))])
    assert K.preferred_affinity_score(p, node("n", {"b": ""})) == 0 and K.node_admits(p, node("n", {"b": ""}))
    assert K.preferred_affinity_score(p, node("n", {"a": "1"})) == 9 and not K.node_admits(p, node("n", {"a": "1"}))


PNS = "PreferNoSchedule"


@pytest.mark.parametrize("taints,tols,want", [
    ([], [], 0),
    ([taint("k", "v", PNS)], [], 1),
    ([taint("k", "v", PNS), taint("j", "", PNS)], [], 2),
    ([taint("k", "v"), taint("j", "", "NoExecute")], [], 0),                        # the filtering effects do not count
    ([taint("k", "v", PNS)], [tol("k", "Equal", "v", PNS)], 0),
    ([taint("k", "v", PNS)], [tol("k", "Equal", "v")], 0),                          # an empty-effect toleration counts
    ([taint("k", "v", PNS)], [tol("k", "Equal", "v", "NoSchedule")], 1),            # a NoSchedule toleration does not
    ([taint("k", "v", PNS)], [tol("k", "Exists", effect="NoExecute")], 1),
    ([taint("k", "v", PNS)], [tol("k", "Equal", "w")], 1),
    ([taint("k", "v", PNS)], [tol("k", "Exists")], 0),
    ([taint("k", "v", PNS), taint("j", "", PNS)], [tol("", "Exists")], 0),          # Exists without a key: every taint
    ([taint("k", "v", PNS), taint("j", "", PNS)], [tol("", "Exists", effect="NoSchedule")], 2),
    ([taint("k", "v", PNS), taint("j", "", PNS)], [tol("k", "Exists")], 1),
    ([taint("k", "v", PNS), taint("k", "v")], [tol("k", "Exists", effect=PNS)], 0),
])
def test_prefer_no_schedule_count(msh, taints, tols, want):
    assert msh.constraints.prefer_no_schedule_count(pod(tolerations=tols), node(taints=taints)) == want


def test_preference_key(msh):
    K = msh.constraints
    a = ppod([pref(5, expr("a", "In", "1"))], tolerations=[tol("k", "Exists"), tol("j", "Exists")])
    b = ppod([pref(5, expr("a", "In", "1"))], tolerations=[tol("j", "Exists"), tol("k", "Exists")])
    assert K.preference_key(a) == K.preference_key(b)  # the tolerations' order does not matter
    assert K.preference_key(a) != K.preference_key(ppod([pref(6, expr("a", "In", "1"))], tolerations=a["spec"]["tolerations"]))
    assert K.preference_key(ppod()) == K.preference_key(pod()) and K.class_key(a) == K.class_key(pod(tolerations=a["spec"]["tolerations"]))


# ---- the Scheduler's class ids with preferences on and off ----

def cluster():
    return [node("node0", {"pool": "gpu", "zone": "a"}), node("node1", {"pool": "cpu", "zone": "a"}),
            node("node2", {"pool": "cpu", "zone": "b"}, [taint("spot", "", PNS)])]


def pnamed(name, prefs=None, **kw):
    p = ppod(prefs, **kw)
    p["metadata"]["name"] = name
    return p


def test_class_ids_with_preferences_off(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx)
    s.update_nodes(cluster())
    zone_a = pnamed("a1", [pref(10, expr("zone", "In", "a"))])
    assert s.pod_class_ids([zone_a, named("b2")]).tolist() == [-1, -1]  # nothing filters: no class, as before
    s.schedule_sequential([zone_a])
    assert ctx.names()[-1] == "schedule_sequential"
    assert not {"set_preference_weights", "upload_node_class_prefs", "schedule_sequential_prefs"} & set(ctx.names())


def test_class_ids_with_preferences_on(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx, preferred_affinity_weight=1, prefer_no_schedule_weight=1)
    assert ("set_preference_weights", (1, 1), {}) in ctx.calls
    s.update_nodes(cluster())
    zone_a = pnamed("a1", [pref(10, expr("zone", "In", "a"))])       # A = (10, 10, 0), T = (0, 0, 1): an id
    tolerant = pnamed("b2", tolerations=[tol("spot", "Exists")])      # admitted everywhere, A = T = 0: -1
    gpu = pnamed("c3", selector={"pool": "gpu"})                      # T = 1 on node2, which it is not admitted to
    nowhere = pnamed("d4", [pref(10, expr("zone", "In", "q"))], tolerations=[tol("", "Exists")])  # all raw values 0: -1
    ids = s.pod_class_ids([zone_a, tolerant, gpu, nowhere, zone_a])
    assert ids.tolist() == [0, -1, 1, -1, 0]
    s.schedule_sequential([tolerant, nowhere])  # no class at all: the call as before
    assert ctx.names()[-1] == "schedule_sequential"
    s.schedule_sequential([zone_a, tolerant, gpu])
    up = [c for c in ctx.calls if c[0] == "upload_node_class_prefs"]
    bits = [c for c in ctx.calls if c[0] == "upload_node_class_bits"]
    assert len(up) == 1 and len(bits) == 1 and up[0][1][0] == bits[0][1][0] == 2  # both columns, the same C
    assert np.asarray(up[0][1][1]).tolist() == [[10, 10, 0], [0, 0, 0]]
    assert np.asarray(up[0][1][2]).tolist() == [[0, 0, 1], [0, 0, 1]]
    assert np.asarray(bits[0][1][1]).tolist() == [0b11, 0b01, 0b01]
    call = ctx.calls[-1]
    assert call[0] == "schedule_sequential_prefs" and call[1][3].tolist() == [0, -1, 1]
    # same constraints, other preferences: another class
    other = pnamed("e5", [pref(20, expr("zone", "In", "a"))])
    assert s.pod_class_ids([other, zone_a]).tolist() == [2, 0]
    # a new snapshot starts over
    s.update_nodes(cluster()[:2])
    assert s.pod_class_ids([gpu, zone_a]).tolist() == [0, 1]


def test_a_class_without_a_raw_value_takes_the_class_call(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx, preferred_affinity_weight=3)
    s.update_nodes(cluster()[:2])  # no taints
    s.schedule_sequential([pnamed("c3", selector={"pool": "gpu"})])  # a filter, no preference
    assert ctx.names()[-1] == "schedule_sequential_classes"


def test_the_65th_class_and_a_sum_above_uint16_raise(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx, preferred_affinity_weight=1)
    s.update_nodes(cluster())
    pods = [pnamed(f"p{k}", [pref(k + 1, expr("zone", "In", "a"))]) for k in range(65)]
    assert s.pod_class_ids(pods[:64]).tolist() == list(range(64))
    with pytest.raises(ValueError, match="64"):
        s.pod_class_ids(pods)
    s.update_nodes(cluster())
    heavy = pnamed("h", [pref(100, expr("zone", "In", "a"))] * 656)  # 65,600 on nodes 0 and 1
    with pytest.raises(ValueError, match="65,535"):
        s.pod_class_ids([heavy])
    with pytest.raises(ValueError):
        msh.Scheduler(ctx=RecordingCtx(), prefer_no_schedule_weight=101)


# ---- what the GPU sweep's generator has to reach, on the references alone ----

def test_the_sweep_generator_reaches_what_the_sweep_is_for(oracle):
    """In at least half of the sweep's cases some pod's placement differs from the zero-weight placement, and in at
    least a quarter some class's maxA or maxT changes between two of its pods within the call."""
    seeds = list(SWEEP_SEEDS)
    differ = moves = 0
    for seed in seeds:
        c = PR.gen_case(seed)
        assert c["n"] <= 700 and c["p"] <= 300
        assert 100 * ((c["rs_weight"] if c["score_mode"] != PR.NONE else 0) + c["w_aff"] + c["w_taint"]) <= 65534
        trace = []
        a = run(PR.per_pod, oracle, c, trace=trace)
        b = run(PR.per_pod, oracle, c, 0, 0)
        differ += bool((a[0] != b[0]).any())
        seen, moved = {}, False
        for k, ma, mt in trace:
            if k >= 0:
                moved = moved or seen.setdefault(k, (ma, mt)) != (ma, mt)
        moves += moved
    assert 2 * differ >= len(seeds), (differ, len(seeds))
    assert 4 * moves >= len(seeds), (moves, len(seeds))
