"""The whole path from pod and node objects to placements, differentially: Scheduler (constraints.py, snapshot.py,
scheduler.py) over tests/column_ctx.py against tests/cluster_ref.py, the object-level one-pod-at-a-time reference, on
the seeded scenarios of tests/cluster_gen.py. The reference itself is held to hand-written cases whose placements were
worked out by hand; the scenarios are held to coverage conditions computed from the reference alone; and ten mutants of
the host layer must each make the differential fail. tests/test_cluster_gpu.py runs the same comparison on the device."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

import cluster_gen as G
import cluster_ref as R
from column_ctx import ColumnCtx

ZONE, HOST = G.ZONE, G.HOSTNAME
SMALL = [s for s in G.SCENARIOS if G.SCENARIOS[s][4] != "big"]


def run_scenario(msh, O, sc, ctx, steps=None):
    """Scheduler over `ctx` against the reference: every pod's outcome, node name and score, and after every call the
    pod counts, the used amounts, the spread counts and the inter-pod state words against what the reference derives
    from its placed list. Returns the reference and the scheduler."""
    cfg = sc["config"]
    s = msh.Scheduler(ctx=ctx, **cfg)
    ref = R.ClusterRef(O, **cfg)
    for k, step in enumerate(sc["steps"] if steps is None else steps):
        what = f"{sc['name']}, step {k}"
        if step[0] == "nodes":
            s.update_nodes(step[1])
            ref.update_nodes(step[1])
            assert s.nodes.names == [n["metadata"]["name"] for n in ref.nodes], f"{what}: List order"
            continue
        _, pods, mpn = step
        got = s.schedule_sequential(pods, max_pods_per_node=mpn)
        want = ref.schedule(pods, mpn)
        assert len(got) == len(want) == len(pods)
        for j, (g, w) in enumerate(zip(got, want)):
            have = (g.outcome.name, g.node_name, g.score if g.outcome.name == R.PLACED else 0)
            assert have == w, f"{what}, pod {j} {pods[j]['metadata']['name']}: got {have}, want {w} ({ctx_calls(ctx)})"
        assert np.asarray(ctx.node_pod_counts()).tolist() == ref.node_pod_counts(), f"{what}: pod counts"
        if cfg.get("resources"):
            res = ctx.node_resources()
            assert res is not None and np.asarray(res[1]).tolist() == ref.used_amounts(), f"{what}: used amounts"
        if cfg.get("zones"):
            assert np.asarray(ctx.spread_counts()).tolist() == ref.spread_counts(), f"{what}: spread counts"
        terms = s.pod_affinity_terms()
        if terms:
            pr, rp = ctx.pod_affinity_state()
            want_pr, want_rp = ref.affinity_words([(t, ns) for t, ns, _ in terms])
            assert np.asarray(pr).tolist() == want_pr, f"{what}: present words"
            assert np.asarray(rp).tolist() == want_rp, f"{what}: repel words"
    return ref, s


def ctx_calls(ctx):
    calls = getattr(ctx, "calls", None)
    return "" if calls is None else f"last calls {calls[-4:]}"


@pytest.fixture(scope="module")
def scenarios():
    return {name: G.scenario(name) for name in G.SCENARIOS}


@pytest.mark.parametrize("name", list(G.SCENARIOS))
def test_scheduler_matches_the_object_reference(msh, oracle, scenarios, name):
    ctx = ColumnCtx(oracle)
    run_scenario(msh, oracle, scenarios[name], ctx)


# ---- coverage: from the reference alone, so that no scenario passes by deciding nothing ----

def reference_run(O, sc, forget=False):
    ref = R.ClusterRef(O, **sc["config"])
    ref.forget_before_first_term = forget
    outs = []
    for step in sc["steps"]:
        if step[0] == "nodes":
            ref.update_nodes(step[1])
        else:
            outs.append((step[1], ref.schedule(step[1], step[2])))
    return ref, outs


def features(sc) -> set:
    """The filters a scenario exercises, by its configuration and its objects."""
    f = {"unschedulable", "static"}
    pods = [p for step in sc["steps"] if step[0] == "pods" for p in step[1]]
    nodes = [n for step in sc["steps"] if step[0] == "nodes" for n in step[1]]
    if any(step[0] == "pods" and step[2] for step in sc["steps"]) or any("pods" in n["status"]["allocatable"] for n in nodes):
        f.add("capacity")
    if sc["config"].get("resources"):
        f.add("resources")
    if sc["config"].get("zones") and any(p["metadata"]["labels"].get("app") in ("web", "db") for p in pods):
        f.add("spread")
    if any((p["spec"].get("affinity") or {}).keys() & {"podAffinity", "podAntiAffinity"} for p in pods):
        f.add("interpod")
    if sc["shape"] == "profiles":
        f -= {"unschedulable", "static"}
    return f


@pytest.mark.parametrize("name", list(G.SCENARIOS))
def test_scenarios_decide_something(oracle, scenarios, name):
    sc = scenarios[name]
    ref, outs = reference_run(oracle, sc)
    for f in features(sc):
        assert ref.rejections[f] > 0, f"{name}: the {f} filter rejects no node that the others left"
    con = [w[0] for pods, want in outs for p, w in zip(pods, want) if p["metadata"]["annotations"]["kind"] != "plain"]
    share = con.count(R.PLACED) / len(con)
    assert 0.2 <= share <= 0.8, f"{name}: {share:.2f} of the constrained pods are placed"
    kinds = {p["metadata"]["annotations"]["kind"] for pods, _ in outs for p in pods}
    if "series" in kinds:
        assert ref.first_pod > 0, f"{name}: the first-pod exception never fires"
    if "interpod" in features(sc) and sc["shape"] != "profiles":
        _, forgot = reference_run(oracle, sc, forget=True)
        assert [w for _, want in outs for w in want] != [w for _, want in forgot for w in want], \
            f"{name}: the late term changes no placement"


def test_scenarios_take_every_route(msh, oracle, scenarios):
    """Every entry point is reached, several within one snapshot, and the inter-pod stages arrive in the order the
    generator promises: no term, the first term, a new profile alone, a term of the other topology."""
    seen = set()
    for name in SMALL:
        ctx = ColumnCtx(oracle)
        run_scenario(msh, oracle, scenarios[name], ctx)
        routes = [c for c in ctx.calls if c.startswith("schedule_sequential")]
        seen |= set(routes)
        if scenarios[name]["shape"] == "interpod":
            c = ctx.calls
            assert routes[0] != "schedule_sequential_podaffinity" and routes[1:] == ["schedule_sequential_podaffinity"] * 3
            assert c.count("set_pod_affinity_terms") == 2 and c.count("set_pod_profiles") == 3
            assert c.count("upload_pod_affinity_state") == 2
        if name == "default-routes":
            assert routes == ["schedule_sequential", "schedule_sequential_classes", "schedule_sequential_classes"]
            assert ctx.calls.count("upload_node_class_bits") == 2  # a class first seen in the later call
        if name == "most-scored":
            assert routes == ["schedule_sequential_fit", "schedule_sequential_classes", "schedule_sequential_fit"]
        if name == "prefs":
            assert routes == ["schedule_sequential", "schedule_sequential_prefs", "schedule_sequential_prefs"]
        if name == "all-renodes":
            assert ctx.calls.count("upload_nodes") == 2
    assert seen == {"schedule_sequential" + s for s in ("", "_fit", "_spread_scored", "_classes", "_prefs", "_balanced",
                                                         "_podaffinity")}


# ---- mutants of the host layer: each must make the differential fail on at least one scenario ----

def _mutants(msh):
    sched = importlib.import_module("mini-kube-scheduler_amd.scheduler")
    K = importlib.import_module("mini-kube-scheduler_amd.constraints")
    snap = importlib.import_module("mini-kube-scheduler_amd.snapshot")
    S = sched.Scheduler
    import json

    def class_key_without_tolerations(mp):
        mp.setattr(K, "class_key", lambda pod: json.dumps([K.pod_node_name(pod), sorted(K.pod_node_selector(pod).items()),
                                                           K._plain(K.pod_affinity_terms(pod))], sort_keys=True))

    def classes_kept_across_update_nodes(mp):
        orig = S.update_nodes

        def update_nodes(self, nodes):
            keep = (self._class_ids, self._class_masks, self._class_aff, self._class_pns, self._class_prefers)
            out = orig(self, nodes)
            self._class_ids, self._class_masks, self._class_aff, self._class_pns, self._class_prefers = keep
            return out
        mp.setattr(S, "update_nodes", update_nodes)

    def zone_column_in_input_order(mp):
        orig = S.node_zone_ids

        def node_zone_ids(self):
            col, names = orig(self)
            out = np.empty_like(col)
            out[self.nodes.order] = col
            return out, names
        mp.setattr(S, "node_zone_ids", node_zone_ids)

    def capacity_not_permuted(mp):
        orig = sched.pack_nodes

        def pack_nodes(nodes):
            t = orig(nodes)
            if t.allocatable_pods is not None:
                cap = np.empty_like(t.allocatable_pods)
                cap[t.order] = t.allocatable_pods
                t.allocatable_pods = cap
            return t
        mp.setattr(sched, "pack_nodes", pack_nodes)

    def term_key_without_namespaces(mp):
        mp.setattr(K, "term_key", lambda term, ns: json.dumps([K._plain(K._get(term, "labelSelector", default=None)),
                                                               K._get(term, "topologyKey", default="")], sort_keys=True))

    def no_state_upload(mp):
        mp.setattr(ColumnCtx, "upload_pod_affinity_state", lambda self, present=None, repel=None: None)

    def rebuilt_repel_empty(mp):
        orig = S.pod_affinity_state
        mp.setattr(S, "pod_affinity_state", lambda self: (orig(self)[0], np.zeros(len(self._node_objs), np.uint32)))

    def profiles_kept(mp):
        class Sticky(dict):  # a table that is never thrown away: assigning {} over it keeps what it held
            pass
        orig = S.pod_profile_ids

        def pod_profile_ids(self, pods):
            before = dict(self._pa_profiles)
            n_terms = len(self._pa_terms)
            out = orig(self, pods)
            if out is not None and len(self._pa_terms) > n_terms and before:
                merged = dict(before)
                remap = {}
                for prof, q in self._pa_profiles.items():
                    remap[q] = merged.setdefault(prof, len(merged))
                if len(merged) > 64:
                    raise ValueError("more than 64 pod profiles")
                self._pa_profiles = merged
                out = np.array([remap.get(int(q), -1) for q in out], np.int32)
            return out
        mp.setattr(S, "pod_profile_ids", pod_profile_ids)

    def init_containers_ignored(mp):
        orig = sched.pod_requests

        def pod_requests(p, names):
            q = {"metadata": p.get("metadata"), "spec": {k: v for k, v in p["spec"].items() if k != "initContainers"}}
            return orig(q, names)
        mp.setattr(sched, "pod_requests", pod_requests)

    def notin_false_on_absent_key(mp):
        orig = K._expression_matches

        def expression_matches(e, labels):
            if K._get(e, "operator", default="") == "NotIn" and K._get(e, "key", default="") not in labels:
                return False
            return orig(e, labels)
        mp.setattr(K, "_expression_matches", expression_matches)

    return {f.__name__: f for f in (class_key_without_tolerations, classes_kept_across_update_nodes,
                                    zone_column_in_input_order, capacity_not_permuted, term_key_without_namespaces,
                                    no_state_upload, rebuilt_repel_empty, profiles_kept, init_containers_ignored,
                                    notin_false_on_absent_key)}


MUTANTS = ("class_key_without_tolerations", "classes_kept_across_update_nodes", "zone_column_in_input_order",
           "capacity_not_permuted", "term_key_without_namespaces", "no_state_upload", "rebuilt_repel_empty",
           "profiles_kept", "init_containers_ignored", "notin_false_on_absent_key")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_differential_catches_the_mutant(msh, oracle, scenarios, monkeypatch, mutant):
    _mutants(msh)[mutant](monkeypatch)
    caught = []
    for name in SMALL:
        try:
            run_scenario(msh, oracle, scenarios[name], ColumnCtx(oracle))
        except Exception as e:  # a wrong placement, a wrong read-back or a refusal: all are failures of the differential
            caught.append((name, type(e).__name__))
    assert caught, f"{mutant} survives every scenario"


# ---- hand-written cases: the reference (and the scheduler) against placements worked out by hand ----
# Pod names end in 9 and no node's does, so NodeNumber scores 0 everywhere and the first feasible node in List order
# wins, unless the case is about a score. Expected: a node name, None for a FIT_ERROR, "score" for a SCORE_ERROR, or
# (node name, total) where the total is part of the case.

def node(name, labels=None, taints=None, unschedulable=False, **alloc):
    spec = {}
    if taints:
        spec["taints"] = taints
    if unschedulable:
        spec["unschedulable"] = True
    return {"metadata": {"name": name, "labels": dict(labels or {})}, "spec": spec,
            "status": {"allocatable": {k.replace("_", "-"): v for k, v in alloc.items()}}}


def pod(name="p-9", labels=None, ns=None, requests=None, init=None, **spec):
    meta = {"name": name, "labels": dict(labels or {}), "annotations": {"kind": "hand"}}
    if ns:
        meta["namespace"] = ns
    if requests is not None:
        spec["containers"] = [{"resources": {"requests": r}} for r in requests]
    if init is not None:
        spec["initContainers"] = [{"resources": {"requests": r}} for r in init]
    return {"metadata": meta, "spec": spec}


def required(*terms):
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": list(terms)}}}


def ex(key, op, *values):
    return {"matchExpressions": [dict(key=key, operator=op, **({"values": list(values)} if values else {}))]}


def term(labels, key=HOST, namespaces=None):
    return G._pod_term(labels, key, namespaces)


def anti(*terms):
    return {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": list(terms)}}


def affine(*terms):
    return {"podAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": list(terms)}}


def taint(key, value="", effect="NoSchedule"):
    return {"key": key, "value": value, "effect": effect}


ABC = [node("b1", {"pool": "y", "gpu": "mi300"}), node("c2", {"pool": "y", "tier": "x7"}), node("a0", {"pool": "x"})]
ABCD = ABC + [node("d3", {"pool": "x", "tier": "5"})]
TAINTED = [node("a0", taints=[taint("k", "v")]), node("b1", taints=[taint("m", effect="NoExecute")]), node("c2")]
ZONED = [node("a0", {"zone": "z1"}), node("b1", {"zone": "z1"}), node("c2"), node("d3", {"zone": "z2"})]
Z = dict(zones="zone", spread_groups={"web": 1})
SIZED = [node("a0", cpu="100m", memory="1Gi"), node("b1", cpu="1", memory="1.5Gi"), node("c2", cpu="2", memory="12e6")]
CPU2 = [node("a0", cpu="1", memory="1Gi"), node("b1", cpu="4", memory="1Gi")]
REP = {"role": "rep"}
rep = lambda name="r-9": pod(name, REP, affinity=anti(term(REP)))          # noqa: E731
ser = lambda name="s-9": pod(name, {"role": "ser"}, affinity=affine(term({"role": "ser"}, "zone")))  # noqa: E731
fol = lambda name="f-9": pod(name, {"role": "fol"}, affinity=affine(term({"role": "ser"}, "zone")))  # noqa: E731
CPU_MEM = dict(resources=("cpu", "memory"))

HAND = {
    "first node in List order": ({}, [ABC, ([pod()], 0)], ["a0"]),
    "NodeNumber picks the node with the pod's digit": ({}, [ABC, ([pod("p-2")], 0)], [("c2", 10)]),
    "sorted order differs from input order (node1 < node10 < node2)":
        ({}, [[node("node2"), node("node10"), node("node1")], ([pod(), pod(), pod()], 1)], ["node1", "node10", "node2"]),
    "nodeSelector": ({}, [ABC, ([pod(nodeSelector={"pool": "y"})], 0)], ["b1"]),
    "NotIn on an absent key matches": ({}, [ABC, ([pod(affinity=required(ex("gpu", "NotIn", "mi300")))] * 3, 1)],
                                       ["a0", "c2", None]),
    "Gt on a non-integer label matches nothing": ({}, [ABC, ([pod(affinity=required(ex("tier", "Gt", "3")))], 0)], [None]),
    "Gt on an integer label": ({}, [ABCD, ([pod(affinity=required(ex("tier", "Gt", "3")))], 0)], ["d3"]),
    "an empty nodeSelectorTerms matches nothing": ({}, [ABC, ([pod(affinity=required())], 0)], [None]),
    "a term with neither expressions nor fields matches nothing": ({}, [ABC, ([pod(affinity=required({}))], 0)], [None]),
    "terms are ORed, an empty one is skipped": ({}, [ABC, ([pod(affinity=required({}, ex("pool", "In", "y")))], 0)], ["b1"]),
    "matchFields on metadata.name":
        ({}, [ABC, ([pod(affinity=required({"matchFields": [dict(key="metadata.name", operator="In", values=["c2"])]}))], 0)],
         ["c2"]),
    "In without values is invalid": ({}, [ABC, ([pod(affinity=required(ex("pool", "In")))], 0)], [None]),
    "Exists with values is invalid, DoesNotExist matches the absent key":
        ({}, [ABC, ([pod(affinity=required(ex("pool", "Exists", "x"))), pod(affinity=required(ex("gpu", "DoesNotExist"))),
                     pod(affinity=required(ex("gpu", "DoesNotExist")))], 1)], [None, "a0", "c2"]),
    "a toleration with an empty key and Exists tolerates every taint":
        ({}, [TAINTED, ([pod(), pod(tolerations=[{"operator": "Exists"}])], 0)], ["c2", "a0"]),
    "effect-less tolerations; another effect does not tolerate":
        ({}, [TAINTED, ([pod(tolerations=[{"key": "k", "value": "v"}]),
                         pod(tolerations=[{"key": "k", "value": "v", "effect": "NoExecute"}]),
                         pod(tolerations=[{"key": "m", "operator": "Exists"}]),
                         pod(tolerations=[{"key": "k", "value": "w"}])], 0)], ["a0", "c2", "b1", "c2"]),
    "PreferNoSchedule never filters": ({}, [[node("a0", taints=[taint("s", effect="PreferNoSchedule")]), node("b1")],
                                            ([pod()], 0)], ["a0"]),
    "the unschedulable toleration": ({}, [[node("a0", unschedulable=True), node("b1")], (
        [pod(), pod(tolerations=[{"key": "node.kubernetes.io/unschedulable", "operator": "Exists", "effect": "NoSchedule"}]),
         pod(tolerations=[{"key": "node.kubernetes.io/unschedulable", "operator": "Exists", "effect": "NoExecute"}])], 0)],
        ["b1", "a0", "b1"]),
    "NodeName": ({}, [ABC, ([pod(nodeName="c2"), pod(nodeName="gone")], 0)], ["c2", None]),
    "quantities 100m, 1.5Gi, 0.5 and 12e6 (the exponent form parse_quantity refused)":
        (CPU_MEM, [SIZED, ([pod(requests=[{"cpu": "0.5"}]), pod(requests=[{"memory": "1.5Gi"}]),
                            pod(requests=[{"cpu": "100m", "memory": "12e6"}]), pod(requests=[{"cpu": "100m"}]),
                            pod(requests=[{"memory": "12e6"}]), pod(requests=[{"cpu": "1.5"}]),
                            pod(requests=[{"cpu": "1E3"}])], 0)],
         ["b1", "b1", "a0", "b1", "a0", "c2", None]),
    "an init container larger than the sum of the containers":
        (CPU_MEM, [CPU2, ([pod(requests=[{"cpu": "250m"}, {"cpu": "250m"}], init=[{"cpu": "2"}])] * 3, 0)], ["b1", "b1", None]),
    "allocatable.pods on one node only, with and without max_pods_per_node":
        ({}, [[node("a0", pods="1"), node("b1"), node("c2")], ([pod()] * 3, 0), ([pod()] * 2, 2)],
         ["a0", "b1", "b1", "c2", "c2"]),
    "the skew rule over the snapshot's zones; an unzoned node takes no grouped pod":
        (Z, [[node("a0", {"zone": "z1"}), node("b1", {"zone": "z2"}), node("c2")],
             ([pod(labels={"app": "web"})] * 3 + [pod()], 0), ([pod(labels={"app": "web"})] * 3, 2)],
         ["a0", "b1", "a0", "a0", "b1", None, None]),  # the second call: a0 holds 3 pods, b1 takes its second and is full
    "a self-affine series opens one zone": (Z, [ZONED, ([ser(), ser(), ser()], 1)], ["a0", "b1", None]),
    "a follower has no first-pod exception": (Z, [ZONED, ([fol(), ser(), fol()], 0)], [None, "a0", "a0"]),
    "a term with namespaces; without them the owner's namespace":
        ({}, [ABC, ([pod(labels=REP, ns="other"), pod(affinity=anti(term(REP))),
                     pod(affinity=anti(term(REP, HOST, ["other"])))], 0)], ["a0", "a0", "b1"]),
    "a placed pod's anti-affinity repels a pod that has none of its own":
        ({}, [ABC, ([rep(), pod(labels=REP), pod()], 0)], ["a0", "b1", "a0"]),
    "own anti-affinity: one replica per node": ({}, [ABC, ([rep()] * 4, 0)], ["a0", "b1", "c2", None]),
    "zone anti-affinity; a node without the zone is in no domain":
        (Z, [ZONED, ([pod(labels=REP), pod(affinity=anti(term(REP, "zone"))), pod(affinity=anti(term(REP, "zone")))], 1)],
         ["a0", "c2", "d3"]),
    "a term that arrives in a later call is evaluated against the pods placed before it":
        ({}, [ABC, ([pod(labels=REP), pod(labels=REP)], 0), ([rep()], 0), ([pod(labels=REP)], 0)], ["a0", "a0", "b1", "a0"]),
    "update_nodes forgets the placed pods and the terms":
        ({}, [ABC, ([rep(), rep()], 0), ABC, ([rep(), pod(labels=REP)], 0)], ["a0", "b1", "a0", "b1"]),
    "the PreferNoSchedule score": (dict(prefer_no_schedule_weight=1),
                                   [[node("a0", taints=[taint("s", effect="PreferNoSchedule")]), node("b1")], ([pod()], 0)],
                                   [("b1", 100)]),
    "the preferred node affinity score":
        (dict(preferred_affinity_weight=2), [ABC, ([pod(affinity={"nodeAffinity": {
            "preferredDuringSchedulingIgnoredDuringExecution": [{"weight": 10, "preference": ex("pool", "In", "y")},
                                                                {"weight": 4, "preference": ex("tier", "Exists")}]}})], 0)],
         [("c2", 200)]),
    "LeastAllocated": (dict(resources=("cpu",), resource_score="least"),
                       [CPU2, ([pod(requests=[{"cpu": "500m"}])], 0)], [("b1", 87)]),
    "MostAllocated": (dict(resources=("cpu",), resource_score="most"),
                      [CPU2, ([pod(requests=[{"cpu": "500m"}])], 0)], [("a0", 50)]),
    "BalancedAllocation": (dict(resources=("cpu", "memory"), balanced_allocation_weight=1),
                           [[node("a0", cpu="2", memory="1Gi"), node("b1", cpu="1", memory="1Gi")],
                            ([pod(requests=[{"cpu": "500m", "memory": "512Mi"}])], 0)], [("b1", 100)]),
    "a name without a digit is a SCORE_ERROR only when a node is feasible":
        ({}, [ABC, ([pod("px"), pod("px", nodeName="gone")], 0)], ["score", None]),
}


@pytest.mark.parametrize("case", list(HAND))
def test_hand_case(msh, oracle, case):
    cfg, steps, expected = HAND[case]
    steps = [("nodes", s) if isinstance(s, list) else ("pods", *s) for s in steps]
    want = [(R.PLACED, e, None) if isinstance(e, str) and e != "score" else (R.FIT_ERROR, None, 0) if e is None
            else (R.SCORE_ERROR, None, 0) if e == "score" else (R.PLACED, *e) for e in expected]
    ref, outs = reference_run(oracle, dict(config=cfg, steps=steps))
    got = [w for _, ws in outs for w in ws]
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g[:2] == w[:2] and (w[2] is None or g[2] == w[2]), f"{case}, pod {j}: the reference gives {g}, by hand {w}"
    run_scenario(msh, oracle, dict(name=case, config=cfg, steps=steps), ColumnCtx(oracle))  # and the scheduler agrees


def test_parse_quantity_takes_the_decimal_exponent(msh):
    """The API serves "12e6" and "1E3"; parse_quantity refused both before this test came."""
    snap = importlib.import_module("mini-kube-scheduler_amd.snapshot")
    for s, milli in (("12e6", False), ("1E3", False), ("5e-1", True), ("1.5e3", False), ("1e-3", False), ("+2e0", True),
                     ("100m", True), ("1.5Gi", False), ("0.5", True), (".5", True), ("1m", False)):
        assert snap.parse_quantity(s, milli) == R.quantity(s, milli), s
    assert snap.parse_quantity("12e6") == 12_000_000 and snap.parse_quantity("5e-1", milli=True) == 500
    for bad in ("1e", "e3", "1e3Ki", "1Kie3", "1e3.5", "1e999"):
        with pytest.raises(ValueError):
            snap.parse_quantity(bad)
