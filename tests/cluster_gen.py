"""Seeded scenarios for the object-level differential (tests/test_cluster.py, tests/test_cluster_gpu.py). A scenario is
one Scheduler configuration plus a list of steps, each ("nodes", nodes) for update_nodes or ("pods", pods,
max_pods_per_node) for schedule_sequential. Objects are plain k8s-shaped dicts. Test infrastructure only.

Node names are node<k> with k drawn without order from a range ten times the table, so that List order (byte-wise:
node10 < node2) differs from input order and the suffix digits are spread. Every node carries kubernetes.io/hostname
equal to its name. The generator stays inside the documented limits (64 classes, 32 terms, 64 profiles, 64 zones, one
required affinity term per pod, topology keys hostname or the zone label), so a refusal is a finding.

A pod's metadata.annotations.kind names the template it was made from; nothing reads it but the coverage checks."""
from __future__ import annotations

import copy

import numpy as np

ZONE = "topology.kubernetes.io/zone"
HOSTNAME = "kubernetes.io/hostname"
CPUS = ("2", "4", "2500m", "1.5", "8")
MEMS = ("4Gi", "8Gi", "12e9", "1.5Gi", "6000M")


def make_nodes(rng, n, zones=0, nres=2, taints=True, caps=False, unzoned=0.15):
    ids = rng.choice(np.arange(1, 10 * n + 10), n, replace=False)
    nodes = []
    for k in ids:
        name = f"node{int(k)}"
        labels = {HOSTNAME: name, "pool": str(rng.choice(["a", "b", "c"])),
                  "tier": str(rng.choice(["1", "3", "5", "x7", "+4"]))}
        if rng.random() < 0.2:
            labels["gpu"] = str(rng.choice(["mi300", "mi355"]))
        if zones and rng.random() >= unzoned:
            labels[ZONE] = f"z{int(rng.integers(0, zones))}"
        spec = {}
        if rng.random() < 0.08:
            spec["unschedulable"] = True
        if taints:
            ts = []
            if rng.random() < 0.15:
                ts.append({"key": "dedicated", "value": "infra", "effect": "NoSchedule"})
            if rng.random() < 0.08:
                ts.append({"key": "maint", "effect": "NoExecute"})
            if rng.random() < 0.25:
                ts.append({"key": "soft", "value": str(rng.choice(["x", "y"])), "effect": "PreferNoSchedule"})
            if ts:
                spec["taints"] = ts
        alloc = {"cpu": str(rng.choice(CPUS)), "memory": str(rng.choice(MEMS))}
        if nres >= 3:
            alloc["ephemeral-storage"] = str(rng.choice(["20Gi", "1e10", "50G"]))
        if rng.random() < 0.05:
            del alloc["memory"]  # a node lacking a value has 0 of it
        if caps and rng.random() < 0.4:
            alloc["pods"] = str(int(rng.integers(0, 4)))
        nodes.append({"metadata": {"name": name, "labels": labels}, "spec": spec, "status": {"allocatable": alloc}})
    return nodes


def _aff(terms):
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": terms}}}


def _expr(key, op, *values):
    e = {"key": key, "operator": op}
    if values:
        e["values"] = list(values)
    return e


def _pod_term(labels, key=HOSTNAME, namespaces=None):
    t = {"labelSelector": {"matchLabels": dict(labels)}, "topologyKey": key}
    if namespaces:
        t["namespaces"] = list(namespaces)
    return t


STATIC_KINDS = ("selector", "in", "notin_absent", "gt", "field", "empty_terms", "node_name", "tol_equal", "tol_all",
                "tol_effectless", "tol_unsched", "two_terms")
PREF_KINDS = ("prefer_pool", "prefer_tier", "tol_soft")
GROUP_KINDS = ("web", "db")
# inter-pod kinds by the stage that first brings them
POD_KINDS = {"victim": ("victim",), "first_term": ("replica", "victim"), "new_profile": ("replica", "victim", "bystander"),
             "zone_term": ("replica", "zone_replica", "series", "follower", "ns_anti", "ns_victim", "orphan")}


def make_pod(rng, j, kind, nodes, nres=0, big_init=False):
    """One pod of template `kind`; the name ends in a digit (one in forty does not: a SCORE_ERROR)."""
    d = int(rng.integers(0, 10))
    name = f"{kind.replace('_', '')}-{j}x" if rng.random() < 0.025 else f"{kind.replace('_', '')}-{j}-{d}"
    meta = {"name": name, "labels": {}, "annotations": {"kind": kind}}
    spec = {}
    aff = {}
    if kind == "selector":
        spec["nodeSelector"] = {"pool": str(rng.choice(["a", "b"]))}
    elif kind == "in":
        aff.update(_aff([{"matchExpressions": [_expr("pool", "In", "b", "c"), _expr("tier", "Exists")]}]))
    elif kind == "notin_absent":  # most nodes lack the key: NotIn matches them
        aff.update(_aff([{"matchExpressions": [_expr("gpu", "NotIn", "mi300"), _expr("pool", "In", "a", "b")]}]))
    elif kind == "gt":            # "x7" is no integer: no match; "+4" parses
        aff.update(_aff([{"matchExpressions": [_expr("tier", "Gt", "3")]}]))
    elif kind == "field":
        aff.update(_aff([{"matchFields": [_expr("metadata.name", "NotIn", nodes[0]["metadata"]["name"])],
                          "matchExpressions": [_expr("gpu", "DoesNotExist"), _expr("pool", "NotIn", "c")]}]))
    elif kind == "empty_terms":
        aff.update(_aff([] if rng.random() < 0.5 else [{}]))
    elif kind == "two_terms":     # ORed terms, the first invalid (Lt with two values)
        aff.update(_aff([{"matchExpressions": [_expr("tier", "Lt", "3", "4")]},
                         {"matchExpressions": [_expr("tier", "Lt", "4")]}]))
    elif kind == "node_name":
        spec["nodeName"] = nodes[int(rng.integers(0, len(nodes)))]["metadata"]["name"] if rng.random() < 0.7 else "gone"
    elif kind == "tol_equal":
        spec["tolerations"] = [{"key": "dedicated", "operator": "Equal", "value": "infra", "effect": "NoSchedule"}]
        spec["nodeSelector"] = {"pool": "c"}
    elif kind == "tol_all":
        spec["tolerations"] = [{"operator": "Exists"}]
    elif kind == "tol_effectless":
        spec["tolerations"] = [{"key": "maint", "operator": "Exists"}, {"key": "dedicated", "value": "infra"}]
    elif kind == "tol_unsched":
        spec["tolerations"] = [{"key": "node.kubernetes.io/unschedulable", "operator": "Exists", "effect": "NoSchedule"}]
    elif kind == "prefer_pool":
        aff["nodeAffinity"] = {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 10, "preference": {"matchExpressions": [_expr("pool", "In", "a")]}},
            {"weight": 5, "preference": {"matchExpressions": [_expr("tier", "Gt", "2")]}},
            {"weight": 0, "preference": {"matchExpressions": [_expr("pool", "Exists")]}}]}
    elif kind == "prefer_tier":
        aff["nodeAffinity"] = {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 7, "preference": {"matchFields": [_expr("metadata.name", "In", nodes[-1]["metadata"]["name"])]}},
            {"weight": 3, "preference": {}}]}
    elif kind == "tol_soft":
        spec["tolerations"] = [{"key": "soft", "operator": "Equal", "value": "x", "effect": "PreferNoSchedule"}]
    elif kind in GROUP_KINDS:
        meta["labels"]["app"] = kind
    elif kind == "replica":       # one per node: repels its own kind
        meta["labels"]["role"] = "rep"
        aff["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [_pod_term({"role": "rep"})]}
    elif kind == "zone_replica":  # one per zone, and none where a victim already is
        meta["labels"]["role"] = "zrep"
        aff["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [_pod_term({"role": "rep"}, ZONE)]}
    elif kind == "victim":        # matches what the replicas repel, repels nothing
        meta["labels"]["role"] = "rep"
    elif kind == "bystander":     # the replicas' term again, from a pod that does not match it: a profile of its own
        meta["labels"]["role"] = "by"
        aff["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [_pod_term({"role": "rep"}),
                                                                                   _pod_term({"role": "rep"})]}
    elif kind == "series":        # self-affine on the zone: the first one opens a zone
        meta["labels"]["role"] = "ser"
        aff["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [_pod_term({"role": "ser"}, ZONE)]}
    elif kind == "follower":      # wants the series' zone, matches nothing: no first-pod exception
        meta["labels"]["role"] = "fol"
        aff["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [_pod_term({"role": "ser"}, ZONE)]}
    elif kind == "orphan":        # wants a pod that never comes and does not match it itself
        meta["labels"]["role"] = "orp"
        aff["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [_pod_term({"role": "nobody"})]}
    elif kind == "ns_anti":       # the same selector as the replicas', over another namespace: another term
        meta["labels"]["role"] = "nsa"
        aff["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [
            _pod_term({"role": "rep"}, HOSTNAME, ["other"])]}
    elif kind == "ns_victim":
        meta["labels"]["role"] = "rep"
        meta["namespace"] = "other"
    elif kind.startswith("subset"):  # many profiles: a subset of six labels, each label a term of `subset_anti`
        for b in range(6):
            if int(kind[6:]) >> b & 1:
                meta["labels"][f"k{b}"] = "1"
    elif kind.startswith("anti"):    # repels label k<b> per node
        b = int(kind[4:])
        meta["labels"]["role"] = "anti"
        aff["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": [_pod_term({f"k{b}": "1"})]}
    if aff:
        spec["affinity"] = aff
    if nres:
        req = {"cpu": str(rng.choice(["100m", "250m", "0.5", "1", "1.5"])),
               "memory": str(rng.choice(["64Mi", "12e6", "1Gi", "1.5Gi", "500M"]))}
        if nres >= 3:
            req["ephemeral-storage"] = str(rng.choice(["1Gi", "2e9"]))
        if rng.random() < 0.15:
            del req[str(rng.choice(list(req)))]
        cs = [{"name": "main", "resources": {"requests": req}}]
        if rng.random() < 0.3:
            cs.append({"name": "side", "resources": {"requests": {"cpu": "50m"}}})
        if rng.random() < 0.1:
            cs = [{"name": "idle"}]
        spec["containers"] = cs
        if big_init or rng.random() < 0.2:  # an init container larger than the sum
            spec["initContainers"] = [{"name": "init", "resources": {"requests": {"cpu": "2", "memory": "3Gi"}}}]
    return {"metadata": meta, "spec": spec}


def make_pods(rng, p, kinds, nodes, nres=0, plain=0.3, start=0, hard=0.2):
    """p pods of `kinds`; a share `plain` without constraints and a share `hard` that no node can take."""
    out = []
    for j in range(p):
        kind = "plain" if rng.random() < plain else str(rng.choice(kinds))
        if kind != "plain" and len(kinds) > 1 and rng.random() < hard:
            kind = str(rng.choice(["empty_terms", "node_name", "gt"]))
        out.append(make_pod(rng, start + j, kind, nodes, nres))
    return out


CONFIGS = {
    "default": {},
    "resources": dict(resources=("cpu", "memory")),
    "least": dict(resources=("cpu", "memory"), resource_score="least", resource_score_weight=2,
                  resource_weights={"cpu": 3, "memory": 1}),
    "most": dict(resources=("cpu", "memory"), resource_score="most", resource_weights=[1, 2]),
    "zones": dict(zones=ZONE, spread_groups={"web": 1, "db": 2}),
    "prefs": dict(preferred_affinity_weight=2, prefer_no_schedule_weight=3),
    "balanced": dict(resources=("cpu", "memory"), balanced_allocation_weight=2),
    "all": dict(resources=("cpu", "memory"), resource_score="least", resource_weights=[2, 1], zones=ZONE,
                spread_groups={"web": 1, "db": 2}, preferred_affinity_weight=1, prefer_no_schedule_weight=2,
                balanced_allocation_weight=1),
    "all3": dict(resources=("cpu", "memory", "ephemeral-storage"), resource_score="most", resource_weights=[1, 1, 1],
                 zones=ZONE, spread_groups={"web": 1, "db": 2}, preferred_affinity_weight=1,
                 prefer_no_schedule_weight=1, balanced_allocation_weight=1),
}

# name: (config, seed, nodes, pods per call, what the steps hold). The seeds were picked on the CPU so that the coverage
# conditions of tests/test_cluster.py hold.
SCENARIOS = {
    "default-routes": ("default", 11, 40, 60, "static"),
    "resources-fit": ("resources", 12, 30, 70, "static"),
    "least-scored": ("least", 13, 40, 60, "static"),
    "most-scored": ("most", 14, 25, 60, "plainfirst"),
    "zones-spread": ("zones", 15, 50, 60, "groups"),
    "prefs": ("prefs", 16, 40, 50, "prefs"),
    "balanced": ("balanced", 17, 30, 60, "static"),
    "interpod-default": ("zones", 18, 30, 40, "interpod"),
    "interpod-all": ("all", 19, 60, 40, "interpod"),
    "many-profiles": ("default", 104, 24, 70, "profiles"),
    "all-renodes": ("all", 21, 80, 50, "everything"),
    "wave4": ("all", 105, 300, 40, "big"),
    "wave16": ("all", 115, 1100, 30, "big"),
    "three-resources": ("all3", 130, 600, 45, "big"),
}


def scenario(name: str) -> dict:
    cfg_name, seed, n, p, shape = SCENARIOS[name]
    cfg = copy.deepcopy(CONFIGS[cfg_name])
    rng = np.random.default_rng(4_000_000 + seed)
    nres = len(cfg.get("resources", ()))
    zones = 5 if "zones" in cfg else 0
    prefs = bool(cfg.get("preferred_affinity_weight"))
    kinds = STATIC_KINDS + (GROUP_KINDS if zones else ()) + (PREF_KINDS if prefs else ())
    nodes = make_nodes(rng, n, zones, nres, caps=shape in ("static", "everything", "groups"))
    steps = [("nodes", nodes)]
    mk = lambda q, ks, plain=0.3, s=0: make_pods(rng, q, ks, nodes, nres, plain, s)  # noqa: E731
    if shape == "static":      # plain (no class) -> classes -> a class first seen later, with a scalar limit
        steps += [("pods", mk(p // 2, ("tol_all",), 0.0), 0),
                  ("pods", mk(p, kinds[:8]), 0),
                  ("pods", mk(p, kinds, s=1000), 3)]
    elif shape == "plainfirst":  # untainted nodes: plain pods take the fit call, constrained ones the class call
        nodes[:] = make_nodes(rng, n, zones, nres, taints=False)
        steps += [("pods", mk(p // 2, ("plain",), 1.0), 0), ("pods", mk(p, kinds), 2), ("pods", mk(p // 2, ("plain",), 1.0, 500), 0)]
    elif shape == "groups":   # grouped pods that tolerate everything -> the spread call; then the class call
        first = make_pods(rng, p // 3, GROUP_KINDS, nodes, nres, 0.3, hard=0.0)
        for q in first:
            q["spec"]["tolerations"] = [{"operator": "Exists"}]
        steps += [("pods", first, 0)]
        steps += [("pods", mk(p, GROUP_KINDS, 0.4), 0), ("pods", mk(p, kinds), 0), ("pods", mk(p, GROUP_KINDS, 0.2, 1000), 2)]
    elif shape == "prefs":     # pods that tolerate everything -> the plain call; then the preference call
        steps += [("pods", mk(p // 2, ("tol_all",), 0.0), 0), ("pods", mk(p, kinds, s=1000), 0), ("pods", mk(p, PREF_KINDS, s=2000), 2)]
    elif shape == "interpod":
        base = ("selector", "tol_all") + (GROUP_KINDS if zones else ())
        steps += [("pods", mk(p, base + POD_KINDS["victim"], 0.3), 0)]
        for k, stage in enumerate(("first_term", "new_profile", "zone_term")):
            steps.append(("pods", mk(p, base[:1] + POD_KINDS[stage], 0.15, 1000 * (k + 1)), 6 if stage == "zone_term" else 0))
    elif shape == "profiles":  # six terms and ~40 profiles, then a seventh term and ~40 more against the same snapshot
        nodes[:] = make_nodes(rng, n, 0, 0, taints=False)
        one = lambda ks, s: [make_pod(rng, s + j, k, nodes) for j, k in enumerate(ks)]  # noqa: E731
        steps += [("pods", one([f"anti{b}" for b in range(6)] + [f"subset{m}" for m in range(1, 46)], 0), 2),
                  ("pods", one(["replica"] + [f"subset{m}" for m in range(20, 64)], 1000), 4)]
    elif shape == "everything":
        steps += [("pods", mk(p, kinds + POD_KINDS["victim"]), 0), ("pods", mk(p, kinds + POD_KINDS["first_term"], s=1000), 2)]
        nodes2 = make_nodes(rng, n // 2 + 7, zones, nres, caps=True)
        steps += [("nodes", nodes2)]
        mk2 = lambda q, ks, s: make_pods(rng, q, ks, nodes2, nres, 0.3, s)  # noqa: E731
        steps += [("pods", mk2(p, kinds + POD_KINDS["victim"], 2000), 0), ("pods", mk2(p, kinds + POD_KINDS["zone_term"], 3000), 0)]
    elif shape == "big":
        steps += [("pods", mk(p, kinds + POD_KINDS["victim"]), 0), ("pods", mk(p, kinds[:4] + POD_KINDS["zone_term"], s=1000), 1)]
    assert sum(1 for s in steps if s[0] == "pods") <= 6
    return dict(name=name, config=cfg, steps=steps, shape=shape)
