"""An object-level reference for Scheduler.schedule_sequential: a serial one-pod-at-a-time scheduler over k8s-shaped
dicts. Not the code under test and sharing nothing with it: nothing of constraints.py, snapshot.py or scheduler.py is
imported. Only scalar score arithmetic that the kernel tests already check is borrowed: oracle.normalize / _wrap64
(NodeNumber's totals), resource_score_ref.resource_score (Least / MostAllocated) and balanced_ref.bs (float64).

For each pod in order and each node in List order (node names sorted byte-wise, as the packer sorts them) it decides
feasibility, then the total; it takes the first maximum in List order and commits. The state is the snapshot and the
list `placed` of (node position, pod) placed against it, plus one flag (`term_seen`, see departure 6). Pod counts, used
amounts, a spread group's count per zone and the pods that match an inter-pod term in a topology domain are recomputed
from `placed` whenever a pod needs them.

The rules are restated from the published v1.22 sources: NodeUnschedulable (the toleration of
node.kubernetes.io/unschedulable:NoSchedule), NodeName, nodeSelector, required node affinity (matchExpressions with the
six operators, matchFields on metadata.name, empty terms and lists match nothing), TaintToleration (filter and the
PreferNoSchedule count), resource.Quantity parsing with `fractions` (decimal exponent form included), NodeResourcesFit
requests (sum over containers, maximum with each init container), allocatable.pods, PodTopologySpread's DoNotSchedule
skew rule over the zones present in the snapshot, the preferred node affinity sum, and InterPodAffinity's required
rules (own anti-affinity, the anti-affinity of existing pods, affinity with the first-pod exception; namespaces by
getNamespacesFromPodAffinityTerm).

Departures from upstream that this reference follows, each with the document it rests on:
 1. Existing pods are only the pods placed against the snapshot by earlier calls. Scheduler docstring: "Only pods placed
    by this scheduler against the snapshot are in the record".
 2. A hostname term makes every node its own domain, with or without the kubernetes.io/hostname label. Scheduler
    docstring: "The topologyKey of a term is kubernetes.io/hostname (every node is its own domain) or the `zones` label."
 3. A pod belongs to at most one spread group, named by its `spread_label` label, on the one topology key `zones`, and
    the group counts only pods placed against the snapshot; the minimum is over every zone of the snapshot. Scheduler
    docstring: "a pod belongs to the group named by its `spread_label` label ... placed only where its group's count in
    the node's zone stays within max_skew of the group's emptiest zone".
 4. A request of 0 is never checked, a node lacking an allocatable value has 0 of it, cpu is in milli-units and pod
    overhead is not included; pods that request nothing get no default request in the scores. Scheduler docstring: "a
    node lacking a value counts as 0", "The library substitutes no defaults for pods that request nothing".
 5. NodeNumber is a score plugin (the project's reference scheduler, not upstream): 10 where the last byte of the pod's
    and the node's name are the same digit; a pod whose name does not end in a digit is a SCORE_ERROR once it has a
    feasible node. DESIGN.md, the plugin list of the reference.
 6. The two preference scores are part of a pod's total only in a call made with schedule_sequential_prefs or a form
    above it: when a preference weight is set and the call holds a pod with a nonzero raw value on some node, or the
    balanced weight is set, or the snapshot has seen an inter-pod term. Scheduler docstring: "a call in which some pod
    has such a preference is made with DeviceContext.schedule_sequential_prefs; every other call takes the paths
    above", "With a nonzero weight every schedule_sequential call is DeviceContext.schedule_sequential_balanced", "Once
    the snapshot has a term, every pod of every later call ... is DeviceContext.schedule_sequential_podaffinity". In a
    call without them a pod's total lacks the constant 100 x prefer_no_schedule_weight; no placement depends on it.
 7. The balanced score is upstream's over the first two names of `resources`. Scheduler docstring: "the first two being
    the ones upstream balances".
 8. A grouped pod is never placed on a node without the zone label; a node without it is in no zone domain of an
    inter-pod term either (as upstream)."""
from __future__ import annotations

import re
from fractions import Fraction

import balanced_ref as BR
import resource_score_ref as RS

PLACED, FIT_ERROR, SCORE_ERROR = "PLACED", "FIT_ERROR", "SCORE_ERROR"
HOSTNAME = "kubernetes.io/hostname"
UNSCHEDULABLE_TAINT = {"key": "node.kubernetes.io/unschedulable", "value": "", "effect": "NoSchedule"}
INT32_MAX = 2**31 - 1
FILTERS = ("unschedulable", "capacity", "static", "resources", "spread", "interpod")

_NUMBER = re.compile(r"^([+-]?)(\d*)(?:\.(\d*))?(?:([eE][+-]?\d+)|(m|k|M|G|T|P|E|Ki|Mi|Gi|Ti|Pi|Ei))?$")
_SUFFIX = {"m": Fraction(1, 1000), "k": 10**3, "M": 10**6, "G": 10**9, "T": 10**12, "P": 10**15, "E": 10**18,
           "Ki": 2**10, "Mi": 2**20, "Gi": 2**30, "Ti": 2**40, "Pi": 2**50, "Ei": 2**60}


def quantity(s, milli=False) -> int:
    """apimachinery resource.Quantity: <sign><digits>[.<digits>] then a decimal exponent (e6, E-3), a decimal SI suffix
    or a binary suffix. Value() / MilliValue() round up (away from zero for what is positive)."""
    if isinstance(s, bool):
        raise ValueError(f"not a quantity: {s!r}")
    if isinstance(s, int):
        v = Fraction(s)
    else:
        m = _NUMBER.match(s.strip()) if isinstance(s, str) else None
        if m is None or not (m.group(2) or m.group(3)):
            raise ValueError(f"not a quantity: {s!r}")
        v = Fraction(int((m.group(2) or "0") + (m.group(3) or "")), 10 ** len(m.group(3) or ""))
        if m.group(4):
            v *= Fraction(10) ** int(m.group(4)[1:])
        elif m.group(5):
            v *= _SUFFIX[m.group(5)]
        if m.group(1) == "-":
            v = -v
    if milli:
        v *= 1000
    return -((-v.numerator) // v.denominator)  # the ceiling


def list_order(nodes) -> list:
    return sorted(nodes, key=lambda n: n["metadata"]["name"].encode("utf-8"))


def digit(name: str) -> int:
    c = name.encode("utf-8")[-1]
    return c - 48 if 48 <= c <= 57 else -1


def labels_of(obj) -> dict:
    return (obj.get("metadata") or {}).get("labels") or {}


def namespace_of(pod) -> str:
    return (pod.get("metadata") or {}).get("namespace") or "default"


def tolerates(tol, taint) -> bool:
    """Toleration.ToleratesTaint."""
    if tol.get("effect") and tol["effect"] != taint.get("effect", ""):
        return False
    if tol.get("key") and tol["key"] != taint.get("key", ""):
        return False
    op = tol.get("operator") or "Equal"
    if op == "Exists":
        return True
    return op == "Equal" and (tol.get("value") or "") == (taint.get("value") or "")


def tolerations_of(pod) -> list:
    return (pod.get("spec") or {}).get("tolerations") or []


def taints_of(node) -> list:
    return (node.get("spec") or {}).get("taints") or []


def _int64(s):
    if not re.fullmatch(r"[+-]?[0-9]+", s):
        return None
    v = int(s)
    return v if -2**63 <= v < 2**63 else None


def requirement_matches(e, labels, pod_selector=False) -> bool:
    """labels.Requirement.Matches after NewRequirement's validation; an invalid requirement matches nothing."""
    key, op, values = e.get("key", ""), e.get("operator", ""), [str(v) for v in e.get("values") or []]
    if op == "In":
        return bool(values) and key in labels and str(labels[key]) in values
    if op == "NotIn":
        return bool(values) and (key not in labels or str(labels[key]) not in values)
    if op == "Exists":
        return not values and key in labels
    if op == "DoesNotExist":
        return not values and key not in labels
    if op in ("Gt", "Lt") and not pod_selector:
        if len(values) != 1 or key not in labels:
            return False
        a, b = _int64(str(labels[key])), _int64(values[0])
        if a is None or b is None:
            return False
        return a > b if op == "Gt" else a < b
    return False


def node_term_matches(term, node) -> bool:
    exprs, fields = term.get("matchExpressions") or [], term.get("matchFields") or []
    if not exprs and not fields:
        return False
    for f in fields:
        values = [str(v) for v in f.get("values") or []]
        if f.get("key") != "metadata.name" or len(values) != 1 or f.get("operator") not in ("In", "NotIn"):
            return False
        if (node["metadata"]["name"] == values[0]) != (f["operator"] == "In"):
            return False
    return all(requirement_matches(e, labels_of(node)) for e in exprs)


def static_admits(pod, node) -> bool:
    """NodeName, nodeSelector, required node affinity, TaintToleration's filter."""
    spec = pod.get("spec") or {}
    if spec.get("nodeName") and spec["nodeName"] != node["metadata"]["name"]:
        return False
    nl = labels_of(node)
    for k, v in (spec.get("nodeSelector") or {}).items():
        if k not in nl or str(nl[k]) != str(v):
            return False
    req = ((spec.get("affinity") or {}).get("nodeAffinity") or {}).get("requiredDuringSchedulingIgnoredDuringExecution")
    if req is not None and not any(node_term_matches(t, node) for t in req.get("nodeSelectorTerms") or []):
        return False
    for taint in taints_of(node):
        if taint.get("effect") in ("NoSchedule", "NoExecute") and not any(tolerates(t, taint) for t in tolerations_of(pod)):
            return False
    return True


def preferred_sum(pod, node) -> int:
    pref = ((pod.get("spec") or {}).get("affinity") or {}).get("nodeAffinity") or {}
    return sum(int(t.get("weight") or 0) for t in pref.get("preferredDuringSchedulingIgnoredDuringExecution") or []
               if int(t.get("weight") or 0) and node_term_matches(t.get("preference") or {}, node))


def prefer_no_schedule(pod, node) -> int:
    tols = [t for t in tolerations_of(pod) if (t.get("effect") or "") in ("", "PreferNoSchedule")]
    return sum(1 for taint in taints_of(node)
               if taint.get("effect") == "PreferNoSchedule" and not any(tolerates(t, taint) for t in tols))


def requests(pod, names) -> list[int]:
    spec = pod.get("spec") or {}

    def of(c):
        r = (c.get("resources") or {}).get("requests") or {}
        return [quantity(r[nm], nm == "cpu") if r.get(nm) is not None else 0 for nm in names]
    total = [0] * len(names)
    for c in spec.get("containers") or []:
        total = [a + b for a, b in zip(total, of(c))]
    for c in spec.get("initContainers") or []:
        total = [max(a, b) for a, b in zip(total, of(c))]
    return total


def allocatable(node, names) -> list[int]:
    a = (node.get("status") or {}).get("allocatable") or {}
    return [quantity(a[nm], nm == "cpu") if a.get(nm) is not None else 0 for nm in names]


def selector_matches(sel, labels) -> bool:
    """metav1.LabelSelectorAsSelector: nil matches nothing, empty everything."""
    if sel is None:
        return False
    for k, v in (sel.get("matchLabels") or {}).items():
        if k not in labels or str(labels[k]) != str(v):
            return False
    return all(requirement_matches(e, labels, pod_selector=True) for e in sel.get("matchExpressions") or [])


def term_matches(term, owner, pod) -> bool:
    """AffinityTerm.Matches with getNamespacesFromPodAffinityTerm: no namespaces means the owner's own."""
    spaces = term.get("namespaces") or [namespace_of(owner)]
    return namespace_of(pod) in spaces and selector_matches(term.get("labelSelector"), labels_of(pod))


def pod_terms(pod, kind) -> list:
    return ((pod.get("spec") or {}).get("affinity") or {}).get(kind, {}).get(
        "requiredDuringSchedulingIgnoredDuringExecution") or []


class ClusterRef:
    def __init__(self, O, *, resources=None, resource_score=None, resource_score_weight=1, resource_weights=None,
                 zones=None, spread_groups=None, spread_label="app", preferred_affinity_weight=0,
                 prefer_no_schedule_weight=0, balanced_allocation_weight=0, nn_weight=1, nn_normalize=0):
        self.O = O
        self.resources = list(resources or ())
        self.mode = {None: 0, "least": RS.LEAST, "most": RS.MOST}[resource_score]
        self.rs_weight = resource_score_weight
        if isinstance(resource_weights, dict):
            resource_weights = [resource_weights.get(r, 0) for r in self.resources]
        self.rw = list(resource_weights or [1] * len(self.resources))
        self.zones, self.groups, self.spread_label = zones, dict(spread_groups or {}), spread_label
        self.w_aff, self.w_pns, self.w_bal = preferred_affinity_weight, prefer_no_schedule_weight, balanced_allocation_weight
        self.nn_weight, self.nn_normalize = nn_weight, nn_normalize
        self.nodes: list = []
        self.placed: list = []  # (node position in List order, pod)
        self.term_seen = False
        self.forget_before_first_term = False  # coverage only: the first term is evaluated against an empty record
        self.interpod_from = 0
        self.rejections = dict.fromkeys(FILTERS, 0)  # nodes a filter rejected that the filters before it had left
        self.first_pod = 0                           # pods the first-pod exception admitted

    def update_nodes(self, nodes):
        self.nodes = list_order(nodes)
        self.placed = []
        self.term_seen = False
        self.interpod_from = 0

    # -- derived from the placed list --
    def count(self, i) -> int:
        return sum(1 for k, _ in self.placed if k == i)

    def used(self, i) -> list[int]:
        tot = [0] * len(self.resources)
        for k, q in self.placed:
            if k == i:
                tot = [a + b for a, b in zip(tot, requests(q, self.resources))]
        return tot

    def zone(self, i):
        return labels_of(self.nodes[i]).get(self.zones) if self.zones is not None else None

    def group(self, pod):
        g = labels_of(pod).get(self.spread_label)
        return g if g in self.groups else None

    def group_count(self, g, z) -> int:
        return sum(1 for k, q in self.placed if self.group(q) == g and self.zone(k) == z)

    def zone_names(self) -> list:
        """The zones of the snapshot in the order in which List order first shows them."""
        out = []
        for i in range(len(self.nodes)):
            z = self.zone(i)
            if z is not None and z not in out:
                out.append(z)
        return out

    def domain(self, key, i):
        """The topology domain of node i for a term's topologyKey; None: the node lacks the key."""
        if key == HOSTNAME:
            return ("host", i)
        z = self.zone(i) if key == self.zones else None
        return None if z is None else ("zone", z)

    def view(self, pod) -> dict:
        """Everything the pod needs from the placed list, recomputed for this pod: pod counts and used amounts by node,
        its group's count by zone, and per inter-pod term the topology domains that hold a matching pod."""
        counts, used = {}, {}
        for k, q in self.placed:
            counts[k] = counts.get(k, 0) + 1
            if self.resources:
                used[k] = [a + b for a, b in zip(used.get(k, [0] * len(self.resources)), requests(q, self.resources))]
        g = self.group(pod) if self.zones is not None else None
        by_zone = {}
        if g is not None:
            by_zone = {z: self.group_count(g, z) for z in self.zone_names()}
        repelled = set()  # (topologyKey, domain) where an existing pod's anti-affinity term matches this pod
        existing = self.placed[self.interpod_from:]
        for k, e in existing:
            for t in pod_terms(e, "podAntiAffinity"):
                d = self.domain(t.get("topologyKey"), k)
                if d is not None and term_matches(t, e, pod):
                    repelled.add((t.get("topologyKey"), d))

        def holders(t):  # the domains that hold a pod matching the pod's own term t
            return {d for d in (self.domain(t.get("topologyKey"), k) for k, e in existing if term_matches(t, pod, e))
                    if d is not None}
        anti = [(t.get("topologyKey"), holders(t)) for t in pod_terms(pod, "podAntiAffinity")]
        aff = [(t.get("topologyKey"), holders(t)) for t in pod_terms(pod, "podAffinity")]
        # the first-pod exception: no existing pod matches any affinity term anywhere, and the pod matches them all
        first = bool(aff) and not any(h for _, h in aff) and all(term_matches(t, pod, pod)
                                                                 for t in pod_terms(pod, "podAffinity"))
        return dict(counts=counts, used=used, group=g, by_zone=by_zone, repelled=repelled, anti=anti, aff=aff, first=first)

    def interpod_ok(self, v, i, first_ok) -> bool:
        for key, d in v["repelled"]:  # the anti-affinity of existing pods
            if self.domain(key, i) == d:
                return False
        for key, held in v["anti"]:   # its own
            if self.domain(key, i) in held:
                return False
        for key, held in v["aff"]:
            d = self.domain(key, i)
            if d is None:
                return False
            if d not in held:
                return first_ok
        return True

    def used_on(self, v, i) -> list[int]:
        return v["used"].get(i, [0] * len(self.resources))

    def feasible(self, pod, max_pods_per_node, v=None, record=True) -> list[int]:
        v = self.view(pod) if v is None else v
        tol_unsched = any(tolerates(t, UNSCHEDULABLE_TAINT) for t in tolerations_of(pod))
        capped = any(((n.get("status") or {}).get("allocatable") or {}).get("pods") is not None for n in self.nodes)
        req = requests(pod, self.resources)
        g = v["group"]
        lowest = min(v["by_zone"].values(), default=0)
        out = []
        for i, node in enumerate(self.nodes):
            verdicts = {}
            verdicts["unschedulable"] = not (node.get("spec") or {}).get("unschedulable") or tol_unsched
            cap = None
            if capped:
                c = ((node.get("status") or {}).get("allocatable") or {}).get("pods")
                cap = INT32_MAX if c is None else int(c)
            if max_pods_per_node > 0:
                cap = max_pods_per_node if cap is None else min(cap, max_pods_per_node)
            verdicts["capacity"] = cap is None or v["counts"].get(i, 0) < cap
            verdicts["static"] = static_admits(pod, node)
            if any(r > 0 for r in req):
                al, us = allocatable(node, self.resources), self.used_on(v, i)
                verdicts["resources"] = all(r <= a - u for r, a, u in zip(req, al, us) if r > 0)
            else:
                verdicts["resources"] = True
            if g is not None:
                z = self.zone(i)
                verdicts["spread"] = z is not None and v["by_zone"][z] - lowest < self.groups[g]
            else:
                verdicts["spread"] = True
            verdicts["interpod"] = self.interpod_ok(v, i, v["first"])
            if all(verdicts.values()):
                out.append(i)
            elif record:
                bad = [f for f in FILTERS if not verdicts[f]]
                if len(bad) == 1:  # the only filter that rejects the node: it rejects what the others left
                    self.rejections[bad[0]] += 1
        return out

    def keyed(self, pods) -> bool:
        """Departure 6: whether the call's totals hold the two preference scores."""
        if not (self.w_aff or self.w_pns):
            return False
        if self.term_seen or self.w_bal:
            return True
        return any(preferred_sum(p, n) or prefer_no_schedule(p, n) for p in pods for n in self.nodes)

    def totals(self, pod, feas, keyed, v) -> list[int]:
        O = self.O
        pd = digit(pod["metadata"]["name"])
        raw = [10 if 0 <= digit(self.nodes[i]["metadata"]["name"]) == pd else 0 for i in feas]
        total = [O._wrap64(s * self.nn_weight) for s in O.normalize(self.nn_normalize, raw)]
        req = requests(pod, self.resources)
        if self.mode:
            for k, i in enumerate(feas):
                al, us = allocatable(self.nodes[i], self.resources), self.used_on(v, i)
                total[k] += self.rs_weight * RS.resource_score(self.mode, al, [u + r for u, r in zip(us, req)], self.rw)
        if keyed:
            ra = [preferred_sum(pod, self.nodes[i]) for i in feas]
            rt = [prefer_no_schedule(pod, self.nodes[i]) for i in feas]
            ma, mt = max(ra), max(rt)
            for k in range(len(feas)):
                total[k] += self.w_aff * (0 if ma == 0 else ra[k] * 100 // ma)
                total[k] += self.w_pns * (100 if mt == 0 else 100 - rt[k] * 100 // mt)
        if self.w_bal:
            for k, i in enumerate(feas):
                al, us = allocatable(self.nodes[i], self.resources), self.used_on(v, i)
                total[k] += self.w_bal * BR.bs(us[0] + req[0], al[0], us[1] + req[1], al[1])
        return total

    def schedule(self, pods, max_pods_per_node=0) -> list[tuple]:
        """(outcome, node name or None, score) per pod."""
        pods = list(pods)
        if any(pod_terms(p, "podAffinity") or pod_terms(p, "podAntiAffinity") for p in pods):
            if not self.term_seen and self.forget_before_first_term:
                self.interpod_from = len(self.placed)
            self.term_seen = True
        keyed = self.keyed(pods)
        out = []
        for pod in pods:
            v = self.view(pod)
            feas = self.feasible(pod, max_pods_per_node, v)
            if not feas:
                out.append((FIT_ERROR, None, 0))
                continue
            if digit(pod["metadata"]["name"]) < 0:
                out.append((SCORE_ERROR, None, 0))
                continue
            total = self.totals(pod, feas, keyed, v)
            best = max(total)
            sel = feas[total.index(best)]
            if v["aff"] and not self.interpod_ok(v, sel, False):
                self.first_pod += 1
            self.placed.append((sel, pod))
            out.append((PLACED, self.nodes[sel]["metadata"]["name"], best))
        return out

    # -- what the device's read-backs must show, from the placed list --
    def node_pod_counts(self) -> list[int]:
        return [self.count(i) for i in range(len(self.nodes))]

    def used_amounts(self) -> list[list[int]]:
        """[resource][node]."""
        per = [self.used(i) for i in range(len(self.nodes))]
        return [[u[r] for u in per] for r in range(len(self.resources))]

    def spread_counts(self) -> list[list[int]]:
        """[group][zone id], zone ids in the order List order first shows them, 64 wide."""
        zs = self.zone_names()
        return [[self.group_count(g, zs[z]) if z < len(zs) else 0 for z in range(64)] for g in self.groups]

    def affinity_words(self, terms) -> tuple[list[int], list[int]]:
        """(present, repel) per node for `terms`, a list of (term, owner namespace) in bit order."""
        n = len(self.nodes)
        present, repel = [0] * n, [0] * n
        for k, e in self.placed:
            for b, (t, owner_ns) in enumerate(terms):
                owner = {"metadata": {"namespace": owner_ns}}
                if term_matches(t, owner, e):
                    present[k] |= 1 << b
                if any(_same_term(t, owner_ns, u, namespace_of(e)) for u in pod_terms(e, "podAntiAffinity")):
                    repel[k] |= 1 << b
        return present, repel


def _same_term(t, t_ns, u, u_ns) -> bool:
    """Two terms that read the same: selector, namespaces and topology key."""
    return (t.get("labelSelector") == u.get("labelSelector") and t.get("topologyKey") == u.get("topologyKey")
            and sorted(set(t.get("namespaces") or [t_ns])) == sorted(set(u.get("namespaces") or [u_ns])))
