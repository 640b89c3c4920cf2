"""Static node filters of the v1.22 default profile, evaluated on the host: NodeName, nodeSelector, required node
affinity and TaintToleration. Their verdict for a (pod, node) pair depends only on the pod's spec and the node's
name, labels and taints, never on a commit, so the scheduler evaluates them once per (class of pods, node) and
hands the device one bit per pair (DeviceContext.upload_node_class_bits).

The rules are restated from the published v1.22 sources; each function cites the file and function it follows.
Objects are k8s-shaped dicts or attribute objects, as in snapshot.py: a node gives metadata.name, metadata.labels
and spec.taints (or the attributes name, labels, taints), a pod gives spec.nodeName, spec.nodeSelector,
spec.affinity.nodeAffinity.requiredDuringSchedulingIgnoredDuringExecution.nodeSelectorTerms and spec.tolerations (or
the attributes node_name, node_selector, node_affinity_terms, tolerations).
"""
from __future__ import annotations

import json
import re
from typing import Any, Mapping

from .snapshot import _get, _tol_field, node_name, pod_tolerations

_INT64 = re.compile(r"^[+-]?[0-9]+$")  # what strconv.ParseInt(s, 10, 64) takes, before its range check
_REQUIRED = ("affinity", "nodeAffinity", "requiredDuringSchedulingIgnoredDuringExecution")


def node_labels(n: Any) -> Mapping[str, str]:
    v = n.labels if hasattr(n, "labels") else _get(n, "metadata", "labels")
    return v or {}


def node_taints(n: Any) -> list:
    v = n.taints if hasattr(n, "taints") else _get(n, "spec", "taints")
    return list(v or ())


def pod_node_name(p: Any) -> str:
    v = p.node_name if hasattr(p, "node_name") else _get(p, "spec", "nodeName")
    return v or ""


def pod_node_selector(p: Any) -> Mapping[str, str]:
    v = p.node_selector if hasattr(p, "node_selector") else _get(p, "spec", "nodeSelector")
    return v or {}


def pod_affinity_terms(p: Any) -> list | None:
    """The required node affinity's nodeSelectorTerms; None when the pod has no required node affinity (an empty
    list is a required affinity that matches nothing)."""
    if hasattr(p, "node_affinity_terms"):
        return None if p.node_affinity_terms is None else list(p.node_affinity_terms)
    req = _get(p, "spec", *_REQUIRED)
    if req is None:
        return None
    return list(_get(req, "nodeSelectorTerms", default=()) or ())


def _parse_int64(s: Any) -> int | None:
    if not isinstance(s, str) or not _INT64.match(s):
        return None
    v = int(s)
    return v if -(1 << 63) <= v < (1 << 63) else None


def fits_node_name(pod: Any, node: Any) -> bool:
    """pkg/scheduler/framework/plugins/nodename/node_name.go: Fits. spec.nodeName is empty or the node's name."""
    want = pod_node_name(pod)
    return want == "" or want == node_name(node)


def matches_node_selector(pod: Any, node: Any) -> bool:
    """component-helpers/scheduling/corev1/nodeaffinity/nodeaffinity.go: GetRequiredNodeAffinity and
    RequiredNodeAffinity.Match, the labelSelector half (labels.SelectorFromSet of spec.nodeSelector): every
    key / value pair is present and equal in the node's labels."""
    labels = node_labels(node)
    return all(k in labels and str(labels[k]) == str(v) for k, v in pod_node_selector(pod).items())


def _expression_matches(e: Any, labels: Mapping[str, str]) -> bool:
    """component-helpers/scheduling/corev1/nodeaffinity/nodeaffinity.go: nodeSelectorRequirementsAsSelector, then
    apimachinery/pkg/labels/selector.go: NewRequirement (what makes a requirement invalid) and Requirement.Matches.
    An invalid requirement makes its term match nothing; here it is simply false, which ANDs to the same."""
    key, op = _get(e, "key", default=""), _get(e, "operator", default="")
    values = [str(v) for v in (_get(e, "values", default=()) or ())]
    has = key in labels
    if op == "In":
        return bool(values) and has and str(labels[key]) in values
    if op == "NotIn":  # matches when the label is absent
        return bool(values) and not (has and str(labels[key]) in values)
    if op == "Exists":
        return not values and has
    if op == "DoesNotExist":
        return not values and not has
    if op in ("Gt", "Lt"):  # exactly one value; both sides base-10 int64, anything else is no match
        if len(values) != 1 or not has:
            return False
        lhs, rhs = _parse_int64(str(labels[key])), _parse_int64(values[0])
        if lhs is None or rhs is None:
            return False
        return lhs > rhs if op == "Gt" else lhs < rhs
    return False


def _field_matches(e: Any, name: str) -> bool:
    """component-helpers/scheduling/corev1/nodeaffinity/nodeaffinity.go: nodeSelectorRequirementsAsFieldSelector.
    metadata.name only, In / NotIn only, with exactly one value; anything else is invalid and matches nothing."""
    values = [str(v) for v in (_get(e, "values", default=()) or ())]
    if _get(e, "key", default="") != "metadata.name" or len(values) != 1:
        return False
    op = _get(e, "operator", default="")
    if op == "In":
        return name == values[0]
    if op == "NotIn":
        return name != values[0]
    return False


def matches_node_affinity(pod: Any, node: Any) -> bool:
    """component-helpers/scheduling/corev1/nodeaffinity/nodeaffinity.go: NodeSelector.Match (LazyErrorNodeSelector)
    over requiredDuringSchedulingIgnoredDuringExecution.nodeSelectorTerms: terms are ORed; within a term
    matchExpressions and matchFields are ANDed; a term with neither matches nothing (newNodeSelectorTerm /
    isEmptyNodeSelectorTerm), and so does an empty term list. No required affinity matches every node."""
    terms = pod_affinity_terms(pod)
    if terms is None:
        return True
    labels, name = node_labels(node), node_name(node)
    for t in terms:
        exprs = list(_get(t, "matchExpressions", default=()) or ())
        fields = list(_get(t, "matchFields", default=()) or ())
        if not exprs and not fields:
            continue
        if all(_expression_matches(e, labels) for e in exprs) and all(_field_matches(f, name) for f in fields):
            return True
    return False


def toleration_tolerates_taint(tol: Any, taint: Any) -> bool:
    """k8s.io/api/core/v1/toleration.go: Toleration.ToleratesTaint. An empty effect or the taint's effect; an empty
    key or the taint's key (validation admits an empty key with operator Exists only); then Exists is true and
    Equal, or an empty operator, compares the values."""
    effect, key = _tol_field(tol, "effect"), _tol_field(tol, "key")
    if effect and effect != _tol_field(taint, "effect"):
        return False
    if key and key != _tol_field(taint, "key"):
        return False
    op = _tol_field(tol, "operator", "op")
    if op in ("", "Equal"):
        return _tol_field(tol, "value") == _tol_field(taint, "value")
    return op == "Exists"


def tolerates_node_taints(pod: Any, node: Any) -> bool:
    """pkg/scheduler/framework/plugins/tainttoleration/taint_toleration.go: Filter (with
    component-helpers/scheduling/corev1/helpers.go: FindMatchingUntoleratedTaint): every taint of spec.taints with
    effect NoSchedule or NoExecute is tolerated by some toleration; PreferNoSchedule never filters.
    spec.unschedulable is NodeUnschedulable's business, through the pod table's tolerates bit."""
    tols = pod_tolerations(pod)
    for taint in node_taints(node):
        if _tol_field(taint, "effect") not in ("NoSchedule", "NoExecute"):
            continue
        if not any(toleration_tolerates_taint(t, taint) for t in tols):
            return False
    return True


def node_admits(pod: Any, node: Any) -> bool:
    """The AND of the four static filters: NodeName, nodeSelector, required node affinity, TaintToleration."""
    return (fits_node_name(pod, node) and matches_node_selector(pod, node) and matches_node_affinity(pod, node)
            and tolerates_node_taints(pod, node))


_PREFERRED = ("affinity", "nodeAffinity", "preferredDuringSchedulingIgnoredDuringExecution")


def pod_preferred_terms(p: Any) -> list:
    """The preferred node affinity's terms, each with `weight` and `preference` (a NodeSelectorTerm); empty without
    one. Attribute objects give node_affinity_preferred."""
    if hasattr(p, "node_affinity_preferred"):
        return list(p.node_affinity_preferred or ())
    return list(_get(p, "spec", *_PREFERRED, default=()) or ())


def _term_matches(term: Any, labels: Mapping[str, str], name: str) -> bool | None:
    """One NodeSelectorTerm against a node, by matches_node_affinity's rules; None for a term with neither
    matchExpressions nor matchFields."""
    exprs = list(_get(term, "matchExpressions", default=()) or ())
    fields = list(_get(term, "matchFields", default=()) or ())
    if not exprs and not fields:
        return None
    return all(_expression_matches(e, labels) for e in exprs) and all(_field_matches(f, name) for f in fields)


def preferred_affinity_score(pod: Any, node: Any) -> int:
    """pkg/scheduler/framework/plugins/nodeaffinity/node_affinity.go: Score, with
    component-helpers/scheduling/corev1/nodeaffinity/nodeaffinity.go: NewPreferredSchedulingTerms and
    PreferredSchedulingTerms.Score. The sum of `weight` over the preferred terms whose `preference` matches the node;
    a term of weight 0, or whose preference has neither matchExpressions nor matchFields, is skipped."""
    labels, name = node_labels(node), node_name(node)
    total = 0
    for t in pod_preferred_terms(pod):
        w = int(_get(t, "weight", default=0) or 0)
        if w == 0:
            continue
        if _term_matches(_get(t, "preference", default={}) or {}, labels, name):
            total += w
    return total


def prefer_no_schedule_count(pod: Any, node: Any) -> int:
    """pkg/scheduler/framework/plugins/tainttoleration/taint_toleration.go: Score, with
    getAllTolerationPreferNoSchedule and countIntolerableTaintsPreferNoSchedule. The node's taints of effect
    PreferNoSchedule that none of the pod's tolerations with an empty effect or effect PreferNoSchedule tolerates."""
    tols = [t for t in pod_tolerations(pod) if _tol_field(t, "effect") in ("", "PreferNoSchedule")]
    return sum(1 for taint in node_taints(node)
               if _tol_field(taint, "effect") == "PreferNoSchedule"
               and not any(toleration_tolerates_taint(t, taint) for t in tols))


def preference_key(pod: Any) -> str:
    """The canonical form of what preferred_affinity_score and prefer_no_schedule_count read from a pod: the
    preferred terms in order, and the tolerations as class_key reduces them. Pods with equal keys get equal raw
    values on every node."""
    tols = sorted([_tol_field(t, "key"), _tol_field(t, "operator", "op"), _tol_field(t, "value"),
                   _tol_field(t, "effect")] for t in pod_tolerations(pod))
    return json.dumps([_plain(pod_preferred_terms(pod)), tols], sort_keys=True)


SPREAD_MODES = {"DoNotSchedule": 0, "ScheduleAnyway": 1}  # MSH_SPREAD_DO_NOT_SCHEDULE / MSH_SPREAD_SCHEDULE_ANYWAY


def spread_mode(pod: Any, topology_key: str) -> int | None:
    """The mode of the pod's topology spread constraint on `topology_key` as DeviceContext.set_spread_group_modes
    takes it: spec.topologySpreadConstraints[*].whenUnsatisfiable of the first constraint with that key, DoNotSchedule
    (the API's default, also for an absent field) -> 0, ScheduleAnyway -> 1. None when the pod has no constraint on
    the key; any other value raises ValueError (the API server rejects it)."""
    if hasattr(pod, "topology_spread_constraints"):
        cons = pod.topology_spread_constraints
    else:
        cons = _get(pod, "spec", "topologySpreadConstraints")
    for con in cons or ():
        if _get(con, "topologyKey") != topology_key:
            continue
        when = _get(con, "whenUnsatisfiable") or "DoNotSchedule"
        if when not in SPREAD_MODES:
            raise ValueError(f"whenUnsatisfiable is DoNotSchedule or ScheduleAnyway, not {when!r}")
        return SPREAD_MODES[when]
    return None


def _plain(x: Any) -> Any:
    """A JSON-able copy of the public fields of x (dicts, sequences, attribute objects)."""
    if isinstance(x, Mapping):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if x is None or isinstance(x, (str, int, float, bool)):
        return x
    return {k: _plain(v) for k, v in vars(x).items() if not k.startswith("_")}


def class_key(pod: Any) -> str:
    """The canonical form of what node_admits reads from a pod: (nodeName, nodeSelector, required affinity,
    tolerations). Pods with equal keys get equal verdicts on every node. Tolerations are reduced to their four
    fields and sorted (their order does not matter to the filter); affinity terms keep their order."""
    tols = sorted([_tol_field(t, "key"), _tol_field(t, "operator", "op"), _tol_field(t, "value"),
                   _tol_field(t, "effect")] for t in pod_tolerations(pod))
    sel = sorted((str(k), str(v)) for k, v in pod_node_selector(pod).items())
    return json.dumps([pod_node_name(pod), sel, _plain(pod_affinity_terms(pod)), tols], sort_keys=True)


# ---- required inter-pod affinity and anti-affinity (the filter half of InterPodAffinity) ----

HOSTNAME_LABEL = "kubernetes.io/hostname"
_POD_AFFINITY = ("affinity", "podAffinity", "requiredDuringSchedulingIgnoredDuringExecution")
_POD_ANTI_AFFINITY = ("affinity", "podAntiAffinity", "requiredDuringSchedulingIgnoredDuringExecution")


def pod_labels(p: Any) -> Mapping[str, str]:
    v = p.labels if hasattr(p, "labels") else _get(p, "metadata", "labels")
    return v or {}


def pod_namespace(p: Any) -> str:
    """metadata.namespace; an object without one is in "default", as the API server would have put it."""
    v = p.namespace if hasattr(p, "namespace") else _get(p, "metadata", "namespace")
    return v or "default"


def _pod_name(p: Any) -> str:
    v = p.name if hasattr(p, "name") else _get(p, "metadata", "name")
    return v or "<unnamed>"


def pod_required_pod_affinity(p: Any) -> list:
    """spec.affinity.podAffinity.requiredDuringSchedulingIgnoredDuringExecution: a list of PodAffinityTerms, empty
    without one. Attribute objects give pod_affinity_required."""
    if hasattr(p, "pod_affinity_required"):
        return list(p.pod_affinity_required or ())
    return list(_get(p, "spec", *_POD_AFFINITY, default=()) or ())


def pod_required_pod_anti_affinity(p: Any) -> list:
    """spec.affinity.podAntiAffinity.requiredDuringSchedulingIgnoredDuringExecution, as pod_required_pod_affinity.
    Attribute objects give pod_anti_affinity_required."""
    if hasattr(p, "pod_anti_affinity_required"):
        return list(p.pod_anti_affinity_required or ())
    return list(_get(p, "spec", *_POD_ANTI_AFFINITY, default=()) or ())


def label_selector_matches(selector: Any, labels: Mapping[str, str]) -> bool:
    """apimachinery/pkg/apis/meta/v1/helpers.go: LabelSelectorAsSelector, then labels.Selector.Matches. A nil selector
    matches nothing, an empty one everything; matchLabels and matchExpressions (In, NotIn, Exists, DoesNotExist) are
    ANDed. NotIn and DoesNotExist match when the key is absent. Any other operator, In / NotIn without values, or
    Exists / DoesNotExist with values is invalid there; here it matches nothing."""
    if selector is None:
        return False
    for k, v in (_get(selector, "matchLabels", default=None) or {}).items():
        if k not in labels or str(labels[k]) != str(v):
            return False
    for e in _get(selector, "matchExpressions", default=()) or ():
        if _get(e, "operator", default="") not in ("In", "NotIn", "Exists", "DoesNotExist"):
            return False
        if not _expression_matches(e, labels):
            return False
    return True


def term_namespaces(term: Any, owner_namespace: str) -> list[str]:
    """pkg/scheduler/framework/types.go: getNamespacesFromPodAffinityTerm. An empty `namespaces` list (with no
    namespaceSelector) means the namespace of the pod that owns the term."""
    ns = [str(x) for x in (_get(term, "namespaces", default=()) or ())]
    return sorted(set(ns)) if ns else [owner_namespace]


def term_matches_pod(term: Any, term_owner_namespace: str, pod: Any) -> bool:
    """pkg/scheduler/framework/types.go: AffinityTerm.Matches: the pod's namespace is one of the term's and the term's
    labelSelector matches the pod's labels."""
    if pod_namespace(pod) not in term_namespaces(term, term_owner_namespace):
        return False
    return label_selector_matches(_get(term, "labelSelector", default=None), pod_labels(pod))


def term_key(term: Any, owner_namespace: str) -> str:
    """The canonical form of what term_matches_pod and the topology read from a term: terms with equal keys are one
    term of the device's table."""
    return json.dumps([_plain(_get(term, "labelSelector", default=None)), term_namespaces(term, owner_namespace),
                       _get(term, "topologyKey", default="")], sort_keys=True)


def check_pod_affinity(pod: Any, zone_label: str | None) -> tuple[list, list]:
    """(the pod's required affinity terms, its required anti-affinity terms), after refusing what the device's bit form
    cannot hold exactly (ValueError naming the pod): a non-empty namespaceSelector, a topologyKey other than
    kubernetes.io/hostname or the scheduler's zone label, more than one required affinity term (upstream counts only
    the existing pods that match all of them: one bit per term cannot say that)."""
    aff, anti = pod_required_pod_affinity(pod), pod_required_pod_anti_affinity(pod)
    who = f"pod {pod_namespace(pod)}/{_pod_name(pod)}"
    for t in aff + anti:
        sel = _get(t, "namespaceSelector", default=None)
        if sel is not None and (_get(sel, "matchLabels", default=None) or _get(sel, "matchExpressions", default=None)):
            raise ValueError(f"{who}: a non-empty namespaceSelector in a required pod (anti-)affinity term is not supported")
        key = _get(t, "topologyKey", default="")
        if key != HOSTNAME_LABEL and (zone_label is None or key != zone_label):
            raise ValueError(f"{who}: topologyKey {key!r} is neither {HOSTNAME_LABEL!r} nor the scheduler's zone label "
                             f"{zone_label!r}")
    if len(aff) > 1:
        raise ValueError(f"{who}: {len(aff)} required pod affinity terms; one term per pod is supported (upstream matches "
                         "an existing pod against all of them at once)")
    return aff, anti
