"""Per-class node masks in sequential-commit mode, the parts that need no GPU: the two CPU references of
tests/classes_ref.py against each other and against spread_score_ref, the pure-Python constraint evaluator
(constraints.node_admits) rule by rule, the Scheduler's class-id assignment on a recording ctx, and the header
against the binding."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import classes_ref as KR
import node_capacity_ref as CR
import spread_ref as S
import spread_score_ref as X

NEW_SYMBOLS = ["msh_upload_node_class_bits", "msh_patch_node_class_bits", "msh_clear_node_class_bits",
               "msh_node_class_bits", "msh_seq_classes_max_nodes", "msh_schedule_sequential_classes",
               "msh_schedule_sequential_classes_device"]
SWEEP_SEEDS = range(12000, 12150)
NAMES = ("idx", "score", "status", "counts", "used", "cnt")


def case_args(c):
    """gen_case's dict as the references' positional arguments up to rw."""
    return (c["unsched"], c["node_digit"], c["pod_digit"], c["pod_tol"]), CR.effective(c["cap"]), \
        (c["alloc"], np.zeros_like(c["alloc"]), c["req"]), (c["zone"], c["group"], c["max_skew"]), \
        (c["score_mode"], c["rs_weight"], c["rw"])


def case_plugins(oracle, c):
    return oracle.PluginSet(weights=[c["weight"]], normalize=[c["mode"]])


def same(a, b, what):
    for x, y, nm in zip(a, b, NAMES):
        assert np.array_equal(np.asarray(x), np.asarray(y)), f"{what}: {nm} differs"


def test_new_symbols_are_declared_exported_and_bound(msh):
    header = (Path(__file__).resolve().parent.parent / "include" / "minisched_hip.h").read_text()
    lib = msh._native.lib()
    for nm in NEW_SYMBOLS:
        assert re.search(r"^int " + nm + r"\(", header, re.M), f"{nm} is not declared in the header"
        assert nm in msh._native.EXPORTED and hasattr(lib, nm), nm
        assert nm in msh._native._SIGS
    m = re.search(r"^#define MSH_MAX_POD_CLASSES (\d+)", header, re.M)
    assert m and int(m.group(1)) == msh._native.MAX_POD_CLASSES == KR.MAX_CLASSES == 64
    # the argument counts of the two calls: _spread_scored's and one more pointer
    sigs = msh._native._SIGS
    assert len(sigs["msh_schedule_sequential_classes"][1]) == len(sigs["msh_schedule_sequential_spread_scored"][1]) + 1
    assert len(sigs["msh_schedule_sequential_classes_device"][1]) == \
        len(sigs["msh_schedule_sequential_spread_scored_device"][1]) + 1
    # argument checks that need no device: a NULL ctx is MSH_ERR_INVALID
    inv = msh._native.MSH_ERR_INVALID
    assert lib.msh_upload_node_class_bits(None, 0, 1, None) == inv
    assert lib.msh_patch_node_class_bits(None, 0, None, None) == inv
    assert lib.msh_clear_node_class_bits(None) == inv
    assert lib.msh_node_class_bits(None, None, None, None) == inv
    assert lib.msh_seq_classes_max_nodes(None, 0, None) == inv


def test_per_pod_equals_serial_on_200_seeds(oracle):
    kinds, placed, fit, modes, sizes = set(), 0, 0, set(), set()
    for seed in range(210):
        c = KR.gen_case(seed, max_n=40, max_p=60)
        assert 1 <= c["C"] <= 64 and c["pod_class"].min() >= -1 and c["pod_class"].max() < c["C"]
        assert not (c["bits"] >> np.uint64(c["C"] - 1) >> np.uint64(1)).any(), "a bit at or above C"
        ps = case_plugins(oracle, c)
        cols, eff, res, sp, sc = case_args(c)
        extra = (c["bits"], c["C"], c["pod_class"])
        a = KR.serial(oracle, *cols, ps, eff, *res, *sp, *sc, *extra)
        b = KR.per_pod(oracle, *cols, ps, eff, *res, *sp, *sc, *extra)
        same(a, b, f"seed {seed}")
        kinds |= set(c["kinds"])
        modes.add(c["score_mode"])
        sizes.add(c["C"])
        placed += int((a[2] == KR.PLACED).sum())
        fit += int((a[2] == KR.FIT_ERROR).sum())
    assert kinds == set(KR.DENSITIES) and modes == {KR.NONE, KR.LEAST, KR.MOST} and {1, 64} <= sizes
    assert placed > 1000 and fit > 1000


def test_absent_inputs_are_no_zone_no_group_no_class(oracle):
    """zone None is a column of -1, group None a column of -1, pod_class None a column of -1."""
    for seed in range(20):
        c = KR.gen_case(seed, max_n=40, max_p=60)
        ps = case_plugins(oracle, c)
        cols, eff, res, sp, sc = case_args(c)
        n, p = c["n"], c["p"]
        for ref in (KR.serial, KR.per_pod):
            a = ref(oracle, *cols, ps, eff, *res, None, None, c["max_skew"], *sc, c["bits"], c["C"], None)
            b = ref(oracle, *cols, ps, eff, *res, np.full(n, -1), np.full(p, -1), c["max_skew"], *sc, c["bits"], c["C"],
                    np.full(p, -1))
            same(a, b, f"seed {seed}")


@pytest.mark.parametrize("how", ["every class admits every node", "every pod of class -1", "classes out of range"])
def test_without_effective_classes_the_call_is_spread_scored(oracle, how):
    for seed in range(40):
        c = KR.gen_case(seed, max_n=40, max_p=60)
        ps = case_plugins(oracle, c)
        cols, eff, res, sp, sc = case_args(c)
        bits, pod_class = c["bits"], c["pod_class"]
        if how == "every class admits every node":
            full = np.uint64((1 << c["C"]) - 1)
            bits = np.full(c["n"], full, np.uint64)
        elif how == "every pod of class -1":
            pod_class = np.full(c["p"], -1, np.int32)
        else:
            pod_class = np.where(np.arange(c["p"]) % 2 == 0, c["C"], -7).astype(np.int32)
        want = X.serial(oracle, *cols, ps, eff, *res, *sp, *sc)
        same(KR.serial(oracle, *cols, ps, eff, *res, *sp, *sc, bits, c["C"], pod_class), want, f"serial, seed {seed}")
        same(KR.per_pod(oracle, *cols, ps, eff, *res, *sp, *sc, bits, c["C"], pod_class), want, f"per_pod, seed {seed}")


def test_the_sweep_makes_the_classes_decide(oracle):
    """In most sweep cases the placements differ from the class-free call's, and pods are both placed and refused."""
    differ = 0
    seeds = list(SWEEP_SEEDS)[:30]
    for seed in seeds:
        c = KR.gen_case(seed)
        assert c["n"] <= 2048 and c["p"] <= 2000
        ps = case_plugins(oracle, c)
        cols, eff, res, sp, sc = case_args(c)
        a = KR.per_pod(oracle, *cols, ps, eff, *res, *sp, *sc, c["bits"], c["C"], c["pod_class"])
        b = X.per_pod(oracle, *cols, ps, eff, *res, *sp, *sc)
        differ += bool((a[0] != b[0]).any())
    assert 2 * differ >= len(seeds)


# ---- constraints.node_admits, one table per rule ----

def node(name="n1", labels=None, taints=None):
    return {"metadata": {"name": name, "labels": labels or {}}, "spec": {"taints": taints or []}}


def pod(node_name=None, selector=None, terms=None, tolerations=None):
    spec = {}
    if node_name is not None:
        spec["nodeName"] = node_name
    if selector is not None:
        spec["nodeSelector"] = selector
    if terms is not None:
        spec["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": terms}}}
    if tolerations is not None:
        spec["tolerations"] = tolerations
    return {"metadata": {"name": "p"}, "spec": spec}


def expr(key, op, *values):
    return {"key": key, "operator": op, "values": list(values)}


def term(*exprs, fields=()):
    t = {}
    if exprs:
        t["matchExpressions"] = list(exprs)
    if fields:
        t["matchFields"] = list(fields)
    return t


def test_node_name(msh):
    adm = msh.node_admits
    assert adm(pod(), node("a")) and adm(pod(node_name=""), node("a"))
    assert adm(pod(node_name="a"), node("a")) and not adm(pod(node_name="b"), node("a"))


def test_node_selector(msh):
    adm = msh.node_admits
    n = node(labels={"pool": "gpu", "zone": "z1"})
    assert adm(pod(selector={}), n) and adm(pod(selector={"pool": "gpu"}), n)
    assert adm(pod(selector={"pool": "gpu", "zone": "z1"}), n)
    assert not adm(pod(selector={"pool": "cpu"}), n)          # present, not equal
    assert not adm(pod(selector={"pool": "gpu", "disk": "ssd"}), n)  # one pair absent
    assert not adm(pod(selector={"pool": "gpu"}), node())     # no labels at all


@pytest.mark.parametrize("terms,labels,name,want", [
    ([], {"a": "1"}, "n1", False),                                       # an empty term list matches nothing
    ([term()], {"a": "1"}, "n1", False),                                 # the empty term matches nothing
    ([term(), term(expr("a", "In", "1"))], {"a": "1"}, "n1", True),      # terms are ORed, the empty one skipped
    ([term(expr("a", "In", "1", "2"))], {"a": "2"}, "n1", True),
    ([term(expr("a", "In", "1", "2"))], {"a": "3"}, "n1", False),
    ([term(expr("a", "In", "1"))], {}, "n1", False),                     # In on an absent label
    ([term(expr("a", "NotIn", "1"))], {"a": "2"}, "n1", True),
    ([term(expr("a", "NotIn", "1"))], {"a": "1"}, "n1", False),
    ([term(expr("a", "NotIn", "1"))], {}, "n1", True),                   # NotIn matches when the label is absent
    ([term(expr("a", "Exists"))], {"a": ""}, "n1", True),
    ([term(expr("a", "Exists"))], {}, "n1", False),
    ([term(expr("a", "DoesNotExist"))], {}, "n1", True),
    ([term(expr("a", "DoesNotExist"))], {"a": "x"}, "n1", False),
    ([term(expr("a", "Gt", "5"))], {"a": "6"}, "n1", True),
    ([term(expr("a", "Gt", "5"))], {"a": "5"}, "n1", False),
    ([term(expr("a", "Lt", "5"))], {"a": "-3"}, "n1", True),
    ([term(expr("a", "Lt", "5"))], {"a": "5"}, "n1", False),
    ([term(expr("a", "Gt", "five"))], {"a": "6"}, "n1", False),          # an unparsable Gt value
    ([term(expr("a", "Gt", "5"))], {"a": "6.0"}, "n1", False),           # an unparsable label value
    ([term(expr("a", "Gt", "5"))], {"a": str(2**63)}, "n1", False),      # outside int64
    ([term(expr("a", "Gt", "5", "6"))], {"a": "7"}, "n1", False),        # Gt takes exactly one value
    ([term(expr("a", "Gt"))], {"a": "7"}, "n1", False),
    ([term(expr("a", "Gt", "5"))], {}, "n1", False),
    ([term(expr("a", "In", "1"), expr("b", "Exists"))], {"a": "1"}, "n1", False),          # expressions are ANDed
    ([term(expr("a", "In", "1"), expr("b", "Exists"))], {"a": "1", "b": ""}, "n1", True),
    ([term(expr("a", "In", "9")), term(expr("b", "Exists"))], {"b": ""}, "n1", True),      # terms are ORed
    ([term(expr("a", "Near", "1"))], {"a": "1"}, "n1", False),                             # an unknown operator
    ([term(fields=[expr("metadata.name", "In", "n1")])], {}, "n1", True),
    ([term(fields=[expr("metadata.name", "In", "n2")])], {}, "n1", False),
    ([term(fields=[expr("metadata.name", "NotIn", "n2")])], {}, "n1", True),
    ([term(fields=[expr("metadata.name", "NotIn", "n1")])], {}, "n1", False),
    ([term(fields=[expr("metadata.name", "Exists")])], {}, "n1", False),                   # In / NotIn only
    ([term(fields=[expr("metadata.uid", "In", "n1")])], {}, "n1", False),                  # metadata.name only
    ([term(expr("a", "In", "1"), fields=[expr("metadata.name", "In", "n2")])], {"a": "1"}, "n1", False),  # ANDed
    ([term(expr("a", "In", "1"), fields=[expr("metadata.name", "In", "n1")])], {"a": "1"}, "n1", True),
])
def test_required_node_affinity(msh, terms, labels, name, want):
    assert msh.node_admits(pod(terms=terms), node(name, labels)) is want


def test_no_required_affinity_matches_every_node(msh):
    assert msh.node_admits(pod(), node()) and msh.node_admits({"metadata": {"name": "p"}, "spec": {"affinity": {}}}, node())


def taint(key, value="", effect="NoSchedule"):
    return {"key": key, "value": value, "effect": effect}


def tol(key="", op="", value="", effect=""):
    return {"key": key, "operator": op, "value": value, "effect": effect}


@pytest.mark.parametrize("taints,tols,want", [
    ([], [], True),
    ([taint("k", "v")], [], False),
    ([taint("k", "v", "NoExecute")], [], False),
    ([taint("k", "v", "PreferNoSchedule")], [], True),                          # PreferNoSchedule never filters
    ([taint("k", "v")], [tol("k", "Equal", "v", "NoSchedule")], True),
    ([taint("k", "v")], [tol("k", "", "v")], True),                             # an empty operator is Equal, an empty effect any
    ([taint("k", "v")], [tol("k", "Equal", "w")], False),
    ([taint("k", "v")], [tol("k", "Exists")], True),
    ([taint("k", "v")], [tol("j", "Exists")], False),
    ([taint("k", "v")], [tol("k", "Exists", effect="NoExecute")], False),       # another effect
    ([taint("k", "v"), taint("j", "", "NoExecute")], [tol("", "Exists")], True),   # an empty key with Exists: every taint
    ([taint("k", "v")], [tol("k", "Matches", "v")], False),                     # an unknown operator
    ([taint("k", "v"), taint("j")], [tol("k", "Exists")], False),               # every filtering taint must be tolerated
    ([taint("k", "v"), taint("j")], [tol("k", "Exists"), tol("j", "Equal", "")], True),
    ([taint("k", "v"), taint("j", "", "PreferNoSchedule")], [tol("k", "Exists")], True),
])
def test_taint_toleration(msh, taints, tols, want):
    assert msh.node_admits(pod(tolerations=tols), node(taints=taints)) is want


def test_spec_unschedulable_is_not_this_filters_business(msh):
    n = node()
    n["spec"]["unschedulable"] = True
    assert msh.node_admits(pod(), n)


def test_node_admits_is_the_and_of_the_four(msh):
    n = node("n1", {"pool": "gpu"}, [taint("dedicated", "ml")])
    good = dict(node_name="n1", selector={"pool": "gpu"}, terms=[term(expr("pool", "Exists"))],
                tolerations=[tol("dedicated", "Equal", "ml")])
    assert msh.node_admits(pod(**good), n)
    for key, bad in (("node_name", "n2"), ("selector", {"pool": "cpu"}), ("terms", []), ("tolerations", [])):
        assert not msh.node_admits(pod(**{**good, key: bad}), n), key


def test_attribute_objects(msh):
    class Obj:
        def __init__(self, **kw):
            self.__dict__.update(kw)
    n = Obj(name="n1", labels={"a": "1"}, taints=[Obj(key="k", value="v", effect="NoSchedule")])
    p = Obj(name="p", node_name="", node_selector={"a": "1"}, node_affinity_terms=None,
            tolerations=[Obj(key="k", operator="Exists", value="", effect="")])
    assert msh.node_admits(p, n)
    p.tolerations = []
    assert not msh.node_admits(p, n)
    p.node_affinity_terms = []
    p.tolerations = [Obj(key="k", operator="Exists", value="", effect="")]
    assert not msh.node_admits(p, n)


# ---- the Scheduler's class ids, on a ctx that records the calls ----

class RecordingCtx:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*a, **kw):
            self.calls.append((name, a, kw))
            if name.startswith("schedule_sequential"):
                p = len(a[0])
                return np.full(p, -1, np.int32), np.zeros(p, np.int64), np.ones(p, np.int32)
        return record

    def names(self):
        return [c[0] for c in self.calls]


def cluster():
    return [node("node0", {"pool": "gpu"}), node("node1", {"pool": "cpu"}),
            node("node2", {"pool": "cpu"}, [taint("node-role.kubernetes.io/control-plane")])]


def named(name, **kw):
    p = pod(**kw)
    p["metadata"]["name"] = name
    return p


def test_class_ids_persist_and_all_ones_is_minus_one(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx)
    s.update_nodes(cluster())
    gpu = named("a1", selector={"pool": "gpu"})
    cpu = named("b2", selector={"pool": "cpu"})          # node1 only: it does not tolerate node2's taint
    anyw = named("c3", tolerations=[tol("", "Exists")])  # admitted everywhere: -1
    plain = named("d4")                                  # no constraint, but node2 is tainted: a class
    ids = s.pod_class_ids([gpu, cpu, anyw, plain, gpu])
    assert ids.tolist() == [0, 1, -1, 2, 0]
    assert s.node_class_bits().tolist() == [0b101, 0b110, 0b000]
    # the ids persist across calls for the snapshot, whatever the order of the pods
    assert s.pod_class_ids([plain, named("e5", selector={"pool": "cpu"}), gpu]).tolist() == [2, 1, 0]
    s.schedule_sequential([gpu, anyw])
    up = [c for c in ctx.calls if c[0] == "upload_node_class_bits"]
    assert len(up) == 1 and up[0][1][0] == 3 and np.asarray(up[0][1][1]).tolist() == [0b101, 0b110, 0b000]
    call = ctx.calls[-1]
    assert call[0] == "schedule_sequential_classes" and call[1][2] is None and call[1][3].tolist() == [0, -1]
    # the same classes again: no second upload; a new class: one more
    s.schedule_sequential([cpu])
    assert ctx.names().count("upload_node_class_bits") == 1
    s.schedule_sequential([named("f6", node_name="node1")])
    assert ctx.names().count("upload_node_class_bits") == 2 and ctx.calls[-1][1][3].tolist() == [3]
    # a new snapshot starts over
    s.update_nodes(cluster()[:2])
    assert s.pod_class_ids([cpu, gpu]).tolist() == [0, 1]


def test_pods_admitted_everywhere_keep_the_call_they_had(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx)
    s.update_nodes(cluster())
    s.schedule_sequential([named("a1", tolerations=[tol("", "Exists")]), named("b2", tolerations=[tol("", "Exists")])])
    assert ctx.names()[-1] == "schedule_sequential" and "upload_node_class_bits" not in ctx.names()
    s.update_nodes(cluster()[:2])  # no taints: a plain pod has no class
    s.schedule_sequential([named("c3"), named("d4", selector={})])
    assert ctx.names()[-1] == "schedule_sequential" and "upload_node_class_bits" not in ctx.names()


def test_the_65th_class_raises(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx)
    s.update_nodes(cluster())
    pods = [named(f"p{k}", selector={"pool": "gpu", "k": str(k)}) for k in range(65)]  # 65 keys, none admitted anywhere
    assert s.pod_class_ids(pods[:64]).tolist() == list(range(64))
    with pytest.raises(ValueError, match="64"):
        s.pod_class_ids(pods)
    assert s.pod_class_ids(pods[:64]).tolist() == list(range(64))  # the refusal changed nothing
    assert "schedule_sequential_classes" not in ctx.names()
