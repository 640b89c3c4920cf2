"""Required inter-pod affinity and anti-affinity in sequential-commit mode, on the CPU: the reference
(tests/podaffinity_ref.py) against hand-written cases for each rule, the constraints.py parsers, the Scheduler's
bookkeeping on a ctx backed by the reference, the new symbols, and the coverage of the cases the GPU tests use
(tests/test_podaffinity_gpu.py): chosen here so that the reference alone shows every rule deciding."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import classes_ref as KR
import podaffinity_ref as PA
import prefs_ref as PR
import spread_ref as S

HOST, ZONE = PA.HOSTNAME, PA.ZONE
NONE, LEAST, MOST = PA.NONE, PA.LEAST, PA.MOST
NEW_SYMBOLS = ["msh_set_pod_affinity_terms", "msh_get_pod_affinity_terms", "msh_set_pod_profiles", "msh_get_pod_profiles",
               "msh_upload_pod_affinity_state", "msh_patch_pod_affinity_state", "msh_pod_affinity_state",
               "msh_seq_podaffinity_max_nodes", "msh_schedule_sequential_podaffinity",
               "msh_schedule_sequential_podaffinity_device"]


def test_new_symbols_are_declared_exported_and_bound(msh):
    header = (Path(__file__).resolve().parents[1] / "include" / "minisched_hip.h").read_text()
    lib = msh._native.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in msh._native.EXPORTED and hasattr(lib, name)
    for macro, value in (("MSH_MAX_AFFINITY_TERMS", 32), ("MSH_MAX_POD_PROFILES", 64), ("MSH_TOPOLOGY_HOSTNAME", 0),
                         ("MSH_TOPOLOGY_ZONE", 1)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    assert "#define MSH_ABI_VERSION 8" in header
    inv = msh._native.MSH_ERR_INVALID
    assert lib.msh_set_pod_affinity_terms(None, 0, None) == inv
    assert lib.msh_seq_podaffinity_max_nodes(None, 0, None) == inv
    for nm in ("set_pod_affinity_terms", "set_pod_profiles", "upload_pod_affinity_state", "patch_pod_affinity_state",
               "pod_affinity_state", "schedule_sequential_podaffinity", "schedule_sequential_podaffinity_device",
               "seq_podaffinity_max_nodes"):
        assert hasattr(msh.DeviceContext, nm), nm


# ---- the reference against hand-written cases ----

def run(oracle, n, zone, topo, prof, profile, cap=None, state=None):
    """Plain pods (no digits, requests, groups or classes) of the given profiles against n schedulable nodes."""
    p = len(profile)
    st = state or PA.State(n, topo, *prof)
    a, us, rq = S.no_res(n, p)
    eff = S.no_limit(n) if cap is None else np.asarray(cap, np.int64)
    out = PA.per_pod(oracle, np.zeros(n, np.uint8), np.full(n, -1, np.int8), np.zeros(p, np.int8), np.ones(p, np.uint8),
                     oracle.PluginSet(), eff, a, us, rq, zone, None, (), NONE, 1, [], None, 0, None, None, None, 0, 0,
                     None, 0, 0, st, np.asarray(profile, np.int32))
    return out[0].tolist(), out[2].tolist(), st


def test_one_replica_per_node(oracle):
    idx, status, st = run(oracle, 3, None, [HOST], ([1], [1], [-1]), [0] * 5)
    assert idx == [0, 1, 2, -1, -1] and status[3:] == [PA.FIT_ERROR] * 2
    assert st.present.tolist() == [1, 1, 1] and st.repel.tolist() == [1, 1, 1]
    assert st.stats["own_anti"] == 0 + 1 + 2 + 3 + 3 and st.stats["symmetric_anti"] == 0


def test_one_replica_per_zone(oracle):
    zone = [0, 0, 1, 1, -1]
    idx, status, st = run(oracle, 5, zone, [ZONE], ([1], [1], [-1]), [0] * 5)
    # zones 0 and 1 take one each; the node without the key is its own empty domain every time
    assert idx == [0, 2, 4, 4, 4]
    assert st.present.tolist() == [1, 0, 1, 0, 1]


def test_symmetric_repulsion_of_a_pod_without_anti_affinity(oracle):
    # profile 0 repels term 0 and does not match it; profile 1 matches it and has no anti-affinity of its own
    prof = ([0, 1], [1, 0], [-1, -1])
    idx, _, st = run(oracle, 3, None, [HOST], prof, [0, 1, 1, 0])
    assert idx == [0, 1, 1, 0]   # the victims avoid node 0; the repeller then avoids the victims' node 1
    assert st.stats["symmetric_anti"] == 2 and st.stats["own_anti"] == 1


def test_a_self_affine_series_opens_exactly_one_zone(oracle):
    zone = [1, 1, 0, 0, -1, 2]
    cap = [1, 1, 5, 5, 5, 5]
    idx, status, st = run(oracle, 6, zone, [ZONE], ([1], [0], [0]), [0] * 4, cap=cap)
    # the first pod opens zone 1 by the exception; the second fills it; the rest find no node although others are empty
    assert idx == [0, 1, -1, -1] and status == [0, 0, PA.FIT_ERROR, PA.FIT_ERROR]
    assert st.stats["first_pod"] == 1 and st.stats["affinity"] > 0 and st.stats["no_topology_key"] > 0


def test_a_follower_has_no_first_pod_exception(oracle):
    # profile 0 needs a pod matching term 0 and does not match it itself; profile 1 matches it
    prof = ([0, 1], [0, 0], [0, -1])
    idx, status, _ = run(oracle, 3, None, [HOST], prof, [0, 1, 0], cap=[1, 5, 5])
    assert status == [PA.FIT_ERROR, 0, PA.FIT_ERROR] and idx[1] == 0   # node 0 holds the leader and is full


def test_a_zone_term_fails_on_a_node_without_a_zone(oracle):
    zone = [-1, -1, 0]
    idx, _, st = run(oracle, 3, zone, [ZONE], ([1], [0], [0]), [0, 0])
    assert idx == [2, 2] and st.stats["no_topology_key"] == 4 and st.stats["first_pod"] == 1
    # ... while an anti-affinity term on a zone does not: the node is in no domain
    idx, _, _ = run(oracle, 3, zone, [ZONE], ([1], [1], [-1]), [0, 0, 0, 0])
    assert idx == [0, 0, 0, 0]


def test_a_pod_without_a_profile_is_untouched(oracle):
    st = PA.State(3, [HOST], [1], [1], [-1], present=[1, 1, 1], repel=[1, 1, 1])
    idx, _, st = run(oracle, 3, None, [HOST], None, [-1, -1, 7], state=st)
    assert idx == [0, 0, 0] and st.present.tolist() == [1, 1, 1] and sum(st.stats.values()) == 0


def test_hostname_and_zone_terms_together(oracle):
    # term 0: hostname anti-affinity among replicas; term 1: zone affinity to a leader
    zone = [0, 0, 1, 1]
    prof = ([0b10, 0b01], [0, 0b01], [-1, 1])  # profile 0: the leader (matches term 1); profile 1: a replica
    idx, _, _ = run(oracle, 4, zone, [HOST, ZONE], prof, [0, 1, 1, 1], cap=[0, 5, 5, 5])
    assert idx == [1, 1, -1, -1] or idx == [1, 1, 0, -1]
    idx, _, _ = run(oracle, 4, zone, [HOST, ZONE], prof, [0, 1, 1, 1])
    assert idx == [0, 0, 1, -1]   # the leader on node 0: zone 0 has two nodes, one replica each


def test_derived_words_follow_a_new_zone_column(oracle):
    st = PA.State(4, [ZONE], [1], [1], [-1], present=[1, 0, 0, 0], repel=[1, 0, 0, 0])
    assert run(oracle, 4, [0, 0, 1, 1], [ZONE], None, [0], state=st.copy())[0] == [2]
    assert run(oracle, 4, [0, 1, 0, 1], [ZONE], None, [0], state=st.copy())[0] == [1]


# ---- constraints.py ----

def sel(labels=None, exprs=None):
    s = {}
    if labels is not None:
        s["matchLabels"] = labels
    if exprs is not None:
        s["matchExpressions"] = exprs
    return s


def aterm(selector, key="kubernetes.io/hostname", namespaces=None, ns_selector=None):
    t = {"labelSelector": selector, "topologyKey": key}
    if namespaces is not None:
        t["namespaces"] = namespaces
    if ns_selector is not None:
        t["namespaceSelector"] = ns_selector
    return t


def apod(name, labels=None, ns=None, aff=None, anti=None):
    p = {"metadata": {"name": name, "labels": labels or {}}, "spec": {}}
    if ns:
        p["metadata"]["namespace"] = ns
    if aff is not None or anti is not None:
        p["spec"]["affinity"] = {}
    if aff is not None:
        p["spec"]["affinity"]["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": aff}
    if anti is not None:
        p["spec"]["affinity"]["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": anti}
    return p


def test_label_selector(msh):
    K = msh.constraints
    m = K.label_selector_matches
    assert not m(None, {"a": "1"}) and m({}, {}) and m({}, {"a": "1"})
    assert m(sel({"a": "1"}), {"a": "1", "b": "2"}) and not m(sel({"a": "1"}), {"a": "2"}) and not m(sel({"a": "1"}), {})
    e = lambda op, *v: [{"key": "a", "operator": op, "values": list(v)}]
    assert m(sel(exprs=e("In", "1", "2")), {"a": "2"}) and not m(sel(exprs=e("In", "1")), {"a": "2"})
    assert not m(sel(exprs=e("In", "1")), {})
    assert m(sel(exprs=e("NotIn", "1")), {"a": "2"}) and m(sel(exprs=e("NotIn", "1")), {}) and not m(sel(exprs=e("NotIn", "1")), {"a": "1"})
    assert m(sel(exprs=e("Exists")), {"a": ""}) and not m(sel(exprs=e("Exists")), {"b": "1"})
    assert m(sel(exprs=e("DoesNotExist")), {"b": "1"}) and not m(sel(exprs=e("DoesNotExist")), {"a": "1"})
    assert not m(sel(exprs=e("Gt", "1")), {"a": "2"})                       # a node-selector operator: invalid here
    assert not m(sel({"a": "1"}, e("NotIn", "1")), {"a": "1"})              # ANDed


def test_terms_namespaces_and_parsers(msh):
    K = msh.constraints
    t = aterm(sel({"app": "db"}))
    assert K.term_matches_pod(t, "prod", apod("x", {"app": "db"}, "prod"))
    assert not K.term_matches_pod(t, "prod", apod("x", {"app": "db"}, "dev"))       # the owner's namespace only
    assert not K.term_matches_pod(t, "prod", apod("x", {"app": "web"}, "prod"))
    assert K.term_matches_pod(t, "default", apod("x", {"app": "db"}))               # no namespace: "default"
    t2 = aterm(sel({"app": "db"}), namespaces=["dev", "qa"])
    assert K.term_matches_pod(t2, "prod", apod("x", {"app": "db"}, "qa")) and not K.term_matches_pod(t2, "prod", apod("x", {"app": "db"}, "prod"))
    assert not K.term_matches_pod(aterm(None), "prod", apod("x", {"app": "db"}, "prod"))   # a nil selector
    p = apod("p", {"app": "db"}, aff=[t], anti=[t2])
    assert K.pod_required_pod_affinity(p) == [t] and K.pod_required_pod_anti_affinity(p) == [t2]
    assert K.pod_required_pod_affinity(apod("q")) == [] and K.pod_required_pod_anti_affinity(apod("q")) == []
    assert K.term_key(t, "a") != K.term_key(t, "b") and K.term_key(t2, "a") == K.term_key(t2, "b")
    assert K.check_pod_affinity(p, None) == ([t], [t2])
    with pytest.raises(ValueError, match="prod/two"):
        K.check_pod_affinity(apod("two", ns="prod", aff=[t, t2]), None)
    with pytest.raises(ValueError, match="default/nss"):
        K.check_pod_affinity(apod("nss", anti=[aterm(sel(), ns_selector=sel({"team": "a"}))]), None)
    K.check_pod_affinity(apod("nss", anti=[aterm(sel(), ns_selector={})]), None)     # an empty one is fine
    with pytest.raises(ValueError, match="default/rack"):
        K.check_pod_affinity(apod("rack", anti=[aterm(sel(), key="rack")]), "zone")
    K.check_pod_affinity(apod("z", anti=[aterm(sel(), key="zone")]), "zone")
    with pytest.raises(ValueError, match="default/z"):
        K.check_pod_affinity(apod("z", anti=[aterm(sel(), key="zone")]), None)


# ---- the Scheduler on a ctx backed by the reference ----

class RefCtx:
    """What Scheduler.schedule_sequential needs of a DeviceContext for plain pods with inter-pod terms, computed by the
    reference; every call is recorded."""

    def __init__(self, oracle):
        self.O, self.calls = oracle, []
        self.zone, self.state, self.counts = None, None, None

    def __getattr__(self, name):
        def record(*a, **kw):
            self.calls.append(name)
        return record

    def upload_nodes(self, u, nd):
        self.calls.append("upload_nodes")
        self.u, self.nd, self.zone = np.asarray(u), np.asarray(nd), None
        self.counts = np.zeros(len(self.u), np.int32)
        if self.state is not None:
            self.state.present[:] = 0
            self.state.repel[:] = 0

    def upload_node_zones(self, zone):
        self.zone = np.asarray(zone)

    def set_pod_affinity_terms(self, topo):
        self.calls.append("set_pod_affinity_terms")
        self.state = PA.State(len(self.u), topo) if len(topo) else None

    def set_pod_profiles(self, m, a, f):
        self.calls.append("set_pod_profiles")
        self.state.set_profiles(m, a, f)

    def upload_pod_affinity_state(self, present, repel):
        self.calls.append("upload_pod_affinity_state")
        self.state.present[:], self.state.repel[:] = present, repel

    def _run(self, pd, pt, prf, state):
        n, p = len(self.u), len(pd)
        a, us, rq = S.no_res(n, p)
        out = PA.per_pod(self.O, self.u, self.nd, pd, pt, self.O.PluginSet(), S.no_limit(n), a, us, rq, self.zone, None,
                         (), NONE, 1, [], None, 0, None, None, None, 0, 0, None, 0, 0, state, prf, self.counts)
        self.counts = out[3]
        return out[0], out[1], out[2]

    def schedule_sequential(self, pd, pt, max_pods=0):
        self.calls.append("schedule_sequential")
        return self._run(pd, pt, None, PA.State(len(self.u), []))

    def schedule_sequential_spread_scored(self, pd, pt, grp, req, max_pods=0):  # the plain call with `zones` set
        self.calls.append("schedule_sequential_spread_scored")
        assert (np.asarray(grp) == -1).all() and req is None
        return self._run(pd, pt, None, PA.State(len(self.u), []))

    def schedule_sequential_podaffinity(self, pd, pt, grp, cls, prf, req, max_pods=0):
        self.calls.append("schedule_sequential_podaffinity")
        assert (grp is None or (np.asarray(grp) == -1).all()) and cls is None and req is None
        return self._run(pd, pt, prf, self.state)


def nodes3():
    return [{"metadata": {"name": f"node{i}", "labels": {"kubernetes.io/hostname": f"node{i}", "zone": "ab"[i // 2]}},
             "spec": {}} for i in range(3)]


def test_scheduler_rebuilds_the_state_when_a_term_arrives_late(msh, oracle):
    ctx = RefCtx(oracle)
    s = msh.Scheduler(ctx=ctx, zones="zone", spread_groups={})
    web = lambda k: apod(f"web{k}-9", {"app": "web"})  # NodeNumber reads the last digit: no node ends in 9
    # no term yet: the plain call; both pods land on node 0 (first maximum) and go into the record
    r = s.schedule_sequential([web(0), web(1)], nodes3())
    assert [x.node_index for x in r] == [0, 0] and "schedule_sequential_podaffinity" not in ctx.calls
    # a pod that repels app=web per node arrives: the terms are set and the state rebuilt from the record
    lone = apod("lone-9", {"app": "lone"}, anti=[aterm(sel({"app": "web"}))])
    r = s.schedule_sequential([lone, web(2)])
    assert [x.node_index for x in r] == [1, 0]          # away from the web pods; the next web pod away from it
    assert ctx.calls[-4:] == ["set_pod_affinity_terms", "set_pod_profiles", "upload_pod_affinity_state",
                              "schedule_sequential_podaffinity"]
    assert ctx.state.present.tolist() == [1, 0, 0] and ctx.state.repel.tolist() == [0, 1, 0]
    assert [x.tolist() for x in s.pod_affinity_state()] == [[1, 0, 0], [0, 1, 0]]
    # the same term and profiles again: nothing is set again; every pod of the call has a profile or -1
    n_sets = ctx.calls.count("set_pod_affinity_terms")
    r = s.schedule_sequential([web(3), apod("other-9", {"app": "other"})])
    assert [x.node_index for x in r] == [0, 0] and ctx.calls.count("set_pod_affinity_terms") == n_sets
    # a second term, on the zone: web pods now also repel each other per zone; bit 1 is rebuilt from all four web pods
    spread = apod("web4-9", {"app": "web"}, anti=[aterm(sel({"app": "web"}), key="zone")])
    r = s.schedule_sequential([spread])
    assert r[0].node_index == 2 and ctx.calls.count("set_pod_affinity_terms") == n_sets + 1   # zone a holds web pods
    assert [t[2] for t in s.pod_affinity_terms()] == [HOST, ZONE]
    assert ctx.state.present.tolist() == [0b11, 0, 0b11] and ctx.state.repel.tolist() == [0, 0b01, 0b10]
    # a new profile of the same terms: the profiles alone are set again, which keeps the device's state (and with it
    # whatever the caller patched in for pods bound elsewhere)
    ctx.patch_pod_affinity_state([1], [0b10], [0b01])   # the ctx records the call; the model below keeps its state
    both = apod("both-9", {"app": "web"}, anti=[aterm(sel({"app": "web"}))])
    before = (ctx.state.present.copy(), ctx.state.repel.copy())
    r = s.schedule_sequential([both])
    assert r[0].outcome == msh.Outcome.FIT_ERROR            # nodes 0 and 2 hold web pods, node 1 repels them
    assert ctx.calls.count("set_pod_affinity_terms") == n_sets + 1 and "upload_pod_affinity_state" not in ctx.calls[-3:]
    assert ctx.calls[-2:] == ["set_pod_profiles", "schedule_sequential_podaffinity"]
    assert np.array_equal(ctx.state.present, before[0]) and np.array_equal(ctx.state.repel, before[1])
    # a new snapshot forgets it all
    s.update_nodes(nodes3())
    assert s.pod_affinity_terms() == [] and s.pod_profile_ids([web(5)]) is None


def test_the_33rd_term_and_the_65th_profile_raise(msh, oracle):
    ctx = RefCtx(oracle)
    s = msh.Scheduler(ctx=ctx)
    s.update_nodes(nodes3())
    pods = [apod(f"p{k}", {"k": str(k)}, anti=[aterm(sel({"k": str(k)}))]) for k in range(33)]
    assert s.pod_profile_ids(pods[:31]).tolist() == list(range(31))
    with pytest.raises(ValueError, match="32"):
        s.pod_profile_ids(pods[31:])                    # the 32nd term is fine, the 33rd is not: nothing is kept
    assert len(s.pod_affinity_terms()) == 31 and s.pod_profile_ids(pods[:31]).tolist() == list(range(31))
    assert s.pod_profile_ids(pods[31:32]).tolist() == [0] and len(s.pod_affinity_terms()) == 32   # a new term: new ids
    with pytest.raises(ValueError, match="32"):
        s.pod_profile_ids(pods[32:])
    s.update_nodes(nodes3())
    # seven terms on labels t0..t6; a pod's labels choose which it matches: 65 distinct match words
    terms = [aterm(sel({f"t{k}": "1"})) for k in range(7)]
    owner = apod("owner", anti=terms)
    lab = lambda w: {f"t{k}": "1" for k in range(7) if (w >> k) & 1}
    ids = s.pod_profile_ids([owner] + [apod(f"m{w}", lab(w)) for w in range(1, 64)])
    assert sorted(ids.tolist()) == list(range(64))
    with pytest.raises(ValueError, match="64"):
        s.pod_profile_ids([apod("m64", lab(64))])


# ---- the cases of the GPU tests ----

# (nodes, resources, terms): 1, 4 and 16 waves at 4 nodes per thread (two resources) and at 2 (three resources)
GPU_CASES = [(37, 2, 1), (300, 2, 1), (300, 2, 32), (100, 3, 1), (1100, 2, 32),
             (1100, 2, 1), (37, 2, 32), (100, 3, 32), (600, 3, 32), (600, 3, 1)]
# one seed per case, chosen by test_the_gpu_cases_reach_every_rule's condition (podaffinity_ref.gen_case: with one
# term an even seed is a hostname term, an odd one a zone term)
GPU_SEEDS = [2, 9, 0, 15, 0, 10, 1, 1, 4, 15]
GPU_PODS = 150


def gpu_case(case: int, seed: int | None = None) -> dict:
    """podaffinity_ref.gen_case for GPU_CASES[case] plus everything else a call can carry: four spread groups (hard
    and soft), five classes with masks and preference values, the resource score mode and w_balanced by turns."""
    n, nres, T = GPU_CASES[case]
    seed = GPU_SEEDS[case] if seed is None else seed
    c = PA.gen_case(seed, n, GPU_PODS, nres, T)
    rng = np.random.default_rng(31 * 10**6 + seed)
    C = 5
    bits, _ = KR.gen_bits(rng, n, C)
    A, Tt = PR.gen_prefs(rng, n, C)
    mode = (LEAST, MOST, NONE)[case % 3]
    c.update(nn_weight=2, normalize=case % 4, skew=np.array([1, 2, 1, 3], np.int32), modes=np.array([0, 1, 0, 1], np.uint8),
             group=np.where(rng.random(GPU_PODS) < 0.3, rng.integers(0, 4, GPU_PODS), -1).astype(np.int32),
             bits=bits, C=C, A=A, T=Tt,
             pod_class=np.where(rng.random(GPU_PODS) < 0.3, rng.integers(0, C, GPU_PODS), -1).astype(np.int32),
             mode=mode, rs_weight=3, w=(int(rng.integers(0, 20)), int(rng.integers(0, 20))), ws=int(rng.integers(1, 20)),
             wb=(case // 2) % 2)
    c["cap"] = np.maximum(c["cap"], 1 + (n < 100) * 2)
    return c


def ref_case(oracle, c):
    st = PA.State(c["n"], c["topo"], c["match"], c["anti"], c["aff"])
    ps = oracle.PluginSet(weights=[c["nn_weight"]], normalize=[c["normalize"]])
    out = PA.per_pod(oracle, c["unsched"], c["node_digit"], c["pod_digit"], c["pod_tol"], ps, c["cap"], c["alloc"],
                     c["used"], c["req"], c["zone"], c["group"], c["skew"], c["mode"], c["rs_weight"], [1] * c["nres"],
                     c["bits"], c["C"], c["pod_class"], c["A"], c["T"], *c["w"], c["modes"], c["ws"], c["wb"], st,
                     c["profile"])
    return out, st


def coverage(oracle, c):
    out, st = ref_case(oracle, c)
    prof = c["profile"] >= 0
    placed = float((out[2][prof] == PA.PLACED).mean())
    need = [k for k in PA.COUNTERS if k != "no_topology_key" or ZONE in c["topo"]]
    return placed, {k: st.stats[k] for k in need}


def test_the_gpu_cases_reach_every_rule(oracle):
    """On every case of the GPU tests every counter of the reference is > 0 (own anti, symmetric anti, affinity, the
    first-pod exception, and the missing topology key wherever the case has a zone term: a hostname term has no node
    without its key) and between 20 % and 80 % of the profiled pods are placed. Both topologies occur with T = 1."""
    one = set()
    for case, (n, nres, T) in enumerate(GPU_CASES):
        c = gpu_case(case)
        if T == 1:
            one.add(c["topo"][0])
        placed, counters = coverage(oracle, c)
        assert 0.2 <= placed <= 0.8, (case, placed)
        assert all(v > 0 for v in counters.values()), (case, counters)
        assert sorted(set(c["topo"])) == ([HOST, ZONE] if T > 1 else c["topo"])
    assert one == {HOST, ZONE}
