"""Resource requests in sequential-commit mode (msh_schedule_sequential_fit and friends): everything that needs
no GPU. The CPU references agree with each other, the quantity parser and the request helpers follow upstream,
the entry points are declared, bound and exported, and Scheduler(resources=None) is the scheduler it was."""
from __future__ import annotations

import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import node_capacity_ref as CR
import resource_fit_ref as R

ROOT = Path(__file__).resolve().parents[1]
NEW = ("msh_upload_node_resources", "msh_patch_node_resources", "msh_clear_node_resources", "msh_node_resources",
       "msh_schedule_sequential_fit", "msh_schedule_sequential_fit_device")


def snapshot(msh):
    return importlib.import_module(msh.__name__ + ".snapshot")


def random_plugins(O, rng):
    filters = ["NodeUnschedulable"] if rng.random() < 0.8 else []
    prescore = ["NodeNumber"] if rng.random() < 0.85 else []
    if rng.random() < 0.1:
        return O.PluginSet(filters, prescore, [], [], [])
    return O.PluginSet(filters, prescore, ["NodeNumber"], [int(rng.choice([1, 3, 2**32]))], [int(rng.integers(0, 4))])


def small_case(rng, case):
    n, p = int(rng.integers(0, 13)), int(rng.integers(0, 41))
    u = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, 10 if case % 3 else 3, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return n, p, u, nd, pd, pt


def same(a, b, what):
    for x, y, name in zip(a, b, ("idx", "score", "status", "counts", "used")):
        assert np.array_equal(x, y), (what, name)


def test_serial_against_the_oracle_identity(oracle):
    """One resource with unit requests is a second pod capacity, and with zero requests no conjunct at all
    (resource_fit_ref.via_oracle): the serial loop against the unchanged C oracle on 300 small random cases, with
    carried-in counts and used, alloc below used, an optional count limit, every plugin variation."""
    rng = np.random.default_rng(20261)
    for case in range(300):
        n, p, u, nd, pd, pt = small_case(rng, case)
        pl = random_plugins(oracle, rng)
        k = rng.integers(0, 4, n)
        kind = case % 3
        eff = (R.no_limit(n) if kind == 0 else CR.effective(rng.choice([0, 1, 2, 3, 7, 10**6], n), int(rng.choice([0, 2, 5]))))
        alloc = rng.integers(0, 7, (1, n))
        used = rng.integers(0, 4, (1, n))  # above alloc for some nodes
        req = np.full((1, p), 0 if case % 5 == 0 else 1, np.int64)
        a = R.via_oracle(oracle, u, nd, pd, pt, pl, eff, alloc, used, req, k)
        b = R.serial(oracle, u, nd, pd, pt, pl, eff, alloc, used, req, k)
        same(a, b, (case, pl))


def test_per_pod_reference_against_serial(oracle):
    """The numpy per-pod loop used at mid sizes on the GPU against the serial loop: 1..4 resources, mixed
    requests with zeros, 64-bit amounts."""
    rng = np.random.default_rng(20262)
    for case in range(300):
        n, p, u, nd, pd, pt = small_case(rng, case)
        pl = random_plugins(oracle, rng)
        nres = 1 + case % 4
        unit = int(rng.choice([1, 2**31, 2**40]))
        alloc = rng.integers(0, 9, (nres, n)) * unit
        used = rng.integers(0, 3, (nres, n)) * unit
        req = rng.integers(0, 4, (nres, p)) * unit - (rng.random((nres, p)) < 0.2)
        req = np.maximum(req, 0)
        k = rng.integers(0, 3, n)
        eff = R.no_limit(n) if case % 2 else CR.effective(rng.integers(0, 6, n), 0)
        a = R.per_pod(oracle, u, nd, pd, pt, pl, eff, alloc, used, req, k)
        b = R.serial(oracle, u, nd, pd, pt, pl, eff, alloc, used, req, k)
        same(a, b, (case, pl))


def test_serial_rules(oracle):
    """The resource rule's corners in the reference itself: an exact fit passes, one unit over fails, a zero
    request is never rejected (alloc below used included), a score error commits nothing."""
    pl = oracle.PluginSet()
    u, nd = np.zeros(2, np.uint8), np.array([1, 1], np.int8)
    pd, pt = np.array([1, 1, 1, -1], np.int8), np.zeros(4, np.uint8)
    alloc = np.array([[5, 2**40]])
    used = np.array([[7, 0]])  # node 0: alloc below used
    req = np.array([[0, 2**40, 1, 0]])
    idx, score, status, cnt, us = R.serial(oracle, u, nd, pd, pt, pl, R.no_limit(2), alloc, used, req)
    assert idx.tolist() == [0, 1, -1, -1] and status.tolist() == [R.PLACED, R.PLACED, R.FIT_ERROR, R.SCORE_ERROR]
    assert cnt.tolist() == [1, 1] and us.tolist() == [[7, 2**40]]


@pytest.mark.parametrize("text, milli, want", [
    ("500m", True, 500), ("0.5", True, 500), ("2", False, 2), ("2", True, 2000), ("1Gi", False, 2**30),
    ("1G", False, 10**9), ("1.5Gi", False, 3 * 2**29), ("100k", False, 100_000), ("1m", False, 1),
    ("1500m", False, 2), ("0.0001", True, 1), ("1.0001", True, 1001), (".5", True, 500), ("3.", False, 3),
    ("64Mi", False, 2**26), ("2Ki", False, 2048), ("1M", False, 10**6), ("1T", False, 10**12), ("1P", False, 10**15),
    ("1Ti", False, 2**40), ("1Pi", False, 2**50), ("0", False, 0), ("+4", True, 4000), (7, False, 7), (7, True, 7000),
    (" 250m ", True, 250),
])
def test_parse_quantity(msh, text, milli, want):
    assert snapshot(msh).parse_quantity(text, milli=milli) == want


@pytest.mark.parametrize("bad", ["", "abc", "1.2.3", "1 Gi", "m", ".", "Gi", "1mi", "1K", "0x10", "1,5", None, 1.5, True])
def test_parse_quantity_rejects_garbage(msh, bad):
    with pytest.raises(ValueError):
        snapshot(msh).parse_quantity(bad)


def test_pod_requests_and_node_allocatable(msh):
    S = snapshot(msh)
    pod = {"metadata": {"name": "p1"},
           "spec": {"containers": [{"resources": {"requests": {"cpu": "250m", "memory": "64Mi"}}},
                                   {"resources": {"requests": {"cpu": "0.5"}, "limits": {"cpu": "8"}}},
                                   {"name": "no-resources"}],
                    "initContainers": [{"resources": {"requests": {"cpu": "1", "memory": "1Mi"}}},
                                       {"resources": {"requests": {"memory": "100Mi"}}}]}}
    # cpu: max(250 + 500, 1000, 0); memory: max(64Mi, 1Mi, 100Mi); a resource nobody names: 0
    assert S.pod_requests(pod, ("cpu", "memory", "nvidia.com/gpu")) == [1000, 100 * 2**20, 0]
    assert S.pod_requests({"metadata": {"name": "bare"}}, ("cpu",)) == [0]
    node = {"metadata": {"name": "n1"}, "status": {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": "110"}}}
    assert S.node_allocatable(node, ("cpu", "memory", "ephemeral-storage")) == [4000, 8 * 2**30, 0]
    assert S.node_allocatable({"metadata": {"name": "n2"}}, ("cpu", "memory")) == [0, 0]
    with pytest.raises(ValueError):
        S.node_allocatable({"metadata": {"name": "n3"}, "status": {"allocatable": {"cpu": "-1"}}}, ("cpu",))
    with pytest.raises(ValueError):
        S.node_allocatable({"metadata": {"name": "n3"}, "status": {"allocatable": {"memory": "8Ei"}}}, ("memory",))


def test_new_entry_points_are_declared_bound_and_exported(msh):
    hdr = (ROOT / "include" / "minisched_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = msh._native.lib()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert name in msh._native.EXPORTED and name in msh._native._SIGS, name
        assert hasattr(lib, name), name
    assert "#define MSH_MAX_RESOURCES 4" in hdr and msh._native.MAX_RESOURCES == 4
    assert "#define MSH_ABI_VERSION 8" in hdr and lib.msh_abi_version() == 8  # additive
    go = (ROOT / "go" / "minisched" / "gpusched" / "gpusched.go").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, name


def test_null_ctx_is_invalid_without_a_device(msh):
    N = msh._native
    lib, inv = N.lib(), N.MSH_ERR_INVALID
    a = np.ones(3, np.int64)
    idx = np.arange(3, dtype=np.int32)
    present = N.C.c_int32(0)
    assert lib.msh_upload_node_resources(None, 3, 1, N.ptr(a), None) == inv
    assert lib.msh_patch_node_resources(None, 3, N.ptr(idx), N.ptr(a), None) == inv
    assert lib.msh_clear_node_resources(None) == inv
    assert lib.msh_node_resources(None, None, None, None, N.C.byref(present)) == inv
    assert lib.msh_schedule_sequential_fit(None, 0, None, None, 1, None, 0, None, None, None, N.COMMIT_CB(), None) == inv
    assert lib.msh_schedule_sequential_fit_device(None, 0, None, None, 1, None, 0, None, None, None, None) == inv


def test_python_side_validation(msh):
    dc = msh.DeviceContext
    with pytest.raises(ValueError):
        dc._amounts(np.array([[1.5, 2.0]]))
    with pytest.raises(ValueError):
        dc._amounts(np.array([1, 2]))  # not (nres, n)
    with pytest.raises(ValueError):
        dc._amounts(np.array([[2**63]], np.uint64))
    assert dc._amounts([[0, 2**62]]).dtype == np.int64
    assert dc._amounts(np.array([[-1]]))[0, 0] == -1  # negatives reach the library: MSH_ERR_INVALID
    with pytest.raises(ValueError):
        msh.Scheduler(ctx=RecordingCtx(), resources=())
    with pytest.raises(ValueError):
        msh.Scheduler(ctx=RecordingCtx(), resources=("a", "b", "c", "d", "e"))


class RecordingCtx:
    """Stands in for a DeviceContext: records the calls and places every pod on node 0."""

    def __init__(self):
        self.calls = []

    def set_plugins(self, *a):
        self.calls.append("set_plugins")

    def upload_nodes(self, unsched, digit):
        self.calls.append("upload_nodes")

    def upload_node_capacity(self, cap):
        self.calls.append("upload_node_capacity")

    def upload_node_resources(self, alloc, used=None):
        self.calls.append(("upload_node_resources", np.array(alloc)))

    def schedule_sequential(self, pd, pt, max_pods_per_node=0):
        self.calls.append(("schedule_sequential", max_pods_per_node))
        p = len(pd)
        return np.zeros(p, np.int32), np.full(p, 10, np.int64), np.zeros(p, np.int32)

    def schedule_sequential_fit(self, pd, pt, req, max_pods_per_node=0):
        self.calls.append(("schedule_sequential_fit", np.array(req), max_pods_per_node))
        p = len(pd)
        return np.zeros(p, np.int32), np.full(p, 10, np.int64), np.zeros(p, np.int32)

    def close(self):
        pass


NODES = [{"metadata": {"name": "node2"}, "status": {"allocatable": {"cpu": "2", "memory": "1Gi"}}},
         {"metadata": {"name": "node1"}, "status": {"allocatable": {"cpu": "500m"}}}]
PODS = [{"metadata": {"name": "pod1"}, "spec": {"containers": [{"resources": {"requests": {"cpu": "100m", "memory": "1Mi"}}}]}},
        {"metadata": {"name": "pod2"}, "spec": {"containers": [{}]}}]


def test_scheduler_without_resources_is_unchanged(msh):
    """resources=None (the default): no resource call of any kind, the plain sequential entry point, even for
    nodes and pods that carry amounts."""
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx)
    assert s.resources is None
    res = s.schedule_sequential(PODS, NODES, max_pods_per_node=3)
    assert ctx.calls == ["set_plugins", "upload_nodes", ("schedule_sequential", 3)]
    assert [r.node_name for r in res] == ["node1", "node1"]  # List order: node1 first


def test_scheduler_with_resources_uploads_once_per_snapshot(msh):
    ctx = RecordingCtx()
    s = msh.Scheduler(ctx=ctx, resources=("cpu", "memory"))
    s.schedule_sequential(PODS, NODES)
    s.schedule_sequential(PODS[:1])
    kinds = [c if isinstance(c, str) else c[0] for c in ctx.calls]
    assert kinds == ["set_plugins", "upload_nodes", "upload_node_resources", "schedule_sequential_fit",
                     "schedule_sequential_fit"]
    # (nres, n) in List order (node1, node2); cpu in milli, a missing value 0
    assert ctx.calls[2][1].tolist() == [[500, 2000], [0, 2**30]]
    assert ctx.calls[3][1].tolist() == [[100, 0], [2**20, 0]] and ctx.calls[4][1].tolist() == [[100], [2**20]]
    s.update_nodes(NODES)  # a new snapshot: uploaded again
    s.schedule_sequential([])
    kinds = [c if isinstance(c, str) else c[0] for c in ctx.calls]
    assert kinds[5:] == ["upload_nodes", "upload_node_resources", "schedule_sequential_fit"]
    assert ctx.calls[-1][1].shape == (2, 0)
