"""Per-node pod capacity (msh_upload_node_capacity and friends): everything that needs no GPU. The two CPU
references agree with each other, the four entry points are declared, bound and exported, NodeCache keeps
the column under informer events, and arguments are validated before any device is touched."""
from __future__ import annotations

import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import pytest

import node_capacity_ref as R
from oracle_ctx import OracleCtx

ROOT = Path(__file__).resolve().parents[1]
NEW = ("msh_upload_node_capacity", "msh_patch_node_capacity", "msh_clear_node_capacity", "msh_node_capacity")
INT32_MAX = R.INT32_MAX


def random_plugins(O, rng):
    filters = ["NodeUnschedulable"] if rng.random() < 0.8 else []
    prescore = ["NodeNumber"] if rng.random() < 0.85 else []
    if rng.random() < 0.1:
        return O.PluginSet(filters, prescore, [], [], [])
    return O.PluginSet(filters, prescore, ["NodeNumber"], [int(rng.choice([1, 3, 2**32]))], [int(rng.integers(0, 4))])


def test_the_two_references_agree(oracle):
    """The uniform-capacity identity behind reference 1 (the C oracle with shifted counts) against the plain
    serial loop, 300 small random cases: capacities with zeros, carried-in counts above and below them,
    an optional scalar, every plugin variation."""
    rng = np.random.default_rng(20251)
    for case in range(300):
        n, p = int(rng.integers(0, 13)), int(rng.integers(0, 41))
        unsched = (rng.random(n) < 0.3).astype(np.uint8)
        nd = rng.integers(-1, 10, n).astype(np.int8)
        pd = rng.integers(-1, 10 if case % 3 else 3, p).astype(np.int8)
        pt = (rng.random(p) < 0.4).astype(np.uint8)
        cap = rng.choice([0, 1, 2, 3, 7, 10**6], n)
        k = rng.integers(0, 5, n)
        scalar = int(rng.choice([0, 0, 1, 2, 5]))
        eff = R.effective(cap, scalar)
        pl = random_plugins(oracle, rng)
        a = R.via_oracle(oracle, unsched, nd, pd, pt, pl, eff, k)
        b = R.serial(oracle, unsched, nd, pd, pt, pl, eff, k)
        for x, y, what in zip(a, b, ("idx", "score", "status", "counts")):
            assert np.array_equal(x, y), (case, what, pl)


def test_serial_reference_takes_int32_max(oracle):
    """INT32_MAX is in effect unlimited: the serial loop places like no capacity at all."""
    rng = np.random.default_rng(7)
    n, p = 9, 60
    unsched = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(-1, 10, n).astype(np.int8)
    pd = rng.integers(-1, 10, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    pl = oracle.PluginSet()
    got = R.serial(oracle, unsched, nd, pd, pt, pl, np.full(n, INT32_MAX, np.int64))
    want = oracle.c_schedule_sequential(unsched, nd, pd, pt, pl, max_pods=0)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def test_new_entry_points_are_declared_bound_and_exported(msh):
    hdr = (ROOT / "include" / "minisched_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = msh._native.lib()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert name in msh._native.EXPORTED and name in msh._native._SIGS, name
        assert hasattr(lib, name), name
    assert "#define MSH_ABI_VERSION 8" in hdr and lib.msh_abi_version() == 8  # additive
    go = (ROOT / "go" / "minisched" / "gpusched" / "gpusched.go").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, name


def test_null_ctx_is_invalid_without_a_device(msh):
    lib, inv = msh._native.lib(), msh._native.MSH_ERR_INVALID
    cap = np.ones(3, np.int32)
    idx = np.arange(3, dtype=np.int32)
    present = np.zeros(1, np.int32)
    assert lib.msh_upload_node_capacity(None, 3, msh._native.ptr(cap)) == inv
    assert lib.msh_patch_node_capacity(None, 3, msh._native.ptr(idx), msh._native.ptr(cap)) == inv
    assert lib.msh_clear_node_capacity(None) == inv
    assert lib.msh_node_capacity(None, None, present.ctypes.data_as(msh._native.C.POINTER(msh._native.C.c_int32))) == inv


def test_python_side_validation(msh):
    dc = msh.DeviceContext
    with pytest.raises(ValueError):
        dc._capacities(np.array([1.5, 2.0]))
    with pytest.raises(ValueError):
        dc._capacities(np.array([2**31], np.int64))
    assert dc._capacities([0, INT32_MAX]).dtype == np.int32
    assert dc._capacities(np.array([-1], np.int64))[0] == -1  # negatives reach the library: MSH_ERR_INVALID
    snap = importlib_snapshot(msh)
    with pytest.raises(ValueError):
        snap.node_allocatable_pods(N("a", pods=-1))
    with pytest.raises(ValueError):
        snap.node_allocatable_pods(N("a", pods=2**31))
    assert snap.node_allocatable_pods({"metadata": {"name": "n1"}, "status": {"allocatable": {"pods": "110"}}}) == 110
    assert snap.node_allocatable_pods({"metadata": {"name": "n1"}}) is None
    assert snap.node_allocatable_pods(N("a")) is None


def importlib_snapshot(msh):
    import importlib
    return importlib.import_module(msh.__name__ + ".snapshot")


@dataclass
class N:
    name: str
    unschedulable: bool = False
    pods: int | None = None

    @property
    def allocatable_pods(self):
        return self.pods


def test_pack_nodes_carries_the_column_in_list_order(msh):
    snap = importlib_snapshot(msh)
    t = snap.pack_nodes([N("node2", pods=5), N("node1"), N("node3", pods=0)])
    assert t.names == ["node1", "node2", "node3"]
    assert t.allocatable_pods.dtype == np.int32 and t.allocatable_pods.tolist() == [INT32_MAX, 5, 0]
    assert snap.pack_nodes([N("node2"), N("node1")]).allocatable_pods is None


class CapCtx(OracleCtx):
    """The oracle-backed context with the capacity column and the library's lifetime rules."""

    def __init__(self):
        super().__init__()
        self.cap = None

    def upload_nodes(self, unsched, digit):
        super().upload_nodes(unsched, digit)
        self.cap = None  # msh_upload_nodes drops the column

    def upload_node_capacity(self, cap):
        cap = np.array(cap, np.int32)
        assert len(cap) == self.n_nodes and (cap >= 0).all()
        self.cap = cap
        self.calls.append(("cap_upload", len(cap)))

    def patch_node_capacity(self, idx, cap):
        assert self.cap is not None
        idx = np.asarray(idx, np.int64)
        assert len(np.unique(idx)) == len(idx) and (idx >= 0).all() and (idx < self.n_nodes).all()
        self.cap[idx] = cap
        self.calls.append(("cap_patch", sorted(int(i) for i in idx)))

    def clear_node_capacity(self):
        self.cap = None
        self.calls.append(("cap_clear",))

    def node_capacity(self):
        return None if self.cap is None else self.cap.copy()


def test_nodecache_keeps_the_column(msh):
    import importlib
    NodeCache = importlib.import_module(msh.__name__ + ".nodecache").NodeCache
    ctx = CapCtx()
    cache = NodeCache([N("node1", pods=3), N("node3", pods=7), N("node2")])
    assert cache.capacity.tolist() == [3, INT32_MAX, 7]
    assert cache.sync(ctx) == "upload" and ctx.node_capacity().tolist() == [3, INT32_MAX, 7]
    assert ctx.calls == [("upload", 3), ("cap_upload", 3)]
    # a capacity-only Update: one msh_patch_node_capacity, no table call
    ctx.calls.clear()
    cache.update(N("node3", pods=7), N("node3", pods=2))
    assert cache.dirty() and cache.sync(ctx) == "patch"
    assert ctx.calls == [("cap_patch", [2])] and ctx.node_capacity().tolist() == [3, INT32_MAX, 2]
    assert not cache.dirty() and cache.sync(ctx) == "clean"
    # a cordon and a capacity change together: the table patch keeps the column, the capacity patch follows
    ctx.calls.clear()
    cache.update(N("node1", pods=3), N("node1", unschedulable=True, pods=4))
    assert cache.sync(ctx) == "patch"
    assert ctx.calls == [("patch", [0]), ("cap_patch", [0])] and ctx.node_capacity().tolist() == [4, INT32_MAX, 2]
    # Add and Delete re-upload the column with the table, in the new List order
    ctx.calls.clear()
    cache.add(N("node0", pods=9))
    assert cache.sync(ctx) == "upload" and ctx.node_capacity().tolist() == [9, 4, INT32_MAX, 2]
    cache.delete("node1")
    assert cache.sync(ctx) == "upload" and ctx.node_capacity().tolist() == [9, INT32_MAX, 2]
    assert ctx.calls == [("upload", 4), ("cap_upload", 4), ("upload", 3), ("cap_upload", 3)]
    # the last capacities go: the column is cleared; the first one comes back: uploaded whole
    ctx.calls.clear()
    cache.update(N("node0", pods=9), N("node0"))
    cache.update(N("node3", pods=2), N("node3"))
    assert cache.capacity is None and cache.sync(ctx) == "patch" and ctx.node_capacity() is None
    cache.update(N("node2"), N("node2", pods=1))
    assert cache.sync(ctx) == "patch" and ctx.node_capacity().tolist() == [INT32_MAX, 1, INT32_MAX]
    assert ctx.calls == [("cap_clear",), ("cap_upload", 3)]
    # a fresh context after mark_stale gets table and column again
    ctx2 = CapCtx()
    cache.mark_stale()
    assert cache.sync(ctx2) == "upload" and ctx2.node_capacity().tolist() == [INT32_MAX, 1, INT32_MAX]


def test_nodecache_without_capacities_makes_no_capacity_call(msh):
    import importlib
    NodeCache = importlib.import_module(msh.__name__ + ".nodecache").NodeCache
    ctx = CapCtx()
    cache = NodeCache([N("node1"), N("node2")])
    cache.sync(ctx)
    cache.update(N("node1"), N("node1", unschedulable=True))
    cache.sync(ctx)
    assert cache.capacity is None and ctx.calls == [("upload", 2), ("patch", [0])]
