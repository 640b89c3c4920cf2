"""Resource-aware scoring in sequential-commit mode (msh_set_resource_score): everything that needs no GPU. The two
CPU references agree, mode NONE is the unscored reference, hand-worked placements hold, the random sweep the GPU
test runs does exercise the feature, the entry points are declared, bound and exported, and Scheduler validates
its arguments."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import node_capacity_ref as CR
import resource_fit_ref as R
import resource_score_ref as S

ROOT = Path(__file__).resolve().parents[1]
NEW = ("msh_set_resource_score", "msh_get_resource_score", "msh_seq_fit_max_nodes")
SWEEP_SEED, SWEEP_CASES = 20267, 40
SWEEP_SIZES = (9, 33, 64, 65, 200, 257, 300)


def same(a, b, what):
    for x, y, name in zip(a, b, ("idx", "score", "status", "counts", "used")):
        assert np.array_equal(x, y), (what, name)


def eff_of(c):
    if c["cap"] is not None:
        return CR.effective(c["cap"], c["scalar"])
    return np.full(c["n"], c["scalar"], np.int64) if c["scalar"] else R.no_limit(c["n"])


def run(ref, O, c, mode=None):
    return ref(O, c["u"], c["nd"], c["pd"], c["pt"], c["plugins"], eff_of(c), c["alloc"], c["used"], c["req"],
               c["mode"] if mode is None else mode, c["weight"], c["rw"])


def test_the_two_references_agree(oracle):
    rng = np.random.default_rng(20266)
    for case in range(150):
        c = S.sweep_case(oracle, rng, case, (0, 1, 2, 5, 9, 14))
        c["p"] = min(c["p"], 40)
        for k in ("pd", "pt"):
            c[k] = c[k][: c["p"]]
        c["req"] = c["req"][:, : c["p"]]
        if case % 4 == 0 and c["n"]:  # amounts at the top of the range, odd divisors, over-committed nodes
            f = S.SCORE_MAX // (int(max(c["alloc"].max(initial=1), c["used"].max(initial=1), 1)) + 1)
            c["alloc"] = c["alloc"] * f + (c["alloc"] > 0)
            c["used"], c["req"] = c["used"] * f, c["req"] * f
        if case % 7 == 0 and c["n"]:
            c["used"][:, 0] = np.maximum(c["used"][:, 0], 1)
            c["alloc"][:, 0] = c["used"][:, 0] - 1  # q > c on node 0
        same(run(S.serial, oracle, c), run(S.per_pod, oracle, c), case)


def test_mode_none_is_the_unscored_reference(oracle):
    rng = np.random.default_rng(3)
    for case in range(30):
        c = S.sweep_case(oracle, rng, case, (5, 9))
        want = R.serial(oracle, c["u"], c["nd"], c["pd"], c["pt"], c["plugins"], eff_of(c), c["alloc"], c["used"], c["req"])
        same(run(S.serial, oracle, c, S.NONE), want, case)
        same(run(S.per_pod, oracle, c, S.NONE), want, case)


def hand(oracle, alloc, used, req, mode, rw=None, weight=1, nd=None, pd=None, plugins=None, scalar=0):
    alloc, used, req = (np.array(a, np.int64) for a in (alloc, used, req))
    n, p = alloc.shape[1], req.shape[1]
    nd = np.zeros(n, np.int8) if nd is None else np.array(nd, np.int8)
    pd = np.zeros(p, np.int8) if pd is None else np.array(pd, np.int8)
    eff = np.full(n, scalar, np.int64) if scalar else R.no_limit(n)
    args = (oracle, np.zeros(n, np.uint8), nd, pd, np.zeros(p, np.uint8), plugins or oracle.PluginSet(), eff, alloc,
            used, req, mode, weight, rw or [1] * len(alloc))
    a, b = S.serial(*args), S.per_pod(*args)
    same(a, b, "hand-worked")
    return a


def test_hand_worked_placements(oracle):
    # LEAST on three equal empty nodes: round-robin. Every node matches (score 10 each); after a pod lands, that
    # node's (c - q) * 100 / c drops below the others'.
    idx, score, *_ = hand(oracle, [[10, 10, 10]], [[0, 0, 0]], [[1] * 7], S.LEAST)
    assert idx.tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert score.tolist() == [10 + 90, 10 + 90, 10 + 90, 10 + 80, 10 + 80, 10 + 80, 10 + 70]
    # MOST fills node 0 first: q * 100 / c grows where pods already are; then node 1
    idx, score, _, cnt, used = hand(oracle, [[3, 3, 3]], [[0, 0, 0]], [[1] * 7], S.MOST)
    assert idx.tolist() == [0, 0, 0, 1, 1, 1, 2] and cnt.tolist() == [3, 3, 1] and used.tolist() == [[3, 3, 1]]
    assert score.tolist() == [10 + 33, 10 + 66, 10 + 100, 10 + 33, 10 + 66, 10 + 100, 10 + 33]
    # a resource of weight 0 is fitted but does not move the score: resource 1 would prefer node 1 under LEAST
    idx, score, *_ = hand(oracle, [[10, 10], [10, 100]], [[0, 0], [5, 0]], [[1], [1]], S.LEAST, rw=[1, 0])
    assert idx.tolist() == [0] and score.tolist() == [10 + 90]
    idx, score, *_ = hand(oracle, [[10, 10], [10, 100]], [[0, 0], [5, 0]], [[1], [1]], S.LEAST, rw=[1, 1])
    assert idx.tolist() == [1] and score.tolist() == [10 + (90 + 99) // 2]
    # ... but it is still fitted: node 0 has no room for resource 1
    idx, *_ = hand(oracle, [[10, 10], [10, 100]], [[0, 5], [10, 0]], [[1], [1]], S.LEAST, rw=[1, 0])
    assert idx.tolist() == [1]
    # c == 0 scores 0 (a zero request is feasible there); q > c scores 0 (node 1: used 6 of 5)
    for mode in (S.LEAST, S.MOST):
        idx, score, *_ = hand(oracle, [[0, 5, 8]], [[0, 6, 4]], [[0]], mode)
        assert idx.tolist() == [2] and score.tolist() == [10 + 50]
        idx, score, *_ = hand(oracle, [[0, 5]], [[0, 6]], [[0]], mode)
        assert idx.tolist() == [0] and score.tolist() == [10]
    # the weighted mean truncates once, after the sum: (33 * 3 + 66 * 1) / 4 = 41, not 24 + 16
    idx, score, *_ = hand(oracle, [[3], [3]], [[0], [1]], [[1], [1]], S.MOST, rw=[3, 1])
    assert score.tolist() == [10 + (33 * 3 + 66) // 4]
    # the plugin weight multiplies RS; a match (10) against a non-match with the better resource score
    idx, score, *_ = hand(oracle, [[100, 100]], [[50, 40]], [[0]], S.LEAST, nd=[0, 1], weight=1)
    assert idx.tolist() == [0] and score.tolist() == [60]  # 10 + 50 against 0 + 60: a tie, the lower index
    idx, score, *_ = hand(oracle, [[100, 100]], [[50, 39]], [[0]], S.LEAST, nd=[0, 1], weight=1)
    assert idx.tolist() == [1] and score.tolist() == [61]
    idx, score, *_ = hand(oracle, [[100, 100]], [[50, 49]], [[0]], S.LEAST, nd=[0, 1], weight=2**32)
    assert idx.tolist() == [1] and score.tolist() == [51 * 2**32]


def sweep(oracle):
    rng = np.random.default_rng(SWEEP_SEED)
    return [S.sweep_case(oracle, rng, case, SWEEP_SIZES) for case in range(SWEEP_CASES)]


def differs_from_unscored(oracle, c):
    got = run(S.per_pod, oracle, c)
    plain = run(S.per_pod, oracle, c, S.NONE)
    return not np.array_equal(got[0], plain[0])


def test_the_sweep_exercises_the_feature(oracle):
    """At least 90% of the sweep's cases place some pod elsewhere than the unscored reference does."""
    cases = sweep(oracle)
    share = sum(differs_from_unscored(oracle, c) for c in cases) / len(cases)
    assert share >= 0.9, share
    assert {c["mode"] for c in cases} == {S.LEAST, S.MOST} and {c["nres"] for c in cases} == {1, 2, 3, 4}


def test_declared_bound_and_exported(msh):
    N = msh._native
    header = (ROOT / "include" / "minisched_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|void|const char\*)\s+(msh_\w+)\(", header, re.M))
    assert set(NEW) <= declared and set(N.EXPORTED) == declared
    lib = N.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    assert "MSH_ABI_VERSION 8" in header
    assert (N.MSH_RESOURCE_SCORE_NONE, N.MSH_RESOURCE_SCORE_LEAST_ALLOCATED, N.MSH_RESOURCE_SCORE_MOST_ALLOCATED) == (0, 1, 2)
    assert N.RESOURCE_SCORE_MAX == 1 << 55 and "#define MSH_RESOURCE_SCORE_MAX ((int64_t)1 << 55)" in header
    go = (ROOT / "go" / "minisched" / "gpusched" / "gpusched.go").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, name


def test_null_ctx_and_limits_without_a_device(msh):
    N = msh._native
    lib, inv = N.lib(), N.MSH_ERR_INVALID
    w = np.ones(2, np.int32)
    out = N.C.c_int32(-1)
    assert lib.msh_set_resource_score(None, 1, 1, 2, N.ptr(w)) == inv
    assert lib.msh_get_resource_score(None, None, None, None, None) == inv
    assert lib.msh_seq_fit_max_nodes(None, 1, 0, N.C.byref(out)) == inv


def test_scheduler_argument_validation(msh):
    from test_resource_fit import RecordingCtx

    class Ctx(RecordingCtx):
        def set_resource_score(self, mode, weight=1, resource_weights=None):
            self.calls.append(("set_resource_score", mode, weight, list(resource_weights)))

    for kw in (dict(resource_score="least"),                                             # without resources
               dict(resource_weights=[1]),                                               # without resource_score
               dict(resources=("cpu",), resource_weights=[1]),
               dict(resources=("cpu",), resource_score="spread"),
               dict(resources=("cpu", "memory"), resource_score="most", resource_weights=[1]),
               dict(resources=("cpu", "memory"), resource_score="most", resource_weights={"pods": 1}),
               dict(resources=("cpu", "memory"), resource_score="most", resource_weights=[0, 0]),
               dict(resources=("cpu", "memory"), resource_score="most", resource_weights=[1, 101])):
        ctx = Ctx()
        with pytest.raises(ValueError):
            msh.Scheduler(ctx=ctx, **kw)
        assert not any(isinstance(c, tuple) and c[0] == "set_resource_score" for c in ctx.calls), kw
    ctx = Ctx()
    msh.Scheduler(ctx=ctx, resources=("cpu", "memory"))
    assert ctx.calls == ["set_plugins"]  # no resource score: the setter is never called
    for kw, want in ((dict(resource_score="least"), ("least", 1, [1, 1])),
                     (dict(resource_score="most", resource_score_weight=5, resource_weights={"memory": 3}), ("most", 5, [0, 3])),
                     (dict(resource_score=1, resource_weights=(2, 0)), (1, 1, [2, 0]))):
        ctx = Ctx()
        msh.Scheduler(ctx=ctx, resources=("cpu", "memory"), **kw)
        assert ctx.calls == ["set_plugins", ("set_resource_score", *want)]
