"""CPU references for sequential-commit mode with the NodeResourcesBalancedAllocation score (include/minisched_hip.h,
"NodeResourcesBalancedAllocation": msh_schedule_sequential_balanced). Neither is the code under test; test
infrastructure only.

The contract: soft_spread_ref's, with w_balanced * BS added to every feasible node's total. For pod j against node i,
with r in {0, 1} the table's first two resources:
    q_r = used_r[i] + req[r][j],  c_r = alloc_r[i]
    f_r = 1.0 if c_r == 0 else float(q_r) / float(c_r);  f_r = 1.0 if f_r > 1.0
    BS  = int((1.0 - abs(f_0 - f_1)) * 100.0)          (truncation)
in IEEE double, every operation rounded once. `float(q) / float(c)`, not `q / c`: Python's true division of two ints
rounds the exact ratio once, which differs from the rule for amounts above 2^53, where the conversions round first.

`serial` and `per_pod` are seq_ref's two loops without the inter-pod conjunct. The first takes the term from `bs`, in
Python ints and floats (tiny shapes); the second from `bs_nodes`, the nodes in numpy (astype(float64) rounds to nearest
even, `/`, `-` and `*` on float64 arrays are single IEEE operations, astype(int64) truncates).

Arguments are soft_spread_ref.serial's up to w_spread, then w_balanced. `bs_exact`, `bs_f32` and `bs_rounded` are the
three evaluations the rule is not: tests/test_balanced.py searches for the inputs on which each differs from `bs`, the
decider triples that the GPU tests place on nodes. `gen_case` is the seeded generator of the GPU sweep.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import resource_score_ref as RS
import soft_spread_ref as SR
import spread_ref as S

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES
SCHEDULE_ANYWAY = SR.SCHEDULE_ANYWAY
SCORE_MAX = 1 << 55


def frac(q: int, c: int) -> float:
    f = 1.0 if c == 0 else float(q) / float(c)
    return 1.0 if f > 1.0 else f


def bs(q0: int, c0: int, q1: int, c1: int) -> int:
    """The rule."""
    d = frac(q0, c0) - frac(q1, c1)   # rounded once
    u = 1.0 - abs(d)                  # once more
    return int(u * 100.0)             # and the product; int() truncates


def _exact_frac(q: int, c: int) -> Fraction:
    return Fraction(1) if c == 0 else min(Fraction(q, c), Fraction(1))


def bs_exact(q0, c0, q1, c1) -> int:
    """floor of the exact rational value: not the rule."""
    return int((1 - abs(_exact_frac(q0, c0) - _exact_frac(q1, c1))) * 100)


def bs_f32(q0, c0, q1, c1) -> int:
    """The same operations in float32: not the rule."""
    f = np.float32

    def fr(q, c):
        x = f(1.0) if c == 0 else f(q) / f(c)
        return f(1.0) if x > f(1.0) else x
    return int((f(1.0) - abs(fr(q0, c0) - fr(q1, c1))) * f(100.0))


def bs_rounded(q0, c0, q1, c1) -> int:
    """float64 with the product rounded to nearest instead of truncated: not the rule."""
    u = 1.0 - abs(frac(q0, c0) - frac(q1, c1))
    return int(np.rint(u * 100.0))


def bs_nodes(alloc, used, rq) -> np.ndarray:
    """BS of every node in numpy: alloc, used [>= 2][n] int64, rq the pod's requests."""
    f = []
    for r in (0, 1):
        q = (used[r] + np.int64(int(rq[r]))).astype(np.float64)   # int64 -> double, to nearest even
        c = alloc[r].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = q / c
        x = np.where(alloc[r] == 0, 1.0, x)
        f.append(np.where(x > 1.0, 1.0, x))
    d = f[0] - f[1]
    u = 1.0 - np.abs(d)
    return (u * 100.0).astype(np.int64)


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, w_balanced,
           counts=None, cnt=None, moved=None):
    """`moved`, a list: every placed pod appends (j, node, BS of that node)."""
    import seq_ref
    return seq_ref.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                          max_skew, mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread,
                          w_balanced, counts=counts, cnt=cnt, moved=moved)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, w_balanced,
            counts=None, cnt=None):
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                           max_skew, mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread,
                           w_balanced, counts=counts, cnt=cnt)


def gen_case(seed: int, max_n: int = 700, max_p: int = 300) -> dict:
    """One case of the random sweep: soft_spread_ref.gen_case's table, groups, modes, plugins, classes, preference
    values and weights, with 2..4 resources and amounts redrawn for the balanced term: uneven nodes (a third cpu-rich,
    a third memory-rich, the rest even; a few with a capacity of 0 in one resource, a few partly used) against pods
    that are cpu-heavy, memory-heavy, even, or without requests, in a unit of 1, 1000, 2^31 or 2^40, so that the
    node with the most free room and the node that ends up most even are seldom the same. w_balanced in [1, 100],
    the resource weight lowered so that the key holds the sum."""
    c = SR.gen_case(seed, max_n, max_p)
    rng = np.random.default_rng(4 * 10**6 + seed)
    n, p = c["n"], c["p"]
    nres = int(rng.integers(2, 5))
    unit = int(rng.choice([1, 1000, 2**31, 2**40]))
    kind = rng.integers(0, 3, n)
    base = rng.integers(40, 400, (nres, n))
    base[0] = np.where(kind == 0, base[0] * 3, base[0])
    base[1] = np.where(kind == 1, base[1] * 3, base[1])
    alloc = (base * unit).astype(np.int64)
    alloc[rng.random((nres, n)) < 0.02] = 0
    used = ((rng.random((nres, n)) < 0.3) * rng.integers(0, 40, (nres, n)) * unit).astype(np.int64)
    pk = rng.integers(0, 4, p)
    req = rng.integers(0, 6, (nres, p))
    req[0] = np.where(pk == 0, req[0] + rng.integers(5, 30, p), req[0])
    req[1] = np.where(pk == 1, req[1] + rng.integers(5, 30, p), req[1])
    req[:, pk == 3] = 0
    req = (req * unit).astype(np.int64)
    rw = rng.integers(0, 101, nres)
    rw[int(rng.integers(0, nres))] = int(rng.integers(1, 101))
    w_balanced = int(rng.integers(1, 101))
    c["rs_weight"] = int(max(1, min(int(c["rs_weight"]), 655 - c["w_aff"] - c["w_taint"] - c["w_spread"] - w_balanced)))
    c["cap"] = rng.integers(1, 6, n).astype(np.int64) if seed % 5 else c["cap"]
    c.update(nres=nres, alloc=alloc, used=used, req=req, rw=[int(x) for x in rw], w_balanced=w_balanced)
    return c
