"""CPU references for sequential-commit mode with the two preference scores (include/minisched_hip.h, "Preferred
node affinity and PreferNoSchedule scores": msh_schedule_sequential_prefs). Neither is the code under test; test
infrastructure only.

The contract, per pod j in order: the feasible set F is classes_ref's (filter list, count < eff, every positive
request fits, the group's zone skew, bit c of bits[i] when a class column is present and c >= 0). With A and T the raw
values of the pod's class ([C][n] each; a pod of class -1, or any pod without a preference column, has 0 everywhere):
    maxA = max over F of A,  na_i = 0 if maxA == 0 else 100 * A_i // maxA
    maxT = max over F of T,  nt_i = 100 if maxT == 0 else 100 - 100 * T_i // maxT
    total_i = classes_ref's total_i + w_aff * na_i + w_taint * nt_i
and the first maximum in List order wins; status and commit are classes_ref's.

`serial` (a plain Python loop over pods and nodes in Python ints, tiny shapes) and `per_pod` (one pod at a time with
the nodes in numpy int64) are seq_ref's two loops with every later feature left absent.
Neither packs keys, prefetches or keeps a running maximum.

Arguments are classes_ref.serial's up to pod_class, then (A, T, w_aff, w_taint); bits may be None with n_classes > 0
(every node admits every class), A and T may be None (zeros). Both return (idx, score, status, counts after, used
after, cnt after). With `trace` a list, every pod that reaches scoring appends (class, maxA, maxT). `gen_case` is the seeded generator of the GPU sweep; tests/test_prefs.py checks on the references
alone that it reaches what the sweep is for.
"""
from __future__ import annotations

import numpy as np

import classes_ref as KR
import resource_score_ref as RS
import spread_ref as S
import spread_score_ref as X

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, counts=None, cnt=None, trace=None):
    import seq_ref
    return seq_ref.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                          max_skew, mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, counts=counts,
                          cnt=cnt, prefs_trace=trace)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, counts=None, cnt=None, trace=None):
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                           max_skew, mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, counts=counts,
                           cnt=cnt, prefs_trace=trace)


A_VALUES = (0, 10, 50, 100)
T_VALUES = (0, 1, 2)


def gen_prefs(rng, n: int, n_classes: int):
    """A and T, [C][n]: a third of the classes prefers nothing, the others draw A from A_VALUES and T from T_VALUES
    per node, with the nonzero values on about a tenth of the nodes so that the best-preferred nodes fill mid-call."""
    A = np.zeros((n_classes, n), np.uint16)
    T = np.zeros((n_classes, n), np.uint16)
    for c in range(n_classes):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            continue
        if kind in (1, 2):
            A[c] = rng.choice(A_VALUES, n) * (rng.random(n) < 0.1)
        if kind == 2 or rng.random() < 0.5:
            T[c] = rng.choice(T_VALUES, n) * (rng.random(n) < 0.9)
    return A, T


def gen_case(seed: int, max_n: int = 700, max_p: int = 300) -> dict:
    """One case of the random sweep: classes_ref.gen_case's table, groups, amounts, plugins and class masks (every
    third seed runs with resource score mode NONE) with raw values from gen_prefs, weights drawn from [0, 100] (one of
    them 0 in a fifth of the cases), small pod capacities so that preferred nodes fill, and every other seed
    without a class-bits column."""
    c = KR.gen_case(seed, max_n, max_p)
    rng = np.random.default_rng(2 * 10**6 + seed)
    n, p = c["n"], c["p"]
    A, T = gen_prefs(rng, n, c["C"])
    w_aff, w_taint = int(rng.integers(1, 101)), int(rng.integers(1, 101))
    pick = rng.random()
    if pick < 0.1:
        w_aff = 0
    elif pick < 0.2:
        w_taint = 0
    # the packed key holds 100 * (W_res + w_aff + w_taint) <= 65,534
    c["rs_weight"] = int(min(int(c["rs_weight"]), 655 - w_aff - w_taint))
    if (seed // 2) % 2:
        c["bits"] = None
    c["cap"] = rng.integers(1, 4, n).astype(np.int64)
    c.update(A=A, T=T, w_aff=w_aff, w_taint=w_taint)
    return c
