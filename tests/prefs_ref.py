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

1. `serial`: a plain Python loop over pods and nodes in Python ints. Tiny shapes.
2. `per_pod`: written separately, one pod at a time with the nodes in numpy int64.
Neither packs keys, prefetches or keeps a running maximum.

Arguments are classes_ref.serial's up to pod_class, then (A, T, w_aff, w_taint); bits may be None with n_classes > 0
(every node admits every class), A and T may be None (zeros). Both return (idx, score, status, counts after, used
after, cnt after). `gen_case` is the seeded generator of the GPU sweep; tests/test_prefs.py checks on the references
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
    n, p = len(unsched), len(pod_digit)
    assert n * p <= 2 * 10**5, "the serial loop is for tiny shapes"
    nres, G = len(alloc), len(max_skew)
    eff = [int(x) for x in eff]
    count = [0] * n if counts is None else [int(x) for x in counts]
    al = [[int(x) for x in row] for row in alloc]
    us = [[int(x) for x in row] for row in used]
    rw = [int(x) for x in rw]
    zn = [-1] * n if zone is None else [int(z) for z in zone]
    zs = sorted({z for z in zn if z >= 0})
    sk = [int(x) for x in max_skew]
    c = [[0] * MAX_ZONES for _ in range(G)] if cnt is None else [[int(x) for x in row] for row in cnt]
    grp = [-1] * p if group is None else [int(g) if 0 <= int(g) < G else -1 for g in group]
    cls = KR.clean_classes(pod_class, n_classes, p)
    word = None if bits is None else [int(b) for b in bits]
    has_nu = "NodeUnschedulable" in plugins.filters
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    for j in range(p):
        pd, tol, g, k = int(pod_digit[j]), bool(pod_tol[j]), grp[j], cls[j]
        rq = [int(req[r][j]) for r in range(nres)]
        feas = []
        for i in range(n):
            if k >= 0 and word is not None and not (word[i] >> k) & 1:
                continue
            if has_nu and unsched[i] and not tol:
                continue
            if not count[i] < eff[i]:
                continue
            if any(rq[r] > 0 and rq[r] > al[r][i] - us[r][i] for r in range(nres)):
                continue
            if g >= 0:
                if zn[i] < 0:
                    continue
                if c[g][zn[i]] + 1 - min(c[g][z] for z in zs) > sk[g]:
                    continue
            feas.append(i)
        if not feas:
            status[j] = FIT_ERROR
            continue
        if plugins.score and not (nn_pre and 0 <= pd <= 9):  # NodeNumber.Score finds no PreScore state
            status[j] = SCORE_ERROR
            continue
        total = [0] * len(feas)
        for w, nm in zip(plugins.weights, plugins.normalize):
            raw = [10 if 0 <= int(node_digit[i]) == pd else 0 for i in feas]
            total = [O._wrap64(t + s * int(w)) for t, s in zip(total, O.normalize(int(nm), raw))]
        ra = [int(A[k][i]) if k >= 0 and A is not None else 0 for i in feas]
        rt = [int(T[k][i]) if k >= 0 and T is not None else 0 for i in feas]
        max_a, max_t = max(ra), max(rt)
        if trace is not None:
            trace.append((k, max_a, max_t))
        for m, i in enumerate(feas):
            if mode != NONE:
                rs = RS.resource_score(mode, [al[r][i] for r in range(nres)], [us[r][i] + rq[r] for r in range(nres)], rw)
                total[m] += int(weight) * rs
            na = 0 if max_a == 0 else 100 * ra[m] // max_a
            nt = 100 if max_t == 0 else 100 - 100 * rt[m] // max_t
            total[m] = O._wrap64(total[m] + int(w_aff) * na + int(w_taint) * nt)
        best = max(total)
        sel = feas[total.index(best)]  # the first maximum in List order
        idx[j], score[j] = sel, best
        count[sel] += 1
        for r in range(nres):
            us[r][sel] += rq[r]
        if g >= 0:
            c[g][zn[sel]] += 1
    return (idx, score, status, np.array(count, np.int32), np.array(us, np.int64).reshape(nres, n),
            np.array(c, np.int32).reshape(G, MAX_ZONES))


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, counts=None, cnt=None, trace=None):
    n, p = len(unsched), len(pod_digit)
    alloc = np.asarray(alloc, np.int64).reshape(-1, n)
    us = np.array(used, np.int64).reshape(-1, n)
    req = np.asarray(req, np.int64).reshape(-1, p)
    nres, G = alloc.shape[0], len(max_skew)
    if mode != NONE:
        assert max(alloc.max(initial=0), us.max(initial=0), req.max(initial=0)) <= RS.SCORE_MAX, "int64 would overflow"
        rw = np.asarray(rw, np.int64)
        scored = [r for r in range(nres) if rw[r] > 0]
        den = int(rw[scored].sum())
        safe = np.where(alloc == 0, 1, alloc)
    eff = np.asarray(eff, np.int64)
    count = np.zeros(n, np.int64) if counts is None else np.array(counts, np.int64)
    nd = np.asarray(node_digit, np.int64)
    zn = np.full(n, -1, np.int64) if zone is None else np.asarray(zone, np.int64)
    zs = np.unique(zn[zn >= 0])
    zsafe = np.where(zn >= 0, zn, 0)
    sk = np.asarray(max_skew, np.int64)
    c = np.zeros((G, MAX_ZONES), np.int64) if cnt is None else np.array(cnt, np.int64).reshape(G, MAX_ZONES)
    grp = np.full(p, -1, np.int64) if group is None else np.asarray(group, np.int64)
    cls = np.full(p, -1, np.int64) if pod_class is None else np.asarray(pod_class, np.int64)
    word = None if bits is None else np.asarray(bits, np.uint64)
    Aq = np.zeros((max(n_classes, 1), n), np.int64) if A is None else np.asarray(A, np.int64).reshape(-1, n)
    Tq = np.zeros((max(n_classes, 1), n), np.int64) if T is None else np.asarray(T, np.int64).reshape(-1, n)
    blocked = np.asarray(unsched, bool) if "NodeUnschedulable" in plugins.filters else np.zeros(n, bool)
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    lowest = np.iinfo(np.int64).min
    zeros = np.zeros(n, np.int64)
    for j in range(p):
        pd = int(pod_digit[j])
        g = int(grp[j]) if 0 <= grp[j] < G else -1
        k = int(cls[j]) if 0 <= cls[j] < n_classes else -1
        feas = count < eff
        if not pod_tol[j]:
            feas = feas & ~blocked
        if k >= 0 and word is not None:
            feas = feas & ((word >> np.uint64(k)) & np.uint64(1)).astype(bool)
        for r in range(nres):
            if req[r, j] > 0:
                feas = feas & (alloc[r] - us[r] >= req[r, j])
        if g >= 0:
            if len(zs) == 0:
                feas = np.zeros(n, bool)
            else:
                feas = feas & (zn >= 0) & (c[g][zsafe] - c[g][zs].min() < sk[g])
        if not feas.any():
            status[j] = FIT_ERROR
            continue
        if plugins.score and not (nn_pre and 0 <= pd <= 9):
            status[j] = SCORE_ERROR
            continue
        total = np.zeros(n, np.int64)
        raw = np.where((nd == pd) & (nd >= 0), 10, 0).astype(np.int64)
        for w, nm in zip(plugins.weights, plugins.normalize):
            total = total + RS._nn_scores(int(nm), raw, feas) * np.int64(O._wrap64(int(w)))
        if mode != NONE:
            acc = np.zeros(n, np.int64)
            for r in scored:
                q = us[r] + req[r, j]
                part = (alloc[r] - q) if mode == LEAST else q
                none = (alloc[r] == 0) | (q > alloc[r])
                acc += np.where(none, 0, np.where(none, 0, part) * 100 // safe[r]) * rw[r]
            total = total + (acc // den) * np.int64(int(weight))
        ra = Aq[k] if k >= 0 else zeros
        rt = Tq[k] if k >= 0 else zeros
        max_a, max_t = int(ra[feas].max()), int(rt[feas].max())
        if trace is not None:
            trace.append((k, max_a, max_t))
        na = zeros if max_a == 0 else ra * 100 // max_a
        nt = zeros + 100 if max_t == 0 else 100 - rt * 100 // max_t
        total = total + np.int64(int(w_aff)) * na + np.int64(int(w_taint)) * nt
        sel = int(np.argmax(np.where(feas, total, lowest)))  # argmax returns the first maximum
        idx[j], score[j] = sel, total[sel]
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0:
            c[g, zn[sel]] += 1
    return idx, score, status, count.astype(np.int32), us, c.astype(np.int32)


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
