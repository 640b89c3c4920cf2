"""CPU references for sequential-commit mode with per-class node masks (include/minisched_hip.h, "Static node
filters: per-class node masks": msh_schedule_sequential_classes). Neither is the code under test; test
infrastructure only.

The contract, per pod j in order, with group g = group[j] (anything outside [0, G) counts as -1) and class
c = pod_class[j] (anything outside [0, C) counts as -1): node i is feasible iff it is feasible for
msh_schedule_sequential_spread_scored (filter list, count[i] < eff[i], every positive request fits, and for g >= 0 a
zone and cnt[g][zone[i]] + 1 - min over Zset of cnt[g] <= max_skew[g]) and, for c >= 0, bit c of bits[i] is set.
Status, NodeNumber's normalizer extents, the resource score (modes LEAST / MOST; NONE: NodeNumber alone), the first
maximum in List order and the commit are taken over that set; a class does not change what a commit writes, and the
spread minimum stays over Zset.

1. `serial`: a plain Python triple loop (pod, node, resource) in Python ints. Tiny shapes.
2. `per_pod`: written separately, one pod at a time with the nodes in numpy int64.
Neither forms an availability mask or packs keys: a node's verdict is read from bits[i] >> c & 1 directly.

Arguments are spread_score_ref.serial's up to rw, then (bits, n_classes, pod_class); zone, group and pod_class may be
None (no node has a zone, no pod a group, no pod a class). Both return (idx, score, status, counts after, used after,
cnt after). `gen_case` is the seeded generator of the random sweeps.
"""
from __future__ import annotations

import numpy as np

import resource_score_ref as RS
import spread_ref as S
import spread_score_ref as X

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES
MAX_CLASSES = 64


def clean_classes(pod_class, n_classes: int, p: int) -> list[int]:
    if pod_class is None:
        return [-1] * p
    return [int(c) if 0 <= int(c) < n_classes else -1 for c in pod_class]


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           mode, weight, rw, bits, n_classes, pod_class, counts=None, cnt=None):
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
    cls = clean_classes(pod_class, n_classes, p)
    word = [int(b) for b in bits] if bits is not None else [0] * n
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
            if k >= 0 and not (word[i] >> k) & 1:
                continue
            if has_nu and unsched[i] and not tol:
                continue
            if not count[i] < eff[i]:
                continue
            fits = True
            for r in range(nres):
                if rq[r] > 0 and rq[r] > al[r][i] - us[r][i]:
                    fits = False
            if not fits:
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
        if mode != NONE:
            for m, i in enumerate(feas):
                rs = RS.resource_score(mode, [al[r][i] for r in range(nres)], [us[r][i] + rq[r] for r in range(nres)], rw)
                total[m] = O._wrap64(total[m] + int(weight) * rs)
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
            mode, weight, rw, bits, n_classes, pod_class, counts=None, cnt=None):
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
    word = np.zeros(n, np.uint64) if bits is None else np.asarray(bits, np.uint64)
    blocked = np.asarray(unsched, bool) if "NodeUnschedulable" in plugins.filters else np.zeros(n, bool)
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    lowest = np.iinfo(np.int64).min
    for j in range(p):
        pd = int(pod_digit[j])
        g = int(grp[j]) if 0 <= grp[j] < G else -1
        k = int(cls[j]) if 0 <= cls[j] < n_classes else -1
        feas = count < eff
        if not pod_tol[j]:
            feas = feas & ~blocked
        if k >= 0:
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
            total = total + (acc // den) * np.int64(O._wrap64(int(weight)))
        sel = int(np.argmax(np.where(feas, total, lowest)))  # argmax returns the first maximum
        idx[j], score[j] = sel, total[sel]
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0:
            c[g, zn[sel]] += 1
    return idx, score, status, count.astype(np.int32), us, c.astype(np.int32)


DENSITIES = ("none", "one", "tenth", "half", "all")


def gen_bits(rng, n: int, n_classes: int):
    """One word per node for n_classes classes, each class of a density drawn from DENSITIES; returns (bits, the
    density names by class)."""
    bits = np.zeros(n, np.uint64)
    kinds = []
    for c in range(n_classes):
        kind = DENSITIES[int(rng.integers(0, len(DENSITIES)))]
        kinds.append(kind)
        if kind == "none":
            m = np.zeros(n, bool)
        elif kind == "one":
            m = np.zeros(n, bool)
            m[int(rng.integers(0, n))] = True
        elif kind == "all":
            m = np.ones(n, bool)
        else:
            m = rng.random(n) < (0.1 if kind == "tenth" else 0.5)
        bits |= m.astype(np.uint64) << np.uint64(c)
    return bits, kinds


def gen_case(seed: int, max_n: int = 2048, max_p: int = 2000) -> dict:
    """One case of the random sweep: spread_score_ref.gen_case's table, groups, amounts and plugins (its odd and even
    seeds give LEAST and MOST; every third seed here runs unscored) with 1..64 classes of densities drawn from
    {admits none, exactly one node, ~10%, ~50%, all} and about a fifth of the pods without a class."""
    c = X.gen_case(seed, max_n, max_p)
    rng = np.random.default_rng(10**6 + seed)
    C = int(rng.choice([1, 2, 5, 16, 33, 64]))
    bits, kinds = gen_bits(rng, c["n"], C)
    pod_class = rng.integers(0, C, c["p"]).astype(np.int32)
    pod_class[rng.random(c["p"]) < 0.2] = -1
    if seed % 3 == 0:
        c["score_mode"] = NONE
    c.update(C=C, bits=bits, kinds=kinds, pod_class=pod_class)
    return c
