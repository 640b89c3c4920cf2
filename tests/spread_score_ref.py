"""CPU references for sequential-commit mode with pod topology spread and a resource score together
(include/minisched_hip.h, "Topology spread together with a resource score": msh_schedule_sequential_spread_scored).
Neither is the code under test; test infrastructure only.

The contract, per pod j in order, with group g = group[j] (anything outside [0, G) counts as -1): the feasible set
and the status are spread_ref's (filter list, count[i] < eff[i], every positive request fits, and for g >= 0 a zone
and cnt[g][zone[i]] + 1 - min over Zset of cnt[g] <= max_skew[g]); a feasible node's total is resource_score_ref's
(NodeNumber normalized over the feasible list, plus weight x RS with q = used + req before the commit); the pod
goes to the first maximum in List order; a PLACED pod adds 1 to count[sel], its requests to used[:, sel] and, for
g >= 0, 1 to cnt[g][zone[sel]].

1. `serial`: a plain Python loop over every (pod, node) pair, Python ints, the header's formulas. Tiny shapes.
2. `per_pod`: written separately, one pod at a time with the nodes in numpy int64.
Neither forms a per-zone "allowed" set or packs (score, node) into a key: a node's verdict is computed from the cnt
array directly, and the selection is a plain first maximum over the feasible nodes' totals.

Modes as resource_score_ref's: NONE = 0 (then the call is spread_ref's), LEAST = 1, MOST = 2. Argument conventions
are spread_ref.serial's followed by resource_score_ref.serial's (mode, weight, rw); both return
(idx, score, status, counts after, used after, cnt after). `gen_case` is the seeded generator of the random sweeps.
"""
from __future__ import annotations

import numpy as np

import resource_score_ref as RS
import spread_ref as S

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           mode, weight, rw, counts=None, cnt=None):
    if mode == NONE:
        return S.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                        max_skew, counts, cnt)
    n, p = len(unsched), len(pod_digit)
    assert n * p <= 2 * 10**5, "the serial loop is for tiny shapes"
    nres, G = len(alloc), len(max_skew)
    eff = [int(x) for x in eff]
    count = [0] * n if counts is None else [int(x) for x in counts]
    al = [[int(x) for x in row] for row in alloc]
    us = [[int(x) for x in row] for row in used]
    rw = [int(x) for x in rw]
    zn = [int(z) for z in zone]
    zs = S.zset(zone)
    sk = [int(x) for x in max_skew]
    c = [[0] * MAX_ZONES for _ in range(G)] if cnt is None else [[int(x) for x in row] for row in cnt]
    grp = S.clean_groups(group, G)
    has_nu = "NodeUnschedulable" in plugins.filters
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    for j in range(p):
        pd, tol, g = int(pod_digit[j]), bool(pod_tol[j]), int(grp[j])
        rq = [int(req[r][j]) for r in range(nres)]
        feas = []
        for i in range(n):
            if has_nu and unsched[i] and not tol:
                continue
            if not count[i] < eff[i]:
                continue
            if not all(rq[r] <= al[r][i] - us[r][i] for r in range(nres) if rq[r] > 0):
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
        for k, i in enumerate(feas):
            rs = RS.resource_score(mode, [al[r][i] for r in range(nres)], [us[r][i] + rq[r] for r in range(nres)], rw)
            total[k] = O._wrap64(total[k] + int(weight) * rs)
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
            mode, weight, rw, counts=None, cnt=None):
    if mode == NONE:
        return S.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                         max_skew, counts, cnt)
    n, p = len(unsched), len(pod_digit)
    alloc = np.asarray(alloc, np.int64).reshape(-1, n)
    us = np.array(used, np.int64).reshape(-1, n)
    req = np.asarray(req, np.int64).reshape(-1, p)
    assert max(alloc.max(initial=0), us.max(initial=0), req.max(initial=0)) <= RS.SCORE_MAX, "int64 would overflow"
    nres, G = alloc.shape[0], len(max_skew)
    rw = np.asarray(rw, np.int64)
    scored = [r for r in range(nres) if rw[r] > 0]
    den = int(rw[scored].sum())
    eff = np.asarray(eff, np.int64)
    count = np.zeros(n, np.int64) if counts is None else np.array(counts, np.int64)
    nd = np.asarray(node_digit, np.int64)
    zn = np.asarray(zone, np.int64)
    in_zone = [zn == z for z in range(MAX_ZONES)]  # per zone id, the nodes of that zone
    zs = S.zset(zone)
    sk = np.asarray(max_skew, np.int64)
    c = np.zeros((G, MAX_ZONES), np.int64) if cnt is None else np.array(cnt, np.int64).reshape(G, MAX_ZONES)
    grp = S.clean_groups(group, G)
    open_nt = ~np.asarray(unsched, bool) if "NodeUnschedulable" in plugins.filters else np.ones(n, bool)
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    safe = np.where(alloc == 0, 1, alloc)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    lowest = np.iinfo(np.int64).min
    for j in range(p):
        pd, g = int(pod_digit[j]), int(grp[j])
        feas = (count < eff) if pod_tol[j] else (open_nt & (count < eff))
        for r in range(nres):
            if req[r, j] > 0:
                feas = feas & (req[r, j] <= alloc[r] - us[r])
        if g >= 0:
            # a node's skew after taking the pod, from its zone's count; a node without a zone never qualifies
            after = np.full(n, np.iinfo(np.int64).max)
            low = min((int(c[g, z]) for z in zs), default=0)
            for z in zs:
                after[in_zone[z]] = int(c[g, z]) + 1 - low
            feas = feas & (after <= sk[g])
        if not feas.any():
            status[j] = FIT_ERROR
            continue
        if plugins.score and not (nn_pre and 0 <= pd <= 9):
            status[j] = SCORE_ERROR
            continue
        total = np.zeros(n, np.int64)
        raw = np.where((nd == pd) & (nd >= 0), 10, 0).astype(np.int64)
        for w, nm in zip(plugins.weights, plugins.normalize):
            total = total + RS._nn_scores(int(nm), raw, feas) * int(w)
        acc = np.zeros(n, np.int64)
        for r in scored:
            q = us[r] + req[r, j]
            part = (alloc[r] - q) if mode == LEAST else q
            none = (alloc[r] == 0) | (q > alloc[r])
            acc += np.where(none, 0, np.where(none, 0, part) * 100 // safe[r]) * rw[r]
        total = total + (acc // den) * int(weight)
        sel = int(np.argmax(np.where(feas, total, lowest)))  # argmax returns the first maximum
        idx[j], score[j] = sel, total[sel]
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0:
            c[g, zn[sel]] += 1
    return idx, score, status, count.astype(np.int32), us, c.astype(np.int32)


def gen_case(seed: int, max_n: int = 2048, max_p: int = 2000) -> dict:
    """One case of the random sweep. Few digit classes and a small NodeNumber weight, so that many feasible nodes
    tie on NodeNumber and the resource score picks among them; zones of uneven size, small skews and mostly grouped
    pods, so that the zone the score prefers is often over skew. Tables of 1..2,048 nodes, 1..4 resources, 1..16
    groups, 1..8 zones with some nodes at -1, skews 1..3, resource weights with zeros."""
    rng = np.random.default_rng(seed)
    n = min(int(rng.choice([1, 7, 40, 65, 129, 300, 513, 1025, 2048])), max_n)
    p = min(int(rng.choice([301, 450, 777, 1203, 1999])), max_p)
    nres = int(rng.integers(1, 5))
    nz = int(rng.integers(1, 9))
    ids = rng.permutation(MAX_ZONES)[:nz]  # sparse ids in [0, 64)
    w = 1.0 / (1 + np.arange(nz)) ** 1.2   # uneven zones: the score prefers the large ones' many empty nodes
    zone = ids[rng.choice(nz, n, p=w / w.sum())].astype(np.int32)
    zone[rng.random(n) < 0.05] = -1
    G = int(rng.integers(1, 17))
    max_skew = rng.integers(1, 4, G).astype(np.int32)
    group = rng.integers(0, G, p).astype(np.int32)
    group[rng.random(p) < 0.15] = -1
    unit = int(rng.choice([1, 1000, 2**31, 2**40]))
    alloc = (rng.integers(20, 200, (nres, n)) * unit).astype(np.int64)
    alloc[rng.random((nres, n)) < 0.03] = 0
    req = (rng.integers(0, 4, (nres, p)) * unit).astype(np.int64)
    rw = rng.integers(0, 101, nres)
    rw[rng.random(nres) < 0.3] = 0
    rw[int(rng.integers(0, nres))] = int(rng.integers(1, 101))
    cap = rng.integers(0, max(3, 4 * p // max(n, 1)), n).astype(np.int32)
    digits = int(rng.choice([1, 2, 3]))
    return dict(
        seed=seed, n=n, p=p, nres=nres, G=G, score_mode=LEAST if seed % 2 else MOST,
        rs_weight=int(rng.choice([1, 2, 7, 2**32])), rw=[int(x) for x in rw],
        unsched=(rng.random(n) < 0.2).astype(np.uint8), node_digit=rng.integers(-1, digits, n).astype(np.int8),
        pod_digit=rng.integers(-1 if rng.random() < 0.2 else 0, digits, p).astype(np.int8),
        pod_tol=(rng.random(p) < 0.4).astype(np.uint8), zone=zone, group=group, max_skew=max_skew, alloc=alloc,
        req=req, cap=cap, mode=int(rng.integers(0, 4)), weight=int(rng.choice([1, 3, 2**32])))
