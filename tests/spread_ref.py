"""CPU references for sequential-commit mode with pod topology spread (include/minisched_hip.h, "Pod topology
spread for sequential-commit mode"). None of them is the code under test; test infrastructure only.

The contract, per pod j in order, with group g = group[j] (anything outside [0, G) counts as -1): node i is
feasible iff the filter list passes, count[i] < eff[i], every positive request fits alloc - used, and, for g >= 0,
zone[i] >= 0 and cnt[g][zone[i]] + 1 - min over z in Zset of cnt[g][z] <= max_skew[g]. Zset is the set of zone ids
on at least one node. Status, NodeNumber totals in every normalize mode, the first maximum and the commit are the
resource-fit form's; a PLACED grouped pod also adds 1 to cnt[g][zone[sel]].

1. `serial`: a plain Python loop that looks at every (pod, node) pair and reads cnt[g][zone[i]] for every node.
   For tiny shapes (p * n <= 2 * 10^5).
2. `per_pod`: one pod at a time with the nodes in numpy (the skew of every node gathered from the cnt array); the
   totals of the two NodeNumber classes come from oracle.normalize over the raw scores present, as in
   resource_fit_ref.per_pod. tests/test_spread.py shows it equal to `serial` before anything relies on it.

Neither forms a per-zone "allowed" set: each node's verdict is computed from the cnt array directly. alloc / used
are shaped (nres, n) and req (nres, p), with nres = 0 for a call without requests. `gen_case` is the seeded
generator of the random sweeps, shared by the CPU and GPU tests.
"""
from __future__ import annotations

import numpy as np

INT32_MAX = 2**31 - 1
NO_LIMIT = INT32_MAX
MAX_ZONES = 64
PLACED, FIT_ERROR, SCORE_ERROR = 0, 1, 2


def no_limit(n: int) -> np.ndarray:
    return np.full(n, NO_LIMIT, np.int64)


def no_res(n: int, p: int):
    """alloc, used, req of a call without requests."""
    return np.zeros((0, n), np.int64), np.zeros((0, n), np.int64), np.zeros((0, p), np.int64)


def zset(zone) -> list[int]:
    return sorted({int(z) for z in zone if int(z) >= 0})


def clean_groups(group, G: int) -> np.ndarray:
    g = np.asarray(group, np.int64)
    return np.where((g >= 0) & (g < G), g, -1)


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           counts=None, cnt=None):
    """(idx, score, status, counts after, used after, cnt after); cnt shaped (G, MAX_ZONES)."""
    n, p = len(unsched), len(pod_digit)
    assert n * p <= 2 * 10**5, "the serial loop is for tiny shapes"
    nres, G = len(alloc), len(max_skew)
    eff = [int(x) for x in eff]
    count = [0] * n if counts is None else [int(x) for x in counts]
    al = [[int(x) for x in row] for row in alloc]
    us = [[int(x) for x in row] for row in used]
    zn = [int(z) for z in zone]
    zs = zset(zone)
    sk = [int(x) for x in max_skew]
    c = [[0] * MAX_ZONES for _ in range(G)] if cnt is None else [[int(x) for x in row] for row in cnt]
    grp = clean_groups(group, G)
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
        for w, mode in zip(plugins.weights, plugins.normalize):
            raw = [10 if 0 <= int(node_digit[i]) == pd else 0 for i in feas]
            total = [O._wrap64(t + s * int(w)) for t, s in zip(total, O.normalize(int(mode), raw))]
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
            counts=None, cnt=None):
    """(idx, score, status, counts after, used after, cnt after): per pod one numpy pass over the nodes."""
    n, p = len(unsched), len(pod_digit)
    alloc = np.asarray(alloc, np.int64).reshape(-1, n)
    us = np.array(used, np.int64).reshape(-1, n)
    req = np.asarray(req, np.int64).reshape(-1, p)
    nres, G = alloc.shape[0], len(max_skew)
    eff = np.asarray(eff, np.int64)
    count = np.zeros(n, np.int64) if counts is None else np.array(counts, np.int64)
    nd = np.asarray(node_digit, np.int64)
    zn = np.asarray(zone, np.int64)
    zoned = zn >= 0
    zsafe = np.where(zoned, zn, 0)
    zs = np.array(zset(zone), np.int64)
    sk = np.asarray(max_skew, np.int64)
    c = np.zeros((G, MAX_ZONES), np.int64) if cnt is None else np.array(cnt, np.int64).reshape(G, MAX_ZONES)
    grp = clean_groups(group, G)
    has_nu = "NodeUnschedulable" in plugins.filters
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    open_all = np.ones(n, bool)
    open_nt = ~np.asarray(unsched, bool) if has_nu else open_all
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)

    def class_totals(raws):  # totals of the raw scores present among the feasible nodes, by raw score
        total = {r: 0 for r in raws}
        for w, mode in zip(plugins.weights, plugins.normalize):
            for r, s in zip(raws, O.normalize(int(mode), list(raws))):
                total[r] = O._wrap64(total[r] + s * int(w))
        return total

    for j in range(p):
        pd, g = int(pod_digit[j]), int(grp[j])
        feas = (open_all if pod_tol[j] else open_nt) & (count < eff)
        for r in range(nres):
            if req[r, j] > 0:
                feas = feas & (req[r, j] <= alloc[r] - us[r])
        if g >= 0:
            if len(zs) == 0:
                feas = np.zeros(n, bool)
            else:
                feas = feas & zoned & (c[g][zsafe] + 1 - c[g][zs].min() <= sk[g])
        if not feas.any():
            status[j] = FIT_ERROR
            continue
        if plugins.score and not (nn_pre and 0 <= pd <= 9):
            status[j] = SCORE_ERROR
            continue
        match = feas & (nd == pd) & (nd >= 0)
        other = feas & ~match
        fm = int(np.argmax(match)) if match.any() else -1
        fx = int(np.argmax(other)) if other.any() else -1
        raws = ([10] if fm >= 0 else []) + ([0] if fx >= 0 else [])
        total = class_totals(raws)
        if fm >= 0 and fx >= 0:
            if total[10] == total[0]:
                sel, best = min(fm, fx), total[10]
            else:
                sel, best = (fm, total[10]) if total[10] > total[0] else (fx, total[0])
        else:
            sel, best = (fm, total[10]) if fm >= 0 else (fx, total[0])
        idx[j], score[j] = sel, best
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0:
            c[g, zn[sel]] += 1
    return idx, score, status, count.astype(np.int32), us, c.astype(np.int32)


def gen_case(seed: int, max_n: int = 2048, max_p: int = 2000) -> dict:
    """One case of the random sweep: a table whose zones are few next to its groups' demand, per-node pod limits
    that let single zones fill, and mostly grouped pods with small skews, so that the spread conjunct decides."""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([7, 40, 65, 300, 513, 700, max_n]))
    n = min(n, max_n)
    p = min(int(rng.choice([30, 129, 400, 900, max_p])), max_p)
    nz = int(rng.choice([1, 2, 3, 5, 8, 64]))
    ids = rng.permutation(MAX_ZONES)[:nz]  # sparse ids in [0, 64)
    # zone sizes are uneven: the first zones hold most nodes, so small zones fill while large ones have room
    w = 1.0 / (1 + np.arange(nz)) ** 1.5
    zone = ids[rng.choice(nz, n, p=w / w.sum())].astype(np.int32)
    zone[rng.random(n) < 0.05] = -1
    G = int(rng.choice([1, 2, 16, 128]))
    max_skew = rng.choice([1, 1, 2, 5, INT32_MAX], G).astype(np.int32)
    group = rng.integers(0, G, p).astype(np.int32)
    group[rng.random(p) < 0.15] = -1
    nres = int(rng.integers(0, 5))
    alloc = (rng.integers(0, 9, (nres, n)) * 1000).astype(np.int64)
    req = (rng.integers(0, 3, (nres, p)) * 500).astype(np.int64)
    cap = rng.integers(0, max(2, 3 * p // max(n, 1)), n).astype(np.int32)
    mode = int(rng.integers(0, 4))
    weight = int(rng.choice([1, 3, 2**32]))
    return dict(
        seed=seed, n=n, p=p, nres=nres, G=G,
        unsched=(rng.random(n) < 0.2).astype(np.uint8), node_digit=rng.integers(-1, 10, n).astype(np.int8),
        pod_digit=rng.integers(-1 if rng.random() < 0.3 else 0, 10, p).astype(np.int8),
        pod_tol=(rng.random(p) < 0.4).astype(np.uint8), zone=zone, group=group, max_skew=max_skew, alloc=alloc,
        req=req, cap=cap, mode=mode, weight=weight)
