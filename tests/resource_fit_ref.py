"""CPU references for sequential-commit mode with resource requests (include/minisched_hip.h, "Resource
requests for sequential-commit mode"). None of them is the code under test; test infrastructure only.

1. `serial`: node_capacity_ref.serial with the extra conjunct (for every r with req[r][j] > 0:
   req[r][j] <= alloc[r][i] - used[r][i]) and the update of `used` at a commit. A plain Python loop that looks at
   every (pod, node) pair, for tiny shapes (p * n <= 2 * 10^5).
2. `via_oracle`: the identity that ties the feature to the unchanged C oracle. With ONE resource, every request 1,
   alloc = c and used = k0 at the start of the run, node i passes the resource conjunct while
       1 <= c[i] - used[i],  used[i] = k0[i] + (count[i] - count0[i])
   (every commit of the run adds one pod and one unit, count0 the counts at the start), that is while
       count[i] < c[i] - k0[i] + count0[i].
   Together with count[i] < eff[i] the node is feasible while count[i] < min(eff[i], c[i] - k0[i] + count0[i]): a
   second pod capacity. A negative bound (alloc patched below used) never admits a pod, as a bound of 0 does not
   (count >= 0), so it is clamped to 0. The run therefore equals node_capacity_ref.via_oracle with
       eff' = min(eff, max(c - k0 + count0, 0)),
   and used afterwards is k0 + (counts after - count0). With every request 0 the conjunct is empty: the run
   equals the plain capacity run with eff, and used does not change.
3. `per_pod`: one pod at a time, the nodes in numpy, for mid sizes. A node's total depends only on whether its
   digit matches the pod's, so the two classes' totals come from oracle.normalize over the raw scores present
   ([10, 0], [10] or [0]) and the pick is the first feasible node of the better class (the first feasible node
   at a tie). tests/test_resource_fit.py shows it equal to `serial` on tiny cases before anything relies on it.

`eff` is node_capacity_ref.effective(cap, scalar), or NO_LIMIT everywhere for a call with neither a scalar nor a
capacity column.
"""
from __future__ import annotations

import numpy as np

import node_capacity_ref as C

INT32_MAX = C.INT32_MAX
NO_LIMIT = INT32_MAX
PLACED, FIT_ERROR, SCORE_ERROR = C.PLACED, C.FIT_ERROR, C.SCORE_ERROR


def no_limit(n: int) -> np.ndarray:
    return np.full(n, NO_LIMIT, np.int64)


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, counts=None):
    """(idx, score, status, counts after, used after); alloc / used shaped (nres, n), req (nres, p)."""
    n, p = len(unsched), len(pod_digit)
    assert n * p <= 2 * 10**5, "the serial loop is for tiny shapes"
    nres = len(alloc)
    eff = [int(x) for x in eff]
    cnt = [0] * n if counts is None else [int(x) for x in counts]
    al = [[int(x) for x in row] for row in alloc]
    us = [[int(x) for x in row] for row in used]
    has_nu = "NodeUnschedulable" in plugins.filters
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    for j in range(p):
        pd, tol = int(pod_digit[j]), bool(pod_tol[j])
        rq = [int(req[r][j]) for r in range(nres)]
        feas = [i for i in range(n)
                if (not has_nu or not unsched[i] or tol) and cnt[i] < eff[i]
                and all(rq[r] <= al[r][i] - us[r][i] for r in range(nres) if rq[r] > 0)]
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
        cnt[sel] += 1
        for r in range(nres):
            us[r][sel] += rq[r]
    return idx, score, status, np.array(cnt, np.int32), np.array(us, np.int64).reshape(nres, n)


def via_oracle(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, counts=None):
    """(idx, score, status, counts after, used after) through the second-capacity identity (module docstring):
    one resource, and every request 1 or every request 0."""
    alloc, used, req = (np.asarray(a, np.int64) for a in (alloc, used, req))
    assert alloc.shape[0] == used.shape[0] == req.shape[0] == 1, "the identity is for one resource"
    n = len(unsched)
    eff = np.asarray(eff, np.int64)
    k = np.zeros(n, np.int64) if counts is None else np.asarray(counts, np.int64)
    # a run of p pods never brings count[i] to k[i] + p + 1: a limit there or above (NO_LIMIT) is that one, which
    # keeps the oracle's shifted counts within int32
    eff = np.minimum(eff, k + len(pod_digit) + 1)
    if (req == 0).all():
        idx, score, status, after = C.via_oracle(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, k)
        return idx, score, status, after, used.copy()
    assert (req == 1).all(), "the identity is for unit requests"
    bound = np.maximum(alloc[0] - used[0] + k, 0)
    eff2 = np.minimum(eff, bound)
    idx, score, status, after = C.via_oracle(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff2, k)
    return idx, score, status, after, (used[0] + (after.astype(np.int64) - k)).reshape(1, n)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, counts=None):
    """(idx, score, status, counts after, used after): per pod one numpy pass over the nodes (module docstring)."""
    n, p = len(unsched), len(pod_digit)
    alloc = np.asarray(alloc, np.int64)
    us = np.array(used, np.int64)
    req = np.asarray(req, np.int64)
    nres = alloc.shape[0]
    eff = np.asarray(eff, np.int64)
    cnt = np.zeros(n, np.int64) if counts is None else np.array(counts, np.int64)
    nd = np.asarray(node_digit, np.int64)
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
        pd = int(pod_digit[j])
        feas = (open_all if pod_tol[j] else open_nt) & (cnt < eff)
        for r in range(nres):
            if req[r, j] > 0:
                feas = feas & (req[r, j] <= alloc[r] - us[r])
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
        cnt[sel] += 1
        us[:, sel] += req[:, j]
    return idx, score, status, cnt.astype(np.int32), us
