"""CPU references for resource-aware scoring in sequential-commit mode (include/minisched_hip.h, "Resource-aware
scoring": msh_set_resource_score with LEAST_ALLOCATED / MOST_ALLOCATED). Neither is the code under test; test
infrastructure only.

1. `serial`: the literal loop. Per pod the feasible list as resource_fit_ref.serial builds it, per feasible node
   the total from the header's formulas in Python ints (NodeNumber through oracle.normalize over the feasible list,
   plus weight x RS), the first maximum, the commit. Tiny shapes.
2. `per_pod`: written separately, in numpy int64: a feasibility mask, NodeNumber's normalizers spelled out on
   arrays, RS for every node at once, one argmax per pod. Mid sizes.
tests/test_resource_score.py checks the two against each other and mode NONE against resource_fit_ref.serial.

Modes: NONE = 0, LEAST = 1, MOST = 2 (msh_resource_score). `rw`: one weight per resource, 0 = not scored.
"""
from __future__ import annotations

import numpy as np

import resource_fit_ref as R

NONE, LEAST, MOST = 0, 1, 2
SCORE_MAX = 1 << 55  # MSH_RESOURCE_SCORE_MAX
PLACED, FIT_ERROR, SCORE_ERROR = R.PLACED, R.FIT_ERROR, R.SCORE_ERROR


def resource_score(mode, c, q, rw):
    """RS for one (pod, node): c[r] allocatable, q[r] = used + request, Python ints."""
    num = den = 0
    for cr, qr, w in zip(c, q, rw):
        if w <= 0:
            continue
        if cr == 0 or qr > cr:
            s = 0
        elif mode == LEAST:
            s = ((cr - qr) * 100) // cr
        else:
            s = (qr * 100) // cr
        num += s * w
        den += w
    return num // den


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, mode, weight, rw, counts=None):
    """(idx, score, status, counts after, used after); alloc / used shaped (nres, n), req (nres, p)."""
    if mode == NONE:
        return R.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, counts)
    n, p = len(unsched), len(pod_digit)
    assert n * p <= 2 * 10**5, "the serial loop is for tiny shapes"
    nres = len(alloc)
    eff = [int(x) for x in eff]
    cnt = [0] * n if counts is None else [int(x) for x in counts]
    al = [[int(x) for x in row] for row in alloc]
    us = [[int(x) for x in row] for row in used]
    rw = [int(x) for x in rw]
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
        if plugins.score and not (nn_pre and 0 <= pd <= 9):
            status[j] = SCORE_ERROR
            continue
        total = [0] * len(feas)
        for w, nm in zip(plugins.weights, plugins.normalize):
            raw = [10 if 0 <= int(node_digit[i]) == pd else 0 for i in feas]
            total = [O._wrap64(t + s * int(w)) for t, s in zip(total, O.normalize(int(nm), raw))]
        for k, i in enumerate(feas):
            rs = resource_score(mode, [al[r][i] for r in range(nres)], [us[r][i] + rq[r] for r in range(nres)], rw)
            total[k] = O._wrap64(total[k] + int(weight) * rs)
        best = max(total)
        sel = feas[total.index(best)]  # the first maximum in List order
        idx[j], score[j] = sel, best
        cnt[sel] += 1
        for r in range(nres):
            us[r][sel] += rq[r]
    return idx, score, status, np.array(cnt, np.int32), np.array(us, np.int64).reshape(nres, n)


def _nn_scores(nm, raw, feas):
    """NodeNumber's normalized scores over the feasible nodes as an int64 array (entries off `feas` unspecified)."""
    f = raw[feas]
    if nm == 1 or nm == 2:  # DefaultNormalizeScore, plain and reverse
        mx = int(f.max())
        if mx == 0:
            return np.full_like(raw, 100) if nm == 2 else raw
        s = raw * 100 // mx
        return 100 - s if nm == 2 else s
    if nm == 3:  # min-max over the feasible list
        lo, hi = int(f.min()), int(f.max())
        return np.zeros_like(raw) if hi == lo else (raw - lo) * 100 // (hi - lo)
    return raw


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, mode, weight, rw, counts=None):
    """(idx, score, status, counts after, used after): per pod one numpy pass over the nodes, int64 throughout."""
    if mode == NONE:
        return R.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, counts)
    n, p = len(unsched), len(pod_digit)
    alloc = np.asarray(alloc, np.int64)
    us = np.array(used, np.int64)
    req = np.asarray(req, np.int64)
    assert max(alloc.max(initial=0), us.max(initial=0), req.max(initial=0)) <= SCORE_MAX, "int64 would overflow"
    nres = alloc.shape[0]
    rw = np.asarray(rw, np.int64)
    scored = [r for r in range(nres) if rw[r] > 0]
    den = int(rw[scored].sum())
    eff = np.asarray(eff, np.int64)
    cnt = np.zeros(n, np.int64) if counts is None else np.array(counts, np.int64)
    nd = np.asarray(node_digit, np.int64)
    open_nt = ~np.asarray(unsched, bool) if "NodeUnschedulable" in plugins.filters else np.ones(n, bool)
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    safe = np.where(alloc == 0, 1, alloc)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    lowest = np.iinfo(np.int64).min
    for j in range(p):
        pd = int(pod_digit[j])
        feas = (cnt < eff) if pod_tol[j] else (open_nt & (cnt < eff))
        for r in range(nres):
            if req[r, j] > 0:
                feas = feas & (req[r, j] <= alloc[r] - us[r])
        if not feas.any():
            status[j] = FIT_ERROR
            continue
        if plugins.score and not (nn_pre and 0 <= pd <= 9):
            status[j] = SCORE_ERROR
            continue
        total = np.zeros(n, np.int64)
        raw = np.where((nd == pd) & (nd >= 0), 10, 0).astype(np.int64)
        for w, nm in zip(plugins.weights, plugins.normalize):
            total = total + _nn_scores(int(nm), raw, feas) * int(w)
        acc = np.zeros(n, np.int64)
        for r in scored:
            q = us[r] + req[r, j]
            part = (alloc[r] - q) if mode == LEAST else q
            none = (alloc[r] == 0) | (q > alloc[r])
            s = np.where(none, 0, np.where(none, 0, part) * 100 // safe[r])
            acc += s * rw[r]
        total = total + (acc // den) * int(weight)
        sel = int(np.argmax(np.where(feas, total, lowest)))  # argmax returns the first maximum
        idx[j], score[j] = sel, total[sel]
        cnt[sel] += 1
        us[:, sel] += req[:, j]
    return idx, score, status, cnt.astype(np.int32), us


def sweep_case(O, rng, case, sizes):
    """One draw of the random sweep: few digit classes against the nodes and requests small against alloc, so that
    many nodes tie on NodeNumber and the resource score decides. Returns a dict of the inputs."""
    nres = 1 + case % 4
    n = int(rng.choice(sizes))
    p = int(rng.choice([17, 64, 65, 130]))
    mode = LEAST if case % 2 else MOST
    nm, w = [(m, w) for m in (0, 1, 2, 3) for w in (1, 3, 2**32)][case % 12]
    filters = ["NodeUnschedulable"] if rng.random() < 0.7 else []
    kind = rng.random()
    if kind < 0.08:
        plugins = O.PluginSet(filters, ["NodeNumber"], [], [], [])  # NodeNumber absent: the resource score alone
    elif kind < 0.14:
        plugins = O.PluginSet(filters, [], ["NodeNumber"], [w], [nm])  # no PreScore state: score errors
    else:
        plugins = O.PluginSet(filters, ["NodeNumber"], ["NodeNumber"], [w], [nm])
    digits = int(rng.choice([1, 2, 3]))
    u = (rng.random(n) < float(rng.choice([0.0, 0.3]))).astype(np.uint8)
    nd = rng.integers(-1, digits, n).astype(np.int8)
    pd = rng.integers(-1 if rng.random() < 0.3 else 0, digits, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    unit = int(rng.choice([1, 1000, 2**31, 2**40]))
    alloc = (rng.integers(20, 200, (nres, n)) * unit).astype(np.int64)
    alloc[rng.random((nres, n)) < 0.03] = 0
    used = (rng.integers(0, 10, (nres, n)) * unit).astype(np.int64)
    req = (rng.integers(0, 4, (nres, p)) * unit).astype(np.int64)
    rw = rng.integers(0, 101, nres)
    rw[int(rng.integers(0, nres))] = int(rng.integers(1, 101))
    weight = int(rng.choice([1, 2, 7, 2**32]))
    cap = rng.integers(0, 6, n) if case % 5 == 0 else None
    scalar = int(rng.choice([0, 0, 3]))
    return dict(nres=nres, n=n, p=p, mode=mode, plugins=plugins, u=u, nd=nd, pd=pd, pt=pt, alloc=alloc, used=used,
                req=req, rw=[int(x) for x in rw], weight=weight, cap=cap, scalar=scalar)
