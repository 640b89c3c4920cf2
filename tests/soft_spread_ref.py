"""CPU references for sequential-commit mode with the soft topology spread score (include/minisched_hip.h, "Soft
topology spread": msh_schedule_sequential_soft). Neither is the code under test; test infrastructure only.

The contract, per pod j in order. A pod that is ungrouped or whose group's mode is DO_NOT_SCHEDULE is decided as
prefs_ref decides it. A pod of a SCHEDULE_ANYWAY group g passes no spread filter: its feasible set F is the one of an
ungrouped pod of its class. With Zs the zones of the zoned nodes in F and size = |Zs|:
    raw_z = round_half_away(float(cnt[g][z]) * log(size + 2) + float(max_skew[g] - 1))   for z in Zs
            (a product and a sum, each rounded once: two double operations)
    mx, mn = max, min of raw_z over Zs
    ns_i = 100 if mx == 0 else 100 * (mx + mn - raw_zone[i]) // mx   for i in F with a zone, 0 for i in F without one
    total_i = prefs_ref's total_i + w_spread * ns_i
and the first maximum in List order wins. A placed pod of a soft group adds 1 to cnt[g][zone[sel]] only if sel has a
zone.

1. `serial`: a plain Python loop over pods and nodes in Python ints and floats, math.log, rounding by floor and a
   comparison. Tiny shapes.
2. `per_pod`: written separately, one pod at a time with the nodes in numpy; the weights come from `weights`, and
   the rounding is numpy's rint with the ties it sends down put back up.

Arguments are prefs_ref.serial's up to w_taint, then (modes, w_spread): modes one 0 / 1 per group (None: all 0). Both
return (idx, score, status, counts after, used after, cnt after). With `trace` a list, every soft pod that reaches
scoring appends (j, size, mn, mx) (mn = mx = None with Zs empty). `gen_case` is the seeded generator of the GPU sweep;
tests/test_soft_spread.py checks on the references alone that it reaches what the sweep is for.
"""
from __future__ import annotations

import math

import numpy as np

import classes_ref as KR
import prefs_ref as PR
import resource_score_ref as RS
import spread_ref as S

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES
DO_NOT_SCHEDULE, SCHEDULE_ANYWAY = 0, 1
SOFT_MAX = 1 << 24

# log(size + 2) for size = 0..64. The library's table (msh_spread_soft_weight) is its own std::log;
# tests/test_soft_spread.py checks that the two agree bit for bit.
weights = [math.log(k + 2) for k in range(MAX_ZONES + 1)]


def round_half_away(y: float) -> int:
    """Go's math.Round for y >= 0: y - floor(y) is exact."""
    f = math.floor(y)
    return f + (1 if y - f >= 0.5 else 0)


def raw_score(c: int, size: int, skew: int) -> int:
    x = float(c) * math.log(size + 2)   # rounded once
    return round_half_away(x + float(skew - 1))   # and once more


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, counts=None, cnt=None,
           trace=None):
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
    md = [0] * G if modes is None else [int(x) for x in modes]
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
        soft = g >= 0 and md[g] == SCHEDULE_ANYWAY
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
            if g >= 0 and not soft:
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
        ns = {}
        if soft:
            z_feas = sorted({zn[i] for i in feas if zn[i] >= 0})
            rz = {z: raw_score(c[g][z], len(z_feas), sk[g]) for z in z_feas}
            mx, mn = (max(rz.values()), min(rz.values())) if rz else (None, None)
            for z in z_feas:
                ns[z] = 100 if mx == 0 else 100 * (mx + mn - rz[z]) // mx
            if trace is not None:
                trace.append((j, len(z_feas), mn, mx))
        for m, i in enumerate(feas):
            if mode != NONE:
                rs = RS.resource_score(mode, [al[r][i] for r in range(nres)], [us[r][i] + rq[r] for r in range(nres)], rw)
                total[m] += int(weight) * rs
            na = 0 if max_a == 0 else 100 * ra[m] // max_a
            nt = 100 if max_t == 0 else 100 - 100 * rt[m] // max_t
            total[m] = O._wrap64(total[m] + int(w_aff) * na + int(w_taint) * nt + int(w_spread) * ns.get(zn[i], 0))
        best = max(total)
        sel = feas[total.index(best)]  # the first maximum in List order
        idx[j], score[j] = sel, best
        count[sel] += 1
        for r in range(nres):
            us[r][sel] += rq[r]
        if g >= 0 and zn[sel] >= 0:
            c[g][zn[sel]] += 1
    return (idx, score, status, np.array(count, np.int32), np.array(us, np.int64).reshape(nres, n),
            np.array(c, np.int32).reshape(G, MAX_ZONES))


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, counts=None, cnt=None,
            trace=None):
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
    zoned = zn >= 0
    zsafe = np.where(zoned, zn, 0)
    sk = np.asarray(max_skew, np.int64)
    md = np.zeros(G, np.int64) if modes is None else np.asarray(modes, np.int64)
    c = np.zeros((G, MAX_ZONES), np.int64) if cnt is None else np.array(cnt, np.int64).reshape(G, MAX_ZONES)
    grp = np.full(p, -1, np.int64) if group is None else np.asarray(group, np.int64)
    cls = np.full(p, -1, np.int64) if pod_class is None else np.asarray(pod_class, np.int64)
    word = None if bits is None else np.asarray(bits, np.uint64)
    Aq = np.zeros((max(n_classes, 1), n), np.int64) if A is None else np.asarray(A, np.int64).reshape(-1, n)
    Tq = np.zeros((max(n_classes, 1), n), np.int64) if T is None else np.asarray(T, np.int64).reshape(-1, n)
    blocked = np.asarray(unsched, bool) if "NodeUnschedulable" in plugins.filters else np.zeros(n, bool)
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    wt = np.array(weights, np.float64)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    lowest = np.iinfo(np.int64).min
    zeros = np.zeros(n, np.int64)
    for j in range(p):
        pd = int(pod_digit[j])
        g = int(grp[j]) if 0 <= grp[j] < G else -1
        k = int(cls[j]) if 0 <= cls[j] < n_classes else -1
        soft = g >= 0 and md[g] == SCHEDULE_ANYWAY
        feas = count < eff
        if not pod_tol[j]:
            feas = feas & ~blocked
        if k >= 0 and word is not None:
            feas = feas & ((word >> np.uint64(k)) & np.uint64(1)).astype(bool)
        for r in range(nres):
            if req[r, j] > 0:
                feas = feas & (alloc[r] - us[r] >= req[r, j])
        if g >= 0 and not soft:
            if len(zs) == 0:
                feas = np.zeros(n, bool)
            else:
                feas = feas & zoned & (c[g][zsafe] - c[g][zs].min() < sk[g])
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
        na = zeros if max_a == 0 else ra * 100 // max_a
        nt = zeros + 100 if max_t == 0 else 100 - rt * 100 // max_t
        total = total + np.int64(int(w_aff)) * na + np.int64(int(w_taint)) * nt
        if soft:
            in_zs = np.zeros(MAX_ZONES, bool)
            in_zs[zn[feas & zoned]] = True
            size = int(in_zs.sum())
            mn = mx = None
            if size:
                y = c[g].astype(np.float64) * wt[size]   # one rounding
                y = y + np.float64(int(sk[g]) - 1)       # and another
                r = np.rint(y)                           # ties to even ...
                r = r + ((y - np.floor(y) == 0.5) & (r < y))   # ... the ones sent down go up: half away from zero
                rz = r.astype(np.int64)
                mx, mn = int(rz[in_zs].max()), int(rz[in_zs].min())
                nz = np.full(MAX_ZONES, 100, np.int64) if mx == 0 else 100 * (mx + mn - rz) // max(mx, 1)
                total = total + np.int64(int(w_spread)) * np.where(zoned, nz[zsafe], 0)
            if trace is not None:
                trace.append((j, size, mn, mx))
        sel = int(np.argmax(np.where(feas, total, lowest)))  # argmax returns the first maximum
        idx[j], score[j] = sel, total[sel]
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0 and zn[sel] >= 0:
            c[g, zn[sel]] += 1
    return idx, score, status, count.astype(np.int32), us, c.astype(np.int32)


def gen_case(seed: int, max_n: int = 700, max_p: int = 300) -> dict:
    """One case of the random sweep: prefs_ref.gen_case's table, groups, amounts, plugins, classes and preference
    values (its resource score mode by seed: NONE every third, else LEAST / MOST by parity), about half of the groups
    SCHEDULE_ANYWAY, skews 1..3 (1: the first pod of a group sees mx == 0; above 1: mn > 0), a spread weight in
    [1, 100] and the resource weight lowered so that the key holds the sum. By seed % 5:
      0: most nodes lose their zone and the zoned ones take one pod each, so that Zs runs empty mid-call and soft pods
         land on nodes without a zone;
      1: every group is soft;  2: pods of three kinds only in a table of 8 zones whose small zones fill (size < |Zset|);
      others: as drawn."""
    c = PR.gen_case(seed, max_n, max_p)
    rng = np.random.default_rng(3 * 10**6 + seed)
    n, G = c["n"], c["G"]
    modes = (rng.random(G) < 0.5).astype(np.uint8)
    kind = seed % 5
    zone = np.array(c["zone"], np.int32)
    cap = np.array(c["cap"], np.int64)
    if kind == 0:
        zone[rng.random(n) < 0.7] = -1
        cap[zone >= 0] = 1
        modes[0] = 1
    elif kind == 1:
        modes[:] = 1
    elif kind == 2:
        zone = rng.choice(8, n, p=np.array([40, 30, 15, 8, 3, 2, 1, 1]) / 100).astype(np.int32)
        cap[:] = 1
        modes[: max(1, G // 2)] = 1
    w_spread = int(rng.integers(1, 101))
    c["rs_weight"] = int(min(int(c["rs_weight"]), 655 - c["w_aff"] - c["w_taint"] - w_spread))
    c.update(zone=zone, cap=cap, modes=modes, w_spread=w_spread)
    return c
