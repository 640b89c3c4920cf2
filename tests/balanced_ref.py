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

1. `serial`: soft_spread_ref.serial's loop plus the term, in Python ints and floats. Tiny shapes.
2. `per_pod`: soft_spread_ref.per_pod's loop plus the term, the nodes in numpy (astype(float64) rounds to nearest even,
   `/`, `-` and `*` on float64 arrays are single IEEE operations, astype(int64) truncates).

Arguments are soft_spread_ref.serial's up to w_spread, then w_balanced. `bs_exact`, `bs_f32` and `bs_rounded` are the
three evaluations the rule is not: tests/test_balanced.py searches for the inputs on which each differs from `bs`, the
decider triples that the GPU tests place on nodes. `gen_case` is the seeded generator of the GPU sweep.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import classes_ref as KR
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
    n, p = len(unsched), len(pod_digit)
    assert n * p <= 2 * 10**5, "the serial loop is for tiny shapes"
    nres, G = len(alloc), len(max_skew)
    assert not w_balanced or nres >= 2
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
            rz = {z: SR.raw_score(c[g][z], len(z_feas), sk[g]) for z in z_feas}
            mx, mn = (max(rz.values()), min(rz.values())) if rz else (None, None)
            for z in z_feas:
                ns[z] = 100 if mx == 0 else 100 * (mx + mn - rz[z]) // mx
        bal = [0] * len(feas)
        for m, i in enumerate(feas):
            if mode != NONE:
                rs = RS.resource_score(mode, [al[r][i] for r in range(nres)], [us[r][i] + rq[r] for r in range(nres)], rw)
                total[m] += int(weight) * rs
            na = 0 if max_a == 0 else 100 * ra[m] // max_a
            nt = 100 if max_t == 0 else 100 - 100 * rt[m] // max_t
            if w_balanced:
                bal[m] = bs(us[0][i] + rq[0], al[0][i], us[1][i] + rq[1], al[1][i])
            total[m] = O._wrap64(total[m] + int(w_aff) * na + int(w_taint) * nt + int(w_spread) * ns.get(zn[i], 0)
                                 + int(w_balanced) * bal[m])
        best = max(total)
        at = total.index(best)  # the first maximum in List order
        sel = feas[at]
        idx[j], score[j] = sel, best
        if moved is not None:
            moved.append((j, sel, bal[at]))
        count[sel] += 1
        for r in range(nres):
            us[r][sel] += rq[r]
        if g >= 0 and zn[sel] >= 0:
            c[g][zn[sel]] += 1
    return (idx, score, status, np.array(count, np.int32), np.array(us, np.int64).reshape(nres, n),
            np.array(c, np.int32).reshape(G, MAX_ZONES))


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, w_balanced,
            counts=None, cnt=None):
    n, p = len(unsched), len(pod_digit)
    alloc = np.asarray(alloc, np.int64).reshape(-1, n)
    us = np.array(used, np.int64).reshape(-1, n)
    req = np.asarray(req, np.int64).reshape(-1, p)
    nres, G = alloc.shape[0], len(max_skew)
    assert not w_balanced or nres >= 2
    if mode != NONE or w_balanced:
        assert max(alloc.max(initial=0), us.max(initial=0), req.max(initial=0)) <= SCORE_MAX
    if mode != NONE:
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
    wt = np.array(SR.weights, np.float64)
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
            if size:
                y = c[g].astype(np.float64) * wt[size]   # one rounding
                y = y + np.float64(int(sk[g]) - 1)       # and another
                r = np.rint(y)                           # ties to even ...
                r = r + ((y - np.floor(y) == 0.5) & (r < y))   # ... the ones sent down go up: half away from zero
                rz = r.astype(np.int64)
                mx, mn = int(rz[in_zs].max()), int(rz[in_zs].min())
                nz = np.full(MAX_ZONES, 100, np.int64) if mx == 0 else 100 * (mx + mn - rz) // max(mx, 1)
                total = total + np.int64(int(w_spread)) * np.where(zoned, nz[zsafe], 0)
        if w_balanced:
            total = total + np.int64(int(w_balanced)) * bs_nodes(alloc, us, req[:, j])
        sel = int(np.argmax(np.where(feas, total, lowest)))  # argmax returns the first maximum
        idx[j], score[j] = sel, total[sel]
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0 and zn[sel] >= 0:
            c[g, zn[sel]] += 1
    return idx, score, status, count.astype(np.int32), us, c.astype(np.int32)


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
