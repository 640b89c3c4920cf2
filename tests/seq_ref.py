"""The one scheduling step of sequential-commit mode, written twice: the CPU references behind every `*_ref.py` layer
from resource_score_ref to podaffinity_ref. Neither is the code under test; test infrastructure only.

The contract is msh_schedule_sequential_podaffinity's (include/minisched_hip.h), the superset of every grouped
sequential-commit form; the layer modules state their own part of it (the formulae) and delegate here with the later
features left at their defaults. Per pod j in order: the feasible set (filter list, count < eff, every positive
request fits, the class bit, a hard group's zone skew over Zset, the inter-pod conjunct), FIT_ERROR if it is empty,
SCORE_ERROR if NodeNumber scores without its PreScore state, else per feasible node
    total = NodeNumber normalized over the feasible list x its weights + weight * RS + w_aff * na + w_taint * nt
            + w_spread * ns + w_balanced * BS
the first maximum in List order, and the commit (count, used, a grouped pod's zone count, the inter-pod words).

1. `serial`: a plain Python loop over pods and nodes in Python ints and floats, on the scalar helpers (O.normalize,
   O._wrap64, RS.resource_score, SR.raw_score, BR.bs, KR.clean_classes). Tiny shapes (p * n <= 2 * 10^5). It has no
   inter-pod conjunct.
2. `per_pod`: written separately, one pod at a time with the nodes in numpy int64, on the array helpers
   (RS._nn_scores, SR.weights with rint and the tie repair, BR.bs_nodes, PA.conjunct).
Neither calls the other, forms an availability mask per zone, packs (score, node) into a key, prefetches or keeps a
running maximum; that the two agree is what the "per_pod equals serial" tests of the layers and tests/test_seq_ref.py
check.

Arguments after req may be given by keyword; every default means that the feature is absent: zone None (no node has a
zone), group None (no pod a group), max_skew () (no group), mode NONE, bits None (every node admits every class),
pod_class None (no pod a class), A / T None (zeros), modes None (every group DO_NOT_SCHEDULE), state / pod_profile None
(no pod a profile). alloc / used are shaped (nres, n) and req (nres, p), nres = 0 for a call without requests. Both
return (idx, score, status, counts after, used after, cnt after), cnt shaped (G, MAX_ZONES).

Observation hooks, each a list that is appended to: `prefs_trace` gets (class, maxA, maxT) for every pod that reaches
scoring; `soft_trace` gets (j, size, mn, mx) for every pod of a SCHEDULE_ANYWAY group that reaches scoring (mn = mx =
None with Zs empty); `moved` (serial) gets (j, node, BS of that node) for every placed pod; the inter-pod reasons are
counted into state.stats by PA.conjunct.
"""
from __future__ import annotations

import numpy as np

import balanced_ref as BR
import classes_ref as KR
import podaffinity_ref as PA
import resource_score_ref as RS
import soft_spread_ref as SR
import spread_ref as S

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES
SCHEDULE_ANYWAY = SR.SCHEDULE_ANYWAY
SCORE_MAX = BR.SCORE_MAX


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone=None, group=None,
           max_skew=(), mode=NONE, weight=0, rw=(), bits=None, n_classes=0, pod_class=None, A=None, T=None, w_aff=0,
           w_taint=0, modes=None, w_spread=0, w_balanced=0, state=None, pod_profile=None, counts=None, cnt=None,
           prefs_trace=None, soft_trace=None, moved=None):
    assert state is None and pod_profile is None, "the serial loop has no inter-pod conjunct"
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
        if prefs_trace is not None:
            prefs_trace.append((k, max_a, max_t))
        ns = {}
        if soft:
            z_feas = sorted({zn[i] for i in feas if zn[i] >= 0})
            rz = {z: SR.raw_score(c[g][z], len(z_feas), sk[g]) for z in z_feas}
            mx, mn = (max(rz.values()), min(rz.values())) if rz else (None, None)
            for z in z_feas:
                ns[z] = 100 if mx == 0 else 100 * (mx + mn - rz[z]) // mx
            if soft_trace is not None:
                soft_trace.append((j, len(z_feas), mn, mx))
        bal = [0] * len(feas)
        for m, i in enumerate(feas):
            if mode != NONE:
                rs = RS.resource_score(mode, [al[r][i] for r in range(nres)], [us[r][i] + rq[r] for r in range(nres)], rw)
                total[m] += int(weight) * rs
            na = 0 if max_a == 0 else 100 * ra[m] // max_a
            nt = 100 if max_t == 0 else 100 - 100 * rt[m] // max_t
            if w_balanced:
                bal[m] = BR.bs(us[0][i] + rq[0], al[0][i], us[1][i] + rq[1], al[1][i])
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
        if g >= 0 and zn[sel] >= 0:  # a hard group's pod always lands in a zone
            c[g][zn[sel]] += 1
    return (idx, score, status, np.array(count, np.int32), np.array(us, np.int64).reshape(nres, n),
            np.array(c, np.int32).reshape(G, MAX_ZONES))


def _rows(a, m: int) -> np.ndarray:
    """A copy of `a` as int64 [nres][m]; with m == 0 reshape(-1, 0) could not tell nres."""
    a = np.array(a, np.int64)
    return a.reshape(-1, m) if m else a.reshape(len(a), 0)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone=None, group=None,
            max_skew=(), mode=NONE, weight=0, rw=(), bits=None, n_classes=0, pod_class=None, A=None, T=None, w_aff=0,
            w_taint=0, modes=None, w_spread=0, w_balanced=0, state=None, pod_profile=None, counts=None, cnt=None,
            prefs_trace=None, soft_trace=None):
    """`state` (a PA.State) is updated in place."""
    n, p = len(unsched), len(pod_digit)
    alloc, us, req = _rows(alloc, n), _rows(used, n), _rows(req, p)
    nres, G = alloc.shape[0], len(max_skew)
    assert not w_balanced or nres >= 2
    if mode != NONE or w_balanced:
        assert max(alloc.max(initial=0), us.max(initial=0), req.max(initial=0)) <= SCORE_MAX, "int64 would overflow"
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
    prf = np.full(p, -1, np.int64) if pod_profile is None else np.asarray(pod_profile, np.int64)
    Q = 0 if state is None else len(state.match)
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
    if state is not None:
        pz, rz, anyw = state.derived(zone)
    for j in range(p):
        pd = int(pod_digit[j])
        g = int(grp[j]) if 0 <= grp[j] < G else -1
        k = int(cls[j]) if 0 <= cls[j] < n_classes else -1
        q = int(prf[j]) if 0 <= prf[j] < Q else -1
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
                feas = feas & zoned & (c[g][zsafe] - c[g][zs].min() < sk[g])   # the minimum over Zset, not narrowed
        first = False
        if q >= 0:
            ok, first, AF = PA.conjunct(state, q, zn, zoned, zsafe, pz, rz, anyw, feas)
            feas = feas & ok
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
                qq = us[r] + req[r, j]
                part = (alloc[r] - qq) if mode == LEAST else qq
                none = (alloc[r] == 0) | (qq > alloc[r])
                acc += np.where(none, 0, np.where(none, 0, part) * 100 // safe[r]) * rw[r]
            total = total + (acc // den) * np.int64(O._wrap64(int(weight)))
        ra = Aq[k] if k >= 0 else zeros
        rt = Tq[k] if k >= 0 else zeros
        max_a, max_t = int(ra[feas].max()), int(rt[feas].max())
        if prefs_trace is not None:
            prefs_trace.append((k, max_a, max_t))
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
                rzz = r.astype(np.int64)
                mx, mn = int(rzz[in_zs].max()), int(rzz[in_zs].min())
                nz = np.full(MAX_ZONES, 100, np.int64) if mx == 0 else 100 * (mx + mn - rzz) // max(mx, 1)
                total = total + np.int64(int(w_spread)) * np.where(zoned, nz[zsafe], 0)
            if soft_trace is not None:
                soft_trace.append((j, size, mn, mx))
        if w_balanced:
            total = total + np.int64(int(w_balanced)) * BR.bs_nodes(alloc, us, req[:, j])
        sel = int(np.argmax(np.where(feas, total, lowest)))  # argmax returns the first maximum
        idx[j], score[j] = sel, total[sel]
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0 and zn[sel] >= 0:  # a hard group's pod always lands in a zone
            c[g, zn[sel]] += 1
        if q >= 0:
            M, AA = state.match[q], state.anti[q]
            if first and AF and not ((state.present[sel] & state.HM) | (pz[zn[sel]] & state.ZM if zn[sel] >= 0 else 0)) & AF:
                state.stats["first_pod"] += 1
            state.present[sel] |= M
            state.repel[sel] |= AA
            if zn[sel] >= 0:
                pz[zn[sel]] |= M
                rz[zn[sel]] |= AA
                anyw |= M & state.ZM
            anyw |= M & state.HM
    return idx, score, status, count.astype(np.int32), us, c.astype(np.int32)
