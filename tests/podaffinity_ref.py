"""CPU reference for the required inter-pod affinity and anti-affinity filter in sequential-commit mode
(include/minisched_hip.h, "Required inter-pod affinity": msh_schedule_sequential_podaffinity). Not the code under test;
test infrastructure only.

The contract: balanced_ref.per_pod's, with one more conjunct of the feasible set. A ctx holds T terms, each with a
topology (0: the node itself, 1: the node's zone), and Q profiles (match, anti, aff). The state is two words per node,
present[i] and repel[i]. For a pod of profile q >= 0 with M = match[q], AA = anti[q], AF = 1 << aff[q] (0 without an
affinity term) and node i,
    P_i = (present[i] & HM) | (presentZ[zone[i]] & ZM if zone[i] >= 0 else 0)      R_i likewise from repel
    presentZ[z] = OR of present over the nodes of zone z,  any = OR of (present & HM) over all nodes
                                                                 | OR of (present & ZM) over the zoned nodes
node i passes when (P_i & AA) == 0 (own anti), (R_i & M) == 0 (symmetric anti) and, with AF != 0, the node has the
term's topology key and (P_i & AF) != 0 or the first-pod exception holds, (any & AF) == 0 and (M & AF) != 0. A placed
pod ORs M into present[sel] and AA into repel[sel]. A pod of profile -1 reads and writes none of it.

`State` carries present / repel between calls; `per_pod` is balanced_ref.per_pod's loop, node-vectorised in numpy, with
the conjunct, and counts why nodes were rejected and how often the exception admitted a pod (`stats`): a node is
counted under the first of own anti, symmetric anti, missing topology key, affinity that rejects it, among the nodes
the other filters left. `gen_case` is the seeded generator of the GPU tests."""
from __future__ import annotations

import numpy as np

import balanced_ref as BR
import resource_score_ref as RS
import soft_spread_ref as SR

NONE, LEAST, MOST = BR.NONE, BR.LEAST, BR.MOST
PLACED, FIT_ERROR, SCORE_ERROR = BR.PLACED, BR.FIT_ERROR, BR.SCORE_ERROR
MAX_ZONES = BR.MAX_ZONES
SCHEDULE_ANYWAY = BR.SCHEDULE_ANYWAY
HOSTNAME, ZONE = 0, 1
MAX_TERMS, MAX_PROFILES = 32, 64
COUNTERS = ("own_anti", "symmetric_anti", "no_topology_key", "affinity", "first_pod")


class State:
    """The terms, the profiles and the two words per node."""

    def __init__(self, n: int, topo, match=(), anti=(), aff=(), present=None, repel=None):
        self.topo = [int(t) for t in topo]
        assert len(self.topo) <= MAX_TERMS and all(t in (HOSTNAME, ZONE) for t in self.topo)
        self.HM = sum(1 << t for t, k in enumerate(self.topo) if k == HOSTNAME)
        self.ZM = sum(1 << t for t, k in enumerate(self.topo) if k == ZONE)
        self.set_profiles(match, anti, aff)
        self.present = np.zeros(n, np.int64) if present is None else np.array(present, np.int64)
        self.repel = np.zeros(n, np.int64) if repel is None else np.array(repel, np.int64)
        self.stats = dict.fromkeys(COUNTERS, 0)

    def set_profiles(self, match, anti, aff):
        T = len(self.topo)
        self.match, self.anti, self.aff = [int(x) for x in match], [int(x) for x in anti], [int(x) for x in aff]
        assert len(self.match) == len(self.anti) == len(self.aff) <= MAX_PROFILES
        assert all(x >> T == 0 for x in self.match + self.anti) and all(-1 <= x < T for x in self.aff)

    def copy(self) -> "State":
        s = State(len(self.present), self.topo, self.match, self.anti, self.aff, self.present, self.repel)
        s.stats = dict(self.stats)
        return s

    def derived(self, zone):
        """presentZ, repelZ ([MAX_ZONES] each) and `any` for a zone column (None: no node has a zone)."""
        pz, rz = np.zeros(MAX_ZONES, np.int64), np.zeros(MAX_ZONES, np.int64)
        anyw = int(np.bitwise_or.reduce(self.present & self.HM)) if len(self.present) else 0
        if zone is not None:
            zn = np.asarray(zone, np.int64)
            for z in np.unique(zn[zn >= 0]):
                pz[z] = np.bitwise_or.reduce(self.present[zn == z])
                rz[z] = np.bitwise_or.reduce(self.repel[zn == z])
            anyw |= int(np.bitwise_or.reduce(pz)) & self.ZM
        return pz, rz, anyw


def conjunct(st: State, q: int, zn, zoned, zsafe, pz, rz, anyw, others=None):
    """The nodes that pass for a pod of profile q (bool [n]); with `others` (the nodes the other filters left) the
    reasons are counted into st.stats."""
    M, AA = st.match[q], st.anti[q]
    AF = 1 << st.aff[q] if st.aff[q] >= 0 else 0
    P = (st.present & st.HM) | np.where(zoned, pz[zsafe] & st.ZM, 0)
    R = (st.repel & st.HM) | np.where(zoned, rz[zsafe] & st.ZM, 0)
    own = (P & AA) != 0
    sym = (R & M) != 0
    ok = ~own & ~sym
    nokey = np.zeros(len(P), bool)
    noaff = np.zeros(len(P), bool)
    first = False
    if AF:
        nokey = ~zoned if AF & st.ZM else nokey
        first = (anyw & AF) == 0 and (M & AF) != 0
        noaff = ((P & AF) == 0) & (not first)
        ok = ok & ~nokey & ~noaff
    if others is not None:
        left = others.copy()
        for name, rej in (("own_anti", own), ("symmetric_anti", sym), ("no_topology_key", nokey), ("affinity", noaff)):
            st.stats[name] += int((left & rej).sum())
            left &= ~rej
    return ok, first, AF


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, w_balanced,
            state: State, pod_profile, counts=None, cnt=None):
    """balanced_ref.per_pod with the conjunct; `state` is updated in place. pod_profile None: no pod has a profile.
    Returns balanced_ref.per_pod's tuple."""
    n, p = len(unsched), len(pod_digit)
    alloc = np.asarray(alloc, np.int64).reshape(-1, n)
    us = np.array(used, np.int64).reshape(-1, n)
    req = np.asarray(req, np.int64).reshape(-1, p)
    nres, G = alloc.shape[0], len(max_skew)
    assert not w_balanced or nres >= 2
    if mode != NONE or w_balanced:
        assert max(alloc.max(initial=0), us.max(initial=0), req.max(initial=0)) <= BR.SCORE_MAX
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
    Q = len(state.match)
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
            ok, first, AF = conjunct(state, q, zn, zoned, zsafe, pz, rz, anyw, feas)
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
                y = c[g].astype(np.float64) * wt[size]
                y = y + np.float64(int(sk[g]) - 1)
                r = np.rint(y)
                r = r + ((y - np.floor(y) == 0.5) & (r < y))
                rzz = r.astype(np.int64)
                mx, mn = int(rzz[in_zs].max()), int(rzz[in_zs].min())
                nz = np.full(MAX_ZONES, 100, np.int64) if mx == 0 else 100 * (mx + mn - rzz) // max(mx, 1)
                total = total + np.int64(int(w_spread)) * np.where(zoned, nz[zsafe], 0)
        if w_balanced:
            total = total + np.int64(int(w_balanced)) * BR.bs_nodes(alloc, us, req[:, j])
        sel = int(np.argmax(np.where(feas, total, lowest)))
        idx[j], score[j] = sel, total[sel]
        count[sel] += 1
        us[:, sel] += req[:, j]
        if g >= 0 and zn[sel] >= 0:
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


def gen_case(seed: int, n: int, p: int, nres: int, T: int, n_zones: int = 6) -> dict:
    """A table of n nodes (a tenth without a zone), T terms of both topologies (T = 1: the topology is seed's parity)
    and profiles of four kinds: replicas that repel their own kind (anti on a term they match), victims that match a
    term others repel and have no anti of their own, self-affine series (aff on a term they match), and followers
    (aff on a term they do not match); with T > 1 all 64 profiles exist and the pods use eight of them. Two in five
    pods have no profile. Amounts are balanced_ref's uneven ones."""
    rng = np.random.default_rng(9 * 10**6 + seed)
    topo = [seed & 1] if T == 1 else [int(x) for x in rng.integers(0, 2, T)]
    if T > 1:
        topo[0], topo[1] = HOSTNAME, ZONE
    Q = min(MAX_PROFILES, 4 * T) if T > 1 else 4
    match, anti, aff = [], [], []
    for q in range(Q):
        t = (q // 2) % T if T > 1 else 0
        kind = q % 4
        o = (t + 1) % T
        if kind == 0:    # a replica: one per domain of term t
            match.append(1 << t), anti.append(1 << t), aff.append(-1)
        elif kind == 1:  # a victim of the replicas of term t, with nothing of its own
            match.append(1 << t), anti.append(0), aff.append(-1)
        elif kind == 2:  # a self-affine series on term o
            match.append(1 << o), anti.append(0), aff.append(o)
        else:            # a follower of term t that does not match it, and repels the series of o
            match.append(0), anti.append((1 << o) if o != t else 0), aff.append(t)
    zone = rng.integers(0, n_zones, n).astype(np.int32)
    zone[rng.random(n) < 0.1] = -1
    prof = rng.choice(rng.choice(Q, min(Q, 8), replace=False), p).astype(np.int32)  # eight profiles share the pods
    prof[rng.random(p) < 0.4] = -1
    alloc = rng.integers(40, 400, (nres, n)) if nres else np.zeros((0, n), np.int64)
    used = (rng.random((nres, n)) < 0.3) * rng.integers(0, 40, (nres, n)) if nres else np.zeros((0, n), np.int64)
    req = rng.integers(0, 5, (nres, p)) if nres else np.zeros((0, p), np.int64)
    return dict(n=n, p=p, nres=nres, topo=topo, match=match, anti=anti, aff=aff, zone=zone, profile=prof,
                alloc=np.asarray(alloc, np.int64), used=np.asarray(used, np.int64), req=np.asarray(req, np.int64),
                unsched=(rng.random(n) < 0.1).astype(np.uint8), node_digit=rng.integers(-1, 10, n).astype(np.int8),
                pod_digit=rng.integers(0, 10, p).astype(np.int8), pod_tol=(rng.random(p) < 0.5).astype(np.uint8),
                cap=rng.integers(1, 4, n).astype(np.int64))
