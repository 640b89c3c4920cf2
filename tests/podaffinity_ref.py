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

`State` carries present / repel between calls; `per_pod` is seq_ref.per_pod, the loop of every layer node-vectorised in
numpy, which applies `conjunct` to the nodes the other filters left and commits into the state. `conjunct` counts why
nodes were rejected, and the loop how often the exception admitted a pod (`stats`): a node is counted under the first of
own anti, symmetric anti, missing topology key, affinity that rejects it, among the nodes the other filters left. `gen_case` is the seeded generator of the GPU tests."""
from __future__ import annotations

import numpy as np

import balanced_ref as BR

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
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                           max_skew, mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread,
                           w_balanced, state, pod_profile, counts=counts, cnt=cnt)


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
