"""CPU references for sequential-commit mode with pod topology spread and a resource score together
(include/minisched_hip.h, "Topology spread together with a resource score": msh_schedule_sequential_spread_scored).
Neither is the code under test; test infrastructure only.

The contract, per pod j in order, with group g = group[j] (anything outside [0, G) counts as -1): the feasible set
and the status are spread_ref's (filter list, count[i] < eff[i], every positive request fits, and for g >= 0 a zone
and cnt[g][zone[i]] + 1 - min over Zset of cnt[g] <= max_skew[g]); a feasible node's total is resource_score_ref's
(NodeNumber normalized over the feasible list, plus weight x RS with q = used + req before the commit); the pod
goes to the first maximum in List order; a PLACED pod adds 1 to count[sel], its requests to used[:, sel] and, for
g >= 0, 1 to cnt[g][zone[sel]].

`serial` (Python ints, the header's formulas, tiny shapes) and `per_pod` (one pod at a time with the nodes in numpy
int64) are seq_ref's two loops with every later feature left absent.
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
    import seq_ref
    return seq_ref.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                          max_skew, mode, weight, rw, counts=counts, cnt=cnt)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, counts=None, cnt=None):
    if mode == NONE:
        return S.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                         max_skew, counts, cnt)
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                           max_skew, mode, weight, rw, counts=counts, cnt=cnt)


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
