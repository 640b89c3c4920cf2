"""CPU references for sequential-commit mode with pod topology spread (include/minisched_hip.h, "Pod topology
spread for sequential-commit mode"). None of them is the code under test; test infrastructure only.

The contract, per pod j in order, with group g = group[j] (anything outside [0, G) counts as -1): node i is
feasible iff the filter list passes, count[i] < eff[i], every positive request fits alloc - used, and, for g >= 0,
zone[i] >= 0 and cnt[g][zone[i]] + 1 - min over z in Zset of cnt[g][z] <= max_skew[g]. Zset is the set of zone ids
on at least one node. Status, NodeNumber totals in every normalize mode, the first maximum and the commit are the
resource-fit form's; a PLACED grouped pod also adds 1 to cnt[g][zone[sel]].

`serial` (a plain Python loop that reads cnt[g][zone[i]] for every node, for tiny shapes: p * n <= 2 * 10^5) and
`per_pod` (one pod at a time with the nodes in numpy, the skew of every node gathered from the cnt array) are
seq_ref's two loops with no score beyond NodeNumber and every later feature left absent. tests/test_spread.py shows
`per_pod` equal to `serial`, and both equal to resource_fit_ref and node_capacity_ref on ungrouped pods, before
anything relies on them.

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
    import seq_ref
    return seq_ref.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                          max_skew, counts=counts, cnt=cnt)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            counts=None, cnt=None):
    """(idx, score, status, counts after, used after, cnt after): per pod one numpy pass over the nodes."""
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                           max_skew, counts=counts, cnt=cnt)


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
