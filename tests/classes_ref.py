"""CPU references for sequential-commit mode with per-class node masks (include/minisched_hip.h, "Static node
filters: per-class node masks": msh_schedule_sequential_classes). Neither is the code under test; test
infrastructure only.

The contract, per pod j in order, with group g = group[j] (anything outside [0, G) counts as -1) and class
c = pod_class[j] (anything outside [0, C) counts as -1): node i is feasible iff it is feasible for
msh_schedule_sequential_spread_scored (filter list, count[i] < eff[i], every positive request fits, and for g >= 0 a
zone and cnt[g][zone[i]] + 1 - min over Zset of cnt[g] <= max_skew[g]) and, for c >= 0, bit c of bits[i] is set.
Status, NodeNumber's normalizer extents, the resource score (modes LEAST / MOST; NONE: NodeNumber alone), the first
maximum in List order and the commit are taken over that set; a class does not change what a commit writes, and the
spread minimum stays over Zset.

`serial` (a plain Python loop over pods, nodes and resources in Python ints, tiny shapes) and `per_pod` (one pod at a
time with the nodes in numpy int64) are seq_ref's two loops with every later feature left absent.
Neither forms an availability mask or packs keys: a node's verdict is read from bits[i] >> c & 1 directly.

Arguments are spread_score_ref.serial's up to rw, then (bits, n_classes, pod_class); zone, group and pod_class may be
None (no node has a zone, no pod a group, no pod a class). Both return (idx, score, status, counts after, used after,
cnt after). `gen_case` is the seeded generator of the random sweeps.
"""
from __future__ import annotations

import numpy as np

import resource_score_ref as RS
import spread_ref as S
import spread_score_ref as X

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES
MAX_CLASSES = 64


def clean_classes(pod_class, n_classes: int, p: int) -> list[int]:
    if pod_class is None:
        return [-1] * p
    return [int(c) if 0 <= int(c) < n_classes else -1 for c in pod_class]


def _column(bits, n: int):
    """Here an absent column admits no node to any class (from prefs_ref on it admits every node)."""
    return np.zeros(n, np.uint64) if bits is None else bits


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           mode, weight, rw, bits, n_classes, pod_class, counts=None, cnt=None):
    import seq_ref
    return seq_ref.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                          max_skew, mode, weight, rw, _column(bits, len(unsched)), n_classes, pod_class, counts=counts,
                          cnt=cnt)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, counts=None, cnt=None):
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                           max_skew, mode, weight, rw, _column(bits, len(unsched)), n_classes, pod_class, counts=counts,
                           cnt=cnt)


DENSITIES = ("none", "one", "tenth", "half", "all")


def gen_bits(rng, n: int, n_classes: int):
    """One word per node for n_classes classes, each class of a density drawn from DENSITIES; returns (bits, the
    density names by class)."""
    bits = np.zeros(n, np.uint64)
    kinds = []
    for c in range(n_classes):
        kind = DENSITIES[int(rng.integers(0, len(DENSITIES)))]
        kinds.append(kind)
        if kind == "none":
            m = np.zeros(n, bool)
        elif kind == "one":
            m = np.zeros(n, bool)
            m[int(rng.integers(0, n))] = True
        elif kind == "all":
            m = np.ones(n, bool)
        else:
            m = rng.random(n) < (0.1 if kind == "tenth" else 0.5)
        bits |= m.astype(np.uint64) << np.uint64(c)
    return bits, kinds


def gen_case(seed: int, max_n: int = 2048, max_p: int = 2000) -> dict:
    """One case of the random sweep: spread_score_ref.gen_case's table, groups, amounts and plugins (its odd and even
    seeds give LEAST and MOST; every third seed here runs unscored) with 1..64 classes of densities drawn from
    {admits none, exactly one node, ~10%, ~50%, all} and about a fifth of the pods without a class."""
    c = X.gen_case(seed, max_n, max_p)
    rng = np.random.default_rng(10**6 + seed)
    C = int(rng.choice([1, 2, 5, 16, 33, 64]))
    bits, kinds = gen_bits(rng, c["n"], C)
    pod_class = rng.integers(0, C, c["p"]).astype(np.int32)
    pod_class[rng.random(c["p"]) < 0.2] = -1
    if seed % 3 == 0:
        c["score_mode"] = NONE
    c.update(C=C, bits=bits, kinds=kinds, pod_class=pod_class)
    return c
