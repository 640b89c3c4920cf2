"""CPU references for resource-aware scoring in sequential-commit mode (include/minisched_hip.h, "Resource-aware
scoring": msh_set_resource_score with LEAST_ALLOCATED / MOST_ALLOCATED). Neither is the code under test; test
infrastructure only.

The contract, per pod in order: the feasible list is resource_fit_ref.serial's; a feasible node's total is the
header's formula (NodeNumber normalized over the feasible list, plus weight x RS with q = used + req before the
commit); the first maximum in List order wins; the commit is resource_fit_ref's. Mode NONE leaves NodeNumber alone.

`serial` (Python ints, tiny shapes) and `per_pod` (numpy int64, mid sizes) are seq_ref's two loops with every later
feature left absent; `resource_score` and `_nn_scores` are the helpers those loops use, the first in `serial` only and
the second (NodeNumber's normalizers spelled out on arrays) in `per_pod` only. tests/test_resource_score.py checks the
two against each other and mode NONE against resource_fit_ref.serial, which shares no code with them.

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
    import seq_ref
    return seq_ref.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, mode=mode,
                          weight=weight, rw=rw, counts=counts)[:5]


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
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, mode=mode,
                           weight=weight, rw=rw, counts=counts)[:5]


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
