"""CPU references for sequential-commit mode with a per-node capacity column (include/minisched_hip.h,
"Per-node pod capacity"). Two of them, neither the code under test; test infrastructure only.

1. `via_oracle`: the existing C oracle, unchanged. A node of capacity c_i holding k_i pods decides exactly
   like a node under the uniform capacity M = max(c) that already holds M - c_i + k_i pods, so
   oracle.c_schedule_sequential(..., max_pods=M, counts=M - cap + k) gives the expected outputs and its
   returned counts minus (M - cap) the expected counts. (M is at least 1: the oracle reads 0 as "no
   capacity".) For caps far below 2^31 only: M + k must stay within int32.
2. `serial`: a plain loop in Python that evaluates every (pod, node) pair per pod with oracle.normalize and
   oracle._wrap64. For tiny shapes, and for INT32_MAX capacities.
"""
from __future__ import annotations

import numpy as np

INT32_MAX = 2**31 - 1
PLACED, FIT_ERROR, SCORE_ERROR = 0, 1, 2


def effective(cap, scalar: int = 0) -> np.ndarray:
    """eff[i] = cap[i], or min(cap[i], scalar) for a positive max_pods_per_node."""
    cap = np.asarray(cap, np.int64)
    return np.minimum(cap, scalar) if scalar > 0 else cap.copy()


def via_oracle(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, counts=None):
    """(idx, score, status, counts after) through the uniform-capacity identity."""
    eff = np.asarray(eff, np.int64)
    n = len(eff)
    k = np.zeros(n, np.int64) if counts is None else np.asarray(counts, np.int64)
    m = max(1, int(eff.max())) if n else 1
    assert m + int(k.max(initial=0)) + len(pod_digit) <= INT32_MAX, "the identity needs int32 head-room"
    shifted = np.zeros(max(n, 1), np.int32)
    shifted[:n] = m - eff + k
    idx, score, status, after = O.c_schedule_sequential(unsched, node_digit, pod_digit, pod_tol, plugins,
                                                        max_pods=m, counts=shifted)
    return idx, score, status, (after.astype(np.int64) - (m - eff)).astype(np.int32)


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, counts=None):
    """(idx, score, status, counts after): one pod at a time, every node looked at for every pod."""
    n, p = len(unsched), len(pod_digit)
    eff = [int(x) for x in eff]
    cnt = [0] * n if counts is None else [int(x) for x in counts]
    has_nu = "NodeUnschedulable" in plugins.filters
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score)
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    for j in range(p):
        pd, tol = int(pod_digit[j]), bool(pod_tol[j])
        feas = [i for i in range(n) if (not has_nu or not unsched[i] or tol) and cnt[i] < eff[i]]
        if not feas:
            status[j] = FIT_ERROR
            continue
        if plugins.score and not (nn_pre and 0 <= pd <= 9):  # NodeNumber.Score finds no PreScore state
            status[j] = SCORE_ERROR
            continue
        total = [0] * len(feas)
        for w, mode in zip(plugins.weights, plugins.normalize):
            raw = [10 if 0 <= int(node_digit[i]) == pd else 0 for i in feas]
            total = [O._wrap64(t + s * int(w)) for t, s in zip(total, O.normalize(int(mode), raw))]
        best = max(total)
        sel = feas[total.index(best)]  # the first maximum in List order
        idx[j], score[j] = sel, best
        cnt[sel] += 1
    return idx, score, status, np.array(cnt, np.int32)
