"""CPU reference of MSH_TIEBREAK_RANDOM (include/minisched_hip.h, "tie-break among the maximum totals").

Every (pod, node) pair is evaluated directly: feasibility, raw score, NormalizeScore, weight, total; the
tie set is `total == max` over the feasible nodes and the pod goes to its k-th element. Nothing here
knows about matches and non-matches as classes, so it checks the kernel's case analysis instead of
repeating it. numpy, one row per distinct pod input; test infrastructure only.
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
_GOLDEN, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def draw64(seed: int, counter: int) -> int:
    """SplitMix64 at position `counter` of the stream seeded with `seed` (all 64 bits)."""
    z = (seed + (counter + 1) * _GOLDEN) & M64
    z = ((z ^ (z >> 30)) * _M1) & M64
    z = ((z ^ (z >> 27)) * _M2) & M64
    return z ^ (z >> 31)


def draw(seed: int, counter: int) -> int:
    """The tie-break's u: the high 32 bits."""
    return draw64(seed, counter) >> 32


def draws(seed: int, base: int, p: int) -> np.ndarray:
    """u for counters base .. base + p - 1, as uint64 (values below 2^32)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + (np.uint64(base & M64) + np.arange(1, p + 1, dtype=np.uint64)) * np.uint64(_GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def _trunc_div(a, b):
    q = np.abs(a) // np.abs(b)
    return np.where((a >= 0) == (b >= 0), q, -q)


def pick(unsched, node_digit, pod_digit, pod_tol, plugins, seed: int, base: int, block: int = 256):
    """(idx int32, score int64, status int32) of a batch in RANDOM mode. `plugins` has the fields of
    oracle.PluginSet (filters, prescore, score, weights, normalize); score-column plugins are not covered."""
    unsched = np.asarray(unsched).astype(bool)
    node_digit = np.asarray(node_digit).astype(np.int64)
    pod_digit = np.asarray(pod_digit).astype(np.int64)
    pod_tol = np.asarray(pod_tol).astype(bool)
    n, p = len(unsched), len(pod_digit)
    has_nu = "NodeUnschedulable" in plugins.filters
    nn_pre = "NodeNumber" in plugins.prescore
    assert all(s == "NodeNumber" for s in plugins.score), "score columns are outside the random tie-break"
    idx = np.full(p, -1, np.int32)
    score = np.zeros(p, np.int64)
    status = np.zeros(p, np.int32)
    u = draws(seed, base, p)
    # pods with the same (digit, tolerates) inputs have the same totals: each distinct pod is evaluated
    # once against every node (memoisation, not a case analysis), then every pod takes its own k
    keys, inverse = np.unique(np.stack([pod_digit, pod_tol.astype(np.int64)], axis=1), axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for lo in range(0, len(keys) if p else 0, block):
        hi = min(lo + block, len(keys))
        pd, pt = keys[lo:hi, 0], keys[lo:hi, 1].astype(bool)
        m = hi - lo
        feas = (~unsched[None, :] | pt[:, None]) if has_nu else np.ones((m, n), bool)
        anyf = feas.any(axis=1)
        st = np.where(anyf, 0, 1)
        if plugins.score:  # NodeNumber.Score without its PreScore state: the pod errors (nodenumber.go:74-77)
            st = np.where(anyf & ((not nn_pre) | (pd < 0) | (pd > 9)), 2, st)
        total = np.zeros((m, n), np.int64)
        imin, imax = np.iinfo(np.int64).min, np.iinfo(np.int64).max
        with np.errstate(over="ignore"):
            for _name, w, mode in zip(plugins.score, plugins.weights, plugins.normalize):
                raw = np.where(node_digit[None, :] == pd[:, None], 10, 0).astype(np.int64)
                hi_ = np.where(feas, raw, imin).max(axis=1, initial=imin)[:, None]
                lo_ = np.where(feas, raw, imax).min(axis=1, initial=imax)[:, None]
                if mode in (1, 2):  # DefaultNormalizeScore(100, reverse) over the feasible list
                    mx = np.maximum(hi_, 0)
                    sc = _trunc_div(100 * raw, np.maximum(mx, 1))
                    raw = np.where(mx == 0, raw if mode == 1 else 100, sc if mode == 1 else 100 - sc)
                elif mode == 3:  # min-max over the feasible list
                    raw = np.where(hi_ == lo_, 0, _trunc_div((raw - lo_) * 100, np.where(hi_ == lo_, 1, hi_ - lo_)))
                total = total + raw * np.int64(w)
        best = np.where(feas, total, imin).max(axis=1, initial=imin)
        tie = feas & (total == best[:, None])
        for r in range(m):
            members = np.flatnonzero(inverse == lo + r)
            status[members] = st[r]
            if st[r] != 0:
                continue
            pos = np.flatnonzero(tie[r])  # the tie set, List order
            k = (u[members] * np.uint64(len(pos))) >> np.uint64(32)
            idx[members] = pos[k.astype(np.int64)]
            score[members] = best[r]
    return idx, score, status
