"""Quotient-boundary cases for generic_kernel's normalizing columns, shared by tests/test_generic_exact.py (CPU: the
restatement below and its mutants) and tests/test_generic_exact_gpu.py (schedule_batch against the oracle). Test
infrastructure only.

A case is one normalizing column X (ScoreColumn0; DEFAULT, REVERSE or MIN-MAX, weight w) whose raws sit on the quotient
boundaries of its divisor, and NONE columns that cancel X's expected normalized score on every node (ScoreColumn1 at
weight w; for the large negative quotients also ScoreColumn2 at weight w * 2^20), so every expected total of a pod
that does not tolerate the unschedulable taint is the same (0, or a ballast column's constant) and its first feasible
node wins. The listed nodes come first and
are cordoned one per step, so each takes its turn as first feasible; behind them sit the keepers, copies of the nodes
that define the extents, always schedulable. A quotient that is 1 too large anywhere, or 1 too small at the head, moves
some pod's node or score. Only the winner is visible per pod, which is why the construction is needed.

Node layout: [pad fillers, unschedulable throughout] [listed, L nodes] [keepers] [one unschedulable node holding a
positive maximum: the cases whose two tolerate classes must see different extents].
"""
from __future__ import annotations

import numpy as np

NONE, DEFAULT, REVERSE, MINMAX = 0, 1, 2, 3
P = 130                                     # two 64-pod blocks and a ragged third, both tolerate classes in each
DIVISORS = [1, 3, 7, 100, (1 << 31) - 1, 1 << 31]
LO = -(1 << 31)
SPLIT = 1 << 20
# weight of X per key width (a score weight is at most 2^32): 32-bit keys (the host's bound on |total|, 200 w, below
# 2^31), doubles (below 2^53), uint64_t by weight (past 2^53: the same weight and a ballast column, one more NONE
# column at weight 2^32 that holds 2^22 on every node and so adds the same 2^54 to every total), uint64_t forced
BALLAST_W, BALLAST = 1 << 32, 1 << 22
WIDTHS = {"k32": (3, "auto"), "f53": (1 << 32, "auto"), "u64w": (1 << 32, "auto"), "u64f": (1 << 32, "u64")}
# raws down to -101 (a score bound of 10,100 per unit of weight); the cases with quotients near -2^37.6 carry a second
# cancelling column at w * 2^20: smaller weights
WIDTHS_SMALL = {"k32": (3, "auto"), "f53": (1 << 30, "auto"), "u64w": (1 << 30, "auto"), "u64f": (1 << 30, "u64")}
WIDTHS_NEG = {"k32": (3, "auto"), "f53": (1 << 10, "auto"), "u64w": (1 << 10, "auto"), "u64f": (1 << 10, "u64")}

def go_div(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def normalize(mode: int, raws: list[int]) -> list[int]:
    """helper.DefaultNormalizeScore(100, reverse) and min-max over the feasible nodes' raws, in Go's int64 division."""
    mx, mn = max(raws), min(raws)
    if mode == DEFAULT:
        m = max(mx, 0)
        return list(raws) if m == 0 else [go_div(100 * r, m) for r in raws]
    if mode == REVERSE:
        m = max(mx, 0)
        return [100] * len(raws) if m == 0 else [100 - go_div(100 * r, m) for r in raws]
    if mode == MINMAX:
        return [0] * len(raws) if mx == mn else [go_div((r - mn) * 100, mx - mn) for r in raws]
    return list(raws)


def boundary_raws(lo: int, span: int) -> list[int]:
    """For each k in 0..100 the smallest raw whose quotient 100 * (raw - lo) / span reaches k, and the one below."""
    out = set()
    for k in range(101):
        b = -((-k * span) // 100)
        out.update(x + lo for x in (b - 1, b) if 0 <= x <= span)
    return sorted(out)


def make(name, mode, listed, keepers, widths, width, pad=0, hidden=None):
    w, keys = widths[width]
    raws = [0] * pad + list(listed) + list(keepers) + ([hidden] if hidden is not None else [])
    n = len(raws)
    uns = np.zeros(n, np.uint8)
    uns[:pad] = 1
    if hidden is not None:
        uns[n - 1] = 1
    c = dict(name=f"{name}-{width}", mode=mode, w=w, keys=keys, raws=raws, n=n, pad=pad, L=len(listed), unsched=uns,
             same_extents=hidden is None, ballast=BALLAST if width == "u64w" else 0)
    # the cancelling columns, from the expected normalized scores of the class that does not tolerate the taint;
    # an unschedulable node's is taken over all nodes (only the tolerating class sees it)
    feas = [i for i in range(n) if not uns[i]]
    norm = dict(zip(feas, normalize(mode, [raws[i] for i in feas])))
    allnorm = normalize(mode, raws)
    c1, c2 = [], []
    for i in range(n):
        neg = -norm.get(i, allnorm[i])
        hi = go_div(neg, SPLIT)
        c1.append(neg - hi * SPLIT)
        c2.append(hi)
    c["c1"], c["c2"] = c1, c2
    c["two"] = any(c2)
    assert max(map(abs, raws + c1 + c2)) <= 1 << 31       # what a score column may hold
    # the key width the host picks (generic_args in msh_capi.cpp: its bound on a feasible |total|) is the one meant
    bound, c24 = host_bound(c)
    if width == "k32":
        assert c24 and bound <= (1 << 31) - 2, c["name"]
    elif width == "u64w":
        assert bound > (1 << 53) - 2, c["name"]
    else:
        assert (not c24 or bound > (1 << 31) - 2) and bound <= (1 << 53) - 2, c["name"]
    return c


def host_bound(c):
    """The host's bound on |total| and whether every normalizing term is a 24-bit product (32-bit keys need both)."""
    lo, hi = min(c["raws"]), max(c["raws"])
    if c["mode"] == DEFAULT:
        sb = 100 if lo >= 0 else max(100, 100 * -lo)
    elif c["mode"] == REVERSE:
        sb = 100 if lo >= 0 else 100 + 100 * -lo
    else:
        sb = 100
    bound = c["w"] * sb + c["w"] * max(map(abs, c["c1"]))
    if c["two"]:
        bound += c["w"] * SPLIT * max(map(abs, c["c2"]))
    bound += BALLAST_W * c["ballast"]
    return bound, c["w"] < (1 << 23) and sb < (1 << 23)


def cases():
    out = []
    for mode, tag in ((DEFAULT, "default"), (REVERSE, "reverse"), (MINMAX, "minmax")):
        spans = [(0, m) for m in DIVISORS] + ([(LO, (1 << 32) - 1)] if mode == MINMAX else [])
        for lo, m in spans:
            keep = [lo + m] + ([lo] if mode == MINMAX else [])
            for width in WIDTHS:
                out.append(make(f"{tag}-{m}", mode, boundary_raws(lo, m), keep, WIDTHS, width))
    # one case past an LDS tile boundary (2,560 nodes of 32-bit keys, 1,706 of 8-byte ones): the listed nodes straddle it
    for width in WIDTHS:
        pad = 2500 if width == "k32" else 1650
        out.append(make("default-100-tiles", DEFAULT, boundary_raws(0, 100), [100], WIDTHS, width, pad=pad))
    # negative raws under DEFAULT beside the boundaries of m = 1 and m = 3: quotients down to -100 * 2^31 (/ 3)
    for m in (1, 3):
        neg = [LO, LO + 1, LO + 2, -4, -3, -2, -1]
        for width in ("f53", "u64w", "u64f"):
            out.append(make(f"default-{m}-negative", DEFAULT, neg + boundary_raws(0, m), [m], WIDTHS_NEG, width))
    # a feasible maximum of 0 and a negative one (DefaultNormalizeScore's maxCount stays 0: DEFAULT leaves the raws,
    # REVERSE gives 100); with the negative one a positive maximum hides on an unschedulable node, so the tolerating
    # class divides by 7 where the other one does not divide
    small = [-101, -100, -7, -3, -2]
    for mode, tag in ((DEFAULT, "default"), (REVERSE, "reverse")):
        for big in (False, True):
            ws = ("f53", "u64w", "u64f") if big else tuple(WIDTHS)
            lst = ([LO, LO + 1] if big else []) + small
            sz = "big" if big else "small"
            wt = WIDTHS_NEG if big else WIDTHS_SMALL
            for width in ws:
                out.append(make(f"{tag}-max0-{sz}", mode, lst + [-1, 0], [0], wt, width))
                out.append(make(f"{tag}-maxneg-{sz}", mode, lst + [-1], [-1], wt, width, hidden=7))
    return out


def plugin_list(c):
    """(name, weight, normalize) per score plugin."""
    pl = [("ScoreColumn0", c["w"], c["mode"]), ("ScoreColumn1", c["w"], NONE)]
    if c["two"]:
        pl.append(("ScoreColumn2", c["w"] * SPLIT, NONE))
    if c["ballast"]:
        pl.append((f"ScoreColumn{len(pl)}", BALLAST_W, NONE))
    assert all(1 <= w <= 1 << 32 for _, w, _ in pl)
    return pl


def columns(c):
    cols = {0: np.array(c["raws"], np.int64), 1: np.array(c["c1"], np.int64), 2: np.array(c["c2"], np.int64),
            3: np.zeros(c["n"], np.int64)}
    if c["ballast"]:
        cols[3 if c["two"] else 2] = np.full(c["n"], c["ballast"], np.int64)
    return cols


def base_total(c) -> int:
    """The total every node of the non-tolerating class is expected to have: 0, or the ballast's."""
    return BALLAST_W * c["ballast"]


def unsched_at(c, t: int) -> np.ndarray:
    """Step t: the first t listed nodes are cordoned."""
    u = c["unsched"].copy()
    u[c["pad"]:c["pad"] + t] = 1
    return u


def pods():
    pd = (np.arange(P) % 10).astype(np.int8)
    pt = ((np.arange(P) % 3) == 0).astype(np.uint8)
    return pd, pt


def outcome(c, t: int, tol: bool, mutate=None):
    """The expected (node, total) of a pod at step t, in Python integers. mutate = (node, s): that pair's quotient is
    off by s (for the class whose quotient the case lists: both, or the non-tolerating one where the extents differ)."""
    u = unsched_at(c, t)
    feas = [i for i in range(c["n"]) if tol or not u[i]]
    norm = normalize(c["mode"], [c["raws"][i] for i in feas])
    if mutate is not None and (c["same_extents"] or not tol) and mutate[0] in feas:
        norm[feas.index(mutate[0])] += -mutate[1] if c["mode"] == REVERSE else mutate[1]
    w = c["w"]
    best, at = None, -1
    for i, s in zip(feas, norm):
        tot = w * s + w * c["c1"][i] + w * SPLIT * c["c2"][i] + base_total(c)
        assert abs(tot) < 1 << 62
        if best is None or tot > best:
            best, at = tot, i
    return at, best
