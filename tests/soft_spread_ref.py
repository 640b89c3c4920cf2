"""CPU references for sequential-commit mode with the soft topology spread score (include/minisched_hip.h, "Soft
topology spread": msh_schedule_sequential_soft). Neither is the code under test; test infrastructure only.

The contract, per pod j in order. A pod that is ungrouped or whose group's mode is DO_NOT_SCHEDULE is decided as
prefs_ref decides it. A pod of a SCHEDULE_ANYWAY group g passes no spread filter: its feasible set F is the one of an
ungrouped pod of its class. With Zs the zones of the zoned nodes in F and size = |Zs|:
    raw_z = round_half_away(float(cnt[g][z]) * log(size + 2) + float(max_skew[g] - 1))   for z in Zs
            (a product and a sum, each rounded once: two double operations)
    mx, mn = max, min of raw_z over Zs
    ns_i = 100 if mx == 0 else 100 * (mx + mn - raw_zone[i]) // mx   for i in F with a zone, 0 for i in F without one
    total_i = prefs_ref's total_i + w_spread * ns_i
and the first maximum in List order wins. A placed pod of a soft group adds 1 to cnt[g][zone[sel]] only if sel has a
zone.

`serial` and `per_pod` are seq_ref's two loops with every later feature left absent. The first works in Python ints
and floats through `raw_score` (math.log, rounding by floor and a comparison; tiny shapes); the second, one pod at a
time with the nodes in numpy, takes the weights from `weights` and rounds with numpy's rint, the ties it sends down
put back up.

Arguments are prefs_ref.serial's up to w_taint, then (modes, w_spread): modes one 0 / 1 per group (None: all 0). Both
return (idx, score, status, counts after, used after, cnt after). With `trace` a list, every soft pod that reaches
scoring appends (j, size, mn, mx) (mn = mx = None with Zs empty). `gen_case` is the seeded generator of the GPU sweep;
tests/test_soft_spread.py checks on the references alone that it reaches what the sweep is for.
"""
from __future__ import annotations

import math

import numpy as np

import prefs_ref as PR
import resource_score_ref as RS
import spread_ref as S

NONE, LEAST, MOST = RS.NONE, RS.LEAST, RS.MOST
PLACED, FIT_ERROR, SCORE_ERROR = S.PLACED, S.FIT_ERROR, S.SCORE_ERROR
MAX_ZONES = S.MAX_ZONES
DO_NOT_SCHEDULE, SCHEDULE_ANYWAY = 0, 1
SOFT_MAX = 1 << 24

# log(size + 2) for size = 0..64. The library's table (msh_spread_soft_weight) is its own std::log;
# tests/test_soft_spread.py checks that the two agree bit for bit.
weights = [math.log(k + 2) for k in range(MAX_ZONES + 1)]


def round_half_away(y: float) -> int:
    """Go's math.Round for y >= 0: y - floor(y) is exact."""
    f = math.floor(y)
    return f + (1 if y - f >= 0.5 else 0)


def raw_score(c: int, size: int, skew: int) -> int:
    x = float(c) * math.log(size + 2)   # rounded once
    return round_half_away(x + float(skew - 1))   # and once more


def serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
           mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, counts=None, cnt=None,
           trace=None):
    import seq_ref
    return seq_ref.serial(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                          max_skew, mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread,
                          counts=counts, cnt=cnt, soft_trace=trace)


def per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group, max_skew,
            mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread, counts=None, cnt=None,
            trace=None):
    import seq_ref
    return seq_ref.per_pod(O, unsched, node_digit, pod_digit, pod_tol, plugins, eff, alloc, used, req, zone, group,
                           max_skew, mode, weight, rw, bits, n_classes, pod_class, A, T, w_aff, w_taint, modes, w_spread,
                           counts=counts, cnt=cnt, soft_trace=trace)


def gen_case(seed: int, max_n: int = 700, max_p: int = 300) -> dict:
    """One case of the random sweep: prefs_ref.gen_case's table, groups, amounts, plugins, classes and preference
    values (its resource score mode by seed: NONE every third, else LEAST / MOST by parity), about half of the groups
    SCHEDULE_ANYWAY, skews 1..3 (1: the first pod of a group sees mx == 0; above 1: mn > 0), a spread weight in
    [1, 100] and the resource weight lowered so that the key holds the sum. By seed % 5:
      0: most nodes lose their zone and the zoned ones take one pod each, so that Zs runs empty mid-call and soft pods
         land on nodes without a zone;
      1: every group is soft;  2: pods of three kinds only in a table of 8 zones whose small zones fill (size < |Zset|);
      others: as drawn."""
    c = PR.gen_case(seed, max_n, max_p)
    rng = np.random.default_rng(3 * 10**6 + seed)
    n, G = c["n"], c["G"]
    modes = (rng.random(G) < 0.5).astype(np.uint8)
    kind = seed % 5
    zone = np.array(c["zone"], np.int32)
    cap = np.array(c["cap"], np.int64)
    if kind == 0:
        zone[rng.random(n) < 0.7] = -1
        cap[zone >= 0] = 1
        modes[0] = 1
    elif kind == 1:
        modes[:] = 1
    elif kind == 2:
        zone = rng.choice(8, n, p=np.array([40, 30, 15, 8, 3, 2, 1, 1]) / 100).astype(np.int32)
        cap[:] = 1
        modes[: max(1, G // 2)] = 1
    w_spread = int(rng.integers(1, 101))
    c["rs_weight"] = int(min(int(c["rs_weight"]), 655 - c["w_aff"] - c["w_taint"] - w_spread))
    c.update(zone=zone, cap=cap, modes=modes, w_spread=w_spread)
    return c
