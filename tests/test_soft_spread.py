"""Soft topology spread (whenUnsatisfiable: ScheduleAnyway) in sequential-commit mode, the parts that need no GPU:
the two CPU references of tests/soft_spread_ref.py against each other and against prefs_ref, hand-worked placements,
the library's weight table against math.log, the search for a (count, size, skew) triple that a fused multiply-add
would round differently, what the GPU sweep's generator has to reach, the wrappers' argument checks and
constraints.spread_mode."""
from __future__ import annotations

import ctypes as C
import math
import re
import struct
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import node_capacity_ref as CR
import prefs_ref as PR
import soft_spread_ref as SR
import spread_ref as S
from test_classes import case_args, case_plugins, same

NEW_SYMBOLS = ["msh_set_spread_group_modes", "msh_get_spread_group_modes", "msh_set_spread_score_weight",
               "msh_spread_score_weight", "msh_spread_soft_weight", "msh_seq_soft_max_nodes",
               "msh_schedule_sequential_soft", "msh_schedule_sequential_soft_device"]
SWEEP_SEEDS = range(33000, 33060)
MODES = (SR.NONE, SR.LEAST, SR.MOST)


def run(ref, oracle, c, modes=None, w_spread=None, trace=None):
    cols, eff, res, sp, sc = case_args(c)
    return ref(oracle, *cols, case_plugins(oracle, c), eff, *res, *sp, *sc, c["bits"], c["C"], c["pod_class"],
               c["A"], c["T"], c["w_aff"], c["w_taint"], c["modes"] if modes is None else modes,
               c["w_spread"] if w_spread is None else w_spread, trace=trace)


def run_prefs(ref, oracle, c):
    cols, eff, res, sp, sc = case_args(c)
    return ref(oracle, *cols, case_plugins(oracle, c), eff, *res, *sp, *sc, c["bits"], c["C"], c["pod_class"],
               c["A"], c["T"], c["w_aff"], c["w_taint"])


def test_new_symbols_are_declared_exported_and_bound(msh):
    header = (Path(__file__).resolve().parent.parent / "include" / "minisched_hip.h").read_text()
    N = msh._native
    lib = N.lib()
    for nm in NEW_SYMBOLS:
        assert re.search(r"^int " + nm + r"\(", header, re.M), f"{nm} is not declared in the header"
        assert nm in N.EXPORTED and hasattr(lib, nm) and nm in N._SIGS, nm
    sigs = N._SIGS
    assert len(sigs["msh_schedule_sequential_soft"][1]) == len(sigs["msh_schedule_sequential_prefs"][1])
    assert len(sigs["msh_schedule_sequential_soft_device"][1]) == len(sigs["msh_schedule_sequential_prefs_device"][1])
    for name, value in (("MSH_SPREAD_DO_NOT_SCHEDULE", "0"), ("MSH_SPREAD_SCHEDULE_ANYWAY", "1"),
                        ("MSH_SPREAD_SOFT_MAX", "(1 << 24)")):
        assert f"#define {name} {value}" in header
    assert (N.SPREAD_DO_NOT_SCHEDULE, N.SPREAD_SCHEDULE_ANYWAY, N.SPREAD_SOFT_MAX) == (0, 1, 1 << 24) \
        and SR.SOFT_MAX == N.SPREAD_SOFT_MAX
    inv = N.MSH_ERR_INVALID
    assert lib.msh_set_spread_group_modes(None, 0, None) == inv
    assert lib.msh_get_spread_group_modes(None, None, None) == inv
    assert lib.msh_set_spread_score_weight(None, 1) == inv
    assert lib.msh_spread_score_weight(None, None) == inv
    assert lib.msh_seq_soft_max_nodes(None, 0, None) == inv
    assert lib.msh_schedule_sequential_soft(None, 0, None, None, None, None, 0, None, 0, None, None, None,
                                            N.COMMIT_CB(), None) == inv
    assert lib.msh_schedule_sequential_soft_device(None, 0, None, None, None, None, 0, None, 0, None, None, None, None) == inv
    for nm in ("set_spread_group_modes", "spread_group_modes", "set_spread_score_weight", "spread_score_weight",
               "seq_soft_max_nodes", "schedule_sequential_soft", "schedule_sequential_soft_device"):
        assert callable(getattr(msh.DeviceContext, nm)), nm


def test_the_weight_table_is_math_log_bit_for_bit(msh):
    """msh_spread_soft_weight(size) is the library's std::log(size + 2); the references use math.log. On this
    platform the two are the same bits for every size, so the references need not read the table through the getter."""
    lib = msh._native.lib()
    out = C.c_double()
    for size in range(65):
        assert lib.msh_spread_soft_weight(size, C.byref(out)) == msh._native.MSH_OK
        assert struct.pack("<d", out.value) == struct.pack("<d", math.log(size + 2)) == struct.pack("<d", SR.weights[size])
    for bad in (-1, 65):
        assert lib.msh_spread_soft_weight(bad, C.byref(out)) == msh._native.MSH_ERR_INVALID
    assert lib.msh_spread_soft_weight(3, None) == msh._native.MSH_ERR_INVALID


def test_per_pod_equals_serial_on_150_seeds(oracle):
    soft_scored = 0
    modes = set()
    for seed in range(150):
        c = SR.gen_case(seed, max_n=40, max_p=60)
        trace = []
        a = run(SR.serial, oracle, c, trace=trace)
        tb = []
        b = run(SR.per_pod, oracle, c, trace=tb)
        same(a, b, f"seed {seed}")
        assert trace == tb, f"seed {seed}: Zs, mn or mx differ"
        soft_scored += len(trace)
        modes.add(c["score_mode"])
    assert modes == set(MODES) and soft_scored > 1500


def test_without_a_soft_group_the_references_are_prefs_ref(oracle):
    for seed in range(60):
        c = SR.gen_case(seed, max_n=40, max_p=60)
        want = run_prefs(PR.serial, oracle, c)
        for w in (0, 1, 100):
            same(run(SR.serial, oracle, c, np.zeros(c["G"], np.uint8), w), want, f"serial, seed {seed}, w {w}")
            same(run(SR.per_pod, oracle, c, np.zeros(c["G"], np.int32), w), want, f"per_pod, seed {seed}, w {w}")


def tiny(oracle, zone, cap, p, skew=1, cnt=None, w_spread=1, modes=(1,), ref=SR.serial, trace=None):
    """Plain nodes without digits, p pods of group 0 and no class, NodeNumber out of the score list, no resources: the
    spread term alone (plus w_taint * 100 = 0 with the weights 0)."""
    n = len(zone)
    ps = oracle.PluginSet(score=[], weights=[], normalize=[])
    a, us, rq = S.no_res(n, p)
    return ref(oracle, np.zeros(n, np.uint8), np.full(n, -1, np.int8), np.zeros(p, np.int8), np.ones(p, np.uint8), ps,
               CR.effective(np.asarray(cap, np.int64)), a, us, rq, np.asarray(zone, np.int32), np.zeros(p, np.int32),
               [skew], SR.NONE, 0, [], None, 0, None, None, None, 0, 0, modes, w_spread, cnt=cnt, trace=trace)


@pytest.mark.parametrize("ref", [SR.serial, SR.per_pod])
def test_hand_worked_two_zones(oracle, ref):
    """Nodes 0, 1 in zone 0, node 2 in zone 1, node 3 without a zone, capacities (2, 1, 2, 5); max_skew 1, so
    raw = Round(cnt * log(size + 2)), log 4 = 1.386 with both zones feasible.
    Pod 0: counts (0, 0): raw (0, 0), mx = 0: ns = 100 on the zoned nodes, 0 on node 3: node 0 at 100.
    Pod 1: counts (1, 0): raw (1, 0), mx = 1, mn = 0: ns = (100 * (1 + 0 - 1) / 1, 100 * 1 / 1) = (0, 100): node 2.
    Pod 2: counts (1, 1): raw (1, 1): ns = 100 * (1 + 1 - 1) / 1 = 100 in both: node 0, which is then full.
    Pod 3: counts (2, 1): raw (Round(2.77) = 3, 1): ns = (100 * 1 / 3 = 33, 100 * 3 / 3 = 100): node 2, then full.
    Pod 4: nodes 1 and 3 are left, Zs = {0}: size 1, raw = Round(2 * log 3 = 2.197) = 2 = mx = mn:
           ns = 100 * (2 + 2 - 2) / 2 = 100: node 1.
    Pod 5: node 3 alone: Zs is empty, ns = 0, and no zone's count moves."""
    tr = []
    out = tiny(oracle, [0, 0, 1, -1], [2, 1, 2, 5], 6, ref=ref, trace=tr)
    assert out[0].tolist() == [0, 2, 0, 2, 1, 3]
    assert out[1].tolist() == [100, 100, 100, 100, 100, 0]
    assert out[5][0].tolist()[:2] == [3, 2] and out[5].sum() == 5
    assert tr == [(0, 2, 0, 0), (1, 2, 0, 1), (2, 2, 1, 1), (3, 2, 1, 3), (4, 1, 2, 2), (5, 0, None, None)]


@pytest.mark.parametrize("ref", [SR.serial, SR.per_pod])
def test_hand_worked_skew_and_ignored_nodes(oracle, ref):
    """max_skew 3 adds 2 to every raw value: counts (4, 0) over two zones give raw (Round(4 * 1.386 + 2) = 8, 2):
    ns = (100 * (8 + 2 - 8) / 8 = 25, 100 * 8 / 8 = 100). The node without a zone scores 0 and still wins when the
    zoned nodes are full: a soft pod is never a FIT_ERROR for its zone."""
    cnt = np.zeros((1, S.MAX_ZONES), np.int32)
    cnt[0, 0] = 4
    out = tiny(oracle, [0, 1, -1], [1, 1, 1], 4, skew=3, cnt=cnt, w_spread=7, ref=ref)
    assert out[0].tolist() == [1, 0, 2, -1] and out[1].tolist() == [700, 700, 0, 0]
    assert out[2].tolist() == [SR.PLACED] * 3 + [SR.FIT_ERROR]
    assert out[5][0, :2].tolist() == [5, 1]
    hard = tiny(oracle, [0, 1, -1], [1, 1, 1], 4, skew=3, cnt=cnt, w_spread=7, modes=(0,), ref=ref)
    # the filter instead: zone 0 is 4 ahead of zone 1, above max_skew 3, until zone 1 holds 2: FIT_ERRORs
    assert hard[0].tolist() == [1, -1, -1, -1]


def test_round_half_away():
    assert [SR.round_half_away(x) for x in (0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 2.4999999999999996)] == [0, 0, 1, 2, 3, 2]
    y = np.array([0.5, 1.5, 2.5, 3.5, 0.49999999999999994, 7.0])
    r = np.rint(y)
    assert (r + ((y - np.floor(y) == 0.5) & (r < y))).tolist() == [1, 2, 3, 4, 0, 7]


def test_no_count_below_2_pow_20_is_rounded_differently_by_a_fused_multiply_add():
    """c in [0, 2^20), size in 1..64, skew in 1..4: y = fl(fl(c * w) + (skew - 1)) against the fused fl(c * w + (skew -
    1)) (exact rational arithmetic, rounded once). The two doubles differ by at most 2^-29 here (y < 2^23), so their
    integer roundings can differ only when y is within 2^-28 of a half; every such triple is checked exactly. None
    exists in this range (DESIGN.md records it), so the GPU suite carries no such case; the kernel's two-step
    evaluation is checked by its assembly (profiles/soft_spread_regs.json)."""
    c = np.arange(1 << 20, dtype=np.float64)
    found, checked = [], 0
    for size in range(1, 65):
        w = math.log(size + 2)
        x = c * w
        for skew in range(1, 5):
            y = x + float(skew - 1)
            for ci in np.flatnonzero(np.abs(y - np.floor(y) - 0.5) <= 2.0 ** -28):
                checked += 1
                fused = float(Fraction(int(ci)) * Fraction(w) + (skew - 1))
                if SR.round_half_away(float(y[ci])) != SR.round_half_away(fused):
                    found.append((int(ci), size, skew))
    assert found == [], f"put {found[0]} into tests/test_soft_spread_gpu.py as a patched count ({checked} candidates)"


def test_the_sweep_generator_reaches_what_the_sweep_is_for(oracle):
    """Per resource score mode, over SWEEP_SEEDS: soft pods with size < |Zset|, with mn > 0, with mx == 0, with Zs
    empty, one placed on a node without a zone, one whose selection differs from the w_spread = 0 run, and a call that
    mixes pods of hard groups, of soft groups and of none."""
    names = ("size < |Zset|", "mn > 0", "mx == 0", "Zs empty", "on a node without a zone", "differs from w_spread 0",
             "hard, soft and ungrouped")
    seen = {m: set() for m in MODES}
    for seed in SWEEP_SEEDS:
        c = SR.gen_case(seed)
        assert c["n"] <= 700 and c["p"] <= 300
        wres = c["rs_weight"] if c["score_mode"] != SR.NONE else 0
        assert 0 <= 100 * (wres + c["w_aff"] + c["w_taint"] + c["w_spread"]) <= 65534 and wres >= 0
        trace = []
        a = run(SR.per_pod, oracle, c, trace=trace)
        b = run(SR.per_pod, oracle, c, w_spread=0)
        got = seen[c["score_mode"]]
        nzset = len(set(c["zone"][c["zone"] >= 0].tolist()))
        md, grp = c["modes"], c["group"]
        soft_pod = (grp >= 0) & (md[np.clip(grp, 0, None)] == 1)
        for j, size, mn, mx in trace:
            if 0 < size < nzset:
                got.add(names[0])
            if size and mn > 0:
                got.add(names[1])
            if size and mx == 0:
                got.add(names[2])
            if size == 0:
                got.add(names[3])
            if a[0][j] >= 0 and c["zone"][a[0][j]] < 0:
                got.add(names[4])
        if (a[0][soft_pod] != b[0][soft_pod]).any():
            got.add(names[5])
        if soft_pod.any() and ((grp >= 0) & ~soft_pod).any() and (grp < 0).any():
            got.add(names[6])
    for m in MODES:
        assert seen[m] == set(names), (m, set(names) - seen[m])


def test_wrapper_validation(msh):
    d = msh.DeviceContext.__new__(msh.DeviceContext)  # the checks below run before any library call
    for bad in ([[0, 1]], [0.5], [-1], [256]):
        with pytest.raises(ValueError):
            msh.DeviceContext.set_spread_group_modes(d, bad)
    with pytest.raises(ValueError):
        msh.DeviceContext.schedule_sequential_soft(d, np.zeros(3, np.int8), np.zeros(2, np.uint8))


@pytest.mark.parametrize("constraints,want", [
    (None, None),
    ([], None),
    ([{"maxSkew": 1, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule"}], 0),
    ([{"maxSkew": 2, "topologyKey": "zone", "whenUnsatisfiable": "ScheduleAnyway"}], 1),
    ([{"maxSkew": 2, "topologyKey": "zone"}], 0),                                        # the API's default
    ([{"maxSkew": 1, "topologyKey": "host", "whenUnsatisfiable": "ScheduleAnyway"},
      {"maxSkew": 1, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule"}], 0),   # the zone key's constraint
    ([{"maxSkew": 1, "topologyKey": "host", "whenUnsatisfiable": "ScheduleAnyway"}], None),
])
def test_spread_mode(msh, constraints, want):
    pod = {"metadata": {"name": "p"}, "spec": {}}
    if constraints is not None:
        pod["spec"]["topologySpreadConstraints"] = constraints
    assert msh.constraints.spread_mode(pod, "zone") == want
    with pytest.raises(ValueError):
        msh.constraints.spread_mode({"spec": {"topologySpreadConstraints": [
            {"maxSkew": 1, "topologyKey": "zone", "whenUnsatisfiable": "Sometimes"}]}}, "zone")
