"""NodeResourcesBalancedAllocation in sequential-commit mode, the parts that need no GPU: the new symbols, the two CPU
references of tests/balanced_ref.py against each other and (with w_balanced = 0) against soft_spread_ref, hand-worked
values of the rule, the search for the inputs that tell the float64 rule from its near misses (the decider triples the
GPU tests place on nodes), what the GPU sweep's generator has to reach, and the wrappers' argument checks."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import balanced_ref as BR
import node_capacity_ref as CR
import soft_spread_ref as SR
from test_classes import case_plugins, same

NEW_SYMBOLS = ["msh_set_balanced_score", "msh_balanced_score", "msh_seq_balanced_max_nodes",
               "msh_schedule_sequential_balanced", "msh_schedule_sequential_balanced_device"]
SWEEP_SEEDS = range(44000, 44040)


def run(ref, oracle, c, w_balanced=None, **kw):
    return ref(oracle, c["unsched"], c["node_digit"], c["pod_digit"], c["pod_tol"], case_plugins(oracle, c),
               CR.effective(c["cap"]), c["alloc"], c.get("used", np.zeros_like(c["alloc"])), c["req"], c["zone"],
               c["group"], c["max_skew"], c["score_mode"], c["rs_weight"], c["rw"], c["bits"], c["C"], c["pod_class"],
               c["A"], c["T"], c["w_aff"], c["w_taint"], c["modes"], c["w_spread"],
               c["w_balanced"] if w_balanced is None else w_balanced, **kw)


def test_new_symbols_are_declared_exported_and_bound(msh):
    header = (Path(__file__).resolve().parent.parent / "include" / "minisched_hip.h").read_text()
    N = msh._native
    lib = N.lib()
    for nm in NEW_SYMBOLS:
        assert re.search(r"^int " + nm + r"\(", header, re.M), f"{nm} is not declared in the header"
        assert nm in N.EXPORTED and hasattr(lib, nm) and nm in N._SIGS, nm
    sigs = N._SIGS
    assert len(sigs["msh_schedule_sequential_balanced"][1]) == len(sigs["msh_schedule_sequential_soft"][1])
    assert len(sigs["msh_schedule_sequential_balanced_device"][1]) == len(sigs["msh_schedule_sequential_soft_device"][1])
    inv = N.MSH_ERR_INVALID
    assert lib.msh_set_balanced_score(None, 1) == inv
    assert lib.msh_balanced_score(None, None) == inv
    assert lib.msh_seq_balanced_max_nodes(None, 0, None) == inv
    assert lib.msh_schedule_sequential_balanced(None, 0, None, None, None, None, 0, None, 0, None, None, None,
                                                N.COMMIT_CB(), None) == inv
    assert lib.msh_schedule_sequential_balanced_device(None, 0, None, None, None, None, 0, None, 0, None, None, None,
                                                       None) == inv
    for nm in ("set_balanced_score", "balanced_score", "seq_balanced_max_nodes", "schedule_sequential_balanced",
               "schedule_sequential_balanced_device"):
        assert callable(getattr(msh.DeviceContext, nm)), nm


def test_scheduler_argument_checks(msh):
    """Before any device work: the weight's range, and resources with at least two names."""
    for bad in (-1, 101, True, 1.0):
        with pytest.raises(ValueError):
            msh.Scheduler(resources=("cpu", "memory"), balanced_allocation_weight=bad)
    with pytest.raises(ValueError):
        msh.Scheduler(balanced_allocation_weight=1)
    with pytest.raises(ValueError):
        msh.Scheduler(resources=("cpu",), balanced_allocation_weight=1)


@pytest.mark.parametrize("q0,c0,q1,c1,want,why", [
    (0, 1, 4, 5, 19, "1 - 0.8 is 0.19999999999999996 in float64: 19, where the exact value is 20"),
    (0, 1, 3, 5, 40, "1 - 0.6 is exactly 0.4 in float64: 40, where float32 gives 39"),
    (7, 0, 1, 2, 50, "a resource without capacity counts as full: f = 1"),
    (0, 0, 0, 7, 0, "... also with nothing requested of it: 1 against 0"),
    (9, 4, 1, 2, 50, "q > c after a lowered alloc: the fraction is clamped to 1"),
    (3, 7, 6, 14, 100, "equal fractions: 100"),
    (1 << 40, 1 << 41, 5, 10, 100, "equal fractions in different units"),
    (0, 5, 5, 5, 0, "one at 0 and one at 1: 0"),
    (5, 5, 0, 5, 0, "and the other way round"),
    (1, 3, 2, 3, 66, "1/3 against 2/3: 66.66... truncates to 66"),
])
def test_hand_worked_values(q0, c0, q1, c1, want, why):
    assert BR.bs(q0, c0, q1, c1) == want, why
    al = np.array([[c0], [c1]], np.int64)
    assert BR.bs_nodes(al, np.array([[q0], [q1]], np.int64), [0, 0])[0] == want, why
    assert BR.bs_nodes(al, np.zeros((2, 1), np.int64), [q0, q1])[0] == want, why


def test_the_near_misses_of_the_hand_worked_values():
    assert BR.bs_exact(0, 1, 4, 5) == 20 and BR.bs(0, 1, 4, 5) == 19
    assert BR.bs_f32(0, 1, 3, 5) == 39 and BR.bs(0, 1, 3, 5) == 40
    assert BR.bs_rounded(1, 3, 2, 3) == 67 and BR.bs(1, 3, 2, 3) == 66


# amounts near 2^55 where the int64 -> double conversion rounds (ties to even, up and down), and fractions of them
BIG = [(1 << 55) - 1, (1 << 55) - 3, (1 << 54) + 1, (1 << 54) + 3, (1 << 53) + 1, (1 << 53) + 3, (1 << 55) - (1 << 2) - 1,
       3 * (1 << 53) + 5, (1 << 55)]


def big_quads():
    """(q0, c0, q1, c1) with q <= c <= 2^55 from BIG and its thirds and fifths."""
    vals = sorted(set(BIG) | {b // 3 for b in BIG} | {b // 5 * 2 + 1 for b in BIG})
    rng = np.random.default_rng(55)
    out = []
    while len(out) < 48:
        a, b, c, d = (int(vals[k]) for k in rng.integers(0, len(vals), 4))
        out.append((min(a, b), max(a, b), min(c, d), max(c, d)))
    return out


def decider_triples(limit: int = 12, per_kind: int = 16):
    """The small inputs on which the rule differs from a near miss, as (kind, (q0, c0, q1, c1), rule's value, the
    near miss's value): kind "exact" (the exact rational floor), "f32" (the float32 evaluation), "rounded" (round to
    nearest instead of truncation). The first per_kind of each in the search order, which starts from the small
    capacities; and a robust input for every value that occurs: one on which all four evaluations agree."""
    found = {"exact": [], "f32": [], "rounded": []}
    robust = {}
    near = {"exact": BR.bs_exact, "f32": BR.bs_f32, "rounded": BR.bs_rounded}
    for c0 in range(1, limit + 1):
        for c1 in range(1, limit + 1):
            for q0 in range(c0 + 1):
                for q1 in range(c1 + 1):
                    quad = (q0, c0, q1, c1)
                    v = BR.bs(*quad)
                    others = {k: f(*quad) for k, f in near.items()}
                    if all(o == v for o in others.values()):
                        robust.setdefault(v, quad)
                    for k, o in others.items():
                        if o != v and len(found[k]) < per_kind:
                            found[k].append((k, quad, v, o))
    triples = found["exact"] + found["f32"] + found["rounded"]
    # a value with no robust input among the small ones (10: every small way to 0.9 is a decider itself): 0 against
    # q / c with larger capacities
    for v in sorted({max(v, o) for _, _, v, o in triples} - set(robust)):
        robust[v] = next(quad for c1 in range(13, 400) for q1 in range(c1 + 1) for quad in [(0, 1, q1, c1)]
                         if BR.bs(*quad) == v and all(f(*quad) == v for f in near.values()))
    return triples, robust


def test_decider_triples_exist_and_have_comparators():
    """Each near miss is told from the rule by some small input, and for each such input a robust node with the
    larger of the two values exists: the GPU test pairs them so that the pick itself differs."""
    triples, robust = decider_triples()
    kinds = {k for k, *_ in triples}
    assert kinds == {"exact", "f32", "rounded"}
    assert len(triples) == 48
    for k, quad, v, o in triples:
        assert v != o and 0 <= v <= 100
        assert max(v, o) in robust, (k, quad, v, o)
    assert ("exact", (0, 1, 4, 5), 19, 20) in triples


def test_conversions_round_near_two_to_the_55():
    """The big amounts are no doubles, so float(q) rounds; the two references agree on them, and on some of them
    Python's int / int (the exact ratio rounded once) is another double than float(q) / float(c)."""
    assert all(float(b) != b or b == 1 << 55 for b in BIG) and max(BIG) == BR.SCORE_MAX
    assert float((1 << 53) + 1) == float(1 << 53) and float((1 << 53) + 3) == float((1 << 53) + 4)   # ties to even
    quads = big_quads()
    differ = 0
    for q0, c0, q1, c1 in quads:
        al = np.array([[c0], [c1]], np.int64)
        assert BR.bs_nodes(al, np.array([[q0], [q1]], np.int64), [0, 0])[0] == BR.bs(q0, c0, q1, c1)
        differ += (q0 / c0 != float(q0) / float(c0)) or (q1 / c1 != float(q1) / float(c1))
    assert differ > 0


def test_with_weight_zero_the_reference_is_soft_spread_ref(oracle):
    for seed in range(200):
        c = BR.gen_case(50000 + seed, max_n=40, max_p=60)
        cols = (c["unsched"], c["node_digit"], c["pod_digit"], c["pod_tol"])
        want = SR.serial(oracle, *cols, case_plugins(oracle, c), CR.effective(c["cap"]), c["alloc"], c["used"], c["req"],
                         c["zone"], c["group"], c["max_skew"], c["score_mode"], c["rs_weight"], c["rw"], c["bits"],
                         c["C"], c["pod_class"], c["A"], c["T"], c["w_aff"], c["w_taint"], c["modes"], c["w_spread"])
        same(run(BR.serial, oracle, c, w_balanced=0), want, f"seed {seed}, serial")
        if seed < 40:
            same(run(BR.per_pod, oracle, c, w_balanced=0), want, f"seed {seed}, per_pod")


def test_the_two_references_agree(oracle):
    for seed in range(60):
        c = BR.gen_case(51000 + seed, max_n=65, max_p=80)
        same(run(BR.per_pod, oracle, c), run(BR.serial, oracle, c), f"seed {seed}")


def test_the_sweep_generator_reaches_what_the_sweep_is_for(oracle):
    """In at least half of the sweep's cases some pod lands on another node than with w_balanced = 0; the cases cover
    2, 3 and 4 resources, the three resource score modes, capacities of 0, clamped fractions and pods without requests."""
    moved = 0
    nres, modes, zero_cap, clamped, no_req = set(), set(), 0, 0, 0
    for seed in SWEEP_SEEDS:
        c = BR.gen_case(seed)
        a = run(BR.per_pod, oracle, c)
        b = run(BR.per_pod, oracle, c, w_balanced=0)
        moved += not np.array_equal(a[0], b[0])
        nres.add(c["nres"])
        modes.add(c["score_mode"])
        zero_cap += bool((c["alloc"][:2] == 0).any())
        clamped += bool((a[4][:2] > c["alloc"][:2]).any() or (c["used"][:2] > c["alloc"][:2]).any())
        no_req += bool((c["req"].sum(axis=0) == 0).any())
    n = len(SWEEP_SEEDS)
    assert n == 40 and moved >= n // 2, moved
    assert nres == {2, 3, 4} and modes == {BR.NONE, BR.LEAST, BR.MOST}
    assert zero_cap >= n // 4 and clamped >= n // 4 and no_req >= n // 2, (zero_cap, clamped, no_req)
