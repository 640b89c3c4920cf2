"""The one-flag cases prove their own coverage, on the CPU: for every table of
pair_one_flag_cases, the oracle places the targeted pods on the intended node above group 0 and every
other pod with a digit inside group 0 (tests/test_pair_lds_one_flag_gpu.py asserts the same before
each GPU call)."""
from __future__ import annotations

import numpy as np
import pytest

import pair_one_flag_cases as C


def _want(oracle, case, pd, pt, w=3, norm=1):
    ps = oracle.PluginSet(filters=["NodeUnschedulable"], prescore=["NodeNumber"], score=["NodeNumber"],
                          weights=[w], normalize=[norm])
    return oracle.c_schedule_batch(case.u, case.nd, pd, pt, ps)


@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: c.name)
def test_case_coverage(oracle, case):
    for p in C.PODS:
        pd, pt = C.pods(p)
        want = _want(oracle, case, pd, pt)
        hit = C.check_coverage(case, pd, pt, want[0], want[2])
        assert (hit > 0) == bool(case.above)


def test_shard_case_goes_past_its_own_group0(oracle):
    """In the second shard alone (its node_base is the cut) the targeted pods resolve above its group 0."""
    case, cut = C.shard_case()
    pd, pt = C.pods(513)
    want = _want(oracle, case, pd, pt)
    assert C.check_coverage(case, pd, pt, want[0], want[2], base=cut) > 0
    local = C.Case("shard 1", case.u[cut:], case.nd[cut:],
                   {k: v - cut for k, v in case.expect.items() if k in case.above}, case.above)
    lw = _want(oracle, local, pd, pt)
    for kind in case.above:
        sel = (pd == kind[0]) & (pt == kind[1])
        assert sel.any() and (lw[0][sel] == local.expect[kind]).all() and local.expect[kind] >= C.G


def test_pods_mix_every_kind_in_one_block():
    pd, pt = C.pods(64)
    kinds = {(int(d), int(t)) for d, t in zip(pd, pt)}
    for d in (7, 8, 9, 3, -1):
        assert (d, 0) in kinds and (d, 1) in kinds
    pd1, pt1 = C.pods(1)
    assert (int(pd1[0]), int(pt1[0])) == (7, 0)


def test_tables_have_the_stated_groups():
    groups = sorted({-(-len(c.u) // C.G) for c in C.above_cases()})
    assert groups == [2, 3, 5, 20]
    assert -(-len(C.big_case().u) // C.G) == 129 and len(C.big_case().u) == 33_024
    assert any(len(c.u) < C.G for c in C.group0_cases())
    firsts = {c.expect[(7, 0)] for c in C.group0_cases() if len(c.u) == 600}
    assert firsts == {0, 31, 32, 127, 128, 255}
